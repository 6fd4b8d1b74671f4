"""CPU: the edge inputs of tests/cql_edge_cases.py are what they claim to be, so tests/test_gpu_cql_edges.py can compare every
tensor without excluding anything: ties are bit-exact in float32, overflow really would happen without the maximum, the
clamp cases sit at / outside their bounds, and the largest entry of every gradient compared relatively is non-zero."""
import numpy as np
import pytest

from tests import cql_edge_cases as EC


def _values(c):
    """The three float32 values per row and critic as the kernel forms them: [2, 3, B R]."""
    off = np.float32(np.log(0.5 ** c["A"]))
    return np.stack([c["q_rand"] - off, c["q_cur"] - c["logp_cur"][None], c["q_next"] - c["logp_next"][None]], axis=1).astype(np.float32)


@pytest.mark.parametrize("A,B,R", EC.SHAPES)
def test_edge_inputs(A, B, R):
    for kind in EC.KINDS:
        c = EC.make(kind, A, B, R)
        ref = EC.reference(c)
        assert np.all(np.isfinite(ref["loss9"])), kind
        assert np.abs(ref["d_data"]).max() > 0, kind
        if kind in EC.ZERO_REP_GRAD:
            assert np.all(ref["d_rep"] == 0.0), kind
        else:
            assert np.abs(ref["d_rep"]).max() > 0, kind
        v = _values(c)
        rep = (lambda x: np.repeat(x, R)) if c["calib"] is not None else None
        if kind == "big_values":
            z = v / np.float32(c["cfg"]["temperature"])
            assert z.max() > 390 and z.min() < -390 and z.max() > np.log(np.finfo(np.float32).max)
            assert np.all(v > rep(c["calib"])[None, None])
        if kind == "all_equal":
            assert np.all(v[:, 1] == v[:, 2]) and np.abs(v[:, 0] - v[:, 1]).max() <= 1e-6
            g = ref["d_rep"] / np.abs(ref["d_rep"]).sum(axis=1, keepdims=True)
            assert np.abs(np.abs(g) - 1.0 / 3.0).max() < 1e-6
        if kind == "calib_above":
            assert np.all(v < rep(c["calib"])[None, None])
            want = c["calib"].astype(np.float64).mean() / c["cfg"]["temperature"] + np.log(3.0)
            assert abs(ref["loss9"][2] - want) < 1e-12 and abs(ref["loss9"][3] - want) < 1e-12
        if kind == "calib_tie":
            r = rep(c["calib"]).reshape(B, R)
            cur = v[:, 1].reshape(2, B, R)
            assert np.all(cur[:, :, 0] == r[None, :, 0])                      # bit for bit, in float32
            assert np.all(c["q_cur"].reshape(2, B, R)[:, :, 0].astype(np.float64) == r[None, :, 0].astype(np.float64))
            # exactly half of w c softmax / (B R), the gradient the same row would get above the return
            off = np.log(0.5 ** A)
            v64 = np.stack([c["q_rand"] - off, c["q_cur"].astype(np.float64) - c["logp_cur"][None], c["q_next"].astype(np.float64) - c["logp_next"][None]], axis=1)
            z = np.maximum(v64, rep(c["calib"]).astype(np.float64)[None, None]) / c["cfg"]["temperature"]
            sm = np.exp(z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
            up = c["cfg"]["cql_weight"] * ref["loss9"][6] / (B * R)
            np.testing.assert_allclose(ref["d_rep"][:, 1].reshape(2, B, R)[:, :, 0], 0.5 * up * sm[:, 1].reshape(2, B, R)[:, :, 0], rtol=1e-9)
            others = ref["d_rep"][:, 0]
            assert np.abs(others).max() > 0
        ea = float(np.exp(np.float32(c["cql_log_alpha"][0])))
        lo, hi = c["cfg"]["alpha_min"], c["cfg"]["alpha_max"]
        if kind == "alpha_at_min":
            assert ea == lo and ref["loss9"][8] != 0.0
        if kind == "alpha_at_max":
            assert ea == hi and ref["loss9"][8] != 0.0
        if kind == "alpha_below":
            assert ea < lo and ref["loss9"][8] == 0.0 and ref["loss9"][6] == lo and ref["loss9"][7] != 0.0
        if kind == "alpha_above":
            assert ea > hi and ref["loss9"][8] == 0.0 and ref["loss9"][6] == hi and ref["loss9"][7] != 0.0
        if kind == "weight_zero":
            np.testing.assert_allclose(ref["d_data"], 2.0 * (c["q_data"].astype(np.float64) - c["target"][None]) / B, rtol=1e-12)


def test_shapes_cover_the_thread_map():
    assert {s[1] for s in EC.SHAPES} == {1, 257} and {s[2] for s in EC.SHAPES} == {1, 3, 10} and {s[0] for s in EC.SHAPES} == {1, 6, 32}
    assert any((b * r) % 64 != 0 and b * r > 256 for _, b, r in EC.SHAPES)
