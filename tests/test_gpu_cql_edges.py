"""GPU: the continuous-CQL loss kernels (ts_cql_loss: cql_loss_kernel + cql_finish_kernel) against float64 autograd of
tests/oracle_cql.py's formula on the edge inputs of tests/cql_edge_cases.py (checked on the CPU by
tests/test_cql_edge_inputs_cpu.py).  Tolerances of tests/test_gpu_td3_edges.py: losses rtol 1e-5 / atol 1e-6, gradients within
2e-5 of the tensor's largest entry, exact zeros and exact halves compared exactly.  Nothing is excluded."""
import numpy as np
import pytest
import torch

from tests import cql_edge_cases as EC

pytestmark = pytest.mark.gpu


def run(c):
    from tianshou_amd import cql as Q

    cfg = Q.CQLConfig(**c["cfg"])
    d = lambda x: None if x is None else torch.as_tensor(x).cuda()  # noqa: E731
    d_data, d_rep, loss9 = Q.cql_loss(d(c["q_data"]), d(c["target"]), d(c["q_rand"]), d(c["q_cur"]), d(c["q_next"]), d(c["logp_cur"]),
                                      d(c["logp_next"]), d(c["calib"]), d(c["cql_log_alpha"]), c["A"], cfg)
    torch.cuda.synchronize()
    return d_data.cpu().numpy(), d_rep.cpu().numpy(), loss9.cpu().numpy()


def close_grad(got, want, what):
    top = np.abs(want).max()
    if top == 0.0:
        assert np.all(got == 0.0), what
    else:
        assert np.abs(got.astype(np.float64) - want).max() <= 2e-5 * top, (what, np.abs(got - want).max() / top)


@pytest.mark.parametrize("A,B,R", EC.SHAPES)
def test_loss_kernels_on_edge_inputs(A, B, R):
    for kind in EC.KINDS:
        c = EC.make(kind, A, B, R)
        ref = EC.reference(c)
        d_data, d_rep, loss9 = run(c)
        print(kind, A, B, R, "loss9", loss9, "ref", ref["loss9"])
        np.testing.assert_allclose(loss9, ref["loss9"], rtol=1e-5, atol=1e-6, err_msg=kind)
        close_grad(d_data, ref["d_data"], (kind, "d_data"))
        close_grad(d_rep, ref["d_rep"], (kind, "d_rep"))
        if kind in EC.ZERO_REP_GRAD:
            assert np.all(d_rep == 0.0), kind
        if kind in ("alpha_below", "alpha_above"):
            assert loss9[8] == 0.0 and loss9[7] != 0.0, kind
        if kind in ("alpha_at_min", "alpha_at_max"):
            assert loss9[6] == 1.0 and loss9[8] != 0.0, kind
        if kind == "calib_tie":
            # the tied entries against the reference's half gradient (mask exactly 0.5); the bit-exact half is the next test's
            got = d_rep[:, 1].reshape(2, B, R)[:, :, 0]
            assert np.abs(got - ref["d_rep"][:, 1].reshape(2, B, R)[:, :, 0]).max() <= 2e-5 * np.abs(ref["d_rep"]).max()
            assert np.all(got > 0)
        if kind == "all_equal":
            s = np.abs(d_rep).sum(axis=1, keepdims=True)
            assert np.abs(np.abs(d_rep) / s - 1.0 / 3.0).max() < 1e-6
        if kind == "weight_zero":
            assert np.array_equal(d_data, (2.0 * (torch.as_tensor(c["q_data"]) - torch.as_tensor(c["target"])[None]) / float(B)).numpy())
        if kind == "calib_above":
            want = c["calib"].astype(np.float64).mean() / c["cfg"]["temperature"] + np.log(3.0)
            np.testing.assert_allclose(loss9[2:4], want, rtol=1e-6)


def test_tie_is_exactly_half_of_the_untied_gradient():
    """One row, one critic pair: the return below the pi(s) value gives gradient g there, the return EQUAL to it g / 2 bit for bit
    (the softmax weights are the same floats: the maximum does not change the value)."""
    c = EC.make("calib_tie", 6, 1, 1)
    tie = run(c)[1]
    c2 = dict(c)
    c2["calib"] = np.nextafter(c["calib"], np.float32(-np.inf)).astype(np.float32)
    # (the other two values must sit on the same side of both returns)
    lo = run(c2)[1]
    assert np.array_equal(tie[:, 1] * 2.0, lo[:, 1]) and np.array_equal(tie[:, 0], lo[:, 0]) and np.array_equal(tie[:, 2], lo[:, 2])


def test_same_call_twice_gives_the_same_bits():
    c = EC.make("generic", 6, 257, 10)
    a, b = run(c), run(c)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
