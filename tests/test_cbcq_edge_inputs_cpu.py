"""CPU: every edge input of tests/cbcq_edge_cases.py has the property it claims, under float64 (and, where the claim is about
float32, float32) autograd of tests/oracle_cbcq.py's formulas, and every reference value is finite."""
import numpy as np
import pytest
import torch

from tests import cbcq_edge_cases as EC


def _finite(d):
    for k, v in d.items():
        assert np.all(np.isfinite(np.asarray(v, np.float64))), k


@pytest.mark.parametrize("A,L,B,R", EC.SHAPES)
def test_latent_inputs(A, L, B, R):
    for kind in EC.LATENT_KINDS:
        c = EC.latent_case(kind, B, L)
        ref = EC.latent_reference(c)
        _finite(ref)
        assert all(c[k].dtype == np.float32 and c[k].shape == (B, L) for k in ("mean", "log_std", "eps", "dz"))
        if kind == "ls_at_min":
            assert np.all(c["log_std"] == -4.0) and np.all(ref["d_log_std"] != 0.0)        # the gradient passes AT the bound
        if kind == "ls_at_max":
            assert np.all(c["log_std"] == 15.0) and np.all(ref["d_log_std"] != 0.0)
            assert (B * L == 1 or ((c["eps"] > 0).any() and (c["eps"] < 0).any())) and np.abs(ref["z"]).max() > 1e4
            assert np.all(np.isfinite(EC.latent_reference(c, torch.float32)["d_log_std"]))
        if kind == "ls_beyond":
            assert np.all((c["log_std"] < -4.0) | (c["log_std"] > 15.0)) and np.all(ref["d_log_std"] == 0.0)
            assert np.all(np.abs(c["log_std"] - np.clip(c["log_std"], -4, 15)) < 2e-6) and np.any(ref["d_mean"] != 0.0)
        if kind == "zero":
            assert ref["kl"] == 0.0 and np.all(ref["d_mean"] == 0.0) and np.all(ref["d_log_std"] == 0.0)
            assert np.array_equal(ref["z"], c["eps"].astype(np.float64))
            r32 = EC.latent_reference(c, torch.float32)
            assert r32["kl"] == 0.0 and np.all(r32["d_mean"] == 0.0) and np.all(r32["d_log_std"] == 0.0)


@pytest.mark.parametrize("A,L,B,R", EC.SHAPES)
def test_recon_inputs(A, L, B, R):
    M = EC.MAX_ACTION
    for kind in EC.RECON_KINDS:
        c = EC.recon_case(kind, B, A)
        for dt in (torch.float64, torch.float32):
            ref = EC.recon_reference(c, dt)
            _finite(ref)
            if kind == "saturated":                 # tanh(+-20) rounds to +-1 in both formats: an exact-zero gradient
                assert np.all(np.abs(c["logits"]) == 20.0) and np.all(np.abs(ref["recon"]) == M) and np.all(ref["d_logits"] == 0.0)
                assert ref["mse"] > 0.0
            if kind == "recon_equals_act":
                assert np.array_equal(ref["recon"], c["act"].astype(ref["recon"].dtype)) and ref["mse"] == 0.0
                assert np.all(ref["d_logits"] == 0.0)
        if kind == "generic":
            assert np.abs(ref["d_logits"]).max() > 0.0


@pytest.mark.parametrize("A,L,B,R", EC.SHAPES)
def test_target_inputs(A, L, B, R):
    for kind in EC.TARGET_KINDS:
        c = EC.target_case(kind, B, R)
        ref = EC.target_reference(c)
        assert np.all(np.isfinite(ref)) and ref.shape == (B,)
        q1, q2 = c["q1"].reshape(B, c["R"]).astype(np.float64), c["q2"].reshape(B, c["R"]).astype(np.float64)
        tq = c["lmbda"] * np.minimum(q1, q2) + (1 - c["lmbda"]) * np.maximum(q1, q2)
        if kind.startswith("q_equal"):
            assert np.array_equal(c["q1"], c["q2"]) and c["lmbda"] in (0.0, 0.75, 1.0)
            np.testing.assert_allclose(tq, q1, rtol=1e-15)              # the tie is a tie: lmbda drops out
        if kind == "max_first":
            assert np.all(tq.argmax(1) == 0)
        if kind == "max_last":
            assert np.all(tq.argmax(1) == c["R"] - 1)
        if kind == "all_equal":
            assert np.all(tq == tq[:, :1])
        if kind == "all_done":
            assert np.all(c["done"] == 1.0) and np.array_equal(ref, c["rew"].astype(np.float64))
        if kind == "r_one":
            assert c["R"] == 1 and c["q1"].shape == (B,)
        if kind == "generic" and B > 8:
            assert 0 < c["done"].sum() < B


@pytest.mark.parametrize("A,L,B,R", EC.SHAPES)
def test_perturb_inputs(A, L, B, R):
    M = EC.MAX_ACTION
    for kind in EC.PERTURB_KINDS:
        c = EC.perturb_case(kind, B, A)
        for dt in (torch.float64, torch.float32):
            ref = EC.perturb_reference(c, dt)
            _finite(ref)
            if kind == "at_bound":                  # the entry sits exactly on the bound and the gradient passes
                assert np.all(np.abs(c["sampled"]) == M) and np.all(np.abs(ref["perturbed"]) == M)
                want = c["dq"].astype(np.float64) * (EC.PHI * M)
                np.testing.assert_allclose(ref["d_logits"], want, rtol=1e-6)
                assert np.all(ref["d_logits"] != 0.0)
            if kind == "beyond":
                assert np.all(np.abs(c["sampled"]) > M) and np.all(np.abs(ref["perturbed"]) == M) and np.all(ref["d_logits"] == 0.0)
            if kind == "phi_zero":
                assert np.all(ref["d_logits"] == 0.0)
                assert np.array_equal(ref["perturbed"], np.clip(c["sampled"], -M, M).astype(ref["perturbed"].dtype))
        if kind == "generic":
            # no entry so close to the bound that float32 and float64 could fall on different sides of it
            x = torch.as_tensor(c["logits"]).double()
            pre = EC.PHI * M * torch.tanh(x) + torch.as_tensor(c["sampled"]).double()
            assert float((pre.abs() - M).abs().min()) > 1e-5
            if B * A > 50:
                assert (ref["d_logits"] == 0.0).any() and (ref["d_logits"] != 0.0).any()


@pytest.mark.parametrize("first_row", [False, True])
@pytest.mark.parametrize("N,T", [(1, 1), (1, 100), (5, 1), (5, 100)])
def test_policy_cases_have_no_near_tie(N, T, first_row):
    """The seed of the policy-forward cases leaves NO observation with a float64 top-two gap under 1e-4 of the larger value, so
    tests/test_gpu_cbcq_policy.py compares every index."""
    c = EC.policy_case(N, T, first_row)
    ref = EC.policy_reference(c)
    _finite({k: ref[k] for k in ("act", "q", "cand")})
    gap = EC.top_two_gap(ref["q"])
    print(N, T, first_row, "gaps", gap, "spread", ref["q"].max(1) - ref["q"].min(1))
    assert np.all(gap > EC.POLICY_GAP), gap
    assert np.array_equal(ref["act"], ref["cand"][np.arange(N), ref["idx"]])


@pytest.mark.parametrize("first_row", [False, True])
def test_policy_tie_case_is_a_tie(first_row):
    c = EC.policy_case(5, 100, first_row, tie=True)
    ref = EC.policy_reference(c)
    for n in range(5):
        q = ref["q"][n]
        top = np.flatnonzero(q == q.max())
        assert len(top) == 2 and top[1] == top[0] + 1 and top[0] == c["want_idx"][n] == ref["idx"][n], (n, top)
        assert np.array_equal(c["noise"][n, top[0]], c["noise"][n, top[1]])
        assert first_row is False or top[1] != 0
