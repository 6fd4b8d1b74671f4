"""CPU: the oracle (tests/oracle_dsac_cnn.py) on the edge inputs of tests/dsac_cnn_edge_cases.py -- the statements the GPU
test of the raw-array kernels (test_gpu_dsac_cnn_edges.py) relies on hold for the reference's own expressions, and the float32
oracle agrees with a float64 run of itself within the tolerances used there."""
import numpy as np
import pytest
import torch

from tests import dsac_cnn_edge_cases as EC

CASES = EC.cases()
IDS = [n for n, _ in CASES]


def test_the_case_list_covers_the_shapes_and_branches():
    shapes = {(c["logits"].shape[1], c["logits"].shape[0]) for _, c in CASES}
    assert {(a, b) for a in EC.A_SET for b in EC.B_SET} <= shapes
    assert any(c["weight"] is None for _, c in CASES) and any(c["weight"] is not None and not c["weight"].any() for _, c in CASES)
    assert any(c["weight"] is not None and (c["weight"] == 0).any() and c["weight"].any() for _, c in CASES)
    assert any(c["device_alpha"] for _, c in CASES) and any(not c["device_alpha"] for _, c in CASES)
    for _, c in CASES:
        b, a = c["logits"].shape
        assert c["act"][0] == 0 and (b == 1 or c["act"][-1] == a - 1) and c["act"].min() >= 0 and c["act"].max() < a


@pytest.mark.parametrize("name,c", CASES, ids=IDS)
def test_oracle_on_edge_inputs(name, c):
    e = EC.expected(c)
    b, a = c["logits"].shape
    assert all(np.isfinite(v).all() for v in e.values()), name
    w = np.ones(b) if c["weight"] is None else c["weight"].astype(np.float64)
    # the critic's closed form: 2 w td / B at act, exact zeros elsewhere
    hot = np.zeros((b, a))
    hot[np.arange(b), c["act"]] = 1.0
    assert np.all(e["dq"][hot == 0] == 0.0)
    np.testing.assert_allclose(e["dq"][hot == 1], 2.0 * w * e["td"] / b, rtol=1e-6, atol=1e-30)
    np.testing.assert_allclose(e["critic_loss"], (e["td"] ** 2 * w).mean(), rtol=1e-6)
    # the entropy lies in [0, log A], the probabilities sum to one
    assert (e["entropy"] >= 0.0).all() and (e["entropy"] <= np.log(a) + 1e-5).all()
    np.testing.assert_allclose(e["probs"].sum(1), 1.0, rtol=1e-6)
    # the actor gradient sums to zero over the actions (softmax): to rounding
    assert np.abs(e["dlogits"].sum(1)).max() <= 1e-5 * max(np.abs(e["dlogits"]).max(), 1e-30) * a + 1e-12
    if a == 1:
        assert np.all(e["entropy"] == 0.0) and np.all(e["dlogits"] == 0.0) and np.all(e["probs"] == 1.0)
        np.testing.assert_allclose(e["target"], np.minimum(c["q1"], c["q2"])[:, 0], rtol=1e-6)
    if name.startswith("dominant"):
        top = c["logits"].argmax(1)
        assert np.all(np.sort(e["probs"], 1)[:, :-1] == 0.0) and np.all(e["probs"][np.arange(b), top] == 1.0)
        assert np.all(e["entropy"] == 0.0)
        np.testing.assert_allclose(e["target"], np.minimum(c["q1"], c["q2"])[np.arange(b), top], rtol=1e-6)
        assert np.all(e["dlogits"][e["probs"] == 0.0] == 0.0)                 # p = 0: no gradient reaches that logit
    if name.startswith("uniform"):
        # the normalised logits are lg - logsumexp(lg): at a level of 50 one float32 rounding of the logsumexp is 3.8e-6
        level = np.abs(c["logits"][:, 0]).astype(np.float64)
        assert np.all(np.abs(e["entropy"] - np.log(a)) <= 1e-6 * np.log(a) + 2.0 ** -23 * (level + np.log(a)))
        np.testing.assert_allclose(e["probs"], 1.0 / a, rtol=1e-6)
    if name.startswith("ties"):
        np.testing.assert_array_equal(np.minimum(c["q1"], c["q2"]), c["q1"])
    if name == "weight-zero":
        assert e["critic_loss"] == 0.0 and np.all(e["dq"] == 0.0) and np.abs(e["td"]).min() > 0
    if name == "td-large":
        assert np.abs(e["td"]).max() > 9e5 and e["critic_loss"] > 1e11
    if name == "alpha-zero":
        np.testing.assert_allclose(e["target"], (e["probs"] * np.minimum(c["q1"], c["q2"])).sum(1), rtol=1e-6)


def test_device_alpha_and_fixed_alpha_cases_share_inputs():
    d = dict(CASES)
    a, f = d["alpha-device"], d["alpha-fixed"]
    assert all(np.array_equal(a[k], f[k]) for k in ("logits", "q1", "q2", "act", "y"))
    # exp(float32(log 1.5)) is within one float32 rounding of 1.5
    assert abs(EC.alpha_of(a) - 1.5) <= 1.5 * 2.0 ** -23 and EC.alpha_of(f) == 1.5


@pytest.mark.parametrize("name,c", CASES, ids=IDS)
def test_float32_oracle_agrees_with_float64_within_the_kernel_bars(name, c):
    """The bars of test_gpu_dsac_cnn_edges.py must leave room for a correct float32 evaluation: the float32 oracle against the
    float64 oracle stays within HALF of each (two float32 evaluations then lie within the bar of each other)."""
    e32, e64 = EC.expected(c, torch.float32), EC.expected(c, torch.float64)
    for k in ("target", "td", "dq", "dlogits", "critic_loss", "actor_loss", "entropy"):
        scale = max(np.abs(e64[k]).max(), 1e-30)
        assert np.abs(e32[k] - e64[k]).max() <= 0.5 * EC.TOL * scale, (k, np.abs(e32[k] - e64[k]).max() / scale)
