"""GPU: the three DiscreteSAC head kernels on raw arrays (ts_dsac_cnn_target / _critic / _actor through tianshou_amd.dsac_cnn)
on the edge inputs of tests/dsac_cnn_edge_cases.py, against the oracle's values and autograd gradients.  Every output buffer
is pre-filled with a sentinel that must be gone afterwards, padding columns must be exact zeros."""
import numpy as np
import pytest
import torch

from tests import dsac_cnn_edge_cases as EC

pytestmark = pytest.mark.gpu

CASES = EC.cases()
IDS = [n for n, _ in CASES]
SENTINEL = -12345.0


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    assert err <= EC.TOL * scale, (what, err, scale)


def _run(c):
    from tianshou_amd import dsac_cnn as DS

    la = EC.log_alpha_of(c)
    kw = dict(alpha=c["alpha"], log_alpha=None if la is None else torch.tensor([la], dtype=torch.float32, device="cuda"))
    tgt = DS.target_value(c["logits"], c["q1"], c["q2"], fill=SENTINEL, **kw)
    cr = DS.critic_terms(c["q1"], c["act"], c["y"], c["weight"], fill=SENTINEL)
    ac = DS.actor_terms(c["logits"], c["q1"], c["q2"], fill=SENTINEL, **kw)
    return tgt, cr, ac


@pytest.mark.parametrize("name,c", CASES, ids=IDS)
def test_head_kernels_on_edge_inputs(name, c):
    b, a = c["logits"].shape
    ld = (a + 31) // 32 * 32
    e = EC.expected(c)
    tgt, cr, ac = _run(c)
    outs = {"target": tgt, **{"critic." + k: v for k, v in cr.items()}, **{"actor." + k: v for k, v in ac.items()}}
    for k, v in outs.items():                                                     # every element written, nothing but numbers
        v = v.cpu().numpy()
        assert np.isfinite(v).all() and not (v == SENTINEL).any(), k
    assert tuple(cr["dq"].shape) == (b, ld) and tuple(ac["dlogits"].shape) == (b, ld)
    dq, dl = cr["dq"].cpu().numpy(), ac["dlogits"].cpu().numpy()
    assert np.all(dq[:, a:] == 0.0) and np.all(dl[:, a:] == 0.0)                   # padding: exact zeros
    _close(tgt.cpu(), e["target"], "target")
    _close(cr["td"].cpu(), e["td"], "td")
    _close(cr["loss"].cpu()[0], e["critic_loss"], "critic_loss")
    _close(dq[:, :a], e["dq"], "dq")
    assert np.all(dq[:, :a][e["dq"] == 0.0] == 0.0)                                # zero away from act, and under zero weights
    _close(ac["entropy"].cpu(), e["entropy"], "entropy")
    _close(ac["loss"].cpu()[0], e["actor_loss"], "actor_loss")
    _close(dl[:, :a], e["dlogits"], "dlogits")
    w = np.ones(b, np.float32) if c["weight"] is None else c["weight"]
    np.testing.assert_array_equal(cr["terms"].cpu().numpy(), cr["td"].cpu().numpy() ** 2 * w)
    if a == 1:
        assert np.all(ac["entropy"].cpu().numpy() == 0.0) and np.all(dl == 0.0)
    if name.startswith("dominant"):
        assert np.all(ac["entropy"].cpu().numpy() == 0.0)                          # p exactly 0 / 1
        assert np.all(dl[:, :a][e["dlogits"] == 0.0] == 0.0)                       # exactly 0 where the reference's gradient is
        top = c["logits"].argmax(1)
        np.testing.assert_array_equal(tgt.cpu().numpy(), np.minimum(c["q1"], c["q2"])[np.arange(b), top])
    if name.startswith("uniform"):
        level = np.abs(c["logits"][:, 0]).astype(np.float64)
        assert np.all(np.abs(ac["entropy"].cpu().numpy() - np.log(a)) <= 1e-6 * np.log(a) + 2.0 ** -23 * (level + np.log(a)))
    if name == "weight-zero":
        assert float(cr["loss"]) == 0.0 and np.all(dq == 0.0)
    # reruns are bit-identical (fixed summation order in the batch means)
    tgt2, cr2, ac2 = _run(c)
    assert torch.equal(tgt, tgt2) and all(torch.equal(cr[k], cr2[k]) for k in cr) and all(torch.equal(ac[k], ac2[k]) for k in ac)


def test_ties_do_not_depend_on_which_critic_is_read():
    from tianshou_amd import dsac_cnn as DS

    c = dict(CASES)["ties-A33"]
    a = DS.target_value(c["logits"], c["q1"], c["q2"], alpha=0.2)
    b = DS.target_value(c["logits"], c["q2"], c["q1"], alpha=0.2)
    one = DS.target_value(c["logits"], c["q1"], c["q1"], alpha=0.2)
    assert torch.equal(a, b) and torch.equal(a, one)
    x, y = DS.actor_terms(c["logits"], c["q1"], c["q2"], alpha=0.2), DS.actor_terms(c["logits"], c["q2"], c["q1"], alpha=0.2)
    assert all(torch.equal(x[k], y[k]) for k in x)


def test_device_alpha_equals_fixed_alpha_of_the_same_value():
    """alpha read from log_alpha on the device against the same value passed as a scalar: equal to a rounding of exp()."""
    from tianshou_amd import dsac_cnn as DS

    c = dict(CASES)["alpha-device"]
    la = torch.tensor([EC.log_alpha_of(c)], dtype=torch.float32, device="cuda")
    fixed = float(la.exp().item())                    # the device's own exp of that float32
    t_dev = DS.target_value(c["logits"], c["q1"], c["q2"], log_alpha=la)
    t_fix = DS.target_value(c["logits"], c["q1"], c["q2"], alpha=fixed)
    np.testing.assert_allclose(t_dev.cpu().numpy(), t_fix.cpu().numpy(), rtol=2e-7)
    a_dev = DS.actor_terms(c["logits"], c["q1"], c["q2"], log_alpha=la)
    a_fix = DS.actor_terms(c["logits"], c["q1"], c["q2"], alpha=fixed)
    for k in a_dev:
        np.testing.assert_allclose(a_dev[k].cpu().numpy(), a_fix[k].cpu().numpy(), rtol=2e-6, atol=1e-7, err_msg=k)
    assert torch.equal(a_dev["entropy"], a_fix["entropy"])                        # alpha does not enter the entropy


def test_argument_checks():
    from tianshou_amd import dsac_cnn as DS

    z = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="differ in shape"):
        DS.target_value(z, z, np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="batch sizes differ"):
        DS.critic_terms(z, [0, 1, 2], [0.0] * 4)
    with pytest.raises(ValueError, match="n_act"):
        DS.actor_terms(np.zeros((4, 65), np.float32), np.zeros((4, 65), np.float32), np.zeros((4, 65), np.float32))
    with pytest.raises(ValueError, match="one float32"):
        DS.target_value(z, z, z, log_alpha=[0.0, 1.0])
