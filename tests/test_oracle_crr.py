"""CPU: tests/oracle_crr.py, the torch restatement of the reference's DiscreteCRR path, against the fixtures recorded from the
unmodified reference (tools/gen_golden_crr.py), against a float64 run of itself (the yardstick of the tolerances in
tests/crr_common.py), and its closed-form head gradients against autograd."""
import numpy as np
import pytest
import torch

from tests import crr_common as CC
from tests import oracle_crr as OC


def _replay(tag, dtype=torch.float32):
    g, d, cfg, _ = CC.load_crr(tag)
    p = {k: v.to(dtype) for k, v in OC.init_params(d["c"], d["h"], d["w"], d["n_act"], d["seed"]).items()}
    st = OC.make_state(p, cfg)
    out = []
    for u in range(d["n_updates"]):
        col: dict = {}
        losses = OC.update_with_batch(st, cfg, *CC.batch_of(g, u), collect=col)
        out.append((losses, col, {k: v.detach().clone() for k, v in st.params.items()},
                    None if st.params_old is None else {k: v.clone() for k, v in st.params_old.items()}))
    return g, d, cfg, st, out


@pytest.mark.parametrize("tag", CC.TAGS)
def test_oracle_replays_the_reference_fixture(tag):
    g, d, cfg, st, out = _replay(tag)
    for u, (losses, col, params, old) in enumerate(out):
        assert np.array_equal(CC.batch_of(g, u)[4], g[f"u{u}_done"])
        np.testing.assert_allclose(CC.batch_of(g, u)[3], g[f"u{u}_batch_rew"].astype(np.float32))
        np.testing.assert_allclose(col["target"].numpy(), g[f"u{u}_target"], rtol=CC.RTOL)
        np.testing.assert_allclose(col["adv"].numpy(), g[f"u{u}_adv"], rtol=1e-4, atol=1e-6)
        for name, x in zip(CC.LOSS_NAMES, losses):
            np.testing.assert_allclose(x, float(g[f"u{u}_{name}"]), rtol=CC.RTOL, err_msg=name)
        t = [params[k] for k in OC.PARAM_ORDER]
        flat = torch.cat([x.reshape(-1) for x in t]).numpy()
        CC.check_params(flat[::CC.STRIDE], g[f"u{u}_params_strided"], tag, u, cfg.lr)
        CC.check_params(torch.cat([t[i].reshape(-1) for i in range(1, 14, 2)]).numpy(), g[f"u{u}_biases"], tag, u, cfg.lr, "biases")
        if cfg.target_update_freq > 0:
            o = [old[k] for k in OC.PARAM_ORDER]
            for name, pos in (("actor_old", CC.ACTOR_OLD), ("critic_old", CC.CRITIC_OLD)):
                flat = torch.cat([o[i].reshape(-1) for i in pos]).numpy()
                CC.check_params(flat[::CC.STRIDE], g[f"u{u}_{name}_strided"], tag, max(u - 1, 0), cfg.lr, name)   # the live net of an earlier update
        else:
            assert old is None and f"u{u}_actor_old_strided" not in g.files
    assert st.adam_step == int(g["adam_step"]) and st.iter == d["n_updates"]
    for (which, key), tol in zip((("exp_avg", "adam_m_strided"), ("exp_avg_sq", "adam_v_strided")), CC.moment_bars(tag)):
        m = st.moments(which)
        flat = torch.cat([m[k].reshape(-1) for k in OC.PARAM_ORDER]).numpy()[::CC.STRIDE]
        assert np.abs(flat - g[key]).max() <= tol * np.abs(g[key]).max()


def test_fixtures_meet_their_conditions():
    g, d, cfg, _ = CC.load_crr("exp")
    assert cfg.policy_improvement_mode == "exp" and cfg.target_update_freq == 2 and cfg.min_q_weight == 10 and d["n_updates"] >= 5
    frac, dist = g["conditions"][:, 0], g["conditions"][:, 1]
    assert frac.min() >= 0.2 and frac.max() <= 0.8 and dist.min() >= 1e-3
    for u in range(d["n_updates"]):
        e = np.exp(g[f"u{u}_adv"].astype(np.float64) / cfg.beta)
        assert 0.2 <= (e > cfg.ratio_upper_bound).mean() <= 0.8
        assert 0 < (g[f"u{u}_done"] > 0).sum() < d["batch"]
    # the sync fires at updates 0, 2 and 4: the lagged samples change there and only there
    same = [np.array_equal(g[f"u{u}_actor_old_strided"], g[f"u{u - 1}_actor_old_strided"]) for u in range(1, d["n_updates"])]
    assert same == [True, False, True, False]
    g, d, cfg, _ = CC.load_crr("binary")
    assert cfg.policy_improvement_mode == "binary" and cfg.target_update_freq == 0 and cfg.min_q_weight != 10 and d["n_updates"] == 3
    assert g["conditions"][:, 0].min() >= 0.2 and g["conditions"][:, 0].max() <= 0.8 and g["conditions"][:, 1].min() >= 1e-4
    for u in range(3):
        assert 0 < (g[f"u{u}_done"] > 0).sum() < d["batch"]


@pytest.mark.parametrize("tag", CC.TAGS)
def test_float32_oracle_vs_float64(tag):
    """The numbers behind the tolerances (tests/crr_common.py): the float32 oracle's deviation from a float64 run of itself on
    the fixture's inputs -- losses, targets, parameters after every update, Adam moments at the end -- stays within twice the
    recorded figures (the summation order of a float32 reduction may differ from one torch build to the next)."""
    g, d, cfg, st32, o32 = _replay(tag)
    _, _, _, st64, o64 = _replay(tag, torch.float64)
    e_loss = max(abs(a - b) / abs(b) for (la, *_), (lb, *_) in zip(o32, o64) for a, b in zip(la, lb))
    e_tgt = max(float((ca["target"].double() - cb["target"]).abs().max() / cb["target"].abs().max())
                for (_, ca, *_), (_, cb, *_) in zip(o32, o64))
    print(tag, "float32 vs float64: losses", e_loss, "targets", e_tgt)
    assert e_loss <= 2 * CC.F32_VS_F64["loss"] and e_tgt <= 2 * CC.F32_VS_F64["target"]
    assert 4 * CC.F32_VS_F64["loss"] <= CC.RTOL and 4 * CC.F32_VS_F64["target"] <= CC.RTOL
    for u, ((_, _, pa, _), (_, _, pb, _)) in enumerate(zip(o32, o64)):
        a = torch.cat([pa[k].reshape(-1) for k in OC.PARAM_ORDER]).double().numpy()
        b = torch.cat([pb[k].reshape(-1) for k in OC.PARAM_ORDER]).numpy()
        diff = np.abs(a - b)
        frac = float((diff > CC.RTOL * np.abs(b) + CC.ATOL_LR * cfg.lr).mean())
        print(tag, f"u{u} parameters: fraction beyond the BCQ bar", frac, "largest deviation / lr", diff.max() / cfg.lr)
        assert frac <= 2 * CC.PARAM_DEV[tag][u][0] + 1e-5 and diff.max() / cfg.lr <= 2 * CC.PARAM_DEV[tag][u][1]
    for which, rec in zip(("exp_avg", "exp_avg_sq"), CC.MOMENT_DEV[tag]):
        a = torch.cat([st32.moments(which)[k].reshape(-1) for k in OC.PARAM_ORDER]).double().numpy()
        b = torch.cat([st64.moments(which)[k].reshape(-1) for k in OC.PARAM_ORDER]).numpy()
        dev = np.abs(a - b).max() / np.abs(b).max()
        print(tag, which, "float32 vs float64", dev)
        assert dev <= 2 * rec


@pytest.mark.parametrize("mode", OC.MODES)
@pytest.mark.parametrize("a", [1, 3, 6, 64])
def test_closed_form_head_gradients_vs_autograd(a, mode):
    """dq / dl as crr_grad_kernel writes them against autograd through the reference's expressions, in float64."""
    rng = np.random.default_rng(a)
    b = 7
    q = torch.tensor(rng.normal(size=(b, a)), requires_grad=True)
    lg = torch.tensor(rng.normal(size=(b, a)), requires_grad=True)
    act, y = rng.integers(0, a, size=b), torch.tensor(rng.normal(size=b))
    args = (mode, 0.5, 1.5, 2.5)
    loss, *_ = OC.losses_from_heads(q, lg, act, y, *args)
    loss.backward()
    dq, dl = OC.closed_form_grads(q, lg, act, y, *args)
    np.testing.assert_allclose(dq.numpy(), q.grad.numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(dl.numpy(), lg.grad.numpy(), rtol=1e-10, atol=1e-13)
    if a == 1:
        assert not lg.grad.any()


@pytest.mark.parametrize("mode", OC.MODES)
def test_broadcast_forms_vs_per_sample_forms(mode):
    """The reference's two [B] against [B, 1] broadcasts: the CQL mean over B x B terms equals mean_b (lse_b - qa_b); the
    actor loss, the mean of a [B, B] product, equals mean(nll) * mean(coef) -- value and gradient alike -- and is NOT
    mean_b (nll_b coef_b) unless the weight is constant."""
    rng = np.random.default_rng(5)
    b, a = 9, 4
    q0, l0 = torch.tensor(rng.normal(size=(b, a))), torch.tensor(rng.normal(size=(b, a)))
    act, y = rng.integers(0, a, size=b), torch.tensor(rng.normal(size=b))
    grads = []
    for per_sample in (False, True):
        q, lg = q0.clone().requires_grad_(True), l0.clone().requires_grad_(True)
        loss, al, cl, ql, adv = OC.losses_from_heads(q, lg, act, y, mode, 0.5, 1.5, 2.5, per_sample=per_sample)
        loss.backward()
        grads.append((loss.item(), al.item(), ql.item(), q.grad.clone(), lg.grad.clone()))
    for x, z in zip(*grads):
        np.testing.assert_allclose(np.asarray(x), np.asarray(z), rtol=1e-12, atol=1e-14)
    nll = -torch.distributions.Categorical(logits=l0).log_prob(torch.as_tensor(act))
    coef = {"exp": (adv.detach() / 0.5).exp().clamp(0, 1.5), "binary": (adv.detach() > 0).double(), "all": torch.ones(b).double()}[mode]
    rowwise = float((nll * coef).mean())
    if mode == "all":
        assert abs(rowwise - grads[0][1]) < 1e-12
    else:
        assert abs(rowwise - grads[0][1]) > 1e-3
