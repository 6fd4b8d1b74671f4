"""GPU parity of continuous CQL (tianshou_amd.cql over ts_cql_update) against tests/oracle_cql.py, the restatement pinned to the
reference by tests/golden/cql_*.npz (tests/test_oracle_cql.py)."""
import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from tests import cql_common as CC
from tests import oracle_cql as OC

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _batch(B, R, obs_dim, act_dim, seed, done_p=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(obs=r(B, obs_dim), act=torch.rand(B, act_dim, generator=g) * 2 - 1, rew=r(B),
                done=(torch.rand(B, generator=g) < done_p).float(), obs_next=r(B, obs_dim), noise_actor=r(B, act_dim),
                noise_next=r(B, act_dim), random_act=torch.rand(B * R, act_dim, generator=g) * 2 - 1,
                noise_rep_cur=r(B * R, act_dim), noise_rep_next=r(B * R, act_dim), calib=r(B) * 2)


def _stats_close(got, out, rtol, atol=1e-7):
    want = CC.stats_vector(out)
    keep = ~np.isnan(want)
    np.testing.assert_allclose(np.asarray(got, np.float64)[keep], want[keep], rtol=rtol, atol=atol)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_update_matches_reference_golden(tag):
    """Both fixtures on the engine, update by update, at tests/test_gpu_td3bc.py / test_gpu_sac.py's bars: statistics rtol 2e-5 /
    atol 1e-7, strided parameters and lagged parameters rtol 1e-5 / atol 0.02 lr, the final moments rtol 1e-4 with atol 1e-7 /
    1e-10; the target against the oracle's (rtol 1e-5 / atol 2e-5, the returns' bar), the critics' gradient norms before
    clipping and cql_log_alpha at the statistics' bar; the embedding's padding stays zero."""
    from tianshou_amd import sac as S
    from tianshou_amd import widths as W

    g, d, cfg = CC.load_cql(tag)
    p0 = OS.init_sac_params(d["obs_dim"], d["act_dim"], d["seed"], d["hidden"])
    eng = CC.engine_from(*p0, cfg, d["activation"])
    st = OC.CQLState.create(*p0, cfg)
    sa, sc = OS.layer_sizes(d["hidden"])
    pc, pa = eng.critic1.numel(), eng.actor.numel()
    for u in range(d["n_updates"]):
        b = CC.batch_of(g, u, cfg.calibrated)
        with OS.activation(d["activation"]):
            ref = OC.update_with_batch(st, cfg, **b)
        grads = torch.zeros(2 * pc + pa, dtype=torch.float32, device="cuda")
        tgt = torch.zeros(d["batch"], dtype=torch.float32, device="cuda")
        stats = eng.update_with_batch(**b, grads_out=grads, target_out=tgt)
        s = stats.cpu().numpy().astype(np.float64)
        want = g[f"u{u}_stats"]
        keep = ~np.isnan(want)
        print(tag, u, "stats", s, "golden", want)
        np.testing.assert_allclose(s[keep], want[keep], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(tgt.cpu().numpy(), ref["target"].numpy(), rtol=1e-5, atol=2e-5)
        norms = [float(torch.linalg.vector_norm(grads[k * pc:(k + 1) * pc].double())) for k in range(2)]
        np.testing.assert_allclose(norms, g[f"u{u}_grad_norms"], rtol=2e-5)
        if cfg.with_lagrange:
            np.testing.assert_allclose(float(eng.cql_log_alpha), float(g[f"u{u}_cql_log_alpha"][0]), rtol=2e-5, atol=1e-7)
        for name in CC.NETS:
            conv = S.actor_flat_to_torch if name.startswith("actor") else S.critic_flat_to_torch
            sz = sa if name.startswith("actor") else sc
            full = conv(getattr(eng, name), d["obs_dim"], d["act_dim"], eng.hidden, depth=eng.depth)
            assert W.padding_is_zero_layers(full, sz), name
            flat = torch.cat([t.reshape(-1) for t in W.unpad_layers(full, sz)])
            lr = cfg.actor_lr if name.startswith("actor") else cfg.critic_lr
            np.testing.assert_allclose(flat.cpu().numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=0.02 * lr, err_msg=name)
    assert eng.adam_step == d["n_updates"]
    for name in ("actor", "critic1", "critic2"):
        conv = S.actor_flat_to_torch if name == "actor" else S.critic_flat_to_torch
        sz = sa if name == "actor" else sc
        for suffix, atol in (("m", 1e-7), ("v", 1e-10)):
            full = conv(getattr(eng, f"{name}_{suffix}"), d["obs_dim"], d["act_dim"], eng.hidden, depth=eng.depth)
            flat = torch.cat([t.reshape(-1) for t in W.unpad_layers(full, sz)])
            np.testing.assert_allclose(flat.cpu().numpy()[::61], g[f"adam_{suffix}_{name}"], rtol=1e-4, atol=atol, err_msg=name + suffix)
    if cfg.with_lagrange:
        np.testing.assert_allclose([float(eng.cql_log_alpha_m), float(eng.cql_log_alpha_v)], g["adam_cql_alpha"][1:], rtol=1e-4)


ROUTES = [(256, "relu", 17, 6, 80, 10), (64, "tanh", 11, 3, 70, 3)]


def _grad_only_cfg(**kw):
    base = dict(actor_lr=-1.0, critic_lr=-1.0, alpha_lr=-1.0, cql_alpha_lr=-1.0, tau=0.0, alpha=0.15, auto_alpha=False)
    base.update(kw)
    return OC.CQLConfig(**base)


@pytest.mark.parametrize("hidden,activation,obs_dim,act_dim,B,R", ROUTES)
def test_gradient_only_mode_vs_oracle(hidden, activation, obs_dim, act_dim, B, R):
    """Every learning rate -1, tau 0: nothing moves, and the three gradients, the statistics and the target equal the oracle's
    (rel_err < 2e-5 per tensor, statistics rtol 2e-5): the fused Net[256, 256] route and a per-layer route (hidden 64, tanh)."""
    from tianshou_amd import sac as S

    cfg = _grad_only_cfg(num_repeat_actions=R, temperature=0.8, cql_weight=2.0, lagrange_threshold=1.0, auto_alpha=True,
                         target_entropy=-float(act_dim))
    p = OS.init_sac_params(obs_dim, act_dim, 31, hidden)
    eng = CC.engine_from(*p, cfg, activation)
    eng._cql3[0] = 0.4
    names = ("actor", "critic1", "critic2", "critic1_old", "critic2_old", "actor_m", "critic1_v", "log_alpha", "log_alpha_m", "_cql3")
    before = [getattr(eng, n).clone() for n in names]
    b = _batch(B, R, obs_dim, act_dim, 4)
    st = OC.CQLState.create(*p, cfg)
    st.cql_log_alpha = torch.tensor(0.4)
    col: dict = {}
    with OS.activation(activation):
        ref = OC.update_with_batch(st, cfg, **b, collect=col, step=False)
    pa, pc = eng.actor.numel(), eng.critic1.numel()
    grads = torch.zeros(2 * pc + pa, dtype=torch.float32, device="cuda")
    tgt = torch.zeros(B, dtype=torch.float32, device="cuda")
    stats = eng.update_with_batch(**b, grads_out=grads, target_out=tgt)
    for n, t in zip(names, before):
        assert torch.equal(getattr(eng, n), t), n
    _stats_close(stats.cpu().numpy(), ref, 2e-5)
    np.testing.assert_allclose(tgt.cpu().numpy(), ref["target"].numpy(), rtol=1e-5, atol=2e-5)
    got = {"critic1": S.critic_flat_to_torch(grads[:pc], obs_dim, act_dim, eng.hidden),
           "critic2": S.critic_flat_to_torch(grads[pc:2 * pc], obs_dim, act_dim, eng.hidden),
           "actor": S.actor_flat_to_torch(grads[2 * pc:], obs_dim, act_dim, eng.hidden)}
    for name, tensors in got.items():
        order = OS.ACTOR_ORDER if name == "actor" else OS.CRITIC_ORDER
        for t, key in zip(tensors, order):
            e = rel_err(t.cpu(), col[name + "_grads"][key])
            print(name, key, e)
            assert e < 2e-5, (name, key, e)


def test_actor_and_plain_critic_gradients_are_sacs():
    """Same parameters, noise and returns (= target_out): the actor gradient equals ts_sac_update's (printed: bit-identical or
    not), and at cql_weight = 0 without the multiplier the critic gradient equals ts_sac_update's within 2e-5 of its largest
    entry (the stacked pass sums B (1 + 3R) rows, all but B of them with zero upstream gradient, in another order)."""
    from tianshou_amd import sac as S

    obs_dim, act_dim, B, R = 17, 6, 80, 4
    cfg = _grad_only_cfg(num_repeat_actions=R, cql_weight=0.0, with_lagrange=False, calibrated=False)
    p = OS.init_sac_params(obs_dim, act_dim, 33, 256)
    q, s = CC.engine_from(*p, cfg), CC.engine_from(*p, cfg, cls=S.SACEngine)
    b = _batch(B, R, obs_dim, act_dim, 6)
    pa, pc = q.actor.numel(), q.critic1.numel()
    gq, gs = (torch.zeros(2 * pc + pa, dtype=torch.float32, device="cuda") for _ in range(2))
    tgt = torch.zeros(B, dtype=torch.float32, device="cuda")
    b.pop("calib")
    q.update_with_batch(**b, grads_out=gq, target_out=tgt)
    s.update_with_batch(b["obs"], b["act"], tgt, b["noise_actor"], grads_out=gs)
    same = torch.equal(gq[2 * pc:], gs[2 * pc:])
    print("actor gradient bit-identical to ts_sac_update's:", same, "max abs diff", float((gq[2 * pc:] - gs[2 * pc:]).abs().max()))
    assert rel_err(gq[2 * pc:].cpu(), gs[2 * pc:].cpu()) < 2e-5
    for k in range(2):
        assert rel_err(gq[k * pc:(k + 1) * pc].cpu(), gs[k * pc:(k + 1) * pc].cpu()) < 2e-5, k


def test_clip_scales_adams_input_and_nonpositive_norm_does_not_clip():
    """One update from the same state at three settings of max_grad_norm: below the pre-clip norm, the step is Adam's on
    coef * grad (coef = max_norm / (norm + 1e-6), the recorded gradient and torch's arithmetic: first moment = 0.1 coef g,
    second = 0.001 (coef g)^2 at the moments' bars); far above it and <= 0, the step is Adam's on the gradient itself, and the
    two are bit-identical."""
    obs_dim, act_dim, B, R = 11, 3, 70, 3
    p = OS.init_sac_params(obs_dim, act_dim, 35, 64)
    b = _batch(B, R, obs_dim, act_dim, 8)
    res = {}
    for mg in (1e-3, 1e9, 0.0, -1.0):
        cfg = OC.CQLConfig(num_repeat_actions=R, max_grad_norm=mg, critic_lr=1e-3, actor_lr=-1.0, alpha=0.2)
        eng = CC.engine_from(*p, cfg, "tanh")
        pc, pa = eng.critic1.numel(), eng.actor.numel()
        grads = torch.zeros(2 * pc + pa, dtype=torch.float32, device="cuda")
        eng.update_with_batch(**b, grads_out=grads)
        res[mg] = (grads[:pc].clone(), eng.critic1_m.clone(), eng.critic1_v.clone(), eng.critic1.clone())
    g = res[1e-3][0]
    assert torch.equal(g, res[1e9][0]) and torch.equal(g, res[0.0][0])             # grads_out is the gradient BEFORE clipping
    norm = float(torch.linalg.vector_norm(g.double()))
    assert norm > 1e-3
    coef = 1e-3 / (norm + 1e-6)
    np.testing.assert_allclose(res[1e-3][1].cpu().numpy(), (0.1 * coef * g).cpu().numpy(), rtol=1e-4, atol=1e-7 * coef)
    np.testing.assert_allclose(res[1e-3][2].cpu().numpy(), (0.001 * (coef * g) ** 2).cpu().numpy(), rtol=1e-4, atol=1e-10 * coef * coef)
    np.testing.assert_allclose(res[0.0][1].cpu().numpy(), (0.1 * g).cpu().numpy(), rtol=1e-5, atol=1e-8)
    for k in range(1, 4):
        assert torch.equal(res[0.0][k], res[-1.0][k]) and torch.equal(res[0.0][k], res[1e9][k]), k
    assert not torch.equal(res[0.0][3], res[1e-3][3])


def test_done_all_ones_gives_the_reward_as_target():
    obs_dim, act_dim, B, R = 11, 3, 70, 3
    cfg = _grad_only_cfg(num_repeat_actions=R)
    eng = CC.engine_from(*OS.init_sac_params(obs_dim, act_dim, 36, 64), cfg)
    b = _batch(B, R, obs_dim, act_dim, 9)
    b["done"] = torch.ones(B)
    tgt = torch.zeros(B, dtype=torch.float32, device="cuda")
    eng.update_with_batch(**b, target_out=tgt)
    assert torch.equal(tgt.cpu(), b["rew"])


@pytest.mark.parametrize("hidden,activation", [(256, "relu"), (64, "tanh")])
def test_actor_on_2b_rows_equals_actor_on_repeated_rows(hidden, activation):
    """The R repeated rows of an observation are identical, so the engine runs the actor on B rows per observation set instead
    of B R: ts_sac_policy_forward on literally repeated rows gives the same bits as on the B rows, repeated afterwards."""
    obs_dim, act_dim, B, R = 17, 6, 48, 10
    cfg = _grad_only_cfg(num_repeat_actions=R)
    eng = CC.engine_from(*OS.init_sac_params(obs_dim, act_dim, 37, hidden), cfg, activation)
    g = torch.Generator().manual_seed(1)
    obs, noise = torch.randn(B, obs_dim, generator=g).cuda(), torch.randn(B * R, act_dim, generator=g).cuda()
    rep = obs.unsqueeze(1).repeat(1, R, 1).view(B * R, obs_dim).contiguous()
    a_rep, lp_rep = eng.policy_forward(rep, noise)
    # B rows: the head is evaluated once per observation; the same noise rows then need the repeated head, which
    # policy_forward only offers through its inputs -- so compare per repeat index r: rows b R + r of the repeated call
    # against a B-row call with noise[b R + r]
    same = True
    for r in range(R):
        a_b, lp_b = eng.policy_forward(obs, noise.view(B, R, act_dim)[:, r].contiguous())
        same &= torch.equal(a_b, a_rep.view(B, R, act_dim)[:, r]) and torch.equal(lp_b, lp_rep.view(B, R, 1)[:, r])
    print("actor on B rows bit-identical to repeated rows:", same)
    assert same


def test_argument_errors():
    from tianshou_amd import _lib

    obs_dim, act_dim, B, R = 7, 3, 5, 2
    b = _batch(B, R, obs_dim, act_dim, 0)
    p = OS.init_sac_params(obs_dim, act_dim, 1, 64)
    for over in (dict(temperature=0.0), dict(alpha_min=2.0, alpha_max=1.0), dict(cql_weight=float("nan")), dict(num_repeat_actions=0)):
        eng = CC.engine_from(*p, _grad_only_cfg(num_repeat_actions=R), **over)
        bb = dict(b)
        if over.get("num_repeat_actions") == 0:
            bb.update(random_act=torch.zeros(0, act_dim), noise_rep_cur=torch.zeros(0, act_dim), noise_rep_next=torch.zeros(0, act_dim))
        with pytest.raises(_lib.EngineError) as e:
            eng.update_with_batch(**bb)
        assert e.value.code == _lib.TS_ERR_INVALID_ARG and eng.adam_step == 0
    eng = CC.engine_from(*p, _grad_only_cfg(num_repeat_actions=R))
    bb = dict(b)
    bb.pop("calib")
    with pytest.raises(ValueError):
        eng.update_with_batch(**bb)


# -- the HipCQL drop-in over tests/standin_cql.py ------------------------------------------------------------------------
def _host_buffer(SC, g, d):
    """A host replay-buffer stand-in holding the fixture's (full) buffer and its calibration_returns."""
    E, slots = d["E"], d["slots"]
    assert d["steps"] == slots
    buf = SC.VectorReplayBuffer(E * slots, E, obs_shape=(d["obs_dim"],), act_shape=(d["act_dim"],))
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated", "done"):
        getattr(buf, k)[:] = g[k]
    buf._lengths[:], buf.last_index[:] = slots, buf._offset + slots - 1
    for sb in buf.buffers:
        sb._size, sb._insertion_idx = slots, 0
    buf._meta.calibration_returns = g["calibration_returns"]
    return buf


def _make_algo(SC, d, cfg, seed=None, auto_alpha=None):
    from torch import nn
    from tianshou_amd.integration import make_hip_cql

    sa, sc = OS.layer_sizes(d["hidden"])
    fn = nn.Tanh if d["activation"] == "tanh" else nn.ReLU
    obs_dim, act_dim = d["obs_dim"], d["act_dim"]
    actor = SC.ContinuousActorProbabilistic(SC.Net(obs_dim, list(sa), fn), act_dim, unbounded=True, conditioned_sigma=True)
    c1, c2 = (SC.ContinuousCritic(SC.Net(obs_dim + act_dim, list(sc), fn)) for _ in range(2))
    p0 = OS.init_sac_params(obs_dim, act_dim, d["seed"] if seed is None else seed, (sa, sc))
    for mod, pd in ((actor, p0[0]), (c1, p0[1]), (c2, p0[2])):
        mod.load_state_dict(dict(zip(mod.state_dict(), pd.values())))
    auto = cfg.auto_alpha if auto_alpha is None else auto_alpha
    alpha = SC.AutoAlpha(cfg.target_entropy, cfg.log_alpha0, cfg.alpha_lr) if auto else 0.2
    algo = make_hip_cql(ref=SC)(policy=SC.Policy(actor), critic=c1, critic2=c2, lr=cfg.actor_lr, critic_lr=cfg.critic_lr,
                                cql_alpha_lr=cfg.cql_alpha_lr, cql_weight=cfg.cql_weight, tau=cfg.tau, gamma=cfg.gamma, alpha=alpha,
                                temperature=cfg.temperature, with_lagrange=cfg.with_lagrange, lagrange_threshold=cfg.lagrange_threshold,
                                min_action=d["min_action"], max_action=d["max_action"], num_repeat_actions=cfg.num_repeat_actions,
                                alpha_min=cfg.alpha_min, alpha_max=cfg.alpha_max, max_grad_norm=cfg.max_grad_norm,
                                calibrated=cfg.calibrated, device="cuda", update_noise="torch").to("cuda")
    algo.policy.is_within_training_step = True
    return (actor, c1, c2), algo


def _draws(seed, B, R, A, lo, hi):
    """The five random tensors of one update as HipCQL draws them: the reference's order and calls."""
    torch.manual_seed(seed)
    n1, n2 = torch.randn(B, A), torch.randn(B, A)
    ra = torch.FloatTensor(B * R, A).uniform_(-lo, hi)
    return dict(noise_actor=n1, noise_next=n2, random_act=ra, noise_rep_cur=torch.randn(B * R, A), noise_rep_next=torch.randn(B * R, A))


def test_hip_cql_update_against_the_oracle():
    """HipCQL.update() (make_hip_cql over tests/standin_cql.py) on a host buffer with calibration_returns, update_noise="torch":
    two updates against the oracle fed the same rows and the same draws -- CQLTrainingStats (rtol 2e-5 / atol 2e-6), the written-back
    networks and lagged networks (rtol 1e-5 / atol 0.02 lr), cql_log_alpha and its optimizer state."""
    from tests import standin_cql as SC

    g, d, cfg = CC.load_cql("calibrated")
    mods, algo = _make_algo(SC, d, cfg)
    assert type(algo).__name__ == "HipCQL" and isinstance(algo, SC.CQL)
    buf = _host_buffer(SC, g, d)
    st = OC.CQLState.create(*OS.init_sac_params(d["obs_dim"], d["act_dim"], d["seed"], d["hidden"]), cfg)
    B, R, A = d["batch"], d["R"], d["act_dim"]
    for u in range(2):
        torch.manual_seed(100 + u)
        stat = algo.update(buf, B)
        idx = algo._hip_idx.cpu().numpy()
        assert type(stat).__name__ == "CQLTrainingStats"
        ref = OC.update_with_batch(st, cfg, obs=g["obs"][idx], act=g["act"][idx], rew=g["rew"][idx].astype(np.float32),
                                   done=g["done"][idx].astype(np.float32), obs_next=g["obs_next"][idx],
                                   calib=g["calibration_returns"][idx].astype(np.float32),
                                   **_draws(100 + u, B, R, A, d["min_action"], d["max_action"]))
        got = [stat.actor_loss, stat.critic1_loss, stat.critic2_loss, stat.alpha, stat.alpha_loss, stat.cql_alpha, stat.cql_alpha_loss]
        print(u, got, CC.stats_vector(ref))
        np.testing.assert_allclose(got, CC.stats_vector(ref), rtol=2e-5, atol=2e-6)
        pairs = (("actor", mods[0]), ("critic1", mods[1]), ("critic2", mods[2]), ("critic1_old", algo.critic_old.module),
                 ("critic2_old", algo.critic2_old.module))
        for name, mod in pairs:
            flat = torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu().numpy()
            p = getattr(st.sac, name)
            lr = cfg.actor_lr if name == "actor" else cfg.critic_lr
            np.testing.assert_allclose(flat, OS.flatten(p, OS.order_of(p)).numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=name)
        leaf = algo._hip_cql_leaf()
        np.testing.assert_allclose(float(leaf.detach()), float(st.cql_log_alpha), rtol=2e-5, atol=1e-7)
        cs = algo.cql_alpha_optim.state[leaf]
        assert float(cs["step"]) == u + 1
        np.testing.assert_allclose(float(cs["exp_avg"]), float(st.opt_cql_alpha.m["a"]), rtol=1e-4)
    assert all(float(algo.policy_optim._optim.state[p]["step"]) == 2.0 for p in mods[0].parameters())


def test_hip_cql_resumes_from_its_state_dict():
    """state_dict() after two updates holds cql_log_alpha and cql_alpha_optim's state; a second instance (other initial networks)
    that loads it builds an engine that computes the next update bit for bit as the uninterrupted run."""
    import copy

    from tests import standin_cql as SC

    g, d, cfg = CC.load_cql("calibrated")
    buf = _host_buffer(SC, g, d)
    mods_a, a = _make_algo(SC, d, cfg, auto_alpha=False)          # (AutoAlpha's optimizer is outside the reference's state_dict())
    B = d["batch"]

    def step(algo, u):
        torch.manual_seed(200 + u)
        batch = algo._preprocess_batch(SC.Batch(), buf, g[f"u{u}_indices"])
        return algo._update_with_batch(batch)

    for u in range(2):
        step(a, u)
    state = copy.deepcopy(a.state_dict())
    extra = state[a._HIP_STATE_KEY]
    assert float(extra["cql_log_alpha"]) != 0.0 and float(extra["cql_log_alpha"]) == float(a._hip_cql_leaf().detach())
    assert float(list(extra["optim"]["state"].values())[0]["step"]) == 2.0
    mods_b, b = _make_algo(SC, d, cfg, seed=77, auto_alpha=False)
    b.load_state_dict(state)
    leaf_b = b._hip_cql_leaf()
    assert float(leaf_b.detach()) == float(extra["cql_log_alpha"])
    assert float(b.cql_alpha_optim.state[leaf_b]["exp_avg"]) == float(a.cql_alpha_optim.state[a._hip_cql_leaf()]["exp_avg"])
    sa_, sb_ = step(a, 2), step(b, 2)
    assert b._hip_engine.adam_step == a._hip_engine.adam_step == 3
    for f in ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "cql_alpha", "cql_alpha_loss"):
        assert getattr(sa_, f) == getattr(sb_, f), f
    for ma, mb in zip(mods_a + (a.critic_old.module, a.critic2_old.module), mods_b + (b.critic_old.module, b.critic2_old.module)):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb)
    assert torch.equal(a._hip_cql_leaf().detach(), b._hip_cql_leaf().detach())
    assert torch.equal(a._hip_engine._cql3, b._hip_engine._cql3)
