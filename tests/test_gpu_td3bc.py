"""GPU parity of TD3+BC (tianshou_amd.td3bc over ts_td3bc_update) against tests/oracle_td3bc.py, the restatement pinned to the
reference by tests/golden/td3bc_*.npz (tests/test_oracle_td3bc.py), and through the HipTD3BC drop-in over tests/standin_td3bc.py."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from oracle import oracle_sac as OS
from tests import oracle_td3bc as OB
from tests import td3bc_common as CC

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _batch(B, obs_dim, act_dim, max_action, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, obs_dim, generator=g), (torch.rand(B, act_dim, generator=g) * 2 - 1) * max_action,
            torch.randn(B, generator=g))


@pytest.mark.parametrize("obs_dim,act_dim,B,hidden", [(376, 17, 512, 256), (17, 6, 80, 128)])
def test_gradients_stats_and_lmbda_vs_oracle(obs_dim, act_dim, B, hidden):
    """Gradient only (actor_lr = critic_lr = -1): the actor's gradient layer by layer, both critics', the statistics and lmbda
    against the oracle at tests/test_gpu_td3.py's bars (rel_err < 2e-5 per tensor, statistics rtol 2e-5)."""
    from tianshou_amd import td3 as T

    cfg = OB.TD3BCConfig(max_action=1.5, actor_lr=-1.0, critic_lr=-1.0, tau=0.0, update_actor_freq=1, alpha=2.5)
    actor, c1, c2 = OS.init_td3_params(obs_dim, act_dim, 21, True, hidden)
    eng = CC.engine_from(actor, c1, c2, cfg)
    before = [t.clone() for t in (eng.actor, eng.critic1, eng.critic2, eng.actor_old)]
    obs, act, ret = _batch(B, obs_dim, act_dim, cfg.max_action, 3)
    st = OS.TD3State.create(actor, c1, c2, cfg)
    col: dict = {}
    # the oracle's critic step precedes its actor loss; a gradient-only engine leaves the critics alone, so the oracle's
    # optimizers must too: lr = 0 keeps every parameter bit for bit (p - 0 * m / denom)
    st.opt_c1.lr = st.opt_c2.lr = st.opt_actor.lr = 0.0
    ref = OB.update_with_batch(st, cfg, obs, act, ret, collect=col)
    pa, pc = eng.actor.numel(), eng.critic1.numel()
    grads = torch.zeros(2 * pc + pa, dtype=torch.float32, device="cuda")
    stats, w = eng.update_with_batch(obs, act, ret, grads_out=grads)
    for t, b in zip((eng.actor, eng.critic1, eng.critic2, eng.actor_old), before):
        assert torch.equal(t, b)
    s = stats.cpu().numpy()
    np.testing.assert_allclose(s, [ref["actor_loss"], ref["critic1_loss"], ref["critic2_loss"], ref["lmbda"]], rtol=2e-5)
    np.testing.assert_allclose(w.cpu().numpy(), ref["weight"].numpy(), rtol=1e-5, atol=1e-5)
    got = {"critic1": T.critic_flat_to_torch(grads[:pc], obs_dim, act_dim, eng.hidden),
           "critic2": T.critic_flat_to_torch(grads[pc:2 * pc], obs_dim, act_dim, eng.hidden),
           "actor": T.actor_flat_to_torch(grads[2 * pc:], obs_dim, act_dim, eng.hidden)}
    for name, tensors in got.items():
        order = OS.DET_ACTOR_ORDER if name == "actor" else OS.CRITIC_ORDER
        for t, key in zip(tensors, order):
            assert rel_err(t.cpu(), col[name + "_grads"][key]) < 2e-5, (name, key)


def _device_buffer(g):
    from tianshou_amd.buffer import DeviceReplayBuffer

    return DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                              insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"],
                              truncated=g["truncated"], obs=g["obs"], act=g["act"], obs_next=g["obs_next"])


@pytest.mark.parametrize("tag", CC.TAGS)
def test_update_matches_reference_golden(tag):
    """Both fixtures on the engine at tests/test_gpu_td3.py::test_update_matches_reference_golden's tolerances: returns,
    statistics, strided parameters and lagged networks; the embedding's padding stays zero; the new priorities at the bar that
    test family uses for batch.weight (rtol 1e-5 / atol 1e-5)."""
    from tianshou_amd import td3 as T
    from tianshou_amd import widths as W

    g, d, cfg, _ = CC.load_td3bc(tag)
    eng = CC.engine_from(*OS.init_td3_params(d["obs_dim"], d["act_dim"], d["seed"], True, d["hidden"]), cfg, d["activation"])
    sa, sc = OS.layer_sizes(d["hidden"])
    assert eng.depth == len(sa) == len(sc)
    buf = _device_buffer(g)
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        ret = eng.preprocess(buf, idx, g[f"u{u}_noise"])
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=2e-5)
        stats, w = eng.update_with_batch(buf.obs[idx], buf.act[idx], ret, CC.is_weight(g, u, d["prioritized"]))
        np.testing.assert_allclose(stats.cpu().numpy()[:3], g[f"u{u}_stats"], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(w.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=1e-5)
        for name in CC.NETS:
            conv = T.actor_flat_to_torch if name.startswith("actor") else T.critic_flat_to_torch
            sz = sa if name.startswith("actor") else sc
            full = conv(getattr(eng, name), d["obs_dim"], d["act_dim"], eng.hidden, depth=eng.depth)
            assert W.padding_is_zero_layers(full, sz), name
            flat = torch.cat([t.reshape(-1) for t in W.unpad_layers(full, sz)])
            lr = cfg.actor_lr if name.startswith("actor") else cfg.critic_lr
            np.testing.assert_allclose(flat.cpu().numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=0.02 * lr, err_msg=name)
    assert eng.cnt == d["n_updates"] and eng.actor_steps == int(g["adam_step_actor"])


def test_critic_phase_is_td3s_bit_for_bit():
    """The critic phase is shared code: a TD3Engine and a TD3BCEngine fed the same batches and returns for 3 updates hold
    torch.equal critic parameters, moments, priorities and critic losses; the actors differ."""
    from tianshou_amd import td3 as T

    obs_dim, act_dim, B = 7, 3, 80
    cfg = OB.TD3BCConfig(max_action=1.0, actor_lr=3e-4, critic_lr=1e-3, tau=0.01, update_actor_freq=1, alpha=2.5)
    p = OS.init_td3_params(obs_dim, act_dim, 8, True, 64)
    a, b = CC.engine_from(*p, cfg, cls=T.TD3Engine), CC.engine_from(*p, cfg)
    assert type(a) is T.TD3Engine and type(b).__name__ == "TD3BCEngine"
    for u in range(3):
        obs, act, ret = _batch(B, obs_dim, act_dim, cfg.max_action, 10 + u)
        wgt = torch.rand(B, generator=torch.Generator().manual_seed(u)) + 0.5
        sa_, wa_ = a.update_with_batch(obs, act, ret, wgt)
        sb_, wb_ = b.update_with_batch(obs, act, ret, wgt)
        assert torch.equal(wa_, wb_) and torch.equal(sa_[1:3], sb_[1:3]), u
        for n in ("critic1", "critic2"):
            for suffix in ("", "_m", "_v", "_old"):
                assert torch.equal(getattr(a, n + suffix), getattr(b, n + suffix)), (u, n + suffix)
        assert not torch.equal(a.actor, b.actor) and float(sa_[0]) != float(sb_[0])


def test_same_update_twice_gives_the_same_bits():
    """Determinism: the reductions take no atomics, so the same gradient-only update from the same state gives bit-identical
    grads_out and statistics (B = 1500: the loss kernel's workgroup 0 loops, three workgroups write d_q)."""
    obs_dim, act_dim, B = 7, 6, 1500
    cfg = OB.TD3BCConfig(max_action=1.5, actor_lr=-1.0, critic_lr=-1.0, tau=0.0, update_actor_freq=1, alpha=2.5)
    eng = CC.engine_from(*OS.init_td3_params(obs_dim, act_dim, 9, True, 64), cfg)
    obs, act, ret = _batch(B, obs_dim, act_dim, cfg.max_action, 5)
    n = 2 * eng.critic1.numel() + eng.actor.numel()
    outs = []
    for _ in range(2):
        grads = torch.zeros(n, dtype=torch.float32, device="cuda")
        stats, w = eng.update_with_batch(obs, act, ret, grads_out=grads)
        outs.append((grads.clone(), stats.clone(), w.clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_argument_errors():
    from tianshou_amd import _lib
    from tianshou_amd import td3bc as TB

    obs_dim, act_dim, B = 7, 3, 5
    cfg = OB.TD3BCConfig(actor_lr=-1.0, critic_lr=-1.0, tau=0.0)
    eng = CC.engine_from(*OS.init_td3_params(obs_dim, act_dim, 1, True, 64), cfg)
    obs, act, ret = _batch(B, obs_dim, act_dim, 1.0, 0)
    with pytest.raises(ValueError):
        TB.TD3BCConfig(twin=False)
    with pytest.raises(ValueError):
        eng.update_with_batch(obs, act[:, :-1], ret)
    for bad in (-1.0, float("nan"), float("inf")):
        eng.cfg.alpha = bad
        with pytest.raises(_lib.EngineError, match="bc_alpha") as e:
            eng.update_with_batch(obs, act, ret)
        assert e.value.code == _lib.TS_ERR_INVALID_ARG and "ts_td3bc_update" in str(e.value)
    assert eng.cnt == 0 and eng.actor_steps == 0                 # a refused call leaves the counters alone
    eng.cfg.alpha = 0.0
    stats, w = eng.update_with_batch(obs, act, ret)
    assert tuple(stats.shape) == (4,) and float(stats[3]) == 0.0 and tuple(w.shape) == (B,) and eng.cnt == 1


# ---- the drop-in class over the stand-ins -------------------------------------------------------------------------------------
def _host_buffer(SB, g, d):
    """A host replay-buffer stand-in holding the fixture's buffer: prioritized or plain, as the fixture was recorded."""
    E, slots = d["E"], d["slots"]
    kw = dict(obs_shape=(d["obs_dim"],), act_shape=(d["act_dim"],))
    buf = (SB.PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4, **kw) if d["prioritized"]
           else SB.VectorReplayBuffer(E * slots, E, **kw))
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated"):
        getattr(buf, k)[:] = g[k]
    buf.done[:] = g["terminated"] | g["truncated"]
    buf._lengths[:], buf.last_index[:] = g["buf_lengths"], g["buf_last_index"]
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
    return buf


def _make_algo(SB, d, cfg, seed=None):
    """HipTD3BC over the stand-ins on the fixture's networks: the seeded initial ones, or (seed given) other ones, to be overwritten
    by load_state_dict."""
    from tianshou_amd.integration import make_hip_td3bc

    sa, sc = OS.layer_sizes(d["hidden"])
    fn = nn.Tanh if d["activation"] == "tanh" else nn.ReLU
    obs_dim, act_dim = d["obs_dim"], d["act_dim"]
    actor = SB.ContinuousActorDeterministic(SB.Net(obs_dim, list(sa), fn), act_dim, max_action=cfg.max_action)
    c1, c2 = (SB.ContinuousCritic(SB.Net(obs_dim + act_dim, list(sc), fn)) for _ in range(2))
    p0 = OS.init_td3_params(obs_dim, act_dim, d["seed"] if seed is None else seed, True, (sa, sc))
    for mod, pd in ((actor, p0[0]), (c1, p0[1]), (c2, p0[2])):
        mod.load_state_dict(dict(zip(mod.state_dict(), pd.values())))
    algo = make_hip_td3bc(ref=SB)(policy=SB.Policy(actor), critic=c1, critic2=c2, lr=cfg.actor_lr, critic_lr=cfg.critic_lr,
                                  tau=cfg.tau, gamma=cfg.gamma, policy_noise=cfg.policy_noise,
                                  update_actor_freq=cfg.update_actor_freq, noise_clip=cfg.noise_clip, alpha=cfg.alpha,
                                  n_step_return_horizon=cfg.n_step, device="cuda").to("cuda")
    algo.policy.is_within_training_step = True
    return (actor, c1, c2), algo


def _hook_step(SB, algo, buf, g, d, u, monkeypatch):
    """The two hooks on the fixture's indices (and PER weights); the hooks' one torch.randn per update is served from the fixture."""
    idx = g[f"u{u}_indices"]
    batch = SB.Batch(act=buf.act[idx])
    if d["prioritized"]:
        batch.weight = g[f"u{u}_is_weight"]
    real_randn = torch.randn
    served = [torch.from_numpy(g[f"u{u}_noise"])]

    def randn(*a, **k):
        if not served or k.get("device") is not None:
            return real_randn(*a, **k)
        return served.pop(0).clone()

    monkeypatch.setattr(torch, "randn", randn)
    try:
        batch = algo._preprocess_batch(batch, buf, idx)
    finally:
        monkeypatch.setattr(torch, "randn", real_randn)
    assert not served
    return batch, algo._update_with_batch(batch)


def _modules(mods, algo):
    actor, c1, c2 = mods
    return (("actor", actor), ("critic1", c1), ("critic2", c2), ("actor_old", algo.actor_old.module),
            ("critic1_old", algo.critic_old.module), ("critic2_old", algo.critic2_old.module))


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_td3bc_update_replays_reference_golden(tag, monkeypatch):
    """Both fixtures through the drop-in: HipTD3BC (make_hip_td3bc over tests/standin_td3bc.py), its hooks called with the
    fixture's indices, noise (and PER weights) over a host buffer stand-in: returns, batch.weight, TD3TrainingStats, `_cnt` /
    `_last`, and the written-back torch networks, lagged networks and Adam state, at test_hip_td3_ddpg_hooks_replay_the_reference's
    tolerances."""
    from tests import standin_td3bc as SB

    g, d, cfg, _ = CC.load_td3bc(tag)
    mods, algo = _make_algo(SB, d, cfg)
    assert type(algo).__name__ == "HipTD3BC" and isinstance(algo, SB.TD3BC)
    buf = _host_buffer(SB, g, d)
    for u in range(d["n_updates"]):
        batch, stat = _hook_step(SB, algo, buf, g, d, u, monkeypatch)
        np.testing.assert_allclose(batch.returns.cpu().numpy().reshape(-1), g[f"u{u}_returns"], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(batch.weight.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=1e-5)
        assert type(stat).__name__ == "TD3TrainingStats"
        np.testing.assert_allclose([stat.actor_loss, stat.critic1_loss, stat.critic2_loss], g[f"u{u}_stats"], rtol=2e-5, atol=2e-6)
        assert algo._cnt == u + 1 and algo._last == stat.actor_loss
        for name, mod in _modules(mods, algo):
            flat = torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu().numpy()
            lr = cfg.actor_lr if name.startswith("actor") else cfg.critic_lr
            np.testing.assert_allclose(flat[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=0.02 * lr, err_msg=f"update {u}: {name}")
    for name, mod, optim in (("actor", mods[0], algo.policy_optim), ("critic1", mods[1], algo.critic_optim),
                             ("critic2", mods[2], algo.critic2_optim)):
        st = [optim._optim.state[p] for p in mod.parameters()]
        assert all(float(s["step"]) == float(g[f"adam_step_{name}"]) for s in st), name
        m = torch.cat([s["exp_avg"].reshape(-1) for s in st]).cpu().numpy()[::61]
        v = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).cpu().numpy()[::61]
        # the moments are sums of at most four gradients, so the gradient bar applies: 2e-5 of each vector's scale (m is linear in
        # the gradients; v is quadratic: twice the relative error, 4e-5 of its scale)
        m_ref, v_ref = g[f"adam_m_{name}"], g[f"adam_v_{name}"]
        print("adam moments", name, np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max())
        assert np.abs(m - m_ref).max() <= 2e-5 * np.abs(m_ref).max(), name
        assert np.abs(v - v_ref).max() <= 4e-5 * np.abs(v_ref).max(), name


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_td3bc_resumes_from_the_written_back_state(tag, monkeypatch):
    """A second instance built from the written-back torch state after update 2 (state_dict() + `_cnt`, which the reference keeps
    outside it) computes updates 3.. bit for bit as the uninterrupted run; `alpha` changed on the algorithm object reaches the
    engine at the next update."""
    from tests import standin_td3bc as SB

    g, d, cfg, _ = CC.load_td3bc(tag)
    buf = _host_buffer(SB, g, d)
    mods_a, a = _make_algo(SB, d, cfg)
    for u in range(2):
        _hook_step(SB, a, buf, g, d, u, monkeypatch)
    state = copy.deepcopy(a.state_dict())                           # (state_dict() holds live tensors)
    mods_b, b = _make_algo(SB, d, cfg, seed=77)
    b.load_state_dict(state)
    b._cnt, b._last = a._cnt, a._last
    for u in range(2, d["n_updates"]):
        batch_a, stat_a = _hook_step(SB, a, buf, g, d, u, monkeypatch)
        batch_b, stat_b = _hook_step(SB, b, buf, g, d, u, monkeypatch)
        assert (stat_a.actor_loss, stat_a.critic1_loss, stat_a.critic2_loss) == (stat_b.actor_loss, stat_b.critic1_loss, stat_b.critic2_loss)
        assert torch.equal(batch_a.weight, batch_b.weight) and torch.equal(batch_a.returns, batch_b.returns)
        for (name, ma), (_, mb) in zip(_modules(mods_a, a), _modules(mods_b, b)):
            for pa, pb in zip(ma.parameters(), mb.parameters()):
                assert torch.equal(pa, pb), (u, name)
    assert b._cnt == a._cnt == d["n_updates"]
    b.alpha = 0.0
    _hook_step(SB, b, buf, g, d, 0, monkeypatch)
    assert b._hip_engine.cfg.alpha == 0.0
    assert (b._cnt - 1) % cfg.update_actor_freq == 0 and float(b._hip_engine._stats[3]) == 0.0       # it stepped the actor: lmbda == 0
