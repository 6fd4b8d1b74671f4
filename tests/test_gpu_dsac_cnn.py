"""GPU parity of DiscreteSAC on the Atari trunk -- through the C ABI (tianshou_amd.dsac_cnn), against the torch restatement of
the reference (tests/oracle_dsac_cnn.py, pinned to the unmodified reference by tests/golden/dsac_cnn_*.npz in
test_oracle_dsac_cnn.py) and through the HipDiscreteSACCnn drop-in over tests/standin_dsac_cnn.py.
Tolerances: tests/dsac_cnn_common.py (those of test_gpu_bcq.py / crr_common.py for the same kinds of quantity)."""
import copy

import numpy as np
import pytest
import torch

from tests import dsac_cnn_common as DC
from tests import oracle_dsac_cnn as OS

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def l2_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30)


def _nhwc(a):
    return torch.as_tensor(a).permute(0, 2, 3, 1).contiguous().cuda()


def _flat_cat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


def _sac_config(ocfg):
    from tianshou_amd.sac import SACConfig

    return SACConfig(gamma=ocfg.gamma, tau=ocfg.tau, n_step=ocfg.n_step, alpha=ocfg.alpha, auto_alpha=ocfg.auto_alpha,
                     target_entropy=ocfg.target_entropy, log_alpha0=ocfg.log_alpha0, actor_lr=ocfg.actor_lr,
                     critic_lr=ocfg.critic_lr, alpha_lr=ocfg.alpha_lr, betas=ocfg.betas, adam_eps=ocfg.adam_eps)


def _engine(c, h, w, A, H, seed, ocfg):
    from tianshou_amd import dsac_cnn as DS

    p = OS.init_params(c, h, w, A, H, seed)
    eng = DS.DiscreteSACCnnEngine(c, h, w, A, H, DS.flat_from_torch([p[k] for k in OS.PARAM_ORDER], c, h, w, A, H), _sac_config(ocfg))
    return p, eng


def _frames(rng, n, c, h, w):
    """The fixtures' kind of frames: a quarter of the pixels set (tools/gen_golden_dsac_cnn.py on why)."""
    f = rng.integers(0, 256, size=(n, c, h, w), dtype=np.uint8)
    return np.where(rng.random(f.shape) < 0.25, f, 0).astype(np.uint8)


def _layer_parts(lay, H, ld):
    """name -> (start, end) of every weight matrix and bias of one gradient set (trunk | own head)."""
    off, F, T = lay["off"], lay["F"], lay["T"]
    parts = {"conv1": (off[0], off[1]), "conv2": (off[1], off[2]), "conv3": (off[2], off[3]), "Wfc": (off[3], off[3] + F * H),
             "bfc": (off[3] + F * H, T), "Whead": (T, T + H * ld), "bhead": (T + H * ld, T + (H + 1) * ld)}
    return {k: (int(a), int(b)) for k, (a, b) in parts.items()}


def test_layout_and_flat_round_trip():
    from tianshou_amd import dsac_cnn as DS

    c, h, w, A, H = 2, 44, 36, 6, 64
    lay = DS.layout(c, h, w, A, H)
    assert lay["F"] == 128 and lay["ld"] == 32 and lay["Hd"] == 65 * 32
    assert lay["total"] == DS.param_count(c, h, w, A, H) == lay["T"] + 3 * lay["Hd"]
    assert list(lay["off"][4:]) == [lay["T"] + k * lay["Hd"] for k in range(4)]
    p = OS.init_params(c, h, w, A, H, 3)
    for order in (OS.PARAM_ORDER, OS.LAGGED_ORDER, OS.set_order("critic2")):
        t = [p[k] for k in order]
        flat = DS.flat_from_torch(t, c, h, w, A, H)
        assert flat.numel() == lay["T"] + (len(order) - 8) // 2 * lay["Hd"]
        back = DS.flat_to_torch(flat, c, h, w, A, H)
        assert len(back) == len(t) and all(torch.equal(x.cpu(), y) for x, y in zip(back, t))
    for bad in (dict(n_act=0), dict(n_act=65), dict(hidden=48), dict(hidden=2048), dict(h=20)):
        kw = dict(c=c, h=h, w=w, n_act=A, hidden=H)
        kw.update(bad)
        with pytest.raises(ValueError):
            DS.param_count(**kw)


@pytest.mark.parametrize("H", [512, 64])
@pytest.mark.parametrize("A,B", [(6, 64), (3, 24), (2, 5)])
def test_three_gradients_and_one_update_vs_oracle(A, B, H):
    """Gradient-only mode: the three gradients -- critic 1, critic 2, actor, each over the trunk and its own head, all at the
    unchanged parameters -- layer by layer against the CPU oracle's autograd; reruns bit-identical, no state touched.  Then the
    policy pass and the target with a lagged vector perturbed away from the live one, and ONE applied update: parameters after
    three chained Adam steps, the three moment sets, the lagged vector, log alpha."""
    from tianshou_amd import dsac_cnn as DS

    c, h, w = 2, 44, 36
    rng = np.random.default_rng(11 + A)
    auto = A != 3
    ocfg = OS.DSACConfig(gamma=0.9, tau=0.05, alpha=0.1, auto_alpha=auto, target_entropy=0.98 * float(np.log(A)), log_alpha0=-0.7,
                         actor_lr=3e-4, critic_lr=1e-4, alpha_lr=1e-3)
    p, eng = _engine(c, h, w, A, H, seed=5, ocfg=ocfg)
    st = OS.make_state(p, ocfg)
    gen = torch.Generator().manual_seed(0)
    st.params_old = {k: p[k] + 0.02 * torch.randn(p[k].shape, generator=gen) for k in OS.LAGGED_ORDER}
    eng.params_old = DS.flat_from_torch([st.params_old[k] for k in OS.LAGGED_ORDER], c, h, w, A, H)
    obs, obs_next = _frames(rng, B, c, h, w), _frames(rng, B, c, h, w)
    act = rng.integers(0, A, size=B)
    act[0], act[-1] = 0, A - 1
    weight = None if A == 6 else (0.25 + rng.random(B)).astype(np.float32)

    # the policy pass and the target value
    lg_ref = OS.policy_logits(p, obs)
    lg = eng.policy_forward(_nhwc(obs))
    assert tuple(lg.shape) == (B, A) and rel_err(lg.cpu(), lg_ref) < 1e-5
    tq_ref = OS.target_q(st, ocfg, obs_next)
    tq = eng.target_q(_nhwc(obs_next))
    print("target_q", rel_err(tq.cpu(), tq_ref))
    assert rel_err(tq.cpu(), tq_ref) < 1e-5
    assert torch.equal(eng.target_q(_nhwc(obs_next)), tq)
    ret = (0.3 * rng.normal(size=B) + 0.9 * tq_ref.numpy()).astype(np.float32)

    # gradient only
    col: dict = {}
    stats_ref, w_ref = OS.update_with_batch(st, ocfg, obs, act, ret, weight, collect=col, apply=False)
    lay = DS.layout(c, h, w, A, H)
    ld, G = lay["ld"], eng.G
    grads = torch.full((3, G), 7.0, dtype=torch.float32, device="cuda")      # pre-filled: every element must be written
    names = ("params", "params_old", "adam_m", "adam_v", "log_alpha", "log_alpha_m", "log_alpha_v")
    snap = [getattr(eng, n).clone() for n in names]
    stats, w_out = eng.update_with_batch(_nhwc(obs), act, ret, weight, grads_out=grads, apply=False)
    grads_b = torch.empty_like(grads)
    stats_b, w_b = eng.update_with_batch(_nhwc(obs), act, ret, weight, grads_out=grads_b, apply=False)
    assert torch.equal(stats, stats_b) and torch.equal(grads, grads_b) and torch.equal(w_out, w_b)      # bit-identical reruns
    assert all(torch.equal(a, getattr(eng, n)) for a, n in zip(snap, names)) and eng.adam_step == 0
    got = stats.cpu().tolist()
    print("stats", got, stats_ref)
    for i, name in enumerate(OS.STAT_NAMES[:4]):
        assert abs(got[i] - stats_ref[name]) <= 1e-5 * abs(stats_ref[name]), (name, got[i], stats_ref[name])
    assert abs(got[4] - stats_ref["alpha_loss"]) <= 1e-5 * abs(stats_ref["alpha_loss"]) + DC.ALPHA_LOSS_ATOL
    np.testing.assert_allclose(w_out.cpu().numpy(), w_ref.numpy(), rtol=1e-5, atol=DC.WEIGHT_ATOL)
    gc = grads.cpu()
    parts = _layer_parts(lay, H, ld)
    for k, which in enumerate(OS.SETS):
        g_ref = DS.flat_from_torch([col["grads"][which][n] for n in OS.set_order(which)], c, h, w, A, H, device="cpu")
        errs = {n: (rel_err(gc[k, a:b], g_ref[a:b]), l2_err(gc[k, a:b], g_ref[a:b])) for n, (a, b) in parts.items()}
        print(which, "gradient (max, L2)", errs)
        for n, (e_max, e_l2) in errs.items():
            assert e_max < 1e-5 and e_l2 < 1e-5, (which, n, e_max, e_l2)
        assert float(gc[k, lay["T"]:].reshape(H + 1, ld)[:, A:].abs().max()) == 0.0      # head padding: exact zeros
    # the three sets differ in the trunk: three optimizers see three different trunk gradients
    assert not torch.equal(gc[0, :lay["T"]], gc[1, :lay["T"]]) and not torch.equal(gc[0, :lay["T"]], gc[2, :lay["T"]])

    # one applied update against the oracle's
    stats_ref, w_ref = OS.update_with_batch(st, ocfg, obs, act, ret, weight)
    stats2, w2 = eng.update_with_batch(_nhwc(obs), act, ret, weight)
    assert eng.adam_step == 1
    assert torch.equal(stats2[1:2], stats[1:2])                            # critic 1 starts from the same parameters
    got = stats2.cpu().tolist()
    print("stats after the applied update", got, stats_ref)
    for i, name in enumerate(OS.STAT_NAMES[:4]):
        assert abs(got[i] - stats_ref[name]) <= 1e-5 * abs(stats_ref[name]), (name, got[i], stats_ref[name])
    np.testing.assert_allclose(w2.cpu().numpy(), w_ref.numpy(), rtol=1e-5, atol=DC.WEIGHT_ATOL)
    # critic 2 and the actor have seen the moved trunk: their losses differ from the gradient-only call's
    assert got[2] != stats.cpu().tolist()[2] and got[0] != stats.cpu().tolist()[0]
    lr = DC.lr_of(ocfg)
    new = _flat_cat(DS.flat_to_torch(eng.params, c, h, w, A, H))
    ref = _flat_cat([st.params[k] for k in OS.PARAM_ORDER])
    DC.check_first_step(new, ref, lr, "parameters after one update")
    DC.check_first_step(_flat_cat(DS.flat_to_torch(eng.params_old, c, h, w, A, H)), _flat_cat([st.params_old[k] for k in OS.LAGGED_ORDER]),
                        lr, "lagged vector after one update")
    for i in range(4, 7):                       # head padding: exact zeros in the parameters after the step
        assert float(eng.params[lay["off"][i]:lay["off"][i + 1]].reshape(H + 1, ld)[:, A:].abs().max()) == 0.0
    for k, which in enumerate(OS.SETS):
        m = _flat_cat(DS.flat_to_torch(eng.adam_m[k], c, h, w, A, H))
        v = _flat_cat(DS.flat_to_torch(eng.adam_v[k], c, h, w, A, H))
        m_ref = _flat_cat(list(st.moments(which, "exp_avg").values()))
        v_ref = _flat_cat(list(st.moments(which, "exp_avg_sq").values()))
        assert np.abs(m - m_ref).max() <= 1e-5 * np.abs(m_ref).max() and np.abs(v - v_ref).max() <= 2e-5 * np.abs(v_ref).max(), which
        assert float(eng.adam_m[k, lay["T"]:].reshape(H + 1, ld)[:, A:].abs().max()) == 0.0
    if auto:
        np.testing.assert_allclose(float(eng.log_alpha), float(st.log_alpha.detach()), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(float(eng.alpha), stats_ref["alpha"], rtol=1e-5)
    else:
        assert float(eng.log_alpha) == float(np.float32(ocfg.log_alpha0)) and got[3] == pytest.approx(0.1) and got[4] == 0.0


@pytest.mark.parametrize("tag", DC.TAGS)
def test_update_sequence_matches_reference_golden(tag):
    """Replays the reference's DiscreteSAC.update() sequence (sampled indices and importance weights from the fixture) on the
    engine over a DeviceReplayBuffer: n-step returns, the five statistics, batch.weight, parameters, the lagged vector against
    BOTH lagged modules, log alpha, and at the end ALL THREE optimizers' moments.  An engine with one moment set, or one that
    reused one trunk pass for the three steps, fails here."""
    from tianshou_amd import dqn as D
    from tianshou_amd import dsac_cnn as DS
    from tianshou_amd.buffer import DeviceReplayBuffer

    g, d, ocfg, _ = DC.load(tag)
    c, h, w, A, H = d["c"], d["h"], d["w"], d["n_act"], d["hidden"]
    _, eng = _engine(c, h, w, A, H, d["seed"], ocfg)
    buf = DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                             insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"], truncated=g["truncated"])
    frames, frames_next = torch.as_tensor(g["frames"]).cuda(), torch.as_tensor(g["frames_next"]).cuda()
    act_all = torch.as_tensor(g["act"]).cuda()
    lr, T, Hd = DC.lr_of(ocfg), eng.T, eng.Hd
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        ret = eng.preprocess(buf, frames, idx, 1, obs_next_frames=frames_next)
        assert tuple(ret.shape) == (d["batch"],)
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        obs = D.gather_obs_nhwc(frames, buf, idx, 1, as_u8=True)
        stats, w_out = eng.update_with_batch(obs, act_all[idx], ret, DC.is_weight(g, d, u))
        side = torch.cuda.Stream()                       # a second stream behind the "TD ready" event reads the finished weights
        eng.wait_td(side)
        with torch.cuda.stream(side):
            w_side = w_out.clone()
        side.synchronize()
        assert torch.equal(w_side, w_out)
        DC.check_stats(stats.cpu().tolist(), g, u, ocfg, A)
        DC.check_weight(w_out.cpu().numpy(), g, u)
        live = DS.flat_to_torch(eng.params, c, h, w, A, H)
        DC.check_params(_flat_cat(live)[::DC.STRIDE], g[f"u{u}_params_strided"], DC.PARAM_DEV[tag][u], lr, f"{tag} u{u} parameters")
        DC.check_params(_flat_cat(live[1::2]), g[f"u{u}_biases"], DC.PARAM_DEV[tag][u], lr, f"{tag} u{u} biases")
        for name, a in (("critic_old", T), ("critic2_old", T + Hd)):                       # each: the ONE lagged trunk + own head
            own = DS.flat_to_torch(torch.cat([eng.params_old[:T], eng.params_old[a:a + Hd]]), c, h, w, A, H)
            DC.check_params(_flat_cat(own)[::DC.STRIDE], g[f"u{u}_{name}_strided"], DC.LAGGED_DEV[tag][u], lr, f"{tag} u{u} {name}")
        if ocfg.auto_alpha:
            np.testing.assert_allclose(float(eng.log_alpha), float(g[f"u{u}_log_alpha"]), rtol=1e-5, atol=1e-7)
    assert eng.adam_step == int(g["adam_step"])
    for k, which in enumerate(OS.SETS):
        m = _flat_cat(DS.flat_to_torch(eng.adam_m[k], c, h, w, A, H))[::DC.STRIDE]
        v = _flat_cat(DS.flat_to_torch(eng.adam_v[k], c, h, w, A, H))[::DC.STRIDE]
        DC.check_moments(m, v, g, tag, which)
    if ocfg.auto_alpha:
        DC.check_alpha_moments(float(eng.log_alpha_m), float(eng.log_alpha_v), g)


# ---- hook level: HipDiscreteSACCnn over the stand-ins ------------------------------------------------------------------------
def _host_buffer(SD, g, d):
    """A plain host replay-buffer stand-in holding the fixture's buffer (whole [c, h, w] observations per slot)."""
    c, h, w, E, slots = d["c"], d["h"], d["w"], d["E"], d["slots"]
    buf = SD.VectorReplayBuffer(E * slots, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    buf.obs[:], buf.obs_next[:], buf.act[:], buf.rew[:] = g["frames"], g["frames_next"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    assert np.array_equal(buf._extend_offset, g["buf_offset"])
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
        buf._lengths[e] = g["buf_lengths"][e]
        buf.last_index[e] = g["buf_last_index"][e]
    return buf


def _make_algo(SD, d, ocfg, seed, **kw):
    from tianshou_amd.integration import make_hip_discrete_sac_cnn

    torch.manual_seed(seed)
    net = SD.DQNet(d["c"], d["h"], d["w"], action_shape=d["n_act"], features_only=True, output_dim_added_layer=d["hidden"])
    actor = SD.DiscreteActor(preprocess_net=net, action_shape=d["n_act"], softmax_output=False)
    critic1 = SD.DiscreteCritic(preprocess_net=net, last_size=d["n_act"])
    critic2 = SD.DiscreteCritic(preprocess_net=net, last_size=d["n_act"])
    alpha = SD.AutoAlpha(ocfg.target_entropy, ocfg.log_alpha0, ocfg.alpha_lr) if ocfg.auto_alpha else float(ocfg.alpha)
    algo = make_hip_discrete_sac_cnn(ref=SD)(policy=SD.DiscreteSACPolicy(actor=actor), critic=critic1, critic2=critic2,
                                             lr=ocfg.actor_lr, critic_lr=ocfg.critic_lr, tau=ocfg.tau, gamma=ocfg.gamma, alpha=alpha,
                                             n_step_return_horizon=ocfg.n_step, device="cuda", **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return algo


def _hook_step(SD, algo, buf, g, d, u):
    idx = g[f"u{u}_indices"]
    batch = SD.Batch(act=buf.act[idx])
    if d["prioritized"]:
        batch.weight = g[f"u{u}_is_weight"]
    batch = algo._preprocess_batch(batch, buf, idx)
    return batch, algo._update_with_batch(batch)


def _live14(algo):
    from tianshou_amd import dsac_cnn as DS

    named = dict(torch.nn.ModuleList([algo.policy, algo.critic, algo.critic2]).named_parameters())
    return [named[k] for k in DS.TIANSHOU_KEYS]


def _stat5(stat):
    return [stat.actor_loss, stat.critic1_loss, stat.critic2_loss, stat.alpha, stat.alpha_loss if stat.alpha_loss is not None else 0.0]


@pytest.mark.parametrize("tag", DC.TAGS)
def test_hip_discrete_sac_cnn_replays_reference_golden(tag):
    """Both fixtures through the drop-in, its hooks called with the fixture's indices (and importance weights) over a host
    buffer stand-in that stores whole stacks per slot: returns, statistics, batch.weight, and the written-back torch state --
    live parameters, both lagged modules (each with the one lagged trunk), the three optimizers' moments and steps, alpha."""
    from tests import standin_dsac_cnn as SD
    from tianshou_amd import dsac_cnn as DS

    g, d, ocfg, _ = DC.load(tag)
    algo = _make_algo(SD, d, ocfg, d["seed"])
    assert type(algo).__name__ == "HipDiscreteSACCnn"
    buf = _host_buffer(SD, g, d)
    lr = DC.lr_of(ocfg)
    set_keys = DS.TRUNK_KEYS + DS.HEAD_KEYS
    for u in range(d["n_updates"]):
        batch, stat = _hook_step(SD, algo, buf, g, d, u)
        assert tuple(batch.returns.shape) == (d["batch"], 1)
        np.testing.assert_allclose(batch.returns.cpu().numpy().reshape(-1), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        assert type(stat).__name__ == "DiscreteSACTrainingStats" and (stat.alpha_loss is None) == (not ocfg.auto_alpha)
        DC.check_stats(_stat5(stat), g, u, ocfg, d["n_act"])
        DC.check_weight(batch.weight.cpu().numpy(), g, u)
        live = [p.detach() for p in _live14(algo)]
        DC.check_params(_flat_cat(live)[::DC.STRIDE], g[f"u{u}_params_strided"], DC.PARAM_DEV[tag][u], lr, f"{tag} u{u} parameters")
        for name, mod in (("critic_old", algo.critic_old.module), ("critic2_old", algo.critic2_old.module)):
            named = dict(mod.named_parameters())
            DC.check_params(_flat_cat([named[k] for k in set_keys])[::DC.STRIDE], g[f"u{u}_{name}_strided"], DC.LAGGED_DEV[tag][u],
                            lr, f"{tag} u{u} {name}")
        if ocfg.auto_alpha:
            np.testing.assert_allclose(float(algo.alpha._log_alpha.detach()), float(g[f"u{u}_log_alpha"]), rtol=1e-5, atol=1e-7)
    assert algo.policy.actor.preprocess is algo.critic.preprocess is algo.critic2.preprocess
    live = _live14(algo)
    sets = {"critic1": (algo.critic_optim, live[:8] + live[10:12]), "critic2": (algo.critic2_optim, live[:8] + live[12:14]),
            "actor": (algo.policy_optim, live[:10])}
    for which, (opt, own) in sets.items():
        st = opt._optim.state
        assert all(float(st[p]["step"]) == float(g["adam_step"]) for p in own)
        DC.check_moments(_flat_cat([st[p]["exp_avg"] for p in own])[::DC.STRIDE], _flat_cat([st[p]["exp_avg_sq"] for p in own])[::DC.STRIDE],
                         g, tag, which)
    if ocfg.auto_alpha:
        s = algo.alpha._optim.state[algo.alpha._log_alpha]
        DC.check_alpha_moments(float(s["exp_avg"]), float(s["exp_avg_sq"]), g)
        assert float(s["step"]) == float(g["alpha_adam"][2])


@pytest.mark.parametrize("tag", DC.TAGS)
def test_hip_discrete_sac_cnn_resumes_from_the_written_back_state(tag):
    """A second algorithm restored from state_dict() after update 0 computes update 1 as the first one does -- parameters, both
    lagged modules, three moment sets, alpha -- and a checkpoint whose two lagged trunks differ is refused by name."""
    from tests import standin_dsac_cnn as SD

    g, d, ocfg, _ = DC.load(tag)
    buf = _host_buffer(SD, g, d)
    a = _make_algo(SD, d, ocfg, 3, match_rng_stream=False)
    _hook_step(SD, a, buf, g, d, 0)
    state = copy.deepcopy(a.state_dict())                           # (state_dict() holds live tensors)
    assert "critic2_old.module.preprocess.net.1.weight" in state    # the reference's format: every module lists the trunk
    alpha_opt = copy.deepcopy(a.alpha._optim.state_dict()) if ocfg.auto_alpha else None
    batch_a, stat_a = _hook_step(SD, a, buf, g, d, 1)
    b = _make_algo(SD, d, ocfg, 4, match_rng_stream=False)
    b.load_state_dict(state)
    if ocfg.auto_alpha:             # AutoAlpha's optimizer lives outside Algorithm._optimizers (sac.py:193): restored by hand
        b.alpha._optim.load_state_dict(alpha_opt)
    batch_b, stat_b = _hook_step(SD, b, buf, g, d, 1)
    assert _stat5(stat_a) == _stat5(stat_b)
    assert torch.equal(batch_a.returns, batch_b.returns) and torch.equal(batch_a.weight, batch_b.weight)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    for oa, ob in zip(a._optimizers, b._optimizers):
        for sa, sb in zip(oa._optim.state.values(), ob._optim.state.values()):
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    bad = copy.deepcopy(state)
    bad["critic2_old.module.preprocess.net.1.bias"] = bad["critic2_old.module.preprocess.net.1.bias"] + 1.0
    e = _make_algo(SD, d, ocfg, 5, match_rng_stream=False)
    e.load_state_dict(bad)
    with pytest.raises(NotImplementedError, match="trunks of critic_old and critic2_old differ"):
        _hook_step(SD, e, buf, g, d, 1)


def test_hooks_on_last_frame_storage_equal_hooks_on_whole_stacks():
    """The second buffer layout: single [h, w] frames per slot, stacked `stack_num` times on the device, no stored obs_next.
    The same transitions stored as whole stacks (built on the host with the buffer's own index arithmetic) must give the very
    same returns, statistics and weights: the two layouts differ only in how the device gathers its observations."""
    from oracle import oracle as O
    from tests import standin as SI
    from tests import standin_dsac_cnn as SD

    c, h, w, A, H, E, T, B = 2, 44, 36, 4, 64, 3, 20, 16
    rng = np.random.default_rng(7)
    d = dict(c=c, h=h, w=w, n_act=A, hidden=H)
    ocfg = OS.DSACConfig(gamma=0.9, tau=0.05, n_step=2, alpha=0.1, actor_lr=3e-4, critic_lr=1e-4)
    single = SD.PrioritizedVectorReplayBuffer(E * T, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                              stack_num=c, alpha=0.6, beta=0.4)
    single._meta = SI._Meta(("obs", "act", "rew", "terminated", "truncated", "done"))       # ignore_obs_next=True
    frames = _frames(rng, (T + 5) * E, 1, h, w).reshape(T + 5, E, h, w)
    for t in range(T + 5):                                           # more steps than slots: every sub-buffer wraps
        term = rng.random(E) < 0.1
        single.add(SD.Batch(obs=frames[t], act=rng.integers(0, A, size=E), rew=rng.normal(size=E), terminated=term,
                            truncated=(rng.random(E) < 0.05) & ~term, obs_next=frames[t]))
    bs = O.BufferState(single._extend_offset, single.last_index, single._lengths, [sb._insertion_idx for sb in single.buffers],
                       single.rew, single.terminated, single.truncated)
    slots = np.arange(E * T)
    stack = [slots]
    for _ in range(c - 1):
        stack.append(bs.prev(stack[-1]))
    full_obs = np.stack([single.obs[i] for i in stack[::-1]], axis=1)                       # oldest frame first
    whole = SD.VectorReplayBuffer(E * T, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    whole.obs[:], whole.obs_next[:] = full_obs, full_obs[bs.next(slots)]
    for k in ("act", "rew", "terminated", "truncated", "done", "_lengths", "last_index"):
        getattr(whole, k)[:] = getattr(single, k)
    for sa, sb in zip(whole.buffers, single.buffers):
        sa._size, sa._insertion_idx = sb._size, sb._insertion_idx
    out = []
    for buf in (single, whole):
        algo = _make_algo(SD, d, ocfg, 9)
        torch.manual_seed(1)
        res = []
        for u in range(2):
            idx = np.random.default_rng(u).integers(0, E * T, size=B)
            batch = SD.Batch(act=buf.act[idx], weight=np.linspace(0.5, 1.0, B))
            batch = algo._preprocess_batch(batch, buf, idx)
            stat = algo._update_with_batch(batch)
            res.append((batch.returns.clone(), batch.weight.clone(), _stat5(stat)))
        out.append(res)
        assert algo._hip_stack == (c if buf is single else 1)
    for (r1, w1, s1), (r2, w2, s2) in zip(*out):
        assert torch.equal(r1, r2) and torch.equal(w1, w2) and s1 == s2
        assert float(r1.abs().max()) > 0 and all(np.isfinite(s1))


def test_argument_errors():
    from tianshou_amd import dsac_cnn as DS

    c, h, w, A, H = 2, 44, 36, 3, 64
    _, eng = _engine(c, h, w, A, H, 1, OS.DSACConfig())
    obs = torch.zeros((4, h, w, c), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="pass grads_out"):
        eng.update_with_batch(obs, [0] * 4, [0.0] * 4, apply=False)
    with pytest.raises(ValueError, match="batch sizes differ"):
        eng.update_with_batch(obs, [0] * 3, [0.0] * 4)
    with pytest.raises(ValueError, match="grads_out must be"):
        eng.update_with_batch(obs, [0] * 4, [0.0] * 4, grads_out=torch.zeros(5, device="cuda"), apply=False)
    with pytest.raises(ValueError, match="NHWC"):
        eng.policy_forward(torch.zeros((4, c, h, w), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        DS.DiscreteSACCnnEngine(c, h, w, A, H, torch.zeros(10, device="cuda"), eng.cfg)
    assert eng.adam_step == 0
