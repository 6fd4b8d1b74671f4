"""GPU parity of DiscreteCRR on the Atari trunk -- through the C ABI (tianshou_amd.crr), against the torch restatement of the
reference (tests/oracle_crr.py, pinned to the unmodified reference by tests/golden/crr_*.npz in test_oracle_crr.py) and through
the HipDiscreteCRR drop-in over tests/standin_crr.py.
Tolerances are DiscreteBCQ's for the same quantities (test_gpu_bcq.py: the same trunk, the same GEMM kernels): 1e-5 relative on
losses and targets, 1e-5 of each gradient tensor's scale for its largest element and for the L2 norm of the difference,
rtol = 1e-5 with atol = 0.02 * lr on parameters after an update, 1e-5 / 2e-5 on the Adam moments -- except in the last update of
crr_exp.npz, where the float32 oracle itself leaves them against float64 and the bar is twice its deviation.
tests/crr_common.py states the measurements and the reasoning."""
import copy

import numpy as np
import pytest
import torch

from tests import crr_common as CC
from tests import oracle_crr as OC

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def l2_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30)


def _nhwc(a):
    return torch.as_tensor(a).permute(0, 2, 3, 1).contiguous().cuda()


def _engine(c, h, w, A, seed, **kw):
    from tianshou_amd import crr as CR

    p = OC.init_params(c, h, w, A, seed)
    eng = CR.CRREngine(c, h, w, A, CR.flat_from_torch([p[k] for k in OC.PARAM_ORDER], c, h, w, A), CR.CRRConfig(**kw))
    return p, eng


def _flat_cat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()


@pytest.mark.parametrize("mode", OC.MODES)
@pytest.mark.parametrize("A,B", [(6, 64), (3, 24), (1, 5)])
def test_batch_gradient_vs_oracle(A, B, mode):
    """The targets, the four losses and the gradient of the whole network of one minibatch, layer by layer -- both heads and
    the trunk that takes the sum of their feature gradients -- against the CPU oracle's autograd, with a lagged net that
    differs from the live one; then the Adam step."""
    from tianshou_amd import crr as CR

    c, h, w = 2, 44, 36
    rng = np.random.default_rng(9)
    kw = dict(lr=1e-4, policy_improvement_mode=mode, beta=0.5, ratio_upper_bound=1.5, min_q_weight=2.5, gamma=0.9,
              target_update_freq=10)
    p, eng = _engine(c, h, w, A, seed=4, **kw)
    ocfg = OC.CRRConfig(**kw)
    st = OC.make_state(p, ocfg)
    gen = torch.Generator().manual_seed(0)
    st.params_old = {k: p[k] + 0.02 * torch.randn(p[k].shape, generator=gen) for k in OC.PARAM_ORDER}
    eng.params_old = CR.flat_from_torch([st.params_old[k] for k in OC.PARAM_ORDER], c, h, w, A)
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    obs_next = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    rew = rng.normal(size=B).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.uint8) * rng.integers(1, 3, size=B).astype(np.uint8)
    col: dict = {}
    losses_ref = OC.update_with_batch(st, ocfg, obs, obs_next, act, rew, done, collect=col, apply=False)
    if mode == "exp" and A > 1:
        e = (col["adv"] / ocfg.beta).exp()
        assert (e > ocfg.ratio_upper_bound).any() and (e < ocfg.ratio_upper_bound).any()       # the clamp decides rows
    assert (done > 0).any() and (done == 0).any()

    lay = CR.layout(c, h, w, A)
    off, F, ld = lay["off"], lay["F"], lay["ld"]
    grad = torch.full((eng.P,), 7.0, dtype=torch.float32, device="cuda")   # pre-filled: every element must be written
    tgt = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    snap = [t.clone() for t in (eng.params, eng.params_old, eng.adam_m, eng.adam_v)]
    args = (_nhwc(obs), _nhwc(obs_next), act, rew, done)
    losses = eng.update_with_batch(*args, grad_out=grad, target_out=tgt, apply=False)
    grad_b = torch.empty_like(grad)
    losses_b = eng.update_with_batch(*args, grad_out=grad_b, apply=False)
    assert torch.equal(losses, losses_b) and torch.equal(grad, grad_b)     # bit-identical reruns
    assert all(torch.equal(a, b) for a, b in zip(snap, (eng.params, eng.params_old, eng.adam_m, eng.adam_v)))
    assert (eng.iter, eng.adam_step) == (0, 0)
    got = losses.cpu().tolist()
    print("losses", got, losses_ref, "targets", rel_err(tgt.cpu(), col["target"]))
    assert tuple(losses.shape) == (4,)
    assert rel_err(tgt.cpu(), col["target"]) < 1e-5
    for name, x, r in zip(CC.LOSS_NAMES, got, losses_ref):
        if A == 1 and name in ("actor_loss", "cql_loss"):
            assert abs(x) <= 1e-6 and abs(r) <= 1e-6                       # one action: log_softmax and lse(q) - qa are 0
        else:
            assert abs(x - r) <= 1e-5 * abs(r), (name, x, r)
    g_ref = CR.flat_from_torch([col["grads"][k] for k in OC.PARAM_ORDER], c, h, w, A, device="cpu")
    gc = grad.cpu()
    parts = {"conv1": (off[0], off[1]), "conv2": (off[1], off[2]), "conv3": (off[2], off[3])}
    for name, i in (("c", 3), ("a", 5)):                                   # the critic in the Q head's place, then the actor
        parts.update({f"W{name}1": (off[i], off[i] + F * 512), f"b{name}1": (off[i] + F * 512, off[i + 1]),
                      f"W{name}2": (off[i + 1], off[i + 1] + 512 * ld), f"b{name}2": (off[i + 1] + 512 * ld, off[i + 2])})
    errs = {k: (rel_err(gc[a:b], g_ref[a:b]), l2_err(gc[a:b], g_ref[a:b])) for k, (a, b) in parts.items()}
    print("gradient (max, L2)", errs)
    for k, (e_max, e_l2) in errs.items():
        if A == 1 and k.startswith(("Wa", "ba")):                          # one action: the actor's gradient is exactly 0
            assert float(gc[parts[k][0]:parts[k][1]].abs().max()) == 0.0 and float(g_ref[parts[k][0]:parts[k][1]].abs().max()) == 0.0
        else:
            assert e_max < 1e-5 and e_l2 < 1e-5, (k, e_max, e_l2)
    for i in (4, 6):                            # head padding: exact zeros in the gradient of both heads
        assert float(gc[off[i]:off[i + 1]].reshape(513, ld)[:, A:].abs().max()) == 0.0
    eng.cfg.target_update_freq = ocfg.target_update_freq = 10**6           # keep the perturbed lagged net through the step
    eng.iter = st.iter = 1
    OC.update_with_batch(st, ocfg, obs, obs_next, act, rew, done)
    losses2 = eng.update_with_batch(*args)
    assert torch.equal(losses2, losses) and (eng.iter, eng.adam_step) == (2, 1)
    for i in (4, 6):                            # ... and in the parameters after the step
        assert float(eng.params[off[i]:off[i + 1]].reshape(513, ld)[:, A:].abs().max()) == 0.0
    new = _flat_cat(CR.flat_to_torch(eng.params, c, h, w, A))
    ref = torch.cat([st.params[k].detach().reshape(-1) for k in OC.PARAM_ORDER]).numpy()
    diff = np.abs(new - ref)
    bad = diff > 1e-5 * np.abs(ref) + 0.02 * ocfg.lr
    print("adam", bad.mean(), diff.max())
    assert bad.mean() < 1e-4 and diff.max() <= 2 * ocfg.lr


def _check_adam_moments(m, v, g, tag):
    """Bars: tests/crr_common.moment_bars -- BCQ's 1e-5 / 2e-5 of each vector's scale, or twice the float32 oracle's own
    deviation from float64 where that is larger."""
    m_ref, v_ref = g["adam_m_strided"], g["adam_v_strided"]
    bar_m, bar_v = CC.moment_bars(tag)
    print("adam moments", np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max(), "bars", bar_m, bar_v)
    assert np.abs(m - m_ref).max() <= bar_m * np.abs(m_ref).max()
    assert np.abs(v - v_ref).max() <= bar_v * np.abs(v_ref).max()


def _check_losses(got4, g, u):
    print(f"u{u} losses", [float(x) for x in got4], [float(g[f"u{u}_{n}"]) for n in CC.LOSS_NAMES])
    for name, x in zip(CC.LOSS_NAMES, got4):
        np.testing.assert_allclose(float(x), float(g[f"u{u}_{name}"]), rtol=1e-5, err_msg=name)


def _check_params(tensors14, old14, g, u, lr, tag):
    CC.check_params(_flat_cat(tensors14)[::CC.STRIDE], g[f"u{u}_params_strided"], tag, u, lr)
    CC.check_params(_flat_cat([tensors14[i] for i in range(1, 14, 2)]), g[f"u{u}_biases"], tag, u, lr, "biases")
    if old14 is not None:
        for name, pos in (("actor_old", CC.ACTOR_OLD), ("critic_old", CC.CRITIC_OLD)):
            CC.check_params(_flat_cat([old14[i] for i in pos])[::CC.STRIDE], g[f"u{u}_{name}_strided"], tag, max(u - 1, 0), lr, name)   # the live net of an earlier update


def _engine_cfg(ocfg):
    return dict(gamma=ocfg.gamma, policy_improvement_mode=ocfg.policy_improvement_mode, beta=ocfg.beta,
                ratio_upper_bound=ocfg.ratio_upper_bound, min_q_weight=ocfg.min_q_weight,
                target_update_freq=ocfg.target_update_freq, lr=ocfg.lr)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_update_sequence_matches_reference_golden(tag):
    """Replays the reference's DiscreteCRR.update() sequence (sampled indices from the fixture) on the engine: the targets,
    the four losses, parameters, biases and lagged parameters after every update, the Adam moments at the end."""
    from tianshou_amd import crr as CR

    g, d, ocfg, _ = CC.load_crr(tag)
    c, h, w, A = d["c"], d["h"], d["w"], d["n_act"]
    _, eng = _engine(c, h, w, A, seed=d["seed"], **_engine_cfg(ocfg))
    lagged = ocfg.target_update_freq > 0
    assert lagged or eng.params_old is eng.params
    for u in range(d["n_updates"]):
        obs, obs_next, act, rew, done = CC.batch_of(g, u)
        tgt = torch.empty(d["batch"], dtype=torch.float32, device="cuda")
        losses = eng.update_with_batch(_nhwc(obs), _nhwc(obs_next), act, rew, done, target_out=tgt)
        print(f"u{u} targets", rel_err(tgt.cpu(), g[f"u{u}_target"]))
        np.testing.assert_allclose(tgt.cpu().numpy(), g[f"u{u}_target"], rtol=1e-5, atol=1e-5 * np.abs(g[f"u{u}_target"]).max())
        _check_losses(losses.cpu().tolist(), g, u)
        _check_params(CR.flat_to_torch(eng.params, c, h, w, A), CR.flat_to_torch(eng.params_old, c, h, w, A) if lagged else None,
                      g, u, ocfg.lr, tag)
    assert eng.adam_step == int(g["adam_step"]) and eng.iter == d["n_updates"]
    m = _flat_cat(CR.flat_to_torch(eng.adam_m, c, h, w, A))
    v = _flat_cat(CR.flat_to_torch(eng.adam_v, c, h, w, A))
    _check_adam_moments(m[::CC.STRIDE], v[::CC.STRIDE], g, tag)


def _host_buffer(SC, g, d):
    """A plain host replay-buffer stand-in holding the fixture's buffer."""
    c, h, w, E, slots = d["c"], d["h"], d["w"], d["E"], d["slots"]
    buf = SC.VectorReplayBuffer(E * slots, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    buf.obs[:], buf.obs_next[:], buf.act[:], buf.rew[:] = g["frames"], g["frames_next"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    assert np.array_equal(buf._extend_offset, g["buf_offset"])
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
        buf._lengths[e] = g["buf_lengths"][e]
        buf.last_index[e] = g["buf_last_index"][e]
    return buf


def _make_algo(SC, d, ocfg, seed, **kw):
    from tianshou_amd.integration import make_hip_discrete_crr

    torch.manual_seed(seed)
    trunk = SC.DQNetFeaturesOnly(d["c"], d["h"], d["w"])
    actor = SC.DiscreteActor(preprocess_net=trunk, action_shape=d["n_act"], hidden_sizes=[512], softmax_output=False)
    critic = SC.DiscreteCritic(preprocess_net=trunk, hidden_sizes=[512], last_size=d["n_act"])
    algo = make_hip_discrete_crr(ref=SC)(policy=SC.DiscreteActorPolicy(actor=actor), critic=critic, lr=ocfg.lr, gamma=ocfg.gamma,
                                         policy_improvement_mode=ocfg.policy_improvement_mode,
                                         ratio_upper_bound=ocfg.ratio_upper_bound, beta=ocfg.beta, min_q_weight=ocfg.min_q_weight,
                                         target_update_freq=ocfg.target_update_freq, device="cuda", **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return algo


def _hook_step(SC, algo, buf, g, u):
    idx = g[f"u{u}_indices"]
    batch = algo._preprocess_batch(SC.Batch(act=buf.act[idx]), buf, idx)
    return batch, algo._update_with_batch(batch)


def _named14(algo):
    from tianshou_amd import crr as CR

    named = dict(torch.nn.ModuleList([algo.policy, algo.critic]).named_parameters())
    return [named[k] for k in CR.TIANSHOU_KEYS]


def _old14(algo):
    """The lagged tensors in TIANSHOU_KEYS order, with critic_old's own trunk checked against actor_old's."""
    a = list(algo.actor_old.module.parameters())
    c = list(algo.critic_old.module.parameters())
    assert all(torch.equal(x, y) for x, y in zip(a[:6], c[:6]))
    return [p.detach() for p in a + c[6:]]


def _stats4(s):
    return (s.loss, s.actor_loss, s.critic_loss, s.cql_loss)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_discrete_crr_update_replays_reference_golden(tag):
    """Both fixtures through the drop-in: HipDiscreteCRR (make_hip_discrete_crr over tests/standin_crr.py), its hooks called
    with the fixture's indices over a host buffer stand-in holding the fixture's buffer: the four statistics, and the
    written-back torch parameters (the shared trunk once), both lagged modules and the Adam state."""
    from tests import standin_crr as SC

    g, d, ocfg, _ = CC.load_crr(tag)
    algo = _make_algo(SC, d, ocfg, d["seed"])
    assert type(algo).__name__ == "HipDiscreteCRR"
    buf = _host_buffer(SC, g, d)
    lagged = ocfg.target_update_freq > 0
    for u in range(d["n_updates"]):
        batch, stat = _hook_step(SC, algo, buf, g, u)
        assert not hasattr(batch, "weight") and len(batch.returns) == d["batch"]
        assert type(stat).__name__ == "DiscreteCRRTrainingStats"
        _check_losses(_stats4(stat), g, u)
        _check_params([p.detach() for p in _named14(algo)], _old14(algo) if lagged else None, g, u, ocfg.lr, tag)
    assert algo._iter == d["n_updates"] and algo.base_preprocess_calls == d["n_updates"]
    assert algo.policy.actor.preprocess is algo.critic.preprocess
    st = algo.optim._optim.state
    params = _named14(algo)
    assert all(float(st[p]["step"]) == float(g["adam_step"]) for p in params)
    m = _flat_cat([st[p]["exp_avg"] for p in params])
    v = _flat_cat([st[p]["exp_avg_sq"] for p in params])
    _check_adam_moments(m[::CC.STRIDE], v[::CC.STRIDE], g, tag)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_discrete_crr_resumes_from_the_written_back_state(tag):
    """A second algorithm restored from state_dict() after update 0 computes update 1 as the first one does; the scalars
    changed on the algorithm object between two updates reach the engine."""
    from tests import standin_crr as SC

    g, d, ocfg, _ = CC.load_crr(tag)
    buf = _host_buffer(SC, g, d)
    a = _make_algo(SC, d, ocfg, 3)
    _hook_step(SC, a, buf, g, 0)
    state = copy.deepcopy(a.state_dict())                           # (state_dict() holds live tensors)
    _, stat_a = _hook_step(SC, a, buf, g, 1)
    b = _make_algo(SC, d, ocfg, 4)
    b.load_state_dict(state)
    b._iter = 1                                                     # the reference keeps `_iter` outside state_dict() too
    _, stat_b = _hook_step(SC, b, buf, g, 1)
    assert _stats4(stat_a) == _stats4(stat_b)
    for pa, pb in zip(a.parameters(), b.parameters()):              # live and lagged modules alike
        assert torch.equal(pa, pb)
    b._min_q_weight, b._beta, b._ratio_upper_bound = 2.0 * ocfg.min_q_weight + 0.25, 2.0 * ocfg.beta, 3.0
    b._policy_improvement_mode = "all"
    b.discounted_return_computation.gamma = 0.5
    _, stat_c = _hook_step(SC, b, buf, g, 2)
    cfg = b._hip_engine.cfg
    assert (cfg.min_q_weight, cfg.beta, cfg.ratio_upper_bound, cfg.policy_improvement_mode, cfg.gamma) == \
        (b._min_q_weight, b._beta, 3.0, "all", 0.5)
    np.testing.assert_allclose(stat_c.loss, stat_c.actor_loss + stat_c.critic_loss + b._min_q_weight * stat_c.cql_loss, rtol=1e-6)


@pytest.mark.parametrize("mode", OC.MODES)
def test_live_networks_as_targets_equal_a_lagged_copy_of_them(mode):
    """params_old == params (target_update_freq == 0) gives the result of a lagged copy equal to the live vector, bit for
    bit: targets, losses, gradient, and the parameters after the step (the target is complete before Adam writes)."""
    c, h, w, A, B = 2, 44, 36, 3, 24
    rng = np.random.default_rng(2)
    kw = dict(lr=1e-3, policy_improvement_mode=mode, beta=0.05, ratio_upper_bound=1.5, min_q_weight=2.5)
    _, live = _engine(c, h, w, A, seed=6, target_update_freq=0, **kw)
    _, copy_ = _engine(c, h, w, A, seed=6, target_update_freq=1000, **kw)
    assert live.params_old is live.params and copy_.params_old is not copy_.params
    args = (_nhwc(rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)), _nhwc(rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)),
            rng.integers(0, A, size=B), rng.normal(size=B).astype(np.float32), (rng.random(B) < 0.3).astype(np.uint8))
    out = []
    for eng in (live, copy_):
        tgt, grad = torch.empty(B, device="cuda"), torch.empty(eng.P, device="cuda")
        losses = eng.update_with_batch(*args, target_out=tgt, grad_out=grad)
        out.append((losses, tgt, grad, eng.params.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert not torch.equal(copy_.params, copy_.params_old)          # the step moved the live vector, not the copy


def test_argument_errors():
    from tianshou_amd import _lib
    from tianshou_amd import crr as CR

    c, h, w, A, B = 2, 44, 36, 3, 5
    _, eng = _engine(c, h, w, A, seed=0)
    x = torch.zeros((B, h, w, c), dtype=torch.uint8, device="cuda")
    act, rew, done = np.zeros(B, np.int64), np.zeros(B, np.float32), np.zeros(B, np.uint8)
    grad = torch.zeros(eng.P, device="cuda")
    with pytest.raises(ValueError):                       # rew must be [B]
        eng.update_with_batch(x, x, act, np.zeros(B + 1, np.float32), done, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # act must be [B]
        eng.update_with_batch(x, x, act[:-1], rew, done, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # done must be [B]
        eng.update_with_batch(x, x, act, rew, done[:-1], grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # NHWC observations of the engine's geometry
        eng.update_with_batch(torch.zeros((B, w, h, c), dtype=torch.uint8, device="cuda"), x, act, rew, done, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # obs and obs_next alike
        eng.update_with_batch(x, x.float(), act, rew, done, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # grad_out holds the whole flat gradient
        eng.update_with_batch(x, x, act, rew, done, grad_out=torch.zeros(eng.P - 1, device="cuda"), apply=False)
    with pytest.raises(ValueError):                       # a gradient-only call needs somewhere to put it
        eng.update_with_batch(x, x, act, rew, done, apply=False)
    with pytest.raises(ValueError):
        CR.CRREngine(c, h, w, A, torch.zeros(eng.P - 1, device="cuda"), CR.CRRConfig())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.CRREngine(c, h, w, A, torch.zeros(eng.P), CR.CRRConfig())
    snap = eng.params.clone()
    for field, bads, word in (("beta", (0.0, float("nan"), float("inf")), "beta"), ("ratio_upper_bound", (float("nan"),), "ratio_upper_bound"),
                              ("min_q_weight", (float("nan"), float("inf")), "min_q_weight"), ("gamma", (float("nan"), float("-inf")), "gamma")):
        good = getattr(eng.cfg, field)
        for bad in bads:
            setattr(eng.cfg, field, bad)
            with pytest.raises(_lib.EngineError, match=word) as e:
                eng.update_with_batch(x, x, act, rew, done, grad_out=grad, apply=False)
            assert e.value.code == _lib.TS_ERR_INVALID_ARG
        setattr(eng.cfg, field, good)
    # the raw entry points: a mode outside the three, n_act beyond 64, a NULL pointer
    lib = _lib.load()
    s = _lib.current_stream(eng.device)
    f = torch.zeros(B * 64, device="cuda")
    i64 = torch.zeros(B, dtype=torch.int64, device="cuda")
    u8 = torch.zeros(B, dtype=torch.uint8, device="cuda")
    P = _lib.ptr
    bad_calls = [
        lib.ts_crr_loss(P(f), P(f), P(i64), P(f), _lib.i64(B), _lib.i64(A), _lib.i64(3), _lib.f64(1.0), _lib.f64(20.0), _lib.f64(1.0),
                        P(f), P(f), P(f), P(f), s),
        lib.ts_crr_loss(P(f), P(f), P(i64), P(f), _lib.i64(B), _lib.i64(65), _lib.i64(0), _lib.f64(1.0), _lib.f64(20.0), _lib.f64(1.0),
                        P(f), P(f), P(f), P(f), s),
        lib.ts_crr_loss(P(f), P(f), P(i64), P(f), _lib.i64(B), _lib.i64(A), _lib.i64(0), _lib.f64(1.0), _lib.f64(20.0), _lib.f64(1.0),
                        P(f), None, P(f), P(f), s),
        lib.ts_crr_loss(P(f), P(f), P(i64), P(f), _lib.i64(0), _lib.i64(A), _lib.i64(0), _lib.f64(1.0), _lib.f64(20.0), _lib.f64(1.0),
                        P(f), P(f), P(f), P(f), s),
        lib.ts_crr_target(P(f), P(f), P(f), P(u8), _lib.i64(B), _lib.i64(0), _lib.f64(0.9), P(f), s),
        lib.ts_crr_target(P(f), P(f), P(f), None, _lib.i64(B), _lib.i64(A), _lib.f64(0.9), P(f), s),
        lib.ts_crr_target(P(f), P(f), P(f), P(u8), _lib.i64(B), _lib.i64(A), _lib.f64(float("nan")), P(f), s),
    ]
    assert bad_calls == [_lib.TS_ERR_INVALID_ARG] * len(bad_calls)
    torch.cuda.synchronize()
    assert not f.any() and torch.equal(eng.params, snap) and (eng.iter, eng.adam_step) == (0, 0)      # nothing was launched
    losses = eng.update_with_batch(x, x, act, rew, done, grad_out=grad, apply=False)
    assert tuple(losses.shape) == (4,) and bool(torch.isfinite(losses).all())
