"""GPU parity of DiscreteBCQ on the Atari trunk -- through the C ABI (tianshou_amd.bcq), against the torch restatement of the
reference (tests/oracle_bcq.py, pinned to the unmodified reference by tests/golden/bcq_*.npz in test_oracle_bcq.py) and through
the HipDiscreteBCQ drop-in over tests/standin_bcq.py.
Tolerances are the project's own (test_gpu_iqn.py, test_gpu_dcql.py: the same trunk, the same GEMM kernels): 1e-5 relative on
the scale of each tensor, for the largest element and for the L2 norm of the difference."""
import copy

import numpy as np
import pytest
import torch

from tests import bcq_common as BC
from tests import oracle_bcq as OB

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
    from tianshou_amd import bcq as BQ

    p = OB.init_params(c, h, w, A, seed)
    eng = BQ.BCQEngine(c, h, w, A, BQ.flat_from_torch([p[k] for k in OB.PARAM_ORDER], c, h, w, A), BQ.BCQConfig(**kw))
    return p, eng


def _flat_cat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()


@pytest.mark.parametrize("A,B", [(6, 64), (3, 24), (1, 5)])
def test_batch_gradient_vs_oracle(A, B):
    """The four losses and the gradient of the whole network of one minibatch, layer by layer -- both heads and the trunk that
    takes the sum of their feature gradients -- against the CPU oracle's autograd, then the Adam step."""
    from tianshou_amd import bcq as BQ

    c, h, w = 2, 44, 36
    rng = np.random.default_rng(9)
    kw = dict(lr=1e-4, imitation_logits_penalty=0.5, target_update_freq=10)
    p, eng = _engine(c, h, w, A, seed=4, **kw)
    ocfg = OB.BCQConfig(**kw)
    st = OB.make_state(p, ocfg)
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    col: dict = {}
    q0 = OB.head(p, OB.features(p, obs), "q").detach().numpy()[np.arange(B), act]
    size = np.where(np.arange(B) % 2 == 0, 0.3, 2.0) * (1.0 + rng.random(B))  # |delta| in [0.3, 0.6] and in [2, 4], row by row
    ret = (q0 + size * rng.choice([-1.0, 1.0], size=B)).astype(np.float32)
    losses_ref = OB.update_with_batch(st, ocfg, obs, act, ret, collect=col)
    delta = col["q"][torch.arange(B), torch.as_tensor(act)].numpy() - ret
    assert (np.abs(delta) < 1).any() and (np.abs(delta) > 1).any()         # both Huber branches

    lay = BQ.layout(c, h, w, A)
    off, F, ld = lay["off"], lay["F"], lay["ld"]
    grad = torch.full((eng.P,), 7.0, dtype=torch.float32, device="cuda")   # pre-filled: every element must be written
    snap = [t.clone() for t in (eng.params, eng.params_old, eng.adam_m, eng.adam_v)]
    losses = eng.update_with_batch(_nhwc(obs), act, ret, grad_out=grad, apply=False)
    grad_b = torch.empty_like(grad)
    losses_b = eng.update_with_batch(_nhwc(obs), act, ret, grad_out=grad_b, apply=False)
    assert torch.equal(losses, losses_b) and torch.equal(grad, grad_b)     # bit-identical reruns
    # apply=False leaves parameters, moments and counters untouched
    assert all(torch.equal(a, b) for a, b in zip(snap, (eng.params, eng.params_old, eng.adam_m, eng.adam_v)))
    assert (eng.iter, eng.adam_step) == (0, 0)
    got = losses.cpu().tolist()
    print("losses", got, losses_ref)
    assert tuple(losses.shape) == (4,)
    for name, x, r in zip(BC.LOSS_NAMES, got, losses_ref):
        if A == 1 and name == "i_loss":
            assert x == 0.0 and abs(r) <= 1e-6                             # one action: log_softmax is 0
        else:
            assert abs(x - r) <= 1e-5 * abs(r), (name, x, r)
    g_ref = BQ.flat_from_torch([col["grads"][k] for k in OB.PARAM_ORDER], c, h, w, A, device="cpu")
    gc = grad.cpu()
    parts = {"conv1": (off[0], off[1]), "conv2": (off[1], off[2]), "conv3": (off[2], off[3])}
    for name, i in (("q", 3), ("i", 5)):
        parts.update({f"W{name}1": (off[i], off[i] + F * 512), f"b{name}1": (off[i] + F * 512, off[i + 1]),
                      f"W{name}2": (off[i + 1], off[i + 1] + 512 * ld), f"b{name}2": (off[i + 1] + 512 * ld, off[i + 2])})
    errs = {k: (rel_err(gc[a:b], g_ref[a:b]), l2_err(gc[a:b], g_ref[a:b])) for k, (a, b) in parts.items()}
    print("gradient (max, L2)", errs)
    if A == 1:                                  # one action: the imitator's softmax gradient is exactly 0, the penalty's is left
        assert float(g_ref[off[5]:].abs().max()) > 0
    for k, (e_max, e_l2) in errs.items():
        assert e_max < 1e-5 and e_l2 < 1e-5, (k, e_max, e_l2)
    for i in (4, 6):                            # head padding: exact zeros in the gradient of both heads
        pad = gc[off[i]:off[i + 1]].reshape(513, ld)[:, A:]
        assert float(pad.abs().max()) == 0.0
    losses2 = eng.update_with_batch(_nhwc(obs), act, ret)
    assert torch.equal(losses2, losses) and (eng.iter, eng.adam_step) == (1, 1)
    for i in (4, 6):                            # ... and in the parameters after the step
        assert float(eng.params[off[i]:off[i + 1]].reshape(513, ld)[:, A:].abs().max()) == 0.0
    new = _flat_cat(BQ.flat_to_torch(eng.params, c, h, w, A))
    ref = torch.cat([st.params[k].reshape(-1) for k in OB.PARAM_ORDER]).numpy()
    diff = np.abs(new - ref)
    bad = diff > 1e-5 * np.abs(ref) + 0.02 * ocfg.lr
    print("adam", bad.mean(), diff.max())
    assert bad.mean() < 1e-4 and diff.max() <= 2 * ocfg.lr


@pytest.mark.parametrize("tag", BC.TAGS)
def test_forward_and_target_q_vs_oracle(tag):
    """The policy pass (q, logits, masked action) and the target on the fixture's first batch with a lagged net that differs
    from the live one: the action equal row for row (the fixture's threshold distances and Q gaps make it well-defined)."""
    from tianshou_amd import bcq as BQ

    g, d, ocfg, _ = BC.load_bcq(tag)
    c, h, w, A = d["c"], d["h"], d["w"], d["n_act"]
    p, eng = _engine(c, h, w, A, seed=d["seed"], unlikely_action_threshold=ocfg.unlikely_action_threshold,
                     target_update_freq=ocfg.target_update_freq)
    st = OB.make_state(p, ocfg)
    gen = torch.Generator().manual_seed(0)
    st.params_old = {k: p[k] + 0.02 * torch.randn(p[k].shape, generator=gen) for k in OB.LAGGED_ORDER}
    eng.params_old = BQ.flat_from_torch([st.params_old[k] for k in OB.LAGGED_ORDER], c, h, w, A)
    obs = g["frames_next"][g["u0_indices"]]
    q_ref, lg_ref, act_ref = OB.policy_forward(p, obs, ocfg.log_tau())
    q, lg, act = eng.forward(_nhwc(obs))
    print("forward", rel_err(q.cpu(), q_ref), rel_err(lg.cpu(), lg_ref))
    assert rel_err(q.cpu(), q_ref) < 1e-5 and rel_err(lg.cpu(), lg_ref) < 1e-5
    assert torch.equal(act.cpu(), act_ref)
    if tag == "masked":
        assert (act_ref != q_ref.argmax(1)).float().mean() >= 0.25          # the mask decides in a quarter of the rows
    tq_ref, tact_ref = OB.target_q(st, ocfg, obs, want_act=True)
    tq, tact = eng.target_q(_nhwc(obs), want_act=True)
    assert torch.equal(tact.cpu(), tact_ref) and torch.equal(tact, act)
    print("target_q", rel_err(tq.cpu(), tq_ref))
    assert rel_err(tq.cpu(), tq_ref) < 1e-5
    assert torch.equal(eng.target_q(_nhwc(obs)), tq)                        # without the action output: the same values


def _check_adam_moments(m, v, g):
    """Adam moments after the fixture's three updates (tests/test_gpu_dcql.py's bars: sums of three gradients, so the gradient
    bar applies -- 1e-5 of each vector's scale; v is quadratic: 2e-5 of its scale)."""
    m_ref, v_ref = g["adam_m_strided"], g["adam_v_strided"]
    print("adam moments", np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max())
    assert np.abs(m - m_ref).max() <= 1e-5 * np.abs(m_ref).max()
    assert np.abs(v - v_ref).max() <= 2e-5 * np.abs(v_ref).max()


def _check_losses(got4, g, u):
    for name, x in zip(BC.LOSS_NAMES, got4):
        np.testing.assert_allclose(float(x), float(g[f"u{u}_{name}"]), rtol=1e-5, err_msg=name)


def _check_params(tensors14, old10, g, u, lr):
    flat = _flat_cat(tensors14)
    np.testing.assert_allclose(flat[::BC.STRIDE], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * lr)
    biases = _flat_cat([tensors14[i] for i in range(1, 14, 2)])
    np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-5, atol=0.02 * lr)
    np.testing.assert_allclose(_flat_cat(old10)[::BC.STRIDE], g[f"u{u}_old_params_strided"], rtol=1e-5, atol=0.02 * lr)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_update_sequence_matches_reference_golden(tag):
    """Replays the reference's DiscreteBCQ.update() sequence (sampled indices from the fixture) on the engine over a
    DeviceReplayBuffer: the target pass's action, n-step returns, the four losses, parameters, lagged parameters, Adam moments."""
    from tianshou_amd import bcq as BQ
    from tianshou_amd import dqn as D
    from tianshou_amd.buffer import DeviceReplayBuffer

    g, d, ocfg, _ = BC.load_bcq(tag)
    c, h, w, A = d["c"], d["h"], d["w"], d["n_act"]
    _, eng = _engine(c, h, w, A, seed=d["seed"], gamma=ocfg.gamma, n_step=ocfg.n_step, target_update_freq=ocfg.target_update_freq,
                     lr=ocfg.lr, unlikely_action_threshold=ocfg.unlikely_action_threshold,
                     imitation_logits_penalty=ocfg.imitation_logits_penalty)
    buf = DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                             insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"],
                             truncated=g["truncated"])
    frames, frames_next = torch.as_tensor(g["frames"]).cuda(), torch.as_tensor(g["frames_next"]).cuda()
    act_all = torch.as_tensor(g["act"]).cuda()
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        seen = []
        orig = eng.target_q
        eng.target_q = lambda on, want_act=False: seen.append(orig(on, want_act=True)) or seen[-1][0]
        try:
            ret = eng.preprocess(buf, frames, idx, 1, obs_next_frames=frames_next)
        finally:
            del eng.target_q
        assert len(seen) == 1 and np.array_equal(seen[0][1].cpu().numpy(), g[f"u{u}_target_act"])
        assert tuple(ret.shape) == (d["batch"],)
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        obs = D.gather_obs_nhwc(frames, buf, idx, 1, as_u8=True)
        losses = eng.update_with_batch(obs, act_all[idx], ret)
        _check_losses(losses.cpu().tolist(), g, u)
        _check_params(BQ.flat_to_torch(eng.params, c, h, w, A), BQ.flat_to_torch(eng.params_old, c, h, w, A)[:10], g, u, ocfg.lr)
    assert eng.adam_step == int(g["adam_step"]) and eng.iter == d["n_updates"]
    m = _flat_cat(BQ.flat_to_torch(eng.adam_m, c, h, w, A))
    v = _flat_cat(BQ.flat_to_torch(eng.adam_v, c, h, w, A))
    _check_adam_moments(m[::BC.STRIDE], v[::BC.STRIDE], g)


def _host_buffer(SB, g, d):
    """A plain host replay-buffer stand-in holding the fixture's buffer."""
    c, h, w, E, slots = d["c"], d["h"], d["w"], d["E"], d["slots"]
    buf = SB.VectorReplayBuffer(E * slots, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    buf.obs[:], buf.obs_next[:], buf.act[:], buf.rew[:] = g["frames"], g["frames_next"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    assert np.array_equal(buf._extend_offset, g["buf_offset"])
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
        buf._lengths[e] = g["buf_lengths"][e]
        buf.last_index[e] = g["buf_last_index"][e]
    return buf


def _make_algo(SB, d, ocfg, seed, **kw):
    from tianshou_amd.integration import make_hip_discrete_bcq

    torch.manual_seed(seed)
    trunk = SB.DQNetFeaturesOnly(d["c"], d["h"], d["w"])
    model, imitator = (SB.DiscreteActor(preprocess_net=trunk, action_shape=d["n_act"], hidden_sizes=[512], softmax_output=False)
                       for _ in range(2))
    policy = SB.DiscreteBCQPolicy(model=model, imitator=imitator, unlikely_action_threshold=ocfg.unlikely_action_threshold,
                                  target_update_freq=ocfg.target_update_freq)
    algo = make_hip_discrete_bcq(ref=SB)(policy=policy, lr=ocfg.lr, gamma=ocfg.gamma, n_step_return_horizon=ocfg.n_step,
                                         target_update_freq=ocfg.target_update_freq,
                                         imitation_logits_penalty=ocfg.imitation_logits_penalty, device="cuda", **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return algo


def _hook_step(SB, algo, buf, g, u):
    idx = g[f"u{u}_indices"]
    batch = algo._preprocess_batch(SB.Batch(act=buf.act[idx]), buf, idx)
    return batch, algo._update_with_batch(batch)


def _named14(algo):
    from tianshou_amd import bcq as BQ

    named = dict(algo.policy.named_parameters())
    return [named[k] for k in BQ.TIANSHOU_KEYS]


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hip_discrete_bcq_update_replays_reference_golden(tag):
    """Both fixtures through the drop-in: HipDiscreteBCQ (make_hip_discrete_bcq over tests/standin_bcq.py), its hooks called
    with the fixture's indices over a host buffer stand-in holding the fixture's buffer: returns, the four statistics, and the
    written-back torch parameters (the shared trunk once), model_old and Adam state."""
    from tests import standin_bcq as SB

    g, d, ocfg, _ = BC.load_bcq(tag)
    algo = _make_algo(SB, d, ocfg, d["seed"])
    assert type(algo).__name__ == "HipDiscreteBCQ"
    buf = _host_buffer(SB, g, d)
    for u in range(d["n_updates"]):
        batch, stat = _hook_step(SB, algo, buf, g, u)
        np.testing.assert_allclose(batch.returns.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        assert not hasattr(batch, "weight")                              # BCQ reads no batch.weight and writes none
        assert type(stat).__name__ == "DiscreteBCQTrainingStats"
        _check_losses((stat.loss, stat.q_loss, stat.i_loss, stat.reg_loss), g, u)
        _check_params([p.detach() for p in _named14(algo)], [p.detach() for p in algo.model_old.module.parameters()], g, u, ocfg.lr)
    assert algo._iter == d["n_updates"]
    assert algo.policy.model.preprocess is algo.policy.imitator.preprocess
    st = algo.optim._optim.state
    params = _named14(algo)
    assert all(float(st[p]["step"]) == float(g["adam_step"]) for p in params)
    m = _flat_cat([st[p]["exp_avg"] for p in params])
    v = _flat_cat([st[p]["exp_avg_sq"] for p in params])
    _check_adam_moments(m[::BC.STRIDE], v[::BC.STRIDE], g)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hip_discrete_bcq_resumes_from_the_written_back_state(tag):
    """A second algorithm restored from state_dict() after update 0 computes update 1 as the first one does; the threshold and
    the penalty changed on the algorithm object between two updates reach the engine."""
    from tests import standin_bcq as SB

    g, d, ocfg, _ = BC.load_bcq(tag)
    buf = _host_buffer(SB, g, d)
    a = _make_algo(SB, d, ocfg, 3)
    _hook_step(SB, a, buf, g, 0)
    state = copy.deepcopy(a.state_dict())                           # (state_dict() holds live tensors)
    assert "policy.imitator.preprocess.net.0.weight" in state       # the reference's format: the trunk listed twice
    batch_a, stat_a = _hook_step(SB, a, buf, g, 1)
    b = _make_algo(SB, d, ocfg, 4)
    b.load_state_dict(state)
    b._iter = 1                                                     # the reference keeps `_iter` outside state_dict() too
    batch_b, stat_b = _hook_step(SB, b, buf, g, 1)
    assert (stat_a.loss, stat_a.q_loss, stat_a.i_loss, stat_a.reg_loss) == (stat_b.loss, stat_b.q_loss, stat_b.i_loss, stat_b.reg_loss)
    assert torch.equal(batch_a.returns, batch_b.returns)
    for pa, pb in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(pa, pb)
    for pa, pb in zip(a.model_old.parameters(), b.model_old.parameters()):
        assert torch.equal(pa, pb)
    b._weight_reg = 2.0 * ocfg.imitation_logits_penalty + 0.25
    b.policy._log_tau = float(np.log(0.5))
    _, stat_c = _hook_step(SB, b, buf, g, 2)
    eng = b._hip_engine
    assert eng.cfg.imitation_logits_penalty == b._weight_reg and eng.log_tau() == float(np.float32(np.log(0.5)))
    np.testing.assert_allclose(stat_c.loss, stat_c.q_loss + stat_c.i_loss + b._weight_reg * stat_c.reg_loss, rtol=1e-6)


def test_argument_errors():
    from tianshou_amd import _lib
    from tianshou_amd import bcq as BQ

    c, h, w, A, B = 2, 44, 36, 3, 5
    _, eng = _engine(c, h, w, A, seed=0)
    x = torch.zeros((B, h, w, c), dtype=torch.uint8, device="cuda")
    act, ret = np.zeros(B, np.int64), np.zeros(B, np.float32)
    grad = torch.zeros(eng.P, device="cuda")
    with pytest.raises(ValueError):                       # returns must be [B]
        eng.update_with_batch(x, act, np.zeros(B + 1, np.float32), grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # act must be [B]
        eng.update_with_batch(x, act[:-1], ret, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # NHWC observations of the engine's geometry
        eng.update_with_batch(torch.zeros((B, w, h, c), dtype=torch.uint8, device="cuda"), act, ret, grad_out=grad, apply=False)
    with pytest.raises(ValueError):                       # grad_out holds the whole flat gradient
        eng.update_with_batch(x, act, ret, grad_out=torch.zeros(eng.P - 1, device="cuda"), apply=False)
    with pytest.raises(ValueError):                       # a gradient-only call needs somewhere to put it
        eng.update_with_batch(x, act, ret, apply=False)
    with pytest.raises(ValueError):
        eng.forward(torch.zeros((B, w, h, c), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="target_update_freq"):
        BQ.BCQConfig(target_update_freq=0)
    with pytest.raises(ValueError):
        BQ.BCQEngine(c, h, w, A, torch.zeros(eng.P - 1, device="cuda"), BQ.BCQConfig())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BQ.BCQEngine(c, h, w, A, torch.zeros(eng.P), BQ.BCQConfig())
    for bad in (-1.0, float("nan"), float("inf")):
        eng.cfg.imitation_logits_penalty = bad
        with pytest.raises(_lib.EngineError, match="imitation_logits_penalty") as e:
            eng.update_with_batch(x, act, ret, grad_out=grad, apply=False)
        assert e.value.code == _lib.TS_ERR_INVALID_ARG
    eng.cfg.imitation_logits_penalty = 0.01
    for bad in (0.5, float("nan")):
        eng.cfg.log_tau = bad
        with pytest.raises(_lib.EngineError, match="log_tau") as e:
            eng.forward(x)
        assert e.value.code == _lib.TS_ERR_INVALID_ARG
    eng.cfg.log_tau = None
    losses = eng.update_with_batch(x, act, ret, grad_out=grad, apply=False)
    assert tuple(losses.shape) == (4,) and bool(torch.isfinite(losses).all())
    q, lg, a = eng.forward(x)
    assert tuple(q.shape) == tuple(lg.shape) == (B, A) and tuple(a.shape) == (B,) and a.dtype == torch.int64
