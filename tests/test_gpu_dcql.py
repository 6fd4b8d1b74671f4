"""GPU parity of DiscreteCQL on the QRDQN trunk -- through the C ABI (tianshou_amd.dcql), against the torch restatement of the
reference (tests/oracle_dcql.py, pinned to the unmodified reference by tests/golden/dcql_*.npz in test_oracle_dcql.py), against
the QRDQN engine at min_q_weight = 0 and through the HipDiscreteCQL drop-in over tests/standin_dcql.py.
Tolerances are the project's own (test_gpu_distq.py): 1e-5 relative on the scale of each tensor."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle_distq as OQ
from oracle import oracle_dqn as OD
from tests import dcql_common as CC
from tests import oracle_dcql as OC

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _nhwc(a):
    return torch.as_tensor(a).permute(0, 2, 3, 1).contiguous().cuda()


def _engine(c, h, w, A, N, seed, **kw):
    from tianshou_amd import dcql as CQ
    from tianshou_amd import distq as Q

    p = OQ.init_params(c, h, w, A, N, seed)
    eng = CQ.DiscreteCQLEngine(c, h, w, A, Q.flat_from_torch([p[k] for k in OD.PARAM_ORDER], c, h, w, A, N),
                               CQ.DiscreteCQLConfig(n_atoms=N, **kw))
    return p, eng


@pytest.mark.parametrize("A,N,B,weighted", [(6, 200, 64, True), (4, 31, 37, False), (1, 8, 5, True)])
def test_batch_gradient_vs_oracle(A, N, B, weighted):
    """loss / qr_loss / cql_loss, new priorities and the whole gradient of one minibatch layer by layer, then the Adam step."""
    from tianshou_amd import distq as Q
    from tianshou_amd import dqn as D

    c, h, w = 4, 84, 84
    rng = np.random.default_rng(9)
    kw = dict(lr=1e-4, min_q_weight=10.0)
    p, eng = _engine(c, h, w, A, N, seed=4, **kw)
    ocfg = OC.DiscreteCQLConfig(n_atoms=N, **kw)
    st = OD.DQNState.create(p, ocfg.dqn())
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    ret = (rng.normal(size=(B, N)) * 2.5).astype(np.float32)         # |d| on both sides of 1
    weight = rng.random(B).astype(np.float32) if weighted else None
    col: dict = {}
    loss_ref, prio_ref = OC.update_with_batch(st, ocfg, obs, act, ret, A, weight=weight, collect=col)

    off, _ = D.layer_layout(c, h, w, 1)
    bounds = list(off[:5]) + [eng.P]
    ld = Q.head_width(A, N)
    grad = torch.full((eng.P,), 7.0, dtype=torch.float32, device="cuda")          # pre-filled: every element must be written
    losses, prio = eng.update_with_batch(_nhwc(obs), act, ret, weight, grad_out=grad, apply=False)
    grad_b = torch.empty_like(grad)
    losses_b, prio_b = eng.update_with_batch(_nhwc(obs), act, ret, weight, grad_out=grad_b, apply=False)
    assert torch.equal(losses, losses_b) and torch.equal(prio, prio_b) and torch.equal(grad, grad_b)      # bit-identical reruns
    got = losses.cpu().tolist()
    print("losses", got, loss_ref, "prio", rel_err(prio.cpu(), prio_ref))
    assert tuple(losses.shape) == (3,)
    for name, x, r in zip(("loss", "qr_loss", "cql_loss"), got, loss_ref):
        if A == 1 and name == "cql_loss":
            assert x == 0.0 and abs(r) <= 1e-6                                     # one action: logsumexp(q) - q
        else:
            assert abs(x - r) <= 1e-5 * abs(r), (name, x, r)
    assert rel_err(prio.cpu(), prio_ref) < 1e-5
    g_ref = Q.flat_from_torch([col["grads"][k] for k in OD.PARAM_ORDER], c, h, w, A, N, device="cpu")
    gc = grad.cpu()
    errs = [rel_err(gc[bounds[i]:bounds[i + 1]], g_ref[bounds[i]:bounds[i + 1]]) for i in range(5)]
    print("gradient", errs)
    for i, e in enumerate(errs):
        assert e < 1e-5, f"layer {i}: {e}"
    head = gc[bounds[4]:].reshape(513, ld)
    assert head[:, A * N:].numel() == 0 or float(head[:, A * N:].abs().max()) == 0.0       # padding columns: exact zeros
    if A > 1:                        # the CQL term reaches the columns of actions no sample took as well: all live columns move
        assert bool((head[512, :A * N] != 0).all())
    losses2, _ = eng.update_with_batch(_nhwc(obs), act, ret, weight)
    assert torch.equal(losses2, losses)
    new = torch.cat([t.reshape(-1) for t in Q.flat_to_torch(eng.params, c, h, w, A, N)]).cpu().numpy()
    pad = eng.params[bounds[4]:].reshape(513, -1)[:, A * N:]
    assert pad.numel() == 0 or float(pad.abs().max()) == 0.0          # padding columns stay exactly zero
    ref = OD.flatten_params(st.params).numpy()
    diff = np.abs(new - ref)
    bad = diff > 1e-5 * np.abs(ref) + 0.02 * ocfg.lr
    print("adam", bad.mean(), diff.max())
    assert bad.mean() < 1e-4 and diff.max() <= 2 * ocfg.lr


@pytest.mark.parametrize("A,N,B,weighted", [(6, 200, 64, True), (3, 21, 24, False)])
def test_zero_min_q_weight_is_qrdqn_bit_for_bit(A, N, B, weighted):
    """Two updates on the same inputs: DiscreteCQLEngine(min_q_weight=0) against DistQEngine(kind="qr")."""
    from tianshou_amd import distq as Q

    c, h, w = 4, 84, 84
    kw = dict(lr=1e-3, target_update_freq=1, max_grad_norm=5.0)
    p, cql = _engine(c, h, w, A, N, seed=6, min_q_weight=0.0, **kw)
    qr = Q.DistQEngine(c, h, w, A, Q.flat_from_torch([p[k] for k in OD.PARAM_ORDER], c, h, w, A, N),
                       Q.DistQConfig(kind="qr", n_atoms=N, **kw))
    rng = np.random.default_rng(3)
    for _ in range(2):
        obs = _nhwc(rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8))
        act = rng.integers(0, A, size=B)
        ret = (rng.normal(size=(B, N)) * 2.5).astype(np.float32)
        weight = rng.random(B).astype(np.float32) if weighted else None
        losses, prio_c = cql.update_with_batch(obs, act, ret, weight)
        loss, prio_q = qr.update_with_batch(obs, act, ret, weight)
        assert torch.equal(prio_c, prio_q)
        assert float(losses[0]) == float(losses[1]) == float(loss[0])
        assert float(losses[2]) > 0.0 and np.isfinite(float(losses[2]))      # the term is still reported
    assert torch.equal(cql.params, qr.params) and torch.equal(cql.adam_m, qr.adam_m) and torch.equal(cql.adam_v, qr.adam_v)
    assert torch.equal(cql.params_old, qr.params_old) and cql.adam_step == qr.adam_step == 2 and cql.iter == qr.iter == 2


def _check_adam_moments(m, v, g):
    """Adam moments after the fixture's three updates.  They are sums of three gradients, so the gradient bar applies: 1e-5
    of each vector's scale (m is linear in the gradients; v is quadratic: twice the relative error, 2e-5 of its scale)."""
    m_ref, v_ref = g["adam_m_strided"], g["adam_v_strided"]
    print("adam moments", np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max())
    assert np.abs(m - m_ref).max() <= 1e-5 * np.abs(m_ref).max()
    assert np.abs(v - v_ref).max() <= 2e-5 * np.abs(v_ref).max()


def _check_losses(got3, g, u):
    for name, x in zip(("loss", "qr_loss", "cql_loss"), got3):
        np.testing.assert_allclose(float(x), float(g[f"u{u}_{name}"]), rtol=1e-5, err_msg=name)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_update_sequence_matches_reference_golden(tag):
    """Replays the reference's DiscreteCQL.update() sequence (sampled indices and, for the prioritized buffer, PER weights from
    the fixture) on the engine over a DeviceReplayBuffer: n-step returns, priorities, the loss triple, parameters."""
    from tianshou_amd import distq as Q
    from tianshou_amd import dqn as D
    from tianshou_amd.buffer import DeviceReplayBuffer

    g, d, ocfg, _ = CC.load_dcql(tag)
    lagged = ocfg.target_update_freq > 0
    c, h, w, A, N = d["c"], d["h"], d["w"], d["n_act"], d["n_atoms"]
    _, eng = _engine(c, h, w, A, N, seed=d["seed"], gamma=ocfg.gamma, n_step=ocfg.n_step,
                     target_update_freq=ocfg.target_update_freq, lr=ocfg.lr, min_q_weight=ocfg.min_q_weight)
    buf = DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                             insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"],
                             truncated=g["truncated"])
    frames, frames_next = torch.as_tensor(g["frames"]).cuda(), torch.as_tensor(g["frames_next"]).cuda()
    act_all = torch.as_tensor(g["act"]).cuda()
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        ret = eng.preprocess(buf, frames, idx, 1, obs_next_frames=frames_next)
        assert tuple(ret.shape) == (d["batch"], N)
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        obs = D.gather_obs_nhwc(frames, buf, idx, 1, as_u8=True)
        losses, prio = eng.update_with_batch(obs, act_all[idx], ret, CC.is_weight(g, u, d["prioritized"]))
        np.testing.assert_allclose(prio.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=2e-5)
        _check_losses(losses.cpu().tolist(), g, u)
        tensors = Q.flat_to_torch(eng.params, c, h, w, A, N)
        flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(tensors[0].cpu().numpy(), g[f"u{u}_conv1_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        biases = torch.cat([tensors[i].reshape(-1) for i in range(1, 10, 2)]).cpu().numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-5, atol=0.02 * ocfg.lr)
        if lagged:
            old = torch.cat([t.reshape(-1) for t in Q.flat_to_torch(eng.params_old, c, h, w, A, N)]).cpu().numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
    assert eng.adam_step == int(g["adam_step"])
    m = torch.cat([t.reshape(-1) for t in Q.flat_to_torch(eng.adam_m, c, h, w, A, N)]).cpu().numpy()
    v = torch.cat([t.reshape(-1) for t in Q.flat_to_torch(eng.adam_v, c, h, w, A, N)]).cpu().numpy()
    _check_adam_moments(m[::61], v[::61], g)


def _host_buffer(SC, g, d):
    """A host replay-buffer stand-in holding the fixture's buffer: prioritized or plain, as the fixture was recorded."""
    c, h, w, E, slots = d["c"], d["h"], d["w"], d["E"], d["slots"]
    kw = dict(obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    if d["prioritized"]:
        buf = SC.PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4, **kw)
    else:
        buf = SC.VectorReplayBuffer(E * slots, E, **kw)
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
    from tianshou_amd.integration import make_hip_discrete_cql

    torch.manual_seed(seed)
    net = SC.QRDQNet(d["c"], d["h"], d["w"], d["n_act"], d["n_atoms"])
    algo = make_hip_discrete_cql(ref=SC)(policy=SC.DiscreteQLearningPolicy(net), lr=ocfg.lr, min_q_weight=ocfg.min_q_weight,
                                         gamma=ocfg.gamma, num_quantiles=d["n_atoms"], n_step_return_horizon=ocfg.n_step,
                                         target_update_freq=ocfg.target_update_freq, device="cuda", **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return net, algo


def _hook_step(SC, algo, buf, g, d, u):
    idx = g[f"u{u}_indices"]
    batch = SC.Batch(act=buf.act[idx])
    if d["prioritized"]:
        batch.weight = g[f"u{u}_is_weight"]
    batch = algo._preprocess_batch(batch, buf, idx)
    stat = algo._update_with_batch(batch)
    return batch, stat


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_discrete_cql_update_replays_reference_golden(tag):
    """Both fixtures through the drop-in: HipDiscreteCQL (make_hip_discrete_cql over tests/standin_dcql.py), its hooks called with
    the fixture's indices (and PER weights) over a host buffer stand-in holding the fixture's buffer: returns, batch.weight, the
    statistics triple, and the written-back torch parameters, model_old and Adam state."""
    from tests import standin_dcql as SC

    g, d, ocfg, _ = CC.load_dcql(tag)
    lagged = ocfg.target_update_freq > 0
    net, algo = _make_algo(SC, d, ocfg, d["seed"])
    assert type(algo).__name__ == "HipDiscreteCQL"
    buf = _host_buffer(SC, g, d)
    keys = OD.TIANSHOU_KEYS
    for u in range(d["n_updates"]):
        batch, stat = _hook_step(SC, algo, buf, g, d, u)
        np.testing.assert_allclose(batch.returns.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(batch.weight.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=2e-5)
        assert type(stat).__name__ == "DiscreteCQLTrainingStats"
        _check_losses((stat.loss, stat.qr_loss, stat.cql_loss), g, u)
        sd = net.state_dict()                                         # the torch modules after the write-back
        flat = torch.cat([sd[k].reshape(-1) for k in keys]).cpu().numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(sd[keys[0]].cpu().numpy(), g[f"u{u}_conv1_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        biases = torch.cat([sd[k].reshape(-1) for k in keys if k.endswith("bias")]).cpu().numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-5, atol=0.02 * ocfg.lr)
        if lagged:
            so = algo.model_old.module.state_dict()
            old = torch.cat([so[k].reshape(-1) for k in keys]).cpu().numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
    assert algo._iter == d["n_updates"]
    st = algo.optim._optim.state
    params = [dict(net.named_parameters())[k] for k in keys]
    assert all(float(st[p]["step"]) == float(g["adam_step"]) for p in params)
    m = torch.cat([st[p]["exp_avg"].reshape(-1) for p in params]).cpu().numpy()
    v = torch.cat([st[p]["exp_avg_sq"].reshape(-1) for p in params]).cpu().numpy()
    _check_adam_moments(m[::61], v[::61], g)


@pytest.mark.parametrize("tag", CC.TAGS)
def test_hip_discrete_cql_resumes_from_the_written_back_state(tag):
    """A second algorithm restored from state_dict() after update 0 computes update 1 as the first one does; `min_q_weight`
    changed on the algorithm object between two updates reaches the engine."""
    from tests import standin_dcql as SC

    g, d, ocfg, _ = CC.load_dcql(tag)
    buf = _host_buffer(SC, g, d)
    _, a = _make_algo(SC, d, ocfg, 3)
    _hook_step(SC, a, buf, g, d, 0)
    state = copy.deepcopy(a.state_dict())                           # (state_dict() holds live tensors)
    batch_a, stat_a = _hook_step(SC, a, buf, g, d, 1)
    _, b = _make_algo(SC, d, ocfg, 4)
    b.load_state_dict(state)
    b._iter = 1                                                     # the reference keeps `_iter` outside state_dict() too
    batch_b, stat_b = _hook_step(SC, b, buf, g, d, 1)
    assert (stat_a.loss, stat_a.qr_loss, stat_a.cql_loss) == (stat_b.loss, stat_b.qr_loss, stat_b.cql_loss)
    assert torch.equal(batch_a.weight, batch_b.weight)
    for pa, pb in zip(a.policy.model.parameters(), b.policy.model.parameters()):
        assert torch.equal(pa, pb)
    b.min_q_weight = 2.0 * ocfg.min_q_weight
    _, stat_c = _hook_step(SC, b, buf, g, d, 2)
    assert b._hip_engine.cfg.min_q_weight == 2.0 * ocfg.min_q_weight
    np.testing.assert_allclose(stat_c.loss, stat_c.qr_loss + 2.0 * ocfg.min_q_weight * stat_c.cql_loss, rtol=1e-6)


def test_argument_errors():
    from tianshou_amd import _lib
    from tianshou_amd import dcql as CQ

    c, h, w, A, N, B = 2, 44, 36, 3, 11, 5
    _, eng = _engine(c, h, w, A, N, seed=0)
    x = torch.zeros((B, h, w, c), dtype=torch.uint8, device="cuda")
    act, ret = np.zeros(B, np.int64), np.zeros((B, N), np.float32)
    with pytest.raises(ValueError):                       # returns must be [B, n_atoms]
        eng.update_with_batch(x, act, np.zeros(B, np.float32), apply=False)
    with pytest.raises(ValueError):                       # act must be [B]
        eng.update_with_batch(x, act[:-1], ret, apply=False)
    with pytest.raises(ValueError):                       # weight must be [B]
        eng.update_with_batch(x, act, ret, np.ones(B + 1, np.float32), apply=False)
    with pytest.raises(ValueError):                       # NHWC observations of the engine's geometry
        eng.update_with_batch(torch.zeros((B, w, h, c), dtype=torch.uint8, device="cuda"), act, ret, apply=False)
    with pytest.raises(ValueError):                       # grad_out holds the whole flat gradient
        eng.update_with_batch(x, act, ret, grad_out=torch.zeros(eng.P - 1, device="cuda"), apply=False)
    with pytest.raises(ValueError):
        CQ.DiscreteCQLConfig(kind="c51", n_atoms=N)
    for bad in (-1.0, float("nan"), float("inf")):
        eng.cfg.min_q_weight = bad
        with pytest.raises(_lib.EngineError, match="min_q_weight") as e:
            eng.update_with_batch(x, act, ret, apply=False)
        assert e.value.code == _lib.TS_ERR_INVALID_ARG
    eng.cfg.min_q_weight = 1.0
    losses, prio = eng.update_with_batch(x, act, ret, apply=False)
    assert tuple(losses.shape) == (3,) and tuple(prio.shape) == (B,) and bool(torch.isfinite(losses).all())
