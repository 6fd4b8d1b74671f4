"""GPU parity of DQN on the recurrent Q network (SURVEY 8f N4's recurrent item; test/discrete/test_drqn.py's setup): LSTM
forward / backward through time on the GEMM kernels, stacked vector observations, n-step double-Q targets, DQN loss, Adam --
through the C ABI, against the oracle (oracle/oracle_drqn.py) and the reference fixtures tests/golden/drqn_*.npz."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from oracle import oracle_drqn as ORQ
from tests import dqn_common as DC
from tests.drqn_edge_cases import rand_params

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["layer_kernels", "per_step"], autouse=True)
def lstm_path(request, monkeypatch):
    """Every test runs on both recurrent paths: a whole LSTM layer per launch (lstm_layer_fwd / bwd_kernel, H = 32, 64, 128)
    and one GEMM + one cell launch per step (TS_RNN_PER_STEP, the path of the other widths)."""
    if request.param == "per_step":
        monkeypatch.setenv("TS_RNN_PER_STEP", "1")


def make_engine(p, obs_dim, hidden, layers, n_act, ocfg):
    from tianshou_amd import dqn as D
    from tianshou_amd import drqn as R

    cfg = D.DQNConfig(gamma=ocfg.gamma, n_step=ocfg.n_step, target_update_freq=ocfg.target_update_freq, is_double=ocfg.is_double,
                      huber_delta=ocfg.huber_delta, lr=ocfg.lr, max_grad_norm=ocfg.max_grad_norm)
    flat = R.flat_from_torch([p[k] for k in ORQ.param_keys(layers)], obs_dim, hidden, layers, n_act)
    return R.RecurrentDQNEngine(obs_dim, hidden, layers, n_act, flat, cfg)


def torch_order(flat, obs_dim, hidden, layers, n_act):
    from tianshou_amd import drqn as R

    return torch.cat([t.reshape(-1) for t in R.flat_to_torch(flat, obs_dim, hidden, layers, n_act)]).cpu().numpy()


SHAPES = [(4, 128, 2, 2, 33, 4), (37, 64, 1, 5, 257, 3), (17, 32, 3, 32, 64, 1)]


@pytest.mark.parametrize("obs_dim,hidden,layers,n_act,B,T", SHAPES)
def test_forward_and_state_passing_vs_oracle(obs_dim, hidden, layers, n_act, B, T):
    from tianshou_amd import drqn as R

    p = rand_params(obs_dim, hidden, layers, n_act, 1)
    eng = make_engine(p, obs_dim, hidden, layers, n_act, OD.DQNConfig())
    flat = R.flat_from_torch([p[k] for k in ORQ.param_keys(layers)], obs_dim, hidden, layers, n_act)
    assert all(torch.equal(a.cpu(), p[k]) for a, k in zip(R.flat_to_torch(flat, obs_dim, hidden, layers, n_act), ORQ.param_keys(layers)))
    g = torch.Generator().manual_seed(B)
    obs = torch.randn(B, T, obs_dim, generator=g)
    q, act, (h, c) = eng.forward(obs, want_state=True)
    q_want, (h_want, c_want) = ORQ.forward(p, obs, want_state=True)
    np.testing.assert_allclose(q.cpu().numpy(), q_want.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(h.cpu().numpy(), h_want.transpose(0, 1).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(c.cpu().numpy(), c_want.transpose(0, 1).numpy(), rtol=1e-5, atol=1e-5)
    qs = np.sort(q_want.numpy(), axis=1)
    clear = (qs[:, -1] - qs[:, -2] > 1e-4) if n_act > 1 else np.ones(B, bool)
    np.testing.assert_array_equal(act.cpu().numpy()[clear], q_want.argmax(dim=1).numpy()[clear])
    # one more evaluation-mode step from the carried state (obs [B, dim])
    o2 = torch.randn(B, obs_dim, generator=g)
    q2, _, (h2, c2) = eng.forward(o2, state=(h, c), want_state=True)
    q2_want, (h2_want, _) = ORQ.forward(p, o2, state=(h_want, c_want), want_state=True)
    np.testing.assert_allclose(q2.cpu().numpy(), q2_want.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(h2.cpu().numpy(), h2_want.transpose(0, 1).numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("obs_dim,hidden,layers,n_act,B,T", SHAPES)
@pytest.mark.parametrize("huber,weighted,clip", [(1.0, False, None), (None, True, 0.5)])
def test_gradient_and_step_vs_oracle(obs_dim, hidden, layers, n_act, B, T, huber, weighted, clip):
    p = rand_params(obs_dim, hidden, layers, n_act, 2)
    ocfg = OD.DQNConfig(huber_delta=huber, lr=3e-4, max_grad_norm=clip)
    eng = make_engine(p, obs_dim, hidden, layers, n_act, ocfg)
    st = OD.DQNState.create(p, ocfg)
    g = torch.Generator().manual_seed(B + 7)
    obs = torch.randn(B, T, obs_dim, generator=g)
    act = torch.randint(0, n_act, (B,), generator=g)
    ret = torch.randn(B, generator=g) * 2
    w = torch.rand(B, generator=g) + 0.5 if weighted else None
    col = {}
    loss_want, td_want = ORQ.update_with_batch(st, ocfg, obs, act, ret, w, collect=col)
    grad = torch.empty_like(eng.params)
    before = eng.params.clone()
    loss, td = eng.update_with_batch(obs, act, ret, w, grad_out=grad, apply=False)
    assert torch.equal(eng.params, before)
    assert abs(float(loss) - loss_want) <= 1e-5 * max(1.0, abs(loss_want))
    np.testing.assert_allclose(td.cpu().numpy(), td_want.numpy(), rtol=1e-5, atol=1e-5)
    g_want = torch.cat([col["grads"][k].reshape(-1) for k in ORQ.param_keys(layers)]).numpy()
    g_got = torch_order(grad, obs_dim, hidden, layers, n_act)
    np.testing.assert_allclose(g_got, g_want, rtol=1e-4, atol=1e-5 * np.abs(g_want).max())
    # the padding rows / columns receive exactly zero gradient (they must stay zero under Adam)
    lay = eng.lay
    if lay["k0"] > obs_dim:
        assert float(grad[lay["fc1"]:lay["fc1"] + (lay["k0"] + 1) * hidden].reshape(-1, hidden)[obs_dim:lay["k0"]].abs().max()) == 0.0
    if n_act < 32:
        assert float(grad[lay["fc2"]:].reshape(hidden + 1, 32)[:, n_act:].abs().max()) == 0.0
    eng.iter = 0
    loss2, _ = eng.update_with_batch(obs, act, ret, w)
    assert float(loss2) == float(loss)
    after = ORQ.flatten(st.params, layers).numpy()
    np.testing.assert_allclose(torch_order(eng.params, obs_dim, hidden, layers, n_act), after, rtol=1e-4, atol=0.02 * ocfg.lr)


@pytest.mark.parametrize("tag", ["cartpole", "per"])
def test_update_sequence_matches_reference_fixture(tag):
    """Replays the reference's DQN.update() sequence on the Recurrent network (sampled indices from the fixture)."""
    from tianshou_amd import drqn as R
    from tianshou_amd.buffer import DeviceReplayBuffer

    g, d, ocfg, bstate = DC.load_drqn(tag)
    dims = (d["obs_dim"], d["hidden"], d["layers"], d["n_act"])
    p0 = ORQ.unflatten(g["params0"], *dims)
    eng = make_engine(p0, *dims, ocfg)
    buf = DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                             insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"], truncated=g["truncated"])
    rows = torch.as_tensor(g["obs_rows"]).cuda()
    act_all = torch.as_tensor(g["act"]).cuda()
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        obs = R.gather_stacked_obs(rows, buf, idx, d["stack_num"])
        if u == 0:
            np.testing.assert_array_equal(obs.cpu().numpy(), g["u0_obs"])
        ret = eng.preprocess(buf, rows, idx, d["stack_num"])
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        w = torch.as_tensor(g[f"u{u}_is_weight"]).cuda() if d["per"] else None
        loss, td = eng.update_with_batch(obs, act_all[idx], ret, w)
        np.testing.assert_allclose(td.cpu().numpy(), g[f"u{u}_td"], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(float(loss), float(g[f"u{u}_loss"]), rtol=2e-5)
        tensors = dict(zip(ORQ.param_keys(d["layers"]), (t.cpu() for t in R.flat_to_torch(eng.params, *dims))))
        tol = dict(rtol=1e-4, atol=0.02 * ocfg.lr * (u + 1))
        np.testing.assert_allclose(ORQ.flatten(tensors, d["layers"]).numpy()[::17], g[f"u{u}_params_strided"], **tol)
        np.testing.assert_allclose(DC.drqn_small(tensors, d["layers"]), g[f"u{u}_small"], **tol)
    # evaluation-mode steps with the carried state, on the final parameters (as the fixture recorded them)
    q1, _, s1 = eng.forward(torch.as_tensor(g["eval_obs"][0]), want_state=True)
    q2, _, s2 = eng.forward(torch.as_tensor(g["eval_obs"][1]), state=s1, want_state=True)
    np.testing.assert_allclose(torch.stack([q1, q2]).cpu().numpy(), g["eval_q"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(s2[0].cpu().numpy(), g["eval_hidden"], rtol=1e-3, atol=1e-4)


def test_bad_arguments_fail_loudly():
    from tianshou_amd import _lib
    from tianshou_amd import dqn as D
    from tianshou_amd import drqn as R

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.RecurrentDQNEngine(4, 128, 2, 2, torch.zeros(10), D.DQNConfig())
    with pytest.raises((ValueError, _lib.EngineError)):
        R.layout(4, 48, 2, 2)                      # hidden not a multiple of 32
    with pytest.raises((ValueError, _lib.EngineError)):
        R.layout(4, 64, 2, 33)                     # more than 32 actions
    p = rand_params(4, 32, 1, 2, 0)
    eng = make_engine(p, 4, 32, 1, 2, OD.DQNConfig())
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(3, 2, 5))
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(3, 4), state=(torch.zeros(3, 2, 32), torch.zeros(3, 2, 32)))


def test_prefetched_forward_and_concurrent_target_pass_give_identical_updates():
    """RecurrentDQNEngine.preprocess_with_obs (batch.obs gathered first, its forward pass on the workspace's second side stream
    into a cache that ts_rnnq_update_cached consumes; the lagged network's pass of _target_q on the first side stream) against
    the plain order preprocess -> update_with_batch: four updates with a target sync in between, identical returns, losses, TD
    errors, parameters and Adam moments; a stale prefetch (parameters written since) is ignored."""
    from tianshou_amd import drqn as R
    from tianshou_amd.buffer import DeviceReplayBuffer

    obs_dim, hidden, layers, n_act, B, T, slots, E = 4, 128, 2, 2, 96, 4, 2048, 4
    p = rand_params(obs_dim, hidden, layers, n_act, 4)
    ocfg = OD.DQNConfig(gamma=0.95, n_step=3, target_update_freq=2, is_double=True, lr=1e-3)
    g = torch.Generator().manual_seed(9)
    Tn = slots // E
    off = np.arange(E + 1, dtype=np.int64) * Tn
    buf = DeviceReplayBuffer(offset=off, last_index=off[:-1] + Tn - 1, lengths=np.full(E, Tn, np.int64), insertion=np.zeros(E, np.int64),
                             rew=torch.randn(slots, generator=g).double().numpy(), terminated=(torch.rand(slots, generator=g) < 0.05).numpy(),
                             truncated=np.zeros(slots, bool), obs=torch.randn(slots, obs_dim, generator=g).numpy(),
                             act=torch.randint(0, n_act, (slots,), generator=g).numpy())
    plain, pre = make_engine(p, obs_dim, hidden, layers, n_act, ocfg), make_engine(p, obs_dim, hidden, layers, n_act, ocfg)
    for it in range(4):
        idx = torch.randint(0, slots, (B,), generator=g).cuda()
        ret0 = plain.preprocess(buf, buf.obs, idx, T)
        out0 = plain.update_with_batch(R.gather_stacked_obs(buf.obs, buf, idx, T), buf.act[idx], ret0)
        obs, ret1 = pre.preprocess_with_obs(buf, buf.obs, idx, T)
        assert pre._pre is not None and pre._pre[0] is obs
        out1 = pre.update_with_batch(obs, buf.act[idx], ret1)
        assert pre._pre is None
        assert torch.equal(ret0, ret1) and torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1]), it
        for name in ("params", "adam_m", "adam_v", "params_old"):
            assert torch.equal(getattr(plain, name), getattr(pre, name)), (it, name)
    # a prefetch that predates a parameter write is ignored (own forward pass)
    obs = pre.prefetch_forward(R.gather_stacked_obs(buf.obs, buf, idx, T))
    stale, pre._pre = pre._pre, None
    pre.update_with_batch(obs.clone(), buf.act[idx], ret1)
    plain.update_with_batch(obs.clone(), buf.act[idx], ret1)
    pre._pre = stale
    a, b = pre.update_with_batch(obs, buf.act[idx], ret1), plain.update_with_batch(obs, buf.act[idx], ret1)
    assert torch.equal(a[0], b[0]) and torch.equal(plain.params, pre.params)


@pytest.mark.parametrize("n_step,stack", [(1, 1), (1, 4), (3, 4), (4, 2), (2, 16)])
def test_stacked_rows_pair_equals_the_index_kernels_and_row_gathers(n_step, stack):
    """ts_stacked_rows_pair (one launch) against nstep_indices + next() + 2 x (stack_indices + gather_rows) + act[index] on a
    ragged buffer (five sub-buffers of different fill, random episode ends, repeated / unordered indices), with and without
    stored obs_next rows; layouts outside the kernel's return None."""
    from tianshou_amd import drqn as R
    from tianshou_amd.buffer import DeviceReplayBuffer
    from tianshou_amd.returns import nstep_indices

    rng = np.random.default_rng(10 * n_step + stack)
    sizes, fill = np.array([9, 1, 30, 17, 4]), np.array([9, 1, 12, 17, 0])
    off = np.concatenate([[0], np.cumsum(sizes)])
    total = int(off[-1])
    last = off[:-1] + np.array([3, 0, 11, 5, 0])
    rb = DeviceReplayBuffer(offset=off, last_index=last, lengths=fill, insertion=(last + 1 - off[:-1]) % sizes,
                            rew=rng.standard_normal(total), terminated=rng.random(total) < 0.15, truncated=rng.random(total) < 0.1)
    rows = torch.as_tensor(rng.standard_normal((total, 5)).astype(np.float32)).cuda()
    rows_next = torch.as_tensor(rng.standard_normal((total, 5)).astype(np.float32)).cuda()
    act_col = torch.as_tensor(rng.integers(0, 7, total)).cuda()
    valid = np.concatenate([np.arange(off[e], off[e] + fill[e]) for e in range(5)])
    ix = torch.as_tensor(rng.choice(valid, 301)).cuda()
    after = nstep_indices(rb, ix, n_step)
    for nxt in (None, rows_next):
        pair = R.gather_stacked_obs_pair(rows, rb, ix, n_step, stack, nxt, act_col)
        assert pair is not None
        assert torch.equal(pair[0], R.gather_stacked_obs(rows, rb, ix, stack))
        want = R.gather_stacked_obs(rows, rb, rb.next(after), stack) if nxt is None else R.gather_stacked_obs(nxt, rb, after, stack)
        assert torch.equal(pair[1], want)
        assert torch.equal(pair[2], act_col[ix])
    assert R.gather_stacked_obs_pair(rows, rb, ix, n_step, stack)[2] is None
    assert R.gather_stacked_obs_pair(rows.double(), rb, ix, n_step, stack) is None
    assert R.gather_stacked_obs_pair(rows, rb, ix, n_step, 17) is None
    assert R.gather_stacked_obs_pair(rows, rb, ix[:0], n_step, stack)[0].shape == (0, stack, 5)


def test_replay_stream_cycle_on_a_uniform_buffer_equals_the_sequential_cycle(monkeypatch):
    """dqn.ReplayStream without priorities + drqn.replay_prepare (next batch's indices, both stacked gathers, actions and n-step
    coefficients on a second stream beside the update) against sample -> preprocess -> update on one stream through the index
    kernels (TS_DRQN_NO_PAIR): six updates with target syncs, identical indices, returns, losses, TD errors and parameters."""
    from tianshou_amd import dqn as D
    from tianshou_amd import drqn as R
    from tianshou_amd.buffer import DeviceReplayBuffer

    obs_dim, hidden, layers, n_act, B, T, slots, E = 4, 128, 2, 2, 64, 4, 2048, 4

    def cycle(use_stream: bool):
        g = torch.Generator().manual_seed(9)
        Tn = slots // E
        off = np.arange(E + 1, dtype=np.int64) * Tn
        buf = DeviceReplayBuffer(offset=off, last_index=off[:-1] + Tn - 1, lengths=np.full(E, Tn, np.int64),
                                 insertion=np.zeros(E, np.int64), rew=torch.randn(slots, generator=g).double().numpy(),
                                 terminated=(torch.rand(slots, generator=g) < 0.05).numpy(), truncated=np.zeros(slots, bool),
                                 obs=torch.randn(slots, obs_dim, generator=g).numpy(),
                                 act=torch.randint(0, n_act, (slots,), generator=g).numpy())
        eng = make_engine(rand_params(obs_dim, hidden, layers, n_act, 4), obs_dim, hidden, layers, n_act,
                          OD.DQNConfig(gamma=0.95, n_step=3, target_update_freq=2, is_double=True, lr=1e-3))
        tick = [0]

        def draw():
            tick[0] += 1
            return buf.sample_indices(B, seed=(0x5A7, tick[0]))

        rs = (D.ReplayStream(eng, buf, buf.obs, None, T, draw, None, prepare=R.replay_prepare(eng, buf, buf.obs, T, buf.act))
              if use_stream else None)
        log = []
        for _ in range(6):
            if rs is None:
                idx = draw()
                obs, ret = eng.preprocess_with_obs(buf, buf.obs, idx, T)
                loss, td = eng.update_with_batch(obs, buf.act[idx], ret)
            else:
                idx, _, _, pair, coef = rs.take()
                obs, ret = eng.preprocess_with_obs(buf, buf.obs, idx, T, pair=pair, coef=coef)
                loss, td = eng.update_with_batch(obs, pair[2], ret)
                rs.give(idx, None)
            log.append((idx.clone(), ret.clone(), loss.clone(), td.clone()))
        torch.cuda.synchronize()
        return log, eng.params.clone()

    with monkeypatch.context() as m:
        m.setenv("TS_DRQN_NO_PAIR", "1")
        a = cycle(False)
    b = cycle(True)
    for it, (x, y) in enumerate(zip(a[0], b[0])):
        for u, v in zip(x, y):
            assert torch.equal(u, v), it
    assert torch.equal(a[1], b[1])


@pytest.mark.parametrize("lagged,stored_next", [(True, False), (False, True)])
def test_learn_step_equals_sample_preprocess_update(lagged, stored_next):
    """RecurrentDQNEngine.learn_step (ts_rnnq_learn_step: sampling, both stacked gathers, n-step coefficients, target passes,
    forward / backward / Adam and the next update's batch in one library call) against buffer.sample_indices ->
    preprocess_with_obs -> update_with_batch: seven updates with target syncs, a `learn_reset` in the middle (the batch is then
    sampled inside the call), identical losses, TD errors, parameters and Adam moments."""
    from tianshou_amd.buffer import DeviceReplayBuffer

    obs_dim, hidden, layers, n_act, B, T, slots, E = 4, 128, 2, 2, 64, 4, 2048, 4
    g = torch.Generator().manual_seed(9)
    Tn = slots // E
    off = np.arange(E + 1, dtype=np.int64) * Tn
    buf = DeviceReplayBuffer(offset=off, last_index=off[:-1] + Tn - 1, lengths=np.full(E, Tn, np.int64), insertion=np.zeros(E, np.int64),
                             rew=torch.randn(slots, generator=g).double().numpy(), terminated=(torch.rand(slots, generator=g) < 0.05).numpy(),
                             truncated=np.zeros(slots, bool), obs=torch.randn(slots, obs_dim, generator=g).numpy(),
                             act=torch.randint(0, n_act, (slots,), generator=g).numpy())
    nxt = torch.randn(slots, obs_dim, generator=g).cuda() if stored_next else None
    ocfg = OD.DQNConfig(gamma=0.95, n_step=3, target_update_freq=2 if lagged else 0, is_double=True, lr=1e-3)
    p = rand_params(obs_dim, hidden, layers, n_act, 4)
    ref, one = make_engine(p, obs_dim, hidden, layers, n_act, ocfg), make_engine(p, obs_dim, hidden, layers, n_act, ocfg)
    for it in range(1, 8):
        idx = buf.sample_indices(B, seed=(77, it))
        obs, ret = ref.preprocess_with_obs(buf, buf.obs, idx, T, obs_next_rows=nxt)
        want = ref.update_with_batch(obs, buf.act[idx], ret)
        if it == 4:
            one.learn_reset()
        got = one.learn_step(buf, buf.obs, buf.act, B, T, (77, it), obs_next_rows=nxt)
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), it
        for name in ("params", "adam_m", "adam_v") + (("params_old",) if lagged else ()):
            assert torch.equal(getattr(ref, name), getattr(one, name)), (it, name)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        one.learn_step(buf, buf.obs.double(), buf.act, B, T, (77, 9))
