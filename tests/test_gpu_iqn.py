"""GPU parity of IQN on the Atari trunk -- through the C ABI (tianshou_amd.iqn), against the torch restatement of the
reference (tests/oracle_iqn.py, pinned to the unmodified reference by tests/golden/iqn_*.npz in test_oracle_iqn.py).
Tolerances are the project's own (test_gpu_distq.py): 1e-5 relative on the scale of each tensor."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from tests import oracle_iqn as OI
from tests.iqn_edge_cases import fractions_off_the_kink as _fractions_off_the_kink

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _nhwc(a):
    return torch.as_tensor(a).permute(0, 2, 3, 1).contiguous().cuda()


def _engine(c, h, w, A, seed, **kw):
    from tianshou_amd import iqn as I

    p = OI.init_params(c, h, w, A, seed=seed)
    eng = I.IQNEngine(c, h, w, A, I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], c, h, w, A), I.IQNConfig(**kw))
    return p, eng


def test_layout_and_flat_round_trip():
    from tianshou_amd import iqn as I

    c, h, w, A = 4, 84, 84, 6
    lay = I.layout(c, h, w, A)
    assert lay["F"] == 3136 and lay["ld"] == 32 and lay["total"] == I.param_count(c, h, w, A)
    assert list(np.diff(lay["off"])) == [(64 * c + 1) * 32, 513 * 64, 577 * 64, 65 * 3136, 3137 * 512, 513 * 32]
    p = OI.init_params(c, h, w, A, seed=0)
    flat = I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], c, h, w, A)
    assert flat.numel() == lay["total"]
    back = I.flat_to_torch(flat, c, h, w, A)
    for k, t in zip(OI.PARAM_ORDER, back):
        assert torch.equal(t.cpu(), p[k]), k


@pytest.mark.parametrize("A,N", [(6, 8), (3, 2), (5, 32), (64, 64)])
def test_forward_logits_q_act_vs_oracle(A, N):
    c, h, w, B = 4, 84, 84, 33
    p, eng = _engine(c, h, w, A, seed=3)
    rng = np.random.default_rng(1)
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    tau = torch.as_tensor(rng.random((B, N), dtype=np.float32))
    lg_ref, q_ref, act_ref = OI.policy_forward(p, obs, tau)
    for as_u8 in (True, False):
        x = _nhwc(obs)
        lg, q, act = eng.forward(x if as_u8 else x.float(), tau=tau.cuda())
        print("forward", A, N, as_u8, rel_err(lg.cpu(), lg_ref), rel_err(q.cpu(), q_ref))
        assert tuple(lg.shape) == (B, A, N)
        assert rel_err(lg.cpu(), lg_ref) < 1e-5
        assert rel_err(q.cpu(), q_ref) < 1e-5
        assert torch.equal(act.cpu(), act_ref)


@pytest.mark.parametrize("route", ["default", "fused", "unfused"])
def test_embed_multiply_forward_alone(route):
    """R = 33 * 5 rows (no multiple of any tile), tau = 0, tau one ulp below 1, negative pre-activations (ReLU mask); the
    one-launch kernel and the route through the generic GEMM kernels meet the same bar."""
    from tianshou_amd import iqn as I

    B, N, F, K = 33, 5, 3136, 64
    g = torch.Generator().manual_seed(7)
    tau = torch.rand((B, N), generator=g)
    tau[0, 0] = 0.0
    tau[1, 2] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    tau[32, 4] = 0.0
    feat = torch.relu(torch.randn((B, F), generator=g))
    we = torch.randn((F, K), generator=g) * 0.2
    be = torch.randn(F, generator=g) * 0.1
    p = {"emb.w": we, "emb.b": be}
    i_pi = np.pi * torch.arange(1, K + 1, dtype=torch.float32).view(1, 1, K)
    pre = torch.nn.functional.linear(torch.cos(tau.view(B, N, 1) * i_pi).view(B * N, K), we, be)
    assert (pre < 0).any() and (pre > 0).any()
    ref = (feat.unsqueeze(1) * OI.embed(p, tau)).view(B * N, F)
    we_be = torch.cat([we.t(), be.view(1, F)]).contiguous().cuda()
    x = I.embed_mul(tau.cuda(), feat.cuda(), we_be, route=route)
    print("embed forward", route, rel_err(x.cpu(), ref))
    assert rel_err(x.cpu(), ref) < 1e-5
    x2 = I.embed_mul(tau.cuda(), feat.cuda(), we_be, route=route)
    assert torch.equal(x, x2)


@pytest.mark.parametrize("route", ["default", "fused", "unfused"])
@pytest.mark.parametrize("B,N", [(33, 5), (40, 8), (3, 64), (70, 7)])
def test_embed_multiply_backward_alone(B, N, route):
    from tianshou_amd import iqn as I

    F, K = 640, 64
    g = torch.Generator().manual_seed(11 + B)
    tau = torch.rand((B, N), generator=g)
    feat = torch.relu(torch.randn((B, F), generator=g)).requires_grad_(True)
    we = (torch.randn((F, K), generator=g) * 0.2).requires_grad_(True)
    be = (torch.randn(F, generator=g) * 0.1).requires_grad_(True)
    dx = torch.randn((B * N, F), generator=g)
    x = (feat.unsqueeze(1) * OI.embed({"emb.w": we, "emb.b": be}, tau)).view(B * N, F)
    x.backward(dx)
    dfeat_ref = feat.grad * (feat.detach() > 0)
    we_be = torch.cat([we.detach().t(), be.detach().view(1, F)]).contiguous().cuda()
    dfeat, dwe = I.embed_mul_backward(tau.cuda(), feat.detach().cuda(), we_be, dx.cuda(), route=route)
    print("embed backward", route, B, N, rel_err(dfeat.cpu(), dfeat_ref), rel_err(dwe[:K].cpu(), we.grad.t()), rel_err(dwe[K].cpu(), be.grad))
    assert rel_err(dfeat.cpu(), dfeat_ref) < 1e-5
    assert rel_err(dwe[:K].cpu(), we.grad.t()) < 1e-5
    assert rel_err(dwe[K].cpu(), be.grad) < 1e-5
    dfeat2, dwe2 = I.embed_mul_backward(tau.cuda(), feat.detach().cuda(), we_be, dx.cuda(), route=route)
    assert torch.equal(dfeat, dfeat2) and torch.equal(dwe, dwe2)


def test_unfused_route_refuses_large_row_counts():
    """validated before any HIP call: the unfused route is defined below 2^14 rows"""
    from tianshou_amd import _lib
    from tianshou_amd import iqn as I

    t = torch.zeros((1 << 12, 4), device="cuda")
    with pytest.raises(_lib.EngineError, match="16384"):
        I.embed_mul(t, torch.zeros((1 << 12, 64), device="cuda"), torch.zeros((65, 64), device="cuda"), route="unfused")


@pytest.mark.parametrize("lagged", [True, False])
def test_next_dist_vs_oracle(lagged):
    from tianshou_amd import iqn as I

    c, h, w, A, N, Np, B = 2, 44, 36, 4, 5, 7, 40
    p, eng = _engine(c, h, w, A, seed=5, target_update_freq=3 if lagged else 0, online_sample_size=N, target_sample_size=Np)
    ocfg = OI.IQNConfig(target_update_freq=3 if lagged else 0)
    st = OD.DQNState.create(p, ocfg.dqn())
    if lagged:                                           # make the lagged net differ from the online one
        g = torch.Generator().manual_seed(0)
        st.params_old = {k: v + 0.02 * torch.randn(v.shape, generator=g) for k, v in p.items()}
        eng.params_old = I.flat_from_torch([st.params_old[k] for k in OI.PARAM_ORDER], c, h, w, A)
    rng = np.random.default_rng(2)
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    tau_o = torch.as_tensor(rng.random((B, N), dtype=np.float32))
    tau_t = torch.as_tensor(rng.random((B, Np), dtype=np.float32))
    ref = OI.next_dist(st, obs, tau_o, tau_t)
    out = eng.next_dist(_nhwc(obs), tau_o.cuda(), tau_t.cuda() if lagged else None)
    assert tuple(out.shape) == (B, Np if lagged else N)
    print("next_dist", lagged, rel_err(out.cpu(), ref))
    assert rel_err(out.cpu(), ref) < 1e-5


@pytest.mark.parametrize("A,N,Np,B,weighted", [(6, 8, 5, 64, True), (4, 5, 7, 37, False)])
def test_batch_gradient_vs_oracle(A, N, Np, B, weighted):
    """loss, new priorities and the whole gradient of one minibatch, layer by layer, then the Adam step."""
    from tianshou_amd import iqn as I

    c, h, w = 4, 84, 84
    rng = np.random.default_rng(9)
    p, eng = _engine(c, h, w, A, seed=4, lr=1e-4, online_sample_size=N, target_sample_size=Np)
    ocfg = OI.IQNConfig(lr=1e-4)
    st = OD.DQNState.create(p, ocfg.dqn())
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    ret = (rng.normal(size=(B, Np)) * 2.5).astype(np.float32)
    tau = _fractions_off_the_kink(p, rng, B, N)
    weight = rng.random(B).astype(np.float32) if weighted else None
    col: dict = {}
    loss_ref, prio_ref = OI.update_with_batch(st, ocfg, obs, act, ret, tau, weight=weight, collect=col)
    theta = col["logits"][torch.arange(B), torch.as_tensor(act), :]
    d = torch.as_tensor(ret).unsqueeze(1) - theta.unsqueeze(2)
    assert (d.abs() < 1).any() and (d.abs() > 1).any()                 # both Huber branches

    lay = I.layout(c, h, w, A)
    off, F, ld = lay["off"], lay["F"], lay["ld"]
    pad0 = eng.params[off[5]:].reshape(513, ld)[:, A:]
    assert float(pad0.abs().max()) == 0.0
    grad = torch.empty(eng.P, dtype=torch.float32, device="cuda")
    loss, prio = eng.update_with_batch(_nhwc(obs), act, ret, weight, tau=tau.cuda(), grad_out=grad, apply=False)
    grad_b = torch.empty_like(grad)
    loss_b, prio_b = eng.update_with_batch(_nhwc(obs), act, ret, weight, tau=tau.cuda(), grad_out=grad_b, apply=False)
    assert torch.equal(loss, loss_b) and torch.equal(prio, prio_b) and torch.equal(grad, grad_b)      # bit-identical reruns
    print("loss", float(loss), loss_ref, "prio", rel_err(prio.cpu(), prio_ref))
    assert abs(float(loss) - loss_ref) <= 1e-5 * abs(loss_ref)
    assert rel_err(prio.cpu(), prio_ref) < 1e-5
    g_ref = I.flat_from_torch([col["grads"][k] for k in OI.PARAM_ORDER], c, h, w, A, device="cpu")
    gc = grad.cpu()
    parts = {"conv1": (off[0], off[1]), "conv2": (off[1], off[2]), "conv3": (off[2], off[3]),
             "We": (off[3], off[3] + 64 * F), "be": (off[3] + 64 * F, off[4]),
             "W1": (off[4], off[4] + F * 512), "b1": (off[4] + F * 512, off[5]),
             "W2": (off[5], off[5] + 512 * ld), "b2": (off[5] + 512 * ld, off[6])}
    errs = {k: rel_err(gc[a:b], g_ref[a:b]) for k, (a, b) in parts.items()}
    print("gradient", errs)
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
    assert float(gc[off[5]:].reshape(513, ld)[:, A:].abs().max()) == 0.0      # head padding: exact zeros in the gradient
    loss2, _ = eng.update_with_batch(_nhwc(obs), act, ret, weight, tau=tau.cuda())
    assert float(loss2) == float(loss)
    pad = eng.params[off[5]:].reshape(513, ld)[:, A:]
    assert float(pad.abs().max()) == 0.0                                       # ... and in the parameters after the step
    new = torch.cat([t.reshape(-1) for t in I.flat_to_torch(eng.params, c, h, w, A)]).cpu().numpy()
    ref = torch.cat([st.params[k].reshape(-1) for k in OI.PARAM_ORDER]).numpy()
    diff = np.abs(new - ref)
    bad = diff > 1e-5 * np.abs(ref) + 0.02 * ocfg.lr
    print("adam", bad.mean(), diff.max())
    assert bad.mean() < 1e-4 and diff.max() <= 2 * ocfg.lr


@pytest.mark.parametrize("tag", ["lagged", "single"])
def test_update_sequence_matches_reference_golden(tag):
    """Replays the reference's IQN.update() sequence (sampled indices, PER weights and every fraction tensor from the
    fixture) on the engine over a DeviceReplayBuffer: n-step returns of whole quantile rows, priorities, losses, parameters."""
    from tests import iqn_common as IC
    from tianshou_amd import dqn as D
    from tianshou_amd import iqn as I
    from tianshou_amd.buffer import DeviceReplayBuffer

    g, d, ocfg, bstate = IC.load_iqn(tag)
    lagged = ocfg.target_update_freq > 0
    c, h, w, A = d["c"], d["h"], d["w"], d["n_act"]
    p, eng = _engine(c, h, w, A, seed=d["seed"], sample_size=9, online_sample_size=d["n_online"],
                     target_sample_size=d["n_target"], gamma=ocfg.gamma, n_step=ocfg.n_step,
                     target_update_freq=ocfg.target_update_freq, lr=ocfg.lr)
    buf = DeviceReplayBuffer(offset=g["buf_offset"], last_index=g["buf_last_index"], lengths=g["buf_lengths"],
                             insertion=g["buf_insertion"], rew=g["rew"], terminated=g["terminated"],
                             truncated=g["truncated"])
    frames, frames_next = torch.as_tensor(g["frames"]).cuda(), torch.as_tensor(g["frames_next"]).cuda()
    act_all = torch.as_tensor(g["act"]).cuda()
    dev = lambda a: None if a is None else torch.as_tensor(a).cuda()
    for u in range(d["n_updates"]):
        idx = torch.as_tensor(g[f"u{u}_indices"]).cuda()
        tau_o, tau_t, tau_u = IC.taus_of(g, u, lagged)
        ret = eng.preprocess(buf, frames, idx, 1, obs_next_frames=frames_next, tau_online=dev(tau_o), tau_target=dev(tau_t))
        assert tuple(ret.shape) == (d["batch"], d["n_target"] if lagged else d["n_online"])
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        obs = D.gather_obs_nhwc(frames, buf, idx, 1, as_u8=True)
        loss, prio = eng.update_with_batch(obs, act_all[idx], ret, g[f"u{u}_is_weight"], tau=dev(tau_u))
        np.testing.assert_allclose(prio.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(float(loss), float(g[f"u{u}_loss"]), rtol=1e-5)
        tensors = I.flat_to_torch(eng.params, c, h, w, A)
        flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(tensors[0].cpu().numpy(), g[f"u{u}_conv1_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(tensors[8].cpu().numpy(), g[f"u{u}_fc2_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(tensors[10].cpu().numpy().reshape(-1)[::7], g[f"u{u}_emb_w_strided"], rtol=1e-5,
                                   atol=0.02 * ocfg.lr)
        biases = torch.cat([tensors[i].reshape(-1) for i in range(1, 12, 2)]).cpu().numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-5, atol=0.02 * ocfg.lr)
        if lagged:
            old = torch.cat([t.reshape(-1) for t in I.flat_to_torch(eng.params_old, c, h, w, A)]).cpu().numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
    assert eng.adam_step == int(g["adam_step"]) and eng.tau_counter == 0          # every fraction came from the file
    m = torch.cat([t.reshape(-1) for t in I.flat_to_torch(eng.adam_m, c, h, w, A)]).cpu().numpy()
    v = torch.cat([t.reshape(-1) for t in I.flat_to_torch(eng.adam_v, c, h, w, A)]).cpu().numpy()
    _check_adam_moments(m[::61], v[::61], g)


def _check_adam_moments(m, v, g):
    """Adam moments after the fixture's three updates.  They are sums of three gradients, so the gradient bar applies: 1e-5
    of each vector's scale (m is linear in the gradients; v is quadratic: twice the relative error, 2e-5 of its scale)."""
    m_ref, v_ref = g["adam_m_strided"], g["adam_v_strided"]
    print("adam moments", np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max())
    assert np.abs(m - m_ref).max() <= 1e-5 * np.abs(m_ref).max()
    assert np.abs(v - v_ref).max() <= 2e-5 * np.abs(v_ref).max()


@pytest.mark.parametrize("tag", ["lagged", "single"])
def test_hip_iqn_update_replays_reference_golden(tag):
    """Both fixtures through the drop-in: HipIQN (make_hip_iqn over tests/standin_iqn.py) with `hip_taus=` from the file, its
    hooks called with the fixture's indices and PER weights over a host PrioritizedVectorReplayBuffer stand-in holding the
    fixture's buffer: returns, priorities, loss, and the written-back torch parameters, model_old and Adam state."""
    from tests import iqn_common as IC
    from tests import standin_iqn as SQ
    from tianshou_amd.integration import make_hip_iqn

    g, d, ocfg, _ = IC.load_iqn(tag)
    lagged = ocfg.target_update_freq > 0
    c, h, w, A, E, slots = d["c"], d["h"], d["w"], d["n_act"], d["E"], d["slots"]
    taus = []
    for u in range(d["n_updates"]):
        taus += [t for t in IC.taus_of(g, u, lagged) if t is not None]
    torch.manual_seed(d["seed"])
    net = SQ.ImplicitQuantileNetwork(preprocess_net=SQ.DQNetFeaturesOnly(c, h, w), action_shape=[A], hidden_sizes=[512])
    policy = SQ.IQNPolicy(model=net, sample_size=9, online_sample_size=d["n_online"], target_sample_size=d["n_target"])
    algo = make_hip_iqn(ref=SQ)(policy=policy, lr=ocfg.lr, gamma=ocfg.gamma, n_step_return_horizon=ocfg.n_step,
                                target_update_freq=ocfg.target_update_freq, device="cuda", hip_taus=iter(taus)).to("cuda")
    buf = SQ.PrioritizedVectorReplayBuffer(E * slots, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8,
                                           act_dtype=np.int64, alpha=0.6, beta=0.4)
    buf.obs[:], buf.obs_next[:], buf.act[:], buf.rew[:] = g["frames"], g["frames_next"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    assert np.array_equal(buf._extend_offset, g["buf_offset"])
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
        buf._lengths[e] = g["buf_lengths"][e]
        buf.last_index[e] = g["buf_last_index"][e]
    algo.policy.is_within_training_step = True
    keys = OI.TIANSHOU_KEYS
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        batch = SQ.Batch(act=buf.act[idx], weight=g[f"u{u}_is_weight"])
        batch = algo._preprocess_batch(batch, buf, idx)
        np.testing.assert_allclose(batch.returns.cpu().numpy(), g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        stat = algo._update_with_batch(batch)
        np.testing.assert_allclose(batch.weight.cpu().numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(stat.loss, float(g[f"u{u}_loss"]), rtol=1e-5)
        sd = net.state_dict()                                         # the torch modules after the write-back
        flat = torch.cat([sd[k].reshape(-1) for k in keys]).cpu().numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(sd[keys[8]].cpu().numpy(), g[f"u{u}_fc2_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        biases = torch.cat([sd[k].reshape(-1) for k in keys if k.endswith("bias")]).cpu().numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-5, atol=0.02 * ocfg.lr)
        if lagged:
            so = algo.model_old.module.state_dict()
            old = torch.cat([so[k].reshape(-1) for k in keys]).cpu().numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
    assert algo._iter == d["n_updates"] and algo.hip_extra_state()["tau_counter"] == 0      # every fraction came from the file
    with pytest.raises(StopIteration):
        algo._hip_next_tau()                                                                  # ... and all of them were used
    st = algo.optim._optim.state
    params = [dict(net.named_parameters())[k] for k in keys]
    assert all(float(st[p]["step"]) == float(g["adam_step"]) for p in params)
    m = torch.cat([st[p]["exp_avg"].reshape(-1) for p in params]).cpu().numpy()
    v = torch.cat([st[p]["exp_avg_sq"].reshape(-1) for p in params]).cpu().numpy()
    _check_adam_moments(m[::61], v[::61], g)


def test_hip_iqn_own_fraction_stream_resumes():
    """Without `hip_taus` the drop-in draws from the engine's stream; a second algorithm restored from state_dict() +
    hip_extra_state() computes the same next update (it does not replay earlier draws)."""
    from tests import iqn_common as IC
    from tests import standin_iqn as SQ
    from tianshou_amd.integration import make_hip_iqn

    g, d, ocfg, _ = IC.load_iqn("lagged")
    c, h, w, A, E, slots = d["c"], d["h"], d["w"], d["n_act"], d["E"], d["slots"]

    def make():
        torch.manual_seed(3)
        net = SQ.ImplicitQuantileNetwork(preprocess_net=SQ.DQNetFeaturesOnly(c, h, w), action_shape=[A], hidden_sizes=[512])
        policy = SQ.IQNPolicy(model=net, sample_size=9, online_sample_size=5, target_sample_size=7)
        algo = make_hip_iqn(ref=SQ)(policy=policy, lr=1e-4, gamma=0.95, n_step_return_horizon=3, target_update_freq=2,
                                    device="cuda", hip_seed=7).to("cuda")
        algo.policy.is_within_training_step = True
        return algo

    buf = SQ.PrioritizedVectorReplayBuffer(E * slots, E, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8,
                                           act_dtype=np.int64, alpha=0.6, beta=0.4)
    buf.obs[:], buf.obs_next[:], buf.act[:], buf.rew[:] = g["frames"], g["frames_next"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
        buf._lengths[e] = g["buf_lengths"][e]
        buf.last_index[e] = g["buf_last_index"][e]

    def step(algo, u):
        idx = g[f"u{u}_indices"]
        batch = SQ.Batch(act=buf.act[idx], weight=g[f"u{u}_is_weight"])
        batch = algo._preprocess_batch(batch, buf, idx)
        return algo._update_with_batch(batch).loss, batch.weight.clone()

    a = make()
    step(a, 0)
    assert a.hip_extra_state() == {"tau_seed": 7, "tau_counter": 3}
    model_state, extra = copy.deepcopy(a.state_dict()), a.hip_extra_state()      # (state_dict() holds live tensors)
    loss_a, prio_a = step(a, 1)
    b = make()
    b.load_state_dict(model_state)
    b.load_hip_extra_state(extra)
    loss_b, prio_b = step(b, 1)
    assert loss_a == loss_b and torch.equal(prio_a, prio_b)
    assert b.hip_extra_state()["tau_counter"] == 6


def test_engine_checkpoint_round_trip():
    """checkpoint.iqn_engine_state / load_iqn_engine_state: a restored engine continues bit for bit, fraction draws included."""
    from tianshou_amd import checkpoint as CK

    c, h, w, A, B = 2, 44, 36, 3, 16
    _, a = _engine(c, h, w, A, seed=1, target_update_freq=2, online_sample_size=4, target_sample_size=6, lr=1e-3)
    rng = np.random.default_rng(0)
    obs = _nhwc(rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8))
    act = rng.integers(0, A, size=B)

    def step(eng):
        ret = eng.next_dist(obs)
        return eng.update_with_batch(obs, act, ret)

    step(a)
    state = CK.iqn_engine_state(a)
    assert state["tau_counter"] == 3 and state["adam_step"] == 1 and not state["params"].is_cuda
    la, pa = step(a)
    _, b = _engine(c, h, w, A, seed=2, target_update_freq=2, online_sample_size=4, target_sample_size=6, lr=1e-3)
    CK.load_iqn_engine_state(b, state)
    lb, pb = step(b)
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(a.params, b.params) and torch.equal(a.adam_v, b.adam_v)
    assert b.tau_counter == a.tau_counter == 6 and torch.equal(a.params_old, b.params_old)


def test_uniform_fill_f32():
    from tianshou_amd import iqn as I

    n = 1 << 20
    u = I.uniform_fractions(n, seed=1234, counter=5)
    assert u.dtype == torch.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert torch.equal(u, I.uniform_fractions(n, seed=1234, counter=5))
    assert torch.equal(u[:1000], I.uniform_fractions(1000, seed=1234, counter=5))
    v = I.uniform_fractions(n, seed=1234, counter=6)
    assert float((u == v).float().mean()) < 1e-3
    assert not torch.equal(u, I.uniform_fractions(n, seed=1235, counter=5))
    assert abs(float(u.double().mean()) - 0.5) < 1e-2 and abs(float(u.double().var()) - 1.0 / 12.0) < 1e-2


def test_engine_draws_its_own_fractions_and_counts_them():
    c, h, w, A = 2, 44, 36, 3
    _, eng = _engine(c, h, w, A, seed=1)
    obs = torch.zeros((5, h, w, c), dtype=torch.uint8, device="cuda")
    eng.forward(obs)
    t0 = eng.last_tau.clone()
    assert tuple(t0.shape) == (5, eng.cfg.sample_size) and eng.tau_counter == 1
    eng.forward(obs)
    assert eng.tau_counter == 2 and not torch.equal(t0, eng.last_tau)
    state = eng.extra_state()
    eng.forward(obs)
    t2 = eng.last_tau.clone()
    eng.load_extra_state(state)                          # a restored counter continues the stream: same next draw
    eng.forward(obs)
    assert torch.equal(t2, eng.last_tau)


def test_limits_are_reported():
    from tianshou_amd import _lib
    from tianshou_amd import iqn as I

    with pytest.raises(ValueError):
        I.param_count(4, 84, 84, 65)
    with pytest.raises(ValueError):
        I.param_count(4, 84, 84, 6, n_cos=32)
    _, eng = _engine(2, 44, 36, 3, seed=1)
    obs = torch.zeros((4, 44, 36, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        eng.forward(obs, tau=torch.rand(4, 65).cuda())
    with pytest.raises(_lib.EngineError, match="sample size"):          # validated before any HIP call
        _lib.check(_lib.load().ts_iqn_forward(
            eng._ws.handle, _lib.ptr(eng.params), *eng._dims(), _lib.ptr(obs), 1, _lib.i64(4), _lib.ptr(torch.rand(4, 1).cuda()),
            _lib.i64(1), None, None, None, _lib.current_stream(eng.device)))
