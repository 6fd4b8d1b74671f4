"""GPU parity of behaviour cloning on the three routes of tianshou_amd/bc.py -- through the C ABI, against the torch restatement
of the reference (tests/oracle_bc.py, pinned to the unmodified reference by tests/golden/bc_*.npz in test_oracle_bc.py) and
through the Hip imitation classes over tests/standin_bc.py.
Tolerances are the project's own (test_gpu_dqn.py / test_gpu_td3.py): 1e-5 relative on the scale of each tensor; the Adam step
under test_gpu_dcql.py's rule."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from oracle import oracle_sac as OS
from tests import bc_common as CC
from tests import oracle_bc as OB

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _nhwc(a):
    return torch.as_tensor(a).permute(0, 2, 3, 1).contiguous().cuda()


class _Route:
    """One route at one shape: the oracle's parameters, the engine, the flat converters and the layer bounds."""

    def __init__(self, kind, *, seed=4, c=2, h=44, w=36, n_out=3, obs_dim=4, hidden=(64, 64), activation="relu", max_action=1.0,
                 params=None, **cfg):
        from tianshou_amd import bc as BC
        from tianshou_amd import dqn as D
        from tianshou_amd import dsac
        from tianshou_amd.sac import mlp_layout

        self.kind, self.max_action, self.activation, self.cfg = kind, max_action, activation, cfg
        if kind == "dqnet":
            self.order = OD.PARAM_ORDER
            self.p = OD.init_params(c, h, w, n_out, seed) if params is None else params
            dims = (c, h, w, n_out)
            self.flat = lambda d, dev="cuda": D.flat_from_torch([d[k] for k in self.order], *dims, device=dev)
            self.unflat = lambda f: D.flat_to_torch(f, *dims)
            self.eng = BC.BCDQNetEngine(*dims, self.flat(self.p), BC.BCConfig(**cfg))
            self.bounds = [int(x) for x in D.layer_layout(c, h, w, 1)[0][:5]] + [self.eng.P]
        else:
            depth, H = len(hidden), max(hidden)
            self.order = OB.mlp_order(depth)
            self.p = OB.init_mlp_params(obs_dim, n_out, hidden, seed) if params is None else params
            self.flat = lambda d, dev="cuda": BC.mlp_flat_from_torch(kind, [d[k] for k in self.order], obs_dim, n_out, H, dev)
            self.unflat = lambda f: BC.mlp_flat_to_torch(kind, f, obs_dim, n_out, H, depth=depth)
            self.eng = BC.BCMlpEngine(kind, obs_dim, n_out, self.flat(self.p), BC.BCConfig(max_action=max_action, **cfg), hidden=H,
                                      depth=depth, activation=activation)
            offs = mlp_layout(obs_dim, H, depth, 32)[1] if kind == "continuous" else dsac.layout(obs_dim, n_out, H, depth)["offs"]
            self.bounds = [int(x) for x in offs]
        self.ocfg = OD.DQNConfig(lr=cfg.get("lr", 1e-3), max_grad_norm=cfg.get("max_grad_norm"))

    def obs_dev(self, obs):
        return _nhwc(obs) if self.kind == "dqnet" else torch.as_tensor(obs).cuda()

    def oracle(self):
        return OS.activation(self.activation)

    def params_np(self, flat):
        return torch.cat([t.reshape(-1) for t in self.unflat(flat)]).cpu().numpy()


def _check_update(r: _Route, obs, act):
    """Loss and the whole gradient layer by layer against the oracle, bit-identical reruns, a pre-filled grad_out written
    everywhere, then the Adam step (with the route's max_grad_norm)."""
    st = OD.DQNState.create(r.p, r.ocfg)
    col: dict = {}
    with r.oracle():
        loss_ref = OB.update_with_batch(st, r.ocfg, r.kind, obs, act, r.max_action, collect=col)
    eng = r.eng
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    loss = eng.update_with_batch(r.obs_dev(obs), act, grad_out=grad, apply=False)
    grad_b = torch.empty_like(grad)
    loss_b = eng.update_with_batch(r.obs_dev(obs), act, grad_out=grad_b, apply=False)
    assert torch.equal(loss, loss_b) and torch.equal(grad, grad_b)                    # bit-identical reruns
    assert eng.adam_step == 0 and tuple(loss.shape) == (1,)
    got = float(loss)
    print("loss", got, loss_ref)
    assert abs(got - loss_ref) <= 1e-5 * abs(loss_ref) if loss_ref != 0.0 else got == 0.0
    g_ref = r.flat(col["grads"], "cpu")
    gc = grad.cpu()
    assert not bool((gc == SENTINEL).any())
    b = r.bounds
    errs = [rel_err(gc[b[i]:b[i + 1]], g_ref[b[i]:b[i + 1]]) for i in range(len(b) - 1)]
    print("gradient", errs)
    for i, e in enumerate(errs):
        assert e < 1e-5, f"layer {i}: {e}"
    loss2 = eng.update_with_batch(r.obs_dev(obs), act)
    assert torch.equal(loss2, loss) and eng.adam_step == 1
    new, ref = r.params_np(eng.params), CC.flat(st.params, r.order)
    diff = np.abs(new - ref)
    bad = diff > 1e-5 * np.abs(ref) + 0.02 * r.ocfg.lr
    print("adam", bad.mean(), diff.max())
    assert bad.mean() < 1e-4 and diff.max() <= 2 * r.ocfg.lr
    return gc


@pytest.mark.parametrize("A", [1, 3, 33, 64])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_dqnet_update_vs_oracle(A, B):
    rng = np.random.default_rng(9 + A + B)
    clip = 0.5 if (A + B) % 2 else None                       # max_grad_norm on and off across the grid
    r = _Route("dqnet", n_out=A, lr=1e-4, max_grad_norm=clip)
    obs = rng.integers(0, 256, size=(B, 2, 44, 36), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    gc = _check_update(r, obs, act)
    head = gc[r.bounds[4]:].reshape(513, A)
    if A > 1:                                                 # the dense gradient reaches every action's column, taken or not
        assert bool((head[512] != 0).all())
    else:
        assert not gc.any()                                   # one action: softmax = onehot, exactly


@pytest.mark.parametrize("u8", [True, False])
def test_dqnet_atari_shape(u8):
    rng = np.random.default_rng(21)
    r = _Route("dqnet", c=4, h=84, w=84, n_out=6, lr=1e-4, max_grad_norm=None if u8 else 10.0)
    obs = rng.integers(0, 256, size=(32, 4, 84, 84), dtype=np.uint8)
    _check_update(r, obs if u8 else obs.astype(np.float32), rng.integers(0, 6, size=32))


@pytest.mark.parametrize("obs_dim,hidden,A,B,clip", [(4, (64, 64), 2, 37, None), (5, (32,), 33, 5, 0.3)])
def test_discrete_mlp_update_vs_oracle(obs_dim, hidden, A, B, clip):
    """A = 33 runs on the 64-column head (the documented limit is 2 .. 64 logits)."""
    rng = np.random.default_rng(31 + A)
    r = _Route("discrete", obs_dim=obs_dim, hidden=hidden, n_out=A, lr=1e-3, max_grad_norm=clip)
    gc = _check_update(r, rng.normal(size=(B, obs_dim)).astype(np.float32), rng.integers(0, A, size=B))
    hw = (A + 31) // 32 * 32
    head = gc[r.bounds[-2]:].reshape(-1, hw)
    assert not head[:, A:].any()                               # padding columns of the head gradient: exact zeros


def test_discrete_mlp_head_limits_are_refused():
    from tianshou_amd import bc as BC

    for n_out in (1, 65):
        with pytest.raises(NotImplementedError, match="2 .. 64 outputs"):
            BC.BCMlpEngine("discrete", 4, n_out, torch.zeros(8, device="cuda"), BC.BCConfig(), hidden=32, depth=1)
    with pytest.raises(NotImplementedError, match="1 .. 32 outputs"):
        BC.BCMlpEngine("continuous", 4, 33, torch.zeros(8, device="cuda"), BC.BCConfig(), hidden=32, depth=1)


@pytest.mark.parametrize("obs_dim,hidden,A,B,act_fn,m,clip", [(17, (256, 256), 6, 37, "relu", 2.5, None),
                                                              (17, (256, 256), 6, 5, "relu", 1.0, 0.05),
                                                              (3, (32,), 1, 5, "tanh", 1.0, None)])
def test_continuous_mlp_update_vs_oracle(obs_dim, hidden, A, B, act_fn, m, clip):
    rng = np.random.default_rng(41 + B)
    r = _Route("continuous", obs_dim=obs_dim, hidden=hidden, n_out=A, activation=act_fn, max_action=m, lr=1e-3, max_grad_norm=clip)
    obs = rng.normal(size=(B, obs_dim)).astype(np.float32)
    gc = _check_update(r, obs, rng.uniform(-m, m, size=(B, A)).astype(np.float32))
    head = gc[r.bounds[-2]:].reshape(-1, 32)
    assert not head[:, A:].any()


@pytest.mark.parametrize("case", list(CC.CASES))
def test_update_sequence_matches_reference_golden(case):
    """Replays the reference's update sequence (the sampled indices from the fixture) on the engine: losses, parameters, moments."""
    s = CC.load(case)
    g, tag = s.g, s.tag
    if s.route == "dqnet":
        r = _Route("dqnet", c=s.c, h=s.h, w=s.w, n_out=s.n_act, params=s.params0, lr=s.lr)
    else:
        r = _Route(s.route, obs_dim=s.obs_dim, hidden=s.hidden, n_out=s.n_out, max_action=s.max_action, params=s.params0, lr=s.lr)
    obs_all, act_all = r.obs_dev(s.obs), torch.as_tensor(s.act).cuda()
    for u in range(s.n_updates):
        idx = torch.as_tensor(g[f"{tag}u{u}_indices"]).cuda()
        loss = r.eng.update_with_batch(obs_all[idx], act_all[idx])
        np.testing.assert_allclose(float(loss), float(g[f"{tag}u{u}_loss"]), rtol=1e-5)
        tensors = r.unflat(r.eng.params)
        flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
        np.testing.assert_allclose(flat[::CC.STRIDE], g[f"{tag}u{u}_params_strided"], rtol=1e-5, atol=0.02 * s.lr)
        biases = torch.cat([tensors[i].reshape(-1) for i in range(1, len(tensors), 2)]).cpu().numpy()
        np.testing.assert_allclose(biases, g[f"{tag}u{u}_biases"], rtol=1e-5, atol=0.02 * s.lr)
    assert r.eng.adam_step == int(g[f"{tag}adam_step"])
    m, v = r.params_np(r.eng.adam_m)[::CC.STRIDE], r.params_np(r.eng.adam_v)[::CC.STRIDE]
    m_ref, v_ref = g[f"{tag}adam_m_strided"], g[f"{tag}adam_v_strided"]
    # sums of a few gradients: the gradient bar, 1e-5 of each vector's scale (v is quadratic in them: 2e-5)
    assert np.abs(m - m_ref).max() <= 1e-5 * np.abs(m_ref).max()
    assert np.abs(v - v_ref).max() <= 2e-5 * np.abs(v_ref).max()


def test_forward_matches_the_torch_module_and_takes_the_first_maximum():
    rng = np.random.default_rng(5)
    # DQNet: actions 0 and 1 share their head weights and carry the largest bias -> a tie in every row
    p = OD.init_params(2, 44, 36, 4, 3)
    p["fc2.w"][1], p["fc2.b"][1] = p["fc2.w"][0], p["fc2.b"][0]
    p["fc2.b"][:2] += 50.0
    r = _Route("dqnet", n_out=4, params=p)
    obs = rng.integers(0, 256, size=(6, 2, 44, 36), dtype=np.uint8)
    logits, act = r.eng.forward(_nhwc(obs))
    ref, act_ref = OB.policy_forward("dqnet", p, obs)
    assert rel_err(logits.cpu(), ref) < 1e-5 and torch.equal(logits[:, 0], logits[:, 1])
    assert act.cpu().tolist() == act_ref.tolist() == [0] * 6 and act.dtype == torch.int64
    # discrete MLP: the same construction on the 33-logit head; the last two columns tie as well and lose
    p = OB.init_mlp_params(5, 33, (32,), 3)
    p["wa"][8], p["ba"][8] = p["wa"][7], p["ba"][7]
    p["ba"][7:9] += 50.0
    r = _Route("discrete", obs_dim=5, hidden=(32,), n_out=33, params=p)
    x = rng.normal(size=(7, 5)).astype(np.float32)
    logits, act = r.eng.forward(torch.as_tensor(x).cuda())
    ref, act_ref = OB.policy_forward("discrete", p, x)
    assert tuple(logits.shape) == (7, 33) and rel_err(logits.cpu(), ref) < 1e-5
    assert torch.equal(logits[:, 7], logits[:, 8]) and act.cpu().tolist() == act_ref.tolist() == [7] * 7
    # continuous: max_action * tanh(head)
    p = OB.init_mlp_params(17, 6, (256, 256), 3)
    r = _Route("continuous", obs_dim=17, hidden=(256, 256), n_out=6, max_action=2.5, params=p)
    x = rng.normal(size=(9, 17)).astype(np.float32)
    a = r.eng.forward(torch.as_tensor(x).cuda())
    assert tuple(a.shape) == (9, 6) and rel_err(a.cpu(), OB.policy_forward("continuous", p, x, 2.5)[0]) < 1e-5


def test_from_module_and_to_module_round_trip():
    from tests import standin_bc as SB
    from tianshou_amd import bc as BC

    torch.manual_seed(2)
    net = SB.DQNet(2, 44, 36, 3)
    eng = BC.BCDQNetEngine.from_module(net, 2, 44, 36, BC.BCConfig())
    want = [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    eng.to_module(net)
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), want))
    for mode, actor in (("discrete", SB.ActionNet(5, 33, [48, 32])), ("continuous", SB.ContinuousActorDeterministic(SB.Net(7, [64]), 3))):
        params = list(actor.parameters())
        eng = BC.BCMlpEngine.from_module(mode, params, BC.BCConfig())
        want = [p.detach().clone() for p in params]
        with torch.no_grad():
            for p in params:
                p.zero_()
        eng.to_module(params)
        assert all(torch.equal(a, b) for a, b in zip(params, want)) and eng.hidden in (64,)


def _make_algo(case, offline: bool, write_back: str, max_grad_norm=None):
    from tests import standin_bc as SB
    from tianshou_amd.integration import make_hip_imitation

    s = CC.load(case)
    torch.manual_seed(s.seed)
    if s.route == "dqnet":
        actor, space = SB.DQNet(s.c, s.h, s.w, s.n_act), SB.Discrete(s.n_act)
    elif s.route == "discrete":
        actor, space = SB.ActionNet(s.obs_dim, s.n_out, list(s.hidden)), SB.Discrete(s.n_out)
    else:
        actor = SB.ContinuousActorDeterministic(SB.Net(s.obs_dim, list(s.hidden)), s.n_out, s.max_action)
        space = SB.Box(-s.max_action, s.max_action, (s.n_out,))
    for p, k in zip(actor.parameters(), s.order):                # same construction order: the fixture's seeded initial net
        assert torch.equal(p.detach(), s.params0[k]), k
    policy = SB.ImitationPolicy(actor=actor, action_space=space)
    algo = make_hip_imitation(offline, ref=SB)(policy=policy, lr=s.lr, max_grad_norm=max_grad_norm, device="cuda",
                                               write_back=write_back)
    return SB, s, algo, actor


@pytest.mark.parametrize("case,offline,write_back", [("atari", True, "lazy"), ("cartpole", False, "eager"), ("d4rl_b", True, "lazy")])
def test_hip_imitation_over_the_standins(case, offline, write_back):
    """The drop-in on the real engine: the fixture's updates through `_update_with_batch` (losses as the reference's), lazy
    write-back leaves the torch modules alone until `state_dict()`, which then equals the engine's parameters; one more update
    through `update()` on a host buffer."""
    SB, s, algo, actor = _make_algo(case, offline, write_back)
    g, tag = s.g, s.tag
    before = [p.detach().clone() for p in actor.parameters()]
    for u in range(s.n_updates):
        idx = g[f"{tag}u{u}_indices"]
        stats = algo._update_with_batch(SB.Batch(obs=s.obs[idx], act=s.act[idx]))
        assert type(stats) is SB.ImitationTrainingStats
        np.testing.assert_allclose(stats.loss, float(g[f"{tag}u{u}_loss"]), rtol=1e-5)
    eng = algo._hip_engine
    assert eng.adam_step == s.n_updates
    stale = all(torch.equal(p.detach(), q) for p, q in zip(actor.parameters(), before))
    assert stale == (write_back == "lazy")
    sd = algo.state_dict()
    keys = algo._hip_route.keys
    from tianshou_amd import bc as BC
    from tianshou_amd import dqn as D

    if s.route == "dqnet":
        want = D.flat_to_torch(eng.params, s.c, s.h, s.w, s.n_act)
    else:
        want = BC.mlp_flat_to_torch(s.route, eng.params, s.obs_dim, s.n_out, eng.hidden, sizes=s.hidden)
    for k, t in zip(keys, want):
        assert torch.equal(sd["policy.actor." + k].cpu(), t.cpu()), k
    flat = torch.cat([sd["policy.actor." + k].reshape(-1) for k in keys]).cpu().numpy()
    np.testing.assert_allclose(flat[::CC.STRIDE], g[f"{tag}u{s.n_updates - 1}_params_strided"], rtol=1e-5, atol=0.02 * s.lr)
    opt = algo.optim._optim
    st0 = opt.state[next(iter(actor.parameters()))]
    assert int(float(st0["step"])) == s.n_updates and "exp_avg" in st0
    # update() on a host buffer: sample, the base class's _preprocess_batch, the engine, statistics
    kw = dict(obs_shape=s.obs.shape[1:], act_shape=s.act.shape[1:], obs_dtype=s.obs.dtype, act_dtype=s.act.dtype)
    buf = SB.VectorReplayBuffer(len(s.obs), 2, **kw)
    buf.obs[:], buf.act[:] = s.obs, s.act
    for e, sb in enumerate(buf.buffers):
        sb._size = sb.maxsize
        buf._lengths[e] = sb.maxsize
    algo.policy.is_within_training_step = True
    stats = algo.update(buf, s.batch)
    assert np.isfinite(stats.loss) and algo._hip_engine.adam_step == s.n_updates + 1


def test_hip_imitation_reads_max_grad_norm_and_lr_at_every_update():
    SB, s, algo, actor = _make_algo("cartpole", False, "eager", max_grad_norm=1e-3)
    idx = s.g["u0_indices"]
    batch = SB.Batch(obs=s.obs[idx], act=s.act[idx])
    algo._update_with_batch(batch)
    eng = algo._hip_engine
    assert eng.cfg.max_grad_norm == 1e-3 and eng.cfg.lr == s.lr
    st = OD.DQNState.create(s.params0, OD.DQNConfig(lr=s.lr, max_grad_norm=1e-3))
    OB.update_with_batch(st, OD.DQNConfig(lr=s.lr, max_grad_norm=1e-3), "discrete", s.obs[idx], s.act[idx])
    got = torch.cat([p.detach().reshape(-1) for p in actor.parameters()]).numpy()
    assert np.abs(got - CC.flat(st.params, s.order)).max() <= 0.02 * s.lr + 1e-5 * np.abs(got).max()
    algo.optim._optim.param_groups[0]["lr"] = 5e-4
    algo.optim._max_grad_norm = None
    algo._update_with_batch(batch)
    assert eng.cfg.lr == 5e-4 and eng.cfg.max_grad_norm is None and algo._hip_engine is eng
