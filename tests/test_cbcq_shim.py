"""CPU: the HipBCQ drop-in (tianshou_amd.integration.make_hip_bcq) without an engine -- over the real reference classes where the
reference is mounted, over tests/standin_cbcq.py otherwise: the class it builds, the config it hands the engine, the rows and
draws of an update, write-back and the state_dict round trip; the argument checks of the ts_cbcq_* entry points, which run before
any HIP call, and ts_cbcq_layout against offsets computed by hand."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_cbcq as SB

REAL = ref_shim.reference_available()
OBS, ACT, LAT = 11, 3, 6


def _real_parts(hidden=(256, 256), vae_hidden=(512, 512), pert_net="mlp", activation=nn.ReLU, max_action=1.0, phi=0.05):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.imitation.bcq import BCQPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import MLP, Net
    from tianshou.utils.net.continuous import VAE, ContinuousCritic, Perturbation

    if pert_net == "mlp":
        net_a = MLP(input_dim=OBS + ACT, output_dim=ACT, hidden_sizes=list(hidden), activation=activation)
    else:
        net_a = Net(state_shape=(OBS + ACT,), action_shape=(ACT,), hidden_sizes=list(hidden), activation=activation)
    actor = Perturbation(preprocess_net=net_a, max_action=max_action, phi=phi)
    mk = lambda: Net(state_shape=(OBS,), action_shape=(ACT,), hidden_sizes=list(hidden), concat=True, activation=activation)  # noqa: E731
    n1, n2 = mk(), mk()
    c1, c2 = ContinuousCritic(preprocess_net=n1), ContinuousCritic(preprocess_net=n2)
    enc = MLP(input_dim=OBS + ACT, hidden_sizes=list(vae_hidden))
    dec = MLP(input_dim=OBS + LAT, output_dim=ACT, hidden_sizes=list(vae_hidden))
    vae = VAE(encoder=enc, decoder=dec, hidden_dim=vae_hidden[-1], latent_dim=LAT, max_action=max_action)
    policy = BCQPolicy(actor_perturbation=actor, action_space=gym.spaces.Box(low=-max_action, high=max_action, shape=(ACT,)), critic=c1,
                       vae=vae)
    return dict(policy=policy, actor_perturbation_optim=AdamOptimizerFactory(lr=3e-4), critic_optim=AdamOptimizerFactory(lr=1e-3),
                critic2=c2, critic2_optim=AdamOptimizerFactory(lr=5e-4), vae_optim=AdamOptimizerFactory(lr=2e-3))


def _fake_parts(**kw):
    return SB.build(OBS, ACT, LAT, actor_perturbation_lr=3e-4, critic_lr=1e-3, critic2_lr=5e-4, vae_lr=2e-3, **kw)


def _make(net_kw=None, **kw):
    from tianshou_amd.integration import make_hip_bcq

    net_kw = net_kw or {}
    if REAL:
        parts = _real_parts(**net_kw)                   # (installs the shim that makes the reference importable)
        return make_hip_bcq()(device="cpu", update_noise="torch", **parts, **kw)
    return make_hip_bcq(ref=SB)(device="cpu", update_noise="torch", **_fake_parts(**net_kw), **kw)


def test_class_and_hyper_parameters_are_carried():
    algo = _make(lmbda=0.6, gamma=0.9, tau=0.01, num_sampled_action=4)
    assert type(algo).__name__ == "HipBCQ" and [p.name for p in algo._hip_parts()] == ["pert", "critic1", "critic2", "vae"]
    assert [p.old is None for p in algo._hip_parts()] == [False, False, False, True]
    algo.critic_optim._max_grad_norm = 0.5
    f = algo._hip_cbcq_fields()
    assert (f["lmbda"], f["gamma"], f["tau"], f["num_sampled_action"], f["phi"], f["max_action"], f["forward_sampled_times"]) == \
        (0.6, 0.9, 0.01, 4, 0.05, 1.0, 100)
    assert (f["pert_lr"], f["critic1_lr"], f["critic2_lr"], f["vae_lr"]) == (3e-4, 1e-3, 5e-4, 2e-3)
    assert (f["critic1_max_grad_norm"], f["critic2_max_grad_norm"], f["pert_max_grad_norm"], f["vae_max_grad_norm"]) == (0.5, 0.0, 0.0, 0.0)
    assert f["pert_first_row"] is True and f["betas"] == (0.9, 0.999) and f["adam_eps"] == 1e-8
    assert (algo._hip_obs_dim, algo._hip_act_dim, algo._hip_latent, algo._hip_hidden, algo._hip_vhidden, algo._hip_depth, algo._hip_vdepth) == \
        (OBS, ACT, LAT, 256, 512, 2, 2)
    other = _make(net_kw=dict(hidden=(64, 48, 40), vae_hidden=(96, 72), pert_net="net", activation=nn.Tanh, max_action=2.0, phi=0.3))
    g = other._hip_cbcq_fields()
    assert g["pert_first_row"] is False and (g["phi"], g["max_action"]) == (0.3, 2.0)
    assert (other._hip_hidden, other._hip_vhidden, other._hip_depth, other._hip_vdepth, other._hip_actfn, other._hip_vactfn) == \
        (64, 96, 3, 2, "tanh", "relu")
    from tianshou_amd.integration import make_hip_bcq

    with pytest.raises(ValueError):
        make_hip_bcq(ref=SB)(device="cpu", update_noise="numpy", **_fake_parts())


def test_unsupported_networks_are_refused_with_a_sentence():
    from tianshou_amd.integration import make_hip_bcq

    parts = _fake_parts()
    parts["policy"].vae.encoder.model[1] = nn.Sigmoid()
    with pytest.raises(NotImplementedError, match="MLP / Net trunk of 1 .. 6 hidden Linear layers"):
        make_hip_bcq(ref=SB)(device="cpu", **parts)
    parts = _fake_parts()
    parts["policy"].critic.last = SB.MLP(input_dim=256, output_dim=1, hidden_sizes=[8])
    with pytest.raises(NotImplementedError, match="single Linear layer"):
        make_hip_bcq(ref=SB)(device="cpu", **parts)
    with pytest.raises(NotImplementedError, match="one depth and one activation"):
        make_hip_bcq(ref=SB)(device="cpu", **SB.build(OBS, ACT, LAT, hidden=(64, 64), pert_net="mlp") | dict(
            critic2=SB.ContinuousCritic(SB.Net(OBS + ACT, [64, 64, 64]))))


def test_engine_config_and_layout_by_hand():
    """ts_cbcq_layout against offsets computed by hand for (obs 11, act 3, L 6) at the defaults and (obs 17, act 6, L 12, vae 512)
    at hidden 64 / depth 3; the hyper-parameter vector in TS_CBCQ_HP_* order."""
    from tianshou_amd import cbcq as Q
    from tianshou_amd.sac import MLPTrunk

    cfg = Q.CBCQConfig()
    assert (cfg.gamma, cfg.tau, cfg.lmbda, cfg.phi, cfg.num_sampled_action, cfg.forward_sampled_times) == (0.99, 0.005, 0.75, 0.05, 10, 100)
    assert list(cfg.to_c()) == [1e-3, 1e-3, 1e-3, 1e-3, 0.9, 0.999, 1e-8, 0.005, 0.99, 0.75, 0.05, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert list(Q.CBCQConfig(vae_lr=-1.0, pert_lr=2e-3).to_c(0.5))[:4] == [1e-3, 5e-4, 5e-4, -1.0]
    lay = Q.layout(11, 3, 6, MLPTrunk(256, 2, "relu"), MLPTrunk(512, 2, "relu"))
    kc, kd, lp = 32, 32, 32                                 # pad32(14), pad32(17), pad32(6)
    critic = (kc + 1) * 256 + 257 * 256 + 257 * 32
    enc = (kc + 1) * 512 + 513 * 512 + 513 * 2 * lp
    dec = (kd + 1) * 512 + 513 * 512 + 513 * 32
    assert lay == dict(kc=kc, kd=kd, lp=lp, pert_count=critic, critic_count=critic, encoder_count=enc, decoder_count=dec,
                       vae_count=enc + dec, critic_head=(kc + 1) * 256 + 257 * 256, encoder_head=(kc + 1) * 512 + 513 * 512,
                       decoder=enc, decoder_head=enc + (kd + 1) * 512 + 513 * 512)
    lay = Q.layout(17, 6, 12, MLPTrunk(64, 3, "tanh"), MLPTrunk(512, 2, "relu"))
    critic = 33 * 64 + 2 * 65 * 64 + 65 * 32                # kc = pad32(23) = 32
    enc = 33 * 512 + 513 * 512 + 513 * 64                   # lp = 32
    dec = 33 * 512 + 513 * 512 + 513 * 32                   # kd = pad32(29) = 32
    assert (lay["kc"], lay["kd"], lay["lp"], lay["critic_count"], lay["encoder_count"], lay["decoder_count"]) == (32, 32, 32, critic, enc, dec)
    assert lay["critic_head"] == 33 * 64 + 2 * 65 * 64 and lay["decoder_head"] == enc + 33 * 512 + 513 * 512
    lay = Q.layout(40, 6, 40, MLPTrunk(64, 1, "relu"), MLPTrunk(96, 1, "relu"))
    assert (lay["kc"], lay["kd"], lay["lp"], lay["encoder_count"]) == (64, 96, 64, 65 * 96 + 97 * 128)


def test_converters_round_trip_and_place_the_heads():
    """The flat VAE vector: `mean` in head columns [0, L), `log_std` in [lp, lp + L), the decoder behind the encoder; unequal
    widths are embedded by zero padding and come back unchanged."""
    from tianshou_amd import cbcq as Q
    from tests import cbcq_common as BC
    from tests import oracle_cbcq as OB

    pert, c1, c2, vae = OB.init_params(OBS, ACT, LAT, 3, (48, 64), (40, 72))
    enc, dec = BC.vae_lists(vae)
    flat = Q.vae_flat_from_torch(enc, dec, OBS, ACT, LAT, device="cpu")
    n_enc = 33 * 96 + 97 * 96 + 97 * 64
    assert flat.numel() == n_enc + 33 * 96 + 97 * 96 + 97 * 32
    head = flat[33 * 96 + 97 * 96: n_enc].reshape(97, 64)
    assert torch.equal(head[:72, :LAT], vae["wmean"].t()) and torch.equal(head[96, 32:32 + LAT], vae["bls"])
    assert not head[:, LAT:32].any() and not head[:, 32 + LAT:].any() and not head[72:96].any()
    e2, d2 = Q.vae_flat_to_torch(flat, OBS, ACT, LAT, 96, 2, (40, 72), (40, 72))
    for a, b in zip(e2 + d2, enc + dec):
        assert torch.equal(a, b)
    pf = Q.pert_flat_from_torch(list(pert.values()), OBS, ACT, device="cpu")
    for a, b in zip(Q.pert_flat_to_torch(pf, OBS, ACT, 64, 2, (48, 64)), pert.values()):
        assert torch.equal(a, b)


class _FakeEngine:
    """tianshou_amd.cbcq.CBCQEngine's interface on the CPU: every update adds 2 to the perturbation net, 1.5 to the lagged
    critic 2, 1 to the VAE and 0.125 to the VAE's first Adam moment."""

    seen: dict = {}

    def __init__(self, obs_dim, act_dim, latent_dim, pert, c1, c2, vae, cfg, hidden=256, depth=2, activation="relu", vae_hidden=512,
                 vae_depth=2, vae_activation="relu"):
        from tianshou_amd import cbcq as Q

        assert isinstance(cfg, Q.CBCQConfig) and (obs_dim, act_dim, latent_dim, hidden, depth, vae_hidden, vae_depth) == (OBS, ACT, LAT, 256, 2, 512, 2)
        assert (activation, vae_activation, cfg.pert_first_row, cfg.num_sampled_action) == ("relu", "relu", True, 3)
        self.obs_dim, self.act_dim, self.latent_dim, self.cfg, self.adam_step = obs_dim, act_dim, latent_dim, cfg, 0
        self.pert, self.critic1, self.critic2, self.vae = pert.clone(), c1.clone(), c2.clone(), vae.clone()
        self.pert_old, self.critic1_old, self.critic2_old = pert.clone(), c1.clone(), c2.clone()
        for n in ("pert", "critic1", "critic2", "vae"):
            setattr(self, n + "_m", torch.zeros_like(getattr(self, n)))
            setattr(self, n + "_v", torch.zeros_like(getattr(self, n)))

    def update_with_batch(self, obs, act, rew, done, obs_next, e1, e2, e3):
        s = type(self).seen
        assert obs.shape == obs_next.shape == (8, OBS) and act.shape == (8, ACT) and rew.shape == done.shape == (8,)
        assert rew.dtype == done.dtype == torch.float32
        s.setdefault("lmbda", []).append(self.cfg.lmbda)
        s.setdefault("lr", []).append(self.cfg.critic2_lr)
        s.update(obs=obs.clone(), rew=rew.clone(), done=done.clone(), obs_next=obs_next.clone(), draws=[t.clone() for t in (e1, e2, e3)])
        self.adam_step += 1
        self.pert += 2.0
        self.critic2_old += 1.5
        self.vae += 1.0
        self.vae_m += 0.125
        return torch.tensor([0.1, 0.2, 0.3, 0.4])


def test_hip_bcq_wrapper_runs_with_engine_double(monkeypatch):
    """Two update() calls of HipBCQ over a CPU double of CBCQEngine: the config, the hyper-parameters and learning rates re-read
    at every update, the rows gathered by index (`done`, not `terminated`), the three draws in the reference's order and shapes
    from torch's generator, the statistics' type, the write-back of parameters, lagged networks and Adam state, and the
    state_dict() / load_state_dict() round trip into a second instance whose rebuilt engine continues from it."""
    import tianshou_amd.cbcq as Q
    from tests.test_integration_shim import _patch_for_cpu

    if REAL:
        from tianshou.data import Batch, VectorReplayBuffer
        from tianshou.utils.torch_utils import policy_within_training_step as training
        buf = VectorReplayBuffer(32, 2)
    else:
        import contextlib

        Batch = SB.Batch
        buf = SB.VectorReplayBuffer(32, 2, obs_shape=(OBS,), act_shape=(ACT,))

        @contextlib.contextmanager
        def training(policy):
            policy.is_within_training_step = True
            yield
            policy.is_within_training_step = False

    R = 3
    _FakeEngine.seen = seen = {}
    algo = _make(num_sampled_action=R)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(Q, "CBCQEngine", _FakeEngine)
    rng = np.random.default_rng(0)
    for t in range(16):
        buf.add(Batch(obs=rng.normal(size=(2, OBS)).astype(np.float32), act=rng.normal(size=(2, ACT)).astype(np.float32),
                      rew=rng.normal(size=2), terminated=np.array([t % 5 == 4, False]), truncated=np.array([False, t % 3 == 2]),
                      obs_next=rng.normal(size=(2, OBS)).astype(np.float32)))
    assert (np.asarray(buf.done) != np.asarray(buf.terminated)).any()
    p_first = next(iter(algo.policy.actor_perturbation.parameters()))
    old_first = next(iter(algo.critic2_target.module.parameters()))
    pert_old_first = next(iter(algo.actor_perturbation_target.module.parameters()))
    v_first = next(iter(algo.policy.vae.parameters()))
    before = [t.detach().clone() for t in (p_first, old_first, pert_old_first, v_first)]
    with training(algo.policy):
        torch.manual_seed(5)
        stats = algo.update(buffer=buf, sample_size=8)
        idx = algo._hip_idx.numpy()
        assert type(stats).__name__ == "BCQTrainingStats"
        assert [round(x, 6) for x in (stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.vae_loss)] == [0.1, 0.2, 0.3, 0.4]
        np.testing.assert_array_equal(seen["obs"].numpy(), np.asarray(buf.obs)[idx])
        np.testing.assert_array_equal(seen["obs_next"].numpy(), np.asarray(buf.obs_next)[idx])
        np.testing.assert_array_equal(seen["done"].numpy(), np.asarray(buf.done)[idx].astype(np.float32))
        np.testing.assert_array_equal(seen["rew"].numpy(), np.asarray(buf.rew)[idx].astype(np.float32))
        torch.manual_seed(5)                           # the reference's order and shapes
        want = [torch.randn(8, LAT), torch.randn(8 * R, LAT), torch.randn(8, LAT)]
        for g, w in zip(seen["draws"], want):
            assert torch.equal(g, w)
        algo.lmbda = 0.5
        algo.critic2_optim._optim.param_groups[0]["lr"] = 7e-4
        algo.update(buffer=buf, sample_size=8)
        algo.num_sampled_action = R + 1
        with pytest.raises(NotImplementedError, match="hip_invalidate"):
            algo.update(buffer=buf, sample_size=8)
        algo.num_sampled_action = R
    assert seen["lmbda"] == [0.75, 0.5] and seen["lr"] == [5e-4, 7e-4]
    after = [p_first, old_first, pert_old_first, v_first]
    for t, b, add in zip(after, before, (4.0, 3.0, 0.0, 2.0)):
        assert torch.allclose(t.detach(), b + add)
    st = algo.vae_optim._optim.state[v_first]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.25))
    assert float(algo.critic_optim._optim.state[next(iter(algo.policy.critic.parameters()))]["step"]) == 2.0
    sd = algo.state_dict()
    other = _make(num_sampled_action=R)
    other.load_state_dict(sd)
    for a, b in zip(algo.parameters(), other.parameters()):
        assert torch.equal(a, b)
    eng = other._engine()                               # a rebuilt engine continues from the loaded state
    assert eng.adam_step == 2
    for part in other._hip_parts():                     # (through the converters: the double also wrote the padding entries)
        for suffix in ("", "_m", "_v") + (("_old",) if part.old is not None else ()):
            for a, b in zip(part.to_torch(getattr(eng, part.name + suffix)), part.to_torch(getattr(algo._hip_engine, part.name + suffix))):
                assert torch.equal(a, b), part.name + suffix


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_cbcq_standins_have_the_reference_surface():
    from tianshou.algorithm.imitation.bcq import BCQ, BCQTrainingStats
    from tianshou_amd.integration import make_hip_bcq

    for net_kw in (dict(), dict(hidden=(64, 48, 40), vae_hidden=(96, 72), pert_net="net", activation=nn.Tanh, max_action=2.0, phi=0.3)):
        kw = dict(gamma=0.9, tau=0.01, lmbda=0.6, num_sampled_action=4)
        real, fake = BCQ(**_real_parts(**net_kw), **kw), SB.BCQ(**_fake_parts(**net_kw), **kw)
        pairs = ((real.policy.actor_perturbation, fake.policy.actor_perturbation), (real.policy.critic, fake.policy.critic),
                 (real.critic2, fake.critic2), (real.policy.vae, fake.policy.vae),
                 (real.actor_perturbation_target.module, fake.actor_perturbation_target.module),
                 (real.critic_target.module, fake.critic_target.module), (real.critic2_target.module, fake.critic2_target.module))
        for a, b in pairs:
            sa, sb = a.state_dict(), b.state_dict()
            assert list(sa.keys()) == list(sb.keys())
            assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
        for name in kw:
            assert getattr(real, name) == getattr(fake, name), name
        for name in ("phi", "max_action"):
            assert getattr(real.policy.actor_perturbation, name) == getattr(fake.policy.actor_perturbation, name)
        assert real.policy.vae.latent_dim == fake.policy.vae.latent_dim and real.policy.forward_sampled_times == fake.policy.forward_sampled_times
        for name in ("actor_perturbation_optim", "critic_optim", "critic2_optim", "vae_optim"):
            r, f = getattr(real, name), getattr(fake, name)
            assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm is None, name
            assert r._optim.param_groups[0]["lr"] == f._optim.param_groups[0]["lr"]
    s = dict(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0, vae_loss=4.0)
    assert BCQTrainingStats(**s).vae_loss == SB.BCQTrainingStats(**s).vae_loss == 4.0
    A_, B_ = make_hip_bcq(), make_hip_bcq(ref=SB)
    assert A_.__name__ == B_.__name__ == "HipBCQ" and issubclass(A_, BCQ) and issubclass(B_, SB.BCQ)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts", "_hip_noises", "_hip_cbcq_fields"):
        fa, fb = getattr(A_, name), getattr(B_, name)
        assert getattr(fa, "__wrapped__", fa).__code__.co_code == getattr(fb, "__wrapped__", fb).__code__.co_code, name


def test_ts_cbcq_entry_points_validate_before_any_hip_call():
    """R < 1, B R / B (R + 1) beyond int, latent_dim outside [1, 64], max_action <= 0, phi < 0, lmbda outside [0, 1], a non-finite
    hyper-parameter and a missing second critic fail as TS_ERR_INVALID_ARG on a workspace that has never touched a device (the
    dummy pointers are never dereferenced); so do NULL arguments and the trunk checks, and a NULL workspace as TS_ERR_WORKSPACE."""
    from tianshou_amd import _lib, cbcq, sac
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    d = C.c_void_p(4096)
    i64, f64 = C.c_int64, C.c_double

    def upd(ws=ws, B=5, R=2, L=6, obs=d, eps=d, stats=d, missing=(), hidden=64, depth=2, vhidden=96, vdepth=2, step=1, hp=True, **over):
        st = (C.c_void_p * len(cbcq.CBCQ_ST))(*[None if n in missing else 4096 for n in cbcq.CBCQ_ST])
        t, tv = sac.MLPTrunk(hidden, depth, "relu", 0.0), sac.MLPTrunk(vhidden, vdepth, "relu", 0.0)
        return lib.ts_cbcq_update(ws, st, i64(step), obs, d, d, d, d, d, eps, d, i64(B), i64(R), i64(7), i64(3), i64(L), C.byref(t),
                                  C.byref(tv), cbcq.CBCQConfig(**over).to_c() if hp else None, stats, None, None, None)

    def fwd(ws=ws, N=2, T=5, L=6, obs=d, out=d, phi=0.05, max_action=1.0, hidden=64):
        t, tv = sac.MLPTrunk(hidden, 2, "relu", 0.0), sac.MLPTrunk(96, 2, "relu", 0.0)
        return lib.ts_cbcq_policy_forward(ws, d, d, d, obs, d, i64(N), i64(T), i64(7), i64(3), i64(L), C.byref(t), C.byref(tv), f64(phi),
                                          f64(max_action), C.c_int32(0), out, None, None, None, None)

    inf, nan = float("inf"), float("nan")
    try:
        assert upd(ws=None) == _lib.TS_ERR_WORKSPACE and b"ts_cbcq_update" in lib.ts_last_error()
        for kw in (dict(R=0), dict(R=-1), dict(B=0), dict(B=2**31 // 3 + 1, R=2), dict(B=2**31 // 2 + 1, R=1), dict(B=5, R=2**31),
                   dict(L=0), dict(L=65), dict(max_action=0.0), dict(max_action=-1.0), dict(phi=-0.1), dict(lmbda=-0.01),
                   dict(lmbda=1.01), dict(gamma=nan), dict(tau=inf), dict(vae_lr=nan), dict(critic2_max_grad_norm=-inf),
                   dict(phi=nan), dict(max_action=inf), dict(missing=("critic2",)), dict(missing=("critic2_old",)),
                   dict(missing=("critic2_m", "critic2_v"))):
            assert upd(**kw) == _lib.TS_ERR_INVALID_ARG, kw
            assert b"ts_cbcq_update" in lib.ts_last_error(), kw
        assert b"both critics" in lib.ts_last_error()
        for kw in (dict(obs=None), dict(eps=None), dict(stats=None), dict(step=0), dict(hp=False), dict(missing=("pert",)),
                   dict(missing=("vae_v",)), dict(missing=("pert_old",)), dict(hidden=100), dict(depth=7), dict(vhidden=100),
                   dict(vdepth=0 - 1)):
            assert upd(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        assert fwd(ws=None) == _lib.TS_ERR_WORKSPACE
        for kw in (dict(N=0), dict(T=0), dict(N=2**31 // 4, T=5), dict(L=0), dict(L=65), dict(obs=None), dict(out=None), dict(phi=-1.0),
                   dict(max_action=0.0), dict(hidden=100)):
            assert fwd(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        assert lib.ts_cbcq_latent(ws, d, d, d, d, i64(4), i64(65), d, d, d, d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_latent(ws, d, d, d, None, i64(4), i64(6), d, d, d, d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_recon(ws, d, d, i64(4), i64(33), f64(1.0), d, d, d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_recon(ws, d, d, i64(4), i64(3), f64(0.0), d, d, d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_target(ws, d, d, d, d, i64(4), i64(0), f64(0.99), f64(0.75), d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_target(ws, d, d, d, d, i64(4), i64(2), f64(0.99), f64(1.5), d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_perturb(ws, d, d, d, i64(4), i64(3), f64(-0.1), f64(1.0), d, d, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_cbcq_perturb(ws, d, d, None, i64(4), i64(3), f64(0.1), f64(1.0), d, d, None) == _lib.TS_ERR_INVALID_ARG
        for fn, args in ((lib.ts_cbcq_latent, (d, d, d, d, i64(4), i64(6), d, d, d, d, None)),
                         (lib.ts_cbcq_recon, (d, d, i64(4), i64(3), f64(1.0), d, d, d, None)),
                         (lib.ts_cbcq_target, (d, d, d, d, i64(4), i64(2), f64(0.99), f64(0.75), d, None)),
                         (lib.ts_cbcq_perturb, (d, d, d, i64(4), i64(3), f64(0.1), f64(1.0), d, d, None))):
            assert fn(None, *args) == _lib.TS_ERR_WORKSPACE
    finally:
        lib.ts_workspace_destroy(ws)
