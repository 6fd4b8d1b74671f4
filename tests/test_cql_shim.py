"""CPU: the HipCQL drop-in (tianshou_amd.integration.make_hip_cql) without an engine -- over the real reference classes where
the reference is mounted, over tests/standin_cql.py otherwise: the class it builds, the config it hands the engine, the rows and
random tensors of an update, the write-back of the Lagrange multiplier, and the argument checks of ts_cql_update / ts_cql_loss,
which run before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_cql as SC

REAL = ref_shim.reference_available()
OBS, ACT = 11, 3


def _real_parts(hidden=(256, 256)):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.sac import SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(OBS,), hidden_sizes=list(hidden)), action_shape=(ACT,),
                                         unbounded=True, conditioned_sigma=True)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(OBS,), action_shape=(ACT,), hidden_sizes=list(hidden),  # noqa: E731
                                                     concat=True))
    policy = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(ACT,)))
    return dict(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-4), critic=mk(), critic_optim=AdamOptimizerFactory(lr=3e-4),
                critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=3e-4))


def _fake(hidden=(256, 256), **kw):
    actor = SC.ContinuousActorProbabilistic(SC.Net(OBS, list(hidden), nn.ReLU), ACT, unbounded=True, conditioned_sigma=True)
    mk = lambda: SC.ContinuousCritic(SC.Net(OBS + ACT, list(hidden), nn.ReLU))          # noqa: E731
    return dict(policy=SC.Policy(actor), critic=mk(), critic2=mk(), lr=1e-4, critic_lr=3e-4, **kw)


def _make(**kw):
    from tianshou_amd.integration import make_hip_cql

    if REAL:
        parts = _real_parts()                           # (installs the shim that makes the reference importable)
        return make_hip_cql()(device="cpu", update_noise="torch", **parts, **kw)
    return make_hip_cql(ref=SC)(device="cpu", update_noise="torch", **_fake(**kw))


def test_class_and_hyper_parameters_are_carried():
    algo = _make(cql_weight=5.0, temperature=0.7, num_repeat_actions=3, with_lagrange=False, calibrated=False, min_action=1.0,
                 max_grad_norm=0.5)
    assert type(algo).__name__ == "HipCQL" and len(algo._hip_parts()) == 3
    f = algo._hip_cql_fields()
    assert (f["cql_weight"], f["temperature"], f["num_repeat_actions"], f["with_lagrange"], f["calibrated"], f["min_action"],
            f["max_grad_norm"], f["cql_alpha_lr"]) == (5.0, 0.7, 3, False, False, 1.0, 0.5, 1e-4)
    assert algo._hip_cql_leaf() is algo.cql_alpha_optim.param_groups[0]["params"][0]
    from tianshou_amd.integration import make_hip_cql

    with pytest.raises(ValueError):
        make_hip_cql(ref=SC)(device="cpu", update_noise="numpy", **_fake())


def test_engine_classes():
    from tianshou_amd import cql, sac

    cfg = cql.CQLConfig()
    assert isinstance(cfg, sac.SACConfig) and issubclass(cql.CQLEngine, sac.SACEngine)
    assert (cfg.cql_alpha_lr, cfg.cql_weight, cfg.temperature, cfg.with_lagrange, cfg.lagrange_threshold, cfg.min_action, cfg.max_action,
            cfg.num_repeat_actions, cfg.alpha_min, cfg.alpha_max, cfg.max_grad_norm, cfg.calibrated) == \
        (1e-4, 1.0, 1.0, True, 10.0, -1.0, 1.0, 10, 0.0, 1e6, 1.0, True)                       # cql.py:44-58
    assert list(cfg.cql_hp()) == [0.99, 1.0, 1.0, 1.0, 10.0, 0.0, 1e6, 1e-4, 1.0]
    own = [n for n in vars(cql.CQLEngine) if not n.startswith("__")]
    assert own == ["update_with_batch"], own


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_cql_standin_has_the_reference_surface():
    from tianshou.algorithm.imitation.cql import CQL, CQLTrainingStats
    from tianshou_amd.integration import make_hip_cql

    kw = dict(cql_alpha_lr=3e-4, cql_weight=2.0, tau=0.01, gamma=0.98, alpha=0.2, temperature=0.7, with_lagrange=True,
              lagrange_threshold=5.0, min_action=1.0, max_action=1.0, num_repeat_actions=4, alpha_min=0.1, alpha_max=100.0,
              max_grad_norm=0.5, calibrated=False)
    real, fake = CQL(**_real_parts((128, 128)), **kw), SC.CQL(**_fake((128, 128), **kw))
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.critic2, fake.critic2),
             (real.critic_old.module, fake.critic_old.module), (real.critic2_old.module, fake.critic2_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in kw:
        if name not in ("cql_alpha_lr", "alpha", "max_grad_norm"):
            assert getattr(real, name) == getattr(fake, name), name
    assert not hasattr(real, "n_step_return_horizon") and not hasattr(fake, "n_step_return_horizon")
    assert real.alpha.value == fake.alpha.value == 0.2
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm, name
        assert r._optim.param_groups[0]["lr"] == f._optim.param_groups[0]["lr"]
    assert real.policy_optim._max_grad_norm is None and real.critic_optim._max_grad_norm == 0.5
    for a in (real, fake):
        g = a.cql_alpha_optim.param_groups[0]
        assert type(a.cql_alpha_optim) is torch.optim.Adam and g["lr"] == 3e-4 and g["params"][0] is a.cql_log_alpha
        assert tuple(a.cql_log_alpha.shape) == (1,) and float(a.cql_log_alpha.detach()) == 0.0
    s = dict(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0, alpha=0.2, alpha_loss=None, cql_alpha=1.0, cql_alpha_loss=-2.0)
    assert CQLTrainingStats(**s).cql_alpha_loss == SC.CQLTrainingStats(**s).cql_alpha_loss == -2.0
    A_, B_ = make_hip_cql(), make_hip_cql(ref=SC)
    assert A_.__name__ == B_.__name__ == "HipCQL" and issubclass(A_, CQL) and issubclass(B_, SC.CQL)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts", "_hip_noises", "_hip_write_back"):
        fa, fb = getattr(A_, name), getattr(B_, name)
        assert getattr(fa, "__wrapped__", fa).__code__.co_code == getattr(fb, "__wrapped__", fb).__code__.co_code, name


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_hip_cql_wrapper_runs_with_engine_double(monkeypatch):
    """Two update() calls of HipCQL over a CPU double of CQLEngine on a buffer with calibration_returns: the config, the
    hyper-parameters re-read at every update, the rows (obs, act, rew, done, obs_next, calibration returns) gathered by index,
    the five random tensors in the reference's draw order from torch's generator (all-ones random actions with the default
    bounds), the statistics' type, the write-back of parameters, lagged networks, Adam state, cql_log_alpha and its optimizer
    state, and the state_dict() / load_state_dict() round trip of the multiplier."""
    from tianshou.algorithm.imitation.cql import CQLTrainingStats
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.cql as Q
    from tests.test_integration_shim import _patch_for_cpu, _zeros_like_all

    seen = {"weight": [], "idx": []}
    R = 3

    class FakeCQL:
        def __init__(self, obs_dim, act_dim, actor, c1, c2, cfg, hidden=256, depth=2, max_action=0.0, activation="relu"):
            assert isinstance(cfg, Q.CQLConfig) and cfg.num_repeat_actions == R and cfg.calibrated and cfg.with_lagrange
            assert (obs_dim, act_dim, hidden, depth, max_action, cfg.actor_lr, cfg.critic_lr, cfg.max_grad_norm, cfg.cql_alpha_lr) == \
                (OBS, ACT, 256, 2, 0.0, 1e-4, 3e-4, 1.0, 1e-4)
            assert cfg.auto_alpha is False and cfg.alpha == 0.2 and not hasattr(cfg, "n_step") or cfg.n_step == 1
            self.hidden, self.obs_dim, self.act_dim, self.cfg, self.adam_step = hidden, obs_dim, act_dim, cfg, 0
            self.actor, self.critic1, self.critic2 = actor.clone(), c1.clone(), c2.clone()
            self.critic1_old, self.critic2_old = c1.clone(), c2.clone()
            _zeros_like_all(self, ("actor", "critic1", "critic2"))
            self.log_alpha, self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)
            self.cql_log_alpha, self.cql_log_alpha_m, self.cql_log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)

        def update_with_batch(self, obs, act, rew, done, obs_next, n1, n2, ra, n4, n5, calib=None):
            assert obs.shape == obs_next.shape == (8, OBS) and act.shape == (8, ACT) and rew.shape == done.shape == calib.shape == (8,)
            assert rew.dtype == done.dtype == calib.dtype == torch.float32
            assert n1.shape == n2.shape == (8, ACT) and ra.shape == n4.shape == n5.shape == (8 * R, ACT)
            seen["weight"].append(self.cfg.cql_weight)
            seen.update(obs=obs.clone(), rew=rew.clone(), done=done.clone(), calib=calib.clone(), draws=[t.clone() for t in (n1, n2, ra, n4, n5)])
            self.adam_step += 1
            self.actor += 2.0
            self.critic2_old += 1.5
            self.actor_m += 0.125
            self.cql_log_alpha += 0.25
            self.cql_log_alpha_m += 0.5
            return torch.tensor([0.1, 0.2, 0.3, 0.2, 0.0, 1.5, -2.5])

    algo = _make(num_repeat_actions=R)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(Q, "CQLEngine", FakeCQL)
    buf = VectorReplayBuffer(32, 2)
    rng = np.random.default_rng(0)
    for t in range(16):
        buf.add(Batch(obs=rng.normal(size=(2, OBS)).astype(np.float32), act=np.zeros((2, ACT), np.float32), rew=rng.normal(size=2),
                      terminated=np.array([t % 5 == 4, False]), truncated=np.array([False, t % 7 == 6]),
                      obs_next=np.zeros((2, OBS), np.float32)))
    buf = algo.process_buffer(buf)                     # the reference's: calibration_returns, once
    a_first = next(iter(algo.policy.actor.parameters()))
    old_first = next(iter(algo.critic2_old.module.parameters()))
    before, old_before = a_first.detach().clone(), old_first.detach().clone()
    with policy_within_training_step(algo.policy):
        torch.manual_seed(5)
        stats = algo.update(buffer=buf, sample_size=8)
        idx = algo._hip_idx.numpy()
        assert isinstance(stats, CQLTrainingStats)
        assert abs(stats.actor_loss - 0.1) < 1e-6 and abs(stats.critic2_loss - 0.3) < 1e-6 and stats.alpha_loss is None
        assert abs(stats.cql_alpha - 1.5) < 1e-6 and abs(stats.cql_alpha_loss + 2.5) < 1e-6
        np.testing.assert_array_equal(seen["obs"].numpy(), np.asarray(buf.obs)[idx])
        np.testing.assert_array_equal(seen["done"].numpy(), np.asarray(buf.done)[idx].astype(np.float32))
        np.testing.assert_array_equal(seen["rew"].numpy(), np.asarray(buf.rew)[idx].astype(np.float32))
        np.testing.assert_array_equal(seen["calib"].numpy(), np.asarray(buf._meta.calibration_returns)[idx].astype(np.float32))
        torch.manual_seed(5)                           # the reference's order and calls
        want = [torch.randn(8, ACT), torch.randn(8, ACT), torch.FloatTensor(8 * R, ACT).uniform_(1.0, 1.0), torch.randn(8 * R, ACT),
                torch.randn(8 * R, ACT)]
        for g, w in zip(seen["draws"], want):
            assert torch.equal(g, w)
        assert torch.all(seen["draws"][2] == 1.0)
        algo.cql_weight = 0.5
        algo.update(buffer=buf, sample_size=8)
    assert seen["weight"] == [1.0, 0.5]
    assert torch.allclose(a_first.detach(), before + 4.0) and torch.allclose(old_first.detach(), old_before + 3.0)
    st = algo.policy_optim._optim.state[a_first]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.25))
    leaf = algo._hip_cql_leaf()
    assert float(leaf.detach()) == 0.5 and float(algo.cql_log_alpha.detach()) == 0.5
    cs = algo.cql_alpha_optim.state[leaf]
    assert float(cs["step"]) == 2.0 and float(cs["exp_avg"]) == 1.0
    sd = algo.state_dict()
    other = _make(num_repeat_actions=R)
    other.load_state_dict(sd)
    assert float(other._hip_cql_leaf().detach()) == 0.5 and float(other.cql_alpha_optim.state[other._hip_cql_leaf()]["exp_avg"]) == 1.0
    eng = other._engine()                               # a rebuilt engine continues from the loaded multiplier
    assert float(eng.cql_log_alpha) == 0.5 and float(eng.cql_log_alpha_m) == 1.0 and eng.adam_step == 2


def test_ts_cql_entry_points_validate_before_any_hip_call():
    """R < 1, B (1 + 3R) beyond int, temperature <= 0, alpha_min > alpha_max and a non-finite hyper-parameter fail as
    TS_ERR_INVALID_ARG naming the entry point on a workspace that has never touched a device (the dummy pointers are never
    dereferenced); so do NULL arguments, the trunk checks of every SAC-family entry point, and a NULL workspace as
    TS_ERR_WORKSPACE."""
    from tianshou_amd import _lib, cql, sac
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    d = C.c_void_p(4096)
    hp = sac.SACHParams(-1.0, -1.0, -1.0, 0.9, 0.999, 1e-8, 0.0, 0.2, 0.0, 0, 0)
    names = [n for n, _ in sac.SACStateC._fields_]

    def upd(ws=ws, B=5, R=2, obs=d, noise=d, stats=d, cql3=d, missing=(), hidden=64, depth=2, step=1, **over):
        st = sac.SACStateC(*[None if n in missing else 4096 for n in names])
        trunk = sac.MLPTrunk(hidden, depth, "relu", 0.0)
        return lib.ts_cql_update(ws, C.byref(st), cql3, C.c_int64(step), obs, d, d, d, d, None, d, d, d, noise, d, C.c_int64(B), C.c_int64(R),
                                 C.c_int64(7), C.c_int64(3), C.byref(trunk), C.byref(hp), cql.CQLConfig(**over).cql_hp(), stats, None, None,
                                 None)

    def loss(ws=ws, B=5, R=2, q=d, out=d, A=3, **over):
        return lib.ts_cql_loss(ws, q, d, d, d, d, d, d, None, d, C.c_int64(B), C.c_int64(R), C.c_int64(A), cql.CQLConfig(**over).cql_hp(),
                               out, d, d, None)

    try:
        for fn, name in ((upd, b"ts_cql_update"), (loss, b"ts_cql_loss")):
            assert fn(ws=None) == _lib.TS_ERR_WORKSPACE and name in lib.ts_last_error()
            for kw in (dict(R=0), dict(R=-1), dict(B=0), dict(B=2**31 // 7 + 1, R=2), dict(B=5, R=2**31), dict(temperature=0.0),
                       dict(temperature=-1.0), dict(alpha_min=2.0, alpha_max=1.0), dict(cql_weight=float("nan")),
                       dict(lagrange_threshold=float("inf")), dict(gamma=float("nan")), dict(max_grad_norm=-float("inf"))):
                assert fn(**kw) == _lib.TS_ERR_INVALID_ARG, (name, kw)
                assert name in lib.ts_last_error(), (name, kw)
        for kw in (dict(obs=None), dict(noise=None), dict(stats=None), dict(cql3=None), dict(step=0), dict(missing=("actor",)),
                   dict(missing=("critic2_old",)), dict(missing=("critic1_v",)), dict(hidden=100), dict(depth=7)):
            assert upd(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        assert upd(cql3=None, with_lagrange=False, B=0) == _lib.TS_ERR_INVALID_ARG
        for kw in (dict(q=None), dict(out=None), dict(A=0), dict(A=33)):
            assert loss(**kw) == _lib.TS_ERR_INVALID_ARG, kw
    finally:
        lib.ts_workspace_destroy(ws)
