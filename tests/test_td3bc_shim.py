"""CPU: the HipTD3BC drop-in (tianshou_amd.integration.make_hip_td3bc) without an engine -- over the real reference classes where
the reference is mounted, over tests/standin_td3bc.py otherwise: the class it builds, the way `alpha` travels, what the shared
factory leaves of HipTD3 / HipDDPG, and ts_td3bc_update's argument checks, which run before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_td3bc as SB

REAL = ref_shim.reference_available()
OBS, ACT = 11, 3


def _real_parts(hidden=(256, 256), max_action=1.0):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.ddpg import ContinuousDeterministicPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousCritic

    actor = ContinuousActorDeterministic(preprocess_net=Net(state_shape=(OBS,), hidden_sizes=list(hidden)), action_shape=(ACT,),
                                         max_action=max_action)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(OBS,), action_shape=(ACT,), hidden_sizes=list(hidden),  # noqa: E731
                                                     concat=True))
    policy = ContinuousDeterministicPolicy(actor=actor, action_space=gym.spaces.Box(low=-max_action, high=max_action, shape=(ACT,)),
                                           exploration_noise=None)
    return dict(policy=policy, policy_optim=AdamOptimizerFactory(lr=3e-4), critic=mk(), critic_optim=AdamOptimizerFactory(lr=1e-3)), mk


def _make(twin_given=True, **kw):
    """HipTD3BC on Net[256, 256] networks (real classes or stand-ins)."""
    from tianshou_amd.integration import make_hip_td3bc

    if REAL:
        parts, mk = _real_parts()
        from tianshou.algorithm.optim import AdamOptimizerFactory

        if twin_given:
            parts.update(critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3))
        return make_hip_td3bc()(device="cpu", **parts, **kw)
    actor = SB.ContinuousActorDeterministic(SB.Net(OBS, [256, 256], nn.ReLU), ACT, max_action=1.0)
    mk = lambda: SB.ContinuousCritic(SB.Net(OBS + ACT, [256, 256], nn.ReLU))          # noqa: E731
    return make_hip_td3bc(ref=SB)(policy=SB.Policy(actor), critic=mk(), critic2=mk() if twin_given else None, lr=3e-4,
                                  critic_lr=1e-3, device="cpu", **kw)


def test_class_and_alpha_are_carried():
    algo = _make(alpha=1.25, update_actor_freq=3)
    assert type(algo).__name__ == "HipTD3BC" and algo.alpha == 1.25 and algo.update_actor_freq == 3
    assert (algo._cnt, algo._last) == (0, 0)
    assert _make().alpha == 2.5                                         # the reference's default
    if REAL:
        from tianshou.algorithm.algorithm_base import OfflineAlgorithm
        from tianshou.algorithm.imitation.td3_bc import TD3BC
        from tianshou.algorithm.modelfree.td3 import TD3

        mro = type(algo).__mro__
        assert isinstance(algo, TD3BC) and mro.index(TD3BC) < mro.index(OfflineAlgorithm) < mro.index(TD3)


def test_a_missing_second_critic_is_copied_as_the_reference_does():
    algo = _make(twin_given=False)
    assert algo.critic2 is not algo.critic and algo.critic2_optim is not algo.critic_optim
    for a, b in zip(algo.critic.parameters(), algo.critic2.parameters()):
        assert a is not b and torch.equal(a, b)
    assert len(algo._hip_parts()) == 3


def test_engine_config_is_always_twin():
    from tianshou_amd import td3, td3bc

    cfg = td3bc.TD3BCConfig()
    assert cfg.twin and cfg.alpha == 2.5 and isinstance(cfg, td3.TD3Config) and issubclass(td3bc.TD3BCEngine, td3.TD3Engine)
    assert cfg.update_actor_freq == 2 and td3bc.TD3BCConfig(alpha=0.0).alpha == 0.0
    with pytest.raises(ValueError, match="twin"):
        td3bc.TD3BCConfig(twin=False)
    own = [n for n in vars(td3bc.TD3BCEngine) if not n.startswith("__")]
    assert own == ["update_with_batch"], own                            # everything else is TD3Engine's, untouched


def test_the_td3_and_ddpg_drop_ins_are_unchanged_by_the_shared_factory():
    from tianshou_amd.integration import make_hip_ddpg, make_hip_td3, make_hip_td3bc

    T3, DD, BC = make_hip_td3(ref=SB), make_hip_ddpg(ref=SB), make_hip_td3bc(ref=SB)
    assert (T3.__name__, DD.__name__, BC.__name__) == ("HipTD3", "HipDDPG", "HipTD3BC")
    assert SB.TD3BC in BC.__mro__ and SB.TD3BC not in T3.__mro__ and SB.TD3BC not in DD.__mro__
    assert SB.TD3 in T3.__mro__ and SB.DDPG in DD.__mro__
    actor = SB.ContinuousActorDeterministic(SB.Net(OBS, [64, 64], nn.ReLU), ACT)
    mk = lambda: SB.ContinuousCritic(SB.Net(OBS + ACT, [64, 64], nn.ReLU))             # noqa: E731
    assert not hasattr(T3(policy=SB.Policy(actor), critic=mk(), critic2=mk(), device="cpu"), "alpha")
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts"):   # one body for the three classes
        assert getattr(T3, name).__code__.co_code == getattr(BC, name).__code__.co_code, name


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_td3bc_standin_has_the_reference_surface():
    """tests/standin_td3bc.py against the real TD3BC: state_dict keys and shapes of the networks and their lagged copies, the
    attributes the hooks read, the optimizers; the hook bodies are the same code over either namespace."""
    from tianshou.algorithm.imitation.td3_bc import TD3BC
    from tianshou.algorithm.modelfree.td3 import TD3TrainingStats
    from tianshou.algorithm.optim import AdamOptimizerFactory

    parts, mk = _real_parts((128, 128), 1.5)
    real = TD3BC(critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3), tau=0.01, gamma=0.98, policy_noise=0.2,
                 update_actor_freq=2, noise_clip=0.5, alpha=1.25, n_step_return_horizon=3, **parts)
    f_actor = SB.ContinuousActorDeterministic(SB.Net(OBS, [128, 128], nn.ReLU), ACT, max_action=1.5)
    fake = SB.TD3BC(policy=SB.Policy(f_actor), critic=SB.ContinuousCritic(SB.Net(OBS + ACT, [128, 128], nn.ReLU)),
                    critic2=SB.ContinuousCritic(SB.Net(OBS + ACT, [128, 128], nn.ReLU)), lr=3e-4, critic_lr=1e-3, tau=0.01, gamma=0.98,
                    policy_noise=0.2, update_actor_freq=2, noise_clip=0.5, alpha=1.25, n_step_return_horizon=3)
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.critic2, fake.critic2),
             (real.actor_old.module, fake.actor_old.module), (real.critic_old.module, fake.critic_old.module),
             (real.critic2_old.module, fake.critic2_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("tau", "gamma", "n_step_return_horizon", "policy_noise", "update_actor_freq", "noise_clip", "alpha", "_cnt", "_last"):
        assert getattr(real, name) == getattr(fake, name), name
    assert float(real.policy.actor.max_action) == float(fake.policy.actor.max_action)
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert r._optim.param_groups[0]["lr"] == f._optim.param_groups[0]["lr"]
    assert TD3TrainingStats(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0).critic2_loss == \
        SB.TD3TrainingStats(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0).critic2_loss
    from tianshou_amd.integration import make_hip_td3bc

    A_, B_ = make_hip_td3bc(), make_hip_td3bc(ref=SB)
    assert A_.__name__ == B_.__name__ == "HipTD3BC" and issubclass(A_, TD3BC) and issubclass(B_, SB.TD3BC)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts"):
        assert getattr(A_, name).__code__.co_code == getattr(B_, name).__code__.co_code, name


@pytest.mark.skipif(not REAL, reason="reference not mounted")
@pytest.mark.parametrize("prioritized", [False, True])
def test_hip_td3bc_wrapper_runs_with_engine_double(prioritized, monkeypatch):
    """Two update() calls of HipTD3BC over a CPU double of TD3BCEngine (the pattern of tests/test_integration_shim.py), on a plain
    and on a prioritized buffer: the config with `alpha`, `alpha` re-read at every update, `_cnt` / `_last`, the statistics'
    type, and the write-back of parameters, lagged networks and Adam state."""
    from tianshou.algorithm.modelfree.td3 import TD3TrainingStats
    from tianshou.data import PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.td3bc as TB
    from tests.test_integration_shim import _fill, _patch_for_cpu, _zeros_like_all

    seen = {"alpha": [], "weight": []}

    class FakeTD3BC:
        def __init__(self, obs_dim, act_dim, actor, c1, c2, cfg, hidden=256, depth=2, activation="relu"):
            assert isinstance(cfg, TB.TD3BCConfig) and cfg.twin and cfg.alpha == 1.25 and c2 is not None
            assert (obs_dim, act_dim, hidden, depth, cfg.update_actor_freq, cfg.actor_lr, cfg.critic_lr) == (OBS, ACT, 256, 2, 2, 3e-4, 1e-3)
            self.hidden, self.obs_dim, self.act_dim, self.cfg, self.cnt, self.actor_steps = hidden, obs_dim, act_dim, cfg, 0, 0
            self.actor, self.critic1, self.critic2 = actor.clone(), c1.clone(), c2.clone()
            for n in ("actor", "critic1", "critic2"):
                setattr(self, n + "_old", getattr(self, n).clone())
            _zeros_like_all(self, ("actor", "critic1", "critic2"))

        def preprocess(self, m, idx, noise):
            assert noise is not None and tuple(noise.shape) == (idx.numel(), ACT)
            return torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret, weight=None):
            assert obs.shape == (8, OBS) and act.shape == (8, ACT)
            seen["alpha"].append(self.cfg.alpha)
            seen["weight"].append(weight is not None)
            self.cnt += 1
            self.actor_steps += 1
            self.actor += 2.0
            self.critic2 += 3.0
            self.actor_old += 1.5
            self.actor_m += 0.125
            return torch.tensor([0.1 * self.cnt, 0.2, 0.3, 7.0]), torch.ones(8)

    algo = _make(alpha=1.25)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(TB, "TD3BCEngine", FakeTD3BC)
    buf = PrioritizedVectorReplayBuffer(32, 2, alpha=0.6, beta=0.4) if prioritized else VectorReplayBuffer(32, 2)
    _fill(buf, 12, (OBS,), np.zeros((2, ACT), np.float32))
    a_first = next(iter(algo.policy.actor.parameters()))
    c2_first = next(iter(algo.critic2.parameters()))
    old_first = next(iter(algo.actor_old.module.parameters()))
    before, c2_before, old_before = (t.detach().clone() for t in (a_first, c2_first, old_first))
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
        assert isinstance(stats, TD3TrainingStats)
        assert abs(stats.actor_loss - 0.1) < 1e-6 and abs(stats.critic1_loss - 0.2) < 1e-6 and abs(stats.critic2_loss - 0.3) < 1e-6
        assert algo._cnt == 1 and abs(algo._last - 0.1) < 1e-6
        algo.alpha = 0.5
        stats = algo.update(buffer=buf, sample_size=8)
    assert seen["alpha"] == [1.25, 0.5] and seen["weight"] == [prioritized] * 2
    assert algo._cnt == 2 and abs(algo._last - 0.2) < 1e-6 and abs(stats.actor_loss - 0.2) < 1e-6
    assert torch.allclose(a_first.detach(), before + 4.0) and torch.allclose(c2_first.detach(), c2_before + 6.0)
    assert torch.allclose(old_first.detach(), old_before + 3.0)
    st = algo.policy_optim._optim.state[a_first]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.25))
    assert float(algo.critic2_optim._optim.state[c2_first]["step"]) == 2.0


def test_ts_td3bc_update_validates_before_any_hip_call():
    """Everything ts_td3_update refuses, plus a negative / non-finite bc_alpha and a missing second critic, fails as
    TS_ERR_INVALID_ARG with a message naming ts_td3bc_update on a workspace that has never touched a device (ts_workspace_create
    only allocates host memory; the dummy pointers are never dereferenced), and a NULL workspace as TS_ERR_WORKSPACE."""
    from tianshou_amd import _lib, sac, td3
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    d = 4096
    hp = td3.TD3HParams(-1.0, -1.0, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0)
    names = [n for n, _ in td3.TD3StateC._fields_]

    def call(ws=ws, missing=(), obs=C.c_void_p(d), act=C.c_void_p(d), ret=C.c_void_p(d), stats=C.c_void_p(d), hp_=C.byref(hp),
             B=5, alpha=2.5, critic_step=1, actor_step=1, hidden=64, depth=2, state=True):
        st = td3.TD3StateC(*[None if n in missing else d for n in names])
        trunk = sac.MLPTrunk(hidden, depth, "relu", 0.0)
        return lib.ts_td3bc_update(ws, C.byref(st) if state else None, C.c_int64(critic_step), C.c_int64(actor_step), obs, act, ret,
                                   None, C.c_int64(B), C.c_int64(7), C.c_int64(3), C.byref(trunk), hp_, C.c_double(alpha), stats,
                                   None, None, None)

    try:
        assert call(ws=None) == _lib.TS_ERR_WORKSPACE and b"ts_td3bc_update" in lib.ts_last_error()
        for kw in (dict(obs=None), dict(act=None), dict(ret=None), dict(stats=None), dict(hp_=None), dict(state=False), dict(B=0),
                   dict(B=-3), dict(critic_step=0), dict(actor_step=0), dict(missing=("actor",)), dict(missing=("critic1_m",)),
                   dict(missing=("actor_old",)), dict(missing=("critic2_v",)), dict(missing=("critic2_old",))):
            assert call(**kw) == _lib.TS_ERR_INVALID_ARG, kw
            assert b"ts_td3bc_update" in lib.ts_last_error(), kw
        for kw in (dict(hidden=100), dict(depth=7)):                              # the trunk, as every SAC-family entry point
            assert call(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
            assert call(alpha=bad) == _lib.TS_ERR_INVALID_ARG, bad
            assert b"ts_td3bc_update" in lib.ts_last_error() and b"bc_alpha" in lib.ts_last_error()
        for missing in (("critic2",), ("critic2", "critic2_m", "critic2_v", "critic2_old")):      # TD3+BC is always twin
            assert call(missing=missing) == _lib.TS_ERR_INVALID_ARG, missing
            assert b"ts_td3bc_update" in lib.ts_last_error() and b"critic" in lib.ts_last_error()
        # the same state is DDPG for ts_td3_update: its checks and messages are as before
        st = td3.TD3StateC(*[None if n == "critic2_v" else d for n in names])
        trunk = sac.MLPTrunk(64, 2, "relu", 0.0)
        rc = lib.ts_td3_update(ws, C.byref(st), C.c_int64(1), C.c_int64(1), C.c_void_p(d), C.c_void_p(d), C.c_void_p(d), None,
                               C.c_int64(5), C.c_int64(7), C.c_int64(3), C.byref(trunk), C.byref(hp), C.c_void_p(d), None, None, None)
        assert rc == _lib.TS_ERR_INVALID_ARG and lib.ts_last_error() == b"ts_td3_update: incomplete second critic"
    finally:
        lib.ts_workspace_destroy(ws)
