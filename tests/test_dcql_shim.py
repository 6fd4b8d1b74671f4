"""CPU: the HipDiscreteCQL drop-in (tianshou_amd.integration.make_hip_discrete_cql) without an engine -- over the real reference
classes where the reference is mounted, over tests/standin_dcql.py otherwise: the model check, the optimizer check and the way
`min_q_weight` travels."""
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_dcql as SC

REAL = ref_shim.reference_available()
C_, H_, W_, A_, N_ = 2, 44, 36, 3, 21


def _make(model, optim="adam", **kw):
    """HipDiscreteCQL over `model` (real classes or stand-ins); optim: "adam" or "rmsprop"."""
    from tianshou_amd.integration import make_hip_discrete_cql

    kw.setdefault("num_quantiles", N_)
    if REAL:
        ref_shim.install()
        import gymnasium as gym
        from tianshou.algorithm.modelfree.qrdqn import QRDQNPolicy
        from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory

        factory = AdamOptimizerFactory(lr=1e-4) if optim == "adam" else RMSpropOptimizerFactory(lr=1e-4)
        policy = QRDQNPolicy(model=model, action_space=gym.spaces.Discrete(A_))
        return make_hip_discrete_cql()(policy=policy, optim=factory, device="cpu", **kw)
    extra = {} if optim == "adam" else {"optim": (torch.optim.RMSprop, {})}
    return make_hip_discrete_cql(ref=SC)(policy=SC.DiscreteQLearningPolicy(model), lr=1e-4, device="cpu", **extra, **kw)


def _qrdqnet():
    if REAL:
        ref_shim.install()
        from tianshou.env.atari.atari_network import QRDQNet

        return QRDQNet(c=C_, h=H_, w=W_, action_shape=[A_], num_quantiles=N_)
    return SC.QRDQNet(C_, H_, W_, A_, N_)


def test_qrdqnet_is_accepted_and_min_q_weight_is_carried():
    algo = _make(_qrdqnet(), min_q_weight=2.5, target_update_freq=2)
    assert type(algo).__name__ == "HipDiscreteCQL" and algo.model_old is not None
    assert algo.min_q_weight == 2.5 and algo._n_atoms() == N_
    assert _make(_qrdqnet()).min_q_weight == 10.0                       # the reference's default
    if REAL:
        from tianshou.algorithm.imitation.discrete_cql import DiscreteCQL

        assert isinstance(algo, DiscreteCQL)


def test_model_with_other_keys_is_rejected():
    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(nn.Flatten(), nn.Linear(C_ * H_ * W_, 64), nn.ReLU(), nn.Linear(64, A_ * N_))

    with pytest.raises(NotImplementedError, match="HipDiscreteCQL: the model must be QRDQNet"):
        _make(Other())


def test_non_adam_optimizer_is_rejected():
    with pytest.raises(NotImplementedError, match="Adam"):
        _make(_qrdqnet(), optim="rmsprop")


def test_engine_config_pins_the_quantile_kind():
    from tianshou_amd import dcql

    cfg = dcql.DiscreteCQLConfig(n_atoms=N_)
    assert cfg.kind == "qr" and cfg.min_q_weight == 10.0 and cfg.to_c().lr == cfg.lr
    with pytest.raises(ValueError):
        dcql.DiscreteCQLConfig(kind="c51")


def test_the_qrdqn_and_c51_drop_ins_are_unchanged_by_the_shared_factory():
    from tianshou_amd.integration import make_hip_c51, make_hip_qrdqn

    assert make_hip_qrdqn(ref=SC).__name__ == "HipQRDQN" and make_hip_c51(ref=SC).__name__ == "HipC51"
    assert not hasattr(make_hip_qrdqn(ref=SC)(policy=SC.DiscreteQLearningPolicy(SC.QRDQNet(C_, H_, W_, A_, N_)), lr=1e-4,
                                             num_quantiles=N_, device="cpu"), "min_q_weight")


def test_ts_dcql_update_validates_before_any_hip_call():
    """NULL pointers, B < 1, a negative / non-finite min_q_weight and network dimensions outside make_net's range fail as
    TS_ERR_INVALID_ARG on a workspace that has never touched a device (ts_workspace_create only allocates host memory; the dummy
    pointers are never dereferenced), and a NULL workspace as TS_ERR_WORKSPACE."""
    import ctypes as C

    from tianshou_amd import _lib, distq
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    hp = distq.DistQHParams(-1.0, 0.9, 0.999, 1e-8, 0.0, -10.0, 10.0)
    d = C.c_void_p(4096)

    def call(ws=ws, params=d, act=d, ret=d, hp_=C.byref(hp), B=5, mqw=1.0, n_act=3, n_atoms=21, prio=d, loss3=d, tau=d):
        return lib.ts_dcql_update(ws, params, d, d, C.c_int64(1), C.c_int64(2), C.c_int64(44), C.c_int64(36), C.c_int64(n_act),
                                  C.c_int64(n_atoms), tau, d, 1, act, ret, None, C.c_int64(B), hp_, C.c_double(mqw), prio, loss3,
                                  None, None)

    try:
        assert call(ws=None) == _lib.TS_ERR_WORKSPACE
        for kw in (dict(params=None), dict(act=None), dict(ret=None), dict(hp_=None), dict(prio=None), dict(loss3=None),
                   dict(tau=None), dict(B=0), dict(B=-3), dict(n_act=65), dict(n_act=0), dict(n_atoms=1), dict(n_atoms=257)):
            assert call(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
            assert call(mqw=bad) == _lib.TS_ERR_INVALID_ARG, bad
            assert b"min_q_weight" in lib.ts_last_error()
    finally:
        lib.ts_workspace_destroy(ws)


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_hip_discrete_cql_wrapper_runs_with_engine_double(monkeypatch):
    """One update() of HipDiscreteCQL over a CPU double of DiscreteCQLEngine (the pattern of tests/test_integration_shim.py):
    the config with `min_q_weight`, the three statistics, and the write-back of parameters, lagged network and
    Adam state."""
    import numpy as np
    from tianshou.algorithm.imitation.discrete_cql import DiscreteCQLTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.env.atari.atari_network import QRDQNet
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.dcql as CQ
    import tianshou_amd.dqn as D
    from tests.test_integration_shim import _fill, _patch_for_cpu

    seen = {}

    class FakeCQL:
        def __init__(self, c, h, w, n_act, flat, cfg):
            assert (c, h, w, n_act) == (4, 84, 84, 6) and (cfg.kind, cfg.n_atoms, cfg.min_q_weight) == ("qr", N_, 2.5)
            assert (cfg.target_update_freq, cfg.lr) == (2, 1e-4)
            assert flat.numel() == 8224 + 32832 + 36928 + 3137 * 512 + 513 * ((6 * N_ + 31) // 32 * 32)
            self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
            self.params, self.params_old = flat.clone(), flat.clone()
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

        def preprocess(self, m, frames, idx, stack, obs_next_frames=None):
            assert frames.dtype == torch.uint8 and stack == 1 and obs_next_frames is not None
            return torch.zeros((idx.numel(), N_))

        def update_with_batch(self, obs, act, ret, weight=None, obs_next_nhwc=None):
            assert obs.shape == (8, 84, 84, 4) and ret.shape == (8, N_) and obs_next_nhwc is None
            seen["min_q_weight"] = self.cfg.min_q_weight
            self.adam_step += 1
            self.iter += 1
            self.params += 2.0
            self.params_old += 0.5
            self.adam_m += 0.125
            return torch.tensor([1.75, 0.5, 0.25]), torch.arange(8, dtype=torch.float32)

    algo = _make(QRDQNet(c=4, h=84, w=84, action_shape=[6], num_quantiles=N_), min_q_weight=2.5, target_update_freq=2)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(CQ, "DiscreteCQLEngine", FakeCQL)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    first = next(iter(algo.policy.model.parameters()))
    old_first = next(iter(algo.model_old.parameters()))
    before = first.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, DiscreteCQLTrainingStats) and (stats.loss, stats.qr_loss, stats.cql_loss) == (1.75, 0.5, 0.25)
    assert seen["min_q_weight"] == 2.5
    assert torch.allclose(first.detach(), before + 2.0)                        # engine -> nn.Parameter
    st = algo.optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125))
    assert old_first is not first and torch.allclose(old_first.detach(), before + 0.5)      # lagged network: its own values
