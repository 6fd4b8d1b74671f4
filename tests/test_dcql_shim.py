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
