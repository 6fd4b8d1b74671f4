"""CPU: the HipIQN drop-in (tianshou_amd.integration.make_hip_iqn) without an engine -- over the real reference classes where
the reference is mounted, over tests/standin_iqn.py otherwise: the model check and the fraction counter's save / restore."""
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_iqn as SQ

REAL = ref_shim.reference_available()


def _classes():
    """-> (HipIQN, make_algo(model, **kw)) over the real classes or the stand-ins."""
    from tianshou_amd.integration import make_hip_iqn

    if REAL:
        ref_shim.install()
        import gymnasium as gym
        from tianshou.algorithm.modelfree.iqn import IQNPolicy
        from tianshou.algorithm.optim import AdamOptimizerFactory

        Hip = make_hip_iqn()

        def make(model, n_act, **kw):
            policy = IQNPolicy(model=model, action_space=gym.spaces.Discrete(n_act), sample_size=9, online_sample_size=5,
                               target_sample_size=7)
            return Hip(policy=policy, optim=AdamOptimizerFactory(lr=1e-4), target_update_freq=2, device="cpu", **kw)
    else:
        Hip = make_hip_iqn(ref=SQ)

        def make(model, n_act, **kw):
            policy = SQ.IQNPolicy(model=model, sample_size=9, online_sample_size=5, target_sample_size=7)
            return Hip(policy=policy, lr=1e-4, target_update_freq=2, device="cpu", **kw)
    return Hip, make


def _iqn_net(hidden, c=2, h=44, w=36, n_act=3, mlp=False):
    if REAL:
        from tianshou.env.atari.atari_network import DQNet
        from tianshou.utils.net.common import Net
        from tianshou.utils.net.discrete import ImplicitQuantileNetwork

        pre = Net(state_shape=(8,), hidden_sizes=[64, 64]) if mlp else DQNet(c=c, h=h, w=w, action_shape=[n_act], features_only=True)
        return ImplicitQuantileNetwork(preprocess_net=pre, action_shape=[n_act], hidden_sizes=hidden, num_cosines=64)

    class MlpPre(nn.Module):                      # the `Net` MLP of test/discrete/test_iqn.py, as far as its keys go
        def __init__(self):
            super().__init__()
            self.model = SQ.SI._MLP([8, 64, 64], nn.ReLU)

        def get_output_dim(self):
            return 64

    pre = MlpPre() if mlp else SQ.DQNetFeaturesOnly(c, h, w)
    return SQ.ImplicitQuantileNetwork(preprocess_net=pre, action_shape=[n_act], hidden_sizes=hidden, num_cosines=64)


def test_supported_model_is_accepted():
    _, make = _classes()
    algo = make(_iqn_net([512]), 3)
    assert type(algo).__name__ == "HipIQN" and algo.model_old is not None


def test_mlp_preprocess_net_is_rejected():
    _, make = _classes()
    with pytest.raises(NotImplementedError, match="DQNet\\(features_only=True\\)"):
        make(_iqn_net([512], mlp=True), 3)


@pytest.mark.parametrize("hidden", [[256], [], [512, 512]])
def test_other_hidden_sizes_are_rejected(hidden):
    _, make = _classes()
    with pytest.raises(NotImplementedError, match="hidden_sizes=\\[512\\]"):
        make(_iqn_net(hidden), 3)


def test_fraction_counter_survives_extra_state():
    _, make = _classes()
    algo = make(_iqn_net([512]), 3, hip_seed=11)
    assert algo.hip_extra_state() == {"tau_seed": 11, "tau_counter": 0}
    # a stub in place of the engine: the live counter is the engine's
    stub = SimpleNamespace(tau_counter=42, cfg=SimpleNamespace(seed=11))
    algo.__dict__["_hip_engine_obj"] = stub
    state = algo.hip_extra_state()
    assert state == {"tau_seed": 11, "tau_counter": 42}
    other = make(_iqn_net([512]), 3)
    other.load_hip_extra_state(state)                       # before the engine exists: kept for its construction
    assert other.hip_extra_state() == state and other._hip_tau_counter == 42 and other._hip_seed == 11
    stub2 = SimpleNamespace(tau_counter=0, cfg=SimpleNamespace(seed=0))
    other.__dict__["_hip_engine_obj"] = stub2
    other.load_hip_extra_state(state)                       # with an engine: written through
    assert stub2.tau_counter == 42 and stub2.cfg.seed == 11


def test_hip_taus_are_consumed_in_call_order():
    _, make = _classes()
    seq = [torch.full((2, 5), 0.1), torch.full((2, 7), 0.2), torch.full((2, 5), 0.3)]
    algo = make(_iqn_net([512]), 3, hip_taus=iter(seq))
    assert [float(algo._hip_next_tau()[0, 0]) for _ in range(3)] == pytest.approx([0.1, 0.2, 0.3])
    calls = []
    algo2 = make(_iqn_net([512]), 3, hip_taus=lambda: calls.append(1) or seq[0])
    assert tuple(algo2._hip_next_tau().shape) == (2, 5) and calls == [1]
    assert make(_iqn_net([512]), 3)._hip_next_tau() is None
