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


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_hip_iqn_wrapper_runs_with_engine_double(monkeypatch):
    """One update() of HipIQN over a CPU double of IQNEngine (the pattern of tests/test_integration_shim.py): hook order and
    arguments, the statistics, and the write-back of parameters, lagged network and Adam state."""
    import numpy as np
    from tianshou.algorithm.modelfree.reinforce import SimpleLossTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.dqn as D
    import tianshou_amd.iqn as I
    from tests.test_integration_shim import _fill, _patch_for_cpu

    calls = []

    class FakeIQN:
        def __init__(self, c, h, w, n_act, flat, cfg):
            assert (c, h, w, n_act) == (4, 84, 84, 6)
            assert (cfg.n_cos, cfg.sample_size, cfg.online_sample_size, cfg.target_sample_size) == (64, 9, 5, 7)
            assert (cfg.target_update_freq, cfg.lr, cfg.seed) == (2, 1e-4, 3)
            assert flat.numel() == (8 * 8 * 4 + 1) * 32 + 513 * 64 + 577 * 64 + 65 * 3136 + 3137 * 512 + 513 * 32
            self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
            self.params, self.params_old = flat.clone(), flat.clone()
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0
            self.tau_counter = 0

        def preprocess(self, m, frames, idx, stack, obs_next_frames=None, tau_online=None, tau_target=None):
            assert frames.dtype == torch.uint8 and stack == 1 and obs_next_frames is not None
            assert tau_online is None and tau_target is None                   # no hip_taus: the engine's own stream
            calls.append("preprocess")
            self.tau_counter += 2
            return torch.zeros((idx.numel(), 7))

        def update_with_batch(self, obs, act, ret, weight=None, tau=None):
            assert obs.shape == (8, 84, 84, 4) and obs.dtype == torch.uint8 and ret.shape == (8, 7) and tau is None
            calls.append("update")
            self.tau_counter += 1
            self.adam_step += 1
            self.iter += 1
            self.params += 2.0
            self.params_old += 0.5
            self.adam_m += 0.125
            return torch.tensor([0.5]), torch.arange(8, dtype=torch.float32)

    _, make = _classes()
    algo = make(_iqn_net([512], c=4, h=84, w=84, n_act=6), 6, hip_seed=3)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(I, "IQNEngine", FakeIQN)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    first = next(iter(algo.policy.model.parameters()))
    old_first = next(iter(algo.model_old.parameters()))
    before = first.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, SimpleLossTrainingStats) and stats.loss == 0.5 and calls == ["preprocess", "update"]
    assert torch.allclose(first.detach(), before + 2.0)                        # engine -> nn.Parameter
    st = algo.optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125))
    assert old_first is not first and torch.allclose(old_first.detach(), before + 0.5)      # lagged network: its own values
    assert algo.hip_extra_state() == {"tau_seed": 3, "tau_counter": 3}
