"""Minimal stand-ins of the reference's DiscreteBCQ classes for the GPU tests (the reference package is absent on the GPU
box), on top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_discrete_bcq` touches and nothing
else.  test_oracle_bcq.py checks them against the real classes where the reference is mounted."""
import copy
import math
from dataclasses import dataclass

import numpy as np
import torch
from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_discrete_bcq(ref=...) resolves every name in one namespace)


class DQNetFeaturesOnly(nn.Module):
    """env/atari/atari_network.py:60-122 with features_only=True and no added layer: `net` = Sequential(conv, ReLU, conv,
    ReLU, conv, ReLU, Flatten); `output_dim`."""

    def __init__(self, c, h, w):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(c, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, 4, 2), nn.ReLU(), nn.Conv2d(64, 64, 3, 1),
                                 nn.ReLU(), nn.Flatten())
        with torch.no_grad():
            self.output_dim = int(self.net(torch.zeros(1, c, h, w)).shape[1])

    def get_output_dim(self):
        return self.output_dim

    def forward(self, obs, state=None, info=None):
        return self.net(torch.as_tensor(obs, dtype=torch.float32, device=self.net[0].weight.device)), state


class DiscreteActor(nn.Module):
    """utils/net/discrete.py:22-101 with hidden layers: `preprocess`, `last` = MLP(hidden_sizes + n_act outputs, no activation
    behind the output layer), `softmax_output`."""

    def __init__(self, *, preprocess_net, action_shape, hidden_sizes=(), softmax_output=True):
        super().__init__()
        n_act = int(action_shape[0]) if hasattr(action_shape, "__len__") else int(action_shape)
        self.preprocess = preprocess_net
        self.last = SI._MLP([preprocess_net.get_output_dim(), *hidden_sizes, n_act], nn.ReLU)
        self.last.model = nn.Sequential(*list(self.last.model)[:-1])
        self.softmax_output = softmax_output

    def forward(self, obs, state=None, info=None):
        x, state = self.preprocess(obs, state)
        x = self.last.model(x)
        return (torch.softmax(x, dim=-1) if self.softmax_output else x), state


class DiscreteBCQPolicy(SI.DiscreteQLearningPolicy):
    """imitation/discrete_bcq.py:37-127: `model`, `imitator`, `_log_tau`, `is_within_training_step`."""

    def __init__(self, *, model, imitator, target_update_freq=8000, unlikely_action_threshold=0.3):
        super().__init__(model)
        self.imitator = imitator
        assert target_update_freq > 0, f"BCQ needs target_update_freq>0 but got: {target_update_freq}."
        assert 0.0 <= unlikely_action_threshold < 1.0
        self._log_tau = math.log(unlikely_action_threshold) if unlikely_action_threshold > 0 else -np.inf


@dataclass(kw_only=True)
class DiscreteBCQTrainingStats(SI.SimpleLossTrainingStats):
    """imitation/discrete_bcq.py:30-34."""
    q_loss: float
    i_loss: float
    reg_loss: float


class DiscreteBCQ(SI.Algorithm):
    """imitation/discrete_bcq.py:130-211: ONE optimizer over the whole policy, `gamma`, `n_step`, `freq`, `_iter`, `_weight_reg`,
    `model_old` = a lagged copy of `policy.model` alone."""

    def __init__(self, *, policy, lr=1e-4, gamma=0.99, n_step_return_horizon=1, target_update_freq=8000,
                 imitation_logits_penalty=1e-2, max_grad_norm=None, optim=None):
        super().__init__(policy)
        self.optim = self._create_optimizer(policy, lr, max_grad_norm, optim=optim)
        self.gamma, self.n_step = gamma, n_step_return_horizon
        self._target = target_update_freq > 0
        self.freq = target_update_freq
        self._iter = 0
        if self._target:
            self.model_old = SI.EvalModeModuleWrapper(copy.deepcopy(policy.model))
        self._weight_reg = imitation_logits_penalty

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))
