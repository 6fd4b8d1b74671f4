"""Minimal stand-ins of the reference's IQN classes for the GPU tests (the reference package is absent on the GPU box), on top
of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_iqn` touches and nothing else.
test_oracle_iqn.py checks them against the real classes where the reference is mounted."""
import torch
from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_iqn(ref=...) resolves every name in one namespace)


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


class CosineEmbeddingNetwork(nn.Module):
    """utils/net/discrete.py:126-160: `net` = Sequential(Linear(num_cosines, embedding_dim), ReLU)."""

    def __init__(self, num_cosines, embedding_dim):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(num_cosines, embedding_dim), nn.ReLU())
        self.num_cosines, self.embedding_dim = num_cosines, embedding_dim


class ImplicitQuantileNetwork(nn.Module):
    """utils/net/discrete.py:163-216: `preprocess`, `last` (MLP: hidden layers + n_act outputs), `embed_model`, in the
    reference's construction order (the state_dict order and the RNG consumption follow from it)."""

    def __init__(self, *, preprocess_net, action_shape, hidden_sizes=(), num_cosines=64):
        super().__init__()
        n_act = int(action_shape[0]) if hasattr(action_shape, "__len__") else int(action_shape)
        self.preprocess = preprocess_net
        self.input_dim = preprocess_net.get_output_dim()
        self.last = SI._MLP([self.input_dim, *hidden_sizes, n_act], nn.ReLU)
        self.last.model = nn.Sequential(*list(self.last.model)[:-1])          # no activation behind the output layer
        self.embed_model = CosineEmbeddingNetwork(num_cosines, self.input_dim)


class IQNPolicy(SI.DiscreteQLearningPolicy):
    """modelfree/iqn.py:21-70: `model`, the three sample sizes, `is_within_training_step`."""

    def __init__(self, *, model, sample_size=32, online_sample_size=8, target_sample_size=8):
        super().__init__(model)
        self.sample_size, self.online_sample_size, self.target_sample_size = sample_size, online_sample_size, target_sample_size


class IQN(SI.QRDQN):
    """modelfree/iqn.py:103-154: QRDQN's attributes."""

    def __init__(self, *, policy, lr=1e-4, gamma=0.99, num_quantiles=200, n_step_return_horizon=1, target_update_freq=0,
                 max_grad_norm=None):
        super().__init__(policy=policy, lr=lr, gamma=gamma, num_quantiles=num_quantiles,
                         n_step_return_horizon=n_step_return_horizon, target_update_freq=target_update_freq,
                         max_grad_norm=max_grad_norm)
