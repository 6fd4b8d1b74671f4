"""Minimal stand-ins of the reference's classes behind examples/atari/atari_sac.py for the GPU tests (the reference package is
absent on the GPU box), on top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_discrete_sac_cnn`
touches, plus the forward passes bench_dsac_cnn.py's eager baseline runs.  test_dsac_cnn_shim.py checks them against the real
classes where the reference is mounted."""
import copy

import torch
from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_discrete_sac_cnn(ref=...) resolves every name in one namespace)


class DQNet(SI.DQNetFeatures):
    """env/atari/atari_network.py:60-122 with features_only=True and output_dim_added_layer: `net` = Sequential(Sequential(conv,
    ReLU, conv, ReLU, conv, ReLU, Flatten), Linear, ReLU); raw pixel values in, no scaling."""

    def __init__(self, c, h, w, action_shape=None, features_only=True, output_dim_added_layer=512):
        assert features_only and output_dim_added_layer is not None
        super().__init__(c, h, w, output_dim=output_dim_added_layer)

    def get_output_dim(self):
        return self.output_dim

    def forward(self, obs, state=None, info=None):
        return self.net(torch.as_tensor(obs, dtype=torch.float32, device=self.net[1].weight.device)), state


class DiscreteActor(SI.DiscreteActor):
    """utils/net/discrete.py:22-101 without hidden layers."""

    def __init__(self, *, preprocess_net, action_shape, softmax_output=True):
        super().__init__(preprocess_net, int(action_shape), softmax_output=softmax_output)

    def forward(self, obs, state=None, info=None):
        x, state = self.preprocess(obs, state)
        x = self.last.model(x)
        return (torch.softmax(x, dim=-1) if self.softmax_output else x), state


class DiscreteCritic(SI.DiscreteCritic):
    """utils/net/discrete.py:104-163 without hidden layers."""

    def __init__(self, *, preprocess_net, last_size=1):
        super().__init__(preprocess_net, last_size=last_size)

    def forward(self, obs, state=None, info=None):
        x, _ = self.preprocess(obs, state)
        return self.last.model(x)


class DiscreteSACPolicy(SI.Policy):
    """modelfree/discrete_sac.py:28-80: `actor`, `is_within_training_step`."""

    def __init__(self, *, actor, action_space=None, deterministic_eval=True):
        super().__init__(actor, action_space=action_space, deterministic_eval=deterministic_eval)


class DiscreteSAC(SI.DiscreteSAC):
    """modelfree/discrete_sac.py:83-145 over ddpg.py ActorDualCriticsOffPolicyAlgorithm: `critic2=None` deep-copies the first
    critic -- and with it the trunk (ddpg.py:228); `max_grad_norm` reaches the three optimizer wrappers."""

    def __init__(self, *, policy, critic, critic2=None, max_grad_norm=None, **kw):
        super().__init__(policy=policy, critic=critic, critic2=critic2 if critic2 is not None else copy.deepcopy(critic), **kw)
        for o in (self.policy_optim, self.critic_optim, self.critic2_optim):
            o._max_grad_norm = max_grad_norm
