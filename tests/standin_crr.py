"""Minimal stand-ins of the reference's DiscreteCRR classes for the GPU tests (the reference package is absent on the GPU
box), on top of tests/standin.py and tests/standin_bcq.py: the attribute surface
`tianshou_amd.integration.make_hip_discrete_crr` touches and nothing else.  test_crr_shim.py checks them against the real
classes where the reference is mounted."""
import copy
from dataclasses import dataclass

import numpy as np
from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_discrete_crr(ref=...) resolves every name in one namespace)
from tests.standin_bcq import DiscreteActor, DQNetFeaturesOnly  # noqa: F401


class DiscreteCritic(nn.Module):
    """utils/net/discrete.py:94-123 with hidden layers: `preprocess`, `last` = MLP(hidden_sizes + last_size outputs)."""

    def __init__(self, *, preprocess_net, hidden_sizes=(), last_size=1):
        super().__init__()
        self.preprocess = preprocess_net
        self.last = SI._MLP([preprocess_net.get_output_dim(), *hidden_sizes, last_size], nn.ReLU)
        self.last.model = nn.Sequential(*list(self.last.model)[:-1])

    def forward(self, obs, state=None, info=None):
        x, _ = self.preprocess(obs, state)
        return self.last.model(x)


class DiscreteActorPolicy(SI.Policy):
    """modelfree/reinforce.py DiscreteActorPolicy: `actor`, `is_within_training_step`."""

    def __init__(self, *, actor, action_space=None):
        super().__init__(actor, action_space=action_space)


@dataclass(kw_only=True)
class DiscreteCRRTrainingStats(SI.SimpleLossTrainingStats):
    """imitation/discrete_crr.py:26-30."""
    actor_loss: float
    critic_loss: float
    cql_loss: float


class DiscreteCRR(SI.Algorithm):
    """imitation/discrete_crr.py:33-123: ONE optimizer over ModuleList([policy, critic]), `discounted_return_computation`,
    `_target`, `_freq`, `_iter`, `actor_old` / `critic_old` = two lagged deep copies (the live modules with
    target_update_freq == 0), the four scalars.  `_preprocess_batch` stands in for add_discounted_returns, whose result the
    update never reads: it writes zeros and counts its calls."""

    def __init__(self, *, policy, critic, lr=1e-4, gamma=0.99, policy_improvement_mode="exp", ratio_upper_bound=20.0, beta=1.0,
                 min_q_weight=10.0, target_update_freq=0, return_standardization=False, max_grad_norm=None, optim=None):
        super().__init__(policy)
        self.discounted_return_computation = SI.DiscountedReturnComputation(gamma, return_standardization)
        self.critic = critic
        self.optim = self._create_optimizer(nn.ModuleList([self.policy, self.critic]), lr, max_grad_norm, optim=optim)
        self._target = target_update_freq > 0
        self._freq = target_update_freq
        self._iter = 0
        if self._target:
            self.actor_old = SI.EvalModeModuleWrapper(copy.deepcopy(self.policy.actor))
            self.critic_old = SI.EvalModeModuleWrapper(copy.deepcopy(self.critic))
        else:
            # (as the reference: plain attributes would register the live modules a second time; nn.Module allows it)
            self.actor_old = self.policy.actor
            self.critic_old = self.critic
        self._policy_improvement_mode = policy_improvement_mode
        self._ratio_upper_bound = ratio_upper_bound
        self._beta = beta
        self._min_q_weight = min_q_weight
        self.base_preprocess_calls = 0

    def _preprocess_batch(self, batch, buffer, indices):
        self.base_preprocess_calls += 1
        batch.returns = np.zeros(len(indices))
        return batch

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))
