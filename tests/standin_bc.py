"""Minimal stand-ins of the reference's vanilla imitation-learning classes for the GPU tests (the reference package is absent on
the GPU box), on top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_imitation` touches and nothing
else.  test_bc_shim.py checks them against the real classes where the reference is mounted."""
from dataclasses import dataclass

import torch
from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_imitation(ref=...) resolves every name in one namespace)


@dataclass(kw_only=True)
class ImitationTrainingStats:
    """imitation_base.py:32-34 (TrainingStats' own fields left out)."""

    loss: float = 0.0
    train_time: float = 0.0


class Discrete:
    """gymnasium.spaces.Discrete: `n`."""

    def __init__(self, n):
        self.n = int(n)


class ActionNet(nn.Module):
    """utils/net/common.py:246-369, Net(state_shape, action_shape, hidden_sizes): the MLP ends in a bare Linear layer of
    action_shape outputs -> state_dict keys `model.model.{0, 2, ..., 2 d}.{weight, bias}`; forward -> (logits, state)."""

    def __init__(self, in_dim, n_act, hidden_sizes, activation=nn.ReLU, norm_layer=None):
        super().__init__()
        self.model = SI._MLP([in_dim, *hidden_sizes], activation, norm_layer=norm_layer)
        self.model.model.append(nn.Linear(hidden_sizes[-1], n_act))
        self.softmax, self.use_dueling = False, False

    def forward(self, obs, state=None, info=None):
        x = torch.as_tensor(obs, dtype=torch.float32, device=next(self.parameters()).device)
        return self.model.model(x.flatten(1)), state


class ImitationPolicy(SI.Policy):
    """imitation_base.py:37-105: `actor`, `action_type` (algorithm_base.py Policy: "discrete" for a Discrete action space,
    "continuous" for a Box), the action-bound fields of `map_action`."""

    def __init__(self, *, actor, action_space, observation_space=None, action_scaling=False, action_bound_method="clip"):
        super().__init__(actor, action_space=action_space, action_scaling=action_scaling, action_bound_method=action_bound_method)
        self.action_type = "continuous" if isinstance(action_space, SI.Box) else "discrete"


class _Imitation(SI.Algorithm):
    """imitation_base.py:130-183: one optimizer over the policy; `_preprocess_batch` is the base class's (the batch as sampled)."""

    def __init__(self, *, policy, lr=1e-3, optim=None, max_grad_norm=None):
        super().__init__(policy)
        self.optim = self._create_optimizer(policy, lr, max_grad_norm, optim=optim)

    def _preprocess_batch(self, batch, buffer, indices):
        return batch

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))


class OffPolicyImitationLearning(_Imitation):
    pass


class OfflineImitationLearning(_Imitation):
    pass
