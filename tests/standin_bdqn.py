"""Minimal stand-ins of the reference's Branching DQN classes for the GPU tests (the reference package is absent on the GPU box), on
top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_bdqn` touches and nothing else -- no loss, no
target.  tests/test_bdqn_shim.py checks them against the real classes where the reference is mounted."""
import copy

from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_bdqn(ref=...) resolves every name in one namespace)


class MLP(nn.Module):
    """utils/net/common.py:90-178: `.model` = Sequential(Linear, [norm,] act, ..., [Linear]) -- an activation behind every hidden
    Linear, an output Linear only when output_dim > 0 -> state_dict keys `model.{0,2,...}.{weight,bias}` without a norm layer."""

    def __init__(self, input_dim, output_dim=0, hidden_sizes=(), norm_layer=None, activation=nn.ReLU):
        super().__init__()
        layers, k = [], input_dim
        for h in hidden_sizes:
            layers.append(nn.Linear(k, h))
            if norm_layer is not None:
                layers.append(norm_layer(h))
            if activation is not None:
                layers.append(activation())
            k = h
        if output_dim > 0:
            layers.append(nn.Linear(k, output_dim))
        self.model = nn.Sequential(*layers)
        self.output_dim = output_dim or k


class BranchingNet(nn.Module):
    """utils/net/common.py:553-674: `common` (its last hidden layer is its output), `value` -> 1, `branches` = ModuleList of
    num_branches MLPs -> action_per_branch; `num_branches`, `action_per_branch`."""

    def __init__(self, *, state_shape, num_branches=0, action_per_branch=2, common_hidden_sizes=None, value_hidden_sizes=None,
                 action_hidden_sizes=None, norm_layer=None, activation=nn.ReLU):
        super().__init__()
        common, value, action = common_hidden_sizes or [], value_hidden_sizes or [], action_hidden_sizes or []
        self.num_branches, self.action_per_branch = num_branches, action_per_branch
        kw = dict(norm_layer=norm_layer, activation=activation)
        self.common = MLP(int(state_shape), 0, common, **kw)
        self.value = MLP(common[-1], 1, value, **kw)
        self.branches = nn.ModuleList([MLP(common[-1], action_per_branch, action, **kw) for _ in range(num_branches)])

    def forward(self, obs, state=None, info=None):
        """common.py:658-674 (used by the tests to act with the written-back parameters, never by the hooks)."""
        import torch

        h = self.common.model(obs)
        v = self.value.model(h).unsqueeze(1)
        adv = torch.stack([b.model(h) for b in self.branches], 1)
        return v + (adv - adv.mean(2, keepdim=True)), state


class BDQNPolicy(SI.DiscreteQLearningPolicy):
    """modelfree/bdqn.py:29-103: a DiscreteQLearningPolicy over a BranchingNet."""


class BDQN(SI.Algorithm):
    """modelfree/bdqn.py:106-224 over QLearningOffPolicyAlgorithm (dqn.py:190-285): `optim` over the policy, `gamma`, `n_step` = 1,
    `target_update_freq`, `is_double`, `_iter`, `model_old` (an EvalModeModuleWrapper around a deep copy, or None),
    `_compute_return(batch, buffer, indice, gamma=0.99)` -- the default the reference's `_preprocess_batch` ends up using.  The
    stand-in takes the optimizer's learning rate instead of a factory, as tests/standin.py's classes do."""

    def __init__(self, *, policy, lr=1e-3, optim=None, max_grad_norm=None, gamma=0.99, target_update_freq=0, is_double=True):
        super().__init__(policy)
        self.optim = self._create_optimizer(policy, lr, max_grad_norm, optim=optim)
        self.gamma, self.n_step, self.target_update_freq, self.is_double = gamma, 1, target_update_freq, is_double
        self._iter = 0
        self.model_old = SI.EvalModeModuleWrapper(copy.deepcopy(policy.model)) if target_update_freq > 0 else None

    def _compute_return(self, batch, buffer, indice, gamma=0.99):
        raise NotImplementedError("stand-in: the hooks under test replace the target computation")

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))
