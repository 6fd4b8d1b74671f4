"""Minimal stand-ins for the FQF-MLP tests (the reference package is absent on the GPU box): tests/standin_iqn_mlp.py's network with the
reference's FQF classes around it, the attribute surface `tianshou_amd.integration.make_hip_fqf_mlp` touches and nothing else
(real classes: tests/test_oracle_fqf_mlp.py)."""
from dataclasses import dataclass

import torch
from torch import nn

from tests.standin_iqn_mlp import *  # noqa: F401,F403  (make_hip_fqf_mlp(ref=...) resolves every name in one namespace)
from tests import standin_iqn_mlp as SI


class FractionProposalNetwork(nn.Module):
    """utils/net/discrete.py:219-237: `net` = Linear(embedding_dim, num_fractions), xavier_uniform(gain=0.01), zero bias."""

    def __init__(self, num_fractions, embedding_dim):
        super().__init__()
        self.net = nn.Linear(embedding_dim, num_fractions)
        torch.nn.init.xavier_uniform_(self.net.weight, gain=0.01)
        torch.nn.init.constant_(self.net.bias, 0)
        self.num_fractions, self.embedding_dim = num_fractions, embedding_dim


class FQFPolicy(SI.DiscreteQLearningPolicy):
    """modelfree/fqf.py:27-64: `model`, `fraction_model`."""

    def __init__(self, *, model, fraction_model):
        super().__init__(model)
        self.fraction_model = fraction_model


@dataclass(kw_only=True)
class FQFTrainingStats:
    """fqf.py:20-24."""
    loss: float
    quantile_loss: float
    fraction_loss: float
    entropy_loss: float


class FQF(SI.QRDQN):
    """fqf.py:109-176: QRDQN's attributes; `optim` over the model alone, `fraction_optim` (a (torch.optim class, kwargs) pair, as
    tests/standin.py's `_create_optimizer` takes it) over the fraction model, `ent_coef`."""

    def __init__(self, *, policy, lr=1e-4, fraction_optim=(torch.optim.RMSprop, {}), fraction_lr=2.5e-9, gamma=0.99, num_fractions=32,
                 ent_coef=0.0, n_step_return_horizon=1, target_update_freq=0, max_grad_norm=None):
        super().__init__(policy=policy, lr=lr, gamma=gamma, num_quantiles=num_fractions, n_step_return_horizon=n_step_return_horizon,
                         target_update_freq=target_update_freq, max_grad_norm=max_grad_norm)
        self._optimizers.clear()
        self.optim = self._create_optimizer(policy.model, lr, max_grad_norm)
        self.ent_coef = ent_coef
        self.fraction_optim = self._create_optimizer(policy.fraction_model, fraction_lr, optim=fraction_optim)


def build(layers, num_fractions, **kw):
    """-> (FullQuantileFunction, which holds ImplicitQuantileNetwork's modules and nothing more; FractionProposalNetwork)."""
    net = SI.build(layers, **kw)
    return net, FractionProposalNetwork(num_fractions, net.input_dim)
