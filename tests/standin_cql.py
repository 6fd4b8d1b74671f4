"""Minimal stand-in of the reference's CQL class for the GPU tests (the reference package is absent on the GPU box), on top of
tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_cql` touches and nothing else.
test_cql_shim.py checks it against the real class where the reference is mounted."""
from dataclasses import dataclass

import torch

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_cql(ref=...) resolves every name in one namespace)


@dataclass(kw_only=True)
class CQLTrainingStats(SI.SACTrainingStats):
    """imitation/cql.py:19-28."""

    cql_alpha: float | None = None
    cql_alpha_loss: float | None = None


class CQL(SI.SAC):
    """imitation/cql.py:32-201: SAC's networks, lagged critics and optimizers (the critics' with `max_grad_norm`), the CQL
    hyper-parameters under the reference's names, `cql_log_alpha` and its plain torch.optim.Adam.  No n-step horizon."""

    def __init__(self, *, policy, critic, critic2, lr=1e-4, critic_lr=3e-4, cql_alpha_lr=1e-4, cql_weight=1.0, tau=0.005, gamma=0.99,
                 alpha=0.2, temperature=1.0, with_lagrange=True, lagrange_threshold=10.0, min_action=-1.0, max_action=1.0,
                 num_repeat_actions=10, alpha_min=0.0, alpha_max=1e6, max_grad_norm=1.0, calibrated=True):
        super().__init__(policy=policy, critic=critic, critic2=critic2, lr=lr, critic_lr=critic_lr, tau=tau, gamma=gamma, alpha=alpha)
        del self.n_step_return_horizon
        self.critic_optim._max_grad_norm = self.critic2_optim._max_grad_norm = max_grad_norm
        self.temperature, self.with_lagrange, self.lagrange_threshold, self.cql_weight = temperature, with_lagrange, lagrange_threshold, cql_weight
        self.cql_log_alpha = torch.tensor([0.0], requires_grad=True)
        self.cql_alpha_optim = torch.optim.Adam([self.cql_log_alpha], lr=cql_alpha_lr)
        self.min_action, self.max_action, self.num_repeat_actions = min_action, max_action, num_repeat_actions
        self.alpha_min, self.alpha_max, self.calibrated = alpha_min, alpha_max, calibrated

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))
