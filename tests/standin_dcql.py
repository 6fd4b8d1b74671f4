"""Minimal stand-ins of the reference's DiscreteCQL classes for the GPU tests (the reference package is absent on the GPU
box), on top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_discrete_cql` touches and nothing
else.  test_oracle_dcql.py checks them against the real classes where the reference is mounted."""
from dataclasses import dataclass

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_discrete_cql(ref=...) resolves every name in one namespace)


@dataclass(kw_only=True)
class DiscreteCQLTrainingStats(SI.SimpleLossTrainingStats):
    """imitation/discrete_cql.py:16-19."""
    cql_loss: float
    qr_loss: float


class DiscreteCQL(SI.QRDQN):
    """imitation/discrete_cql.py:23-78: QRDQN's attributes plus `min_q_weight`.  `optim` = (torch.optim class, kwargs) stands
    for another OptimizerFactory than Adam's."""

    def __init__(self, *, policy, lr=1e-4, min_q_weight=10.0, gamma=0.99, num_quantiles=200, n_step_return_horizon=1,
                 target_update_freq=0, max_grad_norm=None, optim=None):
        super().__init__(policy=policy, lr=lr, gamma=gamma, num_quantiles=num_quantiles,
                         n_step_return_horizon=n_step_return_horizon, target_update_freq=target_update_freq,
                         max_grad_norm=max_grad_norm)
        if optim is not None:
            self._optimizers.clear()
            self.optim = self._create_optimizer(policy, lr, max_grad_norm, optim=optim)
        self.min_q_weight = min_q_weight
