"""Minimal stand-in of the reference's GAIL class for the GPU tests (the reference package is absent on the GPU box), on top of
tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_gail` touches and nothing else.
test_gail_shim.py checks it against the real class where the reference is mounted."""
from dataclasses import dataclass

import numpy as np

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_gail(ref=...) resolves every name in one namespace)


@dataclass(kw_only=True)
class GailTrainingStats(SI.A2CTrainingStats):
    """imitation/gail.py:24-28."""
    disc_loss: SI.SequenceSummaryStats
    acc_pi: SI.SequenceSummaryStats
    acc_exp: SI.SequenceSummaryStats


class ExpertBuffer:
    """A full, plain ReplayBuffer as GAIL reads it (data/buffer/buffer_base.py:98, 503-517): `obs` / `act` storage, `__len__`,
    and `sample_indices(batch_size)` = `_random_state.choice(size, batch_size)` from the buffer's own RandomState(random_seed)."""

    def __init__(self, obs, act, random_seed=42):
        self.obs, self.act = np.asarray(obs, np.float32), np.asarray(act, np.float32)
        self.maxsize = self._size = len(self.obs)
        self._random_state = np.random.RandomState(random_seed)

    def __len__(self):
        return self._size

    def sample_indices(self, batch_size):
        return self._random_state.choice(self._size, batch_size)


class GAIL(SI.PPO):
    """imitation/gail.py:30-191: PPO's attributes plus `expert_buffer`, `disc_net`, `disc_optim` (created AFTER PPO's optimizer:
    second in `_optimizers`), `disc_update_num`, `action_dim`.  The stand-in takes the discriminator optimizer's learning rate and
    clipping norm instead of a factory, as tests/standin.py's classes do."""

    def __init__(self, *, policy, critic, expert_buffer, disc_net, disc_lr=1e-3, disc_max_grad_norm=None, disc_optim=None,
                 disc_update_num=4, **kw):
        super().__init__(policy=policy, critic=critic, **kw)
        self.disc_net = disc_net
        self.disc_optim = self._create_optimizer(self.disc_net, disc_lr, disc_max_grad_norm, optim=disc_optim)
        self.disc_update_num = disc_update_num
        self.expert_buffer = expert_buffer
        self.action_dim = int(policy.actor.mu.model[0].out_features)
