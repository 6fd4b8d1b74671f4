"""What the SAC route tests share (tests/test_gpu_sac.py, tests/test_gpu_sac_edges.py): the replay buffer their row-indexed and
one-call entry points read."""
import numpy as np
import torch


def random_replay_buffer(obs_dim: int, act_dim: int, slots: int, n_env: int = 4, seed: int = 3):
    """A full DeviceReplayBuffer of `n_env` equal sub-buffers with N(0, 1) observations and rewards, actions in [-1, 1) and
    10 % terminations."""
    from tianshou_amd.buffer import DeviceReplayBuffer

    g = torch.Generator().manual_seed(seed)
    T = slots // n_env
    off = np.arange(n_env + 1, dtype=np.int64) * T
    return DeviceReplayBuffer(offset=off, last_index=off[:-1] + T - 1, lengths=np.full(n_env, T, np.int64),
                              insertion=np.zeros(n_env, np.int64), rew=torch.randn(slots, generator=g).double().numpy(),
                              terminated=(torch.rand(slots, generator=g) < 0.1).numpy(), truncated=np.zeros(slots, bool),
                              obs=torch.randn(slots, obs_dim, generator=g).numpy(),
                              act=(torch.rand(slots, act_dim, generator=g) * 2 - 1).numpy(),
                              obs_next=torch.randn(slots, obs_dim, generator=g).numpy())
