"""HipSAC / HipDQN over the stand-ins (tests/standin.py) at small sizes, with their buffers and fills: the algorithms of the
default-mode-vs-reference-exact tests (tests/test_gpu_hooks.py) and of the lazy write-back state matrix
(tests/test_gpu_lazy_state.py), which drive a reference-exact twin (`host_batch=True, write_back="eager"`) and a default twin
through the same operations."""
import numpy as np
import torch
from torch import nn

from tests import standin as SI

SAC_OBS, SAC_ACT, SAC_ENVS, SAC_BATCH = 23, 5, 4, 64
DQN_C, DQN_H, DQN_W, DQN_ACT, DQN_ENVS, DQN_SIZE, DQN_BATCH = 4, 44, 36, 3, 4, 40, 32


def fill_vector(buf, T, obs_dim, act_dim, rng):
    """T vector steps of Gaussian observations / actions / rewards with random terminations and truncations."""
    E = buf.buffer_num
    obs = rng.normal(size=(T + 1, E, obs_dim)).astype(np.float32)
    for t in range(T):
        term = rng.random(E) < 0.03
        buf.add(SI.Batch(obs=obs[t], act=rng.normal(size=(E, act_dim)).astype(np.float32),
                         rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.02) & ~term, obs_next=obs[t + 1]))


# ------------------------------------------------------------------------------------ HipSAC
def sac_build(update_noise="torch", **kw):
    from tianshou_amd.integration import make_hip_sac

    obs_dim, act_dim = SAC_OBS, SAC_ACT
    torch.manual_seed(11)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [256, 256], nn.ReLU), act_dim, unbounded=True, conditioned_sigma=True)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
    c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
    algo = make_hip_sac(ref=SI)(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=1e-3, tau=0.01, gamma=0.97,
                                alpha=SI.AutoAlpha(-float(act_dim), -0.5, 3e-4), device="cuda", update_noise=update_noise,
                                **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return algo


def sac_buffer():
    return SI.VectorReplayBuffer(SAC_ENVS * 200, SAC_ENVS, obs_shape=(SAC_OBS,), act_shape=(SAC_ACT,), seed=4)


def sac_fill(buf, rng, T):
    fill_vector(buf, T, SAC_OBS, SAC_ACT, rng)


# ------------------------------------------------------------------------------------ HipDQN
def dqn_build(**kw):
    from tianshou_amd.integration import make_hip_dqn

    torch.manual_seed(5)
    model = SI.DQNet(DQN_C, DQN_H, DQN_W, DQN_ACT)
    with torch.no_grad():
        model.net[0][0].weight.mul_(1.0 / 255.0)     # uint8 frames (0..255) times default-init weights: keep Q values O(1)
    algo = make_hip_dqn(ref=SI)(policy=SI.DiscreteQLearningPolicy(model), lr=1e-4, gamma=0.97, n_step_return_horizon=3,
                                target_update_freq=2, is_double=True, huber_loss_delta=None, device="cuda", **kw).to("cuda")
    algo.policy.is_within_training_step = True
    return algo


def dqn_buffer(layout):
    """`stored_obs_next`, or `atari_frames`: ReplayBuffer(ignore_obs_next=True, save_only_last_obs=True) as
    examples/atari/atari_dqn.py builds it (the default mode's one-call ts_dqn_learn_rows path)."""
    buf = SI.PrioritizedVectorReplayBuffer(DQN_ENVS * DQN_SIZE, DQN_ENVS, obs_shape=(DQN_H, DQN_W), act_shape=(), obs_dtype=np.uint8,
                                           act_dtype=np.int64, seed=2, stack_num=DQN_C, alpha=0.6, beta=0.4)
    if layout == "atari_frames":
        buf._meta = SI._Meta(("obs", "act", "rew", "terminated", "truncated", "done"))        # ignore_obs_next=True
    return buf


def dqn_fill(buf, rng, n):
    E, h, w = DQN_ENVS, DQN_H, DQN_W
    for _ in range(n):
        term = rng.random(E) < 0.08
        buf.add(SI.Batch(obs=rng.integers(0, 256, (E, h, w)).astype(np.uint8), act=rng.integers(0, DQN_ACT, E),
                         rew=rng.normal(size=E), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                         obs_next=rng.integers(0, 256, (E, h, w)).astype(np.uint8)))
