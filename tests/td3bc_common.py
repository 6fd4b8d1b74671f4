"""Shared by the TD3+BC tests: the fixtures of tools/gen_golden_td3bc.py (tests/golden/td3bc_offline.npz, td3bc_per_tanh.npz)
and the engine built from oracle parameters."""
import os

import numpy as np

from oracle import oracle as O
from oracle import oracle_sac as OS
from tests import oracle_td3bc as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("offline", "per_tanh")
NETS = ("actor", "critic1", "critic2", "actor_old", "critic1_old", "critic2_old")
CFG_KEYS = ("gamma", "tau", "n_step", "twin", "policy_noise", "noise_clip", "update_actor_freq", "max_action", "actor_lr",
            "critic_lr", "alpha")


def load_td3bc(tag: str):
    g = np.load(os.path.join(GOLDEN, f"td3bc_{tag}.npz"))
    E, slots, steps, obs_dim, act_dim, batch, n_updates, seed, prioritized, n_step = (int(x) for x in g["dims"])
    c = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OB.TD3BCConfig(gamma=c["gamma"], tau=c["tau"], n_step=int(c["n_step"]), twin=True, policy_noise=c["policy_noise"],
                         noise_clip=c["noise_clip"], update_actor_freq=int(c["update_actor_freq"]), max_action=c["max_action"],
                         actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], alpha=c["alpha"])
    d = dict(E=E, slots=slots, steps=steps, obs_dim=obs_dim, act_dim=act_dim, batch=batch, n_updates=n_updates, seed=seed,
             prioritized=bool(prioritized), activation="tanh" if c.get("tanh_trunks") else "relu",
             hidden=(tuple(int(x) for x in g["hidden_actor"]), tuple(int(x) for x in g["hidden_critic"])))
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, d, cfg, bstate


def is_weight(g, u: int, prioritized: bool):
    """The PER weights of update u (None for the plain buffer: the reference's batch carries no `weight`)."""
    return g[f"u{u}_is_weight"] if prioritized else None


def engine_from(actor: dict, c1: dict, c2: dict, cfg, activation: str = "relu", cls=None):
    """`TD3BCEngine` (or `cls`, e.g. TD3Engine with a TD3 config) on oracle parameter dicts, embedded by zero padding as
    tests/test_gpu_td3.py::make_engine does."""
    from tianshou_amd import td3 as T
    from tianshou_amd import td3bc as TB
    from tianshou_amd import widths as W

    lists = [list(actor.values()), list(c1.values()), list(c2.values())]
    H = W.engine_hidden([W.layer_widths(t, 1) for t in lists])
    obs_dim, act_dim = actor["w1"].shape[1], actor["ba"].numel()
    bc = cls is None
    keys = CFG_KEYS if bc else CFG_KEYS[:-1]
    config = (TB.TD3BCConfig if bc else T.TD3Config)(**{k: getattr(cfg, k) for k in keys})
    return (TB.TD3BCEngine if bc else cls)(
        obs_dim, act_dim, T.actor_flat_from_torch(lists[0], obs_dim, act_dim, hidden=H),
        T.critic_flat_from_torch(lists[1], obs_dim, act_dim, hidden=H), T.critic_flat_from_torch(lists[2], obs_dim, act_dim, hidden=H),
        config, hidden=H, depth=OS.depth_of(actor), activation=activation)
