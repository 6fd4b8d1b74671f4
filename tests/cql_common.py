"""Shared by the continuous-CQL tests: the fixtures of tools/gen_golden_cql.py (tests/golden/cql_calibrated.npz, cql_plain.npz),
the replay of one recorded update and the engine built from oracle parameters."""
import os

import numpy as np

from oracle import oracle_sac as OS
from tests import oracle_cql as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("calibrated", "plain")
NETS = ("actor", "critic1", "critic2", "critic1_old", "critic2_old")
STATS = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss", "cql_alpha", "cql_alpha_loss")
SAC_KEYS = ("gamma", "tau", "alpha", "auto_alpha", "target_entropy", "log_alpha0", "actor_lr", "critic_lr", "alpha_lr")
CQL_KEYS = ("cql_alpha_lr", "cql_weight", "temperature", "with_lagrange", "lagrange_threshold", "num_repeat_actions", "alpha_min",
            "alpha_max", "max_grad_norm", "calibrated")
BOOLS, INTS = ("auto_alpha", "with_lagrange", "calibrated"), ("num_repeat_actions",)


def cfg_kwargs(c: dict) -> dict:
    kw = {k: c[k] for k in SAC_KEYS + CQL_KEYS}
    for k in BOOLS:
        kw[k] = bool(kw[k])
    for k in INTS:
        kw[k] = int(kw[k])
    return kw


def load_cql(tag: str):
    g = np.load(os.path.join(GOLDEN, f"cql_{tag}.npz"))
    E, slots, steps, obs_dim, act_dim, batch, n_updates, seed, R = (int(x) for x in g["dims"])
    c = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OC.CQLConfig(**cfg_kwargs(c))
    d = dict(E=E, slots=slots, steps=steps, obs_dim=obs_dim, act_dim=act_dim, batch=batch, n_updates=n_updates, seed=seed, R=R,
             activation="tanh" if c.get("tanh_trunks") else "relu", min_action=c["min_action"], max_action=c["max_action"],
             hidden=(tuple(int(x) for x in g["hidden_actor"]), tuple(int(x) for x in g["hidden_critic"])))
    return g, d, cfg


def batch_of(g, u: int, calibrated: bool) -> dict:
    """The arguments of update u in `update_with_batch` order (oracle and engine take the same names)."""
    idx = g[f"u{u}_indices"]
    return dict(obs=g["obs"][idx], act=g["act"][idx], rew=g["rew"][idx].astype(np.float32), done=g["done"][idx].astype(np.float32),
                obs_next=g["obs_next"][idx], noise_actor=g[f"u{u}_noise_actor"], noise_next=g[f"u{u}_noise_next"],
                random_act=g[f"u{u}_random_act"], noise_rep_cur=g[f"u{u}_noise_rep_cur"], noise_rep_next=g[f"u{u}_noise_rep_next"],
                calib=g["calibration_returns"][idx].astype(np.float32) if calibrated else None)


def stats_vector(out: dict) -> np.ndarray:
    return np.array([np.nan if out[k] is None else out[k] for k in STATS], np.float64)


def engine_from(actor: dict, c1: dict, c2: dict, cfg, activation: str = "relu", cls=None, **over):
    """`CQLEngine` (or `cls`, e.g. SACEngine with SAC's config) on oracle parameter dicts, embedded by zero padding as
    tests/test_gpu_sac.py does."""
    from tianshou_amd import cql as Q
    from tianshou_amd import sac as S
    from tianshou_amd import widths as W

    lists = [list(actor.values()), list(c1.values()), list(c2.values())]
    H = W.engine_hidden([W.layer_widths(lists[0], 2), W.layer_widths(lists[1], 1), W.layer_widths(lists[2], 1)])
    obs_dim, act_dim = actor["w1"].shape[1], actor["bmu"].numel()
    kw = {k: getattr(cfg, k) for k in SAC_KEYS}
    if cls is None:
        kw.update({k: getattr(cfg, k) for k in CQL_KEYS})
    kw.update(over)
    config = (Q.CQLConfig if cls is None else S.SACConfig)(**kw)
    return (Q.CQLEngine if cls is None else cls)(
        obs_dim, act_dim, S.actor_flat_from_torch(lists[0], obs_dim, act_dim, hidden=H),
        S.critic_flat_from_torch(lists[1], obs_dim, act_dim, hidden=H), S.critic_flat_from_torch(lists[2], obs_dim, act_dim, hidden=H),
        config, hidden=H, depth=OS.depth_of(actor), activation=activation)
