"""Shared by the continuous-BCQ tests: the fixtures of tools/gen_golden_cbcq.py (tests/golden/cbcq_d4rl.npz, cbcq_odd.npz), the
replay of one recorded update and the engine built from oracle parameters."""
import os

import numpy as np
import torch

from tests import oracle_cbcq as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("d4rl", "odd")
NETS = ("pert", "critic1", "critic2", "vae")
LAGGED = ("pert_old", "critic1_old", "critic2_old")
STATS = ("actor_loss", "critic1_loss", "critic2_loss", "vae_loss")
OPTS = {"pert": "opt_pert", "critic1": "opt_c1", "critic2": "opt_c2", "vae": "opt_vae"}
CFG_KEYS = ("gamma", "tau", "lmbda", "phi", "max_action", "num_sampled_action", "pert_lr", "critic1_lr", "critic2_lr", "vae_lr",
            "critic1_max_grad_norm", "critic2_max_grad_norm", "pert_first_row")
ENGINE_KEYS = CFG_KEYS + ("pert_max_grad_norm", "vae_max_grad_norm", "forward_sampled_times")


def load_cbcq(tag: str):
    g = np.load(os.path.join(GOLDEN, f"cbcq_{tag}.npz"))
    E, slots, steps, obs_dim, act_dim, latent_dim, batch, n_updates, seed, R = (int(x) for x in g["dims"])
    c = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    kw = {k: c[k] for k in CFG_KEYS}
    kw["num_sampled_action"], kw["pert_first_row"] = int(kw["num_sampled_action"]), bool(kw["pert_first_row"])
    cfg = OB.CBCQConfig(activation="tanh" if c["tanh_trunks"] else "relu", **kw)
    d = dict(E=E, slots=slots, steps=steps, obs_dim=obs_dim, act_dim=act_dim, latent_dim=latent_dim, batch=batch,
             n_updates=n_updates, seed=seed, R=R, hidden=tuple(int(x) for x in g["hidden"]),
             vae_hidden=tuple(int(x) for x in g["vae_hidden"]))
    return g, d, cfg


def init_of(d: dict):
    return OB.init_params(d["obs_dim"], d["act_dim"], d["latent_dim"], d["seed"], d["hidden"], d["vae_hidden"])


def batch_of(g, u: int) -> dict:
    """The arguments of update u in `update_with_batch` order (oracle and engine take the same names)."""
    idx = g[f"u{u}_indices"]
    return dict(obs=g["obs"][idx], act=g["act"][idx], rew=g["rew"][idx].astype(np.float32), done=g["done"][idx].astype(np.float32),
                obs_next=g["obs_next"][idx], eps1=g[f"u{u}_eps1"], eps2=g[f"u{u}_eps2"], eps3=g[f"u{u}_eps3"])


def stats_vector(out: dict) -> np.ndarray:
    return np.array([out[k] for k in STATS], np.float64)


def random_batch(seed: int, B: int, R: int, obs_dim: int, act_dim: int, latent_dim: int, max_action: float = 1.0) -> dict:
    r = np.random.default_rng(seed)
    f = lambda *s: r.normal(size=s).astype(np.float32)  # noqa: E731
    return dict(obs=f(B, obs_dim), act=r.uniform(-max_action, max_action, (B, act_dim)).astype(np.float32), rew=f(B),
                done=(r.random(B) < 0.2).astype(np.float32), obs_next=f(B, obs_dim), eps1=f(B, latent_dim), eps2=f(B * R, latent_dim),
                eps3=f(B, latent_dim))


def vae_lists(vae: dict):
    """(enc, dec) tensor lists of an oracle VAE dict in `tianshou_amd.cbcq.vae_flat_from_torch`'s order."""
    enc = [v for k, v in vae.items() if k.startswith("e_")] + [vae["wmean"], vae["bmean"], vae["wls"], vae["bls"]]
    dec = [v for k, v in vae.items() if k.startswith("d_")]
    return enc, dec


def engine_from(pert: dict, c1: dict, c2: dict, vae: dict, cfg, **over):
    """`CBCQEngine` on oracle parameter dicts (widths embedded by zero padding)."""
    from tianshou_amd import cbcq as Q
    from tianshou_amd import widths as W

    enc, dec = vae_lists(vae)
    lists = [list(pert.values()), list(c1.values()), list(c2.values())]
    H = W.engine_hidden([W.layer_widths(t, 1) for t in lists])
    HV = W.engine_hidden([W.layer_widths(enc, 2), W.layer_widths(dec, 1)])
    act_dim, latent_dim = pert["ba"].numel(), vae["bmean"].numel()
    obs_dim = pert["w1"].shape[1] - act_dim
    kw = {k: getattr(cfg, k) for k in ENGINE_KEYS}
    kw.update(over)
    return Q.CBCQEngine(obs_dim, act_dim, latent_dim, Q.pert_flat_from_torch(lists[0], obs_dim, act_dim, hidden=H),
                        Q.critic_flat_from_torch(lists[1], obs_dim, act_dim, hidden=H),
                        Q.critic_flat_from_torch(lists[2], obs_dim, act_dim, hidden=H),
                        Q.vae_flat_from_torch(enc, dec, obs_dim, act_dim, latent_dim, hidden=HV), Q.CBCQConfig(**kw), hidden=H,
                        depth=len(lists[0]) // 2 - 1, activation=cfg.activation, vae_hidden=HV, vae_depth=len(dec) // 2 - 1,
                        vae_activation=cfg.vae_activation)


def engine_net(eng, name: str) -> torch.Tensor:
    """A network (or lagged network / Adam moment vector: `pert_old`, `vae_m`, ...) of the engine as the flat vector of the
    oracle's / the reference's parameter order, on the host."""
    from tianshou_amd import cbcq as Q

    flat = getattr(eng, name).detach().cpu()
    kind = name.split("_")[0]
    if kind == "vae":
        enc, dec = Q.vae_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.latent_dim, eng.vae_hidden, eng.vae_depth)
        ts = enc + dec
    elif kind == "pert":
        ts = Q.pert_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.hidden, eng.depth)
    else:
        ts = Q.critic_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.hidden, depth=eng.depth)
    return torch.cat([t.reshape(-1) for t in ts])
