"""TEST INFRASTRUCTURE ONLY - torch autograd restatement of the reference's continuous BCQ update and policy forward.

Never imported by the product (`tianshou_amd/`).

Follows:
  update    BCQ._update_with_batch imitation/bcq.py:188-263: VAE step (:202-208), target with the updated VAE, the lagged
            critics and batch.done (:211-237), critic 1 then critic 2 (:239-245), the perturbation step on the updated critic 1
            (:247-253), Polyak (:256).  Every optimizer step is zero_grad, backward, optional clip_grad_norm_ over its own
            module, step (algorithm_base.py:484-500).
  networks  VAE / Perturbation utils/net/continuous.py:378-490; critics ContinuousCritic(Net(concat=True)).
  forward   BCQPolicy.forward bcq.py:91-116, one observation at a time.
The random tensors are inputs, RAW, in the reference's draw order: randn_like(std) [B, L] of the VAE step, randn [B R, L] of the
target's decode, randn [B, L] of the actor loss's decode; the +-0.5 clamp is part of `decode`.
Parameter dicts (torch nn.Linear layout, in the reference's parameter order):
  perturbation  w1, b1, ..., wd, bd, wa, ba          critic  w1, ..., wq, bq
  vae           e_w1, e_b1, ..., wmean, bmean, wls, bls, d_w1, d_b1, ..., d_wa, d_ba
Tensors follow the parameters' dtype, so the same code in float64 is the reference of the kernel edge tests.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_sac as OS

ACT = {"relu": F.relu, "tanh": torch.tanh}
LS_MIN, LS_MAX, Z_CLIP = -4.0, 15.0, 0.5


@dataclass
class CBCQConfig:
    gamma: float = 0.99
    tau: float = 0.005
    lmbda: float = 0.75
    phi: float = 0.05
    max_action: float = 1.0
    num_sampled_action: int = 10
    forward_sampled_times: int = 100
    pert_lr: float = 1e-3
    critic1_lr: float = 1e-3
    critic2_lr: float = 1e-3
    vae_lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    adam_eps: float = 1e-8
    pert_max_grad_norm: float = 0.0          # <= 0: no clip
    critic1_max_grad_norm: float = 0.0
    critic2_max_grad_norm: float = 0.0
    vae_max_grad_norm: float = 0.0
    activation: str = "relu"                 # perturbation net and critics
    vae_activation: str = "relu"
    # Perturbation.forward takes `[0]` of its preprocess net's output (continuous.py:409): of the (logits, state) pair of a
    # `Net`, but the FIRST ROW of the logits of a plain `MLP` (examples/offline/d4rl_bcq.py) -- every row of the batch is then
    # perturbed by the first row's logits
    pert_first_row: bool = False


def _depth(p: dict, prefix: str = "") -> int:
    d = 0
    while f"{prefix}w{d + 1}" in p:
        d += 1
    return d


def _trunk(p, x, fn, prefix=""):
    for i in range(1, _depth(p, prefix) + 1):
        x = fn(F.linear(x, p[f"{prefix}w{i}"], p[f"{prefix}b{i}"]))
    return x


def critic_forward(p, obs, act, cfg: CBCQConfig):
    return F.linear(_trunk(p, torch.cat([obs, act], 1), ACT[cfg.activation]), p["wq"], p["bq"])


def pert_logits(p, obs, act, cfg: CBCQConfig):
    return F.linear(_trunk(p, torch.cat([obs, act], 1), ACT[cfg.activation]), p["wa"], p["ba"])


def perturb(logits, sampled, cfg: CBCQConfig):
    """continuous.py:409-412 behind the preprocess net."""
    if cfg.pert_first_row:
        logits = logits[0]
    noise = cfg.phi * cfg.max_action * torch.tanh(logits)
    return (noise + sampled).clamp(-cfg.max_action, cfg.max_action)


def pert_forward(p, obs, act, cfg: CBCQConfig):
    return perturb(pert_logits(p, obs, act, cfg), act, cfg)


def encode(p, obs, act, cfg: CBCQConfig):
    """-> (mean, raw log_std)"""
    h = _trunk(p, torch.cat([obs, act], 1), ACT[cfg.vae_activation], "e_")
    return F.linear(h, p["wmean"], p["bmean"]), F.linear(h, p["wls"], p["bls"])


def latent(mean, raw_log_std, eps):
    """continuous.py:466-470 -> (z, std)"""
    std = torch.exp(raw_log_std.clamp(LS_MIN, LS_MAX))
    return mean + std * eps, std


def kl_term(mean, std):
    """bcq.py:205"""
    return (-torch.log(std) + (std.pow(2) + mean.pow(2) - 1) / 2).mean()


def dec_logits(p, obs, z, cfg: CBCQConfig):
    h = _trunk(p, torch.cat([obs, z], 1), ACT[cfg.vae_activation], "d_")
    return F.linear(h, p["d_wa"], p["d_ba"])


def decode(p, obs, z, cfg: CBCQConfig, raw: bool = False):
    """continuous.py:475-490; raw=True: z is a raw normal draw and is clamped to +-0.5 here, as decode(state) does."""
    if raw:
        z = z.clamp(-Z_CLIP, Z_CLIP)
    return cfg.max_action * torch.tanh(dec_logits(p, obs, z, cfg))


def target_value(q1, q2, rew, done, R: int, cfg: CBCQConfig):
    """bcq.py:223-237 from the lagged critics' outputs [B R] -> [B]"""
    tq = cfg.lmbda * torch.min(q1, q2) + (1 - cfg.lmbda) * torch.max(q1, q2)
    tq = tq.reshape(-1, R).max(dim=1)[0]
    return (rew + torch.logical_not(done.bool()) * cfg.gamma * tq).to(q1.dtype)


@dataclass
class CBCQState:
    pert: dict
    critic1: dict
    critic2: dict
    vae: dict
    pert_old: dict
    critic1_old: dict
    critic2_old: dict
    opt_pert: OS.Adam
    opt_c1: OS.Adam
    opt_c2: OS.Adam
    opt_vae: OS.Adam

    @classmethod
    def create(cls, pert, critic1, critic2, vae, cfg: CBCQConfig, dtype=torch.float32):
        c = lambda d: {k: v.detach().clone().to(dtype) for k, v in d.items()}  # noqa: E731
        mk = lambda lr: OS.Adam(lr, tuple(cfg.betas), cfg.adam_eps)           # noqa: E731
        return cls(c(pert), c(critic1), c(critic2), c(vae), c(pert), c(critic1), c(critic2), mk(cfg.pert_lr), mk(cfg.critic1_lr),
                   mk(cfg.critic2_lr), mk(cfg.vae_lr))


def clip_coef(grads: dict, max_norm: float) -> tuple[float, float]:
    """clip_grad_norm_ (torch/nn/utils/clip_grad.py): (total norm, clamp(max_norm / (norm + 1e-6), max=1))."""
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads.values()]))
    return float(norm), float(torch.clamp(max_norm / (norm + 1e-6), max=1.0))


def _step(params: dict, grads: dict, opt: OS.Adam, max_norm: float, lr: float) -> dict:
    opt.lr = lr
    if max_norm > 0:
        coef = clip_coef(grads, max_norm)[1]
        grads = {n: v * coef for n, v in grads.items()}
    return opt.apply(params, grads)


def _leaf(d):
    return {k: v.clone().requires_grad_(True) for k, v in d.items()}


def update_with_batch(st: CBCQState, cfg: CBCQConfig, obs, act, rew, done, obs_next, eps1, eps2, eps3, collect=None,
                      step: bool = True):
    """bcq.py:188-263 -> dict(actor_loss, critic1_loss, critic2_loss, vae_loss, target).  `step=False`: gradients only (every
    phase then sees the parameters as they were)."""
    dt = next(iter(st.pert.values())).dtype
    t = lambda x: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dt)  # noqa: E731
    obs, act, rew, obs_next, done = t(obs), t(act), t(rew).flatten(), t(obs_next), t(done).flatten()
    eps1, eps2, eps3 = t(eps1), t(eps2), t(eps3)
    R = cfg.num_sampled_action
    out = {}
    # 1. VAE
    p = _leaf(st.vae)
    mean, raw = encode(p, obs, act, cfg)
    z, std = latent(mean, raw, eps1)
    recon = decode(p, obs, z, cfg)
    vae_loss = F.mse_loss(act, recon) + kl_term(mean, std) / 2
    g = OS._grads(vae_loss, p)
    if collect is not None:
        collect["vae_grads"] = g
    if step:
        st.vae = _step(st.vae, g, st.opt_vae, cfg.vae_max_grad_norm, cfg.vae_lr)
    out["vae_loss"] = float(vae_loss.detach())
    # 2. target
    with torch.no_grad():
        on = obs_next.repeat_interleave(R, dim=0)
        an = decode(st.vae, on, eps2, cfg, raw=True)
        target = target_value(critic_forward(st.critic1_old, on, an, cfg).flatten(), critic_forward(st.critic2_old, on, an, cfg).flatten(),
                              rew, done, R, cfg)
    out["target"] = target
    # 3. critics
    gs, ls = [], []
    for name in ("critic1", "critic2"):
        p = _leaf(getattr(st, name))
        loss = F.mse_loss(critic_forward(p, obs, act, cfg).flatten(), target)
        gs.append(OS._grads(loss, p))
        ls.append(loss)
    for k, (name, opt) in enumerate((("critic1", st.opt_c1), ("critic2", st.opt_c2))):
        out[name + "_loss"] = float(ls[k].detach())
        if collect is not None:
            collect[name + "_grads"] = gs[k]
        if step:
            setattr(st, name, _step(getattr(st, name), gs[k], opt, getattr(cfg, name + "_max_grad_norm"), getattr(cfg, name + "_lr")))
    # 4. perturbation net on the updated critic 1 and VAE
    p = _leaf(st.pert)
    with torch.no_grad():
        sampled = decode(st.vae, obs, eps3, cfg, raw=True)
    actor_loss = -critic_forward(st.critic1, obs, pert_forward(p, obs, sampled, cfg), cfg).mean()
    g = OS._grads(actor_loss, p)
    if collect is not None:
        collect["pert_grads"] = g
    if step:
        st.pert = _step(st.pert, g, st.opt_pert, cfg.pert_max_grad_norm, cfg.pert_lr)
    out["actor_loss"] = float(actor_loss.detach())
    # 5. Polyak
    if step:
        for old, new in ((st.pert_old, st.pert), (st.critic1_old, st.critic1), (st.critic2_old, st.critic2)):
            for k in old:
                old[k] = cfg.tau * new[k] + (1 - cfg.tau) * old[k]
    return out


def policy_forward(pert, critic1, vae, cfg: CBCQConfig, obs, noise):
    """bcq.py:103-114 with the draws noise [N, T, L] -> (act [N, A], idx [N], q [N, T], candidates [N, T, A])"""
    dt = next(iter(pert.values())).dtype
    obs, noise = torch.as_tensor(obs).to(dt), torch.as_tensor(noise).to(dt)
    acts, idxs, qs, cands = [], [], [], []
    with torch.no_grad():
        for n in range(obs.shape[0]):
            o = obs[n].reshape(1, -1).repeat(noise.shape[1], 1)
            a = pert_forward(pert, o, decode(vae, o, noise[n], cfg, raw=True), cfg)
            q1 = critic_forward(critic1, o, a, cfg)
            i = int(q1.argmax(0))
            acts.append(a[i]); idxs.append(i); qs.append(q1.flatten()); cands.append(a)
    return torch.stack(acts), torch.tensor(idxs), torch.stack(qs), torch.stack(cands)


# ---- parameter construction (nn.Linear default init, one fixed order) -------------------------------------------------
def _mlp(in_dim: int, sizes, out_dim: int, names_prefix: str, head: str, g: dict):
    k = in_dim
    for i, h in enumerate(sizes, 1):
        lin = torch.nn.Linear(k, h)
        g[f"{names_prefix}w{i}"], g[f"{names_prefix}b{i}"] = lin.weight.detach().clone(), lin.bias.detach().clone()
        k = h
    if head:
        lin = torch.nn.Linear(k, out_dim)
        g[f"{names_prefix}w{head}"], g[f"{names_prefix}b{head}"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return k


def init_params(obs_dim: int, act_dim: int, latent_dim: int, seed: int, hidden=(256, 256), vae_hidden=(512, 512)):
    """-> (pert, critic1, critic2, vae) in the construction order of examples/offline/d4rl_bcq.py:102-148: perturbation net,
    the two critic trunks, the two critic heads, encoder, decoder, then VAE's mean / log_std heads."""
    torch.manual_seed(seed)
    pert, c1, c2, vae_e, vae_d, heads = {}, {}, {}, {}, {}, {}
    _mlp(obs_dim + act_dim, hidden, act_dim, "", "a", pert)
    _mlp(obs_dim + act_dim, hidden, 1, "", "", c1)
    _mlp(obs_dim + act_dim, hidden, 1, "", "", c2)
    for c in (c1, c2):
        lin = torch.nn.Linear(hidden[-1], 1)
        c["wq"], c["bq"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    k = _mlp(obs_dim + act_dim, vae_hidden, 0, "e_", "", vae_e)
    _mlp(obs_dim + latent_dim, vae_hidden, act_dim, "d_", "a", vae_d)
    for name in ("mean", "ls"):
        lin = torch.nn.Linear(k, latent_dim)
        heads[f"w{name}"], heads[f"b{name}"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return pert, c1, c2, {**vae_e, **heads, **vae_d}


def flatten(p: dict) -> torch.Tensor:
    return torch.cat([v.reshape(-1) for v in p.values()])
