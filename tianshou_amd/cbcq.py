"""Continuous BCQ learn() path and policy forward on the MI355X engine.

Mirrors, on device tensors:
    BCQ._update_with_batch        tianshou/algorithm/imitation/bcq.py:188-263 (arXiv 1812.02900)
    BCQPolicy.forward             bcq.py:91-116 (all observations in one call instead of a Python loop)
    VAE / Perturbation            tianshou/utils/net/continuous.py:378-490
Networks of examples/offline/d4rl_bcq.py: a perturbation net and twin critics on concat(obs, act) (one trunk), a conditional VAE
(a second trunk).  The flat layouts are documented with ts_cbcq_layout in include/tsengine.h; the critics' is SAC's.  The three
normal draws of an update are arguments, RAW: the +-0.5 clamp of `decode` happens in the engine.
`pert_first_row`: Perturbation.forward takes `[0]` of its preprocess net's output -- the (logits, state) pair of a `Net`, but the
first ROW of the logits of a plain `MLP` (the examples' choice); with the latter every row of a batch is perturbed by the first
row's logits, and the engine does the same when the switch is on.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from . import widths as W
from .sac import HID, MLPTrunk, _dense, _l1, critic_flat_from_torch, critic_flat_to_torch  # noqa: F401

# TS_CBCQ_HP_* / TS_CBCQ_ST_* (include/tsengine.h)
CBCQ_HP = ("pert_lr", "critic1_lr", "critic2_lr", "vae_lr", "beta1", "beta2", "adam_eps", "tau", "gamma", "lmbda", "phi",
           "max_action", "pert_max_grad_norm", "critic1_max_grad_norm", "critic2_max_grad_norm", "vae_max_grad_norm",
           "split_decode", "pert_first_row")
CBCQ_ST = ("pert", "pert_m", "pert_v", "pert_old", "critic1", "critic1_m", "critic1_v", "critic1_old", "critic2", "critic2_m",
           "critic2_v", "critic2_old", "vae", "vae_m", "vae_v")
NETS = ("pert", "critic1", "critic2", "vae")


def pad32(n: int) -> int:
    return (int(n) + 31) // 32 * 32


@dataclass
class CBCQConfig:
    """Hyper-parameters of the reference BCQ (bcq.py:125-186) + the four Adam factories; a `*_max_grad_norm` <= 0 = no clip."""

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
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    pert_max_grad_norm: float = 0.0
    critic1_max_grad_norm: float = 0.0
    critic2_max_grad_norm: float = 0.0
    vae_max_grad_norm: float = 0.0
    pert_first_row: bool = False
    split_decode: bool = False           # the decoder's target rows and actor-loss rows as two passes (comparison only)

    def to_c(self, lr_scale: float = 1.0):
        v = {n: float(getattr(self, n)) for n in CBCQ_HP if n not in ("beta1", "beta2")}
        v["beta1"], v["beta2"] = float(self.betas[0]), float(self.betas[1])
        for n in ("pert_lr", "critic1_lr", "critic2_lr", "vae_lr"):
            v[n] *= lr_scale if v[n] >= 0 else 1.0
        return (C.c_double * len(CBCQ_HP))(*[v[n] for n in CBCQ_HP])


def layout(obs_dim: int, act_dim: int, latent_dim: int, trunk: MLPTrunk, vae_trunk: MLPTrunk) -> dict[str, int]:
    """ts_cbcq_layout: widths, element counts and head offsets of the four flat vectors."""
    out = (C.c_int64 * 12)()
    _lib.check(_lib.load().ts_cbcq_layout(_lib.i64(obs_dim), _lib.i64(act_dim), _lib.i64(latent_dim), C.byref(trunk), C.byref(vae_trunk),
                                          out))
    keys = ["kc", "kd", "lp", "pert_count", "critic_count", "encoder_count", "decoder_count", "vae_count", "critic_head",
            "encoder_head", "decoder", "decoder_head"]
    return dict(zip(keys, (int(v) for v in out)))


def _offsets(k: int, H: int, depth: int, cols: int) -> list[int]:
    o = [0, (k + 1) * H]
    for _ in range(1, depth):
        o.append(o[-1] + (H + 1) * H)
    o.append(o[-1] + (H + 1) * cols)
    return o


def mlp_flat_from_torch(t: list[torch.Tensor], in_dim: int, hidden: int, cols: int, head_cols: list[int]) -> torch.Tensor:
    """[w1, b1, ..., wd, bd, head weights / biases ...] (torch nn.Linear layout; also valid for Adam moments) -> the flat
    vector of an engine MLP whose head block is `cols` wide, head i in columns [head_cols[i], head_cols[i] + its outputs).
    Unequal widths / widths that are no multiple of 32 are embedded by zero padding (`tianshou_amd.widths`).  Host tensor."""
    nh = len(head_cols)
    d = W.depth_of(t, nh)
    H = int(hidden)
    t = W.pad_layers(t, H, nh)
    k = pad32(in_dim)
    head = torch.zeros((H + 1, cols), dtype=torch.float32)
    for i, c0 in enumerate(head_cols):
        w, b = t[2 * d + 2 * i].detach().float().cpu(), t[2 * d + 2 * i + 1].detach().float().cpu()
        head[:H, c0:c0 + w.shape[0]] = w.t()
        head[H, c0:c0 + w.shape[0]] = b
    return torch.cat([_l1(t[0], t[1], k)] + [_dense(t[2 * i], t[2 * i + 1]) for i in range(1, d)] + [head.reshape(-1)])


def mlp_flat_to_torch(flat: torch.Tensor, in_dim: int, hidden: int, depth: int, cols: int, heads: list[tuple[int, int]],
                      sizes=None) -> list[torch.Tensor]:
    """The inverse; heads = [(first column, outputs), ...]; sizes = the torch network's own hidden widths."""
    H, k = int(hidden), pad32(in_dim)
    offs = _offsets(k, H, depth, cols)
    f = flat.detach()
    l1 = f[: offs[1]].reshape(k + 1, H)
    out = [l1[:in_dim].t().contiguous(), l1[k].clone()]
    for i in range(1, depth):
        li = f[offs[i]: offs[i + 1]].reshape(H + 1, H)
        out += [li[:H].t().contiguous(), li[H].clone()]
    hd = f[offs[depth]: offs[depth + 1]].reshape(H + 1, cols)
    for c0, n in heads:
        out += [hd[:H, c0:c0 + n].t().contiguous(), hd[H, c0:c0 + n].clone()]
    return W.unpad_layers(out, sizes) if sizes is not None else out


def pert_flat_from_torch(t, obs_dim: int, act_dim: int, device="cuda", hidden: int | None = None) -> torch.Tensor:
    """[w1, b1, ..., wd, bd, wa, ba] of the perturbation net's MLP(obs + act -> hidden -> act)."""
    H = int(hidden or W.engine_hidden([W.layer_widths(t, 1)]))
    return mlp_flat_from_torch(t, obs_dim + act_dim, H, 32, [0]).to(device).contiguous()


def pert_flat_to_torch(flat, obs_dim: int, act_dim: int, hidden: int, depth: int, sizes=None) -> list[torch.Tensor]:
    return mlp_flat_to_torch(flat, obs_dim + act_dim, hidden, depth, 32, [(0, act_dim)], sizes)


def vae_flat_from_torch(enc, dec, obs_dim: int, act_dim: int, latent_dim: int, device="cuda", hidden: int | None = None) -> torch.Tensor:
    """enc = [w1, b1, ..., wd, bd, wmean, bmean, wlog_std, blog_std], dec = [w1, b1, ..., wd, bd, wa, ba] -> encoder | decoder."""
    H = int(hidden or W.engine_hidden([W.layer_widths(enc, 2), W.layer_widths(dec, 1)]))
    lp = pad32(latent_dim)
    return torch.cat([mlp_flat_from_torch(enc, obs_dim + act_dim, H, 2 * lp, [0, lp]),
                      mlp_flat_from_torch(dec, obs_dim + latent_dim, H, 32, [0])]).to(device).contiguous()


def vae_flat_to_torch(flat, obs_dim: int, act_dim: int, latent_dim: int, hidden: int, depth: int, enc_sizes=None, dec_sizes=None):
    """-> (enc tensors, dec tensors) in `vae_flat_from_torch`'s order."""
    lp = pad32(latent_dim)
    n_enc = _offsets(pad32(obs_dim + act_dim), int(hidden), depth, 2 * lp)[-1]
    return (mlp_flat_to_torch(flat[:n_enc], obs_dim + act_dim, hidden, depth, 2 * lp, [(0, latent_dim), (lp, latent_dim)], enc_sizes),
            mlp_flat_to_torch(flat[n_enc:], obs_dim + latent_dim, hidden, depth, 32, [(0, act_dim)], dec_sizes))


class CBCQEngine:
    """State of one continuous-BCQ learner on one GPU: four networks, three lagged copies, four Adam states."""

    def __init__(self, obs_dim: int, act_dim: int, latent_dim: int, pert: torch.Tensor, critic1: torch.Tensor, critic2: torch.Tensor,
                 vae: torch.Tensor, cfg: CBCQConfig, hidden: int = HID, depth: int = 2, activation: str = "relu",
                 vae_hidden: int = 512, vae_depth: int = 2, vae_activation: str = "relu"):
        if not pert.is_cuda:
            raise RuntimeError("CBCQEngine needs parameters on an MI355X (no CPU fallback)")
        self.obs_dim, self.act_dim, self.latent_dim, self.cfg, self.device = int(obs_dim), int(act_dim), int(latent_dim), cfg, pert.device
        self.hidden, self.depth, self.activation = int(hidden), int(depth), activation
        self.vae_hidden, self.vae_depth, self.vae_activation = int(vae_hidden), int(vae_depth), vae_activation
        self._trunk = MLPTrunk(hidden, depth, activation)
        self._vae_trunk = MLPTrunk(vae_hidden, vae_depth, vae_activation)
        self.lay = layout(obs_dim, act_dim, latent_dim, self._trunk, self._vae_trunk)
        if pert.numel() != self.lay["pert_count"] or critic1.numel() != self.lay["critic_count"] \
                or critic2.numel() != self.lay["critic_count"] or vae.numel() != self.lay["vae_count"]:
            raise ValueError("flat parameter vectors do not match ts_cbcq_layout")
        cl = lambda t: t.detach().float().contiguous().clone()   # noqa: E731
        self.pert, self.critic1, self.critic2, self.vae = cl(pert), cl(critic1), cl(critic2), cl(vae)
        self.pert_old, self.critic1_old, self.critic2_old = cl(pert), cl(critic1), cl(critic2)
        for n in NETS:
            setattr(self, n + "_m", torch.zeros_like(getattr(self, n)))
            setattr(self, n + "_v", torch.zeros_like(getattr(self, n)))
        self.adam_step = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _f32(self, x, shape=None) -> torch.Tensor:
        t = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
        return t if shape is None else t.reshape(shape)

    def _state_c(self):
        return (C.c_void_p * len(CBCQ_ST))(*[getattr(self, n).data_ptr() for n in CBCQ_ST])

    def grads_size(self) -> int:
        return self.lay["vae_count"] + 2 * self.lay["critic_count"] + self.lay["pert_count"]

    def update_with_batch(self, obs, act, rew, done, obs_next, eps1, eps2, eps3, grads_out: torch.Tensor | None = None,
                          target_out: torch.Tensor | None = None, lr_scale: float = 1.0) -> torch.Tensor:
        """-> stats float32[4] (device) = {actor_loss, critic1_loss, critic2_loss, vae_loss}.  eps1 [B, L], eps2 [B R, L],
        eps3 [B, L]: the raw normal draws in the reference's order.  grads_out (nullable): [vae | critic1 | critic2 | pert]
        before clipping.  The hyper-parameters are read from `cfg` at every call."""
        cfg = self.cfg
        obs, act, obs_next = self._f32(obs), self._f32(act), self._f32(obs_next)
        b, r, ld = obs.shape[0], int(cfg.num_sampled_action), self.latent_dim
        if obs.shape != (b, self.obs_dim) or obs_next.shape != obs.shape or act.shape != (b, self.act_dim):
            raise ValueError("obs / act / obs_next shapes do not match the engine")
        rew, done = self._f32(rew, (b,)), self._f32(done, (b,))
        eps1, eps2, eps3 = self._f32(eps1, (b, ld)), self._f32(eps2, (b * max(r, 0), ld)), self._f32(eps3, (b, ld))
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        st = self._state_c()
        _lib.check(_lib.load().ts_cbcq_update(
            self._ws.handle, st, _lib.i64(self.adam_step + 1), _lib.ptr(obs), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done),
            _lib.ptr(obs_next), _lib.ptr(eps1), _lib.ptr(eps2), _lib.ptr(eps3), _lib.i64(b), _lib.i64(r), _lib.i64(self.obs_dim),
            _lib.i64(self.act_dim), _lib.i64(ld), C.byref(self._trunk), C.byref(self._vae_trunk), cfg.to_c(lr_scale), _lib.ptr(stats),
            _lib.ptr(target_out), _lib.ptr(grads_out), _lib.current_stream(self.device)))
        self.adam_step += 1                              # (after the call: a refused argument leaves the counter alone)
        return stats

    def policy_forward(self, obs, noise, return_all: bool = False):
        """obs [N, obs_dim], noise [N, T, L] raw normal draws -> act [N, act_dim]; return_all: (act, idx int64[N], q [N],
        candidates [N, T, act_dim])."""
        obs, noise = self._f32(obs), self._f32(noise)
        n, t = obs.shape[0], noise.shape[1]
        if obs.shape != (n, self.obs_dim) or noise.shape != (n, t, self.latent_dim):
            raise ValueError("policy_forward: obs [N, obs_dim], noise [N, T, latent_dim]")
        act = torch.empty((n, self.act_dim), dtype=torch.float32, device=self.device)
        idx = q = cand = None
        if return_all:
            idx = torch.empty(n, dtype=torch.int64, device=self.device)
            q = torch.empty(n, dtype=torch.float32, device=self.device)
            cand = torch.empty((n, t, self.act_dim), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_cbcq_policy_forward(
            self._ws.handle, _lib.ptr(self.pert), _lib.ptr(self.critic1), _lib.ptr(self.vae), _lib.ptr(obs), _lib.ptr(noise),
            _lib.i64(n), _lib.i64(t), _lib.i64(self.obs_dim), _lib.i64(self.act_dim), _lib.i64(self.latent_dim), C.byref(self._trunk),
            C.byref(self._vae_trunk), _lib.f64(self.cfg.phi), _lib.f64(self.cfg.max_action), C.c_int32(int(self.cfg.pert_first_row)),
            _lib.ptr(act), _lib.ptr(idx), _lib.ptr(q), _lib.ptr(cand), _lib.current_stream(self.device)))
        return (act, idx, q, cand) if return_all else act


def _dense32(*ts):
    return [None if t is None else t.to(torch.float32).contiguous() for t in ts]


def cbcq_latent(mean, log_std, eps, dz):
    """ts_cbcq_latent on dense [B, L] device arrays -> (z, kl (one float, device), d_mean, d_log_std)."""
    mean, log_std, eps, dz = _dense32(mean, log_std, eps, dz)
    b, ld = mean.shape
    z, dm, dl = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    kl = torch.empty(1, dtype=torch.float32, device=mean.device)
    ws = _lib.default_workspace(mean.device.index or 0)
    _lib.check(_lib.load().ts_cbcq_latent(ws.handle, _lib.ptr(mean), _lib.ptr(log_std), _lib.ptr(eps), _lib.ptr(dz), _lib.i64(b),
                                          _lib.i64(ld), _lib.ptr(z), _lib.ptr(kl), _lib.ptr(dm), _lib.ptr(dl),
                                          _lib.current_stream(mean.device)))
    return z, kl, dm, dl


def cbcq_recon(logits, act, max_action: float):
    """ts_cbcq_recon on dense [B, A] device arrays -> (recon, mse (one float, device), d_logits)."""
    logits, act = _dense32(logits, act)
    b, a = logits.shape
    recon, dl = torch.empty_like(logits), torch.empty_like(logits)
    mse = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = _lib.default_workspace(logits.device.index or 0)
    _lib.check(_lib.load().ts_cbcq_recon(ws.handle, _lib.ptr(logits), _lib.ptr(act), _lib.i64(b), _lib.i64(a), _lib.f64(max_action),
                                         _lib.ptr(recon), _lib.ptr(mse), _lib.ptr(dl), _lib.current_stream(logits.device)))
    return recon, mse, dl


def cbcq_target(q1, q2, rew, done, num_sampled_action: int, gamma: float, lmbda: float):
    """ts_cbcq_target: q1 / q2 [B R], rew / done [B] -> target [B]."""
    q1, q2, rew, done = _dense32(q1, q2, rew, done)
    b, r = rew.numel(), int(num_sampled_action)
    if q1.numel() != b * r or q2.numel() != b * r or done.numel() != b:
        raise ValueError("cbcq_target: q1 / q2 [B R], rew / done [B]")
    out = torch.empty(b, dtype=torch.float32, device=q1.device)
    ws = _lib.default_workspace(q1.device.index or 0)
    _lib.check(_lib.load().ts_cbcq_target(ws.handle, _lib.ptr(q1), _lib.ptr(q2), _lib.ptr(rew), _lib.ptr(done), _lib.i64(b), _lib.i64(r),
                                          _lib.f64(gamma), _lib.f64(lmbda), _lib.ptr(out), _lib.current_stream(q1.device)))
    return out


def cbcq_perturb(logits, sampled, dq_da, phi: float, max_action: float):
    """ts_cbcq_perturb on dense [B, A] device arrays (each row perturbed by its own logits) -> (perturbed, d_logits)."""
    logits, sampled, dq_da = _dense32(logits, sampled, dq_da)
    b, a = logits.shape
    out, dl = torch.empty_like(logits), torch.empty_like(logits)
    ws = _lib.default_workspace(logits.device.index or 0)
    _lib.check(_lib.load().ts_cbcq_perturb(ws.handle, _lib.ptr(logits), _lib.ptr(sampled), _lib.ptr(dq_da), _lib.i64(b), _lib.i64(a),
                                           _lib.f64(phi), _lib.f64(max_action), _lib.ptr(out), _lib.ptr(dl),
                                           _lib.current_stream(logits.device)))
    return out, dl
