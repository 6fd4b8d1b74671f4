"""Continuous CQL learn() path on the MI355X engine: SAC's networks and state (tianshou_amd.sac) with the conservative term.

Mirrors, on device tensors:
    CQL._update_with_batch        tianshou/algorithm/imitation/cql.py:268-400 (arXiv 2006.04779, Cal-QL option arXiv 2303.05479)
The order inside one update is the reference's, not SAC's: actor step on the critics before their update, alpha step, target
with the updated actor and alpha, critic losses + CQL term, Lagrange step, the two clipped critic steps, Polyak.  The policy
forward, the flat parameter layouts, their converters and the SAC part of a checkpoint's state are inherited from `SACEngine`;
the state this class adds is the Lagrange multiplier `cql_log_alpha` with its Adam moments.
`cql_log_alpha` LEARNS here, as it does in the reference on the CPU (on a cuda device the reference's `.to(device)` copy is
never stepped and the multiplier stays at its initial value).
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .sac import SACConfig, SACEngine

# TS_CQL_HP_* (include/tsengine.h)
CQL_HP = ("gamma", "cql_weight", "temperature", "with_lagrange", "lagrange_threshold", "alpha_min", "alpha_max", "cql_alpha_lr",
          "max_grad_norm")


@dataclass
class CQLConfig(SACConfig):
    """`SACConfig` + cql.py:44-58.  `min_action` / `max_action` only shape the random actions the CALLER draws
    (`uniform_(-min_action, max_action)`, cql.py:303-307: the defaults (-1, 1) give uniform_(1, 1), all ones)."""

    cql_alpha_lr: float = 1e-4
    cql_weight: float = 1.0
    temperature: float = 1.0
    with_lagrange: bool = True
    lagrange_threshold: float = 10.0
    min_action: float = -1.0
    max_action: float = 1.0
    num_repeat_actions: int = 10
    alpha_min: float = 0.0
    alpha_max: float = 1e6
    max_grad_norm: float = 1.0
    calibrated: bool = True
    cql_log_alpha0: float = 0.0

    def cql_hp(self, lr_scale: float = 1.0):
        v = {n: float(getattr(self, n)) for n in CQL_HP}
        v["cql_alpha_lr"] *= lr_scale if v["cql_alpha_lr"] >= 0 else 1.0
        return (C.c_double * len(CQL_HP))(*[v[n] for n in CQL_HP])


class CQLEngine(SACEngine):
    """State of one CQL learner on one GPU: `SACEngine` + the Lagrange multiplier; `update_with_batch` on ts_cql_update."""

    def __init__(self, obs_dim, act_dim, actor, critic1, critic2, cfg: CQLConfig, **kw):
        super().__init__(obs_dim, act_dim, actor, critic1, critic2, cfg, **kw)
        # {cql_log_alpha, exp_avg, exp_avg_sq} in one vector (ts_cql_update's cql_log_alpha3); the three views below alias it
        self._cql3 = torch.tensor([cfg.cql_log_alpha0, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.cql_log_alpha, self.cql_log_alpha_m, self.cql_log_alpha_v = self._cql3[0:1], self._cql3[1:2], self._cql3[2:3]

    def update_with_batch(self, obs, act, rew, done, obs_next, noise_actor, noise_next, random_act, noise_rep_cur,
                          noise_rep_next, calib=None, grads_out: torch.Tensor | None = None, lr_scale: float = 1.0,
                          target_out: torch.Tensor | None = None) -> torch.Tensor:
        """-> stats float32[7] (device) = {actor_loss, critic1_loss, critic2_loss, alpha, alpha_loss, cql_alpha,
        cql_alpha_loss}.  The five random tensors in the reference's draw order: rsample eps [B, A] of the actor loss and of
        the target, random_act [B R, A], rsample eps [B R, A] of pi(tmp_obs) and of pi(tmp_obs_next).  `calib`: the batch's
        `calibration_returns` [B] (required when cfg.calibrated).  grads_out (nullable): [critic1 | critic2 | actor], the
        critics' gradients before clipping.  The hyper-parameters are read from `cfg` at every call."""
        cfg = self.cfg
        obs, act, obs_next = self._f32(obs), self._f32(act), self._f32(obs_next)
        b, r, a = obs.shape[0], int(cfg.num_repeat_actions), self.act_dim
        if obs.shape != (b, self.obs_dim) or obs_next.shape != obs.shape or act.shape != (b, a):
            raise ValueError("obs / act / obs_next shapes do not match the engine")
        if cfg.calibrated and calib is None:
            raise ValueError("calibrated CQL needs the batch's calibration_returns")
        rew, done = self._f32(rew, (b,)), self._f32(done, (b,))
        calib = self._f32(calib, (b,)) if cfg.calibrated else None
        noise_actor, noise_next = self._f32(noise_actor, (b, a)), self._f32(noise_next, (b, a))
        random_act = self._f32(random_act, (b * r, a))
        noise_rep_cur, noise_rep_next = self._f32(noise_rep_cur, (b * r, a)), self._f32(noise_rep_next, (b * r, a))
        stats = torch.empty(7, dtype=torch.float32, device=self.device)
        st, hp = self._state_c(), cfg.to_c(lr_scale)
        _lib.check(_lib.load().ts_cql_update(
            self._ws.handle, C.byref(st), _lib.ptr(self._cql3), _lib.i64(self.adam_step + 1), _lib.ptr(obs), _lib.ptr(act),
            _lib.ptr(rew), _lib.ptr(done), _lib.ptr(obs_next), _lib.ptr(calib), _lib.ptr(noise_actor), _lib.ptr(noise_next),
            _lib.ptr(random_act), _lib.ptr(noise_rep_cur), _lib.ptr(noise_rep_next), _lib.i64(b), _lib.i64(r),
            _lib.i64(self.obs_dim), _lib.i64(a), C.byref(self._trunk), C.byref(hp), cfg.cql_hp(lr_scale), _lib.ptr(stats),
            _lib.ptr(target_out), _lib.ptr(grads_out), _lib.current_stream(self.device)))
        self.adam_step += 1                              # (after the call: a refused argument leaves the counter alone)
        return stats


def cql_loss(q_data, target, q_rand, q_cur, q_next, logp_cur, logp_next, calib, cql_log_alpha, act_dim: int, cfg: CQLConfig):
    """ts_cql_loss: the loss kernels alone on dense device arrays of both critics (q_data [2, B], q_* [2, B R]) ->
    (d_data [2, B], d_rep [2, 3, B R], loss9 = {mse_1, mse_2, mean logsumexp 1, 2, cql_1, cql_2, cql_alpha, cql_alpha_loss,
    d cql_alpha_loss / d cql_log_alpha}).  `cql_log_alpha`: a one-element device tensor (read only)."""
    dev = q_data.device
    f = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
    q_data, target, q_rand, q_cur, q_next = f(q_data), f(target), f(q_rand), f(q_cur), f(q_next)
    b = target.numel()
    r = int(cfg.num_repeat_actions)
    if q_data.shape != (2, b) or any(t.shape != (2, b * r) for t in (q_rand, q_cur, q_next)):
        raise ValueError("cql_loss: q_data [2, B], q_rand / q_cur / q_next [2, B R]")
    d_data = torch.empty((2, b), dtype=torch.float32, device=dev)
    d_rep = torch.empty((2, 3, b * r), dtype=torch.float32, device=dev)
    loss9 = torch.empty(9, dtype=torch.float32, device=dev)
    ws = _lib.default_workspace(dev.index or 0)
    _lib.check(_lib.load().ts_cql_loss(
        ws.handle, _lib.ptr(q_data), _lib.ptr(target), _lib.ptr(q_rand), _lib.ptr(q_cur), _lib.ptr(q_next),
        _lib.ptr(f(logp_cur).reshape(b * r)), _lib.ptr(f(logp_next).reshape(b * r)), _lib.ptr(f(calib)), _lib.ptr(f(cql_log_alpha)),
        _lib.i64(b), _lib.i64(r), _lib.i64(act_dim), cfg.cql_hp(), _lib.ptr(d_data), _lib.ptr(d_rep), _lib.ptr(loss9),
        _lib.current_stream(dev)))
    return d_data, d_rep, loss9
