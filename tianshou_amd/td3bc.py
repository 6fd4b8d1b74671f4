"""TD3+BC learn() path on the MI355X engine: TD3 (tianshou_amd.td3) with the behaviour-cloning term in the actor loss.

Mirrors, on device tensors:
    TD3BC._update_with_batch        tianshou/algorithm/imitation/td3_bc.py:102-127 (arXiv 2106.06860)
Everything else is TD3's and is inherited from `TD3Engine`: the policy forward, `_target_q` with the smoothing noise, the
n-step returns of `_preprocess_batch`, the critic steps, the delayed actor, the Polyak updates and the state a checkpoint
carries (`cnt`, `actor_steps`, moments, lagged networks).  The flat parameter layouts are td3's.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .td3 import TD3Config, TD3Engine, TD3HParams, TD3StateC


@dataclass
class TD3BCConfig(TD3Config):
    """`TD3Config` of a twin TD3 + td3_bc.py:31 `alpha` (the weight of the Q term relative to behaviour cloning)."""

    alpha: float = 2.5

    def __post_init__(self):
        if not self.twin:
            raise ValueError("TD3+BC is TD3 with a behaviour-cloning term: twin must be True (two critics)")


class TD3BCEngine(TD3Engine):
    """State of one TD3+BC learner on one GPU: `TD3Engine` with `update_with_batch` on ts_td3bc_update."""

    def update_with_batch(self, obs, act, returns, weight=None, grads_out=None, lr_scale: float = 1.0):
        """-> (stats float32[4] = {actor_loss, critic1_loss, critic2_loss, lmbda}, weight); actor_loss and lmbda are those of
        the latest actor update.  `cfg.alpha` is read at every call; the library refuses a negative or non-finite one
        (EngineError, TS_ERR_INVALID_ARG).  Where mean|Q1| is 0, lmbda is inf / NaN as in the reference."""
        cfg = self.cfg
        obs, act = self._f32(obs), self._f32(act)
        b = obs.shape[0]
        returns = self._f32(returns, (b,))
        weight = None if weight is None else self._f32(weight, (b,))
        if obs.shape != (b, self.obs_dim) or act.shape != (b, self.act_dim):
            raise ValueError("obs / act shapes do not match the engine")
        upd = self.cnt % cfg.update_actor_freq == 0                                  # td3_bc.py:113
        if not hasattr(self, "_stats"):
            self._stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        w_out = torch.empty(b, dtype=torch.float32, device=self.device)
        names = [n for n, _ in TD3StateC._fields_]
        st = TD3StateC(*[None if getattr(self, n) is None else getattr(self, n).data_ptr() for n in names])
        hp = TD3HParams(cfg.actor_lr * lr_scale, cfg.critic_lr * lr_scale, cfg.betas[0], cfg.betas[1], cfg.adam_eps,
                        cfg.tau, cfg.max_action, int(upd), 0)
        _lib.check(_lib.load().ts_td3bc_update(
            self._ws.handle, C.byref(st), _lib.i64(self.cnt + 1), _lib.i64(max(self.actor_steps + int(upd), 1)), _lib.ptr(obs),
            _lib.ptr(act), _lib.ptr(returns), _lib.ptr(weight), _lib.i64(b), _lib.i64(self.obs_dim),
            _lib.i64(self.act_dim), C.byref(self._trunk), C.byref(hp), _lib.f64(cfg.alpha), _lib.ptr(self._stats),
            _lib.ptr(w_out), _lib.ptr(grads_out), _lib.current_stream(self.device)))
        self.cnt += 1                                # (after the call: a refused alpha leaves the counters alone)
        self.actor_steps += int(upd)
        return self._stats.clone(), w_out
