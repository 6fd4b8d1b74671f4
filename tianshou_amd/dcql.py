"""DiscreteCQL learn() path on the MI355X engine: QRDQN (tianshou_amd.distq) with the conservative term in the loss.

Mirrors, on device tensors:
    DiscreteCQL._update_with_batch        tianshou/algorithm/imitation/discrete_cql.py:80-113
Everything else is QRDQN's and is inherited from `DistQEngine`: QRDQNet.forward, `_target_q`, the n-step quantile targets of
`_preprocess_batch`, the periodic hard sync and the Adam step.  The flat parameter layout is distq's.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .buffer import _i64_dev
from .distq import QR, DistQConfig, DistQEngine
from .dqn import _u8_flag
from .lagged import full_parameter_update


@dataclass
class DiscreteCQLConfig(DistQConfig):
    """`DistQConfig` of a QRDQN (`kind` is fixed) + discrete_cql.py:31 `min_q_weight`."""

    min_q_weight: float = 10.0

    def __post_init__(self):
        if self.kind != QR:
            raise ValueError("DiscreteCQL is QRDQN with a conservative term: kind must be 'qr'")


class DiscreteCQLEngine(DistQEngine):
    """State of one DiscreteCQL learner on one GPU: `DistQEngine` (QR) with `update_with_batch` on ts_dcql_update."""

    def update_with_batch(self, obs_nhwc, act, returns, weight=None, obs_next_nhwc=None,
                          grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (losses float32[3] device tensor = [loss, qr_loss, cql_loss], new batch.weight float32[B]).
        `obs_next_nhwc` is accepted for call compatibility with the parent and unused (QRDQN needs none).  `cfg.min_q_weight` is
        read at every call; the library refuses a negative or non-finite one (EngineError, TS_ERR_INVALID_ARG)."""
        cfg = self.cfg
        if apply:
            if self.params_old is not None and self.iter % cfg.target_update_freq == 0:    # dqn.py:283-285
                full_parameter_update(self.params_old, self.params)
            self.iter += 1
            self.adam_step += 1
        obs_nhwc = self._check_obs(obs_nhwc)
        b, n = obs_nhwc.shape[0], cfg.n_atoms
        act = _i64_dev(act, self.device).reshape(-1)
        returns = torch.as_tensor(returns, dtype=torch.float32, device=self.device).contiguous()
        if weight is not None:
            weight = torch.as_tensor(weight, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if act.numel() != b or tuple(returns.shape) != (b, n) or (weight is not None and weight.numel() != b):
            raise ValueError("obs / act / returns / weight batch sizes differ")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32 or not grad_out.is_cuda):
            raise ValueError(f"grad_out must be a float32 device tensor of {self.P} elements")
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        losses = torch.empty(3, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_dcql_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
            _lib.i64(max(self.adam_step, 1)), _lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act),
            _lib.i64(n), _lib.ptr(self.aux), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.ptr(act), _lib.ptr(returns),
            _lib.ptr(weight), _lib.i64(b), C.byref(hp), _lib.f64(cfg.min_q_weight), _lib.ptr(prio), _lib.ptr(losses),
            _lib.ptr(grad_out), _lib.current_stream(self.device)))
        return losses, prio
