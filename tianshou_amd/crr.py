"""DiscreteCRR learn() path on the MI355X engine (discrete critic-regularized regression, arXiv:2006.15134, on the Atari trunk).

Mirrors, on device tensors:
    DiscreteActor.forward / DiscreteCritic.forward   tianshou/utils/net/discrete.py (one DQNet(features_only=True), hidden [512])
    DiscreteCRR._update_with_batch                   tianshou/algorithm/imitation/discrete_crr.py:125-167 (periodic hard sync
                                                     first, expected-value target of the lagged pair, advantage-weighted actor
                                                     loss with an attached weight, critic loss, CQL term, ONE Adam).  The
                                                     reference's actor loss is the mean of a [B] x [B, 1] product, that is
                                                     mean(nll) * mean(weight); the engine computes that.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.

The network is DiscreteBCQ's (tianshou_amd/bcq.py, ts_bcq_layout): conv1 | conv2 | conv3 | first head | second head, with the
first head (BCQ's Q head) = the critic and the second (BCQ's imitator) = the actor.  `TIANSHOU_KEYS` is the order in which
`ModuleList([policy, critic]).named_parameters()` yields the reference's fourteen tensors -- the shared trunk once (under the
actor), the actor head, the critic head -- so `flat_from_torch` / `flat_to_torch` are bcq's conversions behind a permutation of
the two heads.  The lagged vector has the same length and both of its heads are read: the reference's `actor_old` and
`critic_old` are synced together, so their two trunks are equal and the engine keeps one.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib
from . import bcq as _bcq
from .buffer import _i64_dev
from .dqn import DQNHParams, _u8_flag
from .lagged import full_parameter_update

# ModuleList([policy, critic]).named_parameters() with policy.actor = DiscreteActor(feature_net, [512]) and critic =
# DiscreteCritic(feature_net, [512], last_size = n_act) on the SAME feature_net (listed once, under the actor)
TIANSHOU_KEYS = ["0.actor.preprocess.net.0.weight", "0.actor.preprocess.net.0.bias", "0.actor.preprocess.net.2.weight",
                 "0.actor.preprocess.net.2.bias", "0.actor.preprocess.net.4.weight", "0.actor.preprocess.net.4.bias",
                 "0.actor.last.model.0.weight", "0.actor.last.model.0.bias", "0.actor.last.model.2.weight",
                 "0.actor.last.model.2.bias", "1.last.model.0.weight", "1.last.model.0.bias", "1.last.model.2.weight",
                 "1.last.model.2.bias"]
HIDDEN = _bcq.HIDDEN
MODES = {"exp": 0, "binary": 1, "all": 2}
LOSS_NAMES = ("loss", "actor_loss", "critic_loss", "cql_loss")
_TO_BCQ = list(range(6)) + [10, 11, 12, 13, 6, 7, 8, 9]        # TIANSHOU_KEYS order -> trunk, critic (Q) head, actor (imitator) head

param_count = _bcq.param_count
layout = _bcq.layout


def flat_from_torch(tensors: list[torch.Tensor], c: int, h: int, w: int, n_act: int, device="cuda") -> torch.Tensor:
    """The fourteen tensors of TIANSHOU_KEYS in torch layout (also valid for the matching Adam moments) -> the flat vector."""
    if len(tensors) != 14:
        raise ValueError("expected the fourteen parameters of ModuleList([policy, critic]) (TIANSHOU_KEYS)")
    return _bcq.flat_from_torch([tensors[i] for i in _TO_BCQ], c, h, w, n_act, device)


def flat_to_torch(flat: torch.Tensor, c: int, h: int, w: int, n_act: int) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> fourteen tensors in torch layout, TIANSHOU_KEYS order (on flat's device)."""
    t = _bcq.flat_to_torch(flat, c, h, w, n_act)
    out: list = [None] * 14
    for j, i in enumerate(_TO_BCQ):
        out[i] = t[j]
    return out


def mode_id(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"policy_improvement_mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


# ---- the per-sample kernels on raw arrays (edge tests) ------------------------------------------------------------------
def _u8_dev(x, device) -> torch.Tensor:
    return torch.as_tensor(x, device=device).to(torch.uint8).reshape(-1).contiguous()


def _f32_1d(x, device) -> torch.Tensor:
    return torch.as_tensor(x, device=device).to(torch.float32).reshape(-1).contiguous()


def expected_target(q_old, logits_old, rew, done, gamma: float, device="cuda") -> torch.Tensor:
    """rew + gamma * (done > 0 ? 0 : sum_j softmax(logits_old)_j q_old_j) of float32[B, A] arrays (ts_crr_target) -> float32[B].
    `done`: uint8 flags (any integer array in [0, 255] is converted)."""
    q_old, logits_old = _bcq._f32_2d(q_old, device), _bcq._f32_2d(logits_old, device)
    b = q_old.shape[0]
    rew, done = _f32_1d(rew, q_old.device), _u8_dev(done, q_old.device)
    if q_old.shape != logits_old.shape or rew.numel() != b or done.numel() != b:
        raise ValueError("q_old / logits_old / rew / done batch sizes differ")
    out = torch.empty(b, dtype=torch.float32, device=q_old.device)
    _lib.check(_lib.load().ts_crr_target(_lib.ptr(q_old), _lib.ptr(logits_old), _lib.ptr(rew), _lib.ptr(done), _lib.i64(b),
                                         _lib.i64(q_old.shape[1]), _lib.f64(gamma), _lib.ptr(out),
                                         _lib.current_stream(q_old.device)))
    return out


def loss_terms(q, logits, act, target, mode: str, beta: float, ratio_upper_bound: float, min_q_weight: float, device="cuda",
               fill: float | None = None) -> dict:
    """The loss kernels on raw arrays (ts_crr_loss) -> {dq [B, ld], dlogits [B, ld], terms [6, B], losses [6] =
    [loss, actor_loss, critic_loss, cql_loss, mean nll, mean coef]}.
    `fill`: value every output buffer holds before the call (a sentinel that must be gone afterwards)."""
    q, logits = _bcq._f32_2d(q, device), _bcq._f32_2d(logits, device)
    b, a = q.shape
    ld = (a + 31) // 32 * 32
    act = _i64_dev(act, q.device).reshape(-1)
    target = _f32_1d(target, q.device)
    if q.shape != logits.shape or act.numel() != b or target.numel() != b:
        raise ValueError("q / logits / act / target batch sizes differ")
    mk = (lambda *s: torch.empty(s, dtype=torch.float32, device=q.device)) if fill is None else \
        (lambda *s: torch.full(s, fill, dtype=torch.float32, device=q.device))
    out = {"dq": mk(b, ld), "dlogits": mk(b, ld), "terms": mk(6, b), "losses": mk(6)}
    _lib.check(_lib.load().ts_crr_loss(_lib.ptr(q), _lib.ptr(logits), _lib.ptr(act), _lib.ptr(target), _lib.i64(b), _lib.i64(a),
                                       _lib.i64(mode_id(mode)), _lib.f64(beta), _lib.f64(ratio_upper_bound),
                                       _lib.f64(min_q_weight), _lib.ptr(out["dq"]), _lib.ptr(out["dlogits"]),
                                       _lib.ptr(out["terms"]), _lib.ptr(out["losses"]), _lib.current_stream(q.device)))
    return out


@dataclass
class CRRConfig:
    """Hyper-parameters of the reference DiscreteCRR (discrete_crr.py:39-111) + Adam (optim.py:89-110)."""

    gamma: float = 0.99
    policy_improvement_mode: str = "exp"
    ratio_upper_bound: float = 20.0
    beta: float = 1.0
    min_q_weight: float = 10.0
    target_update_freq: int = 0           # 0: no lagged networks, the target reads the live pair
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None

    def __post_init__(self):
        mode_id(self.policy_improvement_mode)
        if not (math.isfinite(self.beta) and self.beta != 0):
            raise ValueError(f"beta must be finite and nonzero but got: {self.beta}")

    def to_c(self, grad_only: bool = False) -> DQNHParams:
        return DQNHParams(-1.0 if grad_only else self.lr, self.betas[0], self.betas[1], self.adam_eps, 1.0,
                          self.max_grad_norm or 0.0)


class CRREngine:
    """State of one DiscreteCRR learner on one GPU: flat parameters, lagged copy, Adam moments, counters."""

    def __init__(self, c: int, h: int, w: int, n_act: int, flat_params: torch.Tensor, cfg: CRRConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("CRREngine needs parameters on an MI355X (no CPU fallback)")
        self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
        self.P = param_count(c, h, w, n_act)
        if flat_params.numel() != self.P:
            raise ValueError(f"expected {self.P} parameters, got {flat_params.numel()}")
        self.device = flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        # discrete_crr.py:102-107: two lagged copies with target_update_freq > 0, the live networks themselves otherwise
        self.params_old = self.params.clone() if cfg.target_update_freq > 0 else self.params
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.adam_step = 0
        self.iter = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _check_obs(self, obs: torch.Tensor) -> torch.Tensor:
        if tuple(obs.shape[1:]) != (self.h, self.w, self.c) or obs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs must be float32 or uint8 [B, {self.h}, {self.w}, {self.c}] (NHWC)")
        return obs.contiguous()

    def wait_td(self, stream: torch.cuda.Stream) -> None:
        """`stream` waits for the four losses of the last `update_with_batch`, not for its backward pass and Adam step."""
        _lib.check(_lib.load().ts_dqn_wait_td(self._ws.handle, C.c_void_p(stream.cuda_stream)))

    # -- _update_with_batch ---------------------------------------------------------------------------------
    def update_with_batch(self, obs_nhwc, obs_next_nhwc, act, rew, done, grad_out: torch.Tensor | None = None,
                          target_out: torch.Tensor | None = None, apply: bool = True):
        """-> losses float32[4] device tensor = [loss, actor_loss, critic_loss, cql_loss].  rew float32[B], done uint8[B]
        (`> 0` masks the bootstrap).  `cfg.lr`, the mode, `beta`, `ratio_upper_bound`, `min_q_weight` and `gamma` are read at
        every call; target_out float32[B] receives the targets; apply=False computes the gradient only (into grad_out) and
        leaves parameters, lagged parameters, moments and counters untouched."""
        cfg = self.cfg
        if not apply and grad_out is None:
            raise ValueError("apply=False computes the gradient only: pass grad_out")
        obs_nhwc, obs_next_nhwc = self._check_obs(obs_nhwc), self._check_obs(obs_next_nhwc)
        b = obs_nhwc.shape[0]
        if obs_next_nhwc.shape != obs_nhwc.shape or obs_next_nhwc.dtype != obs_nhwc.dtype:
            raise ValueError("obs and obs_next differ in shape or dtype")
        act = _i64_dev(act, self.device).reshape(-1)
        rew, done = _f32_1d(rew, self.device), _u8_dev(done, self.device)
        if b < 1 or act.numel() != b or rew.numel() != b or done.numel() != b:
            raise ValueError("obs / act / rew / done batch sizes differ")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32 or not grad_out.is_cuda):
            raise ValueError(f"grad_out must be a float32 device tensor of {self.P} elements")
        if target_out is not None and (target_out.numel() != b or target_out.dtype != torch.float32 or not target_out.is_cuda):
            raise ValueError("target_out must be a float32 device tensor of B elements")
        if apply:
            if cfg.target_update_freq > 0 and self.iter % cfg.target_update_freq == 0:      # discrete_crr.py:129-130
                full_parameter_update(self.params_old, self.params)
            self.iter += 1
            self.adam_step += 1
        old = self.params_old if cfg.target_update_freq > 0 else self.params
        losses = torch.empty(6, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_crr_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(old), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
            _lib.i64(max(self.adam_step, 1)), _lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act),
            _lib.ptr(obs_nhwc), _lib.ptr(obs_next_nhwc), _u8_flag(obs_nhwc), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done),
            _lib.i64(b), C.byref(hp), _lib.f64(cfg.gamma), _lib.i64(mode_id(cfg.policy_improvement_mode)), _lib.f64(cfg.beta),
            _lib.f64(cfg.ratio_upper_bound), _lib.f64(cfg.min_q_weight), _lib.ptr(losses), _lib.ptr(target_out),
            _lib.ptr(grad_out), _lib.current_stream(self.device)))
        return losses[:4]
