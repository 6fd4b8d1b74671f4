"""DiscreteBCQ learn() path on the MI355X engine (discrete batch-constrained Q-learning, arXiv:1910.01708, on the Atari trunk).

Mirrors, on device tensors:
    DiscreteActor.forward (twice, one trunk)   tianshou/utils/net/discrete.py (DQNet(features_only=True), hidden [512], no softmax)
    DiscreteBCQPolicy.forward                  tianshou/algorithm/imitation/discrete_bcq.py:104-127
    DiscreteBCQ._target_q / _preprocess_batch  discrete_bcq.py:213-234 (n-step via tianshou_amd.returns)
    DiscreteBCQ._update_with_batch             discrete_bcq.py:236-261 (periodic hard sync first, update 0 included)
There is no CPU path: every function calls libtsengine.so and raises when it is missing.

Parameter layout (ts_bcq_layout): conv1 | conv2 | conv3 (the DQN engine's matrices) | Q fc1 [F + 1, 512] | Q fc2 [513, ld] |
I fc1 [F + 1, 512] | I fc2 [513, ld]; F in (h, w, c) order, ld = n_act rounded up to a multiple of 32 with zero padding
columns.  `flat_from_torch` / `flat_to_torch` convert the fourteen parameters of the reference policy (`TIANSHOU_KEYS`: the
shared trunk once, then the two heads).  The lagged vector has the same length; the reference's `model_old` is a copy of
`policy.model` alone, so its imitator part is unused and never read.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .buffer import DeviceReplayBuffer, _i64_dev
from .dqn import DQNHParams, _u8_flag, gather_obs_nhwc
from .lagged import full_parameter_update
from .returns import compute_nstep_return

# DiscreteBCQPolicy.named_parameters() with policy.model = DiscreteActor(feature_net, [512]) and policy.imitator = the same
# class on the SAME feature_net (the shared trunk is listed once, under the model)
TIANSHOU_KEYS = ["model.preprocess.net.0.weight", "model.preprocess.net.0.bias", "model.preprocess.net.2.weight",
                 "model.preprocess.net.2.bias", "model.preprocess.net.4.weight", "model.preprocess.net.4.bias",
                 "model.last.model.0.weight", "model.last.model.0.bias", "model.last.model.2.weight", "model.last.model.2.bias",
                 "imitator.last.model.0.weight", "imitator.last.model.0.bias", "imitator.last.model.2.weight",
                 "imitator.last.model.2.bias"]
N_LAGGED = 10            # model_old holds the trunk and the Q head: the first ten tensors
HIDDEN = 512


def param_count(c: int, h: int, w: int, n_act: int) -> int:
    lib = _lib.load()
    lib.ts_bcq_param_count.restype = C.c_int64
    lib.ts_bcq_param_count.argtypes = [C.c_int64] * 4
    n = int(lib.ts_bcq_param_count(c, h, w, n_act))
    if n < 0:
        raise ValueError("unsupported DiscreteBCQ network (1 <= n_act <= 64, observation >= 36 x 36)")
    return n


def layout(c: int, h: int, w: int, n_act: int) -> dict:
    """-> {F, ld, total, off: int64[8] = starts of conv1, conv2, conv3, Q fc1, Q fc2, I fc1, I fc2 and the end}."""
    out = (C.c_int64 * 10)()
    _lib.check(_lib.load().ts_bcq_layout(_lib.i64(c), _lib.i64(h), _lib.i64(w), _lib.i64(n_act), out))
    v = [int(x) for x in out]
    return {"F": v[0], "ld": v[1], "total": v[2], "off": np.array(v[3:10] + [v[2]], np.int64)}


def _conv_hw(h: int, w: int) -> tuple[int, int]:
    for k, s in ((8, 4), (4, 2), (3, 1)):
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return h, w


def log_tau_f32(threshold: float) -> float:
    """log(unlikely_action_threshold) rounded to float32, the precision the reference compares in; -inf for 0."""
    if not 0.0 <= threshold < 1.0:
        raise ValueError(f"unlikely_action_threshold should be in [0, 1) but got: {threshold}")
    return float(np.float32(math.log(threshold))) if threshold > 0 else -math.inf


def flat_from_torch(tensors: list[torch.Tensor], c: int, h: int, w: int, n_act: int, device="cuda") -> torch.Tensor:
    """The fourteen tensors of TIANSHOU_KEYS in torch layout (also valid for the matching Adam moments) -> the flat vector.
    Ten tensors (a lagged `model_old`) fill the trunk and the Q head; the imitator part is zero."""
    if len(tensors) not in (N_LAGGED, 14):
        raise ValueError("expected the fourteen parameters of DiscreteBCQPolicy (TIANSHOU_KEYS), or the first ten of them")
    t = [x.detach().float().cpu() for x in tensors]
    oh, ow = _conv_hw(h, w)
    f, ld = 64 * oh * ow, (n_act + 31) // 32 * 32
    parts = []
    for i in range(3):
        parts += [t[2 * i].permute(2, 3, 1, 0).reshape(-1), t[2 * i + 1].reshape(-1)]     # [oc, ic, kh, kw] -> [(kh, kw, ic), oc]
    for j in (6, 10):
        if j >= len(t):
            parts.append(torch.zeros((f + 1) * HIDDEN + (HIDDEN + 1) * ld, dtype=torch.float32))
            continue
        parts += [t[j].reshape(HIDDEN, 64, oh, ow).permute(2, 3, 1, 0).reshape(-1), t[j + 1].reshape(-1)]
        head = torch.zeros((HIDDEN + 1, ld), dtype=torch.float32)
        head[:HIDDEN, :n_act] = t[j + 2].t()
        head[HIDDEN, :n_act] = t[j + 3]
        parts.append(head.reshape(-1))
    flat = torch.cat(parts)
    assert flat.numel() == (8 * 8 * c + 1) * 32 + 513 * 64 + 577 * 64 + 2 * ((f + 1) * HIDDEN + (HIDDEN + 1) * ld)
    return flat.to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, c: int, h: int, w: int, n_act: int) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> fourteen tensors in torch layout, TIANSHOU_KEYS order (on flat's device)."""
    oh, ow = _conv_hw(h, w)
    f, ld = 64 * oh * ow, (n_act + 31) // 32 * 32
    out, o = [], 0
    for ic, k, oc in ((c, 8, 32), (32, 4, 64), (64, 3, 64)):
        kk = k * k * ic
        wb = flat[o:o + (kk + 1) * oc].reshape(kk + 1, oc)
        out += [wb[:kk].reshape(k, k, ic, oc).permute(3, 2, 0, 1).contiguous(), wb[kk].clone()]
        o += (kk + 1) * oc
    for _ in range(2):
        wb = flat[o:o + (f + 1) * HIDDEN].reshape(f + 1, HIDDEN)
        o += (f + 1) * HIDDEN
        out += [wb[:f].reshape(oh, ow, 64, HIDDEN).permute(3, 2, 0, 1).reshape(HIDDEN, f).contiguous(), wb[f].clone()]
        wb = flat[o:o + (HIDDEN + 1) * ld].reshape(HIDDEN + 1, ld)
        o += (HIDDEN + 1) * ld
        out += [wb[:HIDDEN, :n_act].t().contiguous(), wb[HIDDEN, :n_act].clone()]
    return out


# ---- the per-sample kernels on raw arrays (edge tests) ------------------------------------------------------------------
def _f32_2d(x, device) -> torch.Tensor:
    x = torch.as_tensor(x, device=device).to(torch.float32).contiguous()
    if x.dim() != 2 or not 1 <= x.shape[1] <= 64:
        raise ValueError("expected float32 [B, n_act], 1 <= n_act <= 64")
    return x


def masked_argmax(q, logits, log_tau: float, device="cuda") -> torch.Tensor:
    """DiscreteBCQPolicy.forward's action of q / logits float32[B, A] (ts_bcq_head) -> int64[B]."""
    q, logits = _f32_2d(q, device), _f32_2d(logits, device)
    if q.shape != logits.shape:
        raise ValueError("q and logits differ in shape")
    act = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    _lib.check(_lib.load().ts_bcq_head(_lib.ptr(q), _lib.ptr(logits), _lib.i64(q.shape[0]), _lib.i64(q.shape[1]),
                                       _lib.f64(log_tau), _lib.ptr(act), _lib.current_stream(q.device)))
    return act


def target_select(q, logits, q_old, log_tau: float, device="cuda"):
    """-> (q_old[b, act[b]] float32[B], act int64[B]) with act = the masked argmax of the live pair (ts_bcq_target)."""
    q, logits, q_old = _f32_2d(q, device), _f32_2d(logits, device), _f32_2d(q_old, device)
    if q.shape != logits.shape or q.shape != q_old.shape:
        raise ValueError("q, logits and q_old differ in shape")
    out = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    act = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    _lib.check(_lib.load().ts_bcq_target(_lib.ptr(q), _lib.ptr(logits), _lib.ptr(q_old), _lib.i64(q.shape[0]),
                                         _lib.i64(q.shape[1]), _lib.f64(log_tau), _lib.ptr(out), _lib.ptr(act),
                                         _lib.current_stream(q.device)))
    return out, act


def loss_terms(q, logits, act, returns, penalty: float, device="cuda", fill: float | None = None) -> dict:
    """The loss kernels on raw arrays (ts_bcq_loss) -> {dq [B, ld], dlogits [B, ld], terms [4, B], losses [4]}.
    `fill`: value every output buffer holds before the call (a sentinel that must be gone afterwards)."""
    q, logits = _f32_2d(q, device), _f32_2d(logits, device)
    b, a = q.shape
    ld = (a + 31) // 32 * 32
    act = _i64_dev(act, q.device).reshape(-1)
    returns = torch.as_tensor(returns, device=q.device).to(torch.float32).reshape(-1).contiguous()
    if q.shape != logits.shape or act.numel() != b or returns.numel() != b:
        raise ValueError("q / logits / act / returns batch sizes differ")
    mk = (lambda *s: torch.empty(s, dtype=torch.float32, device=q.device)) if fill is None else \
        (lambda *s: torch.full(s, fill, dtype=torch.float32, device=q.device))
    out = {"dq": mk(b, ld), "dlogits": mk(b, ld), "terms": mk(4, b), "losses": mk(4)}
    _lib.check(_lib.load().ts_bcq_loss(_lib.ptr(q), _lib.ptr(logits), _lib.ptr(act), _lib.ptr(returns), _lib.i64(b), _lib.i64(a),
                                       _lib.f64(penalty), _lib.ptr(out["dq"]), _lib.ptr(out["dlogits"]), _lib.ptr(out["terms"]),
                                       _lib.ptr(out["losses"]), _lib.current_stream(q.device)))
    return out


@dataclass
class BCQConfig:
    """Hyper-parameters of the reference DiscreteBCQPolicy / DiscreteBCQ (discrete_bcq.py:37-211) + Adam (optim.py:89-110)."""

    gamma: float = 0.99
    n_step: int = 1
    target_update_freq: int = 8000
    unlikely_action_threshold: float = 0.3
    imitation_logits_penalty: float = 1e-2
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None
    log_tau: float | None = None      # set: used instead of log(unlikely_action_threshold) (the reference policy keeps only `_log_tau`)

    def __post_init__(self):
        if not self.target_update_freq > 0:                                    # discrete_bcq.py:93-95
            raise ValueError(f"BCQ needs target_update_freq>0 but got: {self.target_update_freq}.")
        log_tau_f32(self.unlikely_action_threshold)

    def to_c(self, grad_only: bool = False) -> DQNHParams:
        return DQNHParams(-1.0 if grad_only else self.lr, self.betas[0], self.betas[1], self.adam_eps, 1.0,
                          self.max_grad_norm or 0.0)


class BCQEngine:
    """State of one DiscreteBCQ learner on one GPU: flat parameters, lagged copy, Adam moments, counters."""

    def __init__(self, c: int, h: int, w: int, n_act: int, flat_params: torch.Tensor, cfg: BCQConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("BCQEngine needs parameters on an MI355X (no CPU fallback)")
        self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
        self.P = param_count(c, h, w, n_act)
        if flat_params.numel() != self.P:
            raise ValueError(f"expected {self.P} parameters, got {flat_params.numel()}")
        self.device = flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        self.params_old = self.params.clone()               # discrete_bcq.py:209-210 (the imitator part is never read)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.adam_step = 0
        self.iter = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _dims(self):
        return (_lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act))

    def _check_obs(self, obs: torch.Tensor) -> torch.Tensor:
        if tuple(obs.shape[1:]) != (self.h, self.w, self.c) or obs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs must be float32 or uint8 [B, {self.h}, {self.w}, {self.c}] (NHWC)")
        return obs.contiguous()

    def log_tau(self) -> float:
        """The threshold the kernels compare with: float32(log tau), read from the config at every call."""
        if self.cfg.log_tau is not None:
            return float(np.float32(self.cfg.log_tau))
        return log_tau_f32(self.cfg.unlikely_action_threshold)

    # -- DiscreteBCQPolicy.forward ---------------------------------------------------------------------
    def forward(self, obs_nhwc: torch.Tensor, params: torch.Tensor | None = None):
        """-> (q float32[B, A], imitation logits float32[B, A], act int64[B] = the threshold-masked argmax)."""
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        logits = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        p = self.params if params is None else params
        _lib.check(_lib.load().ts_bcq_forward(
            self._ws.handle, _lib.ptr(p), *self._dims(), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.i64(b),
            _lib.f64(self.log_tau()), _lib.ptr(q), _lib.ptr(logits), _lib.ptr(act), _lib.current_stream(self.device)))
        return q, logits, act

    # -- DiscreteBCQ._target_q ----------------------------------------------------------------------------
    def target_q(self, obs_next_nhwc: torch.Tensor, want_act: bool = False):
        """Q_old(obs_next)[act], act from the live Q head and the live imitator -> float32[B] (and act int64[B])."""
        obs_next_nhwc = self._check_obs(obs_next_nhwc)
        b = obs_next_nhwc.shape[0]
        out = torch.empty(b, dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device) if want_act else None
        _lib.check(_lib.load().ts_bcq_target_q(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), *self._dims(), _lib.ptr(obs_next_nhwc),
            _u8_flag(obs_next_nhwc), _lib.i64(b), _lib.f64(self.log_tau()), _lib.ptr(out), _lib.ptr(act),
            _lib.current_stream(self.device)))
        return (out, act) if want_act else out

    # -- _preprocess_batch (discrete_bcq.py:213-226) --------------------------------------------------------
    def preprocess(self, buffer: DeviceReplayBuffer, frames: torch.Tensor, indices, stack_num: int,
                   obs_next_frames: torch.Tensor | None = None) -> torch.Tensor:
        """n-step returns float32[I] of the batch-constrained target."""

        def tq_fn(buf, after):
            if obs_next_frames is None:
                on = gather_obs_nhwc(frames, buf, buf.next(after), stack_num, as_u8=True)
            else:
                on = gather_obs_nhwc(obs_next_frames, buf, after, stack_num, as_u8=True)
            return self.target_q(on)

        class _B:
            pass

        return compute_nstep_return(_B(), buffer, indices, tq_fn, self.cfg.gamma, self.cfg.n_step).returns

    def wait_td(self, stream: torch.cuda.Stream) -> None:
        """`stream` waits for the four losses of the last `update_with_batch`, not for its backward pass and Adam step."""
        _lib.check(_lib.load().ts_dqn_wait_td(self._ws.handle, C.c_void_p(stream.cuda_stream)))

    # -- _update_with_batch ---------------------------------------------------------------------------------
    def update_with_batch(self, obs_nhwc, act, returns, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> losses float32[4] device tensor = [loss, q_loss, i_loss, reg_loss].  returns float32[B].  `cfg.lr`,
        `cfg.imitation_logits_penalty` are read at every call; apply=False computes the gradient only (into grad_out) and
        leaves parameters, moments and counters untouched."""
        cfg = self.cfg
        if not apply and grad_out is None:
            raise ValueError("apply=False computes the gradient only: pass grad_out")
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        act = _i64_dev(act, self.device).reshape(-1)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if b < 1 or act.numel() != b or returns.numel() != b:
            raise ValueError("obs / act / returns batch sizes differ (returns: float32 [B])")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32 or not grad_out.is_cuda):
            raise ValueError(f"grad_out must be a float32 device tensor of {self.P} elements")
        if apply:
            if self.iter % cfg.target_update_freq == 0:                      # discrete_bcq.py:240-241
                full_parameter_update(self.params_old, self.params)
            self.iter += 1
            self.adam_step += 1
        losses = torch.empty(4, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_bcq_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
            _lib.i64(max(self.adam_step, 1)), *self._dims(), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.ptr(act),
            _lib.ptr(returns), _lib.i64(b), C.byref(hp), _lib.f64(cfg.imitation_logits_penalty), _lib.ptr(losses),
            _lib.ptr(grad_out), _lib.current_stream(self.device)))
        return losses
