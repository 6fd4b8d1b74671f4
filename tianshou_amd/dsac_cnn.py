"""DiscreteSAC learn() path on the Atari trunk on the MI355X engine (arXiv:1910.07207; examples/atari/atari_sac.py).

Mirrors, on device tensors:
    DiscreteActor.forward / DiscreteCritic.forward   tianshou/utils/net/discrete.py (single Linear heads on ONE shared
                                                     DQNet(features_only=True, output_dim_added_layer=H))
    _target_q / _target_q_compute_value              ddpg.py:327-339, discrete_sac.py:147-155 (n-step via tianshou_amd.returns)
    DiscreteSAC._update_with_batch                   discrete_sac.py:157-196: critic 1, critic 2, actor, AutoAlpha, Polyak
There is no CPU path: every function calls libtsengine.so and raises when it is missing.

The shared trunk's eight tensors sit in ALL THREE optimizers of the reference (`policy_optim`, `critic_optim`, `critic2_optim`
hold ten tensors each: the trunk and their own head), so the trunk is stepped three times per update by three Adam instances
with three moment sets, strictly in sequence.  The engine keeps three moment pairs, each over trunk | own head, in the order
critic 1, critic 2, actor (`SETS`).  `critic_old` and `critic2_old` each own a deep copy of the trunk; both start equal and are
Polyak-averaged from the same live trunk with the same tau, so they stay bit-equal: the engine keeps one lagged trunk.

Parameter layout (ts_dsac_cnn_layout): conv1 | conv2 | conv3 | fc [F + 1, H] | actor head | critic-1 head | critic-2 head, the
heads [H + 1, ld]; F in (h, w, c) order, ld = n_act rounded up to a multiple of 32 with zero padding columns.  Lagged vector:
conv1 | conv2 | conv3 | fc | critic-1 head | critic-2 head.  `TIANSHOU_KEYS` is the order in which
`ModuleList([policy, critic, critic2]).named_parameters()` yields the reference's fourteen tensors: the trunk once (under the
actor), then the three heads.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .buffer import DeviceReplayBuffer, _i64_dev
from .dqn import _u8_flag, gather_obs_nhwc
from .returns import compute_nstep_return, nstep_return_from_target_q
from .sac import SACConfig

TRUNK_KEYS = ["preprocess.net.0.0.weight", "preprocess.net.0.0.bias", "preprocess.net.0.2.weight", "preprocess.net.0.2.bias",
              "preprocess.net.0.4.weight", "preprocess.net.0.4.bias", "preprocess.net.1.weight", "preprocess.net.1.bias"]
HEAD_KEYS = ["last.model.0.weight", "last.model.0.bias"]
TIANSHOU_KEYS = (["0.actor." + k for k in TRUNK_KEYS + HEAD_KEYS] + ["1." + k for k in HEAD_KEYS] + ["2." + k for k in HEAD_KEYS])
SETS = ("critic1", "critic2", "actor")              # order of the three gradient / moment sets
STAT_NAMES = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")


def param_count(c: int, h: int, w: int, n_act: int, hidden: int = 512) -> int:
    lib = _lib.load()
    lib.ts_dsac_cnn_param_count.restype = C.c_int64
    lib.ts_dsac_cnn_param_count.argtypes = [C.c_int64] * 5
    n = int(lib.ts_dsac_cnn_param_count(c, h, w, n_act, hidden))
    if n < 0:
        raise ValueError("unsupported DiscreteSAC network (1 <= n_act <= 64, hidden a multiple of 32 in [32, 1024], "
                         "observation >= 36 x 36)")
    return n


def layout(c: int, h: int, w: int, n_act: int, hidden: int = 512) -> dict:
    """-> {F, ld, total, T (trunk length), Hd (one head's length), off: int64[8] = starts of conv1, conv2, conv3, fc, actor head,
    critic-1 head, critic-2 head and the end}."""
    out = (C.c_int64 * 11)()
    _lib.check(_lib.load().ts_dsac_cnn_layout(_lib.i64(c), _lib.i64(h), _lib.i64(w), _lib.i64(n_act), _lib.i64(hidden), out))
    v = [int(x) for x in out]
    return {"F": v[0], "ld": v[1], "total": v[2], "T": v[3], "Hd": (hidden + 1) * v[1], "off": np.array(v[4:11] + [v[2]], np.int64)}


def _conv_hw(h: int, w: int) -> tuple[int, int]:
    for k, s in ((8, 4), (4, 2), (3, 1)):
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return h, w


def _trunk_parts(t: list[torch.Tensor], oh: int, ow: int, hidden: int) -> list[torch.Tensor]:
    parts = []
    for i in range(3):
        parts += [t[2 * i].permute(2, 3, 1, 0).reshape(-1), t[2 * i + 1].reshape(-1)]     # [oc, ic, kh, kw] -> [(kh, kw, ic), oc]
    return parts + [t[6].reshape(hidden, 64, oh, ow).permute(2, 3, 1, 0).reshape(-1), t[7].reshape(-1)]


def _head_part(wt: torch.Tensor, b: torch.Tensor, hidden: int, n_act: int, ld: int) -> torch.Tensor:
    head = torch.zeros((hidden + 1, ld), dtype=torch.float32)
    head[:hidden, :n_act] = wt.t()
    head[hidden, :n_act] = b
    return head.reshape(-1)


def flat_from_torch(tensors: list[torch.Tensor], c: int, h: int, w: int, n_act: int, hidden: int = 512, device="cuda") -> torch.Tensor:
    """The trunk's eight tensors followed by k heads (weight, bias each), in torch layout (also valid for the matching Adam
    moments) -> trunk | head ... | head.  k = 3 (TIANSHOU_KEYS): the live vector; k = 2: the lagged vector (critic 1, critic 2);
    k = 1: one optimizer's set.  A pure permutation plus the zero padding columns."""
    if len(tensors) not in (10, 12, 14):
        raise ValueError("expected the trunk's eight tensors and one, two or three heads (TIANSHOU_KEYS)")
    t = [x.detach().float().cpu() for x in tensors]
    oh, ow = _conv_hw(h, w)
    ld = (n_act + 31) // 32 * 32
    if tuple(t[6].shape) != (hidden, 64 * oh * ow):
        raise ValueError(f"the added layer must be Linear({64 * oh * ow}, {hidden}), got {tuple(t[6].shape)}")
    parts = _trunk_parts(t, oh, ow, hidden)
    for j in range(8, len(t), 2):
        parts.append(_head_part(t[j], t[j + 1], hidden, n_act, ld))
    return torch.cat(parts).to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, c: int, h: int, w: int, n_act: int, hidden: int = 512) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> the trunk's eight tensors and as many heads as `flat` holds (on flat's device)."""
    oh, ow = _conv_hw(h, w)
    f, ld = 64 * oh * ow, (n_act + 31) // 32 * 32
    out, o = [], 0
    for ic, k, oc in ((c, 8, 32), (32, 4, 64), (64, 3, 64)):
        kk = k * k * ic
        wb = flat[o:o + (kk + 1) * oc].reshape(kk + 1, oc)
        out += [wb[:kk].reshape(k, k, ic, oc).permute(3, 2, 0, 1).contiguous(), wb[kk].clone()]
        o += (kk + 1) * oc
    wb = flat[o:o + (f + 1) * hidden].reshape(f + 1, hidden)
    o += (f + 1) * hidden
    out += [wb[:f].reshape(oh, ow, 64, hidden).permute(3, 2, 0, 1).reshape(hidden, f).contiguous(), wb[f].clone()]
    hd = (hidden + 1) * ld
    if (flat.numel() - o) % hd or not 1 <= (flat.numel() - o) // hd <= 3:
        raise ValueError("flat vector does not hold the trunk and one, two or three heads")
    while o < flat.numel():
        wb = flat[o:o + hd].reshape(hidden + 1, ld)
        o += hd
        out += [wb[:hidden, :n_act].t().contiguous(), wb[hidden, :n_act].clone()]
    return out


# ---- the per-sample kernels on raw arrays (edge tests) ------------------------------------------------------------------
def _f32_2d(x, device) -> torch.Tensor:
    x = torch.as_tensor(x, device=device).to(torch.float32).contiguous()
    if x.dim() != 2 or not 1 <= x.shape[1] <= 64 or x.shape[0] < 1:
        raise ValueError("expected float32 [B, n_act], B >= 1, 1 <= n_act <= 64")
    return x


def _f32_1d(x, device) -> torch.Tensor:
    return torch.as_tensor(x, device=device).to(torch.float32).reshape(-1).contiguous()


def _mk(fill, device):
    if fill is None:
        return lambda *s: torch.empty(s, dtype=torch.float32, device=device)
    return lambda *s: torch.full(s, fill, dtype=torch.float32, device=device)


def _alpha_args(alpha, log_alpha, device):
    """-> (pointer to log_alpha on the device or NULL, the fixed scalar, the tensor kept alive)."""
    if log_alpha is None:
        return None, float(alpha), None
    la = _f32_1d(log_alpha, device)
    if la.numel() != 1:
        raise ValueError("log_alpha must hold one float32")
    return la, 0.0, la


def target_value(logits, q1_old, q2_old, alpha: float = 0.0, log_alpha=None, device="cuda", fill: float | None = None) -> torch.Tensor:
    """sum_j p_j min(q1_old, q2_old)_j + alpha H(p) of float32[B, A] arrays (ts_dsac_cnn_target) -> float32[B].  `log_alpha`
    (one float32, host or device): alpha = exp(log_alpha) is read on the device instead of the scalar."""
    logits, q1_old, q2_old = _f32_2d(logits, device), _f32_2d(q1_old, device), _f32_2d(q2_old, device)
    if logits.shape != q1_old.shape or logits.shape != q2_old.shape:
        raise ValueError("logits, q1_old and q2_old differ in shape")
    la, fixed, _keep = _alpha_args(alpha, log_alpha, logits.device)
    out = _mk(fill, logits.device)(logits.shape[0])
    _lib.check(_lib.load().ts_dsac_cnn_target(_lib.ptr(logits), _lib.ptr(q1_old), _lib.ptr(q2_old), _lib.ptr(la), _lib.f64(fixed),
                                              _lib.i64(logits.shape[0]), _lib.i64(logits.shape[1]), _lib.ptr(out),
                                              _lib.current_stream(logits.device)))
    return out


def critic_terms(q, act, target, weight=None, device="cuda", fill: float | None = None) -> dict:
    """The critic kernels on raw arrays (ts_dsac_cnn_critic) -> {dq [B, ld], td [B], terms [B] = td^2 w, loss [1]}.
    `fill`: value every output buffer holds before the call (a sentinel that must be gone afterwards)."""
    q = _f32_2d(q, device)
    b, a = q.shape
    ld = (a + 31) // 32 * 32
    act = _i64_dev(act, q.device).reshape(-1)
    target = _f32_1d(target, q.device)
    weight = None if weight is None else _f32_1d(weight, q.device)
    if act.numel() != b or target.numel() != b or (weight is not None and weight.numel() != b):
        raise ValueError("q / act / target / weight batch sizes differ")
    mk = _mk(fill, q.device)
    out = {"dq": mk(b, ld), "td": mk(b), "terms": mk(b), "loss": mk(1)}
    _lib.check(_lib.load().ts_dsac_cnn_critic(_lib.ptr(q), _lib.ptr(act), _lib.ptr(target), _lib.ptr(weight), _lib.i64(b), _lib.i64(a),
                                              _lib.ptr(out["dq"]), _lib.ptr(out["td"]), _lib.ptr(out["terms"]), _lib.ptr(out["loss"]),
                                              _lib.current_stream(q.device)))
    return out


def actor_terms(logits, q1, q2, alpha: float = 0.0, log_alpha=None, device="cuda", fill: float | None = None) -> dict:
    """The actor kernels on raw arrays (ts_dsac_cnn_actor) -> {dlogits [B, ld], entropy [B], terms [B] = alpha H + sum_j p_j
    min(q1, q2)_j, loss [1] = -mean(terms)}."""
    logits, q1, q2 = _f32_2d(logits, device), _f32_2d(q1, device), _f32_2d(q2, device)
    if logits.shape != q1.shape or logits.shape != q2.shape:
        raise ValueError("logits, q1 and q2 differ in shape")
    b, a = logits.shape
    ld = (a + 31) // 32 * 32
    la, fixed, _keep = _alpha_args(alpha, log_alpha, logits.device)
    mk = _mk(fill, logits.device)
    out = {"dlogits": mk(b, ld), "entropy": mk(b), "terms": mk(b), "loss": mk(1)}
    _lib.check(_lib.load().ts_dsac_cnn_actor(_lib.ptr(logits), _lib.ptr(q1), _lib.ptr(q2), _lib.ptr(la), _lib.f64(fixed), _lib.i64(b),
                                             _lib.i64(a), _lib.ptr(out["dlogits"]), _lib.ptr(out["entropy"]), _lib.ptr(out["terms"]),
                                             _lib.ptr(out["loss"]), _lib.current_stream(logits.device)))
    return out


class DiscreteSACCnnEngine:
    """State of one DiscreteSAC learner on the Atari trunk on one GPU (hyper-parameters: tianshou_amd.sac.SACConfig): the live
    vector, the lagged vector, three Adam moment pairs (rows of `adam_m` / `adam_v` in SETS order, each trunk | own head),
    log alpha with its moments, the shared step counter."""

    def __init__(self, c: int, h: int, w: int, n_act: int, hidden: int, flat_params: torch.Tensor, cfg: SACConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("DiscreteSACCnnEngine needs parameters on an MI355X (no CPU fallback)")
        self.c, self.h, self.w, self.n_act, self.hidden, self.cfg = c, h, w, n_act, int(hidden), cfg
        self.lay = layout(c, h, w, n_act, self.hidden)
        self.P, self.T, self.Hd = self.lay["total"], self.lay["T"], self.lay["Hd"]
        self.G = self.T + self.Hd                              # one gradient / moment set
        if flat_params.numel() != self.P:
            raise ValueError(f"expected {self.P} parameters, got {flat_params.numel()}")
        self.device = flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        self.params_old = self.lagged_from_live(self.params)
        self.adam_m = torch.zeros((3, self.G), dtype=torch.float32, device=self.device)
        self.adam_v = torch.zeros_like(self.adam_m)
        self.log_alpha = torch.full((1,), cfg.log_alpha0, dtype=torch.float32, device=self.device)
        self.log_alpha_m, self.log_alpha_v = torch.zeros_like(self.log_alpha), torch.zeros_like(self.log_alpha)
        self.adam_step = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def lagged_from_live(self, flat: torch.Tensor) -> torch.Tensor:
        """trunk | critic-1 head | critic-2 head of a live vector (a copy)."""
        return torch.cat([flat[:self.T], flat[self.T + self.Hd:]]).contiguous()

    def _dims(self):
        return (_lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act), _lib.i64(self.hidden))

    def _check_obs(self, obs: torch.Tensor) -> torch.Tensor:
        if tuple(obs.shape[1:]) != (self.h, self.w, self.c) or obs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs must be float32 or uint8 [B, {self.h}, {self.w}, {self.c}] (NHWC)")
        return obs.contiguous()

    def _alpha_ptr(self):
        return _lib.ptr(self.log_alpha if self.cfg.auto_alpha else None)

    @property
    def alpha(self) -> torch.Tensor:
        if self.cfg.auto_alpha:
            return self.log_alpha.exp()
        return torch.full((1,), self.cfg.alpha, dtype=torch.float32, device=self.device)

    # -- DiscreteSACPolicy.forward -------------------------------------------------------------------------
    def policy_forward(self, obs_nhwc: torch.Tensor, params: torch.Tensor | None = None) -> torch.Tensor:
        """-> logits float32[B, n_act] (the input of Categorical(logits=...), discrete_sac.py:73-74)."""
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        out = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        p = self.params if params is None else params
        _lib.check(_lib.load().ts_dsac_cnn_forward(self._ws.handle, _lib.ptr(p), *self._dims(), _lib.ptr(obs_nhwc),
                                                   _u8_flag(obs_nhwc), _lib.i64(b), _lib.ptr(out), _lib.current_stream(self.device)))
        return out

    # -- _target_q_compute_value ------------------------------------------------------------------------------
    def target_q(self, obs_next_nhwc: torch.Tensor) -> torch.Tensor:
        """sum_j p_j min(Q1_old, Q2_old)_j + alpha H(p) on obs_next, p from the live actor -> float32[B]."""
        obs_next_nhwc = self._check_obs(obs_next_nhwc)
        b = obs_next_nhwc.shape[0]
        out = torch.empty(b, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_dsac_cnn_target_q(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), self._alpha_ptr(), _lib.f64(self.cfg.alpha),
            *self._dims(), _lib.ptr(obs_next_nhwc), _u8_flag(obs_next_nhwc), _lib.i64(b), _lib.ptr(out),
            _lib.current_stream(self.device)))
        return out

    # -- _preprocess_batch (ddpg.py:287-301) ---------------------------------------------------------------------
    def preprocess(self, buffer: DeviceReplayBuffer, frames: torch.Tensor, indices, stack_num: int,
                   obs_next_frames: torch.Tensor | None = None) -> torch.Tensor:
        """n-step returns float32[I] of the soft state value, one target pass per batch."""
        calls = []

        def tq_fn(buf, after):
            calls.append(1)
            if len(calls) != 1:
                raise RuntimeError("DiscreteSACCnnEngine.preprocess: one target pass per batch")
            if obs_next_frames is None:
                on = gather_obs_nhwc(frames, buf, buf.next(after), stack_num, as_u8=True)
            else:
                on = gather_obs_nhwc(obs_next_frames, buf, after, stack_num, as_u8=True)
            return self.target_q(on)

        class _B:
            pass

        return compute_nstep_return(_B(), buffer, indices, tq_fn, self.cfg.gamma, self.cfg.n_step).returns.reshape(-1)

    def returns_from_obs_next(self, buffer: DeviceReplayBuffer, indices, obs_next_nhwc: torch.Tensor) -> torch.Tensor:
        """`preprocess` for a caller that already holds the observations `_target_q` reads (buffer[indices_after_n].obs_next):
        target_q + the arithmetic half of compute_nstep_return (algorithm_base.py:793-812) -> float32[I]."""
        return nstep_return_from_target_q(buffer, indices, self.target_q(obs_next_nhwc), self.cfg.gamma,
                                          self.cfg.n_step).reshape(-1)

    def wait_td(self, stream: torch.cuda.Stream) -> None:
        """`stream` waits for the new batch.weight of the last `update_with_batch`, not for the rest of the update."""
        _lib.check(_lib.load().ts_dqn_wait_td(self._ws.handle, C.c_void_p(stream.cuda_stream)))

    # -- _update_with_batch ------------------------------------------------------------------------------------
    def update_with_batch(self, obs_nhwc, act, returns, weight=None, grads_out: torch.Tensor | None = None, apply: bool = True):
        """-> (stats float32[5] device = {actor_loss, critic1_loss, critic2_loss, alpha, alpha_loss},
        weight float32[B] = (td1 + td2) / 2).  `cfg` is read at every call.  apply=False computes the three gradients only, at
        the unchanged parameters, into grads_out float32[3, T + Hd] (SETS order) and leaves every piece of state untouched."""
        cfg = self.cfg
        if not apply and grads_out is None:
            raise ValueError("apply=False computes the gradients only: pass grads_out")
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        act = _i64_dev(act, self.device).reshape(-1)
        returns = _f32_1d(returns, self.device)
        weight = None if weight is None else _f32_1d(weight, self.device)
        if b < 1 or act.numel() != b or returns.numel() != b or (weight is not None and weight.numel() != b):
            raise ValueError("obs / act / returns / weight batch sizes differ (returns: float32 [B])")
        if grads_out is not None and (grads_out.numel() != 3 * self.G or grads_out.dtype != torch.float32 or not grads_out.is_cuda
                                      or not grads_out.is_contiguous()):
            raise ValueError(f"grads_out must be a contiguous float32 device tensor of 3 x {self.G} elements")
        if apply:
            self.adam_step += 1
        stats = torch.empty(5, dtype=torch.float32, device=self.device)
        w_out = torch.empty(b, dtype=torch.float32, device=self.device)
        hp = cfg.to_c()
        if not apply:
            hp.actor_lr = hp.critic_lr = hp.alpha_lr = -1.0
        _lib.check(_lib.load().ts_dsac_cnn_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
            _lib.ptr(self.log_alpha), _lib.ptr(self.log_alpha_m), _lib.ptr(self.log_alpha_v), _lib.i64(max(self.adam_step, 1)),
            *self._dims(), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.ptr(act), _lib.ptr(returns), _lib.ptr(weight), _lib.i64(b),
            C.byref(hp), _lib.ptr(stats), _lib.ptr(w_out), _lib.ptr(grads_out), _lib.current_stream(self.device)))
        return stats, w_out
