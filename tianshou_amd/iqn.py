"""IQN learn() path on the MI355X engine (Implicit Quantile Networks, arXiv:1806.06923, on the Atari trunk).

Mirrors, on device tensors:
    ImplicitQuantileNetwork.forward       tianshou/utils/net/discrete.py:200-216 (DQNet(features_only=True) trunk, hidden [512])
    CosineEmbeddingNetwork.forward        discrete.py:144-160
    IQNPolicy.forward                     tianshou/algorithm/modelfree/iqn.py:72-100
    QRDQN._target_q                       modelfree/qrdqn.py:94-106 (n-step via tianshou_amd.returns, whole quantile rows)
    IQN._update_with_batch                iqn.py:156-183 (+ periodic hard sync dqn.py:277-285)
There is no CPU path: every function calls libtsengine.so and raises when it is missing.

Fractions.  The reference draws tau = torch.rand(B, sample_size) inside the model.  Every method here takes the fractions as
optional tensors (float32 [B, N]); when they are None the engine draws them itself with ts_uniform_fill_f32 from
(cfg.seed, self.tau_counter) -- Philox, NOT torch's generator stream -- and advances the counter, which is part of the engine
state (`extra_state` / `load_extra_state`): a resumed run continues the stream instead of replaying it.

Parameter layout (ts_iqn_layout): conv1 | conv2 | conv3 (the DQN engine's matrices) | [We; be] [n_cos + 1, F] |
[W1; b1] [F + 1, 512] | [W2; b2] [513, ld]; F in (h, w, c) order, ld = n_act rounded up to a multiple of 32 with zero
padding columns.  `flat_from_torch` / `flat_to_torch` convert the twelve state-dict tensors of the reference net.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .buffer import DeviceReplayBuffer, _i64_dev
from .distq import DistQHParams
from .dqn import _u8_flag, gather_obs_nhwc
from .lagged import full_parameter_update
from .returns import compute_nstep_return, nstep_return_from_target_q

# state_dict keys of ImplicitQuantileNetwork(preprocess_net=DQNet(features_only=True), hidden_sizes=[512]), in order
TIANSHOU_KEYS = ["preprocess.net.0.weight", "preprocess.net.0.bias", "preprocess.net.2.weight", "preprocess.net.2.bias",
                 "preprocess.net.4.weight", "preprocess.net.4.bias", "last.model.0.weight", "last.model.0.bias",
                 "last.model.2.weight", "last.model.2.bias", "embed_model.net.0.weight", "embed_model.net.0.bias"]
HIDDEN = 512


def param_count(c: int, h: int, w: int, n_act: int, n_cos: int = 64) -> int:
    lib = _lib.load()
    lib.ts_iqn_param_count.restype = C.c_int64
    lib.ts_iqn_param_count.argtypes = [C.c_int64] * 5
    n = int(lib.ts_iqn_param_count(c, h, w, n_act, n_cos))
    if n < 0:
        raise ValueError("unsupported IQN network (1 <= n_act <= 64, num_cosines = 64, observation >= 36 x 36)")
    return n


def layout(c: int, h: int, w: int, n_act: int, n_cos: int = 64) -> dict:
    """-> {F, ld, total, off: int64[7] = starts of conv1, conv2, conv3, embedding, fc1, fc2 and the end}."""
    out = (C.c_int64 * 9)()
    _lib.check(_lib.load().ts_iqn_layout(_lib.i64(c), _lib.i64(h), _lib.i64(w), _lib.i64(n_act), _lib.i64(n_cos), out))
    v = [int(x) for x in out]
    return {"F": v[0], "ld": v[1], "total": v[2], "off": np.array(v[3:9] + [v[2]], np.int64)}


def _conv_hw(h: int, w: int) -> tuple[int, int]:
    for k, s in ((8, 4), (4, 2), (3, 1)):
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return h, w


def flat_from_torch(tensors: list[torch.Tensor], c: int, h: int, w: int, n_act: int, n_cos: int = 64,
                    device="cuda") -> torch.Tensor:
    """The twelve tensors of TIANSHOU_KEYS in torch layout (also valid for the matching Adam moments) -> the flat vector."""
    if len(tensors) != 12:
        raise ValueError("expected the twelve state-dict tensors of ImplicitQuantileNetwork (TIANSHOU_KEYS)")
    t = [x.detach().float().cpu() for x in tensors]
    oh, ow = _conv_hw(h, w)
    f, ld = 64 * oh * ow, (n_act + 31) // 32 * 32
    parts = []
    for i in range(3):
        parts += [t[2 * i].permute(2, 3, 1, 0).reshape(-1), t[2 * i + 1].reshape(-1)]     # [oc, ic, kh, kw] -> [(kh, kw, ic), oc]
    we, be = t[10], t[11]                                                                  # [F, n_cos], [F]; F in (c, h, w) order
    parts += [we.reshape(64, oh, ow, n_cos).permute(3, 1, 2, 0).reshape(-1), be.reshape(64, oh, ow).permute(1, 2, 0).reshape(-1)]
    parts += [t[6].reshape(HIDDEN, 64, oh, ow).permute(2, 3, 1, 0).reshape(-1), t[7].reshape(-1)]
    head = torch.zeros((HIDDEN + 1, ld), dtype=torch.float32)
    head[:HIDDEN, :n_act] = t[8].t()
    head[HIDDEN, :n_act] = t[9]
    parts.append(head.reshape(-1))
    flat = torch.cat(parts)
    assert flat.numel() == (8 * 8 * c + 1) * 32 + 513 * 64 + 577 * 64 + (n_cos + 1) * f + (f + 1) * HIDDEN + (HIDDEN + 1) * ld
    return flat.to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, c: int, h: int, w: int, n_act: int, n_cos: int = 64) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> twelve tensors in torch layout, TIANSHOU_KEYS order (on flat's device)."""
    oh, ow = _conv_hw(h, w)
    f, ld = 64 * oh * ow, (n_act + 31) // 32 * 32
    out, o = [], 0
    for ic, k, oc in ((c, 8, 32), (32, 4, 64), (64, 3, 64)):
        kk = k * k * ic
        wb = flat[o:o + (kk + 1) * oc].reshape(kk + 1, oc)
        out += [wb[:kk].reshape(k, k, ic, oc).permute(3, 2, 0, 1).contiguous(), wb[kk].clone()]
        o += (kk + 1) * oc
    emb = flat[o:o + (n_cos + 1) * f].reshape(n_cos + 1, f)
    o += (n_cos + 1) * f
    we = emb[:n_cos].reshape(n_cos, oh, ow, 64).permute(3, 1, 2, 0).reshape(f, n_cos).contiguous()
    be = emb[n_cos].reshape(oh, ow, 64).permute(2, 0, 1).reshape(f).contiguous()
    wb = flat[o:o + (f + 1) * HIDDEN].reshape(f + 1, HIDDEN)
    o += (f + 1) * HIDDEN
    out += [wb[:f].reshape(oh, ow, 64, HIDDEN).permute(3, 2, 0, 1).reshape(HIDDEN, f).contiguous(), wb[f].clone()]
    wb = flat[o:o + (HIDDEN + 1) * ld].reshape(HIDDEN + 1, ld)
    out += [wb[:HIDDEN, :n_act].t().contiguous(), wb[HIDDEN, :n_act].clone()]
    return out + [we, be]


def uniform_fractions(n: int, seed: int, counter: int, device="cuda") -> torch.Tensor:
    """float32[n] in [0, 1) from the engine's own Philox stream at (seed, counter) -- ts_uniform_fill_f32."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    _lib.check(_lib.load().ts_uniform_fill_f32(_lib.ptr(out), _lib.i64(n), C.c_uint64(int(seed) & (2**64 - 1)),
                                               C.c_uint64(int(counter) & (2**64 - 1)), _lib.current_stream(out.device)))
    return out


ROUTES = {"default": 0, "fused": 1, "unfused": 2}          # TS_IQN_ROUTE_*


def embed_mul(tau: torch.Tensor, feat: torch.Tensor, we_be: torch.Tensor, out: torch.Tensor | None = None,
              route: str = "default") -> torch.Tensor:
    """x[b * N + n, :] = feat[b, :] * relu(cos(tau[b, n] * pi * (1 .. 64)) @ We + be) -- the embedding kernel on its own
    (`out`: a preallocated float32 [B * N, F])."""
    b, n = tau.shape
    f = feat.shape[1]
    x = torch.empty((b * n, f), dtype=torch.float32, device=feat.device) if out is None else out
    if tuple(x.shape) != (b * n, f) or x.dtype != torch.float32:
        raise ValueError(f"out must be float32 [{b * n}, {f}]")
    ws = _lib.default_workspace(feat.device.index or 0)
    _lib.check(_lib.load().ts_iqn_embed_mul(ws.handle, _lib.ptr(tau), _lib.ptr(feat), _lib.ptr(we_be), _lib.i64(b), _lib.i64(n),
                                            _lib.i64(f), _lib.i64(we_be.shape[0] - 1), C.c_int(ROUTES[route]), _lib.ptr(x),
                                            _lib.current_stream(feat.device)))
    return x


def embed_mul_backward(tau: torch.Tensor, feat: torch.Tensor, we_be: torch.Tensor, dx: torch.Tensor, out=None,
                       route: str = "default"):
    """-> (dfeat [B, F] masked by feat > 0, [d We; d be] [65, F]) of embed_mul for the upstream gradient dx [B * N, F]
    (`out`: a preallocated pair of that shape)."""
    b, n = tau.shape
    f = feat.shape[1]
    dfeat, dwe = (torch.empty_like(feat), torch.empty_like(we_be)) if out is None else out
    if dfeat.shape != feat.shape or dwe.shape != we_be.shape or tuple(dx.shape) != (b * n, f):
        raise ValueError("embed_mul_backward: shapes of dx / out do not match tau, feat and we_be")
    ws = _lib.default_workspace(feat.device.index or 0)
    _lib.check(_lib.load().ts_iqn_embed_mul_backward(ws.handle, _lib.ptr(tau), _lib.ptr(feat), _lib.ptr(we_be), _lib.ptr(dx),
                                                     _lib.i64(b), _lib.i64(n), _lib.i64(f), _lib.i64(we_be.shape[0] - 1),
                                                     C.c_int(ROUTES[route]), _lib.ptr(dfeat), _lib.ptr(dwe), _lib.current_stream(feat.device)))
    return dfeat, dwe


@dataclass
class IQNConfig:
    """Hyper-parameters of the reference IQNPolicy / IQN (iqn.py:21-154) + Adam (optim.py:89-110)."""

    n_cos: int = 64
    sample_size: int = 32             # evaluation forward
    online_sample_size: int = 8       # N: training forward of the online net
    target_sample_size: int = 8       # N': forward of the lagged net
    gamma: float = 0.99
    n_step: int = 1
    target_update_freq: int = 0
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None
    seed: int = 0                     # key of the engine's own fraction stream

    def to_c(self, grad_only: bool = False) -> DistQHParams:
        return DistQHParams(-1.0 if grad_only else self.lr, self.betas[0], self.betas[1], self.adam_eps,
                            self.max_grad_norm or 0.0, 0.0, 0.0)


class IQNEngine:
    """State of one IQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters (the fraction counter
    included)."""

    def __init__(self, c: int, h: int, w: int, n_act: int, flat_params: torch.Tensor, cfg: IQNConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("IQNEngine needs parameters on an MI355X (no CPU fallback)")
        for name in ("sample_size", "online_sample_size", "target_sample_size"):
            if not 2 <= getattr(cfg, name) <= 64:
                raise ValueError(f"{name} must be in [2, 64]")
        self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
        self.P = param_count(c, h, w, n_act, cfg.n_cos)
        if flat_params.numel() != self.P:
            raise ValueError(f"expected {self.P} parameters, got {flat_params.numel()}")
        self.device = flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        self.params_old = self.params.clone() if cfg.target_update_freq > 0 else None    # dqn.py:240-246
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.adam_step = 0
        self.iter = 0
        self.tau_counter = 0
        self.last_tau = None              # the fractions of the last forward / update_with_batch (iqn.py:99 `taus`)
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _dims(self):
        return (_lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act), _lib.i64(self.cfg.n_cos))

    def _check_obs(self, obs: torch.Tensor) -> torch.Tensor:
        if tuple(obs.shape[1:]) != (self.h, self.w, self.c) or obs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs must be float32 or uint8 [B, {self.h}, {self.w}, {self.c}] (NHWC)")
        return obs.contiguous()

    # -- fractions --------------------------------------------------------------------------------------
    def draw(self, b: int, n: int) -> torch.Tensor:
        """torch.rand(b, n) of the engine's own stream; advances the counter."""
        tau = uniform_fractions(b * n, self.cfg.seed, self.tau_counter, self.device).reshape(b, n)
        self.tau_counter += 1
        return tau

    def _tau(self, tau, b: int, n: int | None) -> torch.Tensor:
        if tau is None:
            return self.draw(b, n)
        tau = torch.as_tensor(tau, device=self.device).to(torch.float32).contiguous()
        if tau.dim() != 2 or tau.shape[0] != b or not 2 <= tau.shape[1] <= 64 or (n is not None and tau.shape[1] != n):
            raise ValueError(f"fractions must be float32 [{b}, {n if n is not None else 'N'}], 2 <= N <= 64")
        return tau

    def extra_state(self) -> dict:
        """Counters a checkpoint must carry beside the tensors: a resumed run continues the fraction stream."""
        return {"tau_seed": int(self.cfg.seed), "tau_counter": int(self.tau_counter), "iter": int(self.iter),
                "adam_step": int(self.adam_step)}

    def load_extra_state(self, state: dict) -> None:
        self.tau_counter = int(state["tau_counter"])
        self.cfg.seed = int(state.get("tau_seed", self.cfg.seed))       # the stream is (seed, counter): both travel
        self.iter = int(state.get("iter", self.iter))
        self.adam_step = int(state.get("adam_step", self.adam_step))

    # -- policy forward -------------------------------------------------------------------------------
    def forward(self, obs_nhwc: torch.Tensor, tau=None, sample_size: int | None = None, params: torch.Tensor | None = None,
                want_logits: bool = True):
        """-> (logits float32[B, A, N] or None, q float32[B, A], act int64[B] = argmax_a q); the fractions used are
        `self.last_tau`.  sample_size defaults to cfg.sample_size (IQNPolicy.forward outside training)."""
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        tau = self._tau(tau, b, sample_size if tau is not None else (sample_size or self.cfg.sample_size))
        n = tau.shape[1]
        logits = torch.empty((b, self.n_act, n), dtype=torch.float32, device=self.device) if want_logits else None
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        p = self.params if params is None else params
        _lib.check(_lib.load().ts_iqn_forward(
            self._ws.handle, _lib.ptr(p), *self._dims(), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.i64(b), _lib.ptr(tau),
            _lib.i64(n), _lib.ptr(logits), _lib.ptr(q), _lib.ptr(act), _lib.current_stream(self.device)))
        self.last_tau = tau
        return logits, q, act

    def next_dist(self, obs_next_nhwc: torch.Tensor, tau_online=None, tau_target=None) -> torch.Tensor:
        """The lagged net's quantiles of the online net's greedy action -> float32[B, N'] ([B, N] without a lagged net).
        Draw order as the reference's (qrdqn.py:99-105): the online net's fractions first."""
        obs_next_nhwc = self._check_obs(obs_next_nhwc)
        b = obs_next_nhwc.shape[0]
        tau_online = self._tau(tau_online, b, None if tau_online is not None else self.cfg.online_sample_size)
        two = self.params_old is not None
        if two:
            tau_target = self._tau(tau_target, b, None if tau_target is not None else self.cfg.target_sample_size)
        n_out = tau_target.shape[1] if two else tau_online.shape[1]
        out = torch.empty((b, n_out), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_iqn_next_dist(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), *self._dims(), _lib.ptr(obs_next_nhwc),
            _u8_flag(obs_next_nhwc), _lib.i64(b), _lib.ptr(tau_online), _lib.i64(tau_online.shape[1]),
            _lib.ptr(tau_target if two else None), _lib.i64(n_out), _lib.ptr(out), _lib.current_stream(self.device)))
        return out

    # -- _preprocess_batch (dqn.py:257-275 with QRDQN._target_q) ------------------------------------------
    def preprocess(self, buffer: DeviceReplayBuffer, frames: torch.Tensor, indices, stack_num: int,
                   obs_next_frames: torch.Tensor | None = None, tau_online=None, tau_target=None) -> torch.Tensor:
        """n-step returns float32[I, N'] of the next-state quantiles."""

        calls = []

        def tq_fn(buf, after):
            # compute_nstep_return asks for the target once per batch (algorithm_base.py:793): one pair of fraction tensors --
            # given ones would be reused and drawn ones would advance the counter twice if that ever changed
            calls.append(1)
            assert len(calls) == 1, "IQNEngine.preprocess: one target pass per batch"
            if obs_next_frames is None:
                on = gather_obs_nhwc(frames, buf, buf.next(after), stack_num, as_u8=True)
            else:
                on = gather_obs_nhwc(obs_next_frames, buf, after, stack_num, as_u8=True)
            return self.next_dist(on, tau_online, tau_target)

        class _B:
            pass

        return compute_nstep_return(_B(), buffer, indices, tq_fn, self.cfg.gamma, self.cfg.n_step).returns

    def returns_from_obs_next(self, buffer: DeviceReplayBuffer, indices, obs_next_nhwc: torch.Tensor, tau_online=None,
                              tau_target=None) -> torch.Tensor:
        """`preprocess` for a caller that already holds the observations `_target_q` reads (buffer[indices_after_n].obs_next):
        next_dist + the arithmetic half of compute_nstep_return (algorithm_base.py:793-812) -> float32[I, N']."""
        return nstep_return_from_target_q(buffer, indices, self.next_dist(obs_next_nhwc, tau_online, tau_target),
                                          self.cfg.gamma, self.cfg.n_step)

    def wait_td(self, stream: torch.cuda.Stream) -> None:
        """`stream` waits for the new priorities and the loss of the last `update_with_batch`, not for its backward pass and
        Adam step (ts_dqn_wait_td; see dqn.ReplayStream)."""
        _lib.check(_lib.load().ts_dqn_wait_td(self._ws.handle, C.c_void_p(stream.cuda_stream)))

    # -- _update_with_batch ------------------------------------------------------------------------------
    def update_with_batch(self, obs_nhwc, act, returns, weight=None, tau=None, grad_out: torch.Tensor | None = None,
                          apply: bool = True):
        """-> (loss float32[1] device tensor, new batch.weight float32[B]).  returns float32[B, N']; tau float32[B, N]
        (None: drawn, N = cfg.online_sample_size)."""
        cfg = self.cfg
        if apply:
            if self.params_old is not None and self.iter % cfg.target_update_freq == 0:    # dqn.py:283-285
                full_parameter_update(self.params_old, self.params)
            self.iter += 1
            self.adam_step += 1
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        tau = self._tau(tau, b, None if tau is not None else cfg.online_sample_size)
        act = _i64_dev(act, self.device).reshape(-1)
        returns = torch.as_tensor(returns, dtype=torch.float32, device=self.device).contiguous()
        if weight is not None:
            weight = torch.as_tensor(weight, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if (act.numel() != b or returns.dim() != 2 or returns.shape[0] != b or not 2 <= returns.shape[1] <= 64
                or (weight is not None and weight.numel() != b)):
            raise ValueError("obs / act / returns / weight batch sizes differ (returns: float32 [B, N'], 2 <= N' <= 64)")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32):
            raise ValueError(f"grad_out must be float32[{self.P}]")
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_iqn_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
            _lib.i64(max(self.adam_step, 1)), *self._dims(), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.ptr(act),
            _lib.ptr(returns), _lib.i64(returns.shape[1]), _lib.ptr(tau), _lib.i64(tau.shape[1]), _lib.ptr(weight), _lib.i64(b),
            C.byref(hp), _lib.ptr(prio), _lib.ptr(loss), _lib.ptr(grad_out), _lib.current_stream(self.device)))
        self.last_tau = tau
        return loss, prio
