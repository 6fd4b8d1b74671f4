"""Behaviour cloning (vanilla imitation learning) on the MI355X engine: the loss alone on an actor network.

Mirrors, on device tensors:
    ImitationPolicy.forward                                   tianshou/algorithm/imitation/imitation_base.py:85-105
    ImitationLearningAlgorithmMixin._imitation_update         imitation_base.py:109-127
        discrete:    F.nll_loss(F.log_softmax(logits, -1), act)      (softmax cross-entropy over all actions)
        continuous:  F.mse_loss(max_action * tanh(head), act)        (ContinuousActorDeterministic, continuous.py:70-85)
followed by `Algorithm.Optimizer.step` (algorithm_base.py:484-500: global-norm clip, Adam).  Three routes:
    BCDQNetEngine                     DQNet(c, h, w, n_act) on NHWC u8 / f32 frames (examples/offline/atari_il.py); dqn's flat layout
    BCMlpEngine(mode="discrete")      Net(obs, n_act, hidden_sizes) (test/discrete/test_a2c_with_il.py); dsac's network layout
    BCMlpEngine(mode="continuous")    ContinuousActorDeterministic over a Net (examples/offline/d4rl_il.py); td3's actor layout
State of every engine: flat `params`, `adam_m`, `adam_v`, `adam_step`.  No layout is introduced here.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib, dsac
from . import td3 as T
from .buffer import _i64_dev
from .dqn import DQNHParams, _u8_flag, flat_from_torch, flat_to_torch, param_count  # noqa: F401  (the DQNet route's layout is dqn's)
from .sac import MLPTrunk, mlp_layout

DISCRETE, CONTINUOUS = "discrete", "continuous"
_MODE_C = {DISCRETE: 0, CONTINUOUS: 1}          # TS_BC_DISCRETE / TS_BC_CONTINUOUS (include/tsengine.h)
MAX_ACT = 64                                    # cross-entropy: one lane of a wavefront per action
MAX_ACT_DIM = 32                                # the MLP actor head's columns


@dataclass
class BCConfig:
    """Adam (optim.py:89-110) and the clip of `Algorithm.Optimizer`; `max_action` is read by the continuous route only."""

    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None
    max_action: float = 1.0


def ce_loss(logits: torch.Tensor, act: torch.Tensor, n_act: int | None = None):
    """ts_bc_ce_loss on raw arrays: logits float32[B, ld] (the first `n_act` columns are real, default all), act int64[B] ->
    (loss float32[1], dlogits float32[B, ld])."""
    b, ld = logits.shape
    a = ld if n_act is None else int(n_act)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ce_loss_into(logits, act, a, loss, dlogits)
    return loss, dlogits


def ce_loss_into(logits: torch.Tensor, act: torch.Tensor, n_act: int, loss: torch.Tensor, dlogits: torch.Tensor) -> None:
    """`ce_loss` into caller-owned outputs (any float32 device storage of at least 1 / B * ld elements)."""
    if not logits.is_cuda or logits.dtype != torch.float32 or not logits.is_contiguous() or act.dtype != torch.int64:
        raise ValueError("ce_loss: contiguous float32 device logits and int64 actions")
    b, ld = logits.shape
    _lib.check(_lib.load().ts_bc_ce_loss(_lib.ptr(logits), _lib.i64(ld), _lib.ptr(act), _lib.i64(b), _lib.i64(n_act),
                                         _lib.ptr(loss), _lib.ptr(dlogits), _lib.current_stream(logits.device)))


def mse_loss(head: torch.Tensor, act_data: torch.Tensor, max_action: float = 1.0):
    """ts_bc_mse_loss on raw arrays: head float32[B, 32] (pre-tanh), act_data float32[B, act_dim] -> (loss float32[1],
    dhead float32[B, 32])."""
    loss = torch.empty(1, dtype=torch.float32, device=head.device)
    dhead = torch.empty_like(head)
    mse_loss_into(head, act_data, max_action, loss, dhead)
    return loss, dhead


def mse_loss_into(head: torch.Tensor, act_data: torch.Tensor, max_action: float, loss: torch.Tensor, dhead: torch.Tensor) -> None:
    if not head.is_cuda or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[1] != 32 \
            or act_data.dtype != torch.float32 or not act_data.is_contiguous() or act_data.shape[0] != head.shape[0]:
        raise ValueError("mse_loss: contiguous float32 device head [B, 32] and act_data [B, act_dim]")
    _lib.check(_lib.load().ts_bc_mse_loss(_lib.ptr(head), _lib.ptr(act_data), _lib.i64(head.shape[0]), _lib.i64(act_data.shape[1]),
                                          _lib.f64(max_action), _lib.ptr(loss), _lib.ptr(dhead), _lib.current_stream(head.device)))


class _BCEngine:
    """What the two engines share: the state vectors and the `grad_out` check."""

    def _init_state(self, flat_params: torch.Tensor, count: int, cfg: BCConfig) -> None:
        if not flat_params.is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs parameters on an MI355X (no CPU fallback)")
        if flat_params.numel() != count:
            raise ValueError(f"expected {count} parameters, got {flat_params.numel()}")
        self.P, self.cfg, self.device = count, cfg, flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.adam_step = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _check_grad_out(self, grad_out) -> None:
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32 or not grad_out.is_cuda):
            raise ValueError(f"grad_out must be a float32 device tensor of {self.P} elements")


class BCDQNetEngine(_BCEngine):
    """State of one behaviour-cloning learner on DQNet on one GPU (`update_with_batch` on ts_bc_dqnet_update)."""

    def __init__(self, c: int, h: int, w: int, n_act: int, flat_params: torch.Tensor, cfg: BCConfig):
        self.c, self.h, self.w, self.n_act = int(c), int(h), int(w), int(n_act)
        self._init_state(flat_params, param_count(c, h, w, n_act), cfg)

    @classmethod
    def from_module(cls, net: torch.nn.Module, c: int, h: int, w: int, cfg: BCConfig, device="cuda") -> "BCDQNetEngine":
        """`net`: a DQNet (its ten parameters in state_dict order)."""
        t = [p.detach() for p in net.parameters()]
        n_act = int(t[8].shape[0])
        return cls(c, h, w, n_act, flat_from_torch(t, c, h, w, n_act, device), cfg)

    def to_module(self, net: torch.nn.Module) -> None:
        with torch.no_grad():
            for p, t in zip(net.parameters(), flat_to_torch(self.params, self.c, self.h, self.w, self.n_act)):
                p.copy_(t.reshape(p.shape))

    def _check_obs(self, obs_nhwc: torch.Tensor) -> torch.Tensor:
        if tuple(obs_nhwc.shape[1:]) != (self.h, self.w, self.c) or obs_nhwc.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs must be float32 or uint8 [B, {self.h}, {self.w}, {self.c}] (NHWC)")
        return obs_nhwc.contiguous()

    def forward(self, obs_nhwc: torch.Tensor):
        """ImitationPolicy.forward, discrete branch -> (logits float32[B, A], act int64[B] = the first maximum)."""
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_dqn_forward(
            self._ws.handle, _lib.ptr(self.params), _lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act),
            _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc), _lib.i64(b), _lib.ptr(q), _lib.ptr(act), _lib.current_stream(self.device)))
        return q, act

    def update_with_batch(self, obs_nhwc, act, grad_out: torch.Tensor | None = None, apply: bool = True) -> torch.Tensor:
        """-> loss float32[1] device tensor.  apply=False: gradient only (no Adam step, no counter)."""
        cfg = self.cfg
        obs_nhwc = self._check_obs(obs_nhwc)
        b = obs_nhwc.shape[0]
        act = _i64_dev(act, self.device).reshape(-1)
        if act.numel() != b:
            raise ValueError("obs / act batch sizes differ")
        self._check_grad_out(grad_out)
        if apply:
            self.adam_step += 1
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = DQNHParams(cfg.lr if apply else -1.0, cfg.betas[0], cfg.betas[1], cfg.adam_eps, -1.0, cfg.max_grad_norm or 0.0)
        _lib.check(_lib.load().ts_bc_dqnet_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), _lib.i64(max(self.adam_step, 1)),
            _lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), _lib.i64(self.n_act), _lib.ptr(obs_nhwc), _u8_flag(obs_nhwc),
            _lib.ptr(act), _lib.i64(b), C.byref(hp), _lib.ptr(loss), _lib.ptr(grad_out), _lib.current_stream(self.device)))
        return loss


def mlp_param_count(mode: str, obs_dim: int, n_out: int, hidden: int, depth: int) -> int:
    if mode == CONTINUOUS:
        return mlp_layout(obs_dim, hidden, depth, 32)[1][-1]
    return dsac.layout(obs_dim, n_out, hidden, depth)["count"]


def mlp_flat_from_torch(mode: str, t: list[torch.Tensor], obs_dim: int, n_out: int, hidden: int, device="cuda") -> torch.Tensor:
    """[w1, b1, ..., wd, bd, w_head, b_head] in nn.Linear layout (also valid for Adam moments) -> the route's flat vector:
    td3's actor layout (continuous) or dsac's network layout (discrete)."""
    if mode == CONTINUOUS:
        return T.actor_flat_from_torch(t, obs_dim, n_out, device, hidden=hidden)
    return dsac.net_flat_from_torch(t, obs_dim, n_out, hidden, device)


def mlp_flat_to_torch(mode: str, flat: torch.Tensor, obs_dim: int, n_out: int, hidden: int, sizes=None, depth: int | None = None):
    if mode == CONTINUOUS:
        return T.actor_flat_to_torch(flat, obs_dim, n_out, hidden, sizes=sizes, depth=depth)
    return dsac.net_flat_to_torch(flat, obs_dim, n_out, hidden, sizes=sizes, depth=depth)


class BCMlpEngine(_BCEngine):
    """State of one behaviour-cloning learner on an MLP actor on one GPU (`update_with_batch` on ts_bc_mlp_update).
    mode "discrete": Net(obs_dim, n_out, [hidden] * depth), 2 <= n_out <= 64 logits.  mode "continuous":
    ContinuousActorDeterministic over Net(obs_dim, [hidden] * depth), n_out <= 32 action dimensions, cfg.max_action."""

    def __init__(self, mode: str, obs_dim: int, n_out: int, flat_params: torch.Tensor, cfg: BCConfig, hidden: int = 256,
                 depth: int = 2, activation: str = "relu"):
        if mode not in _MODE_C:
            raise ValueError("mode must be 'discrete' or 'continuous'")
        limit = MAX_ACT_DIM if mode == CONTINUOUS else MAX_ACT
        if not (1 if mode == CONTINUOUS else 2) <= n_out <= limit:
            raise NotImplementedError(f"BCMlpEngine({mode}): the head holds {'1' if mode == CONTINUOUS else '2'} .. {limit} outputs, "
                                      f"got {n_out}")
        self.mode, self.obs_dim, self.n_out = mode, int(obs_dim), int(n_out)
        self.hidden, self.depth, self.activation = int(hidden), int(depth), activation
        self._trunk = MLPTrunk(hidden, depth, activation)
        self._init_state(flat_params, mlp_param_count(mode, obs_dim, n_out, self.hidden, self.depth), cfg)

    @classmethod
    def from_module(cls, mode: str, tensors: list[torch.Tensor], cfg: BCConfig, hidden: int | None = None,
                    activation: str = "relu", device="cuda") -> "BCMlpEngine":
        """`tensors`: [w1, b1, ..., wd, bd, w_head, b_head] of the actor, in nn.Linear layout."""
        from . import widths as W

        t = [p.detach() for p in tensors]
        depth = W.depth_of(t, 1)
        hidden = int(hidden or W.engine_hidden([W.layer_widths(t, 1)]))
        obs_dim, n_out = int(t[0].shape[1]), int(t[-1].shape[0])
        if mode == DISCRETE and not 2 <= n_out <= MAX_ACT or mode == CONTINUOUS and n_out > MAX_ACT_DIM:
            raise NotImplementedError(f"BCMlpEngine({mode}): unsupported head width {n_out}")
        return cls(mode, obs_dim, n_out, mlp_flat_from_torch(mode, t, obs_dim, n_out, hidden, device), cfg, hidden, depth, activation)

    def to_module(self, tensors: list[torch.Tensor]) -> None:
        from . import widths as W

        sizes = W.layer_widths([p.detach() for p in tensors], 1)
        with torch.no_grad():
            for p, t in zip(tensors, mlp_flat_to_torch(self.mode, self.params, self.obs_dim, self.n_out, self.hidden, sizes=sizes)):
                p.copy_(t.reshape(p.shape))

    def _f32(self, x, shape) -> torch.Tensor:
        t = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
        if tuple(t.shape[1:]) != shape:
            raise ValueError(f"expected rows of shape {shape}, got {tuple(t.shape)}")
        return t

    def forward(self, obs):
        """ImitationPolicy.forward: discrete -> (logits float32[B, A], act int64[B] = the first maximum); continuous -> act
        float32[B, act_dim] = max_action * tanh(head)."""
        obs = self._f32(obs, (self.obs_dim,))
        b = obs.shape[0]
        if self.mode == CONTINUOUS:
            act = torch.empty((b, self.n_out), dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().ts_td3_policy_forward(
                self._ws.handle, _lib.ptr(self.params), _lib.ptr(obs), _lib.i64(b), _lib.i64(self.obs_dim), _lib.i64(self.n_out),
                C.byref(self._trunk), _lib.f64(self.cfg.max_action), _lib.ptr(act), _lib.current_stream(self.device)))
            return act
        logits = torch.empty((b, self.n_out), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_bc_mlp_forward(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(obs), _lib.i64(b), _lib.i64(self.obs_dim), _lib.i64(self.n_out),
            C.byref(self._trunk), _lib.ptr(logits), _lib.ptr(act), _lib.current_stream(self.device)))
        return logits, act

    def update_with_batch(self, obs, act, grad_out: torch.Tensor | None = None, apply: bool = True) -> torch.Tensor:
        """-> loss float32[1] device tensor.  `act`: int64[B] (discrete) or float32[B, act_dim] (continuous)."""
        cfg = self.cfg
        obs = self._f32(obs, (self.obs_dim,))
        b = obs.shape[0]
        if self.mode == CONTINUOUS:
            act = self._f32(act, (self.n_out,))
        else:
            act = _i64_dev(act, self.device).reshape(-1)
        if act.shape[0] != b:
            raise ValueError("obs / act batch sizes differ")
        self._check_grad_out(grad_out)
        if apply:
            self.adam_step += 1
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_bc_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), _lib.i64(max(self.adam_step, 1)),
            _lib.ptr(obs), _lib.ptr(act), _lib.i64(b), _lib.i64(self.obs_dim), _lib.i64(self.n_out), C.byref(self._trunk),
            C.c_int(_MODE_C[self.mode]), _lib.f64(cfg.max_action), _lib.f64(cfg.lr if apply else -1.0), _lib.f64(cfg.betas[0]),
            _lib.f64(cfg.betas[1]), _lib.f64(cfg.adam_eps), _lib.f64(cfg.max_grad_norm or 0.0), _lib.ptr(loss), _lib.ptr(grad_out),
            _lib.current_stream(self.device)))
        return loss
