"""The discriminator half of GAIL on the MI355X engine; the PPO half is tianshou_amd.ppo / ppo_wide unchanged.

Mirrors, on device tensors:
    GAIL._preprocess_batch       tianshou/algorithm/imitation/gail.py:203-206   rew = -logsigmoid(-D(obs, act))
    GAIL._update_with_batch      gail.py:220-235                                 the discriminator steps before the PPO update
The discriminator is `ContinuousCritic(preprocess_net=Net(..., concat=True))` on concat(obs, act) or any bare `Net` trunk with
one output: a critic in the flat layout of ts_net_layout with obs_dim := obs_dim + act_dim.  One call runs every
discriminator step of an update (pack, forward, logistic loss, reverse pass, clip + optimizer step) without a host
synchronisation; the per-step statistics stay on the device until the caller reads them.
There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .ppo_wide import net_flat_from_tensors, net_flat_to_tensors

ROUTES = {"auto": 0, "per_layer": 1, "one_launch": 2}
OPTIMIZERS = {"adam": 0, "rmsprop": 1}


@dataclass
class GAILConfig:
    """gail.py:43 `disc_update_num` and the discriminator optimizer's fields (tianshou/algorithm/optim.py: AdamOptimizerFactory /
    RMSpropOptimizerFactory; `max_grad_norm` as Optimizer.step applies it)."""

    disc_update_num: int = 4
    optimizer: str = "adam"
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    rms_alpha: float = 0.99
    rms_momentum: float = 0.0
    rms_centered: bool = False
    max_grad_norm: float | None = None
    route: str = "auto"

    def __post_init__(self):
        if self.disc_update_num < 1:
            raise ValueError("disc_update_num must be >= 1")
        if self.optimizer not in OPTIMIZERS:
            raise NotImplementedError(f"discriminator optimizer must be one of {sorted(OPTIMIZERS)}, got {self.optimizer!r}")
        if self.route not in ROUTES:
            raise ValueError(f"route must be one of {sorted(ROUTES)}, got {self.route!r}")


def chunking(n: int, disc_update_num: int) -> tuple[int, int]:
    """-> (bsz, steps) of gail.py:224-225 (`Batch.split(bsz, merge_last=True)`): bsz = n // disc_update_num, n // bsz steps, the
    last one takes the remainder.  The reference fails an assertion where bsz is 0; here that is a ValueError."""
    bsz = int(n) // int(disc_update_num)
    if bsz < 1:
        raise ValueError(f"GAIL: the batch has {n} transitions, fewer than disc_update_num = {disc_update_num}")
    return bsz, int(n) // bsz


def loss(logits: torch.Tensor, n_pi: int):
    """ts_gail_loss: the loss kernel alone on a float32 device vector of logits, policy rows first -> (stats float32[3] =
    {disc_loss, acc_pi, acc_exp}, d loss / d logits)."""
    logits = logits.detach().to(torch.float32).reshape(-1).contiguous()
    n_exp = logits.numel() - int(n_pi)
    d, stats = torch.empty_like(logits), torch.empty(3, dtype=torch.float32, device=logits.device)
    ws = _lib.default_workspace(logits.device.index or 0)
    _lib.check(_lib.load().ts_gail_loss(ws.handle, _lib.ptr(logits), _lib.i64(n_pi), _lib.i64(n_exp), _lib.ptr(d), _lib.ptr(stats),
                                        _lib.current_stream(logits.device)))
    return stats, d


class GAILDiscriminator:
    """The discriminator, its optimizer state and a device copy of the expert buffer's obs / act."""

    def __init__(self, obs_dim: int, act_dim: int, hidden, activation: str, disc: torch.Tensor, expert_obs, expert_act,
                 cfg: GAILConfig):
        if not disc.is_cuda:
            raise RuntimeError("GAILDiscriminator needs parameters on an MI355X (no CPU fallback)")
        self.obs_dim, self.act_dim, self.cfg = int(obs_dim), int(act_dim), cfg
        self.hidden, self.activation = [int(h) for h in hidden], activation
        self._net = _lib.NetDesc.make(self.obs_dim + self.act_dim, self.hidden, activation)
        out = (C.c_int64 * 3)()
        _lib.check(_lib.load().ts_net_layout(C.byref(self._net), _lib.i64(1), out))
        self.k0, self.count = int(out[0]), int(out[2])
        if disc.numel() != self.count:
            raise ValueError(f"the flat discriminator vector has {disc.numel()} entries, ts_net_layout gives {self.count}")
        self.device = disc.device
        self.disc = disc.detach().float().contiguous().clone()
        self.state_m, self.state_v = torch.zeros_like(self.disc), torch.zeros_like(self.disc)
        self.optim_step = 0
        self.set_expert(expert_obs, expert_act)
        self._ws = _lib.default_workspace(self.device.index or 0)

    # -- converters (nn.Linear-layout tensor lists <-> the flat vector) -------------------------------------------------------
    @staticmethod
    def flat_from_tensors(t, obs_dim: int, act_dim: int, hidden, device="cuda") -> torch.Tensor:
        return net_flat_from_tensors(list(t), obs_dim + act_dim, [int(h) for h in hidden], None, device)

    def to_tensors(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        return net_flat_to_tensors(self.disc if flat is None else flat, self.obs_dim + self.act_dim, self.hidden, 1, False)

    @classmethod
    def from_module(cls, module, obs_dim: int, act_dim: int, expert_obs, expert_act, cfg: GAILConfig, device="cuda"):
        """`module`: ContinuousCritic(preprocess_net=Net(..., concat=True)) or a bare Net with one output."""
        hidden, activation, tensors = describe_module(module, obs_dim + act_dim)
        return cls(obs_dim, act_dim, hidden, activation, cls.flat_from_tensors(tensors, obs_dim, act_dim, hidden, device),
                   expert_obs, expert_act, cfg)

    def to_module(self, module) -> None:
        """Writes the engine's parameters into `module`'s tensors (the order `describe_module` reads them in)."""
        _, _, tensors = describe_module(module, self.obs_dim + self.act_dim)
        with torch.no_grad():
            for dst, src in zip(tensors, self.to_tensors()):
                dst.copy_(src.to(dst.device).reshape(dst.shape))

    # -- data ------------------------------------------------------------------------------------------------------------------
    def _f32(self, x, shape=None) -> torch.Tensor:
        t = torch.as_tensor(x).to(device=self.device, dtype=torch.float32)
        return (t.reshape(shape) if shape is not None else t).contiguous()

    def _i64(self, x) -> torch.Tensor:
        return torch.as_tensor(x).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()

    def set_expert(self, expert_obs, expert_act) -> None:
        self.expert_obs = self._f32(expert_obs).reshape(-1, self.obs_dim)
        self.expert_act = self._f32(expert_act).reshape(self.expert_obs.shape[0], self.act_dim)
        if self.expert_obs.shape[0] < 1:
            raise ValueError("GAIL: the expert buffer is empty")

    # -- the two passes --------------------------------------------------------------------------------------------------------
    def reward(self, obs, act, want_logits: bool = False, route: str | None = None):
        """gail.py:205 -> rew float32[B] (and the logits)."""
        obs = self._f32(obs).reshape(-1, self.obs_dim)
        b = obs.shape[0]
        act = self._f32(act, (b, self.act_dim))
        rew = torch.empty(b, dtype=torch.float32, device=self.device)
        logits = torch.empty(b, dtype=torch.float32, device=self.device) if want_logits else None
        _lib.check(_lib.load().ts_gail_reward(
            self._ws.handle, _lib.ptr(self.disc), C.byref(self._net), _lib.i64(self.act_dim), _lib.ptr(obs), _lib.ptr(act), _lib.i64(b),
            _lib.ptr(rew), _lib.ptr(logits), C.c_int32(ROUTES[route or self.cfg.route]), _lib.current_stream(self.device)))
        return (rew, logits) if want_logits else rew

    def disc_update(self, obs, act, perm, exp_index, grad_out: torch.Tensor | None = None, apply: bool = True,
                    route: str | None = None) -> torch.Tensor:
        """gail.py:220-235 with the draws as inputs -> stats float32[steps, 3] = {disc_loss, acc_pi, acc_exp} per step, on the
        device.  `perm`: the split permutation of the N rows of obs / act; `exp_index`: steps * bsz rows of the expert copy.
        apply=False: gradients and statistics only (grad_out receives the last step's gradient)."""
        cfg = self.cfg
        obs = self._f32(obs).reshape(-1, self.obs_dim)
        n = obs.shape[0]
        act = self._f32(act, (n, self.act_dim))
        bsz, steps = chunking(n, cfg.disc_update_num)
        perm, exp_index = self._i64(perm), self._i64(exp_index)
        if perm.numel() != n or exp_index.numel() != steps * bsz:
            raise ValueError(f"GAIL: perm must have {n} entries and exp_index {steps} x {bsz}")
        if grad_out is not None and (grad_out.numel() != self.count or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the discriminator's size")
        stats = torch.empty((steps, 3), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_gail_disc_steps(
            self._ws.handle, _lib.ptr(self.disc), _lib.ptr(self.state_m), _lib.ptr(self.state_v), _lib.i64(self.optim_step + 1),
            C.byref(self._net), _lib.i64(self.act_dim), _lib.ptr(obs), _lib.ptr(act), _lib.ptr(perm), _lib.i64(n),
            _lib.ptr(self.expert_obs), _lib.ptr(self.expert_act), _lib.i64(self.expert_obs.shape[0]), _lib.ptr(exp_index),
            _lib.i64(bsz), C.c_int32(OPTIMIZERS[cfg.optimizer]), _lib.f64(cfg.lr if apply else -1.0), _lib.f64(cfg.betas[0]),
            _lib.f64(cfg.betas[1]), _lib.f64(cfg.eps), _lib.f64(cfg.weight_decay), _lib.f64(cfg.rms_alpha),
            _lib.f64(cfg.rms_momentum), C.c_int32(int(cfg.rms_centered)), _lib.f64(cfg.max_grad_norm or 0.0),
            C.c_int32(ROUTES[route or cfg.route]), _lib.ptr(stats), _lib.ptr(grad_out), _lib.current_stream(self.device)))
        if apply:
            self.optim_step += steps               # (after the call: a refused argument leaves the counter alone)
        return stats


def describe_module(module, in_dim: int):
    """-> (hidden widths, activation name, [w1, b1, ..., w_head, b_head]) of a discriminator module, or raises naming what was
    found.  Accepted: a critic-like module with `preprocess` (a Net / MLP trunk) and `last` (a linear head of one output), or a
    bare Net / MLP whose last Linear has one output."""
    linears, acts = [], set()
    for m in module.modules():
        if isinstance(m, torch.nn.LayerNorm) or "Norm" in type(m).__name__:
            raise NotImplementedError(f"GAIL discriminator: normalisation layers are not supported (found {type(m).__name__})")
        if isinstance(m, torch.nn.Linear):
            linears.append(m)
        elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)):
            acts.add("tanh" if isinstance(m, torch.nn.Tanh) else "relu")
        elif len(list(m.children())) == 0 and not isinstance(m, (torch.nn.Identity, torch.nn.Flatten)):
            raise NotImplementedError(f"GAIL discriminator: only Linear layers with tanh / ReLU are supported (found {type(m).__name__})")
    if len(linears) < 2:
        raise NotImplementedError(f"GAIL discriminator: a Net trunk with a linear head is needed (found {len(linears)} Linear layers)")
    if len(acts) > 1:
        raise NotImplementedError("GAIL discriminator: one activation for all hidden layers is supported (found tanh and ReLU)")
    if linears[-1].out_features != 1:
        raise NotImplementedError(f"GAIL discriminator: the head must have one output (found {linears[-1].out_features})")
    if linears[0].in_features != in_dim:
        raise ValueError(f"GAIL discriminator: the first layer takes {linears[0].in_features} inputs, obs_dim + act_dim is {in_dim}")
    for a, b in zip(linears[:-1], linears[1:]):
        if a.out_features != b.in_features:
            raise NotImplementedError("GAIL discriminator: the Linear layers do not form one chain")
    if any(l.bias is None for l in linears):
        raise NotImplementedError("GAIL discriminator: Linear layers without bias are not supported")
    hidden = [l.out_features for l in linears[:-1]]
    tensors = [p for l in linears for p in (l.weight, l.bias)]
    return hidden, (acts.pop() if acts else "none"), tensors
