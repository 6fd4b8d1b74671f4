"""What the six Q-learning engines on vector observations share on the host (dqn_mlp, qrdqn_mlp, c51_mlp, rainbow_mlp, iqn_mlp,
fqf_mlp): the refusals of a family under its own name and envelope (`Family`), the `[K + 1, N]` block converters, the walk over a
Linear / ReLU `Sequential`, and the engine state with the bookkeeping around the one library call of an update (`VecQEngine`).  A new
member of the family subclasses VecQEngine and keeps a Family; it copies none of this.

Not here: rainbow_mlp's converters and stream walk (a NoisyLinear layer is a mu block and a sigma block, and its tensors come as
mu_W, sigma_W, mu_bias, sigma_bias: not a list of (weight, bias) blocks), and the fraction streams of iqn_mlp (tianshou_amd.iqn's).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .buffer import _i64_dev, gather_rows
from .drqn import gather_stacked_obs_pair
from .returns import nstep_coefficients, nstep_indices

MAX_BATCH = 4096
_NET_ATTRS = ("model", "use_dueling", "softmax", "num_atoms")


class Family:
    """A family member's display name ("QRDQN MLP") and ENVELOPE string: every refusal reads `<who>: <reason>; supported: <envelope>`."""

    def __init__(self, who: str, envelope: str):
        self.who, self.envelope = who, envelope

    def refuse(self, reason: str, part: str = "") -> NotImplementedError:
        return NotImplementedError(f"{self.who}{' ' + part if part else ''}: {reason}; supported: {self.envelope}")

    # -- the envelope ------------------------------------------------------------------------------------------------------------
    def in_range(self, name: str, value: int, lo: int, hi: int, note: str = "") -> None:
        """obs_dim, num_atoms, num_cosines, num_fractions, the sample sizes."""
        if not lo <= value <= hi:
            raise self.refuse(f"{name} = {value} is outside [{lo}, {hi}]{note}")

    def count(self, n: int, what: str, lo: int, hi: int) -> None:
        """The trunk depth ("hidden layers"), the depth of `last`, the actions."""
        if not lo <= n <= hi:
            raise self.refuse(f"{n} {what} ({lo} .. {hi})")

    def widths(self, widths, hi: int, what: str = "hidden width") -> None:
        bad = [w for w in widths if w % 32 or not 32 <= w <= hi]
        if bad:
            raise self.refuse(f"{what} {bad[0]} is no multiple of 32 in [32, {hi}]")

    def layout(self, fn: str, desc, batch: int, **slots) -> dict:
        """The library's `fn`(desc, batch, out) -> {count, lds_bytes, workspace_bytes} = out[0 .. 2] and `slots` (name=index, which
        may also move one of the three); NotImplementedError when the library refuses the shape (a tile that does not fit the LDS)."""
        out = (C.c_int64 * 16)()
        try:
            _lib.check(getattr(_lib.load(), fn)(desc, _lib.i64(batch), out))
        except _lib.EngineError as e:
            if e.code != _lib.TS_ERR_UNSUPPORTED:
                raise
            raise self.refuse(str(e)) from None
        return {k: int(out[i]) for k, i in {"count": 0, "lds_bytes": 1, "workspace_bytes": 2, **slots}.items()}

    # -- modules -------------------------------------------------------------------------------------------------------------------
    def require_net(self, net, extra=(), need: str = "a Net is needed", hint: str = "") -> None:
        """`net` has what a Net has (common.py:286-341), and `extra`."""
        for name in (*_NET_ATTRS[:1], *extra, *_NET_ATTRS[1:]):
            if not hasattr(net, name):
                raise self.refuse(f"{need} (found {type(net).__name__} without `{name}`{hint})")

    def chain(self, seq, part: str = ""):
        """Sequential(Linear, ReLU, Linear, ReLU, ...(, Linear)) -> ([hidden Linear], last Linear or None)."""
        mods = list(seq.children())
        for j, m in enumerate(mods):
            if j % 2 == 0 and (not isinstance(m, torch.nn.Linear) or m.bias is None):
                raise self.refuse(f"Linear layers with bias followed by ReLU only, no norm_layer (found {type(m).__name__})", part)
            if j % 2 == 1 and not isinstance(m, torch.nn.ReLU):
                raise self.refuse(f"the activation must be ReLU, with no norm_layer before it (found {type(m).__name__})", part)
        lin = mods[0::2]
        return (lin[:-1], lin[-1]) if len(mods) % 2 else (lin, None)

    def same_parameters(self, module, keys, what: str, trainable_only: bool = False) -> None:
        have = [k for k, p in module.named_parameters() if p.requires_grad or not trainable_only]
        if have != keys:
            raise self.refuse(f"the model's parameters {have} are not {what} {keys}")

    # -- flat vector <-> tensors: `blocks` = [(state-dict prefix, K, N)] in flat order, `order` = the prefixes in state_dict() order --
    def flat_from_torch(self, tensors, blocks, order, device) -> torch.Tensor:
        t = list(tensors)
        if len(t) != 2 * len(order):
            raise ValueError(f"{self.who}: expected {2 * len(order)} tensors, got {len(t)}")
        given = {p: (t[2 * i], t[2 * i + 1]) for i, p in enumerate(order)}
        parts = []
        for prefix, k, n in blocks:
            w, b = given[prefix]
            if tuple(w.shape) != (n, k) or b.numel() != n:
                raise ValueError(f"{self.who}: {prefix} must be Linear({k}, {n}), got weight {tuple(w.shape)} and {b.numel()} biases")
            parts += [w.detach().float().cpu().t().reshape(-1), b.detach().float().cpu().reshape(-1)]
        return torch.cat(parts).to(device).contiguous()

    def flat_to_torch(self, flat: torch.Tensor, blocks, order) -> list[torch.Tensor]:
        f, off, got = flat.detach(), 0, {}
        for prefix, k, n in blocks:
            got[prefix] = (f[off:off + k * n].reshape(k, n).t().contiguous(), f[off + k * n:off + (k + 1) * n].clone())
            off += (k + 1) * n
        if off != f.numel():
            raise ValueError(f"{self.who}: the flat vector has {f.numel()} entries, the layout {off}")
        return [x for p in order for x in got[p]]


class VecQEngine:
    """State of one learner on one GPU: flat parameters, lagged copy, Adam moments, the two counters, the workspace.  A subclass sets
    `FAMILY`, validates its layers and hands them over with their desc array and parameter count; its `update_with_batch` is
    `_batch_args`, its own checks, one library call (with `_sync_now()` and `_adam_arg(apply)`), then `_stepped(apply)`: no counter
    moves before `_lib.check` has returned, so a refused argument leaves the lagged network and the counters alone."""

    FAMILY: Family

    def _require_device(self, *flats) -> None:
        if not all(f.is_cuda for f in flats):
            raise RuntimeError(f"{type(self).__name__} needs parameters on an MI355X (no CPU fallback)")

    def __init__(self, layers, desc, count: int, flat_params: torch.Tensor, cfg):
        self._require_device(flat_params)
        self.layers, self._d, self.P, self.cfg = layers, desc, count, cfg
        self.obs_dim = layers[0]
        if flat_params.numel() != self.P:
            raise ValueError(f"expected {self.P} parameters, got {flat_params.numel()}")
        self.device = flat_params.device
        self.params = flat_params.detach().float().contiguous().clone()
        self.params_old = self.params.clone() if cfg.target_update_freq > 0 else None    # dqn.py:240-246
        self.adam_m, self.adam_v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.adam_step = 0
        self.iter = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _obs(self, obs) -> torch.Tensor:
        obs = torch.as_tensor(obs, device=self.device).to(torch.float32)
        if obs.dim() < 2 or obs[0].numel() != self.obs_dim:
            raise ValueError(f"obs must be [B, {self.obs_dim}]")
        obs = obs.reshape(obs.shape[0], self.obs_dim).contiguous()
        if not 1 <= obs.shape[0] <= MAX_BATCH:
            raise NotImplementedError(f"{self.FAMILY.who}: a batch of {obs.shape[0]} rows (1 .. {MAX_BATCH})")
        return obs

    def _obs_pair(self, buffer, obs_rows, indices, n_step: int, obs_next_rows=None, pair=None, stack_num: int = 1):
        """-> (rows at `indices`, rows n_step transitions later), both from one launch (drqn.gather_stacked_obs_pair with stack_num
        1); rows of another layout go through the index kernels."""
        if stack_num != 1:
            raise NotImplementedError(f"{self.FAMILY.who}: frame stacking is not supported (stack_num must be 1)")
        if pair is None:
            pair = gather_stacked_obs_pair(obs_rows, buffer, indices, n_step, 1, obs_next_rows)
        if pair is None:
            idx = _i64_dev(indices, buffer.device).reshape(-1)
            after = idx if n_step == 1 else nstep_indices(buffer, idx, n_step)
            nxt = gather_rows(obs_rows, buffer.next(after)) if obs_next_rows is None else gather_rows(obs_next_rows, after)
            pair = (gather_rows(obs_rows, idx), nxt)
        return pair

    def _preprocess(self, buffer, obs_rows, indices, stack_num, obs_next_rows, pair, coef, *target_args):
        """`preprocess_with_obs` of the members whose target is a network pass: -> (batch.obs float32[I, obs_dim],
        self.target_returns(obs n_step later, the n-step coefficients, *target_args))."""
        pair = self._obs_pair(buffer, obs_rows, indices, self.cfg.n_step, obs_next_rows, pair, stack_num)
        if coef is None:
            coef = nstep_coefficients(buffer, indices, self.cfg.gamma, self.cfg.n_step)
        return self._obs(pair[0]), self.target_returns(pair[1], coef, *target_args)

    def _batch_args(self, b: int, act, weight, grad_out):
        """-> (act int64[b], weight float32[b] or None) on the device; ValueError for a wrong length or a wrong `grad_out`."""
        act = _i64_dev(act, self.device).reshape(-1)
        if act.numel() != b:
            raise ValueError(f"act must hold {b} entries")
        if weight is not None:
            weight = torch.as_tensor(weight, device=self.device).to(torch.float32).reshape(-1).contiguous()
            if weight.numel() != b:
                raise ValueError("weight length mismatch")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the model's size")
        return act, weight

    def _sync_now(self) -> bool:
        """This call synchronises the lagged network: every target_update_freq-th one, the first included (dqn.py:283-285)."""
        return self.params_old is not None and self.iter % self.cfg.target_update_freq == 0

    def _adam_arg(self, apply: bool):
        return _lib.i64(self.adam_step + 1 if apply else max(self.adam_step, 1))

    def _stepped(self, apply: bool) -> None:
        self.iter += 1
        if apply:
            self.adam_step += 1

    def apply_gradient(self, grad: torch.Tensor) -> None:
        """clip_grad_norm_ + Adam on a flat gradient of the model (algorithm_base.py:496-500)."""
        cfg = self.cfg
        self.adam_step += 1
        _lib.check(_lib.load().ts_adam_step(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), _lib.ptr(grad),
            _lib.i64(self.P), _lib.i64(self.adam_step), _lib.f64(cfg.lr), _lib.f64(cfg.betas[0]),
            _lib.f64(cfg.betas[1]), _lib.f64(cfg.adam_eps), _lib.f64(cfg.max_grad_norm or 0.0),
            _lib.current_stream(self.device)))
