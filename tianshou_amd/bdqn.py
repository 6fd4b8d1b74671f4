"""Branching Dueling Q-Network (arXiv 1711.08946) on the MI355X engine.

Mirrors, on device tensors:
    BranchingNet.forward                 tianshou/utils/net/common.py:658-674     q = v + adv - mean_a adv
    BDQN._target_q / _compute_return     tianshou/algorithm/modelfree/bdqn.py:155-195   1-step, mean over the branches
    BDQN._update_with_batch              bdqn.py:206-224                           lagged sync, loss, one optimizer step
The model is one flat vector (ts_bdqn_layout): the common chain, the "fan" block -- the first layers of `value` and of all D
branches side by side, one GEMM -- and the D + 1 heads.  `dims` = (obs_dim, common_hidden, value_hidden, action_hidden, D, A,
activation) describes it everywhere; value_hidden / action_hidden are a width or 0 (no hidden layer).
Deviation from the reference: at B = 1 with D > 1 the reference's `.squeeze()` drops the batch axis and the branch mean is
skipped; the engine computes ret[b] = rew[b] + gamma mean_d q_eval[b, d, a*] (1 - end[b]) at every B.
Actions outside [0, A) are clamped into it.  There is no CPU path: every function calls libtsengine.so and raises when it is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib

OPTIMIZERS = {"adam": 0, "rmsprop": 1}
ACTIVATIONS = {"tanh": 0, "relu": 1}
MAX_HIDDEN = 7                                     # TS_NET_MAX_HIDDEN
MAX_BRANCHES, MAX_ACTIONS, MAX_WIDTH = 32, 64, 1024        # TS_BDQN_MAX_BRANCHES, TS_BDQN_MAX_ACTIONS
ENVELOPE = (f"BranchingNet with 1 .. {MAX_HIDDEN} common hidden layers, at most one hidden layer in value_hidden_sizes and in "
            f"action_hidden_sizes, widths 1 .. {MAX_WIDTH}, ReLU or tanh, no norm_layer, 1 <= num_branches <= {MAX_BRANCHES}, "
            f"1 <= action_per_branch <= {MAX_ACTIONS}")


@dataclass
class BDQNConfig:
    """bdqn.py:109-153 and the optimizer's fields (tianshou/algorithm/optim.py: AdamOptimizerFactory / RMSpropOptimizerFactory;
    `max_grad_norm` as Optimizer.step applies it)."""

    gamma: float = 0.99
    target_update_freq: int = 0
    is_double: bool = True
    optimizer: str = "adam"
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    weight_decay: float = 0.0
    rms_alpha: float = 0.99
    rms_momentum: float = 0.0
    rms_centered: bool = False
    max_grad_norm: float | None = None

    def __post_init__(self):
        if self.optimizer not in OPTIMIZERS:
            raise NotImplementedError(f"BDQN optimizer must be one of {sorted(OPTIMIZERS)}, got {self.optimizer!r}")


def _pad32(n: int) -> int:
    return (int(n) + 31) // 32 * 32


def make_dims(obs_dim, common_hidden, value_hidden, action_hidden, num_branches, action_per_branch, activation="relu") -> tuple:
    """The model description every function here takes; raises NotImplementedError outside the envelope."""
    ch = tuple(int(h) for h in common_hidden)
    hv, ha, d, a = int(value_hidden or 0), int(action_hidden or 0), int(num_branches), int(action_per_branch)
    if not 1 <= len(ch) <= MAX_HIDDEN:
        raise NotImplementedError(f"BDQN: common_hidden_sizes must have 1 .. {MAX_HIDDEN} layers, got {len(ch)}; supported: {ENVELOPE}")
    if any(not 1 <= w <= MAX_WIDTH for w in ch) or not 0 <= hv <= MAX_WIDTH or not 0 <= ha <= MAX_WIDTH:
        raise NotImplementedError(f"BDQN: hidden widths {ch}, {hv}, {ha} are outside 1 .. {MAX_WIDTH}; supported: {ENVELOPE}")
    if not 1 <= d <= MAX_BRANCHES or not 1 <= a <= MAX_ACTIONS:
        raise NotImplementedError(f"BDQN: num_branches = {d}, action_per_branch = {a}; supported: {ENVELOPE}")
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f"BDQN: activation {activation!r}; supported: {ENVELOPE}")
    return (int(obs_dim), ch, hv, ha, d, a, activation)


def layout(dims):
    """-> (blocks, where, count): blocks = [(offset, K_pad, columns)], where = {state-dict prefix: (block, first column, k, n)},
    count = floats of the flat vector (ts_bdqn_layout gives the same)."""
    obs_dim, ch, hv, ha, d_n, a_n, _ = dims
    blocks, where, o = [], {}, 0

    def add(kp, cols):
        nonlocal o
        blocks.append((o, kp, cols))
        o += (kp + 1) * cols
        return len(blocks) - 1

    k = obs_dim
    for i, n in enumerate(ch):
        where[f"common.model.{2 * i}"] = (add(_pad32(k), _pad32(n)), 0, k, n)
        k = n
    hc = k
    if hv or ha:
        fan = add(_pad32(hc), _pad32(hv) + (d_n * _pad32(ha) if ha else 0))
        if hv:
            where["value.model.0"] = (fan, 0, hc, hv)
        if ha:
            for d in range(d_n):
                where[f"branches.{d}.model.0"] = (fan, _pad32(hv) + d * _pad32(ha), hc, ha)
    kv = hv or hc
    where[f"value.model.{2 if hv else 0}"] = (add(_pad32(kv), 32), 0, kv, 1)
    ka = ha or hc
    for d in range(d_n):
        where[f"branches.{d}.model.{2 if ha else 0}"] = (add(_pad32(ka), _pad32(a_n)), 0, ka, a_n)
    return blocks, where, o


def state_keys(dims) -> list[str]:
    """The parameter names of a BranchingNet of this shape, in state_dict() order (common.py:616-656)."""
    _, ch, hv, ha, d_n, _, _ = dims
    pre = [f"common.model.{2 * i}" for i in range(len(ch))]
    pre += ["value.model.0"] + (["value.model.2"] if hv else [])
    for d in range(d_n):
        pre += [f"branches.{d}.model.0"] + ([f"branches.{d}.model.2"] if ha else [])
    return [f"{p}.{s}" for p in pre for s in ("weight", "bias")]


def flat_from_torch(tensors, *dims_and_device) -> torch.Tensor:
    """[w, b, ...] in `state_keys` order (nn.Linear layout; parameters or their moments) -> the flat vector."""
    *dims, device = dims_and_device
    dims = tuple(dims)
    keys, t = state_keys(dims), list(tensors)
    if len(t) != len(keys):
        raise ValueError(f"BDQN: expected {len(keys)} tensors, got {len(t)}")
    blocks, where, count = layout(dims)
    flat = torch.zeros(count, dtype=torch.float32)
    views = [flat[o:o + (kp + 1) * cols].view(kp + 1, cols) for o, kp, cols in blocks]
    for key, x in zip(keys, t):
        prefix, kind = key.rsplit(".", 1)
        bi, c0, k, n = where[prefix]
        x = x.detach().float().cpu()
        if kind == "weight":
            if tuple(x.shape) != (n, k):
                raise ValueError(f"BDQN: {key} must be {(n, k)}, got {tuple(x.shape)}")
            views[bi][:k, c0:c0 + n] = x.t()
        else:
            if x.numel() != n:
                raise ValueError(f"BDQN: {key} must have {n} entries, got {x.numel()}")
            views[bi][blocks[bi][1], c0:c0 + n] = x.reshape(-1)
    return flat.to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, *dims) -> list[torch.Tensor]:
    blocks, where, count = layout(tuple(dims))
    f = flat.detach()
    if f.numel() != count:
        raise ValueError(f"BDQN: the flat vector has {f.numel()} entries, the layout {count}")
    out = []
    for key in state_keys(tuple(dims)):
        prefix, kind = key.rsplit(".", 1)
        bi, c0, k, n = where[prefix]
        o, kp, cols = blocks[bi]
        blk = f[o:o + (kp + 1) * cols].view(kp + 1, cols)
        out.append(blk[:k, c0:c0 + n].t().contiguous() if kind == "weight" else blk[kp, c0:c0 + n].clone())
    return out


def padding_mask(dims, device="cpu") -> torch.Tensor:
    """bool[count]: True at the padding entries of the flat vector (they are zero and stay zero)."""
    blocks, where, count = layout(dims)
    mask = torch.ones(count, dtype=torch.bool)
    for bi, c0, k, n in where.values():
        o, kp, cols = blocks[bi]
        v = mask[o:o + (kp + 1) * cols].view(kp + 1, cols)
        v[:k, c0:c0 + n] = False
        v[kp, c0:c0 + n] = False
    return mask.to(device)


def describe_model(model) -> dict:
    """-> {dims, keys} of a BranchingNet-shaped module (`common`, `value`, `branches`, `num_branches`, `action_per_branch`;
    common.py:574-656), or raises NotImplementedError naming what is supported."""
    for name in ("common", "value", "branches", "num_branches", "action_per_branch"):
        if not hasattr(model, name):
            raise NotImplementedError(f"BDQN: a BranchingNet is needed (found {type(model).__name__} without `{name}`); supported: {ENVELOPE}")
    acts = set()

    def linears(net, who):
        out = []
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                if m.bias is None:
                    raise NotImplementedError(f"BDQN {who}: Linear layers without bias are not supported; supported: {ENVELOPE}")
                out.append(m)
            elif isinstance(m, (torch.nn.ReLU, torch.nn.Tanh)):
                acts.add("relu" if isinstance(m, torch.nn.ReLU) else "tanh")
            elif "Norm" in type(m).__name__:
                raise NotImplementedError(f"BDQN {who}: norm_layer is not supported (found {type(m).__name__}); supported: {ENVELOPE}")
            elif len(list(m.children())) == 0 and not isinstance(m, (torch.nn.Identity, torch.nn.Flatten)):
                raise NotImplementedError(f"BDQN {who}: only Linear layers with ReLU / tanh (found {type(m).__name__}); supported: {ENVELOPE}")
        return out

    common = linears(model.common, "common")
    value = linears(model.value, "value")
    branches = [linears(b, f"branches[{d}]") for d, b in enumerate(model.branches)]
    if not common or not value or not branches:
        raise NotImplementedError(f"BDQN: common, value and at least one branch need a Linear layer; supported: {ENVELOPE}")
    if len(value) > 2 or any(len(b) > 2 for b in branches):
        raise NotImplementedError(f"BDQN: value / branch MLPs with {len(value) - 1} / {max(len(b) for b in branches) - 1} hidden "
                                  f"layers; supported: {ENVELOPE}")
    if len(acts) != 1:
        raise NotImplementedError(f"BDQN: one activation, ReLU or tanh, behind every hidden layer (found {sorted(acts) or 'none'}); "
                                  f"supported: {ENVELOPE}")
    shapes = {tuple((l.in_features, l.out_features) for l in b) for b in branches}
    if len(shapes) != 1 or len(branches) != int(model.num_branches) or branches[0][-1].out_features != int(model.action_per_branch):
        raise NotImplementedError(f"BDQN: the branches must be num_branches equal MLPs ending in action_per_branch outputs; supported: {ENVELOPE}")
    hc = common[-1].out_features
    if value[0].in_features != hc or branches[0][0].in_features != hc or value[-1].out_features != 1:
        raise NotImplementedError(f"BDQN: value and branches must read the common net's {hc} outputs, value ending in 1; supported: {ENVELOPE}")
    dims = make_dims(common[0].in_features, [l.out_features for l in common], value[0].out_features if len(value) == 2 else 0,
                     branches[0][0].out_features if len(branches[0]) == 2 else 0, len(branches), model.action_per_branch, acts.pop())
    keys = state_keys(dims)
    have = [k for k, _ in model.named_parameters()]
    if have != keys:
        raise NotImplementedError(f"BDQN: the model's parameters {have} are not a BranchingNet's {keys}; supported: {ENVELOPE}")
    return {"dims": dims, "keys": keys}


def target(q_sel, q_eval, rew, end, gamma: float) -> torch.Tensor:
    """ts_bdqn_target on raw tables: q_sel / q_eval float32[B, D, A], rew [B], end [B] (non-zero = stop) -> ret float32[B]."""
    q_sel, q_eval = q_sel.detach().float().contiguous(), q_eval.detach().float().contiguous()
    b, d, a = q_sel.shape
    if q_eval.shape != q_sel.shape:
        raise ValueError("BDQN target: q_sel and q_eval must both be [B, D, A]")
    dev = q_sel.device
    rew = torch.as_tensor(rew).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    end = (torch.as_tensor(end).to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
    if rew.numel() != b or end.numel() != b:
        raise ValueError("BDQN target: rew and end must have B entries")
    ret = torch.empty(b, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ts_bdqn_target(_lib.ptr(q_sel), _lib.ptr(q_eval), _lib.ptr(rew), _lib.ptr(end), _lib.i64(b), _lib.i64(d),
                                          _lib.i64(a), _lib.f64(gamma), _lib.ptr(ret), _lib.current_stream(dev)))
    return ret


def loss(q, act, ret, weight=None, want_dq: bool = True):
    """ts_bdqn_loss on a raw q float32[B, D, A], act int64[B, D], ret [B], weight [B] or None -> (loss float32[1], prio [B],
    dq [B, D, A] or None)."""
    q = q.detach().float().contiguous()
    b, d, a = q.shape
    dev = q.device
    act = torch.as_tensor(act).to(device=dev, dtype=torch.int64).reshape(b, d).contiguous()
    ret = torch.as_tensor(ret).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if ret.numel() != b:
        raise ValueError("BDQN loss: ret must have B entries")
    if weight is not None:
        weight = torch.as_tensor(weight).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if weight.numel() != b:
            raise ValueError("BDQN loss: weight must have B entries")
    out, prio = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev)
    dq = torch.empty_like(q) if want_dq else None
    ws = _lib.default_workspace(dev.index or 0)
    _lib.check(_lib.load().ts_bdqn_loss(ws.handle, _lib.ptr(q), _lib.ptr(act), _lib.ptr(ret), _lib.ptr(weight), _lib.i64(b), _lib.i64(d),
                                        _lib.i64(a), _lib.ptr(out), _lib.ptr(prio), _lib.ptr(dq), _lib.current_stream(dev)))
    return out, prio, dq


class BDQNEngine:
    """The network's flat vector, its lagged copy, the optimizer state and the two counters."""

    def __init__(self, obs_dim, common_hidden, value_hidden, action_hidden, num_branches, action_per_branch, activation,
                 params: torch.Tensor, cfg: BDQNConfig):
        if not params.is_cuda:
            raise RuntimeError("BDQNEngine needs parameters on an MI355X (no CPU fallback)")
        self.dims = make_dims(obs_dim, common_hidden, value_hidden, action_hidden, num_branches, action_per_branch, activation)
        self.obs_dim, self.common_hidden, self.value_hidden, self.action_hidden, self.D, self.A, self.activation = self.dims
        self.cfg = cfg
        self._net = _lib.NetDesc.make(self.obs_dim, list(self.common_hidden), self.activation)
        out = (C.c_int64 * 8)()
        _lib.check(_lib.load().ts_bdqn_layout(*self._dims(), out))
        self.count = int(out[0])
        if self.count != layout(self.dims)[2]:
            raise RuntimeError(f"ts_bdqn_layout gives {self.count} floats, the converters {layout(self.dims)[2]}")
        if params.numel() != self.count:
            raise ValueError(f"the flat BDQN vector has {params.numel()} entries, ts_bdqn_layout gives {self.count}")
        self.device = params.device
        self.params = params.detach().float().contiguous().clone()
        self.params_old = self.params.clone() if cfg.target_update_freq > 0 else None
        self.adam_m, self.adam_v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.adam_step = 0
        self.iter = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _dims(self):
        """The model's description as every ts_bdqn_* entry point takes it."""
        return C.byref(self._net), _lib.i64(self.value_hidden), _lib.i64(self.action_hidden), _lib.i64(self.D), _lib.i64(self.A)

    # -- converters -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_model(cls, model, cfg: BDQNConfig, device="cuda"):
        d = describe_model(model)
        named = dict(model.named_parameters())
        return cls(*d["dims"], flat_from_torch([named[k] for k in d["keys"]], *d["dims"], device), cfg)

    def to_tensors(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        return flat_to_torch(self.params if flat is None else flat, *self.dims)

    # -- data -------------------------------------------------------------------------------------------------------------------
    def _obs(self, obs):
        return torch.as_tensor(obs).to(device=self.device, dtype=torch.float32).reshape(-1, self.obs_dim).contiguous()

    def _vec(self, x, b, dtype, what):
        x = torch.as_tensor(x).to(device=self.device, dtype=dtype).reshape(-1).contiguous()
        if x.numel() != b:
            raise ValueError(f"BDQN: {what} must have one entry per transition")
        return x

    # -- the passes -------------------------------------------------------------------------------------------------------------
    def forward(self, obs, old: bool = False, want_act: bool = True):
        """-> (q float32[B, D, A], act int64[B, D] or None) of the online (old=True: the lagged) network."""
        obs = self._obs(obs)
        b = obs.shape[0]
        params = self.params_old if old else self.params
        if params is None:
            raise RuntimeError("BDQN: there is no lagged network (target_update_freq = 0)")
        q = torch.empty((b, self.D, self.A), dtype=torch.float32, device=self.device)
        act = torch.empty((b, self.D), dtype=torch.int64, device=self.device) if want_act else None
        _lib.check(_lib.load().ts_bdqn_forward(self._ws.handle, _lib.ptr(params), *self._dims(), _lib.ptr(obs), _lib.i64(b), _lib.ptr(q),
                                               _lib.ptr(act), _lib.current_stream(self.device)))
        return q, act

    def target_q(self, obs_next, rew, end) -> torch.Tensor:
        """bdqn.py:155-195 -> ret float32[B] = rew + gamma mean_d Q_eval(s', argmax_a Q_sel(s')) (1 - end)."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        rew = self._vec(rew, b, torch.float32, "rew")
        end = (self._vec(end, b, torch.float32, "end") != 0).to(torch.uint8)
        ret = torch.empty(b, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_bdqn_target_q(self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), *self._dims(),
                                                _lib.ptr(obs_next), _lib.ptr(rew), _lib.ptr(end), _lib.i64(b), _lib.f64(self.cfg.gamma),
                                                C.c_int32(int(self.cfg.is_double)), _lib.ptr(ret), _lib.current_stream(self.device)))
        return ret

    def _step(self, obs, act, ret, weight, grad_out, apply: bool):
        cfg = self.cfg
        obs = self._obs(obs)
        b = obs.shape[0]
        act = torch.as_tensor(act).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if act.numel() != b * self.D:
            raise ValueError(f"BDQN: act must be [B, {self.D}]")
        ret = self._vec(ret, b, torch.float32, "ret")
        weight = None if weight is None else self._vec(weight, b, torch.float32, "weight")
        if grad_out is not None and (grad_out.numel() != self.count or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the model's size")
        loss_out = torch.empty(1, dtype=torch.float32, device=self.device)
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_bdqn_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), _lib.i64(self.adam_step + 1),
            *self._dims(), _lib.ptr(obs), _lib.ptr(act), _lib.ptr(ret), _lib.ptr(weight), _lib.i64(b),
            C.c_int32(OPTIMIZERS[cfg.optimizer]), _lib.f64(cfg.lr if apply else -1.0), _lib.f64(cfg.betas[0]), _lib.f64(cfg.betas[1]),
            _lib.f64(cfg.adam_eps), _lib.f64(cfg.weight_decay), _lib.f64(cfg.rms_alpha), _lib.f64(cfg.rms_momentum),
            C.c_int32(int(cfg.rms_centered)), _lib.f64(cfg.max_grad_norm or 0.0), _lib.ptr(loss_out), _lib.ptr(prio), _lib.ptr(grad_out),
            _lib.current_stream(self.device)))
        return loss_out, prio

    def update(self, obs, act, ret, weight=None):
        """bdqn.py:206-224: the lagged network is synchronised FIRST (dqn.py:277-285: every target_update_freq-th call, the
        first included), then one optimizer step -> (loss float32[1], prio float32[B] = sum_d td, signed), both on the device."""
        sync = self.params_old is not None and self.iter % self.cfg.target_update_freq == 0
        saved = self.params_old.clone() if sync else None
        if sync:
            self.params_old.copy_(self.params)
        try:
            out = self._step(obs, act, ret, weight, None, True)
        except Exception:                          # a refused argument leaves the lagged network and both counters alone
            if sync:
                self.params_old.copy_(saved)
            raise
        self.iter += 1
        self.adam_step += 1
        return out

    def gradient(self, obs, act, ret, weight=None):
        """-> (grad float32[count], loss, prio) at unchanged parameters, optimizer state and counters."""
        grad = torch.empty(self.count, dtype=torch.float32, device=self.device)
        loss_out, prio = self._step(obs, act, ret, weight, grad, False)
        return grad, loss_out, prio
