"""The Intrinsic Curiosity Module on the Atari trunk on the MI355X engine; the wrapped algorithm's update is tianshou_amd.ppo_cnn.

The model of examples/atari/atari_ppo.py:136-160 (and atari_dqn.py / atari_sac.py / vizdoom_ppo.py, which build it the same way):
    feature_net   = DQNet(c, h, w, action_shape, features_only=True).net   three convolutions, a ReLU behind each, Flatten
    forward_model = MLP(F + A -> hidden_sizes -> F), inverse_model = MLP(2F -> hidden_sizes -> A), both ReLU
with F = 64 OH3 OW3 (3136 at 84 x 84).  One flat vector `conv1 | conv2 | conv3 | forward | inverse` (ts_icm_cnn_layout): the conv
blocks as in ppo_cnn / dqn, the model blocks as in icm.  The engine indexes features in NHWC flatten order (h, w, channel), torch
in (channel, h, w): the converters permute the feature rows of both models' first layers and the columns and bias of the forward
model's last layer.  Frames are NHWC uint8 or float32, raw values.

`update` walks the batch in chunks: ts_icm_cnn_grad adds every chunk's gradient and loss sums onto one accumulator in chunk
order, ts_icm_cnn_apply then does the ONE optimizer step of icm.py:90-109.  The frames of a large rollout can be gathered chunk by
chunk (`rows(lo, hi)`) and are never all resident.  No CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .dqn import _u8_flag
from .icm import MAX_ACTIONS, MAX_HIDDEN, OPTIMIZERS, ICMConfig, _linear_chain, _pad32, net_descs

CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1))       # (out channels, kernel, stride) of DQNet's three convolutions
# Transitions per ts_icm_cnn_grad call: the largest of {1024, 4096, 8192} that is not slower per transition at 84 x 84.  Measured
# on an MI355X at N = 16,384 (profiles/icm_cnn_bench.json, `us_per_transition_by_chunk`, frame gather included): 1.92 / 1.35 /
# 1.23 us per transition (a larger chunk pays the weight-gradient slab sums and the accumulate pass over the 6.5 M-entry gradient
# less often; which of the two it is was not profiled).  atari_ppo.py's N = 1,000 is one chunk either way.
DEFAULT_CHUNK = 8192


def conv_out(h: int, w: int):
    """-> [(oh, ow)] x 3 of the conv stack on an h x w frame (entries < 1: the frame is too small)."""
    out = []
    for _, k, s in CONVS:
        h, w = (h - k) // s + 1 if h >= k else 0, (w - k) // s + 1 if w >= k else 0
        out.append((h, w))
    return out


def feature_dim(h: int, w: int) -> int:
    oh, ow = conv_out(h, w)[2]
    return 64 * oh * ow


def model_dims(f: int, n_act: int, model_hidden) -> list[list[int]]:
    mh = [int(x) for x in model_hidden]
    return [[f + n_act, *mh, f], [2 * f, *mh, n_act]]


def _feat_perm(h: int, w: int) -> torch.Tensor:
    """perm[e] = the torch feature index (channel, h, w) of the engine's feature e (h, w, channel)."""
    oh, ow = conv_out(h, w)[2]
    return torch.arange(64 * oh * ow).reshape(64, oh, ow).permute(1, 2, 0).reshape(-1)


def _model_tensors_to_engine(t: list[torch.Tensor], f: int, perm: torch.Tensor, inverse: bool = False) -> list[torch.Tensor]:
    """The four permutations on [w, b, ...] of forward + inverse model (nn.Linear layout [out, in]); inverse=True: engine -> torch."""
    t = [x.detach().float().cpu().clone() for x in t]
    n_fwd = len(t) // 2                              # both models have the same number of layers
    p = torch.argsort(perm) if inverse else perm

    def cols(wt, lo):                                # input features [lo, lo + f) of a first layer
        wt[:, lo:lo + f] = wt[:, lo:lo + f][:, p]

    cols(t[0], 0)                                    # rows [0, F) of the forward model's first layer
    t[n_fwd - 2] = t[n_fwd - 2][p, :]                # columns of the forward model's last layer ...
    t[n_fwd - 1] = t[n_fwd - 1][p]                   # ... and its bias
    cols(t[n_fwd], 0)                                # rows [0, F) of the inverse model's first layer
    cols(t[n_fwd], f)                                # rows [F, 2F)
    return t


def flat_from_torch(tensors, c: int, h: int, w: int, n_act: int, model_hidden, device="cuda") -> torch.Tensor:
    """[conv1.w, conv1.b, conv2.w, conv2.b, conv3.w, conv3.b, forward (w, b)..., inverse (w, b)...] in torch layout (parameters
    or their moments) -> the flat vector."""
    t = list(tensors)
    f = feature_dim(h, w)
    dims = model_dims(f, n_act, model_hidden)
    if len(t) != 6 + 2 * sum(len(d) - 1 for d in dims):
        raise ValueError(f"ICM: expected {6 + 2 * sum(len(d) - 1 for d in dims)} tensors, got {len(t)}")
    parts, ic = [], c
    for i, (oc, k, _) in enumerate(CONVS):
        wt, b = t[2 * i].detach().float().cpu(), t[2 * i + 1].detach().float().cpu()
        if tuple(wt.shape) != (oc, ic, k, k) or b.numel() != oc:
            raise ValueError(f"ICM: conv{i + 1} must be {(oc, ic, k, k)}, got {tuple(wt.shape)}")
        parts += [wt.permute(2, 3, 1, 0).reshape(-1), b.reshape(-1)]
        ic = oc
    mt = _model_tensors_to_engine(t[6:], f, _feat_perm(h, w))
    for d in dims:
        for kk, n in zip(d[:-1], d[1:]):
            wt, b = mt.pop(0), mt.pop(0)
            if tuple(wt.shape) != (n, kk) or b.numel() != n:
                raise ValueError(f"ICM: a layer of {kk} -> {n} got a weight of shape {tuple(wt.shape)}")
            blk = torch.zeros((_pad32(kk) + 1, _pad32(n)), dtype=torch.float32)
            blk[:kk, :n], blk[_pad32(kk), :n] = wt.t(), b.reshape(-1)
            parts.append(blk.reshape(-1))
    return torch.cat(parts).to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, c: int, h: int, w: int, n_act: int, model_hidden) -> list[torch.Tensor]:
    f = feature_dim(h, w)
    fl, out, o, ic = flat.detach(), [], 0, c
    for oc, k, _ in CONVS:
        kk = k * k * ic
        wb = fl[o:o + (kk + 1) * oc].reshape(kk + 1, oc)
        out += [wb[:kk].reshape(k, k, ic, oc).permute(3, 2, 0, 1).contiguous(), wb[kk].clone()]
        o, ic = o + (kk + 1) * oc, oc
    mt = []
    for d in model_dims(f, n_act, model_hidden):
        for kk, n in zip(d[:-1], d[1:]):
            kp, np_ = _pad32(kk), _pad32(n)
            blk = fl[o:o + (kp + 1) * np_].reshape(kp + 1, np_)
            mt += [blk[:kk, :n].t().contiguous(), blk[kp, :n].clone()]
            o += (kp + 1) * np_
    dev = flat.device
    return out + [x.to(dev) for x in _model_tensors_to_engine(mt, f, _feat_perm(h, w), inverse=True)]


def padding_mask(c: int, h: int, w: int, n_act: int, model_hidden, device="cpu") -> torch.Tensor:
    """bool[count]: True at the padding entries of the flat vector (the conv blocks have none)."""
    blocks, ic = [], c
    for oc, k, _ in CONVS:
        blocks.append(torch.zeros((k * k * ic + 1) * oc, dtype=torch.bool))
        ic = oc
    for d in model_dims(feature_dim(h, w), n_act, model_hidden):
        for kk, n in zip(d[:-1], d[1:]):
            blk = torch.ones((_pad32(kk) + 1, _pad32(n)), dtype=torch.bool)
            blk[:kk, :n], blk[_pad32(kk), :n] = False, False
            blocks.append(blk.reshape(-1))
    return torch.cat(blocks).to(device)


class ICMCnnEngine:
    """The curiosity model's flat vector, its optimizer state and step counter."""

    def __init__(self, c: int, h: int, w: int, n_act: int, model_hidden, params: torch.Tensor, cfg: ICMConfig):
        if not params.is_cuda:
            raise RuntimeError("ICMCnnEngine needs parameters on an MI355X (no CPU fallback)")
        self.c, self.h, self.w, self.n_act, self.cfg = int(c), int(h), int(w), int(n_act), cfg
        self.model_hidden = [int(x) for x in model_hidden]
        _, self._model_net = net_descs(1, max(feature_dim(self.h, self.w), 1), [], "relu", self.model_hidden)
        out = (C.c_int64 * 12)()
        _lib.check(_lib.load().ts_icm_cnn_layout(*self._dims(), out))
        self.count, self.feature_dim = int(out[0]), int(out[1])
        self.offsets = {k: (int(out[2 + 2 * i]), int(out[3 + 2 * i])) for i, k in enumerate(("conv1", "conv2", "conv3", "forward", "inverse"))}
        if params.numel() != self.count:
            raise ValueError(f"the flat ICM vector has {params.numel()} entries, ts_icm_cnn_layout gives {self.count}")
        self.device = params.device
        self.params = params.detach().float().contiguous().clone()
        self.state_m, self.state_v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.optim_step = 0
        self._ws = _lib.default_workspace(self.device.index or 0)

    def _dims(self):
        return _lib.i64(self.c), _lib.i64(self.h), _lib.i64(self.w), C.byref(self._model_net), _lib.i64(self.n_act)

    # -- converters ---------------------------------------------------------------------------------------------------------------
    def to_tensors(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        return flat_to_torch(self.params if flat is None else flat, self.c, self.h, self.w, self.n_act, self.model_hidden)

    @classmethod
    def from_module(cls, module, c: int, h: int, w: int, cfg: ICMConfig, device="cuda"):
        """`module`: an IntrinsicCuriosityModule-shaped object (`describe_module`)."""
        d = describe_module(module, c, h, w)
        return cls(c, h, w, d["n_act"], d["model_hidden"], flat_from_torch(d["tensors"], c, h, w, d["n_act"], d["model_hidden"], device), cfg)

    def to_module(self, module) -> None:
        tensors = describe_module(module, self.c, self.h, self.w)["tensors"]
        with torch.no_grad():
            for dst, src in zip(tensors, self.to_tensors()):
                dst.copy_(src.to(dst.device).reshape(dst.shape))

    # -- data ---------------------------------------------------------------------------------------------------------------------
    def _rows(self, obs, act, obs_next):
        def frames(x):
            x = torch.as_tensor(x).to(self.device)
            if x.dtype not in (torch.uint8, torch.float32):
                x = x.to(torch.float32)
            if x.dim() != 4 or tuple(x.shape[1:]) != (self.h, self.w, self.c):
                raise ValueError(f"ICM: frames must be NHWC [B, {self.h}, {self.w}, {self.c}], got {tuple(x.shape)}")
            return x.contiguous()

        obs, obs_next = frames(obs), frames(obs_next)
        if obs_next.dtype != obs.dtype:
            obs, obs_next = obs.to(torch.float32), obs_next.to(torch.float32)
        act = torch.as_tensor(act).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if obs_next.shape[0] != obs.shape[0] or act.numel() != obs.shape[0]:
            raise ValueError("ICM: obs, act and obs_next differ in length")
        return obs, act, obs_next, obs.shape[0]

    # -- the passes ---------------------------------------------------------------------------------------------------------------
    def forward(self, obs, act, obs_next, want_act_hat: bool = True):
        """discrete.py:410-428 -> (mse_loss float32[B], act_hat float32[B, A] or None)."""
        obs, act, obs_next, b = self._rows(obs, act, obs_next)
        mse = torch.empty(b, dtype=torch.float32, device=self.device)
        act_hat = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device) if want_act_hat else None
        _lib.check(_lib.load().ts_icm_cnn_forward(self._ws.handle, _lib.ptr(self.params), *self._dims(), _lib.ptr(obs), _u8_flag(obs),
                                                  _lib.ptr(act), _lib.ptr(obs_next), _lib.i64(b), _lib.ptr(mse), _lib.ptr(act_hat),
                                                  _lib.current_stream(self.device)))
        return mse, act_hat

    def reward(self, obs, act, obs_next, rew, want_mse: bool = False):
        """icm.py:83 -> rew + float64(mse_loss * reward_scale), float64[B] (and mse_loss)."""
        obs, act, obs_next, b = self._rows(obs, act, obs_next)
        rew = torch.as_tensor(rew).to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        if rew.numel() != b:
            raise ValueError("ICM: rew must have one entry per transition")
        out = torch.empty_like(rew)
        mse = torch.empty(b, dtype=torch.float32, device=self.device) if want_mse else None
        _lib.check(_lib.load().ts_icm_cnn_reward(self._ws.handle, _lib.ptr(self.params), *self._dims(), _lib.ptr(obs), _u8_flag(obs),
                                                 _lib.ptr(act), _lib.ptr(obs_next), _lib.i64(b), _lib.ptr(rew),
                                                 _lib.f64(self.cfg.reward_scale), _lib.ptr(out), _lib.ptr(mse),
                                                 _lib.current_stream(self.device)))
        return (out, mse) if want_mse else out

    def update(self, obs, act=None, obs_next=None, chunk: int | None = None, grad_out: torch.Tensor | None = None, apply: bool = True,
               n: int | None = None) -> torch.Tensor:
        """icm.py:90-109 -> stats float32[3] = {icm_loss, icm_forward_loss, icm_inverse_loss} on the device, at the parameters
        before the step.  `obs`: NHWC frames with `act` / `obs_next`, or a callable rows(lo, hi) -> (obs, act, obs_next) of the
        transitions [lo, hi) of a batch of `n`.  apply=False: gradient (into grad_out) and statistics only."""
        cfg = self.cfg
        if callable(obs):
            if n is None:
                raise ValueError("ICM: update(rows, n=...) needs the batch length")
            rows, n = obs, int(n)
        else:
            whole = self._rows(obs, act, obs_next)
            n = whole[3]
            rows = lambda lo, hi: (whole[0][lo:hi], whole[1][lo:hi], whole[2][lo:hi])  # noqa: E731
        if n < 1:
            raise ValueError("ICM: update needs at least one transition")
        chunk = int(chunk or DEFAULT_CHUNK)
        if chunk < 1:
            raise ValueError("ICM: chunk must be positive")
        if grad_out is not None and (grad_out.numel() != self.count or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the ICM model's size")
        grad = grad_out if grad_out is not None else torch.empty(self.count, dtype=torch.float32, device=self.device)
        sums, stats = torch.empty(2, dtype=torch.float32, device=self.device), torch.empty(3, dtype=torch.float32, device=self.device)
        lib, stream = _lib.load(), _lib.current_stream(self.device)
        for lo in range(0, n, chunk):
            o, a, o2, b = self._rows(*rows(lo, min(lo + chunk, n)))
            _lib.check(lib.ts_icm_cnn_grad(self._ws.handle, _lib.ptr(self.params), *self._dims(), _lib.ptr(o), _u8_flag(o), _lib.ptr(a),
                                           _lib.ptr(o2), _lib.i64(b), _lib.i64(n), _lib.f64(cfg.forward_loss_weight), _lib.f64(cfg.lr_scale),
                                           C.c_int(int(lo > 0)), _lib.ptr(grad), _lib.ptr(sums), stream))
        _lib.check(lib.ts_icm_cnn_apply(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.state_m), _lib.ptr(self.state_v), _lib.i64(self.optim_step + 1),
            *self._dims(), _lib.ptr(grad), _lib.ptr(sums), _lib.i64(n), _lib.f64(cfg.forward_loss_weight), _lib.f64(cfg.lr_scale),
            C.c_int32(OPTIMIZERS[cfg.optimizer]), _lib.f64(cfg.lr if apply else -1.0), _lib.f64(cfg.betas[0]), _lib.f64(cfg.betas[1]),
            _lib.f64(cfg.eps), _lib.f64(cfg.weight_decay), _lib.f64(cfg.rms_alpha), _lib.f64(cfg.rms_momentum),
            C.c_int32(int(cfg.rms_centered)), _lib.f64(cfg.max_grad_norm or 0.0), _lib.ptr(stats), stream))
        if apply:
            self.optim_step += 1                   # (after the call: a refused argument leaves the counter alone)
        return stats


def _conv_chain(net, c: int):
    """-> the three Conv2d of DQNet(features_only=True).net, or NotImplementedError naming what was found."""
    leaves = [m for m in net.modules() if len(list(m.children())) == 0 and not isinstance(m, torch.nn.Identity)]
    want = "Sequential(Conv2d(c,32,8,4), ReLU, Conv2d(32,64,4,2), ReLU, Conv2d(64,64,3,1), ReLU, Flatten)"
    names = [type(m).__name__ for m in leaves]
    if names != ["Conv2d", "ReLU", "Conv2d", "ReLU", "Conv2d", "ReLU", "Flatten"]:
        raise NotImplementedError(f"ICM feature_net: {want} is supported (found {', '.join(names) or 'no layers'})")
    convs, ic = leaves[0:6:2], c
    for i, (m, (oc, k, s)) in enumerate(zip(convs, CONVS)):
        found = (m.in_channels, m.out_channels, tuple(m.kernel_size), tuple(m.stride), tuple(m.padding), tuple(m.dilation), m.groups)
        if found != (ic, oc, (k, k), (s, s), (0, 0), (1, 1), 1):
            raise NotImplementedError(f"ICM feature_net: conv{i + 1} must be Conv2d({ic}, {oc}, {k}, {s}) (found Conv2d({m.in_channels}, "
                                      f"{m.out_channels}, kernel_size={tuple(m.kernel_size)}, stride={tuple(m.stride)}, "
                                      f"padding={tuple(m.padding)}, dilation={tuple(m.dilation)}, groups={m.groups}))")
        if m.bias is None:
            raise NotImplementedError(f"ICM feature_net: conv{i + 1} without bias is not supported")
        ic = oc
    return convs


def describe_module(module, c: int | None = None, h: int | None = None, w: int | None = None) -> dict:
    """-> {c, n_act, feature_dim, model_hidden, tensors = [w, b, ...] of conv1..3, forward, inverse} of an
    IntrinsicCuriosityModule-shaped object on c x h x w frames, or raises NotImplementedError naming what was found.
    c / h / w None: the channel count is conv1's, and the frame size -- not known before a buffer is seen -- is not checked
    (feature_dim is then the forward model's output width and must be a multiple of 64)."""
    for name in ("feature_net", "forward_model", "inverse_model"):
        if not hasattr(module, name):
            raise NotImplementedError(f"ICM model: an IntrinsicCuriosityModule is needed (found {type(module).__name__} without `{name}`)")
    if c is None:
        first = next((m for m in module.feature_net.modules() if isinstance(m, torch.nn.Conv2d)), None)
        c = first.in_channels if first is not None else 0
    convs = _conv_chain(module.feature_net, c)
    fwd, _ = _linear_chain(module.forward_model, "forward_model", ("relu",))
    inv, _ = _linear_chain(module.inverse_model, "inverse_model", ("relu",))
    n_act = inv[-1].out_features
    if h is None or w is None:
        f_dim, where = fwd[-1].out_features, "a multiple of 64"
        if f_dim % 64:
            raise NotImplementedError(f"ICM model: feature_dim must be 64 OH3 OW3, the conv stack's output (found {f_dim})")
    else:
        if min(min(o) for o in conv_out(h, w)) < 1:
            raise NotImplementedError(f"ICM feature_net: a {h} x {w} frame is too small for the conv stack")
        f_dim, where = feature_dim(h, w), f"64 OH3 OW3 on {h} x {w} frames"
    if int(getattr(module, "feature_dim", f_dim)) != f_dim or int(getattr(module, "action_dim", n_act)) != n_act:
        raise NotImplementedError(f"ICM model: feature_dim / action_dim ({getattr(module, 'feature_dim', None)}, "
                                  f"{getattr(module, 'action_dim', None)}) do not match the networks' outputs ({f_dim} = {where}, "
                                  f"{n_act})")
    if fwd[0].in_features != f_dim + n_act or fwd[-1].out_features != f_dim or inv[0].in_features != 2 * f_dim:
        raise NotImplementedError(f"ICM model: the dimensions do not chain (forward_model {fwd[0].in_features} -> {fwd[-1].out_features}, "
                                  f"inverse_model {inv[0].in_features} -> {n_act}, feature_dim {f_dim})")
    mh = [l.out_features for l in fwd[:-1]]
    if mh != [l.out_features for l in inv[:-1]]:
        raise NotImplementedError(f"ICM model: forward_model and inverse_model must share their hidden sizes (found {mh} and "
                                  f"{[l.out_features for l in inv[:-1]]})")
    if n_act > MAX_ACTIONS:
        raise NotImplementedError(f"ICM model: at most {MAX_ACTIONS} actions (found {n_act})")
    if mh and max(mh) > 1024:
        raise NotImplementedError(f"ICM model: hidden widths up to 1024 are supported (found {max(mh)})")
    assert len(mh) <= MAX_HIDDEN
    return {"c": int(c), "n_act": n_act, "feature_dim": f_dim, "model_hidden": mh,
            "tensors": [p for l in list(convs) + fwd + inv for p in (l.weight, l.bias)]}
