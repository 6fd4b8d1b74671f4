"""DQN on vector observations (the dueling MLP `Net`) on the MI355X engine.

Mirrors, on device tensors:
    Net.forward                          tianshou/utils/net/common.py:343-369 (dueling: q - mean_a q + v)
    DiscreteQLearningPolicy.forward      tianshou/algorithm/modelfree/dqn.py:101-143
    DQN._target_q / _preprocess_batch    dqn.py:257-275, 365-379 (n-step via tianshou_amd.returns)
    DQN._update_with_batch               dqn.py:381-404 (+ periodic hard sync :277-285)
Setups: examples/discrete/discrete_dqn.py, examples/box2d/lunarlander_dqn.py, examples/box2d/acrobot_dualdqn.py.
`target_q` + `update_with_batch` are three launches (ts_dqn_mlp.hip).  There is no CPU path: every function calls libtsengine.so.

`layers` = (obs_dim, trunk widths, Q hidden widths, V hidden widths, n_act) describes the model everywhere; Q and V are None for a
plain Net (its last Linear is then the Q head).  Flat layout (ts_dqn_mlp_layout): per layer [K + 1, N], row K the bias, in the
order trunk | Q hidden | V hidden | Q head | V head.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .buffer import DeviceReplayBuffer, _i64_dev, gather_rows
from .dqn import DQNConfig
from .drqn import gather_stacked_obs_pair
from .returns import nstep_coefficients, nstep_indices

MAX_OBS, MAX_TRUNK, MAX_STREAM, MAX_WIDTH, MAX_ACTIONS, MAX_BATCH = 256, 4, 2, 256, 32, 4096
ENVELOPE = (f"Net on vector observations of 1 .. {MAX_OBS} entries, 1 .. {MAX_TRUNK} hidden layers, no dueling or dueling_param with "
            f"0 .. {MAX_STREAM} hidden layers in each of Q and V, widths multiples of 32 in [32, {MAX_WIDTH}], ReLU, no norm_layer, "
            f"softmax=False, num_atoms=1, concat=False, 1 .. {MAX_ACTIONS} actions, the activations of a 32-row tile within 160 KB of LDS")


def make_layers(obs_dim, trunk, q_hidden, v_hidden, n_act) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    trunk = tuple(int(w) for w in trunk)
    dueling = q_hidden is not None or v_hidden is not None
    q = tuple(int(w) for w in (q_hidden or ())) if dueling else None
    v = tuple(int(w) for w in (v_hidden or ())) if dueling else None
    obs_dim, n_act = int(obs_dim), int(n_act)
    if not 1 <= obs_dim <= MAX_OBS:
        raise NotImplementedError(f"DQN MLP: obs_dim = {obs_dim} is outside [1, {MAX_OBS}]; supported: {ENVELOPE}")
    if not 1 <= len(trunk) <= MAX_TRUNK:
        raise NotImplementedError(f"DQN MLP: {len(trunk)} trunk hidden layers (1 .. {MAX_TRUNK}); supported: {ENVELOPE}")
    if dueling and (len(q) > MAX_STREAM or len(v) > MAX_STREAM):
        raise NotImplementedError(f"DQN MLP: Q / V streams with {len(q)} / {len(v)} hidden layers (0 .. {MAX_STREAM}); supported: {ENVELOPE}")
    bad = [w for w in trunk + (q or ()) + (v or ()) if w % 32 or not 32 <= w <= MAX_WIDTH]
    if bad:
        raise NotImplementedError(f"DQN MLP: hidden width {bad[0]} is no multiple of 32 in [32, {MAX_WIDTH}]; supported: {ENVELOPE}")
    if not 1 <= n_act <= MAX_ACTIONS:
        raise NotImplementedError(f"DQN MLP: {n_act} actions (1 .. {MAX_ACTIONS}); supported: {ENVELOPE}")
    layers = (obs_dim, trunk, q, v, n_act)
    layout(layers)                                     # the LDS carve of a tile is the library's arithmetic
    return layers


def _desc(layers):
    obs_dim, trunk, q, v, n_act = layers
    pad = lambda t, n: list(t) + [0] * (n - len(t))  # noqa: E731
    q_, v_ = q or (), v or ()
    return (C.c_int64 * 14)(obs_dim, n_act, int(q is not None), len(trunk), len(q_), len(v_), *pad(trunk, 4), *pad(q_, 2), *pad(v_, 2))


def layout(layers, batch: int = 1) -> dict:
    """ts_dqn_mlp_layout -> {count, lds_bytes, workspace_bytes}; NotImplementedError when the tile does not fit the LDS."""
    out = (C.c_int64 * 16)()
    try:
        _lib.check(_lib.load().ts_dqn_mlp_layout(_desc(layers), _lib.i64(batch), out))
    except _lib.EngineError as e:
        if e.code != _lib.TS_ERR_UNSUPPORTED:
            raise
        raise NotImplementedError(f"DQN MLP: {e}; supported: {ENVELOPE}") from None
    return {"count": int(out[0]), "lds_bytes": int(out[1]), "workspace_bytes": int(out[2])}


def _blocks(layers):
    """-> ([(state-dict prefix, K, N)] in FLAT order, the same prefixes in state_dict() order)."""
    obs_dim, trunk, q, v, n_act = layers
    hidden, k = [], obs_dim
    for i, n in enumerate(trunk):
        hidden.append((f"model.model.{2 * i}", k, n))
        k = n
    top = k
    if q is None:
        flat = hidden + [(f"model.model.{2 * len(trunk)}", top, n_act)]
        return flat, [b[0] for b in flat]
    streams = {}
    for name, widths, n_out in (("Q", q, n_act), ("V", v, 1)):
        k, rows = top, []
        for i, n in enumerate(widths):
            rows.append((f"{name}.model.{2 * i}", k, n))
            k = n
        streams[name] = (rows, (f"{name}.model.{2 * len(widths)}", k, n_out))
    flat = hidden + streams["Q"][0] + streams["V"][0] + [streams["Q"][1], streams["V"][1]]
    order = [b[0] for b in hidden + streams["Q"][0] + [streams["Q"][1]] + streams["V"][0] + [streams["V"][1]]]
    return flat, order


def state_dict_keys(layers) -> list[str]:
    """Net.state_dict() order (common.py:336-341: model, Q, V)."""
    return [f"{p}.{s}" for p in _blocks(layers)[1] for s in ("weight", "bias")]


def flat_from_torch(tensors, *layers_and_device) -> torch.Tensor:
    """[w, b, ...] in `state_dict_keys` order (nn.Linear layout; parameters or their moments) -> the flat vector."""
    *layers, device = layers_and_device
    flat, order = _blocks(tuple(layers))
    t = list(tensors)
    if len(t) != 2 * len(order):
        raise ValueError(f"DQN MLP: expected {2 * len(order)} tensors, got {len(t)}")
    given = {p: (t[2 * i], t[2 * i + 1]) for i, p in enumerate(order)}
    parts = []
    for prefix, k, n in flat:
        w, b = given[prefix]
        if tuple(w.shape) != (n, k) or b.numel() != n:
            raise ValueError(f"DQN MLP: {prefix} must be Linear({k}, {n}), got weight {tuple(w.shape)} and {b.numel()} biases")
        parts += [w.detach().float().cpu().t().reshape(-1), b.detach().float().cpu().reshape(-1)]
    return torch.cat(parts).to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, *layers) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> tensors in `state_dict_keys` order (on flat's device)."""
    blocks, order = _blocks(tuple(layers))
    f, off, got = flat.detach(), 0, {}
    for prefix, k, n in blocks:
        got[prefix] = (f[off:off + k * n].reshape(k, n).t().contiguous(), f[off + k * n:off + (k + 1) * n].clone())
        off += (k + 1) * n
    if off != f.numel():
        raise ValueError(f"DQN MLP: the flat vector has {f.numel()} entries, the layout {off}")
    return [x for p in order for x in got[p]]


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module (`model`, `Q`, `V`, `use_dueling`, `softmax`, `num_atoms`; common.py:286-341), or
    raises NotImplementedError naming what is not supported."""
    for name in ("model", "use_dueling", "softmax", "num_atoms"):
        if not hasattr(net, name):
            raise NotImplementedError(f"DQN MLP: a Net is needed (found {type(net).__name__} without `{name}`); supported: {ENVELOPE}")
    if net.softmax:
        raise NotImplementedError(f"DQN MLP: softmax=True is not supported; supported: {ENVELOPE}")
    if int(net.num_atoms) != 1:
        raise NotImplementedError(f"DQN MLP: num_atoms = {net.num_atoms} is not supported; supported: {ENVELOPE}")

    def chain(mlp, who, ends_linear: bool):
        """[Linear, ReLU, Linear, ReLU, ...(, Linear)] -> ([hidden Linear], last Linear or None)."""
        mods = list(mlp.model.children())
        lin = []
        for j, m in enumerate(mods):
            if j % 2 == 0:
                if not isinstance(m, torch.nn.Linear):
                    raise NotImplementedError(f"DQN MLP {who}: Linear layers followed by ReLU only, no norm_layer (found "
                                              f"{type(m).__name__}); supported: {ENVELOPE}")
                if m.bias is None:
                    raise NotImplementedError(f"DQN MLP {who}: Linear layers without bias are not supported; supported: {ENVELOPE}")
                lin.append(m)
            elif not isinstance(m, torch.nn.ReLU):
                raise NotImplementedError(f"DQN MLP {who}: the activation must be ReLU (found {type(m).__name__}); supported: {ENVELOPE}")
        if ends_linear != (len(mods) % 2 == 1):
            raise NotImplementedError(f"DQN MLP {who}: " + ("the last layer must be a Linear onto the outputs (concat=True is not supported)"
                                                            if ends_linear else "the trunk of a dueling Net ends in its last hidden layer")
                                      + f"; supported: {ENVELOPE}")
        return (lin[:-1], lin[-1]) if ends_linear else (lin, None)

    dueling = bool(net.use_dueling)
    trunk, head = chain(net.model, "model", not dueling)
    if not trunk:
        raise NotImplementedError(f"DQN MLP: at least one hidden layer is needed; supported: {ENVELOPE}")
    q = v = None
    if dueling:
        q_lin, head = chain(net.Q, "Q", True)
        v_lin, v_head = chain(net.V, "V", True)
        if v_head.out_features != 1:
            raise NotImplementedError(f"DQN MLP: V must end in one output, found {v_head.out_features}; supported: {ENVELOPE}")
        q, v = [l.out_features for l in q_lin], [l.out_features for l in v_lin]
    layers = make_layers(trunk[0].in_features, [l.out_features for l in trunk], q, v, head.out_features)
    have = [k for k, _ in net.named_parameters()]
    if have != state_dict_keys(layers):
        raise NotImplementedError(f"DQN MLP: the model's parameters {have} are not a Net's {state_dict_keys(layers)}; supported: {ENVELOPE}")
    return layers


class DQNMlpEngine:
    """State of one DQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters."""

    def __init__(self, layers, flat_params: torch.Tensor, cfg: DQNConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("DQNMlpEngine needs parameters on an MI355X (no CPU fallback)")
        self.layers = make_layers(*layers)
        self.obs_dim, self.n_act, self.cfg = self.layers[0], self.layers[4], cfg
        self._d = _desc(self.layers)
        self.P = layout(self.layers)["count"]
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
            raise NotImplementedError(f"DQN MLP: a batch of {obs.shape[0]} rows (1 .. {MAX_BATCH})")
        return obs

    # -- Net.forward + DiscreteQLearningPolicy.forward -------------------------------------------------------------------------
    def forward(self, obs, params: torch.Tensor | None = None):
        """-> (q float32[B, A], act int64[B] = argmax, the first index on ties)."""
        obs = self._obs(obs)
        b = obs.shape[0]
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_dqn_mlp_forward(_lib.ptr(self.params if params is None else params), self._d, _lib.ptr(obs),
                                                  _lib.i64(b), _lib.ptr(q), _lib.ptr(act), _lib.current_stream(self.device)))
        return q, act

    # -- DQN._target_q -----------------------------------------------------------------------------------------------------------
    def target_returns(self, obs_next, coef) -> torch.Tensor:
        """`_target_q` on obs_next in one launch; with `coef` (returns.nstep_coefficients) the same launch ends in
        float(double(target_q * mask) * gamma^n + sum gamma^k r), the n-step returns."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        mask, gpow, mc = coef if coef is not None else (None, None, None)
        out = torch.empty(b, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_dqn_mlp_target_q(
            _lib.ptr(self.params), _lib.ptr(self.params_old), self._d, _lib.ptr(obs_next), _lib.i64(b), C.c_int32(int(self.cfg.is_double)),
            _lib.ptr(mask), _lib.ptr(gpow), _lib.ptr(mc), _lib.ptr(out), _lib.current_stream(self.device)))
        return out

    def target_q(self, obs_next) -> torch.Tensor:
        return self.target_returns(obs_next, None)

    # -- DQN._preprocess_batch -------------------------------------------------------------------------------------------------
    def preprocess_with_obs(self, buffer: DeviceReplayBuffer, obs_rows: torch.Tensor, indices, stack_num: int = 1,
                            obs_next_rows: torch.Tensor | None = None, prefetch: bool = False, pair=None, coef=None):
        """-> (batch.obs float32[I, obs_dim], returns float32[I]): both observation gathers from one launch
        (drqn.gather_stacked_obs_pair with stack_num 1; rows of another layout go through the index kernels), the n-step
        coefficients, then target + returns in one launch.  `prefetch` is accepted for the interface's sake: the update is one
        launch chain on one stream."""
        if stack_num != 1:
            raise NotImplementedError("DQN MLP: frame stacking is not supported (stack_num must be 1)")
        if pair is None:
            pair = gather_stacked_obs_pair(obs_rows, buffer, indices, self.cfg.n_step, 1, obs_next_rows)
        if pair is None:
            idx = _i64_dev(indices, buffer.device).reshape(-1)
            after = nstep_indices(buffer, idx, self.cfg.n_step)
            nxt = gather_rows(obs_rows, buffer.next(after)) if obs_next_rows is None else gather_rows(obs_next_rows, after)
            pair = (gather_rows(obs_rows, idx), nxt)
        if coef is None:
            coef = nstep_coefficients(buffer, indices, self.cfg.gamma, self.cfg.n_step)
        return self._obs(pair[0]), self.target_returns(pair[1], coef)

    # -- the two halves of an update ---------------------------------------------------------------------------------------------
    def gradient(self, obs, act, returns, weight, grad_out: torch.Tensor):
        """Periodic target sync + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, td)."""
        return self.update_with_batch(obs, act, returns, weight, grad_out=grad_out, apply=False)

    def apply_gradient(self, grad: torch.Tensor) -> None:
        """clip_grad_norm_ + Adam on a flat gradient (algorithm_base.py:496-500)."""
        cfg = self.cfg
        self.adam_step += 1
        _lib.check(_lib.load().ts_adam_step(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), _lib.ptr(grad),
            _lib.i64(self.P), _lib.i64(self.adam_step), _lib.f64(cfg.lr), _lib.f64(cfg.betas[0]),
            _lib.f64(cfg.betas[1]), _lib.f64(cfg.adam_eps), _lib.f64(cfg.max_grad_norm or 0.0),
            _lib.current_stream(self.device)))

    # -- DQN._update_with_batch --------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (loss float32[1] device tensor, td_error float32[B]); td_error is the new batch.weight.  The lagged network takes
        the pre-step parameters inside the call (every target_update_freq-th call, the first included).  A refused argument
        leaves the lagged network and both counters alone."""
        cfg = self.cfg
        obs = self._obs(obs)
        b = obs.shape[0]
        act = _i64_dev(act, self.device).reshape(-1)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if act.numel() != b or returns.numel() != b:
            raise ValueError("act / returns length mismatch")
        if weight is not None:
            weight = torch.as_tensor(weight, device=self.device).to(torch.float32).reshape(-1).contiguous()
            if weight.numel() != b:
                raise ValueError("weight length mismatch")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the model's size")
        sync = self.params_old is not None and self.iter % cfg.target_update_freq == 0    # dqn.py:283-285
        td = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_dqn_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(sync)), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), _lib.i64(self.adam_step + 1 if apply else max(self.adam_step, 1)), self._d, _lib.ptr(obs), _lib.ptr(act),
            _lib.ptr(returns), _lib.ptr(weight), _lib.i64(b), C.byref(hp), _lib.ptr(td), _lib.ptr(loss), _lib.ptr(grad_out),
            _lib.current_stream(self.device)))
        self.iter += 1
        if apply:
            self.adam_step += 1
        return loss, td
