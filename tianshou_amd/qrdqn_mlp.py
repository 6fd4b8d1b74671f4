"""QRDQN on vector observations (the plain MLP `Net` with `num_atoms` quantiles per action) on the MI355X engine.

Mirrors, on device tensors:
    Net.forward                          tianshou/utils/net/common.py:343-369 (logits.view(B, A, N))
    QRDQNPolicy.compute_q_value          tianshou/algorithm/modelfree/qrdqn.py:19-21 (mean over the quantiles)
    QRDQN._target_q / _preprocess_batch  qrdqn.py:94-106 (n-step via tianshou_amd.returns, on a [B, N] target)
    QRDQN._update_with_batch             qrdqn.py:108-131 (+ periodic hard sync, dqn.py:277-285)
Setup: test/discrete/test_qrdqn.py.  `target_returns` + `update_with_batch` are three launches (ts_qrdqn_mlp.hip).  There is no
CPU path: every function calls libtsengine.so.

`layers` = (obs_dim, trunk widths, n_act, n_atoms) describes the model everywhere.  Flat layout (ts_qrdqn_mlp_layout): per layer
[K + 1, width], row K the bias; the hidden layers, then the head [top + 1, n_act * n_atoms] -- dqn_mlp's layout of the plain Net
whose last Linear has n_act * n_atoms outputs, so its converters serve here.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import dqn_mlp as M
from .buffer import DeviceReplayBuffer, _i64_dev, gather_rows
from .dqn import DQNConfig
from .drqn import gather_stacked_obs_pair
from .returns import nstep_coefficients, nstep_indices

MAX_OBS, MAX_TRUNK, MAX_WIDTH, MAX_ACTIONS, MAX_ATOMS, MAX_BATCH = 256, 4, 256, 32, 256, 4096
ENVELOPE = (f"Net on vector observations of 1 .. {MAX_OBS} entries, 1 .. {MAX_TRUNK} hidden layers, widths multiples of 32 in "
            f"[32, {MAX_WIDTH}], ReLU, no norm_layer, no dueling_param, softmax=False, concat=False, 1 .. {MAX_ACTIONS} actions, "
            f"num_atoms 2 .. {MAX_ATOMS}, the activations and quantile tables of a 32-row tile within 160 KB of LDS")


def make_layers(obs_dim, trunk, n_act, n_atoms) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    obs_dim, trunk, n_act, n_atoms = int(obs_dim), tuple(int(w) for w in trunk), int(n_act), int(n_atoms)
    if not 1 <= obs_dim <= MAX_OBS:
        raise NotImplementedError(f"QRDQN MLP: obs_dim = {obs_dim} is outside [1, {MAX_OBS}]; supported: {ENVELOPE}")
    if not 1 <= len(trunk) <= MAX_TRUNK:
        raise NotImplementedError(f"QRDQN MLP: {len(trunk)} hidden layers (1 .. {MAX_TRUNK}); supported: {ENVELOPE}")
    bad = [w for w in trunk if w % 32 or not 32 <= w <= MAX_WIDTH]
    if bad:
        raise NotImplementedError(f"QRDQN MLP: hidden width {bad[0]} is no multiple of 32 in [32, {MAX_WIDTH}]; supported: {ENVELOPE}")
    if not 1 <= n_act <= MAX_ACTIONS:
        raise NotImplementedError(f"QRDQN MLP: {n_act} actions (1 .. {MAX_ACTIONS}); supported: {ENVELOPE}")
    if not 2 <= n_atoms <= MAX_ATOMS:
        raise NotImplementedError(f"QRDQN MLP: num_atoms = {n_atoms} is outside [2, {MAX_ATOMS}]; supported: {ENVELOPE}")
    layers = (obs_dim, trunk, n_act, n_atoms)
    layout(layers)                                     # the LDS carve of a tile is the library's arithmetic
    return layers


def _desc(layers):
    obs_dim, trunk, n_act, n_atoms = layers
    return (C.c_int64 * 15)(obs_dim, n_act, 0, len(trunk), 0, 0, *trunk, *([0] * (4 - len(trunk))), 0, 0, 0, 0, n_atoms)


def _plain(layers) -> tuple:
    """The dqn_mlp layers tuple with the same flat layout: a plain Net whose last Linear has n_act * n_atoms outputs."""
    obs_dim, trunk, n_act, n_atoms = layers
    return (obs_dim, trunk, None, None, n_act * n_atoms)


def layout(layers, batch: int = 1) -> dict:
    """ts_qrdqn_mlp_layout -> {count, lds_bytes, workspace_bytes}; NotImplementedError when the tile does not fit the LDS."""
    out = (C.c_int64 * 16)()
    try:
        _lib.check(_lib.load().ts_qrdqn_mlp_layout(_desc(layers), _lib.i64(batch), out))
    except _lib.EngineError as e:
        if e.code != _lib.TS_ERR_UNSUPPORTED:
            raise
        raise NotImplementedError(f"QRDQN MLP: {e}; supported: {ENVELOPE}") from None
    return {"count": int(out[0]), "lds_bytes": int(out[1]), "workspace_bytes": int(out[2])}


def state_dict_keys(layers) -> list[str]:
    return M.state_dict_keys(_plain(layers))


def flat_from_torch(tensors, *layers_and_device) -> torch.Tensor:
    """[w, b, ...] in `state_dict_keys` order (nn.Linear layout; parameters or their moments) -> the flat vector."""
    *layers, device = layers_and_device
    return M.flat_from_torch(tensors, *_plain(tuple(layers)), device)


def flat_to_torch(flat: torch.Tensor, *layers) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> tensors in `state_dict_keys` order (on flat's device)."""
    return M.flat_to_torch(flat, *_plain(tuple(layers)))


def tau_hat(n_atoms: int, device) -> torch.Tensor:
    """qrdqn.py:87-91: the quantile midpoints, in torch's own float32 arithmetic."""
    tau = torch.linspace(0, 1, n_atoms + 1)
    return ((tau[:-1] + tau[1:]) / 2).to(device).contiguous()


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module (`model`, `use_dueling`, `softmax`, `num_atoms`; common.py:286-341), or raises
    NotImplementedError naming what is not supported."""
    for name in ("model", "use_dueling", "softmax", "num_atoms"):
        if not hasattr(net, name):
            raise NotImplementedError(f"QRDQN MLP: a Net is needed (found {type(net).__name__} without `{name}`); supported: {ENVELOPE}")
    if net.softmax:
        raise NotImplementedError(f"QRDQN MLP: softmax=True is not supported; supported: {ENVELOPE}")
    if net.use_dueling:
        raise NotImplementedError(f"QRDQN MLP: dueling_param with quantiles is not supported; supported: {ENVELOPE}")
    n_atoms = int(net.num_atoms)
    if not 2 <= n_atoms <= MAX_ATOMS:
        raise NotImplementedError(f"QRDQN MLP: num_atoms = {n_atoms} is outside [2, {MAX_ATOMS}]"
                                  + (" (DQN on a Net is dqn_mlp's)" if n_atoms == 1 else "") + f"; supported: {ENVELOPE}")
    mods = list(net.model.model.children())
    for j, m in enumerate(mods):
        if j % 2 == 0 and (not isinstance(m, torch.nn.Linear) or m.bias is None):
            raise NotImplementedError(f"QRDQN MLP: Linear layers with bias followed by ReLU only, no norm_layer (found {type(m).__name__}); "
                                      f"supported: {ENVELOPE}")
        if j % 2 == 1 and not isinstance(m, torch.nn.ReLU):
            raise NotImplementedError(f"QRDQN MLP: the activation must be ReLU (found {type(m).__name__}); supported: {ENVELOPE}")
    if len(mods) % 2 == 0 or len(mods) < 3:
        raise NotImplementedError(f"QRDQN MLP: at least one hidden layer and a last Linear onto the outputs are needed (concat=True is "
                                  f"not supported); supported: {ENVELOPE}")
    lin = mods[0::2]
    if lin[-1].out_features % n_atoms:
        raise NotImplementedError(f"QRDQN MLP: {lin[-1].out_features} outputs are no multiple of num_atoms = {n_atoms}; supported: {ENVELOPE}")
    layers = make_layers(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features // n_atoms, n_atoms)
    have = [k for k, _ in net.named_parameters()]
    if have != state_dict_keys(layers):
        raise NotImplementedError(f"QRDQN MLP: the model's parameters {have} are not a Net's {state_dict_keys(layers)}; supported: {ENVELOPE}")
    return layers


class QRDQNMlpEngine:
    """State of one QRDQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters.  `cfg` is a DQNConfig
    (`is_double`: the online network selects the action read from the lagged one, as the reference always does; `huber_delta` is
    not read: the quantile Huber loss has kappa = 1)."""

    def __init__(self, layers, flat_params: torch.Tensor, cfg: DQNConfig):
        if not flat_params.is_cuda:
            raise RuntimeError("QRDQNMlpEngine needs parameters on an MI355X (no CPU fallback)")
        self.layers = make_layers(*layers)
        self.obs_dim, _, self.n_act, self.n_atoms = self.layers
        self.cfg = cfg
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
        self.tau_hat = tau_hat(self.n_atoms, self.device)
        self._ws = _lib.default_workspace(self.device.index or 0)

    _obs = M.DQNMlpEngine._obs
    apply_gradient = M.DQNMlpEngine.apply_gradient

    # -- Net.forward + QRDQNPolicy.compute_q_value + the greedy action ----------------------------------------------------------
    def forward(self, obs, params: torch.Tensor | None = None):
        """-> (dist float32[B, A, N], q float32[B, A] = mean over the quantiles, act int64[B] = argmax, the first index on ties)."""
        obs = self._obs(obs)
        b = obs.shape[0]
        dist = torch.empty((b, self.n_act, self.n_atoms), dtype=torch.float32, device=self.device)
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_qrdqn_mlp_forward(_lib.ptr(self.params if params is None else params), self._d, _lib.ptr(obs), _lib.i64(b),
                                                    _lib.ptr(dist), _lib.ptr(q), _lib.ptr(act), _lib.current_stream(self.device)))
        return dist, q, act

    # -- QRDQN._target_q -----------------------------------------------------------------------------------------------------------
    def target_returns(self, obs_next, coef) -> torch.Tensor:
        """`_target_q` on obs_next in one launch -> float32[B, N]; with `coef` (returns.nstep_coefficients) the same launch ends in
        float(double(target * mask) * gamma^n + sum gamma^k r) per quantile, the n-step returns."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        mask, gpow, mc = coef if coef is not None else (None, None, None)
        out = torch.empty((b, self.n_atoms), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_qrdqn_mlp_target_dist(
            _lib.ptr(self.params), _lib.ptr(self.params_old), self._d, _lib.ptr(obs_next), _lib.i64(b), C.c_int32(int(self.cfg.is_double)),
            _lib.ptr(mask), _lib.ptr(gpow), _lib.ptr(mc), _lib.ptr(out), _lib.current_stream(self.device)))
        return out

    def target_dist(self, obs_next) -> torch.Tensor:
        return self.target_returns(obs_next, None)

    # -- QRDQN._preprocess_batch -------------------------------------------------------------------------------------------------
    def preprocess_with_obs(self, buffer: DeviceReplayBuffer, obs_rows: torch.Tensor, indices, stack_num: int = 1,
                            obs_next_rows: torch.Tensor | None = None, prefetch: bool = False, pair=None, coef=None):
        """-> (batch.obs float32[I, obs_dim], returns float32[I, N]): as DQNMlpEngine.preprocess_with_obs (both observation gathers
        from one launch, the n-step coefficients, then target + returns in one launch)."""
        if stack_num != 1:
            raise NotImplementedError("QRDQN MLP: frame stacking is not supported (stack_num must be 1)")
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
        """Periodic target sync + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, prio)."""
        return self.update_with_batch(obs, act, returns, weight, grad_out=grad_out, apply=False)

    # -- QRDQN._update_with_batch --------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (loss float32[1] device tensor, prio float32[B]); prio is the new batch.weight (qrdqn.py:128).  The lagged network
        takes the pre-step parameters inside the call (every target_update_freq-th call, the first included).  A refused argument
        leaves the lagged network and both counters alone."""
        cfg = self.cfg
        obs = self._obs(obs)
        b = obs.shape[0]
        act = _i64_dev(act, self.device).reshape(-1)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).contiguous()
        if act.numel() != b or tuple(returns.shape) != (b, self.n_atoms):
            raise ValueError(f"act must hold {b} entries and returns must be [{b}, {self.n_atoms}]")
        if weight is not None:
            weight = torch.as_tensor(weight, device=self.device).to(torch.float32).reshape(-1).contiguous()
            if weight.numel() != b:
                raise ValueError("weight length mismatch")
        if grad_out is not None and (grad_out.numel() != self.P or grad_out.dtype != torch.float32):
            raise ValueError("grad_out must be a float32 vector of the model's size")
        sync = self.params_old is not None and self.iter % cfg.target_update_freq == 0    # dqn.py:283-285
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_qrdqn_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(sync)), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), _lib.i64(self.adam_step + 1 if apply else max(self.adam_step, 1)), self._d, _lib.ptr(obs), _lib.ptr(act),
            _lib.ptr(returns), _lib.ptr(weight), _lib.ptr(self.tau_hat), _lib.i64(b), C.byref(hp), _lib.ptr(loss), _lib.ptr(prio),
            _lib.ptr(grad_out), _lib.current_stream(self.device)))
        self.iter += 1
        if apply:
            self.adam_step += 1
        return loss, prio
