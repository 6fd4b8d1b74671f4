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
from . import vecq as V
from .buffer import DeviceReplayBuffer
from .dqn import DQNConfig

MAX_OBS, MAX_TRUNK, MAX_STREAM, MAX_WIDTH, MAX_ACTIONS, MAX_BATCH = 256, 4, 2, 256, 32, V.MAX_BATCH
ENVELOPE = (f"Net on vector observations of 1 .. {MAX_OBS} entries, 1 .. {MAX_TRUNK} hidden layers, no dueling or dueling_param with "
            f"0 .. {MAX_STREAM} hidden layers in each of Q and V, widths multiples of 32 in [32, {MAX_WIDTH}], ReLU, no norm_layer, "
            f"softmax=False, num_atoms=1, concat=False, 1 .. {MAX_ACTIONS} actions, the activations of a 32-row tile within 160 KB of LDS")
_F = V.Family("DQN MLP", ENVELOPE)


def make_layers(obs_dim, trunk, q_hidden, v_hidden, n_act) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    trunk = tuple(int(w) for w in trunk)
    dueling = q_hidden is not None or v_hidden is not None
    q = tuple(int(w) for w in (q_hidden or ())) if dueling else None
    v = tuple(int(w) for w in (v_hidden or ())) if dueling else None
    obs_dim, n_act = int(obs_dim), int(n_act)
    _F.in_range("obs_dim", obs_dim, 1, MAX_OBS)
    _F.count(len(trunk), "trunk hidden layers", 1, MAX_TRUNK)
    if dueling and (len(q) > MAX_STREAM or len(v) > MAX_STREAM):
        raise _F.refuse(f"Q / V streams with {len(q)} / {len(v)} hidden layers (0 .. {MAX_STREAM})")
    _F.widths(trunk + (q or ()) + (v or ()), MAX_WIDTH)
    _F.count(n_act, "actions", 1, MAX_ACTIONS)
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
    return _F.layout("ts_dqn_mlp_layout", _desc(layers), batch)


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
    return _F.flat_from_torch(tensors, *_blocks(tuple(layers)), device)


def flat_to_torch(flat: torch.Tensor, *layers) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> tensors in `state_dict_keys` order (on flat's device)."""
    return _F.flat_to_torch(flat, *_blocks(tuple(layers)))


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module (`model`, `Q`, `V`, `use_dueling`, `softmax`, `num_atoms`; common.py:286-341), or
    raises NotImplementedError naming what is not supported."""
    _F.require_net(net)
    if net.softmax:
        raise _F.refuse("softmax=True is not supported")
    if int(net.num_atoms) != 1:
        raise _F.refuse(f"num_atoms = {net.num_atoms} is not supported")

    def chain(mlp, part, ends_linear: bool):
        hidden, last = _F.chain(mlp.model, part)
        if ends_linear != (last is not None):
            raise _F.refuse("the last layer must be a Linear onto the outputs (concat=True is not supported)" if ends_linear
                            else "the trunk of a dueling Net ends in its last hidden layer", part)
        return hidden, last

    dueling = bool(net.use_dueling)
    trunk, head = chain(net.model, "model", not dueling)
    if not trunk:
        raise _F.refuse("at least one hidden layer is needed")
    q = v = None
    if dueling:
        q_lin, head = chain(net.Q, "Q", True)
        v_lin, v_head = chain(net.V, "V", True)
        if v_head.out_features != 1:
            raise _F.refuse(f"V must end in one output, found {v_head.out_features}")
        q, v = [l.out_features for l in q_lin], [l.out_features for l in v_lin]
    layers = make_layers(trunk[0].in_features, [l.out_features for l in trunk], q, v, head.out_features)
    _F.same_parameters(net, state_dict_keys(layers), "a Net's")
    return layers


class DQNMlpEngine(V.VecQEngine):
    """State of one DQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters."""

    FAMILY = _F

    def __init__(self, layers, flat_params: torch.Tensor, cfg: DQNConfig):
        self._require_device(flat_params)
        layers = make_layers(*layers)
        super().__init__(layers, _desc(layers), layout(layers)["count"], flat_params, cfg)
        self.n_act = layers[4]

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
        return self._preprocess(buffer, obs_rows, indices, stack_num, obs_next_rows, pair, coef)

    # -- the two halves of an update ---------------------------------------------------------------------------------------------
    def gradient(self, obs, act, returns, weight, grad_out: torch.Tensor):
        """Periodic target sync + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, td)."""
        return self.update_with_batch(obs, act, returns, weight, grad_out=grad_out, apply=False)

    # -- DQN._update_with_batch --------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (loss float32[1] device tensor, td_error float32[B]); td_error is the new batch.weight.  The lagged network takes
        the pre-step parameters inside the call (every target_update_freq-th call, the first included).  A refused argument
        leaves the lagged network and both counters alone."""
        obs = self._obs(obs)
        b = obs.shape[0]
        act, weight = self._batch_args(b, act, weight, grad_out)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if returns.numel() != b:
            raise ValueError("act / returns length mismatch")
        td = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = self.cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_dqn_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(self._sync_now())), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), self._adam_arg(apply), self._d, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(returns), _lib.ptr(weight),
            _lib.i64(b), C.byref(hp), _lib.ptr(td), _lib.ptr(loss), _lib.ptr(grad_out), _lib.current_stream(self.device)))
        self._stepped(apply)
        return loss, td
