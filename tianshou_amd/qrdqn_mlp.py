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
whose last Linear has n_act * n_atoms outputs (`_plain`), so its blocks and converters serve here.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import dqn_mlp as M
from . import vecq as V
from .buffer import DeviceReplayBuffer
from .dqn import DQNConfig

MAX_OBS, MAX_TRUNK, MAX_WIDTH, MAX_ACTIONS, MAX_ATOMS, MAX_BATCH = 256, 4, 256, 32, 256, V.MAX_BATCH
ENVELOPE = (f"Net on vector observations of 1 .. {MAX_OBS} entries, 1 .. {MAX_TRUNK} hidden layers, widths multiples of 32 in "
            f"[32, {MAX_WIDTH}], ReLU, no norm_layer, no dueling_param, softmax=False, concat=False, 1 .. {MAX_ACTIONS} actions, "
            f"num_atoms 2 .. {MAX_ATOMS}, the activations and quantile tables of a 32-row tile within 160 KB of LDS")
_F = V.Family("QRDQN MLP", ENVELOPE)


def _make_layers(fam: V.Family, layout_of, obs_dim, trunk, n_act, n_atoms) -> tuple:
    """`make_layers` of a family on the plain Net with n_atoms outputs per action (here and c51_mlp)."""
    obs_dim, trunk, n_act, n_atoms = int(obs_dim), tuple(int(w) for w in trunk), int(n_act), int(n_atoms)
    fam.in_range("obs_dim", obs_dim, 1, MAX_OBS)
    fam.count(len(trunk), "hidden layers", 1, MAX_TRUNK)
    fam.widths(trunk, MAX_WIDTH)
    fam.count(n_act, "actions", 1, MAX_ACTIONS)
    fam.in_range("num_atoms", n_atoms, 2, MAX_ATOMS)
    layers = (obs_dim, trunk, n_act, n_atoms)
    layout_of(layers)                                  # the LDS carve of a tile is the library's arithmetic
    return layers


def make_layers(obs_dim, trunk, n_act, n_atoms) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    return _make_layers(_F, layout, obs_dim, trunk, n_act, n_atoms)


def _desc(layers):
    obs_dim, trunk, n_act, n_atoms = layers
    return (C.c_int64 * 15)(obs_dim, n_act, 0, len(trunk), 0, 0, *trunk, *([0] * (4 - len(trunk))), 0, 0, 0, 0, n_atoms)


def _plain(layers) -> tuple:
    """The dqn_mlp layers tuple with the same flat layout: a plain Net whose last Linear has n_act * n_atoms outputs."""
    obs_dim, trunk, n_act, n_atoms = layers
    return (obs_dim, trunk, None, None, n_act * n_atoms)


def layout(layers, batch: int = 1) -> dict:
    """ts_qrdqn_mlp_layout -> {count, lds_bytes, workspace_bytes}; NotImplementedError when the tile does not fit the LDS."""
    return _F.layout("ts_qrdqn_mlp_layout", _desc(layers), batch)


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


def _describe_plain(fam: V.Family, make, net, n_atoms: int) -> tuple:
    """The walk of `describe_module` over a plain Net with n_atoms outputs per action, once the family's own checks of
    `softmax`, `use_dueling` and `num_atoms` are through (here and c51_mlp)."""
    hidden, last = fam.chain(net.model.model)
    if last is None or not hidden:
        raise fam.refuse("at least one hidden layer and a last Linear onto the outputs are needed (concat=True is not supported)")
    if last.out_features % n_atoms:
        raise fam.refuse(f"{last.out_features} outputs are no multiple of num_atoms = {n_atoms}")
    layers = make(hidden[0].in_features, [l.out_features for l in hidden], last.out_features // n_atoms, n_atoms)
    fam.same_parameters(net, state_dict_keys(layers), "a Net's")
    return layers


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module (`model`, `use_dueling`, `softmax`, `num_atoms`; common.py:286-341), or raises
    NotImplementedError naming what is not supported."""
    _F.require_net(net)
    if net.softmax:
        raise _F.refuse("softmax=True is not supported")
    if net.use_dueling:
        raise _F.refuse("dueling_param with quantiles is not supported")
    n_atoms = int(net.num_atoms)
    _F.in_range("num_atoms", n_atoms, 2, MAX_ATOMS, " (DQN on a Net is dqn_mlp's)" if n_atoms == 1 else "")
    return _describe_plain(_F, make_layers, net, n_atoms)


class QRDQNMlpEngine(V.VecQEngine):
    """State of one QRDQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters.  `cfg` is a DQNConfig
    (`is_double`: the online network selects the action read from the lagged one, as the reference always does; `huber_delta` is
    not read: the quantile Huber loss has kappa = 1)."""

    FAMILY = _F

    def __init__(self, layers, flat_params: torch.Tensor, cfg: DQNConfig):
        self._require_device(flat_params)
        layers = make_layers(*layers)
        super().__init__(layers, _desc(layers), layout(layers)["count"], flat_params, cfg)
        _, _, self.n_act, self.n_atoms = layers
        self.tau_hat = tau_hat(self.n_atoms, self.device)

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
        return self._preprocess(buffer, obs_rows, indices, stack_num, obs_next_rows, pair, coef)

    # -- the two halves of an update ---------------------------------------------------------------------------------------------
    def gradient(self, obs, act, returns, weight, grad_out: torch.Tensor):
        """Periodic target sync + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, prio)."""
        return self.update_with_batch(obs, act, returns, weight, grad_out=grad_out, apply=False)

    # -- QRDQN._update_with_batch --------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (loss float32[1] device tensor, prio float32[B]); prio is the new batch.weight (qrdqn.py:128).  The lagged network
        takes the pre-step parameters inside the call (every target_update_freq-th call, the first included).  A refused argument
        leaves the lagged network and both counters alone."""
        obs = self._obs(obs)
        b = obs.shape[0]
        act, weight = self._batch_args(b, act, weight, grad_out)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).contiguous()
        if tuple(returns.shape) != (b, self.n_atoms):
            raise ValueError(f"returns must be [{b}, {self.n_atoms}]")
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = self.cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_qrdqn_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(self._sync_now())), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), self._adam_arg(apply), self._d, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(returns), _lib.ptr(weight),
            _lib.ptr(self.tau_hat), _lib.i64(b), C.byref(hp), _lib.ptr(loss), _lib.ptr(prio), _lib.ptr(grad_out),
            _lib.current_stream(self.device)))
        self._stepped(apply)
        return loss, prio
