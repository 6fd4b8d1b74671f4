"""C51 on vector observations (the plain MLP `Net(softmax=True, num_atoms=N)`) on the MI355X engine.

Mirrors, on device tensors:
    Net.forward                       tianshou/utils/net/common.py:343-369 (softmax over the atoms of each action)
    C51Policy.compute_q_value         tianshou/algorithm/modelfree/c51.py:66-67 (sum_j p_j z_j)
    C51._target_q / _preprocess_batch c51.py:120-121 (the n-step returns of the support: no network)
    C51._target_dist                  c51.py:123-141 (online network selects, lagged network evaluates, categorical projection)
    C51._update_with_batch            c51.py:143-160 (the periodic hard sync of dqn.py:277-285 comes BEFORE the target)
Setup: test/discrete/test_c51.py.  `update_with_batch` is two launches (ts_c51_mlp.hip): the target distribution is a phase of the
step kernel.  There is no CPU path: every function calls libtsengine.so.

`layers` = (obs_dim, trunk widths, n_act, n_atoms) and the flat layout are qrdqn_mlp's (a plain Net whose last Linear has
n_act * n_atoms outputs), so its converters, envelope checks and module walk serve here.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import qrdqn_mlp as Q
from . import vecq as V
from .buffer import DeviceReplayBuffer
from .dqn import DQNConfig
from .returns import nstep_coefficients

MAX_ATOMS = Q.MAX_ATOMS
ENVELOPE = (f"Net on vector observations of 1 .. {Q.MAX_OBS} entries, 1 .. {Q.MAX_TRUNK} hidden layers, widths multiples of 32 in "
            f"[32, {Q.MAX_WIDTH}], ReLU, no norm_layer, no dueling_param, softmax=True, concat=False, 1 .. {Q.MAX_ACTIONS} actions, "
            f"num_atoms 2 .. {MAX_ATOMS}, the activations and the three atom tables of a 32-row tile within 160 KB of LDS")
_F = V.Family("C51 MLP", ENVELOPE)

_desc = Q._desc
state_dict_keys, flat_from_torch, flat_to_torch = Q.state_dict_keys, Q.flat_from_torch, Q.flat_to_torch


def layout(layers, batch: int = 1) -> dict:
    """ts_c51_mlp_layout -> {count, lds_bytes, workspace_bytes}; NotImplementedError when the tile does not fit the LDS."""
    return _F.layout("ts_c51_mlp_layout", _desc(layers), batch)


def make_layers(obs_dim, trunk, n_act, n_atoms) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    return Q._make_layers(_F, layout, obs_dim, trunk, n_act, n_atoms)      # (`layout`: the carve with three tables)


def support(v_min: float, v_max: float, n_atoms: int, device) -> torch.Tensor:
    """c51.py:61-64: the atoms, in torch's own float32 arithmetic."""
    return torch.linspace(v_min, v_max, n_atoms).to(device).contiguous()


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module with `softmax=True` (common.py:286-341), or raises NotImplementedError naming what is
    not supported."""
    _F.require_net(net)
    if not net.softmax:
        raise _F.refuse("softmax=True is needed (QRDQN on a Net is qrdqn_mlp's)")
    if net.use_dueling:
        raise _F.refuse("dueling_param with atoms is not supported")
    n_atoms = int(net.num_atoms)
    _F.in_range("num_atoms", n_atoms, 2, MAX_ATOMS)
    return Q._describe_plain(_F, make_layers, net, n_atoms)


class C51MlpEngine(V.VecQEngine):
    """State of one C51 learner on one GPU: flat parameters, lagged copy, Adam moments, counters, the support.  `cfg` is a DQNConfig
    (`is_double` and `huber_delta` are not read: the online network always selects, c51.py:124-131, and the loss is a cross-entropy)."""

    FAMILY = _F

    def __init__(self, layers, flat_params: torch.Tensor, cfg: DQNConfig, v_min: float = -10.0, v_max: float = 10.0):
        self._require_device(flat_params)
        self._check_support(v_min, v_max)
        layers = make_layers(*layers)
        super().__init__(layers, _desc(layers), layout(layers)["count"], flat_params, cfg)
        _, _, self.n_act, self.n_atoms = layers
        self._set_support(v_min, v_max)

    @staticmethod
    def _check_support(v_min, v_max) -> None:
        if not v_min < v_max:
            raise ValueError(f"v_max must be larger than v_min, got {v_min=} and {v_max=}")

    def _set_support(self, v_min, v_max) -> None:
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.delta_z = (self.v_max - self.v_min) / (self.n_atoms - 1)                      # c51.py:118
        self.support = support(self.v_min, self.v_max, self.n_atoms, self.device)

    def _z(self):
        return _lib.ptr(self.support), self.v_min, self.v_max, self.delta_z

    # -- Net.forward + C51Policy.compute_q_value + the greedy action -------------------------------------------------------------
    def forward(self, obs, params: torch.Tensor | None = None):
        """-> (dist float32[B, A, N] probabilities, q float32[B, A] = sum_j p_j z_j, act int64[B] = argmax, the first index on ties)."""
        obs = self._obs(obs)
        b = obs.shape[0]
        dist = torch.empty((b, self.n_act, self.n_atoms), dtype=torch.float32, device=self.device)
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_c51_mlp_forward(_lib.ptr(self.params if params is None else params), self._d, _lib.ptr(self.support),
                                                  _lib.ptr(obs), _lib.i64(b), _lib.ptr(dist), _lib.ptr(q), _lib.ptr(act),
                                                  _lib.current_stream(self.device)))
        return dist, q, act

    # -- C51._target_q + compute_nstep_return --------------------------------------------------------------------------------------
    def support_returns(self, buffer: DeviceReplayBuffer, indices, coef=None) -> torch.Tensor:
        """The n-step returns of the support, float32[I, N] = float(double(z_j mask) gamma^n + sum gamma^k r): `_target_q` is the
        support itself (c51.py:120-121), so no network is read."""
        mask, gpow, mc = coef if coef is not None else nstep_coefficients(buffer, indices, self.cfg.gamma, self.cfg.n_step)
        return ((self.support.view(1, -1) * mask.view(-1, 1)).double() * gpow.view(-1, 1) + mc.view(-1, 1)).float()

    # -- C51._preprocess_batch ---------------------------------------------------------------------------------------------------
    def preprocess_with_obs(self, buffer: DeviceReplayBuffer, obs_rows: torch.Tensor, indices, stack_num: int = 1,
                            obs_next_rows: torch.Tensor | None = None, coef=None):
        """-> (batch.obs float32[I, obs_dim], batch.obs_next float32[I, obs_dim], returns float32[I, N]).  obs_next is the ONE-step
        batch.obs_next (buffer_base.py:624-626): `_target_dist` reads it inside the update."""
        pair = self._obs_pair(buffer, obs_rows, indices, 1, obs_next_rows, None, stack_num)
        return self._obs(pair[0]), self._obs(pair[1]), self.support_returns(buffer, indices, coef)

    def _returns(self, returns, b):
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).contiguous()
        if tuple(returns.shape) != (b, self.n_atoms):
            raise ValueError(f"returns must be [{b}, {self.n_atoms}]")
        return returns

    def _lagged(self):
        """The network `_target_dist` evaluates at this call: the sync comes first (c51.py:147-149), so on a sync iteration it is
        the online one."""
        return None if self._sync_now() else self.params_old

    def _update_args(self, obs, act, obs_next, returns, weight, grad_out, target_out):
        """The argument checks of `update_with_batch` (RainbowMlpEngine's too) -> the converted (obs, act, obs_next, returns, weight)."""
        obs, obs_next = self._obs(obs), self._obs(obs_next)
        b = obs.shape[0]
        returns = self._returns(returns, b)
        if obs_next.shape[0] != b:
            raise ValueError(f"act and obs_next must hold {b} rows")
        act, weight = self._batch_args(b, act, weight, grad_out)
        if target_out is not None and (tuple(target_out.shape) != (b, self.n_atoms) or target_out.dtype != torch.float32
                                       or not target_out.is_contiguous()):
            raise ValueError(f"target_out must be a contiguous float32 [{b}, {self.n_atoms}]")
        return obs, act, obs_next, returns, weight

    # -- C51._target_dist ----------------------------------------------------------------------------------------------------------
    def target_dist(self, obs_next, returns) -> torch.Tensor:
        """The target distribution the next `update_with_batch` would build -> float32[B, N]; changes no state."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        returns = self._returns(returns, b)
        out = torch.empty((b, self.n_atoms), dtype=torch.float32, device=self.device)
        z, v_min, v_max, dz = self._z()
        _lib.check(_lib.load().ts_c51_mlp_target_dist(_lib.ptr(self.params), _lib.ptr(self._lagged()), self._d, z, v_min, v_max, dz,
                                                      _lib.ptr(obs_next), _lib.ptr(returns), _lib.i64(b), _lib.ptr(out),
                                                      _lib.current_stream(self.device)))
        return out

    # -- the two halves of an update ---------------------------------------------------------------------------------------------
    def gradient(self, obs, act, obs_next, returns, weight, grad_out: torch.Tensor, target_out: torch.Tensor | None = None):
        """Periodic target sync + target + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, prio)."""
        return self.update_with_batch(obs, act, obs_next, returns, weight, grad_out=grad_out, apply=False, target_out=target_out)

    # -- C51._update_with_batch ----------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, obs_next, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True,
                          target_out: torch.Tensor | None = None):
        """-> (loss float32[1] device tensor, prio float32[B]); prio is the new batch.weight (c51.py:157).  On every
        target_update_freq-th call, the first included, the target is read from the current parameters and the lagged network takes
        the pre-step parameters inside the call.  A refused argument leaves the lagged network and both counters alone."""
        obs, act, obs_next, returns, weight = self._update_args(obs, act, obs_next, returns, weight, grad_out, target_out)
        b = obs.shape[0]
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = self.cfg.to_c(grad_only=not apply)
        z, v_min, v_max, dz = self._z()
        _lib.check(_lib.load().ts_c51_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(self._sync_now())), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), self._adam_arg(apply), self._d, z, v_min, v_max, dz, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(obs_next),
            _lib.ptr(returns), _lib.ptr(weight), _lib.i64(b), C.byref(hp), _lib.ptr(loss), _lib.ptr(prio), _lib.ptr(grad_out),
            _lib.ptr(target_out), _lib.current_stream(self.device)))
        self._stepped(apply)
        return loss, prio
