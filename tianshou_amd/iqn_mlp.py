"""IQN on vector observations (`ImplicitQuantileNetwork` over the plain MLP `Net`) on the MI355X engine.

Mirrors, on device tensors:
    ImplicitQuantileNetwork.forward      tianshou/utils/net/discrete.py:200-216 (preprocess_net = Net, `last` = MLP(hidden_sizes))
    CosineEmbeddingNetwork.forward       discrete.py:144-160
    IQNPolicy.forward                    tianshou/algorithm/modelfree/iqn.py:72-100 (mean over the samples, argmax)
    QRDQN._target_q / _preprocess_batch  modelfree/qrdqn.py:94-106 (n-step via tianshou_amd.returns, on a [B, N'] target)
    IQN._update_with_batch               iqn.py:156-183 (+ periodic hard sync, dqn.py:277-285)
Setup: test/discrete/test_iqn.py.  `target_returns` is one launch, `update_with_batch` two (ts_iqn_mlp.hip).  There is no CPU
path: every function calls libtsengine.so.

`layers` = (obs_dim, trunk widths, feat, num_cosines, `last` hidden widths, n_act) describes the model everywhere.  `feat` is the
width of the Net's linear output layer (`Net(action_shape=F)`: the features are linear, as test_iqn.py builds them), or 0 when the
Net has none (`action_shape=0`: the features are its last ReLU layer).  Flat layout (ts_iqn_mlp_layout): per layer [K + 1, width],
row K the bias, in the order trunk | the Net's output layer | [We; be] | `last` hidden layers | final Linear.

Fractions: as tianshou_amd.iqn.  Every method takes them as optional float32 [B, N] tensors; None draws them from the engine's own
Philox stream (`cfg.seed`, `tau_counter`; `extra_state`).  The fractions a call used stay in `last_tau` (forward, update) and
`last_tau_online` / `last_tau_target` (target pass), so that a caller can replay them.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import vecq as V
from .buffer import DeviceReplayBuffer
from .iqn import IQNConfig, IQNEngine

MAX_OBS, MAX_TRUNK, MAX_LAST, MAX_WIDTH, MAX_ACTIONS, MAX_COS, MAX_SAMPLES, MAX_BATCH = 256, 4, 2, 256, 32, 64, 64, V.MAX_BATCH
ENVELOPE = (f"ImplicitQuantileNetwork(preprocess_net=Net, hidden_sizes, num_cosines) on vector observations of 1 .. {MAX_OBS} entries; "
            f"the Net with 1 .. {MAX_TRUNK} hidden layers, ReLU, no norm_layer, no dueling_param, softmax=False, num_atoms=1, "
            f"concat=False, with or without a Linear output layer; 0 .. {MAX_LAST} hidden layers in `last`; every width and the feature "
            f"width multiples of 32 in [32, {MAX_WIDTH}]; num_cosines 1 .. {MAX_COS}; 1 .. {MAX_ACTIONS} actions; sample counts 2 .. "
            f"{MAX_SAMPLES}; the activations and sample tables of a 32-row tile within 160 KB of LDS")


_F = V.Family("IQN MLP", ENVELOPE)


def _check_layers(fam: V.Family, max_last: int, obs_dim, trunk, feat, n_cos, hidden, n_act) -> tuple:
    """The envelope of a family on this module's network (here and fqf_mlp, whose `last` may be deeper), before the LDS check."""
    obs_dim, trunk, feat, n_cos = int(obs_dim), tuple(int(w) for w in trunk), int(feat or 0), int(n_cos)
    hidden, n_act = tuple(int(w) for w in hidden), int(n_act)
    fam.in_range("obs_dim", obs_dim, 1, MAX_OBS)
    fam.count(len(trunk), "hidden layers in the Net", 1, MAX_TRUNK)
    fam.count(len(hidden), "hidden layers in `last`", 0, max_last)
    fam.widths(trunk + hidden, MAX_WIDTH)
    if feat:
        fam.widths((feat,), MAX_WIDTH, "feature width")
    fam.in_range("num_cosines", n_cos, 1, MAX_COS)
    fam.count(n_act, "actions", 1, MAX_ACTIONS)
    return obs_dim, trunk, feat, n_cos, hidden, n_act


def make_layers(obs_dim, trunk, feat, n_cos, hidden, n_act) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    layers = _check_layers(_F, MAX_LAST, obs_dim, trunk, feat, n_cos, hidden, n_act)
    layout(layers)                                     # the LDS carve of a tile is the library's arithmetic
    return layers


def _desc(layers):
    obs_dim, trunk, feat, n_cos, hidden, n_act = layers
    return (C.c_int64 * 12)(obs_dim, n_act, len(trunk), *trunk, *([0] * (4 - len(trunk))), feat, n_cos, len(hidden), *hidden,
                            *([0] * (2 - len(hidden))))


def layout(layers, batch: int = 1) -> dict:
    """ts_iqn_mlp_layout -> {count, lds_bytes, workspace_bytes, F}; NotImplementedError when the tile does not fit the LDS."""
    return _F.layout("ts_iqn_mlp_layout", _desc(layers), batch, F=12)


def _blocks(layers):
    """-> ([(state-dict prefix, K, N)] in FLAT order, the same prefixes in state_dict() order: preprocess, last, embed_model)."""
    obs_dim, trunk, feat, n_cos, hidden, n_act = layers
    pre, k = [], obs_dim
    for i, n in enumerate(trunk + ((feat,) if feat else ())):
        pre.append((f"preprocess.model.model.{2 * i}", k, n))
        k = n
    emb = ("embed_model.net.0", n_cos, k)
    last = []
    for i, n in enumerate(hidden + (n_act,)):
        last.append((f"last.model.{2 * i}", k, n))
        k = n
    return pre + [emb] + last, [b[0] for b in pre + last + [emb]]


def state_dict_keys(layers) -> list[str]:
    """ImplicitQuantileNetwork.state_dict() order."""
    return [f"{p}.{s}" for p in _blocks(layers)[1] for s in ("weight", "bias")]


def flat_from_torch(tensors, *layers_and_device) -> torch.Tensor:
    """[w, b, ...] in `state_dict_keys` order (nn.Linear layout; parameters or their moments) -> the flat vector."""
    *layers, device = layers_and_device
    return _F.flat_from_torch(tensors, *_blocks(tuple(layers)), device)


def flat_to_torch(flat: torch.Tensor, *layers) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> tensors in `state_dict_keys` order (on flat's device)."""
    return _F.flat_to_torch(flat, *_blocks(tuple(layers)))


def describe_module(model, make=None, fam: V.Family = _F) -> tuple:
    """-> `layers` of an ImplicitQuantileNetwork-shaped module (`preprocess` = a Net, `last`, `embed_model`; discrete.py:163-198),
    or raises NotImplementedError naming what is not supported.  `make`, `fam`: the envelope check and the Family of a sibling with
    the same module shape (tianshou_amd.fqf_mlp), in place of `make_layers` and this module's."""
    for name in ("preprocess", "last", "embed_model"):
        if not hasattr(model, name):
            raise fam.refuse(f"an ImplicitQuantileNetwork is needed (found {type(model).__name__} without `{name}`)")
    net = model.preprocess
    fam.require_net(net, need="the preprocess_net must be a Net", hint="; the Atari trunk is tianshou_amd.iqn's")
    if net.softmax:
        raise fam.refuse("softmax=True is not supported")
    if net.use_dueling:
        raise fam.refuse("dueling_param is not supported")
    if int(net.num_atoms) != 1:
        raise fam.refuse(f"num_atoms = {net.num_atoms} is not supported")
    trunk, out = fam.chain(net.model.model, "preprocess_net")
    if not trunk:
        raise fam.refuse("the Net needs at least one hidden layer")
    hidden, head = fam.chain(model.last.model, "last")
    if head is None:
        raise fam.refuse("`last` must end in a Linear onto the actions")
    emb = list(model.embed_model.net.children())
    if len(emb) != 2 or not isinstance(emb[0], torch.nn.Linear) or not isinstance(emb[1], torch.nn.ReLU):
        raise fam.refuse("embed_model.net must be Sequential(Linear, ReLU)")
    layers = (make or make_layers)(trunk[0].in_features, [l.out_features for l in trunk], out.out_features if out is not None else 0,
                                   emb[0].in_features, [l.out_features for l in hidden], head.out_features)
    fam.same_parameters(model, state_dict_keys(layers), "those of an ImplicitQuantileNetwork on a Net (concat=True is not supported),")
    return layers


class IQNMlpEngine(V.VecQEngine):
    """State of one IQN learner on one GPU: flat parameters, lagged copy, Adam moments, counters (the fraction counter included).
    `cfg` is tianshou_amd.iqn's IQNConfig (`n_cos` is not read: the layers carry it)."""

    FAMILY = _F

    def __init__(self, layers, flat_params: torch.Tensor, cfg: IQNConfig):
        self._require_device(flat_params)
        for name in ("sample_size", "online_sample_size", "target_sample_size"):
            _F.in_range(name, getattr(cfg, name), 2, MAX_SAMPLES)
        layers = make_layers(*layers)
        super().__init__(layers, _desc(layers), layout(layers)["count"], flat_params, cfg)
        self.n_act = layers[5]
        self.tau_counter = 0
        self.last_tau = self.last_tau_online = self.last_tau_target = None

    draw, _tau, extra_state, load_extra_state = IQNEngine.draw, IQNEngine._tau, IQNEngine.extra_state, IQNEngine.load_extra_state

    # -- ImplicitQuantileNetwork.forward + IQNPolicy.forward ------------------------------------------------------------------------
    def forward(self, obs, tau=None, sample_size: int | None = None, params: torch.Tensor | None = None):
        """-> (logits float32[B, A, N], q float32[B, A] = mean over the samples, act int64[B] = argmax, the first index on ties);
        the fractions used are `self.last_tau`.  sample_size defaults to cfg.sample_size."""
        obs = self._obs(obs)
        b = obs.shape[0]
        tau = self._tau(tau, b, sample_size if tau is not None else (sample_size or self.cfg.sample_size))
        n = tau.shape[1]
        logits = torch.empty((b, self.n_act, n), dtype=torch.float32, device=self.device)
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_iqn_mlp_forward(_lib.ptr(self.params if params is None else params), self._d, _lib.ptr(obs), _lib.i64(b),
                                                  _lib.ptr(tau), _lib.i64(n), _lib.ptr(logits), _lib.ptr(q), _lib.ptr(act),
                                                  _lib.current_stream(self.device)))
        self.last_tau = tau
        return logits, q, act

    # -- QRDQN._target_q -------------------------------------------------------------------------------------------------------------
    def target_returns(self, obs_next, coef, tau_online=None, tau_target=None) -> torch.Tensor:
        """`_target_q` on obs_next in one launch -> float32[B, N'] ([B, N] without a lagged network); with `coef`
        (returns.nstep_coefficients) the same launch ends in float(double(target * mask) * gamma^n + sum gamma^k r) per quantile.
        Draw order as the reference's (qrdqn.py:99-105): the online network's fractions first."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        tau_online = self._tau(tau_online, b, None if tau_online is not None else self.cfg.online_sample_size)
        two = self.params_old is not None
        tau_target = self._tau(tau_target, b, None if tau_target is not None else self.cfg.target_sample_size) if two else None
        n_out = tau_target.shape[1] if two else tau_online.shape[1]
        mask, gpow, mc = coef if coef is not None else (None, None, None)
        out = torch.empty((b, n_out), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ts_iqn_mlp_next_dist(
            _lib.ptr(self.params), _lib.ptr(self.params_old), self._d, _lib.ptr(obs_next), _lib.i64(b), _lib.ptr(tau_online),
            _lib.i64(tau_online.shape[1]), _lib.ptr(tau_target), _lib.i64(n_out), _lib.ptr(mask), _lib.ptr(gpow), _lib.ptr(mc),
            _lib.ptr(out), _lib.current_stream(self.device)))
        self.last_tau_online, self.last_tau_target = tau_online, tau_target
        return out

    def next_dist(self, obs_next, tau_online=None, tau_target=None) -> torch.Tensor:
        return self.target_returns(obs_next, None, tau_online, tau_target)

    # -- QRDQN._preprocess_batch -----------------------------------------------------------------------------------------------------
    def preprocess_with_obs(self, buffer: DeviceReplayBuffer, obs_rows: torch.Tensor, indices, stack_num: int = 1,
                            obs_next_rows: torch.Tensor | None = None, prefetch: bool = False, pair=None, coef=None,
                            tau_online=None, tau_target=None):
        """-> (batch.obs float32[I, obs_dim], returns float32[I, N']): as DQNMlpEngine.preprocess_with_obs (both observation gathers
        from one launch, the n-step coefficients, then target + returns in one launch)."""
        return self._preprocess(buffer, obs_rows, indices, stack_num, obs_next_rows, pair, coef, tau_online, tau_target)

    # -- the two halves of an update -------------------------------------------------------------------------------------------------
    def gradient(self, obs, act, returns, weight, grad_out: torch.Tensor, tau=None):
        """Periodic target sync + forward + loss + backward; grad_out[:P] = d loss / d params, no optimizer step -> (loss, prio)."""
        return self.update_with_batch(obs, act, returns, weight, tau=tau, grad_out=grad_out, apply=False)

    # -- IQN._update_with_batch ------------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, tau=None, grad_out: torch.Tensor | None = None, apply: bool = True):
        """-> (loss float32[1] device tensor, prio float32[B]); prio is the new batch.weight (iqn.py:180).  returns float32[B, N'];
        tau float32[B, N] (None: drawn, N = cfg.online_sample_size).  The lagged network takes the pre-step parameters inside the
        call (every target_update_freq-th call, the first included).  A refused argument leaves the lagged network and the
        counters alone."""
        obs = self._obs(obs)
        b = obs.shape[0]
        act, weight = self._batch_args(b, act, weight, grad_out)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).contiguous()
        if returns.dim() != 2 or returns.shape[0] != b or not 2 <= returns.shape[1] <= MAX_SAMPLES:
            raise ValueError(f"returns must be [{b}, N'], 2 <= N' <= {MAX_SAMPLES}")
        tau = self._tau(tau, b, None if tau is not None else self.cfg.online_sample_size)
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = self.cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_iqn_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(self._sync_now())), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), self._adam_arg(apply), self._d, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(tau), _lib.i64(tau.shape[1]),
            _lib.ptr(returns), _lib.i64(returns.shape[1]), _lib.ptr(weight), _lib.i64(b), C.byref(hp), _lib.ptr(loss), _lib.ptr(prio),
            _lib.ptr(grad_out), _lib.current_stream(self.device)))
        self.last_tau = tau
        self._stepped(apply)
        return loss, prio
