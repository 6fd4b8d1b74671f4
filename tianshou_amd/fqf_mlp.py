"""FQF on vector observations (`FullQuantileFunction` over the plain MLP `Net`, with a `FractionProposalNetwork`) on the MI355X engine.

Mirrors, on device tensors:
    FractionProposalNetwork.forward      tianshou/utils/net/discrete.py:239-252 (on the detached features)
    FullQuantileFunction.forward         discrete.py:293-314 (the walk of tianshou_amd.iqn_mlp at tau_hats, and at taus[:, 1:-1])
    FQFPolicy.forward                    tianshou/algorithm/modelfree/fqf.py:66-106 (q weighted by taus[j + 1] - taus[j], argmax)
    FQF._target_q / _preprocess_batch    fqf.py:178-193 (n-step via tianshou_amd.returns, on a [B, N] target)
    FQF._update_with_batch               fqf.py:195-256 (+ periodic hard sync, dqn.py:277-285)
Setup: test/discrete/test_fqf.py.  `target_returns` is one launch, `update_with_batch` three (ts_fqf_mlp.hip).  There is no CPU
path: every function calls libtsengine.so.

`layers` is tianshou_amd.iqn_mlp's (obs_dim, trunk widths, feat, num_cosines, `last` hidden widths, n_act), here with up to three
hidden layers in `last`; `num_fractions` N goes beside it.  Two flat vectors: the model's in iqn_mlp's layout, the fraction
network's [F + 1, N] (row F the bias).

Fractions are not drawn: every call proposes them from the batch's own features.  The ones a call used stay in `last_taus` /
`last_tau_hats` (forward, update) and `last_target_taus` / `last_target_tau_hats` (target pass), so that a caller can replay them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from . import iqn_mlp as I
from . import vecq as V
from .distq import DistQHParams

MAX_LAST, MIN_FRACTIONS, MAX_FRACTIONS = 3, 2, 64
ENVELOPE = (f"FullQuantileFunction(preprocess_net=Net, hidden_sizes, num_cosines) + FractionProposalNetwork(num_fractions, F) on "
            f"vector observations of 1 .. {I.MAX_OBS} entries; the Net with 1 .. {I.MAX_TRUNK} hidden layers, ReLU, no norm_layer, no "
            f"dueling_param, softmax=False, num_atoms=1, concat=False, with or without a Linear output layer; 0 .. {MAX_LAST} hidden "
            f"layers in `last`; every width and the feature width F multiples of 32 in [32, {I.MAX_WIDTH}]; num_cosines 1 .. "
            f"{I.MAX_COS}; 1 .. {I.MAX_ACTIONS} actions; num_fractions {MIN_FRACTIONS} .. {MAX_FRACTIONS}; the fraction network one "
            f"Linear(F, num_fractions) with bias; the activations and fraction tables of a 32-row tile within 160 KB of LDS")
_F = V.Family("FQF MLP", ENVELOPE)


@dataclass
class FQFConfig:
    """Hyper-parameters of the reference FQF (fqf.py:112-170): Adam on the model (optim.py:89-110); the fraction optimizer's fields
    are `integration.optimizer_fields`' (Adam or RMSprop, optim.py:89-140), prefixed `f_`."""

    gamma: float = 0.99
    n_step: int = 1
    target_update_freq: int = 0
    ent_coef: float = 0.0
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None
    f_optimizer: str = "rmsprop"          # test_fqf.py: RMSpropOptimizerFactory
    f_lr: float = 2.5e-9
    f_betas: tuple[float, float] = (0.9, 0.999)
    f_adam_eps: float = 1e-8              # eps of either optimizer
    f_weight_decay: float = 0.0
    f_rms_alpha: float = 0.99
    f_rms_momentum: float = 0.0
    f_rms_centered: bool = False

    def to_c(self, grad_only: bool = False):
        """-> (ts_distq_hparams: the model's Adam; ts_ppo_hparams: the fraction optimizer's fields and ent_coef)."""
        if self.f_optimizer not in ("adam", "rmsprop"):
            raise NotImplementedError(f"FQF MLP: the fraction optimizer must be Adam or RMSprop, not {self.f_optimizer!r}")
        fhp = _lib.PPOHParams(ent_coef=self.ent_coef, lr=self.f_lr, beta1=self.f_betas[0], beta2=self.f_betas[1], adam_eps=self.f_adam_eps,
                              optimizer=int(self.f_optimizer == "rmsprop"), rms_centered=int(self.f_rms_centered),
                              weight_decay=self.f_weight_decay, rms_alpha=self.f_rms_alpha, rms_momentum=self.f_rms_momentum)
        return DistQHParams(-1.0 if grad_only else self.lr, self.betas[0], self.betas[1], self.adam_eps, self.max_grad_norm or 0.0, 0.0, 0.0), fhp


def make_layers(obs_dim, trunk, feat, n_cos, hidden, n_act, num_fractions=32) -> tuple:
    """iqn_mlp's model description under this module's envelope; raises NotImplementedError, naming the reason, outside it."""
    layers = I._check_layers(_F, MAX_LAST, obs_dim, trunk, feat, n_cos, hidden, n_act)
    _F.in_range("num_fractions", int(num_fractions), MIN_FRACTIONS, MAX_FRACTIONS)
    layout(layers, num_fractions)                  # the LDS carve of a tile is the library's arithmetic
    return layers


def _desc(layers, num_fractions):
    obs_dim, trunk, feat, n_cos, hidden, n_act = layers
    return (C.c_int64 * 14)(obs_dim, n_act, len(trunk), *trunk, *([0] * (4 - len(trunk))), feat, n_cos, len(hidden), *hidden,
                            *([0] * (3 - len(hidden))), num_fractions)


def layout(layers, num_fractions, batch: int = 1) -> dict:
    """ts_fqf_mlp_layout -> {count, fraction_count, lds_bytes, workspace_bytes, F}; NotImplementedError when the tile does not fit."""
    return _F.layout("ts_fqf_mlp_layout", _desc(layers, num_fractions), batch, fraction_count=1, lds_bytes=2, workspace_bytes=3, F=4)


state_dict_keys, flat_from_torch, flat_to_torch = I.state_dict_keys, I.flat_from_torch, I.flat_to_torch      # the model's: iqn_mlp's
FRACTION_KEYS = ["net.weight", "net.bias"]                                # FractionProposalNetwork.state_dict() order


def fraction_from_torch(tensors, feat: int, num_fractions: int, device) -> torch.Tensor:
    """[net.weight [N, F], net.bias [N]] (parameters or their moments) -> the flat [F + 1, N] vector."""
    w, b = tensors
    if tuple(w.shape) != (num_fractions, feat) or b.numel() != num_fractions:
        raise ValueError(f"FQF MLP: the fraction network must be Linear({feat}, {num_fractions}), got weight {tuple(w.shape)} and "
                         f"{b.numel()} biases")
    return torch.cat([w.detach().float().cpu().t().reshape(-1), b.detach().float().cpu().reshape(-1)]).to(device).contiguous()


def fraction_to_torch(flat: torch.Tensor, feat: int, num_fractions: int) -> list[torch.Tensor]:
    """Inverse of fraction_from_torch -> [weight [N, F], bias [N]] (on flat's device)."""
    f = flat.detach()
    if f.numel() != (feat + 1) * num_fractions:
        raise ValueError(f"FQF MLP: the fraction vector has {f.numel()} entries, the layout {(feat + 1) * num_fractions}")
    return [f[:feat * num_fractions].reshape(feat, num_fractions).t().contiguous(), f[feat * num_fractions:].clone()]


def describe_module(model, fraction_model) -> tuple:
    """-> (`layers`, num_fractions) of a FullQuantileFunction-shaped module and its FractionProposalNetwork (discrete.py:219-314), or
    raises NotImplementedError naming what is not supported."""
    net = getattr(fraction_model, "net", None)
    if not isinstance(net, torch.nn.Linear) or net.bias is None or [k for k, _ in fraction_model.named_parameters()] != FRACTION_KEYS:
        raise _F.refuse(f"the fraction network must be one Linear(F, num_fractions) with bias in `net` (found {type(net).__name__})")
    n = int(net.out_features)
    layers = I.describe_module(model, make=lambda *a: make_layers(*a, num_fractions=n), fam=_F)
    feat = layout(layers, n)["F"]
    if int(net.in_features) != feat:
        raise _F.refuse(f"the fraction network reads {net.in_features} features, the model has {feat}")
    return layers, n


class FQFMlpEngine(V.VecQEngine):
    """State of one FQF learner on one GPU: the model's flat parameters, lagged copy and Adam moments, the fraction network's flat
    parameters and optimizer state (`f_m`, `f_v`: ts_optim_step's mapping), and the counters."""

    FAMILY = _F

    def __init__(self, layers, num_fractions: int, flat_params: torch.Tensor, flat_fraction_params: torch.Tensor, cfg: FQFConfig):
        self._require_device(flat_params, flat_fraction_params)
        self.N = int(num_fractions)
        layers = make_layers(*layers, num_fractions=self.N)
        cfg.to_c()                                                       # refuses an unknown fraction optimizer
        lay = layout(layers, self.N)
        self.P2, self.F = lay["fraction_count"], lay["F"]
        if flat_params.numel() != lay["count"] or flat_fraction_params.numel() != self.P2:
            raise ValueError(f"expected {lay['count']} + {self.P2} parameters, got {flat_params.numel()} + {flat_fraction_params.numel()}")
        super().__init__(layers, _desc(layers, self.N), lay["count"], flat_params, cfg)      # (no lagged fraction network)
        self.n_act = layers[5]
        self.fparams = flat_fraction_params.detach().float().contiguous().clone()
        self.f_m, self.f_v = torch.zeros_like(self.fparams), torch.zeros_like(self.fparams)
        self.f_step = 0
        self.last_taus = self.last_tau_hats = self.last_entropies = self.last_target_taus = self.last_target_tau_hats = None

    def _stepped(self, apply: bool) -> None:
        super()._stepped(apply)
        if apply:
            self.f_step += 1

    def _fractions(self, b):
        return (torch.empty((b, self.N + 1), dtype=torch.float32, device=self.device),
                torch.empty((b, self.N), dtype=torch.float32, device=self.device))

    # -- FullQuantileFunction.forward + FQFPolicy.forward ---------------------------------------------------------------------------
    def forward(self, obs, fractions=None, want_quantiles_tau: bool = False, params: torch.Tensor | None = None):
        """-> (logits float32[B, A, N] at tau_hats, q float32[B, A] weighted by taus[j + 1] - taus[j], act int64[B], the first index
        on ties) and, with want_quantiles_tau, float32[B, A, N - 1] at taus[:, 1:-1] behind them.  `fractions` = (taus [B, N + 1],
        tau_hats [B, N]) replaces the proposal (the reference's `fractions=`); else `last_entropies` is the proposal's entropy.
        The fractions used are `last_taus` / `last_tau_hats`."""
        obs = self._obs(obs)
        b = obs.shape[0]
        given = None
        if fractions is not None:
            given = tuple(torch.as_tensor(t, device=self.device).to(torch.float32).contiguous() for t in fractions)
            if tuple(given[0].shape) != (b, self.N + 1) or tuple(given[1].shape) != (b, self.N):
                raise ValueError(f"fractions must be (taus [{b}, {self.N + 1}], tau_hats [{b}, {self.N}])")
        logits = torch.empty((b, self.n_act, self.N), dtype=torch.float32, device=self.device)
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        taus, tau_hats = self._fractions(b)
        ent = torch.empty(b, dtype=torch.float32, device=self.device) if given is None else None
        qtau = torch.empty((b, self.n_act, self.N - 1), dtype=torch.float32, device=self.device) if want_quantiles_tau else None
        _lib.check(_lib.load().ts_fqf_mlp_forward(
            _lib.ptr(self.params if params is None else params), _lib.ptr(self.fparams), self._d, _lib.ptr(obs), _lib.i64(b),
            _lib.ptr(given[0] if given else None), _lib.ptr(given[1] if given else None), _lib.ptr(logits), _lib.ptr(q), _lib.ptr(act),
            _lib.ptr(taus), _lib.ptr(tau_hats), _lib.ptr(ent), _lib.ptr(qtau), _lib.current_stream(self.device)))
        self.last_taus, self.last_tau_hats, self.last_entropies = taus, tau_hats, ent
        return (logits, q, act, qtau) if want_quantiles_tau else (logits, q, act)

    # -- FQF._target_q ---------------------------------------------------------------------------------------------------------------
    def target_returns(self, obs_next, coef) -> torch.Tensor:
        """`_target_q` on obs_next in one launch -> float32[B, N]; with `coef` (returns.nstep_coefficients) the same launch ends in
        float(double(target * mask) * gamma^n + sum gamma^k r) per quantile."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        mask, gpow, mc = coef if coef is not None else (None, None, None)
        out = torch.empty((b, self.N), dtype=torch.float32, device=self.device)
        taus, tau_hats = self._fractions(b)
        _lib.check(_lib.load().ts_fqf_mlp_next_dist(
            _lib.ptr(self.params), _lib.ptr(self.params_old), _lib.ptr(self.fparams), self._d, _lib.ptr(obs_next), _lib.i64(b),
            _lib.ptr(mask), _lib.ptr(gpow), _lib.ptr(mc), _lib.ptr(out), _lib.ptr(taus), _lib.ptr(tau_hats),
            _lib.current_stream(self.device)))
        self.last_target_taus, self.last_target_tau_hats = taus, tau_hats
        return out

    def next_dist(self, obs_next) -> torch.Tensor:
        return self.target_returns(obs_next, None)

    # -- QRDQN._preprocess_batch -----------------------------------------------------------------------------------------------------
    def preprocess_with_obs(self, buffer, obs_rows: torch.Tensor, indices, stack_num: int = 1, obs_next_rows: torch.Tensor | None = None,
                            pair=None, coef=None):
        """-> (batch.obs float32[I, obs_dim], returns float32[I, N]): as IQNMlpEngine.preprocess_with_obs (both gathers, the n-step coefficients), then target + returns in
        one launch."""
        return self._preprocess(buffer, obs_rows, indices, stack_num, obs_next_rows, pair, coef)

    # -- the two halves of an update -------------------------------------------------------------------------------------------------
    def gradient(self, obs, act, returns, weight, grad_out: torch.Tensor, fgrad_out: torch.Tensor):
        """Periodic target sync + forward + both losses + both backward passes; grad_out[:P] = d quantile_loss / d params, fgrad_out[:P2]
        = d (fraction_loss - ent_coef entropy_loss) / d fraction params; no optimizer step -> (losses, prio)."""
        return self.update_with_batch(obs, act, returns, weight, grad_out=grad_out, fgrad_out=fgrad_out, apply=False)

    # -- FQF._update_with_batch ------------------------------------------------------------------------------------------------------
    def update_with_batch(self, obs, act, returns, weight=None, grad_out=None, fgrad_out=None, apply: bool = True):
        """-> (losses float32[3] device tensor = quantile, fraction, entropy; prio float32[B]); prio is the new batch.weight
        (fqf.py:220).  returns float32[B, N].  The lagged network takes the pre-step parameters inside the call (every
        target_update_freq-th call, the first included).  A refused argument leaves the lagged network and the counters alone."""
        obs = self._obs(obs)
        b = obs.shape[0]
        act, weight = self._batch_args(b, act, weight, grad_out)
        returns = torch.as_tensor(returns, device=self.device).to(torch.float32).contiguous()
        if tuple(returns.shape) != (b, self.N):
            raise ValueError(f"returns must be [{b}, {self.N}]")
        if fgrad_out is not None and (fgrad_out.numel() != self.P2 or fgrad_out.dtype != torch.float32):
            raise ValueError("fgrad_out must be a float32 vector of the fraction network's size")
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        losses = torch.empty(3, dtype=torch.float32, device=self.device)
        taus, tau_hats = self._fractions(b)
        hp, fhp = self.cfg.to_c(grad_only=not apply)
        _lib.check(_lib.load().ts_fqf_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.params_old), C.c_int32(int(self._sync_now())), _lib.ptr(self.adam_m),
            _lib.ptr(self.adam_v), self._adam_arg(apply), _lib.ptr(self.fparams), _lib.ptr(self.f_m), _lib.ptr(self.f_v),
            _lib.i64(self.f_step + 1 if apply else max(self.f_step, 1)), self._d, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(returns),
            _lib.ptr(weight), _lib.i64(b), C.byref(hp), C.byref(fhp), _lib.ptr(losses), _lib.ptr(prio), _lib.ptr(grad_out), _lib.ptr(fgrad_out),
            _lib.ptr(taus), _lib.ptr(tau_hats), _lib.current_stream(self.device)))
        self.last_taus, self.last_tau_hats = taus, tau_hats
        self._stepped(apply)
        return losses, prio
