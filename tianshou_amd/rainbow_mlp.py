"""Rainbow on vector observations (`Net(softmax=True, num_atoms=N, dueling_param=(Q, V))` with NoisyLinear or plain Linear streams)
on the MI355X engine.

Mirrors, on device tensors:
    Net.forward                        tianshou/utils/net/common.py:343-369 (dueling over the atoms: q - mean_a q + v, then softmax)
    NoisyLinear.forward                tianshou/utils/net/discrete.py:366-374 (mu + sigma * eps_q.ger(eps_p), composed per call)
    C51._target_dist / _update_with_batch   c51.py:123-160, as tianshou_amd.c51_mlp
    RainbowDQN._update_with_batch      rainbow.py:93-101 (both networks' noise is drawn first: the caller's `set_noise`)
Setup: test/discrete/test_rainbow.py.  `update_with_batch` is two launches (ts_rainbow_mlp.hip).  There is no CPU path: every function
calls libtsengine.so.

`layers` = (obs_dim, trunk widths, Q hidden widths, V hidden widths, n_act, n_atoms, noisy).  Flat layout (ts_rainbow_mlp_layout): the
trunk layers [K + 1, width] (row K the bias), then the Q stream, then the V stream; a stream layer of a noisy network is its mu block
[K + 1, width] followed by its sigma block.  The noise is a separate vector per network: per stream layer eps_p[K] then eps_q[width].
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import c51_mlp as C5
from . import qrdqn_mlp as Q
from . import vecq as V
from .dqn import DQNConfig

MAX_ATOMS, MAX_STREAM = Q.MAX_ATOMS, 1
ENVELOPE = (f"Net on vector observations of 1 .. {Q.MAX_OBS} entries, 1 .. {Q.MAX_TRUNK} trunk hidden layers, dueling_param with 0 .. "
            f"{MAX_STREAM} hidden layer in each of Q and V, both streams all NoisyLinear or all nn.Linear, widths multiples of 32 in "
            f"[32, {Q.MAX_WIDTH}], ReLU, no norm_layer, softmax=True, concat=False, 1 .. {Q.MAX_ACTIONS} actions, num_atoms 2 .. "
            f"{MAX_ATOMS}, the activations, four atom tables and staged noise of a 32-row tile within 160 KB of LDS")
_F = V.Family("Rainbow MLP", ENVELOPE)
_NOISY, _PLAIN = ("mu_W", "sigma_W", "mu_bias", "sigma_bias"), ("weight", "bias")

support = C5.support


def make_layers(obs_dim, trunk, q_hidden, v_hidden, n_act, n_atoms, noisy) -> tuple:
    """The model description every function here takes; raises NotImplementedError, naming the reason, outside the envelope."""
    trunk, q, v = (tuple(int(w) for w in t) for t in (trunk, q_hidden, v_hidden))
    obs_dim, n_act, n_atoms = int(obs_dim), int(n_act), int(n_atoms)
    _F.in_range("obs_dim", obs_dim, 1, Q.MAX_OBS)
    _F.count(len(trunk), "trunk hidden layers", 1, Q.MAX_TRUNK)
    if len(q) > MAX_STREAM or len(v) > MAX_STREAM:
        raise _F.refuse(f"Q / V streams with {len(q)} / {len(v)} hidden layers (0 .. {MAX_STREAM})")
    _F.widths(trunk + q + v, Q.MAX_WIDTH)
    _F.count(n_act, "actions", 1, Q.MAX_ACTIONS)
    _F.in_range("num_atoms", n_atoms, 2, MAX_ATOMS)
    layers = (obs_dim, trunk, q, v, n_act, n_atoms, bool(noisy))
    layout(layers)                                     # the LDS carve of a tile is the library's arithmetic
    return layers


def _desc(layers):
    obs_dim, trunk, q, v, n_act, n_atoms, noisy = layers
    pad = lambda t, n: list(t) + [0] * (n - len(t))  # noqa: E731
    return (C.c_int64 * 16)(obs_dim, n_act, 1, len(trunk), len(q), len(v), *pad(trunk, 4), *pad(q, 2), *pad(v, 2), n_atoms, int(noisy))


def layout(layers, batch: int = 1) -> dict:
    """ts_rainbow_mlp_layout -> {count, lds_bytes, workspace_bytes, noise_count}; NotImplementedError when the tile does not fit the LDS."""
    return _F.layout("ts_rainbow_mlp_layout", _desc(layers), batch, noise_count=11)


def _blocks(layers) -> list:
    """[(state-dict prefix, K, width, noisy)] in flat order, which is Net.state_dict()'s (common.py:336-341: model, Q, V)."""
    obs_dim, trunk, q, v, n_act, n_atoms, noisy = layers
    out, k = [], obs_dim
    for i, n in enumerate(trunk):
        out.append((f"model.model.{2 * i}", k, n, False))
        k = n
    for name, widths, n_out in (("Q", q, n_act * n_atoms), ("V", v, n_atoms)):
        kin = k
        for i, n in enumerate(tuple(widths) + (n_out,)):
            out.append((f"{name}.model.{2 * i}", kin, n, noisy))
            kin = n
    return out


def state_dict_keys(layers) -> list[str]:
    """The trainable parameters, in `named_parameters()` order (eps_p / eps_q do not require grad: `noise_keys`)."""
    return [f"{p}.{s}" for p, _, _, nz in _blocks(layers) for s in (_NOISY if nz else _PLAIN)]


def noise_keys(layers) -> list[str]:
    return [f"{p}.{s}" for p, _, _, nz in _blocks(layers) if nz for s in ("eps_p", "eps_q")]


def flat_from_torch(tensors, *layers_and_device) -> torch.Tensor:
    """Tensors in `state_dict_keys` order (nn.Linear / NoisyLinear layout; parameters or their moments) -> the flat vector."""
    *layers, device = layers_and_device
    blocks, t, parts = _blocks(tuple(layers)), list(tensors), []
    if len(t) != sum(4 if nz else 2 for *_, nz in blocks):
        raise ValueError(f"Rainbow MLP: expected {sum(4 if nz else 2 for *_, nz in blocks)} tensors, got {len(t)}")
    for prefix, k, n, nz in blocks:
        ws, bs = (t[:2], t[2:4]) if nz else (t[:1], t[1:2])
        t = t[4 if nz else 2:]
        for w, b in zip(ws, bs):                       # mu block, then sigma block
            if tuple(w.shape) != (n, k) or b.numel() != n:
                raise ValueError(f"Rainbow MLP: {prefix} must map {k} -> {n}, got weight {tuple(w.shape)} and {b.numel()} biases")
            parts += [w.detach().float().cpu().t().reshape(-1), b.detach().float().cpu().reshape(-1)]
    return torch.cat(parts).to(device).contiguous()


def flat_to_torch(flat: torch.Tensor, *layers) -> list[torch.Tensor]:
    """Inverse of flat_from_torch -> tensors in `state_dict_keys` order (on flat's device)."""
    f, off, out = flat.detach(), 0, []
    for _, k, n, nz in _blocks(tuple(layers)):
        ws, bs = [], []
        for _ in range(2 if nz else 1):
            ws.append(f[off:off + k * n].reshape(k, n).t().contiguous())
            bs.append(f[off + k * n:off + (k + 1) * n].clone())
            off += (k + 1) * n
        out += ws + bs
    if off != f.numel():
        raise ValueError(f"Rainbow MLP: the flat vector has {f.numel()} entries, the layout {off}")
    return out


def noise_from_torch(tensors, *layers_and_device) -> torch.Tensor:
    """[eps_p, eps_q, ...] in `noise_keys` order -> the engine's noise vector (empty for plain streams)."""
    *layers, device = layers_and_device
    t = [torch.as_tensor(x).detach().float().reshape(-1) for x in tensors]
    want = [d for _, k, n, nz in _blocks(tuple(layers)) if nz for d in (k, n)]
    if [x.numel() for x in t] != want:
        raise ValueError(f"Rainbow MLP: the noise vectors must have {want} entries, got {[x.numel() for x in t]}")
    return torch.cat(t).to(device).contiguous() if t else torch.empty(0, dtype=torch.float32, device=device)


def describe_module(net) -> tuple:
    """-> `layers` of a Net-shaped module with `softmax=True` and `dueling_param` (common.py:286-341), or raises NotImplementedError
    naming what is not supported."""
    _F.require_net(net, extra=("Q", "V"))
    if not net.softmax:
        raise _F.refuse("softmax=True is needed (dueling DQN on a Net is dqn_mlp's)")
    if not net.use_dueling:
        raise _F.refuse("dueling_param is needed (C51 on a plain Net is c51_mlp's)")
    n_atoms = int(net.num_atoms)
    _F.in_range("num_atoms", n_atoms, 2, MAX_ATOMS)

    def chain(mlp, who, ends_linear, kinds):
        """[layer, ReLU, layer, ReLU, ...(, layer)] -> [(in, out)] of the layers; `kinds`: the layer classes' names seen."""
        mods, dims = list(mlp.model.children()), []
        for j, m in enumerate(mods):
            if j % 2 == 1:
                if not isinstance(m, torch.nn.ReLU):
                    raise _F.refuse(f"the activation must be ReLU (found {type(m).__name__})", who)
            elif (isinstance(m, torch.nn.Linear) and m.bias is not None) or (who != "model" and hasattr(m, "mu_W") and hasattr(m, "eps_q")):
                kinds.add("noisy" if hasattr(m, "mu_W") else "plain")
                dims.append((m.in_features, m.out_features))
            else:
                raise _F.refuse(("Linear layers with bias" if who == "model" else "NoisyLinear or Linear layers with bias")
                                + f" followed by ReLU only, no norm_layer (found {type(m).__name__})", who)
        if ends_linear != (len(mods) % 2 == 1):
            raise _F.refuse("the last layer must map onto the outputs (concat=True is not supported)" if ends_linear
                            else "the trunk of a dueling Net ends in its last hidden layer", who)
        return dims

    kinds: set = set()
    trunk = chain(net.model, "model", False, set())
    if not trunk:
        raise _F.refuse("at least one trunk hidden layer is needed")
    q, v = chain(net.Q, "Q", True, kinds), chain(net.V, "V", True, kinds)
    if len(kinds) != 1:
        raise _F.refuse("both streams all NoisyLinear or all nn.Linear (found a mix)")
    if q[-1][1] % n_atoms or v[-1][1] != n_atoms:
        raise _F.refuse(f"Q must end in n_act * {n_atoms} outputs and V in {n_atoms}, found {q[-1][1]} and {v[-1][1]}")
    layers = make_layers(trunk[0][0], [d[1] for d in trunk], [d[1] for d in q[:-1]], [d[1] for d in v[:-1]], q[-1][1] // n_atoms, n_atoms,
                         kinds == {"noisy"})
    _F.same_parameters(net, state_dict_keys(layers), "a Net's", trainable_only=True)
    return layers


class RainbowMlpEngine(C5.C51MlpEngine):
    """State of one Rainbow learner on one GPU: C51MlpEngine's surface (flat parameters, lagged copy, Adam moments, counters, the
    support) plus one noise vector per network, set by `set_noise` before every update (rainbow.py:97-100)."""

    FAMILY = _F

    def __init__(self, layers, flat_params: torch.Tensor, noise: torch.Tensor | None, cfg: DQNConfig, v_min: float = -10.0, v_max: float = 10.0):
        self._require_device(flat_params)
        self._check_support(v_min, v_max)
        layers = make_layers(*layers)
        lay = layout(layers)
        V.VecQEngine.__init__(self, layers, _desc(layers), lay["count"], flat_params, cfg)      # (lagged: deepcopy, weights and noise)
        self.n_act, self.n_atoms, self.noisy, self.n_noise = layers[4], layers[5], layers[6], lay["noise_count"]
        self.noise = self.noise_old = None
        if self.noisy:
            if noise is None or noise.numel() != self.n_noise:
                raise ValueError(f"expected a noise vector of {self.n_noise} entries")
            self.noise = noise.detach().float().to(self.device).contiguous().clone()
            self.noise_old = self.noise.clone() if self.params_old is not None else None
        self._set_support(v_min, v_max)

    def set_noise(self, noise: torch.Tensor, noise_old: torch.Tensor | None = None) -> None:
        """The result of RainbowDQN._sample_noise on the online (and the lagged) network; nothing to set for plain streams."""
        if not self.noisy:
            return
        self.noise.copy_(torch.as_tensor(noise).to(self.device).reshape(-1))
        if noise_old is not None and self.noise_old is not None:
            self.noise_old.copy_(torch.as_tensor(noise_old).to(self.device).reshape(-1))

    # -- Net.forward + C51Policy.compute_q_value + the greedy action -------------------------------------------------------------
    def forward(self, obs, training: bool = True):
        """-> (dist float32[B, A, N] probabilities, q float32[B, A] = sum_j p_j z_j, act int64[B] = argmax, the first index on ties);
        training=False: eval-mode layers, the noise is not read."""
        obs = self._obs(obs)
        b = obs.shape[0]
        dist = torch.empty((b, self.n_act, self.n_atoms), dtype=torch.float32, device=self.device)
        q = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        act = torch.empty(b, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ts_rainbow_mlp_forward(_lib.ptr(self.params), _lib.ptr(self.noise if training else None), self._d,
                                                      _lib.ptr(self.support), _lib.ptr(obs), _lib.i64(b), _lib.ptr(dist), _lib.ptr(q),
                                                      _lib.ptr(act), _lib.current_stream(self.device)))
        return dist, q, act

    # -- C51._target_dist ----------------------------------------------------------------------------------------------------------
    def target_dist(self, obs_next, returns) -> torch.Tensor:
        """The target distribution the next `update_with_batch` would build -> float32[B, N]; changes no state."""
        obs_next = self._obs(obs_next)
        b = obs_next.shape[0]
        returns = self._returns(returns, b)
        out = torch.empty((b, self.n_atoms), dtype=torch.float32, device=self.device)
        z, v_min, v_max, dz = self._z()
        _lib.check(_lib.load().ts_rainbow_mlp_target_dist(
            _lib.ptr(self.params), _lib.ptr(self.noise), _lib.ptr(self._lagged()), _lib.ptr(self.noise_old), self._d, z, v_min, v_max, dz,
            _lib.ptr(obs_next), _lib.ptr(returns), _lib.i64(b), _lib.ptr(out), _lib.current_stream(self.device)))
        return out

    # -- RainbowDQN._update_with_batch, once the noise is set ------------------------------------------------------------------------
    def update_with_batch(self, obs, act, obs_next, returns, weight=None, grad_out: torch.Tensor | None = None, apply: bool = True,
                          target_out: torch.Tensor | None = None):
        """As C51MlpEngine.update_with_batch.  On a sync iteration the lagged network takes the pre-step parameters inside the call
        and the lagged noise takes the online noise (load_state_dict copies the eps vectors too)."""
        obs, act, obs_next, returns, weight = self._update_args(obs, act, obs_next, returns, weight, grad_out, target_out)
        b, sync = obs.shape[0], self._sync_now()
        prio = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        hp = self.cfg.to_c(grad_only=not apply)
        z, v_min, v_max, dz = self._z()
        _lib.check(_lib.load().ts_rainbow_mlp_update(
            self._ws.handle, _lib.ptr(self.params), _lib.ptr(self.noise), _lib.ptr(self.params_old), _lib.ptr(self.noise_old),
            C.c_int32(int(sync)), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v), self._adam_arg(apply), self._d, z, v_min, v_max, dz,
            _lib.ptr(obs), _lib.ptr(act), _lib.ptr(obs_next), _lib.ptr(returns), _lib.ptr(weight), _lib.i64(b), C.byref(hp), _lib.ptr(loss),
            _lib.ptr(prio), _lib.ptr(grad_out), _lib.ptr(target_out), _lib.current_stream(self.device)))
        if sync and self.noise_old is not None:
            self.noise_old.copy_(self.noise)
        self._stepped(apply)
        return loss, prio
