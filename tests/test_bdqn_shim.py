"""CPU: the HipBDQN drop-in without a GPU -- the stand-ins of tests/standin_bdqn.py against the real classes (where the reference
is mounted), the hook bodies over an engine double (call order, data in and out, lagged sync, write-back), every refusal of the
envelope, and the C ABI's argument checks (made before any launch, so a GPU-less host can make them)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import bdqn_common as BC
from tests import oracle_bdqn as OB
from tests import standin_bdqn as SM
from tianshou_amd import _lib
from tianshou_amd import bdqn as BD
from tianshou_amd.build import build_library
from tianshou_amd.integration import make_hip_bdqn


def standin_net(dims, **kw):
    obs_dim, common, hv, ha, D, A, act = dims
    args = dict(state_shape=obs_dim, num_branches=D, action_per_branch=A, common_hidden_sizes=list(common),
                value_hidden_sizes=[hv] if hv else [], action_hidden_sizes=[ha] if ha else [],
                activation=nn.ReLU if act == "relu" else nn.Tanh)
    args.update(kw)
    return SM.BranchingNet(**args)


# ---- the stand-ins against the real classes -----------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("tag", BC.TAGS)
def test_standins_have_the_reference_surface(tag):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.bdqn import BDQN, BDQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import BranchingNet

    dims = BC.dims_of(BC.load(tag))
    obs_dim, common, hv, ha, D, A, act = dims
    real = BranchingNet(state_shape=obs_dim, num_branches=D, action_per_branch=A, common_hidden_sizes=list(common),
                        value_hidden_sizes=[hv] if hv else [], action_hidden_sizes=[ha] if ha else [],
                        activation=nn.ReLU if act == "relu" else nn.Tanh)
    mine = standin_net(dims)
    assert list(real.state_dict()) == list(mine.state_dict()) == BD.state_keys(dims) == OB.state_keys(dims)
    assert {k: tuple(v.shape) for k, v in real.state_dict().items()} == OB.shapes(dims)
    assert BD.describe_model(real)["dims"] == BD.describe_model(mine)["dims"] == dims
    mine.load_state_dict(real.state_dict())
    x = torch.randn(3, obs_dim)
    assert torch.equal(real(x)[0], mine(x)[0])
    for freq in (0, 2):
        r = BDQN(policy=BDQNPolicy(model=real, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=1e-3), gamma=0.9,
                 target_update_freq=freq, is_double=False)
        s = SM.BDQN(policy=SM.BDQNPolicy(mine), lr=1e-3, gamma=0.9, target_update_freq=freq, is_double=False)
        for name in ("gamma", "n_step", "target_update_freq", "is_double", "_iter"):
            assert getattr(r, name) == getattr(s, name), name
        assert (r.model_old is None) == (s.model_old is None) == (freq == 0)
        if freq:
            assert list(dict(r.model_old.module.named_parameters())) == list(dict(s.model_old.module.named_parameters()))
        assert [k for k in r.state_dict() if k != "_optimizers"] == [k for k in s.state_dict() if k != "_optimizers"]
        assert type(r.optim._optim).__name__ == type(s.optim._optim).__name__ == "Adam" and r.optim._max_grad_norm == s.optim._max_grad_norm
    # the discount the reference's targets use: `_preprocess_batch` calls `_compute_return` without `gamma`
    sig_r, sig_s = inspect.signature(BDQN._compute_return), inspect.signature(SM.BDQN._compute_return)
    assert list(sig_r.parameters) == list(sig_s.parameters) and sig_r.parameters["gamma"].default == sig_s.parameters["gamma"].default == 0.99
    assert "gamma" not in inspect.getsource(BDQN._preprocess_batch)
    assert make_hip_bdqn()(policy=BDQNPolicy(model=real, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=1e-3),
                           device="cpu")._hip_desc["dims"] == dims


# ---- the hook bodies over an engine double ------------------------------------------------------------------------------------
class FakeEngine:
    """Records the calls; `update` adds 1 to every parameter and fills the optimizer state with recognisable values."""
    calls: list = []

    def __init__(self, *args):
        *dims, params, cfg = args
        self.dims, self.cfg = BD.make_dims(*dims), cfg
        self.D, self.A = self.dims[4], self.dims[5]
        self.params = params.clone()
        self.params_old = params.clone() if cfg.target_update_freq > 0 else None
        self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(params), torch.zeros_like(params), 0, 0
        FakeEngine.calls.append(("init", cfg.gamma, cfg.target_update_freq, cfg.is_double, cfg.optimizer))

    def target_q(self, obs_next, rew, end):
        FakeEngine.calls.append(("target_q", np.asarray(obs_next).copy(), np.asarray(rew).copy(), np.asarray(end).copy()))
        return torch.arange(len(rew), dtype=torch.float32) + 0.5

    def update(self, obs, act, ret, weight):
        if self.params_old is not None and self.iter % self.cfg.target_update_freq == 0:
            self.params_old.copy_(self.params)
        self.iter += 1
        self.adam_step += 1
        FakeEngine.calls.append(("update", np.asarray(obs).copy(), np.asarray(act).copy(), ret.clone(), None if weight is None else weight.clone(),
                                 self.cfg.lr))
        mask = ~BD.padding_mask(self.dims)
        self.params[mask] += 1.0
        self.adam_m[mask], self.adam_v[mask] = 0.25, 0.5
        return torch.tensor([1.5]), -torch.arange(len(ret), dtype=torch.float32)


def make_algo(monkeypatch, g, **kw):
    import tianshou_amd.integration as I

    monkeypatch.setattr(I, "_require_gpu", lambda device, who: None)
    monkeypatch.setattr(BD, "BDQNEngine", FakeEngine)
    FakeEngine.calls = []
    dims, c = BC.dims_of(g), BC.cfg_of(g)
    net = standin_net(dims)
    args = dict(policy=SM.BDQNPolicy(net), lr=c["lr"], optim=(torch.optim.RMSprop, {}) if c["optimizer"] == "rmsprop" else None,
                gamma=float(g["cfg"][1]), target_update_freq=c["target_update_freq"], is_double=c["is_double"], device="cpu")
    args.update(kw)
    return make_hip_bdqn(ref=SM)(**args)


def make_buffer(g):
    from tests.test_gpu_bdqn import build_buffer

    return build_buffer(g)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hook_bodies_over_an_engine_double(monkeypatch, tag):
    g = BC.load(tag)
    dims = BC.dims_of(g)
    algo, buf = make_algo(monkeypatch, g), make_buffer(g)
    keys = OB.state_keys(dims)
    named = dict(algo.policy.model.named_parameters())
    start = {k: named[k].detach().clone() for k in keys}
    for u in range(2):
        idx = g[f"u{u}_indices"]
        buf.sample_indices = lambda n, idx=idx: idx.copy()
        algo.policy.is_within_training_step = True
        stats = algo.update(buf, len(idx))
        algo.policy.is_within_training_step = False
        kinds = [c[0] for c in FakeEngine.calls]
        assert kinds == ["init"] + ["target_q", "update"] * (u + 1)             # ONE target call, then ONE update call
        _, obs_next, rew, end = FakeEngine.calls[-2]
        assert np.array_equal(obs_next, g["obs_next"][idx]) and np.array_equal(rew, g["rew"][idx].astype(np.float32))
        assert np.array_equal(end, g[f"u{u}_end"])                              # done with the unfinished indices forced to true
        _, obs, act, ret, weight, lr = FakeEngine.calls[-1]
        assert np.array_equal(obs, g["obs"][idx]) and np.array_equal(act, g["act"][idx]) and act.dtype == np.int64
        assert torch.equal(ret, torch.arange(len(idx), dtype=torch.float32) + 0.5) and lr == BC.cfg_of(g)["lr"]
        if tag == "per":
            if u == 0:                                                          # (later ones follow the double's priorities)
                np.testing.assert_allclose(weight.numpy(), g["u0_is_weight"], rtol=1e-6)
            assert weight.dtype == torch.float32 and weight.shape == (len(idx),)
            i, w = buf.weight_updates[-1]
            np.testing.assert_allclose(w, np.arange(len(idx)) + BC.PER_EPS)       # the signed priorities: the buffer takes abs
        else:
            assert weight is None
        assert stats.loss == 1.5 and algo._iter == u + 1
        for k in keys:                                                          # eager write-back after every update
            assert torch.allclose(named[k].detach(), start[k] + (u + 1), rtol=0, atol=1e-6)
    init = FakeEngine.calls[0]
    assert init[1:] == (float(g["cfg"][2]), BC.cfg_of(g)["target_update_freq"], BC.cfg_of(g)["is_double"], BC.cfg_of(g)["optimizer"])
    if algo.model_old is not None:                                              # freq 2: synchronised at update 0 only
        old = dict(algo.model_old.module.named_parameters())
        assert all(torch.equal(old[k].detach(), start[k]) for k in keys), "the lagged network moved"
    sd = algo.state_dict()
    st = algo.optim._optim.state[named[keys[0]]]
    second = "square_avg" if tag == "per" else "exp_avg_sq"
    assert float(st[second].flatten()[0]) == 0.5 and int(float(st["step"])) == 2 and len(sd["_optimizers"]) == 1
    if tag == "double":
        assert float(st["exp_avg"].flatten()[0]) == 0.25
    # a load drops the engine; the next update rebuilds it from the torch state (moments and counters included)
    algo.load_state_dict(sd)
    assert algo._hip_engine is None
    eng = algo._engine()
    assert eng.adam_step == 2 and eng.iter == 2 and float(eng.adam_v[~BD.padding_mask(dims)][0]) == 0.5
    assert torch.equal(torch.cat([t.reshape(-1) for t in BD.flat_to_torch(eng.params, *dims)]), torch.cat([named[k].detach().reshape(-1) for k in keys]))


def test_returns_are_an_expanded_view_and_b1_works(monkeypatch):
    g = BC.load("double")
    algo, buf = make_algo(monkeypatch, g), make_buffer(g)
    D, A = BC.dims_of(g)[4], BC.dims_of(g)[5]
    for idx in (g["u0_indices"], g["u0_indices"][:1]):
        batch = SM.Batch(obs=buf.obs[idx], act=buf.act[idx], rew=buf.rew[idx], obs_next=buf.obs_next[idx])
        out = algo._preprocess_batch(batch, buf, idx)
        assert out.returns.shape == (len(idx), D, A) and out.returns.stride() == (1, 0, 0)
        assert torch.equal(out.returns[:, 0, 0], torch.arange(len(idx), dtype=torch.float32) + 0.5)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
BASE = (5, (16,), 8, 8, 3, 4, "relu")


@pytest.mark.parametrize("what,build", [
    ("norm_layer", lambda: standin_net(BASE, norm_layer=nn.LayerNorm)),
    ("activation", lambda: standin_net(BASE, activation=nn.Sigmoid)),
    ("no activation", lambda: standin_net(BASE, activation=None)),
    ("deeper value", lambda: standin_net(BASE, value_hidden_sizes=[8, 8])),
    ("deeper branches", lambda: standin_net(BASE, action_hidden_sizes=[8, 8])),
    ("too many common layers", lambda: standin_net(BASE, common_hidden_sizes=[8] * 8)),
    ("too many branches", lambda: standin_net(BASE, num_branches=33)),
    ("too many actions", lambda: standin_net(BASE, action_per_branch=65)),
    ("too wide", lambda: standin_net(BASE, common_hidden_sizes=[1025])),
    ("not a BranchingNet", lambda: nn.Linear(5, 4)),
])
def test_everything_outside_the_envelope_is_refused(what, build):
    with pytest.raises(NotImplementedError, match="supported: BranchingNet with 1 .. 7 common hidden layers"):
        make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(build()), device="cpu")


def test_other_optimizers_are_refused():
    with pytest.raises(NotImplementedError, match="Adam and torch.optim.RMSprop"):
        make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(standin_net(BASE)), optim=(torch.optim.SGD, {}), device="cpu")
    with pytest.raises(NotImplementedError, match="one of"):
        BD.BDQNConfig(optimizer="sgd")
    make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(standin_net(BASE)), optim=(torch.optim.RMSprop, {"alpha": 0.95}), device="cpu")


def test_a_gamma_the_targets_do_not_use_is_announced():
    import warnings

    with pytest.warns(UserWarning, match="not used by the targets.*0.99"):
        make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(standin_net(BASE)), gamma=0.9, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(standin_net(BASE)), gamma=0.99, device="cpu")


def test_no_gpu_means_an_error_not_a_fallback():
    algo = make_hip_bdqn(ref=SM)(policy=SM.BDQNPolicy(standin_net(BASE)), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        algo._preprocess_batch(SM.Batch(), None, np.arange(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BD.BDQNEngine(*BASE, torch.zeros(BD.layout(BASE)[2]), BD.BDQNConfig())


def test_converters_round_trip_and_padding():
    for _, dims, _ in __import__("tests.bdqn_edge_cases", fromlist=["SHAPES"]).SHAPES:
        p = OB.random_params(dims, 1)
        keys = BD.state_keys(dims)
        flat = BD.flat_from_torch([p[k] for k in keys], *dims, "cpu")
        pad = BD.padding_mask(dims)
        assert not flat[pad].any() and int((~pad).sum()) == sum(v.numel() for v in p.values())
        assert all(torch.equal(t, p[k]) for t, k in zip(BD.flat_to_torch(flat, *dims), keys))
    with pytest.raises(ValueError, match="expected"):
        BD.flat_from_torch([], *BASE, "cpu")


# ---- the C ABI's argument checks, before any launch -----------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    i64, f64, d = C.c_int64, C.c_double, C.c_void_p(4096)
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    try:
        def net(hidden=(16,), act="relu", flags=0):
            n = _lib.NetDesc.make(5, list(hidden), act)
            n.flags = flags
            return n

        def forward(n=None, hv=8, ha=8, D=3, A=4, B=4, params=d, obs=d, q=d):
            n = n or net()
            return lib.ts_bdqn_forward(ws, params, C.byref(n), i64(hv), i64(ha), i64(D), i64(A), obs, i64(B), q, None, None)

        def update(B=4, step=1, kind=0, act=d, D=3, **kw):
            n = net()
            return lib.ts_bdqn_update(ws, d, d, d, i64(step), C.byref(n), i64(8), i64(8), i64(D), i64(4), d, act, d, None, i64(B), C.c_int32(kind),
                                      f64(1e-3), f64(0.9), f64(0.999), f64(1e-8), f64(0), f64(0.99), f64(0), C.c_int32(0), f64(0), d, d, None, None)

        def target_q(B=4, rew=d, D=3):
            n = net()
            return lib.ts_bdqn_target_q(ws, d, None, C.byref(n), i64(8), i64(8), i64(D), i64(4), d, rew, d, i64(B), f64(0.99), C.c_int32(1), d, None)

        for rc in (forward(params=None), forward(obs=None), forward(q=None), forward(B=0), forward(B=-3), forward(D=0), forward(A=0),
                   update(B=0), update(act=None), update(step=0), update(kind=2), target_q(B=0), target_q(rew=None),
                   lib.ts_bdqn_target(d, None, d, d, i64(4), i64(3), i64(4), f64(0.9), d, None),
                   lib.ts_bdqn_target(d, d, d, d, i64(0), i64(3), i64(4), f64(0.9), d, None),
                   lib.ts_bdqn_loss(ws, d, d, None, None, i64(4), i64(3), i64(4), d, d, None, None),
                   lib.ts_bdqn_loss(ws, d, d, d, None, i64(0), i64(3), i64(4), d, d, None, None),
                   lib.ts_bdqn_layout(None, i64(8), i64(8), i64(3), i64(4), (C.c_int64 * 8)())):
            assert rc == _lib.TS_ERR_INVALID_ARG, lib.ts_last_error()
        for rc in (forward(D=33), forward(A=65), forward(hv=1025), forward(ha=2000), forward(n=net(act="none")), forward(n=net(flags=2)),
                   forward(n=net(hidden=(16, 1025))), update(D=33), target_q(D=40),
                   lib.ts_bdqn_target(d, d, d, d, i64(4), i64(33), i64(4), f64(0.9), d, None),
                   lib.ts_bdqn_loss(ws, d, d, d, None, i64(4), i64(3), i64(65), d, d, None, None)):
            assert rc == _lib.TS_ERR_UNSUPPORTED, lib.ts_last_error()
        zero = net()
        zero.n_hidden = 0
        assert forward(n=zero) == _lib.TS_ERR_UNSUPPORTED and b"1 .. 7 hidden layers" in lib.ts_last_error()
        out = (C.c_int64 * 8)()
        n = net(hidden=(48, 40))
        assert lib.ts_bdqn_layout(C.byref(n), i64(24), i64(20), i64(3), i64(5), out) == 0
        assert int(out[0]) == BD.layout((5, (48, 40), 24, 20, 3, 5, "relu"))[2] and list(out)[2:5] == [128, 32, 32]
    finally:
        lib.ts_workspace_destroy(ws)
