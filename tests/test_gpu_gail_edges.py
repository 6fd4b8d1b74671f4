"""GPU: the GAIL discriminator kernels at their edges -- the loss kernel alone (ts_gail_loss), one discriminator step's gradient
on both routes (ts_gail_disc_steps with lr < 0), the chunking rule, determinism and the refused arguments.  Inputs:
tests/gail_edge_cases.py, whose properties tests/test_gail_edge_inputs_cpu.py checks; reference: tests/oracle_gail.py in float64.

Bars (tests/test_gpu_npg.py::test_critic_step_vs_oracle, whose network code and reductions these kernels share): loss 1e-5
relative; gradient within 1e-5 of float64 or twice as close to it as the float32 oracle.  Accuracies are compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gail_edge_cases as E
from tests import oracle_gail as OG

pytestmark = pytest.mark.gpu
LOSS = E.loss_cases()
TS_ERR_INVALID_ARG, TS_ERR_UNSUPPORTED = -1, -4


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def make_engine(case, route="auto", num=None, **cfg):
    from tianshou_amd import gail as G

    c = G.GAILConfig(disc_update_num=num or case["num"], route=route, **cfg)
    flat = G.GAILDiscriminator.flat_from_tensors(case["t"], case["obs_dim"], case["act_dim"], case["hidden"])
    return G.GAILDiscriminator(case["obs_dim"], case["act_dim"], case["hidden"], case["activation"], flat, case["obs_exp"],
                               case["act_exp"], c)


# ---- the loss kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LOSS))
def test_loss_kernel_vs_float64(name):
    from tianshou_amd import gail as G

    l, n_pi, _ = LOSS[name]
    n_exp = l.numel() - n_pi
    st, d = G.loss(l.cuda(), n_pi)
    st, d = st.cpu(), d.cpu()
    st64, g64 = OG.loss_and_grad(l.double(), n_pi)
    print(name, "loss", float(st[0]), float(st64[0]), "acc", st[1:].tolist(), st64[1:].tolist())
    assert torch.isfinite(st).all() and torch.isfinite(d).all()
    assert abs(float(st[0]) - float(st64[0])) <= 1e-5 * abs(float(st64[0]))
    assert float(st[1]) == float(np.float32(float(st64[1]))) and float(st[2]) == float(np.float32(float(st64[2])))     # exact
    # every row carries its own side's 1 / n: |d| <= 1 / n, sign by side, and the float64 value within float32 rounding
    assert bool((d[:n_pi] >= 0).all()) and bool((d[n_pi:] <= 0).all())
    assert float(d[:n_pi].max()) <= 1.0 / n_pi * (1 + 1e-6) and float(-d[n_pi:].min()) <= 1.0 / n_exp * (1 + 1e-6)
    np.testing.assert_allclose(d.numpy(), g64.numpy(), rtol=1e-5, atol=1e-37)
    if name in E.SATURATED:
        z = torch.cat([l[:n_pi], -l[n_pi:]])
        w = torch.cat([torch.full((n_pi,), 1.0 / n_pi), torch.full((n_exp,), -1.0 / n_exp)])
        lose = z > 0
        assert torch.equal(d[lose], w[lose]) and bool((d[~lose].abs() <= 1e-38).all()) and bool((d[~lose & (z < -100)] == 0).all())
        # the loss is the mean |l| of the losing rows per side, to one ulp of the largest term
        want = float(z[:n_pi].clamp(min=0).double().mean() + z[n_pi:].clamp(min=0).double().mean())
        assert abs(float(st[0]) - want) <= 1.2e-7 * float(z.abs().max())


def test_zero_logits_count_for_neither_accuracy():
    from tianshou_amd import gail as G

    l, n_pi, _ = LOSS["zeros"]
    st, d = G.loss(l.cuda(), n_pi)
    assert st[1:].tolist() == [0.0, 0.0]
    assert abs(float(st[0]) - 2 * np.log(2.0)) <= 1e-5 * 2 * np.log(2.0)
    np.testing.assert_allclose(d.cpu().numpy(), [0.5 / 3] * 3 + [-0.5 / 3] * 3, rtol=1e-6)


# ---- one discriminator step, gradient only --------------------------------------------------------------------------------------
def _routes(name):
    return ["per_layer", "one_launch"] if E.one_launch_shape(E.STEP_CASES[name]) else ["per_layer"]


def _grad(case, route):
    eng = make_engine(case, route)
    before = eng.disc.clone()
    grad = torch.full((eng.count,), float("nan"), device="cuda")
    stats = eng.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"], grad_out=grad, apply=False)
    assert torch.equal(eng.disc, before) and eng.optim_step == 0 and not eng.state_m.any() and not eng.state_v.any()
    return eng, stats.cpu(), grad


@pytest.mark.parametrize("name", sorted(E.STEP_CASES))
def test_step_gradient_vs_oracle_on_every_route(name):
    case = E.step_case(name)
    st64, g64 = E.step_reference(case, torch.float64)
    st32, g32 = E.step_reference(case, torch.float32)
    grads = {}
    for route in _routes(name) + ["auto"]:
        eng, stats, grad = _grad(case, route)
        grads[route] = grad
        assert stats.shape == (len(case["chunks"]), 3)
        for k in range(stats.shape[0]):
            print(name, route, k, stats[k].tolist(), st64[k].tolist())
            assert abs(float(stats[k, 0]) - float(st64[k, 0])) <= 1e-5 * abs(float(st64[k, 0]))
            assert float(stats[k, 1]) == float(np.float32(float(st64[k, 1])))
            assert float(stats[k, 2]) == float(np.float32(float(st64[k, 2])))
        for i, t in enumerate(eng.to_tensors(grad)):                       # the last step's gradient
            e, e0 = rel_err(t.cpu(), g64[-1][i]), rel_err(g32[-1][i], g64[-1][i])
            print(name, route, "grad", i, e, e0)
            assert e < max(1e-5, 2 * e0), (name, route, i, e, e0)
        # padding entries of the gradient are exactly zero: what the unpadded tensors do not cover
        mask = eng.flat_from_tensors([torch.ones_like(x) for x in case["t"]], case["obs_dim"], case["act_dim"], case["hidden"])
        assert not grad[mask == 0].any() and torch.isfinite(grad).all()
    if "one_launch" in grads:                                               # the two routes agree within the same bar
        a, b = grads["one_launch"].cpu(), grads["per_layer"].cpu()
        assert rel_err(a, b) < 1e-5 or all(
            rel_err(x, z) < max(1e-5, 2 * rel_err(y, z))
            for x, y, z in zip(eng.to_tensors(grads["one_launch"].cpu()), g32[-1], g64[-1]))


def test_width_33_takes_the_per_layer_route_and_is_refused_on_the_one_launch_route():
    from tianshou_amd import _lib

    case = E.step_case("w33_64x64")
    _, st_auto, g_auto = _grad(case, "auto")
    _, st_pl, g_pl = _grad(case, "per_layer")
    assert torch.equal(g_auto, g_pl) and torch.equal(st_auto, st_pl)
    eng = make_engine(case, "one_launch")
    with pytest.raises(_lib.EngineError) as e:
        eng.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"], apply=False)
    assert e.value.code == TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.EngineError) as e:
        eng.reward(case["obs"], case["act"])
    assert e.value.code == TS_ERR_UNSUPPORTED


# ---- chunking -------------------------------------------------------------------------------------------------------------------
def test_38_rows_in_10_updates_are_12_steps_and_the_last_has_5_policy_rows():
    case = E.step_case("relu3")
    eng, stats, grad = _grad(case, "auto")
    assert stats.shape == (12, 3) and case["chunks"][-1] == (33, 38)
    # acc_pi of the last step is a multiple of 1 / 5, of every other step of 1 / 3 -- and the oracle's
    st64, _ = E.step_reference(case, torch.float64)
    assert float(stats[-1, 1]) in [float(np.float32(k / 5)) for k in range(6)]
    assert torch.equal(stats[:, 1:], st64[:, 1:].float())
    # the last step's policy rows carry 1 / 5: the head-bias gradient is sum(d_logit), policy part in (0, 1), expert part in (-1, 0)
    l_pi, l_exp = E.step_logits64(case)[-1]
    want = float(torch.sigmoid(l_pi).sum() / 5 - torch.sigmoid(-l_exp).sum() / 3)
    got = float(eng.to_tensors(grad)[-1].reshape(-1)[0])
    assert abs(got - want) <= 1e-5 * max(abs(want), 0.1)


def test_n_equal_num_gives_single_row_chunks_and_the_step_counter_advances_by_steps():
    case = E.step_case("relu3")
    eng = make_engine(case, num=38, lr=1e-3)
    ei = torch.arange(38) % case["obs_exp"].shape[0]
    stats = eng.disc_update(case["obs"], case["act"], case["perm"], ei)
    assert stats.shape == (38, 3) and eng.optim_step == 38
    assert set(stats[:, 1].cpu().tolist()) <= {0.0, 1.0}                    # one policy row per step
    eng2 = make_engine(case, num=10, lr=1e-3)
    eng2.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"])
    assert eng2.optim_step == 12                                            # steps, not disc_update_num
    eng2.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"])
    assert eng2.optim_step == 24


def test_steps_are_the_loop_of_single_steps():
    """12 steps in one call == the oracle's loop of 12 single Adam steps in float64, at the post-Adam bar."""
    case = E.step_case("relu3")
    lr = 1e-3
    eng = make_engine(case, lr=lr, max_grad_norm=0.5)
    stats = eng.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"]).cpu()
    opt = OG.Adam(lr=lr, max_grad_norm=0.5)
    t64, st64 = OG.disc_update([x.double() for x in case["t"]], opt, case["obs"].double(), case["act"].double(), case["perm"],
                               case["obs_exp"].double(), case["act_exp"].double(), case["exp_index"], case["num"], case["activation"])
    assert opt.step == 12
    np.testing.assert_allclose(stats[:, 0].numpy(), st64[:, 0].numpy(), rtol=1e-5)
    for t, r in zip(eng.to_tensors(), t64):
        np.testing.assert_allclose(t.cpu().numpy(), r.numpy(), rtol=1e-5, atol=0.02 * lr)


# ---- determinism and errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows70", "relu3"])
def test_same_call_twice_gives_the_same_bits(name):
    case = E.step_case(name)
    for route in _routes(name):
        out = []
        for _ in range(2):
            eng = make_engine(case, route, lr=1e-3)
            stats = eng.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"])
            out.append((stats.clone(), eng.disc.clone(), eng.state_m.clone(), eng.state_v.clone(), eng.reward(case["obs"], case["act"])))
        assert all(torch.equal(a, b) for a, b in zip(*out)), (name, route)


def test_refused_arguments_leave_the_state_untouched():
    from tianshou_amd import _lib

    case = E.step_case("rows33")
    eng = make_engine(case, lr=1e-3)
    lib = _lib.load()
    obs, act = case["obs"].cuda(), case["act"].cuda()
    perm, ei = case["perm"].cuda(), case["exp_index"].cuda()
    stats = torch.zeros(2, 3, device="cuda")
    snap = (eng.disc.clone(), eng.state_m.clone(), eng.state_v.clone())

    def call(**over):
        a = dict(disc=_lib.ptr(eng.disc), m=_lib.ptr(eng.state_m), v=_lib.ptr(eng.state_v), step0=1, net=C.byref(eng._net), act_dim=6,
                 obs=_lib.ptr(obs), act=_lib.ptr(act), perm=_lib.ptr(perm), n=33, obs_exp=_lib.ptr(eng.expert_obs),
                 act_exp=_lib.ptr(eng.expert_act), n_exp_rows=9, ei=_lib.ptr(ei), bsz=16, route=0, stats=_lib.ptr(stats))
        a.update(over)
        return lib.ts_gail_disc_steps(
            eng._ws.handle, a["disc"], a["m"], a["v"], _lib.i64(a["step0"]), a["net"], _lib.i64(a["act_dim"]), a["obs"], a["act"],
            a["perm"], _lib.i64(a["n"]), a["obs_exp"], a["act_exp"], _lib.i64(a["n_exp_rows"]), a["ei"], _lib.i64(a["bsz"]),
            C.c_int32(0), _lib.f64(1e-3), _lib.f64(0.9), _lib.f64(0.999), _lib.f64(1e-8), _lib.f64(0), _lib.f64(0.99), _lib.f64(0),
            C.c_int32(0), _lib.f64(0), C.c_int32(a["route"]), a["stats"], C.c_void_p(0), _lib.current_stream(eng.device))

    null = C.c_void_p(0)
    for over in (dict(disc=null), dict(m=null), dict(v=null), dict(net=null), dict(obs=null), dict(act=null), dict(perm=null),
                 dict(obs_exp=null), dict(act_exp=null), dict(ei=null), dict(stats=null), dict(bsz=0), dict(bsz=-1), dict(n=15),
                 dict(n_exp_rows=0), dict(step0=0), dict(act_dim=0), dict(act_dim=23), dict(route=3), dict(route=-1)):
        assert call(**over) == TS_ERR_INVALID_ARG, over
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(snap, (eng.disc, eng.state_m, eng.state_v))) and not stats.any()
    # the loss and reward entry points
    l = torch.zeros(4, device="cuda")
    d, st = torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda")
    s = _lib.current_stream(eng.device)
    assert lib.ts_gail_loss(eng._ws.handle, _lib.ptr(l), _lib.i64(0), _lib.i64(4), _lib.ptr(d), _lib.ptr(st), s) == TS_ERR_INVALID_ARG
    assert lib.ts_gail_loss(eng._ws.handle, _lib.ptr(l), _lib.i64(4), _lib.i64(0), _lib.ptr(d), _lib.ptr(st), s) == TS_ERR_INVALID_ARG
    assert lib.ts_gail_loss(eng._ws.handle, null, _lib.i64(2), _lib.i64(2), _lib.ptr(d), _lib.ptr(st), s) == TS_ERR_INVALID_ARG
    rew = torch.zeros(33, device="cuda")
    assert lib.ts_gail_reward(eng._ws.handle, null, C.byref(eng._net), _lib.i64(6), _lib.ptr(obs), _lib.ptr(act), _lib.i64(33),
                              _lib.ptr(rew), null, C.c_int32(0), s) == TS_ERR_INVALID_ARG
    assert lib.ts_gail_reward(eng._ws.handle, _lib.ptr(eng.disc), C.byref(eng._net), _lib.i64(6), _lib.ptr(obs), _lib.ptr(act),
                              _lib.i64(0), _lib.ptr(rew), null, C.c_int32(0), s) == TS_ERR_INVALID_ARG
    # a layer-norm descriptor is outside the envelope
    ln = _lib.NetDesc.make(23, [64, 64], "tanh", _lib.NetDesc.LAYERNORM)
    assert call(net=C.byref(ln)) == TS_ERR_UNSUPPORTED
    # it still works afterwards
    eng.disc_update(case["obs"], case["act"], case["perm"], case["exp_index"])
    assert eng.optim_step == 2 and not torch.equal(eng.disc, snap[0])
