"""The NPG / TRPO actor step (ts_npg.hip: cg_update_kernel's done flag, candidate(s_all)_kernel, kl_eval / kl_finish_kernel,
trpo_select_kernel; ts_npg_q.h: npg_eval_kernel + its finish kernel) where tests/test_gpu_npg.py never goes: a line search that
backtracks, ends on its last candidate or accepts nothing, max_backtracks 1 .. 32, conjugate gradients leaving the loop after 1 .. 6
iterations, shapes on either side of the one-launch / per-layer boundary, B = 1 and B round the 32-row tile and the 256-thread
block, other trunks -- through NPGEngine.actor_step / NetNPGEngine.actor_step (the C ABI) on every route that takes the shape:
the one-launch kernels (TS_NPG_FVP=1), the per-layer GEMM passes (TS_NPG_FVP=0) and NetNPGEngine.

Every case comes from tests/npg_edge_cases.py, which states the bars (the suite's existing ones, against float64) and the
preconditions each case meets on the CPU (tests/test_npg_edge_inputs_cpu.py iterates the same lists, and shows there that each
assertion below fails for a step that picks the wrong candidate, does not restore, or ignores / misses the CG exit).  Each check
prints its error / bar per quantity (`pytest -s`)."""
import pytest
import torch

from tests import npg_edge_cases as E

pytestmark = pytest.mark.gpu


def _on_routes(cases):
    return [pytest.param(c["name"], route, id=f"{c['name']}-{route}") for c in cases for route in c["routes"]]


def make_engine(case, route, monkeypatch, **cfg_over):
    """-> (engine, flat vector -> [w1, b1, ..., w_mu, b_mu, sigma_param] of the case's own widths, padding mask of the flat vector)."""
    from tianshou_amd import npg as NG
    from tianshou_amd.ppo_wide import net_flat_from_tensors as nf

    net, o, a = E.inputs(case)["net"], case["obs_dim"], case["act_dim"]
    t = E.net_tensors(net)
    cfg = NG.NPGConfig(optim_critic_iters=1, **{**E.cfg_of(case), **cfg_over})
    if route == "net":
        hid = list(case["hidden"])
        tc = [torch.zeros(32, o), torch.zeros(32), torch.zeros(1, 32), torch.zeros(1)]
        eng = NG.NetNPGEngine(o, a, hid, [32], case["activation"], nf(t, o, hid, a), nf(tc, o, [32], None), cfg)
        to_tensors, from_tensors = eng.actor_to_tensors, (lambda tt: nf(tt, o, hid, a))
    else:
        monkeypatch.setenv("TS_NPG_FVP", "1" if route == "one_launch" else "0")
        tc = [torch.zeros(64, o), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1)]
        eng = NG.NPGEngine(o, a, 64, NG.actor_flat_from_torch(t, o, 64, a), NG.critic_flat_from_torch(tc, o, 64), cfg)
        sizes = case["hidden"] if case["embed"] else None
        to_tensors, from_tensors = (lambda f: NG.actor_flat_to_torch(f, o, 64, a, sizes)), (lambda tt: NG.actor_flat_from_torch(tt, o, 64, a))
    padding = from_tensors([torch.ones_like(x) for x in t]) == 0          # (an embedded network's padding units included)
    for got, want in zip(to_tensors(eng.actor), t):                       # layout round trip
        assert torch.equal(got.cpu().reshape(want.shape), want)
    assert int(padding.sum()) == eng.actor.numel() - sum(x.numel() for x in t) and not eng.actor[padding].any()
    return eng, to_tensors, padding


def step(case, eng):
    i = E.inputs(case)
    stats, dbg = eng.actor_step(i["obs"], i["act"], i["adv"], i["logp_old"], want_debug=True)
    torch.cuda.synchronize()
    return tuple(float(v) for v in stats.cpu()), dbg


def run_case(name, route, monkeypatch):
    """One actor step -> every assertion of the module docstring's list."""
    case = E.CASES[name]
    eng, to_tensors, padding = make_engine(case, route, monkeypatch)
    before = eng.actor.clone()
    stats, dbg = step(case, eng)
    r64, r32, cfg = E.reference64(case), E.reference32(case), E.cfg_of(case)
    got = dict(grad=E.ref_order(to_tensors(dbg[0])), search_direction=-E.ref_order(to_tensors(dbg[1])),
               fg=E.ref_order(to_tensors(dbg[2])), new=E.ref_order(to_tensors(eng.actor)), stats=stats)
    q = E.ratios(got, r64, r32, cfg)
    print(f"  {name:36s} {route:10s} pick {r64['pick']:2d} exit {r64['exit_iter']:2d}  " + "  ".join(f"{k} {v:.3f}" for k, v in q.items()))
    # padding: observation rows obs_dim .. k0 - 1, head columns >= act_dim, log-sigma slots >= act_dim, embedded padding units
    assert not eng.actor[padding].any() and not dbg[0][padding].any() and not dbg[1][padding].any()
    for k in ("grad", "fg", "cg", "new"):
        assert k not in q or q[k] < 1.0, (k, q)
    assert q["stats"] <= 1.0, (stats, r64["stats"])
    assert q["pick"] == 0.0, (stats, r64["step0"], r64["pick"])
    if case["algo"] == "npg":
        assert stats[2] == 0.0
    elif r64["pick"] < 0:                                   # nothing accepted: bit-exact restore, step 0, the last candidate's kl
        assert torch.equal(eng.actor, before) and stats[2] == 0.0 and q["restored"] == 0.0
        assert abs(stats[1] - r64["cand_kl"][-1]) <= E.STATS_ATOL + E.STATS_RTOL * abs(r64["cand_kl"][-1])
    else:
        assert stats[2] > 0.0 and not torch.equal(eng.actor, before)


@pytest.mark.parametrize("name,route", _on_routes(E.LINE_SEARCH))
def test_line_search(name, route, monkeypatch):
    run_case(name, route, monkeypatch)


@pytest.mark.parametrize("name,route", _on_routes(E.CG_EXIT))
def test_cg_exit(name, route, monkeypatch):
    """(the conjugate-gradient solution is the assertion that fails if the done flag is ignored or set an iteration late)"""
    run_case(name, route, monkeypatch)


@pytest.mark.parametrize("name,route", _on_routes(E.SHAPES))
def test_shapes(name, route, monkeypatch):
    run_case(name, route, monkeypatch)


@pytest.mark.parametrize("name,route", _on_routes(E.ZERO_ADV))
def test_zero_advantages_leave_the_parameters_alone(name, route, monkeypatch):
    """The gradient is 0, conjugate gradients divide 0 by 0, every candidate is NaN: the reference accepts nothing and restores."""
    case = E.CASES[name]
    eng, _, _ = make_engine(case, route, monkeypatch)
    before = eng.actor.clone()
    stats, dbg = step(case, eng)
    assert torch.equal(eng.actor, before) and stats[2] == 0.0
    assert not dbg[0].any()                                  # the gradient itself is exactly 0


@pytest.mark.parametrize("route", E.ROUTES)
@pytest.mark.parametrize("over", [dict(max_backtracks=0), dict(max_backtracks=33), dict(max_kl=0.0)], ids=str)
def test_argument_bounds(over, route, monkeypatch):
    case = E.CASES["pick 1 of 10"]
    eng, _, _ = make_engine(case, route, monkeypatch, **over)
    before = eng.actor.clone()
    i = E.inputs(case)
    with pytest.raises(Exception):
        eng.actor_step(i["obs"], i["act"], i["adv"], i["logp_old"], want_debug=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.actor, before)
