"""CPU checks of tests/npg_edge_cases.py: every case tests/test_gpu_npg_edges.py runs has the property that test relies on --
preconditions (a) to (e) of that module's docstring (`pytest -s` prints the ratios it quotes) -- the lists contain what they must,
reference32 is oracle_npg.minibatch_step bit for bit (which tests/test_oracle_golden.py pins to the unmodified reference), and
every assertion of the GPU file is sensitive: a deliberately wrong step violates its bar against reference64 on a listed case."""
import math

import pytest
import torch

from oracle import oracle_npg as ON
from oracle import oracle_ppo as OP
from tests import npg_edge_cases as E


def _names(cases):
    return [c["name"] for c in cases]


def test_the_lists_cover_what_they_must():
    ls = E.LINE_SEARCH
    assert all(c["algo"] == "trpo" for c in ls)
    picks = {(c["pick"], c["max_backtracks"]) for c in ls}
    assert any(p == 0 for p, _ in picks) and any(0 < p < m - 1 for p, m in picks) and any(p == m - 1 and m > 1 for p, m in picks)
    assert any(p == -1 for p, _ in picks) and {m for _, m in picks} >= {1, 2, 10, 32}
    assert any(c["stale"] for c in ls) and any(c["B"] == 1 for c in ls)
    assert all(abs(c["max_kl"] - 5.0) > 1e-9 for c in ls)                      # candidate 2 sits at 1.008 max_kl there
    assert set(E.LOSS_ONLY) <= set(E.CASES)
    for algo in ("npg", "trpo"):
        exits = [c["exit_iter"] for c in E.CG_EXIT if c["algo"] == algo]
        assert 1 in exits and 0 in exits and any(2 <= j <= 4 for j in exits) and any(5 <= j <= 8 for j in exits)
    sh = E.SHAPES
    dims = {(c["algo"], c["obs_dim"], c["act_dim"]) for c in sh if c["hidden"] == (64, 64)}
    assert dims >= {(a, o, k) for a in ("npg", "trpo") for o, k in ((32, 8), (33, 1), (8, 9), (5, 32))}
    assert {(c["algo"], c["B"]) for c in sh if (c["obs_dim"], c["act_dim"]) == (17, 6)} == \
        {(a, b) for a in ("npg", "trpo") for b in (1, 31, 32, 33, 255, 256, 257)}
    trunks = {(c["hidden"], c["activation"], c["embed"]): c for c in sh}
    for key in (((64, 48, 32), "relu", None), ((96,), "tanh", None), ((48, 32), "tanh", (64, 64))):
        assert trunks[key]["algo"] == "trpo" and trunks[key]["pick"] >= 1
    assert trunks[((64, 48, 32), "relu", None)]["routes"] == ("net",) and trunks[((96,), "tanh", None)]["routes"] == ("net",)
    assert trunks[((48, 32), "tanh", (64, 64))]["routes"] == ("one_launch", "per_layer")
    for c in E.ALL_CASES + E.ZERO_ADV:
        assert c["obs_dim"] <= 33 and c["B"] <= 700 and max(c["hidden"]) <= 96, c["name"]
        if c["hidden"] == (64, 64) and c["activation"] == "tanh":          # every route that supports the shape
            want = ("one_launch",) * (c["obs_dim"] <= 32 and c["act_dim"] <= 8) + ("per_layer", "net")
            assert c["routes"] == want, c["name"]
    assert all(c["zero_adv"] and c["algo"] == "trpo" for c in E.ZERO_ADV) and not any(c["zero_adv"] for c in E.ALL_CASES)


@pytest.mark.parametrize("name", _names(E.ALL_CASES))
def test_preconditions(name):
    """(a), (b), (c), (e) for exactly the lists the GPU file parametrises over, (d) for CG_EXIT; the intended pick / exit."""
    case = E.CASES[name]
    r64, r32 = E.reference64(case), E.reference32(case)
    for k in ("grad", "fg", "search_direction", "new"):
        assert torch.isfinite(r32[k]).all(), k
    q = E.ratios(r32, r64, None, E.cfg_of(case))
    extra = f"  no-break {E.no_break_difference(case):.1e}" if case in E.CG_EXIT and r64["exit_iter"] else ""
    print(f"  {name:36s} pick {r64['pick']:2d} exit {r64['exit_iter']:2d}  " + "  ".join(f"{k} {v:.3f}" for k, v in q.items()) + extra)
    assert E.precondition_failures(case, no_break=case in E.CG_EXIT) == []
    assert case["pick"] is None or r64["pick"] == case["pick"]
    assert case["exit_iter"] is None or r64["exit_iter"] == case["exit_iter"]
    for k in E.LOSS_ONLY.get(name, ()):
        for r in (r64, r32):
            assert k < r["pick"] and r["cand_kl"][k] < case["max_kl"] and r["cand_loss"][k] >= r["stats"][0]
    if case["stale"]:
        assert float((E.inputs(case)["logp_old"] - E.inputs(E.CASES["pick 1 of 10"])["logp_old"]).abs().max()) > 0.1


@pytest.mark.parametrize("name", _names(E.ZERO_ADV))
def test_zero_advantages_restore_in_the_reference(name):
    case = E.CASES[name]
    for r in (E.reference64(case), E.reference32(case)):
        assert not r["grad"].any() and math.isnan(r["step0"]) and all(math.isnan(k) for k in r["cand_kl"])
        assert r["pick"] == -1 and r["stats"][2] == 0.0 and torch.equal(r["new"], r["old"])


@pytest.mark.parametrize("name", ["pick 0 of 10", "pick 1 of 10", "none of 2", "stale logp_old, pick 1 of 10", "B 1, pick 0 of 10",
                                  "npg cg exit 3", "trpo cg exit 5", "npg cg exit never", "npg B 33", "trpo obs 33 act 1",
                                  "npg obs 5 act 32"])
def test_reference32_is_the_pinned_oracle(name):
    """reference32 against oracle_npg.minibatch_step on Net[64, 64] tanh, bit for bit: NPG and TRPO, backtracking, nothing
    accepted, a stale logp_old, B = 1, conjugate gradients leaving early."""
    case, i = E.CASES[name], E.inputs(E.CASES[name])
    t = E.net_tensors(i["net"])
    p = dict(zip(("a_w1", "a_b1", "a_w2", "a_b2", "a_wmu", "a_bmu", "a_sigma"), (x.clone() for x in t)))
    p.update({k: v for k, v in OP.init_params(case["obs_dim"], case["act_dim"], seed=0).items() if k.startswith("c_")})
    cfg = ON.NPGConfig(optim_critic_iters=1, **E.cfg_of(case))
    st, col = OP.PPOState(params=p), {}
    res = ON.minibatch_step(st, cfg, i["obs"], i["act"], i["adv"], torch.zeros(case["B"]), i["logp_old"], collect=col)
    r32 = E.reference32(case)
    assert torch.equal(col["flat_grads"], r32["grad"]) and torch.equal(col["mvp_of_grad"], r32["fg"])
    assert torch.equal(col["search_direction"], r32["search_direction"])
    assert torch.equal(torch.cat([st.params[k].reshape(-1) for k in ON.ACTOR_KEYS]), r32["new"])
    assert res[0] == r32["stats"][0] and res[2] == r32["stats"][1]
    assert case["algo"] == "npg" or res[3] == r32["stats"][2]


def _worst(mutate, cases, keys):
    """The largest error / bar over `keys` that the wrong step `mutate` reaches on `cases` against reference64."""
    worst = 0.0
    for case in cases:
        got = E.reference64(case, mutate)
        q = E.ratios(got, E.reference64(case), E.reference32(case), E.cfg_of(case))
        worst = max([worst] + [q[k] for k in keys if k in q])
    return worst


def test_every_gpu_assertion_is_sensitive():
    """What replaces mutating the kernels: five wrong steps, each against the bars the GPU file applies."""
    unmutated = _worst(None, E.ALL_CASES, ("grad", "fg", "cg", "new", "stats", "pick", "restored"))
    assert unmutated == 0.0
    ls = E.LINE_SEARCH
    for keys in (("pick",), ("stats",), ("new",)):                       # the recovered k, the reported kl / step, the parameters
        assert _worst("always_pick_0", [c for c in ls if c["pick"] > 0], keys) > 1.0, keys
        assert _worst("pick_late", [c for c in ls if c["pick"] >= 0], keys) > 1.0, keys
    for c in ls:                                                         # EVERY case with a pick notices either mistake
        if c["pick"] > 0:
            assert _worst("always_pick_0", [c], ("pick",)) > 1.0, c["name"]
        if c["pick"] >= 0:
            assert _worst("pick_late", [c], ("pick",)) > 1.0, c["name"]
    none = [c for c in ls if c["pick"] < 0]
    assert none and all(_worst("no_restore", [c], ("restored",)) > 1.0 for c in none)
    exiting = [c for c in E.CG_EXIT if c["exit_iter"]]
    for c in exiting:
        assert _worst("ignore_break", [c], ("cg",)) > 1.0, c["name"]
    assert _worst("break_late", exiting, ("cg",)) > 1.0
    late = {c["name"]: round(_worst("break_late", [c], ("cg",)), 2) for c in exiting}
    print("  break one iteration late, cg error / bar:", late)
    assert all(v > 1.0 for v in late.values()), late
