"""CPU checks of tests/drqn_edge_cases.py: every case tests/test_gpu_drqn_edges.py runs has the property that test relies on.
(a) the float32 oracle sits within a quarter of every parity bar (`pytest -s` prints the ratios quoted in drqn_edge_cases.py);
(b) the saturated gates are exactly saturated in float32; (c) tie rows are bit-identical and the oracle takes the lowest index;
(d) the Huber cases' t = ret - q are exactly the intended values.  The references themselves are pinned to
oracle_drqn.update_with_batch, which tests/test_oracle_golden.py pins to the unmodified reference."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from oracle import oracle_drqn as ORQ
from tests import drqn_edge_cases as E


def _names(cases):
    return [c["name"] for c in cases]


def test_the_grid_covers_what_it_must():
    g = E.GRID_CASES
    assert {c["obs_dim"] for c in g} == {4, 32, 33} and {c["A"] for c in g} == {1, 2, 5, 32}
    shapes = {(c["H"], c["L"], c["B"], c["T"]) for c in g}
    want = ({(32, 3, b, 64) for b in (1, 16, 17)} | {(32, 1, 1, 256)} | {(64, 1, b, 64) for b in (1, 15, 17)}
            | {(128, 2, b, 64) for b in (1, 16, 17)} | {(128, 2, 17, 2), (96, 2, 17, 17)})
    assert want <= shapes
    for c in g:
        assert c["paths"] == (("per_step",) if c["H"] == 96 else E.PATHS), c["name"]
        if c["H"] == 64:
            assert c["obs_dim"] == 32                                   # no fc1 padding rows
    assert all(n in E.CASES and E.CASES[n]["T"] == 64 and 0 < t1 < 64 for n, t1 in E.CARRIED)
    carried = {(E.CASES[n]["H"], E.CASES[n]["B"], t1) for n, t1 in E.CARRIED}
    assert carried == {(h, b, t) for h in (32, 128) for b in (1, 17) for t in (1, 32, 63)}
    assert all(E.CASES[n]["B"] == 1 and E.CASES[n]["T"] == 64 for n in E.CARRIED_STEPS)


@pytest.mark.parametrize("name", _names(E.PARITY_CASES))
def test_float32_oracle_is_within_a_quarter_of_every_bar(name):
    """Condition (a), for exactly the list the GPU file parametrises over."""
    case = E.CASES[name]
    r32, r64 = E.reference32(case), E.reference64(case)
    for k, v in E.outputs_of(r32).items():
        assert torch.isfinite(v).all(), k
    r = E.ratios(r32, r64, case["zero"])
    print(f"  {name:36s} " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(r.items())))
    assert max(r.values()) <= E.QUARTER, r


@pytest.mark.parametrize("name", ["grid H32 L3 B17 T64", "grid H64 L1 B15 T64", "o -110 H32 L3 B1 T16"])
def test_reference32_is_the_pinned_oracle(name):
    """reference32 (oracle_drqn.forward + the loss expressions) against oracle_drqn.update_with_batch, bit for bit: MSE with
    weights, Huber with delta 2.5, B = 1."""
    case, i = E.CASES[name], E.inputs(E.CASES[name])
    ocfg = OD.DQNConfig(huber_delta=case["huber"])
    col: dict = {}
    loss, td = ORQ.update_with_batch(OD.DQNState.create(i["p"], ocfg), ocfg, i["obs"], i["act"], i["ret"], i["weight"], collect=col)
    r32 = E.reference32(case)
    assert float(r32["loss"]) == loss and torch.equal(td, r32["td"]) and torch.equal(col["q_all"], r32["q"])
    for k in ORQ.param_keys(case["L"]):
        assert torch.equal(col["grads"][k], r32["grads"][k]), k


def test_saturation_is_exact_in_float32():
    """Condition (b)."""
    s, t = torch.sigmoid, torch.tanh
    assert float(s(torch.tensor(-110.0))) == 0.0 and float(s(torch.tensor(110.0))) == 1.0
    assert float(t(torch.tensor(60.0))) == 1.0 and float(t(torch.tensor(-60.0))) == -1.0
    assert float(s(torch.tensor(-100.0))) == 0.0 and float(s(torch.tensor(100.0))) == 1.0 and float(t(torch.tensor(50.0))) == 1.0
    for case in E.ZERO_CASES:
        gate = 0 if case["name"].startswith("i") else 3
        m = E.gate_margin(case, gate)
        print(f"  {case['name']}: margin {m:.1f}")
        assert m > 100.0, case["name"]
        r32, L = E.reference32(case), case["L"]
        assert not r32["h"].any(), case["name"]
        if gate == 0:
            assert not r32["c"].any()
        assert torch.equal(r32["q"], E.inputs(case)["p"]["fc2.bias"].expand(case["B"], -1))
        for k in ORQ.param_keys(L)[:-1]:
            assert not r32["grads"][k].any(), (case["name"], k)
        assert r32["grads"]["fc2.bias"].any()
    case = E.CASES["o +110 g +-60 H64 L2 B17 T16"]
    assert E.gate_margin(case, 3) > 100.0 and E.gate_margin(case, 2) > 50.0
    off = case["gate_bias"][2]
    assert bool((off == 60.0).any()) and bool((off == -60.0).any())


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("A,tied", E.TIES)
def test_tie_rows(A, tied, negative):
    """Condition (c)."""
    rows = E.tie_rows(A, tied, negative)
    assert rows.dtype == torch.float32 and rows.shape == (A,)
    assert bool((rows[list(tied)] == rows[tied[0]]).all()) and float(rows.max()) == float(rows[tied[0]])
    others = [a for a in range(A) if a not in tied]
    assert bool((rows[others] < rows[tied[0]]).all()) and len(set(rows[others].tolist())) == len(others)
    assert not negative or bool((rows < 0).all())
    assert negative or bool((rows > 0).all())
    obs = torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(3))
    q = ORQ.forward(E.edge_params(rows), obs)
    assert torch.equal(q, rows.expand(5, -1))                                # Q IS the bias row
    assert bool((q.argmax(dim=1) == tied[0]).all()) and bool((q.max(dim=1)[1] == tied[0]).all())
    old = E.lagged_rows(A, tied)
    assert len(set(old.tolist())) == A
    assert A == 1 or int(old.argmax()) != tied[0]
    assert torch.equal(ORQ.forward(E.edge_params(old, seed=2), obs), old.expand(5, -1))


@pytest.mark.parametrize("delta", E.HUBER_DELTAS)
def test_huber_cases_hit_delta_exactly(delta):
    """Condition (d)."""
    c = E.huber_case(delta)
    d = np.float32(delta)
    want = [0.0, 0.0]
    for s in (np.float32(1.0), np.float32(-1.0)):
        want += [s * d, np.nextafter(s * d, np.float32(0.0)), np.nextafter(s * d, s * np.float32(np.inf))]
    want = np.asarray(want, dtype=np.float32)
    assert len(set(want.tolist())) == 7 and float(np.abs(want[3])) < delta < float(np.abs(want[4]))
    q = ORQ.forward(c["p"], c["obs"])
    assert torch.equal(q, c["rows"].expand(c["B"], -1))
    t = c["ret"] - q[torch.arange(c["B"]), c["act"]]                          # float32, as the kernel and the oracle subtract
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), want)
    assert torch.equal(c["t"], t) and 2 not in c["act"].tolist() and {0, 1} == set(c["act"].tolist())
    r32 = E.reference(c["p"], c["obs"], c["act"], c["ret"], None, delta, torch.float32)
    r64 = E.reference(c["p"], c["obs"], c["act"], c["ret"], None, delta, torch.float64)
    assert torch.equal(r32["td"], t) and torch.equal(r64["td"], t.double())
    r = E.ratios(r32, r64)
    assert max(r.values()) <= E.QUARTER, r
    for k in ORQ.param_keys(1)[:-2]:
        assert not r32["grads"][k].any(), k
    assert not r32["grads"]["fc2.bias"][2].any() and not r32["grads"]["fc2.weight"][2].any()


@pytest.mark.parametrize("B", E.BATCH_SIZES)
def test_batch_cases_are_well_conditioned(B):
    for huber in (None, 1.0):
        c = E.batch_case(B, huber)
        a = (c["p"], c["obs"], c["act"], c["ret"], c["weight"], huber)
        r32, r64 = E.reference(*a, torch.float32), E.reference(*a, torch.float64)
        assert torch.equal(r32["q"], c["rows"].expand(B, -1))
        sel = {k: v for k, v in E.ratios(r32, r64).items() if k in ("q", "td", "loss")}
        assert max(sel.values()) <= E.QUARTER, sel
