"""CPU: the preconditions of tests/test_gpu_dcql_edges.py, checked without a GPU on the inputs of tests/dcql_edge_cases.py --
the way tests/test_distq_edge_inputs_cpu.py serves tests/test_gpu_distq_edges.py.  For the float32 torch formula alone, against
float64: the logsumexp is finite in every case, tied values are tied exactly and untied ones are far apart, the dominated
row's other exponentials underflow in both precisions, the offset cases' means are exact, and the float32 formula stays within
the bar's own floor (so `4 err32 + 4 ulp` is a bar a correct float32 kernel can meet).  `pytest -s` prints the figures."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from tests import dcql_edge_cases as CE
from tests import distq_edge_cases as E
from tests import oracle_dcql as OC

CASES = CE.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_formula_is_finite_and_within_the_floor(name):
    case = CASES[name]
    ref = CE.reference(case)
    for k in ("prio", "qr_loss", "cql_loss", "loss", "gbias"):
        assert torch.isfinite(torch.as_tensor(ref[k])).all() and torch.isfinite(ref[k + "_32"]).all(), k
    q32 = case["rows"].float().mean(-1)
    assert torch.isfinite(q32.logsumexp(0)) and torch.isfinite(ref["q"].logsumexp(0))
    assert bool((ref["cql_b"] >= 0).all())                                   # logsumexp_a q >= q_act
    units = CE.err32_units(ref)
    print(f"  {name}: err32 / (eps32 * scale) = " + ", ".join(f"{k} {v:.2f}" for k, v in units.items()))
    for k, v in units.items():
        assert v <= 4.0, (k, v)                                              # the float32 oracle needs no more than the floor


def test_one_action_has_no_cql_term():
    for n in CE.N_GRID:
        ref = CE.reference(CE.grid_case(1, n, 5))
        assert float(ref["cql_loss"]) == 0.0 and float(ref["cql_loss_32"]) == 0.0
        assert not ref["gbias_cql"].any() and torch.equal(ref["gbias"], ref["gbias_qr"])


def test_tied_actions_are_tied_exactly_in_float32():
    for case in (CE.tied_case(), CE.tied_case(act=torch.tensor([0, 4, 2, 4, 0, 1]))):
        q32 = case["rows"].float().mean(-1)
        assert bool((q32 == q32[0]).all())
        ref = CE.reference(case)
        a = case["A"]
        assert float((ref["p"] - 1.0 / a).abs().max()) <= 1e-15
        assert float((ref["cql_b"] - np.log(a)).abs().max()) <= 1e-14
        # with act = 0 everywhere the columns of the other actions carry min_q_weight / (N A) in the bias row
        if not case["act"].any():
            want = case["mqw"] / (case["N"] * a)
            assert float((ref["gbias"][1:] - want).abs().max()) <= 1e-14 * want


def test_dominated_row_underflows_in_both_precisions():
    for act_hot in (True, False):
        case = CE.dominated_case(act_hot)
        q64, hot = case["rows"].double().mean(-1), 2
        q32 = case["rows"].float().mean(-1)
        gap = float(q64[hot] - q64[torch.arange(case["A"]) != hot].max())
        assert gap >= 1.0e4 - 8.0
        others = torch.arange(case["A"]) != hot
        assert not torch.exp(q64[others] - q64[hot]).any() and not torch.exp(q32[others] - q32[hot]).any()
        ref = CE.reference(case)
        if act_hot:
            assert float(ref["cql_loss"]) == 0.0 and float(ref["cql_loss_32"]) == 0.0
            assert not ref["gbias_cql"].any()
        else:
            assert bool(((ref["cql_b"] - 1.0e4).abs() <= 8.0).all())


@pytest.mark.parametrize("offset", [1.0e6, -1.0e6])
def test_offset_rows_have_exact_float32_means(offset):
    case, base = CE.offset_case(offset), CE.offset_case(0.0)
    assert torch.equal(case["rows"].double(), base["rows"].double() + offset)           # the inputs are exact in float32
    assert torch.equal(case["ret"].double(), base["ret"].double() + offset)
    n = case["N"]
    for perm in (torch.arange(n), torch.arange(n).flip(0), torch.randperm(n, generator=torch.Generator().manual_seed(1))):
        s = torch.zeros(case["A"])
        for j in perm:                                                               # one after the other, in float32
            s = s + case["rows"][:, j]
        assert torch.equal((s / n).double(), case["rows"].double().mean(-1))
    ref, ref0 = CE.reference(case), CE.reference(base)
    assert abs(float(ref["cql_loss"] - ref0["cql_loss"])) <= 1e-9
    assert float((ref["gbias"] - ref0["gbias"]).abs().max()) <= 1e-9 * float(ref0["gbias"].abs().max())
    assert float((ref["prio"] - ref0["prio"]).abs().max()) <= 1e-9


def test_untied_grid_rows_are_far_apart():
    """The grid's q values differ by much more than float32 can blur, so softmax and logsumexp are well conditioned."""
    for name, case in CASES.items():
        if name.startswith("grid") and case["A"] > 1:
            q = case["rows"].double().mean(-1)
            assert float((q.max() - q.min())) > 64 * E.EPS32 * float(case["rows"].abs().max()), name


def test_float32_formula_is_the_oracle_on_an_edge_network():
    """`loss32` against oracle_dcql.update_with_batch on the edge network itself (conv trunk included): the losses, the
    priorities and the head-bias gradient agree, and nothing flows below the head."""
    case = CE.grid_case(3, 21, 5)
    p = E.edge_params(case["A"], case["N"], case["rows"])
    cfg = OC.DiscreteCQLConfig(n_atoms=case["N"], min_q_weight=case["mqw"])
    st = OD.DQNState.create(p, cfg.dqn())
    col: dict = {}
    (loss, qr_loss, cql_loss), prio = OC.update_with_batch(st, cfg, case["obs"], case["act"], case["ret"], case["A"],
                                                           weight=case["weight"], collect=col)
    prio32, (l32, qr32, cq32), g32 = CE.loss32(case)
    assert torch.equal(col["dist"][0], case["rows"].float()) and bool((col["dist"] == col["dist"][0]).all())
    np.testing.assert_allclose([loss, qr_loss, cql_loss], [float(l32), float(qr32), float(cq32)], rtol=1e-6)
    np.testing.assert_allclose(prio.numpy(), prio32.numpy(), rtol=1e-6)
    np.testing.assert_allclose(col["grads"]["fc2.b"].view(case["A"], case["N"]).numpy(), g32.numpy(), rtol=1e-5, atol=1e-7)
    for k in OD.PARAM_ORDER[:8]:
        assert not col["grads"][k].any(), k
