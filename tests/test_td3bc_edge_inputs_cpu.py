"""CPU, float64: the edge inputs of tests/td3bc_edge_cases.py have the properties tests/test_gpu_td3bc_edges.py relies on, at
every (A, B) that test runs."""
import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from tests import td3bc_edge_cases as E

OBS, HID = 7, 64
SIZES = [(A, B) for A in (1, 6, 32) for B in (1, 257, 1025)]


@pytest.mark.parametrize("A,B", SIZES)
@pytest.mark.parametrize("kind", E.KINDS)
def test_mean_abs_q_keeps_lmbda_well_conditioned(kind, A, B):
    """(a) mean|Q| >= 0.05 in every case (so the GPU test excludes nothing), every input finite, alpha as the case says."""
    case = E.edge_case(kind, OBS, A, B, 4, HID)
    q = E.q64(case)
    assert float(q.abs().mean()) >= 0.05
    for k in ("obs", "act", "ret"):
        assert torch.isfinite(case[k]).all() and case[k].dtype == torch.float32
    assert case["act"].shape == (B, A) and float(case["act"].abs().max()) <= E.MAX_ACTION
    assert case["alpha"] == (0.0 if kind == "alpha0" else E.ALPHA)
    ref = E.reference64(case)
    assert np.isfinite(ref["loss"]) and (ref["lmbda"] > 0.0) == (kind != "alpha0")
    assert all(torch.isfinite(g).all() for g in ref["grads"].values())


@pytest.mark.parametrize("A,B", [s for s in SIZES if s[1] > 1])
@pytest.mark.parametrize("kind", ["mixed", "alpha0"])
def test_mixed_q_has_both_signs_and_a_cancelling_mean(kind, A, B):
    """(b) Q has both signs with |mean Q| <= 0.1 mean|Q|.  B = 1 cannot: one sample has one sign and |mean Q| == mean|Q|; there
    the case is Q = 0.5."""
    q = E.q64(E.edge_case(kind, OBS, A, B, 4, HID))
    assert bool((q > 0).any()) and bool((q < 0).any())
    assert abs(float(q.mean())) <= 0.1 * float(q.abs().mean())


@pytest.mark.parametrize("A", [1, 6, 32])
def test_mixed_single_sample_is_half(A):
    q = E.q64(E.edge_case("mixed", OBS, A, 1, 4, HID))
    assert abs(float(q[0]) - 0.5) < 1e-6


@pytest.mark.parametrize("A,B", SIZES)
def test_negative_q_is_negative_everywhere(A, B):
    """(c) every Q < 0, with a margin no float32 forward pass crosses."""
    q = E.q64(E.edge_case("negative", OBS, A, B, 4, HID))
    assert float(q.max()) <= -0.49


@pytest.mark.parametrize("A,B", SIZES)
@pytest.mark.parametrize("kind", ["saturated", "cloned"])
def test_saturated_columns_saturate_in_float32(kind, A, B):
    """(d) the head of a saturated column is +-12 in every row (zero head weights), where tanh == +-1.0f in float32 and
    1 - tanh^2 == 0.0f; free columns stay inside."""
    case = E.edge_case(kind, OBS, A, B, 4, HID)
    cols = case["cols"]
    assert sorted(np.concatenate([cols["saturated"], cols["free"]]).tolist()) == list(range(A))
    assert not case["actor"]["wa"].any()
    head = case["actor"]["ba"].expand(B, A)
    t = torch.tanh(head)
    assert t.dtype == torch.float32
    for j in cols["saturated"]:
        assert bool((t[:, j].abs() == 1.0).all()) and bool((1.0 - t[:, j] * t[:, j] == 0.0).all()), j
    for j in cols["free"]:
        assert bool((t[:, j].abs() < 1.0).all()), j
    assert len(cols["free"]) > 0 or kind == "saturated"                  # (A = 1, saturated: the only column is +12)
    if A >= 6:
        assert len(cols["saturated"]) > 0 and len(cols["free"]) > 0


@pytest.mark.parametrize("A,B", SIZES)
def test_cloned_actions_are_the_float32_policy_action_bit_for_bit(A, B):
    """(e) a_data == pi(s) in float32, bit for bit -- and pi(s) is 0 or +-max_action, values every float32 evaluation of
    max_action * tanh(0 / +-12) gives, whatever order the trunk is summed in (zero head weights); so the cloning loss and its
    gradient are exactly zero in float32, and the float64 gradient is lmbda times plain TD3's."""
    case = E.edge_case("cloned", OBS, A, B, 4, HID)
    with torch.no_grad():
        pi = OS.det_actor_forward(case["actor"], case["obs"], E.MAX_ACTION)
    assert pi.dtype == torch.float32 and torch.equal(pi, case["act"])
    assert set(np.unique(case["act"].numpy()).tolist()) <= {0.0, E.MAX_ACTION, -E.MAX_ACTION}
    # float64 does not saturate at +-12 (1 - tanh^2 = 1.5e-10 there), so its cloning term is not 0 but 1e-20: nothing at 2e-5
    ref = E.reference64(case)
    assert ref["bc_loss"] < 1e-18
    for k in ("wa", "ba"):                                               # (zero head weights: the trunk's gradient is zero)
        g = ref["grads"][k]
        scale = float(g.abs().max())
        assert scale > 0.0 and float((g - ref["lmbda"] * ref["td3"][k]).abs().max()) <= 1e-9 * scale, k


@pytest.mark.parametrize("A,B", SIZES)
def test_alpha0_reference_is_pure_behaviour_cloning(A, B):
    ref = E.reference64(E.edge_case("alpha0", OBS, A, B, 4, HID))
    assert ref["lmbda"] == 0.0 and ref["loss"] == ref["bc_loss"]
    for k, g in ref["grads"].items():
        assert torch.equal(g, ref["bc"][k]), k
    assert float(ref["bc"]["ba"].abs().max()) > 0.0
