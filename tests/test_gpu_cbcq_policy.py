"""GPU: ts_cbcq_policy_forward (BCQPolicy.forward for N observations at once) against tests/oracle_cbcq.policy_forward on the
cases of tests/cbcq_edge_cases.py, whose seed leaves no observation with a top-two gap under 1e-4 (checked on the CPU by
tests/test_cbcq_edge_inputs_cpu.py): every index is compared."""
import numpy as np
import pytest
import torch

from tests import cbcq_common as BC
from tests import cbcq_edge_cases as EC

pytestmark = pytest.mark.gpu


def run(c):
    eng = BC.engine_from(*c["params"], c["cfg"])
    act, idx, q, cand = eng.policy_forward(c["obs"], c["noise"], return_all=True)
    plain = eng.policy_forward(c["obs"], c["noise"])
    assert torch.equal(plain, act)
    return act.cpu().numpy(), idx.cpu().numpy(), q.cpu().numpy(), cand.cpu().numpy()


@pytest.mark.parametrize("first_row", [False, True])
@pytest.mark.parametrize("N,T", [(1, 1), (1, 100), (5, 1), (5, 100)])
def test_policy_forward_matches_oracle(N, T, first_row):
    """The returned action IS candidate idx of the engine's own candidates, bit for bit; idx equals the float64 oracle's argmax
    for every observation (all gaps exceed 1e-4 of the larger value); the candidates and the chosen value at float32 accuracy
    (rtol 1e-5 / atol 2e-5, the target's bar)."""
    c = EC.policy_case(N, T, first_row)
    ref = EC.policy_reference(c)
    act, idx, q, cand = run(c)
    assert cand.shape == (N, T, EC.POLICY_DIMS["act_dim"]) and idx.dtype == np.int64
    assert np.array_equal(act, cand[np.arange(N), idx])
    keep = EC.top_two_gap(ref["q"]) > EC.POLICY_GAP
    assert keep.all()
    assert np.array_equal(idx[keep], ref["idx"][keep])
    np.testing.assert_allclose(cand, ref["cand"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(q, ref["q"].max(1), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(act, ref["act"], rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("first_row", [False, True])
def test_tie_goes_to_the_lower_index(first_row):
    """Two identical draws at the top of every observation: identical candidates, and the lower index is returned."""
    c = EC.policy_case(5, 100, first_row, tie=True)
    act, idx, q, cand = run(c)
    w = c["want_idx"]
    assert np.array_equal(cand[np.arange(5), w], cand[np.arange(5), w + 1])
    assert np.array_equal(idx, w)
    assert np.array_equal(act, cand[np.arange(5), w])
