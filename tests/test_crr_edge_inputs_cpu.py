"""CPU: the edge tables of tests/crr_edge_cases.py are what they claim to be, and the closed-form head gradients that
crr_grad_kernel writes (tests/oracle_crr.closed_form_grads) agree with torch autograd through the reference's own expressions
on every one of them, NaN positions included."""
import numpy as np
import pytest
import torch

from tests import crr_edge_cases as CE
from tests import oracle_crr as OC


@pytest.mark.parametrize("name", list(CE.LOSS_CASES))
def test_closed_form_matches_autograd_on_every_edge_case(name):
    c = CE.LOSS_CASES[name]()
    ref = CE.reference(c)
    dq, dl = OC.closed_form_grads(c["q"], c["logits"], c["act"], c["target"], c["mode"], c["beta"], c["U"], c["w"])
    CE.close(dq, ref["dq"], "dq")
    CE.close(dl, ref["dlogits"], "dlogits")
    per = CE.reference(c, per_sample=True)                   # the forms the kernels compute: same losses, same gradients
    for k in ("dq", "dlogits", "losses"):
        CE.close(per[k], ref[k], k)


@pytest.mark.parametrize("a", CE.A_GRID)
@pytest.mark.parametrize("mode", OC.MODES)
def test_closed_form_matches_autograd_on_the_grid(a, mode):
    c = CE.grid_case(a, 5, mode)
    ref = CE.reference(c)
    dq, dl = OC.closed_form_grads(c["q"], c["logits"], c["act"], c["target"], c["mode"], c["beta"], c["U"], c["w"])
    CE.close(dq, ref["dq"], "dq")
    CE.close(dl, ref["dlogits"], "dlogits")
    if mode == "exp" and a > 1:
        e = CE.e_of(CE.grid_case(a, 259, mode))
        assert (e > c["U"]).any() and (e < c["U"]).any()     # the clamp decides some rows and not others


def test_clamp_cases_sit_where_they_say():
    for adv in (0.0, 0.25):
        c = CE.clamp_at_equality_case(adv=adv)
        e = CE.e_of(c)
        assert float(e[0]) == c["U"] and float(e[1]) <= c["U"]
        if adv == 0.0:
            assert c["U"] == 1.0
    c = CE.clamp_at_equality_case()
    ref = CE.reference(c)
    above = CE.clamp_at_equality_case(ulps_below=1)
    e = CE.e_of(above)
    assert float(e[0]) > above["U"] and float(torch.nextafter(torch.tensor(above["U"]), torch.tensor(9.0))) == float(e[0])
    ref_above = CE.reference(above)
    # at equality the gradient passes through the weight into the logits' row 0 (tied logits: the plain term alone is
    # cbar * (1/2 - hot)); one ulp above it does not
    cbar = float(ref_above["losses"][5])
    assert torch.allclose(ref_above["dlogits"][0], cbar * torch.tensor([-0.5, 0.5]) / 2, rtol=1e-6)
    assert not torch.allclose(ref["dlogits"][0], float(ref["losses"][5]) * torch.tensor([-0.5, 0.5]) / 2, rtol=1e-3)


def test_binary_zero_overflow_and_tie_cases():
    c = CE.binary_zero_case()
    ref = CE.reference(c)
    assert ref["terms"][5].tolist() == [0.0, 0.0, 0.75, -0.25] and ref["terms"][3].tolist() == [0.0, 0.0, 1.0, 0.0]
    c = CE.overflow_case()
    ref = CE.reference(c)
    assert torch.isinf(CE.e_of(c)[0]) and ref["terms"][3].tolist()[0] == c["U"]
    assert torch.isnan(ref["dq"][0]).all() and torch.isnan(ref["dlogits"][0]).all()
    assert torch.isfinite(ref["dq"][1]).all() and torch.isfinite(ref["dlogits"][1]).all() and torch.isfinite(ref["losses"]).all()
    for mode in ("exp", "binary"):
        ref = CE.reference(CE.tied_case(mode))
        assert not ref["terms"][5].any()
        assert ref["terms"][3].tolist() == ([1.0] * 3 if mode == "exp" else [0.0] * 3)
    ref = CE.reference(CE.big_logit_case("all"))
    assert torch.isfinite(ref["dlogits"]).all() and ref["terms"][2].tolist()[:2] == [0.0, 160.0]
    ref = CE.reference(CE.grid_case(1, 5, "exp"))
    assert not ref["terms"][5].any() and not ref["dlogits"].any()             # A = 1: pi = 1, adv = 0, no actor gradient


def test_target_cases():
    t = CE.target_case(3, 259)
    done = t["done"].numpy()
    assert set(done.tolist()) == {0, 1, 2}
    ref = CE.target_reference(t)
    assert torch.equal(ref[torch.as_tensor(done > 0)], t["rew"][torch.as_tensor(done > 0)])       # > 0 masks: 1 and 2 alike
    assert not torch.equal(ref, t["rew"])
    ref = CE.target_reference(CE.target_pm80_case())
    np.testing.assert_allclose(ref.numpy(), [0.5 + 0.5 * 1.0, -0.5 + 0.5 * 2.0, 0.5 * 1.5], rtol=1e-6)
