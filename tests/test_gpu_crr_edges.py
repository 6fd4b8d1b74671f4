"""crr_target_kernel, crr_terms_kernel, crr_mean_kernel and crr_grad_kernel of ts_crr.hip on raw arrays (ts_crr_target,
ts_crr_loss), where tests/test_gpu_crr.py never goes: exp(adv / beta) exactly at the bound and one ulp above it, adv == 0 in
"binary" mode, an overflowing exp (NaN positions as torch's), ties, logits of +-80, done in {0, 1, 2}, actions out of range,
min_q_weight = 0, A = 1 .. 64 with and without padding columns, B no multiple of a workgroup's samples and beyond one stride of
the mean kernel.  The reference is torch autograd in float32 on the same device through the reference's own expressions; the
bar and the construction of the cases are stated in tests/crr_edge_cases.py, and tests/test_crr_edge_inputs_cpu.py checks the
preconditions without a GPU."""
import numpy as np
import pytest
import torch

from tests import crr_edge_cases as CE
from tests import oracle_crr as OC

pytestmark = pytest.mark.gpu


def run_loss(c):
    from tianshou_amd import crr as CR

    out = CR.loss_terms(c["q"], c["logits"], c["act"], c["target"], c["mode"], c["beta"], c["U"], c["w"], fill=CE.SENTINEL)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_loss(c, out=None):
    """Per-sample terms, the losses and both head gradients against autograd on the device; the padding columns exactly 0.0;
    the sentinel gone from every element."""
    a, b = c["A"], c["B"]
    out = run_loss(c) if out is None else out
    ref = CE.reference(c, device="cuda")
    print(f"  A={a} B={b} mode={c['mode']} U={c['U']}")
    assert tuple(out["dq"].shape) == tuple(out["dlogits"].shape) == (b, CE.ld_of(a))
    assert tuple(out["terms"].shape) == (6, b) and tuple(out["losses"].shape) == (6,)
    qs, ls, ys = (float(c[k].abs().max()) for k in ("q", "logits", "target"))       # the operands' scales of the differences
    floors = {"delta": max(qs, ys), "nll": ls, "cql": qs, "adv": qs, "loss": c["w"] * qs, "cql_loss": qs, "mean_nll": ls}
    for k, name in enumerate(("delta", "half_delta_sq", "nll", "coef", "cql", "adv")):
        CE.close(out["terms"][k], ref["terms"][k], name, floor=floors.get(name, 0.0))
    for k, name in enumerate(("loss", "actor_loss", "critic_loss", "cql_loss", "mean_nll", "mean_coef")):
        CE.close(out["losses"][k], ref["losses"][k], name, floor=floors.get(name, 0.0))
    CE.close(out["dq"][:, :a], ref["dq"], "dq")
    CE.close(out["dlogits"][:, :a], ref["dlogits"], "dlogits")
    for name in ("dq", "dlogits"):
        assert not out[name][:, a:].any(), name                                       # padding columns: exact zeros
    for v in out.values():
        assert not (v == CE.SENTINEL).any()
    return out, ref


@pytest.mark.parametrize("mode", OC.MODES)
@pytest.mark.parametrize("a", CE.A_GRID)
@pytest.mark.parametrize("b", CE.B_GRID)
def test_loss_on_the_shape_grid(a, b, mode):
    check_loss(CE.grid_case(a, b, mode))


@pytest.mark.parametrize("name", list(CE.LOSS_CASES))
def test_edge_cases(name):
    check_loss(CE.LOSS_CASES[name]("cuda"))


def test_clamp_passes_the_gradient_at_equality_and_not_one_ulp_above():
    for adv in (0.0, 0.25):
        c = CE.clamp_at_equality_case("cuda", adv=adv)
        out, _ = check_loss(c)
        assert float(out["terms"][3][0]) == c["U"]                                    # e == U to the bit
    above = CE.clamp_at_equality_case("cuda", ulps_below=1)
    out, _ = check_loss(above)
    assert float(out["terms"][3][0]) == above["U"]                                    # clamped
    cbar = out["losses"][5]
    want = (cbar * torch.tensor([-0.5, 0.5]) / 2).tolist()                            # tied logits, no gradient through the weight
    assert out["dlogits"][0, :2].tolist() == want


def test_binary_zero_advantage_has_no_weight():
    out, _ = check_loss(CE.binary_zero_case())
    assert out["terms"][5].tolist() == [0.0, 0.0, 0.75, -0.25] and out["terms"][3].tolist() == [0.0, 0.0, 1.0, 0.0]


def test_overflow_gives_torchs_nan_positions():
    c = CE.overflow_case()
    out, _ = check_loss(c)
    assert float(out["terms"][3][0]) == c["U"] and torch.isfinite(out["losses"]).all()
    assert torch.isnan(out["dq"][0, :2]).all() and torch.isnan(out["dlogits"][0, :2]).all()
    assert torch.isfinite(out["dq"][1]).all() and torch.isfinite(out["dlogits"][1]).all()


def test_one_action():
    out, _ = check_loss(CE.grid_case(1, 5, "exp"))
    assert not out["terms"][5].any() and not out["dlogits"].any() and out["terms"][3].tolist() == [1.0] * 5


def test_act_out_of_range_is_clamped():
    c = CE.grid_case(3, 5)
    lo, hi = dict(c, act=torch.full((5,), -4)), dict(c, act=torch.full((5,), 99))
    for x, a in ((lo, 0), (hi, 2)):
        got, want = run_loss(x), run_loss(dict(c, act=torch.full((5,), a)))
        assert all(torch.equal(got[k], want[k]) for k in got)


def test_reruns_are_bit_identical():
    c = CE.grid_case(33, 259)
    a, b = run_loss(c), run_loss(c)
    assert all(torch.equal(a[k], b[k], ) or (torch.isnan(a[k]) == torch.isnan(b[k])).all() for k in a)


@pytest.mark.parametrize("a", CE.A_GRID)
@pytest.mark.parametrize("b", CE.B_GRID)
def test_target_on_the_shape_grid(a, b):
    from tianshou_amd import crr as CR

    t = CE.target_case(a, b)
    got = CR.expected_target(t["q_old"], t["l_old"], t["rew"], t["done"], t["gamma"]).cpu()
    CE.close(got, CE.target_reference(t, "cuda"), "target")
    masked = t["done"] > 0                                                            # done = 1 and done = 2 alike: rew alone
    assert torch.equal(got[masked], t["rew"][masked])


def test_target_with_logits_of_80():
    from tianshou_amd import crr as CR

    t = CE.target_pm80_case()
    got = CR.expected_target(t["q_old"], t["l_old"], t["rew"], t["done"], t["gamma"]).cpu()
    CE.close(got, CE.target_reference(t, "cuda"), "target")
    np.testing.assert_allclose(got.numpy(), [1.0, 0.5, 0.75], rtol=1e-6)
