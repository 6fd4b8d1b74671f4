"""Edge inputs of the DiscreteCRR per-sample kernels (ts_crr_target / ts_crr_loss on raw arrays), shared by
tests/test_crr_edge_inputs_cpu.py (the preconditions and the closed forms, without a GPU) and tests/test_gpu_crr_edges.py.

The reference of every case is torch autograd in float32 through tests/oracle_crr.losses_from_heads -- the reference's own
expressions, both [B] x [B, 1] broadcasts included -- on the device the test runs on, so that exp / log and the float32
decisions `e <= U` and `adv > 0` are those of one implementation.  Cases whose point is a decision are built from ties and
dyadic values, where every intermediate is exact in float32.

Bar.  The kernels are another float32 evaluation of the same expressions: a dozen operations and one exp / log pair per
element, each good to a few ulp (eps = 6e-8), on values of the tensor's own scale.  1e-5 of the largest finite magnitude of the
reference tensor, the project's bar for these quantities (tests/test_gpu_bcq.py), leaves that a factor of about ten.  For a
quantity that is a difference of two larger ones the scale is that of its operands (`close(..., floor=)`).  NaN positions
must be equal; infinities must be equal with sign.
"""
import numpy as np
import torch

from tests import oracle_crr as OC

SENTINEL = 12345.0
RTOL = 1e-5
A_GRID = (1, 2, 31, 32, 33, 64)
B_GRID = (1, 4, 5, 259)


def f32(x):
    return torch.as_tensor(np.asarray(x, np.float32))


def ld_of(a: int) -> int:
    return (a + 31) // 32 * 32


def case(q, logits, act, target, mode="exp", beta=1.0, U=20.0, w=10.0):
    q, logits = f32(q), f32(logits)
    return dict(q=q, logits=logits, act=torch.as_tensor(np.asarray(act, np.int64)), target=f32(target), mode=mode,
                beta=float(beta), U=float(U), w=float(w), A=q.shape[1], B=q.shape[0])


def grid_case(a: int, b: int, mode: str = "exp", w: float = 10.0, seed: int = 0):
    """Random rows: |q|, |logits| of order 1, beta = 0.5 and U = 1.5, so that the clamp decides some rows and not others."""
    rng = np.random.default_rng(1000 * a + b + seed)
    return case(rng.normal(size=(b, a)), 1.5 * rng.normal(size=(b, a)), rng.integers(0, a, size=b), rng.normal(size=b), mode=mode,
                beta=0.5, U=1.5, w=w)


def e_of(c, device="cpu") -> torch.Tensor:
    """exp(adv / beta) as the float32 oracle forms it on `device` -> [B]."""
    q, lg = c["q"].to(device), c["logits"].to(device)
    *_, adv = OC.losses_from_heads(q, lg, c["act"].to(device), c["target"].to(device), "all", 1.0, 1.0, 0.0)
    return (adv / c["beta"]).exp()


def clamp_at_equality_case(device="cpu", adv: float = 0.25, ulps_below: int = 0):
    """A = 2, beta = 1, tied logits (pi = 1/2 exactly), q = [0.5 + adv, 0.5 - adv] dyadic: adv and V are exact, and U is the
    float32 value exp(adv) takes on `device` (ulps_below = 0: e == U, the gradient passes as in torch.clamp's backward) or the
    float32 number just below it (ulps_below = 1: e is one ulp above U, clamped, no gradient).  A second row with adv = -adv
    stays under the bound either way."""
    c = case([[0.5 + 2 * adv, 0.5], [0.5, 0.5 + 2 * adv]], [[0.0, 0.0], [3.0, 3.0]], [0, 0], [0.25, -0.5], beta=1.0, U=1.0, w=0.5)
    e = e_of(c, device)[0].cpu()
    for _ in range(ulps_below):
        e = torch.nextafter(e, torch.tensor(0.0))
    c["U"] = float(e)
    return c


def binary_zero_case():
    """"binary", A = 4, tied logits (pi = 1/4 exactly) and dyadic Q, so that V and adv are exact: adv == 0 in row 0 (every Q
    tied) and in row 1 (qa equal to the mean of four different Q): coef = 0 there; adv = 0.75 in row 2 (coef = 1) and -0.25 in
    row 3 (coef = 0)."""
    return case([[1.5, 1.5, 1.5, 1.5], [0.5, 1.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]], np.zeros((4, 4)) - 2.0,
                [1, 0, 0, 2], [0.0, 1.0, 2.0, -1.0], mode="binary", w=1.0)


def overflow_case():
    """exp(adv / beta) = inf in row 0 under a finite bound: the loss uses the clamped value, the gradient of that row is
    0 * inf = NaN in torch's autograd and here; row 1 is ordinary."""
    return case([[400.0, 0.0], [0.25, 0.5]], [[0.0, 0.0], [0.5, -0.5]], [0, 1], [1.0, 0.0], beta=1.0, U=20.0, w=1.0)


def tied_case(mode="exp"):
    """Every logit tied and every Q tied (A = 5): pi and softmax(q) are 1/5, adv = 0, e = 1."""
    return case(np.full((3, 5), 0.75), np.full((3, 5), -1.25), [0, 2, 4], [0.5, 0.75, 1.0], mode=mode, beta=0.5, U=20.0, w=2.0)


def big_logit_case(mode="exp"):
    """Logits of +-80 (exp(160) overflows float32 without the max-subtraction), the taken action at either end."""
    lg = [[80.0, -80.0, 0.0], [-80.0, 80.0, 0.0], [80.0, 80.0, -80.0], [-80.0, -80.0, -80.0]]
    return case([[0.5, -0.5, 0.25]] * 4, lg, [0, 0, 1, 2], [0.0, 0.5, -0.5, 1.0], mode=mode, beta=1.0, U=20.0, w=1.0)


LOSS_CASES = {
    "clamp_equal_adv0": lambda dev="cpu": clamp_at_equality_case(dev, adv=0.0),
    "clamp_equal": lambda dev="cpu": clamp_at_equality_case(dev),
    "clamp_one_ulp_above": lambda dev="cpu": clamp_at_equality_case(dev, ulps_below=1),
    "binary_adv_zero": lambda dev="cpu": binary_zero_case(),
    "exp_overflow": lambda dev="cpu": overflow_case(),
    "tied_exp": lambda dev="cpu": tied_case("exp"),
    "tied_binary": lambda dev="cpu": tied_case("binary"),
    "logits_pm80_exp": lambda dev="cpu": big_logit_case("exp"),
    "logits_pm80_all": lambda dev="cpu": big_logit_case("all"),
    "min_q_weight_zero": lambda dev="cpu": grid_case(6, 5, "exp", w=0.0),
    "one_action_exp": lambda dev="cpu": grid_case(1, 5, "exp"),
    "infinite_bound": lambda dev="cpu": dict(grid_case(3, 7, "exp"), U=float("inf")),
}


def reference(c, device="cpu", dtype=torch.float32, per_sample: bool = False) -> dict:
    """Autograd on `device` -> {dq [B, A], dlogits [B, A], terms [6, B], losses [6]} (the layout of crr.loss_terms)."""
    q = c["q"].to(device, dtype).requires_grad_(True)
    lg = c["logits"].to(device, dtype).requires_grad_(True)
    act, y = c["act"].to(device), c["target"].to(device, dtype)
    loss, al, cl, ql, adv = OC.losses_from_heads(q, lg, act, y, c["mode"], c["beta"], c["U"], c["w"], per_sample=per_sample)
    loss.backward()
    with torch.no_grad():
        a = act.clamp(0, c["A"] - 1)
        qa = q.gather(1, a[:, None]).flatten()
        nll = -torch.distributions.Categorical(logits=lg).log_prob(a)
        if c["mode"] == "exp":
            coef = (adv / c["beta"]).exp().clamp(0, c["U"])
        elif c["mode"] == "binary":
            coef = (adv > 0).to(dtype)
        else:
            coef = torch.ones_like(adv)
        delta = qa - y
        terms = torch.stack([delta, 0.5 * delta * delta, nll, coef, q.logsumexp(1) - qa, adv])
        losses = torch.stack([loss, al, cl, ql, nll.mean(), coef.mean()])
    return {"dq": q.grad.cpu(), "dlogits": lg.grad.cpu(), "terms": terms.cpu(), "losses": losses.detach().cpu()}


def close(got: torch.Tensor, ref: torch.Tensor, what: str, rtol: float = RTOL, floor: float = 0.0) -> None:
    """NaN and inf positions equal (inf with sign); the finite rest within rtol of the reference tensor's largest finite
    magnitude -- or of `floor`, if larger: the scale of the operands of a quantity that is a difference (lse(q) - qa, qa - V,
    qa - y), whose rounding error is an ulp of the operands however small the difference comes out (with one action
    lse(q) - qa is 0 and torch's own result is rounding noise of 1e-8; with q = 400 the reference's B x B mean of the CQL term
    adds and subtracts 400)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN positions", got, ref)
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), (what, "inf positions", got, ref)
    fin = torch.isfinite(ref)
    if fin.any():
        scale = max(float(ref[fin].abs().max()), floor, 1e-30)
        err = float((got[fin] - ref[fin]).abs().max())
        assert err <= rtol * scale, (what, err, scale)


# ---- target: q_old, logits_old, rew, done (uint8 values), gamma
def target_case(a: int, b: int, seed: int = 0):
    rng = np.random.default_rng(77 * a + b + seed)
    return dict(q_old=f32(rng.normal(size=(b, a))), l_old=f32(2.0 * rng.normal(size=(b, a))), rew=f32(rng.normal(size=b)),
                done=torch.as_tensor(rng.integers(0, 3, size=b).astype(np.uint8)), gamma=0.97)


def target_pm80_case():
    lg = [[80.0, -80.0, 0.0], [-80.0, 80.0, 0.0], [80.0, 80.0, -80.0]]
    return dict(q_old=f32([[1.0, 2.0, 4.0]] * 3), l_old=f32(lg), rew=f32([0.5, -0.5, 0.0]),
                done=torch.as_tensor(np.array([0, 0, 0], np.uint8)), gamma=0.5)


def target_reference(t, device="cpu") -> torch.Tensor:
    return OC.expected_target(t["q_old"].to(device), t["l_old"].to(device), t["rew"], t["done"], t["gamma"]).cpu()
