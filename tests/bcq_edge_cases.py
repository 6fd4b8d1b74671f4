"""Inputs and references for the per-sample DiscreteBCQ kernels on raw arrays (ts_bcq_head, ts_bcq_target, ts_bcq_loss in
tianshou_amd/csrc/ts_bcq.hip).  Shared by tests/test_bcq_edge_inputs_cpu.py and the GPU test tests/test_gpu_bcq_edges.py;
nothing here touches the GPU path.

Masked argmax.  The reference's rule (imitation/discrete_bcq.py:116-118) is a float32 rule: ratio = logits - max logits and
`ratio < log tau` are float32 operations on float32(log tau), and a masked action's value is q - FLT_MAX in float32.
`masked_argmax32` states it with numpy float32 scalars operations (IEEE: the same bits on every machine); the hand-made cases
carry the expected action as a literal beside it.

Loss.  `loss64` is the closed form of discrete_bcq.py:244-252 and of its head gradients in float64 (no autograd); `loss32` is
tests/oracle_bcq.py's float32 torch expression applied to q / logits directly (autograd).

Bars (the rule of tests/dcql_edge_cases.py, nothing tuned against a kernel): exact claims are asserted exactly; the rest is
        |got - ref64| <= 4 * err32 + 4 * eps32 * scale,        err32 = |loss32's value - ref64| of that element,
`scale` being the largest magnitude the evaluation passes through, written down from the formulas:
    delta      max(|Q[b, a_b]|, |returns[b]|)                       a difference of two numbers of that size
    huber      huber + min(|delta|, 1) * delta's scale              d huber / d delta = clamp(delta, -1, 1)
    nll        1 + |lse| + |z_a| + sum_c p_c |z_c|,  z = logits - max: nll = lse - z_a; float32 holds every z_c to eps32 |z_c|
               and d lse / d z_c = p_c; the sum and the logarithm round at the size of 1 + |lse|
    sumsq      sum_a logits^2                                       (positive terms)
    q_loss / i_loss / reg_loss    the mean of their rows' scales;  loss: (q + i) + theta * reg of the three scales
    dq         (1{|delta| < 1} * delta's scale + |clamp(delta)|) / B
    dlogits    (amp_a + 1{a = a_b}) / B + 2 theta |logits| / (B A),  amp_a = p_a (1 + (1 - p_a) |z_a| + sum_{c != a} p_c |z_c|):
               the conditioning of the softmax in its arguments (tests/dcql_edge_cases.py derives it), which no order avoids
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)
FLT_MAX = np.float32(np.finfo(np.float32).max)
SENTINEL = 7.0
A_GRID = [1, 2, 31, 32, 33, 64]
B_GRID = [1, 5, 37]                     # 37: no multiple of a workgroup's four samples


def f32(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def log_tau32(threshold: float) -> float:
    return float(np.float32(np.log(threshold))) if threshold > 0 else -np.inf


def nextafter32(x: float, toward: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(toward)))


def bar(err32, scale):
    return 4.0 * torch.as_tensor(err32, dtype=torch.float64) + 4.0 * EPS32 * torch.as_tensor(scale, dtype=torch.float64)


def ld_of(a: int) -> int:
    return (a + 31) // 32 * 32


# ---- masked argmax ------------------------------------------------------------------------------------------------------
def masked_argmax32(q, logits, log_tau: float) -> np.ndarray:
    q, lg = np.asarray(q, np.float32), np.asarray(logits, np.float32)
    ratio = lg - lg.max(axis=1, keepdims=True)                               # float32 - float32
    mask = (ratio < np.float32(log_tau)).astype(np.float32)
    with np.errstate(over="ignore"):
        return (q - FLT_MAX * mask).argmax(axis=1).astype(np.int64)          # numpy's argmax: the first maximum, as torch's


LT = log_tau32(0.3)
# name -> (q, logits, log_tau, expected action per row)
ARGMAX_CASES = {
    "ratio_equal_to_log_tau_is_not_masked": ([[0.0, 1.0]], [[0.0, LT]], LT, [1]),
    "one_ulp_below_is_masked": ([[0.0, 1.0]], [[0.0, nextafter32(LT, -np.inf)]], LT, [0]),
    "one_ulp_above_is_not_masked": ([[0.0, 1.0]], [[0.0, nextafter32(LT, 0.0)]], LT, [1]),
    "equality_under_a_common_offset": ([[0.0, 1.0]], [[4.0, float(np.float32(4.0) + np.float32(LT))]], LT,
                                       [1 if np.float32(np.float32(4.0) + np.float32(LT)) - np.float32(4.0) >= np.float32(LT) else 0]),
    "threshold_zero_masks_nothing": ([[0.0, 1.0]], [[0.0, -200.0]], -np.inf, [1]),
    "best_q_is_masked": ([[1.0, 5.0, 3.0, 2.0]], [[0.0, -5.0, -0.1, -0.2]], LT, [2]),
    "all_but_one_masked": ([[4.0, 3.0, -7.0, 5.0]], [[-9.0, -9.0, 0.0, -9.0]], LT, [2]),
    "tie_among_allowed_picks_the_first": ([[1.0, 2.0, 2.0, 2.0]], [[0.0, -5.0, 0.0, 0.0]], LT, [2]),
    "tie_of_everything_picks_action_zero": ([[2.0, 2.0, 2.0]], [[0.0, 0.0, 0.0]], LT, [0]),
    "masked_3e38_loses": ([[0.0, 3e38, -1.0]], [[0.0, -5.0, 0.0]], LT, [0]),
    # q - FLT_MAX is -4.03e37 for q = 3e38, not -FLT_MAX: the reference lets it beat an allowed -1e38, and so does the kernel
    "masked_3e38_against_minus_1e38": ([[-1e38, 3e38]], [[0.0, -5.0]], LT, [1]),
}


def grid_pair(a: int, b: int, seed: int = 0):
    """q: normal draws; logits: multiples of 0.25 in [-3, 0] with one 0 per row -- every ratio is exact and at least 0.04 from
    log 0.3 = -1.2040; -> (q, logits, q_old) float32 [b, a]."""
    g = torch.Generator().manual_seed(7000 + 100 * a + b + seed)
    q, q_old = torch.randn(b, a, generator=g), torch.randn(b, a, generator=g)
    lg = -torch.randint(0, 13, (b, a), generator=g).float() * 0.25
    lg[torch.arange(b), torch.randint(0, a, (b,), generator=g)] = 0.0
    return q, lg, q_old


# ---- loss ---------------------------------------------------------------------------------------------------------------
def loss_case(q, logits, act, ret, theta: float) -> dict:
    q, logits = f32(q), f32(logits)
    return dict(q=q, logits=logits, act=torch.as_tensor(np.asarray(act, np.int64)), ret=f32(ret).reshape(-1), theta=float(theta),
                B=q.shape[0], A=q.shape[1])


def grid_loss_case(a: int, b: int, theta: float = 0.01) -> dict:
    g = torch.Generator().manual_seed(9000 + 100 * a + b)
    q = torch.randn(b, a, generator=g) * 2.0
    lg = torch.randn(b, a, generator=g) * 1.5
    act = torch.randint(0, a, (b,), generator=g)
    ret = torch.randn(b, generator=g) * 2.0                                    # |delta| on both sides of 1
    return loss_case(q, lg, act, ret, theta)


ONE_UP, ONE_DOWN = nextafter32(1.0, 2.0), nextafter32(1.0, 0.0)
DELTAS = [0.0, 1.0, -1.0, ONE_UP, -ONE_UP, ONE_DOWN, -ONE_DOWN, 1e6, -1e6]


def delta_case(a: int = 5, theta: float = 0.01) -> dict:
    """Row k: returns = 0 and Q[k, act_k] = DELTAS[k], so delta is that float32 exactly; act alternates between the first and the
    last action."""
    b = len(DELTAS)
    g = torch.Generator().manual_seed(41)
    q = torch.randn(b, a, generator=g)
    act = torch.tensor([0 if k % 2 == 0 else a - 1 for k in range(b)])
    q[torch.arange(b), act] = f32(DELTAS)
    return loss_case(q, torch.randn(b, a, generator=g), act, torch.zeros(b), theta)


def offset_case(offset: float, a: int = 4, b: int = 6, theta: float = 0.01) -> dict:
    """Small-integer logits + a common offset of magnitude 1e4: logits - max is the offset-free integer exactly."""
    g = torch.Generator().manual_seed(43)
    lg = torch.randint(-3, 4, (b, a), generator=g).float() + offset
    act = torch.tensor([k % a for k in range(b)])
    return loss_case(torch.randn(b, a, generator=g), lg, act, torch.randn(b, generator=g), theta)


def dominated_case(theta: float = 0.01) -> dict:
    """[0, -200]: exp(-200) underflows to 0 in float32 (not in float64: 1.4e-87); act = the dominating and the dominated action."""
    return loss_case([[0.5, -0.5], [0.25, 2.0]], [[0.0, -200.0], [0.0, -200.0]], [0, 1], [0.0, 0.5], theta)


def uniform_case(theta: float, a: int = 4, b: int = 8, level: float = 1000.0) -> dict:
    """Equal logits of a large common value, A and B powers of two: softmax = 1 / A and every division are exact, so the head
    gradient without the regulariser is known to the bit; a regulariser that leaked in would move it by 2 theta 1000 / (B A)."""
    g = torch.Generator().manual_seed(47)
    act = torch.tensor([k % a for k in range(b)])
    return loss_case(torch.randn(b, a, generator=g), torch.full((b, a), level), act, torch.zeros(b), theta)


def loss64(case: dict) -> dict:
    """float64 closed forms and the scales of the module docstring."""
    q, lg, act, ret = case["q"].double(), case["logits"].double(), case["act"], case["ret"].double()
    b, a, th = case["B"], case["A"], case["theta"]
    rows = torch.arange(b)
    qa = q[rows, act]
    delta = qa - ret
    ad = delta.abs()
    huber = torch.where(ad < 1.0, 0.5 * delta * delta, ad - 0.5)
    clamp = delta.clamp(-1.0, 1.0)
    z = lg - lg.max(1, keepdim=True).values
    e = torch.exp(z)
    se = e.sum(1, keepdim=True)
    lse = torch.log(se).squeeze(1)
    p = e / se
    nll = lse - z[rows, act]
    sumsq = (lg * lg).sum(1)
    onehot = F.one_hot(act, a).double()
    out = dict(delta=delta, huber=huber, nll=nll, sumsq=sumsq)
    out["delta_scale"] = torch.maximum(qa.abs(), ret.abs())
    out["huber_scale"] = huber + ad.clamp(max=1.0) * out["delta_scale"]
    pz = (p * z.abs()).sum(1)
    out["nll_scale"] = 1.0 + lse.abs() + z[rows, act].abs() + pz
    out["sumsq_scale"] = sumsq
    out["q_loss"], out["i_loss"], out["reg_loss"] = huber.mean(), nll.mean(), sumsq.sum() / (b * a)
    out["q_loss_scale"], out["i_loss_scale"], out["reg_loss_scale"] = out["huber_scale"].mean(), out["nll_scale"].mean(), out["reg_loss"]
    out["loss"] = out["q_loss"] + out["i_loss"] + th * out["reg_loss"]
    out["loss_scale"] = out["q_loss_scale"] + out["i_loss_scale"] + th * out["reg_loss_scale"]
    out["dq"] = onehot * (clamp / b)[:, None]
    out["dq_scale"] = onehot * (((ad < 1.0).double() * out["delta_scale"] + clamp.abs()) / b)[:, None]
    out["dlogits"] = (p - onehot) / b + 2.0 * th * lg / (b * a)
    amp = p * (1.0 + (1.0 - p) * z.abs() + (pz[:, None] - p * z.abs()))
    out["dlogits_scale"] = (amp + onehot) / b + 2.0 * th * lg.abs() / (b * a)
    out["p"] = p
    return out


def loss32(case: dict) -> dict:
    """tests/oracle_bcq.py's float32 expressions on q / logits directly (autograd)."""
    q = case["q"].float().clone().requires_grad_(True)
    lg = case["logits"].float().clone().requires_grad_(True)
    act, ret, b = case["act"], case["ret"].float(), case["B"]
    cur = q[torch.arange(b), act]
    q_loss = F.smooth_l1_loss(cur, ret)
    i_loss = F.nll_loss(F.log_softmax(lg, dim=-1), act)
    reg_loss = lg.pow(2).mean()
    loss = q_loss + i_loss + case["theta"] * reg_loss
    loss.backward()
    return dict(delta=(cur - ret).detach(), huber=F.smooth_l1_loss(cur, ret, reduction="none").detach(),
                nll=F.nll_loss(F.log_softmax(lg, dim=-1), act, reduction="none").detach(), sumsq=lg.detach().pow(2).sum(1),
                q_loss=q_loss.detach(), i_loss=i_loss.detach(), reg_loss=reg_loss.detach(), loss=loss.detach(), dq=q.grad, dlogits=lg.grad)


QUANTITIES = ("delta", "huber", "nll", "sumsq", "q_loss", "i_loss", "reg_loss", "loss", "dq", "dlogits")


def reference(case: dict) -> dict:
    """float64 values, per-element err32 of the float32 oracle formula and the bars."""
    out = loss64(case)
    got32 = loss32(case)
    for k in QUANTITIES:
        out[k + "_32"] = got32[k]
        out[k + "_err32"] = (got32[k].double() - out[k]).abs()
        out[k + "_bar"] = bar(out[k + "_err32"], out[k + "_scale"])
    return out


def err32_units(ref: dict) -> dict:
    """Largest err32 / (eps32 * scale) per quantity (elements of scale 0 must have err32 0)."""
    units = {}
    for k in QUANTITIES:
        err, scale = ref[k + "_err32"], torch.as_tensor(ref[k + "_scale"], dtype=torch.float64)
        assert not bool(((scale == 0) & (err > 0)).any()), k
        units[k] = float(torch.where(scale > 0, err / (EPS32 * scale.clamp_min(1e-300)), torch.zeros_like(err)).max())
    return units


def all_loss_cases() -> dict:
    cases = {"deltas": delta_case(), "offset_plus": offset_case(1.0e4), "offset_minus": offset_case(-1.0e4),
             "dominated": dominated_case(), "uniform_theta0": uniform_case(0.0), "uniform_theta": uniform_case(0.5),
             "theta0_grid": grid_loss_case(5, 5, theta=0.0), "one_action_theta0": grid_loss_case(1, 5, theta=0.0)}
    for a in A_GRID:
        for b in B_GRID:
            cases[f"grid_A{a}_B{b}"] = grid_loss_case(a, b)
    return cases
