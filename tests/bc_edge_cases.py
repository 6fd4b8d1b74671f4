"""Inputs and references for the two behaviour-cloning loss kernels on raw arrays (ts_bc_ce_loss, ts_bc_mse_loss in
tianshou_amd/csrc/ts_sac.hip).  Shared by tests/test_bc_edge_inputs_cpu.py and the GPU test tests/test_gpu_bc_edges.py; nothing
here touches the GPU path.

Cross-entropy.  `ce64` is the closed form in float64 (no autograd): nll_b = lse(z_b) - z_b[act_b] with z = logits - max,
loss = mean nll, dlogits = (softmax - onehot) / B.  `ce32` is tests/oracle_bc.py's float32 torch expression on the logits
directly (autograd).  Both and the scales are tests/bcq_edge_cases.py's `loss64` / `loss32` with theta = 0 and no Q term.

MSE.  `mse64`: a = max_action tanh(head), loss = mean (a - a*)^2, dhead = 2 (a - a*) / (B A) max_action (1 - tanh^2) in
float64 on the float32 inputs; `mse32`: F.mse_loss(max_action * torch.tanh(head), a*) in float32 (autograd).

Bars (the rule of tests/bcq_edge_cases.py, nothing tuned against a kernel): exact claims are asserted exactly; the rest is
        |got - ref64| <= 4 * err32 + 4 * eps32 * scale,        err32 = |the float32 torch value - ref64| of that element,
`scale` being the largest magnitude the evaluation passes through, written down from the formulas:
    CE loss      the mean of the rows' nll scales 1 + |lse| + |z_a| + sum_c p_c |z_c|        (bcq_edge_cases, theta = 0)
    dlogits      (amp_a + 1{a = a_b}) / B, amp_a the softmax's conditioning in its arguments  (bcq_edge_cases, theta = 0)
    MSE loss     the mean of max(|a|, |a*|)^2: a square of a difference of two numbers of that size
    dhead        max(|a|, |a*|) max_action / (B A): the same difference times factors of at most max_action and 1 / (B A)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import bcq_edge_cases as BQ
from tests.bcq_edge_cases import EPS32, bar, f32, ld_of  # noqa: F401

SENTINEL = 7.0
GUARD = 64                                  # floats behind every output buffer that no kernel may touch
CE_A_GRID = [1, 2, 31, 32, 33, 64]
CE_B_GRID = [1, 5, 37, 257]                 # 37: no multiple of a workgroup's four rows; 257: more than 64 rows per wave
MSE_A_GRID = [1, 6, 17, 31, 32]
MSE_B_GRID = [1, 5, 37, 1025]               # 1025 x 32 elements: more than one pass of the loss workgroup's 1024 threads
MAX_ACTIONS = [1.0, 2.5]
HEAD_PITCH = 32


# ---- cross-entropy ------------------------------------------------------------------------------------------------------
def ce_case(logits, act) -> dict:
    logits = f32(logits)
    return dict(logits=logits, act=torch.as_tensor(np.asarray(act, np.int64)), B=logits.shape[0], A=logits.shape[1])


def ce_grid_case(a: int, b: int) -> dict:
    g = torch.Generator().manual_seed(11000 + 100 * a + b)
    return ce_case(torch.randn(b, a, generator=g) * 1.5, torch.randint(0, a, (b,), generator=g))


def ce_offset_case(offset: float, a: int = 4, b: int = 6) -> dict:
    """Small-integer logits + a common offset: logits - max is the offset-free integer exactly (80 and 1e4 are integers a
    float32 holds together with the +-3)."""
    g = torch.Generator().manual_seed(43)
    return ce_case(torch.randint(-3, 4, (b, a), generator=g).float() + offset, [k % a for k in range(b)])


def ce_spread_case() -> dict:
    """One action dominates by more than 104 (exp(-104) < the smallest float32 denormal 1.4e-45): the losing actions' exp is
    exactly 0 in float32 (not in float64).  Rows: target on the dominating action (first, last column), on a dominated one."""
    return ce_case([[0.0, -105.0, -120.0, -300.0], [-110.0, -105.5, -200.0, 3.0], [0.0, -105.0, -120.0, -300.0],
                    [-110.0, -105.5, -200.0, 3.0]], [0, 3, 1, 2])


def ce_tie_case(a: int = 4, b: int = 8, level: float = 1000.0) -> dict:
    """Equal logits of a large common value, A and B powers of two: softmax = 1 / A and every division are exact."""
    return ce_case(torch.full((b, a), level), [k % a for k in range(b)])


def ce_partial_tie_case() -> dict:
    """Two equal maxima above a lower rest; the target on one of the tied maxima, on the other and on a lower action."""
    return ce_case([[2.0, 2.0, -1.0], [2.0, 2.0, -1.0], [2.0, 2.0, -1.0], [0.5, -3.0, 0.5]], [0, 1, 2, 2])


def ce_extreme_target_case(a: int = 7, b: int = 6) -> dict:
    """The target on the largest logit of the row (even rows) and on the smallest (odd rows)."""
    g = torch.Generator().manual_seed(47)
    lg = torch.randn(b, a, generator=g) * 3.0
    act = [int(lg[k].argmax()) if k % 2 == 0 else int(lg[k].argmin()) for k in range(b)]
    return ce_case(lg, act)


def all_ce_cases() -> dict:
    cases = {"offset_plus_80": ce_offset_case(80.0), "offset_minus_80": ce_offset_case(-80.0), "offset_1e4": ce_offset_case(1.0e4),
             "spread": ce_spread_case(), "ties": ce_tie_case(), "partial_ties": ce_partial_tie_case(),
             "extreme_targets": ce_extreme_target_case()}
    for a in CE_A_GRID:
        for b in CE_B_GRID:
            cases[f"grid_A{a}_B{b}"] = ce_grid_case(a, b)
    return cases


def _as_bcq(case: dict) -> dict:
    b, a = case["B"], case["A"]
    return BQ.loss_case(torch.zeros(b, a), case["logits"], case["act"], torch.zeros(b), 0.0)


def ce64(case: dict) -> dict:
    r = BQ.loss64(_as_bcq(case))
    return dict(nll=r["nll"], loss=r["i_loss"], loss_scale=r["i_loss_scale"], dlogits=r["dlogits"], dlogits_scale=r["dlogits_scale"],
                p=r["p"])


def ce32(case: dict) -> dict:
    lg = case["logits"].float().clone().requires_grad_(True)
    loss = F.nll_loss(F.log_softmax(lg, dim=-1), case["act"])
    loss.backward()
    return dict(loss=loss.detach(), dlogits=lg.grad)


# ---- MSE on the bounded head ----------------------------------------------------------------------------------------------
def mse_case(head, act_data, max_action: float, seed: int = 0) -> dict:
    """`head`: [B, A] pre-tanh values; the kernel's input is the [B, 32] head block, its padding columns filled with draws the
    kernel must not read into the loss."""
    head, act_data = f32(head), f32(act_data)
    b, a = head.shape
    block = torch.randn(b, HEAD_PITCH, generator=torch.Generator().manual_seed(500 + seed)) * 3.0
    block[:, :a] = head
    return dict(head=head, block=block, act_data=act_data, max_action=float(max_action), B=b, A=a)


def mse_grid_case(a: int, b: int, max_action: float) -> dict:
    g = torch.Generator().manual_seed(13000 + 100 * a + b)
    head = torch.randn(b, a, generator=g) * 1.5
    act = (torch.rand(b, a, generator=g) * 2.0 - 1.0) * max_action
    return mse_case(head, act, max_action, seed=a + b)


def mse_saturated_case(max_action: float) -> dict:
    """head = +-20: tanh is exactly +-1 in float32 (1 - 2 exp(-40) rounds to 1), so 1 - tanh^2 and dhead are exactly 0."""
    head = torch.tensor([[20.0, -20.0, 20.0], [-20.0, 20.0, -20.0]])
    return mse_case(head, torch.tensor([[0.3, -0.2, -1.0], [0.9, 0.1, 0.5]]) * max_action, max_action)


def mse_zero_head_case(max_action: float) -> dict:
    """head = 0: a = 0 and 1 - tanh^2 = 1 exactly, so dhead = -2 a* max_action / (B A) up to its own roundings."""
    return mse_case(torch.zeros(3, 4), torch.tensor([[0.5, -0.25, 1.0, 0.0]] * 3) * max_action, max_action)


def mse_on_target_case(max_action: float) -> dict:
    """a* = a: head 0 gives a = 0, head +-20 gives a = +-max_action (one float32 product of max_action and +-1): the loss and
    dhead are exactly 0 although 1 - tanh^2 = 1 in the head = 0 columns."""
    head = torch.tensor([[0.0, 20.0, -20.0, 0.0], [-20.0, 0.0, 0.0, 20.0]])
    return mse_case(head, torch.sign(head) * np.float32(max_action), max_action)


def all_mse_cases() -> dict:
    cases = {}
    for m in MAX_ACTIONS:
        cases[f"saturated_M{m}"] = mse_saturated_case(m)
        cases[f"zero_head_M{m}"] = mse_zero_head_case(m)
        cases[f"on_target_M{m}"] = mse_on_target_case(m)
        for a in MSE_A_GRID:
            for b in MSE_B_GRID:
                cases[f"grid_A{a}_B{b}_M{m}"] = mse_grid_case(a, b, m)
    return cases


def mse64(case: dict) -> dict:
    h, tgt, m = case["head"].double(), case["act_data"].double(), case["max_action"]
    n = case["B"] * case["A"]
    t = torch.tanh(h)
    a = m * t
    big = torch.maximum(a.abs(), tgt.abs())
    return dict(loss=((a - tgt) ** 2).mean(), loss_scale=(big * big).mean(), dhead=2.0 * (a - tgt) / n * m * (1.0 - t * t),
                dhead_scale=big * m / n)


def mse32(case: dict) -> dict:
    h = case["head"].float().clone().requires_grad_(True)
    loss = F.mse_loss(case["max_action"] * torch.tanh(h), case["act_data"])
    loss.backward()
    return dict(loss=loss.detach(), dhead=h.grad)


# ---- references and bars --------------------------------------------------------------------------------------------------
def reference(kind: str, case: dict) -> dict:
    """float64 values, per-element err32 of the float32 torch formula and the bars; kind "ce" | "mse"."""
    out, got32 = (ce64(case), ce32(case)) if kind == "ce" else (mse64(case), mse32(case))
    for k in quantities(kind):
        out[k + "_32"] = got32[k]
        out[k + "_err32"] = (got32[k].double() - out[k]).abs()
        out[k + "_bar"] = bar(out[k + "_err32"], out[k + "_scale"])
    return out


def quantities(kind: str) -> tuple:
    return ("loss", "dlogits") if kind == "ce" else ("loss", "dhead")


def err32_units(kind: str, ref: dict) -> dict:
    """Largest err32 / (eps32 * scale) per quantity (elements of scale 0 must have err32 0).  An element whose float64 value lies
    below the smallest float32 denormal 2^-149 and whose float32 value is 0 counts as exact: no float32 number is nearer (the
    dominated actions of `ce_spread_case`, whose scale -- a relative one -- underflows with them)."""
    units = {}
    for k in quantities(kind):
        err, scale = ref[k + "_err32"], torch.as_tensor(ref[k + "_scale"], dtype=torch.float64)
        err = torch.where((ref[k].abs() < 2.0 ** -149) & (ref[k + "_32"].double() == 0), torch.zeros_like(err), err)
        assert not bool(((scale == 0) & (err > 0)).any()), k
        units[k] = float(torch.where(scale > 0, err / (EPS32 * scale.clamp_min(1e-300)), torch.zeros_like(err)).max())
    return units
