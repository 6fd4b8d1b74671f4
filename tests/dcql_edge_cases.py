"""Inputs that put EXACT quantiles into cql_loss_kernel (tianshou_amd/csrc/ts_distq.hip), and plain float64 references of the
DiscreteCQL head.  Shared by tests/test_dcql_edge_inputs_cpu.py and the GPU test tests/test_gpu_dcql_edges.py; nothing here
touches the GPU path.  Built on tests/distq_edge_cases.py (`E`): the edge networks (zero head weights, head == bias for every
row), the QRDQN references `qr_loss64` / `qr_loss32`, `scatter_rows` and the bar rule are that module's.

On an edge network every sample sees the same quantile rows x[a, j], so q_a = mean_j x[a, j] is one vector; `act`, `returns` and
`weight` carry the per-row variety.  Nothing flows below the head, and the bias-row gradient is the column sum over b of d_head:

    gbias[a, j] = sum_{b: act_b = a} dtheta_b[j]  +  min_q_weight / (B N) * (B p_a - #{b: act_b = a}),   p = softmax(q)

References.  `cql64` is the closed form of imitation/discrete_cql.py:102-106 in float64 (max-subtracted logsumexp, no autograd);
`loss32` is tests/oracle_dcql.py's float32 torch expression applied to the rows directly (autograd);
tests/test_dcql_edge_inputs_cpu.py pins it to `oracle_dcql.update_with_batch` on an edge network.

Bars (the rule of tests/distq_edge_cases.py, nothing tuned against a kernel): exact claims are asserted exactly; the rest is
        |got - ref64| <= 4 * err32 + 4 * eps32 * scale,        err32 = |loss32's value - ref64| of that element,
`scale` being the largest magnitude the accumulation passes through:
    cql_loss   max(|lse|, max_a mean_j |x[a, j]|): cql_b = lse - q_act is a difference of numbers of that size
    loss       qr_loss's scale + min_q_weight * cql_loss's scale
    gbias      the QRDQN term's scale (sum of its rows' scales) + min_q_weight / (B N) * (B amp_a + #{b: act_b = a})
prio and qr_loss are QRDQN's quantities with QRDQN's bars.
`amp_a` is p_a with the conditioning of the softmax, which no summation order can avoid: float32 holds the exponent's argument
q_c - m only to eps32 * t_c, t_c = mean_j |x[c, j]| + |q_c - m| (the mean's own rounding and the subtraction's), and to first
order an error delta_c of the arguments moves p_a by p_a ((1 - p_a) delta_a - sum_{c != a} p_c delta_c), so
        amp_a = p_a (1 + (1 - p_a) t_a + sum_{c != a} p_c t_c).
It is 1 for a dominating action (p_a = 1: nothing competes) and p_a (1 + t) between equals.  Written down from the formula and
the number format before any kernel ran; tests/test_dcql_edge_inputs_cpu.py shows that the float32 torch formula itself stays
below 4 eps32 * scale on every case, i.e. that the floor is of the size of a float32 evaluation's error and not a loophole.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import distq_edge_cases as E

A_GRID = [1, 2, 64]
N_GRID = [2, 63, 64, 65, 256]


def cql_case(a: int, n: int, b: int, rows: torch.Tensor, ret=None, act=None, weight=None, mqw: float = 10.0, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(300 + seed)
    if ret is None:
        ret = torch.randn(b, n, generator=g) * 2.5                          # |d| on both sides of 1
    case = E.qr_case(a, n, b, rows, ret, act=act, weight=weight, seed=seed)
    case["mqw"] = float(mqw)
    return case


def grid_case(a: int, n: int, b: int, mqw: float = 10.0) -> dict:
    g = torch.Generator().manual_seed(1000 * a + 10 * n + b)
    act = torch.randint(0, a, (b,), generator=g)
    weight = (torch.rand(b, generator=g) + 0.25) if b > 1 else None
    return cql_case(a, n, b, E.random_rows(a, n, 11 + a + n), act=act, weight=weight, mqw=mqw, seed=5)


def tied_case(a: int = 5, n: int = 9, b: int = 6, act=None) -> dict:
    """Every action carries the same small-integer row: every q_a is the same float32 under every summation order."""
    row = torch.tensor([float(j % 5) - 2.0 for j in range(n)])
    act = torch.zeros(b, dtype=torch.int64) if act is None else act
    return cql_case(a, n, b, row.repeat(a, 1), act=act, weight=E.f32([1.0, 0.5, 2.0, 0.25, 1.5, 1.0][:b]), seed=1)


def dominated_case(act_hot: bool, a: int = 4, n: int = 8, b: int = 5, hot: int = 2) -> dict:
    """q_hot = 1e4 + the small-integer mean, every other q is a small integer mean: exp(q_a - q_hot) underflows to 0 in float32
    and in float64.  The returns sit near the taken row, so that the QRDQN term stays of order one."""
    rows = E.tie_rows_qr(a, n, ())
    rows[hot] += 1.0e4
    others = [i for i in range(a) if i != hot]
    act = torch.full((b,), hot, dtype=torch.int64) if act_hot else torch.tensor([others[i % len(others)] for i in range(b)])
    g = torch.Generator().manual_seed(17)
    ret = rows[act] + torch.randn(b, n, generator=g) * 1.5
    return cql_case(a, n, b, rows, ret=ret, act=act, weight=E.f32([1.0, 0.5, 2.0, 0.25, 1.5][:b]), seed=2)


def offset_case(offset: float, a: int = 4, n: int = 8, b: int = 5) -> dict:
    """Small-integer rows (+ `offset`, an integer of magnitude 1e6): with N = 8 every partial sum is an integer below 2^24 and
    the division by N is exact, so q_a = offset + (the offset-free mean) exactly in float32, whatever the summation order.  The
    returns move with the offset: the QRDQN term is the offset-free one up to the rounding of T - theta."""
    rows = E.tie_rows_qr(a, n, ())
    g = torch.Generator().manual_seed(19)
    ret = torch.round(torch.randn(b, n, generator=g) * 2.5 * 4.0) / 4.0       # multiples of 0.25: exact next to 1e6 as well
    act = torch.tensor([i % a for i in range(b)])
    return cql_case(a, n, b, rows + offset, ret=ret + offset, act=act, weight=E.f32([1.0, 0.5, 2.0, 0.25, 1.5][:b]), seed=3)


# ---- float64 / float32 references --------------------------------------------------------------------------------------------
def cql64(rows: torch.Tensor, act: torch.Tensor) -> dict:
    """rows [A, N], act [B] -> q [A], p = softmax(q) [A], amp [A] (module docstring), lse, cql_b [B], and the scale of cql_b."""
    x = rows.double()
    q = x.mean(-1)
    m = q.max()
    e = torch.exp(q - m)
    lse = m + torch.log(e.sum())
    p = e / e.sum()
    t = x.abs().mean(-1) + (q - m).abs()
    amp = p * (1.0 + (1.0 - p) * t + ((p * t).sum() - p * t))
    return dict(q=q, p=p, amp=amp, lse=lse, cql_b=lse - q[act], scale=max(abs(float(lse)), float(x.abs().mean(-1).max())))


def loss32(case: dict):
    """tests/oracle_dcql.py's float32 expressions on the rows directly (autograd)
    -> prio [B], (loss, qr_loss, cql_loss), d loss / d rows [A, N] (the bias-row gradient)."""
    a, n, b = case["A"], case["N"], case["B"]
    x = case["rows"].float().clone().requires_grad_(True)
    all_dist = x.unsqueeze(0).expand(b, a, n)
    act = case["act"]
    w = torch.ones(b) if case["weight"] is None else case["weight"].float()
    curr = all_dist[torch.arange(b), act, :].unsqueeze(2)
    tgt = case["ret"].float().unsqueeze(1)
    diff = F.smooth_l1_loss(tgt.expand(-1, n, -1), curr.expand(-1, -1, n), reduction="none")
    huber = (diff * (case["tau"].float().view(1, -1, 1) - (tgt - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1)
    qr_loss = (huber * w).mean()
    q = all_dist.mean(2)
    cql_loss = q.logsumexp(1).mean() - q.gather(1, act.unsqueeze(1)).mean()
    loss = qr_loss + cql_loss * case["mqw"]
    loss.backward()
    return diff.detach().abs().sum(-1).mean(1), (loss.detach(), qr_loss.detach(), cql_loss.detach()), x.grad


def reference(case: dict) -> dict:
    """float64 values, per-element err32 of the float32 oracle formula and the bars of one update on an edge network:
    prio [B], qr_loss, cql_loss, loss, gbias [A, N]."""
    a, n, b, mqw = case["A"], case["N"], case["B"], case["mqw"]
    w = torch.ones(b) if case["weight"] is None else case["weight"].float()
    act = case["act"]
    r = E.qr_loss64(case["rows"][act], case["ret"], case["tau"], w)
    c = cql64(case["rows"], act)
    prio32, (l32, qr32, cq32), g32 = loss32(case)
    count = torch.bincount(act, minlength=a).double()
    cs = mqw / (b * n)
    out = dict(prio=r["prio"], prio_scale=r["prio_scale"], qr_loss=r["loss"], qr_loss_scale=r["loss_scale"],
               cql_loss=c["cql_b"].mean(), cql_loss_scale=torch.tensor(c["scale"], dtype=torch.float64), p=c["p"], q=c["q"],
               cql_b=c["cql_b"])
    out["loss"] = out["qr_loss"] + mqw * out["cql_loss"]
    out["loss_scale"] = out["qr_loss_scale"] + mqw * out["cql_loss_scale"]
    out["gbias_qr"] = E.scatter_rows(r["dtheta"], act, a)
    out["gbias_cql"] = (cs * (b * c["p"] - count))[:, None].expand(a, n)
    out["gbias"] = out["gbias_qr"] + out["gbias_cql"]
    qr_scale = E.scatter_rows(r["dtheta_scale"][:, None].expand(-1, n).contiguous(), act, a).max(-1, keepdim=True).values
    out["gbias_scale"] = qr_scale + (cs * (b * c["amp"] + count))[:, None]
    got32 = dict(prio=prio32, qr_loss=qr32, cql_loss=cq32, loss=l32, gbias=g32)
    for k, v in got32.items():
        out[k + "_32"] = v
        out[k + "_err32"] = (v.double() - out[k]).abs()
        out[k + "_bar"] = E.bar(out[k + "_err32"], out[k + "_scale"])
    return out


def err32_units(ref: dict) -> dict:
    """Largest err32 / (eps32 * scale) per quantity."""
    return {k: float((ref[k + "_err32"] / (E.EPS32 * torch.as_tensor(ref[k + "_scale"]).clamp_min(1e-300))).max())
            for k in ("prio", "qr_loss", "cql_loss", "loss", "gbias")}


def all_cases() -> dict:
    """name -> case: every input of tests/test_gpu_dcql_edges.py."""
    cases = {"tied": tied_case(), "tied_mixed_act": tied_case(act=torch.tensor([0, 4, 2, 4, 0, 1])),
             "dominated_act_hot": dominated_case(True), "dominated_act_other": dominated_case(False),
             "offset_plus": offset_case(1.0e6), "offset_minus": offset_case(-1.0e6), "offset_none": offset_case(0.0)}
    for a in A_GRID:
        for n in N_GRID:
            for b in (1, 5):
                cases[f"grid_A{a}_N{n}_B{b}"] = grid_case(a, n, b)
    for last in (False, True):
        for a, n in ((3, 255), (5, 65)):
            c = grid_case(a, n, 5)
            c["act"] = torch.full((5,), a - 1 if last else 0, dtype=torch.int64)
            cases[f"act_{'last' if last else 'first'}_A{a}_N{n}"] = c
    cases["weights"] = grid_case(3, 21, 5)
    return cases

