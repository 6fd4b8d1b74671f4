"""Inputs that put EXACT logits / quantiles into the per-sample heads of the distributional family (QRDQN, C51, Rainbow), and
plain float64 references of those heads.  Shared by tests/test_distq_edge_inputs_cpu.py and the GPU tests
tests/test_gpu_distq_edges.py / tests/test_gpu_rainbow_edges.py; nothing here touches the GPU path.

The last linear layer gets zero weights, so head[b, a * N + j] == bias[a * N + j] for every row, exactly, whatever the trunk
computes; `returns`, `act`, `weight` and (C51) a substituted `next_dist` carry the per-row variety.  Because the head weights are
zero, nothing flows below the head and the bias-row gradient is the column sum over b of the kernel's d_head.

References.  `head64`, `qr_loss64`, `c51_target64`, `c51_loss64`, `dueling64`, `dueling_bwd64`, `noisy_bias64` are written from
the reference formulas (qrdqn.py:111-128, c51.py:123-158, atari_network.py:203, discrete.py:366-374) in float64, closed forms
without autograd.  `qr_loss32` / `c51_loss32` are the float32 torch expressions of oracle/oracle_distq.py applied to the logits
directly (autograd); tests/test_distq_edge_inputs_cpu.py pins them to `oracle_distq.update_with_batch` on the edge networks.

Bars.  Exact claims are asserted exactly.  Everything else is per element against float64:
        |got - ref64| <= K * err32 + tiny,       K = 4,   err32 = |float32 oracle formula - ref64| of that element,
        tiny = 4 * eps32 * scale                 for every N,
`scale` being the largest magnitude the accumulation of that row passes through: its largest summand or partial sum (a sum
cannot be held to ulps of one summand; for the same-sign sums -- target mass, cross entropy, Huber sums -- that is the result
itself; for d logit_k = p_k g_k - p_k s it is max_k p_k max(|g_k|, |s|) of the row; for a bias gradient the sum of its rows'
scales).  K covers the kernels' other order of summation, the floor the elements where err32 happens to be zero.  Nothing was
tuned against what a kernel returns: the figures below are the float32 oracle's, measured on the host by
tests/test_distq_edge_inputs_cpu.py (`pytest -s` prints them), in units of eps32 * scale:

    case (largest err32 / (eps32 * scale) over its elements)          target   prio    loss    bias gradient
    c51 half-way returns, A 3, N 9                                     0.48     0.97    0.32    0.91
    c51 mass conservation, N 51, dz 0.4                                0.63     1.25    0.46    0.70
    c51 dominated row (+60 / -60)                                      0.32     0.52    0.47    0.00
    c51 graded row (0 .. -25)                                          0.32     0.35    0.38    0.89
    c51 clamp returns                                                  0.77     0.55    0.48    1.98
    c51 grid (A, N) = (1, 256) .. (2, 51), B 1 and 5                   1.12     1.12    0.95    0.99
    qr |d| == 1 and its neighbours                                     -        0.57    0.56    0.58
    qr returns ~1e4                                                    -        0.19    0.20    1.01
    qr grid, B 1 and 5                                                 -        0.97    0.73    1.93
    forward, the grid's shapes: softmax dist 0.89, Q (C51) 1.11, Q (QR mean) 0.46

so the bars in use are 4 err32 + 4 ulp of the row's scale, and the float32 oracle itself never needs more than 2 ulp (asserted
<= 4 in the CPU test).  No case had to be dropped as ill-conditioned: with exact logits every quantity above is a short
same-sign sum or a product.
Two comparisons are not `k err32 + tiny`: the quantile loss in its linear region against the closed form -w tau_i / B
(+w (1 - tau_i) / B), bar 4 N eps32 of the closed form (N rounded terms enter each entry, whatever the order they are added
in); and the cross entropy of a target sitting on an atom whose probability underflowed, which must be -m logf(1e-8f) to 2 ulp
(one for the device's logf, one for the product).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_distq as OQ
from oracle import oracle_rainbow as ORB

EPS32 = float(np.finfo(np.float32).eps)
K_ERR = 4.0
FLOOR_ULPS = 4.0
C, H, W = 2, 44, 36                     # the smallest network the suite uses
QR, C51 = "qr", "c51"
GRID = [(1, 256), (64, 2), (3, 255), (5, 65), (4, 64), (2, 51)]        # (A, N); (4, 64) and (64, 2) have no padding columns
RAINBOW_GRID = [(1, 51), (6, 51), (3, 33), (64, 2)]


def bar(err32, scale):
    """K * err32 + FLOOR_ULPS * eps32 * scale, elementwise (scale broadcasts)."""
    return K_ERR * torch.as_tensor(err32, dtype=torch.float64) + FLOOR_ULPS * EPS32 * torch.as_tensor(scale, dtype=torch.float64)


def head_width(a: int, n: int) -> int:
    return (a * n + 31) // 32 * 32


def f32(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def nextafter32(x: float, toward: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(toward)))


# ---- edge networks -----------------------------------------------------------------------------------------------------------
def edge_params(a: int, n: int, rows: torch.Tensor, seed: int = 1) -> dict:
    """QRDQNet / C51Net parameters whose head is the constant `rows` [A, N]: zero head weights, bias = rows."""
    p = OQ.init_params(C, H, W, a, n, seed)
    p["fc2.w"] = torch.zeros_like(p["fc2.w"])
    p["fc2.b"] = rows.reshape(-1).to(torch.float32).clone()
    return p


def edge_rainbow(a: int, n: int, bq_mu, bq_sigma, bv_mu, bv_sigma, eps_q, eps_v, seed: int = 1):
    """RainbowNet parameters and noise whose Q.2 / V.2 outputs are their effective biases: zero weight mu and sigma."""
    p, noise = ORB.init_params(C, H, W, a, n, seed)
    for L, mu, sg, eps in (("Q2", bq_mu, bq_sigma, eps_q), ("V2", bv_mu, bv_sigma, eps_v)):
        p[L + ".mu_W"], p[L + ".sigma_W"] = torch.zeros_like(p[L + ".mu_W"]), torch.zeros_like(p[L + ".sigma_W"])
        p[L + ".mu_b"], p[L + ".sigma_b"] = f32(mu).reshape(-1).clone(), f32(sg).reshape(-1).clone()
        noise[L + ".eps_q"] = f32(eps).reshape(-1).clone()
    return p, noise


def obs_batch(b: int, seed: int = 0) -> np.ndarray:
    """uint8 NCHW observations (the oracle's layout; the engines take its NHWC permutation)."""
    return np.random.default_rng(seed).integers(0, 256, size=(b, C, H, W), dtype=np.uint8)


def support32(v_min: float, v_max: float, n: int) -> torch.Tensor:
    return torch.linspace(v_min, v_max, n)


# ---- rows --------------------------------------------------------------------------------------------------------------------
def random_rows(a: int, n: int, seed: int, scale: float = 2.0) -> torch.Tensor:
    return torch.randn(a, n, generator=torch.Generator().manual_seed(seed)) * scale


def dominated_row(n: int, hot: int) -> torch.Tensor:
    """One logit +60, the rest -60: every other probability is e^-120, which underflows to 0.0f."""
    r = torch.full((n,), -60.0)
    r[hot] = 60.0
    return r


def graded_row(n: int) -> torch.Tensor:
    """Logits 0, -5, -10, -15, -20, -25 in turn: p ~ 1, 7e-3, 5e-5, 3e-7, 2e-9, 1e-11 straddles the 1e-8 of log(p + 1e-8)."""
    return torch.tensor([-5.0 * (j % 6) for j in range(n)])


def random_dist(b: int, n: int, seed: int, zeros: bool = False) -> torch.Tensor:
    """Rows of a probability simplex in float32 (`zeros`: every third entry exactly 0)."""
    x = torch.rand(b, n, generator=torch.Generator().manual_seed(seed)) + 0.05
    if zeros:
        x[:, ::3] = 0.0
    return (x / x.sum(-1, keepdim=True)).to(torch.float32)


def tie_rows_qr(a: int, n: int, tied: tuple) -> torch.Tensor:
    """Small-integer quantile rows: every summation order is exact.  The tied actions share one row (integers in [3, 7], mean
    >= 3.5), the others are integers in [-4, 2] (mean <= 2) and differ from one another."""
    base = torch.tensor([float(j % 5) - 2.0 for j in range(n)])          # integers in [-2, 2]
    rows = torch.stack([base.roll(i) - float(i % 3) for i in range(a)])
    for i in tied:
        rows[i] = base + 5.0
    return rows


def tie_rows_c51(a: int, n: int, tied: tuple) -> torch.Tensor:
    """Dominated rows: p is exactly one-hot in float32, so Q == support[hot] under every summation order.  The tied actions sit
    on atom n - 2, the others on lower atoms."""
    rows = torch.stack([dominated_row(n, i % (n - 2)) for i in range(a)])
    for i in tied:
        rows[i] = dominated_row(n, n - 2)
    return rows


# ---- float64 references ------------------------------------------------------------------------------------------------------
def softmax64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    e = torch.exp(x - x.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True)


def head64(kind: str, rows: torch.Tensor, support: torch.Tensor | None = None) -> dict:
    """rows [A, N] -> dist [A, N], q [A], act (first maximum), and the floor scales of dist and q."""
    if kind == QR:
        d = rows.double()
        q, qs = d.mean(-1), d.abs().mean(-1)
    else:
        d = softmax64(rows)
        z = support.double()
        q, qs = (d * z).sum(-1), (d * z.abs()).sum(-1)
    act = int(torch.argmax(q))                                              # torch.argmax: the first of several maxima
    return dict(dist=d, q=q, act=act, dist_scale=d.abs().max(-1, keepdim=True).values, q_scale=qs)


GREEDY_GAP_ULPS = 32.0


def greedy_gap(h: dict) -> float:
    """Gap between the two largest float64 Q of `head64`'s result in units of eps32 * (largest Q scale): above GREEDY_GAP_ULPS
    float32 cannot mistake the greedy action (each Q is within a few ulp of its scale), inf at A == 1."""
    if h["q"].numel() == 1:
        return float("inf")
    top2 = torch.topk(h["q"], 2).values
    return float(top2[0] - top2[1]) / (EPS32 * float(h["q_scale"].max()))


def head32(kind: str, rows: torch.Tensor, support: torch.Tensor | None = None):
    """oracle_distq.dist / q_values on the head output directly, float32."""
    d = rows.float() if kind == QR else rows.float().softmax(dim=-1)
    q = d.mean(-1) if kind == QR else (d * support).sum(-1)
    return d, q


def qr_loss64(theta, T, tau, weight, B: int | None = None) -> dict:
    """theta, T [B, N]; tau [N]; weight [B] -> huber, prio [B], loss, dtheta [B, N] and the floor scales."""
    theta, T, tau, w = theta.double(), T.double(), tau.double(), weight.double()
    b, n = theta.shape
    B = b if B is None else B
    d = T[:, None, :] - theta[:, :, None]                                   # [b, i, j] = T_j - theta_i
    ad = d.abs()
    l = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    wt = (tau[None, :, None] - (d <= 0).double()).abs()
    huber, prio = (l * wt).sum(-1).mean(-1), l.sum(-1).mean(-1)
    terms = wt * d.clamp(-1.0, 1.0)
    fac = (w / (B * n))[:, None]
    return dict(huber=huber, prio=prio, loss=(huber * w).sum() / B, dtheta=-fac * terms.sum(-1),
                prio_scale=prio, loss_scale=(huber * w).abs().sum() / B,
                dtheta_scale=(fac.abs() * terms.abs().sum(-1)).max(-1).values)


def qr_loss32(theta, T, tau, weight, B: int | None = None):
    """oracle_distq.update_with_batch's QRDQN branch on theta directly, float32 autograd -> prio, loss, dtheta."""
    th = theta.float().clone().requires_grad_(True)
    B = th.shape[0] if B is None else B
    curr, tgt = th.unsqueeze(2), T.float().unsqueeze(1)
    diff = F.smooth_l1_loss(tgt.expand(-1, th.shape[1], -1), curr.expand(-1, -1, th.shape[1]), reduction="none")
    huber = (diff * (tau.float().view(1, -1, 1) - (tgt - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1)
    loss = (huber * weight.float()).sum() / B
    loss.backward()
    return diff.detach().abs().sum(-1).mean(1), loss.detach(), th.grad


def c51_target64(ret, nd, support, v_min: float, v_max: float) -> torch.Tensor:
    """C51._target_dist's projection (c51.py:133-141): ret, nd [B, N] -> m [B, N] (float64 arithmetic on the float32 support)."""
    n = support.numel()
    dz = (v_max - v_min) / (n - 1)
    ts = ret.double().clamp(v_min, v_max)
    wgt = (1.0 - (ts[:, None, :] - support.double()[None, :, None]).abs() / dz).clamp(0.0, 1.0)
    return (wgt * nd.double()[:, None, :]).sum(-1)


def c51_loss64(logits, m, weight, B: int | None = None) -> dict:
    """logits [B, N] of the taken action, target m [B, N] (float64), weight [B] -> ce [B], loss, dlogits [B, N], scales."""
    p, w = softmax64(logits), weight.double()
    B = p.shape[0] if B is None else B
    terms = m * torch.log(p + 1e-8)
    ce = -terms.sum(-1)
    g = -(w / B)[:, None] * m / (p + 1e-8)
    s = (p * g).sum(-1, keepdim=True)
    return dict(ce=ce, loss=(ce * w).sum() / B, dlogits=p * (g - s), ce_scale=terms.abs().sum(-1),
                loss_scale=(terms.abs().sum(-1) * w.abs()).sum() / B,
                dlogits_scale=(p * torch.maximum(g.abs(), s.abs())).max(-1).values)


def c51_loss32(logits, ret, nd, weight, support, v_min: float, v_max: float, B: int | None = None):
    """oracle_distq.target_dist and the C51 branch of update_with_batch on the logits directly, float32 autograd
    -> target, ce, loss, dlogits."""
    n = support.numel()
    delta_z = (v_max - v_min) / (n - 1)
    ts = ret.float().clamp(v_min, v_max)
    tgt = ((1 - (ts.unsqueeze(1) - support.view(1, -1, 1)).abs() / delta_z).clamp(0, 1) * nd.float().unsqueeze(1)).sum(-1)
    x = logits.float().clone().requires_grad_(True)
    B = x.shape[0] if B is None else B
    ce = -(tgt * torch.log(x.softmax(dim=-1) + 1e-8)).sum(1)
    loss = (ce * weight.float()).sum() / B
    loss.backward()
    return tgt, ce.detach(), loss.detach(), x.grad


def noisy_bias64(mu, sigma, eps) -> torch.Tensor:
    return mu.double() + sigma.double() * eps.double()


def dueling64(bq: torch.Tensor, bv: torch.Tensor) -> torch.Tensor:
    """bq [A, N], bv [N] -> logits [A, N] = q - mean_a q + v."""
    bq = bq.double()
    return bq - bq.mean(0, keepdim=True) + bv.double()[None, :]


def dueling_bwd64(dl: torch.Tensor):
    """dl [A, N] -> (dq [A, N] = dl - mean_a dl, dv [N] = sum_a dl)."""
    dl = dl.double()
    return dl - dl.mean(0, keepdim=True), dl.sum(0)


def scatter_rows(dl: torch.Tensor, act: torch.Tensor, a: int) -> torch.Tensor:
    """Per-sample gradient rows [B, N] of the taken actions -> summed head gradient [A, N]."""
    out = torch.zeros(a, dl.shape[1], dtype=dl.dtype)
    out.index_add_(0, act.long(), dl)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return torch.Generator().manual_seed(seed)


def c51_case(a: int, n: int, b: int, v_min: float, v_max: float, rows: torch.Tensor, ret: torch.Tensor, nd: torch.Tensor,
             act=None, weight=None, seed: int = 0) -> dict:
    g = _rng(100 + seed)
    act = torch.randint(0, a, (b,), generator=g) if act is None else torch.as_tensor(act, dtype=torch.int64)
    return dict(kind=C51, A=a, N=n, B=b, v_min=float(v_min), v_max=float(v_max), rows=rows.float(), ret=ret.float(),
                nd=nd.float(), act=act, weight=weight, obs=obs_batch(b, seed), support=support32(v_min, v_max, n))


def qr_case(a: int, n: int, b: int, rows: torch.Tensor, ret: torch.Tensor, act=None, weight=None, seed: int = 0) -> dict:
    g = _rng(100 + seed)
    act = torch.randint(0, a, (b,), generator=g) if act is None else torch.as_tensor(act, dtype=torch.int64)
    return dict(kind=QR, A=a, N=n, B=b, rows=rows.float(), ret=ret.float(), act=act, weight=weight, obs=obs_batch(b, seed),
                tau=OQ.tau_hat(n))


def halfway_case(a: int = 3, b: int = 5) -> dict:
    """T_j = z_j + 0.5 on the integer support -4 .. 4: nd_j splits 0.5 / 0.5 between atoms j and j + 1 (the last is clamped)."""
    n = 9
    z = support32(-4, 4, n)
    return c51_case(a, n, b, -4, 4, random_rows(a, n, 3), (z + 0.5).repeat(b, 1), random_dist(b, n, 4), seed=1)


def mass_case(a: int = 2, b: int = 8) -> dict:
    """v_min, v_max, N = -10, 10, 51 (dz = 0.4, inexact in float32), random returns inside and outside the range."""
    n = 51
    ret = torch.randn(b, n, generator=_rng(5)) * 8.0                       # ~21 % beyond +-10
    return c51_case(a, n, b, -10, 10, random_rows(a, n, 6), ret, random_dist(b, n, 7, zeros=True), seed=2)


def dominated_case(graded: bool, a: int = 3, b: int = 5) -> dict:
    """Every action's row is dominated (hot atom 2 * act + 1) or graded; the target (random next_dist with exact zeros, returns
    on and between the atoms) puts mass on atoms whose probability is 0.0f / below 1e-8."""
    n = 9
    rows = torch.stack([graded_row(n).roll(i) if graded else dominated_row(n, 2 * i + 1) for i in range(a)])
    z = support32(-4, 4, n)
    ret = z.repeat(b, 1) + torch.tensor([0.0, 0.25, 0.5, -0.75, 1.0])[:b, None]
    return c51_case(a, n, b, -4, 4, rows, ret, random_dist(b, n, 8, zeros=True), weight=f32([1.0, 0.5, 2.0, 0.25, 1.5][:b]), seed=3)


def clamp_returns() -> torch.Tensor:
    """[9] returns: v_min, v_max, their float32 neighbours inward and outward, far outside, +-inf (v_min, v_max = -4, 4)."""
    return f32([-4.0, 4.0, nextafter32(-4.0, 0.0), nextafter32(4.0, 0.0), nextafter32(-4.0, -9.0), nextafter32(4.0, 9.0),
                -1e6, 1e6, float("inf")])


def clamp_case(a: int = 3) -> dict:
    """Row 0: the nine clamp returns; row 1: the same with -inf for +inf; row 2: everything below v_min; row 3: everything
    above v_max (all mass into one end atom)."""
    n = 9
    r0 = clamp_returns()
    r1 = r0.clone()
    r1[8] = float("-inf")
    ret = torch.stack([r0, r1, torch.full((n,), -1e6), torch.full((n,), float("inf"))])
    ret[2, ::2] = nextafter32(-4.0, -9.0)
    return c51_case(a, n, 4, -4, 4, random_rows(a, n, 9), ret, random_dist(4, n, 10), seed=4)


def grid_case(kind: str, a: int, n: int, b: int) -> dict:
    g = _rng(1000 * a + 10 * n + b)
    rows = random_rows(a, n, 11 + a + n)
    act = torch.randint(0, a, (b,), generator=g)
    weight = (torch.rand(b, generator=g) + 0.25) if b > 1 else None
    if kind == C51:
        ret = torch.randn(b, n, generator=g) * 3.0                         # v = +-5: some beyond
        return c51_case(a, n, b, -5, 5, rows, ret, random_dist(b, n, 12 + n, zeros=(n > 2)), act=act, weight=weight, seed=5)
    ret = torch.randn(b, n, generator=g) * 2.5                             # |d| on both sides of 1
    return qr_case(a, n, b, rows, ret, act=act, weight=weight, seed=5)


UNIT_EDGES = tuple(x for c in (1.0, -1.0) for x in (c, nextafter32(c, 0.0), nextafter32(c, 9.0 * c)))


def qr_unit_case(a: int = 3, b: int = 6) -> dict:
    """theta == 0 in the taken action's row, so T_j - theta_i == T_j exactly: the returns cycle through +1, -1 and the float32
    neighbours of both, inward and outward (UNIT_EDGES)."""
    n = 7
    rows = torch.stack([torch.full((n,), float(i)) for i in range(a)])
    ret = f32([[UNIT_EDGES[(j + r) % 6] for j in range(n)] for r in range(b)])
    return qr_case(a, n, b, rows, ret, act=torch.zeros(b, dtype=torch.int64), weight=f32([1.0, 0.5, 2.0, 0.25, 1.5, 1.0][:b]), seed=6)


def qr_large_case(a: int = 3, n: int = 33, b: int = 5) -> dict:
    g = _rng(13)
    return qr_case(a, n, b, random_rows(a, n, 14), 1e4 + torch.randn(b, n, generator=g) * 50.0, weight=torch.rand(b, generator=g) + 0.5,
                   seed=7)


def reference(case: dict) -> dict:
    """float64 values, per-element err32 of the float32 oracle formula and the bars of one update on an edge network:
    prio [B], loss, (C51) target [B, N], gbias [A, N] (the bias-row gradient)."""
    a, n, b = case["A"], case["N"], case["B"]
    w = torch.ones(b) if case["weight"] is None else case["weight"].float()
    taken = case["rows"][case["act"]]
    out: dict = {}
    if case["kind"] == QR:
        r = qr_loss64(taken, case["ret"], case["tau"], w)
        prio32, loss32, d32 = qr_loss32(taken, case["ret"], case["tau"], w)
        d64, rows_scale = r["dtheta"], r["dtheta_scale"]
        out.update(prio=r["prio"], prio_scale=r["prio_scale"], loss=r["loss"], loss_scale=r["loss_scale"])
    else:
        m = c51_target64(case["ret"], case["nd"], case["support"], case["v_min"], case["v_max"])
        r = c51_loss64(taken, m, w)
        t32, prio32, loss32, d32 = c51_loss32(taken, case["ret"], case["nd"], w, case["support"], case["v_min"], case["v_max"])
        d64, rows_scale = r["dlogits"], r["dlogits_scale"]
        t_scale = torch.maximum(m.max(-1).values, case["nd"].double().max(-1).values)[:, None]
        out.update(target=m, target_scale=t_scale, target_err32=(t32.double() - m).abs(), target32=t32,
                   prio=r["ce"], prio_scale=r["ce_scale"], loss=r["loss"], loss_scale=r["loss_scale"])
    out["prio_err32"], out["loss_err32"] = (prio32.double() - out["prio"]).abs(), (loss32.double() - out["loss"]).abs()
    out["rows"], out["rows32"] = d64, d32
    out["gbias"] = scatter_rows(d64, case["act"], a)
    out["gbias_err32"] = (scatter_rows(d32.double(), case["act"], a) - out["gbias"]).abs()
    out["gbias_scale"] = scatter_rows(rows_scale[:, None].expand(-1, n).contiguous(), case["act"], a).max(-1, keepdim=True).values
    for k in ("prio", "loss", "gbias") + (("target",) if case["kind"] == C51 else ()):
        out[k + "_bar"] = bar(out[k + "_err32"], out[k + "_scale"])
    return out


def err32_units(ref: dict) -> dict:
    """Largest err32 / (eps32 * scale) per quantity: the figures of this module's docstring."""
    res = {}
    for k in ("target", "prio", "loss", "gbias"):
        if k in ref:
            res[k] = float((ref[k + "_err32"] / (EPS32 * torch.as_tensor(ref[k + "_scale"]).clamp_min(1e-300))).max())
    return res


# ---- Rainbow -----------------------------------------------------------------------------------------------------------------
def rainbow_case(a: int, n: int, b: int, pattern: str = "random", zero_noise: bool = False, seed: int = 0) -> dict:
    """Q.2 / V.2 bias mu, bias sigma and eps_q of an edge RainbowNet, and one minibatch.
      random      N(0, 1) * 1.5 advantages and values, sigma 0.3, reference-style noise
      dominated   the value row is +60 / -60 (hot atom 1), the advantages small: every action's row is dominated
      on_atom     v_min, v_max, N = -4, 4, 9 (N is forced to 9): integer returns, a permutation of the atoms
      clamp       the nine clamp returns (N forced to 9)"""
    g = _rng(500 + 10 * a + n + seed)
    if pattern in ("on_atom", "clamp"):
        n = 9
    v_min, v_max = (-4.0, 4.0) if n == 9 else (-5.0, 5.0)
    bq_mu, bv_mu = torch.randn(a, n, generator=g) * 1.5, torch.randn(n, generator=g) * 1.5
    if pattern == "dominated":
        bq_mu, bv_mu = bq_mu * 0.1, dominated_row(n, 1)
    bq_sigma, bv_sigma = torch.full((a, n), 0.3), torch.full((n,), 0.3)
    x, y = torch.randn(a, n, generator=g), torch.randn(n, generator=g)
    eps_q, eps_v = x.sign() * x.abs().sqrt(), y.sign() * y.abs().sqrt()
    if zero_noise:
        eps_q, eps_v = torch.zeros(a, n), torch.zeros(n)
    z = support32(v_min, v_max, n)
    if pattern == "on_atom":
        ret = torch.stack([z[torch.randperm(n, generator=g)] for _ in range(b)])
    elif pattern == "clamp":
        ret = clamp_returns().repeat(b, 1)
        ret[1::2, 8] = float("-inf")
    else:
        ret = torch.randn(b, n, generator=g) * 3.0
    return dict(A=a, N=n, B=b, v_min=v_min, v_max=v_max, support=z, bq_mu=bq_mu, bq_sigma=bq_sigma, bv_mu=bv_mu, bv_sigma=bv_sigma,
                eps_q=eps_q, eps_v=eps_v, ret=ret.float(), nd=random_dist(b, n, 20 + seed, zeros=(n > 2)),
                act=torch.randint(0, a, (b,), generator=g), weight=(torch.rand(b, generator=g) + 0.25) if b > 1 else None,
                obs=obs_batch(b, 8 + seed))


def rainbow_params(case: dict):
    return edge_rainbow(case["A"], case["N"], case["bq_mu"], case["bq_sigma"], case["bv_mu"], case["bv_sigma"], case["eps_q"],
                        case["eps_v"])


def rainbow32(case: dict, training: bool = True) -> dict:
    """oracle_rainbow's float32 expressions on the biases directly (autograd): logits, dist, q, target, ce, loss and the
    gradients of the four bias tensors."""
    t = {k: case[k].float().clone().requires_grad_(True) for k in ("bq_mu", "bq_sigma", "bv_mu", "bv_sigma")}
    bq = t["bq_mu"] + t["bq_sigma"] * case["eps_q"] if training else t["bq_mu"] + 0.0 * t["bq_sigma"]
    bv = t["bv_mu"] + t["bv_sigma"] * case["eps_v"] if training else t["bv_mu"] + 0.0 * t["bv_sigma"]
    logits = bq - bq.mean(dim=0, keepdim=True) + bv[None, :]
    d = logits.softmax(dim=-1)
    w = torch.ones(case["B"]) if case["weight"] is None else case["weight"].float()
    n = case["N"]
    delta_z = (case["v_max"] - case["v_min"]) / (n - 1)
    ts = case["ret"].clamp(case["v_min"], case["v_max"])
    tgt = ((1 - (ts.unsqueeze(1) - case["support"].view(1, -1, 1)).abs() / delta_z).clamp(0, 1) * case["nd"].unsqueeze(1)).sum(-1)
    ce = -(tgt * torch.log(d[case["act"]] + 1e-8)).sum(1)
    loss = (ce * w).mean()
    loss.backward()
    return dict(logits=logits.detach(), dist=d.detach(), q=(d.detach() * case["support"]).sum(-1), target=tgt, ce=ce.detach(),
                loss=loss.detach(), grads={k: v.grad for k, v in t.items()})


def rainbow64(case: dict, training: bool = True) -> dict:
    """The float64 yardstick of the same, closed forms, with the bars of every quantity."""
    a, n, b = case["A"], case["N"], case["B"]
    z = torch.zeros(())
    bq = noisy_bias64(case["bq_mu"], case["bq_sigma"], case["eps_q"] if training else z)
    bv = noisy_bias64(case["bv_mu"], case["bv_sigma"], case["eps_v"] if training else z)
    logits = dueling64(bq, bv)
    h = head64(C51, logits, case["support"])
    w = torch.ones(b) if case["weight"] is None else case["weight"].float()
    m = c51_target64(case["ret"], case["nd"], case["support"], case["v_min"], case["v_max"])
    r = c51_loss64(logits[case["act"]], m, w)
    dl = scatter_rows(r["dlogits"], case["act"], a)
    dq, dv = dueling_bwd64(dl)
    grads = dict(bq_mu=dq, bq_sigma=dq * case["eps_q"].double(), bv_mu=dv, bv_sigma=dv * case["eps_v"].double())
    o32 = rainbow32(case, training)
    # scale of the bias gradients: the sum of the rows' d-logit scales (every entry of dq / dv is a sum of at most B + A of them)
    gscale = r["dlogits_scale"].sum()
    out = dict(logits=logits, dist=h["dist"], q=h["q"], act=h["act"], target=m, ce=r["ce"], loss=r["loss"], grads=grads, dl=dl,
               dist_bar=bar((o32["dist"].double() - h["dist"]).abs(), h["dist_scale"]),
               q_bar=bar((o32["q"].double() - h["q"]).abs(), h["q_scale"]),
               target_bar=bar((o32["target"].double() - m).abs(),
                              torch.maximum(m.max(-1).values, case["nd"].double().max(-1).values)[:, None]),
               ce_bar=bar((o32["ce"].double() - r["ce"]).abs(), r["ce_scale"]),
               loss_bar=bar((o32["loss"].double() - r["loss"]).abs(), r["loss_scale"]), o32=o32)
    out["grad_bars"] = {k: bar((o32["grads"][k].double() - grads[k]).abs(),
                               gscale * (1.0 if k.endswith("mu") else case["eps_q" if k[1] == "q" else "eps_v"].double().abs()))
                        for k in grads}
    return out
