"""Inputs that put EXACT quantile values into the per-sample kernels of IQN (iqn_head_kernel, iqn_select_kernel, iqn_loss_kernel,
iqn_mean_kernel of ts_iqn.hip), float64 references of those kernels, and the float64 yardsticks of the cosine-embedding kernels
and of the whole network.  Shared by tests/test_iqn_edge_inputs_cpu.py and the GPU tests tests/test_gpu_iqn_edges.py /
tests/test_gpu_iqn_routes.py; nothing here touches the GPU path.

Edge network.  `edge_params(A, b2)` is `oracle_iqn.init_params` on the suite's smallest network ((C, H, W) = (2, 44, 36),
F = 128) with fc2.w = 0 and fc2.b = b2, so out[r, a] == b2[a] exactly for every row r = b N + n and every fraction.  The
consequence: theta_i = b2[act_b] is the SAME for all i in these cases; the per-i variety comes from tau_i and the per-j variety
from T_j (the random-weight tests of tests/test_gpu_iqn.py cover the row indexing of theta).  Nothing flows below the head, so
the gradient below [W2; b2] must be exactly 0, and the bias-row gradient is the column sum of the kernel's d_out:
gbias[a] = sum over the samples b with act_b == a, and over i, of d loss / d theta_i.

References.  `iqn_loss64` (huber_b, prio_b, loss, d loss / d theta_i = -(w_b / (B N)) sum_j |tau_i - 1{d_ij <= 0}|
clamp(d_ij, -1, 1)) and `head64` (Q as a mean, act as numpy's first maximum) are float64 closed forms written from
iqn.py:162-180 without autograd.  `loss32` is the float32 torch expression of `oracle_iqn.loss_terms` applied to the logits
directly (autograd); tests/test_iqn_edge_inputs_cpu.py pins it to `oracle_iqn.update_with_batch` on the edge networks.

Bars.  Exact claims are asserted exactly.  Everything else is per element against float64, the project's own rule:
        |got - ref64| <= 4 * err32 + 4 * eps32 * scale,     err32 = |float32 oracle formula - ref64| of that element,
`scale` being the largest magnitude the accumulation passes through, bounded by the sum of the absolute summands: prio_b (a
same-sign sum), sum_b |huber_b w_b| / B for the loss, sum over the rows (b, i) of an action of (w_b / (B N)) sum_j |w_ij
clamp(d_ij)| for a bias gradient, |b2[a]| for Q.  Nothing was tuned against what a kernel returns.  A float32 sum of N EQUAL
terms added one after the other can be (N - 1) / 2 ulp off in the worst case (1.9 ulp of the mean at N = 7, 16 at N = 64), so
the Q comparisons at N = 64 use biases that are multiples of 2^-10 (every order of summation is exact) and generic floats at
N <= 7.  The figures below are the float32 oracle's, measured on the host by tests/test_iqn_edge_inputs_cpu.py (`pytest -s`
prints them; another host's torch may add in another order and move them a little), in units of eps32 * scale:

    case group (largest err32 / (eps32 * scale) over its elements)     prio    loss    bias gradient
    linear region, (N, N') = (2, 2) .. (64, 64), both signs            1.16    0.97    1.40
    |d| == 1 and its neighbours                                        0.57    0.02    0.30
    mixed, (A, N, N') = (1, 2, 2) .. (3, 64, 2), +- weight             1.26    0.93    0.60
    mean kernel, B = 1 and 1030                                        0.96    0.65    0.18
    forward Q, A = 1 .. 64, N = 2, 7, 64: 1.25

so the float32 oracle itself never needs more than the 4-ulp floor (asserted <= 4 in the CPU test).
One comparison is not `4 err32 + floor`: the bias gradient in the linear region against the closed form
sum over rows of -w_b N' tau_i / (B N) (+w_b N' (1 - tau_i) / (B N)), bar 4 N' eps32 of the closed form's absolute sum (the bar
the distributional suite uses).  Its shapes keep N <= 7 N' - 3 and one sample per action, so that even the worst case of the
roundings that enter one entry (N' adds, the scale factor, N rows) stays inside: (N' + N + 3) / 2 <= 4 N'.

Part B.  `embed_mul64` / `embed_mul_bwd64` and `net_loss64` are the float64 yardsticks of the embedding kernels and of the whole
update.  The cosine arguments are formed in float32 exactly as the reference forms them (fl32(pi) * (k + 1) rounded, then
tau * ipi rounded); everything after that is float64.  The bar of every tensor there is max(1e-5, 2 e_ref) of its scale, e_ref
being the float32 torch expression's own `rel_err` against float64 on the same input.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_dqn as OD
from tests import oracle_iqn as OI

EPS32 = float(np.finfo(np.float32).eps)
K_ERR = 4.0
FLOOR_ULPS = 4.0
C, H, W = 2, 44, 36                     # the smallest network the suite uses: F = 128
FEAT = 128
GREEDY_GAP_ULPS = 32.0
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
# constants of ts_iqn.hip the part-B shapes are chosen against (tests/test_iqn_edge_inputs_cpu.py recomputes the tile counts)
BM, FWD_SHARES, BWD_SLABS, FUSED_FROM_ROWS = 64, 16, 8, 1 << 14


def bar(err32, scale):
    """K * err32 + FLOOR_ULPS * eps32 * scale, elementwise (scale broadcasts)."""
    return K_ERR * torch.as_tensor(err32, dtype=torch.float64) + FLOOR_ULPS * EPS32 * torch.as_tensor(scale, dtype=torch.float64)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def rel_bar(e_ref: float) -> float:
    """Part B: the project's 1e-5 of a tensor's scale, widened to twice the float32 reference's own error where that is larger."""
    return max(1e-5, 2.0 * e_ref)


def head_ld(a: int) -> int:
    return (a + 31) // 32 * 32


def f32(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def nextafter32(x: float, toward: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(toward)))


def _rng(seed):
    return torch.Generator().manual_seed(seed)


# ---- edge network ------------------------------------------------------------------------------------------------------------
def edge_params(a: int, b2: torch.Tensor, seed: int = 1) -> dict:
    """IQN parameters whose head is the constant b2 [A]: zero fc2 weights, fc2.b = b2."""
    p = OI.init_params(C, H, W, a, seed=seed)
    assert p["emb.w"].shape[0] == FEAT
    p["fc2.w"] = torch.zeros_like(p["fc2.w"])
    p["fc2.b"] = b2.reshape(-1).to(torch.float32).clone()
    return p


def obs_batch(b: int, seed: int = 0) -> np.ndarray:
    """uint8 NCHW observations (the oracle's layout; the engine takes its NHWC permutation)."""
    return np.random.default_rng(seed).integers(0, 256, size=(b, C, H, W), dtype=np.uint8)


def head_bias(a: int, n: int, seed: int, shift: float = 0.0) -> torch.Tensor:
    """Per-action biases N(shift, 2^2): generic floats for N <= 7, multiples of 2^-10 above (module docstring)."""
    v = torch.randn(a, generator=_rng(seed)) * 2.0 + shift
    if n > 7:
        v = torch.round(v * 1024.0) / 1024.0
    return v.float()


def tie_bias(a: int, tied: tuple, negative: bool = False) -> torch.Tensor:
    """The tied actions hold 3.5, action i of the others -1 - i / 8 (distinct, all dyadic); `negative`: everything 20 lower."""
    v = torch.tensor([-1.0 - 0.125 * i for i in range(a)])
    for i in tied:
        v[i] = 3.5
    return v - (20.0 if negative else 0.0)


# (A, tied actions).  Lanes 5 and 37 differ in bit 5 alone: they meet in the first step (offset 32) of the wave's xor butterfly;
# (0, 63) and (31, 32) differ in every bit, so the tie has to survive all six steps; three tied lanes; every action tied
# (act = 0) at each A of the grid; a strict maximum on the last action
TIES = [(64, (0, 63)), (33, (31, 32)), (64, (31, 32)), (64, (5, 37)), (64, (1, 2, 62))] \
    + [(a, tuple(range(a))) for a in (1, 2, 32, 33, 64)] + [(a, (a - 1,)) for a in (2, 32, 33, 64)]
HEAD_A, HEAD_N, HEAD_B = (1, 2, 32, 33, 64), (2, 7, 64), (1, 5)


def head64(b2: torch.Tensor) -> dict:
    """b2 [A] -> q [A] (the mean of N equal values), act (numpy's first maximum), the floor scale of q."""
    q = b2.double()
    return dict(q=q, act=int(np.argmax(q.numpy())), q_scale=q.abs())


def head32(b2: torch.Tensor, n: int) -> torch.Tensor:
    """oracle_iqn.policy_forward's Q on the logits directly, float32."""
    return b2.float().view(1, -1, 1).expand(1, -1, n).contiguous().mean(2)[0]


def greedy_gap(h: dict) -> float:
    """Gap between the two largest float64 Q in units of eps32 * (largest |Q|): above GREEDY_GAP_ULPS float32 cannot mistake
    the greedy action (each Q is within a few ulp of its scale); inf at A == 1."""
    if h["q"].numel() == 1:
        return float("inf")
    top2 = torch.topk(h["q"], 2).values
    return float(top2[0] - top2[1]) / (EPS32 * float(h["q_scale"].max()))


# ---- the loss, float64 closed forms and the float32 formula --------------------------------------------------------------------
def iqn_loss64(theta, T, tau, weight, B: int | None = None) -> dict:
    """theta [B] (the same for every i), T [B, N'], tau [B, N], weight [B] -> huber_b, prio_b [B], loss, dtheta [B, N] and the
    floor scales (iqn.py:162-180; d_ij = T_j - theta does not depend on i here)."""
    theta, T, tau, w = theta.double(), T.double(), tau.double(), weight.double()
    b, n = tau.shape
    B = b if B is None else B
    d = T - theta[:, None]                                                  # [b, j]
    ad = d.abs()
    l = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    wt = (tau[:, :, None] - (d <= 0).double()[:, None, :]).abs()            # [b, i, j] = |tau_i - 1{d_j <= 0}|
    huber, prio = (l[:, None, :] * wt).sum(-1).mean(-1), l.sum(-1)      # (1 / N) sum_i sum_j l_j = sum_j l_j
    terms = wt * d.clamp(-1.0, 1.0)[:, None, :]
    fac = (w / (B * n))[:, None]
    return dict(huber=huber, prio=prio, loss=(huber * w).sum() / B, dtheta=-fac * terms.sum(-1), d=d,
                prio_scale=prio, loss_scale=(huber * w).abs().sum() / B, dtheta_scale=fac.abs() * terms.abs().sum(-1))


def loss32(b2, act, ret, tau, weight):
    """oracle_iqn.loss_terms' float32 torch expression on the logits [B, A, N] = b2 directly, autograd
    -> prio [B], loss, d loss / d logits [B, A, N]."""
    b, n = tau.shape
    lg = b2.float().view(1, -1, 1).expand(b, -1, n).clone().requires_grad_(True)
    curr = lg[torch.arange(b), act.long(), :].unsqueeze(2)
    tgt = ret.float().unsqueeze(1)
    dist_diff = F.smooth_l1_loss(tgt.expand(-1, n, -1), curr.expand(-1, -1, ret.shape[1]), reduction="none")
    huber = (dist_diff * (tau.float().unsqueeze(2) - (tgt - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1)
    loss = (huber * weight.float()).mean()
    loss.backward()
    return dist_diff.detach().abs().sum(-1).mean(1), loss.detach(), lg.grad


def scatter_actions(rows: torch.Tensor, act: torch.Tensor, a: int) -> torch.Tensor:
    """Per-sample values [B] of the taken actions -> summed per action [A]."""
    out = torch.zeros(a, dtype=rows.dtype)
    out.index_add_(0, act.long(), rows)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def make_case(a: int, n: int, np_: int, b2: torch.Tensor, ret: torch.Tensor, tau: torch.Tensor, act, weight=None,
              seed: int = 0) -> dict:
    b = tau.shape[0]
    assert tuple(ret.shape) == (b, np_) and tuple(tau.shape) == (b, n) and b2.numel() == a
    act = torch.as_tensor(act, dtype=torch.int64)
    assert int(act.min()) >= 0 and int(act.max()) < a                       # the kernels are never fed an action outside [0, A)
    assert float(tau.min()) >= 0.0 and float(tau.max()) < 1.0
    return dict(A=a, N=n, Np=np_, B=b, b2=b2.float(), ret=ret.float(), tau=tau.float(), act=act, weight=weight, obs=obs_batch(b, seed))


def edge_fractions(b: int, n: int, g) -> torch.Tensor:
    """Uniform fractions with tau = 0 first and tau one ulp below 1 last in every row."""
    tau = torch.rand(b, n, generator=g)
    tau[:, 0], tau[:, -1] = 0.0, BELOW_ONE
    return tau


LINEAR_SHAPES = [(2, 2), (7, 2), (5, 64), (64, 64), (2, 64)]               # (N, N'), N <= 7 N' - 3 (module docstring)


def linear_case(sign: float, n: int, np_: int) -> dict:
    """sign = +1: every T_j >= theta + 1 (under-estimates); -1: every T_j <= theta - 1.  A = 5, one sample per action:
    sample 0 just beyond |d| = 1 (1.5 .. 4.5), samples 1 and 2 at returns ~1e4, sample 3 with every tau = 0."""
    a, b = 5, 4
    g = _rng(31 + 100 * n + np_ + (7 if sign < 0 else 0))
    b2 = head_bias(a, n, 17)
    act = torch.tensor([0, 1, 2, 4])
    theta = b2[act]
    ret = torch.empty(b, np_)
    ret[0] = theta[0] + sign * (1.5 + 3.0 * torch.rand(np_, generator=g))
    ret[1:3] = sign * (1e4 + 50.0 * torch.randn(2, np_, generator=g))
    ret[3] = theta[3] + sign * (2.0 + torch.rand(np_, generator=g))
    tau = edge_fractions(b, n, g)
    tau[3] = 0.0
    return make_case(a, n, np_, b2, ret, tau, act, weight=f32([1.0, 0.5, 2.0, 0.25]), seed=1)


def linear_closed_form(case: dict, sign: float):
    """-> (gbias [A], size [A]): sum over the rows of -w_b N' tau_i / (B N)  (sign > 0) or +w_b N' (1 - tau_i) / (B N)."""
    tau, w = case["tau"].double(), case["weight"].double()
    fac = (w * case["Np"] / (case["B"] * case["N"]))[:, None]
    rows = -fac * tau if sign > 0 else fac * (1.0 - tau)
    return scatter_actions(rows.sum(-1), case["act"], case["A"]), scatter_actions(rows.abs().sum(-1), case["act"], case["A"])


UNIT_EDGES = tuple(x for c in (1.0, -1.0) for x in (c, nextafter32(c, 0.0), nextafter32(c, 9.0 * c)))


def unit_case() -> dict:
    """theta == 0 (an integer) in the taken action, so d_j = T_j - theta == T_j exactly: the returns cycle through +1, -1 and
    the float32 neighbours of both, one ulp inward and outward (UNIT_EDGES)."""
    a, n, np_, b = 3, 5, 7, 6
    ret = f32([[UNIT_EDGES[(j + r) % 6] for j in range(np_)] for r in range(b)])
    return make_case(a, n, np_, f32([0.0, 1.5, -2.0]), ret, edge_fractions(b, n, _rng(41)), torch.zeros(b, dtype=torch.int64),
                     weight=f32([1.0, 0.5, 2.0, 0.25, 1.5, 1.0]), seed=2)


MIXED_SHAPES = [(1, 2, 2), (64, 64, 64), (33, 5, 64), (3, 64, 2)]           # (A, N, N')
MIXED_WEIGHT = (0.0, 1.0, 0.5, 0.0, 2.0)                                    # rows 0 and 3 have weight 0


def mixed_case(a: int, n: int, np_: int, weighted: bool) -> dict:
    """T_j = theta + 2.5 N(0, 1): both sides of theta, |d| below and above 1.  B = 5; with A >= 5 every sample has its own
    action, with A = 3 action 0 belongs to row 0 alone (a zero-weight row when `weighted`)."""
    b = 5
    g = _rng(51 + 1000 * a + 10 * n + np_)
    b2 = head_bias(a, n, 19 + a)
    act = torch.tensor([0, a - 1, a // 2, 1, a - 2]) if a >= 5 else torch.tensor([0, 2, 1, 1, 2]) if a == 3 else torch.zeros(b, dtype=torch.int64)
    ret = b2[act][:, None] + 2.5 * torch.randn(b, np_, generator=g)
    return make_case(a, n, np_, b2, ret, edge_fractions(b, n, g), act, weight=f32(MIXED_WEIGHT) if weighted else None, seed=3)


def mean_case(b: int) -> dict:
    """N = N' = 2, A = 3: B = 1, and B = 1030 = one more trip through iqn_mean_kernel's 1024-stride loop for six threads."""
    a, n = 3, 2
    g = _rng(61 + b)
    b2 = head_bias(a, n, 23)
    act = torch.randint(0, a, (b,), generator=g)
    ret = b2[act][:, None] + 2.5 * torch.randn(b, n, generator=g)
    return make_case(a, n, n, b2, ret, torch.rand(b, n, generator=g), act, weight=torch.rand(b, generator=g) + 0.25, seed=4)


def reference(case: dict) -> dict:
    """float64 values, err32 of the float32 oracle formula and the bars of one update on an edge network: prio [B], loss,
    gbias [A] (the bias-row gradient)."""
    a, b = case["A"], case["B"]
    w = torch.ones(b) if case["weight"] is None else case["weight"].float()
    r = iqn_loss64(case["b2"][case["act"]], case["ret"], case["tau"], w)
    prio32, l32, g32 = loss32(case["b2"], case["act"], case["ret"], case["tau"], w)
    out = dict(prio=r["prio"], prio_scale=r["prio_scale"], loss=r["loss"], loss_scale=r["loss_scale"], d=r["d"], dtheta=r["dtheta"],
               gbias=scatter_actions(r["dtheta"].sum(-1), case["act"], a),
               gbias_scale=scatter_actions(r["dtheta_scale"].sum(-1), case["act"], a), grad32=g32)
    out["prio_err32"], out["loss_err32"] = (prio32.double() - out["prio"]).abs(), (l32.double() - out["loss"]).abs()
    out["gbias_err32"] = (g32.sum((0, 2)).double() - out["gbias"]).abs()
    for k in ("prio", "loss", "gbias"):
        out[k + "_bar"] = bar(out[k + "_err32"], out[k + "_scale"])
    return out


def err32_units(ref: dict) -> dict:
    """Largest err32 / (eps32 * scale) per quantity: the figures of this module's docstring."""
    return {k: float((ref[k + "_err32"] / (EPS32 * torch.as_tensor(ref[k + "_scale"]).clamp_min(1e-300))).max())
            for k in ("prio", "loss", "gbias")}


# ---- part B: the cosine embedding ----------------------------------------------------------------------------------------------
def fractions_off_the_kink(p, rng, B, N, margin=2e-6):
    """Fractions for a GRADIENT comparison.  d relu / d x jumps at 0, so an embedding pre-activation whose sign the
    reference's own float32 rounding decides has no reference gradient: a 64-term float32 dot product of terms of size
    <= 0.4 carries an error of up to 64 * 2^-24 * 0.4 = 1.5e-6, and both signs are legitimate results inside that band
    (seen: float32 +4.5e-8 where float64 gives -1.8e-8; about 2 of 10^6 elements fall inside the band).  Rows whose
    float64 pre-activations come closer to 0 than `margin` are redrawn; the rule looks at the reference only."""
    K = p["emb.w"].shape[1]
    i_pi = np.pi * torch.arange(1, K + 1, dtype=torch.float32)
    tau = torch.as_tensor(rng.random((B, N), dtype=np.float32))
    for _ in range(100):
        cosv = torch.cos(tau.view(B * N, 1) * i_pi.view(1, K)).double()
        pre = torch.nn.functional.linear(cosv, p["emb.w"].double(), p["emb.b"].double())
        close = (pre.abs() < margin).any(dim=1).view(B, N)
        if not close.any():
            return tau
        tau[close] = torch.as_tensor(rng.random(int(close.sum()), dtype=np.float32))
    raise AssertionError("no fractions off the ReLU kink found")


def cos64(tau: torch.Tensor, k: int = 64) -> torch.Tensor:
    """[B, N] -> cos of the float32 arguments fl32(tau * fl32(fl32(pi) * (i + 1))), in float64: [B N, k]."""
    i_pi = np.pi * torch.arange(1, k + 1, dtype=torch.float32)             # the python scalar is rounded to float32 first
    arg = tau.float().reshape(-1, 1) * i_pi.view(1, k)                      # float32 product, rounded
    return torch.cos(arg.double())


def embed_mul64(tau, feat, we, be) -> torch.Tensor:
    """x[b N + n, :] = feat[b, :] * relu(cos(.) @ We^T + be), float64; we [F, K], be [F] in the reference's layout."""
    n = tau.shape[1]
    phi = torch.relu(cos64(tau, we.shape[1]) @ we.double().t() + be.double())
    return feat.double().repeat_interleave(n, dim=0) * phi


def embed_mul_bwd64(tau, feat, we, be, dx):
    """-> (dfeat [B, F] masked by feat > 0, dWe [K, F], dbe [F]) of embed_mul64 for the upstream gradient dx [B N, F]."""
    b, n = tau.shape
    cosv = cos64(tau, we.shape[1])
    pre = cosv @ we.double().t() + be.double()
    f64 = feat.double()
    dfeat = (dx.double() * torch.relu(pre)).view(b, n, -1).sum(1) * (f64 > 0)
    dphi = dx.double() * f64.repeat_interleave(n, dim=0) * (pre > 0)
    return dfeat, cosv.t() @ dphi, dphi.sum(0)


def embed_mul32(tau, feat, we, be) -> torch.Tensor:
    """The float32 torch expression (oracle_iqn.embed)."""
    b, n = tau.shape
    return (feat.unsqueeze(1) * OI.embed({"emb.w": we, "emb.b": be}, tau)).view(b * n, -1)


def embed_mul_bwd32(tau, feat, we, be, dx):
    f_, w_, b_ = (t.detach().clone().requires_grad_(True) for t in (feat, we, be))
    embed_mul32(tau, f_, w_, b_).backward(dx)
    return f_.grad * (feat > 0), w_.grad.t().contiguous(), b_.grad


FWD_SHAPES = [(157, 7, 64), (157, 7, 192), (20, 64, 128), (1200, 1, 64)]    # (B, N, F)
BWD_SHAPES = [(157, 7, 64), (20, 64, 128), (19, 33, 64), (600, 1, 128)]
BOUNDARY_FUSED, BOUNDARY_UNFUSED = (256, 64, 64), (5461, 3, 64)              # R = 16384 and 16383


def fwd_tiles(b: int, n: int):
    """-> (row tiles, shares) of iqn_embed_fwd_kernel."""
    tiles = (b * n + BM - 1) // BM
    return tiles, min(tiles, FWD_SHARES)


def bwd_tiles(b: int, n: int):
    """-> (row tiles of whole samples, shares, samples per tile) of iqn_embed_bwd_kernel."""
    sb = BM // n
    tiles = (b + sb - 1) // sb
    return tiles, min(tiles, BWD_SLABS), sb


@functools.lru_cache(maxsize=None)
def embed_inputs(b: int, n: int, f: int, off_kink: bool) -> dict:
    """tau [B, N], feat [B, F] (a ReLU output), we [F, 64], be [F], dx [B N, F].  Forward inputs hold tau = 0 and tau one ulp
    below 1 in the last rows (the partial last tile); gradient inputs are drawn off the ReLU kink."""
    k = 64
    g = _rng(7 + b + 100 * n + f)
    feat = torch.relu(torch.randn((b, f), generator=g))
    we, be = torch.randn((f, k), generator=g) * 0.2, torch.randn(f, generator=g) * 0.1
    dx = torch.randn((b * n, f), generator=g)
    if off_kink:
        tau = fractions_off_the_kink({"emb.w": we, "emb.b": be}, np.random.default_rng(b + n + f), b, n)
    else:
        tau = torch.rand((b, n), generator=g)
        tau.view(-1)[-1], tau.view(-1)[-3], tau.view(-1)[0] = 0.0, BELOW_ONE, 0.0
    return dict(tau=tau, feat=feat, we=we, be=be, dx=dx, we_be=torch.cat([we.t(), be.view(1, f)]).contiguous())


@functools.lru_cache(maxsize=None)
def embed_reference(b: int, n: int, f: int, off_kink: bool) -> dict:
    """float64 yardsticks of `embed_inputs` and the float32 expression's own rel_err against them (e_x; e_dfeat, e_dwe, e_dbe
    for gradient inputs)."""
    d = embed_inputs(b, n, f, off_kink)
    args = (d["tau"], d["feat"], d["we"], d["be"])
    x = embed_mul64(*args)
    out = dict(x=x, e_x=rel_err(embed_mul32(*args), x))
    if off_kink:
        out["dfeat"], out["dwe"], out["dbe"] = embed_mul_bwd64(*args, d["dx"])
        for k, v in zip(("dfeat", "dwe", "dbe"), embed_mul_bwd32(*args, d["dx"])):
            out["e_" + k] = rel_err(v, out[k])
    return out


# ---- part B: the whole network on the fused default route ----------------------------------------------------------------------
def layout_offsets(a: int, c: int = C, f: int = FEAT) -> np.ndarray:
    """Starts of conv1, conv2, conv3, embedding, fc1, fc2 and the end in the flat vector (tianshou_amd.iqn.layout()['off'])."""
    sizes = [(64 * c + 1) * 32, 513 * 64, 577 * 64, 65 * f, (f + 1) * 512, 513 * head_ld(a)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def grad_parts(a: int, c: int = C, f: int = FEAT) -> dict:
    """The `parts` split of test_batch_gradient_vs_oracle."""
    off, ld = layout_offsets(a, c, f), head_ld(a)
    return {"conv1": (off[0], off[1]), "conv2": (off[1], off[2]), "conv3": (off[2], off[3]),
            "We": (off[3], off[3] + 64 * f), "be": (off[3] + 64 * f, off[4]),
            "W1": (off[4], off[4] + f * 512), "b1": (off[4] + f * 512, off[5]),
            "W2": (off[5], off[5] + 512 * ld), "b2": (off[5] + 512 * ld, off[6])}


def flat_grads(grads: dict, a: int) -> torch.Tensor:
    """Reference-layout gradients -> the engine's flat layout (tianshou_amd.iqn.flat_from_torch is plain torch on the host)."""
    from tianshou_amd import iqn as I

    return I.flat_from_torch([grads[k] for k in OI.PARAM_ORDER], C, H, W, a, device="cpu")


def logits64(p: dict, obs, tau: torch.Tensor) -> torch.Tensor:
    """oracle_iqn.logits in float64 (cosine arguments formed in float32) -> [B, A, N]; p holds float64 tensors."""
    x = torch.as_tensor(np.asarray(obs)).double()
    for name, stride in (("conv1", 4), ("conv2", 2), ("conv3", 1)):
        x = F.relu(F.conv2d(x, p[name + ".w"], p[name + ".b"], stride=stride))
    feat = x.flatten(1)
    b, n = tau.shape
    phi = F.relu(F.linear(cos64(tau, p["emb.w"].shape[1]), p["emb.w"], p["emb.b"]))
    xr = feat.repeat_interleave(n, dim=0) * phi
    out = F.linear(F.relu(F.linear(xr, p["fc1.w"], p["fc1.b"])), p["fc2.w"], p["fc2.b"])
    return out.view(b, n, -1).transpose(1, 2)


def net_loss64(p32: dict, obs, act, ret, tau, weight=None):
    """float64 restatement of oracle_iqn.loss_terms + backward -> (loss, prio [B], logits [B, A, N], grads in reference layout)."""
    p = {k: v.double().clone().requires_grad_(True) for k, v in p32.items()}
    lg = logits64(p, obs, tau)
    b, n = tau.shape
    theta = lg[torch.arange(b), torch.as_tensor(act).long(), :]            # [B, N]
    d = torch.as_tensor(ret).double()[:, None, :] - theta[:, :, None]       # [b, i, j]
    ad = d.abs()
    l = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    wt = (tau.double()[:, :, None] - (d.detach() <= 0).double()).abs()
    huber = (l * wt).sum(-1).mean(1)
    w = torch.ones(b, dtype=torch.float64) if weight is None else torch.as_tensor(weight).double()
    loss = (huber * w).mean()
    loss.backward()
    return loss.detach(), l.detach().sum(-1).mean(1), lg.detach(), {k: v.grad for k, v in p.items()}


ENGINE_UPDATE = dict(A=3, B=257, N=64, Np=2, seed=6)                        # R = 16448 >= 2^14: the fused default route
ENGINE_FORWARD = dict(A=3, B=512, N=32, seed=8)                             # R = 16384: the evaluation shape over 512 environments


@functools.lru_cache(maxsize=None)
def engine_update_case() -> dict:
    """One weighted minibatch at ENGINE_UPDATE on a random-weight network; float64 loss / prio / flat gradient, and the float32
    oracle's (oracle_iqn.update_with_batch) own rel_err per part."""
    s = ENGINE_UPDATE
    a, b, n, np_ = s["A"], s["B"], s["N"], s["Np"]
    rng = np.random.default_rng(s["seed"])
    p = OI.init_params(C, H, W, a, seed=s["seed"])
    obs = rng.integers(0, 256, size=(b, C, H, W), dtype=np.uint8)
    act = rng.integers(0, a, size=b)
    ret = (rng.normal(size=(b, np_)) * 2.5).astype(np.float32)
    tau = fractions_off_the_kink(p, rng, b, n)
    weight = rng.random(b).astype(np.float32)
    loss, prio, lg, grads = net_loss64(p, obs, act, ret, tau, weight)
    ocfg = OI.IQNConfig()
    col: dict = {}
    loss32_, prio32 = OI.update_with_batch(OD.DQNState.create({k: v.clone() for k, v in p.items()}, ocfg.dqn()), ocfg, obs, act, ret,
                                           tau, weight=weight, collect=col)
    g64, g32 = flat_grads(grads, a), flat_grads(col["grads"], a)
    parts = grad_parts(a)
    e_ref = {k: rel_err(g32[lo:hi], g64[lo:hi]) for k, (lo, hi) in parts.items()}
    e_ref.update(loss=abs(loss32_ - float(loss)) / abs(float(loss)), prio=rel_err(prio32, prio))
    return dict(p=p, obs=obs, act=act, ret=ret, tau=tau, weight=weight, loss=float(loss), prio=prio, logits=lg, grad=g64, parts=parts,
                e_ref=e_ref, d=(torch.as_tensor(ret).double()[:, None, :] - lg[torch.arange(b), torch.as_tensor(act), :][:, :, None]))


@functools.lru_cache(maxsize=None)
def engine_forward_case() -> dict:
    """`forward` at ENGINE_FORWARD: float64 logits / Q / act, the float32 oracle's own rel_err, and the rows whose float64 gap
    between the two largest Q is beyond float32 blur: gap > 2 * (the Q bar), so two sets of Q inside the bar cannot disagree."""
    s = ENGINE_FORWARD
    a, b, n = s["A"], s["B"], s["N"]
    rng = np.random.default_rng(s["seed"])
    p = OI.init_params(C, H, W, a, seed=s["seed"])
    obs = rng.integers(0, 256, size=(b, C, H, W), dtype=np.uint8)
    tau = torch.as_tensor(rng.random((b, n), dtype=np.float32))
    with torch.no_grad():
        lg = logits64({k: v.double() for k, v in p.items()}, obs, tau)
        lg32, q32, act32 = OI.policy_forward(p, obs, tau)
    q = lg.mean(2)
    e_ref = dict(logits=rel_err(lg32, lg), q=rel_err(q32, q))
    top2 = torch.topk(q, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2.0 * rel_bar(e_ref["q"]) * float(q.abs().max())
    return dict(p=p, obs=obs, tau=tau, logits=lg, q=q, act=q.argmax(dim=1), act32=act32, e_ref=e_ref, clear=clear)
