"""Inputs and float64 / float32 references for the recurrent Q engine (ts_rnnq.hip) where tests/test_gpu_drqn.py never goes:
long sequences, B = 1 and batch sizes on the 16-row tile edge, carried state, gates saturated through their bias rows, and a
head whose Q values are exact.  Shared by tests/test_drqn_edge_inputs_cpu.py and tests/test_gpu_drqn_edges.py: BOTH iterate
PARITY_CASES / HUBER_DELTAS / TIES below, so no case reaches the GPU test without its CPU precondition.  Nothing here touches
the GPU path or imports the product.

References.  `reference64(case)` is oracle/oracle_drqn.py::forward in float64 (parameters, observations, state) with the loss of
oracle_drqn.update_with_batch and autograd gradients; `reference32(case)` the same expressions in float32.

Bars (the project's existing ones, no new numbers):
    q, td, h_T, c_T (per tensor)    max|x - ref64| <= 1e-5 max(1, max|ref64|)       tests/test_gpu_drqn.py's rtol = atol = 1e-5 on
                                                                                   the tensor's scale (test_gpu_iqn.py::rel_err)
    loss                            |x - ref64| <= 1e-5 max(1, |ref64|)            tests/test_gpu_drqn.py
    gradients (per parameter block) |g - ref64| <= 1e-4 |ref64| + 2e-5 max|ref64 of the block|
                                                                                   tests/test_gpu_recurrent_nets.py::_close_blocks
Precondition of every parity case: the float32 ORACLE sits within QUARTER = 0.25 of each bar (asserted on the CPU).  That is a
condition on the inputs: it keeps chaotic / ill-conditioned networks out, on which float32 has no answer and a failure would say
nothing about a kernel.  Measured ratios |oracle32 - ref64| / bar (tests/test_drqn_edge_inputs_cpu.py prints them with -s):

    case                                 q      h      c      td     loss   grad
    grid H128 L2 B17 T64                 0.017  0.046  0.030  0.003  0.005  0.035
    grid H128 L2 B16 T64                 0.012  0.076  0.037  0.003  0.007  0.023
    grid H128 L2 B17 T2                  0.010  0.040  0.046  0.003  0.003  0.021
    grid H32 L3 B17 T64                  0.007  0.034  0.029  0.004  0.008  0.015
    grid H32 L1 B1 T256                  0.005  0.009  0.007  0.011  0.017  0.008
    grid H64 L1 B15 T64                  0.031  0.041  0.017  0.003  0.009  0.020
    grid H96 L2 B17 T17 (per-step)       0.009  0.024  0.024  0.002  0.010  0.020
    the B = 1 grid cases                 <= 0.02 everywhere
    forget +3, H128 L1 B17 T32           0.039  0.109  0.028  0.010  0.001  0.029
    gain 1 forget +4, H64 L1 B17 T64     0.018  0.069  0.041  0.007  0.003  0.077
    forget -30, H64 L2 B17 T16           0.007  0.017  0.036  0.003  0.003  0.016
    o +110 g +-60, H64 L2 B17 T16        0.003  0.011  0.017  0.002  0.006  0.020
    o / i -110 (ZERO_CASES)              0.000  0.000  0.003  0.005  0.012  0.002 (fc2.bias; the other blocks are exactly 0)
Rejected by the precondition and therefore absent: forget bias +3 at L = 2, T = 64 (h 0.42 - 0.63), all four gate biases +20
(h 1.9), weight gain 8 (q 2.4).  The networks of the -110 / +110 / +-60 cases use gain 0.5 and observations scaled by 0.25 so
that the bias rows alone decide the gate (gate_margin > 100, > 50 for tanh)."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_drqn as ORQ

QUARTER = 0.25
OUT_TOL = 1e-5                          # q, td, h_T, c_T, loss
GRAD_RTOL, GRAD_ATOL = 1e-4, 2e-5       # gradient blocks
HEAD = 32
PATHS = ("layer_kernels", "per_step")


def f32(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def nextafter32(x: float, toward: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(toward)))


# ---- networks ----------------------------------------------------------------------------------------------------------------
def rand_params(obs_dim, hidden, layers, n_act, seed, gate_bias=None, gain: float = 2.0):
    """U(-gain / sqrt(fan_in), gain / sqrt(fan_in)) for every tensor, in Recurrent.state_dict() order.  `gate_bias`: offsets
    (i, f, g, o) added to nn.bias_ih_l* of every layer, each a number or a tensor [hidden]."""
    g = torch.Generator().manual_seed(seed)
    shapes = ORQ.param_shapes(obs_dim, hidden, layers, n_act)
    p = {}
    for k in ORQ.param_keys(layers):
        bound = 1.0 / np.sqrt(hidden if k.startswith("nn.") or k.startswith("fc2") else obs_dim)
        p[k] = (torch.rand(shapes[k], generator=g) * 2 - 1) * (gain * bound)
    if gate_bias is not None:
        off = torch.cat([torch.as_tensor(b, dtype=torch.float32).expand(hidden) for b in gate_bias])
        for l in range(layers):
            p[f"nn.bias_ih_l{l}"] = p[f"nn.bias_ih_l{l}"] + off
    return p


def edge_params(rows, obs_dim: int = 4, hidden: int = 32, layers: int = 1, seed: int = 1, **kw) -> dict:
    """Any trunk under a head of zero weights and bias `rows` [A]: Q[b, :] == rows for every b, exactly (a sum of H exact
    zeros plus the bias), and nothing flows below the head."""
    rows = torch.as_tensor(rows, dtype=torch.float32).reshape(-1)
    p = rand_params(obs_dim, hidden, layers, rows.numel(), seed, **kw)
    p["fc2.weight"] = torch.zeros_like(p["fc2.weight"])
    p["fc2.bias"] = rows.clone()
    return p


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _alternating(h: int, v: float) -> torch.Tensor:
    return torch.tensor([v if j % 2 == 0 else -v for j in range(h)])


def make_case(name, H, L, B, T, obs_dim=4, A=2, gain=2.0, gate_bias=None, huber=None, weighted=False, paths=PATHS, seed=1,
              obs_scale=1.0, rows=None, zero=False) -> dict:
    return dict(name=name, H=H, L=L, B=B, T=T, obs_dim=obs_dim, A=A, gain=gain, gate_bias=gate_bias, huber=huber,
                weighted=weighted, paths=tuple(paths), seed=seed, obs_scale=obs_scale, rows=rows, zero=zero)


def _grid():
    for B in (1, 16, 17):
        yield make_case(f"grid H32 L3 B{B} T64", 32, 3, B, 64, obs_dim=33, A=5, huber=1.0 if B == 16 else None, weighted=B == 17)
    yield make_case("grid H32 L1 B1 T256", 32, 1, 1, 256, obs_dim=4, A=1)
    for B in (1, 15, 17):
        yield make_case(f"grid H64 L1 B{B} T64", 64, 1, B, 64, obs_dim=32, A=32, huber=2.5 if B == 15 else None, weighted=B == 17)
    for B in (1, 16, 17):
        yield make_case(f"grid H128 L2 B{B} T64", 128, 2, B, 64, obs_dim=4, A=2, huber=1.0 if B == 17 else None, weighted=B == 16)
    yield make_case("grid H128 L2 B17 T2", 128, 2, 17, 2, obs_dim=33, A=5, weighted=True)
    yield make_case("grid H96 L2 B17 T17", 96, 2, 17, 17, obs_dim=4, A=2, huber=1.0, paths=("per_step",))


GRID_CASES = list(_grid())
# gates saturated or integrating through bias rows (never through weight gain) that still meet the parity precondition
SATURATED_PARITY_CASES = [
    make_case("forget +3 H128 L1 B17 T32", 128, 1, 17, 32, gate_bias=(0.0, 3.0, 0.0, 0.0), weighted=True),
    make_case("gain 1 forget +4 H64 L1 B17 T64", 64, 1, 17, 64, gain=1.0, gate_bias=(0.0, 4.0, 0.0, 0.0), huber=1.0),
    make_case("forget -30 H64 L2 B17 T16", 64, 2, 17, 16, gate_bias=(0.0, -30.0, 0.0, 0.0), weighted=True),
    make_case("o +110 g +-60 H64 L2 B17 T16", 64, 2, 17, 16, gain=0.5, gate_bias=(0.0, 0.0, _alternating(64, 60.0), 110.0),
              obs_scale=0.25, weighted=True),
]
# exact zeros: h == 0 (and c == 0 for the i gate) at every layer and step
_SMALL = dict(gain=0.5, obs_scale=0.25, zero=True)
ZERO_CASES = [
    make_case("o -110 H64 L2 B17 T16", 64, 2, 17, 16, gate_bias=(0.0, 0.0, 0.0, -110.0), A=5, **_SMALL),
    make_case("i -110 H128 L2 B17 T16", 128, 2, 17, 16, gate_bias=(-110.0, 0.0, 0.0, 0.0), A=5, **_SMALL),
    make_case("o -110 H32 L3 B1 T16", 32, 3, 1, 16, gate_bias=(0.0, 0.0, 0.0, -110.0), A=5, huber=1.0, **_SMALL),
]
PARITY_CASES = GRID_CASES + SATURATED_PARITY_CASES + ZERO_CASES
CASES = {c["name"]: c for c in PARITY_CASES}
assert len(CASES) == len(PARITY_CASES)

# carried state: (case, T1) -- forward(obs[:, :T1]) then forward(obs[:, T1:], state) against one pass
CARRIED = [(f"grid H{H} L{L} B{B} T64", T1) for H, L in ((32, 3), (128, 2)) for B in (1, 17) for T1 in (1, 32, 63)]
CARRIED_STEPS = ["grid H32 L3 B1 T64", "grid H128 L2 B1 T64"]        # 64 evaluation-mode steps of B = 1, T = 1


@functools.lru_cache(maxsize=None)
def _built(name: str):
    c = CASES[name]
    p = (rand_params(c["obs_dim"], c["H"], c["L"], c["A"], c["seed"], c["gate_bias"], c["gain"]) if c["rows"] is None else
         edge_params(c["rows"], c["obs_dim"], c["H"], c["L"], c["seed"], gate_bias=c["gate_bias"], gain=c["gain"]))
    g = torch.Generator().manual_seed(1000 + c["B"] + c["T"])
    obs = torch.randn(c["B"], c["T"], c["obs_dim"], generator=g) * c["obs_scale"]
    act = torch.randint(0, c["A"], (c["B"],), generator=g)
    ret = torch.randn(c["B"], generator=g) * 2
    w = torch.rand(c["B"], generator=g) + 0.5 if c["weighted"] else None
    return dict(p=p, obs=obs, act=act, ret=ret, weight=w)


def inputs(case: dict) -> dict:
    """params `p` (float32, state_dict keys), obs [B, T, obs_dim], act [B], ret [B], weight [B] or None.  Built once per case;
    callers must not modify the tensors."""
    return _built(case["name"])


# ---- references --------------------------------------------------------------------------------------------------------------
def reference(p: dict, obs, act, ret, weight, huber, dtype, state=None) -> dict:
    """The oracle formulas (oracle_drqn.forward + the loss of oracle_drqn.update_with_batch) in `dtype`, autograd gradients
    -> q [B, A], h / c [L, B, H], td [B], loss, grads {key: tensor}."""
    layers = ORQ.n_layers(p)
    pp = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    if state is not None:
        state = tuple(s.to(dtype) for s in state)
    q_all, (h, c) = ORQ.forward(pp, obs.to(dtype), state=state, want_state=True, dtype=dtype)
    q = q_all[torch.arange(len(act)), act]
    r = ret.to(dtype)
    td = r - q
    if huber is not None:
        loss = F.huber_loss(q.reshape(-1, 1), r.reshape(-1, 1), delta=huber, reduction="mean")
    else:
        loss = (td.pow(2) * (1.0 if weight is None else weight.to(dtype))).mean()
    loss.backward()
    return dict(q=q_all.detach(), h=h.detach(), c=c.detach(), td=td.detach(), loss=loss.detach(),
                grads={k: pp[k].grad.detach() for k in ORQ.param_keys(layers)})


@functools.lru_cache(maxsize=None)
def _ref(name: str, dtype):
    c, i = CASES[name], _built(name)
    return reference(i["p"], i["obs"], i["act"], i["ret"], i["weight"], c["huber"], dtype)


def reference64(case: dict) -> dict:
    return _ref(case["name"], torch.float64)


def reference32(case: dict) -> dict:
    return _ref(case["name"], torch.float32)


def out_bar(ref64: torch.Tensor) -> torch.Tensor:
    return torch.full_like(ref64, OUT_TOL * max(1.0, float(ref64.abs().max())))


def grad_bar(ref64: torch.Tensor) -> torch.Tensor:
    return GRAD_RTOL * ref64.abs() + GRAD_ATOL * float(ref64.abs().max())


def outputs_of(r: dict, zero: bool = False) -> dict:
    """Flat {quantity: tensor}: q, td, loss, h0.., c0.. (one per layer), grad:<key>.  `zero` (ZERO_CASES): of the gradients
    only fc2.bias -- every other block is asserted to be exactly 0.0, where float64 holds sigmoid(-110) = 2e-48."""
    out = dict(q=r["q"], td=r["td"], loss=r["loss"])
    for l in range(r["h"].shape[0]):
        out[f"h{l}"], out[f"c{l}"] = r["h"][l], r["c"][l]
    for k, g in r.get("grads", {}).items():
        if not zero or k == "fc2.bias":
            out["grad:" + k] = g
    return out


def bars_of(ref64: dict, zero: bool = False) -> dict:
    """{quantity: (ref64 tensor, bar tensor)} over outputs_of(ref64)."""
    return {k: (v, grad_bar(v) if k.startswith("grad:") else out_bar(v)) for k, v in outputs_of(ref64, zero).items()}


def ratios(got: dict, ref64: dict, zero: bool = False) -> dict:
    """Largest |got - ref64| / bar per quantity family (q, h, c, td, loss, grad); a zero bar counts inf unless got == ref64."""
    res: dict = {}
    g = outputs_of(got)
    for k, (ref, bar) in bars_of(ref64, zero).items():
        err = (g[k].double().reshape(ref.shape) - ref).abs()
        ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
        fam = "grad" if k.startswith("grad:") else k.rstrip("0123456789")
        res[fam] = max(res.get(fam, 0.0), float(ratio.max()))
    return res


def gate_margin(case: dict, gate: int) -> float:
    """Lower bound of |pre-activation| of gate `gate` (0..3 = i, f, g, o) over every layer, unit, row and step:
    |offset| - (sum|W_ih row| max|x| + sum|W_hh row| + |b_ih - offset| + |b_hh|), with max|x| = the largest |fc1 output| for
    layer 0 and 1 (|h| <= 1) above."""
    i, H = inputs(case), case["H"]
    p = i["p"]
    off = torch.as_tensor(case["gate_bias"][gate], dtype=torch.float32).expand(H).double()
    x_max = float(F.linear(i["obs"].double(), p["fc1.weight"].double(), p["fc1.bias"].double()).abs().max())
    sl = slice(gate * H, (gate + 1) * H)
    worst = float("inf")
    for l in range(case["L"]):
        w_ih, w_hh = p[f"nn.weight_ih_l{l}"].double()[sl], p[f"nn.weight_hh_l{l}"].double()[sl]
        b_ih, b_hh = p[f"nn.bias_ih_l{l}"].double()[sl], p[f"nn.bias_hh_l{l}"].double()[sl]
        rest = w_ih.abs().sum(1) * (x_max if l == 0 else 1.0) + w_hh.abs().sum(1) + (b_ih - off).abs() + b_hh.abs()
        worst = min(worst, float((off.abs() - rest).min()))
    return worst


# ---- head cases: exact Q through edge_params ---------------------------------------------------------------------------------
TIES = [(4, (0, 2)), (5, (3, 4)), (6, (1, 3, 4)), (5, (4,)), (32, (30, 31)), (1, (0,))]


def tie_rows(a: int, tied: tuple, negative: bool) -> torch.Tensor:
    """Q row [A]: the tied actions share the maximum 9.5, the others are distinct and lower; `negative`: everything - 20."""
    rows = torch.tensor([1.0 + 0.25 * ((7 * i) % a) for i in range(a)]) if a > 1 else torch.tensor([1.0])
    rows = rows - 0.125 * torch.arange(a) / max(a, 1)
    rows[list(tied)] = 9.5
    return (rows - (20.0 if negative else 0.0)).float()


def lagged_rows(a: int, tied: tuple) -> torch.Tensor:
    """Distinct Q row [A] of the lagged network whose maximum is NOT at the online network's lowest tied index (A > 1)."""
    rows = torch.tensor([0.5 * i - 3.0 for i in range(a)])
    if a > 1 and int(rows.argmax()) == tied[0]:
        rows = rows.flip(0)
    return rows.float()


HUBER_DELTAS = (0.5, 1.0, 2.5)
Q_EDGE = 2.0 ** -10


def huber_case(delta: float) -> dict:
    """A = 3, Q row (-2^-10, +2^-10, 3): t = ret - q takes exactly 0, +-delta and the float32 neighbours of +-delta inward and
    outward.  Positive t are taken against q = -2^-10 and negative t against q = +2^-10, so ret = q + t is a float32 and the
    subtraction is exact; action 2 is never taken."""
    t = [0.0, 0.0]
    for s in (1.0, -1.0):
        t += [s * delta, nextafter32(s * delta, 0.0), nextafter32(s * delta, s * 9.0 * delta)]
    t = np.asarray(t, dtype=np.float32)
    act = np.where(t > 0, 0, 1)
    act[0] = 0
    rows = np.asarray([-Q_EDGE, Q_EDGE, 3.0], dtype=np.float32)
    ret = (rows[act].astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    B = len(t)
    weight = f32([0.5 + 0.25 * b for b in range(B)])
    g = torch.Generator().manual_seed(int(delta * 8))
    return dict(delta=delta, t=f32(t), rows=f32(rows), act=torch.as_tensor(act, dtype=torch.int64), ret=f32(ret), B=B, A=3,
                weight=weight, obs=torch.randn(B, 3, 4, generator=g), p=edge_params(rows, 4, 32, 1))


BATCH_SIZES = (1, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def _batch_case(B: int, huber):
    """H = 32, L = 1, T = 1 on an edge network of five distinct Q values: td per row and the loss summed over B rows."""
    g = torch.Generator().manual_seed(B)
    rows = f32([0.75, -1.5, 2.25, 0.125, -0.5])
    return dict(B=B, A=5, rows=rows, p=edge_params(rows, 4, 32, 1), obs=torch.randn(B, 1, 4, generator=g),
                act=torch.randint(0, 5, (B,), generator=g), ret=torch.randn(B, generator=g) * 2,
                weight=torch.rand(B, generator=g) + 0.5, huber=huber)


def batch_case(B: int, huber=None) -> dict:
    return _batch_case(B, huber)
