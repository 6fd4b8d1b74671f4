"""TEST INFRASTRUCTURE ONLY - the edge-case tables shared by tests/test_bdqn_edge_inputs_cpu.py (the oracle against float64
autograd and hand-derived values) and tests/test_gpu_bdqn_edges.py (the kernels against the oracle).

SHAPES   networks at the sizes where the kernels change path: B in {1, 2, 63, 65, 257} (one wavefront per sample, 4 samples per
         workgroup, 32 samples per gradient slab), D in {1, 3, 4, 17, 32}, A in {1, 2, 5, 25, 33, 64} (D A crosses the 64 lanes),
         value / action hidden layer present or not in all four combinations, widths that are no multiple of 32, ReLU and tanh.
TARGETS  raw small-integer tables for ts_bdqn_target: exact ties, a strict maximum at the last action, tables that disagree on the
         argmax, end = 1 on rows with large bootstraps.  Every expected value is exact in float32.
LOSSES   raw tables for ts_bdqn_loss: acts at 0 and A - 1, out of range (clamped), w = 0 rows, td errors that cancel in the priority.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_bdqn as OB

# name, dims = (obs_dim, common, value_hidden, action_hidden, D, A, activation), B
SHAPES = [
    ("b1_d1_a1_none", (3, (10,), 0, 0, 1, 1, "relu"), 1),
    ("b2_d3_a2_value_hidden", (5, (20, 33), 20, 0, 3, 2, "relu"), 2),
    ("b63_d4_a5_action_hidden", (7, (33,), 0, 33, 4, 5, "tanh"), 63),
    ("b65_d17_a25_both", (6, (40,), 20, 33, 17, 25, "relu"), 65),
    ("b257_d32_a33_none", (4, (48,), 0, 0, 32, 33, "relu"), 257),
    ("b2_d3_a64_both_tanh", (5, (20,), 33, 20, 3, 64, "tanh"), 2),
]


def shape_case(name: str) -> dict:
    """Seeded parameters and one batch for a SHAPES entry, float64 on the CPU (cast them as needed)."""
    _, dims, b = next(s for s in SHAPES if s[0] == name)
    g = torch.Generator().manual_seed(1000 + len(name))
    d_n, a_n = dims[4], dims[5]
    act = torch.randint(0, a_n, (b, d_n), generator=g)
    act[0, 0], act[-1, -1] = 0, a_n - 1
    if b > 2:
        act[1, 0], act[2, -1] = -3, a_n + 5                                  # out of range: clamped to 0 and A - 1
    w = torch.rand(b, generator=g, dtype=torch.float64) + 0.5
    if b > 1:
        w[b // 2] = 0.0
    return dict(dims=dims, B=b, params=OB.random_params(dims, 77, torch.float64), obs=torch.randn(b, dims[0], generator=g, dtype=torch.float64),
                obs_next=torch.randn(b, dims[0], generator=g, dtype=torch.float64), act=act, ret=torch.randn(b, generator=g, dtype=torch.float64),
                rew=torch.randn(b, generator=g, dtype=torch.float64), end=torch.rand(b, generator=g) < 0.3, weight=w)


def _t(x, dtype=torch.float32):
    return torch.tensor(x, dtype=dtype)


def targets() -> list[dict]:
    """name, q_sel, q_eval [B, D, A], rew, end, gamma, want [B] -- all exact in float32 (gamma = 0.5, D in {1, 2, 4})."""
    cases = []
    # ties: two-way (index 1 and 3 -> 1), three-way (0, 2, 3 -> 0), all equal (-> 0), strict maximum at the last action
    q_sel = _t([[[1, 7, 3, 7], [5, 2, 5, 5]], [[4, 4, 4, 4], [0, 1, 2, 9]]])
    q_eval = _t([[[10, 20, 30, 40], [8, 16, 24, 32]], [[-6, 1, 2, 3], [1, 2, 3, 64]]])
    cases.append(dict(name="ties_lowest_index", q_sel=q_sel, q_eval=q_eval, rew=_t([1.0, -2.0]), end=_t([0, 0], torch.bool), gamma=0.5,
                      want=_t([1.0 + 0.5 * (20 + 8) / 2, -2.0 + 0.5 * (-6 + 64) / 2])))
    # double vs. not: the two tables disagree on the argmax; selecting with q_eval itself is the non-double rule
    a = _t([[[0, 9, 1]], [[3, 2, 1]]])
    b = _t([[[5, 1, 8]], [[1, 2, 4]]])
    cases.append(dict(name="double_online_selects", q_sel=a, q_eval=b, rew=_t([0.0, 0.0]), end=_t([0, 0], torch.bool), gamma=0.5, want=_t([0.5, 0.5])))
    cases.append(dict(name="not_double_lagged_selects", q_sel=b, q_eval=b, rew=_t([0.0, 0.0]), end=_t([0, 0], torch.bool), gamma=0.5, want=_t([4.0, 2.0])))
    # end = 1 on rows with large bootstraps: the return is the reward, bit for bit
    big = _t([[[1e30, -1e30], [3e38, 1.0], [2.0, 1e20], [0.0, 0.0]]] * 3)
    cases.append(dict(name="end_masks_large_bootstraps", q_sel=big, q_eval=big, rew=_t([0.25, -7.0, 3.0]), end=_t([1, 1, 1], torch.bool), gamma=0.5,
                      want=_t([0.25, -7.0, 3.0])))
    # one action: the argmax is 0 whatever the value
    one = _t([[[-3.0]], [[8.0]]])
    cases.append(dict(name="single_action", q_sel=one, q_eval=one, rew=_t([1.0, 1.0]), end=_t([0, 1], torch.bool), gamma=0.5, want=_t([-0.5, 1.0])))
    return cases


def losses() -> list[dict]:
    """name, q [B, D, A], act [B, D], ret [B], weight [B] or None; the expected values come from the float64 oracle."""
    g = torch.Generator().manual_seed(5)
    cases = []
    q = torch.randn(5, 3, 4, generator=g, dtype=torch.float64)
    cases.append(dict(name="acts_at_both_ends_and_clamped", q=q, act=torch.tensor([[0, 3, 0], [3, 3, 3], [-1, 4, 99], [0, 0, 0], [2, 1, -7]]),
                      ret=torch.randn(5, generator=g, dtype=torch.float64), weight=None))
    cases.append(dict(name="zero_weight_rows", q=q, act=torch.randint(0, 4, (5, 3), generator=g), ret=torch.randn(5, generator=g, dtype=torch.float64),
                      weight=torch.tensor([1.0, 0.0, 0.5, 0.0, 2.0], dtype=torch.float64)))
    # td errors that cancel in the priority: ret = 0, the selected q are +k and -k (exact) -> prio 0 with max|td| = 1000
    qc = torch.zeros(2, 2, 3, dtype=torch.float64)
    qc[0, 0, 1], qc[0, 1, 2], qc[1, 0, 0], qc[1, 1, 0] = 1000.0, -1000.0, 0.125, -0.125
    cases.append(dict(name="td_cancel_in_the_priority", q=qc, act=torch.tensor([[1, 2], [0, 0]]), ret=torch.zeros(2, dtype=torch.float64), weight=None))
    qw = torch.randn(70, 32, 64, generator=g, dtype=torch.float64)
    cases.append(dict(name="widest_table", q=qw, act=torch.randint(0, 64, (70, 32), generator=g), ret=torch.randn(70, generator=g, dtype=torch.float64),
                      weight=torch.rand(70, generator=g, dtype=torch.float64)))
    return cases


def expected_dq(q, act, ret, weight=None):
    """d loss / d q written out: -2 w[b] td[b, d] / (B D) at the (clamped) action, 0 elsewhere."""
    b, d_n, a_n = q.shape
    td = OB.td_errors(q, act, ret)
    w = torch.ones(b, dtype=q.dtype) if weight is None else weight.to(q.dtype)
    out = torch.zeros_like(q)
    out.scatter_(-1, act.clamp(0, a_n - 1).unsqueeze(-1), (-2.0 * w.unsqueeze(-1) * td / (b * d_n)).unsqueeze(-1))
    return out


def combine_params(dims, kind: str) -> dict:
    """Parameters that make the dueling combine an exact computation: every branch head has zero weights and biases
    `kind` = "equal": 2.5 for every action (adv - mean = 0, so q = v exactly); "offset": 1e4 + a (a common offset of 1e4 that the
    mean must cancel: adv - mean = a - (A - 1) / 2 exactly, every partial sum an integer below 2^24)."""
    p = OB.random_params(dims, 3, torch.float32)
    d_n, a_n, ha = dims[4], dims[5], dims[3]
    for d in range(d_n):
        key = f"branches.{d}.model.{2 if ha else 0}"
        p[key + ".weight"].zero_()
        p[key + ".bias"] = torch.full((a_n,), 2.5) if kind == "equal" else 1e4 + torch.arange(a_n, dtype=torch.float32)
    return p


def np32(x) -> np.ndarray:
    return x.detach().cpu().to(torch.float32).numpy()
