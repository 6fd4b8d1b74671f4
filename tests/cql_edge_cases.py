"""Edge inputs of the continuous-CQL loss kernels (ts_cql_loss) and their float64 reference: tests/oracle_cql.py's `cql_terms`
under autograd.  Shared by tests/test_gpu_cql_edges.py (the kernels) and tests/test_cql_edge_inputs_cpu.py (the inputs are what
they claim to be).  Every array is float32; the reference sees the same values widened to float64.

Ties are built from values that are exact in float32 AND survive the kernel's own float32 arithmetic: a calibration return ties
with a policy value whose log-probability is 0 (value = Q, no rounding), never with the random value (Q - float32(log 0.5^A)
rounds differently in float64)."""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_cql as OC

SHAPES = [(A, B, R) for A in (1, 6, 32) for B in (1, 257) for R in (1, 3, 10)]
KINDS = ("generic", "big_values", "all_equal", "calib_above", "calib_tie", "alpha_at_min", "alpha_at_max", "alpha_below", "alpha_above",
         "no_lagrange", "weight_zero")
ZERO_REP_GRAD = ("calib_above", "weight_zero")            # kinds whose d_rep is exactly zero (compared exactly)


def make(kind: str, A: int, B: int, R: int) -> dict:
    rng = np.random.default_rng(KINDS.index(kind) * 100000 + A * 1000 + B * 11 + R)
    BR = B * R
    f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    c = dict(q_data=f(rng.normal(size=(2, B))), target=f(rng.normal(size=B)), q_rand=f(rng.normal(size=(2, BR))),
             q_cur=f(rng.normal(size=(2, BR))), q_next=f(rng.normal(size=(2, BR))), logp_cur=f(rng.normal(size=BR)),
             logp_next=f(rng.normal(size=BR)), calib=f(rng.normal(size=B)), cql_log_alpha=f([0.3]))
    cfg = dict(num_repeat_actions=R, temperature=0.8, cql_weight=1.5, with_lagrange=True, lagrange_threshold=2.0, alpha_min=0.1,
               alpha_max=50.0, calibrated=True)
    if kind == "big_values":
        # +-100 at T = 0.25: exp(400) overflows float32 unless the row maximum is subtracted.  Exact values and zero
        # log-probabilities, so near-ties are exact ties; the random value (Q - log 0.5^A = Q + 0.69 A) never ties with the others
        cfg.update(temperature=0.25)
        sign = lambda n: f(np.where(rng.random(n) < 0.5, 100.0, -100.0))  # noqa: E731
        c.update(q_rand=sign((2, BR)), q_cur=sign((2, BR)), q_next=sign((2, BR)), logp_cur=f(np.zeros(BR)), logp_next=f(np.zeros(BR)),
                 calib=f(np.full(B, -150.0)))
        # (q_data stays O(1): with mean Q(s, a) w near logsumexp w T = 150 the scaled term would be a float32 difference of two
        # numbers of that size, 1e-5 off in ANY float32 evaluation, the reference's included)
    elif kind == "all_equal":
        # the three values of a row equal: softmax 1/3 each.  Q_rand = v + float32(log 0.5^A) makes the random value v up to one
        # rounding (no tie with a return is involved: calibration off)
        cfg.update(calibrated=False)
        v = f(rng.integers(-3, 4, size=(2, BR)))
        c.update(q_cur=v, q_next=v.copy(), q_rand=f(v + np.float32(np.log(0.5 ** A))), logp_cur=f(np.zeros(BR)), logp_next=f(np.zeros(BR)))
    elif kind == "calib_above":
        c.update(calib=f(np.full(B, 64.0) + rng.integers(0, 4, size=B)))
    elif kind == "calib_tie":
        # the return equals the pi(s) value of critic 1 bit for bit in every row of observation b's FIRST repeat (log pi = 0 there)
        lp = c["logp_cur"].reshape(B, R).copy()
        lp[:, 0] = 0.0
        q = c["q_cur"].reshape(2, B, R).copy()
        q[0, :, 0] = c["calib"]
        q[1, :, 0] = c["calib"]
        c.update(logp_cur=f(lp.reshape(-1)), q_cur=f(q.reshape(2, BR)))
    elif kind == "alpha_at_min":
        c.update(cql_log_alpha=f([0.0]))
        cfg.update(alpha_min=1.0, alpha_max=2.0)
    elif kind == "alpha_at_max":
        c.update(cql_log_alpha=f([0.0]))
        cfg.update(alpha_min=0.5, alpha_max=1.0)
    elif kind == "alpha_below":
        c.update(cql_log_alpha=f([-1.0]))
        cfg.update(alpha_min=1.0, alpha_max=2.0)
    elif kind == "alpha_above":
        c.update(cql_log_alpha=f([2.0]))
        cfg.update(alpha_min=0.5, alpha_max=1.0)
    elif kind == "no_lagrange":
        cfg.update(with_lagrange=False)
    elif kind == "weight_zero":
        cfg.update(cql_weight=0.0)
    if kind not in ("big_values", "calib_above", "calib_tie"):
        # a return strictly inside critic 1's values of its observation: some above, some below, whatever B and R are
        v = np.stack([c["q_rand"][0] - np.float32(np.log(0.5 ** A)), c["q_cur"][0] - c["logp_cur"], c["q_next"][0] - c["logp_next"]])
        v = np.sort(v.reshape(3, B, R).transpose(1, 0, 2).reshape(B, 3 * R), axis=1)
        c["calib"] = f((v[:, 0] + v[:, 1]) / 2)
    if not cfg["calibrated"]:
        c["calib"] = None
    c["cfg"], c["A"], c["B"], c["R"], c["kind"] = cfg, A, B, R, kind
    return c


def reference(c: dict) -> dict:
    """float64 autograd of oracle_cql.cql_terms -> loss9 (ts_cql_loss's order), d_data [2, B], d_rep [2, 3, B R]."""
    cfg = OC.CQLConfig(**c["cfg"])
    t = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.float64)  # noqa: E731
    la = t(c["cql_log_alpha"]).reshape(()).requires_grad_(True)
    terms, leaves = [], []
    for k in range(2):
        qs = [t(c[n][k]).clone().requires_grad_(True) for n in ("q_data", "q_rand", "q_cur", "q_next")]
        leaves.append(qs)
        terms.append(OC.cql_terms(qs[0], t(c["target"]), qs[1], qs[2], qs[3], t(c["logp_cur"]), t(c["logp_next"]), t(c["calib"]), la,
                                  c["A"], cfg))
    d_data, d_rep = [], []
    for k in range(2):
        gs = torch.autograd.grad(terms[k]["loss"], leaves[k], retain_graph=True)
        d_data.append(gs[0].numpy())
        d_rep.append(np.stack([g.numpy() for g in gs[1:]]))
    if cfg.with_lagrange:
        al = -(terms[0]["cql"] + terms[1]["cql"]) * 0.5
        (g_la,) = torch.autograd.grad(al, [la])
        tail = [float(terms[0]["cql_alpha"].detach()), float(al.detach()), float(g_la)]
    else:
        tail = [1.0, 0.0, 0.0]                              # ts_cql_loss's convention without the multiplier
    loss9 = np.array([float(terms[0]["mse"].detach()), float(terms[1]["mse"].detach()), float(terms[0]["lse"].detach()),
                      float(terms[1]["lse"].detach()), float(terms[0]["cql"].detach()), float(terms[1]["cql"].detach())] + tail)
    return {"loss9": loss9, "d_data": np.stack(d_data), "d_rep": np.stack(d_rep)}
