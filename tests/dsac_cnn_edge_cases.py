"""Edge inputs of the three DiscreteSAC head kernels (ts_dsac_cnn_target / _critic / _actor), shared by the CPU test of the
oracle on them (test_dsac_cnn_edge_inputs_cpu.py) and the GPU test of the raw-array kernels (test_gpu_dsac_cnn_edges.py).

Every case is a dict of host arrays: logits / q1 / q2 float32 [B, A], act int64 [B], y float32 [B], weight float32 [B] or None,
alpha (a float) and device_alpha (whether the kernel reads exp(log_alpha) from the device instead of the scalar).  Shapes: A in
{1, 2, 31, 32, 33, 64} (one action; the smallest distribution; one below, at and one above the 32-wide head tile; the widest
head, a full wave), B in {1, 5, 64} (one sample; five, no multiple of the four waves per block; sixteen full blocks).

References come from tests/oracle_dsac_cnn.py (`expected`): values from the reference's own expressions, gradients from autograd.

Tolerances (TOL): 1e-5 of the scale of each output, the per-sample entropies and both losses included (the project's bar for
per-sample head kernels, test_gpu_crr_edges.py; test_dsac_cnn_edge_inputs_cpu.py checks that the float32 oracle stays within
half of it of a float64 run on every case), and exact statements where the mathematics is exact:
zeros in the padding, zeros of the critic gradient away from act, a zero loss under zero weights, p in {0, 1} and H = 0 with
one logit 200 above the rest (exp(-200) underflows in float32), zero gradient wherever autograd's is zero there.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_dsac_cnn as OS

A_SET = (1, 2, 31, 32, 33, 64)
B_SET = (1, 5, 64)
TOL = 1e-5


def _base(A: int, B: int, seed: int) -> dict:
    rng = np.random.default_rng(1000 * A + 10 * B + seed)
    act = rng.integers(0, A, size=B)
    act[0] = 0
    act[-1] = A - 1 if B > 1 else act[-1]
    return {"logits": rng.normal(size=(B, A)).astype(np.float32) * 2.0, "q1": rng.normal(size=(B, A)).astype(np.float32),
            "q2": rng.normal(size=(B, A)).astype(np.float32), "act": act.astype(np.int64),
            "y": rng.normal(size=B).astype(np.float32), "weight": None, "alpha": 0.2, "device_alpha": False}


def cases() -> list[tuple[str, dict]]:
    out = []
    for A in A_SET:
        for B in B_SET:
            c = _base(A, B, 0)
            c["weight"] = (0.25 + np.random.default_rng(A + B).random(B)).astype(np.float32) if B == 5 else None
            c["device_alpha"] = B == 64                           # the device-read alpha on the largest batch of every width
            out.append((f"random-A{A}-B{B}", c))
    for A in (2, 33, 64):
        c = _base(A, 5, 1)                                        # one logit 200 above the rest, in a different column per row
        c["logits"][:] = np.random.default_rng(A).normal(size=(5, A)).astype(np.float32)
        for b in range(5):
            c["logits"][b, (b * 7) % A] += 200.0
        out.append((f"dominant-A{A}", c))
        c = _base(A, 5, 2)                                        # all logits equal: H = log A, at three different levels
        c["logits"][:] = np.array([0.0, -3.5, 50.0, 1e-3, 7.25], np.float32)[:, None]
        out.append((f"uniform-A{A}", c))
        c = _base(A, 5, 3)                                        # q1 == q2: min picks either, the result must not depend on which
        c["q2"] = c["q1"].copy()
        out.append((f"ties-A{A}", c))
    c = _base(6, 5, 4)
    c["weight"] = np.zeros(5, np.float32)                         # all-zero weights: loss 0, gradient 0
    out.append(("weight-zero", c))
    c = _base(6, 64, 5)
    c["weight"] = np.where(np.arange(64) % 3 == 0, 0.0, np.linspace(0.1, 2.0, 64)).astype(np.float32)      # zeros among the rest
    out.append(("weight-mixed", c))
    c = _base(6, 5, 6)
    c["y"] = np.array([1e6, -1e6, 3e4, 0.0, -2.5e5], np.float32)  # |td| large: td^2 up to 1e12
    out.append(("td-large", c))
    c = _base(3, 5, 7)
    c["alpha"], c["device_alpha"] = 1.5, True                     # the same alpha, fixed and read from the device: see the tests
    out.append(("alpha-device", c))
    c = _base(3, 5, 7)
    c["alpha"] = 1.5
    out.append(("alpha-fixed", c))
    c = _base(3, 5, 8)
    c["alpha"] = 0.0                                              # no entropy term at all
    out.append(("alpha-zero", c))
    return out


def log_alpha_of(c: dict):
    """float32 log alpha for the device-read path; exp(float32(log alpha)) is the alpha the references then use."""
    return np.float32(np.log(c["alpha"])) if c["device_alpha"] else None


def alpha_of(c: dict) -> float:
    la = log_alpha_of(c)
    return float(torch.tensor(la).exp().item()) if la is not None else float(c["alpha"])


def expected(c: dict, dtype=torch.float32) -> dict:
    """The oracle on one case -> numpy arrays: target [B]; td [B], critic_loss, dq [B, A]; entropy [B], actor_loss, dlogits
    [B, A], probs [B, A]."""
    t = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    lg, q1, q2 = t(c["logits"]), t(c["q1"]), t(c["q2"])
    alpha = alpha_of(c)
    out = {"target": OS.target_from_heads(lg, q1, q2, alpha)}
    q = q1.clone().requires_grad_(True)
    loss, td = OS.critic_from_head(q, c["act"], t(c["y"]), None if c["weight"] is None else t(c["weight"]))
    out.update(critic_loss=loss.detach(), td=td.detach(), dq=torch.autograd.grad(loss, q)[0])
    lgg = lg.clone().requires_grad_(True)
    loss, ent = OS.actor_from_heads(lgg, q1, q2, alpha)
    out.update(actor_loss=loss.detach(), entropy=ent.detach(), dlogits=torch.autograd.grad(loss, lgg)[0],
               probs=torch.distributions.Categorical(logits=lg).probs)
    return {k: v.detach().double().numpy() for k, v in out.items()}
