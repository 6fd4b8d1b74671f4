"""TEST INFRASTRUCTURE ONLY - edge inputs of the two TD3+BC kernels of ts_sac.hip (td3bc_actor_loss_kernel,
td3bc_policy_bwd_kernel) and their float64 reference.  tests/test_td3bc_edge_inputs_cpu.py proves on the CPU that the inputs
have the properties tests/test_gpu_td3bc_edges.py relies on.

Every case is one minibatch on freshly initialised Net[hidden, hidden] networks (oracle_sac.init_td3_params) whose critic-1
head is rescaled and biased so that Q = Q1(s, pi(s)) has a prescribed mean and a mean absolute deviation of 0.5 (B = 1: no
deviation to scale, Q is the prescribed mean itself), which keeps lmbda = alpha / mean|Q| well conditioned in every case:

  mixed      Q of both signs around a mean of 0 (B = 1: Q = 0.5; one sample has one sign): -lmbda mean(Q) is a cancellation
  negative   every Q < 0 (largest Q = -0.5): lmbda must come from |Q|, not from Q
  saturated  actor head = TD3_HEAD_BIASES (columns of +-12: tanh == +-1.0f) with zero head weights, mean(Q) = -0.3
  cloned     actor head of 0 / +-12 with zero head weights, so pi(s) is 0 / +-max_action exactly in any float32 arithmetic,
             and a_data = pi(s) bit for bit: the cloning term and its gradient vanish; mean(Q) = 0.4
  alpha0     "mixed" inputs with alpha = 0: lmbda == 0, pure behaviour cloning
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle_sac as OS
from tests import oracle_td3bc as OB
from tests.sac_edge_cases import TD3_HEAD_BIASES, double

KINDS = ("mixed", "negative", "saturated", "cloned", "alpha0")
MAX_ACTION, ALPHA = 1.5, 2.5
CLONED_HEAD = (0.0, 12.0, -12.0, 0.0, 0.0, 12.0)
MEAN_Q = {"mixed": 0.0, "alpha0": 0.0, "saturated": -0.3, "cloned": 0.4}


def q64(case: dict) -> torch.Tensor:
    """Q1(s, pi(s)) [B] in float64 on the case's float32 parameters."""
    with torch.no_grad():
        obs = case["obs"].double()
        return OS.critic_forward(double(case["critic1"]), obs, OS.det_actor_forward(double(case["actor"]), obs, MAX_ACTION)).flatten()


def edge_case(kind: str, obs_dim: int, act_dim: int, B: int, seed: int, hidden=64) -> dict:
    assert kind in KINDS
    actor, c1, c2 = OS.init_td3_params(obs_dim, act_dim, seed, True, hidden)
    actor, c1 = {k: v.clone() for k, v in actor.items()}, {k: v.clone() for k, v in c1.items()}
    g = torch.Generator().manual_seed(1000 * seed + 10 * B + act_dim)
    obs = torch.randn(B, obs_dim, generator=g)
    a_data = (torch.rand(B, act_dim, generator=g) * 2 - 1) * MAX_ACTION
    ret = torch.randn(B, generator=g)
    if kind in ("saturated", "cloned"):
        pattern = TD3_HEAD_BIASES if kind == "saturated" else CLONED_HEAD
        actor["wa"].zero_()
        actor["ba"] = torch.tensor([pattern[j % len(pattern)] for j in range(act_dim)], dtype=torch.float32)
    case = dict(kind=kind, actor=actor, critic1=c1, critic2=c2, obs=obs, act=a_data, ret=ret, alpha=0.0 if kind == "alpha0" else ALPHA)
    head_w, head_b = "wq", "bq"                             # (oracle_sac.critic_order: the single-Linear Q head)
    c1[head_b].zero_()
    q0 = q64(case)
    dev = float((q0 - q0.mean()).abs().mean())
    if dev > 0.0:                                           # B = 1: one sample has no deviation
        c1[head_w] *= 0.5 / dev
        q0 = q64(case)
    if kind == "negative":
        shift = -0.5 - float(q0.max())
    else:
        shift = (0.5 if kind in ("mixed", "alpha0") and B == 1 else MEAN_Q[kind]) - float(q0.mean())
    c1[head_b].fill_(shift)
    if kind == "cloned":
        with torch.no_grad():
            case["act"] = OS.det_actor_forward(actor, obs, MAX_ACTION)            # float32: exactly 0 / +-max_action
    ba = actor["ba"].abs().numpy()
    sat = kind in ("saturated", "cloned")
    case["cols"] = {"saturated": np.flatnonzero(ba == 12.0) if sat else np.zeros(0, np.int64),
                    "free": np.flatnonzero(ba < 12.0) if sat else np.arange(act_dim)}
    return case


def reference64(case: dict) -> dict:
    """float64 autograd of the oracle formula (tests/oracle_td3bc.py::actor_loss_terms) on the case: loss, lmbda, Q, the actor
    gradient, and the gradients of its two terms alone (`td3`: -mean(Q), the plain TD3 actor loss; `bc`: mse_loss)."""
    obs, act = case["obs"].double(), case["act"].double()
    c1 = double(case["critic1"])
    p = {k: v.double().requires_grad_(True) for k, v in case["actor"].items()}
    loss, lmbda, q, pi = OB.actor_loss_terms(p, c1, obs, act, MAX_ACTION, case["alpha"])
    out = dict(loss=float(loss.detach()), lmbda=float(lmbda), q=q.detach(), grads=dict(zip(p, torch.autograd.grad(loss, list(p.values())))))
    p = {k: v.double().requires_grad_(True) for k, v in case["actor"].items()}
    pi = OS.det_actor_forward(p, obs, MAX_ACTION)
    out["td3"] = dict(zip(p, torch.autograd.grad(-OS.critic_forward(c1, obs, pi).mean(), list(p.values()))))
    p = {k: v.double().requires_grad_(True) for k, v in case["actor"].items()}
    bc = torch.nn.functional.mse_loss(OS.det_actor_forward(p, obs, MAX_ACTION), act)
    out["bc_loss"] = float(bc.detach())
    out["bc"] = dict(zip(p, torch.autograd.grad(bc, list(p.values()), allow_unused=True)))
    return out
