"""Edge inputs of the continuous-BCQ per-sample kernels (ts_cbcq_latent / _recon / _target / _perturb) and of ts_cbcq_policy_forward,
with their float64 references: tests/oracle_cbcq.py's formulas under autograd.  Shared by tests/test_gpu_cbcq_edges.py and
tests/test_gpu_cbcq_policy.py (the kernels) and tests/test_cbcq_edge_inputs_cpu.py (the inputs are what they claim to be).  Every
array is float32; the reference sees the same values widened to float64.

Exact cases are built from values at which float32 and float64 agree bit for bit: tanh(0) = 0, tanh(+-20) = +-1 in both, exp(0) = 1,
a bound that is itself a float32 number and its float32 neighbour."""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_cbcq as OB

SHAPES = [(1, 1, 1, 1), (3, 6, 37, 3), (6, 12, 257, 10), (32, 64, 64, 2)]          # (A, L, B, R)
MAX_ACTION, PHI = 1.5, 0.3
LATENT_KINDS = ("generic", "ls_at_min", "ls_at_max", "ls_beyond", "zero")
RECON_KINDS = ("generic", "saturated", "recon_equals_act")
TARGET_KINDS = ("generic", "q_equal_l0", "q_equal_l075", "q_equal_l1", "max_first", "max_last", "all_equal", "all_done", "r_one")
PERTURB_KINDS = ("generic", "at_bound", "beyond", "phi_zero")
f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
t64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)  # noqa: E731


def _rng(kind: str, kinds, *shape):
    return np.random.default_rng(kinds.index(kind) * 100003 + sum(s * 7 ** i for i, s in enumerate(shape)))


def latent_case(kind: str, B: int, L: int) -> dict:
    r = _rng(kind, LATENT_KINDS, B, L)
    c = dict(mean=f32(r.normal(size=(B, L))), log_std=f32(r.uniform(-2, 2, size=(B, L))), eps=f32(r.normal(size=(B, L))),
             dz=f32(r.normal(size=(B, L)) / (B * L)), kind=kind)
    if kind == "ls_at_min":
        c["log_std"] = f32(np.full((B, L), -4.0))
    elif kind == "ls_at_max":                       # exp(15) = 3.3e6: large but finite, eps of both signs
        c["log_std"] = f32(np.full((B, L), 15.0))
        c["eps"] = f32(np.abs(c["eps"]) * np.where(np.arange(B * L).reshape(B, L) % 2 == 0, 1.0, -1.0))
    elif kind == "ls_beyond":                       # the float32 neighbours outside [-4, 15], alternating
        lo, hi = np.nextafter(np.float32(-4), np.float32(-np.inf)), np.nextafter(np.float32(15), np.float32(np.inf))
        c["log_std"] = f32(np.where(np.arange(B * L).reshape(B, L) % 2 == 0, lo, hi))
    elif kind == "zero":                            # KL and every gradient exactly 0, z = eps
        c.update(mean=f32(np.zeros((B, L))), log_std=f32(np.zeros((B, L))), dz=f32(np.zeros((B, L))))
    return c


def latent_reference(c: dict, dtype=torch.float64) -> dict:
    mean, raw = (torch.as_tensor(c[k]).to(dtype).requires_grad_(True) for k in ("mean", "log_std"))
    eps, dz = torch.as_tensor(c["eps"]).to(dtype), torch.as_tensor(c["dz"]).to(dtype)
    z, std = OB.latent(mean, raw, eps)
    kl = OB.kl_term(mean, std)
    dm, dl = torch.autograd.grad((z * dz).sum() + kl / 2, [mean, raw])
    return dict(z=z.detach().numpy(), kl=float(kl.detach()), d_mean=dm.numpy(), d_log_std=dl.numpy())


def recon_case(kind: str, B: int, A: int) -> dict:
    r = _rng(kind, RECON_KINDS, B, A)
    c = dict(logits=f32(r.normal(size=(B, A)) * 2), act=f32(r.uniform(-MAX_ACTION, MAX_ACTION, size=(B, A))), kind=kind)
    if kind == "saturated":
        c["logits"] = f32(np.where(r.random((B, A)) < 0.5, 20.0, -20.0))
    elif kind == "recon_equals_act":                # logits at which tanh is exact: 0 and +-20
        pick = r.integers(0, 3, size=(B, A))
        c["logits"] = f32(np.choose(pick, [0.0, 20.0, -20.0]))
        c["act"] = f32(np.choose(pick, [0.0, MAX_ACTION, -MAX_ACTION]))
    return c


def recon_reference(c: dict, dtype=torch.float64) -> dict:
    cfg = OB.CBCQConfig(max_action=MAX_ACTION)
    x = torch.as_tensor(c["logits"]).to(dtype).requires_grad_(True)
    recon = cfg.max_action * torch.tanh(x)
    mse = torch.nn.functional.mse_loss(torch.as_tensor(c["act"]).to(dtype), recon)
    (dx,) = torch.autograd.grad(mse, [x])
    return dict(recon=recon.detach().numpy(), mse=float(mse.detach()), d_logits=dx.numpy())


def target_case(kind: str, B: int, R: int) -> dict:
    if kind == "r_one":
        R = 1
    r = _rng(kind, TARGET_KINDS, B, R)
    c = dict(q1=f32(r.normal(size=B * R)), q2=f32(r.normal(size=B * R)), rew=f32(r.normal(size=B)),
             done=f32(r.random(B) < 0.3), gamma=0.97, lmbda=0.75, R=R, kind=kind)
    if kind.startswith("q_equal"):
        c["q2"] = c["q1"].copy()
        c["lmbda"] = {"q_equal_l0": 0.0, "q_equal_l075": 0.75, "q_equal_l1": 1.0}[kind]
    elif kind in ("max_first", "max_last"):         # the row maximum (by a margin) at the first / last of the R values
        pos = 0 if kind == "max_first" else R - 1
        for q in ("q1", "q2"):
            v = c[q].reshape(B, R)
            v[:, pos] = 10.0 + np.abs(v[:, pos])
    elif kind == "all_equal":
        c["q1"] = f32(np.repeat(r.integers(-3, 4, size=B), R))
        c["q2"] = f32(np.repeat(r.integers(-3, 4, size=B), R))
    elif kind == "all_done":
        c["done"] = f32(np.ones(B))
    return c


def target_reference(c: dict, dtype=torch.float64) -> np.ndarray:
    cfg = OB.CBCQConfig(gamma=c["gamma"], lmbda=c["lmbda"])
    t = lambda k: torch.as_tensor(c[k]).to(dtype)  # noqa: E731
    return OB.target_value(t("q1"), t("q2"), t("rew"), t("done"), c["R"], cfg).numpy()


def perturb_case(kind: str, B: int, A: int) -> dict:
    r = _rng(kind, PERTURB_KINDS, B, A)
    M = np.float32(MAX_ACTION)
    c = dict(logits=f32(r.normal(size=(B, A))), sampled=f32(r.uniform(-1.1 * MAX_ACTION, 1.1 * MAX_ACTION, size=(B, A))),
             dq=f32(r.normal(size=(B, A)) / B), phi=PHI, kind=kind)
    sign = np.where(r.random((B, A)) < 0.5, 1.0, -1.0)
    if kind == "at_bound":                          # tanh(0) = 0: the perturbed action IS the sampled one, exactly on the bound
        c.update(logits=f32(np.zeros((B, A))), sampled=f32(sign * M))
    elif kind == "beyond":                          # the float32 neighbour of the bound on its outside
        c.update(logits=f32(np.zeros((B, A))), sampled=f32(sign * np.nextafter(M, np.float32(np.inf))))
    elif kind == "phi_zero":
        c["phi"] = 0.0
    return c


def perturb_reference(c: dict, dtype=torch.float64) -> dict:
    cfg = OB.CBCQConfig(phi=c["phi"], max_action=MAX_ACTION)
    x = torch.as_tensor(c["logits"]).to(dtype).requires_grad_(True)
    out = OB.perturb(x, torch.as_tensor(c["sampled"]).to(dtype), cfg)
    (dx,) = torch.autograd.grad((out * torch.as_tensor(c["dq"]).to(dtype)).sum(), [x])
    return dict(perturbed=out.detach().numpy(), d_logits=dx.numpy())


# ---- policy forward -----------------------------------------------------------------------------------------------
POLICY_DIMS = dict(obs_dim=11, act_dim=3, latent_dim=6, hidden=(64, 64), vae_hidden=(96, 96))
POLICY_SEED = 5
POLICY_GAP = 1e-4            # of the larger of the top two values


def policy_case(N: int, T: int, first_row: bool, tie: bool = False) -> dict:
    """Parameters, observations and raw draws [N, T, L].  tie: per observation the float64 oracle's best draw is copied to the
    index behind it (before it when it is the last one), so the two candidates are identical and the lower index wins."""
    d = POLICY_DIMS
    p = OB.init_params(d["obs_dim"], d["act_dim"], d["latent_dim"], POLICY_SEED, d["hidden"], d["vae_hidden"])
    r = np.random.default_rng(POLICY_SEED * 1000 + N * 7 + T)
    # a critic at nn.Linear's default init is nearly flat in the action: the head is scaled up so that the candidates' values
    # are spread by far more than float32 rounding
    p[1]["wq"] = p[1]["wq"] * 8.0
    cfg = OB.CBCQConfig(phi=0.3, max_action=MAX_ACTION, pert_first_row=first_row, forward_sampled_times=T)
    c = dict(params=p, cfg=cfg, obs=f32(r.normal(size=(N, d["obs_dim"]))), noise=f32(r.normal(size=(N, T, d["latent_dim"]))), N=N, T=T,
             want_idx=None)
    if tie:
        assert T >= 3
        idx = policy_reference(c)["idx"]
        want = []
        for n, a in enumerate(idx):
            j = a + 1 if a + 1 < T else a - 1
            c["noise"][n, j] = c["noise"][n, a]
            want.append(min(a, j))
        c["want_idx"] = np.array(want)
    return c


def policy_reference(c: dict, dtype=torch.float64) -> dict:
    cast = lambda p: {k: v.to(dtype) for k, v in p.items()}  # noqa: E731
    pert, c1, _, vae = (cast(p) for p in c["params"])
    act, idx, q, cand = OB.policy_forward(pert, c1, vae, c["cfg"], torch.as_tensor(c["obs"]).to(dtype), torch.as_tensor(c["noise"]).to(dtype))
    return dict(act=act.numpy(), idx=idx.numpy(), q=q.numpy(), cand=cand.numpy())


def top_two_gap(q: np.ndarray) -> np.ndarray:
    """Per observation: (largest - second largest) / |largest| of its T values (inf when T == 1)."""
    if q.shape[1] == 1:
        return np.full(q.shape[0], np.inf)
    s = np.sort(q, axis=1)
    return (s[:, -1] - s[:, -2]) / np.maximum(np.abs(s[:, -1]), 1e-30)
