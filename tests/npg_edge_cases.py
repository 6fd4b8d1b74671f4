"""Inputs and float64 / float32 references for the NPG / TRPO actor step (ts_npg.hip, ts_npg_q.h, the launch code in ts_ppo.hip)
where tests/test_gpu_npg.py never goes: the line search picking another candidate than the first, or none; conjugate gradients
leaving their loop early; shapes on either side of the one-launch / per-layer route boundary; B = 1 and B on the 32-row tile and
256-thread block edges; trunks other than Net[64, 64] tanh.  Shared by tests/test_npg_edge_inputs_cpu.py and
tests/test_gpu_npg_edges.py: BOTH iterate LINE_SEARCH / CG_EXIT / SHAPES below, so no case reaches the GPU test without its CPU
precondition.  Nothing here touches the GPU path or imports the product.

Reference.  `reference_actor_step` restates npg.py:140-224 / trpo.py:123-202 for a Gaussian actor on any trunk (the Fisher-vector
product is the double backward of the mean KL plus damping) and returns a trace of every decision; `reference32(case)` is bit for
bit oracle_npg.minibatch_step on Net[64, 64] tanh (tests/test_npg_edge_inputs_cpu.py), which tests/test_oracle_golden.py pins to
the unmodified reference.  `reference64(case)` is the same in float64 (the ratio is NOT rounded to float32 there).

Bars (the project's existing ones, no new numbers; e32 = the same error of reference32 against reference64):
    grad, fg     rel_err < max(1e-5, 2 e32)                         test_gpu_npg.py::test_actor_step_vs_oracle_and_float64
    cg           rel_err < max(1e-4, 2 e32)                         ..::test_one_launch_actor_passes_match_the_per_layer_passes
    new          max|new - new64| / max|new64 - old| < max(1e-4, 2 e32)                                             the same
    stats        |x - ref64| <= 2e-5 + 2e-3 |ref64|  (actor_loss, kl, step_size)        the golden tests' rtol / atol
    pick         round(log(step_size / step0_64) / log(coeff)) == the reference's pick; nothing accepted: step_size == 0.0 and
                 the parameters bit-identical
Preconditions of every case, asserted on the CPU (conditions on the inputs, not measurements):
    (a) reference32 and reference64 agree on the picked candidate and on the CG exit iteration;
    (b) every candidate up to the picked one (all of them when none is picked): |kl_k / max_kl - 1| >= 0.1 and
        |loss_k - loss_0| >= 1e-3 |loss_0|;
    (c) an exit at iteration j: rdotr_j <= tol / 3 and rdotr_{j-1} >= 3 tol, in float64 and float32;
    (d) CG_EXIT cases that exit: the float64 solution WITHOUT the break differs by >= 1e-3 of its largest entry;
    (e) reference32 sits within QUARTER = 0.25 of every bar's floor (e32 <= floor / 4; stats within a quarter of their bar).
Measured |reference32 - reference64| / floor (tests/test_npg_edge_inputs_cpu.py prints them with -s):

    case                                  pick exit   grad   fg     cg     new    stats
    LINE_SEARCH on (17, 6), B 700 (all)    ..    0    0.119  0.126  0.022  0.022  0.000
    stale logp_old, pick 1 of 10           1     0    0.148  0.133  0.031  0.031  0.000
    B 1, pick 0 of 10                      0     6    0.069  0.087  0.006  0.009  0.000
    loss criterion alone, pick 1 of 10     1     6    0.068  0.070  0.007  0.008  0.000
    npg cg exit 1 / 2 / 3 / 5 / 6          0     j    <= 0.029      0.034  0.005  0.089  0.000   (d): 2.5e-1 1.6e-2 4.5e-3 5.3e-3 1.9e-3
    trpo cg exit 1 / 2 / 3 / 5 / 6         0     j    <= 0.130      0.137  0.013  0.026  0.000   (d): the same
    npg / trpo cg exit never               0     0    0.032 / 0.119 0.126  0.022  0.023  0.000
    npg obs 32 act 8 / 33, 1 / 8, 9 / 5, 32  0   0    <= 0.042      0.067  0.086  0.087  0.000
    trpo obs 32 act 8                      0     0    0.095  0.123  0.024  0.025  0.000
    trpo obs 33 act 1                      1     0    0.020  0.027  0.009  0.008  0.000
    trpo obs 8 act 9                       1     0    0.070  0.152  0.076  0.076  0.000
    trpo obs 5 act 32                      0     0    0.156  0.205  0.044  0.047  0.002
    npg B 1 .. 257                         0   6 | 0  <= 0.047      0.051  0.028  0.028  0.000
    trpo B 1 .. 257 (B 256: pick 1)        0   6 | 0  <= 0.163      0.150  0.031  0.031  0.001
    trpo relu [64, 48, 32]                 1     7    0.041  0.023  0.008  0.009  0.000
    trpo tanh [96]                         1     0    0.052  0.062  0.022  0.021  0.000
    trpo tanh [48, 32] in [64, 64]         1     0    0.058  0.041  0.021  0.020  0.001
A wrong step against the same bars (test_every_gpu_assertion_is_sensitive): breaking one iteration late puts the CG solution at
19 .. 2,400 x its bar on every exiting case, and ignoring the break fails it on each of them too; always picking candidate 0, or
picking one too late, fails the recovered k on every LINE_SEARCH case with a pick, and stats and parameters on at least one.

Rejected by a precondition and therefore absent:
    max_kl 5 on the LINE_SEARCH inputs                          (b) kl_2 / max_kl = 1.008
    cg: damping 0.1, advantages x 1e-5 (exit 1)                 (c) rdotr_0 = 1.9e-10 < 3 tol; no scale fits: rdotr_1 / rdotr_0 = 0.27
    cg: damping 1, advantages x 1e-4 (exit 5) / x 1e-3 (exit 7) (c) rdotr 1.8e-10 -> 3.8e-11 / 4.8e-10 -> 7.3e-11: the residual
                                                                falls by 5 - 7 x an iteration there, the margins need 9 x
    cg: exits at iteration 7 or 8 (damping 2 .. 5, seeds 1 .. 4) (d) the solution without the break differs by 6e-7 .. 3e-4 only
    B = 1 with advantages of unit scale                         (a) the residual reaches rounding: float64 exits at 7, float32 at 8
    trpo obs 5 act 32 at B = 257 and B = 100                    (e) grad 0.288 / 0.314 (B = 400, same seeds: 0.156)
    relu [64, 48, 32] at damping 0.1 / 1                        (e) cg 808 / 4.2: float32 conjugate gradients have no answer there
    trpo B 32, 255, 257 at max_kl 1; obs 33 act 1, B 100 at max_kl 0.3; obs 8 act 9 at max_kl 0.3
                                                                (b) kl_0 / max_kl = 0.906, 0.914, 0.927; 1.001; 0.973

The loss criterion alone.  A candidate with kl_k < max_kl but loss_k >= loss_0 would pin the second half of the select kernel's
`&&`.  Found: with a large damping the step size sqrt(2 max_kl / s (F + damping) s) overshoots the surrogate's minimum while the KL stays far below max_kl.  Grid (Net[64, 64] tanh, (17, 6)): B in {33, 257, 700} x network / data
seeds 1 .. 7 x damping {10, 30} x max_kl {3, 10, 30, 100} x N(0, 1) noise on logp_old x {0, 0.5} = 336 configurations; 6 reject a
candidate by the loss alone, 2 of them meet (a) to (c) and (e).  One is listed ("loss criterion alone, pick 1 of 10": B 257,
seeds 1 / 11, damping 10, max_kl 100: kl_0 / max_kl = 0.566, loss_0' > loss_0, pick 1), and the ReLU trunk of SHAPES is another
(kl_0 / max_kl = 0.79); LOSS_ONLY names both, and the CPU file asserts that candidate 0 fails on the loss alone.  No hook needed."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Independent, Normal, kl_divergence

from oracle import oracle_ppo as OP

QUARTER = 0.25
GRAD_FLOOR, CG_FLOOR, NEW_FLOOR = 1e-5, 1e-4, 1e-4
STATS_RTOL, STATS_ATOL = 2e-3, 2e-5
KL_MARGIN, LOSS_MARGIN, TOL_MARGIN, NO_BREAK_MARGIN = 0.1, 1e-3, 3.0, 1e-3
CG_ITERS, RESIDUAL_TOL = 10, 1e-10                   # NPGConfig.to_c: what the engine is given
ROUTES = ("one_launch", "per_layer", "net")
MUTATIONS = ("always_pick_0", "pick_late", "no_restore", "ignore_break", "break_late")
ACTIVATIONS = {"tanh": torch.tanh, "relu": torch.relu, "none": lambda x: x}


def rel_err(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- networks ----------------------------------------------------------------------------------------------------------------
def rand_net(obs_dim: int, act_dim: int, seed: int, hidden=(64, 64), activation: str = "tanh") -> dict:
    """dict(layers [(w, b)...], activation, mu (w, b), sigma [A]) in nn.Linear layout, float32.  Net[64, 64] tanh: the network of
    tests/test_gpu_npg.py::rand_params (orthogonal trunk, mu head x30 so that the mean depends on the observation, random
    sigma_param); other trunks: N(0, 1 / fan_in) weights, small biases, as test_generic_trunk_fisher_vector_product_vs_float64."""
    g = torch.Generator().manual_seed(seed)
    if tuple(hidden) == (64, 64) and activation == "tanh":
        p = OP.init_params(obs_dim, act_dim, seed=seed)
        sigma = torch.randn(act_dim, generator=g) * 0.3 - 0.5
        return dict(layers=[(p["a_w1"], p["a_b1"]), (p["a_w2"], p["a_b2"])], activation="tanh",
                    mu=(p["a_wmu"] * 30.0, p["a_bmu"]), sigma=sigma)
    layers, k = [], obs_dim
    for h in hidden:
        layers.append((torch.randn(h, k, generator=g) / math.sqrt(k), torch.randn(h, generator=g) * 0.1))
        k = h
    mu = (torch.randn(act_dim, k, generator=g) * 0.3 / math.sqrt(k), torch.randn(act_dim, generator=g) * 0.1)
    return dict(layers=layers, activation=activation, mu=mu, sigma=torch.full((act_dim,), -0.5) + 0.1 * torch.randn(act_dim, generator=g))


def net_tensors(net: dict) -> list:
    """[w1, b1, ..., w_mu, b_mu, sigma_param]: the order of actor_flat_from_torch / net_flat_from_tensors."""
    return [t for wb in net["layers"] for t in wb] + list(net["mu"]) + [net["sigma"]]


def ref_order(tensors) -> torch.Tensor:
    """[w1, b1, ..., w_mu, b_mu, sigma_param] -> the reference's flat vector (policy.actor.parameters(): sigma_param first)."""
    return torch.cat([tensors[-1].reshape(-1)] + [t.reshape(-1) for t in tensors[:-1]]).detach().cpu()


# ---- the reference -----------------------------------------------------------------------------------------------------------
def reference_actor_step(net: dict, obs, act, adv, logp_old, cfg: dict, dtype, mutate: str | None = None) -> dict:
    """One actor step of npg.py:140-177 (cfg["algo"] == "npg") / trpo.py:123-191 ("trpo") in `dtype`.  cfg: algo, damping,
    trust_region_size, max_kl, backtrack_coeff, max_backtracks.  -> trace: grad, fg (= F g + damping g), rdotr [g.g, after
    iteration 1, ...], exit_iter (1-based; 0: the loop ran out), search_direction, step0, cand_kl / cand_loss (every candidate
    k < max_backtracks, also those after the picked one), pick (-1: none), old / new (flat, reference order), stats (actor_loss,
    kl, step_size).  `mutate`: one of MUTATIONS, a deliberately WRONG step (for the CPU sensitivity checks only)."""
    assert mutate is None or mutate in MUTATIONS
    fn = ACTIVATIONS[net["activation"]]
    tensors = [t.detach().to(dtype) for t in net_tensors(net)]
    shapes = [tensors[-1].shape] + [t.shape for t in tensors[:-1]]
    obs, act, adv = obs.to(dtype), act.to(dtype), adv.to(dtype)
    logp_old = None if logp_old is None else logp_old.to(dtype)
    trpo = cfg["algo"] == "trpo"

    def dist_of(plist):                                  # plist in reference order: sigma_param, (w, b)*, w_mu, b_mu
        h = obs
        for i in range(len(net["layers"])):
            h = fn(F.linear(h, plist[1 + 2 * i], plist[2 + 2 * i]))
        mu = F.linear(h, plist[-2], plist[-1])
        # (validate_args=False: with all-zero advantages the candidates are NaN, which the line search has to reject)
        return Independent(Normal(mu, (plist[0].view(1, -1) + torch.zeros_like(mu)).exp(), validate_args=False), 1)

    def split(flat):
        out, off = [], 0
        for s in shapes:
            out.append(flat[off:off + s.numel()].reshape(s).clone())
            off += s.numel()
        return out

    def surrogate(dist):
        if trpo:
            ratio = (dist.log_prob(act) - logp_old).exp().to(dtype).reshape(len(adv), -1).transpose(0, 1)
            return -(ratio * adv).mean()
        return -(dist.log_prob(act).reshape(len(adv), -1).transpose(0, 1) * adv).mean()

    def flat_grad(y, **kw):
        return torch.cat([g.reshape(-1) for g in torch.autograd.grad(y, plist, **kw)])

    flat_params = torch.cat([tensors[-1].reshape(-1)] + [t.reshape(-1) for t in tensors[:-1]])
    plist = [t.clone().requires_grad_(True) for t in split(flat_params)]
    dist = dist_of(plist)
    actor_loss = surrogate(dist)
    flat_grads = flat_grad(actor_loss, retain_graph=True).detach()
    with torch.no_grad():
        old_dist = dist_of(split(flat_params))
    flat_kl_grad = flat_grad(kl_divergence(old_dist, dist).mean(), create_graph=True)

    def mvp(v):                                                         # npg.py:195-200
        return flat_grad((flat_kl_grad * v).sum(), retain_graph=True).detach() + v * cfg["damping"]

    x = torch.zeros_like(flat_grads)                                    # npg.py:202-224
    r, p = flat_grads.clone(), flat_grads.clone()
    rdotr = r.dot(r)
    trace, exit_iter, stop_at = [float(rdotr)], 0, None
    for it in range(1, CG_ITERS + 1):
        z = mvp(p)
        alpha = rdotr / p.dot(z)
        x += alpha * p
        r -= alpha * z
        new_rdotr = r.dot(r)
        trace.append(float(new_rdotr))
        if it == stop_at:
            break
        if new_rdotr < RESIDUAL_TOL and stop_at is None:
            exit_iter = exit_iter or it
            if mutate == "break_late":
                stop_at = it + 1
            elif mutate != "ignore_break":
                break
        p = r + new_rdotr / rdotr * p
        rdotr = new_rdotr
    sd = -x
    out = dict(grad=flat_grads.clone(), fg=mvp(flat_grads), rdotr=trace, exit_iter=exit_iter, search_direction=sd.clone(),
               old=flat_params.clone(), step0=0.0, cand_kl=[], cand_loss=[], pick=0)
    if trpo:                                                            # trpo.py:153-160
        step_size = torch.sqrt(2 * cfg["max_kl"] / (sd * mvp(sd)).sum(0, keepdim=True))
        out["step0"] = float(step_size)
    with torch.no_grad():
        if not trpo:
            new = flat_params + cfg["trust_region_size"] * sd
            kl, step = kl_divergence(old_dist, dist_of(split(new))).mean(), 0.0
            out["cand_kl"] = [float(kl)]
        else:
            cands, pick, mb = [], -1, cfg["max_backtracks"]
            for k in range(mb):                                         # trpo.py:167-191, every candidate evaluated
                cand = flat_params + step_size * sd
                new_dist = dist_of(split(cand))
                new_loss, kl_k = surrogate(new_dist), kl_divergence(old_dist, new_dist).mean()
                if pick < 0 and bool(kl_k < cfg["max_kl"]) and bool(new_loss < actor_loss):
                    pick = k
                cands.append((cand, kl_k, float(step_size)))
                out["cand_kl"].append(float(kl_k))
                out["cand_loss"].append(float(new_loss))
                step_size = step_size * cfg["backtrack_coeff"]
            out["true_pick"] = pick
            if mutate == "always_pick_0":
                pick = 0
            elif mutate == "pick_late" and pick >= 0:
                pick = pick + 1 if pick + 1 < mb else -1
            if pick >= 0:
                new, kl, step = cands[pick]
            else:
                new, kl, step = (cands[-1][0] if mutate == "no_restore" else flat_params.clone()), cands[-1][1], 0.0
            out["pick"] = pick
    out.update(new=new, stats=(float(actor_loss.detach()), float(kl), float(step)))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def make_case(name, algo, obs_dim=17, act_dim=6, B=700, hidden=(64, 64), activation="tanh", seed=3, data_seed=5, adv_scale=1.0,
              damping=0.1, max_kl=0.01, max_backtracks=10, stale=0.0, zero_adv=False, embed=None, pick=None, exit_iter=None) -> dict:
    """`pick` / `exit_iter`: what the case is in the list for (asserted on the CPU; None: whatever the reference does, as
    long as float32 and float64 agree).  `embed`: the engine width a narrower two-layer tanh trunk is zero-padded into."""
    hidden = tuple(hidden)
    fixed = (embed or hidden) == (64, 64) and activation == "tanh"
    routes = tuple(r for r in ROUTES if (r == "net" and embed is None) or (r == "per_layer" and fixed) or
                   (r == "one_launch" and fixed and obs_dim <= 32 and act_dim <= 8))
    return dict(name=name, algo=algo, obs_dim=obs_dim, act_dim=act_dim, B=B, hidden=hidden, activation=activation, seed=seed,
                data_seed=data_seed, adv_scale=adv_scale, damping=damping, max_kl=max_kl, max_backtracks=max_backtracks,
                stale=stale, zero_adv=zero_adv, embed=embed, pick=pick, exit_iter=exit_iter, routes=routes,
                backtrack_coeff=0.8, trust_region_size=0.1 / adv_scale)


def cfg_of(case: dict) -> dict:
    """(trust_region_size = 0.1 / adv_scale: NPG's step is linear in the advantages, TRPO's does not depend on their scale)"""
    return {k: case[k] for k in ("algo", "damping", "trust_region_size", "max_kl", "backtrack_coeff", "max_backtracks")}


# TRPO's line search on rand_net(17, 6, 3), B = 700, data seed 5, steered by max_kl and max_backtracks (kl_k / max_kl: 0.61, ..
# at 0.01; 1.47, 0.73 at 1; 3.40, 1.50, 0.69 at 3; 28.2, 9.9, 3.75, 1.51, 0.63 at 20, where candidates 1 and 2 also RAISE the loss)
_TR = dict(algo="trpo")
LINE_SEARCH = [
    make_case("pick 0 of 10", max_kl=0.01, pick=0, **_TR),
    make_case("pick 1 of 10", max_kl=1.0, pick=1, **_TR),
    make_case("pick 2 of 10", max_kl=3.0, pick=2, **_TR),
    make_case("pick 4 of 10", max_kl=20.0, pick=4, **_TR),
    make_case("pick 1 of 2 (the last)", max_kl=1.0, max_backtracks=2, pick=1, **_TR),
    make_case("pick 2 of 3 (the last)", max_kl=3.0, max_backtracks=3, pick=2, **_TR),
    make_case("none of 1", max_kl=1.0, max_backtracks=1, pick=-1, **_TR),
    make_case("none of 2", max_kl=3.0, max_backtracks=2, pick=-1, **_TR),
    make_case("pick 0 of 1", max_kl=0.01, max_backtracks=1, pick=0, **_TR),
    make_case("pick 1 of 32", max_kl=1.0, max_backtracks=32, pick=1, **_TR),
    make_case("pick 4 of 32", max_kl=20.0, max_backtracks=32, pick=4, **_TR),
    make_case("stale logp_old, pick 1 of 10", max_kl=1.0, stale=0.3, pick=1, **_TR),
    make_case("B 1, pick 0 of 10", B=1, max_kl=1.0, adv_scale=1e-4, pick=0, **_TR),
    make_case("loss criterion alone, pick 1 of 10", B=257, seed=1, data_seed=11, damping=10.0, max_kl=100.0, pick=1, **_TR),
]
# candidates rejected although kl_k < max_kl, because loss_k >= loss_0: the second half of trpo_select_kernel's `&&`
LOSS_ONLY = {"loss criterion alone, pick 1 of 10": (0,), "trpo relu [64, 48, 32]": (0,)}

# conjugate gradients leaving the loop: rdotr scales with the square of the advantages, its decay per iteration with damping
_EXITS = [(1, 10.0, 1.8e-5), (2, 10.0, 1e-4), (3, 10.0, 5e-4), (5, 3.0, 7.6e-4), (6, 2.0, 1.1e-3), (0, 0.1, 1.0)]
CG_EXIT = [make_case(f"{algo} cg exit {j or 'never'}", algo=algo, damping=d, adv_scale=s, exit_iter=j)
           for algo in ("npg", "trpo") for j, d, s in _EXITS]

# either side of the one-launch / per-layer boundary (obs 32 | 33, act 8 | 9), batch sizes round the 32-row tile and the
# 256-thread block, other trunks (NetNPGEngine) through a step that backtracks, a narrower network embedded by zero padding
_B_MAX_KL = {1: 1.0, 31: 1.0, 32: 0.05, 33: 1.0, 255: 0.3, 256: 1.0, 257: 0.3}
SHAPES = (
    [make_case(f"npg obs {o} act {a}", algo="npg", obs_dim=o, act_dim=a, B=257) for o, a in ((32, 8), (33, 1), (8, 9), (5, 32))]
    + [make_case("trpo obs 32 act 8", obs_dim=32, act_dim=8, B=257, max_kl=1.0, pick=0, **_TR),
       make_case("trpo obs 33 act 1", obs_dim=33, act_dim=1, B=100, max_kl=1.0, pick=1, **_TR),
       make_case("trpo obs 8 act 9", obs_dim=8, act_dim=9, B=257, max_kl=1.0, pick=1, **_TR),
       make_case("trpo obs 5 act 32", obs_dim=5, act_dim=32, B=400, max_kl=0.3, pick=0, **_TR)]
    + [make_case(f"{algo} B {B}", algo=algo, B=B, max_kl=_B_MAX_KL[B], adv_scale=1e-4 if B == 1 else 1.0)
       for algo in ("npg", "trpo") for B in (1, 31, 32, 33, 255, 256, 257)]
    + [make_case("trpo relu [64, 48, 32]", obs_dim=13, act_dim=4, B=600, hidden=(64, 48, 32), activation="relu", seed=5,
                 damping=10.0, max_kl=100.0, pick=1, **_TR),
       make_case("trpo tanh [96]", obs_dim=13, act_dim=4, B=600, hidden=(96,), max_kl=10.0, pick=1, **_TR),
       make_case("trpo tanh [48, 32] in [64, 64]", obs_dim=13, act_dim=4, B=600, hidden=(48, 32), embed=(64, 64), max_kl=3.0,
                 pick=1, **_TR)])

# all-zero advantages: the gradient is 0, alpha = 0 / 0, every candidate NaN -- nothing accepted, parameters restored
ZERO_ADV = [make_case("trpo zero advantages", B=257, zero_adv=True, pick=-1, **_TR)]

ALL_CASES = LINE_SEARCH + CG_EXIT + SHAPES
CASES = {c["name"]: c for c in ALL_CASES + ZERO_ADV}
assert len(CASES) == len(ALL_CASES) + len(ZERO_ADV)


@functools.lru_cache(maxsize=None)
def _built(name: str):
    c = CASES[name]
    net = rand_net(c["obs_dim"], c["act_dim"], c["seed"], c["hidden"], c["activation"])
    g = torch.Generator().manual_seed(c["data_seed"])
    B = c["B"]
    obs, act = torch.randn(B, c["obs_dim"], generator=g), torch.randn(B, c["act_dim"], generator=g) * 0.8
    adv = torch.randn(B, generator=g) * c["adv_scale"]
    if c["zero_adv"]:
        adv = torch.zeros(B)
    fn = ACTIVATIONS[net["activation"]]
    with torch.no_grad():
        h = obs
        for w, b in net["layers"]:
            h = fn(F.linear(h, w, b))
        mu = F.linear(h, *net["mu"])
        logp_old = Independent(Normal(mu, (net["sigma"].view(1, -1) + torch.zeros_like(mu)).exp()), 1).log_prob(act)
    if c["stale"]:
        logp_old = logp_old + c["stale"] * torch.randn(B, generator=g)
    return dict(net=net, obs=obs, act=act, adv=adv, logp_old=logp_old)


def inputs(case: dict) -> dict:
    """net, obs [B, obs_dim], act [B, A], adv [B], logp_old [B] (float32).  Built once per case; callers must not modify them."""
    return _built(case["name"])


@functools.lru_cache(maxsize=None)
def _ref(name: str, dtype, mutate=None):
    c, i = CASES[name], _built(name)
    return reference_actor_step(i["net"], i["obs"], i["act"], i["adv"], i["logp_old"], cfg_of(c), dtype, mutate)


def reference64(case: dict, mutate=None) -> dict:
    return _ref(case["name"], torch.float64, mutate)


def reference32(case: dict) -> dict:
    return _ref(case["name"], torch.float32)


# ---- bars --------------------------------------------------------------------------------------------------------------------
def _errors(got: dict, r64: dict) -> dict:
    step = float((r64["new"] - r64["old"]).abs().max())
    e = dict(grad=rel_err(got["grad"], r64["grad"]), fg=rel_err(got["fg"], r64["fg"]),
             cg=rel_err(got["search_direction"], r64["search_direction"]))
    if step > 0:
        e["new"] = float((got["new"].double() - r64["new"]).abs().max()) / step
    return e


FLOORS = dict(grad=GRAD_FLOOR, fg=GRAD_FLOOR, cg=CG_FLOOR, new=NEW_FLOOR)


def recovered_pick(step_size: float, r64: dict, cfg: dict) -> int:
    """The candidate a reported step size belongs to (-1: step size 0.0, nothing accepted); neighbours differ by 20 %."""
    if step_size == 0.0:
        return -1
    return int(round(math.log(step_size / r64["step0"]) / math.log(cfg["backtrack_coeff"])))


def ratios(got: dict, r64: dict, r32: dict | None, cfg: dict) -> dict:
    """error / bar per quantity (> 1 or == 1: the bar is violated) of `got` = dict(grad, fg, search_direction, new, stats) against
    reference64.  r32 None: against the bars' floors alone (what precondition (e) measures reference32 itself with).  `pick`:
    0.0 if the recovered candidate is the reference's, inf otherwise; `restored`: nothing accepted -> new must be old exactly."""
    e, e32 = _errors(got, r64), (_errors(r32, r64) if r32 is not None else {})
    out = {k: v / max(FLOORS[k], 2 * e32.get(k, 0.0)) for k, v in e.items()}
    out["stats"] = max(abs(g - w) / (STATS_ATOL + STATS_RTOL * abs(w)) for g, w in zip(got["stats"], r64["stats"]))
    if cfg["algo"] == "trpo" and not any(math.isnan(v) for v in r64["stats"]):
        out["pick"] = 0.0 if recovered_pick(got["stats"][2], r64, cfg) == r64["pick"] else float("inf")
    else:
        out["pick"] = 0.0 if got["stats"][2] == 0.0 else float("inf")
    if r64["pick"] < 0:
        out["restored"] = 0.0 if torch.equal(got["new"].double(), r64["old"]) else float("inf")
    return out


def precondition_failures(case: dict, no_break: bool = False) -> list:
    """Why `case` may not be in a list: the violated ones of (a), (b), (c), (e) -- and (d) with `no_break` -- as strings."""
    r64, r32, cfg, bad = reference64(case), reference32(case), cfg_of(case), []
    if r64["pick"] != r32["pick"] or r64["exit_iter"] != r32["exit_iter"]:
        bad.append(f"(a) pick {r64['pick']} / {r32['pick']}, exit {r64['exit_iter']} / {r32['exit_iter']}")
    for r in (r64, r32):
        if case["algo"] == "trpo":
            for k in range(case["max_backtracks"] if r["pick"] < 0 else r["pick"] + 1):
                if abs(r["cand_kl"][k] / case["max_kl"] - 1) < KL_MARGIN:
                    bad.append(f"(b) kl_{k} / max_kl = {r['cand_kl'][k] / case['max_kl']:.3f}")
                if abs(r["cand_loss"][k] - r["stats"][0]) < LOSS_MARGIN * abs(r["stats"][0]):
                    bad.append(f"(b) loss_{k} - loss_0 = {r['cand_loss'][k] - r['stats'][0]:.2e}")
        j = r["exit_iter"]
        if j and not (r["rdotr"][j] <= RESIDUAL_TOL / TOL_MARGIN and r["rdotr"][j - 1] >= TOL_MARGIN * RESIDUAL_TOL):
            bad.append(f"(c) rdotr {r['rdotr'][j - 1]:.2e} -> {r['rdotr'][j]:.2e}")
        if not j and min(r["rdotr"]) < TOL_MARGIN * RESIDUAL_TOL:
            bad.append(f"(c) no exit, but rdotr down to {min(r['rdotr']):.2e}")
    if no_break and r64["exit_iter"] and no_break_difference(case) < NO_BREAK_MARGIN:
        bad.append(f"(d) the solution without the break differs by {no_break_difference(case):.2e}")
    q = ratios(r32, r64, None, cfg)
    if max(q.values()) > QUARTER:
        bad.append("(e) " + " ".join(f"{k} {v:.3f}" for k, v in q.items() if v > QUARTER))
    return bad


def no_break_difference(case: dict) -> float:
    """Precondition (d): max|x without the break - x| / max|x|, float64."""
    a, b = reference64(case, "ignore_break")["search_direction"], reference64(case)["search_direction"]
    return float((a - b).abs().max() / b.abs().max())
