"""Inputs that put EXACT values into the per-sample heads of the SAC family (shared by tests/test_sac_edge_inputs_cpu.py and the
tests/test_gpu_{sac,td3,dsac}_edges.py GPU tests; nothing here touches the GPU path).

The actor's last Linear gets zero weights, so head[b, j] == bias[j] for every row, exactly, whatever the trunk computes; the
rsample() noise carries the per-row variety.  That reaches what N(0, 1) observations on a freshly initialised network never do:
the two branches and the two boundaries of clamp(log sigma, -20, 2), tanh at and beyond saturation in float32, Q1 == Q2, and a
softmax row that one logit dominates."""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle_dsac as ODS
from oracle import oracle_sac as OS

EPS32 = float(np.finfo(np.float32).eps)
LOG_SQRT_2PI = 0.5 * float(np.log(2.0 * np.pi))


def _inward(x: float) -> float:
    """The float32 next to x on the side of zero."""
    return float(np.nextafter(np.float32(x), np.float32(0.0)))


# log-sigma biases: the two boundaries of the inclusive clamp, their inward neighbours, beyond the clamp, interior
SIG_BIASES = (OS.SIGMA_MIN, OS.SIGMA_MAX, _inward(OS.SIGMA_MIN), _inward(OS.SIGMA_MAX), -25.0, 3.0, -3.0, -1.0, 0.0, 1.0)
SIG_KINDS = ("boundary", "boundary", "inward", "inward", "beyond", "beyond", "interior", "interior", "interior", "interior")
MU_BIASES = (0.0, 0.5, -0.5, 2.0, -2.0, 3.5, -3.5, 5.0, -5.0, 7.0, -7.0, 9.5, -9.5, 12.0, -12.0, 20.0)
# |a| bands of the accuracy sweep: tanh far from / approaching / inside the band where 1 - tanh^2 falls below float32's
# resolution / saturated (tanh(a) == 1.0f from |a| ~ 9.01 on)
A_BANDS = ((0.0, 3.0), (3.0, 6.0), (6.0, 9.1), (9.1, np.inf))


def gaussian_columns(act_dim: int, shift: int = 0, benign_only: bool = False):
    """(bmu, bsig, {kind: column indices}) for column j = entry (j + shift) of the two cycles; 3 is coprime to 16, so the mu
    cycle pairs every log-sigma kind with small and large means.  `moderate`: |mu| <= 2 and log sigma in [-3, 1], where the
    gradient is well conditioned in the columns this cycle produces; `benign_only`: every column has |mu| <= 0.5 and
    sigma <= e^-1, so that |a| stays below ~2.5 and float32 is within a few ulp of float64 everywhere."""
    j = np.arange(act_dim) + shift
    if benign_only:
        bmu = torch.tensor([MU_BIASES[i] for i in j % 3], dtype=torch.float32)
        bsig = torch.tensor([SIG_BIASES[6 + i] for i in (j // 3) % 2], dtype=torch.float32)
        return bmu, bsig, {"moderate": np.arange(act_dim)}
    si, mi = j % len(SIG_BIASES), (3 * j) % len(MU_BIASES)
    bmu = torch.tensor([MU_BIASES[i] for i in mi], dtype=torch.float32)
    bsig = torch.tensor([SIG_BIASES[i] for i in si], dtype=torch.float32)
    cols = {k: np.flatnonzero(np.array([SIG_KINDS[i] == k for i in si])) for k in set(SIG_KINDS)}
    cols["moderate"] = np.flatnonzero((bmu.abs().numpy() <= 2.0) & (bsig.numpy() >= -3.0) & (bsig.numpy() <= 1.0))
    cols["mu12"] = np.flatnonzero(bmu.abs().numpy() == 12.0)
    return bmu, bsig, cols


def edge_actor(actor: dict, bmu: torch.Tensor, bsig: torch.Tensor) -> dict:
    out = {k: v.clone() for k, v in actor.items()}
    out["wmu"].zero_()
    out["wsig"].zero_()
    out["bmu"], out["bsig"] = bmu.clone(), bsig.clone()
    return out


def zero_noise_row(B: int) -> int | None:
    """The row whose noise is all zero (none at B = 1: there `noise=None` plays the part)."""
    return B // 2 if B > 1 else None


def gaussian_case(obs_dim: int, act_dim: int, B: int, seed: int, hidden=64, shift: int = 0, tie: bool = False,
                  benign_only: bool = False) -> dict:
    """One SAC minibatch on an edge actor.  `tie`: critic 2 is a copy of critic 1, so Q1 == Q2 in every row."""
    actor, c1, c2 = OS.init_sac_params(obs_dim, act_dim, seed, hidden)
    bmu, bsig, cols = gaussian_columns(act_dim, shift, benign_only)
    if tie:
        c2 = {k: v.clone() for k, v in c1.items()}
    g = torch.Generator().manual_seed(1000 * seed + 10 * B + act_dim)
    noise = torch.randn(B, act_dim, generator=g)
    if zero_noise_row(B) is not None:
        noise[zero_noise_row(B)] = 0.0
    return dict(actor=edge_actor(actor, bmu, bsig), critic1=c1, critic2=c2, cols=cols, noise=noise,
                obs=torch.randn(B, obs_dim, generator=g), act=torch.rand(B, act_dim, generator=g) * 2 - 1,
                ret=torch.randn(B, generator=g) * 2, noise_next=torch.randn(B, act_dim, generator=g))


def opposed_tie_case(obs_dim: int, act_dim: int, B: int, seed: int, hidden=64) -> dict:
    """A bit-exact tie whose two sides pull in opposite directions.  bmu = 0 and all-zero noise make the squashed action exactly
    0.0 in every row; critic 2 is critic 1 with the action columns of its first layer negated.  0 * (+-w) adds +-0, so
    Q1 == Q2 bit for bit, but dQ2/da == -dQ1/da exactly, and 1 - tanh(0)^2 = 1 lets that gradient through to bmu.  The halves of
    torch.minimum's backward cancel (the bmu gradient is exactly the alpha * logp part: 0); a rule that hands the tie to one
    critic leaves -dQ1/da or +dQ1/da there.  The log-sigma biases are the edge columns of `gaussian_columns`."""
    case = gaussian_case(obs_dim, act_dim, B, seed, hidden)
    case["actor"]["bmu"] = torch.zeros(act_dim)
    case["noise"] = torch.zeros(B, act_dim)
    c2 = {k: v.clone() for k, v in case["critic1"].items()}
    c2["w1"][:, obs_dim:] = -c2["w1"][:, obs_dim:]
    case["critic2"] = c2
    return case


def sweep_case(obs_dim: int = 7, B: int = 4096, seed: int = 2, hidden=64) -> dict:
    """act_dim 1, mu 0.25, log sigma 3.0 -> clamped to sigma = e^2: N(0, 1) noise sweeps |a| from 0 to ~25, every row's log pi is
    one column's value."""
    actor, c1, c2 = OS.init_sac_params(obs_dim, 1, seed, hidden)
    g = torch.Generator().manual_seed(seed)
    return dict(actor=edge_actor(actor, torch.tensor([0.25]), torch.tensor([3.0])), critic1=c1, critic2=c2,
                obs=torch.randn(B, obs_dim, generator=g), noise=torch.randn(B, 1, generator=g))


def double(p: dict) -> dict:
    return {k: v.double() for k, v in p.items()}


def policy64(actor: dict, obs, noise, max_action: float = 0.0):
    """oracle_sac.policy_forward in float64 -> (squashed, log_prob [B], pre-tanh action a, sigma)."""
    sq, logp, mu, sigma = OS.policy_forward(double(actor), obs.double(), noise.double(), max_action)
    return sq, logp.flatten(), mu + noise.double() * sigma, sigma


def logp_condition(a64: torch.Tensor, logp64: torch.Tensor) -> torch.Tensor:
    """Per-row condition of log pi in float32: |log pi| + sum_j 1 / (1 - tanh(a_j)^2 + TANH_EPS).  One float32 ulp of tanh(a),
    relative to 1, moves log(1 - tanh^2 + eps) by that second term times eps32."""
    sq = torch.tanh(a64)
    return logp64.abs() + (1.0 / (1.0 - sq * sq + OS.TANH_EPS)).sum(-1)


def logp_ratio(logp, a64: torch.Tensor, logp64: torch.Tensor) -> torch.Tensor:
    """|logp - logp64| / (eps32 * condition), per row."""
    return (torch.as_tensor(logp).double().flatten() - logp64).abs() / (EPS32 * logp_condition(a64, logp64))


def logp_rounding(a64: torch.Tensor, noise, sigma64: torch.Tensor) -> torch.Tensor:
    """Per-row bound on what rounding a = mu + noise * sigma to float32 costs Normal.log_prob, absolute.  d = a - mu comes back
    as a multiple of ulp(a): off by at most r = eps32 / 2 * |a| from d64 = noise * sigma, and exactly 0 where |d64| is under
    half an ulp, so |d - d64| <= rr = min(r, |d64|) and d^2 / (2 sigma^2) moves by at most (2 |d64| rr + rr^2) / (2 sigma^2).
    Negligible where sigma is ordinary; up to 1.5 noise^2 in a column whose sigma = e^-20 sits under one ulp of mu, where
    float32 -- oracle and kernel alike -- rounds a back to mu."""
    d = (torch.as_tensor(noise).double() * sigma64).abs()
    rr = torch.minimum(0.5 * EPS32 * a64.abs(), d)
    return ((2.0 * d * rr + rr * rr) / (2.0 * sigma64 * sigma64)).sum(-1)


def band_counts(a64: torch.Tensor) -> list[int]:
    m = a64.abs().flatten()
    return [int(((m >= lo) & (m < hi)).sum()) for lo, hi in A_BANDS]


def mode_logp64(actor: dict, max_action: float = 0.0) -> tuple[torch.Tensor, torch.Tensor]:
    """Zero noise on an edge actor, written out: (tanh(mu) [A], -sum log sigma - A log sqrt(2 pi) - corr) in float64."""
    mu = actor["bmu"].double()
    if max_action > 0.0:
        mu = max_action * torch.tanh(mu)
    log_sigma = actor["bsig"].double().clamp(OS.SIGMA_MIN, OS.SIGMA_MAX)
    sq = torch.tanh(mu)
    corr = torch.log(1.0 - sq * sq + OS.TANH_EPS).sum()
    return sq, -log_sigma.sum() - mu.numel() * LOG_SQRT_2PI - corr


# ---- TD3 / DDPG ------------------------------------------------------------------------------------------------------
TD3_POLICY_NOISE, TD3_NOISE_CLIP = 0.25, 0.5           # powers of two: noise * policy_noise is exact in float32 and float64
# noise entries: exactly on +-clip, just inside, far outside, interior
TD3_NOISE_EDGES = (2.0, -2.0, _inward(2.0), _inward(-2.0), 40.0, -40.0, 0.0, 0.75, -1.5)
TD3_HEAD_BIASES = (12.0, -12.0, 0.0, 0.5, -2.0, 3.5)


def det_case(obs_dim: int, act_dim: int, B: int, seed: int, twin: bool, hidden=64) -> dict:
    """One TD3 / DDPG minibatch on an actor whose head is head[b, j] = TD3_HEAD_BIASES[j % 6]; the smoothing noise cycles through
    TD3_NOISE_EDGES along every fifth entry of the flattened [B, A] index, the rest is N(0, 1) * 3."""
    actor, c1, c2 = OS.init_td3_params(obs_dim, act_dim, seed, twin, hidden)
    actor = {k: v.clone() for k, v in actor.items()}
    actor["wa"].zero_()
    actor["ba"] = torch.tensor([TD3_HEAD_BIASES[j % len(TD3_HEAD_BIASES)] for j in range(act_dim)], dtype=torch.float32)
    g = torch.Generator().manual_seed(1000 * seed + 10 * B + act_dim)
    noise = (torch.randn(B * act_dim, generator=g) * 3.0)
    n_edge = len(TD3_NOISE_EDGES)
    idx = torch.arange(0, B * act_dim, 5)                  # every fifth entry is an edge value, in turn (5: every column gets some)
    noise[idx] = torch.tensor(TD3_NOISE_EDGES, dtype=torch.float32)[(idx // 5) % n_edge]
    cols = {"saturated": np.flatnonzero(actor["ba"].abs().numpy() == 12.0),
            "free": np.flatnonzero(actor["ba"].abs().numpy() < 12.0)}
    return dict(actor=actor, critic1=c1, critic2=c2, cols=cols, noise=noise.reshape(B, act_dim),
                obs=torch.randn(B, obs_dim, generator=g), act=torch.rand(B, act_dim, generator=g) * 2 - 1,
                ret=torch.randn(B, generator=g))


def td3_target64(case: dict, max_action: float, policy_noise: float, noise_clip: float, twin: bool) -> torch.Tensor:
    """oracle_sac.td3_target_q's arithmetic in float64 (the lagged networks equal the live ones at creation)."""
    with torch.no_grad():
        obs = case["obs"].double()
        act = OS.det_actor_forward(double(case["actor"]), obs, max_action)
        if not twin:
            return OS.critic_forward(double(case["critic1"]), obs, act).flatten()
        n = case["noise"].double() * policy_noise
        if noise_clip > 0.0:
            n = n.clamp(-noise_clip, noise_clip)
        act = act + n
        return torch.min(OS.critic_forward(double(case["critic1"]), obs, act),
                         OS.critic_forward(double(case["critic2"]), obs, act)).flatten()


# ---- DiscreteSAC -----------------------------------------------------------------------------------------------------
DSAC_PATTERNS = ("dominant", "underflow", "equal", "tied_max", "spread")


def dsac_case(obs_dim: int, n_act: int, B: int, seed: int, pattern: str, hidden=64) -> dict:
    """Actor and critics whose heads are constant rows (zero head weights):
      dominant   one logit 40 above the rest: p of the rest is e^-40
      underflow  one logit 120 above the rest: p of the rest underflows to 0 in float32 and p log p must be -0, not NaN
      equal      all logits equal: H = log n_act
      tied_max   two equal maxima, 5 above the rest
    and `spread`: the actor's head weights scaled by 60 instead, so that rows differ and the dominant action moves from row to
    row (a kernel that read its neighbour's row would show).  The Q heads are constant rows too, Q1 == Q2 in every third column
    and Q1 < Q2 / Q1 > Q2 in the others."""
    actor, c1, c2 = (dict(p) for p in ODS.init_params(obs_dim, n_act, hidden, seed))
    g = torch.Generator().manual_seed(1000 * seed + 10 * B + n_act)
    hot = (2 * n_act) // 3                                  # (lane 21 of 32, column 42 of 64: not the first, not the last)
    logits = torch.randn(n_act, generator=g) * 0.5
    if pattern == "dominant":
        logits[hot] = logits.max() + 40.0
    elif pattern == "underflow":
        logits[hot] = logits.max() + 120.0
    elif pattern == "equal":
        logits[:] = 1.25
    elif pattern == "tied_max":
        logits[hot] = logits[0] = logits.max() + 5.0
    if pattern == "spread":
        actor["head.w"] = actor["head.w"] * 60.0
    else:
        actor["head.w"] = torch.zeros_like(actor["head.w"])
        actor["head.b"] = logits
    q1 = torch.randn(n_act, generator=g) * 2.0
    q2 = q1 + torch.tensor([(0.0, 0.75, -0.5)[j % 3] for j in range(n_act)])
    for c, q in ((c1, q1), (c2, q2)):
        c["head.w"] = torch.zeros_like(c["head.w"])
        c["head.b"] = q.clone()
    return dict(actor=actor, critic1=c1, critic2=c2, obs=torch.randn(B, obs_dim, generator=g),
                act=torch.randint(0, n_act, (B,), generator=g), ret=torch.randn(B, generator=g) * 2)


def dsac64(case: dict, alpha: float) -> dict:
    """The float64 yardstick of DiscreteSAC's target value and actor step (oracle_dsac's arithmetic on float64 parameters):
    target [B], neg_ent [B] = -H, actor_loss, and the actor's gradients."""
    from torch.distributions import Categorical

    obs = case["obs"].double()
    p = {k: v.double().clone().requires_grad_(True) for k, v in case["actor"].items()}
    x = obs                                                 # (oracle_dsac.net_forward casts its input to float32: restated)
    i = 1
    while f"l{i}.w" in p:
        x = torch.relu(torch.nn.functional.linear(x, p[f"l{i}.w"], p[f"l{i}.b"]))
        i += 1
    dist = Categorical(logits=torch.nn.functional.linear(x, p["head.w"], p["head.b"]))
    q = torch.min(_const_q(case["critic1"], obs), _const_q(case["critic2"], obs))
    entropy = dist.entropy()
    f = alpha * entropy + (dist.probs * q).sum(-1)
    loss = -f.mean()
    grads = dict(zip(p.keys(), torch.autograd.grad(loss, list(p.values()))))
    return dict(target=f.detach(), neg_ent=-entropy.detach(), actor_loss=float(loss.detach()), actor_grads=grads)


def dsac_hidden(case: dict) -> torch.Tensor:
    """The actor trunk's last hidden activations [B, hidden] (the input of its head)."""
    x, p, i = case["obs"], case["actor"], 1
    while f"l{i}.w" in p:
        x = torch.relu(torch.nn.functional.linear(x, p[f"l{i}.w"], p[f"l{i}.b"]))
        i += 1
    return x


def _const_q(critic: dict, obs: torch.Tensor) -> torch.Tensor:
    assert not critic["head.w"].any()
    return critic["head.b"].double().expand(obs.shape[0], -1)
