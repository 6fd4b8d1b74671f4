"""Deterministic inputs, float64 references and route bookkeeping for REDQ (ts_redq_update / ts_redq_target_q of
tianshou_amd/csrc/ts_sac.hip) at the ensemble sizes, subset sizes, batch sizes and input widths where the engine changes path.
Shared by tests/test_redq_edge_inputs_cpu.py and the GPU tests of tests/test_gpu_redq_edges.py; nothing here touches the GPU path.

Cases.  `case(obs_dim, act_dim, B, E, hidden, seed, depth)` draws the actor and the ensemble from `oracle_redq.init_params`, a
`critic_old` that differs from `critic` by a perturbation of the order of the spread between members (every EnsembleLinear
tensor is U(-k, k): the perturbation is N(0, (max|v| / sqrt 3)^2), the standard deviation of that uniform), a batch and
non-uniform PER weights in (0.05, 1].  `copied_case` is the E = 11 ensemble whose members 5..9 are exact copies of 0..4 and whose member 10 is a
copy of member 0.  `subset(E, S)` is unsorted and always holds member E - 1 and member 0 (S = 1: member E - 1 alone).

Off the kink.  d relu / d x jumps at 0, so a hidden pre-activation whose sign float32 rounding decides has no reference
gradient: both masks are legitimate float32 results, and one flipped sample moves a row of dW by percents (seen: member 2 of the
E = 11 case held a layer-1 pre-activation of 6.5e-9 in float64; about 4e-6 of all pre-activations fall inside the band).  A
float32 dot product carries an error well below 32 eps32 times the sum of its absolute summands, so rows of the batch with a
pre-activation closer to 0 than that (`near_kink_rows`, float64, reference only) are redrawn.  The rule covers everything a
gradient flows through: the actor's trunk, and every member's trunk on the batch's actions and on the policy's.

References.  `update_reference` / `target_reference` evaluate `oracle_redq.critic_forward` and `oracle_sac.policy_forward` on
.double() tensors (both are dtype-agnostic): target_q, critic loss, per-member critic gradients and TD rows, the PER output
mean_e td_e, actor loss and actor gradient.  alpha is an input of both (float(exp(float32 log_alpha)), as the oracle forms it).

Bar.  For every quantity `e_ref` is the `rel_err` of the float32 oracle (`oracle_redq.update_with_batch` / `target_q`) against
the float64 reference on the same input, and the bar is rel_bar(e_ref) = max(1e-5, 2 e_ref) of the quantity's scale: 1e-5 is
the suite's own REDQ tolerance (tests/test_gpu_redq.py), the factor 2 over the reference's own float32 error the rule of
tests/test_gpu_iqn_routes.py.  e_ref comes from the reference alone, never from the engine; tests/test_redq_edge_inputs_cpu.py asserts
e_ref < 1e-3 for every case, so the 2 e_ref term is never a loophole.

Routes.  The constants below mirror the ones that decide the engine's path; `update_chunks` / `target_route` /
`forward_kernel` restate the decisions, so every GPU shape names the path it means to hit and the CPU test checks that it does.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import oracle_redq as OR
from oracle import oracle_sac as OS

# ---- the constants that decide the routes (file:line they were read from) -------------------------------------------------------
CHUNK = 5                   # ts_sac.hip:146   WGRADS_MAX_NETS: members per launch of the fused update (:2357-2358, :2403-2404)
MULTI_MAX = 8               # ts_mlp.h:22      MLP3_MAX_NETS: networks per multi-network launch (ts_sac.hip:108, :111, :2313)
FUSED_HIDDEN = 256          # ts_mlp.hip:45    HID; mlp3_supported (:407) wants hidden == HID
K1_STEP, K1_MIN, K1_MAX = 32, 32, 1024      # ts_mlp.hip:407   K1 % 32 == 0 && K1 >= 32 && K1 <= 1024
FUSED_DEPTH = 2             # ts_sac.hip:54    Mlp::three(): two ReLU hidden layers of one width
HP = FUSED_HIDDEN + 4       # ts_mlp.hip:46    LDS pitch of a hidden activation row
ROWS = 16                   # ts_mlp.hip:463   batch rows of a workgroup
LDS4_MAX = 80 * 1024        # ts_mlp.hip:475   four-wave workgroups for nets > 1 only while lds4 <= 80 KB
MAX_ENSEMBLE = 64           # ts_sac.hip:2341  E <= 64 (Act acts[64] :2371, loss_parts :2386); tianshou_amd/redq.py:93
LOSS_STRIDE = 1024          # ts_sac.hip:1149, :1157, :1192   batch stride of redq_critic_loss_kernel / redq_actor_loss_kernel


def pad32(x: int) -> int:
    return (x + 31) // 32 * 32


def kc_of(obs_dim: int, act_dim: int) -> int:
    """Critic input width: obs and action columns rounded up to 32 (make_dims_h, ts_sac.hip:1233)."""
    return pad32(obs_dim + act_dim)


def part_floats(nw: int, rows: int) -> int:
    """ts_mlp.hip:49."""
    return rows * (nw * 64 + 4 * nw)


def lds4_bytes(k1: int) -> int:
    """ts_mlp.hip:474: sizeof(float) * (ROWS (K1 + 4) + 2 ROWS HP + part_floats(4, ROWS)) = 64 K1 + 50944."""
    return 4 * (ROWS * (k1 + 4) + 2 * ROWS * HP + part_floats(4, ROWS))


# 64 K1 + 50944 <= 81920  <=>  K1 <= 484: the last K1 on the four-wave kernel is 480, the first on the eight-wave one 512
LDS4_LAST_K1 = max(k for k in range(K1_MIN, K1_MAX + 1, K1_STEP) if lds4_bytes(k) <= LDS4_MAX)


def fused_shape(hidden: int, kc: int, depth: int = 2) -> bool:
    """Mlp::three() && mlp3_supported (ts_sac.hip:54, ts_mlp.hip:407) for a 32-column critic head."""
    return depth == FUSED_DEPTH and hidden == FUSED_HIDDEN and kc % K1_STEP == 0 and K1_MIN <= kc <= K1_MAX


def forward_kernel(nets: int, k1: int) -> str:
    """mlp3_forward_nx (ts_mlp.hip:475): `four = nets > 1 && lds4 <= 80 KB`."""
    return "four-wave" if nets > 1 and lds4_bytes(k1) <= LDS4_MAX else "eight-wave"


def update_chunks(E: int, hidden: int, kc: int, depth: int = 2):
    """-> (route, chunk sizes) of the critic phase of ts_redq_update (ts_sac.hip:2355-2358, :2399-2433): "fused" = CHUNK
    members per launch, a chunk of 1 falling back to the single-network kernels inside mlp_forward_multi /
    mlp_backward_multi (:111, :217); "per-layer" = one member at a time, alternating between two streams."""
    if fused_shape(hidden, kc, depth):
        return "fused", [min(CHUNK, E - e0) for e0 in range(0, E, CHUNK)]
    return "per-layer", [1] * E


def target_route(S: int, hidden: int, kc: int, depth: int = 2):
    """-> (route, kernel) of ts_redq_target_q (ts_sac.hip:2313-2329): "single" / "multi" = one launch with blockIdx.y = subset
    position (S <= MULTI_MAX on a fused shape), "two-stream" = one member at a time on alternating streams -- on the fused
    single-network kernel for a fused shape, on the per-layer GEMMs otherwise."""
    fused = fused_shape(hidden, kc, depth)
    if fused and S <= MULTI_MAX:
        return ("single" if S == 1 else "multi"), forward_kernel(S, kc)
    return "two-stream", (forward_kernel(1, kc) if fused else "per-layer")


# ---- yardstick --------------------------------------------------------------------------------------------------------------------
def rel_err(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rel_bar(e_ref: float) -> float:
    return max(1e-5, 2.0 * float(e_ref))


def member_errs(t, g) -> np.ndarray:
    """Per-member rel_err of an ensemble tensor [E, ...]: every member's block on its own scale.  A tensor with ONE number per
    member (bq) is judged on the tensor's scale, max over the members, as tests/test_gpu_redq.py judges it: that number is
    2 / (E B) sum_b w_b td_b, a sum that cancels (float32 oracle against float64: up to 1.7e-5 of a member's own value)."""
    t, g = np.asarray(t, np.float64), np.asarray(g, np.float64)
    E = g.shape[0]
    if g[0].size == 1:
        return np.abs(t - g).reshape(E) / max(np.abs(g).max(), 1e-30)
    return np.array([rel_err(t[m], g[m]) for m in range(E)])


LOG_ALPHA0, FIXED_ALPHA = -0.3, 0.15


def hidden_spec(hidden: int, depth: int):
    """`hidden` argument of oracle_redq.init_params: an int for Net[h, h], a nested pair for any other depth."""
    return int(hidden) if depth == 2 else ([int(hidden)] * depth, [int(hidden)] * depth)


def oracle_cfg(c: dict, auto_alpha: bool = True, max_action: float = 0.0, **kw) -> OR.REDQConfig:
    """Gradient-only configuration (learning rates and tau 0, actor step in every update) unless overridden."""
    base = dict(auto_alpha=auto_alpha, log_alpha0=LOG_ALPHA0, alpha=FIXED_ALPHA, target_entropy=-float(c["act_dim"]), actor_lr=0.0,
                critic_lr=0.0, alpha_lr=0.0, tau=0.0, ensemble_size=c["E"], subset_size=min(2, c["E"]), actor_delay=1,
                max_action=max_action)
    base.update(kw)
    return OR.REDQConfig(**base)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
EPS32 = float(np.finfo(np.float32).eps)
KINK_MARGIN = 32.0 * EPS32


def _layers(p: dict, ensemble: bool):
    """Hidden layers as (w [E, in, out], b [E, 1, out]) in float64."""
    out = []
    for i in range(1, OS.depth_of(p) + 1):
        w, b = p[f"w{i}"].double(), p[f"b{i}"].double()
        out.append((w, b) if ensemble else (w.t()[None], b[None, None]))
    return out


def near_kink_rows(actor: dict, critic: dict, obs, act, noise) -> torch.Tensor:
    """Rows b with a hidden pre-activation whose SIGN float32 rounding may decide: |pre| < KINK_MARGIN * (sum_k |x_k w_kj| + |b_j|) in
    float64, for the actor's trunk on obs and for every member's trunk on (obs, act) and on (obs, pi(obs)) -- see `case`."""
    obs, act, noise = obs.double(), act.double(), noise.double()
    with torch.no_grad():
        pi = OS.policy_forward({k: v.double() for k, v in actor.items()}, obs, noise)[0]
    bad = torch.zeros(obs.shape[0], dtype=torch.bool)
    for layers, x in ((_layers(actor, False), obs), (_layers(critic, True), torch.cat([obs, act], 1)), (_layers(critic, True), torch.cat([obs, pi], 1))):
        h = x
        for w, b in layers:
            pre, size = torch.matmul(h, w) + b, torch.matmul(h.abs(), w.abs()) + b.abs()
            bad |= (pre.abs() < KINK_MARGIN * size).any(dim=2).any(dim=0)
            h = torch.relu(pre)
    return bad


def _finish_case(obs_dim, act_dim, B, E, hidden, seed, depth, actor, critic) -> dict:
    g = torch.Generator().manual_seed(1000 + seed)
    critic_old = {k: v + (float(v.abs().max()) / np.sqrt(3.0)) * torch.randn(v.shape, generator=g) for k, v in critic.items()}
    obs = torch.randn(B, obs_dim, generator=g)
    act = torch.rand(B, act_dim, generator=g) * 2 - 1
    ret, noise = torch.randn(B, generator=g) * 2, torch.randn(B, act_dim, generator=g)
    w = 1.0 - 0.95 * torch.rand(B, generator=g)                          # PER weights in (0.05, 1], non-uniform; B = 1: not 1
    for _ in range(200):                                                 # rows off the ReLU kink (module docstring)
        bad = near_kink_rows(actor, critic, obs, act, noise)
        n = int(bad.sum())
        if n == 0:
            break
        obs[bad], act[bad] = torch.randn(n, obs_dim, generator=g), torch.rand(n, act_dim, generator=g) * 2 - 1
        noise[bad] = torch.randn(n, act_dim, generator=g)
    else:
        raise AssertionError("no batch off the ReLU kink found")
    return dict(obs_dim=obs_dim, act_dim=act_dim, B=B, E=E, hidden=hidden, depth=depth, seed=seed, kc=kc_of(obs_dim, act_dim),
                actor=actor, critic=critic, critic_old=critic_old, obs=obs, act=act, ret=ret, noise=noise, weight=w)


@functools.lru_cache(maxsize=None)
def case(obs_dim: int, act_dim: int, B: int, E: int, hidden: int = 256, seed: int = 0, depth: int = 2) -> dict:
    actor, critic = OR.init_params(obs_dim, act_dim, E, seed, hidden_spec(hidden, depth))
    return _finish_case(obs_dim, act_dim, B, E, hidden, seed, depth, actor, critic)


COPIED_E = 11
COPIED = dict(obs_dim=5, act_dim=2, B=33, hidden=256, seed=21)


@functools.lru_cache(maxsize=None)
def copied_case() -> dict:
    """E = 11 = chunks [5, 5, 1]: members 5..9 are exact copies of 0..4 (same launch shape, same position in the launch), member 10
    a copy of member 0 (the single-network kernels)."""
    s = COPIED
    actor, five = OR.init_params(s["obs_dim"], s["act_dim"], CHUNK, s["seed"], s["hidden"])
    critic = {k: torch.cat([v, v, v[:1]]).contiguous() for k, v in five.items()}
    assert all(v.shape[0] == COPIED_E for v in critic.values())
    return _finish_case(s["obs_dim"], s["act_dim"], s["B"], COPIED_E, s["hidden"], s["seed"], 2, actor, critic)


def subset(E: int, S: int, seed: int = 0) -> np.ndarray:
    """S distinct members, unsorted, holding member E - 1 (first) and member 0 (last); the others in random order between."""
    assert 1 <= S <= E
    if S == 1:
        return np.array([E - 1], dtype=np.int64)
    mid = np.random.default_rng(seed).permutation(np.arange(1, E - 1))[:S - 2]
    return np.concatenate([[E - 1], mid, [0]]).astype(np.int64)


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def _alpha(c: dict, auto_alpha: bool) -> float:
    return float(torch.tensor(LOG_ALPHA0).exp().item()) if auto_alpha else FIXED_ALPHA


def _d(p: dict, grad: bool = False) -> dict:
    return {k: v.double().clone().requires_grad_(grad) for k, v in p.items()}


def compute_update_reference(c: dict, weighted: bool = True, auto_alpha: bool = True) -> dict:
    """One update with every learning rate 0 and the actor step: float64 values, the float32 oracle's values and its e_ref.
    Keys of e_ref: "critic_loss", "weight", "actor_loss", ("critic", key) -> float[E] (per member), ("actor", key)."""
    E = c["E"]
    obs, act, ret, noise = (c[k].double() for k in ("obs", "act", "ret", "noise"))
    w = c["weight"].double() if weighted else torch.ones(c["B"], dtype=torch.float64)
    alpha = _alpha(c, auto_alpha)
    p = _d(c["critic"], True)
    td = OR.critic_forward(p, obs, act).flatten(1) - ret
    loss = (td.pow(2) * w).mean()
    cg = dict(zip(p.keys(), torch.autograd.grad(loss, list(p.values()))))
    pa = _d(c["actor"], True)
    a, logp, _, _ = OS.policy_forward(pa, obs, noise)
    qa = OR.critic_forward(_d(c["critic"]), obs, a).mean(dim=0).flatten()
    aloss = (alpha * logp.flatten() - qa).mean()
    ag = dict(zip(pa.keys(), torch.autograd.grad(aloss, list(pa.values()))))
    out = dict(critic_loss=float(loss.detach()), unweighted_loss=float(td.detach().pow(2).mean()), td=td.detach(),
               weight=td.detach().mean(dim=0), critic_grads=cg, actor_loss=float(aloss.detach()), actor_grads=ag, alpha=alpha)
    # the float32 oracle on the same input
    cfg = oracle_cfg(c, auto_alpha)
    st = OR.REDQState.create(c["actor"], c["critic"], cfg)
    col: dict = {}
    o = OR.update_with_batch(st, cfg, c["obs"], c["act"], c["ret"], c["noise"], c["weight"] if weighted else None, collect=col)
    e = {"critic_loss": abs(o["critic_loss"] - out["critic_loss"]) / abs(out["critic_loss"]),
         "actor_loss": abs(o["actor_loss"] - out["actor_loss"]) / abs(out["actor_loss"]),
         "weight": rel_err(o["weight"], out["weight"])}
    for k, g in cg.items():
        e[("critic", k)] = member_errs(col["critic_grads"][k], g)
    for k, g in ag.items():
        e[("actor", k)] = rel_err(col["actor_grads"][k], g)
    out["e_ref"], out["oracle"] = e, dict(o, critic_grads=col["critic_grads"], actor_grads=col["actor_grads"])
    return out


@functools.lru_cache(maxsize=None)
def update_reference(shape: tuple, weighted: bool = True, auto_alpha: bool = True) -> dict:
    return compute_update_reference(case(*shape), weighted, auto_alpha)


@functools.lru_cache(maxsize=None)
def copied_reference(weighted: bool = True) -> dict:
    return compute_update_reference(copied_case(), weighted, True)


def worst_e_ref(ref: dict) -> float:
    return max(float(np.max(v)) for v in ref["e_ref"].values())


@functools.lru_cache(maxsize=None)
def target_reference(shape: tuple, S: int, mode: str, max_action: float = 0.0, auto_alpha: bool = True) -> dict:
    """target_q of the case's `critic_old` on (obs, noise) for `subset(E, S)`: float64 value, the per-member Q it was reduced
    from, the other reductions a wrong kernel could return (mean for min and the reverse, the LIVE critics) and e_ref."""
    c = case(*shape)
    sub = subset(c["E"], S, seed=c["seed"])
    obs, noise = c["obs"].double(), c["noise"].double()
    alpha = _alpha(c, auto_alpha)
    with torch.no_grad():
        a, logp, _, _ = OS.policy_forward(_d(c["actor"]), obs, noise, max_action)
        q_old = OR.critic_forward(_d(c["critic_old"]), obs, a)[:, :, 0]                    # [E, B]
        q_live = OR.critic_forward(_d(c["critic"]), obs, a)[:, :, 0]
        ent = alpha * logp.flatten()
    red = (lambda q: q.min(dim=0)[0]) if mode == "min" else (lambda q: q.mean(dim=0))
    cfg = oracle_cfg(c, auto_alpha, max_action, subset_size=S, target_mode=mode)
    st = OR.REDQState.create(c["actor"], c["critic"], cfg)
    st.critic_old = {k: v.clone() for k, v in c["critic_old"].items()}
    tq32 = OR.target_q(st, cfg, c["obs"], c["noise"], sub).flatten()
    tq = red(q_old[sub]) - ent
    return dict(subset=sub, tq=tq, q_sub=q_old[sub], tq_min=q_old[sub].min(dim=0)[0] - ent, tq_mean=q_old[sub].mean(dim=0) - ent,
                tq_live=red(q_live[sub]) - ent, tq_all=red(q_old) - ent, e_ref=rel_err(tq32, tq), alpha=alpha)


# ---- the shapes of tests/test_gpu_redq_edges.py, each with the path it means to hit ------------------------------------------------
# shape = (obs_dim, act_dim, B, E, hidden, seed, depth); obs_dim = 5, act_dim = 2 gives kc = 32
def shape(E, B=33, hidden=256, obs_dim=5, act_dim=2, depth=2, seed=None):
    return (obs_dim, act_dim, B, E, hidden, (100 * E + B + hidden + depth) if seed is None else seed, depth)


# (tag, shape, route, chunks) -- chunks spelled out where the fused route is meant
CHUNK_SHAPES = [("E6", shape(6), "fused", [5, 1]), ("E7", shape(7), "fused", [5, 2]), ("E10", shape(10), "fused", [5, 5]),
                ("E11", shape(11), "fused", [5, 5, 1])]
LIMIT_SHAPE = ("E64", shape(64, B=8), "fused", [5] * 12 + [4])
SINGLE_SHAPES = [("E1 fused", shape(1), "fused", [1]), ("E1 per-layer", shape(1, hidden=64), "per-layer", [1])]
PER_LAYER_SHAPES = [(f"E7 depth {d}", shape(7, hidden=64, depth=d), "per-layer", [1] * 7) for d in (2, 3, 1)]
BATCH_SIZES = (1, 1023, 1025, 2049)
BATCH_SHAPES = [(f"B{b} hidden {h}", shape(6, B=b, hidden=h), "fused" if h == 256 else "per-layer", [5, 1] if h == 256 else [1] * 6)
                for h in (256, 64) for b in BATCH_SIZES]
# the actor phase's input-gradient columns [obs_dim, obs_dim + act_dim): [30, 33) straddles column 32, [15, 47) is the widest
ACTION_SHAPES = [("act [30, 33)", shape(6, obs_dim=30, act_dim=3), "fused", [5, 1]),
                 ("act [15, 47)", shape(6, obs_dim=15, act_dim=32), "fused", [5, 1])]
WIDE_FUSED = ("kc 1024", shape(6, B=17, obs_dim=1000, act_dim=24), "fused", [5, 1])
WIDE_PER_LAYER = ("kc 1056", shape(6, B=17, obs_dim=1001, act_dim=24), "per-layer", [1] * 6)
STEP_SHAPE = ("delay 3", shape(6, seed=77), "fused", [5, 1])
COPIED_SHAPE = ("copied E11", (COPIED["obs_dim"], COPIED["act_dim"], COPIED["B"], COPIED_E, COPIED["hidden"], COPIED["seed"], 2), "fused",
                [5, 5, 1])
UPDATE_SHAPES = CHUNK_SHAPES + [LIMIT_SHAPE] + SINGLE_SHAPES + PER_LAYER_SHAPES + BATCH_SHAPES + ACTION_SHAPES \
    + [WIDE_FUSED, WIDE_PER_LAYER, STEP_SHAPE]

# (shape, S, mode, max_action); E = 10 on both routes at B = 1 and 300, and E = 1 with S = 1.  The path each (S, hidden) means to hit:
TARGET_ROUTES_MEANT = {(1, 256): ("single", "eight-wave"), (8, 256): ("multi", "four-wave"), (9, 256): ("two-stream", "eight-wave"),
                       (10, 256): ("two-stream", "eight-wave"), (9, 64): ("two-stream", "per-layer"), (10, 64): ("two-stream", "per-layer"),
                       (1, 64): ("two-stream", "per-layer")}
# The B = 300 seeds are the first of a search over seeds 300.. for which, in the float64 reference alone, every subset member is the
# arg-min of some row by a clear margin at every S used (most seeds leave one member above the others on every row).
_T256 = {1: shape(10, B=1, seed=301), 300: shape(10, B=300, seed=319)}
_T64 = {1: shape(10, B=1, hidden=64, seed=365), 300: shape(10, B=300, hidden=64, seed=464)}
TARGET_CASES = [(_T256[b], s, mode, 0.0) for b in (1, 300) for s in (1, 8, 9, 10) for mode in ("min", "mean")] \
    + [(_T64[b], s, mode, 0.0) for b in (1, 300) for s in (9, 10) for mode in ("min", "mean")] \
    + [(_T256[300], 8, "min", 1.5), (_T64[300], 9, "min", 1.5)] \
    + [(shape(1, B=300, hidden=h, seed=41 + h), 1, mode, 0.0) for h in (256, 64) for mode in ("min", "mean")]


def update_variants():
    """(tag, shape, weighted, auto_alpha) of every gradient comparison of the GPU file: every shape with PER weights and
    auto alpha, the chunk shapes also without weights and with a fixed alpha.  (STEP_SHAPE runs against the oracle's steps.)"""
    for tag, shp, _, _ in UPDATE_SHAPES:
        if tag != STEP_SHAPE[0]:
            yield tag, shp, True, True
    for tag, shp, _, _ in CHUNK_SHAPES:
        yield tag + " unweighted", shp, False, False
