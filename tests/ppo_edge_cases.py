"""Edge inputs for the PPO / A2C loss-and-head kernels, their float64 references and the bars the GPU tests hold them to.
Shared by tests/test_ppo_edge_inputs_cpu.py (no GPU), tests/test_gpu_ppo_edges.py and tests/test_gpu_ppo_discrete_edges.py.

The loss is written out by hand in seven places (ts_ppo.hip net_fwd_bwd, ts_ppo_q.h, ts_npg.hip ppo_wide_actor_loss_kernel /
ppo_wide_critic_loss_kernel and ppo_net_actor_loss_cs_kernel, ts_ppo_cnn.hip cnn_ppo_loss_kernel, ts_mlp_small.hip, and the A2C
branch of each).  Every copy restates torch's rules: torch.min backward (`surr1 <= surr2 ? A : 0`), the dual clip only where
A < 0, clamp backward on the CLOSED interval, torch.max backward splitting the gradient on ties, the Categorical entropy and the
tanh bound (MulBackward, then TanhBackward).

Construction
  * Edge networks: an ordinary random trunk, the last layer's WEIGHTS zero.  mu (or the logits), the conditioned log sigma
    columns and V then equal their biases for every row, exactly, whatever the observation; nothing flows below the head, so
    every trunk block's gradient is exactly zero, the head bias gradient is the column sum of the kernel's d_head and the head
    weight gradient its outer product with the trunk output.
  * Dyadic hyper-parameters (eps_clip 0.25, dual_clip 2, vf_coef 0.5, ent_coef 2^-7, max_action 1 or 2): float32 and float64
    agree on every boundary.
  * Homogeneous batches: every row of a batch sits in ONE branch class, only magnitudes vary, so a wrong branch moves the
    result by O(1) instead of hiding in a sum.  Rows differ in obs, act, adv, logp_old, v_s and returns only.
  * The ratio is placed through logp_old = float32(logp64 - log r); the realised ratio is recomputed in float64 from the
    rounded value (`surrogate64`), so the reference never assumes r.
  * References are closed forms per row in float64 (numpy), torch's tie and clamp rules written out.  They do not reuse
    oracle_ppo.ppo_minibatch_loss: that casts the ratio to float32, right for an oracle and wrong for a truth.

Bar (`reference`): per loss figure and per element of a gradient block
        |gpu - ref64| <= 4 * err32 + 4 * eps32 * scale
  err32 is the float32 oracle's own error on the same inputs (oracle_ppo / oracle_ppo_cnn.minibatch_loss with torch autograd),
  4 the margin the SAC and distributional edge suites gave a differently ordered float32 evaluation, and `scale` the block's
  largest sum of |terms| (an entry is a sum over the rows; a float32 sum carries the rounding of its terms, not of its possibly
  cancelled result).  A block whose terms are all exactly zero has bar 0.
  Two terms come on top, both from the precision of float32 and both written down before they are used:
  * The conditioning of the ratio.  ratio = exp(logp - logp_old), and logp is a float32 sum of terms of total size L (per row:
    sum_j d^2 / (2 var) + |log sigma| + log sqrt(2 pi); Categorical: |l_a| + |lse|).  Each term passes through up to four
    roundings of half an ulp (d * d, the factor 1 / (2 var) and its own exp, the running sum), so NO float32 evaluation knows
    logp better than 2 eps32 L, nor anything the ratio multiplies better than that relatively.  err32 is one realisation of
    this error, and a lucky one says nothing about another order of evaluation: with L ~ 3600 (|act - mu| / sigma = 30,
    8 actions) the oracle happened to land within 5e-5 of float64 and the fused kernels, which multiply by a precomputed
    1 / (2 var), within 2e-4.  So every figure the ratio multiplies gets 2 eps32 * sum_b L_b |term_b| on top (PPO objective
    only).  Under the plain bar 12 of 40 GPU tests failed on an MI355X, all on rows with L >= 20 (z = 30, sigma = e^-20,
    ratio 1e30 at A = 1e4), none by a branch: the largest |gpu - ref64| was 6.9 x the plain bar.
  * The bounded fused kernel (ts_ppo.hip BOUNDED) takes t = tanh(raw) from fast_tanh, documented absolute error 2.4e-7:
    `reference(..., tanh_abs=FAST_TANH_ABS)` adds the first-order effect of that error (`tanh_slack`) there and nowhere else.

Known and deliberately not tested: at clip1 == dual_clip * A exactly torch halves the gradient and the kernels pass it whole
(that needs exp() to land on dual_clip bit for bit and cannot be constructed portably); a ratio that overflows to inf gives NaN
in torch and in the kernels alike.  Categorical(probs=softmax(.)) (DiscreteActor(softmax_output=True)) clamps probabilities to
[eps, 1 - eps] before the logarithm, so for logits dominated by more than ~16 it is a different distribution from
Categorical(logits=.); the kernels implement the latter and so do these references.

err32 itself is held to reasoning, not to a guess (`pin_units`): the ratio is exp(logp - logp_old), so the float32 rounding of
logp -- a sum of terms of total size L -- reaches every actor figure L-fold; tests/test_ppo_edge_inputs_cpu.py asserts
err32 <= (8 + 4 L) eps32 * scale on every case and prints the measured table (`pytest -s`)."""
import numpy as np
import torch

from oracle import oracle_ppo as OP
from oracle import oracle_ppo_cnn as OC
from oracle import oracle_ppo_discrete as OD

EPS32 = float(np.finfo(np.float32).eps)
EPS_CLIP, DUAL_CLIP, VF_COEF, ENT_COEF = 0.25, 2.0, 0.5, 2.0 ** -7
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
CS_MIN, CS_MAX = -20.0, 2.0
FLT_MIN = float(np.finfo(np.float32).tiny)   # below it float32 loses bits (or flushes to zero): no relative claim holds there
FAST_TANH_ABS = 2.5e-7           # ts_ppo.hip fast_tanh: |error| <= 2.4e-7
ROW_COUNTS = (33, 257, 1)        # a partial tile, more than one block / several tiles, a single row
RATIO_MARGIN = 1e-4              # realised ratios keep this relative distance from 1 +- eps and dual_clip


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def hyper(**kw):
    base = dict(algo="ppo", eps_clip=EPS_CLIP, dual_clip=None, value_clip=True, advantage_normalization=False, vf_coef=VF_COEF,
                ent_coef=ENT_COEF, max_grad_norm=None, lr=1e-3)
    base.update(kw)
    if base["algo"] == "a2c":           # a2c.py:262-273 has neither value clip nor advantage normalisation nor dual clip
        base.update(value_clip=False, advantage_normalization=False, dual_clip=None)
    return base


# ---- float64 closed forms -------------------------------------------------------------------------------------------------
def normalised_adv64(adv, hp):
    a = np.asarray(adv, np.float64)
    if hp["advantage_normalization"] and hp["algo"] == "ppo":              # ppo.py:184-186 (unbiased std)
        return (a - a.mean()) / (a.std(ddof=1) + 1e-8)
    return a


def surrogate64(logp, rows, hp):
    """-> term [B] (clip_loss = mean), dlogp [B] = d loss / d logp_b (the 1 / B included), ratio [B] or None, normalised adv."""
    B = len(logp)
    A = normalised_adv64(rows["adv"], hp)
    if hp["algo"] == "a2c":
        return -logp * A, -A / B, None, A
    e = hp["eps_clip"]
    ratio = np.exp(logp - rows["logp_old"].astype(np.float64))
    s1, s2 = ratio * A, np.clip(ratio, 1.0 - e, 1.0 + e) * A
    clip1 = np.minimum(s1, s2)
    base = np.where(s1 <= s2, A, 0.0)                                      # torch.min backward; a tie is the same value twice
    term = -clip1
    if hp["dual_clip"]:
        dA = hp["dual_clip"] * A
        neg = A < 0
        term = -np.where(neg, np.maximum(clip1, dA), clip1)                # only where A < 0
        base = np.where(neg & (clip1 < dA), 0.0, base)
    return term, -base * ratio / B, ratio, A


def value64(V, rows, hp):
    """-> vterm [B] (vf_loss = mean), d_v [B] = d loss / d V_b (vf_coef / B included), branch class [B] in {1, 2, 0 = tie}."""
    r, B = rows["returns"].astype(np.float64), len(rows["returns"])
    vf1, g1 = (r - V) ** 2, -2.0 * (r - V)
    if not (hp["value_clip"] and hp["algo"] == "ppo"):
        return vf1, g1 * hp["vf_coef"] / B, np.ones(B, int)
    e, vo = hp["eps_clip"], rows["v_s"].astype(np.float64)
    dvo = V - vo
    vclip = vo + np.clip(dvo, -e, e)
    vf2 = (r - vclip) ** 2
    g2 = np.where((dvo >= -e) & (dvo <= e), -2.0 * (r - vclip), 0.0)       # clamp backward: the closed interval passes
    dv = np.where(vf1 > vf2, g1, np.where(vf2 > vf1, g2, 0.5 * (g1 + g2)))   # torch.max backward: ties split
    return np.maximum(vf1, vf2), dv * hp["vf_coef"] / B, np.where(vf1 > vf2, 1, np.where(vf2 > vf1, 2, 0))


def gauss_logp64(head, act):
    raw, lsr = head["raw"].astype(np.float64), head["ls"].astype(np.float64)
    M = head.get("max_action")
    mu = M * np.tanh(raw) if M else raw
    ls = np.clip(lsr, CS_MIN, CS_MAX) if head.get("cs") else lsr
    d = np.asarray(act, np.float64) - mu[None, :]
    return (-(d * d) / (2.0 * np.exp(2.0 * ls)) - ls - HALF_LOG_2PI).sum(1), d, ls, mu


def gauss_ref64(head, rows, hp):
    """Diagonal Gaussian head (Independent(Normal(mu, sigma), 1)); head = dict(raw [A], ls [A], v, max_action, cs).
    -> losses [4], d_mu [B, A] (w.r.t. the RAW head output), d_ls [B, A], d_v [B], ratio, adv, vclass."""
    B = len(rows["adv"])
    logp, d, ls, _ = gauss_logp64(head, rows["act"])
    var = np.exp(2.0 * ls)
    term, dlogp, ratio, A = surrogate64(logp, rows, hp)
    d_mu = dlogp[:, None] * d / var
    M = head.get("max_action")
    if M:                                                                  # MulBackward, then TanhBackward: 1 - t^2 = sech^2
        raw = head["raw"].astype(np.float64)
        d_mu = d_mu * M * (1.0 / np.cosh(raw) ** 2)[None, :]
    d_ls = dlogp[:, None] * (d * d / var - 1.0) - hp["ent_coef"] / B       # entropy: d / d log sigma = 1
    if head.get("cs"):                                                     # clamp backward: the closed interval passes
        lsr = head["ls"].astype(np.float64)
        d_ls = d_ls * ((lsr >= CS_MIN) & (lsr <= CS_MAX))[None, :]
    ent = float((0.5 + HALF_LOG_2PI + ls).sum())
    vterm, d_v, vclass = value64(float(head["v"]), rows, hp)
    clip, vf = term.mean(), vterm.mean()
    losses = np.array([clip + hp["vf_coef"] * vf - hp["ent_coef"] * ent, clip, vf, ent])
    tsize = np.abs(term)
    if hp["algo"] == "a2c":              # -logp * A: logp is added up from terms that may cancel
        tsize = np.abs(A) * (d * d / (2.0 * var) + np.abs(ls)[None, :] + HALF_LOG_2PI).sum(1)
    esize = float((0.5 + HALF_LOG_2PI + np.abs(ls)).sum())
    lscale = np.array([tsize.mean() + hp["vf_coef"] * np.abs(vterm).mean() + hp["ent_coef"] * esize, tsize.mean(), np.abs(vterm).mean(), esize])
    mag_mu = np.abs(d_mu)
    if M:                                # 1 - t * t cancels as |t| -> 1
        mag_mu = np.abs(dlogp[:, None] * d / var) * M * (1.0 + np.tanh(raw) ** 2)[None, :]
    mag_ls = np.abs(dlogp)[:, None] * (d * d / var + 1.0) + hp["ent_coef"] / B         # d^2 / var - 1 cancels at |z| = 1
    if head.get("cs"):
        mag_ls = mag_ls * ((lsr >= CS_MIN) & (lsr <= CS_MAX))[None, :]
    amp = max(1.0, float((np.abs(d) / var).max()), float((d * d / var).max()))        # what multiplies d loss / d logp at most
    return dict(losses=losses, loss_scale=lscale, d_mu=d_mu, d_ls=d_ls, d_v=d_v, ratio=ratio, adv=A, vclass=vclass, logp=logp,
                d=d, var=var, dlogp=dlogp, term=term, mag_ls=mag_ls, mag_mu=mag_mu, amp=amp,
                L=(d * d / (2.0 * var) + np.abs(ls)[None, :] + HALF_LOG_2PI).sum(1), mag_ls_r=np.abs(dlogp)[:, None] * (d * d / var + 1.0))


def tanh_slack(ref, head, hp, dt):
    """First-order effect of an absolute error dt in t = tanh(raw) (fast_tanh, ts_ppo.hip) on a bounded actor's figures:
    1 - t^2 moves by 2 |t| dt, d = act - M t by M dt, and logp (hence the ratio, which multiplies every actor gradient of the
    PPO objective) by sum_j |d_j| / var_j M dt.  -> (slack of d_mu [B, A], of d_ls [B, A], of the clip loss)."""
    M = head["max_action"]
    raw = head["raw"].astype(np.float64)
    sech2, t = 1.0 / np.cosh(raw) ** 2, np.abs(np.tanh(raw))
    d, var, dlogp = np.abs(ref["d"]), ref["var"], np.abs(ref["dlogp"])[:, None]
    dlp = (d / var).sum(1)[:, None] * M * dt                                # |delta logp| per row
    ppo = 0.0 if hp["algo"] == "a2c" else 1.0                              # A2C: d loss / d logp does not depend on logp
    s_mu = dlogp * d / var * M * (2.0 * t * dt)[None, :] + dlogp / var * (M * M * sech2 * dt)[None, :] + ppo * np.abs(ref["d_mu"]) * dlp
    s_ls = dlogp * 2.0 * d * M * dt / var + ppo * dlogp * np.abs(d * d / var - 1.0) * dlp
    s_clip = float((np.abs(ref["term"]) * dlp[:, 0]).mean()) if ppo else float((np.abs(ref["adv"]) * dlp[:, 0]).mean())
    return s_mu, s_ls, s_clip


def cat_ref64(head, rows, hp):
    """Categorical(logits); head = dict(logits [A], v).  -> losses [4], d_logit [B, A], d_v [B], ..."""
    lg = head["logits"].astype(np.float64)
    B, act = len(rows["adv"]), np.asarray(rows["act"], np.int64)
    m = lg.max()
    lp = lg - (m + np.log(np.exp(lg - m).sum()))
    p = np.exp(lp)
    H = float(-(p * lp).sum())                                             # Categorical.entropy; p == 0 contributes 0
    term, dlogp, ratio, A = surrogate64(lp[act], rows, hp)
    onehot = np.zeros((B, len(lg)))
    onehot[np.arange(B), act] = 1.0
    d_logit = dlogp[:, None] * (onehot - p[None, :]) + (hp["ent_coef"] / B) * (p * (lp + H))[None, :]      # - ent_coef dH / dl
    # sizes of what is added up: 1 - p cancels on a dominant column, and lp = l - lse carries the rounding of l and lse
    lp_size = np.abs(lg) + abs(m + np.log(np.exp(lg - m).sum()))
    h_size = float((p * lp_size).sum())
    mag = np.abs(dlogp)[:, None] * (onehot + p[None, :]) + (hp["ent_coef"] / B) * (p * (lp_size + h_size))[None, :]
    vterm, d_v, vclass = value64(float(head["v"]), rows, hp)
    clip, vf = term.mean(), vterm.mean()
    losses = np.array([clip + hp["vf_coef"] * vf - hp["ent_coef"] * H, clip, vf, H])
    tsize = np.abs(A) * lp_size[act] if hp["algo"] == "a2c" else np.abs(term)      # -logp * A: logp = l - lse may cancel
    lscale = np.array([tsize.mean() + hp["vf_coef"] * np.abs(vterm).mean() + hp["ent_coef"] * h_size, tsize.mean(), np.abs(vterm).mean(), h_size])
    return dict(losses=losses, loss_scale=lscale, d_logit=d_logit, d_v=d_v, ratio=ratio, adv=A, vclass=vclass, logp=lp[act], p=p, H=H,
                dlogp=dlogp, term=term, mag=mag, amp=1.0, L=lp_size[act], mag_r=np.abs(dlogp)[:, None] * (onehot + p[None, :]))


def block64(d, h, mag=None):
    """Head gradient blocks of the per-row head gradient d [B, C] and the float64 trunk output h [B, H]:
    bias = column sums, weight [C, H] = outer products, and the largest sum of |terms| of each (mag: the size of what a
    row's entry is added up from, where that is more than |d|)."""
    mag = np.abs(d) if mag is None else mag
    return dict(b=d.sum(0), w=d.T @ h, b_scale=float(mag.sum(0).max()), w_scale=float((mag.T @ np.abs(h)).max()))


# ---- edge networks --------------------------------------------------------------------------------------------------------
# kind -> (obs_dim, hidden of both trunks, trunk activation): the fused step kernels' envelope (hidden 64), the smallest
# width tests/test_gpu_ppo_wide.py uses, the same for the per-layer engine, the CartPole-shape network
KINDS = {"fused": (11, 64, "tanh"), "wide": (5, 32, "tanh"), "net": (5, 32, "tanh"), "net_cs": (5, 32, "tanh"), "discrete": (6, 64, "relu")}
_PARAMS: dict = {}


def gauss_params(kind, head):
    """oracle_ppo parameter dict (+ a_wsig / a_bsig for conditioned sigma): random trunks, zero head weights, the head's biases."""
    obs_dim, hidden, _ = KINDS[kind]
    A = len(head["raw"])
    key = (kind, A)
    if key not in _PARAMS:
        p = OP.init_params(obs_dim, A, hidden=hidden, seed=7 + A)
        g = torch.Generator().manual_seed(70 + A)
        for k in ("a_b1", "a_b2", "c_b1", "c_b2"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
        _PARAMS[key] = p
    p = {k: v.clone() for k, v in _PARAMS[key].items()}
    p["a_wmu"], p["c_wv"] = torch.zeros_like(p["a_wmu"]), torch.zeros_like(p["c_wv"])
    p["a_bmu"], p["c_bv"] = torch.from_numpy(f32(head["raw"])), torch.from_numpy(f32([head["v"]]))
    if head.get("cs"):
        p["a_sigma"] = torch.zeros(A)
        p["a_wsig"], p["a_bsig"] = torch.zeros_like(p["a_wmu"]), torch.from_numpy(f32(head["ls"]))
    else:
        p["a_sigma"] = torch.from_numpy(f32(head["ls"]))
    return p


def cat_params(head):
    obs_dim, hidden, _ = KINDS["discrete"]
    A = len(head["logits"])
    key = ("discrete", A)
    if key not in _PARAMS:
        p = OD.init_params(obs_dim, hidden, A, 11 + A)
        g = torch.Generator().manual_seed(110 + A)
        for k in ("l1.b", "l2.b"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
        _PARAMS[key] = p
    p = {k: v.clone() for k, v in _PARAMS[key].items()}
    p["actor.w"], p["critic.w"] = torch.zeros_like(p["actor.w"]), torch.zeros_like(p["critic.w"])
    p["actor.b"], p["critic.b"] = torch.from_numpy(f32(head["logits"])), torch.from_numpy(f32([head["v"]]))
    return p


def obs_batch(kind, B, seed):
    return f32(np.random.default_rng(1000 + seed).normal(size=(B, KINDS[kind][0])))


def trunk64(kind, w1, b1, w2, b2, obs):
    fn = np.tanh if KINDS[kind][2] == "tanh" else (lambda x: np.maximum(x, 0.0))
    d = lambda t: t.detach().numpy().astype(np.float64)                    # noqa: E731
    return fn(fn(obs.astype(np.float64) @ d(w1).T + d(b1)) @ d(w2).T + d(b2))


# ---- float32 oracles (torch autograd) --------------------------------------------------------------------------------------
def _cs_actor_forward(p, obs, max_action=None):
    """ContinuousActorProbabilistic(conditioned_sigma=True) (continuous.py:212-234): sigma = clamp(Linear(h), -20, 2).exp()."""
    h = OP._trunk(obs, p["a_w1"], p["a_b1"], p["a_w2"], p["a_b2"])
    mu = torch.nn.functional.linear(h, p["a_wmu"], p["a_bmu"])
    if max_action is not None:
        mu = max_action * torch.tanh(mu)
    return mu, torch.clamp(torch.nn.functional.linear(h, p["a_wsig"], p["a_bsig"]), min=CS_MIN, max=CS_MAX).exp()


def gauss_oracle32(p, head, rows, obs, hp):
    """oracle_ppo.ppo_minibatch_loss / a2c_minibatch_loss + backward on the edge network -> (losses [4], grads dict)."""
    cfg = OP.PPOConfig(max_action=head.get("max_action"), **hp)
    pg = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rows.items()}
    saved = OP.actor_forward
    if head.get("cs"):
        OP.actor_forward = _cs_actor_forward         # the oracle's loss on the conditioned-sigma actor (restored below)
    try:
        if hp["algo"] == "a2c":
            out = OP.a2c_minibatch_loss(pg, cfg, torch.from_numpy(obs), t["act"], t["adv"], t["returns"])
        else:
            out = OP.ppo_minibatch_loss(pg, cfg, torch.from_numpy(obs), t["act"], t["adv"], t["returns"], t["logp_old"], t["v_s"])
        out[0].backward()
    finally:
        OP.actor_forward = saved
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for k, v in pg.items()}
    return np.array([float(x.detach()) for x in out]), grads


def cat_oracle32(p, rows, obs, hp):
    cfg = OP.PPOConfig(**hp)
    pg = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rows.items()}
    out = OC.minibatch_loss(pg, cfg, torch.from_numpy(obs), t["act"], t["adv"], t["returns"], t["logp_old"], t["v_s"],
                            net=OD.MlpNet(softmax_output=False))
    out[0].backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for k, v in pg.items()}
    return np.array([float(x.detach()) for x in out]), grads


GAUSS_TRUNK = ("a_w1", "a_b1", "a_w2", "a_b2", "c_w1", "c_b1", "c_w2", "c_b2")
CAT_TRUNK = ("l1.w", "l1.b", "l2.w", "l2.b")


def reference(kind, case, tanh_abs=0.0):
    """-> dict(params, obs, losses, blocks {name: float64 array}, bars {name: array}, scales, err32 {name: array}, trunk names,
    ref (the per-row closed forms)).  Block names are the oracle's parameter names; "losses" is held to bars["losses"]."""
    head, rows, hp = case["head"], case["rows"], case["hp"]
    B = len(rows["adv"])
    obs = obs_batch(kind, B, case.get("seed", 0))
    if kind == "discrete":
        p = cat_params(head)
        ref = cat_ref64(head, rows, hp)
        h = trunk64(kind, p["l1.w"], p["l1.b"], p["l2.w"], p["l2.b"], obs)
        ba, bc = block64(ref["d_logit"], h, ref["mag"]), block64(ref["d_v"][:, None], h)
        blocks = {"actor.b": ba["b"], "actor.w": ba["w"], "critic.b": bc["b"], "critic.w": bc["w"]}
        scales = {"actor.b": ba["b_scale"], "actor.w": ba["w_scale"], "critic.b": bc["b_scale"], "critic.w": bc["w_scale"]}
        l32, g32 = cat_oracle32(p, rows, obs, hp)
        trunk = CAT_TRUNK
    else:
        p = gauss_params(kind, head)
        ref = gauss_ref64(head, rows, hp)
        ha = trunk64(kind, p["a_w1"], p["a_b1"], p["a_w2"], p["a_b2"], obs)
        hc = trunk64(kind, p["c_w1"], p["c_b1"], p["c_w2"], p["c_b2"], obs)
        bm, bs, bv = block64(ref["d_mu"], ha, ref["mag_mu"]), block64(ref["d_ls"], ha, ref["mag_ls"]), block64(ref["d_v"][:, None], hc)
        blocks = {"a_bmu": bm["b"], "a_wmu": bm["w"], "c_bv": bv["b"], "c_wv": bv["w"]}
        scales = {"a_bmu": bm["b_scale"], "a_wmu": bm["w_scale"], "c_bv": bv["b_scale"], "c_wv": bv["w_scale"]}
        if head.get("cs"):
            blocks.update({"a_bsig": bs["b"], "a_wsig": bs["w"]})
            scales.update({"a_bsig": bs["b_scale"], "a_wsig": bs["w_scale"]})
        else:
            blocks["a_sigma"], scales["a_sigma"] = bs["b"], bs["b_scale"]
        l32, g32 = gauss_oracle32(p, head, rows, obs, hp)
        trunk = GAUSS_TRUNK
    err32 = {k: np.abs(g32[k].reshape(v.shape) - v) for k, v in blocks.items()}
    # (a block with any term gets 4 FLT_MIN per row, times what the term was multiplied by, on top: products like
    # ratio * A = 1e-30 * 1e-30 leave float32's range, and nothing relative can be asked of what remains)
    floor = 4.0 * FLT_MIN * B * ref["amp"]
    bars = {k: 4.0 * err32[k] + 4.0 * EPS32 * scales[k] + (floor if scales[k] > 0 else 0.0) for k in blocks}
    err32["losses"] = np.abs(l32 - ref["losses"])
    bars["losses"] = 4.0 * err32["losses"] + 4.0 * EPS32 * ref["loss_scale"] + np.where(ref["loss_scale"] > 0, floor, 0.0)
    if hp["algo"] == "ppo":              # the conditioning of the ratio (module docstring): 2 eps32 L_b on everything it multiplies
        cond = (2.0 * EPS32 * ref["L"])[:, None]
        if kind == "discrete":
            bars["actor.b"] = bars["actor.b"] + (cond * ref["mag_r"]).sum(0)
            bars["actor.w"] = bars["actor.w"] + (cond * ref["mag_r"]).T @ np.abs(h)
        else:
            sig = ("a_bsig", "a_wsig") if head.get("cs") else ("a_sigma", None)
            bars["a_bmu"] = bars["a_bmu"] + (cond * ref["mag_mu"]).sum(0)
            bars["a_wmu"] = bars["a_wmu"] + (cond * ref["mag_mu"]).T @ np.abs(ha)
            passes = (ref["mag_ls"] > 0)
            bars[sig[0]] = bars[sig[0]] + (cond * ref["mag_ls_r"] * passes).sum(0)
            if sig[1]:
                bars[sig[1]] = bars[sig[1]] + (cond * ref["mag_ls_r"] * passes).T @ np.abs(ha)
        c = float((cond[:, 0] * np.abs(ref["term"])).mean())
        bars["losses"] = bars["losses"] + np.array([c, c, 0.0, 0.0])
    if tanh_abs and head.get("max_action"):
        s_mu, s_ls, s_clip = tanh_slack(ref, head, hp, tanh_abs)
        bars["a_bmu"] = bars["a_bmu"] + s_mu.sum(0)
        bars["a_wmu"] = bars["a_wmu"] + s_mu.T @ np.abs(ha)
        bars["a_sigma"] = bars["a_sigma"] + s_ls.sum(0)
        bars["losses"] = bars["losses"] + np.array([s_clip, s_clip, 0.0, 0.0])
    scales["losses"] = ref["loss_scale"]
    return dict(params=p, obs=obs, losses=ref["losses"], blocks=blocks, bars=bars, scales=scales, err32=err32, trunk=trunk,
                trunk_grads32={k: g32[k] for k in trunk}, ref=ref, oracle_losses=l32, floor=floor)


def err32_units(r):
    """err32 / (eps32 * scale) per quantity (0 where the scale is 0 and the oracle is exact)."""
    out = {}
    for k, e in r["err32"].items():
        s = np.asarray(r["scales"][k], np.float64)
        assert np.all((s > 0) | (e == 0)), k
        out[k] = float((np.maximum(e - r["floor"], 0.0) / np.where(s > 0, EPS32 * s, 1.0)).max())
    return out


def pin_units(case, ref):
    """How far (in eps32 * scale) the float32 oracle may sit from float64: 8 for its sums and products, plus 4 per unit of
    L = the size of the terms that make up logp - logp_old (each rounded once or twice before exp() spreads the error over
    every actor figure); a bounded actor adds tanh's half-ulp through d logp / d t."""
    rows, head = case["rows"], case["head"]
    L = np.abs(rows["logp_old"].astype(np.float64))
    if "logits" in head:
        L = L + np.abs(ref["logp"]) + float(np.abs(head["logits"]).max())
    else:
        ls = np.abs(np.clip(head["ls"].astype(np.float64), CS_MIN, CS_MAX))
        L = L + (ref["d"] ** 2 / (2.0 * ref["var"]) + ls[None, :] + HALF_LOG_2PI).sum(1)
        if head.get("max_action"):       # ... and through 1 - t * t, which cancels as |t| -> 1 (saturated: exactly 0 on both sides)
            L = L + (np.abs(ref["d"]) / ref["var"]).sum(1) * head["max_action"]
            raw = head["raw"].astype(np.float64)
            sech2 = 1.0 / np.cosh(raw) ** 2
            L = L + float(np.where(sech2 > 1e-15, np.abs(np.tanh(raw)) / np.maximum(sech2, 1e-300), 0.0).max())
    return 8.0 + 4.0 * float(L.max())


def check(got_losses, got_blocks, r, worst=None, what=""):
    """Every loss figure and every element of every head block within its bar of float64.  `worst` collects the largest
    |got - ref64| / (eps32 * scale) per quantity (what the module docstrings quote)."""
    got = dict(got_blocks, losses=np.asarray(got_losses, np.float64))
    for k, bar in r["bars"].items():
        ref = r["losses"] if k == "losses" else r["blocks"][k]
        g = np.asarray(got[k], np.float64).reshape(ref.shape)
        assert np.all(np.isfinite(g)), (what, k)
        diff = np.abs(g - ref)
        s = np.asarray(r["scales"][k], np.float64)
        if worst is not None:
            u = float((np.maximum(diff - r["floor"], 0.0) / np.where(s > 0, EPS32 * s, 1.0)).max()) if np.all((s > 0) | (diff == 0)) else float("inf")
            worst[k] = max(worst.get(k, 0.0), u)
        assert np.all(diff <= bar), (what, k, float(diff.max()), float(np.max(diff - bar)), g.ravel()[:4], ref.ravel()[:4])


# ---- rows -----------------------------------------------------------------------------------------------------------------
ADV_CLASSES = ("pos", "neg", "zero", "tiny_pos", "tiny_neg", "big_pos", "big_neg")
# ratio class -> target ratio; "in" classes pass the gradient, the others depend on the advantage's sign
RATIO_CLASSES = {"inside": 1.0625, "hi_in": 1.25 * (1 - 1e-3), "hi_out": 1.25 * (1 + 1e-3), "lo_in": 0.75 * (1 + 1e-3),
                 "lo_out": 0.75 * (1 - 1e-3), "dual_in": 2.0 * (1 - 1e-3), "dual_out": 2.0 * (1 + 1e-3), "far_hi": 8.0, "far_lo": 1e-3,
                 "huge": 1e30, "minute": 1e-30}


def adv_rows(cls, B, rng):
    u = rng.uniform(0.1, 3.0, size=B)
    return f32({"pos": u, "neg": -u, "zero": 0.0 * u, "tiny_pos": 1e-30 * (1 + u), "tiny_neg": -1e-30 * (1 + u), "big_pos": 1e4 * u / 3,
                "big_neg": -1e4 * u / 3, "mixed": u * np.where(rng.random(B) < 0.5, -1.0, 1.0), "const": 0.75 + 0.0 * u}[cls])


def value_rows(cls, B, V, rng):
    """v_s, returns on the grid of multiples of 1/64 (every float32 operation of the value loss is then exact), by class."""
    e = EPS_CLIP
    k = rng.integers(-15, 16, size=B) / 64.0                     # |k| < eps
    j = rng.integers(1, 129, size=B) / 64.0                      # in (0, 2]
    sgn = np.where(rng.random(B) < 0.5, -1.0, 1.0)
    far = e + rng.integers(1, 65, size=B) / 64.0                 # beyond the clamp by 1/64 .. 1
    ulp = np.float32(np.spacing(np.float32(e)))
    if cls == "inside_tie":          # v_clip == V exactly: vf1 == vf2, 0.5 (g1 + g2) = the full gradient
        v_s, ret = V - k, V + sgn * j
    elif cls == "inside_rounded":    # arbitrary float32: v_s + (V - v_s) is V up to rounding, either branch may win
        v_s, ret = V - rng.uniform(-0.2, 0.2, size=B), V + rng.normal(size=B)
    elif cls == "at_plus_eps":       # V - v_s == +eps: the closed interval passes -> tie, full gradient
        v_s, ret = V - e + 0.0 * k, V + sgn * j
    elif cls == "at_minus_eps":
        v_s, ret = V + e + 0.0 * k, V + sgn * j
    elif cls == "ulp_beyond_vf2":    # V = 0: V - v_s = eps + 1 ulp, v_clip = -ulp; returns > 0: vf2 > vf1, clamp blocks -> exactly 0
        assert V == 0.0
        v_s, ret = -(np.float32(e) + ulp) + 0.0 * k, rng.integers(1, 17, size=B) / 64.0
    elif cls == "ulp_beyond_vf1":    # ... returns < 0: vf1 > vf2 -> g1
        assert V == 0.0
        v_s, ret = -(np.float32(e) + ulp) + 0.0 * k, -rng.integers(1, 17, size=B) / 64.0
    elif cls == "far_vf1":           # v_s = V - far: v_clip = V - far + eps < V; returns below both, farther from V -> g1
        v_s, ret = V - far, V - far - j
    elif cls == "far_vf2":           # returns above V: farther from v_clip -> g2 = 0 (outside the clamp): exactly 0
        v_s, ret = V - far, V + j
    elif cls == "far_neg_vf2":       # the other side: v_s = V + far, v_clip = V + far - eps > V, returns below V -> exactly 0
        v_s, ret = V + far, V - j
    elif cls == "clamped_tie":       # returns half way between V and v_clip: vf1 == vf2 with the clamp active -> 0.5 g1
        v_s = V - sgn * far
        ret = V + 0.5 * ((v_s + sgn * e) - V)
    else:
        raise KeyError(cls)
    return f32(v_s), f32(ret)


VALUE_CLASSES = ("inside_tie", "inside_rounded", "at_plus_eps", "at_minus_eps", "ulp_beyond_vf2", "ulp_beyond_vf1", "far_vf1", "far_vf2",
                 "far_neg_vf2", "clamped_tie")
VALUE_EXACT_ZERO = ("ulp_beyond_vf2", "far_vf2", "far_neg_vf2")       # d loss / d V is exactly 0 for every row
VALUE_EXPECT = {"inside_tie": 0, "at_plus_eps": 0, "at_minus_eps": 0, "ulp_beyond_vf2": 2, "ulp_beyond_vf1": 1, "far_vf1": 1, "far_vf2": 2,
                "far_neg_vf2": 2, "clamped_tie": 0}


def gauss_head(A, ls=-0.5, raw=None, v=0.5, max_action=None, cs=False, seed=0):
    rng = np.random.default_rng(300 + seed + A)
    raw = rng.uniform(-0.5, 0.5, size=A) if raw is None else np.broadcast_to(np.asarray(raw, np.float64), (A,))
    return dict(raw=f32(raw), ls=f32(np.broadcast_to(np.asarray(ls, np.float64), (A,))), v=np.float32(v), max_action=max_action, cs=cs)


def gauss_case(name, head, B, hp, ratio=1.0625, adv="pos", value="inside_tie", z_max=2.0, z=None, seed=0):
    """One homogeneous batch: act = mu + sigma z, logp_old = float32(logp64 - log ratio), adv / (v_s, returns) of one class."""
    rng = np.random.default_rng(seed)
    A = len(head["raw"])
    _, _, ls, mu = gauss_logp64(head, np.zeros((1, A)))
    zz = rng.uniform(-z_max, z_max, size=(B, A)) if z is None else np.broadcast_to(np.asarray(z, np.float64), (B, A))
    act = f32(mu[None, :] + np.exp(ls)[None, :] * zz)                   # z == 0 and an unbounded actor: act == mu bit for bit
    logp = gauss_logp64(head, act)[0]
    v_s, ret = value_rows(value, B, float(head["v"]), rng)
    rows = dict(act=act, adv=adv_rows(adv, B, rng), logp_old=f32(logp - np.log(ratio)), v_s=v_s, returns=ret)
    return dict(name=name, head=head, rows=rows, hp=hp, seed=seed, ratio_class=ratio, adv_class=adv, value_class=value)


def cat_head(logits, v=0.5):
    return dict(logits=f32(logits), v=np.float32(v))


def cat_case(name, head, B, hp, ratio=1.0625, adv="pos", value="inside_tie", act=None, seed=0):
    rng = np.random.default_rng(seed)
    A = len(head["logits"])
    a = rng.integers(0, A, size=B) if act is None else np.full(B, act)
    lg = head["logits"].astype(np.float64)
    lp = lg - (lg.max() + np.log(np.exp(lg - lg.max()).sum()))
    v_s, ret = value_rows(value, B, float(head["v"]), rng)
    rows = dict(act=a.astype(np.int64), adv=adv_rows(adv, B, rng), logp_old=f32(lp[a] - np.log(ratio)), v_s=v_s, returns=ret)
    return dict(name=name, head=head, rows=rows, hp=hp, seed=seed, ratio_class=ratio, adv_class=adv, value_class=value)


def _cycle(i):
    return ROW_COUNTS[i % len(ROW_COUNTS)]


HP_VARIANTS = {"dual_off": hyper(), "dual_on": hyper(dual_clip=DUAL_CLIP), "a2c": hyper(algo="a2c")}


def ratio_cases(make, variant):
    """ratio class x advantage class, each its own batch; row counts cycle through ROW_COUNTS.  make(name, B, hp, ratio=, adv=, seed=)."""
    hp = HP_VARIANTS[variant]
    out, i = [], 0
    for rc, r in RATIO_CLASSES.items():
        if variant == "a2c" and rc not in ("inside", "far_hi"):     # A2C has no ratio: logp_old is ignored, two placements do
            continue
        for ac in ADV_CLASSES:
            out.append(make(f"{variant}/{rc}/{ac}/B{_cycle(i)}", _cycle(i), hp, ratio=r, adv=ac, seed=i))
            i += 1
    return out


def advnorm_cases(make):
    """An ordinary minibatch and a constant one (std 0: every normalised advantage is 0, only entropy and value gradients remain)."""
    out = []
    for i, (adv, B) in enumerate((("mixed", 33), ("mixed", 257), ("const", 33), ("const", 257))):
        for variant in ("dual_off", "dual_on"):
            hp = dict(HP_VARIANTS[variant], advantage_normalization=True)
            out.append(make(f"advnorm/{variant}/{adv}/B{B}", B, hp, ratio=1.0625 if adv == "const" else 1.5, adv=adv, seed=50 + i))
    return out


def value_cases(make):
    out = []
    for i, vc in enumerate(VALUE_CLASSES):
        B = _cycle(i)
        out.append(make(f"value/{vc}/B{B}", B, HP_VARIANTS["dual_off"], value=vc, adv="mixed", seed=80 + i))
    return out


def fused_make(A, **head_kw):
    def make(name, B, hp, value="inside_tie", **kw):
        v = 0.0 if value.startswith("ulp_beyond") else 0.5
        return gauss_case(name, gauss_head(A, v=v, **head_kw), B, hp, value=value, **kw)
    return make


def gauss_head_cases(act_dims, cs=False):
    """log sigma in {-5, 0, 2}, act == mu exactly, |act - mu| / sigma graded up to 30, every action count."""
    out, i = [], 0
    for A in act_dims:
        for ls in (-5.0, 0.0, 2.0):
            head = gauss_head(A, ls=ls, cs=cs)
            for zname, kw in (("act_eq_mu", dict(z=0.0)), ("z30", dict(z_max=30.0)), ("z2", dict())):
                for variant, ratio, adv in (("dual_off", 1.0625, "pos"), ("dual_on", 1.5, "neg"), ("a2c", 1.0, "mixed")):
                    B = _cycle(i)
                    out.append(gauss_case(f"gauss/A{A}/ls{ls:g}/{zname}/{variant}/B{B}", head, B, HP_VARIANTS[variant], ratio=ratio,
                                          adv=adv, seed=200 + i, **kw))
                    i += 1
    return out


BOUNDED_RAW = (0.0, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 20.0, -20.0)


def bounded_cases(A, cs=False):
    """Raw head bias in {0, +-0.5, +-3, +-6, +-20} with max_action 1 and 2; act inside (z small) and outside +-max_action."""
    out, i = [], 0
    for M in (1.0, 2.0):
        for raw in BOUNDED_RAW:
            head = gauss_head(A, raw=raw, ls=-0.5, max_action=M, cs=cs)
            for where, z in (("inside", None), ("outside", 6.0 * (-1.0 if raw > 0 else 1.0))):
                for variant, ratio, adv in (("dual_off", 1.0625, "pos"), ("a2c", 1.0, "neg")):
                    B = _cycle(i)
                    kw = dict(z_max=0.25) if z is None else dict(z=z)
                    out.append(gauss_case(f"bounded/M{M:g}/raw{raw:g}/{where}/{variant}/B{B}", head, B, HP_VARIANTS[variant], ratio=ratio,
                                          adv=adv, seed=400 + i, **kw))
                    i += 1
    return out


def cs_clamp_cases(A):
    """Conditioned sigma: the bias at -20 and at 2 exactly (the gradient passes), 1 ulp beyond each (the sigma-column gradient is
    exactly 0 and the entropy uses the clamped value), far beyond, and mid-range."""
    lo, hi = np.float32(CS_MIN), np.float32(CS_MAX)
    vals = {"at_min": lo, "at_max": hi, "ulp_below_min": np.nextafter(lo, np.float32(-np.inf)), "ulp_above_max": np.nextafter(hi, np.float32(np.inf)),
            "far_below": np.float32(-50.0), "far_above": np.float32(7.0), "mid": np.float32(-1.0),
            "ulp_inside_min": np.nextafter(lo, np.float32(0)), "ulp_inside_max": np.nextafter(hi, np.float32(0))}
    out, i = [], 0
    for name, ls in vals.items():
        head = gauss_head(A, ls=float(ls), cs=True)
        for variant, ratio, adv in (("dual_off", 1.0625, "pos"), ("dual_on", 1.5, "neg"), ("a2c", 1.0, "mixed")):
            B = _cycle(i)
            # (at log sigma -20 a z of 2 is an action within 4e-9 of mu: float32 keeps it, the placement only needs logp64)
            out.append(gauss_case(f"cs/{name}/{variant}/B{B}", head, B, HP_VARIANTS[variant], ratio=ratio, adv=adv, seed=600 + i))
            i += 1
    return out


CS_BLOCKED = ("ulp_below_min", "ulp_above_max", "far_below", "far_above")


def cat_logits(pattern, A, hot=0):
    lg = np.zeros(A)
    if pattern == "equal":
        lg[:] = 0.375
    elif pattern.startswith("dom"):
        lg[:] = -0.25
        lg[hot] = -0.25 + float(pattern[3:])
    elif pattern == "graded":
        lg = -1.5 * np.arange(A) + 0.5
    else:
        raise KeyError(pattern)
    return lg


CAT_SIZES = (1, 2, 18, 31)
CAT_PATTERNS = ("equal", "dom20", "dom90", "dom10000", "graded")


def cat_cases(group):
    """Categorical batches by group: "ratio_<variant>", "advnorm", "value", "logits", "logits_dom1e4" (the 1e4-dominated rows on
    their own: float32 resolves such a logit to 1e-3, so the multi-step comparison of the one-launch update with the per-step
    path holds only while both add the bias to the finished sum)."""
    make = lambda name, B, hp, **kw: cat_case(name, cat_head(cat_logits("graded", 6) * 0.3), B, hp, **kw)     # noqa: E731
    if group.startswith("ratio_"):
        return ratio_cases(make, group[6:])
    if group == "advnorm":
        return advnorm_cases(make)
    if group == "value":
        def vmake(name, B, hp, value="inside_tie", **kw):
            v = 0.0 if value.startswith("ulp_beyond") else 0.5
            return cat_case(name, cat_head(cat_logits("graded", 6) * 0.3, v=v), B, hp, value=value, **kw)
        return value_cases(vmake)
    assert group in ("logits", "logits_dom1e4")
    out, i = [], 0
    for A in CAT_SIZES:
        for pat in CAT_PATTERNS:
            if (A == 1 and pat != "equal") or (pat == "dom10000") != (group == "logits_dom1e4"):
                continue
            hot = A // 2
            head = cat_head(cat_logits(pat, A, hot))
            acts = [("hot", hot), ("cold", (hot + 1) % A)] if pat.startswith("dom") else [("any", None)]
            for aname, a in acts:
                for variant, ratio, adv in (("dual_off", 1.0625, "pos"), ("dual_on", 1.5, "neg"), ("a2c", 1.0, "mixed")):
                    B = _cycle(i)
                    out.append(cat_case(f"logits/A{A}/{pat}/act_{aname}/{variant}/B{B}", head, B, HP_VARIANTS[variant], ratio=ratio, adv=adv,
                                        act=a, seed=800 + i))
                    i += 1
    return out


GAUSS_GROUPS = ("ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value", "gauss_head")


def gauss_cases(group, A, cs=False):
    make = fused_make(A, cs=cs)
    if group.startswith("ratio_"):
        return ratio_cases(make, group[6:])
    if group == "advnorm":
        return advnorm_cases(make)
    if group == "value":
        return value_cases(make)
    raise KeyError(group)


def ratio_margin(case, ref):
    """Smallest relative distance of a realised ratio from 1 - eps, 1 + eps and dual_clip (inf for A2C)."""
    if ref["ratio"] is None:
        return float("inf")
    bounds = [1.0 - EPS_CLIP, 1.0 + EPS_CLIP] + ([DUAL_CLIP] if case["hp"]["dual_clip"] else [])
    return float(min(np.abs(ref["ratio"] / b - 1.0).min() for b in bounds))


def exact_zero_blocks(kind, case):
    """Head blocks whose every entry must be exactly 0.0 (either sign) for this case."""
    name, head = case["name"], case["head"]
    out = []
    if case["value_class"] in VALUE_EXACT_ZERO:                          # the clamp blocks the larger branch
        out += ["critic.b", "critic.w"] if kind == "discrete" else ["c_bv", "c_wv"]
    if kind == "discrete":
        if len(head["logits"]) == 1:                                     # one action: p = 1, logp = 0, entropy 0
            out += ["actor.b", "actor.w"]
        return out
    mu = ["a_bmu", "a_wmu"]
    if case["adv_class"] in ("zero", "const") and case["hp"]["algo"] == "ppo":      # a Gaussian's entropy does not depend on mu
        out += mu
    elif case["adv_class"] == "zero":
        out += mu
    if "/act_eq_mu/" in name and not head.get("max_action"):              # d = act - mu = 0
        out += mu
    if head.get("max_action") and abs(float(head["raw"][0])) >= 20.0:     # saturated bound: 1 - t * t = 0
        out += mu
    if head.get("cs") and name.split("/")[1] in CS_BLOCKED:               # beyond the sigma clamp
        out += ["a_bsig", "a_wsig"]
    return sorted(set(out))
