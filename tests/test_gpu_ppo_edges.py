"""The Gaussian PPO / A2C loss-and-head kernels at their clip, clamp and tie edges, one homogeneous batch per edge
(tests/ppo_edge_cases.py states the construction, the float64 references and the bar; tests/test_ppo_edge_inputs_cpu.py checks
the preconditions without a GPU):

  copy 1   ts_ppo.hip net_fwd_bwd (128-sample step kernel; BOUNDED variant)      PPOEngine._run_steps, TS_PPO_STEPQ=0
  copy 2   ts_ppo_q.h (feature-split step kernel, 128- / 168-register builds)    PPOEngine._run_steps, TS_PPO_STEPQ=1 / 2
  copy 3   ts_npg.hip ppo_wide_actor_loss_kernel + ppo_wide_critic_loss_kernel   WidePPOEngine.step; with the tanh bound:
                                                                                 NetPPOEngine.step (WidePPOEngine takes no bound)
  copy 4   ts_npg.hip ppo_net_actor_loss_cs_kernel (conditioned sigma)           NetPPOEngine(conditioned_sigma=True).step
  copy 7   the A2C branch of each: the "ratio_a2c" group and the a2c cases of the others

CnnPPOEngine launches the same loss kernel as DiscretePPOEngine.step (tests/test_gpu_ppo_discrete_edges.py) and needs 84 x 84
inputs: it is left out.  A bounded actor always runs copy 1 (the feature-split kernel has no bounded build), so the bounded
group runs under TS_PPO_STEPQ=0 only.

Bar: |gpu - ref64| <= 4 err32 + 4 eps32 * scale per loss figure and per element of every head block, err32 being the float32
oracle's own error on the same inputs, plus 2 eps32 L relative on what the ratio multiplies (L = the size of the terms logp is
added up from; the shared module's docstring derives it); the fused kernels' bounded actor adds the first-order effect of
fast_tanh's documented 2.5e-7 (E.tanh_slack).  Exact: every trunk block is 0.0 (zero head weights stop the back-propagation), padding entries are 0.0,
and the blocks E.exact_zero_blocks names (saturated bound, beyond the sigma clamp, blocked value clamp, zero / constant
advantages, act == mu) are 0.0.

Measured on an MI355X, worst |gpu - ref64| / (eps32 * scale) over all cases:
  (ratio / advnorm / value groups: L <= 20; gauss_head: L up to 3600; bounded, cs_clamp: L up to ~120)
                         losses   mu bias  mu weight  sigma    V bias  V weight
  copy 1  ratio..value    7.1      9.2      10.6       3.9      0.7     4.1
          gauss_head      846      461      617        975      0.4     3.7      (A = 8; 77 / 105 / 86 / 128 at A = 1)
          bounded         309       62       63        290      0.2     3.9      (fast_tanh; copy 3's tanhf: 39 / 31 / 32 / 37)
  copy 2  ratio..value    6.6     10.8      13.3       4.1      0.4     3.8      (both register builds give the same figures)
          gauss_head      652      400      673        908      0.4     3.4
  copy 3  ratio..value    5.2      6.4       7.5       1.5      0.3     2.3
          gauss_head       94      113      159        113      0.2     1.8      (A = 3)
          bounded          39       31       32         37      0.3     2.2
  copy 4  ratio..value    5.2      6.4       7.5       2.5      0.3     2.3      (sigma = the head's sigma columns, bias / weight)
          gauss_head       94      113      159        112      0.2     1.8
          cs_clamp         69       60       48         47      0.2     1.5
The float32 oracle's own figures on the same cases (tests/test_ppo_edge_inputs_cpu.py) are 5.8 / 11.1 / 12.7 / 4.1 on the ratio
groups and 257 / 238 / 399 / 384 on gauss_head at A = 8: the kernels sit where a float32 evaluation sits, and the fused
kernels' precomputed 1 / (2 var) costs about a factor 2.5 at L = 3600.  No copy took a wrong branch on any case."""
import numpy as np
import pytest
import torch

from oracle import oracle_ppo as OP
from tests import ppo_edge_cases as E

pytestmark = pytest.mark.gpu
SENTINEL = 7.0          # grad_out is pre-filled: an entry the engine must write cannot pass by luck


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def batch(case, r):
    rows = case["rows"]
    return dict(obs=dev(r["obs"]), act=dev(rows["act"]), adv=dev(rows["adv"]), returns=dev(rows["returns"]), logp_old=dev(rows["logp_old"]),
                v_s=dev(rows["v_s"]))


def engine_cfg(case):
    from tianshou_amd import ppo as P

    return P.PPOConfig(max_action=case["head"].get("max_action"), **case["hp"])


def verify(kind, case, r, losses, named, worst):
    """The bars on the losses and the head blocks; exact zeros on the trunk and on the blocks the case's class empties."""
    what = f"{kind} {case['name']}"
    got = {k: named[k].double().cpu().numpy() for k in r["blocks"]}
    E.check(losses.double().cpu().numpy().reshape(4), got, r, worst, what)
    for k in r["trunk"]:
        assert not bool(named[k].any()), (what, k)
    for k in E.exact_zero_blocks(kind, case):
        assert not bool(named[k].any()), (what, k, "must be exactly zero")


def report(tag, worst, n):
    print(f"\n  {tag}: {n} cases, worst |gpu - ref64| / (eps32 * scale): " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


# ---- copies 1-2: the fused step kernels ------------------------------------------------------------------------------------
def run_fused(case, variant, monkeypatch, worst):
    from tianshou_amd import ppo as P

    monkeypatch.setenv("TS_PPO_STEPQ", str(variant))
    obs_dim, A = E.KINDS["fused"][0], len(case["head"]["raw"])
    r = E.reference("fused", case, tanh_abs=E.FAST_TANH_ABS)
    eng = P.PPOEngine(obs_dim, A, OP.flatten_params({k: r["params"][k] for k in OP.PARAM_ORDER}).cuda(), engine_cfg(case))
    losses, grads = eng._run_steps(batch(case, r), None, [0, len(case["rows"]["adv"])], want_grad=True)
    torch.cuda.synchronize()
    named, off = {}, 0
    for k, shp in P.param_shapes(obs_dim, A).items():
        n = int(np.prod(shp))
        named[k] = grads[off:off + n].reshape(shp)
        off += n
    assert off == grads.numel()
    verify("fused", case, r, losses[0], named, worst)


FUSED = [("copy1_stepq0", 0), ("copy2_stepq1", 1), ("copy2_stepq2", 2)]


@pytest.mark.parametrize("copy,variant", FUSED)
@pytest.mark.parametrize("group", ["ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value"])
def test_fused_step_kernels_at_clip_tie_and_clamp_edges(group, copy, variant, monkeypatch):
    worst: dict = {}
    cases = E.gauss_cases(group, 6)
    for case in cases:
        run_fused(case, variant, monkeypatch, worst)
    report(f"{copy} {group}", worst, len(cases))


@pytest.mark.parametrize("copy,variant", FUSED)
@pytest.mark.parametrize("act_dim", [1, 6, 8])
def test_fused_step_kernels_gaussian_head(act_dim, copy, variant, monkeypatch):
    """log sigma -5 / 0 / 2, act == mu, |act - mu| / sigma up to 30; 1, 6 and 8 actions (the kernels pad to 8)."""
    worst: dict = {}
    cases = E.gauss_head_cases((act_dim,))
    for case in cases:
        run_fused(case, variant, monkeypatch, worst)
    report(f"{copy} gauss_head A{act_dim}", worst, len(cases))


def test_fused_bounded_actor_copy1(monkeypatch):
    """mu = M tanh(raw), raw from 0 to +-20, actions inside and outside +-M: 1 - t * t from fast_tanh, exactly 0 at +-20."""
    worst: dict = {}
    cases = E.bounded_cases(6)
    for case in cases:
        run_fused(case, 0, monkeypatch, worst)
    report("copy1_stepq0 bounded", worst, len(cases))


# ---- copies 3-4: the GEMM path ---------------------------------------------------------------------------------------------
A_NAMES = list(OP.PARAM_ORDER[:7])
C_NAMES = list(OP.PARAM_ORDER[7:])
CS_NAMES = A_NAMES[:6] + ["a_wsig", "a_bsig"]


def run_gemm(kind, case, worst):
    from tianshou_amd import ppo_wide as PW

    obs_dim, hidden, _ = E.KINDS[kind]
    A = len(case["head"]["raw"])
    r = E.reference(kind, case)
    p, cfg = r["params"], engine_cfg(case)
    a_names = CS_NAMES if kind == "net_cs" else A_NAMES
    a_t, c_t = [p[k] for k in a_names], [p[k] for k in C_NAMES]
    ones = lambda ts: [torch.ones_like(t) for t in ts]                      # noqa: E731
    if kind == "wide":
        eng = PW.WidePPOEngine(obs_dim, A, hidden, PW.flat_from_tensors(a_t, c_t, obs_dim, hidden, A), cfg)
        split = lambda g: PW.flat_to_tensors(g, obs_dim, hidden, A)         # noqa: E731
        pad = PW.flat_from_tensors(ones(a_t), ones(c_t), obs_dim, hidden, A) == 0
    else:
        cs = kind == "net_cs"
        hid = [hidden, hidden]
        flat = torch.cat([PW.net_flat_from_tensors(a_t, obs_dim, hid, A, conditioned_sigma=cs), PW.net_flat_from_tensors(c_t, obs_dim, hid, None)])
        eng = PW.NetPPOEngine(obs_dim, A, hid, hid, "tanh", flat, cfg, conditioned_sigma=cs)
        split = eng.flat_to_tensors
        pad = torch.cat([PW.net_flat_from_tensors(ones(a_t), obs_dim, hid, A, conditioned_sigma=cs),
                         PW.net_flat_from_tensors(ones(c_t), obs_dim, hid, None)]) == 0
    losses = torch.full((4,), SENTINEL, device="cuda")
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    eng.step(batch(case, r), None, losses, grad_out=grad, apply=False)
    torch.cuda.synchronize()
    ga, gc = split(grad)
    assert len(ga) == len(a_names) and len(gc) == len(C_NAMES)
    named = {k: t.reshape(p[k].shape) for k, t in zip(a_names + C_NAMES, list(ga) + list(gc))}
    if kind == "net_cs":
        named["a_sigma"] = torch.zeros(A)
    verify(kind, case, r, losses, named, worst)
    assert not bool(grad[pad].any()), (kind, case["name"], "padding entries")


@pytest.mark.parametrize("group", ["ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value", "gauss_head"])
def test_copy3_wide_loss_kernels(group):
    worst: dict = {}
    cases = E.gauss_head_cases((3,)) if group == "gauss_head" else E.gauss_cases(group, 3)
    for case in cases:
        run_gemm("wide", case, worst)
    report(f"copy3_wide {group}", worst, len(cases))


def test_copy3_bounded_actor_through_the_per_layer_engine():
    """ppo_wide_actor_loss_kernel with mu_bound > 0 (tanhf): exactly 0 at raw = +-20."""
    worst: dict = {}
    cases = E.bounded_cases(3)
    for case in cases:
        run_gemm("net", case, worst)
    report("copy3_net bounded", worst, len(cases))


@pytest.mark.parametrize("group", ["ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value", "gauss_head", "bounded", "cs_clamp"])
def test_copy4_conditioned_sigma_loss_kernel(group):
    """cs_clamp: the sigma bias at -20 and at 2 exactly (the gradient passes), one float32 beyond either (the sigma columns get
    exactly 0, the entropy is the clamped value's), far beyond, one float32 inside, mid-range."""
    worst: dict = {}
    cases = {"gauss_head": lambda: E.gauss_head_cases((3,), cs=True), "bounded": lambda: E.bounded_cases(3, cs=True),
             "cs_clamp": lambda: E.cs_clamp_cases(3)}.get(group, lambda: E.gauss_cases(group, 3, cs=True))()
    for case in cases:
        run_gemm("net_cs", case, worst)
    report(f"copy4_cs {group}", worst, len(cases))
