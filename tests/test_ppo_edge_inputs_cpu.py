"""CPU checks of tests/ppo_edge_cases.py: the float64 per-row references agree with the float32 oracles (oracle_ppo,
oracle_ppo_discrete's network under oracle_ppo_cnn.minibatch_loss; torch autograd supplies the half-and-half and closed-interval
rules on the tie cases), the preconditions of every exact GPU assertion hold, and err32 -- the float32 oracle's own error
against float64, what the GPU bars are built from -- is measured per quantity: `pytest -s` prints the table.

Measured (err32 / (eps32 * scale), worst over the cases of a group; scale = the block's largest sum of |terms|):
                                   losses   head bias   head weight   sigma    V bias   V weight
  Gaussian, ratio / advnorm / value   6.6     11.1        12.7          4.1      0.7      1.7     (L <= 20)
  Gaussian, gauss_head (A = 8)        257     238         399           384      0.4      2.3     (L up to 3600)
  Gaussian, bounded                    79      62          62            75      0.3      1.7
  conditioned sigma, cs_clamp          23      28          27            13      0.2      1.1
  Categorical, all groups             5.2     10.6        14.5           -       0.4      1.9
Each is asserted <= 8 + 4 L (ppo_edge_cases.pin_units), L being the size of the terms logp is added up from."""
import numpy as np
import pytest

from tests import ppo_edge_cases as E

GAUSS_SETS = [(kind, group) for kind in ("fused", "wide", "net_cs") for group in E.GAUSS_GROUPS if group != "gauss_head"] + [
    ("fused", "gauss_head"), ("wide", "gauss_head"), ("net_cs", "gauss_head"), ("fused", "bounded"), ("net", "bounded"), ("net_cs", "bounded"),
    ("net_cs", "cs_clamp")]
CAT_GROUPS = ("ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value", "logits", "logits_dom1e4")


def cases_of(kind, group):
    if kind == "discrete":
        return E.cat_cases(group)
    cs = kind == "net_cs"
    A = 6 if kind == "fused" else 3
    if group == "gauss_head":
        return E.gauss_head_cases((1, 6, 8) if kind == "fused" else (A,), cs=cs)
    if group == "bounded":
        return E.bounded_cases(A, cs=cs)
    if group == "cs_clamp":
        return E.cs_clamp_cases(A)
    return E.gauss_cases(group, A, cs=cs)


@pytest.mark.parametrize("kind,group", GAUSS_SETS + [("discrete", g) for g in CAT_GROUPS])
def test_float64_references_agree_with_the_oracles(kind, group):
    worst: dict = {}
    cases = cases_of(kind, group)
    assert len(cases) >= 4
    for case in cases:
        r = E.reference(kind, case)
        for k in r["trunk"]:                                     # zero head weights pass nothing down
            assert not r["trunk_grads32"][k].any(), (case["name"], k)
        assert np.all(np.isfinite(r["oracle_losses"])) and np.all(np.isfinite(r["losses"])), case["name"]
        pin = E.pin_units(case, r["ref"])
        for k, u in E.err32_units(r).items():
            worst[k] = max(worst.get(k, 0.0), u)
            assert u <= pin, (case["name"], k, u, pin)
        # realised ratios keep clear of every boundary by far more than float32 logp rounding
        assert E.ratio_margin(case, r["ref"]) >= E.RATIO_MARGIN, (case["name"], E.ratio_margin(case, r["ref"]))
    print(f"{kind} {group}: {len(cases)} cases, err32 / (eps32 * scale) worst: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


def _surrogate_class32(case, ref):
    """The branch the float32 expressions take (ratio from a float32 logp), as the pair (surr1 <= surr2, dual clip cuts)."""
    f = np.float32
    hp, rows = case["hp"], case["rows"]
    A = ref["adv"].astype(f)
    ratio = np.exp(ref["logp"].astype(f) - rows["logp_old"]).astype(f)
    s1 = ratio * A
    s2 = np.clip(ratio, f(1 - hp["eps_clip"]), f(1 + hp["eps_clip"])).astype(f) * A
    cut = np.zeros(len(A), bool)
    if hp["dual_clip"]:
        cut = (A < 0) & (np.minimum(s1, s2) < f(hp["dual_clip"]) * A)
    return s1 <= s2, cut


@pytest.mark.parametrize("kind", ["fused", "discrete"])
@pytest.mark.parametrize("variant", ["dual_off", "dual_on"])
def test_every_ratio_case_has_one_clear_class(kind, variant):
    """All rows of a batch take the same branch, in float64 and in float32 alike; the classes are the intended ones."""
    for case in cases_of(kind, "ratio_" + variant):
        ref = (E.cat_ref64 if kind == "discrete" else E.gauss_ref64)(case["head"], case["rows"], case["hp"])
        A, ratio = ref["adv"], ref["ratio"]
        s1, s2 = ratio * A, np.clip(ratio, 1 - E.EPS_CLIP, 1 + E.EPS_CLIP) * A
        le64 = s1 <= s2
        cut64 = (A < 0) & (np.minimum(s1, s2) < E.DUAL_CLIP * A) if case["hp"]["dual_clip"] else np.zeros(len(A), bool)
        le32, cut32 = _surrogate_class32(case, ref)
        name = case["name"]
        assert np.array_equal(le64, le32) and np.array_equal(cut64, cut32), name
        assert len(set(le64.tolist())) == 1 and len(set(cut64.tolist())) == 1, name
        rc, ac = name.split("/")[1:3]
        inside = rc in ("inside", "hi_in", "lo_in")
        pos, neg = ac.endswith("pos"), ac.endswith("neg")
        high = rc in ("hi_out", "dual_in", "dual_out", "far_hi", "huge")
        # torch.min: the gradient passes inside the range, for A > 0 below it and for A < 0 above it (A == 0: both are 0)
        assert bool(le64[0]) == (inside or ac == "zero" or (pos and not high) or (neg and high)), name
        assert bool(cut64[0]) == (variant == "dual_on" and neg and rc in ("dual_out", "far_hi", "huge")), name
        passes = bool(le64[0]) and not bool(cut64[0]) and ac != "zero"
        assert bool(np.all(ref["dlogp"] != 0)) == passes or ac.startswith("tiny"), name


def test_value_cases_are_exact_in_float32_and_take_the_intended_branch():
    f = np.float32
    e = f(E.EPS_CLIP)
    for case in cases_of("fused", "value"):
        cls = case["value_class"]
        V, rows = f(case["head"]["v"]), case["rows"]
        ref = E.gauss_ref64(case["head"], rows, case["hp"])
        if cls == "inside_rounded":
            continue
        vo, r = rows["v_s"], rows["returns"]
        dvo = (V - vo).astype(f)
        vclip = (vo + np.clip(dvo, -e, e)).astype(f)
        a, b = (r - V).astype(f), (r - vclip).astype(f)
        vf1, vf2 = (a * a).astype(f), (b * b).astype(f)
        # every float32 step is exact: the float64 evaluation of the same expressions gives the same numbers
        assert np.array_equal(dvo.astype(np.float64), V.astype(np.float64) - vo.astype(np.float64)), cls
        assert np.array_equal(vclip.astype(np.float64), vo.astype(np.float64) + np.clip(dvo.astype(np.float64), -0.25, 0.25)), cls
        cls32 = np.where(vf1 > vf2, 1, np.where(vf2 > vf1, 2, 0))
        assert np.array_equal(cls32, ref["vclass"]) and bool(np.all(ref["vclass"] == E.VALUE_EXPECT[cls])), (cls, cls32, ref["vclass"])
        if cls in ("at_plus_eps", "at_minus_eps"):
            assert bool(np.all(np.abs(dvo) == e)) and bool(np.all(vclip == V))          # the closed end: the gradient passes
            assert np.allclose(ref["d_v"], -2.0 * (r.astype(np.float64) - float(V)) * E.VF_COEF / len(r), rtol=1e-15, atol=0)
        if cls.startswith("ulp_beyond"):
            assert bool(np.all(dvo == np.nextafter(e, f(1)))) and bool(np.all(np.abs(dvo) > e))
        if cls in E.VALUE_EXACT_ZERO:
            assert not ref["d_v"].any()
        if cls == "clamped_tie":                                                           # torch gives half of g1
            assert bool(np.all(np.abs(dvo) > e))
            assert np.array_equal(ref["d_v"], 0.5 * -2.0 * (r.astype(np.float64) - float(V)) * E.VF_COEF / len(r)) and ref["d_v"].all()
    # the issue's example: V = 0, v_s = 1, returns = 0.375 -> v_clip = 0.75, vf1 = vf2 = 0.140625
    rows = dict(v_s=E.f32([1.0]), returns=E.f32([0.375]))
    vterm, d_v, cls = E.value64(0.0, rows, E.hyper())
    assert float(vterm[0]) == 0.140625 and int(cls[0]) == 0 and float(d_v[0]) == 0.5 * (-2.0 * 0.375) * E.VF_COEF


def test_constant_advantages_normalise_to_exact_zeros():
    for kind in ("fused", "discrete"):
        for case in cases_of(kind, "advnorm"):
            adv = case["rows"]["adv"]
            r = E.reference(kind, case)
            if "/const/" not in case["name"]:
                assert float(adv.std(ddof=1)) > 0.1
                continue
            assert float(adv.astype(np.float64).std(ddof=1)) == 0.0 and float(adv.std(ddof=1)) == 0.0
            assert float(np.float32(adv.sum()) / np.float32(len(adv))) == float(adv[0])      # the float32 mean is exact too
            assert not r["ref"]["adv"].any() and not r["ref"]["dlogp"].any()
            if kind == "fused":          # a Gaussian's entropy does not depend on mu: nothing but -ent_coef reaches sigma
                assert not r["blocks"]["a_bmu"].any() and not r["blocks"]["a_wmu"].any()
                assert np.allclose(r["blocks"]["a_sigma"], -E.ENT_COEF, rtol=1e-14)
            else:                        # the entropy gradient alone
                ref = r["ref"]
                want = E.ENT_COEF * ref["p"] * (np.log(ref["p"]) + ref["H"])
                assert np.allclose(r["blocks"]["actor.b"], want, rtol=1e-12, atol=1e-18) and r["blocks"]["actor.b"].any()


def test_exact_zero_claims_hold_in_float64_and_in_the_oracle():
    import torch

    # saturated bound: tanh(+-20) is +-1 in float32, 1 - t * t exactly 0
    assert float(torch.tanh(torch.tensor(20.0))) == 1.0 and float(torch.tanh(torch.tensor(-20.0))) == -1.0
    n = 0
    for case in cases_of("net", "bounded"):
        if "/raw20/" in case["name"] or "/raw-20/" in case["name"]:
            r = E.reference("net", case)
            g, _ = E.gauss_oracle32(r["params"], case["head"], case["rows"], r["obs"], case["hp"]), None
            assert not g[1]["a_bmu"].any() and not g[1]["a_wmu"].any() and g[1]["a_sigma"].any()
            assert float(np.abs(r["blocks"]["a_bmu"]).max()) < 1e-12                      # float64: sech^2(20) = 1.7e-17
            n += 1
    assert n == 16
    # beyond the sigma clamp: nothing reaches the sigma columns, and the entropy is the clamped value's
    n = 0
    for case in cases_of("net_cs", "cs_clamp"):
        r = E.reference("net_cs", case)
        name = case["name"].split("/")[1]
        if name in E.CS_BLOCKED:
            assert not r["blocks"]["a_bsig"].any() and not r["blocks"]["a_wsig"].any()
            edge = E.CS_MIN if "min" in name or "below" in name else E.CS_MAX
            assert r["losses"][3] == pytest.approx(3 * (0.5 + E.HALF_LOG_2PI + edge), rel=1e-14)
            n += 1
        else:
            assert r["blocks"]["a_bsig"].all()
    assert n == 12
    # one action: logp = 0, entropy 0, every logit gradient exactly 0
    n = 0
    for case in cases_of("discrete", "logits"):
        if "/A1/" in case["name"]:
            r = E.reference("discrete", case)
            assert not r["ref"]["logp"].any() and r["ref"]["H"] == 0.0 and not r["blocks"]["actor.b"].any() and not r["blocks"]["actor.w"].any()
            assert r["losses"][3] == 0.0 and r["oracle_losses"][3] == 0.0
            n += 1
    assert n == 3


def test_dominated_logits_underflow_in_float32_and_ties_are_exact():
    f = np.float32
    assert float(np.exp(f(-90.0))) < float(np.finfo(f).tiny) and float(np.exp(f(-1e4))) == 0.0          # subnormal / zero
    for A in (2, 18, 31):
        p = E.cat_ref64(E.cat_head(E.cat_logits("equal", A)), dict(act=np.zeros(1, np.int64), adv=E.f32([1.0]), logp_old=E.f32([0.0]),
                                                                    v_s=E.f32([0.5]), returns=E.f32([0.5])), E.hyper())["p"]
        assert np.allclose(p, 1.0 / A, rtol=1e-15)
        p = E.cat_ref64(E.cat_head(E.cat_logits("dom90", A, 1)), dict(act=np.zeros(1, np.int64), adv=E.f32([1.0]), logp_old=E.f32([0.0]),
                                                                      v_s=E.f32([0.5]), returns=E.f32([0.5])), E.hyper())["p"]
        assert 0.0 < p[0] < 1e-38 and p[1] == pytest.approx(1.0)                      # float64 keeps what float32 loses
