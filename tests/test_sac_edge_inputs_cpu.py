"""CPU checks of tests/sac_edge_cases.py: the inputs of the SAC-family edge tests really are where they claim to be, the unmodified
float32 oracle is finite on all of them, and torch's clamp / minimum conventions are the ones the kernels restate.  A change to
the builders cannot quietly empty a regime."""
import numpy as np
import pytest
import torch

from oracle import oracle_dsac as ODS
from oracle import oracle_sac as OS
from tests import sac_edge_cases as E

OBS, HID = 7, 64


def _finite(x) -> bool:
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    return x is None or bool(torch.isfinite(torch.as_tensor(x, dtype=torch.float64)).all())


def test_sweep_fills_every_band_and_the_reference_stays_within_twice_its_condition():
    c = E.sweep_case(OBS)
    B = c["noise"].shape[0]
    _, logp64, a64, sigma = E.policy64(c["actor"], c["obs"], c["noise"])
    assert torch.equal(sigma, torch.full_like(sigma, float(np.exp(2.0))))          # log sigma 3.0 is clamped to 2
    counts = E.band_counts(a64)
    assert sum(counts) == B and all(n >= 0.1 * B for n in counts), counts
    assert float(a64.abs().max()) > 20.0
    _, logp32, _, _ = OS.policy_forward(c["actor"], c["obs"], c["noise"])
    assert _finite(logp32)
    c_ref = float(E.logp_ratio(logp32, a64, logp64).max())
    assert 0.0 < c_ref <= 2.0, c_ref
    # ... while the flat bar of the other SAC tests means nothing here: float32 itself is off by far more than 1e-5
    assert float((logp32.flatten().double() - logp64).abs().max()) > 0.1


@pytest.mark.parametrize("A", [1, 17, 32])
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("max_action", [0.0, 1.3])
def test_gaussian_cases_reach_the_clamp_and_saturation_and_the_reference_is_finite(A, B, max_action):
    for shift in ((0,) if A > 1 else (0, 1, 4, 5)):
        c = E.gaussian_case(OBS, A, B, 3, HID, shift)
        cols, raw = c["cols"], c["actor"]["bsig"]
        mu, sigma = OS.actor_forward(c["actor"], c["obs"], max_action)
        assert torch.equal(mu, (max_action * torch.tanh(c["actor"]["bmu"]) if max_action else c["actor"]["bmu"]).expand(B, A))
        assert torch.equal(sigma[0], raw.clamp(OS.SIGMA_MIN, OS.SIGMA_MAX).exp())
        assert all(float(raw[j]) in (OS.SIGMA_MIN, OS.SIGMA_MAX) for j in cols["boundary"])
        assert all(OS.SIGMA_MIN < float(raw[j]) < OS.SIGMA_MAX for j in cols["inward"])
        assert all(not OS.SIGMA_MIN <= float(raw[j]) <= OS.SIGMA_MAX for j in cols["beyond"])
        if A > 1:
            assert all(len(cols[k]) >= 2 for k in ("boundary", "inward", "beyond", "interior", "moderate", "mu12"))
            assert c["noise"][E.zero_noise_row(B)].abs().max() == 0 if B > 1 else True
        cfg = OS.SACConfig(auto_alpha=True, log_alpha0=-0.3, target_entropy=-float(A), actor_lr=0.0, critic_lr=0.0,
                           alpha_lr=0.0, tau=0.0, max_action=max_action)
        st = OS.SACState.create(c["actor"], c["critic1"], c["critic2"], cfg)
        col: dict = {}
        ref = OS.update_with_batch(st, cfg, c["obs"], c["act"], c["ret"], c["noise"], None, collect=col)
        assert _finite(col["actor_grads"]) and _finite(ref["actor_loss"]) and _finite(OS.target_q(st, cfg, c["obs"], c["noise_next"]))
        # the float32 oracle stays within twice eps32 * condition + the rounding of a = mu + noise * sigma, on every row
        for nz in (c["noise"], c["noise_next"], torch.zeros_like(c["noise"])):
            _, logp64, a64, sigma64 = E.policy64(c["actor"], c["obs"], nz, max_action)
            logp32 = OS.policy_forward(c["actor"], c["obs"], nz, max_action)[1].flatten().double()
            unit = E.EPS32 * E.logp_condition(a64, logp64) + E.logp_rounding(a64, nz, sigma64)
            assert float(((logp32 - logp64).abs() / unit).max()) <= 2.0
        if A > 1 and B > 1 and max_action == 0.0:
            _, _, a64, _ = E.policy64(c["actor"], c["obs"], c["noise"])
            assert int((a64.abs() >= 10.0).sum()) >= B and int((a64.abs() < 3.0).sum()) >= B      # saturated and free entries


def test_torch_clamp_passes_the_gradient_at_the_boundary_itself():
    raw = torch.tensor(E.SIG_BIASES, dtype=torch.float32, requires_grad=True)
    torch.clamp(raw, min=OS.SIGMA_MIN, max=OS.SIGMA_MAX).exp().sum().backward()
    for kind, g, r in zip(E.SIG_KINDS, raw.grad.tolist(), raw.tolist()):
        assert (g == 0.0) == (kind == "beyond"), (kind, r, g)
    assert raw.grad[0] == float(np.exp(np.float32(-20.0))) and raw.grad[1] == torch.tensor(2.0).exp()


def test_torch_minimum_splits_the_gradient_of_a_tie_in_halves():
    a = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    b = torch.tensor([1.0, 3.0, 2.0], requires_grad=True)
    torch.min(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0, 0.0] and b.grad.tolist() == [0.5, 0.0, 1.0]
    # so with critic 2 a copy of critic 1 the actor's gradient is that of alpha * logp - Q1, and the loss is the untied formula
    c = E.gaussian_case(OBS, 17, 33, 3, HID, tie=True)
    g_tie = OS.gradients(c["actor"], c["critic1"], c["critic2"], 0.7, c["obs"], c["act"], c["ret"], c["noise"], dtype=torch.float64)
    p = {k: v.double().requires_grad_(True) for k, v in c["actor"].items()}
    a64, logp, _, _ = OS.policy_forward(p, c["obs"].double(), c["noise"].double())
    loss = (0.7 * logp.flatten() - OS.critic_forward(E.double(c["critic1"]), c["obs"].double(), a64).flatten()).mean()
    for k, g in zip(p, torch.autograd.grad(loss, list(p.values()))):
        torch.testing.assert_close(g_tie["actor_grads"][k], g, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("A,B", [(1, 1), (17, 257), (32, 257)])
def test_opposed_tie_is_bit_exact_and_its_sides_pull_in_opposite_directions(A, B):
    c = E.opposed_tie_case(OBS, A, B, 3, HID)
    for dtype in (torch.float32, torch.float64):
        cast = lambda d: {k: v.to(dtype) for k, v in d.items()}                        # noqa: E731
        obs = c["obs"].to(dtype)
        sq = OS.policy_forward(cast(c["actor"]), obs, c["noise"].to(dtype))[0].clone().requires_grad_(True)
        assert not sq.any()                                                            # the squashed action is exactly 0
        q1, q2 = OS.critic_forward(cast(c["critic1"]), obs, sq), OS.critic_forward(cast(c["critic2"]), obs, sq)
        assert torch.equal(q1, q2)                                                     # a tie in every row, bit for bit
        g1, g2 = torch.autograd.grad(q1.sum(), sq, retain_graph=True)[0], torch.autograd.grad(q2.sum(), sq)[0]
        assert torch.equal(g1, -g2) and float(g1.abs().min()) > 0.0                    # ... whose sides pull apart
    g = OS.gradients(c["actor"], c["critic1"], c["critic2"], 0.7, c["obs"], c["act"], c["ret"], c["noise"], dtype=torch.float64)
    assert not g["actor_grads"]["bmu"].any() and g["actor_grads"]["bsig"].any()        # halves cancel; the logp part stays


@pytest.mark.parametrize("A", [1, 6, 32])
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("twin", [True, False])
def test_deterministic_cases_hit_the_noise_clip_exactly_and_saturate(A, B, twin):
    c = E.det_case(OBS, A, B, 4, twin, HID)
    act = OS.det_actor_forward(c["actor"], c["obs"], 1.5)
    for j in c["cols"]["saturated"]:
        assert (act[:, j].abs() == 1.5).all()
    n = c["noise"] * E.TD3_POLICY_NOISE
    assert torch.equal(n.double(), c["noise"].double() * E.TD3_POLICY_NOISE)                       # exact in float32
    if B > 1:
        on, inside, outside = n.abs() == E.TD3_NOISE_CLIP, n.abs() == E._inward(E.TD3_NOISE_CLIP), n.abs() == 10.0
        assert on.any() and inside.any() and outside.any()
        assert (n.abs() < 0.4).any()
    cfg = OS.TD3Config(twin=twin, max_action=1.5, policy_noise=E.TD3_POLICY_NOISE, noise_clip=E.TD3_NOISE_CLIP, actor_lr=0.0,
                       critic_lr=0.0, tau=0.0, update_actor_freq=1)
    st = OS.TD3State.create(c["actor"], c["critic1"], c["critic2"], cfg)
    tq = OS.td3_target_q(st, cfg, c["obs"], c["noise"]).flatten()
    assert _finite(tq)
    tq64 = E.td3_target64(c, 1.5, E.TD3_POLICY_NOISE, E.TD3_NOISE_CLIP, twin)
    np.testing.assert_allclose(tq.numpy(), tq64.numpy(), rtol=1e-5, atol=1e-5)
    if twin and B > 1:                              # the clamp is live on these inputs: without it the target moves by > 0.1
        assert float((E.td3_target64(c, 1.5, E.TD3_POLICY_NOISE, 0.0, True) - tq64).abs().max()) > 0.2
    col: dict = {}
    OS.td3_update_with_batch(st, cfg, c["obs"], c["act"], c["ret"], collect=col)
    assert _finite(col["actor_grads"])
    assert all(float(col["actor_grads"]["ba"][j]) == 0.0 for j in c["cols"]["saturated"])


@pytest.mark.parametrize("n_act", [2, 31, 32, 33, 64])
@pytest.mark.parametrize("pattern", E.DSAC_PATTERNS)
def test_discrete_cases_are_what_they_say_and_the_reference_is_finite(n_act, pattern):
    B = 33
    c = E.dsac_case(OBS, n_act, B, 5, pattern, HID)
    logits = ODS.net_forward(c["actor"], c["obs"])
    p = torch.softmax(logits, -1)
    if pattern == "spread":
        assert float((logits.max(-1).values - logits.median(-1).values).median()) > 3.0 and len(set(logits.argmax(-1).tolist())) > 1
    else:
        assert torch.equal(logits, c["actor"]["head.b"].expand(B, n_act))
    if pattern == "underflow":
        assert int((p[0] == 0.0).sum()) == n_act - 1                                   # float32 underflow
    if pattern == "dominant":
        assert int((p[0] < 1e-16).sum()) == n_act - 1 and int((p[0] == 0.0).sum()) == 0
    if pattern == "tied_max":
        top = logits[0].topk(2).values
        assert top[0] == top[1]
    q1, q2 = ODS.net_forward(c["critic1"], c["obs"]), ODS.net_forward(c["critic2"], c["obs"])
    assert (q1[0] == q2[0]).any() and (q1[0] < q2[0]).any()
    cfg = OS.SACConfig(auto_alpha=False, alpha=0.15, actor_lr=0.0, critic_lr=0.0, alpha_lr=0.0, tau=0.0)
    st = OS.SACState.create(c["actor"], c["critic1"], c["critic2"], cfg)
    col: dict = {}
    ref = ODS.update_with_batch(st, cfg, c["obs"], c["act"], c["ret"], collect=col)
    assert _finite(col["actor_grads"]) and _finite(col["entropy"]) and _finite(ref["actor_loss"]) and _finite(ODS.target_q(st, cfg, c["obs"]))
    y = E.dsac64(c, cfg.alpha)
    if pattern == "equal":
        np.testing.assert_allclose(-y["neg_ent"].numpy(), np.log(n_act), rtol=1e-12)
    np.testing.assert_allclose(ODS.target_q(st, cfg, c["obs"]).numpy(), y["target"].numpy(), rtol=1e-5, atol=1e-5)
