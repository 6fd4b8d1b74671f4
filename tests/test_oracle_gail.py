"""CPU: tests/oracle_gail.py (the project's restatement of GAIL's reward, discriminator loss, step and chunking rule) is pinned
to what the unmodified reference produced: tests/golden/gail_mujoco.npz and gail_odd.npz (tools/gen_golden_gail.py)."""
import os

import numpy as np
import pytest
import torch

from tests import oracle_gail as OG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACT = {0: "tanh", 1: "relu", 2: "none"}
_CACHE: dict = {}


def load_gail(tag: str) -> dict:
    """The fixture with its scalars unpacked; read once per process and never modified."""
    if tag not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"gail_{tag}.npz")))
        E, T, obs_dim, act_dim, batch_size, repeat, num, n_expert, expert_seed, seed, n_updates, stride = (int(x) for x in g["dims"])
        g.update(E=E, T=T, obs_dim=obs_dim, act_dim=act_dim, batch_size=batch_size, repeat=repeat, num=num, n_expert=n_expert,
                 expert_seed=expert_seed, seed=seed, n_updates=n_updates, stride=stride, N=E * T,
                 cfg=dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]])),
                 disc_act=ACT[int(g["disc_activation"])], act_name=ACT[int(g["activation"])])
        _CACHE[tag] = g
    return _CACHE[tag]


def disc_tensors(g, dtype=torch.float32):
    n = sum(1 for k in g if k.startswith("d") and k.endswith("_0") and k[1:-2].isdigit())
    return [torch.from_numpy(g[f"d{i}_0"]).to(dtype) for i in range(n)]


def strided(ts, stride) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()[::stride]


def replay(g, dtype=torch.float32):
    """Both updates' discriminator halves on the oracle, fed the recorded draws -> per update (rew, stats, tensors), optimizer."""
    t = disc_tensors(g, dtype)
    opt = OG.Adam(lr=g["cfg"]["disc_lr"], max_grad_norm=g["cfg"]["disc_max_grad_norm"] or None)
    e_obs, e_act = torch.from_numpy(g["expert_obs"]).to(dtype), torch.from_numpy(g["expert_act"]).to(dtype)
    out = []
    for u in range(g["n_updates"]):
        idx = g[f"u{u}_pre_indices"]
        obs, act = torch.from_numpy(g["obs"][idx]).to(dtype), torch.from_numpy(g["act"][idx]).to(dtype)
        rew = OG.reward(t, obs, act, g["disc_act"])
        t, stats = OG.disc_update(t, opt, obs, act, g[f"u{u}_split_perm"], e_obs, e_act, g[f"u{u}_exp_index"], g["num"], g["disc_act"])
        out.append((rew, stats, t))
    return out, opt


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_fixture_shapes_follow_the_chunk_rule(tag):
    g = load_gail(tag)
    bsz, ch = OG.chunks(g["N"], g["num"])
    for u in range(g["n_updates"]):
        assert g[f"u{u}_exp_index"].shape == (len(ch), bsz) and g[f"u{u}_disc_stats"].shape == (len(ch), 3)
        assert sorted(g[f"u{u}_split_perm"].tolist()) == list(range(g["N"]))
        assert g[f"u{u}_pre_rew"].dtype == np.float32 and g[f"u{u}_exp_index"].max() < g["n_expert"]
    if tag == "odd":
        assert (bsz, len(ch), ch[-1]) == (3, 12, (33, 38)) and g["n_expert"] < g["N"]
    else:
        assert (bsz, len(ch)) == (64, 2)
    assert int(g["adam_step_d"]) == g["n_updates"] * len(ch)                # steps, not disc_update_num


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_expert_draws_are_the_buffers_own_generator(tag):
    """ReplayBuffer.sample_indices(bsz) on a full plain buffer is RandomState(random_seed).choice(size, bsz) (buffer_base.py:98,
    517): the fixture's draws are reproduced from the seed it records, in order."""
    g = load_gail(tag)
    rs = np.random.RandomState(g["expert_seed"])
    for u in range(g["n_updates"]):
        for row in g[f"u{u}_exp_index"]:
            np.testing.assert_array_equal(rs.choice(g["n_expert"], len(row)), row)


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_oracle_reproduces_the_reference(tag):
    g = load_gail(tag)
    out, opt = replay(g)
    for u, (rew, stats, t) in enumerate(out):
        np.testing.assert_allclose(rew.numpy(), g[f"u{u}_pre_rew"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(stats[:, 0].numpy(), g[f"u{u}_disc_stats"][:, 0], rtol=1e-5)
        np.testing.assert_array_equal(stats[:, 1:].numpy().astype(np.float64), g[f"u{u}_disc_stats"][:, 1:])
        np.testing.assert_allclose(strided(t, g["stride"]), g[f"u{u}_disc_mid"], rtol=1e-5, atol=0.02 * g["cfg"]["disc_lr"])
        np.testing.assert_array_equal(g[f"u{u}_disc_mid"], g[f"u{u}_d"])   # the PPO half leaves the discriminator alone
    assert opt.step == int(g["adam_step_d"])
    np.testing.assert_allclose(strided(opt.m, g["stride"]), g["adam_m_d"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(strided(opt.v, g["stride"]), g["adam_v_d"], rtol=1e-3, atol=1e-8)


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_float64_mode_agrees_and_the_logits_keep_a_margin(tag):
    """The same code in float64 (the reference of the kernel tests) stays within float32 rounding of the float32 run, and no
    float64 logit of any step lies within 1e-4 of 0: the accuracies of these fixtures can be compared exactly."""
    g = load_gail(tag)
    out32, _ = replay(g)
    out64, _ = replay(g, torch.float64)
    for (r32, s32, _), (r64, s64, _) in zip(out32, out64):
        np.testing.assert_allclose(r32.numpy(), r64.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(s32[:, 0].numpy(), s64[:, 0].numpy(), rtol=1e-5)
        assert torch.equal(s32[:, 1:], s64[:, 1:].float())
    # margin, step by step along the float64 trajectory
    t = disc_tensors(g, torch.float64)
    opt = OG.Adam(lr=g["cfg"]["disc_lr"], max_grad_norm=g["cfg"]["disc_max_grad_norm"] or None)
    e_obs, e_act = torch.from_numpy(g["expert_obs"]).double(), torch.from_numpy(g["expert_act"]).double()
    bsz, ch = OG.chunks(g["N"], g["num"])
    for u in range(g["n_updates"]):
        idx = g[f"u{u}_pre_indices"]
        obs, act = torch.from_numpy(g["obs"][idx]).double(), torch.from_numpy(g["act"][idx]).double()
        perm = torch.from_numpy(g[f"u{u}_split_perm"])
        for k, (a, b) in enumerate(ch):
            ei = torch.from_numpy(g[f"u{u}_exp_index"][k])
            with torch.no_grad():
                l_pi = OG.disc_forward(t, obs[perm[a:b]], act[perm[a:b]], g["disc_act"])
                l_exp = OG.disc_forward(t, e_obs[ei], e_act[ei], g["disc_act"])
            assert float(l_pi.abs().min()) >= 1e-4 and float(l_exp.abs().min()) >= 1e-4, (u, k)
            _, gs = OG.disc_grad(t, obs[perm[a:b]], act[perm[a:b]], e_obs[ei], e_act[ei], g["disc_act"])
            t = opt.apply(t, gs)


def test_loss_terms_are_softplus_in_the_stable_form():
    l = torch.tensor([-104.0, -88.0, -1.0, -0.0, 0.0, 1e-6, 3.0, 88.0, 104.0], dtype=torch.float64)
    sp = lambda z: torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))  # noqa: E731
    loss, a_pi, a_exp = OG.loss_terms(l, l)
    assert abs(float(loss) - float(sp(l).mean() + sp(-l).mean())) < 1e-12
    assert float(a_pi) == 3 / 9 and float(a_exp) == 4 / 9                  # strict inequalities: +-0 counts for neither
