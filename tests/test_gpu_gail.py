"""GPU parity of GAIL: the discriminator engine (tianshou_amd.gail over ts_gail_reward / ts_gail_disc_steps) and
the HipGAIL drop-in (integration.make_hip_gail over tests/standin_gail.py) against the oracle (tests/oracle_gail.py) and against
what the unmodified reference produced (tests/golden/gail_mujoco.npz: the irl_gail.py networks, one-launch shape, even chunks;
gail_odd.npz: a three-layer ReLU discriminator, 12 steps of 3 with a last step of 5 policy rows against 3 expert rows).

Bars are the project's: loss 1e-5 relative, post-Adam parameters rtol 1e-5 / atol 0.02 lr against the oracle
(test_gpu_npg.py::test_critic_step_vs_oracle); against the reference's recorded run the bars of the PPO golden tests
(test_gpu_ppo.py / test_gpu_hooks.py: v_s, returns, advantages 1e-5, loss summaries 2e-5, parameters rtol 1e-4 / atol 0.02 lr,
moments rtol 1e-3).  Accuracies are compared exactly (tests/test_oracle_gail.py checks the logits' margin on both fixtures)."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import oracle_gail as OG
from tests import standin_gail as SG
from tests.test_oracle_gail import disc_tensors, load_gail

pytestmark = pytest.mark.gpu
ACT_CLS = {"tanh": nn.Tanh, "relu": nn.ReLU, "none": None}


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def strided(ts, stride) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()[::stride]


def rollout(g, u=0):
    idx = g[f"u{u}_pre_indices"]
    return torch.from_numpy(g["obs"][idx]), torch.from_numpy(g["act"][idx])


def engine(g, route="auto"):
    from tianshou_amd import gail as G

    cfg = G.GAILConfig(disc_update_num=g["num"], lr=g["cfg"]["disc_lr"], max_grad_norm=g["cfg"]["disc_max_grad_norm"] or None,
                       route=route)
    hidden = [int(h) for h in g["hidden_d"]]
    flat = G.GAILDiscriminator.flat_from_tensors(disc_tensors(g), g["obs_dim"], g["act_dim"], hidden)
    return G.GAILDiscriminator(g["obs_dim"], g["act_dim"], hidden, g["disc_act"], flat, g["expert_obs"], g["expert_act"], cfg)


def routes(tag):
    return ["per_layer", "one_launch"] if tag == "mujoco" else ["per_layer"]


# ---- engine level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_reward_vs_oracle(tag):
    g = load_gail(tag)
    obs, act = rollout(g)
    r64 = OG.reward(disc_tensors(g, torch.float64), obs.double(), act.double(), g["disc_act"])
    l64 = OG.disc_forward(disc_tensors(g, torch.float64), obs.double(), act.double(), g["disc_act"]).detach()
    for route in routes(tag) + ["auto"]:
        rew, logits = engine(g, route).reward(obs, act, want_logits=True)
        assert rew.dtype == torch.float32 and rew.shape == (g["N"],)
        print(tag, route, rel_err(rew.cpu(), r64), rel_err(logits.cpu(), l64))
        assert rel_err(rew.cpu(), r64) < 1e-5 and rel_err(logits.cpu(), l64) < 1e-5
        np.testing.assert_allclose(rew.cpu().numpy(), g["u0_pre_rew"], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_disc_steps_with_adam_vs_oracle_float32_on_device_and_float64(tag):
    """Both updates of the fixture's draws (4 resp. 24 Adam steps) against the oracle run in float32 on the same device and in
    float64 on the host."""
    g = load_gail(tag)
    lr = g["cfg"]["disc_lr"]
    mk = lambda: OG.Adam(lr=lr, max_grad_norm=g["cfg"]["disc_max_grad_norm"] or None)     # noqa: E731
    for route in routes(tag):
        eng = engine(g, route)
        t32, o32 = [x.cuda() for x in disc_tensors(g)], mk()
        t64, o64 = disc_tensors(g, torch.float64), mk()
        for u in range(g["n_updates"]):
            obs, act = rollout(g, u)
            perm, ei = g[f"u{u}_split_perm"], g[f"u{u}_exp_index"]
            stats = eng.disc_update(obs, act, perm, ei).cpu()
            t32, s32 = OG.disc_update(t32, o32, obs.cuda(), act.cuda(), perm, eng.expert_obs, eng.expert_act, ei, g["num"], g["disc_act"])
            t64, s64 = OG.disc_update(t64, o64, obs.double(), act.double(), perm, torch.from_numpy(g["expert_obs"]).double(),
                                      torch.from_numpy(g["expert_act"]).double(), ei, g["num"], g["disc_act"])
            print(tag, route, u, rel_err(stats[:, 0], s64[:, 0]), rel_err(s32[:, 0].cpu(), s64[:, 0]))
            np.testing.assert_allclose(stats[:, 0].numpy(), s64[:, 0].numpy(), rtol=1e-5)
            assert torch.equal(stats[:, 1:], s64[:, 1:].float()) and torch.equal(stats[:, 1:], s32[:, 1:].cpu())
            for a, b, c in zip(eng.to_tensors(), t32, t64):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=0.02 * lr)
                np.testing.assert_allclose(a.cpu().numpy(), c.numpy(), rtol=1e-5, atol=0.02 * lr)
        assert eng.optim_step == o64.step == int(g["adam_step_d"])


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_engine_replays_the_reference(tag):
    """The stored split permutation and expert indices fed to the engine: rewards, per-step statistics and the strided
    discriminator samples after each update are the reference's."""
    g = load_gail(tag)
    lr = g["cfg"]["disc_lr"]
    for route in routes(tag):
        eng = engine(g, route)
        for u in range(g["n_updates"]):
            obs, act = rollout(g, u)
            np.testing.assert_allclose(eng.reward(obs, act).cpu().numpy(), g[f"u{u}_pre_rew"], rtol=1e-5, atol=2e-6)
            stats = eng.disc_update(obs, act, g[f"u{u}_split_perm"], g[f"u{u}_exp_index"]).cpu().numpy().astype(np.float64)
            np.testing.assert_allclose(stats[:, 0], g[f"u{u}_disc_stats"][:, 0], rtol=1e-5, atol=2e-6)
            np.testing.assert_array_equal(stats[:, 1:], g[f"u{u}_disc_stats"][:, 1:])
            np.testing.assert_allclose(strided(eng.to_tensors(), g["stride"]), g[f"u{u}_disc_mid"], rtol=1e-4, atol=0.02 * lr)
        np.testing.assert_allclose(strided(eng.to_tensors(eng.state_m), g["stride"]), g["adam_m_d"], rtol=1e-3,
                                   atol=max(1e-7, 2e-7 * float(np.abs(g["adam_m_d"]).max())))
        np.testing.assert_allclose(strided(eng.to_tensors(eng.state_v), g["stride"]), g["adam_v_d"], rtol=1e-3, atol=1e-10)
        assert eng.optim_step == int(g["adam_step_d"])


# ---- through HipGAIL ------------------------------------------------------------------------------------------------------------
def _tensors(mod, head, extra=()):
    lin = [m for m in mod.preprocess.model.model if isinstance(m, nn.Linear)] + [m for m in head.modules() if isinstance(m, nn.Linear)]
    return [p for m in lin for p in (m.weight, m.bias)] + list(extra)


def build(g, gail=True, **kw):
    """(algorithm, actor / critic / discriminator tensors, rollout buffer) with the fixture's initial weights."""
    from tianshou_amd.integration import make_hip_gail, make_hip_ppo

    c = g["cfg"]
    act_cls = ACT_CLS[g["act_name"]]
    actor = SG.ContinuousActorProbabilistic(SG.Net(g["obs_dim"], [int(h) for h in g["hidden_a"]], act_cls), g["act_dim"], unbounded=True)
    critic = SG.ContinuousCritic(SG.Net(g["obs_dim"], [int(h) for h in g["hidden_c"]], act_cls))
    disc = SG.ContinuousCritic(SG.Net(g["obs_dim"] + g["act_dim"], [int(h) for h in g["hidden_d"]], ACT_CLS[g["disc_act"]]))
    pa, pc, pd = _tensors(actor, actor.mu, [actor.sigma_param]), _tensors(critic, critic.last), _tensors(disc, disc.last)
    with torch.no_grad():
        for name, par in (("a", pa), ("c", pc), ("d", pd)):
            for i, p in enumerate(par):
                p.copy_(torch.from_numpy(g[f"{name}{i}_0"]))
    ppo_kw = dict(eps_clip=c["eps_clip"], dual_clip=c["dual_clip"] or None, value_clip=bool(c["value_clip"]),
                  advantage_normalization=bool(c["advantage_normalization"]), vf_coef=c["vf_coef"], ent_coef=c["ent_coef"],
                  max_grad_norm=c["max_grad_norm"] or None, return_scaling=bool(c["return_scaling"]), gae_lambda=c["gae_lambda"],
                  gamma=c["gamma"], lr=c["lr"])
    kw.setdefault("permutations", "host")
    policy = SG.Policy(actor, action_space=SG.Box(-1.0, 1.0, (g["act_dim"],)))
    if gail:
        expert = SG.ExpertBuffer(g["expert_obs"], g["expert_act"], random_seed=g["expert_seed"])
        algo = make_hip_gail(ref=SG)(policy=policy, critic=critic, expert_buffer=expert, disc_net=disc, disc_lr=c["disc_lr"],
                                     disc_max_grad_norm=c["disc_max_grad_norm"] or None, disc_update_num=g["num"], device="cuda",
                                     **ppo_kw, **kw).to("cuda")
    else:
        algo = make_hip_ppo("ppo", ref=SG)(policy=policy, critic=critic, device="cuda", **ppo_kw, **kw).to("cuda")
    E, T = g["E"], g["T"]
    buf = SG.VectorReplayBuffer(E * T, E, obs_shape=(g["obs_dim"],), act_shape=(g["act_dim"],))
    size = buf.maxsize // E
    for t in range(T):                                   # slot e * size + t of the fixture's buffer = env e, step t
        rows = np.arange(E) * size + t
        buf.add(SG.Batch(obs=g["obs"][rows], act=g["act"][rows], rew=g["rew"][rows], terminated=g["terminated"][rows],
                         truncated=g["truncated"][rows], obs_next=g["obs_next"][rows]))
    assert np.array_equal(buf.sample_indices(0), g["u0_pre_indices"])
    algo.policy.is_within_training_step = True
    return algo, (pa, pc, pd), buf


def check_update(g, u, algo, pars, stats):
    c, pa, pc, pd = g["cfg"], *pars
    np.testing.assert_allclose(algo._hip_gail_rew.cpu().numpy(), g[f"u{u}_pre_rew"], rtol=1e-5, atol=2e-6)
    b = algo._hip_batch
    np.testing.assert_allclose(b["v_s"].cpu().numpy(), g[f"u{u}_pre_v_s"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(b["returns"].cpu().numpy(), g[f"u{u}_pre_returns"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(b["adv"].cpu().numpy(), g[f"u{u}_pre_adv"], rtol=1e-5, atol=1e-5)
    assert type(stats).__name__ == "GailTrainingStats" and stats.gradient_steps == int(g[f"u{u}_gradient_steps"])
    seq = SG.SequenceSummaryStats.from_sequence
    for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
        ref = seq(g[f"u{u}_losses"][:, col])
        np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=2e-5, atol=2e-6)
    ref = seq(g[f"u{u}_disc_stats"][:, 0])
    np.testing.assert_allclose([stats.disc_loss.mean, stats.disc_loss.max, stats.disc_loss.min], [ref.mean, ref.max, ref.min],
                               rtol=2e-5, atol=2e-6)
    assert stats.acc_pi == seq(g[f"u{u}_disc_stats"][:, 1]) and stats.acc_exp == seq(g[f"u{u}_disc_stats"][:, 2])
    for name, par, lr in (("a", pa, c["lr"]), ("c", pc, c["lr"]), ("d", pd, c["disc_lr"])):
        np.testing.assert_allclose(strided(par, g["stride"]), g[f"u{u}_{name}"], rtol=1e-4, atol=0.02 * lr, err_msg=name)


def check_moments(g, algo, pars):
    pa, pc, pd = pars
    algo.state_dict()                                     # the moments arrive lazily
    for name, opt, par in (("ac", algo.optim._optim, pa + pc), ("d", algo.disc_optim._optim, pd)):
        m = strided([opt.state[p]["exp_avg"] for p in par], g["stride"])
        v = strided([opt.state[p]["exp_avg_sq"] for p in par], g["stride"])
        np.testing.assert_allclose(m, g[f"adam_m_{name}"], rtol=1e-3, atol=max(1e-6, 2e-7 * float(np.abs(g[f"adam_m_{name}"]).max())))
        np.testing.assert_allclose(v, g[f"adam_v_{name}"], rtol=1e-3, atol=1e-8)
        assert all(float(opt.state[p]["step"]) == int(g[f"adam_step_{name}"]) for p in par)
        assert all(opt.state[p]["exp_avg"].shape == p.shape for p in par)


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_hip_gail_replays_the_reference(tag):
    """make_hip_gail(ref=standin_gail) with permutations="host", NumPy's generator and the expert buffer's seeded as the fixture
    records: both updates reproduce the reference's rewards, returns / advantages, GailTrainingStats, the parameters of all three
    networks and, at the end, both optimizers' moments."""
    g = load_gail(tag)
    algo, pars, buf = build(g)
    kind = {"mujoco": "fused", "odd": "net"}[tag]
    assert algo._hip_dims[3] == kind
    np.random.seed(g["seed"] + 100)
    for u in range(g["n_updates"]):
        stats = algo.update(buf, g["batch_size"], g["repeat"])
        check_update(g, u, algo, pars, stats)
        assert torch.equal(algo.disc_net.last.model[0].bias.detach().cpu(), algo._hip_engine.gail.to_tensors()[-1].cpu())
    check_moments(g, algo, pars)
    assert algo._hip_engine.gail.optim_step == int(g["adam_step_d"]) and algo._hip_engine.adam_step == int(g["adam_step_ac"])


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_checkpoint_has_the_reference_keys_and_a_fresh_object_resumes(tag):
    """state_dict() after the first update: the stand-in GAIL's (= the reference's, tests/test_gail_shim.py) keys; a fresh HipGAIL
    loaded from it, with the generators where the first object left them, continues to the fixture's second update."""
    g = load_gail(tag)
    algo, pars, buf = build(g)
    np.random.seed(g["seed"] + 100)
    algo.update(buf, g["batch_size"], g["repeat"])
    sd = algo.state_dict()
    plain = SG.GAIL(policy=SG.Policy(SG.ContinuousActorProbabilistic(SG.Net(g["obs_dim"], [int(h) for h in g["hidden_a"]], nn.Tanh), g["act_dim"])),
                    critic=SG.ContinuousCritic(SG.Net(g["obs_dim"], [int(h) for h in g["hidden_c"]], nn.Tanh)), expert_buffer=None,
                    disc_net=SG.ContinuousCritic(SG.Net(g["obs_dim"] + g["act_dim"], [int(h) for h in g["hidden_d"]], ACT_CLS[g["disc_act"]])))
    assert set(sd) == set(plain.state_dict()) and len(sd["_optimizers"]) == 2
    assert [int(float(next(iter(o["state"].values()))["step"])) for o in sd["_optimizers"]] == \
        [int(g["u0_gradient_steps"]), int(g["adam_step_d"]) // g["n_updates"]]
    plain.load_state_dict(sd, strict=True)
    np_state, ex_state = np.random.get_state(), algo.expert_buffer._random_state.get_state()
    fresh, pars2, buf2 = build(g)
    fresh.load_state_dict(algo.state_dict(), strict=True)
    fresh.ret_rms.mean, fresh.ret_rms.var, fresh.ret_rms.count = algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count
    np.random.set_state(np_state)
    fresh.expert_buffer._random_state.set_state(ex_state)
    stats = fresh.update(buf2, g["batch_size"], g["repeat"])
    check_update(g, 1, fresh, pars2, stats)
    check_moments(g, fresh, pars2)


@pytest.mark.parametrize("tag", ["mujoco", "odd"])
def test_the_ppo_half_is_hip_ppos(tag):
    """A HipPPO given the rewards HipGAIL computed, the same state and the same permutations produces the same losses and
    parameters bit for bit."""
    g = load_gail(tag)
    gail, (ga, gc, _), buf = build(g)
    ppo, (pa, pc, _), buf2 = build(g, gail=False)
    np.random.seed(5)
    s_g = gail.update(buf, g["batch_size"], g["repeat"])
    rew = gail._hip_gail_rew.clone()
    ppo._hip_rewards = lambda eng, obs, act, r: rew            # the float32 rewards, as HipGAIL feeds them
    np.random.seed(5)
    np.random.permutation(g["N"])                              # (HipGAIL's split permutation comes first)
    s_p = ppo.update(buf2, g["batch_size"], g["repeat"])
    for k in ("loss", "actor_loss", "vf_loss", "ent_loss"):
        assert getattr(s_g, k) == getattr(s_p, k), k
    assert s_g.gradient_steps == s_p.gradient_steps
    for a, b in zip(ga + gc, pa + pc):
        assert torch.equal(a, b)
    assert torch.equal(gail._hip_engine.params, ppo._hip_engine.params) and torch.equal(gail._hip_engine.adam_m, ppo._hip_engine.adam_m)


def test_device_permutations_are_keyed_and_leave_the_host_generators_alone():
    g = load_gail("odd")
    out = []
    for _ in range(2):
        algo, pars, buf = build(g, permutations="device", perm_seed=1234)
        np.random.seed(77)
        before, ex_before = np.random.get_state(), algo.expert_buffer._random_state.get_state()
        stats = [algo.update(buf, g["batch_size"], g["repeat"]) for _ in range(2)]
        after, ex_after = np.random.get_state(), algo.expert_buffer._random_state.get_state()
        assert all(np.array_equal(a, b) for a, b in zip(before, after) if isinstance(a, np.ndarray)) and before[2:] == after[2:]
        assert all(np.array_equal(a, b) for a, b in zip(ex_before, ex_after) if isinstance(a, np.ndarray))
        assert algo.hip_extra_state()["updates"] == 2 and algo.hip_extra_state()["perm_seed"] == 1234
        out.append(([p.detach().clone() for par in pars for p in par], stats))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    for s, t in zip(out[0][1], out[1][1]):
        assert s.disc_loss == t.disc_loss and s.acc_pi == t.acc_pi and s.loss == t.loss
    other, pars3, buf3 = build(g, permutations="device", perm_seed=99)
    s3 = other.update(buf3, g["batch_size"], g["repeat"])
    assert s3.disc_loss != out[0][1][0].disc_loss                # another key, another shuffle


def test_fewer_rows_than_discriminator_updates_is_a_value_error():
    g = load_gail("odd")
    algo, pars, buf = build(g)
    algo.disc_update_num = g["N"] + 1
    before = [p.detach().clone() for p in pars[2]]
    with pytest.raises(ValueError, match="disc_update_num"):
        algo.update(buf, g["batch_size"], g["repeat"])
    assert all(torch.equal(a, b) for a, b in zip(before, pars[2])) and algo._hip_engine.gail.optim_step == 0
