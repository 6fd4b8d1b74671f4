"""GPU: the Hip* hook bodies of tianshou_amd/integration.py driving the REAL engine on an MI355X.

The reference package is absent on the GPU box, so the subclasses are built over the stand-ins of tests/standin.py
(same attribute surface as the reference classes, verified against them in tests/test_standin_surface.py where the
reference is mounted).  What runs here is the production glue: device mirror of a host-filled buffer, incremental
sync, `sample_indices(0)` / gathers / cut positions as kernels, engine creation from torch modules + optimizer,
the per-update learning-rate refresh (schedulers), parameter write-back, lazy Adam-state flush into
`state_dict()`, `load_state_dict` invalidation.  Checked against the CPU oracle (oracle/oracle_ppo.py) fed with the
same host data, permutations and learning rates."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from oracle import oracle as O
from oracle import oracle_ppo as OP
from tests import lazy_twins as LT
from tests import standin as SI

pytestmark = pytest.mark.gpu


def _make_ppo(obs_dim, act_dim, seed, device, hidden=64, algo="ppo", **kw):
    from tianshou_amd.integration import make_hip_ppo

    HipPPO = make_hip_ppo(algo, ref=SI)
    torch.manual_seed(seed)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [hidden, hidden], nn.Tanh), act_dim, unbounded=True)
    critic = SI.ContinuousCritic(SI.Net(obs_dim, [hidden, hidden], nn.Tanh))
    with torch.no_grad():
        actor.sigma_param.fill_(-0.5)
        for p in actor.mu.parameters():
            p.mul_(0.1)
    policy = SI.Policy(actor)
    kw.setdefault("permutations", "host")          # the seed-exact mode: np.random.permutation like Batch.split
    algo = HipPPO(policy=policy, critic=critic, device=device, **kw)
    return algo.to(device) if device != "cpu" else algo


def _oracle_params(algo):
    from tianshou_amd.ppo import flat_from_modules

    flat = flat_from_modules(algo.policy.actor, algo.critic, device="cpu")
    obs_dim, act_dim, hidden, _ = algo._hip_dims
    return OP.unflatten_params(flat.clone(), obs_dim, act_dim, hidden)


_fill = LT.fill_vector


def _oracle_update(st, ocfg, buf, batch_size, repeat, perms):
    idx = buf.sample_indices(0)
    bs = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths,
                       np.asarray([b._insertion_idx for b in buf.buffers]), buf.rew, buf.terminated, buf.truncated)
    assert np.array_equal(bs.sample_indices_all(), idx)
    unf = bs.unfinished_index()
    assert np.array_equal(unf, buf.unfinished_index())
    args = (torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.obs_next[idx]), torch.from_numpy(buf.act[idx]),
            buf.rew[idx], buf.terminated[idx], buf.truncated[idx], idx, unf)
    pre = OP.preprocess(st, ocfg, *args)
    return OP.update(st, ocfg, {"obs": args[0], "act": args[2]}, pre, batch_size, repeat, perms)


@pytest.mark.parametrize("module_device", ["cuda", "cpu"])
def test_hip_ppo_hooks_with_scheduler_against_oracle(module_device):
    """Four update() calls with a linearly decaying learning rate (mujoco_ppo.py's default), a buffer that is reset
    and refilled between updates (on-policy pattern) and, once, only partly refilled; torch modules living on the
    GPU or on the host."""
    obs_dim, act_dim, E, T, batch_size, repeat = 17, 6, 6, 40, 64, 2
    kw = dict(eps_clip=0.2, value_clip=True, vf_coef=0.25, ent_coef=0.0, max_grad_norm=0.5, return_scaling=True,
              advantage_normalization=False, lr=3e-4)
    algo = _make_ppo(obs_dim, act_dim, 3, "cuda", lr_lambda=lambda k: 1.0 - k / 6.0, **kw)
    if module_device == "cpu":
        algo.to("cpu")                       # parameters on the host, engine on the GPU: write-back crosses PCIe
    st = OP.PPOState(params=_oracle_params(algo))
    ocfg = OP.PPOConfig(max_batchsize=4096, **kw)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    rng = np.random.default_rng(0)
    algo.policy.is_within_training_step = True
    for u in range(4):
        if u != 2:
            buf.reset()
            _fill(buf, T, obs_dim, act_dim, rng)
        else:
            _fill(buf, 7, obs_dim, act_dim, rng)          # ring wrap: sample_indices(0) is no longer arange
        n = len(buf)
        np.random.seed(100 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        ocfg.lr = 3e-4 * (1.0 - u / 6.0)
        assert algo.optim._optim.param_groups[0]["lr"] == pytest.approx(ocfg.lr, rel=1e-12)
        losses_o = _oracle_update(st, ocfg, buf, batch_size, repeat, perms)
        np.random.seed(100 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert stats.gradient_steps == losses_o.shape[0] and stats.train_time > 0
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(losses_o[:, col])
            np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=1e-5, atol=2e-6)
        from tianshou_amd.ppo import flat_from_modules

        flat = flat_from_modules(algo.policy.actor, algo.critic, device="cpu").numpy()
        np.testing.assert_allclose(flat, OP.flatten_params(st.params).numpy(), rtol=1e-4, atol=3e-6)
        np.testing.assert_allclose([algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count],
                                   [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)
        assert next(algo.policy.actor.parameters()).device.type == module_device
    # Algorithm.state_dict(): Adam moments arrive lazily, in the reference's per-parameter layout
    params = algo._hip_params()
    assert all(p not in algo.optim._optim.state for p in params)
    sd = algo.state_dict()
    assert len(sd["_optimizers"][0]["state"]) == len(params)
    state = algo.optim._optim.state               # keyed by parameter (state_dict() numbers them in optimizer order)
    m_flat = torch.cat([state[p]["exp_avg"].reshape(-1).cpu() for p in params]).numpy()
    v_flat = torch.cat([state[p]["exp_avg_sq"].reshape(-1).cpu() for p in params]).numpy()
    m_ref = torch.cat([st.adam_m[k].reshape(-1) for k in OP.PARAM_ORDER]).numpy()
    v_ref = torch.cat([st.adam_v[k].reshape(-1) for k in OP.PARAM_ORDER]).numpy()
    np.testing.assert_allclose(m_flat, m_ref, rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(v_flat, v_ref, rtol=1e-3, atol=1e-10)
    assert all(float(state[p]["step"]) == st.adam_step for p in params)
    assert all(state[p]["exp_avg"].device == p.device and state[p]["exp_avg"].shape == p.shape for p in params)


def test_hip_a2c_hooks_against_oracle():
    """HipA2C (make_hip_ppo("a2c") over the stand-ins) on the real engine: the same preprocessing as PPO without logp_old
    (a2c.py:239-247), loss -(logp adv).mean() + vf_coef mse - ent_coef entropy per minibatch (:262-273), joint clipping of the
    actor-critic gradient, three updates on a refilled buffer."""
    obs_dim, act_dim, E, T, batch_size, repeat = 11, 3, 6, 40, 48, 2
    kw = dict(vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, return_scaling=False, gae_lambda=0.9, gamma=0.98, lr=7e-4)
    algo = _make_ppo(obs_dim, act_dim, 8, "cuda", algo="a2c", **kw)
    assert type(algo).__name__ == "HipA2C" and not hasattr(algo, "eps_clip")
    st = OP.PPOState(params=_oracle_params(algo))
    ocfg = OP.PPOConfig(algo="a2c", max_batchsize=4096, **kw)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    rng = np.random.default_rng(6)
    algo.policy.is_within_training_step = True
    for u in range(3):
        buf.reset()
        _fill(buf, T - 5 * u, obs_dim, act_dim, rng)
        n = len(buf)
        np.random.seed(200 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        losses_o = _oracle_update(st, ocfg, buf, batch_size, repeat, perms)
        np.random.seed(200 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert stats.gradient_steps == losses_o.shape[0]
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(losses_o[:, col])
            np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=1e-5, atol=2e-6)
        from tianshou_amd.ppo import flat_from_modules

        flat = flat_from_modules(algo.policy.actor, algo.critic, device="cpu").numpy()
        np.testing.assert_allclose(flat, OP.flatten_params(st.params).numpy(), rtol=1e-4, atol=5e-6)


def _mujoco_nets(obs_dim, act_dim, seed):
    torch.manual_seed(seed)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [64, 64], nn.Tanh), act_dim, unbounded=True)
    critic = SI.ContinuousCritic(SI.Net(obs_dim, [64, 64], nn.Tanh))
    with torch.no_grad():
        actor.sigma_param.fill_(-0.5)
    return actor, critic


def _flat_oracle_params(actor, critic, obs_dim, act_dim):
    from tianshou_amd.ppo import flat_from_modules

    return OP.unflatten_params(flat_from_modules(actor, critic, device="cpu").clone(), obs_dim, act_dim, 64)


def _oracle_batch(buf):
    idx = buf.sample_indices(0)
    bs = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths,
                       np.asarray([b._insertion_idx for b in buf.buffers]), buf.rew, buf.terminated, buf.truncated)
    return idx, bs.unfinished_index()


@pytest.mark.parametrize("which", ["npg", "trpo"])
def test_hip_natural_gradient_hooks_against_oracle(which):
    """HipNPG / HipTRPO (integration.make_hip_npg / make_hip_trpo over the stand-ins) on the real engine: preprocessing with
    normalised advantages and log pi_old (npg.py:123-137), per minibatch the conjugate-gradient natural step (TRPO: with the
    line search, trpo.py:123-214) and `optim_critic_iters` critic steps, write-back of actor + critic + the critic's Adam
    state; two updates against oracle_npg (tolerances of tests/test_gpu_npg.py: both sides are float32 CG solves)."""
    from oracle import oracle_npg as ON
    from tianshou_amd.integration import make_hip_npg, make_hip_trpo

    obs_dim, act_dim, E, T, batch_size, repeat = 17, 6, 6, 60, 128, 1
    Hip = (make_hip_npg if which == "npg" else make_hip_trpo)(ref=SI)
    actor, critic = _mujoco_nets(obs_dim, act_dim, 41)
    kw = dict(lr=1e-3, optim_critic_iters=3, advantage_normalization=True, gae_lambda=0.95, gamma=0.99, return_scaling=True)
    if which == "npg":
        kw["trust_region_size"] = 0.1
    else:
        kw.update(max_kl=0.01, backtrack_coeff=0.8, max_backtracks=10)
    algo = Hip(policy=SI.Policy(actor), critic=critic, device="cuda", **kw).to("cuda")
    assert type(algo).__name__ == ("HipNPG" if which == "npg" else "HipTRPO")
    st = OP.PPOState(params=_flat_oracle_params(actor, critic, obs_dim, act_dim))
    ocfg = ON.NPGConfig(algo=which, gamma=0.99, gae_lambda=0.95, optim_critic_iters=3, trust_region_size=0.1,
                        advantage_normalization=True, return_scaling=True, max_batchsize=4096, lr=1e-3)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    rng = np.random.default_rng(42)
    algo.policy.is_within_training_step = True
    for u in range(2):
        buf.reset()
        _fill(buf, T - 9 * u, obs_dim, act_dim, rng)
        n = len(buf)
        idx, unf = _oracle_batch(buf)
        p_before = OP.flatten_params(st.params).numpy().copy()
        np.random.seed(90 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        obs, act = torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx])
        pre = ON.preprocess(st, ocfg, obs, torch.from_numpy(buf.obs_next[idx]), act, buf.rew[idx], buf.terminated[idx],
                            buf.truncated[idx], idx, unf)
        ref = ON.update(st, ocfg, obs, act, pre, batch_size, repeat, perms)
        np.random.seed(90 + u)
        stats = algo.update(buf, batch_size, repeat)
        cols = [stats.actor_loss, stats.vf_loss, stats.kl] + ([stats.step_size] if which == "trpo" else [])
        for col, s in enumerate(cols):
            r = SI.SequenceSummaryStats.from_sequence(ref[:, col])
            np.testing.assert_allclose([s.mean, s.max, s.min], [r.mean, r.max, r.min], rtol=2e-3, atol=2e-5)
        from tianshou_amd.ppo import flat_from_modules

        flat = flat_from_modules(actor, critic, device="cpu").numpy()
        want = OP.flatten_params(st.params).numpy()
        assert np.abs(flat - want).max() < 5e-3 * np.abs(want - p_before).max()
        np.testing.assert_allclose([algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count],
                                   [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)
    state = algo.optim._optim.state
    w = critic.preprocess.model.model[0].weight
    assert float(state[w]["step"]) == st.adam_step and state[w]["exp_avg"].shape == w.shape
    assert all(p not in state for p in actor.parameters())                  # the optimizer holds the critic only


def test_hip_reinforce_hooks_against_oracle():
    """HipReinforce (integration.make_hip_reinforce over the stand-ins) on the real engine: discounted returns with the
    running standardisation (reinforce.py:273-309), per minibatch -(log pi * G).mean() and clip + Adam on the actor
    (:346-382); three updates against oracle_reinforce."""
    from oracle import oracle_reinforce as OR
    from tianshou_amd.integration import make_hip_reinforce

    obs_dim, act_dim, E, T, batch_size, repeat = 11, 3, 6, 50, 64, 2
    HipReinforce = make_hip_reinforce(ref=SI)
    actor, critic = _mujoco_nets(obs_dim, act_dim, 43)                     # (the critic only completes the oracle's parameter set)
    st = OP.PPOState(params=_flat_oracle_params(actor, critic, obs_dim, act_dim))
    algo = HipReinforce(policy=SI.Policy(actor), lr=1e-3, gamma=0.97, return_standardization=True, max_grad_norm=0.7,
                        device="cuda").to("cuda")
    ocfg = OR.ReinforceConfig(gamma=0.97, return_standardization=True, lr=1e-3, max_grad_norm=0.7)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    rng = np.random.default_rng(44)
    algo.policy.is_within_training_step = True
    for u in range(3):
        buf.reset()
        _fill(buf, T - 6 * u, obs_dim, act_dim, rng)
        n = len(buf)
        idx, unf = _oracle_batch(buf)
        np.random.seed(110 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        ret = OR.preprocess(st, ocfg, buf.rew[idx], buf.terminated[idx], buf.truncated[idx], idx, unf)
        ref = OR.update(st, ocfg, torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx]), ret, batch_size, repeat, perms)
        np.random.seed(110 + u)
        stats = algo.update(buf, batch_size, repeat)
        r = SI.SequenceSummaryStats.from_sequence(ref)
        np.testing.assert_allclose([stats.loss.mean, stats.loss.max, stats.loss.min], [r.mean, r.max, r.min], rtol=2e-5, atol=2e-6)
        drc = algo.discounted_return_computation
        np.testing.assert_allclose([drc.ret_rms.mean, drc.ret_rms.var, drc.ret_rms.count],
                                   [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)
    from tianshou_amd.ppo import TIANSHOU_ACTOR_KEYS

    sd = actor.state_dict()
    for name, k in zip(TIANSHOU_ACTOR_KEYS, ["a_w1", "a_b1", "a_w2", "a_b2", "a_wmu", "a_bmu", "a_sigma"]):
        np.testing.assert_allclose(sd[name].cpu().numpy().reshape(-1), st.params[k].numpy().reshape(-1), rtol=1e-5,
                                   atol=0.05 * 1e-3, err_msg=name)
    state = algo.optim._optim.state
    assert float(state[actor.sigma_param]["step"]) == st.adam_step


def test_hip_ppo_hooks_on_humanoid_shape_use_the_gemm_path():
    """Net[256, 256], obs 376, act 17 (Humanoid; outside the fused kernels' envelope): HipPPO picks WidePPOEngine and the
    whole hook path - mirror, preprocess, update, write-back, Adam flush - matches the oracle."""
    from tianshou_amd.ppo_wide import WidePPOEngine

    obs_dim, act_dim, hidden, E, T, batch_size, repeat = 376, 17, 256, 4, 48, 64, 2
    kw = dict(eps_clip=0.2, value_clip=True, vf_coef=0.25, ent_coef=0.01, max_grad_norm=0.5, return_scaling=True,
              advantage_normalization=True, lr=3e-4)
    algo = _make_ppo(obs_dim, act_dim, 5, "cuda", hidden=hidden, **kw)
    assert algo._hip_dims == (obs_dim, act_dim, hidden, "wide")
    sa, sc = algo.policy.actor.state_dict(), algo.critic.state_dict()
    from tianshou_amd.ppo import TIANSHOU_ACTOR_KEYS, TIANSHOU_CRITIC_KEYS

    params = {k: t.detach().cpu().clone().reshape(OP.param_shapes(obs_dim, act_dim, hidden)[k])
              for k, t in zip(OP.PARAM_ORDER, [sa[k] for k in TIANSHOU_ACTOR_KEYS] + [sc[k] for k in TIANSHOU_CRITIC_KEYS])}
    st = OP.PPOState(params=params)
    ocfg = OP.PPOConfig(max_batchsize=4096, **kw)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    rng = np.random.default_rng(2)
    algo.policy.is_within_training_step = True
    for u in range(2):
        buf.reset()
        _fill(buf, T, obs_dim, act_dim, rng)
        np.random.seed(7 + u)
        perms = [np.random.permutation(len(buf)) for _ in range(repeat)]
        losses_o = _oracle_update(st, ocfg, buf, batch_size, repeat, perms)
        np.random.seed(7 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert isinstance(algo._hip_engine, WidePPOEngine) and stats.gradient_steps == losses_o.shape[0]
        for col, s_ in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(losses_o[:, col])
            np.testing.assert_allclose([s_.mean, s_.max, s_.min], [ref.mean, ref.max, ref.min], rtol=1e-5, atol=2e-6)
        sa, sc = algo.policy.actor.state_dict(), algo.critic.state_dict()
        for k, t in zip(OP.PARAM_ORDER, [sa[k] for k in TIANSHOU_ACTOR_KEYS] + [sc[k] for k in TIANSHOU_CRITIC_KEYS]):
            np.testing.assert_allclose(t.cpu().numpy().reshape(-1), st.params[k].numpy().reshape(-1), rtol=1e-4,
                                       atol=0.02 * 3e-4, err_msg=k)
    algo.state_dict()
    state = algo.optim._optim.state
    for p_, k in zip(algo._hip_params(), OP.PARAM_ORDER):
        np.testing.assert_allclose(state[p_]["exp_avg"].cpu().numpy().reshape(-1), st.adam_m[k].numpy().reshape(-1),
                                   rtol=1e-3, atol=1e-7, err_msg=k)
        assert float(state[p_]["step"]) == st.adam_step


def test_hip_ppo_load_state_dict_rebuilds_the_engine():
    """restoring a checkpoint must not be overwritten by stale engine state at the next write-back."""
    obs_dim, act_dim, E, T = 11, 3, 4, 32
    kw = dict(eps_clip=0.2, value_clip=False, vf_coef=0.5, ent_coef=0.01, max_grad_norm=None, return_scaling=False,
              advantage_normalization=True, lr=1e-3)
    algo = _make_ppo(obs_dim, act_dim, 9, "cuda", **kw)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    _fill(buf, T, obs_dim, act_dim, np.random.default_rng(1))
    algo.policy.is_within_training_step = True
    np.random.seed(0)
    algo.update(buf, 32, 1)
    ckpt = copy.deepcopy(algo.state_dict())
    np.random.seed(1)
    s1 = algo.update(buf, 32, 2)
    assert algo._hip_engine is not None
    algo.load_state_dict(copy.deepcopy(ckpt))
    assert algo._hip_engine is None                       # dropped; rebuilt from the loaded modules + optimizer
    np.random.seed(1)
    s2 = algo.update(buf, 32, 2)                          # same data, same permutations, same restored state
    assert s1.loss.mean == s2.loss.mean and s1.vf_loss.max == s2.vf_loss.max
    # loading into a sub-module only (algorithm.policy.load_state_dict) is caught as well (parameter version counters),
    # and -- ADVICE r2 -- the engine's Adam moments are flushed into torch.optim first, so the rebuilt engine continues
    # from them instead of restarting the bias correction from zero moments
    eng = algo._hip_engine
    step_before, m_before = eng.adam_step, eng.adam_m.clone()
    assert step_before > 0 and float(m_before.abs().max()) > 0
    algo.policy.load_state_dict(copy.deepcopy(algo.policy.state_dict()))
    assert algo._hip_engine is None
    rebuilt = algo._engine()
    assert rebuilt is not eng and rebuilt.adam_step == step_before and torch.equal(rebuilt.adam_m, m_before)
    import pickle

    pickle.dumps(algo.policy)                             # sub-modules carry no closures (persistence.py:106 saves the policy)
    assert not algo.policy._load_state_dict_post_hooks


def test_full_c2_configuration_against_oracle():
    """The exact BASELINE.json configs[1] shape end to end: 512 envs x 2048 steps = 2^20 transitions, obs 17, act 6,
    one repeat of 16 minibatches of 65,536 with a host permutation, preprocessing included; per-step losses vs the
    CPU oracle at rtol 1e-5 (north_star), final parameters on the scale of the Adam steps taken."""
    from tianshou_amd import ppo as P

    E, T, obs_dim, act_dim, batch = 512, 2048, 17, 6, 65536
    n = E * T
    rng = np.random.default_rng(2024)
    params = OP.init_params(obs_dim, act_dim, seed=0)
    g = torch.Generator().manual_seed(1)
    for k in params:
        params[k] = params[k] + 0.02 * torch.randn(params[k].shape, generator=g)
    data = dict(obs=rng.normal(size=(n, obs_dim)).astype(np.float32),
                obs_next=rng.normal(size=(n, obs_dim)).astype(np.float32),
                act=rng.normal(size=(n, act_dim)).astype(np.float32),
                rew=rng.normal(size=n).astype(np.float32).astype(np.float64),
                terminated=rng.random(n) < 0.005, truncated=np.zeros(n, bool))
    data["truncated"].reshape(E, T)[:, 999::1000] = True
    data["truncated"] &= ~data["terminated"]
    kw = dict(eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, max_grad_norm=0.5, value_clip=True,
              advantage_normalization=False, return_scaling=True, lr=3e-4)
    ocfg, cfg = OP.PPOConfig(max_batchsize=65536, **kw), P.PPOConfig(**kw)
    perms = [rng.permutation(n)]
    torch.set_num_threads(min(32, torch.get_num_threads() or 8))
    st = OP.PPOState(params={k: v.clone() for k, v in params.items()})
    bs = O.BufferState.from_vector_fill(data["rew"], data["terminated"], data["truncated"], E)
    idx, unf = bs.sample_indices_all(), bs.unfinished_index()
    args = (torch.from_numpy(data["obs"]), torch.from_numpy(data["obs_next"]), torch.from_numpy(data["act"]),
            data["rew"], data["terminated"], data["truncated"], idx, unf)
    pre_o = OP.preprocess(st, ocfg, *args)
    losses_o = OP.update(st, ocfg, {"obs": args[0], "act": args[2]}, pre_o, batch, 1, perms)
    assert losses_o.shape == (16, 4)

    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")   # noqa: E731
    eng = P.PPOEngine(obs_dim, act_dim, OP.flatten_params(params).cuda(), cfg)
    b = eng.preprocess(dev(data["obs"]), dev(data["obs_next"]), dev(data["act"]), dev(data["rew"]),
                       dev(data["terminated"]), dev(data["truncated"]), dev(unf))
    np.testing.assert_allclose(b["v_s"].cpu().numpy(), pre_o["v_s"].numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(b["adv"].cpu().numpy(), pre_o["adv"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(b["returns"].cpu().numpy(), pre_o["returns"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(b["logp_old"].cpu().numpy(), pre_o["logp_old"].numpy(), rtol=1e-5, atol=1e-5)
    losses, steps = eng.update(b, batch, 1, perms)
    eng.check()
    assert steps == 16
    np.testing.assert_allclose(losses.cpu().numpy(), losses_o, rtol=1e-5, atol=1e-6)
    # 16 Adam steps of lr 3e-4: parameters on the scale of a fraction of one step (atol = 0.02 lr)
    np.testing.assert_allclose(eng.params.cpu().numpy(), OP.flatten_params(st.params).numpy(), rtol=1e-4, atol=0.02 * 3e-4)
    np.testing.assert_allclose(eng.ret_rms, [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)


# ------------------------------------------------------------------------------------ HipSAC
def test_hip_sac_hooks_against_oracle():
    """HipSAC (integration.make_hip_sac over the stand-ins) on the real engine: incremental device mirror of a growing
    host buffer, random minibatch from the buffer's own RandomState, n-step-1 target with the lagged critics, twin-critic
    / actor / auto-alpha steps, Polyak, write-back of five networks + four optimizers - against oracle_sac fed with the
    same indices and the same torch-generator noise."""
    from oracle import oracle_sac as OS
    from tianshou_amd.integration import make_hip_sac

    obs_dim, act_dim, E, B = 23, 5, 4, 64
    HipSAC = make_hip_sac(ref=SI)
    torch.manual_seed(11)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [256, 256], nn.ReLU), act_dim, unbounded=True, conditioned_sigma=True)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
    c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
    alpha = SI.AutoAlpha(-float(act_dim), -0.5, 3e-4)
    # the reference-exact mode: torch's host generator for the rsample() noise, the reference's own Algorithm._update with its host
    # batch, write-back after every update (the defaults -- engine noise, index-only sampling, lazy write-back -- are compared
    # with this mode in test_hip_sac_default_mode_equals_the_reference_exact_mode)
    algo = HipSAC(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=1e-3, tau=0.01, gamma=0.97, alpha=alpha, device="cuda",
                  update_noise="torch", host_batch=True, write_back="eager").to("cuda")
    grab = lambda mod, keys: {k: mod.state_dict()[n].detach().cpu().clone() for k, n in zip(keys, mod.state_dict())}   # noqa: E731
    cfg = OS.SACConfig(gamma=0.97, tau=0.01, n_step=1, auto_alpha=True, target_entropy=-float(act_dim), log_alpha0=-0.5,
                       actor_lr=1e-3, critic_lr=1e-3, alpha_lr=3e-4)
    st = OS.SACState.create(grab(actor, OS.ACTOR_ORDER), grab(c1, OS.CRITIC_ORDER), grab(c2, OS.CRITIC_ORDER), cfg)
    buf = SI.VectorReplayBuffer(E * 200, E, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=4)
    rng = np.random.default_rng(9)
    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, rng)              # the mirror follows the growing buffer
        torch.manual_seed(100 + u)
        stats = algo.update(buf, B)
        idx = seen[-1]
        torch.manual_seed(100 + u)
        noise_t, noise_u = torch.randn(B, act_dim), torch.randn(B, act_dim)
        obs, act = torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx])
        tq = OS.target_q(st, cfg, torch.from_numpy(buf.obs_next[idx]), noise_t).flatten().numpy()
        ret = (buf.rew[idx] + 0.97 * tq.astype(np.float64) * (~buf.terminated[idx])).astype(np.float32)
        ref = OS.update_with_batch(st, cfg, obs, act, ret, noise_u)
        np.testing.assert_allclose([stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.alpha, stats.alpha_loss],
                                   [ref["actor_loss"], ref["critic1_loss"], ref["critic2_loss"], ref["alpha"], ref["alpha_loss"]],
                                   rtol=2e-5, atol=2e-6)
        for mod, want, order in ((actor, st.actor, OS.ACTOR_ORDER), (c1, st.critic1, OS.CRITIC_ORDER), (c2, st.critic2, OS.CRITIC_ORDER),
                                 (algo.critic_old.module, st.critic1_old, OS.CRITIC_ORDER),
                                 (algo.critic2_old.module, st.critic2_old, OS.CRITIC_ORDER)):
            for (name, t), k in zip(mod.state_dict().items(), order):
                np.testing.assert_allclose(t.cpu().numpy(), want[k].numpy(), rtol=1e-4, atol=0.02 * 1e-3, err_msg=f"update {u}: {name}")
        assert abs(float(alpha._log_alpha.detach()) - float(st.log_alpha)) < 0.02 * 3e-4
    w = actor.preprocess.model.model[0].weight
    stt = algo.policy_optim._optim.state[w]
    assert float(stt["step"]) == 4.0 and stt["exp_avg"].shape == w.shape and stt["exp_avg"].device == w.device
    np.testing.assert_allclose(stt["exp_avg"].cpu().numpy(), st.opt_actor.m["w1"].numpy(), rtol=1e-3, atol=1e-7)
    assert len(algo._hip_mirror) == len(buf) and np.array_equal(algo._hip_mirror.rew.cpu().numpy(), buf.rew)


def test_hip_sac_default_mode_equals_the_reference_exact_mode(monkeypatch):
    """The defaults of HipSAC since round 6 -- `update()` samples indices only (no host copy of the batch), write-back of the five
    networks / four optimizers deferred until the torch state is read -- against the reference-exact mode on the same indices
    and noise: identical statistics every update, identical torch state after `hip_sync()`.  And what lazy means: the torch
    modules do not move between syncs; `policy.state_dict()`, `algorithm.state_dict()`, any sub-module's `state_dict()`, pickling
    the policy and `hip_sync()` are readers that sync; a foreign write to ONE module (`critic.load_state_dict`) keeps the engine's progress on the others."""
    import copy
    import pickle

    obs_dim, act_dim, E, B = LT.SAC_OBS, LT.SAC_ACT, LT.SAC_ENVS, LT.SAC_BATCH
    build = LT.sac_build                                           # (update_noise="torch": the reference's stream in both)

    ref, lazy = build(host_batch=True, write_back="eager"), build()
    assert lazy.__dict__["_hip_lazy"] and not ref.__dict__["_hip_lazy"]
    bufs = [LT.sac_buffer() for _ in range(2)]
    rng = [np.random.default_rng(9) for _ in range(2)]
    flat = lambda algo: torch.cat([p.detach().reshape(-1).float().cpu() for p in algo.parameters()])  # noqa: E731
    start = flat(lazy)
    for u in range(4):
        out = []
        for algo, buf, r in zip((ref, lazy), bufs, rng):
            _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, r)
            torch.manual_seed(100 + u)
            out.append(algo.update(buf, B))
        for f in ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss"):
            assert getattr(out[0], f) == getattr(out[1], f), (u, f)
        assert torch.equal(flat(lazy), start)                      # nothing was written back yet
    assert lazy.__dict__["_hip_stale"]
    sd = lazy.policy.state_dict()                                  # a reader: syncs
    assert not lazy.__dict__["_hip_stale"] and torch.equal(flat(lazy), flat(ref)) and not torch.equal(flat(lazy), start)
    assert all(torch.equal(v.cpu(), ref.policy.state_dict()[k].cpu()) for k, v in sd.items())
    w = lazy.policy.actor.preprocess.model.model[0].weight
    st_l, st_r = lazy.policy_optim._optim.state[w], ref.policy_optim._optim.state[ref.policy.actor.preprocess.model.model[0].weight]
    assert float(st_l["step"]) == 4.0 and torch.equal(st_l["exp_avg"], st_r["exp_avg"]) and torch.equal(st_l["exp_avg_sq"], st_r["exp_avg_sq"])
    # one more update each, then: pickling the policy syncs; algorithm.state_dict() syncs
    for algo, buf in zip((ref, lazy), bufs):
        torch.manual_seed(200)
        algo.update(buf, B)
    twin = pickle.loads(pickle.dumps(lazy.policy))
    assert not lazy.__dict__["_hip_stale"] and torch.equal(flat(lazy), flat(ref))
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(twin.state_dict().values(), ref.policy.state_dict().values()))
    for algo, buf in zip((ref, lazy), bufs):
        torch.manual_seed(201)
        algo.update(buf, B)
    assert lazy.__dict__["_hip_stale"]
    c2 = lazy.critic2.state_dict()                                 # a SUB-module's state_dict() is a reader too (pre-hook): syncs
    assert not lazy.__dict__["_hip_stale"] and all(torch.equal(v.cpu(), ref.critic2.state_dict()[k].cpu()) for k, v in c2.items())
    for algo, buf in zip((ref, lazy), bufs):
        torch.manual_seed(204)
        algo.update(buf, B)
    assert lazy.__dict__["_hip_stale"]
    sd_l, sd_r = lazy.state_dict(), ref.state_dict()
    assert not lazy.__dict__["_hip_stale"]
    for k in sd_r:
        if isinstance(sd_r[k], torch.Tensor):
            assert torch.equal(sd_l[k].cpu(), sd_r[k].cpu()), k
    # a foreign write to one module while updates are pending: that module keeps what was loaded, the others what the engine learnt
    for algo, buf in zip((ref, lazy), bufs):
        torch.manual_seed(202)
        algo.update(buf, B)
    loaded = {k: torch.full_like(v, 0.01) for k, v in lazy.critic.state_dict().items()}
    lazy.critic.load_state_dict(copy.deepcopy(loaded))
    ref.critic.load_state_dict(copy.deepcopy(loaded))
    for algo, buf in zip((ref, lazy), bufs):                       # the next hook sees the foreign write and rebuilds the engine
        torch.manual_seed(203)
        algo.update(buf, B)
    lazy.hip_sync()
    assert torch.equal(flat(lazy), flat(ref))


@pytest.mark.parametrize("sizes", [((128, 128), (128, 128)), ((96, 40, 72), (56, 64, 24))], ids=["net_128_128", "three_layers"])
def test_hip_discrete_sac_hooks_against_oracle(sizes):
    """(`three_layers`: round 6, any depth -- actor Net[96, 40, 72], critics Net[56, 64, 24], embedded in Net[96] * 3.)
    HipDiscreteSAC (integration.make_hip_discrete_sac over the stand-ins) on the real engine with Net[128, 128] trunks, 7
    actions, auto-tuned alpha: incremental device mirror of a growing host buffer, n-step-1 target from the expectation under
    the actor with the lagged critics (discrete_sac.py:147-155), critic / actor / alpha steps with the UPDATED critics in
    the actor loss (:157-196), Polyak, write-back of five networks + four optimizers - against oracle_dsac fed with the same
    sampled indices.  (`match_rng_stream` draws the reference's unused Categorical samples; they touch no result.)"""
    from oracle import oracle_dsac as ODS
    from oracle import oracle_sac as OS
    from tianshou_amd.integration import make_hip_discrete_sac

    obs_dim, n_act, E, B = 19, 7, 4, 64
    HipDSAC = make_hip_discrete_sac(ref=SI)
    torch.manual_seed(17)
    actor = SI.DiscreteActor(SI.Net(obs_dim, list(sizes[0]), nn.ReLU), n_act, softmax_output=False)
    c1 = SI.DiscreteCritic(SI.Net(obs_dim, list(sizes[1]), nn.ReLU), last_size=n_act)
    c2 = SI.DiscreteCritic(SI.Net(obs_dim, list(sizes[1]), nn.ReLU), last_size=n_act)
    NET_ORDER = ODS.net_order(len(sizes[0]))
    tgt_ent = 0.98 * float(np.log(n_act))
    alpha = SI.AutoAlpha(tgt_ent, -0.4, 3e-4)
    algo = HipDSAC(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=1e-3, tau=0.02, gamma=0.96, alpha=alpha, device="cuda").to("cuda")
    assert algo._hip_depth == len(sizes[0]) and algo._hip_sizes["critic2"] == tuple(sizes[1])
    grab = lambda mod: {k: t.detach().cpu().clone() for k, t in zip(NET_ORDER, mod.state_dict().values())}   # noqa: E731
    cfg = OS.SACConfig(gamma=0.96, tau=0.02, n_step=1, auto_alpha=True, target_entropy=tgt_ent, log_alpha0=-0.4, actor_lr=1e-3,
                       critic_lr=1e-3, alpha_lr=3e-4)
    st = OS.SACState.create(grab(actor), grab(c1), grab(c2), cfg)
    buf = SI.VectorReplayBuffer(E * 200, E, obs_shape=(obs_dim,), act_shape=(), act_dtype=np.int64, seed=12)
    rng = np.random.default_rng(14)

    def fill(T):
        obs = rng.normal(size=(T + 1, E, obs_dim)).astype(np.float32)
        for t in range(T):
            term = rng.random(E) < 0.05
            buf.add(SI.Batch(obs=obs[t], act=rng.integers(0, n_act, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                             truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        fill(30 if u == 0 else 7)                                            # the mirror follows the growing buffer
        stats = algo.update(buf, B)
        idx = seen[-1]
        tq = ODS.target_q(st, cfg, torch.from_numpy(buf.obs_next[idx])).flatten().numpy()
        ret = (buf.rew[idx] + 0.96 * tq.astype(np.float64) * (~buf.terminated[idx])).astype(np.float32)
        ref = ODS.update_with_batch(st, cfg, torch.from_numpy(buf.obs[idx]), buf.act[idx], ret)
        np.testing.assert_allclose([stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.alpha, stats.alpha_loss],
                                   [ref["actor_loss"], ref["critic1_loss"], ref["critic2_loss"], ref["alpha"], ref["alpha_loss"]],
                                   rtol=2e-5, atol=2e-6)
        for mod, want in ((actor, st.actor), (c1, st.critic1), (c2, st.critic2), (algo.critic_old.module, st.critic1_old),
                          (algo.critic2_old.module, st.critic2_old)):
            for (name, t), k in zip(mod.state_dict().items(), NET_ORDER):
                np.testing.assert_allclose(t.cpu().numpy(), want[k].numpy(), rtol=1e-4, atol=0.02 * 1e-3,
                                           err_msg=f"update {u}: {name}")
        assert abs(float(alpha._log_alpha.detach()) - float(st.log_alpha)) < 0.02 * 3e-4
    w = c2.preprocess.model.model[0].weight
    stt = algo.critic2_optim._optim.state[w]
    assert float(stt["step"]) == 4.0 and stt["exp_avg"].shape == w.shape and stt["exp_avg"].device == w.device
    np.testing.assert_allclose(stt["exp_avg"].cpu().numpy(), st.opt_c2.m["l1.w"].numpy(), rtol=1e-3, atol=1e-7)
    assert len(algo._hip_mirror) == len(buf) and np.array_equal(algo._hip_mirror.act.cpu().numpy(), buf.act)


@pytest.mark.parametrize("sizes", [((256, 256), (256, 256)), ((64,), (48,))], ids=["net_256_256", "one_layer"])
def test_hip_redq_hooks_against_oracle(sizes):
    """(`one_layer`: round 6, any depth -- actor Net[64], EnsembleLinear critic [48], embedded in Net[64].)
    HipREDQ (integration.make_hip_redq over the stand-ins) on the real engine, the nets of test/continuous/test_redq.py:86-107
    with 4 ensemble members: target from a random subset of 2 lagged members (redq.py:248-261; torch.randn then
    np.random.choice, in the reference's order), one critic step on the whole ensemble, the actor / alpha step every 2nd
    update against the ensemble mean (:263-304), Polyak, write-back of the actor, both ensembles and three optimizers --
    against oracle_redq fed with the same sampled indices, noise and subsets."""
    from oracle import oracle_redq as ORQ
    from oracle import oracle_sac as OS
    from tianshou_amd.integration import make_hip_redq

    obs_dim, act_dim, E, S, B, H = 11, 3, 4, 2, 64, sizes[1][-1]
    HipREDQ = make_hip_redq(ref=SI)
    torch.manual_seed(61)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, list(sizes[0]), nn.ReLU), act_dim, unbounded=True, conditioned_sigma=True)
    lin = lambda x, y: SI.EnsembleLinear(E, x, y)   # noqa: E731
    critic = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, list(sizes[1]), nn.ReLU, linear_layer=lin), linear_layer=lin)
    A_ORDER, C_ORDER = OS.actor_order(len(sizes[0])), OS.critic_order(len(sizes[1]))
    alpha = SI.AutoAlpha(-float(act_dim), -0.6, 3e-4)
    algo = HipREDQ(policy=SI.Policy(actor), critic=critic, lr=1e-3, critic_lr=1e-3, ensemble_size=E, subset_size=S, tau=0.01,
                   gamma=0.97, alpha=alpha, actor_delay=2, target_mode="min", device="cuda").to("cuda")
    grab = lambda mod, keys: {k: mod.state_dict()[n].detach().cpu().clone() for k, n in zip(keys, mod.state_dict())}   # noqa: E731
    cfg = ORQ.REDQConfig(gamma=0.97, tau=0.01, n_step=1, auto_alpha=True, target_entropy=-float(act_dim), log_alpha0=-0.6,
                         actor_lr=1e-3, critic_lr=1e-3, alpha_lr=3e-4, ensemble_size=E, subset_size=S, actor_delay=2,
                         target_mode="min")
    assert algo._hip_depth == len(sizes[0]) and algo._hip_sizes == {"actor": tuple(sizes[0]), "critic": tuple(sizes[1])}
    st = ORQ.REDQState.create(grab(actor, A_ORDER), grab(critic, C_ORDER), cfg)
    buf = SI.VectorReplayBuffer(E * 200, 4, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=62)
    rng = np.random.default_rng(63)
    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, rng)
        torch.manual_seed(400 + u)
        np.random.seed(500 + u)
        stats = algo.update(buf, B)
        idx = seen[-1]
        torch.manual_seed(400 + u)
        np.random.seed(500 + u)
        noise_t = torch.randn(B, act_dim)
        subset = np.random.choice(E, S, replace=False)
        actor_step = (st.critic_gradient_step + 1) % 2 == 0
        noise_u = torch.randn(B, act_dim) if actor_step else None
        tq = ORQ.target_q(st, cfg, torch.from_numpy(buf.obs_next[idx]), noise_t, subset).flatten().numpy()
        ret = (buf.rew[idx] + 0.97 * tq.astype(np.float64) * (~buf.terminated[idx])).astype(np.float32)
        ref = ORQ.update_with_batch(st, cfg, torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx]), ret, noise_u)
        np.testing.assert_allclose([stats.actor_loss, stats.critic_loss, stats.alpha], [ref["actor_loss"], ref["critic_loss"], ref["alpha"]],
                                   rtol=2e-5, atol=2e-6)
        assert (stats.alpha_loss is None) == (ref["alpha_loss"] is None)
        if ref["alpha_loss"] is not None:
            np.testing.assert_allclose(stats.alpha_loss, ref["alpha_loss"], rtol=2e-5, atol=2e-6)
        assert algo.critic_gradient_step == st.critic_gradient_step == u + 1
    for mod, want, order in ((actor, st.actor, A_ORDER), (critic, st.critic, C_ORDER),
                             (algo.critic_old.module, st.critic_old, C_ORDER)):
        for (name, t), k in zip(mod.state_dict().items(), order):
            np.testing.assert_allclose(t.cpu().numpy(), want[k].numpy(), rtol=1e-4, atol=0.02 * 1e-3, err_msg=name)
    assert abs(float(alpha._log_alpha.detach()) - float(st.log_alpha)) < 0.02 * 3e-4
    st_c = algo.critic_optim._optim.state[critic.last.model[0].weight]
    st_a = algo.policy_optim._optim.state[actor.mu.model[0].weight]
    assert float(st_c["step"]) == 4.0 and float(st_a["step"]) == 2.0 and st_c["exp_avg"].shape == (E, H, 1)


# ------------------------------------------------------------------------------------ HipDQN
def _dqn_hook_run(huber):
    from oracle import oracle_dqn as OD
    from tianshou_amd import dqn as D
    from tianshou_amd.integration import make_hip_dqn

    c, h, w, A, E, size, B = 4, 44, 36, 3, 4, 40, 32
    HipDQN = make_hip_dqn(ref=SI)
    torch.manual_seed(5)
    model = SI.DQNet(c, h, w, A)
    with torch.no_grad():
        model.net[0][0].weight.mul_(1.0 / 255.0)     # uint8 frames (0..255) times default-init weights: keep Q values O(1)
    algo = HipDQN(policy=SI.DiscreteQLearningPolicy(model), lr=1e-4, gamma=0.97, n_step_return_horizon=3, target_update_freq=2,
                  is_double=True, huber_loss_delta=huber, device="cuda", host_batch=True, write_back="eager").to("cuda")
    # (the reference-exact mode: `Algorithm._update` with its host batch, write-back after every update; the defaults --
    # index-only sampling, lazy write-back -- are compared with it in test_hip_dqn_default_mode_equals_the_reference_exact_mode)
    sd = model.state_dict()
    p0 = {k: sd[n].detach().cpu().clone() for k, n in zip(OD.PARAM_ORDER, D.TIANSHOU_KEYS)}
    ocfg = OD.DQNConfig(gamma=0.97, n_step=3, target_update_freq=2, is_double=True, huber_delta=huber, lr=1e-4)
    st = OD.DQNState.create(p0, ocfg)
    buf = SI.PrioritizedVectorReplayBuffer(E * size, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                           seed=2, stack_num=c, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(3)

    def fill(n):
        for _ in range(n):
            term = rng.random(E) < 0.08
            buf.add(SI.Batch(obs=rng.integers(0, 256, (E, h, w)).astype(np.uint8), act=rng.integers(0, A, E),
                             rew=rng.normal(size=E), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=rng.integers(0, 256, (E, h, w)).astype(np.uint8)))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample

    def sample(bs):
        batch, idx = orig_sample(bs)
        seen.append((idx.copy(), np.asarray(batch.weight).copy()))
        return batch, idx

    buf.sample = sample
    eps = np.finfo(np.float32).eps.item()
    for u in range(5):
        fill(25 if u == 0 else 9)                   # 25 + 4 * 9 = 61 adds per sub-buffer of 40 slots: wrapped by update 2
        stat = algo.update(buf, B)
        idx, w_is = seen[-1]
        m = algo._hip_mirror
        assert np.array_equal(m.obs.cpu().numpy(), buf.obs) and np.array_equal(m.rew.cpu().numpy(), buf.rew)
        assert np.array_equal(m.h_insertion, [b._insertion_idx for b in buf.buffers])          # incl. wrap-around
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)
        ret = OD.preprocess(st, ocfg, bstate, buf.obs, idx, c, obs_next_frames=buf.obs_next)
        obs = OD.stacked_frames(bstate, buf.obs, idx, c)
        loss_o, td_o = OD.update_with_batch(st, ocfg, obs, buf.act[idx], ret, None if huber is not None else w_is)
        np.testing.assert_allclose(stat.loss, loss_o, rtol=2e-5)
        upd_idx, upd_w = buf.weight_updates[-1]                                       # _postprocess_batch -> update_weight
        assert np.array_equal(upd_idx, idx)
        np.testing.assert_allclose(upd_w, np.abs(td_o.numpy()) + eps, rtol=1e-5, atol=2e-5)
        assert algo._iter == st.iter == u + 1
    tensors = [p.detach().cpu() for p in model.parameters()]
    for t, k in zip(tensors, OD.PARAM_ORDER):      # five Adam steps of lr 1e-4: compare on the scale of a fraction of a step
        np.testing.assert_allclose(t.numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    old = [p.detach().cpu() for p in algo.model_old.parameters()]
    for t, k in zip(old, OD.PARAM_ORDER):          # the lagged network was synced at updates 0, 2, 4 (dqn.py:283-285)
        np.testing.assert_allclose(t.numpy(), st.params_old[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    opt_state = algo.optim._optim.state[next(iter(model.parameters()))]
    assert float(opt_state["step"]) == 5.0


@pytest.mark.parametrize("layout", ["stored_obs_next", "atari_frames"])
def test_hip_dqn_default_mode_equals_the_reference_exact_mode(layout):
    """HipDQN's defaults -- `update()` samples indices only (`buffer.sample()`'s host copy of two stacked observations per
    transition is never made; frames, actions, rewards are read from the device mirror), write-back of the two networks and the
    optimizer deferred until the torch state is read -- against the reference-exact mode (`host_batch=True,
    write_back="eager"`: the reference's own `Algorithm._update`) on the same prioritized buffer history: identical loss and
    identical priorities written back every update, identical torch state after a sync (`policy.state_dict()`, `hip_sync()`),
    and the torch modules do not move in between.  The collector-side forward reads the engine's parameters either way.
    `atari_frames`: the buffer does not store obs_next (ReplayBuffer(ignore_obs_next=True, save_only_last_obs=True),
    examples/atari/atari_dqn.py) -- there the two hooks of the default mode are ONE library call (ts_dqn_learn_rows: gathers, n-step
    returns and update for the indices and importance weights the host buffer drew) and must equal the reference-exact mode's
    separate calls bit for bit."""
    c, h, w, B = LT.DQN_C, LT.DQN_H, LT.DQN_W, LT.DQN_BATCH
    build, fill = LT.dqn_build, LT.dqn_fill

    ref, lazy = build(host_batch=True, write_back="eager"), build()
    assert lazy.__dict__["_hip_lazy"] and not ref.__dict__["_hip_lazy"]
    bufs = [LT.dqn_buffer(layout) for _ in range(2)]                 # (atari_frames: ignore_obs_next=True)
    rngs = [np.random.default_rng(3) for _ in range(2)]
    made = []
    orig = bufs[1].sample
    bufs[1].sample = lambda bs: (made.append(bs), orig(bs))[1]          # the default mode must not ask for the host batch
    flat = lambda algo: torch.cat([p.detach().reshape(-1).float().cpu() for p in algo.parameters()])  # noqa: E731
    start = flat(lazy)
    for u in range(5):
        out = []
        for algo, buf, r in zip((ref, lazy), bufs, rngs):
            fill(buf, r, 25 if u == 0 else 9)
            out.append(algo.update(buf, B))
        assert out[0].loss == out[1].loss, u
        (i0, w0), (i1, w1) = bufs[0].weight_updates[-1], bufs[1].weight_updates[-1]
        assert np.array_equal(i0, i1) and np.array_equal(w0, w1)         # same draws, same TD errors -> same priorities
        assert torch.equal(flat(lazy), start)                            # nothing was written back yet
        assert lazy._iter == ref._iter == u + 1
    assert not made and lazy.__dict__["_hip_stale"]
    assert (lazy.__dict__["_hip_engine_obj"]._rows is not None) == (layout == "atari_frames")      # the one-call path ran / did not
    assert ref.__dict__["_hip_engine_obj"]._rows is None
    obs = np.random.default_rng(8).integers(0, 256, (8, c, h, w)).astype(np.uint8)
    q_l = lazy.policy(SI.Batch(obs=obs, info={})).logits
    q_r = ref.policy(SI.Batch(obs=obs, info={})).logits
    assert torch.equal(torch.as_tensor(q_l).cpu(), torch.as_tensor(q_r).cpu())        # the collector sees the engine's parameters
    sd = lazy.policy.state_dict()                                        # a reader: syncs
    assert not lazy.__dict__["_hip_stale"] and torch.equal(flat(lazy), flat(ref)) and not torch.equal(flat(lazy), start)
    assert all(torch.equal(v.cpu(), ref.policy.state_dict()[k].cpu()) for k, v in sd.items())
    p_l, p_r = next(iter(lazy.policy.model.parameters())), next(iter(ref.policy.model.parameters()))
    st_l, st_r = lazy.optim._optim.state[p_l], ref.optim._optim.state[p_r]
    assert float(st_l["step"]) == 5.0 and torch.equal(st_l["exp_avg"], st_r["exp_avg"]) and torch.equal(st_l["exp_avg_sq"], st_r["exp_avg_sq"])
    for algo, buf, r in zip((ref, lazy), bufs, rngs):
        fill(buf, r, 5)
        algo.update(buf, B)
    assert lazy.__dict__["_hip_stale"]
    lazy.hip_sync()
    assert not lazy.__dict__["_hip_stale"] and torch.equal(flat(lazy), flat(ref))
    sd_l, sd_r = lazy.state_dict(), ref.state_dict()
    for k in sd_r:
        if isinstance(sd_r[k], torch.Tensor):
            assert torch.equal(sd_l[k].cpu(), sd_r[k].cpu()), k


@pytest.mark.parametrize("huber", [None, 1.0], ids=["weighted_mse", "huber"])
def test_hip_dqn_hooks_against_oracle(huber):
    """HipDQN (integration.make_hip_dqn over the stand-ins) on the real engine, the Atari layout of
    examples/atari/atari_dqn.py:137-142: single uint8 frames per slot with stack_num = 4, a prioritized buffer, n-step 3,
    double-Q with a lagged network synced every 2 updates.  Per update: `_preprocess_batch` (n-step target through the
    device mirror, dqn.py:257-275) -> `_update_with_batch` (importance-weighted MSE or Huber, dqn.py:381-404) ->
    `_postprocess_batch` (TD errors reach `buffer.update_weight`, prio.py:81-94), against oracle_dqn fed with the same
    sampled indices.  The host buffer keeps growing between updates until every sub-buffer has wrapped: the mirror's
    incremental sync (write log) follows."""
    _dqn_hook_run(huber)


def test_hip_drqn_hooks_against_oracle():
    """HipDRQN (integration.make_hip_drqn over the stand-ins) on the real engine: a two-layer Recurrent Q network over a
    vector-observation buffer with stack_num = 4 (the LSTM's sequence), n-step 2, double-Q with a lagged network synced every 2
    updates, plain squared loss; four updates on a growing buffer against oracle_drqn fed with the same sampled indices."""
    from oracle import oracle_dqn as OD
    from oracle import oracle_drqn as ODR
    from tianshou_amd import drqn as R
    from tianshou_amd.integration import make_hip_drqn

    obs_dim, hidden, layers, A, stack, E, B, gamma, n_step = 6, 64, 2, 3, 4, 4, 32, 0.95, 2
    HipDRQN = make_hip_drqn(ref=SI)
    torch.manual_seed(51)
    model = SI.Recurrent(layers, obs_dim, A, hidden)
    algo = HipDRQN(policy=SI.DiscreteQLearningPolicy(model), lr=1e-3, gamma=gamma, n_step_return_horizon=n_step,
                   target_update_freq=2, is_double=True, huber_loss_delta=None, device="cuda").to("cuda")
    keys = R.state_dict_keys(layers)
    assert list(model.state_dict().keys()) == keys == ODR.param_keys(layers)
    p0 = {k: model.state_dict()[k].detach().cpu().clone() for k in keys}
    ocfg = OD.DQNConfig(gamma=gamma, n_step=n_step, target_update_freq=2, is_double=True, huber_delta=None, lr=1e-3)
    st = OD.DQNState.create(p0, ocfg)
    buf = SI.VectorReplayBuffer(E * 60, E, obs_shape=(obs_dim,), act_shape=(), act_dtype=np.int64, seed=52, stack_num=stack)
    rng = np.random.default_rng(53)

    def fill(T):
        obs = rng.normal(size=(T + 1, E, obs_dim)).astype(np.float32)
        for t in range(T):
            term = rng.random(E) < 0.06
            buf.add(SI.Batch(obs=obs[t], act=rng.integers(0, A, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                             truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        fill(25 if u == 0 else 9)
        stat = algo.update(buf, B)
        idx = seen[-1]
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)

        def tq_fn(after):                                        # the buffer stores obs_next: Q(s') from its rows at `after`
            return ODR.target_q(st, ocfg, OD.stacked_frames(bstate, buf.obs_next, after, stack)).numpy().reshape(-1, 1)

        ret, _ = O.compute_nstep_return(bstate, idx, tq_fn, gamma, n_step)
        obs = OD.stacked_frames(bstate, buf.obs, idx, stack)
        loss_o, _ = ODR.update_with_batch(st, ocfg, obs, buf.act[idx], ret.astype(np.float32).reshape(-1))
        np.testing.assert_allclose(stat.loss, loss_o, rtol=2e-5, atol=1e-6)
        assert algo._iter == st.iter == u + 1
    for k in keys:
        np.testing.assert_allclose(model.state_dict()[k].cpu().numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 1e-3, err_msg=k)
        np.testing.assert_allclose(algo.model_old.module.state_dict()[k].cpu().numpy(), st.params_old[k].numpy(), rtol=1e-5,
                                   atol=0.05 * 1e-3, err_msg="old " + k)
    assert float(algo.optim._optim.state[model.fc1.weight]["step"]) == 4.0


# ------------------------------------------------------------------------------------ HipPPOCnn
def test_hip_ppo_cnn_hooks_against_oracle():
    """HipPPOCnn (integration.make_hip_ppo_cnn over the stand-ins) on the real engine, the layout of
    examples/atari/atari_ppo.py:106-135: one DQNet(features_only, 512) trunk shared by a logits actor and a critic, single
    uint8 frames per slot with stack_num = 4, obs_next stored; PPO with value clipping, advantage normalisation, entropy
    bonus, gradient clipping and return scaling.  Two update() calls on a buffer that is reset and refilled (on-policy):
    `_preprocess_batch` (V(s), V(s'), GAE, log pi_old through the device mirror) -> `_update_with_batch` (minibatches from
    np.random.permutation, replayed for the oracle) -> write-back of the twelve tensors + Adam state, against
    oracle_ppo_cnn on the host copies of the same frames."""
    from oracle import oracle_dqn as OD
    from oracle import oracle_ppo_cnn as OC
    from tianshou_amd.integration import make_hip_ppo_cnn

    c, h, w, A, E, T, batch_size, repeat = 4, 44, 36, 5, 4, 24, 32, 2
    HipPPOCnn = make_hip_ppo_cnn("ppo", ref=SI)
    torch.manual_seed(11)
    trunk = SI.DQNetFeatures(c, h, w)
    actor, critic = SI.DiscreteActor(trunk, A, softmax_output=False), SI.DiscreteCritic(trunk)
    # (frames take values 0..3: with default-init weights the features stay O(1) and the weights large against one Adam
    # step -- scaling conv1 by 1/255 instead would make every step rewrite it and amplify rounding noise chaotically)
    kw = dict(eps_clip=0.1, value_clip=True, vf_coef=0.25, ent_coef=0.01, max_grad_norm=0.5, return_scaling=True,
              advantage_normalization=True, gae_lambda=0.95, gamma=0.99, lr=2.5e-4)
    algo = HipPPOCnn(policy=SI.Policy(actor), critic=critic, device="cuda", **kw).to("cuda")
    hip_params = [p.detach().cpu().clone() for p in algo._hip_params()]
    st = OP.PPOState(params={k: t for k, t in zip(OC.PARAM_ORDER, hip_params)})
    ocfg = OP.PPOConfig(max_batchsize=4096, **kw)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64, stack_num=c)
    rng = np.random.default_rng(12)
    algo.policy.is_within_training_step = True
    for u in range(2):
        buf.reset()
        for _ in range(T):
            term = rng.random(E) < 0.05
            buf.add(SI.Batch(obs=rng.integers(0, 4, (E, h, w)).astype(np.uint8), act=rng.integers(0, A, E),
                             rew=rng.normal(size=E).astype(np.float32), terminated=term,
                             truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=rng.integers(0, 4, (E, h, w)).astype(np.uint8)))
        n = len(buf)
        idx = buf.sample_indices(0)
        bs = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths,
                           np.asarray([b._insertion_idx for b in buf.buffers]), buf.rew, buf.terminated, buf.truncated)
        obs = torch.from_numpy(OD.stacked_frames(bs, buf.obs, idx, c).astype(np.float32))
        obs_next = torch.from_numpy(OD.stacked_frames(bs, buf.obs_next, idx, c).astype(np.float32))
        np.random.seed(50 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        pre = OC.preprocess(st, ocfg, obs, obs_next, buf.act[idx], buf.rew[idx], buf.terminated[idx], buf.truncated[idx], idx,
                            bs.unfinished_index())
        losses_o = OC.update(st, ocfg, obs, buf.act[idx], pre, batch_size, repeat, perms)
        np.random.seed(50 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert stats.gradient_steps == losses_o.shape[0]
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(losses_o[:, col])
            # (minibatches of 32 samples behind four fp32 layers with K up to 3,136; the clip loss is a mean of O(1) normalised
            # advantages times (ratio - 1), i.e. a small difference of large terms: absolute tolerance)
            np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=2e-4, atol=3e-5 if col == 1 else 2e-6)
        np.testing.assert_allclose([algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count],
                                   [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)
    for t, k in zip(algo._hip_params(), OC.PARAM_ORDER):      # a few Adam steps of lr 2.5e-4: compare on a fraction of a step
        np.testing.assert_allclose(t.detach().cpu().numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 2.5e-4, err_msg=k)
    assert trunk.net[1].weight is actor.preprocess.net[1].weight is critic.preprocess.net[1].weight      # still one trunk
    sd = algo.state_dict()                                     # Adam moments arrive lazily, one entry per tensor (12)
    assert len(sd["_optimizers"][0]["state"]) == 12
    state = algo.optim._optim.state
    assert all(float(state[p]["step"]) == st.adam_step for p in algo._hip_params())


def test_hip_ppo_discrete_hooks_against_oracle():
    """HipPPODiscrete (integration.make_hip_ppo_discrete over the stand-ins) on the real engine, BASELINE.json configs[0]'s
    layout (test/discrete/test_ppo_discrete.py:88-127): Net(4, [64, 64]) shared by DiscreteActor (softmax_output=True, so
    dist_fn = Categorical receives probabilities) and DiscreteCritic, minibatch 64, PPO with advantage normalisation, dual
    clip, value clip and return scaling; three update() calls on a reset-and-refilled buffer against oracle_ppo_discrete."""
    from torch.distributions import Categorical

    from oracle import oracle_ppo_cnn as OC
    from oracle import oracle_ppo_discrete as OPD
    from tianshou_amd.integration import make_hip_ppo_discrete

    obs_dim, hidden, A, E, T, batch_size, repeat = 4, 64, 2, 8, 40, 64, 2
    HipPPODiscrete = make_hip_ppo_discrete("ppo", ref=SI)
    torch.manual_seed(31)
    trunk = SI.Net(obs_dim, [hidden, hidden], nn.ReLU)
    actor, critic = SI.DiscreteActor(trunk, A, softmax_output=True), SI.DiscreteCritic(trunk)
    kw = dict(eps_clip=0.2, dual_clip=3.0, value_clip=True, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, return_scaling=True,
              advantage_normalization=True, gae_lambda=0.95, gamma=0.99, lr=3e-4)
    algo = HipPPODiscrete(policy=SI.Policy(actor, dist_fn=Categorical), critic=critic, device="cuda", **kw).to("cuda")
    hip_params = [p.detach().cpu().clone() for p in algo._hip_params()]
    st = OP.PPOState(params={k: t for k, t in zip(OPD.PARAM_ORDER, hip_params)})
    ocfg = OP.PPOConfig(max_batchsize=4096, **kw)
    net = OPD.MlpNet(softmax_output=True)
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(), act_dtype=np.int64)
    rng = np.random.default_rng(32)
    algo.policy.is_within_training_step = True
    for u in range(3):
        buf.reset()
        obs_seq = rng.normal(size=(T + 1, E, obs_dim)).astype(np.float32)
        for t in range(T - 4 * u):
            term = rng.random(E) < 0.05
            buf.add(SI.Batch(obs=obs_seq[t], act=rng.integers(0, A, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                             truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs_seq[t + 1]))
        n = len(buf)
        idx = buf.sample_indices(0)
        bs = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths,
                           np.asarray([b._insertion_idx for b in buf.buffers]), buf.rew, buf.terminated, buf.truncated)
        obs, obs_next = torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.obs_next[idx])
        np.random.seed(70 + u)
        perms = [np.random.permutation(n) for _ in range(repeat)]
        pre = OC.preprocess(st, ocfg, obs, obs_next, buf.act[idx], buf.rew[idx], buf.terminated[idx], buf.truncated[idx], idx,
                            bs.unfinished_index(), net=net)
        losses_o = OC.update(st, ocfg, obs, buf.act[idx], pre, batch_size, repeat, perms, net=net)
        np.random.seed(70 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert stats.gradient_steps == losses_o.shape[0]
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(losses_o[:, col])
            np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=5e-5, atol=5e-6)
        np.testing.assert_allclose([algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count],
                                   [st.ret_rms.mean, st.ret_rms.var, st.ret_rms.count], rtol=1e-5)
    for t, k in zip(algo._hip_params(), OPD.PARAM_ORDER):
        np.testing.assert_allclose(t.detach().cpu().numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 3e-4, err_msg=k)
    assert actor.preprocess.model.model[0].weight is critic.preprocess.model.model[0].weight             # still one trunk
    state = algo.optim._optim.state
    assert all(float(state[p]["step"]) == st.adam_step for p in algo._hip_params())


# ------------------------------------------------------------------------------------ HipQRDQN
def test_hip_qrdqn_hooks_against_oracle():
    """HipQRDQN (integration.make_hip_qrdqn over the stand-ins) on the real engine: single uint8 frames with stack_num = 4,
    a prioritized buffer, n-step 2, a lagged network synced every 2 updates, 16 quantiles.  Per update: `_preprocess_batch`
    (the lagged net's quantiles of the online net's greedy action as the n-step target, qrdqn.py:93-104 through
    dqn.py:257-275) -> `_update_with_batch` (importance-weighted quantile Huber loss, qrdqn.py:106-131) ->
    `_postprocess_batch` (the new priorities reach `buffer.update_weight`), against oracle_distq fed with the same sampled
    indices; the host buffer grows and wraps between updates."""
    from oracle import oracle_distq as OQ
    from oracle import oracle_dqn as OD
    from tianshou_amd import dqn as D
    from tianshou_amd.integration import make_hip_qrdqn

    c, h, w, A, N, E, size, B = 4, 44, 36, 3, 16, 4, 40, 32
    HipQRDQN = make_hip_qrdqn(ref=SI)
    torch.manual_seed(9)
    model = SI.QRDQNet(c, h, w, A, N)
    with torch.no_grad():
        model.net[0][0].weight.mul_(1.0 / 255.0)     # uint8 frames (0..255) times default-init weights: keep quantiles O(1)
    algo = HipQRDQN(policy=SI.DiscreteQLearningPolicy(model), lr=1e-4, gamma=0.97, num_quantiles=N, n_step_return_horizon=2,
                    target_update_freq=2, device="cuda").to("cuda")
    sd = model.state_dict()
    p0 = {k: sd[n].detach().cpu().clone() for k, n in zip(OD.PARAM_ORDER, D.TIANSHOU_KEYS)}
    ocfg = OQ.DistQConfig(kind=OQ.QR, n_atoms=N, gamma=0.97, n_step=2, target_update_freq=2, lr=1e-4)
    st = OD.DQNState.create(p0, ocfg.dqn())
    buf = SI.PrioritizedVectorReplayBuffer(E * size, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                           seed=4, stack_num=c, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(8)

    def fill(n):
        for _ in range(n):
            term = rng.random(E) < 0.08
            buf.add(SI.Batch(obs=rng.integers(0, 256, (E, h, w)).astype(np.uint8), act=rng.integers(0, A, E),
                             rew=rng.normal(size=E), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=rng.integers(0, 256, (E, h, w)).astype(np.uint8)))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample

    def sample(bs):
        batch, idx = orig_sample(bs)
        seen.append((idx.copy(), np.asarray(batch.weight).copy()))
        return batch, idx

    buf.sample = sample
    eps = np.finfo(np.float32).eps.item()
    for u in range(4):
        fill(25 if u == 0 else 9)
        stat = algo.update(buf, B)
        idx, w_is = seen[-1]
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)
        ret = OQ.preprocess(st, ocfg, bstate, buf.obs, idx, A, c, obs_next_frames=buf.obs_next)
        obs = OD.stacked_frames(bstate, buf.obs, idx, c)
        loss_o, prio_o = OQ.update_with_batch(st, ocfg, obs, buf.act[idx], ret, A, weight=w_is)
        np.testing.assert_allclose(stat.loss, loss_o, rtol=2e-5)
        upd_idx, upd_w = buf.weight_updates[-1]
        assert np.array_equal(upd_idx, idx)
        np.testing.assert_allclose(upd_w, np.abs(np.asarray(prio_o)) + eps, rtol=2e-5, atol=2e-5)
        assert algo._iter == st.iter == u + 1
    for t, k in zip([p.detach().cpu() for p in model.parameters()], OD.PARAM_ORDER):
        np.testing.assert_allclose(t.numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    for t, k in zip([p.detach().cpu() for p in algo.model_old.parameters()], OD.PARAM_ORDER):
        np.testing.assert_allclose(t.numpy(), st.params_old[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    assert float(algo.optim._optim.state[next(iter(model.parameters()))]["step"]) == 4.0


def test_hip_c51_hooks_against_oracle():
    """HipC51 (integration.make_hip_c51 over the stand-ins) on the real engine: single uint8 frames with stack_num = 4, a
    prioritized buffer, n-step 2, a lagged network synced every 2 updates, 21 atoms on [-4, 4].  Per update:
    `_preprocess_batch` (the support as `target_q`, so `returns` are the n-step shifted atoms, c51.py:120-121 through
    dqn.py:257-275) -> `_update_with_batch` (projection of the lagged net's distribution at `batch.obs_next`, importance-weighted
    cross-entropy, c51.py:123-160) -> `_postprocess_batch` (the per-sample cross-entropies reach `buffer.update_weight`), against
    oracle_distq fed with the same sampled indices; the host buffer grows and wraps between updates."""
    from oracle import oracle_distq as OQ
    from oracle import oracle_dqn as OD
    from tianshou_amd import dqn as D
    from tianshou_amd.integration import make_hip_c51

    c, h, w, A, N, E, size, B = 4, 44, 36, 3, 21, 4, 40, 32
    HipC51 = make_hip_c51(ref=SI)
    torch.manual_seed(13)
    model = SI.C51Net(c, h, w, A, N)
    with torch.no_grad():
        model.net[0][0].weight.mul_(1.0 / 255.0)     # uint8 frames (0..255) times default-init weights: keep logits O(1)
    algo = HipC51(policy=SI.C51Policy(model, num_atoms=N, v_min=-4.0, v_max=4.0), lr=1e-4, gamma=0.97,
                  n_step_return_horizon=2, target_update_freq=2, device="cuda").to("cuda")
    sd = model.state_dict()
    p0 = {k: sd[n].detach().cpu().clone() for k, n in zip(OD.PARAM_ORDER, D.TIANSHOU_KEYS)}
    ocfg = OQ.DistQConfig(kind=OQ.C51, n_atoms=N, gamma=0.97, n_step=2, target_update_freq=2, lr=1e-4, v_min=-4.0, v_max=4.0)
    st = OD.DQNState.create(p0, ocfg.dqn())
    buf = SI.PrioritizedVectorReplayBuffer(E * size, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                           seed=5, stack_num=c, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(18)

    def fill(n):
        for _ in range(n):
            term = rng.random(E) < 0.08
            buf.add(SI.Batch(obs=rng.integers(0, 256, (E, h, w)).astype(np.uint8), act=rng.integers(0, A, E),
                             rew=rng.normal(size=E), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=rng.integers(0, 256, (E, h, w)).astype(np.uint8)))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample

    def sample(bs):
        batch, idx = orig_sample(bs)
        seen.append((idx.copy(), np.asarray(batch.weight).copy()))
        return batch, idx

    buf.sample = sample
    eps = np.finfo(np.float32).eps.item()
    for u in range(4):
        fill(25 if u == 0 else 9)
        stat = algo.update(buf, B)
        idx, w_is = seen[-1]
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)
        ret = OQ.preprocess(st, ocfg, bstate, buf.obs, idx, A, c, obs_next_frames=buf.obs_next)
        obs = OD.stacked_frames(bstate, buf.obs, idx, c)
        obs_next = OD.stacked_frames(bstate, buf.obs_next, idx, c)                # batch.obs_next (buffer_base.py:624-626)
        loss_o, prio_o = OQ.update_with_batch(st, ocfg, obs, buf.act[idx], ret, A, weight=w_is, obs_next=obs_next)
        np.testing.assert_allclose(stat.loss, loss_o, rtol=2e-5)
        upd_idx, upd_w = buf.weight_updates[-1]
        assert np.array_equal(upd_idx, idx)
        np.testing.assert_allclose(upd_w, np.abs(np.asarray(prio_o)) + eps, rtol=2e-5, atol=2e-5)
        assert algo._iter == st.iter == u + 1
    for t, k in zip([p.detach().cpu() for p in model.parameters()], OD.PARAM_ORDER):
        np.testing.assert_allclose(t.numpy(), st.params[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    for t, k in zip([p.detach().cpu() for p in algo.model_old.parameters()], OD.PARAM_ORDER):
        np.testing.assert_allclose(t.numpy(), st.params_old[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
    assert float(algo.optim._optim.state[next(iter(model.parameters()))]["step"]) == 4.0


def test_hip_rainbow_hooks_against_oracle():
    """HipRainbow (integration.make_hip_rainbow over the stand-ins) on the real engine: RainbowNet (dueling, NoisyLinear) over
    single uint8 frames with stack_num = 4 on a prioritized buffer, n-step 2, a lagged network synced every 2 updates.  The
    NoisyLinear noise is drawn by the torch modules (`_sample_noise`, rainbow.py:93-100) and handed to the engine; the test
    replays the same draws from torch's generator for oracle_rainbow."""
    import copy

    from oracle import oracle_distq as OQ
    from oracle import oracle_dqn as OD
    from oracle import oracle_rainbow as ORB
    from tianshou_amd import rainbow as RB
    from tianshou_amd.integration import make_hip_rainbow

    c, h, w, A, N, E, size, B = 4, 44, 36, 3, 11, 4, 40, 32
    HipRainbow = make_hip_rainbow(ref=SI)
    torch.manual_seed(71)
    model = SI.RainbowNet(c, h, w, A, N)
    with torch.no_grad():
        model.net[0].weight.mul_(1.0 / 255.0)          # uint8 frames (0..255) times default-init weights: keep logits O(1)
    # (the torch modules stay on the host: NoisyLinear draws its noise on the module's device, and the host generator is the
    # one the test can replay; the engine lives on the GPU either way)
    algo = HipRainbow(policy=SI.C51Policy(model, num_atoms=N, v_min=-4.0, v_max=4.0), lr=1e-4, gamma=0.97,
                      n_step_return_horizon=2, target_update_freq=2, device="cuda")
    noise_of = lambda mod: {f"{L}.{t}": mod.state_dict()[f"{m}.{t}"].detach().cpu().clone()   # noqa: E731
                            for L, m in zip(ORB.NOISY, RB.NOISY) for t in ("eps_p", "eps_q")}
    sd = model.state_dict()
    p0 = {k: sd[n].detach().cpu().clone() for k, n in zip(ORB.PARAM_ORDER, RB.TIANSHOU_KEYS)}
    ocfg = OQ.DistQConfig(kind=OQ.C51, n_atoms=N, gamma=0.97, n_step=2, target_update_freq=2, lr=1e-4, v_min=-4.0, v_max=4.0)
    st = ORB.RainbowState(p0, noise_of(model), ocfg)
    scratch, scratch_old = copy.deepcopy(model), copy.deepcopy(model)
    buf = SI.PrioritizedVectorReplayBuffer(E * size, E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                           seed=72, stack_num=c, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(73)

    def fill(n):
        for _ in range(n):
            term = rng.random(E) < 0.08
            buf.add(SI.Batch(obs=rng.integers(0, 256, (E, h, w)).astype(np.uint8), act=rng.integers(0, A, E),
                             rew=rng.normal(size=E), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=rng.integers(0, 256, (E, h, w)).astype(np.uint8)))

    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample

    def sample(bs):
        batch, idx = orig_sample(bs)
        seen.append((idx.copy(), np.asarray(batch.weight).copy()))
        return batch, idx

    buf.sample = sample
    eps = np.finfo(np.float32).eps.item()
    for u in range(4):
        fill(25 if u == 0 else 9)
        rng_state = torch.get_rng_state()
        stat = algo.update(buf, B)
        idx, w_is = seen[-1]
        torch.set_rng_state(rng_state)                       # the two _sample_noise calls of this update, replayed on the host
        SI.RainbowDQN._sample_noise(scratch)
        SI.RainbowDQN._sample_noise(scratch_old)
        noise, noise_old = noise_of(scratch), noise_of(scratch_old)
        for k, v in noise_of(model).items():                 # the hook left this update's draws in the torch module
            assert torch.equal(v, noise[k]), k
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)
        ret = ORB.preprocess(ocfg, bstate, idx)
        obs = OD.stacked_frames(bstate, buf.obs, idx, c)
        obs_next = OD.stacked_frames(bstate, buf.obs_next, idx, c)
        loss_o, prio_o = ORB.update_with_batch(st, ocfg, obs, buf.act[idx], ret, obs_next, A, noise, noise_old, weight=w_is)
        np.testing.assert_allclose(stat.loss, loss_o, rtol=2e-5)
        upd_idx, upd_w = buf.weight_updates[-1]
        assert np.array_equal(upd_idx, idx)
        np.testing.assert_allclose(upd_w, np.abs(np.asarray(prio_o)) + eps, rtol=2e-5, atol=2e-5)
        assert algo._iter == st.dqn.iter == u + 1
        for k, v in noise_of(algo.model_old).items():        # the lagged module's noise: its own draws, or the sync's copy
            assert torch.equal(v, st.noise_old[k]), k
    sd, so = model.state_dict(), algo.model_old.state_dict()
    for k, n in zip(ORB.PARAM_ORDER, RB.TIANSHOU_KEYS):
        np.testing.assert_allclose(sd[n].cpu().numpy(), st.dqn.params[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg=k)
        np.testing.assert_allclose(so[n].cpu().numpy(), st.dqn.params_old[k].numpy(), rtol=1e-5, atol=0.05 * 1e-4, err_msg="old " + k)
    assert float(algo.optim._optim.state[model.Q[0].mu_W]["step"]) == 4.0


# ------------------------------------------------------------------------------------ HipTD3
def test_hip_td3_hooks_against_oracle():
    """HipTD3 (integration.make_hip_td3 over the stand-ins) on the real engine with Net[128, 128] trunks (a width other than
    the example's 256): growing host buffer -> incremental mirror, smoothed lagged-actor target (td3.py:190-202, the
    reference's torch.randn draw replayed), twin critic steps, delayed actor step (every 2nd update), Polyak of three
    networks, write-back of six networks + three optimizers -- against oracle_sac's TD3 restatement fed with the same
    sampled indices."""
    from oracle import oracle_sac as OS
    from tianshou_amd.integration import make_hip_td3

    obs_dim, act_dim, E, B, H = 17, 6, 4, 64, 128
    HipTD3 = make_hip_td3(ref=SI)
    torch.manual_seed(21)
    actor = SI.ContinuousActorDeterministic(SI.Net(obs_dim, [H, H], nn.ReLU), act_dim, max_action=1.0)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [H, H], nn.ReLU))
    c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [H, H], nn.ReLU))
    algo = HipTD3(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=3e-4, critic_lr=1e-3, tau=0.01, gamma=0.98,
                  policy_noise=0.2, update_actor_freq=2, noise_clip=0.5, device="cuda").to("cuda")
    grab = lambda mod, keys: {k: mod.state_dict()[n].detach().cpu().clone() for k, n in zip(keys, mod.state_dict())}   # noqa: E731
    cfg = OS.TD3Config(gamma=0.98, tau=0.01, n_step=1, twin=True, policy_noise=0.2, noise_clip=0.5, update_actor_freq=2,
                       max_action=1.0, actor_lr=3e-4, critic_lr=1e-3)
    st = OS.TD3State.create(grab(actor, OS.DET_ACTOR_ORDER), grab(c1, OS.CRITIC_ORDER), grab(c2, OS.CRITIC_ORDER), cfg)
    buf = SI.VectorReplayBuffer(E * 200, E, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=6)
    rng = np.random.default_rng(2)
    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, rng)
        torch.manual_seed(300 + u)
        stats = algo.update(buf, B)
        idx = seen[-1]
        torch.manual_seed(300 + u)
        noise = torch.randn(B, act_dim)                                           # td3.py:196
        obs, act = torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx])
        tq = OS.td3_target_q(st, cfg, torch.from_numpy(buf.obs_next[idx]), noise).flatten().numpy()
        ret = (buf.rew[idx] + 0.98 * tq.astype(np.float64) * (~buf.terminated[idx])).astype(np.float32)
        ref = OS.td3_update_with_batch(st, cfg, obs, act, ret)
        np.testing.assert_allclose([stats.actor_loss, stats.critic1_loss, stats.critic2_loss],
                                   [ref["actor_loss"], ref["critic1_loss"], ref["critic2_loss"]], rtol=2e-5, atol=2e-6)
        assert algo._cnt == st.cnt == u + 1
    for mod, ref_p, order in ((actor, st.actor, OS.DET_ACTOR_ORDER), (c1, st.critic1, OS.CRITIC_ORDER),
                              (c2, st.critic2, OS.CRITIC_ORDER), (algo.actor_old.module, st.actor_old, OS.DET_ACTOR_ORDER),
                              (algo.critic_old.module, st.critic1_old, OS.CRITIC_ORDER)):
        for (name, t), k in zip(mod.state_dict().items(), order):                  # a few Adam steps: compare on lr's scale
            np.testing.assert_allclose(t.detach().cpu().numpy(), ref_p[k].numpy(), rtol=1e-5, atol=0.05 * 1e-3, err_msg=name)
    st_a = algo.policy_optim._optim.state[next(iter(actor.parameters()))]
    st_c = algo.critic_optim._optim.state[next(iter(c1.parameters()))]
    assert float(st_a["step"]) == 2.0 and float(st_c["step"]) == 4.0               # the actor stepped at updates 0 and 2


def test_hip_ddpg_hooks_against_oracle():
    """HipDDPG (integration.make_hip_ddpg over the stand-ins) on the real engine with Net[64, 64] trunks, n-step 3: the target
    is the single lagged critic at the lagged actor's action (ddpg.py:397-399), one critic step and one actor step per update
    (:401-411), Polyak of both networks, write-back of four networks + two optimizers -- against oracle_sac's DDPG
    restatement (TD3Config(twin=False)) fed with the same sampled indices."""
    from oracle import oracle_sac as OS
    from tianshou_amd.integration import make_hip_ddpg

    obs_dim, act_dim, E, B, H, n_step, gamma = 11, 3, 4, 64, 64, 3, 0.95
    HipDDPG = make_hip_ddpg(ref=SI)
    torch.manual_seed(23)
    actor = SI.ContinuousActorDeterministic(SI.Net(obs_dim, [H, H], nn.ReLU), act_dim, max_action=1.5)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [H, H], nn.ReLU))
    algo = HipDDPG(policy=SI.Policy(actor), critic=c1, lr=3e-4, critic_lr=1e-3, tau=0.02, gamma=gamma,
                   n_step_return_horizon=n_step, device="cuda").to("cuda")
    grab = lambda mod, keys: {k: mod.state_dict()[n].detach().cpu().clone() for k, n in zip(keys, mod.state_dict())}   # noqa: E731
    cfg = OS.TD3Config(gamma=gamma, tau=0.02, n_step=n_step, twin=False, max_action=1.5, actor_lr=3e-4, critic_lr=1e-3)
    st = OS.TD3State.create(grab(actor, OS.DET_ACTOR_ORDER), grab(c1, OS.CRITIC_ORDER), None, cfg)
    buf = SI.VectorReplayBuffer(E * 200, E, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=16)
    rng = np.random.default_rng(22)
    algo.policy.is_within_training_step = True
    seen = []
    orig_sample = buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append(r[1]), r)[1])(orig_sample(bs))
    for u in range(4):
        _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, rng)
        stats = algo.update(buf, B)
        idx = seen[-1]
        bstate = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [b._insertion_idx for b in buf.buffers],
                               buf.rew, buf.terminated, buf.truncated)
        tq_fn = lambda after: OS.td3_target_q(st, cfg, torch.from_numpy(buf.obs_next[after])).numpy()   # noqa: E731
        ret, _ = O.compute_nstep_return(bstate, idx, tq_fn, gamma, n_step)
        ref = OS.td3_update_with_batch(st, cfg, torch.from_numpy(buf.obs[idx]), torch.from_numpy(buf.act[idx]),
                                       ret.astype(np.float32))
        np.testing.assert_allclose([stats.actor_loss, stats.critic_loss], [ref["actor_loss"], ref["critic1_loss"]],
                                   rtol=2e-5, atol=2e-6)
    for mod, ref_p, order in ((actor, st.actor, OS.DET_ACTOR_ORDER), (c1, st.critic1, OS.CRITIC_ORDER),
                              (algo.actor_old.module, st.actor_old, OS.DET_ACTOR_ORDER),
                              (algo.critic_old.module, st.critic1_old, OS.CRITIC_ORDER)):
        for (name, t), k in zip(mod.state_dict().items(), order):
            np.testing.assert_allclose(t.detach().cpu().numpy(), ref_p[k].numpy(), rtol=1e-5, atol=0.05 * 1e-3, err_msg=name)
    st_a = algo.policy_optim._optim.state[next(iter(actor.parameters()))]
    st_c = algo.critic_optim._optim.state[next(iter(c1.parameters()))]
    assert float(st_a["step"]) == 4.0 and float(st_c["step"]) == 4.0


@pytest.mark.parametrize("prio", [False, True])
def test_hip_sac_update_as_one_library_call_equals_the_two_hook_calls(monkeypatch, prio):
    """HipSAC.update() with its defaults (index-only sampling, the engine's rsample noise): `_preprocess_batch` defers the
    target pass and `_update_with_batch` makes ONE call (ts_sac_learn_rows) -- against the same algorithm with the two
    entry points kept apart (TS_SAC_TWO_CALLS=1): identical statistics every update, identical returns on the batch,
    identical priorities written to a prioritized buffer, identical torch state after hip_sync()."""
    from tianshou_amd.integration import make_hip_sac

    obs_dim, act_dim, E, B = 23, 5, 4, 96
    HipSAC = make_hip_sac(ref=SI)

    def build():
        torch.manual_seed(11)
        actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [256, 256], nn.ReLU), act_dim, unbounded=True, conditioned_sigma=True)
        c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
        c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, [256, 256], nn.ReLU))
        algo = HipSAC(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=1e-3, tau=0.01, gamma=0.97,
                      alpha=SI.AutoAlpha(-float(act_dim), -0.5, 3e-4), device="cuda", noise_seed=77).to("cuda")
        algo.policy.is_within_training_step = True
        return algo

    def make_buf():
        if prio:
            return SI.PrioritizedVectorReplayBuffer(E * 200, E, alpha=0.6, beta=0.4, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=4)
        return SI.VectorReplayBuffer(E * 200, E, obs_shape=(obs_dim,), act_shape=(act_dim,), seed=4)

    flat = lambda algo: torch.cat([p.detach().reshape(-1).float().cpu() for p in algo.parameters()])  # noqa: E731
    runs = {}
    for mode in ("one", "two"):
        if mode == "two":
            monkeypatch.setenv("TS_SAC_TWO_CALLS", "1")
        algo, buf, r = build(), make_buf(), np.random.default_rng(9)
        calls = []
        orig = algo._engine().learn_rows
        algo._hip_engine.learn_rows = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        out = []
        for u in range(4):
            _fill(buf, 30 if u == 0 else 7, obs_dim, act_dim, r)
            st = algo.update(buf, B)
            out.append([getattr(st, f) for f in ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")])
        assert len(calls) == (4 if mode == "one" else 0)
        algo.hip_sync()
        runs[mode] = (out, flat(algo), (np.array(buf.prio), len(buf.weight_updates)) if prio else None)
    assert runs["one"][0] == runs["two"][0]
    assert torch.equal(runs["one"][1], runs["two"][1])
    if prio:
        assert np.array_equal(runs["one"][2][0], runs["two"][2][0]) and runs["one"][2][1] == runs["two"][2][1] == 4


@pytest.mark.parametrize("tag", ["relu3", "linear4", "csigma", "ln_relu3"])
def test_hip_ppo_hooks_on_deep_trunks_replay_the_reference(tag):
    """Net trunks outside [h, h] tanh (three ReLU layers of unequal widths with a different critic trunk; four linear layers):
    HipPPO picks the per-layer engine (kind "net", ppo_wide.NetPPOEngine) and the whole hook path -- mirror, preprocess, the
    host-drawn Batch.split permutations, update, write-back, Adam flush -- reproduces what the REFERENCE's PPO.update()
    produced on the same buffer contents, weights and NumPy seed (tests/golden/ppo_net_*.npz, oracle/gen_golden.py::gen_ppo_net).
    ln_relu3: Net(norm_layer=nn.LayerNorm) (utils/net/common.py:25-39) -- Linear -> LayerNorm -> ReLU per hidden layer."""
    import os

    from tianshou_amd.integration import make_hip_ppo
    from tianshou_amd.ppo_wide import NetPPOEngine

    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", f"ppo_net_{tag}.npz")))
    cfg = dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]]))
    E, T, obs_dim, act_dim, batch_size, repeat = (int(x) for x in g["dims"])
    ha, hc = [int(x) for x in g["hidden_a"]], [int(x) for x in g["hidden_c"]]
    act_cls = {0: nn.Tanh, 1: nn.ReLU, 2: None}[int(g["activation"])]
    seed = {"relu3": 11, "linear4": 13, "csigma": 14, "ln_relu3": 31}[tag]
    cs = bool(int(g["conditioned_sigma"]))
    ln = "layer_norm" in g
    nkw = dict(norm_layer=nn.LayerNorm, norm_args=dict(eps=float(g["ln_eps"]))) if ln else {}
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, ha, act_cls, **nkw), act_dim, unbounded=True, conditioned_sigma=cs)
    critic = SI.ContinuousCritic(SI.Net(obs_dim, hc, act_cls, **nkw))

    def params(mod, head, extra=()):
        lin = [m for m in mod.preprocess.model.model if isinstance(m, (nn.Linear, nn.LayerNorm))] + [m for m in head.modules() if isinstance(m, nn.Linear)]
        out = []
        for m in lin:
            out += [m.weight, m.bias]
        return out + list(extra)

    pa = params(actor, actor.mu, list(actor.sigma.model[0].parameters()) if cs else [actor.sigma_param])
    pc = params(critic, critic.last)
    with torch.no_grad():
        for i, p in enumerate(pa):
            p.copy_(torch.from_numpy(g[f"a{i}_0"]))
        for i, p in enumerate(pc):
            p.copy_(torch.from_numpy(g[f"c{i}_0"]))
    kw = dict(eps_clip=cfg["eps_clip"], dual_clip=cfg["dual_clip"] or None, value_clip=bool(cfg["value_clip"]),
              advantage_normalization=bool(cfg["advantage_normalization"]), vf_coef=cfg["vf_coef"], ent_coef=cfg["ent_coef"],
              max_grad_norm=cfg["max_grad_norm"] or None, return_scaling=bool(cfg["return_scaling"]), gae_lambda=cfg["gae_lambda"],
              gamma=cfg["gamma"], lr=cfg["lr"])
    algo = make_hip_ppo("ppo", ref=SI)(policy=SI.Policy(actor), critic=critic, device="cuda", permutations="host", **kw).to("cuda")
    assert algo._hip_dims == (obs_dim, act_dim, (tuple(ha), tuple(hc), {nn.Tanh: "tanh", nn.ReLU: "relu", None: "none"}[act_cls]) +
                              (("conditioned_sigma",) if cs else ()) + ((("layer_norm", float(g["ln_eps"])),) if ln else ()), "net")
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    size = buf.maxsize // E
    for t in range(T):                                   # slot e * size + t of the fixture's buffer = env e, step t
        rows = np.arange(E) * size + t
        buf.add(SI.Batch(obs=g["obs"][rows], act=g["act"][rows], rew=g["rew"][rows], terminated=g["terminated"][rows],
                         truncated=g["truncated"][rows], obs_next=g["obs_next"][rows]))
    assert np.array_equal(buf.sample_indices(0), g["pre_indices"])
    algo.policy.is_within_training_step = True
    np.random.seed(seed + 100)
    stats = algo.update(buf, batch_size, repeat)
    assert isinstance(algo._hip_engine, NetPPOEngine) and stats.gradient_steps == int(g["gradient_steps"])
    for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
        ref = SI.SequenceSummaryStats.from_sequence(g["losses"][:, col])
        np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=2e-5, atol=2e-6)
    for i, p in enumerate(pa):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"a{i}_1"], rtol=1e-4, atol=0.02 * cfg["lr"], err_msg=f"a{i}")
    for i, p in enumerate(pc):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"c{i}_1"], rtol=1e-4, atol=0.02 * cfg["lr"], err_msg=f"c{i}")
    algo.state_dict()                                     # Adam moments arrive lazily, per parameter
    state = algo.optim._optim.state
    for i, p in enumerate(pa):
        np.testing.assert_allclose(state[p]["exp_avg"].cpu().numpy(), g[f"a{i}_m"], rtol=1e-3, atol=1e-6)
        assert state[p]["exp_avg"].shape == p.shape and float(state[p]["step"]) == stats.gradient_steps
    if not cs:      # the collector's forward on the engine (tianshou_amd.policy, "gauss_net") == the written-back torch modules'
        obs = g["obs"][:33]
        out = algo.policy(SI.Batch(obs=obs, info={}))
        with torch.no_grad():
            h = actor.preprocess.model.model(torch.as_tensor(obs, device="cuda"))       # (the stand-in MLPs are containers)
            mu_t = actor.mu.model(h)
        np.testing.assert_allclose(out.logits[0].cpu().numpy(), mu_t.cpu().numpy(), rtol=1e-5, atol=1e-5)



def _r6_optim(cfg):
    """(torch.optim class, kwargs) of the factory that wrote a round-6 fixture (cfg = its cfg_keys / cfg_vals)."""
    if cfg.get("opt_rmsprop"):
        return torch.optim.RMSprop, dict(eps=cfg["opt_eps"], alpha=cfg["rms_alpha"], weight_decay=cfg["weight_decay"],
                                         momentum=cfg["rms_momentum"], centered=bool(cfg["rms_centered"]))
    return torch.optim.Adam, dict(eps=cfg["opt_eps"], weight_decay=cfg["weight_decay"])


@pytest.mark.parametrize("tag", ["bounded", "a2c_rmsprop", "adam_wd"])
def test_hip_ppo_hooks_replay_the_reference_with_its_default_actor_and_other_optimizers(tag):
    """VERDICT r5 items 2 / 4 at hook level: `ContinuousActorProbabilistic(unbounded=False)` -- the constructor default,
    mu = max_action * tanh(.) (utils/net/continuous.py:194, 230-231) -- and the optimizer of examples/mujoco/mujoco_a2c.py:117
    (RMSprop(eps=1e-5, alpha=0.99), optim.py:113-140) / Adam with weight decay (optim.py:95-109).  HipPPO / HipA2C over the
    stand-ins, production hook code on the fused engine: two update() calls on the buffer contents, weights and NumPy seeds of
    the REFERENCE's own run (tests/golden/ppo_<tag>.npz, oracle/gen_golden.py::gen_ppo_round6) reproduce its per-step losses,
    parameters, optimizer state (through state_dict()'s lazy flush, in torch.optim's own keys) and return statistics."""
    import os

    from tianshou_amd.integration import make_hip_ppo
    from tianshou_amd.ppo import PPOEngine, flat_from_modules

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"ppo_{tag}.npz"))
    cfg = dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]]))
    E, T, obs_dim, act_dim, batch_size, repeat, n_updates = (int(x) for x in g["dims"])
    seed = {"bounded": 21, "a2c_rmsprop": 22, "adam_wd": 23}[tag]
    a2c = cfg["is_a2c"] > 0
    bounded = cfg["max_action"] > 0
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, [64, 64], nn.Tanh), act_dim, unbounded=not bounded,
                                            max_action=cfg["max_action"] or 1.0)
    critic = SI.ContinuousCritic(SI.Net(obs_dim, [64, 64], nn.Tanh))
    p0 = OP.unflatten_params(torch.from_numpy(g["flat_params0"]), obs_dim, act_dim)
    from tianshou_amd.ppo import TIANSHOU_ACTOR_KEYS, TIANSHOU_CRITIC_KEYS

    with torch.no_grad():
        for mod, keys, names in ((actor, TIANSHOU_ACTOR_KEYS, OP.PARAM_ORDER[:7]), (critic, TIANSHOU_CRITIC_KEYS, OP.PARAM_ORDER[7:])):
            named = dict(mod.named_parameters())
            for k, nme in zip(keys, names):
                named[k].copy_(p0[nme].reshape(named[k].shape))
    kw = dict(vf_coef=cfg["vf_coef"], ent_coef=cfg["ent_coef"], max_grad_norm=cfg["max_grad_norm"] or None,
              return_scaling=bool(cfg["return_scaling"]), gae_lambda=cfg["gae_lambda"], gamma=cfg["gamma"], lr=cfg["lr"],
              optim=_r6_optim(cfg))
    if not a2c:
        kw.update(eps_clip=cfg["eps_clip"], dual_clip=cfg["dual_clip"] or None, value_clip=bool(cfg["value_clip"]),
                  advantage_normalization=bool(cfg["advantage_normalization"]))
    algo = make_hip_ppo("a2c" if a2c else "ppo", ref=SI)(policy=SI.Policy(actor), critic=critic, device="cuda",
                                                          permutations="host", **kw).to("cuda")
    assert algo._hip_dims == (obs_dim, act_dim, 64, "fused")
    algo.policy.is_within_training_step = True
    for u in range(n_updates):
        pre_ = "" if u == 0 else f"u{u}_"
        buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
        size = buf.maxsize // E
        for t in range(T):                                   # slot e * size + t of the fixture's buffer = env e, step t
            rows = np.arange(E) * size + t
            buf.add(SI.Batch(obs=g[pre_ + "obs"][rows], act=g[pre_ + "act"][rows], rew=g[pre_ + "rew"][rows],
                             terminated=g[pre_ + "terminated"][rows], truncated=g[pre_ + "truncated"][rows],
                             obs_next=g[pre_ + "obs_next"][rows]))
        np.random.seed(seed + 100 + u)
        stats = algo.update(buf, batch_size, repeat)
        assert isinstance(algo._hip_engine, PPOEngine) and stats.gradient_steps == int(g[f"u{u}_gradient_steps"])
        assert (algo._hip_engine.cfg.max_action or 0.0) == cfg["max_action"]
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SI.SequenceSummaryStats.from_sequence(g[f"u{u}_losses"][:, col])
            np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=1e-5, atol=2e-6)
        flat = flat_from_modules(algo.policy.actor, algo.critic, device="cpu").numpy()
        np.testing.assert_allclose(flat, g[f"u{u}_flat_params"], rtol=1e-4, atol=3e-6)
        np.testing.assert_allclose([algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count], g[f"u{u}_ret_rms"], rtol=1e-5)
    algo.state_dict()                                         # optimizer state arrives lazily, under torch.optim's own keys
    state, params = algo.optim._optim.state, algo._hip_params()
    k_m, k_v = ("exp_avg", "exp_avg_sq") if not cfg["opt_rmsprop"] else (None, "square_avg")
    v_flat = torch.cat([state[p][k_v].reshape(-1).cpu() for p in params]).numpy()
    np.testing.assert_allclose(v_flat, g[f"u{n_updates - 1}_adam_v"], rtol=1e-3, atol=1e-10)
    if k_m:
        m_flat = torch.cat([state[p][k_m].reshape(-1).cpu() for p in params]).numpy()
        np.testing.assert_allclose(m_flat, g[f"u{n_updates - 1}_adam_m"], rtol=1e-3, atol=1e-7)
    else:
        assert all("momentum_buffer" not in state[p] and "grad_avg" not in state[p] for p in params)
    assert all(float(state[p]["step"]) == sum(int(g[f"u{u}_gradient_steps"]) for u in range(n_updates)) for p in params)


def test_hip_ppo_hooks_replay_a_bounded_actor_on_the_per_layer_engine():
    """The reference's default (bounded) actor over a three-layer ReLU trunk with RMSprop: HipPPO picks the per-layer engine
    (ts_net_desc.max_action) and reproduces the REFERENCE's update (tests/golden/ppo_net_bounded_relu3.npz)."""
    import os

    from tianshou_amd.integration import make_hip_ppo
    from tianshou_amd.ppo_wide import NetPPOEngine

    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "ppo_net_bounded_relu3.npz")))
    cfg = dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]]))
    E, T, obs_dim, act_dim, batch_size, repeat = (int(x) for x in g["dims"])
    ha, hc = [int(x) for x in g["hidden_a"]], [int(x) for x in g["hidden_c"]]
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, ha, nn.ReLU), act_dim, unbounded=False, max_action=float(g["max_action"]))
    critic = SI.ContinuousCritic(SI.Net(obs_dim, hc, nn.ReLU))

    def params(mod, head, extra=()):
        lin = [m for m in mod.preprocess.model.model if isinstance(m, nn.Linear)] + [m for m in head.modules() if isinstance(m, nn.Linear)]
        out = []
        for m in lin:
            out += [m.weight, m.bias]
        return out + list(extra)

    pa, pc = params(actor, actor.mu, [actor.sigma_param]), params(critic, critic.last)
    with torch.no_grad():
        for i, p in enumerate(pa):
            p.copy_(torch.from_numpy(g[f"a{i}_0"]))
        for i, p in enumerate(pc):
            p.copy_(torch.from_numpy(g[f"c{i}_0"]))
    kw = dict(eps_clip=cfg["eps_clip"], dual_clip=cfg["dual_clip"] or None, value_clip=bool(cfg["value_clip"]),
              advantage_normalization=bool(cfg["advantage_normalization"]), vf_coef=cfg["vf_coef"], ent_coef=cfg["ent_coef"],
              max_grad_norm=cfg["max_grad_norm"] or None, return_scaling=bool(cfg["return_scaling"]), gae_lambda=cfg["gae_lambda"],
              gamma=cfg["gamma"], lr=cfg["lr"], optim=_r6_optim(cfg))
    algo = make_hip_ppo("ppo", ref=SI)(policy=SI.Policy(actor), critic=critic, device="cuda", permutations="host", **kw).to("cuda")
    assert algo._hip_dims[3] == "net"
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    size = buf.maxsize // E
    for t in range(T):
        rows = np.arange(E) * size + t
        buf.add(SI.Batch(obs=g["obs"][rows], act=g["act"][rows], rew=g["rew"][rows], terminated=g["terminated"][rows],
                         truncated=g["truncated"][rows], obs_next=g["obs_next"][rows]))
    algo.policy.is_within_training_step = True
    np.random.seed(26 + 100)
    stats = algo.update(buf, batch_size, repeat)
    assert isinstance(algo._hip_engine, NetPPOEngine) and stats.gradient_steps == int(g["gradient_steps"])
    for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
        ref = SI.SequenceSummaryStats.from_sequence(g["losses"][:, col])
        np.testing.assert_allclose([s.mean, s.max, s.min], [ref.mean, ref.max, ref.min], rtol=2e-5, atol=2e-6)
    for i, p in enumerate(pa):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"a{i}_1"], rtol=1e-4, atol=0.02 * cfg["lr"], err_msg=f"a{i}")
    for i, p in enumerate(pc):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"c{i}_1"], rtol=1e-4, atol=0.02 * cfg["lr"], err_msg=f"c{i}")
    algo.state_dict()
    state = algo.optim._optim.state
    for i, p in enumerate(pa):
        np.testing.assert_allclose(state[p]["square_avg"].cpu().numpy(), g[f"a{i}_v"], rtol=2e-3, atol=1e-9)
        assert "momentum_buffer" not in state[p] and float(state[p]["step"]) == stats.gradient_steps



@pytest.mark.parametrize("tag", ["npg_widths", "trpo_widths", "npg_relu3", "trpo_tanh1"])
def test_hip_natural_gradient_hooks_replay_the_reference_on_other_widths(tag):
    """HipNPG / HipTRPO on two-hidden-layer tanh networks whose widths are neither equal nor multiples of 32 (actor [48, 80] /
    critic [40, 56]; actor [100, 60] / critic [60, 100]) against what the unmodified REFERENCE's NPG.update() / TRPO.update()
    produced on them (tests/golden/npg_{npg,trpo}_widths.npz, oracle/gen_golden.py::gen_npg): the engine runs the networks
    embedded in Net[96, 96] / Net[128, 128] by zero padding (tianshou_amd/widths.py) -- conjugate gradients, Fisher-vector
    products, TRPO's line search and the critic's Adam steps never move a padding entry.  Same buffer, initial weights and
    `np.random.permutation` stream; tolerances of tests/test_gpu_npg.py (both sides are float32 CG solves).
    `npg_relu3` / `trpo_tanh1` (round 6): trunks outside two tanh layers -- NPG on three ReLU layers (actor [64, 48, 32], critic
    [40, 56]), TRPO on one tanh layer ([96] / [80]) -- pick NetNPGEngine (layer by layer on the GEMM kernels)."""
    from tests.test_oracle_golden import load_npg
    from tianshou_amd.integration import make_hip_npg, make_hip_trpo

    g, d, cfg = load_npg(tag)
    obs_dim, act_dim, E, T = d["obs_dim"], d["act_dim"], d["E"], d["T"]
    generic = "hidden_a" in g
    if generic:
        ha, hc = [int(x) for x in g["hidden_a"]], [int(x) for x in g["hidden_c"]]
        act_cls = {0: nn.Tanh, 1: nn.ReLU, 2: None}[int(g["activation"])]
    else:
        ha, hc, act_cls = [int(x) for x in g["hidden"][:2]], [int(x) for x in g["hidden"][2:]], nn.Tanh
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, ha, act_cls), act_dim, unbounded=True)
    critic = SI.ContinuousCritic(SI.Net(obs_dim, hc, act_cls))
    trunk = lambda n: [f"preprocess.model.model.{2 * i}.{x}" for i in range(n) for x in ("weight", "bias")]      # noqa: E731
    keys_a = trunk(len(ha)) + ["mu.model.0.weight", "mu.model.0.bias", "sigma_param"]
    keys_c = trunk(len(hc)) + ["last.model.0.weight", "last.model.0.bias"]

    def load_flat(flat):
        off = 0
        for mod, keys in ((actor, keys_a), (critic, keys_c)):
            sd = mod.state_dict()
            for k in keys:
                n = sd[k].numel()
                sd[k].copy_(torch.as_tensor(flat[off:off + n]).reshape(sd[k].shape))
                off += n
        assert off == flat.size

    def dump_flat():
        return torch.cat([mod.state_dict()[k].reshape(-1).cpu() for mod, keys in ((actor, keys_a), (critic, keys_c)) for k in keys]).numpy()

    load_flat(g["flat_params0"])
    which = "trpo" if cfg.algo == "trpo" else "npg"
    kw = dict(lr=cfg.lr, optim_critic_iters=cfg.optim_critic_iters, advantage_normalization=cfg.advantage_normalization,
              gae_lambda=cfg.gae_lambda, gamma=cfg.gamma, return_scaling=cfg.return_scaling, max_batchsize=cfg.max_batchsize)
    if which == "npg":
        kw["trust_region_size"] = cfg.trust_region_size
    else:
        kw.update(max_kl=cfg.max_kl, backtrack_coeff=cfg.backtrack_coeff, max_backtracks=cfg.max_backtracks)
    algo = (make_hip_npg if which == "npg" else make_hip_trpo)(ref=SI)(policy=SI.Policy(actor), critic=critic, device="cuda", **kw).to("cuda")
    if generic:
        assert not algo._hip_two and algo._hip_trunks[:2] == (ha, hc)
    else:
        assert algo._hip_hidden % 32 == 0 and algo._hip_sizes == {"actor": tuple(ha), "critic": tuple(hc)}
    buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated"):
        getattr(buf, k)[:] = g[k]
    buf.done[:] = g["terminated"] | g["truncated"]
    buf._lengths[:], buf.last_index[:] = g["buf_lengths"], g["buf_last_index"]
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
    assert np.array_equal(buf.sample_indices(0), g["pre_indices"])
    algo.policy.is_within_training_step = True
    np.random.seed(int(g["seed"]) + 100)                                 # gen_npg: the reference's permutation stream
    stats = algo.update(buf, d["batch_size"], d["repeat"])
    cols = [stats.actor_loss, stats.vf_loss, stats.kl] + ([stats.step_size] if which == "trpo" else [])
    for col, s_ in enumerate(cols):
        r = SI.SequenceSummaryStats.from_sequence(g["stats"][:, col])
        np.testing.assert_allclose([s_.mean, s_.max, s_.min], [r.mean, r.max, r.min], rtol=2e-3, atol=2e-5)
    got, want, before = dump_flat(), g["flat_params"], g["flat_params0"]
    moved = np.abs(want - before).max()
    assert moved > 0 and np.abs(got - want).max() <= 2e-3 * moved + 1e-6, (np.abs(got - want).max(), moved)
    # the embedding stayed an embedding: every padding entry of the engine's vectors is still exactly zero
    from tianshou_amd import npg as NG
    from tianshou_amd import widths as W

    eng = algo._hip_engine
    if generic:
        assert isinstance(eng, NG.NetNPGEngine)
        return
    assert W.padding_is_zero(NG.actor_flat_to_torch(eng.actor, obs_dim, eng.hidden, act_dim)[:6], *ha)
    for vec in (eng.critic, eng.critic_m, eng.critic_v):
        assert W.padding_is_zero(NG.critic_flat_to_torch(vec, obs_dim, eng.hidden), *hc)


@pytest.mark.parametrize("tag", ["auto", "fixed", "widths", "depth3", "depth1", "bounded", "bounded_depth3", "tanh"])
def test_hip_sac_hooks_replay_the_reference(tag, monkeypatch):
    """VERDICT r5 item 8 for the SAC family: the HOOK path -- device mirror of a host buffer, `_preprocess_batch` (n-step
    target with the lagged critics; n = 1 and 3), `_update_with_batch` (twin critics, actor, alpha, Polyak), write-back -- on the
    real engine against what the unmodified REFERENCE's SAC.update() produced (tests/golden/sac_{auto,fixed}.npz,
    oracle/gen_golden.py::gen_sac): same buffer contents and initial weights, the reference's own minibatch indices and the
    rsample() noise it drew (the hooks draw `torch.randn` where the reference draws: the two calls per update are served from
    the fixture)."""
    from oracle import oracle_sac as OS
    from tests.test_oracle_golden import load_sac
    from tianshou_amd.integration import make_hip_sac

    g, d, cfg, _ = load_sac(tag)
    obs_dim, act_dim, E, B = d["obs_dim"], d["act_dim"], d["E"], d["batch"]
    # `widths`: actor Net[48, 80], critics Net[72, 40] -- run embedded in Net[96, 96]; `depth3`: actor [64, 48, 32], critics
    # [40, 56, 24]; `depth1`: one hidden layer [96] (round 6: any depth, layer by layer on the GEMM kernels)
    sa, sc = OS.layer_sizes(d["hidden"])
    # `bounded*`: the class-default actor, unbounded=False with max_action 1.5 / 0.8 (mu = max_action * tanh(mu))
    fn = nn.Tanh if d["activation"] == "tanh" else nn.ReLU             # (`tanh`: Net(activation=nn.Tanh) trunks)
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, list(sa), fn), act_dim, unbounded=cfg.max_action == 0.0,
                                            conditioned_sigma=True, max_action=cfg.max_action or 1.0)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, list(sc), fn))
    c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, list(sc), fn))
    p0 = OS.init_sac_params(obs_dim, act_dim, d["seed"], (sa, sc))        # == the reference's initial weights (asserted by gen_sac)
    for mod, pd in ((actor, p0[0]), (c1, p0[1]), (c2, p0[2])):            # (both in layer order: trunk, then heads)
        mod.load_state_dict(dict(zip(mod.state_dict(), pd.values())))
    alpha = SI.AutoAlpha(cfg.target_entropy, cfg.log_alpha0, cfg.alpha_lr) if cfg.auto_alpha else SI.FixedAlpha(cfg.alpha)
    algo = make_hip_sac(ref=SI)(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=cfg.actor_lr, critic_lr=cfg.critic_lr, tau=cfg.tau,
                                gamma=cfg.gamma, alpha=alpha, n_step_return_horizon=cfg.n_step, device="cuda",
                                update_noise="torch").to("cuda")         # (index-only sampling + lazy write-back: the defaults)
    assert algo._hip_depth == len(sa) and algo._hip_sizes["actor"] == tuple(sa) and algo._hip_bound == cfg.max_action
    assert algo._hip_actfn == d["activation"]
    buf = SI.VectorReplayBuffer(E * d["slots"], E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    lengths = g["buf_lengths"]
    for t in range(int(lengths.max())):                                   # slot e * slots + t of the fixture's buffer = env e, step t
        rows = np.arange(E) * d["slots"] + t
        buf.add(SI.Batch(obs=g["obs"][rows], act=g["act"][rows], rew=g["rew"][rows], terminated=g["terminated"][rows],
                         truncated=g["truncated"][rows], obs_next=g["obs_next"][rows]))
    assert np.array_equal(buf._lengths, lengths) and np.array_equal(buf.last_index, g["buf_last_index"])
    algo.policy.is_within_training_step = True
    real_randn = torch.randn
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        monkeypatch.setattr(buf, "sample_indices", lambda bs, idx=idx: idx)
        served = [torch.from_numpy(g[f"u{u}_noise_target"]), torch.from_numpy(g[f"u{u}_noise_actor"])]

        def randn(*a, **k):
            if not served or k.get("device") is not None:
                return real_randn(*a, **k)
            return served.pop(0).clone()

        monkeypatch.setattr(torch, "randn", randn)
        stats = algo.update(buf, B)
        monkeypatch.setattr(torch, "randn", real_randn)
        assert not served                                                 # both draws were consumed, in the reference's order
        ref = g[f"u{u}_stats"]
        np.testing.assert_allclose([stats.actor_loss, stats.critic1_loss, stats.critic2_loss], ref[:3], rtol=2e-5)
        np.testing.assert_allclose(stats.alpha, ref[3], rtol=1e-5)
        if cfg.auto_alpha:
            np.testing.assert_allclose(stats.alpha_loss, ref[4], rtol=1e-5, atol=1e-6)
        algo.hip_sync()                                                   # lazy write-back: the torch modules are read below
        for name, mod in (("actor", actor), ("critic1", c1), ("critic2", c2), ("critic1_old", algo.critic_old.module),
                          ("critic2_old", algo.critic2_old.module)):
            flat = torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu().numpy()
            lr = cfg.actor_lr if name == "actor" else cfg.critic_lr
            np.testing.assert_allclose(flat[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=0.02 * lr, err_msg=f"update {u}: {name}")



def test_hip_dqn_hooks_replay_the_reference():
    """VERDICT r5 item 8 for the DQN family: the HOOK path on the real engine against what the unmodified REFERENCE's
    DQN.update() produced on the Atari layout of examples/atari/atari_dqn.py:137-142 (tests/golden/dqn_atari.npz,
    oracle/gen_golden.py::gen_dqn: single uint8 frames per slot, stack_num 4, no stored obs_next, wrapped sub-buffers, a
    prioritized buffer, n-step 3, double-Q with a lagged network, Huber): the buffer state is the fixture's, `sample` returns the
    reference's own minibatch indices, and per update the importance weights the stand-in buffer attaches, the TD errors that
    reach `update_weight`, the loss and the parameters equal the reference's."""
    from oracle import oracle_dqn as OD
    from tests import dqn_common as DC
    from tianshou_amd import dqn as D
    from tianshou_amd.integration import make_hip_dqn

    g, d, ocfg, _ = DC.load("atari")
    c, h, w, A, E, B = d["c"], d["h"], d["w"], d["n_act"], d["E"], d["batch"]
    assert d["per"] and d["stack"]
    model = SI.DQNet(c, h, w, A)
    p0 = OD.init_params(c, h, w, A, d["seed"])                            # == the reference's initial weights (asserted by gen_dqn)
    model.load_state_dict({name: p0[k] for name, k in zip(D.TIANSHOU_KEYS, OD.PARAM_ORDER)})
    algo = make_hip_dqn(ref=SI)(policy=SI.DiscreteQLearningPolicy(model), lr=ocfg.lr, gamma=ocfg.gamma,
                                n_step_return_horizon=ocfg.n_step, target_update_freq=ocfg.target_update_freq,
                                is_double=ocfg.is_double, huber_loss_delta=ocfg.huber_delta, device="cuda", host_batch=True,
                                write_back="eager").to("cuda")
    buf = SI.PrioritizedVectorReplayBuffer(E * d["slots"], E, obs_shape=(h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                           stack_num=c, alpha=0.6, beta=0.4)
    buf._meta = SI._Meta(("obs", "act", "rew", "terminated", "truncated", "done"))        # ignore_obs_next=True
    buf.obs[:], buf.act[:], buf.rew[:] = g["frames"], g["act"], g["rew"]
    buf.terminated[:], buf.truncated[:] = g["terminated"], g["truncated"]
    buf.done[:] = g["terminated"] | g["truncated"]
    buf._lengths[:], buf.last_index[:] = g["buf_lengths"], g["buf_last_index"]
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
    assert bool((g["buf_insertion"] > 0).any()) and int(g["buf_lengths"].min()) == d["slots"]      # every sub-buffer has wrapped
    n_leaf = E * d["slots"]
    bound = 1
    while bound < n_leaf:
        bound *= 2
    buf.prio[:] = g["tree0"][bound:bound + n_leaf]                        # the reference's sum-tree leaves before the first update
    assert np.all(buf.prio == 1.0)                                        # new slots: max_prio ** alpha with max_prio = 1
    algo.policy.is_within_training_step = True
    eps = np.finfo(np.float32).eps.item()
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        buf.sample_indices = lambda bs, idx=idx: idx
        seen = {}
        orig = SI.PrioritizedVectorReplayBuffer.sample

        def sample(bs, seen=seen):
            batch, i = orig(buf, bs)
            seen["w"] = np.asarray(batch.weight).copy()
            return batch, i

        buf.sample = sample
        stat = algo.update(buf, B)
        np.testing.assert_allclose(seen["w"], g[f"u{u}_is_weight"], rtol=1e-6)                   # prio.py:69-79 on the same priorities
        np.testing.assert_allclose(stat.loss, float(g[f"u{u}_loss"]), rtol=1e-5)
        upd_idx, upd_w = buf.weight_updates[-1]
        assert np.array_equal(upd_idx, idx)
        np.testing.assert_allclose(upd_w, np.abs(g[f"u{u}_td"]) + eps, rtol=1e-5, atol=2e-5)
        tensors = [p.detach().cpu() for p in model.parameters()]
        flat = torch.cat([t.reshape(-1) for t in tensors]).numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-5, atol=0.02 * ocfg.lr)
        np.testing.assert_allclose(tensors[0].numpy(), g[f"u{u}_conv1_w"], rtol=1e-5, atol=0.02 * ocfg.lr)
        lo, hi = g[f"u{u}_prio_minmax"]
        np.testing.assert_allclose([buf._min_prio, buf._max_prio], sorted([float(lo), float(hi)]), rtol=1e-4)



@pytest.mark.parametrize("tag", ["twin", "ddpg", "widths", "ddpg_widths", "depth4", "ddpg_depth1", "tanh3"])
def test_hip_td3_ddpg_hooks_replay_the_reference(tag, monkeypatch):
    """VERDICT r5 item 8 for the deterministic-actor family: HipTD3 / HipDDPG hook paths on the real engine against what the
    unmodified REFERENCE's TD3.update() / DDPG.update() produced (tests/golden/td3_{twin,ddpg}.npz,
    oracle/gen_golden.py::gen_td3): its minibatch indices, its target-policy smoothing noise (the hooks' one `torch.randn` per
    update is served from the fixture), max_action 2 and n-step 2 for DDPG, the delayed actor step and the three / two Polyak
    updates."""
    from oracle import oracle_sac as OS
    from tests.test_oracle_golden import load_td3
    from tianshou_amd.integration import make_hip_ddpg, make_hip_td3

    g, d, cfg, _ = load_td3(tag)
    obs_dim, act_dim, B, twin = d["obs_dim"], d["act_dim"], d["batch"], d["twin"]
    E, slots = int(g["dims"][0]), int(g["dims"][1])
    # `widths`: Net[400, 300] (embedded in 416); `ddpg_widths`: actor [24, 56], critic [40, 24]; `depth4`: four hidden layers, actor
    # [64, 64, 32, 32], critics [48, 64, 64, 40]; `ddpg_depth1`: one hidden layer, actor [128], critic [64] (round 6)
    sa, sc = OS.layer_sizes(d["hidden"])
    fn = nn.Tanh if d["activation"] == "tanh" else nn.ReLU             # (`tanh3`: three nn.Tanh layers per network)
    actor = SI.ContinuousActorDeterministic(SI.Net(obs_dim, list(sa), fn), act_dim, max_action=cfg.max_action)
    c1 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, list(sc), fn))
    c2 = SI.ContinuousCritic(SI.Net(obs_dim + act_dim, list(sc), fn)) if twin else None
    p0 = OS.init_td3_params(obs_dim, act_dim, d["seed"], twin, (sa, sc))  # == the reference's initial weights (asserted by gen_td3)
    for mod, pd in ((actor, p0[0]), (c1, p0[1])) + (((c2, p0[2]),) if twin else ()):
        mod.load_state_dict(dict(zip(mod.state_dict(), pd.values())))
    if twin:
        algo = make_hip_td3(ref=SI)(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=cfg.actor_lr, critic_lr=cfg.critic_lr, tau=cfg.tau,
                                    gamma=cfg.gamma, policy_noise=cfg.policy_noise, update_actor_freq=cfg.update_actor_freq,
                                    noise_clip=cfg.noise_clip, n_step_return_horizon=cfg.n_step, device="cuda").to("cuda")
    else:
        algo = make_hip_ddpg(ref=SI)(policy=SI.Policy(actor), critic=c1, lr=cfg.actor_lr, critic_lr=cfg.critic_lr, tau=cfg.tau,
                                     gamma=cfg.gamma, n_step_return_horizon=cfg.n_step, device="cuda").to("cuda")
    buf = SI.VectorReplayBuffer(E * slots, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated"):
        getattr(buf, k)[:] = g[k]
    buf.done[:] = g["terminated"] | g["truncated"]
    buf._lengths[:], buf.last_index[:] = g["buf_lengths"], g["buf_last_index"]
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = int(g["buf_lengths"][e]), int(g["buf_insertion"][e])
    algo.policy.is_within_training_step = True
    real_randn = torch.randn
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        buf.sample_indices = lambda bs, idx=idx: idx
        served = [torch.from_numpy(g[f"u{u}_noise"])] if twin else []

        def randn(*a, **k):
            if not served or k.get("device") is not None:
                return real_randn(*a, **k)
            return served.pop(0).clone()

        monkeypatch.setattr(torch, "randn", randn)
        stats = algo.update(buf, B)
        monkeypatch.setattr(torch, "randn", real_randn)
        assert not served
        ref = g[f"u{u}_stats"]
        got = [stats.actor_loss, stats.critic1_loss, stats.critic2_loss] if twin else [stats.actor_loss, stats.critic_loss]
        np.testing.assert_allclose(got, ref[:len(got)], rtol=2e-5, atol=2e-6)
        mods = [("actor", actor, cfg.actor_lr), ("critic1", c1, cfg.critic_lr), ("actor_old", algo.actor_old.module, cfg.actor_lr),
                ("critic1_old", algo.critic_old.module, cfg.critic_lr)]
        if twin:
            mods += [("critic2", c2, cfg.critic_lr), ("critic2_old", algo.critic2_old.module, cfg.critic_lr)]
        for name, mod, lr in mods:
            flat = torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu().numpy()
            want = g[f"u{u}_{name}"]
            np.testing.assert_allclose(flat[::61] if want.shape != flat.shape else flat, want, rtol=1e-5, atol=0.02 * lr,
                                       err_msg=f"update {u}: {name}")



@pytest.mark.parametrize("tag", ["net_relu3", "net_tanh1", "net_ln_relu2"])
def test_hip_reinforce_hooks_on_generic_trunks_replay_the_reference(tag):
    """Round 6 (VERDICT r5 Missing #3, Reinforce): HipReinforce on actors outside Net[h, h] tanh -- a three-layer ReLU trunk
    under the reference's default BOUNDED actor (max_action 1.5) with RMSprop and return standardisation; one wide tanh layer
    with Adam + weight decay -- picks the per-layer engine (reinforce.NetReinforceEngine) and reproduces, through the hooks,
    what the unmodified REFERENCE's Reinforce.update() produced on the same rollouts, weights and NumPy seeds
    (tests/golden/reinforce_net_*.npz, oracle/gen_golden.py::gen_reinforce_net): returns, per-step losses, parameters, the
    optimizer's second-moment state and the running return statistics."""
    import os

    from tianshou_amd.integration import make_hip_reinforce
    from tianshou_amd.reinforce import NetReinforceEngine

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"reinforce_{tag}.npz"))
    cfg = dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]]))
    E, T, obs_dim, act_dim, batch_size, repeat, n_updates = (int(x) for x in g["dims"])
    hidden = [int(h) for h in g["hidden"]]
    act_cls = {0: nn.Tanh, 1: nn.ReLU, 2: None}[int(g["activation"])]
    max_action = float(g["max_action"])
    seed = {"net_relu3": 55, "net_tanh1": 56, "net_ln_relu2": 57}[tag]
    nkw = dict(norm_layer=nn.LayerNorm, norm_args=dict(eps=float(g["ln_eps"]))) if "ln_eps" in g.files else {}   # common.py:25-39
    actor = SI.ContinuousActorProbabilistic(SI.Net(obs_dim, hidden, act_cls, **nkw), act_dim, unbounded=max_action == 0,
                                            max_action=max_action or 1.0)
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(actor.state_dict().keys())
    actor.load_state_dict({k: torch.from_numpy(g[f"a{i}_0"]) for i, k in enumerate(keys)})
    algo = make_hip_reinforce(ref=SI)(policy=SI.Policy(actor), lr=cfg["lr"], gamma=cfg["gamma"],
                                      return_standardization=bool(cfg["return_standardization"]), max_grad_norm=cfg["max_grad_norm"] or None,
                                      optim=_r6_optim(cfg), device="cuda").to("cuda")
    assert algo._hip_kind == "net"
    algo.policy.is_within_training_step = True
    named = dict(actor.named_parameters())
    for u in range(n_updates):
        buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=(act_dim,))
        size = buf.maxsize // E
        for t in range(T):                                   # slot e * size + t of the fixture's buffer = env e, step t
            rows = np.arange(E) * size + t
            nxt = np.where(t + 1 < T, rows + 1, rows)
            buf.add(SI.Batch(obs=g[f"u{u}_obs"][rows], act=g[f"u{u}_act"][rows], rew=g[f"u{u}_rew"][rows],
                             terminated=g[f"u{u}_terminated"][rows], truncated=g[f"u{u}_truncated"][rows], obs_next=g[f"u{u}_obs"][nxt]))
        assert np.array_equal(buf.sample_indices(0), g[f"u{u}_indices"])
        np.random.seed(seed + 100 + u)
        seen = {}
        orig_pre = type(algo)._preprocess_batch

        def pre(batch, buffer, indices, seen=seen):
            b = orig_pre(algo, batch, buffer, indices)
            seen["returns"] = b.returns.detach().cpu().numpy().copy()
            return b

        algo._preprocess_batch = pre
        stats = algo.update(buf, batch_size or None, repeat)
        del algo._preprocess_batch
        assert isinstance(algo._hip_engine, NetReinforceEngine)
        np.testing.assert_allclose(seen["returns"], g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        ref = SI.SequenceSummaryStats.from_sequence(g[f"u{u}_losses"])
        np.testing.assert_allclose([stats.loss.mean, stats.loss.max, stats.loss.min], [ref.mean, ref.max, ref.min], rtol=2e-5, atol=2e-6)
        for i, k in enumerate(keys):
            np.testing.assert_allclose(named[k].detach().cpu().numpy(), g[f"u{u}_a{i}"], rtol=1e-4, atol=0.02 * cfg["lr"], err_msg=f"update {u}: {k}")
        drc = algo.discounted_return_computation
        np.testing.assert_allclose([drc.ret_rms.mean, drc.ret_rms.var, drc.ret_rms.count], g[f"u{u}_ret_rms"], rtol=1e-6)
        state = algo.optim._optim.state
        k_v = "square_avg" if cfg["opt_rmsprop"] else "exp_avg_sq"
        for i, k in enumerate(keys):
            np.testing.assert_allclose(state[named[k]][k_v].cpu().numpy(), g[f"u{u}_a{i}_v"], rtol=2e-3, atol=1e-9, err_msg=f"update {u}: {k} v")


# ------------------------------------------------------------------------------------ a rebuilt engine continues (eager bodies)
def _ac_resume_algo(which):
    """HipTD3 / HipDDPG / HipDiscreteSAC / HipREDQ over the stand-ins: observations of 11, 3 actions (5 discrete ones), trunks
    [48, 40] -- unequal widths, no multiple of 32, so the state path goes through the zero-padding embed and `sizes=`."""
    from tianshou_amd import integration as I

    obs_dim, act_dim, n_act, H = 11, 3, 5, [48, 40]
    torch.manual_seed(71)
    net = lambda d, **kw: SI.Net(d, H, nn.ReLU, **kw)   # noqa: E731
    if which in ("td3", "ddpg"):
        actor = SI.ContinuousActorDeterministic(net(obs_dim), act_dim, max_action=1.0)
        kw = dict(policy=SI.Policy(actor), critic=SI.ContinuousCritic(net(obs_dim + act_dim)), lr=3e-4, critic_lr=1e-3, tau=0.01,
                  gamma=0.98, device="cuda")
        if which == "td3":
            algo = I.make_hip_td3(ref=SI)(critic2=SI.ContinuousCritic(net(obs_dim + act_dim)), policy_noise=0.2,
                                          update_actor_freq=2, noise_clip=0.5, **kw)
        else:
            algo = I.make_hip_ddpg(ref=SI)(**kw)
    elif which == "redq":
        lin = lambda x, y: SI.EnsembleLinear(3, x, y)   # noqa: E731
        actor = SI.ContinuousActorProbabilistic(net(obs_dim), act_dim, unbounded=True, conditioned_sigma=True)
        critic = SI.ContinuousCritic(net(obs_dim + act_dim, linear_layer=lin), linear_layer=lin)
        algo = I.make_hip_redq(ref=SI)(policy=SI.Policy(actor), critic=critic, lr=3e-4, critic_lr=1e-3, ensemble_size=3, subset_size=2,
                                       tau=0.01, gamma=0.97, alpha=SI.AutoAlpha(-float(act_dim), -0.6, 3e-4), actor_delay=2,
                                       target_mode="min", device="cuda")
    else:
        actor = SI.DiscreteActor(net(obs_dim), n_act, softmax_output=False)
        c1, c2 = SI.DiscreteCritic(net(obs_dim), last_size=n_act), SI.DiscreteCritic(net(obs_dim), last_size=n_act)
        algo = I.make_hip_discrete_sac(ref=SI)(policy=SI.Policy(actor), critic=c1, critic2=c2, lr=3e-4, critic_lr=1e-3, tau=0.02, gamma=0.96,
                                               alpha=SI.AutoAlpha(0.98 * float(np.log(n_act)), -0.4, 3e-4), device="cuda",
                                               match_rng_stream=which == "dsac_match_rng")
    algo = algo.to("cuda")
    assert algo._hip_hidden == 64 and algo._hip_sizes["actor"] == (48, 40)
    algo.policy.is_within_training_step = True
    discrete = which.startswith("dsac")
    buf = SI.VectorReplayBuffer(4 * 100, 4, obs_shape=(obs_dim,), act_shape=() if discrete else (act_dim,),
                                act_dtype=np.int64 if discrete else np.float32, seed=72)
    rng = np.random.default_rng(73)
    obs = rng.normal(size=(61, 4, obs_dim)).astype(np.float32)
    for t in range(60):                                                          # 240 rows, about 5 % terminals
        term = rng.random(4) < 0.05
        act = rng.integers(0, n_act, 4) if discrete else rng.normal(size=(4, act_dim)).astype(np.float32)
        buf.add(SI.Batch(obs=obs[t], act=act, rew=rng.normal(size=4).astype(np.float32), terminated=term,
                         truncated=(rng.random(4) < 0.03) & ~term, obs_next=obs[t + 1]))
    return algo, buf


def _ac_resume_optimizers(algo):
    opts = [o._optim for o in algo._optimizers]
    return opts + ([algo.alpha._optim] if hasattr(getattr(algo, "alpha", None), "_optim") else [])


@pytest.mark.parametrize("which", ["td3", "ddpg", "dsac_match_rng", "dsac_no_draws", "redq"])
def test_hip_actor_critic_rebuilt_engine_continues_where_the_last_one_stopped(which):
    """The torch<->engine state path of the eager off-policy actor-critic bodies, both directions, on the real engine: run A makes
    four updates; run B, seeded alike, makes two, drops its engine (`_hip_invalidate()`: the next update builds a new one from the
    torch modules and torch.optim) and makes two more.  Write-back and load are plain fp32 copies, so B ends bit for bit where A
    does: every online and lagged parameter, log alpha, every optimizer's moments and step, the last update's statistics.
    (HipDDPG: the critic's Adam step is the engine's `cnt`, which the hooks keep in `_cnt` as for TD3; without it the rebuilt engine
    restarted that count at 0 and the critic ended up to 0.87 lr away, its `step` at 2 instead of 4.)"""
    import dataclasses

    def run(algo, buf, us):
        for u in us:
            torch.manual_seed(900 + u)                                            # the hooks' torch.randn / Categorical draws
            np.random.seed(950 + u)                                               # REDQ's critic subset
            stats = algo.update(buf, 32)
        return dataclasses.asdict(stats)

    a, buf_a = _ac_resume_algo(which)
    stats_a = run(a, buf_a, range(4))
    b, buf_b = _ac_resume_algo(which)
    run(b, buf_b, range(2))
    first = b._hip_engine
    b._hip_invalidate()
    stats_b = run(b, buf_b, range(2, 4))
    assert first is not None and b._hip_engine is not first
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(pa) == list(pb) and any("_old" in k for k in pa) and ("alpha._log_alpha" in pa) == (which not in ("td3", "ddpg"))
    worst = {k: float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa if not torch.equal(pa[k], pb[k])}
    print(which, "parameters that differ:", worst, "statistics:", stats_a, stats_b)
    oa, ob = _ac_resume_optimizers(a), _ac_resume_optimizers(b)
    assert len(oa) == len(ob) == {"td3": 3, "ddpg": 2, "redq": 3}.get(which, 4)
    state = []
    for i, (x, y) in enumerate(zip(oa, ob)):
        for j, (p, q) in enumerate(zip(x.param_groups[0]["params"], y.param_groups[0]["params"])):
            sx, sy = x.state[p], y.state[q]
            assert set(sx) == set(sy) == {"step", "exp_avg", "exp_avg_sq"}, (i, j)
            state += [(i, j, k, float(sx[k]) if k == "step" else None, float(sy[k]) if k == "step" else None)
                      for k in sx if not torch.equal(sx[k].cpu(), sy[k].cpu())]
    print(which, "optimizer state entries that differ:", state)
    assert not worst and not state and stats_a == stats_b


# ------------------------------------------------------------------------------------ a rebuilt engine continues (on-policy bodies)
_ON_RESUME_ROUTES = ["ppo_fused", "ppo_net", "a2c_rmsprop", "ppo_discrete", "ppo_cnn", "npg_two_width", "trpo_net", "reinforce_legacy",
                     "reinforce_net_ln"]


def _on_resume_algo(route):
    """-> (one on-policy Hip* class over the stand-ins on its engine route, fill(buf-or-None, u) -> the buffer holding rollout u):
    4 environments x 32 steps with a few terminals and truncations, return scaling / standardisation on so that `ret_rms` moves."""
    from torch.distributions import Categorical

    from tianshou_amd import integration as I

    E, T, obs_dim, act_dim = 4, 32, 11, 3
    torch.manual_seed(81)
    gauss = lambda h, act, **kw: SI.ContinuousActorProbabilistic(SI.Net(obs_dim, h, act, **kw), act_dim, unbounded=True)   # noqa: E731
    value = lambda h, act: SI.ContinuousCritic(SI.Net(obs_dim, h, act))                                                    # noqa: E731
    frame, n_act = None, 0
    if route in ("ppo_fused", "ppo_net", "a2c_rmsprop"):
        h, act = ([48, 40], nn.ReLU) if route == "ppo_net" else ([64, 64], nn.Tanh)
        kw = dict(optim=(torch.optim.RMSprop, dict(eps=1e-5, alpha=0.99))) if route == "a2c_rmsprop" else dict(eps_clip=0.2, value_clip=True)
        algo = I.make_hip_ppo("a2c" if route == "a2c_rmsprop" else "ppo", ref=SI)(
            policy=SI.Policy(gauss(h, act)), critic=value(h, act), device="cuda", permutations="host", lr=3e-4, vf_coef=0.25,
            max_grad_norm=0.5, return_scaling=True, **kw)
        assert algo._hip_dims[3] == ("net" if route == "ppo_net" else "fused")
    elif route == "ppo_discrete":
        obs_dim, n_act = 4, 2
        trunk = SI.Net(obs_dim, [32, 32], nn.ReLU)
        algo = I.make_hip_ppo_discrete("ppo", ref=SI)(
            policy=SI.Policy(SI.DiscreteActor(trunk, n_act, softmax_output=True), dist_fn=Categorical), critic=SI.DiscreteCritic(trunk),
            device="cuda", lr=3e-4, eps_clip=0.2, value_clip=True, max_grad_norm=0.5, return_scaling=True)
    elif route == "ppo_cnn":
        frame, n_act = (4, 44, 36), 5                                             # (test_hip_ppo_cnn_hooks_against_oracle's frames)
        trunk = SI.DQNetFeatures(*frame)
        algo = I.make_hip_ppo_cnn("ppo", ref=SI)(
            policy=SI.Policy(SI.DiscreteActor(trunk, n_act, softmax_output=False)), critic=SI.DiscreteCritic(trunk), device="cuda",
            lr=2.5e-4, eps_clip=0.1, value_clip=True, vf_coef=0.25, max_grad_norm=0.5, return_scaling=True)
    elif route in ("npg_two_width", "trpo_net"):
        h, act = ([48, 40], nn.Tanh) if route == "npg_two_width" else ([64, 48, 32], nn.ReLU)
        make = I.make_hip_npg if route == "npg_two_width" else I.make_hip_trpo
        algo = make(ref=SI)(policy=SI.Policy(gauss(h, act)), critic=value(h, act), device="cuda", lr=1e-3, optim_critic_iters=3,
                            return_scaling=True)
        assert algo._hip_two == (route == "npg_two_width")
    else:
        ln = dict(norm_layer=nn.LayerNorm, norm_args=dict(eps=1e-5)) if route == "reinforce_net_ln" else {}
        h, act = ([48, 40], nn.ReLU) if ln else ([64, 64], nn.Tanh)
        algo = I.make_hip_reinforce(ref=SI)(policy=SI.Policy(gauss(h, act, **ln)), lr=1e-3, gamma=0.97, return_standardization=True,
                                            max_grad_norm=0.7, device="cuda")
        assert algo._hip_kind == ("net" if ln else "legacy")
    algo = algo.to("cuda")
    algo.policy.is_within_training_step = True

    def fill(buf, u):
        rng = np.random.default_rng(820 + u)
        if buf is None and frame is not None:
            buf = SI.VectorReplayBuffer(E * T, E, obs_shape=frame[1:], act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64, stack_num=frame[0])
        elif buf is None:
            buf = SI.VectorReplayBuffer(E * T, E, obs_shape=(obs_dim,), act_shape=() if n_act else (act_dim,),
                                        act_dtype=np.int64 if n_act else np.float32)
        buf.reset()
        draw = (lambda: rng.integers(0, 4, (E, *frame[1:])).astype(np.uint8)) if frame else (lambda: rng.normal(size=(E, obs_dim)).astype(np.float32))
        obs = draw()
        for _ in range(T):
            term, nxt = rng.random(E) < 0.05, draw()
            buf.add(SI.Batch(obs=obs, act=rng.integers(0, n_act, E) if n_act else rng.normal(size=(E, act_dim)).astype(np.float32),
                             rew=rng.normal(size=E).astype(np.float32), terminated=term, truncated=(rng.random(E) < 0.03) & ~term,
                             obs_next=nxt))
            obs = nxt
        return buf

    return algo, fill


def _on_resume_state(algo, stats):
    """Everything a run ends with, by name: parameters, optimizer state (after `state_dict()`: HipPPO's moves there), ret_rms,
    the last update's statistics."""
    import dataclasses

    algo.state_dict()
    out = {f"param {k}": p.detach().cpu() for k, p in algo.named_parameters()}
    for i, o in enumerate(algo._optimizers):
        for j, p in enumerate(o._optim.param_groups[0]["params"]):
            for k, v in o._optim.state.get(p, {}).items():
                out[f"optim {i}.{j} {k}"] = torch.as_tensor(v).detach().cpu()
    rms = getattr(algo, "discounted_return_computation", algo).ret_rms
    out["ret_rms"] = torch.tensor([rms.mean, rms.var], dtype=torch.float64)
    out["ret_rms count"] = torch.tensor(float(rms.count), dtype=torch.float64)
    for k, v in dataclasses.asdict(stats).items():
        if k != "train_time":
            out[f"stats {k}"] = torch.tensor(list(v.values()) if isinstance(v, dict) else [v], dtype=torch.float64)
    return out


@pytest.mark.parametrize("route", _ON_RESUME_ROUTES)
def test_hip_on_policy_rebuilt_engine_continues_where_the_last_one_stopped(route):
    """The torch<->engine state path of the on-policy bodies (`_on_load` / `_on_write_back`), both directions, on the real engines:
    run A makes three updates on three rollouts; run B, seeded alike (`np.random.seed` before each update draws the same host
    shuffles), makes one, drops its engine (`_hip_invalidate()`: the next update builds a new one from the torch modules and
    torch.optim) and makes two more.  Write-back and load are plain fp32 copies, so B ends bit for bit where A does: every
    parameter, every optimizer state tensor and step, `ret_rms`, the last update's statistics.
    `_hip_invalidate()` is what `load_state_dict` calls after it has replaced the optimizer state, so it drops the engine without
    flushing; HipPPO / HipA2C hand their optimizer state to torch.optim when somebody reads it, and B reads it (`state_dict()`) before
    it drops the engine -- without that read the first update's four Adam steps are discarded by design, on the commit before
    this state path as well (its B ended with step 8 against A's 12 on the three HipPPO routes).
    Whether each engine is itself run-to-run deterministic is measured, not assumed: A runs a second time (A').  On the commit
    before this state path all nine routes repeated themselves bit for bit (the conv path and the gradient-slab reductions
    included), so none has a tolerance: A' must equal A, and then B must equal A, bitwise.  A route that stops repeating itself
    fails here and needs its own measured bound (4 x the largest |A - A'|, step counts and `ret_rms.count` still equal)."""
    def run(invalidate_after=None):
        algo, fill = _on_resume_algo(route)
        buf, engines = None, []
        for u in range(3):
            buf = fill(buf, u)
            np.random.seed(870 + u)
            stats = algo.update(buf, 64, 2)
            engines.append(algo._hip_engine)
            if u == invalidate_after:
                algo.state_dict()
                algo._hip_invalidate()
        return _on_resume_state(algo, stats), engines

    diff = lambda x, y: {k: float((x[k].double() - y[k].double()).abs().max()) for k in x if not torch.equal(x[k], y[k])}   # noqa: E731
    (a, ea), (a2, _), (b, eb) = run(), run(), run(invalidate_after=0)
    assert ea[0] is ea[1] is ea[2] and eb[0] is not None and eb[1] is not eb[0] and eb[1] is eb[2]        # B built a new engine object
    assert list(a) == list(a2) == list(b) and any(k.endswith(" step") for k in a) and any(k.startswith("param ") for k in a)
    spread, moved = diff(a, a2), diff(a, b)
    print(route, "entries that differ between two identical runs (A, A'):", spread)
    print(route, "entries that differ between A and the run with a rebuilt engine (B):", moved)
    assert float(a["ret_rms count"]) > 0 and all(float(a[k]) >= 3 for k in a if k.endswith(" step"))
    assert not spread, "two identical runs differ: this route needs a measured bound"
    assert not moved
