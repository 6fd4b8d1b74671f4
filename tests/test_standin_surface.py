"""CPU, only where the reference is mounted: the stand-ins of tests/standin.py (which let the GPU box drive the Hip*
hook bodies without the reference package) expose the same surface as the reference classes they replace - state_dict
keys and shapes, hyper-parameter attribute names, optimizer wrapper, buffer bookkeeping after identical `add()`
sequences - and the production subclass built over the REAL reference reads them the same way."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin as SI

pytestmark = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")


def _real_ppo(**kw):
    ref_shim.install()
    import gymnasium as gym
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.ppo import PPO
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                         action_shape=(6,), unbounded=True)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
    policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=True,
                                      action_bound_method="clip",
                                      action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    return PPO(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), **kw)


def _standin_ppo(**kw):
    actor = SI.ContinuousActorProbabilistic(SI.Net(17, [64, 64], nn.Tanh), 6, unbounded=True)
    critic = SI.ContinuousCritic(SI.Net(17, [64, 64], nn.Tanh))
    return SI.PPO(policy=SI.Policy(actor), critic=critic, lr=3e-4, **kw)


def test_bounded_actor_and_rmsprop_standins_have_the_reference_surface():
    """Round 6: the stand-ins of the reference's DEFAULT actor (unbounded=False, max_action) and of an Algorithm whose
    optimizer comes from RMSpropOptimizerFactory (optim.py:113-140) expose what ppo_config_from / optimizer_fields read."""
    ref_shim.install()
    import gymnasium as gym
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import RMSpropOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_ppo, ppo_config_from

    def real_nets():
        a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                         action_shape=(6,), max_action=1.7)
        return a, ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))

    ra, rc = real_nets()
    fa = SI.ContinuousActorProbabilistic(SI.Net(17, [64, 64], nn.Tanh), 6, unbounded=False, max_action=1.7)
    assert (ra._unbounded, ra.max_action) == (fa._unbounded, fa.max_action) == (False, 1.7)
    assert list(ra.state_dict().keys()) == list(fa.state_dict().keys())
    ru = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                      action_shape=(6,), unbounded=True, max_action=1.7)          # discarded (continuous.py:199-201)
    assert ru.max_action == SI.ContinuousActorProbabilistic(SI.Net(17, [64, 64], nn.Tanh), 6, unbounded=True, max_action=1.7).max_action == 1.0
    policy = ProbabilisticActorPolicy(actor=ra, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=False,
                                      action_bound_method=None, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    kw = dict(vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, gae_lambda=0.95, gamma=0.99, return_scaling=True)
    real = make_hip_ppo("a2c")(policy=policy, critic=rc, optim=RMSpropOptimizerFactory(lr=7e-4, eps=1e-5, alpha=0.99),
                               device="cpu", **kw)
    fake = make_hip_ppo("a2c", ref=SI)(policy=SI.Policy(fa), critic=SI.ContinuousCritic(SI.Net(17, [64, 64], nn.Tanh)), lr=7e-4,
                                       optim=(torch.optim.RMSprop, dict(eps=1e-5, alpha=0.99)), device="cpu", **kw)
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.RMSprop
    g_r, g_f = real.optim._optim.param_groups[0], fake.optim._optim.param_groups[0]
    for k in ("lr", "alpha", "eps", "weight_decay", "momentum", "centered"):
        assert g_r[k] == g_f[k], k
    assert ppo_config_from(real) == ppo_config_from(fake)
    assert ppo_config_from(real).max_action == 1.7 and ppo_config_from(real).optimizer == "rmsprop"
    assert real._hip_dims == fake._hip_dims == (17, 6, 64, "fused")


def test_ppo_standin_has_the_reference_surface():
    kw = dict(eps_clip=0.2, dual_clip=None, value_clip=True, advantage_normalization=False, recompute_advantage=False,
              vf_coef=0.25, ent_coef=0.0, max_grad_norm=0.5, gae_lambda=0.95, gamma=0.99, return_scaling=True)
    real, fake = _real_ppo(**kw), _standin_ppo(**kw)
    for a, b in ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("_unbounded", "_c_sigma", "max_action"):
        assert getattr(real.policy.actor, name) == getattr(fake.policy.actor, name), name
    # every attribute ppo_config_from() / the hooks read, with equal values
    for name in ("gamma", "gae_lambda", "eps_clip", "dual_clip", "value_clip", "advantage_normalization", "recompute_adv",
                 "vf_coef", "ent_coef", "return_scaling", "max_batchsize"):
        assert getattr(real, name) == getattr(fake, name), name
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm == 0.5
    g_r, g_f = real.optim._optim.param_groups[0], fake.optim._optim.param_groups[0]
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert (g_r["lr"], g_r["betas"], g_r["eps"], g_r["weight_decay"]) == (g_f["lr"], g_f["betas"], g_f["eps"], g_f["weight_decay"])
    assert (real.ret_rms.mean, real.ret_rms.var, real.ret_rms.count) == (fake.ret_rms.mean, fake.ret_rms.var, fake.ret_rms.count)
    assert real.lr_schedulers == fake.lr_schedulers == [] and len(real._optimizers) == len(fake._optimizers) == 1
    assert real.policy.is_within_training_step is False and fake.policy.is_within_training_step is False
    sd_r, sd_f = real.state_dict(), fake.state_dict()
    assert "_optimizers" in sd_r and "_optimizers" in sd_f
    # the optimizer steps the same parameters in the same order (what adam_state / store_adam_state index by)
    n_r = [p.numel() for p in real.optim._optim.param_groups[0]["params"]]
    n_f = [p.numel() for p in fake.optim._optim.param_groups[0]["params"]]
    assert n_r == n_f
    from tianshou_amd.integration import ppo_config_from

    assert ppo_config_from(real) == ppo_config_from(fake)


def test_buffer_standin_keeps_the_reference_bookkeeping():
    ref_shim.install()
    from tianshou.data import Batch, VectorReplayBuffer

    rng = np.random.default_rng(0)
    real = VectorReplayBuffer(30, 3)
    fake = SI.VectorReplayBuffer(30, 3, obs_shape=(5,), act_shape=(2,))

    def step(ids=None):
        k = 3 if ids is None else len(ids)
        term = rng.random(k) < 0.2
        d = dict(obs=rng.normal(size=(k, 5)).astype(np.float32), act=rng.normal(size=(k, 2)).astype(np.float32),
                 rew=rng.normal(size=k), terminated=term, truncated=(rng.random(k) < 0.1) & ~term,
                 obs_next=rng.normal(size=(k, 5)).astype(np.float32))
        real.add(Batch(**d), buffer_ids=ids)
        fake.add(SI.Batch(**d), buffer_ids=ids)

    def same():
        assert len(real) == len(fake) and real.maxsize == fake.maxsize
        assert np.array_equal(real._extend_offset, fake._extend_offset)
        assert np.array_equal(real._lengths, fake._lengths)
        assert np.array_equal(real.last_index, fake.last_index)
        assert [b._insertion_idx for b in real.buffers] == [b._insertion_idx for b in fake.buffers]
        assert [len(b) for b in real.buffers] == [len(b) for b in fake.buffers]
        assert np.array_equal(real.unfinished_index(), fake.unfinished_index())
        assert np.array_equal(real.sample_indices(0), fake.sample_indices(0))
        for key in ("obs", "act", "rew", "terminated", "truncated", "done", "obs_next"):
            assert np.array_equal(np.asarray(getattr(real, key)), getattr(fake, key)), key
            assert np.asarray(getattr(real, key)).dtype == getattr(fake, key).dtype, key
        assert set(fake._meta.get_keys()) <= set(real._meta.get_keys())

    for _ in range(4):
        step()
    same()
    for ids in ([0, 2], [1], [1], [2, 0], None, None):
        for _ in range(3):
            step(ids)
        same()
    for _ in range(9):                    # wrap every ring
        step()
    same()
    real.reset()
    fake.reset()
    step()
    same()
    b, idx = fake.sample(0)
    rb, ridx = real.sample(0)
    assert np.array_equal(idx, ridx) and np.array_equal(b.obs, rb.obs) and np.array_equal(b.rew, rb.rew)


def test_real_subclass_and_standin_subclass_are_the_same_hook_code():
    """make_hip_ppo() over the reference and over the stand-ins yields classes whose hook functions come from the same
    source lines (the `ref=` argument only swaps the base / statistics classes)."""
    ref_shim.install()
    from tianshou_amd.integration import make_hip_ppo

    A, B = make_hip_ppo("ppo"), make_hip_ppo("ppo", ref=SI)
    for name in ("update", "_preprocess_batch", "_update_with_batch", "_engine", "_hip_write_back", "_hip_flush"):
        fa, fb = getattr(A, name), getattr(B, name)
        assert fa.__code__.co_code == fb.__code__.co_code and fa.__code__.co_firstlineno == fb.__code__.co_firstlineno, name


def test_sac_standin_has_the_reference_surface():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.sac import SAC, AutoAlpha, SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[256, 256]), action_shape=(3,),
                                         unbounded=True, conditioned_sigma=True)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[256, 256], concat=True))  # noqa: E731
    real = SAC(policy=SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,))),
               policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(), critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=mk(),
               critic2_optim=AdamOptimizerFactory(lr=1e-3), tau=0.005, gamma=0.99,
               alpha=AutoAlpha(-3.0, 0.0, AdamOptimizerFactory(lr=3e-4)))
    f_actor = SI.ContinuousActorProbabilistic(SI.Net(11, [256, 256], nn.ReLU), 3, unbounded=True, conditioned_sigma=True)
    fake = SI.SAC(policy=SI.Policy(f_actor), critic=SI.ContinuousCritic(SI.Net(14, [256, 256], nn.ReLU)),
                  critic2=SI.ContinuousCritic(SI.Net(14, [256, 256], nn.ReLU)), lr=1e-3, tau=0.005, gamma=0.99,
                  alpha=SI.AutoAlpha(-3.0, 0.0, 3e-4))
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.critic2, fake.critic2),
             (real.critic_old.module, fake.critic_old.module), (real.critic2_old.module, fake.critic2_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("tau", "gamma", "n_step_return_horizon"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert [p.numel() for p in r._optim.param_groups[0]["params"]] == [p.numel() for p in f._optim.param_groups[0]["params"]]
    for name in ("_target_entropy", "_log_alpha", "_optim", "value"):
        assert hasattr(real.alpha, name) and hasattr(fake.alpha, name), name
    assert float(real.alpha._log_alpha) == float(fake.alpha._log_alpha) and real.alpha._target_entropy == fake.alpha._target_entropy
    assert type(real.alpha._optim) is type(fake.alpha._optim)
    from tianshou_amd.integration import make_hip_sac

    A, B = make_hip_sac(), make_hip_sac(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_dqn_standin_has_the_reference_surface():
    """DQN / DQNet / PrioritizedVectorReplayBuffer stand-ins against the real classes: state_dict keys and shapes, the
    hyper-parameter attribute names HipDQN reads, the lagged network wrapper, the optimizer, and PER weights after the
    same add / update_weight sequence."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou.env.atari.atari_network import DQNet

    real = DQN(policy=DiscreteQLearningPolicy(model=DQNet(c=4, h=44, w=36, action_shape=3), action_space=gym.spaces.Discrete(3)),
               optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97, n_step_return_horizon=3, target_update_freq=5, is_double=True,
               huber_loss_delta=1.0)
    fake = SI.DQN(policy=SI.DiscreteQLearningPolicy(SI.DQNet(4, 44, 36, 3)), lr=1e-4, gamma=0.97, n_step_return_horizon=3,
                  target_update_freq=5, is_double=True, huber_loss_delta=1.0)
    for a, b in ((real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("gamma", "n_step", "target_update_freq", "is_double", "huber_loss_delta", "_iter"):
        assert getattr(real, name) == getattr(fake, name), name
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    assert [p.numel() for p in real.optim._optim.param_groups[0]["params"]] == \
        [p.numel() for p in fake.optim._optim.param_groups[0]["params"]]

    rb = PrioritizedVectorReplayBuffer(24, 2, alpha=0.6, beta=0.4)
    fb = SI.PrioritizedVectorReplayBuffer(24, 2, obs_shape=(3,), act_shape=(), act_dtype=np.int64, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(0)
    for _ in range(9):
        kw = dict(obs=rng.normal(size=(2, 3)).astype(np.float32), act=rng.integers(0, 3, 2), rew=rng.normal(size=2),
                  terminated=rng.random(2) < 0.2, truncated=np.zeros(2, bool), obs_next=rng.normal(size=(2, 3)).astype(np.float32))
        rb.add(Batch(**kw))
        fb.add(SI.Batch(**kw))
    idx = np.array([0, 3, 13, 14])
    td = np.array([0.5, -2.0, 0.01, 3.0])
    rb.update_weight(idx, td)
    fb.update_weight(idx, td)
    assert np.allclose(np.asarray(rb.weight[idx]), fb.prio[idx]) and rb._max_prio == fb._max_prio and rb._min_prio == fb._min_prio
    assert np.allclose(rb.get_weight(idx) / 1.0, (fb.prio[idx] / fb._min_prio) ** (-0.4))
    from tianshou_amd.integration import make_hip_dqn

    A, B = make_hip_dqn(), make_hip_dqn(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_ppo_cnn_standin_has_the_reference_surface():
    """The Atari actor-critic stand-ins (DQNetFeatures / DiscreteActor / DiscreteCritic) against the real modules:
    state_dict keys and shapes of actor and critic, the shared trunk, `softmax_output`; the hook bodies of HipPPOCnn are
    the same code objects over either namespace."""
    ref_shim.install()
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

    net = DQNet(c=4, h=44, w=36, action_shape=5, features_only=True, output_dim_added_layer=512)
    ra, rc = DiscreteActor(preprocess_net=net, action_shape=5, softmax_output=False), DiscreteCritic(preprocess_net=net)
    trunk = SI.DQNetFeatures(4, 44, 36)
    fa, fc = SI.DiscreteActor(trunk, 5, softmax_output=False), SI.DiscreteCritic(trunk)
    for a, b in ((ra, fa), (rc, fc)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert ra.softmax_output is fa.softmax_output is False and fa.preprocess is fc.preprocess
    from tianshou_amd import ppo_cnn as PC
    from tianshou_amd.integration import make_hip_ppo_cnn

    assert list(fa.state_dict().keys()) == PC.TRUNK_KEYS + PC.HEAD_KEYS
    A, B = make_hip_ppo_cnn("ppo"), make_hip_ppo_cnn("ppo", ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_hip_params"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_qrdqn_standin_has_the_reference_surface():
    """QRDQN / QRDQNet stand-ins against the real classes: state_dict keys and shapes, the attribute names HipQRDQN reads
    (`num_quantiles` included), the lagged wrapper; and the hook bodies are the same code objects over either namespace."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.qrdqn import QRDQN, QRDQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import QRDQNet

    real = QRDQN(policy=QRDQNPolicy(model=QRDQNet(c=4, h=44, w=36, action_shape=3, num_quantiles=16),
                                    action_space=gym.spaces.Discrete(3)),
                 optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97, num_quantiles=16, n_step_return_horizon=2, target_update_freq=2)
    fake = SI.QRDQN(policy=SI.DiscreteQLearningPolicy(SI.QRDQNet(4, 44, 36, 3, 16)), lr=1e-4, gamma=0.97, num_quantiles=16,
                    n_step_return_horizon=2, target_update_freq=2)
    for a, b in ((real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("gamma", "n_step", "target_update_freq", "num_quantiles", "_iter"):
        assert getattr(real, name) == getattr(fake, name), name
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    from tianshou.algorithm.modelfree.reinforce import LossSequenceTrainingStats, SimpleLossTrainingStats

    assert SimpleLossTrainingStats(loss=1.5).loss == SI.SimpleLossTrainingStats(loss=1.5).loss
    assert hasattr(LossSequenceTrainingStats, "__init__") and SI.LossSequenceTrainingStats(loss=2.0).loss == 2.0
    from tianshou_amd.integration import make_hip_qrdqn

    A, B = make_hip_qrdqn(), make_hip_qrdqn(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_n_atoms"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_discrete_sac_standin_has_the_reference_surface():
    """DiscreteSAC over Net-based DiscreteActor / DiscreteCritic(last_size = n_act) (test/discrete/test_discrete_sac.py:88-97)
    against the real classes: state_dict keys and shapes of the five networks, hyper-parameter attributes, optimizers, the
    alpha object; the hook bodies are the same code objects over either namespace."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.discrete_sac import DiscreteSAC, DiscreteSACPolicy, DiscreteSACTrainingStats
    from tianshou.algorithm.modelfree.sac import AutoAlpha
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

    actor = DiscreteActor(preprocess_net=Net(state_shape=(19,), hidden_sizes=[128, 128]), action_shape=7, softmax_output=False)
    mk = lambda: DiscreteCritic(preprocess_net=Net(state_shape=(19,), hidden_sizes=[128, 128]), last_size=7)  # noqa: E731
    real = DiscreteSAC(policy=DiscreteSACPolicy(actor=actor, action_space=gym.spaces.Discrete(7)),
                       policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(), critic_optim=AdamOptimizerFactory(lr=1e-3),
                       critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3), tau=0.02, gamma=0.96,
                       alpha=AutoAlpha(1.9, -0.4, AdamOptimizerFactory(lr=3e-4)))
    f_actor = SI.DiscreteActor(SI.Net(19, [128, 128], nn.ReLU), 7, softmax_output=False)
    fake = SI.DiscreteSAC(policy=SI.Policy(f_actor), critic=SI.DiscreteCritic(SI.Net(19, [128, 128], nn.ReLU), last_size=7),
                          critic2=SI.DiscreteCritic(SI.Net(19, [128, 128], nn.ReLU), last_size=7), lr=1e-3, tau=0.02, gamma=0.96,
                          alpha=SI.AutoAlpha(1.9, -0.4, 3e-4))
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.critic2, fake.critic2),
             (real.critic_old.module, fake.critic_old.module), (real.critic2_old.module, fake.critic2_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert real.policy.actor.softmax_output is fake.policy.actor.softmax_output is False
    for name in ("tau", "gamma", "n_step_return_horizon"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert [p.numel() for p in r._optim.param_groups[0]["params"]] == [p.numel() for p in f._optim.param_groups[0]["params"]]
    assert float(real.alpha._log_alpha) == float(fake.alpha._log_alpha) and real.alpha._target_entropy == fake.alpha._target_entropy
    kw = dict(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0, alpha=0.5, alpha_loss=None)
    a, b = DiscreteSACTrainingStats(**kw), SI.DiscreteSACTrainingStats(**kw)
    assert all(getattr(a, k) == getattr(b, k) for k in kw)
    from tianshou_amd.integration import make_hip_discrete_sac

    A, B = make_hip_discrete_sac(), make_hip_discrete_sac(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_draw", "_hip_parts"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_c51_standin_has_the_reference_surface():
    """C51 / C51Policy / C51Net stand-ins against the real classes: state_dict keys and shapes (the policy's `support`
    included), the attributes HipC51 reads (`num_atoms`, `v_min`, `v_max`), the optimizer's parameter list, the lagged wrapper;
    and the hook bodies are the same code objects over either namespace."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.c51 import C51, C51Policy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import C51Net

    real = C51(policy=C51Policy(model=C51Net(c=4, h=44, w=36, action_shape=[3], num_atoms=21),
                                action_space=gym.spaces.Discrete(3), num_atoms=21, v_min=-4.0, v_max=4.0),
               optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97, n_step_return_horizon=2, target_update_freq=2)
    fake = SI.C51(policy=SI.C51Policy(SI.C51Net(4, 44, 36, 3, 21), num_atoms=21, v_min=-4.0, v_max=4.0), lr=1e-4, gamma=0.97,
                  n_step_return_horizon=2, target_update_freq=2)
    for a, b in ((real.policy, fake.policy), (real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert torch.equal(real.policy.support, fake.policy.support) and not fake.policy.support.requires_grad
    for name in ("gamma", "n_step", "target_update_freq", "delta_z", "_iter"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("num_atoms", "v_min", "v_max"):
        assert getattr(real.policy, name) == getattr(fake.policy, name), name
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    shapes = lambda o: [tuple(p.shape) for g in o._optim.param_groups for p in g["params"]]   # noqa: E731
    assert shapes(real.optim) == shapes(fake.optim)
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    from tianshou_amd.integration import make_hip_c51

    A, B = make_hip_c51(), make_hip_c51(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_n_atoms"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_td3_standin_has_the_reference_surface():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.ddpg import ContinuousDeterministicPolicy
    from tianshou.algorithm.modelfree.td3 import TD3
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousCritic

    actor = ContinuousActorDeterministic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[128, 128]), action_shape=(3,),
                                         max_action=1.5)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[128, 128], concat=True))  # noqa: E731
    real = TD3(policy=ContinuousDeterministicPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.5, high=1.5, shape=(3,))),
               policy_optim=AdamOptimizerFactory(lr=3e-4), critic=mk(), critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=mk(),
               critic2_optim=AdamOptimizerFactory(lr=1e-3), tau=0.01, gamma=0.98, policy_noise=0.2, update_actor_freq=2,
               noise_clip=0.5)
    f_actor = SI.ContinuousActorDeterministic(SI.Net(11, [128, 128], nn.ReLU), 3, max_action=1.5)
    fake = SI.TD3(policy=SI.Policy(f_actor), critic=SI.ContinuousCritic(SI.Net(14, [128, 128], nn.ReLU)),
                  critic2=SI.ContinuousCritic(SI.Net(14, [128, 128], nn.ReLU)), lr=3e-4, critic_lr=1e-3, tau=0.01, gamma=0.98,
                  policy_noise=0.2, update_actor_freq=2, noise_clip=0.5)
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.critic2, fake.critic2),
             (real.actor_old.module, fake.actor_old.module), (real.critic_old.module, fake.critic_old.module),
             (real.critic2_old.module, fake.critic2_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("tau", "gamma", "n_step_return_horizon", "policy_noise", "update_actor_freq", "noise_clip", "_cnt", "_last"):
        assert getattr(real, name) == getattr(fake, name), name
    assert float(real.policy.actor.max_action) == float(fake.policy.actor.max_action)
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert r._optim.param_groups[0]["lr"] == f._optim.param_groups[0]["lr"]
    from tianshou_amd.integration import make_hip_td3

    A, B = make_hip_td3(), make_hip_td3(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_ddpg_standin_has_the_reference_surface():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.ddpg import DDPG, ContinuousDeterministicPolicy, DDPGTrainingStats
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousCritic

    actor = ContinuousActorDeterministic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[64, 64]), action_shape=(3,),
                                         max_action=1.5)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[64, 64], concat=True))
    real = DDPG(policy=ContinuousDeterministicPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.5, high=1.5, shape=(3,))),
                policy_optim=AdamOptimizerFactory(lr=3e-4), critic=critic, critic_optim=AdamOptimizerFactory(lr=1e-3), tau=0.02,
                gamma=0.95, n_step_return_horizon=3)
    f_actor = SI.ContinuousActorDeterministic(SI.Net(11, [64, 64], nn.ReLU), 3, max_action=1.5)
    fake = SI.DDPG(policy=SI.Policy(f_actor), critic=SI.ContinuousCritic(SI.Net(14, [64, 64], nn.ReLU)), lr=3e-4, critic_lr=1e-3,
                   tau=0.02, gamma=0.95, n_step_return_horizon=3)
    pairs = ((real.policy.actor, fake.policy.actor), (real.critic, fake.critic), (real.actor_old.module, fake.actor_old.module),
             (real.critic_old.module, fake.critic_old.module))
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for name in ("tau", "gamma", "n_step_return_horizon"):
        assert getattr(real, name) == getattr(fake, name), name
    assert float(real.policy.actor.max_action) == float(fake.policy.actor.max_action)
    for name in ("policy_optim", "critic_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert r._optim.param_groups[0]["lr"] == f._optim.param_groups[0]["lr"]
    a, b = DDPGTrainingStats(actor_loss=1.0, critic_loss=2.0), SI.DDPGTrainingStats(actor_loss=1.0, critic_loss=2.0)
    assert (a.actor_loss, a.critic_loss) == (b.actor_loss, b.critic_loss)
    from tianshou_amd.integration import make_hip_ddpg

    A, B = make_hip_ddpg(), make_hip_ddpg(ref=SI)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_ppo_discrete_standin_has_the_reference_surface():
    """The CartPole-shape actor-critic (test/discrete/test_ppo_discrete.py:88-127) over the stand-ins against the real modules
    and the real ProbabilisticActorPolicy: state_dict keys and shapes, the shared trunk, `softmax_output`, `policy.dist_fn`
    (and the identity of the default logits dist_fn the hook compares against); the hook bodies are the same code objects."""
    ref_shim.install()
    import gymnasium as gym
    from torch.distributions import Categorical

    from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy, ProbabilisticActorPolicy, dist_fn_categorical_from_logits
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

    net = Net(state_shape=(4,), hidden_sizes=[64, 64])
    ra, rc = DiscreteActor(preprocess_net=net, action_shape=2), DiscreteCritic(preprocess_net=net)
    trunk = SI.Net(4, [64, 64], nn.ReLU)
    fa, fc = SI.DiscreteActor(trunk, 2), SI.DiscreteCritic(trunk)
    for a, b in ((ra, fa), (rc, fc)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert ra.softmax_output is fa.softmax_output is True and fa.preprocess is fc.preprocess
    real = ProbabilisticActorPolicy(actor=ra, dist_fn=Categorical, action_space=gym.spaces.Discrete(2), action_scaling=False)
    fake = SI.Policy(fa, dist_fn=Categorical)
    assert real.dist_fn is fake.dist_fn is Categorical
    default = DiscreteActorPolicy(actor=DiscreteActor(preprocess_net=net, action_shape=2, softmax_output=False),
                                  action_space=gym.spaces.Discrete(2))
    assert default.dist_fn is dist_fn_categorical_from_logits
    lg = torch.randn(5, 2)
    assert torch.equal(dist_fn_categorical_from_logits(lg).probs, SI.dist_fn_categorical_from_logits(lg).probs)
    from tianshou_amd import ppo_discrete as PD
    from tianshou_amd.integration import make_hip_ppo_discrete

    assert list(fa.state_dict().keys()) == PD.TRUNK_KEYS + PD.HEAD_KEYS
    A, B = make_hip_ppo_discrete("ppo"), make_hip_ppo_discrete("ppo", ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine", "_hip_params"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def _real_mujoco_nets():
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                         action_shape=(6,), unbounded=True)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
    return actor, critic


def _fake_mujoco_nets():
    return (SI.ContinuousActorProbabilistic(SI.Net(17, [64, 64], nn.Tanh), 6, unbounded=True),
            SI.ContinuousCritic(SI.Net(17, [64, 64], nn.Tanh)))


def _same_state_dicts(pairs):
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]


@pytest.mark.parametrize("which", ["npg", "trpo"])
def test_natural_gradient_standins_have_the_reference_surface(which):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.npg import NPG
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.modelfree.trpo import TRPO
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from torch.distributions import Independent, Normal

    ra, rc = _real_mujoco_nets()
    fa, fc = _fake_mujoco_nets()
    pol = ProbabilisticActorPolicy(actor=ra, dist_fn=lambda loc_scale: Independent(Normal(*loc_scale), 1),
                                   action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    kw = dict(optim_critic_iters=3, advantage_normalization=True, gae_lambda=0.9, gamma=0.98, return_scaling=True)
    if which == "npg":
        real = NPG(policy=pol, critic=rc, optim=AdamOptimizerFactory(lr=1e-3), trust_region_size=0.1, **kw)
        fake = SI.NPG(policy=SI.Policy(fa), critic=fc, lr=1e-3, trust_region_size=0.1, **kw)
        names = ("trust_region_size",)
    else:
        real = TRPO(policy=pol, critic=rc, optim=AdamOptimizerFactory(lr=1e-3), max_kl=0.02, backtrack_coeff=0.7, max_backtracks=8, **kw)
        fake = SI.TRPO(policy=SI.Policy(fa), critic=fc, lr=1e-3, max_kl=0.02, backtrack_coeff=0.7, max_backtracks=8, **kw)
        names = ("max_kl", "backtrack_coeff", "max_backtracks")
    _same_state_dicts(((real.policy.actor, fake.policy.actor), (real.critic, fake.critic)))
    for name in names + ("optim_critic_iters", "advantage_normalization", "gae_lambda", "gamma", "return_scaling", "_damping"):
        assert getattr(real, name) == getattr(fake, name), name
    assert (real.ret_rms.mean, real.ret_rms.var, real.ret_rms.count) == (fake.ret_rms.mean, fake.ret_rms.var, fake.ret_rms.count)
    shapes = lambda o: [tuple(p.shape) for g in o._optim.param_groups for p in g["params"]]   # noqa: E731
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam and shapes(real.optim) == shapes(fake.optim)
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    from tianshou_amd.integration import make_hip_npg, make_hip_trpo

    mk = make_hip_npg if which == "npg" else make_hip_trpo
    A, B = mk(), mk(ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_reinforce_standin_has_the_reference_surface():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy, Reinforce
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from torch.distributions import Independent, Normal

    ra, _ = _real_mujoco_nets()
    fa, _ = _fake_mujoco_nets()
    pol = ProbabilisticActorPolicy(actor=ra, dist_fn=lambda loc_scale: Independent(Normal(*loc_scale), 1),
                                   action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    real = Reinforce(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=0.97, return_standardization=True)
    fake = SI.Reinforce(policy=SI.Policy(fa), lr=1e-3, gamma=0.97, return_standardization=True)
    _same_state_dicts(((real.policy.actor, fake.policy.actor),))
    r, f = real.discounted_return_computation, fake.discounted_return_computation
    assert (r.gamma, r.return_standardization, r.eps) == (f.gamma, f.return_standardization, f.eps)
    assert (r.ret_rms.mean, r.ret_rms.var, r.ret_rms.count) == (f.ret_rms.mean, f.ret_rms.var, f.ret_rms.count)
    shapes = lambda o: [tuple(p.shape) for g in o._optim.param_groups for p in g["params"]]   # noqa: E731
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam and shapes(real.optim) == shapes(fake.optim)
    from tianshou_amd.integration import make_hip_reinforce

    A, B = make_hip_reinforce(), make_hip_reinforce(ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine", "_dims"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_recurrent_standin_has_the_reference_surface():
    """Recurrent (utils/net/common.py:372-452) under DQN: state_dict keys and shapes of the model and its lagged copy; the hook
    bodies of HipDRQN are the same code objects over either namespace."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Recurrent

    real = DQN(policy=DiscreteQLearningPolicy(model=Recurrent(layer_num=2, state_shape=(6,), action_shape=3, hidden_layer_size=64),
                                              action_space=gym.spaces.Discrete(3)),
               optim=AdamOptimizerFactory(lr=1e-3), gamma=0.95, n_step_return_horizon=2, target_update_freq=2)
    fake = SI.DQN(policy=SI.DiscreteQLearningPolicy(SI.Recurrent(2, 6, 3, 64)), lr=1e-3, gamma=0.95, n_step_return_horizon=2,
                  target_update_freq=2)
    _same_state_dicts(((real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)))
    for name in ("gamma", "n_step", "target_update_freq", "is_double", "huber_loss_delta", "_iter"):
        assert getattr(real, name) == getattr(fake, name), name
    from tianshou_amd import drqn as R
    from tianshou_amd.integration import make_hip_drqn

    assert list(fake.policy.model.state_dict().keys()) == R.state_dict_keys(2)
    A, B = make_hip_drqn(), make_hip_drqn(ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_redq_standin_has_the_reference_surface():
    """REDQ over the nets of test/continuous/test_redq.py:86-107 (EnsembleLinear critics) against the real classes."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.redq import REDQ, REDQPolicy, REDQTrainingStats
    from tianshou.algorithm.modelfree.sac import AutoAlpha
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import EnsembleLinear, Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    E = 4
    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[256, 256]), action_shape=(3,),
                                         unbounded=True, conditioned_sigma=True)
    lin = lambda x, y: EnsembleLinear(E, x, y)   # noqa: E731
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[256, 256], concat=True,
                                                 linear_layer=lin), linear_layer=lin, flatten_input=False)
    real = REDQ(policy=REDQPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,))),
                policy_optim=AdamOptimizerFactory(lr=1e-3), critic=critic, critic_optim=AdamOptimizerFactory(lr=1e-3),
                ensemble_size=E, subset_size=2, tau=0.01, gamma=0.97, alpha=AutoAlpha(-3.0, -0.6, AdamOptimizerFactory(lr=3e-4)),
                actor_delay=2, target_mode="min")
    f_actor = SI.ContinuousActorProbabilistic(SI.Net(11, [256, 256], nn.ReLU), 3, unbounded=True, conditioned_sigma=True)
    flin = lambda x, y: SI.EnsembleLinear(E, x, y)   # noqa: E731
    f_critic = SI.ContinuousCritic(SI.Net(14, [256, 256], nn.ReLU, linear_layer=flin), linear_layer=flin)
    fake = SI.REDQ(policy=SI.Policy(f_actor), critic=f_critic, lr=1e-3, critic_lr=1e-3, ensemble_size=E, subset_size=2, tau=0.01,
                   gamma=0.97, alpha=SI.AutoAlpha(-3.0, -0.6, 3e-4), actor_delay=2, target_mode="min")
    _same_state_dicts(((real.policy.actor, fake.policy.actor), (real.critic, fake.critic),
                       (real.critic_old.module, fake.critic_old.module)))
    for name in ("ensemble_size", "subset_size", "tau", "gamma", "n_step_return_horizon", "actor_delay", "target_mode",
                 "critic_gradient_step", "_last_actor_loss"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("policy_optim", "critic_optim"):
        r, f = getattr(real, name), getattr(fake, name)
        assert type(r._optim) is type(f._optim) is torch.optim.Adam and r._max_grad_norm == f._max_grad_norm
        assert [tuple(p.shape) for p in r._optim.param_groups[0]["params"]] == [tuple(p.shape) for p in f._optim.param_groups[0]["params"]]
    assert float(real.alpha._log_alpha) == float(fake.alpha._log_alpha)
    kw = dict(actor_loss=1.0, critic_loss=2.0, alpha=0.5, alpha_loss=None)
    a, b = REDQTrainingStats(**kw), SI.REDQTrainingStats(**kw)
    assert all(getattr(a, k) == getattr(b, k) for k in kw)
    # EnsembleLinear's initialisation draws: same shapes, same bound
    w = SI.EnsembleLinear(E, 14, 256)
    assert float(w.weight.abs().max()) <= (1.0 / 14) ** 0.5 and tuple(w.bias_weights.shape) == (E, 1, 256)
    from tianshou_amd.integration import make_hip_redq

    A, B = make_hip_redq(), make_hip_redq(ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine", "_hip_parts"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_rainbow_standin_has_the_reference_surface():
    """RainbowDQN / RainbowNet / NoisyLinear stand-ins against the real classes: state_dict keys and shapes (the eps vectors
    included), the bare lagged module, `_sample_noise` consuming torch's generator exactly as the reference (same draws ->
    same noise vectors), the optimizer's parameter list; the hook bodies are the same code objects over either namespace."""
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.c51 import C51Policy
    from tianshou.algorithm.modelfree.rainbow import RainbowDQN
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import RainbowNet

    torch.manual_seed(5)
    real = RainbowDQN(policy=C51Policy(model=RainbowNet(c=4, h=44, w=36, action_shape=[3], num_atoms=21),
                                       action_space=gym.spaces.Discrete(3), num_atoms=21, v_min=-4.0, v_max=4.0),
                      optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97, n_step_return_horizon=2, target_update_freq=2)
    torch.manual_seed(5)
    fake = SI.RainbowDQN(policy=SI.C51Policy(SI.RainbowNet(4, 44, 36, 3, 21), num_atoms=21, v_min=-4.0, v_max=4.0), lr=1e-4,
                         gamma=0.97, n_step_return_horizon=2, target_update_freq=2)
    _same_state_dicts(((real.policy.model, fake.policy.model), (real.model_old, fake.model_old)))
    for k, v in real.policy.model.state_dict().items():               # same constructor draws: identical tensors
        assert torch.equal(v, fake.policy.model.state_dict()[k]), k
    assert real.use_target_network is fake.use_target_network is True
    torch.manual_seed(6)
    assert real._sample_noise(real.policy.model) and real._sample_noise(real.model_old)
    torch.manual_seed(6)
    assert fake._sample_noise(fake.policy.model) and fake._sample_noise(fake.model_old)
    for a, b in ((real.policy.model, fake.policy.model), (real.model_old, fake.model_old)):
        for k in ("Q.0.eps_p", "Q.2.eps_q", "V.0.eps_q", "V.2.eps_p"):
            assert torch.equal(a.state_dict()[k], b.state_dict()[k]), k
    shapes = lambda o: [tuple(p.shape) for g in o._optim.param_groups for p in g["params"]]   # noqa: E731
    assert shapes(real.optim) == shapes(fake.optim)
    from tianshou_amd import rainbow as RB
    from tianshou_amd.integration import make_hip_rainbow

    assert sorted(fake.policy.model.state_dict().keys()) == sorted(RB.TIANSHOU_KEYS + RB.NOISE_KEYS)
    A, B = make_hip_rainbow(), make_hip_rainbow(ref=SI)
    for name in ("__init__", "_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_noise_of"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_a2c_standin_has_the_reference_surface():
    """A2C over the MuJoCo nets: the stand-in carries exactly the attributes the real A2C has (none of PPO's clipping ones), and
    `ppo_config_from` maps both to the same engine configuration; HipA2C's hook bodies are HipPPO's over either namespace."""
    ref_shim.install()
    import gymnasium as gym
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.a2c import A2C
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory

    ra, rc = _real_mujoco_nets()
    fa, fc = _fake_mujoco_nets()
    pol = ProbabilisticActorPolicy(actor=ra, dist_fn=lambda ls: Independent(Normal(*ls), 1),
                                   action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    kw = dict(vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, gae_lambda=0.9, gamma=0.98, return_scaling=False)
    real = A2C(policy=pol, critic=rc, optim=AdamOptimizerFactory(lr=7e-4), **kw)
    fake = SI.A2C(policy=SI.Policy(fa), critic=fc, lr=7e-4, **kw)
    _same_state_dicts(((real.policy.actor, fake.policy.actor), (real.critic, fake.critic)))
    for name in ("vf_coef", "ent_coef", "gae_lambda", "gamma", "return_scaling", "max_batchsize"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("eps_clip", "dual_clip", "value_clip", "advantage_normalization", "recompute_adv"):
        assert not hasattr(real, name) and not hasattr(fake, name), name
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm == 0.5
    from tianshou_amd.integration import make_hip_ppo, ppo_config_from

    assert ppo_config_from(real) == ppo_config_from(fake)
    A, B = make_hip_ppo("a2c"), make_hip_ppo("a2c", ref=SI)
    assert A.__name__ == B.__name__ == "HipA2C"
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_hip_params"):
        assert getattr(A, name).__code__.co_code == getattr(B, name).__code__.co_code, name


def test_layer_norm_trunks_reference_and_standin_agree():
    """Round 6: MLP(norm_layer=nn.LayerNorm) (utils/net/common.py:25-39).  The REAL Net and the stand-in build the same module
    sequence / state_dict keys; `_check_supported` describes both as the per-layer engine's ("net", ..., ("layer_norm", eps))
    with the key order (w, b, gamma, beta)* the flat layout stores; trunks the engine does not cover raise: a norm layer on
    one network only, BatchNorm, NPG's hooks (no forward-mode pass through a layer norm)."""
    ref_shim.install()
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

    from tianshou_amd.integration import _check_supported, _net_keys, _trunk_spec

    def real(norm=nn.LayerNorm, norm_c="same", args=None):
        a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[96, 40], activation=nn.ReLU,
                                                            norm_layer=norm, norm_args=args), action_shape=(3,), unbounded=True)
        c = ContinuousCritic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[64], activation=nn.ReLU,
                                                norm_layer=norm if norm_c == "same" else norm_c, norm_args=args))
        return a, c

    ra, rc = real(args=dict(eps=1e-3))
    fa = SI.ContinuousActorProbabilistic(SI.Net(11, [96, 40], nn.ReLU, norm_layer=nn.LayerNorm, norm_args=dict(eps=1e-3)), 3, unbounded=True)
    fc = SI.ContinuousCritic(SI.Net(11, [64], nn.ReLU, norm_layer=nn.LayerNorm, norm_args=dict(eps=1e-3)))
    assert list(ra.state_dict().keys()) == list(fa.state_dict().keys()) and list(rc.state_dict().keys()) == list(fc.state_dict().keys())
    for a, c in ((ra, rc), (fa, fc)):
        assert _check_supported(a, c) == (11, 3, ((96, 40), (64,), "relu", ("layer_norm", 1e-3)), "net")
        ka, kc = _net_keys(a, c)
        assert ka == ["preprocess.model.model.0.weight", "preprocess.model.model.0.bias", "preprocess.model.model.1.weight",
                      "preprocess.model.model.1.bias", "preprocess.model.model.3.weight", "preprocess.model.model.3.bias",
                      "preprocess.model.model.4.weight", "preprocess.model.model.4.bias", "mu.model.0.weight", "mu.model.0.bias", "sigma_param"]
        assert kc == ["preprocess.model.model.0.weight", "preprocess.model.model.0.bias", "preprocess.model.model.1.weight",
                      "preprocess.model.model.1.bias", "last.model.0.weight", "last.model.0.bias"]
        with pytest.raises(NotImplementedError):            # the hooks of the other families pass norm=False
            _trunk_spec(a, "actor")
    with pytest.raises(NotImplementedError):
        _check_supported(*real(norm_c=None))                # LayerNorm on the actor only
    with pytest.raises(NotImplementedError):
        _check_supported(*real(norm=nn.BatchNorm1d))
    assert _check_supported(*real(norm=None))[2] == ((96, 40), (64,), "relu")
