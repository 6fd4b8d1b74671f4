"""CPU, only where the reference is mounted (/root/reference, authoring container): the HipPPO
subclass wires into the unmodified reference PPO - hooks overridden with the reference's
signatures, hyper-parameters mapped 1:1, and the product path fails LOUDLY without a GPU (no
silent CPU fallback).  Skipped on the GPU box, where /root/reference does not exist."""
import inspect

import numpy as np
import pytest
import torch

from oracle import ref_shim

pytestmark = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")


@pytest.fixture(scope="module", autouse=True)
def _shim():            # every test here imports the reference: no test may depend on another one having installed the shim
    if ref_shim.reference_available():
        ref_shim.install()


@pytest.fixture(scope="module")
def algo():
    return _make_ppo_algo()


def _make_ppo_algo():
    ref_shim.install()
    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_ppo

    HipPPO = make_hip_ppo()
    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                         action_shape=(6,), unbounded=True)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
    policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1),
                                      action_scaling=True, action_bound_method="clip",
                                      action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    return HipPPO(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), eps_clip=0.2,
                  value_clip=True, vf_coef=0.25, ent_coef=0.0, max_grad_norm=0.5, return_scaling=True,
                  advantage_normalization=False, dual_clip=None, device="cpu", permutations="host")


def test_hooks_keep_reference_signatures(algo):
    from tianshou.algorithm.modelfree.ppo import PPO

    for name in ("_preprocess_batch", "_update_with_batch"):
        mine = inspect.signature(getattr(type(algo), name))
        ref = inspect.signature(getattr(PPO, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(PPO, name)


def test_hyperparameters_map_one_to_one(algo):
    from tianshou_amd.integration import ppo_config_from

    c = ppo_config_from(algo)
    assert (c.eps_clip, c.value_clip, c.vf_coef, c.ent_coef, c.max_grad_norm, c.return_scaling) == \
        (0.2, True, 0.25, 0.0, 0.5, True)
    assert (c.gamma, c.gae_lambda, c.lr, c.betas, c.adam_eps) == (0.99, 0.95, 3e-4, (0.9, 0.999), 1e-8)
    assert c.advantage_normalization is False and c.dual_clip is None and c.recompute_advantage is False


def test_flat_layout_round_trip(algo):
    from tianshou_amd.ppo import flat_from_modules, flat_to_modules

    flat = flat_from_modules(algo.policy.actor, algo.critic, device="cpu")
    assert flat.numel() == 11085
    flat2 = flat + 1.0
    flat_to_modules(flat2, algo.policy.actor, algo.critic)
    assert torch.equal(flat_from_modules(algo.policy.actor, algo.critic, device="cpu"), flat2)


def test_no_silent_cpu_fallback(algo):
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    buf = VectorReplayBuffer(16, 2)
    for _ in range(8):
        buf.add(Batch(obs=np.zeros((2, 17), np.float32), act=np.zeros((2, 6), np.float32), rew=np.zeros(2),
                      terminated=np.zeros(2, bool), truncated=np.zeros(2, bool), obs_next=np.zeros((2, 17), np.float32)))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, batch_size=8, repeat=1)


def test_unsupported_nets_are_rejected():
    ref_shim.install()
    from torch import nn

    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import _check_supported

    def nets(hidden, act=nn.Tanh, n_act=6):
        a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=act),
                                         action_shape=(n_act,), unbounded=True)
        return a, ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=act))

    assert _check_supported(*nets([64, 64])) == (17, 6, 64, "fused")
    assert _check_supported(*nets([128, 128])) == (17, 6, 128, "wide")          # GEMM path (tianshou_amd/ppo_wide.py)
    assert _check_supported(*nets([64, 64], n_act=12)) == (17, 12, 64, "wide")
    # every other trunk Net builds from hidden_sizes + one activation: the per-layer engine (ppo_wide.NetPPOEngine)
    assert _check_supported(*nets([100, 100])) == (17, 6, ((100, 100), (100, 100), "tanh"), "net")
    assert _check_supported(*nets([64, 64], act=nn.ReLU)) == (17, 6, ((64, 64), (64, 64), "relu"), "net")
    assert _check_supported(*nets([64, 32])) == (17, 6, ((64, 32), (64, 32), "tanh"), "net")
    assert _check_supported(*nets([256, 128, 64], act=None)) == (17, 6, ((256, 128, 64), (256, 128, 64), "none"), "net")
    a3, _ = nets([96, 72, 40], act=nn.ReLU)
    _, c2 = nets([64, 48], act=nn.ReLU)
    assert _check_supported(a3, c2) == (17, 6, ((96, 72, 40), (64, 48), "relu"), "net")
    a_cs = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                        action_shape=(6,), unbounded=True, conditioned_sigma=True)
    a_norm = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh,
                                                             norm_layer=nn.LayerNorm), action_shape=(6,), unbounded=True)
    a_mixed, _ = nets([64, 64], act=nn.ELU)
    _, c_relu = nets([64, 64], act=nn.ReLU)
    assert _check_supported(a_cs, nets([64, 64])[1]) == (17, 6, ((64, 64), (64, 64), "tanh", "conditioned_sigma"), "net")
    a_cs20 = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                          action_shape=(20,), unbounded=True, conditioned_sigma=True)
    for bad in (nets([64, 64], n_act=40), nets([32] * 8), nets([2048, 64]), (a_cs20, nets([64, 64])[1]), (a_norm, nets([64, 64])[1]),
                (a_mixed, nets([64, 64])[1]), (nets([64, 64])[0], c_relu)):
        with pytest.raises(NotImplementedError):
            _check_supported(*bad)


def test_trunks_that_are_not_linear_activation_pairs_are_rejected():
    """a Net built with action_shape > 0 (MLP output_dim > 0, utils/net/common.py:169-170) ends in a bare Linear
    layer, Net(softmax=True) appends a softmax; the engines apply the activation after EVERY trunk layer, so both must be
    refused instead of silently training a different network.  Without an activation the trailing Linear IS just another
    linear layer (same function): accepted."""
    ref_shim.install()
    from torch import nn

    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import _check_supported, _trunk_spec

    def actor(net):
        return ContinuousActorProbabilistic(preprocess_net=net, action_shape=(6,), unbounded=True)

    critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
    with_out = Net(state_shape=(17,), action_shape=24, hidden_sizes=[64, 64], activation=nn.Tanh)
    assert isinstance(list(with_out.model.model)[-1], nn.Linear)
    with pytest.raises(NotImplementedError, match="followed by its activation"):
        _check_supported(actor(with_out), critic)
    with pytest.raises(NotImplementedError, match="softmax"):
        _trunk_spec(actor(Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh, softmax=True)), "actor")
    lin = Net(state_shape=(17,), action_shape=24, hidden_sizes=[64, 64], activation=None)
    assert _trunk_spec(actor(lin), "actor")[1:] == ([64, 64, 24], "none")


def test_default_bounded_actor_and_rmsprop_are_inside_the_envelope():
    """ContinuousActorProbabilistic's constructor default is unbounded=False (continuous.py:194,
    230-231) and examples/mujoco/mujoco_a2c.py:117 trains with RMSprop: both map onto the engine configuration."""
    ref_shim.install()
    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import _check_supported, make_hip_ppo, ppo_config_from

    def build(algo, hidden, optim, **actor_kw):
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=nn.Tanh),
                                             action_shape=(6,), **actor_kw)
        critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=nn.Tanh))
        policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=False,
                                          action_bound_method=None, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
        return make_hip_ppo(algo)(policy=policy, critic=critic, optim=optim, device="cpu", permutations="host")

    a = build("a2c", [64, 64], RMSpropOptimizerFactory(lr=7e-4, eps=1e-5, alpha=0.99))            # mujoco_a2c.py:117-121
    assert a._hip_dims == (17, 6, 64, "fused")
    c = ppo_config_from(a)
    assert (c.algo, c.optimizer, c.lr, c.adam_eps, c.rms_alpha, c.rms_momentum, c.rms_centered, c.weight_decay) == \
        ("a2c", "rmsprop", 7e-4, 1e-5, 0.99, 0.0, False, 0.0)
    assert c.max_action == 1.0 and c.to_c().optimizer == 1 and c.to_c().max_action == 1.0          # default actor: bounded
    b = build("ppo", [128, 128], AdamOptimizerFactory(lr=1e-3, weight_decay=1e-2), max_action=2.5)
    assert b._hip_dims == (17, 6, ((128, 128), (128, 128), "tanh"), "net")       # bounded: the per-layer engine, not "wide"
    cb = ppo_config_from(b)
    assert (cb.optimizer, cb.weight_decay, cb.max_action) == ("adam", 1e-2, 2.5)
    u = build("ppo", [128, 128], AdamOptimizerFactory(lr=1e-3), unbounded=True)
    assert u._hip_dims == (17, 6, 128, "wide") and ppo_config_from(u).max_action is None
    with pytest.raises(NotImplementedError, match="one auxiliary"):
        ppo_config_from(build("a2c", [64, 64], RMSpropOptimizerFactory(lr=1e-3, momentum=0.9, centered=True)))


def test_collector_side_policies_become_engine_backed_subclasses_of_the_real_classes():
    """SURVEY 8f N2 on the REAL reference classes (CPU: no kernel runs): HipPPO / HipSAC / HipDQN give `algorithm.policy` --
    the object the Collector calls (data/collector.py:735-744) -- a subclass of its own class whose forward / map_action are
    the engine's; everything else (isinstance, state_dict keys, compute_action, add_exploration_noise, pickling as
    highlevel/persistence.py:106 does it) is the reference's, `policy_forward="torch"` leaves the object alone, and without a
    GPU the forward raises instead of computing on the CPU."""
    ref_shim.install()
    import io
    import pickle

    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.dqn import DiscreteQLearningPolicy
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.modelfree.sac import SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd import policy as HP
    from tianshou_amd.integration import make_hip_dqn, make_hip_ppo, make_hip_sac

    def ppo(hidden, **kw):
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=nn.Tanh),
                                             action_shape=(6,), unbounded=True)
        critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=hidden, activation=nn.Tanh))
        policy = ProbabilisticActorPolicy(actor=actor, dist_fn=_normal_dist, action_scaling=True, action_bound_method="clip",
                                          action_space=gym.spaces.Box(low=-2.0, high=2.0, shape=(6,)))
        return make_hip_ppo()(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), device="cpu", **kw)

    for hidden, fam in (([64, 64], "gauss"), ([128, 128], "gauss_wide"), ([96, 40], "gauss_net")):
        a = ppo(hidden)
        p = a.policy
        assert isinstance(p, ProbabilisticActorPolicy) and isinstance(p, HP._HipForward) and p._hip_family == fam
        assert type(p).__mro__[2] is ProbabilisticActorPolicy and p._hip_owner() is a
        assert list(p.state_dict().keys()) == list(ProbabilisticActorPolicy.state_dict(p).keys())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p(Batch(obs=np.zeros((3, 17), np.float32), info={}), None)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.compute_action(np.zeros(17, np.float32))                       # algorithm_base.py:307-329 goes through forward
        # map_action on an array that did not come from the last forward: the reference's own code
        np.testing.assert_allclose(p.map_action(np.full((2, 6), 0.5, np.float32)), np.full((2, 6), 1.0))
        import copy

        from tests import standin as SI

        pc = copy.deepcopy(p)
        assert type(pc) is type(p) and pc._hip_owner() is None
        pc.action_space = SI.Box(-2.0, 2.0, (6,))          # (the shim's gymnasium stub defines Box locally: not picklable by name)
        buf = io.BytesIO()
        torch.save(pc, buf)                                                   # persistence.py:106
        buf.seek(0)
        q = torch.load(buf, weights_only=False)
        assert type(q) is type(p) and q._hip_owner() is None and q._hip_spec == p._hip_spec
        assert all(torch.equal(x, y) for x, y in zip(q.state_dict().values(), p.state_dict().values()))
        assert isinstance(pickle.loads(pickle.dumps(pc)), ProbabilisticActorPolicy)
    t = ppo([64, 64], policy_forward="torch")
    assert type(t.policy) is ProbabilisticActorPolicy
    with torch.no_grad():
        assert t.policy(Batch(obs=np.zeros((3, 17), np.float32), info={}), None).act.shape == (3, 6)       # the reference's forward

    # SAC
    def sac_net():
        return Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[256, 256], concat=True)

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[256, 256]), action_shape=(3,),
                                         unbounded=True, conditioned_sigma=True)
    sp = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,)))
    s = make_hip_sac()(policy=sp, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=ContinuousCritic(preprocess_net=sac_net()),
                       critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=ContinuousCritic(preprocess_net=sac_net()),
                       critic2_optim=AdamOptimizerFactory(lr=1e-3), device="cpu")
    assert isinstance(s.policy, SACPolicy) and s.policy._hip_family == "sac" and s.policy._hip_spec == dict(obs_dim=11, act_dim=3, hidden=256, depth=2, max_action=0.0, activation="relu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.policy(Batch(obs=np.zeros((2, 11), np.float32), info={}), None)
    # DQN
    qp = DiscreteQLearningPolicy(model=DQNet(c=2, h=44, w=36, action_shape=5), action_space=gym.spaces.Discrete(5), eps_training=0.3)
    d = make_hip_dqn()(policy=qp, optim=AdamOptimizerFactory(lr=1e-4), device="cpu")
    assert isinstance(d.policy, DiscreteQLearningPolicy) and d.policy._hip_family == "q" and d.policy._hip_spec == {"n_act": 5}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.policy(Batch(obs=np.zeros((2, 2, 44, 36), np.uint8), info={}), None)
    d.policy.is_within_training_step = True                                  # epsilon-greedy stays the reference's (dqn.py:153-174)
    np.random.seed(0)
    acts = d.policy.add_exploration_noise(np.zeros(2000, np.int64), Batch(obs=np.zeros((2000, 1)), info={}))
    assert 0.15 < float((acts != 0).mean()) < 0.3                             # eps * (1 - 1 / n_act) = 0.24


def _normal_dist(loc_scale):
    from torch.distributions import Independent, Normal

    return Independent(Normal(*loc_scale), 1)


def test_hip_ppo_update_orchestration_with_engine_double(monkeypatch):
    """HipPPO.update over the REAL reference PPO (CPU engine double): same steps as Algorithm._update
    (algorithm_base.py:586-631) minus the host `buffer.sample(0)`; the scheduler's learning rate reaches the engine on
    every update (mujoco_ppo.py's default linear decay), Adam moments reach torch.optim lazily through state_dict(),
    and load_state_dict drops the engine."""
    ref_shim.install()
    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.a2c import A2CTrainingStats
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory, LRSchedulerFactoryLinear
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.buffer as B
    import tianshou_amd.integration as I
    import tianshou_amd.returns as R

    seen = {"lr": [], "cut": [], "n": []}

    class FakePPO:
        def __init__(self, obs_dim, act_dim, flat, cfg):
            assert (obs_dim, act_dim, flat.numel()) == (17, 6, 11085)
            self.cfg = cfg
            self.params, self.adam_m, self.adam_v, self.adam_step = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat), 0
            self.ret_rms = [0.0, 1.0, 0.0]

        def preprocess(self, obs, obs_next, act, rew, term, trunc, cut, d_n):
            n = obs.shape[0]
            assert obs.shape == obs_next.shape == (n, 17) and act.shape == (n, 6) and rew.dtype == torch.float64
            seen["cut"].append(sorted(int(c) for c in cut[: int(d_n)]))
            seen["n"].append(n)
            z = torch.zeros(n)
            self.ret_rms = [0.5, 2.0, float(n)]
            return {"obs": obs, "act": act, "v_s": z, "returns": z, "adv": z, "logp_old": z}

        def update(self, b, batch_size, repeat, perms):
            assert batch_size == 8 and len(perms) == repeat == 2 and all(len(p) == b["obs"].shape[0] for p in perms)
            seen["lr"].append(self.cfg.lr)
            self.adam_step += 6
            self.params = self.params + 1.0
            self.adam_m = self.adam_m + 0.25
            return torch.tensor([[4.0, 3.0, 2.0, 1.0]] * 6), 6

        def check(self):
            pass

    def cpu_sample_all(self, batch_size):
        assert batch_size == 0
        return torch.as_tensor(np.concatenate([
            self.h_offset[e] + (np.arange(self.h_lengths[e]) if self.h_lengths[e] < (self.h_offset[e + 1] - self.h_offset[e])
                                else (self.h_insertion[e] + np.arange(self.h_lengths[e])) % self.h_lengths[e])
            for e in range(self.buffer_num)]).astype(np.int64))

    def cpu_cuts(m, idx):
        unf = [int(m.h_last_index[e]) for e in range(m.buffer_num) if m.h_lengths[e] > 0 and not bool(m.done[m.h_last_index[e]])]
        pos = np.nonzero(np.isin(idx.numpy(), unf))[0]
        return torch.as_tensor(pos), torch.tensor([len(pos)])

    monkeypatch.setattr(I, "_require_gpu", lambda device, who: None)
    monkeypatch.setattr(I, "PPOEngine", FakePPO)
    monkeypatch.setattr(B, "gather_rows", lambda src, idx: src[idx])
    monkeypatch.setattr(B, "gather_rows_multi", lambda srcs, idx: [s[idx] for s in srcs])
    monkeypatch.setattr(B.DeviceReplayBuffer, "sample_indices", cpu_sample_all)
    monkeypatch.setattr(R, "cut_positions", cpu_cuts)

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                         action_shape=(6,), unbounded=True)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
    policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=True,
                                      action_bound_method="clip", action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
    optim = AdamOptimizerFactory(lr=3e-4).with_lr_scheduler_factory(
        LRSchedulerFactoryLinear(max_epochs=2, epoch_num_steps=40, collection_step_num_env_steps=20))
    algo = I.make_hip_ppo()(policy=policy, critic=critic, optim=optim, eps_clip=0.2, value_clip=True, vf_coef=0.25,
                             ent_coef=0.0, max_grad_norm=0.5, return_scaling=True, advantage_normalization=False,
                             dual_clip=None, device="cpu", permutations="host")
    buf = VectorReplayBuffer(20, 2)
    rng = np.random.default_rng(0)

    def fill(n, done_last=False):
        for i in range(n):
            term = np.array([done_last and i == n - 1, False])
            buf.add(Batch(obs=rng.normal(size=(2, 17)).astype(np.float32), act=rng.normal(size=(2, 6)).astype(np.float32),
                          rew=rng.normal(size=2), terminated=term, truncated=np.zeros(2, bool),
                          obs_next=rng.normal(size=(2, 17)).astype(np.float32)))

    w1 = actor.preprocess.model.model[0].weight
    w0 = w1.detach().clone()
    fill(10, done_last=True)
    with policy_within_training_step(algo.policy):
        with pytest.raises(RuntimeError, match="training step"):
            algo.policy.is_within_training_step = False
            algo.update(buffer=buf, batch_size=8, repeat=2)
        algo.policy.is_within_training_step = True
        s0 = algo.update(buffer=buf, batch_size=8, repeat=2)
        buf.reset()                          # on-policy pattern: same length, same insertion index afterwards
        fill(10)
        s1 = algo.update(buffer=buf, batch_size=8, repeat=2)
    assert isinstance(s0, A2CTrainingStats) and s0.gradient_steps == 6 and s0.loss.mean == 4.0 and s1.train_time > 0
    assert seen["lr"] == [3e-4, pytest.approx(3e-4 * 0.75)]                 # max_update_num = ceil(40 / 20) * 2 = 4
    assert seen["n"] == [20, 20]
    assert seen["cut"] == [[19], [9, 19]]        # env 0 ended on a termination in the first rollout only
    m = algo._hip_mirror
    assert np.array_equal(m.obs.numpy(), np.asarray(buf.obs)) and np.array_equal(m.rew.numpy(), np.asarray(buf.rew))
    assert torch.allclose(w1.detach(), w0 + 2.0)                             # written back after every update
    assert (algo.ret_rms.mean, algo.ret_rms.var, algo.ret_rms.count) == (0.5, 2.0, 20.0)
    assert w1 not in algo.optim._optim.state                                 # Adam moments move lazily ...
    sd = algo.state_dict()                                                   # ... here
    st = algo.optim._optim.state[w1]
    assert float(st["step"]) == 12.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.5))
    assert len(sd["_optimizers"][0]["state"]) == 13
    eng = algo._hip_engine
    algo.load_state_dict(sd)
    assert algo._hip_engine is None and eng is not None
    with policy_within_training_step(algo.policy):
        algo.update(buffer=buf, batch_size=8, repeat=2)
    assert algo._hip_engine is not eng and algo._hip_engine.adam_step == 18  # rebuilt from the loaded optimizer state
    assert torch.allclose(algo._hip_engine.adam_m, torch.full_like(algo._hip_engine.adam_m, 0.75))


# ------------------------------------------------------------------------------------ DQN / SAC subclasses
@pytest.fixture(scope="module")
def dqn_algo():
    return _make_dqn_algo()


def _make_dqn_algo():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.dqn import DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import DQNet
    from tianshou_amd.integration import make_hip_dqn

    net = DQNet(c=4, h=84, w=84, action_shape=6)
    policy = DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(6))
    return make_hip_dqn()(policy=policy, optim=AdamOptimizerFactory(lr=1e-4), gamma=0.99, n_step_return_horizon=3,
                          target_update_freq=500, is_double=True, huber_loss_delta=1.0, device="cpu")


@pytest.fixture(scope="module")
def sac_algo():
    return _make_sac_algo()


def _make_sac_algo():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.sac import AutoAlpha, SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_sac

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[256, 256]),
                                         action_shape=(3,), unbounded=True, conditioned_sigma=True)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[256, 256],  # noqa: E731
                                                     concat=True))
    policy = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,)))
    return make_hip_sac()(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(),
                          critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=mk(),
                          critic2_optim=AdamOptimizerFactory(lr=1e-3), tau=0.005, gamma=0.99,
                          alpha=AutoAlpha(-3.0, 0.0, AdamOptimizerFactory(lr=3e-4)), device="cpu",
                          update_noise="torch")        # (the engine's Philox noise needs the GPU library)


@pytest.mark.parametrize("which", ["dqn", "sac"])
def test_offpolicy_hooks_keep_reference_signatures(which, dqn_algo, sac_algo):
    algo = dqn_algo if which == "dqn" else sac_algo
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)


@pytest.mark.parametrize("which", ["dqn", "sac"])
def test_offpolicy_no_silent_cpu_fallback(which, dqn_algo, sac_algo):
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = dqn_algo if which == "dqn" else sac_algo
    buf = VectorReplayBuffer(16, 2)
    shape, act = ((4, 84, 84), np.zeros(2, np.int64)) if which == "dqn" else ((11,), np.zeros((2, 3), np.float32))
    for _ in range(8):
        buf.add(Batch(obs=np.zeros((2, *shape), np.uint8 if which == "dqn" else np.float32), act=act, rew=np.zeros(2),
                      terminated=np.zeros(2, bool), truncated=np.zeros(2, bool),
                      obs_next=np.zeros((2, *shape), np.uint8 if which == "dqn" else np.float32)))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)


def test_unsupported_dqn_model_is_rejected():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.dqn import DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou_amd.integration import make_hip_dqn

    policy = DiscreteQLearningPolicy(model=Net(state_shape=(4,), action_shape=2, hidden_sizes=[64]),
                                     action_space=gym.spaces.Discrete(2))
    with pytest.raises(NotImplementedError):
        make_hip_dqn()(policy=policy, optim=AdamOptimizerFactory(lr=1e-3), device="cpu")


def test_mirror_incremental_sync_tracks_the_reference_buffer():
    """DeviceReplayBuffer.sync_from_tianshou copies exactly the slots written since the last sync (ring wrap,
    uneven sub-buffers); host-side logic, checked here on a CPU mirror."""
    ref_shim.install()
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou_amd.buffer import DeviceReplayBuffer

    rng = np.random.default_rng(0)
    buf = VectorReplayBuffer(30, 3)

    def add(n, ids=None):
        ids = np.arange(3) if ids is None else np.asarray(ids)
        for _ in range(n):
            k = len(ids)
            buf.add(Batch(obs=rng.normal(size=(k, 5)).astype(np.float32), act=rng.normal(size=(k, 2)).astype(np.float32),
                          rew=rng.normal(size=k), terminated=rng.random(k) < 0.2, truncated=rng.random(k) < 0.1,
                          obs_next=rng.normal(size=(k, 5)).astype(np.float32)), buffer_ids=ids)

    add(4)
    m = DeviceReplayBuffer.from_tianshou(buf, device="cpu")
    total = 0
    for n, ids in ((3, None), (5, [0, 2]), (9, [1]), (0, None), (4, None)):
        add(n, ids)
        total += m.sync_from_tianshou(buf)
        for key in ("obs", "act", "obs_next"):
            assert np.array_equal(getattr(m, key).numpy(), np.asarray(getattr(buf, key))), key
        assert np.array_equal(m.rew.numpy(), np.asarray(buf.rew))
        assert np.array_equal(m.done.numpy().astype(bool), np.asarray(buf.done))
        assert np.array_equal(m.last_index.numpy(), np.asarray(buf.last_index))
        assert np.array_equal(m.lengths.numpy(), np.asarray(buf._lengths))
    assert 0 < total < 4 * 30            # incremental, not whole-buffer copies

    def same():
        for key in ("obs", "act", "obs_next"):
            assert np.array_equal(getattr(m, key).numpy(), np.asarray(getattr(buf, key))), key
        assert np.array_equal(m.rew.numpy(), np.asarray(buf.rew))
        assert np.array_equal(m.done.numpy().astype(bool), np.asarray(buf.done))

    # the cases `_insertion_idx` / len() cannot tell apart from "nothing happened" (ADVICE r1):
    add(10)                              # exactly `size` adds to every (already full) sub-buffer
    assert m.sync_from_tianshou(buf) == 30
    same()
    add(23, [1])                         # more than `size` adds to one sub-buffer
    assert m.sync_from_tianshou(buf) == 10
    same()
    buf.reset()                          # on-policy pattern: reset, then refill to the same length
    add(10)
    assert m.sync_from_tianshou(buf) == 30
    same()
    assert m.sync_from_tianshou(buf) == 0
    # the write log is plain data: the buffer still pickles / deep-copies, and a copy keeps counting
    import copy
    import pickle
    buf2 = pickle.loads(pickle.dumps(buf))
    buf3 = copy.deepcopy(buf)
    assert np.array_equal(np.asarray(buf2.rew), np.asarray(buf.rew)) and len(buf3) == len(buf)
    add(2)
    assert m.sync_from_tianshou(buf) == 6
    same()


# ------------------------------------------------------------------------------------ Atari PPO, TD3, DDPG subclasses
def _det_algo(twin):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.ddpg import ContinuousDeterministicPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousCritic
    from tianshou_amd.integration import make_hip_ddpg, make_hip_td3

    actor = ContinuousActorDeterministic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[256, 256]),
                                         action_shape=(3,), max_action=1.0)
    mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[256, 256],  # noqa: E731
                                                     concat=True))
    policy = ContinuousDeterministicPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,)),
                                           exploration_noise=None)
    kw = dict(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(),
              critic_optim=AdamOptimizerFactory(lr=1e-3), device="cpu")
    if twin:
        return make_hip_td3()(critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3), **kw)
    return make_hip_ddpg()(**kw)


def _ppo_cnn_algo():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic
    from tianshou_amd.integration import make_hip_ppo_cnn

    net = DQNet(c=4, h=84, w=84, action_shape=6, features_only=True, output_dim_added_layer=512)
    actor = DiscreteActor(preprocess_net=net, action_shape=6, softmax_output=False)
    critic = DiscreteCritic(preprocess_net=net)
    policy = DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(6))
    return make_hip_ppo_cnn()(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=2.5e-4, eps=1e-5),
                              eps_clip=0.1, value_clip=True, vf_coef=0.25, ent_coef=0.01, max_grad_norm=0.5,
                              device="cpu")


@pytest.mark.parametrize("which", ["td3", "ddpg", "ppo_cnn"])
def test_more_subclasses_keep_signatures_and_fail_loudly(which):
    from tianshou.data import Batch, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _ppo_cnn_algo() if which == "ppo_cnn" else _det_algo(which == "td3")
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    for _ in range(8):
        if which == "ppo_cnn":
            b = Batch(obs=np.zeros((2, 4, 84, 84), np.uint8), act=np.zeros(2, np.int64), rew=np.zeros(2),
                      terminated=np.zeros(2, bool), truncated=np.zeros(2, bool), obs_next=np.zeros((2, 4, 84, 84), np.uint8))
        else:
            b = Batch(obs=np.zeros((2, 11), np.float32), act=np.zeros((2, 3), np.float32), rew=np.zeros(2),
                      terminated=np.zeros(2, bool), truncated=np.zeros(2, bool), obs_next=np.zeros((2, 11), np.float32))
        buf.add(b)
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        if which == "ppo_cnn":
            algo.update(buffer=buf, batch_size=8, repeat=1)
        else:
            algo.update(buffer=buf, sample_size=8)


# ------------------------------------------------------------------------------------ wrappers run end to end (CPU doubles)
# The kernels cannot run in this container, so the device engines are replaced by CPU doubles with the engines'
# interface; what is exercised is the shipped wrapper plumbing: device mirror of the host buffer, hook order and
# arguments, stats objects, write-back of parameters / lagged networks / Adam state.
def _patch_for_cpu(monkeypatch):
    import tianshou_amd.buffer as B
    import tianshou_amd.integration as I

    monkeypatch.setattr(I, "_require_gpu", lambda device, who: None)
    monkeypatch.setattr(B, "gather_rows", lambda src, idx: src[idx])
    monkeypatch.setattr(B, "gather_rows_multi", lambda srcs, idx: [s[idx] for s in srcs])


def _zeros_like_all(obj, names):
    for n in names:
        setattr(obj, n + "_m", torch.zeros_like(getattr(obj, n)))
        setattr(obj, n + "_v", torch.zeros_like(getattr(obj, n)))


def _fill(buf, n, obs_shape, act, dtype=np.float32):
    from tianshou.data import Batch

    for _ in range(n):
        buf.add(Batch(obs=(np.random.rand(2, *obs_shape) * 255).astype(dtype), act=act, rew=np.zeros(2),
                      terminated=np.zeros(2, bool), truncated=np.zeros(2, bool),
                      obs_next=np.zeros((2, *obs_shape), dtype)))


class _FakeSAC:
    """tianshou_amd.sac.SACEngine's interface on the CPU: every update adds 1 to the actor, 0.5 to its first Adam moment,
    0.25 to log alpha, 0.125 to log alpha's first Adam moment and 0.125 to the lagged critics."""

    def __init__(self, obs_dim, act_dim, actor, c1, c2, cfg, hidden=256, depth=2, max_action=0.0, activation="relu"):
        assert hidden == 256
        self.hidden = hidden
        self.obs_dim, self.act_dim, self.cfg, self.adam_step = obs_dim, act_dim, cfg, 0
        self.actor, self.critic1, self.critic2 = actor.clone(), c1.clone(), c2.clone()
        self.critic1_old, self.critic2_old = c1.clone(), c2.clone()
        _zeros_like_all(self, ("actor", "critic1", "critic2"))
        self.log_alpha, self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)

    def preprocess(self, m, idx, noise):
        assert noise.shape == (idx.numel(), self.act_dim) and m.obs_next is not None
        return torch.zeros(idx.numel())

    def update_with_batch(self, obs, act, ret, noise, weight=None):
        assert obs.shape == (8, self.obs_dim) and act.shape == (8, self.act_dim)
        self.adam_step += 1
        self.actor += 1.0
        self.actor_m += 0.5
        self.log_alpha += 0.25
        self.log_alpha_m += 0.125
        self.critic1_old += 0.125
        return torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]), torch.ones(8)


class _FakeDQN:
    """tianshou_amd.dqn.DQNEngine's interface on the CPU: every update adds 2 to the parameters, 0.5 to the lagged network's and
    0.25 to the second Adam moment."""

    def __init__(self, c, h, w, n_act, flat, cfg):
        self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
        self.params, self.params_old = flat.clone(), flat.clone()
        self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

    def preprocess_with_obs(self, m, frames, idx, stack, obs_next_frames=None, prefetch=True):
        assert frames.dtype == torch.uint8 and stack == 1 and obs_next_frames is not None and prefetch
        return frames[idx].permute(0, 2, 3, 1), torch.zeros(idx.numel())

    def update_with_batch(self, obs, act, ret, weight=None):
        assert obs.shape == (8, 84, 84, 4) and obs.dtype == torch.uint8
        self.adam_step += 1
        self.iter += 1
        self.params += 2.0
        self.params_old += 0.5
        self.adam_v += 0.25
        return torch.tensor([0.75]), torch.arange(8, dtype=torch.float32)


def test_hip_sac_wrapper_runs_with_engine_double(sac_algo, monkeypatch):
    from tianshou.algorithm.modelfree.sac import SACTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.sac as S

    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(S, "SACEngine", _FakeSAC)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (11,), np.zeros((2, 3), np.float32))
    sac_algo._hip_engine = None
    first = next(iter(sac_algo.policy.actor.parameters()))
    before = first.detach().clone()
    with policy_within_training_step(sac_algo.policy):
        stats = sac_algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, SACTrainingStats) and (stats.actor_loss, stats.critic2_loss, stats.alpha) == (1.0, 3.0, 4.0)
    assert torch.equal(first.detach(), before)                    # write_back="auto" + the engine's policy forward: lazy
    sac_algo.policy.state_dict()                                  # a reader of the torch state: syncs
    assert torch.allclose(first.detach(), before + 1.0)                                   # engine -> nn.Parameter
    st = sac_algo.policy_optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.5))
    assert abs(float(sac_algo.alpha._log_alpha) - 0.25) < 1e-6


def test_hip_dqn_wrapper_runs_with_engine_double(dqn_algo, monkeypatch):
    from tianshou.algorithm.modelfree.reinforce import SimpleLossTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.dqn as D

    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(D, "DQNEngine", _FakeDQN)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    dqn_algo._hip_engine = None
    first = next(iter(dqn_algo.policy.model.parameters()))
    before = first.detach().clone()
    with policy_within_training_step(dqn_algo.policy):
        stats = dqn_algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, SimpleLossTrainingStats) and stats.loss == 0.75
    # defaults since round 6: index-only sampling, write-back when the torch state is read (the policy forward is the engine's)
    assert dqn_algo.__dict__["_hip_lazy"] and dqn_algo.__dict__["_hip_stale"] and torch.equal(first.detach(), before)
    sd = dqn_algo.policy.state_dict()                       # a reader (the real reference module's state_dict()): syncs
    assert not dqn_algo.__dict__["_hip_stale"] and torch.allclose(sd["model.net.0.0.weight"], before + 2.0)
    assert torch.allclose(first.detach(), before + 2.0)
    st = dqn_algo.optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.25))


@pytest.mark.parametrize("twin", [True, False])
def test_hip_td3_ddpg_wrapper_runs_with_engine_double(twin, monkeypatch):
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.td3 as T

    class FakeTD3:
        def __init__(self, obs_dim, act_dim, actor, c1, c2, cfg, hidden=256, depth=2, max_action=0.0, activation="relu"):
            self.hidden = hidden
            self.obs_dim, self.act_dim, self.cfg, self.cnt, self.actor_steps = obs_dim, act_dim, cfg, 0, 0
            self.actor, self.critic1, self.critic2 = actor.clone(), c1.clone(), None if c2 is None else c2.clone()
            names = ("actor", "critic1") + (("critic2",) if c2 is not None else ())
            for n in names:
                setattr(self, n + "_old", getattr(self, n).clone())
            _zeros_like_all(self, names)

        def preprocess(self, m, idx, noise):
            assert (noise is not None) == self.cfg.twin
            return torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret, weight=None):
            self.cnt += 1
            self.actor_steps += 1
            self.critic1 += 3.0
            self.actor_old += 1.5
            return torch.tensor([0.1, 0.2, 0.3]), torch.ones(8)

    algo = _det_algo(twin)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(T, "TD3Engine", FakeTD3)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (11,), np.zeros((2, 3), np.float32))
    c_first = next(iter(algo.critic.parameters()))
    before = c_first.detach().clone()
    old_first = next(iter(algo.actor_old.module.parameters()))
    old_before = old_first.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert abs(stats.actor_loss - 0.1) < 1e-6 and abs((stats.critic1_loss if twin else stats.critic_loss) - 0.2) < 1e-6
    assert torch.allclose(c_first.detach(), before + 3.0) and torch.allclose(old_first.detach(), old_before + 1.5)
    assert float(algo.critic_optim._optim.state[c_first]["step"]) == 1.0


def test_hip_ppo_cnn_wrapper_runs_with_engine_double(monkeypatch):
    from tianshou.algorithm.modelfree.a2c import A2CTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.ppo_cnn as PC

    class FakeCnnPPO:
        def __init__(self, c, h, w, n_act, flat, cfg):
            self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
            self.params, self.adam_m, self.adam_v, self.adam_step = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat), 0
            self.ret_rms = [0.0, 1.0, 0.0]

        def preprocess(self, m, frames, act, stack, obs_next_frames=None):
            n = len(m)
            assert frames.dtype == torch.uint8 and act.shape[0] == m.maxsize
            z = torch.zeros(n)
            return {"indices": torch.arange(n), "act": act[:n], "v_s": z, "returns": z, "adv": z, "logp_old": z}

        def update(self, m, frames, pre, stack, batch_size, repeat, perms):
            assert len(perms) == repeat and sorted(perms[0].tolist()) == list(range(pre["indices"].numel()))
            self.adam_step += 3
            self.params += 1.0
            return torch.tensor([[4.0, 3.0, 2.0, 1.0]] * 3), 3

    algo = _ppo_cnn_algo()
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(PC, "CnnPPOEngine", FakeCnnPPO)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    head = algo.critic.last.model[0].weight
    before = head.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, batch_size=8, repeat=1)
    assert isinstance(stats, A2CTrainingStats) and stats.gradient_steps == 3 and stats.loss.mean == 4.0
    assert torch.allclose(head.detach(), before + 1.0)
    assert float(algo.optim._optim.state[head]["step"]) == 3.0


# ------------------------------------------------------------------------------------ QRDQN / C51 subclasses
def _distq_algo(kind):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou_amd.integration import make_hip_c51, make_hip_qrdqn

    if kind == "qr":
        from tianshou.algorithm.modelfree.qrdqn import QRDQNPolicy
        from tianshou.env.atari.atari_network import QRDQNet

        net = QRDQNet(c=4, h=84, w=84, action_shape=[6], num_quantiles=20)
        policy = QRDQNPolicy(model=net, action_space=gym.spaces.Discrete(6))
        return make_hip_qrdqn()(policy=policy, optim=AdamOptimizerFactory(lr=1e-4), num_quantiles=20,
                                n_step_return_horizon=3, target_update_freq=500, device="cpu")
    from tianshou.algorithm.modelfree.c51 import C51Policy
    from tianshou.env.atari.atari_network import C51Net

    net = C51Net(c=4, h=84, w=84, action_shape=[6], num_atoms=11)
    policy = C51Policy(model=net, action_space=gym.spaces.Discrete(6), num_atoms=11, v_min=-2.0, v_max=3.0)
    return make_hip_c51()(policy=policy, optim=AdamOptimizerFactory(lr=1e-4), n_step_return_horizon=2,
                          target_update_freq=0, device="cpu")


@pytest.mark.parametrize("kind", ["qr", "c51"])
def test_distq_subclasses_keep_signatures_and_fail_loudly(kind):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _distq_algo(kind)
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    assert type(algo).__name__ == ("HipQRDQN" if kind == "qr" else "HipC51")
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)


@pytest.mark.parametrize("kind", ["qr", "c51"])
def test_hip_distq_wrapper_runs_with_engine_double(kind, monkeypatch):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.distq as Q
    import tianshou_amd.dqn as D

    n_atoms = 20 if kind == "qr" else 11

    class FakeDistQ:
        def __init__(self, c, h, w, n_act, flat, cfg):
            assert (c, h, w, n_act) == (4, 84, 84, 6) and cfg.kind == kind and cfg.n_atoms == n_atoms
            assert flat.numel() == 8224 + 32832 + 36928 + 3137 * 512 + 513 * ((6 * n_atoms + 31) // 32 * 32)
            if kind == "c51":
                assert (cfg.v_min, cfg.v_max) == (-2.0, 3.0)
            self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
            self.params = flat.clone()
            self.params_old = flat.clone() if cfg.target_update_freq > 0 else None
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

        def preprocess(self, m, frames, idx, stack, obs_next_frames=None):
            assert frames.dtype == torch.uint8 and stack == 1 and obs_next_frames is not None
            return torch.zeros((idx.numel(), n_atoms))

        def update_with_batch(self, obs, act, ret, weight=None, obs_next_nhwc=None):
            assert obs.shape == (8, 84, 84, 4) and ret.shape == (8, n_atoms)
            assert (obs_next_nhwc is not None) == (kind == "c51")
            self.adam_step += 1
            self.iter += 1
            self.params += 2.0
            self.adam_m += 0.125
            return torch.tensor([0.5]), torch.arange(8, dtype=torch.float32)

    algo = _distq_algo(kind)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(Q, "DistQEngine", FakeDistQ)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    first = next(iter(algo.policy.model.parameters()))
    before = first.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    loss = stats.loss if kind == "qr" else stats.loss
    assert float(loss if isinstance(loss, float) else getattr(loss, "mean", loss)) == 0.5
    assert torch.allclose(first.detach(), before + 2.0)
    st = algo.optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125))
    if kind == "qr":                                       # lagged network written back too
        old_first = next(iter(algo.model_old.parameters()))
        assert torch.allclose(old_first.detach(), before)


# ------------------------------------------------------------------------------------ DiscreteSAC subclass
def _dsac_algo(auto=True, hidden=64, **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.discrete_sac import DiscreteSACPolicy
    from tianshou.algorithm.modelfree.sac import AutoAlpha
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic
    from tianshou_amd.integration import make_hip_discrete_sac

    mk = lambda: Net(state_shape=(11,), hidden_sizes=[hidden, hidden])  # noqa: E731
    actor = DiscreteActor(preprocess_net=mk(), action_shape=5, softmax_output=False)
    c1, c2 = DiscreteCritic(preprocess_net=mk(), last_size=5), DiscreteCritic(preprocess_net=mk(), last_size=5)
    policy = DiscreteSACPolicy(actor=actor, action_space=gym.spaces.Discrete(5))
    alpha = AutoAlpha(0.98 * float(np.log(5)), 0.0, AdamOptimizerFactory(lr=3e-4)) if auto else 0.05
    return make_hip_discrete_sac()(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=c1,
                                   critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=c2,
                                   critic2_optim=AdamOptimizerFactory(lr=1e-3), alpha=alpha, n_step_return_horizon=2,
                                   device="cpu", **kw)


def test_discrete_sac_subclass_keeps_signatures_and_fails_loudly():
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _dsac_algo()
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (11,), np.zeros(2, np.int64))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)
    a48 = _dsac_algo(hidden=48)                            # other widths: embedded by zero padding (round 6, widths.py)
    assert a48._hip_hidden == 64 and a48._hip_sizes["actor"] == (48, 48)
    with pytest.raises(NotImplementedError):
        _dsac_algo(hidden=1100)


@pytest.mark.parametrize("match_rng", [True, False])
def test_hip_discrete_sac_wrapper_runs_with_engine_double(match_rng, monkeypatch):
    ref_shim.install()
    from tianshou.algorithm.modelfree.discrete_sac import DiscreteSACTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.dsac as DS
    import tianshou_amd.returns as R

    calls = {"policy_forward": 0}

    class FakeDSAC:
        def __init__(self, obs_dim, n_act, hidden, actor, c1, c2, cfg, depth=2, activation="relu"):
            assert (obs_dim, n_act, hidden) == (11, 5, 64) and cfg.auto_alpha and cfg.n_step == 2
            assert abs(cfg.target_entropy - 0.98 * np.log(5)) < 1e-12
            self.obs_dim, self.n_act, self.hidden, self.cfg, self.adam_step = obs_dim, n_act, hidden, cfg, 0
            self.actor, self.critic1, self.critic2 = actor.clone(), c1.clone(), c2.clone()
            self.critic1_old, self.critic2_old = c1.clone(), c2.clone()
            _zeros_like_all(self, ("actor", "critic1", "critic2"))
            self.log_alpha, self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)

        def policy_forward(self, obs):
            calls["policy_forward"] += 1
            return torch.zeros((obs.shape[0], self.n_act))

        def preprocess(self, m, idx):
            assert m.obs_next is not None
            return torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret, weight=None):
            assert obs.shape == (8, 11) and act.shape == (8,) and act.dtype == torch.int64
            self.adam_step += 1
            self.critic2 += 1.0
            self.critic2_old += 0.5
            self.critic2_v += 0.25
            self.log_alpha += 0.125
            return torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]), torch.ones(8)

    algo = _dsac_algo(match_rng_stream=match_rng)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(DS, "DiscreteSACEngine", FakeDSAC)
    monkeypatch.setattr(DS, "layout", lambda o, a, h, d=2: {"ka": 32, "hw": 32, "count": 33 * h + (h + 1) * h + (h + 1) * 32,
                                                             "offs": [0, 33 * h, 33 * h + (h + 1) * h, 33 * h + (h + 1) * h + (h + 1) * 32]})
    monkeypatch.setattr(R, "nstep_indices", lambda m, idx, n: idx)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (11,), np.zeros(2, np.int64))
    first = next(iter(algo.critic2.parameters()))
    before = first.detach().clone()
    old_first = next(iter(algo.critic2_old.module.parameters()))
    old_before = old_first.detach().clone()
    torch.manual_seed(0)
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, DiscreteSACTrainingStats) and (stats.actor_loss, stats.critic2_loss, stats.alpha) == (1.0, 3.0, 4.0)
    assert calls["policy_forward"] == (2 if match_rng else 0)        # the two unused Categorical.sample() draws
    assert torch.allclose(first.detach(), before + 1.0) and torch.allclose(old_first.detach(), old_before + 0.5)
    st = algo.critic2_optim._optim.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.25))
    assert abs(float(algo.alpha._log_alpha.detach()) - 0.125) < 1e-6


# ------------------------------------------------------------------------------------ PPO, CartPole shape (configs[0])
def _ppo_discrete_algo(softmax=True, hidden=64, dist="match", **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic
    from tianshou_amd.integration import make_hip_ppo_discrete

    net = Net(state_shape=(4,), hidden_sizes=[hidden, hidden])
    actor = DiscreteActor(preprocess_net=net, action_shape=2, softmax_output=softmax)
    critic = DiscreteCritic(preprocess_net=net)
    pk = {}
    if (softmax and dist == "match") or (not softmax and dist == "mismatch"):
        pk["dist_fn"] = torch.distributions.Categorical
    policy = DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(2), **pk)
    return make_hip_ppo_discrete()(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), gamma=0.99,
                                   max_grad_norm=0.5, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, gae_lambda=0.95,
                                   return_scaling=False, dual_clip=None, value_clip=False,
                                   advantage_normalization=False, recompute_advantage=False, device="cpu", **kw)


def test_ppo_discrete_subclass_keeps_signatures_and_fails_loudly():
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    for softmax in (True, False):
        algo = _ppo_discrete_algo(softmax=softmax)
        base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
        for name in ("_preprocess_batch", "_update_with_batch"):
            mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
            assert list(mine.parameters) == list(ref.parameters), name
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (4,), np.zeros(2, np.int64))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, batch_size=8, repeat=1)
    with pytest.raises(NotImplementedError):                    # probabilities handed to a logits dist_fn
        _ppo_discrete_algo(softmax=True, dist="mismatch")
    with pytest.raises(NotImplementedError):
        _ppo_discrete_algo(softmax=False, dist="mismatch")
    with pytest.raises(NotImplementedError):
        _ppo_discrete_algo(hidden=48)


def test_hip_ppo_discrete_wrapper_runs_with_engine_double(monkeypatch):
    ref_shim.install()
    from tianshou.algorithm.modelfree.a2c import A2CTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.ppo_discrete as PD

    class FakeDiscretePPO:
        def __init__(self, obs_dim, hidden, n_act, flat, cfg):
            assert (obs_dim, hidden, n_act) == (4, 64, 2) and flat.numel() == 33 * 64 + 65 * 64 + 65 * 32
            assert cfg.vf_coef == 0.5 and cfg.eps_clip == 0.2 and cfg.max_grad_norm == 0.5 and not cfg.value_clip
            self.obs_dim, self.hidden, self.n_act, self.cfg = obs_dim, hidden, n_act, cfg
            self.params, self.adam_m, self.adam_v, self.adam_step = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat), 0
            self.ret_rms = [0.0, 1.0, 0.0]

        def preprocess(self, m):
            n = len(m)
            assert m.obs.shape == (m.maxsize, 4) and m.obs_next is not None
            z = torch.zeros(n)
            return {"indices": torch.arange(n), "act": m.act[:n], "v_s": z, "returns": z, "adv": z, "logp_old": z}

        def update(self, m, pre, batch_size, repeat, perms):
            assert batch_size == 8 and len(perms) == repeat == 2
            self.adam_step += 6
            self.params += 1.0
            self.adam_v += 0.5
            return torch.tensor([[4.0, 3.0, 2.0, 1.0]] * 6), 6

    algo = _ppo_discrete_algo()
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(PD, "DiscretePPOEngine", FakeDiscretePPO)
    monkeypatch.setattr(PD, "layout", lambda o, h, a: {"k0": 32, "head": 32, "count": 33 * h + (h + 1) * h + (h + 1) * 32})
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4,), np.zeros(2, np.int64))
    head = algo.critic.last.model[0].weight
    trunk = next(iter(algo.policy.actor.preprocess.parameters()))
    before_h, before_t = head.detach().clone(), trunk.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, batch_size=8, repeat=2)
    assert isinstance(stats, A2CTrainingStats) and stats.gradient_steps == 6 and stats.loss.mean == 4.0
    assert torch.allclose(head.detach(), before_h + 1.0) and torch.allclose(trunk.detach(), before_t + 1.0)
    st = algo.optim._optim.state[head]
    assert float(st["step"]) == 6.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.5))


# ------------------------------------------------------------------------------------ A2C variants of the on-policy subclasses
def test_a2c_subclasses_map_hyperparameters_and_fail_loudly():
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.a2c import A2C
    from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy, ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic
    from tianshou.utils.torch_utils import policy_within_training_step
    from tianshou_amd import integration as I

    kw = dict(optim=AdamOptimizerFactory(lr=7e-4), gamma=0.98, gae_lambda=0.9, vf_coef=0.4, ent_coef=0.02, max_grad_norm=0.6,
              return_scaling=True, device="cpu")
    net = Net(state_shape=(4,), hidden_sizes=[64, 64])
    actor = DiscreteActor(preprocess_net=net, action_shape=2, softmax_output=False)
    disc = I.make_hip_a2c_discrete()(policy=DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(2)),
                                     critic=DiscreteCritic(preprocess_net=net), **kw)
    a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=torch.nn.Tanh),
                                     action_shape=(6,), unbounded=True)
    c = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=torch.nn.Tanh))

    def dist_fn(loc_scale):
        return torch.distributions.Independent(torch.distributions.Normal(*loc_scale), 1)

    pol = ProbabilisticActorPolicy(actor=a, dist_fn=dist_fn, action_space=gym.spaces.Box(-1, 1, (6,)))
    cont = I.make_hip_a2c()(policy=pol, critic=c, **kw)
    for algo, name in ((disc, "HipA2CDiscrete"), (cont, "HipA2C")):
        assert isinstance(algo, A2C) and type(algo).__name__ == name and not hasattr(algo, "eps_clip")
        cfg = I.ppo_config_from(algo)
        assert cfg.algo == "a2c" and (cfg.vf_coef, cfg.ent_coef, cfg.max_grad_norm, cfg.lr) == (0.4, 0.02, 0.6, 7e-4)
        assert (cfg.gamma, cfg.gae_lambda, cfg.return_scaling) == (0.98, 0.9, True) and cfg.to_c().algo == 1
        for name_ in ("_preprocess_batch", "_update_with_batch"):
            mine, ref = inspect.signature(getattr(type(algo), name_)), inspect.signature(getattr(A2C, name_))
            assert list(mine.parameters) == list(ref.parameters), name_
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (4,), np.zeros(2, np.int64))
    with policy_within_training_step(disc.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        disc.update(buffer=buf, batch_size=8, repeat=1)
    assert issubclass(I.make_hip_a2c_cnn(), A2C) and I.make_hip_a2c_cnn().__name__ == "HipA2CCnn"


# ------------------------------------------------------------------------------------ REDQ subclass
def _redq_algo(auto=True, hidden=256, actor_delay=2, **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.redq import REDQPolicy
    from tianshou.algorithm.modelfree.sac import AutoAlpha
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import EnsembleLinear, Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_redq

    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[hidden, hidden]), action_shape=(3,),
                                         unbounded=True, conditioned_sigma=True)
    linear = lambda x, y: EnsembleLinear(4, x, y)  # noqa: E731
    net_c = Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[hidden, hidden], concat=True, linear_layer=linear)
    critic = ContinuousCritic(preprocess_net=net_c, linear_layer=linear, flatten_input=False)
    policy = REDQPolicy(actor=actor, action_space=gym.spaces.Box(-1, 1, (3,)))
    alpha = AutoAlpha(-3.0, 0.0, AdamOptimizerFactory(lr=3e-4)) if auto else 0.2
    return make_hip_redq()(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=critic,
                           critic_optim=AdamOptimizerFactory(lr=1e-3), ensemble_size=4, subset_size=2, alpha=alpha,
                           actor_delay=actor_delay, target_mode="min", n_step_return_horizon=2, device="cpu", **kw)


def test_redq_subclass_keeps_signatures_and_fails_loudly():
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _redq_algo()
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (11,), np.zeros((2, 3), np.float32))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)
    assert _redq_algo(hidden=128)._hip_hidden == 128           # any [h, h] with h a multiple of 32 (<= 1024)
    assert _redq_algo(hidden=100)._hip_hidden == 128           # other widths: embedded by zero padding (round 6, widths.py)
    with pytest.raises(NotImplementedError):
        _redq_algo(hidden=1100)


def test_hip_redq_wrapper_runs_with_engine_double(monkeypatch):
    ref_shim.install()
    from tianshou.algorithm.modelfree.redq import REDQTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.redq as RQ

    seen = {"subsets": [], "noise": []}

    class FakeREDQ:
        def __init__(self, obs_dim, act_dim, actor, critics, cfg, hidden=256, depth=2, max_action=0.0, activation="relu"):
            self.hidden = hidden
            assert (obs_dim, act_dim) == (11, 3) and (cfg.ensemble_size, cfg.subset_size, cfg.actor_delay) == (4, 2, 2)
            assert cfg.auto_alpha and cfg.target_mode == "min" and cfg.n_step == 2 and critics.numel() % 4 == 0
            self.obs_dim, self.act_dim, self.cfg = obs_dim, act_dim, cfg
            self.actor, self.critics, self.critics_old = actor.clone(), critics.clone(), critics.clone()
            _zeros_like_all(self, ("actor", "critics"))
            self.log_alpha, self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)
            self.critic_gradient_step, self.actor_steps, self._stats = 0, 0, torch.zeros(4)

        def will_update_actor(self):
            return (self.critic_gradient_step + 1) % self.cfg.actor_delay == 0

        def preprocess(self, m, idx, noise, subset):
            assert noise.shape == (idx.numel(), 3) and len(subset) == 2 and len(set(subset.tolist())) == 2
            seen["subsets"].append(subset)
            return torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret, noise=None, weight=None):
            do = self.will_update_actor()
            assert (noise is not None) == do
            seen["noise"].append(noise is not None)
            self.critic_gradient_step += 1
            self.actor_steps += int(do)
            self.critics += 1.0
            self.critics_old += 0.5
            self.critics_m += 0.25
            if do:
                self.actor += 2.0
                self.log_alpha += 0.125
            return torch.tensor([3.0 if do else 0.0, 2.0, 1.0, 0.5 if do else float("nan")]), torch.ones(8)

    algo = _redq_algo()
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(RQ, "REDQEngine", FakeREDQ)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (11,), np.zeros((2, 3), np.float32))
    c_first = next(iter(algo.critic.parameters()))
    a_first = next(iter(algo.policy.actor.parameters()))
    c0, a0 = c_first.detach().clone(), a_first.detach().clone()
    old_first = next(iter(algo.critic_old.module.parameters()))
    o0 = old_first.detach().clone()
    with policy_within_training_step(algo.policy):
        s1 = algo.update(buffer=buf, sample_size=8)
        s2 = algo.update(buffer=buf, sample_size=8)
    assert isinstance(s2, REDQTrainingStats) and seen["noise"] == [False, True] and len(seen["subsets"]) == 2
    assert (s1.actor_loss, s1.critic_loss, s1.alpha_loss) == (0.0, 2.0, None) and (s2.actor_loss, s2.alpha_loss) == (3.0, 0.5)
    assert algo.critic_gradient_step == 2 and algo._last_actor_loss == 3.0
    assert torch.allclose(c_first.detach(), c0 + 2.0) and torch.allclose(a_first.detach(), a0 + 2.0)
    assert torch.allclose(old_first.detach(), o0 + 1.0)
    st = algo.critic_optim._optim.state[c_first]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.5))
    assert float(algo.policy_optim._optim.state[a_first]["step"]) == 1.0
    assert abs(float(algo.alpha._log_alpha.detach()) - 0.125) < 1e-6


# ------------------------------------------------------------------------------------ Rainbow subclass
def _rainbow_algo(freq=2, **net_kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.c51 import C51Policy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import RainbowNet
    from tianshou_amd.integration import make_hip_rainbow

    net = RainbowNet(c=4, h=84, w=84, action_shape=[6], num_atoms=11, **net_kw)
    policy = C51Policy(model=net, action_space=gym.spaces.Discrete(6), num_atoms=11, v_min=-2.0, v_max=3.0)
    return make_hip_rainbow()(policy=policy, optim=AdamOptimizerFactory(lr=1e-4), n_step_return_horizon=3,
                              target_update_freq=freq, device="cpu")


def test_rainbow_subclass_keeps_signatures_and_fails_loudly():
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _rainbow_algo()
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)
    with pytest.raises(NotImplementedError):
        _rainbow_algo(is_dueling=False)
    with pytest.raises(NotImplementedError):
        _rainbow_algo(is_noisy=False)


def test_hip_rainbow_wrapper_runs_with_engine_double(monkeypatch):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.dqn as D
    import tianshou_amd.rainbow as RB

    lay = {"F": 3136, "ldq": 96, "ldv": 32}
    n_noise = 2 * (3136 + 512) + 2 * 512 + 96 + 32
    count = 8224 + 32832 + 36928 + 2 * (2 * 3137 * 512 + 513 * 96 + 513 * 32)
    offs, o = [], 0
    for n in (3136, 512, 512, 96, 3136, 512, 512, 32):
        offs.append(o)
        o += n
    lin, o = [], 8224 + 32832 + 36928
    for fin, pad in ((3136, 512), (512, 96), (3136, 512), (512, 32)):
        lin.append(o)
        o += 2 * (fin + 1) * pad
    monkeypatch.setattr(RB, "layout", lambda *a: {**lay, "count": count, "noise_count": n_noise, "conv": [0, 8224, 41056],
                                                  "lin": lin, "noise": offs})
    seen = {"set_noise": []}

    class FakeRainbow:
        def __init__(self, c, h, w, n_act, flat, noise, cfg):
            assert (c, h, w, n_act, cfg.n_atoms, cfg.kind) == (4, 84, 84, 6, 11, "c51") and (cfg.v_min, cfg.v_max) == (-2.0, 3.0)
            assert flat.numel() == count and noise.numel() == n_noise and cfg.target_update_freq == 2
            self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
            self.params, self.params_old, self.noise, self.noise_old = flat.clone(), flat.clone(), noise.clone(), noise.clone()
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

        def preprocess(self, m, idx):
            return torch.zeros((idx.numel(), 11))

        def set_noise(self, noise, noise_old=None):
            seen["set_noise"].append((noise.clone(), None if noise_old is None else noise_old.clone()))

        def update_with_batch(self, obs, act, ret, obs_next, weight=None):
            assert obs.shape == obs_next.shape == (8, 84, 84, 4) and ret.shape == (8, 11)
            self.adam_step += 1
            self.iter += 1
            self.params += 1.0
            self.adam_v += 0.5
            return torch.tensor([0.25]), torch.arange(8, dtype=torch.float32)

    algo = _rainbow_algo()
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(RB, "RainbowEngine", FakeRainbow)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    model = algo.policy.model
    sig = model.V[2].sigma_W
    before = sig.detach().clone()
    eps_before = model.Q[0].eps_q.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert float(getattr(stats.loss, "mean", stats.loss)) == 0.25
    assert torch.allclose(sig.detach(), before + 1.0)                          # engine -> nn.Parameter (sigma of a noisy layer)
    assert not torch.equal(model.Q[0].eps_q.detach(), eps_before)              # the torch modules drew fresh noise ...
    noise, noise_old = seen["set_noise"][0]
    assert noise_old is not None and not torch.equal(noise, noise_old)
    assert torch.allclose(noise[3136:3136 + 512], model.Q[0].eps_q.detach())   # ... and the engine received exactly it
    assert torch.equal(algo.model_old.Q[0].eps_q, model.Q[0].eps_q)            # first update syncs: noise carried along
    st = algo.optim._optim.state[sig]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.5))


# ------------------------------------------------------------------------------------ NPG / TRPO subclasses
def _natural_algo(which, hidden=64, **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd import integration as I

    a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[hidden, hidden], activation=torch.nn.Tanh),
                                     action_shape=(6,), unbounded=True)
    c = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[hidden, hidden], activation=torch.nn.Tanh))

    def dist_fn(loc_scale):
        return torch.distributions.Independent(torch.distributions.Normal(*loc_scale), 1)

    pol = ProbabilisticActorPolicy(actor=a, dist_fn=dist_fn, action_space=gym.spaces.Box(-1, 1, (6,)))
    common = dict(policy=pol, critic=c, optim=AdamOptimizerFactory(lr=1e-3), optim_critic_iters=3, gae_lambda=0.9, gamma=0.98,
                  device="cpu")
    if which == "npg":
        return I.make_hip_npg()(trust_region_size=0.2, **common, **kw)
    return I.make_hip_trpo()(max_kl=0.02, backtrack_coeff=0.7, max_backtracks=8, **common, **kw)


@pytest.mark.parametrize("which", ["npg", "trpo"])
def test_natural_gradient_subclasses_keep_signatures_and_fail_loudly(which):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _natural_algo(which)
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    assert type(algo).__name__ == ("HipNPG" if which == "npg" else "HipTRPO")
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (17,), np.zeros((2, 6), np.float32))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, batch_size=8, repeat=1)
    a48 = _natural_algo(which, hidden=48)                  # other widths: embedded by zero padding (round 6, widths.py)
    assert a48._hip_hidden == 64 and a48._hip_sizes == {"actor": (48, 48), "critic": (48, 48)}
    with pytest.raises(NotImplementedError):
        _natural_algo(which, hidden=1100)


@pytest.mark.parametrize("which", ["npg", "trpo"])
def test_hip_natural_wrapper_runs_with_engine_double(which, monkeypatch):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.npg as NG

    class FakeNPG:
        def __init__(self, obs_dim, act_dim, hidden, actor, critic, cfg):
            assert (obs_dim, act_dim, hidden, cfg.algo) == (17, 6, 64, which) and cfg.optim_critic_iters == 3
            assert (cfg.gamma, cfg.gae_lambda, cfg.damping, cfg.lr) == (0.98, 0.9, 0.1, 1e-3)
            if which == "npg":
                assert cfg.trust_region_size == 0.2
            else:
                assert (cfg.max_kl, cfg.backtrack_coeff, cfg.max_backtracks) == (0.02, 0.7, 8)
            self.obs_dim, self.act_dim, self.hidden, self.cfg = obs_dim, act_dim, hidden, cfg
            self.actor, self.critic = actor.clone(), critic.clone()
            self.critic_m, self.critic_v, self.adam_step = torch.zeros_like(critic), torch.zeros_like(critic), 0
            self.ret_rms = [0.0, 1.0, 0.0]

        def preprocess(self, obs, obs_next, act, rew, term, trunc, cut):
            n = obs.shape[0]
            assert obs.shape == obs_next.shape == (n, 17) and act.shape == (n, 6) and rew.dtype == torch.float64
            z = torch.zeros(n)
            return {"obs": obs, "act": act, "v_s": z, "returns": z, "adv": z, "logp_old": z}

        def update(self, pre, batch_size, repeat, perms):
            assert batch_size == 8 and len(perms) == repeat == 2
            self.adam_step += 9
            self.actor += 1.0
            self.critic += 2.0
            self.critic_m += 0.5
            return torch.tensor([[1.0, 2.0, 3.0, 4.0]] * 6), 6

    algo = _natural_algo(which)
    monkeypatch.setattr("tianshou_amd.integration._require_gpu", lambda device, who: None)
    monkeypatch.setattr(NG, "NPGEngine", FakeNPG)
    monkeypatch.setattr(NG, "layout", lambda o, h, a: {"k0": 32, "actor_count": 33 * h + (h + 1) * h + (h + 1) * 32 + 32,
                                                       "critic_count": 33 * h + (h + 1) * h + (h + 1) * 32})
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (17,), np.zeros((2, 6), np.float32))
    sig = algo.policy.actor.sigma_param
    w1, cw = algo.policy.actor.preprocess.model.model[0].weight, algo.critic.last.model[0].weight
    s0, w0, c0 = sig.detach().clone(), w1.detach().clone(), cw.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, batch_size=8, repeat=2)
    assert (stats.actor_loss.mean, stats.vf_loss.mean, stats.kl.mean) == (1.0, 2.0, 3.0)
    assert (which == "trpo") == hasattr(stats, "step_size") and (which != "trpo" or stats.step_size.mean == 4.0)
    assert torch.allclose(sig.detach(), s0 + 1.0) and torch.allclose(w1.detach(), w0 + 1.0) and torch.allclose(cw.detach(), c0 + 2.0)
    st = algo.optim._optim.state[cw]
    assert float(st["step"]) == 9.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.5))
    assert not algo.optim._optim.state.get(w1)                      # the actor has no optimizer state (natural-gradient steps)


def _reinforce_algo(hidden=64, **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic
    from tianshou_amd import integration as I

    a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[hidden, hidden], activation=torch.nn.Tanh),
                                     action_shape=(6,), unbounded=True)

    def dist_fn(loc_scale):
        return torch.distributions.Independent(torch.distributions.Normal(*loc_scale), 1)

    pol = ProbabilisticActorPolicy(actor=a, dist_fn=dist_fn, action_space=gym.spaces.Box(-1, 1, (6,)))
    return I.make_hip_reinforce()(policy=pol, optim=AdamOptimizerFactory(lr=2e-3), gamma=0.97, return_standardization=True,
                                  device="cpu", **kw)


def test_reinforce_subclass_keeps_signatures_and_fails_loudly():
    ref_shim.install()
    import gymnasium as gym
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step

    algo = _reinforce_algo()
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    assert type(algo).__name__ == "HipReinforce" and base.__name__ == "Reinforce"
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(16, 2)
    _fill(buf, 8, (17,), np.zeros((2, 6), np.float32))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, batch_size=8, repeat=1)
    assert algo._hip_kind == "legacy"
    # round 6: trunks outside Net[h, h] with h a multiple of 32 take the per-layer engine instead of raising; what the engines do
    # not model still raises at construction
    assert _reinforce_algo(hidden=48)._hip_kind == "net"
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic
    from tianshou_amd import integration as I

    def build(optim, net_kw=None, **actor_kw):
        a = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[96, 40, 24], activation=torch.nn.ReLU, **(net_kw or {})),
                                         action_shape=(6,), **actor_kw)
        pol = ProbabilisticActorPolicy(actor=a, dist_fn=_normal_dist, action_space=gym.spaces.Box(-1, 1, (6,)))
        return I.make_hip_reinforce()(policy=pol, optim=optim, gamma=0.97, device="cpu")

    b = build(RMSpropOptimizerFactory(lr=1e-3, eps=1e-5), max_action=1.5)                    # the default (bounded) actor + RMSprop
    assert b._hip_kind == "net" and b._hip_net[:3] == ([96, 40, 24], "relu", 1.5) and b._hip_net[3]["optimizer"] == "rmsprop"
    assert build(AdamOptimizerFactory(lr=1e-3), unbounded=True)._hip_kind == "net"
    with pytest.raises(NotImplementedError):
        build(AdamOptimizerFactory(lr=1e-3), unbounded=True, conditioned_sigma=True)
    ln = build(AdamOptimizerFactory(lr=1e-3), net_kw=dict(norm_layer=torch.nn.LayerNorm, norm_args=dict(eps=1e-4)), unbounded=True)
    assert ln._hip_kind == "net" and ln._hip_ln == 1e-4 and ln._hip_keys[:4] == [                 # LayerNorm trunks (round 6)
        "preprocess.model.model.0.weight", "preprocess.model.model.0.bias", "preprocess.model.model.1.weight", "preprocess.model.model.1.bias"]
    with pytest.raises(NotImplementedError):
        build(AdamOptimizerFactory(lr=1e-3), net_kw=dict(norm_layer=torch.nn.BatchNorm1d), unbounded=True)


def test_hip_reinforce_wrapper_runs_with_engine_double(monkeypatch):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.npg as NG
    import tianshou_amd.reinforce as RF

    class FakeReinforce:
        def __init__(self, obs_dim, act_dim, hidden, actor, cfg):
            assert (obs_dim, act_dim, hidden) == (17, 6, 64)
            assert (cfg.gamma, cfg.return_standardization, cfg.lr) == (0.97, True, 2e-3)
            self.actor, self.cfg = actor.clone(), cfg
            self.adam_m, self.adam_v, self.adam_step = torch.zeros_like(actor), torch.zeros_like(actor), 0
            self.ret_rms = [0.0, 1.0, 0.0]

        def preprocess(self, rew, term, trunc, cut):
            assert rew.dtype == torch.float64 and rew.shape == term.shape == trunc.shape and cut.dtype == torch.int64
            self.ret_rms = [0.25, 2.0, float(rew.numel())]
            return torch.zeros(rew.numel())

        def update(self, obs, act, returns, batch_size, repeat, perms):
            n = obs.shape[0]
            assert obs.shape == (n, 17) and act.shape == (n, 6) and returns.shape == (n,)
            assert batch_size == 8 and len(perms) == repeat == 2
            self.adam_step += 6
            self.actor += 1.0
            self.adam_m += 0.5
            return torch.tensor([[1.0], [3.0]] * 3), 6

    algo = _reinforce_algo()
    monkeypatch.setattr("tianshou_amd.integration._require_gpu", lambda device, who: None)
    monkeypatch.setattr(RF, "ReinforceEngine", FakeReinforce)
    monkeypatch.setattr(NG, "layout", lambda o, h, a: {"k0": 32, "actor_count": 33 * h + (h + 1) * h + (h + 1) * 32 + 32,
                                                       "critic_count": 0})
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (17,), np.zeros((2, 6), np.float32))
    sig, w1 = algo.policy.actor.sigma_param, algo.policy.actor.preprocess.model.model[0].weight
    s0, w0 = sig.detach().clone(), w1.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, batch_size=8, repeat=2)
    assert stats.loss.mean == 2.0
    assert torch.allclose(sig.detach(), s0 + 1.0) and torch.allclose(w1.detach(), w0 + 1.0)
    st = algo.optim._optim.state[w1]
    assert float(st["step"]) == 6.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.5))
    rms = algo.discounted_return_computation.ret_rms
    assert (rms.mean, rms.var, rms.count) == (0.25, 2.0, 24.0)


def _drqn_algo(hidden=64, layers=2, **kw):
    ref_shim.install()
    import gymnasium as gym

    from tianshou.algorithm.modelfree.dqn import DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Recurrent
    from tianshou_amd import integration as I

    net = Recurrent(layer_num=layers, state_shape=(4,), action_shape=2, hidden_layer_size=hidden)
    pol = DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(2))
    return I.make_hip_drqn()(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=0.95, n_step_return_horizon=3,
                             target_update_freq=4, device="cpu", **kw)


def test_drqn_subclass_keeps_signatures_and_fails_loudly(dqn_algo):
    ref_shim.install()
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    from tianshou_amd import integration as I

    algo = _drqn_algo()
    base = type(algo).__mro__[2]            # [1] is the _HipGlue mixin
    assert type(algo).__name__ == "HipDRQN" and base.__name__ == "DQN" and algo._hip_dims == (4, 64, 2, 2)
    for name in ("_preprocess_batch", "_update_with_batch"):
        mine, ref = inspect.signature(getattr(type(algo), name)), inspect.signature(getattr(base, name))
        assert list(mine.parameters) == list(ref.parameters), name
        assert getattr(type(algo), name) is not getattr(base, name)
    buf = VectorReplayBuffer(32, 2, stack_num=4, ignore_obs_next=True)
    _fill(buf, 8, (4,), np.zeros(2, np.int64))
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.update(buffer=buf, sample_size=8)
    with pytest.raises(NotImplementedError):
        _drqn_algo(hidden=48)
    from tianshou.algorithm.optim import AdamOptimizerFactory

    with pytest.raises(NotImplementedError):                  # a DQNet is not a Recurrent model
        I.make_hip_drqn()(policy=dqn_algo.policy, optim=AdamOptimizerFactory(lr=1e-3), device="cpu")


def test_hip_drqn_wrapper_runs_with_engine_double(monkeypatch):
    ref_shim.install()
    from tianshou.algorithm.modelfree.reinforce import SimpleLossTrainingStats
    from tianshou.data import VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.drqn as R

    class FakeDRQN:
        def __init__(self, obs_dim, hidden, layers, n_act, flat, cfg):
            assert (obs_dim, hidden, layers, n_act) == (4, 64, 2, 2)
            assert (cfg.gamma, cfg.n_step, cfg.target_update_freq, cfg.is_double, cfg.lr) == (0.95, 3, 4, True, 1e-3)
            self.params, self.params_old, self.cfg = flat.clone(), flat.clone(), cfg
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

        def preprocess_with_obs(self, m, rows, idx, stack, obs_next_rows=None, prefetch=True):
            assert rows.dtype == torch.float32 and rows.shape[1] == 4 and stack == 4 and obs_next_rows is None and prefetch
            return R.gather_stacked_obs(rows, m, idx, stack), torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret, weight=None):
            assert obs.shape == (8, 4, 4) and act.shape == (8,) and ret.shape == (8,)
            self.adam_step += 1
            self.iter += 1
            self.params += 2.0
            self.params_old += 1.0
            self.adam_v += 0.25
            return torch.tensor([0.75]), torch.arange(8, dtype=torch.float32)

    # the real layout converters run on CPU tensors here: only the engine and the two device gathers are doubles
    def cpu_from_torch(t, obs_dim, hidden, layers, n_act, device="cuda"):
        return real_from(t, obs_dim, hidden, layers, n_act, "cpu")

    real_from = R.flat_from_torch
    algo = _drqn_algo()
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(R, "RecurrentDQNEngine", FakeDRQN)
    monkeypatch.setattr(R, "flat_from_torch", cpu_from_torch)
    monkeypatch.setattr(R, "gather_stacked_obs", lambda rows, m, idx, stack: rows[idx][:, None, :].expand(-1, stack, -1))
    buf = VectorReplayBuffer(32, 2, stack_num=4, ignore_obs_next=True)
    _fill(buf, 12, (4,), np.zeros(2, np.int64))
    w_hh = algo.policy.model.nn.weight_hh_l1
    fc2_b = algo.policy.model.fc2.bias
    old_b = algo.model_old.module.fc2.bias
    w0, b0, o0 = w_hh.detach().clone(), fc2_b.detach().clone(), old_b.detach().clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, SimpleLossTrainingStats) and stats.loss == 0.75
    assert torch.allclose(w_hh.detach(), w0 + 2.0) and torch.allclose(fc2_b.detach(), b0 + 2.0)
    assert torch.allclose(old_b.detach(), o0 + 1.0)
    st = algo.optim._optim.state[w_hh]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.25))


def test_drqn_layout_converters_round_trip_on_cpu():
    from oracle import oracle_drqn as ORQ
    import tianshou_amd.drqn as R

    g = torch.Generator().manual_seed(0)
    for obs_dim, hidden, layers, n_act in [(4, 64, 2, 2), (37, 32, 1, 5), (32, 96, 3, 32)]:
        shapes = ORQ.param_shapes(obs_dim, hidden, layers, n_act)
        keys = ORQ.param_keys(layers)
        assert keys == R.state_dict_keys(layers)
        t = [torch.randn(shapes[k], generator=g) for k in keys]
        flat = R.flat_from_torch(t, obs_dim, hidden, layers, n_act, device="cpu")
        k0 = (obs_dim + 31) // 32 * 32
        assert flat.numel() == (k0 + 1) * hidden + layers * 2 * (hidden + 1) * 4 * hidden + (hidden + 1) * 32
        back = R.flat_to_torch(flat, obs_dim, hidden, layers, n_act)
        assert all(torch.equal(a, b) for a, b in zip(back, t))
        # gate order and transposition: column j of W_ih's block = row j of torch's weight_ih (i, f, g, o stacked)
        off = (k0 + 1) * hidden
        w_ih = flat[off:off + (hidden + 1) * 4 * hidden].reshape(hidden + 1, 4 * hidden)
        assert torch.equal(w_ih[:hidden].t(), t[0]) and torch.equal(w_ih[hidden], t[2])


# ------------------------------------------------------------------------------------ the Q-learning classes' one state path
class _QDouble:
    """What the five Q-learning class bodies (HipDQN, HipDRQN, HipQRDQN / HipC51 / HipDiscreteCQL, HipIQN, HipRainbow) use of
    their engines, on the CPU: every update adds 2 to the parameters, 0.5 to the lagged network's and 0.125 / 0.25 to the two
    Adam moments.  `built` (one list per test, see `_q_body`) collects the engines in the order they were constructed."""

    def __init__(self, *args):                               # four dims, flat[, noise], cfg
        self.c, self.h, self.w, self.n_act, flat = args[:5]
        self.cfg = args[-1]
        self.params, self.params_old = flat.clone(), flat.clone()
        self.adam_m, self.adam_v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.adam_step = self.iter = self.tau_counter = 0
        self.built.append(self)

    def preprocess(self, *a, **k):
        return torch.zeros(8, 1)

    def preprocess_with_obs(self, *a, **k):
        return torch.zeros(8, 1), torch.zeros(8)

    def set_noise(self, *a):
        pass

    def update_with_batch(self, *a, **k):
        self.adam_step += 1
        self.iter += 1
        self.params += 2.0
        self.params_old += 0.5
        self.adam_m += 0.125
        self.adam_v += 0.25
        return torch.tensor([0.5]), torch.arange(8, dtype=torch.float32)


_Q_BODIES = ["dqn", "drqn", "distq", "iqn", "rainbow"]


def _q_body(which, monkeypatch):
    """-> (the algorithm of one class body with a `_QDouble` in place of its engine, a buffer to sample 8 of, the doubles built so
    far, flat vector -> tensors in torch layout by the engine module's own converter)."""
    from tianshou.data import VectorReplayBuffer
    import tianshou_amd.distq as Q
    import tianshou_amd.dqn as D
    import tianshou_amd.drqn as R
    import tianshou_amd.iqn as I
    import tianshou_amd.rainbow as RB

    if which == "iqn":
        from tests import test_iqn_shim as TI

        iqn = TI._classes()[1](TI._iqn_net([512], c=4, h=84, w=84, n_act=6), 6)
    algo, mod, engine, dims = {"dqn": lambda: (_make_dqn_algo(), D, "DQNEngine", (4, 84, 84, 6)),
                               "drqn": lambda: (_drqn_algo(), R, "RecurrentDQNEngine", (4, 64, 2, 2)),
                               "distq": lambda: (_distq_algo("qr"), Q, "DistQEngine", (4, 84, 84, 6, 20)),
                               "iqn": lambda: (iqn, I, "IQNEngine", (4, 84, 84, 6, 64)),
                               "rainbow": lambda: (_rainbow_algo(), RB, "RainbowEngine", (4, 84, 84, 6, 11))}[which]()
    double = type("Double", (_QDouble,), {"built": []})
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(mod, engine, double)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    if which == "drqn":
        buf = VectorReplayBuffer(32, 2, stack_num=4, ignore_obs_next=True)
        _fill(buf, 12, (4,), np.zeros(2, np.int64))
    else:
        buf = VectorReplayBuffer(32, 2)
        _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    return algo, buf, double.built, lambda flat: mod.flat_to_torch(flat, *dims)


@pytest.mark.parametrize("which", _Q_BODIES)
def test_q_engine_rebuilt_from_torch_receives_what_the_last_one_wrote_back(which, monkeypatch):
    """Load and write-back are inverses: after one update, the engine is dropped and built again from the torch modules and
    torch.optim; it starts from the Adam moments, step count, update count and lagged parameters the first one ended with.
    (Compared in torch layout: the padding of a flat vector is not state.)"""
    from tianshou.utils.torch_utils import policy_within_training_step

    algo, buf, built, to_torch = _q_body(which, monkeypatch)
    with policy_within_training_step(algo.policy):
        algo.update(buffer=buf, sample_size=8)
    algo.hip_sync()                                        # (HipDQN writes back when somebody reads; the others already have)
    first = built[0]
    algo._hip_invalidate()
    second = algo._engine() if which == "drqn" else algo._engine(4, 84, 84)
    assert built == [first, second] and second is not first
    assert second.adam_step == first.adam_step == 1 and second.iter == first.iter == 1
    for name, inc in (("params", 2.0), ("params_old", 0.5), ("adam_m", 0.125), ("adam_v", 0.25)):
        a, b = to_torch(getattr(first, name)), to_torch(getattr(second, name))
        assert len(a) == len(b) > 0 and all(torch.equal(x, y.to(x.dtype)) for x, y in zip(a, b)), name
        if name.startswith("adam"):
            assert all(bool((y == inc).all()) for y in b), name           # ... and it is what the update left, not zeros
    old, new = to_torch(second.params_old), to_torch(second.params)
    assert all(torch.allclose(o + 1.5, n) for o, n in zip(old, new))      # the lagged network kept its own values


@pytest.mark.parametrize("which", [w for w in _Q_BODIES if w != "dqn"])
def test_q_write_back_leaves_a_foreign_write_alone(which, monkeypatch):
    """`_hip_write_back` of every Q-learning class goes through `_hip_put`: a parameter somebody else has written since the
    engine snapshotted it (`_hip_skip_ids`, set by the `_hip_engine` property) keeps its value, all others are written."""
    from tianshou.utils.torch_utils import policy_within_training_step

    algo, buf, built, _ = _q_body(which, monkeypatch)
    with policy_within_training_step(algo.policy):
        algo.update(buffer=buf, sample_size=8)
    params = [p for p in algo.policy.model.parameters() if p.requires_grad]      # (RainbowNet's noise is not learnt)
    before = [p.detach().clone() for p in params]
    built[0].params += 1.0
    algo.__dict__["_hip_skip_ids"] = {id(params[1])}
    try:
        algo._hip_write_back()
    finally:
        algo.__dict__["_hip_skip_ids"] = None
    assert torch.equal(params[1].detach(), before[1])
    assert all(torch.allclose(p.detach(), b + 1.0) for i, (p, b) in enumerate(zip(params, before)) if i != 1)


# ------------------------------------------------------------------------------------ the actor-critic classes' one state path
class _ACDouble:
    """What the four off-policy actor-critic class bodies (HipSAC, HipREDQ, HipDiscreteSAC, HipTD3 / HipDDPG / HipTD3BC) use of
    their engines, on the CPU.  `names` (set per body, see `_ac_body`) are the engine's networks, `lagged` those with a `_old` copy.
    Every update adds a constant of its own to each network's parameters, lagged parameters and two Adam moments (`INC` plus the
    network's position / 128: all exact in fp32, all distinct) and to log alpha and its moments, and advances the counters as the
    real engines do.  `built` collects the engines in the order they were constructed."""
    INC = {"": 2.0, "_old": 0.5, "_m": 0.125, "_v": 0.25, "log_alpha": 0.0625, "log_alpha_m": 0.03125, "log_alpha_v": 0.046875}

    def __init__(self, *args, hidden=None, **kw):            # dims (hidden among them for DiscreteSAC), one flat per network, cfg
        flats = [a for a in args if isinstance(a, torch.Tensor)]
        dims = [a for a in args if isinstance(a, int)]
        self.obs_dim, self.act_dim, self.hidden = dims[0], dims[1], hidden if hidden is not None else dims[2]
        self.n_act, self.cfg = self.act_dim, [a for a in args if a is not None][-1]
        assert len(flats) == len(self.names)
        for n, f in zip(self.names, flats):
            setattr(self, n, f.clone())
            setattr(self, n + "_m", torch.zeros_like(f))
            setattr(self, n + "_v", torch.zeros_like(f))
            if n in self.lagged:
                setattr(self, n + "_old", f.clone())
        self.log_alpha, self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1), torch.zeros(1)
        self.adam_step = self.cnt = self.actor_steps = self.critic_gradient_step = 0
        self._stats = torch.zeros(4)
        self.built.append(self)

    @classmethod
    def inc(cls, name, kind):
        return cls.INC[kind] + cls.names.index(name) / 128.0

    def will_update_actor(self):                             # REDQEngine
        return (self.critic_gradient_step + 1) % self.cfg.actor_delay == 0

    def policy_forward(self, obs):                           # DiscreteSACEngine
        return torch.zeros(obs.shape[0], self.n_act)

    def preprocess(self, *a, **k):
        return torch.zeros(8)

    def update_with_batch(self, *a, **k):
        self.adam_step += 1                                  # SACEngine, DiscreteSACEngine
        self.actor_steps += int(self.will_update_actor() if hasattr(self.cfg, "actor_delay") else
                                self.cnt % (self.cfg.update_actor_freq if self.cfg.twin else 1) == 0 if hasattr(self.cfg, "twin") else 0)
        self.critic_gradient_step += 1                       # REDQEngine
        self.cnt += 1                                        # TD3Engine
        for n in self.names:
            for kind in ("", "_m", "_v") + (("_old",) if n in self.lagged else ()):
                self.add(n, kind)
        for n in ("log_alpha", "log_alpha_m", "log_alpha_v"):
            getattr(self, n).add_(self.INC[n])
        return torch.arange(1.0, 6.0), torch.ones(8)

    def add(self, name, kind):
        getattr(self, name + kind).add_(self.inc(name, kind))


_AC_BODIES = ["sac", "dsac", "redq", "td3", "ddpg", "td3bc"]


def _ac_body(which, monkeypatch, double=_ACDouble):
    """-> (the algorithm of one class body with an `_ACDouble` in place of its engine, a buffer to sample 8 of, the doubles built so
    far, per engine network: (flat vector -> tensors in torch layout by the engine module's own converter, the online torch module,
    the lagged one or None, its optimizer, the engine counter that is its step count, whether the optimizer's step is loaded))."""
    from tianshou.data import VectorReplayBuffer
    import tianshou_amd.dsac as DS
    import tianshou_amd.redq as RQ
    import tianshou_amd.returns as R
    import tianshou_amd.sac as S
    import tianshou_amd.td3 as T
    import tianshou_amd.td3bc as TB

    act = np.zeros(2, np.int64) if which == "dsac" else np.zeros((2, 3), np.float32)
    if which == "td3bc":
        from tests import test_td3bc_shim as TT

        if not TT.REAL:
            pytest.skip("reference not mounted")
        algo, mod, engine = TT._make(alpha=1.25), TB, "TD3BCEngine"
    else:
        algo, mod, engine = {"sac": lambda: (_make_sac_algo(), S, "SACEngine"),
                             "dsac": lambda: (_dsac_algo(), DS, "DiscreteSACEngine"),
                             "redq": lambda: (_redq_algo(actor_delay=1), RQ, "REDQEngine"),       # (the actor steps at update 1)
                             "td3": lambda: (_det_algo(True), T, "TD3Engine"),
                             "ddpg": lambda: (_det_algo(False), T, "TD3Engine")}[which]()
    actor = algo.policy.actor
    if which in ("sac", "dsac"):
        conv_a = (lambda f: S.actor_flat_to_torch(f, 11, 3, 256)) if which == "sac" else (lambda f: DS.net_flat_to_torch(f, 11, 5, 64))
        conv_c = (lambda f: S.critic_flat_to_torch(f, 11, 3, 256)) if which == "sac" else conv_a
        nets = {"actor": (conv_a, actor, None, algo.policy_optim, "adam_step", True),
                "critic1": (conv_c, algo.critic, algo.critic_old.module, algo.critic_optim, "adam_step", True),
                "critic2": (conv_c, algo.critic2, algo.critic2_old.module, algo.critic2_optim, "adam_step", True)}
    elif which == "redq":
        nets = {"actor": (lambda f: S.actor_flat_to_torch(f, 11, 3, 256), actor, None, algo.policy_optim, "actor_steps", True),
                "critics": (lambda f: RQ.ensemble_flat_to_torch(f, 4, 11, 3, 256), algo.critic, algo.critic_old.module, algo.critic_optim,
                            "critic_gradient_step", False)}
    else:
        conv_c = lambda f: T.critic_flat_to_torch(f, 11, 3, 256)   # noqa: E731
        nets = {"actor": (lambda f: T.actor_flat_to_torch(f, 11, 3, 256), actor, algo.actor_old.module, algo.policy_optim, "actor_steps", True),
                "critic1": (conv_c, algo.critic, algo.critic_old.module, algo.critic_optim, "cnt", False)}
        if which != "ddpg":
            nets["critic2"] = (conv_c, algo.critic2, algo.critic2_old.module, algo.critic2_optim, "cnt", False)
    double = type("Double", (double,), {"built": [], "names": tuple(nets), "lagged": tuple(n for n, v in nets.items() if v[2] is not None)})
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(mod, engine, double)
    monkeypatch.setattr(DS, "layout", lambda o, a, h, d=2: {"ka": 32, "hw": 32, "count": 33 * h + (h + 1) * h + (h + 1) * 32,
                                                             "offs": [0, 33 * h, 33 * h + (h + 1) * h, 33 * h + (h + 1) * h + (h + 1) * 32]})
    monkeypatch.setattr(R, "nstep_indices", lambda m, idx, n: idx)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (11,), act)
    return algo, buf, double.built, nets


def _ac_update(algo, buf):
    from tianshou.utils.torch_utils import policy_within_training_step

    with policy_within_training_step(algo.policy):
        algo.update(buffer=buf, sample_size=8)
    algo.hip_sync()                                        # (HipSAC writes back when somebody reads; the others already have)


@pytest.mark.parametrize("which", _AC_BODIES)
def test_ac_engine_rebuilt_from_torch_receives_what_the_last_one_wrote_back(which, monkeypatch):
    """Load and write-back are inverses: after one update, the engine is dropped and built again from the torch modules and
    torch.optim; it starts from the parameters, lagged parameters, Adam moments, step counts and log alpha moments the first one
    ended with.  (Compared in torch layout: the padding of a flat vector is not state.)"""
    algo, buf, built, nets = _ac_body(which, monkeypatch)
    _ac_update(algo, buf)
    first = built[0]
    algo._hip_invalidate()
    second = algo._engine()
    assert built == [first, second] and second is not first
    for name, (to_torch, _, old, _, counter, loaded) in nets.items():
        assert getattr(second, counter) == getattr(first, counter) == 1, (name, counter)       # (the critics': by the algorithm)
        for kind in ("", "_m", "_v") + (("_old",) if old is not None else ()):
            a, b = to_torch(getattr(first, name + kind)), to_torch(getattr(second, name + kind))
            assert len(a) == len(b) > 0 and all(torch.equal(x, y.to(x.dtype)) for x, y in zip(a, b)), (name, kind)
            if kind in ("_m", "_v"):
                assert all(bool((y == first.inc(name, kind)).all()) for y in b), (name, kind)  # ... what the update left, not zeros
        if old is not None:                                                   # the lagged network kept its own values
            assert all(torch.allclose(o + 1.5, n) for o, n in zip(to_torch(getattr(second, name + "_old")), to_torch(getattr(second, name))))
    if which in ("sac", "dsac", "redq"):
        assert second.cfg.auto_alpha and float(second.cfg.log_alpha0) == float(first.log_alpha) == 0.0625
        assert (float(second.log_alpha_m), float(second.log_alpha_v)) == (0.03125, 0.046875)


@pytest.mark.parametrize("which", _AC_BODIES)
def test_ac_write_back_leaves_a_foreign_write_alone(which, monkeypatch):
    """`_hip_write_back` of every actor-critic class goes through `_hip_put`: a parameter somebody else has written since the
    engine snapshotted it (`_hip_skip_ids`, set by the `_hip_engine` property) keeps its value, online or lagged; all others,
    of every module, are written."""
    algo, buf, built, nets = _ac_body(which, monkeypatch)
    _ac_update(algo, buf)
    mods = [m for _, m, old, _, _, _ in nets.values() for m in (m, old) if m is not None]
    params = [p for m in mods for p in m.parameters()]
    before = [p.detach().clone() for p in params]
    for name, (_, _, old, _, _, _) in nets.items():
        getattr(built[0], name).add_(1.0)
        if old is not None:
            getattr(built[0], name + "_old").add_(1.0)
    last = list(nets.values())[-1]                         # a critic: it has a lagged copy in every body
    skip = {id(list(last[1].parameters())[1]), id(list(last[2].parameters())[0])}
    algo.__dict__["_hip_skip_ids"] = skip
    try:
        algo._hip_write_back()
    finally:
        algo.__dict__["_hip_skip_ids"] = None
    assert sum(id(p) in skip for p in params) == 2
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b) if id(p) in skip else torch.allclose(p.detach(), b + 1.0)


def test_ac_write_back_follows_key_order_not_definition_order(monkeypatch):
    """HipSAC's write-back pairs the converters' tensors, which come in `keys` order, with the parameters of those names, for
    the parameters as for the Adam state: an update that moves the k-th tensor (in key order) of every network by k + 1 is found
    under the k-th key, in whatever order the module defines its parameters."""
    import tianshou_amd.sac as S

    class ByPosition(_ACDouble):
        def add(self, name, kind):
            back = S.actor_flat_to_torch if name == "actor" else S.critic_flat_to_torch
            fwd = S.actor_flat_from_torch if name == "actor" else S.critic_flat_from_torch
            t = back(getattr(self, name + kind), 11, 3, 256)
            setattr(self, name + kind, fwd([x + (k + 1) for k, x in enumerate(t)], 11, 3, "cpu", hidden=256))

    algo, buf, built, nets = _ac_body("sac", monkeypatch, ByPosition)
    mods = {"actor": algo.policy.actor, "critic1": algo.critic, "critic2": algo.critic2}
    keys = {"actor": S.actor_keys(2), "critic1": S.critic_keys(2), "critic2": S.critic_keys(2)}
    # definition order is NOT key order here: the heads come first in the modules' own parameter lists
    for m in mods.values():
        m._modules["preprocess"] = m._modules.pop("preprocess")
        assert [k for k, _ in m.named_parameters()][0].split(".")[0] != "preprocess"
    before = {n: {k: p.detach().clone() for k, p in m.named_parameters()} for n, m in mods.items()}
    _ac_update(algo, buf)
    for n, m in mods.items():
        named = dict(m.named_parameters())
        for k, key in enumerate(keys[n]):
            assert torch.allclose(named[key].detach(), before[n][key] + (k + 1)), (n, key)
            st = nets[n][3]._optim.state[named[key]]
            assert bool((st["exp_avg"] == k + 1).all()) and bool((st["exp_avg_sq"] == k + 1).all()), (n, key)


# ------------------------------------------------------------------------------------ the on-policy classes' one state path
class _OnDouble:
    """What the five on-policy class bodies (HipPPO / HipA2C, HipNPG / HipTRPO, HipReinforce, HipPPOCnn / HipA2CCnn,
    HipPPODiscrete / HipA2CDiscrete) use of their engines, on the CPU.  `vectors` (set per body, see `_on_body`) are the engine's
    parameter vectors in constructor order, `moments` the two optimizer-state vectors, which belong to the last of them.  Every
    update adds 2 to the parameters, 0.125 / 0.25 to the two moments and 1 to the step count; preprocessing moves the return
    statistics to `RMS`, as the engines' does.  `built` collects the engines in the order they were constructed."""
    RMS = [0.5, 2.0, 7.0]
    INC = (0.125, 0.25)

    def __init__(self, *args, **kw):                         # dims (c, h, w first for the CNN), one flat per vector, cfg
        flats = [a for a in args if isinstance(a, torch.Tensor)]
        self.c, self.h, self.w = args[:3]
        self.cfg = args[-1]
        assert len(flats) == len(self.vectors)
        for n, f in zip(self.vectors, flats):
            setattr(self, n, f.clone())
        for n in self.moments:
            setattr(self, n, torch.zeros_like(flats[-1]))
        self.adam_step, self.ret_rms = 0, [0.0, 1.0, 0.0]
        self.built.append(self)

    def preprocess(self, first, *a, **k):                    # `first`: observations, rewards or the device mirror
        self.ret_rms = list(self.RMS)
        z = torch.zeros(len(first))
        return z if self.vectors == ("actor",) else {"obs": first, "act": z, "v_s": z, "returns": z, "adv": z, "logp_old": z}

    def update(self, *a, **k):
        self.adam_step += 1
        for n in self.vectors:
            getattr(self, n).add_(2.0)
        for n, inc in zip(self.moments, self.INC):
            getattr(self, n).add_(inc)
        return torch.tensor([[4.0, 3.0, 2.0, 1.0]])[:, :1 if self.vectors == ("actor",) else 4], 1

    def check(self):
        pass


_ON_BODIES = ["ppo", "npg", "trpo", "reinforce_ln_rmsprop", "ppo_cnn", "ppo_discrete"]


def _cpu_sample_all(self, batch_size):
    """DeviceReplayBuffer.sample_indices(0) without its kernel."""
    return torch.as_tensor(np.concatenate([
        self.h_offset[e] + (np.arange(self.h_lengths[e]) if self.h_lengths[e] < (self.h_offset[e + 1] - self.h_offset[e])
                            else (self.h_insertion[e] + np.arange(self.h_lengths[e])) % self.h_lengths[e])
        for e in range(self.buffer_num)]).astype(np.int64))


def _cpu_cuts(m, idx):
    """returns.cut_positions without its kernel."""
    unf = [int(m.h_last_index[e]) for e in range(m.buffer_num) if m.h_lengths[e] > 0 and not bool(m.done[m.h_last_index[e]])]
    pos = np.nonzero(np.isin(idx.numpy(), unf))[0]
    return torch.as_tensor(pos), torch.tensor([len(pos)])


def _reinforce_ln_rmsprop_algo():
    """HipReinforce on the per-layer engine: a LayerNorm trunk of unequal widths under RMSprop with momentum (its first state
    vector is the momentum buffer)."""
    import gymnasium as gym
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import RMSpropOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic
    from tianshou_amd import integration as I

    net = Net(state_shape=(17,), hidden_sizes=[48, 40], activation=torch.nn.ReLU, norm_layer=torch.nn.LayerNorm)
    a = ContinuousActorProbabilistic(preprocess_net=net, action_shape=(6,), unbounded=True)
    pol = ProbabilisticActorPolicy(actor=a, dist_fn=_normal_dist, action_space=gym.spaces.Box(-1, 1, (6,)))
    return I.make_hip_reinforce()(policy=pol, optim=RMSpropOptimizerFactory(lr=1e-3, eps=1e-5, momentum=0.9), gamma=0.97, device="cpu")


def _on_body(which, monkeypatch):
    """-> (the algorithm of one class body with an `_OnDouble` in place of its engine, a buffer, the doubles built so far, the
    names of the optimizer's two state tensors, per engine vector: (flat vector -> tensors in torch layout by the engine module's
    own converter, the torch parameters it maps to, whether the optimizer holds them)); `rebuild(algo)` builds the engine again."""
    from tianshou.data import VectorReplayBuffer
    import tianshou_amd.buffer as B
    import tianshou_amd.integration as I
    import tianshou_amd.npg as NG
    import tianshou_amd.ppo_cnn as PC
    import tianshou_amd.ppo_discrete as PD
    import tianshou_amd.ppo_wide as PW
    import tianshou_amd.reinforce as RF
    import tianshou_amd.returns as R
    from tianshou_amd.checkpoint import params_by_keys

    lay = lambda o, h, a: {"k0": 32, "head": 32, "actor_count": 33 * h + (h + 1) * h + (h + 1) * 32 + 32,       # noqa: E731
                           "critic_count": 33 * h + (h + 1) * h + (h + 1) * 32, "count": 33 * h + (h + 1) * h + (h + 1) * 32}
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(NG, "layout", lay)
    monkeypatch.setattr(PD, "layout", lay)
    monkeypatch.setattr(B.DeviceReplayBuffer, "sample_indices", _cpu_sample_all)
    monkeypatch.setattr(R, "cut_positions", _cpu_cuts)
    obs, act, dtype, state = (17,), np.zeros((2, 6), np.float32), np.float32, ("exp_avg", "exp_avg_sq")
    if which == "ppo":
        algo, mod, engine = _make_ppo_algo(), I, "PPOEngine"
        sizes = [p.numel() for p in algo._hip_params()]                           # (the fused layout is the tensors end to end)
        nets = {"params": (lambda f: torch.split(f, sizes), algo._hip_params(), True)}
    elif which in ("npg", "trpo"):
        algo, mod, engine = _natural_algo(which), NG, "NPGEngine"
        nets = {"actor": (lambda f: NG.actor_flat_to_torch(f, 17, 64, 6), params_by_keys(algo.policy.actor, algo._hip_akeys), False),
                "critic": (lambda f: NG.critic_flat_to_torch(f, 17, 64), params_by_keys(algo.critic, algo._hip_ckeys), True)}
    elif which == "reinforce_ln_rmsprop":
        algo, mod, engine, state = _reinforce_ln_rmsprop_algo(), RF, "NetReinforceEngine", ("momentum_buffer", "square_avg")
        nets = {"actor": (lambda f: PW.net_flat_to_tensors(f, 17, [48, 40], 6, True, layer_norm=True),
                          params_by_keys(algo.policy.actor, algo._hip_keys), True)}
    elif which == "ppo_cnn":
        algo, mod, engine, obs, act, dtype = _ppo_cnn_algo(), PC, "CnnPPOEngine", (4, 84, 84), np.zeros(2, np.int64), np.uint8
        nets = {"params": (lambda f: PC.flat_to_torch(f, 4, 84, 84, 6), algo._hip_params(), True)}
    else:
        algo, mod, engine, obs, act = _ppo_discrete_algo(), PD, "DiscretePPOEngine", (4,), np.zeros(2, np.int64)
        nets = {"params": (lambda f: PD.flat_to_torch(f, 4, 64, 2), algo._hip_params(), True)}
    double = type("Double", (_OnDouble,), {"built": [], "vectors": tuple(nets),
                                           "moments": ("critic_m", "critic_v") if "critic" in nets else ("adam_m", "adam_v")})
    monkeypatch.setattr(mod, engine, double)
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, obs, act, dtype)
    return algo, buf, double.built, state, nets, (lambda a: a._engine(4, 84, 84) if which == "ppo_cnn" else a._engine())


def _on_update(algo, buf):
    from tianshou.utils.torch_utils import policy_within_training_step

    with policy_within_training_step(algo.policy):
        return algo.update(buffer=buf, batch_size=8, repeat=2)


@pytest.mark.parametrize("which", _ON_BODIES)
def test_on_policy_engine_rebuilt_from_torch_receives_what_the_last_one_wrote_back(which, monkeypatch):
    """Load and write-back are inverses: after one update and a `state_dict()` (HipPPO's optimizer state moves there), the engine
    is dropped and built again from the torch modules and torch.optim; it starts from the parameters, optimizer moments, step
    count and return statistics the first one ended with.  The NPG / TRPO actor has no optimizer: its part carries no moments,
    the critic's does.  (Compared in torch layout: the padding of a flat vector is not state.)"""
    algo, buf, built, _, nets, rebuild = _on_body(which, monkeypatch)
    _on_update(algo, buf)
    algo.state_dict()
    first = built[0]
    algo._hip_invalidate()
    second = rebuild(algo)
    assert built == [first, second] and second is not first
    assert second.adam_step == first.adam_step == 1 and second.ret_rms == first.ret_rms == _OnDouble.RMS
    for name, (to_torch, params, _) in nets.items():
        a, b = to_torch(getattr(first, name)), to_torch(getattr(second, name))
        assert len(a) == len(b) > 0 and all(torch.equal(x, y) for x, y in zip(a, b)), name
        assert len(params) == len(b) and all(torch.equal(p.detach().reshape(-1), y.reshape(-1)) for p, y in zip(params, b)), name
    to_torch = list(nets.values())[-1][0]                                     # the vector the optimizer holds
    for name, inc in zip(first.moments, _OnDouble.INC):
        a, b = to_torch(getattr(first, name)), to_torch(getattr(second, name))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), name
        assert all(bool((y == inc).all()) for y in b), name                   # ... and it is what the update left, not zeros
    parts = algo._hip_parts(second)
    assert [p.name for p in parts] == list(nets) and [p.moments for p in parts if p.moments] == [first.moments]
    assert [p.moments is not None for p in parts] == [held for _, _, held in nets.values()]


@pytest.mark.parametrize("which", _ON_BODIES)
def test_on_policy_write_back_leaves_a_foreign_write_alone(which, monkeypatch):
    """`_hip_write_back` of every on-policy class goes through `_hip_put`: a parameter somebody else has written since the engine
    snapshotted it (`_hip_skip_ids`, set by the `_hip_engine` property) keeps its value, all others, of every module, are written."""
    algo, buf, built, _, nets, _ = _on_body(which, monkeypatch)
    _on_update(algo, buf)
    params = [p for _, ps, _ in nets.values() for p in ps]
    before = [p.detach().clone() for p in params]
    for name in nets:
        getattr(built[0], name).add_(1.0)
    algo.__dict__["_hip_skip_ids"] = {id(params[1])}
    try:
        algo._hip_write_back()
    finally:
        algo.__dict__["_hip_skip_ids"] = None
    assert torch.equal(params[1].detach(), before[1])
    assert all(torch.allclose(p.detach(), b + 1.0) for i, (p, b) in enumerate(zip(params, before)) if i != 1)


@pytest.mark.parametrize("which", _ON_BODIES)
def test_on_policy_optimizer_state_arrives_with_the_update_except_for_hip_ppo(which, monkeypatch):
    """After an update and before any reader the four eager bodies hold the optimizer's state of step 1 in torch.optim; HipPPO's
    torch.optim is still what it was (empty) and receives the same state at `state_dict()` (`_hip_flush`)."""
    algo, buf, built, (k_m, k_v), nets, _ = _on_body(which, monkeypatch)
    opt = algo.optim._optim
    held = [p for _, ps, h in nets.values() if h for p in ps]
    assert held and not opt.state
    _on_update(algo, buf)
    if which == "ppo":
        assert not opt.state and all(p not in opt.state for p in held)
        algo.state_dict()
    assert set(opt.state) == set(held)
    for p in held:
        st = opt.state[p]
        assert float(st["step"]) == 1.0 and bool((st[k_m] == 0.125).all()) and bool((st[k_v] == 0.25).all())


def test_device_permutation_key_follows_numpy_seed_and_travels_in_the_checkpoint():
    """permutations="device" (HipPPO's default): the shuffle key is one draw from NumPy's global generator at construction
    -- `np.random.seed` selects it like it selects Batch.split's permutations in the reference -- and (seed, update counter)
    are part of state_dict(), so a resumed run continues the sequence; a checkpoint of the reference class (no such key)
    still loads; "host" mode leaves the generator untouched."""
    ref_shim.install()
    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.ppo import PPO
    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_ppo

    def build(cls, **kw):
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                             action_shape=(6,), unbounded=True)
        critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
        policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=True,
                                          action_bound_method="clip", action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
        return cls(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), **kw)

    HipPPO = make_hip_ppo()
    np.random.seed(5)
    a = build(HipPPO, device="cpu")
    np.random.seed(5)
    b = build(HipPPO, device="cpu")
    np.random.seed(6)
    c = build(HipPPO, device="cpu")
    assert a._hip_perm_seed == b._hip_perm_seed != c._hip_perm_seed
    assert build(HipPPO, device="cpu", perm_seed=11)._hip_perm_seed == 11
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    build(HipPPO, device="cpu", permutations="host")
    assert np.array_equal(before, np.random.get_state()[1])            # the reference's stream is not consumed
    a._hip_updates = 7
    sd = a.state_dict()
    ref = build(PPO)
    assert set(sd) == set(ref.state_dict())                            # the reference's checkpoint format, nothing added
    ref.load_state_dict(dict(sd), strict=True)                         # a HipPPO checkpoint loads into the reference class
    c.load_state_dict(dict(sd))                                        # (the reference's load pops `_optimizers`: copies)
    c.load_hip_extra_state(a.hip_extra_state())
    assert (c._hip_perm_seed, c._hip_updates) == (a._hip_perm_seed, 7)
    legacy = dict(sd); legacy["_hip_perm_state"] = torch.tensor([3, 9])  # round-4 checkpoints carried the pair inline
    c.load_state_dict(legacy)
    assert (c._hip_perm_seed, c._hip_updates) == (3, 9)
    c.load_hip_extra_state(a.hip_extra_state())
    ref_sd = build(PPO).state_dict()
    c.load_state_dict(ref_sd)                                          # a checkpoint written by the reference class
    assert (c._hip_perm_seed, c._hip_updates) == (a._hip_perm_seed, 7)


def test_off_policy_hooks_refuse_activations_the_engine_does_not_compute():
    """The state_dict keys of Net(hidden_sizes=[h, h], activation=X) are the same for every X: the off-policy hooks look at the
    modules -- nn.ReLU (Net's default) and nn.Tanh are computed, anything else raises instead of silently becoming ReLU."""
    ref_shim.install()
    import gymnasium as gym
    from torch import nn

    from tianshou.algorithm.modelfree.sac import SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou_amd.integration import make_hip_sac

    def build(act_cls, **kw):
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(11,), hidden_sizes=[64, 64, 32], activation=act_cls),
                                             action_shape=(3,), conditioned_sigma=True, **kw)
        mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(11,), action_shape=(3,), hidden_sizes=[48, 64, 64],  # noqa: E731
                                                         concat=True, activation=act_cls))
        policy = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(3,)))
        return make_hip_sac()(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(),
                              critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3),
                              device="cpu")

    a = build(nn.Tanh, unbounded=True)
    assert (a._hip_depth, a._hip_actfn, a._hip_bound, a._hip_hidden) == (3, "tanh", 0.0, 64)
    b = build(nn.ReLU, max_action=2.0)                        # the class default: unbounded=False
    assert (b._hip_actfn, b._hip_bound) == ("relu", 2.0) and b.policy._hip_spec["max_action"] == 2.0
    with pytest.raises(NotImplementedError, match="nn.ReLU or nn.Tanh"):
        build(nn.ELU, unbounded=True)


def test_hip_sac_one_call_update_on_the_real_reference_classes(monkeypatch):
    """Round 6: HipSAC.update() on tianshou's OWN SAC / SACPolicy / PrioritizedVectorReplayBuffer with an engine double (CPU: no
    kernel runs).  With the defaults the two hooks of an n_step = 1 update make ONE engine call (`learn_rows`: ts_sac_learn_rows) --
    on the indices `buffer.sample_indices` drew, with the importance weights `PrioritizedReplayBuffer.__getitem__` would attach
    (prio.py:69-79, 103-106), the two rsample() draws' counters in order -- and `_postprocess_batch` hands the engine's TD weights
    to `buffer.update_weight` (prio.py:81-100).  With torch's noise (`update_noise="torch"`) the hooks stay two calls."""
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.sac import AutoAlpha, SACPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.integration as I

    monkeypatch.setattr(I, "_require_gpu", lambda device, who: None)
    obs_dim, act_dim, B = 11, 3, 8

    class Cfg:
        n_step, auto_alpha = 1, True

    class Engine:                                     # the interface of tianshou_amd.sac.SACEngine the hooks use
        cfg, act_dim = Cfg(), 3

        def __init__(self):
            self.calls = []

        def _rows_ok(self, m):
            return True

        def learn_rows(self, m, idx, noise=None, noise_key=None, weight=None, lr_scale=1.0, noise_streams=1):
            self.calls.append(("learn_rows", idx.clone(), noise_key, None if weight is None else np.asarray(weight).copy(), noise_streams))
            n = idx.numel()
            return torch.arange(5.0), torch.linspace(0.5, 1.5, n), torch.full((n,), 7.0), None

        def preprocess(self, m, idx, noise):
            self.calls.append(("preprocess", idx.clone(), tuple(noise.shape)))
            return torch.full((idx.numel(),), 7.0)

        def update_with_rows(self, m, idx, returns, noise, weight=None, lr_scale=1.0):
            self.calls.append(("update_with_rows", idx.clone(), tuple(noise.shape)))
            return torch.arange(5.0), torch.linspace(0.5, 1.5, idx.numel())

    def build(**kw):
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(obs_dim,), hidden_sizes=[256, 256]), action_shape=(act_dim,),
                                             unbounded=True, conditioned_sigma=True)
        mk = lambda: ContinuousCritic(preprocess_net=Net(state_shape=(obs_dim,), action_shape=(act_dim,), hidden_sizes=[256, 256],  # noqa: E731
                                                         concat=True))
        policy = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(act_dim,)))
        algo = I.make_hip_sac()(policy=policy, policy_optim=AdamOptimizerFactory(lr=1e-3), critic=mk(),
                                critic_optim=AdamOptimizerFactory(lr=1e-3), critic2=mk(), critic2_optim=AdamOptimizerFactory(lr=1e-3),
                                alpha=AutoAlpha(-3.0, 0.0, AdamOptimizerFactory(lr=3e-4)), device="cpu", policy_forward="torch",
                                write_back="lazy", noise_seed=5, **kw)
        algo._hip_engine = Engine()
        return algo

    def buffer():
        buf = PrioritizedVectorReplayBuffer(32, 2, alpha=0.6, beta=0.4)
        rng = np.random.default_rng(1)
        for _ in range(12):
            buf.add(Batch(obs=rng.normal(size=(2, obs_dim)).astype(np.float32), act=rng.normal(size=(2, act_dim)).astype(np.float32),
                          rew=rng.normal(size=2), terminated=np.zeros(2, bool), truncated=np.zeros(2, bool),
                          obs_next=rng.normal(size=(2, obs_dim)).astype(np.float32)))
        buf.update_weight(np.arange(6), np.linspace(0.1, 2.0, 6))           # uneven priorities: the weights are not all 1
        return buf

    algo, buf = build(), buffer()
    drawn = []
    orig = buf.sample_indices
    monkeypatch.setattr(buf, "sample_indices", lambda n: (drawn.append(orig(n)), drawn[-1])[1])
    with policy_within_training_step(algo.policy):
        for _ in range(2):
            stats = algo.update(buffer=buf, sample_size=B)
    calls = algo._hip_engine.calls
    assert [c[0] for c in calls] == ["learn_rows", "learn_rows"]
    key = 5 ^ 0x5AC
    for u, c in enumerate(calls):
        assert np.array_equal(c[1].numpy(), drawn[u])
        assert c[2] == (key, 2 * u + 1) and c[4] == 2                       # target draw 2u + 1, update draw 2u + 2
    w0 = buffer().get_weight(drawn[0])                                      # (a fresh buffer: update 0 has rewritten these priorities)
    np.testing.assert_allclose(calls[0][3], w0 / np.max(w0))
    assert (stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.alpha, stats.alpha_loss) == (0.0, 1.0, 2.0, 3.0, 4.0)
    eps = np.finfo(np.float32).eps.item()                                  # prio.py:81-94: (|w| + eps) ** alpha
    last = {int(i): k for k, i in enumerate(drawn[1])}                      # (an index drawn twice keeps its last weight)
    np.testing.assert_allclose(buf.weight[np.array(list(last))], (np.linspace(0.5, 1.5, B)[list(last.values())] + eps) ** 0.6, rtol=1e-6)
    assert algo.__dict__["_hip_stale"]                                     # lazy write-back: nothing touched the torch modules

    two, buf2 = build(update_noise="torch"), buffer()
    with policy_within_training_step(two.policy):
        two.update(buffer=buf2, sample_size=B)
    assert [c[0] for c in two._hip_engine.calls] == ["preprocess", "update_with_rows"]
    assert two._hip_engine.calls[0][2] == (B, act_dim) and two._hip_engine.calls[1][2] == (B, act_dim)


# ------------------------------------------------------------------------------------ lazy write-back: state coherence (CPU doubles)
# The CPU versions of tests/test_gpu_lazy_state.py's regressions: what a reader, `hip_invalidate()` and a checkpoint restore see
# after lazy updates, on the real reference classes with the engine doubles above.
def _lazy_twin(which, monkeypatch):
    """-> (algorithm with the defaults: lazy write-back, index-only sampling; its buffer)."""
    from tianshou.data import VectorReplayBuffer
    import tianshou_amd.dqn as D
    import tianshou_amd.sac as S

    _patch_for_cpu(monkeypatch)
    buf = VectorReplayBuffer(32, 2)
    if which == "dqn":
        monkeypatch.setattr(D, "DQNEngine", _FakeDQN)
        monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
        _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
        algo = _make_dqn_algo()
    else:
        monkeypatch.setattr(S, "SACEngine", _FakeSAC)
        _fill(buf, 12, (11,), np.zeros((2, 3), np.float32))
        algo = _make_sac_algo()
    assert algo.__dict__["_hip_lazy"]
    return algo, buf


def _run_updates(algo, buf, k):
    from tianshou.utils.torch_utils import policy_within_training_step

    with policy_within_training_step(algo.policy):
        for _ in range(k):
            algo.update(buffer=buf, sample_size=8)


def _values(mod):
    return [p.detach().clone() for p in mod.parameters()]


_READERS = {
    "algorithm_state_dict": lambda algo, mod: algo.state_dict(),
    "policy_state_dict": lambda algo, mod: algo.policy.state_dict(),
    "module_state_dict": lambda algo, mod: mod.state_dict(),
    # (`copy.deepcopy` goes through the policy's `__reduce__` as pickling does; the shimmed gymnasium spaces are local classes)
    "copy_policy": lambda algo, mod: __import__("copy").deepcopy(algo.policy),
    "hip_sync": lambda algo, mod: algo.hip_sync(),
}


@pytest.mark.parametrize("reader", list(_READERS))
@pytest.mark.parametrize("which", ["dqn", "sac"])
def test_foreign_load_then_a_reader_keeps_what_was_loaded(which, reader, monkeypatch):
    """Lazy updates pending, `load_state_dict(best)` on a sub-module, then a reader with no update in between: the loaded module
    holds exactly `best`, every other module and the optimizer state hold what the engine learnt, and the next update continues
    from `best` -- what eager write-back shows.  (Before: the reader wrote the engine's weights over the loaded ones.)"""
    algo, buf = _lazy_twin(which, monkeypatch)
    if which == "dqn":
        mod, learner, lagged, opt = algo.policy.model, None, algo.model_old, algo.optim._optim
        first = next(iter(mod.parameters()))
    else:
        mod, learner, lagged, opt = algo.critic, algo.policy.actor, algo.critic_old.module, algo.policy_optim._optim
        first = next(iter(learner.parameters()))
    learner0, lagged0 = (_values(learner) if learner is not None else None), _values(lagged)
    _run_updates(algo, buf, 2)
    best = {k: torch.full_like(v, 7.0) for k, v in mod.named_parameters()}       # (mod.state_dict() would be a reader)
    mod.load_state_dict(best)
    assert algo.__dict__["_hip_stale"]                               # updates still pending
    _READERS[reader](algo, mod)
    assert not algo.__dict__["_hip_stale"]
    assert all(torch.equal(v, best[k]) for k, v in mod.state_dict().items())
    lag = 0.5 if which == "dqn" else 0.125
    assert all(torch.allclose(p, p0 + 2 * lag) for p, p0 in zip(_values(lagged), lagged0))      # the lagged network: learnt
    st = opt.state[first]
    assert float(st["step"]) == 2.0
    if which == "dqn":
        assert torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.5))
    else:
        assert all(torch.allclose(p, p0 + 2.0) for p, p0 in zip(_values(learner), learner0))
        assert torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 1.0))
        assert abs(float(algo.alpha._log_alpha) - 0.5) < 1e-6
    _run_updates(algo, buf, 1)                                       # continues from `best` and from the learnt optimizer state
    algo.hip_sync()
    assert float(opt.state[first]["step"]) == 3.0
    if which == "dqn":
        assert all(torch.allclose(p, torch.full_like(p, 9.0)) for p in mod.parameters())
    else:
        assert all(torch.equal(v, best[k]) for k, v in mod.state_dict().items())
        assert all(torch.allclose(p, p0 + 3.0) for p, p0 in zip(_values(learner), learner0))


def test_hip_invalidate_with_updates_pending_raises_and_loses_nothing(monkeypatch):
    """`hip_invalidate()` cannot tell a `.data` edit from the updates the engine still holds: with lazy updates pending it raises
    and drops nothing.  `hip_sync()` then `hip_invalidate()` equals eager write-back's `hip_invalidate()`, and so does the next
    update (rebuilt from the torch state: parameters and Adam state continue)."""
    algo, buf = _lazy_twin("dqn", monkeypatch)
    first = next(iter(algo.policy.model.parameters()))
    before = first.detach().clone()
    _run_updates(algo, buf, 2)
    eng = algo.__dict__["_hip_engine_obj"]
    with pytest.raises(RuntimeError, match="hip_sync"):
        algo.hip_invalidate()
    assert algo.__dict__["_hip_engine_obj"] is eng and algo.__dict__["_hip_stale"]            # nothing was dropped
    assert torch.equal(first.detach(), before)
    algo.hip_sync()
    assert torch.allclose(first.detach(), before + 4.0)
    algo.hip_invalidate()                                            # nothing pending now: drops the engine
    assert algo.__dict__["_hip_engine_obj"] is None and torch.allclose(first.detach(), before + 4.0)
    st = algo.optim._optim.state[first]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.5))
    _run_updates(algo, buf, 1)
    assert algo.__dict__["_hip_engine_obj"] is not eng
    algo.hip_sync()
    st = algo.optim._optim.state[first]
    assert torch.allclose(first.detach(), before + 6.0)
    assert float(st["step"]) == 3.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.75))


def test_hip_invalidate_without_the_optimizer_keeps_the_optimizer_state_the_caller_loaded(monkeypatch):
    """`hip_invalidate(keep_optimizer=False)` after the caller replaced parameters (a sub-module load) AND the optimizer state:
    nothing of the engine is written into torch.optim -- neither by the drop nor by the version check of the load.  With lazy
    updates pending it raises without writing anything; after `hip_sync()` first, the caller's state is what the next update
    starts from."""
    algo, buf = _lazy_twin("dqn", monkeypatch)
    model, opt = algo.policy.model, algo.optim._optim
    sevens = {k: torch.full_like(v, 7.0) for k, v in model.named_parameters()}
    _run_updates(algo, buf, 2)
    model.load_state_dict(sevens)                                    # (no sync first: updates are pending)
    opt.state.clear()
    with pytest.raises(RuntimeError, match="hip_sync"):
        algo.hip_invalidate(keep_optimizer=False)
    assert not opt.state and all(torch.equal(p.detach(), sevens[k]) for k, p in model.named_parameters())   # nothing written
    algo, buf = _lazy_twin("dqn", monkeypatch)                       # the recipe: hip_sync() before replacing the state
    model, opt = algo.policy.model, algo.optim._optim
    first = next(iter(model.parameters()))
    old_before = _values(algo.model_old)
    _run_updates(algo, buf, 2)
    algo.hip_sync()
    model.load_state_dict(sevens)
    opt.state.clear()
    algo.hip_invalidate(keep_optimizer=False)
    assert algo.__dict__["_hip_engine_obj"] is None and not opt.state
    assert all(torch.equal(p.detach(), sevens[k]) for k, p in model.named_parameters())
    assert all(torch.allclose(p, p0 + 1.0) for p, p0 in zip(_values(algo.model_old), old_before))     # the lagged network: learnt
    _run_updates(algo, buf, 1)                                       # the engine starts from the caller's (empty) optimizer state
    algo.hip_sync()
    st = opt.state[first]
    assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg_sq"], torch.full_like(st["exp_avg_sq"], 0.25))
    assert torch.allclose(first.detach(), torch.full_like(first, 9.0))


def test_algorithm_load_with_updates_pending_keeps_what_the_checkpoint_does_not_hold(monkeypatch):
    """`algorithm.load_state_dict(ckpt)` with lazy updates pending: everything the checkpoint holds is the checkpoint's, and
    what it does not hold -- AutoAlpha's optimizer, which is outside `Algorithm._optimizers` (sac.py:193,
    algorithm_base.py:523-543) -- keeps what the engine learnt, as under eager write-back (the load syncs first)."""
    algo, buf = _lazy_twin("sac", monkeypatch)
    ckpt = _make_sac_algo().state_dict()
    _run_updates(algo, buf, 2)
    assert algo.__dict__["_hip_stale"]
    algo.load_state_dict(dict(ckpt))
    sd = algo.state_dict()
    for k, v in ckpt.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(sd[k], v), k
    assert sd["_optimizers"] == ckpt["_optimizers"]                  # (the fresh algorithm's: no Adam state yet)
    st = algo.alpha._optim.state[algo.alpha._log_alpha]
    assert float(st["step"]) == 2.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.25))


def test_data_edit_recipe_keeps_the_learning_and_the_edit(monkeypatch):
    """The documented recipe for a `.data` edit under lazy write-back -- `hip_sync()`, the edit, `hip_invalidate()` -- keeps both
    what the engine learnt and the edit; and the collector forward's flat copy of the torch parameters (used while no engine
    exists, keyed on data pointers and version counters, which a `.data` edit changes neither of) is rebuilt after it."""
    algo, buf = _lazy_twin("dqn", monkeypatch)
    model = algo.policy.model
    weight, bias = model.net[0][0].weight, model.net[0][0].bias
    w0, b0 = weight.detach().clone(), bias.detach().clone()
    _run_updates(algo, buf, 2)
    algo.hip_sync()
    bias.data.add_(5.0)
    algo.hip_invalidate()
    _run_updates(algo, buf, 1)
    algo.hip_sync()
    assert torch.allclose(weight.detach(), w0 + 6.0) and torch.allclose(bias.detach(), b0 + 11.0)
    assert float(algo.optim._optim.state[weight]["step"]) == 3.0
    algo.hip_invalidate()                                            # no engine from here on: the collector reads the torch modules
    builds = []
    flat = lambda: algo.policy._hip_cached([model], lambda: (builds.append(1), bias.detach().clone())[1])  # noqa: E731
    v1 = flat()
    assert torch.equal(flat(), v1) and len(builds) == 1              # cached while nothing changes
    bias.data.add_(1.0)
    algo.hip_invalidate()
    assert torch.equal(flat(), v1 + 1.0) and len(builds) == 2


def test_hip_ppo_extra_state_restores_in_either_order(monkeypatch):
    """HipPPO's run state beside `state_dict()` -- the device-permutation key and the collector forward's sampling counter --
    restored with `load_hip_extra_state()` before or after `load_state_dict()`: the same counters, and no "shuffle sequence
    restarts" warning at the next update (before: loading the state dict second cleared the restored flag).  A checkpoint
    without its extra state still warns; an extra state without the sampling counter (older builds) still loads."""
    import warnings

    import gymnasium as gym
    from torch import nn
    from torch.distributions import Independent, Normal

    from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic
    import tianshou_amd.buffer as B
    import tianshou_amd.integration as I

    class FakePPO:
        def __init__(self, obs_dim, act_dim, flat, cfg):
            self.cfg, self.params, self.ret_rms = cfg, flat.clone(), [0.0, 1.0, 0.0]
            self.adam_m, self.adam_v, self.adam_step = torch.zeros_like(flat), torch.zeros_like(flat), 0

        def update(self, b, batch_size, repeat, perms):
            self.adam_step += 1
            return torch.zeros((1, 4)), 1

        def check(self):
            pass

    monkeypatch.setattr(I, "PPOEngine", FakePPO)
    monkeypatch.setattr(B, "random_permutation", lambda n, key, device: torch.randperm(n))

    def build():
        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                             action_shape=(6,), unbounded=True)
        critic = ContinuousCritic(preprocess_net=Net(state_shape=(17,), hidden_sizes=[64, 64], activation=nn.Tanh))
        policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_scaling=True,
                                          action_bound_method="clip", action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(6,)))
        algo = I.make_hip_ppo()(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), device="cpu", perm_seed=3)
        algo._hip_batch = {"obs": torch.zeros(16, 17)}
        return algo

    def update(algo):                                # the hook that consumes the key (the engine double stands for the kernels)
        algo._update_with_batch(None, 8, 1)

    a = build()
    assert a.policy._hip_family == "gauss" and a.hip_extra_state()["policy_calls"] == 0
    update(a)
    a.policy.__dict__["_hip_rt_calls"] = 5           # five collector forwards with device sampling
    sd, extra = a.state_dict(), a.hip_extra_state()
    assert extra == {"perm_seed": 3, "updates": 1, "policy_calls": 5}
    for order in ("extra_first", "state_dict_first"):
        b = build()
        if order == "extra_first":
            b.load_hip_extra_state(extra)
            b.load_state_dict(dict(sd))
        else:
            b.load_state_dict(dict(sd))
            b.load_hip_extra_state(extra)
        assert b.hip_extra_state() == extra, order
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            update(b)
        assert b._hip_updates == 2 and b._hip_engine.adam_step == 2, order
    c = build()
    c.load_state_dict(dict(sd))
    with pytest.warns(UserWarning, match="device-permutation key"):
        update(c)
    d = build()
    d.policy.__dict__["_hip_rt_calls"] = 2
    d.load_hip_extra_state({"perm_seed": 3, "updates": 1})
    assert d.hip_extra_state() == {"perm_seed": 3, "updates": 1, "policy_calls": 2}


def test_hip_sac_extra_state_carries_both_noise_counters(monkeypatch):
    """HipSAC's run state beside `state_dict()`: the update-noise counter of the engine's Philox stream and the collector forward's
    sampling counter; restored in either order around `load_state_dict()`; an extra state without them leaves the counters."""
    algo, buf = _lazy_twin("sac", monkeypatch)
    algo._hip_noise_calls, algo.policy.__dict__["_hip_rt_calls"] = 12, 4
    sd, extra = algo.state_dict(), algo.hip_extra_state()
    assert extra == {"update_noise_calls": 12, "policy_calls": 4}
    for first in (True, False):
        b = _make_sac_algo()
        if first:
            b.load_hip_extra_state(extra)
        b.load_state_dict(dict(sd))
        if not first:
            b.load_hip_extra_state(extra)
        assert b.hip_extra_state() == extra
    b.load_hip_extra_state({})
    assert b.hip_extra_state() == extra
