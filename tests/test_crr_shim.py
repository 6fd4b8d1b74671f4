"""CPU: the HipDiscreteCRR drop-in (tianshou_amd.integration.make_hip_discrete_crr) without an engine -- over the real
reference classes where the reference is mounted, over tests/standin_crr.py otherwise: every refusal of the model check, the
refusal of two lagged trunks that differ, the key permutation, and, with an engine double, the call order, the scalars read per
update, the counters and the write-back into both lagged modules, with and without lagged networks."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_crr as SC

REAL = ref_shim.reference_available()
C_, H_, W_, A_ = 2, 44, 36, 3


def _nets(hidden=(512,), shared=True, c=C_, h=H_, w=W_, n_act=A_, softmax=False, critic_out=None):
    if REAL:
        ref_shim.install()
        from tianshou.env.atari.atari_network import DQNet
        from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

        trunk = lambda: DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True)      # noqa: E731
    else:
        trunk = lambda: SC.DQNetFeaturesOnly(c, h, w)      # noqa: E731
        DiscreteActor, DiscreteCritic = SC.DiscreteActor, SC.DiscreteCritic
    t1 = trunk()
    t2 = t1 if shared else trunk()
    actor = DiscreteActor(preprocess_net=t1, action_shape=n_act, hidden_sizes=list(hidden), softmax_output=softmax)
    critic = DiscreteCritic(preprocess_net=t2, hidden_sizes=list(hidden), last_size=n_act if critic_out is None else critic_out)
    return actor, critic


def _make(actor, critic, optim="adam", n_act=A_, **kw):
    from tianshou_amd.integration import make_hip_discrete_crr

    kw.setdefault("target_update_freq", 2)
    if REAL:
        import gymnasium as gym
        from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy
        from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory

        factory = AdamOptimizerFactory(lr=1e-4) if optim == "adam" else RMSpropOptimizerFactory(lr=1e-4)
        policy = DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(n_act))
        return make_hip_discrete_crr()(policy=policy, critic=critic, optim=factory, device="cpu", **kw)
    extra = {} if optim == "adam" else {"optim": (torch.optim.RMSprop, {})}
    policy = SC.DiscreteActorPolicy(actor=actor)
    return make_hip_discrete_crr(ref=SC)(policy=policy, critic=critic, lr=1e-4, device="cpu", **extra, **kw)


def _old(m):
    return getattr(m, "module", m)


def test_supported_model_is_accepted():
    from tianshou_amd import crr as CR

    algo = _make(*_nets(), min_q_weight=2.5, policy_improvement_mode="binary")
    assert type(algo).__name__ == "HipDiscreteCRR" and algo._min_q_weight == 2.5
    assert list(dict(nn.ModuleList([algo.policy, algo.critic]).named_parameters()).keys()) == CR.TIANSHOU_KEYS
    assert len(list(_old(algo.actor_old).parameters())) == 10 and len(list(_old(algo.critic_old).parameters())) == 10
    assert _old(algo.actor_old).preprocess is not _old(algo.critic_old).preprocess
    if REAL:
        from tianshou.algorithm.imitation.discrete_crr import DiscreteCRR

        assert isinstance(algo, DiscreteCRR)
    live = _make(*_nets(), target_update_freq=0)
    assert live.actor_old is live.policy.actor and live.critic_old is live.critic


def test_two_trunks_are_rejected():
    with pytest.raises(NotImplementedError, match="HipDiscreteCRR"):
        _make(*_nets(shared=False))


@pytest.mark.parametrize("hidden", [(256,), (), (512, 512)])
def test_other_hidden_sizes_are_rejected(hidden):
    with pytest.raises(NotImplementedError, match="hidden_sizes=\\[512\\]"):
        _make(*_nets(hidden=hidden))


def test_softmax_actor_is_rejected():
    with pytest.raises(NotImplementedError, match="softmax_output=True"):
        _make(*_nets(softmax=True))


def test_heads_of_different_width_are_rejected():
    with pytest.raises(NotImplementedError, match="same number of actions"):
        _make(*_nets(critic_out=A_ + 1))


def test_other_trunk_is_rejected():
    actor, critic = _nets()
    conv = actor.preprocess.net[0]
    actor.preprocess.net[0] = nn.Conv2d(conv.in_channels, 32, 6, 4)
    with pytest.raises(NotImplementedError, match="DQNet convolution trunk"):
        _make(actor, critic)


def test_mlp_model_is_rejected():
    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(nn.Flatten(), nn.Linear(C_ * H_ * W_, 64), nn.ReLU(), nn.Linear(64, A_))

    with pytest.raises(NotImplementedError, match="HipDiscreteCRR: policy.actor must be DiscreteActor"):
        _make(Other(), Other())


def test_non_adam_optimizer_is_rejected():
    with pytest.raises(NotImplementedError, match="Adam"):
        _make(*_nets(), optim="rmsprop")


def test_a_second_optimizer_group_is_rejected():
    algo = _make(*_nets())
    opt = algo.optim._optim
    g = opt.param_groups[0]
    moved = g["params"].pop()
    opt.add_param_group({"params": [moved]})
    with pytest.raises(NotImplementedError, match="one optimizer group"):
        algo._hip_check_model()


def test_engine_config():
    from tianshou_amd import crr as CR

    with pytest.raises(ValueError, match="policy_improvement_mode"):
        CR.CRRConfig(policy_improvement_mode="softmax")
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            CR.CRRConfig(beta=bad)
    assert [CR.mode_id(m) for m in ("exp", "binary", "all")] == [0, 1, 2]
    hp = CR.CRRConfig(lr=2e-4, max_grad_norm=5.0).to_c()
    assert (hp.lr, hp.max_grad_norm) == (2e-4, 5.0) and CR.CRRConfig().to_c(grad_only=True).lr < 0
    assert CR.CRRConfig().target_update_freq == 0                  # the reference's default: no lagged networks


def test_flat_converters_are_inverse_permutations():
    """flat_to_torch(flat_from_torch(t)) == t for the fourteen tensors, on the CPU; the flat vector is the BCQ layout with the
    critic in the Q head's place and the actor in the imitator's; the padding columns of both heads are zero."""
    from tests import oracle_crr as OC
    from tianshou_amd import bcq as BQ
    from tianshou_amd import crr as CR

    p = OC.init_params(C_, H_, W_, A_, 1)
    t = [p[k] for k in OC.PARAM_ORDER]
    flat = CR.flat_from_torch(t, C_, H_, W_, A_, device="cpu")
    back = CR.flat_to_torch(flat, C_, H_, W_, A_)
    assert len(back) == 14 and all(torch.equal(a, b) for a, b in zip(t, back))
    assert sorted(flat[flat != 0].tolist()) == sorted(x for v in t for x in v.reshape(-1).tolist() if x != 0)
    assert torch.equal(flat, BQ.flat_from_torch(t[:6] + t[10:] + t[6:10], C_, H_, W_, A_, device="cpu"))
    head = (64 * 2 * 1 + 1) * 512 + 513 * 32
    assert flat.numel() == (8 * 8 * C_ + 1) * 32 + 513 * 64 + 577 * 64 + 2 * head
    for end in (flat.numel() - head, flat.numel()):
        assert float(flat[end - 513 * 32:end].reshape(513, 32)[:, A_:].abs().max()) == 0.0
    actor_head = BQ.flat_to_torch(flat, C_, H_, W_, A_)[10:]
    assert all(torch.equal(a, b) for a, b in zip(actor_head, t[6:10]))
    with pytest.raises(ValueError):
        CR.flat_from_torch(t[:10], C_, H_, W_, A_, device="cpu")


class FakeCRR:
    """tianshou_amd.crr.CRREngine's interface on the CPU: every update adds 2 to the parameters, 0.5 to the lagged vector and
    0.125 to the first Adam moment, and records the scalars it was handed."""
    calls: list = []
    seen: list = []

    def __init__(self, c, h, w, n_act, flat, cfg):
        self.c, self.h, self.w, self.n_act, self.cfg = c, h, w, n_act, cfg
        self.params = flat.clone()
        self.params_old = flat.clone() if cfg.target_update_freq > 0 else self.params
        self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

    def update_with_batch(self, obs, obs_next, act, rew, done):
        b = obs.shape[0]
        assert obs.shape == obs_next.shape == (b, self.h, self.w, self.c) and obs.dtype == obs_next.dtype == torch.uint8
        assert act.shape == rew.shape == done.shape == (b,) and rew.dtype == torch.float32 and done.dtype == torch.uint8
        cfg = self.cfg
        FakeCRR.calls.append("update")
        FakeCRR.seen.append((cfg.policy_improvement_mode, cfg.beta, cfg.ratio_upper_bound, cfg.min_q_weight, cfg.gamma))
        self.adam_step += 1
        self.iter += 1
        self.params += 2.0
        if cfg.target_update_freq > 0:
            self.params_old += 0.5
        self.adam_m += 0.125
        return torch.tensor([1.75, 0.5, 0.25, 4.0])


def _buffer(c, h, w, prio=False, n=12):
    rng = np.random.default_rng(0)
    if REAL:
        from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer

        buf = PrioritizedVectorReplayBuffer(32, 2, alpha=0.6, beta=0.4) if prio else VectorReplayBuffer(32, 2)
    else:
        Batch = SC.Batch
        cls = SC.PrioritizedVectorReplayBuffer if prio else SC.VectorReplayBuffer
        buf = cls(32, 2, obs_shape=(c, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    for t in range(n):
        buf.add(Batch(obs=rng.integers(0, 255, size=(2, c, h, w)).astype(np.uint8), act=np.zeros(2, np.int64),
                      rew=np.full(2, 0.5 * t), terminated=np.array([t % 5 == 4, False]), truncated=np.zeros(2, bool),
                      obs_next=rng.integers(0, 255, size=(2, c, h, w)).astype(np.uint8)))
    return buf


def _patch(monkeypatch):
    import tianshou_amd.crr as CR
    import tianshou_amd.dqn as D
    from tests.test_integration_shim import _patch_for_cpu

    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(CR, "CRREngine", FakeCRR)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    FakeCRR.calls, FakeCRR.seen = [], []


def _update(algo, buf, n=8):
    algo.policy.is_within_training_step = True
    try:
        return algo.update(buffer=buf, sample_size=n)
    finally:
        algo.policy.is_within_training_step = False


def _live14(algo):
    from tianshou_amd import crr as CR

    named = dict(nn.ModuleList([algo.policy, algo.critic]).named_parameters())
    return [named[k] for k in CR.TIANSHOU_KEYS]


def test_wrapper_runs_with_engine_double_and_writes_both_lagged_modules_back(monkeypatch):
    _patch(monkeypatch)
    algo = _make(*_nets(), gamma=0.9, policy_improvement_mode="exp", beta=0.5, ratio_upper_bound=3.0, min_q_weight=2.5)
    buf = _buffer(C_, H_, W_)
    params = _live14(algo)
    a_old, c_old = list(_old(algo.actor_old).parameters()), list(_old(algo.critic_old).parameters())
    assert all(o is not p for o, p in zip(a_old + c_old, params + params))
    before = [p.detach().clone() for p in params]
    stats = _update(algo, buf)
    assert type(stats).__name__ == "DiscreteCRRTrainingStats"
    assert (stats.loss, stats.actor_loss, stats.critic_loss, stats.cql_loss) == (1.75, 0.5, 0.25, 4.0)
    assert FakeCRR.calls == ["update"] and algo._iter == 1
    assert FakeCRR.seen == [("exp", 0.5, 3.0, 2.5, 0.9)]
    assert hasattr(algo._hip_mirror, "done")                                    # the base preprocessing ran first, then the mirror
    for p, b in zip(params, before):                                            # engine -> all fourteen nn.Parameters, once each
        assert torch.allclose(p.detach(), b + 2.0)
    assert algo.policy.actor.preprocess is algo.critic.preprocess
    # the lagged trunk into BOTH modules, the actor head into actor_old, the critic head into critic_old
    for o, b in zip(a_old, before[:10]):
        assert torch.allclose(o.detach(), b + 0.5)
    for o, b in zip(c_old, before[:6] + before[10:]):
        assert torch.allclose(o.detach(), b + 0.5)
    for p in params:
        st = algo.optim._optim.state[p]
        assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125))
    # the scalars are read from the algorithm at every update; a prioritized buffer is accepted, its weights are ignored
    algo._policy_improvement_mode, algo._beta, algo._ratio_upper_bound, algo._min_q_weight = "binary", 2.0, 7.0, 0.0
    algo.discounted_return_computation.gamma = 0.5
    _update(algo, _buffer(C_, H_, W_, prio=True))
    assert FakeCRR.calls == ["update"] * 2 and algo._iter == 2
    assert FakeCRR.seen[1] == ("binary", 2.0, 7.0, 0.0, 0.5)
    for p, b in zip(params, before):
        assert torch.allclose(p.detach(), b + 4.0)


def test_base_preprocessing_is_kept(monkeypatch):
    """`_preprocess_batch` is the reference's own: batch.returns holds its discounted returns (on the stand-in: its call is
    counted), and with return standardization its running statistics move."""
    _patch(monkeypatch)
    algo = _make(*_nets(), return_standardization=True)
    buf = _buffer(C_, H_, W_)
    seen = {}
    orig = type(algo)._update_with_batch
    monkeypatch.setattr(type(algo), "_update_with_batch", lambda self, batch: seen.update(ret=np.asarray(batch.returns)) or orig(self, batch))
    _update(algo, buf)
    assert seen["ret"].shape == (8,)
    if REAL:
        assert algo.discounted_return_computation.ret_rms.count > 1
    else:
        assert algo.base_preprocess_calls == 1


def test_unequal_lagged_trunks_are_refused(monkeypatch):
    _patch(monkeypatch)
    algo = _make(*_nets())
    with torch.no_grad():
        next(iter(_old(algo.critic_old).preprocess.parameters())).data.add_(1e-3)
    with pytest.raises(NotImplementedError, match="trunks of actor_old and critic_old differ"):
        _update(algo, _buffer(C_, H_, W_))
    assert FakeCRR.calls == []


def test_without_lagged_networks_nothing_lagged_is_loaded_or_written(monkeypatch):
    _patch(monkeypatch)
    algo = _make(*_nets(), target_update_freq=0)
    params = _live14(algo)
    before = [p.detach().clone() for p in params]
    _update(algo, _buffer(C_, H_, W_))
    eng = algo._hip_engine
    assert eng.cfg.target_update_freq == 0 and eng.params_old is eng.params
    for p, b in zip(params, before):
        assert torch.allclose(p.detach(), b + 2.0)
    assert algo.actor_old is algo.policy.actor and algo.critic_old is algo.critic and algo._iter == 1
