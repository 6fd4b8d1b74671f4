"""CPU: the HipDiscreteBCQ drop-in (tianshou_amd.integration.make_hip_discrete_bcq) without an engine -- over the real
reference classes where the reference is mounted, over tests/standin_bcq.py otherwise: the model check, the optimizer check,
and, with an engine double, the call order, the scalars read per update, the counters and the write-back."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_bcq as SB

REAL = ref_shim.reference_available()
C_, H_, W_, A_ = 2, 44, 36, 3


def _nets(hidden=(512,), shared=True, c=C_, h=H_, w=W_, n_act=A_, softmax=False):
    if REAL:
        ref_shim.install()
        from tianshou.env.atari.atari_network import DQNet
        from tianshou.utils.net.discrete import DiscreteActor

        trunk = lambda: DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True)      # noqa: E731
        actor = DiscreteActor
    else:
        trunk = lambda: SB.DQNetFeaturesOnly(c, h, w)      # noqa: E731
        actor = SB.DiscreteActor
    t1 = trunk()
    t2 = t1 if shared else trunk()
    kw = dict(action_shape=n_act, hidden_sizes=list(hidden), softmax_output=softmax)
    return actor(preprocess_net=t1, **kw), actor(preprocess_net=t2, **kw)


def _make(model, imitator, optim="adam", threshold=0.3, n_act=A_, **kw):
    from tianshou_amd.integration import make_hip_discrete_bcq

    kw.setdefault("target_update_freq", 2)
    if REAL:
        import gymnasium as gym
        from tianshou.algorithm.imitation.discrete_bcq import DiscreteBCQPolicy
        from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory

        factory = AdamOptimizerFactory(lr=1e-4) if optim == "adam" else RMSpropOptimizerFactory(lr=1e-4)
        policy = DiscreteBCQPolicy(model=model, imitator=imitator, action_space=gym.spaces.Discrete(n_act),
                                   unlikely_action_threshold=threshold, target_update_freq=kw["target_update_freq"])
        return make_hip_discrete_bcq()(policy=policy, optim=factory, device="cpu", **kw)
    extra = {} if optim == "adam" else {"optim": (torch.optim.RMSprop, {})}
    policy = SB.DiscreteBCQPolicy(model=model, imitator=imitator, unlikely_action_threshold=threshold,
                                  target_update_freq=kw["target_update_freq"])
    return make_hip_discrete_bcq(ref=SB)(policy=policy, lr=1e-4, device="cpu", **extra, **kw)


def test_supported_model_is_accepted():
    from tianshou_amd import bcq as BQ

    algo = _make(*_nets(), imitation_logits_penalty=0.25)
    assert type(algo).__name__ == "HipDiscreteBCQ" and algo._weight_reg == 0.25
    assert list(dict(algo.policy.named_parameters()).keys()) == BQ.TIANSHOU_KEYS
    assert len(list(algo.model_old.parameters())) == BQ.N_LAGGED
    if REAL:
        from tianshou.algorithm.imitation.discrete_bcq import DiscreteBCQ

        assert isinstance(algo, DiscreteBCQ)


def test_two_trunks_are_rejected():
    with pytest.raises(NotImplementedError, match="shared DQNet\\(features_only=True\\)"):
        _make(*_nets(shared=False))


@pytest.mark.parametrize("hidden", [(256,), (), (512, 512)])
def test_other_hidden_sizes_are_rejected(hidden):
    with pytest.raises(NotImplementedError, match="hidden_sizes=\\[512\\]"):
        _make(*_nets(hidden=hidden))


def test_softmax_heads_are_rejected():
    with pytest.raises(NotImplementedError, match="softmax_output=False"):
        _make(*_nets(softmax=True))


def test_mlp_model_is_rejected():
    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(nn.Flatten(), nn.Linear(C_ * H_ * W_, 64), nn.ReLU(), nn.Linear(64, A_))

    with pytest.raises(NotImplementedError, match="HipDiscreteBCQ: policy.model and policy.imitator must be DiscreteActor"):
        _make(Other(), Other())


def test_non_adam_optimizer_is_rejected():
    with pytest.raises(NotImplementedError, match="Adam"):
        _make(*_nets(), optim="rmsprop")


def test_engine_config_and_threshold_rounding():
    from tianshou_amd import bcq as BQ

    with pytest.raises(ValueError, match="target_update_freq>0"):
        BQ.BCQConfig(target_update_freq=0)
    with pytest.raises(ValueError):
        BQ.BCQConfig(unlikely_action_threshold=1.0)
    lt = BQ.log_tau_f32(0.3)
    assert lt == float(np.float32(np.log(0.3))) and lt < np.log(0.3) and BQ.log_tau_f32(0.0) == -np.inf
    hp = BQ.BCQConfig(lr=2e-4, max_grad_norm=5.0).to_c()
    assert (hp.lr, hp.max_grad_norm) == (2e-4, 5.0) and BQ.BCQConfig().to_c(grad_only=True).lr < 0


def test_flat_converters_are_inverse_permutations():
    """flat_to_torch(flat_from_torch(t)) == t for the fourteen tensors, on the CPU; ten tensors (a lagged network) leave the
    imitator part zero; the padding columns of both heads are zero."""
    from tests import oracle_bcq as OB
    from tianshou_amd import bcq as BQ

    p = OB.init_params(C_, H_, W_, A_, 1)
    t = [p[k] for k in OB.PARAM_ORDER]
    flat = BQ.flat_from_torch(t, C_, H_, W_, A_, device="cpu")
    back = BQ.flat_to_torch(flat, C_, H_, W_, A_)
    assert len(back) == 14 and all(torch.equal(a, b) for a, b in zip(t, back))
    assert sorted(flat[flat != 0].tolist()) == sorted(x for v in t for x in v.reshape(-1).tolist() if x != 0)
    f = 64 * 2 * 1
    head = (f + 1) * 512 + 513 * 32
    assert flat.numel() == (8 * 8 * C_ + 1) * 32 + 513 * 64 + 577 * 64 + 2 * head
    for end in (flat.numel() - head, flat.numel()):
        assert float(flat[end - 513 * 32:end].reshape(513, 32)[:, A_:].abs().max()) == 0.0
    old = BQ.flat_from_torch(t[:10], C_, H_, W_, A_, device="cpu")
    assert torch.equal(old[:-head], flat[:-head]) and float(old[-head:].abs().max()) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(t[:10], BQ.flat_to_torch(old, C_, H_, W_, A_)))


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_hip_discrete_bcq_wrapper_runs_with_engine_double(monkeypatch):
    """Two update() calls of HipDiscreteBCQ over a CPU double of BCQEngine (the pattern of tests/test_integration_shim.py): call
    order, the threshold and the penalty read at every update, the counters, the statistics, and the write-back into all
    fourteen tensors plus the ten lagged ones, the shared trunk written once."""
    from tianshou.algorithm.imitation.discrete_bcq import DiscreteBCQTrainingStats
    from tianshou.data import PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou.utils.torch_utils import policy_within_training_step
    import tianshou_amd.bcq as BQ
    import tianshou_amd.dqn as D
    from tests.test_integration_shim import _fill, _patch_for_cpu

    calls, seen = [], []
    c, h, w, A = 4, 84, 84, 6
    head = 3137 * 512 + 513 * 32

    class FakeBCQ:
        def __init__(self, c_, h_, w_, n_act, flat, cfg):
            assert (c_, h_, w_, n_act) == (c, h, w, A)
            assert (cfg.gamma, cfg.n_step, cfg.target_update_freq, cfg.lr) == (0.9, 2, 2, 1e-4)
            assert flat.numel() == (8 * 8 * 4 + 1) * 32 + 513 * 64 + 577 * 64 + 2 * head
            self.c, self.h, self.w, self.n_act, self.cfg = c_, h_, w_, n_act, cfg
            self.params, self.params_old = flat.clone(), flat.clone()
            self.adam_m, self.adam_v, self.adam_step, self.iter = torch.zeros_like(flat), torch.zeros_like(flat), 0, 0

        def preprocess(self, m, frames, idx, stack, obs_next_frames=None):
            assert frames.dtype == torch.uint8 and stack == 1 and obs_next_frames is not None
            calls.append("preprocess")
            seen.append((self.cfg.log_tau, self.cfg.imitation_logits_penalty))
            return torch.zeros(idx.numel())

        def update_with_batch(self, obs, act, ret):
            assert obs.shape == (8, 84, 84, 4) and obs.dtype == torch.uint8 and ret.shape == (8,) and act.shape == (8,)
            calls.append("update")
            seen.append((self.cfg.log_tau, self.cfg.imitation_logits_penalty))
            self.adam_step += 1
            self.iter += 1
            self.params += 2.0
            self.params_old += 0.5
            self.adam_m += 0.125
            return torch.tensor([1.75, 0.5, 0.25, 4.0])

    algo = _make(*_nets(c=c, h=h, w=w, n_act=A), threshold=0.3, n_act=A, gamma=0.9, n_step_return_horizon=2,
                 imitation_logits_penalty=0.25)
    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(BQ, "BCQEngine", FakeBCQ)
    monkeypatch.setattr(D, "gather_obs_nhwc", lambda frames, m, idx, stack, as_u8=False: frames[idx].permute(0, 2, 3, 1))
    buf = VectorReplayBuffer(32, 2)
    _fill(buf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    params = [dict(algo.policy.named_parameters())[k] for k in BQ.TIANSHOU_KEYS]
    olds = list(algo.model_old.parameters())
    assert len(olds) == 10 and all(o is not p for o, p in zip(olds, params))
    before = [p.detach().clone() for p in params]
    with policy_within_training_step(algo.policy):
        stats = algo.update(buffer=buf, sample_size=8)
    assert isinstance(stats, DiscreteBCQTrainingStats)
    assert (stats.loss, stats.q_loss, stats.i_loss, stats.reg_loss) == (1.75, 0.5, 0.25, 4.0)
    assert calls == ["preprocess", "update"] and algo._iter == 1
    assert seen == [(float(np.log(0.3)), 0.25)] * 2
    for p, b in zip(params, before):                                           # engine -> all fourteen nn.Parameters, once each
        assert torch.allclose(p.detach(), b + 2.0)
    assert algo.policy.imitator.preprocess is algo.policy.model.preprocess
    for o, b in zip(olds, before):                                             # the ten lagged tensors: their own values
        assert torch.allclose(o.detach(), b + 0.5)
    for p in params:
        st = algo.optim._optim.state[p]
        assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125))
    sd = algo.state_dict()                                                     # the reference's format: the trunk twice
    assert torch.equal(sd["policy.imitator.preprocess.net.0.weight"], sd["policy.model.preprocess.net.0.weight"])
    # the scalars are read from the algorithm at every update; a prioritized buffer is accepted, its weights are ignored
    algo.policy._log_tau, algo._weight_reg = float(np.log(0.5)), 0.75
    pbuf = PrioritizedVectorReplayBuffer(32, 2, alpha=0.6, beta=0.4)
    _fill(pbuf, 12, (4, 84, 84), np.zeros(2, np.int64), np.uint8)
    with policy_within_training_step(algo.policy):
        algo.update(buffer=pbuf, sample_size=8)
    assert calls == ["preprocess", "update"] * 2 and algo._iter == 2
    assert seen[2:] == [(float(np.log(0.5)), 0.75)] * 2
    for p, b in zip(params, before):
        assert torch.allclose(p.detach(), b + 4.0)
