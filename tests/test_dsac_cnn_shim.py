"""CPU: the HipDiscreteSACCnn drop-in (tianshou_amd.integration.make_hip_discrete_sac_cnn) without an engine -- over the real
reference classes where the reference is mounted, over tests/standin_dsac_cnn.py otherwise: every refusal of the model check,
and, with an engine double, the hooks' data flow (call order, importance weights in, batch.weight out, the statistics) and
the state path: write-back of the live tensors, of the ONE lagged trunk into both lagged modules, of three distinct trunk
moment sets into the three optimizers and of alpha; the round trip through state_dict(); the refusal of two lagged trunks
that differ."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_dsac_cnn as SD

REAL = ref_shim.reference_available()
C_, H_, W_, A_, HID = 2, 44, 36, 3, 64


def _classes():
    if REAL:
        ref_shim.install()
        from tianshou.env.atari.atari_network import DQNet
        from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

        return DQNet, DiscreteActor, DiscreteCritic
    return SD.DQNet, SD.DiscreteActor, SD.DiscreteCritic


def _nets(shared=True, shared2=True, hidden=HID, n_act=A_, softmax=False, critic2_out=None, added=True):
    DQNet, DiscreteActor, DiscreteCritic = _classes()

    def trunk():
        if added:
            return DQNet(C_, H_, W_, action_shape=n_act, features_only=True, output_dim_added_layer=hidden)
        if REAL:
            return DQNet(C_, H_, W_, action_shape=n_act, features_only=True)
        from tests.standin_bcq import DQNetFeaturesOnly

        return DQNetFeaturesOnly(C_, H_, W_)

    t = trunk()
    actor = DiscreteActor(preprocess_net=t, action_shape=n_act, softmax_output=softmax)
    critic1 = DiscreteCritic(preprocess_net=t if shared else trunk(), last_size=n_act)
    critic2 = DiscreteCritic(preprocess_net=t if shared2 else trunk(), last_size=n_act if critic2_out is None else critic2_out)
    return actor, critic1, critic2


def _make(actor, critic1, critic2, optim="adam", auto=False, n_act=A_, **kw):
    from tianshou_amd.integration import make_hip_discrete_sac_cnn

    kw.setdefault("tau", 0.05)
    if REAL:
        import gymnasium as gym
        from tianshou.algorithm.modelfree.discrete_sac import DiscreteSACPolicy
        from tianshou.algorithm.modelfree.sac import AutoAlpha
        from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory

        fac = (lambda lr: AdamOptimizerFactory(lr=lr)) if optim == "adam" else (lambda lr: RMSpropOptimizerFactory(lr=lr))
        alpha = AutoAlpha(0.9, -1.0, AdamOptimizerFactory(lr=1e-3)) if auto else 0.2
        policy = DiscreteSACPolicy(actor=actor, action_space=gym.spaces.Discrete(n_act))
        return make_hip_discrete_sac_cnn()(policy=policy, policy_optim=fac(3e-4), critic=critic1, critic_optim=fac(1e-4),
                                           critic2=critic2, critic2_optim=fac(1e-4), alpha=alpha, device="cpu", **kw)
    alpha = SD.AutoAlpha(0.9, -1.0, 1e-3) if auto else 0.2
    algo = make_hip_discrete_sac_cnn(ref=SD)(policy=SD.DiscreteSACPolicy(actor=actor), critic=critic1, critic2=critic2, lr=3e-4,
                                             critic_lr=1e-4, alpha=alpha, device="cpu", **kw)
    if optim != "adam":
        raise AssertionError("the stand-in builds Adam only: swap the optimizer on the built algorithm instead")
    return algo


def _old(m):
    return getattr(m, "module", m)


def test_supported_model_is_accepted():
    from tianshou_amd import dsac_cnn as DC

    algo = _make(*_nets(), auto=True, gamma=0.9, n_step_return_horizon=3)
    assert type(algo).__name__ == "HipDiscreteSACCnn" and (algo._hip_hidden, algo._hip_n_act) == (HID, A_)
    assert list(dict(nn.ModuleList([algo.policy, algo.critic, algo.critic2]).named_parameters()).keys()) == DC.TIANSHOU_KEYS
    for opt in (algo.policy_optim, algo.critic_optim, algo.critic2_optim):         # the trunk sits in all three optimizers
        assert len([p for g in opt._optim.param_groups for p in g["params"]]) == 10
    assert _old(algo.critic_old).preprocess is not _old(algo.critic2_old).preprocess      # two lagged trunk copies
    if REAL:
        from tianshou.algorithm.modelfree.discrete_sac import DiscreteSAC

        assert isinstance(algo, DiscreteSAC)


def test_a_critic_on_its_own_trunk_is_rejected():
    with pytest.raises(NotImplementedError, match="do not share one feature-net object"):
        _make(*_nets(shared=False))


def test_critic2_on_its_own_trunk_and_critic2_none_are_rejected():
    with pytest.raises(NotImplementedError, match="critic2 does not share the feature-net object"):
        _make(*_nets(shared2=False))
    actor, critic1, _ = _nets()
    with pytest.raises(NotImplementedError, match="critic2=None deep-copies"):
        _make(actor, critic1, None)


def test_trunk_without_the_added_layer_is_rejected():
    with pytest.raises(NotImplementedError, match="HipDiscreteSACCnn"):
        _make(*_nets(added=False))


def test_other_conv_trunk_is_rejected():
    actor, critic1, critic2 = _nets()
    conv = actor.preprocess.net[0][0]
    actor.preprocess.net[0][0] = nn.Conv2d(conv.in_channels, 32, 6, 4)
    with pytest.raises(NotImplementedError, match="DQNet convolution trunk"):
        _make(actor, critic1, critic2)


@pytest.mark.parametrize("kw", [dict(stride=2), dict(padding=1), dict(dilation=2), dict(padding="same", stride=1)])
def test_convolutions_of_dqnet_shape_but_other_geometry_are_rejected(kw):
    """The weight shapes alone do not identify DQNet: the same kernels with another stride, padding or dilation are another net."""
    actor, critic1, critic2 = _nets()
    conv = actor.preprocess.net[0][2]
    args = dict(stride=2)
    args.update(kw)
    actor.preprocess.net[0][2] = nn.Conv2d(conv.in_channels, conv.out_channels, 4, **args)
    if args == dict(stride=2):
        _make(actor, critic1, critic2)                     # (the unchanged geometry is accepted)
        return
    with pytest.raises(NotImplementedError, match="stride 4 / 2 / 1"):
        _make(actor, critic1, critic2)


def test_trunk_with_another_activation_or_an_extra_layer_is_rejected():
    actor, critic1, critic2 = _nets()
    actor.preprocess.net[0][1] = nn.Tanh()
    with pytest.raises(NotImplementedError, match="conv, ReLU, conv, ReLU, conv, ReLU, Flatten, Linear, ReLU"):
        _make(actor, critic1, critic2)
    actor, critic1, critic2 = _nets()
    actor.preprocess.net = nn.Sequential(*actor.preprocess.net, nn.Dropout(0.1))       # parameter-free: the keys do not change
    with pytest.raises(NotImplementedError, match="got \\[.*Dropout"):
        _make(actor, critic1, critic2)


@pytest.mark.parametrize("hidden", [48, 2048])
def test_unsupported_added_layer_width_is_rejected(hidden):
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        _make(*_nets(hidden=hidden))


def test_heads_with_hidden_layers_are_rejected():
    actor, critic1, critic2 = _nets()
    critic1.last.model = nn.Sequential(nn.Linear(HID, 32), nn.ReLU(), nn.Linear(32, A_))
    with pytest.raises(NotImplementedError, match="got parameters"):
        _make(actor, critic1, critic2)


def test_heads_of_different_width_are_rejected():
    with pytest.raises(NotImplementedError, match="same 1 <= n_act <= 64"):
        _make(*_nets(critic2_out=A_ + 1))
    with pytest.raises(NotImplementedError, match="same 1 <= n_act <= 64"):
        _make(*_nets(n_act=65), n_act=65)


def test_softmax_actor_is_rejected():
    with pytest.raises(NotImplementedError, match="softmax_output=True"):
        _make(*_nets(softmax=True))


@pytest.mark.parametrize("which", ["policy_optim", "critic_optim", "critic2_optim"])
def test_non_adam_optimizer_clipping_and_foreign_parameters_are_rejected(which):
    algo = _make(*_nets())
    wrapper = getattr(algo, which)
    held = [p for g in wrapper._optim.param_groups for p in g["params"]]
    adam = wrapper._optim
    wrapper._optim = torch.optim.RMSprop(held, lr=1e-4)
    with pytest.raises(NotImplementedError, match="Adam"):
        algo._hip_check_model()
    wrapper._optim = torch.optim.Adam(held, lr=1e-4, weight_decay=1e-2)
    with pytest.raises(NotImplementedError, match="Adam"):
        algo._hip_check_model()
    wrapper._optim = adam
    wrapper._max_grad_norm = 1.0
    with pytest.raises(NotImplementedError, match=f"{which} clips the gradient norm"):
        algo._hip_check_model()
    wrapper._max_grad_norm = None
    wrapper._optim = torch.optim.Adam(held[:8], lr=1e-4)                          # the trunk alone: the own head is missing
    with pytest.raises(NotImplementedError, match=f"{which} must hold the shared trunk and its own head"):
        algo._hip_check_model()
    wrapper._optim = adam
    algo._hip_check_model()


def test_non_adam_alpha_optimizer_is_rejected():
    algo = _make(*_nets(), auto=True)
    algo.alpha._optim = torch.optim.SGD([algo.alpha._log_alpha], lr=1e-3)
    with pytest.raises(NotImplementedError, match="AutoAlpha must use torch.optim.Adam"):
        algo._hip_check_model()


def test_flat_converters_are_inverse_permutations():
    """flat_to_torch(flat_from_torch(t)) == t for the live vector (three heads), the lagged vector (two) and one optimizer's set
    (one), on the CPU; nothing but the tensors' own values and the zero padding columns is in the flat vector."""
    from tests import oracle_dsac_cnn as OS
    from tianshou_amd import dsac_cnn as DC

    p = OS.init_params(C_, H_, W_, A_, HID, 1)
    for order in (OS.PARAM_ORDER, OS.LAGGED_ORDER, OS.set_order("actor")):
        t = [p[k] for k in order]
        flat = DC.flat_from_torch(t, C_, H_, W_, A_, HID, device="cpu")
        back = DC.flat_to_torch(flat, C_, H_, W_, A_, HID)
        assert len(back) == len(t) and all(torch.equal(a, b) for a, b in zip(t, back))
        assert sorted(flat[flat != 0].tolist()) == sorted(x for v in t for x in v.reshape(-1).tolist() if x != 0)
        n_heads = (len(order) - 8) // 2
        trunk = (8 * 8 * C_ + 1) * 32 + 513 * 64 + 577 * 64 + (128 + 1) * HID
        assert flat.numel() == trunk + n_heads * (HID + 1) * 32
        for k in range(n_heads):
            head = flat[trunk + k * (HID + 1) * 32: trunk + (k + 1) * (HID + 1) * 32].reshape(HID + 1, 32)
            assert float(head[:, A_:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        DC.flat_from_torch([p[k] for k in OS.TRUNK], C_, H_, W_, A_, HID, device="cpu")
    with pytest.raises(ValueError, match="added layer"):
        DC.flat_from_torch([p[k] for k in OS.PARAM_ORDER], C_, H_, W_, A_, 128, device="cpu")
    assert DC.TIANSHOU_KEYS == OS.TIANSHOU_KEYS and DC.SETS == OS.SETS


class FakeDSAC:
    """tianshou_amd.dsac_cnn.DiscreteSACCnnEngine's interface on the CPU: every update adds 2 to the parameters, 0.5 to the
    lagged vector, 0.125 * (k + 1) to the first moment of set k, 0.25 to log alpha and 0.0625 to its first moment."""
    calls: list = []
    seen: list = []

    def __init__(self, c, h, w, n_act, hidden, flat, cfg):
        self.c, self.h, self.w, self.n_act, self.hidden, self.cfg = c, h, w, n_act, hidden, cfg
        self.Hd = (hidden + 1) * ((n_act + 31) // 32 * 32)
        self.T = flat.numel() - 3 * self.Hd
        self.G = self.T + self.Hd
        self.params = flat.clone()
        self.params_old = torch.cat([flat[:self.T], flat[self.T + self.Hd:]]).clone()
        self.adam_m, self.adam_v, self.adam_step = torch.zeros((3, self.G)), torch.zeros((3, self.G)), 0
        self.log_alpha = torch.full((1,), cfg.log_alpha0)
        self.log_alpha_m, self.log_alpha_v = torch.zeros(1), torch.zeros(1)

    def policy_forward(self, obs):
        FakeDSAC.calls.append("forward")
        return torch.zeros((obs.shape[0], self.n_act))

    def preprocess(self, m, frames, idx, stack, obs_next_frames=None):
        FakeDSAC.calls.append("preprocess")
        FakeDSAC.seen.append(("preprocess", stack, obs_next_frames is not None, self.cfg.n_step, self.cfg.gamma))
        return torch.arange(idx.numel(), dtype=torch.float32)

    def update_with_batch(self, obs, act, returns, weight=None):
        b = obs.shape[0]
        assert obs.shape == (b, self.h, self.w, self.c) and obs.dtype == torch.uint8
        assert act.shape == returns.shape == (b,) and torch.equal(returns, torch.arange(b, dtype=torch.float32))
        FakeDSAC.calls.append("update")
        FakeDSAC.seen.append(("update", None if weight is None else weight.clone(), self.cfg.actor_lr, self.cfg.critic_lr,
                              self.cfg.alpha_lr, self.adam_m[:, 0].clone(), self.adam_step, float(self.log_alpha_m)))
        self.adam_step += 1
        self.params += 2.0
        self.params_old += 0.5
        for k in range(3):
            self.adam_m[k] += 0.125 * (k + 1)
        self.log_alpha += 0.25
        self.log_alpha_m += 0.0625
        return torch.tensor([1.5, 2.5, 3.5, 0.75, -0.5]), torch.arange(b, dtype=torch.float32) * 0.5


def _buffer(prio=False, n=12, stacked=False):
    rng = np.random.default_rng(0)
    shape = (H_, W_) if stacked else (C_, H_, W_)
    if REAL:
        from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer

        kw = dict(stack_num=C_, ignore_obs_next=True, save_only_last_obs=False) if stacked else {}
        buf = PrioritizedVectorReplayBuffer(32, 2, alpha=0.6, beta=0.4, **kw) if prio else VectorReplayBuffer(32, 2, **kw)
    else:
        Batch = SD.Batch
        cls = SD.PrioritizedVectorReplayBuffer if prio else SD.VectorReplayBuffer
        buf = cls(32, 2, obs_shape=shape, act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64, stack_num=C_ if stacked else 1)
        if stacked:
            from tests import standin as SI

            buf._meta = SI._Meta(("obs", "act", "rew", "terminated", "truncated", "done"))
    for t in range(n):
        buf.add(Batch(obs=rng.integers(0, 255, size=(2, *shape)).astype(np.uint8), act=np.ones(2, np.int64),
                      rew=np.full(2, 0.5 * t), terminated=np.array([t % 5 == 4, False]), truncated=np.zeros(2, bool),
                      obs_next=rng.integers(0, 255, size=(2, *shape)).astype(np.uint8)))
    return buf


def _patch(monkeypatch):
    import tianshou_amd.buffer as B
    import tianshou_amd.dqn as D
    import tianshou_amd.dsac_cnn as DC
    import tianshou_amd.returns as R
    from tests.test_integration_shim import _patch_for_cpu

    _patch_for_cpu(monkeypatch)
    monkeypatch.setattr(DC, "DiscreteSACCnnEngine", FakeDSAC)

    def gather(frames, m, idx, stack, as_u8=False):
        x = frames[idx]
        return x.permute(0, 2, 3, 1) if x.dim() == 4 else torch.stack([x] * stack, dim=-1)

    monkeypatch.setattr(D, "gather_obs_nhwc", gather)
    monkeypatch.setattr(R, "nstep_indices", lambda m, idx, n: idx)
    monkeypatch.setattr(B.DeviceReplayBuffer, "next", lambda self, idx: idx)       # (the index kernels need a device)
    FakeDSAC.calls, FakeDSAC.seen = [], []


def _update(algo, buf, n=8):
    algo.policy.is_within_training_step = True
    try:
        return algo.update(buffer=buf, sample_size=n)
    finally:
        algo.policy.is_within_training_step = False


def _live14(algo):
    from tianshou_amd import dsac_cnn as DC

    named = dict(nn.ModuleList([algo.policy, algo.critic, algo.critic2]).named_parameters())
    return [named[k] for k in DC.TIANSHOU_KEYS]


def _sets(algo):
    p = _live14(algo)
    return ((algo.critic_optim, p[:8] + p[10:12]), (algo.critic2_optim, p[:8] + p[12:14]), (algo.policy_optim, p[:10]))


@pytest.mark.parametrize("stacked", [False, True])
def test_hooks_data_flow_and_write_back_with_engine_double(monkeypatch, stacked):
    _patch(monkeypatch)
    algo = _make(*_nets(), auto=True, gamma=0.9, n_step_return_horizon=3)
    buf = _buffer(prio=True, stacked=stacked)
    params = _live14(algo)
    o1, o2 = list(_old(algo.critic_old).parameters()), list(_old(algo.critic2_old).parameters())
    before = [p.detach().clone() for p in params]
    stats = _update(algo, buf)
    # the reference's two policy calls per update draw unused samples: one forward in front of each engine call
    assert FakeDSAC.calls == ["forward", "preprocess", "forward", "update"]
    pre, upd = FakeDSAC.seen
    assert pre == ("preprocess", C_ if stacked else 1, not stacked, 3, 0.9)
    assert upd[1] is not None and upd[1].dtype == torch.float32 and upd[1].shape == (8,)      # PER weights in
    assert upd[2:5] == (3e-4, 1e-4, 1e-3) and upd[6] == 0
    assert type(stats).__name__ == "DiscreteSACTrainingStats"
    assert (stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.alpha, stats.alpha_loss) == (1.5, 2.5, 3.5, 0.75, -0.5)
    prio = buf.weight_updates[-1][1] if hasattr(buf, "weight_updates") else None               # batch.weight out, to the buffer
    if prio is not None:
        np.testing.assert_allclose(np.asarray(prio), np.arange(8) * 0.5 + np.finfo(np.float32).eps)
    for p, b in zip(params, before):                                             # engine -> all fourteen nn.Parameters, once each
        assert torch.allclose(p.detach(), b + 2.0)
    # the ONE lagged trunk into BOTH lagged modules, each lagged head into its own module
    for o, b in zip(o1, before[:8] + before[10:12]):
        assert torch.allclose(o.detach(), b + 0.5)
    for o, b in zip(o2, before[:8] + before[12:14]):
        assert torch.allclose(o.detach(), b + 0.5)
    # three DISTINCT trunk moment sets
    for k, (opt, own) in enumerate(_sets(algo)):
        for p in own:
            st = opt._optim.state[p]
            assert float(st["step"]) == 1.0 and torch.allclose(st["exp_avg"], torch.full_like(st["exp_avg"], 0.125 * (k + 1)))
    assert float(algo.alpha._log_alpha.detach()) == pytest.approx(-0.75)
    st = algo.alpha._optim.state[algo.alpha._log_alpha]
    assert float(st["exp_avg"]) == pytest.approx(0.0625) and float(st["step"]) == 1.0
    # the learning rates are read from the optimizers at every update
    algo.policy_optim._optim.param_groups[0]["lr"] = 7e-4
    algo.alpha._optim.param_groups[0]["lr"] = 5e-3
    _update(algo, buf)
    assert FakeDSAC.seen[-1][2:5] == (7e-4, 1e-4, 5e-3) and FakeDSAC.seen[-1][6] == 1
    algo.critic2_optim._optim.param_groups[0]["lr"] = 9e-4                        # the engine has ONE critic learning rate
    with pytest.raises(NotImplementedError, match="critic_lr"):
        _update(algo, buf)


def test_fixed_alpha_reports_no_alpha_loss_and_plain_buffer_passes_no_weight(monkeypatch):
    _patch(monkeypatch)
    algo = _make(*_nets(), match_rng_stream=False)
    stats = _update(algo, _buffer())
    assert FakeDSAC.calls == ["preprocess", "update"] and FakeDSAC.seen[1][1] is None
    assert stats.alpha_loss is None and stats.alpha == 0.75


def test_state_dict_round_trip_restores_three_moment_sets_lagged_modules_and_alpha(monkeypatch):
    _patch(monkeypatch)
    a = _make(*_nets(), auto=True, match_rng_stream=False)
    buf = _buffer()
    _update(a, buf)
    state = copy.deepcopy(a.state_dict())
    alpha_opt = copy.deepcopy(a.alpha._optim.state_dict())           # AutoAlpha's optimizer lives outside Algorithm._optimizers
    b = _make(*_nets(), auto=True, match_rng_stream=False)
    b.load_state_dict(state)
    b.alpha._optim.load_state_dict(alpha_opt)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    _update(b, buf)
    upd = FakeDSAC.seen[-1]
    # the fresh engine of `b` started from the loaded state: three distinct moment sets, the step count, alpha's moment
    assert upd[5].tolist() == [0.125, 0.25, 0.375] and upd[6] == 1 and upd[7] == pytest.approx(0.0625)
    eng = b._hip_engine
    assert float(eng.log_alpha) == pytest.approx(-1.0 + 0.5)
    la = _live14(a)
    for p, q in zip(_live14(b), la):
        assert torch.allclose(p.detach(), q.detach() + 2.0)
    for mod_a, mod_b in ((a.critic_old, b.critic_old), (a.critic2_old, b.critic2_old)):
        for p, q in zip(_old(mod_b).parameters(), _old(mod_a).parameters()):
            assert torch.allclose(p.detach(), q.detach() + 0.5)
    for k, (opt, own) in enumerate(_sets(b)):
        for p in own:
            assert float(opt._optim.state[p]["step"]) == 2.0
            assert torch.allclose(opt._optim.state[p]["exp_avg"], torch.full_like(p, 0.25 * (k + 1)))


def test_checkpoint_with_differing_lagged_trunks_is_refused(monkeypatch):
    _patch(monkeypatch)
    a = _make(*_nets(), match_rng_stream=False)
    state = copy.deepcopy(a.state_dict())
    key = next(k for k in state if k.startswith("critic2_old") and k.endswith("preprocess.net.1.bias"))
    state[key] = state[key] + 1e-3
    b = _make(*_nets(), match_rng_stream=False)
    b.load_state_dict(state)
    with pytest.raises(NotImplementedError, match="trunks of critic_old and critic2_old differ"):
        _update(b, _buffer())
    assert FakeDSAC.calls == []


@pytest.mark.skipif(not REAL, reason="needs the reference mounted")
def test_standins_have_the_reference_surface():
    """tests/standin_dsac_cnn.py against the real classes: the same parameter names and shapes in the same order, the same RNG
    consumption at construction, the same optimizer membership, the same forward results."""
    ref_shim.install()
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic

    def build(NetC, ActorC, CriticC):
        torch.manual_seed(7)
        net = NetC(C_, H_, W_, action_shape=A_, features_only=True, output_dim_added_layer=HID)
        return (ActorC(preprocess_net=net, action_shape=A_, softmax_output=False), CriticC(preprocess_net=net, last_size=A_),
                CriticC(preprocess_net=net, last_size=A_))

    real, fake = build(DQNet, DiscreteActor, DiscreteCritic), build(SD.DQNet, SD.DiscreteActor, SD.DiscreteCritic)
    obs = np.random.default_rng(0).integers(0, 255, size=(3, C_, H_, W_)).astype(np.uint8)
    for r, f in zip(real, fake):
        pr, pf = dict(r.named_parameters()), dict(f.named_parameters())
        assert list(pr) == list(pf) and all(torch.equal(pr[k], pf[k]) for k in pr)
        yr, yf = r(obs), f(obs)
        assert torch.equal(yr[0] if isinstance(yr, tuple) else yr, yf[0] if isinstance(yf, tuple) else yf)
    a_real = _make(*real, auto=True)
    algo = SD.DiscreteSAC(policy=SD.DiscreteSACPolicy(actor=fake[0]), critic=fake[1], critic2=fake[2], lr=3e-4, critic_lr=1e-4,
                          alpha=SD.AutoAlpha(0.9, -1.0, 1e-3))
    for name in ("policy_optim", "critic_optim", "critic2_optim"):
        n_real = len([p for g in getattr(a_real, name)._optim.param_groups for p in g["params"]])
        assert n_real == len([p for g in getattr(algo, name)._optim.param_groups for p in g["params"]]) == 10
        assert getattr(a_real, name)._max_grad_norm is None and getattr(algo, name)._max_grad_norm is None
    assert {k for k in a_real.state_dict() if k != "_optimizers"} == {k for k in algo.state_dict() if k != "_optimizers"}
    none = SD.DiscreteSAC(policy=SD.DiscreteSACPolicy(actor=fake[0]), critic=fake[1], critic2=None)
    assert none.critic2.preprocess is not fake[1].preprocess                      # critic2=None: a deep copy with its own trunk


def test_argument_checks_come_before_any_hip_call():
    """The new entry points validate on the host first: NULLs, B in [1, 2^24), n_act, hidden, observation size -- safe on a
    GPU-less host (no pointer is dereferenced); the layout is pure host arithmetic."""
    import ctypes as C

    from tianshou_amd import _lib
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    lib.ts_dsac_cnn_param_count.restype = C.c_int64
    i64, f64, dummy = C.c_int64, C.c_double, C.c_void_p(4096)
    out = (C.c_int64 * 11)()
    assert lib.ts_dsac_cnn_layout(i64(4), i64(84), i64(84), i64(6), i64(512), out) == 0
    f, ld, total, trunk = out[0], out[1], out[2], out[3]
    assert (f, ld) == (3136, 32) and trunk == (256 + 1) * 32 + 513 * 64 + 577 * 64 + 3137 * 512 and total == trunk + 3 * 513 * 32
    assert list(out[4:8]) == [0, 8224, 8224 + 32832, 8224 + 32832 + 36928] and list(out[8:11]) == [trunk + k * 513 * 32 for k in range(3)]
    assert lib.ts_dsac_cnn_param_count(i64(4), i64(84), i64(84), i64(6), i64(512)) == total
    for c, h, w, a, hid in ((4, 84, 84, 0, 512), (4, 84, 84, 65, 512), (4, 84, 84, 6, 500), (4, 84, 84, 6, 16), (4, 84, 84, 6, 1056),
                            (4, 20, 84, 6, 512), (0, 84, 84, 6, 512)):
        assert lib.ts_dsac_cnn_param_count(i64(c), i64(h), i64(w), i64(a), i64(hid)) == -1, (c, h, w, a, hid)
    assert lib.ts_dsac_cnn_layout(i64(4), i64(84), i64(84), i64(6), i64(512), None) == _lib.TS_ERR_INVALID_ARG
    for b in (0, -1, 1 << 24):
        assert lib.ts_dsac_cnn_target(dummy, dummy, dummy, None, f64(0.2), i64(b), i64(3), dummy, None) == _lib.TS_ERR_INVALID_ARG
        assert b"batch size" in lib.ts_last_error()
        assert lib.ts_dsac_cnn_critic(dummy, dummy, dummy, None, i64(b), i64(3), dummy, dummy, dummy, dummy, None) == _lib.TS_ERR_INVALID_ARG
        assert lib.ts_dsac_cnn_actor(dummy, dummy, dummy, None, f64(0.2), i64(b), i64(3), dummy, dummy, dummy, dummy,
                                     None) == _lib.TS_ERR_INVALID_ARG
    assert lib.ts_dsac_cnn_target(dummy, dummy, dummy, None, f64(0.2), i64(4), i64(65), dummy, None) == _lib.TS_ERR_INVALID_ARG
    assert lib.ts_dsac_cnn_target(dummy, dummy, None, None, f64(0.2), i64(4), i64(3), dummy, None) == _lib.TS_ERR_INVALID_ARG
    assert b"NULL" in lib.ts_last_error()
    assert lib.ts_dsac_cnn_target(dummy, dummy, dummy, None, f64(float("nan")), i64(4), i64(3), dummy, None) == _lib.TS_ERR_INVALID_ARG
    assert lib.ts_dsac_cnn_critic(dummy, None, dummy, None, i64(4), i64(3), dummy, dummy, dummy, dummy, None) == _lib.TS_ERR_INVALID_ARG
    assert lib.ts_dsac_cnn_forward(None, dummy, i64(4), i64(84), i64(84), i64(6), i64(512), dummy, 1, i64(4), dummy, None) == _lib.TS_ERR_WORKSPACE
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0          # host memory only: never touches a device
    try:
        def fwd(b=4, a=6, hid=512, params=dummy):
            return lib.ts_dsac_cnn_forward(ws, params, i64(4), i64(84), i64(84), i64(a), i64(hid), dummy, 1, i64(b), dummy, None)

        for kw in (dict(b=0), dict(b=1 << 24), dict(a=0), dict(a=65), dict(hid=48), dict(params=None)):
            assert fwd(**kw) == _lib.TS_ERR_INVALID_ARG, kw
        assert lib.ts_dsac_cnn_target_q(ws, dummy, None, None, f64(0.2), i64(4), i64(84), i64(84), i64(6), i64(512), dummy, 1, i64(4),
                                        dummy, None) == _lib.TS_ERR_INVALID_ARG

        from tianshou_amd.sac import SACConfig

        def upd(hp, b=4, grads=None, la=None, step=1):
            return lib.ts_dsac_cnn_update(ws, dummy, dummy, dummy, dummy, la, la, la, i64(step), i64(4), i64(84), i64(84), i64(6),
                                          i64(512), dummy, 1, dummy, dummy, None, i64(b), C.byref(hp), dummy, dummy, grads, None)

        hp = SACConfig().to_c()
        assert upd(hp, b=0) == _lib.TS_ERR_INVALID_ARG and upd(hp, step=0) == _lib.TS_ERR_INVALID_ARG
        auto = SACConfig(auto_alpha=True).to_c()
        assert upd(auto) == _lib.TS_ERR_INVALID_ARG and b"auto alpha" in lib.ts_last_error()
        hp.actor_lr = hp.critic_lr = -1.0
        assert upd(hp) == _lib.TS_ERR_INVALID_ARG and b"needs grads_out" in lib.ts_last_error()
        hp.critic_lr = 1e-3
        assert upd(hp, grads=dummy) == _lib.TS_ERR_INVALID_ARG and b"both learning rates" in lib.ts_last_error()
    finally:
        lib.ts_workspace_destroy(ws)
