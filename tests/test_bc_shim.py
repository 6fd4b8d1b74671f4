"""CPU: `make_hip_imitation` over the real imitation-learning classes where the reference is mounted and over tests/standin_bc.py
everywhere: the three routes are accepted, every refusal raises NotImplementedError with its message, the stand-ins expose the
real classes' surface, the statistics class and field are the reference's.  No GPU: nothing here runs an update."""
import dataclasses

import numpy as np
import pytest
import torch
from torch import nn

from oracle import oracle_dqn as OD
from oracle import ref_shim
from tests import standin_bc as SB
from tianshou_amd.integration import make_hip_imitation

REAL = ref_shim.reference_available()
SPACES = ["standin"] + (["real"] if REAL else [])


class _Builder:
    """One way to build nets, policies and algorithms over either namespace."""

    def __init__(self, space: str):
        self.space = space
        if space == "real":
            ref_shim.install()
            import gymnasium as gym
            from tianshou.algorithm.imitation import imitation_base as IB
            from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory
            from tianshou.env.atari.atari_network import DQNet
            from tianshou.utils.net.common import Net, Recurrent
            from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousActorProbabilistic

            self.ref, self.IB, self.gym = None, IB, gym
            self._adam, self._rms = AdamOptimizerFactory, RMSpropOptimizerFactory
            self._DQNet, self._Net, self._Recurrent = DQNet, Net, Recurrent
            self._Det, self._Prob = ContinuousActorDeterministic, ContinuousActorProbabilistic
        else:
            self.ref, self.IB = SB, SB

    def hip(self, offline: bool):
        return make_hip_imitation(offline, ref=self.ref)

    def discrete(self, n):
        return self.gym.spaces.Discrete(n) if self.space == "real" else SB.Discrete(n)

    def box(self, act_dim, m=1.0):
        return self.gym.spaces.Box(low=-m, high=m, shape=(act_dim,)) if self.space == "real" else SB.Box(-m, m, (act_dim,))

    def dqnet(self, c=2, h=44, w=36, n_act=3):
        return self._DQNet(c=c, h=h, w=w, action_shape=[n_act]) if self.space == "real" else SB.DQNet(c, h, w, n_act)

    def net(self, obs_dim=4, n_act=2, hidden=(64, 64), activation=nn.ReLU, norm_layer=None):
        if self.space == "real":
            return self._Net(state_shape=(obs_dim,), action_shape=n_act, hidden_sizes=list(hidden), activation=activation,
                             norm_layer=norm_layer)
        return SB.ActionNet(obs_dim, n_act, list(hidden), activation, norm_layer=norm_layer)

    def det(self, obs_dim=17, act_dim=6, hidden=(256, 256), max_action=1.0, activation=nn.ReLU, norm_layer=None):
        if self.space == "real":
            trunk = self._Net(state_shape=(obs_dim,), hidden_sizes=list(hidden), activation=activation, norm_layer=norm_layer)
            return self._Det(preprocess_net=trunk, action_shape=(act_dim,), max_action=max_action)
        return SB.ContinuousActorDeterministic(SB.Net(obs_dim, list(hidden), activation, norm_layer=norm_layer), act_dim, max_action)

    def recurrent(self):
        if self.space == "real":
            return self._Recurrent(layer_num=1, state_shape=(4,), action_shape=2)
        return SB.Recurrent(1, 4, 2, 32)

    def prob(self):
        if self.space == "real":
            return self._Prob(preprocess_net=self._Net(state_shape=(5,), hidden_sizes=[32]), action_shape=(2,))
        return SB.ContinuousActorProbabilistic(SB.Net(5, [32]), 2)

    def algo(self, offline, actor, space, rmsprop=False, **kw):
        policy = self.IB.ImitationPolicy(actor=actor, action_space=space, **kw)
        if self.space == "real":
            optim = (self._rms if rmsprop else self._adam)(lr=1e-3)
            return self.hip(offline)(policy=policy, optim=optim)
        return self.hip(offline)(policy=policy, lr=1e-3, optim=(torch.optim.RMSprop, {}) if rmsprop else None)


@pytest.fixture(params=SPACES)
def mk(request):
    return _Builder(request.param)


@pytest.mark.parametrize("offline", [True, False])
def test_three_routes_are_accepted(mk, offline):
    name = "HipOfflineImitationLearning" if offline else "HipOffPolicyImitationLearning"
    base = mk.IB.OfflineImitationLearning if offline else mk.IB.OffPolicyImitationLearning
    a = mk.algo(offline, mk.dqnet(), mk.discrete(3))
    assert type(a).__name__ == name and isinstance(a, base)
    r = a._hip_route
    assert (r.kind, r.n_out, r.keys) == ("dqnet", 3, OD.TIANSHOU_KEYS)
    r = mk.algo(offline, mk.net(), mk.discrete(2))._hip_route
    assert (r.kind, r.n_out, r.obs_dim, r.sizes, r.activation) == ("discrete", 2, 4, (64, 64), "relu")
    r = mk.algo(offline, mk.net(5, 33, (32,), nn.Tanh), mk.discrete(33))._hip_route          # 33 logits: the 64-column head
    assert (r.kind, r.n_out, r.sizes, r.activation) == ("discrete", 33, (32,), "tanh")
    r = mk.algo(offline, mk.det(max_action=2.5), mk.box(6, 2.5), action_scaling=True, action_bound_method="clip")._hip_route
    assert (r.kind, r.n_out, r.obs_dim, r.sizes, r.max_action) == ("continuous", 6, 17, (256, 256), 2.5)
    r = mk.algo(offline, mk.det(3, 1, (32,), activation=nn.Tanh), mk.box(1), action_bound_method=None)._hip_route
    assert (r.kind, r.n_out, r.sizes, r.activation) == ("continuous", 1, (32,), "tanh")


def test_every_refusal_raises_with_its_message(mk):
    cases = [
        (lambda: mk.algo(True, mk.recurrent(), mk.discrete(2)), r"unsupported actor Recurrent"),
        (lambda: mk.algo(True, mk.prob(), mk.box(2)), r"unsupported actor ContinuousActorProbabilistic"),
        (lambda: mk.algo(True, mk.dqnet(), mk.box(3)), r"DQNet route .* needs a discrete action space"),
        (lambda: mk.algo(False, mk.net(), mk.box(2)), r"discrete MLP route .* needs a discrete action space"),
        (lambda: mk.algo(True, mk.det(), mk.discrete(6)), r"continuous MLP route .* needs a continuous action space"),
        (lambda: mk.algo(True, mk.net(activation=nn.Sigmoid), mk.discrete(2)), r"activation nn.ReLU or nn.Tanh .*Sigmoid"),
        (lambda: mk.algo(False, mk.det(activation=nn.ELU), mk.box(6)), r"activation nn.ReLU or nn.Tanh .*ELU"),
        (lambda: mk.algo(True, mk.net(norm_layer=nn.LayerNorm), mk.discrete(2)), r"norm layer \(LayerNorm\)"),
        (lambda: mk.algo(True, mk.det(norm_layer=nn.LayerNorm), mk.box(6)), r"norm layer \(LayerNorm\)"),
        (lambda: mk.algo(True, mk.net(), mk.discrete(2), rmsprop=True), r"torch.optim.Adam .*RMSprop"),
        (lambda: mk.algo(True, mk.net(n_act=65), mk.discrete(65)), r"2 \.\. 64 outputs, got 65"),
        (lambda: mk.algo(True, mk.det(act_dim=33), mk.box(33)), r"1 \.\. 32 outputs, got 33"),
        (lambda: mk.algo(True, mk.net(hidden=(2048,)), mk.discrete(2)), r"widths up to 1024"),
    ]
    for build, msg in cases:
        with pytest.raises(NotImplementedError, match=msg):
            build()


def test_no_silent_fallback_without_a_gpu(mk):
    """device='cpu': the update raises, it never runs the reference's torch code instead."""
    hip = mk.hip(True)
    a = mk.algo(True, mk.net(), mk.discrete(2))
    a._hip_device = torch.device("cpu")
    batch = mk.IB.Batch(obs=np.zeros((4, 4), np.float32), act=np.zeros(4, np.int64)) if mk.space == "standin" else None
    if batch is None:
        from tianshou.data import Batch

        batch = Batch(obs=np.zeros((4, 4), np.float32), act=np.zeros(4, np.int64), info=Batch())
    before = [p.detach().clone() for p in a.policy.parameters()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a._update_with_batch(batch)
    assert all(torch.equal(p, q) for p, q in zip(a.policy.parameters(), before)) and issubclass(hip, torch.nn.Module)


def test_statistics_are_the_reference_class_with_a_loss_field(mk):
    Stats = mk.IB.ImitationTrainingStats
    assert "loss" in {f.name for f in dataclasses.fields(Stats)}
    assert Stats(loss=0.25).loss == 0.25
    hip = mk.hip(False)
    f = getattr(hip._update_with_batch, "__wrapped__", hip._update_with_batch)
    assert "ImitationTrainingStats" in f.__code__.co_freevars        # what `_update_with_batch` returns is looked up in the namespace
    assert "_preprocess_batch" not in hip.__dict__                    # the base class's hook stays


@pytest.mark.skipif(not REAL, reason="reference not mounted")
def test_standins_have_the_reference_surface():
    real, fake = _Builder("real"), _Builder("standin")
    pairs = [(real.dqnet(), fake.dqnet(), real.discrete(3), fake.discrete(3)),
             (real.net(), fake.net(), real.discrete(2), fake.discrete(2)),
             (real.det(max_action=2.5), fake.det(max_action=2.5), real.box(6, 2.5), fake.box(6, 2.5))]
    for ra, fa, rs, fs in pairs:
        assert list(ra.state_dict().keys()) == list(fa.state_dict().keys())
        assert [tuple(p.shape) for p in ra.parameters()] == [tuple(p.shape) for p in fa.parameters()]
        for offline in (True, False):
            a, b = real.algo(offline, ra, rs), fake.algo(offline, fa, fs)
            assert a.policy.action_type == b.policy.action_type
            assert a._hip_route._replace(keys=[]) == b._hip_route._replace(keys=[]) and a._hip_route.keys == b._hip_route.keys
            assert type(a.optim._optim) is type(b.optim._optim) is torch.optim.Adam
            assert a.optim._max_grad_norm is None and b.optim._max_grad_norm is None
            assert [id(p) for p in a.policy.parameters()] == [id(p) for p in a.policy.actor.parameters()]
            assert [id(p) for p in b.policy.parameters()] == [id(p) for p in b.policy.actor.parameters()]
            for name in ("action_scaling", "action_bound_method", "is_within_training_step"):
                assert hasattr(a.policy, name) and hasattr(b.policy, name), name
    for offline in (True, False):
        A_, B_ = make_hip_imitation(offline), make_hip_imitation(offline, ref=SB)
        assert A_.__name__ == B_.__name__
        for name in ("_update_with_batch", "_engine", "_hip_parts", "_hip_config"):
            fa, fb = getattr(A_, name), getattr(B_, name)
            fa, fb = getattr(fa, "__wrapped__", fa), getattr(fb, "__wrapped__", fb)
            assert fa.__code__.co_code == fb.__code__.co_code, name
