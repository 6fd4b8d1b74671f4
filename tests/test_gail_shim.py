"""CPU: the HipGAIL drop-in (tianshou_amd.integration.make_hip_gail) without an engine -- over the real reference classes where
the reference is mounted, over tests/standin_gail.py otherwise: the class it builds, what the constructor refuses, the parts of
the state path, the checkpoint format; and tests/standin_gail.py against the real class."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import standin_gail as SG

REAL = ref_shim.reference_available()
OBS, ACT = 7, 3


def _expert(n=20, seed=3):
    rng = np.random.default_rng(seed)
    obs, act = rng.normal(size=(n, OBS)).astype(np.float32), rng.normal(size=(n, ACT)).astype(np.float32)
    if not REAL:
        return SG.ExpertBuffer(obs, act, random_seed=5)
    from tianshou.data import Batch, ReplayBuffer

    buf = ReplayBuffer(n, random_seed=5)
    for t in range(n):
        buf.add(Batch(obs=obs[t], act=act[t], rew=0.0, terminated=False, truncated=False, obs_next=obs[t]))
    return buf


def _make(disc=None, hidden_d=(48, 80, 32), disc_act=nn.ReLU, discrete=False, **kw):
    """HipGAIL over real classes or stand-ins: actor / critic Net[64, 64] tanh, a discriminator on its own trunk."""
    from tianshou_amd.integration import make_hip_gail

    kw.setdefault("device", "cpu")
    kw.setdefault("policy_forward", "torch")
    if REAL:
        ref_shim.install()
        import gymnasium as gym
        from torch.distributions import Independent, Normal
        from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy
        from tianshou.algorithm.optim import AdamOptimizerFactory
        from tianshou.utils.net.common import Net
        from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic

        actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(OBS,), hidden_sizes=[64, 64], activation=nn.Tanh),
                                             action_shape=(ACT,), unbounded=True)
        critic = ContinuousCritic(preprocess_net=Net(state_shape=(OBS,), hidden_sizes=[64, 64], activation=nn.Tanh))
        if disc is None:
            disc = ContinuousCritic(preprocess_net=Net(state_shape=(OBS,), action_shape=(ACT,), hidden_sizes=list(hidden_d),
                                                       activation=disc_act, concat=True))
        space = gym.spaces.Discrete(4) if discrete else gym.spaces.Box(low=-1.0, high=1.0, shape=(ACT,))
        policy = ProbabilisticActorPolicy(actor=actor, dist_fn=lambda ls: Independent(Normal(*ls), 1), action_space=space,
                                          action_scaling=not discrete, action_bound_method="clip" if not discrete else None)
        parts = dict(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=3e-4), expert_buffer=_expert(), disc_net=disc,
                     disc_optim=AdamOptimizerFactory(lr=1e-3), disc_update_num=3)
        if kw.pop("plain_reference", False):
            from tianshou.algorithm.imitation.gail import GAIL

            return GAIL(**parts)
        return make_hip_gail()(**parts, **kw)
    actor = SG.ContinuousActorProbabilistic(SG.Net(OBS, [64, 64], nn.Tanh), ACT)
    critic = SG.ContinuousCritic(SG.Net(OBS, [64, 64], nn.Tanh))
    if disc is None:
        disc = SG.ContinuousCritic(SG.Net(OBS + ACT, list(hidden_d), disc_act))

    class Discrete:
        n = 4

    policy = SG.Policy(actor, action_space=Discrete() if discrete else SG.Box(-1.0, 1.0, (ACT,)))
    return make_hip_gail(ref=SG)(policy=policy, critic=critic, expert_buffer=_expert(), disc_net=disc, disc_lr=1e-3,
                                 disc_update_num=3, lr=3e-4, **kw)


def test_class_and_parts():
    algo = _make()
    assert type(algo).__name__ == "HipGAIL" and algo.disc_update_num == 3 and algo.action_dim == ACT
    assert algo._hip_disc == ([48, 80, 32], "relu") and algo._hip_perms == "device"
    parts = algo._hip_parts()
    assert [p.name for p in parts] == ["params", "disc"] and parts[1].holder == "gail" and parts[1].step == "optim_step"
    assert parts[0].holder is None and parts[0].step == "adam_step"           # the actor-critic part is HipPPO's, unchanged
    assert parts[1].optim is algo.disc_optim and len(parts[1].params) == 8
    assert [tuple(p.shape) for p in parts[1].params] == [(48, OBS + ACT), (48,), (80, 48), (80,), (32, 80), (32,), (1, 32), (1,)]
    if REAL:
        from tianshou.algorithm.imitation.gail import GAIL
        from tianshou.algorithm.modelfree.ppo import PPO

        assert isinstance(algo, GAIL) and isinstance(algo, PPO)


def test_constructor_refusals_name_what_was_found():
    with pytest.raises(NotImplementedError, match="data_parallel"):
        _make(data_parallel=True)
    with pytest.raises(NotImplementedError, match="Discrete"):
        _make(discrete=True)
    mk_net = (lambda h, **k: SG.Net(OBS + ACT, h, nn.Tanh, **k))
    if REAL:
        from tianshou.utils.net.common import Net

        mk_net = lambda h, **k: Net(state_shape=(OBS + ACT,), hidden_sizes=h, activation=nn.Tanh, **k)  # noqa: E731
    Critic = SG.ContinuousCritic
    if REAL:
        from tianshou.utils.net.continuous import ContinuousCritic as Critic
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        _make(disc=Critic(preprocess_net=mk_net([32, 32], norm_layer=nn.LayerNorm)) if REAL else Critic(mk_net([32, 32], norm_layer=nn.LayerNorm)))
    with pytest.raises(NotImplementedError, match="one output .found 2"):
        _make(disc=nn.Sequential(nn.Linear(OBS + ACT, 16), nn.Tanh(), nn.Linear(16, 2)))
    with pytest.raises(NotImplementedError, match="Conv1d"):
        _make(disc=nn.Sequential(nn.Conv1d(1, 1, 1), nn.Linear(OBS + ACT, 1), nn.Linear(1, 1)))
    with pytest.raises(ValueError, match="obs_dim \\+ act_dim"):
        _make(disc=nn.Sequential(nn.Linear(OBS, 16), nn.Tanh(), nn.Linear(16, 1)))
    # a bare chain with one output is accepted
    assert _make(disc=nn.Sequential(nn.Linear(OBS + ACT, 16), nn.Tanh(), nn.Linear(16, 1)))._hip_disc == ([16], "tanh")


def test_state_dict_is_the_reference_format_and_round_trips():
    a, b = _make(), _make()
    sd = a.state_dict()
    assert any(k.startswith("disc_net.") for k in sd) and len(sd["_optimizers"]) == 2
    assert not any("hip" in k for k in sd)
    b.load_state_dict(a.state_dict(), strict=True)          # (the reference's load pops `_optimizers` from the dict it is given)
    for p, q in zip(a.disc_net.parameters(), b.disc_net.parameters()):
        assert torch.equal(p, q)
    if REAL:                                     # ... and loads into the reference class itself, strictly, and back
        ref = _make(plain_reference=True)
        assert type(ref).__name__ == "GAIL"
        ref.load_state_dict(a.state_dict(), strict=True)
        for p, q in zip(a.disc_net.parameters(), ref.disc_net.parameters()):
            assert torch.equal(p, q)
        b.load_state_dict(ref.state_dict(), strict=True)


@pytest.mark.skipif(not REAL, reason="the reference is not mounted")
def test_standin_matches_the_real_class():
    """Same state_dict keys (incl. the optimizer list's order and length) and the attributes the hooks read."""
    real = _make()
    actor = SG.ContinuousActorProbabilistic(SG.Net(OBS, [64, 64], nn.Tanh), ACT)
    critic = SG.ContinuousCritic(SG.Net(OBS, [64, 64], nn.Tanh))
    disc = SG.ContinuousCritic(SG.Net(OBS + ACT, [48, 80, 32], nn.ReLU))
    rng = np.random.default_rng(3)
    eb = SG.ExpertBuffer(rng.normal(size=(20, OBS)), rng.normal(size=(20, ACT)), random_seed=5)
    sg = SG.GAIL(policy=SG.Policy(actor, action_space=SG.Box(-1.0, 1.0, (ACT,))), critic=critic, expert_buffer=eb, disc_net=disc,
                 disc_update_num=3)
    sd_r, sd_s = real.state_dict(), sg.state_dict()
    assert set(sd_r) == set(sd_s) and len(sd_r["_optimizers"]) == len(sd_s["_optimizers"]) == 2
    for k in sd_s:
        if k != "_optimizers":
            assert sd_r[k].shape == sd_s[k].shape, k
    for name in ("disc_net", "disc_optim", "disc_update_num", "expert_buffer", "action_dim", "optim", "critic", "ret_rms"):
        assert hasattr(real, name) and hasattr(sg, name), name
    assert sg.action_dim == real.action_dim
    assert [len(o["param_groups"][0]["params"]) for o in sd_r["_optimizers"]] == [len(o["param_groups"][0]["params"]) for o in sd_s["_optimizers"]]
    # the expert stand-in draws what the real buffer draws, and exposes the same storage
    rb = real.expert_buffer
    assert len(rb) == len(eb) and np.asarray(rb.obs).shape == eb.obs.shape and np.asarray(rb.act).shape == eb.act.shape
    for bsz in (3, 5, 3):
        np.testing.assert_array_equal(rb.sample_indices(bsz), eb.sample_indices(bsz))
    np.testing.assert_allclose(np.asarray(rb.obs), eb.obs)


def test_argument_checks_come_before_any_launch():
    """ts_gail_disc_steps / ts_gail_reward / ts_gail_loss refuse bad arguments before any HIP call (so this runs without a GPU)."""
    import ctypes as C

    from tianshou_amd import _lib

    lib = _lib.load()
    net = _lib.NetDesc.make(OBS + ACT, [64, 64], "tanh")
    one = C.c_void_p(8)                       # a non-NULL pointer that is never dereferenced: the call returns before any launch
    null, ws = C.c_void_p(0), _lib_ws()

    def steps(**over):
        a = dict(ws=ws, disc=one, net=C.byref(net), n=10, bsz=5, n_exp_rows=4, step0=1, act_dim=ACT, route=0, perm=one)
        a.update(over)
        return lib.ts_gail_disc_steps(a["ws"], a["disc"], one, one, _lib.i64(a["step0"]), a["net"], _lib.i64(a["act_dim"]), one, one,
                                      a["perm"], _lib.i64(a["n"]), one, one, _lib.i64(a["n_exp_rows"]), one, _lib.i64(a["bsz"]),
                                      C.c_int32(0), _lib.f64(1e-3), _lib.f64(0.9), _lib.f64(0.999), _lib.f64(1e-8), _lib.f64(0),
                                      _lib.f64(0.99), _lib.f64(0), C.c_int32(0), _lib.f64(0), C.c_int32(a["route"]), one, null, null)

    assert steps(ws=null) == -5
    for over in (dict(disc=null), dict(net=null), dict(perm=null), dict(bsz=0), dict(n=4), dict(n_exp_rows=0), dict(step0=0),
                 dict(act_dim=0), dict(act_dim=OBS + ACT), dict(route=3)):
        assert steps(**over) == -1, over
    ln = _lib.NetDesc.make(OBS + ACT, [64, 64], "tanh", _lib.NetDesc.LAYERNORM)
    assert steps(net=C.byref(ln)) == -4
    relu = _lib.NetDesc.make(OBS + ACT, [64, 64], "relu")
    wide = _lib.NetDesc.make(33, [64, 64], "tanh")
    assert steps(net=C.byref(relu), route=2) == -4 and steps(net=C.byref(wide), route=2, act_dim=3) == -4
    assert lib.ts_gail_loss(ws, one, _lib.i64(0), _lib.i64(3), one, one, null) == -1
    assert lib.ts_gail_loss(ws, null, _lib.i64(3), _lib.i64(3), one, one, null) == -1
    assert lib.ts_gail_reward(ws, one, C.byref(net), _lib.i64(ACT), one, one, _lib.i64(0), one, null, C.c_int32(0), null) == -1
    assert lib.ts_gail_reward(ws, one, C.byref(relu), _lib.i64(ACT), one, one, _lib.i64(4), one, null, C.c_int32(2), null) == -4


def _lib_ws():
    """A workspace handle for argument checks: a real one needs a device, so a non-NULL placeholder stands in (the entry points
    only compare it with NULL before the checks under test return)."""
    import ctypes as C

    return C.c_void_p(8)
