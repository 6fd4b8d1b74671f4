"""GPU: lazy write-back against eager write-back, as a differential test of the state layer above the kernels.

Two copies of an algorithm -- the reference-exact twin (`host_batch=True, write_back="eager"`: the torch modules are current
after every update; the hook tests validate it against the oracle) and the default twin (index-only sampling, lazy write-back:
the engine holds the only current parameters, lagged networks and Adam state until somebody reads the torch modules) -- run
the same steps: k = 2 updates (lazy updates pending), one event, the check, one more update, the check again.  The check: every
tensor of `state_dict()` and every torch.optim state entry (incl. `step`) bit-identical in both twins; the collector forward
`policy(batch)` bit-identical; and that forward equal to a float64 recomputation from the twin's torch modules.
HipSAC at the sizes of test_hip_sac_default_mode_equals_the_reference_exact_mode, HipDQN on both of its layouts
(`atari_frames`: the ts_dqn_learn_rows one-call path).  Plus a resumed HipSAC run (defaults: engine noise, device sampling)
against an uninterrupted one."""
import copy
import pickle
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from tests import lazy_twins as LT
from tests import standin as SI

pytestmark = pytest.mark.gpu

READERS = ("algorithm_state_dict", "policy_state_dict", "module_state_dict", "pickle_policy", "hip_sync")
EVENTS = tuple(f"load_then_{r}" for r in READERS) + ("load_then_forward", "algorithm_load", "invalidate_pending",
                                                      "data_edit_invalidate")
ALGOS = ("sac", "dqn_stored_obs_next", "dqn_atari_frames")


class _Twins:
    def __init__(self, which):
        self.which = which
        if which == "sac":
            self.ref, self.lazy = LT.sac_build(host_batch=True, write_back="eager"), LT.sac_build()
            self.bufs = [LT.sac_buffer() for _ in range(2)]
            self.obs = np.random.default_rng(8).normal(size=(16, LT.SAC_OBS)).astype(np.float32)
        else:
            layout = which[len("dqn_"):]
            self.ref, self.lazy = LT.dqn_build(host_batch=True, write_back="eager"), LT.dqn_build()
            self.bufs = [LT.dqn_buffer(layout) for _ in range(2)]
            self.obs = np.random.default_rng(8).integers(0, 256, (8, LT.DQN_C, LT.DQN_H, LT.DQN_W)).astype(np.uint8)
        assert self.lazy.__dict__["_hip_lazy"] and not self.ref.__dict__["_hip_lazy"]
        self.rngs = [np.random.default_rng(9) for _ in range(2)]
        self.u = 0

    def update(self):
        for algo, buf, rng in zip((self.ref, self.lazy), self.bufs, self.rngs):
            first = self.u == 0
            if self.which == "sac":
                LT.sac_fill(buf, rng, 30 if first else 7)
                torch.manual_seed(100 + self.u)                     # update_noise="torch": the same draws in both
                algo.update(buf, LT.SAC_BATCH)
            else:
                LT.dqn_fill(buf, rng, 25 if first else 9)
                algo.update(buf, LT.DQN_BATCH)
        self.u += 1

    @staticmethod
    def module(algo, name):
        return algo.policy.model if name == "model" else getattr(algo.policy if name == "actor" else algo, name)


def _optims(algo):
    if hasattr(algo, "critic2_optim"):
        return [algo.policy_optim._optim, algo.critic_optim._optim, algo.critic2_optim._optim, algo.alpha._optim]
    return [algo.optim._optim]


def _check_torch_state(ref, lazy, where):
    sd_r, sd_l = ref.state_dict(), lazy.state_dict()                # (readers: the lazy twin syncs here)
    assert set(sd_r) == set(sd_l)
    for k, v in sd_r.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(sd_l[k].cpu(), v.cpu()), (where, k)
    for o_r, o_l in zip(_optims(ref), _optims(lazy)):
        p_r = [p for g in o_r.param_groups for p in g["params"]]
        p_l = [p for g in o_l.param_groups for p in g["params"]]
        for i, (a, b) in enumerate(zip(p_r, p_l)):
            s_r, s_l = o_r.state.get(a, {}), o_l.state.get(b, {})
            assert set(s_r) == set(s_l), (where, i)
            for key, v in s_r.items():
                assert torch.equal(torch.as_tensor(s_l[key]).cpu(), torch.as_tensor(v).cpu()), (where, i, key)


def _forward(algo, obs):
    res = algo.policy(SI.Batch(obs=obs, info={}))
    if isinstance(res.logits, tuple):
        return [t.detach().cpu() for t in res.logits]              # SAC: (mu, sigma)
    return [torch.as_tensor(res.logits).detach().cpu()]           # DQN: Q values


def _forward64(algo, obs):
    """The collector forward in float64 with plain torch, from the algorithm's torch modules (after a sync)."""
    algo.hip_sync()
    if hasattr(algo.policy, "actor") and hasattr(algo, "critic2"):
        p = {k: t.detach().double().cpu() for k, t in zip(OS.ACTOR_ORDER, algo.policy.actor.state_dict().values())}
        with torch.no_grad():
            mu, sigma = OS.actor_forward(p, torch.from_numpy(obs).double())
        return [mu, sigma]
    net = SI.DQNet(LT.DQN_C, LT.DQN_H, LT.DQN_W, LT.DQN_ACT).double()
    net.load_state_dict({k: v.detach().double().cpu() for k, v in algo.policy.model.state_dict().items()})
    with torch.no_grad():
        return [net.net(torch.from_numpy(obs).double())]


def _check(tw, where):
    f_r, f_l = _forward(tw.ref, tw.obs), _forward(tw.lazy, tw.obs)
    for a, b in zip(f_r, f_l):
        assert torch.equal(a, b), where
    _check_torch_state(tw.ref, tw.lazy, where)
    want = _forward64(tw.lazy, tw.obs)
    if tw.which == "sac":
        np.testing.assert_allclose(f_l[0].numpy(), want[0].numpy(), rtol=1e-5, atol=2e-6, err_msg=f"{where}: mu")
        np.testing.assert_allclose(f_l[1].numpy(), want[1].numpy(), rtol=1e-5, atol=1e-7, err_msg=f"{where}: sigma")
    else:
        q = want[0].numpy()
        np.testing.assert_allclose(f_l[0].numpy(), q, rtol=1e-5, atol=1e-5 * float(np.abs(q).max()), err_msg=f"{where}: Q")


def _best(tw, name):
    """Weights to load into sub-module `name` of both twins: half of the reference-exact twin's current ones (read without a
    reader of the lazy twin: the eager twin's parameters are current)."""
    mod = tw.module(tw.ref, name)
    return {k: (0.5 * v.detach()).clone() for k, v in mod.named_parameters()}


def _edit_bias(algo, which, delta):
    """A `.data` edit (no version bump) of the bias of the layer the collector forward ends in."""
    bias = algo.policy.actor.mu.model[0].bias if which == "sac" else algo.policy.model.net[3].bias
    bias.data.add_(delta)


@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("which", ALGOS)
def test_lazy_write_back_equals_eager_after(which, event):
    tw = _Twins(which)
    ref, lazy = tw.ref, tw.lazy
    for _ in range(2):
        tw.update()
    assert lazy.__dict__["_hip_stale"]
    if event.startswith("load_then_"):
        reader = event[len("load_then_"):]
        name = "model" if which != "sac" else ("actor" if reader == "forward" else "critic")
        best = _best(tw, name)
        for algo in (ref, lazy):
            tw.module(algo, name).load_state_dict(copy.deepcopy(best))
        assert lazy.__dict__["_hip_stale"]                           # nothing has read the lazy twin yet
        for algo in (ref, lazy):
            mod = tw.module(algo, name)
            if reader == "algorithm_state_dict":
                algo.state_dict()
            elif reader == "policy_state_dict":
                algo.policy.state_dict()
            elif reader == "module_state_dict":
                mod.state_dict()
            elif reader == "pickle_policy":
                pickle.dumps(algo.policy)
            elif reader == "hip_sync":
                algo.hip_sync()
            else:
                _forward(algo, tw.obs)
            if reader != "forward":
                assert all(torch.equal(p.detach(), best[k]) for k, p in mod.named_parameters()), event
    elif event == "algorithm_load":
        ckpt = copy.deepcopy(LT.sac_build().state_dict() if which == "sac" else LT.dqn_build().state_dict())
        for algo in (ref, lazy):
            algo.load_state_dict(copy.deepcopy(ckpt))
        sd = lazy.state_dict()
        for k, v in ckpt.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(sd[k].cpu(), v.cpu()), k
    elif event == "invalidate_pending":
        with pytest.raises(RuntimeError, match="hip_sync"):
            lazy.hip_invalidate()
        assert lazy.__dict__["_hip_stale"] and lazy.__dict__["_hip_engine_obj"] is not None      # nothing was dropped
        _check(tw, f"{event}: after the refusal")
        lazy.hip_sync()
        lazy.hip_invalidate()
        ref.hip_invalidate()
        assert lazy.__dict__["_hip_engine_obj"] is None and ref.__dict__["_hip_engine_obj"] is None
    else:                                                           # data_edit_invalidate: the documented recipe
        lazy.hip_sync()
        for algo in (ref, lazy):
            _edit_bias(algo, which, 0.05)
            algo.hip_invalidate()
        _check(tw, f"{event}: first edit")
        for algo in (ref, lazy):                                    # no engine now: the collector reads the torch modules
            _edit_bias(algo, which, -0.1)
            algo.hip_invalidate()
    _check(tw, event)
    tw.update()
    _check(tw, f"{event}: next update")


@pytest.mark.parametrize("order", ["extra_first", "state_dict_first"])
def test_hip_sac_resumed_run_equals_an_uninterrupted_one(order):
    """The default configuration (engine update noise, device sampling in the collector forward, lazy write-back): 3 updates and
    2 forwards, `state_dict()` + `hip_extra_state()` saved, a fresh object with the same seeds restored (extra state before or
    after `load_state_dict`), 3 more updates and forwards -- bit-identical to 6 uninterrupted updates: statistics, actions,
    parameters, optimizer state; no warning."""
    def build():
        algo = LT.sac_build(update_noise="device")
        assert algo.__dict__["_hip_lazy"] and algo._hip_update_noise == "device" and algo.policy._hip_sampling == "device"
        return algo

    def phase(algo, buf, rng, us, log):
        for u in us:
            LT.sac_fill(buf, rng, 30 if u == 0 else 7)
            s = algo.update(buf, LT.SAC_BATCH)
            log.append(("stats", u, [s.actor_loss, s.critic1_loss, s.critic2_loss, s.alpha, s.alpha_loss]))
            if u != 0:
                res = algo.policy(SI.Batch(obs=obs, info={}))
                log.append(("act", u, res.act.detach().cpu()))

    obs = np.random.default_rng(8).normal(size=(16, LT.SAC_OBS)).astype(np.float32)
    whole, log_w = build(), []
    phase(whole, LT.sac_buffer(), np.random.default_rng(9), range(6), log_w)
    first, log_r = build(), []
    buf, rng = LT.sac_buffer(), np.random.default_rng(9)
    phase(first, buf, rng, range(3), log_r)
    sd, extra = copy.deepcopy(first.state_dict()), first.hip_extra_state()
    # (AutoAlpha's optimizer is outside Algorithm._optimizers and so outside the reference's checkpoint, sac.py:193: saved beside it)
    alpha_optim = copy.deepcopy(first.alpha._optim.state_dict())
    assert extra == {"update_noise_calls": 6, "policy_calls": 2}
    del first
    resumed = build()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        resumed.alpha._optim.load_state_dict(alpha_optim)
        if order == "extra_first":
            resumed.load_hip_extra_state(extra)
        resumed.load_state_dict(sd)
        if order == "state_dict_first":
            resumed.load_hip_extra_state(extra)
        phase(resumed, buf, rng, range(3, 6), log_r)
    assert not [str(w.message) for w in caught if "Hip" in str(w.message) or "tianshou_amd" in (w.filename or "")]
    assert len(log_r) == len(log_w)
    for a, b in zip(log_w, log_r):
        assert a[:2] == b[:2]
        if a[0] == "stats":
            assert a[2] == b[2], a[1]
        else:
            assert torch.equal(a[2], b[2]), a[1]
    _check_torch_state(whole, resumed, "resumed")
    assert resumed.hip_extra_state() == whole.hip_extra_state() == {"update_noise_calls": 12, "policy_calls": 5}
