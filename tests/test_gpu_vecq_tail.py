"""GPU: the last launches of an update as the five families share them (apply_tiles over update_scratch, ts_mlp_tile.h), at the smallest
shape (obs 3, one hidden layer of 32, 2 actions, 3 atoms / 2 samples) and at one row, one full tile, and two tiles with a one-row
second tile.  Every route against the family's oracle, with the bars of the family's own GPU test; the two routes through the clip
(inside update_with_batch, and gradient() + apply_gradient()) against each other bit for bit: they run the same kernels on the same
gradient."""
import pytest
import torch

from tests import test_gpu_c51_mlp as TC
from tests import test_gpu_dqn_mlp as TD
from tests import test_gpu_iqn_mlp as TI
from tests import test_gpu_qrdqn_mlp as TQ
from tests import test_gpu_rainbow_mlp as TR
from tests.bdqn_common import MOM_RTOL, PAR_RTOL
from tianshou_amd.dqn import DQNConfig
from tianshou_amd.iqn import IQNConfig

pytestmark = pytest.mark.gpu
LR, CLIP, FREQ = 1e-3, 0.02, 2
# T: the family's GPU test (its `batch`, `flat`, `close` and oracle); `at`: where grad_out goes among gradient()'s arguments
FAMILIES = {
    "dqn": dict(T=TD, layers=(3, (32,), None, None, 2), at=4, seed=41, double=True),
    "qrdqn": dict(T=TQ, layers=(3, (32,), 2, 3), at=4, seed=42, double=True),
    "c51": dict(T=TC, layers=(3, (32,), 2, 3), at=5, seed=43),
    "rainbow": dict(T=TR, layers=(3, (32,), (), (), 2, 3, True), at=5, seed=44),
    "iqn": dict(T=TI, layers=(3, (32,), 0, 8, (), 2), at=4, seed=45, N=2, N2=2),
}


def make(family, B, clip):
    """-> (case, oracle agent, engine): a lagged network synchronised on every second call, a prioritized batch."""
    c = dict(FAMILIES[family], B=B, freq=FREQ, per=True, clip=clip)
    T, layers = c["T"], c["layers"]
    if family == "qrdqn":
        return TQ.setup(c)
    if family == "rainbow":
        return TR.setup("b1_a1_n2", **c)
    oracle = {"dqn": TD.OM, "c51": TC.OC, "iqn": TI.OI}[family]
    p0 = {k: p.float() for k, p in oracle.init_params(layers, c["seed"]).items()}
    flat0 = T.M.flat_from_torch(list(p0.values()), *layers, "cuda")
    if family == "dqn":                                      # its oracle has no clip: clip_grad_norm_ (algorithm_base.py:496-500) around its gradient
        agent = oracle.Agent(p0, layers, target_update_freq=FREQ, lr=LR)
        if clip:
            raw = agent.gradient

            def clipped(*a):
                grad, loss, td = raw(*a)
                norm = torch.sqrt(sum(g.pow(2).sum() for g in grad.values()))
                return {k: g * torch.clamp(clip / (norm + 1e-6), max=1.0) for k, g in grad.items()}, loss, td
            agent.gradient = clipped
        return c, agent, T.M.DQNMlpEngine(layers, flat0, DQNConfig(target_update_freq=FREQ, lr=LR, max_grad_norm=clip))
    if family == "c51":
        agent = oracle.Agent(p0, layers, target_update_freq=FREQ, lr=LR, max_grad_norm=clip, **TC.V)
        return c, agent, T.M.C51MlpEngine(layers, flat0, DQNConfig(target_update_freq=FREQ, lr=LR, max_grad_norm=clip), **TC.V)
    agent = oracle.Agent(p0, layers, target_update_freq=FREQ, lr=LR, max_grad_norm=clip)
    cfg = IQNConfig(n_cos=layers[3], sample_size=4, online_sample_size=c["N"], target_sample_size=c["N2"], target_update_freq=FREQ, lr=LR,
                    max_grad_norm=clip)
    return c, agent, T.M.IQNMlpEngine(layers, flat0, cfg)


def update_args(family, c, u, agent):
    """The arguments of update u, the same for the oracle's `update` and the engine's `update_with_batch`."""
    b = c["T"].batch(c, u, agent)
    if family in ("c51", "rainbow"):
        return b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"]
    if family == "dqn":
        return b["obs"], b["act"], b["mc"].float(), b["weight"]
    n = 3 if family == "qrdqn" else c["N2"]
    ret = b["mc"].float().reshape(-1, 1) + torch.linspace(-1.0, 1.0, n).reshape(1, -1)
    return (b["obs"], b["act"], ret, b["weight"]) + ((b["tau"],) if family == "iqn" else ())


def check(c, want, got, agent, eng):
    """Loss, priorities, parameters, lagged parameters, moments: the bars of the family's test_three_updates_against_the_oracle."""
    T, layers = c["T"], c["layers"]
    T.close(got[0], want[0])
    T.close(got[1], want[1])
    T.close(eng.params, T.flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
    T.close(eng.params_old, T.flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
    for g, w in ((eng.adam_m, T.flat(agent.m, layers)), (eng.adam_v, T.flat(agent.v, layers))):
        T.close(g, w, rtol=MOM_RTOL, atol=1e-6 * abs(w).max())


@pytest.mark.parametrize("B", (1, 32, 33))
@pytest.mark.parametrize("family", FAMILIES)
def test_the_fused_adam_route_with_and_without_the_lagged_sync(family, B):
    c, agent, eng = make(family, B, None)
    for u in range(2):                                       # update 0 synchronises the lagged network, update 1 does not
        args = update_args(family, c, u, agent)
        before, old = eng.params.clone(), eng.params_old.clone()
        check(c, agent.update(*args), eng.update_with_batch(*args), agent, eng)
        assert torch.equal(eng.params_old, before if u == 0 else old) and not torch.equal(eng.params, before)
    assert eng.iter == eng.adam_step == 2


@pytest.mark.parametrize("B", (1, 32, 33))
@pytest.mark.parametrize("family", FAMILIES)
def test_the_two_routes_through_the_clip_agree_bit_for_bit(family, B):
    c, agent, two = make(family, B, CLIP)
    three, at = make(family, B, CLIP)[2], c["at"]
    for u in range(2):
        args = update_args(family, c, u, agent)
        g2, g3 = (torch.full((two.P,), float("nan"), dtype=torch.float32, device=two.device) for _ in range(2))
        want = agent.update(*args)
        got2 = two.update_with_batch(*args, grad_out=g2)     # the gradient, clip and Adam inside the call
        got3 = three.gradient(*args[:at], g3, *args[at:])    # the gradient on its own, then clip and Adam on it
        three.apply_gradient(g3)
        assert float(g2.norm()) > CLIP                       # (the clip is at work)
        check(c, want, got2, agent, two)
        check(c, want, got3, agent, three)
        assert torch.equal(g2, g3) and torch.equal(got2[0], got3[0]) and torch.equal(got2[1], got3[1])
        for name in ("params", "params_old", "adam_m", "adam_v"):
            assert torch.equal(getattr(two, name), getattr(three, name)), name
        assert two.iter == three.iter == two.adam_step == three.adam_step == u + 1
