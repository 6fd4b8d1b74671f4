"""GPU: the DQN-MLP kernels (ts_dqn_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_dqn_mlp.py, at the
smallest shapes at which they can go wrong.  Bars: tests/bdqn_common.py.  Inputs (`batch`, asserted on the oracle, every row): every ReLU
pre-activation at least 1e-5 from zero and, outside the tie case, the selecting Q's top two at least 1e-4 apart: float32 cannot flip a comparison."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_dqn_mlp as OM
from tests import standin_dqn_mlp as SM
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import dqn_mlp as M
from tianshou_amd.dqn import DQNConfig

pytestmark = pytest.mark.gpu
LR = 1e-3
CASES = {     # layers = (obs_dim, trunk, Q hidden, V hidden, A); every B, obs_dim, trunk, stream shape, A and double x freq of the issue once
    "b1_a1": dict(layers=(1, (32,), (), (), 1), B=1, double=True, freq=0, huber=None, per=False, seed=11),
    "b31_mixed": dict(layers=(5, (96, 160), (64,), (), 2), B=31, double=True, freq=2, huber=None, per=True, seed=12),
    "b33_wide": dict(layers=(17, (256,), (32, 96), (160,), 5), B=33, double=False, freq=2, huber=0.5, per=False, seed=13),
    "b70_plain": dict(layers=(5, (64, 32), None, None, 32), B=70, double=False, freq=0, huber=None, per=True, seed=14),
    "b70_deep": dict(layers=(17, (96, 160), (32, 96), (160,), 32), B=70, double=True, freq=2, huber=0.5, per=True, seed=15),
    "b33_heads": dict(layers=(1, (256,), (), (), 2), B=33, double=True, freq=0, huber=0.5, per=False, seed=16),
}


def unsafe_rows(nets, layers, obs, gaps):
    """bool[B]: the rows that break the input-selection rule under one of `nets` (gaps[i]: network i selects an action)."""
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for p, gap in zip(nets, gaps):
        q, pre = OM.forward(p, layers, obs, want_pre=True)
        for z in pre:
            bad |= z.abs().min(dim=1)[0] < 1e-5
        if gap and q.shape[1] > 1:
            top = q.topk(2, dim=1)[0]
            bad |= (top[:, 0] - top[:, 1]) < 1e-4
    return bad


def setup(case, device="cuda"):
    c = CASES[case] if isinstance(case, str) else case
    p0 = {k: p.float() for k, p in OM.init_params(c["layers"], c["seed"]).items()}
    agent = OM.Agent(p0, c["layers"], target_update_freq=c["freq"], is_double=c["double"], huber_delta=c["huber"], lr=LR)
    cfg = DQNConfig(target_update_freq=c["freq"], is_double=c["double"], huber_delta=c["huber"], lr=LR)
    eng = M.DQNMlpEngine(c["layers"], M.flat_from_torch(list(p0.values()), *c["layers"], device), cfg) if device else None
    return c, agent, eng


def batch(c, u, agent):
    """The rows of update u; a row that breaks the rule is drawn again (no seed keeps 10^5 pre-activations away from zero), then the rule is asserted."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, _, _, A) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g), mask=(torch.rand(B, generator=g) > 0.2).float(),
               gpow=torch.full((B,), 0.9 ** 3, dtype=torch.float64), mc=r(B).double(),
               weight=torch.rand(B, generator=g) * 0.9 + 0.1 if c["per"] else None)
    readers = {"obs": ([agent.params], [False]),
               "obs_next": ([agent.params] + ([agent.old] if agent.old is not None else []), [True, not c["double"]])}
    for key, (nets, gaps) in readers.items():
        for _ in range(8):
            bad = unsafe_rows(nets, c["layers"], out[key], gaps)
            out[key][bad] = r(int(bad.sum()), d)
        assert not unsafe_rows(nets, c["layers"], out[key], gaps).any()
    return out


def flat(d, layers):
    return M.flat_from_torch(list(d.values()), *layers, "cpu").double().numpy()


def close(got, want, rtol=RTOL, atol=Q_ATOL):
    np.testing.assert_allclose(got.detach().cpu().double().numpy().reshape(-1), np.asarray(want, np.float64).reshape(-1), rtol=rtol, atol=atol)


@pytest.mark.parametrize("case", CASES)
def test_three_updates_against_the_oracle(case):
    c, agent, eng = setup(case)
    layers, dev = c["layers"], eng.device
    for u in range(3):
        b = batch(c, u, agent)
        q_next = OM.forward(agent.params, layers, b["obs_next"])
        close(eng.forward(b["obs_next"])[0], q_next)
        assert torch.equal(eng.forward(b["obs_next"])[1].cpu(), q_next.max(dim=1)[1])
        tq = agent.target_q(b["obs_next"])
        close(eng.target_q(b["obs_next"]), tq)
        ret = (tq * b["mask"]).double() * b["gpow"] + b["mc"]
        got = eng.target_returns(b["obs_next"], tuple(b[k].to(dev) for k in ("mask", "gpow", "mc")))
        close(got, ret)
        ret = got.cpu()                                      # both sides continue from the same float32 returns
        if c["huber"] and u == 0:                           # one row at |td| == delta, one far beyond it
            q_sa = OM.forward(agent.params, layers, b["obs"]).gather(1, b["act"].reshape(-1, 1)).reshape(-1)
            ret[0], ret[1] = float(q_sa[0]) + c["huber"], float(q_sa[1]) - 20 * c["huber"]
        if u == 0:                                          # the gradient on its own, at unchanged state (a second engine)
            grad, _, _ = agent.gradient(b["obs"], b["act"], ret, b["weight"])
            other = setup(case)[2]
            g_out = torch.empty(other.P, dtype=torch.float32, device=dev)
            other.gradient(b["obs"], b["act"], ret, b["weight"], g_out)
            want = flat(grad, layers)
            close(g_out, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == 0 and torch.equal(other.params, eng.params)
        loss, td = agent.update(b["obs"], b["act"], ret, b["weight"])
        loss_g, td_g = eng.update_with_batch(b["obs"], b["act"], ret, b["weight"])
        close(loss_g, loss)
        close(td_g, td)
        close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        if c["freq"]:
            close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        for got, want in ((eng.adam_m, flat(agent.m, layers)), (eng.adam_v, flat(agent.v, layers))):
            close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)
    assert eng.iter == eng.adam_step == 3


def test_ties_take_the_first_action():
    """The online network's last Q layer zeroed: every action ties, the double-Q gather reads the lagged network at index 0."""
    c, agent, eng = setup(dict(CASES["b33_wide"], double=True))
    layers = c["layers"]
    old = {k: p.float() for k, p in OM.init_params(layers, 99).items()}
    eng.params_old = M.flat_from_torch(list(old.values()), *layers, eng.device)
    zeroed = {k: (torch.zeros_like(p) if k.startswith("Q.model.4") else p) for k, p in agent.params.items()}
    eng.params = M.flat_from_torch(list(zeroed.values()), *layers, eng.device)
    agent.old = old = {k: p.double() for k, p in old.items()}
    obs = batch(dict(c, double=False), 0, agent)["obs_next"]      # (no gap asked of the tied online network)
    q, act = eng.forward(obs)
    assert torch.equal(q, q[:, :1].expand_as(q)) and int(act.abs().max()) == 0
    close(eng.target_q(obs), OM.forward(old, layers, obs)[:, 0])


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_deep")
    b2 = setup("b70_deep")[2]
    b = batch(c, 0, agent)
    for eng in (a, b2):
        eng.update_with_batch(b["obs"], b["act"], b["mc"].float(), b["weight"])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())


def test_hip_dqn_mlp_update_with_a_prioritized_buffer():
    """One update() over the stand-ins, n-step 3, prioritized buffer: batch.weight comes back as the oracle's td; the write-back fills the torch modules."""
    from tianshou_amd.integration import make_hip_dqn_mlp

    layers, E, B, gamma, n_step = (6, (64,), (32,), (32,), 3), 4, 33, 0.95, 3
    torch.manual_seed(21)
    net = SM.build(layers)
    algo = make_hip_dqn_mlp(ref=SM)(policy=SM.DiscreteQLearningPolicy(net), lr=LR, gamma=gamma, n_step_return_horizon=n_step,
                                    target_update_freq=2, is_double=True, device="cuda").to("cuda")
    agent = OM.Agent({k: p.detach().cpu() for k, p in net.state_dict().items()}, layers, target_update_freq=2, lr=LR)
    buf = SM.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SM.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)
    ret, _ = O.compute_nstep_return(st, idx, lambda after: agent.target_q(torch.as_tensor(buf.obs_next[after])).numpy().reshape(-1, 1), gamma, n_step)
    loss, td = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(ret.astype(np.float32).reshape(-1)),
                            torch.as_tensor(w, dtype=torch.float32))
    np.testing.assert_allclose(stat.loss, float(loss), rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(td.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k, p in net.state_dict().items():
        close(p, agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(algo.model_old.module.state_dict()[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    state = algo.optim._optim.state
    for k, p in net.named_parameters():
        close(state[p]["exp_avg"], agent.m[k], rtol=MOM_RTOL, atol=1e-6 * float(agent.m[k].abs().max()))
        assert float(state[p]["step"]) == 1.0
