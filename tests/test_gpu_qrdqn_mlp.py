"""GPU: the QRDQN-MLP kernels (ts_qrdqn_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_qrdqn_mlp.py, at the
smallest shapes at which they can go wrong.  Bars: tests/bdqn_common.py.  Inputs (`batch`, asserted on the oracle, every row): every ReLU
pre-activation at least 1e-5 from zero and, outside the tie test, the selecting network's top two quantile means at least 1e-4 apart:
float32 cannot flip a comparison.  (The quantile loss is continuous at d = 0 and |d| = 1: no rule is needed there.)"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_qrdqn_mlp as OQ
from tests import standin_qrdqn_mlp as SQ
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import qrdqn_mlp as M
from tianshou_amd.dqn import DQNConfig

pytestmark = pytest.mark.gpu
LR = 1e-3
CASES = {     # layers = (obs_dim, trunk, A, N); every B, N, A N, obs_dim, width, depth and double x freq of the issue once
    "b1_n32": dict(layers=(1, (32,), 1, 32), B=1, double=True, freq=0, per=False, seed=11),
    "b31_n7": dict(layers=(5, (96, 160), 3, 7), B=31, double=True, freq=2, per=True, seed=12),
    "b33_n33": dict(layers=(17, (256,), 1, 33), B=33, double=False, freq=2, per=False, seed=13),
    # tile 0: every row takes action A - 1; tile 1: no row takes action 0; tile 2 (6 rows): as drawn
    "b70_n2": dict(layers=(5, (64, 32, 32, 64), 3, 2), B=70, double=False, freq=0, per=True, seed=14, acts="edges"),
    "b33_a32": dict(layers=(1, (32, 64), 32, 3), B=33, double=True, freq=2, per=True, seed=15, clip=0.02),
    "b70_n200": dict(layers=(5, (128,), 2, 200), B=70, double=True, freq=2, per=True, seed=16),
}


def unsafe_rows(nets, layers, obs, gaps):
    """bool[B]: the rows that break the input-selection rule under one of `nets` (gaps[i]: network i selects an action)."""
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for p, gap in zip(nets, gaps):
        dist, pre = OQ.forward(p, layers, obs, want_pre=True)
        for z in pre:
            bad |= z.abs().min(dim=1)[0] < 1e-5
        if gap and layers[2] > 1:
            top = dist.mean(2).topk(2, dim=1)[0]
            bad |= (top[:, 0] - top[:, 1]) < 1e-4
    return bad


def setup(case, device="cuda"):
    c = CASES[case] if isinstance(case, str) else case
    p0 = {k: p.float() for k, p in OQ.init_params(c["layers"], c["seed"]).items()}
    agent = OQ.Agent(p0, c["layers"], target_update_freq=c["freq"], is_double=c["double"], lr=LR, max_grad_norm=c.get("clip"))
    cfg = DQNConfig(target_update_freq=c["freq"], is_double=c["double"], lr=LR, max_grad_norm=c.get("clip"))
    return c, agent, M.QRDQNMlpEngine(c["layers"], M.flat_from_torch(list(p0.values()), *c["layers"], device), cfg)


def batch(c, u, agent, gap=True):
    """The rows of update u; a row that breaks the rule is drawn again (no seed keeps 10^5 pre-activations away from zero), then the rule is asserted."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, A, _) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g), mask=(torch.rand(B, generator=g) > 0.2).float(),
               gpow=torch.full((B,), 0.9 ** 3, dtype=torch.float64), mc=r(B).double(),
               weight=torch.rand(B, generator=g) * 0.9 + 0.1 if c["per"] else None)
    if c.get("acts") == "edges":
        out["act"][:32] = A - 1
        out["act"][32:64] = torch.randint(1, A, (32,), generator=g)
    readers = {"obs": ([agent.params], [False]),
               "obs_next": ([agent.params] + ([agent.old] if agent.old is not None else []), [gap, gap and not c["double"]])}
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
        dist = OQ.forward(agent.params, layers, b["obs_next"])
        dist_g, q_g, act_g = eng.forward(b["obs_next"])
        close(dist_g, dist)
        close(q_g, dist.mean(2))
        assert torch.equal(act_g.cpu(), dist.mean(2).max(dim=1)[1])
        td = agent.target_dist(b["obs_next"])
        close(eng.target_dist(b["obs_next"]), td)
        ret = (td.float() * b["mask"].reshape(-1, 1)).double() * b["gpow"].reshape(-1, 1) + b["mc"].reshape(-1, 1)
        got = eng.target_returns(b["obs_next"], tuple(b[k].to(dev) for k in ("mask", "gpow", "mc")))
        close(got, ret)
        ret = got.cpu()                                      # both sides continue from the same float32 returns
        if u == 0:                                          # one target on its theta (d = 0: the engine's own float32 theta), one at |d| = 1
            theta = eng.forward(b["obs"])[0].cpu()
            ret[0, 0] = theta[0, b["act"][0], 1]
            ret[-1, 1] = theta[-1, b["act"][-1], 0] + 1.0
            grad, _, _ = agent.gradient(b["obs"], b["act"], ret, b["weight"])      # the gradient on its own, at unchanged state (a second engine)
            other = setup(case)[2]
            g_out = torch.empty(other.P, dtype=torch.float32, device=dev)
            other.gradient(b["obs"], b["act"], ret, b["weight"], g_out)
            want = flat(grad, layers)
            close(g_out, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == 0 and torch.equal(other.params, eng.params)
        loss, prio = agent.update(b["obs"], b["act"], ret, b["weight"])
        loss_g, prio_g = eng.update_with_batch(b["obs"], b["act"], ret, b["weight"])
        print(case, u, "loss", float(loss_g), float(loss), "max rel prio err", float(((prio_g.cpu().double() - prio).abs() / prio).max()))
        close(loss_g, loss)
        close(prio_g, prio)
        close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        if c["freq"]:
            close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        for got, want in ((eng.adam_m, flat(agent.m, layers)), (eng.adam_v, flat(agent.v, layers))):
            close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)
    assert eng.iter == eng.adam_step == 3


def test_ties_take_the_first_action():
    """The online network's last layer zeroed: every quantile mean ties at 0, action 0 wins and the lagged network's row 0 is gathered."""
    c, agent, eng = setup("b31_n7")
    layers = c["layers"]
    old = {k: p.float() for k, p in OQ.init_params(layers, 99).items()}
    eng.params_old = M.flat_from_torch(list(old.values()), *layers, eng.device)
    zeroed = {k: (torch.zeros_like(p) if k.startswith("model.model.4") else p) for k, p in agent.params.items()}
    eng.params = M.flat_from_torch(list(zeroed.values()), *layers, eng.device)
    agent.old = old = {k: p.double() for k, p in old.items()}
    obs = batch(c, 0, agent, gap=False)["obs_next"]           # (no gap asked of the tied online network)
    dist, q, act = eng.forward(obs)
    assert int(dist.abs().max()) == 0 and int(q.abs().max()) == 0 and int(act.abs().max()) == 0
    close(eng.target_dist(obs), OQ.forward(old, layers, obs)[:, 0])


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_n200")
    b2 = setup("b70_n200")[2]
    b = batch(c, 0, agent)
    ret = b["mc"].float().reshape(-1, 1) + torch.linspace(-2, 2, c["layers"][3]).reshape(1, -1)
    out = [eng.update_with_batch(b["obs"], b["act"], ret, b["weight"]) for eng in (a, b2)]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())


def test_hip_qrdqn_mlp_update_with_a_prioritized_buffer():
    """One update() over the stand-ins, n-step 3, prioritized buffer: batch.weight comes back as the oracle's priorities; the write-back
    fills the torch modules and the optimizer state."""
    from tianshou_amd.integration import make_hip_qrdqn_mlp

    layers, E, B, gamma, n_step = (6, (64, 32), 3, 9), 4, 33, 0.95, 3
    torch.manual_seed(21)
    net = SQ.build(layers)
    algo = make_hip_qrdqn_mlp(ref=SQ)(policy=SQ.DiscreteQLearningPolicy(net), lr=LR, gamma=gamma, num_quantiles=layers[3],
                                      n_step_return_horizon=n_step, target_update_freq=2, device="cuda").to("cuda")
    agent = OQ.Agent({k: p.detach().cpu() for k, p in net.state_dict().items()}, layers, target_update_freq=2, lr=LR)
    buf = SQ.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SQ.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)
    ret, _ = O.compute_nstep_return(st, idx, lambda after: agent.target_dist(torch.as_tensor(buf.obs_next[after])).numpy(), gamma, n_step)
    loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(ret.astype(np.float32)),
                              torch.as_tensor(w, dtype=torch.float32))
    np.testing.assert_allclose(stat.loss, float(loss), rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(prio.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k, p in net.state_dict().items():
        close(p, agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(algo.model_old.module.state_dict()[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    state = algo.optim._optim.state
    for k, p in net.named_parameters():
        close(state[p]["exp_avg"], agent.m[k], rtol=MOM_RTOL, atol=1e-6 * float(agent.m[k].abs().max()))
        assert float(state[p]["step"]) == 1.0
