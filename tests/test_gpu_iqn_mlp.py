"""GPU: the IQN-MLP kernels (ts_iqn_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_iqn_mlp.py on the same fractions,
at the smallest shapes at which they can go wrong.  Bars: tests/bdqn_common.py, as tests/test_gpu_qrdqn_mlp.py uses them.  Inputs (`batch`,
asserted on the oracle, every row): every ReLU pre-activation (trunk, embedding, `last`) at least 1e-5 from zero and, outside the tie test,
the selecting network's top two means at least 1e-4 apart: float32 cannot flip a comparison."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_iqn_mlp as OI
from tests import standin_iqn_mlp as SI
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import iqn_mlp as M
from tianshou_amd.iqn import IQNConfig

pytestmark = pytest.mark.gpu
LR = 1e-3
CASES = {     # layers = (obs_dim, trunk, linear feature width or 0 = ReLU features, C, H, A)
    "b1": dict(layers=(1, (32,), 0, 1, (), 1), N=2, N2=2, B=1, freq=0, per=False, seed=31),
    "b31_odd": dict(layers=(5, (96,), 160, 5, (64,), 3), N=3, N2=7, B=31, freq=2, per=True, seed=32),
    "b33_a32": dict(layers=(17, (64, 32), 32, 64, (), 32), N=8, N2=3, B=33, freq=2, per=True, seed=33, clip=0.02),
    # tile 0: every row takes action A - 1; tile 1: no row takes action 0; tile 2 (6 rows): as drawn
    "b70_edges": dict(layers=(5, (64, 32, 32, 64), 0, 64, (32, 64), 3), N=2, N2=2, B=70, freq=0, per=True, seed=34, acts="edges"),
    "b70_n64": dict(layers=(4, (64, 64), 64, 64, (), 2), N=64, N2=64, S=64, B=70, freq=2, per=False, seed=35),
    "b33_wide": dict(layers=(8, (256,), 256, 33, (), 4), N=8, N2=8, B=33, freq=2, per=False, seed=36),
}


def unsafe_rows(p, layers, obs, tau, gap):
    lg, pre = OI.forward(p, layers, obs, tau, want_pre=True)
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for z in pre:
        bad |= z.abs().min(dim=1)[0] < 1e-5
    if gap and layers[5] > 1:
        top = lg.mean(2).topk(2, dim=1)[0]
        bad |= (top[:, 0] - top[:, 1]) < 1e-4
    return bad


def setup(case, device="cuda"):
    c = CASES[case]
    p0 = {k: p.float() for k, p in OI.init_params(c["layers"], c["seed"]).items()}
    agent = OI.Agent(p0, c["layers"], target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"))
    cfg = IQNConfig(n_cos=c["layers"][3], sample_size=c.get("S", 4), online_sample_size=c["N"], target_sample_size=c["N2"],
                    target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"))
    return c, agent, M.IQNMlpEngine(c["layers"], M.flat_from_torch(list(p0.values()), *c["layers"], device), cfg)


def batch(c, u, agent, gap=True):
    """The rows and fractions of update u; a row that breaks the rule gets its observation and fractions drawn again, then the rule is asserted."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, _, _, _, A) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    f = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g), mask=(f(B) > 0.2).float(),
               gpow=torch.full((B,), 0.9 ** 3, dtype=torch.float64), mc=r(B).double(), weight=f(B) * 0.9 + 0.1 if c["per"] else None,
               tau=f(B, c["N"]), tau_online=f(B, c["N"]), tau_target=f(B, c["N2"]) if agent.old is not None else None)
    if c.get("acts") == "edges":
        out["act"][:32] = A - 1
        out["act"][32:64] = torch.randint(1, A, (32,), generator=g)
    readers = {"obs": [(agent.params, "tau", False)], "obs_next": [(agent.params, "tau_online", gap)]}
    if agent.old is not None:
        readers["obs_next"].append((agent.old, "tau_target", False))
    unsafe = lambda key: sum(unsafe_rows(p, c["layers"], out[key], out[t], gp) for p, t, gp in readers[key]) > 0  # noqa: E731
    for key in readers:
        for _ in range(8):
            bad = unsafe(key)
            out[key][bad] = r(int(bad.sum()), d)
            for _, t, _ in readers[key]:
                out[t][bad] = f(int(bad.sum()), out[t].shape[1])
        assert not unsafe(key).any()
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
        lg = OI.forward(agent.params, layers, b["obs_next"], b["tau_online"])
        lg_g, q_g, act_g = eng.forward(b["obs_next"], tau=b["tau_online"])
        close(lg_g, lg)
        close(q_g, lg.mean(2))
        assert torch.equal(act_g.cpu(), lg.mean(2).max(dim=1)[1]) and torch.equal(eng.last_tau.cpu(), b["tau_online"])
        nd = agent.next_dist(b["obs_next"], b["tau_online"], b["tau_target"])
        close(eng.next_dist(b["obs_next"], b["tau_online"], b["tau_target"]), nd)
        ret = (nd.float() * b["mask"].reshape(-1, 1)).double() * b["gpow"].reshape(-1, 1) + b["mc"].reshape(-1, 1)
        got = eng.target_returns(b["obs_next"], tuple(b[k].to(dev) for k in ("mask", "gpow", "mc")), b["tau_online"], b["tau_target"])
        close(got, ret)
        ret = got.cpu()                                      # both sides continue from the same float32 returns
        if u == 0:                                          # one target on its theta (d = 0: the engine's own float32 theta), one at |d| = 1
            theta = eng.forward(b["obs"], tau=b["tau"])[0].cpu()
            ret[0, 0] = theta[0, b["act"][0], 1]
            ret[-1, 1] = theta[-1, b["act"][-1], 0] + 1.0
            grad, _, _ = agent.gradient(b["obs"], b["act"], ret, b["weight"], b["tau"])      # the gradient on its own (a second engine)
            other = setup(case)[2]
            g_out = torch.empty(other.P, dtype=torch.float32, device=dev)
            other.gradient(b["obs"], b["act"], ret, b["weight"], g_out, tau=b["tau"])
            want = flat(grad, layers)
            close(g_out, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == 0 and torch.equal(other.params, eng.params) and int(other.adam_v.abs().max()) == 0
        loss, prio = agent.update(b["obs"], b["act"], ret, b["weight"], b["tau"])
        loss_g, prio_g = eng.update_with_batch(b["obs"], b["act"], ret, b["weight"], tau=b["tau"])
        close(loss_g, loss)
        close(prio_g, prio)
        close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        if c["freq"]:
            close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        for got, want in ((eng.adam_m, flat(agent.m, layers)), (eng.adam_v, flat(agent.v, layers))):
            close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)
    assert eng.iter == eng.adam_step == 3


def test_ties_take_the_first_action():
    """The online network's final Linear zeroed: every q ties at 0, action 0 wins and the lagged network's column 0 is gathered."""
    c, agent, eng = setup("b31_odd")
    layers = c["layers"]
    old = {k: p.float() for k, p in OI.init_params(layers, 99).items()}
    eng.params_old = M.flat_from_torch(list(old.values()), *layers, eng.device)
    zeroed = {k: (torch.zeros_like(p) if k.startswith("last.model.2") else p) for k, p in agent.params.items()}
    eng.params = M.flat_from_torch(list(zeroed.values()), *layers, eng.device)
    agent.old = old = {k: p.double() for k, p in old.items()}
    b = batch(c, 0, agent, gap=False)                         # (no gap asked of the tied online network)
    lg, q, act = eng.forward(b["obs_next"], tau=b["tau_online"])
    assert int(lg.abs().max()) == 0 and int(q.abs().max()) == 0 and int(act.abs().max()) == 0
    close(eng.next_dist(b["obs_next"], b["tau_online"], b["tau_target"]), OI.forward(old, layers, b["obs_next"], b["tau_target"])[:, 0])


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_n64")
    b2 = setup("b70_n64")[2]
    b = batch(c, 0, agent)
    ret = b["mc"].float().reshape(-1, 1) + torch.linspace(-2, 2, c["N2"]).reshape(1, -1)
    out = [eng.update_with_batch(b["obs"], b["act"], ret, b["weight"], tau=b["tau"]) for eng in (a, b2)]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())


def test_hip_iqn_mlp_update_with_a_prioritized_buffer():
    """One update() over the stand-ins, n-step 3, prioritized buffer, the engine's own fractions (replayed by the oracle): batch.weight
    comes back as the oracle's priorities; the write-back fills the torch modules and the optimizer state."""
    from tianshou_amd.integration import make_hip_iqn_mlp

    layers, E, B, gamma, n_step = (6, (64, 32), 64, 9, (32,), 3), 4, 33, 0.95, 3
    torch.manual_seed(21)
    net = SI.build(layers)
    algo = make_hip_iqn_mlp(ref=SI)(policy=SI.IQNPolicy(model=net, sample_size=4, online_sample_size=5, target_sample_size=7), lr=LR,
                                    gamma=gamma, n_step_return_horizon=n_step, target_update_freq=2, device="cuda", hip_seed=5).to("cuda")
    agent = OI.Agent({k: p.detach().cpu() for k, p in net.state_dict().items()}, layers, target_update_freq=2, lr=LR)
    buf = SI.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SI.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    eng = algo._hip_engine
    tau_o, tau_t, tau = eng.last_tau_online.cpu(), eng.last_tau_target.cpu(), eng.last_tau.cpu()
    assert tau_o.shape == (B, 5) and tau_t.shape == (B, 7) and tau.shape == (B, 5) and eng.tau_counter == 3
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)
    ret, _ = O.compute_nstep_return(st, idx, lambda after: agent.next_dist(torch.as_tensor(buf.obs_next[after]), tau_o, tau_t).numpy(), gamma, n_step)
    loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(ret.astype(np.float32)),
                              torch.as_tensor(w, dtype=torch.float32), tau)
    np.testing.assert_allclose(stat.loss, float(loss), rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(prio.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k, p in net.state_dict().items():
        close(p, agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(algo.model_old.module.state_dict()[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    state = algo.optim._optim.state
    for k, p in net.named_parameters():
        close(state[p]["exp_avg"], agent.m[k], rtol=MOM_RTOL, atol=1e-6 * float(agent.m[k].abs().max()))
        assert float(state[p]["step"]) == 1.0
