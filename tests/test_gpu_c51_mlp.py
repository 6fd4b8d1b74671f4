"""GPU: the C51-MLP kernel (ts_c51_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_c51_mlp.py, at the smallest
shapes at which it can go wrong.  Bars: tests/bdqn_common.py.  Inputs (`batch`, asserted on the oracle, every row): every ReLU
pre-activation at least 1e-5 from zero and, outside the tie test, the online network's top two expected values at least 1e-4 apart."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_c51_mlp as OC
from tests import standin_c51_mlp as SC
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import c51_mlp as M
from tianshou_amd.dqn import DQNConfig

pytestmark = pytest.mark.gpu
LR, V = 1e-3, dict(v_min=-2.0, v_max=2.0)
CASES = {     # layers = (obs_dim, trunk, A, N); b70_n2: tile 0 all rows on action A - 1, tile 1 never action 0, tile 2 (6 rows) as drawn
    "b1_n32": dict(layers=(1, (32,), 1, 32), B=1, freq=0, per=False, seed=11),
    "b31_n7": dict(layers=(5, (96, 160), 3, 7), B=31, freq=2, per=True, seed=12),
    "b33_n33": dict(layers=(17, (256,), 1, 33), B=33, freq=2, per=False, seed=13),
    "b70_n2": dict(layers=(5, (64, 32, 32, 64), 3, 2), B=70, freq=0, per=True, seed=14, acts="edges"),
    "b33_a32": dict(layers=(1, (32, 64), 32, 3), B=33, freq=2, per=True, seed=15, clip=0.02),
    "b70_n51": dict(layers=(5, (128,), 2, 51), B=70, freq=2, per=True, seed=16),
    "b33_n256": dict(layers=(4, (32,), 2, 256), B=33, freq=2, per=False, seed=17),      # 104,320 B of LDS (`layout`): the maximal N fits
}


def unsafe_rows(agent, layers, obs, gap):
    """bool[B]: the rows that break the input-selection rule (gap: the online network selects an action on them)."""
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for p in [agent.params] + ([agent.old] if agent.old is not None else []):
        dist, pre, _ = OC.forward(p, layers, obs, want_pre=True)
        for z in pre:
            bad |= z.abs().min(dim=1)[0] < 1e-5
        if gap and p is agent.params and layers[2] > 1:
            top = agent.q(dist).topk(2, dim=1)[0]
            bad |= (top[:, 0] - top[:, 1]) < 1e-4
    return bad


def setup(case, device="cuda"):
    c = CASES[case]
    p0 = {k: p.float() for k, p in OC.init_params(c["layers"], c["seed"]).items()}
    agent = OC.Agent(p0, c["layers"], target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"), **V)
    cfg = DQNConfig(target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"))
    return c, agent, M.C51MlpEngine(c["layers"], M.flat_from_torch(list(p0.values()), *c["layers"], device), cfg, **V)


def batch(c, u, agent, gap=True):
    """The rows of update u; a row that breaks the rule is drawn again, then the rule is asserted.  Returns: the n-step formula on the
    support (mask 20 % zeros, gamma^3, mc ~ 2 N(0, 1)); row 0 is pushed past v_max (even u) or v_min (odd u), one return sits on an atom."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, A, N) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g),
               weight=torch.rand(B, generator=g) * 0.9 + 0.1 if c["per"] else None)
    mask, mc = (torch.rand(B, generator=g) > 0.2).float(), 2 * r(B).double()
    mc[0] = 2.5 if u % 2 == 0 else -2.5
    ret = ((agent.support.view(1, -1) * mask.view(-1, 1)).double() * 0.9 ** 3 + mc.view(-1, 1)).float()
    assert bool((ret[0] > 2).any() or (ret[0] < -2).any()) and (B == 1 or bool((ret > 2).any() and (ret < -2).any()))
    ret[-1, 0] = agent.support[N // 2]
    out["ret"] = ret
    if c.get("acts") == "edges":
        out["act"][:32] = A - 1
        out["act"][32:64] = torch.randint(1, A, (32,), generator=g)
    for key in ("obs", "obs_next"):
        for _ in range(8):
            bad = unsafe_rows(agent, c["layers"], out[key], gap and key == "obs_next")
            out[key][bad] = r(int(bad.sum()), d)
        assert not unsafe_rows(agent, c["layers"], out[key], gap and key == "obs_next").any()
    return out


flat = lambda d, layers: M.flat_from_torch(list(d.values()), *layers, "cpu").double().numpy()  # noqa: E731


def close(got, want, rtol=RTOL, atol=Q_ATOL):
    np.testing.assert_allclose(got.detach().cpu().double().numpy().reshape(-1), np.asarray(want, np.float64).reshape(-1), rtol=rtol, atol=atol)


def check_update(c, agent, eng, b):
    """target_dist, then one update_with_batch: loss, priorities, target_out, parameters, lagged parameters, moments."""
    layers, args = c["layers"], (b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"])
    td = agent.target_dist(b["obs_next"], b["ret"])
    close(eng.target_dist(b["obs_next"], b["ret"]), td)
    loss, prio = agent.update(*args)
    tgt = torch.empty(c["B"], layers[3], dtype=torch.float32, device=eng.device)
    loss_g, prio_g = eng.update_with_batch(*args, target_out=tgt)
    close(loss_g, loss)
    close(prio_g, prio)
    close(tgt, td)
    close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
    if c["freq"]:
        close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
    for got, want in ((eng.adam_m, flat(agent.m, layers)), (eng.adam_v, flat(agent.v, layers))):
        close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)


@pytest.mark.parametrize("case", CASES)
def test_three_updates_against_the_oracle(case):
    c, agent, eng = setup(case)
    layers = c["layers"]
    assert M.layout(layers, c["B"])["lds_bytes"] <= 160 * 1024
    for u in range(3):                                       # freq 2: sync (one network read twice), no sync (two networks), sync
        b = batch(c, u, agent)
        dist = OC.forward(agent.params, layers, b["obs_next"])
        dist_g, q_g, act_g = eng.forward(b["obs_next"])
        close(dist_g, dist)
        close(q_g, agent.q(dist))
        assert torch.equal(act_g.cpu(), agent.q(dist).max(dim=1)[1])
        if u == 0:                                           # the gradient on its own, at unchanged state (a second engine)
            grad, _, _ = agent.gradient(b["obs"], b["act"], (b["obs_next"], b["ret"]), b["weight"])
            other = setup(case)[2]
            g_out = torch.empty(other.P, dtype=torch.float32, device=eng.device)
            other.gradient(b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"], g_out)
            want = flat(grad, layers)
            close(g_out, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == 0 and torch.equal(other.params, eng.params)
        check_update(c, agent, eng, b)
    assert eng.iter == eng.adam_step == 3


def test_saturated_softmax():
    """The last layer scaled up (the scale is found on the oracle): a taken-action probability below 1e-8, so the `+ 1e-8` of the loss
    decides its value and its gradient, with every |logit| below 40."""
    c, agent, eng = setup("b31_n7")
    layers = c["layers"]
    p0, rows = agent.params, torch.arange(c["B"])
    for scale in (4.0, 8.0, 16.0, 32.0, 64.0):               # (powers of two: the scaled parameters are float32 numbers still)
        agent.params = {k: (v * scale if k.startswith("model.model.4") else v) for k, v in p0.items()}
        b = batch(c, 0, agent)                               # the input rule, on the scaled network
        dist, _, logits = OC.forward(agent.params, layers, b["obs"], want_pre=True)
        if float(dist[rows, b["act"]].min()) < 1e-8:
            break
    assert float(dist[rows, b["act"]].min()) < 1e-8 and float(logits.abs().max()) < 40
    eng.params = M.flat_from_torch([v.float() for v in agent.params.values()], *layers, eng.device)
    check_update(c, agent, eng, b)


def test_ties_take_the_first_action():
    """The online head zeroed: every expected value ties, action 0 is selected and row 0 of a different lagged network is projected."""
    c, agent, eng = setup("b31_n7")
    layers = c["layers"]
    agent.old = {k: p.float().double() for k, p in OC.init_params(layers, 99).items()}
    agent.params = {k: (torch.zeros_like(p) if k.startswith("model.model.4") else p) for k, p in agent.params.items()}
    eng.params_old = M.flat_from_torch([p.float() for p in agent.old.values()], *layers, eng.device)
    eng.params = M.flat_from_torch([p.float() for p in agent.params.values()], *layers, eng.device)
    eng.iter = agent.iter = 1                                # no sync at the next update: two networks
    b = batch(c, 0, agent, gap=False)                        # (no gap asked of the tied online network)
    dist, q, act = eng.forward(b["obs_next"])
    assert bool((dist == dist[0, 0, 0]).all()) and bool((q == q[0, 0]).all()) and int(act.abs().max()) == 0
    close(eng.target_dist(b["obs_next"], b["ret"]), agent.target_dist(b["obs_next"], b["ret"]))     # (torch.max: the first index on ties)


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_n51")
    b2 = setup("b70_n51")[2]
    b = batch(c, 0, agent)
    out = [eng.update_with_batch(b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"]) for eng in (a, b2)]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())


def test_hip_c51_mlp_update_with_a_prioritized_buffer():
    """One update() over the stand-ins, n-step 3, prioritized buffer: batch.weight comes back as the oracle's priorities; the write-back
    fills the torch modules and the optimizer state."""
    from tianshou_amd.integration import make_hip_c51_mlp

    layers, E, B, gamma, n_step = (6, (64, 32), 3, 9), 4, 33, 0.95, 3
    torch.manual_seed(21)
    net = SC.build(layers)
    algo = make_hip_c51_mlp(ref=SC)(policy=SC.C51Policy(net, num_atoms=layers[3], **V), lr=LR, gamma=gamma, n_step_return_horizon=n_step,
                                    target_update_freq=2, device="cuda").to("cuda")
    agent = OC.Agent({k: p.detach().cpu() for k, p in net.state_dict().items()}, layers, target_update_freq=2, lr=LR, **V)
    buf = SC.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SC.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)
    ret, _ = O.compute_nstep_return(st, idx, lambda after: agent.support.repeat(len(after), 1).numpy(), gamma, n_step)      # c51.py:120-121
    loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(buf.obs_next[idx]),
                              torch.as_tensor(ret.astype(np.float32)), torch.as_tensor(w, dtype=torch.float32))
    np.testing.assert_allclose(stat.loss, float(loss), rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(prio.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k, p in net.state_dict().items():
        close(p, agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(algo.model_old.module.state_dict()[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    state = algo.optim._optim.state
    for k, p in net.named_parameters():
        close(state[p]["exp_avg"], agent.m[k], rtol=MOM_RTOL, atol=1e-6 * float(agent.m[k].abs().max()))
        assert float(state[p]["step"]) == 1.0
