"""GPU: the Rainbow-MLP kernel (ts_rainbow_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_rainbow_mlp.py, at the smallest shapes
at which it can go wrong.  Bars: tests/bdqn_common.py.  Inputs (`batch`, asserted on the oracle, every row, each network under its own noise): every ReLU
pre-activation at least 1e-5 from zero and, outside the tie test, the online network's top two expected values at least 1e-4 apart."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_rainbow_mlp as OR
from tests import standin_rainbow_mlp as SR
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import rainbow_mlp as M
from tianshou_amd.dqn import DQNConfig

pytestmark = pytest.mark.gpu
LR, V = 1e-3, dict(v_min=-2.0, v_max=2.0)
CASES = {     # layers = (obs_dim, trunk, Q hidden, V hidden, A, N, noisy); b70_n51: tile 0 all rows on action A - 1, tile 1 never action 0
    "b1_a1_n2": dict(layers=(1, (32,), (), (), 1, 2, True), B=1, freq=0, per=False, seed=11),
    "b31_n3": dict(layers=(5, (96, 160), (64,), (), 3, 3, True), B=31, freq=2, per=True, seed=12),
    "b33_n33": dict(layers=(17, (256,), (), (32,), 2, 33, True), B=33, freq=2, per=False, seed=13),
    "b70_n51": dict(layers=(5, (64, 32), (32,), (96,), 3, 51, True), B=70, freq=2, per=True, seed=14, acts="edges"),
    "b33_a32": dict(layers=(3, (32, 64), (), (), 32, 3, True), B=33, freq=2, per=True, seed=15, clip=0.02),
    "b33_n256": dict(layers=(4, (32,), (), (), 2, 256, True), B=33, freq=0, per=False, seed=16),     # 137,472 B of LDS: the maximal N fits
    "b31_plain": dict(layers=(5, (64,), (32,), (), 3, 7, False), B=31, freq=2, per=True, seed=17),
}


def unsafe_rows(agent, layers, obs, gap):
    """bool[B]: the rows that break the input-selection rule (gap: the online network selects an action on them)."""
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for p, e in [(agent.params, agent.noise)] + ([(agent.old, agent.noise_old)] if agent.old is not None else []):
        dist, pre, _ = OR.forward(p, e, layers, obs, want_pre=True)
        for z in pre:
            bad |= z.abs().min(dim=1)[0] < 1e-5
        if gap and p is agent.params and layers[4] > 1:
            top = agent.q(dist).topk(2, dim=1)[0]
            bad |= (top[:, 0] - top[:, 1]) < 1e-4
    return bad


def setup(case, device="cuda", **over):
    c = {**CASES[case], **over}
    layers = c["layers"]
    p0 = {k: p.float() for k, p in OR.init_params(layers, c["seed"]).items()}
    eps = OR.draw_eps(layers, c["seed"]) if layers[6] else None
    agent = OR.Agent(p0, layers, eps, target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"), **V)
    cfg = DQNConfig(target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"))
    noise = M.noise_from_torch(list(eps.values()), *layers, device) if eps else None
    return c, agent, M.RainbowMlpEngine(layers, M.flat_from_torch(list(p0.values()), *layers, device), noise, cfg, **V)


def renoise(c, u, agent, eng, zero=False):
    """rainbow.py:97-100 before update u: fresh, distinct noise for the online and for the lagged network, on both sides."""
    if not c["layers"][6]:
        return
    new, old = (OR.draw_eps(c["layers"], 1000 * c["seed"] + 2 * u + i) for i in (0, 1))
    if zero:
        new, old = ({k: torch.zeros_like(e) for k, e in d.items()} for d in (new, old))
    agent.noise, agent.noise_old = new, old if agent.old is not None else None
    eng.set_noise(*(M.noise_from_torch(list(d.values()), *c["layers"], eng.device) for d in (new, old)))


def batch(c, u, agent, gap=True):
    """The rows of update u (tests/test_gpu_c51_mlp.py's): a row that breaks the rule is drawn again, then the rule is asserted; row 0's returns leave the support."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, _, _, A, N, _) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g),
               weight=torch.rand(B, generator=g) * 0.9 + 0.1 if c["per"] else None)
    mask, mc = (torch.rand(B, generator=g) > 0.2).float(), 2 * r(B).double()
    mc[0] = 2.5 if u % 2 == 0 else -2.5
    ret = ((agent.support.view(1, -1) * mask.view(-1, 1)).double() * 0.9 ** 3 + mc.view(-1, 1)).float()
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


def gradient_of(eng, b):
    g_out = torch.empty(eng.P, dtype=torch.float32, device=eng.device)
    eng.gradient(b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"], g_out)
    return g_out


def check_update(c, agent, eng, b):
    """target_dist, then one update_with_batch: loss, priorities, target_out, parameters, lagged parameters and noise, moments."""
    layers, args = c["layers"], (b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"])
    td = agent.target_dist(b["obs_next"], b["ret"])
    close(eng.target_dist(b["obs_next"], b["ret"]), td)
    synced = c["freq"] and agent.iter % c["freq"] == 0
    loss, prio = agent.update(*args)
    tgt = torch.empty(c["B"], layers[5], dtype=torch.float32, device=eng.device)
    loss_g, prio_g = eng.update_with_batch(*args, target_out=tgt)
    close(loss_g, loss)
    close(prio_g, prio)
    close(tgt, td)
    close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
    if c["freq"]:
        close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        assert not layers[6] or torch.equal(eng.noise_old, eng.noise) == bool(synced)
    for got, want in ((eng.adam_m, flat(agent.m, layers)), (eng.adam_v, flat(agent.v, layers))):
        close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)


@pytest.mark.parametrize("case", CASES)
def test_three_updates_against_the_oracle(case):
    c, agent, eng = setup(case)
    layers = c["layers"]
    for u in range(3):                                       # freq 2: sync (one network read once), no sync (two networks, two noises), sync
        renoise(c, u, agent, eng)
        b = batch(c, u, agent)
        dist = OR.forward(agent.params, agent.noise, layers, b["obs_next"])
        dist_g, q_g, act_g = eng.forward(b["obs_next"])
        close(dist_g, dist)
        close(q_g, agent.q(dist))
        assert torch.equal(act_g.cpu(), agent.q(dist).max(dim=1)[1])
        if u == 0:                                           # the gradient on its own, at unchanged state (a second engine)
            grad, _, _ = agent.gradient(b["obs"], b["act"], (b["obs_next"], b["ret"]), b["weight"])
            other = setup(case)[2]
            other.set_noise(eng.noise, eng.noise_old)
            g_out, want = gradient_of(other, b), flat(grad, layers)
            close(g_out, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == 0 and torch.equal(other.params, eng.params)
            if layers[4] == 1:                               # logits = V: nothing reaches the Q stream
                named = dict(zip(M.state_dict_keys(layers), M.flat_to_torch(g_out, *layers)))
                assert all(not bool(t.any()) for k, t in named.items() if k.startswith("Q."))
        check_update(c, agent, eng, b)
    assert eng.iter == eng.adam_step == 3


def test_zero_noise_is_the_plain_network_bit_for_bit():
    """All eps zero: every sigma gradient is exactly zero and the mu gradients are those of the same network with plain Linear streams."""
    c, agent, eng = setup("b31_n3")
    layers = c["layers"]
    renoise(c, 0, agent, eng, zero=True)
    b = batch(c, 0, agent)
    named = dict(zip(M.state_dict_keys(layers), M.flat_to_torch(gradient_of(eng, b), *layers)))
    assert all(not bool(t.any()) for k, t in named.items() if "sigma" in k) and any("sigma" in k for k in named)
    plain = layers[:6] + (False,)
    mu = [p.float() for k, p in agent.params.items() if "sigma" not in k]
    other = M.RainbowMlpEngine(plain, M.flat_from_torch(mu, *plain, eng.device), None, eng.cfg, **V)
    for got, want in zip([t for k, t in named.items() if "sigma" not in k], M.flat_to_torch(gradient_of(other, b), *plain)):
        assert torch.equal(got, want)


def test_eval_forward_ignores_the_noise():
    c, agent, eng = setup("b33_n33")
    b = batch(c, 0, agent)
    first = eng.forward(b["obs"], training=False)
    close(first[0], OR.forward(agent.params, None, c["layers"], b["obs"]))
    assert bool((first[0] != eng.forward(b["obs"])[0]).any())
    renoise(c, 0, agent, eng)
    assert all(torch.equal(x, y) for x, y in zip(first, eng.forward(b["obs"], training=False)))


def test_ties_take_the_first_action():
    """The online Q output layer zeroed (identical Q columns): every expected value ties, action 0 is selected, a different lagged network is projected."""
    c, agent, eng = setup("b33_n33")
    layers = c["layers"]
    agent.old = {k: p.float().double() for k, p in OR.init_params(layers, 99).items()}
    agent.params = {k: (torch.zeros_like(p) if k.startswith("Q.model.0") else p) for k, p in agent.params.items()}
    eng.params_old = M.flat_from_torch([p.float() for p in agent.old.values()], *layers, eng.device)
    eng.params = M.flat_from_torch([p.float() for p in agent.params.values()], *layers, eng.device)
    eng.iter = agent.iter = 1                                # no sync at the next update: two networks
    renoise(c, 1, agent, eng)
    b = batch(c, 0, agent, gap=False)                        # (no gap asked of the tied online network)
    dist, q, act = eng.forward(b["obs_next"])
    assert torch.equal(dist[:, 0], dist[:, 1]) and torch.equal(q[:, 0], q[:, 1]) and int(act.abs().max()) == 0
    close(eng.target_dist(b["obs_next"], b["ret"]), agent.target_dist(b["obs_next"], b["ret"]))     # (torch.max: the first index on ties)


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_n51")
    b2 = setup("b70_n51")[2]
    b = batch(c, 0, agent)
    out = [eng.update_with_batch(b["obs"], b["act"], b["obs_next"], b["ret"], b["weight"]) for eng in (a, b2)]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())


def test_hip_rainbow_mlp_update_with_a_prioritized_buffer():
    """One update(), n-step 3: batch.weight = the oracle's priorities; the write-back fills the modules, the lagged eps and the optimizer."""
    from tianshou_amd.integration import make_hip_rainbow_mlp

    layers, E, B, gamma, n_step = (6, (64, 32), (32,), (), 3, 9, True), 4, 33, 0.95, 3
    torch.manual_seed(21)
    net = SR.build(layers)
    algo = make_hip_rainbow_mlp(ref=SR)(policy=SR.C51Policy(net, num_atoms=layers[5], **V), lr=LR, gamma=gamma, n_step_return_horizon=n_step,
                                        target_update_freq=2, device="cuda").to("cuda")
    trainable = {k: p.detach().cpu() for k, p in net.named_parameters() if p.requires_grad}
    agent = OR.Agent(trainable, layers, None, target_update_freq=2, lr=LR, **V)
    buf = SR.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SR.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    sd, sd_old = net.state_dict(), algo.model_old.state_dict()
    agent.noise = {k: sd[k].cpu() for k in M.noise_keys(layers)}              # what _sample_noise drew inside update()
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)
    ret, _ = O.compute_nstep_return(st, idx, lambda after: agent.support.repeat(len(after), 1).numpy(), gamma, n_step)      # c51.py:120-121
    loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(buf.obs_next[idx]),
                              torch.as_tensor(ret.astype(np.float32)), torch.as_tensor(w, dtype=torch.float32))
    np.testing.assert_allclose(stat.loss, float(loss), rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(prio.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k in agent.params:
        close(sd[k], agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(sd_old[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    assert all(torch.equal(sd_old[k], sd[k]) for k in M.noise_keys(layers))      # the first update is a sync: it carries the noise along
    state = algo.optim._optim.state
    for k, p in net.named_parameters():
        if p.requires_grad:
            close(state[p]["exp_avg"], agent.m[k], rtol=MOM_RTOL, atol=1e-6 * float(agent.m[k].abs().max()))
            assert float(state[p]["step"]) == 1.0
