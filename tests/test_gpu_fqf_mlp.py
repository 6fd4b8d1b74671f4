"""GPU: the FQF-MLP kernels (ts_fqf_mlp.hip) through the C ABI against the float64 oracle of tests/oracle_fqf_mlp.py, at the smallest
shapes at which they can go wrong.  The proposal is compared with the oracle's own; everything behind it runs in the oracle on the
engine's float32 fractions.  Bars: tests/bdqn_common.py, as tests/test_gpu_iqn_mlp.py uses them.  Inputs (`batch`, asserted on the
oracle, every row): every ReLU pre-activation of both walks at least 1e-5 from zero, outside the tie test the top two weighted q at
least 1e-4 apart, and the two sides of every comparison inside gradient_of_taus at least 1e-4 apart: float32 cannot flip one."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import oracle_fqf_mlp as OF
from tests import oracle_iqn_mlp as OI
from tests.bdqn_common import MOM_RTOL, PAR_RTOL, Q_ATOL, RTOL
from tianshou_amd import fqf_mlp as M

pytestmark = pytest.mark.gpu
LR = 1e-3
# taus, tau_hats and entropies against the float64 proposal: the oracle's own proposal (features included) evaluated in float32 differs
# from it by at most 2.4e-7 absolute on taus / tau_hats (values in [0, 1]) and 3.3e-7 relative on the entropies over every case and
# update below (measured on the CPU), so the project's RTOL = 1e-5 with Q_ATOL = 2e-6 hold for that gap and are the bar.
PROP_RTOL, PROP_ATOL = RTOL, Q_ATOL
CASES = {     # layers = (obs_dim, trunk, linear feature width or 0 = ReLU features, C, H, A); fopt: the fraction optimizer
    "b1_n2": dict(layers=(1, (32,), 0, 1, (), 1), N=2, B=1, freq=0, per=False, ent=0.0, fopt="adam", seed=41),
    "b31_n3": dict(layers=(5, (96,), 160, 5, (64,), 3), N=3, B=31, freq=2, per=True, ent=10.0, fopt="rmsprop", seed=42),
    "b33_a32": dict(layers=(17, (64, 32), 32, 64, (), 32), N=7, B=33, freq=2, per=True, ent=0.0, fopt="adam", seed=43, clip=0.02),
    # tile 0: every row takes action A - 1; tile 1: no row takes action 0; tile 2 (6 rows): as drawn
    "b70_edges": dict(layers=(5, (64, 32, 32, 64), 0, 64, (32, 64, 32), 3), N=4, B=70, freq=0, per=True, ent=10.0, fopt="rmsprop", seed=44,
                      acts="edges"),
    "b70_n64": dict(layers=(4, (64, 64), 64, 64, (), 2), N=64, B=70, freq=2, per=False, ent=0.0, fopt="rmsprop", seed=45),
}


def setup(case, device="cuda"):
    c = CASES[case]
    feat = c["layers"][2] or c["layers"][1][-1]
    # (scale 2: at scale 1 the quantiles of neighbouring fractions lie within 1e-4 of each other on most rows at N = 64)
    p0 = {k: p.float() for k, p in OF.init_params(c["layers"], c["seed"], 2.0).items()}
    f0 = {k: p.float() for k, p in OF.init_fraction_params(feat, c["N"], c["seed"] + 500).items()}
    agent = OF.Agent(p0, f0, c["layers"], target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"), ent_coef=c["ent"],
                     f_optim=c["fopt"], f_lr=LR)
    cfg = M.FQFConfig(target_update_freq=c["freq"], lr=LR, max_grad_norm=c.get("clip"), ent_coef=c["ent"], f_optimizer=c["fopt"], f_lr=LR)
    eng = M.FQFMlpEngine(c["layers"], c["N"], M.flat_from_torch(list(p0.values()), *c["layers"], device),
                         M.fraction_from_torch(list(f0.values()), feat, c["N"], device), cfg)
    return c, agent, eng


@torch.no_grad()
def unsafe_rows(agent, p, obs, gap, act=None):
    layers = agent.layers
    taus, hats, _ = (t.float() for t in agent.fractions(obs))
    lg, pre = OI.forward(p, layers, obs, hats, want_pre=True)
    th, pre2 = OI.forward(p, layers, obs, taus[:, 1:-1], want_pre=True)
    bad = torch.zeros(len(obs), dtype=torch.bool)
    for z in pre + pre2:
        bad |= z.abs().min(dim=1)[0] < 1e-5
    if gap and layers[5] > 1:
        top = OF.weighted_q(lg, taus).topk(2, dim=1)[0]
        bad |= (top[:, 0] - top[:, 1]) < 1e-4
    if act is not None:
        r = torch.arange(len(obs))
        bad |= OF.tau_gradient(lg[r, act], th[r, act])[1] < 1e-4
    return bad


def batch(c, u, agent, gap=True):
    """The rows of update u; a row that breaks the rule gets its observation drawn again, then the rule is asserted."""
    g = torch.Generator().manual_seed(100 * c["seed"] + u)
    B, (d, _, _, _, _, A) = c["B"], c["layers"]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    f = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    out = dict(obs=r(B, d), obs_next=r(B, d), act=torch.randint(0, A, (B,), generator=g), mask=(f(B) > 0.2).float(),
               gpow=torch.full((B,), 0.9 ** 3, dtype=torch.float64), mc=r(B).double(), weight=f(B) * 0.9 + 0.1 if c["per"] else None)
    if c.get("acts") == "edges":
        out["act"][:32] = A - 1
        out["act"][32:64] = torch.randint(1, A, (32,), generator=g)
    readers = {"obs": [(agent.params, False, out["act"] if gap else None)], "obs_next": [(agent.params, gap, None)]}
    if agent.old is not None:
        readers["obs_next"].append((agent.old, False, None))
    unsafe = lambda key: sum(unsafe_rows(agent, p, out[key], gp, a) for p, gp, a in readers[key]) > 0  # noqa: E731
    for key in readers:
        for _ in range(8):
            bad = unsafe(key)
            out[key][bad] = r(int(bad.sum()), d)
        assert not unsafe(key).any()
    return out


def flat(d, layers):
    return M.flat_from_torch(list(d.values()), *layers, "cpu").double().numpy()


def fflat(d, eng):
    return M.fraction_from_torch(list(d.values()), eng.F, eng.N, "cpu").double().numpy()


def close(got, want, rtol=RTOL, atol=Q_ATOL):
    want = want.detach() if isinstance(want, torch.Tensor) else want
    np.testing.assert_allclose(got.detach().cpu().double().numpy().reshape(-1), np.asarray(want, np.float64).reshape(-1), rtol=rtol, atol=atol)


def state(opt, params, key):
    return {k: opt.state[p][key] for k, p in params.items()}


@pytest.mark.parametrize("case", CASES)
def test_three_updates_against_the_oracle(case):
    c, agent, eng = setup(case)
    layers, dev = c["layers"], eng.device
    for u in range(3):
        b = batch(c, u, agent)
        lg_g, q_g, act_g, qtau_g = eng.forward(b["obs_next"], want_quantiles_tau=True)
        taus, hats = eng.last_taus.cpu(), eng.last_tau_hats.cpu()
        for got, want in zip((taus, hats, eng.last_entropies), agent.fractions(b["obs_next"])):
            close(got, want, rtol=PROP_RTOL, atol=PROP_ATOL)
        with torch.no_grad():
            lg = OI.forward(agent.params, layers, b["obs_next"], hats)
            close(lg_g, lg)
            close(q_g, OF.weighted_q(lg, taus))
            assert torch.equal(act_g.cpu(), OF.weighted_q(lg, taus).max(dim=1)[1])
            close(qtau_g, OI.forward(agent.params, layers, b["obs_next"], taus[:, 1:-1]))
        assert torch.equal(eng.forward(b["obs_next"], fractions=(taus, hats))[0], lg_g)       # the reference's `fractions=`
        nd = agent.next_dist(b["obs_next"], taus, hats)
        close(eng.next_dist(b["obs_next"]), nd)
        assert torch.equal(eng.last_target_taus.cpu(), taus) and torch.equal(eng.last_target_tau_hats.cpu(), hats)
        ret = (nd.float() * b["mask"].reshape(-1, 1)).double() * b["gpow"].reshape(-1, 1) + b["mc"].reshape(-1, 1)
        got = eng.target_returns(b["obs_next"], tuple(b[k].to(dev) for k in ("mask", "gpow", "mc")))
        close(got, ret)
        ret = got.cpu()                                      # both sides continue from the same float32 returns
        eng.forward(b["obs"])
        taus, hats = eng.last_taus.cpu(), eng.last_tau_hats.cpu()     # the fractions the update will propose for itself
        if u == 0:                                           # both gradients on their own (a second engine)
            grad, fgrad, _, _ = agent.gradient(b["obs"], b["act"], ret, b["weight"], taus, hats)
            other = setup(case)[2]
            g_out, f_out = (torch.empty(n, dtype=torch.float32, device=dev) for n in (other.P, other.P2))
            other.gradient(b["obs"], b["act"], ret, b["weight"], g_out, f_out)
            for got, want in ((g_out, flat(grad, layers)), (f_out, fflat(fgrad, eng))):
                close(got, want, rtol=0, atol=1e-5 * np.abs(want).max())
            assert other.adam_step == other.f_step == 0 and torch.equal(other.params, eng.params) and torch.equal(other.fparams, eng.fparams)
        losses, prio = agent.update(b["obs"], b["act"], ret, b["weight"], taus, hats)
        losses_g, prio_g = eng.update_with_batch(b["obs"], b["act"], ret, b["weight"])
        assert torch.equal(eng.last_taus.cpu(), taus) and torch.equal(eng.last_tau_hats.cpu(), hats)
        close(losses_g, losses)
        close(prio_g, prio)
        close(eng.params, flat(agent.params, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        close(eng.fparams, fflat(agent.fparams, eng), rtol=PAR_RTOL, atol=0.02 * LR)
        if c["freq"]:
            close(eng.params_old, flat(agent.old, layers), rtol=PAR_RTOL, atol=0.02 * LR)
        moments = [(eng.adam_m, flat(state(agent.optim, agent.params, "exp_avg"), layers)),
                   (eng.adam_v, flat(state(agent.optim, agent.params, "exp_avg_sq"), layers)),
                   (eng.f_v, fflat(state(agent.f_optim, agent.fparams, "square_avg" if c["fopt"] == "rmsprop" else "exp_avg_sq"), eng))]
        if c["fopt"] == "adam":
            moments.append((eng.f_m, fflat(state(agent.f_optim, agent.fparams, "exp_avg"), eng)))
        for got, want in moments:
            close(got, want, rtol=MOM_RTOL, atol=1e-6 * np.abs(want).max())       # (the moments' bar of tests/test_gpu_bdqn.py)
    assert eng.iter == eng.adam_step == eng.f_step == 3


def test_ties_take_the_first_action():
    """The online network's final Linear zeroed: every q ties at 0, action 0 wins and the lagged network's column 0 is gathered."""
    c, agent, eng = setup("b31_n3")
    layers = c["layers"]
    old = {k: p.float() for k, p in OF.init_params(layers, 99).items()}
    eng.params_old = M.flat_from_torch(list(old.values()), *layers, eng.device)
    with torch.no_grad():
        agent.params["last.model.2.weight"].zero_()
        agent.params["last.model.2.bias"].zero_()
    eng.params = M.flat_from_torch(list(agent.params.values()), *layers, eng.device)
    agent.old = {k: p.double() for k, p in old.items()}
    b = batch(c, 0, agent, gap=False)                         # (no gap asked of the tied online network: its quantiles all tie too)
    lg, q, act = eng.forward(b["obs_next"])
    assert int(lg.abs().max()) == 0 and int(q.abs().max()) == 0 and int(act.abs().max()) == 0
    close(eng.next_dist(b["obs_next"]), OI.forward(agent.old, layers, b["obs_next"], eng.last_tau_hats.cpu())[:, 0])


def test_the_same_update_twice_is_bit_identical():
    c, agent, a = setup("b70_n64")
    b2 = setup("b70_n64")[2]
    b = batch(c, 0, agent)
    ret = b["mc"].float().reshape(-1, 1) + torch.linspace(-2, 2, c["N"]).reshape(1, -1)
    out = [eng.update_with_batch(b["obs"], b["act"], ret, b["weight"]) for eng in (a, b2)]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(a.params, b2.params) and torch.equal(a.adam_v, b2.adam_v) and bool((a.params != a.params_old).any())
    assert torch.equal(a.fparams, b2.fparams) and torch.equal(a.f_v, b2.f_v) and bool(a.f_v.abs().max() > 0)


def test_hip_fqf_mlp_update_with_a_prioritized_buffer():
    """One update() over the stand-ins, n-step 3, prioritized buffer, RMSprop on the fraction network; the oracle replays the engine's
    fractions: statistics, priorities, and the write-back of both modules and both optimizers."""
    from tests import standin_fqf_mlp as SF
    from tianshou_amd.integration import make_hip_fqf_mlp

    layers, N, E, B, gamma, n_step, ent = (6, (64, 32), 64, 9, (32,), 3), 5, 4, 33, 0.95, 3, 0.5
    torch.manual_seed(21)
    net, frac = SF.build(layers, N)
    with torch.no_grad():
        frac.net.weight.mul_(100.0)                            # (gain 0.01 leaves the proposal uniform to float32)
        for p in net.parameters():
            p.mul_(2.0)                                        # (`setup`'s scale 2, for the input rules asserted below)
    algo = make_hip_fqf_mlp(ref=SF)(policy=SF.FQFPolicy(model=net, fraction_model=frac), lr=LR, fraction_lr=LR, num_fractions=N, ent_coef=ent,
                                    gamma=gamma, n_step_return_horizon=n_step, target_update_freq=2, device="cuda").to("cuda")
    cpu = lambda m: {k: p.detach().cpu() for k, p in m.state_dict().items()}  # noqa: E731
    agent = OF.Agent(cpu(net), cpu(frac), layers, target_update_freq=2, lr=LR, ent_coef=ent, f_optim="rmsprop", f_lr=LR)
    buf = SF.PrioritizedVectorReplayBuffer(E * 40, E, obs_shape=(6,), act_shape=(), act_dtype=np.int64, seed=22)
    rng = np.random.default_rng(23)
    obs = rng.normal(size=(31, E, 6)).astype(np.float32)
    for t in range(30):
        term = rng.random(E) < 0.06
        buf.add(SF.Batch(obs=obs[t], act=rng.integers(0, 3, E), rew=rng.normal(size=E).astype(np.float32), terminated=term,
                         truncated=(rng.random(E) < 0.03) & ~term, obs_next=obs[t + 1]))
    buf.prio[:] = rng.uniform(0.5, 2.0, buf.maxsize)          # non-uniform importance weights
    seen, orig = [], buf.sample
    buf.sample = lambda bs: (lambda r: (seen.append((r[1], np.asarray(r[0].weight).copy())), r)[1])(orig(bs))
    algo.policy.is_within_training_step = True
    stat = algo.update(buf, B)
    idx, w = seen[-1]
    eng = algo._hip_engine
    st = O.BufferState(buf._extend_offset, buf.last_index, buf._lengths, [s._insertion_idx for s in buf.buffers], buf.rew, buf.terminated, buf.truncated)

    def target(after):                                        # (obs_next of the rows the engine proposed for, in its order)
        nxt = torch.as_tensor(buf.obs_next[after])
        assert len(after) == B and not unsafe_rows(agent, agent.params, nxt, True).any()        # (the lagged network still equals it)
        return agent.next_dist(nxt, eng.last_target_taus.cpu(), eng.last_target_tau_hats.cpu()).numpy()

    ret, _ = O.compute_nstep_return(st, idx, target, gamma, n_step)
    assert not unsafe_rows(agent, agent.params, torch.as_tensor(buf.obs[idx]), False, torch.as_tensor(buf.act[idx])).any()
    losses, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(ret.astype(np.float32)),
                                torch.as_tensor(w, dtype=torch.float32), eng.last_taus.cpu(), eng.last_tau_hats.cpu())
    ql, fl, el = (float(x) for x in losses)
    for got, want in ((stat.quantile_loss, ql), (stat.fraction_loss, fl), (stat.entropy_loss, el), (stat.loss, ql + (fl - ent * el))):
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=Q_ATOL)
    np.testing.assert_allclose(buf.weight_updates[-1][1], np.abs(prio.numpy()) + np.finfo(np.float32).eps, rtol=RTOL, atol=Q_ATOL)
    for k, p in net.state_dict().items():
        close(p, agent.params[k], rtol=PAR_RTOL, atol=0.02 * LR)
        close(algo.model_old.module.state_dict()[k], agent.old[k], rtol=PAR_RTOL, atol=0.02 * LR)
    for k, p in frac.state_dict().items():
        close(p, agent.fparams[k], rtol=PAR_RTOL, atol=0.02 * LR)
    for opt, mod, ref_opt, ref_p, key in ((algo.optim, net, agent.optim, agent.params, "exp_avg"),
                                          (algo.fraction_optim, frac, agent.f_optim, agent.fparams, "square_avg")):
        for k, p in mod.named_parameters():
            want = ref_opt.state[ref_p[k]][key]
            close(opt._optim.state[p][key], want, rtol=MOM_RTOL, atol=1e-6 * float(want.abs().max()))
            assert float(opt._optim.state[p]["step"]) == 1.0
