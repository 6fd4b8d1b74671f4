"""GPU parity of continuous BCQ (tianshou_amd.cbcq over ts_cbcq_update) against tests/oracle_cbcq.py, the restatement pinned to
the reference by tests/golden/cbcq_*.npz (tests/test_oracle_cbcq.py)."""
import numpy as np
import pytest
import torch

from tests import cbcq_common as BC
from tests import oracle_cbcq as OB

pytestmark = pytest.mark.gpu

STATE = tuple(n + s for n in BC.NETS for s in ("", "_m", "_v")) + BC.LAGGED


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_update_matches_reference_golden(tag):
    """Both fixtures on the engine, update by update, at tests/test_gpu_cql.py's bars: statistics rtol 2e-5 / atol 1e-7, the
    target rtol 1e-5 / atol 2e-5, strided parameters and lagged parameters rtol 1e-5 / atol 0.02 lr, the final moments rtol 1e-4
    with atol 1e-7 / 1e-10; the critics' gradient norms before clipping at the statistics' bar."""
    g, d, cfg = BC.load_cbcq(tag)
    p0 = BC.init_of(d)
    eng = BC.engine_from(*p0, cfg)
    lay = eng.lay
    lrs = {"pert": cfg.pert_lr, "critic1": cfg.critic1_lr, "critic2": cfg.critic2_lr, "vae": cfg.vae_lr}
    for u in range(d["n_updates"]):
        grads = torch.zeros(eng.grads_size(), dtype=torch.float32, device="cuda")
        tgt = torch.zeros(d["batch"], dtype=torch.float32, device="cuda")
        stats = eng.update_with_batch(**BC.batch_of(g, u), grads_out=grads, target_out=tgt)
        s = stats.cpu().numpy().astype(np.float64)
        print(tag, u, "stats", s, "golden", g[f"u{u}_stats"])
        np.testing.assert_allclose(s, g[f"u{u}_stats"], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(tgt.cpu().numpy(), g[f"u{u}_target"], rtol=1e-5, atol=2e-5)
        if len(g[f"u{u}_grad_norms"]):
            o, pc = lay["vae_count"], lay["critic_count"]
            norms = [float(torch.linalg.vector_norm(grads[o + k * pc: o + (k + 1) * pc].double())) for k in range(2)]
            np.testing.assert_allclose(norms, g[f"u{u}_grad_norms"], rtol=2e-5)
        for name in BC.NETS + BC.LAGGED:
            np.testing.assert_allclose(BC.engine_net(eng, name).numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5,
                                       atol=0.02 * lrs[name.split("_")[0]], err_msg=name)
    assert eng.adam_step == d["n_updates"]
    for name in BC.NETS:
        for suffix, atol in (("m", 1e-7), ("v", 1e-10)):
            np.testing.assert_allclose(BC.engine_net(eng, f"{name}_{suffix}").numpy()[::61], g[f"adam_{suffix}_{name}"], rtol=1e-4,
                                       atol=atol, err_msg=name + suffix)


# (hidden, activation, vae hidden, vae activation, obs, act, L, B, R, perturbation by the first row)
ROUTES = [((256, 256), "relu", (256, 256), "relu", 17, 6, 12, 80, 10, True),
          ((256, 256), "relu", (512, 512), "relu", 11, 3, 6, 70, 4, False),
          ((64, 64), "tanh", (96, 96, 96), "tanh", 11, 3, 5, 70, 3, False),
          ((64, 48), "tanh", (40, 72), "relu", 9, 2, 3, 33, 2, True)]


def _grad_only_cfg(**kw):
    base = dict(pert_lr=-1.0, critic1_lr=-1.0, critic2_lr=-1.0, vae_lr=-1.0, tau=0.0)
    base.update(kw)
    return OB.CBCQConfig(**base)


def _unflat_grads(eng, grads):
    """grads_out -> {net: flat gradient in the oracle's parameter order} (host)"""
    lay, out, o = eng.lay, {}, 0
    for name, n in (("vae", lay["vae_count"]), ("critic1", lay["critic_count"]), ("critic2", lay["critic_count"]), ("pert", lay["pert_count"])):
        out[name] = grads[o:o + n]
        o += n
    return out


def _engine_tensors(eng, name, flat, sizes):
    from tianshou_amd import cbcq as Q

    flat = flat.detach().cpu()
    if name == "vae":
        enc, dec = Q.vae_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.latent_dim, eng.vae_hidden, eng.vae_depth, sizes[1], sizes[1])
        return enc + dec
    if name == "pert":
        return Q.pert_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.hidden, eng.depth, sizes[0])
    return Q.critic_flat_to_torch(flat, eng.obs_dim, eng.act_dim, eng.hidden, sizes=sizes[0])


@pytest.mark.parametrize("hidden,activation,vae_hidden,vae_activation,obs_dim,act_dim,L,B,R,first_row", ROUTES)
def test_gradient_only_mode_vs_float64_autograd(hidden, activation, vae_hidden, vae_activation, obs_dim, act_dim, L, B, R, first_row):
    """Every learning rate -1, tau 0: nothing moves, and the four gradients equal float64 autograd of the oracle (rel. error
    < 2e-5 per tensor), the statistics and the target the oracle's (rtol 2e-5; 1e-5 / 2e-5): the fused route (hidden 256, with
    the VAE on it too and on the per-layer 512 route), a per-layer tanh route and one of unequal widths embedded by padding."""
    cfg = _grad_only_cfg(num_sampled_action=R, activation=activation, vae_activation=vae_activation, phi=0.4, lmbda=0.6,
                         max_action=1.5, gamma=0.9, pert_first_row=first_row)
    p = OB.init_params(obs_dim, act_dim, L, 31, hidden, vae_hidden)
    eng = BC.engine_from(*p, cfg)
    before = [getattr(eng, n).clone() for n in STATE]
    b = BC.random_batch(4, B, R, obs_dim, act_dim, L, cfg.max_action)
    st = OB.CBCQState.create(*p, cfg, dtype=torch.float64)
    col: dict = {}
    ref = OB.update_with_batch(st, cfg, **b, collect=col, step=False)
    grads = torch.zeros(eng.grads_size(), dtype=torch.float32, device="cuda")
    tgt = torch.zeros(B, dtype=torch.float32, device="cuda")
    stats = eng.update_with_batch(**b, grads_out=grads, target_out=tgt)
    for n, t in zip(STATE, before):
        assert torch.equal(getattr(eng, n), t), n
    np.testing.assert_allclose(stats.cpu().numpy(), BC.stats_vector(ref), rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(tgt.cpu().numpy(), ref["target"].numpy(), rtol=1e-5, atol=2e-5)
    for name, flat in _unflat_grads(eng, grads).items():
        want = col[name + "_grads"]
        for t, (key, w) in zip(_engine_tensors(eng, name, flat, (hidden, vae_hidden)), want.items()):
            e = rel_err(t, w)
            print(name, key, e)
            assert t.shape == w.shape and e < 2e-5, (name, key, e)


def _run(cfg, p, b, n=2, mutate=None, **over):
    eng = BC.engine_from(*p, cfg, **over)
    if mutate:
        mutate(eng)
    outs = []
    for _ in range(n):
        grads = torch.zeros(eng.grads_size(), dtype=torch.float32, device="cuda")
        tgt = torch.zeros(b["obs"].shape[0], dtype=torch.float32, device="cuda")
        outs += [eng.update_with_batch(**b, grads_out=grads, target_out=tgt), grads, tgt]
    return eng, outs


@pytest.mark.parametrize("vae_hidden", [(256, 256), (96, 96)])
def test_merged_decoder_pass_is_bit_identical_to_two_passes(vae_hidden):
    """The decoder over B (R + 1) rows in one pass against its B R target rows and its B actor-loss rows as two passes
    (cfg.split_decode): every output and every state tensor after two updates, bit for bit."""
    cfg = OB.CBCQConfig(num_sampled_action=5)
    p = OB.init_params(17, 6, 12, 5, (256, 256), vae_hidden)
    b = BC.random_batch(6, 70, 5, 17, 6, 12)
    e1, o1 = _run(cfg, p, b)
    e2, o2 = _run(cfg, p, b, split_decode=True)
    for x, y in zip(o1, o2):
        assert torch.equal(x, y)
    for n in STATE:
        assert torch.equal(getattr(e1, n), getattr(e2, n)), n


def test_lagged_perturbation_net_is_updated_and_never_read():
    """actor_perturbation_target is Polyak-updated (tau of the live net) and nothing reads it: another starting value leaves
    every output and every other state tensor bit-identical."""
    cfg = OB.CBCQConfig(num_sampled_action=3, tau=0.1)
    p = OB.init_params(11, 3, 6, 8, (64, 64), (96, 96))
    b = BC.random_batch(9, 37, 3, 11, 3, 6)

    def mutate(eng):
        eng.pert_old.mul_(-3.0).add_(0.5)

    e1, o1 = _run(cfg, p, b)
    e2, o2 = _run(cfg, p, b, mutate=mutate)
    for x, y in zip(o1, o2):
        assert torch.equal(x, y)
    for n in STATE:
        assert torch.equal(getattr(e1, n), getattr(e2, n)) == (n != "pert_old"), n
    e3, _ = _run(cfg, p, b, n=1)
    start = BC.engine_from(*p, cfg).pert
    want = 0.1 * e3.pert.double() + 0.9 * start.double()
    np.testing.assert_allclose(e3.pert_old.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("frozen", BC.NETS)
def test_negative_learning_rate_leaves_that_network_alone(frozen):
    cfg = OB.CBCQConfig(num_sampled_action=3, tau=0.0, **{frozen + "_lr": -1.0})
    p = OB.init_params(11, 3, 6, 8, (64, 64), (96, 96))
    eng = BC.engine_from(*p, cfg)
    before = {n: getattr(eng, n).clone() for n in STATE}
    eng.update_with_batch(**BC.random_batch(9, 37, 3, 11, 3, 6))
    for n in BC.NETS:
        for s in ("", "_m", "_v"):
            assert torch.equal(getattr(eng, n + s), before[n + s]) == (n == frozen), n + s


def test_same_call_twice_gives_the_same_bits():
    cfg = OB.CBCQConfig(num_sampled_action=10, pert_first_row=True, critic1_max_grad_norm=0.3, vae_max_grad_norm=0.2)
    p = OB.init_params(17, 6, 12, 3, (256, 256), (512, 512))
    b = BC.random_batch(2, 257, 10, 17, 6, 12)
    e1, o1 = _run(cfg, p, b)
    e2, o2 = _run(cfg, p, b)
    for x, y in zip(o1, o2):
        assert torch.equal(x, y)
    for n in STATE:
        assert torch.equal(getattr(e1, n), getattr(e2, n)), n


# ---- HipBCQ over the stand-ins (the reference package is absent on the GPU box) ----------------------------------------
def _host_buffer(SB, g, d):
    """A host replay-buffer stand-in filled with the fixture's (full) buffer; `done` as recorded."""
    E, slots = d["E"], d["slots"]
    assert d["steps"] == slots
    buf = SB.VectorReplayBuffer(E * slots, E, obs_shape=(d["obs_dim"],), act_shape=(d["act_dim"],))
    for k in ("obs", "obs_next", "act", "rew", "done"):
        getattr(buf, k)[:] = g[k]
    buf.terminated[:], buf.truncated[:] = g["done"], False
    buf._lengths[:], buf.last_index[:] = slots, buf._offset + slots - 1
    for sb in buf.buffers:
        sb._size, sb._insertion_idx = slots, 0
    return buf


def _make_algo(SB, d, cfg, seed=None, update_noise="torch"):
    from torch import nn
    from tianshou_amd.integration import make_hip_bcq

    torch.manual_seed(d["seed"] if seed is None else seed)        # the construction order is init_params' own
    parts = SB.build(d["obs_dim"], d["act_dim"], d["latent_dim"], d["hidden"], d["vae_hidden"],
                     nn.Tanh if cfg.activation == "tanh" else nn.ReLU, "mlp" if cfg.pert_first_row else "net", cfg.max_action, cfg.phi)
    algo = make_hip_bcq(ref=SB)(**parts, actor_perturbation_lr=cfg.pert_lr, critic_lr=cfg.critic1_lr, critic2_lr=cfg.critic2_lr,
                                vae_lr=cfg.vae_lr, gamma=cfg.gamma, tau=cfg.tau, lmbda=cfg.lmbda, num_sampled_action=cfg.num_sampled_action,
                                device="cuda", update_noise=update_noise).to("cuda")
    if cfg.critic1_max_grad_norm > 0:
        algo.critic_optim._max_grad_norm, algo.critic2_optim._max_grad_norm = cfg.critic1_max_grad_norm, cfg.critic2_max_grad_norm
    algo.policy.is_within_training_step = True
    return algo


def _modules(algo):
    return dict(pert=algo.policy.actor_perturbation, critic1=algo.policy.critic, critic2=algo.critic2, vae=algo.policy.vae,
                pert_old=algo.actor_perturbation_target.module, critic1_old=algo.critic_target.module,
                critic2_old=algo.critic2_target.module)


def _draws(seed, B, R, L):
    torch.manual_seed(seed)
    return dict(eps1=torch.randn(B, L), eps2=torch.randn(B * R, L), eps3=torch.randn(B, L))


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hip_bcq_update_against_the_oracle(tag):
    """HipBCQ.update() (make_hip_bcq over tests/standin_cbcq.py) on a host-filled buffer, update_noise="torch": two updates
    against the oracle fed the same rows and the same draws -- BCQTrainingStats (rtol 2e-5 / atol 2e-6), then the written-back
    networks and lagged networks (rtol 1e-5 / atol 0.02 lr) and the optimizers' step counts; the plain-MLP perturbation net
    (first-row form) in one fixture, the Net one in the other."""
    from tests import standin_cbcq as SB

    g, d, cfg = BC.load_cbcq(tag)
    algo = _make_algo(SB, d, cfg)
    assert type(algo).__name__ == "HipBCQ" and isinstance(algo, SB.BCQ)
    p0 = BC.init_of(d)
    for (name, mod), p in zip(_modules(algo).items(), p0):          # the stand-ins' init IS the oracle's
        assert torch.equal(torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu(), OB.flatten(p)), name
    buf = _host_buffer(SB, g, d)
    st = OB.CBCQState.create(*p0, cfg)
    B, R, L = d["batch"], d["R"], d["latent_dim"]
    lrs = {"pert": cfg.pert_lr, "critic1": cfg.critic1_lr, "critic2": cfg.critic2_lr, "vae": cfg.vae_lr}
    for u in range(2):
        torch.manual_seed(100 + u)
        stat = algo.update(buf, B)
        idx = algo._hip_idx.cpu().numpy()
        assert type(stat).__name__ == "BCQTrainingStats"
        ref = OB.update_with_batch(st, cfg, obs=g["obs"][idx], act=g["act"][idx], rew=g["rew"][idx].astype(np.float32),
                                   done=g["done"][idx].astype(np.float32), obs_next=g["obs_next"][idx], **_draws(100 + u, B, R, L))
        got = [stat.actor_loss, stat.critic1_loss, stat.critic2_loss, stat.vae_loss]
        print(tag, u, got, BC.stats_vector(ref))
        np.testing.assert_allclose(got, BC.stats_vector(ref), rtol=2e-5, atol=2e-6)
        for name, mod in _modules(algo).items():
            flat = torch.cat([t.reshape(-1) for t in mod.state_dict().values()]).cpu().numpy()
            np.testing.assert_allclose(flat, OB.flatten(getattr(st, name)).numpy(), rtol=1e-5, atol=0.02 * lrs[name.split("_")[0]], err_msg=name)
    for opt, mod in ((algo.actor_perturbation_optim, algo.policy.actor_perturbation), (algo.vae_optim, algo.policy.vae),
                     (algo.critic2_optim, algo.critic2)):
        assert all(float(opt._optim.state[p]["step"]) == 2.0 for p in mod.parameters())
    vp = next(iter(algo.policy.vae.parameters()))
    np.testing.assert_allclose(algo.vae_optim._optim.state[vp]["exp_avg"].cpu().numpy(), st.opt_vae.m["e_w1"].numpy(), rtol=1e-4, atol=1e-7)


def test_hip_bcq_resumes_from_its_state_dict_and_forwards():
    """state_dict() after two updates; a second instance (other initial networks) that loads it computes the next update bit for
    bit as the uninterrupted run (device noise from the same key and counter), and `hip_policy_forward` returns the engine's
    forward of the same draws."""
    import copy

    from tests import standin_cbcq as SB

    g, d, cfg = BC.load_cbcq("odd")
    buf = _host_buffer(SB, g, d)
    a = _make_algo(SB, d, cfg, update_noise="device")

    def step(algo, u):
        batch = algo._preprocess_batch(SB.Batch(), buf, g[f"u{u}_indices"])
        return algo._update_with_batch(batch)

    for u in range(2):
        step(a, u)
    state = copy.deepcopy(a.state_dict())
    b = _make_algo(SB, d, cfg, seed=77, update_noise="device")
    b.load_state_dict(state)
    b._hip_noise_key, b._hip_noise_calls = a._hip_noise_key, a._hip_noise_calls
    sa_, sb_ = step(a, 2), step(b, 2)
    assert b._hip_engine.adam_step == a._hip_engine.adam_step == 3
    for f in BC.STATS:
        assert getattr(sa_, f) == getattr(sb_, f), f
    for (name, ma), mb in zip(_modules(a).items(), _modules(b).values()):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb), name
    obs = g["obs"][:5]
    noise = torch.randn(5, 7, d["latent_dim"], generator=torch.Generator().manual_seed(3))
    act = a.hip_policy_forward(obs, noise)
    assert act.shape == (5, d["act_dim"]) and torch.equal(act, a._hip_engine.policy_forward(obs, noise))
    assert float(act.abs().max()) <= cfg.max_action
