"""GPU: the CNN ICM engine (tianshou_amd.icm_cnn over ts_icm_cnn_*) against tests/oracle_icm_cnn.py in float64 and in float32 on the
same device, and the HipICMCnn drop-in over HipPPOCnn over the stand-ins (tests/standin.py + tests/standin_icm.py) against the
reference's recorded runs (tests/golden/icm_cnn_*.npz; initial parameters rebuilt from the stored seed).

Bars: test_gpu_icm.py's, unchanged -- against the oracle: statistics, mse, act_hat and rewards 1e-5 relative, the gradient 1e-5 of
its largest entry, post-step parameters rtol 1e-5 / atol 0.02 lr; against the recorded run: v_s / returns / advantages / log pi_old
1e-5, ICM statistics 2e-5, loss summaries rtol 2e-5 / atol 2e-6, parameters rtol 1e-4 / atol 0.02 lr, moments rtol 1e-3.  The intrinsic part of the
reward is compared at 1e-5 relative, the extrinsic part exactly.  Where a compared value can sit at zero the relative bar carries
an absolute floor of that fraction of the array's largest entry (the values here are raw-frame sized: returns of order 10^2, value
losses of order 10^4).  The fixtures keep every ReLU pre-activation of the ICM model 64 float32 errors away from zero."""
import numpy as np
import pytest
import torch

from tests import icm_cnn_cases as CS
from tests import oracle_icm_cnn as OC
from tests import standin as SI
from tests import standin_icm as SM

pytestmark = pytest.mark.gpu


def close(got, ref, rtol, floor=None, what=""):
    """rtol with an absolute floor of `rtol` x the reference's largest entry (`floor` overrides the factor)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max() / scale) if scale else 0.0
    print(f"{what}: max |err| / max |ref| = {err:.2e} (bar {rtol:.0e})")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=(rtol if floor is None else floor) * scale, err_msg=what)


def engine_of(g, **cfg_kw):
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.icm import ICMConfig

    d, c = g["d"], g["cfg"]
    dims = (d["c"], d["h"], d["w"], d["n_act"], d["model_hidden"])
    kw = dict(lr_scale=c["lr_scale"], reward_scale=c["reward_scale"], forward_loss_weight=c["forward_loss_weight"], lr=c["icm_lr"])
    kw.update(cfg_kw)
    return ICC.ICMCnnEngine(*dims, ICC.flat_from_torch(OC.flat_tensors(CS.fixture_model(g)), *dims, "cuda"), ICMConfig(**kw)), dims


def chains(eng, flat=None):
    t = eng.to_tensors(flat)
    n = 2 * (len(eng.model_hidden) + 1)
    return [t[:6], t[6:6 + n], t[6 + n:]]


@pytest.mark.parametrize("tag", ["small", "odd"])
def test_engine_against_the_oracle_and_the_recorded_run(tag):
    from tianshou_amd import icm_cnn as ICC

    g = CS.load(tag)
    c, stride = g["cfg"], g["d"]["stride"]
    w, lrs, rs, lr = c["forward_loss_weight"], c["lr_scale"], c["reward_scale"], c["icm_lr"]
    eng, dims = engine_of(g)
    o64 = OC.Optim(CS.fixture_model(g, torch.float64), "adam", lr=lr)
    o32 = OC.Optim(OC.cast(CS.fixture_model(g), device="cuda"), "adam", lr=lr)
    pad = ICC.padding_mask(*dims, "cuda")
    for u in range(2):
        obs, act, nxt, rew = (x.cuda() for x in CS.fixture_rows(g, u))
        mse, act_hat = eng.forward(obs, act, nxt)
        aug, mse_r = eng.reward(obs, act, nxt, rew, want_mse=True)
        assert torch.equal(mse, mse_r) and torch.equal(aug, rew + (mse * np.float32(rs)).double())
        for opt, dev in ((o64, "cpu"), (o32, "cuda")):
            with torch.no_grad():
                m_o, a_o = OC.forward(opt.model(), obs.to(dev), act.to(dev), nxt.to(dev))
            np.testing.assert_allclose(mse.cpu().numpy(), m_o.cpu().numpy(), rtol=1e-5)
            close(act_hat.cpu().numpy(), a_o.cpu().numpy(), 1e-5, what=f"{tag} u{u} act_hat vs oracle on {dev}")
            np.testing.assert_allclose((aug - rew).cpu().numpy(), (OC.reward(rew.to(dev), m_o, rs) - rew.to(dev)).cpu().numpy(), rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(mse.cpu().numpy(), g[f"u{u}_pre_mse"], rtol=1e-5)                       # ... and the recorded run
        np.testing.assert_allclose((aug - rew).cpu().numpy(), g[f"u{u}_pre_rew_after"] - g[f"u{u}_pre_rew_before"], rtol=1e-5, atol=1e-12)
        close(act_hat.cpu().numpy().reshape(-1)[::stride], g[f"u{u}_pre_act_hat"], 1e-5, what=f"{tag} u{u} act_hat vs the recorded run")
        grad = torch.empty(eng.count, dtype=torch.float32, device="cuda")
        before = eng.params.clone()
        stats0 = eng.update(obs, act, nxt, grad_out=grad, apply=False)
        assert torch.equal(eng.params, before) and eng.optim_step == u and bool((grad[pad] == 0).all())
        for opt, dev in ((o64, "cpu"), (o32, "cuda")):
            s_o, g_o, _, _ = OC.grads(opt.model(), obs.to(dev), act.to(dev), nxt.to(dev), w, lrs)
            np.testing.assert_allclose(stats0.cpu().numpy(), s_o.cpu().numpy(), rtol=1e-5)
            ref = CS.cat(g_o)
            np.testing.assert_allclose(CS.cat(chains(eng, grad)), ref, rtol=0, atol=1e-5 * float(np.abs(ref).max()))
        stats = eng.update(obs, act, nxt)
        assert torch.equal(stats, stats0) and eng.optim_step == u + 1
        for opt, dev in ((o64, "cpu"), (o32, "cuda")):
            OC.update(opt, obs.to(dev), act.to(dev), nxt.to(dev), w, lrs)
            np.testing.assert_allclose(CS.cat(chains(eng)), CS.cat(opt.model()), rtol=1e-5, atol=0.02 * lr)
        assert bool((eng.params[pad] == 0).all()) and bool((eng.state_m[pad] == 0).all()) and bool((eng.state_v[pad] == 0).all())
        np.testing.assert_allclose(stats.cpu().numpy(), g[f"u{u}_icm_stats"], rtol=1e-5)
        np.testing.assert_allclose(CS.cat(chains(eng))[::stride], g[f"u{u}_i"], rtol=1e-4, atol=0.02 * lr)
    m, v = CS.cat(chains(eng, eng.state_m))[::stride], CS.cat(chains(eng, eng.state_v))[::stride]
    np.testing.assert_allclose(m, g["adam_m_i"], rtol=1e-3, atol=max(1e-6, 2e-7 * float(np.abs(g["adam_m_i"]).max())))
    np.testing.assert_allclose(v, g["adam_v_i"], rtol=1e-3, atol=1e-8 * max(1.0, float(np.abs(g["adam_v_i"]).max())))


def test_module_round_trip():
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.icm import ICMConfig

    g = CS.load("odd")
    d = g["d"]
    eng, dims = engine_of(g)
    mod = SM.IntrinsicCuriosityModule(feature_net=SI.DQNetFeatures(d["c"], d["h"], d["w"]).net[0], feature_dim=d["f_dim"], action_dim=d["n_act"],
                                      hidden_sizes=d["model_hidden"])
    eng.to_module(mod)
    back = ICC.ICMCnnEngine.from_module(mod, d["c"], d["h"], d["w"], ICMConfig())
    assert torch.equal(back.params, eng.params) and back.count == eng.count and back.feature_dim == d["f_dim"]
    for p, t in zip(ICC.describe_module(mod, d["c"], d["h"], d["w"])["tensors"], OC.flat_tensors(CS.fixture_model(g))):
        assert torch.equal(p.detach().cpu(), t)


def build_algo(g, algo="ppo", **icm_kw):
    """HipICMCnn over HipPPOCnn over the stand-ins with the fixture's initial parameters; the fixture's buffer replayed."""
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.integration import make_hip_icm_cnn, make_hip_ppo_cnn

    d, c = g["d"], g["cfg"]
    E, T, ch, h, w, n_act = d["E"], d["T"], d["c"], d["h"], d["w"], d["n_act"]
    trunk = SM.DQNetFeatures(ch, h, w)
    actor, critic = SM.DiscreteActor(trunk, n_act, softmax_output=False), SM.DiscreteCritic(trunk)
    kw = dict(lr=c["lr"], vf_coef=c["vf_coef"], ent_coef=c["ent_coef"], max_grad_norm=c["max_grad_norm"] or None, gae_lambda=c["gae_lambda"],
              gamma=c["gamma"], return_scaling=bool(c["return_scaling"]))
    if algo == "ppo":
        kw.update(eps_clip=c["eps_clip"], dual_clip=c["dual_clip"] or None, value_clip=bool(c["value_clip"]),
                  advantage_normalization=bool(c["advantage_normalization"]), recompute_advantage=bool(c["recompute_advantage"]))
    ppo = make_hip_ppo_cnn(algo, ref=SM)(policy=SM.Policy(actor), critic=critic, device="cuda", **kw)
    with torch.no_grad():
        for p, t in zip(ppo._hip_params(), CS.fixture_ppo(g)):
            p.copy_(t)
    model = SM.IntrinsicCuriosityModule(feature_net=SM.DQNetFeatures(ch, h, w).net[0], feature_dim=d["f_dim"], action_dim=n_act,
                                        hidden_sizes=d["model_hidden"])
    with torch.no_grad():
        for p, t in zip(ICC.describe_module(model, ch, h, w)["tensors"], OC.flat_tensors(CS.fixture_model(g))):
            p.copy_(t)
    kw = dict(lr=c["icm_lr"], lr_scale=c["lr_scale"], reward_scale=c["reward_scale"], forward_loss_weight=c["forward_loss_weight"])
    kw.update(icm_kw)
    algo_ = make_hip_icm_cnn(ref=SM)(wrapped_algorithm=ppo, model=model, **kw).to("cuda")
    stacked = d["stacked"]
    buf = SM.VectorReplayBuffer(E * T, E, obs_shape=(h, w) if stacked else (ch, h, w), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64,
                                stack_num=ch if stacked else 1)
    for t in range(T):
        rows = np.arange(E) * T + t
        nxt = np.zeros_like(g["obs"][rows]) if stacked else g["obs_next"][rows]
        buf.add(SM.Batch(obs=g["obs"][rows], act=g["act"][rows], rew=g["rew"][rows], terminated=g["terminated"][rows],
                         truncated=g["truncated"][rows], obs_next=nxt))
    if stacked:                                     # a buffer that does not store obs_next: the mirror takes obs at next(index)
        buf._meta = SI._Meta(k for k in buf._meta.get_keys() if k != "obs_next")
    return algo_, ppo, buf


def one_update(algo, buf, batch_size, repeat):
    """Algorithm._update's steps by hand, so that the batch can be looked at between the hooks."""
    batch, indices = buf.sample(0)
    rew_host = batch.rew.copy()
    batch = algo._preprocess_batch(batch, buf, indices)
    seen = dict(rew=batch.rew.clone(), v_s=batch.v_s.clone(), returns=batch.returns.clone(), adv=batch.adv.clone(),
                logp_old=batch.logp_old.clone())
    algo.train(True)
    stats = algo._update_with_batch(batch, batch_size, repeat)
    algo._postprocess_batch(batch, buf, indices)
    assert isinstance(batch.rew, np.ndarray) and np.array_equal(batch.rew, rew_host)          # icm.py:88: the reward is restored
    return stats, seen


@pytest.mark.parametrize("tag", ["small", "odd"])
def test_hip_icm_cnn_against_the_recorded_run(tag):
    from tianshou_amd import icm_cnn as ICC

    g = CS.load(tag)
    c, d = g["cfg"], g["d"]
    stride = d["stride"]
    algo, ppo, buf = build_algo(g)
    np.random.seed(d["seed"] + 100)
    for u in range(2):
        ppo_before = [p.detach().clone() for p in ppo._hip_params()]
        stats, seen = one_update(algo, buf, d["batch_size"], d["repeat"])
        before, after = g[f"u{u}_pre_rew_before"], g[f"u{u}_pre_rew_after"]
        assert seen["rew"].dtype == torch.float64 and seen["rew"].is_cuda
        np.testing.assert_allclose(seen["rew"].cpu().numpy() - before, after - before, rtol=1e-5, atol=1e-12)       # the intrinsic part
        for k in ("v_s", "returns", "adv", "logp_old"):
            close(seen[k].cpu().numpy(), g[f"u{u}_pre_{k}"], 1e-5, what=f"{tag} u{u} {k}")
        np.testing.assert_allclose([stats.icm_loss, stats.icm_forward_loss, stats.icm_inverse_loss], g[f"u{u}_icm_stats"], rtol=2e-5)
        assert all(isinstance(x, float) for x in (stats.icm_loss, stats.icm_forward_loss, stats.icm_inverse_loss))
        assert stats.gradient_steps == int(g[f"u{u}_gradient_steps"]) and stats.wrapped_stats.gradient_steps == stats.gradient_steps
        for col, s in enumerate((stats.loss, stats.actor_loss, stats.vf_loss, stats.ent_loss)):
            ref = SM.SequenceSummaryStats.from_sequence(g[f"u{u}_losses"][:, col])
            got = [s.mean, s.max, s.min]
            print(f"{tag} u{u} loss column {col}: {got} against {[ref.mean, ref.max, ref.min]}")
            np.testing.assert_allclose(got, [ref.mean, ref.max, ref.min], rtol=2e-5, atol=2e-6)
        par_p = torch.cat([p.detach().reshape(-1) for p in ppo._hip_params()]).cpu().numpy()[::stride]
        print(f"{tag} u{u} PPO parameters: max |err| / lr = {float(np.abs(par_p - g[f'u{u}_p']).max() / c['lr']):.3f}")
        np.testing.assert_allclose(par_p, g[f"u{u}_p"], rtol=1e-4, atol=0.02 * c["lr"])
        icm_par = ICC.describe_module(algo.model, d["c"], d["h"], d["w"])["tensors"]
        par_i = torch.cat([p.detach().reshape(-1) for p in icm_par]).cpu().numpy()[::stride]
        print(f"{tag} u{u} ICM parameters: max |err| / lr = {float(np.abs(par_i - g[f'u{u}_i']).max() / c['icm_lr']):.3f}")
        np.testing.assert_allclose(par_i, g[f"u{u}_i"], rtol=1e-4, atol=0.02 * c["icm_lr"])
        assert any(not torch.equal(a, b.detach()) for a, b in zip(ppo_before, ppo._hip_params()))
    if c["return_scaling"]:
        np.testing.assert_allclose([ppo.ret_rms.mean, ppo.ret_rms.var, ppo.ret_rms.count], g["ret_rms"], rtol=1e-5)
    sd = algo.state_dict()                                       # the moments arrive with state_dict()
    for name, opt, par in (("p", ppo.optim._optim, ppo._hip_params()), ("i", algo.optim._optim, icm_par)):
        assert all(float(opt.state[p]["step"]) == int(g[f"adam_step_{name}"]) for p in par)
        m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in par]).cpu().numpy()[::stride]
        v = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in par]).cpu().numpy()[::stride]
        np.testing.assert_allclose(m, g[f"adam_m_{name}"], rtol=1e-3, atol=max(1e-6, 2e-7 * float(np.abs(g[f"adam_m_{name}"]).max())))
        np.testing.assert_allclose(v, g[f"adam_v_{name}"], rtol=1e-3, atol=1e-8 * max(1.0, float(np.abs(g[f"adam_v_{name}"]).max())))
    assert len(sd["_optimizers"]) == 1 and len(sd["_optimizers"][0]["state"]) == len(icm_par)


def test_supplied_rewards_reach_the_returns_and_recompute():
    """The seam alone: CnnPPOEngine.preprocess(rew=...) computes the returns from the supplied rewards (not the buffer's), keeps
    them in `pre`, and `recompute` reads them again; without `rew` nothing changes."""
    g = CS.load("odd")
    algo, ppo, buf = build_algo(g)
    batch, indices = buf.sample(0)
    ppo._preprocess_batch(batch, buf, indices)
    eng, m = ppo._hip_engine_obj, ppo._hip_mirror
    rms = list(eng.ret_rms)
    plain = eng.preprocess(m, m.obs, m.act, 4, obs_next_frames=m.obs_next)
    eng.ret_rms = list(rms)
    same = eng.preprocess(m, m.obs, m.act, 4, obs_next_frames=m.obs_next, rew=m.rew[plain["indices"]].clone())
    assert plain["rew"] is None and torch.equal(plain["returns"], same["returns"]) and torch.equal(plain["adv"], same["adv"])
    eng.ret_rms = list(rms)
    shifted = eng.preprocess(m, m.obs, m.act, 4, obs_next_frames=m.obs_next, rew=m.rew[plain["indices"]] + 3.0)
    assert not torch.equal(shifted["returns"], plain["returns"]) and torch.equal(shifted["v_s"], plain["v_s"])
    adv = shifted["adv"].clone()
    eng.ret_rms = list(rms)
    eng.recompute(m, m.obs, shifted, 4)
    np.testing.assert_allclose(shifted["adv"].cpu().numpy(), adv.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(adv.abs().max()))


def test_state_dict_round_trip_and_separate_engines():
    """A HipICMCnn checkpoint goes into the stand-in wrapper and back; a resumed HipICMCnn continues bit-identically; the ICM update
    leaves the wrapped engine's parameters untouched and the wrapped update the ICM engine's."""
    g = CS.load("odd")
    d = g["d"]
    algo, ppo, buf = build_algo(g)
    np.random.seed(5)
    one_update(algo, buf, d["batch_size"], d["repeat"])
    sd = algo.state_dict()
    nested = "wrapped_algorithm._optimizers"
    trunk = SM.DQNetFeatures(d["c"], d["h"], d["w"])
    plain_ppo = SM.PPO(policy=SM.Policy(SM.DiscreteActor(trunk, d["n_act"], softmax_output=False)), critic=SM.DiscreteCritic(trunk))
    plain = SM.ICMOnPolicyWrapper(wrapped_algorithm=plain_ppo, model=SM.IntrinsicCuriosityModule(
        feature_net=SM.DQNetFeatures(d["c"], d["h"], d["w"]).net[0], feature_dim=d["f_dim"], action_dim=d["n_act"], hidden_sizes=d["model_hidden"]),
        lr=1e-3, lr_scale=1.0, reward_scale=1.0, forward_loss_weight=0.5)
    assert set(plain.state_dict()) == set(sd)
    plain.load_state_dict({k: v for k, v in sd.items() if k != nested}, strict=True)
    plain_ppo.optim.load_state_dict(sd[nested][0])
    back = plain.state_dict()
    algo2, ppo2, _ = build_algo(g)
    algo2.load_state_dict(back, strict=True)
    ppo2.ret_rms.mean, ppo2.ret_rms.var, ppo2.ret_rms.count = ppo.ret_rms.mean, ppo.ret_rms.var, ppo.ret_rms.count   # (no state_dict entry)
    np.random.seed(6)
    s1, _ = one_update(algo, buf, d["batch_size"], d["repeat"])
    np.random.seed(6)
    s2, _ = one_update(algo2, buf, d["batch_size"], d["repeat"])
    assert (s1.icm_loss, s1.icm_forward_loss, s1.icm_inverse_loss) == (s2.icm_loss, s2.icm_forward_loss, s2.icm_inverse_loss)
    assert s1.loss.mean == s2.loss.mean
    icm_eng, ppo_eng = algo._hip_engine_obj, ppo._hip_engine_obj
    assert torch.equal(icm_eng.params, algo2._hip_engine_obj.params) and torch.equal(icm_eng.state_v, algo2._hip_engine_obj.state_v)
    assert algo2._hip_engine_obj.optim_step == 2 and torch.equal(ppo_eng.params, ppo2._hip_engine_obj.params)
    assert icm_eng is not ppo_eng
    batch, indices = buf.sample(0)
    batch = algo._preprocess_batch(batch, buf, indices)
    icm_before, ppo_before = icm_eng.params.clone(), ppo_eng.params.clone()
    ppo._update_with_batch(batch, d["batch_size"], d["repeat"])
    assert torch.equal(icm_eng.params, icm_before) and not torch.equal(ppo_eng.params, ppo_before)
    ppo_mid = ppo_eng.params.clone()
    rows, n = algo._hip_rows
    icm_eng.update(rows, n=n)
    assert torch.equal(ppo_eng.params, ppo_mid) and not torch.equal(icm_eng.params, icm_before)


def test_scales_and_learning_rate_are_read_at_every_update():
    g = CS.load("small")
    d = g["d"]
    algo, ppo, buf = build_algo(g, lr_lambda=lambda e: 0.5 ** e, max_grad_norm=0.7)
    np.random.seed(1)
    one_update(algo, buf, d["batch_size"], d["repeat"])
    eng = algo._hip_engine_obj
    assert eng.cfg.lr == g["cfg"]["icm_lr"] and eng.cfg.reward_scale == 0.01 and eng.cfg.max_grad_norm == 0.7
    for s in algo.lr_schedulers:
        s.step()
    algo.reward_scale, algo.lr_scale, algo.forward_loss_weight, algo.optim._max_grad_norm = 0.0, 0.0, 1.0, None
    before = eng.params.clone()
    stats, seen = one_update(algo, buf, d["batch_size"], d["repeat"])
    assert eng.cfg.lr == 0.5 * g["cfg"]["icm_lr"] and (eng.cfg.reward_scale, eng.cfg.lr_scale, eng.cfg.forward_loss_weight) == (0.0, 0.0, 1.0)
    assert eng.cfg.max_grad_norm is None
    assert np.array_equal(seen["rew"].cpu().numpy(), buf.rew[buf.sample_indices(0)])                # reward_scale 0: bit-identical rewards
    assert stats.icm_loss == 0.0 and stats.icm_forward_loss > 0.0
    assert eng.optim_step == 2 and not torch.equal(eng.params, before)      # (a zero gradient: Adam's moments only decay, the step still moves)


def test_hip_a2c_cnn_once():
    """HipICMCnn over HipA2CCnn: the intrinsic reward and the ICM step are the PPO pairing's (the same model, the same rows); the
    wrapped update is A2C's."""
    g = CS.load("small")
    d = g["d"]
    algo, a2c, buf = build_algo(g, algo="a2c")
    assert type(a2c).__name__ == "HipA2CCnn"
    np.random.seed(2)
    stats, seen = one_update(algo, buf, d["batch_size"], 1)
    before, after = g["u0_pre_rew_before"], g["u0_pre_rew_after"]
    np.testing.assert_allclose(seen["rew"].cpu().numpy() - before, after - before, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose([stats.icm_loss, stats.icm_forward_loss, stats.icm_inverse_loss], g["u0_icm_stats"], rtol=2e-5)
    assert np.isfinite(stats.loss.mean) and stats.gradient_steps == 3 and a2c._hip_engine_obj.adam_step == 3
