"""REDQ through REDQEngine at the ensemble size it ships with and at the edges of ts_redq_update / ts_redq_target_q
(tianshou_amd/csrc/ts_sac.hip): a second chunk and remainder chunks of 1 and 2 on the fused route, E = 1 and E = 64, the
per-layer two-stream route with an odd ensemble at depths 1 .. 3, batches of 1, 1023, 1025 and 2049 rows, action columns across a
32-column tile, kc = 1024 (eight-wave multi-network forward) and 1056 (per-layer), subsets of 1, 8, 9 and 10 members, and an actor
step that is skipped.  tests/redq_edge_cases.py holds the inputs and names the path of every shape; tests/test_redq_edge_inputs_cpu.py
checks those paths and that the inputs tell members, chunks, reductions and weights apart.

Yardstick: float64 (tests/redq_edge_cases.py).  Bar of every quantity: max(1e-5, 2 e_ref) of its scale -- e_ref is the float32
oracle's own rel_err against float64 on the same input, computed from the reference alone; `check` prints engine, e_ref, bar and
engine / bar.  Critic gradients are judged member by member, each block on its own scale (the line printed is the worst member's); bq, one
number per member, on the scale of the ensemble's (redq_edge_cases.member_errs).

Measured on an MI355X (this file's own printout, `pytest -s`): per quantity the largest engine / bar over all cases, with the engine's
rel_err, the e_ref and the bar of the case it occurred in.  Nothing needs more than the bar; only target_q ever leaves the 1e-5
floor (its float32 log-probability carries 6e-6, and the engine's error there IS the float32 oracle's, hence exactly half the bar).

    quantity                 engine / bar   engine     e_ref      bar
    critic loss                  0.009      9.34e-08   3.94e-08   1.00e-05
    weight (mean_e td_e)         0.017      1.66e-07   1.89e-08   1.00e-05
    critic gradient w1           0.050      5.03e-07   2.60e-07   1.00e-05
    critic gradient b1           0.053      5.31e-07   2.15e-07   1.00e-05
    critic gradient w2           0.060      6.03e-07   2.99e-07   1.00e-05
    critic gradient b2           0.038      3.80e-07   2.00e-07   1.00e-05
    critic gradient w3 (depth 3) 0.025      2.46e-07   2.58e-07   1.00e-05
    critic gradient b3 (depth 3) 0.012      1.18e-07   1.14e-07   1.00e-05
    critic gradient wq           0.073      7.34e-07   1.12e-06   1.00e-05
    critic gradient bq           0.046      4.58e-07   1.58e-07   1.00e-05
    actor loss                   0.161      1.61e-06   1.61e-06   1.00e-05
    actor gradient w1            0.041      4.07e-07   1.37e-06   1.00e-05
    actor gradient b1            0.023      2.34e-07   2.02e-07   1.00e-05
    actor gradient w2            0.059      5.92e-07   5.76e-07   1.00e-05
    actor gradient b2            0.037      3.67e-07   6.31e-07   1.00e-05
    actor gradient w3 (depth 3)  0.017      1.70e-07   7.33e-07   1.00e-05
    actor gradient b3 (depth 3)  0.014      1.40e-07   7.22e-07   1.00e-05
    actor gradient wmu           0.041      4.07e-07   8.35e-07   1.00e-05
    actor gradient bmu           0.052      5.19e-07   2.31e-06   1.00e-05
    actor gradient wsig          0.043      4.27e-07   9.86e-07   1.00e-05
    actor gradient bsig          0.223      2.23e-06   4.04e-06   1.00e-05
    target_q                     0.500      6.04e-06   6.04e-06   1.21e-05
    copied ensemble: members 5..9 bit-identical to 0..4, reruns bit-identical; member 10 against member 0 (whole block) 1.71e-07

One finding came from the inputs, not from the engine.  The first E = 11 draw put a layer-1 pre-activation of member 2 at 6.5e-9
(float64): the engine's ReLU mask for that sample differed from the float64 one and the member's dW1 was off by 5.4e-2 of its scale,
while the loss agreed to 1e-8.  Both masks are legitimate float32 results, so the batches are now drawn off the kink
(redq_edge_cases.near_kink_rows); no tolerance was touched.  Three deliberate in-bounds errors built into ts_sac.hip -- the TD rows of
every chunk written to chunk 0's, the actor loss summing 63 of 64 members, the last d_out row of a batch above 1024 skipped -- failed 20
of the 58 cases here, each in the tests that name the path (chunk, E = 64, B = 1025 / 2049 on both routes).
"""
import numpy as np
import pytest
import torch

from oracle import oracle_redq as OR
from tests import redq_edge_cases as R
from tests.test_gpu_redq import CFG_KEYS

pytestmark = pytest.mark.gpu


def check(got, ref, e_ref, what):
    """rel_err(got, ref64) < max(1e-5, 2 e_ref); prints the figures and the ratio to the bar."""
    e, bar = R.rel_err(got.cpu() if isinstance(got, torch.Tensor) else got, ref), R.rel_bar(e_ref)
    print(f"    {what}: engine {e:.2e}, float32 reference {e_ref:.2e}, bar {bar:.2e}, engine / bar = {e / bar:.3f}")
    assert np.isfinite(e) and e < bar, (what, e, e_ref)


def engine_for(c, max_action=0.0, **kw):
    """The engine of tests/test_gpu_redq.py::make_engine on the case's own parameters."""
    from tianshou_amd import redq as RQ
    from tianshou_amd import sac as S

    ocfg = R.oracle_cfg(c, max_action=max_action, **kw)
    od, ad, H = c["obs_dim"], c["act_dim"], c["hidden"]
    eng = RQ.REDQEngine(od, ad, S.actor_flat_from_torch(list(c["actor"].values()), od, ad, hidden=H),
                        RQ.ensemble_flat_from_torch(list(c["critic"].values()), od, ad, hidden=H),
                        RQ.REDQConfig(**{k: getattr(ocfg, k) for k in CFG_KEYS}), hidden=H, depth=c["depth"], max_action=max_action)
    return eng, ocfg


def run_update(eng, c, weighted):
    E, pc, pa = c["E"], eng.lay["critic_count"], eng.lay["actor_count"]
    grads = torch.full((E * pc + pa,), float("nan"), dtype=torch.float32, device="cuda")
    stats, w_out = eng.update_with_batch(c["obs"], c["act"], c["ret"], c["noise"], c["weight"] if weighted else None, grads_out=grads)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all()), "a gradient block was left unwritten"
    return stats.cpu(), w_out.cpu(), grads


def check_update(c, ref, out, eng, tag):
    """Critic loss, the `weight` output, every member's critic gradient block, actor loss and actor gradient against float64."""
    from tianshou_amd import redq as RQ
    from tianshou_amd import sac as S

    stats, w_out, grads = out
    E, od, ad, H, d, e = c["E"], c["obs_dim"], c["act_dim"], c["hidden"], c["depth"], ref["e_ref"]
    pc = eng.lay["critic_count"]
    print(f"  {tag}: {R.update_chunks(E, H, c['kc'], d)}")
    check(float(stats[1]), ref["critic_loss"], e["critic_loss"], "critic loss")
    check(w_out, ref["weight"], e["weight"], "weight")
    for t, (key, g) in zip(RQ.ensemble_flat_to_torch(grads[:E * pc], E, od, ad, H, depth=d), ref["critic_grads"].items()):
        t = t.cpu()
        assert t.shape == g.shape, key
        errs = R.member_errs(t, g)
        bars = np.array([R.rel_bar(x) for x in e[("critic", key)]])
        m = int(np.argmax(errs / bars))
        print(f"    critic gradient {key} (worst member {m} of {E}): engine {errs[m]:.2e}, float32 reference {e[('critic', key)][m]:.2e}, "
              f"bar {bars[m]:.2e}, engine / bar = {errs[m] / bars[m]:.3f}")
        assert np.isfinite(errs).all() and (errs < bars).all(), (key, errs.tolist())
    check(float(stats[0]), ref["actor_loss"], e["actor_loss"], "actor loss")
    for t, (key, g) in zip(S.actor_flat_to_torch(grads[E * pc:], od, ad, H, depth=d), ref["actor_grads"].items()):
        check(t, g, e[("actor", key)], f"actor gradient {key}")


def gradient_case(shp, weighted=True, auto=True, tag=""):
    c, ref = R.case(*shp), R.update_reference(shp, weighted, auto)
    eng, _ = engine_for(c, auto_alpha=auto)
    check_update(c, ref, run_update(eng, c, weighted), eng, tag)
    return eng


@pytest.mark.parametrize("weighted", [True, False], ids=["per", "uniform"])
@pytest.mark.parametrize("tag,shp,route,chunks", R.CHUNK_SHAPES, ids=[s[0] for s in R.CHUNK_SHAPES])
def test_second_chunk_and_remainder_chunks(tag, shp, route, chunks, weighted):
    """hidden 256, B = 33: E = 6 -> [5, 1], 7 -> [5, 2], 10 -> [5, 5] (the shipped size), 11 -> [5, 5, 1]; with PER weights and auto
    alpha, and without weights at a fixed alpha."""
    assert R.update_chunks(shp[3], shp[4], R.kc_of(shp[0], shp[1])) == (route, chunks) and len(chunks) >= 2
    gradient_case(shp, weighted, weighted, tag)


def test_copied_chunk_ensemble():
    """E = 11 with members 5..9 exact copies of 0..4 and member 10 a copy of member 0.  Two identical calls give bit-identical
    gradients; the blocks of 5..9 (second chunk: same launch shape, same position in the launch) are bit-identical to those of
    0..4, padding included; member 10 (single-network kernels) meets member 0 at the bar.  The per-member TD rows are no output of
    the engine: they enter through the gradient blocks (bq's gradient is 2 / (E B) sum_b w_b td_b) and the `weight` output."""
    c, ref = R.copied_case(), R.copied_reference(True)
    eng, _ = engine_for(c)
    E, pc = c["E"], eng.lay["critic_count"]
    out = run_update(eng, c, True)
    again = run_update(eng, c, True)
    assert torch.equal(out[2], again[2]) and torch.equal(out[0][:2], again[0][:2]) and torch.equal(out[1], again[1])
    blocks = out[2][:E * pc].reshape(E, pc)
    for m in range(R.CHUNK):
        assert torch.equal(blocks[R.CHUNK + m], blocks[m]), f"member {R.CHUNK + m} differs from member {m}"
    check_update(c, ref, out, eng, "copied E11")
    scale = float(blocks[0].abs().max())
    e = float((blocks[10] - blocks[0]).abs().max()) / scale
    worst = max(float(np.max(v[[0, 10]])) for k, v in ref["e_ref"].items() if isinstance(k, tuple) and k[0] == "critic")
    print(f"    member 10 against member 0, whole block: {e:.2e}, bar {R.rel_bar(worst):.2e}")
    assert e < R.rel_bar(worst)


def test_largest_ensemble_and_the_refusal_beyond_it():
    """E = 64, B = 8: the last slot of acts[64] / loss_parts[64] and the largest workspace, critic phase and actor phase;
    E = 65 is refused by REDQEngine."""
    from tianshou_amd import redq as RQ

    tag, shp, route, chunks = R.LIMIT_SHAPE
    assert shp[3] == R.MAX_ENSEMBLE and len(chunks) == 13
    eng = gradient_case(shp, tag=tag)
    cfg = RQ.REDQConfig(**{**{k: getattr(eng.cfg, k) for k in CFG_KEYS}, "ensemble_size": R.MAX_ENSEMBLE + 1})
    with pytest.raises(ValueError):
        RQ.REDQEngine(shp[0], shp[1], eng.actor, torch.zeros(65 * eng.lay["critic_count"], device="cuda"), cfg)


@pytest.mark.parametrize("tag,shp,route,chunks", R.SINGLE_SHAPES, ids=[s[0] for s in R.SINGLE_SHAPES])
def test_single_member_update(tag, shp, route, chunks):
    """E = 1 on both routes: stride 0 between members, acts[E > 1 ? 1 : 0]."""
    gradient_case(shp, tag=tag)


@pytest.mark.parametrize("tag,shp,route,chunks", R.PER_LAYER_SHAPES, ids=[s[0] for s in R.PER_LAYER_SHAPES])
def test_per_layer_route_with_an_odd_ensemble(tag, shp, route, chunks):
    """hidden 64, E = 7 on two streams (four members on one, three on the other) at depth 2, 3 and 1."""
    gradient_case(shp, tag=tag)


@pytest.mark.parametrize("tag,shp,route,chunks", R.BATCH_SHAPES, ids=[s[0] for s in R.BATCH_SHAPES])
def test_batch_edges(tag, shp, route, chunks):
    """B = 1, 1023, 1025 (a last write row of one element, a second trip of the loss kernels' strided loops), 2049; E = 6 with
    PER weights on both routes."""
    gradient_case(shp, tag=tag)


@pytest.mark.parametrize("tag,shp,route,chunks", R.ACTION_SHAPES, ids=[s[0] for s in R.ACTION_SHAPES])
def test_action_columns_across_a_tile(tag, shp, route, chunks):
    """Input-gradient columns [30, 33) (across column 32) and [15, 47) (the widest action block) of the actor phase."""
    gradient_case(shp, tag=tag)


@pytest.mark.parametrize("tag,shp,route,chunks", [R.WIDE_FUSED, R.WIDE_PER_LAYER], ids=["kc1024", "kc1056"])
def test_wide_input(tag, shp, route, chunks):
    """kc = 1024, the last fused K1: the chunk of 5 on the eight-wave multi-network forward; kc = 1056: the per-layer route."""
    kc = R.kc_of(shp[0], shp[1])
    assert R.update_chunks(shp[3], shp[4], kc)[0] == route and (route != "fused" or R.forward_kernel(5, kc) == "eight-wave")
    gradient_case(shp, tag=tag)


@pytest.mark.parametrize("shp,S,mode,max_action", R.TARGET_CASES,
                         ids=[f"E{c[0][3]}-S{c[1]}-{c[2]}-B{c[0][2]}-h{c[0][4]}-max{c[3]}" for c in R.TARGET_CASES])
def test_target_routes(shp, S, mode, max_action):
    """One launch for S <= 8 (S = 8: blockIdx.y = 7), two streams for S = 9, 10 and for hidden 64; unsorted subsets holding
    member E - 1 and member 0; `critics_old` filled from the case; E = 1 with S = 1 on both routes."""
    from tianshou_amd import redq as RQ

    c, t = R.case(*shp), R.target_reference(shp, S, mode, max_action)
    eng, _ = engine_for(c, max_action=max_action, subset_size=S, target_mode=mode)
    eng.critics_old = RQ.ensemble_flat_from_torch(list(c["critic_old"].values()), c["obs_dim"], c["act_dim"], hidden=c["hidden"])
    out = eng.target_q(c["obs"], c["noise"], t["subset"])
    print(f"  target E {c['E']} S {S} {mode} B {c['B']} hidden {c['hidden']} max_action {max_action}: {R.target_route(S, c['hidden'], c['kc'])}")
    assert out.shape == (c["B"],)
    check(out, t["tq"], t["e_ref"], "target_q")


def test_skipped_actor_step_leaves_the_actor_alone():
    """actor_delay = 3, E = 6, real learning rates, four updates against oracle_redq.update_with_batch.  After updates 1, 2 and 4
    the actor, log_alpha and their Adam moments are bit-identical to before, stats[0] keeps its value and stats[3] is NaN; after
    update 3 the parameters match the oracle (rtol 1e-4, atol 0.1 lr as in test_other_hidden_widths_vs_oracle), with an actor /
    alpha step of the size Adam takes at ITS step 1 (lr; bias-corrected for step 3 it would be 0.64 lr).  critics_old follows
    the oracle's Polyak average on all six members: it moves by tau * (critic step) per update, so its tolerance is tau times
    the critics' (atol 0.1 tau lr per update) plus the suite's 1e-5 relative."""
    from tianshou_amd import redq as RQ
    from tianshou_amd import sac as S

    tag, shp, route, chunks = R.STEP_SHAPE
    c = R.case(*shp)
    E, od, ad, H = c["E"], c["obs_dim"], c["act_dim"], c["hidden"]
    lrs = dict(actor_lr=3e-4, critic_lr=1e-3, alpha_lr=1e-3, tau=0.1, actor_delay=3)
    eng, cfg = engine_for(c, **lrs)
    st = OR.REDQState.create(c["actor"], c["critic"], cfg)
    names = ("actor", "actor_m", "actor_v", "log_alpha", "log_alpha_m", "log_alpha_v")
    old0 = eng.critics_old.clone()
    g = torch.Generator().manual_seed(5)
    last_actor_loss = None
    for u in range(1, 5):
        B = c["B"]
        obs, act = torch.randn(B, od, generator=g), torch.rand(B, ad, generator=g) * 2 - 1
        ret, noise, w = torch.randn(B, generator=g), torch.randn(B, ad, generator=g), 1.0 - 0.95 * torch.rand(B, generator=g)
        before = {n: getattr(eng, n).clone() for n in names}
        steps = eng.will_update_actor()
        assert steps == (u == 3)
        ref = OR.update_with_batch(st, cfg, obs, act, ret, noise, w)
        stats, w_out = eng.update_with_batch(obs, act, ret, noise if steps else None, w)
        s = stats.cpu().numpy()
        np.testing.assert_allclose(s[1], ref["critic_loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(w_out.cpu().numpy(), ref["weight"].numpy(), rtol=1e-5, atol=1e-5)
        if not steps:
            for n in names:
                assert torch.equal(getattr(eng, n), before[n]), (u, n)
            assert np.isnan(s[3]) and (s[0] == 0.0 if last_actor_loss is None else s[0] == last_actor_loss), (u, s)
        else:
            np.testing.assert_allclose(s[0], ref["actor_loss"], rtol=2e-5, atol=1e-6)
            np.testing.assert_allclose(s[3], ref["alpha_loss"], rtol=1e-5, atol=1e-6)
            last_actor_loss = s[0]
            for t, k in zip(S.actor_flat_to_torch(eng.actor, od, ad, H), c["actor"].keys()):
                np.testing.assert_allclose(t.cpu().numpy(), st.actor[k].numpy(), rtol=1e-4, atol=0.1 * cfg.actor_lr, err_msg=k)
            step = float((eng.actor - before["actor"]).abs().max())
            assert 0.99 * cfg.actor_lr < step < 1.01 * cfg.actor_lr, step          # Adam at actor step 1, not critic step 3
            np.testing.assert_allclose(eng.log_alpha.cpu().numpy(), st.log_alpha.numpy().reshape(1), rtol=1e-4, atol=0.1 * cfg.alpha_lr)
            step = float((eng.log_alpha - before["log_alpha"]).abs().max())
            assert 0.99 * cfg.alpha_lr < step < 1.01 * cfg.alpha_lr, step
        np.testing.assert_allclose(s[2], ref["alpha"], rtol=1e-5)
        for t, k in zip(RQ.ensemble_flat_to_torch(eng.critics, E, od, ad, H), c["critic"].keys()):
            np.testing.assert_allclose(t.cpu().numpy(), st.critic[k].numpy(), rtol=1e-4, atol=0.1 * cfg.critic_lr, err_msg=k)
        for t, k in zip(RQ.ensemble_flat_to_torch(eng.critics_old, E, od, ad, H), c["critic"].keys()):
            np.testing.assert_allclose(t.cpu().numpy(), st.critic_old[k].numpy(), rtol=1e-5, atol=0.1 * cfg.tau * cfg.critic_lr * u, err_msg=k)
    pc = eng.lay["critic_count"]
    moved = (eng.critics_old - old0).reshape(E, pc).abs().amax(dim=1).cpu().numpy()
    print(f"  critics_old moved per member by {moved}")
    assert (moved > 2.0 * cfg.tau * cfg.critic_lr).all(), moved                   # at least two of the four Polyak steps' worth
    assert eng.actor_steps == 1 and eng.critic_gradient_step == 4
