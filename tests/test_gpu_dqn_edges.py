"""The three kernels of ts_dqn.hip (head_forward_kernel, target_q_kernel, head_backward_kernel) and nstep_coef_kernel of
ts_returns.hip where tests/test_gpu_dqn.py never goes: every kind of episode end inside an n-step walk, bit-identical Q values,
|td| == huber_delta and its float32 neighbours with delta != 1, actions in the first and last column of an 8-action pass with
A = 7, 8, 9, 17, 64, batch sizes 255 / 256 / 257 / 513 on the 256-sample stride, weights of exactly 0, fc1 units that are
exactly dead.

Every case comes from tests/dqn_edge_cases.py, which states the bars (the suite's existing 1e-5 on each tensor's scale, against
float64) and the precondition each case meets on the CPU (tests/test_dqn_edge_inputs_cpu.py iterates the same lists).  Every
gradient is written into a buffer pre-filled with SENTINEL.  Each check prints its largest |got - ref64| / bar (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_dqn as OD
from tests import dqn_edge_cases as E
from tests.distq_edge_gpu_common import SENTINEL, dev_obs, within

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def flat_of(p, A):
    from tianshou_amd import dqn as D

    return D.flat_from_torch([p[k] for k in OD.PARAM_ORDER], E.C, E.H, E.W, A)


def make_engine(p, A, **cfg):
    from tianshou_amd import dqn as D

    return D.DQNEngine(E.C, E.H, E.W, A, flat_of(p, A), D.DQNConfig(**cfg))


def gradient(eng, obs, act, ret, weight):
    """One gradient-only update into a SENTINEL-filled buffer -> (loss, td, flat gradient), on the host."""
    g = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    before = eng.params.clone()
    loss, td = eng.update_with_batch(obs, act, ret, weight, grad_out=g, apply=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before) and eng.adam_step == 0
    return loss.cpu().reshape(()), td.cpu(), g.cpu()


def blocks(eng, g):
    """Flat gradient -> {oracle_dqn.PARAM_ORDER key: block in torch layout} (a permutation of every element)."""
    from tianshou_amd import dqn as D

    return dict(zip(OD.PARAM_ORDER, D.flat_to_torch(g, E.C, E.H, E.W, eng.n_act)))


def head_of(eng, g):
    """The head's block of the flat gradient as [513, A]: rows 0 .. 511 dW5[k, a], row 512 the bias."""
    from tianshou_amd import dqn as D

    off, _ = D.layer_layout(E.C, E.H, E.W, eng.n_act)
    return g[:off[4]], g[off[4]:off[5]].reshape(E.HIDDEN + 1, eng.n_act)


def check(got, ref64, floor, what):
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    within(got, ref64, torch.full_like(ref64, E.bar_of(ref64, floor)), what)


def run_edge(c, huber, weight, ret=None):
    """A gradient-only update of an edge-network case -> (loss, td, flat gradient, blocks, engine).  Exact claims: td is the
    float32 subtraction itself, nothing flows below the zero head, the columns of actions never taken are 0."""
    eng = make_engine(c["p"], c["A"], huber_delta=huber)
    ret = c["ret"] if ret is None else ret
    loss, td, g = gradient(eng, dev_obs(c["obs"]), c["act"], ret, weight)
    assert np.array_equal(E.bits(td.numpy()), E.bits((torch.as_tensor(ret).float() - c["rows"][c["act"]]).numpy()))
    below, head = head_of(eng, g)
    assert not below.any()
    taken = set(c["act"].tolist())
    for a in range(c["A"]):
        if a not in taken:
            assert not head[:, a].any(), a
    return loss, td, g, blocks(eng, g), eng


def check_edge(c, out, what):
    """loss, td and the fc2 blocks of an edge-network case against float64."""
    loss, td, g, blk, eng = out
    r64 = E.reference64(c)
    print(f"  {what}")
    check(loss, r64["loss"], 1.0, "loss")
    check(td, r64["td"], 1.0, "td")
    for k in ("fc2.w", "fc2.b"):
        check(blk[k], r64["grads"][k], 0.0, k)
    assert blk["fc2.b"].any() and blk["fc2.w"].any()


# ---- A. n-step coefficients ----------------------------------------------------------------------------------------------------
def device_buffer(st):
    from tianshou_amd.buffer import DeviceReplayBuffer

    return DeviceReplayBuffer(offset=st.offset, last_index=st.last_index, lengths=st.lengths, insertion=st.insertion, rew=st.rew,
                              terminated=st.terminated, truncated=st.truncated)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(E.bits(got), E.bits(want)), (what, got, want)


@pytest.mark.parametrize("gamma", E.NSTEP_GAMMAS)
@pytest.mark.parametrize("n_step", E.NSTEP_STEPS)
@pytest.mark.parametrize("name", list(E.NSTEP_BUFFERS))
def test_nstep_coefficients_are_the_host_recurrence(name, n_step, gamma):
    """mask, gpow and mc over every valid index, then over an unordered list with repeats: the same sequence of double
    multiplies and adds as the host recurrence, so bit for bit.  The return formed from them equals ts_nstep_return_fused and
    the oracle cast to float32, bit for bit."""
    from tianshou_amd import returns as R

    st = E.NSTEP_BUFFERS[name]
    buf = device_buffer(st)
    for idx in (E.host_valid(st), E.unordered_indices(st, 128)):
        mask, gpow, mc = R.nstep_coefficients(buf, dev(idx), gamma, n_step)
        h_mask, h_gpow, h_mc, h_after = E.host_coefficients(st, idx, gamma, n_step)
        _same(mask, h_mask, "mask")
        _same(gpow, h_gpow, "gpow")
        _same(mc, h_mc, "mc")
        tq = E.nstep_tq(len(idx))
        mine = E.host_returns(tq, mask.cpu().numpy(), gpow.cpu().numpy(), mc.cpu().numpy())
        _same(R.nstep_return_from_target_q(buf, dev(idx), dev(tq), gamma, n_step), mine, "ts_nstep_return_fused")
        ora, after = O.compute_nstep_return(st, idx, lambda a: tq.reshape(-1, 1), gamma, n_step)
        assert np.array_equal(E.bits(mine), E.bits(ora.reshape(-1).astype(np.float32)))
        assert np.array_equal(R.nstep_indices(buf, dev(idx), n_step).cpu().numpy(), h_after) and np.array_equal(after, h_after)


def test_nstep_coefficients_second_trip_of_the_grid_stride_loop():
    """I = 2048 * 128 + 5: the launch is capped at 2048 workgroups of 128 threads, so the last five indices are a thread's
    second trip.  The indices repeat a pattern of 128, and so must the outputs."""
    from tianshou_amd import returns as R

    st = next(iter(E.NSTEP_BUFFERS.values()))
    buf = device_buffer(st)
    pattern = E.unordered_indices(st, 128, seed=9)
    I = 2048 * 128 + 5
    idx = np.tile(pattern, I // 128 + 1)[:I]
    got = R.nstep_coefficients(buf, dev(idx), 0.99, 3)
    want = E.host_coefficients(st, pattern, 0.99, 3)
    for g, w, what in zip(got, want, ("mask", "gpow", "mc")):
        assert g.shape == (I,)
        _same(g[:128], w, what)
        assert torch.equal(g, g[:128].repeat(I // 128 + 1)[:I]), what


def test_nstep_coefficients_refuse_33_steps():
    from tianshou_amd import _lib
    from tianshou_amd import returns as R

    st = next(iter(E.NSTEP_BUFFERS.values()))
    buf = device_buffer(st)
    idx = dev(E.host_valid(st))
    R.nstep_coefficients(buf, idx, 0.99, E.NSTEP_MAX)
    with pytest.raises(_lib.EngineError):
        R.nstep_coefficients(buf, idx, 0.99, E.NSTEP_MAX + 1)
    with pytest.raises(_lib.EngineError):
        R.nstep_coefficients(buf, idx, 0.99, 0)


# ---- B. argmax ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("A,tied", E.TIES)
def test_argmax_ties_take_the_lowest_index(A, tied, negative):
    """Bit-identical maxima at two or three actions, every entry equal, a strict maximum at the last action, A = 1, 18, 64;
    `negative`: every Q below zero.  forward -> q == rows and the lowest tied index; target_q with a lagged net of distinct Q
    -> its value at that index (double Q) or its own maximum; without a lagged net -> the online maximum under both settings.
    Batch sizes 1, 3, 4, 5: head_forward_kernel handles four samples per workgroup."""
    rows, old = E.tie_rows(A, tied, negative), E.lagged_rows(A, tied)
    p, p_old = E.edge_params(rows), E.edge_params(old, seed=2)
    obs5 = dev_obs(E.obs_batch(5, seed=3))
    for is_double in (True, False):
        eng = make_engine(p, A, target_update_freq=3, is_double=is_double)
        eng.params_old = flat_of(p_old, A)
        single = make_engine(p, A, target_update_freq=0, is_double=is_double)
        assert single.params_old is None
        want = old[tied[0]] if is_double else old.max()
        for B in E.TIE_BATCHES:
            obs = obs5[:B].contiguous()
            q, act = (t.cpu() for t in eng.forward(obs))
            assert np.array_equal(E.bits(q.numpy()), E.bits(rows.expand(B, -1).contiguous().numpy()))
            assert act.dtype == torch.int64 and bool((act == tied[0]).all()), act
            assert torch.equal(eng.target_q(obs).cpu(), want.expand(B)), (is_double, B)
            assert torch.equal(single.target_q(obs).cpu(), rows.max().expand(B)), (is_double, B)


@pytest.mark.parametrize("A", E.TABLE_ACTIONS)
@pytest.mark.parametrize("B", E.TABLE_BATCHES)
def test_bare_target_q_on_tied_tables(B, A):
    """ts_dqn_target_q, the stand-alone C ABI entry on two Q tables: ties at other positions in every row, B on both sides of
    the 256-thread workgroup, against torch.argmax / gather on the host, exactly."""
    from tianshou_amd import _lib

    lib = _lib.load()
    qo, qt = E.tie_tables(B, A, seed=B + A)
    d_qo, d_qt = qo.cuda(), qt.cuda()

    def call(q_online, is_double):
        out = torch.full((B,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(lib.ts_dqn_target_q(_lib.ptr(q_online), _lib.ptr(d_qt), _lib.i64(B), _lib.i64(A), C.c_int(is_double),
                                       _lib.ptr(out), _lib.current_stream()))
        return out.cpu()

    assert torch.equal(call(d_qo, 1), qt.gather(1, qo.argmax(dim=1, keepdim=True)).reshape(-1))
    assert torch.equal(call(d_qo, 0), qt.max(dim=1).values)
    assert torch.equal(call(d_qt, 1), qt.max(dim=1).values)
    assert torch.equal(call(None, 0), qt.max(dim=1).values)                # q_online is not read without double Q
    with pytest.raises(_lib.EngineError):
        call(None, 1)


# ---- C. target_returns arithmetic ----------------------------------------------------------------------------------------------
def test_target_returns_arithmetic_is_the_documented_one():
    """float(double(float(tq * mask)) * gpow + mc) on hand-made coefficients (mask 0, gpow 1.0, a tiny gpow, a huge negative
    mc), bit for bit, with and without a lagged network."""
    A, tied = 5, (3, 4)
    rows, old = E.tie_rows(A, tied, False), E.lagged_rows(A, tied) * 1.1
    n = len(E.TAIL_MASK)
    obs = dev_obs(E.obs_batch(n, seed=4))
    coef = tuple(dev(x) for x in (E.TAIL_MASK, E.TAIL_GPOW, E.TAIL_MC))
    for lagged, is_double in ((True, True), (True, False), (False, True)):
        eng = make_engine(E.edge_params(rows), A, target_update_freq=3 if lagged else 0, is_double=is_double)
        if lagged:
            eng.params_old = flat_of(E.edge_params(old, seed=2), A)
        tq = np.float32(float(old[tied[0]] if is_double else old.max()) if lagged else float(rows.max()))
        assert torch.equal(eng.target_q(obs).cpu(), torch.full((n,), float(tq)))
        got = eng.target_returns(obs, coef).cpu().numpy()
        want = np.asarray([np.float32(np.float64(np.float32(tq * m)) * g + c) for m, g, c in zip(E.TAIL_MASK, E.TAIL_GPOW, E.TAIL_MC)],
                          dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(E.bits(got), E.bits(want)), (got, want)
        assert np.array_equal(E.bits(want), E.bits(E.host_returns(np.full(n, tq), E.TAIL_MASK, E.TAIL_GPOW, E.TAIL_MC)))


# ---- D. Huber and MSE on exact Q -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", E.HUBER_DELTAS)
def test_huber_at_delta_and_its_float32_neighbours(delta):
    c = E.huber_case(delta)
    out = run_edge(c, delta, None)
    assert np.array_equal(E.bits(out[1].numpy()), E.bits(c["t"].numpy()))              # td bit-exact, the intended values
    check_edge(c, out, f"huber delta {delta}")
    weighted = run_edge(c, delta, c["weight"])                                         # the reference ignores `weight` under Huber
    for a, b in zip(out[:3], weighted[:3]):
        assert np.array_equal(E.bits(a.numpy()), E.bits(b.numpy()))


def test_mse_weights_of_zero_one_and_1024():
    """Weighted MSE within the bars; weight=None is bit-identical to all ones; a row of weight 0 contributes exactly nothing:
    the same batch with that row's return changed gives bit-identical loss and gradients."""
    c = E.mse_case()
    out = run_edge(c, None, c["weight"])
    check_edge(c, out, c["name"])
    ret2 = c["ret"].clone()
    ret2[list(c["zero_rows"])] += 3.0
    moved = run_edge(c, None, c["weight"], ret=ret2)
    assert not torch.equal(out[1], moved[1])                                           # td of those rows did move
    keep = [b for b in range(c["B"]) if b not in c["zero_rows"]]
    assert torch.equal(out[1][keep], moved[1][keep])
    assert np.array_equal(E.bits(out[0].numpy()), E.bits(moved[0].numpy()))
    for k in ("fc2.w", "fc2.b"):                                                       # (everything below is 0.0: run_edge)
        assert np.array_equal(E.bits(out[3][k].numpy()), E.bits(moved[3][k].numpy())), k
    none, ones = run_edge(c, None, None), run_edge(c, None, torch.ones(c["B"]))
    for a, b in zip(none[:3], ones[:3]):
        assert np.array_equal(E.bits(a.numpy()), E.bits(b.numpy()))
    r64 = E.reference(c["p"], c["obs"], c["act"], c["ret"], None, None, torch.float64)
    print("  unweighted")
    check(none[0], r64["loss"], 1.0, "loss")
    for k in ("fc2.w", "fc2.b"):
        check(none[3][k], r64["grads"][k], 0.0, k)


# ---- E. the 8-action passes and the 256-sample stride --------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", E.HEAD_GRID)
def test_head_grid_against_float64(A, B):
    """A = 1, 7, 8, 9, 17, 64 at B = 257 and B = 1, 255, 256, 513 at A = 9, the first and last column of every 8-action pass
    taken and one column per pass never: td exact, the loss and the fc2 blocks against float64, two runs bit for bit."""
    c = E.grid_case(A, B)
    out = run_edge(c, c["huber"], c["weight"])
    check_edge(c, out, c["name"])
    again = run_edge(c, c["huber"], c["weight"])
    for a, b in zip(out[:3], again[:3]):
        assert np.array_equal(E.bits(a.numpy()), E.bits(b.numpy()))


# ---- F. dead units under a live head -------------------------------------------------------------------------------------------
def test_dead_units_under_a_live_head():
    """fc1.b[:64] = -1e4 under a random head, (A, B) = (17, 257): H4 of those units is exactly 0 while W5 and dq are not, so the
    `h4 > 0` mask alone keeps dH4 at 0.  Exact zeros in their fc2.w columns, fc1.w rows and fc1.b entries; q, td, loss and the
    fc2, fc1, conv3 and conv2 blocks against float64 (conv1: see dqn_edge_cases.py)."""
    c = E.dead_case()
    n = E.DEAD_UNITS
    r64 = E.reference64(c)
    eng = make_engine(c["p"], c["A"])
    obs = dev_obs(c["obs"])
    q, act = (t.cpu() for t in eng.forward(obs))
    loss, td, g = gradient(eng, obs, c["act"], c["ret"], c["weight"])
    blk = blocks(eng, g)
    print(f"  {c['name']}")
    got = dict(q=q, td=td, loss=loss, grads=blk)
    flat = E.outputs_of(got)
    for k, (ref, bar) in E.bars_of(r64, c["skip"]).items():
        within(flat[k], ref, torch.full_like(ref, bar), k)
    print("    not asserted: " + "  ".join(f"{k} {v:.3f}" for k, v in E.ratios(got, r64).items() if k[5:] in c["skip"]))
    assert set(E.bars_of(r64, c["skip"])) == {"q", "td", "loss"} | {"grad:" + k for k in OD.PARAM_ORDER[2:]}
    top = torch.topk(r64["q"], 2, dim=1).values
    clear = top[:, 0] - top[:, 1] > 1e-4
    assert int(clear.sum()) > c["B"] // 2 and torch.equal(act[clear], r64["q"].argmax(dim=1)[clear])
    assert not blk["fc2.w"][:, :n].any() and blk["fc2.w"][:, n:].any()
    assert not blk["fc1.w"][:n].any() and blk["fc1.w"][n:].any()
    assert not blk["fc1.b"][:n].any() and blk["fc1.b"][n:].any()
    assert torch.isfinite(g).all() and not bool((g == SENTINEL).any())
    loss2, td2, g2 = gradient(eng, obs, c["act"], c["ret"], c["weight"])
    # the weight-gradient GEMMs run on side streams: a missing wait shows as a difference between reruns
    assert torch.equal(g, g2) and torch.equal(td, td2) and torch.equal(loss, loss2)
