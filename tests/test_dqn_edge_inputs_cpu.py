"""CPU checks of tests/dqn_edge_cases.py: every case tests/test_gpu_dqn_edges.py runs has the property that test relies on.
(a) `reference(..., float32)` IS oracle_dqn.update_with_batch on the edge networks, bit for bit; (b) the float32 oracle sits
within a quarter of every parity bar (`pytest -s` prints the ratios quoted in dqn_edge_cases.py); (c) tie rows are bit-identical
and oracle_dqn.target_q / torch.argmax take the lowest index; (d) the Huber cases' t = ret - q are exactly the intended values;
(e) every HEAD_GRID case takes the first and last column of each 8-action pass and leaves one action out; (f) the dead fc1 units
are exactly dead; (g) the hand recurrence for (mask, gpow, mc) reproduces oracle.compute_nstep_return bit for bit."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_dqn as OD
from tests import dqn_edge_cases as E


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid A9 B513 weighted mse", "grid A1 B257 huber 1.0", "huber 2.5", "weighted mse (0, 1, 1024)",
                                  "dead units A17 B257"])
def test_reference32_is_the_pinned_oracle(name):
    """Weighted MSE, Huber with delta 1 and 2.5, zero and live heads."""
    c = E.case_by_name(name)
    ocfg = OD.DQNConfig(huber_delta=c["huber"])
    col: dict = {}
    loss, td = OD.update_with_batch(OD.DQNState.create(c["p"], ocfg), ocfg, c["obs"], c["act"], c["ret"], c["weight"], collect=col)
    r32 = E.reference32(c)
    assert float(r32["loss"]) == loss and torch.equal(td, r32["td"]) and torch.equal(col["q_all"], r32["q"])
    assert torch.equal(r32["q"], OD.forward(c["p"], c["obs"]))
    for k in OD.PARAM_ORDER:
        assert torch.equal(col["grads"][k], r32["grads"][k]), k


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.PARITY_NAMES)
def test_float32_oracle_is_within_a_quarter_of_every_bar(name):
    """For exactly the list the GPU file iterates; only conv1 of the live-head case is left out (E.LIVE_HEAD_SKIPPED)."""
    c = E.case_by_name(name)
    assert tuple(c["skip"]) == (E.LIVE_HEAD_SKIPPED if c["rows"] is None else ())
    r32, r64 = E.reference32(c), E.reference64(c)
    for k, v in E.outputs_of(r32).items():
        assert torch.isfinite(v).all(), k
    r = E.ratios(r32, r64, c["skip"])
    print(f"  {name:34s} " + "  ".join(f"{k.replace('grad:', '')} {v:.3f}" for k, v in r.items() if v > 0 or not k.startswith("grad:")))
    assert max(r.values()) <= E.QUARTER, r
    if c["skip"]:
        left_out = {k: v for k, v in E.ratios(r32, r64).items() if k not in r}
        print("    left out: " + "  ".join(f"{k.replace('grad:', '')} {v:.1f}" for k, v in left_out.items()))
        assert set(left_out) == {"grad:" + k for k in E.LIVE_HEAD_SKIPPED}
    if c["rows"] is not None:                                              # an edge network: exact Q, nothing below the head
        for r_ in (r32, r64):
            assert torch.equal(r_["q"], c["rows"].to(r_["q"].dtype).expand(c["B"], -1))
            for k in OD.PARAM_ORDER[:-2]:
                assert not r_["grads"][k].any(), k
        # td is ONE float32 subtraction on exact operands: the GPU test asserts it bit for bit
        assert torch.equal(r32["td"], torch.as_tensor(c["ret"]).float() - c["rows"][c["act"]])


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_the_tie_list_covers_what_it_must():
    sizes = {a for a, _ in E.TIES}
    assert {1, 18, 64} <= sizes
    assert any(len(t) == 2 for _, t in E.TIES) and any(len(t) == 3 for _, t in E.TIES)
    assert any(len(t) == a and a > 1 for a, t in E.TIES)                   # all entries equal
    assert any(t == (a - 1,) and a > 1 for a, t in E.TIES)                 # a strict maximum at the last action
    assert all(t == tuple(sorted(t)) for _, t in E.TIES)
    assert set(E.TIE_BATCHES) == {1, 3, 4, 5}


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("A,tied", E.TIES)
def test_tie_rows(A, tied, negative):
    rows = E.tie_rows(A, tied, negative)
    assert rows.dtype == torch.float32 and rows.shape == (A,)
    assert np.array_equal(E.bits(rows[list(tied)].numpy()), E.bits(rows[tied[0]].expand(len(tied)).contiguous().numpy()))
    assert float(rows.max()) == float(rows[tied[0]])
    others = [a for a in range(A) if a not in tied]
    assert bool((rows[others] < rows[tied[0]]).all()) and len(set(rows[others].tolist())) == len(others)
    assert bool((rows < 0).all()) if negative else bool((rows > 0).all())
    obs = E.obs_batch(5, seed=3)
    p = E.edge_params(rows)
    q = OD.forward(p, obs)
    assert torch.equal(q, rows.expand(5, -1))                               # Q IS the bias row
    assert bool((q.argmax(dim=1) == tied[0]).all()) and bool((q.max(dim=1)[1] == tied[0]).all())
    old = E.lagged_rows(A, tied)
    assert len(set(old.tolist())) == A
    assert A == 1 or int(old.argmax()) != tied[0]
    p_old = E.edge_params(old, seed=2)
    assert torch.equal(OD.forward(p_old, obs), old.expand(5, -1))
    # the expectation of the GPU test IS oracle_dqn.target_q
    for is_double in (True, False):
        cfg = OD.DQNConfig(target_update_freq=3, is_double=is_double)
        st = OD.DQNState(params=p, params_old=p_old)
        assert torch.equal(OD.target_q(st, cfg, obs), (old[tied[0]] if is_double else old.max()).expand(5))
        assert torch.equal(OD.target_q(OD.DQNState(params=p), cfg, obs), rows.max().expand(5))


@pytest.mark.parametrize("A", E.TABLE_ACTIONS)
@pytest.mark.parametrize("B", E.TABLE_BATCHES)
def test_tie_tables(B, A):
    qo, qt = E.tie_tables(B, A, seed=B + A)
    assert qo.shape == qt.shape == (B, A) and qo.dtype == qt.dtype == torch.float32
    assert len(set(qt.reshape(-1).tolist())) == B * A
    assert int(qo[B - 1].argmax()) == A - 1 and (B == 1 or (int(qo[0].argmax()) == 0 and bool((qo[0] == qo[0, 0]).all())))
    first = torch.tensor([min(a for a in range(A) if qo[b, a] == qo[b].max()) for b in range(B)])
    assert torch.equal(qo.argmax(dim=1), first)                             # torch.argmax takes the first maximum
    if A > 1 and B > 8:
        tied_rows = ((qo == qo.max(dim=1, keepdim=True).values).sum(dim=1) > 1)
        assert int(tied_rows.sum()) > B // 4 and len(set(first[tied_rows].tolist())) > 1


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", E.HUBER_DELTAS)
def test_huber_cases_hit_delta_exactly(delta):
    c = E.huber_case(delta)
    d, inf = np.float32(delta), np.float32(np.inf)
    t = c["t"].numpy()
    assert len(t) == len(set(t.tolist())) == 15 and 0.0 in t
    for s in (np.float32(1.0), np.float32(-1.0)):
        up1, dn1 = np.nextafter(s * d, s * inf), np.nextafter(s * d, np.float32(0))
        want = {float(s * d), float(up1), float(np.nextafter(up1, s * inf)), float(dn1), float(np.nextafter(dn1, np.float32(0))),
                float(s * E.TD_TINY), float(s * E.TD_HUGE)}
        assert want <= set(t.tolist()) and len(want) == 7
    assert (np.abs(t) < d).sum() == 1 + 2 + 4 and (np.abs(t) == d).sum() == 2 and (np.abs(t) > d).sum() == 2 + 4
    assert np.array_equal(c["ret"].numpy().astype(np.float64), c["ret64"])            # ret = q + t is representable
    q, _ = E.forward(c["p"], c["obs"], torch.float32)
    assert torch.equal(q, c["rows"].expand(c["B"], -1))
    td = c["ret"] - q[torch.arange(c["B"]), c["act"]]                                  # float32, as the kernel and the oracle subtract
    assert td.dtype == torch.float32 and np.array_equal(E.bits(td.numpy()), E.bits(t))
    assert 2 not in c["act"].tolist() and {0, 1} == set(c["act"].tolist())
    r32, r64 = E.reference32(c), E.reference64(c)
    assert torch.equal(r32["td"], td) and torch.equal(r64["td"], td.double())
    assert not r32["grads"]["fc2.b"][2].any() and not r32["grads"]["fc2.w"][2].any()
    # the reference ignores `weight` under Huber
    rw = E.reference(c["p"], c["obs"], c["act"], c["ret"], c["weight"], delta, torch.float32)
    assert torch.equal(rw["loss"], r32["loss"]) and torch.equal(rw["grads"]["fc2.w"], r32["grads"]["fc2.w"])


def test_mse_case_weights():
    c = E.mse_case()
    w = c["weight"]
    assert all(float(w[r]) == 0.0 for r in c["zero_rows"]) and bool((w == 1.0).any()) and float(w.max()) == 1024.0
    assert 4 not in c["act"].tolist()
    # a row of weight 0 contributes exactly nothing: its return does not reach the loss or any gradient
    ret2 = c["ret"].clone()
    ret2[list(c["zero_rows"])] += 3.0
    a = E.reference32(c)
    b = E.reference(c["p"], c["obs"], c["act"], ret2, w, None, torch.float32)
    assert torch.equal(a["loss"], b["loss"]) and not torch.equal(a["td"], b["td"])
    for k in OD.PARAM_ORDER:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_the_head_grid_covers_what_it_must():
    assert {a for a, b in E.HEAD_GRID if b == 257} == {1, 7, 8, 9, 17, 64}
    assert {b for a, b in E.HEAD_GRID if a == 9} == {1, 255, 256, 257, 513}
    assert len(E.HEAD_GRID) == len(set(E.HEAD_GRID)) == 10
    assert E.pass_edges(9) == [0, 7, 8] and E.pass_edges(7) == [0, 6] and E.pass_edges(17) == [0, 7, 8, 15, 16]
    assert E.pass_edges(1) == [0] and E.pass_edges(64) == sorted(list(range(0, 64, 8)) + list(range(7, 64, 8)))
    losses = [E.grid_case(a, b)["name"].split(" ", 3)[3] for a, b in E.HEAD_GRID]
    assert {"mse", "weighted mse", "huber 1.0", "huber 2.5"} == set(losses)


@pytest.mark.parametrize("A,B", E.HEAD_GRID)
def test_head_grid_actions(A, B):
    c = E.grid_case(A, B)
    act = set(c["act"].tolist())
    assert c["act"].shape == (B,) and act <= set(range(A)) and A - 1 in act
    left = E.never_taken(A)
    assert not act & set(left) and (len(left) >= 1 or A == 1)
    if B >= len(E.pass_edges(A)):
        assert set(E.pass_edges(A)) <= act
    else:                                       # B = 1 takes one column: the last, a pass of its own
        assert B == 1 and act == {A - 1} and (A - 1) % E.PASS == 0
    if B > E.STRIDE:
        assert int(c["act"][E.STRIDE]) in act   # a second trip of the 256-strided loops exists
    assert len(set(c["rows"].tolist())) == A


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
def test_dead_units_are_exactly_dead():
    c = E.dead_case()
    for dtype in (torch.float32, torch.float64):
        r = E.reference32(c) if dtype == torch.float32 else E.reference64(c)
        assert not r["h4"][:, :E.DEAD_UNITS].any()
        assert bool((r["h4"][:, E.DEAD_UNITS:] > 0).any(dim=0).sum() > 300)           # the other units are alive
        assert not r["grads"]["fc2.w"][:, :E.DEAD_UNITS].any()
        assert not r["grads"]["fc1.w"][:E.DEAD_UNITS].any() and not r["grads"]["fc1.b"][:E.DEAD_UNITS].any()
        assert r["grads"]["fc1.b"][E.DEAD_UNITS:].any() and r["grads"]["fc2.w"][:, E.DEAD_UNITS:].any()
    # margin: without the -1e4 the pre-activations of those units stay below 100, so no summation order revives one
    p = {k: v.double() for k, v in c["p"].items()}
    p["fc1.b"][:E.DEAD_UNITS] = 0.0
    x = E.forward(p, c["obs"], torch.float64)[1][:, :E.DEAD_UNITS]
    print(f"  largest pre-activation of those units without it: {float(x.max()):.1f}")
    assert float(x.max()) < 100.0 < -E.DEAD_BIAS / 4
    assert c["p"]["fc2.w"][:, :E.DEAD_UNITS].abs().min() > 0                           # the head would pass a gradient down


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.NSTEP_BUFFERS))
def test_nstep_buffer_has_every_kind_of_end(name):
    st = E.NSTEP_BUFFERS[name]
    n = int(st.offset[-1])
    assert 55 <= n <= 70 and len(st.rew) == len(st.done) == n
    full = st.lengths == np.diff(st.offset)
    assert any(f and 0 < i for f, i in zip(full, st.insertion))                       # full with a wrapped write pointer
    assert any(0 < l < s for l, s in zip(st.lengths, np.diff(st.offset)))             # partly filled
    assert 1 in st.lengths.tolist() and 0 in st.lengths.tolist()
    assert np.array_equal(E.host_valid(st), st.sample_indices_all()) and len(E.host_valid(st)) == int(st.lengths.sum())
    assert np.array_equal(E.host_unfinished(st), st.unfinished_index()) and len(E.host_unfinished(st)) >= 2
    valid = E.host_valid(st)
    assert np.array_equal([E.host_next(st, int(i)) for i in valid], st.next(valid))
    empty = [e for e in range(len(st.lengths)) if st.lengths[e] == 0]
    assert all(not ((valid >= st.offset[e]) & (valid < st.offset[e + 1])).any() for e in empty)
    t, u = st.terminated[valid], st.truncated[valid]
    assert (t & ~u).any() and (u & ~t).any() and (t & u).any()                        # terminated, truncated only, both
    ends = st.offset[1:] - 1                                                           # the slot just before a sub-buffer wraps
    assert any(full[e] and st.done[ends[e]] and np.diff(st.offset)[e] > 1 for e in range(len(full)))
    assert any(full[e] and not st.done[ends[e]] and ends[e] != st.last_index[e] for e in range(len(full)))   # ... and a wrap crossed
    for n_step in E.NSTEP_STEPS:
        mask, gpow, mc, after = E.host_coefficients(st, valid, 0.5, n_step)
        gam = np.round(np.log2(gpow) / np.log2(0.5)).astype(int)                      # the effective number of steps
        assert gam.max() == n_step and gam.min() == 1
        assert set(mask.tolist()) == {0.0, 1.0}
        if n_step > 1:
            assert ((gam < n_step) & (mask == 1)).any()                               # an end with mask 1
            assert ((gam == n_step) & (mask == 0)).any()                              # terminated at the last of the n steps
        assert (st.terminated[valid] & (gam == 1)).any()                              # terminated at the sampled index itself


@pytest.mark.parametrize("gamma", E.NSTEP_GAMMAS)
@pytest.mark.parametrize("n_step", E.NSTEP_STEPS)
@pytest.mark.parametrize("name", list(E.NSTEP_BUFFERS))
def test_hand_recurrence_is_the_oracle(name, n_step, gamma):
    """float32(float64(float32(tq * mask)) * gpow + mc) == oracle.compute_nstep_return, over every valid index and over an
    unordered list with repeats."""
    st = E.NSTEP_BUFFERS[name]
    for idx in (E.host_valid(st), E.unordered_indices(st, 128)):
        tq = E.nstep_tq(len(idx))
        mask, gpow, mc, after = E.host_coefficients(st, idx, gamma, n_step)
        ora, after_o = O.compute_nstep_return(st, idx, lambda a: tq.reshape(-1, 1), gamma, n_step)
        assert np.array_equal(after, after_o)
        tqm = (tq * mask).astype(np.float32)
        got64 = tqm.astype(np.float64) * gpow + mc
        assert np.array_equal(E.bits(got64), E.bits(ora.reshape(-1)))
        assert np.array_equal(E.bits(E.host_returns(tq, mask, gpow, mc)), E.bits(ora.reshape(-1).astype(np.float32)))
        assert mask.dtype == np.float32 and gpow.dtype == mc.dtype == np.float64


def test_tail_coefficients():
    assert 0.0 in E.TAIL_MASK and 1.0 in E.TAIL_GPOW and E.TAIL_GPOW.min() < 1e-20 and E.TAIL_MC.min() < -1e5
    assert len(E.TAIL_MASK) == len(E.TAIL_GPOW) == len(E.TAIL_MC)
