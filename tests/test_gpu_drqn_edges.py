"""The recurrent Q engine (ts_rnnq.hip: lstm_layer_fwd / bwd_kernel, the per-step cell kernels, head_out_kernel,
rnn_target_q_kernel, td_loss_kernel) where tests/test_gpu_drqn.py never goes: T = 64 and 256, B = 1 and 15 / 16 / 17 (the layer
kernels' 16-row tile edge), a carried state entered with a real sequence, gates saturated through their bias rows, exact Q values
(ties, all-negative Q, A = 1 and 32), |td| == huber_delta and its float32 neighbours, B > 1024 in the one-workgroup loss kernel.

Every case comes from tests/drqn_edge_cases.py, which states the bars (the suite's existing ones, against float64) and the
precondition each case meets on the CPU (tests/test_drqn_edge_inputs_cpu.py iterates the same lists).  Every gradient is written
into a buffer pre-filled with SENTINEL.  Each check prints its largest |got - ref64| / bar (`pytest -s`)."""
import numpy as np
import pytest
import torch

from oracle import oracle_drqn as ORQ
from tests import drqn_edge_cases as E
from tests.distq_edge_gpu_common import SENTINEL, within

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(E.PATHS), autouse=True)
def lstm_path(request, monkeypatch):
    """Every test runs on both recurrent paths: a whole LSTM layer per launch (lstm_layer_fwd / bwd_kernel, H = 32, 64, 128)
    and one GEMM + one cell launch per step (TS_RNN_PER_STEP, the path of the other widths)."""
    if request.param == "per_step":
        monkeypatch.setenv("TS_RNN_PER_STEP", "1")
    return request.param


def _on_paths(cases):
    """(path, case name) for every path the case names: parametrises the fixture itself, so a per-step-only case runs once."""
    return [(path, c["name"]) for c in cases for path in c["paths"]]


def make_engine(p, obs_dim, hidden, layers, n_act, **cfg):
    from tianshou_amd import dqn as D
    from tianshou_amd import drqn as R

    flat = R.flat_from_torch([p[k] for k in ORQ.param_keys(layers)], obs_dim, hidden, layers, n_act)
    return R.RecurrentDQNEngine(obs_dim, hidden, layers, n_act, flat, D.DQNConfig(**cfg))


def engine_of(case, **cfg):
    return make_engine(E.inputs(case)["p"], case["obs_dim"], case["H"], case["L"], case["A"], huber_delta=case["huber"], **cfg)


def gradient(eng, obs, act, ret, weight):
    """One gradient-only update into a SENTINEL-filled buffer -> (loss, td, flat gradient), on the host."""
    g = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    before = eng.params.clone()
    loss, td = eng.update_with_batch(obs, act, ret, weight, grad_out=g, apply=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before)
    return loss.cpu().reshape(()), td.cpu(), g.cpu()


def blocks(eng, g):
    """Flat gradient -> {state_dict key: block}; the padding (fc1 rows obs_dim .. k0, head columns >= A) is asserted to be
    exactly 0.0 on the flat buffer, so together the two cover every element the engine must write."""
    from tianshou_amd import drqn as R

    lay, H = eng.lay, eng.hidden
    if lay["k0"] > eng.obs_dim:
        assert not g[lay["fc1"]:lay["fc1"] + (lay["k0"] + 1) * H].reshape(-1, H)[eng.obs_dim:lay["k0"]].any()
    if eng.n_act < E.HEAD:
        assert not g[lay["fc2"]:].reshape(H + 1, E.HEAD)[:, eng.n_act:].any()
    return dict(zip(ORQ.param_keys(eng.layers), R.flat_to_torch(g, eng.obs_dim, H, eng.layers, eng.n_act)))


def run_case(case):
    """forward + two gradient-only updates -> the flat {quantity: tensor} of E.outputs_of and the engine."""
    i = E.inputs(case)
    eng = engine_of(case)
    q, act, (h, c) = eng.forward(i["obs"], want_state=True)
    loss, td, g = gradient(eng, i["obs"], i["act"], i["ret"], i["weight"])
    loss2, td2, g2 = gradient(eng, i["obs"], i["act"], i["ret"], i["weight"])
    # the weight-gradient GEMMs run on two side streams: a missing wait shows as a difference between reruns
    assert torch.equal(g, g2) and torch.equal(td, td2) and torch.equal(loss, loss2), case["name"]
    got = dict(q=q.cpu(), h=h.cpu().transpose(0, 1), c=c.cpu().transpose(0, 1), td=td, loss=loss, grads=blocks(eng, g))
    return got, act.cpu(), eng


def check_parity(case, got):
    ref = E.reference64(case)
    flat = E.outputs_of(got, case["zero"])
    print(f"  {case['name']}")
    for k, (r, bar) in E.bars_of(ref, case["zero"]).items():
        within(flat[k], r, bar, k)
    for k, v in E.outputs_of(got).items():
        assert torch.isfinite(v).all(), k
    return ref


# ---- A. length x batch grid --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lstm_path,name", _on_paths(E.GRID_CASES), indirect=["lstm_path"])
def test_length_and_batch_grid_against_float64(lstm_path, name):
    """q, h_T and c_T of every layer, td, loss and every gradient block against float64 at T = 2 .. 256, B = 1, 15, 16, 17,
    obs_dim 4 / 32 / 33, A = 1 / 2 / 5 / 32; the gradient of two reruns bit for bit."""
    case = E.CASES[name]
    got, act, _ = run_case(case)
    ref = check_parity(case, got)
    top = torch.topk(ref["q"], min(2, case["A"]), dim=1).values
    clear = (top[:, 0] - top[:, -1] > 1e-4) if case["A"] > 1 else torch.ones(case["B"], dtype=torch.bool)
    assert torch.equal(act[clear], ref["q"].argmax(dim=1)[clear])


# ---- B. carried state --------------------------------------------------------------------------------------------------------
def _state(q, h, c):
    """forward's (q, (h, c)) with the state as [B, L, H] -> {q, h0.., c0..} on the host."""
    out = dict(q=q.cpu())
    for l in range(h.shape[1]):
        out[f"h{l}"], out[f"c{l}"] = h[:, l].cpu(), c[:, l].cpu()
    return out


def _check_state(case, got, full, what):
    print(f"  {case['name']} {what}")
    for k, (r, bar) in E.bars_of(E.reference64(case)).items():
        if k in got:
            within(got[k], r, bar, k + " vs float64")
            within(got[k], full[k].double(), bar, k + " vs one pass")
    assert len(got) == 1 + 2 * case["L"]


def _full_pass(case, eng):
    q, _, (h, c) = eng.forward(E.inputs(case)["obs"], want_state=True)
    return _state(q, h, c)


@pytest.mark.parametrize("name,T1", E.CARRIED)
def test_carried_state_with_a_real_sequence(name, T1):
    """forward(obs[:, :T1]) then forward(obs[:, T1:], state=...) (the layer kernel's zero_init = 0 branch with T > 1) against one
    pass over all 64 steps and against float64.  Not bit-equal by contract: the input-projection GEMM may split differently
    for another row count."""
    case = E.CASES[name]
    obs = E.inputs(case)["obs"]
    eng = engine_of(case)
    full = _full_pass(case, eng)
    _, _, s1 = eng.forward(obs[:, :T1], want_state=True)
    q, _, (h, c) = eng.forward(obs[:, T1:], state=s1, want_state=True)
    _check_state(case, _state(q, h, c), full, f"{T1} + {64 - T1}")


@pytest.mark.parametrize("name", E.CARRIED_STEPS)
def test_64_evaluation_steps_equal_one_pass(name):
    """B = 1, obs [1, dim] per call with the carried state -- the shape of every evaluation-mode call of one environment."""
    case = E.CASES[name]
    obs = E.inputs(case)["obs"]
    eng = engine_of(case)
    full = _full_pass(case, eng)
    state = None
    for t in range(case["T"]):
        q, _, state = eng.forward(obs[:, t], state=state, want_state=True)
    _check_state(case, _state(q, *state), full, "64 x (T = 1)")


# ---- C. saturated gates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in E.SATURATED_PARITY_CASES])
def test_saturated_and_integrating_gates_against_float64(name):
    """Forget bias +3 / +4 (|c| up to 12), forget bias -30, o-gate +110 with g-gate +-60 (exp overflows to inf inside the
    hardware-exp gate forms): everything finite and within the parity bars."""
    case = E.CASES[name]
    got, _, _ = run_case(case)
    check_parity(case, got)


@pytest.mark.parametrize("name", [c["name"] for c in E.ZERO_CASES])
def test_closed_gates_give_exact_zeros(name):
    """o-gate bias -110: h == 0.0 at every layer, q == fc2.bias, every gradient below the head and the head's weight gradient
    exactly 0.0, its bias gradient within the bar; i-gate bias -110: c == 0.0 as well."""
    case = E.CASES[name]
    got, _, eng = run_case(case)
    check_parity(case, got)
    assert not got["h"].any()
    if name.startswith("i"):
        assert not got["c"].any()
    assert torch.equal(got["q"], E.inputs(case)["p"]["fc2.bias"].expand(case["B"], -1))
    for k in ORQ.param_keys(case["L"])[:-1]:
        assert not got["grads"][k].any(), k
    assert got["grads"]["fc2.bias"].any()


# ---- D. head and target kernels on exact Q -----------------------------------------------------------------------------------
def _flat(p, A, obs_dim=4, H=32, L=1):
    from tianshou_amd import drqn as R

    return R.flat_from_torch([p[k] for k in ORQ.param_keys(L)], obs_dim, H, L, A)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("A,tied", E.TIES)
def test_argmax_ties_take_the_lowest_index(A, tied, negative):
    """Bit-identical maxima at two or three actions, a strict maximum at the last action, A = 32 (no padding column) and A = 1;
    `negative`: every Q below zero.  forward -> the lowest tied index; target_q with a lagged net of distinct Q -> its value at
    that index (double Q) or its own maximum; without a lagged net -> the online maximum under both settings."""
    rows, old = E.tie_rows(A, tied, negative), E.lagged_rows(A, tied)
    obs = torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(3))
    for is_double in (True, False):
        eng = make_engine(E.edge_params(rows), 4, 32, 1, A, target_update_freq=3, is_double=is_double)
        q, act = (t.cpu() for t in eng.forward(obs))
        assert torch.equal(q, rows.expand(5, -1)) and bool((act == tied[0]).all()), act
        eng.params_old = _flat(E.edge_params(old, seed=2), A)
        tq = eng.target_q(obs).cpu()
        want = old[tied[0]] if is_double else old.max()
        assert torch.equal(tq, want.expand(5)), (is_double, tq, want)
        single = make_engine(E.edge_params(rows), 4, 32, 1, A, target_update_freq=0, is_double=is_double)
        assert single.params_old is None and torch.equal(single.target_q(obs).cpu(), rows.max().expand(5))


def test_target_returns_arithmetic_is_the_documented_one():
    """float(double(float(tq * mask)) * gpow + mc) on hand-made coefficients, bit for bit."""
    A, tied = 5, (3, 4)
    rows, old = E.tie_rows(A, tied, False), E.lagged_rows(A, tied) * 1.1
    eng = make_engine(E.edge_params(rows), 4, 32, 1, A, target_update_freq=3, is_double=True)
    eng.params_old = _flat(E.edge_params(old, seed=2), A)
    mask = np.asarray([1, 0, 1, 1, 0, 1], dtype=np.float32)
    gpow = np.asarray([0.99 ** 3, 0.5, 1.0, 0.95 ** 2, 0.97, 1e-3], dtype=np.float64)
    mc = np.asarray([0.1, -2.5, 1e-3, 3.3, 0.0, -1e6 / 3], dtype=np.float64)
    obs = torch.randn(6, 3, 4, generator=torch.Generator().manual_seed(4))
    got = eng.target_returns(obs, tuple(torch.as_tensor(x).cuda() for x in (mask, gpow, mc))).cpu().numpy()
    tq = np.float32(float(old[tied[0]]))
    want = np.asarray([np.float32(np.float64(np.float32(tq * m)) * g + c) for m, g, c in zip(mask, gpow, mc)], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want), (got, want)


# ---- E. td_loss_kernel on exact Q ---------------------------------------------------------------------------------------------
def _edge_update(c, huber, weight, rows=slice(None)):
    eng = make_engine(c["p"], 4, 32, 1, c["A"], huber_delta=huber)
    w = None if weight is None else weight[rows]
    loss, td, g = gradient(eng, c["obs"][rows], c["act"][rows], c["ret"][rows], w)
    blk = blocks(eng, g)
    assert not g[:eng.lay["fc2"]].any()                               # zero head weights pass nothing down
    return loss, td, g, blk, eng


def _check_edge(c, huber, weight, out, what):
    loss, td, g, blk, eng = out
    r64 = E.reference(c["p"], c["obs"], c["act"], c["ret"], weight, huber, torch.float64)
    print(f"  {what}")
    within(loss, r64["loss"], E.out_bar(r64["loss"]), "loss")
    within(td, r64["td"], E.out_bar(r64["td"]), "td")
    for k in ("fc2.weight", "fc2.bias"):
        within(blk[k], r64["grads"][k], E.grad_bar(r64["grads"][k]), k)
    head = g[eng.lay["fc2"]:].reshape(eng.hidden + 1, E.HEAD)
    for a in range(c["A"]):
        if a not in set(c["act"].tolist()):
            assert not head[:, a].any(), a                            # the columns of actions not taken
    return r64


@pytest.mark.parametrize("delta", E.HUBER_DELTAS)
def test_huber_at_delta_and_its_float32_neighbours(delta):
    c = E.huber_case(delta)
    out = _edge_update(c, delta, None)
    assert torch.equal(out[1], c["t"])                                # td bit-exact
    _check_edge(c, delta, None, out, f"huber delta {delta}")
    assert not out[2][out[4].lay["fc2"]:].reshape(33, E.HEAD)[:, 2:].any()
    weighted = _edge_update(c, delta, c["weight"])                    # the reference ignores `weight` under Huber
    for a, b in zip(out[:3], weighted[:3]):
        assert torch.equal(a, b)


def test_mse_absent_unit_and_one_hot_weights():
    """weight=None is bit-identical to all ones; weight = 16 e_r at B = 16 leaves td untouched and gives the loss and the fc2
    gradient of a B = 1 update on row r alone, bit for bit (1 / 16 is exact: the zero-weight rows contribute exactly nothing)."""
    c = E.batch_case(16)
    none = _edge_update(c, None, None)
    ones = _edge_update(c, None, torch.ones(16))
    for a, b in zip(none[:3], ones[:3]):
        assert torch.equal(a, b)
    _check_edge(c, None, None, none, "mse B 16 unweighted")
    _check_edge(c, None, c["weight"], _edge_update(c, None, c["weight"]), "mse B 16 weighted")
    for r in (0, 7, 15):
        w = torch.zeros(16)
        w[r] = 16.0
        hot = _edge_update(c, None, w)
        alone = _edge_update(c, None, None, rows=slice(r, r + 1))
        assert torch.equal(hot[1], none[1]) and hot[1][r] == alone[1][0]
        assert torch.equal(hot[0], alone[0])
        for k in ("fc2.weight", "fc2.bias"):
            assert torch.equal(hot[3][k], alone[3][k]), (r, k)
        assert hot[3]["fc2.bias"].any()


@pytest.mark.parametrize("huber", [None, 1.0])
@pytest.mark.parametrize("B", E.BATCH_SIZES)
def test_loss_kernel_batch_sizes(B, huber):
    """B = 1, 1024, 1025, 2049: td_loss_kernel is ONE workgroup of 1024 threads striding over the batch."""
    c = E.batch_case(B, huber)
    w = None if huber else c["weight"]
    out = _edge_update(c, huber, w)
    assert torch.equal(out[1], c["ret"] - c["rows"][c["act"]])       # td per row, the float32 subtraction itself
    _check_edge(c, huber, w, out, f"B {B} huber {huber}")
