"""The fused three-layer MLP kernels (mlp3_fwd_kernel / mlp3_bwd_kernel<N3, NW, RB>, tianshou_amd/csrc/ts_mlp.hip) through
tianshou_amd.mlp3 (ts_mlp3_forward / ts_mlp3_backward / ts_mlp3_set_variant) at the edges tests/mlp3_edge_cases.py lists: row counts
around one, two and three tiles and around the fill threshold of the 32-row workgroups, every input width from 32 to 1024 on four
and on eight waves, 1 .. 8 networks on shared and on their own input rows, every variant the dispatch can be set to, and
input-gradient ranges of one to eight tiles.  tests/test_mlp3_edge_inputs_cpu.py checks that every case takes the instantiation it
names and that the inputs can tell a wrong kernel from a right one.

Yardstick: float64 (tests/mlp3_edge_cases.py).  Bar of every tensor of every network: max(1e-5, 2 e_ref) of its largest reference
entry -- e_ref is torch's own float32 evaluation of the same formulas against float64 on the same input, computed from the
reference alone; `check` prints engine, e_ref, bar and engine / bar.  Every output lies in a buffer with spare rows before and after
it, pre-filled with a sentinel: rows >= M and dx columns outside the covering tiles must keep it.

Bit-identity, each promised by a comment in the code and each found to hold on an MI355X: a rerun of any case; network k of a
shared launch against its own launch of the same instantiation (ts_mlp.h; four and eight waves -- 32-row workgroups take no single
network, they are tied to the eight-wave 16-row kernel instead, which is tied to its single-network launch); the first M rows of a
longer launch; `out` with and without the h1 / h2 stores; RB = 2 against RB = 1 on eight waves (the summation order at the top of
ts_mlp.hip does not involve the row block).

Measured on an MI355X (this file's own printout, `pytest -s`, test_zz_summary): per tensor the largest engine / bar over all 164
cases, the 256 launches of the width sweep and the bit-identity tests, with the engine's rel_err, the e_ref and the bar of the case it
occurred in.  Nothing leaves the 1e-5 floor, and nothing needs more than a seventh of it.

    tensor   engine / bar   engine     e_ref      bar        case
    h1          0.146       1.46e-06   5.86e-07   1.00e-05   width fwd head 64 nw 4 K1 864
    h2          0.068       6.82e-07   2.80e-07   1.00e-05   rb2 fwd K1 480
    out         0.052       5.16e-07   2.61e-07   1.00e-05   width fwd head 64 nw 4 K1 928
    dh2         0.044       4.35e-07   2.80e-07   1.00e-05   rb2 bwd head 64 fails M 736
    dh1         0.061       6.07e-07   3.70e-07   1.00e-05   rb2 bwd head 64 fails M 736
    dx          0.044       4.37e-07   3.23e-07   1.00e-05   nets 8 bwd

No kernel bug was found: all twelve instantiations, the 32-row LDS overlay and the clamped duplicate tiles of the five- to
seven-tile input-gradient ranges compute what they should.  One hole in the host checks was: mlp3_backward_n took "input gradients
wanted" from network 0 alone, so a dx pointer for a later network only was silently ignored; it is refused now like the reverse.

That the tests bite: three deliberate in-bounds errors built into ts_mlp.hip, this file run once against each (237 tests).
  * the finish sums nks - 1 of the k splits: 180 fail -- all 164 cases (every instantiation has a layer with a k split: the head
    on four waves, every layer on eight), all 8 width sweeps, all 8 shared-launch tests (at check_case, before the bit comparison).
  * WStream::trow one tile low for e = 3 (transposed layers): 114 fail -- all 106 backward cases, the 4 backward width sweeps and
    the 4 backward shared-launch tests; every forward test passes, as it must.
  * the ReLU mask read from row m0 instead of m0 + row: 114 fail -- 104 of the 106 backward cases (the two M = 1 cases have no other
    row), the 4 backward sweeps, the 4 backward shared-launch tests and both backward RB = 2 against RB = 1 tests (m0 differs
    between 16- and 32-row workgroups); every forward test passes.
The refusal and set_variant tests do not launch and pass under all three.
"""
import dataclasses
import functools

import pytest
import torch

from tests import mlp3_edge_cases as R

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
SPARE = 5                      # sentinel rows before and after every output
CASES = R.cases()
NAMES = [c.name for c in CASES]
WORST: dict = {}               # tensor -> (engine / bar, engine, e_ref, bar, case): printed by test_zz_summary


@pytest.fixture(autouse=True)
def restore_variant():
    from tianshou_amd import mlp3

    prev = mlp3.set_variant(0, 0)
    mlp3.set_variant(*prev)
    yield
    mlp3.set_variant(*prev)


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def device_cases():
    """The table for this device's compute-unit count: the same cases in the same order, the rows around the fill threshold moved."""
    return R.cases(cus())


def device_case(name):
    return R.case_by_name(name, cus())


def check(got, ref, e_ref, what, tensor, case):
    e, bar = R.rel_err(got.cpu(), ref), R.rel_bar(e_ref)
    print(f"    {what}: engine {e:.2e}, float32 reference {e_ref:.2e}, bar {bar:.2e}, engine / bar = {e / bar:.3f}")
    if e == e and e / bar > WORST.get(tensor, (-1.0,))[0]:
        WORST[tensor] = (e / bar, e, e_ref, bar, case)
    assert e_ref < 1e-3, (what, e_ref)
    assert e == e and e < bar, (what, e, e_ref)


class Guarded:
    """A float32 [rows, cols] output inside a buffer with SPARE rows of SENTINEL before it and `extra` + SPARE after it."""

    def __init__(self, rows, cols, extra=0):
        self.buf = torch.full((SPARE + rows + extra + SPARE, cols), SENTINEL, device="cuda")
        self.rows = rows
        self.t = self.buf[SPARE:SPARE + rows + extra]          # what the engine is given: `rows` rows to write, the rest spare

    def written(self):
        return self.t[:self.rows]

    def outside_untouched(self) -> bool:
        return bool((self.buf[:SPARE] == SENTINEL).all()) and bool((self.buf[SPARE + self.rows:] == SENTINEL).all())


def dev(tensors):
    """Device copies, one per DISTINCT tensor object (networks that share their input share the device pointer too)."""
    seen = {}
    return [seen.setdefault(id(t), t.cuda()) for t in tensors]


def run(c, M=None, nets=None, store_h=True, variant=None):
    """One launch of the case (its first `nets` networks, its first `M` rows) under its variant -> dict of Guarded outputs per network."""
    from tianshou_amd import mlp3

    M, n = c.M if M is None else M, c.nets if nets is None else len(nets)
    idx = list(range(c.nets)) if nets is None else list(nets)
    inp, ref = R.inputs_for(c.input_key), R.reference_for(c.input_key)
    pick = lambda seq: [seq[k] for k in idx]          # noqa: E731
    wb1, wb2, wb3 = dev(pick(inp["wb1"])), dev(pick(inp["wb2"])), dev(pick(inp["wb3"]))
    out = {}
    with mlp3.variant(*(variant or (c.nw, c.rb))):
        if c.direction == "fwd":
            x = dev(pick(inp["x"]))
            out = {k: [Guarded(M, w, c.M - M) for _ in range(n)] for k, w in (("h1", R.HID), ("h2", R.HID), ("out", c.head))}
            mlp3.forward(x, wb1, wb2, wb3, [g.t for g in out["h1"]] if store_h else None, [g.t for g in out["h2"]] if store_h else None,
                         [g.t for g in out["out"]], M, c.K1, c.head)
        else:
            d_out, h1, h2 = dev(pick(inp["d_out"])), dev(pick(ref["h1"])), dev(pick(ref["h2"]))
            out = {k: [Guarded(M, w, c.M - M) for _ in range(n)] for k, w in (("dh1", R.HID), ("dh2", R.HID), ("dx", c.K1))}
            col0, col1 = c.cols if c.cols else (0, 0)
            mlp3.backward(d_out, wb1, wb2, wb3, h1, h2, [g.t for g in out["dh1"]], [g.t for g in out["dh2"]],
                          [g.t for g in out["dx"]] if c.cols else None, M, c.K1, c.head, col0, col1)
    torch.cuda.synchronize()
    return out


def check_case(c, out, what=""):
    """Every tensor of every network at the bar; rows >= M, the guard rows and the dx columns outside the covering tiles untouched;
    the dx columns inside the covering tiles but outside [col0, col1) hold the gradient too (they belong to the checked hull)."""
    for name in R.TENSORS[c.direction]:
        for k, g in enumerate(out[name]):
            assert g.outside_untouched(), (c.name, name, k, "rows >= M or the guard rows were written")
            if name == "dx":
                if c.cols is None:
                    assert bool((g.buf == SENTINEL).all()), (c.name, "dx written without a column range")
                    continue
                lo, hi = R.hull(c)
                got = g.written()
                assert bool((got[:, :lo] == SENTINEL).all()) and bool((got[:, hi:] == SENTINEL).all()), (c.name, k, "dx outside its tiles")
                got = got[:, lo:hi]
            else:
                got = g.written()
            assert bool((got != SENTINEL).all()), (c.name, name, k, "an element was left unwritten")
            r64, e_ref = R.expected(c, k, name)
            check(got, r64, e_ref, f"{what}{name}[{k}]", name, c.name)


def same(a, b, names):
    return all(torch.equal(x.written(), y.written()) for n in names for x, y in zip(a[n], b[n]))


def outputs_of(c):
    return [n for n in R.TENSORS[c.direction] if n != "dx" or c.cols is not None]


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_case_against_float64(i):
    """Values, sentinels and a bit-identical rerun of every case of the table."""
    c = device_cases()[i]
    print("\n  " + R.describe(c, cus()))
    assert c.kernel(cus()) == c.meant
    out = run(c)
    check_case(c, out)
    assert same(out, run(c), outputs_of(c)), "a rerun differs"


@pytest.mark.parametrize("direction,head,nw", R.SWEEP_COMBOS, ids=[f"{d}-head{h}-nw{n}" for d, h, n in R.SWEEP_COMBOS])
def test_width_sweep(direction, head, nw):
    """K1 = 32 .. 1024 in steps of 32 at M = 17, one network, nw forced: ring lengths of layer 1 from 1 (eight waves) / 2 (four) to
    32 / 64 blocks per wave, the input tile from 2 KB to 64 KB of LDS; backward: dx over the last tiles of every pitch."""
    for K1 in R.SWEEP_K1:
        c = R.sweep_case(direction, head, nw, K1)
        check_case(c, run(c), what=f"K1 {K1} ")


MULTI = [(d, head, nw) for d in ("fwd", "bwd") for head in R.HEADS for nw in (4, 8)]


@pytest.mark.parametrize("direction,head,nw", MULTI, ids=[f"{d}-head{h}-nw{n}" for d, h, n in MULTI])
def test_network_in_a_shared_launch_equals_its_own_launch(direction, head, nw):
    """ts_mlp.h: "per-row results do not depend on which networks share a launch" -- network k of a three-network launch is
    bit-identical to the single-network launch of the same instantiation on the same rows."""
    c = R.Case(f"shared launch {direction} {head} {nw}", "nets", direction, 3, 33, 96, head, nw, 0, True, (17, 90) if direction == "bwd" else None,
               (direction, head, nw, 1))
    assert c.kernel(cus()) == c.meant and dataclasses.replace(c, nets=1).kernel(cus()) == c.meant
    multi = run(c)
    check_case(c, multi)
    for k in range(3):
        single = run(c, nets=[k])
        for n in outputs_of(c):
            assert torch.equal(single[n][0].written(), multi[n][k].written()), (n, k)


PREFIX = [(d, head, v) for d in ("fwd", "bwd") for head in R.HEADS for v in ((4, 0), (8, 0), (0, 2))]


@pytest.mark.parametrize("direction,head,variant", PREFIX, ids=[f"{d}-head{h}-nw{v[0]}-rb{v[1]}" for d, h, v in PREFIX])
def test_first_rows_of_a_longer_launch_equal_the_shorter_launch(direction, head, variant):
    """A row's result does not depend on the rows after it (rows past M repeat the last row, and are not stored): the first M rows
    of a launch over M' > M rows are bit-identical to the launch over M rows.  32-row workgroups: M = 737 inside M' = 769."""
    if variant[1] == 2:
        r = R.rb2_rows(8, cus())
        c = device_case(f"rb2 {direction} head {head} one_more M {r['one_more']}")
        M = r["one_row_last_tile"]
        assert c.meant[2:] == (8, 2) and R.variant_of(direction, c.nets, M, c.K1, 0, 2, cus()) == (8, 2)
    else:
        c = R.Case(f"prefix {direction} {head} {variant}", "rows", direction, 2, 47, 96, head, variant[0], 0, True,
                   (17, 90) if direction == "bwd" else None, (direction, head, variant[0], 1))
        M = 17
    long, short = run(c), run(c, M=M)
    for n in outputs_of(c):
        for k in range(c.nets):
            assert short[n][k].outside_untouched(), (n, k)
            assert torch.equal(short[n][k].written(), long[n][k].written()[:M]), (n, k)


@pytest.mark.parametrize("head,variant", [(h, v) for h in R.HEADS for v in ((4, 0), (8, 0), (0, 2))], ids=str)
def test_inference_only_chain_gives_the_same_output(head, variant):
    """ts_mlp.h: h1 / h2 = nullptr only skips the stores -- `out` is bit-identical, and nothing is written to the buffers that were
    not handed in."""
    if variant[1] == 2:
        c = device_case(f"rb2 fwd head {head} one_row_last_tile M {R.rb2_rows(8, cus())['one_row_last_tile']}")
    else:
        c = R.Case(f"inference {head} {variant}", "nets", "fwd", 2, 33, 96, head, variant[0], 0, True, None, ("fwd", head, variant[0], 1))
    assert c.kernel(cus()) == c.meant
    full, lean = run(c), run(c, store_h=False)
    assert same(full, lean, ["out"])
    assert all(bool((g.buf == SENTINEL).all()) for n in ("h1", "h2") for g in lean[n])


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("head", R.HEADS)
def test_32_row_workgroups_equal_16_row_workgroups_on_eight_waves(direction, head):
    """The summation order documented at the top of ts_mlp.hip does not involve the row block: RB = 2 is bit-identical to RB = 1 at
    eight waves, on a one-row last tile, a full last tile and one row more."""
    for tag, M in R.rb2_rows(8, cus()).items():
        if tag == "fails":
            continue
        c = device_case(f"rb2 {direction} head {head} {tag} M {M}")
        assert c.meant == (direction, head, 8, 2) and R.variant_of(direction, c.nets, c.M, c.K1, 8, 0, cus()) == (8, 1)
        assert same(run(c), run(c, variant=(8, 0)), outputs_of(c)), tag


@pytest.mark.parametrize("name,direction,over,code,msg", R.REFUSALS, ids=[f"{r[1]} {r[0]}" for r in R.REFUSALS])
def test_refusals(name, direction, over, code, msg):
    """The documented error code, a ts_last_error sentence, and every output still holding the sentinel."""
    from tianshou_amd import _lib, mlp3

    a = R.refusal_args(over)
    assert R.refusal_code(direction, a) == code
    n, M, K1, head = a["nets"], a["M"], a["K1"], a["head"]
    slots, rows, width = max(n, 2), max(M, 17), max(K1, 64)
    t = {k: [torch.ones(rows, w, device="cuda") for _ in range(slots)]
         for k, w in (("x", width), ("d_out", max(head, 32)), ("h1", R.HID), ("h2", R.HID))}
    t.update({k: [torch.ones(r + 1, w, device="cuda") for _ in range(slots)] for k, r, w in (("wb1", width, R.HID), ("wb2", R.HID, R.HID),
                                                                                              ("wb3", R.HID, max(head, 32)))})
    outs = {k: [torch.full((rows, w), SENTINEL, device="cuda") for _ in range(slots)]
            for k, w in (("h1o", R.HID), ("h2o", R.HID), ("out", max(head, 32)), ("dh1", R.HID), ("dh2", R.HID), ("dx", width))}
    arrays = {**t, **{k: v for k, v in outs.items()}}
    lists = {k: list(v[:max(n, 0)]) for k, v in arrays.items()}
    if a["null"]:
        lists[a["null"][0]][a["null"][1]] = None
    dx = [d if keep else None for d, keep in zip(lists["dx"], a["dx"])] if direction == "bwd" else None
    with pytest.raises(_lib.EngineError) as err:
        if direction == "fwd":
            mlp3.forward(lists["x"], lists["wb1"], lists["wb2"], lists["wb3"], lists["h1o"], lists["h2o"], lists["out"], M, K1, head, nets=n)
        else:
            mlp3.backward(lists["d_out"], lists["wb1"], lists["wb2"], lists["wb3"], lists["h1"], lists["h2"], lists["dh1"], lists["dh2"],
                          dx, M, K1, head, *a["cols"], nets=n)
    torch.cuda.synchronize()
    print(f"    {direction} {name}: {err.value}")
    assert err.value.code == code and msg in str(err.value)
    assert all(bool((o == SENTINEL).all()) for v in outs.values() for o in v), "a refused call wrote to an output"


def test_set_variant_returns_the_previous_setting_and_refuses_other_values():
    from tianshou_amd import _lib, mlp3

    start = mlp3.set_variant(4, 0)
    assert mlp3.set_variant(0, 2) == (4, 0) and mlp3.set_variant(8, 0) == (0, 2)
    for bad in ((3, 0), (0, 1), (16, 2)):
        with pytest.raises(_lib.EngineError) as err:
            mlp3.set_variant(*bad)
        assert err.value.code == _lib.TS_ERR_INVALID_ARG
    assert mlp3.set_variant(*start) == (8, 0)
    with mlp3.variant(4, 0):
        assert mlp3.set_variant(4, 0) == (4, 0)
    assert mlp3.set_variant(*start) == start


def test_zz_summary():
    """Prints, per tensor, the largest engine / bar over everything this file compared (run the whole file with -s)."""
    print("\n    tensor   engine / bar   engine     e_ref      bar        case")
    for name in ("h1", "h2", "out", "dh2", "dh1", "dx"):
        if name in WORST:
            ratio, e, e_ref, bar, case = WORST[name]
            print(f"    {name:<8} {ratio:>8.3f}       {e:.2e}   {e_ref:.2e}   {bar:.2e}   {case}")
