"""CPU: the case table of tests/mlp3_edge_cases.py does what it claims before a GPU sees it.  Every case takes the kernel
instantiation it names and all twelve instantiations of mlp3_fwd_kernel / mlp3_bwd_kernel are covered, each with a ragged last row
tile; the width sweep holds the ring lengths and the boundaries it is there for; the inputs can tell networks, columns and rows
apart; every batch is off the ReLU kink; the float32 reference error stays below 1e-3, so the 2 e_ref term of the bar is never a
loophole; the refusal cases are refused by the restated rules."""
import pytest
import torch

from tests import mlp3_edge_cases as R
from tests import redq_edge_cases as RQ

CASES = R.cases()
SWEEP = R.sweep_cases()


def test_every_case_takes_the_kernel_it_names_and_all_twelve_are_covered():
    assert len(R.ALL_KERNELS) == 12
    for c in CASES + SWEEP:
        assert c.kernel() == c.meant and c.meant in R.ALL_KERNELS, c.name
        d, n3, NW, RB = c.meant
        nt = R.dx_tiles(*c.cols)[1] if c.cols else 0
        assert R.lds_bytes(d, n3, c.K1, NW, RB) <= R.LDS_MAX, c.name
        assert R.part_fits(d, n3, c.K1, NW, RB, nt), c.name
        assert R.refusal_code(d, dict(R.BASE, nets=c.nets, M=c.M, K1=c.K1, head=c.head, cols=c.cols or (0, 1),
                                      dx=(c.cols is not None,) * c.nets)) is None, c.name
    assert {c.meant for c in CASES} == R.ALL_KERNELS
    assert {c.meant for c in CASES if c.ragged} == R.ALL_KERNELS, "every instantiation with a ragged last tile"
    # the instantiations the suite never launched before: a 64-column head on four waves, every 32-row one
    assert {c.meant for c in CASES if c.group == "variant" and c.nw == 0 and c.rb == 0} >= {("fwd", 64, 4, 1), ("bwd", 64, 4, 1)}


def test_row_cases():
    for direction in ("fwd", "bwd"):
        for nets, NW in ((1, 8), (2, 4)):
            got = {c.M for c in CASES if c.group == "rows" and c.direction == direction and c.nets == nets and c.meant[2:] == (NW, 1)}
            assert got >= set(R.ROW_EDGES), (direction, nets)
    r = R.rb2_rows(8)
    assert r == dict(one_row_last_tile=737, full=768, one_more=769, fails=736)
    assert R.fills(8, r["one_row_last_tile"], 256) and not R.fills(8, r["fails"], 256)
    for direction in ("fwd", "bwd"):
        for head in R.HEADS:
            by_m = {c.M: c for c in CASES if c.name.startswith(f"rb2 {direction} head {head} ")}
            assert sorted(by_m) == [736, 737, 768, 769]
            assert all(by_m[m].meant == (direction, head, 8, 2) for m in (737, 768, 769))
            assert by_m[736].meant == (direction, head, 4, 1), "below the threshold: the 16-row four-wave kernel"
            assert by_m[737].M % 32 == 1 and by_m[768].M % 32 == 0 and by_m[769].M % 32 == 1
    # the 32-row forward overlays its second activation on the input tile: both orders of their sizes, and the first K1 it refuses
    assert R.LDS32_LAST_K1 == 448 and 32 * (448 + 4) > 32 * R.HP > 32 * (160 + 4)
    assert R.case_by_name("rb2 fwd K1 448").meant == ("fwd", 32, 8, 2) and R.case_by_name("rb2 fwd K1 480").meant == ("fwd", 32, 4, 1)
    # with another compute-unit count the threshold moves and the cases follow it
    assert R.rb2_rows(8, 304)["one_row_last_tile"] == 32 * 28 + 1
    assert {c.meant for c in R.cases(304) if c.name.startswith("rb2 bwd head 32 one_row")} == {("bwd", 32, 8, 2)}


def test_width_sweep_ring_lengths_and_boundaries():
    assert len(SWEEP) == 256 and R.SWEEP_K1 == tuple(range(32, 1025, 32)) and R.SWEEP_M == 17
    assert {(c.direction, c.head, c.nw) for c in SWEEP} == set(R.SWEEP_COMBOS) and all(c.meant[2] == c.nw for c in SWEEP)
    # blocks per wave of layer 1 of the forward pass: below the ring length, exactly one trip with an empty tail, a trip and a tail.
    # K1 is a multiple of 32, so four waves (no k split in the hidden layers) see even counts only: 10 = 8 + 2 is their shortest tail
    for NW, want in ((8, {224: (7, 0, 7), 256: (8, 1, 0), 288: (9, 1, 1)}), (4, {96: (6, 0, 6), 128: (8, 1, 0), 160: (10, 1, 2)})):
        for K1, (nbw, trips, tail) in want.items():
            assert K1 in R.SWEEP_K1
            s = R.layer_streams("fwd", 32, K1, NW)[0]
            assert (s["nbw"], s["trips"], s["tail"]) == (nbw, trips, tail), (NW, K1, s)
        lengths = {R.layer_streams("fwd", 32, K1, NW)[0]["nbw"] for K1 in R.SWEEP_K1}
        assert min(lengths) < R.NST and R.NST in lengths and max(lengths) == 1024 // 16 // (NW // 4)
    # both sides of the automatic four- / eight-wave boundary for several networks, on both kernels
    assert R.LDS4_LAST_K1 == 480 and {480, 512} <= set(R.SWEEP_K1)
    assert RQ.forward_kernel(2, 480) == "four-wave" and RQ.forward_kernel(2, 512) == "eight-wave"
    assert {c.meant for c in CASES if c.name.startswith("auto nets 2 fwd K1 480")} == {("fwd", 32, 4, 1), ("fwd", 64, 4, 1)}
    assert {c.meant for c in CASES if c.name.startswith("auto nets 2 fwd K1 512")} == {("fwd", 32, 8, 1), ("fwd", 64, 8, 1)}
    # what the sweep adds to the automatic dispatch: four waves above the boundary, eight waves on a 64-column head
    assert any(c.meant == ("fwd", 64, 4, 1) and c.K1 > 480 for c in SWEEP) and any(c.meant == ("fwd", 32, 4, 1) and c.K1 == 1024 for c in SWEEP)
    # the backward sweep writes the last tiles of every input width
    assert all(c.cols[1] == c.K1 and R.dx_tiles(*c.cols)[1] in (2, 3, 4) for c in SWEEP if c.direction == "bwd")


def test_network_variant_and_range_cases():
    nets = [c for c in CASES if c.group == "nets"]
    assert {c.nets for c in nets} == set(R.NETS) == {1, 2, 3, 4, 5, 8}
    fwd = [c for c in nets if c.direction == "fwd"]
    assert sum(c.own_x for c in fwd) == sum(not c.own_x for c in fwd) == len(R.NETS)
    var = [c for c in CASES if c.group == "variant" and c.name.startswith("variant")]
    assert {(c.direction, c.head, c.nw, c.rb, c.nets) for c in var} == {(d, h, nw, rb, n) for d in ("fwd", "bwd") for h in R.HEADS
                                                                        for nw, rb in R.VARIANTS for n in (1, 3)}
    # eight waves with several networks below K1 = 512, four waves with one network: only a forced nw gives these
    assert any(c.meant[2:] == (8, 1) and c.nets == 3 and c.nw == 8 for c in var) and any(c.meant[2:] == (4, 1) and c.nets == 1 for c in var)
    dx = [c for c in CASES if c.group == "dx"]
    for NW in (4, 8):
        for n in (1, 2):
            mine = [c for c in dx if c.nw == NW and c.nets == n and c.meant[2] == NW]
            assert {(c.cols[0], c.cols[1], c.K1) for c in mine} == set(R.DX_RANGES)
            assert {R.dx_tiles(*c.cols)[1] for c in mine if c.cols[0] % 16} == set(range(1, 9)), "1 .. 8 tiles with an unaligned first column"
    named = {(0, 1), (15, 17), (17, 23), (159, 160), (0, 64), (0, 65), (3, 128), (376, 393), (896, 1024)}
    assert named <= {(a, b) for a, b, _ in R.DX_RANGES} and (376, 393, 416) in R.DX_RANGES and (896, 1024, 1024) in R.DX_RANGES
    # five to eight tiles: two column blocks, the second with clamped duplicate tiles unless all eight are wanted
    for nt, dup in ((4, 0), (5, 3), (6, 2), (7, 1), (8, 0)):
        s = R.stream(R.HID, 16 * nt, 4, 8)
        assert (s["ncw"], s["dup"]) == ((1, 0) if nt <= 4 else (2, dup)), (nt, s)
    assert R.stream(R.HID, 16, 4, 4) == dict(ncw=1, nks=4, nbw=4, trips=0, tail=4, dup=3)
    assert R.stream(R.HID, 0, 4, 8)["nbw"] == 0            # no dx: the third layer has no work


@pytest.mark.parametrize("group", ["rows", "nets", "variant", "dx", "width"])
def test_inputs_tell_things_apart_and_the_reference_error_is_small(group):
    worst = 0.0
    for c in (SWEEP if group == "width" else [c for c in CASES if c.group == group]):
        inp = R.inputs_for(c.input_key)
        assert inp["redraws"] <= R.MAX_REDRAWS
        for k in range(c.nets):
            assert not bool(R.near_kink_rows(inp["x"][k], inp["wb1"][k], inp["wb2"][k]).any()), (c.name, k)
            assert inp["x"][k].shape == (c.M, c.K1) and inp["d_out"][k].shape == (c.M, c.head)       # no row was dropped
            assert bool((inp["d_out"][k].abs().amax(dim=0) > 0).all()) and bool((inp["d_out"][k] != 0).all()), "dense upstream gradient"
            for wb in (inp["wb1"][k], inp["wb2"][k], inp["wb3"][k]):
                assert bool((wb[-1] != 0).all()) and float((wb[:-1] != 0).double().mean()) > 0.9999     # nonzero biases, dense weights
            for j in range(k):
                for name in ("wb1", "wb2", "wb3", "d_out"):
                    assert not bool((inp[name][k] == inp[name][j]).any()), (c.name, name, k, j)     # no two networks share a number
                if c.own_x:
                    assert not bool((inp["x"][k] == inp["x"][j]).any())
                else:
                    assert inp["x"][k] is inp["x"][j]
        ref = R.reference_for(c.input_key)
        for k in range(c.nets):
            r = ref["ref64"][k]
            # both signs of every mask occur, so a mask read from the wrong row or column changes the result
            for h in (r["h1"], r["h2"]):
                assert 0.2 < float((h > 0).double().mean()) < 0.8
            if c.M > 1:
                assert not torch.equal(r["h1"][0] > 0, r["h1"][c.M - 1] > 0)
        e = R.worst_e_ref(c)
        assert e < 1e-3, (c.name, e)
        worst = max(worst, e)
    print(f"  {group}: worst e_ref {worst:.2e}")


def test_refusal_cases_are_refused_by_the_restated_rules():
    names = [r[0] for r in R.REFUSALS]
    for want in ["K1 0", "K1 16", "K1 48", "K1 1056", "head 16", "head 96", "head 128", "nets 0", "nets 9", "M 0", "col0 == col1",
                 "col1 > K1", "nine tiles [0, 129)", "nine tiles [15, 144)", "dx for network 0 only", "dx for network 1 only"]:
        assert want in names
    assert any(n.startswith("NULL") for n in names)
    for name, direction, over, code, _ in R.REFUSALS:
        assert R.refusal_code(direction, R.refusal_args(over)) == code, name
    assert R.refusal_code("fwd", R.BASE) is None and R.refusal_code("bwd", R.BASE) is None
    assert R.dx_tiles(0, 129) == (0, 9) and R.dx_tiles(15, 144) == (0, 9) and R.dx_tiles(0, 128) == (0, 8)
