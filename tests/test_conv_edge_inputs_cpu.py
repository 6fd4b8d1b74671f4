"""CPU checks of tests/conv_edge_cases.py: every case of tests/test_gpu_conv_edges.py takes, pass by pass, the kernel it names; the
cases (with the rows of tests/test_gpu_conv2.py::SHAPES for the routes that file already runs) reach every kernel instantiation
that ts_conv_forward / ts_conv_backward can launch; no split plan ever leaves a split empty; the inputs can tell a wrong kernel from
a right one (rows and column blocks all different, 20 - 80 % of the ReLU outputs positive, nothing on the kink); and torch's own
float32 error against float64 (e_ref, what the GPU bars are built from) stays below 1e-4.  `pytest -s` prints routes and figures."""
import pytest
import torch

from tests import conv_edge_cases as R
from tests.test_gpu_conv2 import SHAPES

CASES = R.cases()


def test_every_case_takes_the_routes_it_names():
    for c in CASES:
        taken = R.routes_taken(c)
        print("  " + R.describe(c, taken))
        for k, got in taken.items():
            assert R.matches(getattr(c, k), got), (c.name, k, getattr(c, k), got)
        assert R.check_geom(c.g) is None and R.dgrad_refusal(c.g) is None
        assert max(c.g.in_elems, c.g.out_elems) * 4 <= 300e6, c.name                    # every tensor under about 300 MB


def test_the_edges_the_table_is_there_for():
    by = {c.name: c for c in CASES}
    # full-size tiles: exactly at the 8192-workgroup threshold, the partner one row tile below it, slices on the half tiles
    assert R.FULL_TILE_WGS == 8192 and not R.small_rows(1023 * 128 + 1, 64, 8) and R.small_rows(1023 * 128, 64, 8)
    assert not R.small_rows(2730 * 256 + 1, 32, 3) and R.small_rows(2730 * 256, 32, 3)
    large = [c for c in CASES if c.large]
    assert {R.kernel_of(c.fwd) for c in large} >= {("gen1", "rows", "128x64"), ("gen1", "rows", "256x32"), ("gen1", "rows", "64x64")}
    assert {R.kernel_of(c.dgrad) for c in large} >= {("gen1", "rows-dg", "128x64"), ("gen1", "rows-dg", "256x32")}
    assert sum(c.mode == 0 for c in large) == 4 and by["full dgrad 256x32 conv parities"].g.S ** 2 == 4
    for c in large:
        if c.name != "half fwd 64x64 partner":
            sizes = R.split_sizes(R.ceil_div(c.g.M, R.BK), c.wgrad[3])
            assert sizes[0] > 4 and 0 < sizes[-1] < sizes[0] and c.g.M % R.BK != 0, (c.name, sizes)     # per > 4, short last split
        for lo, hi in (R.slice_bounds(c) if c.slices else []):
            g = c.g.with_batch(hi - lo)
            f, d = R.fwd_route(g, c.mode), R.dgrad_route(g, c.mode)
            assert f[0] == d[0] == "gen1" and f[2] in ("64x64", "128x32") and d[2] in ("64x64", "128x32"), (c.name, f, d)
        if c.slices:
            assert R.slice_bounds(c)[0][0] == 0 and R.slice_bounds(c)[-1][1] == c.g.B
    # half-size tile edges
    assert {c.g.B for c in CASES if c.name.startswith("edge 64")} == {1, 63, 64, 65}
    assert {c.g.B for c in CASES if c.name.startswith("edge 32")} == {1, 127, 128, 129}
    # split forward: a short last split, both sides of the two conditions
    assert R.split_sizes(17, 5) == [4, 4, 4, 4, 1] and R.split_sizes(21, 6) == [4, 4, 4, 4, 4, 1]
    a, b = by["split 184 tiles"].g, by["no split 192 tiles"].g
    assert R.ceil_div(a.M, 128) * (a.OC // 64) == 184 < R.FWD_SPLIT_MAX_TILES == R.ceil_div(b.M, 128) * (b.OC // 64) and b.M == a.M + 1
    assert by["no split 15 chunks"].g.K // R.BK == 15 and by["split 16 chunks"].g.K // R.BK == R.FWD_SPLIT_MIN_CHUNKS
    # weight-gradient switches: the 64-row tiling on K = 32, 96, 160 (ragged last k tile), a grid of 18 and of 6 work items
    for name in R.TILE64_CASES:
        g = by[name].g
        assert g.K % 64 == 32 and R.wgrad_route(g, -1, tile64_env="1")[2] == "64x64" and R.wgrad_route(g, -1, tile64_env="0")[2] == "128x64"
    for name in R.XCD_CASES:
        kt, ny, ns = R.wgrad_grid(by[name].g, -1)
        assert (kt * ny * ns) % 8 != 0, name
    assert R.wgrad_grid(by[R.XCD_CASES[0]].g, -1) == (2, 3, 3)
    # slab sums: 1, 3, 8, 13, 16, 17 slabs of n = 65664 (a ragged last 1024-block), and a slab count below NS in every few<NS>
    slabs = [c for c in CASES if c.name.startswith("slabs")]
    assert [c.slab[1:] for c in slabs] == [("few4", 1), ("few4", 3), ("few8", 8), ("few16", 13), ("few16", 16), ("generic", 17)]
    assert all(c.g.param_elems == 65664 >= R.SLAB_FEW_MIN_N and c.g.param_elems % 1024 != 0 for c in slabs)
    assert any(c.slab[1] == "generic" and c.g.param_elems < R.SLAB_FEW_MIN_N for c in CASES)
    # generation 2
    assert R.wgrad2_plan(by["gen2 plan 3"].g)[:3] == (3, 256, 64) and by["gen2 plan 3, three column blocks"].g.OC // 64 == 3
    loops = [c for c in CASES if c.loops]
    assert {c.fwd[2] for c in loops} == {"res128", "res64", "streamed"}
    for cus in (R.CPU_CUS, 304, 64):                                                    # whatever the device's compute-unit count
        for c in (x for x in R.cases(cus) if x.loops):
            br, bm, tiles, wgs = R.rows2_tiling(c.g.M, c.g.K, c.g.OC, cus)
            assert br == c.fwd[2] and tiles >= 2 * wgs + 1 and c.g.M % bm == 77, (c.name, cus, br, bm, tiles, wgs)
    assert {c.fwd[2] for c in CASES if c.mode == 1 and c.g.M == 1} == {"res32", "res128", "res64", "streamed"}
    # the hidden shape of tests/test_gpu_conv2.py: four resident 64-column blocks (K = 384: a 128-column block does not fit)
    assert R.rows2_branch(384, 256) == "res64" and 384 * 128 * 4 > R.LDS_MAX and R.rows2_branch(256, 256) == "res128"


def test_the_table_and_conv2_shapes_reach_every_reachable_kernel():
    mine = set()
    for c in CASES:
        mine |= {R.kernel_of(r) for r in R.routes_taken(c).values()}
    by = {c.name: c for c in CASES}
    mine |= {R.kernel_of(R.wgrad_route(by[n].g, -1, tile64_env="1")) for n in R.TILE64_CASES}       # test_wgrad_tile64_... of the GPU file
    borrowed = set()
    for s in SHAPES:
        borrowed |= R.routes_of_shape(*s[1:])
    only_borrowed = sorted(R.ALL_KERNELS - mine)
    print("  kernels reached by the case table:", len(mine), "of", len(R.ALL_KERNELS))
    print("  reached through tests/test_gpu_conv2.py::SHAPES alone:", only_borrowed)
    assert mine | borrowed == R.ALL_KERNELS
    assert only_borrowed == [("gen2", "dgrad", "c32"), ("gen2", "dgrad", "c64"), ("gen2", "dgrad", "ps"), ("gen2", "fwd", "res32-u8"),
                             ("gen2", "wgrad", "plan0-u8"), ("gen2", "wgrad", "plan1")]
    assert len(R.ALL_KERNELS) == 31 and len(R.OUTSIDE) == 9 and "TS_CONV_SMALL" in R.READ_ONCE_PER_PROCESS
    print("  deliberately outside:", ", ".join(R.OUTSIDE), "; read once per process:", ", ".join(R.READ_ONCE_PER_PROCESS))


def test_no_split_plan_leaves_a_split_empty():
    """a.chunks = ceil(total / nsplit) with nsplit = ceil(total / per): the last split starts at (nsplit - 1) a.chunks < total."""
    def check(total, nsplit, what):
        sizes = R.split_sizes(total, nsplit)
        assert min(sizes) >= 1 and sum(sizes) == total, (what, total, nsplit, sizes)

    for c in CASES:
        check(c.g.K // R.BK, R.conv_fwd_splits(c.g, c.mode), c.name)
        check(R.ceil_div(c.g.M, R.BK), R.conv_wgrad_splits(c.g, c.mode), c.name)
    n = 0
    for oc in (32, 64, 96, 128, 192, 256, 512):
        for k in (32, 64, 96, 160, 256, 480, 512, 544, 576, 672, 1024, 3136):
            for m in list(range(1, 300)) + list(range(300, 70000, 193)) + [131021, 698957]:
                g = R.linear(m, k, oc)
                check(k // R.BK, R.conv_fwd_splits(g, -1), ("fwd", m, k, oc))
                check(R.ceil_div(m, R.BK), R.gen1_wgrad_splits(g), ("wgrad", m, k, oc))
                check(R.ceil_div(m, R.CK), R.conv2_wgrad_splits(g), ("wgrad2", m, k, oc))
                n += 3
    print(f"  {n} split plans, none with an empty split")


def test_refusals_are_refusals_by_the_rules():
    for what, xs, kh, kw, s, oc, dx in R.REFUSALS:
        g = R.Geom(*xs, kh, kw, s, oc)
        assert (R.dgrad_refusal(g) if dx else R.check_geom(g)) is not None, what
        if dx:
            assert R.check_geom(g) is None, what          # forward and weight gradient are fine: the input gradient is what is refused


@pytest.fixture(scope="module")
def measured():
    """Inputs, float64 reference and e_ref of every case, once per module: name -> (checks on the inputs, e_ref)."""
    out = {}
    for c in CASES:
        if c.mode == 0:                                    # the same geometry and seed as its "gen -1" twin: the same inputs
            continue
        inp = R.make_inputs(c)
        ref = R.reference(c, inp)
        g, x, wb = c.g, inp["x"], inp["wb"]
        probe = torch.randn(g.K, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        keys = R.patches(x, g).double() @ probe
        blocks = wb[:-1].reshape(g.K, g.OC // 32, 32).permute(1, 0, 2).reshape(g.OC // 32, -1)
        out[c.name] = dict(
            rows_differ=int(torch.unique(keys).numel()) == g.M,
            blocks_differ=int(torch.unique(blocks, dim=0).shape[0]) == g.OC // 32,
            positive=float((ref["y"] > 0).double().mean()),
            kink=int(R.near_kink_rows(x, wb, g).sum()) if c.relu else 0,
            bias_nonzero=bool((wb[-1] != 0).all()),
            mask_zeros=float((x == 0).double().mean()),
            dy_follows_relu=bool((inp["dy"].reshape(-1, g.OC)[ref["y"] <= 0] == 0).all()) if c.relu else True,
            e_ref=ref["e_ref"])
        del inp, ref
    return out


def test_inputs_tell_kernels_apart_and_the_float32_reference_is_tight(measured):
    for c in CASES:
        if c.name not in measured:
            continue
        m = measured[c.name]
        e = m["e_ref"]
        print(f"  {c.name}: e_ref y {e['y']:.2e} d_wb {e['d_wb']:.2e} d_b {e['d_b']:.2e} dx {e['dx']:.2e}; positive {m['positive']:.2f}, "
              f"zeros in x {m['mask_zeros']:.2f}")
        assert m["rows_differ"] and m["blocks_differ"] and m["bias_nonzero"] and m["kink"] == 0 and m["dy_follows_relu"], (c.name, m)
        if c.relu:
            assert 0.2 <= m["positive"] <= 0.8, (c.name, m["positive"])
        assert (0.3 < m["mask_zeros"] < 0.7) if c.masked else m["mask_zeros"] < 1e-6, c.name
        assert max(e.values()) < 1e-4, (c.name, e)
