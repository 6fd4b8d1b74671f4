"""conv_forward / conv_backward of tianshou_amd.dqn (ts_conv_forward / ts_conv_backward: tianshou_amd/csrc/ts_conv.hip, ts_conv2.hip)
at the sizes where the host code changes kernel, element by element over the whole output against float64: the full-size row tiles
of generation 1 (8192 workgroups and more; also against the same call on batch slices that take the half-size tiles, with a guard
region around every output), M = 1 and M one off a tile edge on the half-size tiles, split forward passes with a short last split,
weight-gradient splits of more than four chunks, every slab-sum kernel at 1 .. 17 slabs, TS_WGRAD_TILE64 / TS_WGRAD_XCD (bit-identical,
as the comments of ts_conv.hip promise), plan 3 of the generation-2 weight gradient, its resident 128-column forward with bias, ReLU
and mask, persistent workgroups that loop over several row tiles with a ragged last one, and the shapes the entry points refuse.
tests/conv_edge_cases.py holds the case table, the inputs and the references and names the kernel of every pass;
tests/test_conv_edge_inputs_cpu.py checks those names.

Yardstick: float64 (conv_edge_cases.reference, evaluated on the device).  Bar of every tensor: max(1e-5, 2 e_ref) of its largest
reference entry; e_ref is torch's own float32 error on the same formula and input, computed from the reference alone, and asserted
below 1e-4 here as well.  `pytest -s` prints engine error, e_ref and bar of every tensor.

Measured on an MI355X (this file's own printout): per tensor the largest engine / bar over all cases, with the engine's rel_err, the
e_ref and the bar of the case it occurred in.  No kernel came closer than a tenth of the bar, and the largest engine error anywhere
is 9.4e-7.  The 2 e_ref term opened the bar only for the weight gradients of the full-size-tile cases (torch's own float32 sum over
131,021 and more rows: up to 7.9e-6, bar 1.57e-5), where the engine stood at 7.3e-7 at most.

    tensor                      engine / bar   engine     e_ref      bar
    y                               0.064      6.44e-07   6.26e-07   1.00e-05
    d_wb                            0.061      6.10e-07   6.10e-07   1.00e-05
    d_b (last row, own scale)       0.032      3.25e-07   1.93e-07   1.00e-05
    dx                              0.094      9.37e-07   9.37e-07   1.00e-05
    TS_WGRAD_TILE64 0 / 1 and TS_WGRAD_XCD 0 / 1: torch.equal on every case

Two deliberate in-bounds errors in the host code -- the last chunk of the last weight-gradient split dropped in conv_wgrad, the
kernels of plans 2 and 3 exchanged in conv2_wgrad -- failed the cases that name those paths (d_wb off by 1e-2 .. 1.3 of its scale).
A third one, the clamp `a.M - 1` of conv_rows_kernel turned into `a.M - 2`, changes only the address that rows PAST M load from;
their products are never stored, so no comparison of outputs can see it (and with M = 1 it is an out-of-bounds read, which no test
here provokes).
"""
import ctypes as C

import pytest
import torch

from tests import conv_edge_cases as R

pytestmark = pytest.mark.gpu

CASE_NAMES = [c.name for c in R.cases()]
LARGE_SLICED = [c.name for c in R.cases() if c.slices]
SENTINEL = -7777.0


@pytest.fixture()
def generation():
    """-> set(mode); the mode the process had is restored afterwards."""
    from tianshou_amd import _lib

    lib = _lib.load()
    prev = lib.ts_conv_set_generation(0)
    lib.ts_conv_set_generation(prev)
    yield lambda mode: lib.ts_conv_set_generation(mode)
    lib.ts_conv_set_generation(prev)


def dims_of(x, kh, kw, s, oc):
    """h_dims of the two entry points: B, IH, IW, IC, KH, KW, S, OC."""
    b, ih, iw, ic = x.shape
    return (C.c_int64 * 8)(b, ih, iw, ic, kh, kw, s, oc), ((ih - kh) // s + 1, (iw - kw) // s + 1)


def device_case(name):
    return R.case_by_name(name, torch.cuda.get_device_properties(0).multi_processor_count)


def check(got, ref, e_ref, what):
    e, bar = R.rel_err(got, ref), R.rel_bar(e_ref)
    print(f"    {what}: engine {e:.2e}, float32 reference {e_ref:.2e}, bar {bar:.2e}, engine / bar = {e / bar:.3f}")
    assert e_ref < 1e-4, (what, e_ref)
    assert e == e and e < bar, (what, e, e_ref)


def engine_passes(c, inp):
    from tianshou_amd import dqn as D

    g = c.g
    y = D.conv_forward(inp["x"], inp["wb"], g.KH, g.KW, g.S, c.relu)
    d_wb, dx = D.conv_backward(inp["x"], inp["wb"], inp["dy"], g.KH, g.KW, g.S, mask=inp["x"] if c.masked else None, need_dx=True)
    return y, d_wb, dx


@pytest.mark.parametrize("name", CASE_NAMES)
def test_layer_against_float64(generation, name):
    c = device_case(name)
    print("\n  " + R.describe(c, R.routes_taken(c)))
    inp = R.make_inputs(c, "cuda")
    ref = R.reference(c, inp)
    generation(c.mode)
    y, d_wb, dx = engine_passes(c, inp)
    torch.cuda.synchronize()
    assert y.shape == (c.g.B, c.g.OH, c.g.OW, c.g.OC)
    check(y.reshape(-1, c.g.OC), ref["y"], ref["e_ref"]["y"], "y")
    del y
    check(d_wb, ref["d_wb"], ref["e_ref"]["d_wb"], "d_wb")
    check(d_wb[-1], ref["d_wb"][-1], ref["e_ref"]["d_b"], "d_b (the last row, on its own scale)")
    check(dx, ref["dx"], ref["e_ref"]["dx"], "dx")
    if c.masked:
        assert bool((dx[inp["x"] <= 0] == 0).all())
    del dx, inp, ref
    torch.cuda.empty_cache()


def guarded(shape, rows_of_guard):
    """A float32 tensor of `shape` inside a buffer with `rows_of_guard` rows of SENTINEL before and after it."""
    n = 1
    for s in shape:
        n *= s
    pad = rows_of_guard * shape[-1]
    buf = torch.full((n + 2 * pad,), SENTINEL, device="cuda")
    return buf, buf[pad:pad + n].view(shape), pad


def guard_untouched(buf, pad):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())


@pytest.mark.parametrize("name", LARGE_SLICED)
def test_full_size_tiles_agree_with_half_tile_slices_and_stay_inside_their_output(generation, name):
    """The full-size row tiles (128 x 64, 256 x 32; forward, input gradient, input gradient with four stride parities) against the
    same call on six consecutive batch slices, each small enough for the half-size tiles, at the float64 bar -- and rows past M of
    the last tile written nowhere: the outputs lie inside buffers with 1024 rows of a sentinel on either side.

    Measured on an MI355X: every slice is BIT-IDENTICAL to the matching part of the full output wherever both run a rows kernel (a
    row tile sums the same chunks in the same order whatever its height); the forward slices of "full dgrad 128x64" take the
    split forward (four partial sums added by split_finish_kernel) and differ from the unsplit full pass by a few float32 ulps."""
    from tianshou_amd import _lib
    from tianshou_amd import dqn as D

    c = device_case(name)
    g = c.g
    inp = R.make_inputs(c, "cuda")
    ref = R.reference(c, inp)
    x, wb, dy = inp["x"], inp["wb"], inp["dy"]
    mask = x if c.masked else None
    generation(c.mode)
    dims, _ = dims_of(x, g.KH, g.KW, g.S, g.OC)
    ws = _lib.default_workspace(0)
    ybuf, y, ypad = guarded((g.B, g.OH, g.OW, g.OC), 1024)
    xbuf, dx, xpad = guarded(tuple(x.shape), 1024)
    d_wb = torch.empty_like(wb)
    _lib.check(_lib.load().ts_conv_forward(ws.handle, _lib.ptr(x), C.c_int(0), _lib.ptr(wb), _lib.ptr(y), dims, C.c_int(int(c.relu)),
                                           _lib.current_stream(x.device)))
    _lib.check(_lib.load().ts_conv_backward(ws.handle, _lib.ptr(x), C.c_int(0), _lib.ptr(wb), _lib.ptr(dy), _lib.ptr(mask), _lib.ptr(d_wb),
                                            _lib.ptr(dx), dims, _lib.current_stream(x.device)))
    torch.cuda.synchronize()
    assert guard_untouched(ybuf, ypad), "forward wrote outside [0, M) rows"
    assert guard_untouched(xbuf, xpad), "input gradient wrote outside its tensor"
    check(y.reshape(-1, g.OC), ref["y"], ref["e_ref"]["y"], "y, full-size tiles")
    check(dx, ref["dx"], ref["e_ref"]["dx"], "dx, full-size tiles")
    y_scale, dx_scale = float(ref["y"].abs().max()), float(ref["dx"].abs().max())
    same_y = same_dx = True
    for lo, hi in R.slice_bounds(c):
        gs = g.with_batch(hi - lo)
        assert R.fwd_route(gs, c.mode)[2] in ("64x64", "128x32") and R.dgrad_route(gs, c.mode)[2] in ("64x64", "128x32")
        ys = D.conv_forward(x[lo:hi], wb, g.KH, g.KW, g.S, c.relu)
        _, dxs = D.conv_backward(x[lo:hi], wb, dy[lo:hi], g.KH, g.KW, g.S, mask=None if mask is None else mask[lo:hi], need_dx=True)
        ey = float((ys - y[lo:hi]).abs().max()) / y_scale
        ex = float((dxs - dx[lo:hi]).abs().max()) / dx_scale
        same_y, same_dx = same_y and torch.equal(ys, y[lo:hi]), same_dx and torch.equal(dxs, dx[lo:hi])
        assert ey < R.rel_bar(ref["e_ref"]["y"]) and ex < R.rel_bar(ref["e_ref"]["dx"]), (lo, hi, ey, ex)
        del ys, dxs
    print(f"    {name}: slices bit-identical to the full pass: forward {same_y}, input gradient {same_dx}")
    del inp, ref, ybuf, xbuf, y, dx
    torch.cuda.empty_cache()


def _weight_gradient(c, inp):
    from tianshou_amd import dqn as D

    return D.conv_backward(inp["x"], inp["wb"], inp["dy"], c.g.KH, c.g.KW, c.g.S, mask=None, need_dx=False)[0].clone()


@pytest.mark.parametrize("name", R.TILE64_CASES)
def test_wgrad_tile64_switch_is_bit_identical(generation, monkeypatch, name):
    """TS_WGRAD_TILE64 (read per call): 64 x 64 against 128 x 64 tiles on K = 32, 96 and 160 -- the last 64-row k tile holds 32 rows --
    "every tiling sums the same chunks in the same order: results are bit-identical" (ts_conv.hip, wgrad_tile64)."""
    c = device_case(name)
    inp = R.make_inputs(c, "cuda")
    ref = R.reference(c, inp)
    generation(c.mode)
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("TS_WGRAD_TILE64", v)
        out[v] = _weight_gradient(c, inp)
    assert torch.equal(out["0"], out["1"])
    check(out["1"], ref["d_wb"], ref["e_ref"]["d_wb"], "d_wb, 64 x 64 tiles")
    check(out["0"], ref["d_wb"], ref["e_ref"]["d_wb"], "d_wb, 128 x 64 tiles")


@pytest.mark.parametrize("name", R.XCD_CASES)
def test_wgrad_xcd_block_order_is_bit_identical(generation, monkeypatch, name):
    """TS_WGRAD_XCD (read per call) on grids of 18 and 6 work items, no multiple of the eight XCDs: xcd_item is "a bijection on
    [0, n): results are bit-identical" (ts_conv.hip)."""
    c = device_case(name)
    assert (lambda kt, ny, ns: kt * ny * ns % 8 != 0)(*R.wgrad_grid(c.g, c.mode))
    inp = R.make_inputs(c, "cuda")
    ref = R.reference(c, inp)
    generation(c.mode)
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("TS_WGRAD_XCD", v)
        out[v] = _weight_gradient(c, inp)
    assert torch.equal(out["0"], out["1"])
    check(out["1"], ref["d_wb"], ref["e_ref"]["d_wb"], "d_wb, XCD-aware block order")
    check(out["0"], ref["d_wb"], ref["e_ref"]["d_wb"], "d_wb, plain block order")


@pytest.mark.parametrize("what,xs,kh,kw,s,oc,wants_dx", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
@pytest.mark.parametrize("mode", [-1, 1])
def test_refusals_stay_refusals(generation, mode, what, xs, kh, kw, s, oc, wants_dx):
    """Shapes outside the kernels' limits raise the error _lib.check raises, in both generations, and the refused pass launches
    nothing: its output keeps the sentinel it was filled with."""
    from tianshou_amd import _lib
    from tianshou_amd import dqn as D

    generation(mode)
    x = torch.relu(torch.randn(xs, device="cuda"))
    wb = torch.randn(kh * kw * xs[3] + 1, oc, device="cuda")
    dims, (oh, ow) = dims_of(x, kh, kw, s, oc)
    lib, ws = _lib.load(), _lib.default_workspace(0)
    if not wants_dx:
        y = torch.full((xs[0], oh, ow, oc), SENTINEL, device="cuda")
        with pytest.raises(_lib.EngineError):
            D.conv_forward(x, wb, kh, kw, s, True)
        with pytest.raises(_lib.EngineError):
            _lib.check(lib.ts_conv_forward(ws.handle, _lib.ptr(x), C.c_int(0), _lib.ptr(wb), _lib.ptr(y), dims, C.c_int(1),
                                           _lib.current_stream(x.device)))
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all())
        return
    y = D.conv_forward(x, wb, kh, kw, s, True)                      # forward and weight gradient of these shapes are served
    dy = torch.randn(y.shape, device="cuda")
    D.conv_backward(x, wb, dy, kh, kw, s, mask=None, need_dx=False)
    with pytest.raises(_lib.EngineError):
        D.conv_backward(x, wb, dy, kh, kw, s, mask=x, need_dx=True)
    dx, d_wb = torch.full(xs, SENTINEL, device="cuda"), torch.empty_like(wb)
    with pytest.raises(_lib.EngineError):
        _lib.check(lib.ts_conv_backward(ws.handle, _lib.ptr(x), C.c_int(0), _lib.ptr(wb), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(d_wb),
                                        _lib.ptr(dx), dims, _lib.current_stream(x.device)))
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all())
