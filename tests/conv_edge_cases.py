"""Route bookkeeping, case table, deterministic inputs, float64 references and the bar for the implicit-GEMM layers
(ts_conv_forward / ts_conv_backward of tianshou_amd/csrc/ts_conv.hip and ts_conv2.hip) at the sizes where the host code changes
kernel.  Shared by tests/test_conv_edge_inputs_cpu.py and tests/test_gpu_conv_edges.py; nothing here touches the HIP path.

Routes.  The functions below restate, constant by constant, the host decisions that pick a kernel; every constant carries the
file:line it was read from.  A route is a readable tuple: ("gen1", "rows", "128x64"), ("gen1", "split", "64x64", 5),
("gen1", "rows-dg", "256x32"), ("gen1", "wgrad", "128x32", 96), ("slab", "few8", 8), ("gen2", "fwd", "res128"),
("gen2", "dgrad", "linear", "res64"), ("gen2", "wgrad", "plan3", 15).  `kernel_of` drops the counts: what is left names one
kernel instantiation, and ALL_KERNELS lists every instantiation reachable from the two entry points.  The compute-unit count
(persistent workgroups of generation 2) is 256 here and the device's on the GPU.

Cases.  Every case names the route it means to hit for each of its passes (forward, weight gradient, slab sum, input gradient);
tests/test_conv_edge_inputs_cpu.py checks that it takes them.  `mode` is the argument of ts_conv_set_generation.

Inputs.  Seeded torch.Generator on the CPU; bias N(0, 0.5^2) (nonzero), weights N(0, 1 / K), layer inputs N(0, 1) -- passed through
a ReLU where the case masks its input gradient, so that exact zeros carry the mask.  d relu / dx jumps at 0: an output whose SIGN
float32 rounding decides has no reference value of the gradient that follows, so batch rows that hold a pre-activation with
|pre| < 32 eps32 (sum_k |x_k w_kj| + |b_j|) in float64 are redrawn (`near_kink_rows`, the rule of tests/redq_edge_cases.py).
dY is N(0, 1), times (y > 0) where the case has a ReLU: the gradient with respect to the pre-activation, as the engines pass it.

References.  Linear layers: x.double() @ w.double() + b.  The K = S convolution: a reshape to patches followed by the same matmul.
Gradients from the same formulas (P^T dY, column sums of dY, dY W^T folded back), never from autograd of the engine's output.

Bar.  rel_bar(e_ref) = max(1e-5, 2 e_ref) of each tensor's largest reference entry: 1e-5 is the layer bar of
tests/test_gpu_dqn.py, e_ref the error of torch's own float32 evaluation of the same formula against float64 on the same input --
computed from the reference alone, never from the engine (the rule of tests/redq_edge_cases.py).
"""
from __future__ import annotations

import dataclasses
import math

import torch

# ---- constants that decide the routes (file:line they were read from; C = tianshou_amd/csrc) ---------------------------------------
BK = 32                          # C/ts_conv.hip:23      reduction chunk of generation 1
CK = 32                          # C/ts_conv2.hip:37     reduction chunk of generation 2
TARGET_WGS = 768                 # C/ts_conv.hip:546     workgroups the split plans aim for
FULL_TILE_WGS = 8192             # C/ts_conv.hip:557     small_rows: half-size row tiles below this many workgroups
FWD_SPLIT_MAX_TILES = 192        # C/ts_conv.hip:569     tiles >= 192: no split forward
FWD_SPLIT_MIN_CHUNKS = 16        # C/ts_conv.hip:569     chunks < 16: no split forward
MIN_CHUNKS_PER_SPLIT = 4         # C/ts_conv.hip:572, :598
SLAB_FEW_MIN_N = 65536           # C/ts_conv.hip:756-760 few<NS> kernels from this many gradient elements on
MAX_DG_CLASSES = 64              # C/ts_conv2.hip:80
MAX_CHUNKS = 512                 # C/ts_conv2.hip:81
LDS_MAX = 160 * 1024             # C/ts_conv2.hip:651
CONV2_MIN_ROWS = 1 << 18         # C/ts_conv2.hip:656
CONV2_FIRST_MIN_ROWS = 1 << 17   # C/ts_conv2.hip:657
LINEAR2_MIN_ROWS = 1 << 14       # C/ts_conv2.hip:658
LINEAR2_MIN_WEIGHTS = 1 << 16    # C/ts_conv2.hip:659
RES_MAX_NB = 8                   # C/ts_conv2.hip:948    resident column blocks per launch
WGRAD2_SLOTS_PER_CU_UNIT = 256   # C/ts_conv2.hip:922    slots = per_cu * 256
CPU_CUS = 256                    # compute units assumed without a device (C/ts_conv2.hip:630)
INT31 = 1 << 31


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclasses.dataclass(frozen=True)
class Geom:
    """ts::ConvGeom (C/ts_conv.h:16-22)."""
    B: int
    IH: int
    IW: int
    IC: int
    KH: int
    KW: int
    S: int
    OC: int

    @property
    def OH(self): return (self.IH - self.KH) // self.S + 1

    @property
    def OW(self): return (self.IW - self.KW) // self.S + 1

    @property
    def K(self): return self.KH * self.KW * self.IC

    @property
    def M(self): return self.B * self.OH * self.OW

    @property
    def in_elems(self): return self.B * self.IH * self.IW * self.IC

    @property
    def out_elems(self): return self.M * self.OC

    @property
    def param_elems(self): return (self.K + 1) * self.OC

    @property
    def linear(self): return self.KH == 1 and self.KW == 1 and self.IH == 1 and self.IW == 1

    def with_batch(self, B: int) -> "Geom":
        return dataclasses.replace(self, B=B)


def linear(M: int, IC: int, OC: int) -> Geom:
    return Geom(M, 1, 1, IC, 1, 1, 1, OC)


# ---- generation 1 (C/ts_conv.hip) --------------------------------------------------------------------------------------------------
def check_geom(g: Geom):
    """:526-536 -> None, or the reason the entry points refuse the shape."""
    if not (g.B > 0 and g.OH > 0 and g.OW > 0):
        return "empty geometry"
    if not (g.K % BK == 0 and (g.KW * g.IC) % 4 == 0 and (g.IW * g.IC) % 4 == 0 and (g.S * g.IC) % 4 == 0):
        return "unsupported shape"
    if g.OC % 32 != 0:
        return "output channels must be a multiple of 32"
    if not (g.in_elems < INT31 and g.out_elems < INT31):
        return "tensor too large"
    return None


def dgrad_refusal(g: Geom):
    """conv_dgrad :721-724."""
    if check_geom(g):
        return check_geom(g)
    if g.KH % g.S != 0 or g.KW % g.S != 0:
        return "kernel size must be a multiple of the stride"
    if g.IC % 32 != 0:
        return "input channels must be a multiple of 32"
    return None


def small_rows(M: int, bn: int, other_tiles: int) -> bool:
    """:553-558 (without the TS_CONV_SMALL override, which is read once per process)."""
    bm = 128 if bn == 64 else 256
    return ceil_div(M, bm) * other_tiles < FULL_TILE_WGS


def _tile(bn: int, small: bool) -> str:
    bm = (128 if bn == 64 else 256) // (2 if small else 1)
    return f"{bm}x{bn}"


def conv_fwd_splits(g: Geom, mode: int, u8: bool = False) -> int:
    """:564-574."""
    if conv2_use_forward(g, mode, False):
        return 1
    bn = 64 if g.OC % 64 == 0 else 32
    bm = 128 if bn == 64 else 256
    tiles = ceil_div(g.M, bm) * (g.OC // bn)
    chunks = g.K // BK
    if tiles >= FWD_SPLIT_MAX_TILES or chunks < FWD_SPLIT_MIN_CHUNKS:
        return 1
    want = ceil_div(TARGET_WGS // 2, tiles)
    per = max(MIN_CHUNKS_PER_SPLIT, ceil_div(chunks, want))
    return ceil_div(chunks, per)


def gen1_wgrad_splits(g: Geom) -> int:
    """:593-599."""
    bn = 64 if g.OC % 64 == 0 else 32
    tiles = ceil_div(g.K, 128) * (g.OC // bn)
    chunks = ceil_div(g.M, BK)
    want = ceil_div(TARGET_WGS, tiles)
    per = max(MIN_CHUNKS_PER_SPLIT, ceil_div(chunks, want))
    return ceil_div(chunks, per)


def conv_wgrad_splits(g: Geom, mode: int) -> int:
    """:589-600."""
    return conv2_wgrad_splits(g) if conv2_use_wgrad(g, mode, False) else gen1_wgrad_splits(g)


def split_sizes(total_chunks: int, nsplit: int) -> list:
    """Chunks of every split as the kernels cut them: a.chunks = ceil(total / nsplit) (:611, :658, ts_conv2.hip:1032), split s
    takes [s a.chunks, min(total, (s + 1) a.chunks)).  An entry <= 0 would be an EMPTY split (a slab of zeros at best)."""
    per = ceil_div(total_chunks, nsplit)
    return [min(total_chunks, (s + 1) * per) - s * per for s in range(nsplit)]


def wgrad_tile64(g: Geom, env=None, grouped: bool = False) -> bool:
    """:584-587; env = the value of TS_WGRAD_TILE64 (None: unset)."""
    return g.OC % 64 == 0 and (int(env) != 0 if env is not None else grouped)


def slab_route(nslab: int, n: int):
    """slab_sum :755-763 (without the TS_SLAB_SUM_FEW override, read once per process)."""
    if n >= SLAB_FEW_MIN_N:
        for ns in (4, 8, 16):
            if nslab <= ns:
                return ("slab", f"few{ns}", nslab)
    return ("slab", "generic", nslab)


# ---- generation 2 (C/ts_conv2.hip) -------------------------------------------------------------------------------------------------
def big_enough(g: Geom, rows: int) -> bool:
    """:661-669 (without TS_CONV2_FIRST_MIN_ROWS, read once per process)."""
    if g.linear:
        return rows >= LINEAR2_MIN_ROWS and g.IC * g.OC >= LINEAR2_MIN_WEIGHTS
    if g.OC == 32 and g.K <= 256:
        return rows >= CONV2_FIRST_MIN_ROWS
    return rows >= CONV2_MIN_ROWS


def shape_ok_rows(g: Geom) -> bool:
    """:780-785."""
    s = max(1, g.S)
    return ((g.KW * g.IC) % CK == 0 and g.K % CK == 0 and g.OC % 32 == 0 and g.OH * g.OW < 65536 and g.OW < 65536
            and g.IH * g.IW < 65536 and g.in_elems < INT31 and g.out_elems < INT31 and g.K <= MAX_CHUNKS * CK
            and g.OC * (g.KH // s) * (g.KW // s) <= MAX_CHUNKS * CK)


def conv2_use_forward(g: Geom, mode: int, u8: bool = False) -> bool:
    """:830-835."""
    if mode < 0 or not shape_ok_rows(g):
        return False
    if u8 and g.OC != 32:
        return False
    return mode > 0 or big_enough(g, g.M)


def conv2_use_wgrad(g: Geom, mode: int, u8: bool = False) -> bool:
    """:883-888."""
    return conv2_use_forward(g, mode, u8)


def tap_segments(IH: int, OH: int, KH: int, S: int, p: int) -> list:
    """:793-802 -> [(lo, n, j0, nj)]."""
    out = []
    n = 0 if IH - p <= 0 else ceil_div(IH - p, S)
    JH = KH // S
    for a in range(n):
        lo, hi = max(0, a - (OH - 1)), min(JH - 1, a)
        nj = max(0, hi - lo + 1)
        j0 = lo if nj else 0
        if out and out[-1][2] == j0 and out[-1][3] == nj:
            out[-1] = (out[-1][0], out[-1][1] + 1, j0, nj)
        else:
            out.append((a, 1, j0, nj))
    return out


def dgrad_class_count(g: Geom) -> int:
    """dgrad_classes :804-826."""
    return sum(len(tap_segments(g.IH, g.OH, g.KH, g.S, ph)) * len(tap_segments(g.IW, g.OW, g.KW, g.S, pw))
               for ph in range(g.S) for pw in range(g.S))


def dgrad_ps_ok(g: Geom, ps_env: int = 1) -> bool:
    """:840-859; ps_env = TS_DGRAD_PS (read per call)."""
    if not (g.S >= 2 and g.IC == 32 and g.S * g.S * g.IC == 128 and g.IH % g.S == 0 and g.IW % g.S == 0 and g.KH % g.S == 0
            and g.KW % g.S == 0 and (g.KH // g.S) * (g.KW // g.S) * g.OC * 128 * 4 <= LDS_MAX and ps_env):
        return False
    r0, c0 = tap_segments(g.IH, g.OH, g.KH, g.S, 0), tap_segments(g.IW, g.OW, g.KW, g.S, 0)
    return all(tap_segments(g.IH, g.OH, g.KH, g.S, p) == r0 and tap_segments(g.IW, g.OW, g.KW, g.S, p) == c0
               for p in range(1, g.S))


def conv2_use_dgrad(g: Geom, mode: int, have_ws: bool = True) -> bool:
    """:861-881 for the whole column range (ts_conv_backward passes its workspace: have_ws; TS_DGRAD_PS_MIN_ROWS is read once
    per process and unset: generation 2 in mode 0 by big_enough alone)."""
    if mode < 0 or not shape_ok_rows(g) or g.IC % 32 != 0:
        return False
    if g.KH % g.S != 0 or g.KW % g.S != 0 or not have_ws:
        return False
    if not g.linear:
        if g.IC > 64:
            return False
        if (g.KH // g.S) * (g.KW // g.S) * g.OC * (64 if g.IC % 64 == 0 else 32) * 4 > LDS_MAX:
            return False
        if g.S * g.S * (2 * (g.KH // g.S) + 1) * (2 * (g.KW // g.S) + 1) > MAX_DG_CLASSES and dgrad_class_count(g) > MAX_DG_CLASSES:
            return False
    return mode > 0 or big_enough(g, g.B * g.IH * g.IW)


def rows2_branch(K: int, N: int, u8: bool = False) -> str:
    """The branches of rows2_forward :949-968."""
    if N == 32 and K * 32 * 4 <= LDS_MAX:
        return "res32-u8" if u8 else "res32"
    if N % 128 == 0 and K * 128 * 4 <= LDS_MAX and N // 128 <= RES_MAX_NB:
        return "res128"
    if N % 64 == 0 and K * 64 * 4 <= LDS_MAX and N // 64 <= RES_MAX_NB:
        return "res64"
    return "streamed"


# BM of launch_one (:747) = (WAVES / WN) TM 32 with the (TN, WN, waves, tm) of every launch_rows2 call (:952-968, :1013-1022)
ROWS2_BM = {"res32-u8": 512, "res32": 512, "res128": 256, "res64": 512, "streamed": 256, "ps": 256, "c64": 512, "c32": 1024}
ROWS2_BN = {"res32-u8": 32, "res32": 32, "res128": 128, "res64": 64, "streamed": 128}


def rows2_tiling(M: int, K: int, N: int, cus: int = CPU_CUS, u8: bool = False):
    """-> (branch, BM, row tiles, persistent workgroups per column block) of a rows2_forward launch (:949-968, launch_one :754-755)."""
    br = rows2_branch(K, N, u8)
    if br.startswith("res32"):
        budget = (2 if K * 32 * 4 <= 40 * 1024 else 1) * cus
    else:
        budget = max(1, cus // ceil_div(N, ROWS2_BN[br]))
    tiles = ceil_div(M, ROWS2_BM[br])
    return br, ROWS2_BM[br], tiles, max(1, min(tiles, budget))


def conv2_dgrad_branch(g: Geom, ps_env: int = 1):
    """conv2_dgrad :976-1023."""
    if g.linear:
        return ("gen2", "dgrad", "linear", rows2_branch(g.OC, g.IC))
    if dgrad_ps_ok(g, ps_env):
        return ("gen2", "dgrad", "ps")
    return ("gen2", "dgrad", "c64" if g.IC % 64 == 0 else "c32")


def wgrad2_plan(g: Geom):
    """:893-912 (without TS_WGRAD2_PLAN, read once per process) -> (plan, bkt, bn, per_cu)."""
    if g.OC % 64 != 0:
        return 0, 256, 32, 2
    k = g.K
    w512, w192, w256 = ceil_div(k, 512) * 512, ceil_div(k, 192) * 192, ceil_div(k, 256) * 256
    plan = 1 if w512 * 100 <= k * 115 else (2 if w192 <= w256 else 3)
    if g.OC % 128 == 0 and w256 * 100 <= k * 115:
        plan = 4
    return {4: (4, 256, 128, 1), 1: (1, 512, 64, 1), 2: (2, 192, 64, 2), 3: (3, 256, 64, 1)}[plan]


def conv2_wgrad_splits(g: Geom) -> int:
    """:914-936."""
    _, bkt, bn, per_cu = wgrad2_plan(g)
    tiles = ceil_div(g.K, bkt) * (g.OC // bn)
    chunks = ceil_div(g.M, CK)
    slots = per_cu * WGRAD2_SLOTS_PER_CU_UNIT
    max_splits = max(1, min(chunks // 8, ceil_div(4 * slots, tiles)))

    def eff_of(sp):
        per = ceil_div(chunks, sp)
        if ceil_div(chunks, per) != sp:
            return 0.0
        wgs = tiles * sp
        return wgs / (ceil_div(wgs, slots) * slots)

    top = max(eff_of(sp) for sp in range(1, max_splits + 1))
    for sp in range(1, max_splits + 1):
        if eff_of(sp) >= top - 0.02:
            return sp
    return 1


# ---- the three passes ----------------------------------------------------------------------------------------------------------------
def fwd_route(g: Geom, mode: int, u8: bool = False):
    """conv_forward :602-637."""
    assert check_geom(g) is None, check_geom(g)
    if conv2_use_forward(g, mode, u8):
        return ("gen2", "fwd", rows2_branch(g.K, g.OC, u8))
    nsplit = conv_fwd_splits(g, mode)
    bn = 64 if g.OC % 64 == 0 else 32
    tile = _tile(bn, small_rows(g.M, bn, g.OC // bn * nsplit))
    return ("gen1", "split", tile, nsplit) if nsplit > 1 else ("gen1", "rows", tile)


def wgrad_route(g: Geom, mode: int, u8: bool = False, tile64_env=None):
    """conv_wgrad :645-674, conv2_wgrad :1025-1052 (without TS_WGRAD2_W16)."""
    assert check_geom(g) is None, check_geom(g)
    if conv2_use_wgrad(g, mode, False):
        assert conv2_use_wgrad(g, mode, u8), "uint8 input with other than 32 output channels is refused"
        plan = wgrad2_plan(g)[0]
        return ("gen2", "wgrad", f"plan{plan}" + ("-u8" if u8 else ""), conv2_wgrad_splits(g))
    tile = "64x64" if wgrad_tile64(g, tile64_env) else ("128x64" if g.OC % 64 == 0 else "128x32")
    return ("gen1", "wgrad", tile, gen1_wgrad_splits(g))


def wgrad_grid(g: Geom, mode: int, tile64_env=None):
    """Grid of a generation-1 weight-gradient launch (:662-670): (k tiles, column tiles, splits)."""
    r = wgrad_route(g, mode, tile64_env=tile64_env)
    assert r[0] == "gen1"
    bm, bn = (int(v) for v in r[2].split("x"))
    return ceil_div(g.K, bm), g.OC // bn, r[3]


def slab_route_of(g: Geom, mode: int):
    """ts_conv_backward :847-852."""
    return slab_route(conv_wgrad_splits(g, mode), g.param_elems)


def dgrad_route(g: Geom, mode: int, ps_env: int = 1):
    """conv_dgrad :719-749 over the whole column range."""
    assert dgrad_refusal(g) is None, dgrad_refusal(g)
    if conv2_use_dgrad(g, mode):
        return conv2_dgrad_branch(g, ps_env)
    bn = 64 if g.IC % 64 == 0 else 32
    rows = g.B * ceil_div(g.IH, g.S) * ceil_div(g.IW, g.S)
    return ("gen1", "rows-dg", _tile(bn, small_rows(rows, bn, g.IC // bn * g.S * g.S)))


def kernel_of(route):
    """The kernel instantiation a route names: the route without its counts."""
    if route[:2] == ("gen1", "split"):
        return ("gen1", "split")
    if route[0] == "slab":
        return route[:2]
    return tuple(route[:3])


GEN1_TILES = ("128x64", "64x64", "256x32", "128x32")
ALL_KERNELS = frozenset(
    [("gen1", "rows", t) for t in GEN1_TILES] + [("gen1", "rows-dg", t) for t in GEN1_TILES] + [("gen1", "split")]
    + [("gen1", "wgrad", t) for t in ("128x64", "64x64", "128x32")] + [("slab", k) for k in ("generic", "few4", "few8", "few16")]
    + [("gen2", "fwd", b) for b in ("res32-u8", "res32", "res128", "res64", "streamed")]
    + [("gen2", "dgrad", b) for b in ("linear", "ps", "c64", "c32")]
    + [("gen2", "wgrad", p) for p in ("plan0-u8", "plan0", "plan1", "plan2", "plan3", "plan4")])

# Deliberately outside: TS_WGRAD2_W16 and the TS_R2_WAVES / TS_R2_TM / TS_R2_KSEQ tuning overrides (and TS_CONV2_RES_MAX_NB,
# TS_DG_OVERHEAD); column-range input gradients and the grouped weight-gradient launch (conv_wgrad_group / slab_sum_multi: not
# reachable from ts_conv_forward / ts_conv_backward, the SAC-family tests run them); every switch that is read once per process.
OUTSIDE = ("TS_WGRAD2_W16", "TS_R2_WAVES", "TS_R2_TM", "TS_R2_KSEQ", "TS_CONV2_RES_MAX_NB", "TS_DG_OVERHEAD",
           "conv_dgrad column ranges", "conv_wgrad_group", "slab_sum_multi")
READ_ONCE_PER_PROCESS = ("TS_CONV_SMALL", "TS_SLAB_SUM_FEW", "TS_WGRAD2_PLAN", "TS_CONV_V2", "TS_CONV2_FIRST_MIN_ROWS",
                         "TS_DGRAD_PS_MIN_ROWS", "TS_WGRAD_NO_GROUP")


def routes_of_shape(B, IH, IW, IC, K, S, OC, u8, modes=(-1, 1)) -> set:
    """Kernels a row of tests/test_gpu_conv2.py::SHAPES runs (both generations, input gradient where that test asks for one)."""
    g, out = Geom(B, IH, IW, IC, K, K, S, OC), set()
    for mode in modes:
        out.add(kernel_of(fwd_route(g, mode, u8)))
        out.add(kernel_of(wgrad_route(g, mode, u8)))
        out.add(kernel_of(slab_route_of(g, mode)))
        if IC % 32 == 0 and K % S == 0:
            out.add(kernel_of(dgrad_route(g, mode)))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    g: Geom
    mode: int                 # ts_conv_set_generation
    relu: bool
    masked: bool              # the input is a ReLU output and masks the input gradient
    fwd: tuple
    wgrad: tuple
    slab: tuple
    dgrad: tuple
    large: bool = False       # full-size-tile case: references on the device, also compared with half-tile slices
    slices: int = 0           # consecutive batch slices that take the half-size tiles (large cases)
    loops: bool = False       # generation 2: more row tiles than persistent workgroups, ragged last tile


def _looping_rows(bm: int, nb: int, cus: int) -> int:
    """Two full row tiles for every persistent workgroup of a column block and 77 rows of a last one."""
    return 2 * bm * max(1, cus // nb) + 77


def cases(cus: int = CPU_CUS) -> list:
    """The case table.  `cus` moves only the row counts of the "loops" cases of generation 2."""
    L = linear
    out = []
    # -- full-size row tiles of generation 1: the smallest row counts with 8192 workgroups (tensors of about 270 MB)
    m128, m256 = 1023 * 128 + 77, 2730 * 256 + 77
    big = [
        ("full fwd 128x64", L(m128, 32, 512), True, True, ("gen1", "rows", "128x64"), ("gen1", "wgrad", "128x64", 96),
         ("slab", "generic", 96), ("gen1", "rows-dg", "128x32"), 6),
        ("full fwd 256x32", L(m256, 32, 96), True, False, ("gen1", "rows", "256x32"), ("gen1", "wgrad", "128x32", 254),
         ("slab", "generic", 254), ("gen1", "rows-dg", "128x32"), 6),
        ("full dgrad 128x64", L(m128, 512, 32), False, True, ("gen1", "rows", "128x32"), ("gen1", "wgrad", "128x32", 187),
         ("slab", "generic", 187), ("gen1", "rows-dg", "128x64"), 6),
        ("full dgrad 256x32", L(m256, 96, 32), True, True, ("gen1", "rows", "128x32"), ("gen1", "wgrad", "128x32", 754),
         ("slab", "generic", 754), ("gen1", "rows-dg", "256x32"), 6),
    ]
    for name, g, relu, masked, f, w, s, d, ns in big:
        out.append(Case(name + " gen -1", g, -1, relu, masked, f, w, s, d, large=True, slices=ns))
    for name, g, relu, masked, f, w, s, d, ns in big:         # mode 0: big_enough leaves narrow layers on generation 1
        out.append(Case(name + " gen 0", g, 0, relu, masked, f, w, s, d, large=True))
    out.append(Case("half fwd 64x64 partner", L(1023 * 128, 32, 512), -1, True, True, ("gen1", "rows", "64x64"),
                    ("gen1", "wgrad", "128x64", 96), ("slab", "generic", 96), ("gen1", "rows-dg", "128x32"), large=True))
    out.append(Case("full dgrad 256x32 conv parities", Geom(m128, 4, 4, 32, 2, 2, 2, 32), -1, True, True, ("gen1", "rows", "128x32"),
                    ("gen1", "wgrad", "128x32", 745), ("slab", "generic", 745), ("gen1", "rows-dg", "256x32"), large=True, slices=6))
    # -- tile edges of the half-size tiles
    for oc, ms, tile, wt in ((64, (1, 63, 64, 65), "64x64", "128x64"), (32, (1, 127, 128, 129), "128x32", "128x32")):
        for m in ms:
            for relu, masked in ((True, True), (True, False), (False, True), (False, False)):
                ns = 2 if m == 129 else 1
                out.append(Case(f"edge {oc} cols M {m} relu {'on' if relu else 'off'} mask {'on' if masked else 'off'}", L(m, oc, oc), -1,
                                relu, masked, ("gen1", "rows", tile), ("gen1", "wgrad", wt, ns), ("slab", "generic", ns),
                                ("gen1", "rows-dg", tile)))
    # -- split forward: a short last split (17 = 4 x 4 + 1, 21 = 5 x 4 + 1), both sides of tiles >= 192 and of chunks < 16
    out += [
        Case("split 17 chunks", L(100, 32 * 17, 64), -1, True, True, ("gen1", "split", "64x64", 5), ("gen1", "wgrad", "128x64", 1),
             ("slab", "generic", 1), ("gen1", "rows-dg", "128x32")),
        Case("split 21 chunks", L(77, 32 * 21, 64), -1, False, False, ("gen1", "split", "64x64", 6), ("gen1", "wgrad", "128x64", 1),
             ("slab", "generic", 1), ("gen1", "rows-dg", "128x32")),
        Case("split 184 tiles", L(23 * 128, 512, 512), -1, True, True, ("gen1", "split", "64x64", 3), ("gen1", "wgrad", "128x64", 23),
             ("slab", "generic", 23), ("gen1", "rows-dg", "64x64")),
        Case("no split 192 tiles", L(23 * 128 + 1, 512, 512), -1, True, True, ("gen1", "rows", "64x64"), ("gen1", "wgrad", "128x64", 24),
             ("slab", "generic", 24), ("gen1", "rows-dg", "64x64")),
        Case("no split 15 chunks", L(100, 480, 64), -1, True, False, ("gen1", "rows", "64x64"), ("gen1", "wgrad", "128x64", 1),
             ("slab", "generic", 1), ("gen1", "rows-dg", "128x32")),
        Case("split 16 chunks", L(100, 512, 64), -1, True, False, ("gen1", "split", "64x64", 4), ("gen1", "wgrad", "128x64", 1),
             ("slab", "generic", 1), ("gen1", "rows-dg", "64x64")),
    ]
    # -- weight gradient: ragged last k tile on the three tilings (TS_WGRAD_TILE64 / TS_WGRAD_XCD: WGRAD_SWITCH_CASES below)
    for k in (32, 96, 160):
        out.append(Case(f"wgrad K {k} OC 64", L(300, k, 64), -1, True, True, ("gen1", "rows", "64x64"), ("gen1", "wgrad", "128x64", 3),
                        ("slab", "generic", 3), ("gen1", "rows-dg", "128x32")))
    out.append(Case("wgrad K 160 OC 96", L(300, 160, 96), -1, True, True, ("gen1", "rows", "128x32"), ("gen1", "wgrad", "128x32", 3),
                    ("slab", "generic", 3), ("gen1", "rows-dg", "128x32")))
    # -- slab sums: n = 513 x 128 = 65664 (a ragged last 1024-block) with 1, 3, 8, 13, 16 and 17 slabs
    for m, ns, kern in ((100, 1, "few4"), (353, 3, "few4"), (1000, 8, "few8"), (1637, 13, "few16"), (2048, 16, "few16"),
                        (2049, 17, "generic")):
        out.append(Case(f"slabs {ns}", L(m, 512, 128), -1, True, False, ("gen1", "split", "64x64", 4),
                        ("gen1", "wgrad", "128x64", ns), ("slab", kern, ns), ("gen1", "rows-dg", "64x64")))
    # -- generation 2, forced
    out += [
        Case("gen2 plan 3", L(4165, 256, 64), 1, True, True, ("gen2", "fwd", "res64"), ("gen2", "wgrad", "plan3", 10),
             ("slab", "generic", 10), ("gen2", "dgrad", "linear", "res128")),
        Case("gen2 plan 3, three column blocks", L(4165, 256, 192), 1, True, False, ("gen2", "fwd", "res64"),
             ("gen2", "wgrad", "plan3", 14), ("slab", "generic", 14), ("gen2", "dgrad", "linear", "res128")),
        Case("gen2 256 -> 256", L(2000, 256, 256), 1, True, True, ("gen2", "fwd", "res128"), ("gen2", "wgrad", "plan4", 5),
             ("slab", "few8", 5), ("gen2", "dgrad", "linear", "res128")),
        Case("gen2 256 -> 256 loops", L(_looping_rows(256, 2, cus), 256, 256), 1, True, True, ("gen2", "fwd", "res128"),
             ("gen2", "wgrad", "plan4", None), ("slab", None, None), ("gen2", "dgrad", "linear", "res128"), loops=True),
        Case("gen2 64 -> 192 loops", L(_looping_rows(512, 3, cus), 64, 192), 1, True, True, ("gen2", "fwd", "res64"),
             ("gen2", "wgrad", "plan2", None), ("slab", "generic", None), ("gen2", "dgrad", "linear", "res64"), loops=True),
        Case("gen2 64 -> 96 loops", L(_looping_rows(256, 1, cus), 64, 96), 1, True, True, ("gen2", "fwd", "streamed"),
             ("gen2", "wgrad", "plan0", None), ("slab", "generic", None), ("gen2", "dgrad", "linear", "res64"), loops=True),
        Case("gen2 M 1 res32", L(1, 64, 32), 1, True, True, ("gen2", "fwd", "res32"), ("gen2", "wgrad", "plan0", 1),
             ("slab", "generic", 1), ("gen2", "dgrad", "linear", "res64")),
        Case("gen2 M 1 res128", L(1, 256, 256), 1, True, True, ("gen2", "fwd", "res128"), ("gen2", "wgrad", "plan4", 1),
             ("slab", "few4", 1), ("gen2", "dgrad", "linear", "res128")),
        Case("gen2 M 1 res64", L(1, 64, 192), 1, True, True, ("gen2", "fwd", "res64"), ("gen2", "wgrad", "plan2", 1),
             ("slab", "generic", 1), ("gen2", "dgrad", "linear", "res64")),
        Case("gen2 M 1 streamed", L(1, 64, 96), 1, True, True, ("gen2", "fwd", "streamed"), ("gen2", "wgrad", "plan0", 1),
             ("slab", "generic", 1), ("gen2", "dgrad", "linear", "res64")),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


def matches(meant, got) -> bool:
    """A route taken against the route a case names; None in the table leaves a count (or a whole pass) to the arithmetic."""
    if meant is None:
        return True
    return len(meant) == len(got) and all(m is None or m == v for m, v in zip(meant, got))


def routes_taken(c: Case) -> dict:
    return dict(fwd=fwd_route(c.g, c.mode), wgrad=wgrad_route(c.g, c.mode), slab=slab_route_of(c.g, c.mode),
                dgrad=dgrad_route(c.g, c.mode))


def case_by_name(name: str, cus: int = CPU_CUS) -> Case:
    return next(c for c in cases(cus) if c.name == name)


def slice_bounds(c: Case) -> list:
    """Consecutive batch slices of a full-size-tile case, each small enough for the half-size tiles."""
    step = ceil_div(c.g.B, c.slices)
    return [(lo, min(c.g.B, lo + step)) for lo in range(0, c.g.B, step)]


# TS_WGRAD_TILE64 0 / 1 (K = 32, 96, 160: one, three and five reduction... k chunks of 32 rows, i.e. a ragged last 64-row k tile)
# and TS_WGRAD_XCD 0 / 1 on a grid of 2 x 3 x 3 = 18 work items (no multiple of 8).  Both are read per call.
TILE64_CASES = ("wgrad K 32 OC 64", "wgrad K 96 OC 64", "wgrad K 160 OC 64")
XCD_CASES = ("wgrad K 160 OC 96", "wgrad K 160 OC 64")

# refusals (GPU file): (what, x shape NHWC, kh, kw, stride, OC, input gradient wanted)
REFUSALS = [
    ("OC 48", (3, 1, 1, 32), 1, 1, 1, 48, False),
    ("K no multiple of 32", (3, 1, 1, 48), 1, 1, 1, 32, False),
    ("input gradient at IC 48", (3, 1, 2, 48), 1, 2, 1, 32, True),
    ("input gradient at K 3, S 2", (3, 5, 5, 32), 3, 3, 2, 32, True),
]


# ---- yardstick -----------------------------------------------------------------------------------------------------------------------
def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| over the whole tensor, relative to the largest reference entry (float64 on the reference's device)."""
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def rel_bar(e_ref: float) -> float:
    return max(1e-5, 2.0 * float(e_ref))


# ---- inputs and references -------------------------------------------------------------------------------------------------------------
EPS32 = float(torch.finfo(torch.float32).eps)
KINK_MARGIN = 32.0 * EPS32
ROW_BLOCK = 1 << 17            # rows per block of the float64 work on large cases (bounds the memory, not the result)


def patches(x: torch.Tensor, g: Geom) -> torch.Tensor:
    """[B, IH, IW, IC] -> the im2col matrix [M, K] of a linear layer or a K = S convolution (a reshape: windows do not overlap)."""
    if g.linear:
        return x.reshape(x.shape[0], g.IC)
    assert g.KH == g.S and g.KW == g.S and g.IH == g.OH * g.S and g.IW == g.OW * g.S, "reshape form: K = S, no remainder"
    B = x.shape[0]
    return x.reshape(B, g.OH, g.KH, g.OW, g.KW, g.IC).permute(0, 1, 3, 2, 4, 5).reshape(B * g.OH * g.OW, g.K)


def unpatch(p: torch.Tensor, g: Geom) -> torch.Tensor:
    """Inverse of `patches`: [M, K] -> [B, IH, IW, IC]."""
    B = p.shape[0] // (g.OH * g.OW)
    if g.linear:
        return p.reshape(B, 1, 1, g.IC)
    return p.reshape(B, g.OH, g.OW, g.KH, g.KW, g.IC).permute(0, 1, 3, 2, 4, 5).reshape(B, g.IH, g.IW, g.IC)


def near_kink_rows(x: torch.Tensor, wb: torch.Tensor, g: Geom) -> torch.Tensor:
    """bool[B]: batch rows with a pre-activation whose sign float32 rounding may decide (float64, reference only)."""
    w, b = wb[:-1].double(), wb[-1].double()
    per, bad = g.OH * g.OW, []
    for lo in range(0, x.shape[0], ROW_BLOCK):
        p = patches(x[lo:lo + ROW_BLOCK], g).double()
        near = ((p @ w + b).abs() < KINK_MARGIN * (p.abs() @ w.abs() + b.abs())).any(dim=1)
        bad.append(near.reshape(-1, per).any(dim=1))
    return torch.cat(bad)


def seed_of(c: Case) -> int:
    g = c.g
    # (the mode is left out: a geometry run in two modes has one set of inputs)
    return (g.B * 31 + g.IC * 7 + g.OC * 3 + g.KH + 2 * c.relu + c.masked) % (1 << 31)


def make_inputs(c: Case, device="cpu") -> dict:
    """x [B, IH, IW, IC], wb [K + 1, OC], dy [B, OH, OW, OC] (float32, on `device`) and the float64 forward they were drawn
    against.  Drawn on the CPU from one seeded generator; the kink test and the forward run on `device`."""
    g = c.g
    gen = torch.Generator().manual_seed(seed_of(c))
    draw = (lambda n: torch.relu(torch.randn(n, g.IH, g.IW, g.IC, generator=gen))) if c.masked else \
        (lambda n: torch.randn(n, g.IH, g.IW, g.IC, generator=gen))
    x = draw(g.B).to(device)
    wb = torch.cat([torch.randn(g.K, g.OC, generator=gen) / math.sqrt(g.K), 0.5 * torch.randn(1, g.OC, generator=gen)]).to(device)
    if c.relu:
        for _ in range(200):
            bad = near_kink_rows(x, wb, g)
            n = int(bad.sum())
            if n == 0:
                break
            x[bad] = draw(n).to(device)
        else:
            raise AssertionError("no batch off the ReLU kink found")
    y64 = forward64(c, x, wb)
    dy = torch.randn(g.B, g.OH, g.OW, g.OC, generator=gen).to(device)
    if c.relu:
        dy = dy * (y64 > 0).reshape(dy.shape)
    return dict(x=x, wb=wb, dy=dy, y64=y64)


def _forward(c: Case, x, wb, dtype):
    g, w, b = c.g, wb[:-1].to(dtype), wb[-1].to(dtype)
    out = torch.empty(x.shape[0] * g.OH * g.OW, g.OC, dtype=dtype, device=x.device)
    per = g.OH * g.OW
    for lo in range(0, x.shape[0], ROW_BLOCK):
        y = patches(x[lo:lo + ROW_BLOCK], g).to(dtype) @ w + b
        out[lo * per:lo * per + y.shape[0]] = torch.relu(y) if c.relu else y
    return out


def forward64(c: Case, x, wb) -> torch.Tensor:
    """float64 [M, OC]: x.double() @ w.double() + b, ReLU where the case has one."""
    return _forward(c, x, wb, torch.float64)


def _backward(c: Case, x, wb, dy, dtype, whole: bool):
    """-> (d_wb [K + 1, OC], dx [B, IH, IW, IC]) from P^T dY, the column sums of dY and dY W^T folded back, times (x > 0) where
    the case masks.  whole: one matmul over all rows (torch's own float32 evaluation); otherwise row blocks summed in `dtype`."""
    g, w = c.g, wb[:-1].to(dtype)
    per, step = g.OH * g.OW, (x.shape[0] if whole else ROW_BLOCK)
    gw = torch.zeros(g.K + 1, g.OC, dtype=dtype, device=x.device)
    dx = torch.empty(x.shape, dtype=dtype, device=x.device)
    d = dy.reshape(-1, g.OC)
    for lo in range(0, x.shape[0], step):
        xs = x[lo:lo + step]
        p, ds = patches(xs, g).to(dtype), d[lo * per:(lo + step) * per].to(dtype)
        gw[:-1] += p.t() @ ds
        gw[-1] += ds.sum(dim=0)
        gx = unpatch(ds @ w.t(), g)
        dx[lo:lo + step] = gx * (xs > 0).to(dtype) if c.masked else gx
    return gw, dx


def reference(c: Case, inp: dict) -> dict:
    """float64 values y [M, OC], d_wb, dx and e_ref of each (d_b: the bias row of d_wb on its own scale): the rel_err of the same
    formulas in float32 (whole-matrix matmuls)."""
    x, wb, dy = inp["x"], inp["wb"], inp["dy"]
    y64 = inp["y64"]
    gw64, dx64 = _backward(c, x, wb, dy, torch.float64, whole=False)
    y32 = _forward(c, x, wb, torch.float32)
    e_y = rel_err(y32, y64)
    del y32
    gw32, dx32 = _backward(c, x, wb, dy, torch.float32, whole=True)
    e = dict(y=e_y, d_wb=rel_err(gw32, gw64), d_b=rel_err(gw32[-1], gw64[-1]), dx=rel_err(dx32, dx64))
    return dict(y=y64, d_wb=gw64, dx=dx64, e_ref=e)


def describe(c: Case, taken: dict) -> str:
    g = c.g
    shape = f"{g.IC} -> {g.OC} M {g.M}" if g.linear else f"conv {g.IH}x{g.IW}x{g.IC} k{g.KH} s{g.S} -> {g.OC}, B {g.B} (M {g.M})"
    return f"{c.name}: {shape}, mode {c.mode}: " + ", ".join(f"{k} {'/'.join(str(v) for v in r)}" for k, r in taken.items())
