"""Route bookkeeping, case table, deterministic inputs, float64 references and the bar for the fused three-layer MLP kernels
(mlp3_fwd_kernel / mlp3_bwd_kernel<N3, NW, RB> of tianshou_amd/csrc/ts_mlp.hip behind ts_mlp3_forward / ts_mlp3_backward /
ts_mlp3_set_variant) at the row counts, input widths, network counts, variants and input-gradient ranges where the host code or
the kernels change path.  Shared by tests/test_mlp3_edge_inputs_cpu.py and tests/test_gpu_mlp3_edges.py; nothing here touches HIP.

Routes.  The functions below restate, constant by constant, what mlp3_forward_nx / mlp3_backward_n decide (`two`, `four`, the LDS
sizes, the grid) and what WStream / mlp_layer derive per layer (column blocks ncw, k splits nks, blocks per wave nbw, trips of the
eight-stage ring and the tail after them); every constant carries the file:line it was read from.  A kernel is the tuple
(direction, N3, NW, RB); ALL_KERNELS lists the twelve instantiations.  The compute-unit count is 256 here and the device's on the
GPU; only the fill condition of the 32-row workgroups, nets * ceil(M / 32) >= 3 CUs / 4, depends on it.  What
tests/redq_edge_cases.py already restates of the same file (lds4_bytes, LDS4_LAST_K1, part_floats, HP, ROWS) is imported from there.

Cases.  Every case names the instantiation it means to hit; tests/test_mlp3_edge_inputs_cpu.py checks that it takes it.  `nw` / `rb`
are the arguments of ts_mlp3_set_variant.  Groups: rows (M around one, two and three 16-row tiles; the three M around the fill
threshold of the 32-row workgroups and the largest M below it), width (K1 = 32 .. 1024 in steps of 32 on four and on eight waves),
nets (1, 2, 3, 4, 5, 8 networks, shared and per-network input rows), variant (automatic and every forced combination, one and
several networks), dx (input-gradient ranges of 1 .. 8 tiles with unaligned first columns, on four and eight waves).

Inputs.  Seeded torch.Generator on the CPU: weights N(0, 1 / K), biases N(0, 0.5^2) (nonzero), x and d_out dense N(0, 1) -- d_out
over all N3 columns, so every column of W3^T meets a nonzero operand.  d relu / dx jumps at 0: a pre-activation whose SIGN float32
rounding decides has no reference value for anything downstream, so batch rows that hold a layer-1 or layer-2 pre-activation with
|pre| < 32 eps32 (sum_k |x_k w_kj| + |b_j|) in float64 are redrawn, never dropped (the rule of redq_edge_cases.near_kink_rows).
The backward pass takes h1 / h2 as inputs: the float64 reference activations rounded to float32, so the mask (h > 0) is exact on
what the kernel is given.

References.  Plain float64: h1 = relu(x W1 + b1), h2 = relu(h1 W2 + b2), out = h2 W3 + b3; dh2 = (d_out W3^T)(h2 > 0),
dh1 = (dh2 W2^T)(h1 > 0), dx = dh1 W1^T (all K1 columns; the tests take the ones they need).  Never autograd of an engine output.

Bar.  Per tensor and per network rel_bar(e_ref) = max(1e-5, 2 e_ref) of the tensor's largest reference entry, e_ref being torch's own
float32 evaluation of the same formulas against float64 on the same input -- computed from the reference alone (rel_bar is
redq_edge_cases.rel_bar, the project's rule).  tests/test_mlp3_edge_inputs_cpu.py asserts e_ref < 1e-3 for every case.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from tests.conv_edge_cases import rel_err  # noqa: F401  (torch tensors, relative to the largest reference entry)
from tests.redq_edge_cases import (HP, K1_MAX, K1_MIN, K1_STEP, KINK_MARGIN, LDS4_LAST_K1, LDS4_MAX, MULTI_MAX, ROWS,  # noqa: F401
                                   lds4_bytes, part_floats, rel_bar)

# ---- constants that decide the routes (M = tianshou_amd/csrc/ts_mlp.hip) ------------------------------------------------------------------
HID = 256                        # M:45        hidden width; mlp3_supported (:407) wants hidden == HID
NST = 8                          # M:47        register stages of the weight ring
HEADS = (32, 64)                 # M:407       head_cols == 32 || head_cols == 64
LDS_MAX = 160 * 1024             # M:435, :473 dynamic LDS a kernel may ask for; lds32 <= 160 KB for the 32-row forward
ROWS2 = 32                       # M:468, :526 rows of a 32-row workgroup
DX_MAX_TILES = 8                 # M:519       dx_nt <= 8
CPU_CUS = 256                    # M:429       compute units assumed without a device
VARIANTS = ((0, 0), (4, 0), (8, 0), (0, 2))       # (nw, rb) of ts_mlp3_set_variant: automatic and every forced combination
TS_ERR_INVALID_ARG, TS_ERR_UNSUPPORTED = -1, -4   # include/tsengine.h

ALL_KERNELS = frozenset((d, n3, nw, rb) for d in ("fwd", "bwd") for n3 in HEADS for nw, rb in ((4, 1), (8, 1), (8, 2)))


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def supported(K1: int, head: int) -> bool:
    """mlp3_supported, M:407."""
    return head in HEADS and K1 % K1_STEP == 0 and K1_MIN <= K1 <= K1_MAX


def lds8_bytes(K1: int) -> int:
    """M:476, the eight-wave 16-row forward."""
    return 4 * (ROWS * (K1 + 4) + 2 * ROWS * HP + part_floats(8, ROWS))


def lds32_bytes(K1: int) -> int:
    """M:468: the second activation overlays the input rows, whichever is larger."""
    return 4 * (max(ROWS2 * (K1 + 4), ROWS2 * HP) + ROWS2 * HP + part_floats(8, ROWS2))


LDS32_LAST_K1 = max(k for k in range(K1_MIN, K1_MAX + 1, K1_STEP) if lds32_bytes(k) <= LDS_MAX)      # 448


def fills(nets: int, M: int, cus: int) -> bool:
    """M:472, :524: 32-row workgroups only while they still cover 3/4 of the CUs."""
    return nets * ceil_div(M, ROWS2) >= 3 * cus // 4


def variant_of(direction: str, nets: int, M: int, K1: int, nw: int, rb: int, cus: int = CPU_CUS):
    """-> (NW, RB) of the launch: `two` and `four` of mlp3_forward_nx (M:472-475) / mlp3_backward_n (M:524-525)."""
    if direction == "fwd":
        two = rb == 2 and nets > 1 and fills(nets, M, cus) and lds32_bytes(K1) <= LDS_MAX and not nw
        four = (nw == 4) if nw else (nets > 1 and lds4_bytes(K1) <= LDS4_MAX)
    else:
        two = rb == 2 and nets > 1 and fills(nets, M, cus) and not nw
        four = (nw == 4) if nw else nets > 1
    return (8, 2) if two else ((4, 1) if four else (8, 1))


def lds_bytes(direction: str, head: int, K1: int, NW: int, RB: int) -> int:
    """M:476 / M:527."""
    if direction == "fwd":
        return lds32_bytes(K1) if RB == 2 else (lds4_bytes(K1) if NW == 4 else lds8_bytes(K1))
    rows = ROWS * RB
    return 4 * (rows * (head + 4) + 2 * rows * HP + part_floats(NW, rows))


def grid_of(nets: int, M: int, RB: int):
    """M:477 / M:528: (row tiles, networks)."""
    return ceil_div(M, ROWS * RB), nets


def dx_tiles(col0: int, col1: int):
    """M:517-518 -> (dx_c0, dx_nt): the 16-column tiles covering [col0, col1)."""
    c0 = col0 // 16 * 16
    return c0, ceil_div(col1 - c0, 16)


def stream(K: int, ncols: int, tpw: int, NW: int) -> dict:
    """WStream (M:97-102) and the ring of mlp_layer (M:207, :215) for one layer: column blocks, k splits, 16-deep blocks per wave,
    full trips of the NST-stage ring and the tail after them; `dup` = clamped duplicate tiles of a transposed layer (M:105)."""
    per = 16 * tpw
    want = ceil_div(ncols, per)
    ncw = 1 if want <= 1 else (2 if want == 2 else 4)
    nks = NW // ncw
    nbw = K // 16 // nks if ncols > 0 else 0
    assert ncols == 0 or (K // 16) % nks == 0
    return dict(ncw=ncw, nks=nks, nbw=nbw, trips=nbw // NST, tail=nbw % NST, dup=(4 * ncw - ncols // 16) if ncols else 0)


def layer_streams(direction: str, head: int, K1: int, NW: int, dx_nt: int = 0) -> list:
    """The three weight streams of a kernel in launch order (M:321-323 forward, M:369-371 backward)."""
    if direction == "fwd":
        return [stream(K1, HID, 4, NW), stream(HID, HID, 4, NW), stream(HID, head, 2 if head == 32 else 4, NW)]
    return [stream(head, HID, 4, NW), stream(HID, HID, 4, NW), stream(HID, 16 * dx_nt, 4, NW)]


def part_fits(direction: str, head: int, K1: int, NW: int, RB: int, dx_nt: int = 0) -> bool:
    """Every layer's partial sums (nks x rows x (columns of its column blocks + 4), M:157-158, :222) inside part_floats (M:49)."""
    rows = ROWS * RB
    tpws = ((4, 4, 2 if head == 32 else 4) if direction == "fwd" else (4, 4, 4))
    return all(s["nks"] * rows * (16 * t * s["ncw"] + 4) <= part_floats(NW, rows)
               for s, t in zip(layer_streams(direction, head, K1, NW, dx_nt), tpws))


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str                # rows / width / nets / variant / dx
    direction: str            # fwd / bwd
    nets: int
    M: int
    K1: int
    head: int
    nw: int                   # ts_mlp3_set_variant
    rb: int
    own_x: bool               # every network on its own input rows (the _nx form) or all on the same
    cols: tuple | None        # backward: (col0, col1) of dx, None = no input gradient
    meant: tuple              # (direction, N3, NW, RB)

    @property
    def input_key(self):
        """What the inputs and the reference depend on: cases that differ in variant, direction or columns share both."""
        return self.nets, self.M, self.K1, self.head, self.own_x

    def kernel(self, cus: int = CPU_CUS):
        return (self.direction, self.head) + variant_of(self.direction, self.nets, self.M, self.K1, self.nw, self.rb, cus)

    @property
    def ragged(self) -> bool:
        return self.M % (ROWS * self.meant[3]) != 0


def rb2_rows(nets: int, cus: int = CPU_CUS) -> dict:
    """The row counts around the fill threshold of the 32-row workgroups for `nets` networks."""
    tiles = ceil_div(3 * cus // 4, nets)
    return dict(one_row_last_tile=ROWS2 * (tiles - 1) + 1, full=ROWS2 * tiles, one_more=ROWS2 * tiles + 1, fails=ROWS2 * (tiles - 1))


ROW_EDGES = (1, 15, 16, 17, 31, 32, 33, 47)
NETS = (1, 2, 3, 4, 5, 8)
# (col0, col1, K1): dx_nt = 1 .. 8, each with a first column that is no multiple of 16 (and the aligned ones the issue names)
DX_RANGES = [(0, 1, 160), (15, 17, 160), (17, 23, 160), (159, 160, 160), (0, 64, 160), (0, 65, 160), (3, 128, 160), (376, 393, 416),
             (896, 1024, 1024), (5, 40, 160), (33, 90, 160), (7, 80, 160), (19, 100, 160), (35, 140, 160), (901, 1024, 1024)]


def _case(name, group, direction, nets, M, K1, head, nw, rb, own_x, cols, cus):
    meant = (direction, head) + variant_of(direction, nets, M, K1, nw, rb, cus)
    return Case(name, group, direction, nets, M, K1, head, nw, rb, own_x, cols if direction == "bwd" else None, meant)


def cases(cus: int = CPU_CUS) -> list:
    out = []
    # rows: one network on the eight-wave kernel (head 32), two on the four-wave kernel (head 64)
    for direction in ("fwd", "bwd"):
        for nets, head in ((1, 32), (2, 64)):
            for M in ROW_EDGES:
                out.append(_case(f"rows {direction} nets {nets} M {M}", "rows", direction, nets, M, 64, head, 0, 0, True, (30, 33), cus))
    # rows of the 32-row workgroups, eight networks: a one-row last tile, a full one, one more row; below the threshold the launch
    # falls back to the 16-row four-wave kernel (`meant` names it)
    r = rb2_rows(8, cus)
    for direction in ("fwd", "bwd"):
        for head in HEADS:
            for tag, M in r.items():
                out.append(_case(f"rb2 {direction} head {head} {tag} M {M}", "rows", direction, 8, M, 160, head, 0, 2, head == 64, (3, 128), cus))
    # the widest input the 32-row forward takes (the input tile is the larger part of the overlaid region) and the first it does not
    for K1 in (LDS32_LAST_K1, LDS32_LAST_K1 + K1_STEP):
        out.append(_case(f"rb2 fwd K1 {K1}", "rows", "fwd", 8, r["one_row_last_tile"], K1, 32, 0, 2, False, None, cus))
    # networks: each with its own weights; on shared and on per-network input rows
    for nets in NETS:
        for own in (False, True):
            out.append(_case(f"nets {nets} fwd {'own' if own else 'shared'} x", "nets", "fwd", nets, 33, 96, 32 if own else 64, 0, 0, own, None, cus))
        out.append(_case(f"nets {nets} bwd", "nets", "bwd", nets, 33, 96, 64 if nets % 2 else 32, 0, 0, True, (17, 90), cus))
    # the automatic boundary between the four-wave and the eight-wave forward for several networks
    for K1 in (LDS4_LAST_K1, LDS4_LAST_K1 + K1_STEP):
        for head in HEADS:
            out.append(_case(f"auto nets 2 fwd K1 {K1} head {head}", "variant", "fwd", 2, 17, K1, head, 0, 0, True, None, cus))
    # variants: automatic and every forced combination, one network and three, both heads, M = 33 (a ragged last tile)
    for direction in ("fwd", "bwd"):
        for head in HEADS:
            for nw, rb in VARIANTS:
                for nets in (1, 3):
                    out.append(_case(f"variant {direction} head {head} nw {nw} rb {rb} nets {nets}", "variant", direction, nets, 33, 96, head,
                                     nw, rb, True, (0, 65), cus))
    # input-gradient ranges on four and eight waves, one network and two
    for i, (c0, c1, K1) in enumerate(DX_RANGES):
        for nw in (4, 8):
            for nets in (1, 2):
                out.append(_case(f"dx [{c0}, {c1}) of {K1} nw {nw} nets {nets}", "dx", "bwd", nets, 17, K1, HEADS[(i + nets) % 2], nw, 0, True,
                                 (c0, c1), cus))
    assert len({c.name for c in out}) == len(out)
    return out


def case_by_name(name: str, cus: int = CPU_CUS) -> Case:
    return next(c for c in cases(cus) if c.name == name)


SWEEP_K1 = tuple(range(K1_MIN, K1_MAX + 1, K1_STEP))
SWEEP_M = 17
SWEEP_COMBOS = [(d, head, nw) for d in ("fwd", "bwd") for head in HEADS for nw in (4, 8)]


def sweep_case(direction: str, head: int, nw: int, K1: int) -> Case:
    """One launch of the width sweep: a single network, nw forced, M = 17; backward: the last three tiles of the input."""
    cols = (max(K1 - 41, 0), K1)
    return _case(f"width {direction} head {head} nw {nw} K1 {K1}", "width", direction, 1, SWEEP_M, K1, head, nw, 0, True, cols, CPU_CUS)


def sweep_cases() -> list:
    return [sweep_case(d, head, nw, K1) for d, head, nw in SWEEP_COMBOS for K1 in SWEEP_K1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
# (name, direction, overrides of BASE, code, a piece of the ts_last_error sentence); `dx` = which networks get a dx pointer,
# `null` = (array name, network) of one NULL entry
BASE = dict(nets=2, M=17, K1=64, head=32, cols=(3, 20), dx=(True, True), null=None)
REFUSALS = [(f"K1 {k}", d, dict(K1=k), TS_ERR_UNSUPPORTED, "unsupported shape") for k in (0, 16, 48, 1056) for d in ("fwd", "bwd")] \
    + [(f"head {h}", d, dict(head=h), TS_ERR_UNSUPPORTED, "unsupported shape") for h in (16, 96, 128) for d in ("fwd", "bwd")] \
    + [(f"nets {n}", d, dict(nets=n), TS_ERR_INVALID_ARG, "networks") for n in (0, 9) for d in ("fwd", "bwd")] \
    + [("M 0", d, dict(M=0), TS_ERR_INVALID_ARG, "bad argument") for d in ("fwd", "bwd")] \
    + [("col0 == col1", "bwd", dict(cols=(5, 5)), TS_ERR_INVALID_ARG, "column range"),
       ("col0 > col1", "bwd", dict(cols=(9, 5)), TS_ERR_INVALID_ARG, "column range"),
       ("col1 > K1", "bwd", dict(cols=(60, 65)), TS_ERR_INVALID_ARG, "column range"),
       ("nine tiles [0, 129)", "bwd", dict(K1=160, cols=(0, 129)), TS_ERR_UNSUPPORTED, "wider than 128"),
       ("nine tiles [15, 144)", "bwd", dict(K1=160, cols=(15, 144)), TS_ERR_UNSUPPORTED, "wider than 128"),
       ("dx for network 0 only", "bwd", dict(dx=(True, False)), TS_ERR_INVALID_ARG, "all networks or none"),
       ("dx for network 1 only", "bwd", dict(dx=(False, True)), TS_ERR_INVALID_ARG, "all networks or none"),
       ("NULL x entry", "fwd", dict(null=("x", 1)), TS_ERR_INVALID_ARG, "bad argument"),
       ("NULL wb2 entry", "fwd", dict(null=("wb2", 0)), TS_ERR_INVALID_ARG, "bad argument"),
       ("NULL out entry", "fwd", dict(null=("out", 1)), TS_ERR_INVALID_ARG, "bad argument"),
       ("NULL d_out entry", "bwd", dict(null=("d_out", 1)), TS_ERR_INVALID_ARG, "bad argument"),
       ("NULL h1 entry", "bwd", dict(null=("h1", 0)), TS_ERR_INVALID_ARG, "bad argument"),
       ("NULL dh2 entry", "bwd", dict(null=("dh2", 1)), TS_ERR_INVALID_ARG, "bad argument")]


def refusal_args(overrides: dict) -> dict:
    return {**BASE, **overrides}


def refusal_code(direction: str, a: dict):
    """The checks of mlp3_forward_nx (M:450-456) / mlp3_backward_n (M:501-519) in their order -> error code or None."""
    if not supported(a["K1"], a["head"]):
        return TS_ERR_UNSUPPORTED
    if not 1 <= a["nets"] <= MULTI_MAX or a["M"] < 1:
        return TS_ERR_INVALID_ARG
    required = ("x", "wb1", "wb2", "wb3", "out") if direction == "fwd" else ("d_out", "wb1", "wb2", "wb3", "h1", "h2", "dh1", "dh2")
    if a["null"] is not None and a["null"][0] in required and a["null"][1] < a["nets"]:
        return TS_ERR_INVALID_ARG
    if direction == "bwd" and any(a["dx"][:a["nets"]]):
        if not all(a["dx"][:a["nets"]]):
            return TS_ERR_INVALID_ARG
        col0, col1 = a["cols"]
        if not 0 <= col0 < col1 <= a["K1"]:
            return TS_ERR_INVALID_ARG
        if dx_tiles(col0, col1)[1] > DX_MAX_TILES:
            return TS_ERR_UNSUPPORTED
    return None


# ---- inputs and references -----------------------------------------------------------------------------------------------------------------
MAX_REDRAWS = 200


def _wb(K: int, N: int, g: torch.Generator) -> torch.Tensor:
    """[K + 1, N]: weights N(0, 1 / K), last row the bias N(0, 0.5^2)."""
    return torch.cat([torch.randn(K, N, generator=g) / K ** 0.5, 0.5 * torch.randn(1, N, generator=g)]).contiguous()


def near_kink_rows(x: torch.Tensor, wb1: torch.Tensor, wb2: torch.Tensor) -> torch.Tensor:
    """bool[M]: rows with a layer-1 or layer-2 pre-activation whose sign float32 rounding may decide (float64, reference only)."""
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    h = x.double()
    for wb in (wb1, wb2):
        w, b = wb[:-1].double(), wb[-1].double()
        pre = h @ w + b
        bad |= (pre.abs() < KINK_MARGIN * (h.abs() @ w.abs() + b.abs())).any(dim=1)
        h = torch.relu(pre)
    return bad


def seed_of(key: tuple) -> int:
    nets, M, K1, head, own_x = key
    return 77_000_000 + ((nets * 4099 + M) * 1031 + K1) * 4 + (head == 64) * 2 + int(own_x)


@functools.lru_cache(maxsize=None)
def inputs_for(key: tuple) -> dict:
    """Lists over the networks: wb1, wb2, wb3, x (the same tensor object `nets` times unless own_x), d_out; `redraws` = passes of
    the off-the-kink loop that redrew a row."""
    nets, M, K1, head, own_x = key
    g = torch.Generator().manual_seed(seed_of(key))
    wb1 = [_wb(K1, HID, g) for _ in range(nets)]
    wb2 = [_wb(HID, HID, g) for _ in range(nets)]
    wb3 = [_wb(HID, head, g) for _ in range(nets)]
    xs = [torch.randn(M, K1, generator=g) for _ in range(nets if own_x else 1)]
    d_out = [torch.randn(M, head, generator=g) for _ in range(nets)]
    redraws = 0
    for _ in range(MAX_REDRAWS + 1):
        clean = True
        for i, x in enumerate(xs):
            bad = torch.zeros(M, dtype=torch.bool)
            for k in (range(nets) if not own_x else (i,)):
                bad |= near_kink_rows(x, wb1[k], wb2[k])
            n = int(bad.sum())
            if n:
                x[bad] = torch.randn(n, K1, generator=g)
                clean = False
        if clean:
            break
        redraws += 1
    else:
        raise AssertionError("no batch off the ReLU kink found")
    x = xs if own_x else xs * nets
    return dict(wb1=wb1, wb2=wb2, wb3=wb3, x=x, d_out=d_out, redraws=redraws)


def _chain(x, wb1, wb2, wb3, d_out, dtype, h1_in=None, h2_in=None) -> dict:
    """The formulas of the module docstring in `dtype`.  The backward half takes the activations the kernel is given (h1_in / h2_in:
    the float64 ones rounded to float32) for its masks."""
    x, d_out = x.to(dtype), d_out.to(dtype)
    w1, b1, w2, b2, w3, b3 = (t.to(dtype) for wb in (wb1, wb2, wb3) for t in (wb[:-1], wb[-1]))
    h1 = torch.relu(x @ w1 + b1)
    h2 = torch.relu(h1 @ w2 + b2)
    out = h2 @ w3 + b3
    m1 = (h1 if h1_in is None else h1_in) > 0
    m2 = (h2 if h2_in is None else h2_in) > 0
    dh2 = (d_out @ w3.t()) * m2
    dh1 = (dh2 @ w2.t()) * m1
    dx = dh1 @ w1.t()
    return dict(h1=h1, h2=h2, out=out, dh2=dh2, dh1=dh1, dx=dx)


TENSORS = {"fwd": ("h1", "h2", "out"), "bwd": ("dh2", "dh1", "dx")}


@functools.lru_cache(maxsize=None)
def reference_for(key: tuple) -> dict:
    """-> ref64 / ref32: lists over the networks of the dicts of `_chain`; h1 / h2: the float32 activations the backward pass is given."""
    inp = inputs_for(key)
    ref64, ref32, h1, h2 = [], [], [], []
    for k in range(key[0]):
        args = (inp["x"][k], inp["wb1"][k], inp["wb2"][k], inp["wb3"][k], inp["d_out"][k])
        r = _chain(*args, torch.float64)
        a1, a2 = r["h1"].float().contiguous(), r["h2"].float().contiguous()
        assert bool(((a1 > 0) == (r["h1"] > 0)).all()) and bool(((a2 > 0) == (r["h2"] > 0)).all())       # rounding keeps the masks
        ref64.append(r)
        ref32.append(_chain(*args, torch.float32, a1, a2))
        h1.append(a1)
        h2.append(a2)
    return dict(ref64=ref64, ref32=ref32, h1=h1, h2=h2)


def hull(c: Case):
    """Columns of dx the kernel writes: [floor16(col0), ceil16(col1))."""
    c0, nt = dx_tiles(*c.cols)
    return c0, c0 + 16 * nt


def expected(c: Case, k: int, name: str):
    """-> (float64 reference, e_ref) of tensor `name` of network k for this case (dx: the written hull of columns)."""
    ref = reference_for(c.input_key)
    r64, r32 = ref["ref64"][k][name], ref["ref32"][k][name]
    if name == "dx":
        lo, hi = hull(c)
        r64, r32 = r64[:, lo:hi], r32[:, lo:hi]
    return r64, rel_err(r32, r64)


def worst_e_ref(c: Case) -> float:
    names = [n for n in TENSORS[c.direction] if n != "dx" or c.cols is not None]
    return max(expected(c, k, n)[1] for k in range(c.nets) for n in names)


def describe(c: Case, cus: int = CPU_CUS) -> str:
    d, n3, NW, RB = c.kernel(cus)
    nt = dx_tiles(*c.cols)[1] if c.cols else 0
    ls = layer_streams(d, n3, c.K1, NW, nt)
    rings = ", ".join(f"{s['ncw']}x{s['nks']} nbw {s['nbw']} = {s['trips']} trips + {s['tail']}" for s in ls)
    return (f"{c.name}: mlp3_{d}_kernel<{n3}, {NW}, {RB}> grid {grid_of(c.nets, c.M, RB)} lds {lds_bytes(d, n3, c.K1, NW, RB)} B; "
            f"layers (column blocks x k splits, ring): {rings}" + (f"; dx tiles {dx_tiles(*c.cols)}" if c.cols else ""))
