"""The fused three-layer MLP kernels (tianshou_amd/csrc/ts_mlp.hip) as layer-level calls: ts_mlp3_forward / ts_mlp3_backward /
ts_mlp3_set_variant of include/tsengine.h.  Marshalling only: the caller owns every tensor, outputs included (so tests can
hand in sentinel-filled buffers with spare rows); lists hold one device tensor per network."""
from __future__ import annotations

import contextlib
import ctypes as C

from . import _lib


def _ptrs(tensors):
    """Host array of device pointers (None -> NULL array; a None entry -> NULL entry)."""
    if tensors is None:
        return None
    return (C.c_void_p * max(len(tensors), 1))(*[_lib.ptr(t).value for t in tensors])


def _device(tensors):
    return next((t.device for t in tensors or () if t is not None), None)


def forward(x, wb1, wb2, wb3, h1, h2, out, M: int, K1: int, head_cols: int, nets: int | None = None) -> None:
    """out[k][:M] = head(relu(relu(x[k] W1 + b1) W2 + b2)); h1 / h2 lists or None (inference-only chain)."""
    n = len(out) if nets is None else nets
    _lib.check(_lib.load().ts_mlp3_forward(None, C.c_int(n), _ptrs(x), _ptrs(wb1), _ptrs(wb2), _ptrs(wb3), _ptrs(h1), _ptrs(h2),
                                           _ptrs(out), _lib.i64(M), _lib.i64(K1), _lib.i64(head_cols),
                                           _lib.current_stream(_device(out))))


def backward(d_out, wb1, wb2, wb3, h1, h2, dh1, dh2, dx, M: int, K1: int, head_cols: int, col0: int = 0, col1: int = 0,
             nets: int | None = None) -> None:
    """dh2[k], dh1[k] and (dx a list) dx[k][:, col0:col1) of the chain; dx = None skips the last layer."""
    n = len(dh1) if nets is None else nets
    _lib.check(_lib.load().ts_mlp3_backward(None, C.c_int(n), _ptrs(d_out), _ptrs(wb1), _ptrs(wb2), _ptrs(wb3), _ptrs(h1), _ptrs(h2),
                                            _ptrs(dh1), _ptrs(dh2), _ptrs(dx), _lib.i64(M), _lib.i64(K1), _lib.i64(head_cols),
                                            _lib.i64(col0), _lib.i64(col1), _lib.current_stream(_device(dh1))))


def set_variant(nw: int = 0, rb: int = 0) -> tuple[int, int]:
    """-> the previous (nw, rb).  nw in {0, 4, 8}, rb in {0, 2}; process-wide (include/tsengine.h)."""
    prev = _lib.load().ts_mlp3_set_variant(C.c_int(nw), C.c_int(rb))
    _lib.check(min(prev, 0))
    return divmod(prev, 10)


@contextlib.contextmanager
def variant(nw: int = 0, rb: int = 0):
    """`with variant(4, 0): ...` -- restores the variant it found."""
    prev = set_variant(nw, rb)
    try:
        yield
    finally:
        set_variant(*prev)
