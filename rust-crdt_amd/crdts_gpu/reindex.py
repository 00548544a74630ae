"""Re-index resident dense states on the device when a dictionary or a capacity grows
(include/crdt_gpu.h, "re-index resident states"; csrc/reindex.hip).

An axis map is an (n_out,) int32 device tensor `src`: output index j takes the data of input index
src[j]; a value outside [0, n_in) (index_map writes -1, the u32 0xFFFFFFFF) means nobody: zeros.
`None` is the identity on min(n_in, n_out) indices, the pure capacity change.

    index_map(old_ids, new_ids) -> (src, n_lost)   positions of new_ids in old_ids, no synchronisation
    rows(x, src, width, planes=1)                  (N, planes * A_in) rows -> (N, planes * width)
    bitmaps(x, src, bits)                          (N, W_in) bitmap rows -> (N, ceil(bits / 64))

The per-type forms are orswot.reindex, map.reindex, mvreg.reindex, vclock / gcounter / pncounter /
gset.reindex.  Each returns its output with a status (N,) int32 tensor of REINDEX_* bits.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _abi
from .context import Context, dptr

U32_DTYPES = (torch.int32, torch.uint32)


def src_ptr(ctx: Context, src: Optional[torch.Tensor], what: str) -> Tuple[ctypes.c_void_p, Optional[int]]:
    """(device pointer or NULL, length or None) of an axis map."""
    if src is None:
        return ctypes.c_void_p(None), None
    ctx.check_tensor(src, what, dtypes=U32_DTYPES)
    if src.dim() != 1 or not src.is_contiguous():
        raise ValueError(f"{what}: an axis map is a contiguous (n_out,) int32 tensor")
    return dptr(src), src.shape[0]


def out_size(given: Optional[int], n_map: Optional[int], n_in: int, what: str) -> int:
    """A missing size is the map's length, or the input's size without a map."""
    n = given if given is not None else (n_map if n_map is not None else n_in)
    if n_map is not None and n > n_map:
        raise ValueError(f"{what}: size {n} past the map's {n_map} entries")
    return int(n)


def index_map(old_ids: torch.Tensor, new_ids: torch.Tensor, ctx: Optional[Context] = None):
    """src[j] = position of new_ids[j] in old_ids, or -1 when absent; n_lost (1,) int32 = how many old
    ids are absent from new_ids.  Both dictionaries ascending and unique (as u32 / u64), of one dtype:
    int32 / uint32 for u32 ids, int64 / uint64 for u64 ids.  Both results stay on the device."""
    ctx = ctx or Context.default(new_ids.device.index)
    wide = new_ids.dtype in (torch.int64, torch.uint64)
    dt = (torch.int64, torch.uint64) if wide else U32_DTYPES
    for t, nm in ((old_ids, "old_ids"), (new_ids, "new_ids")):
        ctx.check_tensor(t, f"reindex.index_map({nm})", dtypes=dt)
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"reindex.index_map({nm}): a contiguous 1-D dictionary expected")
    src = torch.empty(new_ids.shape[0], dtype=torch.int32, device=new_ids.device)
    n_lost = torch.empty(1, dtype=torch.int32, device=new_ids.device)
    ctx.call("crdt_reindex_map_u64" if wide else "crdt_reindex_map_u32", dptr(old_ids), old_ids.shape[0], dptr(new_ids),
             new_ids.shape[0], dptr(src), dptr(n_lost))
    return src, n_lost


def _rows2d(ctx, x, what):
    ctx.check_tensor(x, what)
    if x.dim() != 2 or (x.numel() and x.shape[1] > 1 and x.stride(1) != 1):  # an empty tensor's strides are arbitrary
        raise ValueError(f"{what}: (N, W) rows with unit stride along W expected, got {tuple(x.shape)}")


def rows(x: torch.Tensor, src: Optional[torch.Tensor], width: Optional[int] = None, planes: int = 1,
         out: Optional[torch.Tensor] = None, ctx: Optional[Context] = None):
    """Gather the columns of N rows of `planes` x A_in u64 words into rows of planes x `width`
    (planes = 2: PNCounter's P and N halves).  Returns (out, status); status bit REINDEX_DROPPED marks
    a row that held a non-zero counter in a column the map drops."""
    ctx = ctx or Context.default(x.device.index)
    _rows2d(ctx, x, "reindex.rows(x)")
    if planes < 1 or x.shape[1] % planes:
        raise ValueError(f"reindex.rows: {x.shape[1]} words are not {planes} planes")
    N, A_in = x.shape[0], x.shape[1] // planes
    sp, n_map = src_ptr(ctx, src, "reindex.rows(src)")
    A_out = out_size(width, n_map, A_in, "reindex.rows")
    if out is None:
        out = torch.empty((N, planes * A_out), dtype=x.dtype, device=x.device)
    _rows2d(ctx, out, "reindex.rows(out)")
    if tuple(out.shape) != (N, planes * A_out):
        raise ValueError(f"reindex.rows: out {tuple(out.shape)}, expected {(N, planes * A_out)}")
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    ctx.call("crdt_rows_reindex", dptr(x), x.stride(0), A_in, dptr(out), out.stride(0), A_out, planes, N, sp, dptr(status))
    return out, status


def bitmaps(x: torch.Tensor, src: Optional[torch.Tensor], bits: Optional[int] = None, out: Optional[torch.Tensor] = None,
            ctx: Optional[Context] = None, bits_in: Optional[int] = None):
    """Gather N bitmap rows bit by bit: output bit j is input bit src[j].  `bits` is the output universe
    (default: the map's length), `bits_in` the input's (default: every bit of the input's words).
    Returns (out, status); bits past `bits` in the last output word are 0."""
    ctx = ctx or Context.default(x.device.index)
    _rows2d(ctx, x, "reindex.bitmaps(x)")
    N = x.shape[0]
    U_in = int(bits_in) if bits_in is not None else x.shape[1] * 64
    if U_in > x.shape[1] * 64:
        raise ValueError(f"reindex.bitmaps: bits_in = {U_in} past the rows' {x.shape[1]} words")
    sp, n_map = src_ptr(ctx, src, "reindex.bitmaps(src)")
    U_out = out_size(bits, n_map, U_in, "reindex.bitmaps")
    W_out = (U_out + 63) // 64
    if out is None:
        out = torch.empty((N, W_out), dtype=x.dtype, device=x.device)
    _rows2d(ctx, out, "reindex.bitmaps(out)")
    if tuple(out.shape) != (N, W_out):
        raise ValueError(f"reindex.bitmaps: out {tuple(out.shape)}, expected {(N, W_out)}")
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    ctx.call("crdt_bitmap_reindex", dptr(x), x.stride(0), U_in, dptr(out), out.stride(0), U_out, N, sp, dptr(status))
    return out, status
