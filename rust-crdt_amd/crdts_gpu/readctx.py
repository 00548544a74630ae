"""`ReadCtx` and the contexts derived from it (reference: src/ctx.rs:8-55), batched and dense.

Every read of the reference returns `ReadCtx { add_clock, rm_clock, val }`; `derive_add_ctx` /
`derive_rm_ctx` are the only supported way to build the next Op.  Here the clocks are device
tensors of dense rows, one per state or query, and `val` is what the read computed:

    orswot.read      val = (members (N, Mw) int64 bitmap, len (N,) int32)
    orswot.contains  val = (Q,) uint8
    mvreg.read       val = (vals (N, V) int64 compacted in Vec order, nval (N,) int32)
    map.read         val = (keys (N, Kw) int64 bitmap, len (N,) int32)
    map.get          val = MapGetVal(present, vclk, vval, nval, val_clock)
    map.counter_get / orswot_get / nested_get      val = MapCounterGetVal / MapOrswotGetVal / MapNestedGetVal
    map.orswot_contains / nested_get_inner         the nested value's own ReadCtx (val (Q,) uint8 / MapGetVal)
    map.counter_read / orswot_read / nested_read   val = keys, len and every key's total / members / inner keys

so read -> derive ctx -> op -> apply_batch stays on the device (include/crdt_gpu.h "batched
ReadCtx queries").  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Any, NamedTuple, Optional

import torch

from .context import Context, U64_DTYPES, dptr

U32_DTYPES = (torch.int32, torch.uint32)


class ReadCtx(NamedTuple):  # ctx.rs:12-21
    add_clock: torch.Tensor  # (..., A)
    rm_clock: torch.Tensor   # (..., A)
    val: Any


class AddCtx(NamedTuple):  # ctx.rs:24-31
    clock: torch.Tensor    # (Q, A): add_clock with the dot applied
    actor: torch.Tensor    # (Q,) int32: dot.actor
    counter: torch.Tensor  # (Q,) int64: dot.counter (u64 bits)
    status: torch.Tensor   # (Q,) int32: bit 1 = actor out of range, bit 2 = counter overflow


class RmCtx(NamedTuple):  # ctx.rs:34-38
    clock: torch.Tensor  # (Q, A)


def check_args(what: str, rows=(), index=()) -> None:
    """Argument checks shared by the read wrappers, all ValueError and all before any library call:
    `rows` are (tensor, name) of u64 rows (int64 / uint64, innermost axis contiguous), `index` are
    (Q,) int32 query vectors (state indices, members, keys, actors).  dtypes and layouts of every
    argument first, then the device."""
    for group, dtypes in ((rows, U64_DTYPES), (index, U32_DTYPES)):
        for t, nm in group:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}({nm}): expected a torch.Tensor")
            if t.dtype not in dtypes:
                raise ValueError(f"{what}({nm}): dtype {t.dtype}; expected one of {dtypes}")
            if t.dim() > 0 and t.shape[-1] > 1 and t.stride(-1) != 1:
                raise ValueError(f"{what}({nm}): the innermost axis must be contiguous (stride {t.stride(-1)})")
    for t, nm in index:
        if t.dim() != 1:
            raise ValueError(f"{what}({nm}): expected a (Q,) int32 tensor")
    for t, nm in tuple(rows) + tuple(index):
        if t.device.type != "cuda":
            raise ValueError(f"{what}({nm}): tensor on {t.device}; expected a cuda tensor")


def gather_rows(ctx: Context, rows: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """rows[idx[q]] as (Q, A), zeros where idx[q] is out of range, without a host sync: the
    contains gather over `rows` seen as N one-member states."""
    N, A = rows.shape
    Q = idx.shape[0]
    out = torch.empty((Q, A), dtype=rows.dtype, device=rows.device)
    if Q:
        zero = torch.zeros(Q, dtype=torch.int32, device=rows.device)
        val = torch.empty(Q, dtype=torch.uint8, device=rows.device)
        st = torch.empty(Q, dtype=torch.int32, device=rows.device)
        ctx.call("crdt_orswot_contains", dptr(rows), A, rows.stride(0) if N > 1 else A, N, 1, A, dptr(idx),
                 dptr(zero), Q, dptr(val), dptr(out), A, dptr(st))
    return out


def derive_add_ctx(rc: ReadCtx, actor, ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None) -> AddCtx:
    """ReadCtx::derive_add_ctx (ctx.rs:42-48) of every row of rc.add_clock ((Q, A) or (A,)):
    dot = add_clock.inc(actor); clock = add_clock with the dot applied.  `actor` is a (Q,) int32
    device tensor or one int for every row.  `out` may be rc.add_clock itself (in place)."""
    clock = rc.add_clock
    scalar = isinstance(actor, int)
    check_args("derive_add_ctx", [(clock, "add_clock")] + ([] if out is None else [(out, "out")]),
               [] if scalar else [(actor, "actor")])
    c = clock.unsqueeze(0) if clock.dim() == 1 else clock
    if c.dim() != 2:
        raise ValueError("derive_add_ctx: add_clock (Q, A) or (A,) expected")
    Q, A = c.shape
    if scalar:
        actor = torch.full((Q,), actor, dtype=torch.int32, device=c.device)
    if actor.shape[0] != Q:
        raise ValueError(f"derive_add_ctx: actor has {actor.shape[0]} entries, add_clock {Q} rows")
    if out is None:
        o = torch.empty((Q, A), dtype=c.dtype, device=c.device)
    else:
        o = out.unsqueeze(0) if out.dim() == 1 else out
        if tuple(o.shape) != (Q, A) or o.dtype != c.dtype:
            raise ValueError(f"derive_add_ctx: out {tuple(out.shape)} does not match add_clock {tuple(clock.shape)}")
        if o.data_ptr() == c.data_ptr() and Q > 1 and o.stride(0) != c.stride(0):
            raise ValueError("derive_add_ctx: out aliases add_clock with another row stride")
    ctx = ctx or Context.default(c.device.index)
    ctx.check_tensor(c, "derive_add_ctx(add_clock)")
    ctx.check_tensor(o, "derive_add_ctx(out)")
    ctx.check_tensor(actor, "derive_add_ctx(actor)", U32_DTYPES)
    counter = torch.empty(Q, dtype=torch.int64, device=c.device)
    status = torch.empty(Q, dtype=torch.int32, device=c.device)
    ctx.call("crdt_vclock_derive_add", dptr(c), c.stride(0) if Q > 1 else A, Q, A, dptr(actor), dptr(o),
             o.stride(0) if Q > 1 else A, dptr(counter), dptr(status))
    return AddCtx(o[0] if clock.dim() == 1 else o, actor, counter, status)


def derive_rm_ctx(rc: ReadCtx) -> RmCtx:
    """ReadCtx::derive_rm_ctx (ctx.rs:50-54): the rm_clock rows (no kernel; apply_batch copies
    nothing out of them either: an op batch's rm_clock / clk_pool can be this tensor)."""
    return RmCtx(rc.rm_clock)
