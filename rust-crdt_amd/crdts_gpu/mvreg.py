"""Batched `MVReg<u64, A>` on its own (reference: src/mvreg.rs:112-166; include/crdt_gpu.h "MVReg").

Dense register (the value layout of the Map entry points): slots in Vec order,
    vclk (..., V, A)  value clocks (empty slot <=> all-zero row)
    vval (..., V)     values, u64 ids interned by the caller (merge / apply never compare values)

    lub_many(vclk (G, R, V, A) or (R, V, A), vval)  acc = MVReg::new(); for r: acc.merge(r)  (mvreg.rs:112-128)
    merge_batch(self (N, V, A), other)               self[i].merge(other[i]), in place
    apply_batch(vclk (N, V, A), vval, ops)           reg[i].apply(op) for its ops in order   (mvreg.rs:130-166)
    read(vclk (N, V, A), vval)                       reg[i].read() as a ReadCtx              (mvreg.rs:183-215)
    forget_batch(vclk (N, V, A), vval, y)            reg[i].forget(y or y[i]), in place      (mvreg.rs:88-104)
    eq_batch(x (N, Vx, A), x_vval, y (N, Vy, A), y_vval)  x[i] == y[i], order-free            (mvreg.rs:62-86)
Every call takes registers of up to V = 64 slots.  Past 16 slots merge_batch, apply_batch and lub_many
keep the working register in LDS (about V * A * 8 bytes within 160 KiB: V = 64 reaches A = 314; past
that CrdtGpuError with CRDT_EUNSUPPORTED); forget_batch and eq_batch keep no state and take A <= 1024
at every V.
The wire forms (register frames, Vec<Op::Put> frames) are in wire.py: mvreg_ingest / mvreg_egress /
mvreg_ops_ingest / mvreg_ops_egress.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _abi
from . import readctx as _rc
from .context import Context


class MVRegLub(NamedTuple):
    vclk: torch.Tensor   # (G, Vout, A)
    vval: torch.Tensor   # (G, Vout)
    nval: torch.Tensor   # (G,) int32
    flags: torch.Tensor  # (G,) int32


class MVRegCapacityError(RuntimeError):
    """A register holds more values than the output (or its own) slots."""


def _check_regs(ctx, vclk, vval, what, lead):
    ctx.check_tensor(vclk, f"{what}(vclk)")
    ctx.check_tensor(vval, f"{what}(vval)")
    if vclk.dim() != lead + 2 or vval.dim() != lead + 1 or tuple(vclk.shape[:-1]) != tuple(vval.shape):
        raise ValueError(f"{what}: vclk (..., V, A) and vval (..., V) expected")
    V, A = vclk.shape[-2], vclk.shape[-1]
    if vclk.stride(-1) != 1 or vclk.stride(-2) != A or vval.stride(-1) != 1:
        raise ValueError(f"{what}: each register's slots must be packed")
    return V, A


def lub_many(vclk: torch.Tensor, vval: torch.Tensor, vout: int = 4, ctx: Optional[Context] = None,
             check: bool = True, vstate: int = 0) -> MVRegLub:
    """Left fold of each group's replicas from MVReg::new().  A group needing more than `vout`
    values raises MVRegCapacityError (check=True); a fold state overflow reruns with 16 slots.
    `vstate` = 17..64 asks for the deep pass (registers that overflow 16 values are folded again with
    `vstate` slots); `vout` may then go up to 64 instead of 16.  Input registers of V = 17..64 slots
    (a deep fold's own output, for one) need `vstate` = 17..64: every group then folds in LDS."""
    ctx = ctx or Context.default(vclk.device.index)
    squeeze = vclk.dim() == 3
    vc = vclk.unsqueeze(0) if squeeze else vclk
    vv = vval.unsqueeze(0) if squeeze else vval
    V, A = _check_regs(ctx, vc, vv, "mvreg.lub_many", 2)
    G, R = vc.shape[0], vc.shape[1]
    dev = vclk.device
    out_c = torch.empty((G, vout, A), dtype=torch.int64, device=dev)
    out_v = torch.empty((G, vout), dtype=torch.int64, device=dev)
    nval = torch.empty(G, dtype=torch.int32, device=dev)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    b = _abi.MVRegBatch(G, R, A, V, vc.data_ptr(), vc.stride(1), vc.stride(0), vv.data_ptr(), vv.stride(1),
                        vv.stride(0))
    o = _abi.MVRegOut(vout, vstate, out_c.data_ptr(), out_v.data_ptr(), nval.data_ptr(), flags.data_ptr())
    ctx.call("crdt_mvreg_lub_many", ctypes.byref(b), ctypes.byref(o))
    if check:
        f = int(np.bitwise_or.reduce(flags.cpu().numpy())) if G else 0
        if f & 4 and vstate < 16:
            return lub_many(vclk, vval, vout, ctx, check, vstate=16)
        if f & 4 and vstate > 16:  # the deep pass ran out of its slots too
            raise MVRegCapacityError(f"mvreg.lub_many: a register held more than vstate={vstate} values "
                                     "during the fold (vstate goes up to 64)")
        if f & 4:
            raise MVRegCapacityError("mvreg.lub_many: a register held more than 16 values during the fold "
                                     "(pass vstate=17..64 for the deep pass)")
        if f & 1:
            raise MVRegCapacityError(f"mvreg.lub_many: a register folds to more than vout={vout} values")
    if squeeze:
        return MVRegLub(out_c[0], out_v[0], nval, flags)
    return MVRegLub(out_c, out_v, nval, flags)


def _states(ctx, vclk, vval, what):
    V, A = _check_regs(ctx, vclk, vval, what, 1)
    return _abi.MVRegStates(vclk.shape[0], A, V, vclk.data_ptr(), vclk.stride(0), vval.data_ptr(), vval.stride(0))


def merge_batch(self_vclk: torch.Tensor, self_vval: torch.Tensor, other_vclk: torch.Tensor,
                other_vval: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    """self[i].merge(other[i]) in place on (N, V, A) / (N, V); returns status (N,) int32 (bit 4 =
    more than self's V values: that register is incomplete).  V <= 64 on both sides, which may differ."""
    ctx = ctx or Context.default(self_vclk.device.index)
    a = _states(ctx, self_vclk, self_vval, "mvreg.merge_batch(self)")
    b = _states(ctx, other_vclk, other_vval, "mvreg.merge_batch(other)")
    status = torch.empty(a.N, dtype=torch.int32, device=self_vclk.device)
    ctx.call("crdt_mvreg_merge_batch", ctypes.byref(a), ctypes.byref(b), status.data_ptr())
    return status


def eq_batch(x_vclk: torch.Tensor, x_vval: torch.Tensor, y_vclk: torch.Tensor, y_vval: torch.Tensor,
             ctx: Optional[Context] = None) -> torch.Tensor:
    """x[i] == y[i] by MVReg's PartialEq (mvreg.rs:62-86) on (N, V, A) / (N, V) registers: sets of
    (clock, value) over the non-empty slots, so slot order, holes and V (which may differ between the
    sides) do not matter.  Returns ne (N,) int32: 0 = equal, else NE_VALUES.  Both sides are read only."""
    ctx = ctx or Context.default(x_vclk.device.index)
    a = _states(ctx, x_vclk, x_vval, "mvreg.eq_batch(x)")
    b = _states(ctx, y_vclk, y_vval, "mvreg.eq_batch(y)")
    if (a.N, a.A) != (b.N, b.A):
        raise ValueError("mvreg.eq_batch: x and y differ in N or A")
    ne = torch.empty(a.N, dtype=torch.int32, device=x_vclk.device)
    ctx.call("crdt_mvreg_eq_batch", ctypes.byref(a), ctypes.byref(b), ne.data_ptr())
    return ne


def reindex(vclk: torch.Tensor, vval: torch.Tensor, actors: Optional[torch.Tensor] = None, A: Optional[int] = None,
            V: Optional[int] = None, ctx: Optional[Context] = None):
    """The (N, V, A) / (N, V) registers gathered into another dense layout (crdt_mvreg_reindex): actor
    columns through the axis map `actors` (reindex.index_map builds it; None = the identity prefix),
    `V` value slots (slot v stays slot v, holes included).  A missing size is the map's length, or the
    input's.  Returns ((vclk, vval), status): status (N,) int32 of REINDEX_DROPPED / REINDEX_VALUES."""
    from . import reindex as _rx
    ctx = ctx or Context.default(vclk.device.index)
    a = _states(ctx, vclk, vval, "mvreg.reindex(in)")
    ap, na = _rx.src_ptr(ctx, actors, "mvreg.reindex(actors)")
    A2 = _rx.out_size(A, na, a.A, "mvreg.reindex(A)")
    V2 = a.V if V is None else int(V)
    out_c = torch.empty((a.N, V2, A2), dtype=vclk.dtype, device=vclk.device)
    out_v = torch.empty((a.N, V2), dtype=vval.dtype, device=vclk.device)
    b = _states(ctx, out_c, out_v, "mvreg.reindex(out)")
    status = torch.empty(a.N, dtype=torch.int32, device=vclk.device)
    ctx.call("crdt_mvreg_reindex", ctypes.byref(a), ap, ctypes.byref(b), status.data_ptr())
    return (out_c, out_v), status


class MVRegOpBatch(NamedTuple):
    op_off: torch.Tensor    # (N+1,) int64
    clk_row: torch.Tensor   # (n_ops,) int32
    clk_pool: torch.Tensor  # (n_clk, A) int64
    val: torch.Tensor       # (n_ops,) int64


def encode_ops(streams: Sequence, A: int, device) -> MVRegOpBatch:
    """Per-register streams of Op::Put (mvreg.rs:38-47) as (clock, val): clock a mapping actor ->
    counter or a dense row of A counters, val a u64 id."""
    op_off, clk_row, val, pool = [0], [], [], []
    for ops in streams:
        for clock, v in ops:
            r = np.zeros(A, np.uint64)
            if hasattr(clock, "items"):
                for a, c in clock.items():
                    r[int(a)] = np.uint64(c)
            else:
                r[:] = np.asarray(clock, np.uint64)
            clk_row.append(len(pool))
            pool.append(r)
            val.append(int(v))
        op_off.append(len(val))
    pool.append(np.zeros(A, np.uint64))
    t = lambda x, dt: torch.from_numpy(np.asarray(x, dtype=dt)).to(device)  # noqa: E731
    return MVRegOpBatch(t(op_off, np.int64), t(clk_row or [0], np.int32)[:len(clk_row)],
                        torch.from_numpy(np.stack(pool).view(np.int64)).to(device),
                        torch.from_numpy(np.array(val or [0], np.uint64).view(np.int64)).to(device)[:len(val)])


def apply_batch(vclk: torch.Tensor, vval: torch.Tensor, ops: MVRegOpBatch, ctx: Optional[Context] = None) -> torch.Tensor:
    """Apply every register's op stream in place; returns status (N,) int32 (include/crdt_gpu.h).
    V <= 64."""
    ctx = ctx or Context.default(vclk.device.index)
    st = _states(ctx, vclk, vval, "mvreg.apply_batch")
    n = ops.val.shape[0]
    if ops.op_off.shape[0] != st.N + 1 or ops.clk_row.shape[0] != n or ops.clk_pool.shape[1] != st.A:
        raise ValueError("mvreg.apply_batch: op_off (N+1,), clk_row (n_ops,), clk_pool (n, A)")
    o = _abi.MVRegOps(n, ops.op_off.data_ptr(), ops.clk_row.data_ptr(), ops.clk_pool.data_ptr(),
                      ops.clk_pool.shape[0], ops.val.data_ptr())
    status = torch.empty(st.N, dtype=torch.int32, device=vclk.device)
    ctx.call("crdt_mvreg_apply_batch", ctypes.byref(st), ctypes.byref(o), status.data_ptr())
    return status


def forget_batch(vclk: torch.Tensor, vval: torch.Tensor, y: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    """Causal::forget (mvreg.rs:88-104) in place on (N, V, A) / (N, V): register i forgets y (A,)
    (one clock for all registers) or y[i] of (N, A).  Values whose clock empties are dropped, the
    survivors move to the first slots in order.  Returns status (N,) int32 (no bit defined: 0)."""
    _rc.check_args("mvreg.forget_batch", [(vclk, "vclk"), (vval, "vval"), (y, "y")])
    ctx = ctx or Context.default(vclk.device.index)
    st = _states(ctx, vclk, vval, "mvreg.forget_batch")
    ctx.check_tensor(y, "mvreg.forget_batch(y)")
    if y.dim() == 1 and y.shape[0] == st.A and y.stride(0) == 1:
        ys = 0
    elif y.dim() == 2 and tuple(y.shape) == (st.N, st.A) and y.stride(1) == 1 and (st.N <= 1 or y.stride(0) >= st.A):
        ys = y.stride(0)
    else:
        raise ValueError(f"mvreg.forget_batch: y must be ({st.A},) or ({st.N}, {st.A}) with contiguous rows")
    status = torch.empty(st.N, dtype=torch.int32, device=vclk.device)
    ctx.call("crdt_mvreg_forget_batch", ctypes.byref(st), y.data_ptr(), ys, status.data_ptr())
    return status


def read(vclk: torch.Tensor, vval: torch.Tensor, ctx: Optional[Context] = None) -> "_rc.ReadCtx":
    """MVReg::read (mvreg.rs:183-215) of N registers (vclk (N, V, A), vval (N, V)): ReadCtx(add_clock
    = rm_clock = the join of the non-empty slots' clocks (N, A), val = (vals (N, V) int64: the values
    in Vec order, the rest 0, nval (N,) int32))."""
    _rc.check_args("mvreg.read", [(vclk, "vclk"), (vval, "vval")])
    if vclk.dim() != 3 or vval.dim() != 2 or tuple(vclk.shape[:2]) != tuple(vval.shape):
        raise ValueError("mvreg.read: vclk (N, V, A) and vval (N, V) expected")
    N, V, A = vclk.shape
    if V > 1 and vclk.stride(1) != A:
        raise ValueError("mvreg.read: each register's slots must be packed")
    ctx = ctx or Context.default(vclk.device.index)
    st = _states(ctx, vclk, vval, "mvreg.read")
    clock = torch.empty((N, A), dtype=vclk.dtype, device=vclk.device)
    vals = torch.empty((N, V), dtype=vval.dtype, device=vclk.device)
    nval = torch.empty(N, dtype=torch.int32, device=vclk.device)
    ctx.call("crdt_mvreg_read", ctypes.byref(st), clock.data_ptr(), A, vals.data_ptr(), nval.data_ptr())
    return _rc.ReadCtx(clock, clock, (vals, nval))
