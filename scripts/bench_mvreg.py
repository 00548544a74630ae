"""MVReg on its own on one MI355X: crdt_mvreg_forget_batch and the standalone wire forms.

forget: 1M registers x V = 4 x A = 32 against crdt_map_forget_batch over the same value bytes arranged
as K = 1 Maps (the project's yardstick for a forget stream), same run, same shared y; the registers
are restored before every launch.  Reported: call times by HIP events and the time per byte of the
arrays each call streams (the Map call also reads and writes a clock and an entry clock per state).
wire, states: 1M registers -> crdt_mvreg_egress / crdt_mvreg_ingest.  wire, ops: 65,536 registers x
64 Puts -> crdt_mvreg_ops_egress / crdt_mvreg_ops_ingest, and the crdt_mvreg_apply_batch the
ingest feeds.  Beside each: a pinned host-to-device copy of the same frame bytes.

20 launches after 5 warm-ups each, median [min].  One JSON line per part, printed and appended to
--log (default profiles/mvreg_bench.log)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd"), os.path.join(ROOT, "oracle")]
import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regs", type=int, default=1 << 20)
ap.add_argument("--op-regs", type=int, default=65536)
ap.add_argument("--ops", type=int, default=64)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--vals", type=int, default=4)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=["forget", "states", "ops"], default=None)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mvreg_bench.log"))
args = ap.parse_args()
A, V = args.actors, args.vals

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = "cuda"
LOG = open(args.log, "a")


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def events(fn, before=None):
    """Call times by HIP events -> (median, min) in microseconds."""
    for _ in range(args.warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.launches):
        if before:
            before()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us)


def host_clock(fn):
    for _ in range(args.warmup):
        fn()
    us = []
    for _ in range(args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us), min(us)


def sparse_ids(n, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(1, 1 << 20, (n,), generator=g, device=DEV, dtype=torch.int64).cumsum(0).to(torch.int32)


def registers(N, seed):
    """N registers of V occupied slots, about three dots a value, counters 1..255."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    cnt = torch.randint(1, 256, (N, V, A), generator=g, device=DEV, dtype=torch.int64)
    keep = torch.rand((N, V, A), generator=g, device=DEV) < 3.0 / A
    keep[:, torch.arange(V), torch.arange(V) % A] = True  # no empty slot
    vclk = cnt * keep
    vval = torch.randint(1, 1 << 62, (N, V), generator=g, device=DEV, dtype=torch.int64)
    return vclk, vval


def t(x):
    return {"median": x[0], "min": x[1]}


def h2d(data):
    pinned = data.cpu().pin_memory()
    dst = torch.empty_like(data)
    return events(lambda: dst.copy_(pinned, non_blocking=True))


def run_forget():
    N = args.regs
    vclk0, vval0 = registers(N, 1)
    y = torch.full((A,), 128, dtype=torch.int64, device=DEV)  # forgets about half the dots
    vclk, vval = vclk0.clone(), vval0.clone()

    def reset():
        vclk.copy_(vclk0)
        vval.copy_(vval0)

    t_reg = events(lambda: cg.mvreg.forget_batch(vclk, vval, y, ctx=ctx), before=reset)
    # the same value bytes as K = 1 Maps: a clock and an entry clock per state on top
    clock0 = vclk0.amax(dim=1)
    clock, ec = clock0.clone(), clock0.clone().view(N, 1, A)
    m_c, m_v = vclk.view(N, 1, V, A), vval.view(N, 1, V)

    def reset_map():
        reset()
        clock.copy_(clock0)
        ec.copy_(clock0.view(N, 1, A))

    t_map = events(lambda: cg.map.forget_batch(clock, ec, m_c, m_v, y, ctx=ctx), before=reset_map)
    # both calls leave the same registers (the Map forget zeroes an emptied slot where it sits; a
    # forget of the zero clock closes those holes)
    reset()
    cg.mvreg.forget_batch(vclk, vval, y, ctx=ctx)
    a_c, a_v = vclk.clone(), vval.clone()
    reset_map()
    cg.map.forget_batch(clock, ec, m_c, m_v, y, ctx=ctx)
    cg.mvreg.forget_batch(vclk, vval, torch.zeros_like(y), ctx=ctx)
    same = torch.equal(a_c, vclk) and torch.equal(a_v, vval)
    b_reg = (vclk.numel() + vval.numel()) * 8
    b_map = b_reg + (clock.numel() + ec.numel()) * 8
    ps_reg, ps_map = t_reg[0] * 1e6 / b_reg, t_map[0] * 1e6 / b_map
    emit({"op": "mvreg_forget", "regs": N, "V": V, "A": A, "same_result_as_map_forget": same,
          "mvreg_forget_us": t(t_reg), "map_forget_k1_us": t(t_map), "clock": "HIP events, states restored before every launch",
          "array_bytes": {"mvreg": b_reg, "map_k1": b_map},
          "ps_per_array_byte": {"mvreg": ps_reg, "map_k1": ps_map, "ratio": ps_reg / ps_map},
          "GBs_read_plus_write": {"mvreg": 2 * b_reg / t_reg[0] / 1e3, "map_k1": 2 * b_map / t_map[0] / 1e3},
          "within_10_percent_of_map_forget": ps_reg <= 1.10 * ps_map})
    return same


def run_states():
    N = args.regs
    vclk, vval = registers(N, 2)
    actors = sparse_ids(A, 3)
    off, data = wire.mvreg_egress(vclk, vval, actors, ctx=ctx)
    nbytes = data.numel()
    i_c, i_v, st = wire.mvreg_ingest(data, off, actors, V, ctx=ctx)
    ok = not st.any().item() and torch.equal(i_c, vclk) and torch.equal(i_v, vval)
    off2, data2 = wire.mvreg_egress(i_c, i_v, actors, ctx=ctx)
    ok = ok and torch.equal(off, off2) and torch.equal(data, data2)
    s = _abi.MVRegStates(N, A, V, i_c.data_ptr(), V * A, i_v.data_ptr(), V)
    t_in = events(lambda: ctx.call("crdt_mvreg_ingest", dptr(data), dptr(off), N, dptr(actors), A, ctypes.byref(s), dptr(st)))
    t_eg = host_clock(lambda: wire.mvreg_egress(vclk, vval, actors, ctx=ctx))
    t_h2d = h2d(data)
    gbs = lambda us: nbytes / us / 1e3  # noqa: E731
    emit({"op": "mvreg_states_wire", "regs": N, "V": V, "A": A, "frame_bytes": nbytes, "bytes_per_frame": nbytes / N,
          "round_trip": "ok" if ok else "MISMATCH",
          "ingest_us": dict(t(t_in), GBs=gbs(t_in[0]), clock="HIP events, the C entry point on buffers allocated once"),
          "egress_us": dict(t(t_eg), GBs=gbs(t_eg[0]), clock="host (two passes + sizing sync, wrapper allocations)"),
          "h2d_pinned_us": dict(t(t_h2d), GBs=gbs(t_h2d[0]), clock="HIP events"),
          "ingest_over_h2d": t_in[0] / t_h2d[0]})
    return ok


def run_ops():
    N, T = args.op_regs, args.ops
    g = torch.Generator(device=DEV)
    g.manual_seed(4)
    # every register's Puts advance four of its actors: each clock dominates the one before
    writers = torch.rand((N, 1, A), generator=g, device=DEV).argsort(dim=2) < 4
    inc = torch.randint(0, 4, (N, T, A), generator=g, device=DEV, dtype=torch.int64) * writers
    inc[:, :, 0] += writers[:, :, 0].long().expand(N, T)
    pool = inc.cumsum(dim=1).reshape(N * T, A).contiguous()
    pool = torch.cat([pool, torch.zeros((1, A), dtype=torch.int64, device=DEV)])
    ops = cg.mvreg.MVRegOpBatch(torch.arange(0, N * T + 1, T, dtype=torch.int64, device=DEV),
                                torch.arange(N * T, dtype=torch.int32, device=DEV), pool,
                                torch.randint(1, 1 << 62, (N * T,), generator=g, device=DEV, dtype=torch.int64))
    actors = sparse_ids(A, 5)
    off, data, est = wire.mvreg_ops_egress(ops, actors, ctx=ctx)
    nbytes = data.numel()
    want = 8 * N + 20 * N * T + 12 * int((pool != 0).sum().item())
    back = wire.mvreg_ops_ingest(data, off, actors, ctx=ctx)
    n = N * T
    ok = (not est.any().item() and nbytes == want and not back.status.any().item() and back.totals == (n, n)
          and torch.equal(back.ops.op_off, ops.op_off) and torch.equal(back.ops.clk_row[:n], ops.clk_row)
          and torch.equal(back.ops.clk_pool[:n], pool[:n]) and torch.equal(back.ops.val[:n], ops.val))
    off2, data2, _ = wire.mvreg_ops_egress(back.ops, actors, ctx=ctx)
    ok = ok and torch.equal(off, off2) and torch.equal(data, data2)
    o = back.ops
    b = _abi.MVRegOpsBuf(n, dptr(o.op_off), dptr(o.clk_row), dptr(o.clk_pool), n, dptr(o.val))
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    t_in = events(lambda: ctx.call("crdt_mvreg_ops_ingest", dptr(data), dptr(off), N, dptr(actors), A, ctypes.byref(b),
                                   dptr(st), None))
    ok = ok and not st.any().item()
    t_sync = host_clock(lambda: wire.mvreg_ops_ingest(data, off, actors, ctx=ctx))
    t_eg = host_clock(lambda: wire.mvreg_ops_egress(ops, actors, ctx=ctx))
    t_h2d = h2d(data)
    vclk = torch.zeros((N, V, A), dtype=torch.int64, device=DEV)
    vval = torch.zeros((N, V), dtype=torch.int64, device=DEV)

    def reset():
        vclk.zero_()
        vval.zero_()

    t_apply = events(lambda: cg.mvreg.apply_batch(vclk, vval, back.ops, ctx=ctx), before=reset)
    gbs = lambda us: nbytes / us / 1e3  # noqa: E731
    emit({"op": "mvreg_ops_wire", "regs": N, "ops_per_reg": T, "A": A, "frame_bytes": nbytes,
          "round_trip": "ok" if ok else "MISMATCH",
          "ingest_nosync_us": dict(t(t_in), GBs=gbs(t_in[0]), clock="HIP events, the C entry point on buffers allocated once"),
          "ingest_sync_us": dict(t(t_sync), GBs=gbs(t_sync[0]), clock="host (sizing call + fill, wrapper allocations)"),
          "egress_us": dict(t(t_eg), GBs=gbs(t_eg[0]), clock="host (two passes + sizing sync)"),
          "h2d_pinned_us": dict(t(t_h2d), GBs=gbs(t_h2d[0]), clock="HIP events"),
          "apply_us": dict(t(t_apply), clock="HIP events, registers zeroed before every launch"),
          "ingest_over_h2d": t_in[0] / t_h2d[0]})
    return ok


parts = {"forget": run_forget, "states": run_states, "ops": run_ops}
good = all([fn() for nm, fn in parts.items() if args.only in (None, nm)])
sys.exit(0 if good else 1)
