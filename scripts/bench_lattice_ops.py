"""The lattice types' op streams on one MI355X: the wire forms of Vec<Dot<u32>> / Vec<pncounter::Op> /
Vec<u64> / Vec<LWWReg> frames and crdt_lwwreg_apply_batch.

wire: 1,048,576 states x 64 ops (A = 32 actors, U = 256 elements) per type: the no-sync ingest (the C
entry point on buffers allocated once), the egress, the apply the ingest feeds and the chain
bytes -> ingest -> apply.  Beside them, in the same process: a pinned host-to-device copy of the same
frame bytes, and the time per frame byte of crdt_mvreg_ops_ingest at 65,536 x 64 Puts, A = 32.
lwwreg apply: uniform 64-op streams against crdt_lwwreg_lub_many with CRDT_ACCUMULATE and
first_conflict at G = N, R = 64 on the same data, the two interleaved launch by launch, states restored
before every launch; then a ragged batch of the same total (lengths 0..128) against the uniform one.

20 launches after 5 warm-ups each, median [min].  One JSON line per part, printed and appended to
--log (default profiles/lattice_ops_bench.log)."""
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
from crdts_gpu import _abi, lwwreg, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--states", type=int, default=1 << 20)
ap.add_argument("--ops", type=int, default=64)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--elems", type=int, default=256)
ap.add_argument("--put-regs", type=int, default=65536)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=["put", "vclock", "pncounter", "gset", "lwwreg", "apply"], default=None)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "lattice_ops_bench.log"))
args = ap.parse_args()
N, T, A, U = args.states, args.ops, args.actors, args.elems
REC = {"vclock": 12, "pncounter": 16, "gset": 8, "lwwreg": 16}

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = "cuda"
LOG = open(args.log, "a")


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def events(fn, before=None):
    """Call times by HIP events -> (median, min, max) in microseconds."""
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
        us.append(one(fn))
    return statistics.median(us), min(us), max(us)


def interleaved(fa, fb, before):
    """Two calls alternated launch by launch, `before` ahead of each -> their (median, min, max)."""
    for _ in range(args.warmup):
        before()
        fa()
        before()
        fb()
    ua, ub = [], []
    for _ in range(args.launches):
        for fn, us in ((fa, ua), (fb, ub)):
            before()
            torch.cuda.synchronize()
            us.append(one(fn))
    return tuple((statistics.median(u), min(u), max(u)) for u in (ua, ub))


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
    return statistics.median(us), min(us), max(us)


def t(x):
    return {"median": x[0], "min": x[1], "max": x[2]}


def h2d(data):
    pinned = data.cpu().pin_memory()
    dst = torch.empty_like(data)
    return events(lambda: dst.copy_(pinned, non_blocking=True))


def sparse_ids(n, seed, dt):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(1, 1 << 20, (n,), generator=g, device=DEV, dtype=torch.int64).cumsum(0).to(dt)


def run_put():
    """The Put-stream ingest of scripts/bench_mvreg.py, for its time per frame byte."""
    R = args.put_regs
    g = torch.Generator(device=DEV)
    g.manual_seed(4)
    writers = torch.rand((R, 1, A), generator=g, device=DEV).argsort(dim=2) < 4
    inc = torch.randint(0, 4, (R, T, A), generator=g, device=DEV, dtype=torch.int64) * writers
    inc[:, :, 0] += writers[:, :, 0].long().expand(R, T)
    pool = torch.cat([inc.cumsum(dim=1).reshape(R * T, A), torch.zeros((1, A), dtype=torch.int64, device=DEV)])
    ops = cg.mvreg.MVRegOpBatch(torch.arange(0, R * T + 1, T, dtype=torch.int64, device=DEV),
                                torch.arange(R * T, dtype=torch.int32, device=DEV), pool,
                                torch.randint(1, 1 << 62, (R * T,), generator=g, device=DEV, dtype=torch.int64))
    actors = sparse_ids(A, 5, torch.int32)
    off, data, _ = wire.mvreg_ops_egress(ops, actors, ctx=ctx)
    back = wire.mvreg_ops_ingest(data, off, actors, ctx=ctx)
    o, n = back.ops, R * T
    b = _abi.MVRegOpsBuf(n, dptr(o.op_off), dptr(o.clk_row), dptr(o.clk_pool), n, dptr(o.val))
    st = torch.empty(R, dtype=torch.int32, device=DEV)
    t_in = events(lambda: ctx.call("crdt_mvreg_ops_ingest", dptr(data), dptr(off), R, dptr(actors), A, ctypes.byref(b),
                                   dptr(st), None))
    t_eg = host_clock(lambda: wire.mvreg_ops_egress(ops, actors, ctx=ctx))
    ok = not st.any().item()
    PUT.update(ps_in=t_in[0] * 1e6 / data.numel(), ps_eg=t_eg[0] * 1e6 / data.numel())
    emit({"op": "mvreg_put_ingest_reference", "regs": R, "ops_per_reg": T, "A": A, "frame_bytes": data.numel(),
          "ok": ok, "ingest_nosync_us": t(t_in), "egress_us": t(t_eg), "ps_per_frame_byte": PUT})
    return ok


PUT = {}


def dense_ops(kind, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    n = N * T
    off = torch.arange(0, n + 1, T, dtype=torch.int64, device=DEV)
    if kind == "lwwreg":
        return lwwreg.LwwRegOpBatch(off, torch.randint(0, 1024, (n,), generator=g, device=DEV, dtype=torch.int64),
                                    torch.randint(0, 4, (n,), generator=g, device=DEV, dtype=torch.int64))
    sidx = torch.arange(N, dtype=torch.int32, device=DEV).repeat_interleave(T)
    col = torch.randint(0, U if kind == "gset" else A, (n,), generator=g, device=DEV, dtype=torch.int32)
    counter = None if kind == "gset" else torch.randint(1, 1 << 40, (n,), generator=g, device=DEV, dtype=torch.int64)
    dr = torch.randint(0, 2, (n,), generator=g, device=DEV, dtype=torch.uint8) if kind == "pncounter" else None
    return wire.DotOpBatch(off, sidx, col, counter, dr)


def run_wire(kind):
    n = N * T
    ops = dense_ops(kind, 10 + len(kind))
    d = None if kind == "lwwreg" else sparse_ids(U, 7, torch.int64) if kind == "gset" else sparse_ids(A, 7, torch.int32)
    dargs = () if d is None else (d,)
    eg = getattr(wire, f"{kind}_ops_egress")
    off, data, est = eg(ops, *dargs, ctx=ctx)
    nbytes = data.numel()
    back = getattr(wire, f"{kind}_ops_ingest")(data, off, *dargs, ctx=ctx)
    same = all(b is None or torch.equal(a, b) for a, b in zip(ops, back.ops))
    ok = not est.any().item() and nbytes == N * (8 + REC[kind] * T) and not back.status.any().item() \
        and back.totals == (n,) and same
    o = back.ops
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    if kind == "lwwreg":
        buf = _abi.LwwRegOpsBuf(n, dptr(o.op_off), dptr(o.marker), dptr(o.val))
        head = (dptr(data), dptr(off), N)
    else:
        buf = _abi.DotOpsBuf(n, dptr(o.op_off), dptr(o.state_idx), dptr(o.actor),
                             None if o.counter is None else dptr(o.counter), None if o.dir is None else dptr(o.dir))
        head = (dptr(data), dptr(off), N, dptr(d), d.shape[0])
    ingest = lambda: ctx.call(f"crdt_{kind}_ops_ingest", *head, ctypes.byref(buf), dptr(st), None)  # noqa: E731
    t_in = events(ingest)
    ok = ok and not st.any().item()
    t_sync = host_clock(lambda: getattr(wire, f"{kind}_ops_ingest")(data, off, *dargs, ctx=ctx))
    t_eg = host_clock(lambda: eg(ops, *dargs, ctx=ctx))
    t_h2d = h2d(data)
    # the apply the ingest feeds, and the chain bytes -> ingest -> apply
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    if kind == "lwwreg":
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        m0 = torch.randint(0, 1024, (N,), generator=g, device=DEV, dtype=torch.int64)
        states, v = m0.clone(), torch.zeros(N, dtype=torch.int64, device=DEV)
        conflict = torch.empty(n, dtype=torch.uint8, device=DEV)
        ast = torch.empty(N, dtype=torch.int32, device=DEV)
        lo = _abi.LwwRegOps(n, dptr(o.op_off), dptr(o.marker), dptr(o.val))
        reset = lambda: (states.copy_(m0), v.zero_())  # noqa: E731
        app = lambda: ctx.call("crdt_lwwreg_apply_batch", dptr(states), dptr(v), N, ctypes.byref(lo), dptr(conflict),  # noqa: E731
                               dptr(ast))
    else:
        W = (U + 63) // 64 if kind == "gset" else (2 * A if kind == "pncounter" else A)
        states = torch.zeros((N, W), dtype=torch.int64, device=DEV)
        reset = states.zero_
        tail = () if kind == "gset" else (dptr(o.counter),) + ((dptr(o.dir),) if kind == "pncounter" else ())
        app = lambda: ctx.call(f"crdt_{kind}_apply_batch", dptr(states), N, U if kind == "gset" else A, W,  # noqa: E731
                               dptr(o.state_idx), dptr(o.actor), *tail, n, dptr(bad))
    t_app = events(app, before=reset)
    t_chain = events(lambda: (ingest(), app()), before=reset)
    ok = ok and bad.item() == 0
    gbs = lambda us: nbytes / us / 1e3  # noqa: E731
    ps = t_in[0] * 1e6 / nbytes
    emit({"op": f"{kind}_ops_wire", "states": N, "ops_per_state": T, "dict": 0 if d is None else d.shape[0],
          "frame_bytes": nbytes, "round_trip": "ok" if ok else "MISMATCH",
          "ingest_nosync_us": dict(t(t_in), GBs=gbs(t_in[0]), clock="HIP events, the C entry point on buffers allocated once"),
          "ingest_sync_us": dict(t(t_sync), GBs=gbs(t_sync[0]), clock="host (sizing call + fill, wrapper allocations)"),
          "egress_us": dict(t(t_eg), GBs=gbs(t_eg[0]), clock="host (two passes + sizing sync)"),
          "h2d_pinned_us": dict(t(t_h2d), GBs=gbs(t_h2d[0]), clock="HIP events"),
          "ingest_over_h2d": t_in[0] / t_h2d[0], "egress_over_h2d": t_eg[0] / t_h2d[0],
          "ps_per_frame_byte": {"ingest": ps, "egress": t_eg[0] * 1e6 / nbytes, "put_ingest": PUT.get("ps_in"),
                                "put_egress": PUT.get("ps_eg"),
                                "ingest_over_put_ingest": ps / PUT["ps_in"] if PUT else None,
                                "egress_over_put_egress": t_eg[0] * 1e6 / nbytes / PUT["ps_eg"] if PUT else None},
          "apply_us": dict(t(t_app), ops_per_s=n / t_app[0] * 1e6, clock="HIP events, states reset before every launch"),
          "chain_us": dict(t(t_chain), sum_of_parts=t_in[0] + t_app[0], over_sum=t_chain[0] / (t_in[0] + t_app[0]),
                           over_apply=t_chain[0] / t_app[0], clock="HIP events around ingest + apply")})
    return ok


def run_apply():
    n = N * T
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    m0 = torch.randint(0, 1024, (N,), generator=g, device=DEV, dtype=torch.int64)
    v0 = torch.randint(0, 4, (N,), generator=g, device=DEV, dtype=torch.int64)
    om = torch.randint(0, 1024, (n,), generator=g, device=DEV, dtype=torch.int64)
    ov = torch.randint(0, 4, (n,), generator=g, device=DEV, dtype=torch.int64)
    off = torch.arange(0, n + 1, T, dtype=torch.int64, device=DEV)
    m, v = m0.clone(), v0.clone()
    conflict = torch.empty(n, dtype=torch.uint8, device=DEV)
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    fc = torch.empty(N, dtype=torch.int64, device=DEV)
    lo = _abi.LwwRegOps(n, dptr(off), dptr(om), dptr(ov))

    def reset():
        m.copy_(m0)
        v.copy_(v0)

    app = lambda: ctx.call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), N, ctypes.byref(lo), dptr(conflict), dptr(st))  # noqa: E731
    fold = lambda: ctx.call("crdt_lwwreg_lub_many", dptr(om), dptr(ov), N, T, T, dptr(m), dptr(v), dptr(fc),  # noqa: E731
                            _abi.CRDT_ACCUMULATE)
    reset()
    app()
    am, av = m.clone(), v.clone()
    c = conflict.view(N, T) != 0
    first = torch.where(c.any(dim=1), c.to(torch.int64).argmax(dim=1), torch.full((N,), -1, dtype=torch.int64, device=DEV))
    reset()
    fold()
    ok = torch.equal(am, m) and torch.equal(av, v) and torch.equal(first, fc)
    t_app, t_fold = interleaved(app, fold, reset)
    # ragged: lengths 0..128 in pairs (l, 128 - l): the same total
    half = torch.randint(0, 129, (N // 2,), generator=g, device=DEV, dtype=torch.int64)
    lens = torch.stack([half, 2 * T - half], dim=1).reshape(-1) if T == 64 else torch.full((N,), T, device=DEV)
    roff = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), lens.cumsum(0)])
    assert int(roff[-1]) == n
    ro = _abi.LwwRegOps(n, dptr(roff), dptr(om), dptr(ov))
    rag = lambda: ctx.call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), N, ctypes.byref(ro), dptr(conflict), dptr(st))  # noqa: E731
    t_uni, t_rag = interleaved(app, rag, reset)
    nbytes = 16 * n + n + 16 * 2 * N + 8 * N + 4 * N
    emit({"op": "lwwreg_apply_batch", "regs": N, "ops_per_reg": T, "same_states_and_first_conflict_as_lub_many": ok,
          "clock": "HIP events, the two calls alternated launch by launch, states restored before every launch",
          "apply_uniform_us": t(t_app), "lub_many_accumulate_first_conflict_us": t(t_fold),
          "apply_over_lub_many": t_app[0] / t_fold[0],
          "lub_many_spread_max_over_min": t_fold[2] / t_fold[1],
          "extra_traffic_of_the_conflict_bytes": 1 / 16,
          "within_extra_traffic_plus_baseline_spread": t_app[0] <= t_fold[0] * (1 + 1 / 16) * (t_fold[2] / t_fold[1]),
          "apply_bytes": nbytes, "apply_GBs": nbytes / t_app[0] / 1e3,
          "second_pair": {"apply_uniform_us": t(t_uni), "apply_ragged_us": t(t_rag), "ragged_over_uniform": t_rag[0] / t_uni[0]}})
    return ok


parts = [("put", run_put)] + [(k, (lambda k=k: run_wire(k))) for k in ("vclock", "pncounter", "gset", "lwwreg")] \
    + [("apply", run_apply)]
good = all([fn() for nm, fn in parts if args.only in (None, nm)])
sys.exit(0 if good else 1)
