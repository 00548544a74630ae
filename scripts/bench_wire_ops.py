"""Op streams on the wire on one MI355X: crdt_*_ops_ingest / crdt_*_ops_egress at the apply benches'
shapes (Orswot: 65,536 states x 64 ops, M = 1,024, A = 64, 20% Rms; Map<K, MVReg>: K = 256, A = 32,
V = 4).  The device op batch is built as scripts/bench_orswot_apply.py / bench_map_apply.py build it,
the frames are produced by the new egress, and every run checks ingest(egress(batch)) == batch.

Reported per type: the frame bytes (computed from the batch and checked against the egress total)
and call times, 20 launches after 5 warm-ups each, median [min]: by HIP events the no-sync ingest
(the C entry point on buffers allocated once, and the Python wrapper, which allocates its outputs in
every call); by the host clock, since they synchronise, the sizing + fill ingest, its count half alone
(the sizing call) and the egress (both passes and the sizing synchronisation); GB/s of frames; and in
the same run, by HIP events, (a) a pinned host-to-device copy of those frame bytes (the feed) and (b)
the apply kernel's time on the ingested batch (states reset before every launch).  One JSON line per
type."""
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
ap.add_argument("--states", type=int, default=65536)
ap.add_argument("--ops", type=int, default=64)
ap.add_argument("--members", type=int, default=1024)
ap.add_argument("--actors", type=int, default=64)
ap.add_argument("--keys", type=int, default=256)
ap.add_argument("--map-actors", type=int, default=32)
ap.add_argument("--vals", type=int, default=4)
ap.add_argument("--dcap", type=int, default=16)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=["orswot", "map"], default=None)
args = ap.parse_args()
N, T = args.states, args.ops

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = "cuda"


def events(fn, launches=args.launches, warmup=args.warmup, before=None):
    """Call times by HIP events -> (median, min) in microseconds."""
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(launches):
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


def host_clock(fn, launches=args.launches, warmup=args.warmup):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us), min(us)


def sparse_ids(n, dtype, seed):
    """n distinct ascending ids (not their own indices): odd multiples spread over the id space."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    step = torch.randint(1, 1 << 20, (n,), generator=g, device=DEV, dtype=torch.int64)
    ids = step.cumsum(0) * (1 if dtype == torch.int32 else 1 << 20)
    return ids.to(dtype)


def nnz_rows(pool, rows):
    return int((pool[rows.long()] != 0).sum().item())


def same_orswot(a, b):
    """Batch equality by meaning (the synthetic batch is not in the ingest's canonical layout: it
    keeps a clock row per op and an actor on Rms)."""
    add = a.kind == 0
    ok = torch.equal(a.op_off, b.op_off) and torch.equal(a.kind, b.kind[:a.kind.shape[0]])
    n = a.kind.shape[0]
    ok &= torch.equal(a.actor[add], b.actor[:n][add]) and torch.equal(a.counter[add], b.counter[:n][add])
    ok &= torch.equal(a.rm_clock[a.rm_row[~add].long()], b.rm_clock[b.rm_row[:n][~add].long()])
    la, lb = a.mem_off[1:n + 1] - a.mem_off[:n], b.mem_off[1:n + 1] - b.mem_off[:n]
    ok &= torch.equal(la, lb) and bool((la == 1).all())
    ok &= torch.equal(a.mem[a.mem_off[:n]], b.mem[b.mem_off[:n]])
    return bool(ok)


def same_map(a, b):
    n = a.kind.shape[0]
    up = a.kind == 0
    ok = torch.equal(a.op_off, b.op_off) and torch.equal(a.kind, b.kind[:n])
    for f in ("actor", "counter", "key", "val"):
        ok &= torch.equal(getattr(a, f)[up], getattr(b, f)[:n][up])
    ok &= torch.equal(a.clk_pool[a.clk_row.long()], b.clk_pool[b.clk_row[:n].long()])
    lb = b.key_off[1:n + 1] - b.key_off[:n]
    ok &= bool((lb[~up] == 1).all()) and bool((lb[up] == 0).all())
    ok &= torch.equal(a.keys[a.key_off[:n][~up]], b.keys[b.key_off[:n][~up]])
    return bool(ok)


def run(name):
    is_map = name == "map"
    if is_map:
        A, U = args.map_actors, args.keys
        ops = cg.synth.map_op_streams(N, T, U, A, seed=0x5EED000A, device=DEV)
        actors, ids = sparse_ids(A, torch.int32, 1), sparse_ids(U, torch.int32, 2)
        egress, ingest, same = wire.map_ops_egress, wire.map_ops_ingest, same_map
        n_rm = int((ops.kind == 1).sum().item())
        n_up = N * T - n_rm
        nnz = int((ops.clk_pool != 0).sum().item())
        # Up: tag 4 + dot 12 + key 4 + MVReg tag 4 + clock (8 + 12 nnz) + val 8; Rm: tag 4 + clock + len 8 + key 4
        want_bytes = 8 * N + 40 * n_up + 24 * n_rm + 12 * nnz
    else:
        A, U = args.actors, args.members
        ops = cg.synth.orswot_op_streams(N, T, U, A, seed=0x5EED0009, p_rm=0.2, p_future=0.3, device=DEV)
        actors, ids = sparse_ids(A, torch.int32, 3), sparse_ids(U, torch.int64, 4)
        egress, ingest, same = wire.orswot_ops_egress, wire.orswot_ops_ingest, same_orswot
        rm = ops.kind == 1
        n_rm = int(rm.sum().item())
        nnz = nnz_rows(ops.rm_clock, ops.rm_row[rm])
        # Add: tag 4 + dot 12 + len 8 + member 8; Rm: tag 4 + clock (8 + 12 nnz) + len 8 + member 8
        want_bytes = 8 * N + 32 * (N * T - n_rm) + 28 * n_rm + 12 * nnz
    off, data, est = egress(ops, actors, ids, ctx=ctx)
    assert not est.any().item() and data.numel() == want_bytes, (data.numel(), want_bytes)
    back = ingest(data, off, actors, ids, ctx=ctx)
    ok = not back.status.any().item() and same(ops, back.ops)
    off2, data2, _ = egress(back.ops, actors, ids, ctx=ctx)
    ok = ok and torch.equal(off, off2) and torch.equal(data, data2)
    caps = back.totals
    nbytes = data.numel()

    t_wrap = events(lambda: ingest(data, off, actors, ids, sync=False, caps=caps, ctx=ctx))
    t_sync = host_clock(lambda: ingest(data, off, actors, ids, ctx=ctx))
    tot = (ctypes.c_uint64 * 3)()
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    fn = "crdt_map_ops_ingest" if is_map else "crdt_orswot_ops_ingest"
    # the entry point alone: the output buffers of one wrapper call, filled again in place
    held = ingest(data, off, actors, ids, sync=False, caps=caps, ctx=ctx)
    o = held.ops
    b = (_abi.MapOpsBuf if is_map else _abi.OrswotOpsBuf)()
    b.op_cap, b.row_cap, b.id_cap = caps
    b.op_off, b.kind, b.actor, b.counter = dptr(o.op_off), dptr(o.kind), dptr(o.actor), dptr(o.counter)
    if is_map:
        b.key, b.val, b.clk_row, b.clk_pool, b.key_off, b.keys = (dptr(o.key), dptr(o.val), dptr(o.clk_row),
                                                                  dptr(o.clk_pool), dptr(o.key_off), dptr(o.keys))
    else:
        b.rm_row, b.rm_clock, b.mem_off, b.mem = dptr(o.rm_row), dptr(o.rm_clock), dptr(o.mem_off), dptr(o.mem)
    t_in = events(lambda: ctx.call(fn, dptr(data), dptr(off), N, dptr(actors), A, dptr(ids), U, ctypes.byref(b),
                                   dptr(held.row_off), dptr(held.id_off), dptr(st), None))
    ok = ok and not st.any().item() and same(ops, held.ops)
    t_count = host_clock(lambda: ctx.call(fn, dptr(data), dptr(off), N, dptr(actors), A, dptr(ids), U, None, None, None,
                                          dptr(st), tot))
    t_eg = host_clock(lambda: egress(ops, actors, ids, ctx=ctx))
    # (a) the feed: a pinned host-to-device copy of the frame bytes
    pinned = data.cpu().pin_memory()
    dst = torch.empty_like(data)
    t_h2d = events(lambda: dst.copy_(pinned, non_blocking=True))
    # (b) the apply kernel on the ingested batch
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    if is_map:
        Kw = (U + 63) // 64
        stt = [z(N, A), z(N, U, A), z(N, U, args.vals, A), z(N, U, args.vals), z(N, args.dcap, A), z(N, args.dcap, Kw)]
        apply = lambda: cg.map.apply_batch(*stt, cnt, back.ops, ctx=ctx)  # noqa: E731
    else:
        stt = [z(N, A), z(N, U, A), z(N, args.dcap, A), z(N, args.dcap, (U + 63) // 64)]
        apply = lambda: cg.orswot.apply_batch(*stt, cnt, back.ops, ctx=ctx)  # noqa: E731

    def reset():
        for t in stt[:4 if is_map else 2]:
            t.zero_()
        cnt.zero_()

    t_apply = events(apply, before=reset)
    gbs = lambda us: nbytes / us / 1e3  # noqa: E731
    print(json.dumps({
        "op": f"{name}_ops_wire", "states": N, "ops_per_state": T, "actors": A, "ids": U, "removes": n_rm,
        "frame_bytes": nbytes, "round_trip": "ok" if ok else "MISMATCH",
        "ingest_nosync_us": {"median": t_in[0], "min": t_in[1], "GBs": gbs(t_in[0]),
                             "clock": "HIP events, the C entry point on buffers allocated once"},
        "ingest_nosync_wrapper_us": {"median": t_wrap[0], "min": t_wrap[1], "GBs": gbs(t_wrap[0]),
                                     "clock": "HIP events, the Python wrapper (allocates its outputs per call)"},
        "ingest_sync_us": {"median": t_sync[0], "min": t_sync[1], "GBs": gbs(t_sync[0]), "clock": "host"},
        "ingest_count_half_us": {"median": t_count[0], "min": t_count[1], "clock": "host (the sizing call)"},
        "egress_us": {"median": t_eg[0], "min": t_eg[1], "GBs": gbs(t_eg[0]), "clock": "host (two passes + sizing sync)"},
        "h2d_pinned_us": {"median": t_h2d[0], "min": t_h2d[1], "GBs": gbs(t_h2d[0]), "clock": "HIP events"},
        "apply_us": {"median": t_apply[0], "min": t_apply[1], "clock": "HIP events"},
        "ingest_over_h2d": t_in[0] / t_h2d[0],
    }), flush=True)
    return ok


good = all([run(n) for n in (["orswot", "map"] if args.only is None else [args.only])])
sys.exit(0 if good else 1)
