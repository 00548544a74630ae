"""The value-typed Maps' op streams on the wire on one MI355X: crdt_map_{counter,orswot,nested}_ops_ingest /
_egress at scripts/bench_vmap_ops.py's shapes (Map<K, PNCounter> and Map<K, Orswot<M>>: 65,536 states x
64 ops; Map<K, Map<K2, MVReg>>: 32,768 x 32; A = 32, 15% Map Rms, Dcap 16).  The op batch is built on
the device in the ingest's own layout, the frames are produced by the new egress, and every run checks
ingest(egress(batch)) == batch field for field and egress(ingest(frames)) == frames byte for byte.

Reported per type, 20 launches after 5 warm-ups, median [min]: by HIP events the no-sync ingest (the C
entry point on buffers allocated once), a pinned host-to-device copy of the same frame bytes (the
feed), the apply the ingest feeds (states reset before every launch) and, as the comparator in the
same run, crdt_map_ops_ingest (Map<K, MVReg>, K = 256) at the same states x ops; by the host clock,
since it synchronises, the egress (both passes and the sizing synchronisation).  One JSON line per type."""
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
ap.add_argument("--nested-states", type=int, default=32768)
ap.add_argument("--nested-ops", type=int, default=32)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--dcap", type=int, default=16)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=["counter", "orswot", "nested"], default=None)
args = ap.parse_args()
A, Dcap = args.actors, args.dcap

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = "cuda"
gen = torch.Generator(device=DEV)
gen.manual_seed(0x5EED00A1)


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


def rand(*shape):
    return torch.rand(shape, generator=gen, device=DEV)


def randint(hi, n):
    return torch.randint(0, hi, (n,), generator=gen, device=DEV, dtype=torch.int64)


def sparse_ids(n, dtype, seed):
    """n distinct ascending ids (not their own indices)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    step = torch.randint(1, 1 << 20, (n,), generator=g, device=DEV, dtype=torch.int64)
    return (step.cumsum(0) * (1 if dtype == torch.int32 else 1 << 20)).to(dtype)


def rm_rows(t_of_op, ahead):
    """One rm clock row per op given: each actor present w.p. 0.3 with a counter up to the op's index + ahead."""
    hi = (t_of_op + ahead).clamp(min=2)[:, None].double()
    rows = 1 + (rand(t_of_op.shape[0], A).double() * (hi - 1)).long()
    rows[rand(t_of_op.shape[0], A) > 0.3] = 0
    return rows


def common(N, T, p_rm=0.15):
    n = N * T
    kind = (rand(n) < p_rm).to(torch.uint8)
    t = torch.arange(T, device=DEV).repeat(N)
    up = kind == 0
    counter = t + 1
    counter[rand(n) < 0.05] = 1  # seen dots
    excl = lambda x: torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), x.long().cumsum(0)])  # noqa: E731
    return n, kind, t, up, randint(A, n) * up, counter * up, excl


def build(name, N, T):
    """-> (batch in the ingest's layout, dictionaries after the actors' and keys', wire bytes it must take)."""
    i32, u8 = (lambda x: x.to(torch.int32)), (lambda x: x.to(torch.uint8))  # noqa: E731
    n, kind, t, up, actor, counter, excl = common(N, T)
    op_off = torch.arange(N + 1, device=DEV) * T
    rm = kind == 1
    n_rm = int(rm.sum())
    if name == "counter":  # Map<K, PNCounter>
        K = 64
        key = randint(K, n)
        pool = rm_rows(t[rm], 1)
        row = (excl(rm)[:-1] * rm)
        b = cg.map.MapCounterOpBatch(op_off, kind, i32(actor), counter, i32(key * up), i32(randint(A, n) * up),
                                     (1 + randint((1 << 20) - 1, n)) * up, u8(randint(2, n) * up), i32(row), pool,
                                     excl(rm), i32(key[rm]))
        nbytes = 8 * N + 36 * (n - n_rm) + 24 * n_rm + 12 * int((pool != 0).sum())
        return b, K, [], nbytes
    if name == "orswot":  # Map<K, Orswot<M>>
        K, M = 16, 8
        key = randint(K, n)
        vkind = u8((rand(n) < 0.2) & up)
        need = rm | (vkind == 1)
        pool = rm_rows(t[need], 1)
        row = excl(need)[:-1] * need
        add = up & (vkind == 0)
        b = cg.map.MapOrswotOpBatch(op_off, kind, i32(actor), counter, i32(key * up), vkind, i32(randint(A, n) * add),
                                    (t + 1) * add, i32(row), pool, excl(rm), i32(key[rm]), excl(up), i32(randint(M, n)[up]))
        n_add, n_orm = int(add.sum()), int((vkind == 1).sum())
        nbytes = 8 * N + 52 * n_add + 48 * n_orm + 24 * n_rm + 12 * int((pool != 0).sum())
        return b, K, [sparse_ids(M, torch.int64, 13)], nbytes
    K, K2 = 16, 8  # Map<K, Map<K2, MVReg>>
    key = randint(K, n)
    ikind = u8((rand(n) < 0.2) & up)
    put = up & (ikind == 0)
    iactor, icounter = randint(A, n) * put, (t + 1) * put
    pool = rm_rows(t, 2)
    pool[put] = 0
    pool[put.nonzero().squeeze(1), iactor[put]] = icounter[put]  # a Put's clock: its own dot (a fresh write)
    ikeys = (1 << randint(K2, n)) * (ikind == 1)
    b = cg.map.MapNestedOpBatch(op_off, kind, i32(actor), counter, i32(key * up), ikind, i32(iactor), icounter,
                                i32(randint(K2, n) * put), randint(1000, n) * put, ikeys, i32(torch.arange(n, device=DEV)),
                                pool, excl(rm), i32(key[rm]))
    n_put, n_irm = int(put.sum()), int((ikind == 1).sum())
    nbytes = 8 * N + 60 * n_put + 44 * n_irm + 24 * n_rm + 12 * int((pool != 0).sum())
    return b, K, [sparse_ids(K2, torch.int32, 14)], nbytes


def same_batch(a, b):
    """Field for field; b may have been filled into larger (capacity-sized) buffers."""
    ok = True
    for nm, x, y in zip(a._fields, a, b):
        y = y.reshape(-1)[:x.numel()].reshape(x.shape) if y.numel() >= x.numel() else y
        ok &= x.dtype == y.dtype and bool(torch.equal(x, y))
    return ok


def comparator(N, T):
    """crdt_map_ops_ingest (Map<K, MVReg>) at the same states x ops: no-sync, buffers allocated once."""
    K = 256
    ops = cg.synth.map_op_streams(N, T, K, A, seed=0x5EED000A, device=DEV)
    actors, keys = sparse_ids(A, torch.int32, 1), sparse_ids(K, torch.int32, 2)
    off, data, est = wire.map_ops_egress(ops, actors, keys, ctx=ctx)
    sized = wire.map_ops_ingest(data, off, actors, keys, ctx=ctx)
    held = wire.map_ops_ingest(data, off, actors, keys, sync=False, caps=sized.totals, ctx=ctx)
    o = held.ops
    b = _abi.MapOpsBuf()
    b.op_cap, b.row_cap, b.id_cap = sized.totals
    for nm in o._fields:
        setattr(b, nm, dptr(getattr(o, nm)))
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    t = events(lambda: ctx.call("crdt_map_ops_ingest", dptr(data), dptr(off), N, dptr(actors), A, dptr(keys), K,
                                ctypes.byref(b), dptr(held.row_off), dptr(held.id_off), dptr(st), None))
    assert not est.any().item() and not st.any().item()
    return t, data.numel()


def run(name):
    N, T = (args.nested_states, args.nested_ops) if name == "nested" else (args.states, args.ops)
    batch, K, third, want_bytes = build(name, N, T)
    actors, keys = sparse_ids(A, torch.int32, 11), sparse_ids(K, torch.int32, 12)
    pn = {"pn": True} if name == "counter" else {}
    egress = getattr(wire, f"map_{name}_ops_egress")
    ingest = getattr(wire, f"map_{name}_ops_ingest")
    off, data, est = egress(batch, actors, keys, *third, ctx=ctx, **pn)
    assert not est.any().item() and data.numel() == want_bytes, (data.numel(), want_bytes)
    back = ingest(data, off, actors, keys, *third, ctx=ctx, **pn)
    ok = not back.status.any().item() and same_batch(batch, back.batch)
    off2, data2, _ = egress(back.batch, actors, keys, *third, ctx=ctx, **pn)
    ok = ok and torch.equal(off, off2) and torch.equal(data, data2)
    nbytes = data.numel()
    caps = back.totals if name == "orswot" else back.totals[:3]
    # the entry point alone: the output buffers of one wrapper call, filled again in place
    held = ingest(data, off, actors, keys, *third, sync=False, caps=caps, ctx=ctx, **pn)
    o = held.batch
    b = {"counter": _abi.MapCounterOpsBuf, "orswot": _abi.MapOrswotOpsBuf, "nested": _abi.MapNestedOpsBuf}[name]()
    b.op_cap, b.row_cap, b.key_cap = caps[:3]
    if name == "orswot":
        b.mem_cap = caps[3]
    for nm in o._fields:
        setattr(b, nm, dptr(getattr(o, nm)))
    dicts = [dptr(actors), A, dptr(keys), K] + ([1] if name == "counter" else [dptr(third[0]), third[0].shape[0]])
    firsts = [dptr(held.row_off), dptr(held.key_first)] + ([dptr(held.mem_first)] if name == "orswot" else [])
    st = torch.empty(N, dtype=torch.int32, device=DEV)
    fn = f"crdt_map_{name}_ops_ingest"
    t_in = events(lambda: ctx.call(fn, dptr(data), dptr(off), N, *dicts, ctypes.byref(b), *firsts, dptr(st), None))
    ok = ok and not st.any().item() and same_batch(batch, held.batch)
    t_eg = host_clock(lambda: egress(batch, actors, keys, *third, ctx=ctx, **pn))
    # the feed: a pinned host-to-device copy of the frame bytes
    pinned = data.cpu().pin_memory()
    dst = torch.empty_like(data)
    t_h2d = events(lambda: dst.copy_(pinned, non_blocking=True))
    # the apply the ingest feeds
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)  # noqa: E731
    slots = [z(N, Dcap, A), z(N, Dcap, 1), z32(N)]
    if name == "counter":
        stt = [z(N, A), z(N, K, A), z(N, K, 2, A)]
        apply = lambda: cg.map.counter_apply_batch(*stt, *slots, back.batch, ctx=ctx)  # noqa: E731
    elif name == "orswot":
        stt = [z(N, A), z(N, K, A), z(N, K, A), z(N, K, 8, A), z32(N, K), z(N, K, 16, A), z(N, K, 16)]
        res = cg.map.MapOrswotLub(*stt, None, None, None)
        apply = lambda: cg.map.orswot_apply_batch(res, *slots, back.batch, ctx=ctx)  # noqa: E731
    else:
        stt = [z(N, A), z(N, K, A), z(N, K, A), z(N, K, 8, A), z(N, K, 8, 8, A), z(N, K, 8, 8), z32(N, K, 8), z32(N, K),
               z(N, K, 16, A), z(N, K, 16)]
        res = wire.MapNestedFrames(*stt, *slots)
        apply = lambda: cg.map.nested_apply_batch(res, *slots, back.batch, ctx=ctx)  # noqa: E731

    def reset():
        for t in stt + slots:
            t.zero_()

    t_apply = events(apply, before=reset)
    del stt, slots
    t_cmp, cmp_bytes = comparator(N, T)
    n_ops = N * T
    print(json.dumps({
        "op": f"map_{name}_ops_wire", "states": N, "ops_per_state": T, "actors": A, "keys": K, "dcap": Dcap,
        "removes": int((batch.kind == 1).sum()), "frame_bytes": nbytes, "round_trip": "ok" if ok else "MISMATCH",
        "ingest_nosync_us": {"median": t_in[0], "min": t_in[1], "GBs": nbytes / t_in[0] / 1e3,
                             "Mops_per_s": n_ops / t_in[0], "clock": "HIP events, the C entry point on buffers allocated once"},
        "egress_us": {"median": t_eg[0], "min": t_eg[1], "GBs": nbytes / t_eg[0] / 1e3,
                      "clock": "host (two passes + sizing sync)"},
        "h2d_pinned_us": {"median": t_h2d[0], "min": t_h2d[1], "GBs": nbytes / t_h2d[0] / 1e3, "clock": "HIP events"},
        "apply_us": {"median": t_apply[0], "min": t_apply[1], "clock": "HIP events"},
        "map_mvreg_ops_ingest_us": {"median": t_cmp[0], "min": t_cmp[1], "frame_bytes": cmp_bytes,
                                    "Mops_per_s": n_ops / t_cmp[0],
                                    "clock": "HIP events, crdt_map_ops_ingest at the same states x ops, same run"},
        "ingest_over_h2d": t_in[0] / t_h2d[0], "ingest_over_apply": t_in[0] / t_apply[0],
        "ops_rate_over_mvreg_map": t_cmp[0] / t_in[0],
    }), flush=True)
    return ok


good = all([run(n) for n in (["counter", "orswot", "nested"] if args.only is None else [args.only])])
sys.exit(0 if good else 1)
