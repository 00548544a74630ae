"""Batched state equality of the value-typed Maps on one MI355X: crdt_map_counter_eq_batch (W = 1, 2),
crdt_map_orswot_eq_batch (M = 4) and crdt_map_nested_eq_batch (K2 = 8, Vs = 8) at K = 1,024, A = 32, with
N chosen so that both sides' live bytes are several GiB.  Live bytes are what the semantics require to
be read: every row and count, but no nested slot past vd_n / id_n and no register row past nval.

Each type runs twice: "identical" = y a bit-identical copy of x with all lists empty, "permuted" = inner
register slots rolled by one (nested), 4 live nested slots on every 16th key with y's reversed, and 4 live
Map-level slots with y's reversed (equal states on another layout).  Reported per run: the call time by
HIP events (20 launches after 5 warm-ups, median [min]), GB/s over the live bytes of both sides, the
share of 8 TB/s, the time per byte against crdt_map_eq_batch at 8,192 x K 1,024 x V 2 x A 32 (the
yardstick, run three times so its own spread shows), the ratio to the matching *_merge_batch on the same
pairs (self restored before every launch, outside the events) and to the torch expression
(x == y).flatten(1).all(1) over the same tensors.  One JSON line per run, printed and appended to --log
(default profiles/eq_vmap_bench.log).

Without --only every part runs in a child process of its own under a time limit, and the first failing
step stops the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ["yardstick", "counter1", "counter2", "orswot", "nested"]
ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=PARTS, default=None)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scale", type=float, default=1.0, help="multiplies every N (a smaller run for a first look)")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--tune", default=None, help='CRDT_TUNE keys for the ctx, e.g. "eqvppl=4,eqvbpc=64"')
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "eq_vmap_bench.log"))
args = ap.parse_args()

if args.only is None:
    for part in PARTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", part] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"bench_eq_vmap: step {part} failed with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402

sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd"), os.path.join(ROOT, "oracle")]
import crdts_gpu as cg  # noqa: E402
from crdts_gpu import synth, wire  # noqa: E402

torch.cuda.set_device(0)
ctx = cg.Context(0)
if args.tune:
    ctx.tune(args.tune)
DEV = torch.device("cuda", 0)
LOG = open(args.log, "a")
K, A, DCAP, LCAP = 1024, 32, 8, 16
GEN = torch.Generator(device=DEV)
GEN.manual_seed(7)


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


def rnd(*shape, lo=1, hi=256):
    return torch.randint(lo, hi, shape, generator=GEN, device=DEV, dtype=torch.int64)


def zeros(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def torch_eq(x, y):
    acc = None
    for a, b in zip(x, y):
        r = (a == b).reshape(a.shape[0], -1).all(1)
        acc = r if acc is None else acc & r
    return acc


def slots(N, cap, W, live):
    """(clock (N, cap, A), sets (N, cap, W), count (N,)) with `live` slots used; and the same reversed."""
    dc, ds = zeros(N, cap, A), zeros(N, cap, W)
    if live:
        dc[:, :live] = rnd(N, live, A, lo=1 << 20, hi=1 << 21)
        ds[:, :live] = rnd(N, live, W, lo=0, hi=1 << 62)
    cnt = torch.full((N,), live, dtype=torch.int32, device=DEV)
    rc, rs = dc.clone(), ds.clone()
    if live:
        rc[:, :live], rs[:, :live] = dc[:, :live].flip(1), ds[:, :live].flip(1)
    return (dc, ds, cnt), (rc, rs, cnt.clone())


def nested_lists(N, W, live):
    """Per-key lists: `live` slots on every 16th key, none elsewhere; and the same with the slots reversed."""
    n, c, s = zeros(N, K, dtype=torch.int32), zeros(N, K, LCAP, A), zeros(N, K, LCAP, W)
    if live:
        n[:, ::16] = live
        c[:, ::16, :live] = rnd(N, K // 16, live, A, lo=1 << 20, hi=1 << 21)
        s[:, ::16, :live] = rnd(N, K // 16, live, W, lo=1, hi=255)
    rc, rs = c.clone(), s.clone()
    if live:
        rc[:, :, :live], rs[:, :, :live] = c[:, :, :live].flip(2), s[:, :, :live].flip(2)
    sq = (lambda t: t[..., 0].contiguous()) if W == 1 else (lambda t: t)
    per_key = live * (A + W) * 8 // 16  # live list bytes per key, averaged
    return (n, c, sq(s)), (n.clone(), rc, sq(rs)), per_key


def report(op, case, shape, x, y, live_bytes, eq, merge, yard):
    ne = eq()
    unequal = int((ne != 0).sum())
    t_eq = events(eq)
    work = type(x)(*[t.clone() for t in x])
    t_merge = events(lambda: merge(work, y, ctx=ctx), lambda: [w.copy_(s) for w, s in zip(work, x)])
    del work
    torch.cuda.empty_cache()
    t_torch = events(lambda: torch_eq(x, y))
    d = {"op": op, "case": case, **shape, "unequal_pairs": unequal, "live_bytes_both_sides": live_bytes,
         "eq_us": {"median": t_eq[0], "min": t_eq[1]}, "GBs": live_bytes / t_eq[0] / 1e3,
         "frac_of_8TBs": live_bytes / t_eq[0] / 8e6, "ns_per_KiB": t_eq[0] * 1e3 / (live_bytes / 1024),
         "per_byte_over_map_eq": (t_eq[0] / live_bytes) / yard if yard else None,
         "merge_batch_us": {"median": t_merge[0], "min": t_merge[1]}, "eq_over_merge": t_eq[0] / t_merge[0],
         "torch_us": {"median": t_torch[0], "min": t_torch[1]}, "eq_over_torch": t_eq[0] / t_torch[0]}
    emit(d)
    return d


def yardstick(runs=3, N=8192):
    """crdt_map_eq_batch, identical layout: us per byte, `runs` times."""
    N = max(64, int(N * args.scale))
    a = synth.map_replicas(ctx, N, K, A, 2, 0x5EED0004, kmax=256, p_def=0.2)
    d, _ = slots(N, DCAP, K // 64, 0)
    x = cg.map.MapStates(a.clock, a.ec, a.vclk, a.vval, *d)
    y = cg.map.MapStates(*[t.clone() for t in x])
    b = 2 * nbytes(x[:4])
    per = []
    for i in range(runs):
        t = events(lambda: cg.map.eq_batch(x, y, ctx=ctx))
        per.append(t[0] / b)
        emit({"op": "map_eq_batch", "case": "yardstick", "run": i, "pairs": N, "K": K, "V": 2, "A": A, "bytes_both_sides": b,
              "eq_us": {"median": t[0], "min": t[1]}, "GBs": b / t[0] / 1e3, "frac_of_8TBs": b / t[0] / 8e6,
              "ns_per_KiB": t[0] * 1e3 / (b / 1024)})
    emit({"op": "map_eq_batch", "case": "yardstick", "spread_max_over_min": max(per) / min(per)})
    del x, y, a
    torch.cuda.empty_cache()
    return statistics.median(per)


def finish(op, out):
    emit({"op": op, "permuted_over_identical": out[1]["eq_us"]["median"] / out[0]["eq_us"]["median"]})


def counter(W):
    N = max(16, int(4096 * args.scale))
    yard = yardstick(1)
    clock, ec, val = rnd(N, A), rnd(N, K, A), rnd(N, K, W, A)
    out = []
    for case, live in (("identical", 0), ("permuted", 4)):
        dx, dy = slots(N, DCAP, K // 64, live)
        x = wire.MapCounterFrames(clock, ec, val, *dx)
        y = wire.MapCounterFrames(clock.clone(), ec.clone(), val.clone(), *dy)
        b = 2 * (nbytes(x[:3]) + N * 4 + N * live * (A + K // 64) * 8)
        out.append(report("map_counter_eq_batch", case, {"pairs": N, "K": K, "W": W, "A": A, "live_deferred": live}, x, y, b,
                          lambda: cg.map.counter_eq_batch(x, y, ctx=ctx), cg.map.counter_merge_batch, yard))
        del x, y, dx, dy
        torch.cuda.empty_cache()
    finish(f"map_counter_eq_batch W={W}", out)


def orswot():
    N, M = max(16, int(1024 * args.scale)), 4
    yard = yardstick(1)
    clock, ec, oc, ent = rnd(N, A), rnd(N, K, A), rnd(N, K, A), rnd(N, K, M, A)
    out = []
    for case, live in (("identical", 0), ("permuted", 4)):
        dx, dy = slots(N, DCAP, K // 64, live)
        lx, ly, per_key = nested_lists(N, 1, live)
        x = wire.MapOrswotFrames(clock, ec, oc, ent, *lx, *dx)
        y = wire.MapOrswotFrames(clock.clone(), ec.clone(), oc.clone(), ent.clone(), *ly, *dy)
        b = 2 * (nbytes(x[:4]) + N * K * (4 + per_key) + N * 4 + N * live * (A + K // 64) * 8)
        out.append(report("map_orswot_eq_batch", case, {"pairs": N, "K": K, "M": M, "A": A, "live_deferred": live,
                                                        "live_nested_every_16th_key": live}, x, y, b,
                          lambda: cg.map.orswot_eq_batch(x, y, ctx=ctx), cg.map.orswot_merge_batch, yard))
        del x, y, dx, dy, lx, ly
        torch.cuda.empty_cache()
    finish("map_orswot_eq_batch", out)


def nested():
    N, K2, VS = max(4, int(128 * args.scale)), 8, 8
    yard = yardstick(1)
    clock, ec, ic, iec = rnd(N, A), rnd(N, K, A), rnd(N, K, A), rnd(N, K, K2, A)
    ivc, ivv = rnd(N, K, K2, VS, A), rnd(N, K, K2, VS, lo=1, hi=1 << 40)
    nval = torch.full((N, K, K2), VS, dtype=torch.int32, device=DEV)
    out = []
    for case, live in (("identical", 0), ("permuted", 4)):
        dx, dy = slots(N, DCAP, K // 64, live)
        lx, ly, per_key = nested_lists(N, 1, live)
        x = wire.MapNestedFrames(clock, ec, ic, iec, ivc, ivv, nval, *lx, *dx)
        yc, yv = (ivc.clone(), ivv.clone()) if not live else (ivc.roll(1, 3).contiguous(), ivv.roll(1, 3).contiguous())
        y = wire.MapNestedFrames(clock.clone(), ec.clone(), ic.clone(), iec.clone(), yc, yv, nval.clone(), *ly, *dy)
        b = 2 * (nbytes(x[:7]) + N * K * (4 + per_key) + N * 4 + N * live * (A + K // 64) * 8)
        out.append(report("map_nested_eq_batch", case, {"pairs": N, "K": K, "K2": K2, "Vs": VS, "A": A, "live_deferred": live,
                                                        "live_inner_every_16th_key": live, "slots_rolled": bool(live)},
                          x, y, b, lambda: cg.map.nested_eq_batch(x, y, ctx=ctx), cg.map.nested_merge_batch, yard))
        del x, y, dx, dy, lx, ly, yc, yv
        torch.cuda.empty_cache()
    finish("map_nested_eq_batch", out)


{"yardstick": lambda: yardstick(3), "counter1": lambda: counter(1), "counter2": lambda: counter(2), "orswot": orswot,
 "nested": nested}[args.only]()
