"""Batched state equality on one MI355X: crdt_mvreg_eq_batch, crdt_orswot_eq_batch, crdt_map_eq_batch.

MVReg: 1,048,576 pairs x V = 4 x A = 32 (the forget bench's shape).  Orswot / Map: 8,192 pairs at the
config-3 / config-4 state shapes (the merge_batch rows' shapes).  Each type runs twice: "fast" = y a
bit-identical copy of x with empty deferred lists, "permuted" = y's value slots rolled by one and 4 live
deferred slots per state, y's in reverse order (equal states on another layout).  Reported per run: the
call time by HIP events (20 launches after 5 warm-ups, median [min]), GB/s over the bytes of both
sides, the share of 8 TB/s, the ratio to crdt_*_merge_batch on the same pairs (self restored before
every launch, outside the events) and to the torch expression (x == y).flatten(1).all(1) over the same
tensors.  One JSON line per run, printed and appended to --log (default profiles/eq_bench.log).

Without --only every type runs in a child process of its own under a time limit, and the first
failing step stops the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["mvreg", "orswot", "map"], default=None)
ap.add_argument("--regs", type=int, default=1 << 20)
ap.add_argument("--pairs", type=int, default=8192)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "eq_bench.log"))
args = ap.parse_args()

if args.only is None:
    for part in ("mvreg", "orswot", "map"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", part] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"bench_eq: step {part} failed with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402

sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd"), os.path.join(ROOT, "oracle")]
import crdts_gpu as cg  # noqa: E402
from crdts_gpu import synth  # noqa: E402

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = torch.device("cuda", 0)
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


def nbytes(side):
    return sum(t.numel() * t.element_size() for t in side)


def torch_eq(x, y):
    acc = None
    for a, b in zip(x, y):
        r = (a == b).flatten(1).all(1)
        acc = r if acc is None else acc & r
    return acc


def report(op, case, shape, x, y, eq, merge, restore):
    """x, y: the tensors both calls stream (tuples); eq / merge: the calls; restore: self before a merge."""
    ne = eq()
    unequal = int((ne != 0).sum())
    t_eq = events(eq)
    t_merge = events(merge, restore)
    t_torch = events(lambda: torch_eq(x, y))
    b = nbytes(x) + nbytes(y)
    d = {"op": op, "case": case, **shape, "unequal_pairs": unequal, "bytes_both_sides": b,
         "eq_us": {"median": t_eq[0], "min": t_eq[1]}, "GBs": b / t_eq[0] / 1e3, "frac_of_8TBs": b / t_eq[0] / 8e6,
         "merge_batch_us": {"median": t_merge[0], "min": t_merge[1]}, "eq_over_merge": t_eq[0] / t_merge[0],
         "torch_us": {"median": t_torch[0], "min": t_torch[1]}, "eq_over_torch": t_eq[0] / t_torch[0]}
    emit(d)
    return d


def deferred(N, Dcap, A, W, live, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    dc = torch.zeros((N, Dcap, A), dtype=torch.int64, device=DEV)
    ds = torch.zeros((N, Dcap, W), dtype=torch.int64, device=DEV)
    if live:
        dc[:, :live] = torch.randint(1 << 20, 1 << 21, (N, live, A), generator=g, device=DEV, dtype=torch.int64)
        ds[:, :live] = torch.randint(0, 1 << 62, (N, live, W), generator=g, device=DEV, dtype=torch.int64)
    return dc, ds, torch.full((N,), live, dtype=torch.int32, device=DEV)


def reversed_live(dc, ds, cnt, live):
    dc, ds = dc.clone(), ds.clone()
    if live:
        dc[:, :live] = dc[:, :live].flip(1)
        ds[:, :live] = ds[:, :live].flip(1)
    return dc, ds, cnt.clone()


def mvreg():
    N, V, A = args.regs, 4, 32
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    cnt = torch.randint(1, 256, (N, V, A), generator=g, device=DEV, dtype=torch.int64)
    keep = torch.rand((N, V, A), generator=g, device=DEV) < 3.0 / A
    keep[:, torch.arange(V), torch.arange(V) % A] = True  # no empty slot
    x = (cnt * keep, torch.randint(1, 1 << 62, (N, V), generator=g, device=DEV, dtype=torch.int64))
    out = []
    for case in ("fast", "permuted"):
        y = tuple(t.clone() for t in x) if case == "fast" else tuple(t.roll(1, 1).contiguous() for t in x)
        work = tuple(t.clone() for t in x)
        out.append(report("mvreg_eq_batch", case, {"pairs": N, "V": V, "A": A}, x, y,
                          lambda: cg.mvreg.eq_batch(*x, *y, ctx=ctx), lambda: cg.mvreg.merge_batch(*work, *y, ctx=ctx),
                          lambda: [w.copy_(s) for w, s in zip(work, x)]))
        del y, work
    emit({"op": "mvreg_eq_batch", "permuted_over_fast": out[1]["eq_us"]["median"] / out[0]["eq_us"]["median"]})


def orswot():
    N, M, A, Dcap = args.pairs, 4096, 64, 8
    a = synth.orswot_replicas(ctx, N, M, A, seed=0x5EED0003, kmax=48, p_def=0.2)
    out = []
    for case, live in (("fast", 0), ("permuted", 4)):
        d = deferred(N, Dcap, A, (M + 63) // 64, live, 2)
        x = cg.orswot.OrswotStates(a.clock, a.entries, *d)
        y = cg.orswot.OrswotStates(a.clock.clone(), a.entries.clone(), *reversed_live(*d, live))
        work = cg.orswot.OrswotStates(*[t.clone() for t in x])
        out.append(report("orswot_eq_batch", case, {"pairs": N, "M": M, "A": A, "live_deferred": live}, tuple(x[:2]),
                          tuple(y[:2]), lambda: cg.orswot.eq_batch(x, y, ctx=ctx),
                          lambda: cg.orswot.merge_batch(work, y, ctx=ctx), lambda: [w.copy_(s) for w, s in zip(work, x)]))
        del x, y, work, d
        torch.cuda.empty_cache()
    emit({"op": "orswot_eq_batch", "permuted_over_fast": out[1]["eq_us"]["median"] / out[0]["eq_us"]["median"]})


def mapb():
    N, K, A, V, Dcap = args.pairs, 1024, 32, 2, 8
    a = synth.map_replicas(ctx, N, K, A, V, 0x5EED0004, kmax=256, p_def=0.2)
    out = []
    for case, live in (("fast", 0), ("permuted", 4)):
        d = deferred(N, Dcap, A, (K + 63) // 64, live, 3)
        x = cg.map.MapStates(a.clock, a.ec, a.vclk, a.vval, *d)
        if case == "fast":
            vc, vv = a.vclk.clone(), a.vval.clone()
        else:
            vc, vv = a.vclk.roll(1, 2).contiguous(), a.vval.roll(1, 2).contiguous()
        y = cg.map.MapStates(a.clock.clone(), a.ec.clone(), vc, vv, *reversed_live(*d, live))
        work = cg.map.MapStates(*[t.clone() for t in x])
        out.append(report("map_eq_batch", case, {"pairs": N, "K": K, "V": V, "A": A, "live_deferred": live},
                          tuple(x[:4]), tuple(y[:4]), lambda: cg.map.eq_batch(x, y, ctx=ctx),
                          lambda: cg.map.merge_batch(work, y, ctx=ctx), lambda: [w.copy_(s) for w, s in zip(work, x)]))
        del x, y, work, d, vc, vv
        torch.cuda.empty_cache()
    emit({"op": "map_eq_batch", "permuted_over_fast": out[1]["eq_us"]["median"] / out[0]["eq_us"]["median"]})


{"mvreg": mvreg, "orswot": orswot, "map": mapb}[args.only]()
