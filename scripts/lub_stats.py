#!/usr/bin/env python3
"""Where the blocks of the fused lattice lub ran and when (-DLUB_STATS build of csrc/lattice.hip).

    scripts/build_variant.sh stats lattice.hip -DLUB_STATS
    CRDT_GPU_LIB=rust-crdt_amd/libcrdt_gpu_stats.so python3 scripts/lub_stats.py [--tune lubpg=512]

Runs bench.py's step (GCounter R x A + PNCounter R x 2A in one crdt_lub_many_multi launch) a few
times; the instrumented library writes one record per block of the last launch (workgroup, segment,
wall_clock64 at entry / exit, HW_ID and XCC_ID of the CU).  Printed: how the blocks of the segments
were paired on the CUs, the first / median / last exit per segment, and the share of the launch
during which fewer than cu_count CUs held a block.  The stats build is never the timed build."""
import argparse
import collections
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-crdt_amd"))

TICK_US = 0.01  # wall_clock64(): 100 MHz


def parse_records(path):
    head, recs = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("# grid"):
                w = line.split()
                head = {w[i]: int(w[i + 1]) for i in range(1, len(w) - 1, 2)}
            elif not line.startswith("#"):
                b, seg, wg, t0, t1, xcc, hw = (int(x) for x in line.split())
                # HW_ID (gfx9): cu_id 11:8, sh_id 12, se_id 15:13 -> one key per CU of an XCC
                recs.append(dict(block=b, seg=seg, wg=wg, t0=t0, t1=t1, cu=(xcc, (hw >> 8) & 0xFF)))
    return head, recs


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def report(head, recs, names, out=sys.stdout):
    p = lambda *a: print(*a, file=out)  # noqa: E731
    start = min(r["t0"] for r in recs)
    end = max(r["t1"] for r in recs)
    span = end - start
    cu_count = head.get("cu_count", 0)
    p(f"launch: grid {head.get('grid')} workgroups, {len(recs)} blocks, {head.get('segments')} segments, "
      f"{span * TICK_US:.1f} us from first entry to last exit, {cu_count} CUs")
    by_cu = collections.defaultdict(list)
    for r in recs:
        by_cu[r["cu"]].append(r)
    p(f"CUs that ran a block: {len(by_cu)}")
    comp = collections.Counter()
    overlap = 0
    for rs in by_cu.values():
        rs.sort(key=lambda r: r["t0"])
        comp["+".join(sorted(names[r["seg"]] for r in rs))] += 1
        if any(a["t1"] > b["t0"] for a, b in zip(rs, rs[1:])):
            overlap += 1
    for k, n in sorted(comp.items()):
        p(f"  CUs holding {k}: {n}")
    p(f"  CUs on which two blocks ran at the same time: {overlap}")
    for s in sorted({r["seg"] for r in recs}):
        ex = [(r["t1"] - start) * TICK_US for r in recs if r["seg"] == s]
        en = [(r["t0"] - start) * TICK_US for r in recs if r["seg"] == s]
        p(f"segment {s} ({names[s]}): {len(ex)} blocks, entry first {min(en):.1f} / median {median(en):.1f} / last "
          f"{max(en):.1f} us, exit first {min(ex):.1f} / median {median(ex):.1f} / last {max(ex):.1f} us")
    last_seg = max(r["seg"] for r in recs)
    ex = [(r["t1"] - start) * TICK_US for r in recs if r["seg"] == last_seg]
    p(f"last segment: median exit {median(ex):.1f} us, last exit {max(ex):.1f} us: the last trails the median by "
      f"{(max(ex) - median(ex)) / (span * TICK_US) * 100:.2f}% of the launch")
    # busy CUs over time: +1 when a CU's first running block enters, -1 when its last one exits
    ev = []
    for rs in by_cu.values():
        cur_s, cur_e = rs[0]["t0"], rs[0]["t1"]
        for r in rs[1:]:
            if r["t0"] <= cur_e:
                cur_e = max(cur_e, r["t1"])
            else:
                ev += [(cur_s, 1), (cur_e, -1)]
                cur_s, cur_e = r["t0"], r["t1"]
        ev += [(cur_s, 1), (cur_e, -1)]
    ev.sort()
    busy, last_t, short = 0, start, 0
    full = cu_count or len(by_cu)
    for t, d in ev:
        if busy < full:
            short += t - last_t
        busy += d
        last_t = t
    p(f"fewer than {full} CUs busy during {short / span * 100:.2f}% of the launch ({short * TICK_US:.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1 << 20)
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tune", default="", help="CRDT_TUNE spec for the run, e.g. lubpg=512")
    ap.add_argument("--records", default=None, help="keep the raw per-block records in this file")
    args = ap.parse_args()
    path = args.records or os.path.join(tempfile.mkdtemp(), "lub_stats.txt")
    os.environ["LUB_STATS_OUT"] = path

    import torch

    import crdts_gpu as cg

    torch.cuda.set_device(0)
    ctx = cg.Context.default(0)
    if args.tune:
        ctx.tune(args.tune)
    R, A = args.replicas, args.actors
    g = torch.empty((R, A), dtype=torch.int64, device="cuda")
    pn = torch.empty((R, 2 * A), dtype=torch.int64, device="cuda")
    cg.synth_fill(ctx, g, 0x5EED0002, 0)
    cg.synth_fill(ctx, pn, 0x5EED0003, 0)
    items = [("gcounter", g, torch.empty(A, dtype=torch.int64, device="cuda")),
             ("pncounter", pn, torch.empty(2 * A, dtype=torch.int64, device="cuda"))]
    for _ in range(args.warmup + 1):
        cg.lub_many_multi(items, ctx=ctx)
    torch.cuda.synchronize()
    if not os.path.exists(path):
        sys.exit("lub_stats.py: no records written: CRDT_GPU_LIB must name a -DLUB_STATS build of lattice.hip")
    head, recs = parse_records(path)
    print(f"library: {os.path.relpath(os.environ.get('CRDT_GPU_LIB', 'rust-crdt_amd/libcrdt_gpu.so'), ROOT)}  tune: {args.tune or '(default)'}  "
          f"GCounter {R} x {A} + PNCounter {R} x {2 * A}")
    report(head, recs, {0: "G", 1: "PN"})


if __name__ == "__main__":
    main()
