"""Presence scan (crdt_orswot_read / crdt_map_read) on one MI355X against two yardsticks from the
same run on the same box:

  scan    crdt_orswot_read on packed entries 2,048 states x 4,096 members x 64 actors (4 GiB), and
          crdt_map_read at config 4's ec shape, 16,384 x 1,024 x 32 (4 GiB)
  (a)     the torch expression a caller would write without it: (entries != 0).any(-1), packed
          into 64-bit words, plus the per-state count
  (b)     lattice.hip's fold stream on a 4 GiB input (PNCounter lub_many of 1,048,576 x 512, config
          2's second fold): the read-stream rate the library achieves

All three read the same 4 GiB buffer, far past the 256 MiB last-level cache.  Every launch is
timed by its own pair of HIP events after `--warmup` launches; min and median over `--launches`.
Bytes are the algorithm's: the input once plus the outputs.  The scan's words and counts are compared
with (a)'s on the device.  `--sweep` alternates the launch-geometry knobs (CRDT_TUNE rdbpc / rdu /
rdnt) in the same run.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd")]
import crdts_gpu as cg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scale", type=int, default=1, help="divide the state / replica counts (smoke runs)")
ap.add_argument("--sweep", nargs="?", const="rdbpc=1;rdbpc=2;rdbpc=8;rdbpc=32;rdu=4;rdnt=0", default="",
                help="also time the scan under other launch geometries: ';'-separated CRDT_TUNE specs")
args = ap.parse_args()
assert args.launches >= 1 and torch.cuda.is_available(), "needs an MI355X"

torch.cuda.set_device(0)
ctx = cg.Context(0)
N, M, A = 2048 // args.scale, 4096, 64            # Orswot entries
R4, K4, A4 = 16384 // args.scale, 1024, 32        # config 4's ec
RL, WL = (1 << 20) // args.scale, 512             # config 2's PNCounter rows
words = N * M * A
assert words == R4 * K4 * A4 == RL * WL
buf = torch.empty(words, dtype=torch.int64, device="cuda")
cg.synth_fill(ctx, buf.view(RL, WL), 0x5EED00AD, 0)
# about half of the 32-word rows absent (so are a quarter of the 64-word ones)
gone = torch.rand(words // 32, device="cuda") < 0.5
buf.view(-1, 32)[gone] = 0
del gone
torch.cuda.synchronize()


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)


def report(what, ms, nbytes, **kw):
    mn, md = ms[0], statistics.median(ms)
    d = dict(what=what, launches=len(ms), min_ms=round(mn, 4), median_ms=round(md, 4), bytes=nbytes,
             min_TBs=round(nbytes / mn / 1e9, 3), median_TBs=round(nbytes / md / 1e9, 3),
             median_frac_of_8TBs=round(nbytes / md / 8e9, 4), **kw)
    print(json.dumps(d), flush=True)
    return md


def torch_scan(x):
    """(a): presence per row, packed 64 rows to a word, and the count per state."""
    n, m, _ = x.shape
    b = (x != 0).any(-1)
    sh = torch.arange(64, device=x.device, dtype=torch.int64)
    pad = (-m) % 64
    bp = torch.nn.functional.pad(b, (0, pad)) if pad else b
    return (bp.view(n, -1, 64).to(torch.int64) << sh).sum(-1), b.sum(-1, dtype=torch.int32)


def scan_case(name, fn, x, tune=""):
    n, m, a = x.shape
    clock = torch.zeros((n, a), dtype=torch.int64, device="cuda")
    if tune:
        ctx.tune(tune)
    out = {}
    ctx.timing_reset()
    ctx.set_timing(True)
    ms = timed(lambda: out.__setitem__("v", fn(clock, x, ctx=ctx)))
    lib_ms, lib_n = ctx.timing("read_scan")
    ctx.set_timing(False)
    nbytes = x.numel() * 8 + n * ((m + 63) // 64) * 8 + n * 4
    bits, cnt = out["v"].val
    want_bits, want_cnt = torch_scan(x)
    ok = bool(torch.equal(bits, want_bits) and torch.equal(cnt, want_cnt))
    md = report(name, ms, nbytes, shape=[n, m, a], tune=tune or "default", parity="ok" if ok else "MISMATCH",
                present_frac=round(float(want_cnt.sum()) / (n * m), 4),
                ctx_timing_mean_ms=round(lib_ms / max(lib_n, 1), 4))
    return md, ok


DEFAULT_TUNE = "rdbpc=0,rdu=8,rdnt=1"  # csrc/common.hpp Tune::read_*
entries = buf.view(N, M, A)
ec = buf.view(R4, K4, A4)
ok = True
t_scan, o = scan_case("crdt_orswot_read", cg.orswot.read, entries)
ok &= o
t_map, o = scan_case("crdt_map_read (config 4 ec)", cg.map.read, ec)
ok &= o
t_torch = report("(a) torch (entries != 0).any(-1) packed + count", timed(lambda: torch_scan(entries)),
                 words * 8 + N * (M // 64) * 8 + N * 4, shape=[N, M, A])
t_torch4 = report("(a) torch, config 4 ec", timed(lambda: torch_scan(ec)), words * 8 + R4 * (K4 // 64) * 8 + R4 * 4,
                  shape=[R4, K4, A4])
rows = buf.view(RL, WL)
acc = torch.empty(WL, dtype=torch.int64, device="cuda")
t_fold = report("(b) lattice fold stream: pncounter.lub_many 4 GiB", timed(lambda: cg.pncounter.lub_many(rows, out=acc, ctx=ctx)),
                words * 8 + WL * 8, shape=[RL, WL])
print(json.dumps(dict(summary="scan vs yardsticks (median ms)", orswot_read=round(t_scan, 4), map_read=round(t_map, 4),
                      torch_a=round(t_torch, 4), torch_a_c4=round(t_torch4, 4), fold_b=round(t_fold, 4),
                      scan_over_torch=round(t_scan / t_torch, 4), scan_over_fold=round(t_scan / t_fold, 4),
                      map_over_fold=round(t_map / t_fold, 4))), flush=True)
if args.sweep:
    for tune in args.sweep.split(";"):
        _, o = scan_case("crdt_orswot_read", cg.orswot.read, entries, tune=tune)
        ok &= o
        _, o = scan_case("crdt_map_read (config 4 ec)", cg.map.read, ec, tune=tune)
        ok &= o
        ctx.tune(DEFAULT_TUNE)
    # the default again, last: the spread of the same code within this run
    scan_case("crdt_orswot_read (repeat)", cg.orswot.read, entries)
sys.exit(0 if ok and t_scan <= t_torch and t_map <= t_torch4 else 3)
