"""MVReg registers of 64 value slots on one MI355X, beside the same calls at 16 slots in the same run:
crdt_mvreg_merge_batch, _forget_batch, _eq_batch and _apply_batch over 65,536 registers of A = 32.

  merge   self V = 64 with 32 live values against other V = 32 (all live)   | self 16 with 8 live against other 8
  forget  V = 64, every slot live, a shared y that forgets about half the dots | V = 16
  ==      V = 64 against a bit-identical copy, and against the slots rolled by one | V = 16
  apply   V = 64 with 32 live values, 16 Puts a register, each dominating the Put before | V = 16 with 8 live

Each call: HIP events, 5 warm-ups, then 20 launches, median [min]; the registers are restored before
every launch, outside the events.  Reported as time per byte touched (self read and written, the other
side / y / the op clocks read).  forget and == are streams, merge and apply are compare-bound
(O(Vs * Vo) row tests).  One JSON line per call, printed and appended to --log (default
profiles/mvreg_wide_bench.log)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd"), os.path.join(ROOT, "oracle")]
import crdts_gpu as cg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regs", type=int, default=65536)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--puts", type=int, default=16)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mvreg_wide_bench.log"))
args = ap.parse_args()
N, A = args.regs, args.actors

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = "cuda"
LOG = open(args.log, "a")


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def events(fn, before):
    """Call times by HIP events -> (median, min) in microseconds."""
    for _ in range(args.warmup):
        before()
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.launches):
        before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us)


def registers(V, live, seed):
    """N registers of V slots, the first `live` occupied: about three dots a value, counters 1..255
    (so nearly every pair of values is concurrent)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    cnt = torch.randint(1, 256, (N, V, A), generator=g, device=DEV, dtype=torch.int64)
    keep = torch.rand((N, V, A), generator=g, device=DEV) < 3.0 / A
    keep[:, torch.arange(V), torch.arange(V) % A] = True  # no empty slot among the live ones
    keep[:, live:] = False
    vval = torch.randint(1, 1 << 62, (N, V), generator=g, device=DEV, dtype=torch.int64)
    vval[:, live:] = 0
    return cnt * keep, vval


def row(op, V, t, nbytes, **more):
    emit(dict({"op": op, "regs": N, "A": A, "V": V, "us": {"median": t[0], "min": t[1]}, "bytes_touched": nbytes,
               "ps_per_byte": t[0] * 1e6 / nbytes, "GBs": nbytes / t[0] / 1e3,
               "clock": "HIP events, registers restored before every launch"}, **more))
    return t[0] * 1e6 / nbytes


def words(*tensors):
    return sum(x.numel() for x in tensors) * 8


def run_merge(Vs, live, Vo, seed):
    s_c0, s_v0 = registers(Vs, live, seed)
    o_c, o_v = registers(Vo, Vo, seed + 1)
    s_c, s_v = s_c0.clone(), s_v0.clone()

    def reset():
        s_c.copy_(s_c0)
        s_v.copy_(s_v0)

    st = cg.mvreg.merge_batch(s_c, s_v, o_c, o_v, ctx=ctx)
    over = int((st != 0).sum().item())
    n_out = float(s_c.any(dim=2).sum(dim=1).float().mean().item())
    t = events(lambda: cg.mvreg.merge_batch(s_c, s_v, o_c, o_v, ctx=ctx), reset)
    return row("mvreg_merge", Vs, t, 2 * words(s_c, s_v) + words(o_c, o_v), other_V=Vo, live_self=live,
               mean_values_after=n_out, registers_over_capacity=over)


def run_forget(V, seed):
    c0, v0 = registers(V, V, seed)
    c, v = c0.clone(), v0.clone()
    y = torch.full((A,), 128, dtype=torch.int64, device=DEV)

    def reset():
        c.copy_(c0)
        v.copy_(v0)

    t = events(lambda: cg.mvreg.forget_batch(c, v, y, ctx=ctx), reset)
    return row("mvreg_forget", V, t, 2 * words(c, v), mean_values_after=float(c.any(dim=2).sum(dim=1).float().mean().item()))


def run_eq(V, seed):
    x_c, x_v = registers(V, V, seed)
    out = {}
    for name, (y_c, y_v) in {"identical": (x_c.clone(), x_v.clone()),
                             "rolled": (x_c.roll(1, dims=1).contiguous(), x_v.roll(1, dims=1).contiguous())}.items():
        ne = cg.mvreg.eq_batch(x_c, x_v, y_c, y_v, ctx=ctx)
        assert not ne.any().item(), "equal registers reported unequal"
        t = events(lambda: cg.mvreg.eq_batch(x_c, x_v, y_c, y_v, ctx=ctx), lambda: None)
        out[name] = row("mvreg_eq", V, t, words(x_c, x_v, y_c, y_v), y=name)
    return out


def run_apply(V, live, seed):
    T = args.puts
    c0, v0 = registers(V, live, seed)
    c, v = c0.clone(), v0.clone()
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 7)
    # every register's Puts advance four of its actors: each clock dominates the one before
    writers = torch.rand((N, 1, A), generator=g, device=DEV).argsort(dim=2) < 4
    inc = torch.randint(0, 4, (N, T, A), generator=g, device=DEV, dtype=torch.int64) * writers
    inc[:, :, 0] += writers[:, :, 0].long().expand(N, T)
    pool = torch.cat([inc.cumsum(dim=1).reshape(N * T, A).contiguous(), torch.zeros((1, A), dtype=torch.int64, device=DEV)])
    ops = cg.mvreg.MVRegOpBatch(torch.arange(0, N * T + 1, T, dtype=torch.int64, device=DEV),
                                torch.arange(N * T, dtype=torch.int32, device=DEV), pool,
                                torch.randint(1, 1 << 62, (N * T,), generator=g, device=DEV, dtype=torch.int64))

    def reset():
        c.copy_(c0)
        v.copy_(v0)

    st = cg.mvreg.apply_batch(c, v, ops, ctx=ctx)
    over = int((st != 0).sum().item())
    t = events(lambda: cg.mvreg.apply_batch(c, v, ops, ctx=ctx), reset)
    return row("mvreg_apply", V, t, 2 * words(c, v) + words(pool[:-1], ops.val), puts_per_reg=T, live=live,
               registers_with_status=over)


m64, m16 = run_merge(64, 32, 32, 1), run_merge(16, 8, 8, 3)
f64, f16 = run_forget(64, 5), run_forget(16, 6)
e64, e16 = run_eq(64, 7), run_eq(16, 8)
a64, a16 = run_apply(64, 32, 9), run_apply(16, 8, 10)
emit({"op": "mvreg_wide_summary", "ps_per_byte_V64_over_V16": {
    "merge": m64 / m16, "forget": f64 / f16, "eq_identical": e64["identical"] / e16["identical"],
    "eq_rolled": e64["rolled"] / e16["rolled"], "apply": a64 / a16}})
