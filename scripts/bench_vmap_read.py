"""The batched ReadCtx gathers of the value-typed Maps on one MI355X, against crdt_map_get:
  crdt_map_counter_get (PNCounter values), crdt_map_orswot_get / _contains, crdt_map_nested_get /
  _get_inner, at the shapes of scripts/bench_vmap_ops.py (65,536 states x 64 keys for the counter and
  Orswot Maps, 32,768 x 32 for the nested Map, A = 32), one query per (state, key), once in state
  order and once shuffled.  The yardstick is crdt_map_get on Map<K, MVReg> states of the same N, K, A
  and Q with V = 4, timed in the same process and alternated launch by launch with the new call.
HIP events around each launch of the C entry point (outputs allocated once), 5 warm-ups, the median
of 20.  Bytes per query are the words a query reads (the value only where the key is present) plus
the words it writes.  One JSON line per call and order; written to profiles/vmap_read_bench.log."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd")]
import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--states", type=int, default=65536)
ap.add_argument("--keys", type=int, default=64)
ap.add_argument("--nested-states", type=int, default=32768)
ap.add_argument("--nested-keys", type=int, default=32)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--members", type=int, default=8)
ap.add_argument("--inner-keys", type=int, default=8)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vmap_read_bench.log"))
args = ap.parse_args()
A, V = args.actors, 4
torch.cuda.set_device(0)
ctx = cg.Context(0)
dev = "cuda"
gen = torch.Generator(device=dev)
gen.manual_seed(0x5EED00B2)
lines = []


def rows(*shape, p=1.0):
    """u64 rows of small counters; a row is all zero with probability 1 - p."""
    x = torch.randint(1, 1 << 20, shape, dtype=torch.int64, device=dev, generator=gen)
    if p < 1.0:
        x *= (torch.rand(shape[:-1], device=dev, generator=gen) < p).unsqueeze(-1)
    return x


def out(*shape, dtype=torch.int64):
    return torch.empty(shape, dtype=dtype, device=dev)


def time_pair(yard, new):
    """Median launch time (us) of the two calls, alternated."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for _ in range(args.warmup):
        yard()
        new()
    torch.cuda.synchronize()
    t = ([], [])
    for _ in range(args.reps):
        for i, fn in enumerate((yard, new)):
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[i].append(a.elapsed_time(b) * 1e3)
    return float(np.median(t[0])), float(np.median(t[1]))


def emit(name, order, Q, us, bpq, yard_us, yard_bpq, extra):
    per_byte, yard_per_byte = us / (Q * bpq), yard_us / (Q * yard_bpq)
    rec = dict({"call": name, "order": order, "queries": Q, "actors": A, "us": round(us, 1),
                "queries_per_s": round(Q / us * 1e6), "bytes_per_query": round(bpq, 1),
                "GBs": round(Q * bpq / us / 1e3, 1), "map_get_us": round(yard_us, 1),
                "map_get_bytes_per_query": round(yard_bpq, 1), "map_get_GBs": round(Q * yard_bpq / yard_us / 1e3, 1),
                "time_per_query_vs_map_get": round(us / yard_us, 3),
                "time_per_byte_vs_map_get": round(per_byte / yard_per_byte, 3)}, **extra)
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def run(N, K, calls, extra):
    """calls: (name, fn(state_idx, key) -> launch closure, bytes per query)."""
    Q = N * K
    p = 0.7  # keys present
    # the yardstick's states: Map<K, MVReg>, V = 4, two values per present register
    ec = rows(N, K, A, p=p)
    live = (ec[..., :1] != 0).unsqueeze(2)
    vclk = rows(N, K, V, A) * live
    vclk[:, :, 2:] = 0
    vval = rows(N, K, V)
    ms = _abi.MapStates()
    ms.N, ms.K, ms.A, ms.V = N, K, A, V
    ms.clock, ms.clock_stride = rows(N, A).data_ptr(), A
    ms.ec, ms.ec_stride, ms.vclk, ms.vclk_stride = ec.data_ptr(), K * A, vclk.data_ptr(), K * V * A
    ms.vval, ms.vval_stride = vval.data_ptr(), K * V
    yo = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, V, A), out(Q, V), out(Q, dtype=torch.int32), out(Q, A),
          out(Q, dtype=torch.int32)]
    pf = float((ec[..., 0] != 0).float().mean())
    # reads: 2 indices, the ec row, the register where present; writes: every output
    yard_bpq = 8 + 8 * A + pf * (8 * V * A + 8 * V) + (1 + 8 * A + 8 * V * A + 8 * V + 4 + 8 * A + 4)
    s_lin = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(K)
    k_lin = torch.arange(K, dtype=torch.int32, device=dev).repeat(N)
    perm = torch.randperm(Q, device=dev, generator=gen)
    for order, (si, ki) in (("state order", (s_lin, k_lin)), ("shuffled", (s_lin[perm].contiguous(),
                                                                          k_lin[perm].contiguous()))):
        yard = lambda: ctx.call("crdt_map_get", ctypes.byref(ms), si.data_ptr(), ki.data_ptr(), Q,  # noqa: E731
                                *[t.data_ptr() for t in yo])
        for name, make, bpq in calls:
            fn = make(si, ki)
            yus, us = time_pair(yard, fn)
            emit(name, order, Q, us, bpq(pf), yus, yard_bpq, dict(extra, states=N, keys=K, present=round(pf, 3)))
    del ec, vclk, vval, yo


# ---- Map<K, PNCounter> -------------------------------------------------------------------------------
N, K, W = args.states, args.keys, 2
Q = N * K
c_ec = rows(N, K, A, p=0.7)
c_val = rows(N, K, W, A) * (c_ec[..., :1] != 0).unsqueeze(2)
c_clock = rows(N, A)
cs = _abi.MapCounterStates()
cs.N, cs.K, cs.A, cs.W = N, K, A, W
cs.clock, cs.clock_stride, cs.ec, cs.ec_stride = c_clock.data_ptr(), A, c_ec.data_ptr(), K * A
cs.val, cs.val_stride = c_val.data_ptr(), K * W * A
co = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, W, A), out(Q, 2), out(Q, dtype=torch.int32)]
run(N, K, [("crdt_map_counter_get", lambda si, ki: lambda: ctx.call(
    "crdt_map_counter_get", ctypes.byref(cs), si.data_ptr(), ki.data_ptr(), Q, *[t.data_ptr() for t in co]),
    lambda pf: 8 + 8 * A + pf * 8 * W * A + (1 + 8 * A + 8 * W * A + 16 + 4))], {"W": W})
del c_ec, c_val, co

# ---- Map<K, Orswot<M>> -----------------------------------------------------------------------------
M = args.members
Mw = (M + 63) // 64
o_ec = rows(N, K, A, p=0.7)
o_live = (o_ec[..., :1] != 0)
o_oc = rows(N, K, A) * o_live
o_ent = rows(N, K, M, A, p=0.5) * o_live.unsqueeze(2)
o_vdn = torch.zeros((N, K), dtype=torch.int32, device=dev)
os_ = _abi.MapOrswotStates()
os_.N, os_.K, os_.M, os_.A = N, K, M, A
os_.clock, os_.ec, os_.oc, os_.ent, os_.vd_n = (c_clock.data_ptr(), o_ec.data_ptr(), o_oc.data_ptr(),
                                                o_ent.data_ptr(), o_vdn.data_ptr())
oo = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, A), out(Q, Mw), out(Q, dtype=torch.int32),
      out(Q, dtype=torch.int32), out(Q, dtype=torch.int32)]
mem = torch.randint(0, M, (Q,), dtype=torch.int32, device=dev, generator=gen)
oc_ = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, A), out(Q, dtype=torch.int32)]
run(N, K, [
    ("crdt_map_orswot_get", lambda si, ki: lambda: ctx.call(
        "crdt_map_orswot_get", ctypes.byref(os_), si.data_ptr(), ki.data_ptr(), Q, *[t.data_ptr() for t in oo]),
     lambda pf: 8 + 8 * A + pf * (8 * A + 8 * M * A + 4) + (1 + 16 * A + 8 * Mw + 12)),
    ("crdt_map_orswot_contains", lambda si, ki: lambda: ctx.call(
        "crdt_map_orswot_contains", ctypes.byref(os_), si.data_ptr(), ki.data_ptr(), mem.data_ptr(), Q,
        *[t.data_ptr() for t in oc_]),
     lambda pf: 12 + 8 * A + pf * 16 * A + (1 + 16 * A + 4)),
], {"M": M})
del o_ec, o_oc, o_ent, oo, oc_, c_clock

# ---- Map<K, Map<K2, MVReg>> --------------------------------------------------------------------------
N, K, K2, Vs = args.nested_states, args.nested_keys, args.inner_keys, 8
Q = N * K
K2w = (K2 + 63) // 64
n_clock = rows(N, A)
n_ec = rows(N, K, A, p=0.7)
n_live = (n_ec[..., :1] != 0)
n_ic = rows(N, K, A) * n_live
n_iec = rows(N, K, K2, A, p=0.5) * n_live.unsqueeze(2)
n_nval = (torch.randint(1, 3, (N, K, K2), device=dev, generator=gen) * (n_iec[..., 0] != 0)).to(torch.int32)
n_ivc = rows(N, K, K2, Vs, A)
n_ivv = rows(N, K, K2, Vs)
nst = _abi.MapNestedStates()
nst.N, nst.K, nst.K2, nst.A, nst.Vs = N, K, K2, A, Vs
for nm, t_ in (("clock", n_clock), ("ec", n_ec), ("ic", n_ic), ("iec", n_iec), ("ivc", n_ivc), ("ivv", n_ivv),
               ("nval", n_nval)):
    setattr(nst, nm, t_.data_ptr())
no = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, A), out(Q, K2w), out(Q, dtype=torch.int32),
      out(Q, dtype=torch.int32)]
ik = torch.randint(0, K2, (Q,), dtype=torch.int32, device=dev, generator=gen)
ni = [out(Q, dtype=torch.uint8), out(Q, A), out(Q, A), out(Q, Vs, A), out(Q, Vs), out(Q, dtype=torch.int32), out(Q, A),
      out(Q, dtype=torch.int32)]
nv = 1.5 * 0.5  # values read per query under a present outer key: 1.5 per present inner key, half of them present
run(N, K, [
    ("crdt_map_nested_get", lambda si, ki: lambda: ctx.call(
        "crdt_map_nested_get", ctypes.byref(nst), si.data_ptr(), ki.data_ptr(), Q, *[t.data_ptr() for t in no]),
     lambda pf: 8 + 8 * A + pf * (8 * A + 8 * K2 * A) + (1 + 16 * A + 8 * K2w + 8)),
    ("crdt_map_nested_get_inner", lambda si, ki: lambda: ctx.call(
        "crdt_map_nested_get_inner", ctypes.byref(nst), si.data_ptr(), ki.data_ptr(), ik.data_ptr(), Q,
        *[t.data_ptr() for t in ni]),
     lambda pf: 12 + 8 * A + pf * (16 * A + 4 + nv * (8 * A + 8)) + (1 + 24 * A + 8 * Vs * A + 8 * Vs + 8)),
], {"K2": K2, "Vs": Vs})

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
