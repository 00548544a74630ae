"""Cost of the Map fold's deep pass (vstate = 17..64, csrc/map_deep.hip) at BASELINE config 4's shape
(16,384 replicas x 1,024 keys x 32 actors, 2 value slots per key, deferred removes) when a few keys
are written concurrently by all 32 actors: `--deep-keys` keys (default 8) are blanked in every replica
and then written once by each actor, in 32 replicas spread over the fold, with a counter above every
generated one, so each of them folds to 32 values.  Times the "map_fold" and "map_fold_deep" sections
of the same calls (vout = 4, so the first pass is the fast path; flags bit 0 is then expected), runs
one more call with vout = 32 and checks the deep keys plus a sample of the others against the oracle.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=16384)
ap.add_argument("--keys", type=int, default=1024)
ap.add_argument("--actors", type=int, default=32)
ap.add_argument("--slots", type=int, default=2)
ap.add_argument("--kmax", type=int, default=256)
ap.add_argument("--p-def", type=float, default=0.1)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--deep-keys", type=int, default=8)
ap.add_argument("--sample-keys", type=int, default=8)
ap.add_argument("--vstate", type=int, default=32)
args = ap.parse_args()

R, K, A, V = args.replicas, args.keys, args.actors, args.slots
SEED = 0x5EED0004
T0 = time.time()
assert R >= A and args.vstate >= A


def log(msg):
    print(f"[{time.time() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


torch.cuda.set_device(0)
ctx = cg.Context(0)
log(f"generating {R}x{K}x{A} V={V}")
inp = synth.map_replicas(ctx, R, K, A, V, SEED, kmax=args.kmax, p_def=args.p_def)
rng = np.random.default_rng(2)
deep = np.sort(rng.choice(K, size=args.deep_keys, replace=False))
others = np.sort(rng.choice(np.setdiff1d(np.arange(K), deep), size=min(args.sample_keys, K - len(deep)), replace=False))
tk = torch.from_numpy(deep).cuda()
C = args.kmax + 1  # above every generated counter: no generated clock dominates these writes
inp.ec[:, tk] = 0
inp.vclk[:, tk] = 0
inp.vval[:, tk] = 0
for a in range(A):
    r = a * (R // A) + (R // A) // 2
    inp.clock[r, a] = C
    inp.ec[r, tk, a] = C
    inp.vclk[r, tk, 0, a] = C
    inp.vval[r, tk, 0] = 1000 + a
torch.cuda.synchronize()
kw = dict(def_off=inp.def_off, def_row=inp.def_row, def_clock=inp.def_clock, def_keys=inp.def_keys, ctx=ctx,
          check=False)


def run(vout):
    return cg.map.lub_many(inp.clock, inp.ec, inp.vclk, inp.vval, vout=vout, vstate=args.vstate, **kw)


for _ in range(2):
    res = run(4)
torch.cuda.synchronize()
ctx.timing_reset()
ctx.set_timing(True)
t1 = time.perf_counter()
for _ in range(args.steps):
    res = run(4)
torch.cuda.synchronize()
wall = (time.perf_counter() - t1) / args.steps
fold_ms, n1 = ctx.timing("map_fold")
deep_ms, n2 = ctx.timing("map_fold_deep")
ctx.set_timing(False)
full = run(A)
torch.cuda.synchronize()

# ---- parity: the deep keys and a sample of the others vs the oracle, all replicas ----------------
import oracle as O  # noqa: E402  (checker only)

keys = np.sort(np.concatenate([deep, others]))
sk = torch.from_numpy(keys).cuda()
host = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
log(f"parity: oracle fold of keys {keys.tolist()} over all replicas")
peak = np.zeros(len(keys), np.uint64)
exp = O.map_fold(host(inp.clock), host(inp.ec[:, sk]), host(inp.vclk[:, sk]), host(inp.vval[:, sk]),
                 inp.def_row.cpu().numpy().astype(np.int64), host(inp.def_clock),
                 O.restrict_deferred_keys(host(inp.def_keys), keys), A, peak=peak)
is_deep = np.isin(keys, deep)
ok = bool(np.all(exp[4][is_deep] == A)) and bool(np.all(peak[~is_deep] <= 4))
ok = ok and int(np.bitwise_or.reduce(full.flags.cpu().numpy())) == 0
ok = ok and (np.array_equal(host(full.clock), exp[0]) and np.array_equal(host(full.ec)[keys], exp[1])
             and np.array_equal(host(full.vclk)[keys], exp[2]) and np.array_equal(host(full.vval)[keys], exp[3])
             and np.array_equal(full.nval.cpu().numpy()[keys], exp[4]))
# the timed calls (vout = 4): the same entry clocks and counts, the first 4 values of each key
ok = ok and (np.array_equal(host(res.ec)[keys], exp[1]) and np.array_equal(host(res.vclk)[keys], exp[2][:, :4])
             and np.array_equal(res.nval.cpu().numpy()[keys], exp[4]))
print(json.dumps({"workload": f"map<u32,mvreg<u64>> lub {R}x{K}x{A} V={V}, {len(deep)} keys with {A} concurrent values",
                  "deep_keys": deep.tolist(), "vstate": args.vstate, "wall_ms": wall * 1e3,
                  "map_fold_ms": fold_ms / max(n1, 1), "map_fold_deep_ms": deep_ms / max(n2, 1),
                  "deep_over_fold": (deep_ms / max(n2, 1)) / (fold_ms / max(n1, 1)),
                  "flags_vout4": int(np.bitwise_or.reduce(res.flags.cpu().numpy())),
                  "parity": "ok" if ok else "MISMATCH", "checked_keys": keys.tolist()}), flush=True)
sys.exit(0 if ok else 3)
