"""Re-index of resident states on one MI355X: crdt_mvreg_reindex, crdt_orswot_reindex, crdt_map_reindex.

Shapes of scripts/bench_eq.py: 1,048,576 MVReg registers (V = 4, A = 32), 8,192 config-3 Orswot states
(M = 4,096, A = 64), 8,192 config-4 Map states (K = 1,024, V = 2, A = 32), 4 live deferred slots of 8.
Cases: (i) "grow" pure growth (NULL maps; Dcap and V / M / K a quarter larger), (ii) "actors" two actors
inserted, one at the front and one in the middle, (iii) "ids" 64 members / keys interleaved, (iv) "both".
Reported per case: the call time by HIP events (20 launches after 5 warm-ups, median [min]); (bytes read
+ bytes written) / time as a share of 8 TB/s; a torch copy_ moving the same total bytes in the same
run; the torch statement of the same gather (zero_ + index_copy_ per tensor and axis, buffers allocated
outside the timing; the deferred bitmaps are only padded by words there, not gathered by bit, which
favours torch); with an actor map, the same call with the column gather reading 8-byte words straight
from memory (CRDT_TUNE rxlds=0) instead of rows staged in LDS; and the egress -> ingest round trip the
call replaces (wall time, it synchronises with the host twice).  Every output is compared with the numpy
gather on a sample of states.  One JSON line per case and one per type with the two expectations
(every case faster than the torch statement and than the round trip; pure growth within 10% of the
copy's time per byte) as met or not met, printed and appended to --log (default
profiles/reindex_bench.log).

Without --only every type runs in a child process of its own under a time limit, and the first failing
step stops the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["mvreg", "orswot", "map"], default=None)
ap.add_argument("--regs", type=int, default=1 << 20)
ap.add_argument("--states", type=int, default=8192)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=280)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "reindex_bench.log"))
args = ap.parse_args()

if args.only is None:
    for part in ("mvreg", "orswot", "map"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", part] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"bench_reindex: step {part} failed with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path[:0] = [os.path.join(ROOT, "rust-crdt_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import crdts_gpu as cg  # noqa: E402
import reindex_util as R  # noqa: E402  (the numpy statement of the gather)
from crdts_gpu import synth, wire  # noqa: E402

torch.cuda.set_device(0)
ctx = cg.Context(0)
DEV = torch.device("cuda", 0)
LOG = open(args.log, "a")


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def events(fn):
    """Call times by HIP events -> (median, min) in microseconds."""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us)


def wall(fn, n=5):
    """Wall time of a host-synchronous step -> (median, min) in microseconds."""
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us), min(us)


def nbytes(side):
    return sum(t.numel() * t.element_size() for t in side)


def insert(n_in, where):
    """`where`: the output positions of the new ids -> (src int32 device map or None, pos: new position of
    every old index, device int64, numpy src)."""
    if not len(where):
        return None, torch.arange(n_in, device=DEV), None
    n_out = n_in + len(where)
    src = np.full(n_out, -1, np.int64)
    old = np.setdiff1d(np.arange(n_out), np.asarray(where))
    src[old] = np.arange(n_in)
    return torch.from_numpy(src.astype(np.int32)).to(DEV), torch.from_numpy(old).to(DEV), src


def ids(n, dt):
    """An ascending dictionary of n ids."""
    return torch.arange(10, 10 + 3 * n, 3, dtype=dt, device=DEV)


def sub(d1, src):
    return d1 if src is None else d1[torch.from_numpy(src >= 0).to(DEV)].contiguous()


class TorchGather:
    """zero_ + index_copy_ per tensor and axis; specs[i] = [(dim, pos or None)] of the axes that change."""

    def __init__(self, xs, outs, specs):
        self.steps = []
        for x, out, spec in zip(xs, outs, specs):
            chain, cur = [], x
            for i, (dim, pos) in enumerate(spec):
                shape = list(cur.shape)
                shape[dim] = out.shape[dim]
                buf = torch.empty(shape, dtype=x.dtype, device=DEV) if i + 1 < len(spec) else torch.empty_like(out)
                n = min(cur.shape[dim], shape[dim])
                idx = pos if pos is not None else torch.arange(n, device=DEV)
                chain.append((buf, dim, idx, n if pos is None else cur.shape[dim]))
                cur = buf
            self.steps.append((x, out, chain))

    def __call__(self):
        for x, out, chain in self.steps:
            cur = x
            if not chain:
                out.copy_(x)
            for buf, dim, idx, n in chain:
                buf.zero_()
                buf.index_copy_(dim, idx, cur.narrow(dim, 0, n))
                cur = buf


def report(op, case, shape, xs, run, outs_of, specs, round_trip, parity, cols=False):
    out, status = run()
    outs = outs_of(out)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any(), "a benchmarked reindex reported a loss"
    parity(out)
    t = events(run)
    t_direct = None
    if cols:  # the column gather's other form: 8-byte words straight from memory instead of rows staged in LDS
        ctx.tune("rxlds=0")
        parity(run()[0])
        t_direct = events(run)
        ctx.tune("rxlds=1")
    b = nbytes(xs) + nbytes(outs)
    half = torch.empty(b // 16, dtype=torch.int64, device=DEV), torch.empty(b // 16, dtype=torch.int64, device=DEV)
    t_copy = events(lambda: half[1].copy_(half[0]))
    del half
    tg = TorchGather(xs, outs, specs)
    t_torch = events(tg)
    del tg
    torch.cuda.empty_cache()
    t_rt = wall(round_trip)
    torch.cuda.empty_cache()
    d = {"op": op, "case": case, **shape, "bytes_read_and_written": b,
         "reindex_us": {"median": t[0], "min": t[1]}, "GBs": b / t[0] / 1e3, "frac_of_8TBs": b / t[0] / 8e6,
         "copy_same_bytes_us": {"median": t_copy[0], "min": t_copy[1]}, "reindex_over_copy": t[0] / t_copy[0],
         "torch_statement_us": {"median": t_torch[0], "min": t_torch[1]}, "reindex_over_torch": t[0] / t_torch[0],
         "egress_ingest_us": {"median": t_rt[0], "min": t_rt[1]}, "reindex_over_round_trip": t[0] / t_rt[0],
         "parity": "numpy gather on sampled states: equal"}
    if t_direct:
        d["direct_gather_us"] = {"median": t_direct[0], "min": t_direct[1]}
        d["lds_over_direct"] = t[0] / t_direct[0]
    emit(d)
    DONE.append(d)
    return d


DONE = []


def expectations(op):
    grow = [d["reindex_over_copy"] for d in DONE if d["case"] == "grow"]
    emit({"op": op, "expectations": {
        "every case faster than the torch statement and the round trip":
            "met" if all(d["reindex_over_torch"] < 1 and d["reindex_over_round_trip"] < 1 for d in DONE) else "not met",
        "pure growth within 10% of the copy's time per byte": "met" if all(g <= 1.10 for g in grow) else "not met",
        "pure_growth_over_copy": grow}})


def sample(N):
    return sorted({0, 1, N // 2, N - 1})


def host(t, idx):
    return t[idx].cpu().numpy().view(np.uint64)


def deferred(N, Dcap, A, W, live, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    dc = torch.zeros((N, Dcap, A), dtype=torch.int64, device=DEV)
    ds = torch.zeros((N, Dcap, W), dtype=torch.int64, device=DEV)
    dc[:, :live] = torch.randint(1 << 20, 1 << 21, (N, live, A), generator=g, device=DEV, dtype=torch.int64)
    ds[:, :live] = torch.randint(0, 1 << 62, (N, live, W), generator=g, device=DEV, dtype=torch.int64)
    return dc, ds, torch.full((N,), live, dtype=torch.int32, device=DEV)


def pooled(st):
    cnt = st.def_count.to(torch.int64)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(cnt, 0)])
    live = torch.arange(st.def_clock.shape[1], device=DEV)[None, :] < cnt[:, None]
    return off, st.def_clock[live].contiguous(), st.def_members[live].contiguous()


def cases(A, n_ids, grow):
    """case -> (actor positions inserted, member / key positions inserted, grow the capacities)."""
    two = [0, (A + 2) // 2]
    inter = list(range(3, n_ids + 64, (n_ids + 64) // 64))[:64] if n_ids else []
    return {"grow": ([], [], True), "actors": (two, [], False), "ids": ([], inter, False), "both": (two, inter, False)}


def mvreg():
    N, V, A = args.regs, 4, 32
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    cnt = torch.randint(1, 256, (N, V, A), generator=g, device=DEV, dtype=torch.int64)
    keep = torch.rand((N, V, A), generator=g, device=DEV) < 3.0 / A
    keep[:, torch.arange(V), torch.arange(V) % A] = True  # no empty slot
    x = (cnt * keep, torch.randint(1, 1 << 62, (N, V), generator=g, device=DEV, dtype=torch.int64))
    del cnt, keep
    for case, (ins_a, _, grow) in cases(A, 0, True).items():
        if case in ("ids", "both"):
            continue  # a register has no member / key axis
        sa, pa, fa = insert(A, ins_a)
        V2 = V + 1 if grow else V
        d1 = ids(A + len(ins_a), torch.int32)
        d0 = sub(d1, fa)

        def parity(out):
            idx = sample(N)
            exp, _ = R.mvreg_reindex(dict(vclk=host(x[0], idx), vval=host(x[1], idx)), fa, A + len(ins_a), V2)
            assert np.array_equal(host(out[0], idx), exp["vclk"]) and np.array_equal(host(out[1], idx), exp["vval"])

        def round_trip():
            off, data = wire.mvreg_egress(*x, d0, ctx=ctx)
            wire.mvreg_ingest(data, off, d1, V2, ctx=ctx)

        report("mvreg_reindex", case, {"registers": N, "V": [V, V2], "A": [A, A + len(ins_a)]}, x,
               lambda: cg.mvreg.reindex(*x, sa, V=V2, ctx=ctx), lambda o: o,
               [[(2, pa if fa is not None else None)] * (fa is not None) + [(1, None)] * grow, [(1, None)] * grow],
               round_trip, parity, cols=fa is not None)


def orswot():
    N, M, A, Dcap = args.states, 4096, 64, 8
    a = synth.orswot_replicas(ctx, N, M, A, seed=0x5EED0003, kmax=48, p_def=0.2)
    x = cg.orswot.OrswotStates(a.clock, a.entries, *deferred(N, Dcap, A, (M + 63) // 64, 4, 2))
    for case, (ins_a, ins_m, grow) in cases(A, M, True).items():
        sa, pa, fa = insert(A, ins_a)
        sm, pm, fm = insert(M, ins_m)
        M2, A2, D2 = (M + M // 4 if grow else M + len(ins_m)), A + len(ins_a), (Dcap + 2 if grow else Dcap)
        a1, m1 = ids(A2, torch.int32), ids(M2, torch.int64)
        a0, m0 = sub(a1, fa), (sub(m1, fm) if not grow else m1[:M].contiguous())
        pool = pooled(x)

        def parity(out):
            idx = sample(N)
            st = dict(clock=host(x.clock, idx), entries=host(x.entries, idx), dcl=host(x.def_clock, idx),
                      dset=host(x.def_members, idx), cnt=x.def_count[idx].cpu().numpy())
            exp, _ = R.orswot_reindex(st, fa, fm, M2, A2, D2)
            got = dict(clock=host(out.clock, idx), entries=host(out.entries, idx), dcl=host(out.def_clock, idx),
                       dset=host(out.def_members, idx), cnt=out.def_count[idx].cpu().numpy())
            for k in exp:
                assert np.array_equal(got[k], exp[k]), k

        def round_trip():
            off, data = wire.orswot_egress(x.clock, x.entries, a0, m0, *pool, ctx=ctx)
            wire.orswot_ingest(data, off, a1, m1, def_cap=pool[1].shape[0], ctx=ctx)

        col = [(-1, pa)] if fa is not None else []
        row = [(1, pm)] if fm is not None else ([(1, None)] if grow else [])
        fix = lambda spec, nd: [(d % nd, p) for d, p in spec]  # noqa: E731
        report("orswot_reindex", case, {"states": N, "M": [M, M2], "A": [A, A2], "Dcap": [Dcap, D2], "live_deferred": 4},
               tuple(x[:4]), lambda: cg.orswot.reindex(x, sa, sm, M=M2, Dcap=D2, ctx=ctx), lambda o: tuple(o[:4]),
               [fix(col, 2), fix(row + col, 3), fix(([(1, None)] if grow else []) + col, 3),
                [(1, None)] * grow + [(2, None)] * (M2 != M)], round_trip, parity, cols=fa is not None)
        torch.cuda.empty_cache()


def mapb():
    N, K, A, V, Dcap = args.states, 1024, 32, 2, 8
    a = synth.map_replicas(ctx, N, K, A, V, 0x5EED0004, kmax=256, p_def=0.2)
    x = cg.map.MapStates(a.clock, a.ec, a.vclk, a.vval, *deferred(N, Dcap, A, (K + 63) // 64, 4, 3))
    for case, (ins_a, ins_k, grow) in cases(A, K, True).items():
        sa, pa, fa = insert(A, ins_a)
        sk, pk, fk = insert(K, ins_k)
        K2, A2 = (K + K // 4 if grow else K + len(ins_k)), A + len(ins_a)
        V2, D2 = (V + 1, Dcap + 2) if grow else (V, Dcap)
        a1, k1 = ids(A2, torch.int32), ids(K2, torch.int32)
        a0, k0 = sub(a1, fa), (sub(k1, fk) if not grow else k1[:K].contiguous())

        def parity(out):
            idx = sample(N)
            pick = lambda s: dict(clock=host(s.clock, idx), ec=host(s.ec, idx), vclk=host(s.vclk, idx),  # noqa: E731
                                  vval=host(s.vval, idx), dcl=host(s.def_clock, idx), dset=host(s.def_keys, idx),
                                  cnt=s.def_count[idx].cpu().numpy())
            exp, _ = R.map_reindex(pick(x), fa, fk, K2, V2, A2, D2)
            got = pick(out)
            for k in exp:
                assert np.array_equal(got[k], exp[k]), k

        def round_trip():
            off, data = wire.map_egress(x, a0, k0, ctx=ctx)
            wire.map_ingest(data, off, a1, k1, V2, D2, ctx=ctx)

        col = lambda d: [(d, pa)] if fa is not None else []  # noqa: E731
        row = [(1, pk)] if fk is not None else ([(1, None)] if grow else [])
        slot = [(2, None)] if grow else []
        report("map_reindex", case, {"states": N, "K": [K, K2], "V": [V, V2], "A": [A, A2], "Dcap": [Dcap, D2],
                                     "live_deferred": 4},
               tuple(x[:6]), lambda: cg.map.reindex(x, sa, sk, K=K2, V=V2, Dcap=D2, ctx=ctx), lambda o: tuple(o[:6]),
               [col(1), row + col(2), row + slot + col(3), row + slot, ([(1, None)] if grow else []) + col(2),
                [(1, None)] * grow + [(2, None)] * ((K2 + 63) // 64 != (K + 63) // 64)], round_trip, parity,
               cols=fa is not None)
        torch.cuda.empty_cache()


{"mvreg": mvreg, "orswot": orswot, "map": mapb}[args.only]()
expectations(args.only + "_reindex")
