"""GPU: the capacity cut of the sized op-stream ingests at a width the other cut tests do not reach:
N = 1,100 states, so the finalize kernel (one thread per state, 256 a workgroup) spans five workgroups
and the exclusive scans two scan blocks (1,024 items each).  One representative of every family:
Orswot ops (three counted quantities), PNCounter-Map ops (three of four), Orswot-Map ops (four),
MVReg Puts and VClock dots (one).  Every state adds to every quantity its family counts, so any
state can be the cut; each capacity in turn binds, with the cut state once in [256, 512) and once in
[1,024, 1,100).  Expected values come from the host encoders and numpy alone.  Exact integer equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lattice_ops_util as L
import oracle as O
import test_gpu_wire_ops as TO
import test_gpu_wire_vmap_ops as TV
import wire_mvreg_util as WM
import wire_ops_util as W
import wire_vmap_ops_util as V
from orswot_apply_util import random_ops

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

DEV = "cuda:0"
N = 1100
CUT_STATES = (300, 1060)  # past one finalize workgroup; past one scan block
CANARY = TO.CANARY
A, M, K = 5, 40, 30
host = TO.host


def mixed(rng, must, extra):
    """The ops every state must carry plus up to 3 - len(must) of `extra(n)`, in a random order."""
    ops = list(must) + extra(int(rng.integers(0, 4 - len(must))))
    return [ops[i] for i in rng.permutation(len(ops))]


def one_clock(rng):
    return O.VClock({int(rng.integers(A)): int(rng.integers(1, 9))})


def every_state_adds(offsets):
    """The property the cuts rest on: every state adds to every counted quantity."""
    for nm, off in offsets.items():
        assert len(off) == N + 1 and off[0] == 0 and (np.diff(off) > 0).all(), nm


def check_cut(got, st, offsets, cut):
    """status, and every offset array: the host's cumulative sums up to the cut, its value there after."""
    assert not st[:cut].any() and (st[cut:] == wire.CAP).all()
    for nm, w in offsets.items():
        assert got[nm][:cut + 1].tolist() == w[:cut + 1].tolist() and (got[nm][cut + 1:N + 1] == w[cut]).all(), nm


def binding(offsets, which, cut):
    """Capacities = the totals, but `which` ends one short of state `cut`'s end."""
    caps = {nm: int(off[-1]) for nm, off in offsets.items()}
    caps[which] = int(offsets[which][cut + 1]) - 1
    assert caps[which] >= offsets[which][cut]
    return caps


# ---- Orswot ops: ops, rows, ids --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def orswot_case():
    rng = np.random.default_rng(1)
    streams = [mixed(rng, [O.OrswotRm(one_clock(rng), [int(rng.integers(M))])], lambda n: random_ops(rng, n, M, A, 8))
               for _ in range(N)]
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    ref = TO.orswot_ref(streams, A)
    op_off, kind, mem_off = host(ref.op_off), host(ref.kind), host(ref.mem_off)
    rows = np.concatenate([[0], np.cumsum(kind)]).astype(np.int64)
    offsets = {"op_off": op_off, "row_off": rows[op_off], "id_off": mem_off[op_off]}
    data, off = W.pack_frames([W.enc_orswot_frame(s, aid, mid) for s in streams])
    return data, off, aid, mid, {nm: host(t) for nm, t in zip(ref._fields, ref)}, offsets


@pytest.mark.parametrize("cut", CUT_STATES)
@pytest.mark.parametrize("which", ["op_off", "row_off", "id_off"])
def test_orswot_ops(gpu_ctx, which, cut):
    data, off, aid, mid, ref, offsets = orswot_case()
    every_state_adds(offsets)
    data, off, actors, members = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV), TO.d32(aid), TO.d64(mid)
    totals, st = TO.raw_ingest(gpu_ctx, False, data, off, actors, members, None, sizing=True)
    assert totals == tuple(int(o[-1]) for o in offsets.values()) and not host(st).any()
    caps = binding(offsets, which, cut)
    got, st = TO.raw_ingest(gpu_ctx, False, data, off, actors, members, list(caps.values()))
    check_cut(got, st, offsets, cut)
    n, r, i = (int(o[cut]) for o in offsets.values())
    for k, nm in dict(kind="kind", actor="actor", counter="counter", row="rm_row").items():
        assert np.array_equal(got[k][:n], ref[nm][:n]), nm
    assert np.array_equal(got["pool"][:r * A], ref["rm_clock"].reshape(-1)[:r * A])
    assert np.array_equal(got["ids_off"][:n + 1], ref["mem_off"][:n + 1])
    assert np.array_equal(got["ids"][:i], ref["mem"][:i])
    co, cr, ci = caps.values()
    for k, cap in (("kind", co), ("actor", co), ("counter", co), ("row", co), ("pool", cr * A), ("ids_off", co + 1),
                   ("ids", ci), ("op_off", N + 1), ("row_off", N + 1), ("id_off", N + 1)):
        assert (got[k][cap:] == CANARY).all(), k


# ---- the value-typed Maps: ops, rows, keys (PNCounter), and members (Orswot) -------------------------
@functools.lru_cache(maxsize=None)
def vmap_case(kind):
    rng = np.random.default_rng(2 + V.KINDS.index(kind))
    key_rm = lambda: O.MapRm(one_clock(rng), {int(rng.integers(K))})  # noqa: E731  (an op, a row, a key)
    mem_rm = lambda: O.MapUp(O.Dot(int(rng.integers(A)), int(rng.integers(1, 9))), int(rng.integers(K)),  # noqa: E731
                             O.OrswotRm(one_clock(rng), [int(rng.integers(M))]))  # (an op, a row, a member)
    must = (lambda: [key_rm(), mem_rm()]) if kind == "orswot" else (lambda: [key_rm()])
    U = M if kind == "orswot" else 0
    streams = [mixed(rng, must(), lambda n: V.random_ops(kind, rng, n, A, K, U)) for _ in range(N)]
    c = TV.make_case(kind, rng, streams, A, K, U)
    want = TV.ref(c)
    firsts, totals = TV.layout(kind, want)
    offsets = dict(zip(("op_off", "row_off", "key_first", "mem_first"), firsts))
    if kind != "orswot":
        assert not offsets.pop("mem_first").any()
    data, off = V.pack_frames(TV.enc_frames(c))
    return c, data, off, {nm: host(t).reshape(-1) for nm, t in zip(want._fields, want)}, offsets, totals


VMAP_CUTS = [("pn", w) for w in ("op_off", "row_off", "key_first")] + \
            [("orswot", w) for w in ("op_off", "row_off", "key_first", "mem_first")]


@pytest.mark.parametrize("cut", CUT_STATES)
@pytest.mark.parametrize("kind,which", VMAP_CUTS)
def test_vmap_ops(gpu_ctx, kind, which, cut):
    c, data, off, want, offsets, totals = vmap_case(kind)
    every_state_adds(offsets)
    data, off = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)
    got_totals, st = TV.raw_ingest(gpu_ctx, c, data, off, None, sizing=True)
    assert got_totals == totals and not st.any()
    caps = binding(offsets, which, cut)
    got, st, sizes = TV.raw_ingest(gpu_ctx, c, data, off, list(caps.values()) + [0] * (4 - len(caps)))
    check_cut(got, st, offsets, cut)
    n, r, k = (int(offsets[nm][cut]) for nm in ("op_off", "row_off", "key_first"))
    m = int(offsets["mem_first"][cut]) if kind == "orswot" else 0
    upto = dict(op_off=cut + 1, clk_pool=r * A, key_off=n + 1, keys=k, mem_off=n + 1, mems=m)
    for nm, w in want.items():
        cnt = upto.get(nm, n)
        assert np.array_equal(got[nm][:cnt], w[:cnt]), nm
    for nm, a in got.items():
        assert (a[sizes[nm]:] == CANARY).all() and len(a) == sizes[nm] + 4, nm


# ---- MVReg Puts: ops and rows are one number, the smaller capacity binds -------------------------------
@functools.lru_cache(maxsize=None)
def mvreg_case():
    rng = np.random.default_rng(7)
    streams = [[O.MVRegPut(one_clock(rng), int(rng.integers(1, 1 << 60))) for _ in range(int(rng.integers(1, 4)))]
               for _ in range(N)]
    aid = WM.sparse_dict(rng, A, 32)
    want = cg.mvreg.encode_ops([[(dict(op.clock.dots), op.val) for op in s] for s in streams], A, DEV)
    op_off = host(want.op_off)
    assert np.array_equal(op_off, np.cumsum([0] + [len(s) for s in streams]))
    data, off = WM.pack_frames([WM.enc_ops(s, aid) for s in streams])
    return data, off, aid, host(want.clk_pool).reshape(-1), host(want.val), op_off


@pytest.mark.parametrize("cut", CUT_STATES)
@pytest.mark.parametrize("which", ["ops", "rows"])
def test_mvreg_puts(gpu_ctx, which, cut):
    data, off, aid, pool, val, op_off = mvreg_case()
    every_state_adds({"op_off": op_off})
    data, off, actors = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV), TO.d32(aid)
    head = (dptr(data), dptr(off), N, dptr(actors), A)
    status = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    tot = (ctypes.c_uint64 * 2)()
    gpu_ctx.call("crdt_mvreg_ops_ingest", *head, None, dptr(status), tot)
    n_ops = int(op_off[-1])
    assert (int(tot[0]), int(tot[1])) == (n_ops, n_ops) and not host(status).any()
    cap = binding({"op_off": op_off}, "op_off", cut)["op_off"]
    op_cap, row_cap = (cap, n_ops) if which == "ops" else (n_ops, cap)
    mk = lambda cnt, dt: torch.full((cnt + 4,), CANARY, dtype=dt, device=DEV)  # noqa: E731
    bufs = dict(op_off=mk(N + 1, torch.int64), clk_row=mk(op_cap, torch.int32), clk_pool=mk(row_cap * A, torch.int64),
                val=mk(op_cap, torch.int64))
    b = _abi.MVRegOpsBuf(op_cap, dptr(bufs["op_off"]), dptr(bufs["clk_row"]), dptr(bufs["clk_pool"]), row_cap,
                         dptr(bufs["val"]))
    gpu_ctx.call("crdt_mvreg_ops_ingest", *head, ctypes.byref(b), dptr(status), None)
    got = {nm: host(t) for nm, t in bufs.items()}
    check_cut(got, host(status), {"op_off": op_off}, cut)
    kept = int(op_off[cut])
    assert np.array_equal(got["clk_row"][:kept], np.arange(kept))
    assert np.array_equal(got["clk_pool"][:kept * A], pool[:kept * A]) and np.array_equal(got["val"][:kept], val[:kept])
    # nothing past the ops kept, and so nothing past a capacity
    for nm, cnt in (("op_off", N + 1), ("clk_row", kept), ("clk_pool", kept * A), ("val", kept)):
        assert (got[nm][cnt:] == CANARY).all(), nm


# ---- VClock dots: one capacity ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vclock_case():
    rng = np.random.default_rng(9)
    streams = [[O.Dot(int(rng.integers(A)), int(rng.integers(1, 1 << 40))) for _ in range(int(rng.integers(1, 4)))]
               for _ in range(N)]
    ids = L.sparse_dict(rng, A, 32)
    data, off = L.pack_frames([L.enc_frame("vclock", s, ids) for s in streams])
    return data, off, ids, L.Dense("vclock", streams)


@pytest.mark.parametrize("cut", CUT_STATES)
def test_vclock_dots(gpu_ctx, cut):
    data, off, ids, d = vclock_case()
    every_state_adds({"op_off": d.op_off})
    data, off, actors = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV), TO.d32(ids)
    head = (dptr(data), dptr(off), N, dptr(actors), A)
    status = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    tot = (ctypes.c_uint64 * 1)()
    gpu_ctx.call("crdt_vclock_ops_ingest", *head, None, dptr(status), tot)
    assert int(tot[0]) == d.n and not host(status).any()
    cap = binding({"op_off": d.op_off}, "op_off", cut)["op_off"]
    mk = lambda cnt, dt: torch.full((cnt + 4,), CANARY, dtype=dt, device=DEV)  # noqa: E731
    bufs = dict(op_off=mk(N + 1, torch.int64), state_idx=mk(cap, torch.int32), actor=mk(cap, torch.int32),
                counter=mk(cap, torch.int64))
    b = _abi.DotOpsBuf(cap, dptr(bufs["op_off"]), dptr(bufs["state_idx"]), dptr(bufs["actor"]), dptr(bufs["counter"]),
                       None)
    gpu_ctx.call("crdt_vclock_ops_ingest", *head, ctypes.byref(b), dptr(status), None)
    got = {nm: host(t) for nm, t in bufs.items()}
    check_cut(got, host(status), {"op_off": d.op_off}, cut)
    kept = int(d.op_off[cut])
    assert np.array_equal(got["state_idx"][:kept].view(np.uint32), d.state_idx[:kept])
    assert np.array_equal(got["actor"][:kept].view(np.uint32), d.actor[:kept])
    assert np.array_equal(got["counter"][:kept].view(np.uint64), d.counter[:kept])
    for nm, cnt in (("op_off", N + 1), ("state_idx", kept), ("actor", kept), ("counter", kept)):
        assert (got[nm][cnt:] == CANARY).all(), nm
