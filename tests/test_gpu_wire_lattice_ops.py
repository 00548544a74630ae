"""The lattice types' op streams on the wire (csrc/wire_lattice_ops.hip) against the test-side codec
(tests/lattice_ops_util.py) and the oracle: Vec<Dot<u32>> (VClock / GCounter), Vec<pncounter::Op<u32>>,
Vec<u64> (GSet) and Vec<LWWReg<u64, u64>> frames, N = 200 per batch through sparse dictionaries; the
sizing / synchronising / no-sync modes, the prefix cut, the refusals with their neighbours intact,
and one frames -> ingest -> apply_batch -> state egress loop per type."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import lattice_ops_util as L
import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, apply, lwwreg, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

N = 200
U = 300
BAD, MISSING, CAP = 1, 2, 4
NONE = 0xFFFFFFFF
CASES = [("vclock", 5), ("vclock", 200), ("pncounter", 5), ("pncounter", 200), ("gset", U), ("lwwreg", 0)]
DICT_CASES = [c for c in CASES if c[0] != "lwwreg"]
_CACHE = {}


def counts():
    rng = np.random.default_rng(3)
    n = [int(x) for x in rng.integers(0, 71, size=N)]
    n[0] = n[N - 1] = 0
    n[1:6] = [1, 63, 64, 65, 70]
    for i, k in ((7, 5), (66, 64), (100, 20), (120, 3), (121, 2), (150, 9), (151, 4), (180, 66), (190, 2)):
        n[i] = k  # the frames the refusal and prefix-cut tests rewrite
    return n


def gen_op(kind, rng, D):
    if kind == "lwwreg":
        return (int(rng.integers(0, 3)), int(rng.integers(0, 8)))
    if kind == "gset":
        return int(rng.integers(0, D))
    dot = O.Dot(int(rng.integers(0, D)), int(rng.integers(1, 1 << 40)))
    return dot if kind == "vclock" else (dot, (O.PNCounter.POS, O.PNCounter.NEG)[int(rng.integers(0, 2))])


def case(kind, D):
    """-> (ids, streams, frames, dense): the dictionary, per-state ops, their frames, the dense batch."""
    if (kind, D) not in _CACHE:
        rng = np.random.default_rng(100 + D + len(kind))
        ids = None if kind == "lwwreg" else L.sparse_dict(rng, D, 64 if kind == "gset" else 32)
        streams = [[gen_op(kind, rng, D) for _ in range(n)] for n in counts()]
        frames = [L.enc_frame(kind, s, ids) for s in streams]
        _CACHE[(kind, D)] = (ids, streams, frames, L.Dense(kind, streams))
    return _CACHE[(kind, D)]


def dev_frames(frames):
    data, off = L.pack_frames(frames)
    return torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")


def dev_dict(kind, ids):
    if kind == "gset":
        return to_dev(np.asarray(ids, np.uint64))
    return torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to("cuda:0")


def ingest(kind, data, off, ids, **kw):
    if kind == "lwwreg":
        return wire.lwwreg_ops_ingest(data, off, **kw)
    return getattr(wire, f"{kind}_ops_ingest")(data, off, dev_dict(kind, ids), **kw)


def egress(kind, ops, ids):
    if kind == "lwwreg":
        return wire.lwwreg_ops_egress(ops)
    return getattr(wire, f"{kind}_ops_egress")(ops, dev_dict(kind, ids))


def u32(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def same_batch(kind, ops, d, n=None):
    """The first n (default: all) ops of the ingested batch are the dense batch's."""
    n = d.n if n is None else n
    if kind == "lwwreg":
        assert np.array_equal(to_host(ops.marker)[:n], d.marker[:n]) and np.array_equal(to_host(ops.val)[:n], d.val[:n])
        return
    assert np.array_equal(u32(ops.state_idx)[:n], d.state_idx[:n])
    assert np.array_equal(u32(ops.actor)[:n], d.actor[:n])
    if kind != "gset":
        assert np.array_equal(to_host(ops.counter)[:n], d.counter[:n])
    if kind == "pncounter":
        assert np.array_equal(ops.dir.cpu().numpy()[:n], d.dir[:n])


def dense_dev(kind, d):
    """The dense batch as the op batch the egress wrappers take."""
    off = torch.from_numpy(d.op_off).to("cuda:0")
    if kind == "lwwreg":
        return lwwreg.LwwRegOpBatch(off, to_dev(d.marker), to_dev(d.val))
    i32 = lambda a: torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")  # noqa: E731
    return wire.DotOpBatch(off, i32(d.state_idx), i32(d.actor), None if d.counter is None else to_dev(d.counter),
                           None if d.dir is None else torch.from_numpy(d.dir.copy()).to("cuda:0"))


@pytest.mark.parametrize("kind,D", CASES)
def test_ingest_egress_round_trip(gpu_ctx, kind, D):
    ids, streams, frames, d = case(kind, D)
    assert {0, 1, 63, 64, 65, 70} <= {len(s) for s in streams} and not streams[0] and not streams[-1]
    data, off = dev_frames(frames)
    r = ingest(kind, data, off, ids)
    assert r.totals == (d.n,) and not r.status.cpu().numpy().any()
    assert np.array_equal(r.ops.op_off.cpu().numpy(), d.op_off)
    same_batch(kind, r.ops, d)
    # egress of the codec's dense batch: the encoder's bytes and offsets
    f_off, out, st = egress(kind, dense_dev(kind, d), ids)
    assert not st.cpu().numpy().any() and np.array_equal(f_off.cpu().numpy(), off.cpu().numpy())
    assert bytes(out.cpu().numpy()) == b"".join(frames)
    assert [L.dec_frame(kind, b, ids) for b in L.split(out.cpu().numpy(), f_off.cpu().numpy())] == streams
    # ingest -> egress is byte-identical
    f_off2, out2, st2 = egress(kind, r.ops, ids)
    assert bytes(out2.cpu().numpy()) == b"".join(frames) and np.array_equal(f_off2.cpu().numpy(), off.cpu().numpy())
    assert not st2.cpu().numpy().any()


def raw_ingest(ctx, kind, data, off, ids, buf, status, totals):
    n = off.shape[0] - 1
    if kind == "lwwreg":
        ctx.call("crdt_lwwreg_ops_ingest", dptr(data), dptr(off), n, buf, dptr(status), totals)
    else:
        dd = dev_dict(kind, ids)
        ctx.call(f"crdt_{kind}_ops_ingest", dptr(data), dptr(off), n, dptr(dd), dd.shape[0], buf, dptr(status), totals)


@pytest.mark.parametrize("kind,D", CASES)
def test_sizing_sync_and_no_sync_modes(gpu_ctx, kind, D):
    ids, streams, frames, d = case(kind, D)
    data, off = dev_frames(frames)
    status = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    tot = (ctypes.c_uint64 * 1)(12345)
    raw_ingest(gpu_ctx, kind, data, off, ids, None, status, tot)  # out = NULL: the sizing call
    assert tot[0] == d.n and not status.cpu().numpy().any()
    # the bound a caller sizes by without a sync: exact for well-formed frames
    bound = sum((len(f) - 8) // L.REC[kind] for f in frames)
    assert bound == d.n
    a, b = ingest(kind, data, off, ids), ingest(kind, data, off, ids, sync=False, caps=(bound,))
    assert b.totals is None and a.totals == (d.n,)
    for r in (a, b):
        assert np.array_equal(r.ops.op_off.cpu().numpy(), d.op_off) and not r.status.cpu().numpy().any()
        same_batch(kind, r.ops, d)
    # N = 0
    e = ingest(kind, data[:0], off[:1], ids)
    assert e.totals == (0,) and e.ops.op_off.cpu().tolist() == [0]


@pytest.mark.parametrize("kind,D", CASES)
def test_prefix_cut(gpu_ctx, kind, D):
    ids, streams, frames, d = case(kind, D)
    data, off = dev_frames(frames)
    kept = int(d.op_off[100])
    cap = kept + 3
    assert d.op_off[101] > cap  # frame 100 does not fit
    S8, S32, S64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device="cuda:0")  # noqa: E731
    op_off = full(N + 1, -1, torch.int64)
    status = full(N, -1, torch.int32)
    room = d.n + 8  # the arrays are longer than op_cap: nothing past op_cap may be touched
    if kind == "lwwreg":
        arrs = {"marker": full(room, S64, torch.int64), "val": full(room, S64, torch.int64)}
        buf = _abi.LwwRegOpsBuf(cap, dptr(op_off), dptr(arrs["marker"]), dptr(arrs["val"]))
        ops = lwwreg.LwwRegOpBatch(op_off, arrs["marker"], arrs["val"])
    else:
        arrs = {"state_idx": full(room, S32, torch.int32), "actor": full(room, S32, torch.int32),
                "counter": full(room, S64, torch.int64), "dir": full(room, S8, torch.uint8)}
        buf = _abi.DotOpsBuf(cap, dptr(op_off), dptr(arrs["state_idx"]), dptr(arrs["actor"]), dptr(arrs["counter"]),
                             dptr(arrs["dir"]))
        ops = wire.DotOpBatch(op_off, arrs["state_idx"], arrs["actor"], arrs["counter"], arrs["dir"])
    raw_ingest(gpu_ctx, kind, data, off, ids, ctypes.byref(buf), status, None)
    st, go = status.cpu().numpy(), op_off.cpu().numpy()
    assert not st[:100].any() and (st[100:] == CAP).all()
    assert np.array_equal(go[:101], d.op_off[:101]) and (go[100:] == kept).all()
    same_batch(kind, ops, d, kept)
    for nm, t in arrs.items():  # untouched past the kept ops (and so past op_cap)
        written = {"counter": kind != "gset", "dir": kind == "pncounter"}.get(nm, True)
        tail = t.cpu().numpy()[kept if written else 0:]
        assert (tail == tail.dtype.type(S64 & ((1 << (8 * tail.itemsize)) - 1))).all(), nm


def refusals(kind, frames, streams, ids):
    """-> (frames with malformed ones swapped in, the indices refused)."""
    fr = list(frames)
    rec = L.REC[kind]
    assert all(len(streams[i]) >= 2 for i in (7, 66, 150, 180)) and len(streams[151]) >= 1
    fr[7] = fr[7][:-4]                                   # truncated
    fr[66] = fr[66] + b"\0\0\0\0"                        # trailing bytes
    fr[120] = struct.pack("<Q", 1 << 61)                 # n x rec wraps to the 0 bytes that follow (rec 8 / 16)
    fr[121] = struct.pack("<Q", 1 << 61) + b"\0" * rec   # and with one record behind it
    fr[150] = fr[150] + b"\0\0"                          # frame 150 ends, and 151 starts, off a 4-byte boundary
    fr[151] = fr[151] + b"\0\0"
    bad = [7, 66, 120, 121, 150, 151]
    if kind == "pncounter":
        b = bytearray(fr[180])
        struct.pack_into("<I", b, 8 + 16 * (len(streams[180]) - 1) + 12, 2)  # the last op's dir tag
        fr[180] = bytes(b)
        bad.append(180)
    fr[190] = fr[190][:4]                                # shorter than a length
    bad.append(190)
    return fr, bad


@pytest.mark.parametrize("kind,D", CASES)
def test_refusals_leave_the_neighbours_intact(gpu_ctx, kind, D):
    ids, streams, frames, _ = case(kind, D)
    fr, bad = refusals(kind, frames, streams, ids)
    d = L.Dense(kind, [[] if i in bad else s for i, s in enumerate(streams)])
    data, off = dev_frames(fr)
    assert int(off[151]) % 4 == 2
    for kw in ({}, {"sync": False, "caps": (d.n + 5,)}):
        r = ingest(kind, data, off, ids, **kw)
        st = r.status.cpu().numpy()
        assert [i for i in range(N) if st[i]] == sorted(bad) and all(st[i] == BAD for i in bad)
        assert np.array_equal(r.ops.op_off.cpu().numpy(), d.op_off)
        same_batch(kind, r.ops, d)
        assert kw or r.totals == (d.n,)


def reduced(kind, D):
    """The case's frames (written with the full dictionary) read through a dictionary that lacks one
    id in use -> (short ids, the dense batch expected: shifted indices, NONE for the lost id)."""
    ids, streams, frames, d = case(kind, D)
    lost = 2
    short = ids[:lost] + ids[lost + 1:]
    col = d.actor.astype(np.int64)
    want = np.where(col == lost, NONE, np.where(col > lost, col - 1, col)).astype(np.uint32)
    assert (col == lost).any()
    return short, want, lost


@pytest.mark.parametrize("kind,D", DICT_CASES)
def test_missing_ids_keep_their_place_and_apply_skips_them(gpu_ctx, kind, D):
    ids, streams, frames, d = case(kind, D)
    short, want, lost = reduced(kind, D)
    data, off = dev_frames(frames)
    r = ingest(kind, data, off, short)
    st = r.status.cpu().numpy()
    hit = np.array([any((op if kind == "gset" else op.actor if kind == "vclock" else op[0].actor) == lost for op in s)
                    for s in streams])
    assert np.array_equal(st, np.where(hit, MISSING, 0)) and r.totals == (d.n,)
    assert np.array_equal(r.ops.op_off.cpu().numpy(), d.op_off) and np.array_equal(u32(r.ops.actor), want)
    if kind != "gset":
        assert np.array_equal(to_host(r.ops.counter), d.counter)
    # the apply that follows counts them into bad and applies the rest
    Ds = D - 1
    if kind == "gset":
        rows = torch.zeros((N, (Ds + 63) // 64), dtype=torch.int64, device="cuda:0")
        nbad = apply.apply_inserts(rows, r.ops.state_idx, r.ops.element, Ds)
        exp = np.zeros((N, (Ds + 63) // 64), np.uint64)
        for s, c in zip(d.state_idx, want):
            if c != NONE:
                exp[s, c // 64] |= np.uint64(1 << int(c % 64))
    else:
        k = 2 if kind == "pncounter" else 1
        rows = torch.zeros((N, k * Ds), dtype=torch.int64, device="cuda:0")
        nbad = apply.apply_dots(kind, rows, r.ops.state_idx, r.ops.actor, r.ops.counter, r.ops.dir)
        exp = np.zeros((N, k * Ds), np.uint64)
        for o, (s, c) in enumerate(zip(d.state_idx, want)):
            if c != NONE:
                w = int(c) + (Ds if kind == "pncounter" and d.dir[o] else 0)
                exp[s, w] = max(exp[s, w], d.counter[o])
    assert nbad == int((want == NONE).sum()) and np.array_equal(to_host(rows), exp)


@pytest.mark.parametrize("kind,D", DICT_CASES)
def test_egress_refuses_ops_with_no_wire_form(gpu_ctx, kind, D):
    ids, streams, frames, d = case(kind, D)
    ops = dense_dev(kind, d)
    bad = [2, 5]
    actor = d.actor.copy()
    actor[d.op_off[2]] = D          # an index >= A / U (frame 2 holds 63 ops: its first)
    actor[d.op_off[6] - 1] = NONE   # what ingest writes for a missing id (frame 5: its last op)
    ops = ops._replace(actor=torch.from_numpy(actor.view(np.int32).copy()).to("cuda:0"))
    if kind == "pncounter":
        dr = d.dir.copy()
        dr[d.op_off[4] + 10] = 3    # a dir of 3 (frame 4 holds 65 ops)
        ops = ops._replace(dir=torch.from_numpy(dr).to("cuda:0"))
        bad.append(4)
    f_off, out, st = egress(kind, ops, ids)
    st = st.cpu().numpy()
    assert [i for i in range(N) if st[i]] == sorted(bad) and all(st[i] == MISSING for i in bad)
    want = [struct.pack("<Q", 0) if i in bad else f for i, f in enumerate(frames)]
    assert L.split(out.cpu().numpy(), f_off.cpu().numpy()) == want


def test_lwwreg_egress_refuses_an_invalid_op_off(gpu_ctx):
    _, streams, frames, d = case("lwwreg", 0)
    off = d.op_off.copy()
    off[10] = off[9] - 1 if off[9] else d.n + 1  # register 9 runs backwards (or past n_ops)
    ops = dense_dev("lwwreg", d)._replace(op_off=torch.from_numpy(off).to("cuda:0"))
    f_off, out, st = wire.lwwreg_ops_egress(ops)
    got = L.split(out.cpu().numpy(), f_off.cpu().numpy())
    st = st.cpu().numpy()
    assert st[9] == MISSING and got[9] == struct.pack("<Q", 0)
    assert all(got[i] == frames[i] and st[i] == 0 for i in range(N) if i not in (9, 10))


def test_full_range_counters_pass_through(gpu_ctx):
    ids = [3, 9, 0xFFFFFFFF]
    streams = [[O.Dot(2, 2**64 - 1), O.Dot(0, 5)], [O.Dot(1, 2**63), O.Dot(1, 2**63 - 1), O.Dot(2, 1)]]
    frames = [L.enc_frame("vclock", s, ids) for s in streams]
    data, off = dev_frames(frames)
    r = ingest("vclock", data, off, ids)
    assert to_host(r.ops.counter).tolist() == [2**64 - 1, 5, 2**63, 2**63 - 1, 1] and not r.status.cpu().numpy().any()
    rows = to_dev(np.array([[1, 0, 2**63], [0, 7, 0]], np.uint64))
    assert apply.apply_dots("vclock", rows, r.ops.state_idx, r.ops.actor, r.ops.counter) == 0
    assert to_host(rows).tolist() == [[5, 0, 2**64 - 1], [0, 2**63, 1]]
    f_off, out, st = egress("vclock", r.ops, ids)
    assert bytes(out.cpu().numpy()) == b"".join(frames) and not st.cpu().numpy().any()
    s_off, s_out = wire.vclock_egress(rows, dev_dict("vclock", ids))
    assert L.split(s_out.cpu().numpy(), s_off.cpu().numpy()) == [O.bc_vclock({3: 5, 0xFFFFFFFF: 2**64 - 1}),
                                                                  O.bc_vclock({9: 2**63, 0xFFFFFFFF: 1})]


@pytest.mark.parametrize("kind,D", [("vclock", 13000), ("gset", 7000)])
def test_dictionaries_past_the_lds_budget(gpu_ctx, kind, D):
    """52 KiB of actors / 56 KiB of elements: past the 48 KiB staged in LDS, searched in global memory."""
    rng = np.random.default_rng(D)
    ids = L.sparse_dict(rng, D, 64 if kind == "gset" else 32)
    streams = [[gen_op(kind, rng, D) for _ in range(n)] for n in (0, 70, 1, 64)]
    streams[1][0] = O.Dot(D - 1, 9) if kind == "vclock" else D - 1  # the dictionary's last and first ids
    streams[1][1] = O.Dot(0, 9) if kind == "vclock" else 0
    frames = [L.enc_frame(kind, s, ids) for s in streams]
    d = L.Dense(kind, streams)
    data, off = dev_frames(frames)
    r = ingest(kind, data, off, ids)
    assert r.totals == (d.n,) and not r.status.cpu().numpy().any()
    assert np.array_equal(r.ops.op_off.cpu().numpy(), d.op_off)
    same_batch(kind, r.ops, d)
    f_off, out, st = egress(kind, r.ops, ids)
    assert bytes(out.cpu().numpy()) == b"".join(frames) and not st.cpu().numpy().any()
    # an id between two dictionary entries is missing
    gap = next(x + 1 for x, y in zip(ids, ids[1:]) if y > x + 1)
    rec = struct.pack("<IQ", gap, 5) if kind == "vclock" else struct.pack("<Q", gap)
    data, off = dev_frames([struct.pack("<Q", 1) + rec])
    r = ingest(kind, data, off, ids)
    assert r.status.cpu().tolist() == [MISSING] and u32(r.ops.actor).tolist() == [NONE]


LOOPS = [("vclock", "vclock", 200), ("vclock", "gcounter", 5), ("pncounter", "pncounter", 5),
         ("pncounter", "pncounter", 200), ("gset", "gset", U), ("lwwreg", "lwwreg", 0)]


@pytest.mark.parametrize("kind,typ,D", LOOPS)
def test_frames_to_ops_to_apply_to_frames(gpu_ctx, kind, typ, D):
    """bytes -> op batch -> apply_batch onto non-empty states -> state bytes, against the oracle's
    classes applied op by op and encoded by O.bc_*."""
    ids, streams, frames, d = case(kind, D)
    rng = np.random.default_rng(9 + D)
    data, off = dev_frames(frames)
    r = ingest(kind, data, off, ids)
    if kind == "lwwreg":
        m0 = rng.integers(0, 8, size=N).astype(np.uint64)
        v0 = rng.integers(0, 3, size=N).astype(np.uint64)
        regs = [O.LWWReg(int(v), int(m)) for m, v in zip(m0, v0)]
        conf = [c for reg, s in zip(regs, streams) for c in L.replay_lww(reg, s)]
        m, v = to_dev(m0), to_dev(v0)
        conflict, status = lwwreg.apply_batch(m, v, r.ops)
        assert conflict.cpu().numpy().tolist() == conf and any(conf)
        s_off, s_out = wire.lwwreg_egress(m, v)
        want = [O.bc_lwwreg(reg.val, reg.marker) for reg in regs]
    elif kind == "gset":
        W = (D + 63) // 64
        init = rng.integers(0, 1 << 63, size=(N, W)).astype(np.uint64) & rng.integers(0, 1 << 63, size=(N, W)).astype(np.uint64)
        init[:, W - 1] &= np.uint64((1 << (D % 64)) - 1) if D % 64 else np.uint64(2**64 - 1)
        sets = [O.GSet(ids[e] for e in range(D) if (int(init[i, e // 64]) >> (e % 64)) & 1) for i in range(N)]
        for g, s in zip(sets, streams):
            for e in s:
                g.apply(ids[e])
        rows = to_dev(init)
        assert apply.apply_inserts(rows, r.ops.state_idx, r.ops.element, D) == 0
        s_off, s_out = wire.gset_egress(rows, dev_dict(kind, ids))
        want = [O.bc_gset(g.value) for g in sets]
    else:
        k = 2 if kind == "pncounter" else 1
        init = rng.integers(0, 1 << 40, size=(N, k * D)).astype(np.uint64) * (rng.random((N, k * D)) < 0.4)
        objs = []
        for i in range(N):
            o = {"vclock": O.VClock, "gcounter": O.GCounter, "pncounter": O.PNCounter}[typ]()
            halves = [o.p.inner, o.n.inner] if typ == "pncounter" else [o.inner if typ == "gcounter" else o]
            for h, clk in enumerate(halves):
                clk.dots = {a: int(init[i, h * D + a]) for a in range(D) if init[i, h * D + a]}
            for op in streams[i]:
                o.apply(op)
            objs.append(halves)
        rows = to_dev(init)
        assert apply.apply_dots(typ, rows, r.ops.state_idx, r.ops.actor, r.ops.counter, r.ops.dir) == 0
        named = lambda clk: {ids[a]: c for a, c in clk.dots.items()}  # noqa: E731
        if kind == "pncounter":
            s_off, s_out = wire.pncounter_egress(rows, dev_dict(kind, ids))
            want = [O.bc_pncounter(named(p), named(n)) for p, n in objs]
        else:
            s_off, s_out = wire.vclock_egress(rows, dev_dict(kind, ids))
            want = [O.bc_vclock(named(c)) for c, in objs]
    assert L.split(s_out.cpu().numpy(), s_off.cpu().numpy()) == want
