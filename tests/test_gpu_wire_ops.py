"""GPU: op streams on the wire (crdt_*_ops_ingest / crdt_*_ops_egress) against the host encoder
(orswot.encode_ops / map.encode_ops), the test-side frame codec (wire_ops_util) and the oracle's
apply.  Exact integer equality everywhere."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import oracle as O
import wire_ops_util as W
from gpu_util import to_dev, to_host
from orswot_apply_util import dense_states, oracle_streams, random_ops, replay_streams, to_object

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import wire  # noqa: E402

DEV = "cuda:0"
SHAPES = [(70, 9, 90), (5, 64, 70), (3, 65, 40), (2, 1, 30)]  # (N, A, M or K)
LENS = [0, 1, 63, 64, 65, 130]  # the 64-op parse batch's edges


def d32(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.uint32).view(np.int32)).to(DEV)


def d64(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64)).to(DEV)


def dev_frames(frames):
    data, off = W.pack_frames(frames)
    return torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def frames_of(off, data):
    off, data = host(off), host(data).tobytes()
    return [data[off[s]:off[s + 1]] for s in range(len(off) - 1)]


def same_batch(got, ref):
    """Every array of the two op batches (pads included: the sync wrapper leaves encode_ops' pads)."""
    for nm, g, r in zip(got._fields, got, ref):
        g, r = host(g), host(r)
        assert g.shape == r.shape and np.array_equal(g, r), nm


def random_map_ops(rng, n, K, A):
    ops = []
    for _ in range(n):
        clk = O.VClock({int(a): int(rng.integers(1, 6)) for a in rng.choice(A, size=int(rng.integers(0, min(A, 3) + 1)),
                                                                               replace=False)})
        if rng.random() < 0.6:
            ops.append(O.MapUp(O.Dot(int(rng.integers(A)), int(rng.integers(1, 9))), int(rng.integers(K)),
                               O.MVRegPut(clk, int(rng.integers(1, 1 << 40)))))
        else:
            ops.append(O.MapRm(clk, {int(k) for k in rng.choice(K, size=int(rng.integers(0, 4)), replace=False)}))
    return ops


def sized(rng, streams, shape_ix, more):
    """Stream s cut or extended (with more(n)) to LENS[(s + shape_ix) % 6] ops."""
    out = []
    for s, ops in enumerate(streams):
        n = LENS[(s + shape_ix) % len(LENS)]
        out.append(list(ops[:n]) + more(max(0, n - len(ops))))
    return out


@functools.lru_cache(maxsize=None)
def orswot_case(ix):
    N, A, M = SHAPES[ix]
    rng = np.random.default_rng(100 + ix)
    streams = replay_streams(100 + ix, N, A, M, 200)
    streams = sized(rng, streams, ix, lambda n: random_ops(rng, n, M, A, 8))
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    return streams, aid, mid


@functools.lru_cache(maxsize=None)
def map_case(ix):
    from test_gpu_map_apply import replay_streams as map_replay
    N, A, K = SHAPES[ix]
    rng = np.random.default_rng(200 + ix)
    streams = map_replay(200 + ix, N, A, K, 200)
    streams = sized(rng, streams, ix, lambda n: random_map_ops(rng, n, K, A))
    aid, kid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, K, 32)
    return streams, aid, kid


def orswot_ref(streams, A):
    return cg.orswot.encode_ops([[W.orswot_tuple(o) for o in s] for s in streams], A, DEV)


def map_ref(streams, A):
    return cg.map.encode_ops([[W.map_tuple(o) for o in s] for s in streams], A, DEV)


def orswot_ingest(streams, aid, mid, ctx, **kw):
    data, off = dev_frames([W.enc_orswot_frame(s, aid, mid) for s in streams])
    return wire.orswot_ops_ingest(data, off, d32(aid), d64(mid), ctx=ctx, **kw)


def map_ingest(streams, aid, kid, ctx, **kw):
    data, off = dev_frames([W.enc_map_frame(s, aid, kid) for s in streams])
    return wire.map_ops_ingest(data, off, d32(aid), d32(kid), ctx=ctx, **kw)


def check_offsets(res, ref, is_map):
    """row_off / id_off are the state's first clock row / id, totals the sums."""
    op_off, kind = host(ref.op_off), host(ref.kind)
    ids_off = host(ref.key_off if is_map else ref.mem_off)
    rows = np.concatenate([[0], np.cumsum(np.ones_like(kind) if is_map else kind)]).astype(np.int64)
    assert np.array_equal(host(res.row_off), rows[op_off])
    assert np.array_equal(host(res.id_off), ids_off[op_off])
    assert res.totals == (len(kind), int(rows[-1]), int(ids_off[-1]))


# ---- 1. ingest equals the host encoder ---------------------------------------------------------------
@pytest.mark.parametrize("ix", range(len(SHAPES)))
def test_orswot_ingest_equals_encode_ops(gpu_ctx, ix):
    streams, aid, mid = orswot_case(ix)
    assert ix != 0 or {len(s) for s in streams} >= set(LENS)
    res = orswot_ingest(streams, aid, mid, gpu_ctx)
    assert not host(res.status).any()
    ref = orswot_ref(streams, len(aid))
    same_batch(res.ops, ref)
    check_offsets(res, ref, False)
    # clock rows through rm_row
    rc, rr, k = to_host(res.ops.rm_clock), host(res.ops.rm_row), host(res.ops.kind)
    flat = [o for s in streams for o in s]
    for o, op in enumerate(flat):
        assert k[o] == isinstance(op, O.OrswotRm)
        if k[o]:
            assert {a: int(v) for a, v in enumerate(rc[rr[o]]) if v} == {a: c for a, c in op.clock.dots.items() if c}


@pytest.mark.parametrize("ix", range(len(SHAPES)))
def test_map_ingest_equals_encode_ops(gpu_ctx, ix):
    streams, aid, kid = map_case(ix)
    assert ix != 0 or {len(s) for s in streams} >= set(LENS)
    res = map_ingest(streams, aid, kid, gpu_ctx)
    assert not host(res.status).any()
    ref = map_ref(streams, len(aid))
    same_batch(res.ops, ref)
    check_offsets(res, ref, True)
    pool, cr = to_host(res.ops.clk_pool), host(res.ops.clk_row)
    for o, op in enumerate(o for s in streams for o in s):
        clk = op.op.clock if isinstance(op, O.MapUp) else op.clock
        assert {a: int(v) for a, v in enumerate(pool[cr[o]]) if v} == {a: c for a, c in clk.dots.items() if c}


# ---- 2. through the kernels ---------------------------------------------------------------------------
def orswot_apply(ops, N, M, A, Dcap, ctx, objs=None):
    objs = objs if objs is not None else [O.Orswot() for _ in range(N)]
    clock, entries, dcl, dmb, cnt = dense_states(objs, M, A, Dcap)
    st = [to_dev(clock), to_dev(entries), to_dev(dcl), to_dev(dmb), torch.from_numpy(cnt).to(DEV)]
    status = cg.orswot.apply_batch(*st, ops, ctx=ctx)
    got = [to_host(t) for t in st[:4]] + [host(st[4])]
    return [to_object(*got, s) for s in range(N)], host(status)


@pytest.mark.parametrize("ix", [0, 2])
def test_orswot_frames_to_apply(gpu_ctx, ix):
    streams, aid, mid = orswot_case(ix)
    N, A, M = SHAPES[ix]
    res = orswot_ingest(streams, aid, mid, gpu_ctx)
    Dcap = max(1, max(sum(isinstance(o, O.OrswotRm) for o in s) for s in streams))
    got, status = orswot_apply(res.ops, N, M, A, Dcap, gpu_ctx)
    assert not status.any()
    want = oracle_streams([O.Orswot() for _ in streams], streams)
    for s in range(N):
        assert got[s] == want[s], s


def map_apply(ops, N, K, A, V, Dcap, ctx):
    Kw = (K + 63) // 64
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    st = [z(N, A), z(N, K, A), z(N, K, V, A), z(N, K, V), z(N, Dcap, A), z(N, Dcap, Kw),
          torch.zeros(N, dtype=torch.int32, device=DEV)]
    status = cg.map.apply_batch(*st, ops, ctx=ctx)
    c, e, vc, vv, dc, dk = (to_host(t) for t in st[:6])
    n = host(st[6])
    maps = []
    for s in range(N):
        deferred = [(dc[s, d], O.bitmap_members(dk[s, d])) for d in range(int(n[s]))]
        maps.append(O.dense_to_map(c[s], e[s], vc[s], vv[s], deferred))
    return maps, host(status)


def map_oracle(streams):
    out, peak = [], 1
    for ops in streams:
        m = O.Map(O.MVReg)
        for op in ops:
            m.apply(op)
            peak = max([peak] + [len(e.val.vals) for e in m.entries.values()])
        out.append(m)
    return out, peak


@pytest.mark.parametrize("ix", [0, 2])
def test_map_frames_to_apply(gpu_ctx, ix):
    streams, aid, kid = map_case(ix)
    N, A, K = SHAPES[ix]
    res = map_ingest(streams, aid, kid, gpu_ctx)
    want, peak = map_oracle(streams)
    Dcap = max(1, max(sum(isinstance(o, O.MapRm) for o in s) for s in streams))
    got, status = map_apply(res.ops, N, K, A, peak, Dcap, gpu_ctx)
    assert not status.any()
    for s in range(N):
        assert got[s].clock == want[s].clock and got[s].entries == want[s].entries and \
            got[s].deferred == want[s].deferred, s


# ---- 3. egress ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ix", [0, 1, 3])
def test_orswot_egress_decodes_to_the_ops(gpu_ctx, ix):
    streams, aid, mid = orswot_case(ix)
    off, data, status = wire.orswot_ops_egress(orswot_ref(streams, len(aid)), d32(aid), d64(mid), ctx=gpu_ctx)
    assert not host(status).any()
    for s, f in enumerate(frames_of(off, data)):
        assert f == W.enc_orswot_frame(streams[s], aid, mid), s  # encode_ops lists members ascending
        assert [W.orswot_key(o) for o in W.dec_orswot_frame(f, aid, mid)] == [W.orswot_key(o) for o in streams[s]]


@pytest.mark.parametrize("ix", [0, 1, 3])
def test_map_egress_decodes_to_the_ops(gpu_ctx, ix):
    streams, aid, kid = map_case(ix)
    off, data, status = wire.map_ops_egress(map_ref(streams, len(aid)), d32(aid), d32(kid), ctx=gpu_ctx)
    assert not host(status).any()
    for s, f in enumerate(frames_of(off, data)):
        assert W.dec_map_frame(f, aid, kid) == streams[s], s


def shuffled_orswot_frame(rng, ops, aid, mid):
    """Members in arbitrary order, now and then with a duplicate (a HashSet serializes in any order;
    the ingest keeps the list as written)."""
    out = struct.pack("<Q", len(ops))
    for op in ops:
        ms = [int(m) for m in rng.permutation(sorted(op.members))]
        if ms and rng.random() < 0.3:
            ms.append(ms[0])
        out += W.enc_orswot_op(op, aid, mid, members=ms)
    return out


def test_orswot_ingest_egress_is_byte_identical(gpu_ctx):
    streams, aid, mid = orswot_case(0)
    rng = np.random.default_rng(7)
    frames = [shuffled_orswot_frame(rng, s, aid, mid) for s in streams]
    data, off = dev_frames(frames)
    res = wire.orswot_ops_ingest(data, off, d32(aid), d64(mid), ctx=gpu_ctx)
    assert not host(res.status).any()
    # duplicates kept, frame order kept
    lists = [ms for f in frames for ms in W.dec_orswot_frame(f, aid, mid, with_lists=True)[1]]
    assert host(res.ops.mem)[:-1].tolist() == [m for ms in lists for m in ms]
    off2, data2, status = wire.orswot_ops_egress(res.ops, d32(aid), d64(mid), ctx=gpu_ctx)
    assert not host(status).any()
    assert np.array_equal(host(off2), host(off)) and host(data2).tobytes() == host(data).tobytes()


def test_map_ingest_egress_is_byte_identical(gpu_ctx):
    streams, aid, kid = map_case(0)
    data, off = dev_frames([W.enc_map_frame(s, aid, kid) for s in streams])
    res = wire.map_ops_ingest(data, off, d32(aid), d32(kid), ctx=gpu_ctx)
    off2, data2, status = wire.map_ops_egress(res.ops, d32(aid), d32(kid), ctx=gpu_ctx)
    assert not host(status).any() and not host(res.status).any()
    assert np.array_equal(host(off2), host(off)) and host(data2).tobytes() == host(data).tobytes()


def orswot_ops_struct(ops):
    from crdts_gpu import _abi
    from crdts_gpu.context import dptr
    o = _abi.OrswotOps()
    o.n_ops = ops.kind.shape[0]
    o.op_off, o.kind, o.actor, o.counter = dptr(ops.op_off), dptr(ops.kind), dptr(ops.actor), dptr(ops.counter)
    o.rm_row, o.rm_clock, o.n_rm_rows = dptr(ops.rm_row), dptr(ops.rm_clock), ops.rm_clock.shape[0]
    o.mem_off, o.mem, o.n_mem = dptr(ops.mem_off), dptr(ops.mem), ops.mem.shape[0]
    return o


def test_egress_sizing_call_with_null_bytes(gpu_ctx):
    from crdts_gpu.context import dptr
    streams, aid, mid = orswot_case(1)
    ops = orswot_ref(streams, len(aid))
    N = len(streams)
    frame_off = torch.empty(N + 1, dtype=torch.int64, device=DEV)
    status = torch.empty(N, dtype=torch.int32, device=DEV)
    total = ctypes.c_size_t()
    a, m = d32(aid), d64(mid)
    gpu_ctx.call("crdt_orswot_ops_egress", ctypes.byref(orswot_ops_struct(ops)), N, dptr(a), len(aid), dptr(m), len(mid),
                 dptr(frame_off), None, 0, ctypes.byref(total), dptr(status))
    lens = [len(W.enc_orswot_frame(s, aid, mid)) for s in streams]
    assert total.value == sum(lens) and host(frame_off).tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert not host(status).any()


def test_egress_op_without_a_wire_form(gpu_ctx):
    streams, aid, mid = orswot_case(0)
    streams = [s for s in streams if len(s) >= 1][:4]
    ops = orswot_ref(streams, len(aid))
    op_off = host(ops.op_off)
    mem, kind, mem_off = host(ops.mem).copy(), host(ops.kind).copy(), host(ops.mem_off)
    o1 = next(o for o in range(op_off[1], op_off[2]) if mem_off[o + 1] > mem_off[o])
    mem[mem_off[o1]] = len(mid)      # state 1: a member index out of range
    kind[op_off[2]] = 2              # state 2: a bad kind
    bad = ops._replace(mem=torch.from_numpy(mem).to(DEV), kind=torch.from_numpy(kind).to(DEV))
    off, data, status = wire.orswot_ops_egress(bad, d32(aid), d64(mid), ctx=gpu_ctx)
    assert host(status).tolist() == [0, wire.MISSING, wire.MISSING, 0]
    fr = frames_of(off, data)
    assert fr[1] == fr[2] == struct.pack("<Q", 0)
    assert fr[0] == W.enc_orswot_frame(streams[0], aid, mid) and fr[3] == W.enc_orswot_frame(streams[3], aid, mid)
    # the Map twin: a key index out of range in a keyset, a clock row past the pool
    mstreams, maid, kid = map_case(0)
    mstreams = [s for s in mstreams if any(isinstance(o, O.MapRm) and o.keyset for o in s)][:3]
    mops = map_ref(mstreams, len(maid))
    m_off, keys, key_off, row = host(mops.op_off), host(mops.keys).copy(), host(mops.key_off), host(mops.clk_row).copy()
    o0 = next(o for o in range(m_off[0], m_off[1]) if key_off[o + 1] > key_off[o])
    keys[key_off[o0]] = len(kid)
    row[m_off[2]] = mops.clk_pool.shape[0]
    mbad = mops._replace(keys=torch.from_numpy(keys).to(DEV), clk_row=torch.from_numpy(row).to(DEV))
    off, data, status = wire.map_ops_egress(mbad, d32(maid), d32(kid), ctx=gpu_ctx)
    assert host(status).tolist() == [wire.MISSING, 0, wire.MISSING]
    fr = frames_of(off, data)
    assert fr[0] == fr[2] == struct.pack("<Q", 0) and W.dec_map_frame(fr[1], maid, kid) == mstreams[1]


# ---- 4. long and wide ops -------------------------------------------------------------------------------
def test_long_and_wide_ops(gpu_ctx):
    rng = np.random.default_rng(11)
    A, M = 700, 3100
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    big = O.OrswotRm(O.VClock({int(a): int(rng.integers(1, 1 << 50)) for a in rng.choice(A, size=600, replace=False)}),
                     [int(m) for m in rng.choice(M, size=3000, replace=False)])
    wide = O.OrswotAdd(O.Dot(3, 9), [int(m) for m in rng.choice(M, size=70, replace=False)])
    # clocks of 63, 64, 65 and 130 records: up to 64 an op's own lane parses them, past that the wave
    edge = [O.OrswotRm(O.VClock({int(a): int(rng.integers(1, 99)) for a in rng.choice(A, size=n, replace=False)}), [n])
            for n in (63, 64, 65, 130)]
    streams = [random_ops(rng, 5, M, A, 8), random_ops(rng, 3, M, A, 8) + [big, wide] + random_ops(rng, 70, M, A, 8),
               [wide, big], random_ops(rng, 4, M, A, 8) + edge]
    frames = [W.enc_orswot_frame(s, aid, mid) for s in streams]
    assert len(frames[1]) > 8192 * 3, "longer than the LDS ring"
    res = orswot_ingest(streams, aid, mid, gpu_ctx)
    assert not host(res.status).any()
    same_batch(res.ops, orswot_ref(streams, A))
    off, data, status = wire.orswot_ops_egress(res.ops, d32(aid), d64(mid), ctx=gpu_ctx)
    assert not host(status).any() and frames_of(off, data) == frames
    # the Map twin: a 600-actor Put clock and a 200-key keyset
    K = 300
    kid = W.sparse_dict(rng, K, 32)
    up = O.MapUp(O.Dot(1, 2), 7, O.MVRegPut(O.VClock({int(a): 5 for a in rng.choice(A, size=600, replace=False)}), 99))
    rm = O.MapRm(O.VClock({int(a): 3 for a in rng.choice(A, size=650, replace=False)}),
                 {int(k) for k in rng.choice(K, size=200, replace=False)})
    medge = [O.MapUp(O.Dot(2, n), 1, O.MVRegPut(O.VClock({int(a): 7 for a in rng.choice(A, size=n, replace=False)}), n))
             for n in (64, 65)]
    mstreams = [random_map_ops(rng, 3, K, A) + medge, [up, rm, up] + random_map_ops(rng, 66, K, A) + [rm], [rm]]
    mres = map_ingest(mstreams, aid, kid, gpu_ctx)
    assert not host(mres.status).any()
    same_batch(mres.ops, map_ref(mstreams, A))
    off, data, status = wire.map_ops_egress(mres.ops, d32(aid), d32(kid), ctx=gpu_ctx)
    assert not host(status).any() and frames_of(off, data) == [W.enc_map_frame(s, aid, kid) for s in mstreams]


# ---- 5. malformed ---------------------------------------------------------------------------------------
def u64(x):
    return struct.pack("<Q", x)


def u32(x):
    return struct.pack("<I", x)


def malformed_batch(ingest, ref, enc, valid0, valid1, two_ops, extra, aid, ids, ids_dev, ctx):
    f = enc(two_ops, aid, ids)
    bad = [f[:k] for k in range(0, len(f), 4)] + [f + u32(0), f + u64(0)] + extra
    frames = [enc(valid0, aid, ids)] + bad + [enc(valid1, aid, ids)]
    data, off = dev_frames(frames)
    res = ingest(data, off, d32(aid), ids_dev(ids), ctx=ctx)  # ids_dev: d64 (members) or d32 (keys)
    st = host(res.status)
    assert st[0] == 0 and st[-1] == 0 and (st[1:-1] == wire.BAD).all(), st
    # no ops from the malformed frames; the neighbours' ops and offsets intact
    same_batch(res.ops, ref([valid0] + [[] for _ in bad] + [valid1], len(aid)))
    return res


def test_orswot_malformed_frames(gpu_ctx):
    streams, aid, mid = orswot_case(2)
    v0, v1 = streams[1][:7], streams[2][:9]
    add, rm = O.OrswotAdd(O.Dot(1, 4), [2, 5]), O.OrswotRm(O.VClock({0: 3, 2: 1}), [1])
    tag2 = bytearray(W.enc_orswot_frame([add, rm], aid, mid))
    tag2[8:12] = u32(2)
    one = W.enc_orswot_frame([add], aid, mid)
    extra = [bytes(tag2),
             u64(1 << 40) + W.enc_orswot_frame([add, rm], aid, mid)[8:],             # n_ops
             one[:24] + u64(1 << 40) + one[32:],                                      # a set length
             u64(1) + u32(1) + u64(1 << 40) + u32(aid[0]) + u64(1) + u64(0),          # a clock length
             u64(1) + u32(1) + u64(6) + u32(aid[0]) + u64(1) + u64(0),                # ... that passes the frame's end
             u64((1 << 64) - 1), u64(1), u32(0)]
    malformed_batch(wire.orswot_ops_ingest, orswot_ref, W.enc_orswot_frame, v0, v1, [add, rm], extra, aid, mid, d64, gpu_ctx)


def test_map_malformed_frames(gpu_ctx):
    streams, aid, kid = map_case(2)
    v0, v1 = streams[1][:7], streams[2][:9]
    up, rm = O.MapUp(O.Dot(1, 4), 3, O.MVRegPut(O.VClock({0: 3, 2: 1}), 77)), O.MapRm(O.VClock({1: 2}), {0, 4})
    f = W.enc_map_frame([up, rm], aid, kid)
    tag2, mv1 = bytearray(f), bytearray(f)
    tag2[8:12] = u32(2)
    mv1[28:32] = u32(1)  # n_ops 8 | tag 4 | dot 12 | key 4 | MVReg tag
    assert f[28:32] == u32(0) and f[24:28] == u32(kid[3])
    rm1 = W.enc_map_frame([rm], aid, kid)
    extra = [bytes(tag2), bytes(mv1),
             u64(1 << 40) + f[8:],                                         # n_ops
             rm1[:-16] + u64(1 << 40) + rm1[-8:],                          # a keyset length
             u64(1) + u32(0) + u64(1 << 40) + u32(aid[0]) + u64(1) + u64(0),  # an rm clock length
             f[:32] + u64(1 << 40) + f[40:]]                               # a Put clock length
    malformed_batch(wire.map_ops_ingest, map_ref, W.enc_map_frame, v0, v1, [up, rm], extra, aid, kid, d32, gpu_ctx)


def test_misaligned_offsets(gpu_ctx):
    streams, aid, mid = orswot_case(2)
    v0, v1 = streams[1][:7], streams[2][:9]
    f0, f, f1 = (W.enc_orswot_frame(s, aid, mid) for s in (v0, streams[1][:2], v1))
    raw = f0 + b"\0\0" + f + b"\0\0" + f1
    cuts = [0, len(f0), len(f0) + 2, len(f0) + 2 + len(f), len(f0) + 4 + len(f), len(raw)]
    data = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)
    off = torch.tensor(cuts, dtype=torch.int64, device=DEV)
    res = wire.orswot_ops_ingest(data, off, d32(aid), d64(mid), ctx=gpu_ctx)
    assert host(res.status).tolist() == [0, wire.BAD, wire.BAD, wire.BAD, 0]
    same_batch(res.ops, orswot_ref([v0, [], [], [], v1], len(aid)))


# ---- 6. missing ids -------------------------------------------------------------------------------------
def test_orswot_missing_ids(gpu_ctx):
    rng = np.random.default_rng(21)
    A, M, N = 6, 40, 3
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    aid_x = aid + [next(x for x in range(1, 1 << 20) if x not in aid)]  # index A / M: an id in no dictionary
    mid_x = mid + [next(x for x in range(1, 1 << 20) if x not in mid)]
    assert aid_x[A] not in aid and mid_x[M] not in mid
    good = [random_ops(rng, 12, M, A, 8) for _ in range(N)]
    sent = [good[0][:5] + [O.OrswotAdd(O.Dot(A, 5), [1, 2]), O.OrswotAdd(O.Dot(0, 9), [3, M]),
                           O.OrswotRm(O.VClock({0: 2, A: 7}), [4])] + good[0][5:], good[1], good[2] + [O.OrswotRm(O.VClock({A: 1}), [M])]]
    kept = [good[0][:5] + [O.OrswotAdd(O.Dot(0, 9), [3]), O.OrswotRm(O.VClock({0: 2}), [4])] + good[0][5:], good[1],
            good[2] + [O.OrswotRm(O.VClock(), [])]]
    data, off = dev_frames([W.enc_orswot_frame(s, aid_x, mid_x) for s in sent])
    res = wire.orswot_ops_ingest(data, off, d32(aid), d64(mid), ctx=gpu_ctx)
    assert host(res.status).tolist() == [wire.MISSING, 0, wire.MISSING]
    op_off, actor, mem, mem_off = host(res.ops.op_off), host(res.ops.actor), host(res.ops.mem), host(res.ops.mem_off)
    assert op_off.tolist() == [0, len(sent[0]), len(sent[0]) + len(sent[1]), sum(map(len, sent))]
    assert actor[5] == -1 and (actor[:5] >= 0).all()                       # the op keeps its place
    assert mem[mem_off[6]:mem_off[7]].tolist() == [3, -1]
    rc, rr = to_host(res.ops.rm_clock), host(res.ops.rm_row)
    assert {a: int(v) for a, v in enumerate(rc[rr[7]]) if v} == {0: 2}      # the missing actor's record skipped
    assert not rc[rr[op_off[3] - 1]].any() and mem[mem_off[op_off[3] - 1]] == -1
    Dcap = 16
    got, status = orswot_apply(res.ops, N, M, A, Dcap, gpu_ctx)
    assert [int(x) & 2 for x in status] == [2, 0, 2] and not (status & ~2).any()
    want = oracle_streams([O.Orswot() for _ in kept], kept)
    for s in range(N):
        assert got[s] == want[s], s


def test_map_missing_ids(gpu_ctx):
    rng = np.random.default_rng(22)
    A, K, N = 5, 30, 2
    aid, kid = W.sparse_dict(rng, A, 31), W.sparse_dict(rng, K, 31)
    aid_x, kid_x = aid + [(1 << 31) + 5], kid + [(1 << 31) + 9]
    good = [random_map_ops(rng, 10, K, A) for _ in range(N)]
    put = lambda dots, v: O.MVRegPut(O.VClock(dots), v)  # noqa: E731
    sent = [good[0][:4] + [O.MapUp(O.Dot(A, 3), 2, put({0: 1}, 5)), O.MapUp(O.Dot(1, 30), K, put({1: 30}, 6)),
                           O.MapUp(O.Dot(2, 40), 3, put({2: 40, A: 9}, 7)), O.MapRm(O.VClock({3: 50, A: 1}), {1, K})]
            + good[0][4:], good[1]]
    kept = [good[0][:4] + [O.MapUp(O.Dot(2, 40), 3, put({2: 40}, 7)), O.MapRm(O.VClock({3: 50}), {1})] + good[0][4:], good[1]]
    data, off = dev_frames([W.enc_map_frame(s, aid_x, kid_x) for s in sent])
    res = wire.map_ops_ingest(data, off, d32(aid), d32(kid), ctx=gpu_ctx)
    assert host(res.status).tolist() == [wire.MISSING, 0]
    actor, key, keys, key_off = host(res.ops.actor), host(res.ops.key), host(res.ops.keys), host(res.ops.key_off)
    assert actor[4] == -1 and key[5] == -1 and keys[key_off[7]:key_off[8]].tolist() == [1, -1]
    pool, cr = to_host(res.ops.clk_pool), host(res.ops.clk_row)
    assert {a: int(v) for a, v in enumerate(pool[cr[6]]) if v} == {2: 40}
    want, peak = map_oracle(kept)
    got, status = map_apply(res.ops, N, K, A, max(peak, 2), 16, gpu_ctx)
    assert [int(x) & 2 for x in status] == [2, 0] and not (status & ~2).any()
    for s in range(N):
        assert got[s].clock == want[s].clock and got[s].entries == want[s].entries and \
            got[s].deferred == want[s].deferred, s


# ---- 7. the no-sync path and capacities ---------------------------------------------------------------
def test_no_sync_wrapper_with_room(gpu_ctx):
    streams, aid, mid = orswot_case(0)
    ref = orswot_ref(streams, len(aid))
    n, r, i = ref.kind.shape[0], ref.rm_clock.shape[0] - 1, ref.mem.shape[0] - 1
    res = orswot_ingest(streams, aid, mid, gpu_ctx, sync=False, caps=(n + 5, r + 3, i + 9))
    assert res.totals is None and not host(res.status).any()
    assert np.array_equal(host(res.ops.op_off), host(ref.op_off))
    for nm, cnt in (("kind", n), ("actor", n), ("counter", n), ("rm_row", n), ("rm_clock", r), ("mem_off", n + 1), ("mem", i)):
        assert np.array_equal(host(getattr(res.ops, nm))[:cnt], host(getattr(ref, nm))[:cnt]), nm
    # the capacity-sized batch goes to apply_batch as it is
    N, A, M = SHAPES[0]
    Dcap = max(1, max(sum(isinstance(o, O.OrswotRm) for o in s) for s in streams))
    got, status = orswot_apply(res.ops, N, M, A, Dcap, gpu_ctx)
    want = oracle_streams([O.Orswot() for _ in streams], streams)
    assert not status.any() and all(got[s] == want[s] for s in range(N))


CANARY = 0x5A


def raw_ingest(ctx, is_map, data, off, actors, ids, caps, sizing=False):
    """The C entry point with caller-made buffers: 4 canary elements after every capacity."""
    from crdts_gpu import _abi
    from crdts_gpu.context import dptr
    N = off.shape[0] - 1
    A = actors.shape[0]
    fn = "crdt_map_ops_ingest" if is_map else "crdt_orswot_ops_ingest"
    status = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    head = (dptr(data), dptr(off), N, dptr(actors), A, dptr(ids), ids.shape[0])
    tot = (ctypes.c_uint64 * 3)()
    if sizing:
        ctx.call(fn, *head, None, None, None, dptr(status), tot)
        return tuple(int(x) for x in tot), status
    n, r, i = caps
    mk = lambda cnt, dt: torch.full((cnt + 4,), CANARY, dtype=dt, device=DEV)  # noqa: E731
    bufs = dict(op_off=mk(N + 1, torch.int64), kind=mk(n, torch.uint8), actor=mk(n, torch.int32), counter=mk(n, torch.int64),
                row=mk(n, torch.int32), pool=mk(r * A, torch.int64), ids_off=mk(n + 1, torch.int64), ids=mk(i, torch.int32),
                key=mk(n, torch.int32), val=mk(n, torch.int64), row_off=mk(N + 1, torch.int64), id_off=mk(N + 1, torch.int64))
    b = (_abi.MapOpsBuf if is_map else _abi.OrswotOpsBuf)()
    b.op_cap, b.row_cap, b.id_cap = n, r, i
    b.op_off, b.kind, b.actor, b.counter = (dptr(bufs[k]) for k in ("op_off", "kind", "actor", "counter"))
    if is_map:
        b.key, b.val, b.clk_row, b.clk_pool, b.key_off, b.keys = (dptr(bufs[k]) for k in ("key", "val", "row", "pool", "ids_off", "ids"))
    else:
        b.rm_row, b.rm_clock, b.mem_off, b.mem = (dptr(bufs[k]) for k in ("row", "pool", "ids_off", "ids"))
    ctx.call(fn, *head, ctypes.byref(b), dptr(bufs["row_off"]), dptr(bufs["id_off"]), dptr(status), None)
    return {k: host(v) for k, v in bufs.items()}, host(status)


@pytest.mark.parametrize("which", ["ops", "rows", "ids"])
@pytest.mark.parametrize("is_map", [False, True])
def test_capacities_cut_between_states(gpu_ctx, is_map, which):
    streams, aid, ids = (map_case if is_map else orswot_case)(0)
    N, A = len(streams), len(aid)
    enc = W.enc_map_frame if is_map else W.enc_orswot_frame
    ref = (map_ref if is_map else orswot_ref)(streams, A)
    data, off = dev_frames([enc(s, aid, ids) for s in streams])
    actors, idd = d32(aid), (d32(ids) if is_map else d64(ids))
    op_off, kind = host(ref.op_off), host(ref.kind)
    ids_off = host(ref.key_off if is_map else ref.mem_off)
    rows = np.concatenate([[0], np.cumsum(np.ones_like(kind) if is_map else kind)]).astype(np.int64)
    row_off, id_off = rows[op_off], ids_off[op_off]
    totals, st = raw_ingest(gpu_ctx, is_map, data, off, actors, idd, None, sizing=True)
    assert totals == (int(op_off[-1]), int(row_off[-1]), int(id_off[-1])) and not host(st).any()
    # the first state at or past N/2 that adds to the cut quantity: the capacity ends right before it
    per = {"ops": op_off, "rows": row_off, "ids": id_off}[which]
    c = next(s for s in range(N // 2, N) if per[s + 1] > per[s])
    caps = [int(op_off[-1]), int(row_off[-1]), int(id_off[-1])]
    caps[["ops", "rows", "ids"].index(which)] = int(per[c + 1]) - 1
    got, st = raw_ingest(gpu_ctx, is_map, data, off, actors, idd, caps)
    assert not st[:c].any() and (st[c:] == wire.CAP).all()
    n, r, i = int(op_off[c]), int(row_off[c]), int(id_off[c])
    for nm, want in (("op_off", op_off), ("row_off", row_off), ("id_off", id_off)):
        assert got[nm][:c + 1].tolist() == want[:c + 1].tolist() and (got[nm][c + 1:N + 1] == want[c]).all(), nm
    names = dict(kind="kind", actor="actor", counter="counter", row="clk_row" if is_map else "rm_row")
    if is_map:
        names.update(key="key", val="val")
    for k, nm in names.items():
        assert np.array_equal(got[k][:n], host(getattr(ref, nm))[:n]), nm
    assert np.array_equal(got["pool"][:r * A], host(ref.clk_pool if is_map else ref.rm_clock).reshape(-1)[:r * A])
    assert np.array_equal(got["ids_off"][:n + 1], ids_off[:n + 1])
    assert np.array_equal(got["ids"][:i], host(ref.keys if is_map else ref.mem)[:i])
    # nothing past a capacity: the canaries stand
    canary = lambda a: (a == CANARY).all()  # noqa: E731
    for k, cap in (("kind", caps[0]), ("actor", caps[0]), ("counter", caps[0]), ("row", caps[0]), ("pool", caps[1] * A),
                   ("ids_off", caps[0] + 1), ("ids", caps[2]), ("op_off", N + 1), ("row_off", N + 1), ("id_off", N + 1)):
        assert canary(got[k][cap:]), k


# ---- 8. a dictionary past LDS ---------------------------------------------------------------------------
def test_member_dictionary_past_lds(gpu_ctx):
    rng = np.random.default_rng(31)
    N, A, M = 3, 5, 24000
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    streams = [random_ops(rng, n, M, A, 8) for n in (40, 0, 70)]
    streams[2].append(O.OrswotAdd(O.Dot(1, 1), [0, M - 1, M // 2] + [int(m) for m in rng.choice(M, size=80, replace=False)]))
    res = orswot_ingest(streams, aid, mid, gpu_ctx)
    assert not host(res.status).any()
    same_batch(res.ops, orswot_ref(streams, A))
    off, data, status = wire.orswot_ops_egress(res.ops, d32(aid), d64(mid), ctx=gpu_ctx)
    assert frames_of(off, data) == [W.enc_orswot_frame(s, aid, mid) for s in streams]


# ---- 9. replication over the wire -----------------------------------------------------------------------
def i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32), dtype=torch.int32, device=DEV)


def i64(x):
    return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int64, device=DEV)


def test_replication_over_the_wire(gpu_ctx):
    """Replica X runs the device read loop (read -> derive ctx -> op batch); the batch leaves as
    frames, comes back through the ingest and is applied to replica Y's states; Y equals the oracle
    replica that applied the decoded frames."""
    M, A, Dcap, N = 70, 5, 24, 3
    rng = np.random.default_rng(41)
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    actors, members = d32(aid), d64(mid)
    xs = oracle_streams([O.Orswot() for _ in range(N)], replay_streams(2, N, A, M, 140))
    ys = oracle_streams([O.Orswot() for _ in range(N)], replay_streams(3, N, A, M, 100))
    xc, xe = (to_dev(t) for t in dense_states(xs, M, A, Dcap)[:2])
    yd = dense_states(ys, M, A, Dcap)
    yst = [to_dev(yd[0]), to_dev(yd[1]), to_dev(yd[2]), to_dev(yd[3]), torch.from_numpy(yd[4]).to(DEV)]

    def ship(ops, tag):
        off, data, est = wire.orswot_ops_egress(ops, actors, members, ctx=gpu_ctx)
        assert not host(est).any()
        back = wire.orswot_ops_ingest(data, off, actors, members, ctx=gpu_ctx)
        assert not host(back.status).any()
        status = cg.orswot.apply_batch(*yst, back.ops, ctx=gpu_ctx)
        assert not host(status).any()
        for s, f in enumerate(frames_of(off, data)):  # what a peer running the reference would decode
            for op in W.dec_orswot_frame(f, aid, mid):
                ys[s].apply(op)
        got = [to_host(t) for t in yst[:4]] + [host(yst[4])]
        for s in range(N):
            assert to_object(*got, s) == ys[s], (tag, s)
        return sum(len(W.dec_orswot_frame(f, aid, mid)) for f in frames_of(off, data))

    # contains -> derive_rm_ctx -> Rm: a present and an absent member of every X state
    src, mem = [], []
    for s in range(N):
        present = sorted(xs[s].entries)
        absent = [m for m in range(M) if m not in xs[s].entries]
        for m in (present[-1], present[0], absent[0]):
            src.append(s), mem.append(m)
    Q = len(src)
    rc, qst = cg.orswot.contains(xc, xe, i32(src), i32(mem), ctx=gpu_ctx)
    rm = cg.derive_rm_ctx(rc)
    ops = cg.orswot.OrswotOpBatch(i64(np.searchsorted(src, np.arange(N + 1))), torch.ones(Q, dtype=torch.uint8, device=DEV),
                                  i32(np.zeros(Q)), i64(np.zeros(Q)), i32(np.arange(Q)), rm.clock, i64(np.arange(Q + 1)),
                                  i32(mem))
    assert not host(qst).any() and ship(ops, "rm") == Q
    # read -> derive_add_ctx -> Add
    read = cg.orswot.read(xc, xe, ctx=gpu_ctx)
    add = cg.derive_add_ctx(read, i32([s % A for s in range(N)]), ctx=gpu_ctx)
    ops = cg.orswot.OrswotOpBatch(i64(np.arange(N + 1)), torch.zeros(N, dtype=torch.uint8, device=DEV), add.actor, add.counter,
                                  i32(np.zeros(N)), i64(np.zeros((1, A))), i64(np.arange(N + 1)),
                                  i32([(11 * s + 3) % M for s in range(N)]))
    assert not host(add.status).any() and ship(ops, "add") == N
