"""GPU: the value-typed Maps' op streams on the wire (crdt_map_{counter,orswot,nested}_ops_ingest /
_egress) against the host encoders (map.encode_counter_ops / encode_orswot_map_ops / encode_nested_ops),
the test-side frame codec (wire_vmap_ops_util) and the oracle's apply.  Exact integer equality
everywhere.  The four types: "g" Map<u32, GCounter>, "pn" Map<u32, PNCounter>, "orswot"
Map<u32, Orswot<u64, u32>>, "nested" Map<u32, Map<u32, MVReg<u64, u32>, u32>>."""
import ctypes
import functools
import struct
from typing import NamedTuple

import numpy as np
import pytest
import torch

import oracle as O
import wire_vmap_ops_util as V
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

DEV = "cuda:0"
SHAPES = [(70, 9, 90), (5, 64, 70), (3, 65, 40), (2, 1, 30)]  # (N, A, K); A = 65: clocks past one lane's records
M = 33                      # Orswot values
K2S = [8, 64, 65, 256]      # nested: inner keys per shape (65 crosses to two mask words)
LENS = [0, 1, 63, 64, 65, 130]  # the 64-op parse batch's edges
KINDS = V.KINDS
POS, NEG = O.PNCounter.POS, O.PNCounter.NEG

BATCH = {"g": cg.map.MapCounterOpBatch, "pn": cg.map.MapCounterOpBatch, "orswot": cg.map.MapOrswotOpBatch,
         "nested": cg.map.MapNestedOpBatch}
BUF = {"g": _abi.MapCounterOpsBuf, "pn": _abi.MapCounterOpsBuf, "orswot": _abi.MapOrswotOpsBuf,
       "nested": _abi.MapNestedOpsBuf}
CONST = {"g": _abi.MapCounterOps, "pn": _abi.MapCounterOps, "orswot": _abi.MapOrswotOps, "nested": _abi.MapNestedOps}
FN = {"g": "counter", "pn": "counter", "orswot": "orswot", "nested": "nested"}


def d32(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.uint32).view(np.int32)).to(DEV)


def d64(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Case(NamedTuple):
    kind: str
    streams: tuple
    aid: tuple
    kid: tuple
    vid: tuple  # member ids (orswot) / inner-key ids (nested) / ()

    @property
    def A(self):
        return len(self.aid)

    def dicts(self):
        """The dictionaries as device tensors, in argument order."""
        out = [d32(self.aid), d32(self.kid)]
        if self.kind == "orswot":
            out.append(d64(self.vid))
        elif self.kind == "nested":
            out.append(d32(self.vid))
        return out

    def with_streams(self, streams):
        return self._replace(streams=tuple(tuple(s) for s in streams))


def make_case(kind, rng, streams, A, K, U):
    vid = () if kind in ("g", "pn") else tuple(V.sparse_dict(rng, U, 64 if kind == "orswot" else 32))
    return Case(kind, tuple(tuple(s) for s in streams), tuple(V.sparse_dict(rng, A, 32)), tuple(V.sparse_dict(rng, K, 32)),
                vid)


def value_size(kind, ix):
    return {"orswot": M, "nested": K2S[ix]}.get(kind, 0)


@functools.lru_cache(maxsize=None)
def case(kind, ix):
    """Random streams of every op variant, stream s of LENS[(s + ix) % 6] ops; now and then a clock over
    all A actors (A = 65: more records than a lane parses)."""
    N, A, K = SHAPES[ix]
    U = value_size(kind, ix)
    rng = np.random.default_rng(300 + 10 * KINDS.index(kind) + ix)
    streams = [V.random_ops(kind, rng, LENS[(s + ix) % len(LENS)], A, K, U, full=0.1) for s in range(N)]
    return make_case(kind, rng, streams, A, K, U)


def enc_frames(c, streams=None):
    return [V.enc_frame(c.kind, s, c.aid, c.kid, c.vid) for s in (c.streams if streams is None else streams)]


def dev_frames(frames):
    data, off = V.pack_frames(frames)
    return torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)


def frames_of(off, data):
    off, data = host(off), host(data).tobytes()
    return [data[off[s]:off[s + 1]] for s in range(len(off) - 1)]


def ingest_frames(c, frames, ctx, **kw):
    data, off = dev_frames(frames)
    fn = getattr(wire, f"map_{FN[c.kind]}_ops_ingest")
    if c.kind in ("g", "pn"):
        kw["pn"] = c.kind == "pn"
    return fn(data, off, *c.dicts(), ctx=ctx, **kw)


def ingest(c, ctx, streams=None, **kw):
    return ingest_frames(c, enc_frames(c, streams), ctx, **kw)


def egress(c, batch, ctx):
    fn = getattr(wire, f"map_{FN[c.kind]}_ops_egress")
    kw = {"pn": c.kind == "pn"} if c.kind in ("g", "pn") else {}
    return fn(batch, *c.dicts(), ctx=ctx, **kw)


def ref(c, streams=None):
    """The host encoder's batch: the specification of the dense form."""
    tuples = [[V.op_tuple(c.kind, o) for o in s] for s in (c.streams if streams is None else streams)]
    if c.kind in ("g", "pn"):
        return cg.map.encode_counter_ops(tuples, c.A, DEV)
    if c.kind == "orswot":
        return cg.map.encode_orswot_map_ops(tuples, c.A, DEV)
    return cg.map.encode_nested_ops(tuples, c.A, DEV, K2=len(c.vid))


def same_batch(got, want):
    """Every array of the two op batches, pads included (the sync wrapper allocates as the encoders do)."""
    assert type(got) is type(want)
    for nm, g, r in zip(got._fields, got, want):
        g, r = host(g), host(r)
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), nm


def layout(kind, b):
    """(op_off, row_off, key_first, mem_first) of an encoder's batch, and its totals."""
    op_off, k = host(b.op_off), host(b.kind)
    if kind in ("g", "pn"):
        has_row = k == 1
    elif kind == "orswot":
        has_row = (k == 1) | (host(b.vkind) == 1)
    else:
        has_row = np.ones_like(k, dtype=bool)
    rows = np.concatenate([[0], np.cumsum(has_row)]).astype(np.int64)
    key_off = host(b.key_off)
    mem_off = host(b.mem_off) if kind == "orswot" else np.zeros(len(k) + 1, np.int64)
    return (op_off, rows[op_off], key_off[op_off], mem_off[op_off]), (len(k), int(rows[-1]), int(key_off[-1]), int(mem_off[-1]))


def check_offsets(c, res, want):
    (op_off, row_off, key_first, mem_first), totals = layout(c.kind, want)
    assert np.array_equal(host(res.row_off), row_off) and np.array_equal(host(res.key_first), key_first)
    if c.kind == "orswot":
        assert np.array_equal(host(res.mem_first), mem_first)
    else:
        assert res.mem_first is None
    assert res.totals == totals


# ---- 1. ingest equals the host encoder ---------------------------------------------------------------
@pytest.mark.parametrize("ix", range(len(SHAPES)))
@pytest.mark.parametrize("kind", KINDS)
def test_ingest_equals_the_host_encoder(gpu_ctx, kind, ix):
    c = case(kind, ix)
    assert ix != 0 or {len(s) for s in c.streams} >= set(LENS)
    res = ingest(c, gpu_ctx)
    assert not host(res.status).any()
    want = ref(c)
    same_batch(res.batch, want)
    check_offsets(c, res, want)
    if kind == "nested":
        assert tuple(res.batch.ikeys.shape[1:]) == ((2,) if K2S[ix] == 65 else (4,) if K2S[ix] == 256 else ())
    if SHAPES[ix][1] == 65:  # the wave-loop clock path ran: a clock of 65 records is in the frames
        assert any(len(v.dots) == 65 for s in c.streams for o in s for v in clocks_of(o))


def clocks_of(op):
    """The VClocks an op carries (an Rm's, an Orswot Rm's, a Put's or an inner Rm's)."""
    if isinstance(op, O.MapRm):
        return [op.clock]
    v = op.op
    if isinstance(v, (O.OrswotRm, O.MapRm)):
        return [v.clock]
    if isinstance(v, O.MapUp):
        return [v.op.clock]
    return []


# ---- 2. frames -> ingest -> apply on the GPU equals the oracle ---------------------------------------
def slots_of(d, N, Dcap, A, K):
    Kw = (K + 63) // 64
    dcl, dks, cnt = np.zeros((N, Dcap, A), np.uint64), np.zeros((N, Dcap, Kw), np.uint64), np.zeros(N, np.int32)
    for j in range(d["def_row"].shape[0]):  # the replicas' own deferred removes, as slots
        n = int(d["def_row"][j])
        dcl[n, cnt[n]], dks[n, cnt[n]] = d["def_clock"][j], d["def_keys"][j]
        cnt[n] += 1
    return dcl, dks, cnt


@pytest.mark.parametrize("kind", ["g", "pn"])
def test_counter_frames_to_apply(gpu_ctx, kind):
    from test_gpu_map_counter_apply import _streams
    W = 1 if kind == "g" else 2
    N, K, A, T, Dcap = 24, 6, 6, 40, 16
    maps = O.map_counter_objects(N, K, A, W, seed=40, steps=220)
    d = O.map_counter_to_dense(maps, K, A, W)
    rng = np.random.default_rng(W)
    _, oops = _streams(rng, maps, K, A, W, T)
    c = make_case(kind, rng, oops, A, K, 0)
    res = ingest(c, gpu_ctx)
    assert not host(res.status).any()
    dcl, dks, cnt = slots_of(d, N, Dcap, A, K)
    clock, ec, val = to_dev(d["clock"]), to_dev(d["ec"]), to_dev(d["val"])
    tdc, tdk, tcnt = to_dev(dcl), to_dev(dks), torch.from_numpy(cnt).cuda()
    status = host(cg.map.counter_apply_batch(clock, ec, val, tdc, tdk, tcnt, res.batch, ctx=gpu_ctx))
    cc, e, v = to_host(clock), to_host(ec), to_host(val)
    hdc, hdk, hcnt = to_host(tdc), to_host(tdk), host(tcnt)
    for n in range(N):
        exp = maps[n].copy()
        for op in oops[n]:
            exp.apply(op)
        assert status[n] == 0, (n, status[n])
        dfr = [(hdc[n, i], O.bitmap_members(hdk[n, i])) for i in range(int(hcnt[n]))]
        assert O.dense_to_map_counter(cc[n], e[n], v[n], dfr) == exp, n


def orswot_replay(seed=3):
    """The op-replay states and streams of test_map_orswot_apply at M = 33 (CPU only; lru-cached below)."""
    from test_gpu_map_orswot_apply import _streams
    N, K, A, T = 16, 4, 6, 30
    maps = O.map_orswot_objects(N, K, M, A, seed=60 + seed, steps=160, p_vrm=0.4)
    exps = [O.map_fold_objects([m]) for m in maps]
    rng = np.random.default_rng(seed)
    _, oops = _streams(rng, exps, K, M, A, T)
    for n in range(N):
        for op in oops[n]:
            exps[n].apply(op)
    return maps, exps, oops, rng, (N, K, A)


def test_orswot_frames_to_apply(gpu_ctx):
    from test_gpu_map_orswot_apply import _states
    maps, exps, oops, rng, (N, K, A) = orswot_replay()
    Dcap = 16
    assert all(len(e.val.deferred) <= cg.map.VD_CAP for x in exps for e in x.entries.values())
    assert all(len(x.deferred) <= Dcap for x in exps)
    c = make_case("orswot", rng, oops, A, K, M)
    got = ingest(c, gpu_ctx)
    assert not host(got.status).any()
    res, kw, off = _states(gpu_ctx, maps, K, M, A)
    Kw = (K + 63) // 64
    dcl, dks, cnt = np.zeros((N, Dcap, A), np.uint64), np.zeros((N, Dcap, Kw), np.uint64), np.zeros(N, np.int32)
    if kw:
        keep, hk, hc = host(res.def_keep), to_host(res.def_keys), to_host(kw["def_clock"])
        for n in range(N):
            for j in range(off[n], off[n + 1]):
                if keep[j]:
                    dcl[n, cnt[n]], dks[n, cnt[n]] = hc[j], hk[j]
                    cnt[n] += 1
    tdc, tdk, tcnt = to_dev(dcl), to_dev(dks), torch.from_numpy(cnt).cuda()
    status = host(cg.map.orswot_apply_batch(res, tdc, tdk, tcnt, got.batch, ctx=gpu_ctx))
    cc, e, o, m = to_host(res.clock), to_host(res.ec), to_host(res.oc), to_host(res.ent)
    vn, vc, vm = host(res.vd_n), to_host(res.vd_clock), to_host(res.vd_mem)
    hdc, hdk, hcnt = to_host(tdc), to_host(tdk), host(tcnt)
    for n in range(N):
        assert status[n] == 0, (n, status[n])
        mw = (lambda k, i: vm[n, k, i]) if vm.ndim == 4 else (lambda k, i: vm[n, k, i:i + 1])  # noqa: E731
        vd = {k: [(vc[n, k, i], O.bitmap_members(mw(k, i))) for i in range(int(vn[n, k]))] for k in range(K)}
        dfr = [(hdc[n, i], O.bitmap_members(hdk[n, i])) for i in range(int(hcnt[n]))]
        g = O.dense_to_map_orswot(cc[n], e[n], o[n], m[n], vd, dfr)
        assert g.clock == exps[n].clock and g.entries == exps[n].entries and g.deferred == exps[n].deferred, n


@pytest.mark.parametrize("K,K2,A,seed", [(4, 6, 5, 1), (3, 65, 5, 4)])
def test_nested_frames_to_apply(gpu_ctx, K, K2, A, seed):
    from test_gpu_map_nested import _slot_deferred, canon, decode_states, nested_states
    from test_gpu_map_nested_apply import _fits, _regs_in_order, _streams
    N, T = 24, 30
    maps = [m for m in O.nested_map_objects(N + 8, K, K2, A, seed=80 + seed, steps=200, p_irm=0.5, p_ooo=0.8, p_rm=0.3)
            if _fits(m)][:N]
    rng = np.random.default_rng(seed)
    _, oops = _streams(rng, maps, K, K2, A, T)
    exps = [m.copy() for m in maps]
    for n in range(len(maps)):
        for op in oops[n]:
            exps[n].apply(op)
    keep = [n for n in range(len(maps)) if _fits(exps[n])]
    assert len(keep) >= 12
    maps, exps, oops = [maps[n] for n in keep], [exps[n] for n in keep], [oops[n] for n in keep]
    c = make_case("nested", rng, oops, A, K, K2)
    res = ingest(c, gpu_ctx)
    assert not host(res.status).any()
    st, slots, _ = nested_states(maps, K, K2, A)
    status = host(cg.map.nested_apply_batch(st, *slots, res.batch, ctx=gpu_ctx))
    for n, exp in enumerate(exps):
        assert status[n] == 0, (n, status[n])
        got = decode_states(st, n, _slot_deferred(slots, n))
        assert canon(got) == canon(exp) and _regs_in_order(got) == _regs_in_order(exp), n


# ---- 3. egress ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ix", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_egress_decodes_to_the_ops(gpu_ctx, kind, ix):
    c = case(kind, ix)
    off, data, status = egress(c, ref(c), gpu_ctx)
    assert not host(status).any()
    want = enc_frames(c)  # the encoders list members and keys ascending, as the test codec writes them
    for s, f in enumerate(frames_of(off, data)):
        assert f == want[s], s
        assert [V.op_key(kind, o) for o in V.dec_frame(kind, f, c.aid, c.kid, c.vid)] == \
            [V.op_key(kind, o) for o in c.streams[s]]


def shuffled_orswot_frame(rng, c, ops):
    """Members in arbitrary order, now and then with a duplicate (a HashSet serializes in any order; the
    ingest keeps the list as written)."""
    out = struct.pack("<Q", len(ops))
    for op in ops:
        ms = None
        if isinstance(op, O.MapUp):
            ms = [int(m) for m in rng.permutation(sorted(op.op.members))]
            if ms and rng.random() < 0.3:
                ms.append(ms[0])
        out += V.enc_op("orswot", op, c.aid, c.kid, c.vid, members=ms)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_ingest_egress_is_byte_identical(gpu_ctx, kind):
    c = case(kind, 0)
    frames = enc_frames(c)
    if kind == "orswot":
        rng = np.random.default_rng(7)
        frames = [shuffled_orswot_frame(rng, c, s) for s in c.streams]
    res = ingest_frames(c, frames, gpu_ctx)
    assert not host(res.status).any()
    if kind == "orswot":  # duplicates kept, frame order kept
        lists = [ms for f in frames for ms in V.dec_frame(kind, f, c.aid, c.kid, c.vid, with_lists=True)[1] if ms is not None]
        assert host(res.batch.mems).tolist() == [m for ms in lists for m in ms]
    off, data, status = egress(c, res.batch, gpu_ctx)
    assert not host(status).any()
    assert frames_of(off, data) == frames


def const_struct(kind, b, drop=()):
    o = CONST[kind]()
    o.n_ops = b.kind.shape[0]
    for nm, t in zip(b._fields, b):
        setattr(o, nm, dptr(t))
    o.n_clk_rows, o.n_keys = b.clk_pool.shape[0], b.keys.shape[0]
    if kind == "orswot":
        o.n_mems = b.mems.shape[0]
    for nm in drop:  # an array the header allows to be NULL
        setattr(o, nm, None)
    return o


def dict_args(c, tensors):
    args = []
    for t in tensors:
        args += [dptr(t), t.shape[0]]
    if c.kind in ("g", "pn"):
        args.append(1 if c.kind == "pn" else 0)
    return args


def raw_egress_sizes(ctx, c, b, drop=()):
    """The sizing call: bytes == NULL."""
    N = b.op_off.shape[0] - 1
    frame_off = torch.empty(N + 1, dtype=torch.int64, device=DEV)
    status = torch.empty(N, dtype=torch.int32, device=DEV)
    total = ctypes.c_size_t()
    tensors = c.dicts()
    ctx.call(f"crdt_map_{FN[c.kind]}_ops_egress", ctypes.byref(const_struct(c.kind, b, drop)), N, *dict_args(c, tensors),
             dptr(frame_off), None, 0, ctypes.byref(total), dptr(status))
    return total.value, host(frame_off), host(status)


@pytest.mark.parametrize("kind", KINDS)
def test_egress_sizing_call_with_null_bytes(gpu_ctx, kind):
    c = case(kind, 1)
    total, frame_off, status = raw_egress_sizes(gpu_ctx, c, ref(c))
    lens = [len(f) for f in enc_frames(c)]
    assert total == sum(lens) and frame_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert not status.any()


# ---- 4. ops without a wire form --------------------------------------------------------------------------
def base_stream(kind):
    """One op of every variant, every clock and list non-empty; indices 0 = Up, 1 = Rm, 2 = the other Up."""
    rm = O.MapRm(O.VClock({0: 3, 2: 1}), {1, 4})
    if kind in ("g", "pn"):
        return [O.MapUp(O.Dot(1, 4), 3, O.Dot(2, 7) if kind == "g" else (O.Dot(2, 7), POS)), rm,
                O.MapUp(O.Dot(0, 5), 2, O.Dot(1, 8) if kind == "g" else (O.Dot(1, 8), NEG))]
    if kind == "orswot":
        return [O.MapUp(O.Dot(1, 4), 3, O.OrswotAdd(O.Dot(2, 7), {5, 9})), rm,
                O.MapUp(O.Dot(0, 5), 2, O.OrswotRm(O.VClock({1: 2}), {6, 7}))]
    return [O.MapUp(O.Dot(1, 4), 3, O.MapUp(O.Dot(2, 7), 5, O.MVRegPut(O.VClock({0: 1}), 77))), rm,
            O.MapUp(O.Dot(0, 5), 2, O.MapRm(O.VClock({1: 2}), {1, 6}))]


def mutations(kind, A, K, U, n_rows, n_keys, n_mems):
    """(field, op index in the state (0..2), value): what one state's op gets.  An offset array is changed
    at the op's end entry, which no other op reads as its begin (the op after it has no list of that kind)."""
    muts = [("kind", 0, 2), ("kind", 1, 255), ("actor", 0, A), ("key", 2, K), ("clk_row", 1, n_rows),
            ("key_off", 1, "reversed"), ("key_off", 1, n_keys + 1), ("keys", 1, K)]
    if kind in ("g", "pn"):
        muts += [("vdir", 0, 2), ("vactor", 2, A), ("vdir", 0, 1 if kind == "g" else 3)]
    elif kind == "orswot":
        muts += [("vkind", 0, 2), ("vactor", 0, A), ("mems", 0, U), ("mems", 2, U), ("clk_row", 2, n_rows),
                 ("mem_off", 0, "reversed"), ("mem_off", 0, n_mems + 1)]
    else:
        muts += [("ikind", 2, 2), ("iactor", 0, A), ("ikey", 0, U), ("ikeys", 2, "bit"), ("clk_row", 0, n_rows),
                 ("clk_row", 2, n_rows + 7)]
    return muts


@pytest.mark.parametrize("kind,U", [("g", 0), ("pn", 0), ("orswot", M), ("nested", 8), ("nested", 64), ("nested", 65),
                                    ("nested", 200)])
def test_egress_op_without_a_wire_form(gpu_ctx, kind, U):
    A, K = 4, 6
    rng = np.random.default_rng(5)
    base = base_stream(kind)
    L = len(base)
    muts = mutations(kind, A, K, U, 0, 0, 0)
    N = 2 * len(muts) + 1  # a good state on each side of every mutated one
    c = make_case(kind, rng, [base] * N, A, K, U)
    good = ref(c)
    arrs = {nm: host(t).copy() for nm, t in zip(good._fields, good)}
    n_rows, n_keys = arrs["clk_pool"].shape[0], arrs["keys"].shape[0]
    n_mems = arrs["mems"].shape[0] if kind == "orswot" else 0
    muts = mutations(kind, A, K, U, n_rows, n_keys, n_mems)
    bad_states = []
    for i, (field, j, val) in enumerate(muts):
        s = 2 * i + 1
        o = s * L + j
        bad_states.append(s)
        if val == "reversed":  # this op's range ends before it begins; no other op reads the entry changed
            arrs[field][o + 1] = arrs[field][o] - 1
        elif field in ("key_off", "mem_off"):
            arrs[field][o + 1] = val
        elif field == "keys":
            arrs[field][arrs["key_off"][o]] = val
        elif field == "mems":
            arrs[field][arrs["mem_off"][o]] = val
        elif val == "bit":  # an inner key at K2 (past 64: in the mask's last word), or past every word the mask has
            if arrs[field].ndim == 1:
                arrs[field][o] |= np.int64(1) << np.int64(U) if U < 64 else np.int64(0)
            else:
                arrs[field][o, U // 64] |= np.int64(1) << np.int64(U % 64)
            if U == 64:
                bad_states.pop()  # K2 = 64: every bit of the one word names a key
        else:
            arrs[field][o] = val
    bad = type(good)(*(torch.from_numpy(arrs[nm]).to(DEV) for nm in good._fields))
    off, data, status = egress(c, bad, gpu_ctx)
    want_status = [wire.MISSING if s in bad_states else 0 for s in range(N)]
    assert host(status).tolist() == want_status
    ok = V.enc_frame(kind, base, c.aid, c.kid, c.vid)
    assert frames_of(off, data) == [struct.pack("<Q", 0) if s in bad_states else ok for s in range(N)]
    # an op_off past the ops: the last state alone
    arrs = {nm: host(t).copy() for nm, t in zip(good._fields, good)}
    arrs["op_off"][-1] += 1
    bad = type(good)(*(torch.from_numpy(arrs[nm]).to(DEV) for nm in good._fields))
    off, data, status = egress(c, bad, gpu_ctx)
    assert host(status).tolist() == [0] * (N - 1) + [wire.MISSING]
    assert frames_of(off, data) == [ok] * (N - 1) + [struct.pack("<Q", 0)]


@pytest.mark.parametrize("kind", KINDS)
def test_egress_map_rm_without_key_off(gpu_ctx, kind):
    base = base_stream(kind)
    c = make_case(kind, np.random.default_rng(6), [base, [base[0], base[2]], base[1:2], []], 4, 6, value_size(kind, 0))
    total, frame_off, status = raw_egress_sizes(gpu_ctx, c, ref(c), drop=("key_off",))
    assert status.tolist() == [wire.MISSING, 0, wire.MISSING, 0]
    lens = [len(f) for f in enc_frames(c)]
    assert np.diff(frame_off).tolist() == [8, lens[1], 8, 8] and total == 24 + lens[1]


@pytest.mark.parametrize("kind", ["g", "pn"])
def test_counter_egress_without_vdir(gpu_ctx, kind):
    """vdir == NULL means all P."""
    rng = np.random.default_rng(8)
    streams = [[O.MapUp(o.dot, o.key, (o.op[0], POS)) if kind == "pn" and isinstance(o, O.MapUp) else o for o in s]
               for s in (V.random_ops(kind, rng, n, 5, 9) for n in (20, 0, 70))]
    c = make_case(kind, rng, streams, 5, 9, 0)
    total, frame_off, status = raw_egress_sizes(gpu_ctx, c, ref(c), drop=("vdir",))
    assert not status.any() and np.diff(frame_off).tolist() == [len(f) for f in enc_frames(c)]
    off, data, status = egress(c, ref(c), gpu_ctx)
    assert frames_of(off, data) == enc_frames(c) and total == data.numel()


def test_nested_refuses_more_than_256_inner_keys(gpu_ctx):
    rng = np.random.default_rng(9)
    c = make_case("nested", rng, [[]], 3, 4, 257)
    with pytest.raises(_abi.CrdtGpuError) as e:
        ingest(c, gpu_ctx)
    assert e.value.code == _abi.CRDT_EUNSUPPORTED
    b = ref(make_case("nested", rng, [base_stream("nested")], 3, 7, 200))
    with pytest.raises(_abi.CrdtGpuError) as e:
        egress(c, b._replace(ikeys=torch.zeros((3, 5), dtype=torch.int64, device=DEV)), gpu_ctx)
    assert e.value.code == _abi.CRDT_EUNSUPPORTED


# ---- 5. long and wide ops -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_long_and_wide_ops(gpu_ctx, kind):
    rng = np.random.default_rng(11)
    A, K = 70, 320
    U = {"orswot": 24000, "nested": 256}.get(kind, 0)  # a member dictionary too large for LDS
    clk = lambda n, hi=1 << 50: O.VClock({int(a): int(rng.integers(1, hi)) for a in rng.choice(A, size=n, replace=False)})  # noqa: E731
    pick = lambda n, top: [int(x) for x in rng.choice(top, size=n, replace=False)]  # noqa: E731
    wide_rm = O.MapRm(clk(65), pick(300, K))
    if kind in ("g", "pn"):
        big = [O.MapUp(O.Dot(3, 9), 7, O.Dot(5, 1 << 60) if kind == "g" else (O.Dot(5, 1 << 60), NEG))]
    elif kind == "orswot":
        big = [O.MapUp(O.Dot(3, 9), 7, O.OrswotAdd(O.Dot(5, 6), pick(300, U) + [0, U - 1])),
               O.MapUp(O.Dot(4, 9), 8, O.OrswotRm(clk(65), pick(70, U))),
               O.MapUp(O.Dot(4, 10), 8, O.OrswotRm(clk(64), pick(5, U)))]
    else:
        big = [O.MapUp(O.Dot(3, 9), 7, O.MapRm(clk(65), pick(200, U) + [0, U - 1])),
               O.MapUp(O.Dot(3, 10), 7, O.MapRm(clk(3), pick(5, U))),
               O.MapUp(O.Dot(4, 9), 8, O.MapUp(O.Dot(5, 6), 255, O.MVRegPut(clk(65), 1 << 63))),
               O.MapUp(O.Dot(4, 10), 8, O.MapUp(O.Dot(5, 7), 64, O.MVRegPut(clk(64), 5)))]
    rnd = lambda n: V.random_ops(kind, rng, n, A, K, U, full=0.02)  # noqa: E731
    streams = [rnd(5), rnd(3) + big + [wide_rm] + rnd(70), [wide_rm] + big, rnd(2000), big[::-1] + rnd(4) + [wide_rm]]
    c = make_case(kind, rng, streams, A, K, U)
    frames = enc_frames(c)
    assert len(frames[3]) > 8 * 256 * 4 * 4, "longer than the LDS ring"
    res = ingest_frames(c, frames, gpu_ctx)
    assert not host(res.status).any()
    same_batch(res.batch, ref(c))
    off, data, status = egress(c, res.batch, gpu_ctx)
    assert not host(status).any() and frames_of(off, data) == frames


# ---- 6. malformed ---------------------------------------------------------------------------------------
def u64(x):
    return struct.pack("<Q", x)


def u32(x):
    return struct.pack("<I", x)


def patched(f, at, new):
    assert at + len(new) <= len(f)
    return f[:at] + new + f[at + len(new):]


def malformed_cases(kind, c, base):
    """One-op frames with one field broken; byte offsets follow the layout rows (n_ops 8 | tag 4 | ...)."""
    enc = lambda ops: V.enc_frame(kind, ops, c.aid, c.kid, c.vid)  # noqa: E731
    f = enc(base)
    up0, rm, up2 = enc(base[0:1]), enc(base[1:2]), enc(base[2:3])
    rm_n = len(base[1].clock.dots)
    rm_cnt_at = 8 + 4 + 8 + 12 * rm_n
    out = [f + u32(0), f + u64(0), up0 + u32(1),                          # trailing words
           patched(f, 8, u32(2)), patched(rm, 8, u32(7)),                 # an unknown outer tag
           u64(1 << 40) + f[8:], u64((1 << 64) - 1), u64(1), u32(0), b"",  # n_ops
           patched(rm, 12, u64(rm_n + 1)), patched(rm, 12, u64(1 << 62)),  # the rm clock's length
           patched(rm, rm_cnt_at, u64(len(base[1].keyset) + 1)), patched(rm, rm_cnt_at, u64(1 << 62)),  # the keyset's
           patched(rm, 12, u64(((1 << 64) - 1) // 3 + 2))]                # 3 * n wraps to a small number
    vt = 8 + 4 + 12 + 4  # the value's first word: its tag, or the counter's dot
    if kind == "pn":
        out += [patched(up0, vt + 12, u32(2)), patched(up2, vt + 12, u32(1 << 31))]  # dir
    if kind == "g":
        out += [up0[:-4], V.enc_frame("pn", [O.MapUp(base[0].dot, base[0].key, (base[0].op, NEG))], c.aid, c.kid)]  # a PNCounter Up
    if kind == "orswot":
        add, orm = up0, up2
        n = len(base[2].op.clock.dots)
        out += [patched(add, vt, u32(2)), patched(orm, vt, u32(9)),       # an unknown value tag
                patched(add, vt + 16, u64(len(base[0].op.members) + 1)), patched(add, vt + 16, u64(1 << 62)),
                patched(orm, vt + 4, u64(n + 1)), patched(orm, vt + 4, u64(1 << 62)),
                patched(orm, vt + 12 + 12 * n, u64(len(base[2].op.members) + 1)),
                patched(orm, vt + 12 + 12 * n, u64(1 << 62)), patched(orm, vt + 12 + 12 * n, u64(1 << 63))]
    if kind == "nested":
        put, irm = up0, up2
        n, pn_ = len(base[2].op.clock.dots), len(base[0].op.op.clock.dots)
        out += [patched(put, vt, u32(2)), patched(irm, vt, u32(5)),       # an unknown value tag
                patched(put, vt + 20, u32(1)),                             # the MVReg tag
                patched(put, vt + 24, u64(pn_ + 1)), patched(put, vt + 24, u64(1 << 62)),  # the Put clock's length
                patched(irm, vt + 4, u64(n + 1)), patched(irm, vt + 4, u64(1 << 62)),
                patched(irm, vt + 12 + 12 * n, u64(len(base[2].op.keyset) + 1)),
                patched(irm, vt + 12 + 12 * n, u64(1 << 62))]
    return out


@pytest.mark.parametrize("kind,U", [("g", 0), ("pn", 0), ("orswot", M), ("nested", 8), ("nested", 65)])
def test_malformed_frames(gpu_ctx, kind, U):
    rng = np.random.default_rng(13)
    A, K = 4, 6
    base = base_stream(kind)
    v0, v1 = V.random_ops(kind, rng, 7, A, K, U), V.random_ops(kind, rng, 9, A, K, U)
    c = make_case(kind, rng, [], A, K, U)
    enc = lambda ops: V.enc_frame(kind, ops, c.aid, c.kid, c.vid)  # noqa: E731
    f = enc(base)
    # every proper prefix of one small frame, as one batch between two well-formed neighbours
    prefixes = [f[:k] for k in range(0, len(f), 4)]
    res = ingest_frames(c, [enc(v0)] + prefixes + [enc(v1)], gpu_ctx)
    st = host(res.status)
    assert st[0] == 0 and st[-1] == 0 and (st[1:-1] == wire.BAD).all(), st
    same_batch(res.batch, ref(c, [v0] + [[] for _ in prefixes] + [v1]))
    # one broken field per frame, a well-formed neighbour on each side of each
    bad = malformed_cases(kind, c, base)
    frames, streams = [enc(v0)], [v0]
    for i, b in enumerate(bad):
        v = v1 if i % 2 == 0 else v0
        frames += [b, enc(v)]
        streams += [[], v]
    res = ingest_frames(c, frames, gpu_ctx)
    st = host(res.status)
    assert (st[0::2] == 0).all() and (st[1::2] == wire.BAD).all(), st
    want = ref(c, streams)
    same_batch(res.batch, want)
    check_offsets(c, res, want)


@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_offsets(gpu_ctx, kind):
    rng = np.random.default_rng(14)
    A, K, U = 4, 6, value_size(kind, 0)
    v0, v1, mid = (V.random_ops(kind, rng, n, A, K, U) for n in (7, 9, 2))
    c = make_case(kind, rng, [], A, K, U)
    f0, f, f1 = (V.enc_frame(kind, s, c.aid, c.kid, c.vid) for s in (v0, mid, v1))
    raw = f0 + b"\0\0" + f + b"\0\0" + f1
    cuts = [0, len(f0), len(f0) + 2, len(f0) + 2 + len(f), len(f0) + 4 + len(f), len(raw)]
    data = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)
    off = torch.tensor(cuts, dtype=torch.int64, device=DEV)
    kw = {"pn": kind == "pn"} if kind in ("g", "pn") else {}
    res = getattr(wire, f"map_{FN[kind]}_ops_ingest")(data, off, *c.dicts(), ctx=gpu_ctx, **kw)
    assert host(res.status).tolist() == [0, wire.BAD, wire.BAD, wire.BAD, 0]
    same_batch(res.batch, ref(c, [v0, [], [], [], v1]))


# ---- 7. missing ids -------------------------------------------------------------------------------------
def extended(c):
    """The case's id lists with one more entry each, an id in no dictionary (index A / K / U)."""
    spare = lambda ids: next(x for x in range(1, 1 << 20) if x not in ids)  # noqa: E731
    return c._replace(aid=c.aid + (spare(c.aid),), kid=c.kid + (spare(c.kid),),
                      vid=c.vid + (spare(c.vid),) if c.vid else ())


def clock_of(pool, row):
    return {a: int(v) for a, v in enumerate(pool[row]) if v}


@pytest.mark.parametrize("pn", [False, True])
def test_counter_missing_ids(gpu_ctx, pn):
    kind = "pn" if pn else "g"
    rng = np.random.default_rng(21)
    A, K, N = 5, 30, 3
    good = [V.random_ops(kind, rng, 10, A, K) for _ in range(N)]
    v = (lambda d: (d, NEG)) if pn else (lambda d: d)
    sent = [good[0][:4] + [O.MapUp(O.Dot(A, 3), 2, v(O.Dot(0, 1))), O.MapUp(O.Dot(1, 30), K, v(O.Dot(1, 2))),
                           O.MapUp(O.Dot(2, 40), 3, v(O.Dot(A, 3))), O.MapRm(O.VClock({3: 50, A: 1}), {1, K})] + good[0][4:],
            good[1], good[2] + [O.MapRm(O.VClock({A: 1}), {K})]]
    kept = [good[0][:4] + [O.MapRm(O.VClock({3: 50}), {1})] + good[0][4:], good[1], good[2]]
    c = make_case(kind, rng, sent, A, K, 0)
    res = ingest_frames(c, enc_frames(extended(c)), gpu_ctx)
    assert host(res.status).tolist() == [wire.MISSING, 0, wire.MISSING]
    b = res.batch
    assert host(b.op_off).tolist() == [0, len(sent[0]), len(sent[0]) + len(sent[1]), sum(map(len, sent))]
    actor, key, vactor, keys, key_off = (host(x) for x in (b.actor, b.key, b.vactor, b.keys, b.key_off))
    assert actor[4] == -1 and key[5] == -1 and vactor[6] == -1 and (actor[:4] >= 0).all()  # the ops keep their places
    assert [actor[5], actor[6], key[4], key[6], vactor[4], vactor[5]] == [1, 2, 2, 3, 0, 1]
    assert keys[key_off[7]:key_off[8]].tolist() == [1, -1]
    pool, cr = to_host(b.clk_pool), host(b.clk_row)
    assert clock_of(pool, cr[7]) == {3: 50}  # the missing actor's record skipped
    last = len(host(b.kind)) - 1
    assert not pool[cr[last]].any() and keys[key_off[last]] == -1
    W, Dcap = 2 if pn else 1, 16
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    st = [z(N, A), z(N, K, A), z(N, K, W, A), z(N, Dcap, A), z(N, Dcap, 1), torch.zeros(N, dtype=torch.int32, device=DEV)]
    status = host(cg.map.counter_apply_batch(*st, b, ctx=gpu_ctx))
    assert [int(x) & 2 for x in status] == [2, 0, 2] and not (status & ~2).any()
    cc, e, vv, dc, dk, cnt = [to_host(t) for t in st[:5]] + [host(st[5])]
    for s in range(N):
        exp = O.Map(O.PNCounter if pn else O.GCounter)
        for op in kept[s]:
            exp.apply(op)
        dfr = [(dc[s, i], O.bitmap_members(dk[s, i])) for i in range(int(cnt[s]))]
        assert O.dense_to_map_counter(cc[s], e[s], vv[s], dfr) == exp, s


def test_orswot_missing_ids(gpu_ctx):
    rng = np.random.default_rng(22)
    A, K = 5, 30
    good = [V.random_ops("orswot", rng, 8, A, K, M) for _ in range(2)]
    add, orm = O.OrswotAdd, O.OrswotRm
    sent = [good[0][:3] + [O.MapUp(O.Dot(A, 3), 2, add(O.Dot(0, 1), {1})),            # 3: the Map dot's actor
                           O.MapUp(O.Dot(1, 30), K, add(O.Dot(1, 2), {2})),           # 4: the key
                           O.MapUp(O.Dot(2, 40), 3, add(O.Dot(A, 3), {3})),           # 5: the Orswot dot's actor
                           O.MapUp(O.Dot(2, 41), 3, add(O.Dot(1, 3), {4, M})),        # 6: a member of an Add
                           O.MapUp(O.Dot(2, 42), 3, orm(O.VClock({0: 2, A: 7}), {5, M})),  # 7: a clock record, a member
                           O.MapRm(O.VClock({3: 50, A: 1}), {1, K})] + good[0][3:],   # 8: a clock record, a keyset key
            good[1]]
    c = make_case("orswot", rng, sent, A, K, M)
    res = ingest_frames(c, enc_frames(extended(c)), gpu_ctx)
    assert host(res.status).tolist() == [wire.MISSING, 0]
    b = res.batch
    actor, key, vactor, keys, key_off, mems, mem_off = (host(x) for x in (b.actor, b.key, b.vactor, b.keys, b.key_off,
                                                                            b.mems, b.mem_off))
    assert actor[3] == -1 and key[4] == -1 and vactor[5] == -1
    assert mems[mem_off[6]:mem_off[7]].tolist() == [4, -1] and mems[mem_off[7]:mem_off[8]].tolist() == [5, -1]
    assert keys[key_off[8]:key_off[9]].tolist() == [1, -1]
    pool, cr = to_host(b.clk_pool), host(b.clk_row)
    assert clock_of(pool, cr[7]) == {0: 2} and clock_of(pool, cr[8]) == {3: 50}
    # the apply that follows skips them and reports its own bit 1 (crdt_map_orswot_apply_batch's status)
    N, Dcap = 2, 16
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)  # noqa: E731
    Vd = cg.map.VD_CAP  # empty Map<u32, Orswot> states, in the fold's output layout
    st = cg.map.MapOrswotLub(clock=z(N, A), ec=z(N, K, A), oc=z(N, K, A), ent=z(N, K, M, A), vd_n=z32(N, K),
                             vd_clock=z(N, K, Vd, A), vd_mem=z(N, K, Vd), flags=z32(N), def_keep=None, def_keys=None)
    slots = [z(N, Dcap, A), z(N, Dcap, 1), z32(N)]
    status = host(cg.map.orswot_apply_batch(st, *slots, b, ctx=gpu_ctx))
    assert [int(x) & 2 for x in status] == [2, 0] and not (status & ~2).any()
    # state 1 had nothing missing: it equals the oracle
    exp = O.Map(O.Orswot)
    for op in good[1]:
        exp.apply(op)
    vn, vc, vm = host(st.vd_n), to_host(st.vd_clock), to_host(st.vd_mem)
    mw = (lambda k, i: vm[1, k, i]) if vm.ndim == 4 else (lambda k, i: vm[1, k, i:i + 1])  # noqa: E731
    vd = {k: [(vc[1, k, i], O.bitmap_members(mw(k, i))) for i in range(int(vn[1, k]))] for k in range(K)}
    dc, dk, cnt = to_host(slots[0]), to_host(slots[1]), host(slots[2])
    dfr = [(dc[1, i], O.bitmap_members(dk[1, i])) for i in range(int(cnt[1]))]
    g = O.dense_to_map_orswot(to_host(st.clock)[1], to_host(st.ec)[1], to_host(st.oc)[1], to_host(st.ent)[1], vd, dfr)
    assert g.clock == exp.clock and g.entries == exp.entries and g.deferred == exp.deferred


@pytest.mark.parametrize("K2", [8, 65])
def test_nested_missing_ids(gpu_ctx, K2):
    from test_gpu_map_nested import _slot_deferred, canon, decode_states, nested_states
    rng = np.random.default_rng(23)
    A, K = 5, 6
    good = [V.random_ops("nested", rng, 8, A, K, K2) for _ in range(2)]
    put = lambda d, j, dots, x: O.MapUp(d, j, O.MVRegPut(O.VClock(dots), x))  # noqa: E731
    sent = [good[0][:3] + [O.MapUp(O.Dot(A, 3), 2, put(O.Dot(0, 1), 1, {0: 1}, 5)),        # 3: the outer dot's actor
                           O.MapUp(O.Dot(1, 30), K, put(O.Dot(1, 2), 1, {1: 2}, 6)),       # 4: the key
                           O.MapUp(O.Dot(2, 40), 3, put(O.Dot(A, 3), 1, {2: 1}, 7)),       # 5: the inner dot's actor
                           O.MapUp(O.Dot(2, 41), 3, put(O.Dot(1, 3), K2, {2: 1}, 8)),      # 6: the inner key of an Up
                           O.MapUp(O.Dot(2, 42), 3, put(O.Dot(1, 4), 2, {2: 40, A: 9}, 9)),  # 7: a Put clock record
                           O.MapUp(O.Dot(2, 43), 3, O.MapRm(O.VClock({0: 2, A: 7}), {K2 - 1, 1, K2})),  # 8: an inner Rm's key
                           O.MapRm(O.VClock({3: 50, A: 1}), {1, K})] + good[0][3:],        # 9
            good[1]]
    kept = [good[0][:3] + [put_ for put_ in [O.MapUp(O.Dot(2, 42), 3, put(O.Dot(1, 4), 2, {2: 40}, 9)),
                                              O.MapUp(O.Dot(2, 43), 3, O.MapRm(O.VClock({0: 2}), {K2 - 1, 1})),
                                              O.MapRm(O.VClock({3: 50}), {1})]] + good[0][3:], good[1]]
    c = make_case("nested", rng, sent, A, K, K2)
    res = ingest_frames(c, enc_frames(extended(c)), gpu_ctx)
    assert host(res.status).tolist() == [wire.MISSING, 0]
    b = res.batch
    actor, key, iactor, ikey, keys, key_off = (host(x) for x in (b.actor, b.key, b.iactor, b.ikey, b.keys, b.key_off))
    assert actor[3] == -1 and key[4] == -1 and iactor[5] == -1 and ikey[6] == -1 and ikey[7] == 2
    assert keys[key_off[9]:key_off[10]].tolist() == [1, -1]
    mask = to_host(b.ikeys).reshape(len(actor), -1)[8]  # the missing inner key is left out: a mask has no slot for it
    assert O.bitmap_members(mask) == {1, K2 - 1}
    pool, cr = to_host(b.clk_pool), host(b.clk_row)
    assert clock_of(pool, cr[7]) == {2: 40} and clock_of(pool, cr[8]) == {0: 2} and clock_of(pool, cr[9]) == {3: 50}
    maps = [O.Map(lambda: O.Map(O.MVReg)) for _ in range(2)]
    st, slots, _ = nested_states(maps, K, K2, A)
    status = host(cg.map.nested_apply_batch(st, *slots, b, ctx=gpu_ctx))
    assert [int(x) & 2 for x in status] == [2, 0] and not (status & ~2).any()
    for s in range(2):
        exp = O.Map(lambda: O.Map(O.MVReg))
        for op in kept[s]:
            exp.apply(op)
        assert canon(decode_states(st, s, _slot_deferred(slots, s))) == canon(exp), s


# ---- 8. the no-sync path and capacities ---------------------------------------------------------------
CANARY = 0x5A


def raw_ingest(ctx, c, data, off, caps, sizing=False):
    """The C entry point with caller-made buffers: 4 canary elements after every capacity."""
    kind = c.kind
    N, A = off.shape[0] - 1, c.A
    tensors = c.dicts()
    fn = f"crdt_map_{FN[kind]}_ops_ingest"
    status = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    head = (dptr(data), dptr(off), N, *dict_args(c, tensors))
    firsts = ("row_off", "key_first") + (("mem_first",) if kind == "orswot" else ())
    tot = (ctypes.c_uint64 * 4)()
    if sizing:
        ctx.call(fn, *head, None, *((None,) * len(firsts)), dptr(status), tot)
        return tuple(int(x) for x in tot), host(status)
    n, r, k, m = caps
    K2w = wire._k2w(len(c.vid)) if kind == "nested" else 1
    sizes = dict(op_off=N + 1, clk_pool=r * A, key_off=n + 1, keys=k, mem_off=n + 1, mems=m, ikeys=n * K2w)
    mk = lambda cnt, dt: torch.full((cnt + 4,), CANARY, dtype=dt, device=DEV)  # noqa: E731
    bufs = {nm: mk(sizes.get(nm, n), wire._VOPS_DTYPES.get(nm, (torch.int64,))[0]) for nm in BATCH[kind]._fields}
    for nm in firsts:
        bufs[nm] = mk(N + 1, torch.int64)
    b = BUF[kind]()
    b.op_cap, b.row_cap, b.key_cap = n, r, k
    if kind == "orswot":
        b.mem_cap = m
    for nm in BATCH[kind]._fields:
        setattr(b, nm, dptr(bufs[nm]))
    ctx.call(fn, *head, ctypes.byref(b), *(dptr(bufs[nm]) for nm in firsts), dptr(status), None)
    sizes.update({nm: N + 1 for nm in firsts})
    return {nm: host(t) for nm, t in bufs.items()}, host(status), {nm: sizes.get(nm, n) for nm in bufs}


CUTS = [(k, w) for k in KINDS for w in ("ops", "rows", "keys")] + [("orswot", "mems")]


@pytest.mark.parametrize("kind,which", CUTS)
def test_capacities_cut_between_states(gpu_ctx, kind, which):
    c = case(kind, 0)
    N, A = len(c.streams), c.A
    want = ref(c)
    data, off = dev_frames(enc_frames(c))
    (op_off, row_off, key_first, mem_first), totals = layout(kind, want)
    got_totals, st = raw_ingest(gpu_ctx, c, data, off, None, sizing=True)
    assert got_totals == totals and not st.any()
    # the first state at or past N/2 that adds to the cut quantity: the capacity ends right before it
    names = ["ops", "rows", "keys", "mems"]
    per = dict(zip(names, (op_off, row_off, key_first, mem_first)))[which]
    cut = next(s for s in range(N // 2, N) if per[s + 1] > per[s])
    caps = list(totals)
    caps[names.index(which)] = int(per[cut + 1]) - 1
    got, st, sizes = raw_ingest(gpu_ctx, c, data, off, caps)
    assert not st[:cut].any() and (st[cut:] == wire.CAP).all()
    firsts = {"op_off": op_off, "row_off": row_off, "key_first": key_first}
    if kind == "orswot":
        firsts["mem_first"] = mem_first
    for nm, w in firsts.items():
        assert got[nm][:cut + 1].tolist() == w[:cut + 1].tolist() and (got[nm][cut + 1:N + 1] == w[cut]).all(), nm
    # the states before the cut: a prefix equal to an uncut call
    n, r, k, m = int(op_off[cut]), int(row_off[cut]), int(key_first[cut]), int(mem_first[cut])
    K2w = wire._k2w(len(c.vid)) if kind == "nested" else 1
    upto = dict(op_off=cut + 1, clk_pool=r * A, key_off=n + 1, keys=k, mem_off=n + 1, mems=m, ikeys=n * K2w)
    for nm in want._fields:
        cnt = upto.get(nm, n)
        assert np.array_equal(got[nm][:cnt], host(getattr(want, nm)).reshape(-1)[:cnt]), nm
    # nothing past a capacity: the guard words stand
    for nm, a in got.items():
        assert (a[sizes[nm]:] == CANARY).all() and len(a) == sizes[nm] + 4, nm


@pytest.mark.parametrize("kind", KINDS)
def test_no_sync_wrapper_with_room(gpu_ctx, kind):
    c = case(kind, 0)
    want = ref(c)
    _, totals = layout(kind, want)
    n, r, k, m = totals
    caps = (n + 5, r + 3, k + 9) + ((m + 7,) if kind == "orswot" else ())
    res = ingest(c, gpu_ctx, sync=False, caps=caps)
    sync = ingest(c, gpu_ctx)
    assert res.totals is None and not host(res.status).any()
    for nm in ("status", "row_off", "key_first") + (("mem_first",) if kind == "orswot" else ()):
        assert np.array_equal(host(getattr(res, nm)), host(getattr(sync, nm))), nm
    K2w = wire._k2w(len(c.vid)) if kind == "nested" else 1
    upto = dict(op_off=len(c.streams) + 1, clk_pool=r * c.A, key_off=n + 1, keys=k, mem_off=n + 1, mems=m, ikeys=n * K2w)
    for nm in want._fields:
        cnt = upto.get(nm, n)
        assert np.array_equal(host(getattr(res.batch, nm)).reshape(-1)[:cnt], host(getattr(sync.batch, nm)).reshape(-1)[:cnt]), nm
    # the capacity-sized batch goes back out as the same frames
    off, data, status = egress(c, res.batch, gpu_ctx)
    assert not host(status).any() and frames_of(off, data) == enc_frames(c)


# ---- 9. replication over the wire -----------------------------------------------------------------------
def test_replication_over_the_wire(gpu_ctx):
    """Two replicas of N Map<u32, PNCounter> states each apply their own op stream, ship it as frames
    (egress on the sender, ingest on the receiver) and apply the other's: both sides equal the oracle
    state that applied both streams."""
    N, K, A, W, Dcap = 6, 8, 6, 2, 16
    rng = np.random.default_rng(41)
    c = make_case("pn", rng, [], A, K, 0)

    def own_ops(actors):
        """Per state: ops a replica holding `actors` makes on its own state (its dots ascend), removes included."""
        streams = []
        for _ in range(N):
            m, ops = O.Map(O.PNCounter), []
            for _ in range(int(rng.integers(20, 40))):
                a, k = int(rng.choice(actors)), int(rng.integers(K))
                if rng.random() < 0.75 or not m.entries:
                    e = m.entries.get(k)
                    cnt = (e.val.p if rng.random() < 0.5 else e.val.n).inner.get(a) + 1 if e is not None else 1
                    way = POS if rng.random() < 0.5 else NEG
                    op = O.MapUp(O.Dot(a, m.clock.get(a) + 1), k, (O.Dot(a, cnt), way))
                else:
                    k = int(rng.choice(sorted(m.entries)))
                    op = O.MapRm(O.VClock(dict(m.entries[k].clock.dots)), {k})
                m.apply(op)
                ops.append(op)
            streams.append(ops)
        return streams

    sx, sy = own_ops([0, 1, 2]), own_ops([3, 4, 5])
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)  # noqa: E731
    new_state = lambda: [z(N, A), z(N, K, A), z(N, K, W, A), z(N, Dcap, A), z(N, Dcap, 1),  # noqa: E731
                         torch.zeros(N, dtype=torch.int32, device=DEV)]
    X, Y = new_state(), new_state()
    bx, by = ref(c, sx), ref(c, sy)
    for st, b in ((X, bx), (Y, by)):  # each side applies its own ops
        assert not host(cg.map.counter_apply_batch(*st, b, ctx=gpu_ctx)).any()

    def ship(b, to, sent):
        off, data, est = egress(c, b, gpu_ctx)
        assert not host(est).any()
        frames = frames_of(off, data)
        back = ingest_frames(c, frames, gpu_ctx)
        assert not host(back.status).any()
        assert not host(cg.map.counter_apply_batch(*to, back.batch, ctx=gpu_ctx)).any()
        # what a peer running the reference would decode
        assert [[V.op_key("pn", o) for o in V.dec_frame("pn", f, c.aid, c.kid)] for f in frames] == \
            [[V.op_key("pn", o) for o in s] for s in sent]

    ship(bx, Y, sx)
    ship(by, X, sy)
    for st, first, then in ((X, sx, sy), (Y, sy, sx)):
        cc, e, v, dc, dk = (to_host(t) for t in st[:5])
        cnt = host(st[5])
        for s in range(N):
            exp = O.Map(O.PNCounter)
            for op in first[s] + then[s]:
                exp.apply(op)
            dfr = [(dc[s, i], O.bitmap_members(dk[s, i])) for i in range(int(cnt[s]))]
            assert O.dense_to_map_counter(cc[s], e[s], v[s], dfr) == exp, s
    assert all(to_host(a).tolist() == to_host(b).tolist() for a, b in zip(X[:3], Y[:3]))  # converged
