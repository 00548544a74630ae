"""GPU: the batched ReadCtx reads of the value-typed Maps (crdt_map_counter_get, crdt_map_orswot_get,
crdt_map_orswot_contains, crdt_map_nested_get, crdt_map_nested_get_inner and the whole-state
compositions) against the oracle objects' own get / contains / read / len (map.rs:233-262,
orswot.rs:253-279, gcounter.rs:70-72, pncounter.rs:110-114, mvreg.rs:183-215).  States are op-replay
objects folded alone on the device; queries are every (state, key[, member | inner key]) in shuffled
order with duplicates, plus one per axis with that index one past its range (status 2, zero outputs);
every output array is compared whole."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle as O
import vmap_read_util as U
from gpu_util import to_dev, to_host
from vmap_read_util import i32

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi  # noqa: E402

N, K = 6, 5
COUNTER = ("present", "val", "total")
OGET = ("present", "val_clock", "members", "len", "vd_n")
NGET = ("present", "val_clock", "ikeys", "len")
INNER = ("present", "vclk", "vval", "nval", "val_clock")


def _absent_key(m):
    return next(k for k in range(K) if k not in m.entries)


# ---- Map<K, GCounter / PNCounter> ------------------------------------------------------------------
@pytest.mark.parametrize("W,A,seed,steps", [(1, 3, 14, 160), (2, 5, 12, 160), (2, 70, 13, 600)])
def test_counter_get(gpu_ctx, W, A, seed, steps):
    maps = O.map_counter_objects(N, K, A, W, seed=seed, steps=steps)
    exps = U.folded(maps)
    npresent = sum(len(m.entries) for m in exps)
    assert 0 < npresent < N * K, "some keys present and some absent"
    totals = [e.val.read() for m in exps for e in m.entries.values()]
    if W == 2:
        assert min(totals) < 0 < max(totals), "totals of both signs"
    if A >= 70:
        used = {a for m in exps for e in m.entries.values() for a in O.counter_rows(e.val, A).any(0).nonzero()[0]}
        assert max(used) >= 64, "an actor past the first lane word"
    res, _, _ = U.counter_states(gpu_ctx, maps, K, A, W)
    (qs, qk), bad = U.queries(np.random.default_rng(seed), (N, K))
    rc, status = cg.map.counter_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    U.assert_same(U.got_arrays(rc, status, COUNTER), U.expect_counter_get(exps, qs, qk, bad, A, W))
    # the whole-state composition
    rd = cg.map.counter_read(res, ctx=gpu_ctx)
    keys, lens, total = to_host(rd.val.keys), rd.val.len.cpu().numpy(), to_host(rd.val.total)
    assert rd.add_clock is res.clock and rd.rm_clock is res.clock
    for s, m in enumerate(exps):
        assert np.array_equal(keys[s], U.bits(m.entries.keys(), 1)) and lens[s] == m.len().val, s
        for k in range(K):
            e = m.entries.get(k)
            assert np.array_equal(total[s, k], U.total_words(e.val.read() if e else 0)), (s, k)


def _hand_counters(W, A):
    """Three states of two keys: several counters of 2^64 - 1 (the carry into the high word), a
    PNCounter with N > P (a negative total), an absent key."""
    big = (1 << 64) - 1
    ec = np.zeros((3, 2, A), np.uint64)
    val = np.zeros((3, 2, W, A), np.uint64)
    ec[0, 0, 0] = ec[0, 1, 1] = ec[1, 0, A - 1] = ec[2, 1, 0] = 1
    val[0, 0, 0, :] = big                      # A counters of 2^64 - 1
    val[0, 1, 0, ::2] = big                    # every other one
    val[1, 0, 0, 0], val[1, 0, 0, A - 1] = 5, big
    val[2, 1, 0, A // 2] = 7
    if W == 2:
        val[0, 0, 1, 0] = 3                    # P - N still positive, a borrow from the high word
        val[0, 1, 1, :] = big                  # N > P: negative, high word borrowed
        val[1, 0, 1, :2] = big
        val[2, 1, 1, A - 1] = 9                # 7 - 9
    return ec, val


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("A", [5, 70])
def test_counter_totals_hand_built(gpu_ctx, W, A):
    ec, val = _hand_counters(W, A)
    st = SimpleNamespace(clock=to_dev(np.ones((3, A), np.uint64)), ec=to_dev(ec), val=to_dev(val))
    qs, qk = [0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]
    rc, status = cg.map.counter_get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    total, present = to_host(rc.val.total), rc.val.present.cpu().numpy()
    neg = hi = 0
    for q, (s, k) in enumerate(zip(qs, qk)):
        want = sum(int(x) for x in val[s, k, 0]) - (sum(int(x) for x in val[s, k, 1]) if W == 2 else 0)
        assert present[q] == int(ec[s, k].any())
        assert np.array_equal(total[q], U.total_words(want)), (q, want, total[q])
        neg += want < 0
        hi += want >= 1 << 64
    assert hi > 0 and (W == 1 or neg > 0)
    assert not status.cpu().numpy().any()
    assert np.array_equal(to_host(rc.val.val), val[qs, qk])
    whole = to_host(cg.map.counter_read(st, ctx=gpu_ctx).val.total)
    assert np.array_equal(whole[qs, qk], total)


def test_counter_get_strided_states(gpu_ctx):
    """val_stride > K*W*A and ec_stride > K*A: the states as views of wider rows."""
    W, A, seed = 2, 5, 12
    maps = O.map_counter_objects(N, K, A, W, seed=seed, steps=160)
    exps = U.folded(maps)
    res, _, _ = U.counter_states(gpu_ctx, maps, K, A, W)
    pad = lambda t, n: torch.full((N, n + 7), -1, dtype=torch.int64, device="cuda:0")  # noqa: E731
    bc, be, bv = pad(res.clock, A), pad(res.ec, K * A), pad(res.val, K * W * A)
    st = SimpleNamespace(clock=bc[:, :A], ec=be[:, :K * A].unflatten(1, (K, A)),
                         val=bv[:, :K * W * A].unflatten(1, (K, W, A)))
    st.clock.copy_(res.clock), st.ec.copy_(res.ec), st.val.copy_(res.val)
    assert st.val.stride(0) > K * W * A and st.ec.stride(0) > K * A and not st.val.is_contiguous()
    (qs, qk), bad = U.queries(np.random.default_rng(5), (N, K))
    rc, status = cg.map.counter_get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    U.assert_same(U.got_arrays(rc, status, COUNTER), U.expect_counter_get(exps, qs, qk, bad, A, W))
    with pytest.raises(ValueError, match="packed"):
        cg.map.counter_read(st, ctx=gpu_ctx)


@pytest.mark.parametrize("Q", [0, 1, 37, 20000])
def test_counter_get_query_counts(gpu_ctx, Q):
    """Q = 0 launches nothing; 20,000 queries are more than the grid's waves, so the grid-stride loop
    runs more than once per wave."""
    Ns, Ks, A, W = 50, 7, 4, 2
    rng = np.random.default_rng(Q)
    ec = rng.integers(0, 3, size=(Ns, Ks, A)).astype(np.uint64) * (rng.random((Ns, Ks, 1)) < 0.6)
    val = rng.integers(0, 1 << 63, size=(Ns, Ks, W, A)).astype(np.uint64) * ec.any(-1)[:, :, None, None]
    clock = rng.integers(1, 9, size=(Ns, A)).astype(np.uint64)
    st = SimpleNamespace(clock=to_dev(clock), ec=to_dev(ec), val=to_dev(val))
    qs, qk = rng.integers(0, Ns, size=Q), rng.integers(0, Ks, size=Q)
    rc, status = cg.map.counter_get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    assert rc.add_clock.shape == (Q, A) and rc.val.total.shape == (Q, 2) and status.shape == (Q,)
    if Q == 0:
        return
    assert np.array_equal(to_host(rc.add_clock), clock[qs]) and np.array_equal(to_host(rc.rm_clock), ec[qs, qk])
    present = ec[qs, qk].any(-1)
    assert 0 < present.sum() or Q == 1
    assert np.array_equal(rc.val.present.cpu().numpy(), present.astype(np.uint8))
    assert np.array_equal(to_host(rc.val.val), val[qs, qk])
    want = [U.total_words(sum(int(x) for x in v[0]) - sum(int(x) for x in v[1])) for v in val[qs, qk]]
    assert np.array_equal(to_host(rc.val.total), np.array(want, np.uint64))
    assert not status.cpu().numpy().any()


# ---- Map<K, Orswot<M>> -----------------------------------------------------------------------------
def _orswot_case(M, A, seed, steps):
    maps = O.map_orswot_objects(N, K, M, A, seed=seed, steps=steps)
    if not any(not e.val.entries for m in U.folded(maps) for e in m.entries.values()):
        # a present key holding an empty set: an Up whose Orswot op removes from the default set
        m = maps[0]
        k = _absent_key(m)
        m.apply(m.update(k, m.get(k).derive_add_ctx(0), lambda v, c: v.rm(0, v.contains(0).derive_rm_ctx())))
    exps = U.folded(maps)
    sets = [e.val for m in exps for e in m.entries.values()]
    assert 0 < len(sets) < N * K, "some keys present and some absent"
    assert any(not v.entries for v in sets), "a present key holding an empty set"
    assert any(v.deferred for v in sets), "a nested deferred remove pending"
    mems = {x for v in sets for x in v.entries}
    if M == 130:
        assert any(64 <= x < 128 for x in mems) and any(x >= 128 for x in mems), "members in every bitmap word"
    if A >= 70:
        assert max(a for v in sets for c in v.entries.values() for a in c.dots) >= 64
    return maps, exps


ORSWOT_CASES = [(4, 5, 21, 160), (70, 6, 22, 160), (130, 8, 23, 300), (4, 80, 24, 800),
                # the scan's narrow and middle lane segments: 1, 2 and 16 lanes per row (16-byte pieces)
                (5, 2, 40, 160), (5, 4, 42, 160), (6, 32, 40, 400),
                # a row longer than its 64-lane segment (70 pieces): the rest-of-row loop
                (4, 140, 50, 1200)]


@pytest.mark.parametrize("M,A,seed,steps", ORSWOT_CASES)
def test_orswot_get_and_contains(gpu_ctx, M, A, seed, steps):
    maps, exps = _orswot_case(M, A, seed, steps)
    res, _, _ = U.orswot_states(gpu_ctx, maps, K, M, A)
    rng = np.random.default_rng(seed)
    (qs, qk), bad = U.queries(rng, (N, K))
    rc, status = cg.map.orswot_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, OGET)
    U.assert_same(got, U.expect_orswot_get(exps, qs, qk, bad, A, M))
    assert got["vd_n"].max() > 0 and ((got["present"] == 1) & (got["len"] == 0)).any()
    (qs, qk, qm), bad = U.queries(rng, (N, K, M))
    rc, status = cg.map.orswot_contains(res, i32(qs), i32(qk), i32(qm), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, None)
    U.assert_same(got, U.expect_orswot_contains(exps, qs, qk, qm, bad, A))
    assert 0 < got["val"].sum() < len(qs)
    # the whole-state composition
    rd = cg.map.orswot_read(res, ctx=gpu_ctx)
    keys, lens, members, mlens = (to_host(rd.val.keys), rd.val.len.cpu().numpy(), to_host(rd.val.members),
                                  rd.val.lens.cpu().numpy())
    assert rd.add_clock is res.clock and members.shape == (N, K, (M + 63) // 64)
    for s, m in enumerate(exps):
        assert np.array_equal(keys[s], U.bits(m.entries.keys(), 1)) and lens[s] == m.len().val, s
        for k in range(K):
            want = m.entries[k].val.read().val if k in m.entries else set()
            assert np.array_equal(members[s, k], U.bits(want, (M + 63) // 64)) and mlens[s, k] == len(want), (s, k)


# ---- Map<K, Map<K2, MVReg>> ------------------------------------------------------------------------
def _nested_put(m, k, j, actor, x):
    m.apply(m.update(k, m.get(k).derive_add_ctx(actor),
                     lambda v, c: v.update(j, c, lambda reg, cx: reg.write(x, cx))))


def _nested_case(K2, A, seed, steps):
    maps = O.nested_map_objects(N, K, K2, A, seed=seed, steps=steps)
    if K2 == 70:  # the generator's largest inner key is below 64: an Up on inner key 69
        _nested_put(maps[1], next(iter(maps[1].entries)), 69, 1, 7001)
    if A >= 70:   # an actor past the first lane word
        _nested_put(maps[2], next(iter(maps[2].entries)), 1, A - 1, 7002)
    if not any(not e.val.entries for m in U.folded(maps) for e in m.entries.values()):
        # a present key holding an empty inner Map: an Up whose inner op removes from the default Map
        m = maps[0]
        k = _absent_key(m)
        m.apply(m.update(k, m.get(k).derive_add_ctx(0), lambda v, c: v.rm(0, v.get(0).derive_rm_ctx())))
    exps = U.folded(maps)
    inner = [e.val for m in exps for e in m.entries.values()]
    assert 0 < len(inner) < N * K, "some keys present and some absent"
    assert any(not v.entries for v in inner), "a present key holding an empty inner Map"
    if K2 == 3 and A == 5:
        assert max(len(ie.val.vals) for v in inner for ie in v.entries.values()) > 1, "a register with two values"
    if K2 == 70:
        assert max(j for v in inner for j in v.entries) >= 64, "an inner key in the second bitmap word"
    if A >= 70:
        assert max(a for m in exps for e in m.entries.values() for a in e.clock.dots) >= 64
    return maps, exps


NESTED_CASES = [(3, 5, 31, 200), (70, 6, 32, 500), (3, 70, 33, 800),
                # 1, 2 and 16 lanes per row
                (3, 2, 41, 200), (3, 4, 42, 200), (3, 32, 40, 500),
                # a row longer than its 64-lane segment
                (3, 140, 52, 1200)]


@pytest.mark.parametrize("K2,A,seed,steps", NESTED_CASES)
def test_nested_get_and_get_inner(gpu_ctx, K2, A, seed, steps):
    maps, exps = _nested_case(K2, A, seed, steps)
    res, _, _ = U.nested_states(gpu_ctx, maps, K, K2, A)
    Vs = res.ivc.shape[3]
    rng = np.random.default_rng(seed)
    (qs, qk), bad = U.queries(rng, (N, K))
    rc, status = cg.map.nested_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, NGET)
    U.assert_same(got, U.expect_nested_get(exps, qs, qk, bad, A, K2))
    assert ((got["present"] == 1) & (got["len"] == 0)).any()
    (qs, qk, qj), bad = U.queries(rng, (N, K, K2))
    rc, status = cg.map.nested_get_inner(res, i32(qs), i32(qk), i32(qj), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, INNER)
    U.assert_same(got, U.expect_nested_get_inner(exps, qs, qk, qj, bad, A, Vs))
    assert 0 < got["present"].sum() < len(qs)
    if K2 == 3 and A == 5:
        assert got["nval"].max() > 1
    # the whole-state composition
    rd = cg.map.nested_read(res, ctx=gpu_ctx)
    keys, lens, ikeys, ilens = (to_host(rd.val.keys), rd.val.len.cpu().numpy(), to_host(rd.val.ikeys),
                                rd.val.lens.cpu().numpy())
    assert rd.add_clock is res.clock and ikeys.shape == (N, K, (K2 + 63) // 64)
    for s, m in enumerate(exps):
        assert np.array_equal(keys[s], U.bits(m.entries.keys(), 1)) and lens[s] == m.len().val, s
        for k in range(K):
            want = set(m.entries[k].val.entries) if k in m.entries else set()
            assert np.array_equal(ikeys[s, k], U.bits(want, (K2 + 63) // 64)) and ilens[s, k] == len(want), (s, k)


def _off_by_a_word(t):
    """The same values at an address 8 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    return out


@pytest.mark.parametrize("A", [6, 32])
def test_scans_on_rows_off_16_byte_alignment(gpu_ctx, A):
    """Even A with ent / iec one word off a 16-byte boundary: the scans take 8-byte pieces (A = 32: 32
    lanes per row) and give what the aligned states give."""
    M, K2 = 6, 3
    seed, steps = (22, 160) if A == 6 else (40, 400)
    maps, exps = _orswot_case(M, A, seed, steps)
    res, _, _ = U.orswot_states(gpu_ctx, maps, K, M, A)
    st = SimpleNamespace(clock=res.clock, ec=res.ec, oc=res.oc, ent=_off_by_a_word(res.ent), vd_n=res.vd_n)
    (qs, qk), bad = U.queries(np.random.default_rng(A), (N, K))
    rc, status = cg.map.orswot_get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, OGET)
    U.assert_same(got, U.expect_orswot_get(exps, qs, qk, bad, A, M))
    assert got["len"].max() > 0
    maps, exps = _nested_case(K2, A, 32 if A == 6 else 40, 500)
    res, _, _ = U.nested_states(gpu_ctx, maps, K, K2, A)
    st = SimpleNamespace(clock=res.clock, ec=res.ec, ic=res.ic, iec=_off_by_a_word(res.iec))
    rc, status = cg.map.nested_get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    got = U.got_arrays(rc, status, NGET)
    U.assert_same(got, U.expect_nested_get(exps, qs, qk, bad, A, K2))
    assert got["len"].max() > 0


# ---- the C entry points directly: every element written, NULL optional outputs, refusals -----------
def _ones(*shape, dtype=torch.int64):
    return torch.full(shape, -1, dtype=dtype, device="cuda:0")


def _raw(ctx, fn, st, index, outs):
    """One ctx.call with every output pre-filled with all-ones (None stays NULL)."""
    Q = index[0].shape[0]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ctx.call(fn, ctypes.byref(st), *[t.data_ptr() for t in index], Q, *[ptr(t) for t in outs])
    torch.cuda.synchronize()
    return outs


def _same(ts, ws):
    for i, (t, w) in enumerate(zip(ts, ws)):
        if t is not None:
            assert torch.equal(t.view(torch.uint8), w.contiguous().view(torch.uint8)), i


def test_every_element_written_counter(gpu_ctx):
    W, A = 2, 5
    maps = O.map_counter_objects(N, K, A, W, seed=12, steps=160)
    res, _, _ = U.counter_states(gpu_ctx, maps, K, A, W)
    (qs, qk), _ = U.queries(np.random.default_rng(1), (N, K))
    idx, Q = [i32(qs), i32(qk)], len(qs)
    rc, status = cg.map.counter_get(res, *idx, ctx=gpu_ctx)
    want = [rc.val.present, rc.rm_clock, rc.val.val, rc.val.total, status]
    st = _abi.MapCounterStates()
    st.N, st.K, st.A, st.W = N, K, A, W
    st.clock, st.clock_stride, st.ec, st.ec_stride = res.clock.data_ptr(), A, res.ec.data_ptr(), K * A
    st.val, st.val_stride = res.val.data_ptr(), K * W * A
    fresh = lambda: [_ones(Q, dtype=torch.uint8), _ones(Q, A), _ones(Q, W, A), _ones(Q, 2),  # noqa: E731
                     _ones(Q, dtype=torch.int32)]
    _same(_raw(gpu_ctx, "crdt_map_counter_get", st, idx, fresh()), want)
    for skip in ((2,), (3,), (2, 3)):  # val and / or total NULL
        outs = fresh()
        for i in skip:
            outs[i] = None
        _same(_raw(gpu_ctx, "crdt_map_counter_get", st, idx, outs), want)


def _orswot_struct(res, M, A):
    st = _abi.MapOrswotStates()
    st.N, st.K, st.M, st.A = N, K, M, A
    st.clock, st.ec, st.oc, st.ent = res.clock.data_ptr(), res.ec.data_ptr(), res.oc.data_ptr(), res.ent.data_ptr()
    st.vd_n, st.vd_clock, st.vd_mem = res.vd_n.data_ptr(), res.vd_clock.data_ptr(), res.vd_mem.data_ptr()
    return st


def test_every_element_written_orswot(gpu_ctx):
    M, A = 70, 6
    maps, _ = _orswot_case(M, A, 22, 160)
    res, _, _ = U.orswot_states(gpu_ctx, maps, K, M, A)
    st = _orswot_struct(res, M, A)
    (qs, qk), _ = U.queries(np.random.default_rng(2), (N, K))
    idx, Q = [i32(qs), i32(qk)], len(qs)
    rc, status = cg.map.orswot_get(res, *idx, ctx=gpu_ctx)
    want = [rc.val.present, rc.rm_clock, rc.val.val_clock, rc.val.members, rc.val.len, rc.val.vd_n, status]
    fresh = lambda: [_ones(Q, dtype=torch.uint8), _ones(Q, A), _ones(Q, A), _ones(Q, 2),  # noqa: E731
                     _ones(Q, dtype=torch.int32), _ones(Q, dtype=torch.int32), _ones(Q, dtype=torch.int32)]
    _same(_raw(gpu_ctx, "crdt_map_orswot_get", st, idx, fresh()), want)
    outs = fresh()
    outs[5] = None  # vd_n NULL
    _same(_raw(gpu_ctx, "crdt_map_orswot_get", st, idx, outs), want)
    (qs, qk, qm), _ = U.queries(np.random.default_rng(3), (N, K, M))
    idx, Q = [i32(qs), i32(qk), i32(qm)], len(qs)
    rc, status = cg.map.orswot_contains(res, *idx, ctx=gpu_ctx)
    outs = [_ones(Q, dtype=torch.uint8), _ones(Q, A), _ones(Q, A), _ones(Q, dtype=torch.int32)]
    _same(_raw(gpu_ctx, "crdt_map_orswot_contains", st, idx, outs), [rc.val, rc.add_clock, rc.rm_clock, status])


def _nested_struct(res, K2, A):
    st = _abi.MapNestedStates()
    st.N, st.K, st.K2, st.A, st.Vs, st.Id = N, K, K2, A, res.ivc.shape[3], res.id_clock.shape[2]
    for nm in ("clock", "ec", "ic", "iec", "ivc", "ivv", "nval", "id_n", "id_clock", "id_keys"):
        setattr(st, nm, getattr(res, nm).data_ptr())
    return st


def test_every_element_written_nested(gpu_ctx):
    K2, A = 3, 5
    maps, _ = _nested_case(K2, A, 31, 200)
    res, _, _ = U.nested_states(gpu_ctx, maps, K, K2, A)
    st, Vs = _nested_struct(res, K2, A), res.ivc.shape[3]
    (qs, qk), _ = U.queries(np.random.default_rng(4), (N, K))
    idx, Q = [i32(qs), i32(qk)], len(qs)
    rc, status = cg.map.nested_get(res, *idx, ctx=gpu_ctx)
    outs = [_ones(Q, dtype=torch.uint8), _ones(Q, A), _ones(Q, A), _ones(Q, 1), _ones(Q, dtype=torch.int32),
            _ones(Q, dtype=torch.int32)]
    _same(_raw(gpu_ctx, "crdt_map_nested_get", st, idx, outs),
          [rc.val.present, rc.rm_clock, rc.val.val_clock, rc.val.ikeys, rc.val.len, status])
    (qs, qk, qj), _ = U.queries(np.random.default_rng(5), (N, K, K2))
    idx, Q = [i32(qs), i32(qk), i32(qj)], len(qs)
    rc, status = cg.map.nested_get_inner(res, *idx, ctx=gpu_ctx)
    outs = [_ones(Q, dtype=torch.uint8), _ones(Q, A), _ones(Q, A), _ones(Q, Vs, A), _ones(Q, Vs),
            _ones(Q, dtype=torch.int32), _ones(Q, A), _ones(Q, dtype=torch.int32)]
    _same(_raw(gpu_ctx, "crdt_map_nested_get_inner", st, idx, outs),
          [rc.val.present, rc.add_clock, rc.rm_clock, rc.val.vclk, rc.val.vval, rc.val.nval, rc.val.val_clock, status])


def test_refusals(gpu_ctx):
    """NULL states and a too-small stride are CRDT_EINVAL, a dimension past its limit CRDT_EUNSUPPORTED
    naming the limit; all before anything is launched."""
    A, Q = 4, 2
    idx = i32([0, 0])
    u8, w, u32 = _ones(Q, dtype=torch.uint8), _ones(Q, 64 * A), _ones(Q, dtype=torch.int32)
    p = lambda *ts: [t.data_ptr() for t in ts]  # noqa: E731
    calls = {
        "crdt_map_counter_get": lambda st: p(idx, idx) + [Q] + p(u8, w, w, w, u32),
        "crdt_map_orswot_get": lambda st: p(idx, idx) + [Q] + p(u8, w, w, w, u32, u32, u32),
        "crdt_map_orswot_contains": lambda st: p(idx, idx, idx) + [Q] + p(u8, w, w, u32),
        "crdt_map_nested_get": lambda st: p(idx, idx) + [Q] + p(u8, w, w, w, u32, u32),
        "crdt_map_nested_get_inner": lambda st: p(idx, idx, idx) + [Q] + p(u8, w, w, w, w, u32, w, u32),
    }
    for fn, args in calls.items():
        with pytest.raises(cg.CrdtGpuError) as e:
            gpu_ctx.call(fn, None, *args(None))
        assert e.value.code == _abi.CRDT_EINVAL, fn
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    c = _abi.MapCounterStates()
    c.N, c.K, c.A, c.W = 2, 3, A, 2
    c.clock, c.ec, c.val = buf.data_ptr(), buf.data_ptr(), buf.data_ptr()
    c.clock_stride, c.ec_stride, c.val_stride = A, 3 * A, 3 * 2 * A - 1
    with pytest.raises(cg.CrdtGpuError, match="stride") as e:
        gpu_ctx.call("crdt_map_counter_get", ctypes.byref(c), *calls["crdt_map_counter_get"](c))
    assert e.value.code == _abi.CRDT_EINVAL
    c.ec_stride, c.val_stride = 3 * A - 1, 3 * 2 * A
    with pytest.raises(cg.CrdtGpuError, match="stride"):
        gpu_ctx.call("crdt_map_counter_get", ctypes.byref(c), *calls["crdt_map_counter_get"](c))
    o = _abi.MapOrswotStates()
    o.N, o.K, o.M, o.A = 1, 1, 1025, A
    for fn in ("crdt_map_orswot_get", "crdt_map_orswot_contains"):
        with pytest.raises(cg.CrdtGpuError, match="1024") as e:
            gpu_ctx.call(fn, ctypes.byref(o), *calls[fn](o))
        assert e.value.code == _abi.CRDT_EUNSUPPORTED, fn
    for K2, Vs, limit in ((257, 8, "256"), (3, 65, "64")):
        n = _abi.MapNestedStates()
        n.N, n.K, n.K2, n.A, n.Vs = 1, 1, K2, A, Vs
        for fn in ("crdt_map_nested_get", "crdt_map_nested_get_inner"):
            with pytest.raises(cg.CrdtGpuError, match=limit) as e:
                gpu_ctx.call(fn, ctypes.byref(n), *calls[fn](n))
            assert e.value.code == _abi.CRDT_EUNSUPPORTED, (fn, K2, Vs)
    torch.cuda.synchronize()
    assert (u8 == 255).all() and (u32 == -1).all() and (w == -1).all(), "nothing was launched"
