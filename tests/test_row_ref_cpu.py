"""row_ref.py's NumPy restatements against the oracle's objects (VClock, GCounter, PNCounter,
Orswot, Map<K, MVReg>, LWWReg) on small random cases drawn from edge_counters: counters on both
sides of the sign bit and of the u64 wrap.  No GPU: this is what lets the GPU tests compare bit for
bit against row_ref at sizes where one object per row would be too slow."""
import numpy as np

import oracle as O
import row_ref as RR

CODE = {O.EQUAL: 0, O.GREATER: 1, O.LESS: -1, O.NONE: 2}


def vc(row):
    return O.VClock({a: int(c) for a, c in enumerate(np.asarray(row).tolist()) if c})


def dense(v, A):
    r = np.zeros(A, np.uint64)
    for a, c in v.dots.items():
        r[a] = c
    return r


def test_edge_counters_draw_every_edge_and_small_values():
    c = RR.edge_counters(np.random.default_rng(0), (400, 9), 0.4)
    assert c.dtype == np.uint64
    assert set(RR.EDGES.tolist()) <= set(c.reshape(-1).tolist())
    assert {2, 3, 4, 5} <= set(c.reshape(-1).tolist())
    assert (c >> np.uint64(63)).any() and not (c >> np.uint64(63)).all()


def test_pair_and_cmp_refs():
    seen = set()
    for seed, (N, A) in enumerate([(200, 1), (200, 5), (200, 6), (64, 33)]):
        x, y = RR.edge_pairs(np.random.default_rng(seed), N, A)
        glb, fgt, inter = (RR.pair_ref(op, x, y) for op in (RR.GLB, RR.FORGET, RR.INTERSECTION))
        cmpv = RR.cmp_ref(x, y)
        for i in range(N):
            a, b = vc(x[i]), vc(y[i])
            g = a.copy()
            g.glb(b)
            f = a.copy()
            f.forget(b)
            assert np.array_equal(glb[i], dense(g, A)), i
            assert np.array_equal(fgt[i], dense(f, A)), i
            assert np.array_equal(fgt[i], dense(a.clone_without(b), A)), i
            assert np.array_equal(inter[i], dense(O.VClock.intersection(a, b), A)), i
            assert cmpv[i] == CODE[a.partial_cmp(b)], i
        if A > 1:
            assert set(cmpv.tolist()) == {0, 1, -1, 2}, (N, A)  # the pair generator's promise
        seen |= set(cmpv.tolist())
    assert seen == {0, 1, -1, 2}


def test_cmp_matrix_ref():
    rng = np.random.default_rng(7)
    x = RR.edge_counters(rng, (24, 5), 0.4, small=3)
    x[::5] = x[0]
    m = RR.cmp_matrix_ref(x)
    assert m.shape == (24, 24) and m.dtype == np.int8
    for i in range(24):
        for j in range(24):
            assert m[i, j] == CODE[vc(x[i]).partial_cmp(vc(x[j]))], (i, j)
    assert set(m.reshape(-1).tolist()) == {0, 1, -1, 2}


def test_sum128_ref():
    rng = np.random.default_rng(8)
    for A in (1, 6, 7, 40):
        g = RR.edge_counters(rng, (100, A), 0.6)
        got = RR.sum128_ref(g)
        for i in range(100):
            c = O.GCounter()
            c.inner = vc(g[i])
            assert got[i] == c.read(), i
        pn = RR.edge_counters(rng, (100, 2 * A), 0.6)
        got = RR.sum128_ref(pn, pn=True)
        for i in range(100):
            c = O.PNCounter()
            c.p.inner, c.n.inner = vc(pn[i, :A]), vc(pn[i, A:])
            assert got[i] == c.read(), i
        assert min(got) < 0 < max(got) or A == 1
    assert RR.sum128_ref(np.full(5, (1 << 64) - 1, np.uint64)) == [5 * ((1 << 64) - 1)]


def _deferred_case(rng, N, A, D):
    dc = RR.edge_counters(rng, (D, A), 0.3)
    st = rng.integers(0, N, size=D).astype(np.int32)
    st[::7] = N + rng.integers(0, 3, size=len(st[::7]))  # rows naming no state
    st[3] = -1
    dc[::5] = 0  # an empty rm clock: dropped by any forget
    return dc, st


def _check_deferred(dc, st, ys, dc2, keep):
    """Each deferred row alone in an Orswot of its state, through Orswot::forget."""
    N, A = ys.shape
    for d in range(dc.shape[0]):
        s = int(st[d]) & 0xFFFFFFFF
        if s >= N:
            assert np.array_equal(dc2[d], dc[d]) and keep[d] == 1, d
            continue
        o = O.Orswot()
        if dc[d].any():
            o.deferred[vc(dc[d])] = {0}
        o.forget(vc(ys[s]))
        assert bool(keep[d]) == bool(o.deferred), d
        exp = dense(next(iter(o.deferred)), A) if o.deferred else np.zeros(A, np.uint64)
        assert np.array_equal(dc2[d], exp), d


def test_orswot_forget_ref():
    for seed, (N, M, A, shared) in enumerate([(60, 3, 8, False), (40, 5, 7, True), (30, 2, 1, False)]):
        rng = np.random.default_rng(100 + seed)
        clock = RR.edge_counters(rng, (N, A), 0.3)
        entries = RR.edge_counters(rng, (N, M, A), 0.3)
        entries[rng.random((N, M)) < 0.2] = 0
        y = RR.edge_counters(rng, (A,) if shared else (N, A), 0.4)
        dc, st = _deferred_case(rng, N, A, 90)
        c2, e2, dc2, keep = RR.orswot_forget_ref(clock, entries, y, dc, st)
        ys = np.broadcast_to(y, (N, A))
        emptied = 0
        for s in range(N):
            o = O.Orswot()
            o.clock = vc(clock[s])
            o.entries = {m: vc(entries[s, m]) for m in range(M) if entries[s, m].any()}
            o.forget(vc(ys[s]))
            assert np.array_equal(c2[s], dense(o.clock, A)), s
            for m in range(M):
                exp = o.entries.get(m)
                assert np.array_equal(e2[s, m], dense(exp, A) if exp else np.zeros(A, np.uint64)), (s, m)
                emptied += entries[s, m].any() and exp is None
        assert emptied > 0
        _check_deferred(dc, st, ys, dc2, keep)
        assert 0 < keep.sum() < len(keep)
    assert RR.orswot_forget_ref(clock, entries, y)[2:] == (None, None)


def test_map_forget_ref():
    for seed, (N, K, V, A, shared) in enumerate([(40, 4, 2, 8, False), (30, 3, 5, 7, True), (25, 2, 1, 3, False)]):
        rng = np.random.default_rng(200 + seed)
        clock = RR.edge_counters(rng, (N, A), 0.3)
        ec = RR.edge_counters(rng, (N, K, A), 0.3)
        vclk = RR.edge_counters(rng, (N, K, V, A), 0.3)
        vclk[rng.random((N, K, V)) < 0.2] = 0
        vval = (1 + np.arange(N * K * V, dtype=np.uint64)).reshape(N, K, V)  # unique: MVReg == needs it
        y = RR.edge_counters(rng, (A,) if shared else (N, A), 0.4)
        ys = np.broadcast_to(y, (N, A))
        dying = rng.random((N, K)) < 0.3  # the entry clock empties; a value clock would survive
        ec[dying] = np.minimum(ec, ys[:, None, :])[dying]
        dc, st = _deferred_case(rng, N, A, 60)
        c2, ec2, vc2, vv2, dc2, keep = RR.map_forget_ref(clock, ec, vclk, vval, y, dc, st)
        would_survive = (vclk > ys[:, None, None, :]).any(-1).any(-1)
        assert (dying & would_survive).any()
        assert not vc2[dying].any() and not vv2[dying].any()
        assert not vv2[~vc2.any(-1)].any() and np.array_equal(vv2[vc2.any(-1)], vval[vc2.any(-1)])
        for s in range(N):
            m = O.dense_to_map(clock[s], ec[s], vclk[s], vval[s])
            m.forget(vc(ys[s]))
            got = O.dense_to_map(c2[s], ec2[s], vc2[s], vv2[s])
            assert got.clock == m.clock and got.entries == m.entries, s
            # and back through the dense ingest: the same clocks, values compacted to the front
            d = O.map_to_dense([m], K, A, V)
            assert np.array_equal(d["clock"][0], c2[s]) and np.array_equal(d["ec"][0], ec2[s]), s
            for k in range(K):
                live = vc2[s, k].any(-1)
                n = int(live.sum())
                assert np.array_equal(d["vclk"][0, k, :n], vc2[s, k][live]), (s, k)
                assert np.array_equal(d["vval"][0, k, :n], vv2[s, k][live]), (s, k)
                assert not d["vclk"][0, k, n:].any()
        _check_deferred(dc, st, ys, dc2, keep)


def _lww_loop(marker, val, init):
    """The fold as a loop of LWWReg::merge into the init register."""
    reg = O.LWWReg(int(init[1]), int(init[0]))
    first = RR.NONE
    for i, (m, v) in enumerate(zip(marker.tolist(), val.tolist())):
        try:
            reg.merge(O.LWWReg(v, m))
        except O.ConflictingMarker:
            if first == RR.NONE:
                first = i
    return reg.marker, reg.val, first


def test_lww_ref():
    rng = np.random.default_rng(9)
    outcomes = set()
    for case in range(300):
        R = int(rng.integers(1, 12))
        marker = RR.edge_counters(rng, R, 0.4, small=3)
        val = rng.integers(0, 2, size=R).astype(np.uint64)
        # without init: replica 0 starts the fold
        lm, lv, lf = _lww_loop(marker[1:], val[1:], (marker[0], val[0]))
        assert RR.lww_ref(marker, val) == (lm, lv, lf if lf == RR.NONE else lf + 1), case
        init = (int(RR.edge_counters(rng, 1, 0.4, small=3)[0]), int(rng.integers(0, 2)))
        got = RR.lww_ref(marker, val, init)
        assert got == _lww_loop(marker, val, init), case
        outcomes.add((got[0] == init[0], got[2] == RR.NONE, got[2] == 0))
    assert len(outcomes) >= 5  # init wins / loses, with and without conflicts, conflict at replica 0
