"""The reindex calls on the GPU against the numpy statement of the gather (reindex_util) and the
oracle's re-labelled objects: the map builder, rows and bitmaps, Orswot / MVReg / Map states, pure
growth against eq_util.widen, the status word's four bits, and the edges.  N = 257, so the last wave
is partly idle."""
import ctypes

import numpy as np
import pytest
import torch

import eq_util as E
import reindex_util as R
from gpu_util import to_dev, to_host
from orswot_apply_util import map_orswot

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N = 257
U1 = np.uint64(1)


def dsrc(src):
    return None if src is None else torch.from_numpy(np.asarray(src).astype(np.int32)).cuda()


def status_of(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def orswot_host(o):
    return dict(clock=to_host(o.clock), entries=to_host(o.entries), dcl=to_host(o.def_clock), dset=to_host(o.def_members),
                cnt=status_of(o.def_count))


def map_host(o):
    return dict(clock=to_host(o.clock), ec=to_host(o.ec), vclk=to_host(o.vclk), vval=to_host(o.vval),
                dcl=to_host(o.def_clock), dset=to_host(o.def_keys), cnt=status_of(o.def_count))


@pytest.fixture(params=["rxlds=1", "rxlds=0"], ids=["lds", "direct"])
def rctx(request, gpu_ctx):
    """Both forms of the column gather: input rows staged in LDS (the default where the rows are 16-byte
    aligned and fit) and 8-byte words read straight from memory."""
    gpu_ctx.tune(request.param)
    yield gpu_ctx
    gpu_ctx.tune("rxlds=1")


def same(got, exp):
    for k in exp:
        assert got[k].shape == exp[k].shape, (k, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), k


# ---- the map builder -------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_index_map(gpu_ctx, n, wide):
    rng = np.random.default_rng(n + wide)
    dt, view = (np.uint64, np.int64) if wide else (np.uint32, np.int32)
    # ids on both sides of the sign bit of their width: the compare is unsigned
    base = (1 << 63) - 2 * n - 40 if wide else (1 << 31) - 2 * n - 40
    old = np.sort(rng.choice(4 * n, size=n, replace=False)).astype(dt) + dt(10 + base)
    free = np.setdiff1d(np.arange(4 * n).astype(dt) + dt(10 + base), old)
    inside = free[(free > old[0]) & (free < old[-1])]
    fresh = [old[0] - dt(3), old[-1] + dt(5)] + ([inside[len(inside) // 2]] if len(inside) else [])
    cases = {
        "same": old,
        "grown": np.sort(np.concatenate([old, np.array(fresh, dt)])),
        "subset": old[::2] if n > 1 else old[:0],
        "mixed": np.sort(np.concatenate([old[1::2], np.array(fresh, dt)])),
    }
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda()  # noqa: E731
    for name, new in cases.items():
        for o in (old, old[:0]):  # and the empty old dictionary
            src, n_lost = cg.reindex.index_map(dev(o), dev(new), ctx=gpu_ctx)
            pos = np.searchsorted(o, new)
            found = (pos < len(o)) & (o[np.minimum(pos, max(len(o) - 1, 0))] == new) if len(o) else np.zeros(len(new), bool)
            exp = np.where(found, pos, -1).astype(np.int32)
            assert np.array_equal(status_of(src), exp), (name, len(o))
            assert int(status_of(n_lost)[0]) == len(o) - int(found.sum()), (name, len(o))
    assert int(status_of(cg.reindex.index_map(dev(old), dev(cases["subset"]), ctx=gpu_ctx)[1])[0]) == n - len(cases["subset"])


# ---- rows and bitmaps ------------------------------------------------------------------------------
def shrink_map(n_in, n_out):
    """n_out of n_in indices, ascending, dropping the last one among others."""
    return np.sort(np.random.default_rng(n_in).choice(n_in - 1, size=n_out, replace=False)).astype(np.int64)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("A_in,A_out", [(3, 5), (32, 34), (64, 65), (65, 64), (130, 200), (300, 301), (1024, 1030),
                                         (504, 506), (506, 508)])
def test_rows(rctx, A_in, A_out, planes):
    """The issue's shapes, and the two widths either side of the LDS staging bound (A_in 504 is the widest row a
    workgroup stages, 506 gathers straight from memory)."""
    rng = np.random.default_rng(A_in * 7 + planes)
    x = rng.integers(1, 2**63, size=(N, planes, A_in), dtype=np.int64).astype(np.uint64)
    x[::3, :, -1] = 0  # a dropped last column is empty in every third row
    x[N - 1, :, -1] = 77
    src = R.insert_map(A_in, A_out - A_in, seed=A_in)[0] if A_out > A_in else shrink_map(A_in, A_out)
    for s in (src, None):
        exp = R.gather(x, s, 2, A_out)
        lost = (x[:, :, R.dropped(s, A_in, A_out)] != 0).any(axis=(1, 2))
        for in_gap, out_gap in ((0, 0), (3, 1), (2, 4)):  # packed; odd strides (8-byte path); even strides
            xin = np.full((N, planes * A_in + in_gap), np.uint64(2**64 - 1), np.uint64)
            xin[:, :planes * A_in] = x.reshape(N, -1)
            full = to_dev(np.full((N, planes * A_out + out_gap), np.uint64(2**64 - 1), np.uint64))
            out, status = cg.reindex.rows(to_dev(xin)[:, :planes * A_in], dsrc(s), A_out, planes=planes,
                                          out=full[:, :planes * A_out], ctx=rctx)
            got = to_host(full)
            assert np.array_equal(got[:, :planes * A_out], exp.reshape(N, -1)), (s is None, in_gap)
            assert (got[:, planes * A_out:] == np.uint64(2**64 - 1)).all(), "the gap between strided rows was written"
            assert np.array_equal(status_of(status), np.where(lost, R.DROPPED, 0)), (s is None, in_gap)
    assert lost[N - 1] or A_out > A_in
    # the per-type forms are these rows
    fn = cg.pncounter.reindex if planes == 2 else cg.vclock.reindex
    out, status = fn(to_dev(x.reshape(N, -1)), dsrc(src), ctx=rctx)
    assert np.array_equal(to_host(out), R.gather(x, src, 2).reshape(N, -1))
    if planes == 1:
        out, _ = cg.gcounter.reindex(to_dev(x.reshape(N, -1)), None, A_out, ctx=rctx)
        assert np.array_equal(to_host(out), R.gather(x, None, 2, A_out).reshape(N, -1))


@pytest.mark.parametrize("U_in,U_out", [(60, 70), (70, 130), (128, 64), (4096, 4100)])
def test_bitmaps(gpu_ctx, U_in, U_out):
    rng = np.random.default_rng(U_in)
    bits = (rng.random((N, U_in)) < 0.4).astype(np.uint8)
    bits[::2, -1] = 0
    bits[N - 1, -1] = 1
    x = R.pack(bits)
    src = R.insert_map(U_in, U_out - U_in, seed=U_in)[0] if U_out > U_in else shrink_map(U_in, U_out)
    for s in (src, None):
        exp = R.pack(R.gather(bits, s, 1, U_out))  # the bits past U_out are zero
        lost = (bits[:, R.dropped(s, U_in, U_out)] != 0).any(axis=1)
        for gap in (0, 1):
            xin = np.full((N, x.shape[1] + gap), np.uint64(2**64 - 1), np.uint64)
            xin[:, :x.shape[1]] = x
            full = to_dev(np.full((N, exp.shape[1] + gap), np.uint64(2**64 - 1), np.uint64))
            out, status = cg.gset.reindex(to_dev(xin)[:, :x.shape[1]], dsrc(s), U_out, ctx=gpu_ctx, U_in=U_in) \
                if gap == 0 else cg.reindex.bitmaps(to_dev(xin)[:, :x.shape[1]], dsrc(s), U_out,
                                                    out=full[:, :exp.shape[1]], ctx=gpu_ctx, bits_in=U_in)
            assert np.array_equal(to_host(out), exp), (s is None, gap)
            if gap:
                assert (to_host(full)[:, exp.shape[1]:] == np.uint64(2**64 - 1)).all()
            assert np.array_equal(status_of(status), np.where(lost, R.DROPPED, 0)), (s is None, gap)
    assert lost[N - 1] or U_out > U_in
    if U_in % 64:  # a stray input bit past U_in is no element: neither gathered nor reported as a loss
        stray = x.copy()
        stray[:, -1] |= U1 << np.uint64(63)
        out, status = cg.reindex.bitmaps(to_dev(stray), dsrc(src), U_out, ctx=gpu_ctx, bits_in=U_in)
        lost = (bits[:, R.dropped(src, U_in, U_out)] != 0).any(axis=1)
        assert np.array_equal(to_host(out), R.pack(R.gather(bits, src, 1, U_out)))
        assert np.array_equal(status_of(status), np.where(lost, R.DROPPED, 0))


# ---- Orswot ----------------------------------------------------------------------------------------
def orswot_case(seed, M, A):
    pool = E.orswot_pool(seed, M, A)
    while not any(o.deferred for o in pool):  # a replay that left deferred removes
        seed += 1
        pool = E.orswot_pool(seed, M, A)
    Dcap = max(len(o.deferred) for o in pool)
    return pool, E.orswot_dense(pool, N, M, A, Dcap), Dcap


@pytest.mark.parametrize("M,A,wide_rows", [(5, 3, False), (33, 64, False), (70, 32, False), (4, 300, False), (33, 64, True)])
def test_orswot(rctx, M, A, wide_rows):
    pool, st, Dcap = orswot_case(M * 100 + A, M, A)
    assert (st["cnt"] == Dcap).any() and st["cnt"].any()
    fa, pa = R.insert_map(A, 3, seed=1)
    fm, pm = R.insert_map(M, 3, seed=2)
    exp, exp_status = R.orswot_reindex(st, fa, fm, M + 3, A + 3, Dcap + 3)
    assert not exp_status.any()
    side = E.orswot_side(st)
    if wide_rows:  # entry_mstride = 2 A on the input
        big = to_dev(np.full((N, M, 2 * A), np.uint64(2**64 - 1), np.uint64))
        big[:, :, :A] = side.entries
        side = side._replace(entries=big[:, :, :A])
    out, status = cg.orswot.reindex(side, dsrc(fa), dsrc(fm), Dcap=Dcap + 3, ctx=rctx)
    got = orswot_host(out)
    same(got, exp)
    assert not status_of(status).any()
    for s in list(range(len(pool))) + [N - 1]:
        want = map_orswot(pool[s % len(pool)], lambda a: int(pa[a]), lambda m: int(pm[m]))
        assert E.orswot_object(got, s) == want, s


# ---- MVReg -----------------------------------------------------------------------------------------
def mvreg_case(seed, A, V):
    st = E.mvreg_dense(E.mvreg_pool(seed, A, V), N, A, V)
    for i in range(0, N, 5):  # holes: the last value moves to the last slot
        used = np.flatnonzero(st["vclk"][i].any(axis=1))
        if len(used) and used[-1] != V - 1:
            s = int(used[-1])
            st["vclk"][i, V - 1], st["vval"][i, V - 1] = st["vclk"][i, s], st["vval"][i, s]
            st["vclk"][i, s], st["vval"][i, s] = 0, 0
    return st


@pytest.mark.parametrize("A,V,V_out", [(3, 1, 2), (32, 4, 5), (65, 16, 17), (300, 4, 5), (32, 20, 64)])
def test_mvreg(rctx, A, V, V_out):
    st = mvreg_case(A + V, A, V)
    fa, _ = R.insert_map(A, 3, seed=3)
    exp, exp_status = R.mvreg_reindex(st, fa, A + 3, V_out)
    assert not exp_status.any()
    (vc, vv), status = cg.mvreg.reindex(*E.mvreg_side(st), dsrc(fa), V=V_out, ctx=rctx)
    same(dict(vclk=to_host(vc), vval=to_host(vv)), exp)
    assert not status_of(status).any()
    assert E.undense(exp["vclk"][:16, :, R.inverse(fa, A)], exp["vval"][:16]) == E.undense(st["vclk"][:16], st["vval"][:16])


# ---- Map -------------------------------------------------------------------------------------------
def map_case(seed, K, V, A):
    pool = E.map_pool(seed, K, V, A)
    while not any(m.deferred for m in pool):  # a replay that left deferred removes
        seed += 1
        pool = E.map_pool(seed, K, V, A)
    Dcap = max(len(m.deferred) for m in pool)
    return pool, E.map_dense(pool, N, K, V, A, Dcap), Dcap


@pytest.mark.parametrize("K,V,A", [(5, 2, 3), (64, 4, 32), (70, 8, 24), (3, 20, 16), (2, 4, 300)])
def test_map(rctx, K, V, A):
    pool, st, Dcap = map_case(K * 10 + V, K, V, A)
    fa, pa = R.insert_map(A, 3, seed=4)
    fk, pk = R.insert_map(K, 3, seed=5)  # K = 64: one word of key bits becomes two
    exp, exp_status = R.map_reindex(st, fa, fk, K + 3, V + 1, A + 3, Dcap + 3)
    assert not exp_status.any()
    out, status = cg.map.reindex(E.map_side(st), dsrc(fa), dsrc(fk), V=V + 1, Dcap=Dcap + 3, ctx=rctx)
    got = map_host(out)
    same(got, exp)
    assert not status_of(status).any()
    back, status = R.map_reindex(got, R.inverse(fa, A), R.inverse(fk, K), K, V, A, Dcap)
    for s in range(len(pool)):  # read back through the inverse maps, the objects are the pool's
        assert E.map_object(back, s) == pool[s], s


# ---- pure growth -----------------------------------------------------------------------------------
def test_pure_growth_is_widen(gpu_ctx):
    _, st, Dcap = orswot_case(7, 60, 6)
    side = E.orswot_side(st)
    out, status = cg.orswot.reindex(side, Dcap=Dcap + 3, ctx=gpu_ctx)
    same(orswot_host(out), E.widen(st, ["dcl", "dset"], {"dcl": 1, "dset": 1}, 3))
    assert not status_of(status).any()
    out, status = cg.orswot.reindex(side, M=70, ctx=gpu_ctx)  # one word of member bits becomes two
    same(orswot_host(out), E.widen(E.widen(st, ["entries"], {"entries": 1}, 10), ["dset"], {"dset": 2}, 1))
    assert not status_of(status).any()
    _, mt, Dm = map_case(8, 60, 3, 6)
    mside = E.map_side(mt)
    out, status = cg.map.reindex(mside, V=5, ctx=gpu_ctx)
    same(map_host(out), E.widen(mt, ["vclk", "vval"], {"vclk": 2, "vval": 2}, 2))
    assert not status_of(status).any()
    out, status = cg.map.reindex(mside, K=70, Dcap=Dm + 2, ctx=gpu_ctx)
    w = E.widen(E.widen(mt, ["ec", "vclk", "vval"], {"ec": 1, "vclk": 1, "vval": 1}, 10), ["dset"], {"dset": 2}, 1)
    w = E.widen(w, ["dcl", "dset"], {"dcl": 1, "dset": 1}, 2)
    same(map_host(out), w)
    assert not status_of(status).any()
    rg = mvreg_case(9, 12, 4)
    (vc, vv), status = cg.mvreg.reindex(*E.mvreg_side(rg), V=9, ctx=gpu_ctx)
    same(dict(vclk=to_host(vc), vval=to_host(vv)), E.widen(rg, ["vclk", "vval"], {"vclk": 1, "vval": 1}, 5))
    assert not status_of(status).any()


# ---- loss and invalid input ------------------------------------------------------------------------
def states_of(k, n_classes):
    """Every n_classes-th state from k, and the last state of the batch."""
    return sorted(set(range(k, N, n_classes)) | {N - 1})


def test_orswot_loss_bits(rctx):
    M, A = 33, 8
    _, st, Dcap = orswot_case(11, M, A)
    Dcap += 1
    st = E.widen(st, ["dcl", "dset"], {"dcl": 1, "dset": 1}, 1)  # every state has a slot past its count
    st["clock"][:, -1] = 0
    st["entries"][:, :, -1] = 0
    st["entries"][:, -1, :] = 0
    st["dcl"][:, :, -1] = 0
    st["dset"][:, :, -1] &= ~(U1 << np.uint64((M - 1) % 64))
    fa, fm = np.arange(A - 1), np.arange(M - 1)  # the last actor and the last member are dropped
    side = E.orswot_side(st)
    out, status = cg.orswot.reindex(side, dsrc(fa), dsrc(fm), ctx=rctx)
    exp, exp_status = R.orswot_reindex(st, fa, fm, M - 1, A - 1, Dcap)
    assert not exp_status.any() and not status_of(status).any()  # the dropped ids are empty everywhere
    same(orswot_host(out), exp)
    hit = set()
    for s in states_of(0, 7):
        c = s % 6
        if c == 0:
            st["clock"][s, -1] = 5
        elif c == 1:
            st["entries"][s, 2, -1] = 7  # a dropped column of a kept row
        elif c == 2:
            st["entries"][s, -1, 0] = 3  # a dropped row
        elif c in (3, 4):
            if st["cnt"][s] == 0:
                st["cnt"][s] = 1
                st["dcl"][s, 0, 0] = 1 << 40
            if c == 3:
                st["dcl"][s, st["cnt"][s] - 1, -1] = 9
            else:
                st["dset"][s, st["cnt"][s] - 1, -1] |= U1 << np.uint64((M - 1) % 64)
        else:  # a slot past the count is not live: no loss
            st["dcl"][s, st["cnt"][s], -1] = 9
            st["dset"][s, st["cnt"][s], -1] |= U1 << np.uint64((M - 1) % 64)
            continue
        hit.add(s)
    exp, exp_status = R.orswot_reindex(st, fa, fm, M - 1, A - 1, Dcap)
    assert set(np.flatnonzero(exp_status)) == hit and (exp_status[sorted(hit)] == R.DROPPED).all()
    out, status = cg.orswot.reindex(E.orswot_side(st), dsrc(fa), dsrc(fm), ctx=rctx)
    assert np.array_equal(status_of(status), exp_status)
    same(orswot_host(out), exp)
    # the same through NULL maps with smaller sizes
    out, status = cg.orswot.reindex(E.orswot_side(st), M=M - 1, A=A - 1, ctx=rctx)
    assert np.array_equal(status_of(status), exp_status)
    same(orswot_host(out), exp)


def test_orswot_dcap_and_invalid(rctx):
    M, A = 20, 5
    _, st, Dcap = orswot_case(12, M, A)
    Dcap += 2
    st = E.widen(st, ["dcl", "dset"], {"dcl": 1, "dset": 1}, 2)
    for s in states_of(1, 9):  # full lists, the last state among them
        for d in range(int(st["cnt"][s]), Dcap):
            st["dcl"][s, d, d % A] = (1 << 41) + d
            st["dset"][s, d, 0] = U1 << np.uint64(d % M)
        st["cnt"][s] = Dcap
    bad = states_of(4, 9)[:-1]
    st["cnt"][bad] = Dcap + 1  # invalid
    st["cnt"][3] = 2**31 - 1
    fa, _ = R.insert_map(A, 1, seed=6)
    exp, exp_status = R.orswot_reindex(st, fa, None, M, A + 1, 1)
    assert exp_status[N - 1] == R.DCAP and (exp_status[bad] == R.INVALID).all() and exp_status[3] == R.INVALID
    assert (exp["cnt"][exp_status == R.DCAP] == 1).all() and not exp["clock"][bad].any()
    out, status = cg.orswot.reindex(E.orswot_side(st), dsrc(fa), Dcap=1, ctx=rctx)
    assert np.array_equal(status_of(status), exp_status)
    same(orswot_host(out), exp)
    exp, exp_status = R.orswot_reindex(st, fa, None, M, A + 1, Dcap + 4)  # growing keeps the invalid ones invalid
    out, status = cg.orswot.reindex(E.orswot_side(st), dsrc(fa), Dcap=Dcap + 4, ctx=rctx)
    assert np.array_equal(status_of(status), exp_status) and set(np.unique(exp_status)) == {0, R.INVALID}
    same(orswot_host(out), exp)
    # the last state of the batch invalid too: bit 2 alone and the empty output state, whatever the out Dcap
    st["cnt"][N - 1] = Dcap + 1
    for D2 in (1, Dcap, Dcap + 4):
        exp, exp_status = R.orswot_reindex(st, fa, None, M, A + 1, D2)
        assert exp_status[N - 1] == R.INVALID and exp["cnt"][N - 1] == 0
        assert not (exp["clock"][N - 1].any() or exp["entries"][N - 1].any() or exp["dcl"][N - 1].any()
                    or exp["dset"][N - 1].any())
        out, status = cg.orswot.reindex(E.orswot_side(st), dsrc(fa), Dcap=D2, ctx=rctx)
        assert np.array_equal(status_of(status), exp_status), D2
        same(orswot_host(out), exp)


def test_map_dcap_and_invalid(rctx):
    """Bits 0 and 2 on the Map: full lists cut to the out Dcap (the first slots kept, the count clamped), and a
    count above the in Dcap giving the empty state; the last state of the batch takes part in both."""
    K, V, A = 20, 3, 6
    _, st, Dcap = map_case(15, K, V, A)
    Dcap += 2
    st = E.widen(st, ["dcl", "dset"], {"dcl": 1, "dset": 1}, 2)
    for s in states_of(1, 9):  # full lists, the last state among them
        for d in range(int(st["cnt"][s]), Dcap):
            st["dcl"][s, d, d % A] = (1 << 41) + d
            st["dset"][s, d, 0] = U1 << np.uint64(d % K)
        st["cnt"][s] = Dcap
    bad = states_of(4, 9)[:-1]
    st["cnt"][bad] = Dcap + 1
    st["cnt"][3] = 2**31 - 1
    fa, _ = R.insert_map(A, 2, seed=7)
    fk, _ = R.insert_map(K, 3, seed=8)
    for last_invalid in (False, True):
        if last_invalid:
            st["cnt"][N - 1] = Dcap + 1
        for D2 in (1, Dcap + 4):
            exp, exp_status = R.map_reindex(st, fa, fk, K + 3, V, A + 2, D2)
            assert exp_status[N - 1] == (R.INVALID if last_invalid else (R.DCAP if D2 == 1 else 0))
            assert (exp_status[bad] == R.INVALID).all() and exp_status[3] == R.INVALID
            assert not (exp["clock"][bad].any() or exp["ec"][bad].any() or exp["vclk"][bad].any()
                        or exp["vval"][bad].any() or exp["cnt"][bad].any())
            assert (exp["cnt"][exp_status == R.DCAP] == D2).all() and (D2 != 1 or (exp_status == R.DCAP).any())
            out, status = cg.map.reindex(E.map_side(st), dsrc(fa), dsrc(fk), Dcap=D2, ctx=rctx)
            assert np.array_equal(status_of(status), exp_status), (last_invalid, D2)
            same(map_host(out), exp)


def test_even_actor_insertion(rctx):
    """A 32 -> 34: both sides even, so entry / value / deferred rows (many rows per state) take the column
    gather with 16-byte stores, staged or direct."""
    M, K, V, A = 33, 5, 2, 32
    fa, pa = R.insert_map(A, 2, seed=9)
    pool, st, Dcap = orswot_case(16, M, A)
    exp, exp_status = R.orswot_reindex(st, fa, None, M, A + 2, Dcap)
    out, status = cg.orswot.reindex(E.orswot_side(st), dsrc(fa), ctx=rctx)
    got = orswot_host(out)
    same(got, exp)
    assert not exp_status.any() and not status_of(status).any()
    for s in range(len(pool)):
        assert E.orswot_object(got, s) == map_orswot(pool[s], lambda a: int(pa[a]), lambda m: m), s
    _, mt, Dm = map_case(17, K, V, A)
    fk, _ = R.insert_map(K, 2, seed=10)
    exp, exp_status = R.map_reindex(mt, fa, fk, K + 2, V, A + 2, Dm)
    out, status = cg.map.reindex(E.map_side(mt), dsrc(fa), dsrc(fk), ctx=rctx)
    same(map_host(out), exp)
    assert not exp_status.any() and not status_of(status).any()
    rg = mvreg_case(18, A, 4)
    exp, exp_status = R.mvreg_reindex(rg, fa, A + 2, 4)
    (vc, vv), status = cg.mvreg.reindex(*E.mvreg_side(rg), dsrc(fa), ctx=rctx)
    same(dict(vclk=to_host(vc), vval=to_host(vv)), exp)
    assert not status_of(status).any()


def test_map_and_mvreg_loss_bits(rctx):
    K, V, A = 9, 4, 6
    _, st, Dcap = map_case(13, K, V, A)
    st["clock"][:, -1] = 0
    st["ec"][:, :, -1] = 0
    st["ec"][:, -1, :] = 0
    st["vclk"][:, :, :, -1] = 0
    st["vclk"][:, :, V - 1, :] = 0  # the last slot is empty ...
    st["vclk"][:, -1] = 0
    st["dcl"][:, :, -1] = 0
    st["dset"][:, :, -1] &= ~(U1 << np.uint64(K - 1))
    fa, fk = np.arange(A - 1), np.arange(K - 1)
    exp, exp_status = R.map_reindex(st, fa, fk, K - 1, V - 1, A - 1, Dcap)
    out, status = cg.map.reindex(E.map_side(st), dsrc(fa), dsrc(fk), V=V - 1, ctx=rctx)
    assert not exp_status.any() and not status_of(status).any()
    same(map_host(out), exp)
    want = {}
    for s in states_of(2, 5):
        c = (s // 5) % 5
        if c == 0:
            st["ec"][s, -1, 1] = 4  # a dropped key that is present
            want[s] = R.DROPPED
        elif c == 1:
            st["ec"][s, 0, 0] = max(int(st["ec"][s, 0, 0]), 1)
            st["vclk"][s, 0, V - 1, -1] = 6  # a filled slot at a position >= out V (of a kept key)
            want[s] = R.VALUES
        elif c == 2:
            st["vclk"][s, 1, 0, -1] = 8  # a dropped actor in a kept slot of a kept key
            want[s] = R.DROPPED
        elif c == 3:
            st["vclk"][s, 1, 0, -1] = 8
            st["vclk"][s, K - 2, V - 1, 0] = 2
            want[s] = R.DROPPED | R.VALUES
        else:
            st["vclk"][s, -1, V - 1, -1] = 3  # the value slots of a dropped key go with it: no bit
    exp, exp_status = R.map_reindex(st, fa, fk, K - 1, V - 1, A - 1, Dcap)
    assert {int(s): int(exp_status[s]) for s in np.flatnonzero(exp_status)} == want
    out, status = cg.map.reindex(E.map_side(st), dsrc(fa), dsrc(fk), V=V - 1, ctx=rctx)
    assert np.array_equal(status_of(status), exp_status)
    same(map_host(out), exp)
    # MVReg: the same two bits on the registers of key 1
    rg = dict(vclk=np.ascontiguousarray(st["vclk"][:, 1]), vval=np.ascontiguousarray(st["vval"][:, 1]))
    rg["vclk"][N - 1, V - 1, -1] = 1
    exp, exp_status = R.mvreg_reindex(rg, fa, A - 1, V - 1)
    assert exp_status[N - 1] == R.VALUES and (exp_status == R.DROPPED).any()
    (vc, vv), status = cg.mvreg.reindex(*E.mvreg_side(rg), dsrc(fa), V=V - 1, ctx=rctx)
    assert np.array_equal(status_of(status), exp_status)
    same(dict(vclk=to_host(vc), vval=to_host(vv)), exp)


# ---- edges -----------------------------------------------------------------------------------------
def test_edges(gpu_ctx):
    _, st, Dcap = orswot_case(14, 9, 4)
    side = E.orswot_side(st)
    empty = type(side)(*[t[:0] for t in side])
    out, status = cg.orswot.reindex(empty, A=6, ctx=gpu_ctx)
    assert tuple(out.entries.shape) == (0, 9, 6) and tuple(status.shape) == (0,)
    x = to_dev(np.ones((0, 5), np.uint64))
    out, status = cg.reindex.rows(x, None, 7, ctx=gpu_ctx)
    assert tuple(out.shape) == (0, 7)
    # equal base pointers
    a = cg.orswot._states_struct(gpu_ctx, side, "test")
    with pytest.raises(cg.CrdtGpuError) as ei:
        gpu_ctx.call("crdt_orswot_reindex", ctypes.byref(a), None, None, ctypes.byref(a), None)
    assert ei.value.code == cg._abi.CRDT_EINVAL
    with pytest.raises(cg.CrdtGpuError) as ei:
        cg.reindex.rows(side.clock, None, 4, out=side.clock, ctx=gpu_ctx)
    assert ei.value.code == cg._abi.CRDT_EINVAL
    assert np.array_equal(to_host(side.clock), st["clock"])
    with pytest.raises(ValueError):
        cg.orswot.reindex(side, dsrc(np.arange(3)), A=5, ctx=gpu_ctx)  # a size past the map's length
    hctx = cg.Context(0)  # a host-memory ctx: device pointers only, refused before anything is read
    hctx.call("crdt_ctx_set_mem_kind", cg._abi.CRDT_MEM_HOST)
    try:
        for call in (lambda: cg.orswot.reindex(side, ctx=hctx), lambda: cg.reindex.rows(side.clock, None, 5, ctx=hctx),
                     lambda: cg.reindex.index_map(dsrc(np.arange(3)), dsrc(np.arange(4)), ctx=hctx)):
            with pytest.raises(cg.CrdtGpuError) as ei:
                call()
            assert ei.value.code == cg._abi.CRDT_EUNSUPPORTED
    finally:
        hctx.close()
    assert (cg.REINDEX_DCAP, cg.REINDEX_DROPPED, cg.REINDEX_INVALID, cg.REINDEX_VALUES) == (1, 2, 4, 16)
