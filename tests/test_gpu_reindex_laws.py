"""Laws of the reindex calls, checked through kernels that exist independently of them: the round trip
through the union dictionary and back is bit-identical; egress of the re-indexed states with the new
dictionaries is byte for byte the egress of the input with the old ones; reindex commutes with
merge_batch (by eq_batch, and against the oracle's merge of the re-labelled objects)."""
import numpy as np
import pytest
import torch

import eq_util as E
import oracle as O
import reindex_util as R
from gpu_util import to_dev, to_host
from orswot_apply_util import map_orswot

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import wire  # noqa: E402

N = 257


def dsrc(src):
    return torch.from_numpy(np.asarray(src).astype(np.int32)).cuda()


def dicts(seed, n, extra, wide=False):
    """(old ids, new ids = old with `extra` new ones at the front, inside and at the end, src) on the device."""
    rng = np.random.default_rng(seed)
    src, _ = R.insert_map(n, extra, seed=seed)
    if wide:
        new = np.sort(rng.choice(2**62, size=n + extra, replace=False)).astype(np.uint64)
        dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()  # noqa: E731
    else:
        new = np.sort(rng.choice(2**32 - 1, size=n + extra, replace=False)).astype(np.uint32)
        dev = lambda a: torch.from_numpy(a.view(np.int32).copy()).cuda()  # noqa: E731
    return dev(new[src >= 0]), dev(new), src


def built_map(old, new, src, ctx):
    got, n_lost = cg.reindex.index_map(old, new, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), src) and int(n_lost.cpu()[0]) == 0
    return got


def same_bytes(a, b):
    (off_a, data_a), (off_b, data_b) = a, b
    torch.cuda.synchronize()
    assert off_a.cpu().tolist() == off_b.cpu().tolist()
    assert bytes(data_a.cpu().numpy().tobytes()) == bytes(data_b.cpu().numpy().tobytes())
    assert data_a.numel() > 0


def pooled(st):
    """Per-state deferred slots -> the pool in state order that orswot_egress takes."""
    cnt = st.def_count.to(torch.int64)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cnt.device), torch.cumsum(cnt, 0)])
    live = torch.arange(st.def_clock.shape[1], device=cnt.device)[None, :] < cnt[:, None]
    return off, st.def_clock[live].contiguous(), st.def_members[live].contiguous()


def orswot_states(seed, M, A, extra_d=0, shift=0):
    pool = E.orswot_pool(seed, M, A)
    pool = pool[shift:] + pool[:shift]
    Dcap = max(1, max(len(o.deferred) for o in pool)) + extra_d
    return pool, E.orswot_dense(pool, N, M, A, Dcap)


def map_states(seed, K, V, A, extra_d=0, shift=0, Vd=None):
    pool = E.map_pool(seed, K, V, A, lawful=True)
    pool = pool[shift:] + pool[:shift]
    Dcap = max(1, max(len(m.deferred) for m in pool)) + extra_d
    return pool, E.map_dense(pool, N, K, Vd or V, A, Dcap)


def bit_same(a, b):
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)


# ---- round trip ------------------------------------------------------------------------------------
def test_round_trip_is_bit_identical(gpu_ctx):
    M, A, K, V = 40, 9, 12, 3
    fa, fm, fk = R.insert_map(A, 3, 1)[0], R.insert_map(M, 30, 2)[0], R.insert_map(K, 60, 3)[0]
    ia, im, ik = dsrc(R.inverse(fa, A)), dsrc(R.inverse(fm, M)), dsrc(R.inverse(fk, K))
    _, st = orswot_states(21, M, A)
    x = E.orswot_side(st)
    y, s1 = cg.orswot.reindex(x, dsrc(fa), dsrc(fm), Dcap=x.def_clock.shape[1] + 2, ctx=gpu_ctx)
    z, s2 = cg.orswot.reindex(y, ia, im, Dcap=x.def_clock.shape[1], ctx=gpu_ctx)
    bit_same(z, x)
    assert not s1.cpu().numpy().any() and not s2.cpu().numpy().any()
    _, mt = map_states(22, K, V, A)
    x = E.map_side(mt)
    y, s1 = cg.map.reindex(x, dsrc(fa), dsrc(fk), V=V + 2, Dcap=x.def_clock.shape[1] + 2, ctx=gpu_ctx)
    z, s2 = cg.map.reindex(y, ia, ik, V=V, Dcap=x.def_clock.shape[1], ctx=gpu_ctx)
    bit_same(z, x)
    assert not s1.cpu().numpy().any() and not s2.cpu().numpy().any()
    rg = E.mvreg_dense(E.mvreg_pool(23, A, 4), N, A, 4)
    x = E.mvreg_side(rg)
    y, s1 = cg.mvreg.reindex(*x, dsrc(fa), V=7, ctx=gpu_ctx)
    z, s2 = cg.mvreg.reindex(*y, ia, V=4, ctx=gpu_ctx)
    bit_same(z, x)
    assert not s1.cpu().numpy().any() and not s2.cpu().numpy().any()


# ---- egress ----------------------------------------------------------------------------------------
def test_egress_bytes_do_not_change_lattice(gpu_ctx):
    rng = np.random.default_rng(31)
    A, U = 37, 90
    a0, a1, fa = dicts(32, A, 4)
    src = built_map(a0, a1, fa, gpu_ctx)
    rows = rng.integers(1, 2**63, size=(N, 2 * A), dtype=np.int64).astype(np.uint64)
    rows[rng.random((N, 2 * A)) > 0.6] = 0
    vc = to_dev(rows[:, :A])
    same_bytes(wire.vclock_egress(cg.vclock.reindex(vc, src, ctx=gpu_ctx)[0], a1, ctx=gpu_ctx),
               wire.vclock_egress(vc, a0, ctx=gpu_ctx))
    pn = to_dev(rows)
    same_bytes(wire.pncounter_egress(cg.pncounter.reindex(pn, src, ctx=gpu_ctx)[0], a1, ctx=gpu_ctx),
               wire.pncounter_egress(pn, a0, ctx=gpu_ctx))
    e0, e1, fe = dicts(33, U, 70, wide=True)
    esrc = built_map(e0, e1, fe, gpu_ctx)
    gs = to_dev(R.pack((rng.random((N, U)) < 0.3).astype(np.uint8)))
    out, status = cg.gset.reindex(gs, esrc, U_in=U, ctx=gpu_ctx)
    same_bytes(wire.gset_egress(out, e1, ctx=gpu_ctx), wire.gset_egress(gs, e0, ctx=gpu_ctx))
    assert not status.cpu().numpy().any()


def test_egress_bytes_do_not_change_causal(gpu_ctx):
    M, A, K, V = 40, 9, 12, 3
    a0, a1, fa = dicts(34, A, 3)
    m0, m1, fm = dicts(35, M, 30, wide=True)
    k0, k1, fk = dicts(36, K, 60)
    sa, sm, sk = built_map(a0, a1, fa, gpu_ctx), built_map(m0, m1, fm, gpu_ctx), built_map(k0, k1, fk, gpu_ctx)
    _, st = orswot_states(24, M, A)
    x = E.orswot_side(st)
    y, _ = cg.orswot.reindex(x, sa, sm, Dcap=x.def_clock.shape[1] + 3, ctx=gpu_ctx)
    same_bytes(wire.orswot_egress(y.clock, y.entries, a1, m1, *pooled(y), ctx=gpu_ctx),
               wire.orswot_egress(x.clock, x.entries, a0, m0, *pooled(x), ctx=gpu_ctx))
    assert int(x.def_count.sum()) > 0
    rg = E.mvreg_dense(E.mvreg_pool(25, A, 4), N, A, 4)
    x = E.mvreg_side(rg)
    y, _ = cg.mvreg.reindex(*x, sa, V=6, ctx=gpu_ctx)
    same_bytes(wire.mvreg_egress(*y, a1, ctx=gpu_ctx), wire.mvreg_egress(*x, a0, ctx=gpu_ctx))
    _, mt = map_states(29, K, V, A)
    x = E.map_side(mt)
    y, _ = cg.map.reindex(x, sa, sk, V=V + 1, Dcap=x.def_clock.shape[1] + 3, ctx=gpu_ctx)
    same_bytes(wire.map_egress(y, a1, k1, ctx=gpu_ctx), wire.map_egress(x, a0, k0, ctx=gpu_ctx))
    assert int(x.def_count.sum()) > 0


# ---- merge -----------------------------------------------------------------------------------------
def clone(st):
    return type(st)(*[t.clone() for t in st])


def relabel_map(m, pa, pk):
    fa = lambda c: O.VClock({int(pa[a]): n for a, n in c.dots.items()})  # noqa: E731
    r = O.Map(O.MVReg)
    r.clock = fa(m.clock)
    r.entries = {int(pk[k]): O.MapEntry(fa(e.clock), O.MVReg([(fa(c), v) for c, v in e.val.vals])) for k, e in m.entries.items()}
    r.deferred = {fa(c): {int(pk[k]) for k in ks} for c, ks in m.deferred.items()}
    return r


def merged(a, b):
    x = a.copy()
    x.merge(b.copy())
    return x


def test_reindex_commutes_with_merge_orswot(gpu_ctx):
    M, A = 40, 9
    (fa, pa), (fm, pm) = R.insert_map(A, 3, 1), R.insert_map(M, 30, 2)
    px, sx = orswot_states(27, M, A, extra_d=0)
    py, sy = orswot_states(27, M, A, shift=3)
    D = 2 * sx["dcl"].shape[1] + 2
    x, y = E.orswot_side(E.widen(sx, ["dcl", "dset"], {"dcl": 1, "dset": 1}, D - sx["dcl"].shape[1])), E.orswot_side(sy)
    m = clone(x)
    assert not cg.orswot.merge_batch(m, y, ctx=gpu_ctx).cpu().numpy().any()
    lhs, s0 = cg.orswot.reindex(m, dsrc(fa), dsrc(fm), ctx=gpu_ctx)
    rhs, s1 = cg.orswot.reindex(x, dsrc(fa), dsrc(fm), ctx=gpu_ctx)
    ry, s2 = cg.orswot.reindex(y, dsrc(fa), dsrc(fm), ctx=gpu_ctx)
    assert not cg.orswot.merge_batch(rhs, ry, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.orswot.eq_batch(lhs, rhs, ctx=gpu_ctx).cpu().numpy().any()
    assert not (s0.cpu().numpy().any() or s1.cpu().numpy().any() or s2.cpu().numpy().any())
    for side in (lhs, rhs):
        got = dict(clock=to_host(side.clock), entries=to_host(side.entries), dcl=to_host(side.def_clock),
                   dset=to_host(side.def_members), cnt=side.def_count.cpu().numpy())
        for s in range(len(px)):
            want = map_orswot(merged(px[s], py[s]), lambda a: int(pa[a]), lambda i: int(pm[i]))
            assert E.orswot_object(got, s) == want, s


def test_reindex_commutes_with_merge_map_and_mvreg(gpu_ctx):
    K, V, A = 12, 3, 9
    (fa, pa), (fk, pk) = R.insert_map(A, 3, 1), R.insert_map(K, 60, 3)
    px, sx = map_states(33, K, V, A, Vd=2 * V)
    py, sy = map_states(33, K, V, A, shift=5)
    D = 2 * sx["dcl"].shape[1] + 2
    x, y = E.map_side(E.widen(sx, ["dcl", "dset"], {"dcl": 1, "dset": 1}, D - sx["dcl"].shape[1])), E.map_side(sy)
    m = clone(x)
    assert not cg.map.merge_batch(m, y, ctx=gpu_ctx).cpu().numpy().any()
    lhs, s0 = cg.map.reindex(m, dsrc(fa), dsrc(fk), ctx=gpu_ctx)
    rhs, s1 = cg.map.reindex(x, dsrc(fa), dsrc(fk), ctx=gpu_ctx)
    ry, s2 = cg.map.reindex(y, dsrc(fa), dsrc(fk), ctx=gpu_ctx)
    assert not cg.map.merge_batch(rhs, ry, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.map.eq_batch(lhs, rhs, ctx=gpu_ctx).cpu().numpy().any()
    assert not (s0.cpu().numpy().any() or s1.cpu().numpy().any() or s2.cpu().numpy().any())
    for side in (lhs, rhs):
        got = dict(clock=to_host(side.clock), ec=to_host(side.ec), vclk=to_host(side.vclk), vval=to_host(side.vval),
                   dcl=to_host(side.def_clock), dset=to_host(side.def_keys), cnt=side.def_count.cpu().numpy())
        for s in range(len(px)):
            assert E.map_object(got, s) == relabel_map(merged(px[s], py[s]), pa, pk), s
    # MVReg on its own
    regs = E.mvreg_pool(29, A, 4)
    rx, ry_ = E.mvreg_dense(regs, N, A, 8), E.mvreg_dense(regs[3:] + regs[:3], N, A, 4)
    x, y = E.mvreg_side(rx), E.mvreg_side(ry_)
    m = tuple(t.clone() for t in x)
    assert not cg.mvreg.merge_batch(*m, *y, ctx=gpu_ctx).cpu().numpy().any()
    lhs, _ = cg.mvreg.reindex(*m, dsrc(fa), ctx=gpu_ctx)
    rhs, _ = cg.mvreg.reindex(*x, dsrc(fa), ctx=gpu_ctx)
    ry2, _ = cg.mvreg.reindex(*y, dsrc(fa), ctx=gpu_ctx)
    assert not cg.mvreg.merge_batch(*rhs, *ry2, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.mvreg.eq_batch(*lhs, *rhs, ctx=gpu_ctx).cpu().numpy().any()
    want = []
    for s in range(len(regs)):
        r = merged(regs[s], regs[(s + 3) % len(regs)])
        want.append(O.MVReg([(O.VClock({int(pa[a]): n for a, n in c.dots.items()}), v) for c, v in r.vals]))
    assert E.undense(to_host(lhs[0])[:len(regs)], to_host(lhs[1])[:len(regs)]) == want
