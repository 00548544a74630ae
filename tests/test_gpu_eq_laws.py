"""The reference's merge laws with the merge and the comparison both on the device: commutativity
(merge_batch(a, b) against merge_batch(b, a)) and idempotency (merge_batch(a, a)) judged by
crdt_*_eq_batch, 129 replay-built pairs per type at one narrow and one wide shape.  The expectation is
the oracle's `==` on the read-back results, pair by pair, not an assumed all-zero."""
import numpy as np
import pytest
import torch

import eq_util as E
from gpu_util import to_host
from eq_util import map_side, mvreg_side, orswot_side

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N = 129


def pairs(pool):
    return [pool[i % len(pool)] for i in range(N)], [pool[(7 * i + 3) % len(pool)] for i in range(N)]


def back(side, fields=None):
    """The dense arrays of a device side, as eq_util's expected_* read them."""
    if fields is None:
        return dict(vclk=to_host(side[0]), vval=to_host(side[1]))
    out = {k: to_host(getattr(side, f)) for k, f in fields.items()}
    out["cnt"] = side.def_count.cpu().numpy()
    return out


ORSWOT_F = dict(clock="clock", entries="entries", dcl="def_clock", dset="def_members")
MAP_F = dict(clock="clock", ec="ec", vclk="vclk", vval="vval", dcl="def_clock", dset="def_keys")


def clone(side):
    ts = [t.clone() for t in side]
    return type(side)(*ts) if hasattr(side, "_fields") else tuple(ts)


@pytest.mark.parametrize("A", [6, 300])
def test_mvreg_merge_laws(gpu_ctx, A):
    V = 8
    a, b = pairs(E.mvreg_pool(40 + A, A, 3, P=48))
    da, db = mvreg_side(E.mvreg_dense(a, N, A, V)), mvreg_side(E.mvreg_dense(b, N, A, V))
    ab, ba = clone(da), clone(db)
    assert not cg.mvreg.merge_batch(*ab, *db, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.mvreg.merge_batch(*ba, *da, ctx=gpu_ctx).cpu().numpy().any()
    got = cg.mvreg.eq_batch(*ab, *ba, ctx=gpu_ctx).cpu().numpy()
    exp = E.expected_mvreg(back(ab), back(ba))
    assert np.array_equal(got, exp) and not exp.any()  # mvreg.rs: merge commutes
    same = (ab[0] == ba[0]).flatten(1).all(1) & (ab[1] == ba[1]).flatten(1).all(1)
    assert not bool(same.all()), "no pair differs bytewise: the test would not exercise order-freedom"
    aa = clone(da)
    assert not cg.mvreg.merge_batch(*aa, *clone(da), ctx=gpu_ctx).cpu().numpy().any()
    got = cg.mvreg.eq_batch(*aa, *da, ctx=gpu_ctx).cpu().numpy()
    assert np.array_equal(got, E.expected_mvreg(back(aa), back(da))) and not got.any()


@pytest.mark.parametrize("M,A", [(12, 4), (70, 300)])
def test_orswot_merge_laws(gpu_ctx, M, A):
    a, b = pairs(E.orswot_pool(50 + M, M, A, P=48))
    Dcap = 2 * max(len(o.deferred) for o in a + b) + 1
    da, db = orswot_side(E.orswot_dense(a, N, M, A, Dcap)), orswot_side(E.orswot_dense(b, N, M, A, Dcap + 2))
    ab, ba = clone(da), clone(db)
    assert not cg.orswot.merge_batch(ab, db, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.orswot.merge_batch(ba, da, ctx=gpu_ctx).cpu().numpy().any()
    got = cg.orswot.eq_batch(ab, ba, ctx=gpu_ctx).cpu().numpy()
    exp = E.expected_orswot(back(ab, ORSWOT_F), back(ba, ORSWOT_F))
    assert np.array_equal(got, exp) and not exp.any()
    aa = clone(da)
    assert not cg.orswot.merge_batch(aa, clone(da), ctx=gpu_ctx).cpu().numpy().any()
    got = cg.orswot.eq_batch(aa, da, ctx=gpu_ctx).cpu().numpy()
    assert np.array_equal(got, E.expected_orswot(back(aa, ORSWOT_F), back(da, ORSWOT_F))) and not got.any()


@pytest.mark.parametrize("K,A", [(10, 3), (70, 300)])
def test_map_merge_laws(gpu_ctx, K, A):
    V = 3
    a, b = pairs(E.map_pool(60 + K, K, V, A, P=48, lawful=True))
    Dcap = 2 * max(len(m.deferred) for m in a + b) + 1
    da = map_side(E.map_dense(a, N, K, 2 * V, A, Dcap))
    db = map_side(E.map_dense(b, N, K, 2 * V + 1, A, Dcap + 2))
    ab, ba = clone(da), clone(db)
    assert not cg.map.merge_batch(ab, db, ctx=gpu_ctx).cpu().numpy().any()
    assert not cg.map.merge_batch(ba, da, ctx=gpu_ctx).cpu().numpy().any()
    got = cg.map.eq_batch(ab, ba, ctx=gpu_ctx).cpu().numpy()
    exp = E.expected_map(back(ab, MAP_F), back(ba, MAP_F))
    assert np.array_equal(got, exp) and not exp.any()
    same = (ab.vval == ba.vval[:, :, :2 * V]).flatten(1).all(1)
    assert not bool(same.all()), "no pair differs bytewise: the test would not exercise order-freedom"
    aa = clone(da)
    assert not cg.map.merge_batch(aa, clone(da), ctx=gpu_ctx).cpu().numpy().any()
    got = cg.map.eq_batch(aa, da, ctx=gpu_ctx).cpu().numpy()
    assert np.array_equal(got, E.expected_map(back(aa, MAP_F), back(da, MAP_F))) and not got.any()
