"""The reference's merge laws for the value-typed Maps with the merge and the comparison both on the
device: commutativity (merge_batch(a, b) against merge_batch(b, a)) and idempotency (merge_batch(a, a)
against a) judged by crdt_map_{counter,orswot,nested}_eq_batch, 65 replay-built pairs per type at one
narrow shape.  The expectation is the oracle's `==` on the read-back results, pair by pair, not an
assumed all-zero.  merge_batch leaves stale rows past the nested counts and its own slot order: the
commuted results differ bytewise, which is what the comparison must be immune to."""
import numpy as np
import pytest

import eq_vmap_util as V
import oracle as O
from gpu_util import to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N = 65
MERGE = {"counter": cg.map.counter_merge_batch, "orswot": cg.map.orswot_merge_batch, "nested": cg.map.nested_merge_batch}
EQ = {"counter": cg.map.counter_eq_batch, "orswot": cg.map.orswot_eq_batch, "nested": cg.map.nested_eq_batch}
FIELDS = {
    "counter": dict(clock="clock", ec="ec", val="val"),
    "orswot": dict(clock="clock", ec="ec", oc="oc", ent="ent", vcl="vd_clock", vset="vd_mem"),
    "nested": dict(clock="clock", ec="ec", ic="ic", iec="iec", ivc="ivc", ivv="ivv", vcl="id_clock", vset="id_keys"),
}
COUNTS = {"counter": {}, "orswot": dict(vn="vd_n"), "nested": dict(vn="id_n", nval="nval")}


def back(kind, side):
    """The dense arrays of a device side, as eq_vmap_util.expected reads them."""
    out = {k: to_host(getattr(side, f)) for k, f in FIELDS[kind].items()}
    out.update(dcl=to_host(side.def_clock), dset=to_host(side.def_keys), cnt=side.def_count.cpu().numpy())
    for k, f in COUNTS[kind].items():
        out[k] = getattr(side, f).cpu().numpy()
    if kind != "counter" and out["vset"].ndim == 3:
        out["vset"] = out["vset"][..., None]
    return out


def future_rm(m, actor, i, key):
    m = m.copy()
    m.apply(O.MapRm(O.VClock({actor: (1 << 30) + i}), {key}))
    return m


def clone(side):
    return type(side)(*[t.clone() for t in side])


@pytest.mark.parametrize("kind,K,A,T", [("counter", 6, 5, 2), ("orswot", 5, 5, 7), ("nested", 4, 5, 5)])
def test_value_map_merge_laws(gpu_ctx, kind, K, A, T):
    pool = V.pool(kind, 70 + K, 24, (K, A, T), lawful=True)
    a = [pool[i % len(pool)] for i in range(N)]
    b = [pool[(7 * i + 3) % len(pool)] for i in range(N)]
    for i in range(0, N, 4):  # a remove from the future on each side: both survive, in the merge's own slot order
        a[i], b[i] = future_rm(a[i], 0, i, 0), future_rm(b[i], 1, i, K - 1)
    Dcap = 2 * max(len(m.deferred) for m in a + b) + 1
    da = V.side(kind, V.densify(kind, a, N, K, A, T, Dcap, small=(K, A, T)))
    db = V.side(kind, V.densify(kind, b, N, K, A, T, Dcap, small=(K, A, T)))
    ab, ba = clone(da), clone(db)
    MERGE[kind](ab, db, ctx=gpu_ctx)
    MERGE[kind](ba, da, ctx=gpu_ctx)
    got = EQ[kind](ab, ba, ctx=gpu_ctx).cpu().numpy()
    exp = V.expected(kind, back(kind, ab), back(kind, ba))
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)
    assert np.array_equal(EQ[kind](ba, ab, ctx=gpu_ctx).cpu().numpy(), exp)
    same = np.ones(N, bool)
    for x, y in zip(ab, ba):
        same &= (x == y).reshape(N, -1).all(1).cpu().numpy()
    assert not same.all(), "no pair differs bytewise: the test would not exercise order-freedom"
    aa = clone(da)
    MERGE[kind](aa, clone(da), ctx=gpu_ctx)
    got = EQ[kind](aa, da, ctx=gpu_ctx).cpu().numpy()
    assert np.array_equal(got, V.expected(kind, back(kind, aa), back(kind, da)))
