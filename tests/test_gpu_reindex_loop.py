"""The scenario the reindex calls exist for.  States are resident under dictionaries D0; a second batch
of frames names a new actor (ids below, inside and above D0's range) and new members / keys, so its
ingest with D0 reports status bit 1; the caller builds D1 = D0 u new ids, re-indexes the resident
states on the device, ingests the batch with D1, merges, and egresses with D1.  The decoded frames are
the oracle's a.merge(b).  And the capacity case: an apply_batch that runs out of deferred slots
succeeds after reindex to a larger Dcap."""
import numpy as np
import pytest
import torch

import eq_util as E
import oracle as O
import reindex_util as R
import test_gpu_wire as TW
from gpu_util import to_host
from orswot_apply_util import map_orswot, op_tuple
from test_gpu_reindex_laws import merged, relabel_map

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import wire  # noqa: E402

N = 257


def union_dicts(seed, n0, extra, wide):
    """ids1 (n0 + extra ascending ids), the device dictionaries D0 / D1, src (D1 position -> D0 position or
    -1), pos (D0 position -> D1 position) and the D1 positions of the new ids (front, middle, end)."""
    rng = np.random.default_rng(seed)
    src, pos = R.insert_map(n0, extra, seed=seed)
    if wide:
        ids1 = np.sort(rng.choice(2**62, size=n0 + extra, replace=False)).astype(np.uint64)
        dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()  # noqa: E731
    else:
        ids1 = np.sort(rng.choice(2**32 - 1, size=n0 + extra, replace=False)).astype(np.uint32)
        dev = lambda a: torch.from_numpy(a.view(np.int32).copy()).cuda()  # noqa: E731
    return ids1, dev(ids1[src >= 0]), dev(ids1), src, pos, np.flatnonzero(src < 0)


def slots(fr, Dcap):
    """wire.OrswotFrames (removes pooled in state order) -> OrswotStates with Dcap slots per state."""
    n, dev = fr.clock.shape[0], fr.clock.device
    cnt = fr.def_off[1:] - fr.def_off[:-1]
    state = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
    d = torch.arange(state.shape[0], device=dev) - fr.def_off[:-1][state]
    dcl = torch.zeros((n, Dcap, fr.clock.shape[1]), dtype=torch.int64, device=dev)
    dmb = torch.zeros((n, Dcap, fr.def_members.shape[1]), dtype=torch.int64, device=dev)
    dcl[state, d] = fr.def_clock
    dmb[state, d] = fr.def_members
    return cg.orswot.OrswotStates(fr.clock, fr.entries, dcl, dmb, cnt.to(torch.int32))


def pooled(st):
    cnt = st.def_count.to(torch.int64)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cnt.device), torch.cumsum(cnt, 0)])
    live = torch.arange(st.def_clock.shape[1], device=cnt.device)[None, :] < cnt[:, None]
    return off, st.def_clock[live].contiguous(), st.def_members[live].contiguous()


def orswot_wire(o):
    return (dict(o.clock.dots), {m: dict(e.dots) for m, e in o.entries.items()},
            {tuple(sorted(k.dots.items())): set(ms) for k, ms in o.deferred.items()})


def orswot_names(o, new_a, new_m):
    acts = set(o.clock.dots) | {a for e in o.entries.values() for a in e.dots} | {a for k in o.deferred for a in k.dots}
    mems = set(o.entries) | {m for ms in o.deferred.values() for m in ms}
    return bool(acts & set(new_a.tolist()) or mems & set(new_m.tolist()))


def test_orswot_new_ids_then_merge(gpu_ctx):
    rng = np.random.default_rng(51)
    A0, M0 = 6, 20
    aids, ad0, ad1, fa, pa, new_a = union_dicts(52, A0, 3, wide=False)
    mids, md0, md1, fm, pm, new_m = union_dicts(53, M0, 3, wide=True)
    base_a, base_b = E.orswot_pool(54, 12, 4), E.orswot_pool(55, 12, 4)
    old_act, old_mem = pa[[0, 2, 3, 5]], pm[np.arange(12) + 4]
    b_act = np.array([new_a[0], new_a[1], new_a[2], pa[1]])
    b_mem = np.concatenate([new_m, pm[:9]])
    a = [map_orswot(base_a[s % 16], lambda i: int(old_act[i]), lambda m: int(old_mem[m])) for s in range(N)]
    b = [map_orswot(base_b[s % 16], lambda i: int(b_act[i]), lambda m: int(b_mem[m])) if s % 2 == 0 or s == N - 1 else
         map_orswot(base_b[s % 16], lambda i: int(old_act[i]), lambda m: int(old_mem[m])) for s in range(N)]
    blob_a, off_a = TW.orswot_blob([orswot_wire(o) for o in a], aids, mids, rng)
    blob_b, off_b = TW.orswot_blob([orswot_wire(o) for o in b], aids, mids, rng)
    exp = [merged(x, y) for x, y in zip(a, b)]
    Dcap = max(1, max(len(o.deferred) for o in a + b + exp))
    # 1. the resident states under D0
    fr = wire.orswot_ingest(TW.dev_bytes(blob_a), TW.dev_off(off_a), ad0, md0, ctx=gpu_ctx)
    assert not fr.status.cpu().numpy().any()
    res = slots(fr, Dcap)
    # 2-3. the second batch under D0: bit 1 on exactly the frames that name a new id
    fb = wire.orswot_ingest(TW.dev_bytes(blob_b), TW.dev_off(off_b), ad0, md0, ctx=gpu_ctx)
    names = np.array([orswot_names(o, new_a, new_m) for o in b])
    assert np.array_equal((fb.status.cpu().numpy() & 2) != 0, names) and names.any() and not names.all()
    # 4. D1 and the maps, on the device
    sa, lost_a = cg.reindex.index_map(ad0, ad1, ctx=gpu_ctx)
    sm, lost_m = cg.reindex.index_map(md0, md1, ctx=gpu_ctx)
    res1, status = cg.orswot.reindex(res, sa, sm, ctx=gpu_ctx)
    assert not status.cpu().numpy().any() and int(lost_a.cpu()[0]) == 0 and int(lost_m.cpu()[0]) == 0
    assert np.array_equal(sa.cpu().numpy(), fa) and np.array_equal(sm.cpu().numpy(), fm)
    # 5. the second batch under D1
    fb1 = wire.orswot_ingest(TW.dev_bytes(blob_b), TW.dev_off(off_b), ad1, md1, ctx=gpu_ctx)
    assert not fb1.status.cpu().numpy().any()
    # 6. merge and egress under D1
    assert not cg.orswot.merge_batch(res1, slots(fb1, Dcap), ctx=gpu_ctx).cpu().numpy().any()
    eoff, edata = wire.orswot_egress(res1.clock, res1.entries, ad1, md1, *pooled(res1), ctx=gpu_ctx)
    # 7. the oracle's a.merge(b)
    for s, frame in enumerate(TW.host_frames(edata, eoff)):
        c, e, d, pos = O.unbc_orswot(frame)
        assert pos == len(frame)
        wc, we, wd = orswot_wire(exp[s])
        assert c == {int(aids[i]): v for i, v in wc.items()}, s
        assert e == {int(mids[m]): {int(aids[i]): v for i, v in x.items()} for m, x in we.items()}, s
        assert d == {tuple(sorted((int(aids[i]), v) for i, v in k)): {int(mids[m]) for m in ms} for k, ms in wd.items()}, s
    assert any(o.deferred for o in exp) and any(set(o.entries) & set(new_m.tolist()) for o in exp)


def map_names(m, new_a, new_k):
    clocks = [m.clock] + [e.clock for e in m.entries.values()] + [c for e in m.entries.values() for c, _ in e.val.vals] \
        + list(m.deferred)
    acts = {a for c in clocks for a in c.dots}
    keys = set(m.entries) | {k for ks in m.deferred.values() for k in ks}
    return bool(acts & set(new_a.tolist()) or keys & set(new_k.tolist()))


def test_map_new_ids_then_merge(gpu_ctx):
    A0, K0 = 5, 14
    aids, ad0, ad1, fa, pa, new_a = union_dicts(56, A0, 3, wide=False)
    kids, kd0, kd1, fk, pk, new_k = union_dicts(57, K0, 3, wide=False)
    base_a, base_b = E.map_pool(32, 10, 3, 3, lawful=True), E.map_pool(33, 10, 3, 3, lawful=True)
    old_act, old_key = pa[[0, 2, 4]], pk[np.arange(10) + 3]
    b_key = np.concatenate([new_k, pk[:7]])
    a = [relabel_map(base_a[s % 16], old_act, old_key) for s in range(N)]
    b = [relabel_map(base_b[s % 16], new_a, b_key) if s % 2 == 0 or s == N - 1 else
         relabel_map(base_b[s % 16], old_act, old_key) for s in range(N)]
    exp = [merged(x, y) for x, y in zip(a, b)]
    V = max(1, O.max_vals(exp), O.max_vals(a), O.max_vals(b))
    Dcap = max(1, max(len(m.deferred) for m in a + b + exp))
    blob_a, off_a = TW.map_blob(a, aids, kids)
    blob_b, off_b = TW.map_blob(b, aids, kids)
    res, st = wire.map_ingest(TW.dev_bytes(blob_a), TW.dev_off(off_a), ad0, kd0, V, Dcap, ctx=gpu_ctx)
    assert not st.cpu().numpy().any()
    _, st = wire.map_ingest(TW.dev_bytes(blob_b), TW.dev_off(off_b), ad0, kd0, V, Dcap, ctx=gpu_ctx)
    names = np.array([map_names(m, new_a, new_k) for m in b])
    assert np.array_equal((st.cpu().numpy() & 2) != 0, names) and names.any() and not names.all()
    sa, lost_a = cg.reindex.index_map(ad0, ad1, ctx=gpu_ctx)
    sk, lost_k = cg.reindex.index_map(kd0, kd1, ctx=gpu_ctx)
    res1, status = cg.map.reindex(res, sa, sk, ctx=gpu_ctx)
    assert not status.cpu().numpy().any() and int(lost_a.cpu()[0]) == 0 and int(lost_k.cpu()[0]) == 0
    other, st = wire.map_ingest(TW.dev_bytes(blob_b), TW.dev_off(off_b), ad1, kd1, V, Dcap, ctx=gpu_ctx)
    assert not st.cpu().numpy().any()
    assert not cg.map.merge_batch(res1, other, ctx=gpu_ctx).cpu().numpy().any()
    eoff, edata = wire.map_egress(res1, ad1, kd1, ctx=gpu_ctx)
    for s, frame in enumerate(TW.host_frames(edata, eoff)):
        c, e, d, pos = O.unbc_map(frame)
        assert pos == len(frame)
        assert (c, e, d) == TW.map_decoded(exp[s], aids, kids), s
    assert any(m.deferred for m in exp) and any(set(m.entries) & set(new_k.tolist()) for m in exp)


def test_orswot_capacity_then_apply(gpu_ctx):
    """apply_batch reports bit 0 at Dcap = 2; the same ops succeed after reindex(..., Dcap=8)."""
    M, A, P = 12, 4, 16
    pool = [o for o in E.orswot_pool(60, M, A) if len(o.deferred) <= 2]
    objs = [pool[s % len(pool)] for s in range(N)]
    st = E.orswot_dense(objs, N, M, A, 2)
    big = 1 << 40
    ops = [[O.OrswotRm(O.VClock({s % A: big + i}), [(s + i) % M]) for i in range(1 + s % 5)] for s in range(N)]
    ops[N - 1] = [O.OrswotRm(O.VClock({A - 1: big + i}), [M - 1]) for i in range(5)]
    want = []
    for o, stream in zip(objs, ops):
        o = o.copy()
        for op in stream:
            o.apply(op)
        want.append(o)
    over = np.array([len(o.deferred) > 2 for o in want])
    assert over.any() and not over.all() and max(len(o.deferred) for o in want) <= 8
    batch = cg.orswot.encode_ops([[op_tuple(op) for op in stream] for stream in ops], A, "cuda:0")
    keep = E.orswot_side(st)
    work = type(keep)(*[t.clone() for t in keep])
    status = cg.orswot.apply_batch(*work, batch, ctx=gpu_ctx).cpu().numpy()
    assert np.array_equal((status & 1) != 0, over)  # the precondition: retry with a larger Dcap
    wide, rs = cg.orswot.reindex(keep, Dcap=8, ctx=gpu_ctx)
    assert not rs.cpu().numpy().any()
    status = cg.orswot.apply_batch(*wide, batch, ctx=gpu_ctx).cpu().numpy()
    assert not status.any()
    got = dict(clock=to_host(wide.clock), entries=to_host(wide.entries), dcl=to_host(wide.def_clock),
               dset=to_host(wide.def_members), cnt=wide.def_count.cpu().numpy())
    for s in range(N):
        assert E.orswot_object(got, s) == want[s], s
