"""get -> derive ctx -> op -> *_apply_batch on the value-typed Maps entirely on the device, against
the oracle doing the same through its API (Map::get / update / rm, PNCounter::inc / dec,
Orswot::add / rm / contains, the inner Map's get / update / rm, ReadCtx::derive_*).  After each step
the device states, decoded with the oracle's dense_to_*, equal the oracle objects."""
import numpy as np
import pytest
import torch

import oracle as O
import vmap_read_util as U
from gpu_util import to_host
from vmap_read_util import i32, i64

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N, DCAP = 4, 16


def u8(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.uint8), dtype=torch.uint8, device="cuda:0")


def _present_absent(objs, K):
    """One present and one absent key of every state, as query columns sorted by state."""
    qs, qk = [], []
    for s, m in enumerate(objs):
        present = sorted(m.entries)
        absent = [k for k in range(K) if k not in m.entries]
        assert present and absent, s
        for k in (present[0], absent[0]):
            qs.append(s), qk.append(k)
    return qs, qk


def _mixed_keys(objs, K):
    """One key per state: present in the even states, absent in the odd ones."""
    out = []
    for s, m in enumerate(objs):
        present = sorted(m.entries)
        absent = [k for k in range(K) if k not in m.entries]
        out.append(present[-1] if s % 2 == 0 else absent[-1])
    return out


def _mixed(present, Q):
    p = present.cpu().numpy()
    assert 0 < p.sum() < Q, "present neither all 0 nor all 1"
    return p


def _quiet(*statuses):
    for st in statuses:
        assert not st.cpu().numpy().any()


def _map_rm_fields(rc, qs, qk):
    """The fields shared by the three types' Map Rm batches: one Op::Rm per query, its clock the
    query's rm_clock row (derive_rm_ctx), its keyset the queried key."""
    Q = len(qs)
    rm = cg.derive_rm_ctx(rc)
    return dict(op_off=i64(np.searchsorted(qs, np.arange(N + 1))), kind=u8(np.ones(Q)), clk_row=i32(np.arange(Q)),
                clk_pool=rm.clock, key_off=i64(np.arange(Q + 1)), keys=i32(qk)), i32(np.zeros(Q)), i64(np.zeros(Q))


# ---- Map<K, PNCounter> -----------------------------------------------------------------------------
def test_counter_map_get_derive_apply_loop(gpu_ctx):
    K, A, W = 6, 4, 2
    objs = U.folded(O.map_counter_objects(N, K, A, W, seed=16, steps=120))
    assert any(m.deferred for m in objs), "a Map-level deferred remove pending"
    res, kw, off = U.counter_states(gpu_ctx, objs, K, A, W)
    slots = U.def_slots(res, kw, off, N, K, A, DCAP)

    def check(tag):
        c, e, v = to_host(res.clock), to_host(res.ec), to_host(res.val)
        for s in range(N):
            assert O.dense_to_map_counter(c[s], e[s], v[s], U.slot_deferred(slots, s)) == objs[s], (tag, s)

    check("ingest")

    # -- counter_get -> derive_rm_ctx -> Map Rm
    qs, qk = _present_absent(objs, K)
    Q = len(qs)
    rc, qst = cg.map.counter_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    f, z32, z64 = _map_rm_fields(rc, qs, qk)
    ops = cg.map.MapCounterOpBatch(f["op_off"], f["kind"], z32, z64, z32, z32, z64, u8(np.zeros(Q)), f["clk_row"],
                                   f["clk_pool"], f["key_off"], f["keys"])
    status = cg.map.counter_apply_batch(res.clock, res.ec, res.val, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, status)
    present = _mixed(rc.val.present, Q)
    for q in range(Q):
        m = objs[qs[q]]
        want = m.get(qk[q])
        assert bool(present[q]) == (want.val is not None)
        m.apply(m.rm(qk[q], want.derive_rm_ctx()))
    check("rm")

    # -- counter_get -> derive_add_ctx (the Map's dot) + derive_add_ctx over the gotten P / N row (the
    #    counter's dot) -> Up: inc in states 0 and 1, dec in states 2 and 3
    qk = _mixed_keys(objs, K)
    actors = [(s + 1) % A for s in range(N)]
    dirs = [0, 0, 1, 1]
    rc, qst = cg.map.counter_get(res, i32(np.arange(N)), i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    rows = rc.val.val[torch.arange(N, device="cuda:0"), i64(dirs)]  # (Q, A): the P or the N row
    vadd = cg.derive_add_ctx(cg.ReadCtx(rows, rows, None), i32(actors), ctx=gpu_ctx)
    ops = cg.map.MapCounterOpBatch(i64(np.arange(N + 1)), u8(np.zeros(N)), add.actor, add.counter, i32(qk), vadd.actor,
                                   vadd.counter, u8(dirs), i32(np.zeros(N)), i64(np.zeros((1, A))),
                                   i64(np.zeros(N + 1)), i32([0]))
    status = cg.map.counter_apply_batch(res.clock, res.ec, res.val, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, add.status, vadd.status, status)
    present = _mixed(rc.val.present, N)
    vcounter = to_host(vadd.counter)
    for s, m in enumerate(objs):
        got = m.get(qk[s])
        assert bool(present[s]) == (got.val is not None)
        a = actors[s]
        op = m.update(qk[s], got.derive_add_ctx(a), lambda v, c, a=a, d=dirs[s]: v.dec(a) if d else v.inc(a))
        assert int(vcounter[s]) == op.op[0].counter and (present[s] or vcounter[s] == 1)
        m.apply(op)
    check("up")


# ---- Map<K, Orswot<M>> -----------------------------------------------------------------------------
def test_orswot_map_get_derive_apply_loop(gpu_ctx):
    K, M, A = 6, 6, 4
    objs = U.folded(O.map_orswot_objects(N - 1, K, M, A, seed=21, steps=120))
    # state 3: state 0 with member m0 of key k0 added again by another actor, so a remove whose context
    # is read on state 3 names a dot state 0's set has not seen and defers there
    k0 = next(k for k, e in sorted(objs[0].entries.items()) if e.val.entries)
    m0 = sorted(objs[0].entries[k0].val.entries)[0]
    more = objs[0].copy()
    a0 = (max(objs[0].clock.dots, key=objs[0].clock.get) + 1) % A
    more.apply(more.update(k0, more.get(k0).derive_add_ctx(a0), lambda v, c: v.add(m0, c)))
    objs.append(more)
    assert not more.entries[k0].val.entries[m0] <= objs[0].entries[k0].val.clock
    res, kw, off = U.orswot_states(gpu_ctx, objs, K, M, A)
    slots = U.def_slots(res, kw, off, N, K, A, DCAP)

    def check(tag):
        c, e, o, m = to_host(res.clock), to_host(res.ec), to_host(res.oc), to_host(res.ent)
        vn, vc, vm = res.vd_n.cpu().numpy(), to_host(res.vd_clock), to_host(res.vd_mem)
        for s in range(N):
            vd = {k: [(vc[s, k, i], O.bitmap_members(vm[s, k, i:i + 1])) for i in range(int(vn[s, k]))]
                  for k in range(K)}
            got = O.dense_to_map_orswot(c[s], e[s], o[s], m[s], vd, U.slot_deferred(slots, s))
            assert got == objs[s], (tag, s)

    check("ingest")
    states = i32(np.arange(N))
    zero_pool, no_keys = i64(np.zeros((1, A))), (i64(np.zeros(N + 1)), i32([0]))

    # -- orswot_get -> derive_add_ctx -> Up with an Add: the one dot names the entry and the member
    qk = _mixed_keys(objs, K)
    actors = [(a0 + 1 + s) % A for s in range(N)]  # state 0's is not a0: its set must not see state 3's dot
    mems = [(2 * s + 1) % M for s in range(N)]
    rc, qst = cg.map.orswot_get(res, states, i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    ops = cg.map.MapOrswotOpBatch(i64(np.arange(N + 1)), u8(np.zeros(N)), add.actor, add.counter, i32(qk),
                                  u8(np.zeros(N)), add.actor, add.counter, i32(np.zeros(N)), zero_pool, *no_keys,
                                  i64(np.arange(N + 1)), i32(mems))
    status = cg.map.orswot_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, add.status, status)
    present, lens = _mixed(rc.val.present, N), rc.val.len.cpu().numpy()
    for s, m in enumerate(objs):
        got = m.get(qk[s])
        assert bool(present[s]) == (got.val is not None) and lens[s] == (len(got.val.read().val) if got.val else 0)
        m.apply(m.update(qk[s], got.derive_add_ctx(actors[s]), lambda v, c, x=mems[s]: v.add(x, c)))
    check("add")

    # -- orswot_contains -> derive_rm_ctx -> Up with the nested Rm; state 0's context is read on state 3
    src = [3, 1, 2, 3]
    qk, qm = [k0], [m0]
    for s in (1, 2, 3):
        k = next(k for k, e in sorted(objs[s].entries.items()) if e.val.entries)
        qk.append(k)
        # a present member, but an absent one in state 2
        qm.append(sorted(objs[s].entries[k].val.entries)[0] if s != 2 else
                  next(x for x in range(M) if x not in objs[s].entries[k].val.entries))
    actors = [(s + 3) % A for s in range(N)]
    rc, qst = cg.map.orswot_get(res, states, i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    crc, cst = cg.map.orswot_contains(res, i32(src), i32(qk), i32(qm), ctx=gpu_ctx)
    rm = cg.derive_rm_ctx(crc)
    ops = cg.map.MapOrswotOpBatch(i64(np.arange(N + 1)), u8(np.zeros(N)), add.actor, add.counter, i32(qk),
                                  u8(np.ones(N)), i32(np.zeros(N)), i64(np.zeros(N)), i32(np.arange(N)), rm.clock,
                                  *no_keys, i64(np.arange(N + 1)), i32(qm))
    status = cg.map.orswot_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, cst, add.status, status)
    vals = _mixed(crc.val, N)
    before = sum(len(e.val.deferred) for e in objs[0].entries.values())
    for s, m in enumerate(objs):
        held = objs[src[s]].get(qk[s]).val
        want = (held if held is not None else O.Orswot()).contains(qm[s])
        assert bool(vals[s]) == want.val
        m.apply(m.update(qk[s], m.get(qk[s]).derive_add_ctx(actors[s]),
                         lambda v, c, x=qm[s], w=want: v.rm(x, w.derive_rm_ctx())))
    assert sum(len(e.val.deferred) for e in objs[0].entries.values()) == before + 1, "the remove deferred"
    check("nested rm")

    # -- orswot_get -> derive_rm_ctx -> Map Rm
    qs, qk = _present_absent(objs, K)
    Q = len(qs)
    rc, qst = cg.map.orswot_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    f, z32, z64 = _map_rm_fields(rc, qs, qk)
    ops = cg.map.MapOrswotOpBatch(f["op_off"], f["kind"], z32, z64, z32, u8(np.zeros(Q)), z32, z64, f["clk_row"],
                                  f["clk_pool"], f["key_off"], f["keys"], i64(np.zeros(Q + 1)), i32([0]))
    status = cg.map.orswot_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, status)
    present = _mixed(rc.val.present, Q)
    for q in range(Q):
        m = objs[qs[q]]
        want = m.get(qk[q])
        assert bool(present[q]) == (want.val is not None)
        m.apply(m.rm(qk[q], want.derive_rm_ctx()))
    check("rm")


# ---- Map<K, Map<K2, MVReg>> ------------------------------------------------------------------------
def test_nested_map_get_derive_apply_loop(gpu_ctx):
    K, K2, A = 7, 3, 4
    objs = U.folded(O.nested_map_objects(N, K, K2, A, seed=40, steps=140))
    res, kw, off = U.nested_states(gpu_ctx, objs, K, K2, A)
    slots = U.def_slots(res, kw, off, N, K, A, DCAP)

    def canon(m):  # registers as sorted multisets (MVReg's own equality is order-free too)
        c = lambda vc: tuple(sorted(vc.dots.items()))  # noqa: E731
        inner = lambda n: (c(n.clock), tuple(sorted((j, c(e.clock), tuple(sorted((c(x), v) for x, v in e.val.vals)))  # noqa: E731
                                                    for j, e in n.entries.items())),
                           tuple(sorted((c(rm), tuple(sorted(ks))) for rm, ks in n.deferred.items())))
        return (c(m.clock), tuple(sorted((k, c(e.clock), inner(e.val)) for k, e in m.entries.items())),
                tuple(sorted((c(rm), tuple(sorted(ks))) for rm, ks in m.deferred.items())))

    def check(tag):
        h = {nm: to_host(getattr(res, nm)) for nm in ("clock", "ec", "ic", "iec", "ivc", "ivv", "id_clock", "id_keys")}
        nval, idn = res.nval.cpu().numpy(), res.id_n.cpu().numpy()
        for s in range(N):
            idef = {k: [(h["id_clock"][s, k, i], O.bitmap_members(h["id_keys"][s, k, i:i + 1]))
                        for i in range(int(idn[s, k]))] for k in range(K)}
            got = O.dense_to_nested_map(h["clock"][s], h["ec"][s], h["ic"][s], h["iec"][s], h["ivc"][s], h["ivv"][s],
                                        nval[s], idef, U.slot_deferred(slots, s))
            assert canon(got) == canon(objs[s]), (tag, s)

    check("ingest")
    states = i32(np.arange(N))
    z32, z64 = i32(np.zeros(N)), i64(np.zeros(N))
    no_keys = (i64(np.zeros(N + 1)), i32([0]))

    # -- nested_get -> derive_add_ctx -> Up with an inner Up with a Put: the one context at every level
    qk = _mixed_keys(objs, K)
    actors = [(s + 1) % A for s in range(N)]
    ikeys = [(s + 1) % K2 for s in range(N)]
    vals = [8000 + s for s in range(N)]
    rc, qst = cg.map.nested_get(res, states, i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    ops = cg.map.MapNestedOpBatch(i64(np.arange(N + 1)), u8(np.zeros(N)), add.actor, add.counter, i32(qk),
                                  u8(np.zeros(N)), add.actor, add.counter, i32(ikeys), i64(vals), z64,
                                  i32(np.arange(N)), add.clock, *no_keys)
    status = cg.map.nested_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, add.status, status)
    present, lens = _mixed(rc.val.present, N), rc.val.len.cpu().numpy()
    for s, m in enumerate(objs):
        got = m.get(qk[s])
        assert bool(present[s]) == (got.val is not None) and lens[s] == (got.val.len().val if got.val else 0)
        m.apply(m.update(qk[s], got.derive_add_ctx(actors[s]),
                         lambda v, c, j=ikeys[s], x=vals[s]: v.update(j, c, lambda reg, cx: reg.write(x, cx))))
    check("put")

    # -- nested_get_inner -> derive_rm_ctx -> Up with an inner Rm (a present inner key, absent in state 2)
    qk, qj = [], []
    for s, m in enumerate(objs):
        k = next(k for k, e in sorted(m.entries.items()) if 0 < len(e.val.entries) < K2)
        held = sorted(m.entries[k].val.entries)
        qk.append(k)
        qj.append(held[0] if s != 2 else next(j for j in range(K2) if j not in held))
    actors = [(s + 2) % A for s in range(N)]
    rc, qst = cg.map.nested_get(res, states, i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    irc, ist = cg.map.nested_get_inner(res, states, i32(qk), i32(qj), ctx=gpu_ctx)
    rm = cg.derive_rm_ctx(irc)
    ops = cg.map.MapNestedOpBatch(i64(np.arange(N + 1)), u8(np.zeros(N)), add.actor, add.counter, i32(qk),
                                  u8(np.ones(N)), z32, z64, z32, z64, i64([1 << j for j in qj]), i32(np.arange(N)),
                                  rm.clock, *no_keys)
    status = cg.map.nested_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, ist, add.status, status)
    present = _mixed(irc.val.present, N)
    nvals = irc.val.nval.cpu().numpy()
    for s, m in enumerate(objs):
        want = m.get(qk[s]).val.get(qj[s])
        assert bool(present[s]) == (want.val is not None) and nvals[s] == (len(want.val.vals) if want.val else 0)
        m.apply(m.update(qk[s], m.get(qk[s]).derive_add_ctx(actors[s]),
                         lambda v, c, j=qj[s], w=want: v.rm(j, w.derive_rm_ctx())))
    check("inner rm")

    # -- nested_get -> derive_rm_ctx -> outer Rm
    qs, qk = _present_absent(objs, K)
    Q = len(qs)
    rc, qst = cg.map.nested_get(res, i32(qs), i32(qk), ctx=gpu_ctx)
    f, q32, q64 = _map_rm_fields(rc, qs, qk)
    ops = cg.map.MapNestedOpBatch(f["op_off"], f["kind"], q32, q64, q32, u8(np.zeros(Q)), q32, q64, q32, q64, q64,
                                  f["clk_row"], f["clk_pool"], f["key_off"], f["keys"])
    status = cg.map.nested_apply_batch(res, *slots, ops, ctx=gpu_ctx)
    _quiet(qst, status)
    present = _mixed(rc.val.present, Q)
    for q in range(Q):
        m = objs[qs[q]]
        want = m.get(qk[q])
        assert bool(present[q]) == (want.val is not None)
        m.apply(m.rm(qk[q], want.derive_rm_ctx()))
    check("rm")
