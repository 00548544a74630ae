"""read -> derive ctx -> op -> apply_batch entirely on the device, against the oracle doing the same
through its API (Orswot::contains / read / rm / add, Map::get / rm / update, ReadCtx::derive_*)."""
import numpy as np
import pytest
import torch

import oracle as O
from gpu_util import to_dev, to_host
from orswot_apply_util import dense_states, oracle_streams, replay_streams, to_object

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402


def i32(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.int32), dtype=torch.int32, device="cuda:0")


def i64(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int64, device="cuda:0")


def test_orswot_read_derive_apply_loop(gpu_ctx):
    M, A, Dcap = 70, 5, 8
    streams = replay_streams(2, 3, A, M, 140)
    objs = oracle_streams([O.Orswot() for _ in streams], streams)
    # state 3: state 0 with member m0 re-added by another actor, so a remove whose context was read
    # from state 0 (the older view) leaves the newer dot
    m0 = sorted(objs[0].entries)[0]
    readd = objs[0].copy()
    actor = (max(objs[0].entries[m0].dots) + 1) % A
    readd.apply(readd.add(m0, readd.read().derive_add_ctx(actor)))
    objs.append(readd)
    N = len(objs)
    assert N == 4 and any(o.deferred for o in objs), "one state has a deferred remove pending"
    assert set(readd.entries[m0].dots) > set(objs[0].entries[m0].dots)
    clock, entries, dcl, dmb, cnt = dense_states(objs, M, A, Dcap)
    st = cg.orswot.OrswotStates(to_dev(clock), to_dev(entries), to_dev(dcl), to_dev(dmb),
                                torch.from_numpy(cnt).to("cuda:0"))

    # -- contains -> derive_rm_ctx -> Rm: query q is read on state src[q], its remove applied to dst[q]
    src, dst, mem = [], [], []
    for s in range(3):
        present = sorted(objs[s].entries)
        absent = [m for m in range(M) if m not in objs[s].entries]
        for m in (present[-1], absent[0]):
            src.append(s), dst.append(s), mem.append(m)
    src.append(0), dst.append(3), mem.append(m0)          # the concurrent re-add
    src.append(1), dst.append(2), mem.append(sorted(objs[1].entries)[0])  # a context from another replica
    order = np.argsort(dst, kind="stable")
    src, dst, mem = ([v[i] for i in order] for v in (src, dst, mem))
    rc, qst = cg.orswot.contains(st.clock, st.entries, i32(src), i32(mem), ctx=gpu_ctx)
    rm = cg.derive_rm_ctx(rc)
    Q = len(src)
    op_off = np.searchsorted(dst, np.arange(N + 1)).astype(np.int64)
    ops = cg.orswot.OrswotOpBatch(
        i64(op_off), torch.ones(Q, dtype=torch.uint8, device="cuda:0"), i32(np.zeros(Q)), i64(np.zeros(Q)),
        i32(np.arange(Q)), rm.clock, i64(np.arange(Q + 1)), i32(mem))
    status = cg.orswot.apply_batch(*st, ops, ctx=gpu_ctx)
    assert not qst.cpu().numpy().any() and not status.cpu().numpy().any()
    vals = rc.val.cpu().numpy()
    assert 0 < vals.sum() < Q
    for q in range(Q):
        want = objs[src[q]].contains(mem[q])
        assert bool(vals[q]) == want.val
        objs[dst[q]].apply(objs[dst[q]].rm(mem[q], want.derive_rm_ctx()))
    assert m0 in objs[3].entries and set(objs[3].entries[m0].dots) == {actor}, "the survivor keeps the newer dot"

    def check(tag):
        got = [to_host(t) for t in st[:4]] + [st.def_count.cpu().numpy()]
        for s in range(N):
            assert to_object(*got, s) == objs[s], (tag, s)
            for name, g, w in zip(("clock", "entries"), got[:2], dense_states(objs, M, A, Dcap)[:2]):
                assert np.array_equal(g[s], w[s]), (tag, name, s)

    check("rm")

    # -- read -> derive_add_ctx -> Add: the dot's actor / counter come from the device result
    actors = [s % A for s in range(N)]
    members = [(11 * s + 3) % M for s in range(N)]
    read = cg.orswot.read(st.clock, st.entries, ctx=gpu_ctx)
    add = cg.derive_add_ctx(read, i32(actors), ctx=gpu_ctx)
    ops = cg.orswot.OrswotOpBatch(
        i64(np.arange(N + 1)), torch.zeros(N, dtype=torch.uint8, device="cuda:0"), add.actor, add.counter,
        i32(np.zeros(N)), i64(np.zeros((1, A))), i64(np.arange(N + 1)), i32(members))
    status = cg.orswot.apply_batch(*st, ops, ctx=gpu_ctx)
    assert not add.status.cpu().numpy().any() and not status.cpu().numpy().any()
    lens = read.val[1].cpu().numpy()
    for s, o in enumerate(objs):
        r = o.read()
        assert int(lens[s]) == len(r.val)
        ctx = r.derive_add_ctx(actors[s])
        assert int(to_host(add.counter)[s]) == ctx.dot.counter
        o.apply(o.add(members[s], ctx))
    check("add")


def replay_maps(seed, n_states, A, K, n_ops):
    rng = np.random.default_rng(seed)
    origins = [O.Map(O.MVReg) for _ in range(A)]
    ops, val = [], 1
    for _ in range(n_ops):
        a = int(rng.integers(A))
        m = origins[a]
        x = rng.random()
        if x < 0.1:
            m.merge(origins[int(rng.integers(A))])
            continue
        k = int(rng.integers(K))
        if x < 0.8:
            op = m.update(k, m.get(k).derive_add_ctx(a), lambda r, c, v=val: r.write(v, c))
            val += 1
        else:
            op = m.rm(k, origins[int(rng.integers(A))].get(k).derive_rm_ctx())
        m.apply(op)
        ops.append(op)
    out = []
    for _ in range(n_states):
        keep = np.flatnonzero(rng.random(len(ops)) < rng.uniform(0.5, 1.0))
        idx = keep[np.argsort(keep + rng.normal(0, 6, size=keep.shape[0]))]
        m = O.Map(O.MVReg)
        for i in idx:
            m.apply(ops[i])
        out.append(m)
    return out


def test_map_get_derive_apply_loop(gpu_ctx):
    N, A, K, V, Dcap = 4, 4, 14, 6, 16
    Kw = (K + 63) // 64
    maps = replay_maps(5, N, A, K, 120)
    assert max(len(e.val.vals) for m in maps for e in m.entries.values()) > 1, "a register with concurrent values"
    d = O.map_to_dense(maps, K, A, V)
    dcl, dks, cnt = np.zeros((N, Dcap, A), np.uint64), np.zeros((N, Dcap, Kw), np.uint64), np.zeros(N, np.int32)
    for r, c, k in zip(d["def_row"], d["def_clock"], d["def_keys"]):
        dcl[int(r), cnt[int(r)]], dks[int(r), cnt[int(r)]] = c, k
        cnt[int(r)] += 1
    st = cg.map.MapStates(to_dev(d["clock"]), to_dev(d["ec"]), to_dev(d["vclk"]), to_dev(d["vval"]), to_dev(dcl),
                          to_dev(dks), torch.from_numpy(cnt).to("cuda:0"))

    def check(tag):
        c, e, vc, vv = (to_host(t) for t in st[:4])
        dc, dk, n = to_host(st.def_clock), to_host(st.def_keys), st.def_count.cpu().numpy()
        for s in range(N):
            deferred = [(dc[s, j], O.bitmap_members(dk[s, j])) for j in range(int(n[s]))]
            assert O.dense_to_map(c[s], e[s], vc[s], vv[s], deferred) == maps[s], (tag, s)

    check("ingest")

    # -- get -> derive_rm_ctx -> Rm (a present and an absent key per state)
    qs, qk = [], []
    for s, m in enumerate(maps):
        present = sorted(m.entries)
        absent = [k for k in range(K) if k not in m.entries]
        assert present and absent
        for k in present[:1] + absent[:1]:
            qs.append(s), qk.append(k)
    Q = len(qs)
    rc, qst = cg.map.get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    rm = cg.derive_rm_ctx(rc)
    zero32, zero64 = i32(np.zeros(Q)), i64(np.zeros(Q))
    ops = cg.map.MapOpBatch(i64(np.searchsorted(qs, np.arange(N + 1))), torch.ones(Q, dtype=torch.uint8, device="cuda:0"),
                            zero32, zero64, zero32, zero64, i32(np.arange(Q)), rm.clock, i64(np.arange(Q + 1)), i32(qk))
    status = cg.map.apply_batch(*st, ops, ctx=gpu_ctx)
    assert not qst.cpu().numpy().any() and not status.cpu().numpy().any()
    present = rc.val.present.cpu().numpy()
    assert 0 < present.sum() < Q
    for q in range(Q):
        m = maps[qs[q]]
        want = m.get(qk[q])
        assert bool(present[q]) == (want.val is not None)
        m.apply(m.rm(qk[q], want.derive_rm_ctx()))
    check("rm")

    # -- get -> derive_add_ctx -> Up with a Put whose clock is the derived one
    qs = list(range(N))
    qk = [(5 * s + 1) % K for s in range(N)]
    actors = [(s + 1) % A for s in range(N)]
    vals = [9000 + s for s in range(N)]
    rc, qst = cg.map.get(st, i32(qs), i32(qk), ctx=gpu_ctx)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    ops = cg.map.MapOpBatch(i64(np.arange(N + 1)), torch.zeros(N, dtype=torch.uint8, device="cuda:0"), add.actor,
                            add.counter, i32(qk), i64(vals), i32(np.arange(N)), add.clock, i64(np.zeros(N + 1)),
                            i32([0]))
    status = cg.map.apply_batch(*st, ops, ctx=gpu_ctx)
    assert not qst.cpu().numpy().any() and not add.status.cpu().numpy().any() and not status.cpu().numpy().any()
    for s, m in enumerate(maps):
        m.apply(m.update(qk[s], m.get(qk[s]).derive_add_ctx(actors[s]), lambda r, c, v=vals[s]: r.write(v, c)))
    check("up")
