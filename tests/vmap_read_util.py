"""Shared by the value-typed Maps' read tests: oracle objects -> device states through the existing
single-replica folds (each object one group, R = 1), the Map-level deferred removes the folds keep as
apply slots, and the expected outputs of every read from the oracle objects' own get / contains /
read / len."""
import numpy as np
import torch

import oracle as O
from gpu_util import to_dev, to_host

import crdts_gpu as cg

MASK = (1 << 64) - 1


def i32(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.int32), dtype=torch.int32, device="cuda:0")


def i64(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int64, device="cuda:0")


def row(vc, A):
    out = np.zeros(A, np.uint64)
    for a, c in vc.dots.items():
        out[a] = c
    return out


def bits(items, words):
    out = np.zeros(words, np.uint64)
    for i in items:
        out[i // 64] |= np.uint64(1 << (i % 64))
    return out


def total_words(x):
    """A Python integer as the (lo, hi) words of its 128-bit two's complement."""
    x &= (1 << 128) - 1
    return np.array([x & MASK, x >> 64], np.uint64)


def _group(x, N):
    return to_dev(x.reshape((N, 1) + x.shape[1:]))


def _def_kw(maps, d):
    D = d["def_row"].shape[0]
    off = [0]
    for m in maps:
        off.append(off[-1] + len(m.deferred))
    kw = dict(def_off=off, def_row=torch.zeros(D, dtype=torch.int32, device="cuda:0"),
              def_clock=to_dev(d["def_clock"]), def_keys=to_dev(d["def_keys"])) if D else {}
    return kw, off


def def_slots(res, kw, off, N, K, A, Dcap):
    """The Map-level removes a fold kept (def_keep) as apply slots (N, Dcap, A) / (N, Dcap, Kw) / (N,)."""
    Kw = (K + 63) // 64
    dcl, dks, cnt = np.zeros((N, Dcap, A), np.uint64), np.zeros((N, Dcap, Kw), np.uint64), np.zeros(N, np.int32)
    if kw:
        keep, hk, hc = res.def_keep.cpu().numpy(), to_host(res.def_keys), to_host(kw["def_clock"])
        for n in range(N):
            for j in range(off[n], off[n + 1]):
                if keep[j]:
                    dcl[n, cnt[n]], dks[n, cnt[n]] = hc[j], hk[j]
                    cnt[n] += 1
    return to_dev(dcl), to_dev(dks), torch.from_numpy(cnt).cuda()


def slot_deferred(slots, n):
    dcl, dks, cnt = to_host(slots[0]), to_host(slots[1]), slots[2].cpu().numpy()
    return [(dcl[n, i], O.bitmap_members(dks[n, i])) for i in range(int(cnt[n]))]


def counter_states(ctx, maps, K, A, W):
    N = len(maps)
    d = O.map_counter_to_dense(maps, K, A, W)
    kw, off = _def_kw(maps, d)
    res = cg.map.counter_lub_many(_group(d["clock"], N), _group(d["ec"], N), _group(d["val"], N), ctx=ctx, **kw)
    return res, kw, off


def orswot_states(ctx, maps, K, M, A):
    N = len(maps)
    d = O.map_orswot_to_dense(maps, K, M, A)
    kw, off = _def_kw(maps, d)
    Dv = int(d["vd_off"][-1])
    vkw = dict(vd_clock=to_dev(d["vd_clock"]), vd_mem=to_dev(d["vd_members"])) if Dv else {}
    res = cg.map.orswot_lub_many(_group(d["clock"], N), _group(d["ec"], N), _group(d["oc"], N), _group(d["ent"], N),
                                 to_dev(d["vd_off"]), ctx=ctx, **vkw, **kw)
    return res, kw, off


def nested_states(ctx, maps, K, K2, A):
    N = len(maps)
    V = max([len(ie.val.vals) for m in maps for e in m.entries.values() for ie in e.val.entries.values()] + [1])
    d = O.nested_map_to_dense(maps, K, K2, A, V)
    kw, off = _def_kw(maps, d)
    Di = d["id_clock"].shape[0]
    ikw = dict(id_clock=to_dev(d["id_clock"]), id_keys=to_dev(d["id_keys"])) if Di else {}
    res = cg.map.nested_lub_many(_group(d["clock"], N), _group(d["ec"], N), _group(d["ic"], N), _group(d["iec"], N),
                                 _group(d["ivc"], N), _group(d["ivv"], N), to_dev(d["id_off"]), ctx=ctx,
                                 id_cap="auto", v_cap=max(8, V), **ikw, **kw)
    return res, kw, off


def folded(maps):
    """What a single-replica fold holds: Map::new().merge(m) (the object's own deferred removes applied)."""
    return [O.map_fold_objects([m]) for m in maps]


def queries(rng, dims, extra=24):
    """Every index tuple below `dims` in shuffled order, `extra` duplicates, and one query per axis with
    that index one past its range.  -> (columns as int lists, bad: per query whether out of range)."""
    grid = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, len(dims))
    dup = grid[rng.integers(grid.shape[0], size=extra)]
    past = np.array([[d if i == ax else 0 for i, d in enumerate(dims)] for ax in range(len(dims))])
    q = np.concatenate([grid, dup, past])
    q = q[rng.permutation(q.shape[0])]
    bad = (q >= np.array(dims)).any(axis=1)
    return [q[:, i].tolist() for i in range(len(dims))], bad


# ---- expected outputs, from the oracle objects -----------------------------------------------------
def expect_counter_get(exps, qs, qk, bad, A, W):
    Q = len(qs)
    out = dict(add_clock=np.zeros((Q, A), np.uint64), rm_clock=np.zeros((Q, A), np.uint64),
               present=np.zeros(Q, np.uint8), val=np.zeros((Q, W, A), np.uint64), total=np.zeros((Q, 2), np.uint64),
               status=np.where(bad, 2, 0).astype(np.int32))
    for q in range(Q):
        if qs[q] < len(exps):
            out["add_clock"][q] = row(exps[qs[q]].clock, A)
        if bad[q]:
            continue
        r = exps[qs[q]].get(qk[q])
        out["rm_clock"][q] = row(r.rm_clock, A)
        if r.val is not None:
            out["present"][q] = 1
            out["val"][q] = O.counter_rows(r.val, A)
            out["total"][q] = total_words(r.val.read())
    return out


def expect_orswot_get(exps, qs, qk, bad, A, M):
    Q, Mw = len(qs), (M + 63) // 64
    out = dict(add_clock=np.zeros((Q, A), np.uint64), rm_clock=np.zeros((Q, A), np.uint64),
               present=np.zeros(Q, np.uint8), val_clock=np.zeros((Q, A), np.uint64),
               members=np.zeros((Q, Mw), np.uint64), len=np.zeros(Q, np.int32), vd_n=np.zeros(Q, np.int32),
               status=np.where(bad, 2, 0).astype(np.int32))
    for q in range(Q):
        if qs[q] < len(exps):
            out["add_clock"][q] = row(exps[qs[q]].clock, A)
        if bad[q]:
            continue
        r = exps[qs[q]].get(qk[q])
        out["rm_clock"][q] = row(r.rm_clock, A)
        if r.val is not None:
            rd = r.val.read()
            assert rd.add_clock == rd.rm_clock
            out["present"][q] = 1
            out["val_clock"][q] = row(rd.add_clock, A)
            out["members"][q] = bits(rd.val, Mw)
            out["len"][q] = len(rd.val)
            out["vd_n"][q] = len(r.val.deferred)
    return out


def expect_orswot_contains(exps, qs, qk, qm, bad, A):
    Q = len(qs)
    out = dict(add_clock=np.zeros((Q, A), np.uint64), rm_clock=np.zeros((Q, A), np.uint64),
               val=np.zeros(Q, np.uint8), status=np.where(bad, 2, 0).astype(np.int32))
    for q in range(Q):
        if bad[q]:
            continue
        v = exps[qs[q]].get(qk[q]).val
        r = (v if v is not None else O.Orswot()).contains(qm[q])
        out["add_clock"][q], out["rm_clock"][q], out["val"][q] = row(r.add_clock, A), row(r.rm_clock, A), r.val
    return out


def expect_nested_get(exps, qs, qk, bad, A, K2):
    Q, K2w = len(qs), (K2 + 63) // 64
    out = dict(add_clock=np.zeros((Q, A), np.uint64), rm_clock=np.zeros((Q, A), np.uint64),
               present=np.zeros(Q, np.uint8), val_clock=np.zeros((Q, A), np.uint64),
               ikeys=np.zeros((Q, K2w), np.uint64), len=np.zeros(Q, np.int32),
               status=np.where(bad, 2, 0).astype(np.int32))
    for q in range(Q):
        if qs[q] < len(exps):
            out["add_clock"][q] = row(exps[qs[q]].clock, A)
        if bad[q]:
            continue
        r = exps[qs[q]].get(qk[q])
        out["rm_clock"][q] = row(r.rm_clock, A)
        if r.val is not None:
            ln = r.val.len()
            out["present"][q] = 1
            out["val_clock"][q] = row(ln.add_clock, A)
            out["ikeys"][q] = bits(r.val.entries.keys(), K2w)
            out["len"][q] = ln.val
    return out


def expect_nested_get_inner(exps, qs, qk, qj, bad, A, Vs):
    Q = len(qs)
    out = dict(add_clock=np.zeros((Q, A), np.uint64), rm_clock=np.zeros((Q, A), np.uint64),
               present=np.zeros(Q, np.uint8), vclk=np.zeros((Q, Vs, A), np.uint64), vval=np.zeros((Q, Vs), np.uint64),
               nval=np.zeros(Q, np.int32), val_clock=np.zeros((Q, A), np.uint64),
               status=np.where(bad, 2, 0).astype(np.int32))
    for q in range(Q):
        if bad[q]:
            continue
        v = exps[qs[q]].get(qk[q]).val
        r = (v if v is not None else O.Map(O.MVReg)).get(qj[q])
        out["add_clock"][q], out["rm_clock"][q] = row(r.add_clock, A), row(r.rm_clock, A)
        if r.val is not None:
            out["present"][q] = 1
            out["nval"][q] = len(r.val.vals)
            for s, (c, x) in enumerate(r.val.vals):
                out["vclk"][q, s], out["vval"][q, s] = row(c, A), x
            out["val_clock"][q] = row(r.val.read().add_clock, A)
    return out


def got_arrays(rc, status, fields):
    """A wrapper's (ReadCtx, status) as the dict the expect_* functions build."""
    out = dict(add_clock=to_host(rc.add_clock), rm_clock=to_host(rc.rm_clock), status=status.cpu().numpy())
    if fields is None:  # val is one tensor
        out["val"] = rc.val.cpu().numpy()
        return out
    for nm in fields:
        t = getattr(rc.val, nm)
        out[nm] = to_host(t) if t.dtype == torch.int64 else t.cpu().numpy()
    return out


def assert_same(got, exp, tag=""):
    assert set(got) == set(exp), (tag, sorted(got), sorted(exp))
    for nm in exp:
        assert got[nm].shape == exp[nm].shape, (tag, nm, got[nm].shape, exp[nm].shape)
        assert np.array_equal(got[nm], exp[nm]), (tag, nm, np.argwhere(got[nm] != exp[nm])[:5])
