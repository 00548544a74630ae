"""Shared by the batched-equality tests (crdt_*_eq_batch): replay-built base states in the dense
pairwise layouts, the mutations that derive y from x, and the expected CRDT_NE_* words, which always
come from the oracle's objects (O.MVReg / O.Orswot / O.Map `==`), never from the code under test."""
import numpy as np
import torch

import crdts_gpu as cg
import oracle as O
from gpu_util import to_dev
from orswot_apply_util import dense_states, map_orswot, oracle_streams, replay_streams
from wire_mvreg_util import dense as mv_dense, replay as mv_replay, undense

CLOCK, ENTRIES, VALUES, DEFERRED, INVALID = 1, 2, 4, 8, 16
U1 = np.uint64(1)


def spread(n_small, n):
    """n_small indices spread over 0..n-1, the last one n-1."""
    return [int(x) for x in np.unique(np.linspace(0, n - 1, min(n_small, n)).round().astype(np.int64))]


# ---- dense numpy states -> device sides ------------------------------------------------------------
def mvreg_side(st):
    return to_dev(st["vclk"]), to_dev(st["vval"])


def _count(st):
    return torch.from_numpy(st["cnt"].astype(np.int32)).cuda()


def orswot_side(st):
    return cg.orswot.OrswotStates(to_dev(st["clock"]), to_dev(st["entries"]), to_dev(st["dcl"]), to_dev(st["dset"]),
                                  _count(st))


def map_side(st):
    return cg.map.MapStates(to_dev(st["clock"]), to_dev(st["ec"]), to_dev(st["vclk"]), to_dev(st["vval"]),
                            to_dev(st["dcl"]), to_dev(st["dset"]), _count(st))


# ---- expected words from the oracle's objects ------------------------------------------------------
def orswot_object(st, s):
    """orswot_apply_util.to_object without its distinct-clock assert: equal clocks union their sets."""
    o = O.Orswot()
    o.clock = O._vc_row(st["clock"][s])
    for m in np.flatnonzero(st["entries"][s].any(axis=1)):
        o.entries[int(m)] = O._vc_row(st["entries"][s, m])
    for d in range(int(st["cnt"][s])):
        o.deferred.setdefault(O._vc_row(st["dcl"][s, d]), set()).update(O.bitmap_members(st["dset"][s, d]))
    return o


def map_object(st, s):
    deferred = {}
    for d in range(int(st["cnt"][s])):
        deferred.setdefault(O._vc_row(st["dcl"][s, d]), set()).update(O.bitmap_members(st["dset"][s, d]))
    m = O.dense_to_map(st["clock"][s], st["ec"][s], st["vclk"][s], st["vval"][s])
    m.deferred = deferred
    return m


def expected_mvreg(x, y):
    a, b = undense(x["vclk"], x["vval"]), undense(y["vclk"], y["vval"])
    return np.array([0 if p == q else VALUES for p, q in zip(a, b)], np.int32)


def orswot_word(a, b):
    return ((CLOCK if a.clock != b.clock else 0) | (ENTRIES if a.entries != b.entries else 0)
            | (DEFERRED if a.deferred != b.deferred else 0))


def map_word(a, b):
    w = (CLOCK if a.clock != b.clock else 0) | (DEFERRED if a.deferred != b.deferred else 0)
    if {k: e.clock for k, e in a.entries.items()} != {k: e.clock for k, e in b.entries.items()}:
        w |= ENTRIES
    reg = lambda m, k: m.entries[k].val if k in m.entries else O.MVReg()  # noqa: E731
    if any(not (reg(a, k) == reg(b, k)) for k in set(a.entries) | set(b.entries)):
        w |= VALUES
    return w


def expected_orswot(x, y):
    N = x["clock"].shape[0]
    return np.array([orswot_word(orswot_object(x, s), orswot_object(y, s)) for s in range(N)], np.int32)


def expected_map(x, y):
    N = x["clock"].shape[0]
    return np.array([map_word(map_object(x, s), map_object(y, s)) for s in range(N)], np.int32)


# ---- base states by op replay ----------------------------------------------------------------------
def mvreg_pool(seed, A, vmax, P=16):
    rng = np.random.default_rng(seed)
    regs = []
    while len(regs) < P:
        r, _ = mv_replay(rng, A, min(A, 6), vmax, int(rng.integers(2, 10)), wide=0.3)
        if r.vals:
            regs.append(r)
    return regs


def orswot_pool(seed, M, A, P=16):
    mm, aa = spread(12, M), spread(4, A)
    streams = replay_streams(seed, P, len(aa), len(mm), 90)
    states = oracle_streams([O.Orswot() for _ in streams], streams)
    return [map_orswot(o, lambda a: aa[a], lambda m: mm[m]) for o in states]


def map_replay(seed, n_states, n_origins, K, n_ops):
    """Map<K, MVReg> states by op replay with the reference's ctx API (writes with the ctx of get(key),
    removes with an rm ctx read here or at another origin, test/map.rs:71-146 style), each state a random
    subset of the ops in perturbed causal order, cut at a random point: removes defer and concurrent
    writes leave several values per register."""
    rng = np.random.default_rng(seed)
    origins = [O.Map(O.MVReg) for _ in range(n_origins)]
    ops, val = [], 1
    for _ in range(n_ops):
        a = int(rng.integers(n_origins))
        m = origins[a]
        x = rng.random()
        if x < 0.1:
            m.merge(origins[int(rng.integers(n_origins))])
            continue
        k = int(rng.integers(K))
        if x < 0.75:
            op = m.update(k, m.get(k).derive_add_ctx(a), lambda r, c, v=val: r.write(v, c))
            val += 1
        else:
            src = m if rng.random() < 0.5 else origins[int(rng.integers(n_origins))]
            op = m.rm(k, src.get(k).derive_rm_ctx())
        m.apply(op)
        ops.append(op)
    maps = []
    for _ in range(n_states):
        keep = np.flatnonzero(rng.random(len(ops)) < rng.uniform(0.4, 1.0))
        idx = keep[np.argsort(keep + rng.normal(0, rng.uniform(0, 10), size=keep.shape[0]))]
        idx = idx[:int(rng.integers(len(idx) // 2, len(idx) + 1))]
        m = O.Map(O.MVReg)
        for i in idx:
            m.apply(ops[i])
        maps.append(m)
    return maps


def map_pool(seed, K, V, A, P=16, lawful=False):
    """lawful: keep only states on which the oracle's own merge is idempotent.  A replayed state whose
    dropped or reordered ops left a register holding a dominated value is not one: the reference's
    a.merge(a) drops that value."""
    kk, aa = spread(10, K), spread(3, A)
    fa = lambda c: O.VClock({aa[a]: n for a, n in c.dots.items()})  # noqa: E731
    out, s = [], seed
    while len(out) < P:
        maps = map_replay(s, 2 * P, len(aa), len(kk), 80)
        s += 1000
        for m in maps:
            if O.max_vals([m]) > V or len(out) == P:
                continue
            if lawful:
                twice = m.copy()
                twice.merge(m.copy())
                if not (twice == m):
                    continue
            r = O.Map(O.MVReg)
            r.clock = fa(m.clock)
            r.entries = {kk[k]: O.MapEntry(fa(e.clock), O.MVReg([(fa(c), v) for c, v in e.val.vals]))
                         for k, e in m.entries.items()}
            r.deferred = {fa(c): {kk[k] for k in ks} for c, ks in m.deferred.items()}
            out.append(r)
    return out


def mvreg_dense(regs, N, A, V):
    vc, vv = mv_dense([regs[i % len(regs)] for i in range(N)], A, V)
    return dict(vclk=vc, vval=vv)


def orswot_dense(pool, N, M, A, Dcap):
    c, e, dc, dm, n = dense_states([pool[i % len(pool)] for i in range(N)], M, A, Dcap)
    return dict(clock=c, entries=e, dcl=dc, dset=dm, cnt=n)


def map_dense(pool, N, K, V, A, Dcap):
    d = O.map_to_dense([pool[i % len(pool)] for i in range(N)], K, A, V)
    dcl = np.zeros((N, Dcap, A), np.uint64)
    dks = np.zeros((N, Dcap, (K + 63) // 64), np.uint64)
    cnt = np.zeros(N, np.int32)
    for j, r in enumerate(d["def_row"].astype(np.int64)):
        dcl[r, cnt[r]] = d["def_clock"][j]
        dks[r, cnt[r]] = d["def_keys"][j]
        cnt[r] += 1
    return dict(clock=d["clock"], ec=d["ec"], vclk=d["vclk"], vval=d["vval"], dcl=dcl, dset=dks, cnt=cnt)


def widen(st, keys, axis, n):
    """A copy of the dense state with `n` more (zero) slots along `axis` of the arrays `keys`."""
    out = {k: v.copy() for k, v in st.items()}
    for k in keys:
        pad = [(0, 0)] * st[k].ndim
        pad[axis[k]] = (0, n)
        out[k] = np.pad(st[k], pad)
    return out


# ---- mutations: y derived from x -------------------------------------------------------------------
class Mutator:
    """kind 'mvreg' | 'orswot' | 'map'.  Every mutation edits pair i of (x, y) in place and returns
    True when it applied.  `bits` is the set size of a deferred bitmap (M or K)."""

    def __init__(self, kind, x, y, bits, seed):
        self.kind, self.x, self.y, self.bits = kind, x, y, bits
        self.rng = np.random.default_rng(seed)
        self.fresh = 1 << 40  # counters of made-up deferred clocks: above anything the replay produced

    # registers of pair i: (vclk (V, A) view, vval (V,) view) per side
    def regs(self, st, i):
        if self.kind == "mvreg":
            return [(st["vclk"][i], st["vval"][i])]
        return [(st["vclk"][i, k], st["vval"][i, k]) for k in np.flatnonzero(st["ec"][i].any(axis=1))]

    def rows(self, st, i):  # the entry rows (member dots / entry clocks) or, for a register, its slots
        return {"mvreg": "vclk", "orswot": "entries", "map": "ec"}[self.kind], st

    def a_register(self, i, need=1):
        cand = [r for r in self.regs(self.y, i) if r[0].any(axis=1).sum() >= need]
        return cand[int(self.rng.integers(len(cand)))] if cand else None

    def a_cell(self, arr):  # index of a non-zero cell of arr, or None
        nz = np.argwhere(arr)
        return tuple(nz[int(self.rng.integers(len(nz)))]) if len(nz) else None

    def ensure_def(self, i, n):
        """At least n live deferred slots on both sides of pair i (the same fresh slots added to both)."""
        x, y = self.x, self.y
        while x["cnt"][i] < n or y["cnt"][i] < n:
            if x["cnt"][i] >= x["dcl"].shape[1] or y["cnt"][i] >= y["dcl"].shape[1] or x["cnt"][i] != y["cnt"][i]:
                return False
            self.fresh += 1
            ms = self.rng.choice(self.bits, size=min(self.bits, 3), replace=False)
            a = int(self.rng.integers(x["dcl"].shape[2]))
            for st in (x, y):
                d = st["cnt"][i]
                st["dcl"][i, d] = 0
                st["dcl"][i, d, a] = self.fresh
                st["dset"][i, d] = 0
                for m in ms:
                    st["dset"][i, d, m // 64] |= U1 << np.uint64(m % 64)
                st["cnt"][i] += 1
        return True

    # -- the classes
    def identical(self, i):
        return True

    def slots_permuted(self, i):
        r = self.a_register(i)
        if r is None:
            return False
        r[0][:] = np.roll(r[0], 1, axis=0)
        r[1][:] = np.roll(r[1], 1)
        return True

    def hole(self, i):
        r = self.a_register(i)
        if r is None or r[0][-1].any():
            return False
        s = int(np.flatnonzero(r[0].any(axis=1))[-1])  # the last value moves to the last slot
        if s == r[0].shape[0] - 1:
            return False
        r[0][-1], r[1][-1] = r[0][s], r[1][s]
        r[0][s], r[1][s] = 0, 0
        return True

    def deferred_permuted(self, i):
        if not self.ensure_def(i, 2):
            return False
        n = int(self.y["cnt"][i])
        self.y["dcl"][i, :n] = self.y["dcl"][i, :n][::-1].copy()
        self.y["dset"][i, :n] = self.y["dset"][i, :n][::-1].copy()
        return True

    def clock_cell(self, i):
        self.y["clock"][i, int(self.rng.integers(self.y["clock"].shape[1]))] += U1
        return True

    def last_cell(self, i):
        key, y = self.rows(self.y, i)
        if self.kind == "mvreg":
            used = np.flatnonzero(y[key][i].any(axis=1))
            y[key][i, int(used[-1]) if len(used) else 0, -1] += U1
        else:
            y[key][i, -1, -1] += U1
        return True

    def high32(self, i):
        key, y = self.rows(self.y, i)
        c = self.a_cell(y[key][i])
        if c is None:
            return False
        y[key][i][c] += np.uint64(2**32)
        return True

    def row_zeroed(self, i):
        key, y = self.rows(self.y, i)
        live = np.flatnonzero(y[key][i].any(axis=1))
        if not len(live):
            return False
        y[key][i, int(live[int(self.rng.integers(len(live)))])] = 0
        return True

    def value_changed(self, i):
        r = self.a_register(i)
        if r is None:
            return False
        s = int(np.flatnonzero(r[0].any(axis=1))[0])
        r[1][s] ^= np.uint64(5)
        return True

    def slot_added(self, i):
        cand = [r for r in self.regs(self.y, i) if not r[0].any(axis=1).all()]  # registers with an empty slot
        if not cand:
            return False
        r = cand[int(self.rng.integers(len(cand)))]
        s = int(np.flatnonzero(~r[0].any(axis=1))[0])
        r[0][s, int(self.rng.integers(r[0].shape[1]))] = np.uint64(1 << 41) + np.uint64(i)  # a clock no slot holds
        r[1][s] = np.uint64(77)
        return True

    def slot_dropped(self, i):
        r = self.a_register(i)
        if r is None:
            return False
        s = int(np.flatnonzero(r[0].any(axis=1))[-1])
        r[0][s], r[1][s] = 0, 0
        return True

    def deferred_bit(self, i):
        if not self.ensure_def(i, 1):
            return False
        d, m = int(self.rng.integers(self.y["cnt"][i])), int(self.rng.integers(self.bits))
        self.y["dset"][i, d, m // 64] ^= U1 << np.uint64(m % 64)
        return True

    def deferred_clock_cell(self, i):
        if not self.ensure_def(i, 1):
            return False
        d = int(self.rng.integers(self.y["cnt"][i]))
        self.y["dcl"][i, d, int(self.rng.integers(self.y["dcl"].shape[2]))] += U1
        return True

    def deferred_empty_slot(self, i):
        y = self.y
        d = int(y["cnt"][i])
        if d >= y["dcl"].shape[1]:
            return False
        self.fresh += 1
        y["dcl"][i, d] = 0
        y["dcl"][i, d, 0] = self.fresh
        y["dset"][i, d] = 0
        y["cnt"][i] += 1
        return True

    def deferred_split(self, i):
        y = self.y
        if not self.ensure_def(i, 1) or y["cnt"][i] >= y["dcl"].shape[1]:
            return False
        d, n = int(self.rng.integers(y["cnt"][i])), int(y["cnt"][i])
        ms = sorted(O.bitmap_members(y["dset"][i, d]))
        y["dcl"][i, n] = y["dcl"][i, d]
        y["dset"][i, n] = 0
        for m in ms[len(ms) // 2:]:  # the upper half moves to the second slot of the same clock
            y["dset"][i, d, m // 64] ^= U1 << np.uint64(m % 64)
            y["dset"][i, n, m // 64] |= U1 << np.uint64(m % 64)
        y["cnt"][i] += 1
        return True

    def two_components(self, i):
        return self.clock_cell(i) and (self.deferred_empty_slot(i) if self.kind == "orswot" else self.value_changed(i))


CLASSES = {
    "mvreg": ["identical", "slots_permuted", "hole", "last_cell", "high32", "value_changed", "slot_added",
              "slot_dropped"],
    "orswot": ["identical", "deferred_permuted", "clock_cell", "last_cell", "high32", "row_zeroed", "deferred_bit",
               "deferred_clock_cell", "deferred_empty_slot", "deferred_split", "two_components"],
    "map": ["identical", "slots_permuted", "hole", "deferred_permuted", "clock_cell", "last_cell", "high32",
            "row_zeroed", "value_changed", "slot_added", "slot_dropped", "deferred_bit", "deferred_clock_cell",
            "deferred_empty_slot", "deferred_split", "two_components"],
}


def mutate(kind, x, y, bits, seed):
    """Spread the kind's mutation classes over the pairs (the last pair takes last_cell).  Returns
    {class: [pairs it applied to]}; a pair whose mutation did not apply stays an identical copy."""
    mu = Mutator(kind, x, y, bits, seed)
    N = next(iter(x.values())).shape[0]
    names = CLASSES[kind]
    applied = {n: [] for n in names}
    for i in range(N):
        name = "last_cell" if i == N - 1 else [n for n in names if n != "last_cell"][i % (len(names) - 1)]
        if getattr(mu, name)(i):
            applied[name].append(i)
        else:
            applied["identical"].append(i)
    return applied
