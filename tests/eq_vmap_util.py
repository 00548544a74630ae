"""Shared by the value-typed Maps' batched-equality tests (crdt_map_{counter,orswot,nested}_eq_batch):
replay-built base states densified with the nested lists as [N][K][Vd | Id] slots, the mutations that
derive y from x, and the expected CRDT_NE_* words.  The words always come from the oracle's objects
(O.Map(O.GCounter / O.PNCounter / O.Orswot / lambda: O.Map(O.MVReg)) and their `==`), built here from
the numpy arrays after mutation by the header's rules (equal rm clocks union their sets, empty register
slots are skipped, a pair held twice counts once) and compared component by component; never from the
code under test.

A state is a dict of numpy arrays: clock (N, A), ec (N, K, A), dcl / dset / cnt the Map-level slots, and
  counter: val (N, K, W, A)
  orswot:  oc (N, K, A), ent (N, K, M, A), vn (N, K), vcl (N, K, Vd, A), vset (N, K, Vd, Mw)
  nested:  ic (N, K, A), iec (N, K, K2, A), ivc (N, K, K2, Vs, A), ivv (N, K, K2, Vs), nval (N, K, K2),
           vn (N, K), vcl (N, K, Id, A), vset (N, K, Id, K2w)"""
import numpy as np
import torch

import eq_util as E
import oracle as O
from crdts_gpu import wire
from gpu_util import to_dev

CLOCK, ENTRIES, VALUES, DEFERRED, INVALID = E.CLOCK, E.ENTRIES, E.VALUES, E.DEFERRED, E.INVALID
U1 = E.U1


def words_of(n):  # bitmap words of a member / inner-key set: one word up to 64
    return (n + 63) // 64 if n > 64 else 1


def vnew_of(kind, W=1):
    return {"counter": O.GCounter if W == 1 else O.PNCounter, "orswot": O.Orswot,
            "nested": lambda: O.Map(O.MVReg)}[kind]


# ---- base states by op replay ----------------------------------------------------------------------
def pool(kind, seed, P, small, lawful=False):
    """P replay-built objects at the small dims (K, A, third): lawful keeps those on which the oracle's
    own merge is idempotent."""
    K, A, T = small
    out, s = [], seed
    while len(out) < P:
        if kind == "counter":
            maps = O.map_counter_objects(2 * P, K, A, T, seed=s, steps=40 * P)
        elif kind == "orswot":
            maps = O.map_orswot_objects(2 * P, K, T, A, seed=s, steps=40 * P)
        else:
            maps = O.nested_map_objects(2 * P, K, T, A, seed=s, steps=40 * P)
        s += 1000
        for m in maps:
            if len(out) == P:
                break
            if kind == "nested" and max([len(ie.val.vals) for e in m.entries.values()
                                         for ie in e.val.entries.values()] + [0]) > 8:
                continue
            if kind != "counter" and max([len(e.val.deferred) for e in m.entries.values()] + [0]) > 12:
                continue
            if lawful:
                twice = m.copy()
                twice.merge(m.copy())
                if not (twice == m):
                    continue
            out.append(m)
    return out


def _bitmap(items, f, nw):
    out = np.zeros(nw, np.uint64)
    for it in items:
        out[f[it] // 64] |= U1 << np.uint64(f[it] % 64)
    return out


def densify(kind, maps, N, K, A, T, Dcap, Lcap=16, Vs=8, small=None):
    """N states (the pool cycled) at the full dims; the pool's keys / actors / members or inner keys
    are spread over the full ranges, the last one on the last index."""
    Ks, As, Ts = small
    kk, aa = E.spread(Ks, K), E.spread(As, A)
    tt = E.spread(Ts, T) if kind != "counter" else None
    Kw, LW = (K + 63) // 64, words_of(T)

    def row(vc):
        out = np.zeros(A, np.uint64)
        for a, c in vc.dots.items():
            out[aa[a]] = c
        return out

    st = dict(clock=np.zeros((N, A), np.uint64), ec=np.zeros((N, K, A), np.uint64),
              dcl=np.zeros((N, Dcap, A), np.uint64), dset=np.zeros((N, Dcap, Kw), np.uint64), cnt=np.zeros(N, np.int32))
    if kind == "counter":
        st["val"] = np.zeros((N, K, T, A), np.uint64)
    else:
        st.update(vn=np.zeros((N, K), np.int32), vcl=np.zeros((N, K, Lcap, A), np.uint64),
                  vset=np.zeros((N, K, Lcap, LW), np.uint64))
    if kind == "orswot":
        st.update(oc=np.zeros((N, K, A), np.uint64), ent=np.zeros((N, K, T, A), np.uint64))
    if kind == "nested":
        st.update(ic=np.zeros((N, K, A), np.uint64), iec=np.zeros((N, K, T, A), np.uint64),
                  ivc=np.zeros((N, K, T, Vs, A), np.uint64), ivv=np.zeros((N, K, T, Vs), np.uint64),
                  nval=np.zeros((N, K, T), np.int32))
    for s in range(N):
        m = maps[s % len(maps)]
        st["clock"][s] = row(m.clock)
        for d, (rm, keys) in enumerate(m.deferred.items()):
            st["dcl"][s, d], st["dset"][s, d] = row(rm), _bitmap(keys, kk, Kw)
        st["cnt"][s] = len(m.deferred)
        for k0, e in m.entries.items():
            k = kk[k0]
            st["ec"][s, k] = row(e.clock)
            if kind == "counter":
                parts = [e.val.inner] if T == 1 else [e.val.p.inner, e.val.n.inner]
                for w, vc in enumerate(parts):
                    st["val"][s, k, w] = row(vc)
                continue
            for d, (rm, items) in enumerate(e.val.deferred.items()):
                st["vcl"][s, k, d], st["vset"][s, k, d] = row(rm), _bitmap(items, tt, LW)
            st["vn"][s, k] = len(e.val.deferred)
            if kind == "orswot":
                st["oc"][s, k] = row(e.val.clock)
                for mem, mc in e.val.entries.items():
                    st["ent"][s, k, tt[mem]] = row(mc)
            else:
                st["ic"][s, k] = row(e.val.clock)
                for j0, ie in e.val.entries.items():
                    j = tt[j0]
                    st["iec"][s, k, j] = row(ie.clock)
                    for q, (vcl, x) in enumerate(ie.val.vals):
                        st["ivc"][s, k, j, q], st["ivv"][s, k, j, q] = row(vcl), x
                    st["nval"][s, k, j] = len(ie.val.vals)
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def widen(st, key, axis, n):
    """A copy with n slots along `axis` of array `key` (zero padded): another Dcap / Vd / Id / Vs."""
    out = copy_state(st)
    pad = [(0, 0)] * st[key].ndim
    pad[axis] = (0, n - st[key].shape[axis])
    out[key] = np.pad(st[key], pad)
    return out


def widen_lists(st, n):
    return widen(widen(st, "vcl", 2, n), "vset", 2, n)


def widen_slots(st, n):
    return widen(widen(st, "dcl", 1, n), "dset", 1, n)


def widen_regs(st, n):
    return widen(widen(st, "ivc", 3, n), "ivv", 3, n)


# ---- dense numpy state -> device side --------------------------------------------------------------
def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).cuda()


def side(kind, st):
    slots = (to_dev(st["dcl"]), to_dev(st["dset"]), _i32(st["cnt"]))
    if kind == "counter":
        return wire.MapCounterFrames(to_dev(st["clock"]), to_dev(st["ec"]), to_dev(st["val"]), *slots)
    vset = st["vset"][..., 0] if st["vset"].shape[-1] == 1 else st["vset"]
    if kind == "orswot":
        return wire.MapOrswotFrames(to_dev(st["clock"]), to_dev(st["ec"]), to_dev(st["oc"]), to_dev(st["ent"]),
                                    _i32(st["vn"]), to_dev(st["vcl"]), to_dev(vset), *slots)
    return wire.MapNestedFrames(to_dev(st["clock"]), to_dev(st["ec"]), to_dev(st["ic"]), to_dev(st["iec"]),
                                to_dev(st["ivc"]), to_dev(st["ivv"]), _i32(st["nval"]), _i32(st["vn"]),
                                to_dev(st["vcl"]), to_dev(vset), *slots)


# ---- expected words from the oracle's objects ------------------------------------------------------
def _deferred(cl, sets, n):
    out = {}
    for d in range(int(n)):
        out.setdefault(O._vc_row(cl[d]), set()).update(O.bitmap_members(sets[d]))
    return out


def value_object(kind, st, s, k):
    if kind == "counter":
        return O.counter_from_rows(st["val"][s, k], st["val"].shape[2])
    if kind == "orswot":
        o = O.Orswot()
        o.clock = O._vc_row(st["oc"][s, k])
        for m in np.flatnonzero(st["ent"][s, k].any(axis=1)):
            o.entries[int(m)] = O._vc_row(st["ent"][s, k, m])
    else:
        o = O.Map(O.MVReg)
        o.clock = O._vc_row(st["ic"][s, k])
        for j in np.flatnonzero(st["iec"][s, k].any(axis=1)):
            vals = []
            for q in range(int(st["nval"][s, k, j])):
                if st["ivc"][s, k, j, q].any():
                    v = (O._vc_row(st["ivc"][s, k, j, q]), int(st["ivv"][s, k, j, q]))
                    if v not in vals:
                        vals.append(v)
            o.entries[int(j)] = O.MapEntry(O._vc_row(st["iec"][s, k, j]), O.MVReg(vals))
    o.deferred = _deferred(st["vcl"][s, k], st["vset"][s, k], st["vn"][s, k])
    return o


def map_object(kind, st, s):
    m = O.Map(vnew_of(kind, st["val"].shape[2] if kind == "counter" else 1))
    m.clock = O._vc_row(st["clock"][s])
    for k in np.flatnonzero(st["ec"][s].any(axis=1)):
        m.entries[int(k)] = O.MapEntry(O._vc_row(st["ec"][s, k]), value_object(kind, st, s, int(k)))
    m.deferred = _deferred(st["dcl"][s], st["dset"][s], st["cnt"][s])
    return m


def map_word(a, b, vnew):
    w = (CLOCK if a.clock != b.clock else 0) | (DEFERRED if a.deferred != b.deferred else 0)
    if {k: e.clock for k, e in a.entries.items()} != {k: e.clock for k, e in b.entries.items()}:
        w |= ENTRIES
    val = lambda m, k: m.entries[k].val if k in m.entries else vnew()  # noqa: E731
    if any(not (val(a, k) == val(b, k)) for k in set(a.entries) | set(b.entries)):
        w |= VALUES
    assert (w == 0) == (a == b)  # the components are the whole of the oracle's ==
    return w


def expected(kind, x, y):
    N = x["clock"].shape[0]
    vnew = vnew_of(kind, x["val"].shape[2] if kind == "counter" else 1)
    return np.array([map_word(map_object(kind, x, s), map_object(kind, y, s), vnew) for s in range(N)], np.int32)


# ---- mutations: y derived from a copy of x ---------------------------------------------------------
class VMutator(E.Mutator):
    """The Map-level classes are eq_util.Mutator's (clock, ec, dcl / dset / cnt); the value classes are
    added here.  `lst` runs the deferred classes on the nested lists, one "pair" per key."""

    def __init__(self, vkind, x, y, K, T, seed):
        super().__init__("map", x, y, K, seed)
        self.vkind, self.K = vkind, K
        if vkind != "counter":
            flat = lambda st: dict(dcl=st["vcl"].reshape((-1,) + st["vcl"].shape[2:]),  # noqa: E731
                                   dset=st["vset"].reshape((-1,) + st["vset"].shape[2:]), cnt=st["vn"].reshape(-1))
            self.lst = E.Mutator("orswot", flat(x), flat(y), T, seed + 1)
            self.lst.fresh = 1 << 42

    def a_key(self, i):  # a key present in y[i] (and, y being a copy, in x[i])
        live = np.flatnonzero(self.y["ec"][i].any(axis=1) & self.x["ec"][i].any(axis=1))
        return int(live[int(self.rng.integers(len(live)))]) if len(live) else None

    def regs(self, st, i):
        out = []
        for k in np.flatnonzero(st["ec"][i].any(axis=1)):
            for j in np.flatnonzero(st["iec"][i, k].any(axis=1)):
                out.append((st["ivc"][i, k, j], st["ivv"][i, k, j]))
        return out

    def renorm(self, i):  # nval covers the last non-empty slot again
        used = self.y["ivc"][i].any(axis=-1)
        self.y["nval"][i] = np.where(used.any(axis=-1), used.shape[-1] - np.argmax(used[..., ::-1], axis=-1), 0)

    def _reg(self, name, i):
        ok = getattr(E.Mutator, name)(self, i)
        self.renorm(i)
        return ok

    def reg_permuted(self, i):
        r = self.a_register(i, need=2)
        if r is None:
            return False
        n = int(np.flatnonzero(r[0].any(axis=1))[-1]) + 1
        r[0][:n] = np.roll(r[0][:n], 1, axis=0)
        r[1][:n] = np.roll(r[1][:n], 1)
        return True

    def reg_hole(self, i):
        return self._reg("hole", i)

    def reg_value_changed(self, i):
        return self._reg("value_changed", i)

    def reg_slot_added(self, i):
        return self._reg("slot_added", i)

    def reg_slot_dropped(self, i):
        return self._reg("slot_dropped", i)

    def value_cell(self, i):
        k, y = self.a_key(i), self.y
        if k is None:
            return False
        if self.vkind == "counter":
            y["val"][i, k, -1, int(self.rng.integers(y["val"].shape[3]))] += U1  # PNCounter: the N row
            return True
        arr = y["ent" if self.vkind == "orswot" else "iec"][i, k]
        c = self.a_cell(arr)
        if c is None:
            return False
        arr[c] += U1
        return True

    def member_row_zeroed(self, i):
        k = self.a_key(i)
        if k is None:
            return False
        arr = self.y["ent" if self.vkind == "orswot" else "iec"][i, k]
        live = np.flatnonzero(arr.any(axis=1))
        if not len(live):
            return False
        arr[int(live[int(self.rng.integers(len(live)))])] = 0
        return True

    def vclock_cell(self, i):
        k = self.a_key(i)
        if k is None:
            return False
        arr = self.y["oc" if self.vkind == "orswot" else "ic"]
        arr[i, k, int(self.rng.integers(arr.shape[2]))] += U1
        return True

    def _list(self, name, i):
        k = self.a_key(i)
        return k is not None and getattr(self.lst, name)(i * self.K + k)

    def list_reversed(self, i):
        return self._list("deferred_permuted", i)

    def list_bit(self, i):
        return self._list("deferred_bit", i)

    def list_clock_cell(self, i):
        return self._list("deferred_clock_cell", i)

    def list_empty_slot(self, i):
        return self._list("deferred_empty_slot", i)

    def list_split(self, i):
        return self._list("deferred_split", i)

    def two_components(self, i):
        return self.value_cell(i) and self.clock_cell(i)  # value_cell changes nothing when it does not apply


MAP_CLASSES = ["identical", "clock_cell", "last_cell", "high32", "row_zeroed", "value_cell", "deferred_permuted",
               "deferred_bit", "deferred_split", "two_components"]
LIST_CLASSES = ["member_row_zeroed", "vclock_cell", "list_reversed", "list_bit", "list_clock_cell", "list_empty_slot",
                "list_split"]
REG_CLASSES = ["reg_permuted", "reg_hole", "reg_value_changed", "reg_slot_added", "reg_slot_dropped"]
CLASSES = {"counter": MAP_CLASSES, "orswot": MAP_CLASSES + LIST_CLASSES, "nested": MAP_CLASSES + LIST_CLASSES + REG_CLASSES}
EQUAL = ("identical", "deferred_permuted", "deferred_split", "list_reversed", "list_split", "reg_permuted", "reg_hole")
VERDICT = dict(clock_cell=CLOCK, last_cell=ENTRIES, high32=ENTRIES, row_zeroed=ENTRIES, value_cell=VALUES,
               deferred_bit=DEFERRED, member_row_zeroed=VALUES, vclock_cell=VALUES, list_bit=VALUES,
               list_clock_cell=VALUES, list_empty_slot=VALUES, reg_value_changed=VALUES, reg_slot_added=VALUES,
               reg_slot_dropped=VALUES)


def pairs_for(kind):
    return 3 * len(CLASSES[kind]) + 1


def mutate(kind, x, y, K, T, seed):
    """Spread the kind's classes over the pairs (the last pair takes last_cell).  Returns {class: [pairs
    it applied to]}; a pair whose mutation did not apply stays an identical copy."""
    mu = VMutator(kind, x, y, K, T, seed)
    N, names = x["clock"].shape[0], CLASSES[kind]
    applied = {n: [] for n in names}
    rest = [n for n in names if n != "last_cell"]
    for i in range(N):
        name = "last_cell" if i == N - 1 else rest[i % len(rest)]
        applied[name if getattr(mu, name)(i) else "identical"].append(i)
    return applied


def check_classes(kind, applied, exp):
    """Every class of the type applied to some pair, and the classes with a fixed verdict have it in the
    oracle."""
    for name in CLASSES[kind]:
        assert applied[name], f"mutation class {name} never applied"
    for name in EQUAL:
        assert not exp[applied.get(name, [])].any(), name  # the same state on another layout
    for name, bit in VERDICT.items():
        assert (exp[applied.get(name, [])] & bit).all(), name
    for i in applied["two_components"]:
        assert bin(int(exp[i])).count("1") >= 2
    assert exp[-1] & ENTRIES and applied["last_cell"] == [len(exp) - 1]


def garbage(kind, st, rng):
    """Random words wherever the semantics say nothing is read: the value arrays of keys absent in this
    state, nested slots at and past vn, register slots at and past nval.  In place."""
    rnd = lambda shape: rng.integers(1, 1 << 63, size=shape, dtype=np.uint64)  # noqa: E731
    absent = ~st["ec"].any(axis=2)
    names = {"counter": ("val",), "orswot": ("oc", "ent", "vcl", "vset"), "nested": ("ic", "iec", "ivc", "ivv", "vcl", "vset")}
    for nm in names[kind]:
        st[nm][absent] = rnd(st[nm][absent].shape)
    if kind == "counter":
        return st
    st["vn"][absent] = 0  # a valid count: counts are read for every key
    past = np.arange(st["vcl"].shape[2])[None, None, :] >= st["vn"][:, :, None]
    st["vcl"][past] = rnd(st["vcl"][past].shape)
    st["vset"][past] = rnd(st["vset"][past].shape)
    if kind == "nested":
        st["nval"][absent] = 0
        past = np.arange(st["ivc"].shape[3])[None, None, None, :] >= st["nval"][..., None]
        st["ivc"][past] = rnd(st["ivc"][past].shape)
        st["ivv"][past] = rnd(st["ivv"][past].shape)
    return st
