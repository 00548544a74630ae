"""Test-side encoder / decoder of the value-typed Maps' op frames (include/crdt_gpu.h "serde wire format
of the value-typed Maps' op streams"), written from the reference's serde derives and independent of
the device code.  Ops are oracle objects over dense indices: O.MapRm, or O.MapUp whose `op` is

    "g"       a Dot                                        Map<u32, GCounter>
    "pn"      (Dot, O.PNCounter.POS / NEG)                 Map<u32, PNCounter>
    "orswot"  O.OrswotAdd / O.OrswotRm                     Map<u32, Orswot<u64, u32>>
    "nested"  O.MapUp(dot, ikey, O.MVRegPut) / O.MapRm     Map<u32, Map<u32, MVReg<u64, u32>, u32>>

`aid` / `kid` / `vid` map a dense actor / key / value-level index (member or inner key) to its id
(ascending, so index order is id order).  In 32-bit words:

    Op::Rm (every type)  = 0, VClock, u64 k, k x u32 key
    Op::Up, "g"          = 1, Dot, u32 key, Dot
    Op::Up, "pn"         = 1, Dot, u32 key, Dot, u32 dir (0 Pos, 1 Neg)
    Op::Up, "orswot"     = 1, Dot, u32 key, 0 (Add), Dot, u64 k, k x u64 member
                         | 1, Dot, u32 key, 1 (Rm), VClock, u64 k, k x u64 member
    Op::Up, "nested"     = 1, Dot, u32 key, 0 (inner Rm), VClock, u64 k, k x u32 ikey
                         | 1, Dot, u32 key, 1 (inner Up), Dot, u32 ikey, 0 (Put), VClock, u64 val
    frame                = u64 n_ops, then the ops back to back
"""
import struct

import oracle as O
from wire_ops_util import identity, pack_frames, sparse_dict  # noqa: F401  (re-exported)

KINDS = ("g", "pn", "orswot", "nested")


def _u32(x):
    return struct.pack("<I", int(x))


def _u64(x):
    return struct.pack("<Q", int(x))


def _dot(d, aid):
    return _u32(aid[d.actor]) + _u64(d.counter)


def _clock(v, aid):
    return O.bc_vclock({int(aid[a]): c for a, c in v.dots.items()})


def _set32(xs, ids):
    xs = sorted(xs)
    return _u64(len(xs)) + b"".join(_u32(ids[x]) for x in xs)


def enc_op(kind, op, aid, kid, vid=None, members=None) -> bytes:
    """`members` (Orswot values): the member list written (any order, duplicates allowed); default ascending."""
    if isinstance(op, O.MapRm):
        return _u32(0) + _clock(op.clock, aid) + _set32(op.keyset, kid)
    head = _u32(1) + _dot(op.dot, aid) + _u32(kid[op.key])
    v = op.op
    if kind == "g":
        return head + _dot(v, aid)
    if kind == "pn":
        d, way = v
        return head + _dot(d, aid) + _u32(0 if way == O.PNCounter.POS else 1)
    if kind == "orswot":
        ms = sorted(v.members) if members is None else list(members)
        tail = _u64(len(ms)) + b"".join(_u64(vid[m]) for m in ms)
        if isinstance(v, O.OrswotAdd):
            return head + _u32(0) + _dot(v.dot, aid) + tail
        return head + _u32(1) + _clock(v.clock, aid) + tail
    assert kind == "nested"
    if isinstance(v, O.MapRm):
        return head + _u32(0) + _clock(v.clock, aid) + _set32(v.keyset, vid)
    assert isinstance(v.op, O.MVRegPut)
    return (head + _u32(1) + _dot(v.dot, aid) + _u32(vid[v.key]) + _u32(0) + _clock(v.op.clock, aid)
            + _u64(v.op.val))


def enc_frame(kind, ops, aid, kid, vid=None) -> bytes:
    return _u64(len(ops)) + b"".join(enc_op(kind, op, aid, kid, vid) for op in ops)


class _Reader:
    def __init__(self, b):
        self.b, self.pos = b, 0

    def u32(self):
        (x,) = struct.unpack_from("<I", self.b, self.pos)
        self.pos += 4
        return x

    def u64(self):
        (x,) = struct.unpack_from("<Q", self.b, self.pos)
        self.pos += 8
        return x

    def dot(self, ai):
        a = self.u32()
        return O.Dot(ai[a], self.u64())

    def clock(self, ai):
        dots, self.pos = O.unbc_vclock(self.b, self.pos)
        return O.VClock({ai[a]: c for a, c in dots.items()})

    def set32(self, ix):
        xs = [ix[self.u32()] for _ in range(self.u64())]
        assert xs == sorted(set(xs)), "a BTreeSet serializes ascending"
        return xs


def dec_frame(kind, b: bytes, aid, kid, vid=None, with_lists=False):
    """-> the ops (and, with_lists, every Orswot op's member list as written, None for the other ops)."""
    ai = {int(x): i for i, x in enumerate(aid)}
    ki = {int(x): i for i, x in enumerate(kid)}
    vi = {int(x): i for i, x in enumerate(vid)} if vid is not None else {}
    r = _Reader(b)
    ops, lists = [], []
    for _ in range(r.u64()):
        tag = r.u32()
        ms = None
        if tag == 0:
            clk = r.clock(ai)
            ops.append(O.MapRm(clk, r.set32(ki)))
        else:
            assert tag == 1
            dot, key = r.dot(ai), ki[r.u32()]
            if kind == "g":
                v = r.dot(ai)
            elif kind == "pn":
                d = r.dot(ai)
                way = r.u32()
                assert way <= 1
                v = (d, O.PNCounter.POS if way == 0 else O.PNCounter.NEG)
            elif kind == "orswot":
                vt = r.u32()
                assert vt <= 1
                head = r.dot(ai) if vt == 0 else r.clock(ai)
                ms = [vi[r.u64()] for _ in range(r.u64())]
                v = O.OrswotAdd(head, ms) if vt == 0 else O.OrswotRm(head, ms)
            else:
                vt = r.u32()
                assert vt <= 1
                if vt == 0:
                    clk = r.clock(ai)
                    v = O.MapRm(clk, r.set32(vi))
                else:
                    idot, ikey, mv = r.dot(ai), vi[r.u32()], r.u32()
                    assert mv == 0
                    clk = r.clock(ai)
                    v = O.MapUp(idot, ikey, O.MVRegPut(clk, r.u64()))
            ops.append(O.MapUp(dot, key, v))
        lists.append(ms)
    assert r.pos == len(b), "trailing bytes"
    return (ops, lists) if with_lists else ops


def _nz(v):
    return tuple(sorted((a, c) for a, c in v.dots.items() if c))


def op_key(kind, op):
    """Comparable form of an op (the oracle's Orswot op classes define no equality)."""
    if isinstance(op, O.MapRm):
        return ("rm", _nz(op.clock), tuple(sorted(op.keyset)))
    head = ("up", op.dot.actor, op.dot.counter, op.key)
    v = op.op
    if kind == "g":
        return head + (v.actor, v.counter)
    if kind == "pn":
        return head + (v[0].actor, v[0].counter, v[1])
    if kind == "orswot":
        if isinstance(v, O.OrswotAdd):
            return head + ("add", v.dot.actor, v.dot.counter, tuple(sorted(v.members)))
        return head + ("orm", _nz(v.clock), tuple(sorted(v.members)))
    if isinstance(v, O.MapRm):
        return head + ("irm", _nz(v.clock), tuple(sorted(v.keyset)))
    return head + ("put", v.dot.actor, v.dot.counter, v.key, _nz(v.op.clock), v.op.val)


def op_tuple(kind, op):
    """The tuple map.encode_counter_ops / encode_orswot_map_ops / encode_nested_ops take."""
    if isinstance(op, O.MapRm):
        return ("rm", dict(op.clock.dots), sorted(op.keyset))
    a, c, k, v = op.dot.actor, op.dot.counter, op.key, op.op
    if kind == "g":
        return ("up", a, c, k, v.actor, v.counter, 0)
    if kind == "pn":
        return ("up", a, c, k, v[0].actor, v[0].counter, 0 if v[1] == O.PNCounter.POS else 1)
    if kind == "orswot":
        if isinstance(v, O.OrswotAdd):
            return ("add", a, c, k, v.dot.actor, v.dot.counter, sorted(v.members))
        return ("orm", a, c, k, dict(v.clock.dots), sorted(v.members))
    if isinstance(v, O.MapRm):
        return ("irm", a, c, k, dict(v.clock.dots), sorted(v.keyset))
    return ("put", a, c, k, v.dot.actor, v.dot.counter, v.key, dict(v.op.clock.dots), v.op.val)


def random_clock(rng, A, most=3, full=0.0):
    """A VClock over up to `most` actors; with probability `full`, over all A of them."""
    n = A if rng.random() < full else int(rng.integers(0, min(A, most) + 1))
    return O.VClock({int(a): int(rng.integers(1, 6)) for a in rng.choice(A, size=n, replace=False)})


def random_ops(kind, rng, n, A, K, U=0, full=0.0):
    """n ops of every variant of the type (U: members M or inner keys K2)."""
    ops = []
    for _ in range(n):
        if rng.random() < 0.3:
            ops.append(O.MapRm(random_clock(rng, A, full=full),
                               {int(k) for k in rng.choice(K, size=int(rng.integers(0, min(K, 3) + 1)), replace=False)}))
            continue
        dot, key = O.Dot(int(rng.integers(A)), int(rng.integers(1, 9))), int(rng.integers(K))
        vdot = O.Dot(int(rng.integers(A)), int(rng.integers(1, 1 << 40)))
        if kind == "g":
            v = vdot
        elif kind == "pn":
            v = (vdot, O.PNCounter.POS if rng.random() < 0.5 else O.PNCounter.NEG)
        elif kind == "orswot":
            ms = [int(m) for m in rng.choice(U, size=int(rng.integers(0, min(U, 6) + 1)), replace=False)]
            v = O.OrswotAdd(vdot, ms) if rng.random() < 0.6 else O.OrswotRm(random_clock(rng, A, full=full), ms)
        elif rng.random() < 0.6:
            v = O.MapUp(vdot, int(rng.integers(U)), O.MVRegPut(random_clock(rng, A, full=full), int(rng.integers(1, 1 << 60))))
        else:
            v = O.MapRm(random_clock(rng, A, full=full),
                        {int(j) for j in rng.choice(U, size=int(rng.integers(0, min(U, 6) + 1)), replace=False)})
        ops.append(O.MapUp(dot, key, v))
    return ops
