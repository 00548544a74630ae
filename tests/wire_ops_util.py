"""Test-side encoder / decoder of the op-stream frames (include/crdt_gpu.h "serde wire format of op
streams"), built on oracle.bc_vclock / unbc_vclock, and id mapping through sparse random
dictionaries.  Ops are oracle objects over dense indices (O.OrswotAdd / O.OrswotRm / O.MapUp /
O.MapRm); `aid` / `mid` / `kid` map a dense index to its id (ascending, so index order is id order).

    Dot<u32>                 = u32 actor, u64 counter
    orswot::Op<u64, u32>     = u32 0 (Add), Dot, u64 k, k x u64 member
                             | u32 1 (Rm),  VClock, u64 k, k x u64 member
    map::Op<u32, MVReg, u32> = u32 0 (Rm),  VClock, u64 k, k x u32 key
                             | u32 1 (Up),  Dot, u32 key, u32 0 (Put), VClock clock, u64 val
    frame                    = u64 n_ops, then the ops back to back
"""
import struct

import numpy as np

import oracle as O


def sparse_dict(rng, n, bits):
    """n distinct ids below 2**bits, ascending (a dictionary whose ids are not their indices)."""
    ids = set()
    while len(ids) < n:
        ids.update(int(x) for x in rng.integers(1, 1 << bits, size=n - len(ids), dtype=np.uint64))
    return sorted(ids)


def identity(n):
    return list(range(n))


def _clock(v, aid):
    return O.bc_vclock({int(aid[a]): c for a, c in v.dots.items()})


def enc_orswot_op(op, aid, mid, members=None) -> bytes:
    """`members`: the list written (any order, duplicates allowed); default: ascending."""
    ms = sorted(op.members) if members is None else list(members)
    tail = struct.pack("<Q", len(ms)) + b"".join(struct.pack("<Q", int(mid[m])) for m in ms)
    if isinstance(op, O.OrswotAdd):
        return struct.pack("<IIQ", 0, int(aid[op.dot.actor]), int(op.dot.counter)) + tail
    return struct.pack("<I", 1) + _clock(op.clock, aid) + tail


def enc_map_op(op, aid, kid) -> bytes:
    if isinstance(op, O.MapRm):
        ks = sorted(op.keyset)
        return (struct.pack("<I", 0) + _clock(op.clock, aid) + struct.pack("<Q", len(ks))
                + b"".join(struct.pack("<I", int(kid[k])) for k in ks))
    assert isinstance(op.op, O.MVRegPut)
    return (struct.pack("<IIQII", 1, int(aid[op.dot.actor]), int(op.dot.counter), int(kid[op.key]), 0)
            + _clock(op.op.clock, aid) + struct.pack("<Q", int(op.op.val)))


def enc_frame(ops, enc, *dicts) -> bytes:
    return struct.pack("<Q", len(ops)) + b"".join(enc(op, *dicts) for op in ops)


def enc_orswot_frame(ops, aid, mid) -> bytes:
    return enc_frame(ops, enc_orswot_op, aid, mid)


def enc_map_frame(ops, aid, kid) -> bytes:
    return enc_frame(ops, enc_map_op, aid, kid)


def _unclock(b, pos, ai):
    dots, pos = O.unbc_vclock(b, pos)
    return O.VClock({ai[a]: c for a, c in dots.items()}), pos


def dec_orswot_frame(b: bytes, aid, mid, with_lists=False):
    """-> the ops (and, with_lists, every op's member list as written)."""
    ai = {int(x): i for i, x in enumerate(aid)}
    mi = {int(x): i for i, x in enumerate(mid)}
    (n,) = struct.unpack_from("<Q", b, 0)
    pos, ops, lists = 8, [], []
    for _ in range(n):
        (tag,) = struct.unpack_from("<I", b, pos)
        pos += 4
        if tag == 0:
            a, c = struct.unpack_from("<IQ", b, pos)
            pos += 12
        else:
            assert tag == 1
            clk, pos = _unclock(b, pos, ai)
        (k,) = struct.unpack_from("<Q", b, pos)
        ms = [mi[x] for x in struct.unpack_from(f"<{k}Q", b, pos + 8)]
        pos += 8 + 8 * k
        ops.append(O.OrswotAdd(O.Dot(ai[a], c), ms) if tag == 0 else O.OrswotRm(clk, ms))
        lists.append(ms)
    assert pos == len(b), "trailing bytes"
    return (ops, lists) if with_lists else ops


def dec_map_frame(b: bytes, aid, kid):
    ai = {int(x): i for i, x in enumerate(aid)}
    ki = {int(x): i for i, x in enumerate(kid)}
    (n,) = struct.unpack_from("<Q", b, 0)
    pos, ops = 8, []
    for _ in range(n):
        (tag,) = struct.unpack_from("<I", b, pos)
        pos += 4
        if tag == 0:
            clk, pos = _unclock(b, pos, ai)
            (k,) = struct.unpack_from("<Q", b, pos)
            ks = [ki[x] for x in struct.unpack_from(f"<{k}I", b, pos + 8)]
            assert ks == sorted(set(ks)), "a BTreeSet serializes ascending"
            pos += 8 + 4 * k
            ops.append(O.MapRm(clk, ks))
        else:
            assert tag == 1
            a, c, key, mv = struct.unpack_from("<IQII", b, pos)
            assert mv == 0
            clk, pos = _unclock(b, pos + 20, ai)
            (val,) = struct.unpack_from("<Q", b, pos)
            pos += 8
            ops.append(O.MapUp(O.Dot(ai[a], c), ki[key], O.MVRegPut(clk, val)))
    assert pos == len(b), "trailing bytes"
    return ops


def orswot_key(op):
    """Comparable form of an Orswot op (the oracle's op classes define no equality)."""
    if isinstance(op, O.OrswotAdd):
        return ("add", op.dot.actor, op.dot.counter, tuple(sorted(op.members)))
    return ("rm", tuple(sorted((a, c) for a, c in op.clock.dots.items() if c)), tuple(sorted(op.members)))


def map_key(op):
    nz = lambda v: tuple(sorted((a, c) for a, c in v.dots.items() if c))  # noqa: E731
    if isinstance(op, O.MapUp):
        return ("up", op.dot.actor, op.dot.counter, op.key, nz(op.op.clock), op.op.val)
    return ("rm", nz(op.clock), tuple(sorted(op.keyset)))


def orswot_tuple(op):
    """The tuple orswot.encode_ops takes."""
    if isinstance(op, O.OrswotAdd):
        return ("add", op.dot.actor, op.dot.counter, sorted(op.members))
    return ("rm", dict(op.clock.dots), sorted(op.members))


def map_tuple(op):
    """The tuple map.encode_ops takes."""
    if isinstance(op, O.MapUp):
        return ("up", op.dot.actor, op.dot.counter, op.key, dict(op.op.clock.dots), op.op.val)
    return ("rm", dict(op.clock.dots), sorted(op.keyset))


def pack_frames(frames):
    """-> (all bytes as a uint8 array, frame_off int64 (N+1,))."""
    off, out = [0], b""
    for f in frames:
        out += f
        off.append(len(out))
    return np.frombuffer(out, dtype=np.uint8).copy(), np.asarray(off, dtype=np.int64)
