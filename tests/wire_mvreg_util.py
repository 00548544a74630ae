"""Test-side encoder / decoder of the standalone MVReg frames (include/crdt_gpu.h "MVReg<u64, u32> on
its own"), built on oracle.bc_vclock / unbc_vclock, plus the dense forms the tests compare with.
Registers are O.MVReg over dense actor indices with u64 values, ops O.MVRegPut; `aid` maps a dense
index to its id (ascending, so index order is id order).

    MVReg<u64, u32>     = u64 n, n x (VClock clock, u64 val), values in Vec order
    mvreg::Op<u64, u32> = u32 0 (Put), VClock clock, u64 val
    op frame            = Vec<Op>: u64 n_ops, then the ops back to back
"""
import struct

import numpy as np

import oracle as O
from wire_ops_util import identity, pack_frames, sparse_dict  # noqa: F401  (re-exported)


def _clock(v, aid):
    return O.bc_vclock({int(aid[a]): c for a, c in v.dots.items()})


def enc_reg(reg, aid) -> bytes:
    return struct.pack("<Q", len(reg.vals)) + b"".join(_clock(c, aid) + struct.pack("<Q", int(v)) for c, v in reg.vals)


def enc_put(op, aid) -> bytes:
    return struct.pack("<I", 0) + _clock(op.clock, aid) + struct.pack("<Q", int(op.val))


def enc_ops(ops, aid) -> bytes:
    return struct.pack("<Q", len(ops)) + b"".join(enc_put(op, aid) for op in ops)


def _unclock(b, pos, ai):
    dots, pos = O.unbc_vclock(b, pos)
    assert list(dots) == sorted(dots), "a BTreeMap serializes ascending"
    return O.VClock({ai[a]: c for a, c in dots.items()}), pos


def dec_reg(b: bytes, aid) -> O.MVReg:
    ai = {int(x): i for i, x in enumerate(aid)}
    (n,) = struct.unpack_from("<Q", b, 0)
    pos, r = 8, O.MVReg()
    for _ in range(n):
        c, pos = _unclock(b, pos, ai)
        (v,) = struct.unpack_from("<Q", b, pos)
        pos += 8
        r.vals.append((c, v))
    assert pos == len(b), "trailing bytes"
    return r


def dec_ops(b: bytes, aid):
    ai = {int(x): i for i, x in enumerate(aid)}
    (n,) = struct.unpack_from("<Q", b, 0)
    pos, ops = 8, []
    for _ in range(n):
        (tag,) = struct.unpack_from("<I", b, pos)
        assert tag == 0
        c, pos = _unclock(b, pos + 4, ai)
        (v,) = struct.unpack_from("<Q", b, pos)
        pos += 8
        ops.append(O.MVRegPut(c, v))
    assert pos == len(b), "trailing bytes"
    return ops


def dense(regs, A, V):
    """O.MVReg objects -> (vclk (N, V, A), vval (N, V)) uint64: values from slot 0 in Vec order."""
    vc = np.zeros((len(regs), V, A), np.uint64)
    vv = np.zeros((len(regs), V), np.uint64)
    for i, r in enumerate(regs):
        assert len(r.vals) <= V
        for s, (c, v) in enumerate(r.vals):
            assert c.dots and all(c.dots.values()), "a stored value has a non-empty clock without zeros"
            for a, k in c.dots.items():
                vc[i, s, a] = k
            vv[i, s] = v
    return vc, vv


def undense(vc, vv):
    """-> O.MVReg objects, empty slots skipped wherever they sit."""
    out = []
    for i in range(vc.shape[0]):
        r = O.MVReg()
        for s in range(vc.shape[1]):
            row = vc[i, s]
            if row.any():
                r.vals.append((O.VClock({int(a): int(row[a]) for a in np.flatnonzero(row)}), int(vv[i, s])))
        out.append(r)
    return out


def split(data, off):
    """bytes + offsets (numpy) -> the frames."""
    raw = bytes(np.asarray(data, dtype=np.uint8))
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def replay(rng, A, nact, vmax, steps, wide=0.0):
    """A register and the `steps` Puts that built it, as test/mvreg.rs:130-140 builds its registers:
    every Put's clock advances one or two random actors of a history the register sometimes adopts,
    so values end up concurrent, dominated or equal.  With probability `wide` a Put's clock advances
    more than 64 actors (A > 64)."""
    r, ops, base = O.MVReg(), [], O.VClock()
    acts = rng.choice(A, size=min(nact, A), replace=False)  # this register's writers, anywhere in 0..A
    tries = 0
    while len(ops) < steps and tries < 50 * steps + 50:
        tries += 1
        c = base.copy()
        who = rng.choice(acts, size=int(rng.integers(1, min(3, len(acts) + 1))), replace=False)
        if A > 64 and rng.random() < wide:
            who = rng.choice(A, size=int(rng.integers(65, A + 1)), replace=False)
        for a in who:
            c.apply(O.Dot(int(a), c.get(int(a)) + int(rng.integers(1, 4))))
        if rng.random() < 0.5:
            base = c.copy()
        op = O.MVRegPut(c, int(rng.integers(1, 2**63)))
        before = r.copy()
        r.apply(op)
        if len(r.vals) > vmax:  # keep within the dense form's slots
            r = before
            base.merge(r.clock())  # the next Put has seen every value: it replaces them
            continue
        ops.append(op)
    return r, ops
