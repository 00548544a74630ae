"""Test-side encoder / decoder of the lattice types' op-stream frames (include/crdt_gpu.h "the lattice
types' op streams") and their dense batches.  Ops are oracle objects over dense indices: O.Dot for
VClock / GCounter, (O.Dot, O.PNCounter.POS / NEG) for PNCounter, the dense element index for GSet,
(val, marker) for LWWReg; `aid` / `eid` map a dense index to its id (ascending).

    Vec<Dot<u32>>            = u64 n, n x (u32 actor, u64 counter)
    Vec<pncounter::Op<u32>>  = u64 n, n x (u32 actor, u64 counter, u32 dir: 0 = Pos, 1 = Neg)
    Vec<u64>                 = u64 n, n x u64 element
    Vec<LWWReg<u64, u64>>    = u64 n, n x (u64 val, u64 marker)
"""
import struct

import numpy as np

import oracle as O
from wire_ops_util import pack_frames, sparse_dict  # noqa: F401  (re-exported)

KINDS = ("vclock", "pncounter", "gset", "lwwreg")
REC = {"vclock": 12, "pncounter": 16, "gset": 8, "lwwreg": 16}
DIR = {O.PNCounter.POS: 0, O.PNCounter.NEG: 1}
RID = {0: O.PNCounter.POS, 1: O.PNCounter.NEG}


def enc_op(kind, op, ids) -> bytes:
    if kind == "vclock":
        return struct.pack("<IQ", int(ids[op.actor]), int(op.counter))
    if kind == "pncounter":
        dot, d = op
        return struct.pack("<IQI", int(ids[dot.actor]), int(dot.counter), DIR[d])
    if kind == "gset":
        return struct.pack("<Q", int(ids[op]))
    val, marker = op
    return struct.pack("<QQ", int(val), int(marker))


def enc_frame(kind, ops, ids=None) -> bytes:
    return struct.pack("<Q", len(ops)) + b"".join(enc_op(kind, op, ids) for op in ops)


def dec_frame(kind, b: bytes, ids=None):
    """-> the ops over dense indices; raises on a frame that is not 8 + n x rec bytes."""
    (n,) = struct.unpack_from("<Q", b, 0)
    assert len(b) == 8 + n * REC[kind], "frame length"
    inv = {int(x): i for i, x in enumerate(ids)} if ids is not None else None
    ops = []
    for i in range(n):
        pos = 8 + i * REC[kind]
        if kind == "vclock":
            a, c = struct.unpack_from("<IQ", b, pos)
            ops.append(O.Dot(inv[a], c))
        elif kind == "pncounter":
            a, c, d = struct.unpack_from("<IQI", b, pos)
            ops.append((O.Dot(inv[a], c), RID[d]))
        elif kind == "gset":
            ops.append(inv[struct.unpack_from("<Q", b, pos)[0]])
        else:
            ops.append(struct.unpack_from("<QQ", b, pos))
    return ops


class Dense:
    """The dense batch of per-state op streams, as numpy arrays (what ingest must produce)."""

    def __init__(self, kind, streams):
        self.kind = kind
        self.op_off = np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)
        flat = [op for s in streams for op in s]
        self.n = len(flat)
        self.state_idx = np.repeat(np.arange(len(streams), dtype=np.uint32), [len(s) for s in streams])
        self.actor = self.counter = self.dir = self.marker = self.val = None
        if kind == "vclock":
            self.actor = np.array([d.actor for d in flat], np.uint32)
            self.counter = np.array([d.counter for d in flat], np.uint64)
        elif kind == "pncounter":
            self.actor = np.array([d.actor for d, _ in flat], np.uint32)
            self.counter = np.array([d.counter for d, _ in flat], np.uint64)
            self.dir = np.array([DIR[x] for _, x in flat], np.uint8)
        elif kind == "gset":
            self.actor = np.array(flat, np.uint32)
        else:
            self.val = np.array([v for v, _ in flat], np.uint64)
            self.marker = np.array([m for _, m in flat], np.uint64)


def split(data: np.ndarray, off: np.ndarray):
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def replay_lww(state, ops):
    """Apply (val, marker) ops to O.LWWReg `state` one by one -> the conflict flag of every op."""
    out = []
    for val, marker in ops:
        try:
            state.update(val, marker)
            out.append(0)
        except O.ConflictingMarker:
            out.append(1)
    return out
