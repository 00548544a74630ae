"""Plain NumPy uint64 / Python-int restatements of the row-stream operations, written from the
reference's semantics (vclock.rs:68-80, :95-105, :218-227, :246-259; gcounter.rs:70-72;
pncounter.rs:110-115; orswot.rs:150-183; map.rs:85-114; mvreg.rs:88-104; lwwreg.rs:84-98) on the
dense convention "actor absent <=> 0".  test_row_ref_cpu.py checks each against the oracle's
objects; the GPU tests then compare bit for bit against these at sizes where one object per row
would be too slow."""
import numpy as np

import oracle as O

U64 = np.uint64
NONE = (1 << 64) - 1  # first_conflict: no merge erred
EDGES = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=U64)
GLB, FORGET, INTERSECTION = "glb", "forget", "intersection"


def edge_counters(rng, shape, p_edge=0.3, small=6):
    """Counters below `small` with a share p_edge drawn from EDGES (both sides of the sign bit and of
    the u64 wrap)."""
    out = rng.integers(0, small, size=shape).astype(U64)
    edge = rng.random(shape) < p_edge
    out[edge] = EDGES[rng.integers(0, len(EDGES), size=int(edge.sum()))]
    return out


def edge_pairs(rng, N, A, p_edge=0.3):
    """Row pairs from edge_counters in every ordering: a quarter each equal, y below x, y above x,
    unrelated.  With N >= 64 all four partial_cmp results appear (cmp_ref of the pairs says so)."""
    x = edge_counters(rng, (N, A), p_edge)
    r = edge_counters(rng, (N, A), p_edge)
    kind = np.arange(N) % 4
    rng.shuffle(kind)
    k = kind[:, None]
    y = np.where(k == 0, x, np.where(k == 1, np.minimum(x, r), np.where(k == 2, np.maximum(x, r), r)))
    return x, y.astype(U64)


def pair_ref(op, x, y):
    x, y = np.asarray(x, U64), np.asarray(y, U64)
    if op == GLB:
        return np.minimum(x, y)
    if op == FORGET:
        return np.where(x > y, x, U64(0))
    if op == INTERSECTION:
        return np.where(x == y, x, U64(0))
    raise ValueError(op)


def _codes(ge, le):
    return np.where(ge & le, 0, np.where(ge, 1, np.where(le, -1, 2))).astype(np.int8)


def cmp_ref(x, y):
    """partial_cmp of row pairs: Equal 0, Greater 1, Less -1, None 2."""
    x, y = np.asarray(x, U64), np.asarray(y, U64)
    return _codes((x >= y).all(-1), (x <= y).all(-1))


def cmp_matrix_ref(x):
    x = np.asarray(x, U64)
    return _codes((x[:, None, :] >= x[None, :, :]).all(-1), (x[:, None, :] <= x[None, :, :]).all(-1))


def _row_sums(rows):
    """Exact sums of (N, W) u64 rows as Python ints: the 32-bit halves summed apart (W < 2^32 terms
    of < 2^32 cannot wrap a u64), then combined."""
    rows = np.asarray(rows, U64)
    lo = (rows & U64(0xFFFFFFFF)).sum(axis=-1, dtype=U64)
    hi = (rows >> U64(32)).sum(axis=-1, dtype=U64)
    return [int(l) + (int(h) << 32) for l, h in zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist())]


def sum128_ref(rows, pn=False):
    """GCounter::read of every row; pn: rows are P ‖ N and the read is P - N (signed)."""
    rows = np.asarray(rows, U64)
    rows = rows.reshape(1, -1) if rows.ndim == 1 else rows
    if not pn:
        return _row_sums(rows)
    A = rows.shape[1] // 2
    return [p - n for p, n in zip(_row_sums(rows[:, :A]), _row_sums(rows[:, A:]))]


def _per_state(y, N):
    y = np.asarray(y, U64)
    return np.broadcast_to(y, (N, y.shape[-1])) if y.ndim == 1 else y


def _fgt(x, y):
    return np.where(x > y, x, U64(0))


def deferred_forget_ref(def_clock, def_state, ys):
    """Deferred rm clocks forget their own state's y; keep = the row is still nonempty.  A row naming
    a state >= N is left as it is with keep = 1."""
    N = ys.shape[0]
    dc = np.asarray(def_clock, U64)
    st = np.asarray(def_state).astype(np.int64) & 0xFFFFFFFF  # the kernels read the index as u32
    valid = st < N
    yd = ys[np.where(valid, st, 0)]
    out = np.where(valid[:, None], _fgt(dc, yd), dc)
    keep = np.where(valid, out.any(-1), True).astype(np.uint8)
    return out, keep


def orswot_forget_ref(clock, entries, y, def_clock=None, def_state=None):
    """-> (clock', entries', def_clock', keep): no compaction, an emptied entry is an all-zero row."""
    clock, entries = np.asarray(clock, U64), np.asarray(entries, U64)
    ys = _per_state(y, clock.shape[0])
    dc = keep = None
    if def_clock is not None:
        dc, keep = deferred_forget_ref(def_clock, def_state, ys)
    return _fgt(clock, ys), _fgt(entries, ys[:, None, :]), dc, keep


def map_forget_ref(clock, ec, vclk, vval, y, def_clock=None, def_state=None):
    """-> (clock', ec', vclk', vval', def_clock', keep) of Map<K, MVReg>::forget on dense states."""
    clock, ec, vclk, vval = (np.asarray(t, U64) for t in (clock, ec, vclk, vval))
    ys = _per_state(y, clock.shape[0])
    ec2 = _fgt(ec, ys[:, None, :])
    alive = ec2.any(-1)
    vclk2 = np.where(alive[:, :, None, None] & (vclk > ys[:, None, None, :]), vclk, U64(0))
    vval2 = np.where(vclk2.any(-1), vval, U64(0))
    dc = keep = None
    if def_clock is not None:
        dc, keep = deferred_forget_ref(def_clock, def_state, ys)
    return _fgt(clock, ys), ec2, vclk2, vval2, dc, keep


def lww_ref(marker, val, init=None):
    """The fold of one group -> (marker, val, first_conflict).  init = (marker, val) is the state the
    fold continues from: it is merged as a replica before replica 0, and the conflict index counts
    this call's replicas."""
    marker, val = np.asarray(marker, U64).reshape(-1), np.asarray(val, U64).reshape(-1)
    if init is None:
        return O.lwwreg_fold(marker, val)[:3]
    m = np.concatenate([np.array([init[0]], U64), marker])
    v = np.concatenate([np.array([init[1]], U64), val])
    om, ov, fc = O.lwwreg_fold(m, v)[:3]
    return om, ov, fc if fc == NONE else fc - 1
