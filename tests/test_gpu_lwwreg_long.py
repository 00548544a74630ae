"""crdt_lwwreg_lub_many on groups of more than 16 and more than 256 chunks, where a workgroup scans a
group's chunk aggregates (lww_chunk_scan_block) 256 at a time with a carry between steps:
tied markers (random, and placed across a chunk edge and across the 256-chunk step edge), markers at
the top of the u64 range and all zero, groups as views of a wider buffer (group_stride > R, base at
8 and at 0 mod 16), and init= (CRDT_ACCUMULATE).  Every case is checked for marker, val and first
conflict against row_ref.lww_ref: the oracle's fold over the whole input, the init register merged
as a replica before replica 0."""
import numpy as np
import pytest

import row_ref as RR
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

CHUNK = 8 * 256  # lwwreg.hip:23-24: kLwwChunk = kBlock * kLwwPer replicas per chunk (one workgroup)
# lwwreg.hip:275: more than 16 chunks take lww_chunk_scan_block; :163: it steps 256 chunks at a time.
# 17 and 20 chunks (the smallest block scans), 257 and 258 chunks (a second step of the carry loop)
LENGTHS = [32769, 40001, 524289, 526341]
ACC_LENGTHS = [40001, 526341]
NONE = RR.NONE
TOP = (1 << 64) - 1


def n_chunks(R):
    return -(-R // CHUNK)


def test_lengths_take_the_block_scan_and_its_second_step():
    assert [n_chunks(R) for R in LENGTHS] == [17, 20, 257, 258]
    assert all(R % CHUNK for R in LENGTHS)  # a ragged last chunk


def run(ctx, m, v, init=None, col=None, pad=0):
    """lub_many of (G, R) groups, packed or as the view big[:, col:col + R] of a (G, col + R + pad) buffer
    (marker and val alike); -> [(marker, val, first_conflict)] per group."""
    m, v = np.atleast_2d(m), np.atleast_2d(v)
    G, R = m.shape
    kw = {}
    if init is not None:
        kw["init"] = (to_dev(np.array([i[0] for i in init], np.uint64)), to_dev(np.array([i[1] for i in init], np.uint64)))
    if col is None:
        dm, dv = to_dev(m), to_dev(v)
        res = cg.lwwreg.lub_many(dm, dv, ctx=ctx, **kw)
        assert np.array_equal(to_host(dm), m) and np.array_equal(to_host(dv), v)
    else:
        hm = np.full((G, col + R + pad), 0xA5A5A5A5A5A5A5A5, np.uint64)
        hv = hm.copy()
        hm[:, col:col + R], hv[:, col:col + R] = m, v
        bm, bv = to_dev(hm), to_dev(hv)
        dm, dv = bm[:, col:col + R], bv[:, col:col + R]
        assert dm.data_ptr() % 16 == (8 * col) % 16 and dm.stride(0) == col + R + pad
        res = cg.lwwreg.lub_many(dm, dv, ctx=ctx, **kw)
        assert np.array_equal(to_host(bm), hm) and np.array_equal(to_host(bv), hv)
    if init is not None:  # the caller's tensors are not the accumulator
        assert to_host(kw["init"][0]).tolist() == [i[0] for i in init]
    gm, gv, gf = (to_host(t).reshape(-1).tolist() for t in res)
    return list(zip(gm, gv, gf))


def check(ctx, m, v, init=None, **layout):
    m, v = np.atleast_2d(m), np.atleast_2d(v)
    got = run(ctx, m, v, init, **layout)
    exp = [RR.lww_ref(m[g], v[g], None if init is None else init[g]) for g in range(m.shape[0])]
    assert got == exp
    return exp


# ---------------------------------------------------------------------------------------------
# random ties
# ---------------------------------------------------------------------------------------------
def tied(rng, kind, R):
    """One group's markers and vals (vals mod 2)."""
    v = rng.integers(0, 2, size=R).astype(np.uint64)
    if kind == "mod3":
        m = rng.integers(0, 3, size=R)
    elif kind in ("mod50", "mod50-late-vals"):
        m = rng.integers(0, 50, size=R)
        if kind == "mod50-late-vals":  # equal vals up to the last seventh: the first conflict is far in
            v[:R - R // 7] = 0
    elif kind == "edges":  # the winner is 2^64 - 1
        m = RR.EDGES[rng.integers(0, len(RR.EDGES), size=R)]
    elif kind == "edges-below-top":  # the winner is 2^64 - 2
        m = RR.EDGES[rng.integers(0, len(RR.EDGES) - 1, size=R)]
    elif kind == "zeros":  # every marker 0: replica 0 wins, the first differing val conflicts
        m = np.zeros(R)
    else:
        raise ValueError(kind)
    return np.asarray(m).astype(np.uint64), v


KINDS = ["mod3", "mod50", "mod50-late-vals", "edges", "edges-below-top", "zeros"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", LENGTHS)
def test_random_ties(gpu_ctx, R, G, kind):
    rng = np.random.default_rng(R + 10 * G + KINDS.index(kind))
    kinds = [kind] if G == 1 else [kind, "edges", "zeros"]
    m, v = (np.stack(t) for t in zip(*(tied(rng, k, R) for k in kinds)))
    exp = check(gpu_ctx, m, v)
    want = {"edges": TOP, "edges-below-top": TOP - 1, "zeros": 0}
    for k, e in zip(kinds, exp):
        assert k not in want or e[0] == want[k]
        assert e[2] != NONE  # ties with differing vals: some merge erred
    if kind == "mod50-late-vals":
        assert exp[0][2] >= R - R // 7


# ---------------------------------------------------------------------------------------------
# placed ties
# ---------------------------------------------------------------------------------------------
def unique_small(rng, R):
    """Unique markers 1..R (no two tie) with random vals: no merge errs."""
    return (1 + rng.permutation(R)).astype(np.uint64), rng.integers(0, 1 << 62, size=R).astype(np.uint64)


def edge_chunks(R):
    """c whose chunk c + 1 exists: the first chunk edge, the last edge a 16-chunk group has not, the
    256-chunk step edge, and the last whole chunk (chunk c + 1 is the ragged one)."""
    return [c for c in (0, 15, 255, R // CHUNK - 1) if (c + 1) * CHUNK < R]


def straddle(rng, R, c, conflict, top=TOP):
    """The maximum at the last index of chunk c and again at the first index of chunk c + 1."""
    m, v = unique_small(rng, R)
    i, j = c * CHUNK + CHUNK - 1, (c + 1) * CHUNK
    m[i] = m[j] = top
    v[j] = v[i] ^ np.uint64(1) if conflict else v[i]
    return m, v, (top, int(v[i]), j if conflict else NONE)


@pytest.mark.parametrize("conflict", [True, False], ids=["other-val", "equal-val"])
@pytest.mark.parametrize("R,c", [(R, c) for R in LENGTHS for c in edge_chunks(R)])
def test_tie_across_a_chunk_edge(gpu_ctx, R, c, conflict):
    rng = np.random.default_rng(R + c)
    m, v, want = straddle(rng, R, c, conflict, TOP if c % 2 else (1 << 63) + 5)
    assert check(gpu_ctx, m, v) == [want]


@pytest.mark.parametrize("R", LENGTHS)
def test_ties_across_chunk_edges_three_groups(gpu_ctx, R):
    rng = np.random.default_rng(R)
    cs = edge_chunks(R)
    groups = [straddle(rng, R, cs[-1], True), straddle(rng, R, cs[0], False), straddle(rng, R, cs[len(cs) // 2], True, 1 << 63)]
    m, v = np.stack([g[0] for g in groups]), np.stack([g[1] for g in groups])
    assert check(gpu_ctx, m, v) == [g[2] for g in groups]


@pytest.mark.parametrize("R", LENGTHS)
def test_maximum_only_in_the_ragged_last_chunk(gpu_ctx, R):
    rng = np.random.default_rng(R + 1)
    last0 = (n_chunks(R) - 1) * CHUNK
    m, v = unique_small(rng, R)
    m[R - 1] = TOP
    assert check(gpu_ctx, m, v) == [(TOP, int(v[R - 1]), NONE)]
    m[last0] = TOP  # and twice in it, vals differing: the second one conflicts
    v[R - 1] = v[last0] ^ np.uint64(1)
    assert check(gpu_ctx, m, v) == [(TOP, int(v[last0]), NONE if R - 1 == last0 else R - 1)]


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", LENGTHS)
def test_maximum_at_replica_0_repeated_in_the_last_chunk(gpu_ctx, R, G):
    """Every chunk in between holds only smaller markers and takes lww_conflict's early exit; the
    conflict in the last chunk must still be found."""
    rng = np.random.default_rng(R + 2)
    ms, vs, want = [], [], []
    for g in range(G):
        m, v = unique_small(rng, R)
        j = R - 1 - g  # R - 1 is the last chunk's first index at R = k * CHUNK + 1: still that chunk
        j = max(j, (n_chunks(R) - 1) * CHUNK)
        m[0] = m[j] = TOP - g
        v[j] = v[0] ^ np.uint64(1)
        ms.append(m)
        vs.append(v)
        want.append((TOP - g, int(v[0]), j))
    assert check(gpu_ctx, np.stack(ms), np.stack(vs)) == want


# ---------------------------------------------------------------------------------------------
# layout: groups as views of a wider buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("col,odd", [(1, True), (1, False), (2, True), (2, False)],
                         ids=["at-8mod16-odd-stride", "at-8mod16-even-stride", "at-0mod16-odd-stride",
                              "at-0mod16-even-stride"])
@pytest.mark.parametrize("R", ACC_LENGTHS)
def test_groups_as_views(gpu_ctx, R, col, odd, G):
    """lwwreg.hip:266: p.vec = marker 16-byte aligned && (G == 1 || group_stride even); with p.vec false
    whole chunks are staged by 8-byte loads."""
    rng = np.random.default_rng(R + col + 2 * odd + 4 * G)
    pad = 3 + ((col + R + 3) % 2 != odd)  # -> group_stride = col + R + pad odd or even as asked
    assert (col + R + pad) % 2 == odd
    c = edge_chunks(R)[-2]
    groups = [tied(rng, "mod50-late-vals", R)] + [straddle(rng, R, c, True)[:2], tied(rng, "edges", R)][:G - 1]
    m, v = np.stack([g[0] for g in groups]), np.stack([g[1] for g in groups])
    exp = check(gpu_ctx, m, v, col=col, pad=pad)
    if G == 3:
        assert exp[1][2] == (c + 1) * CHUNK
    init = [(49, 1)] * G  # the same layouts under CRDT_ACCUMULATE
    check(gpu_ctx, m, v, init=init, col=col, pad=pad)


# ---------------------------------------------------------------------------------------------
# init= (CRDT_ACCUMULATE)
# ---------------------------------------------------------------------------------------------
def with_maximum(rng, R, at, top):
    m, v = unique_small(rng, R)
    m[at] = top
    return m, v


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", ACC_LENGTHS)
def test_init_against_the_maximum(gpu_ctx, R, G):
    rng = np.random.default_rng(R + 3 * G)
    top = (1 << 63) + 9
    at = [3 * CHUNK + 5, (n_chunks(R) - 1) * CHUNK + 1, 17 * CHUNK][:G]  # the first index holding the maximum
    ms, vs = (np.stack(t) for t in zip(*(with_maximum(rng, R, a, top) for a in at)))
    held = [int(vs[g, at[g]]) for g in range(G)]
    # above every marker: the result is init, no conflict
    assert check(gpu_ctx, ms, vs, init=[(top + 1, 7)] * G) == [(top + 1, 7, NONE)] * G
    assert check(gpu_ctx, ms, vs, init=[(TOP, 7)] * G) == [(TOP, 7, NONE)] * G
    # equal to the maximum, another val: the first index holding the maximum conflicts, init's val stays
    assert check(gpu_ctx, ms, vs, init=[(top, h ^ 1) for h in held]) == [(top, h ^ 1, a) for h, a in zip(held, at)]
    # equal to the maximum, the same val: no conflict
    assert check(gpu_ctx, ms, vs, init=[(top, h) for h in held]) == [(top, h, NONE) for h in held]
    # below the maximum
    assert check(gpu_ctx, ms, vs, init=[(top - 1, 7)] * G) == [(top, h, NONE) for h in held]
    assert check(gpu_ctx, ms, vs, init=[(0, 7)] * G) == [(top, h, NONE) for h in held]


@pytest.mark.parametrize("kind", ["mod3", "mod50-late-vals", "edges", "zeros"])
@pytest.mark.parametrize("R", ACC_LENGTHS)
def test_init_with_random_ties(gpu_ctx, R, kind):
    rng = np.random.default_rng(R + KINDS.index(kind))
    kinds = [kind, "mod50", "edges-below-top"]
    m, v = (np.stack(t) for t in zip(*(tied(rng, k, R) for k in kinds)))
    for init in ([(0, 0)] * 3, [(2, 1), (49, 0), (TOP - 1, 1)], [(TOP, 0), (50, 1), (TOP, 1)]):
        check(gpu_ctx, m, v, init=init)


@pytest.mark.parametrize("past", [0, 1], ids=["split-at-chunk-edge", "split-one-past"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", ACC_LENGTHS)
def test_init_continues_the_fold(gpu_ctx, R, G, past):
    """lub of the tail continued from the lub of the head == lub of everything (the tail alone still
    takes the block scan, at R = 526341 with its second step), and the tail's conflict index + split ==
    the global first conflict when the head has none."""
    rng = np.random.default_rng(R + G + past)
    split = CHUNK + past
    assert n_chunks(R - split) > (256 if R > 256 * CHUNK else 16)
    kinds = ["mod50-late-vals", "mod3", "edges"][:G]
    m, v = (np.stack(t) for t in zip(*(tied(rng, k, R) for k in kinds)))
    full = check(gpu_ctx, m, v)
    head = check(gpu_ctx, m[:, :split], v[:, :split])
    tail = check(gpu_ctx, m[:, split:], v[:, split:], init=[h[:2] for h in head])
    for g in range(G):
        assert tail[g][:2] == full[g][:2]
        exp = head[g][2] if head[g][2] != NONE else (NONE if tail[g][2] == NONE else tail[g][2] + split)
        assert full[g][2] == exp
    assert full[0][2] > split and head[0][2] == NONE  # group 0: the conflict lies in the tail
