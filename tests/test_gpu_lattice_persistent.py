"""GPU parity of the persistent multi-segment lattice lub: crdt_lub_many_multi launches
min(blocks, cap) workgroups and workgroup w runs blocks w, w + grid, w + 2*grid, ... of the
concatenated block list, so one workgroup runs the single-lub body several times (and may be the
last arriver of several clusters), and the last eighth of the launch's bytes is handed out in
chunks from a ticket counter (tune key lubchunk: bytes per chunk).  Whatever the grid (tune key
lubpg) and the chunk, every segment must get the oracle's fold (vclock.rs:130-136, pncounter.rs:70-75, gset.rs:38-40) and, bit for bit, what one
crdt_<kind>_lub_many call writes."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

MODS = {"vclock": cg.vclock, "gcounter": cg.gcounter, "pncounter": cg.pncounter, "gset": cg.gset}


def fold(kind, rows):
    """Oracle fold of (R, W) host rows (or (G, R, W))."""
    if rows.ndim == 3:
        return np.stack([fold(kind, r) for r in rows]) if rows.shape[0] else np.zeros((0, rows.shape[2]), np.uint64)
    if rows.shape[0] == 0:
        return np.zeros(rows.shape[1], np.uint64)
    if kind == "gset":
        return O.gset_fold(rows)[0]
    if kind == "pncounter":
        return O.pncounter_fold(rows)[0]
    return O.vclock_fold(rows)[0]


@functools.lru_cache(maxsize=None)
def segment(seed, kind, G, R, W):
    """(host rows (R, W) or (G, R, W), oracle fold) of one synthetic segment; computed once, never written."""
    rows = O.synth_matrix(seed, G * R, W, 1 if kind == "gset" else 0).reshape(G, R, W)
    rows = rows if G > 1 else rows[0]
    exp = fold(kind, rows)
    exp.setflags(write=False)
    return rows, exp


@pytest.fixture
def tuned():
    """A ctx of its own per test, so a tune spec never leaks into the session's ctx."""
    made = []

    def make(spec):
        ctx = cg.Context(0)
        if spec:
            ctx.tune(spec)
        made.append(ctx)
        return ctx

    torch.cuda.set_device(0)
    yield make
    for ctx in made:
        ctx.close()


def run_and_check(ctx, specs, seed0):
    """One lub_many_multi over `specs` [(kind, G, R, W)]: every out equals the oracle fold and the
    single-segment call."""
    items, exps = [], []
    for i, (kind, G, R, W) in enumerate(specs):
        rows, exp = segment(seed0 + i, kind, G, R, W)
        out = torch.full((G, W) if G > 1 else (W,), 7, dtype=torch.int64, device="cuda")
        items.append((kind, to_dev(rows), out))
        exps.append(exp)
    cg.lub_many_multi(items, ctx=ctx)
    for (kind, x, out), exp in zip(items, exps):
        got = to_host(out)
        np.testing.assert_array_equal(got, exp, err_msg=f"{kind} vs oracle")
        np.testing.assert_array_equal(got, to_host(MODS[kind].lub_many(x, ctx=ctx)), err_msg=f"{kind} vs lub_many")


MINI = [("gcounter", 1, 4096, 256), ("pncounter", 1, 4096, 512)]


# 64 slices per segment = two clusters each, so both combine levels run; 128 blocks in the launch:
# one workgroup running every block and every combine itself, uneven shares (3, 5), two blocks per
# workgroup (64), one block per workgroup (128) and a cap above the number of blocks (200).
@pytest.mark.parametrize("lubpg", [1, 3, 5, 64, 128, 200])
def test_bench_shape_in_miniature(tuned, lubpg):
    run_and_check(tuned(f"minsteps=1,grid=64,lubpg={lubpg}"), MINI, 0x5EED0A00)


@pytest.mark.parametrize("lubpg", [0, 3])  # 0: the default cap (one workgroup per CU)
def test_cluster_edge(tuned, lubpg):
    """33 slices: a second cluster of size 1."""
    run_and_check(tuned(f"minsteps=1,grid=33,lubpg={lubpg}"), MINI, 0x5EED0A00)


# test_gpu_lattice_multi.py's CASES: mixed kinds, G > 1, odd W (the V = 1 launch class), R = 0 and
# R = 1, W = 1024 (two column blocks), the GSet OR.
CASES = [("gcounter", 1, 2000, 256), ("pncounter", 1, 700, 2 * 100), ("vclock", 3, 77, 63), ("gset", 2, 300, 5),
         ("vclock", 1, 0, 8), ("gcounter", 40, 9, 130), ("vclock", 1, 1, 2), ("gset", 1, 4097, 64),
         ("pncounter", 5, 33, 2 * 7), ("vclock", 2, 1000, 1024), ("gcounter", 1, 65536, 6)]


@pytest.mark.parametrize("lubpg", [2, 7])
def test_mixed_cases(tuned, lubpg):
    run_and_check(tuned(f"lubpg={lubpg}"), CASES, 0x5EED0B00)


@pytest.mark.parametrize("spec", ["lubpg=3", "minsteps=1,grid=8,lubpg=3"])
def test_strided_and_accumulate(tuned, spec):
    ctx = tuned(spec)
    big, _ = segment(0x5EED0C00, "vclock", 1, 600, 80)
    dev = to_dev(big)
    views = [("vclock", dev[::3, 8:72]), ("gcounter", dev[1::2, 1:64]), ("pncounter", dev[:500, :80])]
    start = [segment(0x5EED0C01 + i, "vclock", 1, 1, v.shape[1])[0][0] for i, (_, v) in enumerate(views)]
    items = [(k, v, to_dev(s0)) for (k, v), s0 in zip(views, start)]
    cg.lub_many_multi(items, ctx=ctx, accumulate=True)
    for (kind, v, out), s0 in zip(items, start):
        got = to_host(out)
        np.testing.assert_array_equal(got, fold(kind, np.concatenate([s0[None], to_host(v)])), err_msg=kind)
        one = MODS[kind].lub_many(v, out=to_dev(s0), accumulate=True, ctx=ctx)
        np.testing.assert_array_equal(got, to_host(one), err_msg=f"{kind} vs lub_many")


def test_counter_reuse(tuned):
    """The arrival counters reset themselves: calls of different shapes on one ctx, then the first again."""
    ctx = tuned("minsteps=1,grid=64,lubpg=5")
    shapes = [MINI, [("gset", 3, 500, 64), ("gset", 1, 4097, 64)], [("vclock", 2, 1000, 1024), ("pncounter", 1, 700, 200)]]
    for k in (0, 1, 2, 1, 2, 0):
        run_and_check(ctx, shapes[k], 0x5EED0D00 + 16 * k)


# The dynamic tail at small sizes (lubchunk=1: chunks of one unrolled block step of rows).  The last
# segment decides the shape: 6 chunks per slice; fewer workgroups than slices with every row of the
# tail slices dynamic (5 workgroups, 8 chunks each); a short last slice (R = 4001); odd W (V = 1,
# TR = 4) with rows that end inside a chunk; the GSet OR; a last round that spans two segments and
# a chunk size of 0 (both: no tail).  Twice on one ctx: the ticket counter resets itself.
TAILS = [("minsteps=1,grid=16,lubpg=16,lubchunk=1", MINI),
         ("minsteps=1,grid=64,lubpg=5,lubchunk=1", MINI),
         ("minsteps=1,grid=16,lubpg=16,lubchunk=1", [("gcounter", 1, 4096, 256), ("pncounter", 1, 4001, 512)]),
         ("minsteps=1,grid=8,lubpg=8,lubchunk=1", [("gcounter", 2, 500, 129), ("vclock", 1, 3001, 63)]),
         ("minsteps=1,grid=16,lubpg=7,lubchunk=1", [("gset", 1, 300, 6), ("gset", 1, 4097, 64)]),
         ("minsteps=1,grid=16,lubpg=40,lubchunk=1", MINI),
         ("minsteps=1,grid=16,lubpg=16,lubchunk=0", MINI)]


@pytest.mark.parametrize("spec,shapes", TAILS, ids=[f"{i}" for i in range(len(TAILS))])
def test_dynamic_tail(tuned, spec, shapes):
    ctx = tuned(spec)
    for _ in range(2):
        run_and_check(ctx, shapes, 0x5EED0F00)


def test_default_tune(gpu_ctx):
    run_and_check(gpu_ctx, [("gcounter", 1, 20000, 256), ("pncounter", 1, 20000, 512)], 0x5EED0E00)
