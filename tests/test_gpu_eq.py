"""GPU parity of the batched state equality (crdt_mvreg_eq_batch, crdt_orswot_eq_batch,
crdt_map_eq_batch) against the oracle's `==` (MVReg mvreg.rs:62-86, the derived PartialEq of Orswot
orswot.rs:20, Map map.rs:31-47 and VClock vclock.rs:56): 257 pairs per shape, x built by op replay, y
derived from x by every mutation class that applies to the type (eq_util.CLASSES), all 257 words of
every run compared with the oracle's, plus the deferred-count, invalid-count, aliasing, empty-batch
and dimension-mismatch cases."""
import numpy as np
import pytest
import torch

import eq_util as E

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N = 257  # the last wave is partly idle


mvreg_side, orswot_side, map_side = E.mvreg_side, E.orswot_side, E.map_side


def check_classes(kind, applied, exp):
    """Every class of the type appears, and the classes with a fixed verdict have it in the oracle."""
    for name in E.CLASSES[kind]:
        assert applied[name], f"mutation class {name} never applied"
    assert not exp[applied["identical"]].any()
    for name in ("slots_permuted", "hole", "deferred_permuted", "deferred_split"):
        assert not exp[applied.get(name, [])].any(), name  # the same state on another layout
    for name, bit in (("deferred_empty_slot", E.DEFERRED), ("clock_cell", E.CLOCK), ("value_changed", E.VALUES),
                      ("slot_added", E.VALUES), ("slot_dropped", E.VALUES), ("row_zeroed", E.ENTRIES),
                      ("deferred_bit", E.DEFERRED), ("deferred_clock_cell", E.DEFERRED)):
        assert (exp[applied.get(name, [])] & bit).all(), name
    for i in applied.get("two_components", []):
        assert bin(int(exp[i])).count("1") >= 2
    assert exp[-1] != 0 and applied["last_cell"] == [len(exp) - 1]


@pytest.mark.parametrize("A,V", [(3, 1), (32, 4), (64, 8), (65, 16), (300, 4), (200, 3), (200, 7), (131, 3), (131, 7)])
def test_mvreg_eq_batch(gpu_ctx, A, V):
    """The non-vector path, three segment widths, V > 8 and A > 256, and two chunks per lane (128 < A <=
    256) in 16-byte pieces (A = 200) and 8-byte words (A = 131), each with 4 and with 8 slots on y; y holds
    one slot more than x (one fewer at the 16-slot limit).  The last pair differs in actor word A - 1."""
    Vy = V + 1 if V < 16 else V - 1
    pool = E.mvreg_pool(100 + A, A, min(V, Vy))
    x, y = E.mvreg_dense(pool, N, A, V), E.mvreg_dense(pool, N, A, Vy)
    applied = E.mutate("mvreg", x, y, 0, 7 * A + V)
    exp = E.expected_mvreg(x, y)
    check_classes("mvreg", applied, exp)
    got = cg.mvreg.eq_batch(*mvreg_side(x), *mvreg_side(y), ctx=gpu_ctx).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, exp), np.flatnonzero(got != exp)
    got = cg.mvreg.eq_batch(*mvreg_side(y), *mvreg_side(x), ctx=gpu_ctx).cpu().numpy()  # == is symmetric
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("M,A", [(5, 3), (33, 64), (70, 32), (4, 300)])
def test_orswot_eq_batch(gpu_ctx, M, A):
    pool = E.orswot_pool(200 + M, M, A)
    Dcap = max(len(o.deferred) for o in pool) + 3
    x = E.orswot_dense(pool, N, M, A, Dcap)
    y = E.widen(x, ("dcl", "dset"), {"dcl": 1, "dset": 1}, 2)  # Dcap larger on one side
    applied = E.mutate("orswot", x, y, M, 11 * M + A)
    exp = E.expected_orswot(x, y)
    check_classes("orswot", applied, exp)
    assert (exp[applied["two_components"]] & E.CLOCK).all()
    got = cg.orswot.eq_batch(orswot_side(x), orswot_side(y), ctx=gpu_ctx).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, exp), np.flatnonzero(got != exp)
    assert np.array_equal(cg.orswot.eq_batch(orswot_side(y), orswot_side(x), ctx=gpu_ctx).cpu().numpy(), exp)


@pytest.mark.parametrize("M,A", [(5, 3), (9, 16)])
def test_orswot_eq_batch_strided_rows(gpu_ctx, M, A):
    """x's member rows are not packed (entry_mstride = 2A): the row-by-row form of the dense kernel,
    in 8-byte words (A = 3) and 16-byte pieces (A = 16), against y's packed rows."""
    pool = E.orswot_pool(400 + M, M, A)
    Dcap = max(len(o.deferred) for o in pool) + 3
    x = E.orswot_dense(pool, N, M, A, Dcap)
    y = E.widen(x, ("dcl", "dset"), {"dcl": 1, "dset": 1}, 2)
    E.mutate("orswot", x, y, M, 17 * M + A)
    exp = E.expected_orswot(x, y)
    assert (exp & E.ENTRIES).any() and not exp.all()
    sx, sy = orswot_side(x), orswot_side(y)
    wide = torch.zeros((N, M, 2 * A), dtype=torch.int64, device="cuda:0")
    wide[:, :, A:] = -1  # the gap between rows is never read
    wide[:, :, :A] = sx.entries
    sx = sx._replace(entries=wide[:, :, :A])
    assert sx.entries.stride(1) == 2 * A
    assert np.array_equal(cg.orswot.eq_batch(sx, sy, ctx=gpu_ctx).cpu().numpy(), exp)
    assert np.array_equal(cg.orswot.eq_batch(sy, sx, ctx=gpu_ctx).cpu().numpy(), exp)


@pytest.mark.parametrize("K,V,A", [(5, 2, 3), (64, 4, 32), (70, 8, 24), (3, 20, 16), (2, 4, 300), (3, 3, 200),
                                   (3, 7, 200), (4, 3, 131), (4, 7, 131)])
def test_map_eq_batch(gpu_ctx, K, V, A):
    """Kw = 2 at K = 70, the workgroup-per-key kernel at V > 8 and A > 256, two chunks per lane at
    A = 200 (16-byte pieces) and A = 131 (8-byte words), each with 4 and 8 slots on y; y holds V + 1 value slots and two more
    deferred slots than x.  The replay's actors sit at words 0, A / 2 and A - 1."""
    pool = E.map_pool(300 + K, K, V, A)
    Dcap = max(len(m.deferred) for m in pool) + 3
    x = E.map_dense(pool, N, K, V, A, Dcap)
    y = E.widen(x, ("vclk", "vval", "dcl", "dset"), {"vclk": 2, "vval": 2, "dcl": 1, "dset": 1}, 1)
    y = E.widen(y, ("dcl", "dset"), {"dcl": 1, "dset": 1}, 1)
    applied = E.mutate("map", x, y, K, 13 * K + A)
    exp = E.expected_map(x, y)
    check_classes("map", applied, exp)
    got = cg.map.eq_batch(map_side(x), map_side(y), ctx=gpu_ctx).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, exp), np.flatnonzero(got != exp)
    assert np.array_equal(cg.map.eq_batch(map_side(y), map_side(x), ctx=gpu_ctx).cpu().numpy(), exp)


def long_lists(kind, bits, A, rng):
    """Pairs with deferred counts 0 / 0, 0 / 1 and 70 / 70 in permuted order, Dcap 70 against 96 (past
    a wave's lanes and the 16-slot window of the apply kernels); the 70 / 70 pair once equal, once
    with one set bit flipped in a late slot, once with one clock of y replaced."""
    n, W = 5, (bits + 63) // 64
    base = dict(clock=np.ones((n, A), np.uint64), cnt=np.zeros(n, np.int32))
    if kind == "orswot":
        base["entries"] = np.zeros((n, bits, A), np.uint64)
    else:
        base.update(ec=np.zeros((n, bits, A), np.uint64), vclk=np.zeros((n, bits, 1, A), np.uint64),
                    vval=np.zeros((n, bits, 1), np.uint64))
    x = dict(base, dcl=np.zeros((n, 70, A), np.uint64), dset=np.zeros((n, 70, W), np.uint64))
    y = dict({k: v.copy() for k, v in base.items()}, dcl=np.zeros((n, 96, A), np.uint64),
             dset=np.zeros((n, 96, W), np.uint64))
    y["cnt"][1] = 1
    y["dcl"][1, 0, 0] = 9
    for i in (2, 3, 4):
        clocks = rng.integers(1, 4, size=(70, A)).astype(np.uint64)
        clocks[:, 0] = np.arange(1, 71)  # pairwise distinct
        sets = rng.integers(0, 2**63, size=(70, W)).astype(np.uint64) & np.uint64((1 << min(bits, 63)) - 1)
        perm = rng.permutation(70)
        x["dcl"][i], x["dset"][i], x["cnt"][i] = clocks, sets, 70
        y["dcl"][i, :70], y["dset"][i, :70], y["cnt"][i] = clocks[perm], sets[perm], 70
    y["dset"][3, 66, 0] ^= E.U1
    y["dcl"][4, 69, A - 1] += np.uint64(100)
    return x, y


def blank(kind, n, bits, A, dx, dy):
    """n pairs of states with equal clocks, no members / keys, and dx / dy empty deferred slots."""
    W = (bits + 63) // 64
    base = dict(clock=np.ones((n, A), np.uint64), cnt=np.zeros(n, np.int32))
    if kind == "orswot":
        base["entries"] = np.zeros((n, bits, A), np.uint64)
    else:
        base.update(ec=np.zeros((n, bits, A), np.uint64), vclk=np.zeros((n, bits, 1, A), np.uint64),
                    vval=np.zeros((n, bits, 1), np.uint64))
    x = dict(base, dcl=np.zeros((n, dx, A), np.uint64), dset=np.zeros((n, dx, W), np.uint64))
    y = dict({k: v.copy() for k, v in base.items()}, dcl=np.zeros((n, dy, A), np.uint64),
             dset=np.zeros((n, dy, W), np.uint64))
    return x, y


def past_window_lists(kind, bits, A, rng):
    """200 / 200 live slots in permuted order, Dcap 200 against 224: past the 128 row hashes a side keeps
    in LDS, so slots 128.. are hashed on the fly and compared row by row.  Pair 0 equal; 1 a set bit
    flipped in y's slot 190; 2 a clock replaced in y's slot 150; 3 the clock of y's slot 140 held twice
    (slots 140 and 200) with its set split, which is equal; 4 the same with one more bit in the second
    slot, which is not."""
    n, W, D = 5, (bits + 63) // 64, 200
    x, y = blank(kind, n, bits, A, D, D + 24)
    for i in range(n):
        clocks = rng.integers(1, 4, size=(D, A)).astype(np.uint64)
        clocks[:, 0] = np.arange(1, D + 1)  # pairwise distinct
        sets = rng.integers(0, 2**63, size=(D, W)).astype(np.uint64) & np.uint64((1 << min(bits, 63)) - 1)
        sets[:, 1:] = 0
        perm = rng.permutation(D)
        x["dcl"][i], x["dset"][i], x["cnt"][i] = clocks, sets, D
        y["dcl"][i, :D], y["dset"][i, :D], y["cnt"][i] = clocks[perm], sets[perm], D
    y["dset"][1, 190, 0] ^= E.U1
    y["dcl"][2, 150, A - 1] += np.uint64(100)
    for i in (3, 4):
        y["dcl"][i, D] = y["dcl"][i, 140]
        y["dset"][i, D, 0] = y["dset"][i, 140, 0] & np.uint64(0x15)  # some of its bits move to the second slot
        y["dset"][i, 140, 0] &= ~np.uint64(0x15)
        y["cnt"][i] = D + 1
    if y["dset"][4, 140, 0] & np.uint64(2):  # bit 1 stays in the first slot's half: the union loses or gains it
        y["dset"][4, 140, 0] &= ~np.uint64(2)
    else:
        y["dset"][4, D, 0] |= np.uint64(2)
    return x, y


def run(kind, ctx, x, y, sx=None, sy=None):
    """-> (the device's words, the oracle's) for dense numpy sides (or ready device sides sx / sy)."""
    side, call = (orswot_side, cg.orswot.eq_batch) if kind == "orswot" else (map_side, cg.map.eq_batch)
    exp = (E.expected_orswot if kind == "orswot" else E.expected_map)(x, y)
    return call(sx or side(x), sy or side(y), ctx=ctx).cpu().numpy(), exp


@pytest.mark.parametrize("kind", ["orswot", "map"])
def test_eq_batch_deferred_counts(gpu_ctx, kind):
    rng = np.random.default_rng(5)
    x, y = long_lists(kind, 70, 6, rng)
    got, exp = run(kind, gpu_ctx, x, y)
    assert exp.tolist() == [0, E.DEFERRED, 0, E.DEFERRED, E.DEFERRED]  # the oracle's verdicts
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["orswot", "map"])
def test_eq_batch_deferred_past_lds_window(gpu_ctx, kind):
    rng = np.random.default_rng(8)
    x, y = past_window_lists(kind, 70, 6, rng)
    got, exp = run(kind, gpu_ctx, x, y)
    assert exp.tolist() == [0, E.DEFERRED, E.DEFERRED, 0, E.DEFERRED]  # the oracle's verdicts
    assert np.array_equal(got, exp)
    got, exp = run(kind, gpu_ctx, y, x)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["orswot", "map"])
def test_eq_batch_invalid_def_count(gpu_ctx, kind):
    """def_count above Dcap on one side: exactly NE_INVALID for that pair, its neighbours unaffected.
    The invalid pair also differs in its clock and in a member / key row (for the Map: entry clock and
    value, which the per-key kernel would otherwise OR in): no other bit is reported."""
    rng = np.random.default_rng(6)
    x, y = long_lists(kind, 5, 4, rng)
    y["clock"][2, 1] += E.U1
    rows = "entries" if kind == "orswot" else "ec"
    x[rows][2, 1, 0], y[rows][2, 1, 0] = 3, 4
    if kind == "map":
        x["vclk"][2, 1, 0, 0], y["vclk"][2, 1, 0, 0] = 2, 2
        x["vval"][2, 1, 0], y["vval"][2, 1, 0] = 5, 6
    side = orswot_side if kind == "orswot" else map_side
    for bad_x in (True, False):
        sx, sy = side(x), side(y)
        got, exp = run(kind, gpu_ctx, x, y, sx, sy)
        assert exp[2] == E.CLOCK | E.ENTRIES | (E.VALUES if kind == "map" else 0) and np.array_equal(got, exp)
        (sx if bad_x else sy).def_count[2] = 71 if bad_x else 97
        want = exp.copy()
        want[2] = cg.NE_INVALID
        assert np.array_equal(run(kind, gpu_ctx, x, y, sx, sy)[0], want)


@pytest.mark.parametrize("kind", ["orswot", "map"])
def test_eq_batch_count_with_no_slots(gpu_ctx, kind):
    """Dcap == 0 with a def_count passed: the count is still read, and a non-zero one is NE_INVALID."""
    x, y = blank(kind, 3, 5, 4, 0, 2)
    y["clock"][0, 0] += E.U1
    side = orswot_side if kind == "orswot" else map_side
    sx, sy = side(x), side(y)
    got, exp = run(kind, gpu_ctx, x, y, sx, sy)
    assert exp.tolist() == [E.CLOCK, 0, 0] and np.array_equal(got, exp)
    sx.def_count[1] = 1
    assert run(kind, gpu_ctx, x, y, sx, sy)[0].tolist() == [E.CLOCK, cg.NE_INVALID, 0]
    assert run(kind, gpu_ctx, y, x, sy, sx)[0].tolist() == [E.CLOCK, cg.NE_INVALID, 0]


def odd_word(t):
    """The same tensor at an address that is 8-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def test_eq_batch_alignment_fallbacks(gpu_ctx):
    """Every mix of 16-byte pieces and 8-byte words: an odd A with an even M * A (clock in words, member
    rows in pieces), and even shapes whose clock, member rows, value clocks or entry clocks start at an
    odd word, on either side."""
    M, A = 4, 3
    pool = E.orswot_pool(500, M, A)
    x = E.orswot_dense(pool, N, M, A, 4)
    y = E.widen(x, ("dcl", "dset"), {"dcl": 1, "dset": 1}, 2)
    E.mutate("orswot", x, y, M, 1)
    got, exp = run("orswot", gpu_ctx, x, y)
    assert (exp & E.ENTRIES).any() and (exp & E.CLOCK).any() and np.array_equal(got, exp)
    M, A = 3, 4
    pool = E.orswot_pool(501, M, A)
    x = E.orswot_dense(pool, N, M, A, 4)
    y = E.widen(x, ("dcl", "dset"), {"dcl": 1, "dset": 1}, 2)
    E.mutate("orswot", x, y, M, 2)
    for fields in (("entries",), ("clock",), ("clock", "entries")):
        sx, sy = orswot_side(x), orswot_side(y)
        sy = sy._replace(**{f: odd_word(getattr(sy, f)) for f in fields})
        got, exp = run("orswot", gpu_ctx, x, y, sx, sy)
        assert (exp & E.ENTRIES).any() and (exp & E.CLOCK).any() and np.array_equal(got, exp), fields
        assert np.array_equal(run("orswot", gpu_ctx, y, x, sy, sx)[0], exp), fields
    K, V, A = 5, 2, 8
    pool = E.map_pool(502, K, V, A)
    x = E.map_dense(pool, N, K, V, A, 4)
    y = E.widen(x, ("vclk", "vval"), {"vclk": 2, "vval": 2}, 1)
    E.mutate("map", x, y, K, 3)
    for fields in (("vclk",), ("ec",), ("clock",)):
        sx, sy = map_side(x), map_side(y)
        sx = sx._replace(**{f: odd_word(getattr(sx, f)) for f in fields})
        got, exp = run("map", gpu_ctx, x, y, sx, sy)
        assert (exp & E.VALUES).any() and (exp & E.ENTRIES).any() and np.array_equal(got, exp), fields
    A, V = 8, 3
    rx = E.mvreg_dense(E.mvreg_pool(503, A, V), N, A, V)
    ry = E.mvreg_dense(E.mvreg_pool(503, A, V), N, A, V + 1)
    E.mutate("mvreg", rx, ry, 0, 4)
    exp = E.expected_mvreg(rx, ry)
    (xc, xv), (yc, yv) = mvreg_side(rx), mvreg_side(ry)
    assert exp.any() and np.array_equal(cg.mvreg.eq_batch(xc, xv, odd_word(yc), yv, ctx=gpu_ctx).cpu().numpy(), exp)


def test_eq_batch_aliased_and_empty(gpu_ctx):
    pool = E.mvreg_pool(1, 8, 3)
    r = mvreg_side(E.mvreg_dense(pool, 33, 8, 4))
    assert not cg.mvreg.eq_batch(*r, *r, ctx=gpu_ctx).cpu().numpy().any()
    assert cg.mvreg.eq_batch(r[0][:0], r[1][:0], r[0][:0], r[1][:0], ctx=gpu_ctx).shape == (0,)
    o = orswot_side(E.orswot_dense(E.orswot_pool(2, 9, 4), 33, 9, 4, 6))
    assert not cg.orswot.eq_batch(o, o, ctx=gpu_ctx).cpu().numpy().any()
    assert cg.orswot.eq_batch(type(o)(*[t[:0] for t in o]), type(o)(*[t[:0] for t in o]), ctx=gpu_ctx).shape == (0,)
    m = map_side(E.map_dense(E.map_pool(3, 6, 3, 4), 33, 6, 3, 4, 6))
    assert not cg.map.eq_batch(m, m, ctx=gpu_ctx).cpu().numpy().any()
    assert cg.map.eq_batch(type(m)(*[t[:0] for t in m]), type(m)(*[t[:0] for t in m]), ctx=gpu_ctx).shape == (0,)


def test_eq_batch_dimension_mismatch(gpu_ctx):
    pool = E.mvreg_pool(1, 8, 3)
    a, b = mvreg_side(E.mvreg_dense(pool, 4, 8, 4)), mvreg_side(E.mvreg_dense(E.mvreg_pool(1, 6, 3), 4, 6, 4))
    with pytest.raises(ValueError, match="differ"):
        cg.mvreg.eq_batch(*a, *b, ctx=gpu_ctx)
    op = E.orswot_pool(2, 9, 4)
    for M, A in ((8, 4), (9, 5)):
        with pytest.raises(ValueError, match="differ"):
            cg.orswot.eq_batch(orswot_side(E.orswot_dense(op, 4, 9, 4, 6)),
                               orswot_side(E.orswot_dense(E.orswot_pool(2, M, A), 4, M, A, 6)), ctx=gpu_ctx)
    mp = E.map_pool(3, 6, 3, 4)
    for K, A in ((5, 4), (6, 3)):
        with pytest.raises(ValueError, match="differ"):
            cg.map.eq_batch(map_side(E.map_dense(mp, 4, 6, 3, 4, 6)),
                            map_side(E.map_dense(E.map_pool(3, K, 3, A), 4, K, 3, A, 6)), ctx=gpu_ctx)
    assert (cg.NE_CLOCK, cg.NE_ENTRIES, cg.NE_VALUES, cg.NE_DEFERRED, cg.NE_INVALID) == (1, 2, 4, 8, 16)
