"""GPU parity of the value-typed Maps' batched state equality (crdt_map_counter_eq_batch,
crdt_map_orswot_eq_batch, crdt_map_nested_eq_batch) against the oracle's `==` on objects built from the
same arrays (eq_vmap_util): x by op replay, y derived from x by every mutation class of the type, every
word of every run compared with the oracle's and with the swapped call; plus garbage where nothing may
be read, one-sided presence, nested lists past the LDS hash window, the INVALID counts, aliasing, the
empty batch, dimension mismatches and a host-memory ctx."""
import numpy as np
import pytest

import eq_vmap_util as V

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

CALL = {"counter": cg.map.counter_eq_batch, "orswot": cg.map.orswot_eq_batch, "nested": cg.map.nested_eq_batch}


def small_of(K, A, T, counter=False):
    return (min(K, 5), min(A, 4), T if counter else min(T, 6))


def run(kind, ctx, x, y, sx=None, sy=None):
    """-> (the device's words, the oracle's); the swapped call must give the same words."""
    sx, sy = sx or V.side(kind, x), sy or V.side(kind, y)
    got = CALL[kind](sx, sy, ctx=ctx).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(CALL[kind](sy, sx, ctx=ctx).cpu().numpy(), got)  # == is symmetric
    return got, V.expected(kind, x, y)


def base(kind, seed, K, A, T, N=None, Dcap=6, **kw):
    small = small_of(K, A, T, kind == "counter")
    N = N or V.pairs_for(kind)
    pool = V.pool(kind, seed, 12, small)
    Dcap = max([len(m.deferred) for m in pool] + [0]) + Dcap
    return V.densify(kind, pool, N, K, A, T, Dcap, small=small, **kw), Dcap


def mutated(kind, seed, K, A, T, vs_y=None):
    x, Dcap = base(kind, seed, K, A, T)
    y = V.widen_slots(x, Dcap + 3)  # another Dcap
    if kind != "counter":
        y = V.widen_lists(y, 20)  # Vd / Id 16 on x, 20 on y
    if vs_y:
        y = V.widen_regs(y, vs_y)
    applied = V.mutate(kind, x, y, K, T, seed)
    exp = V.expected(kind, x, y)
    V.check_classes(kind, applied, exp)
    return x, y, exp


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("K,A", [(5, 4), (9, 7), (70, 6), (6, 70), (3, 300)])
def test_map_counter_eq_batch(gpu_ctx, W, K, A):
    """Odd A (8-byte words), two key-bitmap words, a row longer than a wave, several pieces per lane."""
    x, y, exp = mutated("counter", 11 + K + W, K, A, W)
    got, _ = run("counter", gpu_ctx, x, y)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)


@pytest.mark.parametrize("K,M,A", [(4, 6, 4), (5, 9, 7), (3, 70, 5), (4, 5, 70), (2, 40, 64)])
def test_map_orswot_eq_batch(gpu_ctx, K, M, A):
    """Mw = 2 at M = 70; (2, 40, 64) is 20 KiB a key, past the segment-to-workgroup switch."""
    x, y, exp = mutated("orswot", 21 + M, K, M, A)
    got, _ = run("orswot", gpu_ctx, x, y)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)


@pytest.mark.parametrize("K,K2,A,Vs", [(3, 4, 4, 8), (4, 5, 7, 8), (2, 70, 5, 8), (3, 4, 70, 8), (2, 3, 6, 20)])
def test_map_nested_eq_batch(gpu_ctx, K, K2, A, Vs):
    """K2w = 2 at K2 = 70; the last shape has Vs = 8 on x and 20 on y."""
    x, y, exp = mutated("nested", 31 + K2 + A, K, K2, A, vs_y=Vs if Vs != 8 else None)
    got, _ = run("nested", gpu_ctx, x, y)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)


SHAPE = {"counter": (6, 2, 6),"orswot": (5, 7, 6), "nested": (4, 5, 6)}  # K, T (W / M / K2), A


@pytest.mark.parametrize("kind", ["counter", "orswot", "nested"])
def test_garbage_where_nothing_is_read(gpu_ctx, kind):
    """Equal states whose unread rows differ: absent keys' value arrays, nested slots at and past the
    counts, register slots at and past nval, and another Dcap / Vd / Id / Vs on y."""
    K, T, A = SHAPE[kind]
    x, Dcap = base(kind, 41, K, A, T, N=24)
    x["ec"][::3, 1] = 0  # a key absent on both sides, its value rows still there
    y = V.widen_slots(x, Dcap + 5)
    if kind != "counter":
        y = V.widen_lists(y, 20)
    if kind == "nested":
        y = V.widen_regs(y, 11)
    rng = np.random.default_rng(3)
    V.garbage(kind, x, rng)
    V.garbage(kind, y, rng)
    past = np.arange(y["dcl"].shape[1])[None, :] >= y["cnt"][:, None]
    y["dcl"][past] = 7
    got, exp = run(kind, gpu_ctx, x, y)
    assert not exp.any() and np.array_equal(got, exp)
    assert not all(np.array_equal(x[k], y[k]) for k in x)  # not equal byte by byte


@pytest.mark.parametrize("kind", ["counter", "orswot", "nested"])
def test_one_sided_presence(gpu_ctx, kind):
    """A key present on x only: ENTRIES, and VALUES exactly when x's value is not V::default().  y keeps
    the key's value rows (stale): they must not be read as a value."""
    K, T, A = SHAPE[kind]
    x, _ = base(kind, 42, K, A, T, N=8)
    vals = {"counter": ("val",), "orswot": ("oc", "ent", "vn"), "nested": ("ic", "iec", "vn")}[kind]
    for s in range(8):
        x["ec"][s, 2] = 0
        x["ec"][s, 2, s % A] = 9  # present on x
        if s % 2 == 0:  # ... with the default value
            for nm in vals:
                x[nm][s, 2] = 0
        elif kind == "counter":
            x["val"][s, 2, -1, 0] = 3
        elif s % 4 == 1:
            x["oc" if kind == "orswot" else "ic"][s, 2, 0] += V.U1
        else:  # only a member / inner entry row, the value's clock zero
            x["oc" if kind == "orswot" else "ic"][s, 2] = 0
            x["vn"][s, 2] = 0
            x["ent" if kind == "orswot" else "iec"][s, 2] = 0
            x["ent" if kind == "orswot" else "iec"][s, 2, -1, -1] = 5
    y = V.copy_state(x)
    y["ec"][:, 2] = 0
    got, exp = run(kind, gpu_ctx, x, y)
    assert exp.tolist() == [V.ENTRIES, V.ENTRIES | V.VALUES] * 4  # the oracle's verdicts
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["orswot", "nested"])
def test_nested_lists_past_the_lds_window(gpu_ctx, kind):
    """One key with 130 live nested slots (Vd / Id = 140, M / K2 = 8, A = 4): y's in reverse order is
    equal, one of y's sets flipped is VALUES, one clock changed past the window is VALUES."""
    K, T, A, L, Lcap = 2, 8, 4, 130, 140
    x, _ = base(kind, 43, K, A, T, N=4, Lcap=Lcap)
    rng = np.random.default_rng(9)
    x["ec"][:, 1, 0] = 4
    x["vn"][:, 1] = L
    x["vcl"][:, 1, :L] = 0
    x["vcl"][:, 1, :L, 1] = np.arange(1, L + 1, dtype=np.uint64) + np.uint64(1 << 40)
    x["vset"][:, 1, :L, 0] = rng.integers(1, 255, size=(4, L), dtype=np.uint64)
    y = V.copy_state(x)
    for s in range(1, 4):
        y["vcl"][s, 1, :L] = x["vcl"][s, 1, :L][::-1]
        y["vset"][s, 1, :L] = x["vset"][s, 1, :L][::-1]
    y["vset"][2, 1, 3, 0] ^= np.uint64(2)
    y["vcl"][3, 1, 1, 2] = 6  # the slot that was x's 128: past the window on x
    got, exp = run(kind, gpu_ctx, x, y)
    assert exp.tolist() == [0, 0, V.VALUES, V.VALUES]  # the oracle's verdicts
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind,field,cap", [("counter", "cnt", "dcl"), ("orswot", "cnt", "dcl"), ("orswot", "vn", "vcl"),
                                            ("nested", "cnt", "dcl"), ("nested", "vn", "vcl"), ("nested", "nval", "ivc")])
def test_invalid_counts(gpu_ctx, kind, field, cap):
    """A count above its capacity on one side of one pair: exactly NE_INVALID there (the pair also
    differs in its clock, an entry clock and a value), the neighbours as the oracle says."""
    K, T, A = SHAPE[kind]
    x, _ = base(kind, 44, K, A, T, N=5)
    y = V.copy_state(x)
    V.mutate(kind, x, y, K, T, 5)
    y["clock"][2, 0] += V.U1
    x["ec"][2, 0, 0], y["ec"][2, 0, 0] = 3, 4
    vrow = {"counter": "val", "orswot": "oc", "nested": "ic"}[kind]
    x[vrow][2, 0].flat[0], y[vrow][2, 0].flat[0] = 5, 6
    capacity = {"dcl": 1, "vcl": 2, "ivc": 3}[cap]
    for bad_x in (True, False):
        sx, sy = V.side(kind, x), V.side(kind, y)
        got, exp = run(kind, gpu_ctx, x, y, sx, sy)
        assert exp[2] == V.CLOCK | V.ENTRIES | V.VALUES and exp[1] != V.INVALID and np.array_equal(got, exp)
        st, arr = (sx, x) if bad_x else (sy, y)
        t = getattr(st, {"cnt": "def_count", "vn": "vd_n" if kind == "orswot" else "id_n", "nval": "nval"}[field])
        t[2].view(-1)[-1] = arr[cap].shape[capacity] + 1
        want = exp.copy()
        want[2] = cg.NE_INVALID
        assert np.array_equal(run(kind, gpu_ctx, x, y, sx, sy)[0], want)


@pytest.mark.parametrize("kind", ["counter", "orswot", "nested"])
def test_aliased_empty_mismatch_and_host_ctx(gpu_ctx, kind):
    K, T, A = SHAPE[kind]
    x, _ = base(kind, 45, K, A, T, N=9)
    sx = V.side(kind, x)
    assert not CALL[kind](sx, sx, ctx=gpu_ctx).cpu().numpy().any()
    z = type(sx)(*[t[:0] for t in sx])
    assert tuple(CALL[kind](z, z, ctx=gpu_ctx).shape) == (0,)
    for dims in ((K + 1, T, A), (K, T + 1, A), (K, T, A + 1)):
        o, _ = base(kind, 45, dims[0], dims[2], dims[1], N=9)
        with pytest.raises(ValueError):
            CALL[kind](sx, V.side(kind, o), ctx=gpu_ctx)
    o, _ = base(kind, 45, K, A, T, N=8)
    with pytest.raises(ValueError):
        CALL[kind](sx, V.side(kind, o), ctx=gpu_ctx)
    hctx = cg.Context(0)  # a host-memory ctx: device pointers only, refused before anything is read
    hctx.call("crdt_ctx_set_mem_kind", cg._abi.CRDT_MEM_HOST)
    try:
        with pytest.raises(cg.CrdtGpuError) as ei:
            CALL[kind](sx, sx, ctx=hctx)
        assert ei.value.code == cg._abi.CRDT_EUNSUPPORTED
    finally:
        hctx.close()
