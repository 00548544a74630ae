"""The row-stream kernels of causal.hip and forget.hip on the paths test_gpu_causal.py and
test_gpu_forget_states.py never reach: a second and a ragged third trip round the grid-stride loop
(rbpc=1 / mfbpc=1 grids, row counts sized from the device's CU count), counters with the top bit
set, the 8-byte fallbacks with even A (odd strides, bases at 8 mod 16), gap words between strided
rows, and deferred rows that name no state.  Every case is bit for bit against row_ref.py (checked
against the oracle's objects in test_row_ref_cpu.py) and runs the oracle's objects on a sample of
at least 64 of its own rows or states.  Each case restates the launcher's dispatch predicate and
asserts that it takes the branch its id names."""
import numpy as np
import pytest
import torch

import oracle as O
import row_ref as RR
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

SENT = np.uint64(0xA5A5A5A5A5A5A5A5)  # fill of every word a kernel must leave alone
CODE = {O.EQUAL: 0, O.GREATER: 1, O.LESS: -1, O.NONE: 2}
K_U = 4  # forget.hip:42 kU: row groups per lane in flight


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


# ---------------------------------------------------------------------------------------------
# sizing: restated from the launch code
# ---------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def row_lr_log(pieces, ppl=8):
    """common.hpp:364 row_lr_log: lanes per row so that a lane moves about 8 pieces."""
    lg = 0
    while lg < 6 and (pieces + (1 << lg) - 1) >> lg > ppl:
        lg += 1
    return lg


def fit_lr_log(pieces):
    """forget.hip:303 / :376: the smallest power of two of lanes >= pieces (one access per row), <= 64."""
    lg = 0
    while lg < 6 and (1 << lg) < pieces:
        lg += 1
    return lg


def pass_rows(lr_log, ku=1, bpc=1):
    """Rows one trip of the whole grid covers when the grid is capped at CU x bpc workgroups
    (causal.hip:222 rows_grid, forget.hip:183 forget_grid): 4 waves x (64 >> lr_log) rows, x kU."""
    return cu_count() * bpc * 4 * (64 >> lr_log) * ku


def wrap_rows(one_pass):
    """Three trips: two whole ones and a ragged last one that is no multiple of the rows per wave."""
    return 2 * one_pass + one_pass // 2 + 3


def al16(t):
    return t.data_ptr() % 16 == 0


def vc(row):
    return O.VClock({a: int(c) for a, c in enumerate(np.asarray(row).tolist()) if c})


def dense(v, A):
    r = np.zeros(A, np.uint64)
    for a, c in v.dots.items():
        r[a] = c
    return r


def sample_rows(rng, n, marks=()):
    """>= 64 row indices: the first, the last, the rows either side of each mark, random ones."""
    idx = {0, n - 1} | {int(i) for i in rng.integers(0, n, 64)}
    for m in marks:
        idx |= {i for i in (m - 1, m, m + 1) if 0 <= i < n}
    return sorted(idx)


class Placed:
    """Rows (..., A) laid into a flat device buffer of SENT words at word offset `off` with `stride`
    words between rows: .view is the strided tensor, .check(rows) asserts that the buffer holds `rows`
    and that every other word (gaps, the words before the first and after the last row) is SENT."""

    def __init__(self, a, stride=None, off=0, tail=5):
        a = np.ascontiguousarray(a, np.uint64)
        self.shape = a.shape
        A = a.shape[-1]
        n = a.size // A
        stride = stride or A
        self.host = np.full(off + n * stride + tail, SENT, np.uint64)
        self.idx = off + np.arange(n)[:, None] * stride + np.arange(A)[None, :]
        self.host[self.idx] = a.reshape(n, A)
        self.flat = to_dev(self.host)
        strides, s = [], stride
        for d in reversed(a.shape[:-1]):
            strides.append(s)
            s *= d
        self.view = torch.as_strided(self.flat, a.shape, tuple(reversed(strides)) + (1,), off)
        assert self.view.data_ptr() % 16 == (8 * off) % 16

    def rows(self):
        return to_host(self.flat)[self.idx].reshape(self.shape)

    def check(self, rows, what=""):
        exp = self.host.copy()
        exp[self.idx] = np.asarray(rows, np.uint64).reshape(self.idx.shape)
        got = to_host(self.flat)
        assert np.array_equal(got[self.idx], exp[self.idx]), f"{what}: rows differ"
        assert np.array_equal(got, exp), f"{what}: a word outside the rows was written"


def full_counters(rng, shape):
    """Full-range u64 counters with a share of row_ref's edge values."""
    c = rng.integers(0, (1 << 64) - 1, size=shape, dtype=np.uint64, endpoint=True)
    e = RR.edge_counters(rng, shape, 1.0)
    return np.where(rng.random(shape) < 0.3, e, c)


# ---------------------------------------------------------------------------------------------
# pair ops, partial_cmp, concurrent
# ---------------------------------------------------------------------------------------------
OPS = ((RR.GLB, cg.causal.glb), (RR.FORGET, cg.causal.forget), (RR.INTERSECTION, cg.causal.intersection))


def pair_plan(A, tensors):
    """causal.hip:248 / :266: p.vec2 = (A % 2 == 0) && ((strides or-ed) % 2 == 0) && every base
    16-byte aligned; p.lr_log = row_lr_log(p.vec2 ? A / 2 : A)."""
    vec2 = A % 2 == 0 and all(t.stride(0) % 2 == 0 for t in tensors if t.dim() == 2) and all(al16(t) for t in tensors)
    return vec2, row_lr_log(A // 2 if vec2 else A)


def check_pairs(ctx, rng, x, y, px, py, pout, marks=()):
    """All five pair entry points on placed x / y, out into pout's buffer."""
    N, A = x.shape
    outs = {}
    for op, fn in OPS:
        fn(px.view, py.view, out=pout.view, ctx=ctx)
        pout.check(RR.pair_ref(op, x, y), op)
        outs[op] = pout.rows()
    cmpv = cg.causal.partial_cmp(px.view, py.view, ctx=ctx).cpu().numpy()
    conc = cg.causal.concurrent(px.view, py.view, ctx=ctx).cpu().numpy()
    exp = RR.cmp_ref(x, y)
    assert np.array_equal(cmpv, exp)
    assert np.array_equal(conc, exp == 2)
    if N >= 64:
        assert set(exp.tolist()) == {0, 1, -1, 2}
    px.check(x, "x")  # inputs read only
    py.check(y, "y")
    for i in sample_rows(rng, N, marks):
        a, b = vc(x[i]), vc(y[i])
        g = a.copy()
        g.glb(b)
        assert np.array_equal(outs[RR.GLB][i], dense(g, A)), i
        assert np.array_equal(outs[RR.FORGET][i], dense(a.clone_without(b), A)), i
        assert np.array_equal(outs[RR.INTERSECTION][i], dense(O.VClock.intersection(a, b), A)), i
        assert cmpv[i] == CODE[a.partial_cmp(b)] and bool(conc[i]) == a.concurrent(b), i


@pytest.mark.parametrize("A,stride,vec2,lr_log", [
    pytest.param(6, None, True, 0, id="pair-16B-lr0-A6-packed"),
    pytest.param(6, 7, False, 0, id="pair-8B-lr0-A6-odd-stride"),
    pytest.param(130, None, True, 4, id="pair-16B-lr4-A130"),
    pytest.param(7, None, False, 0, id="pair-8B-lr0-A7")])
def test_pair_ops_wrap_the_grid(tuned, A, stride, vec2, lr_log):
    ctx = tuned("rbpc=1")
    one = pass_rows(lr_log)
    N = wrap_rows(one)
    rng = np.random.default_rng(1000 + A + (stride or 0))
    x, y = RR.edge_pairs(rng, N, A)
    px, py = Placed(x, stride), Placed(y, stride)
    pout = Placed(np.zeros_like(x), stride)
    assert pair_plan(A, (px.view, py.view, pout.view)) == (vec2, lr_log)
    assert 2 * one < N < 3 * one and N % (64 >> lr_log)  # a ragged third trip
    check_pairs(ctx, rng, x, y, px, py, pout, marks=(one, 2 * one))


@pytest.mark.parametrize("xo,yo,oo", [
    pytest.param(0, 1, 0, id="pair-8B-y-at-8mod16"), pytest.param(1, 0, 0, id="pair-8B-x-at-8mod16"),
    pytest.param(0, 0, 1, id="pair-8B-out-at-8mod16"), pytest.param(1, 1, 1, id="pair-8B-all-at-8mod16")])
def test_pair_ops_one_operand_misaligned(tuned, xo, yo, oo):
    ctx = tuned("")
    A, N = 6, 301
    rng = np.random.default_rng(1100 + 4 * xo + 2 * yo + oo)
    x, y = RR.edge_pairs(rng, N, A)
    px, py, pout = Placed(x, off=xo), Placed(y, off=yo), Placed(np.zeros_like(x), off=oo)
    assert pair_plan(A, (px.view, py.view, pout.view)) == (False, 0)
    assert [al16(t.view) for t in (px, py, pout)] == [not xo, not yo, not oo]
    check_pairs(ctx, rng, x, y, px, py, pout)


@pytest.mark.parametrize("S,ycol,vec2", [pytest.param(16, 8, True, id="pair-16B-in-place-even-stride"),
                                         pytest.param(15, 7, False, id="pair-8B-in-place-odd-stride")])
def test_pair_ops_in_place_on_strided_views(tuned, S, ycol, vec2):
    """out = x on rows that are views of one (N, S) buffer: x in columns [0, A), y in [ycol, ycol + A)."""
    ctx = tuned("")
    A, N = 6, 300
    rng = np.random.default_rng(1200 + S)
    x, y = RR.edge_pairs(rng, N, A)
    for op, fn in OPS:
        host = np.full(N * S + 3, SENT, np.uint64)
        rows = host[:N * S].reshape(N, S)
        rows[:, :A], rows[:, ycol:ycol + A] = x, y
        flat = to_dev(host)
        big = flat[:N * S].view(N, S)
        dx, dy = big[:, :A], big[:, ycol:ycol + A]
        assert pair_plan(A, (dx, dy, dx)) == (vec2, 0)
        assert fn(dx, dy, out=dx, ctx=ctx) is dx
        rows[:, :A] = RR.pair_ref(op, x, y)
        assert np.array_equal(to_host(flat), host), op
    for i in sample_rows(rng, N):  # the last op: intersection
        assert np.array_equal(rows[i, :A], dense(O.VClock.intersection(vc(x[i]), vc(y[i])), A)), i


def test_pair_ops_single_row(tuned):
    ctx = tuned("")
    rng = np.random.default_rng(1300)
    for A in (1, 6, 7, 130):
        x, y = RR.edge_pairs(rng, 16, A)
        for i in range(16):
            dx, dy = to_dev(x[i]), to_dev(y[i])
            a, b = vc(x[i]), vc(y[i])
            g = a.copy()
            g.glb(b)
            exp = {RR.GLB: g, RR.FORGET: a.clone_without(b), RR.INTERSECTION: O.VClock.intersection(a, b)}
            for op, fn in OPS:
                got = to_host(fn(dx, dy, ctx=ctx))
                assert got.shape == (A,) and np.array_equal(got, RR.pair_ref(op, x[i], y[i])), (A, op)
                assert np.array_equal(got, dense(exp[op], A)), (A, op)
            c = cg.causal.partial_cmp(dx, dy, ctx=ctx)
            assert c.dim() == 0 and int(c) == CODE[a.partial_cmp(b)] == int(RR.cmp_ref(x[i], y[i]))
            assert bool(cg.causal.concurrent(dx, dy, ctx=ctx)) == a.concurrent(b)


# ---------------------------------------------------------------------------------------------
# GCounter / PNCounter read
# ---------------------------------------------------------------------------------------------
def read_plan(A, t):
    """causal.hip:302: p.vec2 = (A % 2 == 0) && (stride % 2 == 0) && al16(in); lr_log as above."""
    vec2 = A % 2 == 0 and t.stride(0) % 2 == 0 and al16(t)
    return vec2, row_lr_log(A // 2 if vec2 else A)


@pytest.mark.parametrize("pn,A,pad,off,wrap,vec2,lr_log", [
    pytest.param(0, 6, 0, 0, True, True, 0, id="read-g-16B-lr0-A6-wrap"),
    pytest.param(0, 40, 0, 0, True, True, 2, id="read-g-16B-lr2-A40-wrap"),
    pytest.param(0, 6, 1, 0, True, False, 0, id="read-g-8B-A6-odd-stride-wrap"),
    pytest.param(0, 40, 2, 0, False, True, 2, id="read-g-16B-A40-even-stride"),
    pytest.param(0, 40, 3, 0, False, False, 3, id="read-g-8B-A40-odd-stride"),
    pytest.param(0, 6, 0, 1, False, False, 0, id="read-g-8B-A6-at-8mod16"),
    pytest.param(1, 6, 0, 0, True, True, 0, id="read-pn-16B-A6-wrap"),
    pytest.param(1, 7, 0, 0, True, False, 0, id="read-pn-8B-A7-wrap"),
    pytest.param(1, 40, 2, 0, False, True, 2, id="read-pn-16B-A40-even-stride"),
    pytest.param(1, 40, 1, 0, False, False, 3, id="read-pn-8B-A40-odd-stride"),
    pytest.param(1, 6, 0, 1, False, False, 0, id="read-pn-8B-A6-at-8mod16")])
def test_counter_reads(tuned, pn, A, pad, off, wrap, vec2, lr_log):
    ctx = tuned("rbpc=1" if wrap else "")
    W = 2 * A if pn else A
    one = pass_rows(lr_log)
    N = wrap_rows(one) if wrap else 333
    rng = np.random.default_rng(1400 + 100 * pn + A + 7 * pad + off)
    rows = full_counters(rng, (N, W))
    p = Placed(rows, W + pad, off)
    assert read_plan(A, p.view) == (vec2, lr_log)
    if wrap:
        assert 2 * one < N < 3 * one and N % (64 >> lr_log)
    got = (cg.pncounter if pn else cg.gcounter).read(p.view, ctx=ctx)
    assert got == RR.sum128_ref(rows, pn=bool(pn))
    p.check(rows, "input")
    for i in sample_rows(rng, N, (one, 2 * one) if wrap else ()):
        if pn:
            c = O.PNCounter()
            c.p.inner, c.n.inner = vc(rows[i, :A]), vc(rows[i, A:])
        else:
            c = O.GCounter()
            c.inner = vc(rows[i])
        assert got[i] == c.read(), i


# ---------------------------------------------------------------------------------------------
# cmp_matrix
# ---------------------------------------------------------------------------------------------
def ordered_clocks(rng, N, A):
    """Half the clocks a chain (running pointwise max, so every pair of them is ordered, across the
    sign bit), the rest unrelated, some duplicated; shuffled."""
    x = RR.edge_counters(rng, (N, A), 0.3)
    h = N // 2
    x[:h] = np.maximum.accumulate(RR.edge_counters(rng, (h, A), 0.08), axis=0)
    x[h::5] = x[rng.integers(0, h, size=len(x[h::5]))]
    return x[rng.permutation(N)]


@pytest.mark.parametrize("A", [32, 33, 64])
@pytest.mark.parametrize("N", [64, 65, 128])
def test_cmp_matrix_tile_and_stage_edges(tuned, N, A):
    """kCmpT = 64 clocks per tile side (causal.hip:101), kCmpK = 32 actors per LDS stage (:102)."""
    check_cmp_matrix(tuned(""), N, A, None)


def test_cmp_matrix_strided(tuned):
    check_cmp_matrix(tuned(""), 65, 33, 37)


def check_cmp_matrix(ctx, N, A, stride):
    rng = np.random.default_rng(1500 + N + A)
    x = ordered_clocks(rng, N, A)
    p = Placed(x, stride)
    m = cg.causal.cmp_matrix(p.view, ctx=ctx).cpu().numpy()
    exp = RR.cmp_matrix_ref(x)
    assert set(exp.reshape(-1).tolist()) == {0, 1, -1, 2}
    np.testing.assert_array_equal(m, exp)
    p.check(x, "input")
    for i, j in zip(rng.integers(0, N, 80), rng.integers(0, N, 80)):
        assert m[i, j] == CODE[vc(x[i]).partial_cmp(vc(x[j]))], (i, j)


# ---------------------------------------------------------------------------------------------
# orswot.forget_batch
# ---------------------------------------------------------------------------------------------
def forget_plan(A, x, y, rstride, sstride, pool=False):
    """forget.hip:298-310 launch_forget: p.vec2 = (A % 2 == 0) && (rstride % 2 == 0) && (sstride % 2
    == 0 || ysel) && (ystride % 2 == 0) && al16(x) && al16(y); W = vec2 ? A / 2 : A pieces; W <= 64:
    forget_rows_kernel with the smallest lr_log that holds W and kU rows in flight, else
    forget_wide_rows_kernel with 8-byte pieces and lr_log = 6.  -> (kernel, vec2, rows per pass)."""
    ystride = y.stride(0) if y.dim() == 2 else 0
    vec2 = (A % 2 == 0 and rstride % 2 == 0 and (sstride % 2 == 0 or pool) and ystride % 2 == 0
            and al16(x) and al16(y))
    W = A // 2 if vec2 else A
    if W <= 64:
        return "rows", vec2, pass_rows(fit_lr_log(W), K_U), 64 >> fit_lr_log(W)
    return "wide", False, pass_rows(6), 1


def deferred_pool(rng, D, ys):
    """D rm clocks of random states: a tenth empty, a fifth below their state's y (emptied by the
    forget), and 15% naming no state (left untouched, keep = 1)."""
    N, A = ys.shape
    dc = RR.edge_counters(rng, (D, A), 0.3)
    dc[rng.random(D) < 0.1] = 0
    st = rng.integers(0, N, size=D).astype(np.int64)
    below = rng.random(D) < 0.2
    dc[below] = np.minimum(dc, ys[st])[below]
    none = rng.random(D) < 0.15
    st[none] = rng.choice([N, N + 1, N + 77, (1 << 31) - 1, -1, -(1 << 31)], size=int(none.sum()))
    return dc, st.astype(np.int32)


def check_deferred_sample(rng, dc, st, ys, dc2, keep):
    N, A = ys.shape
    for d in sample_rows(rng, dc.shape[0]):
        s = int(st[d]) & 0xFFFFFFFF
        if s >= N:
            assert np.array_equal(dc2[d], dc[d]) and keep[d] == 1, d
            continue
        o = O.Orswot()
        if dc[d].any():
            o.deferred[vc(dc[d])] = {0}
        o.forget(vc(ys[s]))
        assert bool(keep[d]) == bool(o.deferred), d
        assert np.array_equal(dc2[d], dense(next(iter(o.deferred)), A) if o.deferred else np.zeros(A, np.uint64)), d


@pytest.mark.parametrize("A,pad,shared,yoff,cpad,kernel,vec2", [
    pytest.param(8, 0, False, 0, 0, "rows", True, id="forget_rows-16B-A8-packed"),
    pytest.param(8, 1, False, 0, 1, "rows", False, id="forget_rows-8B-A8-odd-mstride"),
    pytest.param(8, 2, False, 0, 2, "rows", True, id="forget_rows-16B-A8-even-mstride-gaps"),
    pytest.param(7, 0, False, 0, 0, "rows", False, id="forget_rows-8B-A7"),
    pytest.param(8, 0, True, 0, 0, "rows", True, id="forget_rows-16B-A8-shared-y"),
    pytest.param(8, 0, True, 1, 2, "rows", False, id="forget_rows-8B-A8-shared-y-at-8mod16"),
    pytest.param(8, 2, False, 1, 0, "rows", False, id="forget_rows-8B-A8-y-at-8mod16"),
    pytest.param(130, 0, False, 0, 3, "wide", False, id="forget_wide_rows-A130"),
    pytest.param(130, 2, True, 0, 0, "wide", False, id="forget_wide_rows-A130-gaps-shared-y")])
def test_orswot_forget_wraps_the_grid(tuned, A, pad, shared, yoff, cpad, kernel, vec2):
    """Entry rows over states, and a deferred pool, each three trips of an rbpc=1 grid."""
    ctx = tuned("rbpc=1")
    M = 3
    rng = np.random.default_rng(1600 + A + 10 * pad + 100 * shared + yoff)
    mstride = A + pad
    # a first placement fixes the alignment, and with it the plan and the sizes
    probe = Placed(np.zeros((1, M, A), np.uint64), mstride)
    y_probe = Placed(np.zeros((A,) if shared else (2, A), np.uint64), off=yoff)
    kern, v2, one, rpw = forget_plan(A, probe.view, y_probe.view, mstride, M * mstride)
    assert (kern, v2) == (kernel, vec2)
    N = -(-wrap_rows(one) // M)
    assert 2 * one < N * M < 3 * one and (rpw == 1 or (N * M) % rpw)
    clock = RR.edge_counters(rng, (N, A), 0.3)
    entries = RR.edge_counters(rng, (N, M, A), 0.3)
    entries[rng.random((N, M)) < 0.1] = 0
    y = RR.edge_counters(rng, (A,) if shared else (N, A), 0.4)
    ys = np.broadcast_to(y, (N, A))
    below = rng.random((N, M)) < 0.1  # entries that y empties, whatever A
    entries[below] = np.minimum(entries, ys[:, None, :])[below]
    py = Placed(y, off=yoff)
    pc, pe = Placed(clock, A + cpad), Placed(entries, mstride)
    assert forget_plan(A, pe.view, py.view, mstride, M * mstride)[:3] == (kernel, vec2, one)
    # the pool: contiguous (D, A) rows picked by def_state (ysel), sized by its own plan
    pone, prpw = forget_plan(A, probe.flat, py.view, A, A, pool=True)[2:]
    D = wrap_rows(pone)
    assert 2 * pone < D < 3 * pone and (prpw == 1 or D % prpw)
    dc, st = deferred_pool(rng, D, ys)
    tdc, tst = to_dev(dc), torch.from_numpy(st).cuda()
    assert forget_plan(A, tdc, py.view, A, A, pool=True)[2] == pone
    keep = cg.orswot.forget_batch(pc.view, pe.view, py.view, tdc, tst, ctx=ctx)
    c2, e2, dc2, k2 = RR.orswot_forget_ref(clock, entries, y, dc, st)
    pc.check(c2, "clock")
    pe.check(e2, "entries")
    py.check(y, "y")
    assert np.array_equal(to_host(tdc), dc2)
    kp = keep.cpu().numpy()
    assert np.array_equal(kp, k2)
    assert np.array_equal(tst.cpu().numpy(), st)
    none = (st.astype(np.int64) & 0xFFFFFFFF) >= N
    assert none.any() and kp[none].all() and np.array_equal(dc2[none], dc[none])
    assert (kp[~none] == 0).any() and (dc[~none].any(-1) & (kp[~none] == 0)).any()  # some emptied by y
    assert (entries.any(-1) & ~e2.any(-1)).any()  # entries emptied by y
    ge, gc = pe.rows(), pc.rows()
    for s in sorted({i // M for i in sample_rows(rng, N * M, (one, 2 * one))}):
        o = O.Orswot()
        o.clock = vc(clock[s])
        o.entries = {m: vc(entries[s, m]) for m in range(M) if entries[s, m].any()}
        o.forget(vc(ys[s]))
        assert np.array_equal(gc[s], dense(o.clock, A)), s
        for m in range(M):
            exp = o.entries.get(m)
            assert np.array_equal(ge[s, m], dense(exp, A) if exp else np.zeros(A, np.uint64)), (s, m)
    check_deferred_sample(rng, dc, st, ys, to_host(tdc), kp)


# ---------------------------------------------------------------------------------------------
# map.forget_batch
# ---------------------------------------------------------------------------------------------
def map_forget_plan(A, V, ec, vclk, y, mfv2=True, rbpc=0, mfbpc=1):
    """forget.hip:372-384: vec2 = A even, A <= 128, V <= 4, even state strides and y stride, ec / vclk /
    y 16-byte aligned, tune mfv2 != 0 -> map_forget_vec2_kernel (grid capped at CU x (rbpc or mfbpc));
    else A <= 64 && V <= 4 -> map_forget_narrow_kernel; else map_forget_kernel (both CU x (rbpc or 4)).
    lr_log fits W = vec2 ? A / 2 : A pieces; vec2 and narrow keep kU keys in flight.
    -> (kernel, keys per pass, keys per wave)."""
    ystride = y.stride(0) if y.dim() == 2 else 0
    vec2 = (A % 2 == 0 and A <= 128 and V <= 4 and ec.stride(0) % 2 == 0 and vclk.stride(0) % 2 == 0
            and ystride % 2 == 0 and al16(ec) and al16(vclk) and al16(y) and mfv2)
    lr = fit_lr_log(A // 2 if vec2 else A)
    if vec2:
        return "vec2", pass_rows(lr, K_U, rbpc or mfbpc), 64 >> lr
    if A <= 64 and V <= 4:
        return "narrow", pass_rows(lr, K_U, rbpc or 4), 64 >> lr
    return "general", pass_rows(lr, 1, rbpc or 4), 64 >> lr


def map_case(rng, N, K, V, A, shared):
    clock = RR.edge_counters(rng, (N, A), 0.3)
    ec = RR.edge_counters(rng, (N, K, A), 0.3)
    ec[rng.random((N, K)) < 0.1] = 0
    vclk = RR.edge_counters(rng, (N, K, V, A), 0.3)
    vclk[rng.random((N, K, V)) < 0.2] = 0
    vval = (1 + np.arange(N * K * V, dtype=np.uint64)).reshape(N, K, V)  # unique within a register
    y = RR.edge_counters(rng, (A,) if shared else (N, A), 0.4)
    ys = np.broadcast_to(y, (N, A))
    dying = rng.random((N, K)) < 0.25  # the entry clock empties while a value clock would survive
    ec[dying] = np.minimum(ec, ys[:, None, :])[dying]
    assert (dying & (vclk > ys[:, None, None, :]).any(-1).any(-1)).any()
    return clock, ec, vclk, vval, y, ys, dying


MAP_CASES = [
    # A, V, shared y, y offset, tune, kernel
    pytest.param(8, 2, False, 0, "rbpc=1", "vec2", id="map_forget_vec2-A8-rbpc1"),
    pytest.param(8, 2, True, 0, "mfbpc=1", "vec2", id="map_forget_vec2-A8-mfbpc1-shared-y"),
    pytest.param(7, 2, False, 0, "rbpc=1", "narrow", id="map_forget_narrow-A7"),
    pytest.param(8, 2, True, 0, "rbpc=1,mfv2=0", "narrow", id="map_forget_narrow-A8-mfv2off-shared-y"),
    pytest.param(8, 2, True, 1, "rbpc=1", "narrow", id="map_forget_narrow-A8-shared-y-at-8mod16"),
    pytest.param(8, 2, False, 1, "rbpc=1", "narrow", id="map_forget_narrow-A8-y-at-8mod16"),
    # an even A <= 128 with V <= 4 takes the vec2 kernel, so A = 66 reaches map_forget_kernel only
    # with mfv2=0 (66 > 64 rules the narrow kernel out)
    pytest.param(66, 2, False, 0, "rbpc=1,mfv2=0", "general", id="map_forget_kernel-A66-mfv2off"),
    pytest.param(8, 5, True, 0, "rbpc=1", "general", id="map_forget_kernel-A8-V5-shared-y")]


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "small"])
@pytest.mark.parametrize("A,V,shared,yoff,tune,kernel", MAP_CASES)
def test_map_forget_paths(tuned, A, V, shared, yoff, tune, kernel, wrap):
    ctx = tuned(tune if wrap else ",".join(t for t in tune.split(",") if t.startswith("mfv2")))
    K = 3 if wrap else 8
    rng = np.random.default_rng(1700 + A + 10 * V + 100 * shared + yoff + 1000 * wrap)
    if wrap:
        probe = (to_dev(np.zeros((2, K, A), np.uint64)), to_dev(np.zeros((2, K, V, A), np.uint64)))
        yp = Placed(np.zeros((A,) if shared else (2, A), np.uint64), off=yoff)
        kern, one, rpw = map_forget_plan(A, V, probe[0], probe[1], yp.view, "mfv2=0" not in tune,
                                         rbpc=1 if "rbpc=1" in tune else 0)
        N = -(-wrap_rows(one) // K)
        assert 2 * one < N * K < 3 * one and (rpw == 1 or (N * K) % rpw)
    else:
        N = 41
    clock, ec, vclk, vval, y, ys, dying = map_case(rng, N, K, V, A, shared)
    py = Placed(y, off=yoff)
    tc, tec, tvc, tvv = (to_dev(t) for t in (clock, ec, vclk, vval))
    assert map_forget_plan(A, V, tec, tvc, py.view, "mfv2=0" not in tune)[0] == kernel
    dc, st = deferred_pool(rng, 400, ys)
    tdc, tst = to_dev(dc), torch.from_numpy(st).cuda()
    keep = cg.map.forget_batch(tc, tec, tvc, tvv, py.view, def_clock=tdc, def_state=tst, ctx=ctx)
    c2, ec2, vc2, vv2, dc2, k2 = RR.map_forget_ref(clock, ec, vclk, vval, y, dc, st)
    gc, gec, gvc, gvv = to_host(tc), to_host(tec), to_host(tvc), to_host(tvv)
    assert np.array_equal(gec, ec2)
    assert np.array_equal(gvc, vc2)
    assert np.array_equal(gvv, vv2)
    assert np.array_equal(gc, c2)
    py.check(y, "y")
    assert not gvc[dying].any() and not gvv[dying].any()  # a dropped key's values go with it
    assert np.array_equal(to_host(tdc), dc2) and np.array_equal(keep.cpu().numpy(), k2)
    none = (st.astype(np.int64) & 0xFFFFFFFF) >= N
    assert none.any() and k2[none].all() and not k2[~none].all()
    marks = (one, 2 * one) if wrap else ()
    for s in sorted({i // K for i in sample_rows(rng, N * K, marks)}):
        m = O.dense_to_map(clock[s], ec[s], vclk[s], vval[s])
        m.forget(vc(ys[s]))
        got = O.dense_to_map(gc[s], gec[s], gvc[s], gvv[s])
        assert got.clock == m.clock and got.entries == m.entries, s
    check_deferred_sample(rng, dc, st, ys, to_host(tdc), keep.cpu().numpy())
