"""crdt_mvreg_forget_batch (csrc/mvreg_forget.hip) against the oracle's MVReg.forget (mvreg.rs:88-104):
N = 257 registers built by op replay as test/mvreg.rs:130-140 builds them, compared register by
register, on every kernel path (sub-wave segments of 2 .. 64 lanes, two chunks per lane, and the
workgroup path for V > 8 or A > 256), with a shared and a per-register y."""
import numpy as np
import pytest
import torch

import oracle as O
import wire_mvreg_util as W
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

N = 257
SHAPES = [(3, 1), (32, 4), (64, 8), (65, 16), (300, 4)]  # (A, V): narrow x3, V > 8, A > 256
_CACHE = {}


def regs_for(A, V):
    """The shape's registers (built once, never changed): (objects, vclk, vval)."""
    if (A, V) not in _CACHE:
        rng = np.random.default_rng(1000 * A + V)
        regs = [W.replay(rng, A, min(A, 6), V, int(rng.integers(0, 3 * V + 2)))[0] for _ in range(N)]
        # one register with every slot taken (V concurrent writers), one empty
        regs[7] = O.MVReg([(O.VClock({k: k + 1, (k + 1) % A: 1} if A > 1 else {k: k + 1}), 1000 + k) for k in range(V)])
        regs[8] = O.MVReg()
        assert max(len(r.vals) for r in regs) == V and min(len(r.vals) for r in regs) == 0
        vc, vv = W.dense(regs, A, V)
        vc.setflags(write=False)
        vv.setflags(write=False)
        _CACHE[(A, V)] = (regs, vc, vv)
    return _CACHE[(A, V)]


def rand_y(rng, regs, A, n):
    """n clocks that forget some dots of the registers, all of some values and none of others."""
    y = np.zeros((n, A), np.uint64)
    for i in range(n):
        r = regs[i % len(regs)]
        mode = rng.integers(4)
        if mode == 0 or not r.vals:
            y[i] = rng.integers(0, 4, size=A)
        else:
            c = r.vals[int(rng.integers(len(r.vals)))][0]
            for a, k in c.dots.items():
                y[i, a] = k if mode < 3 else k - 1
            if mode == 2:
                y[i] = np.maximum(y[i], rng.integers(0, 3, size=A).astype(np.uint64))
    return y


def oracle_forget(regs, y):
    out = []
    for i, r in enumerate(regs):
        row = y if y.ndim == 1 else y[i]
        r = r.copy()
        r.forget(O.VClock({int(a): int(row[a]) for a in np.flatnonzero(row)}))
        out.append(r)
    return out


def check_layout(vc, vv, want):
    """Survivors from slot 0 in Vec order, every slot past them zero (clock and value)."""
    V = vc.shape[1]
    evc, evv = W.dense(want, vc.shape[2], V)
    assert np.array_equal(vc, evc) and np.array_equal(vv, evv)


@pytest.mark.parametrize("per_reg", [False, True], ids=["shared_y", "per_register_y"])
@pytest.mark.parametrize("A,V", SHAPES)
def test_forget_vs_oracle(gpu_ctx, A, V, per_reg):
    regs, vc, vv = regs_for(A, V)
    rng = np.random.default_rng(7 * A + V + per_reg)
    if per_reg:
        y = rand_y(rng, regs, A, N)
    else:  # one clock for all: a value of the full register, over a low random floor
        y = rng.integers(0, 3, size=A).astype(np.uint64)
        for a, k in regs[7].vals[V // 2][0].dots.items():
            y[a] = max(int(y[a]), k)
    d_c, d_v = to_dev(vc.copy()), to_dev(vv.copy())
    st = cg.mvreg.forget_batch(d_c, d_v, to_dev(y))
    want = oracle_forget(regs, y)
    assert any(len(w.vals) < len(r.vals) for w, r in zip(want, regs)), "the y must drop some value"
    check_layout(to_host(d_c), to_host(d_v), want)
    assert not st.cpu().numpy().any() and st.shape == (N,)


@pytest.mark.parametrize("A,V", SHAPES)
def test_prop_forget(gpu_ctx, A, V):
    """test/mvreg.rs:211-224: forgetting the zero clock changes nothing (bit for bit); forgetting the
    register's own read().add_clock empties it."""
    regs, vc, vv = regs_for(A, V)
    d_c, d_v = to_dev(vc.copy()), to_dev(vv.copy())
    cg.mvreg.forget_batch(d_c, d_v, torch.zeros(A, dtype=torch.int64, device="cuda:0"))
    assert np.array_equal(to_host(d_c), vc) and np.array_equal(to_host(d_v), vv)
    rd = cg.mvreg.read(d_c, d_v)
    clk = to_host(rd.add_clock)
    for i in (0, 100, N - 1):
        c = regs[i].read().add_clock
        assert {int(a): int(clk[i, a]) for a in np.flatnonzero(clk[i])} == c.dots
    cg.mvreg.forget_batch(d_c, d_v, rd.add_clock)
    assert not to_host(d_c).any() and not to_host(d_v).any()


@pytest.mark.parametrize("A,V", [(3, 4), (32, 4), (200, 8), (65, 16), (300, 4)])
def test_middle_value_dropped_and_holes_closed(gpu_ctx, A, V):
    """Three concurrent values, y empties only the middle one: the survivors sit in slots 0 and 1 in
    their order and slot 2 is zero.  The same with the register laid out around holes (an empty slot
    before, between and after the values), and with a nonzero value in an empty slot."""
    a, b, c = 0, 1, A - 1
    reg = O.MVReg([(O.VClock({a: 5, b: 1}), 11), (O.VClock({b: 3}), 22), (O.VClock({c: 7, b: 2}), 33)])
    y = np.zeros(A, np.uint64)
    y[b] = 3
    packed_c, packed_v = W.dense([reg], A, V)
    lay = [(0, 1, 2)] + ([(1, 2, 3), (0, 2, 3), (0, 1, 3)] if V >= 4 else [])
    n = len(lay) + 1
    vc, vv = np.zeros((n, V, A), np.uint64), np.zeros((n, V), np.uint64)
    for i, slots in enumerate(lay):
        for s, src in zip(slots, range(3)):
            vc[i, s], vv[i, s] = packed_c[0, src], packed_v[0, src]
    if V >= 4:
        vv[2, 1] = 99  # an empty slot's value is not a value
    vc[n - 1, 0], vv[n - 1, 0] = packed_c[0, 1], 22  # the last register holds the middle value alone
    d_c, d_v = to_dev(vc.copy()), to_dev(vv.copy())
    cg.mvreg.forget_batch(d_c, d_v, to_dev(y))
    g_c, g_v = to_host(d_c), to_host(d_v)
    for i in range(len(lay)):
        assert g_c[i, 0, a] == 5 and g_c[i, 0, b] == 0 and g_c[i, 0].sum() == 5 and g_v[i, 0] == 11
        assert g_c[i, 1, c] == 7 and g_c[i, 1].sum() == 7 and g_v[i, 1] == 33
        assert not g_c[i, 2:].any() and not g_v[i, 2:].any()
    assert not g_c[n - 1].any() and not g_v[n - 1].any()
    # holes alone (nothing forgotten) are closed too, order kept
    d_c, d_v = to_dev(vc.copy()), to_dev(vv.copy())
    cg.mvreg.forget_batch(d_c, d_v, to_dev(np.zeros(A, np.uint64)))
    g_c, g_v = to_host(d_c), to_host(d_v)
    for i in range(len(lay)):
        assert np.array_equal(g_c[i], packed_c[0]) and np.array_equal(g_v[i], packed_v[0])


@pytest.mark.parametrize("A,V", [(3, 2), (32, 4), (65, 16), (300, 4)])
def test_unsigned_compare_over_the_full_range(gpu_ctx, A, V):
    """Counters at 2^63 and 2^64 - 1 against y just below and at them."""
    hi, top = 1 << 63, (1 << 64) - 1
    cases = [(hi, hi - 1, True), (hi, hi, False), (hi, top, False), (top, top - 1, True), (top, top, False),
             (top, hi, True), (hi - 1, hi, False), (1, top, False), (hi + 1, hi, True)]
    n = len(cases)
    vc, vv = np.zeros((n, V, A), np.uint64), np.zeros((n, V), np.uint64)
    y = np.zeros((n, A), np.uint64)
    col = A - 1
    for i, (cnt, yy, _) in enumerate(cases):
        vc[i, 0, col], vv[i, 0], y[i, col] = cnt, 100 + i, yy
        vc[i, V - 1, 0], vv[i, V - 1] = 9, 7  # a second value that always survives (y[0] = 0)
    d_c, d_v = to_dev(vc.copy()), to_dev(vv.copy())
    cg.mvreg.forget_batch(d_c, d_v, to_dev(y))
    g_c, g_v = to_host(d_c), to_host(d_v)
    for i, (cnt, yy, keep) in enumerate(cases):
        want = O.MVReg([(O.VClock({col: cnt}), 100 + i), (O.VClock({0: 9}), 7)])
        want.forget(O.VClock({col: yy}))
        assert len(want.vals) == (2 if keep else 1)
        e_c, e_v = W.dense([want], A, V)
        assert np.array_equal(g_c[i], e_c[0]) and np.array_equal(g_v[i], e_v[0]), (cnt, yy)


@pytest.mark.parametrize("A,V,pad", [(32, 4, 6), (7, 3, 5), (65, 16, 3), (300, 4, 2)])
def test_strided_states_leave_the_padding_alone(gpu_ctx, A, V, pad):
    """vclk_stride > V*A (and an odd stride / odd A: the 8-byte path): the padding words are untouched."""
    rng = np.random.default_rng(A)
    n = 67
    regs = [W.replay(rng, A, min(A, 5), V, int(rng.integers(1, 2 * V + 2)))[0] for _ in range(n)]
    vc, vv = W.dense(regs, A, V)
    big_c = np.full((n, V * A + pad), 0xABCDEF, np.uint64)
    big_v = np.full((n, V + pad), 0x123456, np.uint64)
    big_c[:, :V * A] = vc.reshape(n, V * A)
    big_v[:, :V] = vv
    y = rand_y(rng, regs, A, n)
    d_c, d_v = to_dev(big_c), to_dev(big_v)
    view_c = d_c[:, :V * A].unflatten(1, (V, A))
    assert view_c.stride(0) == V * A + pad and view_c.data_ptr() == d_c.data_ptr()
    cg.mvreg.forget_batch(view_c, d_v[:, :V], to_dev(y))
    g_c, g_v = to_host(d_c), to_host(d_v)
    assert (g_c[:, V * A:] == 0xABCDEF).all() and (g_v[:, V:] == 0x123456).all()
    check_layout(g_c[:, :V * A].reshape(n, V, A), g_v[:, :V], oracle_forget(regs, y))


def test_no_registers_is_ok(gpu_ctx):
    e = lambda *s: torch.zeros(s, dtype=torch.int64, device="cuda:0")  # noqa: E731
    st = cg.mvreg.forget_batch(e(0, 4, 8), e(0, 4), e(8))
    assert st.shape == (0,)
    st = cg.mvreg.forget_batch(e(0, 4, 8), e(0, 4), e(0, 8))
    assert st.shape == (0,)
