"""MVReg registers of 17..64 value slots through merge_batch, apply_batch, forget_batch, eq_batch and
lub_many (csrc/mvreg_deep.hip, the 64-slot kernels of mvreg_forget.hip and eq.hip).  Every expected
register, status word and `ne` word comes from O.MVReg (merge / apply / forget / ==); registers are
compared as whole dense arrays, so the Vec order and the zeroing past the values are checked too."""
import numpy as np
import pytest
import torch

import oracle as O
from gpu_util import to_dev, to_host
import mvreg_wide_util as W

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi  # noqa: E402

N = 64
AS = [2, 3, 64, 65, 300]


# ---- merge ------------------------------------------------------------------------------------------
def check_merge(svc, svv, ovc, ovv, exp=None):
    """merge_batch on padded strides against the oracle; returns (status, expected registers)."""
    Vs, A = svc.shape[1], svc.shape[2]
    exp = exp or W.merged(svc, svv, ovc, ovv)
    s_c, s_cw = W.padded(svc, 1)
    s_v, s_vw = W.padded(svv, 3)
    o_c, _ = W.padded(ovc, 2)
    o_v, _ = W.padded(ovv, 1)
    st = cg.mvreg.merge_batch(s_c, s_v, o_c, o_v).cpu().numpy()
    over = np.array([len(r.vals) > Vs for r in exp])
    np.testing.assert_array_equal(st, np.where(over, 16, 0))
    ec, ev = W.dense(exp, A, Vs)
    gc, gv = to_host(s_c.contiguous()), to_host(s_v.contiguous())
    np.testing.assert_array_equal(gc[~over], ec[~over])
    np.testing.assert_array_equal(gv[~over], ev[~over])
    np.testing.assert_array_equal(gc[over], ec[over])  # an overflowed register: the first Vs values
    assert W.padding_intact(s_cw, Vs) and W.padding_intact(s_vw, Vs)
    return st, exp


def test_merge_antichain_two_actors(gpu_ctx):
    """(a) (i + 1, N - i) over two actors: self the even values in 64 slots, other the odd ones in 32."""
    svc, svv = W.dense([O.MVReg(W.antichain(64, 0, 2))], 2, 64)
    ovc, ovv = W.dense([O.MVReg(W.antichain(64, 1, 2))], 2, 32)
    _, exp = check_merge(svc, svv, ovc, ovv)
    assert [v for _, v in exp[0].vals] == [100 + i for i in range(0, 64, 2)] + [100 + i for i in range(1, 64, 2)]


@pytest.mark.parametrize("lo,hi", [(0, 16), (16, 0), (15, 16), (31, 32), (32, 31), (47, 48), (48, 47), (63, 20)])
def test_merge_is_not_chunk_by_chunk(gpu_ctx, lo, hi):
    """(b) other holds a dominated value at slot `lo` and the value dominating it at slot `hi`, in
    different 16-slot chunks.  The reference never compares other's values with each other; merging
    other chunk by chunk does, and gives another register."""
    A, Vo = 3, 64
    svc, svv = W.dense([O.MVReg([(O.VClock({2: 500}), 7)])], A, 64)
    ovc = np.zeros((1, Vo, A), np.uint64)
    ovv = np.zeros((1, Vo), np.uint64)
    for j, s in enumerate(x for x in range(2, Vo, 3) if x not in (lo, hi)):  # concurrent fillers
        ovc[0, s] = (0, j + 1, 400 - j)
        ovv[0, s] = 1000 + s
    ovc[0, lo], ovv[0, lo] = (1, 0, 0), 11
    ovc[0, hi], ovv[0, hi] = (2, 0, 0), 22
    whole = W.merged(svc, svv, ovc, ovv)
    chunked = W.merged(svc, svv, ovc, ovv, chunked=True)
    assert W.vec_lists(whole) != W.vec_lists(chunked)
    assert len(whole[0].vals) == len(chunked[0].vals) + 1
    check_merge(svc, svv, ovc, ovv, exp=whole)


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("Vs,Vo", [(17, 1), (33, 17), (64, 48), (16, 40), (64, 64)])
def test_merge_arbitrary(gpu_ctx, Vs, Vo, A):
    """(c) arbitrary registers with holes; (d) falls out of it wherever the merged register passes Vs."""
    rng = np.random.default_rng(1000 * Vs + 10 * Vo + A)
    svc, svv = W.arbitrary(rng, N, Vs, A, fill=0.5)
    ovc, ovv = W.arbitrary(rng, N, Vo, A, fill=0.6)
    ovv += np.uint64(1 << 50)  # (values of the two sides never collide)
    check_merge(svc, svv, ovc, ovv)


@pytest.mark.parametrize("Vs,Vo", [(17, 64), (40, 33), (16, 64)])
def test_merge_self_too_small(gpu_ctx, Vs, Vo):
    """(d) bit 4 on exactly the registers whose oracle merge has more than Vs values."""
    rng = np.random.default_rng(Vs + Vo)
    regs_s, regs_o = [], []
    for i in range(N):  # antichains of i % 9 + Vs - 4 own and up to Vo incoming values, partly shared
        n = Vs + Vo
        own = W.antichain(n, 0, 1)[:max(1, Vs - 4 + i % 9 - 4)]
        k = int(rng.integers(0, Vo + 1))
        start = int(rng.integers(0, len(own) + 1))
        regs_s.append(O.MVReg(own))
        regs_o.append(O.MVReg(W.antichain(n, 0, 1)[start:start + k]))
    svc, svv = W.dense(regs_s, 2, Vs)
    ovc, ovv = W.dense(regs_o, 2, Vo)
    st, exp = check_merge(svc, svv, ovc, ovv)
    assert 0 < (st == 16).sum() < N and max(len(r.vals) for r in exp) > Vs


@pytest.mark.parametrize("A", [3, 65])
def test_merge_counters_past_2_63(gpu_ctx, A):
    """(e) counters >= 2^63: every compare is unsigned."""
    rng = np.random.default_rng(63 + A)
    svc, svv = W.arbitrary(rng, N, 40, A, fill=0.5, base=2**63)
    ovc, ovv = W.arbitrary(rng, N, 24, A, fill=0.6, base=2**63 - 2)  # straddles the sign bit
    ovv += np.uint64(1 << 50)
    svc[0, :], svv[0, :] = W.dense([O.MVReg(W.antichain(40, 0, 2, base=2**63))], A, 40)
    ovc[0, :], ovv[0, :] = W.dense([O.MVReg(W.antichain(40, 1, 2, base=2**63))], A, 24)
    check_merge(svc, svv, ovc, ovv)


# ---- apply ------------------------------------------------------------------------------------------
def put_streams(rng, regs, V, A):
    """Ragged streams of 0..70 Puts per register, as (clock row, value, malformed) lists: Puts
    dominating half the values, equal to an existing clock, dominated, concurrent (these overflow V),
    with an empty clock, and with an out-of-range clk_row."""
    streams, val = [], 1 << 40
    for i, r0 in enumerate(regs):
        r, ops = r0.copy(), []
        crowd = i % 5 == 0  # this register is pushed past V values
        n_ops = 0 if i % 8 == 7 else (70 if crowd else int(rng.integers(1, 71)))
        for _ in range(n_ops):
            kind = rng.choice(["half", "equal", "below", "new", "empty", "badrow"],
                              p=[0.06, 0.2, 0.15, 0.49, 0.05, 0.05] if not crowd else [0.0, 0.04, 0.04, 0.86, 0.03, 0.03])
            c = O.VClock()
            if kind == "half" and r.vals:
                for vc, _ in r.vals[::2]:
                    c.merge(vc)
            elif kind == "equal" and r.vals:
                c = r.vals[int(rng.integers(len(r.vals)))][0].copy()
            elif kind == "below" and r.vals:
                c = r.vals[int(rng.integers(len(r.vals)))][0].copy()
                a = max(c.dots, key=c.dots.get)
                c.dots[a] -= 1
                c.dots = {k: v for k, v in c.dots.items() if v}
            elif kind == "new" or (kind != "empty" and kind != "badrow"):
                n = len(ops) + 1  # concurrent with every antichain value written before
                c = O.VClock({0: 1000 + n, A - 1: 5000 - n}) if A > 1 else O.VClock({0: 1000 + n})
            val += 1
            bad = kind == "badrow"
            ops.append((c, val, bad))
            if not bad:
                r.apply(O.MVRegPut(c, val))
        streams.append(ops)
    return streams


@pytest.mark.parametrize("A", [3, 65, 300])
@pytest.mark.parametrize("V", [17, 40, 64])
def test_apply_streams(gpu_ctx, V, A):
    rng = np.random.default_rng(17 * V + A)
    vc, vv = W.arbitrary(rng, N, V, A, fill=0.4)
    regs = W.undense(vc, vv)
    streams = put_streams(rng, regs, V, A)
    # the flat op arrays; register 9's range is reversed (op_off[10] < op_off[9]), so register 10 starts early
    pool, clk_row, val, op_off = [np.zeros(A, np.uint64)], [], [], [0]
    for ops in streams:
        for c, v, bad in ops:
            row = np.zeros(A, np.uint64)
            for a, k in c.dots.items():
                row[a] = k
            clk_row.append(-1 if bad else len(pool))
            pool.append(row)
            val.append(v)
        op_off.append(len(val))
    n_rows = len(pool)
    clk_row = np.array([n_rows + 5 if r < 0 else r for r in clk_row], np.int64)
    op_off = np.array(op_off, np.int64)
    assert op_off[9] >= 2
    op_off[10] = op_off[9] - 2
    exp_st = np.zeros(N, np.int32)
    exp = []
    for i, r in enumerate(regs):
        o0, o1 = int(op_off[i]), int(op_off[i + 1])
        r = r.copy()
        if o1 < o0:
            exp_st[i] = 8
        else:
            for o in range(o0, o1):
                if clk_row[o] >= n_rows:
                    exp_st[i] |= 2
                    continue
                r.apply(O.MVRegPut(O._vc_row(pool[clk_row[o]]), int(val[o])))
                if len(r.vals) > V:
                    exp_st[i] |= 16
        exp.append(r)
    assert (exp_st & 16).any() and (exp_st & 2).any() and exp_st[9] == 8 and (exp_st == 0).any()
    ops = cg.mvreg.MVRegOpBatch(torch.from_numpy(op_off).cuda(), torch.from_numpy(clk_row.astype(np.int32)).cuda(),
                                to_dev(np.stack(pool)), to_dev(np.array(val, np.uint64)))
    d_c, d_cw = W.padded(vc, 2)
    d_v, d_vw = W.padded(vv, 1)
    st = cg.mvreg.apply_batch(d_c, d_v, ops).cpu().numpy()
    np.testing.assert_array_equal(st, exp_st)
    ok = (exp_st & 16) == 0
    ec, ev = W.dense(exp, A, V)
    ec[exp_st == 8], ev[exp_st == 8] = vc[exp_st == 8], vv[exp_st == 8]  # untouched, holes and all
    np.testing.assert_array_equal(to_host(d_c.contiguous())[ok], ec[ok])
    np.testing.assert_array_equal(to_host(d_v.contiguous())[ok], ev[ok])
    assert W.padding_intact(d_cw, V) and W.padding_intact(d_vw, V)


def test_apply_equal_clock_moves_last(gpu_ctx):
    """A Put equal to an existing clock removes that value and pushes the new one at the end."""
    vals = W.antichain(40)
    vc, vv = W.dense([O.MVReg(vals)], 2, 40)
    d_c, d_v = to_dev(vc), to_dev(vv)
    ops = cg.mvreg.encode_ops([[({0: 18, 1: 23}, 9999)]], 2, "cuda")  # the clock of value 17
    assert int(cg.mvreg.apply_batch(d_c, d_v, ops).cpu()[0]) == 0
    exp = O.MVReg(vals)
    exp.apply(O.MVRegPut(O.VClock({0: 18, 1: 23}), 9999))
    assert [v for _, v in exp.vals] == [100 + i for i in range(40) if i != 17] + [9999]
    ec, ev = W.dense([exp], 2, 40)
    np.testing.assert_array_equal(to_host(d_c), ec)
    np.testing.assert_array_equal(to_host(d_v), ev)


# ---- forget -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["y_shared", "y_per_register"])
@pytest.mark.parametrize("A", [3, 65, 300, 1024])
@pytest.mark.parametrize("V", [17, 33, 64])
def test_forget(gpu_ctx, V, A, shared):
    rng = np.random.default_rng(V * 2000 + A + int(shared))
    n = 24 if A == 1024 else N
    vc = np.zeros((n, V, A), np.uint64)
    acts = W.actors_of(rng, A, 3)
    vc[:, :, acts] = rng.integers(0, 6, size=(n, V, len(acts)))
    vc[rng.random((n, V)) < 0.2] = 0  # holes in the input
    y = np.zeros((n, A), np.uint64)
    y[:, acts] = rng.integers(0, 4, size=(1 if shared else n, len(acts)))
    emptied = [s for s in (0, 16, 31, 32, 63) if s < V]
    vc[:, emptied] = 0
    vc[:, emptied, acts[-1]] = 1  # a value the forget empties: its one counter is within y
    y[:, acts[-1]] = np.maximum(y[:, acts[-1]], 1)
    vv = rng.integers(1, 2**63, size=(n, V)).astype(np.uint64)
    vv[~vc.any(axis=2)] = 0
    exp = W.undense(vc, vv)
    for i, r in enumerate(exp):
        r.forget(O._vc_row(y[i]))
    assert min(len(r.vals) for r in exp) < max(len(r.vals) for r in exp) <= V - len(emptied)
    d_c, d_cw = W.padded(vc, 1)
    d_v, d_vw = W.padded(vv, 2)
    st = cg.mvreg.forget_batch(d_c, d_v, to_dev(y[0] if shared else y))
    assert not st.cpu().numpy().any()
    ec, ev = W.dense(exp, A, V)
    np.testing.assert_array_equal(to_host(d_c.contiguous()), ec)
    np.testing.assert_array_equal(to_host(d_v.contiguous()), ev)
    assert W.padding_intact(d_cw, V) and W.padding_intact(d_vw, V)


# ---- == ---------------------------------------------------------------------------------------------
EQ_CLASSES = ["identical", "permuted", "payload_last_slot", "clock_word_slot_32", "extra_value", "holes", "empty"]


def eq_pairs(rng, n, Vx, Vy, A):
    """x, y dense registers derived from one list of distinct values per pair, by EQ_CLASSES in turn."""
    xc, xv = np.zeros((n, Vx, A), np.uint64), np.zeros((n, Vx), np.uint64)
    yc, yv = np.zeros((n, Vy, A), np.uint64), np.zeros((n, Vy), np.uint64)
    Vmin = min(Vx, Vy)
    wide_y = Vy >= Vx  # the side with the slots 32 / 63 where there is one
    for i in range(n):
        cls = EQ_CLASSES[i % len(EQ_CLASSES)]
        full = i % 2 == 0
        k = 0 if cls == "empty" else (Vmin - (1 if cls == "extra_value" and Vx == Vy else 0) if full
                                      else int(rng.integers(1, Vmin + 1)))
        k = max(k, 1) if cls != "empty" else 0
        rows = np.zeros((k, A), np.uint64)
        for j in range(k):
            rows[j, (j + i) % A] = j + 1
            rows[j, (7 * j + 1) % A] += 200 - j
        rows[:1, A - 1] += 3
        pay = rng.integers(1, 2**63, size=k).astype(np.uint64)
        sx, sy = np.arange(k), np.arange(k)
        if cls in ("permuted", "holes"):
            sy = rng.choice(Vy, size=k, replace=False)
        if cls == "holes":
            sx = np.sort(rng.choice(Vx, size=k, replace=False))
        big_c, big_v, big_s, V_big = (yc, yv, sy, Vy) if wide_y else (xc, xv, sx, Vx)
        if cls == "payload_last_slot" and k:
            big_s[-1] = V_big - 1  # the last value sits in the last slot of the wide side
        if cls == "clock_word_slot_32" and k:
            big_s[-1] = min(32, V_big - 1)
        xc[i, sx], xv[i, sx] = rows, pay
        yc[i, sy], yv[i, sy] = rows, pay
        if cls == "payload_last_slot" and k:
            big_v[i, V_big - 1] ^= np.uint64(1 << 40)
        if cls == "clock_word_slot_32" and k:
            big_c[i, min(32, V_big - 1), A - 1] += np.uint64(1)
        if cls == "extra_value":
            free = np.flatnonzero(~big_c[i].any(axis=1))
            big_c[i, free[-1], 0] = 777
            big_v[i, free[-1]] = 5
    return xc, xv, yc, yv


@pytest.mark.parametrize("A", [3, 65, 300, 1024])
@pytest.mark.parametrize("Vx,Vy", [(64, 64), (17, 64), (64, 3)])
def test_eq(gpu_ctx, Vx, Vy, A):
    rng = np.random.default_rng(Vx * 100 + Vy + A)
    n = 28 if A == 1024 else 56
    xc, xv, yc, yv = eq_pairs(rng, n, Vx, Vy, A)
    exp = np.array([0 if a == b else 4 for a, b in zip(W.undense(xc, xv), W.undense(yc, yv))], np.int32)
    for j, cls in enumerate(EQ_CLASSES):
        want_ne = cls in ("payload_last_slot", "clock_word_slot_32", "extra_value")
        assert (exp[j::len(EQ_CLASSES)] != 0).all() == want_ne and (exp[j::len(EQ_CLASSES)] != 0).any() == want_ne, cls
    d_xc, _ = W.padded(xc, 1)
    d_xv, _ = W.padded(xv, 2)
    ne = cg.mvreg.eq_batch(d_xc, d_xv, to_dev(yc), to_dev(yv)).cpu().numpy()
    np.testing.assert_array_equal(ne, exp)
    ne = cg.mvreg.eq_batch(to_dev(yc), to_dev(yv), d_xc, d_xv).cpu().numpy()  # the sides swapped
    np.testing.assert_array_equal(ne, exp)


# ---- lub_many ---------------------------------------------------------------------------------------
def fold(vclk, vval):
    acc = O.MVReg()
    for r in W.undense(vclk, vval):
        acc.merge(r)
    return acc


@pytest.mark.parametrize("A", [2, 65])
def test_lub_many_wide_input(gpu_ctx, A):
    """G = 3 folds of R = 4 replicas of 24 slots: an antichain group, an arbitrary group and a mixed one."""
    G, R, V = 3, 4, 24
    rng = np.random.default_rng(A)
    vc, vv = W.arbitrary(rng, G * R, V, A, fill=0.7)
    vv += (np.arange(G * R, dtype=np.uint64) << np.uint64(52))[:, None] * (vv != 0)
    anti = W.antichain(64)
    for r in range(R):  # group 0: 64 pairwise concurrent values, 16 a replica, in scattered order
        vc[r], vv[r] = (x[0] for x in W.dense([O.MVReg(anti[r::4])], A, V))
    vc[2 * R], vv[2 * R] = (x[0] for x in W.dense([O.MVReg(W.antichain(40, 0, 2, base=10))], A, V))
    vc, vv = vc.reshape(G, R, V, A), vv.reshape(G, R, V)
    exp = [fold(vc[g], vv[g]) for g in range(G)]
    assert len(exp[0].vals) == 64 and len(exp[2].vals) > 16 and all(len(e.vals) <= 64 for e in exp)
    res = cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=64, vstate=64)
    assert not res.flags.cpu().numpy().any()
    np.testing.assert_array_equal(res.nval.cpu().numpy(), [len(e.vals) for e in exp])
    ec, ev = W.dense(exp, A, 64)
    np.testing.assert_array_equal(to_host(res.vclk), ec)
    np.testing.assert_array_equal(to_host(res.vval), ev)
    # a fold's own output folds again: 64-slot registers as input
    again = cg.mvreg.lub_many(res.vclk.unsqueeze(1), res.vval.unsqueeze(1), vout=64, vstate=64)
    np.testing.assert_array_equal(to_host(again.vclk), ec)
    np.testing.assert_array_equal(to_host(again.vval), ev)


def test_lub_many_wide_input_needs_vstate(gpu_ctx):
    vc, vv = W.dense([O.MVReg(W.antichain(24))], 2, 24)
    with pytest.raises(_abi.CrdtGpuError) as ei:
        cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=16, vstate=0)
    assert ei.value.code == _abi.CRDT_EUNSUPPORTED


# ---- refusals ---------------------------------------------------------------------------------------
def test_v65_is_refused(gpu_ctx):
    vc, vv = W.dense([O.MVReg(W.antichain(8))], 2, 65)
    small = W.dense([O.MVReg(W.antichain(8))], 2, 4)
    y = to_dev(np.zeros(2, np.uint64))
    ops = cg.mvreg.encode_ops([[({0: 1}, 1)]], 2, "cuda")
    calls = [lambda: cg.mvreg.merge_batch(to_dev(vc), to_dev(vv), to_dev(small[0]), to_dev(small[1])),
             lambda: cg.mvreg.merge_batch(to_dev(small[0]), to_dev(small[1]), to_dev(vc), to_dev(vv)),
             lambda: cg.mvreg.apply_batch(to_dev(vc), to_dev(vv), ops),
             lambda: cg.mvreg.forget_batch(to_dev(vc), to_dev(vv), y),
             lambda: cg.mvreg.eq_batch(to_dev(vc), to_dev(vv), to_dev(small[0]), to_dev(small[1])),
             lambda: cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=64, vstate=64)]
    for call in calls:
        with pytest.raises(_abi.CrdtGpuError) as ei:
            call()
        assert ei.value.code == _abi.CRDT_EUNSUPPORTED


def test_lds_bound_at_64_values_of_1024_actors(gpu_ctx):
    """merge and apply keep the register in LDS: 64 values of 1,024 actors do not fit and are refused
    with the byte count; forget and == keep no state and take the shape."""
    A, V, n = 1024, 64, 4
    rng = np.random.default_rng(5)
    vc, vv = W.arbitrary(rng, n, V, A)
    lds = (V * A + 3 * V) * 8
    ops = cg.mvreg.encode_ops([[({0: 1}, 1)]] * n, A, "cuda")
    for call in (lambda: cg.mvreg.merge_batch(to_dev(vc), to_dev(vv), to_dev(vc[:, :4]), to_dev(vv[:, :4])),
                 lambda: cg.mvreg.apply_batch(to_dev(vc), to_dev(vv), ops)):
        with pytest.raises(_abi.CrdtGpuError) as ei:
            call()
        assert ei.value.code == _abi.CRDT_EUNSUPPORTED
        assert "LDS" in str(ei.value) and any(str(b) in str(ei.value) for b in (lds, lds + 4 * 33 * 8))
    y = np.full(A, 2, np.uint64)
    exp = W.undense(vc, vv)
    for r in exp:
        r.forget(O._vc_row(y))
    d_c, d_v = to_dev(vc), to_dev(vv)
    cg.mvreg.forget_batch(d_c, d_v, to_dev(y))
    ec, ev = W.dense(exp, A, V)
    np.testing.assert_array_equal(to_host(d_c), ec)
    np.testing.assert_array_equal(to_host(d_v), ev)
    yc, yv = vc[:, ::-1].copy(), vv[:, ::-1].copy()  # the slots reversed; pair 1: one payload differs
    yv[1, np.flatnonzero(yc[1].any(axis=1))[0]] ^= np.uint64(1)
    want = [0 if a == b else 4 for a, b in zip(W.undense(vc, vv), W.undense(yc, yv))]
    assert want == [0, 4, 0, 0]
    np.testing.assert_array_equal(cg.mvreg.eq_batch(to_dev(vc), to_dev(vv), to_dev(yc), to_dev(yv)).cpu().numpy(), want)
