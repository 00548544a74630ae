"""The standalone MVReg wire forms on the device (csrc/wire_mvreg.hip) against the oracle and the
test-side codec (tests/wire_mvreg_util.py): register frames (crdt_mvreg_ingest / _egress) and
Vec<Op::Put> frames (crdt_mvreg_ops_ingest / _ops_egress), N = 200 registers (a batch crosses the
64-frame and 64-op groupings) through sparse actor dictionaries; the refusals, each with its
neighbours' results intact; and one frame -> ops -> apply -> forget -> frame -> merge loop."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import oracle as O
import wire_mvreg_util as W
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, wire  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

N = 200
SHAPES = [(3, 1), (64, 4), (200, 16)]  # A = 200: clocks of more than 64 records
BAD, MISSING, CAP, EMPTY = 1, 2, 4, 8
_CACHE = {}


def dev_frames(frames):
    data, off = W.pack_frames(frames)
    return torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")


def dev_dict(aid):
    return torch.from_numpy(np.asarray(aid, np.uint32).view(np.int32).copy()).to("cuda:0")


def batch_for(A, V):
    """The shape's registers, the Put streams that built them and the dictionary (built once)."""
    if (A, V) not in _CACHE:
        rng = np.random.default_rng(77 * A + V)
        aid = W.sparse_dict(rng, A, 32)
        counts = [int(x) for x in rng.integers(0, 71, size=N)]
        counts[0], counts[1], counts[2], counts[3], counts[N - 1] = 0, 64, 70, 65, 0
        regs, streams = [], []
        for n in counts:
            r, ops = W.replay(rng, A, min(A, 6), V, n, wide=0.15)
            assert len(ops) == n
            regs.append(r)
            streams.append(ops)
        # register 4: V concurrent writers, every slot taken
        streams[4] = [O.MVRegPut(O.VClock({k: k + 1}), 500 + k) for k in range(V)]
        regs[4] = O.MVReg([(op.clock, op.val) for op in streams[4]])
        if A > 64:
            assert any(len(c.dots) > 64 for r in regs for c, _ in r.vals)
            assert any(len(op.clock.dots) > 64 for s in streams for op in s)
        assert max(len(r.vals) for r in regs) == V
        _CACHE[(A, V)] = (aid, regs, streams)
    return _CACHE[(A, V)]


def tuples(streams):
    return [[(dict(op.clock.dots), op.val) for op in s] for s in streams]


def same_batch(got, want, n_ops):
    assert np.array_equal(got.op_off.cpu().numpy(), want.op_off.cpu().numpy())
    assert np.array_equal(got.clk_row.cpu().numpy()[:n_ops], np.arange(n_ops))
    assert np.array_equal(to_host(got.clk_pool)[:n_ops], to_host(want.clk_pool)[:n_ops])
    assert np.array_equal(to_host(got.val)[:n_ops], to_host(want.val)[:n_ops])


# ---- states -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,V", SHAPES)
def test_states_ingest_egress_round_trip(gpu_ctx, A, V):
    aid, regs, _ = batch_for(A, V)
    frames = [W.enc_reg(r, aid) for r in regs]
    data, off = dev_frames(frames)
    actors = dev_dict(aid)
    vclk, vval, st = wire.mvreg_ingest(data, off, actors, V)
    assert not st.cpu().numpy().any()
    e_c, e_v = W.dense(regs, A, V)
    assert np.array_equal(to_host(vclk), e_c) and np.array_equal(to_host(vval), e_v)
    # egress of the dense form: decodes to the registers, and is the encoder's bytes
    f_off, out = wire.mvreg_egress(to_dev(e_c), to_dev(e_v), actors)
    assert np.array_equal(f_off.cpu().numpy(), off.cpu().numpy())
    got = W.split(out.cpu().numpy(), f_off.cpu().numpy())
    assert [W.dec_reg(b, aid).vals for b in got] == [r.vals for r in regs]
    # ingest -> egress is byte-identical
    f_off2, out2 = wire.mvreg_egress(vclk, vval, actors)
    assert bytes(out2.cpu().numpy()) == b"".join(frames) and np.array_equal(f_off2.cpu().numpy(), off.cpu().numpy())


def test_states_sizing_call_and_short_buffer(gpu_ctx):
    A, V = 64, 4
    aid, regs, _ = batch_for(A, V)
    e_c, e_v = W.dense(regs, A, V)
    d_c, d_v, actors = to_dev(e_c), to_dev(e_v), dev_dict(aid)
    st = _abi.MVRegStates(N, A, V, d_c.data_ptr(), V * A, d_v.data_ptr(), V)
    f_off = torch.zeros(N + 1, dtype=torch.int64, device="cuda:0")
    total = ctypes.c_size_t(12345)
    gpu_ctx.call("crdt_mvreg_egress", ctypes.byref(st), dptr(actors), dptr(f_off), None, 0, ctypes.byref(total))
    want = sum(len(W.enc_reg(r, aid)) for r in regs)
    assert total.value == want and int(f_off.cpu()[-1]) == want
    # a buffer one byte short: the total again, nothing written
    buf = torch.full((want,), 0x5A, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.call("crdt_mvreg_egress", ctypes.byref(st), dptr(actors), dptr(f_off), dptr(buf), want - 1, ctypes.byref(total))
    torch.cuda.synchronize()
    assert total.value == want and bool((buf == 0x5A).all())
    # N = 0
    st0 = _abi.MVRegStates(0, A, V, None, V * A, None, V)
    gpu_ctx.call("crdt_mvreg_egress", ctypes.byref(st0), dptr(actors), dptr(f_off), None, 0, ctypes.byref(total))
    assert total.value == 0


@pytest.mark.parametrize("A,V", SHAPES)
def test_states_agree_with_the_map_path(gpu_ctx, A, V):
    """Each register wrapped in a one-key Map frame and read by crdt_map_ingest fills the same value
    slots (no register here has an empty-clock value)."""
    aid, regs, _ = batch_for(A, V)
    key = 0x1234
    frames = []
    for r in regs:
        vals = [({aid[a]: k for a, k in c.dots.items()}, v) for c, v in r.vals]
        ec = {aid[a]: k for a, k in r.clock().dots.items()}
        frames.append(O.bc_map(ec, {key: (ec, vals)} if vals else {}, []))
    data, off = dev_frames(frames)
    actors = dev_dict(aid)
    ms, st = wire.map_ingest(data, off, actors, torch.tensor([key], dtype=torch.int32, device="cuda:0"), V, 1)
    assert not st.cpu().numpy().any()
    vclk, vval, st2 = wire.mvreg_ingest(*dev_frames([W.enc_reg(r, aid) for r in regs]), actors, V)
    assert not st2.cpu().numpy().any()
    assert np.array_equal(to_host(ms.vclk)[:, 0], to_host(vclk)) and np.array_equal(to_host(ms.vval)[:, 0], to_host(vval))


def test_state_refusals_leave_neighbours_intact(gpu_ctx):
    A, V = 5, 2
    rng = np.random.default_rng(5)
    aid = W.sparse_dict(rng, A, 32)
    unknown = aid[1] + 1
    assert unknown not in aid
    bad_aid = list(aid)
    bad_aid[1] = unknown
    R = O.MVReg
    C = O.VClock
    g = R([(C({0: 2, 1: 1}), 5), (C({2: 4}), 6)])
    gb = W.enc_reg(g, aid)
    cases = [  # (frame bytes, status, the register ingest must write)
        (gb, 0, g),
        (gb[:-4], BAD, R()),                                                    # truncated
        (gb, 0, g),
        (gb + bytes(4), BAD, R()),                                              # trailing bytes
        (gb, 0, g),
        (struct.pack("<Q", 1 << 61) + gb[8:], BAD, R()),                        # a value count that cannot fit
        (gb[:8] + struct.pack("<Q", 1 << 61) + gb[16:], BAD, R()),              # a record count that cannot fit
        (gb, 0, g),
        (W.enc_reg(g, bad_aid), MISSING, R([(C({0: 2}), 5), (C({2: 4}), 6)])),  # unknown actor: record skipped
        (W.enc_reg(R([(C({0: 1}), 1), (C({1: 1}), 2), (C({2: 1}), 3)]), aid), CAP, R([(C({0: 1}), 1), (C({1: 1}), 2)])),
        (W.enc_reg(R([(C(), 9), (C({2: 4}), 6)]), aid), EMPTY, R([(C({2: 4}), 6)])),  # empty clock on the wire
        (W.enc_reg(R([(C({1: 1}), 7), (C({0: 3}), 8)]), bad_aid), MISSING | EMPTY, R([(C({0: 3}), 8)])),
        (b"", BAD, R()),
        (W.enc_reg(R(), aid), 0, R()),
        (gb, 0, g),
    ]
    data, off = dev_frames([c[0] for c in cases])
    vclk, vval, st = wire.mvreg_ingest(data, off, dev_dict(aid), V)
    assert st.cpu().numpy().tolist() == [c[1] for c in cases]
    e_c, e_v = W.dense([c[2] for c in cases], A, V)
    assert np.array_equal(to_host(vclk), e_c) and np.array_equal(to_host(vval), e_v)
    # a misaligned offset: frame 1 ends and frame 2 starts 2 bytes off; frames 0 and 3 are whole
    raw = gb + gb + bytes(2) + gb + bytes(2) + gb
    L = len(gb)
    off = torch.tensor([0, L, 2 * L + 2, 3 * L + 4, 4 * L + 4], dtype=torch.int64, device="cuda:0")
    vclk, vval, st = wire.mvreg_ingest(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to("cuda:0"), off,
                                       dev_dict(aid), V)
    assert st.cpu().numpy().tolist() == [0, BAD, BAD, 0]
    e_c, e_v = W.dense([g, R(), R(), g], A, V)
    assert np.array_equal(to_host(vclk), e_c) and np.array_equal(to_host(vval), e_v)


# ---- Put streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,V", SHAPES)
def test_ops_ingest_apply_egress(gpu_ctx, A, V):
    aid, regs, streams = batch_for(A, V)
    frames = [W.enc_ops(s, aid) for s in streams]
    data, off = dev_frames(frames)
    actors = dev_dict(aid)
    n_ops = sum(len(s) for s in streams)
    res = wire.mvreg_ops_ingest(data, off, actors)
    assert res.totals == (n_ops, n_ops) and not res.status.cpu().numpy().any()
    want = cg.mvreg.encode_ops(tuples(streams), A, "cuda:0")
    same_batch(res.ops, want, n_ops)
    # the filled buffer goes to apply_batch as is
    vc = torch.zeros((N, V, A), dtype=torch.int64, device="cuda:0")
    vv = torch.zeros((N, V), dtype=torch.int64, device="cuda:0")
    ast = cg.mvreg.apply_batch(vc, vv, res.ops)
    assert not ast.cpu().numpy().any()
    e_c, e_v = W.dense(regs, A, V)
    assert np.array_equal(to_host(vc), e_c) and np.array_equal(to_host(vv), e_v)
    # egress: decodes to the ops; ingest -> egress is byte-identical
    f_off, out, est = wire.mvreg_ops_egress(res.ops, actors)
    assert not est.cpu().numpy().any() and np.array_equal(f_off.cpu().numpy(), off.cpu().numpy())
    got = W.split(out.cpu().numpy(), f_off.cpu().numpy())
    assert got == frames
    assert [W.dec_ops(b, aid) for b in got[:4]] == streams[:4]
    # no sync, with room: the same batch
    res2 = wire.mvreg_ops_ingest(data, off, actors, sync=False, caps=(n_ops + 9, n_ops + 3))
    assert res2.totals is None and not res2.status.cpu().numpy().any()
    same_batch(res2.ops, want, n_ops)


@pytest.mark.parametrize("which", ["ops", "rows"])
def test_ops_capacity_cuts_a_suffix(gpu_ctx, which):
    A, V = 64, 4
    aid, _, streams = batch_for(A, V)
    data, off = dev_frames([W.enc_ops(s, aid) for s in streams])
    actors = dev_dict(aid)
    n_ops = sum(len(s) for s in streams)
    full = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    cut = 120
    assert len(streams[cut]) > 1
    cap = int(full[cut]) + len(streams[cut]) - 1  # ends inside register `cut`: it and all after it are cut
    caps = (cap, n_ops + 5) if which == "ops" else (n_ops + 5, cap)
    res = wire.mvreg_ops_ingest(data, off, actors, sync=False, caps=caps)
    st = res.status.cpu().numpy()
    assert not st[:cut].any() and (st[cut:] == CAP).all()
    op_off = res.ops.op_off.cpu().numpy()
    assert np.array_equal(op_off[:cut + 1], full[:cut + 1]) and (op_off[cut:] == full[cut]).all()
    want = cg.mvreg.encode_ops(tuples(streams[:cut]), A, "cuda:0")
    kept = int(full[cut])
    assert np.array_equal(res.ops.clk_row.cpu().numpy()[:kept], np.arange(kept))
    assert np.array_equal(to_host(res.ops.clk_pool)[:kept], to_host(want.clk_pool)[:kept])
    assert np.array_equal(to_host(res.ops.val)[:kept], to_host(want.val)[:kept])
    # the sizing call alone
    tot = (ctypes.c_uint64 * 2)()
    status = torch.empty(N, dtype=torch.int32, device="cuda:0")
    gpu_ctx.call("crdt_mvreg_ops_ingest", dptr(data), dptr(off), N, dptr(actors), A, None, dptr(status), tot)
    assert (int(tot[0]), int(tot[1])) == (n_ops, n_ops)


def test_ops_refusals_leave_neighbours_intact(gpu_ctx):
    A, V = 5, 4
    rng = np.random.default_rng(6)
    aid = W.sparse_dict(rng, A, 32)
    unknown = aid[1] + 1
    assert unknown not in aid
    bad_aid = list(aid)
    bad_aid[1] = unknown
    P, C = O.MVRegPut, O.VClock
    g = [P(C({0: 1}), 11), P(C({1: 2, 2: 1}), 12)]
    gb = W.enc_ops(g, aid)
    empty_put = [P(C(), 21), P(C({3: 1}), 22), P(C(), 23)]
    cases = [  # (frame, status, the ops the frame contributes)
        (gb, 0, g),
        (gb[:-4], BAD, []),                                              # truncated
        (gb, 0, g),
        (gb + bytes(4), BAD, []),                                        # trailing bytes
        (struct.pack("<Q", 1 << 40) + gb[8:], BAD, []),                  # n_ops cannot fit
        (gb[:8] + struct.pack("<I", 1) + gb[12:], BAD, []),              # tag 1
        (gb, 0, g),
        (gb[:12] + struct.pack("<Q", 1 << 50) + gb[20:], BAD, []),       # a record count that cannot fit
        (W.enc_ops([P(C({0: 1, 1: 2}), 3)], bad_aid), MISSING, [P(C({0: 1}), 3)]),  # record skipped, op kept
        (W.enc_ops(empty_put, aid), 0, empty_put),                       # empty-clock Puts are ops
        (b"", BAD, []),
        (W.enc_ops([], aid), 0, []),
        (gb, 0, g),
    ]
    data, off = dev_frames([c[0] for c in cases])
    actors = dev_dict(aid)
    res = wire.mvreg_ops_ingest(data, off, actors)
    assert res.status.cpu().numpy().tolist() == [c[1] for c in cases]
    streams = [c[2] for c in cases]
    n_ops = sum(len(s) for s in streams)
    assert res.totals == (n_ops, n_ops)
    same_batch(res.ops, cg.mvreg.encode_ops(tuples(streams), A, "cuda:0"), n_ops)
    # apply ignores the empty-clock Puts (mvreg.rs:136-138), as the oracle does
    n = len(cases)
    vc = torch.zeros((n, V, A), dtype=torch.int64, device="cuda:0")
    vv = torch.zeros((n, V), dtype=torch.int64, device="cuda:0")
    assert not cg.mvreg.apply_batch(vc, vv, res.ops).cpu().numpy().any()
    want = []
    for s in streams:
        r = O.MVReg()
        for op in s:
            r.apply(op)
        want.append(r)
    assert want[9].vals == [(C({3: 1}), 22)]
    e_c, e_v = W.dense(want, A, V)
    assert np.array_equal(to_host(vc), e_c) and np.array_equal(to_host(vv), e_v)
    # a misaligned offset
    raw = gb + gb + bytes(2) + gb + bytes(2) + gb
    L = len(gb)
    off = torch.tensor([0, L, 2 * L + 2, 3 * L + 4, 4 * L + 4], dtype=torch.int64, device="cuda:0")
    res = wire.mvreg_ops_ingest(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to("cuda:0"), off, actors)
    assert res.status.cpu().numpy().tolist() == [0, BAD, BAD, 0]
    same_batch(res.ops, cg.mvreg.encode_ops(tuples([g, [], [], g]), A, "cuda:0"), 4)


def test_ops_egress_refuses_an_op_without_a_wire_form(gpu_ctx):
    A, V = 64, 4
    aid, _, streams = batch_for(A, V)
    actors = dev_dict(aid)
    ops = cg.mvreg.encode_ops(tuples(streams), A, "cuda:0")
    full = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    row = ops.clk_row.clone()
    row[int(full[1]) + 63] = ops.clk_pool.shape[0] + 5  # the last op of register 1 (64 ops)
    op_off = ops.op_off.clone()
    op_off[7], op_off[8] = op_off[8].item(), op_off[7].item()  # registers 6 and 8 keep a valid range, 7 is reversed
    assert len(streams[7]) > 0
    f_off, out, st = wire.mvreg_ops_egress(ops._replace(clk_row=row, op_off=op_off), actors)
    st = st.cpu().numpy()
    assert st[1] == MISSING and st[7] == MISSING
    got = W.split(out.cpu().numpy(), f_off.cpu().numpy())
    assert got[1] == bytes(8) and got[7] == bytes(8)
    for i in (0, 2, 3, 5, 9, N - 1):
        assert st[i] == 0 and got[i] == W.enc_ops(streams[i], aid)


# ---- one loop on the device ---------------------------------------------------------------------------
def test_frames_to_frames_loop(gpu_ctx):
    """Replica A's Put frames -> ops_ingest -> apply_batch on replica B's registers -> forget_batch
    by a clock derived from read -> egress -> ingest on a third set -> merge_batch; every step
    against the oracle doing the same on objects."""
    A, V = 64, 4
    aid, regs_a, streams = batch_for(A, V)
    rng = np.random.default_rng(99)
    actors = dev_dict(aid)
    Vb = 2 * V  # B's own values plus A's
    regs_b = [W.replay(rng, A, 6, V, int(rng.integers(0, 6)))[0] for _ in range(N)]
    b_c, b_v = (to_dev(x) for x in W.dense(regs_b, A, Vb))
    res = wire.mvreg_ops_ingest(*dev_frames([W.enc_ops(s, aid) for s in streams]), actors)
    ast = cg.mvreg.apply_batch(b_c, b_v, res.ops).cpu().numpy()
    want = []
    for r, s in zip(regs_b, streams):
        r = r.copy()
        for op in s:
            r.apply(op)
            assert len(r.vals) <= Vb
        want.append(r)
    assert not ast.any()
    e_c, e_v = W.dense(want, A, Vb)
    assert np.array_equal(to_host(b_c), e_c) and np.array_equal(to_host(b_v), e_v)
    # forget what the first value of every register has seen (from the device read: add_clock
    # restricted to that value's actors)
    rd = cg.mvreg.read(b_c, b_v)
    y = rd.add_clock * (b_c[:, 0] != 0)
    cg.mvreg.forget_batch(b_c, b_v, y)
    y_h = to_host(y)
    for i, r in enumerate(want):
        r.forget(O.VClock({int(a): int(y_h[i, a]) for a in np.flatnonzero(y_h[i])}))
    assert any(r.vals for r in want) and any(not r.vals for r in want)
    e_c, e_v = W.dense(want, A, Vb)
    assert np.array_equal(to_host(b_c), e_c) and np.array_equal(to_host(b_v), e_v)
    # ship B's registers to a third replica and merge them into its own
    f_off, out = wire.mvreg_egress(b_c, b_v, actors)
    assert bytes(out.cpu().numpy()) == b"".join(W.enc_reg(r, aid) for r in want)
    i_c, i_v, ist = wire.mvreg_ingest(out, f_off, actors, Vb)
    assert not ist.cpu().numpy().any() and np.array_equal(to_host(i_c), e_c)
    regs_c = [W.replay(rng, A, 6, V, int(rng.integers(0, 6)))[0] for _ in range(N)]
    Vc = V + Vb
    c_c, c_v = (to_dev(x) for x in W.dense(regs_c, A, Vc))
    mst = cg.mvreg.merge_batch(c_c, c_v, i_c, i_v).cpu().numpy()
    assert not mst.any()
    for rc, rb in zip(regs_c, want):
        rc.merge(rb)
    e_c, e_v = W.dense(regs_c, A, Vc)
    assert np.array_equal(to_host(c_c), e_c) and np.array_equal(to_host(c_v), e_v)
