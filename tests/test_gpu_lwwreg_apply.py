"""crdt_lwwreg_apply_batch (csrc/lwwreg_apply.hip) against the oracle's LWWReg.update applied op by
op: ragged streams over N = 200 registers (stream lengths on both sides of the 64-op step and of the
64-register group), the reference's own update sequences, unsigned markers, invalid offsets inside
otherwise valid groups, empty batches, and agreement with the fold of crdt_lwwreg_lub_many."""
import ctypes

import numpy as np
import pytest
import torch

import lattice_ops_util as L
import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi, lwwreg  # noqa: E402
from crdts_gpu.context import dptr  # noqa: E402

N = 200
ERR, BAD_RANGE = 1, 8
_CACHE = {}


def lengths():
    rng = np.random.default_rng(11)
    n = [int(x) for x in rng.integers(0, 71, size=N)]
    n[0] = n[63] = n[N - 1] = 1000
    n[64] = n[N - 2] = 0
    n[1:9] = [1, 2, 63, 64, 65, 127, 128, 129]
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000} <= set(n)
    return n


def batch():
    """Initial states, the (val, marker) streams, and the oracle's replay (built once)."""
    if "b" not in _CACHE:
        rng = np.random.default_rng(12)
        m0 = rng.integers(0, 8, size=N).astype(np.uint64)
        v0 = rng.integers(0, 3, size=N).astype(np.uint64)
        streams = [[(int(rng.integers(0, 3)), int(rng.integers(0, 8))) for _ in range(n)] for n in lengths()]
        _CACHE["b"] = (m0, v0, streams) + replay(m0, v0, streams)
    return _CACHE["b"]


def replay(m0, v0, streams):
    regs = [O.LWWReg(int(v), int(m)) for m, v in zip(m0, v0)]
    conf = [L.replay_lww(r, s) for r, s in zip(regs, streams)]
    em = np.array([r.marker for r in regs], np.uint64)
    ev = np.array([r.val for r in regs], np.uint64)
    return em, ev, conf


def apply(m0, v0, streams):
    m, v = to_dev(m0), to_dev(v0)
    ops = lwwreg.encode_ops(streams, "cuda:0")
    conflict, status = lwwreg.apply_batch(m, v, ops)
    torch.cuda.synchronize()
    return to_host(m), to_host(v), conflict.cpu().numpy(), status.cpu().numpy(), ops


def test_the_batch_holds_every_outcome():
    m0, v0, streams, em, ev, conf = batch()
    seen = set()
    for i, s in enumerate(streams):
        r = O.LWWReg(int(v0[i]), int(m0[i]))
        for k, (val, marker) in enumerate(s):
            kind = ("replace" if marker > r.marker else "stale" if marker < r.marker
                    else "redundant" if val == r.val else "err")
            seen.add(kind)
            if kind == "err" and k == 0:
                seen.add("err on the first op")
            assert L.replay_lww(r, [(val, marker)]) == [int(kind == "err")]
    assert seen == {"replace", "stale", "redundant", "err", "err on the first op"}


def test_ragged_streams_equal_the_oracle():
    m0, v0, streams, em, ev, conf = batch()
    gm, gv, gc, gs, ops = apply(m0, v0, streams)
    assert np.array_equal(gm, em) and np.array_equal(gv, ev)
    assert np.array_equal(gc, np.array([c for s in conf for c in s], np.uint8))
    assert np.array_equal(gs, np.array([ERR if any(s) else 0 for s in conf]))
    # conflict and status both NULL: the same states
    m, v = to_dev(m0), to_dev(v0)
    o = _abi.LwwRegOps(ops.marker.shape[0], dptr(ops.op_off), dptr(ops.marker), dptr(ops.val))
    ctx = cg.Context.default(0)
    ctx.call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), N, ctypes.byref(o), None, None)
    assert np.array_equal(to_host(m), em) and np.array_equal(to_host(v), ev)


# lwwreg.rs:113-138 (test_update) and :66-82 (the doc comment of update): the start state, then
# (val, marker, is_err, state after) per update
REFERENCE = [
    ((123, 0), [(32, 2, 0, (32, 2)), (57, 1, 0, (32, 2)), (32, 2, 0, (32, 2)), (4000, 2, 1, (32, 2))]),
    ((1, 2), [(2, 1, 0, (1, 2)), (2, 2, 1, (1, 2)), (1, 2, 0, (1, 2)), (2, 3, 0, (2, 3))]),
]


def test_the_reference_sequences():
    # every prefix of each sequence as its own register: the state after each update is checked too
    m0, v0, streams, want, errs = [], [], [], [], []
    for (val, marker), seq in REFERENCE:
        for k in range(len(seq) + 1):
            m0.append(marker)
            v0.append(val)
            streams.append([(v, m) for v, m, _, _ in seq[:k]])
            want.append(seq[k - 1][3] if k else (val, marker))
            errs.append([e for _, _, e, _ in seq[:k]])
    m0, v0 = np.array(m0, np.uint64), np.array(v0, np.uint64)
    em, ev, conf = replay(m0, v0, streams)
    assert conf == errs and [(int(v), int(m)) for v, m in zip(ev, em)] == want  # the oracle agrees with the data
    gm, gv, gc, gs, _ = apply(m0, v0, streams)
    assert [(int(v), int(m)) for v, m in zip(gv, gm)] == want
    assert gc.tolist() == [e for s in errs for e in s]
    assert gs.tolist() == [ERR if any(s) else 0 for s in errs]


def test_markers_order_as_unsigned():
    a, b, c = 2**63 - 1, 2**63, 2**64 - 1
    m0 = np.array([a, b, c, 0, c], np.uint64)
    v0 = np.array([7, 7, 7, 7, 7], np.uint64)
    streams = [[(1, b), (2, a), (3, c), (4, c), (3, c)],  # replace, stale, replace, err at 2^64 - 1, redundant
               [(1, a), (2, c), (3, b)],                  # 2^63 - 1 is below 2^63; 2^64 - 1 above
               [(1, b), (1, a), (8, c), (7, c)],          # nothing exceeds 2^64 - 1; an err on it
               [(5, c), (6, b), (9, a)],
               []]
    em, ev, conf = replay(m0, v0, streams)
    assert conf[0] == [0, 0, 0, 1, 0] and conf[2] == [0, 0, 1, 0] and (int(ev[1]), int(em[1])) == (2, c)
    gm, gv, gc, gs, _ = apply(m0, v0, streams)
    assert np.array_equal(gm, em) and np.array_equal(gv, ev)
    assert gc.tolist() == [x for s in conf for x in s]
    assert gs.tolist() == [ERR, 0, ERR, 0, 0]


@pytest.mark.parametrize("case", ["reversed", "past_n_ops"])
def test_invalid_offsets_inside_a_valid_group(case):
    m0, v0, streams, _, _, _ = batch()
    ops = lwwreg.encode_ops(streams, "cuda:0")
    off = ops.op_off.cpu().numpy().copy()
    n_ops = int(off[-1])
    bad = 70 if case == "reversed" else N - 1
    if case == "reversed":
        off[71] = off[70] - 3  # register 70 runs backwards; 71 is valid and re-reads the last 3 ops of 69
        assert off[69] <= off[70] - 3
    else:
        off[N] = n_ops + 5
    valid = [i for i in range(N) if i != bad]
    assert all(off[i] <= off[i + 1] <= n_ops for i in valid) and not off[bad] <= off[bad + 1] <= n_ops
    om, ov = to_host(ops.marker), to_host(ops.val)
    flat = list(zip(ov.tolist(), om.tolist()))
    by_range = [flat[off[i]:off[i + 1]] if i != bad else [] for i in range(N)]
    em, ev, conf = replay(m0, v0, by_range)
    cover = np.zeros(n_ops, np.int64)
    for i in valid:
        cover[off[i]:off[i + 1]] += 1
    m, v = to_dev(m0), to_dev(v0)
    conflict = torch.full((n_ops,), 0x5A, dtype=torch.uint8, device="cuda:0")
    status = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    o = _abi.LwwRegOps(n_ops, dptr(d_off), dptr(ops.marker), dptr(ops.val))
    cg.Context.default(0).call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), N, ctypes.byref(o), dptr(conflict),
                               dptr(status))
    gm, gv, gc, gs = to_host(m), to_host(v), conflict.cpu().numpy(), status.cpu().numpy()
    assert gs[bad] == BAD_RANGE and gm[bad] == m0[bad] and gv[bad] == v0[bad]
    assert np.array_equal(gm, em) and np.array_equal(gv, ev)
    assert [int(gs[i]) for i in valid] == [ERR if any(conf[i]) else 0 for i in valid]
    want = np.full(n_ops, 0x5A, np.uint8)  # an op no valid register covers keeps the sentinel
    for i in valid:
        want[off[i]:off[i + 1]] = conf[i]
    once = cover <= 1  # (an op in two ranges: unspecified)
    assert np.array_equal(gc[once], want[once])
    assert (cover > 1).any() if case == "reversed" else (cover == 0).any()


def test_empty_batches_write_nothing():
    ctx = cg.Context.default(0)
    m0, v0 = np.arange(70, dtype=np.uint64), np.arange(70, dtype=np.uint64) + 100
    m, v = to_dev(m0), to_dev(v0)
    off = torch.zeros(71, dtype=torch.int64, device="cuda:0")
    o = _abi.LwwRegOps(0, dptr(off), None, None)
    ctx.call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), 0, ctypes.byref(o), None, None)  # N = 0, n_ops = 0
    ctx.call("crdt_lwwreg_apply_batch", None, None, 0, None, None, None)
    assert np.array_equal(to_host(m), m0) and np.array_equal(to_host(v), v0)
    # n_ops = 0 over N registers: every range is empty, the states are bit-identical, status 0
    status = torch.full((70,), -1, dtype=torch.int32, device="cuda:0")
    ctx.call("crdt_lwwreg_apply_batch", dptr(m), dptr(v), 70, ctypes.byref(o), None, dptr(status))
    assert np.array_equal(to_host(m), m0) and np.array_equal(to_host(v), v0) and not status.cpu().numpy().any()
    conflict, status = lwwreg.apply_batch(m, v, lwwreg.encode_ops([[]] * 70, "cuda:0"))
    assert conflict.numel() == 0 and not status.cpu().numpy().any()


@pytest.mark.parametrize("G,R", [(130, 70), (3, 600)])
def test_uniform_streams_agree_with_the_fold(G, R):
    rng = np.random.default_rng(G + R)
    m0 = rng.integers(0, 8, size=G).astype(np.uint64)
    v0 = rng.integers(0, 3, size=G).astype(np.uint64)
    om = rng.integers(0, 8, size=(G, R)).astype(np.uint64)
    ov = rng.integers(0, 3, size=(G, R)).astype(np.uint64)
    ov[0, :] = v0[0]  # one value throughout: this register never errs
    fold = lwwreg.lub_many(to_dev(om), to_dev(ov), init=(to_dev(m0), to_dev(v0)))
    m, v = to_dev(m0), to_dev(v0)
    off = torch.arange(0, (G + 1) * R, R, dtype=torch.int64, device="cuda:0")
    ops = lwwreg.LwwRegOpBatch(off, to_dev(om.reshape(-1)), to_dev(ov.reshape(-1)))
    conflict, status = lwwreg.apply_batch(m, v, ops)
    assert np.array_equal(to_host(m), to_host(fold.marker)) and np.array_equal(to_host(v), to_host(fold.val))
    c = conflict.cpu().numpy().reshape(G, R)
    first = np.where(c.any(axis=1), c.argmax(axis=1), -1).astype(np.int64)
    assert np.array_equal(first, fold.first_conflict.cpu().numpy()) and (first >= 0).any() and (first < 0).any()
    assert np.array_equal(status.cpu().numpy(), c.any(axis=1).astype(np.int32))
