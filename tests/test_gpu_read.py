"""Batched reads on the GPU (csrc/read.hip): the presence scan behind orswot.read / map.read and
the contains / get / mvreg.read / derive_add_ctx gathers, against the oracle's objects
(O.Orswot.read / contains, O.MVReg.read, O.Map.len / get, O.ReadCtx.derive_add_ctx)."""
import numpy as np
import pytest
import torch

import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402


SCAN_DEFAULTS = "rdbpc=0,rdu=8,rdnt=1"  # csrc/common.hpp Tune::read_*


def vc_of(row) -> O.VClock:
    return O.VClock({a: int(c) for a, c in enumerate(np.asarray(row).tolist()) if c})


def row_of(vc: O.VClock, A: int) -> np.ndarray:
    r = np.zeros(A, np.uint64)
    for a, c in vc.dots.items():
        r[a] = c
    return r


def bitmap(members, n: int) -> np.ndarray:
    w = np.zeros((n + 63) // 64, np.uint64)
    for m in members:
        w[m // 64] |= np.uint64(1) << np.uint64(m % 64)
    return w


def i32(x) -> torch.Tensor:
    return torch.tensor(np.asarray(x, dtype=np.int64).astype(np.uint32).view(np.int32), dtype=torch.int32,
                        device="cuda:0")


def orswots_of(clock, entries):
    out = []
    for s in range(entries.shape[0]):
        o = O.Orswot()
        o.clock = vc_of(clock[s])
        for m in range(entries.shape[1]):
            if entries[s, m].any():
                o.entries[m] = vc_of(entries[s, m])
        out.append(o)
    return out


def maps_of(clock, ec):
    out = []
    for s in range(ec.shape[0]):
        m = O.Map(O.MVReg)
        m.clock = vc_of(clock[s])
        for k in range(ec.shape[1]):
            if ec[s, k].any():
                m.entries[k] = O.MapEntry(vc_of(ec[s, k]), O.MVReg())
        out.append(m)
    return out


def random_rows(rng, N, M, A):
    """Sparse dot-clock rows: about half the rows present, a present row mostly zeros."""
    e = rng.integers(1, 2**63, size=(N, M, A), dtype=np.uint64) * (rng.random((N, M, A)) < 0.3)
    present = rng.random((N, M)) < 0.5
    one = rng.integers(0, A, size=(N, M))
    for s in range(N):
        for m in range(M):
            if present[s, m] and not e[s, m].any():
                e[s, m, one[s, m]] = 1
    e *= present[:, :, None]
    return e.astype(np.uint64), e.max(axis=1).astype(np.uint64)


def check_scan(ctx, clock, entries, dev_entries=None):
    """orswot.read and map.read of the same rows against O.Orswot.read / O.Map.len."""
    N, M, A = entries.shape
    de = to_dev(entries) if dev_entries is None else dev_entries
    dc = to_dev(clock)
    rc = cg.orswot.read(dc, de, ctx=ctx)
    rm = cg.map.read(dc, de, ctx=ctx)
    assert rc.add_clock is dc and rc.rm_clock is dc
    members, n = to_host(rc.val[0]), rc.val[1].cpu().numpy()
    keys, nk = to_host(rm.val[0]), rm.val[1].cpu().numpy()
    assert members.shape == (N, (M + 63) // 64) and n.dtype == np.int32
    objs, mobjs = orswots_of(clock, entries), maps_of(clock, entries)
    for s in range(N):
        want = objs[s].read()
        assert np.array_equal(members[s], bitmap(want.val, M)), (s, M, A)
        assert int(n[s]) == len(want.val)
        assert np.array_equal(keys[s], bitmap(mobjs[s].entries.keys(), M))
        assert int(nk[s]) == mobjs[s].len().val and (nk[s] == 0) == mobjs[s].is_empty().val
    return objs


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A", [1, 2, 3, 16, 64, 65, 200])
def test_presence_scan_shapes(gpu_ctx, N, A):
    """Odd A: the 8-byte path; A = 200: several loads per row; M = 65, 130: a partial last word."""
    rng = np.random.default_rng(1000 * N + A)
    for M in (1, 63, 64, 65, 130):
        entries, clock = random_rows(rng, N, M, A)
        if M == 1:
            entries[0, 0] = 0
            entries[0, 0, A - 1] = 5  # a present row in every one-member case
        objs = check_scan(gpu_ctx, clock, entries)
        n = sum(len(o.entries) for o in objs)
        assert n > 0 and (M < 63 or n < N * M), "some rows present and some absent"


@pytest.mark.parametrize("tune", ["rdu=4", "rdu=8", "rdbpc=1,rdnt=0", "rdbpc=2,rdu=4,rdnt=0"])
def test_presence_scan_row_patterns(gpu_ctx, tune):
    """Every kernel variant the launch knobs select (4 / 8 loads in flight, non-temporal / plain loads,
    a grid-stride loop of one or two workgroups per CU) on rows that differ in one word."""
    N, M, A = 3, 130, 65
    entries = np.zeros((N, M, A), np.uint64)
    # state 0 stays all absent; state 1 all present: only the first word (even m) / only the last
    entries[1, 0::2, 0] = 7
    entries[1, 1::2, A - 1] = 9
    entries[2, 5, 7] = np.uint64(1) << np.uint64(63)   # lost by a signed or 32-bit reduction
    entries[2, 9, 64] = np.uint64(1) << np.uint64(32)
    entries[2, 64, 0] = 1
    entries[2, 129, A - 1] = 1
    clock = entries.max(axis=1)
    gpu_ctx.tune(tune)
    try:
        objs = check_scan(gpu_ctx, clock, entries)
        # the same patterns on the 16-byte path: A = 64 without the unused column 32
        check_scan(gpu_ctx, np.delete(clock, 32, axis=1), np.delete(entries, 32, axis=2))
    finally:
        gpu_ctx.tune(SCAN_DEFAULTS)
    assert [len(o.entries) for o in objs] == [0, M, 4]


@pytest.mark.parametrize("N,M,A", [(3, 130, 64), (2, 65, 3), (3, 64, 200)])
def test_presence_scan_writes_every_output(gpu_ctx, N, M, A):
    """Buffers pre-filled with 0xFF..: tail bits past M and len come back exact."""
    rng = np.random.default_rng(N * M + A)
    entries, clock = random_rows(rng, N, M, A)
    de = to_dev(entries)
    Mw = (M + 63) // 64
    for fn in ("crdt_orswot_read", "crdt_map_read"):
        bits = torch.full((N, Mw), -1, dtype=torch.int64, device="cuda:0")
        n = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        gpu_ctx.call(fn, de.data_ptr(), A, M * A, N, M, A, bits.data_ptr(), n.data_ptr())
        bits2 = torch.full((N, Mw), -1, dtype=torch.int64, device="cuda:0")
        gpu_ctx.call(fn, de.data_ptr(), A, M * A, N, M, A, bits2.data_ptr(), None)  # len may be NULL
        got, cnt = to_host(bits), n.cpu().numpy()
        for s, o in enumerate(orswots_of(clock, entries)):
            assert np.array_equal(got[s], bitmap(o.read().val, M)), (fn, s)
            assert int(cnt[s]) == len(o.read().val)
        assert np.array_equal(to_host(bits2), got)
    assert 0 < cnt.sum() < N * M


@pytest.mark.parametrize("A,pad,base", [(64, 3, 0), (65, 3, 0), (16, 3, 0), (64, 2, 0), (64, 2, 1), (200, 3, 2)])
def test_presence_scan_strided(gpu_ctx, A, pad, base):
    """entries a view with entry_mstride = A + pad and a state stride past M rows; the padding holds
    non-zero garbage.  pad = 3 gives odd or unaligned rows (8-byte path), (64, 2, 0) padded 16-byte
    rows, base = 1 a pointer one word off 16-byte alignment."""
    N, M = 3, 130
    rng = np.random.default_rng(A * 8 + pad + base)
    entries, clock = random_rows(rng, N, M, A)
    entries[1] = 0  # an all-absent state between garbage
    ms = A + pad
    ss = M * ms + (5 if pad == 3 else 6)
    store = torch.full((base + N * ss + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    view = torch.as_strided(store, (N, M, A), (ss, ms, 1), base)
    view.copy_(to_dev(entries))
    assert (view.data_ptr() % 16 == 8) == (base % 2 == 1)
    objs = check_scan(gpu_ctx, clock, entries, dev_entries=view)
    assert not objs[1].entries and 0 < len(objs[0].entries) < M


# ---- contains / get --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orswot_states():
    from orswot_apply_util import dense_states, oracle_streams, replay_streams
    M, A = 70, 5
    streams = replay_streams(11, 6, A, M, 160)
    objs = oracle_streams([O.Orswot() for _ in streams], streams)
    clock, entries, *_ = dense_states(objs, M, A, 8)
    return objs, clock, entries, M, A


def test_orswot_contains(gpu_ctx, orswot_states):
    objs, clock, entries, M, A = orswot_states
    N = len(objs)
    rng = np.random.default_rng(5)
    qs, qm = [], []
    for s, o in enumerate(objs):
        present = sorted(o.entries)
        absent = [m for m in range(M) if m not in o.entries]
        assert present and absent
        for m in present[:3] + absent[:2] + present[:1]:  # several per state, one repeated
            qs.append(s)
            qm.append(m)
    order = rng.permutation(len(qs))
    qs, qm = [qs[i] for i in order], [qm[i] for i in order]
    qs += [0, N, 1, 2**32 - 1]  # member >= M, state >= N
    qm += [M, 0, 2**31, 0]
    rc, status = cg.orswot.contains(to_dev(clock), to_dev(entries), i32(qs), i32(qm), ctx=gpu_ctx)
    add, rm, val, st = to_host(rc.add_clock), to_host(rc.rm_clock), rc.val.cpu().numpy(), status.cpu().numpy()
    assert val.dtype == np.uint8 and rm.shape == (len(qs), A)
    for q, (s, m) in enumerate(zip(qs, qm)):
        if s >= N or m >= M:
            assert st[q] == 2 and val[q] == 0 and not rm[q].any(), q
            assert np.array_equal(add[q], clock[s] if s < N else np.zeros(A, np.uint64)), q
            continue
        want = objs[s].contains(m)
        assert st[q] == 0 and bool(val[q]) == want.val, q
        assert np.array_equal(rm[q], row_of(want.rm_clock, A)), q
        assert np.array_equal(add[q], row_of(want.add_clock, A)), q
    assert 0 < val.sum() < len(qs)


def gapped_maps(V, K, A, seed):
    """Map<K, MVReg> objects whose registers hold 0..V concurrent values, and their dense form with
    an empty slot moved between the used ones where V allows it."""
    rng = np.random.default_rng(seed)
    maps = []
    for _ in range(3):
        m = O.Map(O.MVReg)
        for k in range(K):
            if k and rng.random() < 0.3:
                continue
            nv = int(rng.integers(1, V + 1)) if k else V  # key 0: a full register
            vals = []
            for j in range(nv):  # pairwise concurrent clocks: each has its own actor ahead
                c = O.VClock({j % A: 10 + j, (j + 1 + k) % A: 1 + int(rng.integers(0, 3))})
                vals.append((c, 100 * k + j + 1))
            ec = O.VClock()
            for c, _ in vals:
                ec.merge(c)
            m.entries[k] = O.MapEntry(ec, O.MVReg(vals))
            m.clock.merge(ec)
        maps.append(m)
    d = O.map_to_dense(maps, K, A, V)
    gaps = 0
    if V >= 4:
        for s, m in enumerate(maps):
            for k, e in m.entries.items():
                n = len(e.val.vals)
                if 2 <= n < V:  # slots [0..n) -> [0..n-1) + slot V-1: a gap between used slots
                    d["vclk"][s, k, V - 1] = d["vclk"][s, k, n - 1]
                    d["vval"][s, k, V - 1] = d["vval"][s, k, n - 1]
                    d["vclk"][s, k, n - 1] = 0
                    d["vval"][s, k, n - 1] = 0
                    gaps += 1
        assert gaps > 0
    return maps, d


class DenseMap:
    def __init__(self, d):
        self.clock, self.ec, self.vclk, self.vval = (to_dev(d[k]) for k in ("clock", "ec", "vclk", "vval"))


@pytest.mark.parametrize("V,A", [(1, 3), (4, 5), (16, 20)])
def test_map_get(gpu_ctx, V, A):
    K = 9
    maps, d = gapped_maps(V, K, A, 40 + V)
    N = len(maps)
    qs = [s for s in range(N) for _ in range(K)] + [1, 1, 0, N, 0]
    qk = [k for _ in range(N) for k in range(K)] + [0, 0, K, 0, 2**31]
    rc, status = cg.map.get(DenseMap(d), i32(qs), i32(qk), ctx=gpu_ctx)
    add, rm, st = to_host(rc.add_clock), to_host(rc.rm_clock), status.cpu().numpy()
    v = rc.val
    present, vclk, vval = v.present.cpu().numpy(), to_host(v.vclk), to_host(v.vval)
    nval, val_clock = v.nval.cpu().numpy(), to_host(v.val_clock)
    assert vclk.shape == (len(qs), V, A) and vval.shape == (len(qs), V)
    seen = set()
    for q, (s, k) in enumerate(zip(qs, qk)):
        if s >= N or k >= K:
            assert st[q] == 2 and present[q] == 0 and nval[q] == 0, q
            assert not rm[q].any() and not vclk[q].any() and not vval[q].any() and not val_clock[q].any(), q
            continue
        want = maps[s].get(k)
        assert st[q] == 0 and bool(present[q]) == (want.val is not None), q
        assert np.array_equal(rm[q], row_of(want.rm_clock, A)) and np.array_equal(add[q], row_of(want.add_clock, A)), q
        vals = want.val.vals if want.val is not None else []
        assert nval[q] == len(vals), q
        for j, (c, x) in enumerate(vals):
            assert np.array_equal(vclk[q, j], row_of(c, A)) and int(vval[q, j]) == x, (q, j)
        assert not vclk[q, len(vals):].any() and not vval[q, len(vals):].any(), q
        read = want.val.read() if want.val is not None else O.MVReg().read()
        assert np.array_equal(val_clock[q], row_of(read.add_clock, A)), q
        assert [int(x) for x in vval[q, :len(vals)]] == read.val
        seen.add(len(vals))
    assert {0, V} <= seen


@pytest.mark.parametrize("A", [1, 3, 64, 300])
def test_mvreg_read(gpu_ctx, A):
    V = 6
    rng = np.random.default_rng(A)
    used = [[], [0], [3], list(range(V)), [0, 2, 5], [1, 4], [5]]  # 0, 1 and V used slots, gaps
    regs, vclk, vval = [], np.zeros((len(used), V, A), np.uint64), np.zeros((len(used), V), np.uint64)
    for i, slots in enumerate(used):
        vals = []
        for j in slots:
            row = rng.integers(1, 2**64, size=A, dtype=np.uint64) * (rng.random(A) < 0.4)
            row[int(rng.integers(0, A))] = np.uint64(2**63 + j) if j % 2 else np.uint64(j + 1)
            vclk[i, j], vval[i, j] = row, 1000 * i + j
            vals.append((vc_of(row), 1000 * i + j))
        regs.append(O.MVReg(vals))
    rc = cg.mvreg.read(to_dev(vclk), to_dev(vval), ctx=gpu_ctx)
    clock, vals, nval = to_host(rc.add_clock), to_host(rc.val[0]), rc.val[1].cpu().numpy()
    assert rc.rm_clock is rc.add_clock and clock.shape == (len(used), A)
    for i, r in enumerate(regs):
        want = r.read()
        assert np.array_equal(clock[i], row_of(r.clock(), A)) and want.add_clock == r.clock(), i
        assert nval[i] == len(want.val) and [int(x) for x in vals[i, :nval[i]]] == want.val, i
        assert not vals[i, nval[i]:].any()


def test_derive_add_ctx(gpu_ctx):
    A = 70
    clocks = [O.VClock({0: 4, 3: 9}), O.VClock({69: 2**63}), O.VClock(), O.VClock({a: a + 1 for a in range(A)}),
              O.VClock({5: 2**64 - 1, 6: 1}), O.VClock({1: 1})]
    actors = [3, 0, 69, 64, 5, A]  # present, absent, absent in an empty clock, present, overflow, out of range
    rows = np.stack([row_of(c, A) for c in clocks])
    dev = to_dev(rows)
    rc = cg.ReadCtx(dev, dev, None)
    add = cg.derive_add_ctx(rc, i32(actors), ctx=gpu_ctx)
    out, counter, st = to_host(add.clock), to_host(add.counter), add.status.cpu().numpy()
    assert np.array_equal(to_host(dev), rows), "the input rows are untouched without out="
    for q, (c, a) in enumerate(zip(clocks, actors)):
        if q < 4:
            want = O.ReadCtx(c, c, None).derive_add_ctx(a)
            assert st[q] == 0 and int(counter[q]) == want.dot.counter and want.dot.actor == a, q
            assert np.array_equal(out[q], row_of(want.clock, A)), q
        else:
            assert st[q] == (4 if q == 4 else 2) and counter[q] == 0 and np.array_equal(out[q], rows[q]), q
    assert cg.derive_rm_ctx(rc).clock is dev
    # in place: out aliases the add_clock rows; a scalar actor serves every row
    alias = cg.derive_add_ctx(rc, 3, ctx=gpu_ctx, out=dev)
    got = to_host(alias.clock)
    assert alias.clock.data_ptr() == dev.data_ptr()
    for q, c in enumerate(clocks):
        assert np.array_equal(got[q], row_of(O.ReadCtx(c, c, None).derive_add_ctx(3).clock, A)), q
