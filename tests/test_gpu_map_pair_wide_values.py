"""crdt_map_merge_batch and crdt_map_eq_batch with 33..64 value slots a side (the generic pair kernel of
merge_pairs.hip and eq_reg_wide_kernel of eq.hip with u64 slot masks): op-replay states whose keys
hold one value per concurrent writer, and arbitrary states, both with deferred removes that name keys
holding more than 32 values.  Expected states come from O.Map.merge, expected `ne` words from O.Map /
O.MVReg `==` (eq_util.map_word)."""
import numpy as np
import pytest

import oracle as O
from eq_util import ENTRIES, VALUES, map_word
from gpu_util import to_host
import mvreg_wide_util as W
from test_gpu_merge_batch import _canon, map_egress, map_side

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402

K, N = 5, 24
SHAPES = [(33, 33), (64, 64), (64, 8), (64, 33), (33, 64)]


def replayed(rng, n, A, vmax):
    """Op-replay states over A >= 64 actors: every writer writes each key once from its own origin, so
    a state that applied w writers' ops holds w concurrent values per key; removes issued by origins
    that saw some of the writes defer on a state that has not.  A state takes at most `vmax` writers."""
    vmax = min(vmax, 64)
    writers = min(A, 64)
    origins = [O.Map(O.MVReg) for _ in range(writers)]
    ups, val = {}, 1
    for a, m in enumerate(origins):
        ups[a] = []  # this writer's ops in its causal order
        for k in rng.permutation(K):
            op = m.update(int(k), m.get(int(k)).derive_add_ctx(a), lambda r, c, v=val: r.write(v, c))
            m.apply(op)
            ups[a].append(op)
            val += 1
    rms = []
    for _ in range(6):  # a remover that saw some writers' ops removes one or two keys
        seer = O.Map(O.MVReg)
        for a in rng.choice(writers, size=int(rng.integers(3, 40)), replace=False):
            for op in ups[int(a)]:
                seer.apply(op)
        k = int(rng.integers(K))
        rms.append(seer.rm(k, seer.get(k).derive_rm_ctx()))
    states = []
    for i in range(n):  # (state 0: exactly vmax writers, every op, no remove)
        m = O.Map(O.MVReg)
        who = rng.choice(writers, size=vmax if i == 0 else int(rng.integers(1, vmax + 1)), replace=False)
        todo = [op for a in who for op in ups[int(a)] if i == 0 or rng.random() < 0.95]  # (a writer's ops stay in order)
        for j in rng.choice(len(rms), size=0 if i == 0 else int(rng.integers(0, 3)), replace=False):
            todo.insert(int(rng.integers(len(todo) + 1)), rms[int(j)])
        for op in todo:
            m.apply(op)
        states.append(m)
    return states


def arbitrary_states(rng, n, A, V, fill):
    """Arbitrary dense states: any clock and entry clocks, registers of W.arbitrary (no antichains,
    holes), deferred removes naming every key that holds more than 32 values."""
    maps = []
    for _ in range(n):
        few = rng.random() < 0.4  # some states hold few values, so some merged pairs fit self's slots
        clock = np.zeros(A, np.uint64)
        ec = np.zeros((K, A), np.uint64)
        acts = W.actors_of(rng, A)
        clock[acts] = rng.integers(0, 4, size=len(acts))
        ec[:, acts] = rng.integers(0, 5, size=(K, len(acts)))
        ec[rng.random(K) < 0.2] = 0
        vclk, vval = W.arbitrary(rng, K, V, A, fill=0.15 if few else fill, full=0.0 if few else 0.3)
        big = [k for k in range(K) if ec[k].any() and vclk[k].any(axis=1).sum() > 32]
        deferred = []
        for _ in range(int(rng.integers(0, 3))):
            rm = np.zeros(A, np.uint64)
            rm[acts] = rng.integers(0, 6, size=len(acts)) * (rng.random(len(acts)) < 0.6)
            keys = set(big) | {int(rng.integers(K))}
            if rm.any() and not any(np.array_equal(rm, r) for r, _ in deferred):
                deferred.append((rm, keys))
        maps.append(O.dense_to_map(clock, ec, vclk, vval, deferred))
    return maps


def check_pairs(ctx, lhs, rhs, A, V1, V2):
    """merge_batch against O.Map.merge with self's V fixed at V1: bit 4 on exactly the pairs where a
    merged register needs more than V1 slots, every other pair identical to the oracle in Vec order."""
    exp = []
    for a, b in zip(lhs, rhs):
        x = a.copy()
        x.merge(b.copy())
        exp.append(x)
    over = np.array([O.max_vals([x]) > V1 for x in exp])
    Dcap = max(1, max(len(x.deferred) for x in list(lhs) + exp))
    me = map_side(lhs, K, A, V1, Dcap)
    other = map_side(rhs, K, A, V2, max(1, max(len(b.deferred) for b in rhs)))
    status = cg.map.merge_batch(me, other, ctx=ctx).cpu().numpy()
    np.testing.assert_array_equal(status, np.where(over, 16, 0))
    got = map_egress(me, len(lhs))
    for i, ((g, vc, vv, ec), e) in enumerate(zip(got, exp)):
        if over[i]:
            continue
        assert _canon(g) == _canon(e), i
        for k, ent in e.entries.items():  # Vec order: kept own values, then other's added ones
            used = [j for j in range(vc.shape[1]) if vc[k, j].any()]
            assert used == list(range(len(used))) and [int(vv[k, j]) for j in used] == [v for _, v in ent.val.vals], (i, k)
        assert not vc[~ec.any(axis=1)].any()
    return exp, over, me


def eq_check(ctx, xs, ys, A, Vx, Vy):
    want = np.array([map_word(a, b) for a, b in zip(xs, ys)], np.int32)
    D = max(1, max(len(m.deferred) for m in list(xs) + list(ys)))
    ne = cg.map.eq_batch(map_side(xs, K, A, Vx, D), map_side(ys, K, A, Vy, D + 1), ctx=ctx).cpu().numpy()
    np.testing.assert_array_equal(ne, want)
    return want


def with_slots(m, f):
    """A copy of the state whose biggest register's value list went through f."""
    y = m.copy()
    if not y.entries:
        return y
    k = max(y.entries, key=lambda k: len(y.entries[k].val.vals))
    y.entries[k].val.vals = f(y.entries[k].val.vals)
    return y


@pytest.mark.parametrize("V1,V2", SHAPES)
def test_map_pairs_replayed(gpu_ctx, V1, V2):
    A = 65
    rng = np.random.default_rng(100 * V1 + V2)
    lhs, rhs = replayed(rng, N, A, V1), replayed(rng, N, A, V2)
    rhs[0] = O.Map(O.MVReg)  # pair 0: min(V1, 64) values a key on self, nothing on the other side
    exp, over, _ = check_pairs(gpu_ctx, lhs, rhs, A, V1, V2)
    assert not over.all() and (over.any() or V1 == 64)  # bit 4 fires when self's V is too small, and only then
    assert max(O.max_vals([x]) for x, o in zip(exp, over) if not o) > min(32, V1 - 1)
    assert any(len(x.deferred) for x in lhs + rhs)
    # ==: a state against itself with the biggest register's slots reversed / one payload changed / one value
    # dropped, and the two sides of every pair against each other
    ys = [m.copy() if i % 4 == 0 else with_slots(m, [lambda v: v[::-1], lambda v: v[:-1] + [(v[-1][0], v[-1][1] ^ 1)],
                                                   lambda v: v[:-1]][i % 4 - 1]) for i, m in enumerate(lhs)]
    want = eq_check(gpu_ctx, lhs, ys, A, V1, 64)
    assert set(want[0::4]) == {0} and set(want[1::4]) == {0} and VALUES in set(want[2::4]) | set(want[3::4])
    eq_check(gpu_ctx, lhs, rhs, A, V1, V2)


@pytest.mark.parametrize("A", [3, 65])
@pytest.mark.parametrize("V1,V2", SHAPES)
def test_map_pairs_arbitrary(gpu_ctx, V1, V2, A):
    rng = np.random.default_rng(1000 * V1 + 10 * V2 + A)
    lhs = arbitrary_states(rng, N, A, V1, 0.85 if V1 == 64 else 0.6)
    rhs = arbitrary_states(rng, N, A, V2, 0.85)
    for m in rhs:  # (values of the two sides never collide)
        for e in m.entries.values():
            e.val.vals = [(c, v + (1 << 50)) for c, v in e.val.vals]
    exp, over, me = check_pairs(gpu_ctx, lhs, rhs, A, V1, V2)
    assert not over.all()
    assert max(O.max_vals([m]) for m in lhs + rhs) > 32
    ys = [m.copy() if i % 3 == 0 else with_slots(m, [lambda v: v[::-1], lambda v: v[1:]][i % 3 - 1]) for i, m in enumerate(lhs)]
    want = eq_check(gpu_ctx, lhs, ys, A, V1, 64)
    assert set(want[0::3]) == {0} and set(want[1::3]) == {0} and VALUES in set(want[2::3])
    w = eq_check(gpu_ctx, lhs, rhs, A, V1, V2)
    assert (w & (VALUES | ENTRIES)).any()
