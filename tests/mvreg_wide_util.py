"""Shared by the tests of MVReg registers of 17..64 value slots (test_gpu_mvreg_wide_values.py,
test_gpu_map_pair_wide_values.py): dense registers <-> O.MVReg, generators of arbitrary and antichain
registers, padded device tensors, and the expected results, which always come from the oracle's
objects (O.MVReg merge / apply / forget / ==), never from the code under test."""
import numpy as np
import torch

import oracle as O

CHUNK = 16  # the slots one vote round of the device merge takes


def undense(vc, vv):
    """(N, V, A), (N, V) -> O.MVReg objects, empty slots skipped wherever they sit."""
    out = []
    for i in range(vc.shape[0]):
        r = O.MVReg()
        for s in np.flatnonzero(vc[i].any(axis=1)):
            row = vc[i, s]
            r.vals.append((O.VClock({int(a): int(row[a]) for a in np.flatnonzero(row)}), int(vv[i, s])))
        out.append(r)
    return out


def dense(regs, A, V):
    """O.MVReg objects -> (vclk (N, V, A), vval (N, V)) from slot 0 in Vec order; values past V are cut."""
    vc = np.zeros((len(regs), V, A), np.uint64)
    vv = np.zeros((len(regs), V), np.uint64)
    for i, r in enumerate(regs):
        for s, (c, v) in enumerate(r.vals[:V]):
            for a, k in c.dots.items():
                vc[i, s, a] = k
            vv[i, s] = v
    return vc, vv


def actors_of(rng, A, n=4):
    """n of the A actors (all of them when A < n), the last actor always among them."""
    n = min(n, A)
    rest = rng.choice(A - 1, size=n - 1, replace=False) if n > 1 else []
    return np.array(sorted([A - 1] + [int(a) for a in rest]), np.int64)


def arbitrary(rng, N, V, A, fill=0.75, base=0, full=0.0):
    """Arbitrary registers: clocks with counters in 0..3 (plus `base` where non-zero) over 4 of the A
    actors, so many pairs are comparable and a register is no antichain; distinct clocks within a
    register (mvreg.rs:72), distinct values, holes at random slots.  With probability `full` a register
    holds as many values as V and the clocks allow."""
    vc = np.zeros((N, V, A), np.uint64)
    vv = np.zeros((N, V), np.uint64)
    for i in range(N):
        acts = actors_of(rng, A)
        ncode = 4 ** len(acts) - 1
        n = min(V if rng.random() < full else int(round(V * fill * rng.uniform(0.5, 1.0))), ncode)
        codes = rng.choice(ncode, size=n, replace=False) + 1
        slots = np.sort(rng.choice(V, size=n, replace=False))
        for s, code in zip(slots, codes):
            for j, a in enumerate(acts):
                c = (int(code) >> (2 * j)) & 3
                vc[i, s, a] = base + c if c else 0
            vv[i, s] = 1 + i * 1000 + int(s) + (int(rng.integers(1, 1 << 20)) << 20)
    return vc, vv


def antichain(n, lo=0, step=1, base=0):
    """Values lo, lo + step, ... < n of the antichain (i + 1, n - i) over two actors -> [(VClock, val)]."""
    return [(O.VClock({0: base + i + 1, 1: base + n - i}), 100 + i) for i in range(lo, n, step)]


def padded(a, pad, fill=0xDEAD):
    """A device tensor of a's shape whose register stride is `pad` slots' worth wider than the register
    (the padding holds `fill`); returns (view, whole)."""
    a = np.ascontiguousarray(a, np.uint64)
    whole = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], fill, np.uint64)
    whole[:, :a.shape[1]] = a
    t = torch.from_numpy(whole.view(np.int64)).to("cuda:0")
    return t[:, :a.shape[1]], t


def padding_intact(whole, V, fill=0xDEAD):
    torch.cuda.synchronize()
    return bool((whole[:, V:].cpu().numpy().view(np.uint64) == np.uint64(fill)).all())


def merged(svc, svv, ovc, ovv, chunked=False):
    """self[i].merge(other[i]) on the oracle -> the merged O.MVReg objects.  chunked: other's slots
    merged CHUNK at a time instead (what the device must NOT compute)."""
    out = []
    for i, s in enumerate(undense(svc, svv)):
        if chunked:
            for c0 in range(0, ovc.shape[1], CHUNK):
                s.merge(undense(ovc[i:i + 1, c0:c0 + CHUNK], ovv[i:i + 1, c0:c0 + CHUNK])[0])
        else:
            s.merge(undense(ovc[i:i + 1], ovv[i:i + 1])[0])
        out.append(s)
    return out


def vec_lists(regs):
    return [[(tuple(sorted(c.dots.items())), v) for c, v in r.vals] for r in regs]
