"""mvreg.lub_many with more than 16 values in a register: the deep pass (`vstate` = 17..64, the LDS
register of csrc/mvreg_lds.hpp).  Expected results are O.MVReg.merge folded in replica order, compared
value by value in Vec order; every test asserts that the oracle's fold really passes 16 values."""
import numpy as np
import pytest

import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi  # noqa: E402


def _fold(vclk, vval):
    """O.MVReg.merge over the replicas (vclk (R, V, A), vval (R, V)) in order -> dense (n, A), (n,)."""
    acc = O.MVReg()
    for r in range(vclk.shape[0]):
        vals = [(O.VClock({a: int(x) for a, x in enumerate(vclk[r, s]) if x}), int(vval[r, s]))
                for s in range(vclk.shape[1]) if vclk[r, s].any()]
        acc.merge(O.MVReg(vals))
    n, A = len(acc.vals), vclk.shape[2]
    oc, ov = np.zeros((n, A), np.uint64), np.zeros(n, np.uint64)
    for s, (c, v) in enumerate(acc.vals):
        for a, k in c.dots.items():
            oc[s, a] = k
        ov[s] = v
    return oc, ov


def _writers(R):
    """R concurrent writers: replica r's one value is written by actor r alone."""
    vc = np.zeros((R, 1, R), np.uint64)
    vv = np.zeros((R, 1), np.uint64)
    for r in range(R):
        vc[r, 0, r] = 1
        vv[r, 0] = 100 + r
    return vc, vv


def _check(vc, vv, vout, vstate, n):
    oc, ov = _fold(vc, vv)
    assert oc.shape[0] == n and n > 16
    res = cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=vout, vstate=vstate)
    assert int(res.nval.cpu()[0]) == n and int(res.flags.cpu()[0]) == 0
    exp_c = np.zeros((vout, vc.shape[2]), np.uint64)
    exp_v = np.zeros(vout, np.uint64)
    exp_c[:n], exp_v[:n] = oc, ov
    np.testing.assert_array_equal(to_host(res.vclk), exp_c)
    np.testing.assert_array_equal(to_host(res.vval), exp_v)


@pytest.mark.parametrize("R", [17, 32, 64])
def test_concurrent_writers(gpu_ctx, R):
    vc, vv = _writers(R)
    _check(vc, vv, R, 64, R)


def test_more_values_than_actors(gpu_ctx):
    """A = 2: value clocks (i + 1, N - i) are pairwise concurrent, 40 values from two actors."""
    N = 40
    vc = np.zeros((N, 1, 2), np.uint64)
    vv = np.zeros((N, 1), np.uint64)
    for i in range(N):
        vc[i, 0] = (i + 1, N - i)
        vv[i, 0] = 7 + i
    _check(vc, vv, 64, 64, N)


def test_default_state_still_reports(gpu_ctx):
    """Without the opt-in nothing changes: 17 writers raise with vout = 16, and vout = 17 is refused."""
    vc, vv = _writers(17)
    assert _fold(vc, vv)[0].shape[0] == 17
    with pytest.raises(cg.mvreg.MVRegCapacityError):
        cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=16)
    with pytest.raises(_abi.CrdtGpuError) as ei:
        cg.mvreg.lub_many(to_dev(vc), to_dev(vv), vout=17)
    assert ei.value.code == _abi.CRDT_EUNSUPPORTED
