"""Map<K, MVReg> lub_many with more than 16 values per key: the deep pass (`vstate` = 17..64,
csrc/map_deep.hip).  The first pass marks the keys whose 16-value fold state overflows and the deep
pass folds them again, exactly, with the value state in LDS; expected results are the CPU oracle's
(O.map_fold with 64 output slots and its per-key `peak`), compared as whole arrays.  Every test
asserts on the oracle's peak / nval that its input really passes 16 values."""
import numpy as np
import pytest
import torch

import oracle as O
from gpu_util import to_dev, to_host

pytestmark = pytest.mark.gpu

import crdts_gpu as cg  # noqa: E402
from crdts_gpu import _abi  # noqa: E402


def _empty(R, K, V, A, D=0):
    Kw = (K + 63) // 64
    return dict(clock=np.zeros((R, A), np.uint64), ec=np.zeros((R, K, A), np.uint64),
                vclk=np.zeros((R, K, V, A), np.uint64), vval=np.zeros((R, K, V), np.uint64),
                def_row=np.zeros(D, np.uint64), def_clock=np.zeros((D, A), np.uint64),
                def_keys=np.zeros((D, Kw), np.uint64))


def _write(d, r, k, t, a):
    """Replica r's value slot t of key k is written by actor a alone (counter 1)."""
    d["clock"][r, a] = 1
    d["ec"][r, k, a] = 1
    d["vclk"][r, k, t, a] = 1
    d["vval"][r, k, t] = 1000 * k + 100 * r + t + 1


def _writers(R, V, A, K=3, extra=0):
    """Concurrent writers: replica r holds V values per key, each written by its own actor r*V + t
    (`extra` more all-empty replicas follow for the caller to fill)."""
    d = _empty(R + extra, K, V, A)
    for r in range(R):
        for k in range(K):
            for t in range(V):
                _write(d, r, k, t, r * V + t)
    return d


def _oracle(d):
    K = d["ec"].shape[1]
    peak = np.zeros(K, np.uint64)
    exp = O.map_fold(d["clock"], d["ec"], d["vclk"], d["vval"], d["def_row"], d["def_clock"], d["def_keys"],
                     64, peak=peak)
    return exp, peak.astype(np.int64)


def _gpu(ctx, d, vout, vstate, doff=False):
    D = d["def_clock"].shape[0]
    kw = {}
    if D:
        off = torch.tensor([0, D], dtype=torch.int64, device="cuda:0") if doff else [0, D]
        kw = dict(def_off=off, def_row=torch.from_numpy(d["def_row"].astype(np.int32)).cuda(),
                  def_clock=to_dev(d["def_clock"]), def_keys=to_dev(d["def_keys"]))
    res = cg.map.lub_many(to_dev(d["clock"]), to_dev(d["ec"]), to_dev(d["vclk"]), to_dev(d["vval"]),
                          vout=vout, vstate=vstate, ctx=ctx, **kw)
    return res, kw


def _assert_equal(res, kw, exp, vout):
    """Whole-array equality with the oracle's result cut to `vout` slots (as tests/test_gpu_map.py::_check)."""
    np.testing.assert_array_equal(to_host(res.clock), exp[0])
    np.testing.assert_array_equal(to_host(res.ec), exp[1])
    np.testing.assert_array_equal(to_host(res.vclk), exp[2][:, :vout])
    np.testing.assert_array_equal(to_host(res.vval), exp[3][:, :vout])
    np.testing.assert_array_equal(res.nval.cpu().numpy(), exp[4])
    got = cg.map.deferred_set(kw["def_clock"], res.def_keep, res.def_keys) if kw else set()
    assert got == exp[5]
    assert int(res.flags.cpu().numpy().max()) == 0


def _check(ctx, d, vout, vstate, exp=None, doff=False):
    if exp is None:
        exp, _ = _oracle(d)
    assert int(exp[4].max()) <= vout
    res, kw = _gpu(ctx, d, vout, vstate, doff)
    _assert_equal(res, kw, exp, vout)


def _tuned(spec):
    torch.cuda.set_device(0)
    ctx = cg.Context(0)
    ctx.tune(spec)
    return ctx


@pytest.mark.parametrize("R,V,A", [(17, 1, 17), (3, 6, 24), (32, 1, 32), (4, 8, 32), (8, 8, 64)])
def test_sizes_around_the_caps(gpu_ctx, R, V, A):
    """Just past the old cap (17, 18), config 4's actor count written by every actor (32), and the
    new cap (64): every key folds to R * V values."""
    d = _writers(R, V, A)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [R * V] * 3 and peak.tolist() == [R * V] * 3 and R * V > 16
    _check(gpu_ctx, d, R * V, 64, exp)


def _dominated(R, V, A):
    """R * V = 20 concurrent writers, then one more replica that has seen them all: its clock is 2 on
    actors 0-19, it holds key 0 with one value of that clock, and keys 1 and 2 not at all."""
    assert R * V == 20
    d = _writers(R, V, A, extra=1)
    d["clock"][R, :20] = 2
    d["ec"][R, 0, :20] = 2
    d["vclk"][R, 0, 0, :20] = 2
    d["vval"][R, 0, 0] = 4242
    return d


def test_peak_above_result(gpu_ctx):
    """The state peaks at 20 values although the result has one (or none): vout = 4 is enough."""
    d = _dominated(20, 1, 24)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [1, 0, 0] and peak.tolist() == [20, 20, 20]
    _check(gpu_ctx, d, 4, 32, exp)


@pytest.mark.parametrize("mode", ["mglds=1,mrs=1", "mglds=0"])
def test_peak_above_result_fast_first_pass(mode):
    """The same with V = 2 and A = 32: with vout = 4 the first pass is the LDS-DMA kernel (mglds=1) or
    the register-staged one (mglds=0) with a 4-value state, whatever vstate says."""
    d = _dominated(10, 2, 32)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [1, 0, 0] and peak.tolist() == [20, 20, 20]
    _check(_tuned(mode), d, 4, 32, exp)


@pytest.mark.parametrize("doff", [False, True], ids=["host_def_off", "device_def_off"])
def test_deferred_remove_meets_deep_key(gpu_ctx, doff):
    """A remove held by replica 20 (clock 1 on actors 0-21) names key 1, which holds 21 values by then:
    the deep pass forgets them and folds on; the remove is dominated in the end."""
    d = _writers(24, 1, 24)
    d["def_row"] = np.array([20], np.uint64)
    d["def_clock"] = np.zeros((1, 24), np.uint64)
    d["def_clock"][0, :22] = 1
    d["def_keys"] = np.array([[2]], np.uint64)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [24, 2, 24] and peak.tolist() == [24, 21, 24] and exp[5] == set()
    _check(gpu_ctx, d, 24, 32, exp, doff=doff)


def _antichain(N):
    """A = 2: replica i has clock, entry clock and value clock (i + 1, N - i): N pairwise-concurrent
    values from two actors."""
    d = _empty(N, 1, 1, 2)
    for i in range(N):
        row = np.array([i + 1, N - i], np.uint64)
        d["clock"][i] = d["ec"][i, 0] = d["vclk"][i, 0, 0] = row
        d["vval"][i, 0, 0] = 7 + i
    return d


def test_more_values_than_actors(gpu_ctx):
    d = _antichain(40)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [40] and peak.tolist() == [40]
    _check(gpu_ctx, d, 40, 64, exp)
    # 70 values pass the deep pass's 64 slots as well: flags bit 2, reported
    d = _antichain(70)
    _, peak = _oracle(d)
    assert int(peak[0]) > 64
    with pytest.raises(cg.map.MapCapacityError, match="vstate=64"):
        _gpu(gpu_ctx, d, 64, 64)


def test_only_marked_keys_are_refolded(gpu_ctx):
    """Two groups of 70 keys (two key words).  Group 0: keys 5 and 69 have 20 concurrent writers, every
    other key is written by replica 0 only.  Group 1: the same with 4 writers, nothing to re-fold."""
    R, K, A = 20, 70, 24
    parts = []
    for n in (20, 4):
        d = _empty(R, K, 1, A)
        for r in range(R):
            d["clock"][r, r] = 1
        for k in range(K):
            for r in range(n if k in (5, 69) else 1):
                _write(d, r, k, 0, r)
        parts.append(d)
    exps = [_oracle(p) for p in parts]
    assert sorted(np.flatnonzero(exps[0][1] > 16).tolist()) == [5, 69] and exps[0][0][4][5] == 20
    assert int(exps[1][1].max()) == 4
    st = {k: np.stack([p[k] for p in parts]) for k in ("clock", "ec", "vclk", "vval")}
    res = cg.map.lub_many(to_dev(st["clock"]), to_dev(st["ec"]), to_dev(st["vclk"]), to_dev(st["vval"]),
                          vout=20, vstate=32, ctx=gpu_ctx)
    assert res.flags.cpu().tolist() == [0, 0]
    for g, (exp, _) in enumerate(exps):
        np.testing.assert_array_equal(to_host(res.clock[g]), exp[0])
        np.testing.assert_array_equal(to_host(res.ec[g]), exp[1])
        np.testing.assert_array_equal(to_host(res.vclk[g]), exp[2][:, :20])
        np.testing.assert_array_equal(to_host(res.vval[g]), exp[3][:, :20])
        np.testing.assert_array_equal(res.nval[g].cpu().numpy(), exp[4])


@pytest.mark.parametrize("R,V,A", [(20, 1, 300), (2, 12, 24)])
def test_wide_first_pass(gpu_ctx, R, V, A):
    """The first pass is the workgroup-per-key kernel (A > 256: multi-wave workgroups; V > 8 input
    slots), and marks there."""
    d = _writers(R, V, A)
    exp, peak = _oracle(d)
    assert exp[4].tolist() == [R * V] * 3 and int(peak.min()) > 16
    _check(gpu_ctx, d, R * V, 32, exp)


def test_refusals(gpu_ctx):
    """64 slots of 1,024 actors do not fit the LDS, and 65 slots pass the slot masks: both refused."""
    d = _writers(2, 1, 1024, K=1)
    with pytest.raises(_abi.CrdtGpuError, match="Vstate = 64.*A = 1024") as ei:
        _gpu(gpu_ctx, d, 4, 64)
    assert ei.value.code == _abi.CRDT_EUNSUPPORTED
    d = _writers(2, 1, 8, K=1)
    with pytest.raises(_abi.CrdtGpuError, match="Vstate = 65") as ei:
        _gpu(gpu_ctx, d, 4, 65)
    assert ei.value.code == _abi.CRDT_EUNSUPPORTED
