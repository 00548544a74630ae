"""CPU checks of the standalone MVReg surface (crdt_mvreg_forget_batch, crdt_mvreg_ingest / _egress,
crdt_mvreg_ops_ingest / _ops_egress): the test-side encoder pins the byte layouts the header
documents, decode(encode(x)) == x, the five entry points are declared, bound and exported, and the
wrappers reject bad tensors before touching the library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
import wire_mvreg_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crdt_mvreg_forget_batch", "crdt_mvreg_ingest", "crdt_mvreg_egress", "crdt_mvreg_ops_ingest",
         "crdt_mvreg_ops_egress")
ID = W.identity(64)


def unhex(s):
    return bytes.fromhex(s.replace("|", " ").replace(" ", ""))


def test_register_layout():
    reg = O.MVReg([(O.VClock({7: 3}), 10)])
    want = unhex("01000000 00000000 | 01000000 00000000 | 07000000 03000000 00000000 | 0a000000 00000000")
    assert len(want) == 36 and W.enc_reg(reg, ID) == want
    assert np.frombuffer(want, "<u4").tolist() == [1, 0, 1, 0, 7, 3, 0, 10, 0]


def test_put_frame_layout():
    op = O.MVRegPut(O.VClock({7: 3}), 10)
    want = unhex("01000000 00000000 | 00000000 | 01000000 00000000 | 07000000 03000000 00000000 | 0a000000 00000000")
    assert len(want) == 40 and W.enc_ops([op], ID) == want
    assert np.frombuffer(want, "<u4").tolist() == [1, 0, 0, 1, 0, 7, 3, 0, 10, 0]
    # the smallest op, a Put with an empty clock, is the 20 bytes the sizing bound divides by
    assert len(W.enc_put(O.MVRegPut(O.VClock(), 1), ID)) == 20 and W.enc_ops([], ID) == bytes(8)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_round_trips_through_a_sparse_dictionary(seed):
    rng = np.random.default_rng(seed)
    A = 9
    aid = W.sparse_dict(rng, A, 32)
    assert aid != list(range(A))
    for _ in range(40):
        reg, ops = W.replay(rng, A, 5, 4, int(rng.integers(0, 12)))
        ops = ops + [O.MVRegPut(O.VClock(), 5)]  # an empty-clock Put is a valid op
        assert W.dec_reg(W.enc_reg(reg, aid), aid).vals == reg.vals
        assert W.dec_ops(W.enc_ops(ops, aid), aid) == ops
        vc, vv = W.dense([reg], A, 4)
        assert W.undense(vc, vv)[0].vals == reg.vals
    b = W.enc_reg(O.MVReg([(O.VClock({8: (1 << 64) - 1}), (1 << 64) - 1)]), aid)
    assert b[16:20] == int(aid[8]).to_bytes(4, "little") and b[-8:] == b"\xff" * 8 and b[20:28] == b"\xff" * 8


def test_declared_bound_and_exported():
    import crdts_gpu._abi as abi
    header = open(os.path.join(ROOT, "include", "crdt_gpu.h")).read()
    declared = set(re.findall(r"^int (crdt_\w+)\(", header, flags=re.M))
    assert os.path.exists(abi.LIB_PATH), "build with `make -C rust-crdt_amd`"
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert name in abi._SIGS and name in abi.EXPORTS, name
        assert hasattr(lib, name), name
    assert "typedef struct crdt_mvreg_ops_buf" in header


def test_ops_buf_is_the_twin_of_ops():
    import crdts_gpu._abi as abi
    assert ctypes.sizeof(abi.MVRegOpsBuf) == ctypes.sizeof(abi.MVRegOps) == 6 * 8
    for (a, _), (b, _) in zip(abi.MVRegOpsBuf._fields_, abi.MVRegOps._fields_):
        assert getattr(abi.MVRegOpsBuf, a).offset == getattr(abi.MVRegOps, b).offset
    assert [n for n, _ in abi.MVRegOpsBuf._fields_] == ["op_cap", "op_off", "clk_row", "clk_pool", "row_cap", "val"]


# ---- the wrappers' argument checks: ValueError before any library call (no GPU here) ---------------
def _frames():
    data = torch.zeros(8, dtype=torch.uint8)
    return data, torch.tensor([0, 8], dtype=torch.int64), torch.tensor([1], dtype=torch.int32)


def test_wire_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import mvreg, wire
    data, off, actors = _frames()
    for fn in (lambda *a: wire.mvreg_ingest(*a, 4), wire.mvreg_ops_ingest):
        with pytest.raises(ValueError, match="cuda"):
            fn(data, off, actors)
        with pytest.raises(ValueError, match="dtype"):
            fn(data, off.to(torch.int32), actors)
        with pytest.raises(ValueError, match="dtype"):
            fn(data.to(torch.int32), off, actors)
        with pytest.raises(ValueError, match="dtype"):
            fn(data, off, actors.to(torch.int64))
        with pytest.raises(ValueError):
            fn(data.numpy(), off, actors)
    vclk, vval = torch.zeros((1, 2, 1), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="cuda"):
        wire.mvreg_egress(vclk, vval, actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.mvreg_egress(vclk.to(torch.int32), vval, actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.mvreg_egress(vclk, vval, actors.to(torch.int64))
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    ob = mvreg.MVRegOpBatch(i64(0, 1), i32(0), torch.zeros((1, 1), dtype=torch.int64), i64(7))
    with pytest.raises(ValueError, match="cuda"):
        wire.mvreg_ops_egress(ob, actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.mvreg_ops_egress(ob._replace(val=i32(7)), actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.mvreg_ops_egress(ob._replace(clk_row=i64(0)), actors)
    with pytest.raises(ValueError, match="fields"):
        wire.mvreg_ops_egress((ob.op_off, ob.val), actors)


def test_forget_wrapper_rejects_cpu_tensors_and_dtypes():
    from crdts_gpu import mvreg
    vclk, vval = torch.zeros((1, 2, 3), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int64)
    y = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="cuda"):
        mvreg.forget_batch(vclk, vval, y)
    with pytest.raises(ValueError, match="dtype"):
        mvreg.forget_batch(vclk, vval, y.to(torch.int32))
    with pytest.raises(ValueError, match="dtype"):
        mvreg.forget_batch(vclk.to(torch.float64), vval, y)


def test_no_sync_path_needs_capacities():
    from crdts_gpu import wire
    data, off, actors = _frames()
    with pytest.raises(ValueError, match="caps"):
        wire.mvreg_ops_ingest(data, off, actors, sync=False)
    with pytest.raises(ValueError, match="caps"):
        wire.mvreg_ops_ingest(data, off, actors, sync=False, caps=(1, 2, 3))
    with pytest.raises(ValueError, match="sizing"):
        wire.mvreg_ops_ingest(data, off, actors, sync=True, caps=(1, 1))
