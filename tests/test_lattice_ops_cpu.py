"""CPU checks of the lattice types' op streams (LWWReg apply_batch; the VClock / PNCounter / GSet /
LWWReg op wire forms): the byte layout the header states, the test-side codec, the new symbols in the
header, the binding and the built library, the _buf twins, and the wrappers' refusals (no GPU here)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import lattice_ops_util as L
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "crdt_gpu.h")).read()
LIB = os.path.join(ROOT, "rust-crdt_amd", "libcrdt_gpu.so")

NEW = ["crdt_lwwreg_apply_batch"] + [f"crdt_{t}_ops_{d}" for t in ("vclock", "pncounter", "gset", "lwwreg")
                                     for d in ("ingest", "egress")]


def words(b):
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def test_example_frames_of_the_header():
    assert words(L.enc_frame("vclock", [O.Dot(0, 3)], [7])) == [1, 0, 7, 3, 0]
    assert words(L.enc_frame("pncounter", [(O.Dot(0, 3), O.PNCounter.NEG)], [7])) == [1, 0, 7, 3, 0, 1]
    assert words(L.enc_frame("lwwreg", [(10, 2)])) == [1, 0, 10, 0, 2, 0]
    assert words(L.enc_frame("gset", [1], [4, 9])) == [1, 0, 9, 0]
    hdr = " ".join(HEADER.split())
    for text in ("Vec[Dot(7, 3)] = 1 0 | 7 3 0", "Vec[Op { dot: (7, 3), dir: Neg }] = 1 0 | 7 3 0 1",
                 "Vec[LWWReg { val: 10, marker: 2 }] = 1 0 | 10 0 | 2 0"):
        assert text in hdr
    # a frame is 8 + n x rec bytes, exactly
    for kind, op, ids in (("vclock", O.Dot(0, 1), [5]), ("pncounter", (O.Dot(0, 1), O.PNCounter.POS), [5]),
                          ("gset", 0, [5]), ("lwwreg", (1, 2), None)):
        assert len(L.enc_frame(kind, [op] * 3, ids)) == 8 + 3 * L.REC[kind]
        assert len(L.enc_frame(kind, [], ids)) == 8


def test_codec_round_trip_through_sparse_dictionaries():
    rng = np.random.default_rng(5)
    aid, eid = L.sparse_dict(rng, 7, 32), L.sparse_dict(rng, 40, 64)
    assert aid != list(range(7))
    dots = [O.Dot(int(rng.integers(0, 7)), int(rng.integers(1, 1 << 63))) for _ in range(20)] + [O.Dot(6, 2**64 - 1)]
    streams = {
        "vclock": dots,
        "pncounter": [(d, (O.PNCounter.POS, O.PNCounter.NEG)[i % 2]) for i, d in enumerate(dots)],
        "gset": [int(x) for x in rng.integers(0, 40, size=30)],
        "lwwreg": [(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 63))) for _ in range(9)] + [(2**64 - 1, 2**63)],
    }
    ids = {"vclock": aid, "pncounter": aid, "gset": eid, "lwwreg": None}
    for kind, ops in streams.items():
        b = L.enc_frame(kind, ops, ids[kind])
        assert L.dec_frame(kind, b, ids[kind]) == ops
        assert L.enc_frame(kind, L.dec_frame(kind, b, ids[kind]), ids[kind]) == b
        with pytest.raises(AssertionError):
            L.dec_frame(kind, b + b"\0\0\0\0", ids[kind])
    d = L.Dense("pncounter", [streams["pncounter"][:3], [], streams["pncounter"][3:5]])
    assert d.op_off.tolist() == [0, 3, 3, 5] and d.state_idx.tolist() == [0, 0, 0, 2, 2]
    assert d.dir.tolist() == [0, 1, 0, 1, 0] and d.counter[0] == dots[0].counter
    # the ids on the wire are the dictionary's, not the indices
    a, c = struct.unpack_from("<IQ", L.enc_frame("vclock", dots[:1], aid), 8)
    assert a == aid[dots[0].actor] and c == dots[0].counter


def test_replay_reports_the_result_of_every_op():
    reg = O.LWWReg(1, 2)
    assert L.replay_lww(reg, [(2, 1), (2, 2), (1, 2), (2, 3)]) == [0, 1, 0, 0] and reg == O.LWWReg(2, 3)


def test_new_symbols_are_declared_bound_and_exported():
    import crdts_gpu._abi as abi
    declared = set(re.findall(r"\b(crdt_[a-z0-9_]+)\s*\(", HEADER))
    assert os.path.exists(LIB), "build with `make -C rust-crdt_amd`"
    lib = ctypes.CDLL(LIB)
    for name in NEW:
        assert name in declared, name
        assert name in abi.EXPORTS and name in abi._SIGS, name
        assert hasattr(lib, name), name
    assert "crdt_gcounter_ops_ingest" not in declared  # GCounter's Dot streams go through the vclock calls
    assert len(abi._SIGS["crdt_lwwreg_apply_batch"][0]) == 7
    assert len(abi._SIGS["crdt_vclock_ops_ingest"][0]) == len(abi._SIGS["crdt_mvreg_ops_ingest"][0]) == 9
    assert len(abi._SIGS["crdt_gset_ops_egress"][0]) == len(abi._SIGS["crdt_mvreg_ops_egress"][0]) == 10
    assert len(abi._SIGS["crdt_lwwreg_ops_ingest"][0]) == 7 and len(abi._SIGS["crdt_lwwreg_ops_egress"][0]) == 8


def test_abi_revision_is_unchanged():
    import crdts_gpu._abi as abi
    assert abi.CRDT_ABI_VERSION == 8
    assert re.search(r"^#define CRDT_ABI_VERSION 8$", HEADER, flags=re.M)
    lib = ctypes.CDLL(LIB)
    assert lib.crdt_abi_version() == 8


def _c_fields(name):
    import rust_ffi_map as F
    _, structs, _ = F.parse_header(HEADER)
    return dict(structs)[name]


@pytest.mark.parametrize("const,buf", [("DotOps", "DotOpsBuf"), ("LwwRegOps", "LwwRegOpsBuf")])
def test_buf_structs_are_twins(const, buf):
    import crdts_gpu._abi as abi
    c, b = getattr(abi, const), getattr(abi, buf)
    assert ctypes.sizeof(c) == ctypes.sizeof(b) == 8 * len(c._fields_)
    assert [n for n, _ in c._fields_][1:] == [n for n, _ in b._fields_][1:]
    assert c._fields_[0][0] == "n_ops" and b._fields_[0][0] == "op_cap"
    for (cn, _), (bn, _) in zip(c._fields_, b._fields_):
        assert getattr(c, cn).offset == getattr(b, bn).offset and getattr(c, cn).size == getattr(b, bn).size
    # and both are the header's structs, field for field
    cname = {"DotOps": "crdt_dot_ops", "LwwRegOps": "crdt_lwwreg_ops"}[const]
    hc, hb = _c_fields(cname), _c_fields(cname + "_buf")
    assert [n for _, n in hc] == [n for n, _ in c._fields_] and [n for _, n in hb] == [n for n, _ in b._fields_]
    assert [t.replace("const ", "") for t, _ in hc] == [t for t, _ in hb]


# ---- the wrappers' argument checks: ValueError before any library call (no GPU here) ---------------
def _frames():
    return (torch.zeros(8, dtype=torch.uint8), torch.tensor([0, 8], dtype=torch.int64),
            torch.tensor([1], dtype=torch.int32), torch.tensor([1], dtype=torch.int64))


def test_ingest_wrappers_reject_cpu_tensors_dtypes_and_missing_capacities():
    from crdts_gpu import wire
    data, off, actors, elems = _frames()
    calls = [(wire.vclock_ops_ingest, (actors,)), (wire.pncounter_ops_ingest, (actors,)), (wire.gset_ops_ingest, (elems,)),
             (wire.lwwreg_ops_ingest, ())]
    for fn, d in calls:
        with pytest.raises(ValueError, match="cuda"):
            fn(data, off, *d)
        with pytest.raises(ValueError, match="dtype"):
            fn(data, off.to(torch.int32), *d)
        with pytest.raises(ValueError, match="dtype"):
            fn(data.to(torch.int32), off, *d)
        with pytest.raises(ValueError):
            fn(data.numpy(), off, *d)
        with pytest.raises(ValueError, match="caps"):
            fn(data, off, *d, sync=False)
        with pytest.raises(ValueError, match="caps"):
            fn(data, off, *d, sync=False, caps=(1, 1))
        with pytest.raises(ValueError, match="sizing call"):
            fn(data, off, *d, caps=(1,))
    with pytest.raises(ValueError, match="dtype"):
        wire.vclock_ops_ingest(data, off, elems)
    with pytest.raises(ValueError, match="dtype"):
        wire.gset_ops_ingest(data, off, actors)


def test_egress_and_apply_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import lwwreg, wire
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    u8 = lambda *x: torch.tensor(x, dtype=torch.uint8)  # noqa: E731
    db = wire.DotOpBatch(i64(0, 1), i32(0), i32(0), i64(1), u8(0))
    lb = lwwreg.LwwRegOpBatch(i64(0, 1), i64(2), i64(10))
    actors, elems = i32(1, 2), i64(5)
    for fn, d in ((wire.vclock_ops_egress, actors), (wire.pncounter_ops_egress, actors), (wire.gset_ops_egress, elems)):
        with pytest.raises(ValueError, match="cuda"):
            fn(db, d)
        with pytest.raises(ValueError, match="dtype"):
            fn(db._replace(actor=i64(0)), d)
        with pytest.raises(ValueError, match="fields"):
            fn(lb, d)
    with pytest.raises(ValueError, match="dtype"):
        wire.vclock_ops_egress(db._replace(counter=i32(1)), actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.pncounter_ops_egress(db._replace(dir=i32(0)), actors)
    with pytest.raises(ValueError, match="dtype"):
        wire.gset_ops_egress(db, actors)
    with pytest.raises(ValueError, match="cuda"):
        wire.lwwreg_ops_egress(lb)
    with pytest.raises(ValueError, match="fields"):
        wire.lwwreg_ops_egress(db)
    with pytest.raises(ValueError, match="dtype"):
        wire.lwwreg_ops_egress(lb._replace(val=i32(10)))
    m, v = i64(0), i64(0)
    with pytest.raises(ValueError, match="cuda"):
        lwwreg.apply_batch(m, v, lb)
    with pytest.raises(ValueError, match="dtype"):
        lwwreg.apply_batch(m.to(torch.int32), v, lb)
    with pytest.raises(ValueError, match="fields"):
        lwwreg.apply_batch(m, v, db)
    b = lwwreg.encode_ops([[(10, 2), (11, 3)], []], "cpu")
    assert b.op_off.tolist() == [0, 2, 2] and b.marker.tolist() == [2, 3] and b.val.tolist() == [10, 11]
