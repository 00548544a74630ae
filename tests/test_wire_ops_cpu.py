"""CPU checks of the op-stream wire form: the test-side encoder pins the byte layouts the header
documents, decode(encode(x)) == x, and the wrappers reject bad tensors before touching the library."""
import numpy as np
import pytest
import torch

import oracle as O
import wire_ops_util as W
from orswot_apply_util import random_ops

ID = W.identity(64)


def unhex(s):
    return bytes.fromhex(s.replace("|", " ").replace(" ", ""))


def test_orswot_add_layout():
    op = O.OrswotAdd(O.Dot(7, 3), {10})
    want = unhex("01000000 00000000 | 00000000 | 07000000 03000000 00000000 | 01000000 00000000 | 0a000000 00000000")
    assert len(want) == 40 and W.enc_orswot_frame([op], ID, ID) == want


def test_map_up_layout():
    op = O.MapUp(O.Dot(7, 3), 5, O.MVRegPut(O.VClock({7: 2}), 9))
    want = unhex("01000000 00000000 | 01000000 | 07000000 03000000 00000000 | 05000000 | 00000000 | "
                 "01000000 00000000 07000000 02000000 00000000 | 09000000 00000000")
    assert len(want) == 60 and W.enc_map_frame([op], ID, ID) == want


def test_orswot_rm_layout():
    op = O.OrswotRm(O.VClock({7: 2, 9: 1}), {10, 11})
    want = unhex("01000000 00000000 | 01000000 | 02000000 00000000 07000000 02000000 00000000 09000000 01000000 00000000 | "
                 "02000000 00000000 | 0a000000 00000000 0b000000 00000000")
    assert len(want) == 68 and W.enc_orswot_frame([op], ID, ID) == want


def test_map_rm_layout():
    op = O.MapRm(O.VClock({7: 2}), {5, 6})
    want = unhex("01000000 00000000 | 00000000 | 01000000 00000000 07000000 02000000 00000000 | "
                 "02000000 00000000 | 05000000 06000000")
    assert len(want) == 48 and W.enc_map_frame([op], ID, ID) == want


def test_ids_go_through_the_dictionaries():
    aid, mid = [3, 70000, 1 << 31], [5, 1 << 40, (1 << 64) - 1]
    op = O.OrswotAdd(O.Dot(2, 9), {1, 2})
    b = W.enc_orswot_frame([op], aid, mid)
    assert b[12:16] == (1 << 31).to_bytes(4, "little") and b[-8:] == b"\xff" * 8
    assert [W.orswot_key(o) for o in W.dec_orswot_frame(b, aid, mid)] == [W.orswot_key(op)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_orswot_round_trip(seed):
    rng = np.random.default_rng(seed)
    M, A = 40, 9
    aid, mid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, M, 64)
    ops = random_ops(rng, 130, M, A, 8) + [O.OrswotRm(O.VClock(), []), O.OrswotAdd(O.Dot(0, 1), [])]
    assert any(not o.members for o in ops[:130])
    got = W.dec_orswot_frame(W.enc_orswot_frame(ops, aid, mid), aid, mid)
    assert [W.orswot_key(o) for o in got] == [W.orswot_key(o) for o in ops]
    assert W.dec_orswot_frame(W.enc_orswot_frame([], aid, mid), aid, mid) == []


def test_map_round_trip():
    rng = np.random.default_rng(4)
    A, K = 7, 20
    aid, kid = W.sparse_dict(rng, A, 32), W.sparse_dict(rng, K, 32)
    ops = []
    for _ in range(100):
        clk = O.VClock({int(a): int(rng.integers(1, 9)) for a in rng.choice(A, size=int(rng.integers(0, 4)), replace=False)})
        if rng.random() < 0.6:
            ops.append(O.MapUp(O.Dot(int(rng.integers(A)), int(rng.integers(1, 99))), int(rng.integers(K)),
                               O.MVRegPut(clk, int(rng.integers(1, 1 << 60)))))
        else:
            ops.append(O.MapRm(clk, {int(k) for k in rng.choice(K, size=int(rng.integers(0, 4)), replace=False)}))
    assert W.dec_map_frame(W.enc_map_frame(ops, aid, kid), aid, kid) == ops


# ---- the wrappers' argument checks: ValueError before any library call (no GPU here) ---------------
def _frames():
    data = torch.zeros(8, dtype=torch.uint8)
    return data, torch.tensor([0, 8], dtype=torch.int64), torch.tensor([1], dtype=torch.int32)


def test_ingest_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import wire
    data, off, actors = _frames()
    members, keys = torch.tensor([1], dtype=torch.int64), torch.tensor([1], dtype=torch.int32)
    with pytest.raises(ValueError, match="cuda"):
        wire.orswot_ops_ingest(data, off, actors, members)
    with pytest.raises(ValueError, match="cuda"):
        wire.map_ops_ingest(data, off, actors, keys)
    with pytest.raises(ValueError, match="dtype"):
        wire.orswot_ops_ingest(data, off.to(torch.int32), actors, members)
    with pytest.raises(ValueError, match="dtype"):
        wire.orswot_ops_ingest(data, off, actors, members.to(torch.int32))
    with pytest.raises(ValueError, match="dtype"):
        wire.map_ops_ingest(data.to(torch.int32), off, actors, keys)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_ops_ingest(data, off, actors, keys.to(torch.int64))
    with pytest.raises(ValueError):
        wire.orswot_ops_ingest(data.numpy(), off, actors, members)


def test_egress_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import map as cmap, orswot, wire
    A = 2
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    u8 = lambda *x: torch.tensor(x, dtype=torch.uint8)  # noqa: E731
    actors, members, keys = i32(1, 2), i64(5), i32(5)
    ob = orswot.OrswotOpBatch(i64(0, 1), u8(0), i32(0), i64(1), i32(0), torch.zeros((1, A), dtype=torch.int64), i64(0, 1),
                              i32(0))
    mb = cmap.MapOpBatch(i64(0, 1), u8(1), i32(0), i64(0), i32(0), i64(0), i32(0), torch.zeros((1, A), dtype=torch.int64),
                         i64(0, 1), i32(0))
    with pytest.raises(ValueError, match="cuda"):
        wire.orswot_ops_egress(ob, actors, members)
    with pytest.raises(ValueError, match="cuda"):
        wire.map_ops_egress(mb, actors, keys)
    with pytest.raises(ValueError, match="dtype"):
        wire.orswot_ops_egress(ob._replace(kind=i32(0)), actors, members)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_ops_egress(mb._replace(val=i32(0)), actors, keys)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_ops_egress(mb, actors, keys.to(torch.int64))
    with pytest.raises(ValueError, match="fields"):
        wire.orswot_ops_egress(mb, actors, members)


def test_no_sync_path_needs_capacities():
    from crdts_gpu import wire
    data, off, actors = _frames()
    with pytest.raises(ValueError, match="caps"):
        wire.orswot_ops_ingest(data, off, actors, torch.tensor([1], dtype=torch.int64), sync=False)
