"""CPU checks of the value-typed Maps' op wire form: the test-side encoder pins every layout row the
header documents against a word list written by hand from the reference's serde derives (map.rs:50-68,
gcounter.rs:37, pncounter.rs:35-51, orswot.rs:31-47, mvreg.rs:38-47, vclock.rs:32-38),
decode(encode(x)) == x, and the wrappers reject bad tensors before touching the library."""
import struct

import numpy as np
import pytest
import torch

import oracle as O
import wire_vmap_ops_util as V

ID = V.identity(64)
POS, NEG = O.PNCounter.POS, O.PNCounter.NEG


def words(*w):
    return b"".join(struct.pack("<I", x) for x in w)


DOT, KEY = O.Dot(7, 3), 5
LAYOUTS = [  # (kind, op, the frame Vec[op] in 32-bit words after the u64 n_ops = 1)
    ("g", O.MapRm(O.VClock({7: 2}), {5, 6}), (0, 1, 0, 7, 2, 0, 2, 0, 5, 6)),
    ("g", O.MapUp(DOT, KEY, O.Dot(8, 4)), (1, 7, 3, 0, 5, 8, 4, 0)),
    ("pn", O.MapUp(DOT, KEY, (O.Dot(8, 4), POS)), (1, 7, 3, 0, 5, 8, 4, 0, 0)),
    ("pn", O.MapUp(DOT, KEY, (O.Dot(8, 4), NEG)), (1, 7, 3, 0, 5, 8, 4, 0, 1)),
    ("orswot", O.MapUp(DOT, KEY, O.OrswotAdd(O.Dot(8, 4), {10})), (1, 7, 3, 0, 5, 0, 8, 4, 0, 1, 0, 10, 0)),
    ("orswot", O.MapUp(DOT, KEY, O.OrswotRm(O.VClock({7: 2}), {10, 11})),
     (1, 7, 3, 0, 5, 1, 1, 0, 7, 2, 0, 2, 0, 10, 0, 11, 0)),
    ("nested", O.MapUp(DOT, KEY, O.MapRm(O.VClock({7: 2}), {1, 4})), (1, 7, 3, 0, 5, 0, 1, 0, 7, 2, 0, 2, 0, 1, 4)),
    ("nested", O.MapUp(DOT, KEY, O.MapUp(O.Dot(8, 4), 6, O.MVRegPut(O.VClock({7: 2}), 9))),
     (1, 7, 3, 0, 5, 1, 8, 4, 0, 6, 0, 1, 0, 7, 2, 0, 9, 0)),
]
SIZES = [10, 8, 9, 9, 13, 17, 15, 18]  # 5 + 3n + k | 8 | 9 | 9 | 11 + 2k | 10 + 3n + 2k | 10 + 3n + k | 15 + 3n


@pytest.mark.parametrize("ix", range(len(LAYOUTS)))
def test_layout(ix):
    kind, op, w = LAYOUTS[ix]
    assert len(w) == SIZES[ix]
    want = words(1, 0) + words(*w)
    assert V.enc_frame(kind, [op], ID, ID, ID) == want
    (got,) = V.dec_frame(kind, want, ID, ID, ID)
    assert V.op_key(kind, got) == V.op_key(kind, op)


def test_the_rm_is_the_same_for_every_type_and_the_smallest_op():
    rm = O.MapRm(O.VClock(), set())
    frames = {V.enc_frame(k, [rm], ID, ID, ID) for k in V.KINDS}
    assert frames == {words(1, 0, 0, 0, 0, 0, 0)} and len(frames.pop()) == 8 + 20


def test_frame_is_count_then_ops_back_to_back():
    ops = [LAYOUTS[4][1], LAYOUTS[0][1], LAYOUTS[5][1]]
    want = words(3, 0) + words(*LAYOUTS[4][2]) + words(*LAYOUTS[0][2]) + words(*LAYOUTS[5][2])
    assert V.enc_frame("orswot", ops, ID, ID, ID) == want
    assert V.enc_frame("pn", [], ID, ID) == words(0, 0)


def test_ids_go_through_the_dictionaries():
    aid, kid, mid = [3, 70000, 1 << 31], [9, 1 << 30], [5, 1 << 40, (1 << 64) - 1]
    op = O.MapUp(O.Dot(2, 9), 1, O.OrswotAdd(O.Dot(1, 4), {1, 2}))
    b = V.enc_frame("orswot", [op], aid, kid, mid)
    assert b[12:16] == (1 << 31).to_bytes(4, "little") and b[24:28] == (1 << 30).to_bytes(4, "little")
    assert b[32:36] == (70000).to_bytes(4, "little") and b[-8:] == b"\xff" * 8
    assert [V.op_key("orswot", o) for o in V.dec_frame("orswot", b, aid, kid, mid)] == [V.op_key("orswot", op)]


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("seed", [1, 2])
def test_round_trip(kind, seed):
    rng = np.random.default_rng(seed)
    A, K, U = 9, 20, 33
    aid, kid = V.sparse_dict(rng, A, 32), V.sparse_dict(rng, K, 32)
    vid = V.sparse_dict(rng, U, 64 if kind == "orswot" else 32)
    ops = V.random_ops(kind, rng, 150, A, K, U, full=0.1)
    got = V.dec_frame(kind, V.enc_frame(kind, ops, aid, kid, vid), aid, kid, vid)
    assert [V.op_key(kind, o) for o in got] == [V.op_key(kind, o) for o in ops]
    assert {V.op_key(kind, o)[4] for o in ops if isinstance(o, O.MapUp)} >= \
        {"orswot": {"add", "orm"}, "nested": {"put", "irm"}}.get(kind, set())
    assert V.dec_frame(kind, V.enc_frame(kind, [], aid, kid, vid), aid, kid, vid) == []


def test_member_lists_are_kept_as_written():
    op = O.MapUp(DOT, KEY, O.OrswotAdd(O.Dot(8, 4), {1, 2, 3}))
    b = struct.pack("<Q", 1) + V.enc_op("orswot", op, ID, ID, ID, members=[3, 1, 3, 2])
    ops, lists = V.dec_frame("orswot", b, ID, ID, ID, with_lists=True)
    assert lists == [[3, 1, 3, 2]] and V.op_key("orswot", ops[0]) == V.op_key("orswot", op)


def test_tuples_are_what_the_host_encoders_take():
    from crdts_gpu import map as cmap
    for kind, enc in (("g", cmap.encode_counter_ops), ("pn", cmap.encode_counter_ops),
                      ("orswot", cmap.encode_orswot_map_ops), ("nested", cmap.encode_nested_ops)):
        ops = [op for k, op, _ in LAYOUTS if k == kind] + [LAYOUTS[0][1]]
        b = enc([[V.op_tuple(kind, o) for o in ops]], 16, "cpu")
        assert b.kind.tolist() == [int(isinstance(o, O.MapRm)) for o in ops]
        assert b.key_off.tolist()[-1] == sum(len(o.keyset) for o in ops if isinstance(o, O.MapRm))
    assert b.ikind.tolist()[:2] == [1, 0] and b.ikeys.tolist()[0] == (1 << 1) | (1 << 4)


# ---- the wrappers' argument checks: ValueError before any library call (no GPU here) ---------------
def _frames():
    data = torch.zeros(8, dtype=torch.uint8)
    return data, torch.tensor([0, 8], dtype=torch.int64), torch.tensor([1], dtype=torch.int32)


def test_ingest_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import wire
    data, off, actors = _frames()
    keys, members, idict = actors.clone(), torch.tensor([1], dtype=torch.int64), actors.clone()
    calls = [(wire.map_counter_ops_ingest, ()), (wire.map_orswot_ops_ingest, (members,)),
             (wire.map_nested_ops_ingest, (idict,))]
    for fn, extra in calls:
        with pytest.raises(ValueError, match="cuda"):
            fn(data, off, actors, keys, *extra)
        with pytest.raises(ValueError, match="dtype"):
            fn(data, off.to(torch.int32), actors, keys, *extra)
        with pytest.raises(ValueError, match="dtype"):
            fn(data.to(torch.int32), off, actors, keys, *extra)
        with pytest.raises(ValueError, match="dtype"):
            fn(data, off, actors, keys.to(torch.int64), *extra)
        with pytest.raises(ValueError):
            fn(data.numpy(), off, actors, keys, *extra)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_orswot_ops_ingest(data, off, actors, keys, members.to(torch.int32))
    with pytest.raises(ValueError, match="dtype"):
        wire.map_nested_ops_ingest(data, off, actors, keys, idict.to(torch.int64))


def test_egress_wrappers_reject_cpu_tensors_and_dtypes():
    from crdts_gpu import map as cmap, wire
    A = 2
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    u8 = lambda *x: torch.tensor(x, dtype=torch.uint8)  # noqa: E731
    pool = torch.zeros((1, A), dtype=torch.int64)
    actors, keys, members, idict = i32(1, 2), i32(5), i64(5), i32(7)
    cb = cmap.MapCounterOpBatch(i64(0, 1), u8(0), i32(0), i64(1), i32(0), i32(0), i64(1), u8(0), i32(0), pool, i64(0, 0),
                                i32(0))
    ob = cmap.MapOrswotOpBatch(i64(0, 1), u8(0), i32(0), i64(1), i32(0), u8(0), i32(0), i64(1), i32(0), pool, i64(0, 0),
                               i32(0), i64(0, 1), i32(0))
    nb = cmap.MapNestedOpBatch(i64(0, 1), u8(0), i32(0), i64(1), i32(0), u8(0), i32(0), i64(1), i32(0), i64(9), i64(0),
                               i32(0), pool, i64(0, 0), i32(0))
    with pytest.raises(ValueError, match="cuda"):
        wire.map_counter_ops_egress(cb, actors, keys)
    with pytest.raises(ValueError, match="cuda"):
        wire.map_orswot_ops_egress(ob, actors, keys, members)
    with pytest.raises(ValueError, match="cuda"):
        wire.map_nested_ops_egress(nb, actors, keys, idict)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_counter_ops_egress(cb._replace(vdir=i32(0)), actors, keys)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_orswot_ops_egress(ob._replace(vcounter=i32(0)), actors, keys, members)
    with pytest.raises(ValueError, match="dtype"):
        wire.map_orswot_ops_egress(ob, actors, keys, members.to(torch.int32))
    with pytest.raises(ValueError, match="dtype"):
        wire.map_nested_ops_egress(nb._replace(ikeys=i32(0)), actors, keys, idict)
    with pytest.raises(ValueError, match="fields"):
        wire.map_counter_ops_egress(ob, actors, keys)
    with pytest.raises(ValueError, match="fields"):
        wire.map_nested_ops_egress(cb, actors, keys, idict)


def test_no_sync_path_needs_capacities():
    from crdts_gpu import wire
    data, off, actors = _frames()
    with pytest.raises(ValueError, match="caps"):
        wire.map_counter_ops_ingest(data, off, actors, actors, sync=False)
    with pytest.raises(ValueError, match="caps"):
        wire.map_orswot_ops_ingest(data, off, actors, actors, torch.tensor([1], dtype=torch.int64), sync=False,
                                   caps=(1, 1, 1))  # the Orswot Map has four
    with pytest.raises(ValueError, match="caps"):
        wire.map_nested_ops_ingest(data, off, actors, actors, actors, sync=False, caps=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="sizing call"):
        wire.map_counter_ops_ingest(data, off, actors, actors, caps=(1, 1, 1))  # sync=True sizes by itself
