"""Serde wire format ingest / egress on the device (include/crdt_gpu.h "serde wire format").

Replicas ship whole serialized states; these calls turn a batch of received frames (the bytes
`bincode::serialize` writes for VClock / GCounter / PNCounter<u32>, GSet<u64>, LWWReg<u64, u64>,
Orswot<u64, u32>) into the dense layout the merge kernels read, and merged dense states back into
frames.  Every tensor is a device tensor: bytes (uint8), frame offsets (int64, N+1, 4-byte
aligned), dictionaries (sorted ascending: actors int32 holding u32 ids, members / elements int64
holding u64 ids).  Nothing here runs on the host except the shape checks.

    rows, status = vclock_ingest(bytes, frame_off, actors)          # (N, A), (N,) int32
    frame_off, data = vclock_egress(rows, actors)                   # (N+1,), (total,) uint8

Op streams travel the same way (one Vec<Op> frame per state, Orswot<u64, u32> and
Map<u32, MVReg<u64, u32>, u32>): orswot_ops_ingest / map_ops_ingest return the OrswotOpBatch /
MapOpBatch that orswot.apply_batch / map.apply_batch take, orswot_ops_egress / map_ops_egress write
such a batch as frames.  The value-typed Maps (Map<u32, GCounter / PNCounter / Orswot<u64, u32> /
Map<u32, MVReg<u64, u32>, u32>, u32>) have map_counter_ops_ingest / map_orswot_ops_ingest /
map_nested_ops_ingest and the three *_ops_egress twins, over the batches map.counter_apply_batch /
orswot_apply_batch / nested_apply_batch take.

MVReg<u64, u32> on its own: mvreg_ingest / mvreg_egress move register frames to and from the dense
(vclk, vval) of mvreg.py, mvreg_ops_ingest / mvreg_ops_egress Vec<mvreg::Op> frames to and from the
MVRegOpBatch mvreg.apply_batch takes.

The lattice types' ops are fixed-width records: vclock_ops_ingest (VClock and GCounter: Vec<Dot<u32>>),
pncounter_ops_ingest, gset_ops_ingest and lwwreg_ops_ingest return the arrays apply.apply_dots /
apply.apply_inserts / lwwreg.apply_batch take; the four *_ops_egress twins write them back as frames.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _abi
from .context import Context, dptr

BAD, MISSING, CAP = 1, 2, 4  # status bits


def _ctx(t: torch.Tensor, ctx: Optional[Context]) -> Context:
    return ctx or Context.default(t.device.index)


def _frames(ctx, data, frame_off, what):
    ctx.check_tensor(data, f"{what}(bytes)", (torch.uint8,))
    ctx.check_tensor(frame_off, f"{what}(frame_off)")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError(f"{what}: bytes must be a contiguous uint8 vector")
    if frame_off.dtype != torch.int64 or frame_off.dim() != 1 or not frame_off.is_contiguous() or frame_off.shape[0] < 1:
        raise ValueError(f"{what}: frame_off must be a contiguous int64 (N+1,) tensor")
    return frame_off.shape[0] - 1


def _dict(ctx, d, dt, what):
    ctx.check_tensor(d, what, (dt,))
    if d.dtype != dt or d.dim() != 1 or not d.is_contiguous() or d.shape[0] == 0:
        raise ValueError(f"{what}: a non-empty contiguous {dt} dictionary is required")
    return d.shape[0]


def _status(N, dev):
    return torch.zeros(N, dtype=torch.int32, device=dev)


def _ptr_or_dummy(data):
    return dptr(data) if data.numel() else None


def vclock_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, out: Optional[torch.Tensor] = None,
                  ctx: Optional[Context] = None, _fn: str = "crdt_vclock_ingest", _k: int = 1):
    """VClock / GCounter frames -> (rows (N, A) int64, status (N,) int32)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.vclock_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.vclock_ingest(actors)")
    if out is None:
        out = torch.empty((N, _k * A), dtype=torch.int64, device=data.device)
    if out.dim() != 2 or out.shape[0] != N or out.shape[1] < _k * A or out.stride(1) != 1:
        raise ValueError(f"wire ingest: out must be ({N}, >= {_k * A}) with contiguous rows")
    st = _status(N, data.device)
    ctx.call(_fn, _ptr_or_dummy(data), dptr(frame_off), N, dptr(actors), A, dptr(out), out.stride(0), dptr(st))
    return out, st


def pncounter_ingest(data, frame_off, actors, out=None, ctx=None):
    """PNCounter frames (p then n) -> (rows (N, 2A) = P | N, status)."""
    return vclock_ingest(data, frame_off, actors, out, ctx, "crdt_pncounter_ingest", 2)


def gset_ingest(data: torch.Tensor, frame_off: torch.Tensor, elems: torch.Tensor, out: Optional[torch.Tensor] = None,
                ctx: Optional[Context] = None):
    """GSet<u64> frames -> (bitmap rows (N, ceil(U/64)), status)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.gset_ingest")
    U = _dict(ctx, elems, torch.int64, "wire.gset_ingest(elems)")
    W = (U + 63) // 64
    if out is None:
        out = torch.empty((N, W), dtype=torch.int64, device=data.device)
    st = _status(N, data.device)
    ctx.call("crdt_gset_ingest", _ptr_or_dummy(data), dptr(frame_off), N, dptr(elems), U, dptr(out), out.stride(0),
             dptr(st))
    return out, st


def lwwreg_ingest(data: torch.Tensor, frame_off: torch.Tensor, ctx: Optional[Context] = None):
    """LWWReg<u64, u64> frames -> (marker (N,), val (N,), status)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.lwwreg_ingest")
    m = torch.empty(N, dtype=torch.int64, device=data.device)
    v = torch.empty_like(m)
    st = _status(N, data.device)
    ctx.call("crdt_lwwreg_ingest", _ptr_or_dummy(data), dptr(frame_off), N, dptr(m), dptr(v), dptr(st))
    return m, v, st


class OrswotFrames(NamedTuple):
    clock: torch.Tensor        # (N, A)
    entries: torch.Tensor      # (N, M, A)
    def_off: torch.Tensor      # (N+1,) int64, device: state s owns removes [def_off[s], def_off[s+1])
    def_clock: torch.Tensor    # (D, A)
    def_members: torch.Tensor  # (D, ceil(M/64))
    status: torch.Tensor       # (N,) int32


def orswot_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, members: torch.Tensor,
                  def_cap: Optional[int] = None, ctx: Optional[Context] = None) -> OrswotFrames:
    """Orswot<u64, u32> frames -> dense states + the deferred removes pooled in state order."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.orswot_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.orswot_ingest(actors)")
    M = _dict(ctx, members, torch.int64, "wire.orswot_ingest(members)")
    Mw = (M + 63) // 64
    dev = data.device
    clock = torch.empty((N, A), dtype=torch.int64, device=dev)
    entries = torch.empty((N, M, A), dtype=torch.int64, device=dev)
    def_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
    cap = def_cap if def_cap is not None else max(1, N)
    dcl = torch.empty((cap, A), dtype=torch.int64, device=dev)
    dmb = torch.empty((cap, Mw), dtype=torch.int64, device=dev)
    st = _status(N, dev)
    nd = ctypes.c_size_t()
    ctx.call("crdt_orswot_ingest", _ptr_or_dummy(data), dptr(frame_off), N, dptr(actors), A, dptr(members), M,
             dptr(clock), dptr(entries), dptr(def_off), dptr(dcl), dptr(dmb), cap, ctypes.byref(nd), dptr(st))
    D = nd.value
    if D > cap and def_cap is None:  # more removes than guessed: once more with exactly enough room
        return orswot_ingest(data, frame_off, actors, members, def_cap=D, ctx=ctx)
    return OrswotFrames(clock, entries, def_off, dcl[:min(D, cap)], dmb[:min(D, cap)], st)


def _egress(ctx, fn, N, dev, *args, with_status=False):
    """The two calls of every egress: the sizing call, the allocation, the write call ->
    (frame_off, bytes), and with_status (the op streams) the (N,) int32 status the calls fill.
    frame_off starts zeroed: the C calls return at N == 0 without writing it."""
    frame_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    total = ctypes.c_size_t()
    status = torch.empty(N, dtype=torch.int32, device=dev) if with_status else None
    tail = (ctypes.byref(total),) + ((dptr(status),) if with_status else ())
    ctx.call(fn, *args, dptr(frame_off), None, 0, *tail)
    data = torch.empty(max(total.value, 1), dtype=torch.uint8, device=dev)
    ctx.call(fn, *args, dptr(frame_off), dptr(data), data.numel(), *tail)
    return (frame_off, data[:total.value]) + ((status,) if with_status else ())


def vclock_egress(rows: torch.Tensor, actors: torch.Tensor, ctx: Optional[Context] = None, _fn="crdt_vclock_egress",
                  _k: int = 1):
    """Dense rows (N, A) -> (frame_off (N+1,), bytes) of VClock / GCounter frames."""
    ctx = _ctx(rows, ctx)
    ctx.check_tensor(rows, "wire.vclock_egress(rows)")
    A = _dict(ctx, actors, torch.int32, "wire.vclock_egress(actors)")
    if rows.dim() != 2 or rows.shape[1] < _k * A or rows.stride(1) != 1:
        raise ValueError(f"wire egress: rows must be (N, >= {_k * A}) with contiguous rows")
    N = rows.shape[0]
    return _egress(ctx, _fn, N, rows.device, dptr(rows), N, A, rows.stride(0), dptr(actors))


def pncounter_egress(rows, actors, ctx=None):
    return vclock_egress(rows, actors, ctx, "crdt_pncounter_egress", 2)


def gset_egress(rows: torch.Tensor, elems: torch.Tensor, ctx: Optional[Context] = None):
    ctx = _ctx(rows, ctx)
    ctx.check_tensor(rows, "wire.gset_egress(rows)")
    U = _dict(ctx, elems, torch.int64, "wire.gset_egress(elems)")
    if rows.dim() != 2 or rows.shape[1] < (U + 63) // 64 or rows.stride(1) != 1:
        raise ValueError("wire.gset_egress: rows must be (N, >= ceil(U/64))")
    N = rows.shape[0]
    return _egress(ctx, "crdt_gset_egress", N, rows.device, dptr(rows), N, U, rows.stride(0), dptr(elems))


def lwwreg_egress(marker: torch.Tensor, val: torch.Tensor, ctx: Optional[Context] = None):
    ctx = _ctx(marker, ctx)
    N = marker.shape[0]
    data = torch.empty(max(16 * N, 1), dtype=torch.uint8, device=marker.device)
    ctx.call("crdt_lwwreg_egress", dptr(marker.contiguous()), dptr(val.contiguous()), N, dptr(data))
    off = torch.arange(0, 16 * (N + 1), 16, dtype=torch.int64, device=marker.device)
    return off, data[:16 * N]


def orswot_egress(clock: torch.Tensor, entries: torch.Tensor, actors: torch.Tensor, members: torch.Tensor,
                  def_off: Optional[torch.Tensor] = None, def_clock: Optional[torch.Tensor] = None,
                  def_members: Optional[torch.Tensor] = None, def_keep: Optional[torch.Tensor] = None,
                  ctx: Optional[Context] = None):
    """Dense Orswot states (clock (N, A), entries (N, M, A)) + removes pooled by state (device
    def_off (N+1,), def_clock, def_members, def_keep or None) -> (frame_off, bytes)."""
    ctx = _ctx(clock, ctx)
    A = _dict(ctx, actors, torch.int32, "wire.orswot_egress(actors)")
    M = _dict(ctx, members, torch.int64, "wire.orswot_egress(members)")
    N = clock.shape[0]
    if tuple(clock.shape) != (N, A) or tuple(entries.shape) != (N, M, A) or not clock.is_contiguous() \
            or not entries.is_contiguous():
        raise ValueError("wire.orswot_egress: clock (N, A) and entries (N, M, A), contiguous")
    dp = [None, None, None, None]
    if def_off is not None:
        dp = [dptr(def_off), dptr(def_clock), dptr(def_members), dptr(def_keep) if def_keep is not None else None]
    return _egress(ctx, "crdt_orswot_egress", N, clock.device, dptr(clock), dptr(entries), N, M, A, dptr(actors),
                   dptr(members), *dp)


def map_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor, V: int,
               Dcap: int, ctx: Optional[Context] = None):
    """Map<u32, MVReg<u64>> frames -> (map.MapStates with V value slots per key and Dcap deferred
    slots per state, status (N,) int32).  keys: sorted u32 key dictionary (int32 tensor)."""
    from .map import MapStates, _map_states_structs
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.map_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.map_ingest(actors)")
    K = _dict(ctx, keys, torch.int32, "wire.map_ingest(keys)")
    dev = data.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
    st = MapStates(z(N, A), z(N, K, A), z(N, K, V, A), z(N, K, V), z(N, max(Dcap, 0), A), z(N, max(Dcap, 0), (K + 63) // 64),
                   torch.zeros(N, dtype=torch.int32, device=dev))
    s, d = _map_states_structs(ctx, st, "wire.map_ingest")
    status = _status(N, dev)
    ctx.call("crdt_map_ingest", _ptr_or_dummy(data), dptr(frame_off), dptr(actors), dptr(keys), ctypes.byref(s),
             ctypes.byref(d), dptr(status))
    return st, status


def map_egress(states, actors: torch.Tensor, keys: torch.Tensor, ctx: Optional[Context] = None):
    """map.MapStates (packed per-state blocks, deferred slots) -> (frame_off (N+1,), bytes)."""
    from .map import _map_states_structs
    ctx = _ctx(states.clock, ctx)
    _dict(ctx, actors, torch.int32, "wire.map_egress(actors)")
    _dict(ctx, keys, torch.int32, "wire.map_egress(keys)")
    s, d = _map_states_structs(ctx, states, "wire.map_egress")
    return _egress(ctx, "crdt_map_egress", states.clock.shape[0], states.clock.device, ctypes.byref(s), ctypes.byref(d),
                   dptr(actors), dptr(keys))


# ---- the value-typed Maps (round 5) ---------------------------------------------------------------
class MapCounterFrames(NamedTuple):
    """Map<u32, GCounter / PNCounter> states in the crdt_map_counter_states layout + deferred slots."""
    clock: torch.Tensor      # (N, A)
    ec: torch.Tensor         # (N, K, A)
    val: torch.Tensor        # (N, K, W, A)
    def_clock: torch.Tensor  # (N, Dcap, A)
    def_keys: torch.Tensor   # (N, Dcap, Kw)
    def_count: torch.Tensor  # (N,) int32


class MapOrswotFrames(NamedTuple):
    """Map<u32, Orswot<u64>> states in the crdt_map_orswot_states layout (the field names of
    map.MapOrswotLub, so map.orswot_apply_batch / orswot_forget_batch take it) + deferred slots."""
    clock: torch.Tensor      # (N, A)
    ec: torch.Tensor         # (N, K, A)
    oc: torch.Tensor         # (N, K, A)
    ent: torch.Tensor        # (N, K, M, A)
    vd_n: torch.Tensor       # (N, K) int32
    vd_clock: torch.Tensor   # (N, K, Vd, A)  (Vd nested slots per key, 16 by default)
    vd_mem: torch.Tensor     # (N, K, Vd) member bitmasks ((N, K, Vd, Mw) past M = 64)
    def_clock: torch.Tensor  # (N, Dcap, A)
    def_keys: torch.Tensor   # (N, Dcap, Kw)
    def_count: torch.Tensor  # (N,) int32


class MapNestedFrames(NamedTuple):
    """Map<u32, Map<u32, MVReg<u64>>> states in the crdt_map_nested_states layout (the field names of
    map.MapNestedLub, so map.nested_apply_batch / nested_forget_batch take it) + deferred slots."""
    clock: torch.Tensor      # (N, A)
    ec: torch.Tensor         # (N, K, A)
    ic: torch.Tensor         # (N, K, A)
    iec: torch.Tensor        # (N, K, K2, A)
    ivc: torch.Tensor        # (N, K, K2, Vs, A)  (Vs MVReg slots per inner key, 8 by default)
    ivv: torch.Tensor        # (N, K, K2, Vs)
    nval: torch.Tensor       # (N, K, K2) int32
    id_n: torch.Tensor       # (N, K) int32
    id_clock: torch.Tensor   # (N, K, Id, A)  (Id inner deferred slots per key, 16 by default)
    id_keys: torch.Tensor    # (N, K, 16) ((N, K, 16, K2w) mask words past K2 = 64)
    def_clock: torch.Tensor  # (N, Dcap, A)
    def_keys: torch.Tensor   # (N, Dcap, Kw)
    def_count: torch.Tensor  # (N,) int32


def _vmap_deferred(st):
    from . import _abi
    d = _abi.MapDeferred()
    Dcap = st.def_clock.shape[1]
    d.clock = dptr(st.def_clock) if Dcap else None
    d.keys = dptr(st.def_keys) if Dcap else None
    d.count = dptr(st.def_count)
    d.Dcap = Dcap
    return d


def _vmap_check(ctx, st, what):
    for nm, t in st._asdict().items():
        ctx.check_tensor(t, f"{what}({nm})", (torch.int32,) if nm in ("vd_n", "def_count", "nval", "id_n") else None)
        if not t.is_contiguous():
            raise ValueError(f"{what}: {nm} must be contiguous")
    N, A = st.clock.shape
    Dcap = st.def_clock.shape[1]
    K = st.ec.shape[1]
    if tuple(st.def_clock.shape) != (N, Dcap, A) or tuple(st.def_keys.shape) != (N, Dcap, (K + 63) // 64) \
            or tuple(st.def_count.shape) != (N,) or st.def_count.dtype != torch.int32:
        raise ValueError(f"{what}: deferred slots must be (N, Dcap, A), (N, Dcap, ceil(K/64)), (N,) int32")
    return N, K, A


def _counter_struct(ctx, st, what):
    from . import _abi
    N, K, A = _vmap_check(ctx, st, what)
    W = st.val.shape[2]
    if tuple(st.ec.shape) != (N, K, A) or tuple(st.val.shape) != (N, K, W, A) or W not in (1, 2):
        raise ValueError(f"{what}: clock (N, A), ec (N, K, A), val (N, K, W, A) with W = 1 or 2 expected")
    s = _abi.MapCounterStates()
    s.N, s.K, s.A, s.W = N, K, A, W
    s.clock, s.clock_stride = dptr(st.clock), A
    s.ec, s.ec_stride = dptr(st.ec), K * A
    s.val, s.val_stride = dptr(st.val), K * W * A
    return s, _vmap_deferred(st)


def _orswot_struct(ctx, st, what):
    from . import _abi
    N, K, A = _vmap_check(ctx, st, what)
    M = st.ent.shape[2]
    Mw = (M + 63) // 64
    Vd = st.vd_clock.shape[2] if st.vd_clock.dim() == 4 else 0
    vm = (N, K, Vd) if Mw == 1 else (N, K, Vd, Mw)
    if (tuple(st.oc.shape) != (N, K, A) or tuple(st.ent.shape) != (N, K, M, A) or tuple(st.vd_n.shape) != (N, K)
            or Vd < 16 or tuple(st.vd_clock.shape) != (N, K, Vd, A) or tuple(st.vd_mem.shape) != vm):
        raise ValueError(f"{what}: the crdt_map_orswot_states shapes expected")
    s = _abi.MapOrswotStates()
    s.N, s.K, s.M, s.A, s.Vd = N, K, M, A, Vd
    s.clock, s.ec, s.oc, s.ent = dptr(st.clock), dptr(st.ec), dptr(st.oc), dptr(st.ent)
    s.vd_n, s.vd_clock, s.vd_mem = dptr(st.vd_n), dptr(st.vd_clock), dptr(st.vd_mem)
    return s, _vmap_deferred(st)


def map_counter_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                       W: int, Dcap: int, ctx: Optional[Context] = None):
    """Map<u32, GCounter<u32>> (W = 1) / Map<u32, PNCounter<u32>> (W = 2) frames ->
    (MapCounterFrames, status (N,) int32); keys: sorted u32 key dictionary (int32 tensor)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.map_counter_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.map_counter_ingest(actors)")
    K = _dict(ctx, keys, torch.int32, "wire.map_counter_ingest(keys)")
    dev = data.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
    st = MapCounterFrames(z(N, A), z(N, K, A), z(N, K, W, A), z(N, Dcap, A), z(N, Dcap, (K + 63) // 64),
                          torch.zeros(N, dtype=torch.int32, device=dev))
    s, d = _counter_struct(ctx, st, "wire.map_counter_ingest")
    status = _status(N, dev)
    ctx.call("crdt_map_counter_ingest", _ptr_or_dummy(data), dptr(frame_off), dptr(actors), dptr(keys),
             ctypes.byref(s), ctypes.byref(d), dptr(status))
    return st, status


def map_counter_egress(states: MapCounterFrames, actors: torch.Tensor, keys: torch.Tensor,
                       ctx: Optional[Context] = None):
    """MapCounterFrames -> (frame_off (N+1,), bytes)."""
    ctx = _ctx(states.clock, ctx)
    _dict(ctx, actors, torch.int32, "wire.map_counter_egress(actors)")
    _dict(ctx, keys, torch.int32, "wire.map_counter_egress(keys)")
    s, d = _counter_struct(ctx, states, "wire.map_counter_egress")
    return _egress(ctx, "crdt_map_counter_egress", states.clock.shape[0], states.clock.device, ctypes.byref(s),
                   ctypes.byref(d), dptr(actors), dptr(keys))


def map_orswot_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                      members: torch.Tensor, Dcap: int, ctx: Optional[Context] = None, vd_cap: int = 16):
    """Map<u32, Orswot<u64, u32>> frames -> (MapOrswotFrames, status (N,) int32); members: sorted
    u64 member dictionary (int64 tensor); vd_cap nested deferred slots per key (>= 16)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.map_orswot_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.map_orswot_ingest(actors)")
    K = _dict(ctx, keys, torch.int32, "wire.map_orswot_ingest(keys)")
    M = _dict(ctx, members, torch.int64, "wire.map_orswot_ingest(members)")
    dev = data.device
    Mw = (M + 63) // 64
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
    st = MapOrswotFrames(z(N, A), z(N, K, A), z(N, K, A), z(N, K, M, A),
                         torch.zeros((N, K), dtype=torch.int32, device=dev), z(N, K, vd_cap, A),
                         z(N, K, vd_cap) if Mw == 1 else z(N, K, vd_cap, Mw), z(N, Dcap, A), z(N, Dcap, (K + 63) // 64),
                         torch.zeros(N, dtype=torch.int32, device=dev))
    s, d = _orswot_struct(ctx, st, "wire.map_orswot_ingest")
    status = _status(N, dev)
    ctx.call("crdt_map_orswot_ingest", _ptr_or_dummy(data), dptr(frame_off), dptr(actors), dptr(keys),
             dptr(members), ctypes.byref(s), ctypes.byref(d), dptr(status))
    return st, status


def map_orswot_egress(states: MapOrswotFrames, actors: torch.Tensor, keys: torch.Tensor, members: torch.Tensor,
                      ctx: Optional[Context] = None):
    """MapOrswotFrames -> (frame_off (N+1,), bytes)."""
    ctx = _ctx(states.clock, ctx)
    _dict(ctx, actors, torch.int32, "wire.map_orswot_egress(actors)")
    _dict(ctx, keys, torch.int32, "wire.map_orswot_egress(keys)")
    _dict(ctx, members, torch.int64, "wire.map_orswot_egress(members)")
    s, d = _orswot_struct(ctx, states, "wire.map_orswot_egress")
    return _egress(ctx, "crdt_map_orswot_egress", states.clock.shape[0], states.clock.device, ctypes.byref(s),
                   ctypes.byref(d), dptr(actors), dptr(keys), dptr(members))


def _nested_struct(ctx, st, what):
    from . import _abi
    N, K, A = _vmap_check(ctx, st, what)
    K2 = st.iec.shape[2]
    K2w = (K2 + 63) // 64 if K2 > 64 else 1
    Id = st.id_clock.shape[2] if st.id_clock.dim() == 4 else 0
    if Id < 16:
        raise ValueError(f"{what}: id_clock (N, K, Id, A) with Id >= 16 expected")
    Vs = st.ivc.shape[3] if st.ivc.dim() == 5 else 0
    if not 8 <= Vs <= 64:
        raise ValueError(f"{what}: ivc (N, K, K2, Vs, A) with Vs in 8..64 expected")
    shapes = dict(ic=(N, K, A), iec=(N, K, K2, A), ivc=(N, K, K2, Vs, A), ivv=(N, K, K2, Vs), nval=(N, K, K2),
                  id_n=(N, K), id_clock=(N, K, Id, A), id_keys=(N, K, Id) if K2w == 1 else (N, K, Id, K2w))
    for nm, shp in shapes.items():
        if tuple(getattr(st, nm).shape) != shp:
            raise ValueError(f"{what}: {nm} must be {shp}")
    s = _abi.MapNestedStates()
    s.N, s.K, s.K2, s.A, s.Id, s.Vs = N, K, K2, A, Id, Vs
    for nm in ("clock", "ec", "ic", "iec", "ivc", "ivv", "nval", "id_n", "id_clock", "id_keys"):
        setattr(s, nm, dptr(getattr(st, nm)))
    return s, _vmap_deferred(st)


def map_nested_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                      ikeys: torch.Tensor, Dcap: int, ctx: Optional[Context] = None, id_cap: int = 16,
                      v_cap: int = 8):
    """Map<u32, Map<u32, MVReg<u64>>> frames -> (MapNestedFrames, status (N,) int32); ikeys: sorted
    u32 inner-key dictionary (int32 tensor, at most 256; past 64 the inner key sets are K2w words)."""
    ctx = _ctx(data, ctx)
    N = _frames(ctx, data, frame_off, "wire.map_nested_ingest")
    A = _dict(ctx, actors, torch.int32, "wire.map_nested_ingest(actors)")
    K = _dict(ctx, keys, torch.int32, "wire.map_nested_ingest(keys)")
    K2 = _dict(ctx, ikeys, torch.int32, "wire.map_nested_ingest(ikeys)")
    dev = data.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
    z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    st = MapNestedFrames(z(N, A), z(N, K, A), z(N, K, A), z(N, K, K2, A), z(N, K, K2, v_cap, A), z(N, K, K2, v_cap),
                         z32(N, K, K2), z32(N, K), z(N, K, id_cap, A),
                         z(N, K, id_cap) if K2 <= 64 else z(N, K, id_cap, (K2 + 63) // 64), z(N, Dcap, A),
                         z(N, Dcap, (K + 63) // 64), z32(N))
    s, d = _nested_struct(ctx, st, "wire.map_nested_ingest")
    status = _status(N, dev)
    ctx.call("crdt_map_nested_ingest", _ptr_or_dummy(data), dptr(frame_off), dptr(actors), dptr(keys), dptr(ikeys),
             ctypes.byref(s), ctypes.byref(d), dptr(status))
    return st, status


def map_nested_egress(states: MapNestedFrames, actors: torch.Tensor, keys: torch.Tensor, ikeys: torch.Tensor,
                      ctx: Optional[Context] = None):
    """MapNestedFrames -> (frame_off (N+1,), bytes)."""
    ctx = _ctx(states.clock, ctx)
    _dict(ctx, actors, torch.int32, "wire.map_nested_egress(actors)")
    _dict(ctx, keys, torch.int32, "wire.map_nested_egress(keys)")
    _dict(ctx, ikeys, torch.int32, "wire.map_nested_egress(ikeys)")
    s, d = _nested_struct(ctx, states, "wire.map_nested_egress")
    return _egress(ctx, "crdt_map_nested_egress", states.clock.shape[0], states.clock.device, ctypes.byref(s),
                   ctypes.byref(d), dptr(actors), dptr(keys), dptr(ikeys))


# ---- op streams on the wire (include/crdt_gpu.h "serde wire format of op streams") ------------------
class OpsIngest(NamedTuple):
    """Result of orswot_ops_ingest / map_ops_ingest."""
    ops: tuple                # orswot.OrswotOpBatch / map.MapOpBatch: goes to apply_batch unchanged
    status: torch.Tensor      # (N,) int32: BAD / MISSING / CAP bits
    row_off: torch.Tensor     # (N+1,) int64: the state's first clock row
    id_off: torch.Tensor      # (N+1,) int64: the state's first member / keyset key
    totals: Optional[tuple]   # (ops, rows, ids) of the well-formed frames; None with sync=False


_I32 = (torch.int32, torch.uint32)
_I64 = (torch.int64, torch.uint64)


def _ops_check(what: str, tensors) -> None:
    """ValueError checks, all before any library call (and before a Context exists): every
    (tensor, name, dtypes) is a contiguous cuda tensor of one of `dtypes`, all on one device."""
    dev = None
    for t, nm, dts in tensors:  # dtypes and layouts of every argument first, then the device
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}({nm}): expected a torch.Tensor")
        if t.dtype not in dts:
            raise ValueError(f"{what}({nm}): dtype {t.dtype}; expected one of {dts}")
        if not t.is_contiguous():
            raise ValueError(f"{what}({nm}): must be contiguous")
    for t, nm, dts in tensors:
        if t.device.type != "cuda":
            raise ValueError(f"{what}({nm}): tensor on {t.device}; expected a cuda tensor")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError(f"{what}({nm}): tensor on {t.device}; the others are on {dev}")


def _frames_check(what, data, frame_off, dicts):
    """The frames and the dictionaries [(tensor, name, dtype)] of an op-stream ingest -> N."""
    _ops_check(what, [(data, "bytes", (torch.uint8,)), (frame_off, "frame_off", (torch.int64,))]
               + [(d, nm, (dt,)) for d, nm, dt in dicts])
    if data.dim() != 1 or frame_off.dim() != 1 or frame_off.shape[0] < 1:
        raise ValueError(f"{what}: bytes must be a uint8 vector and frame_off an int64 (N+1,) tensor")
    if any(d.dim() != 1 or d.shape[0] == 0 for d, _, _ in dicts):
        raise ValueError(f"{what}: the dictionaries must be non-empty vectors")
    return frame_off.shape[0] - 1


def _d32(d, nm):
    return d, nm, torch.int32


def _caps_check(what, sync, caps, names):
    """sync=True takes no capacities (the sizing call chooses them), sync=False one per name."""
    if sync:
        if caps is not None:
            raise ValueError(f"{what}: capacities are chosen by the sizing call unless sync=False")
        return None
    if caps is None or len(caps) != len(names) or any(int(c) < 0 for c in caps):
        raise ValueError(f"{what}: sync=False needs caps=({', '.join(names)}{',' if len(names) == 1 else ''})")
    return tuple(int(c) for c in caps)


def _sized_ingest(fn, data, frame_off, N, dict_args, n_firsts, n_totals, sync, caps, alloc, ctx):
    """The skeleton of every sized op-stream ingest: the sizing call (sync; its n_totals sums become the
    capacities) or the caller's capacities, then the fill.  alloc(caps, op_off) allocates the batch for
    those capacities -> (the _abi buffer struct, the batch, the batch's list-offset tensors, whose first
    entry is 0).  -> (batch, status, the n_firsts (N+1,) per-state offset tensors after op_off, totals)."""
    ctx = _ctx(data, ctx)
    dev = data.device
    status = torch.empty(N, dtype=torch.int32, device=dev)
    op_off, *firsts = (torch.empty(N + 1, dtype=torch.int64, device=dev) for _ in range(1 + n_firsts))
    head = (_ptr_or_dummy(data), dptr(frame_off), N, *dict_args)
    totals = None
    if sync:
        tot = (ctypes.c_uint64 * n_totals)()
        if N:
            ctx.call(fn, *head, None, *((None,) * n_firsts), dptr(status), tot)
        caps = totals = tuple(int(x) for x in tot)
    buf, batch, list_offs = alloc(caps, op_off)
    if N:
        ctx.call(fn, *head, ctypes.byref(buf), *(dptr(t) for t in firsts), dptr(status), None)
    else:
        for t in (op_off, *firsts, *(lo[:1] for lo in list_offs)):
            t.zero_()
    return batch, status, firsts, totals


def _ops_ingest(fn, buf_cls, is_map, data, frame_off, actors, ids, N, sync, caps, ctx):
    from .map import MapOpBatch
    from .orswot import OrswotOpBatch
    dev = data.device
    A, U = actors.shape[0], ids.shape[0]

    def alloc(caps, op_off):  # exactly enough room + one pad row / id, as encode_ops leaves
        n_op, n_row, n_id = caps
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        kind, actor, counter, row = e(n_op, torch.uint8), e(n_op, torch.int32), e(n_op, torch.int64), e(n_op, torch.int32)
        pool = torch.empty((n_row + 1, A), dtype=torch.int64, device=dev)
        ids_off, idv = e(n_op + 1, torch.int64), e(n_id + 1, torch.int32)
        pool[n_row].zero_()
        idv[n_id].zero_()
        b = buf_cls()
        b.op_cap, b.row_cap, b.id_cap = n_op, n_row, n_id
        b.op_off, b.kind, b.actor, b.counter = dptr(op_off), dptr(kind), dptr(actor), dptr(counter)
        if is_map:
            key, val = e(n_op, torch.int32), e(n_op, torch.int64)
            b.key, b.val, b.clk_row, b.clk_pool, b.key_off, b.keys = (dptr(key), dptr(val), dptr(row), dptr(pool),
                                                                      dptr(ids_off), dptr(idv))
            return b, MapOpBatch(op_off, kind, actor, counter, key, val, row, pool, ids_off, idv), (ids_off,)
        b.rm_row, b.rm_clock, b.mem_off, b.mem = dptr(row), dptr(pool), dptr(ids_off), dptr(idv)
        return b, OrswotOpBatch(op_off, kind, actor, counter, row, pool, ids_off, idv), (ids_off,)

    ops, status, (row_off, id_off), totals = _sized_ingest(fn, data, frame_off, N, (dptr(actors), A, dptr(ids), U), 2, 3,
                                                           sync, caps, alloc, ctx)
    return OpsIngest(ops, status, row_off, id_off, totals)


def orswot_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, members: torch.Tensor,
                      sync: bool = True, caps=None, ctx: Optional[Context] = None) -> OpsIngest:
    """Frames of Vec<orswot::Op<u64, u32>> (one per state) -> OpsIngest with an orswot.OrswotOpBatch.
    sync=True sizes first (one host synchronisation) and allocates exactly; sync=False takes
    caps=(op_cap, row_cap, id_cap), never synchronises, and marks states past a capacity with CAP."""
    what = "wire.orswot_ops_ingest"
    caps = _caps_check(what, sync, caps, ("op_cap", "row_cap", "id_cap"))
    N = _frames_check(what, data, frame_off, [_d32(actors, "actors"), (members, "members", torch.int64)])
    return _ops_ingest("crdt_orswot_ops_ingest", _abi.OrswotOpsBuf, False, data, frame_off, actors, members, N, sync, caps,
                       ctx)


def map_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                   sync: bool = True, caps=None, ctx: Optional[Context] = None) -> OpsIngest:
    """Frames of Vec<map::Op<u32, MVReg<u64, u32>, u32>> -> OpsIngest with a map.MapOpBatch (see
    orswot_ops_ingest for sync / caps; id_cap counts keyset keys)."""
    what = "wire.map_ops_ingest"
    caps = _caps_check(what, sync, caps, ("op_cap", "row_cap", "id_cap"))
    N = _frames_check(what, data, frame_off, [_d32(actors, "actors"), _d32(keys, "keys")])
    return _ops_ingest("crdt_map_ops_ingest", _abi.MapOpsBuf, True, data, frame_off, actors, keys, N, sync, caps, ctx)


def _ops_egress(fn, o, ops, N, actors, ids, ctx):
    return _egress(_ctx(ops.op_off, ctx), fn, N, ops.op_off.device, ctypes.byref(o), N, dptr(actors), actors.shape[0],
                   dptr(ids), ids.shape[0], with_status=True)


def _ops_batch_check(what, ops, fields, actors, ids, id_dt, id_nm, pool_nm):
    if not hasattr(ops, "_fields") or tuple(ops._fields) != fields:
        raise ValueError(f"{what}: expected an op batch with fields {fields}")
    want = {"op_off": _I64, "kind": (torch.uint8,), "counter": _I64, "val": _I64, pool_nm: _I64, "mem_off": _I64,
            "key_off": _I64}
    _ops_check(what, [(t, nm, want.get(nm, _I32)) for nm, t in zip(ops._fields, ops)]
               + [(actors, "actors", (torch.int32,)), (ids, id_nm, (id_dt,))])
    n = ops.kind.shape[0]
    pool = getattr(ops, pool_nm)
    if ops.op_off.dim() != 1 or ops.op_off.shape[0] < 1 or pool.dim() != 2 or pool.shape[1] != actors.shape[0]:
        raise ValueError(f"{what}: op_off (N+1,) and {pool_nm} (rows, A) expected")
    if actors.dim() != 1 or ids.dim() != 1 or actors.shape[0] == 0 or ids.shape[0] == 0:
        raise ValueError(f"{what}: the dictionaries must be non-empty vectors")
    for nm, t in zip(ops._fields, ops):
        if nm in ("mem_off", "key_off"):
            if t.dim() != 1 or t.shape[0] < n + 1:
                raise ValueError(f"{what}: {nm} needs n_ops+1 entries")
        elif nm not in ("op_off", pool_nm, "mem", "keys") and tuple(t.shape) != (n,):
            raise ValueError(f"{what}: ops.{nm} must have n_ops entries")
    return ops.op_off.shape[0] - 1, n


def orswot_ops_egress(ops, actors: torch.Tensor, members: torch.Tensor, ctx: Optional[Context] = None):
    """orswot.OrswotOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one Vec<orswot::Op> frame
    per state.  status bit 1 (MISSING): the state had an op with no wire form and its frame is the
    empty Vec."""
    from .orswot import OrswotOpBatch
    what = "wire.orswot_ops_egress"
    N, n = _ops_batch_check(what, ops, OrswotOpBatch._fields, actors, members, torch.int64, "members", "rm_clock")
    o = _abi.OrswotOps()
    o.n_ops = n
    o.op_off, o.kind, o.actor, o.counter = dptr(ops.op_off), dptr(ops.kind), dptr(ops.actor), dptr(ops.counter)
    o.rm_row, o.rm_clock, o.n_rm_rows = dptr(ops.rm_row), dptr(ops.rm_clock), ops.rm_clock.shape[0]
    o.mem_off, o.mem, o.n_mem = dptr(ops.mem_off), dptr(ops.mem), ops.mem.shape[0]
    return _ops_egress("crdt_orswot_ops_egress", o, ops, N, actors, members, ctx)


def map_ops_egress(ops, actors: torch.Tensor, keys: torch.Tensor, ctx: Optional[Context] = None):
    """map.MapOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one Vec<map::Op> frame per
    state (keysets in list order: ascending indices give the BTreeSet's order)."""
    from .map import MapOpBatch
    what = "wire.map_ops_egress"
    N, n = _ops_batch_check(what, ops, MapOpBatch._fields, actors, keys, torch.int32, "keys_dict", "clk_pool")
    o = _abi.MapOps()
    o.n_ops = n
    o.op_off, o.kind, o.actor, o.counter = dptr(ops.op_off), dptr(ops.kind), dptr(ops.actor), dptr(ops.counter)
    o.key, o.val, o.clk_row, o.clk_pool = dptr(ops.key), dptr(ops.val), dptr(ops.clk_row), dptr(ops.clk_pool)
    o.n_clk_rows, o.key_off, o.keys, o.n_keys = ops.clk_pool.shape[0], dptr(ops.key_off), dptr(ops.keys), ops.keys.shape[0]
    return _ops_egress("crdt_map_ops_egress", o, ops, N, actors, keys, ctx)


# ---- the value-typed Maps' op streams (include/crdt_gpu.h "value-typed Maps' op streams") -----------
class VMapOpsIngest(NamedTuple):
    """Result of map_counter_ops_ingest / map_orswot_ops_ingest / map_nested_ops_ingest."""
    batch: tuple                        # map.MapCounterOpBatch / MapOrswotOpBatch / MapNestedOpBatch, as *_apply_batch takes it
    status: torch.Tensor                # (N,) int32: BAD / MISSING / CAP bits
    row_off: torch.Tensor               # (N+1,) int64: the state's first clock row
    key_first: torch.Tensor             # (N+1,) int64: the state's first keyset key
    mem_first: Optional[torch.Tensor]   # (N+1,) int64: the state's first member (Orswot Map only)
    totals: Optional[tuple]             # (ops, rows, keys, mems) of the well-formed frames; None with sync=False


_U8 = (torch.uint8,)
_VOPS_DTYPES = {"kind": _U8, "vdir": _U8, "vkind": _U8, "ikind": _U8, "actor": _I32, "key": _I32, "vactor": _I32,
                "iactor": _I32, "ikey": _I32, "clk_row": _I32, "keys": _I32, "mems": _I32}  # the rest: 64-bit


_VOPS_CAPS = ("op_cap", "row_cap", "key_cap", "mem_cap")


def _vops_ingest(fn, buf_cls, batch_cls, data, frame_off, N, A, dict_args, K2w, sync, caps, ctx):
    """The batch is allocated as the host encoders of map.py leave it (one zero row / id where a pool
    would be empty)."""
    dev = data.device
    has_mem = "mems" in batch_cls._fields
    e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731

    def alloc(caps, op_off):
        n_op, n_row, n_key = caps[:3]
        n_mem = caps[3] if has_mem else 0
        t = {}
        for nm in batch_cls._fields:
            if nm in ("op_off", "clk_pool", "key_off", "keys", "mem_off", "mems", "ikeys"):
                continue
            t[nm] = e(n_op, _VOPS_DTYPES.get(nm, _I64)[0])
        t["op_off"] = op_off
        t["clk_pool"] = torch.empty((max(n_row, 1), A), dtype=torch.int64, device=dev)
        t["key_off"], t["keys"] = e(n_op + 1, torch.int64), e(max(n_key, 1), torch.int32)
        if has_mem:
            t["mem_off"], t["mems"] = e(n_op + 1, torch.int64), e(max(n_mem, 1), torch.int32)
        if "ikeys" in batch_cls._fields:
            t["ikeys"] = e(n_op, torch.int64) if K2w == 1 else torch.empty((n_op, K2w), dtype=torch.int64, device=dev)
        if n_row == 0:
            t["clk_pool"].zero_()
        if n_key == 0:
            t["keys"].zero_()
        if has_mem and n_mem == 0:
            t["mems"].zero_()
        b = buf_cls()
        b.op_cap, b.row_cap, b.key_cap = n_op, n_row, n_key
        if has_mem:
            b.mem_cap = n_mem
        for nm in batch_cls._fields:
            setattr(b, nm, dptr(t[nm]))
        return b, batch_cls(*(t[nm] for nm in batch_cls._fields)), (t["key_off"],) + ((t["mem_off"],) if has_mem else ())

    batch, status, firsts, totals = _sized_ingest(fn, data, frame_off, N, dict_args, 3 if has_mem else 2, 4, sync, caps,
                                                  alloc, ctx)
    return VMapOpsIngest(batch, status, firsts[0], firsts[1], firsts[2] if has_mem else None, totals)


def map_counter_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                           pn: bool = False, sync: bool = True, caps=None, ctx: Optional[Context] = None) -> VMapOpsIngest:
    """Frames of Vec<map::Op<u32, GCounter, u32>> (pn=False) or Vec<map::Op<u32, PNCounter, u32>> (pn=True),
    one per state -> VMapOpsIngest with a map.MapCounterOpBatch for map.counter_apply_batch.  sync=True
    sizes first (one host synchronisation) and allocates exactly; sync=False takes caps=(op_cap, row_cap,
    key_cap), never synchronises, and marks states past a capacity with CAP."""
    from .map import MapCounterOpBatch
    what = "wire.map_counter_ops_ingest"
    caps = _caps_check(what, sync, caps, _VOPS_CAPS[:3])
    N = _frames_check(what, data, frame_off, [_d32(actors, "actors"), _d32(keys, "keys")])
    A, K = actors.shape[0], keys.shape[0]
    return _vops_ingest("crdt_map_counter_ops_ingest", _abi.MapCounterOpsBuf, MapCounterOpBatch, data, frame_off,
                        N, A, (dptr(actors), A, dptr(keys), K, 1 if pn else 0), 1, sync, caps, ctx)


def map_orswot_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                          members: torch.Tensor, sync: bool = True, caps=None,
                          ctx: Optional[Context] = None) -> VMapOpsIngest:
    """Frames of Vec<map::Op<u32, Orswot<u64, u32>, u32>> -> VMapOpsIngest with a map.MapOrswotOpBatch for
    map.orswot_apply_batch (members: the sorted u64 member dictionary, int64; sync=False:
    caps=(op_cap, row_cap, key_cap, mem_cap))."""
    from .map import MapOrswotOpBatch
    what = "wire.map_orswot_ops_ingest"
    caps = _caps_check(what, sync, caps, _VOPS_CAPS)
    N = _frames_check(what, data, frame_off, [_d32(actors, "actors"), _d32(keys, "keys"),
                                              (members, "members", torch.int64)])
    A, K, M = actors.shape[0], keys.shape[0], members.shape[0]
    return _vops_ingest("crdt_map_orswot_ops_ingest", _abi.MapOrswotOpsBuf, MapOrswotOpBatch, data, frame_off,
                        N, A, (dptr(actors), A, dptr(keys), K, dptr(members), M), 1, sync, caps, ctx)


def _k2w(K2: int) -> int:
    return (K2 + 63) // 64 if K2 > 64 else 1


def map_nested_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, keys: torch.Tensor,
                          idict: torch.Tensor, sync: bool = True, caps=None,
                          ctx: Optional[Context] = None) -> VMapOpsIngest:
    """Frames of Vec<map::Op<u32, Map<u32, MVReg<u64, u32>, u32>, u32>> -> VMapOpsIngest with a
    map.MapNestedOpBatch for map.nested_apply_batch (idict: the sorted u32 inner-key dictionary, at most
    256 entries; its size decides the ikeys mask's shape, (n_ops,) up to 64 and (n_ops, ceil(K2/64))
    past it; sync=False: caps=(op_cap, row_cap, key_cap))."""
    from .map import MapNestedOpBatch
    what = "wire.map_nested_ops_ingest"
    caps = _caps_check(what, sync, caps, _VOPS_CAPS[:3])
    N = _frames_check(what, data, frame_off, [_d32(actors, "actors"), _d32(keys, "keys"), _d32(idict, "idict")])
    A, K, K2 = actors.shape[0], keys.shape[0], idict.shape[0]
    return _vops_ingest("crdt_map_nested_ops_ingest", _abi.MapNestedOpsBuf, MapNestedOpBatch, data, frame_off,
                        N, A, (dptr(actors), A, dptr(keys), K, dptr(idict), K2), _k2w(K2), sync, caps, ctx)


def _vops_batch(what, ops, batch_cls, o, actors, keys, third=None, third_dt=None, third_nm=None):
    """Check an op batch before egress and fill the const struct `o` from it; returns (N, dictionary args)."""
    if not hasattr(ops, "_fields") or tuple(ops._fields) != batch_cls._fields:
        raise ValueError(f"{what}: expected an op batch with fields {batch_cls._fields}")
    dicts = [(actors, "actors", (torch.int32,)), (keys, "keys_dict", (torch.int32,))]
    if third_nm:
        dicts.append((third, third_nm, (third_dt,)))
    _ops_check(what, [(t, nm, _VOPS_DTYPES.get(nm, _I64)) for nm, t in zip(ops._fields, ops)] + dicts)
    if any(d.dim() != 1 or d.shape[0] == 0 for d, _, _ in dicts):
        raise ValueError(f"{what}: the dictionaries must be non-empty vectors")
    n = ops.kind.shape[0]
    if (ops.op_off.dim() != 1 or ops.op_off.shape[0] < 1 or ops.clk_pool.dim() != 2
            or ops.clk_pool.shape[1] != actors.shape[0]):
        raise ValueError(f"{what}: op_off (N+1,) and clk_pool (rows, A) expected")
    K2w = _k2w(third.shape[0]) if third_nm == "idict" else 1
    for nm, t in zip(ops._fields, ops):
        if nm in ("mem_off", "key_off"):
            if t.dim() != 1 or t.shape[0] < n + 1:
                raise ValueError(f"{what}: {nm} needs n_ops+1 entries")
        elif nm == "ikeys":
            if tuple(t.shape) != ((n,) if K2w == 1 else (n, K2w)):
                raise ValueError(f"{what}: ops.ikeys must be (n_ops,) or, past 64 inner keys, (n_ops, {K2w})")
        elif nm in ("keys", "mems"):
            if t.dim() != 1:
                raise ValueError(f"{what}: ops.{nm} must be a vector")
        elif nm not in ("op_off", "clk_pool") and tuple(t.shape) != (n,):
            raise ValueError(f"{what}: ops.{nm} must have n_ops entries")
    o.n_ops = n
    for nm, t in zip(ops._fields, ops):
        setattr(o, nm, dptr(t))
    o.n_clk_rows, o.n_keys = ops.clk_pool.shape[0], ops.keys.shape[0]
    if "mems" in ops._fields:
        o.n_mems = ops.mems.shape[0]
    return ops.op_off.shape[0] - 1


def _vops_egress(fn, o, ops, N, dict_args, ctx):
    return _egress(_ctx(ops.op_off, ctx), fn, N, ops.op_off.device, ctypes.byref(o), N, *dict_args, with_status=True)


def map_counter_ops_egress(ops, actors: torch.Tensor, keys: torch.Tensor, pn: bool = False,
                           ctx: Optional[Context] = None):
    """map.MapCounterOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one frame per state of
    Vec<map::Op<u32, GCounter, u32>> (pn=False: an op with vdir = 1 has no wire form) or of the PNCounter
    Map's ops (pn=True).  status bit 1 (MISSING): the state had an op with no wire form and its frame
    is the empty Vec."""
    from .map import MapCounterOpBatch
    what = "wire.map_counter_ops_egress"
    o = _abi.MapCounterOps()
    N = _vops_batch(what, ops, MapCounterOpBatch, o, actors, keys)
    return _vops_egress("crdt_map_counter_ops_egress", o, ops, N,
                        (dptr(actors), actors.shape[0], dptr(keys), keys.shape[0], 1 if pn else 0), ctx)


def map_orswot_ops_egress(ops, actors: torch.Tensor, keys: torch.Tensor, members: torch.Tensor,
                          ctx: Optional[Context] = None):
    """map.MapOrswotOpBatch -> (frame_off, bytes, status): frames of Vec<map::Op<u32, Orswot<u64, u32>, u32>>
    (member lists and keysets in list order)."""
    from .map import MapOrswotOpBatch
    what = "wire.map_orswot_ops_egress"
    o = _abi.MapOrswotOps()
    N = _vops_batch(what, ops, MapOrswotOpBatch, o, actors, keys, members, torch.int64, "members")
    return _vops_egress("crdt_map_orswot_ops_egress", o, ops, N,
                        (dptr(actors), actors.shape[0], dptr(keys), keys.shape[0], dptr(members), members.shape[0]), ctx)


def map_nested_ops_egress(ops, actors: torch.Tensor, keys: torch.Tensor, idict: torch.Tensor,
                          ctx: Optional[Context] = None):
    """map.MapNestedOpBatch -> (frame_off, bytes, status): frames of Vec<map::Op<u32, Map<u32, MVReg>, u32>>
    (an inner Rm's mask bits ascending: the BTreeSet's order)."""
    from .map import MapNestedOpBatch
    what = "wire.map_nested_ops_egress"
    o = _abi.MapNestedOps()
    N = _vops_batch(what, ops, MapNestedOpBatch, o, actors, keys, idict, torch.int32, "idict")
    return _vops_egress("crdt_map_nested_ops_egress", o, ops, N,
                        (dptr(actors), actors.shape[0], dptr(keys), keys.shape[0], dptr(idict), idict.shape[0]), ctx)


# ---- MVReg<u64, u32> on its own (include/crdt_gpu.h "MVReg<u64, u32> on its own") -------------------
EMPTY_CLOCK = 8  # mvreg_ingest status bit 3: a value with an empty clock was dropped


class MVRegOpsIngest(NamedTuple):
    """Result of mvreg_ops_ingest."""
    ops: tuple                # mvreg.MVRegOpBatch: goes to mvreg.apply_batch unchanged
    status: torch.Tensor      # (N,) int32: BAD / MISSING / CAP bits
    totals: Optional[tuple]   # (ops, rows) of the well-formed frames; None with sync=False


def _mvreg_states(what, vclk, vval, actors):
    for t, nm in ((vclk, "vclk"), (vval, "vval")):  # (registers may be strided: no contiguity asked here)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}({nm}): expected a torch.Tensor")
        if t.dtype not in _I64:
            raise ValueError(f"{what}({nm}): dtype {t.dtype}; expected one of {_I64}")
    _ops_check(what, ((actors, "actors", (torch.int32,)),))
    for t, nm in ((vclk, "vclk"), (vval, "vval")):
        if t.device != actors.device:
            raise ValueError(f"{what}({nm}): tensor on {t.device}; expected a cuda tensor on {actors.device}")
    if vclk.dim() != 3 or vval.dim() != 2 or tuple(vclk.shape[:2]) != tuple(vval.shape):
        raise ValueError(f"{what}: vclk (N, V, A) and vval (N, V) expected")
    N, V, A = vclk.shape
    if actors.dim() != 1 or actors.shape[0] != A or A == 0 or V == 0:
        raise ValueError(f"{what}: the actor dictionary must hold A = {A} >= 1 ids and V >= 1")
    if vclk.stride(2) != 1 or vclk.stride(1) != A or vval.stride(1) != 1:
        raise ValueError(f"{what}: each register's slots must be packed")
    return _abi.MVRegStates(N, A, V, vclk.data_ptr(), vclk.stride(0), vval.data_ptr(), vval.stride(0))


def mvreg_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, V: int,
                 ctx: Optional[Context] = None):
    """MVReg<u64, u32> frames -> (vclk (N, V, A) int64, vval (N, V) int64, status (N,) int32): the
    values in Vec order from slot 0, the rest zero.  status bits BAD / MISSING / CAP (more than V
    values: the first V kept) / EMPTY_CLOCK (a value with an empty clock: dropped)."""
    what = "wire.mvreg_ingest"
    N, A = _frames_check(what, data, frame_off, [_d32(actors, "actors")]), actors.shape[0]
    if int(V) < 1:
        raise ValueError(f"{what}: V >= 1 value slots")
    ctx = _ctx(data, ctx)
    dev = data.device
    vclk = torch.empty((N, int(V), A), dtype=torch.int64, device=dev)
    vval = torch.empty((N, int(V)), dtype=torch.int64, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    st = _abi.MVRegStates(N, A, int(V), vclk.data_ptr(), int(V) * A, vval.data_ptr(), int(V))
    ctx.call("crdt_mvreg_ingest", _ptr_or_dummy(data), dptr(frame_off), N, dptr(actors), A, ctypes.byref(st),
             dptr(status))
    return vclk, vval, status


def mvreg_egress(vclk: torch.Tensor, vval: torch.Tensor, actors: torch.Tensor, ctx: Optional[Context] = None):
    """Dense registers (vclk (N, V, A), vval (N, V)) -> (frame_off (N+1,), bytes) of MVReg frames:
    occupied slots in slot order."""
    st = _mvreg_states("wire.mvreg_egress", vclk, vval, actors)
    ctx = _ctx(vclk, ctx)
    return _egress(ctx, "crdt_mvreg_egress", st.N, vclk.device, ctypes.byref(st), dptr(actors))


def mvreg_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, sync: bool = True, caps=None,
                     ctx: Optional[Context] = None) -> MVRegOpsIngest:
    """Frames of Vec<mvreg::Op<u64, u32>> (one per register) -> MVRegOpsIngest with a
    mvreg.MVRegOpBatch.  sync=True sizes first (one host synchronisation) and allocates exactly;
    sync=False takes caps=(op_cap, row_cap), never synchronises, and marks the registers past a
    capacity with CAP."""
    from .mvreg import MVRegOpBatch
    what = "wire.mvreg_ops_ingest"
    caps = _caps_check(what, sync, caps, ("op_cap", "row_cap"))
    N, A = _frames_check(what, data, frame_off, [_d32(actors, "actors")]), actors.shape[0]
    dev = data.device

    def alloc(caps, op_off):  # exactly enough room + one pad row, as encode_ops leaves
        n_op, n_row = caps
        row = torch.empty(n_op, dtype=torch.int32, device=dev)
        val = torch.empty(n_op, dtype=torch.int64, device=dev)
        pool = torch.empty((n_row + 1, A), dtype=torch.int64, device=dev)
        pool[n_row].zero_()
        b = _abi.MVRegOpsBuf(n_op, dptr(op_off), dptr(row), dptr(pool), n_row, dptr(val))
        return b, MVRegOpBatch(op_off, row, pool, val), ()

    ops, status, _, totals = _sized_ingest("crdt_mvreg_ops_ingest", data, frame_off, N, (dptr(actors), A), 0, 2, sync, caps,
                                           alloc, ctx)
    return MVRegOpsIngest(ops, status, totals)


def mvreg_ops_egress(ops, actors: torch.Tensor, ctx: Optional[Context] = None):
    """mvreg.MVRegOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one Vec<mvreg::Op> frame
    per register.  status bit 1 (MISSING): the register had an op with no wire form (clk_row out of
    range, an invalid op_off) and its frame is the empty Vec."""
    from .mvreg import MVRegOpBatch
    what = "wire.mvreg_ops_egress"
    if not hasattr(ops, "_fields") or tuple(ops._fields) != MVRegOpBatch._fields:
        raise ValueError(f"{what}: expected an op batch with fields {MVRegOpBatch._fields}")
    _ops_check(what, ((ops.op_off, "op_off", _I64), (ops.clk_row, "clk_row", _I32), (ops.clk_pool, "clk_pool", _I64),
                      (ops.val, "val", _I64), (actors, "actors", (torch.int32,))))
    n = ops.val.shape[0]
    if actors.dim() != 1 or actors.shape[0] == 0:
        raise ValueError(f"{what}: the actor dictionary must be a non-empty vector")
    if ops.op_off.dim() != 1 or ops.op_off.shape[0] < 1 or ops.clk_pool.dim() != 2 \
            or ops.clk_pool.shape[1] != actors.shape[0] or tuple(ops.clk_row.shape) != (n,) or ops.val.dim() != 1:
        raise ValueError(f"{what}: op_off (N+1,), clk_row / val (n_ops,) and clk_pool (rows, A) expected")
    N = ops.op_off.shape[0] - 1
    o = _abi.MVRegOps(n, dptr(ops.op_off), _ptr_or_dummy(ops.clk_row), _ptr_or_dummy(ops.clk_pool),
                      ops.clk_pool.shape[0], _ptr_or_dummy(ops.val))
    return _egress(_ctx(ops.op_off, ctx), "crdt_mvreg_ops_egress", N, ops.op_off.device, ctypes.byref(o), N, dptr(actors),
                   actors.shape[0], with_status=True)


# ---- the lattice types' op streams (include/crdt_gpu.h "the lattice types' op streams") --------------
class DotOpBatch(NamedTuple):
    """Ops of VClock / GCounter / PNCounter / GSet grouped by state: state_idx / actor / counter (/ dir)
    go to apply.apply_dots, state_idx / element to apply.apply_inserts."""
    op_off: torch.Tensor              # (N+1,) int64
    state_idx: torch.Tensor           # (n_ops,) int32
    actor: torch.Tensor               # (n_ops,) int32: the dense actor index (GSet: the element index)
    counter: Optional[torch.Tensor]   # (n_ops,) int64; None for GSet
    dir: Optional[torch.Tensor]       # (n_ops,) uint8, PNCounter only

    @property
    def element(self) -> torch.Tensor:
        return self.actor


class DotOpsIngest(NamedTuple):
    """Result of vclock_ops_ingest / pncounter_ops_ingest / gset_ops_ingest."""
    ops: DotOpBatch
    status: torch.Tensor      # (N,) int32: BAD / MISSING / CAP bits
    totals: Optional[tuple]   # (ops,) of the well-formed frames; None with sync=False


class LwwRegOpsIngest(NamedTuple):
    """Result of lwwreg_ops_ingest."""
    ops: tuple                # lwwreg.LwwRegOpBatch: goes to lwwreg.apply_batch unchanged
    status: torch.Tensor
    totals: Optional[tuple]


def _dot_ops_ingest(what, kind, data, frame_off, d, d_dt, d_nm, sync, caps, ctx):
    caps = _caps_check(what, sync, caps, ("op_cap",))
    N = _frames_check(what, data, frame_off, [(d, d_nm, d_dt)])
    dev = data.device

    def alloc(caps, op_off):
        (cap,) = caps
        if sync:
            state_idx = torch.empty(cap, dtype=torch.int32, device=dev)
        else:  # entries past the ops kept are never written: an apply of the whole arrays skips them
            state_idx = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        col = torch.empty(cap, dtype=torch.int32, device=dev)
        counter = torch.empty(cap, dtype=torch.int64, device=dev) if kind != "gset" else None
        dr = torch.empty(cap, dtype=torch.uint8, device=dev) if kind == "pncounter" else None
        b = _abi.DotOpsBuf(cap, dptr(op_off), _ptr_or_dummy(state_idx), _ptr_or_dummy(col),
                           None if counter is None else _ptr_or_dummy(counter), None if dr is None else _ptr_or_dummy(dr))
        return b, DotOpBatch(op_off, state_idx, col, counter, dr), ()

    ops, status, _, totals = _sized_ingest(f"crdt_{kind}_ops_ingest", data, frame_off, N, (dptr(d), d.shape[0]), 0, 1, sync,
                                           caps, alloc, ctx)
    return DotOpsIngest(ops, status, totals)


def vclock_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, sync: bool = True, caps=None,
                      ctx: Optional[Context] = None) -> DotOpsIngest:
    """Frames of Vec<Dot<u32>> (one per VClock / GCounter state) -> DotOpsIngest.  sync=True sizes
    first (one host synchronisation) and allocates exactly; sync=False takes caps=(op_cap,), never
    synchronises, and marks the states past the capacity with CAP (op_cap = sum((B_s - 8) // 12)
    over the frames always suffices)."""
    return _dot_ops_ingest("wire.vclock_ops_ingest", "vclock", data, frame_off, actors, torch.int32, "actors", sync,
                           caps, ctx)


def pncounter_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, actors: torch.Tensor, sync: bool = True,
                         caps=None, ctx: Optional[Context] = None) -> DotOpsIngest:
    """Frames of Vec<pncounter::Op<u32>> -> DotOpsIngest with dir (0 = Pos, 1 = Neg); 16-byte records."""
    return _dot_ops_ingest("wire.pncounter_ops_ingest", "pncounter", data, frame_off, actors, torch.int32, "actors",
                           sync, caps, ctx)


def gset_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, elems: torch.Tensor, sync: bool = True, caps=None,
                    ctx: Optional[Context] = None) -> DotOpsIngest:
    """Frames of Vec<u64> (GSet ops) -> DotOpsIngest whose ops.element is the dense element index in
    the sorted u64 dictionary `elems`; 8-byte records."""
    return _dot_ops_ingest("wire.gset_ops_ingest", "gset", data, frame_off, elems, torch.int64, "elems", sync, caps,
                           ctx)


def lwwreg_ops_ingest(data: torch.Tensor, frame_off: torch.Tensor, sync: bool = True, caps=None,
                      ctx: Optional[Context] = None) -> LwwRegOpsIngest:
    """Frames of Vec<LWWReg<u64, u64>> (one per register) -> LwwRegOpsIngest with a
    lwwreg.LwwRegOpBatch; 16-byte records (val, marker), no dictionary."""
    from .lwwreg import LwwRegOpBatch
    what = "wire.lwwreg_ops_ingest"
    caps = _caps_check(what, sync, caps, ("op_cap",))
    N = _frames_check(what, data, frame_off, [])
    dev = data.device

    def alloc(caps, op_off):
        (cap,) = caps
        marker = torch.empty(cap, dtype=torch.int64, device=dev)
        val = torch.empty(cap, dtype=torch.int64, device=dev)
        b = _abi.LwwRegOpsBuf(cap, dptr(op_off), _ptr_or_dummy(marker), _ptr_or_dummy(val))
        return b, LwwRegOpBatch(op_off, marker, val), ()

    ops, status, _, totals = _sized_ingest("crdt_lwwreg_ops_ingest", data, frame_off, N, (), 0, 1, sync, caps, alloc, ctx)
    return LwwRegOpsIngest(ops, status, totals)


def _dot_ops_egress(what, kind, ops, d, d_dt, d_nm, ctx):
    for nm in ("op_off", "actor", "counter", "dir"):
        if not hasattr(ops, nm):
            raise ValueError(f"{what}: expected an op batch with fields {DotOpBatch._fields}")
    ts = [(ops.op_off, "op_off", _I64), (ops.actor, "actor", _I32), (d, d_nm, (d_dt,))]
    if kind != "gset":
        ts.append((ops.counter, "counter", _I64))
    if kind == "pncounter":
        ts.append((ops.dir, "dir", (torch.uint8,)))
    _ops_check(what, ts)
    n = ops.actor.shape[0]
    if d.dim() != 1 or d.shape[0] == 0:
        raise ValueError(f"{what}: the {d_nm} dictionary must be a non-empty vector")
    if ops.op_off.dim() != 1 or ops.op_off.shape[0] < 1 or any(tuple(t.shape) != (n,) for t, _, _ in ts[3:]) \
            or ops.actor.dim() != 1:
        raise ValueError(f"{what}: op_off (N+1,) and (n_ops,) op arrays expected")
    N = ops.op_off.shape[0] - 1
    o = _abi.DotOps(n, dptr(ops.op_off), None, _ptr_or_dummy(ops.actor),
                    None if kind == "gset" else _ptr_or_dummy(ops.counter),
                    _ptr_or_dummy(ops.dir) if kind == "pncounter" else None)
    return _egress(_ctx(ops.op_off, ctx), f"crdt_{kind}_ops_egress", N, ops.op_off.device, ctypes.byref(o), N, dptr(d),
                   d.shape[0], with_status=True)


def vclock_ops_egress(ops, actors: torch.Tensor, ctx: Optional[Context] = None):
    """DotOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one Vec<Dot<u32>> frame per state.
    status bit 1 (MISSING): the state had an op with no wire form (an actor index >= A, an invalid
    op_off) and its frame is the empty Vec.  state_idx is not read."""
    return _dot_ops_egress("wire.vclock_ops_egress", "vclock", ops, actors, torch.int32, "actors", ctx)


def pncounter_ops_egress(ops, actors: torch.Tensor, ctx: Optional[Context] = None):
    """As vclock_ops_egress for Vec<pncounter::Op<u32>> frames (a dir > 1 has no wire form)."""
    return _dot_ops_egress("wire.pncounter_ops_egress", "pncounter", ops, actors, torch.int32, "actors", ctx)


def gset_ops_egress(ops, elems: torch.Tensor, ctx: Optional[Context] = None):
    """As vclock_ops_egress for Vec<u64> frames: ops.actor holds the element indices into `elems`."""
    return _dot_ops_egress("wire.gset_ops_egress", "gset", ops, elems, torch.int64, "elems", ctx)


def lwwreg_ops_egress(ops, ctx: Optional[Context] = None):
    """lwwreg.LwwRegOpBatch -> (frame_off (N+1,), bytes, status (N,) int32): one Vec<LWWReg> frame per
    register; status bit 1: an invalid op_off (the empty Vec)."""
    from .lwwreg import LwwRegOpBatch
    what = "wire.lwwreg_ops_egress"
    if not hasattr(ops, "_fields") or tuple(ops._fields) != LwwRegOpBatch._fields:
        raise ValueError(f"{what}: expected an op batch with fields {LwwRegOpBatch._fields}")
    _ops_check(what, ((ops.op_off, "op_off", _I64), (ops.marker, "marker", _I64), (ops.val, "val", _I64)))
    n = ops.marker.shape[0]
    if ops.op_off.dim() != 1 or ops.op_off.shape[0] < 1 or ops.marker.dim() != 1 or tuple(ops.val.shape) != (n,):
        raise ValueError(f"{what}: op_off (N+1,) and marker / val (n_ops,) expected")
    N = ops.op_off.shape[0] - 1
    o = _abi.LwwRegOps(n, dptr(ops.op_off), _ptr_or_dummy(ops.marker), _ptr_or_dummy(ops.val))
    return _egress(_ctx(ops.op_off, ctx), "crdt_lwwreg_ops_egress", N, ops.op_off.device, ctypes.byref(o), N,
                   with_status=True)
