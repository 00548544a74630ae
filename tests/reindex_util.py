"""Shared by the reindex tests: the plain numpy statement of the gather (exp[..., j] = x[..., src[j]]),
the dense states of eq_util gathered with it, and the expected status words, all independent of the
code under test.  Dense states are the dicts of eq_util (orswot: clock / entries / dcl / dset / cnt;
map: clock / ec / vclk / vval / dcl / dset / cnt; mvreg: vclk / vval)."""
import numpy as np

DCAP, DROPPED, INVALID, VALUES = 1, 2, 4, 16


def norm_src(src, n_out):
    """The map as int64: None is the identity on n_out indices (those past n_in are nobody)."""
    return np.arange(n_out, dtype=np.int64) if src is None else np.asarray(src).astype(np.int64)


def gather(x, src, axis, n_out=None):
    """exp[..., j, ...] = x[..., src[j], ...] along `axis`; src[j] outside [0, n_in) is nobody: zeros."""
    n_in = x.shape[axis]
    src = norm_src(src, n_in if n_out is None else n_out)
    ok = (src >= 0) & (src < n_in)
    shape = [1] * x.ndim
    shape[axis] = len(src)
    if n_in == 0:
        full = list(x.shape)
        full[axis] = len(src)
        return np.zeros(full, x.dtype)
    return np.where(ok.reshape(shape), np.take(x, np.where(ok, src, 0), axis=axis), 0).astype(x.dtype)


def dropped(src, n_in, n_out):
    """The input indices no output index takes."""
    src = norm_src(src, n_out)
    return np.setdiff1d(np.arange(n_in), src[(src >= 0) & (src < n_in)])


def unpack(x, U):
    """(..., W) u64 bitmap words -> (..., U) bits."""
    b = np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1, bitorder="little")
    return b[..., :U]


def pack(bits):
    """(..., U) bits -> (..., ceil(U / 64)) u64 words, the bits past U zero."""
    U = bits.shape[-1]
    W = (U + 63) // 64
    pad = np.zeros(bits.shape[:-1] + (W * 64 - U,), np.uint8)
    b = np.concatenate([bits.astype(np.uint8), pad], axis=-1)
    return np.ascontiguousarray(np.packbits(b, axis=-1, bitorder="little")).view(np.uint64).reshape(bits.shape[:-1] + (W,))


def gather_bits(x, src, U_in, U_out):
    return pack(gather(unpack(x, U_in), src, x.ndim - 1, U_out))


def insert_map(n_in, extra, seed=0):
    """n_in old indices with `extra` new ones inserted: one at the front, one at the end, the rest inside
    (the first of them in the middle).  Returns (src (n_in + extra,) int64 with -1 for the new ones, pos
    (n_in,) the new position of every old index)."""
    n_out = n_in + extra
    rng = np.random.default_rng(seed)
    new = set()
    for cand in (0, n_out - 1, n_out // 2):
        if len(new) < extra:
            new.add(cand)
    while len(new) < extra:
        new.add(int(rng.integers(n_out)))
    src = np.full(n_out, -1, np.int64)
    old = [j for j in range(n_out) if j not in new]
    src[old] = np.arange(n_in)
    return src, np.array(old, np.int64)


def inverse(src, n_in):
    """The map back: input index i takes output index pos[i] (every input index is kept)."""
    src = np.asarray(src).astype(np.int64)
    inv = np.full(n_in, -1, np.int64)
    ok = (src >= 0) & (src < n_in)
    inv[src[ok]] = np.flatnonzero(ok)
    return inv


def _deferred(st, fa, fb, U_in, U_out, A, Dcap):
    """Deferred slots, out count and the bits they contribute."""
    cnt = st["cnt"].astype(np.int64)
    N, Din = st["dcl"].shape[0], st["dcl"].shape[1]
    invalid = cnt > Din
    ocnt = np.where(invalid, 0, np.minimum(cnt, Dcap))
    dcl = gather(gather(st["dcl"], fa, 2, A), None, 1, Dcap)
    dset = gather(gather_bits(st["dset"], fb, U_in, U_out), None, 1, Dcap)
    keep = np.arange(Dcap)[None, :] < ocnt[:, None]
    dcl = np.where(keep[:, :, None], dcl, 0).astype(np.uint64)
    dset = np.where(keep[:, :, None], dset, 0).astype(np.uint64)
    live = np.arange(Din)[None, :] < cnt[:, None]
    da, db = dropped(fa, st["dcl"].shape[2], A), dropped(fb, U_in, U_out)
    lost = (st["dcl"][:, :, da] != 0).any(axis=2) | (unpack(st["dset"], U_in)[:, :, db] != 0).any(axis=2)
    lost = (lost & live).any(axis=1) if Din else np.zeros(N, bool)
    status = np.where(invalid, INVALID, np.where(cnt > Dcap, DCAP, 0))
    return dcl, dset, ocnt.astype(np.int32), invalid, lost, status


def orswot_reindex(st, fa, fm, M, A, Dcap):
    """(gathered dense state, status (N,) int32)."""
    Ain, Min = st["clock"].shape[1], st["entries"].shape[1]
    dcl, dset, ocnt, invalid, lost, status = _deferred(st, fa, fm, Min, M, A, Dcap)
    z = ~invalid
    clock = gather(st["clock"], fa, 1, A) * z[:, None].astype(np.uint64)
    entries = gather(gather(st["entries"], fm, 1, M), fa, 2, A) * z[:, None, None].astype(np.uint64)
    da, dm = dropped(fa, Ain, A), dropped(fm, Min, M)
    lost = lost | (st["clock"][:, da] != 0).any(axis=1) | (st["entries"][:, :, da] != 0).any(axis=(1, 2)) \
        | (st["entries"][:, dm, :] != 0).any(axis=(1, 2))
    status = status | np.where(z & lost, DROPPED, 0)
    return dict(clock=clock, entries=entries, dcl=dcl, dset=dset, cnt=ocnt), status.astype(np.int32)


def _registers(vclk, vval, fa, A, V, kept):
    """vclk (N, K, Vin, Ain) / vval (N, K, Vin) of the kept keys -> slot-resized, column-gathered arrays and
    the per-state DROPPED / VALUES flags."""
    Vin, Ain = vclk.shape[2], vclk.shape[3]
    oc = gather(gather(vclk, fa, 3, A), None, 2, V)
    ov = gather(vval, None, 2, V)
    da = dropped(fa, Ain, A)
    kc = vclk[:, kept]
    lost = (kc[:, :, :min(V, Vin), :][..., da] != 0).any(axis=(1, 2, 3))
    vals = (kc[:, :, V:, :] != 0).any(axis=(1, 2, 3)) if Vin > V else np.zeros(vclk.shape[0], bool)
    return oc, ov, lost, vals


def mvreg_reindex(st, fa, A, V):
    oc, ov, lost, vals = _registers(st["vclk"][:, None], st["vval"][:, None], fa, A, V, np.array([0]))
    status = np.where(lost, DROPPED, 0) | np.where(vals, VALUES, 0)
    return dict(vclk=oc[:, 0], vval=ov[:, 0]), status.astype(np.int32)


def map_reindex(st, fa, fk, K, V, A, Dcap):
    Ain, Kin = st["clock"].shape[1], st["ec"].shape[1]
    dcl, dset, ocnt, invalid, lost, status = _deferred(st, fa, fk, Kin, K, A, Dcap)
    z = ~invalid
    da, dk = dropped(fa, Ain, A), dropped(fk, Kin, K)
    kept = np.setdiff1d(np.arange(Kin), dk)
    oc, ov, rl, vals = _registers(st["vclk"], st["vval"], fa, A, V, kept)
    clock = gather(st["clock"], fa, 1, A) * z[:, None].astype(np.uint64)
    ec = gather(gather(st["ec"], fk, 1, K), fa, 2, A) * z[:, None, None].astype(np.uint64)
    vclk = gather(oc, fk, 1, K) * z[:, None, None, None].astype(np.uint64)
    vval = gather(ov, fk, 1, K) * z[:, None, None].astype(np.uint64)
    lost = lost | rl | (st["clock"][:, da] != 0).any(axis=1) | (st["ec"][:, :, da] != 0).any(axis=(1, 2)) \
        | (st["ec"][:, dk, :] != 0).any(axis=(1, 2))
    status = status | np.where(z & lost, DROPPED, 0) | np.where(z & vals, VALUES, 0)
    return dict(clock=clock, ec=ec, vclk=vclk, vval=vval, dcl=dcl, dset=dset, cnt=ocnt), status.astype(np.int32)
