"""CPU checks of the reindex surface: the seven entry points and the four CRDT_REINDEX_* bits are
declared in the header, bound in _abi.py with matching argument counts, exported by the library and
carried by the Rust FFI file, with CRDT_ABI_VERSION still 8 (additions only); the per-type callables
exist; and the tests' own numpy gather (reindex_util) agrees with the oracle's re-labelled objects."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crdt_gpu.h")
FFI = os.path.join(ROOT, "rust", "src", "gpu", "ffi.rs")

# name -> number of arguments after ctx
API = {"crdt_reindex_map_u32": 6, "crdt_reindex_map_u64": 6, "crdt_rows_reindex": 10, "crdt_bitmap_reindex": 9,
       "crdt_orswot_reindex": 5, "crdt_mvreg_reindex": 4, "crdt_map_reindex": 7}
BITS = {"CRDT_REINDEX_DCAP": 1, "CRDT_REINDEX_DROPPED": 2, "CRDT_REINDEX_INVALID": 4, "CRDT_REINDEX_VALUES": 16}


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"{name} is not declared in include/crdt_gpu.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(API))
def test_entry_point_declared_and_bound(name):
    import crdts_gpu._abi as abi
    args = header_args(name)
    assert args[0] == "crdt_ctx *ctx" and len(args) == API[name] + 1
    if name.startswith("crdt_reindex_map"):
        assert args[-1] == "uint32_t *n_lost"
    else:
        assert args[-1] == "uint32_t *status"
    assert name in abi.EXPORTS
    argtypes, restype = abi._SIGS[name]
    assert len(argtypes) == len(args) and restype is ctypes.c_int


def test_status_bits_in_header_bindings_and_package():
    import crdts_gpu as cg
    import crdts_gpu._abi as abi
    src = open(HEADER).read()
    for name, val in BITS.items():
        assert re.search(r"^#define\s+" + name + r"\s+" + str(val) + r"u\s", src, re.M), name
        assert getattr(abi, name) == val
        assert getattr(cg, name[len("CRDT_"):]) == val
    for mod in (cg.orswot, cg.map, cg.mvreg, cg.vclock, cg.gcounter, cg.pncounter, cg.gset):
        assert callable(mod.reindex)
    for fn in ("index_map", "rows", "bitmaps"):
        assert callable(getattr(cg.reindex, fn))


def test_abi_version_still_8_and_symbols_exported():
    import crdts_gpu._abi as abi
    assert re.search(r"^#define\s+CRDT_ABI_VERSION\s+8\s*$", open(HEADER).read(), re.M)
    assert abi.CRDT_ABI_VERSION == 8
    lib = ctypes.CDLL(abi.LIB_PATH)
    assert lib.crdt_abi_version() == 8
    for name in API:
        assert hasattr(lib, name), name


def test_rust_ffi_carries_the_declarations():
    src = open(FFI).read()
    for name, n in API.items():
        m = re.search(r"pub fn " + name + r"\((.*?)\) -> c_int;", src, re.S)
        assert m, name
        assert len(m.group(1).split(", ")) == n + 1
    for name, val in BITS.items():
        assert re.search(r"pub const " + name + r": c_int = " + str(val) + ";", src), name


def test_numpy_gather_agrees_with_the_relabelled_objects():
    """The reference the GPU tests compare against, pinned to the oracle: the numpy gather of a replayed
    Orswot pool, read back as objects, is map_orswot of the same objects."""
    import eq_util as E
    import reindex_util as R
    from orswot_apply_util import map_orswot
    M, A, D = 33, 7, 6
    pool = E.orswot_pool(0x51, M, A)
    st = E.orswot_dense(pool, len(pool), M, A, D)
    fa, pa = R.insert_map(A, 3, seed=1)
    fm, pm = R.insert_map(M, 4, seed=2)
    got, status = R.orswot_reindex(st, fa, fm, M + 4, A + 3, D + 3)
    assert not status.any()
    assert got["clock"].shape == (len(pool), A + 3) and got["dset"].shape == (len(pool), D + 3, 1)
    assert any(o.deferred for o in pool) and any(o.entries for o in pool)
    for s, o in enumerate(pool):
        assert E.orswot_object(got, s) == map_orswot(o, lambda a: int(pa[a]), lambda m: int(pm[m]))
    # and back: the inverse maps restore the arrays
    back, status = R.orswot_reindex(got, R.inverse(fa, A), R.inverse(fm, M), M, A, D)
    assert not status.any()
    for k in st:
        assert np.array_equal(back[k], st[k]), k
    # a dropped actor / member that holds data is reported for exactly the states that hold it
    keep_a = np.array([a for a in range(A) if a != A - 1])
    _, status = R.orswot_reindex(st, keep_a, None, M, A - 1, D)
    held = np.array([(st["clock"][s, A - 1] != 0) or (st["entries"][s, :, A - 1] != 0).any()
                     or (st["dcl"][s, :st["cnt"][s], A - 1] != 0).any() for s in range(len(pool))])
    assert np.array_equal(status != 0, held) and held.any()
