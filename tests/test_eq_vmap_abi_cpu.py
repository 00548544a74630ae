"""CPU checks of the value-typed Maps' batched-equality surface: the three entry points are declared in
the header with both sides const, bound in _abi.py with matching argument counts, exported by the
library and carried by the Rust FFI file, CRDT_ABI_VERSION is still 8 (additions only), and the three
map.*_eq_batch wrappers exist."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crdt_gpu.h")
FFI = os.path.join(ROOT, "rust", "src", "gpu", "ffi.rs")

# name -> (number of arguments after ctx, the states struct of both sides)
EQ_API = {"crdt_map_counter_eq_batch": (5, "crdt_map_counter_states"),
          "crdt_map_orswot_eq_batch": (5, "crdt_map_orswot_states"),
          "crdt_map_nested_eq_batch": (5, "crdt_map_nested_states")}


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"{name} is not declared in include/crdt_gpu.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EQ_API))
def test_entry_point_declared_and_bound(name):
    import crdts_gpu._abi as abi
    n, states = EQ_API[name]
    args = header_args(name)
    assert args[0] == "crdt_ctx *ctx" and len(args) == n + 1
    assert args[1:] == [f"const {states} *x", "const crdt_map_deferred *xd", f"const {states} *y",
                        "const crdt_map_deferred *yd", "uint32_t *ne"]  # both sides read only
    assert name in abi.EXPORTS
    argtypes, restype = abi._SIGS[name]
    assert len(argtypes) == len(args) and restype is ctypes.c_int
    assert argtypes[1] is argtypes[3] and argtypes[2] is argtypes[4] is ctypes.POINTER(abi.MapDeferred)


def test_abi_version_still_8_and_symbols_exported():
    import crdts_gpu._abi as abi
    assert re.search(r"^#define\s+CRDT_ABI_VERSION\s+8\s*$", open(HEADER).read(), re.M)
    assert abi.CRDT_ABI_VERSION == 8
    lib = ctypes.CDLL(abi.LIB_PATH)
    assert lib.crdt_abi_version() == 8
    for name in EQ_API:
        assert hasattr(lib, name), name


def test_rust_ffi_carries_the_declarations():
    src = open(FFI).read()
    for name, (n, _) in EQ_API.items():
        m = re.search(r"pub fn " + name + r"\((.*?)\) -> c_int;", src, re.S)
        assert m, name
        assert len(m.group(1).split(", ")) == n + 1


def test_wrappers_exist():
    import crdts_gpu as cg
    for fn in ("counter_eq_batch", "orswot_eq_batch", "nested_eq_batch"):
        assert callable(getattr(cg.map, fn)), fn
