"""CPU checks of the batched-equality surface: the three entry points and the five CRDT_NE_* values
are declared in the header, bound in _abi.py with matching argument counts, exported by the library
and carried by the Rust FFI file, with CRDT_ABI_VERSION still 8 (additions only)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crdt_gpu.h")
FFI = os.path.join(ROOT, "rust", "src", "gpu", "ffi.rs")

# name -> number of arguments after ctx
EQ_API = {"crdt_mvreg_eq_batch": 3, "crdt_orswot_eq_batch": 3, "crdt_map_eq_batch": 5}
NE = {"CRDT_NE_CLOCK": 1, "CRDT_NE_ENTRIES": 2, "CRDT_NE_VALUES": 4, "CRDT_NE_DEFERRED": 8, "CRDT_NE_INVALID": 16}


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"{name} is not declared in include/crdt_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EQ_API))
def test_eq_entry_point_declared_and_bound(name):
    import crdts_gpu._abi as abi
    args = header_args(name)
    assert args[0] == "crdt_ctx *ctx" and len(args) == EQ_API[name] + 1
    assert args[-1] == "uint32_t *ne" and all(a.startswith("const ") for a in args[1:-1])  # both sides read only
    assert name in abi.EXPORTS
    argtypes, restype = abi._SIGS[name]
    assert len(argtypes) == len(args) and restype is ctypes.c_int


def test_ne_values_in_header_bindings_and_package():
    import crdts_gpu as cg
    import crdts_gpu._abi as abi
    src = open(HEADER).read()
    for name, val in NE.items():
        assert re.search(r"^#define\s+" + name + r"\s+" + str(val) + r"u\s", src, re.M), name
        assert getattr(abi, name) == val
        assert getattr(cg, name[len("CRDT_"):]) == val
    for mod in (cg.mvreg, cg.orswot, cg.map):
        assert callable(mod.eq_batch)


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
    for name, n in EQ_API.items():
        m = re.search(r"pub fn " + name + r"\((.*?)\) -> c_int;", src, re.S)
        assert m, name
        assert len(m.group(1).split(", ")) == n + 1
    for name, val in NE.items():
        assert re.search(r"pub const " + name + r": c_int = " + str(val) + ";", src), name
