"""CPU checks of the read API's surface: the six entry points are declared, bound with the right
arity and exported, and the Python wrappers reject bad tensors before touching the library."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crdt_gpu.h")

# name -> number of arguments after ctx
READ_API = {"crdt_orswot_read": 8, "crdt_map_read": 8, "crdt_orswot_contains": 13, "crdt_mvreg_read": 5,
            "crdt_map_get": 11, "crdt_vclock_derive_add": 9}


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"{name} is not declared in include/crdt_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(READ_API))
def test_read_entry_point_declared_and_bound(name):
    import crdts_gpu._abi as abi
    args = header_args(name)
    assert args[0] == "crdt_ctx *ctx" and len(args) == READ_API[name] + 1
    assert name in abi.EXPORTS
    argtypes, restype = abi._SIGS[name]
    assert len(argtypes) == len(args) and restype is ctypes.c_int
    for a, t in zip(args, argtypes):  # pointers bind as pointers, sizes as size_t
        assert ("*" in a) == (t is not ctypes.c_size_t), (name, a)
    assert abi.CRDT_ABI_VERSION == 8  # additions only


def test_read_entry_points_exported_by_the_library():
    import crdts_gpu._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in READ_API:
        assert hasattr(lib, name), name


def test_readctx_types_exported():
    import crdts_gpu as cg
    assert cg.ReadCtx._fields == ("add_clock", "rm_clock", "val")
    assert cg.AddCtx._fields == ("clock", "actor", "counter", "status") and cg.RmCtx._fields == ("clock",)
    t = torch.zeros((2, 3), dtype=torch.int64)
    rc = cg.ReadCtx(t, t, None)
    assert cg.derive_rm_ctx(rc).clock is t  # no kernel, no device
    for fn in (cg.orswot.read, cg.orswot.contains, cg.mvreg.read, cg.map.read, cg.map.get, cg.derive_add_ctx):
        assert callable(fn)


class _Map:
    def __init__(self, clock, ec, vclk, vval):
        self.clock, self.ec, self.vclk, self.vval = clock, ec, vclk, vval


def _calls(clock, entries, vclk, vval, idx):
    import crdts_gpu as cg
    return [
        lambda: cg.orswot.read(clock, entries),
        lambda: cg.orswot.contains(clock, entries, idx, idx),
        lambda: cg.map.read(clock, entries),
        lambda: cg.map.get(_Map(clock, entries, vclk, vval), idx, idx),
        lambda: cg.mvreg.read(vclk[0], vval[0]),
        lambda: cg.derive_add_ctx(cg.ReadCtx(clock, clock, None), idx),
    ]


def test_wrappers_reject_bad_tensors_before_the_library():
    """Wrong dtype, non-unit inner stride and CPU tensors raise ValueError; none of these needs a
    device (no Context is created before the checks pass)."""
    N, M, A, V = 2, 3, 4, 2
    ok64 = lambda *s: torch.zeros(s, dtype=torch.int64)  # noqa: E731
    clock, entries, vclk, vval = ok64(N, A), ok64(N, M, A), ok64(N, M, V, A), ok64(N, M, V)
    idx = torch.zeros(N, dtype=torch.int32)
    # CPU tensors of the right dtype and layout
    for call in _calls(clock, entries, vclk, vval, idx):
        with pytest.raises(ValueError, match="cuda"):
            call()
    # wrong dtypes (checked before the device)
    f = lambda t: t.to(torch.float32)  # noqa: E731
    for call in _calls(f(clock), f(entries), f(vclk), f(vval), idx):
        with pytest.raises(ValueError, match="dtype"):
            call()
    import crdts_gpu as cg
    for call in (lambda: cg.orswot.contains(clock, entries, idx.long(), idx),
                 lambda: cg.map.get(_Map(clock, entries, vclk, vval), idx, idx.long()),
                 lambda: cg.derive_add_ctx(cg.ReadCtx(clock, clock, None), idx.to(torch.int16))):
        with pytest.raises(ValueError, match="dtype"):
            call()
    # non-unit inner stride
    wide = lambda *s: torch.zeros(s[:-1] + (2 * s[-1],), dtype=torch.int64)[..., ::2]  # noqa: E731
    sc, se, svc, svv = wide(N, A), wide(N, M, A), wide(N, M, V, A), wide(N, M, V)
    assert se.stride(-1) == 2
    for call in _calls(sc, se, svc, svv, idx):
        with pytest.raises(ValueError, match="contiguous"):
            call()
