"""CPU checks of the value-typed Maps' read surface: the five entry points are declared, bound with
the right arity and exported, and the eight Python wrappers reject bad tensors before touching the
library."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crdt_gpu.h")

# name -> number of arguments after ctx
VMAP_READ_API = {"crdt_map_counter_get": 9, "crdt_map_orswot_get": 11, "crdt_map_orswot_contains": 9,
                 "crdt_map_nested_get": 10, "crdt_map_nested_get_inner": 13}
WRAPPERS = ("counter_get", "orswot_get", "orswot_contains", "nested_get", "nested_get_inner", "counter_read",
            "orswot_read", "nested_read")


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"{name} is not declared in include/crdt_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(VMAP_READ_API))
def test_vmap_read_entry_point_declared_and_bound(name):
    import crdts_gpu._abi as abi
    args = header_args(name)
    assert args[0] == "crdt_ctx *ctx" and len(args) == VMAP_READ_API[name] + 1
    assert name in abi.EXPORTS
    argtypes, restype = abi._SIGS[name]
    assert len(argtypes) == len(args) and restype is ctypes.c_int
    for a, t in zip(args, argtypes):  # pointers bind as pointers, sizes as size_t
        assert ("*" in a) == (t is not ctypes.c_size_t), (name, a)
    assert abi.CRDT_ABI_VERSION == 8  # additions only


def test_vmap_read_entry_points_exported_by_the_library():
    import crdts_gpu._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in VMAP_READ_API:
        assert hasattr(lib, name), name
    assert lib.crdt_abi_version() == 8
    src = open(HEADER).read()
    assert re.search(r"^#define\s+CRDT_ABI_VERSION\s+8\s*$", src, re.M)


def test_vmap_read_wrappers_exist():
    import crdts_gpu as cg
    for nm in WRAPPERS:
        assert callable(getattr(cg.map, nm)), nm


def _states(f, N=2, K=3, A=4, W=2, M=3, K2=3, Vs=8):
    """Counter, Orswot and nested Map states with every u64 tensor made by f(*shape)."""
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    counter = SimpleNamespace(clock=f(N, A), ec=f(N, K, A), val=f(N, K, W, A))
    orswot = SimpleNamespace(clock=f(N, A), ec=f(N, K, A), oc=f(N, K, A), ent=f(N, K, M, A), vd_n=i32(N, K))
    nested = SimpleNamespace(clock=f(N, A), ec=f(N, K, A), ic=f(N, K, A), iec=f(N, K, K2, A),
                             ivc=f(N, K, K2, Vs, A), ivv=f(N, K, K2, Vs), nval=i32(N, K, K2))
    return counter, orswot, nested


def _calls(states, idx, last=None):
    import crdts_gpu as cg
    c, o, n = states
    last = idx if last is None else last  # the last query vector of each call
    return [
        lambda: cg.map.counter_get(c, idx, last),
        lambda: cg.map.orswot_get(o, idx, last),
        lambda: cg.map.orswot_contains(o, idx, idx, last),
        lambda: cg.map.nested_get(n, idx, last),
        lambda: cg.map.nested_get_inner(n, idx, idx, last),
        lambda: cg.map.counter_read(c),
        lambda: cg.map.orswot_read(o),
        lambda: cg.map.nested_read(n),
    ]


def test_vmap_read_wrappers_reject_bad_tensors_before_the_library():
    """CPU tensors, wrong dtypes and a non-unit inner stride raise ValueError; none of these needs a
    device (no Context is created before the checks pass)."""
    idx = torch.zeros(2, dtype=torch.int32)
    ok64 = lambda *s: torch.zeros(s, dtype=torch.int64)  # noqa: E731
    for call in _calls(_states(ok64), idx):
        with pytest.raises(ValueError, match="cuda"):
            call()
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)  # noqa: E731
    for call in _calls(_states(f32), idx):
        with pytest.raises(ValueError, match="dtype"):
            call()
    for call in _calls(_states(ok64), idx, last=idx.long())[:5]:  # an int64 query vector
        with pytest.raises(ValueError, match="dtype"):
            call()
    wide = lambda *s: torch.zeros(s[:-1] + (2 * s[-1],), dtype=torch.int64)[..., ::2]  # noqa: E731
    st = _states(wide)
    assert st[0].ec.stride(-1) == 2
    for call in _calls(st, idx):
        with pytest.raises(ValueError, match="contiguous"):
            call()
