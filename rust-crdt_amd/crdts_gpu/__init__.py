"""crdts_gpu — MI355X batched CvRDT merge for the `crdts` (rust-crdt) data model.

Host-side mirror of the reference crate's merge surface (`CvRDT::merge`, traits.rs:4-7;
`FunkyCvRDT::merge` for LWWReg, traits.rs:49-55) in batched form: for each type module,
`lub_many` folds many replicas and `merge_batch` runs many pairwise merges, on dense
structure-of-arrays states in HBM, through libcrdt_gpu.so (include/crdt_gpu.h).
There is no CPU fallback: without the HIP library every call raises CrdtGpuUnavailable.
"""
from ._abi import CrdtGpuError, CrdtGpuUnavailable, load as load_library  # noqa: F401
from ._abi import (CRDT_NE_CLOCK as NE_CLOCK, CRDT_NE_ENTRIES as NE_ENTRIES, CRDT_NE_VALUES as NE_VALUES,  # noqa: F401
                   CRDT_NE_DEFERRED as NE_DEFERRED, CRDT_NE_INVALID as NE_INVALID)
from ._abi import (CRDT_REINDEX_DCAP as REINDEX_DCAP, CRDT_REINDEX_DROPPED as REINDEX_DROPPED,  # noqa: F401
                   CRDT_REINDEX_INVALID as REINDEX_INVALID, CRDT_REINDEX_VALUES as REINDEX_VALUES)
from .context import Context, synth_fill  # noqa: F401
from ._lattice import lub_many_multi  # noqa: F401
from .readctx import AddCtx, ReadCtx, RmCtx, derive_add_ctx, derive_rm_ctx  # noqa: F401
from . import apply, causal, gcounter, gset, host, intern, lwwreg, map, mvreg, orswot, pncounter, readctx, reindex, shard, synth, vclock, wire  # noqa: F401

__version__ = "0.1.0"
