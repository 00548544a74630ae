/*
 * crdt_gpu.h — C ABI of the MI355X batched CvRDT merge engine (libcrdt_gpu.so).
 *
 * Drop-in boundary for the `crdts` 3.0.0 (rust-crdt) state-merge path.  The reference
 * exposes one merge per pair of states:
 *
 *     CvRDT::merge(&mut self, other: Self)                      traits.rs:4-7
 *     FunkyCvRDT::merge(&mut self, other) -> Result<(), Error>  traits.rs:49-55 (LWWReg)
 *
 * and users fold it over replicas (`acc.merge(r)` loops, test/orswot.rs:50-53,
 * pncounter.rs:151-154).  This library adds the batched forms a `gpu` module of the
 * crate binds through `extern "C"` (see INTEGRATION.md for the Rust / ctypes stubs):
 *
 *     *_lub_many    — G independent left folds, each over R replicas  (acc = T::new(); for r: acc.merge(r))
 *     *_merge_batch — N independent pairwise merges, self[i].merge(other[i]), in place
 *
 * States are dense structure-of-arrays in device memory (HBM): actors/members are interned
 * to dense indices by the caller, an absent actor is a 0 counter (exact: VClock::apply_dot
 * never stores 0, vclock.rs:155-159).  All pointers are DEVICE pointers unless stated or the
 * ctx is in CRDT_MEM_HOST mode (crdt_ctx_set_mem_kind below).
 * Every stride is in 64-bit words.  Results are bit-exact against the reference fold.
 *
 * Conventions
 *   - Return value: CRDT_OK (0) or a negative status; crdt_last_error() has the text.
 *     No C++ exception crosses this ABI.  LWW marker conflicts are DATA, not a status.
 *   - Calls are stream-ordered on the ctx's stream and asynchronous unless stated.
 *     The caller owns every buffer; the library keeps no pointer past return.
 *   - One ctx per host thread; a ctx is bound to one device.
 */
#ifndef CRDT_GPU_H
#define CRDT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define CRDT_OK 0
#define CRDT_EINVAL -1       /* bad argument (null pointer, zero dim, stride < width, ...) */
#define CRDT_EHIP -2         /* a HIP runtime call failed                                   */
#define CRDT_ENOMEM -3       /* device scratch allocation failed                            */
#define CRDT_EUNSUPPORTED -4 /* shape the kernels do not handle                             */
#define CRDT_ECOMM -5        /* an RCCL call failed (sharded entry points)                  */

/* ---- flags for *_lub_many ---------------------------------------------------------- */
/* out := out ⊔ fold(in) instead of out := fold(in): i.e. `self.merge(r)` for every r,
 * starting from the caller's current state rather than from T::new(). */
#define CRDT_ACCUMULATE 0x1u

typedef struct crdt_ctx crdt_ctx;

/* ---- context ------------------------------------------------------------------------- */
/* Create a ctx bound to HIP device `device` (>= 0).  Scratch is owned by the ctx. */
int crdt_ctx_create(int device, crdt_ctx **out);
int crdt_ctx_destroy(crdt_ctx *ctx);
/* Launch on `hip_stream` (a hipStream_t; NULL = the device's null stream). */
int crdt_ctx_set_stream(crdt_ctx *ctx, void *hip_stream);
/* Block until all work issued through ctx has finished. */
int crdt_ctx_synchronize(crdt_ctx *ctx);
/* Text of the last failure on this ctx (static storage owned by ctx). ctx may be NULL. */
const char *crdt_last_error(const crdt_ctx *ctx);
/* Library version, e.g. "0.6.0"; and the gfx target the code objects were built for. */
const char *crdt_version(void);
/* ABI revision of this header: bumped whenever a struct or signature changes incompatibly (round 5
 * appended `size_t Dv` to crdt_map_orswot_batch: revision 5 -> 6; round 6 appended `size_t Vd` to
 * crdt_map_orswot_states / crdt_map_orswot_out and `size_t Id` to crdt_map_nested_states /
 * crdt_map_nested_out: 7 -> 8).  A caller checks
 * crdt_abi_version() == CRDT_ABI_VERSION of the header it was built against before any other call,
 * so a mismatched library fails clearly instead of reading a shorter struct. */
#define CRDT_ABI_VERSION 8
int crdt_abi_version(void);
const char *crdt_build_target(void);

/* Per-kernel timing with HIP events recorded on the ctx stream around the DOMINANT kernel of
 * each call (the replica stream pass).  Enabling costs two event records per call. */
int crdt_ctx_set_timing(crdt_ctx *ctx, int enable);
/* Sum of elapsed ms and launch count for kernel class `name` ("lub_stream", "orswot_join",
 * "lww_reduce", ...) since the last reset.  Synchronises the ctx stream. */
int crdt_ctx_timing(crdt_ctx *ctx, const char *name, double *total_ms, uint64_t *launches);
int crdt_ctx_timing_reset(crdt_ctx *ctx);
/* Override launch-geometry knobs ("key=value,...", the CRDT_TUNE syntax read at create; see
 * DESIGN.md §3).  Results never depend on them; tests use it to exercise every staging path. */
int crdt_ctx_tune(crdt_ctx *ctx, const char *spec);

/* ---- memory kind (crdt_mem_kind) ---------------------------------------------------------
 * CRDT_MEM_DEVICE (default): every buffer pointer is a device pointer and calls are
 * asynchronous on the ctx stream.  CRDT_MEM_HOST: the buffers of
 *     crdt_{vclock,gcounter,pncounter,gset}_lub_many / _merge_batch,
 *     crdt_lwwreg_lub_many / _merge_batch,
 *     crdt_orswot_lub_many / _merge_batch, crdt_map_lub_many / _merge_batch (every pointer in
 *     the structs; def_off stays host)
 * are HOST pointers (pageable, or pinned by crdt_host_alloc for direct DMA).  The lub_many forms
 * stream them through two ctx-owned device chunk buffers (tune key stage_kb, default 256 MiB
 * each), overlapping the H2D copy of chunk k+1 with the fold of chunk k: lattice / LWW folds
 * accumulate; Orswot joins each chunk into a running join kept in HBM and settles the deferred
 * removes once at the end; Map folds each chunk behind the running fold as its replica 0 (its
 * surviving removes carried along), falling back to whole-batch staging when a key needs more than
 * 8 value slots mid-fold.  merge_batch of Orswot / Map stages the whole batch.  The call returns when
 * the results are in host memory.  Results are identical to the device-pointer call.  In host mode
 * crdt_lwwreg_lub_many needs out_marker and out_val; a device pointer is rejected (CRDT_EINVAL);
 * every other entry point returns CRDT_EUNSUPPORTED. */
#define CRDT_MEM_DEVICE 0
#define CRDT_MEM_HOST 1
int crdt_ctx_set_mem_kind(crdt_ctx *ctx, int kind);
/* The ctx's current kind, or CRDT_EINVAL for a NULL ctx. */
int crdt_ctx_mem_kind(const crdt_ctx *ctx);
/* Page-locked host memory (hipHostMalloc): host-mode inputs in it are copied by DMA at the full
 * link rate.  Free with crdt_host_free. */
int crdt_host_alloc(size_t bytes, void **out);
int crdt_host_free(void *p);
/* Device memory on the ctx's GPU in one physically contiguous block (hipExtMallocWithFlags with
 * hipDeviceMallocContiguous), for the large replica batches a fold streams once: a batch in fewer,
 * larger page fragments is walked with fewer translation misses (config 3's 128 GiB Orswot input
 * folds in 20.4 ms from such a block against 21.4-22.9 ms from a torch allocator block on the same
 * box).  CRDT_ENOMEM when no such block is free (callers fall back to any device
 * memory).  Free with crdt_device_free (its ctx may be NULL). */
int crdt_device_alloc(crdt_ctx *ctx, size_t bytes, void **out);
int crdt_device_free(crdt_ctx *ctx, void *p);

/* ---- VClock / GCounter: elementwise-max lub ----------------------------------------------
 * Replaces VClock::merge (vclock.rs:130-136, via apply_dot :155-159) and GCounter::merge
 * (gcounter.rs:44-48) folded over replicas.
 * Replica (g, r) row = in + g*group_stride + r*row_stride, A counters contiguous.
 * Output row g = out + g*out_stride.                                                    */
int crdt_vclock_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                         size_t row_stride, size_t group_stride, uint64_t *out,
                         size_t out_stride, unsigned flags);
/* self[i] := self[i] ⊔ other[i] for i < N (rows of A counters). */
int crdt_vclock_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                            size_t A, size_t self_stride, size_t other_stride);
int crdt_gcounter_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                           size_t row_stride, size_t group_stride, uint64_t *out,
                           size_t out_stride, unsigned flags);
int crdt_gcounter_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                              size_t A, size_t self_stride, size_t other_stride);

/* ---- PNCounter: dual max ---------------------------------------------------------------
 * Replaces PNCounter::merge (pncounter.rs:70-75).  A replica row holds 2*A words:
 * P counters in [0, A), N counters in [A, 2A).  Strides as for VClock (row_stride >= 2A). */
int crdt_pncounter_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                            size_t row_stride, size_t group_stride, uint64_t *out,
                            size_t out_stride, unsigned flags);
int crdt_pncounter_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other,
                               size_t N, size_t A, size_t self_stride, size_t other_stride);

/* ---- GSet: bitmap union ----------------------------------------------------------------
 * Replaces GSet::merge (gset.rs:38-40 → insert :69-71).  Elements are interned to bit
 * positions; a replica row is `words` u64 words (bit u of word u/64 = element u present). */
int crdt_gset_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t words,
                       size_t row_stride, size_t group_stride, uint64_t *out,
                       size_t out_stride, unsigned flags);
int crdt_gset_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                          size_t words, size_t self_stride, size_t other_stride);

/* ---- several lattice lubs in one launch ------------------------------------------------------
 * Each segment is one crdt_{vclock,gcounter,pncounter,gset}_lub_many call (same dims, strides,
 * flags and result); segments of the same join (max: VClock / GCounter / PNCounter; or: GSet)
 * run in ONE launch (up to 8 per launch), so a batch of CRDT states of several types pays one
 * launch ramp and tail.  A = counters per replica (PNCounter: per half) or words (GSet). */
#define CRDT_KIND_VCLOCK 1
#define CRDT_KIND_GCOUNTER 2
#define CRDT_KIND_PNCOUNTER 3
#define CRDT_KIND_GSET 4
typedef struct crdt_lub_segment {
  int kind; /* CRDT_KIND_* */
  const uint64_t *in;
  size_t G, R, A, row_stride, group_stride;
  uint64_t *out;
  size_t out_stride;
  unsigned flags;
} crdt_lub_segment;
int crdt_lub_many_multi(crdt_ctx *ctx, const crdt_lub_segment *segs, size_t nseg);

/* ---- LWWReg<u64 val, u64 marker> -------------------------------------------------------
 * Replaces FunkyCvRDT::merge for LWWReg (lwwreg.rs:43-45 → update :84-98).
 * lub_many folds group g as acc = replica[g][0]; for r in 1..R: acc.merge(replica[g][r]),
 * where an erroring merge leaves acc unchanged (exactly what update does on Err).
 * Outputs: out_marker[g], out_val[g] = the folded state (max marker, val of the FIRST
 * replica holding it); first_conflict[g] = index r of the first merge that returns
 * Err(ConflictingMarker) in that fold, or UINT64_MAX if none.  Any of the three outputs
 * may be NULL.  Inputs: marker/val at [g*group_stride + r].
 * flags = CRDT_ACCUMULATE: acc starts at the caller's state (out_marker[g], out_val[g], both
 * required) and every replica 0..R-1 is merged into it (R may then be 0). */
int crdt_lwwreg_lub_many(crdt_ctx *ctx, const uint64_t *marker, const uint64_t *val, size_t G,
                         size_t R, size_t group_stride, uint64_t *out_marker,
                         uint64_t *out_val, uint64_t *first_conflict, unsigned flags);
/* self[i].merge(other[i]) for i < N; conflict[i] = 1 where it returns Err (state then
 * unchanged), else 0.  conflict may be NULL. */
int crdt_lwwreg_merge_batch(crdt_ctx *ctx, uint64_t *self_marker, uint64_t *self_val,
                            const uint64_t *other_marker, const uint64_t *other_val,
                            size_t N, uint8_t *conflict);

/* Batched FunkyCmRDT::apply of LWWReg (lwwreg.rs:48-57: the op is a whole register, applied through
 * update, :84-98).  Register i applies ops [op_off[i], op_off[i+1]) in order: a larger marker
 * replaces the state, an equal marker with a different value is Err(ConflictingMarker) and leaves
 * it unchanged, anything else is a no-op.  Markers compare as unsigned 64-bit over the full range.
 * Streams are ragged; an empty range leaves the register bit-identical.
 * conflict[o] (device u8, may be NULL) = 1 where op o returned Err, else 0; written for every op of
 * every register with a valid range.  status[i] (device u32, may be NULL; written for every i):
 * bit 0 = some op of the register returned Err; bit 3 = op_off[i] > op_off[i+1] or op_off[i+1] >
 * n_ops: the register is untouched and its conflict bytes are not written.  As in
 * crdt_mvreg_apply_batch a register with a valid range of its own is applied over that range
 * whatever its neighbours' offsets are; where two registers' ranges overlap, the conflict byte of an
 * op in both is unspecified.  Device memory only.  One wave per 64 registers, a segmented scan over
 * their contiguous op range (csrc/lwwreg_apply.hip). */
typedef struct crdt_lwwreg_ops {
  size_t n_ops;
  const uint64_t *op_off;  /* [N+1]   */
  const uint64_t *marker;  /* [n_ops] */
  const uint64_t *val;     /* [n_ops] */
} crdt_lwwreg_ops;

int crdt_lwwreg_apply_batch(crdt_ctx *ctx, uint64_t *marker /* [N] */, uint64_t *val /* [N] */, size_t N,
                            const crdt_lwwreg_ops *ops, uint8_t *conflict /* [n_ops] or NULL */,
                            uint32_t *status /* [N] or NULL */);

/* ---- Orswot<member, actor> ---------------------------------------------------------------
 * Replaces Orswot::merge (orswot.rs:81-149) incl. apply_rm (:230-250) and apply_deferred
 * (:281-286).
 * Exact for ANY input states: the result is the left fold acc = Orswot::new(); for r in replicas
 * { acc.merge(r) }, removes included.  On the reference's own invariants (entry dots covered by
 * their replica's clock, E <= C, as every state its API builds) the per-cell join is associative
 * and the kernels fold replica slices in any grouping; where an input cell has E > C (e.g. a
 * deserialized state) the unit holding it is re-folded in replica order inside the same launch,
 * and applying the deferred removes after the in-order join equals applying them at their own
 * step.  The host-memory mode continues the fold chunk by chunk, the sharded form
 * folds the ranks in rank order when any shard holds such a cell (below).
 * Dense layout per replica (g, r):
 *   clock   C[g][r][a]      at clock   + g*clock_gstride + r*clock_rstride + a
 *   entries E[g][r][m][a]   at entries + g*entry_gstride + r*entry_rstride + m*entry_mstride + a
 *                            (E = the member's dot clock; member absent <=> row all 0)
 *   deferred removes, pooled per group (CSR): group g owns d in [def_off[g], def_off[g+1]);
 *     rm clock  def_clock[d*A + a], member set bitmap def_members[d*Mw + w], Mw = ceil(M/64).
 *     def_off is a HOST array of G+1 entries (crdt_orswot_lub_many_doff below: a device one).
 * Output per group g: out_clock[g*A + a], out_entries[g*M*A + m*A + a] (packed), and for the
 * deferred pool: out_def_keep[d] = 1 iff d is the representative of a surviving deferred
 * remove (¬(rm ≤ final clock), first of its group with that exact clock), and
 * out_def_members[d*Mw + w] = union of the member sets of every surviving deferred of the
 * group with the same clock (only meaningful where out_def_keep[d] = 1). */
typedef struct crdt_orswot_batch {
  size_t G, R, M, A;
  const uint64_t *clock;
  size_t clock_rstride, clock_gstride;
  const uint64_t *entries;
  size_t entry_mstride, entry_rstride, entry_gstride;
  const size_t *def_off; /* host, G+1 entries; NULL or all-zero = no deferred removes */
  const uint64_t *def_clock;
  const uint64_t *def_members;
} crdt_orswot_batch;

typedef struct crdt_orswot_out {
  uint64_t *clock;       /* [G][A]    */
  uint64_t *entries;     /* [G][M][A] */
  uint8_t *def_keep;     /* [D]       */
  uint64_t *def_members; /* [D][Mw]   */
} crdt_orswot_out;

int crdt_orswot_lub_many(crdt_ctx *ctx, const crdt_orswot_batch *in, crdt_orswot_out *out);
/* crdt_orswot_lub_many with the deferred pool's CSR offsets in DEVICE memory (a pool built on the
 * GPU, e.g. by crdt_orswot_ingest, needs no host round trip): in->def_off must be NULL; def_off
 * (device u64 [G+1], or NULL = no deferred removes) with def_off[G] == D, the pool length (the rows
 * of def_clock / def_members, known to the caller from its own allocation).  The offsets are checked
 * on the device: def_off[0] != 0, def_off[G] != D, an entry > D or a decreasing step set bit 0 of
 * *status (device u32, written for every call; may be NULL) and the kernels then read the offsets
 * clamped to [0, D] (in bounds; the results are unreliable).  Device-memory contexts only
 * (CRDT_EUNSUPPORTED otherwise). */
int crdt_orswot_lub_many_doff(crdt_ctx *ctx, const crdt_orswot_batch *in, const uint64_t *def_off, size_t D,
                              crdt_orswot_out *out, uint32_t *status);

/* Batched Orswot CmRDT::apply (orswot.rs:55-79 with apply_rm :230-250 and apply_deferred
 * :281-286): state s < N applies its ops [op_off[s], op_off[s+1]) in order, in place.
 * State layout (device): clock C[s][a] at clock + s*clock_stride + a; entries E[s][m][a] at
 * entries + s*entry_sstride + m*entry_mstride + a (member absent <=> row all 0); the deferred
 * list of state s has def_count[s] <= Dcap slots, slot d holding the rm clock
 * def_clock[(s*Dcap + d)*A + a] and the member bitmap def_members[(s*Dcap + d)*Mw + w],
 * Mw = ceil(M/64), clocks pairwise distinct (the reference's HashMap<VClock, HashSet<M>>).
 * Ops (device): kind[o] 0 = Op::Add { dot: (actor[o], counter[o]), members },
 * 1 = Op::Rm { clock: rm_clock[rm_row[o]*A ..], members }; members of op o are
 * mem[mem_off[o] .. mem_off[o+1]) (u32 member indices, duplicates allowed).  op_off has N+1
 * entries, mem_off n_ops+1.  actor/counter may be NULL if no op is an Add, rm_row/rm_clock if
 * none is an Rm (n_rm_rows = rows of rm_clock).
 * status[s] (device u32, written for every s): bit 0 = the deferred list needed more than Dcap
 * slots (the state is incomplete: retry with a larger Dcap), bit 1 = an op named an actor,
 * member or rm row out of range or a bad kind / member range (reversed, or ending past n_mem)
 * (that op, or its bad members, were skipped), bit 2 = def_count[s] > Dcap on input, bit 3 = op_off[s..s+1] invalid (bits 2 and 3:
 * state left untouched).  Limits: A <= 1024 (1, 4 or 16 clock words per lane; the first slots of
 * the deferred list are kept in LDS, as many as 64 KiB holds; the rest stay in the state's own
 * slots, so Dcap is not bounded). */
typedef struct crdt_orswot_states {
  size_t N, M, A, Dcap;
  uint64_t *clock;
  size_t clock_stride;
  uint64_t *entries;
  size_t entry_mstride, entry_sstride;
  uint64_t *def_clock;   /* [N][Dcap][A]  */
  uint64_t *def_members; /* [N][Dcap][Mw] */
  uint32_t *def_count;   /* [N]           */
} crdt_orswot_states;

typedef struct crdt_orswot_ops {
  size_t n_ops;
  const uint64_t *op_off; /* [N+1]     */
  const uint8_t *kind;    /* [n_ops]   */
  const uint32_t *actor;  /* [n_ops]   */
  const uint64_t *counter; /* [n_ops]  */
  const uint32_t *rm_row; /* [n_ops]   */
  const uint64_t *rm_clock; /* [n_rm_rows][A] */
  size_t n_rm_rows;
  const uint64_t *mem_off; /* [n_ops+1] */
  const uint32_t *mem;      /* [n_mem]   */
  size_t n_mem;             /* entries of mem: a member range ending past it is malformed */
} crdt_orswot_ops;

int crdt_orswot_apply_batch(crdt_ctx *ctx, const crdt_orswot_states *states, const crdt_orswot_ops *ops,
                            uint32_t *status);

/* Pairwise in-place Orswot merge (the batched form of CvRDT::merge, traits.rs:4-7 ->
 * Orswot::merge orswot.rs:81-149 with apply_rm :230-250 and apply_deferred :281-286):
 * self[i].merge(other[i]) for i < N, exact for ANY pair of states.  Both sides use the
 * crdt_orswot_states layout (the apply layout: per-state deferred slots, clocks pairwise distinct
 * within a state); N, M and A must match, Dcap may differ.  self's clock, entries, deferred slots
 * and def_count are rewritten; other is read only (its def_count may be NULL when its Dcap is 0).
 * The surviving deferred removes (!(rm <= merged clock)) of both sides are compacted into self's
 * slots (self's survivors first, in slot order, then other's; identical clocks merge their member
 * sets, as the reference's HashMap<VClock, HashSet<M>> does).
 * status[s] (device u32): bit 0 = more survivors than self's Dcap (state incomplete), bit 2 =
 * def_count above Dcap on input (state untouched).  Dcap is not bounded: a pair with more than
 * 512 removes is forgotten in further passes of 512 (forgets compose and commute). */
int crdt_orswot_merge_batch(crdt_ctx *ctx, const crdt_orswot_states *self, const crdt_orswot_states *other,
                            uint32_t *status);

/* ---- batched Causal::forget of whole states -----------------------------------
 * State s forgets the clock y + s*y_stride (y_stride = 0: one clock for every state), in place.
 * Orswot::forget (orswot.rs:150-183): clock, entry clocks (an emptied entry = all-zero row =
 *     dropped) and deferred rm clocks.  Deferred removes are a pool of D rows: row d belongs to
 *     state def_state[d] (device u32); def_keep[d] = 0 iff its rm clock emptied (dropped by the
 *     reference, :168-180); member sets are untouched.  When two surviving rm clocks of one state
 *     become equal the reference's HashMap collect keeps ONE of them with its own member set,
 *     chosen by hash iteration order (unspecified); both rows are kept here.  Rows with
 *     def_state[d] >= N are left untouched (def_keep[d] = 1).
 * Map::forget (map.rs:85-114) with V = MVReg: entry clocks, every value clock (MVReg::forget
 *     mvreg.rs:88-104: an emptied value is dropped: slot clock all 0, value 0), an entry whose own
 *     clock empties is dropped with its values, deferred rm clocks as for Orswot, the map clock.
 *     Layout (device, per state s): clock + s*clock_stride; ec + s*ec_stride + k*A;
 *     vclk + s*vclk_stride + (k*V + j)*A; vval + s*vval_stride + k*V + j (the crdt_map_lub_many
 *     slot convention: empty slot <=> all-zero clock row, skipped on egress). */
int crdt_orswot_forget_batch(crdt_ctx *ctx, uint64_t *clock, size_t clock_stride, uint64_t *entries,
                             size_t entry_mstride, size_t entry_sstride, size_t N, size_t M, size_t A,
                             const uint64_t *y, size_t y_stride, uint64_t *def_clock,
                             const uint32_t *def_state, size_t D, uint8_t *def_keep);

typedef struct crdt_map_states {
  size_t N, K, A, V;
  uint64_t *clock;
  size_t clock_stride;
  uint64_t *ec;
  size_t ec_stride;
  uint64_t *vclk;
  size_t vclk_stride;
  uint64_t *vval;
  size_t vval_stride;
} crdt_map_states;

int crdt_map_forget_batch(crdt_ctx *ctx, const crdt_map_states *states, const uint64_t *y, size_t y_stride,
                          uint64_t *def_clock, const uint32_t *def_state, size_t D, uint8_t *def_keep);

/* Map::forget (map.rs:85-114) of whole value-typed Map states (round 5), in place, arguments as
 * crdt_map_forget_batch (one forget clock per state, the Map-level deferred rm clocks as a pool of
 * D rows with their states, def_keep[d] = 0 where one emptied):
 *  - Map<K, GCounter / PNCounter>: the crdt_map_counter_lub_many output layout per state s:
 *    clock + s*clock_stride, ec + s*ec_stride + k*A, val + s*val_stride + (k*W + w)*A; a dropped
 *    entry has all-zero rows; the counter rows forget word by word (gcounter.rs:51-53,
 *    pncounter.rs:78-81).
 *  - Map<K, Orswot<M>>: the crdt_map_orswot_lub_many output layout (packed; N states), the Orswot
 *    clock, member rows and nested deferred removes forgotten (orswot.rs:150-183): an emptied member
 *    row is absent, an emptied nested rm clock dropped, two that become equal keep one entry with the
 *    later one's members at the earlier one's place (the fold's rule; the reference's HashMap order is
 *    unspecified), and a dropped entry drops its nested removes (vd_n = 0).  A <= 1,024. */
typedef struct crdt_map_counter_states {
  size_t N, K, A, W;
  uint64_t *clock;
  size_t clock_stride;
  uint64_t *ec;
  size_t ec_stride;
  uint64_t *val;
  size_t val_stride;
} crdt_map_counter_states;

int crdt_map_counter_forget_batch(crdt_ctx *ctx, const crdt_map_counter_states *states, const uint64_t *y,
                                  size_t y_stride, uint64_t *def_clock, const uint32_t *def_state, size_t D,
                                  uint8_t *def_keep);

/* Batched Map<K, GCounter / PNCounter> CmRDT::apply (round 5; map.rs:119-137 with gcounter.rs:36-42 /
 * pncounter.rs:59-68, apply_keyset_rm :318-348, apply_deferred :311-316): state s applies its ops
 * [op_off[s], op_off[s+1]) in order, in place, on the crdt_map_counter_states layout; deferred
 * removes as crdt_map_apply_batch (def_count[s] <= Dcap slots, rm clock def_clock[(s*Dcap + d)*A + a],
 * key bitmap def_keys[(s*Dcap + d)*Kw + w]).  Ops: kind 0 = Op::Up { dot: (actor, counter), key,
 * op: the counter's op (vactor, vcounter) — a Dot — with vdir 0 = P (GCounter: always 0), 1 = N
 * (vdir may be NULL: all P) }, kind 1 = Op::Rm { clock: clk_pool[clk_row*A ..], keyset: keys[key_off[o]
 * .. key_off[o+1]) }.  status[s]: bit 0 = deferred slots exhausted, bit 1 = a malformed op / key
 * skipped, bits 2-3 = invalid input (state untouched).  Limits: A <= 512.  Dcap is not bounded:
 * during the stream the first min(Dcap, 16) slots live in LDS and the rest are used in place in
 * def_clock / def_keys (round 6: exact up to Dcap; bit 0 only past Dcap).  Slots the list vacates
 * during a call (a remove that became dominated) are written zero, so a state whose slots past
 * def_count were zero keeps them zero (the wire ingest's form); the same holds for the Orswot and
 * nested Map apply below. */
typedef struct crdt_map_counter_ops {
  size_t n_ops;
  const uint64_t *op_off;    /* [N+1]       */
  const uint8_t *kind;       /* [n_ops]     */
  const uint32_t *actor;     /* [n_ops] Up: the Map's dot */
  const uint64_t *counter;   /* [n_ops] Up  */
  const uint32_t *key;       /* [n_ops] Up  */
  const uint32_t *vactor;    /* [n_ops] Up: the counter's dot */
  const uint64_t *vcounter;  /* [n_ops] Up  */
  const uint8_t *vdir;       /* [n_ops] Up: 0 P, 1 N (or NULL) */
  const uint32_t *clk_row;   /* [n_ops] Rm  */
  const uint64_t *clk_pool;  /* [n_clk_rows][A] */
  size_t n_clk_rows;
  const uint64_t *key_off;   /* [n_ops+1] Rm */
  const uint32_t *keys;      /* [n_keys]    */
  size_t n_keys;
} crdt_map_counter_ops;

int crdt_map_counter_apply_batch(crdt_ctx *ctx, const crdt_map_counter_states *states, uint64_t *def_clock,
                                 uint64_t *def_keys, uint32_t *def_count, size_t Dcap,
                                 const crdt_map_counter_ops *ops, uint32_t *status);

typedef struct crdt_map_orswot_states {
  size_t N, K, M, A;
  uint64_t *clock;    /* [N][A]            */
  uint64_t *ec;       /* [N][K][A]         */
  uint64_t *oc;       /* [N][K][A]         */
  uint64_t *ent;      /* [N][K][M][A]      */
  uint32_t *vd_n;     /* [N][K]            */
  uint64_t *vd_clock; /* [N][K][Vd][A]     */
  uint64_t *vd_mem;   /* [N][K][Vd][Mw]    */
  size_t Vd;          /* nested deferred slots per key (round 6, ABI 8; 0 = 16) */
} crdt_map_orswot_states;

int crdt_map_orswot_forget_batch(crdt_ctx *ctx, const crdt_map_orswot_states *states, const uint64_t *y,
                                 size_t y_stride, uint64_t *def_clock, const uint32_t *def_state, size_t D,
                                 uint8_t *def_keep);

/* Batched Map<K, Orswot<M>> CmRDT::apply (round 5; map.rs:119-137 with Orswot::apply orswot.rs:55-79,
 * apply_rm :230-250 and apply_deferred :281-286 inside, the Map's apply_keyset_rm :318-348 with
 * Orswot::forget :150-183 and apply_deferred :311-316): state s applies its ops [op_off[s],
 * op_off[s+1]) in order, in place, on the crdt_map_orswot_states layout (nested deferred lists of
 * <= 16 per key); the Map's deferred removes as crdt_map_counter_apply_batch.  Ops: kind 0 = Op::Up
 * { dot: (actor, counter), key, op } with vkind 0 = Orswot Add { dot: (vactor, vcounter), members }
 * or 1 = Orswot Rm { clock: clk_pool[clk_row*A ..], members }, the members mems[mem_off[o] ..
 * mem_off[o+1]); kind 1 = Op::Rm { clock: clk_pool[clk_row*A ..], keyset: keys[key_off[o] ..
 * key_off[o+1]) } (key_off may be NULL when no op is a Map Rm).  status[s]: bit 0 = a deferred list
 * (the Map's or a nested one) exhausted, bit 1 = a malformed op / key / member skipped, bits 2-3 =
 * invalid input (state untouched).  Nested removes whose clocks become equal under a Map-level
 * forget keep one entry, the later one's members (the fold's rule).  Limits: A <= 512, M <= 1,024;
 * Dcap is not bounded (the Map's first min(Dcap, 16) slots in LDS, the rest in place, round 6). */
typedef struct crdt_map_orswot_ops {
  size_t n_ops;
  const uint64_t *op_off;    /* [N+1]       */
  const uint8_t *kind;       /* [n_ops]     */
  const uint32_t *actor;     /* [n_ops] Up: the Map's dot */
  const uint64_t *counter;   /* [n_ops] Up  */
  const uint32_t *key;       /* [n_ops] Up  */
  const uint8_t *vkind;      /* [n_ops] Up: 0 Orswot Add, 1 Orswot Rm */
  const uint32_t *vactor;    /* [n_ops] Up / Add: the Orswot's dot */
  const uint64_t *vcounter;  /* [n_ops] Up / Add */
  const uint32_t *clk_row;   /* [n_ops] Up / Rm and Map Rm: row of clk_pool */
  const uint64_t *clk_pool;  /* [n_clk_rows][A] */
  size_t n_clk_rows;
  const uint64_t *key_off;   /* [n_ops+1] Map Rm keysets */
  const uint32_t *keys;      /* [n_keys]    */
  size_t n_keys;
  const uint64_t *mem_off;   /* [n_ops+1] Up: the Orswot op's members */
  const uint32_t *mems;      /* [n_mems]    */
  size_t n_mems;
} crdt_map_orswot_ops;

int crdt_map_orswot_apply_batch(crdt_ctx *ctx, const crdt_map_orswot_states *states, uint64_t *def_clock,
                                uint64_t *def_keys, uint32_t *def_count, size_t Dcap,
                                const crdt_map_orswot_ops *ops, uint32_t *status);

/* Batched Map<K, MVReg<u64>> CmRDT::apply (map.rs:119-137, apply_keyset_rm :318-348,
 * apply_deferred :311-316, MVReg::apply mvreg.rs:130-166): state s applies its ops
 * [op_off[s], op_off[s+1]) in order, in place, on the crdt_map_states layout (value slots in Vec
 * order, empty slot <=> all-zero clock; an append goes after the last used slot, compacting the
 * slots when that one is the last).  Deferred removes: def_count[s] <= Dcap slots, rm clock
 * def_clock[(s*Dcap + d)*A + a], key bitmap def_keys[(s*Dcap + d)*Kw + w], Kw = ceil(K/64).
 * Ops: kind 0 = Op::Up { dot: (actor, counter), key, op: Put { clock: clk_pool[clk_row*A ..],
 * val } }, kind 1 = Op::Rm { clock: clk_pool[clk_row*A ..], keyset: keys[key_off[o] ..
 * key_off[o+1]) } (key_off: n_ops+1 entries, may be NULL when no op is an Rm).
 * status[s]: bit 0 = deferred slots exhausted, bit 1 = an out-of-range op / key skipped (incl. a
 * key range reversed or ending past n_keys),
 * bits 2-3 = invalid input (state untouched), bit 4 = a register needed more than V values (the
 * state is incomplete: retry with more slots), bit 5 = internal slot invariant violated (never
 * expected; the value was not written).  Limits: A <= 1024, V >= 1 (the value slots are walked in
 * HBM, so V is not bounded; the first deferred slots are kept in LDS, as many as 64 KiB holds; the
 * rest stay in the state's own slots). */
typedef struct crdt_map_ops {
  size_t n_ops;
  const uint64_t *op_off;   /* [N+1]       */
  const uint8_t *kind;      /* [n_ops]     */
  const uint32_t *actor;    /* [n_ops] Up  */
  const uint64_t *counter;  /* [n_ops] Up  */
  const uint32_t *key;      /* [n_ops] Up  */
  const uint64_t *val;      /* [n_ops] Up  */
  const uint32_t *clk_row;  /* [n_ops]     */
  const uint64_t *clk_pool; /* [n_clk_rows][A] */
  size_t n_clk_rows;
  const uint64_t *key_off;  /* [n_ops+1] Rm */
  const uint32_t *keys;     /* [n_keys]    */
  size_t n_keys;            /* entries of keys: a key range ending past it is malformed */
} crdt_map_ops;

int crdt_map_apply_batch(crdt_ctx *ctx, const crdt_map_states *states, uint64_t *def_clock, uint64_t *def_keys,
                         uint32_t *def_count, size_t Dcap, const crdt_map_ops *ops, uint32_t *status);

/* Deferred-remove slots of N Map states (the crdt_map_apply_batch convention): state s holds
 * count[s] <= Dcap removes, rm clock clock[(s*Dcap + d)*A + a], key bitmap keys[(s*Dcap + d)*Kw + w]. */
typedef struct crdt_map_deferred {
  uint64_t *clock;
  uint64_t *keys;
  uint32_t *count;
  size_t Dcap;
} crdt_map_deferred;

/* Pairwise in-place Map<K, MVReg<u64>> merge: self[i].merge(other[i]) for i < N (Map::merge
 * map.rs:140-220, MVReg::merge mvreg.rs:112-128, MVReg::forget :88-104, apply_keyset_rm
 * map.rs:318-348), exact for ANY pair of states, on the crdt_map_states layout (N, K, A equal on
 * both sides; V may differ; value slots in Vec order: self's kept values then other's added ones,
 * written from slot 0, empty slots zeroed).  Deferred removes as crdt_orswot_merge_batch over key
 * bitmaps.  status[s]: bit 0 = deferred slots exhausted, bit 2 = invalid def_count (untouched),
 * bit 4 = some register needed more than self's V slots (that key is incomplete).
 * Limits: A <= 1024, 1 <= V <= 64 on each side (Dcap is not bounded); a side past 32 slots takes
 * the generic one-wave-per-key kernel with 64-bit slot masks. */
int crdt_map_merge_batch(crdt_ctx *ctx, const crdt_map_states *self, const crdt_map_deferred *self_def,
                         const crdt_map_states *other, const crdt_map_deferred *other_def, uint32_t *status);

/* ---- multi-GPU: replica-sharded lub over RCCL ----------------------------
 * One process (one ctx) per GPU.  Rank 0 calls crdt_comm_unique_id and sends the 128 bytes to
 * every rank over the caller's own channel; every rank then calls crdt_ctx_comm_init (collective:
 * all ranks must call it).  The *_sharded calls are collective too: rank k passes its own replica
 * shard (same G and row width on every rank, any R_k >= 0) and every rank receives the global
 * lub, equal to lub_many over the concatenation of the shards.
 *   vclock / gcounter / pncounter: local lub_many + one ncclAllReduce(ncclUint64, ncclMax) of the
 *       packed G x W partials (W = A, 2A for PNCounter) — out is packed [G][W]
 *   gset: local lub_many + ncclAllGather of the partial bitmaps + OR-fold of the world partials
 *   orswot: local join without deferred removes, ncclAllGather of the partial (clock, entries),
 *       all ranks' deferred removes gathered and pooled per group (rank order, then local order),
 *       re-merge of the world partials with every deferred remove (orswot.rs:141-147).  If any
 *       rank's shard holds an entry cell with E > C (flags gathered with the deferred counts), the
 *       partials are not joined as a tree: rank k re-folds its shard starting from rank k-1's state,
 *       one all-gather per step (W-1 extra exchanges), and the re-merge reads the last rank's state —
 *       the left fold over the concatenated shards for any input.  Output:
 *       clock [G][A], entries [G][M][A], and the surviving deferred removes compacted: *ndef (host)
 *       = their number; the first min(*ndef, def_cap) are written as def_clock[d*A + a],
 *       def_members[d*Mw + w] (union over the survivors with that exact clock in the group) and
 *       def_group[d] (device u32), in group order.
 * The replaced reference operation is the same CvRDT::merge fold (traits.rs:4-7), split over
 * processes: a Rust caller would distribute the id over its own transport.
 *
 * Agreement: every *_sharded call first exchanges a small header (this rank's validation status
 * and the call's rank-uniform dims: G, row width, M / K, A, D ...) and only runs its data
 * collectives when every rank validated and the dims agree; otherwise EVERY rank returns an error
 * (CRDT_EINVAL: its own validation failed, or the ranks disagree; CRDT_ECOMM with "another rank"
 * in crdt_last_error: a peer's failed), so a bad argument on one rank never leaves the others
 * blocked in a collective.  The header exchange runs on a side stream while the local fold runs.
 *
 * The caller's own collectives instead of RCCL (crdt_ctx_comm_init_ops): every *_sharded call then
 * runs its exchange through these HOST callbacks on host buffers (the library copies device data
 * to host memory and back around each call, after draining its stream).  A transport seam for
 * callers with their own channel (MPI, TCP, a test harness) and for running the multi-rank code of
 * this file with several ranks on one GPU.  Callbacks return 0 on success; any other value makes
 * the sharded call return CRDT_ECOMM.
 *   allgather:     recv[r*bytes .. (r+1)*bytes) = rank r's `send` bytes, for every rank r
 *   allreduce_u64: buf[i] = op over the ranks of buf[i] (unsigned 64-bit; CRDT_RED_*) */
#define CRDT_UNIQUE_ID_BYTES 128
#define CRDT_RED_MAX 0
#define CRDT_RED_MIN 1
#define CRDT_RED_SUM 2
typedef struct crdt_comm_ops {
  void *user;
  int (*allgather)(void *user, const void *send, void *recv, size_t bytes);
  int (*allreduce_u64)(void *user, uint64_t *buf, size_t n, int op);
} crdt_comm_ops;
int crdt_comm_unique_id(uint8_t *id /* [CRDT_UNIQUE_ID_BYTES] */);
/* Collective.  RCCL is bound at run time (dlopen + dlsym, csrc/shard.hip), from ONE librccl.so.1:
 * $CRDT_RCCL_LIB when set, else the copy the process already has loaded (torch's own RCCL inside
 * a torch process, so the library and torch.distributed share one RCCL), else librccl.so.1 through
 * the library's RUNPATH (/opt/rocm/lib).  CRDT_ECOMM if none loads or it is older than 2.18. */
int crdt_ctx_comm_init(crdt_ctx *ctx, const uint8_t *id, int nranks, int rank);
/* Not collective (the callbacks are the caller's); ops is copied, its user pointer must stay
 * valid until crdt_ctx_comm_destroy. */
int crdt_ctx_comm_init_ops(crdt_ctx *ctx, const crdt_comm_ops *ops, int nranks, int rank);
int crdt_ctx_comm_destroy(crdt_ctx *ctx);
int crdt_ctx_comm_info(const crdt_ctx *ctx, int *nranks, int *rank);
/* The RCCL the ctx's communicator runs on, noted at comm init ("" before it / for caller ops), e.g.
 * "RCCL 2.26.6 (22606) at /.../librccl.so.1, already loaded by the process ..."; storage owned by
 * ctx.  *runtime = the bound RCCL's version code (0 if none binds), *header = the rccl.h version
 * the types were taken from (may be NULL). */
const char *crdt_ctx_comm_note(const crdt_ctx *ctx, int *runtime, int *header);
int crdt_vclock_lub_many_sharded(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                                 size_t row_stride, size_t group_stride, uint64_t *out);
int crdt_gcounter_lub_many_sharded(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                                   size_t row_stride, size_t group_stride, uint64_t *out);
int crdt_pncounter_lub_many_sharded(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                                    size_t row_stride, size_t group_stride, uint64_t *out);
int crdt_gset_lub_many_sharded(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t words,
                               size_t row_stride, size_t group_stride, uint64_t *out);

typedef struct crdt_orswot_sharded_out {
  uint64_t *clock;       /* [G][A]      */
  uint64_t *entries;     /* [G][M][A]   */
  size_t def_cap;        /* rows available below */
  uint64_t *def_clock;   /* [def_cap][A]  */
  uint64_t *def_members; /* [def_cap][Mw] */
  uint32_t *def_group;   /* [def_cap]     */
  size_t *ndef;          /* host: number of surviving deferred removes */
} crdt_orswot_sharded_out;

int crdt_orswot_lub_many_sharded(crdt_ctx *ctx, const crdt_orswot_batch *in, crdt_orswot_sharded_out *out);
/* crdt_orswot_lub_many_sharded with this rank's deferred-pool offsets in DEVICE memory (round 4):
 * in->def_off NULL, def_off device u64 [G+1] (or NULL when D == 0) with def_off[G] == D, D the
 * rank's pool length.  The per-group counts are taken on the device and travel in the exchange's
 * count row, so no host sync is added: the offsets are checked there too (def_off[0] == 0,
 * def_off[G] == D, non-decreasing), and an invalid entry on ANY rank makes every rank return
 * before a deferred row moves (CRDT_EINVAL on that rank, CRDT_ECOMM on the others). */
int crdt_orswot_lub_many_sharded_doff(crdt_ctx *ctx, const crdt_orswot_batch *in, const uint64_t *def_off, size_t D,
                                      crdt_orswot_sharded_out *out);
/* crdt_lub_many_multi over replica shards: one fused local launch, then ONE grouped RCCL call
 * (an in-place ncclMax all-reduce per max segment; GSet segments as crdt_gset_lub_many_sharded).
 * Outputs must be contiguous (out_stride == row words, or G == 1). */
int crdt_lub_many_multi_sharded(crdt_ctx *ctx, const crdt_lub_segment *segs, size_t nseg);

/* LWWReg (lwwreg.rs:43-45 -> update :84-98), replicas split in rank order: rank k holds replicas
 * [base_k, base_k + R_k) of every group (marker / val at [g*group_stride + r], R_k may be 0) and
 * passes its base_k.  Every rank receives the state of the GLOBAL left fold (out_marker[g],
 * out_val[g]) and first_conflict[g] = the global index of its first erroring merge (UINT64_MAX if
 * none; may be NULL): each rank continues the fold from the fold of the lower ranks' states, then a
 * MIN all-reduce.  Exchange: ncclAllGather of (G markers, G vals, R_k) + ncclAllReduce(ncclMin). */
int crdt_lwwreg_lub_many_sharded(crdt_ctx *ctx, const uint64_t *marker, const uint64_t *val, size_t G, size_t R,
                                 size_t group_stride, uint64_t base, uint64_t *out_marker, uint64_t *out_val,
                                 uint64_t *first_conflict);

/* ---- Map<K, MVReg<u64, A>, A> --------------------------------------------------------------
 * Replaces Map::merge (map.rs:140-220) with V = MVReg (MVReg::merge mvreg.rs:112-128,
 * MVReg::forget :88-104), incl. apply_keyset_rm (map.rs:318-348) and apply_deferred (:311-316),
 * folded as acc = Map::new(); for r in 0..R: acc.merge(replica[g][r]).  Exact for any input
 * (no associativity is assumed: each key is folded in replica order).
 * Dense layout per replica (g, r) — keys, actors and MVReg values interned by the caller:
 *   clock C[a]            at clock + g*clock_gstride + r*clock_rstride + a
 *   entry clocks EC[k][a] at ec    + g*ec_gstride    + r*ec_rstride    + k*A + a
 *                          (key absent <=> row all 0)
 *   value clocks VC[k][s][a] at vclk + g*vclk_gstride + r*vclk_rstride + (k*V + s)*A + a and
 *   values VV[k][s]         at vval + g*vval_gstride + r*vval_rstride + k*V + s, for the
 *                          s < V value slots of the key's MVReg in Vec order (slot empty <=>
 *                          clock row all 0; empty slots are skipped)
 *   deferred removes pooled per group (CSR): group g owns d in [def_off[g], def_off[g+1])
 *     (def_off a HOST array of G+1 entries; crdt_map_lub_many_doff: device), held by replica
 *     def_row[d] of the group (device u32, non-decreasing within the group, < R), rm clock
 *     def_clock[d*A + a], key bitmap
 *     def_keys[d*Kw + w], Kw = ceil(K/64).
 * Output per group g (packed): clock[g*A + a], ec[(g*K + k)*A + a], value slots s < Vout:
 * vclk[((g*K + k)*Vout + s)*A + a], vval[(g*K + k)*Vout + s]; nval[g*K + k] = number of values
 * (may be NULL); flags[g] (required): bit 0 = some key folded to more than Vout values (its
 * slots are then incomplete: retry with a larger Vout), bit 1 = def_row not non-decreasing or
 * >= R, bit 2 = the fold state of some key needed more values than it holds (results of the
 * group incomplete: retry with Vstate = 8), bit 3 = internal: a key wave waited past its bound
 * for the workgroup's shared clock-row ring (results of the group unreliable; never expected —
 * report it).  The state holds VO = 2*pow2(V') values, V' the
 * smallest power of two with V' >= V and 2V' >= min(8, max(Vout, Vstate)); VO <= 8.
 * Deferred output as for Orswot (def_keep / def_keys over keys).
 * Limits: A <= 1024, V <= 16, Vout <= 64.  With Vstate <= 16 the fold state holds up to 16 values per
 * key (bit 2 of flags when a key needs more).  17 <= Vstate <= 64 asks for the deep pass
 * (csrc/map_deep.hip): the fold runs as with Vstate = 0, the keys whose state overflows are marked
 * instead of reported, and a second kernel on the same stream folds each marked key again, exactly
 * and in replica order, with up to Vstate values held in LDS; bit 2 then means that a key needed more
 * than Vstate values at some step, bit 0 as before.  The deep pass needs about Vstate * A * 8 + 14 KiB
 * of LDS per key: past 160 KiB (Vstate = 64: A > 256) the call returns CRDT_EUNSUPPORTED before
 * anything is launched, as it does for Vstate > 64.  The sharded and CRDT_MEM_HOST entry points have
 * no deep pass: they treat Vstate > 16 as 16.  A > 256 or V > 8 runs the workgroup-per-key fold
 * (csrc/map_wide.hip: the same exact left fold, no speculative scan — a correctness path, not a
 * tuned one). */
typedef struct crdt_map_batch {
  size_t G, R, K, A, V;
  const uint64_t *clock;
  size_t clock_rstride, clock_gstride;
  const uint64_t *ec;
  size_t ec_rstride, ec_gstride;
  const uint64_t *vclk;
  size_t vclk_rstride, vclk_gstride;
  const uint64_t *vval;
  size_t vval_rstride, vval_gstride;
  const size_t *def_off; /* host, G+1 entries; NULL or all-zero = no deferred removes */
  const uint32_t *def_row;
  const uint64_t *def_clock;
  const uint64_t *def_keys;
} crdt_map_batch;

typedef struct crdt_map_out {
  size_t Vout;
  size_t Vstate; /* <= 16: value capacity hint for the fold state (0 = from Vout and V);
                    17..64: the deep pass with that many values per key (see Limits) */
  uint64_t *clock; /* [G][A]          */
  uint64_t *ec;    /* [G][K][A]       */
  uint64_t *vclk;  /* [G][K][Vout][A] */
  uint64_t *vval;  /* [G][K][Vout]    */
  uint32_t *nval;  /* [G][K] or NULL  */
  uint32_t *flags; /* [G]             */
  uint8_t *def_keep; /* [D]     */
  uint64_t *def_keys; /* [D][Kw] */
} crdt_map_out;

int crdt_map_lub_many(crdt_ctx *ctx, const crdt_map_batch *in, crdt_map_out *out);
/* crdt_map_lub_many with the deferred pool's CSR offsets in DEVICE memory, as for
 * crdt_orswot_lub_many_doff: in->def_off NULL, def_off device u64 [G+1] (or NULL) with
 * def_off[G] == D.  An invalid entry i (checked on the device, as there) sets bit 1 of flags[i-1]
 * and flags[i] (the groups whose range it bounds); the fold then reads the offsets clamped to
 * [0, D].  Device-memory contexts only. */
int crdt_map_lub_many_doff(crdt_ctx *ctx, const crdt_map_batch *in, const uint64_t *def_off, size_t D,
                           crdt_map_out *out);

/* Map<K, MVReg> sharded by KEYS: rank k holds keys [k0, k0 + in->K) of every
 * replica (the crdt_map_batch layout with K = its key count), every replica's clock and the group's
 * whole deferred list with key bitmaps over all K keys (def_keys [D][ceil(K/64)]).  Keys are
 * independent given the clocks and the deferred list, so each rank's fold of its keys is the exact
 * left fold (no data-path collective); out holds the rank's keys, except out->def_keys
 * [D][ceil(K/64)]: the surviving removes' key sets over ALL keys, assembled by one
 * ncclAllReduce(ncclSum) (disjoint ranges: sum = union).  def_keep is the same on every rank. */
int crdt_map_lub_many_sharded(crdt_ctx *ctx, const crdt_map_batch *in, size_t k0, size_t K, crdt_map_out *out);
/* crdt_map_lub_many_sharded with the deferred pool's offsets in DEVICE memory (round 4), as for
 * crdt_map_lub_many_doff: in->def_off NULL, def_off device u64 [G+1] (or NULL when D == 0),
 * def_off[G] == D.  Checked on the device (an invalid entry sets bit 1 of the flags of the groups
 * it bounds, ORed over the ranks); instead of the host offsets' hash in the agreed header, a
 * device hash of the offsets travels in the flags exchange and ranks holding different offsets
 * all return CRDT_EINVAL before the key sets are exchanged. */
int crdt_map_lub_many_sharded_doff(crdt_ctx *ctx, const crdt_map_batch *in, const uint64_t *def_off, size_t D,
                                   size_t k0, size_t K, crdt_map_out *out);

/* ---- Map<K, GCounter<A>, A> and Map<K, PNCounter<A>, A> (round 4) ----------------------------
 * Map::merge (map.rs:140-220) with a counter value: GCounter (gcounter.rs:44-54: merge = the VClock
 * max, Causal::forget = VClock::forget) or PNCounter (pncounter.rs:70-82: P and N each), folded as
 * acc = Map::new(); for r: acc.merge(replica[g][r]) — exact for any input (each key folded in
 * replica order: the fold is not associative for these values either).  Layout as crdt_map_batch,
 * with the value of key k a block of W counter rows (W = 1 GCounter, W = 2 PNCounter: P then N):
 *   val + g*val_gstride + r*val_rstride + (k*W + w)*A + a   (an absent key: its rows all 0)
 * deferred removes pooled per group as for Map<K, MVReg>: def_off a HOST array of G+1 entries,
 * def_row device u32 non-decreasing within the group and < R, def_clock [D][A], def_keys [D][Kw].
 * Output per group g (packed): clock[g*A + a], ec[(g*K + k)*A + a], val[((g*K + k)*W + w)*A + a],
 * flags[g] (required): bit 1 = def_row not non-decreasing or >= R, bit 3 = more than 512 live
 * removes named one key (results of the group unreliable); def_keep / def_keys as crdt_map_out.
 * Limits: A <= 512.  Device and host memory (crdt_mem_kind; round 5). */
typedef struct crdt_map_counter_batch {
  size_t G, R, K, A, W;
  const uint64_t *clock;
  size_t clock_rstride, clock_gstride;
  const uint64_t *ec;
  size_t ec_rstride, ec_gstride;
  const uint64_t *val;
  size_t val_rstride, val_gstride;
  const size_t *def_off; /* host, G+1 entries; NULL = no deferred removes */
  const uint32_t *def_row;
  const uint64_t *def_clock;
  const uint64_t *def_keys;
} crdt_map_counter_batch;

typedef struct crdt_map_counter_out {
  uint64_t *clock;    /* [G][A]       */
  uint64_t *ec;       /* [G][K][A]    */
  uint64_t *val;      /* [G][K][W][A] */
  uint32_t *flags;    /* [G]          */
  uint8_t *def_keep;  /* [D]          */
  uint64_t *def_keys; /* [D][Kw]      */
} crdt_map_counter_out;

int crdt_map_counter_lub_many(crdt_ctx *ctx, const crdt_map_counter_batch *in, crdt_map_counter_out *out);
/* Map<K, GCounter / PNCounter> sharded by KEYS (round 5), as crdt_map_lub_many_sharded: rank k holds keys
 * [k0, k0 + in->K) of every replica (the layout above with K = its key count), every replica's
 * clock and the group's whole deferred list with key bitmaps over all K keys (def_keys
 * [D][ceil(K/64)]); its fold of its keys is the exact left fold (no data-path collective).  out holds
 * the rank's keys, flags ORed over the ranks, and out->def_keys [D][ceil(K/64)] the surviving removes'
 * key sets over ALL keys (one ncclAllReduce(ncclSum): disjoint ranges).  Device memory only. */
int crdt_map_counter_lub_many_sharded(crdt_ctx *ctx, const crdt_map_counter_batch *in, size_t k0, size_t K,
                                      crdt_map_counter_out *out);

/* ---- Map<K, Orswot<M, A>, A> (round 4) ----------------------------------------------------------
 * Map::merge (map.rs:140-220) with a nested Orswot value (orswot.rs:81-149 merge, :150-183 forget)
 * — the value type of the reference's merge_error KAT (map.rs:435-494) — folded as
 * acc = Map::new(); for r: acc.merge(replica[g][r]), exact for any input (each key in replica
 * order).  Contiguous layouts (no strides):
 *   clock [G][R][A], ec [G][R][K][A] the entry clocks, oc [G][R][K][A] the nested Orswot clocks,
 *   ent [G][R][K][M][A] its member dots (a member absent: its row 0; a key absent: ec row 0),
 *   the nested deferred removes as a device CSR over (g, r, k): vd_off u64 [G*R*K + 1],
 *   vd_clock [Dv][A], vd_mem [Dv][Mw] member bitmasks, Mw = ceil(M / 64) words (1 for M <= 64: [Dv])
 *   (an equal clock twice in one list: unioned);
 *   the Map's own deferred removes as for the counter Map: def_off HOST, G+1 entries.
 * Output per group g (packed): clock[g*A + a], ec / oc [(g*K + k)*A + a], ent [((g*K + k)*M + m)*A
 * + a], nested deferred vd_n[g*K + k] (<= Vd) with vd_clock [((g*K + k)*Vd + i)*A + a] and
 * vd_mem [((g*K + k)*Vd + i)*Mw + w] (Vd = out->Vd, 0 meaning 16; round 6: the fold keeps 16 slots per
 * key in LDS and re-folds, exactly, the keys whose list passed 16 with all Vd — a second launch of one
 * wave per marked key, its Vd member masks in LDS: Vd * Mw * 8 + 6 KiB <= 160 KiB); flags[g]: bit 1 =
 * def_row not non-decreasing or >= R, bit 3 = more live Map removes named one key than the deep pass
 * holds (256 in the first pass; the deep pass takes the largest group's whole list, ~80,000 in its
 * LDS), bit 4 = a key's Orswot held more than Vd deferred removes, bit 5 = vd_off invalid (checked on the device: vd_off[0] == 0, non-decreasing,
 * vd_off[G*R*K] == Dv; the fold reads only rows [0, Dv) whatever it holds) — results of the
 * group unreliable; def_keep / def_keys as crdt_map_out.
 * Orswot::forget collects its deferred removes into a new map: two whose clocks become equal keep
 * one entry with the later one's members (the oracle's dict order).
 * Limits: A <= 1,024, M <= 1,024 (round 5: past A = 64 or M = 32 a wide kernel, lane = 64 actors
 * apart, the key's member rows in its own output rows; CRDT_TUNE mowide=1 runs it at every shape).
 * Device and host memory (crdt_mem_kind). */
typedef struct crdt_map_orswot_batch {
  size_t G, R, K, M, A;
  const uint64_t *clock, *ec, *oc, *ent;
  const uint64_t *vd_off;   /* device, G*R*K + 1 */
  const uint64_t *vd_clock; /* [Dv][A] */
  const uint64_t *vd_mem;   /* [Dv][Mw] */
  const size_t *def_off;    /* host, G+1 entries; NULL = no Map-level deferred removes */
  const uint32_t *def_row;
  const uint64_t *def_clock;
  const uint64_t *def_keys;
  size_t Dv;                /* rows of vd_clock / vd_mem (= vd_off[G*R*K]) */
} crdt_map_orswot_batch;

typedef struct crdt_map_orswot_out {
  uint64_t *clock;    /* [G][A]          */
  uint64_t *ec;       /* [G][K][A]       */
  uint64_t *oc;       /* [G][K][A]       */
  uint64_t *ent;      /* [G][K][M][A]    */
  uint32_t *vd_n;     /* [G][K]          */
  uint64_t *vd_clock; /* [G][K][Vd][A]   */
  uint64_t *vd_mem;   /* [G][K][Vd][Mw]  */
  uint32_t *flags;    /* [G]             */
  uint8_t *def_keep;  /* [D]             */
  uint64_t *def_keys; /* [D][Kw]         */
  size_t Vd;          /* nested deferred slots per key (round 6, ABI 8; 0 = 16) */
} crdt_map_orswot_out;

int crdt_map_orswot_lub_many(crdt_ctx *ctx, const crdt_map_orswot_batch *in, crdt_map_orswot_out *out);
/* Map<K, Orswot> sharded by KEYS (round 5), as crdt_map_lub_many_sharded: rank k holds keys
 * [k0, k0 + in->K) of every replica (the layout above with K = its key count; the nested removes' CSR over the rank's (g, r, k)), every replica's
 * clock and the group's whole deferred list with key bitmaps over all K keys (def_keys
 * [D][ceil(K/64)]); its fold of its keys is the exact left fold (no data-path collective).  out holds
 * the rank's keys, flags ORed over the ranks, and out->def_keys [D][ceil(K/64)] the surviving removes'
 * key sets over ALL keys (one ncclAllReduce(ncclSum): disjoint ranges).  Device memory only. */
int crdt_map_orswot_lub_many_sharded(crdt_ctx *ctx, const crdt_map_orswot_batch *in, size_t k0, size_t K,
                                     crdt_map_orswot_out *out);

/* ---- Map<K, Map<K2, MVReg<u64, A>, A>, A> (round 5) -----------------------------------------------
 * The nested type of the reference's own Map tests (TMap, test/map.rs:10; TestMap, map.rs:359):
 * Map::merge (map.rs:140-220) whose value is a Map<K2, MVReg> — merged by Map::merge again with
 * MVReg::merge (mvreg.rs:112-128) innermost, and forgotten by Map's Causal::forget (map.rs:85-114) —
 * folded as acc = Map::new(); for r: acc.merge(replica[g][r]), exact for any input (each outer key in
 * replica order).  Contiguous layouts (no strides), per replica r of group g:
 *   clock [G][R][A]; ec [G][R][K][A] outer entry clocks (key absent: row 0); ic [G][R][K][A] the
 *   inner Map clocks; iec [G][R][K][K2][A] inner entry clocks; ivc [G][R][K][K2][V][A] / ivv
 *   [G][R][K][K2][V] the inner MVReg slots in Vec order (an empty slot: clock row 0); the inner
 *   deferred removes as a device CSR over (g, r, k): id_off u64 [G*R*K + 1], id_clock [Di][A],
 *   id_keys [Di][K2w] inner-key bitmasks (K2w = 1 up to K2 = 64, else ceil(K2/64) words, round 6);
 *   the outer deferred removes as for the MVReg Map: def_off HOST
 *   (G+1), def_row, def_clock [D][A], def_keys [D][Kw].
 * Output per (g, k) (packed): clock [g*A + a], ec / ic [(g*K + k)*A + a], iec [((g*K + k)*K2 + j)*A +
 *   a], Vs slots per inner key (out->Vs, 0 meaning 8, at most 64) ivc [(((g*K + k)*K2 + j)*Vs + s)*A +
 *   a], ivv [((g*K + k)*K2 + j)*Vs + s] with nval [(g*K + k)*K2 + j] used (unused slots 0; round 6: a
 *   key past 8 values re-folds in the deep pass, which also takes inputs with V up to 64), inner deferred id_n [g*K + k] (<= Id = out->Id,
 *   0 meaning 16), id_clock [((g*K + k)*Id + i)*A + a], id_keys [((g*K + k)*Id + i)*K2w + w] (round 6:
 *   the fold keeps 16 in LDS and re-folds, exactly, the keys whose inner list passed 16 with all Id —
 *   a second launch of one wave per marked key); flags[g]: bit 1 = def_row not non-decreasing or >= R,
 *   bit 3 = more live outer removes named one key than the deep pass holds (256 in the first pass,
 *   the largest group's whole list in the deep pass), bit 4 = an inner Map held more than Id deferred
 *   removes, bit 5 = id_off invalid (checked on the device: starts at
 *   0, non-decreasing, ends at Di; the fold never reads past Di), bit 6 = an inner key held more than
 *   Vs values — results of the group unreliable; def_keep / def_keys as crdt_map_out.
 * Map::forget collects the inner deferred removes into a new map: two whose clocks become equal keep
 * one entry with the later one's keys (the oracle's dict order; the reference's is unspecified).
 * Limits: A <= 256 and K2 <= 256 (round 6: lane l holds actors l + 64 j; K2w key-set words), V <= 8.
 * Device and host memory
 * (crdt_mem_kind). */
typedef struct crdt_map_nested_batch {
  size_t G, R, K, K2, V, A;
  const uint64_t *clock, *ec, *ic, *iec, *ivc, *ivv;
  const uint64_t *id_off;   /* device, G*R*K + 1 */
  const uint64_t *id_clock; /* [Di][A] */
  const uint64_t *id_keys;  /* [Di][K2w] */
  size_t Di;
  const size_t *def_off;    /* host, G+1 entries; NULL = no outer deferred removes */
  const uint32_t *def_row;
  const uint64_t *def_clock;
  const uint64_t *def_keys;
} crdt_map_nested_batch;

typedef struct crdt_map_nested_out {
  uint64_t *clock;    /* [G][A]            */
  uint64_t *ec;       /* [G][K][A]         */
  uint64_t *ic;       /* [G][K][A]         */
  uint64_t *iec;      /* [G][K][K2][A]     */
  uint64_t *ivc;      /* [G][K][K2][Vs][A] */
  uint64_t *ivv;      /* [G][K][K2][Vs]    */
  uint32_t *nval;     /* [G][K][K2]        */
  uint32_t *id_n;     /* [G][K]            */
  uint64_t *id_clock; /* [G][K][Id][A]     */
  uint64_t *id_keys;  /* [G][K][Id][K2w]   */
  uint32_t *flags;    /* [G]               */
  uint8_t *def_keep;  /* [D]               */
  uint64_t *def_keys; /* [D][Kw]           */
  size_t Id;          /* inner deferred slots per key (round 6, ABI 8; 0 = 16) */
  size_t Vs;          /* MVReg slots per inner key (round 6, ABI 8; 0 = 8, at most 64) */
} crdt_map_nested_out;

int crdt_map_nested_lub_many(crdt_ctx *ctx, const crdt_map_nested_batch *in, crdt_map_nested_out *out);
/* Map<K, Map<K2, MVReg>> sharded by KEYS (round 5), as crdt_map_lub_many_sharded: rank k holds keys
 * [k0, k0 + in->K) of every replica (the layout above with K = its key count; the inner removes' CSR over the rank's (g, r, k)), every replica's
 * clock and the group's whole deferred list with key bitmaps over all K keys (def_keys
 * [D][ceil(K/64)]); its fold of its keys is the exact left fold (no data-path collective).  out holds
 * the rank's keys, flags ORed over the ranks, and out->def_keys [D][ceil(K/64)] the surviving removes'
 * key sets over ALL keys (one ncclAllReduce(ncclSum): disjoint ranges).  Device memory only. */
int crdt_map_nested_lub_many_sharded(crdt_ctx *ctx, const crdt_map_nested_batch *in, size_t k0, size_t K,
                                     crdt_map_nested_out *out);

/* Map<K, Map<K2, MVReg<u64>>> states in place (round 5), on the crdt_map_nested_lub_many output layout
 * with N states (packed; Vs MVReg slots per inner key in Vec order (states->Vs, 0 = 8), nval used, the rest zero; Id inner
 * deferred slots per key (states->Id, 0 = 16) with a K2w-word inner-key mask each, K2w = 1 up to K2 = 64):
 *   crdt_map_nested_apply_batch — CmRDT::apply (map.rs:119-137, apply_keyset_rm :318-348,
 *     apply_deferred :311-316) with the inner Map's apply one level down and MVReg::apply
 *     (mvreg.rs:130-166) innermost: state s applies ops [op_off[s], op_off[s+1]) in order; the outer
 *     deferred removes as crdt_map_counter_apply_batch (def_count[s] <= Dcap slots); an inner list past
 *     Id sets bit 0.  Ops: kind 0 =
 *     Op::Up { dot: (actor, counter), key, op } with ikind 0 = inner Op::Up { dot: (iactor, icounter),
 *     key: ikey, op: Put { clock: clk_pool[clk_row*A ..], val } } or 1 = inner Op::Rm { clock:
 *     clk_pool[clk_row*A ..], keyset: the inner-key mask ikeys [n_ops][K2w] }; kind 1 = Op::Rm { clock:
 *     clk_pool[clk_row*A ..], keyset: keys[key_off[o] .. key_off[o+1]) } (key_off may be NULL when no
 *     op is an outer Rm).  status[s]: bit 0 = a deferred list (outer Dcap or an inner one's Id)
 *     exhausted, bit 1 = a malformed op skipped whole, bits 2-3 = invalid input (state untouched),
 *     bit 4 = a register needed more than Vs values (that value was not added).
 *   crdt_map_nested_forget_batch — Causal::forget (map.rs:85-114) of the whole state by y[s] (y_stride
 *     0: one row for all): entry clocks, the inner Maps (their entries, registers — MVReg::forget
 *     mvreg.rs:88-104, emptied values dropped, order kept —, deferred removes, clocks), an emptied
 *     entry dropped; the outer deferred pool and the map clock as crdt_map_forget_batch.  Inner removes
 *     whose clocks become equal keep one entry with the later one's keys (the fold's rule).
 * Limits: A <= 512, K2 <= 256 (round 6; a key bit past K2 makes the op malformed); the outer Dcap is not bounded (its first min(Dcap, 16) slots in LDS during
 * an apply stream, the rest used in place, round 6).  Device memory only. */
typedef struct crdt_map_nested_states {
  size_t N, K, K2, A;
  uint64_t *clock;    /* [N][A]           */
  uint64_t *ec;       /* [N][K][A]        */
  uint64_t *ic;       /* [N][K][A]        */
  uint64_t *iec;      /* [N][K][K2][A]    */
  uint64_t *ivc;      /* [N][K][K2][Vs][A] */
  uint64_t *ivv;      /* [N][K][K2][Vs]   */
  uint32_t *nval;     /* [N][K][K2]       */
  uint32_t *id_n;     /* [N][K]           */
  uint64_t *id_clock; /* [N][K][Id][A]    */
  uint64_t *id_keys;  /* [N][K][Id][K2w]  */
  size_t Id;          /* inner deferred slots per key (round 6, ABI 8; 0 = 16) */
  size_t Vs;          /* MVReg slots per inner key (round 6, ABI 8; 0 = 8, at most 64) */
} crdt_map_nested_states;

typedef struct crdt_map_nested_ops {
  size_t n_ops;
  const uint64_t *op_off;    /* [N+1]       */
  const uint8_t *kind;       /* [n_ops] 0 = Op::Up, 1 = Op::Rm */
  const uint32_t *actor;     /* [n_ops] Up: the outer dot */
  const uint64_t *counter;   /* [n_ops] Up  */
  const uint32_t *key;       /* [n_ops] Up  */
  const uint8_t *ikind;      /* [n_ops] Up: 0 inner Up (Put), 1 inner Rm */
  const uint32_t *iactor;    /* [n_ops] inner Up: its dot */
  const uint64_t *icounter;  /* [n_ops] inner Up */
  const uint32_t *ikey;      /* [n_ops] inner Up: the inner key */
  const uint64_t *val;       /* [n_ops] inner Up: the Put's value */
  const uint64_t *ikeys;     /* [n_ops][K2w] inner Rm: inner-key mask */
  const uint32_t *clk_row;   /* [n_ops] the Put clock / an rm clock: row of clk_pool */
  const uint64_t *clk_pool;  /* [n_clk_rows][A] */
  size_t n_clk_rows;
  const uint64_t *key_off;   /* [n_ops+1] outer Rm keysets */
  const uint32_t *keys;      /* [n_keys]    */
  size_t n_keys;
} crdt_map_nested_ops;

int crdt_map_nested_apply_batch(crdt_ctx *ctx, const crdt_map_nested_states *states, uint64_t *def_clock,
                                uint64_t *def_keys, uint32_t *def_count, size_t Dcap,
                                const crdt_map_nested_ops *ops, uint32_t *status);
int crdt_map_nested_forget_batch(crdt_ctx *ctx, const crdt_map_nested_states *states, const uint64_t *y,
                                 size_t y_stride, uint64_t *def_clock, const uint32_t *def_state, size_t D,
                                 uint8_t *def_keep);

/* Pairwise in-place merge of value-typed Map states (round 6): self[i].merge(other[i]) for i < N
 * (Map::merge map.rs:140-220 with the value's merge / forget: gcounter.rs:44-54 / pncounter.rs:70-82,
 * orswot.rs:81-183, or the inner Map's map.rs:85-220 with mvreg.rs:88-128), on the apply layouts
 * (crdt_map_counter_states / crdt_map_orswot_states / crdt_map_nested_states, N, K, A and W / M / K2
 * equal on both sides) with each side's Map-level deferred removes as crdt_map_deferred slots (the
 * counts may differ in Dcap).  Each pair is one group of the exact left fold above with R = 2
 * (Map::new() merged with self, then other): self.merge(other) on every state apply, merge, forget or
 * ingest leaves (deferred removes applied and not dominated by the clock).  self is rewritten: its
 * rows, its nested lists, and its slots with the surviving removes (their merged key sets) in pool
 * order, vacated slots zeroed; other is read only.  status[i]: bit 0 = more surviving removes than
 * self's Dcap (the first Dcap kept), bit 3 = the fold reported a capacity for the pair (more than
 * 256 / 512 live removes naming one key, more than self's Vd / Id nested deferred removes on a key,
 * more than 8 values on an inner key: that pair's state is incomplete).  A def_count above its Dcap or
 * a nested count above its side's Vd / Id fails the call (CRDT_EINVAL) before anything is written.  The call reads the slot
 * counts on the host (one stream synchronisation).  Device memory only. */
int crdt_map_counter_merge_batch(crdt_ctx *ctx, const crdt_map_counter_states *self, const crdt_map_deferred *self_def,
                                 const crdt_map_counter_states *other, const crdt_map_deferred *other_def,
                                 uint32_t *status);
int crdt_map_orswot_merge_batch(crdt_ctx *ctx, const crdt_map_orswot_states *self, const crdt_map_deferred *self_def,
                                const crdt_map_orswot_states *other, const crdt_map_deferred *other_def,
                                uint32_t *status);
int crdt_map_nested_merge_batch(crdt_ctx *ctx, const crdt_map_nested_states *self, const crdt_map_deferred *self_def,
                                const crdt_map_nested_states *other, const crdt_map_deferred *other_def,
                                uint32_t *status);

/* ---- MVReg<u64, A> on its own (outside a Map) ------------------------------------------------
 * Replaces MVReg::merge (mvreg.rs:112-128) and MVReg::apply (mvreg.rs:130-166) for registers in the
 * dense layout the Map entry points use for their values: slots in Vec order, slot s of register i
 * = (clock vclk[i*vclk_stride + s*A + a], value vval[i*vval_stride + s]); an empty slot is an
 * all-zero clock row (skipped; results are written from slot 0, empty slots zeroed).  Values are
 * u64 ids interned by the caller (merge and apply compare clocks only, never values).  Exact for
 * any input: each register is folded / applied in order.
 *   lub_many:    acc = MVReg::new(); for r in 0..R: acc.merge(replica[g][r]) per group g; replica
 *                (g, r) at vclk + g*vclk_gstride + r*vclk_rstride (vval likewise).  out: Vout slots
 *                per group (packed [G][Vout][A] / [G][Vout]), nval[g] (may be NULL), flags[g]: bit 0
 *                = more than Vout values (slots incomplete: retry with a larger Vout), bit 2 = the
 *                fold state overflowed (retry with Vstate = 16; past 16 values it is reported, or
 *                folded exactly by the deep pass: Vstate = 17..64, see Limits).
 *   merge_batch: self[i].merge(other[i]), in place in self's V slots (own kept values, then other's
 *                added ones); status[i] bit 4 = more than self's V values (register incomplete).
 *   apply_batch: register i applies ops [op_off[i], op_off[i+1]) in order, Op::Put { clock:
 *                clk_pool[clk_row[o]*A ..], val: val[o] }; status[i] bit 1 = an op's clk_row out
 *                of range (skipped), bit 3 = op_off invalid (register untouched), bit 4 = more than
 *                V values.
 * Limits: A <= 1024, 1 <= V <= 16 with the working register held in registers, 17 <= V <= 64 with
 * it held in LDS (below; lub_many: Vout <= 16 unless Vstate >= 17); A > 256 or V > 8 run one
 * workgroup of ceil(A / 64) waves per register.  lub_many with 17 <= Vstate <= 64 adds a deep
 * pass: Vout may go up to 64, the registers whose 16-value state overflows are marked instead of
 * reported and folded again, in replica order, with up to Vstate values held in LDS (bit 2 = more
 * than Vstate values at some step).  It needs about Vstate * A * 8 bytes of LDS per register; past
 * 160 KiB, or with Vstate > 64, the call returns CRDT_EUNSUPPORTED before anything is launched.
 * Registers of 17..64 slots (merge_batch with self's or other's V past 16, apply_batch with V past
 * 16, lub_many with input V past 16) keep the working register in LDS too, one workgroup of 64..256
 * threads per register: merge_batch and apply_batch need about V * A * 8 bytes for self's V slots,
 * lub_many takes input V in 17..64 only with Vstate in 17..64 (every group then runs the LDS fold,
 * flags as the deep pass reports them) and needs the bytes of Vstate slots; the same 160 KiB bound
 * holds (V = 64 reaches A = 314), past it CRDT_EUNSUPPORTED naming V, A and the bytes.  When a
 * register overflows self's V slots (bit 4) the slots hold the first V values of the result.  V > 64
 * is CRDT_EUNSUPPORTED.  Shapes of 16 slots or fewer run the kernels they always ran. */
typedef struct crdt_mvreg_states {
  size_t N, A, V;
  uint64_t *vclk;
  size_t vclk_stride;
  uint64_t *vval;
  size_t vval_stride;
} crdt_mvreg_states;

typedef struct crdt_mvreg_batch {
  size_t G, R, A, V;
  const uint64_t *vclk;
  size_t vclk_rstride, vclk_gstride;
  const uint64_t *vval;
  size_t vval_rstride, vval_gstride;
} crdt_mvreg_batch;

typedef struct crdt_mvreg_out {
  size_t Vout;
  size_t Vstate;   /* <= 16: value capacity hint for the fold state (0 = from Vout and V);
                      17..64: the deep pass with that many values (see Limits) */
  uint64_t *vclk;  /* [G][Vout][A] */
  uint64_t *vval;  /* [G][Vout]    */
  uint32_t *nval;  /* [G] or NULL  */
  uint32_t *flags; /* [G]          */
} crdt_mvreg_out;

typedef struct crdt_mvreg_ops {
  size_t n_ops;
  const uint64_t *op_off;   /* [N+1]           */
  const uint32_t *clk_row;  /* [n_ops]         */
  const uint64_t *clk_pool; /* [n_clk_rows][A] */
  size_t n_clk_rows;
  const uint64_t *val;      /* [n_ops]         */
} crdt_mvreg_ops;

int crdt_mvreg_lub_many(crdt_ctx *ctx, const crdt_mvreg_batch *in, crdt_mvreg_out *out);
int crdt_mvreg_merge_batch(crdt_ctx *ctx, const crdt_mvreg_states *self, const crdt_mvreg_states *other,
                           uint32_t *status);
int crdt_mvreg_apply_batch(crdt_ctx *ctx, const crdt_mvreg_states *states, const crdt_mvreg_ops *ops,
                           uint32_t *status);

/* Batched Causal::forget of MVReg (mvreg.rs:88-104 with VClock::forget): register i forgets the
 * clock y + i*y_stride (A counters; y_stride = 0: one clock for all registers, as in
 * crdt_map_forget_batch), in place.  Every value clock keeps v[a] where v[a] > y[a] (an unsigned
 * compare over the full u64 range) and becomes 0 elsewhere; a value whose clock empties is dropped.
 * Result layout as above: the survivors in Vec order from slot 0, every slot past them an all-zero
 * clock and value 0; empty slots of the input are skipped wherever they sit.  All of a register's
 * slots are loaded before any is stored, so the compaction in place is safe.  A register the forget
 * leaves bit-identical is not written.  status[i] (device u32, may be NULL) is written for every i;
 * no bit is defined yet: 0.  Limits: A <= 1024, 1 <= V <= 64 (no LDS state, so every A at every V);
 * A > 256 or V > 8 run one workgroup per register (past 16 slots in two passes over the rows, a
 * thread moving only its own actor column, so the order in place stays safe), below that a register
 * takes a sub-wave lane segment (one lane per 16 bytes of a row). */
int crdt_mvreg_forget_batch(crdt_ctx *ctx, const crdt_mvreg_states *states, const uint64_t *y, size_t y_stride,
                            uint32_t *status);

/* ---- batched state equality: the reference's PartialEq on N pairs of states ------------------
 * ne[i] (device u32[N], written for every i) is 0 iff x[i] == y[i] by the reference's PartialEq:
 * derived on Orswot (orswot.rs:20), Map / Entry (map.rs:31-47) and VClock (vclock.rs:56),
 * hand-written and order-free on MVReg (mvreg.rs:62-86).  Otherwise it is the COMPLETE set of the
 * components that differ (there is no early exit between components).  Both sides are read only; x
 * and y may be the same memory (every word is then 0).  The layouts are those of the matching
 * merge_batch: crdt_mvreg_states, crdt_orswot_states, crdt_map_states + crdt_map_deferred.
 *  - Clock rows and entry rows (Orswot member rows, Map entry clocks) compare word by word over the
 *    full u64.  An absent member / key is an all-zero row, so this is the BTreeMap / HashMap equality
 *    of the derived impls (vclock.rs:56, orswot.rs:20, map.rs:31-47).
 *  - Registers (an MVReg, and every key of a Map) compare as SETS of (clock row, value) over the
 *    non-empty slots, the two loops of mvreg.rs:64-81: an empty slot (all-zero clock) is skipped
 *    wherever it sits, V may differ between the sides, slot order is irrelevant, and the value IS
 *    compared (the same clock with another value is unequal, unlike merge, which never looks at
 *    values).  A pair held twice within one side counts once: the sanity assert_eq!(num_found, 1) of
 *    mvreg.rs:71 / :80 is not reproduced as a failure.  A Map key that is absent (all-zero entry
 *    clock) has the empty register whatever its value slots hold (map.rs:40-47: no Entry, no val).
 *  - Deferred removes: the first def_count[s] slots of each side are a map rm clock -> member / key
 *    set (orswot.rs:24, map.rs:37).  Slot order and Dcap are irrelevant; slots of one side holding the
 *    same clock union their sets, as merge_batch treats them; a slot with an empty set is still a key
 *    of the map ({c: {}} != {}, as in the reference's HashMap).  Bits past M / K in a bitmap's last
 *    word are zero by the layout's invariant and are not masked.
 * Limits (past them CRDT_EUNSUPPORTED before any launch): A <= 1024; MVReg and Map 1 <= V <= 64 on
 * each side (the compare keeps no LDS state, so every A at every V).  N, and M / K / A where applicable,
 * must match across the sides (CRDT_EINVAL).  Dcap and def_count are not bounded: the result is exact
 * for any number of live slots.  N == 0 returns CRDT_OK.  Device memory only.  A deferred side with
 * Dcap == 0 may pass NULL buffers (crdt_map_eq_batch: a NULL crdt_map_deferred); a def_count that IS
 * passed is read whatever Dcap is, so a non-zero count with Dcap == 0 reports CRDT_NE_INVALID. */
#define CRDT_NE_CLOCK    1u  /* the state's own clock differs                                  */
#define CRDT_NE_ENTRIES  2u  /* Orswot: some member's dot row; Map: some key's entry clock     */
#define CRDT_NE_VALUES   4u  /* MVReg / Map: some register differs as a set of (clock, value)  */
#define CRDT_NE_DEFERRED 8u  /* the deferred removes differ as a map rm clock -> set           */
#define CRDT_NE_INVALID 16u  /* def_count above Dcap on either side: no other bit is set       */

int crdt_mvreg_eq_batch(crdt_ctx *ctx, const crdt_mvreg_states *x, const crdt_mvreg_states *y, uint32_t *ne);
int crdt_orswot_eq_batch(crdt_ctx *ctx, const crdt_orswot_states *x, const crdt_orswot_states *y, uint32_t *ne);
int crdt_map_eq_batch(crdt_ctx *ctx, const crdt_map_states *x, const crdt_map_deferred *xd, const crdt_map_states *y,
                      const crdt_map_deferred *yd, uint32_t *ne);

/* The same for the value-typed Maps, on the layouts of their merge_batch (crdt_map_counter_states /
 * crdt_map_orswot_states / crdt_map_nested_states + crdt_map_deferred; a NULL crdt_map_deferred means
 * no Map-level slots).  Map's PartialEq is derived for any V (map.rs:31-47), so ne[i] is 0 iff
 * x[i] == y[i] with the value type's own PartialEq per key, else the complete set of:
 *  - CRDT_NE_CLOCK: the Map's clock row differs.
 *  - CRDT_NE_ENTRIES: some key's entry clock ec[s][k] differs, word by word.  A key is absent exactly
 *    when that row is all zero.
 *  - CRDT_NE_VALUES: for some key the values differ.  The value of a key absent on a side is
 *    V::default(), whatever that key's value arrays hold (the rule crdt_map_eq_batch states for
 *    registers): a key present on one side only differs in its value iff the present value is not
 *    the default one.
 *      Counters (gcounter.rs, pncounter.rs: derived over the inner VClocks): the W rows
 *        val[s][k][w][.], word by word over the full u64.
 *      Orswot (orswot.rs:20, derived): oc[s][k]; the member rows ent[s][k][m][.] (an absent member is
 *        an all-zero row); the first vd_n[s][k] nested deferred slots as a map rm clock -> member set
 *        with the rules of the Map-level list below.  Slots at or past vd_n are never read; Vd may
 *        differ between the sides.
 *      Inner Map (map.rs:31-47 one level down): ic[s][k]; iec[s][k][j] (an inner key is absent iff
 *        that row is all zero, and its register is then the empty one); the first id_n[s][k] inner
 *        deferred slots as a map rm clock -> inner-key set; each present inner key's register as a
 *        set of (clock row, value) over the non-empty slots among its first nval[s][k][j] slots, the
 *        order-free rule of mvreg.rs:62-86 (the value is compared, a pair held twice counts once, Vs
 *        may differ between the sides).  Rows past nval / id_n are never read.
 *  - CRDT_NE_DEFERRED: the Map-level deferred removes differ as a map rm clock -> key set, exactly as
 *    in crdt_map_eq_batch (slot order and Dcap irrelevant, equal clocks within one side union their
 *    sets, {c: {}} != {}).
 *  - CRDT_NE_INVALID, alone, when on either side def_count > Dcap, some vd_n[s][k] > Vd, some
 *    id_n[s][k] > Id or some nval[s][k][j] > Vs (of any key, present or not).  Neighbouring pairs are
 *    unaffected.
 * Limits (past them CRDT_EUNSUPPORTED before any launch): counters A <= 1,024, W in {1, 2}; Orswot
 * values A <= 1,024, M <= 1,024; nested A <= 256, K2 <= 256, Vs <= 64.  Vd, Id and Dcap are not
 * bounded: the result is exact for any number of live slots.  N, K, A and W / M / K2 must match
 * across the sides (CRDT_EINVAL).  N == 0 returns CRDT_OK.  x and y may alias (every word is then 0).
 * Both sides are read only; the calls allocate nothing and do not synchronise with the host.  Device
 * memory only. */
int crdt_map_counter_eq_batch(crdt_ctx *ctx, const crdt_map_counter_states *x, const crdt_map_deferred *xd,
                              const crdt_map_counter_states *y, const crdt_map_deferred *yd, uint32_t *ne);
int crdt_map_orswot_eq_batch(crdt_ctx *ctx, const crdt_map_orswot_states *x, const crdt_map_deferred *xd,
                             const crdt_map_orswot_states *y, const crdt_map_deferred *yd, uint32_t *ne);
int crdt_map_nested_eq_batch(crdt_ctx *ctx, const crdt_map_nested_states *x, const crdt_map_deferred *xd,
                             const crdt_map_nested_states *y, const crdt_map_deferred *yd, uint32_t *ne);

/* ---- re-index resident states when a dictionary or a capacity grows ------------------------------
 * Out-of-place gathers of N dense states from one layout into another along every indexed axis
 * (actor columns, member / key rows and bits, value slots, deferred slots), on the device, without a
 * host synchronisation.  They are what a caller keeping states resident runs when an ingest reports an
 * id missing from its dictionary (status bit 1) or a call reports a capacity ("retry with a larger
 * Dcap" / "more slots", bits 0 and 4): build the union dictionary, crdt_reindex_map_*, reindex, retry.
 *
 * Axis map: a device uint32_t src[n_out].  Output index j takes the data of input index src[j]; any
 * src[j] >= n_in means nobody (zeros: an absent member / key).  A NULL map is the identity on
 * min(n_in, n_out) indices and nobody past it (the pure capacity change).  A map that is not injective
 * gives the gather's result (an input index copied to several outputs); this is not checked.
 *   crdt_reindex_map_u32 / _u64: old_ids[n_old] and new_ids[n_new] ascending and unique, as the ingest
 *   calls require; src[j] = position of new_ids[j] in old_ids, or 0xFFFFFFFF when absent; *n_lost
 *   (device u32[1]) = the number of old ids absent from new_ids.  One lane per new id, a binary search.
 *
 * Layout calls (every output word of every state is written, so out needs no zeroing; gaps between
 * strided rows are not touched; in is read only; overlapping in and out is undefined, and equal base
 * pointers return CRDT_EINVAL):
 *   crdt_rows_reindex    N rows of planes x A_in u64 words (plane q of row i at in + i*in_stride +
 *                        q*A_in) into rows of planes x A_out: planes = 1 for VClock / GCounter rows and
 *                        pooled def_clock[D][A] rows, 2 for PNCounter's P and N halves.
 *   crdt_bitmap_reindex  N bitmap rows of U_in bits into U_out bits, bit by bit (GSet rows, pooled
 *                        def_members[D][Mw] / def_keys[D][Kw] rows; strides in words).  Bits past U_out
 *                        in the last output word are written 0 (the layout's invariant).
 *   crdt_orswot_reindex  clock and entry columns by actor_src, entry rows by member_src, the first
 *                        def_count[s] deferred slots (clock columns, member bits; slot order kept) and
 *                        def_count.  out's M, A and Dcap may each be larger or smaller than in's; Dcap
 *                        == 0 with NULL deferred buffers is accepted on either side (an input def_count
 *                        that IS passed is read whatever Dcap is).
 *   crdt_mvreg_reindex   value clocks by actor_src, slot v to slot v (positions and holes kept); slots
 *                        in [V_in, V_out) are zeroed.
 *   crdt_map_reindex     clock, ec[K][A], vclk[K][V][A], vval[K][V], deferred clocks and key bitmaps; K,
 *                        A, V and Dcap may each differ between the sides; a NULL crdt_map_deferred means
 *                        no slots on that side.
 * status[s] (device u32[N], may be NULL; written for every s):
 *   CRDT_REINDEX_DCAP     def_count[s] > out Dcap: the first out Dcap slots are kept, the output count
 *                         is out Dcap.
 *   CRDT_REINDEX_DROPPED  an id the map drops (no output index takes it) held data in state s: a
 *                         non-zero counter in a dropped actor column of the clock, of an entry row, of a
 *                         value clock in a kept slot of a kept key, or of one of the def_count[s]
 *                         deferred clocks; a non-zero entry row of a dropped member / key; a bit set for
 *                         a dropped member / key in one of the def_count[s] deferred bitmaps.
 *   CRDT_REINDEX_INVALID  def_count[s] > in Dcap: the output state is the empty state with count 0 and
 *                         no other bit is set.
 *   CRDT_REINDEX_VALUES   a non-empty value slot (non-zero clock row) of a kept key / of the register at
 *                         a position >= out V: that slot is dropped.
 * Limits (past them CRDT_EUNSUPPORTED before any launch): 1 <= V <= 64 and planes <= 64; N, Dcap, M, K
 * and A are bounded only by 2^31 - 1 (Map and MVReg: K and A by 2^25), far past the 4,096 / 1,024
 * actors the consuming calls take.  N == 0 returns CRDT_OK.  Device memory only.  The calls keep one
 * flag per input index of a mapped axis in the ctx scratch (grown on the first call that needs more,
 * as for every call); nothing else is allocated. */
#define CRDT_REINDEX_DCAP     1u
#define CRDT_REINDEX_DROPPED  2u
#define CRDT_REINDEX_INVALID  4u
#define CRDT_REINDEX_VALUES  16u

int crdt_reindex_map_u32(crdt_ctx *ctx, const uint32_t *old_ids, size_t n_old, const uint32_t *new_ids, size_t n_new,
                         uint32_t *src, uint32_t *n_lost);
int crdt_reindex_map_u64(crdt_ctx *ctx, const uint64_t *old_ids, size_t n_old, const uint64_t *new_ids, size_t n_new,
                         uint32_t *src, uint32_t *n_lost);
int crdt_rows_reindex(crdt_ctx *ctx, const uint64_t *in, size_t in_stride, size_t A_in, uint64_t *out, size_t out_stride,
                      size_t A_out, size_t planes, size_t N, const uint32_t *src, uint32_t *status);
int crdt_bitmap_reindex(crdt_ctx *ctx, const uint64_t *in, size_t in_stride, size_t U_in, uint64_t *out, size_t out_stride,
                        size_t U_out, size_t N, const uint32_t *src, uint32_t *status);
int crdt_orswot_reindex(crdt_ctx *ctx, const crdt_orswot_states *in, const uint32_t *actor_src, const uint32_t *member_src,
                        const crdt_orswot_states *out, uint32_t *status);
int crdt_mvreg_reindex(crdt_ctx *ctx, const crdt_mvreg_states *in, const uint32_t *actor_src, const crdt_mvreg_states *out,
                       uint32_t *status);
int crdt_map_reindex(crdt_ctx *ctx, const crdt_map_states *in, const crdt_map_deferred *in_def, const uint32_t *actor_src,
                     const uint32_t *key_src, const crdt_map_states *out, const crdt_map_deferred *out_def,
                     uint32_t *status);

/* ---- causal helpers on dense clock rows -----------------------------------
 * Row-pair ops over N pairs (x_i, y_i) of A-word rows (VClock, GCounter inner, or a PNCounter
 * P‖N row with A = 2·actors):
 *   CRDT_PAIR_GLB     out_i = x_i.glb(y_i): pointwise min, a 0 drops the actor   vclock.rs:246-259
 *   CRDT_PAIR_FORGET  out_i = x_i.forget(y_i): keep x[a] iff x[a] > y[a]         vclock.rs:95-105
 *                     (GCounter::forget gcounter.rs:51-53, PNCounter::forget pncounter.rs:78-81
 *                     are the same op on their rows)
 *   CRDT_PAIR_INTERSECTION  out_i = VClock::intersection(x_i, y_i): keep x[a] iff
 *                     y[a] == x[a] (the common dots)                            vclock.rs:218-227
 * `out` may alias `x` (in place, like the reference's &mut self). */
#define CRDT_PAIR_GLB 1
#define CRDT_PAIR_FORGET 2
#define CRDT_PAIR_INTERSECTION 3
int crdt_vclock_pair_op(crdt_ctx *ctx, int op, uint64_t *out, const uint64_t *x, const uint64_t *y,
                        size_t N, size_t A, size_t out_stride, size_t x_stride, size_t y_stride);

/* VClock::partial_cmp (vclock.rs:68-80) of N row pairs: out[i] = 0 Equal, 1 Greater (x ≥ y),
 * -1 Less, 2 None (concurrent). */
int crdt_vclock_partial_cmp(crdt_ctx *ctx, const uint64_t *x, const uint64_t *y, size_t N, size_t A,
                            size_t x_stride, size_t y_stride, int8_t *out);

/* All-pairs partial_cmp of N clocks (the dominance / concurrency matrix): out[i*N + j] =
 * partial_cmp(x_i, x_j) coded as above.  N <= 4,194,240. */
int crdt_vclock_cmp_matrix(crdt_ctx *ctx, const uint64_t *x, size_t N, size_t A, size_t x_stride,
                           int8_t *out);

/* read() of N counters, exact: out[2i] + 2^64·out[2i+1] is
 *   GCounter::read  (gcounter.rs:70-72, BigUint sum of the A counters of row i), or
 *   PNCounter::read (pncounter.rs:110-115, BigInt P − N of row i = P[0..A) ‖ N[A..2A)) as a
 *                   two's-complement 128-bit integer.
 * Exact for A < 2^62 (the reference's num-bigint is unbounded; no sum of u64 counters of one
 * row reaches 2^126). */
int crdt_gcounter_read(crdt_ctx *ctx, const uint64_t *in, size_t N, size_t A, size_t row_stride,
                       uint64_t *out);
int crdt_pncounter_read(crdt_ctx *ctx, const uint64_t *in, size_t N, size_t A, size_t row_stride,
                        uint64_t *out);

/* ---- batched ReadCtx queries (ctx.rs:8-55) -------------------------------------------------
 * Every read of the reference returns ReadCtx { add_clock, rm_clock, val }; the contexts derived
 * from it (derive_add_ctx / derive_rm_ctx, ctx.rs:40-55) are the only supported way to build the
 * next Op.  These calls produce the dense form of those pieces in device memory, so read ->
 * derive ctx -> op -> *_apply_batch never leaves the device.  Every output element is written on
 * every call.  Per-query status[q] (device u32): bit 1 = a state index, member, key or actor out
 * of range (the query's outputs are those of an absent element: zeros).
 *
 * Orswot::read / read_ctx (orswot.rs:264-279) / Map::is_empty, len and read_ctx (map.rs:233-249,
 * :301-307) as a presence scan: N states of M (K) rows of A words, row (s, m) at
 * entries + s*entry_sstride + m*entry_mstride (the crdt_orswot_states layout; a Map's ec with
 * ec_kstride = A, ec_sstride = ec_stride).  members[s*Mw + w] (Mw = ceil(M/64)) has bit b set iff
 * row 64w + b is non-zero (member / key present); bits past M are 0.  len[s] (may be NULL) = the
 * number of present rows; Map::is_empty is len[s] == 0.  add_clock = rm_clock = the state's clock
 * (the caller has it).  crdt_map_read serves Map<K, MVReg> and every value-typed Map (all mark an
 * absent key by an all-zero ec row).  Rows are read with 16-byte loads when A, both strides and
 * the base pointer keep every row 16-byte aligned, with 8-byte loads otherwise. */
int crdt_orswot_read(crdt_ctx *ctx, const uint64_t *entries, size_t entry_mstride, size_t entry_sstride, size_t N,
                     size_t M, size_t A, uint64_t *members /* [N][Mw] */, uint32_t *len /* [N] or NULL */);
int crdt_map_read(crdt_ctx *ctx, const uint64_t *ec, size_t ec_kstride, size_t ec_sstride, size_t N, size_t K,
                  size_t A, uint64_t *keys /* [N][Kw] */, uint32_t *len /* [N] or NULL */);

/* Orswot::contains (orswot.rs:253-262) of Q queries (state_idx[q], member[q]) (device u32):
 * val[q] = 1 iff the member is present, rm_clock + q*rm_stride = the member's dot clock (the
 * ReadCtx's rm_clock; all zeros when absent).  add_clock is the clock row of state state_idx[q]. */
int crdt_orswot_contains(crdt_ctx *ctx, const uint64_t *entries, size_t entry_mstride, size_t entry_sstride,
                         size_t N, size_t M, size_t A, const uint32_t *state_idx, const uint32_t *member, size_t Q,
                         uint8_t *val /* [Q] */, uint64_t *rm_clock, size_t rm_stride, uint32_t *status /* [Q] */);

/* MVReg::read / read_ctx (mvreg.rs:183-215) of the N registers of `regs` (crdt_mvreg_states):
 * clock + i*clock_stride = the pointwise max of the non-empty slot clocks (add_clock = rm_clock,
 * mvreg.rs:207-215), vals[i*V ..] (may be NULL) = the values of the non-empty slots in Vec order,
 * the rest 0, nval[i] (may be NULL) = their count.  V <= 64. */
int crdt_mvreg_read(crdt_ctx *ctx, const crdt_mvreg_states *regs, uint64_t *clock, size_t clock_stride,
                    uint64_t *vals /* [N][V] or NULL */, uint32_t *nval /* [N] or NULL */);

/* Map::get (map.rs:251-262) of Q queries (state_idx[q], key[q]) (device u32) on Map<K, MVReg>
 * states: present[q] = 1 iff the key has an entry, rm_clock[q*A ..] = its entry clock (zeros when
 * absent), the key's register compacted in Vec order (non-empty slots first, the rest zeroed):
 * vclk[(q*V + j)*A ..], vval[q*V + j], nval[q]; val_clock[q*A ..] = the join of its slot clocks,
 * the clock a following MVReg::read of that value returns (mvreg.rs:207-215).  An absent key has
 * no register (val = None): nval 0, zeros.  add_clock is the clock row of state state_idx[q].
 * V <= 64. */
int crdt_map_get(crdt_ctx *ctx, const crdt_map_states *states, const uint32_t *state_idx, const uint32_t *key,
                 size_t Q, uint8_t *present /* [Q] */, uint64_t *rm_clock /* [Q][A] */, uint64_t *vclk /* [Q][V][A] */,
                 uint64_t *vval /* [Q][V] */, uint32_t *nval /* [Q] */, uint64_t *val_clock /* [Q][A] */,
                 uint32_t *status /* [Q] */);

/* Map::get (map.rs:251-262) and the gotten value's own reads on the value-typed Maps, in their
 * apply layouts (crdt_map_counter_states / crdt_map_orswot_states / crdt_map_nested_states; Vs / Vd /
 * Id of 0 mean their defaults, as in the apply calls).  Q queries (state_idx[q], key[q][, member[q] |
 * ikey[q]]), device u32.  For every get: present[q] = 1 iff the key's ec row is non-zero, rm_clock[q*A ..]
 * = that row (zeros when absent); add_clock of the outer get is the clock row of state state_idx[q] (the
 * caller gathers it, as for crdt_map_get).  status[q] bit 1 = a state index, key, member or inner key out
 * of range: the outputs of an absent element (zeros, present 0).  Outputs marked "or NULL" are skipped
 * when NULL; every other output element is written on every call.  Q == 0 launches nothing.  Limits
 * (CRDT_EUNSUPPORTED past them): A <= 512 (the apply calls'), M <= 1,024, K2 <= 256, Vs <= 64.  Device
 * memory only.
 *
 * crdt_map_counter_get — Map<K, GCounter / PNCounter> (W = 1 / 2; ec / val rows at ec + s*ec_stride +
 *   k*A and val + s*val_stride + (k*W + w)*A): val[(q*W + w)*A ..] = the counter's W rows, zeros when
 *   absent (V::default()); total[2q] + 2^64·total[2q+1] = GCounter::read (gcounter.rs:70-72) / PNCounter::read
 *   (pncounter.rs:110-114, P − N in two's complement) of those rows, in the encoding of crdt_gcounter_read /
 *   crdt_pncounter_read; an absent key reads 0.
 * crdt_map_orswot_get — Map<K, Orswot<M>>: val_clock[q*A ..] = the key's oc row, the add_clock =
 *   rm_clock of the gotten set's read() (orswot.rs:264-279); members[q*Mw + w] (Mw = ceil(M/64)) has bit b
 *   set iff member row 64w + b is non-zero, bits past M 0; len[q] = the bit count; vd_n[q] = the key's
 *   pending nested removes.  A present key may hold an empty set (present 1, len 0).
 * crdt_map_orswot_contains — Orswot::contains (orswot.rs:253-262) on the set under key[q]: add_clock =
 *   the oc row, rm_clock = member[q]'s dot row, val[q] = 1 iff that row is non-zero; under an absent key
 *   everything is zero (Orswot::default().contains).
 * crdt_map_nested_get — Map<K, Map<K2, MVReg>>: val_clock = the key's ic row (the inner Map's clock,
 *   map.rs:301-307), ikeys[q*K2w + w] (K2w = ceil(K2/64)) / len[q] = the inner Map's key set and len
 *   (map.rs:233-249) from its iec rows, bits past K2 0.
 * crdt_map_nested_get_inner — the gotten inner Map's get of ikey[q]: add_clock = the ic row, rm_clock =
 *   the iec row (present[q] = 1 iff it is non-zero), the register = the first nval slots (already in Vec
 *   order): vclk[(q*Vs + j)*A ..], vval[q*Vs + j], nval[q], the slots past them zero; val_clock = the join
 *   of those slot clocks (mvreg.rs:207-215).  Under an absent outer or inner key everything is zero.
 * The member / inner-key scans give each row a power-of-two lane segment, one lane per 16 bytes when A is
 * even and ent / iec 16-byte aligned (8-byte words otherwise). */
int crdt_map_counter_get(crdt_ctx *ctx, const crdt_map_counter_states *states, const uint32_t *state_idx,
                         const uint32_t *key, size_t Q, uint8_t *present /* [Q] */, uint64_t *rm_clock /* [Q][A] */,
                         uint64_t *val /* [Q][W][A] or NULL */, uint64_t *total /* [Q][2] or NULL */,
                         uint32_t *status /* [Q] */);
int crdt_map_orswot_get(crdt_ctx *ctx, const crdt_map_orswot_states *states, const uint32_t *state_idx,
                        const uint32_t *key, size_t Q, uint8_t *present /* [Q] */, uint64_t *rm_clock /* [Q][A] */,
                        uint64_t *val_clock /* [Q][A] */, uint64_t *members /* [Q][Mw] */, uint32_t *len /* [Q] */,
                        uint32_t *vd_n /* [Q] or NULL */, uint32_t *status /* [Q] */);
int crdt_map_orswot_contains(crdt_ctx *ctx, const crdt_map_orswot_states *states, const uint32_t *state_idx,
                             const uint32_t *key, const uint32_t *member, size_t Q, uint8_t *val /* [Q] */,
                             uint64_t *add_clock /* [Q][A] */, uint64_t *rm_clock /* [Q][A] */,
                             uint32_t *status /* [Q] */);
int crdt_map_nested_get(crdt_ctx *ctx, const crdt_map_nested_states *states, const uint32_t *state_idx,
                        const uint32_t *key, size_t Q, uint8_t *present /* [Q] */, uint64_t *rm_clock /* [Q][A] */,
                        uint64_t *val_clock /* [Q][A] */, uint64_t *ikeys /* [Q][K2w] */, uint32_t *len /* [Q] */,
                        uint32_t *status /* [Q] */);
int crdt_map_nested_get_inner(crdt_ctx *ctx, const crdt_map_nested_states *states, const uint32_t *state_idx,
                              const uint32_t *key, const uint32_t *ikey, size_t Q, uint8_t *present /* [Q] */,
                              uint64_t *add_clock /* [Q][A] */, uint64_t *rm_clock /* [Q][A] */,
                              uint64_t *vclk /* [Q][Vs][A] */, uint64_t *vval /* [Q][Vs] */, uint32_t *nval /* [Q] */,
                              uint64_t *val_clock /* [Q][A] */, uint32_t *status /* [Q] */);

/* ReadCtx::derive_add_ctx (ctx.rs:40-48: dot = add_clock.inc(actor); add_clock.apply(dot)) of Q
 * clock rows: out_clock + q*out_stride = clock + q*clock_stride with [actor[q]] += 1, counter[q] =
 * that new value (the AddCtx's dot is (actor[q], counter[q])).  out_clock may be clock itself
 * (same pointer and stride).  status[q]: bit 1 = actor[q] >= A, bit 2 = the actor's counter is
 * already UINT64_MAX; in both cases the row is copied unchanged and counter[q] = 0.
 * ReadCtx::derive_rm_ctx (ctx.rs:51-55) needs no call: its clock is the rm_clock row. */
int crdt_vclock_derive_add(crdt_ctx *ctx, const uint64_t *clock, size_t clock_stride, size_t Q, size_t A,
                           const uint32_t *actor, uint64_t *out_clock, size_t out_stride, uint64_t *counter /* [Q] */,
                           uint32_t *status /* [Q] */);

/* ---- batched CmRDT::apply ---------------------------------------------------
 * Apply n_ops ops to N dense states; op i targets state state_idx[i] (row at
 * states + state_idx[i]*row_stride).  The ops of these types are per-cell joins, so they commute:
 * the batch equals applying them one by one in any order, as the reference's apply does.
 *   VClock::apply / apply_dot (vclock.rs:125-127, :155-159), GCounter::apply (gcounter.rs:39-41):
 *       row[actor[i]] = max(row[actor[i]], counter[i])                       (A-word rows)
 *   PNCounter::apply (pncounter.rs:62-67): dir[i] == 0 (Dir::Pos) -> P column actor[i],
 *       1 (Dir::Neg) -> N column A + actor[i]                                 (2A-word rows P ‖ N)
 *   GSet::apply / insert (gset.rs:46-48, :69-71): set bit element[i] of a ceil(U/64)-word bitmap
 * state_idx / actor / element are device u32, counter device u64, dir device u8.  Ops with
 * state_idx >= N or actor >= A (element >= U) are skipped and counted into *bad (device u32,
 * added to; may be NULL). */
int crdt_vclock_apply_batch(crdt_ctx *ctx, uint64_t *states, size_t N, size_t A, size_t row_stride,
                            const uint32_t *state_idx, const uint32_t *actor, const uint64_t *counter,
                            size_t n_ops, uint32_t *bad);
int crdt_gcounter_apply_batch(crdt_ctx *ctx, uint64_t *states, size_t N, size_t A, size_t row_stride,
                              const uint32_t *state_idx, const uint32_t *actor, const uint64_t *counter,
                              size_t n_ops, uint32_t *bad);
int crdt_pncounter_apply_batch(crdt_ctx *ctx, uint64_t *states, size_t N, size_t A, size_t row_stride,
                               const uint32_t *state_idx, const uint32_t *actor, const uint64_t *counter,
                               const uint8_t *dir, size_t n_ops, uint32_t *bad);
int crdt_gset_apply_batch(crdt_ctx *ctx, uint64_t *states, size_t N, size_t U, size_t row_stride,
                          const uint32_t *state_idx, const uint32_t *element, size_t n_ops, uint32_t *bad);

/* ---- serde wire format ingest / egress -------------------------------------
 * Replicas ship whole states serialized through the serde derives of the reference types
 * (vclock.rs:56, gcounter.rs:25, pncounter.rs:28, gset.rs:7, lwwreg.rs:13, orswot.rs:20).  These
 * entry points read / write the bytes `bincode::serialize` (bincode 1.x default options) produces:
 * little-endian fixed-width integers, a struct = its fields in order, a map / set / Vec = u64 length
 * then its entries (key, value).  Instantiations: actors u32, members / set elements u64:
 *   VClock<u32> = GCounter<u32>: u64 n, n x (u32 actor, u64 counter)        (actors ascending)
 *   PNCounter<u32>: GCounter p then GCounter n
 *   GSet<u64>: u64 n, n x u64 (ascending);  LWWReg<u64, u64>: u64 val, u64 marker
 *   Orswot<u64, u32>: VClock clock; u64 n, n x (u64 member, VClock); u64 d, d x (VClock rm,
 *       u64 k, k x u64 member)                     (HashMap / HashSet: any order on input)
 * Frames (device): state s is bytes[frame_off[s] .. frame_off[s+1]), offsets 4-byte aligned.
 * Dictionaries (device, ascending, unique): the dense column / bit / row of an id is its position.
 * status[s] (device u32): bit 0 = malformed frame (truncated, trailing bytes, misaligned), bit 1 = an
 * id missing from its dictionary (skipped), bit 2 = more deferred removes than def_cap.
 * Egress writes the same format (maps in ascending dictionary order) and the frame offsets
 * (device, N+1); it always returns the byte total in *total (host, synchronises) and writes the
 * bytes only when `bytes` is non-NULL and cap >= *total (call once with NULL to size a buffer).
 * Limits: A <= 4096 (VClock family), ceil(U/64) <= 4096, A + ceil(M/64) <= 4096 (Orswot). */
int crdt_vclock_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                       const uint32_t *actors, size_t A, uint64_t *out, size_t row_stride, uint32_t *status);
int crdt_pncounter_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                          const uint32_t *actors, size_t A, uint64_t *out, size_t row_stride, uint32_t *status);
int crdt_gset_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                     const uint64_t *elems, size_t U, uint64_t *out, size_t row_stride, uint32_t *status);
int crdt_lwwreg_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                       uint64_t *marker, uint64_t *val, uint32_t *status);
/* Orswot: clock [N][A], entries [N][M][A] (zero-filled, then the present members' rows), the
 * deferred removes pooled in state order: def_off [N+1] (device, written), rows d < def_cap of
 * def_clock [D][A] / def_members [D][ceil(M/64)], *n_def = D (host). */
int crdt_orswot_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                       const uint32_t *actors, size_t A, const uint64_t *members, size_t M, uint64_t *clock,
                       uint64_t *entries, uint64_t *def_off, uint64_t *def_clock, uint64_t *def_members,
                       size_t def_cap, size_t *n_def, uint32_t *status);
int crdt_vclock_egress(crdt_ctx *ctx, const uint64_t *rows, size_t N, size_t A, size_t row_stride,
                       const uint32_t *actors, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);
int crdt_pncounter_egress(crdt_ctx *ctx, const uint64_t *rows, size_t N, size_t A, size_t row_stride,
                          const uint32_t *actors, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);
int crdt_gset_egress(crdt_ctx *ctx, const uint64_t *rows, size_t N, size_t U, size_t row_stride,
                     const uint64_t *elems, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);
/* 16 bytes per state at bytes + 16*s (val, marker). */
int crdt_lwwreg_egress(crdt_ctx *ctx, const uint64_t *marker, const uint64_t *val, size_t N, uint8_t *bytes);
/* Orswot states (clock [N][A], entries [N][M][A] packed) and their deferred removes pooled by state
 * (def_off device [N+1] or NULL = none; def_keep [D] or NULL = all kept): the lub_many output
 * shape with def_off as a device array. */
int crdt_orswot_egress(crdt_ctx *ctx, const uint64_t *clock, const uint64_t *entries, size_t N, size_t M, size_t A,
                       const uint32_t *actors, const uint64_t *members, const uint64_t *def_off,
                       const uint64_t *def_clock, const uint64_t *def_members, const uint8_t *def_keep,
                       uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);
/* Map<u32, MVReg<u64, u32>, u32> (BASELINE config 4's type; map.rs:31-47, mvreg.rs:32-35) frames
 * <-> packed crdt_map_states: clock_stride A, ec_stride K*A, vclk_stride K*V*A, vval_stride K*V;
 * key k = position of its u32 id in the sorted `keys` dictionary, MVReg values in Vec order in
 * slots 0.., and per-state deferred slots of a crdt_map_deferred.  Ingest status bits as above
 * (4 = a key had more than V values or a state more than Dcap removes: the excess was dropped).
 * Egress writes present keys ascending, occupied value slots in slot order, count[s] removes. */
int crdt_map_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, const uint32_t *actors,
                    const uint32_t *keys, const crdt_map_states *out, const crdt_map_deferred *out_def,
                    uint32_t *status);
int crdt_map_egress(crdt_ctx *ctx, const crdt_map_states *states, const crdt_map_deferred *def, const uint32_t *actors,
                    const uint32_t *keys, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);
/* The value-typed Maps (round 5): Map<u32, GCounter<u32>, u32> / Map<u32, PNCounter<u32>, u32>
 * (W = 1 / 2) frames <-> packed crdt_map_counter_states: clock_stride A, ec_stride K*A, val_stride
 * K*W*A; and Map<u32, Orswot<u64, u32>, u32> frames <-> crdt_map_orswot_states: the nested Orswot's
 * clock oc, member dots ent by the sorted u64 `members` dictionary, its deferred removes in slots
 * 0 .. vd_n[s][k] < Vd with member bitmaps vd_mem [N][K][Vd][ceil(M/64)]; the Map's deferred removes
 * in per-state slots, a crdt_map_deferred.  Value encodings: GCounter = VClock, PNCounter = VClock p,
 * VClock n, Orswot as crdt_orswot_ingest.  Ingest status bits as above (4 = a state held more than
 * Dcap Map removes or a key's Orswot more than Vd: the excess was dropped).  Egress writes present
 * keys ascending (entry clock nonzero), present members ascending (dot row nonzero), vd_n nested
 * removes and count[s] Map removes with their ids ascending. */
int crdt_map_counter_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, const uint32_t *actors,
                            const uint32_t *keys, const crdt_map_counter_states *out, const crdt_map_deferred *out_def,
                            uint32_t *status);
int crdt_map_counter_egress(crdt_ctx *ctx, const crdt_map_counter_states *states, const crdt_map_deferred *def,
                            const uint32_t *actors, const uint32_t *keys, uint64_t *frame_off, uint8_t *bytes,
                            size_t cap, size_t *total);
int crdt_map_orswot_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, const uint32_t *actors,
                           const uint32_t *keys, const uint64_t *members, const crdt_map_orswot_states *out,
                           const crdt_map_deferred *out_def, uint32_t *status);
int crdt_map_orswot_egress(crdt_ctx *ctx, const crdt_map_orswot_states *states, const crdt_map_deferred *def,
                           const uint32_t *actors, const uint32_t *keys, const uint64_t *members, uint64_t *frame_off,
                           uint8_t *bytes, size_t cap, size_t *total);
/* Map<u32, Map<u32, MVReg<u64, u32>, u32>, u32> (the reference's own Map test type, test/map.rs:10)
 * frames <-> crdt_map_nested_states: the inner Map's clock ic, its entries by the sorted u32 inner-key
 * dictionary `ikeys` (K2 <= 256, round 6) with their MVReg values in slots 0 .. nval < 8 (Vec order), its
 * deferred removes in slots 0 .. id_n < 16 with a K2w-word inner-key mask each; the outer Map's removes in
 * per-state slots.  Status bit 4: a register past 8 values, an inner list past 16 or an outer one
 * past Dcap (the excess dropped). */
int crdt_map_nested_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, const uint32_t *actors,
                           const uint32_t *keys, const uint32_t *ikeys, const crdt_map_nested_states *out,
                           const crdt_map_deferred *out_def, uint32_t *status);
int crdt_map_nested_egress(crdt_ctx *ctx, const crdt_map_nested_states *states, const crdt_map_deferred *def,
                           const uint32_t *actors, const uint32_t *keys, const uint32_t *ikeys, uint64_t *frame_off,
                           uint8_t *bytes, size_t cap, size_t *total);

/* ---- serde wire format of op streams (CmRDT ops on the wire) -----------------------------------
 * The reference's ops derive Serialize / Deserialize like its states (orswot.rs:31-47,
 * map.rs:50-68, mvreg.rs:38-47, vclock.rs:32-38).  These entry points turn bincode 1.x frames of
 * op streams into the dense batches crdt_orswot_apply_batch / crdt_map_apply_batch consume, and
 * back.  The rules above, plus: an enum = u32 variant index, then the variant's fields.
 *   Dot<u32>                 = u32 actor, u64 counter                                  (12 B)
 *   VClock<u32>              = u64 n, n x (u32 actor, u64 counter), actors ascending
 *   orswot::Op<u64, u32>     = u32 0 (Add), Dot, u64 k, k x u64 member       (HashSet: any order)
 *                            | u32 1 (Rm),  VClock, u64 k, k x u64 member
 *   map::Op<u32, MVReg, u32> = u32 0 (Rm),  VClock, u64 k, k x u32 key       (BTreeSet: ascending)
 *                            | u32 1 (Up),  Dot, u32 key, u32 0 (mvreg::Op::Put), VClock, u64 val
 *   frame of state s         = Vec<Op>: u64 n_ops, then the ops back to back
 * e.g. Vec[Add { dot: (7, 3), members: {10} }] is the 40 bytes (as 32-bit words)
 *   1 0 | 0 | 7 3 0 | 1 0 | 10 0.
 * The dense kind arrays keep their meaning (Orswot 0 = Add, Map 0 = Up): the Map tag is flipped on
 * the way in and out.  Frames, dictionaries and status bits follow the state wire form: frames
 * bytes[frame_off[s] .. frame_off[s+1]) with 4-byte-aligned offsets, sorted unique dictionaries,
 * nothing is read past a frame.  Device pointers only.
 *
 * Ingest fills a crdt_*_ops_buf: the mutable twin of crdt_orswot_ops / crdt_map_ops, with the same
 * field order and sizes and capacities where the const struct holds counts, so a filled buffer can be cast
 * and handed to the apply call as is.  kind / actor / counter / rm_row (key, val, clk_row) hold
 * op_cap entries, mem_off (key_off) op_cap + 1, rm_clock (clk_pool) row_cap x A, mem (keys)
 * id_cap; row_cap <= 2^32 - 1.  Three per-state offset arrays (device, N+1, written): op_off
 * (in the buffer: the one apply takes), row_off and id_off (the state's first clock row and first
 * member / keyset key).  Layout: ops in frame order, states in order.  Orswot: rm_row[o] numbers
 * the Rm clock rows in op order across the batch (0 on Adds); mem_off / mem hold every op's members
 * in frame order, duplicates kept.  Map: clk_row[o] is one row per op (the Put clock of an Up, the
 * rm clock of an Rm); val / key / actor / counter are 0 on Rms; key_off[o+1] = key_off[o] on Ups.
 * Clock rows are dense [rows][A].  Every element of the first n_ops / n_rows / n_ids entries (+1
 * for mem_off / key_off) is written by the call: nothing needs pre-zeroing.
 * totals (host, may be NULL): non-NULL = the call synchronises once and returns {ops, rows, ids}
 * of all well-formed frames (what the capacities must hold); with out = NULL it only sizes (status
 * then carries bit 0 only).  NULL = no host synchronisation: capacities are checked on the device.
 * A state whose ops, rows or ids end past a capacity gets status bit 2 and contributes no ops; its
 * three offsets repeat the previous state's.  The cut is a suffix: every state after the first one
 * cut gets bit 2 and no ops as well, an empty or small one that would have fit included (its ops
 * end past the same capacity in the uncut layout), so the states kept are always a prefix of the
 * batch, laid out exactly as a call with enough room lays them out.  Nothing is written past a
 * capacity.  Bounds to size by without a sync, B_s = bytes of frame s:
 * ops <= (B_s - 8) / 20 (the smallest op, an Rm with an empty clock and set, is 4 + 8 + 8 bytes),
 * rows <= ops, ids <= B_s / 8 (Orswot) or B_s / 4 (Map).
 * status[s] (device u32, written for every s): bit 0 = malformed (truncated, trailing bytes,
 * misaligned offset, a count that cannot fit the bytes left, an unknown variant tag, a Map Up whose
 * MVReg tag is not 0): the frame contributes no ops at all and shifts no neighbour's offsets;
 * bit 1 = an id missing from its dictionary: in a clock record the record is skipped, as a dot's
 * actor, an Up's key or a set's member / key it is written as 0xFFFFFFFF (the apply kernels skip
 * and report that in their bit 1; the op keeps its place); bit 2 = capacity.
 * Egress writes the frames of N states' op streams with the sizing protocol of crdt_orswot_egress
 * (*total always; the bytes when `bytes` is non-NULL and cap >= *total).  status[s] (device u32,
 * written): bit 1 = the state has an op with no wire form (a kind other than 0 / 1, an index >= A /
 * M / K, a row >= its pool, an id range reversed or ending past n_mem / n_keys, an invalid op_off);
 * its frame is the empty Vec (u64 0).  Clock rows are written as their non-zero actors ascending,
 * id lists in list order, so ingest -> egress reproduces byte for byte any well-formed frame whose
 * ids are all in the dictionaries.  Limits: none on A, M, K (dictionaries that do not fit beside the
 * frame ring in 64 KiB of LDS are searched in global memory). */
typedef struct crdt_orswot_ops_buf {
  size_t op_cap;
  uint64_t *op_off;   /* [N+1]        */
  uint8_t *kind;      /* [op_cap]     */
  uint32_t *actor;    /* [op_cap]     */
  uint64_t *counter;  /* [op_cap]     */
  uint32_t *rm_row;   /* [op_cap]     */
  uint64_t *rm_clock; /* [row_cap][A] */
  size_t row_cap;
  uint64_t *mem_off;  /* [op_cap+1]   */
  uint32_t *mem;      /* [id_cap]     */
  size_t id_cap;
} crdt_orswot_ops_buf;

typedef struct crdt_map_ops_buf {
  size_t op_cap;
  uint64_t *op_off;   /* [N+1]        */
  uint8_t *kind;      /* [op_cap]     */
  uint32_t *actor;    /* [op_cap]     */
  uint64_t *counter;  /* [op_cap]     */
  uint32_t *key;      /* [op_cap]     */
  uint64_t *val;      /* [op_cap]     */
  uint32_t *clk_row;  /* [op_cap]     */
  uint64_t *clk_pool; /* [row_cap][A] */
  size_t row_cap;
  uint64_t *key_off;  /* [op_cap+1]   */
  uint32_t *keys;     /* [id_cap]     */
  size_t id_cap;
} crdt_map_ops_buf;

int crdt_orswot_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const uint32_t *actors, size_t A, const uint64_t *members, size_t M,
                           const crdt_orswot_ops_buf *out, uint64_t *row_off, uint64_t *id_off, uint32_t *status,
                           uint64_t *totals);
int crdt_map_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                        const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const crdt_map_ops_buf *out,
                        uint64_t *row_off, uint64_t *id_off, uint32_t *status, uint64_t *totals);
int crdt_orswot_ops_egress(crdt_ctx *ctx, const crdt_orswot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                           const uint64_t *members, size_t M, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                           size_t *total, uint32_t *status);
int crdt_map_ops_egress(crdt_ctx *ctx, const crdt_map_ops *ops, size_t N, const uint32_t *actors, size_t A,
                        const uint32_t *keys, size_t K, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total,
                        uint32_t *status);

/* ---- serde wire format of the value-typed Maps' op streams -------------------------------------
 * Frames of Vec<map::Op<u32, V, u32>> for V = GCounter<u32>, PNCounter<u32>, Orswot<u64, u32> and
 * Map<u32, MVReg<u64, u32>, u32> (map.rs:50-68 with gcounter.rs:37, pncounter.rs:35-51,
 * orswot.rs:31-47, mvreg.rs:38-47 inside) <-> the dense batches of crdt_map_counter_apply_batch /
 * crdt_map_orswot_apply_batch / crdt_map_nested_apply_batch.  The rules above; in 32-bit words:
 *   Op::Rm (every V)   = 0, VClock, u64 k, k x u32 key              (BTreeSet: ascending)  5 + 3n + k
 *   Op::Up, GCounter   = 1, Dot, u32 key, Dot                                                8
 *   Op::Up, PNCounter  = 1, Dot, u32 key, Dot, u32 dir (0 Pos, 1 Neg)                        9
 *   Op::Up, Orswot     = 1, Dot, u32 key, 0 (Add), Dot, u64 k, k x u64 member                11 + 2k
 *                      | 1, Dot, u32 key, 1 (Rm), VClock, u64 k, k x u64 member              10 + 3n + 2k
 *   Op::Up, Map<MVReg> = 1, Dot, u32 key, 0 (inner Rm), VClock, u64 k, k x u32 ikey          10 + 3n + k
 *                      | 1, Dot, u32 key, 1 (inner Up), Dot, u32 ikey, 0 (Put), VClock, u64 val  15 + 3n
 *   frame of state s   = u64 n_ops, then the ops back to back
 * e.g. Vec[Up { dot: (7, 3), key: 5, op: Dot (7, 2) }] of a Map<u32, GCounter> is the 40 bytes
 *   1 0 | 1 | 7 3 0 | 5 | 7 2 0.
 * The dense kind (0 = Up, 1 = Rm) and ikind (0 = inner Up, 1 = inner Rm) keep the apply structs'
 * meaning: both wire tags are flipped on the way in and out; vkind (0 = Add, 1 = Rm) and vdir match
 * the wire.  Frames, dictionaries (idict: the sorted u32 inner-key dictionary, K2 <= 256, else
 * CRDT_EUNSUPPORTED before any launch), alignment and device-pointers-only as for crdt_map_ops_ingest.
 *
 * Ingest fills a crdt_map_*_ops_buf, the mutable twin of the const struct (same field order and
 * sizes, capacities where it holds counts), laid out as the host encoders of crdts_gpu/map.py lay a
 * batch out.  Counter Maps: clk_row numbers one pool row per Map Rm in op order across the batch, 0
 * on Ups; the Up-only fields are 0 on Rms; key_off[o+1] = key_off[o] on Ups; pn = 0 reads GCounter
 * frames (vdir written 0), pn = 1 PNCounter frames.  Orswot Map: one pool row per Orswot Rm and per
 * Map Rm, none for an Add (clk_row 0); mem_off / mems hold every Up's members in frame order,
 * duplicates kept; key_off / keys the Map Rm keysets.  Nested Map: one pool row per op (the Put
 * clock, the inner rm clock or the outer rm clock); an inner Rm's keyset becomes the mask ikeys
 * [op_cap][K2w] (K2w = 1 up to K2 = 64, else ceil(K2 / 64)), zero on every other op.  Every element
 * the counts cover is written: nothing needs pre-zeroing.  Per-state offsets (device, N+1, written):
 * op_off, row_off, key_first (the state's first keyset key) and, for the Orswot Map, mem_first.
 * totals (host, may be NULL) = {ops, rows, keys, mems} of the well-formed frames, four words for
 * all three types (mems = 0 where there is no member pool).  The sizing call (out = NULL), the
 * no-sync path (totals = NULL) and the suffix cut are those of crdt_map_ops_ingest, over three
 * (Orswot Map: four) capacities: the first state over any capacity and every state after it get
 * bit 2 and no ops, the states kept are a prefix laid out as an uncut call lays them out, nothing
 * is written past a capacity.  No-sync bounds, B_s = bytes of frame s: ops <= (B_s - 8) / 20 (the
 * smallest op is still the 20-byte Rm), rows <= ops, keys <= B_s / 4, mems <= B_s / 8.
 * status[s] (written for every s): bit 0 = malformed (as crdt_map_ops_ingest, plus an unknown value
 * tag, a PNCounter dir > 1, an inner Up whose MVReg tag is not 0): no ops, no neighbour's offsets
 * shifted; bit 1 = an id missing from its dictionary: a clock record is skipped; a dot's actor, an
 * Up's key, a member, a keyset key or an inner Up's ikey is written as 0xFFFFFFFF (the apply kernels
 * skip and report these); a missing inner-Rm key is left out of the mask; bit 2 = capacity.
 * Egress: the sizing protocol of crdt_map_ops_egress.  status[s] bit 1 = the state has an op with no
 * wire form (a kind / vkind / ikind / vdir other than 0 or 1, vdir = 1 with pn = 0, an index >= A /
 * K / M / K2 or a mask bit >= K2, a row >= its pool, an id range reversed or past its pool, a Map Rm
 * while key_off is NULL, an invalid op_off); its frame is the empty Vec.  vdir = NULL: all P.  Clock
 * rows are written as their non-zero actors ascending, id lists in list order, mask bits ascending,
 * so ingest -> egress reproduces byte for byte any well-formed frame whose ids are all in the
 * dictionaries. */
typedef struct crdt_map_counter_ops_buf {
  size_t op_cap;
  uint64_t *op_off;    /* [N+1]        */
  uint8_t *kind;       /* [op_cap]     */
  uint32_t *actor;     /* [op_cap]     */
  uint64_t *counter;   /* [op_cap]     */
  uint32_t *key;       /* [op_cap]     */
  uint32_t *vactor;    /* [op_cap]     */
  uint64_t *vcounter;  /* [op_cap]     */
  uint8_t *vdir;       /* [op_cap]     */
  uint32_t *clk_row;   /* [op_cap]     */
  uint64_t *clk_pool;  /* [row_cap][A] */
  size_t row_cap;
  uint64_t *key_off;   /* [op_cap+1]   */
  uint32_t *keys;      /* [key_cap]    */
  size_t key_cap;
} crdt_map_counter_ops_buf;

typedef struct crdt_map_orswot_ops_buf {
  size_t op_cap;
  uint64_t *op_off;    /* [N+1]        */
  uint8_t *kind;       /* [op_cap]     */
  uint32_t *actor;     /* [op_cap]     */
  uint64_t *counter;   /* [op_cap]     */
  uint32_t *key;       /* [op_cap]     */
  uint8_t *vkind;      /* [op_cap]     */
  uint32_t *vactor;    /* [op_cap]     */
  uint64_t *vcounter;  /* [op_cap]     */
  uint32_t *clk_row;   /* [op_cap]     */
  uint64_t *clk_pool;  /* [row_cap][A] */
  size_t row_cap;
  uint64_t *key_off;   /* [op_cap+1]   */
  uint32_t *keys;      /* [key_cap]    */
  size_t key_cap;
  uint64_t *mem_off;   /* [op_cap+1]   */
  uint32_t *mems;      /* [mem_cap]    */
  size_t mem_cap;
} crdt_map_orswot_ops_buf;

typedef struct crdt_map_nested_ops_buf {
  size_t op_cap;
  uint64_t *op_off;    /* [N+1]        */
  uint8_t *kind;       /* [op_cap]     */
  uint32_t *actor;     /* [op_cap]     */
  uint64_t *counter;   /* [op_cap]     */
  uint32_t *key;       /* [op_cap]     */
  uint8_t *ikind;      /* [op_cap]     */
  uint32_t *iactor;    /* [op_cap]     */
  uint64_t *icounter;  /* [op_cap]     */
  uint32_t *ikey;      /* [op_cap]     */
  uint64_t *val;       /* [op_cap]     */
  uint64_t *ikeys;     /* [op_cap][K2w] */
  uint32_t *clk_row;   /* [op_cap]     */
  uint64_t *clk_pool;  /* [row_cap][A] */
  size_t row_cap;
  uint64_t *key_off;   /* [op_cap+1]   */
  uint32_t *keys;      /* [key_cap]    */
  size_t key_cap;
} crdt_map_nested_ops_buf;

int crdt_map_counter_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                                const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, int pn,
                                const crdt_map_counter_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                                uint32_t *status, uint64_t *totals);
int crdt_map_orswot_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                               const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const uint64_t *members,
                               size_t M, const crdt_map_orswot_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                               uint64_t *mem_first, uint32_t *status, uint64_t *totals);
int crdt_map_nested_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                               const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const uint32_t *idict,
                               size_t K2, const crdt_map_nested_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                               uint32_t *status, uint64_t *totals);
int crdt_map_counter_ops_egress(crdt_ctx *ctx, const crdt_map_counter_ops *ops, size_t N, const uint32_t *actors, size_t A,
                                const uint32_t *keys, size_t K, int pn, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                                size_t *total, uint32_t *status);
int crdt_map_orswot_ops_egress(crdt_ctx *ctx, const crdt_map_orswot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                               const uint32_t *keys, size_t K, const uint64_t *members, size_t M, uint64_t *frame_off,
                               uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);
int crdt_map_nested_ops_egress(crdt_ctx *ctx, const crdt_map_nested_ops *ops, size_t N, const uint32_t *actors, size_t A,
                               const uint32_t *keys, size_t K, const uint32_t *idict, size_t K2, uint64_t *frame_off,
                               uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);

/* ---- serde wire format of MVReg<u64, u32> on its own: states ----------------------------------------
 * MVReg derives Serialize / Deserialize (mvreg.rs:32); these entry points read / write a register
 * outside a Map:
 *   MVReg<u64, u32> = u64 n, n x (VClock<u32> clock, u64 val), values in Vec order
 * e.g. MVReg { vals: [({7: 3}, 10)] } is the 36 bytes (as 32-bit words) 1 0 | 1 0 | 7 3 0 | 10 0.
 * Frames, the actor dictionary and alignment follow the state wire form above; device pointers only.
 * Ingest fills `out` (N registers of A actors and V slots; strides honoured) and writes every slot
 * of every register: the values kept from slot 0 in Vec order, the rest zero (nothing needs
 * pre-zeroing).  status[s] (device u32, written for every s): bit 0 = malformed frame (truncated,
 * trailing bytes, misaligned offset, a count that cannot fit the bytes left): the register is written
 * empty; bit 1 = an actor missing from the dictionary: that record is skipped; bit 2 = more than V
 * values: the first V are kept; bit 3 = a value whose clock is empty on the wire, or empties once
 * unknown actors are skipped: it has no dense form (an all-zero row is an empty slot) and is dropped.
 * Egress uses the sizing protocol of crdt_orswot_egress (*total always written; the bytes when `bytes`
 * is non-NULL and cap >= *total; frame_off device, N+1) and writes occupied slots in slot order, clock
 * records in ascending dictionary order.  Ingest -> egress reproduces byte for byte any well-formed
 * frame whose actors are all in the dictionary and which has no empty-clock value and at most V
 * values.  One wave per frame, through the register parser / writer of the Map frames.  Limit: A <= 4096. */
int crdt_mvreg_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                      const uint32_t *actors, size_t A, const crdt_mvreg_states *out, uint32_t *status);
int crdt_mvreg_egress(crdt_ctx *ctx, const crdt_mvreg_states *states, const uint32_t *actors,
                      uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total);

/* ---- serde wire format of MVReg<u64, u32> on its own: Put streams ------------------------------------
 * mvreg::Op::Put derives serde (mvreg.rs:38-47):
 *   mvreg::Op<u64, u32> = u32 0 (Put), VClock clock, u64 val
 *   frame of register i = Vec<Op>: u64 n_ops, then the ops back to back
 * e.g. Vec[Put { clock: {7: 3}, val: 10 }] is the 40 bytes (as words) 1 0 | 0 | 1 0 | 7 3 0 | 10 0.
 * The contract is the one stated for crdt_orswot_ops_ingest, restricted to ops and rows.  Ingest fills
 * a crdt_mvreg_ops_buf, the mutable twin of crdt_mvreg_ops with the same field order and sizes and
 * capacities where the const struct holds counts: a filled buffer casts to crdt_mvreg_ops and goes to
 * crdt_mvreg_apply_batch as is.  One clock row per op: clk_row[o] = o, rows == ops; clk_row / val
 * hold op_cap entries, clk_pool row_cap x A (row_cap <= 2^32 - 1), op_off N+1.  Every element of the
 * first n_ops entries is written by the call.  A Put with an empty clock is a valid op, kept with an
 * all-zero row (MVReg::apply ignores it, mvreg.rs:136-138, and so does crdt_mvreg_apply_batch).
 * totals (host, may be NULL): non-NULL = the call synchronises once and returns {ops, rows} of all
 * well-formed frames; with out = NULL it only sizes.  NULL = no host synchronisation: capacities
 * are enforced on the device with the prefix cut rule: the first register whose ops end past
 * min(op_cap, row_cap) and every one after it get bit 2 and contribute no ops, so the registers kept
 * are a prefix laid out exactly as an uncut call lays them out.  To size without a sync:
 * ops <= (B_s - 8) / 20 (the smallest op, a Put with an empty clock, is 4 + 8 + 8 bytes).
 * status[s] (device u32, written for every s): bit 0 = malformed frame (an unknown tag included): it
 * contributes nothing and shifts no neighbour; bit 1 = a clock record's actor is missing: the record
 * is skipped; bit 2 = capacity.
 * Egress is count -> scan -> write with the sizing protocol above.  status[s] bit 1 = the register has
 * an op with no wire form (clk_row >= n_clk_rows, or an invalid op_off): its frame is the empty Vec.
 * Ingest -> egress is byte-identical for well-formed frames whose actors are all in the dictionary.
 * No limit on A (a dictionary that does not fit beside the frame ring in 64 KiB of LDS is searched
 * in global memory). */
typedef struct crdt_mvreg_ops_buf { /* mutable twin of crdt_mvreg_ops: same field order and sizes */
  size_t op_cap;
  uint64_t *op_off;   /* [N+1]        */
  uint32_t *clk_row;  /* [op_cap]     */
  uint64_t *clk_pool; /* [row_cap][A] */
  size_t row_cap;
  uint64_t *val;      /* [op_cap]     */
} crdt_mvreg_ops_buf;

int crdt_mvreg_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                          const uint32_t *actors, size_t A, const crdt_mvreg_ops_buf *out, uint32_t *status,
                          uint64_t *totals);
int crdt_mvreg_ops_egress(crdt_ctx *ctx, const crdt_mvreg_ops *ops, size_t N, const uint32_t *actors, size_t A,
                          uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);

/* ---- serde wire format of the lattice types' op streams ----------------------------------------------
 * The ops of VClock / GCounter, PNCounter, GSet and LWWReg derive serde too; every record is
 * fixed-width, so a frame is exactly 8 + n x rec bytes:
 *   Vec<Dot<u32>>           = u64 n, n x (u32 actor, u64 counter)            rec 12  (vclock.rs:32-38)
 *   Vec<pncounter::Op<u32>> = u64 n, n x (u32 actor, u64 counter, u32 dir)   rec 16  (pncounter.rs:35-51)
 *   Vec<u64>                = u64 n, n x u64 element                         rec 8   (gset.rs:43-49)
 *   Vec<LWWReg<u64, u64>>   = u64 n, n x (u64 val, u64 marker)               rec 16  (lwwreg.rs:13-19, :52)
 * dir: 0 = Pos, 1 = Neg.  GCounter's op is the same Dot (gcounter.rs:36-42): its streams go through
 * the vclock calls.  e.g. (as 32-bit words) Vec[Dot(7, 3)] = 1 0 | 7 3 0; Vec[Op { dot: (7, 3), dir: Neg }] = 1 0 | 7 3 0 1;
 * Vec[LWWReg { val: 10, marker: 2 }] = 1 0 | 10 0 | 2 0.
 * The contract is the one stated for crdt_orswot_ops_ingest, restricted to ops (no rows, no ids): the
 * frames, the sorted unique dictionaries (actors u32; elems u64, the GSet universe; none for LWWReg),
 * the status bits, totals, the sizing call, the no-sync path and the prefix cut.  Ingest fills a
 * crdt_dot_ops_buf / crdt_lwwreg_ops_buf, the mutable twin of crdt_dot_ops / crdt_lwwreg_ops with the
 * same field order and sizes and op_cap where the const struct holds n_ops, so a filled buffer casts
 * to the const struct.  crdt_dot_ops is what crdt_vclock / gcounter / pncounter / gset_apply_batch
 * take (state_idx, actor or element, counter, dir), grouped by state: ops in frame order, states in
 * order, state_idx[o] = the frame's index, op_off (N+1) written; GSet leaves counter and dir alone
 * (may be NULL), VClock dir.  Every element of the first n_ops entries is written by the call.
 * totals (host, may be NULL) = {ops}.  Records are fixed-width, so ops <= (B_s - 8) / rec is an exact
 * bound for a well-formed frame of B_s bytes: a caller can size op_cap without a sync from frame_off
 * alone.
 * status[s] (device u32, written for every s): bit 0 = malformed (a misaligned offset, a frame
 * shorter than 8 bytes, a length other than 8 + n x rec, a dir tag other than 0 / 1): no ops, no
 * neighbour's offsets shifted; bit 1 = an actor / element missing from its dictionary: written as
 * 0xFFFFFFFF, the op keeps its place (the apply kernels skip it and count it into bad); bit 2 =
 * capacity (the prefix cut; nothing is written past op_cap).
 * Egress reads the grouped form (op_off and the arrays, never state_idx) with the sizing protocol of
 * crdt_orswot_egress.  status[s] bit 1 = the state has an op with no wire form (an index >= A / U, a
 * dir > 1, an invalid op_off): its frame is the empty Vec.  Ingest -> egress is byte-identical for
 * well-formed frames whose ids are all in the dictionaries.  Device pointers only.  No limit on A / U
 * (a dictionary past 48 KiB is searched in global memory instead of LDS); N <= 2^32 - 1. */
typedef struct crdt_dot_ops {
  size_t n_ops;
  const uint64_t *op_off;    /* [N+1]                                    */
  const uint32_t *state_idx; /* [n_ops]                                  */
  const uint32_t *actor;     /* [n_ops]  (GSet: the dense element index) */
  const uint64_t *counter;   /* [n_ops]  (GSet: NULL)                    */
  const uint8_t *dir;        /* [n_ops]  (PNCounter only, else NULL)     */
} crdt_dot_ops;

typedef struct crdt_dot_ops_buf { /* mutable twin of crdt_dot_ops: same field order and sizes */
  size_t op_cap;
  uint64_t *op_off;    /* [N+1]    */
  uint32_t *state_idx; /* [op_cap] */
  uint32_t *actor;     /* [op_cap] */
  uint64_t *counter;   /* [op_cap] */
  uint8_t *dir;        /* [op_cap] */
} crdt_dot_ops_buf;

typedef struct crdt_lwwreg_ops_buf { /* mutable twin of crdt_lwwreg_ops: same field order and sizes */
  size_t op_cap;
  uint64_t *op_off; /* [N+1]    */
  uint64_t *marker; /* [op_cap] */
  uint64_t *val;    /* [op_cap] */
} crdt_lwwreg_ops_buf;

int crdt_vclock_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const uint32_t *actors, size_t A, const crdt_dot_ops_buf *out, uint32_t *status,
                           uint64_t *totals);
int crdt_pncounter_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                              const uint32_t *actors, size_t A, const crdt_dot_ops_buf *out, uint32_t *status,
                              uint64_t *totals);
int crdt_gset_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                         const uint64_t *elems, size_t U, const crdt_dot_ops_buf *out, uint32_t *status,
                         uint64_t *totals);
int crdt_lwwreg_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const crdt_lwwreg_ops_buf *out, uint32_t *status, uint64_t *totals);
int crdt_vclock_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                           uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);
int crdt_pncounter_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                              uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);
int crdt_gset_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint64_t *elems, size_t U,
                         uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status);
int crdt_lwwreg_ops_egress(crdt_ctx *ctx, const crdt_lwwreg_ops *ops, size_t N, uint64_t *frame_off, uint8_t *bytes,
                           size_t cap, size_t *total, uint32_t *status);

/* ---- synthetic inputs (bench / test data, generated in HBM) --------------------------------
 * Counter-based and reproducible on the CPU (oracle/oracle.py synth_* restates them; small
 * fixtures of both are pinned by tests/golden/make_golden.py -> tests/golden/synth.json).
 * kind 0 = clock/counter cells, 1 = GSet bitmap words, 2 = LWW markers, 3 = LWW vals.
 * Row r < rows of the output is row (first_row + r) of the global synthetic matrix: cell
 * (first_row + r, i) gets synth(seed, (first_row + r)*width + i), stored at out[r*row_stride + i].
 * (first_row lets every rank generate its own replica shard of one global input.) */
int crdt_synth_fill(crdt_ctx *ctx, uint64_t *out, size_t rows, size_t width, size_t row_stride,
                    size_t first_row, uint64_t seed, int kind);

/* Well-formed synthetic Orswot replicas, packed clock[R][A] and entries[R][M][A] (replica r is
 * global replica first_row + r).  clock[r][a] = synth(seed, r*A + a) % (kmax + 1); actor a's
 * k-th add targets member (a*P + k) mod M (P = 0x9E3779B1 mod M), so a dot is unique and
 * entries[r][m][a] = k <= clock[r][a] or 0: a quarter of the dots are removed, and a replica has
 * observed (zeroed) a removed dot once clock[r][a] >= k + 1 + delta(m, a), delta in 0..7.
 * Requires kmax < M.  Restated on the CPU by oracle.synth_orswot. */
int crdt_synth_orswot(crdt_ctx *ctx, uint64_t *clock, uint64_t *entries, size_t R, size_t M,
                      size_t A, size_t first_row, uint64_t seed, uint64_t kmax);
/* For each deferred remove d held by replica def_row[d] (rm clock def_clock[d*A..], member
 * bitmap def_members[d*Mw..]): forget(rm) on those members of that replica's entries — the
 * state apply_rm (orswot.rs:230-238) leaves behind.  Used to build consistent inputs. */
int crdt_synth_orswot_rm(crdt_ctx *ctx, uint64_t *entries, size_t M, size_t A, size_t D,
                         const uint32_t *def_row, const uint64_t *def_clock,
                         const uint64_t *def_members);

/* Well-formed synthetic Map<K, MVReg<u64>> replicas (config 4), packed clock[R][A],
 * ec[R][K][A], vclk[R][K][V][A], vval[R][K][V] for global replicas first_row + r; model in
 * csrc/synth.hip, restated on the CPU by oracle.synth_map.  def_off (device, R+1 local
 * offsets, may be NULL), def_clock[D][A], def_keys[D][Kw]: the replicas' own deferred removes,
 * pre-applied (apply_keyset_rm, map.rs:318-333). */
int crdt_synth_map(crdt_ctx *ctx, uint64_t *clock, uint64_t *ec, uint64_t *vclk, uint64_t *vval,
                   size_t R, size_t K, size_t A, size_t V, size_t first_row, uint64_t seed,
                   uint64_t kmax, const uint64_t *def_off, const uint64_t *def_clock,
                   const uint64_t *def_keys);

#ifdef __cplusplus
}
#endif
#endif /* CRDT_GPU_H */
