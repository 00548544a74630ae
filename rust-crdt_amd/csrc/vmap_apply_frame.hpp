// The frame the three value-typed Map apply kernels share (csrc/map_counter_apply.hip,
// map_orswot_apply.hip, map_nested_apply.hip): the plans' common fields, the tiered store of the Map's deferred
// removes, apply_deferred (map.rs:311-316) and the whole host side of Map::apply (map.rs:119-137).
// One wave per state, lane l holding actors l + 64 j (j < APL) of every row, the Map clock in
// registers, the Map's deferred removes (rm clock + key bitmap) in LDS for the whole op stream.  Each
// kernel keeps its op-header batch, its Op::Up branch and its key_rm(k, r) ("key k's entry forgets
// r", apply_keyset_rm's per-key step, map.rs:319-333), which it hands to vmap_apply_deferred.
//
// The kernels' prologue, Map-level Rm branch and epilogue are still the same text three times.  They
// were tried here as force-inlined functions (over one state struct, and the Rm alone over
// references): these kernels sit at their register budget with SGPRs spilling into VGPR lanes, and
// the allocation moved every time (scratch grew in half the instances, two lost a wave per SIMD, the
// bench ran 4-25% slower; DESIGN 3.13, profiles/vmap_apply_frame_resources.txt).  A fix to that text
// is made in three places.
//
// Any Dcap in two passes.  PASS 0: the whole list fits the Dl LDS slots.  PASS 1: every state, its
// list in the Dl LDS slots only; a state whose list needs slot Dl stores itself and records the op to
// continue from (resume[s]).  PASS 2 (TIER): those states alone, one wave per workgroup with the whole
// wave-LDS budget as slots and the slots past it used in place in the caller's slot arrays (one
// branch per access).  Two passes rather than one body with the branch: that body compiles the slot
// accesses to flat instructions and cost every state ~40% (2.73 vs 1.90 ms at the bench shape).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace crdt {

// Deferred slots held in LDS per state in passes 0 and 1 (the rest of the caller's Dcap slots wait for
// pass 2).  16 = the round-5 LDS footprint.
constexpr size_t kVmapDl = 16;
constexpr u64 kVmapDone = ~0ull;  // resume[s]: nothing left for pass 2

// The plan.  Each kernel takes its own flat plan struct by value; the host side below is a template
// over it and needs these fields in it, by these names (vmap_plan_fill writes the first three lines,
// vmap_apply_run the last):
//   unsigned long long N, K, A, Kw, Dcap;  u64 *def_clock, *def_keys;  unsigned *def_count;
//   const u64 *op_off;  const uint8_t *kind;  const uint32_t *actor, *key;  const u64 *counter;
//   const uint32_t *clk_row;  const u64 *clk_pool;  unsigned long long n_clk_rows;
//   const u64 *key_off;  const uint32_t *keys;  unsigned long long n_keys, n_ops;  unsigned *status;
//   unsigned long long Dl;  unsigned wpb;  u64 *resume;   (Dl: deferred slots held in LDS; resume: [N],
//   the op offset where a state's stream continues in pass 2, or kVmapDone)
// They are not one base struct the three plans derive from, because where a field sits in the plan
// decides how the kernel loads its arguments, and these kernels feel it: with the shared fields
// moved to a common prefix the counter kernel ran 1.5% slower at the bench shape (1.900 -> 1.928 ms,
// outside the run-to-run spread) and the other two 0.2-0.7%; with each plan's fields where they were,
// every timing is within the parent's spread or faster (profiles/vmap_apply_frame_ab.log).

template <int APL>
__device__ __forceinline__ bool vmap_leq(const u64 (&x)[APL], const u64 (&y)[APL]) {  // x <= y (every word)
  bool b = false;
#pragma unroll
  for (int j = 0; j < APL; ++j) b = b || x[j] > y[j];
  return __ballot(b) == 0;
}

// A state's deferred removes: slots d < Dl in LDS, slots Dl <= d < Dcap in the caller's own slot
// arrays (global memory: a long list runs slower, never incomplete below Dcap).  d is wave-uniform;
// without TIER no d >= Dl is ever asked for.
template <bool TIER>
struct VmapSlots {
  u64 *sclk, *skey;  // [Dl][A] rm clocks, [Dl][Kw] key bitmaps (LDS)
  u64 *gclk, *gkey;  // [Dcap][A], [Dcap][Kw] (the caller's)
  unsigned long long A, Kw, Dl;
  int lane;

  __device__ __forceinline__ bool in_place(unsigned d) const { return TIER && d >= Dl; }
  __device__ __forceinline__ u64 clk(unsigned d, unsigned long long a) const {
    if (in_place(d)) return gclk[d * A + a];
    return sclk[d * A + a];
  }
  __device__ __forceinline__ void set_clk(unsigned d, unsigned long long a, u64 v) const {
    if (in_place(d)) gclk[d * A + a] = v;
    else sclk[d * A + a] = v;
  }
  __device__ __forceinline__ u64 key(unsigned d, unsigned long long w) const {
    if (in_place(d)) return gkey[d * Kw + w];
    return skey[d * Kw + w];
  }
  __device__ __forceinline__ void set_key(unsigned d, unsigned long long w, u64 v) const {
    if (in_place(d)) gkey[d * Kw + w] = v;
    else skey[d * Kw + w] = v;
  }
  template <int APL>
  __device__ __forceinline__ void row(unsigned d, u64 (&r)[APL]) const {  // slot d's clock, by actor lane
#pragma unroll
    for (int j = 0; j < APL; ++j) {
      const unsigned long long a = (unsigned long long)lane + 64ull * j;
      r[j] = a < A ? clk(d, a) : 0ull;
    }
  }
  __device__ __forceinline__ void move(unsigned o, unsigned d) const {  // slot d to slot o
    for (unsigned long long a = (unsigned long long)lane; a < A; a += kWave) set_clk(o, a, clk(d, a));
    for (unsigned long long w = (unsigned long long)lane; w < Kw; w += kWave) set_key(o, w, key(d, w));
  }
  __device__ __forceinline__ void stage_in(unsigned n) const {  // the first n slots, memory -> LDS
    for (unsigned d = 0; d < n && d < Dl; ++d) {
      for (unsigned long long a = (unsigned long long)lane; a < A; a += kWave) sclk[d * A + a] = gclk[d * A + a];
      for (unsigned long long w = (unsigned long long)lane; w < Kw; w += kWave) skey[d * Kw + w] = gkey[d * Kw + w];
    }
  }
  __device__ __forceinline__ void write_back(unsigned n) const {  // (slots past Dl are already in place)
    for (unsigned d = 0; d < n && d < Dl; ++d) {
      for (unsigned long long a = (unsigned long long)lane; a < A; a += kWave) gclk[d * A + a] = sclk[d * A + a];
      for (unsigned long long w = (unsigned long long)lane; w < Kw; w += kWave) gkey[d * Kw + w] = skey[d * Kw + w];
    }
  }
  __device__ __forceinline__ void zero(unsigned lo, unsigned hi) const {  // memory slots [lo, hi)
    for (unsigned d = lo; d < hi; ++d) {
      for (unsigned long long a = (unsigned long long)lane; a < A; a += kWave) gclk[d * A + a] = 0ull;
      for (unsigned long long w = (unsigned long long)lane; w < Kw; w += kWave) gkey[d * Kw + w] = 0ull;
    }
  }
};

// apply_deferred re-forgets every key of every deferred remove (map.rs:311-316).  After one full
// pass each remove's keys are forgotten by its clock, and later ops keep that (an Rm forgets its own
// keys by its clock; forgets are idempotent and commute, so the HashMap's order does not matter)
// except an Up, which changes only its own key's rows: every later pass re-forgets that key kk
// alone — the same rows the full pass would change.  The first pass stays full (the input state
// need not hold the invariant).  A remove stays deferred while !(clock c >= rm).  key_rm(k, r) is
// the value type's "key k's entry forgets r" (apply_keyset_rm's per-key step, map.rs:319-333).
template <int APL, bool TIER, class KeyRm>
__device__ __forceinline__ void vmap_apply_deferred(const VmapSlots<TIER> &sl, unsigned &dcnt, bool &full,
                                                    const u64 (&c)[APL], unsigned long long K, unsigned long long kk,
                                                    KeyRm &&key_rm) {
  unsigned o = 0;
  for (unsigned d = 0; d < dcnt; ++d) {
    u64 r[APL];
    sl.row(d, r);
    for (unsigned long long w = full ? 0 : kk / 64; w < (full ? sl.Kw : kk / 64 + 1); ++w) {
      u64 bits = sl.key(d, w) & (full ? ~0ull : 1ull << (kk % 64));
      while (bits) {
        const unsigned long long k = w * 64 + (unsigned long long)__builtin_ctzll(bits);
        bits &= bits - 1;
        if (k < K) key_rm(k, r);
      }
    }
    if (vmap_leq(r, c)) continue;  // no longer deferred
    if (o != d) sl.move(o, d);
    ++o;
  }
  dcnt = o;
  full = false;
}

// The common fields from an entry point's arguments (Ops: crdt_map_counter_ops / _orswot_ops / _nested_ops,
// which name these fields alike).  Dl, wpb and resume are vmap_apply_run's.
template <class Plan, class Ops>
void vmap_plan_fill(Plan &p, size_t N, size_t K, size_t A, size_t Kw, size_t Dcap, uint64_t *def_clock,
                    uint64_t *def_keys, uint32_t *def_count, const Ops &ops, uint32_t *status) {
  p.N = N, p.K = K, p.A = A, p.Kw = Kw, p.Dcap = Dcap;
  p.def_clock = (u64 *)def_clock, p.def_keys = (u64 *)def_keys, p.def_count = def_count;
  p.op_off = (const u64 *)ops.op_off;
  p.kind = ops.kind, p.actor = ops.actor, p.key = ops.key, p.counter = (const u64 *)ops.counter;
  p.clk_row = ops.clk_row, p.clk_pool = (const u64 *)ops.clk_pool, p.n_clk_rows = ops.clk_pool ? ops.n_clk_rows : 0;
  p.key_off = (const u64 *)ops.key_off, p.keys = ops.keys, p.n_keys = ops.keys ? ops.n_keys : 0;
  p.n_ops = ops.n_ops;
  p.status = status;
}

// The host side of an apply entry point, called once the arguments are checked and the plan is
// filled.  It sizes the LDS slots (a wave's LDS holds at most 8,192 words, `extra` of them the value
// type's), carves the scratch, and launches one pass or two.  go(apl, pass, grid, block, lds) launches
// the kernel instance <apl, pass> with the caller's plan, the one p refers to.
template <class Plan, class Go>
int vmap_apply_run(crdt_ctx *ctx, Plan &p, size_t extra, const char *name, Go &&go) {
  const size_t N = p.N, A = p.A, Kw = p.Kw, Dcap = p.Dcap;
  const size_t Dl = std::min<size_t>(Dcap, std::min<size_t>(kVmapDl, (8192 - extra) / (A + Kw)));
  const size_t per_wave = (Dl * (A + Kw) + extra) * 8;
  unsigned wpb = 4;
  while (wpb > 1 && per_wave * wpb > 64 * 1024) --wpb;
  const bool tier = Dcap > Dl;
  if (tier && p.n_ops >= 0xffffffffull)  // (pass 2 resumes at a 32-bit op offset)
    return fail(ctx, CRDT_EUNSUPPORTED, "%s_batch: 2^32 or more ops with Dcap past the LDS slots", name);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  p.Dl = Dl;
  p.wpb = wpb;
  p.resume = nullptr;
  // an Rm op needs key_off (n_ops + 1 entries); without it every Rm reads an empty key range.  Scratch:
  // [resume: N words when Dcap > Dl][zero key_off: n_ops + 1 words when absent]
  const size_t kz = p.key_off ? 0 : (p.n_ops + 1) * 8, rz = tier ? N * 8 : 0;
  if (kz + rz) {
    if (int rc = ensure_scratch(ctx, kz + rz)) return rc;
    char *sc = static_cast<char *>(ctx->scratch);
    if (tier) p.resume = reinterpret_cast<u64 *>(sc);
    if (kz) {
      if (int rc = device_fill(ctx, sc + rz, kz, 0)) return rc;
      p.key_off = reinterpret_cast<const u64 *>(sc + rz);
    }
  }
  auto launch = [&](auto pass, dim3 g, dim3 b, size_t l) {
    if (A <= 64) go(std::integral_constant<int, 1>{}, pass, g, b, l);
    else if (A <= 128) go(std::integral_constant<int, 2>{}, pass, g, b, l);
    else if (A <= 256) go(std::integral_constant<int, 4>{}, pass, g, b, l);
    else go(std::integral_constant<int, 8>{}, pass, g, b, l);
  };
  const dim3 grid((unsigned)((N + wpb - 1) / wpb)), block(wpb * kWave);
  timing_begin(ctx, name);
  if (!tier) {
    launch(std::integral_constant<int, 0>{}, grid, block, per_wave * wpb);  // the whole list fits the LDS slots
  } else {
    launch(std::integral_constant<int, 1>{}, grid, block, per_wave * wpb);
    // pass 2: the few states pass 1 handed on (the rest exit at once), one wave per workgroup with the
    // whole wave-LDS budget as slots (up to 64 KiB), so a long list mostly stays out of global memory
    const size_t Dl2 = std::min<size_t>(Dcap, (8192 - extra) / (A + Kw));
    p.Dl = Dl2;
    p.wpb = 1;
    launch(std::integral_constant<int, 2>{}, dim3((unsigned)N), dim3(kWave), (Dl2 * (A + Kw) + extra) * 8);
  }
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

}  // namespace crdt
