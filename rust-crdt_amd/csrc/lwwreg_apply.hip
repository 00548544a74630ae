// Batched FunkyCmRDT::apply of LWWReg<u64 val, u64 marker> op streams (ragged, one stream per register).
//
// Reference: apply (lwwreg.rs:48-57) -> merge -> update (lwwreg.rs:84-98), op by op:
//     if self.marker < marker                          { self = (val, marker); Ok }
//     elif self.marker == marker && val != self.val    { Err(ConflictingMarker), self unchanged }
//     else Ok (no-op)
// The state after op k of a stream is the join of (the caller's state, op 0 .. op k) under
//     join(a, b) = a.marker >= b.marker ? a : b        (a precedes b: ties keep the held value)
// which is associative (lwwreg.hip's mi_join with the value carried instead of its index), and op k
// errs exactly when its marker equals the marker of the state before it and its value differs.  So a
// batch is a segmented inclusive scan over the concatenated op stream, seeded at every segment's
// first op by the register's state.
//
// One wave per 64 consecutive registers.  Lane = register for the state, the 65 offsets, the status
// and the state written back; lane = op over the group's contiguous op range [off[0], off[64]) in
// steps of 64 ops (coalesced marker / val loads, coalesced conflict bytes).  Per step:
//   owner   every register whose stream starts inside the step drops its lane number at the start's
//           position in a 64-entry LDS row; a ballot of the filled positions gives every op lane its
//           segment's first lane (a clz) and so its owner.  Ops before the first start continue the
//           register open at the end of the previous step.
//   scan    six steps over (marker, val), each taken while its source lane is inside the segment, moved
//           by DPP (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31: VALU, the LDS pipe stays free for the
//           cross-lane gathers); the first lane of a segment joins the register's state (a __shfl
//           from the register's lane) or the carry (lane 63 of the previous step) first.
//   err     op's marker == marker of the scan one lane up (wave_shr 1; the seed on a first lane),
//           values differ.
//   state   a register whose last op is in the step pulls the scan at that lane and stores it.
// A group whose 65 offsets are not non-decreasing and <= n_ops (one ballot) takes a lane-per-register
// loop instead: every register with a valid range of its own is applied, the others get bit 3.
#include "common.hpp"

namespace crdt {

constexpr unsigned kLwwErr = 1u, kLwwBadRange = 8u;
constexpr int kLwwApplyWpb = kBlock / kWave;

struct LwwApplyPlan {
  u64 *marker, *val;  // [N] states, in place
  unsigned long long N, n_ops;
  const u64 *op_off, *om, *ov;
  uint8_t *conflict;  // [n_ops] or null
  uint32_t *status;   // [N] or null
};

struct MV {
  u64 m, v;
};

__device__ __forceinline__ MV mv_join(MV a, MV b) { return a.m >= b.m ? a : b; }  // a precedes b

__device__ __forceinline__ u64 lww_lane64(u64 x, int l) {  // l wave-uniform
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)x, l), hi = __builtin_amdgcn_readlane((unsigned)(x >> 32), l);
  return ((u64)hi << 32) | lo;
}

// x moved across lanes by a DPP control (VALU, no LDS traffic); a lane the control gives no source
// keeps its own x.  Controls: 0x110 + d = row_shr:d (within rows of 16 lanes), 0x138 = wave_shr:1,
// 0x142 / 0x143 = row_bcast:15 / :31 (lane 15 of a row to the next row, lane 31 to rows 2 and 3).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 lww_dpp64(u64 x) {
  const int lo = (int)(unsigned)x, hi = (int)(unsigned)(x >> 32);
  const unsigned rlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  const unsigned rhi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  return ((u64)rhi << 32) | rlo;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ MV mv_dpp(MV x) {
  return MV{lww_dpp64<CTRL, ROW_MASK>(x.m), lww_dpp64<CTRL, ROW_MASK>(x.v)};
}

// Inclusive scan of mv_join over the lanes [s, lane] (s = the lane's segment start, s <= lane): four
// in-row steps, then the two row broadcasts; a step is taken while its source lane is inside the
// segment.  After the in-row steps a lane holds the join over [max(s, row start), lane]; lane 15 of
// the row before (same segment when s is below the row start) completes a 32-lane half, lane 31 the wave.
__device__ __forceinline__ MV mv_segscan(MV x, int lane, int s) {
  const int rl = lane & 15, row0 = lane & ~15;
  MV y;
  y = mv_dpp<0x111, 0xf>(x);
  if (rl >= 1 && lane - 1 >= s) x = mv_join(y, x);
  y = mv_dpp<0x112, 0xf>(x);
  if (rl >= 2 && lane - 2 >= s) x = mv_join(y, x);
  y = mv_dpp<0x114, 0xf>(x);
  if (rl >= 4 && lane - 4 >= s) x = mv_join(y, x);
  y = mv_dpp<0x118, 0xf>(x);
  if (rl >= 8 && lane - 8 >= s) x = mv_join(y, x);
  y = mv_dpp<0x142, 0xa>(x);
  if ((lane & 16) && row0 - 1 >= s) x = mv_join(y, x);
  y = mv_dpp<0x143, 0xc>(x);
  if (lane >= 32 && 31 >= s) x = mv_join(y, x);
  return x;
}

__device__ __forceinline__ void lww_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

__global__ __launch_bounds__(kBlock) void lww_apply_kernel(LwwApplyPlan p) {
  __shared__ int s_head[kLwwApplyWpb][kWave];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  int *head = s_head[wib];
  const unsigned long long ngroups = (p.N + kWave - 1) / kWave;
  for (unsigned long long g = (unsigned long long)blockIdx.x * kLwwApplyWpb + wib; g < ngroups;
       g += (unsigned long long)gridDim.x * kLwwApplyWpb) {
    const unsigned long long g0 = g * kWave;
    const int nreg = p.N - g0 < (unsigned long long)kWave ? (int)(p.N - g0) : kWave;
    const bool reg = lane < nreg;
    u64 b = 0, e = 0, sm = 0, sv = 0;
    if (reg) {
      b = p.op_off[g0 + lane];
      e = p.op_off[g0 + lane + 1];
      sm = p.marker[g0 + lane];
      sv = p.val[g0 + lane];
    }
    const bool bad = reg && (b > e || e > p.n_ops);
    unsigned st = 0;
    if (__ballot(bad)) {
      // a lane per register, each over its own range
      if (reg) {
        if (bad) {
          st = kLwwBadRange;
        } else {
          for (u64 o = b; o < e; ++o) {
            const u64 m = p.om[o], v = p.ov[o];
            uint8_t c = 0;
            if (sm < m) {
              sm = m;
              sv = v;
            } else if (sm == m && sv != v) {
              c = 1;
            }
            if (p.conflict) p.conflict[o] = c;
            st |= c;
          }
          if (b < e) {
            p.marker[g0 + lane] = sm;
            p.val[g0 + lane] = sv;
          }
        }
        if (p.status) p.status[g0 + lane] = st;
      }
      continue;
    }
    const bool has = reg && b < e;
    const u64 B = lww_lane64(b, 0), E = lww_lane64(e, nreg - 1);
    MV carry{0, 0};
    int carry_owner = 0;
    for (u64 base = B; base < E; base += kWave) {
      // the registers whose stream starts in this step, by position
      head[lane] = -1;
      lww_lds_fence();
      if (has && b >= base && b - base < (u64)kWave) head[b - base] = lane;
      lww_lds_fence();
      const int h = head[lane];
      lww_lds_fence();
      const u64 o = base + lane;
      const bool on = o < E;
      MV x{0, 0};
      if (on) {
        x.m = __builtin_nontemporal_load(p.om + o);
        x.v = __builtin_nontemporal_load(p.ov + o);
      }
      const u64 opm = x.m, opv = x.v;
      // the segment's first lane in this step (lane 0 opens the one that continues the carry)
      const u64 hm = __ballot(h >= 0) | 1ull;
      const int s = 63 - __clzll((long long)(hm & (~0ull >> (63 - lane))));
      const int hs = __shfl(h, s, kWave);
      const int owner = hs >= 0 ? hs : carry_owner;
      MV prior;
      prior.m = __shfl(sm, owner, kWave);
      prior.v = __shfl(sv, owner, kWave);
      if (hs < 0) prior = carry;
      if (lane == s) x = mv_join(prior, x);
      x = mv_segscan(x, lane, s);
      // the state each op met: the scan one lane up, or the seed on a segment's first lane
      MV pre = mv_dpp<0x138, 0xf>(x);
      if (lane == s) pre = prior;
      const bool conf = on && opm == pre.m && opv != pre.v;
      if (p.conflict && on) p.conflict[o] = conf ? 1 : 0;
      const u64 cmask = __ballot(conf);
      // register side: errors among my ops of this step; my new state once my last op is in it
      int tl = lane;
      bool fin = false;
      if (has) {
        const u64 lo = b > base ? b : base, hi = e < base + kWave ? e : base + kWave;
        if (lo < hi) {
          const int l0 = (int)(lo - base), l1 = (int)(hi - base);
          const u64 rmask = (l1 == kWave ? ~0ull : (1ull << l1) - 1) & ~((1ull << l0) - 1);
          if (cmask & rmask) st |= kLwwErr;
          if (hi == e) {
            fin = true;
            tl = l1 - 1;
          }
        }
      }
      const u64 nm = __shfl(x.m, tl, kWave), nv = __shfl(x.v, tl, kWave);
      if (fin) {
        p.marker[g0 + lane] = nm;
        p.val[g0 + lane] = nv;
      }
      carry.m = lww_lane64(x.m, kWave - 1);
      carry.v = lww_lane64(x.v, kWave - 1);
      carry_owner = __builtin_amdgcn_readlane(owner, kWave - 1);
    }
    if (p.status && reg) p.status[g0 + lane] = st;
  }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_lwwreg_apply_batch(crdt_ctx *ctx, uint64_t *marker, uint64_t *val, size_t N,
                                       const crdt_lwwreg_ops *ops, uint8_t *conflict, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (N == 0) return CRDT_OK;
  if (!marker || !val || !ops || !ops->op_off) return fail(ctx, CRDT_EINVAL, "lwwreg_apply_batch: NULL states / ops / op_off");
  if (ops->n_ops && (!ops->marker || !ops->val)) return fail(ctx, CRDT_EINVAL, "lwwreg_apply_batch: NULL op arrays");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  LwwApplyPlan p{(u64 *)marker, (u64 *)val, N, ops->n_ops, (const u64 *)ops->op_off, (const u64 *)ops->marker,
                 (const u64 *)ops->val, conflict, status};
  const unsigned long long want = ((N + kWave - 1) / kWave + kLwwApplyWpb - 1) / kLwwApplyWpb;
  const unsigned long long cap = (unsigned long long)ctx->cu_count * 32;
  timing_begin(ctx, "lww_apply");
  hipLaunchKernelGGL(lww_apply_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(kBlock), 0, ctx->stream, p);
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}
