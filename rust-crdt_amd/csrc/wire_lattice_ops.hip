// Serde wire format of the lattice types' op streams, on the device:
//   crdt_vclock_ops_ingest / _egress     Vec<Dot<u32>>             (VClock and GCounter ops)
//   crdt_pncounter_ops_ingest / _egress  Vec<pncounter::Op<u32>>
//   crdt_gset_ops_ingest / _egress       Vec<u64>                  (GSet ops: the element)
//   crdt_lwwreg_ops_ingest / _egress     Vec<LWWReg<u64, u64>>     (LWWReg's op is the register)
// The bincode 1.x rules of wire.hip; every record is fixed-width, in 32-bit words:
//   Dot<u32>          = actor, counter lo, counter hi              (vclock.rs:32-38)          3
//   pncounter::Op     = Dot, dir (0 = Pos, 1 = Neg)                (pncounter.rs:35-51)       4
//   u64               = lo, hi                                     (gset.rs:43-49)            2
//   LWWReg<u64, u64>  = val lo, val hi, marker lo, marker hi       (lwwreg.rs:13-19)          4
//   frame of state s  = u64 n, then n records: 8 + n x rec bytes, exactly
//
// Fixed-width records need no walk: a frame is well formed when its length is 8 + n x rec (and, for
// PNCounter, every dir tag is 0 / 1), and op i sits at word 2 + i x rec.
// Ingest: count -> exclusive scan -> finalize (the capacity) -> fill.
//   count     a wave per 64 frames, lane = frame (coalesced offsets, one header read); for PNCounter
//             the wave then reads the dir tags of every frame that passed, lane = op, so a frame with
//             a bad tag is out before the scan and shifts no neighbour.
//   fill      a wave per frame, lane = op in steps of 64: three / four / two dword loads per lane
//             (a 12-byte record sits at 4-byte alignment: the counter is two dwords), the dictionary
//             searched in LDS (in global memory when it does not fit), coalesced stores per array.
// Egress: count (validate, frame sizes) -> scan -> write, a wave per state, lane = op.
// One kernel template over the record kind serves the four streams.  (Fixed-width records put op i of a
// state at op_off + i, so neither the op-stream walk nor the in-wave prefix sum of wire_ops_common.hpp
// is needed: the sized ingest and the two-pass egress of wire_driver.hpp are.)
#include "wire_driver.hpp"

namespace crdt {

enum LopKind { kLopDot = 0, kLopPn = 1, kLopGset = 2, kLopLww = 3 };
constexpr int kLopWpb = kBlock / kWave;
constexpr size_t kLopDictLds = 48 << 10;  // dictionary bytes staged in LDS; larger ones are searched in global memory

template <int KIND>
struct LopRec {
  static constexpr unsigned words = KIND == kLopDot ? 3 : (KIND == kLopGset ? 2 : 4);
  static constexpr unsigned bytes = 4 * words;
};

static_assert(sizeof(crdt_dot_ops) == sizeof(crdt_dot_ops_buf), "crdt_dot_ops_buf");
static_assert(offsetof(crdt_dot_ops, n_ops) == offsetof(crdt_dot_ops_buf, op_cap), "crdt_dot_ops_buf");
static_assert(offsetof(crdt_dot_ops, dir) == offsetof(crdt_dot_ops_buf, dir), "crdt_dot_ops_buf");
static_assert(sizeof(crdt_lwwreg_ops) == sizeof(crdt_lwwreg_ops_buf), "crdt_lwwreg_ops_buf");
static_assert(offsetof(crdt_lwwreg_ops, val) == offsetof(crdt_lwwreg_ops_buf, val), "crdt_lwwreg_ops_buf");

struct LopsPlan {
  const uint8_t *bytes;
  const u64 *frame_off;
  unsigned long long N, D;  // D: dictionary entries (A or U; 0 for LWWReg)
  const void *dict;         // u32 actors / u64 elements
  int stage;                // the dictionary is staged in LDS
  u64 *counts;              // [N] (count pass)
  const u64 *op_off;        // [N+1], final (after the capacity)
  uint32_t *status;
  uint32_t *state_idx, *col;  // col: actor / element index
  u64 *counter, *marker, *val;
  uint8_t *dir;
};

__device__ __forceinline__ u64 lop_lane64(u64 x, int l) {  // l wave-uniform
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)x, l), hi = __builtin_amdgcn_readlane((unsigned)(x >> 32), l);
  return ((u64)hi << 32) | lo;
}

// A wave per 64 frames, lane = frame.  status[s] = 0 / bit 0, counts[s] = the frame's ops (0: malformed).
template <int KIND>
__global__ __launch_bounds__(kBlock) void lops_count_kernel(LopsPlan p) {
  constexpr u64 rec = LopRec<KIND>::bytes;
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwv = (unsigned long long)gridDim.x * kLopWpb;
  for (unsigned long long s0 = w0 * kWave; s0 < p.N; s0 += nwv * kWave) {
    const unsigned long long s = s0 + lane;
    const bool in = s < p.N;
    bool ok = false;
    u64 n = 0, b = 0;
    if (in) {
      b = p.frame_off[s];
      const u64 e = p.frame_off[s + 1];
      if (!((b | e) & 3) && e >= b && e - b >= 8) {
        n = rd64(reinterpret_cast<const uint32_t *>(p.bytes + b), 0);
        const u64 len = e - b - 8;
        ok = n <= len / rec && n * rec == len;  // (n <= len / rec first: n * rec cannot wrap)
      }
    }
    if (KIND == kLopPn) {  // the dir tags, before the scan
      u64 todo = __ballot(ok && n > 0);
      while (todo) {
        const int j = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const u64 jn = lop_lane64(n, j);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(p.bytes + lop_lane64(b, j) + 8);
        bool tag = false;
        for (u64 i = lane; i < jn; i += kWave) tag |= w[4 * i + 3] > 1u;
        if (__ballot(tag) && lane == j) ok = false;
      }
    }
    if (in) {
      p.status[s] = ok ? 0u : kWireBad;
      p.counts[s] = ok ? n : 0;
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void lops_fill_kernel(LopsPlan p) {
  extern __shared__ u64 lds[];
  constexpr unsigned W = LopRec<KIND>::words;
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  const uint32_t *actors = static_cast<const uint32_t *>(p.dict);
  const u64 *elems = static_cast<const u64 *>(p.dict);
  if (KIND != kLopLww && p.stage) {
    if (KIND == kLopGset) {
      for (unsigned long long i = threadIdx.x; i < p.D; i += blockDim.x) lds[i] = elems[i];
      elems = lds;
    } else {
      uint32_t *la = reinterpret_cast<uint32_t *>(lds);
      for (unsigned long long i = threadIdx.x; i < p.D; i += blockDim.x) la[i] = actors[i];
      actors = la;
    }
    __syncthreads();
  }
  for (unsigned long long s = (unsigned long long)blockIdx.x * kLopWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kLopWpb) {
    const unsigned st = p.status[s];
    const u64 o0 = p.op_off[s], cnt = p.op_off[s + 1] - o0;
    if ((st & (kWireBad | kWireCap)) || cnt == 0) continue;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p.bytes + p.frame_off[s] + 8);
    bool miss = false;
    for (u64 i = lane; i < cnt; i += kWave) {
      const u64 o = o0 + i;
      const uint32_t *r = w + W * i;
      if (KIND == kLopLww) {
        p.val[o] = rd64(r, 0);
        p.marker[o] = rd64(r, 2);
        continue;
      }
      long long c;
      if (KIND == kLopGset) {
        const u64 el = rd64(r, 0);
        c = find_u64(elems, p.D, el, el);
      } else {
        const uint32_t id = r[0];
        c = find_u32(actors, p.D, id, id);
        p.counter[o] = rd64(r, 1);
        if (KIND == kLopPn) p.dir[o] = (uint8_t)r[3];
      }
      if (c < 0) miss = true;
      p.col[o] = c < 0 ? 0xFFFFFFFFu : (uint32_t)c;
      p.state_idx[o] = (uint32_t)s;
    }
    if (KIND != kLopLww && __ballot(miss) && lane == 0) p.status[s] = st | kWireMissing;
  }
}

struct LopsEgressPlan {
  unsigned long long N, D, n_ops;
  const u64 *op_off;
  const uint32_t *col;
  const u64 *counter, *marker, *val;
  const uint8_t *dir;
  const void *dict;
  u64 *sizes;
  const u64 *frame_off;
  uint8_t *bytes;
  uint32_t *status;
};

// One wave per state, lane = op.  write = 0: validate every op, size the frame (status[s], sizes[s]);
// write = 1: write it at frame_off[s] (the empty Vec for a state with bit 1).
template <int KIND>
__global__ __launch_bounds__(kBlock) void lops_egress_kernel(LopsEgressPlan p, int write) {
  constexpr unsigned W = LopRec<KIND>::words;
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwv = (unsigned long long)gridDim.x * kLopWpb;
  const uint32_t *actors = static_cast<const uint32_t *>(p.dict);
  const u64 *elems = static_cast<const u64 *>(p.dict);
  for (unsigned long long s = w0; s < p.N; s += nwv) {
    const u64 b = p.op_off[s], e = p.op_off[s + 1];
    if (!write) {
      bool inv = e < b || e > p.n_ops;
      if (!inv && KIND != kLopLww) {
        for (u64 o = b + lane; o < e; o += kWave) {
          if (p.col[o] >= p.D) inv = true;
          if (KIND == kLopPn && p.dir[o] > 1) inv = true;
        }
      }
      const bool bad = __ballot(inv) != 0;
      if (lane == 0) {
        p.status[s] = bad ? kWireMissing : 0u;
        p.sizes[s] = bad ? 8 : 8 + (e - b) * (u64)(4 * W);
      }
      continue;
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(p.bytes + p.frame_off[s]);
    if (p.status[s] != 0) {
      if (lane == 0) wr64(out, 0, 0);
      continue;
    }
    if (lane == 0) wr64(out, 0, e - b);
    for (u64 o = b + lane; o < e; o += kWave) {
      uint32_t *r = out + 2 + W * (o - b);
      if (KIND == kLopLww) {
        wr64(r, 0, p.val[o]);
        wr64(r, 2, p.marker[o]);
      } else if (KIND == kLopGset) {
        wr64(r, 0, elems[p.col[o]]);
      } else {
        r[0] = actors[p.col[o]];
        wr64(r, 1, p.counter[o]);
        if (KIND == kLopPn) r[3] = p.dir[o];
      }
    }
  }
}

template <int KIND>
static int lops_ingest(crdt_ctx *ctx, const char *what, LopsPlan &p, u64 cap, bool fill, u64 *op_off, uint64_t *totals) {
  const SizedOut<1> o{{cap}, {op_off}, {nullptr, nullptr}, p.status};
  return sized_ingest<1>(
      ctx, what, p.N, o, fill, totals,
      [&](u64 *counts) {
        p.counts = counts;
        hipLaunchKernelGGL(lops_count_kernel<KIND>, dim3(wave_grid(ctx, (p.N + kWave - 1) / kWave, kLopWpb, 32)), dim3(kBlock),
                           0, ctx->stream, p);
      },
      [&] {
        p.op_off = op_off;
        const size_t dict_bytes = KIND == kLopLww ? 0 : p.D * (KIND == kLopGset ? 8 : 4);
        p.stage = dict_bytes <= kLopDictLds;
        hipLaunchKernelGGL(lops_fill_kernel<KIND>, dim3(wave_grid(ctx, p.N, kLopWpb, 32)), dim3(kBlock),
                           p.stage ? (dict_bytes + 7) / 8 * 8 : 0, ctx->stream, p);
      });
}

// The shared front of the three dictionary-typed ingests.
template <int KIND>
static int dot_ops_ingest(crdt_ctx *ctx, const char *what, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                          const void *dict, size_t D, const crdt_dot_ops_buf *out, uint32_t *status, uint64_t *totals) {
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = 0;
  if (N == 0) return CRDT_OK;
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!dict || D == 0) return fail(ctx, CRDT_EINVAL, "%s: need the dictionary", what);
  if (!out && !totals) return fail(ctx, CRDT_EINVAL, "%s: neither an output nor totals asked for", what);
  if (N > 0xFFFFFFFFull) return fail(ctx, CRDT_EUNSUPPORTED, "%s: state_idx is 32-bit, N = %zu", what, N);
  LopsPlan p{};
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.dict = dict;
  p.D = D;
  p.status = status;
  if (out) {
    if (!out->op_off || (out->op_cap && (!out->state_idx || !out->actor || (KIND != kLopGset && !out->counter) ||
                                         (KIND == kLopPn && !out->dir))))
      return fail(ctx, CRDT_EINVAL, "%s: NULL output array", what);
    p.state_idx = out->state_idx;
    p.col = out->actor;
    p.counter = (u64 *)out->counter;
    p.dir = out->dir;
  }
  return lops_ingest<KIND>(ctx, what, p, out ? out->op_cap : 0, out != nullptr, out ? (u64 *)out->op_off : nullptr, totals);
}

template <int KIND>
static int lops_egress(crdt_ctx *ctx, const char *what, LopsEgressPlan &p, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                       size_t *total) {
  return two_pass_egress(ctx, what, lops_egress_kernel<KIND>, p, wave_grid(ctx, p.N, kLopWpb, 32), frame_off, bytes, cap, total);
}

template <int KIND>
static int dot_ops_egress(crdt_ctx *ctx, const char *what, const crdt_dot_ops *ops, size_t N, const void *dict, size_t D,
                          uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off || !dict || D == 0) return fail(ctx, CRDT_EINVAL, "%s: need ops (op_off) and the dictionary", what);
  if (ops->n_ops && (!ops->actor || (KIND != kLopGset && !ops->counter) || (KIND == kLopPn && !ops->dir)))
    return fail(ctx, CRDT_EINVAL, "%s: NULL op arrays", what);
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "%s: need frame_off, total and status", what);
  LopsEgressPlan p{};
  p.N = N;
  p.D = D;
  p.n_ops = ops->n_ops;
  p.op_off = (const u64 *)ops->op_off;
  p.col = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.dir = ops->dir;
  p.dict = dict;
  p.status = status;
  return lops_egress<KIND>(ctx, what, p, frame_off, bytes, cap, total);
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_vclock_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const uint32_t *actors, size_t A, const crdt_dot_ops_buf *out, uint32_t *status,
                           uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_ingest<kLopDot>(ctx, "wire_vclock_ops_ingest", bytes, frame_off, N, actors, A, out, status, totals);
}

int crdt_pncounter_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                              const uint32_t *actors, size_t A, const crdt_dot_ops_buf *out, uint32_t *status,
                              uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_ingest<kLopPn>(ctx, "wire_pncounter_ops_ingest", bytes, frame_off, N, actors, A, out, status, totals);
}

int crdt_gset_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                         const uint64_t *elems, size_t U, const crdt_dot_ops_buf *out, uint32_t *status,
                         uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_ingest<kLopGset>(ctx, "wire_gset_ops_ingest", bytes, frame_off, N, elems, U, out, status, totals);
}

int crdt_lwwreg_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const crdt_lwwreg_ops_buf *out, uint32_t *status, uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = 0;
  if (N == 0) return CRDT_OK;
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!out && !totals) return fail(ctx, CRDT_EINVAL, "lwwreg_ops_ingest: neither an output nor totals asked for");
  LopsPlan p{};
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.status = status;
  if (out) {
    if (!out->op_off || (out->op_cap && (!out->marker || !out->val)))
      return fail(ctx, CRDT_EINVAL, "lwwreg_ops_ingest: NULL output array");
    p.marker = (u64 *)out->marker;
    p.val = (u64 *)out->val;
  }
  return lops_ingest<kLopLww>(ctx, "wire_lwwreg_ops_ingest", p, out ? out->op_cap : 0, out != nullptr,
                              out ? (u64 *)out->op_off : nullptr, totals);
}

int crdt_vclock_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                           uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_egress<kLopDot>(ctx, "wire_vclock_ops_egress", ops, N, actors, A, frame_off, bytes, cap, total, status);
}

int crdt_pncounter_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                              uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_egress<kLopPn>(ctx, "wire_pncounter_ops_egress", ops, N, actors, A, frame_off, bytes, cap, total, status);
}

int crdt_gset_ops_egress(crdt_ctx *ctx, const crdt_dot_ops *ops, size_t N, const uint64_t *elems, size_t U,
                         uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return dot_ops_egress<kLopGset>(ctx, "wire_gset_ops_egress", ops, N, elems, U, frame_off, bytes, cap, total, status);
}

int crdt_lwwreg_ops_egress(crdt_ctx *ctx, const crdt_lwwreg_ops *ops, size_t N, uint64_t *frame_off, uint8_t *bytes,
                           size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off) return fail(ctx, CRDT_EINVAL, "lwwreg_ops_egress: need ops (op_off)");
  if (ops->n_ops && (!ops->marker || !ops->val)) return fail(ctx, CRDT_EINVAL, "lwwreg_ops_egress: NULL op arrays");
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "lwwreg_ops_egress: need frame_off, total and status");
  LopsEgressPlan p{};
  p.N = N;
  p.n_ops = ops->n_ops;
  p.op_off = (const u64 *)ops->op_off;
  p.marker = (const u64 *)ops->marker;
  p.val = (const u64 *)ops->val;
  p.status = status;
  return lops_egress<kLopLww>(ctx, "wire_lwwreg_ops_egress", p, frame_off, bytes, cap, total);
}

}  // extern "C"
