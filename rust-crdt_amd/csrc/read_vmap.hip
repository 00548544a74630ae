// Batched ReadCtx queries on the value-typed Maps (Map<K, GCounter / PNCounter>, Map<K, Orswot<M>>,
// Map<K, Map<K2, MVReg>>): Map::get (map.rs:251-262) with the gotten value's own read —
// GCounter / PNCounter::read (gcounter.rs:70-72, pncounter.rs:110-114), Orswot::read / contains
// (orswot.rs:253-279), the inner Map's len / keys / get — as gathers of one wave per query under
// a grid-stride loop, like crdt_map_get (read.hip).
//
// The clock rows of a query (A words each) are copied a word per lane.  The new ground is the
// per-query presence scan of the gotten value: M member rows (K2 inner entry clocks) of A words
// become a bitmap.  A row gets a segment of LR = 2^lr_log lanes (the power of two >= its pieces,
// at most 64), one lane per 16-byte piece when A is even and the array 16-byte aligned (8-byte
// words otherwise), so a wave-load covers 64 / LR rows.  The first piece of kScanU row groups is
// loaded by plain predicated loads before any of them is used, so kScanU wave-loads are in flight
// before the first vote; only a row longer than its segment (more than 64 pieces: A > 128 on the
// 16-byte path, A > 64 on the 8-byte path) reads its remaining pieces in a loop of dependent loads.
// A group's "non-zero" predicates are balloted, lane j < 64 / LR tests the LR bits of row j, and a
// second ballot gives the 64 / LR presence bits of the word.
#include "common.hpp"
#include "read_common.hpp"

namespace crdt {

constexpr int kScanU = 4;  // row groups whose first piece is loaded before the first vote

template <int VEC>
struct RowPiece;
template <>
struct RowPiece<1> {
  using T = u64;
  static __device__ __forceinline__ bool nz(T v) { return v != 0; }
  static __device__ __forceinline__ T join(T a, T b) { return crdt::join<Op::Or>(a, b); }
};
template <>
struct RowPiece<2> {
  using T = u64x2;
  static __device__ __forceinline__ bool nz(T v) { return (v.x | v.y) != 0; }
  static __device__ __forceinline__ T join(T a, T b) { return join2<Op::Or>(a, b); }
};

// bits[0..Rw) = the presence bitmap of the R packed rows of A words at `rows` (NULL: none present),
// bits past R zero; returns the number of present rows.  Every loop bound is wave-uniform.
template <int VEC>
__device__ __forceinline__ unsigned scan_rows(const u64 *rows, unsigned long long R, unsigned long long Rw,
                                              unsigned long long A, int lr_log, int lane, u64 *bits) {
  using PT = RowPiece<VEC>;
  using T = typename PT::T;
  const int LR = 1 << lr_log, RW = kWave >> lr_log;
  const int gl = lane & (LR - 1), gr = lane >> lr_log;
  const unsigned long long P = A / VEC;
  const u64 rowmask = LR == kWave ? ~0ull : ((1ull << LR) - 1);
  const int myshift = (lane & (RW - 1)) << lr_log;
  unsigned n = 0;
  for (unsigned long long w = 0; w < Rw; ++w) {
    u64 word = 0;
    const unsigned long long row0 = w * kWave;
    if (rows) {
      // the word's 64 rows are LR groups of RW rows
      for (int g0 = 0; g0 < LR && row0 + (unsigned long long)g0 * RW < R; g0 += kScanU) {
        // the first piece of kScanU row groups: plain predicated loads, none used before all are issued
        T v[kScanU];
        const T *src[kScanU];
        bool on[kScanU];
#pragma unroll
        for (int u = 0; u < kScanU; ++u) {
          const unsigned long long row = row0 + (unsigned long long)(g0 + u) * RW + gr;
          on[u] = g0 + u < LR && row < R;
          src[u] = reinterpret_cast<const T *>(rows + (on[u] ? row : 0) * A);
          T x = {};
          if (on[u] && (unsigned long long)gl < P) x = src[u][gl];
          v[u] = x;
        }
        // a row longer than its segment (more than 64 pieces): the rest of it
        if (P > (unsigned long long)LR) {
#pragma unroll
          for (int u = 0; u < kScanU; ++u)
            if (on[u])
              for (unsigned long long piece = gl + LR; piece < P; piece += LR) v[u] = PT::join(v[u], src[u][piece]);
        }
#pragma unroll
        for (int u = 0; u < kScanU; ++u) {
          const u64 b = __ballot(PT::nz(v[u]));
          const u64 present = __ballot(lane < RW && ((b >> myshift) & rowmask) != 0);
          if (g0 + u < LR) word |= present << ((g0 + u) * RW);
        }
      }
    }
    if (lane == 0) bits[w] = word;
    n += (unsigned)__popcll(word);
  }
  return n;
}

// ---- Map<K, GCounter / PNCounter> ---------------------------------------------------------------
struct CounterGetPlan {
  crdt_map_counter_states st;
  unsigned long long Q;
  const unsigned *state_idx, *key;
  uint8_t *present;
  u64 *rm_clock, *val, *total;
  unsigned *status;
};

// the 128-bit sum of a row's A counters (NULL: 0), wave-uniform; copies the row to dst when given
__device__ __forceinline__ void sum_row(const u64 *src, u64 *dst, unsigned long long A, int lane, u64 &lo, u64 &hi) {
  u64 l = 0, h = 0;
  for (unsigned long long a = lane; a < A; a += kWave) {
    const u64 v = src ? src[a] : 0;
    if (dst) dst[a] = v;
    l += v;
    h += l < v;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const u64 ol = __shfl_xor(l, o, kWave), oh = __shfl_xor(h, o, kWave);
    l += ol;
    h += oh + (l < ol);
  }
  lo = l;
  hi = h;
}

__global__ __launch_bounds__(kBlock) void map_counter_get_kernel(CounterGetPlan p) {
  const unsigned long long A = p.st.A, W = p.st.W, K = p.st.K;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q];
    const bool ok = s < p.st.N && k < K;
    const bool present =
        copy_row(p.rm_clock + q * A, ok ? (const u64 *)p.st.ec + s * p.st.ec_stride + k * A : nullptr, A, lane);
    // an absent key reads as V::default(): zero rows, total 0 (Map::get -> val None, map.rs:251-262)
    if (p.val || p.total) {
      const u64 *rows = present ? (const u64 *)p.st.val + s * p.st.val_stride + k * W * A : nullptr;
      u64 lo, hi;
      sum_row(rows, p.val ? p.val + q * W * A : nullptr, A, lane, lo, hi);
      if (W == 2) {  // P - N, two's complement (pncounter.rs:110-114)
        u64 nl, nh;
        sum_row(rows ? rows + A : nullptr, p.val ? p.val + (q * W + 1) * A : nullptr, A, lane, nl, nh);
        hi = hi - nh - (lo < nl);
        lo = lo - nl;
      }
      if (lane == 0 && p.total) {
        p.total[2 * q] = lo;
        p.total[2 * q + 1] = hi;
      }
    }
    if (lane == 0) {
      p.present[q] = present ? 1 : 0;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

// ---- Map<K, Orswot<M>> --------------------------------------------------------------------------
struct OrswotGetPlan {
  crdt_map_orswot_states st;
  unsigned long long Q, Mw;
  const unsigned *state_idx, *key, *member;
  uint8_t *present;  // get: the key's presence; contains: the member's (val)
  u64 *add_clock, *rm_clock, *val_clock, *members;
  unsigned *len, *vd_n, *status;
  int lr_log;
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void map_orswot_get_kernel(OrswotGetPlan p) {
  const unsigned long long A = p.st.A, K = p.st.K, M = p.st.M;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q];
    const bool ok = s < p.st.N && k < K;
    const unsigned long long sk = ok ? s * K + k : 0;
    const bool present = copy_row(p.rm_clock + q * A, ok ? (const u64 *)p.st.ec + sk * A : nullptr, A, lane);
    // an absent key has no set (val None): the default Orswot's read
    copy_row(p.val_clock + q * A, present ? (const u64 *)p.st.oc + sk * A : nullptr, A, lane);
    const unsigned n = scan_rows<VEC>(present ? (const u64 *)p.st.ent + sk * M * A : nullptr, M, p.Mw, A, p.lr_log,
                                      lane, p.members + q * p.Mw);
    if (lane == 0) {
      p.present[q] = present ? 1 : 0;
      p.len[q] = n;
      if (p.vd_n) p.vd_n[q] = present ? p.st.vd_n[sk] : 0u;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void map_orswot_contains_kernel(OrswotGetPlan p) {
  const unsigned long long A = p.st.A, K = p.st.K, M = p.st.M;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q], m = p.member[q];
    const bool ok = s < p.st.N && k < K && m < M;
    const unsigned long long sk = ok ? s * K + k : 0;
    // under an absent key: Orswot::default().contains (orswot.rs:253-262), everything zero
    const bool has = ok && row_nonzero((const u64 *)p.st.ec + sk * A, A, lane);
    copy_row(p.add_clock + q * A, has ? (const u64 *)p.st.oc + sk * A : nullptr, A, lane);
    const bool val = copy_row(p.rm_clock + q * A, has ? (const u64 *)p.st.ent + (sk * M + m) * A : nullptr, A, lane);
    if (lane == 0) {
      p.present[q] = val ? 1 : 0;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

// ---- Map<K, Map<K2, MVReg>> ---------------------------------------------------------------------
struct NestedGetPlan {
  crdt_map_nested_states st;  // Vs resolved (never 0)
  unsigned long long Q, K2w;
  const unsigned *state_idx, *key, *ikey;
  uint8_t *present;
  u64 *add_clock, *rm_clock, *val_clock, *ikeys, *vclk, *vval;
  unsigned *len, *nval, *status;
  int lr_log;
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void map_nested_get_kernel(NestedGetPlan p) {
  const unsigned long long A = p.st.A, K = p.st.K, K2 = p.st.K2;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q];
    const bool ok = s < p.st.N && k < K;
    const unsigned long long sk = ok ? s * K + k : 0;
    const bool present = copy_row(p.rm_clock + q * A, ok ? (const u64 *)p.st.ec + sk * A : nullptr, A, lane);
    copy_row(p.val_clock + q * A, present ? (const u64 *)p.st.ic + sk * A : nullptr, A, lane);
    const unsigned n = scan_rows<VEC>(present ? (const u64 *)p.st.iec + sk * K2 * A : nullptr, K2, p.K2w, A, p.lr_log,
                                      lane, p.ikeys + q * p.K2w);
    if (lane == 0) {
      p.present[q] = present ? 1 : 0;
      p.len[q] = n;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void map_nested_get_inner_kernel(NestedGetPlan p) {
  const unsigned long long A = p.st.A, K = p.st.K, K2 = p.st.K2, Vs = p.st.Vs;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q], j = p.ikey[q];
    const bool ok = s < p.st.N && k < K && j < K2;
    const unsigned long long sk = ok ? s * K + k : 0, skj = sk * K2 + (ok ? j : 0);
    // under an absent outer key: the default inner Map's get, everything zero
    const bool has = ok && row_nonzero((const u64 *)p.st.ec + sk * A, A, lane);
    copy_row(p.add_clock + q * A, has ? (const u64 *)p.st.ic + sk * A : nullptr, A, lane);
    const bool present = copy_row(p.rm_clock + q * A, has ? (const u64 *)p.st.iec + skj * A : nullptr, A, lane);
    // the register: its first nval slots, already in Vec order (an absent inner key has none)
    unsigned long long n = present ? p.st.nval[skj] : 0;
    n = n < Vs ? n : Vs;
    const u64 *vc = (const u64 *)p.st.ivc + skj * Vs * A;
    u64 *oc = p.vclk + q * Vs * A;
    for (unsigned long long a = lane; a < A; a += kWave) {
      u64 mx = 0;
      for (unsigned long long d = 0; d < Vs; ++d) {
        const u64 v = d < n ? vc[d * A + a] : 0;
        oc[d * A + a] = v;
        mx = v > mx ? v : mx;
      }
      p.val_clock[q * A + a] = mx;
    }
    for (unsigned long long d = lane; d < Vs; d += kWave)
      p.vval[q * Vs + d] = d < n ? ((const u64 *)p.st.ivv)[skj * Vs + d] : 0;
    if (lane == 0) {
      p.present[q] = present ? 1 : 0;
      p.nval[q] = (unsigned)n;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lanes per row of the scan: the power of two >= its pieces, at most a wave
static int scan_lr_log(unsigned long long pieces) {
  int lg = 0;
  while (lg < 6 && (1ull << lg) < pieces) ++lg;
  return lg;
}

constexpr size_t kReadMaxA = 512;  // the apply calls' limit for all three types
constexpr size_t kReadMaxM = 1024, kReadMaxK2 = 256, kReadMaxVs = 64;

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_map_counter_get(crdt_ctx *ctx, const crdt_map_counter_states *states, const uint32_t *state_idx,
                                    const uint32_t *key, size_t Q, uint8_t *present, uint64_t *rm_clock,
                                    uint64_t *val, uint64_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_counter_get: NULL states");
  if (Q == 0) return CRDT_OK;
  const crdt_map_counter_states &s = *states;
  if (s.W != 1 && s.W != 2) return fail(ctx, CRDT_EINVAL, "map_counter_get: W = %zu (1 GCounter, 2 PNCounter)", s.W);
  if (s.A > kReadMaxA) return fail(ctx, CRDT_EUNSUPPORTED, "map_counter_get: A = %zu (at most %zu actors)", s.A, kReadMaxA);
  if (!state_idx || !key || !present || !status || (s.A > 0 && !rm_clock))
    return fail(ctx, CRDT_EINVAL, "map_counter_get: NULL output or query buffer");
  if (s.N > 0 && s.K > 0 && s.A > 0 && (!s.ec || !s.val))
    return fail(ctx, CRDT_EINVAL, "map_counter_get: NULL state buffer");
  if (s.N > 1 && (s.ec_stride < s.K * s.A || s.val_stride < s.K * s.W * s.A))
    return fail(ctx, CRDT_EINVAL, "map_counter_get: state stride too small");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  CounterGetPlan p{s, Q, state_idx, key, present, (u64 *)rm_clock, (u64 *)val, (u64 *)total, status};
  hipLaunchKernelGGL(map_counter_get_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

static int orswot_limits(crdt_ctx *ctx, const char *what, const crdt_map_orswot_states &s) {
  if (s.A > kReadMaxA) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu (at most %zu actors)", what, s.A, kReadMaxA);
  if (s.M > kReadMaxM) return fail(ctx, CRDT_EUNSUPPORTED, "%s: M = %zu (at most %zu members)", what, s.M, kReadMaxM);
  if (s.N > 0 && s.K > 0 && s.A > 0 && (!s.ec || !s.oc || (s.M > 0 && !s.ent)))
    return fail(ctx, CRDT_EINVAL, "%s: NULL state buffer", what);
  return CRDT_OK;
}

extern "C" int crdt_map_orswot_get(crdt_ctx *ctx, const crdt_map_orswot_states *states, const uint32_t *state_idx,
                                   const uint32_t *key, size_t Q, uint8_t *present, uint64_t *rm_clock,
                                   uint64_t *val_clock, uint64_t *members, uint32_t *len, uint32_t *vd_n,
                                   uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_orswot_get: NULL states");
  if (Q == 0) return CRDT_OK;
  const crdt_map_orswot_states &s = *states;
  int rc = orswot_limits(ctx, "map_orswot_get", s);
  if (rc != CRDT_OK) return rc;
  const size_t Mw = (s.M + 63) / 64;
  if (!state_idx || !key || !present || !len || !status || (s.A > 0 && (!rm_clock || !val_clock)) ||
      (Mw > 0 && !members) || (vd_n && s.N > 0 && s.K > 0 && !s.vd_n))
    return fail(ctx, CRDT_EINVAL, "map_orswot_get: NULL output, query or state buffer");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  OrswotGetPlan p{s,       Q,   Mw,   state_idx, key, nullptr, present, nullptr, (u64 *)rm_clock, (u64 *)val_clock,
                  (u64 *)members, len, vd_n, status, 0};
  // 16-byte pieces only when every member row starts 16-byte aligned and is a whole number of them
  const bool vec2 = s.A % 2 == 0 && al16(s.ent);
  p.lr_log = scan_lr_log(vec2 ? s.A / 2 : s.A);
  if (vec2)
    hipLaunchKernelGGL(map_orswot_get_kernel<2>, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL(map_orswot_get_kernel<1>, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

extern "C" int crdt_map_orswot_contains(crdt_ctx *ctx, const crdt_map_orswot_states *states,
                                        const uint32_t *state_idx, const uint32_t *key, const uint32_t *member,
                                        size_t Q, uint8_t *val, uint64_t *add_clock, uint64_t *rm_clock,
                                        uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_orswot_contains: NULL states");
  if (Q == 0) return CRDT_OK;
  const crdt_map_orswot_states &s = *states;
  int rc = orswot_limits(ctx, "map_orswot_contains", s);
  if (rc != CRDT_OK) return rc;
  if (!state_idx || !key || !member || !val || !status || (s.A > 0 && (!add_clock || !rm_clock)))
    return fail(ctx, CRDT_EINVAL, "map_orswot_contains: NULL output or query buffer");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  OrswotGetPlan p{s,       Q,       0,       state_idx, key, member, val, (u64 *)add_clock, (u64 *)rm_clock, nullptr,
                  nullptr, nullptr, nullptr, status,    0};
  hipLaunchKernelGGL(map_orswot_contains_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

static int nested_limits(crdt_ctx *ctx, const char *what, crdt_map_nested_states &s, bool regs) {
  if (s.Vs == 0) s.Vs = 8;  // the apply calls' default
  if (s.A > kReadMaxA) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu (at most %zu actors)", what, s.A, kReadMaxA);
  if (s.K2 > kReadMaxK2)
    return fail(ctx, CRDT_EUNSUPPORTED, "%s: K2 = %zu (at most %zu inner keys)", what, s.K2, kReadMaxK2);
  if (s.Vs > kReadMaxVs) return fail(ctx, CRDT_EUNSUPPORTED, "%s: Vs = %zu (at most %zu slots)", what, s.Vs, kReadMaxVs);
  if (s.N > 0 && s.K > 0 && s.A > 0 && (!s.ec || !s.ic || (s.K2 > 0 && !s.iec)))
    return fail(ctx, CRDT_EINVAL, "%s: NULL state buffer", what);
  if (regs && s.N > 0 && s.K > 0 && s.K2 > 0 && (!s.nval || !s.ivv || (s.A > 0 && !s.ivc)))
    return fail(ctx, CRDT_EINVAL, "%s: NULL register buffer", what);
  return CRDT_OK;
}

extern "C" int crdt_map_nested_get(crdt_ctx *ctx, const crdt_map_nested_states *states, const uint32_t *state_idx,
                                   const uint32_t *key, size_t Q, uint8_t *present, uint64_t *rm_clock,
                                   uint64_t *val_clock, uint64_t *ikeys, uint32_t *len, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_nested_get: NULL states");
  if (Q == 0) return CRDT_OK;
  crdt_map_nested_states s = *states;
  int rc = nested_limits(ctx, "map_nested_get", s, false);
  if (rc != CRDT_OK) return rc;
  const size_t K2w = (s.K2 + 63) / 64;
  if (!state_idx || !key || !present || !len || !status || (s.A > 0 && (!rm_clock || !val_clock)) ||
      (K2w > 0 && !ikeys))
    return fail(ctx, CRDT_EINVAL, "map_nested_get: NULL output or query buffer");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  NestedGetPlan p{s,       Q,   K2w,     state_idx, key, nullptr, present, nullptr, (u64 *)rm_clock, (u64 *)val_clock,
                  (u64 *)ikeys, nullptr, nullptr, len, nullptr, status, 0};
  const bool vec2 = s.A % 2 == 0 && al16(s.iec);
  p.lr_log = scan_lr_log(vec2 ? s.A / 2 : s.A);
  if (vec2)
    hipLaunchKernelGGL(map_nested_get_kernel<2>, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL(map_nested_get_kernel<1>, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

extern "C" int crdt_map_nested_get_inner(crdt_ctx *ctx, const crdt_map_nested_states *states,
                                         const uint32_t *state_idx, const uint32_t *key, const uint32_t *ikey,
                                         size_t Q, uint8_t *present, uint64_t *add_clock, uint64_t *rm_clock,
                                         uint64_t *vclk, uint64_t *vval, uint32_t *nval, uint64_t *val_clock,
                                         uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_nested_get_inner: NULL states");
  if (Q == 0) return CRDT_OK;
  crdt_map_nested_states s = *states;
  int rc = nested_limits(ctx, "map_nested_get_inner", s, true);
  if (rc != CRDT_OK) return rc;
  if (!state_idx || !key || !ikey || !present || !nval || !vval || !status ||
      (s.A > 0 && (!add_clock || !rm_clock || !vclk || !val_clock)))
    return fail(ctx, CRDT_EINVAL, "map_nested_get_inner: NULL output or query buffer");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  NestedGetPlan p{s,       Q,           0,           state_idx, key,  ikey,   present, (u64 *)add_clock, (u64 *)rm_clock,
                  (u64 *)val_clock, nullptr, (u64 *)vclk, (u64 *)vval, nullptr, nval, status, 0};
  hipLaunchKernelGGL(map_nested_get_inner_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}
