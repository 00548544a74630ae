// Batched reads (the reference's ReadCtx queries, ctx.rs:8-55):
//   Orswot::contains / read (orswot.rs:253-279), MVReg::read (mvreg.rs:183-215),
//   Map::is_empty / len / get / read_ctx (map.rs:233-307), ReadCtx::derive_add_ctx (ctx.rs:40-48).
// The presence scan (a member / key is present <=> its dot-clock row is non-zero) is a read-only
// stream over the whole entry array; the gathers touch a few rows per query.
#include "common.hpp"
#include "read_common.hpp"

namespace crdt {

// ---- presence scan ------------------------------------------------------------------------
// One wave produces one output word: 64 rows of one state.  A row is P pieces (16-byte pieces on
// the aligned path, 8-byte words otherwise); LR = 2^lr_log lanes (the power of two >= P, at most
// 64) share a row, so one wave-load covers 64 / LR rows (A = 64 on the 16-byte path: 2 rows, 1 KiB)
// and a row longer than 64 pieces takes ceil(P / 64) of them.  U loads are issued before the first
// is tested.  Per load, the lanes' "non-zero" predicates are balloted, lane j < 64 / LR tests the
// LR bits of row j in the ballot, and a second ballot yields the 64 / LR presence bits.
struct ScanPlan {
  const u64 *in;
  unsigned long long N, R, Rw, A, rstride, sstride;
  u64 *bits;  // [N][Rw]
  int lr_log;
};

template <int VEC>
struct ScanPiece;
template <>
struct ScanPiece<1> {
  using T = u64;
  static __device__ __forceinline__ bool nz(T v) { return v != 0; }
};
template <>
struct ScanPiece<2> {
  using T = u64x2;
  static __device__ __forceinline__ bool nz(T v) { return (v.x | v.y) != 0; }
};

template <int VEC, int U, bool NT>
__global__ __launch_bounds__(kBlock) void presence_scan_kernel(ScanPlan p) {
  using T = typename ScanPiece<VEC>::T;
  const int lane = threadIdx.x % kWave;
  const int LR = 1 << p.lr_log;
  const int RW = kWave >> p.lr_log;              // rows per wave-load
  const int gl = lane & (LR - 1), gr = lane >> p.lr_log;
  const unsigned long long P = p.A / VEC;         // pieces per row
  const unsigned CC = (unsigned)((P + LR - 1) >> p.lr_log);  // wave-loads per row group
  const unsigned steps = (unsigned)LR * CC;      // 64 / RW row groups of CC loads each
  const u64 rowmask = LR == 64 ? ~0ull : ((1ull << LR) - 1);
  const unsigned long long words = p.N * p.Rw;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nw = (unsigned long long)gridDim.x * (kBlock / kWave);
  for (unsigned long long w = w0; w < words; w += nw) {
    const unsigned long long s = w / p.Rw, rw = w - s * p.Rw;
    const u64 *base = p.in + s * p.sstride;
    const unsigned long long row0 = rw * kWave;
    u64 word = 0;
    // step t = (row group rg, column chunk c), advanced without a division: lrg / lc for the
    // loads, trg / tc for the tests behind them
    unsigned lrg = 0, lc = 0, trg = 0, tc = 0;
    auto load = [&](T(&v)[U], unsigned t0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned long long row = row0 + (unsigned long long)lrg * RW + gr;
        const unsigned long long piece = ((unsigned long long)lc << p.lr_log) + gl;
        T x = {};
        if (t0 + u < steps && row < p.R && piece < P) {
          const T *q = reinterpret_cast<const T *>(base + row * p.rstride) + piece;
          if constexpr (NT) x = __builtin_nontemporal_load(q);
          else x = *q;
        }
        v[u] = x;
        if (++lc == CC) lc = 0, ++lrg;
      }
    };
    auto test = [&](const T(&v)[U], unsigned t0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u64 b = __ballot(ScanPiece<VEC>::nz(v[u]));
        const u64 rows = __ballot(lane < RW && ((b >> (lane << p.lr_log)) & rowmask) != 0);
        if (t0 + u < steps) word |= rows << (trg * RW);
        if (++tc == CC) tc = 0, ++trg;
      }
    };
    for (unsigned t0 = 0; t0 < steps; t0 += U) {
      T v[U];
      load(v, t0);
      test(v, t0);
    }
    if (lane == 0) p.bits[w] = word;
  }
}

// len[s] = popcount of state s's Rw words; one wave per state.
__global__ __launch_bounds__(kBlock) void presence_count_kernel(const u64 *bits, unsigned long long N,
                                                                unsigned long long Rw, unsigned *len) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nw = (unsigned long long)gridDim.x * (kBlock / kWave);
  for (unsigned long long s = w0; s < N; s += nw) {
    unsigned n = 0;
    for (unsigned long long i = lane; i < Rw; i += kWave) n += (unsigned)__popcll(bits[s * Rw + i]);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
    if (lane == 0) len[s] = n;
  }
}

static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int VEC>
static void launch_scan(crdt_ctx *ctx, const ScanPlan &p, unsigned grid) {
  const bool u8 = ctx->tune.read_unroll >= 8, nt = ctx->tune.read_nt != 0;
#define CRDT_SCAN_LAUNCH(UU, NN) \
  hipLaunchKernelGGL((presence_scan_kernel<VEC, UU, NN>), dim3(grid), dim3(kBlock), 0, ctx->stream, p)
  if (u8 && nt) CRDT_SCAN_LAUNCH(8, true);
  else if (u8) CRDT_SCAN_LAUNCH(8, false);
  else if (nt) CRDT_SCAN_LAUNCH(4, true);
  else CRDT_SCAN_LAUNCH(4, false);
#undef CRDT_SCAN_LAUNCH
}

// bits[N][ceil(R/64)] and len[N] (may be NULL) of N states of R rows of A words.
static int presence_scan(crdt_ctx *ctx, const char *what, const uint64_t *in, size_t rstride, size_t sstride, size_t N,
                         size_t R, size_t A, uint64_t *bits, uint32_t *len) {
  CRDT_CHECK_CTX(ctx);
  if (N == 0) return CRDT_OK;
  const size_t Rw = (R + 63) / 64;
  if ((Rw > 0 && !bits) || (R > 0 && A > 0 && !in)) return fail(ctx, CRDT_EINVAL, "%s: NULL buffer", what);
  if (R > 0 && A > 0) {
    if (R > 1 && rstride < A) return fail(ctx, CRDT_EINVAL, "%s: row stride < A", what);
    if (N > 1 && sstride < (R - 1) * rstride + A) return fail(ctx, CRDT_EINVAL, "%s: state stride too small", what);
  }
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  if (R == 0 || A == 0) {  // nothing can be present
    if (Rw > 0) {
      int rc = device_fill(ctx, bits, N * Rw * sizeof(uint64_t), 0);
      if (rc != CRDT_OK) return rc;
    }
    if (len) return device_fill(ctx, len, N * sizeof(uint32_t), 0);
    return CRDT_OK;
  }
  ScanPlan p{(const u64 *)in, N, R, Rw, A, rstride, sstride, (u64 *)bits, 0};
  // 16-byte pieces only when every row starts 16-byte aligned and is a whole number of them
  const bool vec2 = A % 2 == 0 && al16(in) && (R == 1 || rstride % 2 == 0) && (N == 1 || sstride % 2 == 0);
  const unsigned long long P = vec2 ? A / 2 : A;
  while (p.lr_log < 6 && (1ull << p.lr_log) < P) ++p.lr_log;
  const unsigned long long words = (unsigned long long)N * Rw;
  const unsigned long long want = (words + kBlock / kWave - 1) / (kBlock / kWave);
  const unsigned long long cap =
      ctx->tune.read_bpc > 0 ? (unsigned long long)ctx->cu_count * ctx->tune.read_bpc : 0x7fffffffull;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  timing_begin(ctx, "read_scan");
  if (vec2) launch_scan<2>(ctx, p, grid);
  else launch_scan<1>(ctx, p, grid);
  if (len) {
    const unsigned long long cw = (N + kBlock / kWave - 1) / (kBlock / kWave);
    const unsigned long long ccap = (unsigned long long)ctx->cu_count * 8;
    hipLaunchKernelGGL(presence_count_kernel, dim3((unsigned)(cw < ccap ? cw : ccap)), dim3(kBlock), 0, ctx->stream,
                       (const u64 *)bits, (unsigned long long)N, (unsigned long long)Rw, len);
  }
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

// ---- gathers: one wave per query / register (QUERY_WAVE_LOOP, query_grid, copy_row and
// row_nonzero: read_common.hpp) ---------------------------------------------------------------
struct ContainsPlan {
  const u64 *entries;
  unsigned long long mstride, sstride, N, M, A, Q;
  const unsigned *state_idx, *member;
  uint8_t *val;
  u64 *rm_clock;
  unsigned long long rm_stride;
  unsigned *status;
};

__global__ __launch_bounds__(kBlock) void contains_kernel(ContainsPlan p) {
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], m = p.member[q];
    const bool ok = s < p.N && m < p.M;
    const bool present = copy_row(p.rm_clock + q * p.rm_stride, ok ? p.entries + s * p.sstride + m * p.mstride : nullptr,
                                  p.A, lane);
    if (lane == 0) {
      p.val[q] = present ? 1 : 0;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

// One MVReg (V slots at vclk / vval, or absent: vclk == NULL) read into: the join of its slot
// clocks (clock), its values compacted in Vec order (out_val[V], and out_clk[V][A] when given),
// the count.  V <= 64.
__device__ __forceinline__ unsigned read_register(const u64 *vclk, const u64 *vval, unsigned long long V,
                                                  unsigned long long A, u64 *clock, u64 *out_clk, u64 *out_val,
                                                  int lane) {
  u64 used = 0;
  if (vclk)
    for (unsigned long long j = 0; j < V; ++j)
      if (row_nonzero(vclk + j * A, A, lane)) used |= 1ull << j;
  const unsigned n = (unsigned)__popcll(used);
  for (unsigned long long a = lane; a < A; a += kWave) {
    u64 mx = 0;
    unsigned d = 0;
    for (unsigned long long j = 0; j < V; ++j) {
      if (!((used >> j) & 1)) continue;
      const u64 v = vclk[j * A + a];
      mx = v > mx ? v : mx;
      if (out_clk) out_clk[d * A + a] = v;
      ++d;
    }
    if (out_clk)
      for (; d < V; ++d) out_clk[d * A + a] = 0;
    clock[a] = mx;
  }
  if (out_val)
    for (unsigned long long j = lane; j < V; j += kWave) {
      // slot j of the output = the j-th used input slot
      u64 rest = used;
      for (unsigned long long i = 0; i < j && rest; ++i) rest &= rest - 1;
      out_val[j] = (j < n) ? vval[__ffsll((long long)rest) - 1] : 0;
    }
  return n;
}

struct MVReadPlan {
  const u64 *vclk, *vval;
  unsigned long long vclk_stride, vval_stride, N, A, V;
  u64 *clock;
  unsigned long long clock_stride;
  u64 *vals;
  unsigned *nval;
};

__global__ __launch_bounds__(kBlock) void mvreg_read_kernel(MVReadPlan p) {
  QUERY_WAVE_LOOP(p.N) {
    const unsigned n = read_register(p.vclk + q * p.vclk_stride, p.vval + q * p.vval_stride, p.V, p.A,
                                     p.clock + q * p.clock_stride, nullptr, p.vals ? p.vals + q * p.V : nullptr, lane);
    if (lane == 0 && p.nval) p.nval[q] = n;
  }
}

struct MapGetPlan {
  crdt_map_states st;
  unsigned long long Q;
  const unsigned *state_idx, *key;
  uint8_t *present;
  u64 *rm_clock, *vclk, *vval;
  unsigned *nval;
  u64 *val_clock;
  unsigned *status;
};

__global__ __launch_bounds__(kBlock) void map_get_kernel(MapGetPlan p) {
  const unsigned long long A = p.st.A, V = p.st.V;
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long s = p.state_idx[q], k = p.key[q];
    const bool ok = s < p.st.N && k < p.st.K;
    const bool present =
        copy_row(p.rm_clock + q * A, ok ? (const u64 *)p.st.ec + s * p.st.ec_stride + k * A : nullptr, A, lane);
    // an absent key has no register (Map::get -> val None, map.rs:251-262)
    const u64 *vc = present ? (const u64 *)p.st.vclk + s * p.st.vclk_stride + k * V * A : nullptr;
    const u64 *vv = present ? (const u64 *)p.st.vval + s * p.st.vval_stride + k * V : nullptr;
    const unsigned n = read_register(vc, vv, V, A, p.val_clock + q * A, p.vclk + q * V * A, p.vval + q * V, lane);
    if (lane == 0) {
      p.present[q] = present ? 1 : 0;
      p.nval[q] = n;
      p.status[q] = ok ? 0u : 2u;
    }
  }
}

struct DerivePlan {
  const u64 *clock;
  unsigned long long clock_stride, Q, A;
  const unsigned *actor;
  u64 *out;
  unsigned long long out_stride;
  u64 *counter;
  unsigned *status;
};

// out may be the same rows as clock: every word is read by the lane that then writes it, and the
// actor's word is read before any store of the row.
__global__ __launch_bounds__(kBlock) void derive_add_kernel(DerivePlan p) {
  QUERY_WAVE_LOOP(p.Q) {
    const unsigned long long a = p.actor[q];
    const u64 *row = p.clock + q * p.clock_stride;
    u64 *dst = p.out + q * p.out_stride;
    unsigned st = 0;
    u64 next = 0;
    if (a >= p.A) {
      st = 2u;
    } else {
      const u64 c = row[a];
      if (c == ~0ull) st = 4u;
      else next = c + 1;
    }
    for (unsigned long long i = lane; i < p.A; i += kWave) {
      const u64 v = row[i];
      dst[i] = (st == 0 && i == a) ? next : v;
    }
    if (lane == 0) {
      p.counter[q] = next;
      p.status[q] = st;
    }
  }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_orswot_read(crdt_ctx *ctx, const uint64_t *entries, size_t entry_mstride, size_t entry_sstride,
                                size_t N, size_t M, size_t A, uint64_t *members, uint32_t *len) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return presence_scan(ctx, "orswot_read", entries, entry_mstride, entry_sstride, N, M, A, members, len);
}

extern "C" int crdt_map_read(crdt_ctx *ctx, const uint64_t *ec, size_t ec_kstride, size_t ec_sstride, size_t N,
                             size_t K, size_t A, uint64_t *keys, uint32_t *len) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  return presence_scan(ctx, "map_read", ec, ec_kstride, ec_sstride, N, K, A, keys, len);
}

extern "C" int crdt_orswot_contains(crdt_ctx *ctx, const uint64_t *entries, size_t entry_mstride,
                                    size_t entry_sstride, size_t N, size_t M, size_t A, const uint32_t *state_idx,
                                    const uint32_t *member, size_t Q, uint8_t *val, uint64_t *rm_clock,
                                    size_t rm_stride, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (Q == 0) return CRDT_OK;
  if (!state_idx || !member || !val || !status || (A > 0 && !rm_clock) || (N > 0 && M > 0 && A > 0 && !entries))
    return fail(ctx, CRDT_EINVAL, "orswot_contains: NULL buffer");
  if ((M > 1 && entry_mstride < A) || (N > 1 && M > 0 && entry_sstride < (M - 1) * entry_mstride + A) ||
      (Q > 1 && rm_stride < A))
    return fail(ctx, CRDT_EINVAL, "orswot_contains: stride too small");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  ContainsPlan p{(const u64 *)entries, entry_mstride, entry_sstride, N, M, A, Q, state_idx, member, val,
                 (u64 *)rm_clock, rm_stride, status};
  hipLaunchKernelGGL(contains_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

extern "C" int crdt_mvreg_read(crdt_ctx *ctx, const crdt_mvreg_states *regs, uint64_t *clock, size_t clock_stride,
                               uint64_t *vals, uint32_t *nval) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!regs) return fail(ctx, CRDT_EINVAL, "mvreg_read: NULL states");
  if (regs->N == 0) return CRDT_OK;
  if (regs->V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_read: V = %zu (at most 64 slots)", regs->V);
  if ((regs->A > 0 && !clock) || (regs->V > 0 && ((regs->A > 0 && !regs->vclk) || (vals && !regs->vval))))
    return fail(ctx, CRDT_EINVAL, "mvreg_read: NULL buffer");
  if (regs->N > 1 && (clock_stride < regs->A || regs->vclk_stride < regs->V * regs->A || regs->vval_stride < regs->V))
    return fail(ctx, CRDT_EINVAL, "mvreg_read: stride too small");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  MVReadPlan p{(const u64 *)regs->vclk, (const u64 *)regs->vval, regs->vclk_stride, regs->vval_stride, regs->N,
               regs->A, regs->V, (u64 *)clock, clock_stride, (u64 *)vals, nval};
  hipLaunchKernelGGL(mvreg_read_kernel, dim3(query_grid(ctx, regs->N)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

extern "C" int crdt_map_get(crdt_ctx *ctx, const crdt_map_states *states, const uint32_t *state_idx,
                            const uint32_t *key, size_t Q, uint8_t *present, uint64_t *rm_clock, uint64_t *vclk,
                            uint64_t *vval, uint32_t *nval, uint64_t *val_clock, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "map_get: NULL states");
  if (Q == 0) return CRDT_OK;
  const crdt_map_states &s = *states;
  if (s.V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "map_get: V = %zu (at most 64 slots)", s.V);
  if (!state_idx || !key || !present || !nval || !status || (s.A > 0 && (!rm_clock || !val_clock)) ||
      (s.V > 0 && (!vval || (s.A > 0 && !vclk))))
    return fail(ctx, CRDT_EINVAL, "map_get: NULL output or query buffer");
  if (s.N > 0 && s.K > 0 && ((s.A > 0 && !s.ec) || (s.V > 0 && (!s.vval || (s.A > 0 && !s.vclk)))))
    return fail(ctx, CRDT_EINVAL, "map_get: NULL state buffer");
  if (s.N > 1 && (s.ec_stride < s.K * s.A || s.vclk_stride < s.K * s.V * s.A || s.vval_stride < s.K * s.V))
    return fail(ctx, CRDT_EINVAL, "map_get: state stride too small");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  MapGetPlan p{s, Q, state_idx, key, present, (u64 *)rm_clock, (u64 *)vclk, (u64 *)vval, nval, (u64 *)val_clock, status};
  hipLaunchKernelGGL(map_get_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

extern "C" int crdt_vclock_derive_add(crdt_ctx *ctx, const uint64_t *clock, size_t clock_stride, size_t Q, size_t A,
                                      const uint32_t *actor, uint64_t *out_clock, size_t out_stride,
                                      uint64_t *counter, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (Q == 0) return CRDT_OK;
  if (!actor || !counter || !status || (A > 0 && (!clock || !out_clock)))
    return fail(ctx, CRDT_EINVAL, "vclock_derive_add: NULL buffer");
  if (Q > 1 && (clock_stride < A || out_stride < A)) return fail(ctx, CRDT_EINVAL, "vclock_derive_add: stride < A");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  DerivePlan p{(const u64 *)clock, clock_stride, Q, A, actor, (u64 *)out_clock, out_stride, (u64 *)counter, status};
  hipLaunchKernelGGL(derive_add_kernel, dim3(query_grid(ctx, Q)), dim3(kBlock), 0, ctx->stream, p);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}
