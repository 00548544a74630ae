// Batched Causal::forget of MVReg<u64, A> on its own (mvreg.rs:88-104 with VClock::forget):
//   crdt_mvreg_forget_batch  register i forgets the clock y + i*y_stride, in place
// Every value clock keeps v[a] where v[a] > y[a] (unsigned) and becomes 0 elsewhere; a value whose
// clock empties is dropped, the others keep their order.  Result layout as every MVReg result:
// survivors from slot 0 in Vec order, the slots past them zero (clock and value).
//
// The kernel is a stream (V*A words and one y row in, at most V*A words out), so a register gets no
// more lanes than its row has 16-byte pieces: a segment of G = 1..64 lanes per register, 64 / G
// registers per wave, lane g of a segment holding actors 2(g + G*c), +1 of every slot (c < CH; CH = 2
// covers 128 < A <= 256).  All of a register's slots (and its values) are loaded before the first
// vote.  "Slot s survives" is a wave ballot masked to the segment; a survivor's new slot is the
// count of surviving slots below it.  A register the forget leaves bit-identical (nothing forgotten,
// no hole to close, the slots past the values already zero) is not written.
// Rows are read and written in 16-byte pieces when A is even and rows and y are 16-byte aligned
// (VEC), in 8-byte words otherwise.
//
// Past one wave's shapes (A > 256 or V > 8, the split of mvreg.hip) one workgroup of ceil(A / 64)
// waves takes a register, thread t = actor t, every vote a workgroup vote (up to 16 slots held in
// registers; 17..64 slots: mvreg_forget_wide64_kernel, two passes over the thread's own column).
#include "common.hpp"

namespace crdt {

struct MvForgetPlan {
  u64 *vclk, *vval;
  unsigned long long cs, vs, V, N, A;
  const u64 *y;
  unsigned long long ys;
  uint32_t *status;  // may be NULL
};

template <int G, int CH, int VM, bool VEC>
__global__ __launch_bounds__(kBlock) void mvreg_forget_kernel(MvForgetPlan p) {
  constexpr int RPW = kWave / G;  // registers per wave
  const int lane = threadIdx.x % kWave, g = lane % G, seg = lane / G;
  const u64 smask = G == kWave ? ~0ull : ((1ull << G) - 1);
  const int sshift = seg * G;
  const unsigned long long A = p.A, V = p.V;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long ngroup = (p.N + RPW - 1) / RPW;
  for (unsigned long long wv = wave0; wv < ngroup; wv += nwave) {  // wave-uniform
    const unsigned long long i = wv * RPW + seg;
    const bool live = i < p.N;
    u64 *rc = p.vclk + (live ? i : 0) * p.cs, *rv = p.vval + (live ? i : 0) * p.vs;
    const u64 *ry = p.y + (live ? i : 0) * p.ys;
    // this lane's words of a row: actors a0[c], a0[c] + 1
    bool on0[CH], on1[CH];
    unsigned long long a0[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      a0[c] = 2ull * (g + G * c);
      on0[c] = live && a0[c] < A;
      on1[c] = live && a0[c] + 1 < A;
    }
    u64 yv[CH][2], cv[VM][CH][2], vv[VM];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      yv[c][0] = yv[c][1] = 0;
      if (VEC) {
        if (on0[c]) {
          const u64x2 t = *reinterpret_cast<const u64x2 *>(ry + a0[c]);
          yv[c][0] = t.x;
          yv[c][1] = t.y;
        }
      } else {
        if (on0[c]) yv[c][0] = ry[a0[c]];
        if (on1[c]) yv[c][1] = ry[a0[c] + 1];
      }
    }
#pragma unroll
    for (int s = 0; s < VM; ++s) {
      const bool sl = (unsigned long long)s < V;
      vv[s] = (live && sl) ? rv[s] : 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        cv[s][c][0] = cv[s][c][1] = 0;
        if (VEC) {
          if (sl && on0[c]) {
            const u64x2 t = *reinterpret_cast<const u64x2 *>(rc + s * A + a0[c]);
            cv[s][c][0] = t.x;
            cv[s][c][1] = t.y;
          }
        } else {
          if (sl && on0[c]) cv[s][c][0] = rc[s * A + a0[c]];
          if (sl && on1[c]) cv[s][c][1] = rc[s * A + a0[c] + 1];
        }
      }
    }
    // forget, and the votes: which slots survive, did any word change
    bool chg = false;
    unsigned surv = 0;
#pragma unroll
    for (int s = 0; s < VM; ++s) {
      bool nz = false;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u64 o = cv[s][c][h], n = o > yv[c][h] ? o : 0;
          chg |= n != o;
          nz |= n != 0;
          cv[s][c][h] = n;
        }
      if (((__ballot(nz) >> sshift) & smask) != 0) surv |= 1u << s;
    }
    const int n = __builtin_popcount(surv);
    // bit-identical: no word forgotten, the survivors already in slots 0 .. n-1, no value past them
    bool tail = false;
#pragma unroll
    for (int s = 0; s < VM; ++s) tail |= s >= n && vv[s] != 0;
    const bool same = ((__ballot(chg || tail) >> sshift) & smask) == 0 && surv == (1u << n) - 1u;
    if (live && !same) {
#pragma unroll
      for (int s = 0; s < VM; ++s) {
        if (!((surv >> s) & 1u)) continue;
        const unsigned long long d = __builtin_popcount(surv & ((1u << s) - 1u));
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          if (VEC) {
            if (on0[c]) {
              u64x2 t;
              t.x = cv[s][c][0];
              t.y = cv[s][c][1];
              *reinterpret_cast<u64x2 *>(rc + d * A + a0[c]) = t;
            }
          } else {
            if (on0[c]) rc[d * A + a0[c]] = cv[s][c][0];
            if (on1[c]) rc[d * A + a0[c] + 1] = cv[s][c][1];
          }
        }
        if (g == 0) rv[d] = vv[s];
      }
      for (unsigned long long d = n; d < V; ++d) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          if (VEC) {
            if (on0[c]) {
              u64x2 z;
              z.x = z.y = 0;
              *reinterpret_cast<u64x2 *>(rc + d * A + a0[c]) = z;
            }
          } else {
            if (on0[c]) rc[d * A + a0[c]] = 0;
            if (on1[c]) rc[d * A + a0[c] + 1] = 0;
          }
        }
        if (g == 0) rv[d] = 0;
      }
    }
    if (live && g == 0 && p.status) p.status[i] = 0;
  }
}

// One workgroup per register (A > 256 or V > 8): thread t = actor t, up to 16 slots.
__global__ __launch_bounds__(1024) void mvreg_forget_wide_kernel(MvForgetPlan p) {
  constexpr int VM = 16;
  const unsigned t = threadIdx.x;
  const unsigned long long i = blockIdx.x, A = p.A, V = p.V;
  u64 *rc = p.vclk + i * p.cs, *rv = p.vval + i * p.vs;
  const bool on = t < A;
  const u64 yv = on ? p.y[i * p.ys + t] : 0;
  u64 cv[VM], vv[VM];
#pragma unroll
  for (int s = 0; s < VM; ++s) {
    const bool sl = (unsigned long long)s < V;
    cv[s] = (sl && on) ? rc[s * A + t] : 0;
    vv[s] = sl ? rv[s] : 0;
  }
  bool chg = false;
  unsigned surv = 0;
#pragma unroll
  for (int s = 0; s < VM; ++s) {
    const u64 o = cv[s], n = o > yv ? o : 0;
    chg |= n != o;
    cv[s] = n;
    if (__syncthreads_or(n != 0)) surv |= 1u << s;  // (also: every thread's loads are done before any store)
  }
  const int n = __builtin_popcount(surv);
  bool tail = false;
#pragma unroll
  for (int s = 0; s < VM; ++s) tail |= s >= n && vv[s] != 0;
  const bool same = !__syncthreads_or(chg || tail) && surv == (1u << n) - 1u;
  if (!same) {
#pragma unroll
    for (int s = 0; s < VM; ++s) {
      if (!((surv >> s) & 1u)) continue;
      const unsigned long long d = __builtin_popcount(surv & ((1u << s) - 1u));
      if (on) rc[d * A + t] = cv[s];
      if (t == 0) rv[d] = vv[s];
    }
    for (unsigned long long d = n; d < V; ++d) {
      if (on) rc[d * A + t] = 0;
      if (t == 0) rv[d] = 0;
    }
  }
  if (t == 0 && p.status) p.status[i] = 0;
}

// The 64-slot form (16 < V <= 64): thread t = actor t again, but the rows are not held in registers.
// Pass 1 reads the thread's column (eight slots' loads in flight) and votes the surviving slots into one
// u64 mask; pass 2 reads the column again, eight slots at a time, and compacts the survivors in Vec order.  A thread touches only its own actor column
// and the write slot never passes the read slot (d <= s), so the in-place order is safe without a
// barrier between the passes; thread 0 alone moves the values, in the same order.  A word is written
// only where it changes.
__global__ __launch_bounds__(1024) void mvreg_forget_wide64_kernel(MvForgetPlan p) {
  __shared__ u64 red[1024 / kWave];
  const unsigned t = threadIdx.x;
  const unsigned long long i = blockIdx.x, A = p.A, V = p.V;
  u64 *rc = p.vclk + i * p.cs, *rv = p.vval + i * p.vs;
  const bool on = t < A;
  const u64 yv = on ? p.y[i * p.ys + t] : 0;
  u64 had = 0, surv = 0;  // my column: slot non-zero before / after the forget
  constexpr unsigned GR = 8;  // slots whose loads are issued together
  for (unsigned long long s0 = 0; s0 < V; s0 += GR) {
    u64 c[GR];
#pragma unroll
    for (unsigned u = 0; u < GR; ++u) c[u] = (on && s0 + u < V) ? rc[(s0 + u) * A + t] : 0;
#pragma unroll
    for (unsigned u = 0; u < GR; ++u) {
      if (c[u] != 0) had |= 1ull << (s0 + u);
      if (c[u] > yv) surv |= 1ull << (s0 + u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) surv |= __shfl_xor(surv, off, kWave);
  const unsigned nw = blockDim.x / kWave;
  if (nw > 1) {  // (workgroup-uniform)
    if (t % kWave == 0) red[t / kWave] = surv;
    __syncthreads();
    for (unsigned x = 0; x < nw; ++x) surv |= red[x];
  }
  const unsigned long long n = (unsigned long long)__popcll(surv);
  // a group's loads come before its stores, and its stores go to slots at or below the group's own
  for (unsigned long long s0 = 0; s0 < V; s0 += GR) {
    if (!((surv >> s0) & ((1ull << GR) - 1))) continue;
    u64 c[GR];
#pragma unroll
    for (unsigned u = 0; u < GR; ++u) c[u] = (on && s0 + u < V) ? rc[(s0 + u) * A + t] : 0;
    u64 vv[GR];
    if (t == 0) {
#pragma unroll
      for (unsigned u = 0; u < GR; ++u) vv[u] = s0 + u < V ? rv[s0 + u] : 0;
    }
#pragma unroll
    for (unsigned u = 0; u < GR; ++u) {
      const unsigned long long s = s0 + u;
      if (s >= V || !((surv >> s) & 1)) continue;
      const unsigned long long d = (unsigned long long)__popcll(surv & ((1ull << s) - 1));
      const u64 k = c[u] > yv ? c[u] : 0;
      if (on && (d != s || k != c[u])) rc[d * A + t] = k;
      if (t == 0 && d != s) rv[d] = vv[u];
    }
  }
  for (unsigned long long s = n; s < V; ++s) {
    if ((had >> s) & 1) rc[s * A + t] = 0;
    if (t == 0) rv[s] = 0;
  }
  if (t == 0 && p.status) p.status[i] = 0;
}

template <int G, int CH, int VM>
static void launch_forget_vec(const MvForgetPlan &p, bool vec, unsigned grid, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((mvreg_forget_kernel<G, CH, VM, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((mvreg_forget_kernel<G, CH, VM, false>), dim3(grid), dim3(kBlock), 0, s, p);
}
template <int G, int CH>
static void launch_forget_vm(const MvForgetPlan &p, bool vec, unsigned grid, hipStream_t s) {
  if (p.V <= 4) launch_forget_vec<G, CH, 4>(p, vec, grid, s);
  else launch_forget_vec<G, CH, 8>(p, vec, grid, s);
}

// lanes per register: the 16-byte pieces of a row, rounded up to a power of two
static int mv_forget_lanes(size_t A) {
  const size_t pieces = (A + 1) / 2;
  int g = 1;
  while ((size_t)g < pieces && g < kWave) g *= 2;
  return g;
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_mvreg_forget_batch(crdt_ctx *ctx, const crdt_mvreg_states *states, const uint64_t *y, size_t y_stride,
                            uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!states) return fail(ctx, CRDT_EINVAL, "mvreg_forget_batch: NULL states");
  const size_t N = states->N, A = states->A, V = states->V;
  if (N == 0 || A == 0) return CRDT_OK;
  if (V == 0 || V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_forget_batch: V = %zu not in [1, 64]", V);
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_forget_batch: A = %zu > 1024 actors", A);
  if (!states->vclk || !states->vval || !y) return fail(ctx, CRDT_EINVAL, "mvreg_forget_batch: NULL register buffers / y");
  if (N > 1 && (states->vclk_stride < V * A || states->vval_stride < V))
    return fail(ctx, CRDT_EINVAL, "mvreg_forget_batch: strides below the register size");
  if (y_stride != 0 && y_stride < A) return fail(ctx, CRDT_EINVAL, "mvreg_forget_batch: y_stride < A (0 = one clock for all)");
  if (N > 0x7fffffffULL) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_forget_batch: N too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  MvForgetPlan p{};
  p.vclk = (u64 *)states->vclk;
  p.vval = (u64 *)states->vval;
  p.cs = states->vclk_stride;
  p.vs = states->vval_stride;
  p.V = V;
  p.N = N;
  p.A = A;
  p.y = (const u64 *)y;
  p.ys = y_stride;
  p.status = status;
  timing_begin(ctx, "mvreg_forget");
  if (A > 256 || V > 8) {
    const unsigned nt = (unsigned)std::max<size_t>(64, (A + 63) / 64 * 64);
    if (V > 16) hipLaunchKernelGGL(mvreg_forget_wide64_kernel, dim3((unsigned)N), dim3(nt), 0, ctx->stream, p);
    else hipLaunchKernelGGL(mvreg_forget_wide_kernel, dim3((unsigned)N), dim3(nt), 0, ctx->stream, p);
  } else {
    // 16-byte pieces: every row and y row starts on a 16-byte boundary
    const bool vec = A % 2 == 0 && ((uintptr_t)p.vclk % 16 == 0) && (N == 1 || p.cs % 2 == 0) &&
                     ((uintptr_t)p.y % 16 == 0) && p.ys % 2 == 0;
    const int G = mv_forget_lanes(A);
    const unsigned long long waves = (N + (kWave / G) - 1) / (kWave / G);
    const unsigned long long want = (waves + kBlock / kWave - 1) / (kBlock / kWave);
    const unsigned grid = (unsigned)std::min<unsigned long long>(want, (unsigned long long)ctx->cu_count * ctx->tune.mvreg_forget_bpc);
    hipStream_t s = ctx->stream;
    if (A > 128) launch_forget_vm<64, 2>(p, vec, grid, s);
    else switch (G) {
        case 1: launch_forget_vm<1, 1>(p, vec, grid, s); break;
        case 2: launch_forget_vm<2, 1>(p, vec, grid, s); break;
        case 4: launch_forget_vm<4, 1>(p, vec, grid, s); break;
        case 8: launch_forget_vm<8, 1>(p, vec, grid, s); break;
        case 16: launch_forget_vm<16, 1>(p, vec, grid, s); break;
        case 32: launch_forget_vm<32, 1>(p, vec, grid, s); break;
        default: launch_forget_vm<64, 1>(p, vec, grid, s); break;
      }
  }
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "mvreg_forget_kernel launch");
  return CRDT_OK;
}

}  // extern "C"
