// Batched state equality, the reference's PartialEq on N pairs of dense states:
//   crdt_mvreg_eq_batch   MVReg  (hand-written, order-free: mvreg.rs:62-86)
//   crdt_orswot_eq_batch  Orswot (derived: orswot.rs:20; VClock vclock.rs:56)
//   crdt_map_eq_batch     Map<K, MVReg> (derived: map.rs:31-47, with the MVReg rule per key)
// ne[i] = 0 iff x[i] == y[i], else the complete set of CRDT_NE_* components that differ.  Both sides
// are read only; the work is a 2-read stream with one word out per pair.
//
// Four kernels, each reading its bytes once:
//   eq_dense_kernel     clock row and entry rows (Orswot: entries[M][A]; Map: the clock alone), word by
//                       word over the full u64, in 16-byte non-temporal pieces where rows are 16-byte
//                       aligned (8-byte words otherwise).  Each lane ORs x ^ y into one register per
//                       component, one vote at the end.  A state takes a sub-wave segment of 1..64 lanes
//                       (about 8 pieces per lane) or, past 16 KiB per side, a workgroup.  The owner
//                       writes ne[s] with a plain store (CLOCK | ENTRIES, or INVALID alone when a
//                       def_count is above its Dcap), so ne needs no zeroing.
//   eq_deferred_kernel  one wave per state after the dense kernel; both counts 0 costs the two counts.
//                       Equal counts with slot-by-slot identical rows are equal (one streaming compare).
//                       Otherwise clocks are matched through per-slot 64-bit row hashes in LDS (the
//                       first 128 slots of each side; the slots past them are compared row by row in the
//                       state's own memory), the sets of equal clocks are unioned per side and the unions
//                       compared; a clock of one side missing on the other is unequal whatever its set.
//                       The owner lane ORs DEFERRED into ne[s] (plain read-modify-write, one owner).
//   eq_reg_kernel       registers: MVReg i, or key k of Map state s with its entry-clock row.  A <= 256
//                       and V <= 8: a sub-wave segment per register as in mvreg_forget.hip, all slots of
//                       both sides loaded before the first vote; every lane packs "slot s of x / y is
//                       non-empty", "slot s differs from slot s" (and the entry row's bits) into one
//                       word, OR-reduced over the segment by log2(G) shuffles.  Slot s against slot s with
//                       equal values settles identical layouts; only a wave with a register that fails it
//                       runs the VM x VM search (one 64-bit pair mask per lane, one more reduce).
//   eq_reg_wide_kernel  A > 256 or V > 8: a workgroup per register, thread t = actor t, the same masks
//                       reduced over the workgroup; unmatched slots search the other side's slots by
//                       re-reading them.  The slot masks are u32 words up to 32 slots a side and u64
//                       words for 33..64.
// The Map's register kernels have K owners per state, so a key that differs ORs its bits into ne[s]
// with an atomic; keys that are equal (the stream's common case) write nothing.
// The loads, the plans of the dense and deferred kernels and the list compare itself
// (eq_deferred_pair) are in eq_common.hpp, shared with the value-typed Maps' calls (eq_vmap.hip).
#include "eq_common.hpp"

namespace crdt {


// x ^ y over words [0, n) of two rows, lane g of G, ORed into d
template <bool VEC>
__device__ __forceinline__ void eq_row_diff(const u64 *xr, const u64 *yr, unsigned long long n, unsigned g, unsigned G,
                                            u64 &d) {
  if (VEC) {  // n even, rows 16-byte aligned
    const unsigned long long st = 2ull * G;
    unsigned long long a = 2ull * g;
    for (; a + 3 * st < n; a += 4 * st) {
      u64x2 t[4], u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        t[q] = eq_ld2(xr + a + q * st);
        u[q] = eq_ld2(yr + a + q * st);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) d |= (t[q].x ^ u[q].x) | (t[q].y ^ u[q].y);
    }
    for (; a < n; a += st) {
      const u64x2 t = eq_ld2(xr + a), u = eq_ld2(yr + a);
      d |= (t.x ^ u.x) | (t.y ^ u.y);
    }
  } else {
    unsigned long long a = g;
    for (; a + 3ull * G < n; a += 4ull * G) {
      u64 t[4], u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        t[q] = eq_ld1(xr + a + q * (unsigned long long)G);
        u[q] = eq_ld1(yr + a + q * (unsigned long long)G);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) d |= t[q] ^ u[q];
    }
    for (; a < n; a += G) d |= eq_ld1(xr + a) ^ eq_ld1(yr + a);
  }
}

template <bool VC, bool VE>
__device__ __forceinline__ void eq_dense_diff(const EqDensePlan &p, unsigned long long s, unsigned g, unsigned G, u64 &dc,
                                              u64 &de) {
  eq_row_diff<VC>(p.x.clock + s * p.x.cs, p.y.clock + s * p.y.cs, p.A, g, G, dc);
  for (unsigned long long r = 0; r < p.R; ++r)
    eq_row_diff<VE>(p.x.rows + s * p.x.ss + r * p.x.rs, p.y.rows + s * p.y.ss + r * p.y.rs, p.L, g, G, de);
}

__device__ __forceinline__ bool eq_invalid(const uint32_t *xc, unsigned long long xcap, const uint32_t *yc,
                                           unsigned long long ycap, unsigned long long s) {
  const unsigned long long nx = xc ? xc[s] : 0, ny = yc ? yc[s] : 0;
  return nx > xcap || ny > ycap;
}

template <bool VC, bool VE>
__global__ __launch_bounds__(kBlock) void eq_dense_kernel(EqDensePlan p) {
  const int lane = threadIdx.x % kWave;
  if (p.lg == 8) {  // one workgroup per state
    __shared__ unsigned red[kBlock / kWave];
    for (unsigned long long s = blockIdx.x; s < p.N; s += gridDim.x) {  // workgroup-uniform
      u64 dc = 0, de = 0;
      eq_dense_diff<VC, VE>(p, s, threadIdx.x, kBlock, dc, de);
      const unsigned b = (__ballot(dc != 0) ? CRDT_NE_CLOCK : 0u) | (__ballot(de != 0) ? CRDT_NE_ENTRIES : 0u);
      if (lane == 0) red[threadIdx.x / kWave] = b;
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned bits = 0;
        for (int w = 0; w < kBlock / kWave; ++w) bits |= red[w];
        if (eq_invalid(p.x.cnt, p.x.dcap, p.y.cnt, p.y.dcap, s)) bits = CRDT_NE_INVALID;
        p.ne[s] = bits;
      }
      __syncthreads();  // red is reused by the next state
    }
    return;
  }
  const unsigned G = 1u << p.lg, RPW = kWave >> p.lg;
  const unsigned g = lane & (G - 1), seg = lane >> p.lg;
  const u64 smask = G == kWave ? ~0ull : ((1ull << G) - 1);
  const int sshift = seg * G;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long ngroup = (p.N + RPW - 1) / RPW;
  for (unsigned long long wv = wave0; wv < ngroup; wv += nwave) {  // wave-uniform
    const unsigned long long s = wv * RPW + seg;
    const bool live = s < p.N;
    u64 dc = 0, de = 0;
    if (live) eq_dense_diff<VC, VE>(p, s, g, G, dc, de);
    const bool nc = ((__ballot(dc != 0) >> sshift) & smask) != 0;
    const bool nr = ((__ballot(de != 0) >> sshift) & smask) != 0;
    if (live && g == 0) {
      unsigned bits = (nc ? CRDT_NE_CLOCK : 0u) | (nr ? CRDT_NE_ENTRIES : 0u);
      if (eq_invalid(p.x.cnt, p.x.dcap, p.y.cnt, p.y.dcap, s)) bits = CRDT_NE_INVALID;
      p.ne[s] = bits;
    }
  }
}

// ---- deferred removes ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void eq_deferred_kernel(EqDefPlan p) {
  __shared__ u64 hsh[kBlock / kWave][2][kDefWin];
  const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
  u64 *hx = hsh[wid][0], *hy = hsh[wid][1];
  const unsigned long long A = p.A, W = p.W;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  for (unsigned long long s = wave0; s < p.N; s += nwave) {  // wave-uniform
    if (p.norm) {  // a per-key owner of an earlier launch reported a bad nested count
      const unsigned w = p.ne[s];
      if (w & CRDT_NE_INVALID) {
        if (lane == 0 && w != CRDT_NE_INVALID) p.ne[s] = CRDT_NE_INVALID;
        continue;
      }
    }
    const unsigned long long cx = p.x.cnt ? p.x.cnt[s] : 0, cy = p.y.cnt ? p.y.cnt[s] : 0;
    if (cx > p.x.dcap || cy > p.y.dcap) continue;  // INVALID, written by the dense kernel
    if (cx == 0 && cy == 0) continue;
    const bool ne = eq_deferred_pair(p.x.clock + s * p.x.dcap * A, p.x.sets + s * p.x.dcap * W, (unsigned)cx,
                                     p.y.clock + s * p.y.dcap * A, p.y.sets + s * p.y.dcap * W, (unsigned)cy, A, W, lane, hx,
                                     hy);
    if (ne && lane == 0) p.ne[s] |= CRDT_NE_DEFERRED;
  }
}

// ---- registers -------------------------------------------------------------------------------------
struct EqRegSide {
  const u64 *vclk, *vval, *ec;
  unsigned long long cs, vs, es, V;
  const uint32_t *cnt;
  unsigned long long dcap;
};
struct EqRegPlan {
  EqRegSide x, y;
  unsigned long long N, K, A;  // N states of K registers (MVReg: K = 1)
  uint32_t *ne;
  int lg;
};

// the owner of register (s, k) reports its bits
template <bool MAP>
__device__ __forceinline__ void eq_reg_report(const EqRegPlan &p, unsigned long long s, unsigned bits) {
  if (!MAP) {
    p.ne[s] = bits;
  } else if (bits && !eq_invalid(p.x.cnt, p.x.dcap, p.y.cnt, p.y.dcap, s)) {
    atomicOr(p.ne + s, bits);
  }
}

template <int CH, int VM, bool VEC>
__device__ __forceinline__ void eq_load_reg(const u64 *rc, const u64 *rv, unsigned long long V, unsigned long long A,
                                            const bool (&on0)[CH], const bool (&on1)[CH],
                                            const unsigned long long (&a0)[CH], bool live, u64 (&cv)[VM][CH][2],
                                            u64 (&vv)[VM]) {
#pragma unroll
  for (int s = 0; s < VM; ++s) {
    const bool sl = (unsigned long long)s < V;
    vv[s] = (live && sl) ? rv[s] : 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      cv[s][c][0] = cv[s][c][1] = 0;
      if (VEC) {
        if (sl && on0[c]) {
          const u64x2 t = eq_ld2(rc + s * A + a0[c]);
          cv[s][c][0] = t.x;
          cv[s][c][1] = t.y;
        }
      } else {
        if (sl && on0[c]) cv[s][c][0] = eq_ld1(rc + s * A + a0[c]);
        if (sl && on1[c]) cv[s][c][1] = eq_ld1(rc + s * A + a0[c] + 1);
      }
    }
  }
}

template <int CH, int VM, bool VEC, bool MAP>
__global__ __launch_bounds__(kBlock) void eq_reg_kernel(EqRegPlan p) {
  const int lane = threadIdx.x % kWave;
  const unsigned G = 1u << p.lg, RPW = kWave >> p.lg;
  const unsigned g = lane & (G - 1), seg = lane >> p.lg;
  const unsigned long long A = p.A, NR = p.N * p.K;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long ngroup = (NR + RPW - 1) / RPW;
  constexpr unsigned VMASK = (1u << VM) - 1u;
  for (unsigned long long wv = wave0; wv < ngroup; wv += nwave) {  // wave-uniform
    const unsigned long long r = wv * RPW + seg;
    const bool live = r < NR;
    const unsigned long long s = live ? (MAP ? r / p.K : r) : 0, k = live ? (MAP ? r - s * p.K : 0) : 0;
    bool on0[CH], on1[CH];
    unsigned long long a0[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      a0[c] = 2ull * (g + (unsigned long long)G * c);
      on0[c] = live && a0[c] < A;
      on1[c] = live && a0[c] + 1 < A;
    }
    u64 cx[VM][CH][2], cy[VM][CH][2], vx[VM], vy[VM];
    eq_load_reg<CH, VM, VEC>(p.x.vclk + s * p.x.cs + k * p.x.V * A, p.x.vval + s * p.x.vs + k * p.x.V, p.x.V, A, on0, on1,
                             a0, live, cx, vx);
    eq_load_reg<CH, VM, VEC>(p.y.vclk + s * p.y.cs + k * p.y.V * A, p.y.vval + s * p.y.vs + k * p.y.V, p.y.V, A, on0, on1,
                             a0, live, cy, vy);
    // one word per lane: bits [0, VM) slot of x non-empty, [VM, 2VM) slot of y non-empty, [2VM, 3VM) slot s
    // of x differs from slot s of y; 24 the entry rows differ, 25 / 26 the key is present in x / y
    unsigned m = 0;
    if (MAP) {
      const u64 *ex = p.x.ec + s * p.x.es + k * A, *ey = p.y.ec + s * p.y.es + k * A;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        u64 e0 = 0, e1 = 0, f0 = 0, f1 = 0;
        if (VEC) {
          if (on0[c]) {
            const u64x2 t = eq_ld2(ex + a0[c]), u = eq_ld2(ey + a0[c]);
            e0 = t.x, e1 = t.y, f0 = u.x, f1 = u.y;
          }
        } else {
          if (on0[c]) e0 = eq_ld1(ex + a0[c]), f0 = eq_ld1(ey + a0[c]);
          if (on1[c]) e1 = eq_ld1(ex + a0[c] + 1), f1 = eq_ld1(ey + a0[c] + 1);
        }
        if ((e0 ^ f0) | (e1 ^ f1)) m |= 1u << 24;
        if (e0 | e1) m |= 1u << 25;
        if (f0 | f1) m |= 1u << 26;
      }
    }
#pragma unroll
    for (int q = 0; q < VM; ++q) {
      u64 nx = 0, ny = 0, d = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          nx |= cx[q][c][h];
          ny |= cy[q][c][h];
          d |= cx[q][c][h] ^ cy[q][c][h];
        }
      if (nx) m |= 1u << q;
      if (ny) m |= 1u << (VM + q);
      if (d) m |= 1u << (2 * VM + q);
    }
    for (unsigned off = 1; off < G; off <<= 1) m |= __shfl_xor(m, off, kWave);  // stays inside the segment
    // an absent key's register is the empty set
    const unsigned nzx = (!MAP || ((m >> 25) & 1u)) ? (m & VMASK) : 0u;
    const unsigned nzy = (!MAP || ((m >> 26) & 1u)) ? ((m >> VM) & VMASK) : 0u;
    unsigned same = 0;  // slot q of x and slot q of y hold the same (clock, value)
#pragma unroll
    for (int q = 0; q < VM; ++q)
      if (!((m >> (2 * VM + q)) & 1u) && vx[q] == vy[q]) same |= 1u << q;
    same &= nzx & nzy;
    bool vne = false;
    if (__any((nzx | nzy) & ~same)) {  // some register of this wave is laid out differently: search
      u64 pm = 0;  // bit q * VM + t: slot q of x and slot t of y differ in a word of this lane
#pragma unroll
      for (int q = 0; q < VM; ++q)
#pragma unroll
        for (int t = 0; t < VM; ++t) {
          u64 d = 0;
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) d |= cx[q][c][h] ^ cy[t][c][h];
          if (d) pm |= 1ull << (q * VM + t);
        }
      for (unsigned off = 1; off < G; off <<= 1) pm |= __shfl_xor(pm, off, kWave);
      unsigned fx = 0, fy = 0;
#pragma unroll
      for (int q = 0; q < VM; ++q)
#pragma unroll
        for (int t = 0; t < VM; ++t)
          if (((nzx >> q) & 1u) && ((nzy >> t) & 1u) && !((pm >> (q * VM + t)) & 1ull) && vx[q] == vy[t]) {
            fx |= 1u << q;
            fy |= 1u << t;
          }
      vne = ((nzx & ~fx) | (nzy & ~fy)) != 0;
    }
    if (live && g == 0)
      eq_reg_report<MAP>(p, s, (vne ? CRDT_NE_VALUES : 0u) | ((MAP && ((m >> 24) & 1u)) ? CRDT_NE_ENTRIES : 0u));
  }
}

// Workgroup-wide OR of NW words; every thread gets the result.  red: [16][NW].
template <int NW, typename M>
__device__ __forceinline__ void eq_block_or(M (&v)[NW], M *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int w = 0; w < NW; ++w) v[w] |= __shfl_xor(v[w], off, kWave);
  const int nw = blockDim.x / kWave, wv = threadIdx.x / kWave;
  if (nw == 1) return;
  __syncthreads();  // red may still be read by the round before
  if ((threadIdx.x % kWave) == 0)
#pragma unroll
    for (int w = 0; w < NW; ++w) red[wv * NW + w] = v[w];
  __syncthreads();
  for (int x = 0; x < nw; ++x)
#pragma unroll
    for (int w = 0; w < NW; ++w) v[w] |= red[x * NW + w];
}

// One workgroup per register (A > 256 or V > 8): thread t = actor t; M is the slot mask, u32 for up
// to 32 slots a side and u64 for up to 64.
template <bool MAP, typename M>
__global__ __launch_bounds__(1024) void eq_reg_wide_kernel(EqRegPlan p) {
  __shared__ M red[16 * 4];
  const unsigned t = threadIdx.x;
  const unsigned long long A = p.A, NR = p.N * p.K;
  const unsigned Vx = (unsigned)p.x.V, Vy = (unsigned)p.y.V, Vm = Vx > Vy ? Vx : Vy;
  const bool on = t < A;
  for (unsigned long long r = blockIdx.x; r < NR; r += gridDim.x) {  // workgroup-uniform
    const unsigned long long s = MAP ? r / p.K : r, k = MAP ? r - s * p.K : 0;
    const u64 *xr = p.x.vclk + s * p.x.cs + k * Vx * A, *yr = p.y.vclk + s * p.y.cs + k * Vy * A;
    const u64 *xv = p.x.vval + s * p.x.vs + k * Vx, *yv = p.y.vval + s * p.y.vs + k * Vy;
    M v[4] = {0, 0, 0, 0};  // non-empty slots of x, of y, slot s differs from slot s, entry-row bits
    if (MAP) {
      const u64 e = on ? eq_ld1(p.x.ec + s * p.x.es + k * A + t) : 0, f = on ? eq_ld1(p.y.ec + s * p.y.es + k * A + t) : 0;
      v[3] = (e != f ? 1u : 0u) | (e ? 2u : 0u) | (f ? 4u : 0u);
    }
    for (unsigned q = 0; q < Vm; ++q) {
      const u64 a = (on && q < Vx) ? eq_ld1(xr + q * A + t) : 0, b = (on && q < Vy) ? eq_ld1(yr + q * A + t) : 0;
      if (a) v[0] |= M(1) << q;
      if (b) v[1] |= M(1) << q;
      if (a != b) v[2] |= M(1) << q;
    }
    eq_block_or<4, M>(v, red);
    const M nzx = (!MAP || (v[3] & 2u)) ? v[0] : M(0), nzy = (!MAP || (v[3] & 4u)) ? v[1] : M(0);
    M ux = 0, uy = 0;  // slots not settled by slot s against slot s
    for (unsigned q = 0; q < Vm; ++q) {
      const bool bx = (nzx >> q) & 1u, by = (nzy >> q) & 1u;
      const bool same = bx && by && !((v[2] >> q) & 1u) && xv[q] == yv[q];
      if (bx && !same) ux |= M(1) << q;
      if (by && !same) uy |= M(1) << q;
    }
    bool vne = false;
    for (unsigned q = 0; q < Vx && !vne; ++q) {  // an unsettled slot of x searches y's slots
      if (!((ux >> q) & 1u)) continue;
      const u64 a = on ? xr[q * A + t] : 0;
      M d[1] = {0};
      for (unsigned j = 0; j < Vy; ++j)
        if (!((nzy >> j) & 1u) || a != (on ? yr[j * A + t] : 0)) d[0] |= M(1) << j;
      eq_block_or<1, M>(d, red);
      bool found = false;
      for (unsigned j = 0; j < Vy; ++j) found |= !((d[0] >> j) & 1u) && xv[q] == yv[j];
      vne = !found;
    }
    for (unsigned j = 0; j < Vy && !vne; ++j) {
      if (!((uy >> j) & 1u)) continue;
      const u64 b = on ? yr[j * A + t] : 0;
      M d[1] = {0};
      for (unsigned q = 0; q < Vx; ++q)
        if (!((nzx >> q) & 1u) || b != (on ? xr[q * A + t] : 0)) d[0] |= M(1) << q;
      eq_block_or<1, M>(d, red);
      bool found = false;
      for (unsigned q = 0; q < Vx; ++q) found |= !((d[0] >> q) & 1u) && xv[q] == yv[j];
      vne = !found;
    }
    if (t == 0) eq_reg_report<MAP>(p, s, (vne ? CRDT_NE_VALUES : 0u) | ((MAP && (v[3] & 1u)) ? CRDT_NE_ENTRIES : 0u));
  }
}

// ---- launches --------------------------------------------------------------------------------------
static bool eq_al16(const void *p) { return (uintptr_t)p % 16 == 0; }

void launch_eq_dense(crdt_ctx *ctx, EqDensePlan p) {
  const size_t N = p.N;
  // 16-byte pieces: every row of both sides starts on a 16-byte boundary and has an even length
  const bool vc = p.A % 2 == 0 && eq_al16(p.x.clock) && eq_al16(p.y.clock) && (N == 1 || (p.x.cs % 2 == 0 && p.y.cs % 2 == 0));
  const bool ve = p.R == 0 || (p.L % 2 == 0 && eq_al16(p.x.rows) && eq_al16(p.y.rows) &&
                               (N == 1 || (p.x.ss % 2 == 0 && p.y.ss % 2 == 0)) &&
                               (p.R == 1 || (p.x.rs % 2 == 0 && p.y.rs % 2 == 0)));
  const unsigned long long pieces = (p.A + p.R * p.L + 1) / 2;
  unsigned grid;
  if (pieces > 1024) {
    p.lg = 8;
    grid = (unsigned)std::min<unsigned long long>(N, (unsigned long long)ctx->cu_count * 32);
  } else {
    p.lg = row_lr_log(pieces);
    const unsigned long long rpw = kWave >> p.lg, waves = (N + rpw - 1) / rpw;
    grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                  (unsigned long long)ctx->cu_count * 32);
  }
  hipStream_t s = ctx->stream;
  if (vc && ve) hipLaunchKernelGGL((eq_dense_kernel<true, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (vc) hipLaunchKernelGGL((eq_dense_kernel<true, false>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (ve) hipLaunchKernelGGL((eq_dense_kernel<false, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((eq_dense_kernel<false, false>), dim3(grid), dim3(kBlock), 0, s, p);
}

void launch_eq_deferred(crdt_ctx *ctx, const EqDefPlan &p) {
  const unsigned long long want = (p.N + kBlock / kWave - 1) / (kBlock / kWave);
  const unsigned grid = (unsigned)std::min<unsigned long long>(want, (unsigned long long)ctx->cu_count * 32);
  hipLaunchKernelGGL(eq_deferred_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, p);
}

template <int CH, int VM, bool MAP>
static void launch_eq_reg_vec(const EqRegPlan &p, bool vec, unsigned grid, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((eq_reg_kernel<CH, VM, true, MAP>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((eq_reg_kernel<CH, VM, false, MAP>), dim3(grid), dim3(kBlock), 0, s, p);
}

template <bool MAP>
static void launch_eq_reg(crdt_ctx *ctx, EqRegPlan p) {
  const size_t A = p.A, Vm = std::max(p.x.V, p.y.V);
  const unsigned long long NR = p.N * p.K;
  hipStream_t s = ctx->stream;
  if (A > 256 || Vm > 8) {
    const unsigned nt = (unsigned)std::max<size_t>(64, (A + 63) / 64 * 64);
    const unsigned grid = (unsigned)std::min<unsigned long long>(NR, 0x7fffffffull);
    if (Vm > 32) hipLaunchKernelGGL((eq_reg_wide_kernel<MAP, u64>), dim3(grid), dim3(nt), 0, s, p);
    else hipLaunchKernelGGL((eq_reg_wide_kernel<MAP, unsigned>), dim3(grid), dim3(nt), 0, s, p);
    return;
  }
  bool vec = A % 2 == 0 && eq_al16(p.x.vclk) && eq_al16(p.y.vclk) && (p.N == 1 || (p.x.cs % 2 == 0 && p.y.cs % 2 == 0));
  if (MAP) vec = vec && eq_al16(p.x.ec) && eq_al16(p.y.ec) && (p.N == 1 || (p.x.es % 2 == 0 && p.y.es % 2 == 0));
  int lg = 0;  // lanes per register: the 16-byte pieces of a row, rounded up to a power of two
  while ((1u << lg) < (A + 1) / 2 && lg < 6) ++lg;
  p.lg = lg;
  const unsigned long long rpw = kWave >> lg, waves = (NR + rpw - 1) / rpw;
  const unsigned grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                               (unsigned long long)ctx->cu_count * 32);
  if (A > 128) {
    if (Vm <= 4) launch_eq_reg_vec<2, 4, MAP>(p, vec, grid, s);
    else launch_eq_reg_vec<2, 8, MAP>(p, vec, grid, s);
  } else {
    if (Vm <= 4) launch_eq_reg_vec<1, 4, MAP>(p, vec, grid, s);
    else launch_eq_reg_vec<1, 8, MAP>(p, vec, grid, s);
  }
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_mvreg_eq_batch(crdt_ctx *ctx, const crdt_mvreg_states *x, const crdt_mvreg_states *y, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "mvreg_eq_batch: NULL states");
  if (x->N != y->N || x->A != y->A) return fail(ctx, CRDT_EINVAL, "mvreg_eq_batch: x and y differ in N or A");
  const size_t N = x->N, A = x->A;
  if (N == 0) return CRDT_OK;
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_eq_batch: A = %zu > 1024 actors", A);
  for (const crdt_mvreg_states *st : {x, y}) {
    if (st->V == 0 || st->V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_eq_batch: V = %zu not in [1, 64]", st->V);
    if (A && (!st->vclk || !st->vval)) return fail(ctx, CRDT_EINVAL, "mvreg_eq_batch: NULL register buffers");
    if (N > 1 && (st->vclk_stride < st->V * A || st->vval_stride < st->V))
      return fail(ctx, CRDT_EINVAL, "mvreg_eq_batch: strides below the register size");
  }
  if (!ne) return fail(ctx, CRDT_EINVAL, "mvreg_eq_batch: NULL ne");
  if (N > 0x7fffffffULL) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_eq_batch: N too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  if (A == 0) return device_fill(ctx, ne, N * sizeof(uint32_t), 0);  // every register is empty
  EqRegPlan p{};
  p.x = EqRegSide{(const u64 *)x->vclk, (const u64 *)x->vval, nullptr, x->vclk_stride, x->vval_stride, 0, x->V, nullptr, 0};
  p.y = EqRegSide{(const u64 *)y->vclk, (const u64 *)y->vval, nullptr, y->vclk_stride, y->vval_stride, 0, y->V, nullptr, 0};
  p.N = N;
  p.K = 1;
  p.A = A;
  p.ne = ne;
  timing_begin(ctx, "mvreg_eq");
  launch_eq_reg<false>(ctx, p);
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "eq_reg_kernel launch");
  return CRDT_OK;
}

int crdt_orswot_eq_batch(crdt_ctx *ctx, const crdt_orswot_states *x, const crdt_orswot_states *y, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: NULL states");
  if (x->N != y->N || x->M != y->M || x->A != y->A)
    return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: x and y differ in N, M or A");
  const size_t N = x->N, M = x->M, A = x->A, Mw = (M + 63) / 64;
  if (N == 0) return CRDT_OK;
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "orswot_eq_batch: A = %zu > 1024 actors", A);
  for (const crdt_orswot_states *st : {x, y}) {
    if (A && (!st->clock || (M && !st->entries))) return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: NULL clock / entries");
    if (N > 1 && st->clock_stride < A) return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: clock_stride < A");
    if (M > 1 && st->entry_mstride < A) return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: entry_mstride < A");
    if (N > 1 && M && st->entry_sstride < (M - 1) * st->entry_mstride + A)
      return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: entry_sstride below the state size");
    if (st->Dcap && (!st->def_count || (A && !st->def_clock) || (Mw && !st->def_members)))
      return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: NULL deferred buffers with Dcap > 0");
  }
  if (!ne) return fail(ctx, CRDT_EINVAL, "orswot_eq_batch: NULL ne");
  if (N > 0x7fffffffULL) return fail(ctx, CRDT_EUNSUPPORTED, "orswot_eq_batch: N too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  const bool flat = M <= 1 || (x->entry_mstride == A && y->entry_mstride == A);  // packed rows: one row of M * A words
  EqDensePlan p{};
  p.x = EqDenseSide{(const u64 *)x->clock, x->clock_stride, (const u64 *)x->entries, x->entry_mstride, x->entry_sstride,
                    x->def_count, x->Dcap};
  p.y = EqDenseSide{(const u64 *)y->clock, y->clock_stride, (const u64 *)y->entries, y->entry_mstride, y->entry_sstride,
                    y->def_count, y->Dcap};
  p.N = N;
  p.A = A;
  p.R = (M == 0 || A == 0) ? 0 : (flat ? 1 : M);
  p.L = flat ? M * A : A;
  p.ne = ne;
  timing_begin(ctx, "orswot_eq");
  launch_eq_dense(ctx, p);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && (x->Dcap || y->Dcap)) {
    EqDefPlan d{};
    d.x = EqDefSide{(const u64 *)x->def_clock, (const u64 *)x->def_members, p.x.cnt, x->Dcap};
    d.y = EqDefSide{(const u64 *)y->def_clock, (const u64 *)y->def_members, p.y.cnt, y->Dcap};
    d.N = N;
    d.A = A;
    d.W = Mw;
    d.ne = ne;
    launch_eq_deferred(ctx, d);
    e = hipGetLastError();
  }
  timing_end(ctx);  // the bracket covers every launch of the call
  if (e != hipSuccess) return hip_fail(ctx, e, "orswot_eq_batch kernel launch");
  return CRDT_OK;
}

int crdt_map_eq_batch(crdt_ctx *ctx, const crdt_map_states *x, const crdt_map_deferred *xd, const crdt_map_states *y,
                      const crdt_map_deferred *yd, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "map_eq_batch: NULL states");
  if (x->N != y->N || x->K != y->K || x->A != y->A) return fail(ctx, CRDT_EINVAL, "map_eq_batch: x and y differ in N, K or A");
  const size_t N = x->N, K = x->K, A = x->A, Kw = (K + 63) / 64;
  if (N == 0) return CRDT_OK;
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "map_eq_batch: A = %zu > 1024 actors", A);
  const size_t xcap = xd ? xd->Dcap : 0, ycap = yd ? yd->Dcap : 0;
  for (int side = 0; side < 2; ++side) {
    const crdt_map_states *st = side ? y : x;
    const crdt_map_deferred *df = side ? yd : xd;
    if (st->V == 0 || st->V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "map_eq_batch: V = %zu not in [1, 64]", st->V);
    if (A && (!st->clock || (K && (!st->ec || !st->vclk || !st->vval))))
      return fail(ctx, CRDT_EINVAL, "map_eq_batch: NULL state buffers");
    if (N > 1 && (st->clock_stride < A || st->ec_stride < K * A || st->vclk_stride < K * st->V * A ||
                  st->vval_stride < K * st->V))
      return fail(ctx, CRDT_EINVAL, "map_eq_batch: strides below the state size");
    if (df && df->Dcap && (!df->count || (A && !df->clock) || (Kw && !df->keys)))
      return fail(ctx, CRDT_EINVAL, "map_eq_batch: NULL deferred buffers with Dcap > 0");
  }
  if (!ne) return fail(ctx, CRDT_EINVAL, "map_eq_batch: NULL ne");
  if (N > 0x7fffffffULL || (K && N > 0x7fffffffULL / K)) return fail(ctx, CRDT_EUNSUPPORTED, "map_eq_batch: N * K too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t *xc = xd ? xd->count : nullptr, *yc = yd ? yd->count : nullptr;  // read whenever given
  EqDensePlan p{};  // the clock alone: the entry rows go with their registers
  p.x = EqDenseSide{(const u64 *)x->clock, x->clock_stride, nullptr, 0, 0, xc, xcap};
  p.y = EqDenseSide{(const u64 *)y->clock, y->clock_stride, nullptr, 0, 0, yc, ycap};
  p.N = N;
  p.A = A;
  p.ne = ne;
  timing_begin(ctx, "map_eq");  // the bracket covers every launch of the call
  launch_eq_dense(ctx, p);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && (xcap || ycap)) {
    EqDefPlan d{};
    d.x = EqDefSide{xcap ? (const u64 *)xd->clock : nullptr, xcap ? (const u64 *)xd->keys : nullptr, xc, xcap};
    d.y = EqDefSide{ycap ? (const u64 *)yd->clock : nullptr, ycap ? (const u64 *)yd->keys : nullptr, yc, ycap};
    d.N = N;
    d.A = A;
    d.W = Kw;
    d.ne = ne;
    launch_eq_deferred(ctx, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess && K && A) {
    EqRegPlan r{};
    r.x = EqRegSide{(const u64 *)x->vclk, (const u64 *)x->vval, (const u64 *)x->ec, x->vclk_stride, x->vval_stride,
                    x->ec_stride, x->V, xc, xcap};
    r.y = EqRegSide{(const u64 *)y->vclk, (const u64 *)y->vval, (const u64 *)y->ec, y->vclk_stride, y->vval_stride,
                    y->ec_stride, y->V, yc, ycap};
    r.N = N;
    r.K = K;
    r.A = A;
    r.ne = ne;
    launch_eq_reg<true>(ctx, r);
    e = hipGetLastError();
  }
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "map_eq_batch kernel launch");
  return CRDT_OK;
}

}  // extern "C"
