// Batched state equality of the value-typed Maps, the reference's derived PartialEq (map.rs:31-47) on N
// pairs of dense states with the value type's own PartialEq per key:
//   crdt_map_counter_eq_batch  Map<K, GCounter / PNCounter>  (gcounter.rs / pncounter.rs: derived)
//   crdt_map_orswot_eq_batch   Map<K, Orswot<M>>             (orswot.rs:20: derived)
//   crdt_map_nested_eq_batch   Map<K, Map<K2, MVReg>>        (map.rs:31-47 one level down, mvreg.rs:62-86)
// ne[i] = 0 iff x[i] == y[i], else the complete set of CRDT_NE_* components that differ.  Both sides
// are read only; no allocation, no scratch and no host synchronisation.
//
// Launches of one call, in stream order:
//   eq_dense_kernel (eq.hip)  the Map's clock row; ne[s] by a plain store, so ne needs no zeroing.
//   eqv_key_kernel            one item per key (s, k), a sub-wave segment of 1..64 lanes sized from the
//                             key's bytes or, past 16 KiB a side, a workgroup.  Entry row and the value's
//                             plain rows (counter rows; oc and ent; ic) in 16-byte non-temporal pieces
//                             (8-byte words for odd A), every lane ORing x ^ y, x and y into six
//                             accumulators whose non-zero bits one OR-reduce packs.  The owner decides
//                             without loading presence first.  The nested counts vd_n / id_n are read
//                             here (a non-zero count is a non-default value; one zero and one non-zero
//                             count differ; a count above its capacity is INVALID); the slots are not.
//   eqv_list_kernel           nested lists: a lane per key reads the two counts; keys with both non-zero
//                             take the wave in turn: presence from the two entry rows, then
//                             eq_deferred_pair (eq_common.hpp), the Map-level lists' exact compare.
//   eqv_reg_kernel            nested Map only: one item per inner register (s, k, j), a sub-wave segment
//                             over the row.  Inner entry row, then slot q against slot q below the two
//                             nval counts with its value; per-slot masks in three 64-bit words, one
//                             OR-reduce.  Only a wave with a register that this does not settle searches:
//                             up to 8 slots a side inside the segment (eq_reg_kernel's 64-bit pair mask,
//                             the slots loaded again, one more reduce); past that, untuned, the register
//                             takes the wave and every unsettled slot is compared row by row with the
//                             other side's slots.  A register that differs takes the wave to read the
//                             outer entry rows for presence.
//   eq_deferred_kernel (eq.hip)  the Map-level lists, one owner per state; it also turns a word that
//                             carries INVALID (a bad nested count) into INVALID alone.
// Keys and registers that are equal write nothing; one that differs ORs its bits into ne[s] with an
// atomic.
#include "eq_common.hpp"

namespace crdt {

struct EqvSide {
  const u64 *ec;                    // entry rows: ec + s * es + k * A
  unsigned long long es;
  const u64 *v0, *v1;               // the value's plain rows of key (s, k): v + s * vs + k * vk, vn words
  unsigned long long v0s, v0k, v1s, v1k;
  const uint32_t *ln;               // nested list counts [N * K] or NULL
  const u64 *lclk, *lset;           // [N * K][lcap][A], [N * K][lcap][LW]
  unsigned long long lcap;
  const u64 *iec, *ivc, *ivv;       // nested Map: [N * K][K2][A], [N * K][K2][Vs][A], [N * K][K2][Vs]
  const uint32_t *nval;             // [N * K][K2]
  unsigned long long Vs;
};
struct EqvPlan {
  EqvSide x, y;
  unsigned long long N, K, A, v0n, v1n, LW, K2;
  uint32_t *ne;
  int lg;  // log2 of the lanes per item; 8: one workgroup per item
};

// bits of the packed word of a key
constexpr unsigned kDE = 1, kEX = 2, kEY = 4, kDV = 8, kVX = 16, kVY = 32, kBAD = 64;

// words [0, n) of two rows, lane g of G: x ^ y, x and y ORed into d, ox, oy
template <bool VEC>
__device__ __forceinline__ void eqv_acc(const u64 *xr, const u64 *yr, unsigned long long n, unsigned g, unsigned G, u64 &d,
                                        u64 &ox, u64 &oy) {
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
      for (int q = 0; q < 4; ++q) {
        d |= (t[q].x ^ u[q].x) | (t[q].y ^ u[q].y);
        ox |= t[q].x | t[q].y;
        oy |= u[q].x | u[q].y;
      }
    }
    for (; a < n; a += st) {
      const u64x2 t = eq_ld2(xr + a), u = eq_ld2(yr + a);
      d |= (t.x ^ u.x) | (t.y ^ u.y);
      ox |= t.x | t.y;
      oy |= u.x | u.y;
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
      for (int q = 0; q < 4; ++q) {
        d |= t[q] ^ u[q];
        ox |= t[q];
        oy |= u[q];
      }
    }
    for (; a < n; a += G) {
      const u64 t = eq_ld1(xr + a), u = eq_ld1(yr + a);
      d |= t ^ u;
      ox |= t;
      oy |= u;
    }
  }
}

// the packed word of key r = (s, k) from this lane's pieces
template <bool VEC>
__device__ __forceinline__ unsigned eqv_key_word(const EqvPlan &p, unsigned long long r, unsigned long long s,
                                                 unsigned long long k, unsigned g, unsigned G) {
  u64 de = 0, ex = 0, ey = 0, dv = 0, vx = 0, vy = 0;
  eqv_acc<VEC>(p.x.ec + s * p.x.es + k * p.A, p.y.ec + s * p.y.es + k * p.A, p.A, g, G, de, ex, ey);
  if (p.v0n) eqv_acc<VEC>(p.x.v0 + s * p.x.v0s + k * p.x.v0k, p.y.v0 + s * p.y.v0s + k * p.y.v0k, p.v0n, g, G, dv, vx, vy);
  if (p.v1n) eqv_acc<VEC>(p.x.v1 + s * p.x.v1s + k * p.x.v1k, p.y.v1 + s * p.y.v1s + k * p.y.v1k, p.v1n, g, G, dv, vx, vy);
  unsigned m = (de ? kDE : 0u) | (ex ? kEX : 0u) | (ey ? kEY : 0u) | (dv ? kDV : 0u) | (vx ? kVX : 0u) | (vy ? kVY : 0u);
  if (p.x.ln && g == 0) {
    const unsigned long long nx = p.x.ln[r], ny = p.y.ln[r];
    if (nx > p.x.lcap || ny > p.y.lcap) m |= kBAD;
    else m |= (nx ? kVX : 0u) | (ny ? kVY : 0u) | ((nx == 0) != (ny == 0) ? kDV : 0u);  // both non-zero: the list kernel
  }
  return m;
}

// ENTRIES / VALUES of a key from its reduced word.  A key present on one side only has values that
// differ iff the present side's value is not V::default(); `more`: that side's value has further rows
// (the nested Map's inner entry rows) that the word does not cover.
__device__ __forceinline__ unsigned eqv_key_bits(unsigned m, bool &more_x, bool &more_y) {
  more_x = more_y = false;
  if (m & kBAD) return CRDT_NE_INVALID;
  unsigned bits = (m & kDE) ? CRDT_NE_ENTRIES : 0u;
  const bool px = m & kEX, py = m & kEY;
  if (px && py) {
    if (m & kDV) bits |= CRDT_NE_VALUES;
  } else if (px) {
    if (m & kVX) bits |= CRDT_NE_VALUES;
    else more_x = true;
  } else if (py) {
    if (m & kVY) bits |= CRDT_NE_VALUES;
    else more_y = true;
  }
  return bits;
}

template <bool VEC, bool NESTED>
__global__ __launch_bounds__(kBlock) void eqv_key_kernel(EqvPlan p) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long NK = p.N * p.K;
  if (p.lg == 8) {  // one workgroup per key (never the nested Map: its key is two rows here)
    __shared__ unsigned red[kBlock / kWave];
    for (unsigned long long r = blockIdx.x; r < NK; r += gridDim.x) {  // workgroup-uniform
      const unsigned long long s = r / p.K, k = r - s * p.K;
      unsigned m = eqv_key_word<VEC>(p, r, s, k, threadIdx.x, kBlock);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, kWave);
      if (lane == 0) red[threadIdx.x / kWave] = m;
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned all = 0;
        for (int w = 0; w < kBlock / kWave; ++w) all |= red[w];
        bool mx, my;
        const unsigned bits = eqv_key_bits(all, mx, my);
        if (bits) atomicOr(p.ne + s, bits);
      }
      __syncthreads();  // red is reused by the next key
    }
    return;
  }
  const unsigned G = 1u << p.lg, RPW = kWave >> p.lg;
  const unsigned g = lane & (G - 1), seg = lane >> p.lg;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long ngroup = (NK + RPW - 1) / RPW;
  for (unsigned long long wv = wave0; wv < ngroup; wv += nwave) {  // wave-uniform
    const unsigned long long r = wv * RPW + seg;
    const bool live = r < NK;
    const unsigned long long s = live ? r / p.K : 0, k = live ? r - s * p.K : 0;
    unsigned m = live ? eqv_key_word<VEC>(p, r, s, k, g, G) : 0u;
    for (unsigned off = 1; off < G; off <<= 1) m |= __shfl_xor(m, off, kWave);  // stays inside the segment
    bool mx, my;
    unsigned bits = eqv_key_bits(m, mx, my);
    if (NESTED && __any(mx || my)) {  // present on one side with ic == 0 and no inner removes: any inner entry?
      u64 o = 0;
      if (mx || my) {
        const u64 *row = (mx ? p.x.iec : p.y.iec) + r * p.K2 * p.A;
        for (unsigned long long a = g; a < p.K2 * p.A; a += G) o |= row[a];
      }
      unsigned nz = o ? 1u : 0u;
      for (unsigned off = 1; off < G; off <<= 1) nz |= __shfl_xor(nz, off, kWave);
      if (nz) bits |= CRDT_NE_VALUES;
    }
    if (live && g == 0 && bits) atomicOr(p.ne + s, bits);
  }
}

// ---- nested lists ----------------------------------------------------------------------------------
// both entry rows of key (s, k) non-zero?  The whole wave reads them; wave-uniform.
__device__ __forceinline__ bool eqv_both_present(const EqvPlan &p, unsigned long long s, unsigned long long k, int lane) {
  const u64 *ex = p.x.ec + s * p.x.es + k * p.A, *ey = p.y.ec + s * p.y.es + k * p.A;
  u64 ox = 0, oy = 0;
  for (unsigned long long a = lane; a < p.A; a += kWave) {
    ox |= ex[a];
    oy |= ey[a];
  }
  return __ballot(ox != 0) != 0 && __ballot(oy != 0) != 0;
}

__global__ __launch_bounds__(kBlock) void eqv_list_kernel(EqvPlan p) {
  __shared__ u64 hsh[kBlock / kWave][2][kDefWin];
  const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
  u64 *hx = hsh[wid][0], *hy = hsh[wid][1];
  const unsigned long long NK = p.N * p.K, A = p.A, W = p.LW;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  for (unsigned long long base = wave0 * kWave; base < NK; base += nwave * kWave) {  // wave-uniform
    const unsigned long long r = base + lane;
    unsigned long long nx = 0, ny = 0;
    if (r < NK) {
      nx = p.x.ln[r];
      ny = p.y.ln[r];
    }
    // one count 0: the key kernel decided; a bad count: INVALID, reported there
    u64 todo = __ballot(nx != 0 && ny != 0 && nx <= p.x.lcap && ny <= p.y.lcap);
    while (todo) {
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1;
      const unsigned long long rr = base + b, s = rr / p.K, k = rr - s * p.K;
      const unsigned cx = (unsigned)__shfl(nx, b, kWave), cy = (unsigned)__shfl(ny, b, kWave);
      if (!eqv_both_present(p, s, k, lane)) continue;  // a side's value is V::default(): the key kernel decided
      const bool ne = eq_deferred_pair(p.x.lclk + rr * p.x.lcap * A, p.x.lset + rr * p.x.lcap * W, cx,
                                       p.y.lclk + rr * p.y.lcap * A, p.y.lset + rr * p.y.lcap * W, cy, A, W, lane, hx, hy);
      if (ne && lane == 0) atomicOr(p.ne + s, CRDT_NE_VALUES);
    }
  }
}

// ---- inner registers of the nested Map -------------------------------------------------------------
constexpr int kRegVM = 8;  // slots a side up to which the set search stays inside the register's segment

template <bool VEC>
__device__ __forceinline__ void eqv_piece(const u64 *row, unsigned long long a0, bool on0, bool on1, u64 &w0, u64 &w1) {
  w0 = w1 = 0;
  if (VEC) {
    if (on0) {
      const u64x2 t = eq_ld2(row + a0);
      w0 = t.x;
      w1 = t.y;
    }
  } else {
    if (on0) w0 = eq_ld1(row + a0);
    if (on1) w1 = eq_ld1(row + a0 + 1);
  }
}

// Is some slot of `um` (slots of side a) without an equal (clock row, value) among the slots `nzb` of
// side b?  The whole wave; wave-uniform.
__device__ __forceinline__ bool eqv_unmatched(u64 um, const u64 *ar, const u64 *av, u64 nzb, const u64 *br, const u64 *bv,
                                              unsigned long long A, int lane) {
  while (um) {
    const int q = __builtin_ctzll(um);
    um &= um - 1;
    const u64 v = av[q];
    bool found = false;
    for (u64 t = nzb; t && !found; t &= t - 1) {
      const int j = __builtin_ctzll(t);
      if (bv[j] == v && eq_row_same(ar + (unsigned long long)q * A, br + (unsigned long long)j * A, A, lane)) found = true;
    }
    if (!found) return true;
  }
  return false;
}

template <int CH, bool VEC>
__global__ __launch_bounds__(kBlock) void eqv_reg_kernel(EqvPlan p) {
  const int lane = threadIdx.x % kWave;
  const unsigned G = 1u << p.lg, RPW = kWave >> p.lg;
  const unsigned g = lane & (G - 1), seg = lane >> p.lg;
  const unsigned long long A = p.A, KK = p.K * p.K2, NR = p.N * KK, Vx = p.x.Vs, Vy = p.y.Vs;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long ngroup = (NR + RPW - 1) / RPW;
  for (unsigned long long wv = wave0; wv < ngroup; wv += nwave) {  // wave-uniform
    const unsigned long long r = wv * RPW + seg;
    const bool live = r < NR;
    bool on0[CH], on1[CH];
    unsigned long long a0[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      a0[c] = 2ull * (g + (unsigned long long)G * c);
      on0[c] = live && a0[c] < A;
      on1[c] = live && a0[c] + 1 < A;
    }
    unsigned long long cx = 0, cy = 0;
    bool bad = false;
    if (live) {
      cx = p.x.nval[r];
      cy = p.y.nval[r];
      bad = cx > Vx || cy > Vy;
      if (bad) cx = cy = 0;  // nothing past a capacity is read
    }
    // inner entry row: bit 0 the rows differ, 1 / 2 the inner key is present in x / y
    unsigned e = 0;
    {
      const u64 *ex = p.x.iec + (live ? r : 0) * A, *ey = p.y.iec + (live ? r : 0) * A;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        u64 e0, e1, f0, f1;
        eqv_piece<VEC>(ex, a0[c], on0[c], on1[c], e0, e1);
        eqv_piece<VEC>(ey, a0[c], on0[c], on1[c], f0, f1);
        e |= (((e0 ^ f0) | (e1 ^ f1)) ? 1u : 0u) | ((e0 | e1) ? 2u : 0u) | ((f0 | f1) ? 4u : 0u);
      }
    }
    // slot q against slot q: non-empty in x, non-empty in y, (clock row, value) differ
    u64 nzx = 0, nzy = 0, dq = 0;
    const u64 *xr = p.x.ivc + (live ? r : 0) * Vx * A, *yr = p.y.ivc + (live ? r : 0) * Vy * A;
    const u64 *xv = p.x.ivv + (live ? r : 0) * Vx, *yv = p.y.ivv + (live ? r : 0) * Vy;
    const unsigned qn = (unsigned)(cx > cy ? cx : cy);
#pragma unroll 4
    for (unsigned q = 0; q < qn; ++q) {
      const bool lx = q < cx, ly = q < cy;
      u64 ox = 0, oy = 0, d = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        u64 t0, t1, u0, u1;
        eqv_piece<VEC>(xr + q * A, a0[c], on0[c] && lx, on1[c] && lx, t0, t1);
        eqv_piece<VEC>(yr + q * A, a0[c], on0[c] && ly, on1[c] && ly, u0, u1);
        ox |= t0 | t1;
        oy |= u0 | u1;
        d |= (t0 ^ u0) | (t1 ^ u1);
      }
      if (lx && ly && xv[q] != yv[q]) d = 1;
      if (ox) nzx |= 1ull << q;
      if (oy) nzy |= 1ull << q;
      if (d) dq |= 1ull << q;
    }
    for (unsigned off = 1; off < G; off <<= 1) {  // stays inside the segment
      e |= __shfl_xor(e, off, kWave);
      nzx |= __shfl_xor(nzx, off, kWave);
      nzy |= __shfl_xor(nzy, off, kWave);
      dq |= __shfl_xor(dq, off, kWave);
    }
    const u64 same = nzx & nzy & ~dq;
    const u64 ux = nzx & ~same, uy = nzy & ~same;  // slots not settled by slot q against slot q
    if (bad && g == 0) atomicOr(p.ne + r / KK, CRDT_NE_INVALID);
    // 1: the inner entry rows differ (the inner Maps differ); 2: both present, the set search decides
    int kind = (!live || bad) ? 0 : ((e & 1u) ? 1 : ((e & 6u) == 6u && (ux | uy)) ? 2 : 0);
    if (Vx <= kRegVM && Vy <= kRegVM && __any(kind == 2)) {
      // up to 8 slots a side: the search stays inside the segment, eq_reg_kernel's pair mask.  The
      // slots are loaded again (cache hits) so that the common path holds no slot in registers.
      const bool srch = kind == 2;
      u64 pm = 0;  // bit q * 8 + t: slot q of x and slot t of y differ in a word of this lane
      u64 vx[kRegVM], vy[kRegVM];
#pragma unroll
      for (int q = 0; q < kRegVM; ++q) {
        vx[q] = (srch && (unsigned long long)q < cx) ? xv[q] : 0;
        vy[q] = (srch && (unsigned long long)q < cy) ? yv[q] : 0;
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        u64 sx[kRegVM][2], sy[kRegVM][2];
#pragma unroll
        for (int q = 0; q < kRegVM; ++q) {
          const bool lx = srch && (unsigned long long)q < cx, ly = srch && (unsigned long long)q < cy;
          eqv_piece<VEC>(xr + q * A, a0[c], on0[c] && lx, on1[c] && lx, sx[q][0], sx[q][1]);
          eqv_piece<VEC>(yr + q * A, a0[c], on0[c] && ly, on1[c] && ly, sy[q][0], sy[q][1]);
        }
#pragma unroll
        for (int q = 0; q < kRegVM; ++q)
#pragma unroll
          for (int t = 0; t < kRegVM; ++t)
            if ((sx[q][0] ^ sy[t][0]) | (sx[q][1] ^ sy[t][1])) pm |= 1ull << (q * kRegVM + t);
      }
      for (unsigned off = 1; off < G; off <<= 1) pm |= __shfl_xor(pm, off, kWave);
      if (srch) {
        unsigned fx = 0, fy = 0;  // slots with an equal (clock row, value) on the other side
#pragma unroll
        for (int q = 0; q < kRegVM; ++q)
#pragma unroll
          for (int t = 0; t < kRegVM; ++t)
            if (((nzx >> q) & 1u) && ((nzy >> t) & 1u) && !((pm >> (q * kRegVM + t)) & 1ull) && vx[q] == vy[t]) {
              fx |= 1u << q;
              fy |= 1u << t;
            }
        kind = ((nzx & ~(u64)fx) | (nzy & ~(u64)fy)) ? 1 : 0;
      }
    }
    u64 todo = __ballot(kind != 0 && g == 0);
    while (todo) {  // such a register takes the whole wave
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1;
      const unsigned long long rr = __shfl(r, b, kWave);
      bool ne = true;
      if (__shfl(kind, b, kWave) == 2) {
        const u64 bux = __shfl(ux, b, kWave), buy = __shfl(uy, b, kWave), bzx = __shfl(nzx, b, kWave),
                  bzy = __shfl(nzy, b, kWave);
        const u64 *ar = p.x.ivc + rr * Vx * A, *br = p.y.ivc + rr * Vy * A;
        const u64 *av = p.x.ivv + rr * Vx, *bv = p.y.ivv + rr * Vy;
        ne = eqv_unmatched(bux, ar, av, bzy, br, bv, A, lane) || eqv_unmatched(buy, br, bv, bzx, ar, av, A, lane);
      }
      if (!ne) continue;
      const unsigned long long key = rr / p.K2, s = key / p.K, k = key - s * p.K;
      // hidden unless the outer key is present on both sides (one side only: the key kernel decided)
      if (eqv_both_present(p, s, k, lane) && lane == 0) atomicOr(p.ne + s, CRDT_NE_VALUES);
    }
  }
}

// ---- launches --------------------------------------------------------------------------------------
static bool eqv_al16(const void *p) { return (uintptr_t)p % 16 == 0; }
static bool eqv_even(unsigned long long a, unsigned long long b = 0, unsigned long long c = 0, unsigned long long d = 0) {
  return ((a | b | c | d) & 1) == 0;
}

template <bool NESTED>
static void launch_eqv_key(crdt_ctx *ctx, EqvPlan p, bool vec) {
  const unsigned long long NK = p.N * p.K, pieces = (p.A + p.v0n + p.v1n + 1) / 2;
  unsigned grid;
  if (pieces > 1024 && !NESTED) {
    p.lg = 8;
    grid = (unsigned)std::min<unsigned long long>(NK, (unsigned long long)ctx->cu_count * 32);
  } else {
    p.lg = row_lr_log(pieces, ctx->tune.eqv_ppl);
    // ... but at least 8 lanes a key while a lane keeps 2 pieces: at 512 bytes a side (K 1,024 x W 1 x
    // A 32) 4 lanes x 8 pieces reach 72% of 8 TB/s, 8 x 4 79%, 16 x 2 76% (profiles/eq_vmap_ab.log)
    while (p.lg < 3 && (4ull << p.lg) <= pieces) ++p.lg;
    const unsigned long long rpw = kWave >> p.lg, waves = (NK + rpw - 1) / rpw;
    grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                  (unsigned long long)ctx->cu_count * ctx->tune.eqv_bpc);
  }
  if (vec) hipLaunchKernelGGL((eqv_key_kernel<true, NESTED>), dim3(grid), dim3(kBlock), 0, ctx->stream, p);
  else hipLaunchKernelGGL((eqv_key_kernel<false, NESTED>), dim3(grid), dim3(kBlock), 0, ctx->stream, p);
}

static void launch_eqv_list(crdt_ctx *ctx, const EqvPlan &p) {
  const unsigned long long waves = (p.N * p.K + kWave - 1) / kWave;
  const unsigned grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                               (unsigned long long)ctx->cu_count * 32);
  hipLaunchKernelGGL(eqv_list_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, p);
}

static void launch_eqv_reg(crdt_ctx *ctx, EqvPlan p, bool vec) {
  const unsigned long long NR = p.N * p.K * p.K2;
  int lg = 0;  // lanes per register: the 16-byte pieces of a row, rounded up to a power of two
  while ((1u << lg) < (p.A + 1) / 2 && lg < 6) ++lg;
  p.lg = lg;
  const unsigned long long rpw = kWave >> lg, waves = (NR + rpw - 1) / rpw;
  const unsigned grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                               (unsigned long long)ctx->cu_count * ctx->tune.eqv_bpc);
  hipStream_t s = ctx->stream;
  if (p.A > 128) {
    if (vec) hipLaunchKernelGGL((eqv_reg_kernel<2, true>), dim3(grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((eqv_reg_kernel<2, false>), dim3(grid), dim3(kBlock), 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((eqv_reg_kernel<1, true>), dim3(grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((eqv_reg_kernel<1, false>), dim3(grid), dim3(kBlock), 0, s, p);
  }
}

// what the three calls share: the Map's clock row first, the Map-level lists (and the INVALID rule) last
struct EqvDef {
  const uint32_t *xc, *yc;
  size_t xcap, ycap;
};
static int eqv_deferred_args(crdt_ctx *ctx, const char *what, const crdt_map_deferred *xd, const crdt_map_deferred *yd,
                             size_t A, size_t Kw, EqvDef &d) {
  for (const crdt_map_deferred *df : {xd, yd})
    if (df && df->Dcap && (!df->count || (A && !df->clock) || (Kw && !df->keys)))
      return fail(ctx, CRDT_EINVAL, "%s: NULL deferred buffers with Dcap > 0", what);
  d.xc = xd ? xd->count : nullptr;  // read whenever given
  d.yc = yd ? yd->count : nullptr;
  d.xcap = xd ? xd->Dcap : 0;
  d.ycap = yd ? yd->Dcap : 0;
  return CRDT_OK;
}
static void launch_eqv_clock(crdt_ctx *ctx, const u64 *xclock, size_t xcs, const u64 *yclock, size_t ycs, const EqvDef &d,
                             size_t N, size_t A, uint32_t *ne) {
  EqDensePlan c{};
  c.x = EqDenseSide{xclock, xcs, nullptr, 0, 0, d.xc, d.xcap};
  c.y = EqDenseSide{yclock, ycs, nullptr, 0, 0, d.yc, d.ycap};
  c.N = N;
  c.A = A;
  c.ne = ne;
  launch_eq_dense(ctx, c);
}
static void launch_eqv_deferred(crdt_ctx *ctx, const crdt_map_deferred *xd, const crdt_map_deferred *yd, const EqvDef &d,
                                size_t N, size_t A, size_t Kw, uint32_t *ne) {
  EqDefPlan q{};
  q.x = EqDefSide{d.xcap ? (const u64 *)xd->clock : nullptr, d.xcap ? (const u64 *)xd->keys : nullptr, d.xc, d.xcap};
  q.y = EqDefSide{d.ycap ? (const u64 *)yd->clock : nullptr, d.ycap ? (const u64 *)yd->keys : nullptr, d.yc, d.ycap};
  q.N = N;
  q.A = A;
  q.W = Kw;
  q.ne = ne;
  q.norm = 1;
  launch_eq_deferred(ctx, q);
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_map_counter_eq_batch(crdt_ctx *ctx, const crdt_map_counter_states *x, const crdt_map_deferred *xd,
                              const crdt_map_counter_states *y, const crdt_map_deferred *yd, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  const char *what = "map_counter_eq_batch";
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "%s: NULL states", what);
  if (x->N != y->N || x->K != y->K || x->A != y->A || x->W != y->W)
    return fail(ctx, CRDT_EINVAL, "%s: x and y differ in N, K, A or W", what);
  const size_t N = x->N, K = x->K, A = x->A, W = x->W, Kw = (K + 63) / 64;
  if (N == 0) return CRDT_OK;
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu > 1024 actors", what, A);
  if (W != 1 && W != 2) return fail(ctx, CRDT_EUNSUPPORTED, "%s: W = %zu not 1 or 2", what, W);
  for (const crdt_map_counter_states *st : {x, y}) {
    if (A && (!st->clock || (K && (!st->ec || !st->val)))) return fail(ctx, CRDT_EINVAL, "%s: NULL state buffers", what);
    if (N > 1 && (st->clock_stride < A || st->ec_stride < K * A || st->val_stride < K * W * A))
      return fail(ctx, CRDT_EINVAL, "%s: strides below the state size", what);
  }
  EqvDef d{};
  if (int rc = eqv_deferred_args(ctx, what, xd, yd, A, Kw, d)) return rc;
  if (!ne) return fail(ctx, CRDT_EINVAL, "%s: NULL ne", what);
  if (N > 0x7fffffffULL || (K && N > 0x7fffffffULL / K)) return fail(ctx, CRDT_EUNSUPPORTED, "%s: N * K too large", what);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "map_counter_eq");  // the bracket covers every launch of the call
  launch_eqv_clock(ctx, (const u64 *)x->clock, x->clock_stride, (const u64 *)y->clock, y->clock_stride, d, N, A, ne);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && K && A) {
    EqvPlan p{};
    p.x.ec = (const u64 *)x->ec, p.x.es = x->ec_stride, p.x.v0 = (const u64 *)x->val, p.x.v0s = x->val_stride, p.x.v0k = W * A;
    p.y.ec = (const u64 *)y->ec, p.y.es = y->ec_stride, p.y.v0 = (const u64 *)y->val, p.y.v0s = y->val_stride, p.y.v0k = W * A;
    p.N = N, p.K = K, p.A = A, p.v0n = W * A, p.ne = ne;
    const bool vec = A % 2 == 0 && eqv_al16(x->ec) && eqv_al16(y->ec) && eqv_al16(x->val) && eqv_al16(y->val) &&
                     (N == 1 || eqv_even(x->ec_stride, y->ec_stride, x->val_stride, y->val_stride));
    launch_eqv_key<false>(ctx, p, vec);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_eqv_deferred(ctx, xd, yd, d, N, A, Kw, ne);
    e = hipGetLastError();
  }
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "map_counter_eq_batch kernel launch");
  return CRDT_OK;
}

int crdt_map_orswot_eq_batch(crdt_ctx *ctx, const crdt_map_orswot_states *x, const crdt_map_deferred *xd,
                             const crdt_map_orswot_states *y, const crdt_map_deferred *yd, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  const char *what = "map_orswot_eq_batch";
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "%s: NULL states", what);
  if (x->N != y->N || x->K != y->K || x->M != y->M || x->A != y->A)
    return fail(ctx, CRDT_EINVAL, "%s: x and y differ in N, K, M or A", what);
  const size_t N = x->N, K = x->K, M = x->M, A = x->A, Kw = (K + 63) / 64, Mw = M > 64 ? (M + 63) / 64 : 1;
  if (N == 0) return CRDT_OK;
  if (A > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu > 1024 actors", what, A);
  if (M > 1024) return fail(ctx, CRDT_EUNSUPPORTED, "%s: M = %zu > 1024 members", what, M);
  for (const crdt_map_orswot_states *st : {x, y}) {
    if (A && (!st->clock || (K && (!st->ec || !st->oc || (M && !st->ent)))))
      return fail(ctx, CRDT_EINVAL, "%s: NULL state buffers", what);
    if (K && (!st->vd_n || (A && !st->vd_clock) || !st->vd_mem)) return fail(ctx, CRDT_EINVAL, "%s: NULL nested lists", what);
  }
  EqvDef d{};
  if (int rc = eqv_deferred_args(ctx, what, xd, yd, A, Kw, d)) return rc;
  if (!ne) return fail(ctx, CRDT_EINVAL, "%s: NULL ne", what);
  if (N > 0x7fffffffULL || (K && N > 0x7fffffffULL / K)) return fail(ctx, CRDT_EUNSUPPORTED, "%s: N * K too large", what);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "map_orswot_eq");  // the bracket covers every launch of the call
  launch_eqv_clock(ctx, (const u64 *)x->clock, A, (const u64 *)y->clock, A, d, N, A, ne);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && K && A) {
    EqvPlan p{};
    bool vec = A % 2 == 0;
    for (int side = 0; side < 2; ++side) {
      const crdt_map_orswot_states *st = side ? y : x;
      EqvSide &q = side ? p.y : p.x;
      q.ec = (const u64 *)st->ec, q.es = K * A;
      q.v0 = (const u64 *)st->oc, q.v0s = K * A, q.v0k = A;
      q.v1 = (const u64 *)st->ent, q.v1s = K * M * A, q.v1k = M * A;
      q.ln = st->vd_n, q.lclk = (const u64 *)st->vd_clock, q.lset = (const u64 *)st->vd_mem, q.lcap = st->Vd ? st->Vd : 16;
      vec = vec && eqv_al16(st->ec) && eqv_al16(st->oc) && eqv_al16(st->ent);
    }
    p.N = N, p.K = K, p.A = A, p.v0n = A, p.v1n = M * A, p.LW = Mw, p.ne = ne;
    launch_eqv_key<false>(ctx, p, vec);
    e = hipGetLastError();
    if (e == hipSuccess) {
      launch_eqv_list(ctx, p);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    launch_eqv_deferred(ctx, xd, yd, d, N, A, Kw, ne);
    e = hipGetLastError();
  }
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "map_orswot_eq_batch kernel launch");
  return CRDT_OK;
}

int crdt_map_nested_eq_batch(crdt_ctx *ctx, const crdt_map_nested_states *x, const crdt_map_deferred *xd,
                             const crdt_map_nested_states *y, const crdt_map_deferred *yd, uint32_t *ne) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  const char *what = "map_nested_eq_batch";
  if (!x || !y) return fail(ctx, CRDT_EINVAL, "%s: NULL states", what);
  if (x->N != y->N || x->K != y->K || x->K2 != y->K2 || x->A != y->A)
    return fail(ctx, CRDT_EINVAL, "%s: x and y differ in N, K, K2 or A", what);
  const size_t N = x->N, K = x->K, K2 = x->K2, A = x->A, Kw = (K + 63) / 64, K2w = K2 > 64 ? (K2 + 63) / 64 : 1;
  if (N == 0) return CRDT_OK;
  if (A > 256) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu > 256 actors", what, A);
  if (K2 > 256) return fail(ctx, CRDT_EUNSUPPORTED, "%s: K2 = %zu > 256 inner keys", what, K2);
  for (const crdt_map_nested_states *st : {x, y}) {
    if ((st->Vs ? st->Vs : 8) > 64) return fail(ctx, CRDT_EUNSUPPORTED, "%s: Vs = %zu > 64 register slots", what, st->Vs);
    if (A && (!st->clock || (K && (!st->ec || !st->ic || (K2 && (!st->iec || !st->ivc || !st->ivv || !st->nval))))))
      return fail(ctx, CRDT_EINVAL, "%s: NULL state buffers", what);
    if (K && (!st->id_n || (A && !st->id_clock) || !st->id_keys)) return fail(ctx, CRDT_EINVAL, "%s: NULL inner lists", what);
  }
  EqvDef d{};
  if (int rc = eqv_deferred_args(ctx, what, xd, yd, A, Kw, d)) return rc;
  if (!ne) return fail(ctx, CRDT_EINVAL, "%s: NULL ne", what);
  if (N > 0x7fffffffULL || (K && N > 0x7fffffffULL / K) || (K && K2 && N * K > 0x7fffffffULL / K2))
    return fail(ctx, CRDT_EUNSUPPORTED, "%s: N * K * K2 too large", what);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "map_nested_eq");  // the bracket covers every launch of the call
  launch_eqv_clock(ctx, (const u64 *)x->clock, A, (const u64 *)y->clock, A, d, N, A, ne);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && K && A) {
    EqvPlan p{};
    bool vec = A % 2 == 0, rvec = A % 2 == 0;
    for (int side = 0; side < 2; ++side) {
      const crdt_map_nested_states *st = side ? y : x;
      EqvSide &q = side ? p.y : p.x;
      q.ec = (const u64 *)st->ec, q.es = K * A;
      q.v0 = (const u64 *)st->ic, q.v0s = K * A, q.v0k = A;
      q.ln = st->id_n, q.lclk = (const u64 *)st->id_clock, q.lset = (const u64 *)st->id_keys, q.lcap = st->Id ? st->Id : 16;
      q.iec = (const u64 *)st->iec, q.ivc = (const u64 *)st->ivc, q.ivv = (const u64 *)st->ivv, q.nval = st->nval;
      q.Vs = st->Vs ? st->Vs : 8;
      vec = vec && eqv_al16(st->ec) && eqv_al16(st->ic);
      rvec = rvec && eqv_al16(st->iec) && eqv_al16(st->ivc);
    }
    p.N = N, p.K = K, p.A = A, p.v0n = A, p.LW = K2w, p.K2 = K2, p.ne = ne;
    launch_eqv_key<true>(ctx, p, vec);
    e = hipGetLastError();
    if (e == hipSuccess) {
      launch_eqv_list(ctx, p);
      e = hipGetLastError();
    }
    if (e == hipSuccess && K2) {
      launch_eqv_reg(ctx, p, rvec);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    launch_eqv_deferred(ctx, xd, yd, d, N, A, Kw, ne);
    e = hipGetLastError();
  }
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "map_nested_eq_batch kernel launch");
  return CRDT_OK;
}

}  // extern "C"
