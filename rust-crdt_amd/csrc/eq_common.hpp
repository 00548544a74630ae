// Shared by the batched state-equality kernels (eq.hip: MVReg, Orswot, Map<K, MVReg>; eq_vmap.hip: the
// value-typed Maps): the non-temporal loads, the plans of the clock / deferred kernels with their
// launches (defined in eq.hip), and the exact compare of two deferred-remove lists as maps
// rm clock -> set, which the Map-level lists and the value-typed Maps' nested lists both use.
#pragma once

#include "common.hpp"

namespace crdt {

__device__ __forceinline__ u64x2 eq_ld2(const u64 *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p));
}
__device__ __forceinline__ u64 eq_ld1(const u64 *p) { return __builtin_nontemporal_load(p); }

// ---- clock and entry rows --------------------------------------------------------------------------
struct EqDenseSide {
  const u64 *clock;
  unsigned long long cs;
  const u64 *rows;
  unsigned long long rs, ss;  // row stride, state stride
  const uint32_t *cnt;        // def_count or NULL
  unsigned long long dcap;
};
struct EqDensePlan {
  EqDenseSide x, y;
  unsigned long long N, A, R, L;  // R rows of L words per state
  uint32_t *ne;
  int lg;  // log2 of the lanes per state; 8: one workgroup per state
};

// ---- deferred removes ------------------------------------------------------------------------------
struct EqDefSide {
  const u64 *clock, *sets;
  const uint32_t *cnt;
  unsigned long long dcap;
};
struct EqDefPlan {
  EqDefSide x, y;
  unsigned long long N, A, W;
  uint32_t *ne;
  int norm;  // a word that already carries CRDT_NE_INVALID (a per-key owner's) becomes INVALID alone
};
constexpr int kDefWin = 128;  // row hashes kept in LDS per side
constexpr int kDefAcc = 4;    // set words per lane of one union pass (64 * 4 words = 16,384 members / keys)

// ne[s] by a plain store: CLOCK | ENTRIES, or INVALID alone on a bad def_count
void launch_eq_dense(crdt_ctx *ctx, EqDensePlan p);
// one owner per state ORs DEFERRED into ne[s]
void launch_eq_deferred(crdt_ctx *ctx, const EqDefPlan &p);

__device__ __forceinline__ u64 eq_mix64(u64 z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}
// the whole wave hashes one row; every lane gets the hash
__device__ __forceinline__ u64 eq_row_hash(const u64 *r, unsigned long long A, int lane) {
  u64 h = 0;
  for (unsigned long long a = lane; a < A; a += kWave) h += eq_mix64(r[a] + 0x9e3779b97f4a7c15ull * (a + 1));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, kWave);
  return h;
}
__device__ __forceinline__ bool eq_row_same(const u64 *r, const u64 *q, unsigned long long A, int lane) {
  u64 d = 0;
  for (unsigned long long a = lane; a < A; a += kWave) d |= r[a] ^ q[a];
  return __ballot(d != 0) == 0;
}
// f(j) for every slot j < n of a side whose clock row equals r (hash h): wave-uniform
template <class F>
__device__ __forceinline__ void eq_for_matches(const u64 *r, u64 h, const u64 *sc, const u64 *sh, unsigned n,
                                               unsigned long long A, int lane, F &&f) {
  const unsigned lim = n < (unsigned)kDefWin ? n : (unsigned)kDefWin;
  for (unsigned base = 0; base < lim; base += kWave) {
    const unsigned j = base + lane;
    u64 m = __ballot(j < lim && sh[j < lim ? j : 0] == h);
    while (m) {
      const unsigned jj = base + __builtin_ctzll(m);
      m &= m - 1;
      if (eq_row_same(r, sc + (unsigned long long)jj * A, A, lane)) f(jj);
    }
  }
  for (unsigned jj = lim; jj < n; ++jj)
    if (eq_row_same(r, sc + (unsigned long long)jj * A, A, lane)) f(jj);
}

// One wave: do the lists x (nx slots: clock rows xc [nx][A], sets xm [nx][W]) and y differ as maps
// rm clock -> set?  nx and ny are within their capacities and not both 0.  hx / hy: kDefWin words of LDS
// each, this wave's own.  Equal counts with slot-by-slot identical rows are equal (one streaming
// compare).  Otherwise clocks are matched through per-slot 64-bit row hashes in LDS (the first kDefWin
// slots of each side; the slots past them are compared row by row in memory), the sets of equal clocks
// are unioned per side and the unions compared; a clock of one side missing on the other is unequal
// whatever its set.  The result is wave-uniform.
__device__ __forceinline__ bool eq_deferred_pair(const u64 *xc, const u64 *xm, unsigned nx, const u64 *yc, const u64 *ym,
                                                 unsigned ny, unsigned long long A, unsigned long long W, int lane,
                                                 u64 *hx, u64 *hy) {
  bool ne = nx == 0 || ny == 0;
  bool done = ne;
  if (!done && nx == ny) {  // the same slots in the same order
    u64 d = 0;
    for (unsigned long long a = lane; a < nx * A; a += kWave) d |= xc[a] ^ yc[a];
    for (unsigned long long a = lane; a < nx * W; a += kWave) d |= xm[a] ^ ym[a];
    done = __ballot(d != 0) == 0;
  }
  if (!done) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the previous list's reads of hx / hy
    for (unsigned j = 0; j < nx && j < (unsigned)kDefWin; ++j) {
      const u64 h = eq_row_hash(xc + (unsigned long long)j * A, A, lane);
      if (lane == 0) hx[j] = h;
    }
    for (unsigned j = 0; j < ny && j < (unsigned)kDefWin; ++j) {
      const u64 h = eq_row_hash(yc + (unsigned long long)j * A, A, lane);
      if (lane == 0) hy[j] = h;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    // every clock of x is a clock of y, and the unions of their sets agree
    for (unsigned i = 0; i < nx && !ne; ++i) {
      const u64 *ri = xc + (unsigned long long)i * A;
      const u64 h = i < (unsigned)kDefWin ? hx[i] : eq_row_hash(ri, A, lane);
      unsigned long long cb = 0;
      do {
        u64 ux[kDefAcc], uy[kDefAcc];
#pragma unroll
        for (int q = 0; q < kDefAcc; ++q) ux[q] = uy[q] = 0;
        bool fy = false;
        eq_for_matches(ri, h, xc, hx, nx, A, lane, [&](unsigned j) {
#pragma unroll
          for (int q = 0; q < kDefAcc; ++q) {
            const unsigned long long w = cb + (unsigned long long)q * kWave + lane;
            if (w < W) ux[q] |= xm[(unsigned long long)j * W + w];
          }
        });
        eq_for_matches(ri, h, yc, hy, ny, A, lane, [&](unsigned j) {
          fy = true;
#pragma unroll
          for (int q = 0; q < kDefAcc; ++q) {
            const unsigned long long w = cb + (unsigned long long)q * kWave + lane;
            if (w < W) uy[q] |= ym[(unsigned long long)j * W + w];
          }
        });
        u64 d = 0;
#pragma unroll
        for (int q = 0; q < kDefAcc; ++q) d |= ux[q] ^ uy[q];
        if (!fy || __ballot(d != 0) != 0) ne = true;
        cb += (unsigned long long)kDefAcc * kWave;
      } while (cb < W && !ne);
    }
    // every clock of y is a clock of x
    for (unsigned j = 0; j < ny && !ne; ++j) {
      const u64 *rj = yc + (unsigned long long)j * A;
      const u64 h = j < (unsigned)kDefWin ? hy[j] : eq_row_hash(rj, A, lane);
      bool fx = false;
      eq_for_matches(rj, h, xc, hx, nx, A, lane, [&](unsigned) { fx = true; });
      if (!fx) ne = true;
    }
  }
  return ne;
}

}  // namespace crdt
