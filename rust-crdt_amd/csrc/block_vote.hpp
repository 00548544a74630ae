// Workgroup-wide AND / OR of a handful of 64-bit words: the vote round of the workgroup-per-key folds
// (map_wide.hip, map_deep.hip, the deep MVReg fold of mvreg.hip).
#pragma once

#include "common.hpp"

namespace crdt {

// Block-wide AND / OR of NA + NO 64-bit words: wave shuffles, then one word set per wave in LDS.
// Every thread gets the result.  `red` holds 4 waves * (NA + NO) words.
template <int NA, int NO>
__device__ __forceinline__ void wide_vote(u64 (&a)[NA > 0 ? NA : 1], u64 (&o)[NO > 0 ? NO : 1], u64 *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int w = 0; w < NA; ++w) a[w] &= __shfl_xor(a[w], off, 64);
#pragma unroll
    for (int w = 0; w < NO; ++w) o[w] |= __shfl_xor(o[w], off, 64);
  }
  const int nw = blockDim.x / 64, wv = threadIdx.x / 64;
  if (nw == 1) return;
  constexpr int NWD = NA + NO;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int w = 0; w < NA; ++w) red[wv * NWD + w] = a[w];
#pragma unroll
    for (int w = 0; w < NO; ++w) red[wv * NWD + NA + w] = o[w];
  }
  __syncthreads();
  for (int x = 0; x < nw; ++x) {
#pragma unroll
    for (int w = 0; w < NA; ++w) a[w] &= red[x * NWD + w];
#pragma unroll
    for (int w = 0; w < NO; ++w) o[w] |= red[x * NWD + NA + w];
  }
  __syncthreads();  // red may be reused by the next round
}

// single-flag forms
__device__ __forceinline__ bool wide_all(bool t, u64 *red) {
  u64 a[1] = {t ? 1ull : 0ull}, o[1] = {0};
  wide_vote<1, 0>(a, o, red);
  return a[0] != 0;
}
__device__ __forceinline__ bool wide_any(bool t, u64 *red) {
  u64 a[1] = {~0ull}, o[1] = {t ? 1ull : 0ull};
  wide_vote<0, 1>(a, o, red);
  return o[0] != 0;
}

}  // namespace crdt
