// Shared by the batched ReadCtx gathers (read.hip, read_vmap.hip): one wave per query under a
// grid-stride loop, and the row helpers a query uses.
#pragma once
#include "common.hpp"

namespace crdt {

#define QUERY_WAVE_LOOP(Q)                                                                          \
  const int lane = threadIdx.x % kWave;                                                             \
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;   \
  const unsigned long long nw = (unsigned long long)gridDim.x * (kBlock / kWave);                   \
  for (unsigned long long q = w0; q < (Q); q += nw)

static inline unsigned query_grid(const crdt_ctx *ctx, unsigned long long Q) {
  const unsigned long long want = (Q + kBlock / kWave - 1) / (kBlock / kWave);
  const unsigned long long cap = (unsigned long long)ctx->cu_count * 8;
  return (unsigned)(want < cap ? want : cap);
}

// dst[0..A) = src ? src[0..A) : 0; returns (wave-uniform) whether any copied word is non-zero.
__device__ __forceinline__ bool copy_row(u64 *dst, const u64 *src, unsigned long long A, int lane) {
  bool nz = false;
  for (unsigned long long a = lane; a < A; a += kWave) {
    const u64 v = src ? src[a] : 0;
    dst[a] = v;
    nz |= v != 0;
  }
  return __ballot(nz) != 0;
}

__device__ __forceinline__ bool row_nonzero(const u64 *src, unsigned long long A, int lane) {
  bool nz = false;
  for (unsigned long long a = lane; a < A; a += kWave) nz |= src[a] != 0;
  return __ballot(nz) != 0;
}

}  // namespace crdt
