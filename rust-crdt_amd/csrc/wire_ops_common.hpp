// Shared by the op-stream wire kernels (wire_ops.hip: Orswot and Map<K, MVReg> ops; wire_vmap_ops.hip:
// the value-typed Maps' ops; wire_mvreg.hip: the standalone MVReg's Puts): the frame walk's reader and
// the wave prefix sum of the egress.
#pragma once
#include "wire_driver.hpp"

namespace crdt {

// MapWalk reads forward and expects the window it loads to be in flight already.  An op's id list
// is skipped, not read, so the walk can land past everything issued: restart the ring there.
struct OpWalk : MapWalk<> {
  __device__ void seek(unsigned long long k, int lane) {
    const unsigned long long wi = uni64(k) / kWalkWin;
    if (wi != uni64(cur) && wi >= uni64(issued)) {
      wire_vmcnt<0>();  // nothing of the windows skipped may land in a slot after it is reissued
      issued = wi;
      while (issued < nwin && issued < wi + kWalkRing) {
        dma(issued, lane);
        issued = uni64(issued + 1);
      }
    }
  }
  __device__ uint32_t at(unsigned long long k, int lane) {
    seek(k, lane);
    return get(k, lane);
  }
  __device__ u64 at64(unsigned long long k, int lane) { return (u64)at(k, lane) | ((u64)at(k + 1, lane) << 32); }
};

// Exclusive prefix sum over the wave's lanes (egress: where each op of a batch of 64 starts); total
// = the wave's sum.
__device__ __forceinline__ u64 wave_excl(u64 v, int lane, u64 &total) {
  u64 x = v;
  for (int d = 1; d < kWave; d <<= 1) {
    const u64 y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  total = __shfl(x, kWave - 1, kWave);
  return x - v;
}

}  // namespace crdt
