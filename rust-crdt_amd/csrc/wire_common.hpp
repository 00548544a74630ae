// Shared pieces of the serde wire kernels (wire.hip: the reference types and Map<K, MVReg>;
// wire_vmap.hip: the value-typed Maps; wire_ops.hip: op streams; wire_mvreg.hip: MVReg on its own): frame access, dictionary lookups, VClock parse / write.
// The encoding (bincode 1.x, default options) is restated at the top of wire.hip.
#pragma once
#include "common.hpp"

namespace crdt {

constexpr int kScanItems = 1024;  // items per block of the exclusive scan (wire.hip)

constexpr unsigned kWireBad = 1u, kWireMissing = 2u, kWireCap = 4u;
constexpr int kWireRowLds = 4096;  // u64 words of the LDS row per wave (A or bitmap words)

struct Frame {
  const uint32_t *w;  // 4-aligned base
  unsigned long long nw;  // words in the frame
};

__device__ __forceinline__ u64 rd64(const uint32_t *w, unsigned long long k) {
  return (u64)w[k] | ((u64)w[k + 1] << 32);
}

__device__ __forceinline__ long long find_u32(const uint32_t *dict, unsigned long long n, uint32_t id,
                                              unsigned long long hint) {
  if (hint < n && dict[hint] == id) return (long long)hint;  // the dense, in-order case
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = (lo + hi) / 2;
    if (dict[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && dict[lo] == id) ? (long long)lo : -1;
}
__device__ __forceinline__ long long find_u64(const u64 *dict, unsigned long long n, u64 id, unsigned long long hint) {
  if (hint < n && dict[hint] == id) return (long long)hint;
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = (lo + hi) / 2;
    if (dict[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && dict[lo] == id) ? (long long)lo : -1;
}

__device__ __forceinline__ void wfence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// Parse the VClock at word k of frame f into the LDS row (A u64, zeroed here); returns the word
// after it (or ~0 on a truncated clock).  st |= kWireMissing for an actor not in the dictionary.
__device__ inline unsigned long long parse_vclock(const Frame &f, unsigned long long k, const uint32_t *actors,
                                           unsigned long long A, u64 *row, int lane, unsigned &st) {
  for (unsigned long long a = lane; a < A; a += kWave) row[a] = 0;
  wfence();
  if (k + 2 > f.nw) {
    st |= kWireBad;
    return ~0ull;
  }
  const u64 n = rd64(f.w, k);
  if (n > (f.nw - k - 2) / 3) {
    st |= kWireBad;
    return ~0ull;
  }
  const uint32_t *rec = f.w + k + 2;
  bool miss = false;
  for (unsigned long long i = lane; i < n; i += kWave) {
    const uint32_t id = rec[3 * i];
    const u64 cnt = rd64(rec, 3 * i + 1);
    const long long col = find_u32(actors, A, id, i);
    if (col < 0) miss = true;
    else row[col] = cnt;
  }
  if (__ballot(miss)) st |= kWireMissing;
  wfence();
  return k + 2 + 3 * n;
}

template <typename T>
__device__ __forceinline__ void store_row(u64 *dst, const u64 *row, unsigned long long W, int lane) {
  for (unsigned long long a = lane; a < W; a += kWave) dst[a] = row[a];
}

// nonzero words of a row: one ballot per 64 words (no shuffle-reduction chain; the count is uniform)
__device__ __forceinline__ u64 nnz_row(const u64 *r, unsigned long long A, int lane) {
  unsigned long long c = 0;
  for (unsigned long long a0 = 0; a0 < A; a0 += kWave) {
    const unsigned long long a = a0 + lane;
    c += __popcll(__ballot(a < A && r[a] != 0));
  }
  return c;
}
__device__ __forceinline__ u64 popc_row(const u64 *r, unsigned long long W, int lane) {
  unsigned long long c = 0;
  for (unsigned long long w = lane; w < W; w += kWave) c += __popcll(r[w]);
  for (int off = kWave / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
  return c;
}
__device__ __forceinline__ void wr64(uint32_t *w, unsigned long long k, u64 v) {
  w[k] = (uint32_t)v;
  w[k + 1] = (uint32_t)(v >> 32);
}

// Write a dense row as a VClock at word k (len, then (actor, counter) ascending); returns the
// next word.  Lanes take columns; a wave prefix count gives every nonzero its record slot.
__device__ inline unsigned long long write_vclock(uint32_t *w, unsigned long long k, const u64 *r, unsigned long long A,
                                           const uint32_t *actors, int lane) {
  const u64 n = nnz_row(r, A, lane);
  if (lane == 0) wr64(w, k, n);
  unsigned long long base = 0;
  for (unsigned long long a0 = 0; a0 < A; a0 += kWave) {
    const unsigned long long a = a0 + lane;
    const u64 v = a < A ? r[a] : 0;
    const u64 m = __ballot(v != 0);
    if (v != 0) {
      const unsigned long long i = base + __popcll(m & ((1ull << lane) - 1));
      w[k + 2 + 3 * i] = actors[a];
      wr64(w, k + 3 + 3 * i, v);
    }
    base += __popcll(m);
  }
  return k + 2 + 3 * n;
}

// ---- MVReg<u64, u32> = u64 m, m x (VClock, u64 val) (mvreg.rs:32-35) -------------------------------
// The register of a Map entry (wire.hip) and a whole MVReg frame (wire_mvreg.hip) share these.
//
// Parse the register at word k: every value's clock goes through the LDS row, then put(v, val)
// runs (wave-uniform, the row landed) and decides what becomes of value v.  Returns the word after
// the register, or ~0 with st |= kWireBad on a truncated one.
template <class F>
__device__ __forceinline__ unsigned long long parse_mvreg(const Frame &f, unsigned long long k, const uint32_t *actors,
                                                          unsigned long long A, u64 *row, int lane, unsigned &st,
                                                          F &&put) {
  if (k + 2 > f.nw) {
    st |= kWireBad;
    return ~0ull;
  }
  const u64 m = rd64(f.w, k);
  k += 2;
  for (u64 v = 0; v < m; ++v) {
    k = parse_vclock(f, k, actors, A, row, lane, st);
    if (k == ~0ull || k + 2 > f.nw) {
      st |= kWireBad;
      return ~0ull;
    }
    const u64 val = rd64(f.w, k);
    k += 2;
    put(v, val);
    wfence();
  }
  return k;
}

// Bytes of the occupied slots' records (VClock, u64 val) of the V dense slots at vclk; m = how many
__device__ __forceinline__ u64 mvreg_wire_size(const u64 *vclk, unsigned long long V, unsigned long long A, int lane,
                                               u64 &m) {
  u64 vsz = 0;
  m = 0;
  for (unsigned long long v = 0; v < V; ++v) {
    const u64 nv = nnz_row(vclk + v * A, A, lane);
    if (nv) {
      ++m;
      vsz += 8 + 12 * nv + 8;
    }
  }
  return vsz;
}

// Write the register at word k: u64 m, then the occupied slots in slot (Vec) order; returns the next word.
__device__ inline unsigned long long write_mvreg(uint32_t *w, unsigned long long k, const u64 *vclk, const u64 *vval,
                                                 unsigned long long V, unsigned long long A, const uint32_t *actors,
                                                 u64 m, int lane) {
  if (lane == 0) wr64(w, k, m);
  k += 2;
  for (unsigned long long v = 0; v < V; ++v) {
    const u64 *vr = vclk + v * A;
    if (nnz_row(vr, A, lane) == 0) continue;
    k = write_vclock(w, k, vr, A, actors, lane);
    if (lane == 0) wr64(w, k, vval[v]);
    k += 2;
  }
  return k;
}

// ---- the walk's frame reader (wire.hip "walk + batched parse"; wire_ops.hip) ----------------------
// The frame streams through a per-wave LDS ring of RING windows by LDS-DMA, issued RING windows
// ahead of the walk; the current window sits in four registers per lane, so a word the walk reads
// costs a readlane, not a memory round trip.
constexpr int kWalkWin = 256;  // words per window (one per lane per register, 4 registers)
constexpr int kWalkRing = 8;   // LDS ring windows per wave

template <int N>
__device__ __forceinline__ void wire_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// A wave-uniform 64-bit value the compiler cannot prove uniform (the walk's positions): made so, so
// that the walk's arithmetic and branches stay scalar instead of EXEC-masked vector code.
__device__ __forceinline__ unsigned long long uni64(unsigned long long x) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

template <int RING = kWalkRing>
struct MapWalk {
  const uint32_t *fw;
  unsigned long long nw, nwin, issued, cur;
  uint32_t *ring;
  uint32_t r0, r1, r2, r3;

  __device__ void dma(unsigned long long wi, int lane) {
    uint32_t *dst = ring + (wi % RING) * kWalkWin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long w = wi * kWalkWin + 64 * j + lane;
      __builtin_amdgcn_global_load_lds(fw + (w < nw ? w : nw - 1),
                                       (__attribute__((address_space(3))) void *)(dst + 64 * j), 4, 0, 0);
    }
  }
  __device__ void start(int lane) {
    nw = uni64(nw);
    nwin = uni64(nwin);
    issued = 0;
    cur = ~0ull;
    while (issued < nwin && issued < (unsigned long long)RING) {
      dma(issued, lane);
      issued = uni64(issued + 1);
    }
  }
  // window wi into registers (wi > cur); then keep the ring full
  __device__ void load(unsigned long long wi, int lane) {
    // windows issued after wi: every vector-memory op issued since wi's DMA counts too, so this
    // waits at least for wi (in-order counter)
    switch ((int)(issued - 1 - wi)) {
      case 0: wire_vmcnt<0>(); break;
      case 1: wire_vmcnt<4>(); break;
      case 2: wire_vmcnt<8>(); break;
      case 3: wire_vmcnt<12>(); break;
      case 4: wire_vmcnt<16>(); break;
      case 5: wire_vmcnt<20>(); break;
      case 6: wire_vmcnt<24>(); break;
      default: wire_vmcnt<28>(); break;
    }
    const uint32_t *src = ring + (wi % RING) * kWalkWin + lane;
    r0 = src[0];
    r1 = src[64];
    r2 = src[128];
    r3 = src[192];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot is read: it may be refilled
    cur = uni64(wi);
    while (issued < nwin && issued <= wi + RING) {
      dma(issued, lane);
      issued = uni64(issued + 1);
    }
  }
  __device__ uint32_t get(unsigned long long k, int lane) {
    k = uni64(k);
    const unsigned long long wi = k / kWalkWin;
    if (wi != uni64(cur)) load(wi, lane);
    const int off = (int)(k % kWalkWin), l = off & 63, q = off >> 6;
    // four readlanes and scalar selects: a switch over r0..r3 may be lowered as an indexed access
    // to a stack copy of them (scratch: a memory round trip per word read)
    const uint32_t a = __builtin_amdgcn_readlane(r0, l), b = __builtin_amdgcn_readlane(r1, l);
    const uint32_t c = __builtin_amdgcn_readlane(r2, l), d = __builtin_amdgcn_readlane(r3, l);
    return q == 0 ? a : (q == 1 ? b : (q == 2 ? c : d));
  }
  __device__ u64 get64(unsigned long long k, int lane) { return (u64)get(k, lane) | ((u64)get(k + 1, lane) << 32); }
};

// out[0..n] = exclusive scan of in[0..n), out[n] = sum (wire.hip's scan kernels).  host_total
// non-NULL: the sum is copied back (synchronises).  scratch: ceil(n / kScanItems) + 2 u64.
int exclusive_scan(crdt_ctx *ctx, const u64 *in, u64 *out, unsigned long long n, u64 *scratch,
                   unsigned long long *host_total);

inline unsigned wave_grid(crdt_ctx *ctx, unsigned long long waves, int wpb, int per_cu) {
  const unsigned long long want = (waves + wpb - 1) / wpb;
  const unsigned long long cap = (unsigned long long)ctx->cu_count * per_cu;
  return (unsigned)(want == 0 ? 1 : (want < cap ? want : cap));
}

// frame sizes -> frame_off (device, N+1) -> *total (wire.hip; launches the scan kernels)
int egress_layout(crdt_ctx *ctx, u64 *sizes, u64 *frame_off, unsigned long long N, size_t *total);

inline int wire_scratch(crdt_ctx *ctx, unsigned long long N, u64 **sizes) {
  const unsigned long long nb = (N + kScanItems - 1) / kScanItems + 2;
  int rc = ensure_scratch(ctx, (N + nb + 8) * 8);
  if (rc) return rc;
  *sizes = reinterpret_cast<u64 *>(ctx->scratch);
  return CRDT_OK;
}

inline int check_frames(crdt_ctx *ctx, const void *bytes, const uint64_t *frame_off, size_t N, uint32_t *status) {
  if (N && (!frame_off || !status)) return fail(ctx, CRDT_EINVAL, "ingest: NULL frame_off / status");
  (void)bytes;
  return CRDT_OK;
}

}  // namespace crdt
