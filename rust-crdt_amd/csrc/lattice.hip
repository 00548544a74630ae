// Lattice lub kernels: elementwise max (VClock, GCounter, PNCounter) and bitwise OR (GSet).
//
// Reference semantics (crdts 3.0.0):
//   VClock::merge    vclock.rs:130-136 -> apply_dot :155-159  => out[a] = max(self[a], other[a])
//   GCounter::merge  gcounter.rs:44-48  (VClock on `inner`)
//   PNCounter::merge pncounter.rs:70-75 (P and N independently)  => max over a row of 2A words
//   GSet::merge      gset.rs:38-40 -> insert :69-71             => union = OR of interned bitmaps
// All four joins are associative, commutative and idempotent (README.md:37-47), so the fold
// `acc = T::new(); for r: acc.merge(r)` equals any tree of joins: the kernels fold a slice
// of replicas per thread in registers, combine the threads of a workgroup through LDS and
// the workgroups of a group through a two-level last-arriver combine inside the same launch.
//
// HBM layout: replica (g, r) row = in + g*gstride + r*rstride, W words contiguous.
// Loads are 16 B per lane (u64x2) and non-temporal: every input byte is read exactly once.
#include "common.hpp"

namespace crdt {

template <int V>
struct VecOf;
template <>
struct VecOf<1> {
  using T = u64;
};
template <>
struct VecOf<2> {
  using T = u64x2;
};

template <Op OP>
__device__ __forceinline__ u64 vjoin(u64 a, u64 b) {
  return join<OP>(a, b);
}
template <Op OP>
__device__ __forceinline__ u64x2 vjoin(u64x2 a, u64x2 b) {
  return join2<OP>(a, b);
}

template <typename VT>
__device__ __forceinline__ VT vzero() {
  return VT(0);
}

// Fold n rows spaced `step` vectors apart, U loads in flight per thread.
template <Op OP, typename VT, int U, bool NT>
__device__ __forceinline__ VT fold_rows(const VT *__restrict__ p, size_t n, long long step) {
  VT acc = vzero<VT>();
  size_t i = 0;
  for (; i + U <= n; i += U) {
    VT v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if constexpr (NT) v[k] = __builtin_nontemporal_load(p + k * step);
      else v[k] = p[k * step];
    }
#pragma unroll
    for (int k = 0; k < U; ++k) acc = vjoin<OP>(acc, v[k]);
    p += U * step;
  }
  for (; i < n; ++i) {
    VT v;
    if constexpr (NT) v = __builtin_nontemporal_load(p);
    else v = *p;
    acc = vjoin<OP>(acc, v);
    p += step;
  }
  return acc;
}

// Combine the TR row-lanes of a workgroup that share a column (lane l = rsub*PW + cl).
// Result valid for rsub == 0.  Every thread of the block must call it.
template <Op OP, typename VT>
__device__ __forceinline__ VT block_rows_combine(VT acc, VT *red, int l, int PW, int TR) {
  if (TR > 1) {
    red[l] = acc;
    __syncthreads();
    if (l < PW) {
      for (int j = 1; j < TR; ++j) acc = vjoin<OP>(acc, red[l + j * PW]);
    }
    __syncthreads();
  }
  return acc;
}

struct LubPlan {
  const u64 *in;
  u64 *out;
  u64 *part;   // [units][S][PW] vectors
  u64 *cpart;  // [units][ncl][PW] vectors
  unsigned *cnt1;  // [units][ncl]
  unsigned *cnt2;  // [units]
  long long rstride, gstride, ostride;  // words
  unsigned long long R, Rs;
  int Wv, PW, TR, ncolblk, S, CL, ncl;
  int accumulate;
  int interleave;  // 1: slice s takes row-steps s, s+S, s+2S, ... (all slices sweep HBM together)
};

template <Op OP, typename VT>
__device__ __forceinline__ void store_out(const LubPlan &p, size_t g, int col, VT v) {
  VT *o = reinterpret_cast<VT *>(p.out + g * p.ostride) + col;
  if (p.accumulate) v = vjoin<OP>(v, *o);
  *o = v;
}

// Agent-scope arrival on a counter after this block's stores (MI355X_MICROARCH.md
// "Valid forms": waitcnt -> barrier -> lane-0 release fence -> waitcnt -> atomic).
// Returns (block-uniformly) whether this block is the last of `expected` arrivals; the last
// arriver resets the counter and performs the agent-scope acquire before returning.
__device__ __forceinline__ bool arrive_last(unsigned *counter, unsigned expected, int *s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int last = (t == expected - 1);
    if (last) {
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_flag = last;
  }
  __syncthreads();
  return *s_flag != 0;
}

// Partial rows a lane of the last arriver keeps in flight in the level-1 / level-2 combines: these
// reads are the serial end of every launch, and a cluster's 32 rows take two round trips at 16
// (eight at 4).
constexpr int kLubCombineU = 16;

// Fold n >= 1 partial rows spaced `step` vectors apart, always kLubCombineU loads in flight: a
// batch past the end re-reads the last row instead of branching (the joins are idempotent), so
// a short fold (8 cluster partials, say) is one round trip, not one per row.
template <Op OP, typename VT>
__device__ __forceinline__ VT fold_partials(const VT *p, size_t n, long long step) {
  constexpr int U = kLubCombineU;
  VT acc = vzero<VT>();
  for (size_t i = 0; i < n; i += U) {
    const size_t rem = n - i;
    VT v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = p[(long long)((size_t)k < rem ? (size_t)k : rem - 1) * step];
#pragma unroll
    for (int k = 0; k < U; ++k) acc = vjoin<OP>(acc, v[k]);
    p += U * step;
  }
  return acc;
}

// Rows r0, r0 + rstep, ... < rend of group g folded at vector column col.
template <Op OP, int V, int U, bool NT, typename VT>
__device__ __forceinline__ VT lub_fold_range(const LubPlan &p, size_t g, int col, unsigned long long r0,
                                             unsigned long long rend, unsigned long long rstep) {
  if (r0 >= rend) return vzero<VT>();
  const size_t n = (rend - r0 + rstep - 1) / rstep;
  const VT *src = reinterpret_cast<const VT *>(p.in + g * p.gstride + r0 * p.rstride) + col;
  return fold_rows<OP, VT, U, NT>(src, n, (long long)rstep * p.rstride / V);
}

// The end of block b once its threads hold the fold of its rows in `acc`: combine the block's
// row-lanes, publish the partial row, and (last arrivers only) run the two combine levels.
template <Op OP, typename VT>
__device__ __forceinline__ void lub_finish(const LubPlan &p, unsigned b, VT acc, VT *red, int &s_flag) {
  const int l = threadIdx.x;
  const int s = b % p.S;
  const unsigned u = b / p.S;
  const int cb = u % p.ncolblk;
  const size_t g = u / p.ncolblk;
  const int cl = l % p.PW;
  const int rsub = l / p.PW;
  const int col = cb * kBlock + cl;
  acc = block_rows_combine<OP>(acc, red, l, p.PW, p.TR);
  const bool writer = (l < p.PW) && col < p.Wv;
  if (p.S == 1) {
    if (writer) store_out<OP>(p, g, col, acc);
    return;
  }

  // Level 1: publish this slice's partial row; the last slice of the cluster combines it.
  VT *part = reinterpret_cast<VT *>(p.part);
  if (writer) part[((size_t)u * p.S + s) * p.PW + cl] = acc;
  const int c = s / p.CL;
  const int csize = min(p.CL, p.S - c * p.CL);
  if (!arrive_last(p.cnt1 + (size_t)u * p.ncl + c, csize, &s_flag)) return;

  acc = vzero<VT>();
  {
    const int TRc = p.TR;
    if (rsub < TRc && col < p.Wv) {
      const int r0 = rsub;
      if (r0 < csize) {
        const size_t n = (csize - r0 + TRc - 1) / TRc;
        acc = fold_partials<OP>(part + ((size_t)u * p.S + c * p.CL + r0) * p.PW + cl, n, (long long)TRc * p.PW);
      }
    }
  }
  acc = block_rows_combine<OP>(acc, red, l, p.PW, p.TR);
  if (p.ncl == 1) {
    if (writer) store_out<OP>(p, g, col, acc);
    return;
  }

  // Level 2: publish the cluster partial; the last cluster combines all of them.
  VT *cpart = reinterpret_cast<VT *>(p.cpart);
  if (writer) cpart[((size_t)u * p.ncl + c) * p.PW + cl] = acc;
  if (!arrive_last(p.cnt2 + u, p.ncl, &s_flag)) return;

  acc = vzero<VT>();
  if (rsub < p.TR && col < p.Wv && rsub < p.ncl) {
    const size_t n = (p.ncl - rsub + p.TR - 1) / p.TR;
    acc = fold_partials<OP>(cpart + ((size_t)u * p.ncl + rsub) * p.PW + cl, n, (long long)p.TR * p.PW);
  }
  acc = block_rows_combine<OP>(acc, red, l, p.PW, p.TR);
  if (writer) store_out<OP>(p, g, col, acc);
}

// One launch = the whole lub.  Block b -> (unit u = g*ncolblk + cb, slice s).
template <Op OP, int V, int U, bool NT, typename VT>
__device__ __forceinline__ void lub_stream_body(const LubPlan &p, unsigned b, VT *red, int &s_flag) {
  const int l = threadIdx.x;
  const int s = b % p.S;
  const unsigned u = b / p.S;
  const int cb = u % p.ncolblk;
  const size_t g = u / p.ncolblk;
  const int rsub = l / p.PW;
  const int col = cb * kBlock + l % p.PW;

  VT acc = vzero<VT>();
  if (rsub < p.TR && col < p.Wv) {
    if (p.interleave) {
      acc = lub_fold_range<OP, V, U, NT, VT>(p, g, col, (unsigned long long)s * p.TR + rsub, p.R,
                                             (unsigned long long)p.S * p.TR);
    } else {
      const unsigned long long rbeg = (unsigned long long)s * p.Rs;
      acc = lub_fold_range<OP, V, U, NT, VT>(p, g, col, rbeg + rsub, min(p.R, rbeg + p.Rs), p.TR);
    }
  }
  lub_finish<OP>(p, b, acc, red, s_flag);
}

template <Op OP, int V, int U, bool NT = true>
__global__ __launch_bounds__(kBlock) void lub_stream_kernel(LubPlan p) {
  using VT = typename VecOf<V>::T;
  __shared__ VT red[kBlock];
  __shared__ int s_flag;
  lub_stream_body<OP, V, U, NT, VT>(p, blockIdx.x, red, s_flag);
}

// Several lubs of one join op in ONE persistent launch (crdt_lub_many_multi): segment i owns blocks
// [start[i], start[i+1]) of one concatenated list and every block runs exactly the single-lub body
// on its segment's plan.  The grid is min(blocks, one workgroup per CU) and workgroup w runs blocks
// w, w + grid, w + 2*grid, ...: the CU never holds more than its own stream, and where the segments
// were planned for the same grid every workgroup reads the same bytes (one slice of each segment).
// No block waits for another (the last arriver of a cluster combines, whoever it is), so the
// workgroups need not be co-resident and any grid >= 1 completes.  Where the launch's shape allows
// (lub_plan_tail), the blocks of the last round share the end of their rows through a ticket
// counter (lub_tail_block) so that the workgroups finish together.
constexpr int kLubMultiMax = 8;
struct LubMulti {
  LubPlan p[kLubMultiMax];
  unsigned start[kLubMultiMax + 1];
  int n;
  // Dynamic tail (lub_plan_tail): the blocks of the last round, b >= tail_first, all slices of the
  // last segment, fold only the first tail_rstat rows of their slice themselves; the rest is
  // tail_nch chunks of tail_rc rows per slice, handed out through *ticket.  tail_nch == 0: none.
  unsigned *ticket;
  unsigned tail_first, tail_nch;
  unsigned long long tail_rstat, tail_rc;
#ifdef LUB_STATS
  unsigned long long *stats;  // [total blocks][4]: see LubStat
#endif
};

#ifdef LUB_STATS
// -DLUB_STATS (scripts/build_variant.sh stats lattice.hip -DLUB_STATS; never the timed build): every
// block of a fused launch records who ran it, where and when; the host writes the records of the
// last launch to the file named by LUB_STATS_OUT (scripts/lub_stats.py reads it).
struct LubStat {
  unsigned long long t0, t1;  // wall_clock64() (100 MHz) at entry / exit of the block
  unsigned wg, seg, hw_id, xcc_id;
  __device__ __forceinline__ void begin(unsigned w, int i) {
    wg = w;
    seg = (unsigned)i;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    t0 = wall_clock64();
  }
  __device__ __forceinline__ void end(unsigned long long *stats, unsigned b) {
    t1 = wall_clock64();
    if (threadIdx.x == 0) {
      unsigned long long *o = stats + 4ull * b;
      o[0] = t0;
      o[1] = t1;
      o[2] = (unsigned long long)wg | ((unsigned long long)seg << 32);
      o[3] = (unsigned long long)hw_id | ((unsigned long long)xcc_id << 32);
    }
  }
};

static int lub_stats_begin(crdt_ctx *ctx, LubMulti &m, size_t blocks) {
  static unsigned long long *buf = nullptr;
  static size_t cap = 0;
  if (blocks > cap) {
    if (buf) (void)hipFree(buf);
    cap = 0;
    CRDT_HIP(ctx, hipMalloc(&buf, blocks * 32));
    cap = blocks;
  }
  m.stats = buf;
  return CRDT_OK;
}

static int lub_stats_dump(crdt_ctx *ctx, const LubMulti &m, size_t blocks, unsigned grid) {
  const char *path = getenv("LUB_STATS_OUT");
  if (!path) return CRDT_OK;
  std::vector<unsigned long long> h(blocks * 4);
  CRDT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  CRDT_HIP(ctx, hipMemcpy(h.data(), m.stats, blocks * 32, hipMemcpyDeviceToHost));
  FILE *f = fopen(path, "w");
  if (!f) return fail(ctx, CRDT_EINVAL, "LUB_STATS_OUT: cannot write %s", path);
  fprintf(f, "# grid %u blocks %zu segments %d cu_count %d\n# block seg wg t0 t1 xcc hw_id\n", grid, blocks, m.n,
          ctx->cu_count);
  for (size_t b = 0; b < blocks; ++b)
    fprintf(f, "%zu %llu %llu %llu %llu %llu %llu\n", b, h[4 * b + 2] >> 32, h[4 * b + 2] & 0xffffffffull, h[4 * b],
            h[4 * b + 1], h[4 * b + 3] >> 32, h[4 * b + 3] & 0xffffffffull);
  fclose(f);
  return CRDT_OK;
}
#endif

// A block of the last round with a dynamic tail.  The workgroups do not finish together (their
// exits spread over ~5% of the launch at the bench shape: each CU gets what the fabric gives it),
// so the last eighth of the launch's bytes is not owned by anybody: it is cut into chunks
// (>= 512 KiB each) of the last segment's slices and a workgroup that has folded the static part of
// its slice takes chunks from one agent-scope ticket counter until none is left.  The joins are
// associative, commutative and idempotent and every tail slice belongs to the same unit (one
// group, one column block), so a chunk of ANY slice joins into this workgroup's accumulators and
// the partial row it then publishes for its own slice is as good as any other split of the rows:
// the scratch layout, the counters and the combine are those of the static plan and the result is
// bit for bit the same.  Nobody waits: the next ticket is requested before the current chunk is
// folded (its latency hides behind the chunk's first loads) and a workgroup that draws a ticket
// past the end goes on to publish.  Every workgroup draws exactly one such ticket, so the draw
// numbered tickets + workgroups - 1 is the last one of the launch and resets the counter.
template <Op OP, int V, int U, typename VT>
__device__ __forceinline__ void lub_tail_block(const LubMulti &m, unsigned b, VT *red, int &s_flag,
                                               unsigned *s_tick) {
  const LubPlan &p = m.p[m.n - 1];
  const unsigned bl = b - m.start[m.n - 1];  // = the slice: the tail segment has one unit
  const int l = threadIdx.x;
  const int rsub = l / p.PW;
  const int col = l % p.PW;
  const bool active = rsub < p.TR && col < p.Wv;
  const unsigned s0 = m.tail_first - m.start[m.n - 1];  // first tail slice
  const unsigned nslices = p.S - s0;                    // tail slices (= workgroups of the launch)
  const unsigned ntick = nslices * m.tail_nch;

  VT acc = vzero<VT>();
  {
    const unsigned long long rbeg = (unsigned long long)bl * p.Rs;
    const unsigned long long rend = min(min(p.R, rbeg + p.Rs), rbeg + m.tail_rstat);
    if (active) acc = lub_fold_range<OP, V, U, true, VT>(p, 0, col, rbeg + rsub, rend, p.TR);
  }
  unsigned mine = 0;
  if (l == 0) mine = __hip_atomic_fetch_add(m.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int it = 0;; ++it) {
    // s_tick[it & 1] was last read in iteration it - 2, before the barrier of iteration it - 1,
    // which lane 0 has passed: two slots order the broadcast with one barrier per chunk.
    if (l == 0) s_tick[it & 1] = mine;
    __syncthreads();
    const unsigned t = s_tick[it & 1];
    if (t >= ntick) {
      if (l == 0 && t == ntick + nslices - 1)
        __hip_atomic_store(m.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    if (l == 0) mine = __hip_atomic_fetch_add(m.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long sbeg = (unsigned long long)(s0 + t % nslices) * p.Rs;
    const unsigned long long rbeg = sbeg + m.tail_rstat + (unsigned long long)(t / nslices) * m.tail_rc;
    const unsigned long long rend = min(min(p.R, sbeg + p.Rs), rbeg + m.tail_rc);
    if (active) acc = vjoin<OP>(acc, lub_fold_range<OP, V, U, true, VT>(p, 0, col, rbeg + rsub, rend, p.TR));
  }
  lub_finish<OP>(p, bl, acc, red, s_flag);
}

template <Op OP, int V, int U>
__global__ __launch_bounds__(kBlock) void lub_multi_kernel(LubMulti m) {
  using VT = typename VecOf<V>::T;
  __shared__ VT red[kBlock];
  __shared__ int s_flag;
  __shared__ unsigned s_tick[2];
  // The body runs once per block of this workgroup, so `red` and `s_flag` are reused; every path out
  // of the body is block-uniform (a `return` there is "next block" here) and each reuse is ordered:
  //  - red: block_rows_combine reads red between its two __syncthreads, so the trailing one orders
  //    its reads before the next write of red (the next combine of this block or of the next one);
  //  - s_flag: every thread reads it after arrive_last's second __syncthreads and lane 0 writes it
  //    again only after the first __syncthreads of the next arrive_last, which no thread passes
  //    before it has read the previous value.
  const unsigned total = m.start[kLubMultiMax];  // <= 2^31 - 1, so b + gridDim.x cannot wrap
  for (unsigned b = blockIdx.x; b < total; b += gridDim.x) {
    int i = 0;
#pragma unroll
    for (int j = 1; j < kLubMultiMax; ++j)
      if (j < m.n && b >= m.start[j]) i = j;
#ifdef LUB_STATS
    LubStat st;
    st.begin(blockIdx.x, i);
#endif
    if (m.tail_nch && b >= m.tail_first) lub_tail_block<OP, V, U, VT>(m, b, red, s_flag, s_tick);
    else lub_stream_body<OP, V, U, true, VT>(m.p[i], b - m.start[i], red, s_flag);
#ifdef LUB_STATS
    st.end(m.stats, b);
#endif
  }
}

// self[i] := self[i] ⊔ other[i]: three streams (2 reads, 1 write), TR rows per block step.
template <Op OP, int V>
__global__ __launch_bounds__(kBlock) void merge_pairs_kernel(u64 *__restrict__ self,
                                                             const u64 *__restrict__ other,
                                                             unsigned long long N, int Wv, int PW,
                                                             int TR, long long sstride,
                                                             long long ostride,
                                                             unsigned long long rows_per_block) {
  using VT = typename VecOf<V>::T;
  constexpr int U = 4;  // row pairs in flight per lane
  const int l = threadIdx.x;
  const int cl = l % PW;
  const int rsub = l / PW;
  const int col = blockIdx.y * kBlock + cl;
  if (rsub >= TR || col >= Wv) return;
  const unsigned long long rbeg = (unsigned long long)blockIdx.x * rows_per_block;
  const unsigned long long rend = min(N, rbeg + rows_per_block);
  unsigned long long r = rbeg + rsub;
  for (; r + (U - 1) * TR < rend; r += U * TR) {
    VT a[U], bv[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      a[k] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(self + (r + k * TR) * sstride) + col);
      bv[k] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(other + (r + k * TR) * ostride) + col);
    }
#pragma unroll
    for (int k = 0; k < U; ++k)
      __builtin_nontemporal_store(vjoin<OP>(a[k], bv[k]), reinterpret_cast<VT *>(self + (r + k * TR) * sstride) + col);
  }
  for (; r < rend; r += TR) {
    VT *sp = reinterpret_cast<VT *>(self + r * sstride) + col;
    const VT *op = reinterpret_cast<const VT *>(other + r * ostride) + col;
    *sp = vjoin<OP>(*sp, __builtin_nontemporal_load(op));
  }
}

// merge_batch with 16-byte rows: LR-lane row groups (common.hpp ROW_GROUP_LOOP), ~8 independent
// pieces per lane, 2 workgroups per CU — the shape that measured fastest for the 2-read-1-write
// row passes (1,080 us vs 1,207 us for merge_pairs_kernel at 1M pairs x 256).
template <Op OP>
__global__ __launch_bounds__(kBlock) void merge_rows_kernel(u64 *self, const u64 *other, unsigned long long N,
                                                            unsigned long long W, long long ss, long long os,
                                                            int lr_log) {
  ROW_GROUP_LOOP(N, lr_log) {
    const unsigned long long r = rb + (lane >> lr_log);
    if (r >= N) continue;
    u64 *sr = self + r * ss;
    const u64 *orow = other + r * os;
#pragma unroll 8
    for (unsigned long long c = 2ull * gl; c < W; c += 2ull * LR) {
      const u64x2 a = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(sr + c));
      const u64x2 b = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(orow + c));
      __builtin_nontemporal_store(join2<OP>(a, b), reinterpret_cast<u64x2 *>(sr + c));
    }
  }
}

// merge_batch of packed rows (both strides == W): one flat stream of 16-byte pieces, grid-stride,
// 2 pieces per lane in flight at one workgroup per CU — the shape at which an in-place
// read-self / read-other / write-self stream peaks on this part (scripts/micro/stream_rate.hip,
// 75% vs 65-69% with more requests in flight).
template <Op OP, int U>
__global__ __launch_bounds__(kBlock) void merge_flat_kernel(u64x2 *self, const u64x2 *other, unsigned long long n) {
  const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
  unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  for (; i + (U - 1) * stride < n; i += U * stride) {
    u64x2 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = __builtin_nontemporal_load(self + i + u * stride);
      b[u] = __builtin_nontemporal_load(other + i + u * stride);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(join2<OP>(a[u], b[u]), self + i + u * stride);
  }
  for (; i < n; i += stride) __builtin_nontemporal_store(join2<OP>(self[i], other[i]), self + i);
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Validation and launch geometry of one lub (no scratch yet).  launch = false: nothing to run
// (an empty fold was already written, or G / W is 0).
struct LubSetup {
  LubPlan p;
  int V = 1;
  bool launch = false;
  size_t blocks = 0, part_b = 0, cpart_b = 0, ncnt = 0;
};

static int lub_prepare(crdt_ctx *ctx, Op op, const u64 *in, size_t G, size_t R, size_t W, size_t row_stride,
                       size_t group_stride, u64 *out, size_t out_stride, unsigned flags, LubSetup &su) {
  su = LubSetup{};
  if (G == 0 || W == 0) return CRDT_OK;
  if (!out) return fail(ctx, CRDT_EINVAL, "lub_many: out is NULL");
  if (G > 1 && out_stride < W)
    return fail(ctx, CRDT_EINVAL, "lub_many: out_stride %zu < row width %zu", out_stride, W);
  if (W > (size_t)1 << 30) return fail(ctx, CRDT_EUNSUPPORTED, "lub_many: row width %zu too large", W);
  const bool accumulate = flags & CRDT_ACCUMULATE;
  if (R == 0) {  // fold of nothing = T::new() (all zero); with ACCUMULATE: unchanged
    if (!accumulate)
      CRDT_HIP(ctx, hipMemset2DAsync(out, (G > 1 ? out_stride : W) * 8, 0, W * 8, G, ctx->stream));
    return CRDT_OK;
  }
  if (!in) return fail(ctx, CRDT_EINVAL, "lub_many: in is NULL");
  if (R > 1 && row_stride < W)
    return fail(ctx, CRDT_EINVAL, "lub_many: row_stride %zu < row width %zu", row_stride, W);

  const bool vec2 = (W % 2 == 0) && (R == 1 || row_stride % 2 == 0) &&
                    (G == 1 || (group_stride % 2 == 0 && out_stride % 2 == 0)) && aligned16(in) &&
                    aligned16(out);
  const int V = vec2 ? 2 : 1;
  LubPlan &p = su.p;
  p.in = in;
  p.out = out;
  p.rstride = (long long)row_stride;
  p.gstride = (long long)group_stride;
  p.ostride = (long long)out_stride;
  p.R = R;
  p.Wv = (int)(W / V);
  p.PW = p.Wv <= kBlock ? p.Wv : kBlock;
  p.TR = kBlock / p.PW;
  p.ncolblk = (p.Wv + kBlock - 1) / kBlock;
  p.accumulate = accumulate ? 1 : 0;

  // Slice replicas so the grid holds ~bpc workgroups per CU, each thread folding >= min_steps rows.
  const size_t units = G * (size_t)p.ncolblk;
  const size_t target = ctx->tune.lub_grid > 0 ? (size_t)ctx->tune.lub_grid
                                               : (size_t)ctx->cu_count * ctx->tune.lub_blocks_per_cu;
  const size_t steps = (R + p.TR - 1) / p.TR;
  size_t S = 1;
  if (units < target) {
    S = (target + units - 1) / units;
    size_t max_s = steps / ctx->tune.lub_min_steps;
    if (max_s < 1) max_s = 1;
    if (S > max_s) S = max_s;
  }
  size_t Rs = (R + S - 1) / S;
  Rs = (Rs + p.TR - 1) / p.TR * p.TR;  // whole block steps per slice
  S = (R + Rs - 1) / Rs;
  if ((size_t)units * S > 0x7fffffffULL)
    return fail(ctx, CRDT_EUNSUPPORTED, "lub_many: grid too large (%zu units x %zu slices)", units, S);
  p.S = (int)S;
  p.Rs = Rs;
  p.interleave = ctx->tune.lub_interleave;
  p.CL = 32;
  p.ncl = (p.S + p.CL - 1) / p.CL;
  if (p.S > 1) {
    const size_t vecb = (size_t)V * 8;
    su.part_b = units * S * p.PW * vecb;
    su.cpart_b = units * p.ncl * p.PW * vecb;
    su.ncnt = units * p.ncl + units;
  }
  su.V = V;
  su.blocks = units * S;
  su.launch = true;
  return CRDT_OK;
}

// Scratch of a prepared lub at `base` (part, then cpart) and counters at `cnt`.
static void lub_assign(LubSetup &su, char *base, unsigned *cnt) {
  if (su.p.S <= 1) return;
  const size_t units = su.blocks / su.p.S;
  su.p.cnt1 = cnt;
  su.p.cnt2 = cnt + units * su.p.ncl;
  su.p.part = reinterpret_cast<u64 *>(base);
  su.p.cpart = reinterpret_cast<u64 *>(base + su.part_b);
}

int lattice_lub_many(crdt_ctx *ctx, Op op, const u64 *in, size_t G, size_t R, size_t W,
                     size_t row_stride, size_t group_stride, u64 *out, size_t out_stride,
                     unsigned flags) {
  CRDT_CHECK_CTX(ctx);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  LubSetup su;
  if (int rc = lub_prepare(ctx, op, in, G, R, W, row_stride, group_stride, out, out_stride, flags, su)) return rc;
  if (!su.launch) return CRDT_OK;
  if (su.p.S > 1) {
    if (int rc = ensure_scratch(ctx, su.part_b + su.cpart_b)) return rc;
    if (int rc = ensure_counters(ctx, su.ncnt)) return rc;
    lub_assign(su, static_cast<char *>(ctx->scratch), ctx->counters);
  }
  const LubPlan &p = su.p;
  const int V = su.V;
  const dim3 grid((unsigned)su.blocks);
  timing_begin(ctx, "lub_stream");
  const int U = ctx->tune.lub_unroll;
#define CRDT_LAUNCH_LUB(OPV, VV, UV) \
  hipLaunchKernelGGL((lub_stream_kernel<OPV, VV, UV>), grid, dim3(kBlock), 0, ctx->stream, p)
  if (op == Op::Max) {
    if (V == 2) {
      if (!ctx->tune.lub_nt) hipLaunchKernelGGL((lub_stream_kernel<Op::Max, 2, 8, false>), grid, dim3(kBlock), 0, ctx->stream, p);
      else if (U == 4) CRDT_LAUNCH_LUB(Op::Max, 2, 4);
      else if (U == 16) CRDT_LAUNCH_LUB(Op::Max, 2, 16);
      else if (U == 32) CRDT_LAUNCH_LUB(Op::Max, 2, 32);
      else CRDT_LAUNCH_LUB(Op::Max, 2, 8);
    } else CRDT_LAUNCH_LUB(Op::Max, 1, 8);
  } else {
    if (V == 2) CRDT_LAUNCH_LUB(Op::Or, 2, 8);
    else CRDT_LAUNCH_LUB(Op::Or, 1, 8);
  }
#undef CRDT_LAUNCH_LUB
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

// The dynamic tail of a persistent launch (lub_tail_block), where its shape allows one: the last
// round of blocks (one per workgroup) lies in the last segment, that segment is one unit of
// contiguous slices, and an eighth of a workgroup's share of the launch's bytes holds at least one
// chunk of tune.lub_chunk_bytes (whole unrolled block steps of rows; 0 bytes: no tail).
static void lub_plan_tail(const Tune &tune, LubMulti &m, int V, size_t blocks, unsigned grid, size_t bytes,
                          unsigned *ticket) {
  m.tail_nch = 0;
  const LubPlan &p = m.p[m.n - 1];
  const size_t first = blocks - grid, seg0 = m.start[m.n - 1];
  if (tune.lub_chunk_bytes <= 0 || first < seg0 || blocks - seg0 != (size_t)p.S || p.S <= 1 || p.interleave) return;
  const size_t row_b = (size_t)p.Wv * V * 8, step = 8 * (size_t)p.TR;
  size_t rc = ((size_t)tune.lub_chunk_bytes + row_b - 1) / row_b;
  rc = (rc + step - 1) / step * step;
  size_t nch = bytes / grid / 8 / (rc * row_b);
  if (nch * rc > p.Rs) nch = p.Rs / rc;
  if (nch == 0 || (unsigned long long)grid * nch + grid > 0x7fffffffULL) return;
  m.ticket = ticket;
  m.tail_first = (unsigned)first;
  m.tail_nch = (unsigned)nch;
  m.tail_rc = rc;
  m.tail_rstat = p.Rs - nch * rc;
}

// Several lattice lubs, one launch per (join op, vector width) class of up to kLubMultiMax
// segments; results identical to one lattice_lub_many per segment (each segment's blocks run the
// single-lub body on its own plan and scratch).
int lattice_lub_many_multi(crdt_ctx *ctx, const LubReq *reqs, size_t n) {
  CRDT_CHECK_CTX(ctx);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<LubSetup> su(n);
  for (size_t i = 0; i < n; ++i) {
    const LubReq &q = reqs[i];
    if (int rc = lub_prepare(ctx, q.op, q.in, q.G, q.R, q.W, q.row_stride, q.group_stride, q.out, q.out_stride,
                             q.flags, su[i]))
      return rc;
  }
  // one scratch / counter region for every segment (a later launch of this call never reuses an
  // earlier one's region, so launches need no ordering beyond the stream's)
  size_t sb = 0, nc = 0;
  for (auto &x : su)
    if (x.launch) {
      sb += (x.part_b + x.cpart_b + 255) / 256 * 256;
      nc += x.ncnt;
    }
  if (sb) {
    if (int rc = ensure_scratch(ctx, sb)) return rc;
    if (int rc = ensure_counters(ctx, nc + n)) return rc;  // + one ticket counter per launch
  }
  {
    char *base = static_cast<char *>(ctx->scratch);
    unsigned *cnt = ctx->counters;
    for (auto &x : su)
      if (x.launch && x.p.S > 1) {
        lub_assign(x, base, cnt);
        base += (x.part_b + x.cpart_b + 255) / 256 * 256;
        cnt += x.ncnt;
      }
  }
  std::vector<bool> done(n, false);
  size_t launches = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!su[i].launch || done[i]) continue;
    LubMulti m{};
    m.n = 0;
    size_t blocks = 0, bytes = 0;
    const Op op = reqs[i].op;
    const int V = su[i].V;
    for (size_t j = i; j < n && m.n < kLubMultiMax; ++j) {
      if (!su[j].launch || done[j] || reqs[j].op != op || su[j].V != V) continue;
      m.p[m.n] = su[j].p;
      m.start[m.n] = (unsigned)blocks;
      blocks += su[j].blocks;
      bytes += reqs[j].G * reqs[j].R * reqs[j].W * 8;
      ++m.n;
      done[j] = true;
    }
    if (blocks > 0x7fffffffULL) return fail(ctx, CRDT_EUNSUPPORTED, "lub_many_multi: grid too large");
    for (int k = m.n; k <= kLubMultiMax; ++k) m.start[k] = (unsigned)blocks;
#ifdef LUB_STATS
    if (int rc = lub_stats_begin(ctx, m, blocks)) return rc;
#endif
    // persistent grid: one workgroup per CU (tune lubpg=N: N workgroups), never more than blocks
    const size_t cap = ctx->tune.lub_persist_grid > 0 ? (size_t)ctx->tune.lub_persist_grid
                                                      : (size_t)ctx->cu_count * ctx->tune.lub_blocks_per_cu;
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
    if (sb) lub_plan_tail(ctx->tune, m, V, blocks, grid.x, bytes, ctx->counters + nc + launches);
    ++launches;
    timing_begin(ctx, "lub_stream");
#define CRDT_LAUNCH_MULTI(OPV, VV) \
  hipLaunchKernelGGL((lub_multi_kernel<OPV, VV, 8>), grid, dim3(kBlock), 0, ctx->stream, m)
    if (op == Op::Max) {
      if (V == 2) CRDT_LAUNCH_MULTI(Op::Max, 2);
      else CRDT_LAUNCH_MULTI(Op::Max, 1);
    } else {
      if (V == 2) CRDT_LAUNCH_MULTI(Op::Or, 2);
      else CRDT_LAUNCH_MULTI(Op::Or, 1);
    }
#undef CRDT_LAUNCH_MULTI
    timing_end(ctx);
    CRDT_HIP(ctx, hipGetLastError());
#ifdef LUB_STATS
    if (int rc = lub_stats_dump(ctx, m, blocks, grid.x)) return rc;
#endif
  }
  return CRDT_OK;
}

int lattice_merge_batch(crdt_ctx *ctx, Op op, u64 *self, const u64 *other, size_t N, size_t W,
                        size_t self_stride, size_t other_stride) {
  CRDT_CHECK_CTX(ctx);
  if (N == 0 || W == 0) return CRDT_OK;
  if (!self || !other) return fail(ctx, CRDT_EINVAL, "merge_batch: NULL buffer");
  if (N > 1 && (self_stride < W || other_stride < W))
    return fail(ctx, CRDT_EINVAL, "merge_batch: stride < row width %zu", W);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  const bool vec2 = W % 2 == 0 && (N == 1 || (self_stride % 2 == 0 && other_stride % 2 == 0)) &&
                    aligned16(self) && aligned16(other);
  const bool packed = N == 1 || (self_stride == W && other_stride == W);
  if (vec2 && packed && ctx->tune.merge_flat) {
    const unsigned long long n = (unsigned long long)N * W / 2;  // 16-byte pieces
    const unsigned long long want = (n + kBlock - 1) / kBlock;
    const unsigned long long cap = (unsigned long long)ctx->cu_count * ctx->tune.merge_flat;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    timing_begin(ctx, "merge_pairs");
    u64x2 *sp = reinterpret_cast<u64x2 *>(self);
    const u64x2 *op2 = reinterpret_cast<const u64x2 *>(other);
    const int fu = ctx->tune.merge_flat_u;
#define CRDT_FLAT(OPV, UU) hipLaunchKernelGGL((merge_flat_kernel<OPV, UU>), dim3(grid), dim3(kBlock), 0, ctx->stream, sp, op2, n)
    if (op == Op::Max) {
      if (fu == 1) CRDT_FLAT(Op::Max, 1);
      else if (fu == 4) CRDT_FLAT(Op::Max, 4);
      else CRDT_FLAT(Op::Max, 2);
    } else {
      if (fu == 1) CRDT_FLAT(Op::Or, 1);
      else if (fu == 4) CRDT_FLAT(Op::Or, 4);
      else CRDT_FLAT(Op::Or, 2);
    }
#undef CRDT_FLAT
    timing_end(ctx);
    CRDT_HIP(ctx, hipGetLastError());
    return CRDT_OK;
  }
  if (vec2 && ctx->tune.merge_rows) {
    const int lr_log = row_lr_log(W / 2, ctx->tune.merge_ppl);
    const unsigned long long rpb = 4ull * (kWave >> lr_log);
    const unsigned long long want = (N + rpb - 1) / rpb;
    const unsigned long long cap = (unsigned long long)ctx->cu_count * ctx->tune.merge_blocks_per_cu;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    timing_begin(ctx, "merge_pairs");
    if (op == Op::Max)
      hipLaunchKernelGGL(merge_rows_kernel<Op::Max>, dim3(grid), dim3(kBlock), 0, ctx->stream, self, other,
                         (unsigned long long)N, (unsigned long long)W, (long long)self_stride, (long long)other_stride, lr_log);
    else
      hipLaunchKernelGGL(merge_rows_kernel<Op::Or>, dim3(grid), dim3(kBlock), 0, ctx->stream, self, other,
                         (unsigned long long)N, (unsigned long long)W, (long long)self_stride, (long long)other_stride, lr_log);
    timing_end(ctx);
    CRDT_HIP(ctx, hipGetLastError());
    return CRDT_OK;
  }
  const int V = vec2 ? 2 : 1;
  const int Wv = (int)(W / V);
  const int PW = Wv <= kBlock ? Wv : kBlock;
  const int TR = kBlock / PW;
  const int ncolblk = (Wv + kBlock - 1) / kBlock;
  // Contiguous row ranges, ~mbpc workgroups per CU (each lane >= 16 row steps).
  const unsigned long long want = (unsigned long long)ctx->cu_count * ctx->tune.merge_blocks_per_cu;
  unsigned long long rpb = (N + want - 1) / want;
  rpb = (rpb + TR - 1) / TR * TR;
  if (rpb < (unsigned long long)TR * 16) rpb = (unsigned long long)TR * 16;
  unsigned long long nb = (N + rpb - 1) / rpb;
  if (nb > 0x7fffffffULL) return fail(ctx, CRDT_EUNSUPPORTED, "merge_batch: N too large");
  dim3 grid((unsigned)nb, (unsigned)ncolblk);
  timing_begin(ctx, "merge_pairs");
  if (op == Op::Max) {
    if (V == 2) hipLaunchKernelGGL((merge_pairs_kernel<Op::Max, 2>), grid, dim3(kBlock), 0, ctx->stream, self, other, N, Wv, PW, TR, (long long)self_stride, (long long)other_stride, rpb);
    else hipLaunchKernelGGL((merge_pairs_kernel<Op::Max, 1>), grid, dim3(kBlock), 0, ctx->stream, self, other, N, Wv, PW, TR, (long long)self_stride, (long long)other_stride, rpb);
  } else {
    if (V == 2) hipLaunchKernelGGL((merge_pairs_kernel<Op::Or, 2>), grid, dim3(kBlock), 0, ctx->stream, self, other, N, Wv, PW, TR, (long long)self_stride, (long long)other_stride, rpb);
    else hipLaunchKernelGGL((merge_pairs_kernel<Op::Or, 1>), grid, dim3(kBlock), 0, ctx->stream, self, other, N, Wv, PW, TR, (long long)self_stride, (long long)other_stride, rpb);
  }
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

}  // namespace crdt

using crdt::Op;
using crdt::u64;

// CRDT_MEM_HOST routes the public lattice entry points through the chunked host staging.
static int lub_dispatch(crdt_ctx *ctx, Op op, const u64 *in, size_t G, size_t R, size_t W, size_t row_stride,
                        size_t group_stride, u64 *out, size_t out_stride, unsigned flags) {
  CRDT_CHECK_CTX(ctx);
  if (ctx->mem_kind == CRDT_MEM_HOST)
    return crdt::lattice_lub_many_host(ctx, op, in, G, R, W, row_stride, group_stride, out, out_stride, flags);
  return crdt::lattice_lub_many(ctx, op, in, G, R, W, row_stride, group_stride, out, out_stride, flags);
}
static int merge_dispatch(crdt_ctx *ctx, Op op, u64 *self, const u64 *other, size_t N, size_t W, size_t self_stride,
                          size_t other_stride) {
  CRDT_CHECK_CTX(ctx);
  if (ctx->mem_kind == CRDT_MEM_HOST)
    return crdt::lattice_merge_batch_host(ctx, op, self, other, N, W, self_stride, other_stride);
  return crdt::lattice_merge_batch(ctx, op, self, other, N, W, self_stride, other_stride);
}

// crdt_lub_many_multi: the per-kind dims of each segment mapped to the lattice form
// (PNCounter rows hold 2A words; GCounter is VClock).
int crdt::lub_reqs_from_segments(crdt_ctx *ctx, const crdt_lub_segment *segs, size_t nseg,
                                 std::vector<crdt::LubReq> &reqs) {
  if (nseg && !segs) return crdt::fail(ctx, CRDT_EINVAL, "lub_many_multi: segs is NULL");
  reqs.resize(nseg);
  for (size_t i = 0; i < nseg; ++i) {
    const crdt_lub_segment &sg = segs[i];
    crdt::LubReq &q = reqs[i];
    switch (sg.kind) {
      case CRDT_KIND_VCLOCK:
      case CRDT_KIND_GCOUNTER: q.op = Op::Max; q.W = sg.A; break;
      case CRDT_KIND_PNCOUNTER: q.op = Op::Max; q.W = 2 * sg.A; break;
      case CRDT_KIND_GSET: q.op = Op::Or; q.W = sg.A; break;
      default: return crdt::fail(ctx, CRDT_EINVAL, "lub_many_multi: segment %zu has unknown kind %d", i, sg.kind);
    }
    q.in = (const u64 *)sg.in;
    q.G = sg.G;
    q.R = sg.R;
    q.row_stride = sg.row_stride;
    q.group_stride = sg.group_stride;
    q.out = (u64 *)sg.out;
    q.out_stride = sg.out_stride;
    q.flags = sg.flags;
  }
  return CRDT_OK;
}

extern "C" {

int crdt_vclock_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                         size_t row_stride, size_t group_stride, uint64_t *out,
                         size_t out_stride, unsigned flags) {
  return lub_dispatch(ctx, Op::Max, (const u64 *)in, G, R, A, row_stride, group_stride,
                                (u64 *)out, out_stride, flags);
}
int crdt_vclock_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                            size_t A, size_t self_stride, size_t other_stride) {
  return merge_dispatch(ctx, Op::Max, (u64 *)self, (const u64 *)other, N, A,
                                   self_stride, other_stride);
}
int crdt_gcounter_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                           size_t row_stride, size_t group_stride, uint64_t *out,
                           size_t out_stride, unsigned flags) {
  return crdt_vclock_lub_many(ctx, in, G, R, A, row_stride, group_stride, out, out_stride, flags);
}
int crdt_gcounter_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                              size_t A, size_t self_stride, size_t other_stride) {
  return crdt_vclock_merge_batch(ctx, self, other, N, A, self_stride, other_stride);
}
int crdt_pncounter_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t A,
                            size_t row_stride, size_t group_stride, uint64_t *out,
                            size_t out_stride, unsigned flags) {
  return lub_dispatch(ctx, Op::Max, (const u64 *)in, G, R, 2 * A, row_stride,
                                group_stride, (u64 *)out, out_stride, flags);
}
int crdt_pncounter_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other,
                               size_t N, size_t A, size_t self_stride, size_t other_stride) {
  return merge_dispatch(ctx, Op::Max, (u64 *)self, (const u64 *)other, N, 2 * A,
                                   self_stride, other_stride);
}
int crdt_gset_lub_many(crdt_ctx *ctx, const uint64_t *in, size_t G, size_t R, size_t words,
                       size_t row_stride, size_t group_stride, uint64_t *out,
                       size_t out_stride, unsigned flags) {
  return lub_dispatch(ctx, Op::Or, (const u64 *)in, G, R, words, row_stride,
                                group_stride, (u64 *)out, out_stride, flags);
}
int crdt_gset_merge_batch(crdt_ctx *ctx, uint64_t *self, const uint64_t *other, size_t N,
                          size_t words, size_t self_stride, size_t other_stride) {
  return merge_dispatch(ctx, Op::Or, (u64 *)self, (const u64 *)other, N, words,
                                   self_stride, other_stride);
}

int crdt_lub_many_multi(crdt_ctx *ctx, const crdt_lub_segment *segs, size_t nseg) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  std::vector<crdt::LubReq> reqs;
  if (int rc = crdt::lub_reqs_from_segments(ctx, segs, nseg, reqs)) return rc;
  return crdt::lattice_lub_many_multi(ctx, reqs.data(), reqs.size());
}

}  // extern "C"
