// Out-of-place re-index of resident dense states: every indexed axis (actor columns, member / key rows
// and bits, value slots, deferred slots) of N states is gathered from one dense layout into another,
//   crdt_reindex_map_u32 / _u64   src[j] = position of new_ids[j] in old_ids (binary search per lane)
//   crdt_rows_reindex             N rows of planes x A words (VClock, GCounter, PNCounter, pooled clocks)
//   crdt_bitmap_reindex           N bitmap rows, bit by bit (GSet, pooled member / key sets)
//   crdt_orswot_reindex / crdt_mvreg_reindex / crdt_map_reindex
// with no host synchronisation.  An axis map is a device u32 src[n_out]: output index j takes input
// index src[j]; src[j] >= n_in is nobody (zeros); a NULL map is the identity prefix.
//
// Kernels:
//   rx_prep_kernel   one workgroup per call: used[i] = 1 iff input index i of an axis is referenced by
//                    the map (or, for a NULL map, i < n_out), and any[axis] = 1 iff some index is not.
//                    Both live in ctx scratch; the loss test below reads them, so a call that drops
//                    nothing pays one uniform word per state for it.
//   rx_head_kernel   out def_count (clamped to out Dcap, 0 for an invalid input count) and the status
//                    word's bits 0 / 2, one plain store per state: status needs no zeroing.
//   rx_rows_kernel   the gather of a block of K x V rows of A words per state: K outer rows (member /
//                    key rows through row_src, or deferred slots limited by def_count), V inner rows
//                    (value slots, PNCounter planes: slot v goes to slot v), A columns through
//                    col_src.  A state takes a sub-wave segment of 1..64 lanes or, past 1,024 pieces,
//                    a workgroup (the eq.hip plan); inside it 2^lr lanes span a row and the rest of
//                    the lanes take further rows, four rows per lane in flight before the first store.
//                    Stores are 16-byte non-temporal where the output rows are 16-byte aligned and
//                    even; loads are 16-byte where there is no column map and the input rows are
//                    aligned and even, 8-byte otherwise (so an even side keeps its 16-byte path when
//                    the other side is odd).  With a column map the rows of a batch are staged in LDS
//                    by coalesced 16-byte loads (the lanes of a row are lanes of one wave: fences, no
//                    barrier) and the output lanes gather from LDS; where the input rows are not
//                    16-byte aligned and even, or a workgroup's rows pass 63 KiB (A > 504), the lanes
//                    read 8-byte words straight from memory (CRDT_TUNE rxlds=0 forces that form; the
//                    A/B is in DESIGN.md 3.17).  A lane's first columns are looked up once per kernel, before
//                    its loop over states.  Without a column map an even, aligned input side beside an
//                    odd or unaligned output side keeps its 16-byte loads and stores 8-byte words.
//                    The loss test (bits 1 and 4) is a second loop over the INPUT rows that runs only
//                    when any[] says an index is dropped or V shrinks, and reads only dropped columns,
//                    dropped rows and dropped slots.
//   rx_bits_kernel   one wave per state: lane l of output word w tests input bit src[64 w + l], one
//                    ballot makes the word; 64 words are kept one per lane and stored together.  A
//                    NULL map copies words (the last one masked to the bits both sides have).
// The per-type calls chain these launches on the ctx stream; after the head kernel a launch's owner
// lane ORs its bits into status[s] only when it has any (one owner per state per launch).
#include "wire_common.hpp"

namespace crdt {

namespace {

constexpr unsigned kRxDropped = CRDT_REINDEX_DROPPED, kRxValues = CRDT_REINDEX_VALUES;

__device__ __forceinline__ u64 rx_ld1(const u64 *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ u64x2 rx_ld2(const u64 *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p));
}
__device__ __forceinline__ void rx_st1(u64 *p, u64 v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void rx_st2(u64 *p, u64x2 v) { __builtin_nontemporal_store(v, reinterpret_cast<u64x2 *>(p)); }

// ---- dictionaries -> axis map ------------------------------------------------------------------------
__global__ void rx_lost_init_kernel(uint32_t *n_lost, uint32_t n_old) { *n_lost = n_old; }

template <typename T>
__global__ __launch_bounds__(kBlock) void rx_map_kernel(const T *old_ids, unsigned long long n_old, const T *new_ids,
                                                        unsigned long long n_new, uint32_t *src, uint32_t *n_lost) {
  const unsigned long long j = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  bool found = false;
  if (j < n_new) {
    long long pos;
    if constexpr (sizeof(T) == 4) pos = find_u32(old_ids, n_old, new_ids[j], j);
    else pos = find_u64(old_ids, n_old, new_ids[j], j);
    found = pos >= 0;
    src[j] = found ? (uint32_t)pos : 0xFFFFFFFFu;
  }
  const unsigned n = (unsigned)__popcll(__ballot(found));  // the new dictionary is unique: each hit is another old id
  if (n && (threadIdx.x % kWave) == 0) atomicSub(n_lost, n);
}

// ---- the referenced input indices of up to two axes ---------------------------------------------------
struct RxAxis {
  const uint32_t *src;
  unsigned n_in, n_out;
  uint32_t *used;  // [n_in] in ctx scratch, or NULL: the axis drops nothing and has no map
};
struct RxPrep {
  RxAxis ax[2];
  uint32_t *any;  // [2]
};

__global__ __launch_bounds__(1024) void rx_prep_kernel(RxPrep p) {
  for (int x = 0; x < 2; ++x) {
    const RxAxis a = p.ax[x];
    if (!a.used) {
      if (threadIdx.x == 0) p.any[x] = 0;
      continue;
    }
    for (unsigned i = threadIdx.x; i < a.n_in; i += blockDim.x) a.used[i] = (!a.src && i < a.n_out) ? 1u : 0u;
    __syncthreads();
    if (a.src)
      for (unsigned j = threadIdx.x; j < a.n_out; j += blockDim.x) {
        const uint32_t s = a.src[j];
        if (s < a.n_in) a.used[s] = 1u;  // every writer stores the same word
      }
    __syncthreads();
    int dropped = 0;
    for (unsigned i = threadIdx.x; i < a.n_in; i += blockDim.x) dropped |= a.used[i] == 0;
    dropped = __syncthreads_or(dropped);
    if (threadIdx.x == 0) p.any[x] = dropped ? 1u : 0u;
  }
}

// ---- def_count and the status word's first store -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rx_head_kernel(const uint32_t *cnt, unsigned long long cap_in,
                                                         unsigned long long cap_out, uint32_t *out_cnt, uint32_t *status,
                                                         unsigned long long N) {
  const unsigned long long s = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  if (s >= N) return;
  const unsigned long long c = cnt ? cnt[s] : 0;
  unsigned bits = 0;
  unsigned long long oc = c;
  if (c > cap_in) bits = CRDT_REINDEX_INVALID, oc = 0;
  else if (c > cap_out) bits = CRDT_REINDEX_DCAP, oc = cap_out;
  if (out_cnt) out_cnt[s] = (uint32_t)oc;
  if (status) status[s] = bits;
}

// ---- rows --------------------------------------------------------------------------------------------
struct RxPlan {
  const u64 *in;
  u64 *out;
  unsigned long long N, in_ss, out_ss, in_ks, out_ks;  // state strides and outer-row strides, in words
  unsigned K_in, K_out, V_in, V_out, A_in, A_out;      // inner row v of outer row k starts at k * ks + v * A
  const uint32_t *row_src, *col_src;
  const uint32_t *cnt;  // the input's def_count or NULL: a count above cap_in makes the state the empty one
  unsigned long long cap_in, cap_out;
  int lim;  // the outer rows are deferred slots: the first min(cnt, cap_out) are gathered, cnt are tested
  const uint32_t *used_row, *used_col, *any;  // rx_prep_kernel's; any[0] columns, any[1] rows
  int scan_cols, scan_rows;                   // a dropped column / a dropped outer row with data sets bit 1
  uint32_t *status;
  int lg, lr;  // log2 of the lanes per state (8: a workgroup) and per row
};

// One 16-byte output piece (columns a, a + 1) of input row ir.  With a column map a0 / a1 are the two
// input columns; VI then means the row was staged in LDS (lrow) by 16-byte loads.
template <bool CM, bool VI>
__device__ __forceinline__ u64x2 rx_piece(const RxPlan &p, const u64 *ir, const u64 *lrow, unsigned a, uint32_t a0,
                                          uint32_t a1) {
  u64x2 t = {0, 0};
  if (CM) {
    if (a0 < p.A_in) t.x = VI ? lrow[a0] : rx_ld1(ir + a0);
    if (a1 < p.A_in) t.y = VI ? lrow[a1] : rx_ld1(ir + a1);
  } else if (VI) {
    if (a < p.A_in) t = rx_ld2(ir + a);  // A_in is even
  } else {
    if (a < p.A_in) t.x = rx_ld1(ir + a);
    if (a + 1 < p.A_in) t.y = rx_ld1(ir + a + 1);
  }
  return t;
}

constexpr int kRxRows = 4;  // rows per lane in flight before the first store

// lane g of the G lanes of state s; c0 / c1: the input columns of this lane's first output column(s) (the
// kernel looks them up once); returns this lane's share of the loss bits
template <bool CM, bool VI, bool VO>
__device__ __forceinline__ unsigned rx_state(const RxPlan &p, unsigned long long s, unsigned g, unsigned G, uint32_t c0,
                                             uint32_t c1) {
  constexpr int UR = kRxRows;
  constexpr bool STAGE = CM && VI;
  extern __shared__ u64 rx_lds[];  // STAGE: (kBlock >> lr) * kRxRows rows of A_in words
  const unsigned LR = 1u << p.lr, RP = G >> p.lr, gl = g & (LR - 1), gr = g >> p.lr;
  const unsigned long long c = p.cnt ? p.cnt[s] : 0;
  const bool invalid = c > p.cap_in;
  const unsigned live = p.lim ? (unsigned)(c < p.cap_out ? c : p.cap_out) : p.K_out;
  const u64 *__restrict__ ib = p.in + s * p.in_ss;
  u64 *__restrict__ ob = p.out + s * p.out_ss;
  const unsigned Rout = p.K_out * p.V_out;
  const unsigned af = VO ? 2 * gl : gl;  // this lane's first output column
  u64 *lbase = STAGE ? rx_lds + (unsigned long long)(threadIdx.x >> p.lr) * UR * p.A_in : nullptr;  // this row group's slots
  for (unsigned r0 = gr; r0 < Rout; r0 += UR * RP) {
    bool on[UR], ok[UR];
    const u64 *ir[UR];
    u64 *orow[UR];
#pragma unroll
    for (int q = 0; q < UR; ++q) {
      const unsigned r = r0 + q * RP;
      on[q] = r < Rout;
      ok[q] = false;
      ir[q] = ib;
      orow[q] = ob;
      if (on[q]) {
        const unsigned k = p.V_out == 1 ? r : r / p.V_out, v = r - k * p.V_out;
        const unsigned kin = p.row_src ? p.row_src[k] : k;
        ok[q] = !invalid && v < p.V_in && (p.lim ? k < live : kin < p.K_in);
        if (ok[q]) ir[q] = ib + kin * p.in_ks + (unsigned long long)v * p.A_in;
        orow[q] = ob + k * p.out_ks + (unsigned long long)v * p.A_out;
      }
    }
    if (STAGE) {  // the rows of this batch into LDS by coalesced 16-byte loads (A_in is even); the LR lanes
                  // of a row group are lanes of one wave, so fences order the exchange, no barrier
      for (unsigned a = 2 * gl; a < p.A_in; a += 2 * LR) {
        u64x2 t[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
          t[q] = u64x2{0, 0};
          if (ok[q]) t[q] = rx_ld2(ir[q] + a);
        }
#pragma unroll
        for (int q = 0; q < UR; ++q)
          if (ok[q]) *reinterpret_cast<u64x2 *>(lbase + (unsigned long long)q * p.A_in + a) = t[q];
      }
      wfence();
    }
    if (VO) {  // A_out is even
      for (unsigned a = 2 * gl; a < p.A_out; a += 2 * LR) {
        uint32_t a0 = c0, a1 = c1;
        if (CM && a != af) a0 = p.col_src[a], a1 = p.col_src[a + 1];
        u64x2 t[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
          t[q] = u64x2{0, 0};
          if (ok[q]) t[q] = rx_piece<CM, VI>(p, ir[q], STAGE ? lbase + (unsigned long long)q * p.A_in : nullptr, a, a0, a1);
        }
#pragma unroll
        for (int q = 0; q < UR; ++q)
          if (on[q]) rx_st2(orow[q] + a, t[q]);
      }
    } else if (!CM && VI) {  // an even, aligned input side beside an odd or unaligned output side: 16-byte
                             // loads, 8-byte stores
      for (unsigned a = 2 * gl; a < p.A_out; a += 2 * LR) {
        u64x2 t[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
          t[q] = u64x2{0, 0};
          if (ok[q] && a < p.A_in) t[q] = rx_ld2(ir[q] + a);  // A_in is even
        }
#pragma unroll
        for (int q = 0; q < UR; ++q)
          if (on[q]) {
            rx_st1(orow[q] + a, t[q].x);
            if (a + 1 < p.A_out) rx_st1(orow[q] + a + 1, t[q].y);
          }
      }
    } else {
      for (unsigned a = gl; a < p.A_out; a += LR) {
        uint32_t a0 = CM ? c0 : a;
        if (CM && a != af) a0 = p.col_src[a];
        u64 t[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
          t[q] = 0;
          if (ok[q] && a0 < p.A_in) t[q] = STAGE ? lbase[(unsigned long long)q * p.A_in + a0] : rx_ld1(ir[q] + a0);
        }
#pragma unroll
        for (int q = 0; q < UR; ++q)
          if (on[q]) rx_st1(orow[q] + a, t[q]);
      }
    }
    if (STAGE) wfence();  // the next batch overwrites the slots
  }
  // what the maps drop: only when an index is dropped at all (or V shrinks), and only those words
  if (invalid) return 0;
  const bool need_c = p.scan_cols && p.any[0] != 0, need_r = p.scan_rows && p.any[1] != 0, need_v = p.V_in > p.V_out;
  if (!(need_c || need_r || need_v)) return 0;
  u64 l1 = 0, l4 = 0;
  const unsigned Kscan = p.lim ? (unsigned)c : p.K_in;
  const unsigned long long Rin = (unsigned long long)Kscan * p.V_in;
  for (unsigned long long r = gr; r < Rin; r += RP) {
    const unsigned k = p.V_in == 1 ? (unsigned)r : (unsigned)(r / p.V_in), v = (unsigned)(r - (unsigned long long)k * p.V_in);
    const bool kept = p.used_row ? p.used_row[k] != 0 : true;
    const u64 *row = ib + k * p.in_ks + (unsigned long long)v * p.A_in;
    if (!kept) {
      if (need_r)
        for (unsigned a = gl; a < p.A_in; a += LR) l1 |= row[a];
    } else if (v >= p.V_out) {
      for (unsigned a = gl; a < p.A_in; a += LR) l4 |= row[a];
    } else if (need_c) {
      for (unsigned a = gl; a < p.A_in; a += LR)
        if (!p.used_col[a]) l1 |= row[a];
    }
  }
  return (l1 ? kRxDropped : 0u) | (l4 ? kRxValues : 0u);
}

template <bool CM, bool VI, bool VO>
__global__ __launch_bounds__(kBlock) void rx_rows_kernel(RxPlan p) {
  const int lane = threadIdx.x % kWave;
  // a lane's position in its row, and so its first output column(s), is the same for every row of every
  // state it handles: the map is read for them once per kernel
  uint32_t c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu;
  if (CM) {
    const unsigned gl = threadIdx.x & ((1u << p.lr) - 1), af = VO ? 2 * gl : gl;
    if (af < p.A_out) c0 = p.col_src[af];
    if (VO && af + 1 < p.A_out) c1 = p.col_src[af + 1];
  }
  if (p.lg == 8) {  // one workgroup per state
    __shared__ unsigned red[kBlock / kWave];
    for (unsigned long long s = blockIdx.x; s < p.N; s += gridDim.x) {  // workgroup-uniform
      const unsigned mine = rx_state<CM, VI, VO>(p, s, threadIdx.x, kBlock, c0, c1);
      const unsigned b = (__ballot(mine & kRxDropped) ? kRxDropped : 0u) | (__ballot(mine & kRxValues) ? kRxValues : 0u);
      if (lane == 0) red[threadIdx.x / kWave] = b;
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned bits = 0;
        for (int w = 0; w < kBlock / kWave; ++w) bits |= red[w];
        if (bits && p.status) p.status[s] |= bits;
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
    const bool on = s < p.N;
    const unsigned mine = on ? rx_state<CM, VI, VO>(p, s, g, G, c0, c1) : 0u;
    const bool b1 = ((__ballot(mine & kRxDropped) >> sshift) & smask) != 0;
    const bool b4 = ((__ballot(mine & kRxValues) >> sshift) & smask) != 0;
    if (on && g == 0 && (b1 || b4) && p.status) p.status[s] |= (b1 ? kRxDropped : 0u) | (b4 ? kRxValues : 0u);
  }
}

bool rx_al16(const void *p) { return (uintptr_t)p % 16 == 0; }

void launch_rx_rows(crdt_ctx *ctx, RxPlan p) {
  const bool cm = p.col_src != nullptr;
  const bool in16 = p.A_in % 2 == 0 && rx_al16(p.in) && (p.N == 1 || p.in_ss % 2 == 0) && (p.K_in <= 1 || p.in_ks % 2 == 0);
  const bool vo = p.A_out % 2 == 0 && rx_al16(p.out) && (p.N == 1 || p.out_ss % 2 == 0) && (p.K_out <= 1 || p.out_ks % 2 == 0);
  // a lane moves two columns per step with 16-byte stores, and with 16-byte loads beside 8-byte stores
  const unsigned long long row_pieces = std::max<unsigned long long>(1, (vo || (!cm && in16)) ? (p.A_out + 1ull) / 2 : p.A_out);
  const unsigned long long pieces = std::max<unsigned long long>(1, (unsigned long long)p.K_out * p.V_out * row_pieces);
  int lr = 0;
  while (lr < 6 && (1ull << lr) < row_pieces) ++lr;
  p.lr = lr;
  // a column map over 16-byte-aligned input rows: the rows staged in LDS, where a workgroup's rows fit
  const size_t lds = (size_t)(kBlock >> lr) * kRxRows * p.A_in * sizeof(u64);
  // (63 KiB: the kernel's own reduction words share the 64 KiB a launch may ask for without an attribute)
  const bool stage = cm && in16 && p.A_in > 0 && ctx->tune.rx_lds && lds <= (63u << 10);
  const bool vi = cm ? stage : in16;
  unsigned grid;
  if (pieces > 1024) {
    p.lg = 8;
    grid = (unsigned)std::min<unsigned long long>(p.N, (unsigned long long)ctx->cu_count * 32);
  } else {
    p.lg = std::max(lr, row_lr_log(pieces));
    const unsigned long long rpw = kWave >> p.lg, waves = (p.N + rpw - 1) / rpw;
    grid = (unsigned)std::min<unsigned long long>((waves + kBlock / kWave - 1) / (kBlock / kWave),
                                                  (unsigned long long)ctx->cu_count * 32);
  }
  hipStream_t s = ctx->stream;
  if (stage && vo) hipLaunchKernelGGL((rx_rows_kernel<true, true, true>), dim3(grid), dim3(kBlock), lds, s, p);
  else if (stage) hipLaunchKernelGGL((rx_rows_kernel<true, true, false>), dim3(grid), dim3(kBlock), lds, s, p);
  else if (cm && vo) hipLaunchKernelGGL((rx_rows_kernel<true, false, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (cm) hipLaunchKernelGGL((rx_rows_kernel<true, false, false>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (vo && vi) hipLaunchKernelGGL((rx_rows_kernel<false, true, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (vo) hipLaunchKernelGGL((rx_rows_kernel<false, false, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else if (vi) hipLaunchKernelGGL((rx_rows_kernel<false, true, false>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((rx_rows_kernel<false, false, false>), dim3(grid), dim3(kBlock), 0, s, p);
}

// ---- bitmaps -----------------------------------------------------------------------------------------
struct BxPlan {
  const u64 *in;
  u64 *out;
  unsigned long long N, in_ss, out_ss, in_rs, out_rs;  // state and slot strides, in words
  unsigned long long D_in, D_out;                      // slots per state (1: plain bitmap rows)
  unsigned U_in, U_out;
  const uint32_t *src, *cnt;
  unsigned long long cap_in;
  int lim;
  const uint32_t *used, *any;  // any[0] is this axis' word
  uint32_t *status;
};

__global__ __launch_bounds__(kBlock) void rx_bits_kernel(BxPlan p) {
  const unsigned lane = threadIdx.x % kWave;
  const unsigned long long wave0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwave = (unsigned long long)gridDim.x * (kBlock / kWave);
  const unsigned long long Wi = (p.U_in + 63ull) / 64, Wo = (p.U_out + 63ull) / 64;
  const unsigned Umin = p.U_in < p.U_out ? p.U_in : p.U_out;
  for (unsigned long long s = wave0; s < p.N; s += nwave) {  // wave-uniform
    const unsigned long long c = p.cnt ? p.cnt[s] : 0;
    const bool invalid = c > p.cap_in;
    const unsigned long long live = invalid ? 0 : (p.lim ? (c < p.D_out ? c : p.D_out) : p.D_out);
    const u64 *__restrict__ ib = p.in + s * p.in_ss;
    u64 *__restrict__ ob = p.out + s * p.out_ss;
    if (p.src) {
      for (unsigned long long d = 0; d < p.D_out; ++d) {
        const u64 *irow = ib + d * p.in_rs;
        for (unsigned long long wb = 0; wb < Wo; wb += kWave) {
          const unsigned nw = (unsigned)(Wo - wb < (unsigned long long)kWave ? Wo - wb : kWave);
          u64 mine = 0;
          if (d < live)
            for (unsigned q = 0; q < nw; ++q) {
              const unsigned long long j = (wb + q) * 64 + lane;
              const uint32_t sj = j < p.U_out ? p.src[j] : 0xFFFFFFFFu;
              const bool bit = sj < p.U_in && ((irow[sj >> 6] >> (sj & 63u)) & 1ull);
              const u64 m = __ballot(bit);
              if (lane == q) mine = m;
            }
          if (lane < nw) rx_st1(ob + d * p.out_rs + wb + lane, mine);
        }
      }
    } else {
      for (unsigned long long i = lane; i < p.D_out * Wo; i += kWave) {
        const unsigned long long d = i / Wo, w = i - d * Wo;
        u64 v = 0;
        if (d < live && w < Wi && w * 64 < Umin) {
          v = ib[d * p.in_rs + w];
          const unsigned long long valid = Umin - w * 64;
          if (valid < 64) v &= (1ull << valid) - 1;
        }
        rx_st1(ob + d * p.out_rs + w, v);
      }
    }
    if (invalid || !p.used || p.any[0] == 0) continue;
    const unsigned long long rows = p.lim ? c : p.D_in;
    u64 l1 = 0;
    for (unsigned long long iw = 0; iw < Wi; ++iw) {
      const unsigned long long j = iw * 64 + lane;
      const u64 kept = __ballot(j >= p.U_in || p.used[j] != 0);  // bits past U_in are no member's: never a loss
      for (unsigned long long d = lane; d < rows; d += kWave) l1 |= ib[d * p.in_rs + iw] & ~kept;
    }
    if (__ballot(l1 != 0) && lane == 0 && p.status) p.status[s] |= kRxDropped;
  }
}

void launch_rx_bits(crdt_ctx *ctx, const BxPlan &p) {
  const unsigned long long want = (p.N + kBlock / kWave - 1) / (kBlock / kWave);
  const unsigned grid = (unsigned)std::min<unsigned long long>(want, (unsigned long long)ctx->cu_count * 32);
  hipLaunchKernelGGL(rx_bits_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, p);
}

void launch_rx_head(crdt_ctx *ctx, const uint32_t *cnt, size_t cap_in, size_t cap_out, uint32_t *out_cnt, uint32_t *status,
                    size_t N) {
  if (!out_cnt && !status) return;
  hipLaunchKernelGGL(rx_head_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, cnt, cap_in,
                     cap_out, out_cnt, status, N);
}

// The used[] flags of up to two axes in ctx scratch: [any 4 words][used of axis 0][used of axis 1].  An
// axis with a NULL map that drops nothing (n_in <= n_out) gets no flags and costs nothing later.
struct RxUsed {
  const uint32_t *any = nullptr, *used[2] = {nullptr, nullptr};
};
int rx_prepare(crdt_ctx *ctx, const uint32_t *src0, size_t in0, size_t out0, const uint32_t *src1, size_t in1, size_t out1,
               RxUsed &u) {
  const bool need0 = src0 || in0 > out0, need1 = src1 || in1 > out1;
  if (!need0 && !need1) return CRDT_OK;  // pure growth: nothing can be dropped, no flags are read
  const int rc = ensure_scratch(ctx, (4 + in0 + in1) * sizeof(uint32_t));
  if (rc != CRDT_OK) return rc;
  uint32_t *base = static_cast<uint32_t *>(ctx->scratch);
  RxPrep p{};
  p.any = base;
  p.ax[0] = RxAxis{src0, (unsigned)in0, (unsigned)out0, need0 ? base + 4 : nullptr};
  p.ax[1] = RxAxis{src1, (unsigned)in1, (unsigned)out1, need1 ? base + 4 + in0 : nullptr};
  hipLaunchKernelGGL(rx_prep_kernel, dim3(1), dim3(1024), 0, ctx->stream, p);
  u.any = base;
  u.used[0] = p.ax[0].used;
  u.used[1] = p.ax[1].used;
  return CRDT_OK;
}

constexpr size_t kRxMax = 0x7fffffffull;  // per-state index ranges are u32 on the device

int rx_finish(crdt_ctx *ctx, const char *what) {
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, what);
  return CRDT_OK;
}

template <typename T>
int rx_map(crdt_ctx *ctx, const T *old_ids, size_t n_old, const T *new_ids, size_t n_new, uint32_t *src, uint32_t *n_lost,
           const char *what) {
  if ((n_old && !old_ids) || (n_new && (!new_ids || !src)) || !n_lost) return fail(ctx, CRDT_EINVAL, "%s: NULL argument", what);
  if (n_old > kRxMax || n_new > kRxMax) return fail(ctx, CRDT_EUNSUPPORTED, "%s: more than 2^31 - 1 ids", what);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "reindex_map");
  hipLaunchKernelGGL(rx_lost_init_kernel, dim3(1), dim3(1), 0, ctx->stream, n_lost, (uint32_t)n_old);
  if (n_new)
    hipLaunchKernelGGL((rx_map_kernel<T>), dim3((unsigned)((n_new + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       old_ids, (unsigned long long)n_old, new_ids, (unsigned long long)n_new, src, n_lost);
  return rx_finish(ctx, "reindex_map kernel launch");
}

}  // namespace

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_reindex_map_u32(crdt_ctx *ctx, const uint32_t *old_ids, size_t n_old, const uint32_t *new_ids, size_t n_new,
                         uint32_t *src, uint32_t *n_lost) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  return rx_map<uint32_t>(ctx, old_ids, n_old, new_ids, n_new, src, n_lost, "reindex_map_u32");
}

int crdt_reindex_map_u64(crdt_ctx *ctx, const uint64_t *old_ids, size_t n_old, const uint64_t *new_ids, size_t n_new,
                         uint32_t *src, uint32_t *n_lost) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  return rx_map<u64>(ctx, (const u64 *)old_ids, n_old, (const u64 *)new_ids, n_new, src, n_lost, "reindex_map_u64");
}

int crdt_rows_reindex(crdt_ctx *ctx, const uint64_t *in, size_t in_stride, size_t A_in, uint64_t *out, size_t out_stride,
                      size_t A_out, size_t planes, size_t N, const uint32_t *src, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (N == 0) return CRDT_OK;
  if (planes == 0 || planes > 64) return fail(ctx, CRDT_EUNSUPPORTED, "rows_reindex: planes = %zu not in [1, 64]", planes);
  if (A_in > kRxMax / planes || A_out > kRxMax / planes)
    return fail(ctx, CRDT_EUNSUPPORTED, "rows_reindex: planes * A past 2^31 - 1 words");
  if ((A_in && !in) || (A_out && !out)) return fail(ctx, CRDT_EINVAL, "rows_reindex: NULL rows");
  if (in && (const uint64_t *)out == in) return fail(ctx, CRDT_EINVAL, "rows_reindex: in and out are the same memory");
  if (N > 1 && (in_stride < planes * A_in || out_stride < planes * A_out))
    return fail(ctx, CRDT_EINVAL, "rows_reindex: a stride below planes * A");
  if (N > kRxMax) return fail(ctx, CRDT_EUNSUPPORTED, "rows_reindex: N too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "rows_reindex");
  RxUsed u;
  const int rc = rx_prepare(ctx, src, A_in, A_out, nullptr, 0, 0, u);
  if (rc != CRDT_OK) {
    timing_end(ctx);
    return rc;
  }
  launch_rx_head(ctx, nullptr, 0, 0, nullptr, status, N);
  RxPlan p{};
  p.in = (const u64 *)in, p.out = (u64 *)out;
  p.N = N, p.in_ss = in_stride, p.out_ss = out_stride;
  p.K_in = p.K_out = 1;
  p.V_in = p.V_out = (unsigned)planes;
  p.A_in = (unsigned)A_in, p.A_out = (unsigned)A_out;
  p.col_src = src;
  p.used_col = u.used[0], p.any = u.any;
  p.scan_cols = u.used[0] != nullptr;
  p.status = status;
  launch_rx_rows(ctx, p);
  return rx_finish(ctx, "rows_reindex kernel launch");
}

int crdt_bitmap_reindex(crdt_ctx *ctx, const uint64_t *in, size_t in_stride, size_t U_in, uint64_t *out, size_t out_stride,
                        size_t U_out, size_t N, const uint32_t *src, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (N == 0) return CRDT_OK;
  if (U_in > kRxMax || U_out > kRxMax) return fail(ctx, CRDT_EUNSUPPORTED, "bitmap_reindex: more than 2^31 - 1 bits");
  if ((U_in && !in) || (U_out && !out)) return fail(ctx, CRDT_EINVAL, "bitmap_reindex: NULL rows");
  if (in && (const uint64_t *)out == in) return fail(ctx, CRDT_EINVAL, "bitmap_reindex: in and out are the same memory");
  if (N > 1 && (in_stride < (U_in + 63) / 64 || out_stride < (U_out + 63) / 64))
    return fail(ctx, CRDT_EINVAL, "bitmap_reindex: a stride below the row's words");
  if (N > kRxMax) return fail(ctx, CRDT_EUNSUPPORTED, "bitmap_reindex: N too large");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "bitmap_reindex");
  RxUsed u;
  const int rc = rx_prepare(ctx, src, U_in, U_out, nullptr, 0, 0, u);
  if (rc != CRDT_OK) {
    timing_end(ctx);
    return rc;
  }
  launch_rx_head(ctx, nullptr, 0, 0, nullptr, status, N);
  BxPlan b{};
  b.in = (const u64 *)in, b.out = (u64 *)out;
  b.N = N, b.in_ss = in_stride, b.out_ss = out_stride;
  b.in_rs = (U_in + 63) / 64, b.out_rs = (U_out + 63) / 64;
  b.D_in = b.D_out = 1;
  b.U_in = (unsigned)U_in, b.U_out = (unsigned)U_out;
  b.src = src;
  b.used = u.used[0], b.any = u.any;
  b.status = status;
  launch_rx_bits(ctx, b);
  return rx_finish(ctx, "bitmap_reindex kernel launch");
}

int crdt_orswot_reindex(crdt_ctx *ctx, const crdt_orswot_states *in, const uint32_t *actor_src, const uint32_t *member_src,
                        const crdt_orswot_states *out, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!in || !out) return fail(ctx, CRDT_EINVAL, "orswot_reindex: NULL states");
  if (in->N != out->N) return fail(ctx, CRDT_EINVAL, "orswot_reindex: in and out differ in N");
  const size_t N = in->N;
  if (N == 0) return CRDT_OK;
  for (const crdt_orswot_states *st : {in, out}) {
    const size_t M = st->M, A = st->A, Mw = (M + 63) / 64;
    if (A > kRxMax || M > kRxMax || st->Dcap > kRxMax || N > kRxMax)
      return fail(ctx, CRDT_EUNSUPPORTED, "orswot_reindex: a dimension past 2^31 - 1");
    if (A && (!st->clock || (M && !st->entries))) return fail(ctx, CRDT_EINVAL, "orswot_reindex: NULL clock / entries");
    if (N > 1 && st->clock_stride < A) return fail(ctx, CRDT_EINVAL, "orswot_reindex: clock_stride < A");
    if (M > 1 && st->entry_mstride < A) return fail(ctx, CRDT_EINVAL, "orswot_reindex: entry_mstride < A");
    if (N > 1 && M && st->entry_sstride < (M - 1) * st->entry_mstride + A)
      return fail(ctx, CRDT_EINVAL, "orswot_reindex: entry_sstride below the state size");
    if (st->Dcap && (!st->def_count || (A && !st->def_clock) || (Mw && !st->def_members)))
      return fail(ctx, CRDT_EINVAL, "orswot_reindex: NULL deferred buffers with Dcap > 0");
  }
  if ((in->clock && in->clock == out->clock) || (in->entries && in->entries == out->entries) ||
      (in->def_clock && in->def_clock == out->def_clock) || (in->def_members && in->def_members == out->def_members) ||
      (in->def_count && in->def_count == out->def_count))
    return fail(ctx, CRDT_EINVAL, "orswot_reindex: in and out share a buffer (the call is out of place)");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "orswot_reindex");
  RxUsed u;
  const int rc = rx_prepare(ctx, actor_src, in->A, out->A, member_src, in->M, out->M, u);
  if (rc != CRDT_OK) {
    timing_end(ctx);
    return rc;
  }
  const uint32_t *cnt = in->def_count;  // read whenever given, as the eq calls do
  launch_rx_head(ctx, cnt, in->Dcap, out->Dcap, out->def_count, status, N);
  RxPlan p{};
  p.N = N;
  p.A_in = (unsigned)in->A, p.A_out = (unsigned)out->A;
  p.V_in = p.V_out = 1;
  p.col_src = actor_src;
  p.cnt = cnt, p.cap_in = in->Dcap, p.cap_out = out->Dcap;
  p.used_col = u.used[0], p.any = u.any;
  p.scan_cols = u.used[0] != nullptr;
  p.status = status;
  {  // the clock
    RxPlan c = p;
    c.in = (const u64 *)in->clock, c.out = (u64 *)out->clock;
    c.in_ss = in->clock_stride, c.out_ss = out->clock_stride;
    c.K_in = c.K_out = 1;
    launch_rx_rows(ctx, c);
  }
  if (in->M || out->M) {  // the member rows
    RxPlan e = p;
    e.in = (const u64 *)in->entries, e.out = (u64 *)out->entries;
    e.in_ss = in->entry_sstride, e.out_ss = out->entry_sstride;
    e.in_ks = in->entry_mstride, e.out_ks = out->entry_mstride;
    e.K_in = (unsigned)in->M, e.K_out = (unsigned)out->M;
    e.row_src = member_src;
    e.used_row = u.used[1];
    e.scan_rows = u.used[1] != nullptr;
    launch_rx_rows(ctx, e);
  }
  if (in->Dcap || out->Dcap) {  // the deferred slots: clocks by column, member sets by bit
    RxPlan d = p;
    d.in = (const u64 *)in->def_clock, d.out = (u64 *)out->def_clock;
    d.in_ss = in->Dcap * in->A, d.out_ss = out->Dcap * out->A;
    d.in_ks = in->A, d.out_ks = out->A;
    d.K_in = (unsigned)in->Dcap, d.K_out = (unsigned)out->Dcap;
    d.lim = 1;
    launch_rx_rows(ctx, d);
    BxPlan b{};
    const size_t Wi = (in->M + 63) / 64, Wo = (out->M + 63) / 64;
    b.in = (const u64 *)in->def_members, b.out = (u64 *)out->def_members;
    b.N = N, b.in_ss = in->Dcap * Wi, b.out_ss = out->Dcap * Wo, b.in_rs = Wi, b.out_rs = Wo;
    b.D_in = in->Dcap, b.D_out = out->Dcap;
    b.U_in = (unsigned)in->M, b.U_out = (unsigned)out->M;
    b.src = member_src, b.cnt = cnt, b.cap_in = in->Dcap, b.lim = 1;
    b.used = u.used[1], b.any = u.any ? u.any + 1 : nullptr;
    b.status = status;
    launch_rx_bits(ctx, b);
  }
  return rx_finish(ctx, "orswot_reindex kernel launch");
}

int crdt_mvreg_reindex(crdt_ctx *ctx, const crdt_mvreg_states *in, const uint32_t *actor_src, const crdt_mvreg_states *out,
                       uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!in || !out) return fail(ctx, CRDT_EINVAL, "mvreg_reindex: NULL states");
  if (in->N != out->N) return fail(ctx, CRDT_EINVAL, "mvreg_reindex: in and out differ in N");
  const size_t N = in->N;
  if (N == 0) return CRDT_OK;
  for (const crdt_mvreg_states *st : {in, out}) {
    if (st->V == 0 || st->V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_reindex: V = %zu not in [1, 64]", st->V);
    if (st->A > kRxMax / 64 || N > kRxMax) return fail(ctx, CRDT_EUNSUPPORTED, "mvreg_reindex: a dimension too large");
    if (!st->vval || (st->A && !st->vclk)) return fail(ctx, CRDT_EINVAL, "mvreg_reindex: NULL register buffers");
    if (N > 1 && (st->vclk_stride < st->V * st->A || st->vval_stride < st->V))
      return fail(ctx, CRDT_EINVAL, "mvreg_reindex: strides below the register size");
  }
  if ((in->vclk && in->vclk == out->vclk) || in->vval == out->vval)
    return fail(ctx, CRDT_EINVAL, "mvreg_reindex: in and out share a buffer (the call is out of place)");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "mvreg_reindex");
  RxUsed u;
  const int rc = rx_prepare(ctx, actor_src, in->A, out->A, nullptr, 0, 0, u);
  if (rc != CRDT_OK) {
    timing_end(ctx);
    return rc;
  }
  launch_rx_head(ctx, nullptr, 0, 0, nullptr, status, N);
  RxPlan p{};
  p.N = N;
  p.K_in = p.K_out = 1;
  p.any = u.any;
  p.status = status;
  {  // the value clocks: slot v to slot v, columns through the map
    RxPlan c = p;
    c.in = (const u64 *)in->vclk, c.out = (u64 *)out->vclk;
    c.in_ss = in->vclk_stride, c.out_ss = out->vclk_stride;
    c.V_in = (unsigned)in->V, c.V_out = (unsigned)out->V;
    c.A_in = (unsigned)in->A, c.A_out = (unsigned)out->A;
    c.col_src = actor_src;
    c.used_col = u.used[0];
    c.scan_cols = u.used[0] != nullptr;
    launch_rx_rows(ctx, c);
  }
  {  // the values: a row of V words per register
    RxPlan v = p;
    v.in = (const u64 *)in->vval, v.out = (u64 *)out->vval;
    v.in_ss = in->vval_stride, v.out_ss = out->vval_stride;
    v.V_in = v.V_out = 1;
    v.A_in = (unsigned)in->V, v.A_out = (unsigned)out->V;
    v.status = nullptr;
    launch_rx_rows(ctx, v);
  }
  return rx_finish(ctx, "mvreg_reindex kernel launch");
}

int crdt_map_reindex(crdt_ctx *ctx, const crdt_map_states *in, const crdt_map_deferred *in_def, const uint32_t *actor_src,
                     const uint32_t *key_src, const crdt_map_states *out, const crdt_map_deferred *out_def,
                     uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!in || !out) return fail(ctx, CRDT_EINVAL, "map_reindex: NULL states");
  if (in->N != out->N) return fail(ctx, CRDT_EINVAL, "map_reindex: in and out differ in N");
  const size_t N = in->N;
  if (N == 0) return CRDT_OK;
  for (int side = 0; side < 2; ++side) {
    const crdt_map_states *st = side ? out : in;
    const crdt_map_deferred *df = side ? out_def : in_def;
    const size_t K = st->K, A = st->A, Kw = (K + 63) / 64;
    if (st->V == 0 || st->V > 64) return fail(ctx, CRDT_EUNSUPPORTED, "map_reindex: V = %zu not in [1, 64]", st->V);
    if (A > kRxMax / 64 || K > kRxMax / 64 || N > kRxMax || (df && df->Dcap > kRxMax))
      return fail(ctx, CRDT_EUNSUPPORTED, "map_reindex: a dimension too large");
    if ((A && !st->clock) || (K && !st->vval) || (K && A && (!st->ec || !st->vclk)))
      return fail(ctx, CRDT_EINVAL, "map_reindex: NULL state buffers");
    if (N > 1 && (st->clock_stride < A || st->ec_stride < K * A || st->vclk_stride < K * st->V * A ||
                  st->vval_stride < K * st->V))
      return fail(ctx, CRDT_EINVAL, "map_reindex: strides below the state size");
    if (df && df->Dcap && (!df->count || (A && !df->clock) || (Kw && !df->keys)))
      return fail(ctx, CRDT_EINVAL, "map_reindex: NULL deferred buffers with Dcap > 0");
  }
  const size_t icap = in_def ? in_def->Dcap : 0, ocap = out_def ? out_def->Dcap : 0;
  if ((in->clock && in->clock == out->clock) || (in->ec && in->ec == out->ec) || (in->vclk && in->vclk == out->vclk) ||
      (in->vval && in->vval == out->vval) ||
      (in_def && out_def &&
       ((in_def->clock && in_def->clock == out_def->clock) || (in_def->keys && in_def->keys == out_def->keys) ||
        (in_def->count && in_def->count == out_def->count))))
    return fail(ctx, CRDT_EINVAL, "map_reindex: in and out share a buffer (the call is out of place)");
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  timing_begin(ctx, "map_reindex");
  RxUsed u;
  const int rc = rx_prepare(ctx, actor_src, in->A, out->A, key_src, in->K, out->K, u);
  if (rc != CRDT_OK) {
    timing_end(ctx);
    return rc;
  }
  const uint32_t *cnt = in_def ? in_def->count : nullptr;
  launch_rx_head(ctx, cnt, icap, ocap, out_def ? out_def->count : nullptr, status, N);
  RxPlan p{};
  p.N = N;
  p.A_in = (unsigned)in->A, p.A_out = (unsigned)out->A;
  p.V_in = p.V_out = 1;
  p.K_in = p.K_out = 1;
  p.col_src = actor_src;
  p.cnt = cnt, p.cap_in = icap, p.cap_out = ocap;
  p.used_col = u.used[0], p.any = u.any;
  p.scan_cols = u.used[0] != nullptr;
  p.status = status;
  {  // the clock
    RxPlan c = p;
    c.in = (const u64 *)in->clock, c.out = (u64 *)out->clock;
    c.in_ss = in->clock_stride, c.out_ss = out->clock_stride;
    launch_rx_rows(ctx, c);
  }
  if (in->K || out->K) {
    RxPlan e = p;  // the entry clocks: a dropped key with a non-zero row is a loss
    e.in = (const u64 *)in->ec, e.out = (u64 *)out->ec;
    e.in_ss = in->ec_stride, e.out_ss = out->ec_stride;
    e.in_ks = in->A, e.out_ks = out->A;
    e.K_in = (unsigned)in->K, e.K_out = (unsigned)out->K;
    e.row_src = key_src;
    e.used_row = u.used[1];
    e.scan_rows = u.used[1] != nullptr;
    launch_rx_rows(ctx, e);
    RxPlan v = e;  // the value clocks of the kept keys: slot v to slot v
    v.in = (const u64 *)in->vclk, v.out = (u64 *)out->vclk;
    v.in_ss = in->vclk_stride, v.out_ss = out->vclk_stride;
    v.in_ks = in->V * in->A, v.out_ks = out->V * out->A;
    v.V_in = (unsigned)in->V, v.V_out = (unsigned)out->V;
    v.scan_rows = 0;
    launch_rx_rows(ctx, v);
    RxPlan w = p;  // the values: a row of V words per key
    w.in = (const u64 *)in->vval, w.out = (u64 *)out->vval;
    w.in_ss = in->vval_stride, w.out_ss = out->vval_stride;
    w.in_ks = in->V, w.out_ks = out->V;
    w.K_in = (unsigned)in->K, w.K_out = (unsigned)out->K;
    w.A_in = (unsigned)in->V, w.A_out = (unsigned)out->V;
    w.row_src = key_src;
    w.col_src = nullptr, w.used_col = nullptr, w.scan_cols = 0;
    w.status = nullptr;
    launch_rx_rows(ctx, w);
  }
  if (icap || ocap) {
    RxPlan d = p;
    d.in = icap ? (const u64 *)in_def->clock : nullptr, d.out = ocap ? (u64 *)out_def->clock : nullptr;
    d.in_ss = icap * in->A, d.out_ss = ocap * out->A;
    d.in_ks = in->A, d.out_ks = out->A;
    d.K_in = (unsigned)icap, d.K_out = (unsigned)ocap;
    d.lim = 1;
    launch_rx_rows(ctx, d);
    BxPlan b{};
    const size_t Wi = (in->K + 63) / 64, Wo = (out->K + 63) / 64;
    b.in = icap ? (const u64 *)in_def->keys : nullptr, b.out = ocap ? (u64 *)out_def->keys : nullptr;
    b.N = N, b.in_ss = icap * Wi, b.out_ss = ocap * Wo, b.in_rs = Wi, b.out_rs = Wo;
    b.D_in = icap, b.D_out = ocap;
    b.U_in = (unsigned)in->K, b.U_out = (unsigned)out->K;
    b.src = key_src, b.cnt = cnt, b.cap_in = icap, b.lim = 1;
    b.used = u.used[1], b.any = u.any ? u.any + 1 : nullptr;
    b.status = status;
    launch_rx_bits(ctx, b);
  }
  return rx_finish(ctx, "map_reindex kernel launch");
}

}  // extern "C"
