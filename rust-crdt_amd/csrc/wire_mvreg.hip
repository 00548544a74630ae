// Serde wire format of MVReg<u64, u32> on its own (outside a Map), on the device:
//   crdt_mvreg_ingest / _egress          register frames <-> the dense crdt_mvreg_states
//   crdt_mvreg_ops_ingest / _ops_egress  Vec<mvreg::Op> frames <-> the batches of crdt_mvreg_apply_batch
// The bincode 1.x rules of wire.hip / wire_ops.hip; in 32-bit words:
//   MVReg<u64, u32>      = u64 n, n x (VClock clock, u64 val), values in Vec order   (mvreg.rs:32-35)
//   mvreg::Op<u64, u32>  = u32 0 (Put), VClock clock, u64 val                         (mvreg.rs:38-47)
//   frame of register i  = the MVReg, or Vec<Op>: u64 n_ops, then the ops back to back
//
// States: one wave per frame.  The register is parsed by parse_mvreg (wire_common.hpp), the parser a
// Map frame's values go through, and written by write_mvreg, the Map egress's writer: the record loop
// of each VClock runs across lanes, rows are assembled in the wave's LDS row and stored coalesced.
// Unlike a Map value slot, a standalone register is compacted on the way in: a value whose clock is
// empty (it has no dense form) is dropped and the next one takes its slot.
//
// Op streams: count -> exclusive scan -> finalize (capacities) -> fill, one wave per frame, with
// the frame walk of wire_ops.hip (OpWalk: tags and counts through the LDS ring) and its batched
// parse (every 64 ops found, lane = op; a clock of more than 64 records by the wave).  A Put has one
// clock row and no id list, so rows == ops, clk_row[o] = o and one scan serves both.
#include "wire_ops_common.hpp"

namespace crdt {

constexpr unsigned kWireEmptyClock = 8u;  // state ingest: a value with an empty clock was dropped
constexpr int kMvWpb = kBlock / kWave;
constexpr size_t kMvLdsMax = 64 << 10;

static_assert(sizeof(crdt_mvreg_ops) == sizeof(crdt_mvreg_ops_buf), "crdt_mvreg_ops_buf");
static_assert(offsetof(crdt_mvreg_ops, n_clk_rows) == offsetof(crdt_mvreg_ops_buf, row_cap), "crdt_mvreg_ops_buf");
static_assert(offsetof(crdt_mvreg_ops, val) == offsetof(crdt_mvreg_ops_buf, val), "crdt_mvreg_ops_buf");

// ---- states ---------------------------------------------------------------------------------------
struct MvWirePlan {
  const uint8_t *bytes;
  const u64 *frame_off;
  unsigned long long N, A, V, cs, vs;
  const uint32_t *actors;
  u64 *vclk, *vval;
  uint32_t *status;
  int stage;  // the actor dictionary staged in LDS
  // egress
  u64 *sizes;
  const u64 *frame_out;
  uint8_t *out;
};

// One wave per frame.  Every slot of the register is written: the values kept from slot 0 in Vec
// order, the rest zero (a malformed frame: all of them).
__global__ __launch_bounds__(kBlock) void mvreg_ingest_kernel(MvWirePlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  const int wpb = blockDim.x / kWave;
  const uint32_t *actors = p.actors;
  u64 *base = lds;
  if (p.stage) {
    uint32_t *la = reinterpret_cast<uint32_t *>(lds);
    for (unsigned long long i = threadIdx.x; i < p.A; i += blockDim.x) la[i] = p.actors[i];
    __syncthreads();
    actors = la;
    base = lds + (p.A + 1) / 2;
  }
  u64 *row = base + (unsigned long long)wib * p.A;
  for (unsigned long long s = (unsigned long long)blockIdx.x * wpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * wpb) {
    unsigned st = 0;
    unsigned long long n = 0;  // slots taken
    u64 *vc = p.vclk + s * p.cs, *vv = p.vval + s * p.vs;
    Frame f;
    const u64 b = p.frame_off[s], e = p.frame_off[s + 1];
    if ((b & 3) || (e & 3) || e < b) {
      st = kWireBad;
    } else {
      f.w = reinterpret_cast<const uint32_t *>(p.bytes + b);
      f.nw = (e - b) / 4;
      const unsigned long long k = parse_mvreg(f, 0, actors, p.A, row, lane, st, [&](u64, u64 val) {
        if (nnz_row(row, p.A, lane) == 0) {
          st |= kWireEmptyClock;
        } else if (n < p.V) {
          store_row<u64>(vc + n * p.A, row, p.A, lane);
          if (lane == 0) vv[n] = val;
          ++n;
        } else {
          st |= kWireCap;
        }
      });
      if (k != f.nw) {  // truncated (~0) or trailing bytes
        st |= kWireBad;
        n = 0;
      }
    }
    // (a slot stored above and zeroed here is written by the same lanes, in this order)
    for (unsigned long long x = n * p.A + lane; x < p.V * p.A; x += kWave) vc[x] = 0;
    for (unsigned long long x = n + lane; x < p.V; x += kWave) vv[x] = 0;
    if (lane == 0) p.status[s] = st;
  }
}

// Count (write = 0: frame sizes) or write pass, one wave per register.
__global__ __launch_bounds__(kBlock) void mvreg_egress_kernel(MvWirePlan p, int write) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nw = (unsigned long long)gridDim.x * kMvWpb;
  for (unsigned long long s = w0; s < p.N; s += nw) {
    const u64 *vc = p.vclk + s * p.cs;
    u64 m = 0;
    const u64 vsz = mvreg_wire_size(vc, p.V, p.A, lane, m);
    if (!write) {
      if (lane == 0) p.sizes[s] = 8 + vsz;
      continue;
    }
    write_mvreg(reinterpret_cast<uint32_t *>(p.out + p.frame_out[s]), 0, vc, p.vval + s * p.vs, p.V, p.A, p.actors, m,
                lane);
  }
}

// ---- Put streams: ingest ----------------------------------------------------------------------------
struct MvOpsPlan {
  const uint8_t *bytes;
  const u64 *frame_off;
  unsigned long long N, A;
  const uint32_t *actors;
  unsigned long long dict_words;  // > 0: the actor dictionary is staged in LDS (this many u64 words)
  u64 *counts;                    // [N] ops of every frame (count pass)
  const u64 *op_off;              // [N+1], final (after the capacities)
  uint32_t *status;
  uint32_t *row;  // clk_row
  u64 *pool;      // clk_pool, [rows][A]
  u64 *val;
};

// The walk over one frame (nw >= 2 words): emit(pos, n) for every Put, in order, with pos its first
// word and n its clock's records.  Every count is tested against the words left before anything
// depends on it.  False: malformed (truncated, trailing words, a count that cannot fit, a tag other
// than Put).
template <class F>
__device__ __forceinline__ bool walk_puts(OpWalk &w, int lane, F &&emit) {
  const unsigned long long nw = w.nw;
  const u64 n_ops = w.at64(0, lane);
  if (n_ops > (nw - 2) / 5) return false;  // the smallest Put takes 20 bytes
  unsigned long long k = 2;
  for (u64 i = 0; i < n_ops; ++i) {
    if (k + 3 > nw) return false;
    if (w.at(k, lane) != 0) return false;
    const u64 n = w.at64(k + 1, lane);
    if (n > (nw - k - 3) / 3) return false;
    const unsigned long long next = k + 3 + 3 * n + 2;
    if (next > nw) return false;
    emit(k, uni64(n));
    k = uni64(next);
  }
  return k == nw;
}

__device__ __forceinline__ bool puts_frame(const MvOpsPlan &p, unsigned long long s, OpWalk &w, uint32_t *ring) {
  const u64 b = p.frame_off[s], e = p.frame_off[s + 1];
  if ((b & 3) || (e & 3) || e < b || e - b < 8) return false;
  w.fw = reinterpret_cast<const uint32_t *>(p.bytes + b);
  w.nw = (e - b) / 4;
  w.nwin = (w.nw + kWalkWin - 1) / kWalkWin;
  w.ring = ring;
  return true;
}

__global__ __launch_bounds__(kBlock) void mvops_count_kernel(MvOpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  uint32_t *ring = reinterpret_cast<uint32_t *>(lds) + (size_t)wib * kWalkRing * kWalkWin;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kMvWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kMvWpb) {
    unsigned st = 0;
    u64 no = 0;
    OpWalk w;
    if (!puts_frame(p, s, w, ring)) {
      st = kWireBad;
    } else {
      w.start(lane);
      const bool ok = walk_puts(w, lane, [&](unsigned long long, unsigned long long) { ++no; });
      wire_vmcnt<0>();  // no DMA of this frame may land in the ring after the next one starts
      if (!ok) {
        st = kWireBad;
        no = 0;
      }
    }
    if (lane == 0) {
      p.status[s] = st;
      p.counts[s] = no;
    }
  }
}

__global__ __launch_bounds__(kBlock) void mvops_fill_kernel(MvOpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  const uint32_t *actors = p.actors;
  u64 *base = lds;
  if (p.dict_words) {
    uint32_t *la = reinterpret_cast<uint32_t *>(lds);
    for (unsigned long long i = threadIdx.x; i < p.A; i += blockDim.x) la[i] = p.actors[i];
    __syncthreads();
    actors = la;
    base = lds + p.dict_words;
  }
  uint32_t *ring = reinterpret_cast<uint32_t *>(base) + (size_t)wib * kWalkRing * kWalkWin;
  const unsigned long long A = p.A;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kMvWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kMvWpb) {
    const unsigned st = p.status[s];
    const u64 o0 = p.op_off[s];
    OpWalk w;
    if ((st & (kWireBad | kWireCap)) || p.op_off[s + 1] == o0 || !puts_frame(p, s, w, ring)) continue;
    w.start(lane);
    const uint32_t *fw = w.fw;
    // the batch of Puts the lanes parse next: lane i holds Put i of it
    int cnt = 0;
    u64 done = 0;
    unsigned long long d_pos = 0, d_n = 0;
    bool miss = false;
    auto flush = [&]() {
      // the batch's clock rows are contiguous: zeroed here, coalesced, and landed before the records
      u64 *rows = p.pool + (o0 + done) * A;
      const unsigned long long nz = (unsigned long long)cnt * A;
      for (unsigned long long x = lane; x < nz; x += kWave) rows[x] = 0;
      wire_vmcnt<0>();
      const bool on = lane < cnt;
      const u64 o = o0 + done + lane;
      if (on) {
        p.row[o] = (uint32_t)o;
        p.val[o] = rd64(fw, d_pos + 3 + 3 * d_n);
        u64 *dst = p.pool + o * A;
        for (unsigned long long r = 0; r < (d_n <= (unsigned long long)kWave ? d_n : 0); ++r) {
          const uint32_t id = fw[d_pos + 3 + 3 * r];
          const u64 c = rd64(fw, d_pos + 4 + 3 * r);
          const long long col = find_u32(actors, A, id, r);
          if (col < 0) miss = true;
          else dst[col] = c;
        }
      }
      // a clock with more records than a lane takes: the wave loops over them
      u64 wclk = __ballot(on && d_n > (unsigned long long)kWave);
      while (wclk) {
        const int j = __ffsll((unsigned long long)wclk) - 1;
        wclk &= wclk - 1;
        const unsigned long long jr = __shfl(d_pos, j, kWave) + 3, jn = __shfl(d_n, j, kWave);
        u64 *dst = p.pool + (o0 + done + j) * A;
        for (unsigned long long r = lane; r < jn; r += kWave) {
          const long long col = find_u32(actors, A, fw[jr + 3 * r], r);
          if (col < 0) miss = true;
          else dst[col] = rd64(fw, jr + 3 * r + 1);
        }
      }
      done += cnt;
      cnt = 0;
    };
    walk_puts(w, lane, [&](unsigned long long pos, unsigned long long n) {
      if (lane == cnt) {
        d_pos = pos;
        d_n = n;
      }
      if (++cnt == kWave) flush();
    });
    if (cnt) flush();
    wire_vmcnt<0>();
    if (__ballot(miss) && lane == 0) p.status[s] = st | kWireMissing;
  }
}

// ---- Put streams: egress ----------------------------------------------------------------------------
struct MvOpsEgressPlan {
  unsigned long long N, A, n_ops, n_rows;
  const u64 *op_off;
  const uint32_t *row;
  const u64 *pool, *val;
  const uint32_t *actors;
  u64 *sizes;
  const u64 *frame_off;
  uint8_t *bytes;
  uint32_t *status;
};

// One wave per register, lane = op in batches of 64.  write = 0: validate every op, size the frame
// (status[s], sizes[s]); write = 1: write it at frame_off[s] (the empty Vec for a register with bit 1).
__global__ __launch_bounds__(kBlock) void mvops_egress_kernel(MvOpsEgressPlan p, int write) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwv = (unsigned long long)gridDim.x * kMvWpb;
  const unsigned long long A = p.A;
  for (unsigned long long s = w0; s < p.N; s += nwv) {
    const u64 b = p.op_off[s], e = p.op_off[s + 1];
    bool bad = e < b || e > p.n_ops;
    uint32_t *out = nullptr;
    if (write) {
      out = reinterpret_cast<uint32_t *>(p.bytes + p.frame_off[s]);
      if (p.status[s] != 0) {
        if (lane == 0) wr64(out, 0, 0);
        continue;
      }
      if (lane == 0) wr64(out, 0, e - b);
    }
    u64 run = 2;
    for (u64 ob = b; ob < e && !bad; ob += kWave) {
      const u64 o = ob + lane;
      const bool on = o < e;
      unsigned long long r = 0;
      bool has_row = false;
      if (on) {
        r = p.row[o];
        has_row = r < p.n_rows;
      }
      if (__ballot(on && !has_row)) bad = true;
      // non-zeros of every op's clock row: the wave reads one row at a time, coalesced
      unsigned long long nnz = 0;
      u64 rows = __ballot(has_row);
      while (rows) {
        const int j = __ffsll((unsigned long long)rows) - 1;
        rows &= rows - 1;
        const u64 c = nnz_row(p.pool + __shfl(r, j, kWave) * A, A, lane);
        if (lane == j) nnz = c;
      }
      u64 total;
      const u64 kp = run + wave_excl(on ? 5 + 3 * nnz : 0, lane, total);
      run += total;
      if (!write || bad) continue;
      if (on) {  // tag and value, by the op's lane
        out[kp] = 0;
        wr64(out, kp + 3 + 3 * nnz, p.val[o]);
      }
      rows = __ballot(has_row);
      while (rows) {  // clocks, by the wave
        const int j = __ffsll((unsigned long long)rows) - 1;
        rows &= rows - 1;
        write_vclock(out, __shfl(kp, j, kWave) + 1, p.pool + __shfl(r, j, kWave) * A, A, p.actors, lane);
      }
    }
    if (!write && lane == 0) {
      p.status[s] = bad ? kWireMissing : 0u;
      p.sizes[s] = bad ? 8 : run * 4;
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------
static int mv_wire_plan(crdt_ctx *ctx, const crdt_mvreg_states *st, const uint32_t *actors, MvWirePlan &p,
                        const char *what) {
  if (!st || !actors) return fail(ctx, CRDT_EINVAL, "%s: NULL states / actors", what);
  if (st->A == 0 || st->V == 0) return fail(ctx, CRDT_EINVAL, "%s: need A, V >= 1", what);
  if (st->N && (!st->vclk || !st->vval)) return fail(ctx, CRDT_EINVAL, "%s: NULL register buffers", what);
  if (st->N > 1 && (st->vclk_stride < st->V * st->A || st->vval_stride < st->V))
    return fail(ctx, CRDT_EINVAL, "%s: strides below the register size", what);
  if (st->A > (size_t)kWireRowLds) return fail(ctx, CRDT_EUNSUPPORTED, "%s: A = %zu > %d", what, st->A, kWireRowLds);
  p = MvWirePlan{};
  p.N = st->N;
  p.A = st->A;
  p.V = st->V;
  p.cs = st->vclk_stride;
  p.vs = st->vval_stride;
  p.actors = actors;
  p.vclk = (u64 *)st->vclk;
  p.vval = (u64 *)st->vval;
  return CRDT_OK;
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_mvreg_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N, const uint32_t *actors,
                      size_t A, const crdt_mvreg_states *out, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (N == 0) return CRDT_OK;
  MvWirePlan p;
  if (int rc = mv_wire_plan(ctx, out, actors, p, "mvreg_ingest")) return rc;
  if (out->N != N || out->A != A) return fail(ctx, CRDT_EINVAL, "mvreg_ingest: out holds %zu registers of %zu actors, not %zu of %zu", out->N, out->A, N, A);
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.status = status;
  int wpb = kMvWpb;
  while (wpb > 1 && (size_t)wpb * A * 8 > kMvLdsMax) --wpb;
  const size_t dw = (A + 1) / 2;
  p.stage = (dw + wpb * A) * 8 <= kMvLdsMax;
  const size_t lds = ((p.stage ? dw : 0) + wpb * A) * 8;
  timing_begin(ctx, "wire_mvreg_ingest");
  hipLaunchKernelGGL(mvreg_ingest_kernel, dim3(wave_grid(ctx, N, wpb, 32)), dim3(wpb * kWave), lds, ctx->stream, p);
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

int crdt_mvreg_egress(crdt_ctx *ctx, const crdt_mvreg_states *states, const uint32_t *actors, uint64_t *frame_off,
                      uint8_t *bytes, size_t cap, size_t *total) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  MvWirePlan p;
  if (int rc = mv_wire_plan(ctx, states, actors, p, "mvreg_egress")) return rc;
  const size_t N = p.N;
  if (N == 0) return CRDT_OK;
  if (!frame_off || !total) return fail(ctx, CRDT_EINVAL, "mvreg_egress: need frame_off and total");
  return two_pass_egress(ctx, "wire_mvreg_egress", mvreg_egress_kernel, p, wave_grid(ctx, N, kMvWpb, 32), frame_off, bytes, cap,
                         total, StatePlanOut{});
}

int crdt_mvreg_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                          const uint32_t *actors, size_t A, const crdt_mvreg_ops_buf *out, uint32_t *status,
                          uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = 0;
  if (N == 0) return CRDT_OK;
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!actors || A == 0) return fail(ctx, CRDT_EINVAL, "mvreg_ops_ingest: need the actor dictionary");
  if (!out && !totals) return fail(ctx, CRDT_EINVAL, "mvreg_ops_ingest: neither an output nor totals asked for");
  MvOpsPlan p{};
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.actors = actors;
  p.A = A;
  p.status = status;
  u64 cap = 0;
  if (out) {
    if (!out->op_off || (out->op_cap && (!out->clk_row || !out->val)) || (out->row_cap && !out->clk_pool))
      return fail(ctx, CRDT_EINVAL, "mvreg_ops_ingest: NULL output array");
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "mvreg_ops_ingest: row_cap past 2^32 - 1");
    p.row = out->clk_row;
    p.pool = (u64 *)out->clk_pool;
    p.val = (u64 *)out->val;
    cap = std::min<u64>(out->op_cap, out->row_cap);
  }
  // ops and rows are one number: the smaller capacity binds, and both totals are that count
  const size_t ring_bytes = (size_t)kMvWpb * kWalkRing * kWalkWin * 4;
  const unsigned grid = wave_grid(ctx, N, kMvWpb, 8);
  u64 *op_off = out ? (u64 *)out->op_off : nullptr;
  const SizedOut<1> o{{cap}, {op_off}, {nullptr, nullptr}, status};
  uint64_t n_ops = 0;
  const int rc = sized_ingest<1>(
      ctx, "wire_mvreg_ops_ingest", N, o, out != nullptr, totals ? &n_ops : nullptr,
      [&](u64 *counts) {
        p.counts = counts;
        hipLaunchKernelGGL(mvops_count_kernel, dim3(grid), dim3(kBlock), ring_bytes, ctx->stream, p);
      },
      [&] {
        p.op_off = op_off;
        const unsigned long long dw = (p.A + 1) / 2;
        p.dict_words = dw * 8 + ring_bytes <= kMvLdsMax ? dw : 0;  // else: searched in global memory
        hipLaunchKernelGGL(mvops_fill_kernel, dim3(grid), dim3(kBlock), ring_bytes + p.dict_words * 8, ctx->stream, p);
      });
  if (!rc && totals) totals[0] = totals[1] = n_ops;
  return rc;
}

int crdt_mvreg_ops_egress(crdt_ctx *ctx, const crdt_mvreg_ops *ops, size_t N, const uint32_t *actors, size_t A,
                          uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off || !actors || A == 0)
    return fail(ctx, CRDT_EINVAL, "mvreg_ops_egress: need ops (op_off) and the actor dictionary");
  if (ops->n_ops && (!ops->clk_row || !ops->val || (ops->n_clk_rows && !ops->clk_pool)))
    return fail(ctx, CRDT_EINVAL, "mvreg_ops_egress: NULL op arrays");
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "mvreg_ops_egress: need frame_off, total and status");
  MvOpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_clk_rows;
  p.op_off = (const u64 *)ops->op_off;
  p.row = ops->clk_row;
  p.pool = (const u64 *)ops->clk_pool;
  p.val = (const u64 *)ops->val;
  p.actors = actors;
  p.status = status;
  return two_pass_egress(ctx, "wire_mvreg_ops_egress", mvops_egress_kernel, p, wave_grid(ctx, N, kMvWpb, 32), frame_off, bytes,
                         cap, total);
}

}  // extern "C"
