// Serde wire format of op streams <-> the dense op batches of crdt_orswot_apply_batch /
// crdt_map_apply_batch, on the device.
//
// The reference's ops derive Serialize / Deserialize like its states (orswot.rs:31-47, map.rs:50-68,
// mvreg.rs:38-47, vclock.rs:32-38).  The bincode 1.x rules of wire.hip apply, plus: an enum is a u32
// variant index followed by the variant's fields.  For the two instantiations the grouped apply
// kernels take:
//   Dot<u32>                 = u32 actor, u64 counter
//   orswot::Op<u64, u32>     = u32 0 (Add), Dot, u64 k, k x u64 member            (HashSet: any order)
//                            | u32 1 (Rm),  VClock, u64 k, k x u64 member
//   map::Op<u32, MVReg, u32> = u32 0 (Rm),  VClock, u64 k, k x u32 key            (BTreeSet: ascending)
//                            | u32 1 (Up),  Dot, u32 key, u32 0 (mvreg::Op::Put), VClock clock, u64 val
//   frame of state s         = Vec<Op>: u64 n_ops, then the ops back to back
// The dense `kind` arrays keep their meaning (Orswot 0 = Add, Map 0 = Up): the Map tag is flipped on
// the way in and out.
//
// Ingest is count -> three exclusive scans -> finalize (capacities) -> fill (the sized ingest of
// wire_driver.hpp), one wave per frame in both passes.  A frame is one dependent chain (an op's length decides where the next begins): the
// walk reads only tags and counts, through the LDS-ring reader of wire_common.hpp; every 64 ops
// found the parse runs with lane = op (dot / clock records, dictionary lookups, stores straight
// into the op's SoA slots and its zeroed clock row).  The count pass settles malformed frames and,
// through finalize, capacities, so the fill pass writes only whole, valid states.
// Egress is count (lane = op) -> wave prefix sum -> scan over states -> write (wire_driver.hpp's two passes).
#include "wire_ops_common.hpp"

namespace crdt {

constexpr int kOpsWpb = kBlock / kWave;
constexpr int kLaneIds = 4;  // an op's id list up to this long is parsed by its own lane; longer ones by the wave
constexpr int kLaneRecs = kWave;  // likewise for the records of an op's clock (A <= 64: always the lane)
constexpr size_t kOpsLdsMax = 64 << 10;

struct OpsPlan {
  const uint8_t *bytes;
  const u64 *frame_off;
  unsigned long long N;
  const uint32_t *actors;
  unsigned long long A;
  const u64 *members;    // Orswot: the u64 member dictionary
  const uint32_t *keys;  // Map: the u32 key dictionary
  unsigned long long U;  // its entries (M or K)
  unsigned long long dict_words;  // > 0: the dictionaries are staged in LDS (this many u64 words)
  u64 *counts;           // [3][N] ops, rows, ids of every frame (count pass)
  const u64 *op_off, *row_off, *id_off;  // [N+1], final (after the capacities)
  uint32_t *status;
  uint8_t *kind;
  uint32_t *actor;
  u64 *counter;
  uint32_t *row;   // rm_row / clk_row
  u64 *pool;       // rm_clock / clk_pool, [rows][A]
  u64 *ids_off;    // mem_off / key_off, [ops + 1]
  uint32_t *ids;   // mem / keys
  uint32_t *key;   // Map
  u64 *val;        // Map
};

// The walk over one frame (nw >= 2 words): emit(pos, tag, n, cnt) for every op, in order, with pos
// the op's first word, n its clock's records and cnt its set's ids.  Every count is tested against
// the words left before anything depends on it.  False: malformed (truncated, trailing words, a
// count that cannot fit, an unknown tag, a Map Up whose MVReg tag is not Put).
template <bool MAP, class F>
__device__ __forceinline__ bool walk_ops(OpWalk &w, int lane, F &&emit) {
  const unsigned long long nw = w.nw;
  const u64 n_ops = w.at64(0, lane);
  if (n_ops > (nw - 2) / 5) return false;  // the smallest op takes 20 bytes
  unsigned long long k = 2;
  for (u64 i = 0; i < n_ops; ++i) {
    if (k + 1 > nw) return false;
    const uint32_t tag = w.at(k, lane);
    if (tag > 1) return false;
    unsigned long long n = 0, cnt = 0, next;
    if (MAP ? tag == 1 : tag == 0) {
      if (!MAP) {  // Add: dot, u64 cnt, members
        if (k + 6 > nw) return false;
        cnt = w.at64(k + 4, lane);
        if (cnt > (nw - k - 6) / 2) return false;
        next = k + 6 + 2 * cnt;
      } else {  // Up: dot, key, MVReg tag, clock, val
        if (k + 8 > nw) return false;
        if (w.at(k + 5, lane) != 0) return false;
        n = w.at64(k + 6, lane);
        if (n > (nw - k - 8) / 3) return false;
        next = k + 8 + 3 * n + 2;
        if (next > nw) return false;
      }
    } else {  // Rm: clock, set
      if (k + 3 > nw) return false;
      n = w.at64(k + 1, lane);
      if (n > (nw - k - 3) / 3) return false;
      const unsigned long long p = uni64(k + 3 + 3 * n);
      if (p + 2 > nw) return false;
      cnt = w.at64(p, lane);
      if (MAP) {
        if (cnt > nw - p - 2) return false;
        next = p + 2 + cnt;
      } else {
        if (cnt > (nw - p - 2) / 2) return false;
        next = p + 2 + 2 * cnt;
      }
    }
    emit(k, tag, uni64(n), uni64(cnt));
    k = uni64(next);
  }
  return k == nw;
}

__device__ __forceinline__ bool ops_frame(const OpsPlan &p, unsigned long long s, OpWalk &w, uint32_t *ring) {
  const u64 b = p.frame_off[s], e = p.frame_off[s + 1];
  if ((b & 3) || (e & 3) || e < b || e - b < 8) return false;
  w.fw = reinterpret_cast<const uint32_t *>(p.bytes + b);
  w.nw = (e - b) / 4;
  w.nwin = (w.nw + kWalkWin - 1) / kWalkWin;
  w.ring = ring;
  return true;
}

template <bool MAP>
__global__ __launch_bounds__(kBlock) void ops_count_kernel(OpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  uint32_t *ring = reinterpret_cast<uint32_t *>(lds) + (size_t)wib * kWalkRing * kWalkWin;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kOpsWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kOpsWpb) {
    unsigned st = 0;
    u64 no = 0, nr = 0, ni = 0;
    OpWalk w;
    if (!ops_frame(p, s, w, ring)) {
      st = kWireBad;
    } else {
      w.start(lane);
      const bool ok = walk_ops<MAP>(w, lane, [&](unsigned long long, uint32_t tag, unsigned long long, unsigned long long cnt) {
        ++no;
        nr += MAP ? 1 : tag;
        ni += cnt;
      });
      wire_vmcnt<0>();  // no DMA of this frame may land in the ring after the next one starts
      if (!ok) {
        st = kWireBad;
        no = nr = ni = 0;
      }
    }
    if (lane == 0) {
      p.status[s] = st;
      p.counts[s] = no;
      p.counts[p.N + s] = nr;
      p.counts[2 * p.N + s] = ni;
    }
  }
}

// One op's id list: u64 member ids (Orswot) or u32 key ids (Map) at word `pos` -> dictionary indices.
template <bool MAP>
__device__ __forceinline__ bool ops_id(const OpsPlan &p, const uint32_t *fw, const u64 *members, const uint32_t *keys,
                                       unsigned long long pos, unsigned long long i, uint32_t *dst) {
  long long ix;
  if (MAP) ix = find_u32(keys, p.U, fw[pos + i], ~0ull);
  else ix = find_u64(members, p.U, rd64(fw, pos + 2 * i), ~0ull);
  dst[i] = ix < 0 ? 0xFFFFFFFFu : (uint32_t)ix;
  return ix < 0;
}

template <bool MAP>
__global__ __launch_bounds__(kBlock) void ops_fill_kernel(OpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  const uint32_t *actors = p.actors, *keys = p.keys;
  const u64 *members = p.members;
  u64 *base = lds;
  if (p.dict_words) {  // [actors u32, padded to 8 bytes | members u64 or keys u32]
    uint32_t *la = reinterpret_cast<uint32_t *>(lds);
    for (unsigned long long i = threadIdx.x; i < p.A; i += blockDim.x) la[i] = p.actors[i];
    u64 *lu = lds + (p.A + 1) / 2;
    if (MAP) {
      uint32_t *lk = reinterpret_cast<uint32_t *>(lu);
      for (unsigned long long i = threadIdx.x; i < p.U; i += blockDim.x) lk[i] = p.keys[i];
      keys = lk;
    } else {
      for (unsigned long long i = threadIdx.x; i < p.U; i += blockDim.x) lu[i] = p.members[i];
      members = lu;
    }
    __syncthreads();
    actors = la;
    base = lds + p.dict_words;
  }
  uint32_t *ring = reinterpret_cast<uint32_t *>(base) + (size_t)wib * kWalkRing * kWalkWin;
  const unsigned long long A = p.A;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kOpsWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kOpsWpb) {
    const unsigned st = p.status[s];
    const u64 o0 = p.op_off[s], r0 = p.row_off[s], i0 = p.id_off[s];
    OpWalk w;
    if ((st & (kWireBad | kWireCap)) || p.op_off[s + 1] == o0 || !ops_frame(p, s, w, ring)) continue;
    w.start(lane);
    const uint32_t *fw = w.fw;
    // the batch of ops the lanes parse next: lane i holds op i of it
    int cnt = 0;
    u64 done = 0, rows_run = 0, ids_run = 0, batch_row = 0;
    unsigned long long d_pos = 0, d_n = 0, d_cnt = 0, d_row = 0, d_id = 0;
    uint32_t d_tag = 0;
    bool miss = false;
    auto flush = [&]() {
      // the batch's clock rows are contiguous: zeroed here, coalesced, and landed before the records
      u64 *rows = p.pool + (r0 + batch_row) * A;
      const unsigned long long nz = (rows_run - batch_row) * A;
      for (unsigned long long x = lane; x < nz; x += kWave) rows[x] = 0;
      wire_vmcnt<0>();
      const bool on = lane < cnt;
      unsigned long long ids_pos = 0, rec = 0;
      if (on) {
        const u64 o = o0 + done + lane;
        const bool dot = MAP ? d_tag == 1 : d_tag == 0;
        if (dot) {
          const long long col = find_u32(actors, A, fw[d_pos + 1], ~0ull);
          if (col < 0) miss = true;
          p.actor[o] = col < 0 ? 0xFFFFFFFFu : (uint32_t)col;
          p.counter[o] = rd64(fw, d_pos + 2);
        } else {
          p.actor[o] = 0;
          p.counter[o] = 0;
          rec = d_pos + 3;
          ids_pos = d_pos + 3 + 3 * d_n + 2;
        }
        if (!MAP) {
          p.kind[o] = (uint8_t)d_tag;
          p.row[o] = dot ? 0u : (uint32_t)(r0 + d_row);
          if (dot) ids_pos = d_pos + 6;
        } else {
          p.kind[o] = (uint8_t)(d_tag ^ 1u);
          p.row[o] = (uint32_t)(r0 + d_row);
          if (dot) {
            const long long kx = find_u32(keys, p.U, fw[d_pos + 4], ~0ull);
            if (kx < 0) miss = true;
            p.key[o] = kx < 0 ? 0xFFFFFFFFu : (uint32_t)kx;
            rec = d_pos + 8;
            p.val[o] = rd64(fw, d_pos + 8 + 3 * d_n);
          } else {
            p.key[o] = 0;
            p.val[o] = 0;
          }
        }
        p.ids_off[o + 1] = i0 + d_id + d_cnt;
        u64 *dst = p.pool + (r0 + d_row) * A;
        for (unsigned long long r = 0; r < (d_n <= (unsigned long long)kLaneRecs ? d_n : 0); ++r) {
          const uint32_t id = fw[rec + 3 * r];
          const u64 c = rd64(fw, rec + 3 * r + 1);
          const long long col = find_u32(actors, A, id, r);
          if (col < 0) miss = true;
          else dst[col] = c;
        }
        if (d_cnt <= (unsigned long long)kLaneIds)
          for (unsigned long long i = 0; i < d_cnt; ++i)
            miss |= ops_id<MAP>(p, fw, members, keys, ids_pos, i, p.ids + i0 + d_id);
      }
      // a clock with more records than a lane takes: the wave loops over them
      u64 wclk = __ballot(on && d_n > (unsigned long long)kLaneRecs);
      while (wclk) {
        const int j = __ffsll((unsigned long long)wclk) - 1;
        wclk &= wclk - 1;
        const unsigned long long jr = __shfl(rec, j, kWave), jn = __shfl(d_n, j, kWave);
        u64 *dst = p.pool + (r0 + __shfl(d_row, j, kWave)) * A;
        for (unsigned long long r = lane; r < jn; r += kWave) {
          const long long col = find_u32(actors, A, fw[jr + 3 * r], r);
          if (col < 0) miss = true;
          else dst[col] = rd64(fw, jr + 3 * r + 1);
        }
      }
      // an op with more ids than that: the wave loops over them
      u64 wide = __ballot(on && d_cnt > (unsigned long long)kLaneIds);
      while (wide) {
        const int j = __ffsll((unsigned long long)wide) - 1;
        wide &= wide - 1;
        const unsigned long long jp = __shfl(ids_pos, j, kWave), jc = __shfl(d_cnt, j, kWave);
        uint32_t *dst = p.ids + i0 + __shfl(d_id, j, kWave);
        for (unsigned long long i = lane; i < jc; i += kWave) miss |= ops_id<MAP>(p, fw, members, keys, jp, i, dst);
      }
      done += cnt;
      cnt = 0;
      batch_row = rows_run;
    };
    walk_ops<MAP>(w, lane, [&](unsigned long long pos, uint32_t tag, unsigned long long n, unsigned long long c) {
      if (lane == cnt) {
        d_pos = pos;
        d_tag = tag;
        d_n = n;
        d_cnt = c;
        d_row = rows_run;
        d_id = ids_run;
      }
      rows_run += MAP ? 1 : tag;
      ids_run += c;
      if (++cnt == kWave) flush();
    });
    if (cnt) flush();
    wire_vmcnt<0>();
    if (__ballot(miss) && lane == 0) p.status[s] = st | kWireMissing;
  }
}

// ---- egress ---------------------------------------------------------------------------------------
struct OpsEgressPlan {
  unsigned long long N, A, U, n_ops, n_rows, n_ids;
  const u64 *op_off;
  const uint8_t *kind;
  const uint32_t *actor;
  const u64 *counter;
  const uint32_t *row;
  const u64 *pool;
  const u64 *ids_off;
  const uint32_t *ids;
  const uint32_t *key;
  const u64 *val;
  const uint32_t *actors;
  const u64 *members;
  const uint32_t *keys;
  u64 *sizes;
  const u64 *frame_off;
  uint8_t *bytes;
  uint32_t *status;
};

// One wave per state, lane = op in batches of 64.  write = 0: validate every op, size the frame
// (status[s], sizes[s]); write = 1: write it at frame_off[s] (the empty Vec for a state with bit 1).
template <bool MAP>
__global__ __launch_bounds__(kBlock) void ops_egress_kernel(OpsEgressPlan p, int write) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwv = (unsigned long long)gridDim.x * kOpsWpb;
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
      bool lbad = false, has_row = false;
      uint32_t k = 0;
      unsigned long long r = 0, ib = 0, ie = 0;
      if (on) {
        k = p.kind[o];
        const bool dot = k == 0;
        if (k > 1) lbad = true;
        else if (dot) {
          if (!p.actor || !p.counter || p.actor[o] >= A) lbad = true;
          if (MAP && (!p.key || !p.val || p.key[o] >= p.U)) lbad = true;
        }
        if (!lbad && (MAP || !dot)) {
          has_row = true;
          if (!p.row || !p.pool) lbad = true;
          else {
            r = p.row[o];
            if (r >= p.n_rows) lbad = true;
          }
        }
        if (!lbad && !(MAP && dot)) {
          if (!p.ids_off) lbad = true;
          else {
            ib = p.ids_off[o];
            ie = p.ids_off[o + 1];
            if (ie < ib || ie > p.n_ids || (ie > ib && !p.ids)) lbad = true;
          }
        }
        if (lbad) {
          has_row = false;
          ib = ie = 0;
        }
      }
      const unsigned long long ic = ie - ib;
      if (!write) {  // every id names a dictionary entry
        if (on && ic <= (unsigned long long)kLaneIds)
          for (unsigned long long i = ib; i < ie; ++i) lbad |= p.ids[i] >= p.U;
        u64 wide = __ballot(on && ic > (unsigned long long)kLaneIds);
        while (wide) {
          const int j = __ffsll((unsigned long long)wide) - 1;
          wide &= wide - 1;
          const unsigned long long jb = __shfl(ib, j, kWave), je = __shfl(ie, j, kWave);
          bool x = false;
          for (unsigned long long i = jb + lane; i < je; i += kWave) x |= p.ids[i] >= p.U;
          if (__ballot(x) && lane == j) lbad = true;
        }
      }
      // non-zeros of every op's clock row: the wave reads one row at a time, coalesced
      unsigned long long nnz = 0;
      u64 rows = __ballot(has_row);
      while (rows) {
        const int j = __ffsll((unsigned long long)rows) - 1;
        rows &= rows - 1;
        const unsigned long long jr = __shfl(r, j, kWave);
        const u64 c = nnz_row(p.pool + jr * A, A, lane);
        if (lane == j) nnz = c;
      }
      unsigned long long words = 0;
      if (on) {
        if (MAP) words = k == 0 ? 10 + 3 * nnz : 5 + 3 * nnz + ic;
        else words = k == 0 ? 6 + 2 * ic : 5 + 3 * nnz + 2 * ic;
      }
      if (__ballot(lbad)) bad = true;
      u64 total;
      const u64 kp = run + wave_excl(words, lane, total);
      run += total;
      if (!write || bad) continue;
      // headers, by the op's lane
      unsigned long long ids_at = 0, clk_at = 0;
      if (on) {
        if (!MAP) {
          out[kp] = k;
          if (k == 0) {
            out[kp + 1] = p.actors[p.actor[o]];
            wr64(out, kp + 2, p.counter[o]);
            wr64(out, kp + 4, ic);
            ids_at = kp + 6;
          } else {
            clk_at = kp + 1;
            wr64(out, kp + 3 + 3 * nnz, ic);
            ids_at = kp + 5 + 3 * nnz;
          }
        } else {
          out[kp] = k ^ 1u;
          if (k == 0) {
            out[kp + 1] = p.actors[p.actor[o]];
            wr64(out, kp + 2, p.counter[o]);
            out[kp + 4] = p.keys[p.key[o]];
            out[kp + 5] = 0;
            clk_at = kp + 6;
            wr64(out, kp + 8 + 3 * nnz, p.val[o]);
          } else {
            clk_at = kp + 1;
            wr64(out, kp + 3 + 3 * nnz, ic);
            ids_at = kp + 5 + 3 * nnz;
          }
        }
        if (ic <= (unsigned long long)kLaneIds)
          for (unsigned long long i = 0; i < ic; ++i) {
            if (MAP) out[ids_at + i] = p.keys[p.ids[ib + i]];
            else wr64(out, ids_at + 2 * i, p.members[p.ids[ib + i]]);
          }
      }
      // clocks and long id lists, by the wave
      rows = __ballot(has_row);
      while (rows) {
        const int j = __ffsll((unsigned long long)rows) - 1;
        rows &= rows - 1;
        const unsigned long long jr = __shfl(r, j, kWave), jk = __shfl(clk_at, j, kWave);
        write_vclock(out, jk, p.pool + jr * A, A, p.actors, lane);
      }
      u64 wide = __ballot(on && ic > (unsigned long long)kLaneIds);
      while (wide) {
        const int j = __ffsll((unsigned long long)wide) - 1;
        wide &= wide - 1;
        const unsigned long long jb = __shfl(ib, j, kWave), jc = __shfl(ic, j, kWave), ja = __shfl(ids_at, j, kWave);
        for (unsigned long long i = lane; i < jc; i += kWave) {
          if (MAP) out[ja + i] = p.keys[p.ids[jb + i]];
          else wr64(out, ja + 2 * i, p.members[p.ids[jb + i]]);
        }
      }
    }
    if (!write && lane == 0) {
      p.status[s] = bad ? kWireMissing : 0u;
      p.sizes[s] = bad ? 8 : run * 4;
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------
template <bool MAP>
static int ops_ingest(crdt_ctx *ctx, OpsPlan p, u64 cap_op, u64 cap_row, u64 cap_id, bool fill, u64 *op_off,
                      u64 *row_off, u64 *id_off, uint64_t *totals, const char *what) {
  const size_t ring_bytes = (size_t)kOpsWpb * kWalkRing * kWalkWin * 4;
  const unsigned grid = wave_grid(ctx, p.N, kOpsWpb, 8);
  const SizedOut<3> o{{cap_op, cap_row, cap_id}, {op_off, row_off, id_off}, {p.ids_off, nullptr}, p.status};
  return sized_ingest<3>(
      ctx, what, p.N, o, fill, totals,
      [&](u64 *counts) {
        p.counts = counts;
        hipLaunchKernelGGL(ops_count_kernel<MAP>, dim3(grid), dim3(kBlock), ring_bytes, ctx->stream, p);
      },
      [&] {
        p.op_off = op_off;
        p.row_off = row_off;
        p.id_off = id_off;
        const unsigned long long dw = (p.A + 1) / 2 + (MAP ? (p.U + 1) / 2 : p.U);
        p.dict_words = dw * 8 + ring_bytes <= kOpsLdsMax ? dw : 0;  // else: searched in global memory
        hipLaunchKernelGGL(ops_fill_kernel<MAP>, dim3(grid), dim3(kBlock), ring_bytes + p.dict_words * 8, ctx->stream, p);
      });
}

template <bool MAP>
static int ops_egress(crdt_ctx *ctx, OpsEgressPlan p, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total,
                      const char *what) {
  return two_pass_egress(ctx, what, ops_egress_kernel<MAP>, p, wave_grid(ctx, p.N, kOpsWpb, 32), frame_off, bytes, cap, total);
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_orswot_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                           const uint32_t *actors, size_t A, const uint64_t *members, size_t M,
                           const crdt_orswot_ops_buf *out, uint64_t *row_off, uint64_t *id_off, uint32_t *status,
                           uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = totals[2] = 0;
  if (N == 0) return CRDT_OK;
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!actors || !members || A == 0 || M == 0)
    return fail(ctx, CRDT_EINVAL, "orswot_ops_ingest: need the actor and member dictionaries");
  if (!out && !totals) return fail(ctx, CRDT_EINVAL, "orswot_ops_ingest: neither an output nor totals asked for");
  OpsPlan p{};
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.actors = actors;
  p.A = A;
  p.members = (const u64 *)members;
  p.U = M;
  p.status = status;
  if (out) {
    if (!out->op_off || !row_off || !id_off || !out->mem_off ||
        (out->op_cap && (!out->kind || !out->actor || !out->counter || !out->rm_row)) ||
        (out->row_cap && !out->rm_clock) || (out->id_cap && !out->mem))
      return fail(ctx, CRDT_EINVAL, "orswot_ops_ingest: NULL output array");
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "orswot_ops_ingest: row_cap past 2^32 - 1");
    p.kind = out->kind;
    p.actor = out->actor;
    p.counter = (u64 *)out->counter;
    p.row = out->rm_row;
    p.pool = (u64 *)out->rm_clock;
    p.ids_off = (u64 *)out->mem_off;
    p.ids = out->mem;
  }
  return ops_ingest<false>(ctx, p, out ? out->op_cap : 0, out ? out->row_cap : 0, out ? out->id_cap : 0, out != nullptr,
                           out ? (u64 *)out->op_off : nullptr, (u64 *)row_off, (u64 *)id_off, totals,
                           "wire_ops_ingest");
}

int crdt_map_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                        const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const crdt_map_ops_buf *out,
                        uint64_t *row_off, uint64_t *id_off, uint32_t *status, uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = totals[2] = 0;
  if (N == 0) return CRDT_OK;
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!actors || !keys || A == 0 || K == 0)
    return fail(ctx, CRDT_EINVAL, "map_ops_ingest: need the actor and key dictionaries");
  if (!out && !totals) return fail(ctx, CRDT_EINVAL, "map_ops_ingest: neither an output nor totals asked for");
  OpsPlan p{};
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.actors = actors;
  p.A = A;
  p.keys = keys;
  p.U = K;
  p.status = status;
  if (out) {
    if (!out->op_off || !row_off || !id_off || !out->key_off ||
        (out->op_cap && (!out->kind || !out->actor || !out->counter || !out->key || !out->val || !out->clk_row)) ||
        (out->row_cap && !out->clk_pool) || (out->id_cap && !out->keys))
      return fail(ctx, CRDT_EINVAL, "map_ops_ingest: NULL output array");
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "map_ops_ingest: row_cap past 2^32 - 1");
    p.kind = out->kind;
    p.actor = out->actor;
    p.counter = (u64 *)out->counter;
    p.key = out->key;
    p.val = (u64 *)out->val;
    p.row = out->clk_row;
    p.pool = (u64 *)out->clk_pool;
    p.ids_off = (u64 *)out->key_off;
    p.ids = out->keys;
  }
  return ops_ingest<true>(ctx, p, out ? out->op_cap : 0, out ? out->row_cap : 0, out ? out->id_cap : 0, out != nullptr,
                          out ? (u64 *)out->op_off : nullptr, (u64 *)row_off, (u64 *)id_off, totals, "wire_ops_ingest");
}

int crdt_orswot_ops_egress(crdt_ctx *ctx, const crdt_orswot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                           const uint64_t *members, size_t M, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                           size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off || !actors || !members || A == 0 || M == 0)
    return fail(ctx, CRDT_EINVAL, "orswot_ops_egress: need ops (op_off) and the dictionaries");
  if (ops->n_ops && (!ops->kind || !ops->mem_off)) return fail(ctx, CRDT_EINVAL, "orswot_ops_egress: NULL kind / mem_off");
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "orswot_ops_egress: need frame_off, total and status");
  OpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.U = M;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_rm_rows;
  p.n_ids = ops->n_mem;
  p.op_off = (const u64 *)ops->op_off;
  p.kind = ops->kind;
  p.actor = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.row = ops->rm_row;
  p.pool = (const u64 *)ops->rm_clock;
  p.ids_off = (const u64 *)ops->mem_off;
  p.ids = ops->mem;
  p.actors = actors;
  p.members = (const u64 *)members;
  p.status = status;
  return ops_egress<false>(ctx, p, frame_off, bytes, cap, total, "wire_ops_egress");
}

int crdt_map_ops_egress(crdt_ctx *ctx, const crdt_map_ops *ops, size_t N, const uint32_t *actors, size_t A,
                        const uint32_t *keys, size_t K, uint64_t *frame_off, uint8_t *bytes, size_t cap, size_t *total,
                        uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off || !actors || !keys || A == 0 || K == 0)
    return fail(ctx, CRDT_EINVAL, "map_ops_egress: need ops (op_off) and the dictionaries");
  if (ops->n_ops && !ops->kind) return fail(ctx, CRDT_EINVAL, "map_ops_egress: NULL kind");
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "map_ops_egress: need frame_off, total and status");
  OpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.U = K;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_clk_rows;
  p.n_ids = ops->n_keys;
  p.op_off = (const u64 *)ops->op_off;
  p.kind = ops->kind;
  p.actor = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.key = ops->key;
  p.val = (const u64 *)ops->val;
  p.row = ops->clk_row;
  p.pool = (const u64 *)ops->clk_pool;
  p.ids_off = (const u64 *)ops->key_off;
  p.ids = ops->keys;
  p.actors = actors;
  p.keys = keys;
  p.status = status;
  return ops_egress<true>(ctx, p, frame_off, bytes, cap, total, "wire_ops_egress");
}

}  // extern "C"
