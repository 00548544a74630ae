// Serde wire format of the value-typed Maps' op streams <-> the dense op batches of
// crdt_map_counter_apply_batch / crdt_map_orswot_apply_batch / crdt_map_nested_apply_batch, on the device.
//
// map::Op<u32, V, u32> for V = GCounter, PNCounter, Orswot<u64, u32> and Map<u32, MVReg<u64, u32>, u32>
// (map.rs:50-68 with gcounter.rs:37, pncounter.rs:35-51, orswot.rs:31-47, mvreg.rs:38-47 inside; the
// rules of wire_ops.hip), in 32-bit words:
//   Op::Rm (every V)     = 0, VClock, u64 k, k x u32 key                              5 + 3n + k
//   Op::Up, GCounter     = 1, Dot, u32 key, Dot                                       8
//   Op::Up, PNCounter    = 1, Dot, u32 key, Dot, u32 dir (0 Pos, 1 Neg)               9
//   Op::Up, Orswot       = 1, Dot, u32 key, 0 (Add), Dot, u64 k, k x u64 member       11 + 2k
//                        | 1, Dot, u32 key, 1 (Rm), VClock, u64 k, k x u64 member     10 + 3n + 2k
//   Op::Up, Map<MVReg>   = 1, Dot, u32 key, 0 (inner Rm), VClock, u64 k, k x u32 ikey 10 + 3n + k
//                        | 1, Dot, u32 key, 1 (inner Up), Dot, u32 ikey, 0 (Put), VClock, u64 val  15 + 3n
//   frame of state s     = u64 n_ops, then the ops back to back
// Dense kind: 0 = Up, 1 = Rm and ikind: 0 = inner Up, 1 = inner Rm (both flipped against the wire);
// vkind (0 = Add, 1 = Rm) and vdir as on the wire.
//
// The structure is wire_ops.hip's: count -> four exclusive scans (ops, clock rows, keyset keys,
// members) -> finalize (capacities: the cut is the minimum over the four) -> fill, one wave per
// frame, the walk over tags and counts through the LDS ring, every 64 ops a parse with lane = op.
// The kernels are templated on the value type, so an op costs no branch on it; the counter Maps'
// Ups have a fixed length and the walk reads their tag (and a PNCounter's dir) only.
#include <cstddef>

#include "wire_ops_common.hpp"

namespace crdt {

enum : int { kVG = 0, kVPN = 1, kVOrswot = 2, kVNested = 3 };

constexpr int kVoWpb = kBlock / kWave;
constexpr int kVoLaneIds = 4;       // an op's id list up to this long is parsed by its own lane; longer ones by the wave
constexpr int kVoLaneRecs = kWave;  // likewise for the records of an op's clock
constexpr size_t kVoLdsMax = 64 << 10;

// the const op structs and their mutable twins: one layout
#define VO_SAME(CS, BUF, cf, bf) static_assert(offsetof(CS, cf) == offsetof(BUF, bf), #CS "." #cf " / " #BUF "." #bf)
static_assert(sizeof(crdt_map_counter_ops) == sizeof(crdt_map_counter_ops_buf), "crdt_map_counter_ops_buf");
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, n_ops, op_cap);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, op_off, op_off);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, kind, kind);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, actor, actor);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, counter, counter);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, key, key);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, vactor, vactor);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, vcounter, vcounter);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, vdir, vdir);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, clk_row, clk_row);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, clk_pool, clk_pool);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, n_clk_rows, row_cap);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, key_off, key_off);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, keys, keys);
VO_SAME(crdt_map_counter_ops, crdt_map_counter_ops_buf, n_keys, key_cap);
static_assert(sizeof(crdt_map_orswot_ops) == sizeof(crdt_map_orswot_ops_buf), "crdt_map_orswot_ops_buf");
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, n_ops, op_cap);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, op_off, op_off);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, kind, kind);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, actor, actor);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, counter, counter);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, key, key);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, vkind, vkind);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, vactor, vactor);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, vcounter, vcounter);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, clk_row, clk_row);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, clk_pool, clk_pool);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, n_clk_rows, row_cap);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, key_off, key_off);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, keys, keys);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, n_keys, key_cap);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, mem_off, mem_off);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, mems, mems);
VO_SAME(crdt_map_orswot_ops, crdt_map_orswot_ops_buf, n_mems, mem_cap);
static_assert(sizeof(crdt_map_nested_ops) == sizeof(crdt_map_nested_ops_buf), "crdt_map_nested_ops_buf");
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, n_ops, op_cap);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, op_off, op_off);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, kind, kind);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, actor, actor);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, counter, counter);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, key, key);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, ikind, ikind);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, iactor, iactor);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, icounter, icounter);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, ikey, ikey);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, val, val);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, ikeys, ikeys);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, clk_row, clk_row);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, clk_pool, clk_pool);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, n_clk_rows, row_cap);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, key_off, key_off);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, keys, keys);
VO_SAME(crdt_map_nested_ops, crdt_map_nested_ops_buf, n_keys, key_cap);
#undef VO_SAME

struct VOpsPlan {
  const uint8_t *bytes;
  const u64 *frame_off;
  unsigned long long N;
  const uint32_t *actors;
  unsigned long long A;
  const uint32_t *keys;  // the Map's u32 key dictionary
  unsigned long long K;
  const u64 *members;     // Orswot: the u64 member dictionary
  const uint32_t *idict;  // nested: the u32 inner-key dictionary
  unsigned long long U;   // its entries (M or K2; 0 for the counters)
  unsigned long long K2w; // nested: mask words per op
  unsigned long long dict_words;  // > 0: the dictionaries are staged in LDS (this many u64 words)
  u64 *counts;            // [4][N] ops, rows, keys, members of every frame (count pass)
  const u64 *op_off, *row_off, *key_first, *mem_first;  // [N+1], final (after the capacities)
  uint32_t *status;
  uint8_t *kind;
  uint32_t *actor;
  u64 *counter;
  uint32_t *key;
  uint8_t *sub;       // vdir / vkind / ikind
  uint32_t *vactor;   // the value op's dot (nested: iactor)
  u64 *vcounter;
  uint32_t *ikey;     // nested
  u64 *val;           // nested
  u64 *imask;         // nested: ikeys [ops][K2w]
  uint32_t *row;      // clk_row
  u64 *pool;          // clk_pool, [rows][A]
  u64 *key_off;       // [ops + 1]
  uint32_t *keys_out;
  u64 *mem_off;       // Orswot, [ops + 1]
  uint32_t *mems;
};

// which ops carry a clock row (tag / sub as on the wire)
template <int V>
__device__ __forceinline__ bool vo_has_row(uint32_t tag, uint32_t sub) {
  if (V == kVNested) return true;
  if (V == kVOrswot) return tag == 0 || sub == 1;
  return tag == 0;
}

// The walk over one frame (nw >= 2 words): emit(pos, tag, sub, n, cnt) for every op, in order, with
// pos the op's first word, tag / sub its outer / value variant as on the wire, n its clock's records
// and cnt its set's ids.  Every count is tested against the words left before anything depends on
// it, in the divide form (a product of a count can wrap).  False: malformed (truncated, trailing
// words, a count that cannot fit, an unknown outer / value / MVReg tag, a dir past 1).
template <int V, class F>
__device__ __forceinline__ bool walk_vops(OpWalk &w, int lane, F &&emit) {
  const unsigned long long nw = w.nw;
  const u64 n_ops = w.at64(0, lane);
  if (n_ops > (nw - 2) / 5) return false;  // the smallest op (an Rm) takes 20 bytes: the loop is bounded by the frame
  unsigned long long k = 2;
  for (u64 i = 0; i < n_ops; ++i) {
    if (k + 1 > nw) return false;
    const uint32_t tag = w.at(k, lane);
    if (tag > 1) return false;
    uint32_t sub = 0;
    unsigned long long n = 0, cnt = 0, next;
    if (tag == 0) {  // Rm: clock, keyset
      if (k + 3 > nw) return false;
      n = w.at64(k + 1, lane);
      if (n > (nw - k - 3) / 3) return false;
      const unsigned long long p = uni64(k + 3 + 3 * n);
      if (p + 2 > nw) return false;
      cnt = w.at64(p, lane);
      if (cnt > nw - p - 2) return false;
      next = p + 2 + cnt;
    } else if (V == kVG || V == kVPN) {  // Up: dot, key, dot (, dir)
      constexpr unsigned long long len = V == kVG ? 8 : 9;
      if (k + len > nw) return false;
      if (V == kVPN) {
        sub = w.at(k + 8, lane);
        if (sub > 1) return false;
      }
      next = k + len;
    } else {  // Up: dot, key, value tag, ...
      if (k + 6 > nw) return false;
      sub = w.at(k + 5, lane);
      if (sub > 1) return false;
      if (V == kVOrswot ? sub == 1 : sub == 0) {  // the value's Rm: clock, set
        if (k + 8 > nw) return false;
        n = w.at64(k + 6, lane);
        if (n > (nw - k - 8) / 3) return false;
        const unsigned long long p = uni64(k + 8 + 3 * n);
        if (p + 2 > nw) return false;
        cnt = w.at64(p, lane);
        if (V == kVOrswot) {
          if (cnt > (nw - p - 2) / 2) return false;
          next = p + 2 + 2 * cnt;
        } else {
          if (cnt > nw - p - 2) return false;
          next = p + 2 + cnt;
        }
      } else if (V == kVOrswot) {  // Add: dot, members
        if (k + 11 > nw) return false;
        cnt = w.at64(k + 9, lane);
        if (cnt > (nw - k - 11) / 2) return false;
        next = k + 11 + 2 * cnt;
      } else {  // inner Up: dot, ikey, MVReg tag, clock, val
        if (k + 13 > nw) return false;
        if (w.at(k + 10, lane) != 0) return false;
        n = w.at64(k + 11, lane);
        if (n > (nw - k - 13) / 3) return false;
        next = k + 13 + 3 * n + 2;
        if (next > nw) return false;
      }
    }
    emit(k, tag, sub, uni64(n), uni64(cnt));
    k = uni64(next);
  }
  return k == nw;
}

__device__ __forceinline__ bool vops_frame(const VOpsPlan &p, unsigned long long s, OpWalk &w, uint32_t *ring) {
  const u64 b = p.frame_off[s], e = p.frame_off[s + 1];
  if ((b & 3) || (e & 3) || e < b || e - b < 8) return false;
  w.fw = reinterpret_cast<const uint32_t *>(p.bytes + b);
  w.nw = (e - b) / 4;
  w.nwin = (w.nw + kWalkWin - 1) / kWalkWin;
  w.ring = ring;
  return true;
}

template <int V>
__global__ __launch_bounds__(kBlock) void vops_count_kernel(VOpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  uint32_t *ring = reinterpret_cast<uint32_t *>(lds) + (size_t)wib * kWalkRing * kWalkWin;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kVoWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kVoWpb) {
    unsigned st = 0;
    u64 no = 0, nr = 0, nk = 0, nm = 0;
    OpWalk w;
    if (!vops_frame(p, s, w, ring)) {
      st = kWireBad;
    } else {
      w.start(lane);
      const bool ok = walk_vops<V>(w, lane, [&](unsigned long long, uint32_t tag, uint32_t sub, unsigned long long,
                                                unsigned long long cnt) {
        ++no;
        nr += vo_has_row<V>(tag, sub) ? 1 : 0;
        nk += tag == 0 ? cnt : 0;
        if (V == kVOrswot) nm += tag == 1 ? cnt : 0;
      });
      wire_vmcnt<0>();  // no DMA of this frame may land in the ring after the next one starts
      if (!ok) {
        st = kWireBad;
        no = nr = nk = nm = 0;
      }
    }
    if (lane == 0) {
      p.status[s] = st;
      p.counts[s] = no;
      p.counts[p.N + s] = nr;
      p.counts[2 * p.N + s] = nk;
      p.counts[3 * p.N + s] = nm;
    }
  }
}

struct VoCaps {
  u64 c[4];
};

template <int V>
__global__ __launch_bounds__(kBlock) void vops_fill_kernel(VOpsPlan p) {
  extern __shared__ u64 lds[];
  const int lane = threadIdx.x % kWave, wib = threadIdx.x / kWave;
  const uint32_t *actors = p.actors, *keys = p.keys, *idict = p.idict;
  const u64 *members = p.members;
  u64 *base = lds;
  if (p.dict_words) {  // [actors u32 | keys u32 | members u64 or inner keys u32], each padded to 8 bytes
    uint32_t *la = reinterpret_cast<uint32_t *>(lds);
    for (unsigned long long i = threadIdx.x; i < p.A; i += blockDim.x) la[i] = p.actors[i];
    uint32_t *lk = reinterpret_cast<uint32_t *>(lds + (p.A + 1) / 2);
    for (unsigned long long i = threadIdx.x; i < p.K; i += blockDim.x) lk[i] = p.keys[i];
    u64 *lu = lds + (p.A + 1) / 2 + (p.K + 1) / 2;
    if (V == kVOrswot) {
      for (unsigned long long i = threadIdx.x; i < p.U; i += blockDim.x) lu[i] = p.members[i];
      members = lu;
    } else if (V == kVNested) {
      uint32_t *li = reinterpret_cast<uint32_t *>(lu);
      for (unsigned long long i = threadIdx.x; i < p.U; i += blockDim.x) li[i] = p.idict[i];
      idict = li;
    }
    __syncthreads();
    actors = la;
    keys = lk;
    base = lds + p.dict_words;
  }
  uint32_t *ring = reinterpret_cast<uint32_t *>(base) + (size_t)wib * kWalkRing * kWalkWin;
  const unsigned long long A = p.A, K2w = p.K2w;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kVoWpb + wib; s < p.N;
       s += (unsigned long long)gridDim.x * kVoWpb) {
    const unsigned st = p.status[s];
    const u64 o0 = p.op_off[s], r0 = p.row_off[s], k0 = p.key_first[s];
    const u64 m0 = V == kVOrswot ? p.mem_first[s] : 0;  // (the other Maps have no members and no mem_first)
    OpWalk w;
    if ((st & (kWireBad | kWireCap)) || p.op_off[s + 1] == o0 || !vops_frame(p, s, w, ring)) continue;
    w.start(lane);
    const uint32_t *fw = w.fw;
    // the batch of ops the lanes parse next: lane i holds op i of it
    int cnt = 0;
    u64 done = 0, rows_run = 0, keys_run = 0, mems_run = 0, batch_row = 0;
    unsigned long long d_pos = 0, d_n = 0, d_cnt = 0, d_row = 0, d_key = 0, d_mem = 0;
    uint32_t d_tag = 0, d_sub = 0;
    bool miss = false;
    // one id of a list: kind 0 = keyset key, 1 = Orswot member, 2 = inner key (a mask bit, returned)
    auto one_id = [&](int idk, unsigned long long pos, unsigned long long i, uint32_t *dst, u64 &m0w, u64 &m1w, u64 &m2w,
                      u64 &m3w) {
      long long ix;
      if (V == kVOrswot && idk == 1) ix = find_u64(members, p.U, rd64(fw, pos + 2 * i), ~0ull);
      else if (V == kVNested && idk == 2) ix = find_u32(idict, p.U, fw[pos + i], ~0ull);
      else ix = find_u32(keys, p.K, fw[pos + i], ~0ull);
      if (ix < 0) miss = true;
      if (V == kVNested && idk == 2) {  // a missing inner key has no slot in a mask: left out
        if (ix >= 0) {
          const u64 bit = 1ull << (ix & 63);
          const long long wd = ix >> 6;
          m0w |= wd == 0 ? bit : 0;
          m1w |= wd == 1 ? bit : 0;
          m2w |= wd == 2 ? bit : 0;
          m3w |= wd == 3 ? bit : 0;
        }
      } else {
        dst[i] = ix < 0 ? 0xFFFFFFFFu : (uint32_t)ix;
      }
    };
    auto flush = [&]() __attribute__((always_inline)) {
      // the batch's clock rows are contiguous: zeroed here, coalesced, and landed before the records
      u64 *rows = p.pool + (r0 + batch_row) * A;
      const unsigned long long nz = (rows_run - batch_row) * A;
      for (unsigned long long x = lane; x < nz; x += kWave) rows[x] = 0;
      wire_vmcnt<0>();
      const bool on = lane < cnt;
      const bool rm = d_tag == 0;
      const bool hrow = on && vo_has_row<V>(d_tag, d_sub);
      unsigned long long ids_pos = 0, rec = 0, icnt = 0;
      int idk = 0;
      uint32_t *idst = nullptr;
      u64 mk0 = 0, mk1 = 0, mk2 = 0, mk3 = 0;
      u64 o = 0;
      if (on) {
        o = o0 + done + lane;
        p.kind[o] = rm ? 1 : 0;
        p.row[o] = hrow ? (uint32_t)(r0 + d_row) : 0u;
        p.key_off[o + 1] = k0 + d_key + (rm ? d_cnt : 0);
        if (V == kVOrswot) p.mem_off[o + 1] = m0 + d_mem + (rm ? 0 : d_cnt);
        uint32_t vact = 0, ik = 0;
        u64 vcnt = 0, val = 0;
        uint8_t sub = 0;
        if (rm) {
          p.actor[o] = 0;
          p.counter[o] = 0;
          p.key[o] = 0;
          rec = d_pos + 3;
          ids_pos = d_pos + 3 + 3 * d_n + 2;
          icnt = d_cnt;
          idst = p.keys_out + k0 + d_key;
        } else {
          const long long col = find_u32(actors, A, fw[d_pos + 1], ~0ull);
          const long long kx = find_u32(keys, p.K, fw[d_pos + 4], ~0ull);
          if (col < 0 || kx < 0) miss = true;
          p.actor[o] = col < 0 ? 0xFFFFFFFFu : (uint32_t)col;
          p.counter[o] = rd64(fw, d_pos + 2);
          p.key[o] = kx < 0 ? 0xFFFFFFFFu : (uint32_t)kx;
          unsigned long long vdot = 0;  // the value op's dot, if it has one
          if (V == kVG || V == kVPN) {
            vdot = d_pos + 5;
            sub = (uint8_t)d_sub;
          } else if (V == kVOrswot) {
            sub = (uint8_t)d_sub;
            idk = 1;
            icnt = d_cnt;
            idst = p.mems + m0 + d_mem;
            if (d_sub == 0) {
              vdot = d_pos + 6;
              ids_pos = d_pos + 11;
            } else {
              rec = d_pos + 8;
              ids_pos = d_pos + 8 + 3 * d_n + 2;
            }
          } else {
            sub = (uint8_t)(d_sub ^ 1u);
            if (d_sub == 1) {
              vdot = d_pos + 6;
              const long long jx = find_u32(idict, p.U, fw[d_pos + 9], ~0ull);
              if (jx < 0) miss = true;
              ik = jx < 0 ? 0xFFFFFFFFu : (uint32_t)jx;
              rec = d_pos + 13;
              val = rd64(fw, d_pos + 13 + 3 * d_n);
            } else {
              idk = 2;
              icnt = d_cnt;
              rec = d_pos + 8;
              ids_pos = d_pos + 8 + 3 * d_n + 2;
            }
          }
          if (vdot) {
            const long long vc = find_u32(actors, A, fw[vdot], ~0ull);
            if (vc < 0) miss = true;
            vact = vc < 0 ? 0xFFFFFFFFu : (uint32_t)vc;
            vcnt = rd64(fw, vdot + 1);
          }
        }
        p.sub[o] = sub;
        p.vactor[o] = vact;
        p.vcounter[o] = vcnt;
        if (V == kVNested) {
          p.ikey[o] = ik;
          p.val[o] = val;
        }
        if (hrow) {
          u64 *dst = p.pool + (r0 + d_row) * A;
          for (unsigned long long r = 0; r < (d_n <= (unsigned long long)kVoLaneRecs ? d_n : 0); ++r) {
            const uint32_t id = fw[rec + 3 * r];
            const u64 c = rd64(fw, rec + 3 * r + 1);
            const long long col = find_u32(actors, A, id, r);
            if (col < 0) miss = true;
            else dst[col] = c;
          }
        }
        if (icnt <= (unsigned long long)kVoLaneIds)
          for (unsigned long long i = 0; i < icnt; ++i) one_id(idk, ids_pos, i, idst, mk0, mk1, mk2, mk3);
      }
      // a clock with more records than a lane takes: the wave loops over them
      u64 wclk = __ballot(hrow && d_n > (unsigned long long)kVoLaneRecs);
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
      u64 wide = __ballot(on && icnt > (unsigned long long)kVoLaneIds);
      while (wide) {
        const int j = __ffsll((unsigned long long)wide) - 1;
        wide &= wide - 1;
        const unsigned long long jp = __shfl(ids_pos, j, kWave), jc = __shfl(icnt, j, kWave);
        const int jk = __shfl(idk, j, kWave);
        const unsigned long long dlo = __shfl((unsigned)(uintptr_t)idst, j, kWave);
        const unsigned long long dhi = __shfl((unsigned)((uintptr_t)idst >> 32), j, kWave);
        uint32_t *dst = reinterpret_cast<uint32_t *>((uintptr_t)((dhi << 32) | dlo));
        u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (unsigned long long i = lane; i < jc; i += kWave) one_id(jk, jp, i, dst, a0, a1, a2, a3);
        if (V == kVNested && jk == 2) {  // the lanes' bits -> the op's lane
          for (int off = kWave / 2; off > 0; off >>= 1) {
            a0 |= __shfl_xor(a0, off, kWave);
            a1 |= __shfl_xor(a1, off, kWave);
            a2 |= __shfl_xor(a2, off, kWave);
            a3 |= __shfl_xor(a3, off, kWave);
          }
          if (lane == j) {
            mk0 = a0;
            mk1 = a1;
            mk2 = a2;
            mk3 = a3;
          }
        }
      }
      if (V == kVNested && on) {
        u64 *mw = p.imask + o * K2w;
        mw[0] = mk0;
        if (K2w > 1) mw[1] = mk1;
        if (K2w > 2) mw[2] = mk2;
        if (K2w > 3) mw[3] = mk3;
      }
      done += cnt;
      cnt = 0;
      batch_row = rows_run;
    };
    walk_vops<V>(w, lane, [&](unsigned long long pos, uint32_t tag, uint32_t sub, unsigned long long n, unsigned long long c) {
      if (lane == cnt) {
        d_pos = pos;
        d_tag = tag;
        d_sub = sub;
        d_n = n;
        d_cnt = c;
        d_row = rows_run;
        d_key = keys_run;
        d_mem = mems_run;
      }
      rows_run += vo_has_row<V>(tag, sub) ? 1 : 0;
      keys_run += tag == 0 ? c : 0;
      if (V == kVOrswot) mems_run += tag == 1 ? c : 0;
      if (++cnt == kWave) flush();
    });
    if (cnt) flush();
    wire_vmcnt<0>();
    if (__ballot(miss) && lane == 0) p.status[s] = st | kWireMissing;
  }
}

// ---- egress ---------------------------------------------------------------------------------------
struct VOpsEgressPlan {
  unsigned long long N, A, K, U, K2w, n_ops, n_rows, n_keys, n_mems;
  const u64 *op_off;
  const uint8_t *kind;
  const uint32_t *actor;
  const u64 *counter;
  const uint32_t *key;
  const uint8_t *sub;       // vdir (may be NULL) / vkind / ikind
  const uint32_t *vactor;
  const u64 *vcounter;
  const uint32_t *ikey;
  const u64 *val;
  const u64 *imask;
  const uint32_t *row;
  const u64 *pool;
  const u64 *key_off;
  const uint32_t *keys_pool;
  const u64 *mem_off;
  const uint32_t *mems;
  const uint32_t *actors, *keys, *idict;
  const u64 *members;
  u64 *sizes;
  const u64 *frame_off;
  uint8_t *bytes;
  uint32_t *status;
};

__device__ __forceinline__ u64 vo_wave_excl(u64 v, int lane, u64 &total) {
  u64 x = v;
  for (int d = 1; d < kWave; d <<= 1) {
    const u64 y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  total = __shfl(x, kWave - 1, kWave);
  return x - v;
}

// One wave per state, lane = op in batches of 64.  write = 0: validate every op, size the frame
// (status[s], sizes[s]); write = 1: write it at frame_off[s] (the empty Vec for a state with bit 1).
template <int V>
__global__ __launch_bounds__(kBlock) void vops_egress_kernel(VOpsEgressPlan p, int write) {
  const int lane = threadIdx.x % kWave;
  const unsigned long long w0 = (blockIdx.x * (unsigned long long)kBlock + threadIdx.x) / kWave;
  const unsigned long long nwv = (unsigned long long)gridDim.x * kVoWpb;
  const unsigned long long A = p.A, K2w = p.K2w;
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
      int idk = -1;  // the op's id list: 0 = keyset keys, 1 = members, -1 = none
      uint32_t k = 0, sub = 0;
      unsigned long long r = 0, ib = 0, ie = 0, nbits = 0;
      if (on) {
        k = p.kind[o];
        if (k > 1) lbad = true;
        else if (k == 1) {
          has_row = true;
          idk = 0;
        } else {
          if (p.actor[o] >= A || p.key[o] >= p.K) lbad = true;
          if (V == kVG || V == kVPN) {
            sub = p.sub ? p.sub[o] : 0u;
            if (sub > (V == kVPN ? 1u : 0u) || p.vactor[o] >= A) lbad = true;
          } else if (V == kVOrswot) {
            sub = p.sub[o];
            idk = 1;
            if (sub > 1) lbad = true;
            else if (sub == 1) has_row = true;
            else if (p.vactor[o] >= A) lbad = true;
          } else {
            sub = p.sub[o];
            has_row = true;
            if (sub > 1) lbad = true;
            else if (sub == 0) {
              if (p.vactor[o] >= A || p.ikey[o] >= p.U) lbad = true;
            } else {  // no mask bit at or past K2
              for (unsigned long long x = 0; x < K2w; ++x) {
                const u64 m = p.imask[o * K2w + x];
                const unsigned long long lo = 64 * x;
                const u64 okm = p.U >= lo + 64 ? ~0ull : (p.U > lo ? (1ull << (p.U - lo)) - 1 : 0ull);
                if (m & ~okm) lbad = true;
                nbits += __popcll(m);
              }
            }
          }
        }
        if (!lbad && has_row) {
          r = p.row[o];
          if (r >= p.n_rows) lbad = true;
        }
        if (!lbad && idk >= 0) {
          const u64 *offs = idk == 0 ? p.key_off : p.mem_off;
          if (!offs) lbad = true;
          else {
            ib = offs[o];
            ie = offs[o + 1];
            const unsigned long long np = idk == 0 ? p.n_keys : p.n_mems;
            if (ie < ib || ie > np || (ie > ib && !(idk == 0 ? p.keys_pool : p.mems))) lbad = true;
          }
        }
        if (lbad) {
          has_row = false;
          ib = ie = 0;
          idk = -1;
        }
      }
      const unsigned long long ic = ie - ib;
      const uint32_t *ipool = idk == 1 ? p.mems : p.keys_pool;
      const unsigned long long ibound = idk == 1 ? p.U : p.K;
      if (!write) {  // every id names a dictionary entry
        if (on && ic <= (unsigned long long)kVoLaneIds)
          for (unsigned long long i = ib; i < ie; ++i) lbad |= ipool[i] >= ibound;
        u64 wide = __ballot(on && ic > (unsigned long long)kVoLaneIds);
        while (wide) {
          const int j = __ffsll((unsigned long long)wide) - 1;
          wide &= wide - 1;
          const unsigned long long jb = __shfl(ib, j, kWave), je = __shfl(ie, j, kWave);
          const int jk = __shfl(idk, j, kWave);
          const uint32_t *jpool = jk == 1 ? p.mems : p.keys_pool;
          const unsigned long long jbound = jk == 1 ? p.U : p.K;
          bool x = false;
          for (unsigned long long i = jb + lane; i < je; i += kWave) x |= jpool[i] >= jbound;
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
        if (k == 1) words = 5 + 3 * nnz + ic;
        else if (V == kVG) words = 8;
        else if (V == kVPN) words = 9;
        else if (V == kVOrswot) words = sub == 0 ? 11 + 2 * ic : 10 + 3 * nnz + 2 * ic;
        else words = sub == 0 ? 15 + 3 * nnz : 10 + 3 * nnz + nbits;
      }
      if (__ballot(lbad)) bad = true;
      u64 total;
      const u64 kp = run + vo_wave_excl(words, lane, total);
      run += total;
      if (!write || bad) continue;
      // headers, by the op's lane
      unsigned long long ids_at = 0, clk_at = 0;
      if (on) {
        out[kp] = k ^ 1u;
        if (k == 1) {
          clk_at = kp + 1;
          wr64(out, kp + 3 + 3 * nnz, ic);
          ids_at = kp + 5 + 3 * nnz;
        } else {
          out[kp + 1] = p.actors[p.actor[o]];
          wr64(out, kp + 2, p.counter[o]);
          out[kp + 4] = p.keys[p.key[o]];
          if (V == kVG || V == kVPN) {
            out[kp + 5] = p.actors[p.vactor[o]];
            wr64(out, kp + 6, p.vcounter[o]);
            if (V == kVPN) out[kp + 8] = sub;
          } else if (V == kVOrswot) {
            out[kp + 5] = sub;
            if (sub == 0) {
              out[kp + 6] = p.actors[p.vactor[o]];
              wr64(out, kp + 7, p.vcounter[o]);
              wr64(out, kp + 9, ic);
              ids_at = kp + 11;
            } else {
              clk_at = kp + 6;
              wr64(out, kp + 8 + 3 * nnz, ic);
              ids_at = kp + 10 + 3 * nnz;
            }
          } else {
            out[kp + 5] = sub ^ 1u;
            if (sub == 0) {
              out[kp + 6] = p.actors[p.vactor[o]];
              wr64(out, kp + 7, p.vcounter[o]);
              out[kp + 9] = p.idict[p.ikey[o]];
              out[kp + 10] = 0;
              clk_at = kp + 11;
              wr64(out, kp + 13 + 3 * nnz, p.val[o]);
            } else {  // the mask's bits ascending (at most K2 <= 256 of them)
              clk_at = kp + 6;
              wr64(out, kp + 8 + 3 * nnz, nbits);
              unsigned long long at = kp + 10 + 3 * nnz;
              for (unsigned long long x = 0; x < K2w; ++x) {
                u64 m = p.imask[o * K2w + x];
                while (m) {
                  const int bit = __ffsll((unsigned long long)m) - 1;
                  m &= m - 1;
                  out[at++] = p.idict[64 * x + bit];
                }
              }
            }
          }
        }
        if (ic <= (unsigned long long)kVoLaneIds)
          for (unsigned long long i = 0; i < ic; ++i) {
            if (idk == 1) wr64(out, ids_at + 2 * i, p.members[ipool[ib + i]]);
            else out[ids_at + i] = p.keys[ipool[ib + i]];
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
      u64 wide = __ballot(on && ic > (unsigned long long)kVoLaneIds);
      while (wide) {
        const int j = __ffsll((unsigned long long)wide) - 1;
        wide &= wide - 1;
        const unsigned long long jb = __shfl(ib, j, kWave), jc = __shfl(ic, j, kWave), ja = __shfl(ids_at, j, kWave);
        const int jk = __shfl(idk, j, kWave);
        const uint32_t *jpool = jk == 1 ? p.mems : p.keys_pool;
        for (unsigned long long i = lane; i < jc; i += kWave) {
          if (jk == 1) wr64(out, ja + 2 * i, p.members[jpool[jb + i]]);
          else out[ja + i] = p.keys[jpool[jb + i]];
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
template <int V>
static int vops_ingest(crdt_ctx *ctx, VOpsPlan p, const VoCaps &caps, bool fill, u64 *op_off, u64 *row_off, u64 *key_first,
                       u64 *mem_first, uint64_t *totals) {
  const size_t ring_bytes = (size_t)kVoWpb * kWalkRing * kWalkWin * 4;
  const unsigned grid = wave_grid(ctx, p.N, kVoWpb, 8);
  // (a Map without members passes no mem_first: its member count is always 0 and is not read back)
  const SizedOut<4> o{{caps.c[0], caps.c[1], caps.c[2], caps.c[3]}, {op_off, row_off, key_first, mem_first},
                      {p.key_off, p.mem_off}, p.status};
  return sized_ingest<4>(
      ctx, "wire_vmap_ops_ingest", p.N, o, fill, totals,
      [&](u64 *counts) {
        p.counts = counts;
        hipLaunchKernelGGL(vops_count_kernel<V>, dim3(grid), dim3(kBlock), ring_bytes, ctx->stream, p);
      },
      [&] {
        p.op_off = op_off;
        p.row_off = row_off;
        p.key_first = key_first;
        p.mem_first = mem_first;
        const unsigned long long dw =
            (p.A + 1) / 2 + (p.K + 1) / 2 + (V == kVOrswot ? p.U : (V == kVNested ? (p.U + 1) / 2 : 0));
        p.dict_words = dw * 8 + ring_bytes <= kVoLdsMax ? dw : 0;  // else: searched in global memory
        hipLaunchKernelGGL(vops_fill_kernel<V>, dim3(grid), dim3(kBlock), ring_bytes + p.dict_words * 8, ctx->stream, p);
      });
}

static int vops_ingest_any(int V, crdt_ctx *ctx, const VOpsPlan &p, const VoCaps &caps, bool fill, u64 *op_off, u64 *row_off,
                           u64 *key_first, u64 *mem_first, uint64_t *totals) {
  switch (V) {
    case kVG: return vops_ingest<kVG>(ctx, p, caps, fill, op_off, row_off, key_first, mem_first, totals);
    case kVPN: return vops_ingest<kVPN>(ctx, p, caps, fill, op_off, row_off, key_first, mem_first, totals);
    case kVOrswot: return vops_ingest<kVOrswot>(ctx, p, caps, fill, op_off, row_off, key_first, mem_first, totals);
    default: return vops_ingest<kVNested>(ctx, p, caps, fill, op_off, row_off, key_first, mem_first, totals);
  }
}

static int vops_egress(int V, crdt_ctx *ctx, VOpsEgressPlan p, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                       size_t *total) {
  void (*kern)(VOpsEgressPlan, int) = V == kVG       ? vops_egress_kernel<kVG>
                                      : V == kVPN    ? vops_egress_kernel<kVPN>
                                      : V == kVOrswot ? vops_egress_kernel<kVOrswot>
                                                      : vops_egress_kernel<kVNested>;
  return two_pass_egress(ctx, "wire_vmap_ops_egress", kern, p, wave_grid(ctx, p.N, kVoWpb, 32), frame_off, bytes, cap, total);
}

// the argument checks the three ingests share; the plan's dictionaries and frames
static int vops_ingest_head(crdt_ctx *ctx, const char *what, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                            const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, bool has_out,
                            uint32_t *status, uint64_t *totals, VOpsPlan &p) {
  if (int rc = check_frames(ctx, bytes, frame_off, N, status)) return rc;
  if (!actors || !keys || A == 0 || K == 0) return fail(ctx, CRDT_EINVAL, "%s: need the actor and key dictionaries", what);
  if (!has_out && !totals) return fail(ctx, CRDT_EINVAL, "%s: neither an output nor totals asked for", what);
  p.bytes = bytes;
  p.frame_off = (const u64 *)frame_off;
  p.N = N;
  p.actors = actors;
  p.A = A;
  p.keys = keys;
  p.K = K;
  p.K2w = 1;
  p.status = status;
  return CRDT_OK;
}

}  // namespace crdt

using namespace crdt;

extern "C" {

int crdt_map_counter_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                                const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, int pn,
                                const crdt_map_counter_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                                uint32_t *status, uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
  if (N == 0) return CRDT_OK;
  const char *what = "map_counter_ops_ingest";
  if (pn != 0 && pn != 1) return fail(ctx, CRDT_EINVAL, "%s: pn must be 0 (GCounter) or 1 (PNCounter)", what);
  VOpsPlan p{};
  if (int rc = vops_ingest_head(ctx, what, bytes, frame_off, N, actors, A, keys, K, out != nullptr, status, totals, p))
    return rc;
  VoCaps caps{};
  if (out) {
    if (!out->op_off || !row_off || !key_first || !out->key_off ||
        (out->op_cap && (!out->kind || !out->actor || !out->counter || !out->key || !out->vactor || !out->vcounter ||
                         !out->vdir || !out->clk_row)) ||
        (out->row_cap && !out->clk_pool) || (out->key_cap && !out->keys))
      return fail(ctx, CRDT_EINVAL, "%s: NULL output array", what);
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "%s: row_cap past 2^32 - 1", what);
    p.kind = out->kind;
    p.actor = out->actor;
    p.counter = (u64 *)out->counter;
    p.key = out->key;
    p.sub = out->vdir;
    p.vactor = out->vactor;
    p.vcounter = (u64 *)out->vcounter;
    p.row = out->clk_row;
    p.pool = (u64 *)out->clk_pool;
    p.key_off = (u64 *)out->key_off;
    p.keys_out = out->keys;
    caps.c[0] = out->op_cap;
    caps.c[1] = out->row_cap;
    caps.c[2] = out->key_cap;
    caps.c[3] = 0;  // a counter Map has no members: the count is always 0
  }
  return vops_ingest_any(pn ? kVPN : kVG, ctx, p, caps, out != nullptr, out ? (u64 *)out->op_off : nullptr, (u64 *)row_off,
                         (u64 *)key_first, nullptr, totals);
}

int crdt_map_orswot_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                               const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const uint64_t *members,
                               size_t M, const crdt_map_orswot_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                               uint64_t *mem_first, uint32_t *status, uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
  if (N == 0) return CRDT_OK;
  const char *what = "map_orswot_ops_ingest";
  VOpsPlan p{};
  if (int rc = vops_ingest_head(ctx, what, bytes, frame_off, N, actors, A, keys, K, out != nullptr, status, totals, p))
    return rc;
  if (!members || M == 0) return fail(ctx, CRDT_EINVAL, "%s: need the member dictionary", what);
  p.members = (const u64 *)members;
  p.U = M;
  VoCaps caps{};
  if (out) {
    if (!out->op_off || !row_off || !key_first || !mem_first || !out->key_off || !out->mem_off ||
        (out->op_cap && (!out->kind || !out->actor || !out->counter || !out->key || !out->vkind || !out->vactor ||
                         !out->vcounter || !out->clk_row)) ||
        (out->row_cap && !out->clk_pool) || (out->key_cap && !out->keys) || (out->mem_cap && !out->mems))
      return fail(ctx, CRDT_EINVAL, "%s: NULL output array", what);
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "%s: row_cap past 2^32 - 1", what);
    p.kind = out->kind;
    p.actor = out->actor;
    p.counter = (u64 *)out->counter;
    p.key = out->key;
    p.sub = out->vkind;
    p.vactor = out->vactor;
    p.vcounter = (u64 *)out->vcounter;
    p.row = out->clk_row;
    p.pool = (u64 *)out->clk_pool;
    p.key_off = (u64 *)out->key_off;
    p.keys_out = out->keys;
    p.mem_off = (u64 *)out->mem_off;
    p.mems = out->mems;
    caps.c[0] = out->op_cap;
    caps.c[1] = out->row_cap;
    caps.c[2] = out->key_cap;
    caps.c[3] = out->mem_cap;
  }
  return vops_ingest_any(kVOrswot, ctx, p, caps, out != nullptr, out ? (u64 *)out->op_off : nullptr, (u64 *)row_off,
                         (u64 *)key_first, (u64 *)mem_first, totals);
}

int crdt_map_nested_ops_ingest(crdt_ctx *ctx, const uint8_t *bytes, const uint64_t *frame_off, size_t N,
                               const uint32_t *actors, size_t A, const uint32_t *keys, size_t K, const uint32_t *idict,
                               size_t K2, const crdt_map_nested_ops_buf *out, uint64_t *row_off, uint64_t *key_first,
                               uint32_t *status, uint64_t *totals) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
  const char *what = "map_nested_ops_ingest";
  if (K2 > 256) return fail(ctx, CRDT_EUNSUPPORTED, "%s: K2 = %zu > 256", what, K2);
  if (N == 0) return CRDT_OK;
  VOpsPlan p{};
  if (int rc = vops_ingest_head(ctx, what, bytes, frame_off, N, actors, A, keys, K, out != nullptr, status, totals, p))
    return rc;
  if (!idict || K2 == 0) return fail(ctx, CRDT_EINVAL, "%s: need the inner-key dictionary", what);
  p.idict = idict;
  p.U = K2;
  p.K2w = K2 > 64 ? (K2 + 63) / 64 : 1;
  VoCaps caps{};
  if (out) {
    if (!out->op_off || !row_off || !key_first || !out->key_off ||
        (out->op_cap && (!out->kind || !out->actor || !out->counter || !out->key || !out->ikind || !out->iactor ||
                         !out->icounter || !out->ikey || !out->val || !out->ikeys || !out->clk_row)) ||
        (out->row_cap && !out->clk_pool) || (out->key_cap && !out->keys))
      return fail(ctx, CRDT_EINVAL, "%s: NULL output array", what);
    if (out->row_cap > 0xFFFFFFFFull) return fail(ctx, CRDT_EINVAL, "%s: row_cap past 2^32 - 1", what);
    p.kind = out->kind;
    p.actor = out->actor;
    p.counter = (u64 *)out->counter;
    p.key = out->key;
    p.sub = out->ikind;
    p.vactor = out->iactor;
    p.vcounter = (u64 *)out->icounter;
    p.ikey = out->ikey;
    p.val = (u64 *)out->val;
    p.imask = (u64 *)out->ikeys;
    p.row = out->clk_row;
    p.pool = (u64 *)out->clk_pool;
    p.key_off = (u64 *)out->key_off;
    p.keys_out = out->keys;
    caps.c[0] = out->op_cap;
    caps.c[1] = out->row_cap;
    caps.c[2] = out->key_cap;
    caps.c[3] = 0;
  }
  return vops_ingest_any(kVNested, ctx, p, caps, out != nullptr, out ? (u64 *)out->op_off : nullptr, (u64 *)row_off,
                         (u64 *)key_first, nullptr, totals);
}

int crdt_map_counter_ops_egress(crdt_ctx *ctx, const crdt_map_counter_ops *ops, size_t N, const uint32_t *actors, size_t A,
                                const uint32_t *keys, size_t K, int pn, uint64_t *frame_off, uint8_t *bytes, size_t cap,
                                size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  const char *what = "map_counter_ops_egress";
  if (pn != 0 && pn != 1) return fail(ctx, CRDT_EINVAL, "%s: pn must be 0 (GCounter) or 1 (PNCounter)", what);
  if (!ops || !ops->op_off || !actors || !keys || A == 0 || K == 0)
    return fail(ctx, CRDT_EINVAL, "%s: need ops (op_off) and the dictionaries", what);
  if (ops->n_ops && (!ops->kind || !ops->actor || !ops->counter || !ops->key || !ops->vactor || !ops->vcounter ||
                     !ops->clk_row || !ops->clk_pool))
    return fail(ctx, CRDT_EINVAL, "%s: NULL op array", what);
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "%s: need frame_off, total and status", what);
  VOpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.K = K;
  p.K2w = 1;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_clk_rows;
  p.n_keys = ops->n_keys;
  p.op_off = (const u64 *)ops->op_off;
  p.kind = ops->kind;
  p.actor = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.key = ops->key;
  p.sub = ops->vdir;
  p.vactor = ops->vactor;
  p.vcounter = (const u64 *)ops->vcounter;
  p.row = ops->clk_row;
  p.pool = (const u64 *)ops->clk_pool;
  p.key_off = (const u64 *)ops->key_off;
  p.keys_pool = ops->keys;
  p.actors = actors;
  p.keys = keys;
  p.status = status;
  return vops_egress(pn ? kVPN : kVG, ctx, p, frame_off, bytes, cap, total);
}

int crdt_map_orswot_ops_egress(crdt_ctx *ctx, const crdt_map_orswot_ops *ops, size_t N, const uint32_t *actors, size_t A,
                               const uint32_t *keys, size_t K, const uint64_t *members, size_t M, uint64_t *frame_off,
                               uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  if (N == 0) return CRDT_OK;
  const char *what = "map_orswot_ops_egress";
  if (!ops || !ops->op_off || !actors || !keys || !members || A == 0 || K == 0 || M == 0)
    return fail(ctx, CRDT_EINVAL, "%s: need ops (op_off) and the dictionaries", what);
  if (ops->n_ops && (!ops->kind || !ops->actor || !ops->counter || !ops->key || !ops->vkind || !ops->vactor ||
                     !ops->vcounter || !ops->clk_row || !ops->clk_pool || !ops->mem_off))
    return fail(ctx, CRDT_EINVAL, "%s: NULL op array", what);
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "%s: need frame_off, total and status", what);
  VOpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.K = K;
  p.U = M;
  p.K2w = 1;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_clk_rows;
  p.n_keys = ops->n_keys;
  p.n_mems = ops->n_mems;
  p.op_off = (const u64 *)ops->op_off;
  p.kind = ops->kind;
  p.actor = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.key = ops->key;
  p.sub = ops->vkind;
  p.vactor = ops->vactor;
  p.vcounter = (const u64 *)ops->vcounter;
  p.row = ops->clk_row;
  p.pool = (const u64 *)ops->clk_pool;
  p.key_off = (const u64 *)ops->key_off;
  p.keys_pool = ops->keys;
  p.mem_off = (const u64 *)ops->mem_off;
  p.mems = ops->mems;
  p.actors = actors;
  p.keys = keys;
  p.members = (const u64 *)members;
  p.status = status;
  return vops_egress(kVOrswot, ctx, p, frame_off, bytes, cap, total);
}

int crdt_map_nested_ops_egress(crdt_ctx *ctx, const crdt_map_nested_ops *ops, size_t N, const uint32_t *actors, size_t A,
                               const uint32_t *keys, size_t K, const uint32_t *idict, size_t K2, uint64_t *frame_off,
                               uint8_t *bytes, size_t cap, size_t *total, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (total) *total = 0;
  const char *what = "map_nested_ops_egress";
  if (K2 > 256) return fail(ctx, CRDT_EUNSUPPORTED, "%s: K2 = %zu > 256", what, K2);
  if (N == 0) return CRDT_OK;
  if (!ops || !ops->op_off || !actors || !keys || !idict || A == 0 || K == 0 || K2 == 0)
    return fail(ctx, CRDT_EINVAL, "%s: need ops (op_off) and the dictionaries", what);
  if (ops->n_ops && (!ops->kind || !ops->actor || !ops->counter || !ops->key || !ops->ikind || !ops->iactor ||
                     !ops->icounter || !ops->ikey || !ops->val || !ops->ikeys || !ops->clk_row || !ops->clk_pool))
    return fail(ctx, CRDT_EINVAL, "%s: NULL op array", what);
  if (!frame_off || !total || !status) return fail(ctx, CRDT_EINVAL, "%s: need frame_off, total and status", what);
  VOpsEgressPlan p{};
  p.N = N;
  p.A = A;
  p.K = K;
  p.U = K2;
  p.K2w = K2 > 64 ? (K2 + 63) / 64 : 1;
  p.n_ops = ops->n_ops;
  p.n_rows = ops->n_clk_rows;
  p.n_keys = ops->n_keys;
  p.op_off = (const u64 *)ops->op_off;
  p.kind = ops->kind;
  p.actor = ops->actor;
  p.counter = (const u64 *)ops->counter;
  p.key = ops->key;
  p.sub = ops->ikind;
  p.vactor = ops->iactor;
  p.vcounter = (const u64 *)ops->icounter;
  p.ikey = ops->ikey;
  p.val = (const u64 *)ops->val;
  p.imask = (const u64 *)ops->ikeys;
  p.row = ops->clk_row;
  p.pool = (const u64 *)ops->clk_pool;
  p.key_off = (const u64 *)ops->key_off;
  p.keys_pool = ops->keys;
  p.actors = actors;
  p.keys = keys;
  p.idict = idict;
  p.status = status;
  return vops_egress(kVNested, ctx, p, frame_off, bytes, cap, total);
}

}  // extern "C"
