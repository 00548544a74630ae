// Batched CmRDT::apply of Map<K, GCounter> / Map<K, PNCounter> (round 5): Map::apply (map.rs:119-137)
// with the counter's apply inside (gcounter.rs:36-42: the value op is a Dot, VClock::apply;
// pncounter.rs:59-68: a Dot and a direction, applied to P or N), apply_keyset_rm (:318-348) and
// apply_deferred (:311-316).  State s applies its ops [op_off[s], op_off[s+1]) in order, in place.
//
// One wave per state (ops are ordered: the "seen" test and the deferred removes depend on what came
// before), lane l holding actors l + 64 j of every row (j < APL), the map clock in registers, the
// state's deferred removes (rm clock + key bitmap) staged in LDS for the whole stream and written
// back at the end.  Per op:
//  * Up { dot (a, c), key k, op (va, vc, dir) }: skipped when clock[a] >= c (seen); else the entry
//    clock's word a and the value row dir's word va take the max with c / vc (VClock::apply), the map
//    clock's word a too, then every deferred remove is re-applied (apply_deferred): its keys' entries
//    forget its clock (an emptied entry is dropped: all-zero rows; a surviving one's value rows
//    forget it too) and it stays deferred while !(clock >= rm);
//  * Rm { clock rm, keyset }: the keys' entries forget rm as above, then rm is deferred unless
//    clock >= rm (an equal clock already deferred unions its key set).
// The forgets of apply_deferred commute (each forget is idempotent; an entry emptied by one stays
// empty), so the HashMap's iteration order does not matter.  Each row word is read and written by
// the lane owning its actor (lane-local), the deferred slots live in LDS.
#include "vmap_apply_frame.hpp"

namespace crdt {

// waves per SIMD asked of the register allocator for A <= 128 (build option; A/B in
// profiles/r05_vapply_wpe_ab.log); the wider instances keep the compiler's choice (they would spill).
// With the op headers batched 64 at a time into lanes the kernel runs at 7 waves per SIMD (room for
// the batch's registers): 1.89 ms against 2.17 ms for per-op reads at 8 and 2.30 ms for the batch at
// 8 (profiles/r05_vapply_hdr_ab.log, r05_mca_h1w_ab.log)
#ifndef CRDT_MCA_WPE
#define CRDT_MCA_WPE 7
#endif
#ifndef CRDT_MCA_WPE1  // the pass-1 instance (Dcap past the LDS slots): 6, 2.185 vs 2.334 ms at 7
#define CRDT_MCA_WPE1 6    // (profiles/r06_apply_ab.log)
#endif

struct MapCounterApplyPlan {
  u64 *clock, *ec, *val;
  unsigned long long c_s, e_s, v_s;  // state strides (words)
  unsigned long long N, K, A, W, Kw, Dcap;
  unsigned long long Dl;  // deferred slots held in LDS (<= Dcap); slots Dl .. Dcap-1 stay in def_clock / def_keys
  u64 *def_clock, *def_keys;
  unsigned *def_count;
  const u64 *op_off;
  const uint8_t *kind;
  const uint32_t *actor, *key, *vactor;
  const u64 *counter, *vcounter;
  const uint8_t *vdir;
  const uint32_t *clk_row;
  const u64 *clk_pool;
  unsigned long long n_clk_rows;
  const u64 *key_off;
  const uint32_t *keys;
  unsigned long long n_keys, n_ops;
  unsigned *status;
  unsigned wpb;  // waves per block
  u64 *resume;   // [N] (Dcap > Dl): op offset where the state's stream continues in the tier-2 pass, or kVmapDone
};

// What PASS means and the deferred slots (sl) are csrc/vmap_apply_frame.hpp's.  The prologue, the
// Map-level Rm and the epilogue below are the same text in the three value-typed apply kernels: as
// shared functions they cost registers (see the header).
template <int APL, int PASS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(APL <= 2 ? (PASS == 1 ? CRDT_MCA_WPE1 : CRDT_MCA_WPE) : 1))) void map_counter_apply_kernel(MapCounterApplyPlan p) {
  extern __shared__ u64 lds[];
  const int lane = (int)(threadIdx.x % kWave), wv = (int)(threadIdx.x / kWave);
  const unsigned long long s = (unsigned long long)blockIdx.x * p.wpb + wv;
  if (wv >= (int)p.wpb || s >= p.N) return;  // (whole waves)
  constexpr bool TIER = PASS == 2;
  if constexpr (TIER) {
    if (p.resume[s] == kVmapDone) return;
  }
  const unsigned long long A = p.A, K = p.K, W = p.W, Kw = p.Kw, Dcap = p.Dcap, Dl = p.Dl;
  // The Map's deferred removes: slots d < Dl in LDS, slots Dl <= d < Dcap in the caller's own slot
  // arrays (global memory: a long list runs slower, never incomplete below Dcap)
  u64 *sclk = lds + (unsigned long long)wv * Dl * (A + Kw);  // [Dl][A] rm clocks
  u64 *skey = sclk + Dl * A;                                 // [Dl][Kw] key bitmaps
  u64 *gclk = p.def_clock + s * Dcap * A, *gkey = p.def_keys + s * Dcap * Kw;
  const VmapSlots<TIER> sl{sclk, skey, gclk, gkey, A, Kw, Dl, lane};
  const unsigned long long ob = p.op_off[s], oe = p.op_off[s + 1];
  unsigned dcnt = p.def_count[s];
  if (dcnt > Dcap || oe < ob || oe > p.n_ops) {
    if (lane == 0) {
      p.status[s] = (dcnt > Dcap ? 4u : 0u) | (oe < ob || oe > p.n_ops ? 8u : 0u);
      if (PASS == 1) p.resume[s] = kVmapDone;
    }
    return;  // state left untouched
  }
  if constexpr (PASS == 1) {
    if (dcnt > Dl) {  // arrives with more removes than the LDS slots: the whole stream in pass 2
      if (lane == 0) {
        p.status[s] = 0;
        p.resume[s] = 0;
      }
      return;
    }
  }
  // pass 2 continues with pass 1's status bits and from a state whose first deferred pass is not known
  // to have run (full = true below re-forgets every listed key: exact either way)
  unsigned st = TIER ? p.status[s] : 0u, peak = dcnt;  // peak: the most slots held (vacated ones are zeroed)
  const unsigned long long start = TIER ? ob + p.resume[s] : ob;
  u64 *C = p.clock + s * p.c_s, *E = p.ec + s * p.e_s, *V = p.val + s * p.v_s;
  auto word = [&](int j) { return (unsigned long long)lane + 64ull * j; };
  u64 c[APL];
#pragma unroll
  for (int j = 0; j < APL; ++j) c[j] = word(j) < A ? C[word(j)] : 0ull;
  sl.stage_in(dcnt);

  // the clock's word of actor a (uniform)
  auto clock_of = [&](unsigned a) -> u64 {
    u64 x = 0;
#pragma unroll
    for (int j = 0; j < APL; ++j)
      if ((unsigned)j == a / 64) x = c[j];
    return __shfl(x, (int)(a % 64));
  };
  // key k's entry forgets r: dropped (all-zero rows) when its clock empties, else its value too
  auto key_rm = [&](unsigned long long k, const u64 (&r)[APL]) {
    u64 e[APL];
    bool live = false, left = false;
#pragma unroll
    for (int j = 0; j < APL; ++j) {
      e[j] = word(j) < A ? E[k * A + word(j)] : 0ull;
      live = live || e[j] != 0;
      e[j] = e[j] > r[j] ? e[j] : 0ull;
      left = left || e[j] != 0;
    }
    if (!__ballot(live)) return;  // no entry
    const bool keep = __ballot(left) != 0;
#pragma unroll
    for (int j = 0; j < APL; ++j)
      if (word(j) < A) E[k * A + word(j)] = e[j];
    for (unsigned long long w = 0; w < W; ++w) {
#pragma unroll
      for (int j = 0; j < APL; ++j) {
        if (word(j) >= A) continue;
        u64 *vp = V + (k * W + w) * A + word(j);
        const u64 v = *vp;
        const u64 nv = keep && v > r[j] ? v : 0ull;
        if (nv != v) *vp = nv;
      }
    }
  };
  // apply_deferred: vmap_apply_deferred (the header tells why it may be restricted to the Up's key kk)
  // with the restricted case as one bit test.  This kernel keeps its own: on the shared loop form it
  // needs 7 more VGPRs (APL 8 pass 0: 132, 3 waves per SIMD for 4) and 20-30 B more scratch at APL 1, 2.
  bool full = true;
  auto apply_deferred = [&](unsigned long long kk) {
    unsigned o = 0;
    for (unsigned d = 0; d < dcnt; ++d) {
      u64 r[APL];
      sl.row(d, r);
      if (full) {
        for (unsigned long long w = 0; w < Kw; ++w) {
          u64 bits = sl.key(d, w);
          while (bits) {
            const unsigned long long k = w * 64 + (unsigned long long)__builtin_ctzll(bits);
            bits &= bits - 1;
            if (k < K) key_rm(k, r);
          }
        }
      } else if ((sl.key(d, kk / 64) >> (kk % 64)) & 1ull) {
        key_rm(kk, r);
      }
      if (vmap_leq(r, c)) continue;  // no longer deferred
      if (o != d) sl.move(o, d);
      ++o;
    }
    dcnt = o;
    full = false;
  };
  // pass 1: the op where pass 2 continues (offset within the state's stream; < 2^32, checked on the host)
  unsigned resume_at = 0xffffffffu;
  // Op headers in batches of 64: lane i loads op o0 + i's fields (coalesced, all in flight
  // together) and op o's fields reach the wave by v_readlane, not by a global round trip per op.
  for (unsigned long long o0 = start; o0 < oe; o0 += kWave) {
    const unsigned long long mo = o0 + (unsigned long long)lane;
    const bool hin = mo < oe;
    const unsigned h_kind = hin ? p.kind[mo] : 0u;
    const unsigned h_a = hin ? p.actor[mo] : 0u, h_va = hin ? p.vactor[mo] : 0u, h_k = hin ? p.key[mo] : 0u;
    const u64 h_c = hin ? p.counter[mo] : 0ull, h_vc = hin ? p.vcounter[mo] : 0ull;
    const unsigned h_dir = hin && p.vdir ? p.vdir[mo] : 0u;
    const unsigned h_rr = hin && p.clk_row ? p.clk_row[mo] : 0xffffffffu;
    const u64 h_kb = hin ? p.key_off[mo] : 0ull, h_ke = hin ? p.key_off[mo + 1] : 0ull;
    const int nb = (int)(oe - o0 < (unsigned long long)kWave ? oe - o0 : (unsigned long long)kWave);
  for (int i = 0; i < nb; ++i) {
    const unsigned long long o = o0 + (unsigned long long)i;
    const unsigned kind = rl32(h_kind, i);
    if (kind == 0) {  // ---- Op::Up
      const unsigned a = rl32(h_a, i), va = rl32(h_va, i);
      const unsigned long long k = rl32(h_k, i);
      const u64 cnt = rl64(h_c, i), vc = rl64(h_vc, i);
      const unsigned dir = rl32(h_dir, i);
      if (a >= A || va >= A || k >= K || dir >= W) {
        st |= 2u;
        continue;
      }
      if (clock_of(a) >= cnt) continue;  // seen (map.rs:123-126)
      if ((unsigned long long)lane == a % 64) {
        u64 *ep = E + k * A + a;
        if (*ep < cnt) *ep = cnt;  // entry.clock.apply(dot)
#pragma unroll
        for (int j = 0; j < APL; ++j)
          if ((unsigned)j == a / 64 && c[j] < cnt) c[j] = cnt;  // self.clock.apply(dot)
      }
      if ((unsigned long long)lane == va % 64) {
        u64 *vp = V + (k * W + dir) * A + va;
        if (*vp < vc) *vp = vc;  // entry.val.apply(op)
      }
      apply_deferred(k);
    } else if (kind == 1) {  // ---- Op::Rm -> apply_keyset_rm
      const unsigned rr = rl32(h_rr, i);
      const u64 kb = rl64(h_kb, i), ke = rl64(h_ke, i);
      if (rr >= p.n_clk_rows || ke < kb || ke > p.n_keys) {
        st |= 2u;
        continue;
      }
      u64 r[APL];
#pragma unroll
      for (int j = 0; j < APL; ++j) r[j] = word(j) < A ? p.clk_pool[(unsigned long long)rr * A + word(j)] : 0ull;
      for (u64 i = kb; i < ke; ++i) {
        const unsigned long long k = p.keys[i];
        if (k < K) key_rm(k, r);
        else st |= 2u;
      }
      if (vmap_leq(r, c)) continue;  // every key this clock has seen, we have seen
      int slot = -1;
      for (unsigned d = 0; d < dcnt && slot < 0; ++d) {
        bool ne = false;
#pragma unroll
        for (int j = 0; j < APL; ++j) ne = ne || (word(j) < A && sl.clk(d, word(j)) != r[j]);
        if (!__ballot(ne)) slot = (int)d;
      }
      if (slot < 0) {
        if constexpr (PASS == 1) {
          if (dcnt >= Dl) {  // the list outgrows the LDS slots: pass 2 from this op
            resume_at = (unsigned)(o - ob);
            goto done;
          }
        }
        if (dcnt >= Dcap) {
          st |= 1u;  // deferred capacity exceeded: the state is incomplete
          continue;
        }
        slot = (int)dcnt++;
        if (TIER) peak = dcnt > peak ? dcnt : peak;  // (pass 1: never past the input count's slots in memory)
#pragma unroll
        for (int j = 0; j < APL; ++j)
          if (word(j) < A) sl.set_clk(slot, word(j), r[j]);
        for (unsigned long long w = (unsigned long long)lane; w < Kw; w += kWave) sl.set_key(slot, w, 0);
      }
      // deferred_set.append(keyset): one lane per key word
      for (u64 i = kb; i < ke; ++i) {
        const unsigned long long k = p.keys[i];
        if (k < K && (unsigned long long)lane == (k / 64) % kWave) sl.set_key(slot, k / 64, sl.key(slot, k / 64) | 1ull << (k % 64));
      }
    } else {
      st |= 2u;
    }
  }
  }
done:
  // the state back to memory: clock, the LDS slots, the count and status (and, at a pass-1 exit, the
  // op to continue from)
#pragma unroll
  for (int j = 0; j < APL; ++j)
    if (word(j) < A) C[word(j)] = c[j];
  sl.write_back(dcnt);
  // slots the deferred list vacated, zeroed as a fresh state's: pass 1 wrote none past its final count
  // to memory, so only the input's [dcnt, def_count[s]) can be stale there; pass 2 tracks its peak
  const unsigned hi = TIER ? peak : p.def_count[s];
  sl.zero(dcnt, hi);
  if (lane == 0) {
    p.def_count[s] = dcnt;
    p.status[s] = st;
    if (PASS == 1) p.resume[s] = resume_at == 0xffffffffu ? kVmapDone : resume_at;
  }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_map_counter_apply_batch(crdt_ctx *ctx, const crdt_map_counter_states *m, uint64_t *def_clock,
                                            uint64_t *def_keys, uint32_t *def_count, size_t Dcap,
                                            const crdt_map_counter_ops *ops, uint32_t *status) {
  CRDT_DEVICE_MEM_ONLY(ctx);
  CRDT_CHECK_CTX(ctx);
  if (!m || !ops || !status) return fail(ctx, CRDT_EINVAL, "map_counter_apply_batch: NULL argument");
  const size_t N = m->N, K = m->K, A = m->A, W = m->W;
  if (W != 1 && W != 2) return fail(ctx, CRDT_EINVAL, "map_counter_apply_batch: W = %zu (1 GCounter, 2 PNCounter)", W);
  if (N == 0) return CRDT_OK;
  if (A == 0 || A > 512) return fail(ctx, CRDT_EUNSUPPORTED, "map_counter_apply_batch: A = %zu outside 1..512", A);
  if (!m->clock || !m->ec || (K && !m->val) || !def_count || (Dcap && (!def_clock || !def_keys)) || !ops->op_off)
    return fail(ctx, CRDT_EINVAL, "map_counter_apply_batch: NULL buffer");
  if (ops->n_ops && (!ops->kind || !ops->actor || !ops->counter || !ops->key || !ops->vactor || !ops->vcounter))
    return fail(ctx, CRDT_EINVAL, "map_counter_apply_batch: NULL op buffer");
  if (m->clock_stride < A || m->ec_stride < K * A || m->val_stride < K * W * A)
    return fail(ctx, CRDT_EINVAL, "map_counter_apply_batch: strides smaller than the rows they hold");
  const size_t Kw = K ? (K + 63) / 64 : 1;
  MapCounterApplyPlan p{};
  vmap_plan_fill(p, N, K, A, Kw, Dcap, def_clock, def_keys, def_count, *ops, status);
  p.clock = (u64 *)m->clock, p.ec = (u64 *)m->ec, p.val = (u64 *)m->val;
  p.c_s = m->clock_stride, p.e_s = m->ec_stride, p.v_s = m->val_stride;
  p.W = W;
  p.vactor = ops->vactor, p.vcounter = (const u64 *)ops->vcounter, p.vdir = ops->vdir;
  return vmap_apply_run(ctx, p, 0, "map_counter_apply", [&](auto apl, auto pass, dim3 g, dim3 b, size_t l) {
    hipLaunchKernelGGL((map_counter_apply_kernel<decltype(apl)::value, decltype(pass)::value>), g, b, l, ctx->stream, p);
  });
}
