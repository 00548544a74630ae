// The deep pass of crdt_map_lub_many (17 <= out->Vstate <= 64): the keys whose fold state overflowed the
// first pass's 16 value slots are folded again, exactly and in replica order, with the MVReg state in
// LDS (mvreg_lds.hpp) and up to Vstate values (the reference's MVReg.vals is an unbounded Vec,
// mvreg.rs:32-35; a key written concurrently by 17+ actors is a plain valid input).
//
// The first pass (map_fold_kernel / map_fold_wide_kernel) writes nval = kMapDeepMark for a (group, key)
// whose state overflowed instead of reporting flags bit 2; this kernel runs one workgroup per
// (group, key) and every unmarked workgroup exits at once.  A marked one runs the step of
// map_fold_wide_kernel (map_wide.hip: the entry join of map.rs:142-210 in one vote round,
// MVReg::merge / forget, the live deferred-remove queue with the walk of the group's list past the
// LDS window), 64..256 threads with actors striped over threads, the entry and acc clocks in
// registers and the value state in dynamic LDS.  It rewrites the key's ec, value slots (Vec order),
// vval and nval; out->clock is the first pass's (it does not depend on the value state).  Into
// flags[g] it ORs bit 0 (more than Vout values at the end) and bit 2 (more than Vstate values at some
// step); a malformed remove list (bit 1) was already reported by the first pass.
//
// Every loop is bounded by R, V, Vstate or the remove list; no workgroup waits for another.
#include <algorithm>

#include "common.hpp"
#include "mvreg_lds.hpp"

namespace crdt {

constexpr int kDeepApt = kLdsMvApt;  // actors per thread
constexpr int kDeepList = 1024;      // removes naming one key listed in LDS (beyond: the group list)
constexpr int kDeepLive = 1024;      // live removes tracked in LDS (beyond: a rescan of the started ones)

struct MapDeepPlan {
  const u64 *clock;
  long long c_rs, c_gs;
  const u64 *ec;
  long long e_rs, e_gs;
  const u64 *vclk;
  long long vc_rs, vc_gs;
  const u64 *vval;
  long long vv_rs, vv_gs;
  const size_t *def_off;  // device copy [G+1] (nullptr: no deferred)
  const unsigned *def_row;
  const u64 *def_clock;
  const u64 *def_keys;
  unsigned long long G, R, K, A, V, Kw, Vout, Vstate;
  u64 *o_ec, *o_vclk, *o_vval;
  unsigned *o_flags, *o_nval;  // o_nval [G*K]: kMapDeepMark where the first pass left the key to this one
};

// VIN: the incoming value slots a step's vote round is unrolled for (V <= VIN)
template <int VIN>
__global__ __launch_bounds__(256) void map_fold_deep_kernel(MapDeepPlan p) {
  extern __shared__ u64 deep_lds[];
  __shared__ u64 red[kLdsMvRed];
  __shared__ unsigned lrow[kDeepList], lidx[kDeepList], live[kDeepLive];
  __shared__ unsigned s_cnt[1];
  if (p.o_nval[blockIdx.x] != kMapDeepMark) return;  // (uniform: the whole workgroup leaves)
  const unsigned long long g = blockIdx.x / p.K, k = blockIdx.x % p.K;
  const unsigned tid = threadIdx.x;
  const unsigned long long A = p.A, R = p.R, V = p.V;
  LdsMv mv;
  mv.init(deep_lds, (unsigned)p.Vstate, (unsigned)A);
  bool on[kDeepApt];
  unsigned long long act[kDeepApt];
#pragma unroll
  for (int j = 0; j < kDeepApt; ++j) {
    act[j] = mv.act[j];
    on[j] = mv.on[j];
  }
  bool present = false;
  u64 e[kDeepApt], cs[kDeepApt];
#pragma unroll
  for (int j = 0; j < kDeepApt; ++j) e[j] = cs[j] = 0;

  // the removes naming this key, in replica order (wave 0 gathers them; ballot prefix positions)
  unsigned long long dbeg = 0, dend = 0;
  if (p.def_off) {
    dbeg = p.def_off[g];
    dend = p.def_off[g + 1];
  }
  const unsigned long long kw = k / 64;
  const u64 kbit = 1ull << (k % 64);
  if (tid < 64) {
    unsigned long long nl = 0;
    for (unsigned long long base = dbeg; base < dend; base += 64) {
      const unsigned long long d = base + tid;
      bool hit = false;
      unsigned row = 0;
      if (d < dend) {
        row = p.def_row[d];
        hit = (p.def_keys[d * p.Kw + kw] & kbit) != 0;
      }
      const u64 m = __ballot(hit);
      if (hit) {
        const unsigned long long pos = nl + __popcll(m & ((1ull << tid) - 1));
        if (pos < kDeepList) {
          lrow[pos] = row;
          lidx[pos] = (unsigned)d;
        }
      }
      nl += __popcll(m);
    }
    if (tid == 0) s_cnt[0] = (unsigned)(nl > 0xffffffffull ? 0xffffffffu : nl);
  }
  __syncthreads();
  const unsigned long long nl = s_cnt[0];
  const bool direct = nl > (unsigned long long)kDeepList;  // walk the group's list each step
  unsigned long long lp = 0, dp = dbeg, nlive = 0;
  bool rescan = false;  // more live removes than kDeepLive: rescan the started ones every step

  // a step's entry clock and replica clock are loaded one step ahead (the step itself is a chain of
  // dependent votes: its own loads would add their latency to every one of the R steps)
  u64 nie[kDeepApt], nico[kDeepApt];
  auto fetch = [&](unsigned long long i) {
    const u64 *ecp = p.ec + g * p.e_gs + i * p.e_rs + k * A;
    const u64 *cop = p.clock + g * p.c_gs + i * p.c_rs;
#pragma unroll
    for (int j = 0; j < kDeepApt; ++j) {
      nie[j] = on[j] ? ecp[act[j]] : 0;
      nico[j] = on[j] ? cop[act[j]] : 0;
    }
  };
  if (R > 0) fetch(0);
  for (unsigned long long i = 0; i < R; ++i) {
    const u64 *vcp = p.vclk + g * p.vc_gs + i * p.vc_rs + k * V * A;
    const u64 *vvp = p.vval + g * p.vv_gs + i * p.vv_rs + k * V;
    u64 ie[kDeepApt], ico[kDeepApt];
#pragma unroll
    for (int j = 0; j < kDeepApt; ++j) {
      ie[j] = nie[j];
      ico[j] = nico[j];
    }
    if (i + 1 < R) fetch(i + 1);
    // ---- 1. entry join (map.rs:142-210): every test of the three cases in one round ----
    u64 eA[kDeepApt], riA[kDeepApt], eB[kDeepApt], riB[kDeepApt], common[kDeepApt], dl[kDeepApt];
    bool t_co_ge_e = true, t_cs_ge_ie = true, t_eq = true, n_ie = false, n_common = false, n_dl = false, n_riA = false;
#pragma unroll
    for (int j = 0; j < kDeepApt; ++j) {
      t_co_ge_e &= ico[j] >= e[j];
      t_cs_ge_ie &= cs[j] >= ie[j];
      t_eq &= e[j] == ie[j];
      n_ie |= ie[j] != 0;
      eA[j] = e[j] > ico[j] ? e[j] : 0;
      riA[j] = ico[j] > eA[j] ? ico[j] : 0;
      n_riA |= riA[j] != 0;
      eB[j] = ie[j] > cs[j] ? ie[j] : 0;
      riB[j] = cs[j] > eB[j] ? cs[j] : 0;
      const u64 t0 = e[j] == ie[j] ? e[j] : 0;
      const u64 t1 = ie[j] > cs[j] ? ie[j] : 0;
      const u64 t2 = e[j] > ico[j] ? e[j] : 0;
      const u64 c = t0 > t1 ? t0 : t1;
      common[j] = c > t2 ? c : t2;
      const u64 m = e[j] > ie[j] ? e[j] : ie[j];
      dl[j] = m > common[j] ? m : 0;
      n_common |= common[j] != 0;
      n_dl |= dl[j] != 0;
    }
    {
      u64 a[1] = {(t_co_ge_e ? 1ull : 0) | (t_cs_ge_ie ? 2ull : 0) | (t_eq ? 4ull : 0)};
      u64 o[1] = {(n_ie ? 1ull : 0) | (n_common ? 2ull : 0) | (n_dl ? 4ull : 0) | (n_riA ? 8ull : 0)};
      wide_vote<1, 1>(a, o, red);
      t_co_ge_e = a[0] & 1;
      t_cs_ge_ie = a[0] & 2;
      t_eq = a[0] & 4;
      n_ie = o[0] & 1;
      n_common = o[0] & 2;
      n_dl = o[0] & 4;
      n_riA = o[0] & 8;
    }
    const bool p2 = n_ie;
    if (present && !p2) {
      if (t_co_ge_e) {
        present = false;
        mv.used = 0;
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) e[j] = 0;
      } else {
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) e[j] = eA[j];
        if (n_riA) mv.forget(riA, red);
      }
    } else if (!present && p2) {
      if (!t_cs_ge_ie) {
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) e[j] = eB[j];
        mv.assign_forget(vcp, vvp, V, riB, red);
        present = true;
      }
    } else if (present && p2) {
      bool dl_any = false;
      if (!t_eq) {
        if (!n_common) {
          present = false;
          mv.used = 0;
        } else {
          dl_any = n_dl;
        }
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) e[j] = common[j];
      }
      if (present) {
        mv.template merge<VIN>(vcp, vvp, V, red);
        if (dl_any) mv.forget(dl, red);
      }
    }

    // ---- 2. deferred removes active at step i (map.rs:213-219, :311-348) ----
    bool activating;
    if (direct) {
      activating = dp < dend && p.def_row[dp] <= i;
    } else {
      activating = lp < nl && lrow[lp] <= i;
    }
    if (activating || nlive > 0 || rescan) {
      u64 ceil[kDeepApt];
#pragma unroll
      for (int j = 0; j < kDeepApt; ++j) ceil[j] = 0;
      bool have = false;
      auto fold_in = [&](unsigned long long d) {
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) {
          const u64 x = on[j] ? p.def_clock[d * A + act[j]] : 0;
          ceil[j] = ceil[j] > x ? ceil[j] : x;
        }
        have = true;
      };
      if (!rescan) {
        // expire: a live remove the acc clock (before step i) dominates is dead for good
        unsigned long long w = 0;
        for (unsigned long long base = 0; base < nlive; base += 64) {
          const unsigned long long nb = nlive - base < 64 ? nlive - base : 64;
          u64 a[1] = {~0ull}, o[1] = {0};
          for (unsigned long long x = 0; x < nb; ++x) {
            const unsigned long long d = live[base + x];
            bool ge = true;
#pragma unroll
            for (int j = 0; j < kDeepApt; ++j) ge &= !on[j] || cs[j] >= p.def_clock[d * A + act[j]];
            if (!ge) a[0] &= ~(1ull << x);
          }
          wide_vote<1, 0>(a, o, red);  // bit x: dominated everywhere
          __syncthreads();             // every thread has read live[] of this batch
          if (tid == 0) {              // compaction: entry w <= base + x, never an unread one
            unsigned long long ww = w;
            for (unsigned long long x = 0; x < nb; ++x)
              if (!((a[0] >> x) & 1)) live[ww++] = live[base + x];
          }
          w += nb - __popcll(a[0] & (nb == 64 ? ~0ull : ((1ull << nb) - 1)));
          __syncthreads();
        }
        nlive = w;
      }
      // activate the removes held by replica i that name this key
      while (true) {
        unsigned long long d;
        if (!direct) {
          if (lp >= nl || lrow[lp] > i) break;
          d = lidx[lp++];
        } else {
          if (dp >= dend || p.def_row[dp] > i) break;
          d = dp++;
          if (!(p.def_keys[d * p.Kw + kw] & kbit)) continue;
        }
        if (!rescan && nlive < (unsigned long long)kDeepLive) {
          if (tid == 0) live[nlive] = (unsigned)d;
          ++nlive;
        } else {
          rescan = true;
        }
      }
      __syncthreads();  // the activated entries are visible to every thread
      if (!rescan) {
        for (unsigned long long x = 0; x < nlive; ++x) fold_in(live[x]);
      } else {  // every started remove: live iff held by replica i or not dominated by the acc clock
        const unsigned long long nscan = direct ? dp - dbeg : lp;
        for (unsigned long long x = 0; x < nscan; ++x) {
          const unsigned long long d = direct ? dbeg + x : lidx[x];
          if (direct && !(p.def_keys[d * p.Kw + kw] & kbit)) continue;
          bool ge = true;
#pragma unroll
          for (int j = 0; j < kDeepApt; ++j) ge &= !on[j] || cs[j] >= p.def_clock[d * A + act[j]];
          if (p.def_row[d] == i || !wide_all(ge, red)) fold_in(d);
        }
      }
      if (have && present) {
        bool nz = false;
#pragma unroll
        for (int j = 0; j < kDeepApt; ++j) {
          e[j] = e[j] > ceil[j] ? e[j] : 0;
          nz |= e[j] != 0;
        }
        if (!wide_any(nz, red)) {
          present = false;
          mv.used = 0;
        } else {
          mv.forget(ceil, red);
        }
      }
    }
    // ---- 3. acc.clock.merge(other.clock) (map.rs:217) ----
#pragma unroll
    for (int j = 0; j < kDeepApt; ++j) cs[j] = cs[j] > ico[j] ? cs[j] : ico[j];
  }

  // ---- egress: the key's entry clock and its value slots in Vec order ----
  const unsigned long long gk = g * p.K + k;
#pragma unroll
  for (int j = 0; j < kDeepApt; ++j)
    if (on[j]) p.o_ec[gk * A + act[j]] = present ? e[j] : 0;
  mv.store(p.o_vclk + gk * p.Vout * A, p.o_vval + gk * p.Vout, p.Vout);
  if (tid == 0) {
    const int nv = mv.count();
    p.o_nval[gk] = present ? (unsigned)nv : 0u;
    const unsigned f = ((unsigned long long)nv > p.Vout ? 1u : 0u) | (mv.ovf ? 4u : 0u);
    if (f) atomicOr(p.o_flags + g, f);
  }
}

// the kernel's __shared__ arrays (with the alignment padding between them)
static constexpr size_t kDeepStatic =
    (kLdsMvRed * sizeof(u64) + (2 * kDeepList + kDeepLive + 1) * sizeof(unsigned) + 15) / 16 * 16;

size_t map_deep_lds(size_t Vstate, size_t A) { return lds_mv_bytes(Vstate, A) + kDeepStatic; }

int map_lub_deep(crdt_ctx *ctx, const crdt_map_batch *in, const size_t *def_off_dev, crdt_map_out *out) {
  const size_t A = in->A, V = in->V;
  MapDeepPlan p{};
  p.clock = (const u64 *)in->clock;
  p.c_rs = in->clock_rstride;
  p.c_gs = in->clock_gstride;
  p.ec = (const u64 *)in->ec;
  p.e_rs = in->ec_rstride;
  p.e_gs = in->ec_gstride;
  p.vclk = (const u64 *)in->vclk;
  p.vc_rs = in->vclk_rstride;
  p.vc_gs = in->vclk_gstride;
  p.vval = (const u64 *)in->vval;
  p.vv_rs = in->vval_rstride;
  p.vv_gs = in->vval_gstride;
  p.def_off = def_off_dev;
  p.def_row = in->def_row;
  p.def_clock = (const u64 *)in->def_clock;
  p.def_keys = (const u64 *)in->def_keys;
  p.G = in->G;
  p.R = in->R;
  p.K = in->K;
  p.A = A;
  p.V = V;
  p.Kw = (in->K + 63) / 64;
  p.Vout = out->Vout;
  p.Vstate = out->Vstate;
  p.o_ec = (u64 *)out->ec;
  p.o_vclk = (u64 *)out->vclk;
  p.o_vval = (u64 *)out->vval;
  p.o_nval = out->nval;
  p.o_flags = out->flags;
  const size_t lds = lds_mv_bytes(out->Vstate, A);
  const unsigned nt = (unsigned)std::min<size_t>(256, std::max<size_t>(64, (A + 4 * 64 - 1) / (4 * 64) * 64));
  const void *fn = V <= 2 ? reinterpret_cast<const void *>(&map_fold_deep_kernel<2>)
                          : reinterpret_cast<const void *>(&map_fold_deep_kernel<kLdsMvVin>);
  if (lds + kDeepStatic > 64 * 1024)  // beyond the default dynamic-LDS limit (gfx950 has 160 KB per CU)
    CRDT_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)(in->G * in->K)), blk(nt);
  timing_begin(ctx, "map_fold_deep");
  if (V <= 2) hipLaunchKernelGGL(map_fold_deep_kernel<2>, grid, blk, lds, ctx->stream, p);
  else hipLaunchKernelGGL(map_fold_deep_kernel<kLdsMvVin>, grid, blk, lds, ctx->stream, p);
  timing_end(ctx);
  CRDT_HIP(ctx, hipGetLastError());
  return CRDT_OK;
}

}  // namespace crdt
