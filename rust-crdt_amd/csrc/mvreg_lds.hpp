// The MVReg working state of the deep passes (map_deep.hip, the deep fold of mvreg.hip): up to 64 value
// slots held in dynamic LDS instead of registers, for registers whose 16-value fold state overflowed
// (the reference's MVReg.vals is an unbounded Vec, mvreg.rs:32-35).
//
// One workgroup of 64..256 threads owns one register; thread t holds actors t + nt * j, j < kLdsMvApt,
// as the wide Map fold does.  Layout (u64 words): vc[VS][A] value clocks (lanes index consecutive
// actors of one slot row), val[VS], seq[VS] insertion sequence numbers, ord[VS] (slots in Vec order,
// built when the register is stored).  A thread reads and writes only its own actors' columns of vc,
// so the clock rows need no barrier; the occupancy mask `used` and `next` are uniform registers.
// val / seq are written by thread 0 and read after the barrier of store().
//
// merge() is MVReg::merge (mvreg.rs:112-128) against the V incoming values of one replica: for each
// incoming value t every thread builds two words over the state slots, bit q of le_qt[t] = "slot q
// <= t on my actors" and of le_tq[t] = "t <= slot q", and ONE wide_vote AND-reduces all 2 * V words
// (plus the OR word of the non-empty incoming slots), so a step costs the same barriers whatever the
// slot count is.  slot q < t  <=>  le_qt & !le_tq.
#pragma once

#include "block_vote.hpp"

namespace crdt {

constexpr int kLdsMvApt = 4;    // actors per thread
constexpr int kLdsMvVin = 16;   // incoming value slots per step (V)
constexpr int kLdsMvMax = 64;   // state slots: every slot mask is one u64
constexpr int kLdsMvWalk = 8;   // state slots whose rows one step of the merge's slot walk reads together
constexpr int kLdsMvRed =4 * (2 * kLdsMvVin + 1);  // vote scratch words (4 waves)

// dynamic LDS bytes of a state of VS slots over A actors
inline size_t lds_mv_bytes(size_t VS, size_t A) { return (VS * A + 3 * VS) * sizeof(u64); }

struct LdsMv {
  u64 *vc, *val, *seq, *ord;
  u64 used, next;
  unsigned VS, A;
  unsigned act[kLdsMvApt];
  bool on[kLdsMvApt];
  bool ovf;  // an append found every slot taken: the result is incomplete

  __device__ __forceinline__ void init(u64 *lds, unsigned vs, unsigned a) {
    VS = vs;
    A = a;
    vc = lds;
    val = vc + (size_t)vs * a;
    seq = val + vs;
    ord = seq + vs;
    used = next = 0;
    ovf = false;
#pragma unroll
    for (int j = 0; j < kLdsMvApt; ++j) {
      act[j] = threadIdx.x + blockDim.x * j;
      on[j] = act[j] < a;
    }
  }

  __device__ __forceinline__ int count() const { return __popcll(used); }

  // this thread's actors of a clock row in global memory
  __device__ __forceinline__ bool load_row(u64 (&x)[kLdsMvApt], const u64 *row) const {
    bool nz = false;
#pragma unroll
    for (int j = 0; j < kLdsMvApt; ++j) {
      x[j] = on[j] ? row[act[j]] : 0;
      nz |= x[j] != 0;
    }
    return nz;
  }

  // push (clock, val) at the end of the Vec: the first free slot, the next sequence number
  __device__ __forceinline__ void append(const u64 (&x)[kLdsMvApt], u64 v) {
    const u64 all = VS >= 64 ? ~0ull : ((1ull << VS) - 1);
    const u64 freem = ~used & all;
    if (freem == 0) {
      ovf = true;
      return;
    }
    const int q = __builtin_ctzll(freem);
#pragma unroll
    for (int j = 0; j < kLdsMvApt; ++j)
      if (on[j]) vc[(size_t)q * A + act[j]] = x[j];
    if (threadIdx.x == 0) {
      val[q] = v;
      seq[q] = next;
    }
    ++next;
    used |= 1ull << q;
  }

  // vals.forget(X) for every value, dropping the ones emptied (one vote round; mvreg.rs:88-104)
  __device__ __forceinline__ void forget(const u64 (&X)[kLdsMvApt], u64 *red) {
    u64 a[1] = {~0ull}, o[1] = {0};
    for (u64 m = used; m; m &= m - 1) {
      const int q = __builtin_ctzll(m);
      bool nz = false;
#pragma unroll
      for (int j = 0; j < kLdsMvApt; ++j)
        if (on[j]) {
          const u64 c = vc[(size_t)q * A + act[j]];
          const u64 n = c > X[j] ? c : 0;
          vc[(size_t)q * A + act[j]] = n;
          nz |= n != 0;
        }
      if (nz) o[0] |= 1ull << q;
    }
    wide_vote<0, 1>(a, o, red);
    used &= o[0];
  }

  // self = MVReg{ rows.forget(X) }: the V incoming values that survive forget(X), in their order
  __device__ __forceinline__ void assign_forget(const u64 *rows, const u64 *vals, unsigned long long V,
                                                const u64 (&X)[kLdsMvApt], u64 *red) {
    used = next = 0;
    u64 a[1] = {~0ull}, o[1] = {0};
    for (unsigned long long t = 0; t < V; ++t) {
      u64 x[kLdsMvApt];
      load_row(x, rows + t * A);
      bool nz = false;
#pragma unroll
      for (int j = 0; j < kLdsMvApt; ++j) nz |= x[j] > X[j];
      if (nz) o[0] |= 1ull << t;
    }
    wide_vote<0, 1>(a, o, red);
    for (unsigned long long t = 0; t < V; ++t)
      if ((o[0] >> t) & 1) {
        u64 x[kLdsMvApt];
        load_row(x, rows + t * A);
#pragma unroll
        for (int j = 0; j < kLdsMvApt; ++j) x[j] = x[j] > X[j] ? x[j] : 0;
        append(x, vals[t]);
      }
  }

  // self.merge(other) for other's V <= VIN value rows (empty rows skipped)
  template <int VIN>
  __device__ __forceinline__ void merge(const u64 *rows, const u64 *vals, unsigned long long V, u64 *red) {
    u64 a[2 * VIN], o[1] = {0};
#pragma unroll
    for (int w = 0; w < 2 * VIN; ++w) a[w] = ~0ull;
#pragma unroll
    for (int t = 0; t < VIN; ++t) {
      if ((unsigned long long)t < V) {
        u64 x[kLdsMvApt];
        if (load_row(x, rows + (size_t)t * A)) o[0] |= 1ull << t;
        u64 le_qt = ~0ull, le_tq = ~0ull;
        // the slots in groups of kLdsMvWalk: a group's LDS reads are issued together (a free slot's
        // row is read too and ignored), so the walk waits once per group, not once per slot
        for (unsigned q0 = 0; q0 < VS; q0 += kLdsMvWalk) {
          const unsigned um = (unsigned)(used >> q0) & ((1u << kLdsMvWalk) - 1u);
          if (!um) continue;
          u64 c[kLdsMvWalk][kLdsMvApt];
#pragma unroll
          for (int u = 0; u < kLdsMvWalk; ++u)
#pragma unroll
            for (int j = 0; j < kLdsMvApt; ++j)
              c[u][j] = (on[j] && q0 + u < VS) ? vc[(size_t)(q0 + u) * A + act[j]] : 0;
#pragma unroll
          for (int u = 0; u < kLdsMvWalk; ++u) {
            bool l1 = true, l2 = true;
#pragma unroll
            for (int j = 0; j < kLdsMvApt; ++j) {  // (an actor past A: c = x = 0)
              l1 &= c[u][j] <= x[j];
              l2 &= x[j] <= c[u][j];
            }
            if (((um >> u) & 1) && !l1) le_qt &= ~(1ull << (q0 + u));
            if (((um >> u) & 1) && !l2) le_tq &= ~(1ull << (q0 + u));
          }
        }
        a[t] = le_qt;
        a[VIN + t] = le_tq;
      }
    }
    wide_vote<2 * VIN, 1>(a, o, red);
    const u64 v2m = o[0];  // non-empty incoming values
    u64 keep = used;
#pragma unroll
    for (int t = 0; t < VIN; ++t)  // own < some incoming value: dropped
      if ((v2m >> t) & 1) keep &= ~(a[t] & ~a[VIN + t]);
    used = keep;
#pragma unroll
    for (int t = 0; t < VIN; ++t)  // incoming <= a KEPT own value: not added
      if (((v2m >> t) & 1) && !(a[VIN + t] & keep)) {
        u64 x[kLdsMvApt];
        load_row(x, rows + (size_t)t * A);
        append(x, vals[t]);
      }
  }

  // Load a dense register of V <= VS slots: slot s of the state is slot s of the input (Vec order =
  // slot order), an all-zero row stays a free slot.  One vote round.
  __device__ __forceinline__ void load(const u64 *rows, const u64 *vals, unsigned long long V, u64 *red) {
    u64 a[1] = {~0ull}, o[1] = {0};
    for (unsigned long long s = 0; s < V; ++s) {
      u64 x[kLdsMvApt];
      if (load_row(x, rows + s * A)) o[0] |= 1ull << s;
#pragma unroll
      for (int j = 0; j < kLdsMvApt; ++j)
        if (on[j]) vc[(size_t)s * A + act[j]] = x[j];
      if (threadIdx.x == 0) {
        val[s] = vals[s];
        seq[s] = s;
      }
    }
    wide_vote<0, 1>(a, o, red);
    used = o[0];
    next = V;
  }

  // bit q of le_qx = "slot q <= x on my actors", of le_xq = "x <= slot q", over the slots of `mask`
  // (the walk of merge(); the bits of the other slots stay set)
  __device__ __forceinline__ void cmp_slots(u64 mask, const u64 (&x)[kLdsMvApt], u64 &le_qx, u64 &le_xq) const {
    le_qx = le_xq = ~0ull;
    for (unsigned q0 = 0; q0 < VS; q0 += kLdsMvWalk) {
      const unsigned um = (unsigned)(mask >> q0) & ((1u << kLdsMvWalk) - 1u);
      if (!um) continue;
      u64 c[kLdsMvWalk][kLdsMvApt];
#pragma unroll
      for (int u = 0; u < kLdsMvWalk; ++u)
#pragma unroll
        for (int j = 0; j < kLdsMvApt; ++j)
          c[u][j] = (on[j] && q0 + u < VS) ? vc[(size_t)(q0 + u) * A + act[j]] : 0;
#pragma unroll
      for (int u = 0; u < kLdsMvWalk; ++u) {
        bool l1 = true, l2 = true;
#pragma unroll
        for (int j = 0; j < kLdsMvApt; ++j) {  // (an actor past A: c = x = 0)
          l1 &= c[u][j] <= x[j];
          l2 &= x[j] <= c[u][j];
        }
        if (((um >> u) & 1) && !l1) le_qx &= ~(1ull << (q0 + u));
        if (((um >> u) & 1) && !l2) le_xq &= ~(1ull << (q0 + u));
      }
    }
  }

  // self.merge(other) for other's V <= 64 value rows (empty rows skipped), in chunks of kLdsMvVin.
  // other's values are never compared with each other (mvreg.rs:113-126), so the chunks cannot be
  // merged one after the other: pass 1 collects, over all chunks, the own slots strictly below some
  // incoming value; pass 2 tests every incoming value against the FIXED mask of kept own slots (never
  // against a slot appended during the pass) and appends in incoming order.  One vote per chunk and pass.
  __device__ __forceinline__ void merge_any(const u64 *rows, const u64 *vals, unsigned long long V, u64 *red) {
    constexpr int VIN = kLdsMvVin;
    const u64 own = used;
    u64 drop = 0, v2m = 0;
    for (unsigned long long t0 = 0; t0 < V; t0 += VIN) {
      u64 a[2 * VIN], o[1] = {0};
#pragma unroll
      for (int w = 0; w < 2 * VIN; ++w) a[w] = ~0ull;
#pragma unroll
      for (int t = 0; t < VIN; ++t)
        if (t0 + t < V) {
          u64 x[kLdsMvApt];
          if (load_row(x, rows + (size_t)(t0 + t) * A)) o[0] |= 1ull << t;
          cmp_slots(own, x, a[t], a[VIN + t]);
        }
      wide_vote<2 * VIN, 1>(a, o, red);
#pragma unroll
      for (int t = 0; t < VIN; ++t)  // own < some incoming value: dropped
        if ((o[0] >> t) & 1) drop |= a[t] & ~a[VIN + t];
      v2m |= o[0] << t0;
    }
    const u64 keep = own & ~drop;
    used = keep;
    for (unsigned long long t0 = 0; t0 < V; t0 += VIN) {
      u64 a[VIN], o[1] = {0};
#pragma unroll
      for (int w = 0; w < VIN; ++w) a[w] = ~0ull;
#pragma unroll
      for (int t = 0; t < VIN; ++t)
        if (t0 + t < V && ((v2m >> (t0 + t)) & 1)) {
          u64 x[kLdsMvApt], le_qx;
          load_row(x, rows + (size_t)(t0 + t) * A);
          cmp_slots(keep, x, le_qx, a[t]);
        }
      wide_vote<VIN, 0>(a, o, red);
#pragma unroll
      for (int t = 0; t < VIN; ++t)  // incoming <= a KEPT own value: not added
        if (t0 + t < V && ((v2m >> (t0 + t)) & 1) && !(a[t] & keep)) {
          u64 x[kLdsMvApt];
          load_row(x, rows + (size_t)(t0 + t) * A);
          append(x, vals[t0 + t]);
        }
    }
  }

  // self.apply(Op::Put { clock: x, val: v }) (mvreg.rs:130-166): one vote gives "slot <= x" and
  // "slot >= x" over all slots.  The slots <= x go (Less or Equal); the Put is pushed unless a
  // remaining slot is >= x (then strictly greater).  An empty clock is a no-op.
  __device__ __forceinline__ void apply_put(const u64 (&x)[kLdsMvApt], u64 v, u64 *red) {
    u64 a[2], o[1] = {0};
    cmp_slots(used, x, a[0], a[1]);
#pragma unroll
    for (int j = 0; j < kLdsMvApt; ++j)
      if (x[j] != 0) o[0] = 1;
    wide_vote<2, 1>(a, o, red);
    if (!o[0]) return;  // (workgroup-uniform)
    used &= ~a[0];
    if (!(a[1] & used)) append(x, v);
  }

  // Write the register to Vout slots in Vec order (ascending sequence number, the rest zeroed).
  __device__ __forceinline__ void store(u64 *o_vclk, u64 *o_vval, unsigned long long Vout) {
    __syncthreads();  // seq (thread 0's writes) visible
    const unsigned tid = threadIdx.x;
    if (tid < VS && ((used >> tid) & 1)) {
      unsigned r = 0;
      for (u64 m = used; m; m &= m - 1) r += seq[__builtin_ctzll(m)] < seq[tid] ? 1u : 0u;
      ord[r] = tid;
    }
    __syncthreads();
    const unsigned long long n = (unsigned long long)count();
    for (unsigned long long o = 0; o < Vout; ++o) {
      const bool have = o < n;
      const size_t q = have ? (size_t)ord[o] : 0;
#pragma unroll
      for (int j = 0; j < kLdsMvApt; ++j)
        if (on[j]) o_vclk[o * A + act[j]] = have ? vc[q * A + act[j]] : 0;
      if (tid == 0) o_vval[o] = have ? val[q] : 0;
    }
  }
};

}  // namespace crdt
