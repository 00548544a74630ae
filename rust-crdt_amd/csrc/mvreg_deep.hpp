// Launch plans of the standalone MVReg kernels (mvreg.hip) and the entry points' way into the
// LDS-register kernels of mvreg_deep.hip (registers of 17..64 value slots).
#pragma once

#include "common.hpp"

namespace crdt {

struct MvFoldPlan {
  const u64 *vclk, *vval;
  unsigned long long G, R, A, V;
  unsigned long long c_rs, c_gs, v_rs, v_gs;
  u64 *o_vclk, *o_vval;
  unsigned long long Vout;
  uint32_t *o_nval, *o_flags;
  uint8_t *mark;  // (nullable) per group: the state overflowed, left to the deep pass
  unsigned long long Vstate;  // the deep pass's slots
};

struct MvPairPlan {
  u64 *s_vclk, *s_vval;
  unsigned long long s_cs, s_vs, Vs;
  const u64 *o_vclk, *o_vval;
  unsigned long long o_cs, o_vs, Vo;
  unsigned long long N, A;
  uint32_t *status;
};

struct MvApplyPlan {
  u64 *vclk, *vval;
  unsigned long long cs, vs, V, N, A;
  const u64 *op_off;
  const uint32_t *clk_row;
  const u64 *clk_pool, *val;
  unsigned long long n_ops, n_clk_rows;
  uint32_t *status;
};

// mvreg_deep.hip: one workgroup per register, the register in dynamic LDS.  Each checks the LDS bound
// (CRDT_EUNSUPPORTED before any launch) and launches on ctx->stream.
int mvreg_fold_any(crdt_ctx *ctx, const MvFoldPlan &p);    // input V in 17..64, state p.Vstate slots
int mvreg_pair_deep(crdt_ctx *ctx, const MvPairPlan &p);   // Vs or Vo in 17..64
int mvreg_apply_deep(crdt_ctx *ctx, const MvApplyPlan &p); // V in 17..64

}  // namespace crdt
