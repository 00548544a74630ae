// Standalone MVReg<u64, A> registers of 17..64 value slots (the reference's MVReg.vals is an unbounded
// Vec, mvreg.rs:32-35): the shapes past the 16 register-resident slots of mvreg.hip.
//   mvreg_pair_deep_kernel   self[i].merge(other[i])            self V or other V in 17..64
//   mvreg_apply_deep_kernel  for op in ops[i]: reg[i].apply(op)  V in 17..64
//   mvreg_fold_any_kernel    G left folds of replicas with V in 17..64 slots each
// One workgroup of 64..256 threads per register, actors striped over the threads as in
// mvreg_fold_deep_kernel; the working register is an LdsMv (mvreg_lds.hpp) of self's V slots (the
// fold: Vstate slots) in dynamic LDS.  Every loop is bounded by V, the op count or the replica count,
// every barrier sits in workgroup-uniform control flow, no workgroup waits for another.
#include "mvreg_deep.hpp"
#include "mvreg_lds.hpp"

namespace crdt {

__global__ __launch_bounds__(256) void mvreg_pair_deep_kernel(MvPairPlan p) {
  extern __shared__ u64 mv_deep_lds[];
  __shared__ u64 red[kLdsMvRed];
  const unsigned long long i = blockIdx.x;
  u64 *sc = p.s_vclk + i * p.s_cs, *sv = p.s_vval + i * p.s_vs;
  LdsMv mv;
  mv.init(mv_deep_lds, (unsigned)p.Vs, (unsigned)p.A);
  mv.load(sc, sv, p.Vs, red);
  mv.merge_any(p.o_vclk + i * p.o_cs, p.o_vval + i * p.o_vs, p.Vo, red);
  mv.store(sc, sv, p.Vs);
  if (threadIdx.x == 0) p.status[i] = mv.ovf ? 16u : 0u;
}

__global__ __launch_bounds__(256) void mvreg_apply_deep_kernel(MvApplyPlan p) {
  extern __shared__ u64 mv_deep_lds[];
  __shared__ u64 red[kLdsMvRed];
  const unsigned long long i = blockIdx.x;
  const unsigned long long o0 = p.op_off[i], o1 = p.op_off[i + 1];
  if (o1 < o0 || o1 > p.n_ops) {  // invalid range: register untouched (workgroup-uniform)
    if (threadIdx.x == 0) p.status[i] = 8u;
    return;
  }
  u64 *rc = p.vclk + i * p.cs, *rv = p.vval + i * p.vs;
  LdsMv mv;
  mv.init(mv_deep_lds, (unsigned)p.V, (unsigned)p.A);
  mv.load(rc, rv, p.V, red);
  unsigned st = 0;
  for (unsigned long long o = o0; o < o1; ++o) {
    const unsigned long long row = p.clk_row[o];
    if (row >= p.n_clk_rows) {
      st |= 2u;  // malformed op: skipped
      continue;
    }
    u64 x[kLdsMvApt];
    mv.load_row(x, p.clk_pool + row * p.A);
    mv.apply_put(x, p.val[o], red);
  }
  mv.store(rc, rv, p.V);
  if (mv.ovf) st |= 16u;
  if (threadIdx.x == 0) p.status[i] = st;
}

__global__ __launch_bounds__(256) void mvreg_fold_any_kernel(MvFoldPlan p) {
  extern __shared__ u64 mv_deep_lds[];
  __shared__ u64 red[kLdsMvRed];
  const unsigned long long g = blockIdx.x;
  LdsMv mv;
  mv.init(mv_deep_lds, (unsigned)p.Vstate, (unsigned)p.A);
  for (unsigned long long r = 0; r < p.R; ++r)
    mv.merge_any(p.vclk + g * p.c_gs + r * p.c_rs, p.vval + g * p.v_gs + r * p.v_rs, p.V, red);
  mv.store(p.o_vclk + g * p.Vout * p.A, p.o_vval + g * p.Vout, p.Vout);
  if (threadIdx.x == 0) {
    const unsigned long long n = (unsigned long long)mv.count();
    if (p.o_nval) p.o_nval[g] = (uint32_t)n;
    p.o_flags[g] = (n > p.Vout ? 1u : 0u) | (mv.ovf ? 4u : 0u);
  }
}

// threads of a register's workgroup: kLdsMvApt actors per thread, whole waves, 64..256
static unsigned mv_deep_nt(size_t A) {
  return (unsigned)std::min<size_t>(256, std::max<size_t>(64, (A + 4 * 64 - 1) / (4 * 64) * 64));
}

// The LDS bound of a state of VS slots (state plus vote scratch within 160 KiB), and the opt-in past
// the default dynamic-LDS limit of 64 KiB.
static int mv_deep_prepare(crdt_ctx *ctx, const char *what, const void *fn, size_t VS, size_t A, size_t *bytes) {
  const size_t lds = lds_mv_bytes(VS, A), all = lds + kLdsMvRed * sizeof(u64);
  if (all > 160 * 1024)
    return fail(ctx, CRDT_EUNSUPPORTED, "%s: V = %zu values of A = %zu actors need %zu bytes of LDS (> 160 KiB)", what,
                VS, A, all);
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  if (all > 64 * 1024) CRDT_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  *bytes = lds;
  return CRDT_OK;
}

int mvreg_pair_deep(crdt_ctx *ctx, const MvPairPlan &p) {
  size_t lds = 0;
  if (int rc = mv_deep_prepare(ctx, "mvreg_merge_batch", reinterpret_cast<const void *>(&mvreg_pair_deep_kernel), p.Vs, p.A, &lds))
    return rc;
  timing_begin(ctx, "mvreg_pair_deep");
  hipLaunchKernelGGL(mvreg_pair_deep_kernel, dim3((unsigned)p.N), dim3(mv_deep_nt(p.A)), lds, ctx->stream, p);
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "mvreg_pair_deep_kernel launch");
  return CRDT_OK;
}

int mvreg_apply_deep(crdt_ctx *ctx, const MvApplyPlan &p) {
  size_t lds = 0;
  if (int rc = mv_deep_prepare(ctx, "mvreg_apply_batch", reinterpret_cast<const void *>(&mvreg_apply_deep_kernel), p.V, p.A, &lds))
    return rc;
  timing_begin(ctx, "mvreg_apply_deep");
  hipLaunchKernelGGL(mvreg_apply_deep_kernel, dim3((unsigned)p.N), dim3(mv_deep_nt(p.A)), lds, ctx->stream, p);
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "mvreg_apply_deep_kernel launch");
  return CRDT_OK;
}

int mvreg_fold_any(crdt_ctx *ctx, const MvFoldPlan &p) {
  size_t lds = 0;
  if (int rc = mv_deep_prepare(ctx, "mvreg_lub_many", reinterpret_cast<const void *>(&mvreg_fold_any_kernel), p.Vstate, p.A, &lds))
    return rc;
  timing_begin(ctx, "mvreg_fold_any");
  hipLaunchKernelGGL(mvreg_fold_any_kernel, dim3((unsigned)p.G), dim3(mv_deep_nt(p.A)), lds, ctx->stream, p);
  const hipError_t e = hipGetLastError();
  timing_end(ctx);
  if (e != hipSuccess) return hip_fail(ctx, e, "mvreg_fold_any_kernel launch");
  return CRDT_OK;
}

}  // namespace crdt
