// The host protocol every wire family shares, written once: the two-pass egress (count -> scan ->
// write) of wire.hip, wire_vmap.hip, wire_mvreg.hip and the op-stream files, and the sized ingest
// (count -> J scans -> finalize -> fill) of wire_ops.hip, wire_vmap_ops.hip, wire_mvreg.hip and
// wire_lattice_ops.hip.  The families keep their plans, kernels, grids, LDS sizing and argument
// checks.  Both drivers reach timing_end on every path: no timing entry is left without its stop event.
#pragma once
#include "wire_common.hpp"

namespace crdt {

inline int wire_launched(crdt_ctx *ctx, const char *what, const char *step) {
  return hipGetLastError() == hipSuccess ? CRDT_OK : fail(ctx, CRDT_EHIP, "%s: %s launch", what, step);
}

// ---- two-pass egress ----------------------------------------------------------------------------------
// kern(p, 0) sizes every frame into p.sizes; the scan lays the frames out (frame_off, *total); with
// room (bytes && cap >= *total) set_out(p, frame_off, bytes) points the plan at them and kern(p, 1) writes.
template <class Plan, class SetOut>
int two_pass_egress(crdt_ctx *ctx, const char *what, void (*kern)(Plan, int), Plan &p, unsigned grid, uint64_t *frame_off,
                    uint8_t *bytes, size_t cap, size_t *total, SetOut &&set_out) {
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  u64 *sizes = nullptr;
  if (int rc = wire_scratch(ctx, p.N, &sizes)) return rc;
  p.sizes = sizes;
  timing_begin(ctx, what);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, ctx->stream, p, 0);
  int rc = wire_launched(ctx, what, "count");
  if (!rc) rc = egress_layout(ctx, sizes, (u64 *)frame_off, p.N, total);
  if (!rc && bytes && cap >= *total) {
    set_out(p, (const u64 *)frame_off, bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, ctx->stream, p, 1);
    rc = wire_launched(ctx, what, "write");
  }
  timing_end(ctx);
  return rc;
}

// set_out of the state plans that serve ingest and egress (MapWirePlan, VMapWirePlan, MvWirePlan): frame_off /
// bytes are their ingest's input, the egress destination is frame_out / out.
struct StatePlanOut {
  template <class Plan>
  void operator()(Plan &p, const u64 *frame_off, uint8_t *bytes) const {
    p.frame_out = frame_off;
    p.out = bytes;
  }
};

// The egress-only plans name the two fields frame_off / bytes (the op streams' and wire.hip's EgressPlan).
template <class Plan>
int two_pass_egress(crdt_ctx *ctx, const char *what, void (*kern)(Plan, int), Plan &p, unsigned grid, uint64_t *frame_off,
                    uint8_t *bytes, size_t cap, size_t *total) {
  return two_pass_egress(ctx, what, kern, p, grid, frame_off, bytes, cap, total, [](Plan &q, const u64 *fo, uint8_t *b) {
    q.frame_off = fo;
    q.bytes = b;
  });
}

// ---- sized ingest -------------------------------------------------------------------------------------
// What the finalize kernel settles for the J quantities a family counts per state (ops, rows, ids, ...).
template <int J>
struct SizedOut {
  u64 cap[J];    // the capacities
  u64 *off[J];   // [N+1] each: the states' final offsets (NULL: a quantity nobody reads back)
  u64 *zero[2];  // the list-offset arrays whose first entry is 0 (NULL: none)
  uint32_t *status;
};

// raw [J][N+1]: the scans of the counts.  The first state whose running sum of any quantity ends past
// its capacity, and every state after it, get bit 2 and no room: their offsets repeat that state's start.
template <int J>
__global__ __launch_bounds__(kBlock) void ops_finalize_kernel(const u64 *raw, unsigned long long N, SizedOut<J> o) {
  const unsigned long long i = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  if (i > N) return;
  unsigned long long c = N;
#pragma unroll
  for (int j = 0; j < J; ++j) {  // every raw[j] ascends
    const u64 *r = raw + j * (N + 1);
    unsigned long long lo = 0, hi = N;
    while (lo < hi) {
      const unsigned long long mid = (lo + hi) / 2;
      if (r[mid + 1] > o.cap[j]) hi = mid;
      else lo = mid + 1;
    }
    c = lo < c ? lo : c;
  }
  const unsigned long long at = i < c ? i : c;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (o.off[j]) o.off[j][i] = raw[j * (N + 1) + at];
  if (i < N && i >= c) o.status[i] |= kWireCap;
  if (i == 0) {
    if (o.zero[0]) o.zero[0][0] = 0;
    if (o.zero[1]) o.zero[1][0] = 0;
  }
}

// count(counts) launches the family's count kernel over counts [J][N]; the J scans follow.  With fill,
// the finalize kernel applies o and fill_launch() (which first points its plan at o.off) launches the
// family's fill kernel.  totals non-NULL: the J sums of the well-formed frames are read back (synchronises).
template <int J, class Count, class Fill>
int sized_ingest(crdt_ctx *ctx, const char *what, unsigned long long N, const SizedOut<J> &o, bool fill, uint64_t *totals,
                 Count &&count, Fill &&fill_launch) {
  CRDT_HIP(ctx, hipSetDevice(ctx->device));
  // scratch: counts [J][N] | raw offsets [J][N+1] | scan scratch
  const unsigned long long nb = (N + kScanItems - 1) / kScanItems + 2;
  if (int rc = ensure_scratch(ctx, (J * N + J * (N + 1) + nb + 8) * 8)) return rc;
  u64 *counts = reinterpret_cast<u64 *>(ctx->scratch), *raw = counts + J * N, *sc = raw + J * (N + 1);
  timing_begin(ctx, what);
  count(counts);
  int rc = wire_launched(ctx, what, "count");
  for (int j = 0; j < J && !rc; ++j) rc = exclusive_scan(ctx, counts + j * N, raw + j * (N + 1), N, sc, nullptr);
  if (!rc && fill) {
    hipLaunchKernelGGL(ops_finalize_kernel<J>, dim3((unsigned)((N + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const u64 *)raw, N, o);
    rc = wire_launched(ctx, what, "finalize");
    if (!rc) {
      fill_launch();
      rc = wire_launched(ctx, what, "fill");
    }
  }
  timing_end(ctx);
  if (rc) return rc;
  if (totals) {
    u64 t[J] = {};
    for (int j = 0; j < J; ++j)
      CRDT_HIP(ctx, hipMemcpyAsync(&t[j], raw + j * (N + 1) + N, 8, hipMemcpyDeviceToHost, ctx->stream));
    CRDT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < J; ++j) totals[j] = t[j];
  }
  return CRDT_OK;
}

}  // namespace crdt
