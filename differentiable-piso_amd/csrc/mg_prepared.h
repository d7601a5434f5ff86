// A PREPARED hierarchy: set-up separated from solve (piso_mg_prepare_*, piso_mg_pcg_solve_prepared_*, piso_mg_vcycle_prepared_*).
// prepare runs the set-up kernels of mg.hip / mg_f32.h into a buffer the caller owns (mg_prepared_carve.h: everything that depends on the
// matrix only), makes the one host look with its three refusals, and seals the buffer with a header - written LAST, so a refused or failed
// prepare leaves none.  A solve on the buffer launches the kernels of the ordinary solve over level structs that point into it; what the
// ordinary set-up does per right-hand side is left to two small kernels:
//   mg_rhs_sums   the partials of sum(b) over the present cells, with the grid, the walk and the block sum of mg_setup0's third partial;
//                 its first thread compares the header with the call's arguments and resets MgState - on a mismatch to `done` with
//                 MG_FLAG_NOT_PREPARED, so every later kernel returns at once and the host reports it at its first regular look
//   mg_rhs_fin    one workgroup: re-adds the partials in index order and writes SC_MEAN_B by mg_setup_fin's rule, beside the hierarchy's
//                 SC_SUM_DIAG / SC_NPRESENT, and zeroes SC_RZ0 / SC_RZ1
// so x, the iteration count and the dispatch record are those of the ordinary solve bit for bit, and no host look precedes iteration 1.
// The iteration itself (MgGridT<C>::pcg / ::vcycle of mg_grid.h) is the one statement both kinds of entry call, on the same MgPlanT<C>.
#pragma once

#include "mg_prepared_carve.h"

namespace piso {

static_assert(sizeof(MgHierHeader) == 32, "MgHierHeader is eight words");

__global__ __launch_bounds__(kBlock) void mg_rhs_sums(MgHierHeader want, const MgHierHeader* hdr, const double* __restrict__ dinv, int n,
                                                      const double* __restrict__ b, double* parts, MgState* st) {
  __shared__ double smem[16];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const MgHierHeader h = *hdr;
    const bool ok = h.magic == want.magic && h.nx == want.nx && h.ny == want.ny && h.per_x == want.per_x && h.per_y == want.per_y &&
                    h.cycle_elem == want.cycle_elem && (want.rank_deficient < 0 || h.rank_deficient == want.rank_deficient);
    st->done = ok ? 0 : 1; st->iterations = 0; st->flags = ok ? 0 : MG_FLAG_NOT_PREPARED; st->pad = 0;
  }
  double sb = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step)
    if (dinv[c] != 0) sb += b[c];
  sb = mg_block_sum(sb, smem);
  if (threadIdx.x == 0) parts[2 * kMgGrid + blockIdx.x] = sb;
}
__global__ __launch_bounds__(kBlock) void mg_rhs_fin(const double* parts, int count, const double* hier_scal, double* scal, int rank_deficient) {
  __shared__ double smem[16];
  const double sb = mg_sum_partials(parts + 2 * kMgGrid, count, smem);
  if (threadIdx.x == 0) {
    const double sd = hier_scal[SC_SUM_DIAG], np = hier_scal[SC_NPRESENT];
    scal[SC_SUM_DIAG] = sd; scal[SC_NPRESENT] = np;
    scal[SC_MEAN_B] = (rank_deficient && np > 0) ? sb / np : 0.0;
    scal[SC_RZ0] = 0; scal[SC_RZ1] = 0;
  }
}
__global__ void mg_hier_seal(MgHierHeader h, MgHierHeader* hdr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *hdr = h;
}

// ---- the prepared entries, once over the type of the cycle's values ---------------------------------------------------------------------
// a plan over the two buffers: the levels point into the hierarchy, everything a solve writes into the scratch
template <typename C>
static int mg_prepared_carve(const char* who, int nx, int ny, int per_x, int per_y, void* hierarchy, size_t hierarchy_bytes, void* workspace,
                             size_t workspace_bytes, MgPlanT<C>& P) {
  char msg[160];
  Arena ah(hierarchy, hierarchy_bytes), as(workspace, workspace_bytes);
  if (!mg_hier_carve(nx, ny, per_x, per_y, ah, P.H)) { snprintf(msg, sizeof(msg), "%s: hierarchy buffer too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (!mg_scratch_carve(nx, ny, as, P.S)) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  return PISO_OK;
}
static MgHierHeader mg_header(int nx, int ny, int per_x, int per_y, int elem, int rank_deficient) {
  return MgHierHeader{kMgHierMagic, nx, ny, per_x, per_y, elem, rank_deficient, 0};
}

template <typename C>
static int mg_prepare(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int rank_deficient, void* hierarchy, size_t hierarchy_bytes,
                      void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int px = periodic_x ? 1 : 0, py = periodic_y ? 1 : 0, rd = rank_deficient ? 1 : 0;
  if (int rc = mg_common_args("piso_mg_prepare", nx, ny, laplace, hierarchy, workspace, workspace, 1)) return rc;
  MgPlanT<C> P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_prepare", nx, ny, px, py, hierarchy, hierarchy_bytes, workspace, workspace_bytes, P));
  PISO_HIP_CHECK(hipMemsetAsync(P.H.hdr, 0, sizeof(MgHierHeader), stream));    // whatever was there stops being a hierarchy now
  PISO_TRY(MgGridT<C>(P, 1, stream).build(laplace, nullptr, rd));              // (the set-up's sums stay with the hierarchy: H.scal)
  mg_hier_seal<<<1, 1, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), rd), P.H.hdr);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
template <typename C>
static int mg_solve_prepared(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes, const double* divergence,
                             double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps, int* iterations_out,
                             void* workspace, size_t workspace_bytes, piso_stream_t stream_, const double* x0) {
  const OptScope knobs;
  tl_mg_last_guess = 0;                                       // (until the solve returns: a refused call reports no guess)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int px = periodic_x ? 1 : 0, py = periodic_y ? 1 : 0, rd = rank_deficient ? 1 : 0;
  if (int rc = mg_common_args("piso_mg_pcg_solve_prepared", nx, ny, hierarchy, divergence, x_out, workspace, sweeps)) return rc;
  PISO_TRY(mg_iteration_args("piso_mg_pcg_solve_prepared", max_iterations, residual_reset));
  MgPlanT<C> P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_pcg_solve_prepared", nx, ny, px, py, const_cast<void*>(hierarchy), hierarchy_bytes, workspace, workspace_bytes, P));
  const MgHierT<C>& H = P.H;
  const int g0 = mg_grid(H.L0.n);
  mg_rhs_sums<<<g0, kBlock, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), rd), H.hdr, H.L0.dinv, H.L0.n, divergence, P.S.parts, P.S.st);
  mg_rhs_fin<<<1, kBlock, 0, stream>>>(P.S.parts, g0, H.scal, P.S.scal, rd);
  PISO_LAUNCH_CHECK();
  return MgGridT<C>(P, sweeps, stream).pcg(divergence, x_out, accuracy, max_iterations, rd, residual_reset, iterations_out, x0);
}
template <typename C>
static int mg_vcycle_prepared(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes, const double* r_in, double* z_out,
                              int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int px = periodic_x ? 1 : 0, py = periodic_y ? 1 : 0;
  if (int rc = mg_common_args("piso_mg_vcycle_prepared", nx, ny, hierarchy, r_in, z_out, workspace, sweeps)) return rc;
  MgPlanT<C> P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_vcycle_prepared", nx, ny, px, py, const_cast<void*>(hierarchy), hierarchy_bytes, workspace, workspace_bytes, P));
  // (no right-hand side: one workgroup checks the header and sums nothing; a cycle runs on a hierarchy prepared with either rank_deficient)
  mg_rhs_sums<<<1, kBlock, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), -1), P.H.hdr, P.H.L0.dinv, 0, nullptr, P.S.parts, P.S.st);
  PISO_LAUNCH_CHECK();
  return MgGridT<C>(P, sweeps, stream).vcycle(r_in, z_out, true);
}

}  // namespace piso

extern "C" {

size_t piso_mg_hierarchy_bytes(int nx, int ny, int cycle_elem_size) { return piso::mg_hier_bytes(nx, ny, cycle_elem_size); }
size_t piso_mg_solve_workspace_bytes(int nx, int ny, int cycle_elem_size) { return piso::mg_scratch_bytes(nx, ny, cycle_elem_size); }

#define PISO_MG_PREPARED_ENTRIES(SUFFIX, C)                                                                                                                      \
  int piso_mg_prepare##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int rank_deficient, void* hierarchy,                        \
                              size_t hierarchy_bytes, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                           \
    return piso::mg_prepare<C>(nx, ny, periodic_x, periodic_y, laplace, rank_deficient, hierarchy, hierarchy_bytes, workspace, workspace_bytes, stream);         \
  }                                                                                                                                                              \
  int piso_mg_pcg_solve_prepared##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,                          \
                                         const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,    \
                                         int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                       \
    return piso::mg_solve_prepared<C>(nx, ny, periodic_x, periodic_y, hierarchy, hierarchy_bytes, divergence, x_out, accuracy, max_iterations, rank_deficient,   \
                                      residual_reset, sweeps, iterations_out, workspace, workspace_bytes, stream, nullptr);                                      \
  }                                                                                                                                                              \
  int piso_mg_pcg_solve_prepared_guess##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,                    \
                                               const double* divergence, const double* x0, double* x_out, float accuracy, int max_iterations,                    \
                                               int rank_deficient, int residual_reset, int sweeps, int* iterations_out, void* workspace,                         \
                                               size_t workspace_bytes, piso_stream_t stream) {                                                                   \
    return piso::mg_solve_prepared<C>(nx, ny, periodic_x, periodic_y, hierarchy, hierarchy_bytes, divergence, x_out, accuracy, max_iterations, rank_deficient,   \
                                      residual_reset, sweeps, iterations_out, workspace, workspace_bytes, stream, x0);                                           \
  }                                                                                                                                                              \
  int piso_mg_vcycle_prepared##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes, const double* r_in,         \
                                      double* z_out, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                \
    return piso::mg_vcycle_prepared<C>(nx, ny, periodic_x, periodic_y, hierarchy, hierarchy_bytes, r_in, z_out, sweeps, workspace, workspace_bytes, stream);     \
  }
PISO_MG_PREPARED_ENTRIES(_f64, double)
PISO_MG_PREPARED_ENTRIES(_c32_f64, float)
#undef PISO_MG_PREPARED_ENTRIES

}  // extern "C"
