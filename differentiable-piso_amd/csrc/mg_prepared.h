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
// The iteration itself (mg_pcg_run*, mg_vcycle_run*) is the one statement both kinds of entry call.
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

// ---- the iteration on a plan whose hierarchy is built (ordinary entries: by mg_build; prepared ones: by an earlier prepare) ----------------
// a regular look at the state; a prepared solve's header mismatch is reported here
static int mg_look(MgState* pinned, const MgState* st, hipStream_t stream) {
  PISO_HIP_CHECK(hipMemcpyAsync(pinned, st, sizeof(MgState), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  if (pinned->flags & MG_FLAG_NOT_PREPARED) { set_error_msg("piso_mg: not a hierarchy prepared for this grid"); return PISO_ERR_INVALID_ARG; }
  return PISO_OK;
}
static void mg_record(int nlev, int tail_first, int sweeps, int iterations, int cycles, int recomputed, int elem, int vec_mask) {
  int* d = tl_mg_dispatch;
  d[MD_LEVELS] = nlev; d[MD_TAIL_FIRST] = tail_first; d[MD_SWEEPS] = sweeps; d[MD_ITERATIONS] = iterations;
  d[MD_CYCLES] = cycles; d[MD_RESIDUAL_RECOMPUTATIONS] = recomputed; d[MD_CYCLE_ELEM] = elem; d[MD_VEC_MASK] = vec_mask;
  tl_mg_dispatch_n = MD_COUNT;
}
static void mg_record_f32(const MgRunF& R, int iterations, int cycles, int recomputed) {
  mg_record(R.P.nlev, R.use_tail ? R.P.tail_first : -1, R.nu, iterations, cycles, recomputed, 4, R.vec_mask);
}
static int mg_recomputations(int iterations, int residual_reset) {
  int recomputed = 0;
  for (int k = 1; k < iterations; ++k) recomputed += (k + 1) % residual_reset == 0;
  return recomputed;
}

static int mg_pcg_run(const MgPlan& P, const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient,
                      int residual_reset, int sweeps, int* iterations_out, hipStream_t stream, const double* x0 = nullptr) {
  MgState* pinned = nullptr;
  if (int rc = mg_pinned(&pinned)) return rc;
  const Lv& L0 = P.lv[0];
  const int n = L0.n, g0 = mg_grid(n);
  const bool use_tail = mg_use_tail(P);
  const int check_every = opt(OPT_MG_CHECK_EVERY) > 0 ? opt(OPT_MG_CHECK_EVERY) : kCheckEvery;
  double* r = P.r[0];
  mg_start(L0, divergence, x0, x_out, r, nullptr, P.scal, P.parts, P.part_max, accuracy, P.st, stream);
  bool done = false;
  int iterations = max_iterations;
  for (int k = 0; k < max_iterations && !done; ++k) {
    const bool restart = k > 0 && (k + 1) % residual_reset == 0;
    if (restart) mg_residual<<<g0, kBlock, 0, stream>>>(L0, divergence, x_out, r, P.scal, P.st);
    int n_rz = 0;
    const double* z = mg_cycle(P, r, sweeps, use_tail, &n_rz, stream);
    mg_direction<<<g0, kBlock, 0, stream>>>(L0, z, P.p[k & 1], P.p[(k + 1) & 1], P.q, P.part_rz, n_rz, P.scal, k, (restart || k == 0) ? 1 : 0, P.part_pq, P.st);
    mg_update<<<g0, kBlock, 0, stream>>>(n, x_out, r, P.p[(k + 1) & 1], P.q, P.scal, k, P.part_pq, g0, P.part_max, P.st);
    mg_check<<<1, kBlock, 0, stream>>>(P.part_max, g0, accuracy, k + 1, P.st);
    PISO_LAUNCH_CHECK();
    if ((k + 1) % check_every == 0 || k + 1 == max_iterations) {
      PISO_TRY(mg_look(pinned, P.st, stream));
      if (pinned->done) { done = true; iterations = pinned->iterations; }
    }
  }
  if (rank_deficient) {
    mg_sum_x<<<g0, kBlock, 0, stream>>>(L0, x_out, P.parts);
    mg_finish<<<g0, kBlock, 0, stream>>>(L0, x_out, P.parts, g0, P.scal);
    PISO_LAUNCH_CHECK();
  }
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  if (iterations_out) *iterations_out = iterations;
  mg_guess_record(x0, pinned);
  mg_record(P.nlev, use_tail ? P.tail_first : -1, sweeps, iterations, iterations, mg_recomputations(iterations, residual_reset), 8, 0);
  return PISO_OK;
}
static int mg_pcg_run(const MgPlanF& P, const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient,
                          int residual_reset, int sweeps, int* iterations_out, hipStream_t stream, const double* x0 = nullptr) {
  MgState* pinned = nullptr;
  if (int rc = mg_pinned(&pinned)) return rc;
  const Lv& L0 = P.L0;
  const int n = L0.n, g0 = mg_grid(n);
  MgRunF R{P, sweeps, P.tail_first >= 0 && opt(OPT_MG_TAIL) != 0, opt(OPT_MG_F32_VEC) != 0, stream};
  const int check_every = opt(OPT_MG_CHECK_EVERY) > 0 ? opt(OPT_MG_CHECK_EVERY) : kCheckEvery;
  double* r = P.r64;
  float* r32 = P.r[0];
  mg_start(L0, divergence, x0, x_out, r, r32, P.scal, P.parts, P.part_max, accuracy, P.st, stream);
  bool done = false;
  int iterations = max_iterations;
  for (int k = 0; k < max_iterations && !done; ++k) {
    const bool restart = k > 0 && (k + 1) % residual_reset == 0;
    if (restart) mg_residual_f32<<<g0, kBlock, 0, stream>>>(L0, divergence, x_out, r, P.scal, P.st, r32);
    int n_rz = 0;
    const float* z = R.cycle(r32, r, &n_rz);
    mg_direction_f32<<<g0, kBlock, 0, stream>>>(L0, z, P.p[k & 1], P.p[(k + 1) & 1], P.q, P.part_rz, n_rz, P.scal, k, (restart || k == 0) ? 1 : 0, P.part_pq, P.st);
    mg_update_f32<<<g0, kBlock, 0, stream>>>(n, x_out, r, P.p[(k + 1) & 1], P.q, P.scal, k, P.part_pq, g0, P.part_max, P.st, r32);
    mg_check<<<1, kBlock, 0, stream>>>(P.part_max, g0, accuracy, k + 1, P.st);
    PISO_LAUNCH_CHECK();
    if ((k + 1) % check_every == 0 || k + 1 == max_iterations) {
      PISO_TRY(mg_look(pinned, P.st, stream));
      if (pinned->done) { done = true; iterations = pinned->iterations; }
    }
  }
  if (rank_deficient) {
    mg_sum_x<<<g0, kBlock, 0, stream>>>(L0, x_out, P.parts);
    mg_finish<<<g0, kBlock, 0, stream>>>(L0, x_out, P.parts, g0, P.scal);
    PISO_LAUNCH_CHECK();
  }
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  if (iterations_out) *iterations_out = iterations;
  mg_guess_record(x0, pinned);
  mg_record_f32(R, iterations, iterations, mg_recomputations(iterations, residual_reset));
  return PISO_OK;
}
// one cycle; `prepared`: the call's only look at the state (the header's verdict) replaces the plain wait
static int mg_vcycle_run(const MgPlan& P, const double* r_in, double* z_out, int sweeps, bool prepared, hipStream_t stream) {
  const bool use_tail = mg_use_tail(P);
  int n_rz = 0;
  const double* z = mg_cycle(P, r_in, sweeps, use_tail, &n_rz, stream);
  PISO_LAUNCH_CHECK();
  PISO_HIP_CHECK(hipMemcpyAsync(z_out, z, (size_t)P.lv[0].n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  if (prepared) {
    MgState* pinned = nullptr;
    if (int rc = mg_pinned(&pinned)) return rc;
    PISO_TRY(mg_look(pinned, P.st, stream));
  } else {
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  mg_record(P.nlev, use_tail ? P.tail_first : -1, sweeps, 0, 1, 0, 8, 0);
  return PISO_OK;
}
static int mg_vcycle_run(const MgPlanF& P, const double* r_in, double* z_out, int sweeps, bool prepared, hipStream_t stream) {
  MgRunF R{P, sweeps, P.tail_first >= 0 && opt(OPT_MG_TAIL) != 0, opt(OPT_MG_F32_VEC) != 0, stream};
  const int n = P.L0.n;
  mg_cast_f32<<<mg_grid(n), kBlock, 0, stream>>>(n, r_in, P.r[0]);
  int n_rz = 0;
  const float* z = R.cycle(P.r[0], nullptr, &n_rz);
  mg_widen_f32<<<mg_grid(n), kBlock, 0, stream>>>(n, z, z_out);
  PISO_LAUNCH_CHECK();
  if (prepared) {
    MgState* pinned = nullptr;
    if (int rc = mg_pinned(&pinned)) return rc;
    PISO_TRY(mg_look(pinned, P.st, stream));
  } else {
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  mg_record_f32(R, 0, 1, 0);
  return PISO_OK;
}

// ---- the prepared entries, once over the type of the cycle's values ---------------------------------------------------------------------
template <typename C> struct MgPlanOf;
template <> struct MgPlanOf<double> { typedef MgPlan type; };
template <> struct MgPlanOf<float> { typedef MgPlanF type; };

// a plan over the two buffers: the levels point into the hierarchy, everything a solve writes into the scratch
static void mg_plan_over(const MgHierT<double>& H, const MgScratchT<double>& S, MgPlan& P) {
  P.nlev = H.nlev; P.tail_first = H.tail_first;
  for (int l = 0; l < H.nlev; ++l) { P.lv[l] = H.lv[l]; P.r[l] = S.r[l]; P.z[l] = S.z[l]; P.t[l] = S.t[l]; }
  P.p[0] = S.p[0]; P.p[1] = S.p[1]; P.q = S.q; P.parts = S.parts; P.part_rz = S.part_rz; P.part_pq = S.part_pq; P.part_max = S.part_max;
  P.scal = S.scal; P.st = S.st;
}
static void mg_plan_over(const MgHierT<float>& H, const MgScratchT<float>& S, MgPlanF& P) {
  P.nlev = H.nlev; P.tail_first = H.tail_first; P.L0 = H.L0;
  for (int l = 0; l < H.nlev; ++l) { P.lv[l] = H.lv[l]; P.r[l] = S.r[l]; P.z[l] = S.z[l]; P.t[l] = S.t[l]; }
  P.r64 = S.r64; P.p[0] = S.p[0]; P.p[1] = S.p[1]; P.q = S.q; P.parts = S.parts; P.part_rz = S.part_rz; P.part_pq = S.part_pq;
  P.part_max = S.part_max; P.scal = S.scal; P.st = S.st;
}
static int mg_build_any(const MgPlan& P, const double* laplace, int rank_deficient, hipStream_t s) { return mg_build(P, laplace, nullptr, rank_deficient, s); }
static int mg_build_any(const MgPlanF& P, const double* laplace, int rank_deficient, hipStream_t s) { return mg_build_f32(P, laplace, nullptr, rank_deficient, s); }

template <typename C>
static int mg_prepared_carve(const char* who, int nx, int ny, int per_x, int per_y, void* hierarchy, size_t hierarchy_bytes, void* workspace,
                             size_t workspace_bytes, MgHierT<C>& H, typename MgPlanOf<C>::type& P) {
  char msg[160];
  Arena ah(hierarchy, hierarchy_bytes), as(workspace, workspace_bytes);
  MgScratchT<C> S;
  if (!mg_hier_carve(nx, ny, per_x, per_y, ah, H)) { snprintf(msg, sizeof(msg), "%s: hierarchy buffer too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (!mg_scratch_carve(nx, ny, as, S)) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  mg_plan_over(H, S, P);
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
  MgHierT<C> H;
  typename MgPlanOf<C>::type P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_prepare", nx, ny, px, py, hierarchy, hierarchy_bytes, workspace, workspace_bytes, H, P));
  PISO_HIP_CHECK(hipMemsetAsync(H.hdr, 0, sizeof(MgHierHeader), stream));      // whatever was there stops being a hierarchy now
  P.scal = H.scal;                                                           // the set-up's sums stay with the hierarchy
  PISO_TRY(mg_build_any(P, laplace, rd, stream));
  mg_hier_seal<<<1, 1, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), rd), H.hdr);
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
  if (max_iterations < 1 || residual_reset < 1) { set_error_msg("piso_mg_pcg_solve_prepared: max_iterations and residual_reset must be positive"); return PISO_ERR_INVALID_ARG; }
  MgHierT<C> H;
  typename MgPlanOf<C>::type P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_pcg_solve_prepared", nx, ny, px, py, const_cast<void*>(hierarchy), hierarchy_bytes, workspace, workspace_bytes, H, P));
  const int g0 = mg_grid(H.L0.n);
  mg_rhs_sums<<<g0, kBlock, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), rd), H.hdr, H.L0.dinv, H.L0.n, divergence, P.parts, P.st);
  mg_rhs_fin<<<1, kBlock, 0, stream>>>(P.parts, g0, H.scal, P.scal, rd);
  PISO_LAUNCH_CHECK();
  return mg_pcg_run(P, divergence, x_out, accuracy, max_iterations, rd, residual_reset, sweeps, iterations_out, stream, x0);
}
template <typename C>
static int mg_vcycle_prepared(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes, const double* r_in, double* z_out,
                              int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int px = periodic_x ? 1 : 0, py = periodic_y ? 1 : 0;
  if (int rc = mg_common_args("piso_mg_vcycle_prepared", nx, ny, hierarchy, r_in, z_out, workspace, sweeps)) return rc;
  MgHierT<C> H;
  typename MgPlanOf<C>::type P;
  PISO_TRY(mg_prepared_carve<C>("piso_mg_vcycle_prepared", nx, ny, px, py, const_cast<void*>(hierarchy), hierarchy_bytes, workspace, workspace_bytes, H, P));
  // (no right-hand side: one workgroup checks the header and sums nothing; a cycle runs on a hierarchy prepared with either rank_deficient)
  mg_rhs_sums<<<1, kBlock, 0, stream>>>(mg_header(nx, ny, px, py, (int)sizeof(C), -1), H.hdr, H.L0.dinv, 0, nullptr, P.parts, P.st);
  PISO_LAUNCH_CHECK();
  return mg_vcycle_run(P, r_in, z_out, sweeps, true, stream);
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
