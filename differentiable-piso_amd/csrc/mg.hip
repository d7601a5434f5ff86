// Multigrid-preconditioned CG for the pressure system (fp64): an OPT-IN second pressure solver next to the plain CG of cg.hip.
// The reference has no such solver; it solves the same system, (L + c 1 1^T) x = b, to the same stopping rule (max|r| < accuracy on
// the recurred residual) in tens of iterations where plain CG needs thousands.  tests/mg_reference.py is the numpy twin.
//
// Matrix.  L [N][5] = (-y, -x, diag, +x, +y), diagonal <= 0, symmetric, periodic wrap per axis.  A cell with a ZERO diagonal is ABSENT
// (solid cells, padding): x = 0 there, it joins no aggregate, couplings into it are dropped.  A non-zero border entry in a
// non-periodic direction (which makes the reference stencil read the neighbouring row) is refused, and so is a zero-diagonal row that
// still has entries, and rank_deficient = 1 on a matrix whose rows do not sum to zero: PISO_ERR_UNSUPPORTED_PATTERN, never another system.
// PRECONDITION, not checked: the present cells are CONNECTED.  A pocket of fluid enclosed by solid cells is a second null vector of L
// (rank deficient) or a singular block (open borders); the iteration then does not converge - it runs to max_iterations with a finite x,
// never reports fewer - and neither does the plain CG.  Detecting it on the device is not attempted.
//
// Hierarchy.  2 x 2 aggregation (ceil), piecewise-constant P, A_c = kGalerkin P^T A P built on the device level by level, every level
// in the same five-array layout (couplings across an aggregate face are summed into the coarse off-diagonal, couplings inside go to the
// diagonal, from both sides).  Coarsening stops before a dimension would fall below kMinDim.
//
// Cycle.  V(nu, nu), damped Jacobi (kOmega) from a zero guess; the coarsest level gets kCoarsestSweeps sweeps.  A fixed, symmetric
// linear operator M^-1 ~ L^-1 (negative definite on the present cells), so plain PCG and "the adjoint is the same solve" hold.
// Passes over a level per cycle at nu = 2: [sweep 1 + sweep 2] (the first sweep from zero is pointwise, so both come out of one
// stencil pass over r), [residual + restriction], [prolongation + correction + post-sweep 1], [post-sweep 2].  All levels of at most
// kTailCells cells run inside ONE workgroup (mg_tail: vectors in LDS, coefficients from L2) - without it a cycle on a small grid is
// dozens of launches of nothing.  The per-level kernels and the tail call the same per-cell code: their results are identical.
//
// Constant mode.  On a rank-deficient system L 1_present = 0 (checked), so the rank-one term c 1 1^T couples nothing but the means:
// with x = y + mu 1, b = b' + mean(b) 1 the system splits into L y = b' and c N mu = mean(b).  The solver therefore projects the mean
// out of b once, runs PCG on L alone (q = L p and (p, q) do not see a constant in p, and r stays mean-free because the columns of L sum
// to zero), and at the end replaces the mean of x over the present cells by sum(b) / (c n_present^2) - mean(b) / (c N) without absent
// cells.  With solid cells the shifted system is singular along one direction and plain CG from x0 = 0 converges to the member with
// x = 0 on the solid cells and that same mean: the same x.
//
// Reductions are two-stage, fixed order (per-block partials, re-added in index order): a solve is reproducible bit for bit.  alpha,
// beta and the sums stay on the device; the host queues check_every iterations, then reads the state through a pinned word; kernels of
// iterations queued after convergence see the device flag and return at once, so neither x nor the count depends on the cadence.
//
// Kernels: what looks at a cell's neighbours is one template text over the geometry (whole grid, a rank's slab) and the type of the cycle's
// values (mg_cells.h; four cells per thread: mg_quads.h); the pointwise kernels and the sums are here.
// Host: one driver over the type of the cycle's values (mg_grid.h: set-up, V-cycle, PCG iteration, single cycle, the ordinary entries).
// Opt-in: the same iteration around a float32 cycle (mg_f32.h, piso_mg_*_c32_f64): the float instantiations, under the same fp64 outer iteration.
// Opt-in: a start from a guess x0 instead of x = 0 where its residual is below the right-hand side (mg_guess.h, piso_mg_*_guess_*).
#include <type_traits>
#include <vector>

#include "mg_prepared_carve.h"
#include "mg_slab_carve.h"
#include "mg_slab_plan.h"
#include "options.h"
#include "piso_common.h"
#include "slab_comm.h"

namespace piso {

constexpr double kGalerkin = 0.5;      // constant transfers under-correct by ~2 on cell-centred grids (measured counts)
constexpr double kOmega = 0.8;         // Jacobi damping
constexpr int kMinDim = 4;             // no level has fewer cells than this in a dimension
constexpr int kCoarsestSweeps = 16;    // the coarsest level is "solved" by a FIXED number of sweeps
constexpr double kGuard = 1e-10;       // a coarse diagonal this small against its aggregate's diagonals is round-off: the coarse cell is absent
constexpr int kTailCells = 4096;       // levels of at most this many cells run inside one workgroup
constexpr int kTailLds = 6144;         // cells of all tail levels together (r and z of every tail level live in LDS)
constexpr int kTailThreads = 1024;
constexpr int kTailMaxLevels = 8;
constexpr int kMgMaxLevels = 16;
constexpr int kCheckEvery = 4;         // iterations queued between two host looks
constexpr double kRowSumTol = 1e-9;    // rank_deficient = 1: max|row sum| must stay below this times mean|diag|

// (the host-only plan of mg_slab_plan.h restates the constants that shape a hierarchy)
static_assert(kMinDim == kPlanMinDim && kTailCells == kPlanTailCells && kTailLds == kPlanTailLds && kTailMaxLevels == kPlanTailMaxLevels &&
              kMgMaxLevels == kPlanMaxLevels, "mg_slab_plan.h and mg.hip disagree about the hierarchy's constants");

// (MgState, the SC_* slots of `scal`, the level structs Lv / LvF and kMgGrid: mg_slab_carve.h, host code a driver can walk)
enum { MG_FLAG_BORDER = 1, MG_FLAG_ZERO_DIAG_ROW = 2, MG_FLAG_NOT_SINGULAR = 4, MG_FLAG_NOT_PREPARED = 8 };      // (the last: mg_prepared.h)
static_assert(kPlanMaxRanks == kMaxRanks, "mg_slab_carve.h and peer.h disagree about the ranks of a node");

struct Walk { int begin, step; };
__device__ __forceinline__ Walk grid_walk() { return Walk{(int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x)}; }
__device__ __forceinline__ Walk block_walk() { return Walk{(int)threadIdx.x, (int)blockDim.x}; }

struct Nb { int s, w, e, n; };
// neighbours with wrap; where the axis is not periodic the coefficient of a wrapped neighbour is zero (checked at level 0, inherited below)
__device__ __forceinline__ Nb neighbours(int c, int i, int j, int nx, int ny) {
  Nb q;
  q.s = j > 0 ? c - nx : c + (ny - 1) * nx;
  q.w = i > 0 ? c - 1 : c + (nx - 1);
  q.e = i < nx - 1 ? c + 1 : c - (nx - 1);
  q.n = j < ny - 1 ? c + nx : c - (ny - 1) * nx;
  return q;
}
// summation order of the reference stencil: S, W, C, E, N (T: double, or float in the float32 cycle of mg_f32.h)
// `cf(s)` is the cell's coefficient s: read from the level's arrays (stencil), or from the registers of a four-cell thread (mg_quads.h)
template <typename T, typename CF>
__device__ __forceinline__ T stencil_sum(CF cf, T vs, T vw, T vc, T ve, T vn) {
  T t = cf(0) * vs;
  t += cf(1) * vw;
  t += cf(2) * vc;
  t += cf(3) * ve;
  t += cf(4) * vn;
  return t;
}
template <typename LV, typename T>
__device__ __forceinline__ T stencil(const LV& L, int c, T vs, T vw, T vc, T ve, T vn) {
  return stencil_sum<T>([&](int s) { return L.c[s][c]; }, vs, vw, vc, ve, vn);
}
// what a cell becomes from its stencil sum `az`: the second of two sweeps from zero, a sweep, a term of the restricted residual
template <typename T> __device__ __forceinline__ T pre2_out(T di, T rc, T z1, T az) { return z1 + di * (rc - az); }
template <typename T> __device__ __forceinline__ T jac_out(T di, T rc, T vc, T az) { return vc + di * (rc - az); }
template <typename T> __device__ __forceinline__ T restrict_term(T rc, T az) { return rc - az; }

// ---- the per-cell passes, shared by the per-level kernels (grid_walk) and the one-workgroup tail (block_walk) -------------------------
// first sweep from a zero guess
template <typename LV, typename T>
__device__ __forceinline__ void ph_pre1(const LV& L, const T* r, T* z, Walk w) {
  for (int c = w.begin; c < L.n; c += w.step) z[c] = L.dinv[c] * r[c];
}

// sum over a block of any size up to 1024 threads, the same bits in every thread (lanes by butterfly, then the waves in order)
__device__ __forceinline__ double mg_block_sum(double v, double* smem /* [16] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  double s = 0;
  for (int q = 0; q < nw; ++q) s += smem[q];
  return s;
}
__device__ __forceinline__ double mg_block_max_nan(double v, double* smem /* [16] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_max_nan(v);
  __syncthreads();
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  double s = smem[0];
  for (int q = 1; q < nw; ++q) s = nanmax(s, smem[q]);
  return s;
}
// fixed-order sum of `count` partials written by the previous kernel; every block does it redundantly (L2-served)
__device__ __forceinline__ double mg_sum_partials(const double* part, int count, double* smem) {
  double s = 0;
  for (int b = threadIdx.x; b < count; b += blockDim.x) s += part[b];
  return mg_block_sum(s, smem);
}

}  // namespace piso

// the per-cell code that looks at neighbours, over the geometry and the type of the cycle's values; the four-cell kernels of the float32 cycle
#include "mg_cells.h"
#include "mg_quads.h"

namespace piso {

// ---- hierarchy ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mg_setup_fin(const double* parts, int count, double* scal, int rank_deficient, int ncells, MgState* st) {
  __shared__ double smem[16];
  const double sd = mg_sum_partials(parts, count, smem), np = mg_sum_partials(parts + kMgGrid, count, smem);
  const double sb = mg_sum_partials(parts + 2 * kMgGrid, count, smem);
  double mr = 0;
  for (int b = threadIdx.x; b < count; b += blockDim.x) mr = nanmax(mr, parts[3 * kMgGrid + b]);
  mr = mg_block_max_nan(mr, smem);
  if (threadIdx.x == 0) {
    scal[SC_SUM_DIAG] = sd; scal[SC_NPRESENT] = np;
    scal[SC_MEAN_B] = (rank_deficient && np > 0) ? sb / np : 0.0;
    scal[SC_RZ0] = 0; scal[SC_RZ1] = 0;
    if (rank_deficient && np > 0 && mr > kRowSumTol * (sd / np)) atomicOr(&st->flags, MG_FLAG_NOT_SINGULAR);
    (void)ncells;
  }
}
// ---- outer iteration ------------------------------------------------------------------------------------------------------------------
// (R: the type of the cycle's values.  Under the float32 cycle rc = fl32(r) is written beside r; the fp64 cycle reads r itself and rc is not touched)
// r = b' on the present cells (b' = b - mean over the present cells where rank deficient), 0 elsewhere; x = 0
template <typename R>
__global__ __launch_bounds__(kBlock) void mg_init(Lv L, const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r, const double* scal,
                                                  R* __restrict__ rc) {
  const double mean = scal[SC_MEAN_B];
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    x[c] = 0;
    const double rv = L.dinv[c] != 0 ? b[c] - mean : 0.0;
    r[c] = rv;
    if constexpr (std::is_same<R, float>::value) rc[c] = (float)rv;
  }
}
// x += alpha p, r -= alpha q, partials of max|r|
template <typename R>
__global__ __launch_bounds__(kBlock) void mg_update(int n, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p, const double* __restrict__ q,
                                                    const double* scal, int k, const double* part_pq, int n_pq, double* part_max, const MgState* st,
                                                    R* __restrict__ rc) {
  if (st->done) return;
  __shared__ double smem[16];
  const double pq = mg_sum_partials(part_pq, n_pq, smem);
  const double rz = scal[SC_RZ0 + (k & 1)];
  const double alpha = pq != 0 ? rz / pq : 0.0;                          // (guarded like the reference's alpha)
  double m = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) {
    x[c] += alpha * p[c];
    const double rv = r[c] - alpha * q[c];
    r[c] = rv;
    if constexpr (std::is_same<R, float>::value) rc[c] = (float)rv;
    m = nanmax(m, fabs(rv));
  }
  m = mg_block_max_nan(m, smem);
  if (threadIdx.x == 0) part_max[blockIdx.x] = m;
}
__global__ __launch_bounds__(kBlock) void mg_check(const double* part_max, int count, float accuracy, int iterations, MgState* st) {
  if (st->done) return;
  __shared__ double smem[16];
  double m = 0;
  for (int b = threadIdx.x; b < count; b += blockDim.x) m = nanmax(m, part_max[b]);
  m = mg_block_max_nan(m, smem);
  if (threadIdx.x == 0 && m < (double)accuracy) { st->iterations = iterations; st->done = 1; }    // (false for NaN)
}
__global__ __launch_bounds__(kBlock) void mg_sum_x(Lv L, const double* __restrict__ x, double* part) {
  __shared__ double smem[16];
  double s = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) s += L.dinv[c] != 0 ? x[c] : 0.0;
  s = mg_block_sum(s, smem);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int mg_grid(int n) { return grid_for(n, kBlock, kMgGrid); }

// which shape the calling thread's last solve / cycle had (piso_mg_last_dispatch)
enum { MD_LEVELS = 0, MD_TAIL_FIRST, MD_SWEEPS, MD_ITERATIONS, MD_CYCLES, MD_RESIDUAL_RECOMPUTATIONS, MD_CYCLE_ELEM, MD_VEC_MASK, MD_COUNT };
static thread_local int tl_mg_dispatch[MD_COUNT];
static thread_local int tl_mg_dispatch_n = 0;
static void mg_record(int nlev, int tail_first, int sweeps, int iterations, int cycles, int recomputed, int elem, int vec_mask) {
  int* d = tl_mg_dispatch;
  d[MD_LEVELS] = nlev; d[MD_TAIL_FIRST] = tail_first; d[MD_SWEEPS] = sweeps; d[MD_ITERATIONS] = iterations;
  d[MD_CYCLES] = cycles; d[MD_RESIDUAL_RECOMPUTATIONS] = recomputed; d[MD_CYCLE_ELEM] = elem; d[MD_VEC_MASK] = vec_mask;
  tl_mg_dispatch_n = MD_COUNT;
}
static int mg_recomputations(int iterations, int residual_reset) {
  int recomputed = 0;
  for (int k = 1; k < iterations; ++k) recomputed += (k + 1) % residual_reset == 0;
  return recomputed;
}

struct MgPoll { MgState* pinned = nullptr; };
constexpr int kMgPollDevices = 16;
static thread_local MgPoll tl_mg_poll[kMgPollDevices];
static int mg_pinned(MgState** out) {
  int dev = 0;
  PISO_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMgPollDevices) { set_error_msg("piso_mg: device ordinal out of range"); return PISO_ERR_INVALID_ARG; }
  if (!tl_mg_poll[dev].pinned) PISO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&tl_mg_poll[dev].pinned), sizeof(MgState), hipHostMallocDefault));
  *out = tl_mg_poll[dev].pinned;
  return PISO_OK;
}

// builds every level from the caller's matrix and refuses what the solver does not solve (one host look, as the plain CG's set-up has):
// level 0 and the sums (begin), the coarser levels (MgGridT::build of mg_grid.h, MgSlabT::build of mg_slab.h), the look (end)
static int mg_build_begin(const Lv& L0, const double* laplace, const double* b, int rank_deficient, double* parts, double* scal, MgState* st, hipStream_t stream) {
  PISO_HIP_CHECK(hipMemsetAsync(st, 0, sizeof(MgState), stream));
  const int g0 = mg_grid(L0.n);
  mg_setup0<GeoWhole><<<g0, kBlock, 0, stream>>>(laplace, L0, b, parts, st, GeoWhole{});
  mg_setup_fin<<<1, kBlock, 0, stream>>>(parts, g0, scal, rank_deficient, L0.n, st);
  return PISO_OK;
}
// what the set-up's flags refuse (the slab set-up decides on all-reduced flags: mg_slab.h)
static int mg_refusal(int flags) {
  const char* why = nullptr;
  if (flags & MG_FLAG_BORDER) why = "piso_mg: non-zero border entry in a non-periodic direction (the reference stencil reads the neighbouring row there); use the plain CG";
  else if (flags & MG_FLAG_ZERO_DIAG_ROW) why = "piso_mg: a row with a zero diagonal has non-zero entries; use the plain CG";
  else if (flags & MG_FLAG_NOT_SINGULAR) why = "piso_mg: rank_deficient = 1 but the rows of the matrix do not sum to zero; use the plain CG";
  if (!why) return PISO_OK;
  set_error_msg(why);
  return PISO_ERR_UNSUPPORTED_PATTERN;
}
static int mg_build_end(const MgState* st, hipStream_t stream) {
  MgState* pinned = nullptr;
  if (int rc = mg_pinned(&pinned)) return rc;
  PISO_HIP_CHECK(hipMemcpyAsync(pinned, st, sizeof(MgState), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  return mg_refusal(pinned->flags);
}
static int mg_common_args(const char* who, int nx, int ny, const void* a, const void* b, const void* c, const void* ws, int sweeps) {
  char msg[160];
  if (!mg_prepared_dims_ok(nx, ny)) { snprintf(msg, sizeof(msg), "%s: needs at least %d cells in each dimension", who, kMinDim); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (!a || !b || !c || !ws) { snprintf(msg, sizeof(msg), "%s: NULL pointer", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (sweeps < 1 || sweeps > 8) { snprintf(msg, sizeof(msg), "%s: sweeps must be 1 .. 8", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  return PISO_OK;
}
static int mg_iteration_args(const char* who, int max_iterations, int residual_reset) {
  if (max_iterations >= 1 && residual_reset >= 1) return PISO_OK;
  char msg[128];
  snprintf(msg, sizeof(msg), "%s: max_iterations and residual_reset must be positive", who);
  set_error_msg(msg);
  return PISO_ERR_INVALID_ARG;
}

}  // namespace piso

#include "mg_guess.h"
#include "mg_grid.h"
#include "mg_f32.h"
#include "mg_slab.h"
#include "mg_slab_f32.h"
#include "mg_prepared.h"

namespace piso {

// ---- the slab entry points, once over the type of the cycle's values (mg_slab.h, mg_slab_f32.h) ------------------------------------------------
// what the three communicator entry points share: one context, the rank's rows
template <typename C>
static int mg_slab_comm_begin(MgSlabT<C>& M, const char* who, void* comm, int nx, int nyl, int px, int py, const double* laplace, const void* a, const void* b,
                              void* ws, size_t ws_bytes, int sweeps, hipStream_t stream) {
  PisoComm* pc = static_cast<PisoComm*>(comm);
  char msg[96];
  if (!pc || !laplace || !a || !b || !ws) { snprintf(msg, sizeof(msg), "%s: NULL pointer", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  snprintf(msg, sizeof(msg), "%s: the peer communicator is not connected", who);
  PISO_TRY(comm_ready(pc, msg));
  PISO_TRY(mg_slab_begin(M, who, nx, nyl, pc->world, 1, px, py, sweeps, pc, stream));
  M.R[0].rank = pc->rank; M.R[0].Lin = laplace; M.R[0].b = nullptr;
  return M.carve(who, ws, ws_bytes);
}
// ... and the emulated ones: `slabs` virtual ranks over the full arrays
template <typename C>
static int mg_slab_emulated_begin(MgSlabT<C>& M, const char* who, int slabs, int nx, int ny, int px, int py, const double* laplace, const void* a, const void* b,
                                  void* ws, size_t ws_bytes, int sweeps, hipStream_t stream) {
  char msg[96];
  if (!laplace || !a || !b || !ws) { snprintf(msg, sizeof(msg), "%s: NULL pointer", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (slabs < 1 || slabs > kMaxRanks || ny < slabs) { snprintf(msg, sizeof(msg), "%s: needs 1 .. %d slabs", who, kMaxRanks); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (ny % slabs != 0) {                                      // (the plan's refusal, with the rule)
    const MgSlabPlan sp = mg_slab_plan(nx, ny, slabs, opt(OPT_MG_SLAB_GATHER_CELLS));
    set_error_msg(sp.msg);
    return PISO_ERR_INVALID_ARG;
  }
  PISO_TRY(mg_slab_begin(M, who, nx, ny / slabs, slabs, slabs, px, py, sweeps, nullptr, stream));
  for (int r = 0; r < slabs; ++r) { M.R[r].rank = r; M.R[r].Lin = laplace + (size_t)r * (ny / slabs) * nx * 5; M.R[r].b = nullptr; }
  return M.carve(who, ws, ws_bytes);
}

template <typename C>
static int mg_slab_solve_comm(const char* who, void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* divergence_local,
                              double* x_out_local, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,
                              int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PISO_TRY(mg_iteration_args(who, max_iterations, residual_reset));
  tl_mg_last_guess = 0;                                       // (a slab solve takes no guess)
  MgSlabT<C> M;
  PISO_TRY(mg_slab_comm_begin(M, who, comm, nx, ny_local, periodic_x, periodic_y, laplace_local, divergence_local, x_out_local, workspace, workspace_bytes, sweeps, stream));
  M.R[0].b = divergence_local;
  // a refusal of the set-up is the same on every rank (all-reduced flags); whatever else fails is agreed below
  PISO_TRY(M.solve(accuracy, max_iterations, rank_deficient ? 1 : 0, residual_reset, sweeps, iterations_out));
  PISO_HIP_CHECK(hipMemcpyAsync(x_out_local, M.R[0].x, (size_t)nx * ny_local * sizeof(double), hipMemcpyDeviceToDevice, stream));
  return M.finish(who);
}
template <typename C>
static int mg_slab_solve_emulated(const char* who, int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, double* x_out,
                                  float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps, int* iterations_out,
                                  void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PISO_TRY(mg_iteration_args(who, max_iterations, residual_reset));
  tl_mg_last_guess = 0;
  MgSlabT<C> M;
  PISO_TRY(mg_slab_emulated_begin(M, who, slabs, nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, workspace, workspace_bytes, sweeps, stream));
  const size_t n = (size_t)nx * (ny / slabs);
  for (int r = 0; r < slabs; ++r) M.R[r].b = divergence + r * n;
  PISO_TRY(M.solve(accuracy, max_iterations, rank_deficient ? 1 : 0, residual_reset, sweeps, iterations_out));
  for (int r = 0; r < slabs; ++r) PISO_HIP_CHECK(hipMemcpyAsync(x_out + r * n, M.R[r].x, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  return M.finish(who);
}

// one cycle: the rank's rows of r go into the outer residual's rows, its rows of z come out
template <typename C>
static int mg_slab_one_cycle(MgSlabT<C>& M, const double* const* r_rows, double* const* z_rows, int sweeps, const char* who) {
  PISO_TRY(M.build(0));
  const size_t n = (size_t)M.sp.d.nx[0] * M.sp.nyl;
  for (int q = 0; q < M.nloc(); ++q) PISO_TRY(MgSlabOps<C>::load_r(M.R[q], r_rows[q], n, M.s));
  PISO_TRY(M.cycle(sweeps));
  for (int q = 0; q < M.nloc(); ++q) PISO_TRY(MgSlabOps<C>::store_z(M.R[q], z_rows[q], n, M.s));
  M.record(sweeps, 0, 1, 0);
  return M.finish(who);
}
template <typename C>
static int mg_slab_vcycle_comm(const char* who, void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* r_local,
                               double* z_local, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  MgSlabT<C> M;
  PISO_TRY(mg_slab_comm_begin(M, who, comm, nx, ny_local, periodic_x, periodic_y, laplace_local, r_local, z_local, workspace, workspace_bytes, sweeps,
                              static_cast<hipStream_t>(stream_)));
  return mg_slab_one_cycle(M, &r_local, &z_local, sweeps, who);
}
template <typename C>
static int mg_slab_vcycle_emulated(const char* who, int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out,
                                   int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  MgSlabT<C> M;
  PISO_TRY(mg_slab_emulated_begin(M, who, slabs, nx, ny, periodic_x, periodic_y, laplace, r_in, z_out, workspace, workspace_bytes, sweeps, static_cast<hipStream_t>(stream_)));
  const size_t n = (size_t)nx * (ny / slabs);
  std::vector<const double*> r(slabs);
  std::vector<double*> z(slabs);
  for (int q = 0; q < slabs; ++q) { r[q] = r_in + q * n; z[q] = z_out + q * n; }
  return mg_slab_one_cycle(M, r.data(), z.data(), sweeps, who);
}

// a rank's rows of a sharded level, or the whole replicated level, as [nx_out * rows_out][5] (laplace_level_out NULL: sizes only)
template <typename C>
static int mg_slab_level(MgSlabT<C>& M, int q, int level, int* nx_out, int* rows_out, double* out, const char* who) {
  if (level < 0 || level >= M.sp.d.nlev) { *nx_out = 0; *rows_out = 0; set_error_msg("piso_mg_level_slab: no such level"); return PISO_ERR_INVALID_ARG; }
  *nx_out = M.sp.d.nx[level]; *rows_out = M.sp.rows[level];
  if (!out) return PISO_OK;
  PISO_TRY(M.build(0));
  MgGridOps<C>::export_level(M.R[q].lv[level], out, M.s);
  return M.finish(who);
}
template <typename C>
static int mg_slab_level_comm(const char* who, void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, int level, int* nx_out,
                              int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  MgSlabT<C> M;
  PISO_TRY(mg_slab_comm_begin(M, who, comm, nx, ny_local, periodic_x, periodic_y, laplace_local, nx_out, rows_out, workspace, workspace_bytes, 1,
                              static_cast<hipStream_t>(stream_)));
  return mg_slab_level(M, 0, level, nx_out, rows_out, laplace_level_out, who);
}
template <typename C>
static int mg_slab_level_emulated(const char* who, int slabs, int rank, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out,
                                  int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  MgSlabT<C> M;
  PISO_TRY(mg_slab_emulated_begin(M, who, slabs, nx, ny, periodic_x, periodic_y, laplace, nx_out, rows_out, workspace, workspace_bytes, 1, static_cast<hipStream_t>(stream_)));
  if (rank < 0 || rank >= slabs) { set_error_msg("piso_mg_level_slab_emulated: no such rank"); return PISO_ERR_INVALID_ARG; }
  return mg_slab_level(M, rank, level, nx_out, rows_out, laplace_level_out, who);
}

}  // namespace piso

using namespace piso;

extern "C" {

size_t piso_mg_workspace_bytes(int nx, int ny) { return mg_plan_bytes(nx, ny, 8); }
size_t piso_mg_workspace_bytes_cycle(int nx, int ny, int cycle_elem_size) { return mg_plan_bytes(nx, ny, cycle_elem_size); }

// the ordinary entries (mg_grid.h), once per type of the cycle's values
#define PISO_MG_ENTRIES(SUFFIX, C)                                                                                                                               \
  int piso_mg_pcg_solve##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, double* x_out, float accuracy,  \
                                int max_iterations, int rank_deficient, int residual_reset, int sweeps, int* iterations_out, void* workspace,                    \
                                size_t workspace_bytes, piso_stream_t stream) {                                                                                  \
    return mg_solve_entry<C>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations, rank_deficient, residual_reset, sweeps,       \
                             iterations_out, workspace, workspace_bytes, stream, nullptr);                                                                       \
  }                                                                                                                                                              \
  int piso_mg_pcg_solve_guess##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, const double* x0,         \
                                      double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,                     \
                                      int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                      \
    return mg_solve_entry<C>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations, rank_deficient, residual_reset, sweeps,       \
                             iterations_out, workspace, workspace_bytes, stream, x0);                                                                            \
  }                                                                                                                                                              \
  int piso_mg_vcycle##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out, int sweeps,               \
                             void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                                                    \
    return mg_vcycle_entry<C>(nx, ny, periodic_x, periodic_y, laplace, r_in, z_out, sweeps, workspace, workspace_bytes, stream);                                 \
  }                                                                                                                                                              \
  int piso_mg_level##SUFFIX(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out, int* ny_out,                          \
                            double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                          \
    return mg_level_entry<C>(nx, ny, periodic_x, periodic_y, laplace, level, nx_out, ny_out, laplace_level_out, workspace, workspace_bytes, stream);             \
  }
PISO_MG_ENTRIES(_f64, double)
PISO_MG_ENTRIES(_c32_f64, float)
#undef PISO_MG_ENTRIES

// ---- the same solver on y-slabs (mg_slab.h; the float32 cycle on them: mg_slab_f32.h) ---------------------------------------------------------
size_t piso_mg_slab_workspace_bytes_cycle(int nx, int ny_local, int world, int local_ranks, int cycle_elem_size) {
  const piso::OptScope knobs;
  if (ny_local < 1 || world < 1 || local_ranks < 1 || (cycle_elem_size != 4 && cycle_elem_size != 8)) return 0;
  const MgSlabPlan sp = mg_slab_plan(nx, ny_local * world, world, opt(OPT_MG_SLAB_GATHER_CELLS));
  if (sp.status || (cycle_elem_size == 4 && sp.g == 0)) return 0;
  return mg_slab_g_bytes(local_ranks) + (size_t)local_ranks * (cycle_elem_size == 8 ? mg_slab_rank_bytes<double>(sp) : mg_slab_rank_bytes<float>(sp));
}
size_t piso_mg_slab_workspace_bytes(int nx, int ny_local, int world, int local_ranks) {
  return piso_mg_slab_workspace_bytes_cycle(nx, ny_local, world, local_ranks, 8);
}

int piso_mg_slab_plan(int nx, int ny, int world, int gather_cells, int* out, int capacity) {
  const piso::OptScope knobs;
  const MgSlabPlan sp = mg_slab_plan(nx, ny, world, gather_cells > 0 ? gather_cells : opt(OPT_MG_SLAB_GATHER_CELLS));
  if (sp.status) set_error_msg(sp.msg);
  return out ? mg_slab_plan_record(sp, out, capacity) : 0;
}

// the six entries, once per type of the cycle's values
#define PISO_MG_SLAB_ENTRIES(SUFFIX, C)                                                                                                                          \
  int piso_mg_pcg_solve_slab##SUFFIX(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* divergence_local, \
                                     double* x_out_local, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,                \
                                     int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                       \
    return mg_slab_solve_comm<C>("piso_mg_pcg_solve_slab", comm, nx, ny_local, periodic_x, periodic_y, laplace_local, divergence_local, x_out_local, accuracy,   \
                                 max_iterations, rank_deficient, residual_reset, sweeps, iterations_out, workspace, workspace_bytes, stream);                    \
  }                                                                                                                                                              \
  int piso_mg_pcg_solve_slab_emulated##SUFFIX(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,        \
                                              double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,             \
                                              int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                              \
    return mg_slab_solve_emulated<C>("piso_mg_pcg_solve_slab_emulated", slabs, nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy,             \
                                     max_iterations, rank_deficient, residual_reset, sweeps, iterations_out, workspace, workspace_bytes, stream);                \
  }                                                                                                                                                              \
  int piso_mg_vcycle_slab##SUFFIX(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* r_local,          \
                                  double* z_local, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                  \
    return mg_slab_vcycle_comm<C>("piso_mg_vcycle_slab", comm, nx, ny_local, periodic_x, periodic_y, laplace_local, r_local, z_local, sweeps, workspace,         \
                                  workspace_bytes, stream);                                                                                                      \
  }                                                                                                                                                              \
  int piso_mg_vcycle_slab_emulated##SUFFIX(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out,  \
                                           int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                                          \
    return mg_slab_vcycle_emulated<C>("piso_mg_vcycle_slab_emulated", slabs, nx, ny, periodic_x, periodic_y, laplace, r_in, z_out, sweeps, workspace,            \
                                      workspace_bytes, stream);                                                                                                  \
  }                                                                                                                                                              \
  int piso_mg_level_slab##SUFFIX(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, int level, int* nx_out,          \
                                 int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {                      \
    return mg_slab_level_comm<C>("piso_mg_level_slab", comm, nx, ny_local, periodic_x, periodic_y, laplace_local, level, nx_out, rows_out, laplace_level_out,    \
                                 workspace, workspace_bytes, stream);                                                                                            \
  }                                                                                                                                                              \
  int piso_mg_level_slab_emulated##SUFFIX(int slabs, int rank, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out,    \
                                          int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {             \
    return mg_slab_level_emulated<C>("piso_mg_level_slab_emulated", slabs, rank, nx, ny, periodic_x, periodic_y, laplace, level, nx_out, rows_out,               \
                                     laplace_level_out, workspace, workspace_bytes, stream);                                                                     \
  }
PISO_MG_SLAB_ENTRIES(_f64, double)
PISO_MG_SLAB_ENTRIES(_c32_f64, float)
#undef PISO_MG_SLAB_ENTRIES

int piso_mg_last_guess(void) { return tl_mg_last_guess; }

int piso_mg_last_dispatch(int* out, int capacity) {
  const int n = tl_mg_dispatch_n < capacity ? tl_mg_dispatch_n : capacity;
  for (int i = 0; i < n; ++i) out[i] = tl_mg_dispatch[i];
  return tl_mg_dispatch_n;
}

}  // extern "C"
