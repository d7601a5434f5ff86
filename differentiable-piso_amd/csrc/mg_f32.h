// The float32 V-cycle under the fp64 PCG of mg.hip (opt-in: cycle_elem_size 4, piso_mg_*_c32_f64).  The whole hierarchy and every vector
// of the cycle are stored and computed in float32; the outer iteration - x, r, p, q, the level-0 operator of q = L p and of the residual
// recomputation, alpha, beta, every sum, the stopping rule, the constant mode - stays float64 and runs the kernels of mg.hip or their
// mixed instantiations.  tests/mg_reference_f32.py is the numpy twin.
//   level 0      fl32 of the arrays mg_setup0 produces (couplings into absent cells dropped)
//   level l + 1  fl32(kGalerkin P^T A_l P): accumulated in double from the float32 entries of level l, rounded once per entry; kGuard on the
//                double accumulations
//   dinv         fl32(kOmega / (double)diag32), 0 on absent cells
//   cycle        input fl32(r) (written beside r by mg_init_f32 / mg_update_f32 / mg_residual_f32), every operation float32 in the
//                order of mg_cells.inc (its third inclusion, below), output z float32; mg_direction_f32 widens z when it forms p'
//   (r, z)       partials accumulated in double from the double r and the float z
// No scaling of r: a residual beyond float32's range becomes Inf / NaN in the cycle and never counts as converged, and an `accuracy`
// below ~1e-30 is outside this mode (fl32(r) underflows before the stopping rule is met).
// The four-cell kernels (*_f32x4) are the hot path: a thread owns four consecutive cells of one row and moves them as 16-byte accesses
// (rows are 16-byte aligned: nx % 4 == 0 and the arena aligns to 256); the W / E neighbours of the quad's end cells come from the
// neighbouring lane where it holds the same row, from a load at wave edges, row ends and the periodic seam.  Per cell they evaluate the
// expressions of the scalar kernels (stencil_sum, pre2_out, jac_out, restrict_term): z is bitwise the same (option mg_f32_vec 0: scalar
// kernels on every level).  Levels with nx % 4 != 0, the coarsest level and the tail run scalar.
#pragma once

namespace piso {

#define MG_N(name) name##_f32
#define MG_REAL float
#define MG_LV LvF
#define MG_RDOT_PARAM , const double* rd
#define MG_RDOT_ARG(rd) , rd
#define MG_RDOT(rc, zo, c) (rd ? rd[c] * (double)zo : 0.0)
#define MG_R32_PARAM , float* __restrict__ r32
#define MG_R32_STORE(c, v) r32[c] = (float)v;
#define MG_WHOLE_GRID
#define MG_CYCLE_F32
#define MG_GEO_PARAM
#define MG_NB(c, i, j, nx, ny) neighbours(c, i, j, nx, ny)
#define MG_JS(j, ny) j > 0 ? j - 1 : ny - 1
#define MG_JN(j, ny) j < ny - 1 ? j + 1 : 0
#define MG_EROW(j) (j >> 1)
#define MG_FIRST_ROW(j) j == 0
#define MG_LAST_ROW(j, ny) j == ny - 1
#define MG_DIAG(Lin, idx) Lin[(size_t)idx * 5 + 2]
#define MG_NCELLS(L) (double)L.n
#define MG_DIRECTION_HALO_ROWS
#include "mg_cells.inc"
#include "mg_cells_undef.inc"

// ---- set-up and conversions ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mg_level0_f32(Lv D, LvF F) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < D.n; c += w.step) {
#pragma unroll
    for (int s = 0; s < 5; ++s) F.c[s][c] = (float)D.c[s][c];
    const float dg = (float)D.c[2][c];
    F.dinv[c] = dg != 0 ? (float)(kOmega / (double)dg) : 0.0f;
  }
}
__global__ __launch_bounds__(kBlock) void mg_cast_f32(int n, const double* __restrict__ in, float* __restrict__ out) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) out[c] = (float)in[c];
}
__global__ __launch_bounds__(kBlock) void mg_widen_f32(int n, const float* __restrict__ in, double* __restrict__ out) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) out[c] = in[c];
}

// ---- mixed outer kernels: mg_init / mg_update of mg.hip that also emit fl32(r) --------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mg_init_f32(Lv L, const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r, const double* scal,
                                                      float* __restrict__ r32) {
  const double mean = scal[SC_MEAN_B];
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    x[c] = 0;
    const double rv = L.dinv[c] != 0 ? b[c] - mean : 0.0;
    r[c] = rv;
    r32[c] = (float)rv;
  }
}
__global__ __launch_bounds__(kBlock) void mg_update_f32(int n, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p, const double* __restrict__ q,
                                                        const double* scal, int k, const double* part_pq, int n_pq, double* part_max, const MgState* st,
                                                        float* __restrict__ r32) {
  if (st->done) return;
  __shared__ double smem[16];
  const double pq = mg_sum_partials(part_pq, n_pq, smem);
  const double rz = scal[SC_RZ0 + (k & 1)];
  const double alpha = pq != 0 ? rz / pq : 0.0;
  double m = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) {
    x[c] += alpha * p[c];
    const double rc = r[c] - alpha * q[c];
    r[c] = rc;
    r32[c] = (float)rc;
    m = nanmax(m, fabs(rc));
  }
  m = mg_block_max_nan(m, smem);
  if (threadIdx.x == 0) part_max[blockIdx.x] = m;
}

// ---- four cells per thread ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// the quad of work item `qd` on a level of nx = 4 nxq columns: its row, first column and the places of its neighbours
struct Quad {
  int j, i0, c0, cs, cn, cw, ce;      // c0: first cell; cs / cn: first cell of the quad below / above; cw / ce: the cells left of cell 0 / right of cell 3
  bool lane_w, lane_e;                // the neighbouring lane holds that cell
};
__device__ __forceinline__ Quad quad_at(int row, int iq, int nx, int ny) {
  Quad q;
  const int lane = threadIdx.x & 63;
  q.j = row; q.i0 = iq << 2; q.c0 = row * nx + q.i0;
  q.cs = row > 0 ? q.c0 - nx : q.c0 + (ny - 1) * nx;
  q.cn = row < ny - 1 ? q.c0 + nx : q.c0 - (ny - 1) * nx;
  q.cw = q.i0 > 0 ? q.c0 - 1 : q.c0 + (nx - 1);
  q.ce = q.i0 + 4 < nx ? q.c0 + 4 : q.c0 + 4 - nx;
  q.lane_w = lane > 0 && q.i0 > 0;
  q.lane_e = lane < 63 && q.i0 + 4 < nx;
  return q;
}

// (mg_pre2_f32x4, mg_jacobi_f32x4<HAS_E, RZ>, mg_restrict_f32x4: mg_quads.inc, whole grid; mg_slab_f32.h includes it again for a rank's slab)
#define MG_N(stem) stem##_f32x4
#define MG_GEO_PARAM
#define MG_QUAD_AT(row, iq, nx, ny) quad_at(row, iq, nx, ny)
#define MG_JS(j, ny) j > 0 ? j - 1 : ny - 1
#define MG_JN(j, ny) j < ny - 1 ? j + 1 : 0
#define MG_EROW(j) (j >> 1)
#include "mg_quads.inc"
#include "mg_cells_undef.inc"

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
struct MgPlanF {
  int nlev = 0, tail_first = -1;
  Lv L0;                                   // the fp64 level 0 of the outer iteration
  LvF lv[kMgMaxLevels];
  float *r[kMgMaxLevels], *z[kMgMaxLevels], *t[kMgMaxLevels];
  double *r64, *p[2], *q, *parts, *part_rz, *part_pq, *part_max, *scal;
  MgState* st;
};
static bool mg_plan_f32(int nx, int ny, int per_x, int per_y, Arena& ar, MgPlanF& P) {
  const MgDims d = mg_dims(nx, ny);
  const int n0 = d.nx[0] * d.ny[0];
  Lv& D = P.L0;
  D.nx = d.nx[0]; D.ny = d.ny[0]; D.n = n0; D.per_x = per_x; D.per_y = per_y;
  for (int s = 0; s < 5; ++s) D.c[s] = ar.take<double>(n0);
  D.dinv = ar.take<double>(n0);
  for (int l = 0; l < d.nlev; ++l) {
    LvF& L = P.lv[l];
    L.nx = d.nx[l]; L.ny = d.ny[l]; L.n = L.nx * L.ny; L.per_x = per_x; L.per_y = per_y;
    for (int s = 0; s < 5; ++s) L.c[s] = ar.take<float>(L.n);
    L.dinv = ar.take<float>(L.n);
    P.r[l] = ar.take<float>(L.n); P.z[l] = ar.take<float>(L.n); P.t[l] = ar.take<float>(L.n);
  }
  P.nlev = d.nlev;
  P.tail_first = d.tail_first;
  P.r64 = ar.take<double>(n0);
  P.p[0] = ar.take<double>(n0); P.p[1] = ar.take<double>(n0); P.q = ar.take<double>(n0);
  P.parts = ar.take<double>(4 * kMgGrid);
  P.part_rz = ar.take<double>(kMgGrid); P.part_pq = ar.take<double>(kMgGrid); P.part_max = ar.take<double>(kMgGrid);
  P.scal = ar.take<double>(SC_COUNT_MG);
  P.st = ar.take<MgState>(1);
  return ar.ok();
}

// the fp64 set-up and its refusals (mg_build_begin / mg_build_end of mg.hip), then the float32 levels
static int mg_build_f32(const MgPlanF& P, const double* laplace, const double* b, int rank_deficient, hipStream_t stream) {
  PISO_TRY(mg_build_begin(P.L0, laplace, b, rank_deficient, P.parts, P.scal, P.st, stream));
  mg_level0_f32<<<mg_grid(P.L0.n), kBlock, 0, stream>>>(P.L0, P.lv[0]);
  for (int l = 0; l + 1 < P.nlev; ++l) mg_coarsen_f32<<<mg_grid(P.lv[l + 1].n), kBlock, 0, stream>>>(P.lv[l], P.lv[l + 1]);
  PISO_LAUNCH_CHECK();
  return mg_build_end(P.st, stream);
}

struct MgRunF {
  const MgPlanF& P;
  int nu;
  bool use_tail, vec;
  hipStream_t stream;
  int vec_mask = 0;
  bool quads(int l) const { return vec && (P.lv[l].nx & 3) == 0; }
  int grid(int l, bool x4) const { return x4 ? mg_grid((P.lv[l].nx >> 2) * P.lv[l].ny) : mg_grid(P.lv[l].n); }
  // one sweep on level l; returns the number of (r, z) partials it left (rd given)
  int jacobi(int l, bool x4, const float* r, const float* zin, float* zout, const float* e, const double* rd) const {
    const LvF& L = P.lv[l];
    const int g = grid(l, x4), nxc = e ? P.lv[l + 1].nx : 0;
    double* part = rd ? P.part_rz : nullptr;
    if (!x4) mg_jacobi_f32<<<g, kBlock, 0, stream>>>(L, r, zin, zout, e, nxc, part, P.st, rd);
    else if (e && rd) mg_jacobi_f32x4<true, true><<<g, kBlock, 0, stream>>>(L, r, zin, zout, e, nxc, part, P.st, rd);
    else if (e) mg_jacobi_f32x4<true, false><<<g, kBlock, 0, stream>>>(L, r, zin, zout, e, nxc, part, P.st, rd);
    else if (rd) mg_jacobi_f32x4<false, true><<<g, kBlock, 0, stream>>>(L, r, zin, zout, e, nxc, part, P.st, rd);
    else mg_jacobi_f32x4<false, false><<<g, kBlock, 0, stream>>>(L, r, zin, zout, e, nxc, part, P.st, rd);
    return g;
  }
  float* first_sweeps(int l, bool x4, const float* r, int sweeps) const {
    const LvF& L = P.lv[l];
    float* cur = P.z[l];
    if (sweeps >= 2 && x4) mg_pre2_f32x4<<<grid(l, true), kBlock, 0, stream>>>(L, r, cur, P.st);
    else if (sweeps >= 2) mg_pre2_f32<<<grid(l, false), kBlock, 0, stream>>>(L, r, cur, P.st);
    else mg_pre1_f32<<<grid(l, false), kBlock, 0, stream>>>(L, r, cur, P.st);
    for (int s = 2; s < sweeps; ++s) {
      float* nxt = cur == P.z[l] ? P.t[l] : P.z[l];
      jacobi(l, x4, r, cur, nxt, nullptr, nullptr);
      cur = nxt;
    }
    return cur;
  }
  // z = M^-1 r0 (mg_cycle of mg.hip in float32); rd: the outer residual in double - the partials of (rd, z) are left in P.part_rz
  // (l0: the level r0 lives on - 0, or the first replicated level of a slab solve, as mg_cycle has it)
  float* cycle(const float* r0, const double* rd, int* n_rz, int l0 = 0) {
    const int end = use_tail ? P.tail_first : P.nlev - 1;
    float* zc[kMgMaxLevels];
    vec_mask = 0;
    for (int l = l0; l < end; ++l) {
      const float* r = l == l0 ? r0 : P.r[l];
      const bool x4 = quads(l);
      if (x4) vec_mask |= 1 << l;
      zc[l] = first_sweeps(l, x4, r, nu);
      const LvF& C = P.lv[l + 1];
      if (x4) mg_restrict_f32x4<<<mg_grid((P.lv[l].nx >> 2) * C.ny), kBlock, 0, stream>>>(P.lv[l], r, zc[l], P.r[l + 1], C.nx, C.ny, P.st);
      else mg_restrict_f32<<<mg_grid(C.n), kBlock, 0, stream>>>(P.lv[l], r, zc[l], P.r[l + 1], C.nx, C.ny, P.st);
    }
    const float* rend = end == l0 ? r0 : P.r[end];
    const double* rd_end = end == l0 ? rd : nullptr;
    if (use_tail) {
      MgTail_f32 T;
      T.nlev = P.nlev - end;
      int off = 0;
      for (int k = 0; k < T.nlev; ++k) { T.lv[k] = P.lv[end + k]; T.off[k] = off; off += T.lv[k].n; }
      mg_tail_f32<<<1, kTailThreads, 0, stream>>>(T, rend, P.z[end], rd_end ? P.part_rz : nullptr, nu, P.st, rd_end);
      zc[end] = P.z[end];
      *n_rz = 1;
    } else {
      float* cur = first_sweeps(end, false, rend, kCoarsestSweeps - 1);
      float* nxt = cur == P.z[end] ? P.t[end] : P.z[end];
      *n_rz = jacobi(end, false, rend, cur, nxt, nullptr, rd_end);
      zc[end] = nxt;
    }
    for (int l = end - 1; l >= l0; --l) {
      const float* r = l == l0 ? r0 : P.r[l];
      const bool x4 = quads(l);
      float* cur = zc[l];
      for (int s = 0; s < nu; ++s) {
        float* nxt = cur == P.z[l] ? P.t[l] : P.z[l];
        const int g = jacobi(l, x4, r, cur, nxt, s == 0 ? zc[l + 1] : nullptr, (l == l0 && s == nu - 1) ? rd : nullptr);
        if (l == l0) *n_rz = g;
        cur = nxt;
      }
      zc[l] = cur;
    }
    return zc[l0];
  }
};

}  // namespace piso
