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

// (what the host launches of these, MgGridOps<float>, and the driver over them: mg_grid.h)

}  // namespace piso
