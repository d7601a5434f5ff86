// The float32 V-cycle under the fp64 PCG of mg.hip (opt-in: cycle_elem_size 4, piso_mg_*_c32_f64).  The whole hierarchy and every vector
// of the cycle are stored and computed in float32; the outer iteration - x, r, p, q, the level-0 operator of q = L p and of the residual
// recomputation, alpha, beta, every sum, the stopping rule, the constant mode - stays float64.  Its kernels are the float instantiations of
// mg.hip's and mg_cells.h's templates; this file holds the conversions between the two precisions and what MgGridOps<float> does with them.
// tests/mg_reference_f32.py is the numpy twin.
//   level 0      fl32 of the arrays mg_setup0 produces (couplings into absent cells dropped)
//   level l + 1  fl32(kGalerkin P^T A_l P): accumulated in double from the float32 entries of level l, rounded once per entry; kGuard on the
//                double accumulations
//   dinv         fl32(kOmega / (double)diag32), 0 on absent cells
//   cycle        input fl32(r) (written beside r by mg_init / mg_update / mg_residual / mg_guess_apply), every operation float32 in the
//                order of mg_cells.h, output z float32; mg_direction widens z when it forms p'
//   (r, z)       partials accumulated in double from the double r and the float z
// No scaling of r: a residual beyond float32's range becomes Inf / NaN in the cycle and never counts as converged, and an `accuracy`
// below ~1e-30 is outside this mode (fl32(r) underflows before the stopping rule is met).
// The four-cell kernels (mg_quads.h) are the hot path: z is bitwise the scalar kernels' (option mg_f32_vec 0: scalar kernels on every
// level).  Levels with nx % 4 != 0, the coarsest level and the tail run scalar.
#pragma once

namespace piso {

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

// ---- MgGridOps<float> (mg_grid.h): level 0 is fl32 of the fp64 set-up's; a cycle on its own reads fl32 of the caller's r and forms no
// (r, z); z comes out widened
template <> inline void MgGridOps<float>::level0(const Lv& D, const LvF& F, hipStream_t s) { mg_level0_f32<<<mg_grid(D.n), kBlock, 0, s>>>(D, F); }
template <> inline const float* MgGridOps<float>::load_r(int n, const double* r_in, float* r0, hipStream_t s) {
  mg_cast_f32<<<mg_grid(n), kBlock, 0, s>>>(n, r_in, r0);
  return r0;
}
template <> inline const double* MgGridOps<float>::own_rd(const float*) { return nullptr; }
template <> inline int MgGridOps<float>::store_z(int n, const float* z, double* z_out, hipStream_t s) {
  mg_widen_f32<<<mg_grid(n), kBlock, 0, s>>>(n, z, z_out);
  return PISO_OK;
}

}  // namespace piso
