// The float32 V-cycle of mg_f32.h on the y-slabs of mg_slab.h (part of mg.hip's translation unit): the one-GPU float32 definition - level 0 is
// fl32 of the fp64 set-up, level l + 1 fl32(kGalerkin P^T A_l P) accumulated in double, dinv = fl32(kOmega / (double)diag32), the cycle reads
// fl32(r) written beside r, (r, z) is accumulated in double from the double r and the float z - on the slab plan of mg_slab_plan.h.  The
// driver is MgSlabT<float>: the same text as the fp64 slab solve, launching kernel<GeoSlab, float>.  The outer iteration stays fp64 and sharded.
//   * four-cell kernels (mg_quads.h with GeoSlab) run where nx % 4 == 0 - rows stay 16-byte aligned, the halo offset being nx floats; other
//     levels run the scalar slab kernels; option mg_f32_vec 0 runs scalar everywhere (the same z);
//   * levels g .. coarsest: the rank's float rows of level g are all-gathered and every rank runs MgGridT<float>::cycle from level g.
// g = 0 (the whole cycle replicated) is refused: a float32 cycle has nothing to gain there.
// This file holds what MgSlabOps<float> does differently from the fp64 cycle.
#pragma once

namespace piso {

// the fp64 set-up writes the rank's L0, and the rank's float level 0 comes from those rows
template <> inline Lv& MgSlabOps<float>::outer(RK& k, int) { return k.L0; }
template <> inline void MgSlabOps<float>::level0(RK& k, hipStream_t s) { mg_level0_f32<<<mg_grid(k.L0.n), kBlock, 0, s>>>(k.L0, k.lv[0]); }
template <> inline const float* MgSlabOps<float>::gather_src(RK& k, int) { return k.rchunk; }
// one cycle: fl32 of the caller's rows of r (and the rows themselves, the other factor of (r, z)); z comes out widened
template <> inline int MgSlabOps<float>::load_r(RK& k, const double* rows, size_t n, hipStream_t s) {
  PISO_HIP_CHECK(hipMemcpyAsync(k.ro, rows, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  mg_cast_f32<<<mg_grid((int)n), kBlock, 0, s>>>((int)n, rows, k.r[0]);
  return PISO_OK;
}
template <> inline int MgSlabOps<float>::store_z(RK& k, double* rows, size_t n, hipStream_t s) {
  mg_widen_f32<<<mg_grid((int)n), kBlock, 0, s>>>((int)n, k.z_top, rows);
  return PISO_OK;
}
typedef MgSlabT<float> MgSlabF;

}  // namespace piso
