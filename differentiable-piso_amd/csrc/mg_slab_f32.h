// The float32 V-cycle of mg_f32.h on the y-slabs of mg_slab.h (part of mg.hip's translation unit): the one-GPU float32 definition - level 0 is
// fl32 of the fp64 set-up, level l + 1 fl32(kGalerkin P^T A_l P) accumulated in double, dinv = fl32(kOmega / (double)diag32), the cycle reads
// fl32(r) written beside r, (r, z) is accumulated in double from the double r and the float z - on the slab plan of mg_slab_plan.h.  The
// driver is MgSlabT<float>: the same text as the fp64 slab solve, with the launches below.  The outer iteration stays fp64 and sharded.
//   * per-cell code: mg_cells.inc a fourth time, float + GeoSlab (scalar slab kernels, coarsening, the mixed residual / direction);
//   * four-cell kernels: the bodies of mg_f32.h with QuadSlab - the quads below / above are the storage rows -1 / +1 (halo rows are real
//     rows), coarse rows go through GeoSlab::erow.  Rows stay 16-byte aligned: the halo offset is nx floats and these kernels run only where
//     nx % 4 == 0; other levels run the scalar slab kernels; option mg_f32_vec 0 runs scalar everywhere (the same z);
//   * levels g .. coarsest: the rank's float rows of level g are all-gathered and every rank runs MgGridT<float>::cycle from level g.
// g = 0 (the whole cycle replicated) is refused: a float32 cycle has nothing to gain there.
#pragma once

namespace piso {

#define MG_N(name) name##_slab_f32
#define MG_REAL float
#define MG_LV LvF
#define MG_RDOT_PARAM , const double* rd
#define MG_RDOT_ARG(rd) , rd
#define MG_RDOT(rc, zo, c) (rd ? rd[c] * (double)zo : 0.0)
#define MG_R32_PARAM , float* __restrict__ r32
#define MG_R32_STORE(c, v) r32[c] = (float)v;
#define MG_CYCLE_F32
#define MG_GEO_PARAM , GeoSlab g
#define MG_NB(c, i, j, nx, ny) g.nb(c, i, nx)
#define MG_JS(j, ny) j - 1
#define MG_JN(j, ny) j + 1
#define MG_EROW(j) g.erow(j)
#define MG_FIRST_ROW(j) g.row0 + j == 0
#define MG_LAST_ROW(j, ny) g.row0 + j == g.nyg - 1
#define MG_DIAG(Lin, idx) g.dg[idx]
#define MG_NCELLS(L) g.ncells
// p' = z + beta p on the rank's two halo rows as well (z widened there too)
#define MG_DIRECTION_HALO_ROWS                                                                                                  \
  for (int h = blockIdx.x * blockDim.x + threadIdx.x; h < 2 * L.nx; h += gridDim.x * blockDim.x) {                            \
    const int ch = h < L.nx ? h - L.nx : L.n + (h - L.nx);                                                                      \
    pnew[ch] = restart ? z[ch] : z[ch] + beta * pold[ch];                                                                       \
  }
#include "mg_cells.inc"
#include "mg_cells_undef.inc"

// ---- scalar slab kernels ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mg_pre2_slab_f32(LvF L, const float* r, float* z, const MgState* st, GeoSlab g) {
  if (st->done) return;
  ph_pre2_slab_f32(L, r, z, grid_walk(), g);
}
__global__ __launch_bounds__(kBlock) void mg_jacobi_slab_f32(LvF L, const float* r, const float* zin, float* zout, const float* e, int nxc, double* part_rz,
                                                             const MgState* st, const double* rd, GeoSlab g) {
  if (st->done) return;
  __shared__ double smem[16];
  double acc = ph_jac_slab_f32(L, r, zin, zout, e, nxc, grid_walk(), part_rz ? rd : nullptr, g);
  if (part_rz) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc;
  }
}
__global__ __launch_bounds__(kBlock) void mg_restrict_slab_f32(LvF L, const float* r, const float* z, float* rc, int nxc, int nyc, const MgState* st, GeoSlab g) {
  if (st->done) return;
  ph_restrict_slab_f32(L, r, z, rc, nxc, nyc, grid_walk(), g);
}
struct MgHalosF { int count; float* a[12]; };
__global__ __launch_bounds__(kBlock) void mg_slab_zero_halos_f32(MgHalosF h, int nx, int n) {
  const Walk w = grid_walk();
  for (int i = w.begin; i < nx; i += w.step)
    for (int k = 0; k < h.count; ++k) { h.a[k][i - nx] = 0; h.a[k][n + i] = 0; }
}

// ---- four cells per thread on a slab (mg_quads.inc a second time) ----------------------------------------------------------------------------------
__device__ __forceinline__ Quad quad_at_slab(int row, int iq, int nx) {
  Quad q = quad_at(row, iq, nx, 1);                        // (the columns are the whole grid's)
  q.cs = q.c0 - nx; q.cn = q.c0 + nx;                      // the rows below and above in storage
  return q;
}
#define MG_N(stem) stem##_slab_f32x4
#define MG_GEO_PARAM , GeoSlab g
#define MG_QUAD_AT(row, iq, nx, ny) quad_at_slab(row, iq, nx)
#define MG_JS(j, ny) j - 1
#define MG_JN(j, ny) j + 1
#define MG_EROW(j) g.erow(j)
#include "mg_quads.inc"
#include "mg_cells_undef.inc"

// ---- what MgSlabT<float> launches ---------------------------------------------------------------------------------------------------------------
template <>
struct MgSlabOps<float> {
  typedef MgSlabRankT<float> RK;
  static constexpr bool kRunsG0 = false;
  static Lv& outer(RK& k, int) { return k.L0; }
  // the rank's float level 0 from its fp64 set-up rows
  static void level0(RK& k, hipStream_t s) { mg_level0_f32<<<mg_grid(k.L0.n), kBlock, 0, s>>>(k.L0, k.lv[0]); }
  static void zero_halos(RK& k, int l, hipStream_t s) {
    MgHalosF h{9, {k.lv[l].c[0], k.lv[l].c[1], k.lv[l].c[2], k.lv[l].c[3], k.lv[l].c[4], k.lv[l].dinv, k.r[l], k.z[l], k.t[l]}};
    mg_slab_zero_halos_f32<<<grid_for(k.lv[l].nx, kBlock, 64), kBlock, 0, s>>>(h, k.lv[l].nx, k.lv[l].n);
  }
  static void coarsen_slab(const LvF& F, const LvF& Cc, const GeoSlab& g, hipStream_t s) { mg_coarsen_slab_f32<<<mg_grid(Cc.n), kBlock, 0, s>>>(F, Cc, g); }
  static void coarsen(const LvF& F, const LvF& Cc, hipStream_t s) { mg_coarsen_f32<<<mg_grid(Cc.n), kBlock, 0, s>>>(F, Cc); }
  static bool quads(const LvF& L) { return (L.nx & 3) == 0; }
  static int grid(const LvF& L, bool x4) { return x4 ? mg_grid((L.nx >> 2) * L.ny) : mg_grid(L.n); }
  static void pre(const LvF& L, const float* r, float* z, const MgState* st, const GeoSlab& g, int nu, bool x4, hipStream_t s) {
    if (nu >= 2 && x4) mg_pre2_slab_f32x4<<<grid(L, true), kBlock, 0, s>>>(L, r, z, st, g);
    else if (nu >= 2) mg_pre2_slab_f32<<<grid(L, false), kBlock, 0, s>>>(L, r, z, st, g);
    else mg_pre1_f32<<<grid(L, false), kBlock, 0, s>>>(L, r, z, st);
  }
  static int jacobi(const LvF& L, const float* r, const float* zin, float* zout, const float* e, int nxc, double* part_rz, const MgState* st, const GeoSlab& g,
                    bool x4, const double* rd, hipStream_t s) {
    const int gl = grid(L, x4);
    const bool rz = part_rz != nullptr;
    if (!x4) mg_jacobi_slab_f32<<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
    else if (e && rz) mg_jacobi_slab_f32x4<true, true><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
    else if (e) mg_jacobi_slab_f32x4<true, false><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
    else if (rz) mg_jacobi_slab_f32x4<false, true><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
    else mg_jacobi_slab_f32x4<false, false><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
    return gl;
  }
  static void restrict_to(const LvF& L, const float* r, const float* z, float* rc, int nxc, int nyc, const MgState* st, const GeoSlab& g, bool x4, hipStream_t s) {
    if (x4) mg_restrict_slab_f32x4<<<mg_grid((L.nx >> 2) * nyc), kBlock, 0, s>>>(L, r, z, rc, nxc, nyc, st, g);
    else mg_restrict_slab_f32<<<mg_grid(nxc * nyc), kBlock, 0, s>>>(L, r, z, rc, nxc, nyc, st, g);
  }
  static const float* gather_src(RK& k, int) { return k.rchunk; }
  static void init(const Lv& L0, RK& k, int g0, hipStream_t s) { mg_init_f32<<<g0, kBlock, 0, s>>>(L0, k.b, k.x, k.ro, k.scal, k.r[0]); }
  static void residual(const Lv& L0, RK& k, int g0, const GeoSlab& g, hipStream_t s) {
    mg_residual_slab_f32<<<g0, kBlock, 0, s>>>(L0, k.b, k.x, k.ro, k.scal, k.st, k.r[0], g);
  }
  static void direction(const Lv& L0, RK& k, int g0, int it, int restart, const GeoSlab& g, hipStream_t s) {
    mg_direction_slab_f32<<<g0, kBlock, 0, s>>>(L0, k.z_top, k.p[it & 1], k.p[(it + 1) & 1], k.q, k.g, 1, k.scal, it, restart, k.part_pq, k.st, g);
  }
  static void update(int n0, RK& k, int g0, int it, hipStream_t s) {
    mg_update_f32<<<g0, kBlock, 0, s>>>(n0, k.x, k.ro, k.p[(it + 1) & 1], k.q, k.scal, it, k.g + 1, 1, k.part_max, k.st, k.r[0]);
  }
  static void export_level(const LvF& L, double* out, hipStream_t s) { mg_export_f32<<<mg_grid(L.n), kBlock, 0, s>>>(L, out); }
  // one cycle: fl32 of the caller's rows of r (and the rows themselves, the other factor of (r, z)); z comes out widened
  static int load_r(RK& k, const double* rows, size_t n, hipStream_t s) {
    PISO_HIP_CHECK(hipMemcpyAsync(k.ro, rows, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    mg_cast_f32<<<mg_grid((int)n), kBlock, 0, s>>>((int)n, rows, k.r[0]);
    return PISO_OK;
  }
  static int store_z(RK& k, double* rows, size_t n, hipStream_t s) {
    mg_widen_f32<<<mg_grid((int)n), kBlock, 0, s>>>((int)n, k.z_top, rows);
    return PISO_OK;
  }
};
typedef MgSlabT<float> MgSlabF;

}  // namespace piso
