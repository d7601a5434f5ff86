// The four-cell kernels of the float32 cycle (part of mg.hip's translation unit), templates over the geometry G of mg_cells.h: GeoWhole for
// the whole grid, GeoSlab for a rank's rows of a sharded level - there the quads below / above are the storage rows -1 / +1 (the halo rows
// are real rows) and the coarse row of a fine row comes from GeoSlab::erow (a global row where the coarser level is replicated).
// A thread owns four consecutive cells of one row and moves them as 16-byte accesses (rows are 16-byte aligned: nx % 4 == 0, the arena
// aligns to 256 and a slab's halo offset is nx floats); the W / E neighbours of the quad's end cells come from the neighbouring lane where
// it holds the same row, from a load at wave edges, row ends and the periodic seam.  The trip count is uniform per wave because the lanes
// exchange values.  Per cell the kernels evaluate the expressions of the scalar kernels (stencil_sum, pre2_out, jac_out, restrict_term): z
// is bitwise the same.
#pragma once

namespace piso {

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// sweeps 1 and 2 from a zero guess (ph_pre2)
template <typename G>
__global__ __launch_bounds__(kBlock) void mg_pre2_x4(LvF L, const float* r, float* z, const MgState* st, G g) {
  if (st->done) return;
  const int nxq = L.nx >> 2, nq = nxq * L.ny;
  for (int base = blockIdx.x * blockDim.x; base < nq; base += gridDim.x * blockDim.x) {      // (uniform trip count per wave: the lanes exchange values)
    const int qd = base + (int)threadIdx.x;
    const bool act = qd < nq;
    const int qq = act ? qd : nq - 1;                                                           // an idle lane redoes the last quad and stores nothing
    const int row = qq / nxq;
    const Quad q = g.quad(row, qq - row * nxq, L.nx, L.ny);
    float cf[5][4], di[4], rc[4], z1[4], zs[4], zn[4], a[4], b[4], out[4];
#pragma unroll
    for (int s = 0; s < 5; ++s) ld4(L.c[s] + q.c0, cf[s]);
    ld4(L.dinv + q.c0, di); ld4(r + q.c0, rc);
    ld4(L.dinv + q.cs, a); ld4(r + q.cs, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) zs[k] = a[k] * b[k];
    ld4(L.dinv + q.cn, a); ld4(r + q.cn, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) { zn[k] = a[k] * b[k]; z1[k] = di[k] * rc[k]; }
    float zw = __shfl_up(z1[3], 1, kWave), ze = __shfl_down(z1[0], 1, kWave);
    if (!q.lane_w) zw = L.dinv[q.cw] * r[q.cw];
    if (!q.lane_e) ze = L.dinv[q.ce] * r[q.ce];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float vw = k > 0 ? z1[k > 0 ? k - 1 : 0] : zw, ve = k < 3 ? z1[k < 3 ? k + 1 : 3] : ze;
      const float az = stencil_sum<float>([&](int s) { return cf[s][k]; }, zs[k], vw, z1[k], ve, zn[k]);
      out[k] = pre2_out(di[k], rc[k], z1[k], az);
    }
    if (act) st4(z + q.c0, out);
  }
}

// one sweep (ph_jac); HAS_E: the coarse correction is added first; RZ: the block's part of (rd, zout) in double
template <typename G, bool HAS_E, bool RZ>
__global__ __launch_bounds__(kBlock) void mg_jacobi_x4(LvF L, const float* r, const float* zin, float* zout, const float* e, int nxc, double* part_rz,
                                                          const MgState* st, const double* rd, G g) {
  if (st->done) return;
  __shared__ double smem[16];
  const int nxq = L.nx >> 2, nq = nxq * L.ny;
  double acc = 0;
  for (int base = blockIdx.x * blockDim.x; base < nq; base += gridDim.x * blockDim.x) {
    const int qd = base + (int)threadIdx.x;
    const bool act = qd < nq;
    const int qq = act ? qd : nq - 1;
    const int row = qq / nxq;
    const Quad q = g.quad(row, qq - row * nxq, L.nx, L.ny);
    float cf[5][4], di[4], rc[4], vc[4], vs[4], vn[4], zo[4];
#pragma unroll
    for (int s = 0; s < 5; ++s) ld4(L.c[s] + q.c0, cf[s]);
    ld4(L.dinv + q.c0, di); ld4(r + q.c0, rc);
    ld4(zin + q.c0, vc); ld4(zin + q.cs, vs); ld4(zin + q.cn, vn);
    float vw = 0, ve = 0;
    if (HAS_E) {
      const int js = g.js(q.j, L.ny), jn = g.jn(q.j, L.ny);
      const int col = q.i0 >> 1;                                                                // (even: the two coarse cells above the quad are one 8-byte load)
      const float2 ec = *reinterpret_cast<const float2*>(e + g.erow(q.j) * nxc + col);
      const float2 es = *reinterpret_cast<const float2*>(e + g.erow(js) * nxc + col);
      const float2 en = *reinterpret_cast<const float2*>(e + g.erow(jn) * nxc + col);
      float ds[4], dn[4];
      ld4(L.dinv + q.cs, ds); ld4(L.dinv + q.cn, dn);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ds[k] != 0) vs[k] += k < 2 ? es.x : es.y;
        if (di[k] != 0) vc[k] += k < 2 ? ec.x : ec.y;
        if (dn[k] != 0) vn[k] += k < 2 ? en.x : en.y;
      }
    }
    vw = __shfl_up(vc[3], 1, kWave); ve = __shfl_down(vc[0], 1, kWave);
    if (!q.lane_w) {
      vw = zin[q.cw];
      if (HAS_E) { const int iw = q.i0 > 0 ? q.i0 - 1 : L.nx - 1; if (L.dinv[q.cw] != 0) vw += e[g.erow(q.j) * nxc + (iw >> 1)]; }
    }
    if (!q.lane_e) {
      ve = zin[q.ce];
      if (HAS_E) { const int ie = q.i0 + 4 < L.nx ? q.i0 + 4 : 0; if (L.dinv[q.ce] != 0) ve += e[g.erow(q.j) * nxc + (ie >> 1)]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float w = k > 0 ? vc[k > 0 ? k - 1 : 0] : vw, ee = k < 3 ? vc[k < 3 ? k + 1 : 3] : ve;
      zo[k] = di[k] != 0 ? jac_out(di[k], rc[k], vc[k], stencil_sum<float>([&](int s) { return cf[s][k]; }, vs[k], w, vc[k], ee, vn[k])) : 0.0f;
    }
    if (act) {
      st4(zout + q.c0, zo);
      if (RZ) {
        const double2 r01 = *reinterpret_cast<const double2*>(rd + q.c0), r23 = *reinterpret_cast<const double2*>(rd + q.c0 + 2);
        acc += r01.x * (double)zo[0]; acc += r01.y * (double)zo[1]; acc += r23.x * (double)zo[2]; acc += r23.y * (double)zo[3];
      }
    }
  }
  if (RZ) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc;
  }
}

// rc = P^T (r - A z) on the present cells (ph_restrict): a thread owns four columns of the fine rows 2J, 2J + 1 = two coarse cells
template <typename G>
__global__ __launch_bounds__(kBlock) void mg_restrict_x4(LvF L, const float* r, const float* z, float* rcoarse, int nxc, int nyc, const MgState* st, G g) {
  if (st->done) return;
  const int nxq = L.nx >> 2, nq = nxq * nyc;
  for (int base = blockIdx.x * blockDim.x; base < nq; base += gridDim.x * blockDim.x) {
    const int qd = base + (int)threadIdx.x;
    const bool act = qd < nq;
    const int qq = act ? qd : nq - 1;
    const int J = qq / nxq, iq = qq - J * nxq;
    float s[2] = {0.0f, 0.0f};
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      const bool have = 2 * J + dj < L.ny;                                                      // (odd ny: the last coarse row has one fine row)
      const Quad q = g.quad(have ? 2 * J + dj : 2 * J, iq, L.nx, L.ny);                        // (every lane takes part in the exchange)
      float cf[5][4], di[4], rc[4], zc[4], zs[4], zn[4];
#pragma unroll
      for (int t = 0; t < 5; ++t) ld4(L.c[t] + q.c0, cf[t]);
      ld4(L.dinv + q.c0, di); ld4(r + q.c0, rc);
      ld4(z + q.c0, zc); ld4(z + q.cs, zs); ld4(z + q.cn, zn);
      float zw = __shfl_up(zc[3], 1, kWave), ze = __shfl_down(zc[0], 1, kWave);
      if (!q.lane_w) zw = z[q.cw];
      if (!q.lane_e) ze = z[q.ce];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = k > 0 ? zc[k > 0 ? k - 1 : 0] : zw, ee = k < 3 ? zc[k < 3 ? k + 1 : 3] : ze;
        const float term = restrict_term(rc[k], stencil_sum<float>([&](int t) { return cf[t][k]; }, zs[k], w, zc[k], ee, zn[k]));
        if (have && di[k] != 0) s[k >> 1] += term;
      }
    }
    if (act) *reinterpret_cast<float2*>(rcoarse + J * nxc + (iq << 1)) = make_float2(s[0], s[1]);
  }
}

}  // namespace piso
