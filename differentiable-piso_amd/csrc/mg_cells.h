// The per-cell code of the multigrid that looks at a cell's NEIGHBOURS or at the coarse rows above it - the single statement of that
// arithmetic (part of mg.hip's translation unit), as templates over
//   G  the geometry: where a cell's neighbours, the rows below / above and the coarse row of a fine row are.
//        GeoWhole  the whole grid: wrap arithmetic on both axes;
//        GeoSlab   a rank's rows of a sharded level (mg_slab.h): the arrays hold the rank's rows plus one halo row below (row -1) and one
//                  above (row L.ny), so the y-neighbours are the rows below and above in storage - no wrap; only the coarse row of a
//                  REPLICATED coarser level is a global row;
//   R  the type of the cycle's values, with its level struct LvOf<R>: double, or float (the float32 cycle of mg_f32.h).  The outer
//      iteration is fp64 whatever R: under a float cycle mg_residual writes fl32(r) beside r, mg_direction widens z, and the (r, z) partial
//      multiplies the DOUBLE r (rz_term).  What only the outer iteration needs (set-up of level 0, constant mode) has no R.
// The export, mg_pre1 and the one-workgroup tail exist for the whole grid only (a slab's replicated levels run them: mg_slab.h).
#pragma once

namespace piso {

template <typename R> using LvOf = typename MgLevelOf<R>::type;

// ---- geometry ----------------------------------------------------------------------------------------------------------------------------
// the quad of a work item of the four-cell kernels (mg_quads.h) on a level of nx = 4 nxq columns: its row, first column and the places of
// its neighbours
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

struct GeoWhole {
  static constexpr bool kHaloRows = false;                 // the direction updates the grid's cells, nothing else
  __device__ __forceinline__ Nb nb(int c, int i, int j, int nx, int ny) const { return neighbours(c, i, j, nx, ny); }
  __device__ __forceinline__ int js(int j, int ny) const { return j > 0 ? j - 1 : ny - 1; }         // the fine row below / above
  __device__ __forceinline__ int jn(int j, int ny) const { return j < ny - 1 ? j + 1 : 0; }
  __device__ __forceinline__ int erow(int j) const { return j >> 1; }                               // the coarse row of a fine row
  __device__ __forceinline__ bool first_row(int j) const { return j == 0; }                         // the grid's border rows
  __device__ __forceinline__ bool last_row(int j, int ny) const { return j == ny - 1; }
  __device__ __forceinline__ double diag(const double* Lin, int idx) const { return Lin[(size_t)idx * 5 + 2]; }      // a neighbour's diagonal in the caller's matrix
  __device__ __forceinline__ double cells(int n) const { return (double)n; }                        // cells of the whole grid
  __device__ __forceinline__ Quad quad(int row, int iq, int nx, int ny) const { return quad_at(row, iq, nx, ny); }
};
struct GeoSlab {
  int row0, nyg;             // the rank's first global row of this level and the level's global rows
  int coarse_global;         // the coarser level is replicated: its rows are global rows (else the rank's, with halo rows -1 and L.ny / 2)
  const double* dg;          // set-up only: the diagonals of the rank's rows of the caller's matrix, with halo rows
  double ncells;             // cells of the whole grid
  // p' = z + beta p on the rank's two halo rows as well: p never crosses a cut (beta is the same bits on every rank)
  static constexpr bool kHaloRows = true;
  __device__ __forceinline__ Nb nb(int c, int i, int, int nx, int) const {
    Nb q;
    q.s = c - nx; q.w = i > 0 ? c - 1 : c + (nx - 1); q.e = i < nx - 1 ? c + 1 : c - (nx - 1); q.n = c + nx;
    return q;
  }
  __device__ __forceinline__ int js(int j, int) const { return j - 1; }
  __device__ __forceinline__ int jn(int j, int) const { return j + 1; }
  // coarse row of the rank's fine row j, -1 and L.ny included (periodic y: row -1 of rank 0 is row nyg - 1; without, the halo row's dinv is
  // zero and nobody reads the index)
  __device__ __forceinline__ int erow(int j) const { return coarse_global ? ((row0 + j + nyg) % nyg) >> 1 : j >> 1; }
  __device__ __forceinline__ bool first_row(int j) const { return row0 + j == 0; }
  __device__ __forceinline__ bool last_row(int j, int) const { return row0 + j == nyg - 1; }
  __device__ __forceinline__ double diag(const double*, int idx) const { return dg[idx]; }
  __device__ __forceinline__ double cells(int) const { return ncells; }
  // the columns are the whole grid's; the quads below / above are the rows below and above in storage (the halo rows are real rows)
  __device__ __forceinline__ Quad quad(int row, int iq, int nx, int) const {
    Quad q = quad_at(row, iq, nx, 1);
    q.cs = q.c0 - nx; q.cn = q.c0 + nx;
    return q;
  }
};

// a cell's term of (r, z): the fp64 cycle multiplies its own r; the float32 cycle the outer residual rd, in double (NULL: no sum is wanted)
template <typename R>
__device__ __forceinline__ double rz_term(R rc, R zo, const double* rd, int c) {
  if constexpr (std::is_same<R, double>::value) return rc * zo;
  else return rd ? rd[c] * (double)zo : 0.0;
}

// ---- the per-cell passes, shared by the per-level kernels (grid_walk) and the one-workgroup tail (block_walk) -------------------------
// sweeps 1 and 2 from a zero guess in one stencil pass: z1 = dinv r is pointwise, z2 = z1 + dinv (r - A z1)
template <typename G, typename R>
__device__ __forceinline__ void ph_pre2(const LvOf<R>& L, const R* r, R* z, Walk w, G g) {
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = g.nb(c, i, j, L.nx, L.ny);
    const R di = L.dinv[c], rc = r[c], z1 = di * rc;
    const R az = stencil(L, c, L.dinv[q.s] * r[q.s], L.dinv[q.w] * r[q.w], z1, L.dinv[q.e] * r[q.e], L.dinv[q.n] * r[q.n]);
    z[c] = pre2_out(di, rc, z1, az);
  }
}
// one sweep zout = z' + dinv (r - A z'), z' = zin (+ P e on the present cells where e is given); returns the thread's part of (r, zout)
template <typename G, typename R>
__device__ __forceinline__ double ph_jac(const LvOf<R>& L, const R* r, const R* zin, R* zout, const R* e, int nxc, Walk w, const double* rd, G g) {
  double acc = 0;
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = g.nb(c, i, j, L.nx, L.ny);
    const R di = L.dinv[c], rc = r[c];
    R vs = zin[q.s], vw = zin[q.w], vc = zin[c], ve = zin[q.e], vn = zin[q.n];
    if (e) {
      const int iw = i > 0 ? i - 1 : L.nx - 1, ie = i < L.nx - 1 ? i + 1 : 0;
      const int js = g.js(j, L.ny), jn = g.jn(j, L.ny);
      const int row = g.erow(j) * nxc, col = i >> 1;
      if (L.dinv[q.s] != 0) vs += e[g.erow(js) * nxc + col];
      if (L.dinv[q.w] != 0) vw += e[row + (iw >> 1)];
      if (di != 0) vc += e[row + col];
      if (L.dinv[q.e] != 0) ve += e[row + (ie >> 1)];
      if (L.dinv[q.n] != 0) vn += e[g.erow(jn) * nxc + col];
    }
    const R zo = di != 0 ? jac_out(di, rc, vc, stencil(L, c, vs, vw, vc, ve, vn)) : R(0.0);
    zout[c] = zo;
    acc += rz_term(rc, zo, rd, c);
  }
  return acc;
}
// residual of the present cells, summed over each 2 x 2 aggregate: rc = P^T (r - A z)
template <typename G, typename R>
__device__ __forceinline__ void ph_restrict(const LvOf<R>& L, const R* r, const R* z, R* rc, int nxc, int nyc, Walk w, G g) {
  for (int k = w.begin; k < nxc * nyc; k += w.step) {
    const int J = k / nxc, I = k - J * nxc;
    R s = 0;
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int i = 2 * I + di, j = 2 * J + dj;
        if (i >= L.nx || j >= L.ny) continue;
        const int c = j * L.nx + i;
        if (L.dinv[c] == 0) continue;
        const Nb q = g.nb(c, i, j, L.nx, L.ny);
        s += restrict_term(r[c], stencil(L, c, z[q.s], z[q.w], z[c], z[q.e], z[q.n]));
      }
    rc[k] = s;
  }
}

// ---- hierarchy ------------------------------------------------------------------------------------------------------------------------
// level 0: [N][5] -> five arrays + dinv; couplings into absent cells dropped; pattern checks; partials of sum|diag| (ALL rows, as the
// reference's shift has it), the number of present cells, sum of b over them, max|row sum|
template <typename G>
__global__ __launch_bounds__(kBlock) void mg_setup0(const double* __restrict__ Lin, Lv L, const double* __restrict__ b, double* parts, MgState* st, G g) {
  __shared__ double smem[16];
  double sd = 0, np = 0, sb = 0, mr = 0;
  int flags = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = g.nb(c, i, j, L.nx, L.ny);
    double v[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) v[s] = Lin[(size_t)c * 5 + s];
    const bool present = v[2] != 0;
    // (a NaN there is no pattern: it flows into the solve and comes back as NaN)
    if ((!L.per_y && ((g.first_row(j) && v[0] != 0 && v[0] == v[0]) || (g.last_row(j, L.ny) && v[4] != 0 && v[4] == v[4]))) ||
        (!L.per_x && ((i == 0 && v[1] != 0 && v[1] == v[1]) || (i == L.nx - 1 && v[3] != 0 && v[3] == v[3]))))
      flags |= MG_FLAG_BORDER;
    if (!present && (v[0] != 0 || v[1] != 0 || v[3] != 0 || v[4] != 0)) flags |= MG_FLAG_ZERO_DIAG_ROW;
    const int nb[5] = {q.s, q.w, c, q.e, q.n};
#pragma unroll
    for (int s = 0; s < 5; ++s)
      if (s != 2 && (!present || g.diag(Lin, nb[s]) == 0)) v[s] = 0;
#pragma unroll
    for (int s = 0; s < 5; ++s) L.c[s][c] = v[s];
    L.dinv[c] = present ? kOmega / v[2] : 0.0;
    sd += fabs(v[2]);
    if (present) {
      np += 1.0;
      if (b) sb += b[c];
      mr = nanmax(mr, fabs((((v[0] + v[1]) + v[2]) + v[3]) + v[4]));
    }
  }
  sd = mg_block_sum(sd, smem); np = mg_block_sum(np, smem); sb = mg_block_sum(sb, smem); mr = mg_block_max_nan(mr, smem);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = sd; parts[kMgGrid + blockIdx.x] = np; parts[2 * kMgGrid + blockIdx.x] = sb; parts[3 * kMgGrid + blockIdx.x] = mr;
  }
  if (flags) atomicOr(&st->flags, flags);
}
// A_c = kGalerkin P^T A P, one coarse cell per thread: accumulated in double and rounded ONCE per entry to the level's type; the Jacobi
// weight comes from the STORED diagonal
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_coarsen(LvOf<R> F, LvOf<R> Cc, G g) {
  const Walk w = grid_walk();
  for (int k = w.begin; k < Cc.n; k += w.step) {
    const int J = k / Cc.nx, I = k - J * Cc.nx;
    double dg = 0, oS = 0, oW = 0, oE = 0, oN = 0, scale = 0;
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int i = 2 * I + di, j = 2 * J + dj;
        if (i >= F.nx || j >= F.ny) continue;
        const int c = j * F.nx + i;
        const double cc = F.c[2][c];
        if (cc == 0) continue;
        const Nb q = g.nb(c, i, j, F.nx, F.ny);
        scale += fabs(cc);
        dg += cc;
        const double s = F.c[2][q.s] != 0 ? F.c[0][c] : 0.0, ww = F.c[2][q.w] != 0 ? F.c[1][c] : 0.0;
        const double e = F.c[2][q.e] != 0 ? F.c[3][c] : 0.0, n = F.c[2][q.n] != 0 ? F.c[4][c] : 0.0;
        if (dj == 1) dg += s; else oS += s;
        if (di == 1) dg += ww; else oW += ww;
        if (di == 0 && i + 1 < F.nx) dg += e; else oE += e;
        if (dj == 0 && j + 1 < F.ny) dg += n; else oN += n;
      }
    dg *= kGalerkin; oS *= kGalerkin; oW *= kGalerkin; oE *= kGalerkin; oN *= kGalerkin;
    if (!(fabs(dg) > kGuard * kGalerkin * scale)) dg = oS = oW = oE = oN = 0;
    const R dgs = dg;
    Cc.c[0][k] = oS; Cc.c[1][k] = oW; Cc.c[2][k] = dgs; Cc.c[3][k] = oE; Cc.c[4][k] = oN;
    Cc.dinv[k] = dgs != 0 ? kOmega / dgs : 0.0;
  }
}
template <typename R>
__global__ __launch_bounds__(kBlock) void mg_export(LvOf<R> L, double* __restrict__ out) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step)
    for (int s = 0; s < 5; ++s) out[(size_t)c * 5 + s] = L.c[s][c];
}

// ---- outer iteration: the kernels that look at neighbours (the pointwise ones: mg.hip) ----------------------------------------------------
// the true residual r = b' - L x (float32 cycle: rc = fl32(r) beside it; fp64 cycle: rc is not touched)
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_residual(Lv L, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ r, const double* scal,
                                                      const MgState* st, R* __restrict__ rc, G g) {
  if (st->done) return;
  const double mean = scal[SC_MEAN_B];
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = g.nb(c, i, j, L.nx, L.ny);
    const double rv = L.dinv[c] != 0 ? (b[c] - mean) - stencil(L, c, x[q.s], x[q.w], x[c], x[q.e], x[q.n]) : 0.0;
    r[c] = rv;
    if constexpr (std::is_same<R, float>::value) rc[c] = (float)rv;
  }
}
// p' = z + beta p, q = L p', partials of (p', q); block 0 publishes (r, z) for the update kernel and the next beta
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_direction(Lv L, const R* z, const double* pold, double* pnew, double* q, const double* part_rz, int n_rz,
                                                       double* scal, int k, int restart, double* part_pq, const MgState* st, G g) {
  if (st->done) return;
  __shared__ double smem[16];
  const double rz = mg_sum_partials(part_rz, n_rz, smem);
  const double rz_old = scal[SC_RZ0 + ((k + 1) & 1)];
  const double beta = (restart || rz_old == 0) ? 0.0 : rz / rz_old;
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[SC_RZ0 + (k & 1)] = rz;
  if constexpr (G::kHaloRows) {
    for (int h = blockIdx.x * blockDim.x + threadIdx.x; h < 2 * L.nx; h += gridDim.x * blockDim.x) {
      const int ch = h < L.nx ? h - L.nx : L.n + (h - L.nx);
      pnew[ch] = restart ? z[ch] : z[ch] + beta * pold[ch];
    }
  }
  double acc = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb nb = g.nb(c, i, j, L.nx, L.ny);
    double ps, pw, pc, pe, pn;
    if (restart) { ps = z[nb.s]; pw = z[nb.w]; pc = z[c]; pe = z[nb.e]; pn = z[nb.n]; }     // (beta = 0 must not touch an unset p)
    else {
      ps = z[nb.s] + beta * pold[nb.s]; pw = z[nb.w] + beta * pold[nb.w]; pc = z[c] + beta * pold[c];
      pe = z[nb.e] + beta * pold[nb.e]; pn = z[nb.n] + beta * pold[nb.n];
    }
    const double qc = stencil(L, c, ps, pw, pc, pe, pn);
    pnew[c] = pc; q[c] = qc;
    acc += pc * qc;
  }
  acc = mg_block_sum(acc, smem);
  if (threadIdx.x == 0) part_pq[blockIdx.x] = acc;
}
// the constant mode of the shifted system: mean of x over the present cells := sum(b) / (c n_present^2), c = 0.1 sum|diag| / N
template <typename G>
__global__ __launch_bounds__(kBlock) void mg_finish(Lv L, double* __restrict__ x, const double* part, int count, const double* scal, G g) {
  __shared__ double smem[16];
  const double sx = mg_sum_partials(part, count, smem);
  const double np = scal[SC_NPRESENT], cshift = 0.1 * scal[SC_SUM_DIAG] / g.cells(L.n);
  const double add = (np > 0 && cshift != 0) ? scal[SC_MEAN_B] / (cshift * np) - sx / np : 0.0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) x[c] = L.dinv[c] != 0 ? x[c] + add : 0.0;
}

// ---- per-level cycle kernels -----------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(kBlock) void mg_pre1(LvOf<R> L, const R* r, R* z, const MgState* st) {
  if (st->done) return;
  ph_pre1(L, r, z, grid_walk());
}
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_pre2(LvOf<R> L, const R* r, R* z, const MgState* st, G g) {
  if (st->done) return;
  ph_pre2<G, R>(L, r, z, grid_walk(), g);
}
// (rd: the outer residual in double, the float32 cycle's other factor of the (r, z) partial)
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_jacobi(LvOf<R> L, const R* r, const R* zin, R* zout, const R* e, int nxc, double* part_rz, const MgState* st,
                                                    const double* rd, G g) {
  if (st->done) return;
  __shared__ double smem[16];
  double acc = ph_jac<G, R>(L, r, zin, zout, e, nxc, grid_walk(), part_rz ? rd : nullptr, g);
  if (part_rz) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc;
  }
}
template <typename G, typename R>
__global__ __launch_bounds__(kBlock) void mg_restrict(LvOf<R> L, const R* r, const R* z, R* rc, int nxc, int nyc, const MgState* st, G g) {
  if (st->done) return;
  ph_restrict<G, R>(L, r, z, rc, nxc, nyc, grid_walk(), g);
}

// ---- the coarse tail: levels [0, nlev) of `T` inside one workgroup, whole levels only --------------------------------------------------
template <typename R>
struct MgTailT {
  int nlev;
  LvOf<R> lv[kTailMaxLevels];
  int off[kTailMaxLevels];
};
// nu sweeps from a zero guess into `dst` (scratch `tmp`)
template <typename R>
__device__ __forceinline__ void tail_first_sweeps(const LvOf<R>& L, const R* r, R* dst, R* tmp, int nu, Walk w) {
  const int rest = nu >= 2 ? nu - 2 : 0;
  R* cur = (rest & 1) ? tmp : dst;
  if (nu >= 2) ph_pre2<GeoWhole, R>(L, r, cur, w, GeoWhole{}); else ph_pre1(L, r, cur, w);
  __syncthreads();
  for (int s = 0; s < rest; ++s) {
    R* nxt = cur == dst ? tmp : dst;
    ph_jac<GeoWhole, R>(L, r, cur, nxt, nullptr, 0, w, nullptr, GeoWhole{});
    __syncthreads();
    cur = nxt;
  }
}
template <typename R>
__global__ __launch_bounds__(kTailThreads) void mg_tail(MgTailT<R> T, const R* r_in, R* z_out, double* part_rz, int nu, const MgState* st, const double* rd) {
  if (st->done) return;
  __shared__ R rbuf[kTailLds], zbuf[kTailLds], tbuf[kTailCells];
  __shared__ double smem[16];
  const Walk w = block_walk();
  for (int c = w.begin; c < T.lv[0].n; c += w.step) rbuf[c] = r_in[c];
  __syncthreads();
  const int last = T.nlev - 1;
  for (int l = 0; l < last; ++l) {                                      // down
    const LvOf<R>& L = T.lv[l];
    tail_first_sweeps<R>(L, rbuf + T.off[l], zbuf + T.off[l], tbuf, nu, w);
    ph_restrict<GeoWhole, R>(L, rbuf + T.off[l], zbuf + T.off[l], rbuf + T.off[l + 1], T.lv[l + 1].nx, T.lv[l + 1].ny, w, GeoWhole{});
    __syncthreads();
  }
  tail_first_sweeps<R>(T.lv[last], rbuf + T.off[last], zbuf + T.off[last], tbuf, kCoarsestSweeps, w);
  double acc = 0;
  for (int l = last - 1; l >= 0; --l) {                                  // up
    const LvOf<R>& L = T.lv[l];
    R *cur = zbuf + T.off[l], *nxt = tbuf;
    for (int s = 0; s < nu; ++s) {
      acc = ph_jac<GeoWhole, R>(L, rbuf + T.off[l], cur, nxt, s == 0 ? zbuf + T.off[l + 1] : nullptr, T.lv[l + 1].nx, w, (l == 0 && part_rz) ? rd : nullptr, GeoWhole{});
      __syncthreads();
      R* t = cur; cur = nxt; nxt = t;
    }
    if (cur != zbuf + T.off[l]) {                                       // odd nu: the result sits in the scratch the next level needs
      for (int c = w.begin; c < L.n; c += w.step) zbuf[T.off[l] + c] = tbuf[c];
      __syncthreads();
    }
  }
  if (last == 0) {                                                       // (a one-level tail: the sum was never formed)
    acc = 0;
    for (int c = w.begin; c < T.lv[0].n; c += w.step) acc += rz_term(rbuf[c], zbuf[c], rd, c);
  }
  for (int c = w.begin; c < T.lv[0].n; c += w.step) z_out[c] = zbuf[c];
  if (part_rz) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[0] = acc;
  }
}

}  // namespace piso
