// The per-cell code of the multigrid that looks at a cell's NEIGHBOURS or at the coarse rows above it - the single statement of that
// arithmetic, included four times by mg.hip:
//   * for the WHOLE grid (wrap arithmetic on both axes; the macros expand to the expressions this code has always had, token for token),
//   * for a rank's SLAB of a sharded level (mg_slab.h, GeoSlab g): the arrays hold the rank's rows plus one halo row below (row -1) and
//     one above (row L.ny), so the y-neighbours are the rows below and above in storage - no wrap; only the coarse row of a REPLICATED
//     coarser level is a global row.
//   * for the float32 cycle (mg_f32.h): the whole grid's geometry with MG_REAL float, MG_LV LvF; MG_CYCLE_F32 leaves out what only the
//     fp64 outer iteration needs (set-up of level 0, constant mode); mg_residual and mg_direction become the mixed instantiations that
//     emit fl32(r) (MG_R32_PARAM / MG_R32_STORE) and read a float z; the (r, z) partial multiplies the DOUBLE r (MG_RDOT*).
//   * for the float32 cycle on a rank's slab (mg_slab_f32.h): MG_REAL float with GeoSlab - the scalar slab kernels' passes, the coarsening and
//     the mixed residual / direction of a sharded level.
// MG_REAL / MG_LV: the type of the cycle's values and of its level struct (double / Lv in the first two inclusions, token for token what
// the code had).  MG_WHOLE_GRID adds the export, the per-level cycle kernels and the one-workgroup tail.
// MG_N(name) names a function; MG_GEO_PARAM is the slab's trailing parameter; MG_NB the neighbours; MG_JS / MG_JN / MG_EROW the fine rows
// below / above and the coarse row of a fine row; MG_FIRST_ROW / MG_LAST_ROW the grid's border rows; MG_DIAG a neighbour's diagonal in the
// caller's matrix; MG_NCELLS the cells of the whole grid; MG_DIRECTION_HALO_ROWS what the direction does beyond the rank's rows.
// sweeps 1 and 2 from a zero guess in one stencil pass: z1 = dinv r is pointwise, z2 = z1 + dinv (r - A z1)
__device__ __forceinline__ void MG_N(ph_pre2)(const MG_LV& L, const MG_REAL* r, MG_REAL* z, Walk w MG_GEO_PARAM) {
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = MG_NB(c, i, j, L.nx, L.ny);
    const MG_REAL di = L.dinv[c], rc = r[c], z1 = di * rc;
    const MG_REAL az = stencil(L, c, L.dinv[q.s] * r[q.s], L.dinv[q.w] * r[q.w], z1, L.dinv[q.e] * r[q.e], L.dinv[q.n] * r[q.n]);
    z[c] = pre2_out(di, rc, z1, az);
  }
}
// one sweep zout = z' + dinv (r - A z'), z' = zin (+ P e on the present cells where e is given); returns the thread's part of (r, zout)
__device__ __forceinline__ double MG_N(ph_jac)(const MG_LV& L, const MG_REAL* r, const MG_REAL* zin, MG_REAL* zout, const MG_REAL* e, int nxc, Walk w MG_RDOT_PARAM MG_GEO_PARAM) {
  double acc = 0;
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = MG_NB(c, i, j, L.nx, L.ny);
    const MG_REAL di = L.dinv[c], rc = r[c];
    MG_REAL vs = zin[q.s], vw = zin[q.w], vc = zin[c], ve = zin[q.e], vn = zin[q.n];
    if (e) {
      const int iw = i > 0 ? i - 1 : L.nx - 1, ie = i < L.nx - 1 ? i + 1 : 0;
      const int js = MG_JS(j, L.ny), jn = MG_JN(j, L.ny);
      const int row = MG_EROW(j) * nxc, col = i >> 1;
      if (L.dinv[q.s] != 0) vs += e[MG_EROW(js) * nxc + col];
      if (L.dinv[q.w] != 0) vw += e[row + (iw >> 1)];
      if (di != 0) vc += e[row + col];
      if (L.dinv[q.e] != 0) ve += e[row + (ie >> 1)];
      if (L.dinv[q.n] != 0) vn += e[MG_EROW(jn) * nxc + col];
    }
    const MG_REAL zo = di != 0 ? jac_out(di, rc, vc, stencil(L, c, vs, vw, vc, ve, vn)) : MG_REAL(0.0);
    zout[c] = zo;
    acc += MG_RDOT(rc, zo, c);
  }
  return acc;
}
// residual of the present cells, summed over each 2 x 2 aggregate: rc = P^T (r - A z)
__device__ __forceinline__ void MG_N(ph_restrict)(const MG_LV& L, const MG_REAL* r, const MG_REAL* z, MG_REAL* rc, int nxc, int nyc, Walk w MG_GEO_PARAM) {
  for (int k = w.begin; k < nxc * nyc; k += w.step) {
    const int J = k / nxc, I = k - J * nxc;
    MG_REAL s = 0;
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int i = 2 * I + di, j = 2 * J + dj;
        if (i >= L.nx || j >= L.ny) continue;
        const int c = j * L.nx + i;
        if (L.dinv[c] == 0) continue;
        const Nb q = MG_NB(c, i, j, L.nx, L.ny);
        s += restrict_term(r[c], stencil(L, c, z[q.s], z[q.w], z[c], z[q.e], z[q.n]));
      }
    rc[k] = s;
  }
}
#ifndef MG_CYCLE_F32
// level 0: [N][5] -> five arrays + dinv; couplings into absent cells dropped; pattern checks; partials of sum|diag| (ALL rows, as the
// reference's shift has it), the number of present cells, sum of b over them, max|row sum|
__global__ __launch_bounds__(kBlock) void MG_N(mg_setup0)(const double* __restrict__ Lin, Lv L, const double* __restrict__ b, double* parts, MgState* st MG_GEO_PARAM) {
  __shared__ double smem[16];
  double sd = 0, np = 0, sb = 0, mr = 0;
  int flags = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = MG_NB(c, i, j, L.nx, L.ny);
    double v[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) v[s] = Lin[(size_t)c * 5 + s];
    const bool present = v[2] != 0;
    // (a NaN there is no pattern: it flows into the solve and comes back as NaN)
    if ((!L.per_y && ((MG_FIRST_ROW(j) && v[0] != 0 && v[0] == v[0]) || (MG_LAST_ROW(j, L.ny) && v[4] != 0 && v[4] == v[4]))) ||
        (!L.per_x && ((i == 0 && v[1] != 0 && v[1] == v[1]) || (i == L.nx - 1 && v[3] != 0 && v[3] == v[3]))))
      flags |= MG_FLAG_BORDER;
    if (!present && (v[0] != 0 || v[1] != 0 || v[3] != 0 || v[4] != 0)) flags |= MG_FLAG_ZERO_DIAG_ROW;
    const int nb[5] = {q.s, q.w, c, q.e, q.n};
#pragma unroll
    for (int s = 0; s < 5; ++s)
      if (s != 2 && (!present || MG_DIAG(Lin, nb[s]) == 0)) v[s] = 0;
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
#endif
// A_c = kGalerkin P^T A P, one coarse cell per thread: accumulated in double and rounded ONCE per entry to the level's type; the Jacobi
// weight comes from the STORED diagonal
__global__ __launch_bounds__(kBlock) void MG_N(mg_coarsen)(MG_LV F, MG_LV Cc MG_GEO_PARAM) {
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
        const Nb q = MG_NB(c, i, j, F.nx, F.ny);
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
    const MG_REAL dgs = dg;
    Cc.c[0][k] = oS; Cc.c[1][k] = oW; Cc.c[2][k] = dgs; Cc.c[3][k] = oE; Cc.c[4][k] = oN;
    Cc.dinv[k] = dgs != 0 ? kOmega / dgs : 0.0;
  }
}
// the true residual r = b' - L x (float32 cycle: fl32(r) beside it)
__global__ __launch_bounds__(kBlock) void MG_N(mg_residual)(Lv L, const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ r, const double* scal,
                                                      const MgState* st MG_R32_PARAM MG_GEO_PARAM) {
  if (st->done) return;
  const double mean = scal[SC_MEAN_B];
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb q = MG_NB(c, i, j, L.nx, L.ny);
    const double rv = L.dinv[c] != 0 ? (b[c] - mean) - stencil(L, c, x[q.s], x[q.w], x[c], x[q.e], x[q.n]) : 0.0;
    r[c] = rv;
    MG_R32_STORE(c, rv)
  }
}
// p' = z + beta p, q = L p', partials of (p', q); block 0 publishes (r, z) for the update kernel and the next beta
__global__ __launch_bounds__(kBlock) void MG_N(mg_direction)(Lv L, const MG_REAL* z, const double* pold, double* pnew, double* q, const double* part_rz, int n_rz,
                                                       double* scal, int k, int restart, double* part_pq, const MgState* st MG_GEO_PARAM) {
  if (st->done) return;
  __shared__ double smem[16];
  const double rz = mg_sum_partials(part_rz, n_rz, smem);
  const double rz_old = scal[SC_RZ0 + ((k + 1) & 1)];
  const double beta = (restart || rz_old == 0) ? 0.0 : rz / rz_old;
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[SC_RZ0 + (k & 1)] = rz;
  MG_DIRECTION_HALO_ROWS
  double acc = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const int j = c / L.nx, i = c - j * L.nx;
    const Nb nb = MG_NB(c, i, j, L.nx, L.ny);
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
#ifndef MG_CYCLE_F32
// the constant mode of the shifted system: mean of x over the present cells := sum(b) / (c n_present^2), c = 0.1 sum|diag| / N
__global__ __launch_bounds__(kBlock) void MG_N(mg_finish)(Lv L, double* __restrict__ x, const double* part, int count, const double* scal MG_GEO_PARAM) {
  __shared__ double smem[16];
  const double sx = mg_sum_partials(part, count, smem);
  const double np = scal[SC_NPRESENT], cshift = 0.1 * scal[SC_SUM_DIAG] / MG_NCELLS(L);
  const double add = (np > 0 && cshift != 0) ? scal[SC_MEAN_B] / (cshift * np) - sx / np : 0.0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) x[c] = L.dinv[c] != 0 ? x[c] + add : 0.0;
}
#endif
#ifdef MG_WHOLE_GRID
// ---- whole grid only: the export, the per-level cycle kernels and the coarse tail (the slab has launchers of its own in mg_slab.h) -------
__global__ __launch_bounds__(kBlock) void MG_N(mg_export)(MG_LV L, double* __restrict__ out) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step)
    for (int s = 0; s < 5; ++s) out[(size_t)c * 5 + s] = L.c[s][c];
}

// ---- per-level cycle kernels -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void MG_N(mg_pre1)(MG_LV L, const MG_REAL* r, MG_REAL* z, const MgState* st) {
  if (st->done) return;
  ph_pre1(L, r, z, grid_walk());
}
__global__ __launch_bounds__(kBlock) void MG_N(mg_pre2)(MG_LV L, const MG_REAL* r, MG_REAL* z, const MgState* st) {
  if (st->done) return;
  MG_N(ph_pre2)(L, r, z, grid_walk());
}
__global__ __launch_bounds__(kBlock) void MG_N(mg_jacobi)(MG_LV L, const MG_REAL* r, const MG_REAL* zin, MG_REAL* zout, const MG_REAL* e, int nxc, double* part_rz,
                                                    const MgState* st MG_RDOT_PARAM) {
  if (st->done) return;
  __shared__ double smem[16];
  double acc = MG_N(ph_jac)(L, r, zin, zout, e, nxc, grid_walk() MG_RDOT_ARG(part_rz ? rd : nullptr));
  if (part_rz) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc;
  }
}
__global__ __launch_bounds__(kBlock) void MG_N(mg_restrict)(MG_LV L, const MG_REAL* r, const MG_REAL* z, MG_REAL* rc, int nxc, int nyc, const MgState* st) {
  if (st->done) return;
  MG_N(ph_restrict)(L, r, z, rc, nxc, nyc, grid_walk());
}

// ---- the coarse tail: levels [0, nlev) of `T` inside one workgroup ----------------------------------------------------------------------
struct MG_N(MgTail) {
  int nlev;
  MG_LV lv[kTailMaxLevels];
  int off[kTailMaxLevels];
};
// nu sweeps from a zero guess into `dst` (scratch `tmp`)
__device__ __forceinline__ void MG_N(tail_first_sweeps)(const MG_LV& L, const MG_REAL* r, MG_REAL* dst, MG_REAL* tmp, int nu, Walk w) {
  const int rest = nu >= 2 ? nu - 2 : 0;
  MG_REAL* cur = (rest & 1) ? tmp : dst;
  if (nu >= 2) MG_N(ph_pre2)(L, r, cur, w); else ph_pre1(L, r, cur, w);
  __syncthreads();
  for (int s = 0; s < rest; ++s) {
    MG_REAL* nxt = cur == dst ? tmp : dst;
    MG_N(ph_jac)(L, r, cur, nxt, nullptr, 0, w MG_RDOT_ARG(nullptr));
    __syncthreads();
    cur = nxt;
  }
}
// (float32 cycle: `rd` is the outer residual in double, the other factor of the (r, z) partial)
__global__ __launch_bounds__(kTailThreads) void MG_N(mg_tail)(MG_N(MgTail) T, const MG_REAL* r_in, MG_REAL* z_out, double* part_rz, int nu, const MgState* st MG_RDOT_PARAM) {
  if (st->done) return;
  __shared__ MG_REAL rbuf[kTailLds], zbuf[kTailLds], tbuf[kTailCells];
  __shared__ double smem[16];
  const Walk w = block_walk();
  for (int c = w.begin; c < T.lv[0].n; c += w.step) rbuf[c] = r_in[c];
  __syncthreads();
  const int last = T.nlev - 1;
  for (int l = 0; l < last; ++l) {                                      // down
    const MG_LV& L = T.lv[l];
    MG_N(tail_first_sweeps)(L, rbuf + T.off[l], zbuf + T.off[l], tbuf, nu, w);
    MG_N(ph_restrict)(L, rbuf + T.off[l], zbuf + T.off[l], rbuf + T.off[l + 1], T.lv[l + 1].nx, T.lv[l + 1].ny, w);
    __syncthreads();
  }
  MG_N(tail_first_sweeps)(T.lv[last], rbuf + T.off[last], zbuf + T.off[last], tbuf, kCoarsestSweeps, w);
  double acc = 0;
  for (int l = last - 1; l >= 0; --l) {                                  // up
    const MG_LV& L = T.lv[l];
    MG_REAL *cur = zbuf + T.off[l], *nxt = tbuf;
    for (int s = 0; s < nu; ++s) {
      acc = MG_N(ph_jac)(L, rbuf + T.off[l], cur, nxt, s == 0 ? zbuf + T.off[l + 1] : nullptr, T.lv[l + 1].nx, w MG_RDOT_ARG((l == 0 && part_rz) ? rd : nullptr));
      __syncthreads();
      MG_REAL* t = cur; cur = nxt; nxt = t;
    }
    if (cur != zbuf + T.off[l]) {                                       // odd nu: the result sits in the scratch the next level needs
      for (int c = w.begin; c < L.n; c += w.step) zbuf[T.off[l] + c] = tbuf[c];
      __syncthreads();
    }
  }
  if (last == 0) {                                                       // (a one-level tail: the sum was never formed)
    acc = 0;
    for (int c = w.begin; c < T.lv[0].n; c += w.step) acc += MG_RDOT(rbuf[c], zbuf[c], c);
  }
  for (int c = w.begin; c < T.lv[0].n; c += w.step) z_out[c] = zbuf[c];
  if (part_rz) {
    acc = mg_block_sum(acc, smem);
    if (threadIdx.x == 0) part_rz[0] = acc;
  }
}
#endif
