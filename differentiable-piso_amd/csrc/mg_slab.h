// The multigrid PCG of mg.hip on y-slabs (part of that translation unit: the per-cell code, the whole-grid kernels and the driver MgGridT are its).
// The algorithm, its constants, the hierarchy's dimensions, the stopping rule, the constant-mode treatment and the device-side
// alpha / beta are the one-GPU solver's; only where rows live and how sums are formed differ.  mg_slab_plan.h is the plan:
//   * levels [0, g) are SHARDED: a rank holds its nyl >> l rows of every array plus one halo row below and one above (zero where the
//     grid ends without a periodic wrap).  The slab kernels are the per-cell code of mg_cells.h with GeoSlab: y-neighbours are the rows
//     below and above in storage, coarse indices are the rank's own (2 x 2 aggregates never straddle a cut);
//   * level g and everything coarser is REPLICATED: a rank forms its rows of level g from its rows of level g - 1 (the coefficients
//     once per solve, the restricted residual once per cycle), the rows are all-gathered, and every rank runs levels g .. coarsest
//     with the whole-grid kernels / mg_tail (MgGridT::cycle from level g).  A rank reads its part of the correction e_g directly;
//   * g = 0: the cycle is replicated altogether; the outer iteration (x, r, p, q) is always sharded at level 0.
// What crosses a cut goes through the host collectives of slab_comm.h only (both transports carry it): halo rows by comm_exchange_rows,
// every global sum from per-rank fixed-order partials by comm_allreduce_f64 (bitwise the same on every rank: every rank takes the same
// decisions), the rows of level g and the ranks' maxima of |r| by comm_allgather_f64 (the check kernel takes nanmax over them).
// One driver over a vector of per-rank contexts and a link: the communicator link has one context, the loopback link V virtual ranks
// on one device whose rows it copies - no mailbox - so that one process can test every cut.  The driver is ONE text over the type C of the
// cycle's values, MgSlabT<C>, with its launches in MgSlabOps<C> (kernel<GeoSlab, C>): MgSlab = MgSlabT<double> is this solver, MgSlabT<float>
// runs the float32 cycle of mg_f32.h on the same plan under the same fp64 outer iteration (mg_slab_f32.h).
#pragma once

namespace piso {

// (MgSlabRankT<C>, what a rank holds, and mg_slab_carve, its workspace: mg_slab_carve.h - host code a driver can walk)

// ---- kernels of the slab alone (GeoSlab and the per-cell kernels over it: mg_cells.h) ----------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mg_slab_diag(const double* __restrict__ Lin, double* __restrict__ dg, int n) {
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) dg[c] = Lin[(size_t)c * 5 + 2];
}

// ---- what the sums need around the collectives ---------------------------------------------------------------------------------------------
// out[0] = the `count` partials of the previous kernel in index order
__global__ __launch_bounds__(kBlock) void mg_slab_collapse(const double* part, int count, double* out, const MgState* st) {
  if (st && st->done) return;
  __shared__ double smem[16];
  const double s = mg_sum_partials(part, count, smem);
  if (threadIdx.x == 0) out[0] = s;
}
__global__ __launch_bounds__(kBlock) void mg_slab_collapse_max(const double* part, int count, double* out, const MgState* st) {
  if (st->done) return;
  __shared__ double smem[16];
  double m = 0;
  for (int b = threadIdx.x; b < count; b += blockDim.x) m = nanmax(m, part[b]);
  m = mg_block_max_nan(m, smem);
  if (threadIdx.x == 0) out[0] = m;
}
// the set-up partials of mg_setup0 as summable values g[4 .. 8] = sum|diag|, present cells, sum(b), the two pattern flags; g[9] = max|row sum|
__global__ __launch_bounds__(kBlock) void mg_slab_setup_collapse(const double* parts, int count, const MgState* st, double* g) {
  __shared__ double smem[16];
  const double sd = mg_sum_partials(parts, count, smem), np = mg_sum_partials(parts + kMgGrid, count, smem);
  const double sb = mg_sum_partials(parts + 2 * kMgGrid, count, smem);
  double mr = 0;
  for (int b = threadIdx.x; b < count; b += blockDim.x) mr = nanmax(mr, parts[3 * kMgGrid + b]);
  mr = mg_block_max_nan(mr, smem);
  if (threadIdx.x == 0) {
    g[4] = sd; g[5] = np; g[6] = sb;
    g[7] = (st->flags & MG_FLAG_BORDER) ? 1.0 : 0.0; g[8] = (st->flags & MG_FLAG_ZERO_DIAG_ROW) ? 1.0 : 0.0;
    g[9] = mr;
  }
}
// ... and back into the layout mg_setup_fin reads, as ONE partial per sum and the ranks' maxima: the same kernel finishes the set-up
__global__ void mg_slab_setup_spread(const double* g, const double* gmax, int world, double* parts, MgState* st) {
  if (threadIdx.x != 0) return;
  for (int r = 0; r < world; ++r) {
    parts[r] = r == 0 ? g[4] : 0.0; parts[kMgGrid + r] = r == 0 ? g[5] : 0.0; parts[2 * kMgGrid + r] = r == 0 ? g[6] : 0.0;
    parts[3 * kMgGrid + r] = gmax[r];
  }
  st->flags |= (g[7] != 0 ? MG_FLAG_BORDER : 0) | (g[8] != 0 ? MG_FLAG_ZERO_DIAG_ROW : 0);
}
// zero the halo rows of up to 12 arrays (pointers at owned row 0 of n = nx * rows cells): where the grid ends no exchange writes them
template <typename T> struct MgHalosT { int count; T* a[12]; };
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_slab_zero_halos(MgHalosT<T> h, int nx, int n) {
  const Walk w = grid_walk();
  for (int i = w.begin; i < nx; i += w.step)
    for (int k = 0; k < h.count; ++k) { h.a[k][i - nx] = 0; h.a[k][n + i] = 0; }
}
// g = 0: the rank's rows of the replicated z with the rows below and above them (periodic wrap, or zero)
__global__ __launch_bounds__(kBlock) void mg_slab_take_rows(const double* __restrict__ zfull, double* __restrict__ zloc, int nx, int rows, int row0, int nyg, int per_y,
                                                            const MgState* st) {
  if (st->done) return;
  const Walk w = grid_walk();
  for (int k = w.begin; k < (rows + 2) * nx; k += w.step) {
    const int jl = k / nx - 1, i = k - (jl + 1) * nx;
    int jg = row0 + jl;
    const bool wrapped = jg < 0 || jg >= nyg;
    if (wrapped) jg = jg < 0 ? jg + nyg : jg - nyg;
    zloc[jl * nx + i] = (wrapped && !per_y) ? 0.0 : zfull[(size_t)jg * nx + i];
  }
}
__global__ __launch_bounds__(kBlock) void mg_slab_dot(const double* __restrict__ a, const double* __restrict__ b, int n, double* part, const MgState* st) {
  if (st->done) return;
  __shared__ double smem[16];
  double acc = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < n; c += w.step) acc += a[c] * b[c];
  acc = mg_block_sum(acc, smem);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// loopback all-reduce: the ranks' buffers lie kMgSlabG apart; sum in rank order, write to all
__global__ void mg_loop_allreduce(double* base, int world, int count) {
  const int q = threadIdx.x;
  if (q >= count) return;
  double s = 0;
  for (int r = 0; r < world; ++r) s += base[(size_t)r * kMgSlabG + q];
  for (int r = 0; r < world; ++r) base[(size_t)r * kMgSlabG + q] = s;
}


// ---- the link: exchange the halo rows of one array, all-reduce, all-gather (T: double, or the float rows of the float32 cycle) ---------------
inline int comm_rows(PisoComm* pc, bool per, double* row0, int nx, int rows, hipStream_t s) { return comm_exchange_rows(pc, per, row0, nx, rows, s); }
inline int comm_rows(PisoComm* pc, bool per, float* row0, int nx, int rows, hipStream_t s) { return comm_exchange_rows_f32(pc, per, row0, nx, rows, s); }
inline int comm_gather(PisoComm* pc, const double* src, double* dst, size_t count, hipStream_t s) { return comm_allgather_f64(pc, src, dst, count, s); }
inline int comm_gather(PisoComm* pc, const float* src, float* dst, size_t count, hipStream_t s) { return comm_allgather_f32(pc, src, dst, count, s); }
struct MgLink {
  PisoComm* pc;              // NULL: loopback over the virtual ranks of R
  int world;
  bool periodic_y;
  hipStream_t s;

  // sel(rank) -> owned row 0 of an array of `rows` rows of nx cells with halo rows
  template <typename RK, typename Sel>
  int exchange(std::vector<RK>& R, Sel sel, int nx, int rows, bool ring = false) {
    const bool per = periodic_y || ring;
    if (pc) return comm_rows(pc, per, sel(R[0]), nx, rows, s);
    for (int r = 0; r < world; ++r) {
      const int lo = r > 0 ? r - 1 : (per ? world - 1 : -1), hi = r < world - 1 ? r + 1 : (per ? 0 : -1);
      auto* row0 = sel(R[r]);
      const size_t bytes = (size_t)nx * sizeof(*row0);
      if (lo >= 0) PISO_HIP_CHECK(hipMemcpyAsync(row0 - nx, sel(R[lo]) + (size_t)(rows - 1) * nx, bytes, hipMemcpyDeviceToDevice, s));
      if (hi >= 0) PISO_HIP_CHECK(hipMemcpyAsync(row0 + (size_t)rows * nx, sel(R[hi]), bytes, hipMemcpyDeviceToDevice, s));
    }
    return PISO_OK;
  }
  template <typename RK>
  int allreduce(std::vector<RK>& R, int off, int count) {
    if (pc) return comm_allreduce_f64(pc, R[0].g + off, count, s);
    if (world > 1) mg_loop_allreduce<<<1, 64, 0, s>>>(R[0].g + off, world, count);
    return PISO_OK;
  }
  template <typename RK, typename Src, typename Dst>
  int allgather(std::vector<RK>& R, Src src, Dst dst, size_t count) {
    if (pc) return comm_gather(pc, src(R[0]), dst(R[0]), count, s);
    for (int q = 0; q < world; ++q)
      for (int r = 0; r < world; ++r)
        PISO_HIP_CHECK(hipMemcpyAsync(dst(R[q]) + (size_t)r * count, src(R[r]), count * sizeof(*src(R[r])), hipMemcpyDeviceToDevice, s));
    return PISO_OK;
  }
};

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
template <typename C>
static size_t mg_slab_rank_bytes(const MgSlabPlan& sp) {
  Arena ar(reinterpret_cast<void*>(256), ~(size_t)0);
  MgSlabRankT<C> k;
  mg_slab_carve(sp, 0, 0, ar, k);
  return align_up(ar.used, 256);
}
static size_t mg_slab_g_bytes(int local_ranks) { return align_up((size_t)local_ranks * kMgSlabG * sizeof(double), 256); }

// ---- what the driver launches ------------------------------------------------------------------------------------------------------------------
// (x4, rd and the launches of the kernels that have a four-cell form: mg_grid.h; the replicated levels run MgGridOps<C>)
template <typename C>
struct MgSlabOps {
  typedef MgSlabRankT<C> RK;
  typedef LvOf<C> Level;
  static constexpr bool kRunsG0 = std::is_same<C, double>::value;       // g = 0, the whole cycle replicated, is the fp64 cycle's alone
  static void zero_halos(RK& k, int l, hipStream_t s) {
    MgHalosT<C> h{9, {k.lv[l].c[0], k.lv[l].c[1], k.lv[l].c[2], k.lv[l].c[3], k.lv[l].c[4], k.lv[l].dinv, k.r[l], k.z[l], k.t[l]}};
    mg_slab_zero_halos<C><<<grid_for(k.lv[l].nx, kBlock, 64), kBlock, 0, s>>>(h, k.lv[l].nx, k.lv[l].n);
  }
  static void coarsen_slab(const Level& F, const Level& Cc, const GeoSlab& g, hipStream_t s) { mg_coarsen<GeoSlab, C><<<mg_grid(Cc.n), kBlock, 0, s>>>(F, Cc, g); }
  // the first sweep (nu 1) or the first two (ph_pre2) from a zero guess
  static void pre(const Level& L, const C* r, C* z, const MgState* st, const GeoSlab& g, int nu, bool x4, hipStream_t s) {
    if (nu >= 2) mg_launch_pre2<GeoSlab, C>(L, r, z, st, x4, g, s);
    else mg_pre1<C><<<mg_grid(L.n), kBlock, 0, s>>>(L, r, z, st);
  }
  static int jacobi(const Level& L, const C* r, const C* zin, C* zout, const C* e, int nxc, double* part_rz, const MgState* st, const GeoSlab& g, bool x4,
                    const double* rd, hipStream_t s) {
    return mg_launch_jacobi<GeoSlab, C>(L, r, zin, zout, e, nxc, part_rz, st, x4, rd, g, s);
  }
  static void restrict_to(const Level& L, const C* r, const C* z, C* rc, int nxc, int nyc, const MgState* st, const GeoSlab& g, bool x4, hipStream_t s) {
    mg_launch_restrict<GeoSlab, C>(L, r, z, rc, nxc, nyc, st, x4, g, s);
  }
  // the outer iteration (r[0]: what the cycle reads, fl32(r) beside r under the float32 cycle)
  static void init(const Lv& L0, RK& k, int g0, hipStream_t s) { mg_init<C><<<g0, kBlock, 0, s>>>(L0, k.b, k.x, k.ro, k.scal, k.r[0]); }
  static void residual(const Lv& L0, RK& k, int g0, const GeoSlab& g, hipStream_t s) {
    mg_residual<GeoSlab, C><<<g0, kBlock, 0, s>>>(L0, k.b, k.x, k.ro, k.scal, k.st, k.r[0], g);
  }
  static void direction(const Lv& L0, RK& k, int g0, int it, int restart, const GeoSlab& g, hipStream_t s) {
    mg_direction<GeoSlab, C><<<g0, kBlock, 0, s>>>(L0, k.z_top, k.p[it & 1], k.p[(it + 1) & 1], k.q, k.g, 1, k.scal, it, restart, k.part_pq, k.st, g);
  }
  static void update(int n0, RK& k, int g0, int it, hipStream_t s) {
    mg_update<C><<<g0, kBlock, 0, s>>>(n0, k.x, k.ro, k.p[(it + 1) & 1], k.q, k.scal, it, k.g + 1, 1, k.part_max, k.st, k.r[0]);
  }
  // by type: the fp64 level 0 the set-up writes and the cycle's level 0 from it; the rank's rows of the residual of level g; one cycle from
  // the caller's rows of r, its rows of z out
  static Lv& outer(RK& k, int g);
  static void level0(RK& k, hipStream_t s);
  static const C* gather_src(RK& k, int g);
  static int load_r(RK& k, const double* rows, size_t n, hipStream_t s);
  static int store_z(RK& k, double* rows, size_t n, hipStream_t s);
};
// the fp64 cycle: its level 0 IS the set-up's (g = 0: the chunk is the rank's rows of level 0)
template <> inline Lv& MgSlabOps<double>::outer(RK& k, int g) { return g > 0 ? k.lv[0] : k.chunk; }
template <> inline void MgSlabOps<double>::level0(RK&, hipStream_t) {}
template <> inline const double* MgSlabOps<double>::gather_src(RK& k, int g) { return g > 0 ? k.rchunk : k.ro; }
template <> inline int MgSlabOps<double>::load_r(RK& k, const double* rows, size_t n, hipStream_t s) {
  PISO_HIP_CHECK(hipMemcpyAsync(k.ro, rows, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PISO_OK;
}
template <> inline int MgSlabOps<double>::store_z(RK& k, double* rows, size_t n, hipStream_t s) {
  PISO_HIP_CHECK(hipMemcpyAsync(rows, k.z_top, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PISO_OK;
}

// levels g .. coarsest on a rank's replicated copy, as the one-GPU driver runs them: its plan as a view of the rank's levels (a cycle on its
// own there - the fp64 cycle leaves partials of (r_g, z_g) nobody reads, the float32 cycle none)
template <typename C>
static C* mg_slab_replicated(const MgSlabPlan& sp, bool use_tail, bool vec, MgSlabRankT<C>& k, int nu, int* vec_mask, hipStream_t s) {
  MgPlanT<C> P;
  P.H.nlev = sp.d.nlev; P.H.tail_first = sp.tail_first;
  for (int l = sp.g; l < P.H.nlev; ++l) { P.H.lv[l] = k.lv[l]; P.S.r[l] = k.r[l]; P.S.z[l] = k.z[l]; P.S.t[l] = k.t[l]; }
  P.S.part_rz = k.part_rz; P.S.st = k.st;
  MgGridT<C> run(P, nu, use_tail, vec, s);
  int n_rz = 0;
  C* z = run.cycle(k.r[sp.g], MgGridOps<C>::own_rd(k.r[sp.g]), &n_rz, sp.g);
  *vec_mask |= run.vec_mask;
  return z;
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------------
template <typename C>
struct MgSlabT {
  typedef MgSlabRankT<C> RK;
  typedef MgSlabOps<C> Ops;
  typedef typename RK::Level Level;
  std::vector<RK> R;
  MgLink link;
  MgSlabPlan sp;
  int per_x, per_y;
  hipStream_t s;
  bool use_tail, vec;
  int vec_mask = 0;

  int nloc() const { return (int)R.size(); }
  GeoSlab geo(const RK& k, int l) const {
    GeoSlab g;
    g.row0 = k.rank * (l == 0 ? sp.nyl : sp.rows[l]); g.nyg = sp.d.ny[l]; g.coarse_global = (l + 1 >= sp.g) ? 1 : 0; g.dg = nullptr; g.ncells = (double)sp.d.nx[0] * sp.d.ny[0];
    return g;
  }
  bool quads(const RK& k, int l) const { return vec && MgGridOps<C>::quads(k.lv[l]); }

  // carve `ws` (the g buffers of all local ranks first, contiguous: the loopback all-reduce walks them)
  int carve(const char* who, void* ws, size_t bytes) {
    const size_t per_rank = mg_slab_rank_bytes<C>(sp), gb = mg_slab_g_bytes(nloc());
    char msg[96];
    if (bytes < gb + per_rank * nloc()) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
    PISO_HIP_CHECK(hipMemsetAsync(ws, 0, gb, s));
    for (int q = 0; q < nloc(); ++q) {
      Arena ar(static_cast<char*>(ws) + gb + (size_t)q * per_rank, per_rank);
      R[q].g = static_cast<double*>(ws) + (size_t)q * kMgSlabG;
      if (!mg_slab_carve(sp, per_x, per_y, ar, R[q])) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
    }
    return PISO_OK;
  }

  // every level from the ranks' rows of the caller's matrix; the same refusals as mg_build, decided on all-reduced flags
  int build(int rank_deficient) {
    MgState* pinned = nullptr;
    PISO_TRY(mg_pinned(&pinned));
    const int nx = sp.d.nx[0], n0 = nx * sp.nyl, g0 = mg_grid(n0);
    for (RK& k : R) {
      PISO_HIP_CHECK(hipMemsetAsync(k.st, 0, sizeof(MgState), s));
      for (int l = 0; l < sp.g; ++l) Ops::zero_halos(k, l, s);
      MgHalosT<double> h{3, {k.p[0], k.p[1], k.x}};
      if (sp.g == 0) { h.a[3] = k.ro; h.a[4] = reinterpret_cast<double*>(k.zo); h.count = 5; }      // (g = 0 is the fp64 cycle's alone)
      mg_slab_zero_halos<double><<<grid_for(nx, kBlock, 64), kBlock, 0, s>>>(h, nx, n0);
      mg_slab_diag<<<g0, kBlock, 0, s>>>(k.Lin, k.p[0], n0);          // (p[0] is free until the first direction)
    }
    // (around the ring whatever the border: the whole-grid set-up looks at the wrapped row's diagonal there too)
    PISO_TRY(link.exchange(R, [](RK& k) { return k.p[0]; }, nx, sp.nyl, true));
    for (RK& k : R) {
      GeoSlab g = geo(k, 0);
      g.dg = k.p[0];
      mg_setup0<GeoSlab><<<g0, kBlock, 0, s>>>(k.Lin, Ops::outer(k, sp.g), k.b, k.parts, k.st, g);
      Ops::level0(k, s);
      mg_slab_setup_collapse<<<1, kBlock, 0, s>>>(k.parts, g0, k.st, k.g);
    }
    PISO_TRY(link.allreduce(R, 4, 5));
    PISO_TRY(link.allgather(R, [](RK& k) { return k.g + 9; }, [](RK& k) { return k.gmax; }, 1));
    for (RK& k : R) {
      mg_slab_setup_spread<<<1, 64, 0, s>>>(k.g, k.gmax, sp.world, k.parts, k.st);
      mg_setup_fin<<<1, kBlock, 0, s>>>(k.parts, sp.world, k.scal, rank_deficient, n0 * sp.world, k.st);
      MgHalosT<double> h{2, {k.p[0], k.p[1]}};                                 // (the diagonals' halo rows: p must start from zero ones)
      mg_slab_zero_halos<double><<<grid_for(nx, kBlock, 64), kBlock, 0, s>>>(h, nx, n0);
    }
    // the sharded levels: halo rows of the diagonal (coarsening reads the neighbours' presence) and of dinv, once per solve
    for (int l = 0; l < sp.g; ++l) {
      PISO_TRY(link.exchange(R, [l](RK& k) { return k.lv[l].c[2]; }, sp.d.nx[l], sp.rows[l]));
      PISO_TRY(link.exchange(R, [l](RK& k) { return k.lv[l].dinv; }, sp.d.nx[l], sp.rows[l]));
      for (RK& k : R) Ops::coarsen_slab(k.lv[l], l + 1 < sp.g ? k.lv[l + 1] : k.chunk, geo(k, l), s);
    }
    // level g: the ranks' rows, all-gathered
    for (int a = 0; a < 6; ++a)
      PISO_TRY(link.allgather(R, [a](RK& k) { return a < 5 ? k.chunk.c[a] : k.chunk.dinv; },
                              [a, this](RK& k) { return a < 5 ? k.lv[sp.g].c[a] : k.lv[sp.g].dinv; }, (size_t)R[0].chunk.n));
    for (RK& k : R)
      for (int l = sp.g; l + 1 < sp.d.nlev; ++l) MgGridOps<C>::coarsen(k.lv[l], k.lv[l + 1], s);
    PISO_LAUNCH_CHECK();
    PISO_HIP_CHECK(hipMemcpyAsync(pinned, R[0].st, sizeof(MgState), hipMemcpyDeviceToHost, s));
    PISO_HIP_CHECK(hipStreamSynchronize(s));
    return mg_refusal(pinned->flags);
  }

  // halo rows of array `sel` of sharded level l
  template <typename Sel>
  int halo(int l, Sel sel) { return link.exchange(R, sel, sp.d.nx[l], sp.rows[l]); }

  // z = M^-1 r on every rank's rows: leaves R[q].z_top (halo rows filled) and the rank's part of (r, z) in g[0]
  // (the cycle reads r[l] on sharded levels: r[0] is the outer r itself under the fp64 cycle, fl32 of it under the float32 cycle)
  int cycle(int nu) {
    const int G = sp.g, nx = sp.d.nx[0], n0 = nx * sp.nyl;
    std::vector<std::vector<C*>> zc(nloc(), std::vector<C*>(kMgMaxLevels, nullptr));
    vec_mask = 0;
    for (int l = 0; l < G; ++l) {                                       // down the sharded levels
      const bool x4 = quads(R[0], l);
      if (x4) vec_mask |= 1 << l;
      if (nu >= 2) PISO_TRY(halo(l, [&](RK& k) { return k.r[l]; }));
      for (int q = 0; q < nloc(); ++q) {
        RK& k = R[q];
        zc[q][l] = k.z[l];
        Ops::pre(k.lv[l], k.r[l], k.z[l], k.st, geo(k, l), nu, x4, s);
      }
      for (int sw = 2; sw < nu; ++sw) {
        PISO_TRY(halo(l, [&](RK& k) { return zc[&k - R.data()][l]; }));
        for (int q = 0; q < nloc(); ++q) {
          RK& k = R[q];
          C* nxt = zc[q][l] == k.z[l] ? k.t[l] : k.z[l];
          Ops::jacobi(k.lv[l], k.r[l], zc[q][l], nxt, nullptr, 0, nullptr, k.st, geo(k, l), x4, nullptr, s);
          zc[q][l] = nxt;
        }
      }
      PISO_TRY(halo(l, [&](RK& k) { return zc[&k - R.data()][l]; }));
      for (int q = 0; q < nloc(); ++q) {
        RK& k = R[q];
        const Level& Cc = l + 1 < G ? k.lv[l + 1] : k.chunk;
        Ops::restrict_to(k.lv[l], k.r[l], zc[q][l], l + 1 < G ? k.r[l + 1] : k.rchunk, Cc.nx, Cc.ny, k.st, geo(k, l), x4, s);
      }
    }
    // level g: the ranks' rows of the residual, all-gathered; levels g .. coarsest on every rank, as the one-GPU plan runs them
    PISO_TRY(link.allgather(R, [G](RK& k) { return Ops::gather_src(k, G); }, [G](RK& k) { return k.r[G]; }, (size_t)R[0].chunk.n));
    std::vector<C*> zg(nloc());
    for (int q = 0; q < nloc(); ++q) zg[q] = mg_slab_replicated(sp, use_tail, vec, R[q], nu, &vec_mask, s);
    int n_rz = 0;
    if constexpr (Ops::kRunsG0) {
      if (G == 0) {
        n_rz = mg_grid(n0);
        for (int q = 0; q < nloc(); ++q) {
          RK& k = R[q];
          mg_slab_take_rows<<<mg_grid(n0 + 2 * nx), kBlock, 0, s>>>(zg[q], k.zo, nx, sp.nyl, k.rank * sp.nyl, sp.d.ny[0], per_y, k.st);
          mg_slab_dot<<<n_rz, kBlock, 0, s>>>(k.ro, k.zo, n0, k.part_rz, k.st);
          k.z_top = k.zo;
        }
      }
    }
    for (int l = G - 1; l >= 0; --l) {                                  // up the sharded levels
      const bool x4 = quads(R[0], l);
      if (l + 1 < G) PISO_TRY(halo(l + 1, [&](RK& k) { return zc[&k - R.data()][l + 1]; }));      // e of a sharded coarser level
      for (int sw = 0; sw < nu; ++sw) {
        if (sw > 0) PISO_TRY(halo(l, [&](RK& k) { return zc[&k - R.data()][l]; }));               // (sweep 0: filled before the restriction)
        for (int q = 0; q < nloc(); ++q) {
          RK& k = R[q];
          C* nxt = zc[q][l] == k.z[l] ? k.t[l] : k.z[l];
          const C* e = sw == 0 ? (l + 1 < G ? zc[q][l + 1] : zg[q]) : nullptr;
          const bool last = l == 0 && sw == nu - 1;
          const int gl = Ops::jacobi(k.lv[l], k.r[l], zc[q][l], nxt, e, sp.d.nx[l + 1], last ? k.part_rz : nullptr, k.st, geo(k, l), x4, last ? k.ro : nullptr, s);
          if (last) n_rz = gl;
          zc[q][l] = nxt;
        }
      }
      if (l == 0) {
        PISO_TRY(halo(0, [&](RK& k) { return zc[&k - R.data()][0]; }));                           // for the direction
        for (int q = 0; q < nloc(); ++q) R[q].z_top = zc[q][0];
      }
    }
    for (RK& k : R) mg_slab_collapse<<<1, kBlock, 0, s>>>(k.part_rz, n_rz, k.g, k.st);
    PISO_LAUNCH_CHECK();
    return PISO_OK;
  }

  int solve(float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps, int* iterations_out) {
    PISO_TRY(build(rank_deficient));
    MgState* pinned = nullptr;
    PISO_TRY(mg_pinned(&pinned));
    const int nx = sp.d.nx[0], n0 = nx * sp.nyl, g0 = mg_grid(n0);
    const int check_every = opt(OPT_MG_CHECK_EVERY) > 0 ? opt(OPT_MG_CHECK_EVERY) : kCheckEvery;
    auto L0 = [&](RK& k) { Lv L = Ops::outer(k, sp.g); L.nx = nx; L.ny = sp.nyl; L.n = n0; return L; };
    for (RK& k : R) Ops::init(L0(k), k, g0, s);
    bool done = false;
    int iterations = max_iterations;
    for (int it = 0; it < max_iterations && !done; ++it) {
      const bool restart = it > 0 && (it + 1) % residual_reset == 0;
      if (restart) {
        PISO_TRY(link.exchange(R, [](RK& k) { return k.x; }, nx, sp.nyl));
        for (RK& k : R) Ops::residual(L0(k), k, g0, geo(k, 0), s);
      }
      PISO_TRY(cycle(sweeps));
      PISO_TRY(link.allreduce(R, 0, 1));
      for (RK& k : R) Ops::direction(L0(k), k, g0, it, (restart || it == 0) ? 1 : 0, geo(k, 0), s);
      for (RK& k : R) mg_slab_collapse<<<1, kBlock, 0, s>>>(k.part_pq, g0, k.g + 1, k.st);
      PISO_TRY(link.allreduce(R, 1, 1));
      for (RK& k : R) {
        Ops::update(n0, k, g0, it, s);
        mg_slab_collapse_max<<<1, kBlock, 0, s>>>(k.part_max, g0, k.g + 2, k.st);
      }
      PISO_TRY(link.allgather(R, [](RK& k) { return k.g + 2; }, [](RK& k) { return k.gmax; }, 1));
      for (RK& k : R) mg_check<<<1, kBlock, 0, s>>>(k.gmax, sp.world, accuracy, it + 1, k.st);
      PISO_LAUNCH_CHECK();
      if ((it + 1) % check_every == 0 || it + 1 == max_iterations) {
        PISO_HIP_CHECK(hipMemcpyAsync(pinned, R[0].st, sizeof(MgState), hipMemcpyDeviceToHost, s));
        PISO_HIP_CHECK(hipStreamSynchronize(s));
        if (pinned->done) { done = true; iterations = pinned->iterations; }
      }
    }
    if (rank_deficient) {
      for (RK& k : R) {
        mg_sum_x<<<g0, kBlock, 0, s>>>(L0(k), k.x, k.parts);
        mg_slab_collapse<<<1, kBlock, 0, s>>>(k.parts, g0, k.g + 3, nullptr);
      }
      PISO_TRY(link.allreduce(R, 3, 1));
      for (RK& k : R) mg_finish<GeoSlab><<<g0, kBlock, 0, s>>>(L0(k), k.x, k.g + 3, 1, k.scal, geo(k, 0));
      PISO_LAUNCH_CHECK();
    }
    if (iterations_out) *iterations_out = iterations;
    record(sweeps, iterations, iterations, mg_recomputations(iterations, residual_reset));
    return PISO_OK;
  }

  void record(int sweeps, int iterations, int cycles, int recomputed) const {
    mg_record(sp.d.nlev, use_tail ? sp.tail_first : -1, sweeps, iterations, cycles, recomputed, (int)sizeof(C), vec_mask);
  }

  // copy rank-local results out and make every rank return the same status
  int finish(const char* who) {
    PISO_LAUNCH_CHECK();
    if (link.pc) return comm_agree(link.pc, who, s, opt(OPT_SLAB_FORCE) > 0);
    PISO_HIP_CHECK(hipStreamSynchronize(s));
    return PISO_OK;
  }
};
typedef MgSlabT<double> MgSlab;

// the plan of a call: refusals are the plan's, with its message; the float32 cycle refuses a plan that replicates the whole cycle (g = 0)
template <typename C>
static int mg_slab_begin(MgSlabT<C>& M, const char* who, int nx, int nyl, int world, int local_ranks, int per_x, int per_y, int sweeps, PisoComm* pc, hipStream_t s) {
  char msg[320];
  if (sweeps < 1 || sweeps > 8) { snprintf(msg, sizeof(msg), "%s: sweeps must be 1 .. 8", who); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (nyl < 1 || world < 1 || world > kMaxRanks) { snprintf(msg, sizeof(msg), "%s: needs 1 .. %d ranks with at least one row each", who, kMaxRanks); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  M.sp = mg_slab_plan(nx, nyl * world, world, opt(OPT_MG_SLAB_GATHER_CELLS));
  if (M.sp.status) { snprintf(msg, sizeof(msg), "%s: %s", who, M.sp.msg); set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  if (!MgSlabOps<C>::kRunsG0 && M.sp.g == 0) {
    snprintf(msg, sizeof(msg), "%s: the whole %d x %d grid is within the gather limit (g = 0), so the cycle is replicated and a float32 cycle has nothing to gain; "
             "a solve cut into y-slabs needs cycle_dtype=torch.float64 here", who, nx, nyl * world);
    set_error_msg(msg);
    return PISO_ERR_INVALID_ARG;
  }
  M.per_x = per_x ? 1 : 0; M.per_y = per_y ? 1 : 0; M.s = s;
  M.link = MgLink{pc, world, per_y != 0, s};
  M.use_tail = M.sp.tail_first >= 0 && opt(OPT_MG_TAIL) != 0;
  M.vec = opt(OPT_MG_F32_VEC) != 0;
  M.R.resize(local_ranks);
  return PISO_OK;
}

}  // namespace piso
