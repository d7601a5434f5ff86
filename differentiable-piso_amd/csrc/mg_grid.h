// The one-GPU host driver of the multigrid PCG (part of mg.hip's translation unit, after its kernels and those of mg_guess.h): ONE text over
// the type C of the cycle's values, as the slab driver MgSlabT<C> of mg_slab.h has it.  MgGridOps<C> names the kernels the driver launches,
// kernel<GeoWhole, C>; its four members that differ by type - how level 0 of the cycle comes out of the fp64 set-up, how one cycle reads r
// and writes z - are specialised (double: below; float: mg_f32.h).  MgGridT<C> holds the set-up, the first sweeps, the V-cycle, the PCG
// iteration and the single cycle on an MgPlanT<C> (mg_prepared_carve.h), whoever filled it: the ordinary entries from one workspace
// (below), the prepared entries from their two buffers (mg_prepared.h), the slab driver as a view of a rank's replicated levels (mg_slab.h).
#pragma once

namespace piso {

// ---- the launches of a level's cycle kernels that have a four-cell form, over the geometry G and the type C of the cycle's values ----------
// x4: the level runs the four-cell kernels of mg_quads.h (float only, nx % 4 == 0; the grid counts quads then).  rd: the outer residual in
// double, the float32 cycle's other factor of (r, z), given exactly where part_rz is - NULL: no partials.
template <typename C>
static bool mg_has_quads(const LvOf<C>& L) { return std::is_same<C, float>::value && (L.nx & 3) == 0; }
template <typename G, typename C>
static void mg_launch_pre2(const LvOf<C>& L, const C* r, C* z, const MgState* st, bool x4, const G& g, hipStream_t s) {
  if constexpr (std::is_same<C, float>::value) {
    if (x4) { mg_pre2_x4<G><<<mg_grid((L.nx >> 2) * L.ny), kBlock, 0, s>>>(L, r, z, st, g); return; }
  }
  mg_pre2<G, C><<<mg_grid(L.n), kBlock, 0, s>>>(L, r, z, st, g);
}
// one sweep; returns the number of (r, z) partials it left (part_rz given)
template <typename G, typename C>
static int mg_launch_jacobi(const LvOf<C>& L, const C* r, const C* zin, C* zout, const C* e, int nxc, double* part_rz, const MgState* st, bool x4, const double* rd,
                            const G& g, hipStream_t s) {
  const int gl = x4 ? mg_grid((L.nx >> 2) * L.ny) : mg_grid(L.n);
  if constexpr (std::is_same<C, float>::value) {
    if (x4) {
      if (e && rd) mg_jacobi_x4<G, true, true><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
      else if (e) mg_jacobi_x4<G, true, false><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
      else if (rd) mg_jacobi_x4<G, false, true><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
      else mg_jacobi_x4<G, false, false><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
      return gl;
    }
  }
  mg_jacobi<G, C><<<gl, kBlock, 0, s>>>(L, r, zin, zout, e, nxc, part_rz, st, rd, g);
  return gl;
}
template <typename G, typename C>
static void mg_launch_restrict(const LvOf<C>& L, const C* r, const C* z, C* rc, int nxc, int nyc, const MgState* st, bool x4, const G& g, hipStream_t s) {
  if constexpr (std::is_same<C, float>::value) {
    if (x4) { mg_restrict_x4<G><<<mg_grid((L.nx >> 2) * nyc), kBlock, 0, s>>>(L, r, z, rc, nxc, nyc, st, g); return; }
  }
  mg_restrict<G, C><<<mg_grid(nxc * nyc), kBlock, 0, s>>>(L, r, z, rc, nxc, nyc, st, g);
}

// ---- what the driver launches --------------------------------------------------------------------------------------------------------------
// (rc: what the cycle reads - fl32(r) beside r under the float32 cycle, r itself under the fp64 cycle, where the kernels leave it alone)
template <typename C>
struct MgGridOps {
  typedef LvOf<C> Level;
  typedef MgTailT<C> Tail;
  static bool quads(const Level& L) { return mg_has_quads<C>(L); }
  static void pre1(const Level& L, const C* r, C* z, const MgState* st, hipStream_t s) { mg_pre1<C><<<mg_grid(L.n), kBlock, 0, s>>>(L, r, z, st); }
  static void pre2(const Level& L, const C* r, C* z, const MgState* st, bool x4, hipStream_t s) { mg_launch_pre2<GeoWhole, C>(L, r, z, st, x4, GeoWhole{}, s); }
  static int jacobi(const Level& L, const C* r, const C* zin, C* zout, const C* e, int nxc, double* part_rz, const MgState* st, bool x4, const double* rd,
                    hipStream_t s) {
    return mg_launch_jacobi<GeoWhole, C>(L, r, zin, zout, e, nxc, part_rz, st, x4, rd, GeoWhole{}, s);
  }
  static void restrict_to(const Level& L, const C* r, const C* z, C* rc, const Level& Cc, const MgState* st, bool x4, hipStream_t s) {
    mg_launch_restrict<GeoWhole, C>(L, r, z, rc, Cc.nx, Cc.ny, st, x4, GeoWhole{}, s);
  }
  static void tail(const Tail& T, const C* r, C* z, double* part_rz, int nu, const MgState* st, const double* rd, hipStream_t s) {
    mg_tail<C><<<1, kTailThreads, 0, s>>>(T, r, z, part_rz, nu, st, rd);
  }
  static void coarsen(const Level& F, const Level& Cc, hipStream_t s) { mg_coarsen<GeoWhole, C><<<mg_grid(Cc.n), kBlock, 0, s>>>(F, Cc, GeoWhole{}); }
  static void export_level(const Level& L, double* out, hipStream_t s) { mg_export<C><<<mg_grid(L.n), kBlock, 0, s>>>(L, out); }
  // the outer iteration
  static void residual(const Lv& L0, const double* b, const double* x, double* r, const double* scal, const MgState* st, C* rc, int g0, hipStream_t s) {
    mg_residual<GeoWhole, C><<<g0, kBlock, 0, s>>>(L0, b, x, r, scal, st, rc, GeoWhole{});
  }
  static void direction(const Lv& L0, const C* z, const double* pold, double* pnew, double* q, const double* part_rz, int n_rz, double* scal, int k, int restart,
                        double* part_pq, const MgState* st, int g0, hipStream_t s) {
    mg_direction<GeoWhole, C><<<g0, kBlock, 0, s>>>(L0, z, pold, pnew, q, part_rz, n_rz, scal, k, restart, part_pq, st, GeoWhole{});
  }
  static void update(int n, double* x, double* r, const double* p, const double* q, const double* scal, int k, const double* part_pq, int n_pq, double* part_max,
                     const MgState* st, C* rc, int g0, hipStream_t s) {
    mg_update<C><<<g0, kBlock, 0, s>>>(n, x, r, p, q, scal, k, part_pq, n_pq, part_max, st, rc);
  }
  // by type: level 0 of the cycle from the fp64 set-up's; how a cycle on its own reads the caller's r, which double factor its (r, z) has,
  // how z goes out
  static void level0(const Lv& D, const Level& F, hipStream_t s);
  static const C* load_r(int n, const double* r_in, C* r0, hipStream_t s);
  static const double* own_rd(const C* r);
  static int store_z(int n, const C* z, double* z_out, hipStream_t s);
};
// the fp64 cycle: the set-up writes lv[0] itself; a cycle on its own reads the caller's r where it lies, which is also the double factor of
// (r, z); z is copied out
template <> inline void MgGridOps<double>::level0(const Lv&, const Lv&, hipStream_t) {}
template <> inline const double* MgGridOps<double>::load_r(int, const double* r_in, double*, hipStream_t) { return r_in; }
template <> inline const double* MgGridOps<double>::own_rd(const double* r) { return r; }
template <> inline int MgGridOps<double>::store_z(int n, const double* z, double* z_out, hipStream_t s) {
  PISO_HIP_CHECK(hipMemcpyAsync(z_out, z, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PISO_OK;
}

// a regular look at the state; a prepared solve's header mismatch is reported here
static int mg_look(MgState* pinned, const MgState* st, hipStream_t stream) {
  PISO_HIP_CHECK(hipMemcpyAsync(pinned, st, sizeof(MgState), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  if (pinned->flags & MG_FLAG_NOT_PREPARED) { set_error_msg("piso_mg: not a hierarchy prepared for this grid"); return PISO_ERR_INVALID_ARG; }
  return PISO_OK;
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------------
template <typename C>
struct MgGridT {
  typedef MgGridOps<C> Ops;
  typedef typename MgLevelOf<C>::type Level;
  const MgPlanT<C>& P;
  int nu;
  bool use_tail, vec;
  hipStream_t s;
  int vec_mask = 0;

  MgGridT(const MgPlanT<C>& plan, int sweeps, bool tail, bool vec4, hipStream_t stream) : P(plan), nu(sweeps), use_tail(tail), vec(vec4), s(stream) {}
  MgGridT(const MgPlanT<C>& plan, int sweeps, hipStream_t stream)
      : MgGridT(plan, sweeps, plan.H.tail_first >= 0 && opt(OPT_MG_TAIL) != 0, opt(OPT_MG_F32_VEC) != 0, stream) {}

  // builds every level from the caller's matrix and refuses what the solver does not solve (one host look, as the plain CG's set-up has)
  int build(const double* laplace, const double* b, int rank_deficient) const {
    const MgHierT<C>& H = P.H;
    PISO_TRY(mg_build_begin(H.L0, laplace, b, rank_deficient, P.S.parts, H.scal, P.S.st, s));
    Ops::level0(H.L0, H.lv[0], s);
    for (int l = 0; l + 1 < H.nlev; ++l) Ops::coarsen(H.lv[l], H.lv[l + 1], s);
    PISO_LAUNCH_CHECK();
    return mg_build_end(P.S.st, s);
  }

  bool quads(int l) const { return vec && Ops::quads(P.H.lv[l]); }
  C* other(int l, const C* cur) const { return cur == P.S.z[l] ? P.S.t[l] : P.S.z[l]; }
  // `sweeps` sweeps from a zero guess on level l; returns where the result is
  C* first_sweeps(int l, bool x4, const C* r, int sweeps) const {
    const Level& L = P.H.lv[l];
    C* cur = P.S.z[l];
    if (sweeps >= 2) Ops::pre2(L, r, cur, P.S.st, x4, s); else Ops::pre1(L, r, cur, P.S.st, s);
    for (int sw = 2; sw < sweeps; ++sw) {
      C* nxt = other(l, cur);
      Ops::jacobi(L, r, cur, nxt, nullptr, 0, nullptr, P.S.st, x4, nullptr, s);
      cur = nxt;
    }
    return cur;
  }
  // z = M^-1 r0: returns where z of level l0 is.  rd: the outer residual in double - the last kernel leaves the partials of (rd, z) in
  // part_rz (*n_rz of them); NULL: none.  l0: the level r0 lives on - 0, or the first replicated level of a slab solve, which runs levels
  // l0 .. coarsest exactly like this
  C* cycle(const C* r0, const double* rd, int* n_rz, int l0 = 0) {
    const MgHierT<C>& H = P.H;
    const MgScratchT<C>& S = P.S;
    const int end = use_tail ? H.tail_first : H.nlev - 1;      // levels [l0, end) have a coarser level and run as kernels of their own
    C* zc[kMgMaxLevels];
    vec_mask = 0;
    for (int l = l0; l < end; ++l) {
      const C* r = l == l0 ? r0 : S.r[l];
      const bool x4 = quads(l);
      if (x4) vec_mask |= 1 << l;
      zc[l] = first_sweeps(l, x4, r, nu);
      Ops::restrict_to(H.lv[l], r, zc[l], S.r[l + 1], H.lv[l + 1], S.st, x4, s);
    }
    const C* rend = end == l0 ? r0 : S.r[end];
    const double* rd_end = end == l0 ? rd : nullptr;
    if (use_tail) {
      typename Ops::Tail T;
      T.nlev = H.nlev - end;
      int off = 0;
      for (int k = 0; k < T.nlev; ++k) { T.lv[k] = H.lv[end + k]; T.off[k] = off; off += T.lv[k].n; }
      Ops::tail(T, rend, S.z[end], rd_end ? S.part_rz : nullptr, nu, S.st, rd_end, s);
      zc[end] = S.z[end];
      *n_rz = 1;
    } else {
      C* cur = first_sweeps(end, false, rend, kCoarsestSweeps - 1);
      zc[end] = other(end, cur);
      *n_rz = Ops::jacobi(H.lv[end], rend, cur, zc[end], nullptr, 0, rd_end ? S.part_rz : nullptr, S.st, false, rd_end, s);
    }
    for (int l = end - 1; l >= l0; --l) {
      const C* r = l == l0 ? r0 : S.r[l];
      const bool x4 = quads(l);
      C* cur = zc[l];
      for (int sw = 0; sw < nu; ++sw) {
        C* nxt = other(l, cur);
        const C* e = sw == 0 ? zc[l + 1] : nullptr;
        const double* rd_l = (l == l0 && sw == nu - 1) ? rd : nullptr;
        const int g = Ops::jacobi(H.lv[l], r, cur, nxt, e, e ? H.lv[l + 1].nx : 0, rd_l ? S.part_rz : nullptr, S.st, x4, rd_l, s);
        if (l == l0) *n_rz = g;
        cur = nxt;
      }
      zc[l] = cur;
    }
    return zc[l0];
  }
  void record(int iterations, int cycles, int recomputed) const {
    mg_record(P.H.nlev, use_tail ? P.H.tail_first : -1, nu, iterations, cycles, recomputed, (int)sizeof(C), vec_mask);
  }

  // the PCG iteration on a plan whose hierarchy is built (ordinary entries: by build; prepared ones: by an earlier prepare)
  int pcg(const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int* iterations_out,
          const double* x0) {
    MgState* pinned = nullptr;
    if (int rc = mg_pinned(&pinned)) return rc;
    const Lv& L0 = P.H.L0;
    const MgScratchT<C>& S = P.S;
    const int n = L0.n, g0 = mg_grid(n);
    const int check_every = opt(OPT_MG_CHECK_EVERY) > 0 ? opt(OPT_MG_CHECK_EVERY) : kCheckEvery;
    double* r = S.r64;
    C* rc = S.r[0];                                             // what the cycle reads: fl32(r) beside r, or r itself
    mg_start(L0, divergence, x0, x_out, r, rc, S.scal, S.parts, S.part_max, accuracy, S.st, s);
    bool done = false;
    int iterations = max_iterations;
    for (int k = 0; k < max_iterations && !done; ++k) {
      const bool restart = k > 0 && (k + 1) % residual_reset == 0;
      if (restart) Ops::residual(L0, divergence, x_out, r, S.scal, S.st, rc, g0, s);
      int n_rz = 0;
      const C* z = cycle(rc, r, &n_rz);
      Ops::direction(L0, z, S.p[k & 1], S.p[(k + 1) & 1], S.q, S.part_rz, n_rz, S.scal, k, (restart || k == 0) ? 1 : 0, S.part_pq, S.st, g0, s);
      Ops::update(n, x_out, r, S.p[(k + 1) & 1], S.q, S.scal, k, S.part_pq, g0, S.part_max, S.st, rc, g0, s);
      mg_check<<<1, kBlock, 0, s>>>(S.part_max, g0, accuracy, k + 1, S.st);
      PISO_LAUNCH_CHECK();
      if ((k + 1) % check_every == 0 || k + 1 == max_iterations) {
        PISO_TRY(mg_look(pinned, S.st, s));
        if (pinned->done) { done = true; iterations = pinned->iterations; }
      }
    }
    if (rank_deficient) {
      mg_sum_x<<<g0, kBlock, 0, s>>>(L0, x_out, S.parts);
      mg_finish<GeoWhole><<<g0, kBlock, 0, s>>>(L0, x_out, S.parts, g0, S.scal, GeoWhole{});
      PISO_LAUNCH_CHECK();
    }
    PISO_HIP_CHECK(hipStreamSynchronize(s));
    if (iterations_out) *iterations_out = iterations;
    mg_guess_record(x0, pinned);
    record(iterations, iterations, mg_recomputations(iterations, residual_reset));
    return PISO_OK;
  }
  // one cycle; `prepared`: the call's only look at the state (the header's verdict) replaces the plain wait
  int vcycle(const double* r_in, double* z_out, bool prepared) {
    const int n = P.H.L0.n;
    const C* r0 = Ops::load_r(n, r_in, P.S.r[0], s);
    int n_rz = 0;
    const C* z = cycle(r0, Ops::own_rd(r0), &n_rz);
    PISO_LAUNCH_CHECK();
    PISO_TRY(Ops::store_z(n, z, z_out, s));
    PISO_LAUNCH_CHECK();
    if (prepared) {
      MgState* pinned = nullptr;
      if (int rc = mg_pinned(&pinned)) return rc;
      PISO_TRY(mg_look(pinned, P.S.st, s));
    } else {
      PISO_HIP_CHECK(hipStreamSynchronize(s));
    }
    record(0, 1, 0);
    return PISO_OK;
  }
};

// ---- the ordinary entries, once over the type of the cycle's values ----------------------------------------------------------------------------
template <typename C>
static int mg_carve(const char* who, int nx, int ny, int periodic_x, int periodic_y, void* workspace, size_t workspace_bytes, MgPlanT<C>& P) {
  Arena ar(workspace, workspace_bytes);
  if (mg_plan_carve(nx, ny, periodic_x ? 1 : 0, periodic_y ? 1 : 0, ar, P)) return PISO_OK;
  char msg[96];
  snprintf(msg, sizeof(msg), "%s: workspace too small", who);
  set_error_msg(msg);
  return PISO_ERR_INVALID_ARG;
}
// the solve, with and without a guess (x0 NULL: none)
template <typename C>
static int mg_solve_entry(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, double* x_out, float accuracy,
                          int max_iterations, int rank_deficient, int residual_reset, int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes,
                          piso_stream_t stream, const double* x0) {
  const OptScope knobs;
  tl_mg_last_guess = 0;                                       // (until the solve returns: a refused call reports no guess)
  PISO_TRY(mg_common_args("piso_mg_pcg_solve", nx, ny, laplace, divergence, x_out, workspace, sweeps));
  PISO_TRY(mg_iteration_args("piso_mg_pcg_solve", max_iterations, residual_reset));
  MgPlanT<C> P;
  PISO_TRY(mg_carve("piso_mg_pcg_solve", nx, ny, periodic_x, periodic_y, workspace, workspace_bytes, P));
  MgGridT<C> G(P, sweeps, static_cast<hipStream_t>(stream));
  PISO_TRY(G.build(laplace, divergence, rank_deficient ? 1 : 0));
  return G.pcg(divergence, x_out, accuracy, max_iterations, rank_deficient ? 1 : 0, residual_reset, iterations_out, x0);
}
template <typename C>
static int mg_vcycle_entry(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out, int sweeps, void* workspace,
                           size_t workspace_bytes, piso_stream_t stream) {
  const OptScope knobs;
  PISO_TRY(mg_common_args("piso_mg_vcycle", nx, ny, laplace, r_in, z_out, workspace, sweeps));
  MgPlanT<C> P;
  PISO_TRY(mg_carve("piso_mg_vcycle", nx, ny, periodic_x, periodic_y, workspace, workspace_bytes, P));
  MgGridT<C> G(P, sweeps, static_cast<hipStream_t>(stream));
  PISO_TRY(G.build(laplace, nullptr, 0));
  return G.vcycle(r_in, z_out, false);
}
// a level as [nx_out * ny_out][5] (laplace_level_out NULL: sizes only)
template <typename C>
static int mg_level_entry(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out, int* ny_out, double* laplace_level_out,
                          void* workspace, size_t workspace_bytes, piso_stream_t stream_) {
  const OptScope knobs;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PISO_TRY(mg_common_args("piso_mg_level", nx, ny, laplace, nx_out, ny_out, workspace, 1));
  MgPlanT<C> P;
  PISO_TRY(mg_carve("piso_mg_level", nx, ny, periodic_x, periodic_y, workspace, workspace_bytes, P));
  if (level < 0 || level >= P.H.nlev) { *nx_out = 0; *ny_out = 0; set_error_msg("piso_mg_level: no such level"); return PISO_ERR_INVALID_ARG; }
  *nx_out = P.H.lv[level].nx; *ny_out = P.H.lv[level].ny;
  if (!laplace_level_out) return PISO_OK;
  PISO_TRY(MgGridT<C>(P, 1, stream).build(laplace, nullptr, 0));
  MgGridOps<C>::export_level(P.H.lv[level], laplace_level_out, stream);
  PISO_LAUNCH_CHECK();
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  return PISO_OK;
}

}  // namespace piso
