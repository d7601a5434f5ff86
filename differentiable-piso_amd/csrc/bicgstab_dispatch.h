// Host side of the ILU(0)-BiCGStab's kernel choice (bicgstab.hip): the geometry of the two face arrays, the plan of a solve (bi_plan:
// pure, no HIP calls - band height, row and band ranges, E, LDS forms, grids, first host look, folding, every shape it refuses),
// WHICH (T, E) have LDS-staged forms of bi_sweep / bi_factor (bi_lds_instance: the one statement of it) and the E ladder (bi_with_E: the
// only place that spells it).  Plain C++: a host compiler can include this file and walk every plan without a card.
#pragma once
#include <stddef.h>

#include <type_traits>

#include "../../include/piso_hip.h"

#if defined(__HIPCC__)
#define PISO_BI_HD __host__ __device__
#else
#define PISO_BI_HD
#endif

namespace piso {

constexpr int kBiBlock = 256;     // threads of a workgroup (piso_common.h: kBlock; bicgstab.hip holds the two equal)
constexpr int kBiParts = 1024;    // max blocks per component of a partial-producing kernel
// Slab mode splits a product into interior rows and kEdgeRows face rows at either end of the slab (bi_spmv)
constexpr int kEdgeRows = 2;

struct Geo {
  int nx, ny;
  int W[2], H[2], n[2], r0[2];    // face-array dims, rows, row offset of each component in the concatenated vectors
  int xw[2], yw[2];               // periodic wrap distances in x / y (skip the duplicate face in the own direction)
  int F[2], f0[2];                // frame rows (within 2 of a border) and their offset in the exception tables
  int R, nb[2];                   // band height (face rows) and number of bands
};

PISO_BI_HD inline int frame_rows(int W, int H) {
  const int wi = W > 4 ? W - 4 : 0, hi = H > 4 ? H - 4 : 0;
  return W * H - wi * hi;
}

// the part of the geometry that no band height enters: dims, wrap distances, frame rows, offsets (R = 0: no bands yet)
inline Geo make_geo(int nx, int ny) {
  Geo g;
  g.nx = nx; g.ny = ny;
  g.W[0] = nx + 1; g.H[0] = ny; g.W[1] = nx; g.H[1] = ny + 1;
  for (int c = 0; c < 2; ++c) {
    g.n[c] = g.W[c] * g.H[c];
    g.xw[c] = g.W[c] - 1 - (c == 0);
    g.yw[c] = g.W[c] * (g.H[c] - 1 - (c == 1));
    g.F[c] = frame_rows(g.W[c], g.H[c]);
  }
  g.r0[0] = 0; g.r0[1] = g.n[0];
  g.f0[0] = 0; g.f0[1] = g.F[0];
  g.R = 0; g.nb[0] = g.nb[1] = 0;
  return g;
}
// ... and the bands: band_rows < 0 one band, 0 automatic, > 0 as given; clamped to ny + 1
inline Geo with_bands(Geo g, int band_rows) {
  const int ny = g.ny;
  int R = band_rows;
  if (R < 0) R = (ny + 1);                                   // one band: global structured ILU(0)
  // automatic (2048^2: 8 rows).  The rows of a band are sequential and a band is one workgroup: 2048^2 has 257 bands of 16 rows = ONE workgroup
  // of four waves per CU, and a sweep is then bound by the latency of its row chain (75 / 100 us); 513 bands of 8 rows keep two
  // workgroups per CU busy and halve the chain - 591 instead of 713 us per iteration, the SAME iteration counts (the matrices are
  // strongly diagonally dominant: 3 iterations to 1e-6, 5 to 1e-9 with bands of 4 .. 32 rows; a round-4 A/B script, results in profiles/README.md).  Bands of 4
  // rows gain nothing more at 2048^2 (the sweeps then move ~6 TB/s) and cost an iteration at 256^2.
  // Round 5: smaller grids get lower bands by the same argument - a band is one workgroup, and two components x ny / R bands should be
  // about two workgroups per CU: ny >= 2048: 8 rows, >= 1024: 4, >= 256: 2.  Measured (round 5, solve to 1e-6, same
  // iteration counts): 1024^2 0.833 -> 0.767 ms, 512^2 0.519 -> 0.429, 256^2 0.440 -> 0.366.
  // (grids of fewer than 256 rows - the lid-driven cavity - keep 8: nothing there is bound by the bands' parallelism, and at the
  // reference script's loose 1e-3 the preconditioner decides which iterate inside the tolerance a solve stops at)
  if (R == 0) R = ny >= 2048 ? 8 : (ny >= 1024 ? 4 : (ny >= 256 ? 2 : 8));
  if (R > ny + 1) R = ny + 1;
  g.R = R;
  for (int c = 0; c < 2; ++c) g.nb[c] = (g.H[c] + R - 1) / R;
  return g;
}

// ---- E: row elements per thread of the factorisation and the sweeps, the smallest of the ladder with nx + 1 <= 256 E
// (3, 5, 9: W = nx + 1 with nx a power of two is 2^k / 256 + 1 blocks wide).  bi_with_E calls f(std::integral_constant<int, E>) for a
// value of the ladder; false - and no call - for anything else.
constexpr int kBiLadder[] = {1, 2, 3, 4, 5, 8, 9, 16, 32};
constexpr int bi_pick_E(int need) {
  for (int e : kBiLadder) if (need <= e) return e;
  return 0;                                                  // (rows of more than 32 * 256 faces: bi_plan refuses them)
}
template <typename F>
inline bool bi_with_E(int E, F&& f) {
  switch (E) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 9: f(std::integral_constant<int, 9>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}); return true;
  }
  return false;
}

// ---- which (sizeof T, E) have bi_sweep<T, E, FWD, LDS = true> / bi_factor<T, E, LDS = true> instances: `rows` staged rows of E * 256 + E * 8 elements
// in 96 KB.  The planner asks at run time, the launchers at compile time; nothing else states it.
// (rows of up to 1 024 faces - E <= 4 - are no faster this way: 512^2 89.6 against 97.1 us per iteration, 1024^2 166.0 against 160.9)
constexpr bool bi_lds_rows_fit(size_t elem, int E, int rows) { return (size_t)rows * (E * kBiBlock + E * 8) * elem <= (size_t)96 * 1024; }
constexpr bool bi_lds_instance(size_t elem, int E) { return E >= 5 && bi_lds_rows_fit(elem, E, 4); }
// The sweeps stage four rows, the factorisation five.  Every pair of the ladder that has the four has room for the five as well
// (float E = 5, 8, 9, 16; double E = 5, 8, 9), so ONE predicate serves both kernels and factor_lds == sweep_lds in every plan.
constexpr bool bi_factor_fits_wherever_the_sweeps_do() {
  for (int e : kBiLadder)
    for (size_t elem : {sizeof(float), sizeof(double)})
      if (bi_lds_instance(elem, e) && !bi_lds_rows_fit(elem, e, 5)) return false;
  return true;
}
static_assert(bi_factor_fits_wherever_the_sweeps_do(), "the staged bi_factor holds five rows: an E whose sweeps fit and whose factorisation does not needs a predicate of its own");

// ---- the plan: everything the driver needs to know before it binds a workspace, creates a stream or launches
struct BiQuery {
  int nx, ny, band_rows;
  size_t elem;                       // sizeof(T)
  int transpose;                     // the call's flags (bit 0 A^T, bit 1 negated values)
  size_t ntot;                       // elements of a vector as stored: the whole grid's face rows, or the rank's stored rows (RowMap)
  int bicg_fold, bicg_sweep_lds, bicg_fuse_p, slab_force;   // option values (-1: not set)
  // the communicator of a slab call (comm = false: one GPU, the rest means nothing)
  bool comm, rccl;                   // rccl: halo rows by send / recv, sums by all-reduce (slab_comm.h); else peer mailboxes
  int world, rank;
  size_t row_cap;
  const piso_slab_t* slab_rows;      // local storage (the slab-decomposed step): the rows the caller says it holds, else NULL
};
struct BiPlan {
  int status = PISO_OK;              // != PISO_OK: the shape is refused with `msg`, nothing else of the plan is to be used
  const char* msg = nullptr;
  Geo g;
  // the rows [rb, re) and the bands [bb, be) of each component this rank works on (one GPU: everything)
  int rb[2], re[2], bb[2], be[2];
  int nyl = 0, jb = 0; bool last = true;       // the rank's cell rows [jb, jb + nyl); last: it also owns the duplicate face row v[ny]
  int E = 0; bool sweep_lds = false, factor_lds = false;
  // blocks per component: gv of the vector kernels' own rows, ge of a slab's edge rows, nparts = gv + ge partial records
  int gv = 0, ge = 0, nparts = 0;
  int grid_v = 0, grid_vs = 0, grid_e = 0, grid_b = 0;      // gridDim.x (y = 2 components) of: vector kernels, interior product, edge product, bands
  int look0 = 0;                     // iterations before the first host look
  bool fold_ok = false; int fuse_p = 0;
  bool slab = false, rccl = false;
  int transpose = 0;
};

inline BiPlan bi_plan(const BiQuery& q) {
  BiPlan p;
  const auto refuse = [&p](const char* msg) { p.status = PISO_ERR_INVALID_ARG; p.msg = msg; return p; };
  p.g = with_bands(make_geo(q.nx, q.ny), q.band_rows);
  const Geo& g = p.g;
  const int nx = q.nx, ny = q.ny;
  for (int c = 0; c < 2; ++c) { p.rb[c] = 0; p.re[c] = g.n[c]; p.bb[c] = 0; p.be[c] = g.nb[c]; }
  p.nyl = ny;
  p.slab = q.comm && (q.world > 1 || q.slab_force > 0);     // (slab_force: test knob - one rank, a ring with itself)
  p.rccl = q.comm && q.rccl;
  p.transpose = q.transpose & 3;
  if (q.comm) {
    const int world = q.world, rank = q.rank;
    // (a product is split into interior rows and kEdgeRows face rows at either end of the slab: thinner slabs would make the two
    // edge ranges overlap and count their rows twice in the dot products)
    if (ny % world != 0 || (ny / world) % g.R != 0 || ny / world < 2 * kEdgeRows)
      return refuse("piso_multi_bicgstab_ilu_slab: the slabs (ny / ranks cell rows) must be whole preconditioner bands of at least 4 rows");
    if (!p.rccl && (size_t)(3 * nx + 1) > q.row_cap) return refuse("piso_multi_bicgstab_ilu_slab: communicator row_capacity < 3 nx + 1");
    const int nyl = ny / world, jb = rank * nyl;
    const bool last = rank == world - 1;
    if (q.slab_rows && (q.slab_rows->row_begin != jb || q.slab_rows->row_end != jb + nyl || (q.slab_rows->owns_last_face_row != 0) != last))
      return refuse("piso_multi_bicgstab_ilu_slab: the slab does not match the communicator's rank");
    p.nyl = nyl; p.jb = jb; p.last = last;
    p.rb[0] = jb * g.W[0]; p.re[0] = (jb + nyl) * g.W[0];
    p.rb[1] = jb * g.W[1]; p.re[1] = (jb + nyl + (last ? 1 : 0)) * g.W[1];      // (the duplicate face row v[ny] lives on the last slab)
    p.bb[0] = p.bb[1] = jb / g.R;
    p.be[0] = (jb + nyl) / g.R;
    p.be[1] = last ? g.nb[1] : (jb + nyl) / g.R;
  }
  const int need = (nx + 1 + kBiBlock - 1) / kBiBlock;       // blocks' worth of elements in the longer face row (u: nx + 1)
  p.E = bi_pick_E(need);
  if (!p.E) return refuse("piso_multi_bicgstab_ilu: nx > 8191 not supported");
  p.sweep_lds = p.factor_lds = bi_lds_instance(q.elem, p.E) && q.bicg_sweep_lds != 0;

  const int own0 = p.re[0] - p.rb[0], own1 = p.re[1] - p.rb[1];
  const int nmax = own0 > own1 ? own0 : own1;
  int gv = (nmax + kBiBlock * 4 - 1) / (kBiBlock * 4);
  gv = (gv + 7) & ~7;                                       // (a multiple of the XCD count: stencil_rows deals the rows by XCD)
  if (gv > kBiParts) gv = kBiParts;
  if (gv < 1) gv = 1;
  // slab mode: a product is two launches (interior, edge rows) that write the partial slots [0, gv) and [gv, gv + ge); every other
  // kernel runs gv + ge blocks so that it rewrites ALL slots the scalar kernels add up
  int ge = 0;
  if (p.slab) {
    ge = (2 * kEdgeRows * g.W[0] + kBiBlock * 4 - 1) / (kBiBlock * 4);
    if (gv + ge > kBiParts) gv = kBiParts - ge;
  }
  p.gv = gv; p.ge = ge; p.nparts = gv + ge;
  p.grid_v = gv + ge; p.grid_vs = gv; p.grid_e = ge > 0 ? ge : 1;
  const int nb0 = p.be[0] - p.bb[0], nb1 = p.be[1] - p.bb[1];
  p.grid_b = nb0 > nb1 ? nb0 : nb1;                         // a band is one workgroup
  p.look0 = q.ntot < 32768 ? 1 : 2;                         // first host look (tiny systems - the lid-driven cavity converges in one iteration: a second one is 13 launches for nothing)
  // Scalar stages folded into their consumers (folded_scalars) on one GPU: 14 -> 9 launches per iteration.  Every block of a vector
  // kernel re-reads the partial records in passing (<= 16 KB, L2-resident); at 2048^2 the five launches saved are worth 2.5 % of the
  // iteration (606 -> 590 us, round 5), more on smaller grids.  Option bicg_fold: 0 never.
  p.fold_ok = !p.slab && q.bicg_fold != 0;
  // p = r + beta (p - omega v) inside the forward sweep of p_hat (BiArgs::fuse_p): 9 -> 8 launches per iteration.  Option bicg_fuse_p 0: never.
  p.fuse_p = q.bicg_fuse_p != 0;
  return p;
}

}  // namespace piso
