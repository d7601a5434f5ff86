// What a rank of the slab multigrid (mg_slab.h) holds and how its workspace is carved - pure host code, no HIP calls, like mg_slab_plan.h:
// a host compiler builds a driver over it (tests/mg_slab_carve_driver.cpp) that walks the carve against an arena without memory.
// C is the type of the cycle's values: double (the fp64 cycle) or float (the float32 cycle of mg_f32.h under the fp64 outer iteration).
#pragma once
#include <stddef.h>

#include "mg_slab_plan.h"

namespace piso {

constexpr int kMgGrid = 1024;          // grid cap of every kernel that publishes partials (4 workgroups per CU)
constexpr int kMgSlabG = 16;           // doubles of a rank's collective buffer: [0] (r, z), [1] (p, q), [2] max|r|, [3] sum(x), [4 .. 8] set-up
constexpr int kPlanMaxRanks = 8;       // kMaxRanks of peer.h (mg.hip holds the two equal)

struct MgState { int done, iterations, flags, pad; };
enum { SC_RZ0 = 0, SC_RZ1, SC_SUM_DIAG, SC_NPRESENT, SC_MEAN_B, SC_COUNT_MG = 8 };

struct Lv {
  int nx, ny, n, per_x, per_y;
  double* c[5];        // S, W, C, E, N
  double* dinv;        // kOmega / diag, 0 on absent cells
};
struct LvF {
  int nx, ny, n, per_x, per_y;
  float* c[5];         // S, W, C, E, N
  float* dinv;         // fl32(kOmega / diag), 0 on absent cells
};
template <typename C> struct MgLevelOf;
template <> struct MgLevelOf<double> { typedef Lv type; };
template <> struct MgLevelOf<float> { typedef LvF type; };

template <typename C>
struct MgSlabRankT {
  typedef typename MgLevelOf<C>::type Level;
  int rank;
  const double *Lin, *b;               // the rank's rows of the caller's matrix / right-hand side (b NULL: hierarchy or cycle only)
  Level lv[kPlanMaxLevels];            // l < g: the rank's rows (pointers at owned row 0, halo rows at -1 and ny); l >= g: the whole level
  C *r[kPlanMaxLevels], *z[kPlanMaxLevels], *t[kPlanMaxLevels];
  Level chunk;                         // the rank's rows of level g, before the gather
  C* rchunk;
  Lv L0;                               // float32 cycle: the fp64 level 0 of the outer iteration (the rank's rows, no halo rows)
  double* ro;                          // outer r: = r[0] where the fp64 level 0 is sharded; of its own at g = 0 (halo rows) and under the float32 cycle (none)
  C* zo;                               // g = 0: the rank's rows of z, with halo rows
  double *p[2], *x, *q;                // p, x with halo rows
  double *parts, *part_rz, *part_pq, *part_max, *scal, *gmax, *g;
  MgState* st;
  C* z_top;                            // where the last cycle left the rank's z (halo rows filled)
};

// one rank's share (the same walk sizes it against an arena without memory).  AR: Arena of piso_common.h, or the driver's.
// Every array starts on the arena's 256-byte boundary; the halo offset of a sharded level is nx values, so a float row stays 16-byte aligned
// where nx % 4 == 0 - the levels the four-cell kernels run on.
template <typename C, typename AR>
inline bool mg_slab_carve(const MgSlabPlan& sp, int per_x, int per_y, AR& ar, MgSlabRankT<C>& k) {
  const bool f32 = sizeof(C) == 4;
  const MgDims& d = sp.d;
  for (int l = 0; l < d.nlev; ++l) {
    typename MgSlabRankT<C>::Level& L = k.lv[l];
    const bool sharded = l < sp.g;
    L.nx = d.nx[l]; L.ny = sp.rows[l]; L.n = L.nx * L.ny; L.per_x = per_x; L.per_y = per_y;
    const size_t cells = sharded ? (size_t)L.n + 2 * L.nx : (size_t)L.n, off = sharded ? L.nx : 0;
    for (int s = 0; s < 5; ++s) L.c[s] = ar.template take<C>(cells) + off;
    L.dinv = ar.template take<C>(cells) + off;
    k.r[l] = ar.template take<C>(cells) + off; k.z[l] = ar.template take<C>(cells) + off; k.t[l] = ar.template take<C>(cells) + off;
  }
  const int nxg = d.nx[sp.g], rows_g = d.ny[sp.g] / sp.world;      // (ny_g = ny >> g exactly: nyl % 2^g == 0)
  k.chunk.nx = nxg; k.chunk.ny = rows_g; k.chunk.n = nxg * rows_g; k.chunk.per_x = per_x; k.chunk.per_y = per_y;
  for (int s = 0; s < 5; ++s) k.chunk.c[s] = ar.template take<C>(k.chunk.n);
  k.chunk.dinv = ar.template take<C>(k.chunk.n);
  k.rchunk = ar.template take<C>(k.chunk.n);
  const int nx = d.nx[0];
  const size_t n0 = (size_t)nx * sp.nyl, nh0 = n0 + 2 * nx;
  k.L0.nx = nx; k.L0.ny = sp.nyl; k.L0.n = (int)n0; k.L0.per_x = per_x; k.L0.per_y = per_y;
  for (int s = 0; s < 5; ++s) k.L0.c[s] = nullptr;
  k.L0.dinv = nullptr;
  k.zo = nullptr;
  if (f32) {
    for (int s = 0; s < 5; ++s) k.L0.c[s] = ar.template take<double>(n0);
    k.L0.dinv = ar.template take<double>(n0);
    k.ro = ar.template take<double>(n0);
  } else if (sp.g > 0) {
    k.ro = reinterpret_cast<double*>(k.r[0]);
  } else {
    k.ro = ar.template take<double>(nh0) + nx; k.zo = ar.template take<C>(nh0) + nx;
  }
  k.p[0] = ar.template take<double>(nh0) + nx; k.p[1] = ar.template take<double>(nh0) + nx; k.x = ar.template take<double>(nh0) + nx;
  k.q = ar.template take<double>(n0);
  k.parts = ar.template take<double>(4 * kMgGrid);
  k.part_rz = ar.template take<double>(kMgGrid); k.part_pq = ar.template take<double>(kMgGrid); k.part_max = ar.template take<double>(kMgGrid);
  k.scal = ar.template take<double>(SC_COUNT_MG);
  k.gmax = ar.template take<double>(kPlanMaxRanks);
  k.st = ar.template take<MgState>(1);
  k.z_top = nullptr;
  return ar.ok();
}

}  // namespace piso
