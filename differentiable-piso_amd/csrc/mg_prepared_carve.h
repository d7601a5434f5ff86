// The two buffers of a PREPARED multigrid solve (mg_prepared.h) and how they are carved - pure host code, no HIP calls, like mg_slab_carve.h:
// a host compiler builds a driver over it (tests/mg_prepared_carve_driver.cpp) that walks both carves against arenas without memory.
//   hierarchy  everything that depends on the matrix only, owned by the caller and kept between solves: a header, SC_SUM_DIAG / SC_NPRESENT,
//              the five coefficient arrays and dinv of every level (float32 cycle: the fp64 level 0 of the outer iteration AND the float32 levels)
//   scratch    what one solve writes: r, z, t of every level, p, q, the partials, `scal`, MgState (float32 cycle: the fp64 r beside fl32(r))
// C is the type of the cycle's values, as in mg_slab_carve.h.
#pragma once
#include <stddef.h>

#include "mg_slab_carve.h"

namespace piso {

constexpr unsigned kMgHierMagic = 0x3148474du;      // "MGH1"
// written by the last kernel of a successful prepare, compared by the first kernel of every solve / cycle on the buffer
struct MgHierHeader { unsigned magic; int nx, ny, per_x, per_y, cycle_elem, rank_deficient, pad; };

template <typename C>
struct MgHierT {
  typedef typename MgLevelOf<C>::type Level;
  int nlev, tail_first;
  MgHierHeader* hdr;
  double* scal;                        // SC_COUNT_MG slots; SC_SUM_DIAG and SC_NPRESENT are what a solve copies out
  Lv L0;                               // the fp64 level 0 of the outer iteration (fp64 cycle: the arrays of lv[0])
  Level lv[kPlanMaxLevels];
};
template <typename C>
struct MgScratchT {
  C *r[kPlanMaxLevels], *z[kPlanMaxLevels], *t[kPlanMaxLevels];
  double* r64;                         // the outer r (fp64 cycle: r[0])
  double *p[2], *q, *parts, *part_rz, *part_pq, *part_max, *scal;
  MgState* st;
};

inline bool mg_prepared_dims_ok(int nx, int ny) { return nx >= kPlanMinDim && ny >= kPlanMinDim && (long long)nx * ny <= (1ll << 30); }

inline void mg_hier_level0(MgHierT<double>& H) { H.L0 = H.lv[0]; }
inline void mg_hier_level0(MgHierT<float>&) {}
inline void mg_scratch_outer_r(MgScratchT<double>& S) { S.r64 = S.r[0]; }
inline void mg_scratch_outer_r(MgScratchT<float>&) {}

// AR: Arena of piso_common.h, or the driver's.  Every array starts on the arena's 256-byte boundary, so a float row stays 16-byte aligned where
// nx % 4 == 0 - the levels the four-cell kernels run on.
template <typename C, typename AR>
inline bool mg_hier_carve(int nx, int ny, int per_x, int per_y, AR& ar, MgHierT<C>& H) {
  const MgDims d = mg_dims(nx, ny);
  H.nlev = d.nlev; H.tail_first = d.tail_first;
  H.hdr = ar.template take<MgHierHeader>(1);
  H.scal = ar.template take<double>(SC_COUNT_MG);
  if (sizeof(C) == 4) {
    Lv& D = H.L0;
    D.nx = d.nx[0]; D.ny = d.ny[0]; D.n = D.nx * D.ny; D.per_x = per_x; D.per_y = per_y;
    for (int s = 0; s < 5; ++s) D.c[s] = ar.template take<double>(D.n);
    D.dinv = ar.template take<double>(D.n);
  }
  for (int l = 0; l < d.nlev; ++l) {
    typename MgHierT<C>::Level& L = H.lv[l];
    L.nx = d.nx[l]; L.ny = d.ny[l]; L.n = L.nx * L.ny; L.per_x = per_x; L.per_y = per_y;
    for (int s = 0; s < 5; ++s) L.c[s] = ar.template take<C>(L.n);
    L.dinv = ar.template take<C>(L.n);
  }
  mg_hier_level0(H);
  return ar.ok();
}
template <typename C, typename AR>
inline bool mg_scratch_carve(int nx, int ny, AR& ar, MgScratchT<C>& S) {
  const MgDims d = mg_dims(nx, ny);
  for (int l = 0; l < d.nlev; ++l) {
    const size_t n = (size_t)d.nx[l] * d.ny[l];
    S.r[l] = ar.template take<C>(n); S.z[l] = ar.template take<C>(n); S.t[l] = ar.template take<C>(n);
  }
  const size_t n0 = (size_t)d.nx[0] * d.ny[0];
  if (sizeof(C) == 4) S.r64 = ar.template take<double>(n0);
  mg_scratch_outer_r(S);
  S.p[0] = ar.template take<double>(n0); S.p[1] = ar.template take<double>(n0); S.q = ar.template take<double>(n0);
  S.parts = ar.template take<double>(4 * kMgGrid);
  S.part_rz = ar.template take<double>(kMgGrid); S.part_pq = ar.template take<double>(kMgGrid); S.part_max = ar.template take<double>(kMgGrid);
  S.scal = ar.template take<double>(SC_COUNT_MG);
  S.st = ar.template take<MgState>(1);
  return ar.ok();
}

// the sizes the two carves need (0: not a grid the solver takes, or not a cycle precision)
struct CountingArena {
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    used = (used + 255) / 256 * 256;
    T* p = reinterpret_cast<T*>(256 + used);
    used += count * sizeof(T);
    return p;
  }
  bool ok() const { return true; }
};
inline size_t mg_hier_bytes(int nx, int ny, int cycle_elem_size) {
  if (!mg_prepared_dims_ok(nx, ny) || (cycle_elem_size != 4 && cycle_elem_size != 8)) return 0;
  CountingArena ar;
  if (cycle_elem_size == 8) { MgHierT<double> H; mg_hier_carve(nx, ny, 0, 0, ar, H); }
  else { MgHierT<float> H; mg_hier_carve(nx, ny, 0, 0, ar, H); }
  return ar.used;
}
inline size_t mg_scratch_bytes(int nx, int ny, int cycle_elem_size) {
  if (!mg_prepared_dims_ok(nx, ny) || (cycle_elem_size != 4 && cycle_elem_size != 8)) return 0;
  CountingArena ar;
  if (cycle_elem_size == 8) { MgScratchT<double> S; mg_scratch_carve(nx, ny, ar, S); }
  else { MgScratchT<float> S; mg_scratch_carve(nx, ny, ar, S); }
  return ar.used;
}

}  // namespace piso
