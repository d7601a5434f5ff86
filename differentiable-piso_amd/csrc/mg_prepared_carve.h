// What a one-GPU multigrid solve works on, MgPlanT<C>, and how it is carved - pure host code, no HIP calls, like mg_slab_carve.h: a host
// compiler builds a driver over it (tests/mg_prepared_carve_driver.cpp) that walks every carve against arenas without memory.
//   hierarchy  everything that depends on the matrix only: a header, SC_SUM_DIAG / SC_NPRESENT, the five coefficient arrays and dinv of
//              every level (float32 cycle: the fp64 level 0 of the outer iteration AND the float32 levels)
//   scratch    what one solve writes: r, z, t of every level, p, q, the partials, `scal`, MgState (float32 cycle: the fp64 r beside fl32(r))
// A PREPARED solve (mg_prepared.h) keeps the two in buffers of their own - the hierarchy is the caller's, kept between solves (mg_hier_carve,
// mg_scratch_carve); the ordinary solve carves both out of its one workspace, without a header and with one `scal` (mg_plan_carve).
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

template <typename C>
struct MgPlanT {
  MgHierT<C> H;
  MgScratchT<C> S;
};

inline bool mg_prepared_dims_ok(int nx, int ny) { return nx >= kPlanMinDim && ny >= kPlanMinDim && (long long)nx * ny <= (1ll << 30); }

inline void mg_hier_level0(MgHierT<double>& H) { H.L0 = H.lv[0]; }
inline void mg_hier_level0(MgHierT<float>&) {}
inline void mg_scratch_outer_r(MgScratchT<double>& S) { S.r64 = S.r[0]; }
inline void mg_scratch_outer_r(MgScratchT<float>&) {}

// the pieces the carves share: a level's dimensions and its six arrays; the fp64 vectors, partials, sums and state behind the cycle's vectors
template <typename LV>
inline void mg_level_dims(const MgDims& d, int l, int per_x, int per_y, LV& L) {
  L.nx = d.nx[l]; L.ny = d.ny[l]; L.n = L.nx * L.ny; L.per_x = per_x; L.per_y = per_y;
}
template <typename T, typename LV, typename AR>
inline void mg_level_take(AR& ar, LV& L) {
  for (int s = 0; s < 5; ++s) L.c[s] = ar.template take<T>(L.n);
  L.dinv = ar.template take<T>(L.n);
}
template <typename C, typename AR>
inline void mg_scratch_outer(size_t n0, AR& ar, MgScratchT<C>& S) {
  if (sizeof(C) == 4) S.r64 = ar.template take<double>(n0);
  mg_scratch_outer_r(S);
  S.p[0] = ar.template take<double>(n0); S.p[1] = ar.template take<double>(n0); S.q = ar.template take<double>(n0);
  S.parts = ar.template take<double>(4 * kMgGrid);
  S.part_rz = ar.template take<double>(kMgGrid); S.part_pq = ar.template take<double>(kMgGrid); S.part_max = ar.template take<double>(kMgGrid);
  S.scal = ar.template take<double>(SC_COUNT_MG);
  S.st = ar.template take<MgState>(1);
}

// AR: Arena of piso_common.h, or the driver's.  Every array starts on the arena's 256-byte boundary, so a float row stays 16-byte aligned where
// nx % 4 == 0 - the levels the four-cell kernels run on.
template <typename C, typename AR>
inline bool mg_hier_carve(int nx, int ny, int per_x, int per_y, AR& ar, MgHierT<C>& H) {
  const MgDims d = mg_dims(nx, ny);
  H.nlev = d.nlev; H.tail_first = d.tail_first;
  H.hdr = ar.template take<MgHierHeader>(1);
  H.scal = ar.template take<double>(SC_COUNT_MG);
  mg_level_dims(d, 0, per_x, per_y, H.L0);
  if (sizeof(C) == 4) mg_level_take<double>(ar, H.L0);
  for (int l = 0; l < d.nlev; ++l) {
    mg_level_dims(d, l, per_x, per_y, H.lv[l]);
    mg_level_take<C>(ar, H.lv[l]);
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
  mg_scratch_outer((size_t)d.nx[0] * d.ny[0], ar, S);
  return ar.ok();
}
// the one workspace of the ordinary solve: a level's arrays and its vectors side by side, no header, the set-up's sums in the solve's `scal`
template <typename C, typename AR>
inline bool mg_plan_carve(int nx, int ny, int per_x, int per_y, AR& ar, MgPlanT<C>& P) {
  const MgDims d = mg_dims(nx, ny);
  MgHierT<C>& H = P.H;
  MgScratchT<C>& S = P.S;
  H.nlev = d.nlev; H.tail_first = d.tail_first;
  H.hdr = nullptr;
  mg_level_dims(d, 0, per_x, per_y, H.L0);
  if (sizeof(C) == 4) mg_level_take<double>(ar, H.L0);
  for (int l = 0; l < d.nlev; ++l) {
    mg_level_dims(d, l, per_x, per_y, H.lv[l]);
    mg_level_take<C>(ar, H.lv[l]);
    S.r[l] = ar.template take<C>(H.lv[l].n); S.z[l] = ar.template take<C>(H.lv[l].n); S.t[l] = ar.template take<C>(H.lv[l].n);
  }
  mg_hier_level0(H);
  mg_scratch_outer((size_t)H.L0.n, ar, S);
  H.scal = S.scal;
  return ar.ok();
}

// the sizes the carves need (0: not a grid the solver takes, or not a cycle precision)
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
enum MgBuffer { MG_BUF_HIERARCHY, MG_BUF_SCRATCH, MG_BUF_WORKSPACE };
template <typename C>
inline size_t mg_carved_bytes(int nx, int ny, MgBuffer what) {
  CountingArena ar;
  MgPlanT<C> P;
  if (what == MG_BUF_HIERARCHY) mg_hier_carve(nx, ny, 0, 0, ar, P.H);
  else if (what == MG_BUF_SCRATCH) mg_scratch_carve(nx, ny, ar, P.S);
  else mg_plan_carve(nx, ny, 0, 0, ar, P);
  return ar.used;
}
inline size_t mg_buffer_bytes(int nx, int ny, int cycle_elem_size, MgBuffer what) {
  if (!mg_prepared_dims_ok(nx, ny) || (cycle_elem_size != 4 && cycle_elem_size != 8)) return 0;
  return cycle_elem_size == 8 ? mg_carved_bytes<double>(nx, ny, what) : mg_carved_bytes<float>(nx, ny, what);
}
inline size_t mg_hier_bytes(int nx, int ny, int cycle_elem_size) { return mg_buffer_bytes(nx, ny, cycle_elem_size, MG_BUF_HIERARCHY); }
inline size_t mg_scratch_bytes(int nx, int ny, int cycle_elem_size) { return mg_buffer_bytes(nx, ny, cycle_elem_size, MG_BUF_SCRATCH); }
inline size_t mg_plan_bytes(int nx, int ny, int cycle_elem_size) { return mg_buffer_bytes(nx, ny, cycle_elem_size, MG_BUF_WORKSPACE); }

}  // namespace piso
