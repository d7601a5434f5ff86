// The shape of a multigrid solve (mg.hip) - pure host code, no HIP calls: a host compiler builds a driver over it
// (tests/mg_slab_plan_driver.cpp), in the spirit of cg_dispatch.h / bicgstab_dispatch.h / conv_dispatch.h.
//   mg_dims        the hierarchy of the one-GPU plan: level dimensions (2 x 2 aggregation, ceil) and the first level of the one-workgroup tail;
//   mg_slab_plan   the same hierarchy cut into y-slabs: levels [0, g) are SHARDED (a rank holds its nyl >> l rows plus one halo row below
//                  and one above), level g - the first whose global cell count is within the gather limit - and everything coarser is
//                  REPLICATED (every rank forms its rows of level g, the rows are all-gathered, and levels g .. coarsest run redundantly
//                  with the whole-grid kernels).  2 x 2 aggregates must never straddle a cut: nyl % 2^g == 0, else the plan refuses.
#pragma once
#include <stdio.h>

namespace piso {

// the constants of mg.hip that shape a hierarchy, restated for host code without HIP (mg.hip holds each to its own by static_assert)
constexpr int kPlanMinDim = 4;         // kMinDim: no level has fewer cells than this in a dimension
constexpr int kPlanTailCells = 4096;   // kTailCells: levels of at most this many cells run inside one workgroup
constexpr int kPlanTailLds = 6144;     // kTailLds: cells of all tail levels together
constexpr int kPlanTailMaxLevels = 8;  // kTailMaxLevels
constexpr int kPlanMaxLevels = 16;     // kMgMaxLevels
constexpr int kGatherCells = 8192;     // doubles one all-gather carries over all ranks (peer.h: the gather area of a mailbox)

struct MgDims {
  int nlev, tail_first;                // tail_first: first level of the one-workgroup tail (-1: none fits)
  int nx[kPlanMaxLevels], ny[kPlanMaxLevels];
};
inline MgDims mg_dims(int nx, int ny) {
  MgDims d;
  int l = 0;
  for (;; ++l) {
    d.nx[l] = nx; d.ny[l] = ny;
    const int nxc = (nx + 1) / 2, nyc = (ny + 1) / 2;
    if (nxc < kPlanMinDim || nyc < kPlanMinDim || l + 1 == kPlanMaxLevels) break;
    nx = nxc; ny = nyc;
  }
  d.nlev = l + 1;
  d.tail_first = -1;
  for (int f = 0; f < d.nlev; ++f) {
    int cells = 0;
    for (int k = f; k < d.nlev; ++k) cells += d.nx[k] * d.ny[k];
    if (d.nx[f] * d.ny[f] <= kPlanTailCells && cells <= kPlanTailLds && d.nlev - f <= kPlanTailMaxLevels) { d.tail_first = f; break; }
  }
  return d;
}

// the gather limit: kGatherCells, or the option mg_slab_gather_cells when that is positive and smaller
inline int mg_gather_limit(int option) { return (option > 0 && option < kGatherCells) ? option : kGatherCells; }

struct MgSlabPlan {
  int status;                          // 0: accepted; else refused (PISO_ERR_INVALID_ARG) with `msg`
  char msg[256];
  MgDims d;                            // the one-GPU hierarchy
  int world, nyl, g;                   // ranks, level-0 rows per rank, first replicated level
  int tail_first;                      // first level of the one-workgroup tail among the replicated levels (-1: none)
  int rows[kPlanMaxLevels];              // rows a rank holds of level l: nyl >> l below g (plus two halo rows in storage), all of them from g on
};
constexpr int kMgSlabPlanHead = 6;     // flat record: status, levels, g, tail_first, nyl, world, then {nx, ny, rows} per level
inline int mg_slab_plan_record(const MgSlabPlan& p, int* out, int capacity) {
  const int n = kMgSlabPlanHead + 3 * (p.status ? 0 : p.d.nlev);
  int rec[kMgSlabPlanHead + 3 * kPlanMaxLevels] = {p.status, p.status ? 0 : p.d.nlev, p.g, p.tail_first, p.nyl, p.world};
  for (int l = 0; !p.status && l < p.d.nlev; ++l) { rec[kMgSlabPlanHead + 3 * l] = p.d.nx[l]; rec[kMgSlabPlanHead + 3 * l + 1] = p.d.ny[l]; rec[kMgSlabPlanHead + 3 * l + 2] = p.rows[l]; }
  for (int i = 0; i < n && i < capacity; ++i) out[i] = rec[i];
  return n;
}

inline MgSlabPlan mg_slab_plan(int nx, int ny, int world, int gather_limit) {
  MgSlabPlan p;
  p.status = 1; p.msg[0] = 0; p.world = world; p.nyl = 0; p.g = -1; p.tail_first = -1;
  const int limit = mg_gather_limit(gather_limit);
  const char* rule = "the slab multigrid shards levels 0 .. g - 1, g the first level of at most %d cells (mg_slab_gather_cells), and needs "
                     "ny / ranks divisible by 2^g: %s; use the plain solver (PisoPressureSolverCudaCustom)";
  char why[128];
  if (world < 1 || nx < kPlanMinDim || ny < kPlanMinDim || (long long)nx * ny > (1ll << 30)) {
    snprintf(p.msg, sizeof(p.msg), "piso_mg_slab: needs at least %d cells in each dimension and at least one rank", kPlanMinDim);
    return p;
  }
  if (ny % world != 0) {
    snprintf(why, sizeof(why), "ny = %d is not divisible by %d ranks", ny, world);
    snprintf(p.msg, sizeof(p.msg), rule, limit, why);
    return p;
  }
  p.d = mg_dims(nx, ny);
  p.nyl = ny / world;
  for (int l = 0; l < p.d.nlev; ++l)
    if ((long long)p.d.nx[l] * p.d.ny[l] <= limit) { p.g = l; break; }
  if (p.g < 0) {
    snprintf(why, sizeof(why), "no level of the %d x %d hierarchy is that small", nx, ny);
    snprintf(p.msg, sizeof(p.msg), rule, limit, why);
    return p;
  }
  if (p.nyl % (1 << p.g) != 0) {
    snprintf(why, sizeof(why), "%d rows per rank are not divisible by %d (g = %d)", p.nyl, 1 << p.g, p.g);
    snprintf(p.msg, sizeof(p.msg), rule, limit, why);
    return p;
  }
  for (int l = 0; l < p.d.nlev; ++l) p.rows[l] = l < p.g ? p.nyl >> l : p.d.ny[l];
  p.tail_first = p.d.tail_first < 0 ? -1 : (p.d.tail_first > p.g ? p.d.tail_first : p.g);
  p.status = 0;
  return p;
}

// collectives one iteration issues, counted from the plan (nu sweeps, no residual reset): row exchanges, all-reduces, all-gathers
struct MgSlabCollectives { int exchanges, allreduces, allgathers; };
inline MgSlabCollectives mg_slab_collectives(const MgSlabPlan& p, int nu) {
  MgSlabCollectives c{0, 2, 2};                            // (r, z) and (p, q); the restricted residual (or r itself) and the maxima of |r|
  if (p.g == 0) return c;                                  // the cycle is replicated: z and its neighbour rows are read from the rank's copy
  const int down = (nu >= 2 ? 1 : 0) + (nu > 2 ? nu - 2 : 0) + 1;      // r before pre2, z before every further sweep, z before restriction
  const int up = nu - 1;                                               // z before every post-sweep but the first
  c.exchanges = p.g * (down + up) + (p.g - 1) + 1;                     // + e of a sharded coarser level + z before the direction
  return c;
}

}  // namespace piso
