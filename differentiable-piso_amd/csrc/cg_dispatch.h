// Host side of the pressure CG's kernel choice, shared by the one-GPU driver (cg.hip) and the slab driver (cg_slab.hip): the tiling
// of the two-kernel iteration, the plan of a solve's persistent part (persist_plan: pure, no HIP calls), WHICH cg_persist1 instances
// are compiled (persist_instance_exists: the one statement of it) and the table from a plan to its instance (persist_dispatch: the
// only host code that names cg_persist1).  A new instance is one more line in the predicate - plus a rule in the plan that picks it.
#pragma once
#include <type_traits>

#include "cg_persist1.h"

namespace piso {

constexpr int kXcdCus = 32;                      // CUs of one MI355X XCD
constexpr int kPersistRetry = -1000;             // status of a driver: a persistent segment failed, run the solve again without them

// ---- two-kernel iteration: strips of 64 * V cells, rows per wave, grids of K1 / K2 / the flat kernels (written into `a` as well).
// rpw_knob / maxblocks_knob: options cg_rpw / cg_maxblocks, <= 0 for no override (the slab driver has never honoured them: it passes 0)
struct CgTiling { int rows_per_wave, k1_tiles, g1, g2, gflat; };
template <typename T>
inline CgTiling cg_tile(CgArgs<T>& a, int V, int rpw_knob, int maxblocks_knob) {
  const size_t n = (size_t)a.nx * a.ny;
  a.ntx = (a.nx + 64 * V - 1) / (64 * V);
  int rpw = (int)(((long long)a.ny * a.ntx) / (4 * 1024));
  rpw = rpw < 2 ? 2 : (rpw > 16 ? 16 : rpw);
  if (rpw_knob > 0) rpw = rpw_knob;
  a.rows_per_wave = rpw;
  a.nty = (a.ny + 4 * rpw - 1) / (4 * rpw);
  CgTiling t;
  t.rows_per_wave = rpw; t.k1_tiles = a.ntx * a.nty;
  t.g1 = grid_for((long long)t.k1_tiles, 1, (maxblocks_knob >= 8 && maxblocks_knob <= kMaxPartials) ? maxblocks_knob : 1024);
  t.g2 = grid_for((long long)((n / V + kBlock - 1) / kBlock), 4);
  t.gflat = grid_for((long long)n, kBlock * 4);
  a.nA = t.g1; a.nB = t.g2;
  return t;
}

// iterations per persistent launch: ~10 ms of work per segment at 2048^2 (1 000 iterations; one host look per segment - a converged
// solve leaves its segment by itself).  Measured in the bench: segments of 500 / 1 000 / 2 000 iterations 4.41 / 4.44 / 4.46 steps/s -
// every launch pays its prologue, the state's trip from and to memory and a cold first iteration.  knob: option cg_segment
inline int persist_segment_len(size_t n, int knob) {
  const int len = (int)(40000.0 / ((double)n * 8.5e-6 + 4.0));
  return knob > 0 ? knob : (len < 50 ? 50 : (len > 2000 ? 2000 : len));
}

// ---- which cg_persist1<T, CT, R, NQ, RECON, SYM, SLAB, RAGGED, LOCAL> are compiled.  The planner asks at run time, the table at
// compile time; nothing else states it.
constexpr bool persist_instance_exists(size_t state_bytes, size_t coef_bytes, bool recon, bool slab, int R, int NQ, bool sym, bool ragged, bool local) {
  const bool f64 = state_bytes == 8, compact = coef_bytes == 4;     // fp64 state; off-diagonals that are exact floats
  if (slab && !f64) return false;                            // mailbox rows hold 8-byte elements
  // The symmetric variant - S and W streamed, N and E taken from the neighbours' S and W - is for compact coefficients.  On one GPU it
  // also serves systems whose diagonal cannot be rebuilt from the off-diagonals: open boundaries, where the diagonal carries the face
  // to the outside - BASELINE config 4.  It then streams the diagonal beside S and W: 16 instead of 24 bytes per cell and pass.  fp64
  // state only: the fp32 instances keep their registers only with rebuilt diagonals.  A slab runs such a system unsymmetric.
  if (sym && !(compact && (recon || (f64 && !slab)))) return false;
  // padded grids (RAGGED) and one-XCD solves (LOCAL) exist for the common case only: fp64 state, symmetric compact coefficients with
  // rebuilt diagonals, one GPU; one XCD with regions of 2 / 4 rows (a 16-row grid of <= 32 workgroups is left chip-wide)
  if ((ragged || local) && !(f64 && compact && recon && sym && !slab)) return false;
  if (local && R == 16) return false;
  // one region of 16 rows per wave: only the combinations that keep their registers.  fp32 state without a symmetric matrix with
  // rebuilt diagonals (26-84 spilled vector registers) and fp64 COEFFICIENTS (a general matrix: 8 spilled vector registers) are
  // tiled with regions of 4 / 2 rows instead - those instances spill nothing - or iterate on the two-kernel path; a slab has it for
  // symmetric systems only
  if (R == 16 && NQ == 1) return compact && (f64 ? (sym || !slab) : (recon && sym));
  // ONE region of 2 rows per wave: fp64 state, symmetric compact coefficients, one GPU, not padded
  if (R == 2 && NQ == 1) return f64 && compact && sym && !slab && !ragged;
  return (R == 2 || R == 4) && NQ == 2;                      // two regions of 2 / 4 rows per wave: everybody
}

// ---- the plan: everything the drivers need to know about a solve's persistent part
struct PersistPlan {
  int R = 0, NQ = 0;                 // rows per region, regions per wave.  R == 0: two-kernel iteration only (the shape fields mean nothing)
  int waves = kPersistWaves;         // waves of a workgroup that own regions
  int grid = 0, launch_grid = 0;     // workgroups that take part; workgroups launched (XCD-local: kXcds x grid, some XCD is dealt a full group)
  int nreg = 0, ntx = 0;             // regions, strips per row
  bool sym = false, ragged = false, xcd_local = false;   // the instance's SYM, RAGGED, LOCAL
};
struct PersistQuery {
  int nx, ny, V, per_y; bool padded;                                     // the grid (padded: CgArgs::nx_true != 0)
  size_t state_bytes, coef_bytes; bool recon, symmetric, slab;           // the instance family: sizeof(T), sizeof(CT), RECON, ...
  int cus;                                                               // the device
  int cg_persist, cg_persist_r, cg_persist_half, cg_persist_nq, cg_xcd_local;   // option values (-1: automatic)
  bool xcd_local_failed, allow_persist;
};

// region shape of the persistent kernels for an nx x ny grid (V cells per lane, `cus` compute units): one region of 16 rows per
// wave has the smallest halo overhead and is taken when it keeps at least 3/4 of the waves busy (or when forced); else two
// regions of 2 / 4 rows per wave (two regions of 8 rows do not fit the registers: such shapes - ny a multiple of 8 but not of 16 on
// a grid too large for 4-row regions - iterate on the two-kernel path).  R = 0: the grid cannot be tiled (two-kernel iteration).
struct PersistShape { int R = 0, NQ = 0, nreg = 0, ntx = 0, grid = 0; };
inline PersistShape persist_shape(int nx, int ny, int V, int cus, int force_r) {
  PersistShape s;
  if (nx % (64 * V) != 0) return s;                         // every lane of a strip has cells
  const int ntx = nx / (64 * V);
  if (ny % 16 == 0 && (force_r <= 0 || force_r == 16)) {
    const long long nreg = (long long)ntx * (ny / 16);
    if (nreg <= (long long)cus * kPersistWaves && (force_r > 0 || 4 * nreg >= 3LL * cus * kPersistWaves)) {
      s.R = 16; s.NQ = 1; s.nreg = (int)nreg; s.ntx = ntx;
      s.grid = (int)((nreg + kPersistWaves - 1) / kPersistWaves);
    }
  }
  for (int R : {2, 4}) {
    if (s.R) break;
    if (force_r > 0 && force_r != R) continue;
    if (ny % R != 0) continue;                              // every region has R rows
    const long long nreg = (long long)ntx * (ny / R);
    if (nreg % 2 == 0 && nreg <= (long long)cus * kPersistWaves * 2) {   // a wave owns 2 regions or none
      s.R = R; s.NQ = 2; s.nreg = (int)nreg; s.ntx = ntx;
      s.grid = (int)((nreg + kPersistWaves * 2 - 1) / (kPersistWaves * 2));
    }
  }
  return s;
}

// Persistent segments (cg_persist1.h) are applicable when every wave's region fits on chip.  What the device must still confirm is
// that the whole launch_grid is resident at once (persist_prepare).
inline PersistPlan persist_plan(const PersistQuery& q) {
  PersistPlan p;
  const auto exists = [&](int R, int NQ, bool ragged, bool local) {
    return persist_instance_exists(q.state_bytes, q.coef_bytes, q.recon, q.slab, R, NQ, p.sym, ragged, local);
  };
  p.ragged = q.padded;
  // (a symmetric system whose family has no SYM instance streams all four arrays)
  p.sym = q.symmetric && persist_instance_exists(q.state_bytes, q.coef_bytes, q.recon, q.slab, 2, 2, true, false, false);
  // lanes of 16 bytes; halo rows in y (per_y = 2) are what the slab instances are for, and nobody else can have them
  if (q.V != 16 / (int)q.state_bytes || (q.per_y == 2) != q.slab || !q.allow_persist || q.cg_persist == 0) return p;
  const int cus = q.cus, force_r = q.cg_persist_r;
  PersistShape shape = persist_shape(q.nx, q.ny, q.V, cus, force_r);
  if (shape.R == 16 && !exists(16, 1, false, false)) {      // no 16-row instance: regions of 4 / 2 rows, or two kernels
    shape = PersistShape();
    if (force_r <= 0) { shape = persist_shape(q.nx, q.ny, q.V, cus, 4); if (!shape.R) shape = persist_shape(q.nx, q.ny, q.V, cus, 2); }
  }
  // XCD-local mode: symmetric compact coefficients, fp64, one exchange, at most one XCD's worth of workgroups
  const bool local_ok = exists(2, 2, false, true) && q.cg_xcd_local != 0 && !q.xcd_local_failed && cus == kXcds * kXcdCus;
  // (measured at 2048^2-class work per workgroup: regions of 4 rows to make a 64-workgroup grid fit one XCD lose more in the row
  // loops than the shorter exchange wins - 512^2: 6.2 against 4.5 us per iteration; 256^2, 16 workgroups either way: 3.8 against 4.3)
  p.R = shape.R; p.NQ = shape.NQ; p.grid = shape.grid; p.nreg = shape.nreg; p.ntx = shape.ntx;
  const int grid_nq1 = (shape.nreg + kPersistWaves - 1) / kPersistWaves;   // workgroups with ONE region per wave, all eight at work

  // Small regions: ONE wave with work per SIMD instead of two (waves 4-7 of a workgroup own nothing), twice the workgroups, wherever
  // the doubled grid still fits the chip: a wave then never waits at the exchange's first barrier for the wave it shares a SIMD
  // with (0.6 us of a ~4 us iteration).  Measured: 256^2 3.80 -> 3.47 us per iteration, 512^2 4.45 -> 4.08, 1024 x 256 4.48 -> 4.08,
  // 1024 x 512 unchanged.  Option cg_persist_half 0: never, 1: wherever it fits.  Automatic (-1) leaves out the one case where the
  // doubling would push a grid that fits ONE XCD (17-32 workgroups) out of it: since the XCD-local exchange polls its own XCD's
  // records only, 32 full workgroups there beat 64 half ones chip-wide (512 x 256, round 4: 3.98 against 4.19 us per iteration).
  {
    const bool fits = (p.R == 2 || p.R == 4) && p.NQ == 2 && 2 * p.grid <= cus;
    const bool leaves_xcd = local_ok && p.grid <= kXcdCus && 2 * p.grid > kXcdCus;
    if (fits && q.cg_persist_half != 0 && (q.cg_persist_half == 1 || !leaves_xcd)) {
      p.waves = kPersistWaves / 2;
      p.grid = (shape.nreg + p.waves * p.NQ - 1) / (p.waves * p.NQ);
    }
  }
  p.xcd_local = local_ok && (p.R == 2 || p.R == 4) && p.grid <= kXcdCus;
  // Regions of 2 rows on a grid that runs chip-wide anyway (more than one XCD's worth of workgroups): ONE region per wave, all eight
  // waves of a workgroup at work - the row work per SIMD of the half-occupancy shape (two waves x one region instead of one wave
  // x two) with half its workgroups in the exchange.  Round 5, A/B on one box: 1024 x 256 (config 4) 3.73 -> 3.57 us per iteration,
  // 512^2 3.72 -> 3.60; 256^2 stays on its XCD (2.69 against 3.41).  Option cg_persist_nq: 0 never, 1 wherever the chip holds it.
  if (exists(2, 1, false, false) && q.cg_persist_nq != 0 && p.R == 2 && !q.padded && (!p.xcd_local || q.cg_persist_nq == 1) && grid_nq1 <= cus) {
    p.NQ = 1; p.waves = kPersistWaves; p.xcd_local = false; p.grid = grid_nq1;
  }
  // ... and inside ONE XCD as well, where that needs no more than its 32 workgroups: 256^2 (config 2) 2.74 -> 2.59 us per iteration
  // (eight working waves x one region instead of four x two; 512 x 256 would need 64 workgroups and keeps two regions per wave)
  if (exists(2, 1, false, true) && q.cg_persist_nq != 0 && p.xcd_local && p.R == 2 && p.NQ == 2 && !q.padded && grid_nq1 <= kXcdCus) {
    p.NQ = 1; p.waves = kPersistWaves; p.grid = grid_nq1;
  }
  // tiny grids: two-kernel path (a padded grid is here BECAUSE it is small)
  if (p.R && (size_t)q.nx * q.ny < 16384 && q.cg_persist != 1 && !q.padded) p.R = 0;
  // (the padded-grid variant exists for the common case only; a forced shape may have no instance in this family)
  if (p.R && !exists(p.R, p.NQ, p.ragged, p.xcd_local)) p.R = 0;
  if (!p.R) p.xcd_local = false;
  p.launch_grid = p.xcd_local ? kXcds * p.grid : p.grid;
  if (p.launch_grid > kPersistMaxGrid) p.R = 0;             // (the exchange keeps kPersistMaxGrid / 64 records per lane)
  return p;
}

// ---- the table: calls f(typed kernel pointer) for the instance of plan `p`; false - and no call - if no such instance is compiled
template <typename T, typename CT, bool RECON, bool SLAB, typename F>
inline bool persist_dispatch(const PersistPlan& p, F&& f) {
  bool found = false;
  auto one = [&](auto r, auto nq, auto sym, auto ragged, auto local) {
    constexpr int R = decltype(r)::value, NQ = decltype(nq)::value;
    constexpr bool SYM = decltype(sym)::value, RAGGED = decltype(ragged)::value, LOCAL = decltype(local)::value;
    if constexpr (persist_instance_exists(sizeof(T), sizeof(CT), RECON, SLAB, R, NQ, SYM, RAGGED, LOCAL)) {
      if (p.R == R && p.NQ == NQ && p.sym == SYM && p.ragged == RAGGED && p.xcd_local == LOCAL) {
        f(&cg_persist1<T, CT, R, NQ, RECON, SYM, SLAB, RAGGED, LOCAL>);
        found = true;
      }
    }
  };
  auto shape = [&](auto r, auto nq) {
    constexpr std::false_type no{}; constexpr std::true_type yes{};
    one(r, nq, no, no, no); one(r, nq, no, yes, no); one(r, nq, no, no, yes); one(r, nq, no, yes, yes);
    one(r, nq, yes, no, no); one(r, nq, yes, yes, no); one(r, nq, yes, no, yes); one(r, nq, yes, yes, yes);
  };
  shape(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}); shape(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
  shape(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{}); shape(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
  return found;
}

// Before the first launch.  The exchanges spin: EVERY workgroup must be resident at the same time.  What the occupancy calculator says
// one CU can hold (LDS, registers) times the CUs of the device must cover the launch - else p.R is cleared; what it cannot see
// (another process, a CU mask) is caught by the spin bound -> the drivers restart the solve on the two-kernel path.  Then the control
// block of the solve's launches over workspace `ws` (kPersistWsWordsAll words, cg_persist.h), which is zeroed.
template <typename T, typename CT, bool RECON, bool SLAB>
inline int persist_prepare(PersistPlan& p, int cus, PersistCtl& pc, unsigned* ws, hipStream_t stream) {
  int per_cu = 0;
  hipError_t e = hipSuccess;
  const bool have = persist_dispatch<T, CT, RECON, SLAB>(p, [&](auto kfn) { e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, kPersistThreads, 0); });
  if (e != hipSuccess) { set_error("hipOccupancyMaxActiveBlocksPerMultiprocessor", e); return PISO_ERR_HIP; }
  if (!have || (long long)per_cu * cus < p.launch_grid) p.R = 0;
  pc.rec = nullptr; pc.err = nullptr; pc.nreg = p.nreg; pc.ntx = p.ntx; pc.timing = nullptr; pc.epoch0 = 0; pc.xcd = nullptr; pc.local_n = 0; pc.waves = p.waves;
  if (!p.R) return PISO_OK;
  pc.rec = reinterpret_cast<unsigned long long*>(ws);
  pc.err = reinterpret_cast<int*>(ws + kPersistWsWordsAll - 16);
  pc.xcd = reinterpret_cast<int*>(ws + kPersistRecWords);   // 10 words behind the records, before the error flag
  pc.local_n = p.xcd_local ? p.grid : 0;
  PISO_HIP_CHECK(hipMemsetAsync(ws, 0, kPersistWsWordsAll * sizeof(unsigned), stream));
  return PISO_OK;
}

// one persistent launch: NORMAL iterations [kb, ke).  `epoch0` goes into pc: tags are unique per launch (a 16-bit launch counter above
// a 16-bit exchange counter; a segment has < 2^15 exchanges): a record left by an earlier launch - in memory or in some XCD's L2 - can
// never pass for one of this launch.  The records are zeroed as well, which covers the counter's wrap on one GPU.
template <typename T, typename CT, bool RECON, bool SLAB>
inline int persist_launch(const PersistPlan& p, const CgArgs<T>& a, PersistCtl& pc, unsigned launch_count, int kb, int ke, int sv, bool pending,
                          const std::conditional_t<SLAB, SlabCtl, NoSlab>& sl, hipStream_t stream) {
  pc.epoch0 = (launch_count & 0xffffu) << 16;
  PISO_HIP_CHECK(hipMemsetAsync(pc.rec, 0, kPersistZeroBytes, stream));   // records (both levels) + XCD arrivals
  const bool have = persist_dispatch<T, CT, RECON, SLAB>(p, [&](auto kfn) { kfn<<<p.launch_grid, kPersistThreads, 0, stream>>>(a, pc, kb, ke, sv, pending ? 1 : 0, sl); });
  if (!have) { set_error_msg("pressure CG: the plan names a cg_persist1 instance that is not compiled"); return PISO_ERR_INVALID_ARG; }
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

}  // namespace piso
