// Persistent CG segment kernel: many NORMAL iterations in ONE launch with ONE grid-wide exchange per iteration, for grids whose
// solver state fits on chip (DESIGN.md 3.1 has the measurements behind every choice below; the first persistent kernel of rounds
// 1-2 needed two exchanges).
//
// r, p in registers, x in LDS, float coefficient rows streamed through a circular software pipeline, one workgroup of 512 threads
// per CU; per-cell arithmetic as the two-kernel path (zrow: summation order of calcZ_v4, pressure_solve_op.cu.cc:81-90).  How the
// two dependent reductions of a CG iteration are obtained from one exchange:
//
//   D(k)  p_k = r_k + beta_k p_{k-1};  z' = L p_k;  local sums  S p, p.r, p.z', r.z', z'.z', S z'
//         the PERIMETER of z' is published (sc1 stores, ping-pong buffer k & 1)
//   E(k)  one exchange of 8 sums per workgroup: the six above and  S r_k, #{|r_k| >= accuracy}  left over from U(k-1)
//         -> alpha_k = p.r / (p.z' + vs S p)                                   (pressure_solve_op.cu.cc:301-302)
//            r_{k+1}.z'_k = r.z' - alpha (z'.z' + vs S z'),  S r_{k+1} = S r_k - alpha (S z' + N vs)    [r_{k+1} = r_k - alpha (z' + vs)]
//         -> beta_{k+1} = -(r_{k+1}.z'_k + vs S r_{k+1}) / pz                  (:351-352) without a second reduction
//         -> the stopping test of iteration k (every 5th, device-flag cadence of :312-335) on #{|r_k| >= accuracy}: it is
//            evaluated one exchange later than in cg_persist, BEFORE x and r move on, so a converged solve stops in exactly
//            the reference's state (x_k, iterations = k)
//   U(k)  z' = L p_k again (same registers, same instructions: bitwise the same);  x += alpha p_k;  r -= alpha (z' + vs);
//         local  S r_{k+1}, #{|r_{k+1}| >= accuracy}
//
// Every region keeps copies of r and p on the ring of cells around it and advances them with the SAME fma's as their
// owners (bitwise equal), using the published perimeter of z' - so one vector's perimeter crosses the fabric per iteration
// instead of two, and nothing has to be visible between D and U of one iteration: one exchange.
// Round 4: the exchange is a tree that follows the hardware (workgroup -> XCD leader through that XCD's L2 -> everybody: every wave
// polls the eight XCD records itself, no second barrier; grid_exchange8_hier in cg_persist.h), the end cells of a region's rows are published as
// one packed block per region (kPack: the L2 was full of single-cell cache lines), z' of U's first rows is computed while the
// exchange's records travel (kAhead), and whatever only the rare paths need is read again from the kernarg segment (karg).
// The one-step recurrences start from directly summed quantities in every iteration (no drift); they replace two dot
// products by algebraically equal expressions, so iterates differ from cg_k1 / cg_k2 at round-off level (like any two
// summation orders); converged answers and the stopping cadence are the reference's.  A segment starts from and ends in the
// global-memory state of the two-kernel path, exactly like cg_persist.
#pragma once
#include <cstddef>
#include <type_traits>

#include "cg_persist.h"

namespace piso {

// ---- the three shape parameters an A/B build may still override (-DPISO_PERSIST1_<NAME>=n with scripts/build_variant.py); everything
// else that used to be a compile-time switch here is folded to the variant that shipped (the measurements that decided each one
// are in profiles/README.md, "persistent CG kernel: variants measured and dropped").
// Coefficient rows in flight per wave of the 16-row kernel on a symmetric matrix (kDeep); every other shape: 3 / 4.  With the
// back-and-forth row order: 3 rows 12.5 us, 4 rows 11.8 us, 5 rows 11.5 us per iteration (round 3), 6 rows spill.
#ifndef PISO_PERSIST1_DEPTH
#define PISO_PERSIST1_DEPTH 5
#endif
// Rows of z' = L p that the U pass finds precomputed (kAhead, <= DEPTH).  Round 6 A/B on one box (2048^2, us per iteration):
// DEPTH 5 / AHEAD 2 9.6 - 10.7 (shipped), 4 / 4 10.6 - 10.8, 5 / 3 10.2 - 11.0 (1 VGPR spilled), 5 / 4 11.1 - 11.4 (3), 5 / 5 11.8 - 12.7.
#ifndef PISO_PERSIST1_AHEAD
#define PISO_PERSIST1_AHEAD 2
#endif
// Small regions: U reuses D's z' where z' of all rows of a wave fits this many registers (kKeepZ).  64 would cover the 16-row
// kernel: 26 - 35 VGPRs spill at any DEPTH (round 6), i.e. the registers beside r and p are what z' has no room in.
#ifndef PISO_PERSIST1_KEEP_Z_REGS
#define PISO_PERSIST1_KEEP_Z_REGS 32
#endif

// x-neighbours across the lanes of a wave.  The values beyond the two ends of the strip (`ring`: the left neighbour of row j in
// lane j, the right neighbour in lane 48 + j) enter through the `old` operand of the wave shift: one row-local DPP shift brings
// lane j to lane 0 (row_shl:j) or lane 48 + j to lane 63 (row_shr:15-j), the wave shift keeps it there.  2 VALU instructions
// per 32-bit half - through v_readlane + v_mov (SGPR broadcast) it was 3, and the loop is bound by VALU issue.
template <int CTRL>
__device__ __forceinline__ int dpp_mov32(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }   // (no `old` operand to set up)
template <bool UP>
__device__ __forceinline__ int ring_to_end32(int ring, int j) {     // j: constant after unrolling
  if (UP) {
    switch (j) {
      case 0: return ring;
      case 1: return dpp_mov32<0x101>(ring); case 2: return dpp_mov32<0x102>(ring); case 3: return dpp_mov32<0x103>(ring);
      case 4: return dpp_mov32<0x104>(ring); case 5: return dpp_mov32<0x105>(ring); case 6: return dpp_mov32<0x106>(ring);
      case 7: return dpp_mov32<0x107>(ring); case 8: return dpp_mov32<0x108>(ring); case 9: return dpp_mov32<0x109>(ring);
      case 10: return dpp_mov32<0x10a>(ring); case 11: return dpp_mov32<0x10b>(ring); case 12: return dpp_mov32<0x10c>(ring);
      case 13: return dpp_mov32<0x10d>(ring); case 14: return dpp_mov32<0x10e>(ring); default: return dpp_mov32<0x10f>(ring);
    }
  } else {
    switch (j) {
      case 15: return ring;
      case 14: return dpp_mov32<0x111>(ring); case 13: return dpp_mov32<0x112>(ring); case 12: return dpp_mov32<0x113>(ring);
      case 11: return dpp_mov32<0x114>(ring); case 10: return dpp_mov32<0x115>(ring); case 9: return dpp_mov32<0x116>(ring);
      case 8: return dpp_mov32<0x117>(ring); case 7: return dpp_mov32<0x118>(ring); case 6: return dpp_mov32<0x119>(ring);
      case 5: return dpp_mov32<0x11a>(ring); case 4: return dpp_mov32<0x11b>(ring); case 3: return dpp_mov32<0x11c>(ring);
      case 2: return dpp_mov32<0x11d>(ring); case 1: return dpp_mov32<0x11e>(ring); default: return dpp_mov32<0x11f>(ring);
    }
  }
}
// lane l receives `v` of lane l - 1 (UP) or l + 1 (!UP); lane 0 / lane 63 receives the ring value of row j
template <bool UP, typename S>
__device__ __forceinline__ S shift_ring(S v, S ring, int j) {
  constexpr int ctrl = UP ? 0x138 /* wave_shr:1 */ : 0x130 /* wave_shl:1 */;
  if constexpr (sizeof(S) == 8) {
    const unsigned long long b = (unsigned long long)__double_as_longlong((double)v), e = (unsigned long long)__double_as_longlong((double)ring);
    const int elo = ring_to_end32<UP>((int)(unsigned)e, j), ehi = ring_to_end32<UP>((int)(unsigned)(e >> 32), j);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(elo, (int)(unsigned)b, ctrl, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(ehi, (int)(unsigned)(b >> 32), ctrl, 0xf, 0xf, false);
    return (S)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  } else {
    const int e = ring_to_end32<UP>(__float_as_int((float)ring), j);
    return (S)__int_as_float(__builtin_amdgcn_update_dpp(e, __float_as_int((float)v), ctrl, 0xf, 0xf, false));
  }
}
// lane layout of the ring columns: lanes [0, R) the left neighbours of rows 0 .. R-1, lanes [48, 48 + R) the right neighbours
__device__ __forceinline__ void ring_lane(int lane, int R, int& side, int& er) {
  side = (lane < R) ? 0 : ((lane >= 48 && lane < 48 + R) ? 1 : 2);
  er = (side == 1) ? lane - 48 : lane;
}

constexpr int kSystem = 17;                       // buffer cache policy sc0 | sc1: system scope (peer-mapped mailboxes)

// RAGGED = true: padded-grid mode (CgArgs::nx_true / ny_true): the rank-1 shift skips the cells of the padding - everything else
// about them is zero by construction (zero coefficients, zero right-hand side).
// LOCAL = true: XCD-local mode for grids that need at most one XCD's worth of workgroups (the small BASELINE configurations,
// where an iteration is nothing but the exchange: 4.3 us with 16 workgroups spread over the chip).  The launch has 8 x c.local_n
// workgroups, of which the c.local_n that local_enter elects run the solve.  Inside the group, published data and records are
// stored WITHOUT sc1 (they stay in the XCD's L2) and read with sc1 loads (L1 bypassed, L2-served).
template <typename T, typename CT, int R, int NQ, bool RECON, bool SYM, bool SLAB = false, bool RAGGED = false, bool LOCAL = false>
__global__ __launch_bounds__(kPersistThreads) void cg_persist1(CgArgs<T> a, PersistCtl c, int k_begin, int k_end, int sv, int pend,
                                                               std::conditional_t<SLAB, SlabCtl, NoSlab> sl = {}) {
  // The body in order: 1 entry state, 2 coefficient pipeline (and the lambdas of the row loops), then per iteration 3 D, 4 exchange +
  // scalars, 5 U, and 6 exit.  One function on purpose: the lambdas share the register file, a state struct would not.
  static_assert(!(SLAB && RAGGED), "a slab is never padded");
  static_assert(!(SLAB && LOCAL), "a slab's neighbours are other GPUs");
  // cache policy of what other workgroups read inside the launch (non-temporal hints on the published rows / the halo loads were
  // measured and lose: the publish -> read path lives on the caches)
  constexpr int kPub = LOCAL ? kPlain : kAgent;
  constexpr int kHalo = kAgent;
  constexpr int V = 16 / sizeof(T);                        // 16-byte lane accesses
  static_assert(R * NQ <= 16 && 2 * R <= 64, "at most 16 rows per wave; the edge columns of a region fit one wave-wide load");
  static_assert(!SLAB || sizeof(T) == 8, "mailbox rows hold 8-byte elements");
  __shared__ T xs[kPersistWaves * NQ * R * 64 * V];        // the solution of my regions (128 KB at 16 rows per wave, fp64)
  __shared__ T smem[2 * kX1Sm + (SLAB ? 2 * kX1SmX : 0)];
  // the direction on the rows below / above my regions: parked in LDS (two reads per pass, one read-modify-write per iteration)
  constexpr bool kParkHalos = (NQ * R < 16) || NQ == 1;     // (two regions of 8 rows: x already fills the LDS)
  __shared__ T halo_s[kParkHalos ? kPersistWaves * NQ * 2 * 64 * V : 1];
  // The ring columns of the direction (and, SYM, the W coefficient of the column right of the strip), by lane as `edge` / `eW`
  // hold them: lanes [0, R) the left neighbours of rows 0 .. R-1, lanes [48, 48 + R) the right ones.  Row jj needs its two ring
  // values in lanes 0 and 63 as the `old` operand of the wave shifts; through the DPP network that is a row-local shift per 32-bit
  // half and side (5 VALU instructions per row and pass in a loop that is bound by VALU issue), through the LDS it is one
  // broadcast read per row and pass that every lane receives (ring_issue) and no VALU slot at all.
  // (the slab variant and the fp64-coefficient fallback have no registers for the values in flight: they keep the DPP shifts)
  constexpr bool kRingLds = sizeof(CT) == 4;
  // ... and with kRingLds the ring-column copies of p AND r (one value per lane) live in the wave's LDS ring block between their two
  // uses per iteration (D's start, U's end) instead of in registers across both row loops
  constexpr int kRingBytes = 64 * (int)sizeof(T) + 64 * (int)sizeof(CT) + (kRingLds ? 64 * (int)sizeof(T) : 0);
  constexpr unsigned kRingR = 64u * (unsigned)sizeof(T) + 64u * (unsigned)sizeof(CT);      // byte offset of the parked r column inside a ring block
  __shared__ __attribute__((aligned(16))) unsigned char ring_s[kRingLds ? kPersistWaves * NQ * kRingBytes : 16];
  const int nx = a.nx, ny = a.ny;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform: scalar branches, SGPRs
  int wg = blockIdx.x;                                     // XCD-contiguous bands (block b is observed on XCD b % 8)
  if (gridDim.x % kXcds == 0) wg = (blockIdx.x % kXcds) * (gridDim.x / kXcds) + blockIdx.x / kXcds;
  int nslots = (int)gridDim.x;                             // workgroups that take part in the exchanges
  if constexpr (LOCAL) {
    __shared__ int local_rank_s;
    wg = local_enter(c, &local_rank_s);
    if (wg < 0) return;                                    // not in the group that runs the solve
    nslots = c.local_n;
  }
  const int slot = LOCAL ? wg : (int)blockIdx.x;           // my exchange record
  // chip-wide launches: the exchange is a tree over the XCDs (grid_exchange8_hier); where am I in it?  XCD-local launches: every
  // wave polls the group's records itself (grid_exchange8_local)
  unsigned hx = 0;
  __shared__ int hier_s[4];
  if constexpr (LOCAL) { if (threadIdx.x == 0) hier_s[2] = 0; }          // (the sticky flag; the barriers of the set-up below publish it)
  if constexpr (!LOCAL) {
    hx = hier_enter(c, hier_s);
    if (hier_s[1]) return;                                 // (every workgroup of the launch fails this the same way)
  }
  int j0[NQ], tx0[NQ];
  bool has[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int reg = (wg * c.waves + wave) * NQ + q;
    has[q] = wave < c.waves && reg < c.nreg;
    const int ty = has[q] ? reg / c.ntx : 0;
    tx0[q] = has[q] ? reg - ty * c.ntx : 0;
    j0[q] = ty * R;
  }
  const unsigned nbytesT = (unsigned)((size_t)nx * ny * sizeof(T)), nbytesC = (unsigned)((size_t)nx * ny * sizeof(CT));
  const unsigned rowT = (unsigned)(nx * sizeof(T)), rowC = (unsigned)(nx * sizeof(CT));
  // SLAB: does region q touch the lower / upper edge of the slab, and is there a GPU beyond it (else: a wall of the global grid)?
  // ONE scalar of edge bits per region, opaque to the optimiser (it would expand them into flags that live in SGPRs across the
  // loop): bit 0 first row = the slab's first row AND a GPU lies below, bit 1 last row = the slab's last row AND a GPU lies above,
  // bit 2 / 3 first / last row = the slab's first / last row.  Everything else the two edge waves of a slab need - mailbox
  // addresses, the row capacity - is fetched from the kernarg segment where it is used (karg): it used to occupy ~30 SGPRs in
  // EVERY wave, which came back as v_readlane reloads in a loop that is bound by VALU issue (113 spilled SGPRs, 17-19 us per
  // iteration against 11 for the single-GPU kernel).
  typedef Persist1Kargs<T, std::conditional_t<SLAB, SlabCtl, NoSlab>> KArgs;
  constexpr unsigned sl_off = (unsigned)offsetof(KArgs, sl);
  constexpr unsigned pv_off = sl_off + (unsigned)offsetof(SlabCtl, pv);
  unsigned ef[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ef[q] = 0;
    if constexpr (SLAB) {
      const bool bot = has[q] && j0[q] == 0, top = has[q] && j0[q] + R == ny;
      ef[q] = (bot && sl.pv.lower >= 0 ? 1u : 0u) | (top && sl.pv.upper >= 0 ? 2u : 0u) | (bot ? 4u : 0u) | (top ? 8u : 0u);
      ef[q] = (unsigned)__builtin_amdgcn_readfirstlane((int)ef[q]);
      asm volatile("" : "+s"(ef[q]));
    }
  }
  {                                                         // the mirror of the argument list IS the argument list (every instance: the exit block relies on it)
    typedef CgArgs<T> A;
    if (karg<T*>((unsigned)offsetof(KArgs, a) + (unsigned)offsetof(A, r)) != a.r || karg<int*>((unsigned)offsetof(KArgs, c) + (unsigned)offsetof(PersistCtl, err)) != c.err) {
      if (threadIdx.x == 0) *c.err = 1;
      return;
    }
  }
  if constexpr (SLAB) {
    if (karg<char*>(sl_off + (unsigned)offsetof(SlabCtl, rows_own)) != sl.rows_own || karg<size_t>(pv_off + (unsigned)offsetof(PeerView, row_cap)) != sl.pv.row_cap) {
      if (threadIdx.x == 0) *c.err = 1;
      return;
    }
  }
  const unsigned nbytesH = nbytesT + 2 * rowT;              // r / p[] including their halo rows (resources built where they are used)
  // resource of the eight rows of a mailbox (host-level exchange + z' halos) and the byte offset of z' halo row (parity, side)
  // inside them: built by the edge waves where they use them
  // (on = false: a resource of no bytes - every access through it is dropped by the range check: the edge rows' mailbox stores
  // sit in the row loop without a branch; control flow in the middle of the unrolled loop cost the allocator 95 spilled VGPRs)
  auto mailbox_rows = [&](unsigned field_off, int parity, int side, unsigned& zoff, bool on = true) __attribute__((always_inline)) -> rsrc_t {
    const unsigned cap8 = (unsigned)karg<size_t>(pv_off + (unsigned)offsetof(PeerView, row_cap)) * 8u;
    zoff = (unsigned)(4 + parity * 2 + side) * cap8;
    return make_rsrc(karg<char*>(sl_off + field_off), on ? 8u * cap8 : 0u);
  };
  const rsrc_t RoS = make_rsrc(a.oS, nbytesC), RoW = make_rsrc(a.oW, nbytesC), RoE = make_rsrc(a.oE, nbytesC), RoN = make_rsrc(a.oN, nbytesC);
  const rsrc_t RcC = make_rsrc(a.cC, nbytesT);
  // p[0] / p[1]: the direction of the two-kernel path, read on entry and written on exit.  zp[0] / zp[1]: the published z'
  // perimeters, touched by agent-scope (sc1) stores and loads only - never by a plain load, whose copy of a line in the reader
  // XCD's L2 another XCD's write-through store does not invalidate.
  // (r, x, p[]: resources built at the entry and again at the exit - a resource that stays alive across the loop costs 4 SGPRs,
  // and spilled SGPRs come back through v_readlane: VALU slots of a loop that is bound by VALU issue)
  const rsrc_t Rz0 = make_rsrc(a.zp[0], nbytesT), Rz1 = make_rsrc(a.zp[1], nbytesT);
  auto row_wrap = [&](int j, bool& valid) __attribute__((always_inline)) -> int {   // scalar: rows outside wrap or vanish
    valid = true;
    if (j < 0) { if (!a.per_y) valid = false; return ny - 1; }
    if (j >= ny) { if (!a.per_y) valid = false; return 0; }
    return j;
  };

  // ---- 1 ENTRY STATE.  The state of the two-kernel path: r and the direction p_{k-1} of my regions into registers, x into LDS
  const T alpha0 = pend ? uniform(a.scal[SC_ALPHA]) : (T)0;   // pend: x still lacks alpha p of the iteration before k_begin
  Vec<T, V> rr[NQ][R], pp[NQ][R];
  // kPack (regions of more than two rows): the END CELLS of a region's rows - what the strips to the left and right read - are
  // published as one packed block per region instead of in place: entry (side, row) = the 16 bytes of lane 0 (side 0) or lane 63
  // (side 1), 2 x R x 16 bytes at the start of the region's SECOND row of the z' buffer (interior rows of that buffer are
  // otherwise unused).  In place every end cell dirtied a cache line of its own in the writer's L2 and was fetched as a line of
  // its own by the reader: 28 + 28 lines per region and iteration against 4 + 4 - and ~1 MB per XCD of L2 capacity that the
  // coefficient rows (4.19 MB per XCD at 2048^2 on a 4 MB L2) were missing.
  constexpr bool kPack = R > 2 && V == 2;
  unsigned vT[NQ], vEnd[NQ];                               // vEnd: where lanes 0 and 63 publish their end cells, beyond any buffer elsewhere
  // copies of r (registers) and of the direction (LDS / registers, `edge`) on the ring around my regions
  Vec<T, V> rhb[NQ], rha[NQ], pnb[NQ], pna[NQ];
  T eR[NQ], edge[NQ];
  bool vb[NQ], va[NQ], vl[NQ], vr[NQ];                      // is there a cell below / above / left / right of region q at all? (entry only)
  unsigned nbits[NQ];                                       // ... the same four as bits of one scalar (the loop's copy)
  auto nbit = [&](int q, unsigned bit) __attribute__((always_inline)) -> bool {
    unsigned b = nbits[q];
    asm volatile("" : "+s"(b));
    return (b & bit) != 0;
  };
  {
    const rsrc_t Rr = make_rsrc(a.r, nbytesT), Rx = make_rsrc(a.x, nbytesT), Rp = make_rsrc(a.p[k_begin & 1], nbytesT);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int cq = (tx0[q] * 64 + lane) * V;
      vT[q] = (unsigned)(cq * sizeof(T));
      vEnd[q] = (lane == 0 || lane == 63) ? vT[q] : 0x80000000u;
      if constexpr (kPack) vEnd[q] = lane == 0 ? (unsigned)(tx0[q] * 64 * V * sizeof(T)) : (lane == 63 ? (unsigned)(tx0[q] * 64 * V * sizeof(T)) + (unsigned)(R * 16) : 0x80000000u);
      T* xl = xs + (size_t)(wave * NQ + q) * R * 64 * V + lane * V;
#pragma unroll
      for (int jj = 0; jj < R; ++jj) {
#pragma unroll
        for (int e = 0; e < V; ++e) { rr[q][jj].v[e] = 0; pp[q][jj].v[e] = 0; }
        if (has[q]) {
          rr[q][jj] = bld<T, V>(Rr, vT[q], (unsigned)(j0[q] + jj) * rowT);
          pp[q][jj] = bld<T, V>(Rp, vT[q], (unsigned)(j0[q] + jj) * rowT);
          // (the two-kernel path defers x += alpha p of its last iteration to the next K1: applied here, on entry)
          Vec<T, V> xv = bld<T, V>(Rx, vT[q], (unsigned)(j0[q] + jj) * rowT);
#pragma unroll
          for (int e = 0; e < V; ++e) xv.v[e] = fma(alpha0, pp[q][jj].v[e], xv.v[e]);
          stv<T, V>(xl + jj * 64 * V, xv);
        }
      }
      // the ring: rows below / above (out of range beyond a wall -> 0) and the two neighbouring columns
      // (lane l < R: left neighbour of row l, lane R + l: right neighbour; other lanes and walls read 0)
      const int jb = row_wrap(j0[q] - 1, vb[q]), ja = row_wrap(j0[q] + R, va[q]);
      // SLAB: no wrap inside a slab - beyond its edges lies a neighbour's row (or a wall), which r and p carry as halo rows: through
      // resources that start one row lower
      if constexpr (SLAB) { vb[q] = !(ef[q] & 4u) || (ef[q] & 1u); va[q] = !(ef[q] & 8u) || (ef[q] & 2u); }
      const unsigned hb = (has[q] && vb[q]) ? vT[q] : 0xffffffffu, ha = (has[q] && va[q]) ? vT[q] : 0xffffffffu;
      const rsrc_t RrN = SLAB ? make_rsrc(a.r - nx, nbytesH) : Rr, RpN = SLAB ? make_rsrc(a.p[k_begin & 1] - nx, nbytesH) : Rp;
      const int rb = SLAB ? j0[q] : jb, ra = SLAB ? j0[q] + R + 1 : ja;
      rhb[q] = bld<T, V>(RrN, hb, (unsigned)rb * rowT);
      rha[q] = bld<T, V>(RrN, ha, (unsigned)ra * rowT);
      pnb[q] = bld<T, V>(RpN, hb, (unsigned)rb * rowT);
      pna[q] = bld<T, V>(RpN, ha, (unsigned)ra * rowT);
      if constexpr (kParkHalos) {                            // parked at once: no register of the entry survives into the loop
        T* hs = halo_s + (size_t)((wave * NQ + q) * 2) * 64 * V + lane * V;
        stv<T, V>(hs, pnb[q]);
        stv<T, V>(hs + 64 * V, pna[q]);
      }
      int side, er;
      ring_lane(lane, R, side, er);
      int cc = (side == 0) ? tx0[q] * 64 * V - 1 : (tx0[q] + 1) * 64 * V;
      vl[q] = tx0[q] > 0 || a.per_x;
      vr[q] = tx0[q] + 1 < c.ntx || a.per_x;
      // ONE scalar of neighbour bits per region for the loop (bit 0 / 1: cells below / above, bit 2 / 3: left / right, bits 8.. / 16..:
      // the rows the halo loads read), opaque to the optimiser and made opaque again at every use: as four booleans per region
      // they lived in eight SGPR pairs across the row loops (spilled), and the selects "resource of no bytes beyond a wall" were
      // hoisted out of the loop as VECTOR values - the halo loads' resources were then rebuilt in four waterfall loops per iteration
      nbits[q] = (vb[q] ? 1u : 0u) | (va[q] ? 2u : 0u) | (vl[q] ? 4u : 0u) | (vr[q] ? 8u : 0u);
      nbits[q] = (unsigned)__builtin_amdgcn_readfirstlane((int)nbits[q]);
      asm volatile("" : "+s"(nbits[q]));
      if (cc < 0) cc = a.per_x ? nx - 1 : -1;
      else if (cc >= nx) cc = a.per_x ? 0 : -1;
      const unsigned vo = (has[q] && side < 2 && cc >= 0) ? (unsigned)(j0[q] + er) * rowT + (unsigned)(cc * sizeof(T)) : 0xffffffffu;
      eR[q] = bld1<T>(Rr, vo, 0);
      edge[q] = bld1<T>(Rp, vo, 0);
    }
  }
  CgState st = a.state[sv & 1];
  T pz = uniform(a.scal[SC_PZ]), vs = uniform(a.scal[SC_VS]), alpha = uniform(a.scal[SC_ALPHA]);
  const T sc_c = uniform(a.scal[SC_C]);
  T ncells = (T)((double)nx * (double)ny);
  if constexpr (SLAB) ncells = (T)sl.ncells;
  if constexpr (RAGGED) ncells = (T)a.ncells;
  ncells = uniform(ncells);                                 // (in scalar registers, not in a vector register pair held across the loop)
  // RAGGED: are my columns / the columns next to my strip / the rows around my regions cells of the true system?
  bool col_ok[NQ], lcol_ok[NQ], rcol_ok[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    col_ok[q] = !RAGGED || (tx0[q] * 64 + lane) * V < a.nx_true;         // (nx_true is a multiple of V: a lane's cells are all in or all out)
    lcol_ok[q] = !RAGGED || tx0[q] * 64 * V - 1 < a.nx_true;
    rcol_ok[q] = !RAGGED || (tx0[q] + 1) * 64 * V < a.nx_true;
  }
  // totals of the previous K2 (or previous segment): r.z', sum r, #cells with |r| >= accuracy
  T tB[3];
  {
    T s[3] = {0, 0, 0};
    if (wave == 0) {
      for (int b = lane; b < a.nB; b += 64) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += a.partsB[q * kMaxPartials + b];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] = wave_sum(s[q]);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) smem[q] = s[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) tB[q] = uniform(smem[q]);
    __syncthreads();
    if constexpr (SLAB) {                                   // the all-reduced totals of the previous K2 / segment
#pragma unroll
      for (int q = 0; q < 3; ++q) tB[q] = uniform(a.gB[q]);
    }
  }

  // ---- 2 COEFFICIENT PIPELINE (as in cg_persist) and the lambdas of the row loops: both passes of an iteration stream the coefficient rows of my regions in
  // the same order; the loads of row t + D are issued when row t has been consumed, circularly.
  constexpr int coef_regs = ((SYM ? 2 : 4) * (int)sizeof(CT) * V + (RECON ? 0 : (int)sizeof(T) * V)) / 4;   // VGPRs of a row in flight
  constexpr int NT = NQ * R;
  // (the deep pipeline pays where the loop has registers to spare: the slab variant and the four-array / fp64-coefficient variants
  // keep the round-2 depth, they spill otherwise)
  constexpr bool kDeep = NQ == 1 && NT == 16 && SYM && RECON && sizeof(T) == 8;
  constexpr int depth_max = kDeep ? PISO_PERSIST1_DEPTH : ((NQ == 1) ? 3 : kPersistMaxDepth);
  // (small regions whose rows carry the diagonal too - systems with open boundaries, BASELINE config 4: 8 registers per row - get the
  // registers for FOUR rows in flight as well: with regions of 2 rows that is every row of the wave, i.e. the coefficients stay
  // resident as they do with rebuilt diagonals; with two rows in flight both passes waited for L2: 1024 x 256 4.87 against 4.10 us)
  constexpr int budget = kDeep ? 4 * PISO_PERSIST1_DEPTH : ((NQ == 1 || NT < 16) ? ((NT < 16 && !RECON && SYM) ? 32 : 16) : 8);
  constexpr int Dw = budget / coef_regs < 2 ? 2 : (budget / coef_regs > depth_max ? depth_max : budget / coef_regs);
  constexpr int D = (NT >= Dw) ? Dw : NT;
  constexpr int kBaseLoads = (SYM ? 2 : 4) + (RECON ? 0 : 1);          // vector loads every row issues (some rows one or two more)
  Vec<CT, V> cS[NT], cW[NT], cE[NT], cN[NT], cSh[NQ];
  Vec<T, V> cD[NT];
  CT eW[NQ];
  // byte offset of row j0[q] + jj: recomputed at every use (two scalar instructions) from a value the optimiser cannot see
  // through - hoisted out of the unrolled row loops the 2 x 16 products live in SGPRs that spill, and a spilled SGPR comes back
  // through v_readlane, a VALU slot of a loop that is bound by VALU issue
  auto row_base = [&](int q, int jj, unsigned row_bytes) __attribute__((always_inline)) -> unsigned {
    unsigned j = (unsigned)j0[q];
    asm volatile("" : "+s"(j));
    return (j + (unsigned)jj) * row_bytes;
  };
  auto coef_offset = [&](int q) __attribute__((always_inline)) -> unsigned {
    return (unsigned)((unsigned long long)vT[q] * sizeof(CT) / sizeof(T));
  };
  // Both stencil passes stream the S / W rows of the workgroup's cells, 4.19 MB per XCD and pass at 2048^2 - just above the 4 MB of
  // an XCD's L2, so a cyclic sweep misses almost every time and the row loops run at the speed of the memory fabric (measured 33.5 MB
  // in 3.6 us).  Hence the back-and-forth order: D walks the rows of a wave upwards (t = 0 .. NT-1), U walks them downwards.  The coefficient rows a pass ends with are
  // the rows the next pass starts with: they are still in registers (Dc rows per turn are never reloaded) and the rows behind them
  // are the most recently used lines of the XCD's L2 - a cyclic sweep over a set just above the L2's capacity misses every time,
  // a back-and-forth sweep misses only what does not fit.  (Measured before: both row loops ran at the speed of the memory
  // fabric, ~6 TB/s of coefficient rows, not at the speed of their arithmetic.)
  // kAhead: z' = L p of the first rows of the U pass does not depend on alpha - it is computed WHILE the exchange's records travel
  // (behind the publish, in front of the polling: the SIMDs have nothing else to do for a microsecond or two) and kept in
  // registers; U then skips the stencil of those rows.  With the back-and-forth order these are the rows D ended with: their
  // coefficients are still in registers.  Same instructions on the same registers as D's z': bitwise the same values.
  constexpr int kAhead = (!LOCAL && NQ == 1 && NT == 16 && SYM && RECON && sizeof(T) == 8 && sizeof(CT) == 4) ? PISO_PERSIST1_AHEAD : 0;
  static_assert(kAhead <= Dw || kAhead == 0, "the rows computed ahead are rows whose coefficients D left in registers");
  constexpr bool kShLate = kAhead > 0 && !SLAB && NQ == 1 && SYM;
  // kKeepZ (small regions: a wave's rows are few): z' of D stays in registers until U has used it - U runs no stencil at all (the
  // 16-row instances have no registers for it: they compute z' twice, bitwise the same, and kAhead moves part of that off the path)
  constexpr bool kKeepZ = NT * (int)sizeof(T) * V / 4 <= PISO_PERSIST1_KEEP_Z_REGS;
  // kCountLate (16-row regions, round 6): the residual count is taken in a pass of its own, only in the iterations whose count the
  // stopping test reads ((k + 1) % 5 == 0): 32 fp64 compares less per wave in 4 of 5 iterations of a loop bound by VALU issue
  // (A/B on one box, four rounds: 10.19 - 10.32 against 10.22 - 10.48 us per iteration).  Small regions keep the count in the row loop:
  // their iteration is a latency chain, a branch more on it buys nothing.
  constexpr bool kCountLate = NT == 16 && !RAGGED;
  auto issue_coef = [&](int t) __attribute__((always_inline)) {
    const int q = t / R, jj = t - q * R;
    const unsigned vCq = coef_offset(q);
    const unsigned sT = row_base(q, jj, rowT), sC = row_base(q, jj, rowC);
    cS[t] = bld<CT, V>(RoS, vCq, sC); cW[t] = bld<CT, V>(RoW, vCq, sC);
    if constexpr (!SYM) { cE[t] = bld<CT, V>(RoE, vCq, sC); cN[t] = bld<CT, V>(RoN, vCq, sC); }
    if constexpr (!RECON) cD[t] = bld<T, V>(RcC, vT[q], sT);
  };
  // SYM: W of the first column of the strip to the right (E of my last column; lane R + jj: row jj) and S of the row above the
  // region (N of my last row).  Constants of the launch: loaded ONCE - reloading them with rows 0 / R-1 of every pass put a full
  // memory trip in front of the rows that still used them (0.55 us per iteration at 2048^2).
  // LDS byte address of this wave's ring block, kept in a VGPR (ds instructions take their address from one) and made opaque
  // before every use: the optimiser then cannot merge the reads of the D pass with those of the U pass (which would keep 5
  // registers per row alive across the exchange) and leaves each read where it is issued
  typedef __attribute__((address_space(3))) T lds_T;
  typedef __attribute__((address_space(3))) CT lds_CT;
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  unsigned ring_a = (unsigned)(unsigned long)(lds_u8*)ring_s + (unsigned)(wave * NQ * kRingBytes);
  asm volatile("" : "+v"(ring_a));
  if constexpr (kRingLds) {                                  // the entry's ring columns go to the wave's block at once
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const unsigned rb = ring_a + (unsigned)(q * kRingBytes) + (unsigned)lane * (unsigned)sizeof(T);
      *(lds_T*)(unsigned long)rb = edge[q];
      *(lds_T*)(unsigned long)(rb + kRingR) = eR[q];
    }
  }
  if constexpr (SYM) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int side, er;
      ring_lane(lane, R, side, er);
      int cc = (tx0[q] + 1) * 64 * V;
      if (cc >= nx) cc = a.per_x ? 0 : -1;
      const unsigned vo = (has[q] && side == 1 && cc >= 0) ? (unsigned)(j0[q] + er) * rowC + (unsigned)(cc * sizeof(CT)) : 0xffffffffu;
      eW[q] = bld1<CT>(RoW, vo, 0);
      if constexpr (kRingLds)
        *(lds_CT*)(unsigned long)(ring_a + (unsigned)(q * kRingBytes + 64 * (int)sizeof(T)) + (unsigned)lane * (unsigned)sizeof(CT)) = eW[q];
      bool valid;
      const int jw = row_wrap(j0[q] + R, valid);
      if (SLAB && (ef[q] & 8u)) cSh[q] = bld<CT, V>(RoN, has[q] ? coef_offset(q) : 0xffffffffu, (unsigned)(ny - 1) * rowC);   // N of my last row
      else
      cSh[q] = bld<CT, V>(RoS, (has[q] && valid) ? coef_offset(q) : 0xffffffffu, (unsigned)jw * rowC);
    }
  }
  // kShLate (with kAhead, one 16-row region, no slab edge): S of the row above the region is requested again in every D pass together
  // with the coefficients of the region's last row - its registers are then free from the rows computed ahead to the next request
  // (across U and the first rows of D) instead of held for the whole launch
  auto reload_csh = [&]() __attribute__((always_inline)) {
    if constexpr (SYM && NQ == 1) {
      bool valid;
      const int jw = row_wrap(j0[0] + R, valid);
      cSh[0] = bld<CT, V>(RoS, (has[0] && valid) ? coef_offset(0) : 0xffffffffu, (unsigned)jw * rowC);
    }
  };
  // the ring values of row t (every lane receives them; lanes 0 / 63 are the ones that matter): issued one row ahead
  T rgl[NT], rgr[NT];
  CT rgw[NT];
  auto ring_issue = [&](int t) __attribute__((always_inline)) {
    if constexpr (!kRingLds) return;
    const int q = t / R, jj = t - q * R;
    asm volatile("" : "+v"(ring_a));
    const unsigned base = ring_a + (unsigned)(q * kRingBytes);
    rgl[t] = *(const lds_T*)(unsigned long)(base + (unsigned)(jj * (int)sizeof(T)));
    rgr[t] = *(const lds_T*)(unsigned long)(base + (unsigned)((48 + jj) * (int)sizeof(T)));
    if constexpr (SYM) rgw[t] = *(const lds_CT*)(unsigned long)(base + (unsigned)(64 * (int)sizeof(T) + (48 + jj) * (int)sizeof(CT)));
  };
  // z' = L p of row t of my regions: summation order of calcZ_v4 (pressure_solve_op.cu.cc:81-90).  D and U both call this on
  // the same registers, so they see bitwise the same z'.
  auto zrow = [&](int t) __attribute__((always_inline)) -> Vec<T, V> {
    const int q = t / R, jj = t - q * R;
    T* hs = halo_s + (kParkHalos ? (size_t)((wave * NQ + q) * 2) * 64 * V + lane * V : 0);
    const Vec<T, V> behind = (jj > 0) ? pp[q][jj > 0 ? jj - 1 : 0] : (kParkHalos ? ldv<T, V>(hs) : pnb[q]);
    const Vec<T, V> cur = pp[q][jj];
    const Vec<T, V> ahead = (jj + 1 < R) ? pp[q][jj + 1 < R ? jj + 1 : jj] : (kParkHalos ? ldv<T, V>(hs + (kParkHalos ? 64 * V : 0)) : pna[q]);
    const T left = kRingLds ? shift_lane<true, T>(cur.v[V - 1], rgl[t]) : shift_ring<true, T>(cur.v[V - 1], edge[q], jj);
    const T right = kRingLds ? shift_lane<false, T>(cur.v[0], rgr[t]) : shift_ring<false, T>(cur.v[0], edge[q], jj);
    Vec<CT, V> kN, kE;
    if constexpr (SYM) {
      kN = (jj + 1 < R) ? cS[t + 1 < NT ? t + 1 : t] : cSh[q];
#pragma unroll
      for (int e = 0; e + 1 < V; ++e) kE.v[e] = cW[t].v[e + 1];
      kE.v[V - 1] = kRingLds ? shift_lane<false, CT>(cW[t].v[0], rgw[t]) : shift_ring<false, CT>(cW[t].v[0], eW[q], jj);
    } else {
      kN = cN[t]; kE = cE[t];
    }
    Vec<T, V> kC, z;
    if constexpr (RECON) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        T d = -(T)cS[t].v[e] - (T)kN.v[e];                    // = (0 - S) - N: the first difference of laplace_op.cu.cc:118-135 is exact
        d -= (T)cW[t].v[e]; d -= (T)kE.v[e];
        kC.v[e] = d;
      }
    } else {
      kC = cD[t];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const T pw = (e == 0) ? left : cur.v[e > 0 ? e - 1 : 0];
      const T pe = (e == V - 1) ? right : cur.v[e < V - 1 ? e + 1 : 0];
      T tmp = 0;
      tmp = fma((T)cS[t].v[e], behind.v[e], tmp);
      tmp = fma((T)cW[t].v[e], pw, tmp);
      tmp = fma(kC.v[e], cur.v[e], tmp);
      tmp = fma((T)kE.v[e], pe, tmp);
      tmp = fma((T)kN.v[e], ahead.v[e], tmp);
      z.v[e] = tmp;
    }
    return z;
  };
  Vec<T, V> zk[kKeepZ ? NT : 1];                             // kKeepZ: z' of my rows from D to U
  int k = k_begin;                                           // the iteration (SLAB: its parity picks the mailbox rows)
  // perimeter of row jj of region q (what neighbouring regions read): the whole first / last row, else the two end cells
  auto publish = [&](rsrc_t Rd, int q, int jj, const Vec<T, V>& val) __attribute__((always_inline)) {
    const unsigned sT = row_base(q, jj, rowT);
    if (jj == 0 || jj == R - 1) {
      bst<T, V, kPub>(Rd, vT[q], sT, val);
      if constexpr (kPack) bst<T, V, kPub>(Rd, vEnd[q], row_base(q, 1, rowT) + (unsigned)(jj * 16), val);    // (its end cells into the packed block as well)
      if constexpr (SLAB) {
        // my first row is the row ABOVE the lower neighbour's slab (its side 1), my last row the row BELOW the upper one's (side 0)
        if (jj == 0) {
          unsigned zoff;
          const rsrc_t Rm = mailbox_rows((unsigned)offsetof(SlabCtl, rows_lo), k & 1, 1, zoff, (ef[q] & 1u) != 0);
          bst<T, V, kSystem>(Rm, vT[q], zoff, val);
        }
        if (jj == R - 1) {
          unsigned zoff;
          const rsrc_t Rm = mailbox_rows((unsigned)offsetof(SlabCtl, rows_hi), k & 1, 0, zoff, (ef[q] & 2u) != 0);
          bst<T, V, kSystem>(Rm, vT[q], zoff, val);
        }
      }
    } else {
      // the two end cells of the row: lanes 0 and 63 store their cells of the row (16 bytes each; a lane's inner cell is written
      // too and never read), every other lane carries an offset beyond the buffer and its store is dropped by the range check -
      // no exec mask to build, no data to select (2 compares + 2 selects per row in a loop that is bound by VALU issue)
      if constexpr (kPack) {
        bst<T, V, kPub>(Rd, vEnd[q], row_base(q, 1, rowT) + (unsigned)(jj * 16), val);
      } else {
        bst<T, V, kPub>(Rd, vEnd[q], sT, val);
      }
    }
  };
  // z' on the ring, as published by the neighbours (rows below / above, the two neighbouring columns): issued right after
  // the exchange (every record seen = every perimeter store completed), consumed at the END of U - the row loop hides the trip
  T eZ[NQ];
  Vec<T, V> hbZ[NQ], haZ[NQ];
  auto issue_halos = [&](rsrc_t Rz) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int side, er, lane_now = lane;
      asm volatile("" : "+v"(lane_now));                    // (the ring offset is recomputed here: hoisted, it is one more register across the row loops - spilled)
      ring_lane(lane_now, R, side, er);
      int cc = (side == 0) ? tx0[q] * 64 * V - 1 : (tx0[q] + 1) * 64 * V;
      if (cc < 0) cc = a.per_x ? nx - 1 : -1;
      else if (cc >= nx) cc = a.per_x ? 0 : -1;
      unsigned vo = (side < 2 && cc >= 0) ? (unsigned)(j0[q] + er) * rowT + (unsigned)(cc * sizeof(T)) : 0xffffffffu;
      if constexpr (kPack) {
        // the neighbouring strip's packed block: its side-1 entry (its lane 63, whose last cell is my left neighbour) or its side-0
        // entry (its lane 0, first cell), row `er`
        const int strip = (cc >= 0) ? cc / (64 * V) : 0;
        const unsigned ent = (side == 0) ? (unsigned)(R * 16 + er * 16 + (V - 1) * (int)sizeof(T)) : (unsigned)(er * 16);
        vo = (side < 2 && cc >= 0) ? (unsigned)(j0[q] + 1) * rowT + (unsigned)(strip * 64 * V * (int)sizeof(T)) + ent : 0xffffffffu;
      }
      eZ[q] = bld1<T, kHalo>(Rz, vo, 0);
      bool vbq_unused, vaq_unused;
      const int jb = row_wrap(j0[q] - 1, vbq_unused), ja = row_wrap(j0[q] + R, vaq_unused);
      const bool vbq = nbit(q, 1u), vaq = nbit(q, 2u);
      if constexpr (SLAB) {                                  // (wave-uniform branches: no per-lane offset registers to keep)
        if (!(ef[q] & 4u)) hbZ[q] = bld<T, V, kHalo>(Rz, vT[q], (unsigned)(j0[q] - 1) * rowT);
        else if (ef[q] & 1u) {
          unsigned zoff;
          const rsrc_t Rm = mailbox_rows((unsigned)offsetof(SlabCtl, rows_own), k & 1, 0, zoff);
          hbZ[q] = bld<T, V, kSystem>(Rm, vT[q], zoff);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) hbZ[q].v[e] = 0;
        }
        if (!(ef[q] & 8u)) haZ[q] = bld<T, V, kHalo>(Rz, vT[q], (unsigned)(j0[q] + R) * rowT);
        else if (ef[q] & 2u) {
          unsigned zoff;
          const rsrc_t Rm = mailbox_rows((unsigned)offsetof(SlabCtl, rows_own), k & 1, 1, zoff);
          haZ[q] = bld<T, V, kSystem>(Rm, vT[q], zoff);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) haZ[q].v[e] = 0;
        }
      } else {
      // (beyond a wall: a resource of no bytes - the load is dropped by the range check and returns 0; a per-lane offset that says
      // the same is one more vector register across the row loops)
      hbZ[q] = bld<T, V, kHalo>(make_rsrc(a.zp[k & 1], (unsigned)__builtin_amdgcn_readfirstlane((int)(vbq ? nbytesT : 0u))), vT[q], (unsigned)jb * rowT);
      haZ[q] = bld<T, V, kHalo>(make_rsrc(a.zp[k & 1], (unsigned)__builtin_amdgcn_readfirstlane((int)(vaq ? nbytesT : 0u))), vT[q], (unsigned)ja * rowT);
      }
    }
  };
  if (has[0]) {
#pragma unroll
    for (int t = 0; t < D; ++t) issue_coef(t);
  }

  unsigned epoch = c.epoch0;
  bool healthy = true, first = true;
  unsigned long long tacc[5] = {0, 0, 0, 0, 0}, tsub[4] = {0, 0, 0, 0};
  PhaseClock clk((kPersistDiag && c.timing) ? tacc : nullptr);   // diagnostic builds only (-DPISO_PERSIST_DIAG): D / exchange / U clocks
  // the stopping test of iteration k_begin was left to this launch by the previous one (pressure_solve_op.cu.cc:312-335)
  if (!st.done && k > 0 && (k % 5) == 0) {                  // (!done: a launch queued behind a converged one changes nothing)
    const int exceeded = tB[2] > 0;
    if (st.flag && !exceeded) { st.done = 1; st.iterations = k; }
    else st.flag = 1;
  }
  T rz_next = tB[0], sumr = tB[1], cnt_last = tB[2];          // r_k.z'_{k-1}, sum r_k, #{|r_k| >= accuracy} for the current k
  T lU[2] = {0, 0};                                           // local sum r, count from the last U (for the next exchange)
  const T accuracy = uniform((T)a.accuracy);
  // beta of iteration k needs nothing but the sums of exchange k - 1: it is computed right behind them, in the shadow of U's wait for
  // the neighbours' rows, instead of as a dependent chain of ~25 instructions in front of D (same expression, same operands)
  T beta = uniform(-(rz_next + vs * sumr) / pz);              // (:351-352), unguarded as coded
  for (; k < k_end && healthy && !st.done; ++k) {
    // consecutive iterations alternate buffers: a neighbour's loads of z'_k are consumed before it publishes its record k + 1,
    // which everybody needs before writing the same buffer again in iteration k + 2
    rsrc_t Rz;
    // (16-row regions and the slab instances are short of scalar registers: the buffer's address comes from the kernarg segment, not
    // from four SGPRs held across the loop - 83 -> 58 spilled SGPRs in the 16-row slab instance, 28 -> 23 in the plain one.  Small
    // regions keep the descriptors: their iteration is a latency chain and the scalar load sits on it - 256^2 2.70 -> 2.79 us)
    if constexpr (SLAB || NT == 16) {
      typedef CgArgs<T> A;
      Rz = make_rsrc(karg<T*>((unsigned)offsetof(KArgs, a) + (unsigned)offsetof(A, zp) + 8u * (unsigned)(k & 1)), nbytesT);
    } else {
      Rz = (k & 1) ? Rz1 : Rz0;
    }
    // ---- 3 D(k): p = r + beta p on my cells and on the ring; z' = L p; sums; the perimeter of z' goes out
    T sD[kX1Values] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (has[0]) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
#pragma unroll
          for (int e = 0; e < V; ++e) pp[q][jj].v[e] = fma(beta, pp[q][jj].v[e], rr[q][jj].v[e]);
        }
        if constexpr (kRingLds) {
          const unsigned rb = ring_a + (unsigned)(q * kRingBytes) + (unsigned)lane * (unsigned)sizeof(T);
          const T e_old = *(lds_T*)(unsigned long)rb, r_col = *(lds_T*)(unsigned long)(rb + kRingR);
          *(lds_T*)(unsigned long)rb = fma(beta, e_old, r_col);
        } else {
          edge[q] = fma(beta, edge[q], eR[q]);
        }
        T* hs = halo_s + (kParkHalos ? (size_t)((wave * NQ + q) * 2) * 64 * V + lane * V : 0);
        if constexpr (kParkHalos) {
          pnb[q] = ldv<T, V>(hs); pna[q] = ldv<T, V>(hs + 64 * V);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          pnb[q].v[e] = fma(beta, pnb[q].v[e], rhb[q].v[e]);
          pna[q].v[e] = fma(beta, pna[q].v[e], rha[q].v[e]);
        }
        if constexpr (kParkHalos) {
          stv<T, V>(hs, pnb[q]);
          stv<T, V>(hs + 64 * V, pna[q]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      ring_issue(0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int q = t / R, jj = t - q * R;
        if (t + 1 < NT) ring_issue(t + 1);
        const Vec<T, V> z = zrow(t);
        if constexpr (kKeepZ) zk[t] = z;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          sD[0] += pp[q][jj].v[e];
          sD[1] = fma(pp[q][jj].v[e], rr[q][jj].v[e], sD[1]);
          sD[2] = fma(pp[q][jj].v[e], z.v[e], sD[2]);
          sD[3] = fma(rr[q][jj].v[e], z.v[e], sD[3]);
          sD[4] = fma(z.v[e], z.v[e], sD[4]);
          sD[5] += z.v[e];
        }
        publish(Rz, q, jj, z);
        PISO_SB_A1;
        // (rows 0 .. D-1 of the U pass are issued behind the drain of the perimeter stores, see the exchange: issued here they would
        // be in flight when the wave waits for vmcnt(0), and the wait would cover their trip as well)
        if constexpr (D < NT) { if (t + D < NT) issue_coef(t + D); }
        if constexpr (kShLate) { if (t + D == NT - 1) reload_csh(); }
        PISO_SB_A2;
      }
    }
    // ---- 4 EXCHANGE + SCALARS: the eight sums of all workgroups (with z' of U's first rows computed while the records travel), the
    // stopping test, alpha and beta
    sD[6] = lU[0]; sD[7] = lU[1];
    ++epoch;
    clk.split(0);
    Vec<T, V> zs[kAhead > 0 ? kAhead : 1];
    auto z_ahead = [&]() __attribute__((always_inline)) {
      if constexpr (kAhead > 0) {
        if (has[0]) {
          ring_issue(NT - 1);
#pragma unroll
          for (int tt = 0; tt < kAhead; ++tt) {
            if (tt + 1 < kAhead) ring_issue(NT - 2 - tt);
            zs[tt] = zrow(NT - 1 - tt);
          }
        }
      }
    };
    if constexpr (LOCAL) healthy = grid_exchange8_local<T>(c, sD, epoch, smem, slot, nslots, hier_s + 2, (kPersistDiag && c.timing) ? tsub : nullptr);
    else healthy = grid_exchange8_hier<T, (SLAB ? kPollDelay2Xg : (kAhead > 0 ? kPollDelay2 : kPollDelay2NoAhead)), SLAB>(c, sD, epoch, smem, hx, hier_s + 2, z_ahead, (kPersistDiag && c.timing) ? tsub : nullptr, sl_off, smem + 2 * kX1Sm);
    clk.split(1);
    if (!healthy) break;
    // the stopping test of iteration k, one exchange late but before anything moves (x = x_k): (:312-335)
    if (!first) {
      sumr = sD[6]; cnt_last = sD[7];
      if (k > 0 && (k % 5) == 0) {
        const int exceeded = cnt_last > 0;
        if (st.flag && !exceeded) { st.done = 1; st.iterations = k; }
        else st.flag = 1;
      }
      if (st.done) break;
    }
    first = false;
    // alpha (:301-302) and, by one-step recurrences from the direct sums, what beta of the next iteration needs
    vs = uniform(sc_c * sD[0]);
    pz = uniform(sD[2] + vs * sD[0]);
    alpha = uniform((absval(pz) > 0) ? sD[1] / pz : (T)0);
    rz_next = uniform(sD[3] - alpha * (sD[4] + vs * sD[5]));
    sumr = uniform(sumr - alpha * (sD[5] + ncells * vs));
    beta = uniform(-(rz_next + vs * sumr) / pz);             // ... of iteration k + 1 (see above)
    // ---- 5 U(k): z' again, x += alpha p, r -= alpha (z' + vs) on my cells and on the ring
    lU[0] = 0; lU[1] = 0;
    int cnt_wave = 0;                                        // #{|r_{k+1}| >= accuracy} of the whole wave, counted on the scalar unit
    if (has[0]) {
      issue_halos(Rz);                                       // (requested later in U, the stall moves into D: measured)
      if constexpr (kAhead < NT && !kKeepZ) ring_issue(NT - 1 - kAhead);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int t = NT - 1 - tt;                          // U walks the rows downwards
        const int q = t / R, jj = t - q * R;
        if constexpr (!kKeepZ) { if (tt + 1 < NT && tt + 1 > kAhead) ring_issue(t - 1); }     // (row kAhead's values were requested in front of the loop)
        T* xl = xs + (size_t)(wave * NQ + q) * R * 64 * V + lane * V + jj * 64 * V;
        Vec<T, V> xv = ldv<T, V>(xl);                        // x += alpha p (:303); the LDS latency hides under the stencil
        Vec<T, V> z;
        if constexpr (kKeepZ) z = zk[t];
        else z = (tt < kAhead) ? zs[tt < kAhead ? tt : 0] : zrow(t);
#pragma unroll
        for (int e = 0; e < V; ++e) xv.v[e] = fma(alpha, pp[q][jj].v[e], xv.v[e]);
        stv<T, V>(xl, xv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          T vsc = vs;
          if constexpr (RAGGED) vsc = (col_ok[q] && j0[q] + jj < a.ny_true) ? vs : (T)0;
          const T rn = fma(-alpha, z.v[e] + vsc, rr[q][jj].v[e]);
          rr[q][jj].v[e] = rn;
          lU[0] += rn;
          if constexpr (!kCountLate) {
            // (one compare per cell; ballot + popcount + add run on the scalar unit - the loop is bound by VALU issue.  A NaN counts.)
            // (inline asm: left to the compiler the sixteen rows' masks are parked in VGPR lanes - v_writelane / v_readlane pairs,
            // VALU slots - and counted after the loop)
            const unsigned long long over = __ballot(!(absval(rn) < accuracy));
            int ones;
            asm volatile("s_bcnt1_i32_b64 %1, %2\n\ts_add_i32 %0, %0, %1" : "+s"(cnt_wave), "=&s"(ones) : "s"(over) : "scc");
          }
        }
        PISO_SB_B1;
        if constexpr (D < NT) {
          if (t - D >= 0) issue_coef(t - D);                 // downwards; rows D-1 .. 0 stay in registers for the next D pass
        }
        PISO_SB_B2;
      }
      if constexpr (kCountLate) {
        // #{|r_{k+1}| >= accuracy} is looked at by the stopping test of iteration k + 1 only if (k + 1) % 5 == 0 (:312-335): counted in a
        // pass of its own over the registers, in those iterations only (one wave-uniform branch; 32 fp64 compares less in 4 of 5 iterations)
        if ((k + 1) % 5 == 0) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int q = t / R, jj = t - q * R;
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const unsigned long long over = __ballot(!(absval(rr[q][jj].v[e]) < accuracy));
              int ones;
              asm volatile("s_bcnt1_i32_b64 %1, %2\n\ts_add_i32 %0, %0, %1" : "+s"(cnt_wave), "=&s"(ones) : "s"(over) : "scc");
            }
          }
        }
      }
      // the ring: the same update with the neighbours' z' (beyond a wall there is no cell: the copies stay 0)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        T vsb = nbit(q, 1u) ? vs : (T)0, vsa = nbit(q, 2u) ? vs : (T)0;
        if constexpr (RAGGED) {
          if (!(col_ok[q] && j0[q] - 1 < a.ny_true)) vsb = 0;
          if (!(col_ok[q] && j0[q] + R < a.ny_true)) vsa = 0;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          rhb[q].v[e] = fma(-alpha, hbZ[q].v[e] + vsb, rhb[q].v[e]);
          rha[q].v[e] = fma(-alpha, haZ[q].v[e] + vsa, rha[q].v[e]);
        }
        int side, er_unused, lane_now = lane;
        if constexpr (SLAB) asm volatile("" : "+v"(lane_now));   // (slab variant: recomputed here instead of a register held across the loop)
        ring_lane(lane_now, R, side, er_unused);
        T vse = (side == 0) ? (nbit(q, 4u) ? vs : (T)0) : ((side == 1) ? (nbit(q, 8u) ? vs : (T)0) : (T)0);
        if constexpr (RAGGED) {
          const bool ok = (side == 0 ? lcol_ok[q] : rcol_ok[q]) && j0[q] + er_unused < a.ny_true;
          if (!ok) vse = 0;
        }
        if constexpr (kRingLds) {
          const unsigned rb = ring_a + (unsigned)(q * kRingBytes) + (unsigned)lane * (unsigned)sizeof(T) + kRingR;
          *(lds_T*)(unsigned long)rb = fma(-alpha, eZ[q] + vse, (T) * (lds_T*)(unsigned long)rb);
        } else {
          eR[q] = fma(-alpha, eZ[q] + vse, eR[q]);
        }
      }
      lU[1] = (lane == 0) ? (T)cnt_wave : (T)0;              // (the exchange adds the lanes of a wave)
    }
    clk.split(2);
  }
  if (kPersistDiag && c.timing && threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) c.timing[q * nslots + slot] += tacc[q];            // (XCD-local mode: the group's ranks, not the launch's blocks)
#pragma unroll
    for (int q = 0; q < 4; ++q) c.timing[(5 + q) * nslots + slot] += tsub[q];
    c.timing[9 * nslots + slot] = (unsigned long long)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7);   // the XCD I ran on
    c.timing[10 * nslots + slot] = (unsigned long long)wg;                                                              // the band of regions I own
  }
  // ---- 6 EXIT.  The last U's sum r and count are only known per workgroup: one more exchange (once per segment)
  T tOut[3] = {rz_next, sumr, cnt_last};
  if (!first && healthy && !st.done) {
    T sX[kX1Values] = {0, 0, 0, 0, 0, 0, lU[0], lU[1]};
    ++epoch;
    if constexpr (LOCAL) healthy = grid_exchange8_local<T>(c, sX, epoch, smem, slot, nslots, hier_s + 2);
    else healthy = grid_exchange8_hier<T, kPollDelay2NoAhead, SLAB>(c, sX, epoch, smem, hx, hier_s + 2, NoPrefetch(), nullptr, sl_off, smem + 2 * kX1Sm);     // (nothing to compute ahead)
    tOut[1] = sX[6]; tOut[2] = sX[7];
  }

  // back to the global-memory state of the two-kernel path (iteration k reads its direction from p[k & 1])
  // (the pointers of the exit are read again from the kernarg segment: held in SGPRs across the loop they are spilled, and the
  // reloads of OTHER spilled values land in the row loops)
  struct { T *r, *x, *pk, *partsB, *scal; const T* gB; CgState* state; int nB; } ax;       // (pk: p[k & 1])
  struct { int* err; } cx;
  {
    typedef CgArgs<T> A;
    constexpr unsigned ao = (unsigned)offsetof(KArgs, a), co = (unsigned)offsetof(KArgs, c);
    ax.r = karg<T*>(ao + (unsigned)offsetof(A, r)); ax.x = karg<T*>(ao + (unsigned)offsetof(A, x));
    ax.pk = karg<T*>(ao + (unsigned)offsetof(A, p) + 8u * (unsigned)(k & 1));
    ax.partsB = karg<T*>(ao + (unsigned)offsetof(A, partsB)); ax.scal = karg<T*>(ao + (unsigned)offsetof(A, scal));
    ax.gB = karg<const T*>(ao + (unsigned)offsetof(A, gB)); ax.state = karg<CgState*>(ao + (unsigned)offsetof(A, state));
    ax.nB = karg<int>(ao + (unsigned)offsetof(A, nB));
    cx.err = karg<int*>(co + (unsigned)offsetof(PersistCtl, err));
  }
  {
    const rsrc_t Rr = make_rsrc(ax.r, nbytesT), Rx = make_rsrc(ax.x, nbytesT), Rp = make_rsrc(ax.pk, nbytesT);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (has[q]) {
        T* xl = xs + (size_t)(wave * NQ + q) * R * 64 * V + lane * V;
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
          const unsigned sT = (unsigned)(j0[q] + jj) * rowT;
          bst<T, V>(Rr, vT[q], sT, rr[q][jj]);
          bst<T, V>(Rp, vT[q], sT, pp[q][jj]);
          bst<T, V>(Rx, vT[q], sT, ldv<T, V>(xl + jj * 64 * V));
        }
        if constexpr (SLAB) {                               // the two-kernel slab path continues from the halo rows of r and p
          const rsrc_t RrH = make_rsrc(ax.r - nx, nbytesH), RpH = make_rsrc(ax.pk - nx, nbytesH);
          T* hs = halo_s + (kParkHalos ? (size_t)((wave * NQ + q) * 2) * 64 * V + lane * V : 0);
          if constexpr (kParkHalos) { pnb[q] = ldv<T, V>(hs); pna[q] = ldv<T, V>(hs + 64 * V); }
          if (ef[q] & 1u) { bst<T, V>(RrH, vT[q], 0u, rhb[q]); bst<T, V>(RpH, vT[q], 0u, pnb[q]); }
          if (ef[q] & 2u) { bst<T, V>(RrH, vT[q], (unsigned)(ny + 1) * rowT, rha[q]); bst<T, V>(RpH, vT[q], (unsigned)(ny + 1) * rowT, pna[q]); }
        }
      }
  }
  if (wg == 0) {                                           // (= blockIdx.x 0, or the first arrival of the XCD-local group)
    // the next launch (cg_k1 with do_check, or another segment) finds the last K2-totals in record 0 of partsB
    for (int b = threadIdx.x; b < ax.nB; b += kPersistThreads) {
#pragma unroll
      for (int q = 0; q < 3; ++q) ax.partsB[q * kMaxPartials + b] = (b == 0) ? tOut[q] : (T)0;
    }
    if constexpr (SLAB) {
      if (threadIdx.x == 0) { T* g = const_cast<T*>(ax.gB); g[0] = tOut[0]; g[1] = tOut[1]; g[2] = tOut[2]; }   // (already summed over all GPUs)
    }
    if (threadIdx.x == 0) {
      ax.scal[SC_PZ] = pz; ax.scal[SC_VS] = vs; ax.scal[SC_ALPHA] = alpha;
      ax.state[0] = st; ax.state[1] = st;
      if (!healthy) *cx.err = 1;
    }
  }
}

}  // namespace piso
