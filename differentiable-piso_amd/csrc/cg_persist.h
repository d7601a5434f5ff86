// What the persistent CG kernels share (cg_persist1.h: the segment kernel; cg_tiny.h: one workgroup; cg_slab.hip: the slab
// variant): launch shape, the control block, wave-level helpers on the DPP network, buffer-resource loads / stores with a cache
// policy, lane shifts, kernel arguments read again from the kernarg segment - and the GRID EXCHANGE of the segment kernel, whole:
// record format, lane reductions, the tree over the XCDs (grid_exchange8_hier, with the node level of the slab instance) and its
// XCD-local sibling (grid_exchange8_local).  (Rounds 1-2 also kept a first persistent kernel here - two grid exchanges per iteration with the reference's
// recurrences, z' never stored; `cg_persist1` replaced it for fp64 in round 2 and for fp32 in round 3, DESIGN.md 3.1 has its
// measurements.)
#pragma once
#include <cstddef>

#include "cg_kernels.h"
#include "peer.h"

// scheduling fences of the two row loops (measured: with / without them the iteration time is the same; they keep the
// register allocation of the unrolled loops predictable)
#define PISO_SB_A1 __builtin_amdgcn_sched_barrier(0)
#define PISO_SB_A2 __builtin_amdgcn_sched_barrier(0)
#define PISO_SB_B1 __builtin_amdgcn_sched_barrier(0)
#define PISO_SB_B2 __builtin_amdgcn_sched_barrier(0)

namespace piso {

constexpr int kPersistThreads = 512;            // 8 waves per CU = 2 per SIMD -> 256 VGPRs per lane: state in registers without spills
constexpr int kPersistWaves = kPersistThreads / 64;
// region shapes (rows R x regions per wave NQ): 2 x 1, 2 x 2, 4 x 2 and 16 x 1 - at most 16 rows of 128 columns per wave (cg_dispatch.h)

struct PersistCtl {
  unsigned long long* rec;   // exchange records: [2 (parity)][kPersistMaxGrid][8] 8-byte words, zeroed before every launch
  int* err;             // set to 1 if a spin gave up
  int nreg, ntx;        // regions (= waves with work), strips per row
  unsigned epoch0;      // tags of this launch's exchanges are epoch0 + 1, epoch0 + 2, ...: no record of an earlier launch can match
  unsigned long long* timing;   // diagnostics (-DPISO_PERSIST_DIAG + PISO_CG_PERSIST_TIMING): [5][grid] 100 MHz ticks per phase / exchange
  // XCD-local mode of cg_persist1 (small grids: all participating workgroups on ONE XCD, exchanges through that XCD's L2):
  int* xcd;             // [0..7] arrivals per XCD, [8] 1 + the XCD that runs the solve (0: not decided yet); zeroed before every launch
  int local_n;          // workgroups that take part (the launch has 8 x local_n: some XCD is dealt at least local_n of them)
  int waves;            // waves of a workgroup that own regions: 8, or 4 (one per SIMD: nobody waits for a SIMD's other wave; small grids)
};
#ifdef PISO_PERSIST_DIAG
constexpr bool kPersistDiag = true;     // per-phase clocks of wave 0 (PISO_CG_PERSIST_TIMING=1); costs a few registers
#else
constexpr bool kPersistDiag = false;
#endif
constexpr int kPersistMaxGrid = 256;   // workgroups (one per CU); the exchange keeps kPersistMaxGrid / 64 records per lane in registers
// workspace of the exchanges, in 4-byte words: level-1 records [2 parities][kPersistMaxGrid] x 128 B, then the eight XCD records of
// the tree's second level [2][8] x 128 B (grid_exchange8_hier), then the control words (XCD arrival counters at 0,
// the workgroups' XCDs at kPersistXcdTable, the error flag 16 words from the end).  Records and arrival counters are zeroed before every launch (kPersistZeroBytes).
constexpr size_t kPersistRecWords = (size_t)2 * kPersistMaxGrid * 32 + (size_t)2 * 8 * 32;
constexpr int kPersistXcdTable = 16;    // word offset (from PersistCtl::xcd) of the table "XCD of workgroup b", kPersistMaxGrid entries (hier_enter)
constexpr size_t kPersistWsWordsAll = kPersistRecWords + 64 + kPersistMaxGrid;
constexpr size_t kPersistZeroBytes = kPersistRecWords * 4 + 16 * sizeof(int);
constexpr int kPersistMaxDepth = 4;     // coefficient rows in flight per wave: deeper spills registers, and spills cost more than latency (measured 3..16)

__device__ __forceinline__ double read_lane_c(double v, int src) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// a wave-uniform value moved to scalar registers (the VALU results of the reductions / divisions would otherwise occupy
// vector registers for the whole iteration; every VALU instruction can read one scalar operand directly)
template <typename S>
__device__ __forceinline__ S uniform(S v) {
  if constexpr (sizeof(S) == 8) {
    const unsigned long long b = (unsigned long long)__double_as_longlong((double)v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return (S)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  } else {
    return (S)__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)v)));
  }
}
// Wave-wide sum on the DPP network (no LDS traffic, ~4x shorter dependent chain than the ds_bpermute butterfly of wave_sum):
// quad swaps, half-row and row mirrors leave every lane with the sum of its row of 16; the four row sums are read into scalar
// registers and added in a fixed order.  The result is wave-uniform.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)b, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum_uniform(double v) {
  v += dpp_move<0xB1>(v);                                  // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);                                  // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);                                 // row_half_mirror
  v += dpp_move<0x140>(v);                                 // row_mirror
  return ((read_lane_c(v, 0) + read_lane_c(v, 16)) + read_lane_c(v, 32)) + read_lane_c(v, 48);
}

// ---- buffer addressing: a 128-bit descriptor per array in SGPRs, one per-lane byte offset in a VGPR, the row offset in an
// SGPR.  Keeps the address arithmetic of 32 rows x 9 arrays out of the vector registers (which hold the solver state).
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// cache policy of a buffer access (gfx940+ encoding of the intrinsics' aux operand): kAgent = sc1, the scope at which the
// L2s of the 8 XCDs are coherent - used for everything one workgroup writes and another reads inside a launch.
constexpr int kPlain = 0, kAgent = 16;
template <typename S, int V, int AUX = kPlain>
__device__ __forceinline__ Vec<S, V> bld(rsrc_t r, unsigned voff, unsigned soff) {
  Vec<S, V> o;
  constexpr int B = sizeof(S) * V;
  static_assert(B == 16 || B == 8, "16- or 8-byte lane accesses");
  if constexpr (B == 16) {
    const auto t = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX);
    __builtin_memcpy(&o, &t, 16);
  } else {
    const auto t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX);
    __builtin_memcpy(&o, &t, 8);
  }
  return o;
}
template <typename S, int AUX = kPlain>
__device__ __forceinline__ S bld1(rsrc_t r, unsigned voff, unsigned soff) {
  S o;
  if constexpr (sizeof(S) == 8) {
    const auto t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX);
    __builtin_memcpy(&o, &t, 8);
  } else {
    const auto t = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX);
    __builtin_memcpy(&o, &t, 4);
  }
  return o;
}
// 16-byte stores carry the row offset in the VECTOR offset, not in an SGPR.  A buffer store of more than 8 bytes reads its data
// registers for some cycles after it has issued; a VALU instruction that overwrites one of them right behind it replaces what
// the LAST lanes store (seen: the low dword of lanes 12-15 of every row of 16, on the second wave of a SIMD, when the memory
// pipeline was busy).  The compiler pads that hazard for stores WITHOUT a register soffset only (it assumes the form with an
// SGPR soffset is free of it - not so on gfx950: `buffer_store_dwordx4 v[150:153], v1, s[20:23], s0 offen` followed directly
// by `v_mov_b32 v150, v1` published perimeters with the low dword of a lane offset in them).  voff must be a real offset.
template <typename S, int V, int AUX = kPlain>
__device__ __forceinline__ void bst(rsrc_t r, unsigned voff, unsigned soff, const Vec<S, V>& v) {
  static_assert(sizeof(S) * V == 16, "16-byte lane stores");
  __attribute__((ext_vector_type(4))) unsigned int t;
  __builtin_memcpy(&t, &v, 16);
  __builtin_amdgcn_raw_buffer_store_b128(t, r, voff + soff, 0, AUX);
}
template <typename S, int AUX = kPlain>
__device__ __forceinline__ void bst1(rsrc_t r, unsigned voff, unsigned soff, S v) {
  if constexpr (sizeof(S) == 8) {
    __attribute__((ext_vector_type(2))) unsigned int t;
    __builtin_memcpy(&t, &v, 8);
    __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, AUX);
  } else {
    unsigned int t;
    __builtin_memcpy(&t, &v, 4);
    __builtin_amdgcn_raw_buffer_store_b32(t, r, voff, soff, AUX);
  }
}

// value of lane `src` (compile-time constant after unrolling) as a wave-uniform scalar
template <typename S>
__device__ __forceinline__ S read_lane(S v, int src) {
  if constexpr (sizeof(S) == 8) {
    const unsigned long long b = (unsigned long long)__double_as_longlong((double)v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
    return (S)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  } else {
    return (S)__int_as_float(__builtin_amdgcn_readlane(__float_as_int((float)v), src));
  }
}
// lane l receives `v` of lane l - 1 (UP) or l + 1 (!UP) through the DPP wavefront shifts; the lane without a source keeps `edge`
template <bool UP, typename S>
__device__ __forceinline__ S shift_lane(S v, S edge) {
  constexpr int ctrl = UP ? 0x138 /* wave_shr:1 */ : 0x130 /* wave_shl:1 */;
  if constexpr (sizeof(S) == 8) {
    const unsigned long long b = (unsigned long long)__double_as_longlong((double)v), e = (unsigned long long)__double_as_longlong((double)edge);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)e, (int)(unsigned)b, ctrl, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(e >> 32), (int)(unsigned)(b >> 32), ctrl, 0xf, 0xf, false);
    return (S)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  } else {
    return (S)__int_as_float(__builtin_amdgcn_update_dpp(__float_as_int((float)edge), __float_as_int((float)v), ctrl, 0xf, 0xf, false));
  }
}

// ---- kernel arguments of cg_persist1
// SLAB = true: the kernel works on ONE y-slab of a grid that is cut over the GPUs of a node (cg_slab.hip).  What changes:
//   * the rows just below / above the slab belong to the neighbouring GPU: the edge regions publish their first / last row of z'
//     ALSO into that neighbour's mailbox (peer-mapped memory, system-scope stores over xGMI) and read the neighbour's row from
//     their own mailbox; r, p[] and x carry one halo row below (row -1) and above (row ny) as in the two-kernel slab path - the
//     ring copies start from them and are written back to them when the segment ends;
//   * the exchange's second level crosses the node: the XCD leaders store their records into every rank's mailbox, wave w of every
//     workgroup adds rank w's records, the rank totals meet in LDS (bitwise the same totals on every GPU, so every GPU takes the
//     same decisions; grid_exchange8_hier<..., XG>);
//   * N of the slab's last row comes from the N array (its S twin lives on the neighbour), sums of the previous K2 from a.gB.
struct NoSlab {};
struct SlabCtl {
  PeerView pv;
  double ncells;           // cells of the GLOBAL grid
  char *rows_own, *rows_lo, *rows_hi;   // the row areas (PeerLayout::kRows) of my mailbox and of the lower / upper neighbour's
  unsigned hop_ticks;      // measurements only (option slab_hop_ticks): the XCD leaders' records leave this many 10 ns ticks late
};
// A kernel argument read AGAIN from the kernarg segment (scalar loads through a pointer the optimiser cannot see through).  The
// row loops of the persistent kernels are bound by VALU issue and short of scalar registers: whatever only the rare paths need -
// the mailbox addresses of the two edge waves of a slab, the pointers of the exit block - is fetched where it is used instead of
// living in SGPRs across the loop (a spilled SGPR comes back through v_readlane, a VALU slot; an s_load costs none).
// Persist1Kargs mirrors the argument list of cg_persist1 (arguments are laid out like the members of a struct); the slab kernel
// compares one reloaded field with the argument itself at entry and fails the launch if the layouts ever disagree.
template <typename T, typename SL>
struct Persist1Kargs { CgArgs<T> a; PersistCtl c; int k_begin, k_end, sv, pend; SL sl; };
template <typename F>
__device__ __forceinline__ F karg(unsigned off) {
  typedef __attribute__((address_space(4))) const char kchar;
  typedef __attribute__((address_space(4))) const unsigned kword;
  kchar* kp = (kchar*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  static_assert(sizeof(F) % 4 == 0, "whole dwords");
  constexpr int NW = (int)(sizeof(F) / 4);
  unsigned w[NW];
  kword* src = (kword*)(kp + off);
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = src[i];              // (merged into s_load_dwordx2 / x4 / x8 / x16)
  F out;
  __builtin_memcpy(&out, w, sizeof(F));
  return out;
}

// s_sleep units (64 cycles) of the exchanges' polling (constants, not switches):
constexpr int kPollDelay2 = 40;                  // tree, second level, behind the rows computed ahead (2048^2: 24 -> 9.12, 32 / 40 -> 8.94 us per iteration)
constexpr int kPollDelay2NoAhead = 8;            // ... where nothing is computed ahead (512^2 / 1024 x 256: 24 -> 8: 4.27 -> 4.15 us, 0: 4.22)
constexpr int kPollDelay2Xg = 8;                 // ... of the slab instance's node level (ring of one, 2048^2: 40 -> 8: 10.05 -> 9.67 us)
constexpr int kLocalDelay = 8;                   // XCD-local exchange with one working wave per SIMD
constexpr int kPollSleep = 1;                    // between two polling passes
constexpr int kX1Values = 8;                     // sums per exchange
constexpr int kX1RecWords = 16;                  // 8-byte words per record: 2 per sum {32 payload bits | 32-bit epoch}

// ---- Grid-wide exchange of kX1Values partial sums per workgroup that doubles as the grid barrier (measured 4.4 us for 256 workgroups
// against 11.3 us for "atomic counter + fence + read the partials", scripts/barrier_bench.hip):
//   * every workgroup publishes one record: each double travels as two 8-byte words {32 payload bits | 32-bit epoch}, written and
//     read with relaxed agent-scope atomics (single-copy atomic, coherent across the 8 XCDs' L2s);
//   * the waves poll all records until they carry the current epoch and add them in a fixed order, so every workgroup obtains
//     bitwise the same totals - no counter, no fence, one memory round trip;
//   * records alternate between two arrays (epoch parity): a fast workgroup may publish epoch e+1 while a slow one still reads
//     epoch e, and nobody can reach e+2 before everybody has published e+1.
// DATA written before the exchange (the published perimeter rows) is stored write-through at agent scope (sc1) and drained
// (s_waitcnt vmcnt) by every wave before the workgroup publishes; readers load it at agent scope as well.  The polling is
// COALESCED: lane l reads word l % 16 of record 4 i + l / 16, so one load instruction covers four whole records (512 contiguous
// bytes), one round trip once the records are there (one record per LANE - 64 cache lines per load instruction - is bound by the
// number of fabric transactions).  Lane pairs (2 q, 2 q + 1) hold the two halves of sum q.  The flat form of this exchange - every
// workgroup polling all records through the fabric - is gone: profiles/README.md, "persistent CG kernel: variants measured and dropped".
constexpr int kX1Sm = 160;                        // LDS words per parity (the exchanges use the first 64: [8 sums][8 waves])
struct NoPrefetch { __device__ __forceinline__ void operator()() const {} };

// ---- wave-level reductions of the exchange on as few VALU instructions as possible (the row loops around the exchange are
// bound by VALU issue, and every instruction of a 64-wide wave costs the same ~4.5 SIMD cycles whatever it does).
// 64-bit moves between lanes: DPP inside a row of 16 lanes (VALU, two instructions), the LDS crossbar (ds_bpermute: no VALU
// slot) across rows.
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_update(double old, double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v), o = (unsigned long long)__double_as_longlong(old);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)b, CTRL, 0xf, BANK, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(b >> 32), CTRL, 0xf, BANK, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double lanes_xor4(double v) {    // lane l <- lane l ^ 4: row_shl:4 into banks 0, 2 / row_shr:4 into banks 1, 3
  return dpp_update<0x114, 0xa>(dpp_update<0x104, 0x5>(v, v), v);
}
__device__ __forceinline__ double lanes_xor8(double v) { return dpp_move<0x128>(v); }                  // row_ror:8
// v + (v of lane l ^ 16) and v + (v of lane l ^ 32): gfx950's v_permlane16_swap / v_permlane32_swap exchange the odd rows (the upper
// half) of one register with the even rows (the lower half) of another - two swaps of the value with itself leave "mine" and "the
// partner's" in two registers of EVERY lane, no trip through the LDS crossbar (ds_bpermute: ~100 cycles each in a dependent chain
// that every wave of the chip waits for).  Both lanes of a pair add the same two numbers (a + b, b + a: the same bits), as before.
template <int ROWS>
__device__ __forceinline__ double sum_xor_rows(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  const auto r0 = ROWS == 16 ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false) : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto r1 = ROWS == 16 ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false) : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const double x = __longlong_as_double((long long)(((unsigned long long)r1[0] << 32) | r0[0]));
  const double y = __longlong_as_double((long long)(((unsigned long long)r1[1] << 32) | r0[1]));
  return x + y;
}
__device__ __forceinline__ double sum_xor16(double v) { return sum_xor_rows<16>(v); }
__device__ __forceinline__ double sum_xor32(double v) { return sum_xor_rows<32>(v); }
// Eight per-lane partial sums -> lane l holds the WAVE total of value l & 7.  Reduce-scatter butterfly over lane bits 0, 1, 2 (a
// lane keeps half of its values and receives the partner's contribution to them: 7 + 7 + ... instructions instead of three full
// butterflies of eight values), then plain butterflies of the ONE remaining value over bits 3 (DPP), 4 and 5 (LDS crossbar).
// ~56 VALU instructions; eight wave_sum_uniform calls are ~190.  Every step adds a lane's value and its partner's: both lanes of
// a pair compute a + b and b + a - the same bits.
__device__ __forceinline__ double wave_reduce_scatter8(const double (&v)[8]) {
  const int lane = threadIdx.x & 63;
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0, b2 = (lane & 4) != 0;
  double a[4], b[2];
#pragma unroll
  for (int j = 0; j < 4; ++j)                                // a[j]: value 2 j + b0, summed over lane pairs
    a[j] = (b0 ? v[2 * j + 1] : v[2 * j]) + dpp_move<0xB1>(b0 ? v[2 * j] : v[2 * j + 1]);      // quad_perm [1,0,3,2]
#pragma unroll
  for (int m = 0; m < 2; ++m)                                // b[m]: value 4 m + 2 b1 + b0, summed over quads
    b[m] = (b1 ? a[2 * m + 1] : a[2 * m]) + dpp_move<0x4E>(b1 ? a[2 * m] : a[2 * m + 1]);      // quad_perm [2,3,0,1]
  double c = (b2 ? b[1] : b[0]) + lanes_xor4(b2 ? b[0] : b[1]);                                 // value l & 7, summed over 8 lanes
  c += lanes_xor8(c);
  c = sum_xor16(c);
  c = sum_xor32(c);
  return c;
}

// ---- what the exchanges below are made of
// The per-phase clocks of diagnostic builds (-DPISO_PERSIST_DIAG; acc == nullptr: nobody asked): split(q) adds the time since the
// previous split to acc[q].  The exchanges' phases: [0] reduction + drain of this wave's stores, [1] the barrier, [2] publish +
// polling, [3] adding the records; the kernel's: D, exchange, U.
struct PhaseClock {
  unsigned long long* acc;
  unsigned long long t0;
  __device__ __forceinline__ explicit PhaseClock(unsigned long long* a) : acc(a), t0((kPersistDiag && a) ? wall_clock64() : 0) {}
  __device__ __forceinline__ void split(int q) {
    if (kPersistDiag && acc) { const unsigned long long t = wall_clock64(); acc[q] += t - t0; t0 = t; }
  }
};
// The sums of N x 4 polled records (w[i] of lane l: word l % 16 of record 4 i + l / 16): even lanes assemble a double from their own
// word (low half) and the neighbour lane's (high half), the records of a lane are added in order (in_play(i): does record
// 4 i + l / 16 count?), then the four record rows of the lanes - lane 2 q ends with the total of value q.
template <int N, typename P>
__device__ __forceinline__ double records_sum(const unsigned long long (&w)[N], P in_play) {
  double acc = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const unsigned hi_other = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(w[i] >> 32), 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    const double val = __longlong_as_double((long long)((w[i] >> 32) | ((unsigned long long)hi_other << 32)));   // (odd lanes: garbage that nobody reads)
    acc += in_play(i) ? val : 0.0;
  }
  acc = sum_xor16(acc);
  return sum_xor32(acc);
}
// The start of every exchange: this wave's eight sums into the parity's LDS block sm = [8 sums][8 waves], then the wave's stores
// drained and the workgroup's barrier.
template <typename T>
__device__ __forceinline__ void exchange_prologue(const T (&v)[kX1Values], T* sm, PhaseClock& clk) {
  constexpr int NV = kX1Values;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double vd[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) vd[q] = (double)v[q];
  const double mine = wave_reduce_scatter8(vd);              // lane l: value l & 7, summed over this wave
  if (lane < NV) sm[lane * kPersistWaves + wave] = (T)mine;
  // EVERY vector-memory operation of this wave has completed - in particular its write-through perimeter stores - before the
  // workgroup's record says so.  (A counted wait that lets the two prefetch loads issued behind the last store stay in flight
  // would save ~0.4 us; it relies on loads and stores retiring in one order, which is not promised.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  clk.split(0);
  __syncthreads();                                            // every wave of the workgroup has drained its stores
  clk.split(1);
}

// ---- The exchange as a TREE that follows the hardware (chip-wide launches; round 4): workgroup -> XCD leader -> everybody.
//   level 1  every workgroup stores its record WITHOUT sc1 into the records of ITS XCD (slot = 32 xcd + arrival rank on that XCD;
//            the store stays in that XCD's L2); wave 0 of the XCD's leader (arrival rank 0) polls the XCD's records with sc1 loads
//            (L1 bypassed, served by the L2 both share) and adds them in rank order;
//   level 2  the leader publishes the XCD's sums as one record through the fabric (sc1 store); EVERY wave of every workgroup polls
//            the eight XCD records itself (two coalesced loads per lane) and adds them in XCD order - bitwise the same totals in
//            every wave of the chip, no second barrier, no LDS round trip behind the polling.
// Measured (scripts/barrier_bench.hip, 256 workgroups, 3 sums): 2.40 us per exchange against 3.7-5.3 us for the flat all-to-all
// variants (every workgroup polling 256 records through the fabric: 8 MB of polling reads per pass; here 4 KB per XCD at level 1
// and 2 MB at level 2).  hx packs what a workgroup learnt at entry (hier_enter): bits 0-2 XCD, 3-8 arrival rank, 9-14 workgroups
// on my XCD, 15-22 XCDs that hold workgroups.  A wave whose polling gives up sets the workgroup's LDS flag and the launch's
// error word; all waves of the workgroup read the flag behind the next barrier and leave the loop together.
__device__ __forceinline__ unsigned long long* hier_level2(const PersistCtl& c) {
  return c.rec + (size_t)2 * kPersistMaxGrid * kX1RecWords;                 // right behind the level-1 records (kPersistRecWords)
}
// entry of a chip-wide launch: which XCD am I on, how many workgroups does every XCD hold, and which of them am I?  One returning
// atomic per workgroup, then everybody waits for everybody ONCE per launch (c.xcd[0..7] arrivals per XCD, [9] arrivals in all;
// zeroed by the host before the launch).  My place among my XCD's workgroups is my place by WORKGROUP INDEX, not by arrival: the
// leader adds the records in that order, so two launches that the hardware deals to the XCDs the same way add in the same order
// and a solve is reproducible bit for bit from run to run (by arrival order the forward solves of the 2048^2 benchmark took
// 325 - 360 iterations on the same input, now and then 1 005).  Every workgroup leaves its XCD in a table before it counts itself in.
__device__ __forceinline__ unsigned hier_enter(const PersistCtl& c, int* lds2) {      // lds2: [0] hx, [1] launch cannot run, [2] sticky flag of the exchanges
  int* const table = c.xcd + kPersistXcdTable;
  if (threadIdx.x == 0) {
    const int xcc = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7);       // HW_REG_XCC_ID[3:0]
    __hip_atomic_store(table + blockIdx.x, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int arrival = __hip_atomic_fetch_add(c.xcd + xcc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(c.xcd + 9, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);     // (release: my table entry is out before I count)
    unsigned spins = 0;
    bool ok = arrival < 32;
    while (ok && __hip_atomic_load(c.xcd + 9, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (int)gridDim.x) {
      if (++spins > (1u << 22)) { ok = false; break; }
      __builtin_amdgcn_s_sleep(2);
    }
    unsigned present = 0, mine = 0;
    for (int x = 0; x < kXcds; ++x) {
      const int n = __hip_atomic_load(c.xcd + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n > 0) present |= 1u << x;
      if (n > 32) ok = false;
      if (x == xcc) mine = (unsigned)n;
    }
    if (!ok) *c.err = 1;
    lds2[0] = (int)((unsigned)xcc | ((mine & 63u) << 9) | (present << 15));
    lds2[1] = ok ? 0 : 1;
    lds2[2] = 0;
  }
  __syncthreads();
  if (threadIdx.x < 64 && !lds2[1]) {                        // wave 0: the workgroups of my XCD with a smaller index
    const int xcc = lds2[0] & 7;
    int before = 0;
    for (int b = (int)threadIdx.x; b < (int)gridDim.x; b += 64)
      before += (b < (int)blockIdx.x && __hip_atomic_load(table + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == xcc) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if (threadIdx.x == 0) lds2[0] |= (before & 63) << 3;
  }
  __syncthreads();
  return (unsigned)__builtin_amdgcn_readfirstlane(lds2[0]);
}
// entry of an XCD-local launch (8 x c.local_n workgroups): every workgroup counts itself in on its XCD (HW_REG_XCC_ID), the one that
// completes the first quota of c.local_n names its XCD the winner, the c.local_n first arrivals there run the solve with their
// arrival ranks as workgroup numbers (returned) and everybody else leaves (-1).  Some XCD always collects a quota (8 x local_n
// workgroups over 8 XCDs), whatever the dispatcher does: placement decides nothing but speed.
__device__ __forceinline__ int local_enter(const PersistCtl& c, int* rank_s) {
  if (threadIdx.x == 0) {
    const int xcc = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7);       // HW_REG_XCC_ID[3:0]
    const int arrival = __hip_atomic_fetch_add(c.xcd + xcc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int rank = -1;
    if (arrival < c.local_n) {
      if (arrival == c.local_n - 1) {                    // my XCD's quota is complete: the first such XCD wins
        int none = 0;
        __hip_atomic_compare_exchange_strong(c.xcd + 8, &none, xcc + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      int winner = 0;
      unsigned spins = 0;
      while ((winner = __hip_atomic_load(c.xcd + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
        if (++spins > (1u << 22)) break;                 // (cannot happen: some XCD completes a quota; never hang all the same)
        __builtin_amdgcn_s_sleep(2);
      }
      if (winner == xcc + 1) rank = arrival;
      else if (winner == 0) { *c.err = 1; }
    }
    *rank_s = rank;
  }
  __syncthreads();
  // (wave-uniform BY CONSTRUCTION: an LDS read is a vector value to the compiler - every offset derived from it became per-lane
  // arithmetic, and the halo loads' resources were built in waterfall loops)
  return __builtin_amdgcn_readfirstlane(*rank_s);
}
// XG (slab instance, round 5): the node's level of the exchange rides on the tree's second level instead of following it.  The XCD
// leaders store their XCD's record straight into EVERY rank's mailbox (system-scope stores over xGMI; the own mailbox included);
// wave w of every workgroup polls the eight XCD records of RANK w in its own mailbox and adds them in XCD order, the rank totals
// meet in LDS behind one barrier and every wave adds them by the same butterfly over the rank index - bitwise the same totals in
// every wave of every GPU.  (Round 4 had a serial level here: workgroup 0 waited for the chip's totals, wrote them to the peers,
// and wave 0 of every workgroup polled again - one more uncached round trip per iteration.)  All eight records of a rank also
// certify that every row this rank stored into a peer's mailbox has completed: its workgroups drained their stores before they
// published, and a leader publishes only after it has seen all workgroups of its XCD.  An XCD that holds no workgroups (small
// grids) is published with zero sums by the leader of the rank's lowest XCD in play.  sl_off: where the SlabCtl sits in the
// kernarg segment - mailbox addresses, rank and world are fetched where they are used (karg), not held in SGPRs across the loops.
constexpr int kX1SmX = 80;                        // LDS words of the node level per parity: [8 ranks][8 sums], 8 flags
template <typename T, int DELAY2, bool XG = false, typename F = NoPrefetch>
__device__ __forceinline__ bool grid_exchange8_hier(const PersistCtl& c, T (&v)[kX1Values], unsigned epoch, T* smem, unsigned hx, int* flag,
                                                    F while_records_travel = F(), unsigned long long* tsub = nullptr, unsigned sl_off = 0,
                                                    T* smx2 = nullptr) {
  PhaseClock clk(tsub);
  typedef unsigned long long u64;
  constexpr int NV = kX1Values;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* sm = smem + (epoch & 1) * kX1Sm;                       // parity double buffer (one barrier per exchange separates writers and readers)
  exchange_prologue(v, sm, clk);
  // A polling pass of an EARLIER exchange gave up somewhere in this workgroup: the flag is sticky, every wave reads it here behind the
  // barrier and all of them leave together at the end of this exchange - the wave that gave up included: it returned "healthy" like
  // its siblings.  (No return from here: an exit in the middle of the iteration loop turns its control flow into exec-mask flow and
  // the iteration counter into a vector register.  The polling loops below give up at once instead: spin0.)
  const bool good = __builtin_amdgcn_readfirstlane(*flag) == 0;
  const unsigned spin0 = good ? 0u : (1u << 30);
  const int xcc = (int)(hx & 7u), rank = (int)((hx >> 3) & 63u), nmine = (int)((hx >> 9) & 63u);
  const unsigned present = (hx >> 15) & 0xffu;
  u64* rec1 = c.rec + (size_t)(epoch & 1) * kPersistMaxGrid * kX1RecWords + (size_t)xcc * 32 * kX1RecWords;
  u64* rec2 = hier_level2(c) + (size_t)(epoch & 1) * kXcds * kX1RecWords;
  // lane l polls word l % 16 of record 4 i + l / 16, i.e. 8-byte word 64 i + l of the record array: ONE per-lane offset, made opaque
  // so that nothing derived from it is hoisted out of the iteration loop into vector registers that live across the row loops
  int lw = lane;
  asm volatile("" : "+v"(lw));
  bool mygood = true;
  if (wave == 0) {
    {
      // lane l < 16 publishes word l: sum l / 2, low half (even l) or high half (odd l) - one store instruction, one cache line
      const int vq = (lane >> 1) & (NV - 1);
      T s = 0;
      for (int w = 0; w < kPersistWaves; ++w) s += sm[vq * kPersistWaves + w];
      const u64 bits = (u64)__double_as_longlong((double)s);
      const u64 word = (lane & 1) ? ((bits & 0xffffffff00000000ull) | epoch) : (((bits & 0xffffffffull) << 32) | epoch);
      if (lane < kX1RecWords) __hip_atomic_store(rec1 + (size_t)rank * kX1RecWords + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (rank == 0) {                                          // the XCD's leader: the records of my XCD (through its L2), in rank order
      // (branch-free passes: all eight loads every time, records beyond the XCD's count masked by one compare against a scalar -
      // per-record arrival flags are eight lane masks = sixteen SGPRs the row loops then spill)
      u64 w[8];
      // (opaque: left visible, the eight bounds lim - 64 i are constants of the launch that live in SGPRs across the row loops - spilled,
      // and a spilled SGPR comes back through v_readlane; recomputed here they are eight scalar subtractions per exchange)
      int lim = nmine * kX1RecWords;                          // words of the XCD's block that belong to records in play
      asm volatile("" : "+s"(lim));
      unsigned spins = spin0;
      while (true) {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = __hip_atomic_load(rec1 + lw + i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned bad = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) bad |= (lw < lim - i * 64) ? ((unsigned)(w[i] & 0xffffffffull) ^ epoch) : 0u;
        if (__all(bad == 0)) break;
        if (++spins > (1u << 22)) { mygood = false; break; }
      }
      const double acc = records_sum(w, [&](int i) { return lw < lim - i * 64; });      // even lane 2 q: the XCD's sum of value q
      const double other = dpp_move<0xB1>(acc);              // odd lanes: the even neighbour's sum
      const u64 bits = (u64)__double_as_longlong((lane & 1) ? other : acc);
      const u64 word = (lane & 1) ? ((bits & 0xffffffff00000000ull) | epoch) : (((bits & 0xffffffffull) << 32) | epoch);
      if constexpr (!XG) {
        if (lane < kX1RecWords) __hip_atomic_store(rec2 + (size_t)xcc * kX1RecWords + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        constexpr unsigned pvo = (unsigned)offsetof(SlabCtl, pv);
        const int world = karg<int>(sl_off + pvo + (unsigned)offsetof(PeerView, world));
        const int myrank = karg<int>(sl_off + pvo + (unsigned)offsetof(PeerView, rank));
        // (measurements only - SlabCtl::hop_ticks > 0: the records leave this many 10 ns ticks late, as if the link had that latency)
        const unsigned hop = karg<unsigned>(sl_off + (unsigned)offsetof(SlabCtl, hop_ticks));
        if (hop) { const unsigned long long t_go = wall_clock64() + hop; while (wall_clock64() < t_go) __builtin_amdgcn_s_sleep(1); }
        const bool lowest = (present & ((1u << xcc) - 1u)) == 0;     // (scalar) the leader that also speaks for the XCDs without workgroups
        for (int p = 0; p < world; ++p) {
          char* mb = karg<char*>(sl_off + pvo + (unsigned)offsetof(PeerView, mbox) + 8u * (unsigned)p);
          if (lane < kX1RecWords) peer_store(reinterpret_cast<peer_u64*>(mb + PeerLayout::xcd_rec(epoch & 1, myrank, xcc)) + lane, word);
          if (lowest && present != 0xffu) {
            for (int x = 0; x < kXcds; ++x)
              if (!((present >> x) & 1u) && lane < kX1RecWords)
                peer_store(reinterpret_cast<peer_u64*>(mb + PeerLayout::xcd_rec(epoch & 1, myrank, x)) + lane, (peer_u64)epoch);
          }
        }
      }
    }
  }
  // the records need a microsecond or two to make their way: work that does not depend on the sums goes here (the row loops
  // are bound by VALU issue, and the SIMDs idle while the exchange is in flight)
  while_records_travel();
  if constexpr (!XG) {
    // every wave: the eight XCD records (lane l: word l % 16 of record 4 i + l / 16), added in XCD order
    u64 w[2];
    unsigned spins = spin0;
    if (DELAY2 > 0) __builtin_amdgcn_s_sleep(DELAY2);
    while (true) {
#pragma unroll
      for (int i = 0; i < 2; ++i) w[i] = __hip_atomic_load(rec2 + lw + i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned bad = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)                            // (XCDs without workgroups: nothing to wait for, payload 0)
        bad |= (((present >> (i * 4)) >> (lw >> 4)) & 1u) ? ((unsigned)(w[i] & 0xffffffffull) ^ epoch) : 0u;
      if (__all(bad == 0)) break;
      if (++spins > (1u << 22)) { mygood = false; break; }
      __builtin_amdgcn_s_sleep(kPollSleep);
    }
    clk.split(2);
    // lane 2 q: the total of value q - the same bits in every wave of the chip
    const double acc = records_sum(w, [&](int i) { return (((present >> (i * 4)) >> (lw >> 4)) & 1u) != 0; });
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = (T)read_lane_c(acc, 2 * q);
    if (!mygood) {                                              // (wave-uniform)
      if (lane == 0) { *flag = 1; *c.err = 1; }
    }
    clk.split(3);
    return good;
  } else {
    // wave w: the eight XCD records of rank w in MY mailbox (every XCD slot of a rank in play is published, see above)
    T* smx = smx2 + (epoch & 1) * kX1SmX;
    constexpr unsigned pvo = (unsigned)offsetof(SlabCtl, pv);
    const int world = karg<int>(sl_off + pvo + (unsigned)offsetof(PeerView, world));
    double acc = 0;
    if (wave < world) {
      const char* own = karg<char*>(sl_off + (unsigned)offsetof(SlabCtl, rows_own)) - PeerLayout::kRows;
      const peer_u64* recs = reinterpret_cast<const peer_u64*>(own + PeerLayout::xcd_rec(epoch & 1, wave, 0));
      peer_u64 w[2];
      unsigned spins = spin0;
      if (DELAY2 > 0) __builtin_amdgcn_s_sleep(DELAY2);
      while (true) {
#pragma unroll
        for (int i = 0; i < 2; ++i) w[i] = peer_load(recs + lw + i * 64);
        unsigned bad = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) bad |= (unsigned)(w[i] & 0xffffffffull) ^ epoch;
        if (__all(bad == 0)) break;
        if (++spins > kPeerSpinLimit) { mygood = false; break; }      // (kPeerSpinLimit < spin0)
        __builtin_amdgcn_s_sleep(kPollSleep);
      }
      acc = records_sum(w, [](int) { return true; });       // lane 2 q: rank w's total of value q (XCD order)
    }
    clk.split(2);
    if (lane < 2 * NV && !(lane & 1)) smx[wave * NV + (lane >> 1)] = (T)acc;       // (a wave without a rank: zeros)
    if (!mygood) {
      if (lane == 0) { *flag = 1; *c.err = 1; }
    }
    __syncthreads();
    {
      // one read fetches the 8 x 8 rank totals (lane l: rank l / 8, value l % 8); the butterfly over the rank index leaves every
      // lane with the node's total of value l % 8 - the same order of additions in every wave of every GPU
      double t = (double)smx[lane];
      t += lanes_xor8(t);
      t = sum_xor16(t);
      t = sum_xor32(t);
#pragma unroll
      for (int q = 0; q < NV; ++q) v[q] = (T)read_lane_c(t, q);
    }
    clk.split(3);
    return good && __builtin_amdgcn_readfirstlane(*flag) == 0;
  }
}

// ---- XCD-local launches (LOCAL, at most 32 workgroups, all on one XCD): the same idea in one level.  Wave 0 publishes the workgroup's
// record (plain store: it stays in the XCD's L2), then EVERY wave polls the group's records itself (sc1 loads: L1 bypassed, served
// by that L2; eight coalesced loads per lane cover 32 records) and adds them in slot order - no second barrier, no LDS round trip
// behind the polling (0.36 us of a 3.5 us iteration at 256^2).  Error handling as in grid_exchange8_hier (sticky LDS flag).
template <typename T>
__device__ __forceinline__ bool grid_exchange8_local(const PersistCtl& c, T (&v)[kX1Values], unsigned epoch, T* smem, int slot, int nslots, int* flag,
                                                     unsigned long long* tsub = nullptr) {
  PhaseClock clk(tsub);
  typedef unsigned long long u64;
  constexpr int NV = kX1Values;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* sm = smem + (epoch & 1) * kX1Sm;                       // parity double buffer (one barrier per exchange separates writers and readers)
  exchange_prologue(v, sm, clk);
  const bool good = __builtin_amdgcn_readfirstlane(*flag) == 0;      // (sticky, read behind the barrier: all waves leave together, see grid_exchange8_hier)
  const unsigned spin0 = good ? 0u : (1u << 30);
  u64* rec = c.rec + (size_t)(epoch & 1) * kPersistMaxGrid * kX1RecWords;
  int lw = lane;
  asm volatile("" : "+v"(lw));
  bool mygood = true;
  if (wave == 0) {
    const int vq = (lane >> 1) & (NV - 1);
    T s = 0;
    for (int w = 0; w < kPersistWaves; ++w) s += sm[vq * kPersistWaves + w];
    const u64 bits = (u64)__double_as_longlong((double)s);
    const u64 word = (lane & 1) ? ((bits & 0xffffffff00000000ull) | epoch) : (((bits & 0xffffffffull) << 32) | epoch);
    if (lane < kX1RecWords) __hip_atomic_store(rec + (size_t)slot * kX1RecWords + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  {
    u64 w[8];
    const int lim = nslots * kX1RecWords;
    unsigned spins = spin0;
    // (one working wave per SIMD - c.waves = 4: the record needs ~0.2 us to arrive and a first pass that misses it queues in front
    // of the one that would find it: 256^2 3.33 -> 3.15 us per iteration with 8 units, 4: 3.21, 12: 3.23; with two working waves per
    // SIMD - 512 x 256 - any delay loses: 3.84 / 3.83 / 3.92 / 4.00 / 4.10 with 0 / 4 / 8 / 12 / 16)
    if (kLocalDelay > 0 && c.waves < kPersistWaves) __builtin_amdgcn_s_sleep(kLocalDelay);
    while (true) {
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = __hip_atomic_load(rec + lw + i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned bad = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) bad |= (lw < lim - i * 64) ? ((unsigned)(w[i] & 0xffffffffull) ^ epoch) : 0u;
      if (__all(bad == 0)) break;
      if (++spins > (1u << 22)) { mygood = false; break; }
      __builtin_amdgcn_s_sleep(kPollSleep);
    }
    clk.split(2);
    const double acc = records_sum(w, [&](int i) { return lw < lim - i * 64; });
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = (T)read_lane_c(acc, 2 * q);
  }
  if (!mygood) {
    if (lane == 0) { *flag = 1; *c.err = 1; }
  }
  clk.split(3);
  return good;
}


}  // namespace piso
