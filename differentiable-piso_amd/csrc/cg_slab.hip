// Slab-decomposed pressure CG: the grid is cut into 1-D slabs along y (contiguous row blocks), one rank per GPU.
// SURVEY.md 8(e).  The reference has no multi-GPU path; this is new design.
//
// Per CG iteration and rank:  K1  ->  3-double all-reduce  ->  K2  ->  3-double all-reduce + one-row halo exchange of r.
//   * the kernels are the single-GPU ones (cg_kernels.h) in "halo mode": r, p[2] and x carry one halo row below and above
//     the owned rows; K1 recomputes the new direction on the halo rows from (r_halo, p_halo) and keeps it, so only r has to
//     be exchanged (one row = nx * 8 bytes per neighbour and iteration);
//   * per-block partial sums are collapsed to 3 scalars on the device, all-reduced over RCCL (xGMI), and read back by the
//     next kernel's prologue -- no host round trip; every rank evaluates the same stopping test on the same numbers;
//   * the rank-1 shift uses the global sum |diag| and the global cell count.
// Communication goes through a tiny interface (Comm) with three implementations:
//   * PEER (default inside a node): every rank owns a peer-mapped mailbox (peer.h); reductions and halo rows are written by
//     small kernels straight into the consumers' mailboxes - no library call, no host round trip.  With this transport the
//     NORMAL iterations run inside the persistent kernel cg_persist1<..., SLAB = true>: r, p, x of the slab stay on chip, the
//     perimeter rows at the slab edges and the per-GPU totals cross xGMI from inside the kernel (one extra hop per iteration);
//     resets, the first iteration and shapes the kernel cannot tile use the two-kernel iteration below;
//   * RCCL: two-kernel iteration only.  Both transports live behind the host collectives of the communicator (slab_comm.h, comm.hip);
//   * an in-process LOOPBACK that runs G virtual ranks on one device in lock-step -- the test harness for the multi-rank index
//     logic on a single-GPU box (tests/test_gpu_slab.py).
#include <vector>

#include "cg_driver.h"
#include "cg_kernels.h"
#include "options.h"
#include "peer.h"
#include "slab_comm.h"

namespace piso {

// ------------------------------------------------------------------------------------------------ per-rank context
// (fp64 only: the C ABI has no other slab solve, the mailbox rows hold 8-byte elements)
struct SlabRank {
  CgArgs<double> a;     // r, p[], x point at row 0 of buffers that own one halo row below (row -1) and above (row ny)
  double *rbase, *pbase[2], *xbase;
  double* g;            // [12]: gA[0..2], pad, gB[4..6], pad, gS[8..10] (sum |diag|, #not-f32, #not-recon)
  double* oT; float* oF; double* cC;
  int* flags;
  const double* L;
  double* x_out;        // owned rows of the caller's output
  int rank;             // position in the slab ring
  unsigned* persist_ws; // exchange records + error flag of the persistent kernel
};

// collapse per-block partial records into `count` scalars (fixed order)
template <typename T>
__global__ __launch_bounds__(kBlock) void slab_collapse(const T* __restrict__ parts, int records, int count, T* __restrict__ out) {
  __shared__ T smem[16];
  for (int q = 0; q < count; ++q) {
    T v[1] = {0};
    for (int b = threadIdx.x; b < records; b += kBlock) v[0] += parts[q * kMaxPartials + b];
    block_sum<T, 1>(v, smem);
    if (threadIdx.x == 0) out[q] = v[0];
  }
}
template <typename T>
__global__ void slab_flags_to_sums(const int* flags, T* out) {
  if (threadIdx.x == 0) { out[1] = (T)flags[0]; out[2] = (T)flags[1]; out[3] = (T)flags[2]; }
}
// error flags of a persistent segment (its own exchanges, the waits of the host-level collectives) as a summable value
template <typename T>
__global__ void slab_err_to_sum(const int* seg_err, const int* comm_err, T* out) {
  if (threadIdx.x == 0) out[0] = (T)((*seg_err != 0 || *comm_err != 0) ? 1 : 0);
}
// verification of a slab solve (cg_verify_gap): did the gap exceed its bound on this rank?  (summable)
template <typename T>
__global__ void slab_gap_to_sum(const unsigned* out2, T* out, int force) {
  if (threadIdx.x == 0) {
    const float gap = __uint_as_float(out2[0]), scale = __uint_as_float(out2[1]);
    out[0] = (T)(((gap > 1e-5f * scale && gap > 1e-30f) || force) ? 1 : 0);
  }
}
// loopback all-reduce: bufs of the G virtual ranks live `stride` apart; sum in rank order, write to all
template <typename T>
__global__ void loop_allreduce(T* base, int G, size_t stride, int count) {
  const int q = threadIdx.x;
  if (q >= count) return;
  T s = 0;
  for (int r = 0; r < G; ++r) s += base[(size_t)r * stride + q];
  for (int r = 0; r < G; ++r) base[(size_t)r * stride + q] = s;
}
template <typename T>
__global__ void slab_copy_rows(const T* __restrict__ src, T* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ communication
struct Comm {
  int world;              // slabs in the ring
  bool periodic_y;
  PisoComm* rccl;         // NULL = loopback over the local ranks; else the communicator (RCCL or peer transport)
  size_t g_stride;        // loopback: distance between consecutive ranks' g buffers
  bool peer() const { return rccl && rccl->transport == TRANSPORT_PEER; }

  // sum `count` values at offset `off` of every rank's g buffer
  int allreduce(std::vector<SlabRank>& R, int off, int count, hipStream_t s) {
    if (rccl) return comm_allreduce_f64(rccl, R[0].g + off, count, s);
    loop_allreduce<double><<<1, 64, 0, s>>>(R[0].g + off, world, g_stride, count);
    return PISO_OK;
  }
  // fill the halo rows (row -1 and row ny) of `which` (HALO_R, HALO_X) from the neighbours' edge rows
  int exchange(std::vector<SlabRank>& R, int which, hipStream_t s) {
    const int nx = R[0].a.nx;
    auto base0 = [&](SlabRank& k) { return which == HALO_R ? k.a.r : k.a.x; };   // row 0
    if (rccl) return comm_exchange_rows(rccl, periodic_y, base0(R[0]), nx, R[0].a.ny, s);
    for (int r = 0; r < world; ++r) {
      const int ny = R[r].a.ny;
      const int lo = (r > 0) ? r - 1 : (periodic_y ? world - 1 : -1);
      const int hi = (r < world - 1) ? r + 1 : (periodic_y ? 0 : -1);
      double* row0 = base0(R[r]);
      if (lo >= 0) slab_copy_rows<double><<<4, 256, 0, s>>>(base0(R[lo]) + (size_t)(R[lo].a.ny - 1) * nx, row0 - nx, nx);
      if (hi >= 0) slab_copy_rows<double><<<4, 256, 0, s>>>(base0(R[hi]), row0 + (size_t)ny * nx, nx);
    }
    return PISO_OK;
  }
};

// ------------------------------------------------------------------------------------------------ driver
// One rank's share of the workspace: n owned cells, nh cells with the two halo rows - in this order.  slab_rank_bytes counts it.
static void slab_carve(Arena& ar, size_t n, size_t nh, SlabRank& k) {
  k.cC = ar.take<double>(n); k.oT = ar.take<double>(4 * n); k.oF = ar.take<float>(4 * n);
  k.flags = ar.take<int>(4);
  k.rbase = ar.take<double>(nh); k.pbase[0] = ar.take<double>(nh); k.pbase[1] = ar.take<double>(nh); k.xbase = ar.take<double>(nh);
  CgArgs<double>& a = k.a;
  a.z = ar.take<double>(n);
  a.zp[0] = ar.take<double>(n); a.zp[1] = ar.take<double>(n);   // z' perimeters of the persistent kernel (agent-scope accesses only)
  k.persist_ws = ar.take<unsigned>(kPersistWsWordsAll);
  a.partsA = ar.take<double>(3 * kMaxPartials); a.partsB = ar.take<double>(3 * kMaxPartials); a.partsS = ar.take<double>(kMaxPartials);
  a.scal = ar.take<double>(SC_COUNT);
  a.state = ar.take<CgState>(2);
}
static size_t slab_rank_bytes(int nx, int nyl) {
  Arena ar = counting_arena();
  SlabRank k;
  slab_carve(ar, (size_t)nx * nyl, (size_t)nx * (nyl + 2), k);
  return counted_bytes(ar);
}

struct SlabPinned { CgState st; int pad[4]; double errsum; };
static thread_local SlabPinned* tl_slab_pinned = nullptr;

// The slab link of the iteration (cg_driver.h: cg_iterate): per-local-rank launches, partial sums collapsed and all-reduced, halo rows
// of r / x exchanged.  Every rank queues the same collectives in the same order: whatever decides about one - a segment's failure, the
// verification's verdict, (in slab_solve) the coefficient flags - is read from all-reduced values, never from this rank's alone.
template <typename CT, int V, bool RECON>
struct SlabLink {
  std::vector<SlabRank>& R;
  Comm& comm;
  hipStream_t stream;
  std::vector<int> g1, g2, gflat;
  PersistPlan plan;
  PersistCtl pc;
  SlabCtl sl;
  int seg_len;

  int start(float accuracy, bool symmetric, bool allow_persist, double global_cells) {
    const int nloc = (int)R.size();
    g1.resize(nloc); g2.resize(nloc); gflat.resize(nloc);
    for (int q = 0; q < nloc; ++q) {
      CgArgs<double>& a = R[q].a;
      const CgTiling tile = cg_tile(a, V, 0, 0);               // (options cg_rpw / cg_maxblocks are the one-GPU driver's)
      g1[q] = tile.g1; g2[q] = tile.g2; gflat[q] = tile.gflat;
      a.accuracy = accuracy;
      a.gA = R[q].g; a.gB = R[q].g + 4;
    }
    if (!tl_slab_pinned) PISO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&tl_slab_pinned), sizeof(SlabPinned), hipHostMallocDefault));
    // ---- persistent segments (peer transport, one rank per process): the NORMAL iterations of the slab run inside
    // cg_persist1<..., SLAB>; every rank takes the same decision (same shape, same options, failures are all-reduced).  The plan is the
    // one-GPU driver's (cg_dispatch.h) with full workgroups: a slab has never honoured cg_persist_half / cg_persist_nq / cg_xcd_local
    int cus = 0;
    if (allow_persist && comm.peer() && nloc == 1 && R[0].a.nx <= (int)comm.rccl->row_cap) {
      int dev = 0;
      PISO_HIP_CHECK(hipGetDevice(&dev));
      PISO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
      plan = persist_plan(PersistQuery{R[0].a.nx, R[0].a.ny, V, R[0].a.per_y, false, sizeof(double), sizeof(CT), RECON, symmetric, true, cus,
                                       opt(OPT_CG_PERSIST), opt(OPT_CG_PERSIST_R), 0, 0, 0, false, true});
    }
    PISO_TRY((persist_prepare<double, CT, RECON, true>(plan, cus, pc, R[0].persist_ws, stream)));
    if (plan.R) {
      sl.pv = make_view(comm.rccl, comm.periodic_y);
      sl.ncells = global_cells;
      sl.rows_own = sl.pv.mbox[sl.pv.rank] + PeerLayout::kRows;
      sl.rows_lo = sl.pv.mbox[sl.pv.lower >= 0 ? sl.pv.lower : sl.pv.rank] + PeerLayout::kRows;
      sl.rows_hi = sl.pv.mbox[sl.pv.upper >= 0 ? sl.pv.upper : sl.pv.rank] + PeerLayout::kRows;
      sl.hop_ticks = opt(OPT_SLAB_HOP_TICKS) > 0 ? (unsigned)opt(OPT_SLAB_HOP_TICKS) : 0u;
    }
    seg_len = persist_segment_len((size_t)R[0].a.nx * R[0].a.ny, opt(OPT_CG_SEGMENT));   // (per GPU)
    return PISO_OK;
  }

  bool persistent() const { return plan.R != 0; }
  int segment(int k, int ke, CgLoop& st) {
    PisoComm* c = comm.rccl;
    // tags: a 16-bit launch counter (the same on every rank) above a 16-bit exchange counter.  When the counter wraps, the
    // records of 65536 launches ago could pass for new ones: everybody waits for everybody, then clears its own.
    if ((c->launches & 0xffffu) == 0 && c->launches > 0) {
      PISO_TRY(comm.allreduce(R, 12, 1, stream));
      PISO_HIP_CHECK(hipMemsetAsync(c->mbox[c->rank] + PeerLayout::kXcdRecs, 0, PeerLayout::kXcdRecBytes, stream));
      PISO_TRY(comm.allreduce(R, 12, 1, stream));
    }
    PISO_TRY((persist_launch<double, CT, RECON, true>(plan, R[0].a, pc, c->launches++, k, ke, st.sv, st.pending, sl, stream)));
    // did the segment fail anywhere?  (g[12] = my error flag, summed over the ranks)
    slab_err_to_sum<double><<<1, 64, 0, stream>>>(pc.err, c->err, R[0].g + 12);
    PISO_TRY(comm.allreduce(R, 12, 1, stream));
    PISO_HIP_CHECK(hipMemcpyAsync(&tl_slab_pinned->errsum, R[0].g + 12, sizeof(double), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipMemcpyAsync(&tl_slab_pinned->st, &R[0].a.state[0], sizeof(CgState), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    if (tl_slab_pinned->errsum != 0) {
      ++c->persist_fallbacks;
      PISO_HIP_CHECK(hipMemsetAsync(c->err, 0, sizeof(int), stream));
      return kPersistRetry;
    }
    c->persist_iterations += ke - k;
    if (tl_slab_pinned->st.done) { st.finished = true; st.stop_it = tl_slab_pinned->st.iterations; }
    return PISO_OK;
  }

  int k1(int k, int mode, int sv, int chk, int pend) {
    for (size_t q = 0; q < R.size(); ++q) cg_k1<double, CT, V, RECON><<<g1[q], kBlock, 0, stream>>>(R[q].a, k, mode, sv, chk, pend);
    for (size_t q = 0; q < R.size(); ++q) slab_collapse<double><<<1, kBlock, 0, stream>>>(R[q].a.partsA, g1[q], 3, R[q].g);
    return comm.allreduce(R, 0, 3, stream);
  }
  int k2(int k, int sv) {
    for (size_t q = 0; q < R.size(); ++q) cg_k2<double, V><<<g2[q], kBlock, 0, stream>>>(R[q].a, k, sv);
    for (size_t q = 0; q < R.size(); ++q) slab_collapse<double><<<1, kBlock, 0, stream>>>(R[q].a.partsB, g2[q], 3, R[q].g + 4);
    return comm.allreduce(R, 4, 3, stream);
  }
  int flush(int k, int sv) { for (size_t q = 0; q < R.size(); ++q) cg_flush_x<double><<<gflat[q], kBlock, 0, stream>>>(R[q].a, k, sv); return PISO_OK; }
  int reset_residual(int sv) { for (size_t q = 0; q < R.size(); ++q) cg_reset_residual<double><<<gflat[q], kBlock, 0, stream>>>(R[q].a, sv); return PISO_OK; }
  int halo(int which) { return comm.exchange(R, which, stream); }

  // every 25 iterations and after the last, synchronously (every rank reads the same all-reduced test)
  int look(int k, CgLoop& st) {
    if ((k + 1) % 25 != 0 && k + 1 != st.total) return PISO_OK;
    PISO_HIP_CHECK(hipMemcpyAsync(&tl_slab_pinned->st, &R[0].a.state[st.sv & 1], sizeof(CgState), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    if (tl_slab_pinned->st.done) { st.finished = true; st.stop_it = tl_slab_pinned->st.iterations; }
    return PISO_OK;
  }

  int finish(CgLoop& st) {
    // ---- run-time verification of a solve that used the persistent slab kernel (as cg.hip does on one GPU; here it also covers
    // what crossed xGMI): r must still be b - A^ x for the x this rank returns.  Needs the neighbours' edge rows of x and the
    // global sum(x); the verdicts of all ranks are summed, so all ranks accept or all restart on the two-kernel iteration.
    if (st.segments_run > 0 && opt(OPT_CG_VERIFY) != 0) {
      CgArgs<double>& a0 = R[0].a;
      unsigned* out2 = reinterpret_cast<unsigned*>(pc.err) + 4;
      PISO_HIP_CHECK(hipMemsetAsync(out2, 0, 2 * sizeof(unsigned), stream));
      PISO_TRY(halo(HALO_X));
      const int gvf = grid_for((long long)a0.nx * a0.ny, kBlock * 4, 1024);
      cg_verify_sum_x<double><<<gvf, kBlock, 0, stream>>>(a0, a0.partsA);
      slab_collapse<double><<<1, kBlock, 0, stream>>>(a0.partsA, gvf, 1, R[0].g + 12);
      PISO_TRY(comm.allreduce(R, 12, 1, stream));
      cg_verify_gap<double, CT><<<gvf, kBlock, 0, stream>>>(a0, a0.partsA, 0, out2, R[0].g + 12);
      slab_gap_to_sum<double><<<1, 64, 0, stream>>>(out2, R[0].g + 13, opt(OPT_CG_VERIFY) == 2 ? 1 : 0);
      PISO_TRY(comm.allreduce(R, 13, 1, stream));
      PISO_LAUNCH_CHECK();
      PISO_HIP_CHECK(hipMemcpyAsync(&tl_slab_pinned->errsum, R[0].g + 13, sizeof(double), hipMemcpyDeviceToHost, stream));
      PISO_HIP_CHECK(hipStreamSynchronize(stream));
      ++comm.rccl->verify_runs;
      if (tl_slab_pinned->errsum != 0) {
        ++comm.rccl->verify_failures;
        ++comm.rccl->persist_fallbacks;
        return kPersistRetry;
      }
    }
    for (size_t q = 0; q < R.size(); ++q)
      slab_copy_rows<double><<<gflat[q], kBlock, 0, stream>>>(R[q].a.x, R[q].x_out, (size_t)R[q].a.nx * R[q].a.ny);
    PISO_LAUNCH_CHECK();
    // every rank returns the same status (peer transport: a wait may have given up on one rank only)
    if (comm.rccl) return comm_agree(comm.rccl, "slab CG", stream);
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    return PISO_OK;
  }
};

// Set up the ranks found in `R` (L, b, x_out, rank already filled in) inside `ws`, then iterate.
static int slab_solve(std::vector<SlabRank>& R, Comm& comm, int nx, int nyl, int per_x, const double* const* b,
                      double global_cells, float accuracy, int max_iterations, int rank_deficient, int reset,
                      int* iterations_out, char* ws, hipStream_t stream) {
  const int nloc = (int)R.size();
  const size_t n = (size_t)nx * nyl, nh = (size_t)nx * (nyl + 2), ws_per_rank = slab_rank_bytes(nx, nyl);
  // the g buffers of all local ranks are contiguous (loopback all-reduce walks them with a fixed stride)
  double* gall = reinterpret_cast<double*>(ws);
  const size_t gbytes = align_up((size_t)nloc * 16 * sizeof(double), 256);
  comm.g_stride = 16;
  PISO_HIP_CHECK(hipMemsetAsync(gall, 0, gbytes, stream));
  const int gflat = grid_for((long long)n, kBlock * 4);
  // r, p, x with their halo rows and the partial sums: before the first attempt and again before the second
  const auto zero_state = [&](SlabRank& k) -> int {
    PISO_HIP_CHECK(hipMemsetAsync(k.rbase, 0, nh * sizeof(double), stream));
    PISO_HIP_CHECK(hipMemsetAsync(k.pbase[0], 0, nh * sizeof(double), stream));
    PISO_HIP_CHECK(hipMemsetAsync(k.pbase[1], 0, nh * sizeof(double), stream));
    PISO_HIP_CHECK(hipMemsetAsync(k.xbase, 0, nh * sizeof(double), stream));
    cg_zero_partials<double><<<(3 * kMaxPartials + 255) / 256, 256, 0, stream>>>(k.a.partsA, k.a.partsB, k.a.partsS);
    return PISO_OK;
  };
  for (int q = 0; q < nloc; ++q) {
    SlabRank& k = R[q];
    Arena ar(ws + gbytes + (size_t)q * ws_per_rank, ws_per_rank);
    k.g = gall + (size_t)q * 16;
    slab_carve(ar, n, nh, k);
    if (!ar.ok()) { set_error_msg("piso_cg_solve_slab: workspace too small"); return PISO_ERR_INVALID_ARG; }
    CgArgs<double>& a = k.a;
    a.cC = k.cC; a.b = b[q];
    a.r = k.rbase + nx; a.p[0] = k.pbase[0] + nx; a.p[1] = k.pbase[1] + nx; a.x = k.xbase + nx;
    a.nx = nx; a.ny = nyl; a.per_x = per_x; a.per_y = 2;
    a.gA = nullptr; a.gB = nullptr; a.nt = 0;
    a.nx_true = 0; a.ny_true = 0; a.ncells = 0.0;
    PISO_HIP_CHECK(hipMemsetAsync(k.flags, 0, 4 * sizeof(int), stream));
    PISO_TRY(zero_state(k));
    // symmetry is checked inside the slab (per_y = 2: the N entries of its last row pair with S entries on the neighbour - the
    // persistent kernel reads them from the N array, so nothing is assumed about that pair)
    cg_setup_coeffs<double><<<gflat, kBlock, 0, stream>>>(k.L, k.cC, k.oT, k.oF, a.partsS, k.flags, n, nx, nyl, per_x, 2);
    slab_collapse<double><<<1, kBlock, 0, stream>>>(a.partsS, gflat, 1, k.g + 8);
    slab_flags_to_sums<double><<<1, 64, 0, stream>>>(k.flags, k.g + 8);
  }
  PISO_LAUNCH_CHECK();
  PISO_TRY(comm.allreduce(R, 8, 4, stream));               // every rank reads the same flags: the same instance, the same collectives
  double hg[4];
  PISO_HIP_CHECK(hipMemcpyAsync(hg, R[0].g + 8, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  const CgCoefs coefs = cg_coefs(hg[1], hg[2], hg[3], opt_on(OPT_CG_NO_COMPACT), opt_on(OPT_CG_NO_RECON), opt_on(OPT_CG_NO_SYM));
  // (second attempt: a persistent segment failed on some rank - every rank restarts the solve on the two-kernel iteration)
  return cg_retry_without_segments("slab CG", [&](bool allow_persist) {
    for (int q = 0; q < nloc; ++q) {
      SlabRank& k = R[q];
      if (!allow_persist) {
        PISO_TRY(zero_state(k));
        k.a.gA = nullptr; k.a.gB = nullptr;
      }
      cg_init<double><<<gflat, kBlock, 0, stream>>>(k.a, rank_deficient, k.g + 8, global_cells);
      if (coefs.compact) { k.a.oS = k.oF; k.a.oW = k.oF + n; k.a.oE = k.oF + 2 * n; k.a.oN = k.oF + 3 * n; }
      else { k.a.oS = k.oT; k.a.oW = k.oT + n; k.a.oE = k.oT + 2 * n; k.a.oN = k.oT + 3 * n; }
    }
    PISO_TRY(comm.exchange(R, HALO_R, stream));            // halo rows of r0 = b
    return cg_with_instance<double>(coefs, nx % (16 / (int)sizeof(double)) == 0, [&](auto inst) {
      using I = decltype(inst);
      SlabLink<typename I::CT, I::V, I::RECON> link{R, comm, stream};
      PISO_TRY(link.start(accuracy, coefs.symmetric, allow_persist, global_cells));
      return cg_iterate(link, max_iterations, reset, false, iterations_out);
    });
  });
}

}  // namespace piso

using namespace piso;

extern "C" {

size_t piso_cg_slab_workspace_bytes(int nx, int ny_local, int local_ranks) {
  return (size_t)local_ranks * slab_rank_bytes(nx, ny_local) + align_up((size_t)local_ranks * 16 * sizeof(double), 256) + 4096;
}

int piso_cg_solve_slab_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local,
                           const double* divergence_local, double* x_out_local, double* x_out_global, float accuracy,
                           int max_iterations, int rank_deficient, int residual_reset, int* iterations_out, void* workspace,
                           size_t workspace_bytes, piso_stream_t stream_) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  if (!comm || nx < 1 || ny_local < 1 || !laplace_local || !divergence_local || !x_out_local || !workspace || residual_reset < 1) {
    set_error_msg("piso_cg_solve_slab_f64: invalid argument");
    return PISO_ERR_INVALID_ARG;
  }
  if (workspace_bytes < piso_cg_slab_workspace_bytes(nx, ny_local, 1)) { set_error_msg("piso_cg_solve_slab_f64: workspace too small"); return PISO_ERR_INVALID_ARG; }
  PisoComm* pc = static_cast<PisoComm*>(comm);
  PISO_TRY(comm_ready(pc, "piso_cg_solve_slab_f64: peer communicator not connected"));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::vector<SlabRank> R(1);
  R[0].L = laplace_local; R[0].x_out = x_out_local; R[0].rank = pc->rank;
  Comm cm;
  cm.world = pc->world; cm.periodic_y = periodic_y != 0; cm.rccl = pc; cm.g_stride = 16;
  const double* b[1] = {divergence_local};
  const int rc = slab_solve(R, cm, nx, ny_local, periodic_x, b, (double)nx * ny_local * pc->world, accuracy, max_iterations,
                            rank_deficient, residual_reset, iterations_out, static_cast<char*>(workspace), stream);
  if (rc != PISO_OK) return rc;
  if (x_out_global) {                                       // every rank receives the whole field (replicated PISO step)
    if (pc->world == 1) {
      PISO_HIP_CHECK(hipMemcpyAsync(x_out_global, x_out_local, (size_t)nx * ny_local * sizeof(double), hipMemcpyDeviceToDevice, stream));
    } else if (pc->transport == TRANSPORT_PEER) {
      set_error_msg("piso_cg_solve_slab_f64: x_out_global is an RCCL all-gather; with the peer transport pass NULL and gather the slabs yourself");
      return PISO_ERR_INVALID_ARG;
    } else {
      PISO_TRY(comm_allgather_f64(pc, x_out_local, x_out_global, (size_t)nx * ny_local, stream));
    }
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  return PISO_OK;
}

int piso_cg_solve_slab_emulated_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace,
                                    const double* divergence, double* x_out, float accuracy, int max_iterations,
                                    int rank_deficient, int residual_reset, int* iterations_out, void* workspace,
                                    size_t workspace_bytes, piso_stream_t stream_) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  if (slabs < 1 || nx < 1 || ny < slabs || ny % slabs != 0 || !laplace || !divergence || !x_out || !workspace || residual_reset < 1) {
    set_error_msg("piso_cg_solve_slab_emulated_f64: invalid argument (ny must be a multiple of slabs)");
    return PISO_ERR_INVALID_ARG;
  }
  const int nyl = ny / slabs;
  if (workspace_bytes < piso_cg_slab_workspace_bytes(nx, nyl, slabs)) { set_error_msg("piso_cg_solve_slab_emulated_f64: workspace too small"); return PISO_ERR_INVALID_ARG; }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::vector<SlabRank> R(slabs);
  std::vector<const double*> b(slabs);
  for (int r = 0; r < slabs; ++r) {
    const size_t off = (size_t)r * nyl * nx;
    R[r].L = laplace + off * 5; R[r].x_out = x_out + off; R[r].rank = r;
    b[r] = divergence + off;
  }
  Comm cm;
  cm.world = slabs; cm.periodic_y = periodic_y != 0; cm.rccl = nullptr; cm.g_stride = 16;
  return slab_solve(R, cm, nx, nyl, periodic_x, b.data(), (double)nx * ny, accuracy, max_iterations, rank_deficient,
                    residual_reset, iterations_out, static_cast<char*>(workspace), stream);
}

}  // extern "C"
