// Host driver of the single-GPU pressure CG (kernels: cg_kernels.h).  See cg_kernels.h for the design.
#include <atomic>
#include "cg_kernels.h"
#include "cg_driver.h"
#include "cg_tiny.h"
#include "options.h"
#include <cstdio>
#include <vector>

namespace piso {

// ---------------------------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------------------------
struct CgProfile {
  int enabled = 0, stride = 8;
  double ms[4] = {0, 0, 0, 0};          // K1, K2, persistent segments, (unused)
  long long count[4] = {0, 0, 0, 0};    // launches of K1, K2; ITERATIONS executed inside persistent segments; segment LAUNCHES
};
static CgProfile g_prof;

struct HostPoll {
  CgState* pinned = nullptr;   // [2]
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipEvent_t seg_ev[2] = {nullptr, nullptr};   // timing events around persistent segments (profiling only; created once)
  int cus = 0;                                 // compute units of the device
};
static std::atomic<unsigned> g_persist_launches{0};   // persistent launches so far: the high half of their exchange tags
static int g_persist_fallbacks = 0;            // solves that were restarted on the two-kernel path after an exchange timed out
// option cg_xcd_map 1 (tests): the XCD every workgroup of the solve's LAST chip-wide persistent launch ran on (cg_persist.h: hier_enter)
static thread_local int tl_xcd_map[kPersistMaxGrid];
static thread_local int tl_xcd_map_n = 0;
static long long g_tiny_solves = 0;            // solves that ran inside one workgroup (cg_tiny.h)
// which kernel instance the calling thread's last solve was dispatched to (piso_cg_last_dispatch; fields: include/piso_hip.h)
enum { DI_PATH = 0, DI_SIZEOF_T, DI_SIZEOF_CT, DI_V, DI_RECON, DI_SYMMETRIC, DI_ROWS_PER_WAVE, DI_K1_GRID, DI_K1_TILES, DI_R, DI_NQ,
       DI_WAVES, DI_LAUNCH_GRID, DI_PADDED, DI_XCD_LOCAL, DI_FELL_BACK, DI_TINY_PER_X, DI_K2_GRID, DI_SEGMENTS, DI_COUNT };
static thread_local int tl_dispatch[DI_COUNT];
static thread_local int tl_dispatch_n = 0;
static bool g_xcd_local_failed = false;        // an XCD-local launch gave up once (the device does not behave as assumed): not tried again
static long long g_verify_runs = 0;            // solves whose final state was checked against the true residual (cg_verify_gap)
static int g_verify_failures = 0;              // ... and failed: restarted on the two-kernel path
// one per device and thread (events belong to the device that was current when they were created); ensure_poll() selects
constexpr int kPollDevices = 16;
static thread_local HostPoll tl_poll_dev[kPollDevices];
static thread_local HostPoll* tl_poll_cur = &tl_poll_dev[0];
#define tl_poll (*tl_poll_cur)

static int ensure_poll() {
  int dev = 0;
  PISO_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kPollDevices) { set_error_msg("piso_cg_solve: device ordinal out of range"); return PISO_ERR_INVALID_ARG; }
  tl_poll_cur = &tl_poll_dev[dev];
  if (!tl_poll.pinned) {
    PISO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&tl_poll.pinned), 2 * sizeof(CgState), hipHostMallocDefault));
    PISO_HIP_CHECK(hipEventCreateWithFlags(&tl_poll.ev[0], hipEventDisableTiming));
    PISO_HIP_CHECK(hipEventCreateWithFlags(&tl_poll.ev[1], hipEventDisableTiming));
    PISO_HIP_CHECK(hipDeviceGetAttribute(&tl_poll.cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  return PISO_OK;
}

// Padded-grid mode: a wall-bounded grid the persistent kernel cannot tile (row length not a multiple of 128 cells, rows not a
// multiple of the region height - e.g. the lid-driven cavity's 64 x 65) is embedded in the next grid it can: zero coefficients
// and a zero right-hand side keep the padding at zero (the kernels that add the rank-1 shift skip it, cg_kernels.h).  Only for
// small grids, where two dependent launches per iteration cost ~14 us against ~4 us of a persistent iteration; periodic axes
// cannot be padded (the wrap partner would move).
constexpr size_t kPadMaxCells = (size_t)1 << 19;
static bool padded_dims(int nx, int ny, int per_x, int per_y, int elem, int* nxp, int* nyp) {
  *nxp = nx; *nyp = ny;
  if (elem != 8 || nx % 2 != 0 || nx < 8 || ny < 8) return false;
  // grids the kernel tiles as they are stay as they are: rows of whole 128-cell strips, an even number of rows (regions of 2)
  const bool pad_x = nx % 128 != 0, pad_y = ny % 2 != 0;
  if (!pad_x && !pad_y) return false;
  const int px = (nx + 127) / 128 * 128;
  int py = (ny + 3) / 4 * 4;                      // rows a multiple of 4: the number of 2-row regions comes out even (two per wave)
  if (px != nx && per_x) return false;
  if (py != ny && per_y) {
    py = ny;                                      // periodic in y: only x is padded, if the region count still works out
    if (ny % 2 != 0 || ((long long)(px / 128) * (ny / 2)) % 2 != 0) return false;
  }
  if ((size_t)px * py > kPadMaxCells) return false;
  *nxp = px; *nyp = py;
  return true;
}

// The workspace of a solve on n cells (of the padded grid, if `padded`), in this order.  cg_workspace_bytes counts it.
template <typename T>
struct CgCarve { T *cC, *oT; float* oF; int* flags; T *b_pad, *x_pad; unsigned* persist_ws; };
template <typename T>
static CgCarve<T> cg_carve(Arena& ar, size_t n, bool padded, CgArgs<T>& a) {
  CgCarve<T> c;
  c.cC = ar.take<T>(n);
  c.oT = ar.take<T>(4 * n);
  c.oF = ar.take<float>(4 * n);
  c.flags = ar.take<int>(4);
  c.b_pad = padded ? ar.take<T>(n) : nullptr;
  c.x_pad = padded ? ar.take<T>(n) : nullptr;
  a.r = ar.take<T>(n); a.z = ar.take<T>(n); a.p[0] = ar.take<T>(n); a.p[1] = ar.take<T>(n);
  a.zp[0] = ar.take<T>(n); a.zp[1] = ar.take<T>(n);
  a.partsA = ar.take<T>(3 * kMaxPartials); a.partsB = ar.take<T>(3 * kMaxPartials); a.partsS = ar.take<T>(kMaxPartials);
  a.scal = ar.take<T>(SC_COUNT);
  a.state = ar.take<CgState>(2);
  c.persist_ws = ar.take<unsigned>(kPersistWsWordsAll);
  return c;
}

// (an upper bound: the periodicity is not known here, and periodic grids are never padded.  A grid that may be padded has always been
// advertised as the plain carve on THREE times its padded cells - more than its two padded copies of b and x take - and stays so.)
template <typename T>
static size_t cg_workspace_bytes(int nx_in, int ny_in) {
  int nx = nx_in, ny = ny_in;
  const bool padded = padded_dims(nx_in, ny_in, 0, 0, (int)sizeof(T), &nx, &ny);
  Arena ar = counting_arena();
  CgArgs<T> a;
  cg_carve<T>(ar, (padded ? 3 : 1) * (size_t)nx * ny, false, a);
  return counted_bytes(ar);
}

// The calling thread's dispatch record (fields: include/piso_hip.h).  One workgroup (cg_tiny.h): path 0 / 1, no tiling, no plan;
// otherwise path 2 / 3 and the shape fields from the plan.
static void record_dispatch(int path, size_t state_bytes, size_t coef_bytes, int tiny_per_x, int V = 0, bool recon = false, bool symmetric = false,
                            const CgTiling* t = nullptr, const PersistPlan* p = nullptr, bool fell_back = false) {
  int* d = tl_dispatch;
  for (int i = 0; i < DI_COUNT; ++i) d[i] = 0;
  d[DI_PATH] = path; d[DI_SIZEOF_T] = (int)state_bytes; d[DI_SIZEOF_CT] = (int)coef_bytes; d[DI_TINY_PER_X] = tiny_per_x;
  d[DI_V] = V; d[DI_RECON] = recon ? 1 : 0; d[DI_SYMMETRIC] = symmetric ? 1 : 0; d[DI_FELL_BACK] = fell_back ? 1 : 0;
  if (t) { d[DI_ROWS_PER_WAVE] = t->rows_per_wave; d[DI_K1_GRID] = t->g1; d[DI_K1_TILES] = t->k1_tiles; d[DI_K2_GRID] = t->g2; }
  if (p) d[DI_PADDED] = p->ragged ? 1 : 0;
  if (p && p->R) { d[DI_R] = p->R; d[DI_NQ] = p->NQ; d[DI_WAVES] = p->waves; d[DI_LAUNCH_GRID] = p->launch_grid; d[DI_XCD_LOCAL] = p->xcd_local ? 1 : 0; }
  tl_dispatch_n = DI_COUNT;
}

struct EventPool {
  static constexpr int kMax = 64;
  hipEvent_t start[2][kMax], stop[2][kMax];
  int used[2] = {0, 0};
  bool created = false;
};
static thread_local EventPool tl_events;
struct SegmentTimes { double ms = 0; long long iters = 0, launches = 0; };   // profiling: persistent segments of one solve

static int ensure_events(EventPool& ep) {
  if (ep.created) return PISO_OK;
  for (int q = 0; q < 2; ++q)
    for (int i = 0; i < EventPool::kMax; ++i) {
      PISO_HIP_CHECK(hipEventCreate(&ep.start[q][i]));
      PISO_HIP_CHECK(hipEventCreate(&ep.stop[q][i]));
    }
  ep.created = true;
  return PISO_OK;
}

// profiling: what the solve's sampled K1 / K2 launches and its persistent segments took -> kernel_ms_out (per launch / per iteration), g_prof
static int read_profile(const EventPool& ep, const SegmentTimes& seg, float* kernel_ms_out) {
  double ms[2] = {0, 0};
  for (int q = 0; q < 2; ++q)
    for (int i = 0; i < ep.used[q]; ++i) {
      float t = 0;
      PISO_HIP_CHECK(hipEventElapsedTime(&t, ep.start[q][i], ep.stop[q][i]));
      ms[q] += t;
    }
  if (kernel_ms_out) {
    kernel_ms_out[0] = ep.used[0] ? (float)(ms[0] / ep.used[0]) : 0.f;
    kernel_ms_out[1] = ep.used[1] ? (float)(ms[1] / ep.used[1]) : 0.f;
  }
  if (g_prof.enabled) {
    for (int q = 0; q < 2; ++q) { g_prof.ms[q] += ms[q]; g_prof.count[q] += ep.used[q]; }
    g_prof.ms[2] += seg.ms; g_prof.count[2] += seg.iters; g_prof.count[3] += seg.launches;
  }
  if (kernel_ms_out && seg.iters > 0) { kernel_ms_out[0] = (float)(seg.ms / seg.iters); kernel_ms_out[1] = 0.f; }
  return PISO_OK;
}

// diagnostic builds only (kPersistDiag, option cg_persist_timing): the per-phase clocks of every workgroup, freed with the solve
struct PersistTiming {
  unsigned long long* ticks = nullptr;
  ~PersistTiming() { if (ticks) (void)hipFree(ticks); }
};
static int print_persist_timing(const unsigned long long* ticks, int grid, int k_last) {
  std::vector<unsigned long long> h(12 * grid);
  PISO_HIP_CHECK(hipMemcpy(h.data(), ticks, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const char* names[9] = {"D (p update, stencil, sums, publish)", "exchange", "U (stencil, x / r update, ring)", "-", "-",
                           "  exchange: wave sums + drain of the perimeter stores", "  exchange: first barrier", "  exchange: publish + polling",
                           "  exchange: record sums + second barrier"};
  const double f = 0.01 / (double)(k_last > 0 ? k_last : 1);   // 100 MHz ticks -> us per iteration
  if (opt(OPT_CG_PERSIST_TIMING) >= 2) {                  // the whole table: one line per workgroup
    for (int b = 0; b < grid; ++b)
      fprintf(stderr, "cg_persist_wg %3d xcd %d band %3d  D %.2f  exchange %.2f  U %.2f  | drain %.2f  barrier1 %.2f  publish+poll %.2f  sums %.2f\n", b, (int)h[9 * grid + b], (int)h[10 * grid + b],
              f * (double)h[0 * grid + b], f * (double)h[1 * grid + b], f * (double)h[2 * grid + b],
              f * (double)h[5 * grid + b], f * (double)h[6 * grid + b], f * (double)h[7 * grid + b], f * (double)h[8 * grid + b]);
  }
  for (int q = 0; q < 9; ++q) {
    double s = 0, mn = 1e300, mx = 0;
    for (int b = 0; b < grid; ++b) { const double v = (double)h[q * grid + b]; s += v; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    fprintf(stderr, "cg_persist %s: avg %.2f us/iter  min %.2f  max %.2f\n", names[q], f * s / grid, f * mn, f * mx);
  }
  return PISO_OK;
}

// The persistent kernel lets workgroups read what others published without release / acquire fences (cg_persist1.h).  That is
// checked at run time instead of being trusted: r - the CG recurrence - must still equal b - A^ x for the x the solve returns (to
// eps * condition * |b|; a stale perimeter value would leave an O(alpha |z'|) gap that nothing removes before the next residual
// reset).  One stencil pass per solve; the driver restarts a solve that fails on the two-kernel path and counts it.
template <typename T, typename CT>
static int verify_residual(const CgArgs<T>& a, const PersistCtl& pc, hipStream_t stream, bool* failed) {
  unsigned* out2 = reinterpret_cast<unsigned*>(pc.err) + 4;
  PISO_HIP_CHECK(hipMemsetAsync(out2, 0, 2 * sizeof(unsigned), stream));
  const int gvf = grid_for((long long)a.nx * a.ny, kBlock * 4, 1024);
  cg_verify_sum_x<T><<<gvf, kBlock, 0, stream>>>(a, a.partsA);
  cg_verify_gap<T, CT><<<gvf, kBlock, 0, stream>>>(a, a.partsA, gvf, out2);
  PISO_LAUNCH_CHECK();
  unsigned h2[2] = {0, 0};
  PISO_HIP_CHECK(hipMemcpyAsync(h2, out2, sizeof(h2), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  float gap, scale;
  memcpy(&gap, &h2[0], 4); memcpy(&scale, &h2[1], 4);
  ++g_verify_runs;
  *failed = (gap > 1e-5f * scale && gap > 1e-30f) || opt(OPT_CG_VERIFY) == 2;     // (2: test knob - treat the check as failed)
  return PISO_OK;
}

// waits for poll `slot`: 1 if the solver reported done (*stop_it: at which iteration), 0 if not, -1 on an error
static int inspect_poll(int slot, int* stop_it) {
  hipError_t e = hipEventSynchronize(tl_poll.ev[slot]);
  if (e != hipSuccess) { set_error("hipEventSynchronize", e); return -1; }
  if (tl_poll.pinned[slot].done) { *stop_it = tl_poll.pinned[slot].iterations; return 1; }
  return 0;
}
// poll cadence of the two-kernel iteration: about 1 ms of work between host looks, never fewer than 10 iterations
static int poll_batch(size_t n) {
  const double t_iter_us = (double)n * 120.0 / 4.0e6;    // ~4 TB/s
  const int batch = (int)(1000.0 / (t_iter_us < 8.0 ? 8.0 : t_iter_us));
  return batch < 10 ? 10 : (batch > 200 ? 200 : batch);
}

// The one-GPU link of the iteration (cg_driver.h: cg_iterate): single launches, no halo rows.  Its own: the events around sampled
// NORMAL K1 / K2 launches, the host's looks (one batch behind on the two-kernel path; after a persistent segment, deferred while the
// segments are short), the XCD map, the per-phase timing, the true-residual check, the dispatch record.
template <typename T, typename CT, int V, bool RECON>
struct GpuLink {
  CgArgs<T> a;
  hipStream_t stream;
  bool fixed, prof;
  CgTiling tile;
  PersistPlan plan;                                      // confirmed by the occupancy of the instance it names (cg_dispatch.h)
  PersistCtl pc;
  PersistTiming timing;
  int seg_len, batch, prof_stride, polls = 0, unsynced = 0;
  bool sample = false;                                   // events around this iteration's K1 / K2: sampled NORMAL iterations only
  SegmentTimes seg;
  EventPool& ep = tl_events;

  // everything before the first iteration: tiling, cg_init, the plan of the persistent part, the dispatch record
  int start(unsigned* persist_ws, bool symmetric, int rank_deficient, bool allow_persist) {
    const size_t n = (size_t)a.nx * a.ny;
    tile = cg_tile(a, V, opt(OPT_CG_RPW), opt(OPT_CG_MAXBLOCKS));                   // tuning knobs
    PISO_TRY(ensure_poll());
    if (prof) PISO_TRY(ensure_events(ep));
    ep.used[0] = ep.used[1] = 0;
    prof_stride = g_prof.stride > 0 ? g_prof.stride : 8;
    cg_init<T><<<tile.gflat, kBlock, 0, stream>>>(a, rank_deficient);
    PISO_LAUNCH_CHECK();
    batch = poll_batch(n);
    plan = persist_plan(PersistQuery{a.nx, a.ny, V, a.per_y, a.nx_true != 0, sizeof(T), sizeof(CT), RECON, symmetric, false, tl_poll.cus,
                                     opt(OPT_CG_PERSIST), opt(OPT_CG_PERSIST_R), opt(OPT_CG_PERSIST_HALF), opt(OPT_CG_PERSIST_NQ),
                                     opt(OPT_CG_XCD_LOCAL), g_xcd_local_failed, allow_persist});
    PISO_TRY((persist_prepare<T, CT, RECON, false>(plan, tl_poll.cus, pc, persist_ws, stream)));
    if (plan.R && kPersistDiag && opt_on(OPT_CG_PERSIST_TIMING)) {
      PISO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&timing.ticks), 12 * plan.launch_grid * sizeof(unsigned long long)));
      PISO_HIP_CHECK(hipMemsetAsync(timing.ticks, 0, 12 * plan.launch_grid * sizeof(unsigned long long), stream));
      pc.timing = timing.ticks;
    }
    record_dispatch(plan.R ? 3 : 2, sizeof(T), sizeof(CT), 0, V, RECON, symmetric, &tile, &plan, !allow_persist);
    seg_len = persist_segment_len(n, opt(OPT_CG_SEGMENT));
    hipEvent_t* seg_ev = tl_poll.seg_ev;
    if (plan.R && prof && !seg_ev[0]) { PISO_HIP_CHECK(hipEventCreate(&seg_ev[0])); PISO_HIP_CHECK(hipEventCreate(&seg_ev[1])); }
    return PISO_OK;
  }

  bool persistent() const { return plan.R != 0; }
  int segment(int k, int ke, CgLoop& st) {
    hipEvent_t* seg_ev = tl_poll.seg_ev;
    if (prof) PISO_HIP_CHECK(hipEventRecord(seg_ev[0], stream));
    PISO_TRY((persist_launch<T, CT, RECON, false>(plan, a, pc, g_persist_launches.fetch_add(1, std::memory_order_relaxed), k, ke, st.sv, st.pending, NoSlab{}, stream)));
    if (prof) PISO_HIP_CHECK(hipEventRecord(seg_ev[1], stream));
    // Short segments (frequent residual resets: the reference's default residual_reset = 10 leaves 9 iterations between two
    // resets) are not worth a host round trip each: the host looks again after ~250 iterations.  Everything queued behind a
    // converged or failed segment returns at once (every kernel checks the state record first), the error flag is sticky.
    const bool defer = !prof && ke - k <= 32 && unsynced + (ke - k) <= 256 && ke < st.total;
    unsynced = defer ? unsynced + (ke - k) : 0;
    if (defer) return PISO_OK;
    PISO_HIP_CHECK(hipMemcpyAsync(&tl_poll.pinned[0], &a.state[0], sizeof(CgState), hipMemcpyDeviceToHost, stream));
    int herr = 0;
    PISO_HIP_CHECK(hipMemcpyAsync(&herr, pc.err, sizeof(int), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    if (herr) {                                          // a grid-wide exchange gave up
      ++g_persist_fallbacks;
      if (plan.xcd_local) g_xcd_local_failed = true;
      return kPersistRetry;
    }
    const CgState& hst = tl_poll.pinned[0];
    if (prof) {
      // (a solve that converges inside the launch leaves it there: the iterations it RAN count, not the segment's length)
      const int ran = hst.done ? (hst.iterations - k > 0 ? hst.iterations - k : 0) : ke - k;
      float t = 0; PISO_HIP_CHECK(hipEventElapsedTime(&t, seg_ev[0], seg_ev[1])); seg.ms += t; seg.iters += ran < ke - k ? ran : ke - k; ++seg.launches;
    }
    if (hst.done) { st.finished = true; st.stop_it = hst.iterations; }
    return PISO_OK;
  }

  int k1(int k, int mode, int sv, int chk, int pend) {
    sample = prof && mode == MODE_NORMAL && (k % prof_stride == prof_stride - 1) && ep.used[0] < EventPool::kMax;
    if (sample) PISO_HIP_CHECK(hipEventRecord(ep.start[0][ep.used[0]], stream));
    cg_k1<T, CT, V, RECON><<<tile.g1, kBlock, 0, stream>>>(a, k, mode, sv, chk, pend);
    if (sample) PISO_HIP_CHECK(hipEventRecord(ep.stop[0][ep.used[0]++], stream));
    return PISO_OK;
  }
  int k2(int k, int sv) {
    if (sample) PISO_HIP_CHECK(hipEventRecord(ep.start[1][ep.used[1]], stream));
    cg_k2<T, V><<<tile.g2, kBlock, 0, stream>>>(a, k, sv);
    if (sample) PISO_HIP_CHECK(hipEventRecord(ep.stop[1][ep.used[1]++], stream));
    return PISO_OK;
  }
  int flush(int k, int sv) { cg_flush_x<T><<<tile.gflat, kBlock, 0, stream>>>(a, k, sv); return PISO_OK; }
  int reset_residual(int sv) { cg_reset_residual<T><<<tile.gflat, kBlock, 0, stream>>>(a, sv); return PISO_OK; }
  int halo(int) { return PISO_OK; }

  // queues a copy of the state record and looks at the PREVIOUS copy while this batch is already queued (now: waits for this one)
  int poll(CgLoop& st, bool now) {
    const int slot = polls & 1;
    PISO_HIP_CHECK(hipMemcpyAsync(&tl_poll.pinned[slot], &a.state[st.sv & 1], sizeof(CgState), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipEventRecord(tl_poll.ev[slot], stream));
    if (now || polls > 0) {
      const int r = inspect_poll(now ? slot : (polls - 1) & 1, &st.stop_it);
      if (r < 0) return PISO_ERR_HIP;
      if (r > 0) st.finished = true;
    }
    ++polls;
    return PISO_OK;
  }
  int look(int k, CgLoop& st) { return (!fixed && (k + 1) % batch == 0 && k + 1 < st.total) ? poll(st, false) : PISO_OK; }

  int finish(CgLoop& st) {
    // Final look.  (A success of the test that belongs to the very last iteration is not evaluated: the reference would
    // report iterations == total for it, which is what an unfinished loop reports as well.)
    if (!fixed && !st.finished) PISO_TRY(poll(st, true));
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    if (opt(OPT_CG_XCD_MAP) == 1) {
      tl_xcd_map_n = 0;
      if (st.segments_run > 0 && !plan.xcd_local && plan.grid <= kPersistMaxGrid) {
        PISO_HIP_CHECK(hipMemcpy(tl_xcd_map, pc.xcd + kPersistXcdTable, (size_t)plan.grid * sizeof(int), hipMemcpyDeviceToHost));
        tl_xcd_map_n = plan.grid;
      }
    }
    if (st.segments_run > 0) {                           // (segments whose host look was deferred: did one of them give up?)
      int herr = 0;
      PISO_HIP_CHECK(hipMemcpy(&herr, pc.err, sizeof(int), hipMemcpyDeviceToHost));
      if (herr) { ++g_persist_fallbacks; return kPersistRetry; }
    }
    if (st.segments_run > 0 && sizeof(T) == 8 && !fixed && opt(OPT_CG_VERIFY) != 0) {
      bool failed = false;
      PISO_TRY((verify_residual<T, CT>(a, pc, stream, &failed)));
      if (failed) { ++g_verify_failures; ++g_persist_fallbacks; return kPersistRetry; }
    }
    if (timing.ticks) PISO_TRY(print_persist_timing(timing.ticks, plan.grid, st.k_last));
    tl_dispatch[DI_SEGMENTS] = st.segments_run;
    return PISO_OK;
  }
};

// rows of nx elements between arrays of different leading dimensions (padded-grid mode: b in, x out)
template <typename T>
__global__ __launch_bounds__(kBlock) void cg_copy_rows(const T* __restrict__ src, T* __restrict__ dst, int nx, int ny, int ld_src, int ld_dst) {
  const size_t n = (size_t)nx * ny;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const size_t j = i / (size_t)nx, c = i % (size_t)nx;
    dst[j * (size_t)ld_dst + c] = src[j * (size_t)ld_src + c];
  }
}

template <typename T>
static int cg_solve(int nx, int ny, int per_x, int per_y, const T* L, const T* b, T* x_out, float accuracy,
                    int max_iterations, int rank_deficient, int reset, int fixed, int* iterations_out,
                    float* kernel_ms_out, void* ws, size_t ws_bytes, piso_stream_t stream_, int* iterations_dev = nullptr) {
  tl_dispatch_n = 0;
  if (nx < 1 || ny < 1 || !L || !b || !x_out || !ws || max_iterations < 0 || reset < 1) {
    set_error_msg("piso_cg_solve: invalid argument");
    return PISO_ERR_INVALID_ARG;
  }
  if (ws_bytes < cg_workspace_bytes<T>(nx, ny)) {
    set_error_msg("piso_cg_solve: workspace too small");
    return PISO_ERR_INVALID_ARG;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const size_t n_true = (size_t)nx * ny;
  if (n_true <= (size_t)kTinyMaxCells && opt(OPT_CG_TINY) != 0 && opt(OPT_CG_PERSIST) < 0) {   // (a forced / forbidden persistent path: tests)
    // a tiny grid (the lid-driven cavity): the whole solve in ONE workgroup, one launch (cg_tiny.h)
    CgState* st_dev = reinterpret_cast<CgState*>(ws);
    const int total = fixed ? fixed : max_iterations;
    hipEvent_t* ev = nullptr;
    if (kernel_ms_out) {
      { const int rc = ensure_poll(); if (rc != PISO_OK) return rc; }
      ev = tl_poll.seg_ev;
      if (!ev[0]) { PISO_HIP_CHECK(hipEventCreate(&ev[0])); PISO_HIP_CHECK(hipEventCreate(&ev[1])); }
      PISO_HIP_CHECK(hipEventRecord(ev[0], stream));
    }
    const bool async = iterations_dev != nullptr;         // the iteration count stays on the device: nothing waits for the solve
    const bool cols = nx <= 64 && ny <= kColsMaxNy && (!per_x || nx == 64) && opt(OPT_CG_TINY) != 2;    // (cg_tiny = 2: the general kernel, tests)
    if (cols && per_x)
      cg_tiny_cols<T, true><<<1, kTinyThreads, 0, stream>>>(L, b, x_out, nx, ny, per_y, fixed ? -1.0f : accuracy, total, fixed ? 0 : reset,
                                                            rank_deficient, st_dev, iterations_dev);
    else if (cols)
      cg_tiny_cols<T, false><<<1, kTinyThreads, 0, stream>>>(L, b, x_out, nx, ny, per_y, fixed ? -1.0f : accuracy, total, fixed ? 0 : reset,
                                                             rank_deficient, st_dev, iterations_dev);
    else
      cg_tiny<T><<<1, kTinyThreads, 0, stream>>>(L, b, x_out, nx, ny, per_x, per_y, fixed ? -1.0f : accuracy, total, fixed ? 0 : reset,
                                                 rank_deficient, st_dev, iterations_dev);
    PISO_LAUNCH_CHECK();
    ++g_tiny_solves;
    record_dispatch(cols ? 1 : 0, sizeof(T), sizeof(T), (cols && per_x) ? 1 : 0);
    if (async) return PISO_OK;
    if (ev) PISO_HIP_CHECK(hipEventRecord(ev[1], stream));
    CgState hst;
    PISO_HIP_CHECK(hipMemcpyAsync(&hst, st_dev, sizeof(CgState), hipMemcpyDeviceToHost, stream));
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
    if (iterations_out) *iterations_out = (!fixed && hst.done) ? hst.iterations : total;
    if (ev) { float ms = 0; PISO_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); kernel_ms_out[0] = total > 0 ? ms / (float)total : 0.f; kernel_ms_out[1] = 0.f; }
    return PISO_OK;
  }
  if (iterations_dev) {
    set_error_msg("piso_cg_solve_async: this grid is solved with the host in the loop (segments, stopping test): call piso_cg_solve");
    return PISO_ERR_NEEDS_HOST;
  }
  int nxp = nx, nyp = ny;
  const bool padded = opt(OPT_CG_PERSIST) != 0 && opt(OPT_CG_PAD) != 0 &&
                      padded_dims(nx, ny, per_x, per_y, (int)sizeof(T), &nxp, &nyp);      // (see padded_dims)
  const size_t n = (size_t)nxp * nyp;
  Arena ar(ws, ws_bytes);
  CgArgs<T> a;
  const CgCarve<T> c = cg_carve<T>(ar, n, padded, a);
  a.cC = c.cC;
  a.b = padded ? c.b_pad : b; a.x = padded ? c.x_pad : x_out;
  a.nx = nxp; a.ny = nyp; a.per_x = per_x; a.per_y = per_y;
  a.nx_true = padded ? nx : 0; a.ny_true = padded ? ny : 0; a.ncells = padded ? (double)n_true : 0.0;
  a.ntx = a.nty = a.rows_per_wave = 0; a.nA = a.nB = 0;
  a.accuracy = fixed ? -1.0f : accuracy;                   // fixed-work mode: the test can never succeed
  a.gA = nullptr; a.gB = nullptr;
  a.nt = 0;
  if (opt(OPT_CG_NT) > 0) a.nt = opt(OPT_CG_NT);
  if (!ar.ok()) { set_error_msg("piso_cg_solve: workspace too small"); return PISO_ERR_INVALID_ARG; }

  PISO_HIP_CHECK(hipMemsetAsync(c.flags, 0, 4 * sizeof(int), stream));
  cg_zero_partials<T><<<(3 * kMaxPartials + 255) / 256, 256, 0, stream>>>(a.partsA, a.partsB, a.partsS);
  const int gs = grid_for((long long)n_true, kBlock * 4);
  if (padded) {                                             // zero coefficients and a zero right-hand side keep the padding at zero
    PISO_HIP_CHECK(hipMemsetAsync(c.cC, 0, n * sizeof(T), stream));
    PISO_HIP_CHECK(hipMemsetAsync(c.oT, 0, 4 * n * sizeof(T), stream));
    PISO_HIP_CHECK(hipMemsetAsync(c.oF, 0, 4 * n * sizeof(float), stream));
    PISO_HIP_CHECK(hipMemsetAsync(c.b_pad, 0, n * sizeof(T), stream));
    cg_copy_rows<T><<<gs, kBlock, 0, stream>>>(b, c.b_pad, nx, ny, nx, nxp);
  }
  cg_setup_coeffs<T><<<gs, kBlock, 0, stream>>>(L, c.cC, c.oT, c.oF, a.partsS, c.flags, n_true, nx, ny, per_x, per_y, padded ? nxp : 0, padded ? n : 0);
  PISO_LAUNCH_CHECK();
  int hflags[3] = {1, 1, 1};
  PISO_HIP_CHECK(hipMemcpyAsync(hflags, c.flags, 3 * sizeof(int), hipMemcpyDeviceToHost, stream));
  PISO_HIP_CHECK(hipStreamSynchronize(stream));
  const CgCoefs coefs = cg_coefs(hflags[0], hflags[1], hflags[2], opt_on(OPT_CG_NO_COMPACT), opt_on(OPT_CG_NO_RECON), opt_on(OPT_CG_NO_SYM));
  // (compact with fp32 state: trivially exact - the same path, so that the diagonal can be rebuilt there too)
  if (coefs.compact) { a.oS = c.oF; a.oW = c.oF + n; a.oE = c.oF + 2 * n; a.oN = c.oF + 3 * n; }
  else { a.oS = c.oT; a.oW = c.oT + n; a.oE = c.oT + 2 * n; a.oN = c.oT + 3 * n; }
  const bool aligned = ((reinterpret_cast<uintptr_t>(a.b) | reinterpret_cast<uintptr_t>(a.x)) & 15) == 0;
  const bool vec = aligned && (nxp % (16 / (int)sizeof(T)) == 0);
  const bool prof = (kernel_ms_out != nullptr) || g_prof.enabled;
  const int rc = cg_retry_without_segments("piso_cg_solve", [&](bool allow_persist) {
    return cg_with_instance<T>(coefs, vec, [&](auto inst) {
      using I = decltype(inst);
      GpuLink<T, typename I::CT, I::V, I::RECON> link{a, stream, fixed != 0, prof};
      PISO_TRY(link.start(c.persist_ws, coefs.symmetric, rank_deficient, allow_persist));
      PISO_TRY(cg_iterate(link, fixed ? fixed : max_iterations, reset, fixed != 0, iterations_out));
      return prof ? read_profile(link.ep, link.seg, kernel_ms_out) : PISO_OK;
    });
  });
  if (rc != PISO_OK) return rc;
  if (padded) {                                             // (the solve has synchronised the stream: x_pad is final)
    cg_copy_rows<T><<<gs, kBlock, 0, stream>>>(c.x_pad, x_out, nx, ny, nxp, nx);
    PISO_LAUNCH_CHECK();
    PISO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  return PISO_OK;
}

}  // namespace piso

using namespace piso;

extern "C" {

size_t piso_cg_workspace_bytes(int nx, int ny, int elem_size) {
  return elem_size == 8 ? cg_workspace_bytes<double>(nx, ny) : cg_workspace_bytes<float>(nx, ny);
}

int piso_cg_solve_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                      double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                      int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  return cg_solve<double>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations,
                          rank_deficient, residual_reset, 0, iterations_out, nullptr, workspace, workspace_bytes, stream);
}

int piso_cg_solve_f32(int nx, int ny, int periodic_x, int periodic_y, const float* laplace, const float* divergence,
                      float* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                      int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  return cg_solve<float>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations,
                         rank_deficient, residual_reset, 0, iterations_out, nullptr, workspace, workspace_bytes, stream);
}

int piso_cg_solve_async_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                            double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                            int* iterations_dev, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  if (!iterations_dev) { set_error_msg("piso_cg_solve_async: iterations_dev is NULL"); return PISO_ERR_INVALID_ARG; }
  return cg_solve<double>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations,
                          rank_deficient, residual_reset, 0, nullptr, nullptr, workspace, workspace_bytes, stream, iterations_dev);
}

int piso_cg_solve_async_f32(int nx, int ny, int periodic_x, int periodic_y, const float* laplace, const float* divergence,
                            float* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                            int* iterations_dev, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  if (!iterations_dev) { set_error_msg("piso_cg_solve_async: iterations_dev is NULL"); return PISO_ERR_INVALID_ARG; }
  return cg_solve<float>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, accuracy, max_iterations,
                         rank_deficient, residual_reset, 0, nullptr, nullptr, workspace, workspace_bytes, stream, iterations_dev);
}

int piso_cg_fixed_iterations_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace,
                                 const double* divergence, double* x_out, int rank_deficient, int iterations,
                                 float* kernel_ms_out, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  if (iterations < 1) { set_error_msg("piso_cg_fixed_iterations: iterations < 1"); return PISO_ERR_INVALID_ARG; }
  return cg_solve<double>(nx, ny, periodic_x, periodic_y, laplace, divergence, x_out, 0.f, iterations, rank_deficient,
                          1 << 30, iterations, nullptr, kernel_ms_out, workspace, workspace_bytes, stream);
}

void piso_cg_profile_enable(int enable, int stride) {
  g_prof.enabled = enable;
  if (stride > 0) g_prof.stride = stride;
  for (int q = 0; q < 4; ++q) { g_prof.ms[q] = 0; g_prof.count[q] = 0; }
}

int piso_cg_persist_fallbacks(void) { return g_persist_fallbacks; }
int piso_cg_last_xcd_map(int* out, int capacity) {
  const int n = tl_xcd_map_n < capacity ? tl_xcd_map_n : capacity;
  for (int i = 0; i < n; ++i) out[i] = tl_xcd_map[i];
  return tl_xcd_map_n;
}
long long piso_cg_tiny_solves(void) { return g_tiny_solves; }
int piso_cg_last_dispatch(int* out, int capacity) {
  const int n = tl_dispatch_n < capacity ? tl_dispatch_n : capacity;
  for (int i = 0; i < n; ++i) out[i] = tl_dispatch[i];
  return tl_dispatch_n;
}
void piso_cg_verify_stats(long long* runs_out, int* failures_out) {
  if (runs_out) *runs_out = g_verify_runs;
  if (failures_out) *failures_out = g_verify_failures;
}

void piso_cg_profile_read(double* ms_sum, long long* count) {
  for (int q = 0; q < 4; ++q) { ms_sum[q] = g_prof.ms[q]; count[q] = g_prof.count[q]; }
}

}  // extern "C"
