// The communicator of the slab pressure CG (cg_slab.hip), the slab ILU(0)-BiCGStab (bicgstab.hip) and the sharded step's halo exchanges
// (piso_comm_exchange / piso_comm_check); slab_comm.h is its interface.  Two transports, and this unit alone chooses between them:
//   * PEER (default inside a node): peer-mapped mailboxes (peer.h), shared as hipIpc handles or as POSIX file descriptors.  Exercised on
//     a single-GPU box as well: several PROCESSES share the device and run their kernels concurrently (tests/test_gpu_multiproc.py);
//   * RCCL (librccl is dlopen'ed on first use, so the library has no link-time dependency on it).
#include <dlfcn.h>

#include "options.h"
#include "slab_comm.h"

namespace piso {

// ------------------------------------------------------------------------------------------------ RCCL (lazy)
struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;

static int load_rccl() {
  if (g_rccl.handle) return PISO_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
  if (!h) { set_error_msg("cannot dlopen librccl"); return PISO_ERR_HIP; }
#define PISO_SYM(field, sym) \
  *reinterpret_cast<void**>(&g_rccl.field) = dlsym(h, sym); \
  if (!g_rccl.field) { set_error_msg("librccl lacks " sym); return PISO_ERR_HIP; }
  PISO_SYM(GetUniqueId, "ncclGetUniqueId") PISO_SYM(CommInitRank, "ncclCommInitRank") PISO_SYM(CommDestroy, "ncclCommDestroy")
  PISO_SYM(AllReduce, "ncclAllReduce") PISO_SYM(AllGather, "ncclAllGather") PISO_SYM(Send, "ncclSend") PISO_SYM(Recv, "ncclRecv")
  PISO_SYM(GroupStart, "ncclGroupStart") PISO_SYM(GroupEnd, "ncclGroupEnd") PISO_SYM(GetErrorString, "ncclGetErrorString")
#undef PISO_SYM
  g_rccl.handle = h;
  return PISO_OK;
}

// "<who>: <what>" as the error message; returns `code`
static int fail(int code, const char* who, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  set_error_msg(buf);
  return code;
}
#define PISO_NCCL_CHECK(expr) \
  do { const ncclResult_t _r = (expr); if (_r != ncclSuccess) return fail(PISO_ERR_HIP, #expr, g_rccl.GetErrorString(_r)); } while (0)

// ---- peer transport: one wave sums `count` <= 8 values of every rank.  Lane l < 2 count carries half l & 1 of value l / 2 as a
// tagged word to every rank's mailbox (mine included), then polls the `world` records of its own mailbox and adds them in
// rank order: every rank obtains bitwise the same sums.
__global__ void peer_allreduce(PeerView pv, double* g, int count, unsigned seq, int* err) {
  const int lane = threadIdx.x;
  bool good = true;
  const double acc = peer_wave_sum(pv, lane < 2 * count ? g[lane >> 1] : 0.0, 2 * count, 0, seq, &good);
  if (lane < 2 * count && (lane & 1) == 0) g[lane >> 1] = acc;
  if (!good && lane == 0) *err = 1;
}

// ---- peer transport: halo rows.  Block 0 writes my top row into the upper neighbour's mailbox (the row BELOW its slab, side 0),
// block 1 my bottom row into the lower neighbour's (the row ABOVE its slab, side 1); a system-scope release store of the
// sequence number follows the data.  Then block 0 waits for the row below my slab, block 1 for the row above it, and copies it
// to the halo row.  Every rank pushes before it waits: no ordering between ranks is needed.
__global__ __launch_bounds__(kBlock) void peer_exchange_rows(PeerView pv, const double* bottom_row, const double* top_row,
                                                             double* halo_below, double* halo_above, int nx, unsigned seq, int* err) {
  const int side_out = blockIdx.x;                         // 0: to the upper neighbour, 1: to the lower neighbour
  const int dst = side_out == 0 ? pv.upper : pv.lower;
  const int par = seq & 1;
  if (dst >= 0) {
    const double* src = side_out == 0 ? top_row : bottom_row;
    peer_u64* row = reinterpret_cast<peer_u64*>(pv.mbox[dst] + PeerLayout::ex_row(par, side_out, pv.row_cap));
    for (int i = threadIdx.x; i < nx; i += kBlock) peer_store(row + i, (peer_u64)__double_as_longlong(src[i]));
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0)
      __hip_atomic_store(reinterpret_cast<peer_u64*>(pv.mbox[dst] + PeerLayout::ex_flag(par, side_out)), (peer_u64)seq, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const int side_in = blockIdx.x;                          // 0: the row below my slab (from the lower neighbour), 1: the row above
  const int from = side_in == 0 ? pv.lower : pv.upper;
  if (from < 0) return;
  __shared__ int ok_s;
  if (threadIdx.x == 0) {
    const peer_u64* flag = reinterpret_cast<const peer_u64*>(pv.mbox[pv.rank] + PeerLayout::ex_flag(par, side_in));
    unsigned spins = 0;
    int ok = 1;
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != (peer_u64)seq) {
      if (++spins > kPeerSpinLimit) { ok = 0; *err = 1; break; }
      __builtin_amdgcn_s_sleep(2);
    }
    ok_s = ok;
  }
  __syncthreads();
  if (!ok_s) return;
  const peer_u64* row = reinterpret_cast<const peer_u64*>(pv.mbox[pv.rank] + PeerLayout::ex_row(par, side_in, pv.row_cap));
  double* halo = side_in == 0 ? halo_below : halo_above;
  for (int i = threadIdx.x; i < nx; i += kBlock) halo[i] = __longlong_as_double((long long)peer_load(row + i));
}

// ---- peer transport: all-gather of `count` doubles per rank (count * world <= kGatherCells).  Every rank writes its chunk as tagged
// words {32 payload bits | epoch} into the gather area of EVERY rank's mailbox (its own included), then polls its own area and copies
// out in rank order.  No flag and no fence: a word that carries the epoch is complete by itself.  The area alternates between two
// halves by the parity of the gather's own sequence number: gather n + 2 reuses the half of gather n, and a rank starts it only after
// it finished n + 1, for which every rank had to contribute - which a rank does only after it copied out of n.
__global__ __launch_bounds__(kBlock) void peer_allgather(PeerView pv, size_t area, const double* __restrict__ src, double* __restrict__ dst, int count,
                                                         unsigned seq, int* err) {
  const size_t base = area + (size_t)(seq & 1) * PeerLayout::kGatherParityBytes;
  const int tid = blockIdx.x * kBlock + threadIdx.x, nt = gridDim.x * kBlock;
  for (int w = tid; w < 2 * count; w += nt) {
    const peer_u64 word = peer_tagged(src[w >> 1], w & 1, seq);
    for (int p = 0; p < pv.world; ++p) peer_store(reinterpret_cast<peer_u64*>(pv.mbox[p] + base) + (size_t)pv.rank * 2 * count + w, word);
  }
  const peer_u64* mine = reinterpret_cast<const peer_u64*>(pv.mbox[pv.rank] + base);
  const int total = count * pv.world;
  for (int i = tid; i < total; i += nt) {
    peer_u64 lo = 0, hi = 0;
    unsigned spins = 0;
    while (true) {
      lo = peer_load(mine + 2 * (size_t)i); hi = peer_load(mine + 2 * (size_t)i + 1);
      if ((unsigned)(lo & 0xffffffffull) == seq && (unsigned)(hi & 0xffffffffull) == seq) break;
      if (++spins > kPeerSpinLimit) { *err = 1; return; }
      __builtin_amdgcn_s_sleep(2);
    }
    dst[i] = peer_untag(lo, hi);
  }
}

// ... and of `count` floats per rank: a float is one tagged word {payload | epoch}; source r's chunk starts at word r count of the
// parity's half.  The same epochs and halves as peer_allgather (one sequence over both).
__global__ __launch_bounds__(kBlock) void peer_allgather_f32(PeerView pv, size_t area, const float* __restrict__ src, float* __restrict__ dst, int count,
                                                             unsigned seq, int* err) {
  const size_t base = area + (size_t)(seq & 1) * PeerLayout::kGatherParityBytes;
  const int tid = blockIdx.x * kBlock + threadIdx.x, nt = gridDim.x * kBlock;
  for (int w = tid; w < count; w += nt) {
    const peer_u64 word = ((peer_u64)__float_as_uint(src[w]) << 32) | seq;
    for (int p = 0; p < pv.world; ++p) peer_store(reinterpret_cast<peer_u64*>(pv.mbox[p] + base) + (size_t)pv.rank * count + w, word);
  }
  const peer_u64* mine = reinterpret_cast<const peer_u64*>(pv.mbox[pv.rank] + base);
  const int total = count * pv.world;
  for (int i = tid; i < total; i += nt) {
    peer_u64 word = 0;
    unsigned spins = 0;
    while (true) {
      word = peer_load(mine + (size_t)i);
      if ((unsigned)(word & 0xffffffffull) == seq) break;
      if (++spins > kPeerSpinLimit) { *err = 1; return; }
      __builtin_amdgcn_s_sleep(2);
    }
    dst[i] = __uint_as_float((unsigned)(word >> 32));
  }
}

// ------------------------------------------------------------------------------------------------ host collectives (slab_comm.h)
// (a communicator is made by piso_comm_create or piso_comm_peer_create[_fd] only: what is not PEER is RCCL and has its ncclComm_t)
static bool is_peer(const PisoComm* pc) { return pc->transport == TRANSPORT_PEER; }
int comm_ready(const PisoComm* pc, const char* msg) {
  if (is_peer(pc) && !pc->connected) { set_error_msg(msg); return PISO_ERR_INVALID_ARG; }
  return PISO_OK;
}

int comm_allreduce_f64(PisoComm* pc, double* buf, int count, hipStream_t s) {
  if (pc->world == 1) return PISO_OK;
  if (is_peer(pc)) { peer_allreduce<<<1, 64, 0, s>>>(make_view(pc, true), buf, count, ++pc->seq_ar, pc->err); return PISO_OK; }
  PISO_NCCL_CHECK(g_rccl.AllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, pc->comm, s));
  return PISO_OK;
}
int comm_allreduce_i32(PisoComm* pc, int* buf, int count, hipStream_t s) {
  PISO_NCCL_CHECK(g_rccl.AllReduce(buf, buf, (size_t)count, ncclInt32, ncclSum, pc->comm, s));
  return PISO_OK;
}
int comm_allgather_f64(PisoComm* pc, const double* src, double* dst, size_t count, hipStream_t s) {
  if (is_peer(pc)) {
    if (count * (size_t)pc->world > (size_t)kGatherCells) { set_error_msg("peer transport: an all-gather carries at most 8192 doubles over all ranks"); return PISO_ERR_INVALID_ARG; }
    if (count == 0) return PISO_OK;
    if (pc->world == 1 && opt(OPT_SLAB_FORCE) <= 0) {
      if (src != dst) PISO_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToDevice, s));
      return PISO_OK;
    }
    const int grid = (int)((2 * count + kBlock - 1) / kBlock);
    peer_allgather<<<grid < 32 ? grid : 32, kBlock, 0, s>>>(make_view(pc, true), PeerLayout::gather_area(pc->row_cap), src, dst, (int)count, ++pc->seq_ga, pc->err);
    return PISO_OK;
  }
  PISO_NCCL_CHECK(g_rccl.AllGather(src, dst, count, ncclDouble, pc->comm, s));
  return PISO_OK;
}
int comm_exchange_rows(PisoComm* pc, bool periodic_y, double* row0, int nx, int ny, hipStream_t s) {
  double *top = row0 + (size_t)(ny - 1) * nx, *below = row0 - nx, *above = row0 + (size_t)ny * nx;
  const PeerView pv = make_view(pc, periodic_y);           // (RCCL: for the two neighbours)
  if (is_peer(pc)) {
    if (nx > (int)pc->row_cap) { set_error_msg("peer transport: row longer than the mailbox rows"); return PISO_ERR_INVALID_ARG; }
    peer_exchange_rows<<<2, kBlock, 0, s>>>(pv, row0, top, below, above, nx, ++pc->seq_ex, pc->err);
    return PISO_OK;
  }
  const int lo = pv.lower, hi = pv.upper;                  // (the UPWARD transfer first, then the DOWNWARD one: slab_comm.h)
  constexpr ncclDataType_t dt = ncclDouble;
  PISO_NCCL_CHECK(g_rccl.GroupStart());
  if (hi >= 0) PISO_NCCL_CHECK(g_rccl.Send(top, nx, dt, hi, pc->comm, s));        // my top row -> upper's lower halo
  if (lo >= 0) PISO_NCCL_CHECK(g_rccl.Recv(below, nx, dt, lo, pc->comm, s));      // lower's top row -> my lower halo
  if (lo >= 0) PISO_NCCL_CHECK(g_rccl.Send(row0, nx, dt, lo, pc->comm, s));       // my bottom row -> lower's upper halo
  if (hi >= 0) PISO_NCCL_CHECK(g_rccl.Recv(above, nx, dt, hi, pc->comm, s));      // upper's bottom row -> my upper halo
  PISO_NCCL_CHECK(g_rccl.GroupEnd());
  return PISO_OK;
}

int comm_allgather_f32(PisoComm* pc, const float* src, float* dst, size_t count, hipStream_t s) {
  if (is_peer(pc)) {
    if (count * (size_t)pc->world > (size_t)kGatherCells) { set_error_msg("peer transport: an all-gather carries at most 8192 floats over all ranks"); return PISO_ERR_INVALID_ARG; }
    if (count == 0) return PISO_OK;
    if (pc->world == 1 && opt(OPT_SLAB_FORCE) <= 0) {
      if (src != dst) PISO_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, s));
      return PISO_OK;
    }
    const int grid = (int)((count + kBlock - 1) / kBlock);
    peer_allgather_f32<<<grid < 32 ? grid : 32, kBlock, 0, s>>>(make_view(pc, true), PeerLayout::gather_area(pc->row_cap), src, dst, (int)count, ++pc->seq_ga, pc->err);
    return PISO_OK;
  }
  PISO_NCCL_CHECK(g_rccl.AllGather(src, dst, count, ncclFloat, pc->comm, s));
  return PISO_OK;
}
int comm_exchange_rows_f32(PisoComm* pc, bool periodic_y, float* row0, int nx, int ny, hipStream_t s) {
  float *top = row0 + (size_t)(ny - 1) * nx, *below = row0 - nx, *above = row0 + (size_t)ny * nx;
  const PeerView pv = make_view(pc, periodic_y);
  if (is_peer(pc)) {
    if (nx > (int)pc->row_cap) { set_error_msg("peer transport: row longer than the mailbox rows"); return PISO_ERR_INVALID_ARG; }
    // the four messages of a row exchange, as element offsets from the halo row below: {to upper, to lower, from lower, from upper}.
    // The floats travel as their 32 bits (the int instance: int -> double -> int is exact, so every bit pattern arrives unchanged)
    const HaloMsg up{1, {ny * nx, 0, 0}, {nx, 0, 0}}, down{1, {nx, 0, 0}, {nx, 0, 0}}, from_lo{1, {0, 0, 0}, {nx, 0, 0}}, from_hi{1, {(ny + 1) * nx, 0, 0}, {nx, 0, 0}};
    peer_exchange_segments<int><<<2, 256, 0, s>>>(pv, reinterpret_cast<int*>(below), up, down, from_lo, from_hi, ++pc->seq_ex, pc->err);
    return PISO_OK;
  }
  const int lo = pv.lower, hi = pv.upper;                  // (the UPWARD transfer first, then the DOWNWARD one: slab_comm.h)
  constexpr ncclDataType_t dt = ncclFloat;
  PISO_NCCL_CHECK(g_rccl.GroupStart());
  if (hi >= 0) PISO_NCCL_CHECK(g_rccl.Send(top, nx, dt, hi, pc->comm, s));
  if (lo >= 0) PISO_NCCL_CHECK(g_rccl.Recv(below, nx, dt, lo, pc->comm, s));
  if (lo >= 0) PISO_NCCL_CHECK(g_rccl.Send(row0, nx, dt, lo, pc->comm, s));
  if (hi >= 0) PISO_NCCL_CHECK(g_rccl.Recv(above, nx, dt, hi, pc->comm, s));
  PISO_NCCL_CHECK(g_rccl.GroupEnd());
  return PISO_OK;
}

int comm_exchange_segments(PisoComm* pc, void* vec, int dtype, const HaloMsg* m, hipStream_t s) {
  const PeerView pv = make_view(pc, true);                 // always a ring
  if (is_peer(pc)) {
    const unsigned seq = ++pc->seq_ex;
    if (dtype == 0) peer_exchange_segments<float><<<2, 256, 0, s>>>(pv, static_cast<float*>(vec), m[0], m[1], m[2], m[3], seq, pc->err);
    else if (dtype == 1) peer_exchange_segments<double><<<2, 256, 0, s>>>(pv, static_cast<double*>(vec), m[0], m[1], m[2], m[3], seq, pc->err);
    else peer_exchange_segments<int><<<2, 256, 0, s>>>(pv, static_cast<int*>(vec), m[0], m[1], m[2], m[3], seq, pc->err);
    PISO_LAUNCH_CHECK();
    return PISO_OK;
  }
  const int lo = pv.lower, hi = pv.upper;
  const ncclDataType_t dt = dtype == 0 ? ncclFloat : (dtype == 1 ? ncclDouble : ncclInt32);
  const size_t es = dtype == 1 ? 8 : 4;
  char* base = static_cast<char*>(vec);
  PISO_NCCL_CHECK(g_rccl.GroupStart());
  for (int q = 0; q < m[0].count; ++q) PISO_NCCL_CHECK(g_rccl.Send(base + (size_t)m[0].off[q] * es, (size_t)m[0].len[q], dt, hi, pc->comm, s));
  for (int q = 0; q < m[2].count; ++q) PISO_NCCL_CHECK(g_rccl.Recv(base + (size_t)m[2].off[q] * es, (size_t)m[2].len[q], dt, lo, pc->comm, s));
  for (int q = 0; q < m[1].count; ++q) PISO_NCCL_CHECK(g_rccl.Send(base + (size_t)m[1].off[q] * es, (size_t)m[1].len[q], dt, lo, pc->comm, s));
  for (int q = 0; q < m[3].count; ++q) PISO_NCCL_CHECK(g_rccl.Recv(base + (size_t)m[3].off[q] * es, (size_t)m[3].len[q], dt, hi, pc->comm, s));
  PISO_NCCL_CHECK(g_rccl.GroupEnd());
  return PISO_OK;
}

int comm_agree(PisoComm* pc, const char* who, hipStream_t s, bool ring_of_one) {
  int herr = 0;
  if (is_peer(pc)) {
    if (pc->world > 1 || ring_of_one) peer_agree_on_error<><<<1, 64, 0, s>>>(make_view(pc, true), pc->err, ++pc->seq_ar);
    PISO_HIP_CHECK(hipMemcpyAsync(&herr, pc->err, sizeof(int), hipMemcpyDeviceToHost, s));
  }
  PISO_HIP_CHECK(hipStreamSynchronize(s));
  if (herr) {
    PISO_HIP_CHECK(hipMemsetAsync(pc->err, 0, sizeof(int), s));
    return fail(PISO_ERR_HIP, who, "a wait on a peer's mailbox gave up (peer process gone or not running?)");
  }
  return PISO_OK;
}

}  // namespace piso

using namespace piso;

extern "C" {

int piso_comm_unique_id(void* id128) {
  PISO_TRY(load_rccl());
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  PISO_NCCL_CHECK(g_rccl.GetUniqueId(static_cast<ncclUniqueId*>(id128)));
  return PISO_OK;
}

int piso_comm_create(const void* id128, int rank, int world, void** comm_out) {
  PISO_TRY(load_rccl());
  if (!id128 || !comm_out || world < 1 || rank < 0 || rank >= world) { set_error_msg("piso_comm_create: invalid argument"); return PISO_ERR_INVALID_ARG; }
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  PisoComm* c = new PisoComm;
  c->rank = rank; c->world = world; c->transport = TRANSPORT_RCCL;
  ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) { set_error_msg(g_rccl.GetErrorString(r)); delete c; return PISO_ERR_HIP; }
  *comm_out = c;
  return PISO_OK;
}

int piso_comm_destroy(void* comm) {
  if (!comm) return PISO_OK;
  PisoComm* c = static_cast<PisoComm*>(comm);
  if (c->transport == TRANSPORT_RCCL) {
    if (g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  } else {
    (void)hipDeviceSynchronize();
    if (c->vmm) {
      for (int r = 0; r < c->world; ++r) {
        if (!c->mbox[r]) continue;
        (void)hipMemUnmap(c->mbox[r], c->vmm_bytes);
        (void)hipMemAddressFree(c->mbox[r], c->vmm_bytes);
        if (c->vmm_handle[r]) (void)hipMemRelease(c->vmm_handle[r]);
      }
    } else {
      for (int r = 0; r < c->world; ++r)
        if (r != c->rank && c->mbox[r]) (void)hipIpcCloseMemHandle(c->mbox[r]);
      if (c->mbox[c->rank]) (void)hipFree(c->mbox[c->rank]);
    }
    if (c->err) (void)hipFree(c->err);
  }
  delete c;
  return PISO_OK;
}

// ---- peer transport: create my mailbox (step 1), exchange the 64-byte handles by any means, connect (step 2).
// What the two ways of sharing a mailbox have in common: the communicator before its mailbox exists ...
static PisoComm* peer_new(const char* who, bool outputs, int rank, int world, int row_capacity, int vmm) {
  const bool ok = outputs && world >= 1 && world <= kMaxRanks && rank >= 0 && rank < world && row_capacity >= 1;
  if (!ok) { (void)fail(PISO_ERR_INVALID_ARG, who, "invalid argument (at most 8 ranks: the GPUs of one node)"); return nullptr; }
  PisoComm* c = new PisoComm;
  c->rank = rank; c->world = world; c->transport = TRANSPORT_PEER; c->vmm = vmm;
  c->row_cap = align_up((size_t)row_capacity, 32);
  c->mbox_bytes = PeerLayout::bytes(c->row_cap);
  return c;
}
// ... and once it is mapped at mbox[rank]: zeroed, with a zeroed error flag, ready to be exported
static hipError_t peer_mailbox_ready(PisoComm* c) {
  hipError_t e = hipMemset(c->mbox[c->rank], 0, c->mbox_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->err), sizeof(int));
  if (e == hipSuccess) e = hipMemset(c->err, 0, sizeof(int));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  c->connected = (c->world == 1);
  return e;
}

int piso_comm_peer_create(int rank, int world, int row_capacity, void** comm_out, void* ipc_handle64_out) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  PisoComm* c = peer_new("piso_comm_peer_create", comm_out && ipc_handle64_out, rank, world, row_capacity, 0);
  if (!c) return PISO_ERR_INVALID_ARG;
  void* mb = nullptr;
  // uncached + fine-grained: a peer's write over xGMI is visible to my system-scope loads without any cache maintenance
  hipError_t e = hipExtMallocWithFlags(&mb, c->mbox_bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) { set_error("hipExtMallocWithFlags(mailbox)", e); delete c; return PISO_ERR_HIP; }
  c->mbox[rank] = static_cast<char*>(mb);
  e = peer_mailbox_ready(c);
  if (e == hipSuccess) e = hipIpcGetMemHandle(static_cast<hipIpcMemHandle_t*>(ipc_handle64_out), mb);
  if (e != hipSuccess) { set_error("piso_comm_peer_create", e); (void)hipFree(mb); if (c->err) (void)hipFree(c->err); delete c; return PISO_ERR_HIP; }
  *comm_out = c;
  return PISO_OK;
}

int piso_comm_peer_connect(void* comm, const void* ipc_handles64_all_ranks) {
  PisoComm* c = static_cast<PisoComm*>(comm);
  if (!c || c->transport != TRANSPORT_PEER || !ipc_handles64_all_ranks) { set_error_msg("piso_comm_peer_connect: invalid argument"); return PISO_ERR_INVALID_ARG; }
  const char* h = static_cast<const char*>(ipc_handles64_all_ranks);
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank || c->mbox[r]) continue;
    hipIpcMemHandle_t handle;
    memcpy(&handle, h + (size_t)r * 64, 64);
    void* p = nullptr;
    PISO_HIP_CHECK(hipIpcOpenMemHandle(&p, handle, hipIpcMemLazyEnablePeerAccess));
    c->mbox[r] = static_cast<char*>(p);
  }
  c->connected = true;
  return PISO_OK;
}

// ---- the same mailboxes through the virtual-memory API, for nodes whose driver refuses hipIpcGetMemHandle across ranks: the allocation
// is created exportable (hipMemCreate, uncached type), exported as a POSIX file descriptor, handed to the other ranks by the caller
// (a Unix socket with SCM_RIGHTS: diffpiso/distributed.py) and imported + mapped there.  Everything else of the transport is unchanged.
static int vmm_map(PisoComm* c, int r, hipMemGenericAllocationHandle_t h, int dev) {
  void* p = nullptr;
  hipError_t e = hipMemAddressReserve(&p, c->vmm_bytes, 0, nullptr, 0);
  if (e != hipSuccess) { set_error("hipMemAddressReserve(mailbox)", e); return PISO_ERR_HIP; }
  e = hipMemMap(p, c->vmm_bytes, 0, h, 0);
  if (e != hipSuccess) { set_error("hipMemMap(mailbox)", e); (void)hipMemAddressFree(p, c->vmm_bytes); return PISO_ERR_HIP; }
  hipMemAccessDesc acc{};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = dev;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  e = hipMemSetAccess(p, c->vmm_bytes, &acc, 1);
  if (e != hipSuccess) { set_error("hipMemSetAccess(mailbox)", e); (void)hipMemUnmap(p, c->vmm_bytes); (void)hipMemAddressFree(p, c->vmm_bytes); return PISO_ERR_HIP; }
  c->mbox[r] = static_cast<char*>(p);
  c->vmm_handle[r] = h;
  return PISO_OK;
}

int piso_comm_peer_create_fd(int rank, int world, int row_capacity, void** comm_out, int* fd_out) {
  PisoComm* c = peer_new("piso_comm_peer_create_fd", comm_out && fd_out, rank, world, row_capacity, 1);
  if (!c) return PISO_ERR_INVALID_ARG;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) { set_error("hipGetDevice(&dev)", e); delete c; return PISO_ERR_HIP; }
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypeUncached;               // (as hipDeviceMallocUncached: a peer's write is visible to my system-scope loads)
  prop.requestedHandleType = hipMemHandleTypePosixFileDescriptor;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = dev;
  size_t gran = 0;
  e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
  if (e != hipSuccess || gran == 0) { set_error("hipMemGetAllocationGranularity(mailbox)", e); delete c; return PISO_ERR_HIP; }
  c->vmm_bytes = align_up(c->mbox_bytes, gran);
  hipMemGenericAllocationHandle_t h{};
  e = hipMemCreate(&h, c->vmm_bytes, &prop, 0);
  if (e != hipSuccess) { set_error("hipMemCreate(mailbox, uncached, exportable)", e); delete c; return PISO_ERR_HIP; }
  int rc = vmm_map(c, rank, h, dev);
  if (rc != PISO_OK) { (void)hipMemRelease(h); delete c; return rc; }
  int fd = -1;
  e = peer_mailbox_ready(c);
  if (e == hipSuccess) e = hipMemExportToShareableHandle(&fd, h, hipMemHandleTypePosixFileDescriptor, 0);
  if (e != hipSuccess) { set_error("piso_comm_peer_create_fd", e); (void)piso_comm_destroy(c); return PISO_ERR_HIP; }
  *fd_out = fd;                                           // the caller closes it once every peer has received its copy
  *comm_out = c;
  return PISO_OK;
}

int piso_comm_peer_connect_fd(void* comm, const int* fds_all_ranks) {
  PisoComm* c = static_cast<PisoComm*>(comm);
  if (!c || c->transport != TRANSPORT_PEER || !c->vmm || !fds_all_ranks) { set_error_msg("piso_comm_peer_connect_fd: invalid argument"); return PISO_ERR_INVALID_ARG; }
  int dev = 0;
  PISO_HIP_CHECK(hipGetDevice(&dev));
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank || c->mbox[r]) continue;
    hipMemGenericAllocationHandle_t h{};
    // (this runtime reads the descriptor THROUGH the pointer - handing the integer over as the pointer's value, as the CUDA driver API
    // takes it, makes it dereference address `fd`)
    int fd = fds_all_ranks[r];
    hipError_t e = hipMemImportFromShareableHandle(&h, static_cast<void*>(&fd), hipMemHandleTypePosixFileDescriptor);
    if (e != hipSuccess) { set_error("hipMemImportFromShareableHandle(mailbox)", e); return PISO_ERR_HIP; }
    const int rc = vmm_map(c, r, h, dev);
    if (rc != PISO_OK) { (void)hipMemRelease(h); return rc; }
  }
  c->connected = true;
  return PISO_OK;
}

// Round-trip time of one tagged word between ranks a and b through the mailboxes (`iters` round trips; a == b: a rank's own mailbox).
// EVERY rank calls it with the same arguments; ranks other than a and b return at once.  us_out (host float, written on rank a only):
// microseconds per round trip, timed with events around the initiator's kernel; the one-way hop is half of it.
int piso_comm_pingpong(void* comm, int a, int b, int iters, float* us_out, piso_stream_t stream_) {
  PisoComm* pc = static_cast<PisoComm*>(comm);
  if (!pc || pc->transport != TRANSPORT_PEER || !pc->connected || a < 0 || b < 0 || a >= pc->world || b >= pc->world || iters < 1) {
    set_error_msg("piso_comm_pingpong: needs a connected peer communicator and two of its ranks");
    return PISO_ERR_INVALID_ARG;
  }
  const unsigned seq0 = pc->seq_pp + 1;
  pc->seq_pp += (unsigned)iters + 1;                      // (advances identically on every rank: all of them make every call)
  if (pc->rank != a && pc->rank != b) return PISO_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const PeerView pv = make_view(pc, true);
  hipEvent_t e0, e1;
  PISO_HIP_CHECK(hipEventCreate(&e0));
  PISO_HIP_CHECK(hipEventCreate(&e1));
  PISO_HIP_CHECK(hipEventRecord(e0, stream));
  peer_pingpong<<<1, 64, 0, stream>>>(pv, a, b, iters, seq0, pc->err);
  PISO_HIP_CHECK(hipEventRecord(e1, stream));
  PISO_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0;
  PISO_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (us_out && pc->rank == a) *us_out = 1e3f * ms / (float)iters;
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

// what the communicator did so far: [0] transport (1 RCCL, 2 peer mailboxes), [1] CG iterations executed inside persistent slab
// segments, [2] solves restarted on the two-kernel iteration after a segment failed, [3] persistent launches
int piso_comm_stats(void* comm, long long* out4) {      // (six values: see include/piso_hip.h)
  PisoComm* c = static_cast<PisoComm*>(comm);
  if (!c || !out4) { set_error_msg("piso_comm_stats: invalid argument"); return PISO_ERR_INVALID_ARG; }
  out4[0] = c->transport; out4[1] = c->persist_iterations; out4[2] = c->persist_fallbacks; out4[3] = c->launches;
  out4[4] = c->verify_runs; out4[5] = c->verify_failures;
  return PISO_OK;
}

// Halo rows of ANY globally indexed vector of the slab-decomposed step (faces, cells, CSR values): four messages of up to three
// element segments each, in the order {to the upper neighbour, to the lower neighbour, from the lower, from the upper};
// msgs28 = 4 x {count, off[3], len[3]} (element offsets into `vec`).  Ring neighbours always (without a periodic y axis the wrap
// rows travel and nobody reads them).  One launch; the elements cross xGMI as 8-byte words written into the consumer's mailbox.
int piso_comm_exchange(void* comm, void* vec, int dtype, const int* msgs28, piso_stream_t stream_) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  PisoComm* pc = static_cast<PisoComm*>(comm);
  if (!pc || !vec || !msgs28) { set_error_msg("piso_comm_exchange: invalid argument"); return PISO_ERR_INVALID_ARG; }
  if (pc->world == 1 && opt(OPT_SLAB_FORCE) <= 0) return PISO_OK;        // (slab_force: test knob - a ring of one rank exchanges with itself)
  PISO_TRY(comm_ready(pc, "piso_comm_exchange: the peer communicator is not connected"));
  HaloMsg m[4];
  for (int q = 0; q < 4; ++q) {
    m[q].count = msgs28[7 * q];
    size_t total = 0;
    if (m[q].count < 0 || m[q].count > 3) { set_error_msg("piso_comm_exchange: at most three segments per message"); return PISO_ERR_INVALID_ARG; }
    for (int k = 0; k < 3; ++k) {
      m[q].off[k] = msgs28[7 * q + 1 + k]; m[q].len[k] = msgs28[7 * q + 4 + k];
      if (k < m[q].count) { if (m[q].off[k] < 0 || m[q].len[k] < 0) { set_error_msg("piso_comm_exchange: negative segment"); return PISO_ERR_INVALID_ARG; } total += (size_t)m[q].len[k]; }
    }
    if (pc->transport == TRANSPORT_PEER && total > pc->row_cap) { set_error_msg("piso_comm_exchange: message longer than the communicator's row_capacity"); return PISO_ERR_INVALID_ARG; }
  }
  if (dtype < 0 || dtype > 2) { set_error_msg("piso_comm_exchange: dtype must be 0 (float), 1 (double) or 2 (int32)"); return PISO_ERR_INVALID_ARG; }
  return comm_exchange_segments(pc, vec, dtype, m, static_cast<hipStream_t>(stream_));
}
// All-gather of `count` doubles per rank in rank order: dst [count * world] on every rank (both transports; peer: count * world <= 8192,
// and one rank copies unless the option slab_force sends the chunk through its own mailbox).  Queued on the stream.
int piso_comm_allgather_f64(void* comm, const void* src, void* dst, int count, piso_stream_t stream_) {
  const piso::OptScope knobs;
  PisoComm* pc = static_cast<PisoComm*>(comm);
  if (!pc || !src || !dst || count < 0) { set_error_msg("piso_comm_allgather_f64: invalid argument"); return PISO_ERR_INVALID_ARG; }
  PISO_TRY(comm_ready(pc, "piso_comm_allgather_f64: the peer communicator is not connected"));
  PISO_TRY(comm_allgather_f64(pc, static_cast<const double*>(src), static_cast<double*>(dst), (size_t)count, static_cast<hipStream_t>(stream_)));
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
// ... and of `count` floats per rank (the float rows of the float32 multigrid cycle; peer: count * world <= 8192)
int piso_comm_allgather_f32(void* comm, const void* src, void* dst, int count, piso_stream_t stream_) {
  const piso::OptScope knobs;
  PisoComm* pc = static_cast<PisoComm*>(comm);
  if (!pc || !src || !dst || count < 0) { set_error_msg("piso_comm_allgather_f32: invalid argument"); return PISO_ERR_INVALID_ARG; }
  PISO_TRY(comm_ready(pc, "piso_comm_allgather_f32: the peer communicator is not connected"));
  PISO_TRY(comm_allgather_f32(pc, static_cast<const float*>(src), static_cast<float*>(dst), (size_t)count, static_cast<hipStream_t>(stream_)));
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
// did any wait on a peer give up since the last call?  (agreed over the ranks; synchronises the stream)
int piso_comm_check(void* comm, piso_stream_t stream_) {
  PisoComm* pc = static_cast<PisoComm*>(comm);
  if (!pc) { set_error_msg("piso_comm_check: NULL communicator"); return PISO_ERR_INVALID_ARG; }
  if (pc->transport != TRANSPORT_PEER || pc->world == 1) return PISO_OK;
  return comm_agree(pc, "piso_comm_check", static_cast<hipStream_t>(stream_));
}

}  // extern "C"
