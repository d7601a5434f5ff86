// The communicator of the slab-decomposed solvers and the sharded step: RCCL or peer-mapped mailboxes (peer.h).  Interface of comm.hip.
#pragma once
#include <rccl/rccl.h>

#include "peer.h"

namespace piso {

enum { TRANSPORT_RCCL = 1, TRANSPORT_PEER = 2 };
struct PisoComm {
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  int transport = TRANSPORT_RCCL;
  // peer transport
  char* mbox[kMaxRanks] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool connected = false;
  size_t row_cap = 0, mbox_bytes = 0;
  // how the mailboxes were mapped: 0 = hipIpc handles (piso_comm_peer_create), 1 = virtual-memory allocations shared as POSIX file
  // descriptors (piso_comm_peer_create_fd: hipMemCreate / hipMemExportToShareableHandle / hipMemImportFromShareableHandle)
  int vmm = 0;
  hipMemGenericAllocationHandle_t vmm_handle[kMaxRanks] = {};
  size_t vmm_bytes = 0;
  unsigned seq_pp = 0;                // ping-pong tags (piso_comm_pingpong)
  unsigned seq_ar = 0, seq_ex = 0;    // sequence numbers of the host-level collectives (advance identically on every rank)
  unsigned seq_ga = 0;                // epochs of the peer all-gather: a sequence of its own, so two consecutive gathers never share a slot
  unsigned launches = 0;              // persistent slab launches so far: the high half of their exchange tags
  int* err = nullptr;                 // device flag: a wait on a peer gave up
  int persist_fallbacks = 0;          // solves restarted on the two-kernel iteration after a persistent segment failed
  long long persist_iterations = 0;   // CG iterations executed inside persistent slab segments
  long long verify_runs = 0;          // slab solves checked against the true residual after persistent segments ...
  int verify_failures = 0;            // ... and found wanting on some rank: restarted on the two-kernel iteration
};

inline PeerView make_view(const PisoComm* pc, bool periodic_y) {
  PeerView v;
  for (int r = 0; r < kMaxRanks; ++r) v.mbox[r] = pc->mbox[r];
  v.rank = pc->rank; v.world = pc->world; v.row_cap = pc->row_cap;
  v.lower = (pc->rank > 0) ? pc->rank - 1 : (periodic_y ? pc->world - 1 : -1);
  v.upper = (pc->rank < pc->world - 1) ? pc->rank + 1 : (periodic_y ? 0 : -1);
  return v;
}

// The host collectives (comm.hip): each is the only place that chooses a transport for its job, and queues it on stream `s`.
//   * in-place sum of `count` doubles over the ranks (one rank: nothing); of ints: RCCL only;
//   * the all-gather of `count` doubles per rank, in rank order.  Peer transport: count * world <= kGatherCells, every rank writes its
//     chunk as tagged words into every rank's gather area (its own included), polls its own and copies out; one rank: a copy, unless
//     the option slab_force sends it through the mailbox;
//   * the halo rows -1 and ny of a slab vector whose owned rows start at `row0` (nx doubles a row; neighbours by periodic_y);
//   * the four halo messages of a globally indexed vector {to upper, to lower, from lower, from upper}, always around the ring.
//     RCCL: grouped send / recv of the segments, straight from / into the vector (no staging).  Sends and receives between one pair
//     of ranks are matched in issue order, and with one or two ranks the lower and the upper neighbour are the same peer: every rank
//     issues "to upper" before "to lower" and "from lower" before "from upper" (the rows likewise).  dtype: 0 float, 1 double, 2 int32;
//   * comm_agree: every rank returns the same status.  Peer transport with more than one rank (ring_of_one: or a caller whose sums go
//     through the mailbox even then): the error flags are summed over the ranks (peer.h).  Synchronises the stream; a set flag is
//     cleared and fails the call with "<who>: a wait on a peer's mailbox gave up ...".  comm_ready: not connected yet, refused with `msg`.
int comm_allreduce_f64(PisoComm* pc, double* buf, int count, hipStream_t s);
int comm_allreduce_i32(PisoComm* pc, int* buf, int count, hipStream_t s);
int comm_allgather_f64(PisoComm* pc, const double* src, double* dst, size_t count, hipStream_t s);
int comm_exchange_rows(PisoComm* pc, bool periodic_y, double* row0, int nx, int ny, hipStream_t s);
int comm_exchange_segments(PisoComm* pc, void* vec, int dtype, const HaloMsg* m4, hipStream_t s);
// The float rows of the float32 multigrid cycle (mg_slab_f32.h).  Peer transport: a halo row travels in the row slots of the f64 exchange,
// the 32 bits of a float per 8-byte word (the int instance of the segment messages' kernel; nx <= row_cap), and a float of the gather is ONE tagged word of the gather
// area {32 payload bits | epoch} (count * world <= kGatherCells); both share the sequence numbers of their f64 twins.  RCCL: ncclFloat.
int comm_allgather_f32(PisoComm* pc, const float* src, float* dst, size_t count, hipStream_t s);
int comm_exchange_rows_f32(PisoComm* pc, bool periodic_y, float* row0, int nx, int ny, hipStream_t s);
int comm_agree(PisoComm* pc, const char* who, hipStream_t s, bool ring_of_one = false);
int comm_ready(const PisoComm* pc, const char* msg);

}  // namespace piso
