// What the step driver (sharded_step.hip) uses of its communicator (step_comm.hip): mia_comm itself, its events, the all-gather, the
// placement of a gathered piece and the two halves of the direct peer exchange.  Internal to the library (hidden symbols).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mia_letkf.h"

// ---- the few RCCL declarations needed (ABI of rccl.h 2.x: opaque comm, 128-byte id, C enums)
typedef struct ncclComm* ncclComm_t;

namespace mia {
constexpr int kMaxChunks = 16;   // pieces per block; events: [c] piece c, [kMaxChunks-1] records packed (pieces <= 15)
constexpr int kMaxRanks = 16, kMaxSlots = 8;     // direct exchange: ranks of one node, steps in flight
}  // namespace mia


struct mia_comm {
  int rank = 0, world = 1;
  ncclComm_t nccl = nullptr;
  mia_allgather_fn ag = nullptr;
  mia_allreduce_max_i32_fn ar = nullptr;
  void* ctx = nullptr;
  hipEvent_t ev[mia::kMaxChunks + 2] = {};
  hipEvent_t evp[mia::kMaxChunks] = {};      // piece c gathered (exchange stream -> placement stream)
  hipStream_t place_stream = nullptr;   // optional: mia_comm_set_place_stream
  int n_ev = 0;
  // ---- direct (peer-mapped) exchange, see "Direct exchange" in step_comm.hip
  int peer_slots = 0;                    // result buffers this rank owns (one per step in flight)
  size_t peer_bytes = 0;                 // bytes of one result buffer
  float* peer_buf[mia::kMaxRanks][mia::kMaxSlots] = {};   // [rank][slot]: rank's result buffers as mapped into this process
  uint32_t* peer_sync[mia::kMaxRanks] = {};   // [rank]: its synchronisation area (fine-grained device memory)
  bool peer_owned = false;               // buffers of `rank` were allocated by mia_comm_peer_alloc (freed on destroy)
  bool peer_opened[mia::kMaxRanks] = {};      // mapped through hipIpcOpenMemHandle (closed on destroy)
  int peer_ready = 0;                    // every rank attached
  uint32_t peer_seq[mia::kMaxSlots] = {};     // exchanges done per slot (the sequence number the flags carry)
  // bound of the device-side waits for the peers' flags, in polls of ~1-2 us (mia_comm_peer_wait_bound).  Ranks of a real run
  // drift apart by seconds (I/O of one rank between steps, a first-step table build, a debugger): the default is ~1 minute --
  // an RCCL collective would simply wait; a waiter that gives up raises error bit 2, it never hangs the grid
  int peer_wait_polls = 1 << 25;
};

#pragma GCC visibility push(hidden)
namespace mia {
int comm_events(mia_comm* c);      // creates the communicator's events on first use
int comm_allgather(mia_comm* c, const void* send, void* recv, size_t bytes, hipStream_t s);
// gathered piece [world][rows][nc] (+ the ranks' counter trailers) -> columns r * n + off + i of the (rows, G) result, on stream xs;
// ctr_out: null, or the step's eight counters (this rank's trailer and the maximum over the ranks)
int place_chunk_launch(const float* gath, float* out, int64_t G, int64_t n, int64_t off, int64_t nc, int rows, int world,
                       size_t rank_stride /* floats */, int32_t* ctr_out, int rank, hipStream_t xs);
// direct exchange: the slot whose result buffer Xa is (-1: none, or the peers are not all mapped), and its two halves
int peer_slot_of(const mia_comm* c, const float* Xa);
int peer_begin(mia_comm* c, int slot, hipStream_t ps, uint32_t* seq_out);
int peer_finish(mia_comm* c, int slot, uint32_t seq, int64_t G, int64_t b0, int64_t b1, int rows, int32_t* counters, hipStream_t cs);
}  // namespace mia
#pragma GCC visibility pop
