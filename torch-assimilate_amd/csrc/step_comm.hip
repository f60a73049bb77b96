// The communicator of the step driver (sharded_step.hip) and the direct peer exchange: the run-time binding of RCCL, mia_comm with
// its events, the all-gather / all-reduce wrappers, the placement of a gathered piece into the (m, k, G) result, the peer-mapped
// result buffers with their push / wait kernels, and every mia_comm_* entry of include/mia_letkf.h.  What the step uses of it is
// declared in mia_step_comm.h.
//
// RCCL is bound at run time (dlopen of the library the process already uses, normally torch's bundled
// librccl.so) so that this library keeps loading on machines without RCCL and never pulls in a second
// HIP runtime.
#include <dlfcn.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

#include "mia_common.h"
#include "mia_step_comm.h"

using namespace mia;

// ---- the few RCCL declarations needed (ABI of rccl.h 2.x: opaque comm, 128-byte id, C enums)
typedef struct { char internal[128]; } ncclUniqueId;
enum { kNcclSuccess = 0, kNcclInt32 = 2, kNcclFloat32 = 7, kNcclMax = 2, kNcclUint8 = 1 };
typedef int (*pfn_ncclGetUniqueId)(ncclUniqueId*);
typedef int (*pfn_ncclCommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
typedef int (*pfn_ncclCommDestroy)(ncclComm_t);
typedef int (*pfn_ncclAllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t);
typedef int (*pfn_ncclAllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t);
typedef const char* (*pfn_ncclGetErrorString)(int);

namespace {

struct RcclApi {
  void* handle = nullptr;
  pfn_ncclGetUniqueId GetUniqueId = nullptr;
  pfn_ncclCommInitRank CommInitRank = nullptr;
  pfn_ncclCommDestroy CommDestroy = nullptr;
  pfn_ncclAllGather AllGather = nullptr;
  pfn_ncclAllReduce AllReduce = nullptr;
  pfn_ncclGetErrorString GetErrorString = nullptr;
} g_rccl;

char g_comm_error[512] = "";

void set_error(const char* what, int code) {
  const char* msg = (g_rccl.GetErrorString && code > 0) ? g_rccl.GetErrorString(code) : "";
  snprintf(g_comm_error, sizeof(g_comm_error), "%s (code %d) %s", what, code, msg);
}

// synchronisation area of one rank, in uint32 words: per slot [kMaxRanks] ready, [kMaxRanks] free, [kMaxRanks][4] counters
constexpr int kSyncSlotWords = kMaxRanks * 6;
constexpr size_t kSyncBytes = (size_t)kMaxSlots * kSyncSlotWords * sizeof(uint32_t);

}  // namespace

namespace mia {

int comm_events(mia_comm* c) {
  if (c->n_ev) return MIA_OK;
  for (int i = 0; i < kMaxChunks + 2; ++i) MIA_HIP_TRY(hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming));
  for (int i = 0; i < kMaxChunks; ++i) MIA_HIP_TRY(hipEventCreateWithFlags(&c->evp[i], hipEventDisableTiming));
  c->n_ev = kMaxChunks + 2;
  return MIA_OK;
}

int comm_allgather(mia_comm* c, const void* send, void* recv, size_t bytes, hipStream_t s) {
  if (c->ag) return c->ag(c->ctx, send, recv, bytes, (void*)s) == 0 ? MIA_OK : MIA_ERR_COMM;
  int rc = g_rccl.AllGather(send, recv, bytes, kNcclUint8, c->nccl, s);
  if (rc != kNcclSuccess) { set_error("ncclAllGather failed", rc); return MIA_ERR_COMM; }
  return MIA_OK;
}

}  // namespace mia

namespace {

int comm_allreduce_max(mia_comm* c, int32_t* buf, int n, hipStream_t s) {
  if (c->ar) return c->ar(c->ctx, buf, n, (void*)s) == 0 ? MIA_OK : MIA_ERR_COMM;
  int rc = g_rccl.AllReduce(buf, buf, (size_t)n, kNcclInt32, kNcclMax, c->nccl, s);
  if (rc != kNcclSuccess) { set_error("ncclAllReduce failed", rc); return MIA_ERR_COMM; }
  return MIA_OK;
}

// gathered chunk [world][rows][nc]  ->  result rows [rows][G] at columns r * n + off + i
// (i < nc, off + i < n, column < G).  x: column (4 per thread when everything is 4-aligned), y: row, z: rank.
// Every rank's piece carries a 16-byte trailer {longest list, truncated lists, declined points, error bits};
// with ctr_out the first thread also folds the trailers: ctr_out[0..3] = this rank's, [4..7] = max over ranks
// (the all-reduce of the redo decision rides on the last piece's all-gather instead of being a collective).
// Single-wave workgroups, four column groups per lane: with steps in flight this kernel runs beside a later step's
// analysis kernel, which fills every SIMD's register file -- a lone wave takes the slot of the next analysis wave that
// retires, a 4-wave workgroup waits for one to retire on every SIMD of a CU at once (see localize.hip).
constexpr int kPlaceThreads = 64, kPlaceUnroll = 4;
template <int VEC>
__global__ void __launch_bounds__(kPlaceThreads) place_chunk_kernel(const float* __restrict__ gath, float* __restrict__ out,
                                                          int64_t G, int64_t n, int64_t off, int nc, int rows,
                                                          size_t rank_stride /* floats */, int32_t* ctr_out, int rank) {
  const int r = blockIdx.z, row = blockIdx.y;
  if (ctr_out && blockIdx.x == 0 && row == 0 && r == 0 && threadIdx.x < 4) {
    int mx = 0, own = 0;
    for (int q = 0; q < (int)gridDim.z; ++q) {
      const int v = reinterpret_cast<const int32_t*>(gath + (size_t)q * rank_stride + (size_t)rows * nc)[threadIdx.x];
      mx = q == 0 ? v : (threadIdx.x == 3 ? (mx | v) : (v > mx ? v : mx));
      if (q == rank) own = v;
    }
    ctr_out[threadIdx.x] = own;
    ctr_out[4 + threadIdx.x] = mx;
  }
#pragma unroll
  for (int u = 0; u < kPlaceUnroll; ++u) {
  const int i = ((blockIdx.x * kPlaceUnroll + u) * kPlaceThreads + threadIdx.x) * VEC;
  if (i >= nc) return;
  const int64_t in_block = off + i;
  const int64_t col = (int64_t)r * n + in_block;
  const float* src = gath + (size_t)r * rank_stride + (size_t)row * (size_t)nc + i;
  float* dst = out + (size_t)row * (size_t)G + col;
  if (VEC == 4) {
    if (in_block + 3 < n && col + 3 < G) {
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
      continue;
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (i + v < nc && in_block + v < n && col + v < G) dst[v] = src[v];
  }
}

}  // namespace

// the placement launch of the step: four columns per lane when everything is 4-aligned
int mia::place_chunk_launch(const float* gath, float* out, int64_t G, int64_t n, int64_t off, int64_t nc, int rows, int world,
                            size_t rank_stride, int32_t* ctr_out, int rank, hipStream_t xs) {
  const bool vec = (nc % 4 == 0) && (G % 4 == 0) && (n % 4 == 0) && ((uintptr_t)out % 16 == 0);
  const int per = kPlaceThreads * kPlaceUnroll;
  const dim3 grid((unsigned)((nc / (vec ? 4 : 1) + per - 1) / per), (unsigned)rows, (unsigned)world);
  if (vec) place_chunk_kernel<4><<<grid, kPlaceThreads, 0, xs>>>(gath, out, G, n, off, (int)nc, rows, rank_stride, ctr_out, rank);
  else place_chunk_kernel<1><<<grid, kPlaceThreads, 0, xs>>>(gath, out, G, n, off, (int)nc, rows, rank_stride, ctr_out, rank);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Direct exchange.  The all-gather of the analysis ensemble moves world x (m k n) floats into every rank; RCCL's ring
// forwards each block hop by hop (per-link bound, (world - 1) latencies) into a staging buffer that a placement kernel then
// copies into the (m, k, G) result.  xGMI is point to point, so every rank can instead WRITE ITS BLOCK STRAIGHT INTO THE
// RESULT BUFFER OF ALL PEERS, over its world - 1 links at once: the result buffers are library-owned, exported with
// hipIpcGetMemHandle and mapped by every rank of the node.  Per step and slot, with sequence number q:
//   submit       free[slot][me] = q in every peer's sync area: "my buffer `slot` may be overwritten for step q" (its previous
//                result was collected, or the caller would not reuse the slot)
//   analysis     this rank's block, written into its own result buffer (no staging)
//   exchange stream:  wait  free[slot][p] >= q for all peers
//                     push  block (16-byte accesses) + this rank's four redo counters -> every peer
//                     signal ready[slot][me] = q in every peer's sync area (a kernel of its own: the push kernel's end is the
//                            system-scope release of its stores)
//                     wait  ready[slot][p] >= q for all peers; fold the counters (max over ranks)
// Flags live in fine-grained device memory and are accessed with system-scope atomics; waits are bounded (error bit 1 of
// counters[3] / [7], never a hung grid).  No collective, no staging copy, no placement kernel: 2 x block bytes of local HBM
// traffic instead of 2 x world x block.  RCCL stays the fallback (and the route of the first, exact-list step).
struct PeerPtrs { float* buf[kMaxRanks]; uint32_t* sync[kMaxRanks]; };

__global__ void __launch_bounds__(64) peer_flag_kernel(PeerPtrs pp, int world, int word, uint32_t value) {
  const int p = threadIdx.x;      // one lane per rank (own area included: keeps the arithmetic uniform)
  if (p < world) __hip_atomic_store(pp.sync[p] + word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(64) peer_wait_kernel(const uint32_t* flags /* [kMaxRanks] of this rank's area */, int world,
                                                       int rank, uint32_t seq, int32_t* err, int max_polls,
                                                       const int32_t* ctr_all /* [kMaxRanks][4] or null */, int32_t* counters) {
  const int p = threadIdx.x;
  bool ok = false;
  for (int poll = 0; poll < max_polls; ++poll) {
    const uint32_t v = (p < world && p != rank) ? __hip_atomic_load(flags + p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) : seq;
    ok = (int32_t)(v - seq) >= 0;
    if (__all(ok)) break;
    __builtin_amdgcn_s_sleep(32);
  }
  if (!__all(ok) && p == 0) atomicOr(err, 2);      // exit condition every wave reaches: ~seconds, then report
  if (ctr_all && p < 4) {                             // redo decision: max over the ranks' counters (or of the error bits)
    int mx = 0;
    for (int q = 0; q < world; ++q) {
      const int v = __hip_atomic_load(ctr_all + q * 4 + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      mx = q == 0 ? v : (p == 3 ? (mx | v) : (v > mx ? v : mx));
    }
    counters[4 + p] = p == 3 ? (mx | counters[3]) : mx;
  }
}

// block [rows][n] at column b0 of the (rows, G) result -> the same place in every peer's buffer; blockIdx.z = peer
__global__ void __launch_bounds__(256) peer_push_kernel(PeerPtrs pp, int world, int rank, int64_t G, int64_t b0, int64_t n,
                                                        int rows, int slot_word0, const int32_t* own_counters) {
  int peer = blockIdx.z;
  if (peer >= rank) ++peer;                           // (world - 1 peers)
  const float* src = pp.buf[rank] + (size_t)blockIdx.y * G + b0;
  float* dst = pp.buf[peer] + (size_t)blockIdx.y * G + b0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) {      // this rank's counters: to the peer, and (once) to itself
    const int32_t v = own_counters[threadIdx.x];
    __hip_atomic_store(reinterpret_cast<int32_t*>(pp.sync[peer]) + slot_word0 + 2 * kMaxRanks + 4 * rank + threadIdx.x, v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (blockIdx.z == 0)
      __hip_atomic_store(reinterpret_cast<int32_t*>(pp.sync[rank]) + slot_word0 + 2 * kMaxRanks + 4 * rank + threadIdx.x, v,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // 16-byte accesses where source and destination rows are aligned alike (b0, G multiples of 4), scalars otherwise
  const bool vec = ((G | b0) & 3) == 0 && ((reinterpret_cast<uintptr_t>(pp.buf[rank]) | reinterpret_cast<uintptr_t>(pp.buf[peer])) & 15) == 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
  }
}

}  // namespace

int mia::peer_slot_of(const mia_comm* c, const float* Xa) {
  if (!c || !c->peer_ready) return -1;
  for (int s = 0; s < c->peer_slots; ++s)
    if (c->peer_buf[c->rank][s] == Xa) return s;
  return -1;
}

static PeerPtrs peer_ptrs(const mia_comm* c, int slot) {
  PeerPtrs pp;
  for (int r = 0; r < kMaxRanks; ++r) {
    pp.buf[r] = r < c->world ? c->peer_buf[r][slot] : nullptr;
    pp.sync[r] = r < c->world ? c->peer_sync[r] : nullptr;
  }
  return pp;
}

// first half of an exchange: new sequence number, "my buffer of this slot may be overwritten" to every peer (stream ps)
int mia::peer_begin(mia_comm* c, int slot, hipStream_t ps, uint32_t* seq_out) {
  const uint32_t seq = ++c->peer_seq[slot];
  peer_flag_kernel<<<1, 64, 0, ps>>>(peer_ptrs(c, slot), c->world, slot * kSyncSlotWords + kMaxRanks + c->rank, seq);
  MIA_LAUNCH_CHECK();
  *seq_out = seq;
  return MIA_OK;
}

// second half, on the exchange stream cs (the caller has ordered it behind the block's producer): wait for the peers'
// buffers, push block [rows][b0, b1) and the four counters, signal, wait for the peers' blocks, fold the counters
int mia::peer_finish(mia_comm* c, int slot, uint32_t seq, int64_t G, int64_t b0, int64_t b1, int rows, int32_t* counters,
                     hipStream_t cs) {
  const int world = c->world, rank = c->rank, sw0 = slot * kSyncSlotWords;
  const PeerPtrs pp = peer_ptrs(c, slot);
  const uint32_t* my = c->peer_sync[rank] + sw0;
  peer_wait_kernel<<<1, 64, 0, cs>>>(my + kMaxRanks, world, rank, seq, counters + 3, c->peer_wait_polls, nullptr, nullptr);
  MIA_LAUNCH_CHECK();
  const int64_t nb = b1 > b0 ? b1 - b0 : 0;
  unsigned gx = (unsigned)((nb / 4 + 255) / 256);
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  peer_push_kernel<<<dim3(gx, (unsigned)(nb ? rows : 1), (unsigned)(world - 1)), 256, 0, cs>>>(pp, world, rank, G, nb ? b0 : 0, nb,
                                                                                          rows, sw0, counters);
  MIA_LAUNCH_CHECK();
  peer_flag_kernel<<<1, 64, 0, cs>>>(pp, world, sw0 + rank, seq);
  MIA_LAUNCH_CHECK();
  peer_wait_kernel<<<1, 64, 0, cs>>>(my, world, rank, seq, counters + 3, c->peer_wait_polls,
                                     reinterpret_cast<const int32_t*>(my + 2 * kMaxRanks), counters);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" const char* mia_comm_last_error(void) { return g_comm_error; }

extern "C" int mia_comm_load(const char* rccl_path) {
  if (g_rccl.handle) return MIA_OK;
  const char* path = (rccl_path && rccl_path[0]) ? rccl_path : "librccl.so";
  void* h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
  if (!h) {
    snprintf(g_comm_error, sizeof(g_comm_error), "dlopen(%s) failed: %s", path, dlerror());
    return MIA_ERR_COMM;
  }
  RcclApi api;
  api.handle = h;
  api.GetUniqueId = (pfn_ncclGetUniqueId)dlsym(h, "ncclGetUniqueId");
  api.CommInitRank = (pfn_ncclCommInitRank)dlsym(h, "ncclCommInitRank");
  api.CommDestroy = (pfn_ncclCommDestroy)dlsym(h, "ncclCommDestroy");
  api.AllGather = (pfn_ncclAllGather)dlsym(h, "ncclAllGather");
  api.AllReduce = (pfn_ncclAllReduce)dlsym(h, "ncclAllReduce");
  api.GetErrorString = (pfn_ncclGetErrorString)dlsym(h, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather || !api.AllReduce) {
    snprintf(g_comm_error, sizeof(g_comm_error), "%s does not export the RCCL collectives", path);
    return MIA_ERR_COMM;
  }
  g_rccl = api;
  return MIA_OK;
}

extern "C" int mia_comm_unique_id(void* id128) {
  if (!id128) return MIA_ERR_NULL;
  if (!g_rccl.handle) { set_error("mia_comm_load was not called", 0); return MIA_ERR_COMM; }
  ncclUniqueId id;
  int rc = g_rccl.GetUniqueId(&id);
  if (rc != kNcclSuccess) { set_error("ncclGetUniqueId failed", rc); return MIA_ERR_COMM; }
  memcpy(id128, id.internal, 128);
  return MIA_OK;
}

extern "C" int mia_comm_create(const void* id128, int rank, int world, mia_comm_t** out) {
  if (!id128 || !out) return MIA_ERR_NULL;
  if (world <= 0 || rank < 0 || rank >= world) return MIA_ERR_SIZE;
  if (!g_rccl.handle) { set_error("mia_comm_load was not called", 0); return MIA_ERR_COMM; }
  ncclUniqueId id;
  memcpy(id.internal, id128, 128);
  mia_comm* c = new mia_comm();
  c->rank = rank;
  c->world = world;
  int rc = g_rccl.CommInitRank(&c->nccl, world, id, rank);
  if (rc != kNcclSuccess) { set_error("ncclCommInitRank failed", rc); delete c; return MIA_ERR_COMM; }
  *out = c;
  return MIA_OK;
}

extern "C" int mia_comm_create_custom(int rank, int world, mia_allgather_fn allgather,
                                      mia_allreduce_max_i32_fn allreduce_max, void* ctx, mia_comm_t** out) {
  if (!allgather || !allreduce_max || !out) return MIA_ERR_NULL;
  if (world <= 0 || rank < 0 || rank >= world) return MIA_ERR_SIZE;
  mia_comm* c = new mia_comm();
  c->rank = rank;
  c->world = world;
  c->ag = allgather;
  c->ar = allreduce_max;
  c->ctx = ctx;
  *out = c;
  return MIA_OK;
}

// a communicator that only carries the block partition (rank, world): for steps whose analysis STAYS block-sharded
// (MIA_STEP_NO_GATHER -- what the reference's dask chunks along `grid` do, interface/letkf.py:118-131); no exchange can run on it
extern "C" int mia_comm_create_partition(int rank, int world, mia_comm_t** out) {
  if (!out) return MIA_ERR_NULL;
  if (world <= 0 || rank < 0 || rank >= world) return MIA_ERR_SIZE;
  mia_comm* c = new mia_comm();
  c->rank = rank;
  c->world = world;
  *out = c;
  return MIA_OK;
}

extern "C" int mia_comm_set_place_stream(mia_comm_t* c, void* stream) {
  if (!c) return MIA_ERR_NULL;
  c->place_stream = (hipStream_t)stream;
  return MIA_OK;
}

// ---- direct exchange: buffers, handles, attachment (protocol: see "Direct exchange" above)
extern "C" int mia_comm_peer_alloc(mia_comm_t* c, size_t result_bytes, int n_slots, void* ipc_handles_out) {
  if (!c) return MIA_ERR_NULL;
  if (n_slots < 1 || n_slots > kMaxSlots || result_bytes == 0 || c->world > kMaxRanks) return MIA_ERR_SIZE;
  if (c->peer_slots) return MIA_ERR_UNSUPPORTED;          // one allocation per communicator
  (void)hipGetLastError();
  hipIpcMemHandle_t* hs = reinterpret_cast<hipIpcMemHandle_t*>(ipc_handles_out);
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "the handle table of mia_comm_peer_alloc / _open is 64 bytes per entry");
  for (int s = 0; s < n_slots; ++s) {
    void* b = nullptr;
    if (hipMalloc(&b, mia::align_up(result_bytes, 256)) != hipSuccess) { set_error("hipMalloc of a result buffer failed", 0); (void)hipGetLastError(); return MIA_ERR_COMM; }
    c->peer_buf[c->rank][s] = (float*)b;
    c->peer_slots = s + 1;
    c->peer_owned = true;
    if (hs && hipIpcGetMemHandle(&hs[s], b) != hipSuccess) { set_error("hipIpcGetMemHandle(result buffer) failed", 0); (void)hipGetLastError(); return MIA_ERR_COMM; }
  }
  void* sy = nullptr;
  if (hipExtMallocWithFlags(&sy, kSyncBytes, hipDeviceMallocFinegrained) != hipSuccess) { set_error("fine-grained allocation of the sync area failed", 0); (void)hipGetLastError(); return MIA_ERR_COMM; }
  c->peer_sync[c->rank] = (uint32_t*)sy;
  if (hipMemset(sy, 0, kSyncBytes) != hipSuccess) { (void)hipGetLastError(); return MIA_ERR_COMM; }
  if (hs && hipIpcGetMemHandle(&hs[n_slots], sy) != hipSuccess) { set_error("hipIpcGetMemHandle(sync area) failed", 0); (void)hipGetLastError(); return MIA_ERR_COMM; }
  c->peer_bytes = result_bytes;
  if (c->world == 1) c->peer_ready = 1;
  return MIA_OK;
}

static void peer_check_ready(mia_comm* c) {
  int ok = c->peer_slots > 0;
  for (int r = 0; r < c->world && ok; ++r) {
    ok = c->peer_sync[r] != nullptr;
    for (int s = 0; s < c->peer_slots && ok; ++s) ok = c->peer_buf[r][s] != nullptr;
  }
  c->peer_ready = ok;
}

// all_handles: [world][n_slots + 1] handles as every rank's mia_comm_peer_alloc filled them (any all-gather of the host's)
extern "C" int mia_comm_peer_open(mia_comm_t* c, const void* all_handles) {
  if (!c || !all_handles) return MIA_ERR_NULL;
  if (!c->peer_slots) return MIA_ERR_SIZE;
  (void)hipGetLastError();
  const hipIpcMemHandle_t* hs = reinterpret_cast<const hipIpcMemHandle_t*>(all_handles);
  const int per = c->peer_slots + 1;
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank) continue;
    for (int s = 0; s < per; ++s) {
      void* ptr = nullptr;
      if (hipIpcOpenMemHandle(&ptr, hs[(size_t)r * per + s], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        set_error("hipIpcOpenMemHandle failed", r);
        (void)hipGetLastError();
        return MIA_ERR_COMM;
      }
      if (s < c->peer_slots) c->peer_buf[r][s] = (float*)ptr; else c->peer_sync[r] = (uint32_t*)ptr;
    }
    c->peer_opened[r] = true;
  }
  peer_check_ready(c);
  return c->peer_ready ? MIA_OK : MIA_ERR_COMM;
}

// in-process attachment of a peer's buffers (ranks that share an address space: tests, one process driving several GPUs)
extern "C" int mia_comm_peer_attach(mia_comm_t* c, int peer, void* const* result_bufs, void* sync_area) {
  if (!c || !result_bufs || !sync_area) return MIA_ERR_NULL;
  if (peer < 0 || peer >= c->world || peer == c->rank || !c->peer_slots) return MIA_ERR_SIZE;
  for (int s = 0; s < c->peer_slots; ++s) c->peer_buf[peer][s] = (float*)result_bufs[s];
  c->peer_sync[peer] = (uint32_t*)sync_area;
  peer_check_ready(c);
  return MIA_OK;
}

extern "C" int mia_comm_peer_wait_bound(mia_comm_t* c, int log2_polls) {
  if (!c) return MIA_ERR_NULL;
  if (log2_polls < 10 || log2_polls > 30) return MIA_ERR_SIZE;
  c->peer_wait_polls = 1 << log2_polls;
  return MIA_OK;
}

extern "C" void* mia_comm_peer_buffer(mia_comm_t* c, int slot) {
  return (c && slot >= 0 && slot < c->peer_slots) ? (void*)c->peer_buf[c->rank][slot] : nullptr;
}
extern "C" void* mia_comm_peer_sync_area(mia_comm_t* c) { return c ? (void*)c->peer_sync[c->rank] : nullptr; }

// The exchange alone: block [rows][b0, b1) of result buffer `slot` (already written by work enqueued on `stream`) goes to
// every peer; when `stream` has passed this call, the peers' blocks have landed in this rank's buffer and counters[4..7]
// hold the maximum over the ranks of everybody's counters[0..3] (device int32[8]).  All ranks call it in the same order.
extern "C" int mia_comm_peer_exchange(mia_comm_t* c, int slot, int rows, int64_t G, int64_t b0, int64_t b1, int32_t* counters,
                                      void* stream) {
  if (!c || !counters) return MIA_ERR_NULL;
  if (!c->peer_ready || slot < 0 || slot >= c->peer_slots || rows < 1 || G < 1 || b0 < 0 || b1 > G) return MIA_ERR_SIZE;
  if ((size_t)rows * G * sizeof(float) > c->peer_bytes) return MIA_ERR_SIZE;
  if (c->world == 1) return MIA_OK;
  (void)hipGetLastError();
  uint32_t seq = 0;
  int rc = peer_begin(c, slot, (hipStream_t)stream, &seq);
  if (rc != MIA_OK) return rc;
  return peer_finish(c, slot, seq, G, b0, b1, rows, counters, (hipStream_t)stream);
}

// A waiter of the last exchange on `slot` gave up (error bit 2 of counters[3] / [7]): wait AGAIN for the peers' ready flags of that
// exchange and fold the counters once more -- a peer that has not raised its flag within the bound is late (a first-step table
// build, I/O between two steps, a debugger), and its push does not depend on anything this rank does.  Clears error bit 2 first; it
// is set again if this wait gives up too.  The caller decides how often to come back before it calls the peer dead.
__global__ void __launch_bounds__(64) peer_clear_timeout_kernel(int32_t* counters) {
  if (threadIdx.x == 0) { counters[3] &= ~2; counters[7] &= ~2; }
}
extern "C" int mia_comm_peer_rewait(mia_comm_t* c, int slot, int32_t* counters, void* stream) {
  if (!c || !counters) return MIA_ERR_NULL;
  if (!c->peer_ready || slot < 0 || slot >= c->peer_slots) return MIA_ERR_SIZE;
  if (c->world == 1) return MIA_OK;
  (void)hipGetLastError();
  hipStream_t cs = (hipStream_t)stream;
  const uint32_t* my = c->peer_sync[c->rank] + slot * kSyncSlotWords;
  peer_clear_timeout_kernel<<<1, 64, 0, cs>>>(counters);
  MIA_LAUNCH_CHECK();
  peer_wait_kernel<<<1, 64, 0, cs>>>(my, c->world, c->rank, c->peer_seq[slot], counters + 3, c->peer_wait_polls,
                                     reinterpret_cast<const int32_t*>(my + 2 * kMaxRanks), counters);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_comm_destroy(mia_comm_t* c) {
  if (!c) return MIA_OK;
  for (int r = 0; r < c->world && r < kMaxRanks; ++r) {
    if (r == c->rank || !c->peer_opened[r]) continue;
    for (int s = 0; s < c->peer_slots; ++s) if (c->peer_buf[r][s]) (void)hipIpcCloseMemHandle(c->peer_buf[r][s]);
    if (c->peer_sync[r]) (void)hipIpcCloseMemHandle(c->peer_sync[r]);
  }
  if (c->peer_owned) {
    for (int s = 0; s < c->peer_slots; ++s) if (c->peer_buf[c->rank][s]) (void)hipFree(c->peer_buf[c->rank][s]);
    if (c->peer_sync[c->rank]) (void)hipFree(c->peer_sync[c->rank]);
  }
  (void)hipGetLastError();
  for (int i = 0; i < c->n_ev; ++i) (void)hipEventDestroy(c->ev[i]);
  if (c->n_ev)
    for (int i = 0; i < kMaxChunks; ++i) (void)hipEventDestroy(c->evp[i]);
  if (c->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(c->nccl);
  delete c;
  return MIA_OK;
}
