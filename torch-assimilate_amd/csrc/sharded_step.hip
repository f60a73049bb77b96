// Native driver of one assimilation step of one rank's block of grid points (single C call per step):
//   pack records -> observation cell index + Gaspari-Cohn neighbour lists -> local analysis, and for world > 1
//   the block is analysed in chunks whose RCCL all-gather (+ the copy into the (m, k, G) result) runs on a
//   second HIP stream while the next chunk is analysed.
// Replaces the per-step Python orchestration (≈15 launches through ctypes / torch.distributed cost more host
// time than the ≈0.35 ms of GPU work they enqueue).  The step it drives is the reference's
// DaskLocalization -> localized_etkf -> apply_weights path (pytassim/interface/letkf.py:102-137,
// etkf.py:169-207); the reference has no multi-device path, its unit of distribution is the
// dask chunk of grid points (letkf.py:118-131), which is the block / chunk here.
//
// The file in reading order: the workspace layout; events, the per-workspace table and the once-per-step StepDecision; the small
// stream / event entries; the step itself -- its arguments as one block (mia_step_args_t) plus a StepState, and step_impl as
//   step_plan     every decision that follows from the arguments, the layout and the communicator
//   step_decide   the step's decision about its workspace, taken where the preparation is enqueued, and what follows from it
//   step_prepare  phase 0, stage 1: clears, records / index / lists on the preparation stream, the ordering events
//   step_analyse  phase 0, stage 2: the waits, the one-launch-over-pieces forms, analyse_piece per piece
//   step_redo     phase 1: declined points, piece by piece
//   exchange_piece  wait or segment wait, all-gather, placement
// -- the entries that fill a block from positional parameters; the launch threads and the submitted-step entries.
// The communicator, the placement kernel and the direct peer exchange are step_comm.hip (mia_step_comm.h).
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

#include "mia_common.h"
#include "mia_kernels.h"
#include "mia_options.h"
#include "mia_pack_dev.h"
#include "mia_step_comm.h"
#include "mia_tiles.h"

using mia::kMaxChunks;

namespace {

struct StepLayout {
  size_t rec, loc, cnt, idx, w, done, bufs, gath, total;
  size_t hrec, tl, scratch;      // tile route: split records (P + 1), tile lists of the block, 256 bytes of scratch counters
  size_t loc_bytes, send_bytes, chunk_bytes;
  int cap, ut;
  int64_t n, nc;
};

int step_layout(int64_t G, int m, int k, int64_t P, int n_coord, int world, int n_chunks, int p_max_assumed,
                StepLayout* L, int tile_extra = 0) {
  if (G < 0 || m <= 0 || k <= 0 || P < 0 || n_coord <= 0 || world <= 0 || n_chunks <= 0 || n_chunks > kMaxChunks - 1 ||
      p_max_assumed < 0)
    return MIA_ERR_SIZE;
  const int kp = (k + 1 + 3) / 4 * 4;
  L->n = (G + world - 1) / world;
  L->nc = ((L->n + n_chunks - 1) / n_chunks + 15) / 16 * 16;   // (whole tiles of sixteen points per piece)
  L->cap = p_max_assumed < 8 ? 8 : (p_max_assumed + 7) / 8 * 8;
  size_t o = 0;
  L->rec = o; o = mia::align_up(o + (size_t)(P > 0 ? P : 1) * kp * sizeof(float), 256);
  int rc = mia_letkf_localize_workspace_bytes(P, n_coord, &L->loc_bytes);
  if (rc != MIA_OK) return rc;
  L->loc = o; o = mia::align_up(o + L->loc_bytes, 256);
  L->cnt = o; o = mia::align_up(o + (size_t)L->n * sizeof(int32_t), 256);
  L->idx = o; o = mia::align_up(o + (size_t)L->n * L->cap * sizeof(int32_t), 256);
  L->w = o; o = mia::align_up(o + (size_t)L->n * L->cap * sizeof(double), 256);
  L->done = o; o = mia::align_up(o + (size_t)kMaxChunks * 64 * mia::kSlotStride * sizeof(int32_t), 256);
  // (the workspace is sized for the largest tile lists the ensemble size allows, so that a caller may add slots -- MIA_STEP_TILE_EXTRA
  //  -- without a new workspace query)
  const int ut0 = mia::tile_ut_for(p_max_assumed < L->cap ? p_max_assumed : L->cap), kt = (k + 15) >> 4;
  const int ut_most = kt + 1 < 6 ? kt + 1 : 6;
  L->ut = ut0 + tile_extra;
  L->hrec = L->tl = o;
  if (ut0 <= ut_most) {
    L->hrec = o; o = mia::align_up(o + (size_t)(P + 1) * mia::split_rec_bytes(k), 256);
    L->tl = o; o = mia::align_up(o + mia::tile_list_layout(L->n, ut_most).bytes, 256);
  }
  if (L->ut > ut_most) L->ut = 7;      // (no tile route)
  L->scratch = o; o += 256;
  L->bufs = L->gath = o;
  L->send_bytes = (size_t)m * k * L->nc * sizeof(float) + 16;   // piece + counter trailer
  L->chunk_bytes = mia::align_up(L->send_bytes, 256);
  if (world > 1 || n_chunks > 1) {
    L->bufs = o; o += L->chunk_bytes * n_chunks;
    L->gath = o; o += mia::align_up(L->send_bytes * world, 256) * n_chunks;
  }
  L->total = o;
  return MIA_OK;
}

}  // namespace

namespace {
// one-shot profiling hook (mia_letkf_step_timing_events)
thread_local hipEvent_t t_time_start = nullptr, t_time_stop = nullptr;

// events that order the preparation stream before the analysis stream (no communicator, hence no event storage of
// its own, on the single-rank route): a small ring, created on first use
// (one ring per device: an event belongs to the device that was current when it was created, and the launch threads serve
//  jobs of several devices)
constexpr int kPrepDevices = 16;
hipEvent_t g_prep_ev[kPrepDevices][64];
std::atomic<unsigned> g_prep_next[kPrepDevices];
std::mutex g_prep_mutex;
bool g_prep_init[kPrepDevices] = {};
int prep_event(hipEvent_t* ev) {
  int dev = 0;
  MIA_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kPrepDevices) return MIA_ERR_UNSUPPORTED;
  {
    std::lock_guard<std::mutex> lock(g_prep_mutex);
    if (!g_prep_init[dev]) {
      for (int i = 0; i < 64; ++i) MIA_HIP_TRY(hipEventCreateWithFlags(&g_prep_ev[dev][i], hipEventDisableTiming));
      g_prep_init[dev] = true;
    }
  }
  *ev = g_prep_ev[dev][g_prep_next[dev].fetch_add(1) & 63];
  return MIA_OK;
}
}  // namespace

extern "C" int mia_letkf_step_timing_events(void* start_event, void* stop_event) {
  if ((start_event == nullptr) != (stop_event == nullptr)) return MIA_ERR_NULL;
  t_time_start = (hipEvent_t)start_event;
  t_time_stop = (hipEvent_t)stop_event;
  return MIA_OK;
}

// what the tile lists held by a step workspace were built for (geometry epochs, MIA_STEP_REUSE_LISTS)
struct GeomStamp {
  int route, ut, bucket, n_coord, n_r, rank, world, k;
  int64_t G, P;
  double eps, rc[MIA_MAX_RADII];
  int cg[MIA_MAX_COORD];
  double per[MIA_MAX_COORD];      // periods of the cyclic coordinates (0: open)
};
static std::mutex g_stamp_mu;
// ... and which of the index layout's two per-cell count arrays (cursor / start: the bucket index needs no starts) the workspace's
// NEXT bucket build bins into.  Every bucket step uses one and has its analysis launch put the OTHER back to zero -- the one the
// previous bucket step on this workspace left dirty -- because with the fused kernel (letkf_tile2f.hip) the wavefronts that read
// the counts and the ones that would clear them are the same launch.  cnt_use / fused: the decision taken for the step in flight.
// unknown: the entry was made for a workspace this table knows nothing about (its first step -- or one whose entry was pushed out of
// the table since): the state of its count arrays is not known either, so its next index build clears them whatever the caller
// says about the workspace (MIA_STEP_WS_CLEAN).
struct GeomEntry { void* ws; GeomStamp st; bool valid, reuse; int cnt_cur, cnt_use; bool fused; bool unknown; };
static std::deque<GeomEntry> g_stamps;        // (a handful of pipeline slots per process)
// decide = true (a step's preparation): reuse is granted when asked for AND the workspace's stamp equals `now`; otherwise the
// stamp becomes `now` (lists are rebuilt; route 0 = no tile lists).  decide = false: the decision taken for this workspace.
static bool geom_reuse_decision(void* ws, const GeomStamp& now, bool asked, bool decide) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  GeomEntry* e = nullptr;
  for (auto& x : g_stamps)
    if (x.ws == ws) { e = &x; break; }
  if (!decide) return e ? e->reuse : false;
  if (!e) {
    if (g_stamps.size() >= 64) g_stamps.pop_front();
    g_stamps.push_back(GeomEntry{ws, now, false, false, 0, 0, false, true});
    e = &g_stamps.back();
  }
  e->reuse = asked && e->valid && memcmp(&e->st, &now, sizeof now) == 0;
  if (!e->reuse) { memcpy(&e->st, &now, sizeof now); e->valid = now.route != 0; }      // (bytes, padding included: compared as bytes)
  return e->reuse;
}

// The count array of a step's bucket build and whether its analysis localises in the kernel.  decide = true (the step's
// preparation; after geom_reuse_decision, which creates the entry): `bucket_step` takes the workspace's current array and flips it
// for the next one; decide = false: what was decided.  scan_build: a scan-based index is about to be built on the workspace -- it
// needs array 0 (cursor) clean, returns false when a full clear must come first, and leaves array 0 the current one.
// *must_clear: the workspace's count arrays are in an unknown state (see GeomEntry): the build about to run clears them first.
static void count_array_decision(void* ws, bool decide, bool bucket_step, bool fused, int* use, bool* fused_out, bool* must_clear) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  GeomEntry* e = nullptr;
  for (auto& x : g_stamps)
    if (x.ws == ws) { e = &x; break; }
  *must_clear = false;
  if (!e) { *use = 0; *fused_out = false; *must_clear = true; return; }
  if (decide) {
    if (bucket_step && e->unknown) { *must_clear = true; e->unknown = false; e->cnt_cur = 0; }
    e->fused = bucket_step && fused;
    e->cnt_use = e->cnt_cur;
    if (bucket_step) e->cnt_cur ^= 1;
  }
  *use = e->cnt_use;
  *fused_out = e->fused;
}
// What a step decided where its preparation was enqueued (stage 1 / phase 0), CARRIED by the step -- the job of a step in flight, a
// local of the one-call form -- to where its analysis is enqueued: the table above is only the workspace's memory BETWEEN steps (its
// stamp, which count array comes next).  An entry pushed out of the table while a step is in flight costs that workspace's next
// step a full rebuild (`unknown`), never the step in flight its decisions (round 4 looked them up again by pointer in stage 2).
struct StepDecision { bool set = false, reuse = false, fused = false, must_clear = false; int cnt_use = 0; };

// forget what the table holds about a workspace (its memory is about to be freed or handed to another runner: the next step on that
// address starts from `unknown`)
extern "C" int mia_letkf_step_workspace_release(void* ws) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  for (auto it = g_stamps.begin(); it != g_stamps.end(); ++it)
    if (it->ws == ws) { g_stamps.erase(it); break; }
  return MIA_OK;
}

static bool count_arrays_clean_for_scan(void* ws) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  for (auto& x : g_stamps)
    if (x.ws == ws) {
      const bool clean = x.cnt_cur == 0 && !x.unknown;
      x.cnt_cur = 0;
      x.unknown = false;      // (the caller clears everything when told "not clean")
      return clean;
    }
  return false;
}

// Host-overhead helpers of the pipelined step loop (one ctypes call each instead of five torch calls): the eight counters
// of a step are copied to pinned host memory on `on_stream` once `after_stream` has passed its current point, and an event
// the library owns (created on first use, reused by the caller for the same slot) marks the copy's completion.
extern "C" int mia_letkf_step_readback(const int32_t* counters, int32_t* host8, void* after_stream, void* on_stream,
                                       void** done_event) {
  if (!counters || !host8 || !done_event) return MIA_ERR_NULL;
  (void)hipGetLastError();
  hipStream_t a = (hipStream_t)after_stream, o = (hipStream_t)on_stream;
  hipEvent_t ev = (hipEvent_t)*done_event;
  if (!ev) {
    MIA_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *done_event = (void*)ev;
  }
  if (a != o) {
    hipEvent_t pe;
    int rc = prep_event(&pe);
    if (rc != MIA_OK) return rc;
    MIA_HIP_TRY(hipEventRecord(pe, a));
    MIA_HIP_TRY(hipStreamWaitEvent(o, pe, 0));
  }
  MIA_HIP_TRY(hipMemcpyAsync(host8, counters, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, o));
  MIA_HIP_TRY(hipEventRecord(ev, o));
  return MIA_OK;
}
static int readback_after_event(const int32_t* counters, int32_t* host8, hipEvent_t after, void* on_stream, void** done_event) {
  if (!counters || !host8 || !done_event || !after) return MIA_ERR_NULL;
  (void)hipGetLastError();
  hipStream_t o = (hipStream_t)on_stream;
  hipEvent_t ev = (hipEvent_t)*done_event;
  if (!ev) {
    MIA_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *done_event = (void*)ev;
  }
  MIA_HIP_TRY(hipStreamWaitEvent(o, after, 0));
  MIA_HIP_TRY(hipMemcpyAsync(host8, counters, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, o));
  MIA_HIP_TRY(hipEventRecord(ev, o));
  return MIA_OK;
}
extern "C" int mia_event_synchronize(void* event) {
  if (!event) return MIA_ERR_NULL;
  MIA_HIP_TRY(hipEventSynchronize((hipEvent_t)event));
  return MIA_OK;
}
// `dst` waits for everything enqueued on `src` so far (an event of the caller's, created on first use): the two runtime calls
// of torch's Stream.wait_stream without its per-call Python objects (~8 us of a ~25 us submit)
extern "C" int mia_stream_wait_stream(void* dst_stream, void* src_stream, void** event_io) {
  if (!event_io) return MIA_ERR_NULL;
  (void)hipGetLastError();
  if (!*event_io) {
    hipEvent_t e = nullptr;
    MIA_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *event_io = (void*)e;
  }
  MIA_HIP_TRY(hipEventRecord((hipEvent_t)*event_io, (hipStream_t)src_stream));
  MIA_HIP_TRY(hipStreamWaitEvent((hipStream_t)dst_stream, (hipEvent_t)*event_io, 0));
  return MIA_OK;
}

extern "C" int mia_stream_wait_event(void* stream, void* event) {
  if (!event) return MIA_ERR_NULL;
  MIA_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
  return MIA_OK;
}
extern "C" int mia_event_destroy(void* event) {
  if (event) (void)hipEventDestroy((hipEvent_t)event);
  return MIA_OK;
}

extern "C" int mia_letkf_sharded_step_workspace_bytes(int64_t G, int m, int k, int64_t P, int n_coord, int world,
                                                      int n_chunks, int p_max_assumed, size_t* bytes) {
  if (!bytes) return MIA_ERR_NULL;
  StepLayout L;
  int rc = step_layout(G, m, k, P, n_coord, world, n_chunks, p_max_assumed, &L);
  if (rc != MIA_OK) return rc;
  *bytes = L.total;
  return MIA_OK;
}

extern "C" int mia_letkf_sharded_step_f32(const float* X, int64_t G, int m, int k,
                                          const float* Yb, const float* d, int64_t P,
                                          const double* grid_xyz, const double* obs_xyz, int n_coord,
                                          const int32_t* coord_group, const double* gc_c, int n_r, double gc_eps,
                                          float inf_factor, float gamma, int method, int p_max_assumed,
                                          mia_comm_t* comm, int n_chunks, int phase,
                                          float* Xa, int32_t* flags, int32_t* counters,
                                          void* ws, size_t ws_bytes, void* stream, void* comm_stream) {
  return mia_letkf_sharded_step_streams_f32(X, G, m, k, Yb, d, P, grid_xyz, obs_xyz, n_coord, coord_group, gc_c, n_r,
                                            gc_eps, inf_factor, gamma, method, p_max_assumed, comm, n_chunks, phase, Xa,
                                            flags, counters, ws, ws_bytes, stream, comm_stream, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// The step.  Its arguments travel as ONE block (mia_step_args_t, include/mia_letkf.h) from the ABI boundary to the last launch;
// beside it a step carries only its own state (StepState).  step_impl is: plan, decide, then prepare | analyse | redo, each piece
// of the exchange route through exchange_piece.
constexpr int kStepPrepDone = 0x100;      // internal step flag: the launch thread has waited for the preparation on the host

// What a step carries from call to call besides its arguments: the one-call form makes one on its stack, a step in flight keeps it in
// its job.  stage 0: the whole step.  The launch threads split it: stage 1 = what goes to the preparation stream (free flags of the
// direct exchange, records, index, lists) up to the event that orders the analysis behind it (pe, seq out); stage 2 = everything
// from that wait on (analysis, exchange), with pe / seq as stage 1 left them.
struct StepState {
  int stage = 0;
  int flags = 0;                   // the block's step_flags as this call takes them (the one-call block entry drops MIA_STEP_NO_JOIN,
                                   // the analysis thread adds kStepPrepDone): set where a step enters, copied into the plan
                                   // (StepPlan::flags), which is what the parts read
  hipEvent_t pe = nullptr;         // the preparation is enqueued (recorded on the preparation stream when that is a stream of its own)
  uint32_t seq = 0;                // sequence number of the direct exchange
  hipEvent_t kdone = nullptr;      // completion event carried by the analysis launch itself (stage 2), if any
  StepDecision dec;                // what stage 1 decided about the workspace's lists and count arrays, for stage 2
};

static inline bool step_tables_fit(int n_coord, int n_r) {      // (the block's coordinate-group, radius and period arrays)
  return n_coord >= 1 && n_coord <= MIA_MAX_COORD && n_r >= 1 && n_r <= MIA_MAX_RADII;
}
// the period of a block in the internal convention of the index builds (check_period): the block's array where some coordinate is
// cyclic, nullptr where none is; MIA_ERR_ARG unless every entry is finite and >= 0.  (A block with a bad n_coord is refused by the
// plan, as MIA_ERR_SIZE: no entry is read.)
static inline int step_period(const mia_step_args_t& a, const double** period) {
  const int n = a.n_coord >= 1 && a.n_coord <= MIA_MAX_COORD ? a.n_coord : 0;
  return mia::check_period(a.period, n, period) != MIA_OK ? MIA_ERR_ARG : MIA_OK;
}

// Every decision of a step that follows from its arguments, the layout and the communicator -- evaluated identically by stage 1,
// stage 2 and a redo call (phase 1) of the same step -- and, once step_decide has run, what follows from the step's decision.
struct StepPlan {
  StepLayout L;
  int flags;                       // the step's flags as this call takes them (StepState::flags): what every part reads,
                                   // never the block's step_flags
  int world, rank, n_chunks;       // (n_chunks: pieces actually taken -- one without a communicator, with NO_GATHER, on the peer route)
  int peer_slot, extra, pm_tl, rows;
  // exchange route: any real multi-rank world; a one-rank communicator takes it only when chunking is asked
  // for (lets a single-GPU box drive the RCCL calls and the chunk pipeline)
  // direct exchange: Xa is one of the communicator's peer-mapped result buffers (every rank passes the same slot)
  // MIA_STEP_NO_GATHER: this rank analyses its block of the partition and keeps it -- Xa is the block, (m k, block length),
  // nothing is exchanged and no counter is reduced over the ranks (every rank validates its own step)
  bool no_gather, peer, exch;
  bool signal_mode;                // MIA_SEGMENT_SIGNAL=0: one launch + one event per piece instead of the segmented launch (fallback / A-B runs)
  bool lazy, tl_route, tl_rbf, tl_bucket, want_fused, eig_only;
  int64_t b0, b1;                  // this rank's block of grid points
  hipStream_t s, cs, ps;           // analysis, exchange, preparation (records, index, lists)
  const double* period;            // nullptr = open -- every index build of the step takes it
  const int2* tl_th;               // coefficient table of the tile kernels
  const float2* tl_tc;
  GeomStamp stamp;
  char* base;                      // the workspace and its parts
  float* rec;
  int32_t *cnt, *idx, *done, *ctr;
  double* w;
  size_t gath_stride, done_ints;
  // ---- from the step's decision (step_decide)
  bool tl_reuse, tl_fused, cnt_must_clear, zero_in_kernel, carried;
  int* tl_counts;
  mia::Tile2Housekeeping tl_hk;
  const mia::Tile2Housekeeping* hk;      // &tl_hk where the analysis launch does the housekeeping, else nullptr
  mia::Tile2Loc tl_loc;
  const mia::Tile2Loc* loc;              // &tl_loc where the analysis wavefronts localise, else nullptr
};

static int step_plan(const mia_step_args_t& a, const StepState& st, StepPlan* plan) {
  StepPlan& p = *plan;
  if (step_period(a, &p.period) != MIA_OK) return MIA_ERR_ARG;
  if (!a.X || !a.Xa || !a.flags || !a.counters || !a.ws || !a.grid_xyz) return MIA_ERR_NULL;
  if (a.P > 0 && (!a.Yb || !a.d || !a.obs_xyz)) return MIA_ERR_NULL;
  if (a.method < 0 || a.method > 2 || (a.phase != 0 && a.phase != 1)) return MIA_ERR_SIZE;
  if ((uintptr_t)a.ws % 256) return MIA_ERR_ALIGN;
  if (!step_tables_fit(a.n_coord, a.n_r)) return MIA_ERR_SIZE;
  mia_comm* comm = a.comm;
  const int m = a.m, k = a.k, flags = p.flags = st.flags;
  const int64_t G = a.G, P = a.P;
  p.world = comm ? comm->world : 1;
  p.rank = comm ? comm->rank : 0;
  p.n_chunks = comm ? a.n_chunks : 1;
  p.no_gather = comm && (flags & MIA_STEP_NO_GATHER) != 0;
  if (p.no_gather) p.n_chunks = 1;
  if (comm && !p.no_gather && p.world > 1 && !comm->nccl && !comm->ag) return MIA_ERR_COMM;      // (a partition-only communicator)
  p.peer_slot = (comm && p.world > 1 && !p.no_gather) ? mia::peer_slot_of(comm, a.Xa) : -1;
  p.peer = p.peer_slot >= 0;
  if (p.peer) p.n_chunks = 1;
  p.exch = comm && !p.peer && !p.no_gather && (p.world > 1 || p.n_chunks > 1);
  p.extra = (flags >> 4) & 7;      // MIA_STEP_TILE_EXTRA
  StepLayout& L = p.L;
  int rc = step_layout(G, m, k, P, a.n_coord, p.world, p.n_chunks, a.p_max_assumed, &L, p.extra);
  if (rc != MIA_OK) return rc;
  if (a.ws_bytes < L.total) return MIA_ERR_WORKSPACE;
  if ((p.exch || p.peer) && !a.comm_stream) return MIA_ERR_NULL;
  if (p.peer && (size_t)m * k * G * sizeof(float) > comm->peer_bytes) return MIA_ERR_SIZE;
  p.s = (hipStream_t)a.stream;
  p.cs = (hipStream_t)a.comm_stream;
  p.ps = a.prep_stream ? (hipStream_t)a.prep_stream : p.s;
  p.signal_mode = mia::option(MIA_OPT_SEGMENT_SIGNAL) != 0;
  p.b0 = (int64_t)p.rank * L.n < G ? (int64_t)p.rank * L.n : G;
  p.b1 = p.b0 + L.n < G ? p.b0 + L.n : G;
  const int64_t blk = p.b1 - p.b0;
  p.pm_tl = a.p_max_assumed < L.cap ? a.p_max_assumed : L.cap;
  p.eig_only = a.method == 1;   // auto = matfun at every m (it wins at every m measured, tools/time_rows.py)
  p.rows = m * k;
  // Lazy sort: when the block's analysis is ONE plain launch that the sixteen-points-per-wavefront kernel will take -- it
  // ranks every tile's union by observation index itself, so the order inside a neighbour list means nothing to it -- the
  // observation index is built WITHOUT its per-cell sort (one kernel and one launch gap less in the preparation chain), and
  // only a redo of declined points (phase 1: the eigensolver kernel, which sums in list order) first puts the lists of
  // exactly those points into the order a sorted index gives.  The rule is evaluated from the call's arguments, so phase 0
  // and phase 1 of a step agree; the analysis call is checked against it (analyse_piece).
  p.lazy = mia::option(MIA_OPT_STEP_LAZY_SORT) != 0 && !p.exch && p.n_chunks == 1 && !p.eig_only && blk > 0 && P > 0 && L.cap <= 128 &&
           mia::cheb_tile_will_serve(m, k, p.pm_tl, L.cap, a.gamma, G, G, blk, p.ps);
  // Tile route (round 3): the localisation kernel emits tile-shaped lists (union + sqrt(rho) matrix per sixteen points), the
  // records are packed as scaled half pairs, and letkf_tile2_kernel analyses from both -- no per-point lists are written or
  // read.  Taken when the block's analysis is one plain launch of a shape the kernel covers; a tile whose union does not fit
  // its slots is counted in counters[1] and the caller repeats the step with MIA_STEP_NO_TILE_LISTS (scattered grids).
  // Declined points (phase 1) are redone from per-point lists built then, over the index this step left in its workspace.
  p.tl_th = nullptr;
  p.tl_tc = nullptr;
  // (gamma > 0: the RBF-kernelised filter on the same tile lists -- lketkf_tile_kernel reads Yb and d themselves, no records)
  p.tl_rbf = a.gamma > 0.0f;
  const int64_t ldo = p.exch ? L.nc : (p.no_gather ? blk : G);
  p.tl_route = mia::option(MIA_OPT_TILE_LISTS) != 0 && !(flags & MIA_STEP_NO_TILE_LISTS) && (p.n_chunks == 1 || p.exch) && !p.eig_only &&
               blk > 0 && P > 0 && L.ut <= 6 && mia::option(MIA_OPT_TILE) != 0 &&
               (p.tl_rbf ? mia::lketkf_tile_covers(m, k, p.pm_tl, p.extra, G, ldo, blk, P) && mia::cheb_primal_table(p.ps, &p.tl_th, &p.tl_tc)
                         : mia::option(MIA_OPT_TILE_SPLIT) != 0 && mia::tile2_covers(m, k, p.pm_tl, p.extra, G, ldo, blk) &&
                               mia::tile2_records_addressable(k, P) && mia::cheb_dual_table(p.ps, &p.tl_th, &p.tl_tc));
  p.tl_bucket = p.tl_route && mia::option(MIA_OPT_BUCKET_INDEX) != 0 && !(flags & MIA_STEP_SCAN_INDEX);
  // geometry epoch: the tile lists this workspace holds are used again (the caller vouches for unchanged coordinates, radii,
  // eps and block); only the split records are rebuilt.  Nothing to clear after the analysis: no index was built
  // ... and the library checks what it can: a stamp of what this workspace's lists were built for (route, format, block, radii,
  // eps, coordinate groups, sizes), kept on the host per workspace.  A step that asks for reuse with anything else -- an option or
  // attribute changed in between, another kernel family -- silently rebuilds instead of analysing from stale memory.
  // Fused localisation (letkf_tile2f.hip): the analysis wavefronts build their tiles' lists themselves over the bucket index -- no
  // list kernel, no lists in memory (the workspace's stamp says so: route 0).  Not when the caller declares a geometry epoch: the
  // lists are what an epoch keeps.
  p.want_fused = p.tl_route && p.tl_bucket && !p.tl_rbf && !(flags & (MIA_STEP_REUSE_LISTS | MIA_STEP_KEEP_LISTS)) &&
                 mia::option(MIA_OPT_TILE_FUSED) != 0 && mia::tile2f_covers(m, k, L.ut, a.n_coord);
  GeomStamp& stamp = p.stamp;
  memset(&stamp, 0, sizeof stamp);
  stamp.route = (p.tl_route && !p.want_fused) ? (p.tl_rbf ? 2 : 1) : 0;
  stamp.ut = L.ut; stamp.bucket = p.tl_bucket ? 1 : 0; stamp.n_coord = a.n_coord; stamp.n_r = a.n_r;
  stamp.G = G; stamp.P = P; stamp.rank = p.rank; stamp.world = p.world; stamp.k = k; stamp.eps = a.gc_eps;
  for (int i = 0; i < a.n_r; ++i) stamp.rc[i] = a.gc_c[i];
  for (int i = 0; i < a.n_coord; ++i) stamp.cg[i] = a.coord_group[i];
  for (int i = 0; i < a.n_coord; ++i) stamp.per[i] = p.period ? p.period[i] : 0.0;
  p.base = (char*)a.ws;
  p.rec = (float*)(p.base + L.rec);
  p.cnt = (int32_t*)(p.base + L.cnt);
  p.idx = (int32_t*)(p.base + L.idx);
  p.w = (double*)(p.base + L.w);
  p.done = (int32_t*)(p.base + L.done);
  p.gath_stride = mia::align_up(L.send_bytes * p.world, 256);
  p.done_ints = (size_t)p.n_chunks * 64 * mia::kSlotStride;
  // exchange route: the redo counters live in the trailer of the last piece and travel with its all-gather
  p.ctr = p.exch ? (int32_t*)(p.base + L.bufs + L.chunk_bytes * (p.n_chunks - 1) + (size_t)p.rows * L.nc * sizeof(float)) : a.counters;
  // a step in flight whose analysis is ONE plain launch (stage 2 after the host-side wait): the launch carries its completion
  // (and timing) events in its own dispatch packet
  p.carried = st.stage == 2 && a.phase == 0 && !p.exch && !p.peer && p.n_chunks == 1 && !p.eig_only && (flags & kStepPrepDone) &&
              (!a.time_start_event == !a.time_stop_event);
  return MIA_OK;
}

// The step's decision about its workspace (lists reused? which count array? localised in the kernel?): taken once per step, where its
// preparation is enqueued (`take`), read by the analysis stage from the step's state and by a redo call from what the table still
// knows; then the parts of the plan that follow from it.
static int step_decide(const mia_step_args_t& a, bool take, StepState* st, StepPlan* plan) {
  StepPlan& p = *plan;
  StepDecision& D = st->dec;
  if (take) {
    D.reuse = geom_reuse_decision(a.ws, p.stamp, p.tl_route && (p.flags & MIA_STEP_REUSE_LISTS) != 0, true);
    count_array_decision(a.ws, true, p.tl_bucket && !D.reuse, p.want_fused && !D.reuse, &D.cnt_use, &D.fused, &D.must_clear);
    D.set = true;
  } else if (!D.set) {      // (a redo of declined points, phase 1: a call of its own -- what the table still knows)
    D.reuse = geom_reuse_decision(a.ws, p.stamp, false, false);
    count_array_decision(a.ws, false, false, false, &D.cnt_use, &D.fused, &D.must_clear);
  }
  p.tl_reuse = D.reuse; p.tl_fused = D.fused; p.cnt_must_clear = D.must_clear;
  // (the analysis launch puts the OTHER per-cell count array and the build's error word back to zero, see Tile2Params / GeomEntry)
  p.tl_hk = mia::Tile2Housekeeping{nullptr, nullptr, nullptr, nullptr};
  p.tl_counts = nullptr;
  p.hk = nullptr;
  if (p.tl_bucket && !p.tl_reuse) {
    const mia::IndexLayout IL = mia::index_layout(p.base + p.L.loc, a.P, a.n_coord);
    p.tl_counts = D.cnt_use ? IL.start : IL.cursor;
    p.tl_hk = mia::Tile2Housekeeping{D.cnt_use ? IL.cursor : IL.start, &IL.hdr->ncell, &IL.hdr->err, nullptr};
    p.hk = &p.tl_hk;
  }
  p.tl_hk.err_out = p.ctr + 3;
  p.loc = nullptr;
  if (p.tl_fused) {
    const int rc = mia::make_scan_params(&p.tl_loc.scan, a.grid_xyz, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, a.gc_eps, p.base + p.L.loc,
                                         MIA_TAPER_GC, true);
    if (rc != MIA_OK) return rc;
    p.tl_loc.scan.start = p.tl_counts;
    p.tl_loc.stats = p.ctr;
    p.tl_loc.longest_bound = p.pm_tl;
    p.tl_loc.periodic = p.period ? 1 : 0;
    p.loc = &p.tl_loc;
  }
  // counters[0..3] = {longest list, truncated lists, declined points, error bits} of this rank; [4..7] = max over ranks.
  // They, the trailer copy and the segment slots are cleared by the first index kernel when it runs
  // (every fill launch of its own costs ~5-8 us of the ~100 us this phase takes)
  p.zero_in_kernel = a.P > 0 && p.b1 > p.b0 && !p.tl_reuse;
  return MIA_OK;
}

// prepare (phase 0, stage 1): clears, then records / index / lists on the preparation stream, then the events that order the
// analysis and the exchange stream behind it
static int step_prepare(const mia_step_args_t& a, const StepPlan& p, StepState* st) {
  const StepLayout& L = p.L;
  char* base = p.base;
  const hipStream_t ps = p.ps;
  const int flags = p.flags;
  const bool have_block = p.b1 > p.b0;
  int rc = MIA_OK;
  if (!p.zero_in_kernel) {
    MIA_HIP_TRY(hipMemsetAsync(a.counters, 0, 8 * sizeof(int32_t), ps));
    if (p.exch) {
      MIA_HIP_TRY(hipMemsetAsync(p.ctr, 0, 4 * sizeof(int32_t), ps));
      MIA_HIP_TRY(hipMemsetAsync(p.done, 0, p.done_ints * sizeof(int32_t), ps));
    }
  }
  const mia::ZeroJob zj{{a.counters, p.exch ? p.ctr : nullptr, p.exch ? p.done : nullptr}, {8, p.exch ? 4 : 0, p.exch ? (int64_t)p.done_ints : 0}};
  const mia::ZeroJob* zero = p.zero_in_kernel ? &zj : nullptr;
  if (have_block && p.tl_reuse) {
    if (!p.tl_rbf) {
      rc = mia::split_pack_launch(a.Yb, a.d, a.k, a.P, base + L.hrec, ps);
      if (rc != MIA_OK) return rc;
    }
  } else if (have_block && p.tl_route) {
    // bucket index: one kernel over the cell grid this workspace already holds (validated per observation); the first step on a
    // workspace, or one sent back by error bit 8, runs the bounding-box kernel first
    // (the split records ride in the bucket kernel -- small, and no LDS of its own -- rather than in the tile-list kernel, whose
    //  occupancy the packing's 10 KB of LDS per workgroup would cap)
    const mia::SplitPackJob sj{a.Yb, a.d, (unsigned char*)(base + L.hrec), a.k};
    if (p.tl_bucket)
      rc = mia::index_bucket_build_impl(a.obs_xyz, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, base + L.loc, L.loc_bytes, ps, zero,
                                        !(flags & MIA_STEP_WS_CLEAN) || (flags & MIA_STEP_FRESH_BOX) || p.cnt_must_clear,
                                        p.tl_rbf ? nullptr : &sj, p.tl_counts, p.period);
    else {
      const bool arrays_clean = count_arrays_clean_for_scan(a.ws);      // (a scan-based build counts in array 0)
      rc = mia::index_build_impl(a.obs_xyz, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, base + L.loc, L.loc_bytes, ps, nullptr, zero,
                                 (flags & MIA_STEP_WS_CLEAN) != 0 && arrays_clean, false, p.period);
    }
    if (rc != MIA_OK) return rc;
    if (!p.tl_fused) {
      rc = mia::tile_lists_launch(a.grid_xyz, p.b0, p.b1 - p.b0, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, a.gc_eps, MIA_TAPER_GC, L.ut,
                                  base + L.tl, p.ctr, base + L.loc, ps, (p.tl_bucket || p.tl_rbf) ? nullptr : &sj, p.tl_bucket, p.tl_counts,
                                  p.period);
      if (rc != MIA_OK) return rc;
    }
  } else if (have_block) {
    // the record packing rides inside the first index kernel too (independent work, no launch of its own)
    const mia::PackJob job{a.Yb, a.d, p.rec, a.k, (a.k + 1 + 3) / 4 * 4};
    rc = mia::localize_impl(a.grid_xyz, p.b0, p.b1, a.obs_xyz, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, a.gc_eps, L.cap, p.cnt, p.idx, p.w,
                            p.ctr, base + L.loc, L.loc_bytes, ps, a.P > 0 ? &job : nullptr, true, zero, MIA_TAPER_GC,
                            (flags & MIA_STEP_WS_CLEAN) != 0 && count_arrays_clean_for_scan(a.ws), !p.lazy, p.period);
    if (rc != MIA_OK) return rc;
  }
  if (ps != p.s) {   // the analysis stream starts once the preparation stream has produced records and lists
    rc = prep_event(&st->pe);
    if (rc != MIA_OK) return rc;
    MIA_HIP_TRY(hipEventRecord(st->pe, ps));
  }
  if (p.exch) MIA_HIP_TRY(hipEventRecord(a.comm->ev[mia::kMaxChunks], ps));
  return MIA_OK;
}

// piece c of the block: grid points [c0, c1), written to dst (its send buffer on the exchange route, else the result) with leading
// dimension ldo from column o0; the piece's slices of the per-point lists and flags
struct StepPiece {
  int c;
  int64_t c0, c1, ldo, o0;
  float* dst;
  int32_t *cnt, *idx, *flags;
  double* w;
};
static StepPiece step_piece(const mia_step_args_t& a, const StepPlan& p, int c) {
  const StepLayout& L = p.L;
  StepPiece q;
  q.c = c;
  q.c0 = p.b0 + c * L.nc < p.b1 ? p.b0 + c * L.nc : p.b1;
  q.c1 = q.c0 + L.nc < p.b1 ? q.c0 + L.nc : p.b1;
  q.dst = p.exch ? (float*)(p.base + L.bufs + L.chunk_bytes * c) : a.Xa;
  q.ldo = p.exch ? L.nc : (p.no_gather ? p.b1 - p.b0 : a.G);
  q.o0 = p.exch ? 0 : (p.no_gather ? q.c0 - p.b0 : q.c0);
  q.cnt = p.cnt + (q.c0 - p.b0);
  q.idx = p.idx + (size_t)(q.c0 - p.b0) * L.cap;
  q.w = p.w + (size_t)(q.c0 - p.b0) * L.cap;
  q.flags = a.flags + (q.c0 - p.b0);
  return q;
}

// exchange of a piece: the exchange stream waits for the piece (its segment of a segmented launch, else an event on the analysis
// stream -- ordered: false where an earlier piece's wait already covers this one), all-gather, placement into the result
static int exchange_piece(const mia_step_args_t& a, const StepPlan& p, const StepPiece& q, bool segmented, bool ordered) {
  const StepLayout& L = p.L;
  mia_comm* comm = a.comm;
  const hipStream_t cs = p.cs;
  float* gath = (float*)(p.base + L.gath + p.gath_stride * q.c);
  int rc = MIA_OK;
  if (segmented) {
    if (q.c1 > q.c0) {
      rc = mia::segment_wait_launch(p.done + (size_t)q.c * 64 * mia::kSlotStride, (int)(q.c1 - q.c0), p.ctr + 3, cs);
      if (rc != MIA_OK) return rc;
    }
  } else if (ordered) {
    MIA_HIP_TRY(hipEventRecord(comm->ev[q.c], p.s));
    MIA_HIP_TRY(hipStreamWaitEvent(cs, comm->ev[q.c], 0));
  }
  rc = mia::comm_allgather(comm, q.dst, gath, L.send_bytes, cs);
  if (rc != MIA_OK) return rc;
  // With steps in flight (MIA_STEP_NO_JOIN) and a placement stream, the copy of the gathered piece into the result
  // leaves the exchange stream: the next step's all-gather need not wait for 2 x world x piece bytes of HBM traffic
  hipStream_t xs = cs;
  if (comm->place_stream && (p.flags & MIA_STEP_NO_JOIN)) {
    xs = comm->place_stream;
    MIA_HIP_TRY(hipEventRecord(comm->evp[q.c], cs));
    MIA_HIP_TRY(hipStreamWaitEvent(xs, comm->evp[q.c], 0));
  }
  int32_t* ctr_out = (a.phase == 0 && q.c == p.n_chunks - 1) ? a.counters : nullptr;
  return mia::place_chunk_launch(gath, a.Xa, a.G, L.n, (int64_t)q.c * L.nc, L.nc, p.rows, p.world, L.send_bytes / sizeof(float), ctr_out, p.rank, xs);
}

// the analysis of one piece as a launch of its own: tile kernels, matfun kernel, else the eigensolver entry
static int analyse_piece(const mia_step_args_t& a, const StepPlan& p, StepState* st, const StepPiece& q) {
  const StepLayout& L = p.L;
  const hipEvent_t t_start = (hipEvent_t)a.time_start_event, t_stop = (hipEvent_t)a.time_stop_event;
  int rc = MIA_ERR_UNSUPPORTED;
  if (!p.eig_only) {
    // a step in flight whose analysis is one plain launch: the launch carries its completion event itself
    hipEvent_t kstop = nullptr;
    if (p.carried) {          // (a timed step: the dispatch's own start / stop times, no marker packets either)
      kstop = t_stop;
      if (!kstop) {
        rc = prep_event(&kstop);
        if (rc != MIA_OK) return rc;
      }
      mia::launch_stop_event() = kstop;
      mia::launch_start_event() = t_start;
    }
    const unsigned long long tiles_before = mia::tile_launch_count();
    if (p.tl_route && p.tl_rbf)
      rc = mia::lketkf_tile_launch(a.X, a.G, a.m, a.k, q.c0, q.c1 - q.c0, a.Yb, a.d, a.P, p.base + L.tl, L.ut, a.inf_factor, a.gamma, q.dst, q.ldo,
                                   q.o0, q.flags, p.ctr + 2, mia::option(MIA_OPT_CHEB_DMAX), p.tl_th, p.tl_tc, p.s, 0, 0, p.hk);
    else if (p.tl_route)
      rc = mia::tile2_analysis_launch(a.X, a.G, a.m, a.k, q.c0, q.c1 - q.c0, p.base + L.hrec, a.P, p.base + L.tl, L.ut, a.inf_factor, q.dst, q.ldo,
                                      q.o0, q.flags, p.ctr + 2, mia::option(MIA_OPT_CHEB_DMAX), p.tl_th, p.tl_tc, p.s, 0, 0, p.hk, p.loc);
    else
      rc = mia_letkf_analysis_matfun_f32(a.X, a.G, a.m, a.k, q.c0, q.c1, p.rec, a.P, q.cnt, q.idx, q.w, L.cap, a.p_max_assumed, a.inf_factor,
                                         a.gamma, q.dst, q.ldo, q.o0, q.flags, p.ctr + 2, a.stream);
    // (an unsorted index is only right for the kernel the rule of the plan predicted; the tile route has no other kernel)
    if ((p.lazy || p.tl_route) && (rc != MIA_OK || mia::tile_launch_count() == tiles_before)) {
      mia::launch_stop_event() = nullptr;
      mia::launch_start_event() = nullptr;
      return rc != MIA_OK ? rc : MIA_ERR_UNSUPPORTED;
    }
    if (kstop) {
      if (mia::launch_stop_event() == nullptr) {
        st->kdone = kstop;      // (taken by the tile kernel's launch)
      } else if (t_start) {      // another kernel served the shape: ordinary markers around it (late start: after the fact)
        MIA_HIP_TRY(hipEventRecord(t_start, p.s));
        MIA_HIP_TRY(hipEventRecord(t_stop, p.s));
      }
      mia::launch_stop_event() = nullptr;
      mia::launch_start_event() = nullptr;
    }
  }
  if (rc == MIA_ERR_UNSUPPORTED)
    rc = mia_letkf_analysis_packed_f32(a.X, a.G, a.m, a.k, q.c0, q.c1, p.rec, a.P, q.cnt, q.idx, q.w, L.cap, a.p_max_assumed, a.inf_factor,
                                       a.gamma, q.dst, q.ldo, q.o0, nullptr, q.flags, a.stream);
  return rc;
}

// analyse (phase 0, stage 2): the waits for the preparation, then the block in one launch over its pieces where a kernel can, else
// piece by piece, each piece exchanged as it completes
static int step_analyse(const mia_step_args_t& a, const StepPlan& p, StepState* st) {
  const StepLayout& L = p.L;
  const hipStream_t s = p.s;
  const bool have_block = p.b1 > p.b0;
  int rc = MIA_OK;
  if (p.ps != s && !(p.flags & kStepPrepDone)) MIA_HIP_TRY(hipStreamWaitEvent(s, st->pe, 0));
  // the side stream starts once the lists exist (and the slots it polls have been cleared)
  if (p.exch) MIA_HIP_TRY(hipStreamWaitEvent(p.cs, a.comm->ev[mia::kMaxChunks], 0));
  if (a.time_start_event && !p.carried) MIA_HIP_TRY(hipEventRecord((hipEvent_t)a.time_start_event, s));   // (after the wait for the lists: kernel time only)
  float* bufs = (float*)(p.base + L.bufs);
  const int64_t seg_stride = (int64_t)(L.chunk_bytes / sizeof(float));
  // tile route with several pieces: ONE launch over the block, every tile writes into its piece's buffer; the pieces are
  // exchanged once it has finished (the kernel is a fraction of one piece's all-gather: nothing to overlap inside it)
  bool tl_block = false;
  if (p.tl_route && p.n_chunks > 1 && have_block) {
    rc = p.tl_rbf ? mia::lketkf_tile_launch(a.X, a.G, a.m, a.k, p.b0, p.b1 - p.b0, a.Yb, a.d, a.P, p.base + L.tl, L.ut, a.inf_factor, a.gamma, bufs,
                                            L.nc, 0, a.flags, p.ctr + 2, mia::option(MIA_OPT_CHEB_DMAX), p.tl_th, p.tl_tc, s, (int)L.nc, seg_stride,
                                            p.hk)
                  : mia::tile2_analysis_launch(a.X, a.G, a.m, a.k, p.b0, p.b1 - p.b0, p.base + L.hrec, a.P, p.base + L.tl, L.ut, a.inf_factor, bufs,
                                               L.nc, 0, a.flags, p.ctr + 2, mia::option(MIA_OPT_CHEB_DMAX), p.tl_th, p.tl_tc, s, (int)L.nc,
                                               seg_stride, p.hk, p.loc);
    if (rc != MIA_OK) return rc;
    tl_block = true;
  }
  // one launch over the whole block whose segments are exchanged as they complete (no kernel boundary, no
  // event between the pieces: a 1e5-point block in 4 launches costs 292 us instead of 245 us on MI355X)
  bool segmented = false;
  if (!tl_block && p.exch && p.n_chunks > 1 && !p.eig_only && have_block && p.signal_mode) {
    rc = mia::cheb_analysis_launch(a.X, a.G, a.m, a.k, p.b0, p.b1 - p.b0, p.rec, p.cnt, p.idx, p.w, L.cap, p.pm_tl, a.inf_factor,
                                   a.gamma > 0.0f ? 1 : 0, a.gamma, bufs, L.nc, 0, a.flags, p.ctr + 2, nullptr, nullptr, s, (int)L.nc, seg_stride,
                                   p.done);
    if (rc == MIA_OK) segmented = true;
    else if (rc != MIA_ERR_UNSUPPORTED) return rc;
  }
  for (int c = 0; c < p.n_chunks; ++c) {
    const StepPiece q = step_piece(a, p, c);
    if (q.c1 > q.c0 && !segmented && !tl_block) {
      rc = analyse_piece(a, p, st, q);
      if (rc != MIA_OK) return rc;
    }
    if (p.exch) {      // (the tile route's one launch: the first piece's wait covers all of them)
      rc = exchange_piece(a, p, q, segmented, !tl_block || c == 0);
      if (rc != MIA_OK) return rc;
    }
  }
  return MIA_OK;
}

// redo (phase 1): the points the step's kernel declined, piece by piece, with the eigensolver kernel over per-point lists
static int step_redo(const mia_step_args_t& a, const StepPlan& p) {
  const StepLayout& L = p.L;
  const hipStream_t s = p.s;
  int rc = MIA_OK;
  for (int c = 0; c < p.n_chunks; ++c) {
    const StepPiece q = step_piece(a, p, c);
    if (q.c1 > q.c0) {
      if (p.tl_route) {
        // declined points of the tile route: float32 records and per-point lists are built now (the step's index is still in
        // its workspace, unsorted: the flagged points' lists are put into sorted-index order as on the lazy route)
        if (c == 0) {
          rc = mia_letkf_pack_obs_f32(a.Yb, a.d, a.k, a.P, p.rec, a.stream);
          if (rc != MIA_OK) return rc;
          if (p.tl_bucket) {      // (the buckets are no scan-based index: build one, unsorted like the lazy route's)
            (void)count_arrays_clean_for_scan(a.ws);      // (cleared whole below; the scan counts in array 0)
            rc = mia::index_build_impl(a.obs_xyz, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, p.base + L.loc, L.loc_bytes, s, nullptr, nullptr,
                                       false, false, p.period);
            if (rc != MIA_OK) return rc;
          }
        }
        rc = mia::localize_lists_impl(a.grid_xyz, q.c0, q.c1, a.P, a.n_coord, a.coord_group, a.gc_c, a.n_r, a.gc_eps, L.cap, q.cnt, q.idx, q.w,
                                      (int32_t*)(p.base + L.scratch), p.base + L.loc, s, nullptr, MIA_TAPER_GC, p.period);
        if (rc != MIA_OK) return rc;
      }
      if (p.tl_route || p.lazy) {      // (the lists of the declined points into sorted-index order, see the plan)
        rc = mia::sort_flagged_lists(q.flags, q.cnt, q.idx, q.w, q.c1 - q.c0, (int)L.cap, p.base + L.loc, a.P, a.n_coord, s);
        if (rc != MIA_OK) return rc;
      }
      rc = mia_letkf_analysis_retry_f32(a.X, a.G, a.m, a.k, q.c0, q.c1, p.rec, a.P, q.cnt, q.idx, q.w, L.cap, a.p_max_assumed, a.inf_factor,
                                        a.gamma, q.dst, q.ldo, q.o0, q.flags, a.stream);
      if (rc != MIA_OK) return rc;
    }
    if (p.exch) {
      rc = exchange_piece(a, p, q, false, true);
      if (rc != MIA_OK) return rc;
    }
  }
  return MIA_OK;
}

static int step_impl(const mia_step_args_t& a, StepState* st) {
  const bool do1 = st->stage != 2, do2 = st->stage != 1;
  if (st->stage == 2) st->kdone = nullptr;
  StepPlan p;
  int rc = step_plan(a, *st, &p);
  if (rc != MIA_OK) return rc;
  rc = step_decide(a, a.phase == 0 && do1, st, &p);
  if (rc != MIA_OK) return rc;
  (void)hipGetLastError();
  if (p.exch || p.peer) {
    rc = mia::comm_events(a.comm);
    if (rc != MIA_OK) return rc;
  }
  if (p.peer && do1) {      // "my buffer of this slot may be overwritten": told to every peer before anything else of the step
    rc = mia::peer_begin(a.comm, p.peer_slot, p.ps, &st->seq);
    if (rc != MIA_OK) return rc;
  }
  if (a.phase == 0 && do1) {
    rc = step_prepare(a, p, st);
    if (rc != MIA_OK) return rc;
  }
  if (!do2) return MIA_OK;
  rc = a.phase == 0 ? step_analyse(a, p, st) : step_redo(a, p);
  if (rc != MIA_OK) return rc;
  if (p.peer) {      // block analysed (stream s) -> exchange stream: wait, push, signal, wait (see "Direct exchange", step_comm.hip)
    MIA_HIP_TRY(hipEventRecord(a.comm->ev[0], p.s));
    MIA_HIP_TRY(hipStreamWaitEvent(p.cs, a.comm->ev[0], 0));
    rc = mia::peer_finish(a.comm, p.peer_slot, st->seq, a.G, p.b0, p.b1, p.rows, a.counters, p.cs);
    if (rc != MIA_OK) return rc;
  }
  if (a.phase == 0 && a.time_stop_event && !p.carried) MIA_HIP_TRY(hipEventRecord((hipEvent_t)a.time_stop_event, p.s));
  // (without the exchange route counters[4..7] stay zero: the rank's own [0..3] are the whole story)
  if ((p.exch || p.peer) && !(p.flags & MIA_STEP_NO_JOIN)) {   // the caller's stream continues after the exchange
    MIA_HIP_TRY(hipEventRecord(a.comm->ev[mia::kMaxChunks + 1], p.cs));
    MIA_HIP_TRY(hipStreamWaitEvent(p.s, a.comm->ev[mia::kMaxChunks + 1], 0));
  }
  return MIA_OK;
}

// The positional entries fill one block, once, here at the ABI boundary (the header gives their parameters the same names
// everywhere, so the block is filled by NAME: no second positional list to transpose).  The coordinate-group and radius tables are
// copied into the block: their sizes are checked first.  The macro RETURNS from the entry -- MIA_ERR_NULL for a NULL coord_group or
// gc_c, MIA_ERR_SIZE for n_coord or n_r outside the block's tables -- before it declares the block.  Checking these sizes ahead of
// the copies changes which code a call with TWO faults reports: a NULL X together with n_coord 0 was MIA_ERR_NULL (pointers were
// looked at first) and is MIA_ERR_SIZE now; every single fault reports what it always did (tests/golden/step_call_trace.txt).
#define MIA_STEP_BLOCK_FROM_PARAMETERS(a)                                                                                      \
  if (!coord_group || !gc_c) return MIA_ERR_NULL;                                                                              \
  if (!step_tables_fit(n_coord, n_r)) return MIA_ERR_SIZE;                                                                     \
  mia_step_args_t a;                                                                                                           \
  memset(&a, 0, sizeof a);                                                                                                     \
  a.X = X; a.G = G; a.m = m; a.k = k; a.Yb = Yb; a.d = d; a.P = P; a.grid_xyz = grid_xyz; a.obs_xyz = obs_xyz;                 \
  a.n_coord = n_coord; a.n_r = n_r; a.gc_eps = gc_eps; a.inf_factor = inf_factor; a.gamma = gamma; a.method = method;          \
  for (int c_ = 0; c_ < n_coord; ++c_) a.coord_group[c_] = coord_group[c_];                                                    \
  for (int r_ = 0; r_ < n_r; ++r_) a.gc_c[r_] = gc_c[r_];                                                                      \
  a.p_max_assumed = p_max_assumed; a.comm = comm; a.n_chunks = n_chunks; a.phase = phase; a.Xa = Xa; a.flags = flags;          \
  a.counters = counters; a.ws = ws; a.ws_bytes = ws_bytes; a.stream = stream; a.comm_stream = comm_stream;                     \
  a.prep_stream = prep_stream; a.step_flags = step_flags

// the whole step at once on the caller's thread, timed by the one-shot hook if one was set (mia_letkf_step_timing_events)
static int step_now(mia_step_args_t* a) {
  a->time_start_event = (void*)t_time_start;
  a->time_stop_event = (void*)t_time_stop;
  t_time_start = t_time_stop = nullptr;
  StepState st;
  st.flags = a->step_flags;
  return step_impl(*a, &st);
}

extern "C" int mia_letkf_sharded_step_streams_f32(const float* X, int64_t G, int m, int k,
                                                  const float* Yb, const float* d, int64_t P,
                                                  const double* grid_xyz, const double* obs_xyz, int n_coord,
                                                  const int32_t* coord_group, const double* gc_c, int n_r, double gc_eps,
                                                  float inf_factor, float gamma, int method, int p_max_assumed,
                                                  mia_comm_t* comm, int n_chunks, int phase,
                                                  float* Xa, int32_t* flags, int32_t* counters,
                                                  void* ws, size_t ws_bytes, void* stream, void* comm_stream,
                                                  void* prep_stream, int step_flags) {
  MIA_STEP_BLOCK_FROM_PARAMETERS(a);      // (may return MIA_ERR_NULL / MIA_ERR_SIZE)
  return step_now(&a);
}

extern "C" int mia_letkf_sharded_step_periodic_f32(const float* X, int64_t G, int m, int k, const float* Yb, const float* d, int64_t P,
                                                   const double* grid_xyz, const double* obs_xyz, int n_coord, const int32_t* coord_group,
                                                   const double* period, const double* gc_c, int n_r, double gc_eps, float inf_factor,
                                                   float gamma, int method, int p_max_assumed, mia_comm_t* comm, int n_chunks, int phase,
                                                   float* Xa, int32_t* flags, int32_t* counters, void* ws, size_t ws_bytes, void* stream,
                                                   void* comm_stream, void* prep_stream, int step_flags) {
  if (!period) return MIA_ERR_NULL;
  MIA_STEP_BLOCK_FROM_PARAMETERS(a);      // (may return MIA_ERR_NULL / MIA_ERR_SIZE)
  for (int c = 0; c < n_coord; ++c) a.period[c] = period[c];
  return step_now(&a);
}

// ---------------------------------------------------------------------------------------------------------------------
// Launch threads.  One step is ~9 kernel launches, a copy and half a dozen event operations: ~100 us of HIP runtime calls
// on the calling thread -- more than a step's GPU time since the sixteen-point kernel (host-bound pipeline: 0.104 ms per
// step with the GPU ~75 % busy, whichever thread made the calls).  mia_letkf_step_submit hands the step to TWO worker threads
// of the library (no throughput gain measured at N = 1, where the analysis stream is the bound; the caller's submit() drops
// from 80 to 24 us): thread A enqueues what goes to the preparation stream (stage 1 of step_impl), thread B what follows
// (analysis, exchange, read-back), each in submission order -- every stream sees its work in step order, every rank enqueues
// its exchanges in the same order -- so that the host time per step is the larger half, not the sum, and overlaps the
// caller's own per-step work.  mia_letkf_step_join waits until the job's launches are enqueued (not until the GPU has run
// them: that is what the read-back event is for).
namespace {
struct StepJob {
  mia_step_args_t a;               // the step, as the caller handed it in
  StepState st;                    // what stage 1 leaves for stage 2
  int opts[MIA_OPT_COUNT_];        // the route options as they stood when the caller submitted the step
  long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // host time stamps (ns): submitted, A begins, A done, B has it, its preparation seen done,
                                                   // analysis enqueued, read-back enqueued (mia_debug_step_trace)
  int device = 0;
  int rc = 0;
  bool done = false;
  int run(int stage) {
    struct Scope { Scope(const int* o) { mia::option_override(o); } ~Scope() { mia::option_override(nullptr); } } scope(opts);
    st.stage = stage;
    return step_impl(a, &st);
  }
};
struct LaunchThreads {
  std::thread ta, tb;
  std::mutex mu;
  std::condition_variable cv_a, cv_b, cv_done;
  std::deque<StepJob*> qa, qb;
  int device = 0;
  bool stop = false, started = false;
  int busy = 0;          // jobs handed in and not yet finished by thread B
  std::atomic<long long> ns_a{0}, ns_b{0}, n_jobs{0};     // host time spent enqueueing (mia_letkf_step_launch_stats)
  // entries of the two queues, readable without the lock: a thread whose queue has run dry polls its counter for kSpinUs before
  // it sleeps on the condition variable.  Waking a sleeping thread costs 30-60 us on this host (a step's whole GPU time): the
  // first analysis launch of a burst of steps came 80 us after the first preparation kernel had finished
  // (profiles/r05_timeline_steps20.txt); a caller that submits its next step within kSpinUs finds both threads awake
  std::atomic<int> na{0}, nb_q{0};
  static constexpr int kTraceN = 256;
  std::array<long long, 8> trace[kTraceN];      // the stamps of the last kTraceN steps (mia_debug_step_trace)
  unsigned long long trace_n = 0;
  static long long now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  static constexpr long long kSpinUs = 400;
  void spin_for(const std::atomic<int>& n) {
    if (n.load(std::memory_order_acquire) > 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      for (int i = 0; i < 64; ++i) {
        if (n.load(std::memory_order_acquire) > 0) return;
        __builtin_ia32_pause();
      }
      if (stop_flag.load(std::memory_order_relaxed)) return;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinUs) return;
    }
  }
  std::atomic<bool> stop_flag{false};
  static void relax(int n = 40) {
    for (int i = 0; i < n; ++i) __builtin_ia32_pause();      // 40: ~1 us
  }
  void run_a() {
    int cur_a = device;
    (void)hipSetDevice(device);
    for (;;) {
      StepJob* j;
      spin_for(na);
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_a.wait(lk, [&] { return stop || !qa.empty(); });
        if (qa.empty()) return;
        j = qa.front();
        qa.pop_front();
        --na;
      }
      if (j->device != cur_a) { (void)hipSetDevice(j->device); cur_a = j->device; }
      const auto ta0 = std::chrono::steady_clock::now();
      j->ts[1] = now_ns();
      const int rc = j->run(1);
      j->ts[2] = now_ns();
      ns_a += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - ta0).count();
      ++n_jobs;
      {
        std::lock_guard<std::mutex> lk(mu);
        j->rc = rc;
        qb.push_back(j);
        ++nb_q;
      }
      cv_b.notify_one();
    }
  }
  void run_b() {
    int cur_b = device;
    (void)hipSetDevice(device);
    for (;;) {
      StepJob* j;
      spin_for(nb_q);
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_b.wait(lk, [&] { return stop || !qb.empty(); });
        if (qb.empty()) return;
        j = qb.front();
        qb.pop_front();
        --nb_q;
      }
      if (j->device != cur_b) { (void)hipSetDevice(j->device); cur_b = j->device; }
      j->ts[3] = now_ns();
      int rc = j->rc;
      // Steps in flight: wait for the step's preparation HERE, on the host, and enqueue the analysis kernel with nothing in
      // front of it.  A stream-wait in the analysis queue is a barrier packet between every two analysis kernels (11-16 us
      // from the end of one to the start of the next, 6-7 without): 0.093 -> 0.088 ms per step once the chip has room for
      // the preparation beside the analysis kernel (it made no difference while the three-wave kernel filled it).  The
      // preparation runs two steps ahead, so the wait is short; query + yield rather than a spinning synchronise.
      if (rc == MIA_OK && j->st.pe && (j->st.flags & MIA_STEP_NO_JOIN) && mia::option(MIA_OPT_STEP_HOSTWAIT) != 0) {
        hipError_t q;
        while ((q = hipEventQuery(j->st.pe)) == hipErrorNotReady) relax();      // (a microsecond between two queries: the runtime's locks are
                                                                             //  the caller's and the other launch thread's too)
        if (q == hipSuccess) j->st.flags |= kStepPrepDone;
        else (void)hipGetLastError();         // (leave the ordering to the stream wait)
      }
      const auto tb0 = std::chrono::steady_clock::now();
      j->ts[4] = now_ns();
      if (rc == MIA_OK) rc = j->run(2);
      j->ts[5] = now_ns();
      if (rc == MIA_OK && j->a.host8) {
        // (the read-back waits for the kernel's own completion event when the launch carried one: no marker on the stream)
        if (j->st.kdone && j->a.after_stream == j->a.stream) rc = readback_after_event(j->a.counters, j->a.host8, j->st.kdone, j->a.on_stream, j->a.done_event);
        else rc = mia_letkf_step_readback(j->a.counters, j->a.host8, j->a.after_stream, j->a.on_stream, j->a.done_event);
      }
      j->rc = rc;
      ns_b += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tb0).count();
      j->ts[6] = now_ns();
      {
        std::lock_guard<std::mutex> lk(mu);
        trace[trace_n++ % kTraceN] = *reinterpret_cast<std::array<long long, 8>*>(j->ts);
        j->done = true; --busy;
      }
      cv_done.notify_all();
    }
  }
  ~LaunchThreads() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; stop_flag = true; }
    cv_a.notify_all();
    cv_b.notify_all();
    if (ta.joinable()) ta.join();
    if (tb.joinable()) tb.join();
  }
};
LaunchThreads g_launcher;
}  // namespace

static thread_local long long t_submit_entry = 0;      // (diagnostics: when the argument-block submission was entered, mia_debug_step_trace)
// hands a checked block to the launch threads: the one copy of the block a submitted step costs
static int step_submit(const mia_step_args_t& a, void** job_out) {
  if (!job_out) return MIA_ERR_NULL;
  if (!step_tables_fit(a.n_coord, a.n_r)) return MIA_ERR_SIZE;
  const double* period = nullptr;
  if (step_period(a, &period) != MIA_OK) return MIA_ERR_ARG;
  StepJob* j = new StepJob();
  j->a = a;
  j->st.flags = a.step_flags;
  mia::option_snapshot(j->opts);
  j->ts[0] = LaunchThreads::now_ns();
  j->ts[7] = t_submit_entry;            // (diagnostics: entry of the argument-block submission; 0 through the plain entry)
  t_submit_entry = 0;
  if (hipGetDevice(&j->device) != hipSuccess) { (void)hipGetLastError(); delete j; return MIA_ERR_UNSUPPORTED; }
  {
    std::lock_guard<std::mutex> lk(g_launcher.mu);
    if (!g_launcher.started) {
      g_launcher.device = j->device;
      g_launcher.started = true;
      g_launcher.ta = std::thread([] { g_launcher.run_a(); });
      g_launcher.tb = std::thread([] { g_launcher.run_b(); });
    }
    g_launcher.qa.push_back(j);
    ++g_launcher.na;
    ++g_launcher.busy;
  }
  g_launcher.cv_a.notify_one();
  *job_out = j;
  return MIA_OK;
}

extern "C" int mia_letkf_step_submit(const float* X, int64_t G, int m, int k, const float* Yb, const float* d, int64_t P,
                                     const double* grid_xyz, const double* obs_xyz, int n_coord, const int32_t* coord_group,
                                     const double* gc_c, int n_r, double gc_eps, float inf_factor, float gamma, int method,
                                     int p_max_assumed, mia_comm_t* comm, int n_chunks, int phase, float* Xa, int32_t* flags,
                                     int32_t* counters, void* ws, size_t ws_bytes, void* stream, void* comm_stream,
                                     void* prep_stream, int step_flags, int32_t* host8, void* after_stream, void* on_stream,
                                     void** done_event, void* time_start_event, void* time_stop_event, void** job_out) {
  if (!job_out) return MIA_ERR_NULL;
  MIA_STEP_BLOCK_FROM_PARAMETERS(a);      // (may return MIA_ERR_NULL / MIA_ERR_SIZE)
  a.host8 = host8; a.after_stream = after_stream; a.on_stream = on_stream; a.done_event = done_event;
  a.time_start_event = time_start_event; a.time_stop_event = time_stop_event;
  return step_submit(a, job_out);
}

extern "C" int mia_letkf_step_submit_args(const mia_step_args_t* a, void** job_out) {
  if (!a) return MIA_ERR_NULL;
  t_submit_entry = LaunchThreads::now_ns();
  if (a->in_event) {
    // (an idle caller stream has produced everything it ever will before this call: nothing to wait for -- no event, and no
    //  barrier packet in front of the preparation kernel)
    const hipError_t q = hipStreamQuery((hipStream_t)a->caller_stream);
    if (q != hipSuccess) {
      (void)hipGetLastError();
      const int rc = mia_stream_wait_stream(a->prep_stream, a->caller_stream, a->in_event);
      if (rc != MIA_OK) return rc;
    }
  }
  return step_submit(*a, job_out);
}

// One step taken at once on the caller's thread through the argument block: what mia_letkf_step_drain + the step call +
// mia_letkf_step_readback (+ mia_event_synchronize and a copy of the counters, when out8 is given) do, in one call.
extern "C" int mia_letkf_step_run_args(const mia_step_args_t* a, int32_t* out8) {
  if (!a || !a->done_event || !a->host8) return MIA_ERR_NULL;
  const double* period = nullptr;
  if (step_period(*a, &period) != MIA_OK) return MIA_ERR_ARG;
  int rc = mia_letkf_step_drain();       // (a synchronous step must not overtake queued ones)
  if (rc != MIA_OK) return rc;
  if (a->in_event) {
    rc = mia_stream_wait_stream(a->prep_stream ? a->prep_stream : a->stream, a->caller_stream, a->in_event);
    if (rc != MIA_OK) return rc;
  }
  if ((a->time_start_event == nullptr) != (a->time_stop_event == nullptr)) return MIA_ERR_NULL;
  StepState st;
  st.flags = a->step_flags & ~MIA_STEP_NO_JOIN;
  rc = step_impl(*a, &st);
  if (rc != MIA_OK) return rc;
  rc = mia_letkf_step_readback(a->counters, a->host8, a->after_stream, a->on_stream, a->done_event);
  if (rc != MIA_OK || !out8) return rc;
  MIA_HIP_TRY(hipEventSynchronize((hipEvent_t)*a->done_event));
  for (int i = 0; i < 8; ++i) out8[i] = a->host8[i];
  return MIA_OK;
}

extern "C" int mia_letkf_step_collect(void* job, void** done_event, const int32_t* host8, void* consumer_stream, int consumer_stream_valid,
                                      int32_t* out8) {
  if (!job || !done_event || !host8 || !out8) return MIA_ERR_NULL;
  const int rc = mia_letkf_step_join(job);
  if (rc != MIA_OK) return rc;
  const hipEvent_t ev = (hipEvent_t)*done_event;      // (made by the step's read-back on the launch thread: read after the join)
  if (!ev) return MIA_ERR_NULL;
  MIA_HIP_TRY(hipEventSynchronize(ev));
  for (int i = 0; i < 8; ++i) out8[i] = host8[i];
  if (consumer_stream_valid) MIA_HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, ev, 0));
  return MIA_OK;
}

namespace {
std::mutex g_tev_mutex;
std::vector<hipEvent_t> g_tev_free;
}
extern "C" int mia_timing_event_acquire(void** event) {
  if (!event) return MIA_ERR_NULL;
  {
    std::lock_guard<std::mutex> lk(g_tev_mutex);
    if (!g_tev_free.empty()) { *event = (void*)g_tev_free.back(); g_tev_free.pop_back(); return MIA_OK; }
  }
  hipEvent_t e = nullptr;
  MIA_HIP_TRY(hipEventCreate(&e));
  *event = (void*)e;
  return MIA_OK;
}
extern "C" int mia_timing_event_release(void* event) {
  if (!event) return MIA_ERR_NULL;
  std::lock_guard<std::mutex> lk(g_tev_mutex);
  g_tev_free.push_back((hipEvent_t)event);
  return MIA_OK;
}
extern "C" int mia_timing_event_elapsed_ms(void* start_event, void* stop_event, float* ms) {
  if (!start_event || !stop_event || !ms) return MIA_ERR_NULL;
  MIA_HIP_TRY(hipEventSynchronize((hipEvent_t)stop_event));
  MIA_HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start_event, (hipEvent_t)stop_event));
  return MIA_OK;
}

// the host time stamps of the last steps handed to the launch threads, oldest first: 8 values per step (ns of the steady clock:
// submitted, thread A begins / has enqueued the preparation, thread B takes the step / has seen its preparation finished / has
// enqueued the analysis / the read-back, 0).  Returns the number of steps written (tools/step_trace.py)
extern "C" int mia_debug_step_trace(long long* out, int max_steps) {
  if (!out || max_steps <= 0) return 0;
  std::lock_guard<std::mutex> lk(g_launcher.mu);
  const unsigned long long n = g_launcher.trace_n;
  const int have = (int)(n < (unsigned long long)LaunchThreads::kTraceN ? n : LaunchThreads::kTraceN);
  const int take = have < max_steps ? have : max_steps;
  for (int i = 0; i < take; ++i) {
    const auto& t = g_launcher.trace[(n - take + i) % LaunchThreads::kTraceN];
    for (int q = 0; q < 8; ++q) out[8 * i + q] = t[q];
  }
  return take;
}

// host time the two launch threads have spent enqueueing so far (microseconds: preparation stage, analysis / exchange /
// read-back stage) and the number of steps: tells a pipeline that waits for its launches from one that waits for the GPU
extern "C" int mia_letkf_step_launch_stats(double* prep_us, double* rest_us, long long* steps) {
  if (!prep_us || !rest_us || !steps) return MIA_ERR_NULL;
  *prep_us = g_launcher.ns_a.load() * 1e-3;
  *rest_us = g_launcher.ns_b.load() * 1e-3;
  *steps = g_launcher.n_jobs.load();
  return MIA_OK;
}

// waits until the job's launches are enqueued; returns the step call's status and frees the job
extern "C" int mia_letkf_step_join(void* job) {
  if (!job) return MIA_ERR_NULL;
  StepJob* j = (StepJob*)job;
  std::unique_lock<std::mutex> lk(g_launcher.mu);
  g_launcher.cv_done.wait(lk, [&] { return j->done; });
  const int rc = j->rc;
  lk.unlock();
  delete j;
  return rc;
}

// waits until nothing is queued or running on the launch thread (before a synchronous call that must not overtake it)
extern "C" int mia_letkf_step_drain(void) {
  std::unique_lock<std::mutex> lk(g_launcher.mu);
  g_launcher.cv_done.wait(lk, [&] { return g_launcher.busy == 0; });
  return MIA_OK;
}
