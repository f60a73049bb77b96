// The step driver's call trace (tests/test_step_call_trace.py): a fixed list of scenarios run on ONE caller thread against the stub HIP
// runtime of hip_stub.cc with its call trace switched on.  Per scenario a header line ("# name"), then per C call the runtime calls
// it made (launches with kernel name, grid, block, LDS bytes, stream and events; event records / waits; asynchronous fills and copies;
// the communicator callbacks) followed by "= call rc".  Submitted steps are joined before their trace is printed, one at a time, so
// the launch threads' lines come in a fixed order.  Nothing here depends on addresses: the output is compared line for line with
// tests/golden/step_call_trace.txt.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include "mia_letkf.h"

extern "C" void mia_stub_trace_enable(int on);
extern "C" void mia_stub_trace_note(const char* text);
extern "C" void mia_stub_trace_flush(FILE* to);
extern "C" int hipMalloc(void**, size_t);
extern "C" int hipFree(void*);

static void* dmalloc(size_t n) { void* p = nullptr; if (hipMalloc(&p, n) != 0) abort(); return p; }
static void* stream(uintptr_t i) { return (void*)(0x1000 + 8 * i); }           // idle for the stub (bit 2 clear)
static void* busy_stream(uintptr_t i) { return (void*)(0x1004 + 8 * i); }      // the stub reports it busy (bit 2 set)
static void* const S = stream(0);       // analysis
static void* const CS = stream(1);      // exchange
static void* const PS = stream(2);      // preparation
static void* const RS = stream(3);      // read-back
static void* const XS = stream(4);      // placement

static void header(const char* name) { printf("# %s\n", name); }
static int done(const char* call, int rc) { mia_stub_trace_flush(stdout); printf("= %s %d\n", call, rc); return rc; }
// a submission's own line comes first and its runtime calls with the join's: the launch threads may already be at work when it returns
static int submitted_rc(const char* call, int rc) { printf("= %s %d\n", call, rc); return rc; }
static void opt(const char* name, int v) { if (mia_set_option(name, v) != MIA_OK) abort(); }

static int allgather_cb(void*, const void* send, void* recv, size_t bytes, void* s) {
  char line[96];
  snprintf(line, sizeof line, "allgather %zu stream %#lx", bytes, (unsigned long)(uintptr_t)s);
  mia_stub_trace_note(line);
  memcpy(recv, send, bytes);      // world 1
  return 0;
}
static int allreduce_cb(void*, int32_t*, int n, void* s) {
  char line[96];
  snprintf(line, sizeof line, "allreduce %d stream %#lx", n, (unsigned long)(uintptr_t)s);
  mia_stub_trace_note(line);
  return 0;
}

// one problem, its buffers and one step workspace; every field is an argument of the step
struct Rig {
  int64_t G = 4000, P = 2000;
  int m = 1, k = 40, n_coord = 1, n_r = 1, method = 0, hint = 20, chunks = 1, world = 1;
  float gamma = 0.0f;
  double rc[3] = {10.0, 5.0, 2.5}, per[3] = {0.0, 0.0, 0.0};
  int32_t cg[3] = {0, 0, 0};
  bool periodic_entry = false;
  mia_comm_t* comm = nullptr;
  void* prep = nullptr;
  float *X = nullptr, *Yb, *d, *Xa; double *grid, *obs; void* ws; size_t ws_bytes = 0; int32_t *counters, *flags, *host8;
  void *event = nullptr, *in_event = nullptr;

  int alloc() {
    X = (float*)dmalloc(sizeof(float) * m * k * G); Yb = (float*)dmalloc(sizeof(float) * k * (P + 1)); d = (float*)dmalloc(sizeof(float) * (P + 1));
    grid = (double*)dmalloc(sizeof(double) * G * n_coord); obs = (double*)dmalloc(sizeof(double) * (P + 1) * n_coord);
    for (int64_t g = 0; g < G * n_coord; ++g) grid[g] = (double)(g / n_coord);
    for (int64_t j = 0; j < P * n_coord; ++j) obs[j] = 2.0 * (double)(j / n_coord);
    const int rcb = mia_letkf_sharded_step_workspace_bytes(G, m, k, P, n_coord, world, chunks, hint, &ws_bytes);
    ws = dmalloc(ws_bytes);
    counters = (int32_t*)dmalloc(32); flags = (int32_t*)dmalloc(sizeof(int32_t) * G);
    Xa = (float*)dmalloc(sizeof(float) * m * k * G); host8 = (int32_t*)calloc(8, sizeof(int32_t));
    return rcb;
  }
  ~Rig() {
    if (!X) return;
    mia_letkf_step_workspace_release(ws);
    if (event) mia_event_destroy(event);
    if (in_event) mia_event_destroy(in_event);
    hipFree(X); hipFree(Yb); hipFree(d); hipFree(grid); hipFree(obs); hipFree(ws); hipFree(counters); hipFree(flags); hipFree(Xa); free(host8);
  }
  int sync(int phase, int step_flags) {
    if (periodic_entry)
      return done(phase ? "periodic phase 1" : "periodic phase 0",
                  mia_letkf_sharded_step_periodic_f32(X, G, m, k, Yb, d, P, grid, obs, n_coord, cg, per, rc, n_r, 1e-5, 1.1f, gamma, method, hint, comm, chunks,
                                                      phase, Xa, flags, counters, ws, ws_bytes, S, CS, prep, step_flags));
    return done(phase ? "step phase 1" : "step phase 0",
                mia_letkf_sharded_step_streams_f32(X, G, m, k, Yb, d, P, grid, obs, n_coord, cg, rc, n_r, 1e-5, 1.1f, gamma, method, hint, comm, chunks, phase, Xa,
                                                   flags, counters, ws, ws_bytes, S, CS, prep, step_flags));
  }
  void both(int step_flags) { sync(0, step_flags); sync(1, step_flags); }
  mia_step_args_t block(int phase, int step_flags) {
    mia_step_args_t a;
    memset(&a, 0, sizeof a);
    a.X = X; a.G = G; a.m = m; a.k = k; a.Yb = Yb; a.d = d; a.P = P; a.grid_xyz = grid; a.obs_xyz = obs; a.n_coord = n_coord; a.n_r = n_r;
    for (int i = 0; i < 3; ++i) { a.coord_group[i] = cg[i]; a.gc_c[i] = rc[i]; a.period[i] = per[i]; }
    a.gc_eps = 1e-5; a.inf_factor = 1.1f; a.gamma = gamma; a.method = method; a.p_max_assumed = hint; a.comm = comm; a.n_chunks = chunks; a.phase = phase;
    a.Xa = Xa; a.flags = flags; a.counters = counters; a.ws = ws; a.ws_bytes = ws_bytes; a.stream = S; a.comm_stream = CS; a.prep_stream = prep;
    a.step_flags = step_flags; a.host8 = host8; a.after_stream = comm ? CS : S; a.on_stream = RS; a.done_event = &event;
    return a;
  }
  int run_args(int phase, int step_flags, mia_step_args_t* edit = nullptr) {
    mia_step_args_t a = edit ? *edit : block(phase, step_flags);
    int32_t out8[8];
    return done(phase ? "run_args phase 1" : "run_args phase 0", mia_letkf_step_run_args(&a, out8));
  }
  // a submitted step, joined (plain entry) or collected (argument block) at once
  void submit(int step_flags, bool through_block, void* t0 = nullptr, void* t1 = nullptr, void* caller = nullptr) {
    void* job = nullptr;
    int32_t out8[8];
    if (through_block) {
      mia_step_args_t a = block(0, step_flags);
      a.time_start_event = t0; a.time_stop_event = t1; a.caller_stream = caller; a.in_event = caller ? &in_event : nullptr;
      if (submitted_rc("submit_args", mia_letkf_step_submit_args(&a, &job)) == MIA_OK)
        done("collect", mia_letkf_step_collect(job, &event, host8, S, 1, out8));
    } else {
      if (submitted_rc("submit", mia_letkf_step_submit(X, G, m, k, Yb, d, P, grid, obs, n_coord, cg, rc, n_r, 1e-5, 1.1f, gamma, method, hint, comm, chunks, 0, Xa, flags,
                                               counters, ws, ws_bytes, S, CS, prep, step_flags, host8, comm ? CS : S, RS, &event, t0, t1, &job)) == MIA_OK)
        done("join", mia_letkf_step_join(job));
    }
  }
};

static void one_rank() {
  { header("default route (fused localisation), phases 0 and 1"); Rig r; r.alloc(); r.both(0); }
  { header("run_args: default route, phases 0 and 1"); Rig r; r.alloc(); r.run_args(0, MIA_STEP_NO_JOIN); r.run_args(1, 0); }
  { header("MIA_STEP_NO_TILE_LISTS (lazy sort)"); Rig r; r.alloc(); r.both(MIA_STEP_NO_TILE_LISTS); }
  { header("MIA_STEP_NO_TILE_LISTS, step_lazy_sort=0"); opt("step_lazy_sort", 0); Rig r; r.alloc(); r.both(MIA_STEP_NO_TILE_LISTS); opt("step_lazy_sort", -1); }
  { header("MIA_STEP_SCAN_INDEX"); Rig r; r.alloc(); r.both(MIA_STEP_SCAN_INDEX); }
  { header("geometry epoch: KEEP_LISTS, KEEP_LISTS|REUSE_LISTS, reuse after a radius change");
    Rig r; r.alloc();
    r.both(MIA_STEP_KEEP_LISTS);
    r.both(MIA_STEP_KEEP_LISTS | MIA_STEP_REUSE_LISTS | MIA_STEP_WS_CLEAN);
    r.rc[0] = 12.0;
    r.both(MIA_STEP_KEEP_LISTS | MIA_STEP_REUSE_LISTS | MIA_STEP_WS_CLEAN); }
  { header("geometry epoch with gamma > 0"); Rig r; r.gamma = 0.5f; r.alloc(); r.sync(0, MIA_STEP_KEEP_LISTS); r.sync(0, MIA_STEP_KEEP_LISTS | MIA_STEP_REUSE_LISTS); }
  for (const char* name : {"tile_fused", "bucket_index", "tile_lists", "tile", "tile_split"}) {
    char h[64];
    snprintf(h, sizeof h, "option %s=0", name);
    header(h);
    opt(name, 0); Rig r; r.alloc(); r.both(0); opt(name, -1);
  }
  for (int pair = 0; pair < 2; ++pair) {
    header(pair ? "p_max_assumed 40 (three row blocks), tile_pair=1" : "p_max_assumed 40 (three row blocks), tile_pair=0");
    opt("tile_pair", pair); Rig r; r.hint = 40; r.alloc(); r.both(0); r.both(MIA_STEP_KEEP_LISTS); opt("tile_pair", -1);
  }
  { header("extra row blocks: MIA_STEP_TILE_EXTRA(1), (2), (7)");
    Rig r; r.alloc(); r.both(MIA_STEP_TILE_EXTRA(1)); r.both(MIA_STEP_TILE_EXTRA(2)); r.both(MIA_STEP_TILE_EXTRA(7)); }
  for (int method = 1; method < 3; ++method) {
    header(method == 1 ? "method 1" : "method 2");
    Rig r; r.method = method; r.alloc(); r.both(0);
  }
  { header("gamma > 0, k = 40"); Rig r; r.gamma = 0.5f; r.alloc(); r.both(0); }
  { header("gamma > 0, k = 48"); Rig r; r.gamma = 0.5f; r.k = 48; r.alloc(); r.both(0); }
  { header("m = 2"); Rig r; r.m = 2; r.alloc(); r.both(0); }
  { header("P = 0"); Rig r; r.P = 0; r.alloc(); r.both(0); }
  { header("second and third step on a workspace: MIA_STEP_WS_CLEAN, then MIA_STEP_FRESH_BOX");
    Rig r; r.alloc(); r.sync(0, 0); r.sync(0, MIA_STEP_WS_CLEAN); r.sync(0, MIA_STEP_WS_CLEAN | MIA_STEP_FRESH_BOX);
    r.sync(0, MIA_STEP_WS_CLEAN | MIA_STEP_NO_TILE_LISTS); r.sync(0, MIA_STEP_WS_CLEAN | MIA_STEP_SCAN_INDEX); r.sync(0, MIA_STEP_WS_CLEAN | MIA_STEP_SCAN_INDEX); }
  { header("two coordinates, two radii"); Rig r; r.n_coord = 2; r.n_r = 2; r.cg[1] = 1; r.alloc(); r.both(0); r.both(MIA_STEP_NO_TILE_LISTS); }
  { header("three coordinates"); Rig r; r.n_coord = 3; r.alloc(); r.both(0); r.both(MIA_STEP_KEEP_LISTS); }
  { header("cyclic coordinate through the periodic entry"); Rig r; r.periodic_entry = true; r.per[0] = 4000.0; r.alloc(); r.both(0); r.both(MIA_STEP_NO_TILE_LISTS); }
  { header("periodic entry with every period zero (open)"); Rig r; r.periodic_entry = true; r.alloc(); r.sync(0, 0); }
  { header("cyclic coordinate through the argument block"); Rig r; r.per[0] = 4000.0; r.alloc(); r.run_args(0, 0); r.run_args(1, 0); r.submit(MIA_STEP_NO_JOIN, true); }
  { header("timing hook");
    Rig r; r.alloc();
    void *t0 = nullptr, *t1 = nullptr;
    mia_timing_event_acquire(&t0); mia_timing_event_acquire(&t1);
    done("timing_events", mia_letkf_step_timing_events(t0, t1)); r.both(0);
    done("timing_events", mia_letkf_step_timing_events(t0, t1)); r.sync(0, MIA_STEP_NO_TILE_LISTS);
    mia_step_args_t a = r.block(0, 0);
    a.time_start_event = t0; a.time_stop_event = t1; a.caller_stream = busy_stream(5); a.in_event = &r.in_event;
    r.run_args(0, 0, &a);
    mia_timing_event_release(t0); mia_timing_event_release(t1); }
  { header("preparation stream, synchronous"); Rig r; r.prep = PS; r.alloc(); r.both(0); r.both(MIA_STEP_NO_TILE_LISTS); }
}

static void submitted() {
  void *t0 = nullptr, *t1 = nullptr;
  mia_timing_event_acquire(&t0); mia_timing_event_acquire(&t1);
  for (int hostwait = 1; hostwait >= 0; --hostwait) {
    header(hostwait ? "submitted steps, step_hostwait=1" : "submitted steps, step_hostwait=0");
    opt("step_hostwait", hostwait);
    Rig r; r.prep = PS; r.alloc();
    r.submit(MIA_STEP_NO_JOIN, false);                                                  // first step on the workspace
    r.submit(MIA_STEP_NO_JOIN | MIA_STEP_WS_CLEAN, false);                              // second: the other count array
    r.submit(MIA_STEP_NO_JOIN | MIA_STEP_WS_CLEAN, true, t0, t1, stream(5));            // timed, idle caller stream
    r.submit(MIA_STEP_NO_JOIN | MIA_STEP_WS_CLEAN, true, nullptr, nullptr, busy_stream(5));      // untimed, busy caller stream
    done("workspace_release", mia_letkf_step_workspace_release(r.ws));
    r.submit(MIA_STEP_NO_JOIN | MIA_STEP_WS_CLEAN, false, t0, t1);                      // after a release: starts from unknown
    r.submit(MIA_STEP_NO_JOIN | MIA_STEP_NO_TILE_LISTS, true, t0, t1);                  // per-point lists, timed
    r.submit(0, false);                                                                 // joins: no host wait
    r.gamma = 0.5f;
    r.submit(MIA_STEP_NO_JOIN, true, t0, t1);
    opt("step_hostwait", -1);
  }
  { header("submitted steps without a preparation stream"); Rig r; r.alloc(); r.submit(MIA_STEP_NO_JOIN, false); r.submit(MIA_STEP_NO_JOIN | MIA_STEP_WS_CLEAN, true, t0, t1); }
  { header("submitted step, lists not lazily sorted, timed (another kernel than the tile kernel may serve it)");
    opt("step_lazy_sort", 0); Rig r; r.prep = PS; r.k = 48; r.gamma = 0.5f; r.alloc(); r.submit(MIA_STEP_NO_JOIN, true, t0, t1); r.submit(MIA_STEP_NO_JOIN, true);
    opt("step_lazy_sort", -1); }
  { header("submitted step, method 1"); Rig r; r.prep = PS; r.method = 1; r.alloc(); r.submit(MIA_STEP_NO_JOIN, false); }
  done("drain", mia_letkf_step_drain());
  mia_timing_event_release(t0); mia_timing_event_release(t1);
}

static void communicators() {
  for (int pieces = 2; pieces <= 4; pieces += 2)
    for (int odd = 0; odd < 2; ++odd) {
      char h[96];
      snprintf(h, sizeof h, "custom communicator, world 1, %d pieces, G = %d", pieces, 4000 + odd);
      header(h);
      mia_comm_t* c = nullptr;
      done("comm_create_custom", mia_comm_create_custom(0, 1, allgather_cb, allreduce_cb, nullptr, &c));
      { Rig r; r.G = 4000 + odd; r.comm = c; r.chunks = pieces; r.alloc();
        r.both(0);                                    // tile route: one launch over the pieces
        r.both(MIA_STEP_NO_TILE_LISTS);               // segmented launch
        opt("segment_signal", 0); r.both(MIA_STEP_NO_TILE_LISTS); opt("segment_signal", -1);
        r.sync(0, MIA_STEP_KEEP_LISTS); r.sync(0, MIA_STEP_KEEP_LISTS | MIA_STEP_REUSE_LISTS);
        if (pieces == 2) { r.gamma = 0.5f; r.sync(0, 0); r.gamma = 0.0f; r.method = 1; r.both(0); r.method = 0; }
        done("comm_set_place_stream", mia_comm_set_place_stream(c, XS));
        r.sync(0, 0); r.sync(0, MIA_STEP_NO_JOIN);
        r.prep = PS; r.submit(MIA_STEP_NO_JOIN, false); r.submit(0, true);
        { Rig q; q.comm = c; q.chunks = 1; q.alloc(); q.sync(0, 0); }      // one piece on a one-rank communicator: no exchange
      }
      done("comm_destroy", mia_comm_destroy(c));
    }
  for (int rank = 0; rank < 2; ++rank) {
    header(rank ? "partition communicator, rank 1 of 2, MIA_STEP_NO_GATHER" : "partition communicator, rank 0 of 2, MIA_STEP_NO_GATHER");
    mia_comm_t* c = nullptr;
    done("comm_create_partition", mia_comm_create_partition(rank, 2, &c));
    { Rig r; r.G = 4001; r.comm = c; r.world = 2; r.alloc();
      r.both(MIA_STEP_NO_GATHER); r.both(MIA_STEP_NO_GATHER | MIA_STEP_NO_TILE_LISTS);
      r.sync(0, 0);      // (no exchange can run on a partition-only communicator)
      r.prep = PS; r.submit(MIA_STEP_NO_GATHER | MIA_STEP_NO_JOIN, true); }
    done("comm_destroy", mia_comm_destroy(c));
  }
  { header("partition communicator, rank 3 of 4, G = 6: an empty block");
    mia_comm_t* c = nullptr;
    done("comm_create_partition", mia_comm_create_partition(3, 4, &c));
    { Rig r; r.G = 6; r.P = 20; r.comm = c; r.world = 4; r.alloc(); r.both(MIA_STEP_NO_GATHER); }
    done("comm_destroy", mia_comm_destroy(c)); }
  { header("direct peer exchange, world 2, buffers attached in-process");
    mia_comm_t *c0 = nullptr, *c1 = nullptr;
    done("comm_create_custom", mia_comm_create_custom(0, 2, allgather_cb, allreduce_cb, nullptr, &c0));
    done("comm_create_custom", mia_comm_create_custom(1, 2, allgather_cb, allreduce_cb, nullptr, &c1));
    Rig r; r.comm = c0; r.world = 2; r.alloc();
    const size_t bytes = sizeof(float) * r.m * r.k * r.G;
    done("peer_alloc", mia_comm_peer_alloc(c0, bytes, 2, nullptr));
    done("peer_alloc", mia_comm_peer_alloc(c1, bytes, 2, nullptr));
    void* b1[2] = {mia_comm_peer_buffer(c1, 0), mia_comm_peer_buffer(c1, 1)};
    done("peer_attach", mia_comm_peer_attach(c0, 1, b1, mia_comm_peer_sync_area(c1)));
    float* own = r.Xa;
    r.Xa = (float*)mia_comm_peer_buffer(c0, 1);
    r.both(0); r.sync(0, MIA_STEP_NO_JOIN | MIA_STEP_NO_TILE_LISTS);
    r.prep = PS; r.submit(MIA_STEP_NO_JOIN, false);
    done("peer_exchange", mia_comm_peer_exchange(c0, 1, r.m * r.k, r.G, 0, 2000, r.counters, CS));
    done("peer_rewait", mia_comm_peer_rewait(c0, 1, r.counters, CS));
    r.Xa = own;
    done("comm_destroy", mia_comm_destroy(c0)); done("comm_destroy", mia_comm_destroy(c1)); }
}

static void errors() {
  header("error returns");
  Rig r; r.alloc();
  const int n_fields = 11;
  for (int f = 0; f < n_fields; ++f) {      // each required pointer NULL in turn
    Rig q = r;
    switch (f) {
      case 0: q.X = nullptr; break; case 1: q.Xa = nullptr; break; case 2: q.flags = nullptr; break; case 3: q.counters = nullptr; break;
      case 4: q.ws = nullptr; break; case 5: q.grid = nullptr; break; case 6: q.Yb = nullptr; break; case 7: q.d = nullptr; break;
      case 8: q.obs = nullptr; break; default: break;
    }
    if (f < 9) q.sync(0, 0);
    if (f == 9) done("step, coord_group NULL", mia_letkf_sharded_step_streams_f32(r.X, r.G, r.m, r.k, r.Yb, r.d, r.P, r.grid, r.obs, 1, nullptr, r.rc, 1, 1e-5, 1.1f, 0.0f, 0, 20,
                                                                                nullptr, 1, 0, r.Xa, r.flags, r.counters, r.ws, r.ws_bytes, S, CS, nullptr, 0));
    if (f == 10) done("step, gc_c NULL", mia_letkf_sharded_step_streams_f32(r.X, r.G, r.m, r.k, r.Yb, r.d, r.P, r.grid, r.obs, 1, r.cg, nullptr, 1, 1e-5, 1.1f, 0.0f, 0, 20,
                                                                          nullptr, 1, 0, r.Xa, r.flags, r.counters, r.ws, r.ws_bytes, S, CS, nullptr, 0));
    q.X = nullptr;      // (the copy owns nothing)
  }
  { Rig q = r; q.ws = (char*)r.ws + 8; q.sync(0, 0); q.X = nullptr; }                        // misaligned workspace
  { Rig q = r; q.ws_bytes = r.ws_bytes - 1; q.sync(0, 0); q.X = nullptr; }                   // too small
  { Rig q = r; q.method = 3; q.sync(0, 0); q.method = -1; q.sync(0, 0); q.X = nullptr; }
  { Rig q = r; q.sync(2, 0); q.X = nullptr; }                                                // phase 2
  for (int nc : {0, 4}) { Rig q = r; q.n_coord = nc; q.sync(0, 0); q.periodic_entry = true; q.sync(0, 0); q.run_args(0, 0); q.submit(0, false); q.submit(0, true); q.X = nullptr; }
  for (int nr : {0, MIA_MAX_RADII + 1}) { Rig q = r; q.n_r = nr; q.sync(0, 0); q.run_args(0, 0); q.submit(0, false); q.submit(0, true); q.X = nullptr; }
  for (double bad : {-1.0, std::numeric_limits<double>::infinity(), std::nan("")}) {
    Rig q = r; q.per[0] = bad; q.periodic_entry = true; q.sync(0, 0); q.run_args(0, 0); q.submit(0, true); q.X = nullptr;
  }
  done("periodic entry, period NULL", mia_letkf_sharded_step_periodic_f32(r.X, r.G, r.m, r.k, r.Yb, r.d, r.P, r.grid, r.obs, 1, r.cg, nullptr, r.rc, 1, 1e-5, 1.1f, 0.0f, 0, 20,
                                                                          nullptr, 1, 0, r.Xa, r.flags, r.counters, r.ws, r.ws_bytes, S, CS, nullptr, 0));
  { mia_step_args_t a = r.block(0, 0); void* t0 = nullptr; mia_timing_event_acquire(&t0); a.time_start_event = t0; r.run_args(0, 0, &a); mia_timing_event_release(t0); }
  { mia_step_args_t a = r.block(0, 0); a.host8 = nullptr; r.run_args(0, 0, &a); a = r.block(0, 0); a.done_event = nullptr; r.run_args(0, 0, &a); }
  done("run_args NULL", mia_letkf_step_run_args(nullptr, nullptr));
  done("submit_args NULL", mia_letkf_step_submit_args(nullptr, nullptr));
  { mia_step_args_t a = r.block(0, 0); done("submit_args, job_out NULL", mia_letkf_step_submit_args(&a, nullptr)); }
  done("timing_events, one NULL", mia_letkf_step_timing_events(r.ws, nullptr));
  { Rig q = r; q.chunks = 16; q.sync(0, 0); q.X = nullptr; }      // (without a communicator the step has one piece)
  { mia_comm_t* c = nullptr; mia_comm_create_custom(0, 1, allgather_cb, allreduce_cb, nullptr, &c);
    Rig q = r; q.comm = c; q.chunks = 16; q.sync(0, 0); q.chunks = 2; q.sync(0, 0);      // too many pieces; a workspace sized for one
    q.X = nullptr; mia_comm_destroy(c);
    mia_comm_create_custom(0, 1, allgather_cb, allreduce_cb, nullptr, &c);
    { Rig e; e.comm = c; e.chunks = 2; e.alloc(); mia_step_args_t a = e.block(0, 0); a.comm_stream = nullptr; e.run_args(0, 0, &a); }      // exchange route, no exchange stream
    mia_comm_destroy(c); }
  { mia_comm_t* c = nullptr; mia_comm_create_partition(0, 2, &c); Rig q = r; q.comm = c; q.sync(0, 0); q.X = nullptr; mia_comm_destroy(c); }      // partition-only, gather asked
  done("workspace_bytes NULL", mia_letkf_sharded_step_workspace_bytes(4000, 1, 40, 2000, 1, 1, 1, 20, nullptr));
  done("join NULL", mia_letkf_step_join(nullptr));
}

int main() {
  mia_stub_trace_enable(1);
  one_rank();
  submitted();
  communicators();
  errors();
  done("drain", mia_letkf_step_drain());
  return 0;
}
