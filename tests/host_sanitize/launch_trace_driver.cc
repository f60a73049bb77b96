// The launch trace of the tile entries (tests/test_tile_launch_trace.py): every C entry that ends in a tile kernel, called on ONE thread
// against the stub HIP runtime of hip_stub.cc with its call trace and its attribute trace switched on.  Per call a header line
// ("# entry sizes"), the runtime calls it made (every launch with kernel name and template arguments, grid, block, LDS bytes and stream;
// every hipFuncSetAttribute with kernel name and bytes; fills), and a line with the return code and the string mia_last_analysis_kernel returns
// afterwards.  The array arguments are a few bytes of host memory that no entry reads or writes on the host (the census workspace, which the
// entry zeroes, is real); nothing depends on addresses: the output is compared line for line with tests/golden/tile_launch_trace.txt.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>
#include "mia_letkf.h"

extern "C" void mia_stub_trace_enable(int on);
extern "C" void mia_stub_trace_note(const char* text);
extern "C" void mia_stub_trace_flush(FILE* to);
extern "C" int hipMalloc(void**, size_t);
extern "C" int hipFree(void*);

static void* dmalloc(size_t n) { void* p = nullptr; if (hipMalloc(&p, n) != 0) abort(); return p; }
static void* const S = (void*)0x1000;
alignas(256) static char g_dummy[256];
template <typename T> static T* dummy() { return reinterpret_cast<T*>(g_dummy); }

static void opt(const char* name, int v) { if (mia_set_option(name, v) != MIA_OK) abort(); }
static void section(const char* name) { printf("## %s\n", name); }
static int done(int rc) {
  char name[160];
  mia_stub_trace_flush(stdout);
  mia_last_analysis_kernel(name, (int)sizeof name);
  printf("= %d \"%s\"\n", rc, name);
  return rc;
}

// ---- the float64 entries ---------------------------------------------------------------------------------------------------------
constexpr int64_t kTiles = (int64_t)65536 * 65535;      // the last grid that fits
struct Shape { int k, p_max; int64_t ng; int64_t n_tiles; int ub; };
static const mia_kernel_op_t kProgSq[] = {{MIA_KOP_SQDIST, 0, 0.0}, {MIA_KOP_CONST, 0, -0.5}, {MIA_KOP_MUL, 0, 0.0}, {MIA_KOP_EXP, 0, 0.0}};
static const mia_kernel_op_t kProgDot[] = {{MIA_KOP_DOT, 0, 0.0}};
static const mia_kernel_op_t kProgAll[] = {{MIA_KOP_DOT, 0, 0.0}, {MIA_KOP_SQDIST, 0, 0.0}, {MIA_KOP_ADD, 0, 0.0}, {MIA_KOP_L1DIST, 0, 0.0}, {MIA_KOP_ADD, 0, 0.0}};

enum Entry { A_MATFUN, A_PATCH, A_DENSE, A_WIDE, A_STREAM, W_MATFUN, W_WIDE, W_STREAM, W_PATCH, I_MATFUN, I_WIDE, I_STREAM, A_RBF, A_KERN_SQ,
             A_KERN_DOT, A_KERN_ALL, N_ENTRIES };
static const char* const kEntryName[N_ENTRIES] = {
    "analysis_matfun_f64", "analysis_patch_f64", "analysis_dense_f64", "analysis_wide_f64", "analysis_stream_f64", "weights_matfun_f64",
    "weights_wide_f64", "weights_stream_f64", "weights_patch_f64", "lienks_update_matfun_f64", "lienks_update_wide_f64",
    "lienks_update_stream_f64", "lketkf_rbf_analysis_matfun_f64", "lketkf_kernel_analysis_matfun_f64(sq)",
    "lketkf_kernel_analysis_matfun_f64(dot)", "lketkf_kernel_analysis_matfun_f64(dot,sq,l1)"};
static bool is_dual(Entry e) { return e == A_MATFUN || e == A_WIDE || e == W_MATFUN || e == W_WIDE || e == I_MATFUN || e == I_WIDE; }
static bool is_kernelised(Entry e) { return e >= A_RBF; }
static bool has_map(Entry e) { return e == A_PATCH || e == W_PATCH; }
static bool state_optional(Entry e) { return e >= W_MATFUN && e <= I_STREAM; }

static int call64(Entry e, const Shape& s) {
  const int k = s.k, p_max = s.p_max, p_cap = 512;
  const int64_t ng = s.ng, P = 1000;
  if (has_map(e)) printf("# %s k=%d p_max=%d ng=%lld n_tiles=%lld union_blocks=%d\n", kEntryName[e], k, p_max, (long long)ng, (long long)s.n_tiles, s.ub);
  else printf("# %s k=%d p_max=%d ng=%lld\n", kEntryName[e], k, p_max, (long long)ng);
  double *X = dummy<double>(), *Xa = dummy<double>(), *W = dummy<double>();
  const double *rec = dummy<double>(), *w = dummy<double>();
  const int32_t *cnt = dummy<int32_t>(), *idx = dummy<int32_t>(), *map = dummy<int32_t>();
  int32_t *flags = dummy<int32_t>(), *retry = dummy<int32_t>();
  switch (e) {
    case A_MATFUN: return done(mia_letkf_analysis_matfun_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, Xa, ng, 0, flags, retry, S));
    case A_DENSE: return done(mia_letkf_analysis_dense_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, Xa, ng, 0, flags, retry, S));
    case A_WIDE: return done(mia_letkf_analysis_wide_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, Xa, ng, 0, flags, retry, S));
    case A_STREAM: return done(mia_letkf_analysis_stream_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, Xa, ng, 0, flags, retry, S));
    case A_PATCH: return done(mia_letkf_analysis_patch_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, Xa, ng, 0, flags, retry, map, s.n_tiles, s.ub, S));
    case W_MATFUN: return done(mia_letkf_weights_matfun_f64(nullptr, 0, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, nullptr, 0, 0, W, flags, retry, S));
    case W_WIDE: return done(mia_letkf_weights_wide_f64(nullptr, 0, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, nullptr, 0, 0, W, flags, retry, S));
    case W_STREAM: return done(mia_letkf_weights_stream_f64(nullptr, 0, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, nullptr, 0, 0, W, flags, retry, S));
    case W_PATCH: return done(mia_letkf_weights_patch_f64(nullptr, 0, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.0, nullptr, 0, 0, W, flags, retry, map, s.n_tiles, s.ub, S));
    case I_MATFUN: return done(mia_lienks_update_matfun_f64(W, (int64_t)k * k, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 0.0, W, flags, retry, S));
    case I_WIDE: return done(mia_lienks_update_wide_f64(W, (int64_t)k * k, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 0.0, W, flags, retry, S));
    case I_STREAM: return done(mia_lienks_update_stream_f64(W, 0, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 0.01, W, flags, retry, S));
    case A_RBF: return done(mia_lketkf_rbf_analysis_matfun_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, 0.5, Xa, ng, 0, flags, retry, S));
    case A_KERN_SQ: return done(mia_lketkf_kernel_analysis_matfun_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, kProgSq, 4, Xa, ng, 0, flags, retry, S));
    case A_KERN_DOT: return done(mia_lketkf_kernel_analysis_matfun_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, kProgDot, 1, Xa, ng, 0, flags, retry, S));
    case A_KERN_ALL: return done(mia_lketkf_kernel_analysis_matfun_f64(X, ng, 1, k, 0, ng, rec, P, cnt, idx, w, p_cap, p_max, 1.1, kProgAll, 5, Xa, ng, 0, flags, retry, S));
    default: abort();
  }
}

// one shape inside each entry's cover: dual p_max <= k, primal p_max > k, the kernelised routes either
static Shape covered(Entry e, int64_t ng) { return Shape{16, is_dual(e) || is_kernelised(e) ? 8 : 40, ng, (ng + 15) >> 4, 8}; }

// The k x p_max cross, thinned to what decides a launch: per number of member blocks KT = ceil(k / 16) every number of row blocks
// UT = ceil((p_max + 8) / 16) a ladder can reach (p_max = 0, 9, 25, ... 105), p_max on both sides of every cover, k on both sides of
// every cap.
static void cross64() {
  section("float64 entries, ng = 203: ensemble size x longest list");
  for (int e = 0; e < N_ENTRIES; ++e) {
    const Entry en = (Entry)e;
    if (is_dual(en)) {
      const int cap = en == A_WIDE || en == W_WIDE || en == I_WIDE ? 128 : 64;
      for (int k : {2, 16, 32, 48, 64, 65, 80, 96, 112, 128, 129}) {
        std::set<int> ps = {0};
        if (k <= cap) for (int p : {9, 25, 41, 57, 73, 89, 105}) if (p < k) ps.insert(p);
        if (k == 2 || k == cap) { ps.insert(k); ps.insert(k + 1); }
        if (k <= cap + 1) for (int p : ps) call64(en, Shape{k, p, 203, 13, 8});
      }
    } else if (is_kernelised(en)) {
      for (int k : {2, 17, 40, 41})
        for (int p : {0, 9, 25, 64, 65}) if (k <= 40 || p == 0) call64(en, Shape{k, p, 203, 13, 8});
    } else {      // primal: p_max > k, up to 256 slots or what the resident image holds (224 at k = 64)
      const int cap = en == A_DENSE || en == A_PATCH ? 64 : 128;
      for (int k : {2, 16, 32, 48, 64, 65, 80, 96, 112, 128, 129}) {
        std::set<int> ps = {k + 1};
        if (k == 2 || k == cap) for (int p : {k, 256, 257}) ps.insert(p);
        if (k == 64) for (int p : {224, 225}) ps.insert(p);
        if (k <= cap + 1) for (int p : ps) call64(en, Shape{k, p, 203, 13, 8});
      }
    }
  }
}

static void grids64() {
  section("float64 entries, one covered shape: the grid");
  for (int e = 0; e <= A_KERN_SQ; ++e) {      // (the other statistic sets launch through the same function)
    for (int64_t ng : {(int64_t)1, (int64_t)16, (int64_t)17, (int64_t)1048576, (int64_t)1048577}) call64((Entry)e, covered((Entry)e, ng));
    if (state_optional((Entry)e))      // no state: no leading dimension bounds the range
      for (int64_t ng : {16 * kTiles, 16 * kTiles + 1}) call64((Entry)e, covered((Entry)e, ng));
  }
  section("the two map entries: union_blocks and n_tiles");
  for (Entry e : {A_PATCH, W_PATCH}) {
    for (int ub : {1, 16, 17}) { Shape s = covered(e, 203); s.ub = ub; call64(e, s); }
    { Shape s = covered(e, 203); s.k = 64; s.p_max = 100; for (int ub : {14, 15}) { s.ub = ub; call64(e, s); } }      // (the resident image holds 14 blocks at k = 64)
    for (int64_t nt : {(int64_t)1, (int64_t)65536, (int64_t)65537, kTiles, kTiles + 1}) { Shape s = covered(e, 203); s.n_tiles = nt; call64(e, s); }
  }
}

static void census() {
  section("mia_letkf_tile_union_census");
  const int64_t np = 203;
  int32_t* ws = (int32_t*)dmalloc(sizeof(int32_t) * (np + 2));
  int32_t* out2 = (int32_t*)dmalloc(sizeof(int32_t) * 2);
  for (int count : {1, 0})
    for (int64_t nt : {(int64_t)1, (int64_t)13, (int64_t)65536, (int64_t)65537, kTiles, kTiles + 1, ((int64_t)1 << 31) - 1, (int64_t)1 << 31}) {
      if (count == 0 && nt != 13) continue;
      printf("# tile_union_census n_tiles=%lld n_points=%lld count_unions=%d\n", (long long)nt, (long long)np, count);
      done(mia_letkf_tile_union_census(dummy<int32_t>(), nt, np, dummy<int32_t>(), dummy<int32_t>(), 64, 40, count, out2, ws, sizeof(int32_t) * (np + 2), S));
    }
  hipFree(ws); hipFree(out2);
}

static void options64() {
  for (const char* name : {"tile", "cheb_table"}) {
    char h[64];
    snprintf(h, sizeof h, "float64 entries, option %s=0", name);
    section(h);
    opt(name, 0);
    for (int e = 0; e <= A_KERN_SQ; ++e) call64((Entry)e, covered((Entry)e, 203));
    opt(name, -1);
  }
}

// ---- the float32 entries ---------------------------------------------------------------------------------------------------------
struct Shape32 { int m, k, p_max, extra; int64_t ng; float gamma; };

static void lists32(const char* entry, const Shape32& s, bool weights) {
  printf("# %s m=%d k=%d p_max=%d ng=%lld gamma=%g\n", entry, s.m, s.k, s.p_max, (long long)s.ng, (double)s.gamma);
  float *X = dummy<float>(), *Xa = dummy<float>(), *W = dummy<float>();
  if (weights) done(mia_letkf_weights_matfun_f32(X, s.ng, s.m, s.k, 0, s.ng, dummy<float>(), 1000, dummy<int32_t>(), dummy<int32_t>(), dummy<double>(), 512, s.p_max, 1.1f,
                                                 s.gamma, Xa, s.ng, 0, W, dummy<int32_t>(), dummy<int32_t>(), S));
  else done(mia_letkf_analysis_matfun_f32(X, s.ng, s.m, s.k, 0, s.ng, dummy<float>(), 1000, dummy<int32_t>(), dummy<int32_t>(), dummy<double>(), 512, s.p_max, 1.1f, s.gamma,
                                          Xa, s.ng, 0, dummy<int32_t>(), dummy<int32_t>(), S));
}
static void packed32(const Shape32& s, bool weights, bool retry) {
  printf("# %s m=%d k=%d p_max=%d ng=%lld gamma=%g weights=%d\n", retry ? "analysis_retry_f32" : "analysis_packed_f32", s.m, s.k, s.p_max, (long long)s.ng, (double)s.gamma,
         (int)weights);
  float *X = dummy<float>(), *Xa = dummy<float>(), *W = weights ? dummy<float>() : nullptr;
  if (retry) done(mia_letkf_analysis_retry_f32(X, s.ng, s.m, s.k, 0, s.ng, dummy<float>(), 1000, dummy<int32_t>(), dummy<int32_t>(), dummy<double>(), 512, s.p_max, 1.1f, s.gamma,
                                               Xa, s.ng, 0, dummy<int32_t>(), S));
  else done(mia_letkf_analysis_packed_f32(X, s.ng, s.m, s.k, 0, s.ng, dummy<float>(), 1000, dummy<int32_t>(), dummy<int32_t>(), dummy<double>(), 512, s.p_max, 1.1f, s.gamma, Xa,
                                          s.ng, 0, W, dummy<int32_t>(), S));
}
static void tiles32(const Shape32& s, int which) {      // 0: analysis, 1: weights, 2: RBF
  static const char* const names[] = {"analysis_tiles_f32", "weights_tiles_f32", "lketkf_rbf_analysis_tiles_f32"};
  printf("# %s m=%d k=%d p_max=%d extra_blocks=%d ng=%lld\n", names[which], s.m, s.k, s.p_max, s.extra, (long long)s.ng);
  float *X = dummy<float>(), *Xa = dummy<float>();
  if (which == 0) done(mia_letkf_analysis_tiles_f32(X, s.ng, s.m, s.k, 0, s.ng, g_dummy, 1000, g_dummy, s.p_max, s.extra, 1.1f, Xa, s.ng, 0, dummy<int32_t>(), dummy<int32_t>(), S));
  if (which == 1) done(mia_letkf_weights_tiles_f32(X, s.ng, s.m, s.k, 0, s.ng, g_dummy, 1000, g_dummy, s.p_max, s.extra, 1.1f, Xa, s.ng, 0, dummy<float>(), dummy<int32_t>(),
                                                   dummy<int32_t>(), S));
  if (which == 2) done(mia_lketkf_rbf_analysis_tiles_f32(X, s.ng, s.m, s.k, 0, s.ng, dummy<float>(), dummy<float>(), 1000, g_dummy, s.p_max, s.extra, 1.1f, 0.5f, Xa, s.ng, 0,
                                                         dummy<int32_t>(), dummy<int32_t>(), S));
}

static const int64_t kGrid32[] = {1, 16, 17, 1048576, 1048577};

static void float32_entries() {
  static const int kRowBlocks[] = {0, 9, 25, 41, 57, 73, 88};      // p_max of one, two, ... six row blocks (and the last list the tile kernels take)
  section("analysis_matfun_f32 on the tile kernel (letkf_tile.hip): split-precision and f32 products");
  for (int split = 1; split >= 0; --split) {
    opt("tile_split", split);
    for (int k : {2, 3, 16, 32, 48, 64, 80, 96, 97})
      for (int p : kRowBlocks) if (p <= k && (split || k == 2 || k == 48 || k == 96)) lists32("analysis_matfun_f32", Shape32{1, k, p, 0, 203, 0.0f}, false);
    lists32("analysis_matfun_f32", Shape32{2, 40, 20, 0, 203, 0.0f}, false);
    for (int64_t ng : kGrid32) lists32("analysis_matfun_f32", Shape32{1, 40, 20, 0, ng, 0.0f}, false);
    opt("tile_split", -1);
  }
  section("analysis_matfun_f32 / weights_matfun_f32 off the tile kernel (letkf_cheb.hip)");
  opt("tile", 0);
  for (int k : {16, 64, 80, 128, 129})
    for (int p : {4, 32, 33, 48, 64, 65, 200})
      for (int m : {1, 8}) {
        lists32("analysis_matfun_f32", Shape32{m, k, p, 0, 203, 0.0f}, false);
        if (m == 1 && k == 16) lists32("analysis_matfun_f32", Shape32{m, k, p, 0, 203, 0.5f}, false);
        if (m == 1 && k <= 64) lists32("weights_matfun_f32", Shape32{m, k, p, 0, 203, 0.0f}, true);
      }
  opt("cheb_rowbatch", 0); lists32("analysis_matfun_f32", Shape32{8, 40, 20, 0, 203, 0.0f}, false); opt("cheb_rowbatch", -1);
  opt("cheb_big", 0); lists32("analysis_matfun_f32", Shape32{1, 80, 100, 0, 203, 0.0f}, false); opt("cheb_big", -1);
  for (int64_t ng : kGrid32) {
    lists32("analysis_matfun_f32", Shape32{1, 40, 20, 0, ng, 0.0f}, false);      // letkf_cheb_kernel
    lists32("analysis_matfun_f32", Shape32{8, 40, 20, 0, ng, 0.0f}, false);      // letkf_cheb_rows_kernel
    lists32("weights_matfun_f32", Shape32{1, 40, 20, 0, ng, 0.0f}, true);        // letkf_cheb_weights_kernel
    lists32("analysis_matfun_f32", Shape32{1, 80, 100, 0, ng, 0.0f}, false);     // letkf_cheb_big_kernel
  }
  opt("tile", -1);
  section("analysis_packed_f32 / analysis_retry_f32 (letkf_sys.hip)");
  for (int k : {16, 64, 65})
    for (int p : {4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 65}) if (k == 64 || p == 20 || p == 65) {
      packed32(Shape32{1, k, p, 0, 203, 0.0f}, false, false);
      if (p == 20 || p == 65) packed32(Shape32{1, k, p, 0, 203, 0.0f}, true, false);
      if (k == 16 && p == 20) packed32(Shape32{1, k, p, 0, 203, 0.5f}, false, false);
    }
  packed32(Shape32{1, 40, 20, 0, 203, 0.0f}, false, true);
  for (int64_t ng : kGrid32) packed32(Shape32{1, 40, 20, 0, ng, 0.0f}, false, false);
  section("analysis_tiles_f32 (letkf_tile2.hip, letkf_tile2p.hip), weights_tiles_f32 (letkf_tile2w.hip), lketkf_rbf_analysis_tiles_f32 (lketkf_tile.hip)");
  for (int pair = 1; pair >= 0; --pair) {
    opt("tile_pair", pair);
    for (int k : {2, 16, 32, 48, 64, 80, 96, 97})
      for (int p : kRowBlocks) if (p <= k && (pair == 0 || p >= 25)) {      // (up to two row blocks the option changes nothing)
        tiles32(Shape32{1, k, p, 0, 203, 0.0f}, 0);
        if (p == 9) { tiles32(Shape32{1, k, p, 1, 203, 0.0f}, 0); tiles32(Shape32{2, k, p, 0, 203, 0.0f}, 0); }
      }
    opt("tile_pair", -1);
  }
  for (int k : {2, 16, 40, 64, 96, 97})
    for (int p : {0, 9, 25}) for (int extra : {0, 1}) if (p <= k) tiles32(Shape32{1, k, p, extra, 203, 0.0f}, 1);
  for (int k : {2, 8, 9, 16, 24, 32, 40, 41})
    for (int p : {0, 9, 25, 41, 57}) if (k >= 24 || p <= 25) tiles32(Shape32{1, k, p, 0, 203, 0.0f}, 2);
  for (int which = 0; which < 3; ++which)
    for (int64_t ng : kGrid32) tiles32(Shape32{1, 40, 20, 0, ng, 0.0f}, which);
  for (int64_t ng : kGrid32) tiles32(Shape32{1, 40, 40, 0, ng, 0.0f}, 0);      // (the pair kernel)
  section("float32 entries, option tile=0 / cheb_table=0");
  for (const char* name : {"tile", "cheb_table"}) {
    opt(name, 0);
    lists32("analysis_matfun_f32", Shape32{1, 40, 20, 0, 203, 0.0f}, false);
    for (int which = 0; which < 3; ++which) tiles32(Shape32{1, 40, 20, 0, 203, 0.0f}, which);
    opt(name, -1);
  }
}

// ---- the step entry: the fused tile kernel (letkf_tile2f.hip) and the segmented launches are reached through it alone --------------
static int allgather_cb(void*, const void* send, void* recv, size_t bytes, void*) { memcpy(recv, send, bytes); return 0; }
static int allreduce_cb(void*, int32_t*, int, void*) { return 0; }

static void step_entry() {
  section("mia_letkf_sharded_step_streams_f32: fused tile kernel, segmented launches");
  const int64_t G = 4000, P = 2000;
  const int k = 40;
  for (int scenario = 0; scenario < 6; ++scenario) {
    // 0: default (fused), 1: two state rows, 2: two coordinates, 3: pieces on per-point lists (segmented tile kernel),
    // 4: the same with tile=0 (segmented one-point kernel), 5: gamma > 0 (RBF tile kernel)
    const int m = scenario == 1 ? 2 : 1, n_coord = scenario == 2 ? 2 : 1, pieces = scenario == 3 || scenario == 4 ? 2 : 1;
    const float gamma = scenario == 5 ? 0.5f : 0.0f;
    mia_comm_t* comm = nullptr;
    if (pieces > 1 && mia_comm_create_custom(0, 1, allgather_cb, allreduce_cb, nullptr, &comm) != MIA_OK) abort();
    if (scenario == 4) opt("tile", 0);
    float *X = (float*)dmalloc(sizeof(float) * m * k * G), *Yb = (float*)dmalloc(sizeof(float) * k * (P + 1)), *d = (float*)dmalloc(sizeof(float) * (P + 1));
    float* Xa = (float*)dmalloc(sizeof(float) * m * k * G);
    double *grid = (double*)dmalloc(sizeof(double) * G * n_coord), *obs = (double*)dmalloc(sizeof(double) * (P + 1) * n_coord);
    for (int64_t g = 0; g < G * n_coord; ++g) grid[g] = (double)(g / n_coord);
    for (int64_t j = 0; j < P * n_coord; ++j) obs[j] = 2.0 * (double)(j / n_coord);
    size_t ws_bytes = 0;
    if (mia_letkf_sharded_step_workspace_bytes(G, m, k, P, n_coord, 1, pieces, 20, &ws_bytes) != MIA_OK) abort();
    void* ws = dmalloc(ws_bytes);
    int32_t *counters = (int32_t*)dmalloc(32), *flags = (int32_t*)dmalloc(sizeof(int32_t) * G);
    const int32_t cg[3] = {0, 0, 0};
    const double rc[3] = {10.0, 5.0, 2.5};
    for (int phase = 0; phase < 2; ++phase) {
      printf("# sharded_step_streams_f32 scenario=%d m=%d n_coord=%d pieces=%d gamma=%g phase=%d\n", scenario, m, n_coord, pieces, (double)gamma, phase);
      done(mia_letkf_sharded_step_streams_f32(X, G, m, k, Yb, d, P, grid, obs, n_coord, cg, rc, 1, 1e-5, 1.1f, gamma, 0, 20, comm, pieces, phase, Xa, flags, counters, ws,
                                              ws_bytes, S, (void*)0x1008, nullptr, pieces > 1 ? MIA_STEP_NO_TILE_LISTS : 0));
    }
    mia_letkf_step_workspace_release(ws);
    for (void* p : {(void*)X, (void*)Yb, (void*)d, (void*)Xa, (void*)grid, (void*)obs, ws, (void*)counters, (void*)flags}) hipFree(p);
    if (scenario == 4) opt("tile", -1);
    if (comm) mia_comm_destroy(comm);
  }
  mia_letkf_step_drain();
  mia_stub_trace_flush(stdout);
}

int main() {
  mia_stub_trace_enable(3);
  cross64();
  grids64();
  census();
  options64();
  float32_entries();
  step_entry();
  return 0;
}
