// The launches of mia_lienks_update_patch_f64 (tests/test_ienks_patch64_cover.py): the entry called on ONE thread against the stub HIP
// runtime of hip_stub.cc with its call trace switched on, as launch_trace_driver.cc does for the other tile entries.  Per call a header
// line "# k=.. p_max=.. n_tiles=.. union_blocks=..", the launch the runtime saw (kernel name with template argument, grid, block, LDS
// bytes, stream) and a line with the return code and the string mia_last_analysis_kernel returns afterwards.  The test restates what
// each line must say; nothing here is compared with a recorded file.  The array arguments are a few bytes of host memory that the
// entry neither reads nor writes on the host.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "mia_letkf.h"

extern "C" void mia_stub_trace_enable(int on);
extern "C" void mia_stub_trace_flush(FILE* to);

static void* const S = (void*)0x1000;
alignas(256) static char g_dummy[256];
template <typename T> static T* dummy() { return reinterpret_cast<T*>(g_dummy); }

static void call(int k, int p_max, int64_t n_tiles, int ub, double eps, int64_t w_stride) {
  printf("# k=%d p_max=%d n_tiles=%lld union_blocks=%d\n", k, p_max, (long long)n_tiles, ub);
  const int rc = mia_lienks_update_patch_f64(dummy<double>(), w_stride, k, 0, 203, dummy<double>(), 1000, dummy<int32_t>(), dummy<int32_t>(),
                                             dummy<double>(), 512, p_max, eps, dummy<double>(), dummy<int32_t>(), dummy<int32_t>(),
                                             dummy<int32_t>(), n_tiles, ub, S);
  char name[160];
  mia_stub_trace_flush(stdout);
  mia_last_analysis_kernel(name, (int)sizeof name);
  printf("= %d \"%s\"\n", rc, name);
}

int main() {
  mia_stub_trace_enable(3);
  const int64_t kTiles = (int64_t)65536 * 65535;      // the last grid that fits
  // one call per number of member blocks and per edge of the image, both variants and both strides among them
  for (int k : {2, 16, 32, 48, 64, 80, 96, 112, 128})
    for (int ub : {1, 16}) call(k, k + 1, 13, ub, ub == 1 ? 0.01 : 0.0, ub == 1 ? (int64_t)k * k : 0);
  for (int64_t nt : {(int64_t)1, (int64_t)65536, (int64_t)65537, kTiles, kTiles + 1}) call(16, 40, nt, 8, 0.01, 0);
  return 0;
}
