// Issue rate and dependent latency of v_mfma_f64_16x16x4_f64 (the instruction of csrc/letkf_tile64.hip), next to
// v_mfma_f32_16x16x4_f32 as the yardstick (32 cycles per instruction and SIMD, tools/mfma_rate.hip).  Builtins only.
//   build (anywhere):  hipcc --offload-arch=gfx950 -O3 -std=c++17 -o mfma_rate_f64 tools/mfma_rate_f64.hip
//   run (GPU):         ./mfma_rate_f64 > profiles/tile64_mfma_rate.txt
// One workgroup, W waves per SIMD; every wave runs `iters` trips of NACC independent accumulators (NACC = 1: the dependent
// chain) and stamps s_memtime / s_memrealtime around the loop.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef double d4t __attribute__((ext_vector_type(4)));
typedef float f4t __attribute__((ext_vector_type(4)));

template <int NACC, bool F64>
__global__ void __launch_bounds__(1024) rate_kernel(int iters, float seed, long long* out, double* sink) {
  d4t accd[NACC];
  f4t accf[NACC];
  for (int i = 0; i < NACC; ++i) {
    accd[i] = d4t{seed, seed, seed, seed};
    accf[i] = f4t{seed, seed, seed, seed};
  }
  const double ad = seed * 1e-3 + threadIdx.x * 1e-6, bd = seed * 0.5e-3;
  const float af = (float)ad, bf = (float)bd;
  __syncthreads();
  const long long t0 = __builtin_amdgcn_s_memtime();
  const long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 8 / NACC; ++r)
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        if constexpr (F64) accd[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad, bd, accd[j], 0, 0, 0);
        else accf[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, accf[j], 0, 0, 0);
      }
  }
  double s = 0.0;
  for (int i = 0; i < NACC; ++i) s += accd[i][0] + accd[i][1] + accd[i][2] + accd[i][3] + accf[i][0] + accf[i][1] + accf[i][2] + accf[i][3];
  const long long t1 = __builtin_amdgcn_s_memtime();
  const long long r1 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0) {
    out[(threadIdx.x >> 6) * 2] = t1 - t0;
    out[(threadIdx.x >> 6) * 2 + 1] = r1 - r0;
  }
  if (s == 12345.678) sink[threadIdx.x] = s;
}

template <int NACC, bool F64>
static double run(const char* what, int waves_per_simd, long long* dout, double* sink) {
  const int iters = 2000, nw = 4 * waves_per_simd;
  rate_kernel<NACC, F64><<<1, 64 * nw>>>(iters, 1.0f, dout, sink);
  rate_kernel<NACC, F64><<<1, 64 * nw>>>(iters, 1.0f, dout, sink);
  std::vector<long long> h(2 * nw);
  if (hipMemcpy(h.data(), dout, sizeof(long long) * 2 * nw, hipMemcpyDeviceToHost) != hipSuccess) exit(1);
  long long tmax = 0, rmax = 0;
  for (int w = 0; w < nw; ++w) { if (h[2 * w] > tmax) tmax = h[2 * w]; if (h[2 * w + 1] > rmax) rmax = h[2 * w + 1]; }
  const double per_inst = (double)tmax / iters / 8.0 / waves_per_simd, us = rmax / 100.0;
  printf("%-52s waves/SIMD %d: %7.2f ticks per instruction and SIMD (%.1f ticks/us, %.1f us)\n", what, waves_per_simd, per_inst,
         tmax / us, us);
  return per_inst;
}

int main() {
  long long* dout; double* sink;
  if (hipMalloc(&dout, 4096) != hipSuccess || hipMalloc(&sink, 8192) != hipSuccess) return 1;
  for (int w = 1; w <= 2; ++w) {
    const double f32 = run<8, false>("8 independent v_mfma_f32_16x16x4_f32", w, dout, sink);
    const double f64 = run<8, true>("8 independent v_mfma_f64_16x16x4_f64", w, dout, sink);
    const double f64_2 = run<2, true>("2 independent v_mfma_f64_16x16x4_f64", w, dout, sink);
    const double f64_1 = run<1, true>("dependent chain of v_mfma_f64_16x16x4_f64", w, dout, sink);
    printf("  -> f64 / f32 issue ratio %.2f: with 32 cycles for the f32 form, %.1f cycles per f64 instruction and SIMD; two "
           "accumulators %.1f, dependent chain %.1f\n", f64 / f32, 32.0 * f64 / f32, 32.0 * f64_2 / f32, 32.0 * f64_1 / f32);
  }
  return 0;
}
