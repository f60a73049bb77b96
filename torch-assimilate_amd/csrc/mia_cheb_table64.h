// Float64 Chebyshev coefficient tables of the tile routes (letkf_tile64.hip: dual pair; letkf_dense64.hip: primal pair).
// The grid of letkf_cheb.hip (geometric in T = L / reg, kTabPerOctave per octave over 2^-24 .. 2^8, Gauss-node cosine
// transform), stored unrounded as double2 with kTab64Deg entries per row.  Truncation target exp(-26), degrees up to 127:
// DESIGN 2.8.  The degree depends on T only, so both tables have the same headers; what differs is the pair of functions of
// u = sqrt(1 + t):
//   kTab64Dual    (-1 / (u (1 + u)), 1 / u^2)     functions of S = D G D, applied to Z (letkf_tile64.hip)
//   kTab64Primal  ( 1 / u,           1 / u^2)     functions of C = Yw^T diag(rho) Yw, applied to x' (letkf_dense64.hip)
// Every function here is static: a translation unit that includes this header owns its table (one per device).
#pragma once
#include "mia_common.h"
#include "mia_kernels.h"
#include "mia_options.h"

#include <mutex>
#include <vector>

namespace mia {

constexpr int kTab64Deg = 128;
constexpr double kTab64LogTol = 26.0;
constexpr int kTab64Margin = 2;
constexpr int kTab64Dual = 0, kTab64Primal = 1;
struct Tab64Hdr { int deg; int pad; double two_over_T; };

__global__ __launch_bounds__(kTab64Deg) static void cheb_table64_kernel(Tab64Hdr* hdr, double2* c, double log_tol, int margin, int fn) {
  __shared__ double fs[kTab64Deg][2];
  const int idx = blockIdx.x, tid = threadIdx.x;
  const double T = exp2(double(idx - kTabIdx0) / double(kTabPerOctave));
  const double sq = sqrt(1.0 + T);
  const double rho = (sq + 1.0) / fmax(sq - 1.0, 1e-12);
  double dd = ceil(log_tol / log(rho)) + (double)margin;
  dd = dd < 3.0 ? 3.0 : (dd > 32767.0 ? 32767.0 : dd);
  const int deg = (int)dd;
  if (tid == 0) { Tab64Hdr hd; hd.deg = deg; hd.pad = 0; hd.two_over_T = 2.0 / T; hdr[idx] = hd; }
  c[(size_t)idx * kTab64Deg + tid] = make_double2(0.0, 0.0);
  if (deg > kTab64Deg - 1) return;                    // the kernels decline such points (eigensolver route)
  const int N = deg + 1;
  if (tid < N) {
    const double x = cospi((tid + 0.5) / double(N));
    const double u = sqrt(0.5 * T * (x + 1.0) + 1.0);   // sqrt(t + 1)
    fs[tid][0] = fn == kTab64Primal ? 1.0 / u : -1.0 / (u * (1.0 + u));
    fs[tid][1] = 1.0 / (u * u);
  }
  __syncthreads();
  if (tid < N) {
    double a0 = 0.0, a1 = 0.0;
    for (int i = 0; i < N; ++i) {
      const double cs = cospi(double((long long)tid * (2 * i + 1) % (4LL * N)) / double(2 * N));
      a0 += fs[i][0] * cs; a1 += fs[i][1] * cs;
    }
    const double sc = (tid == 0 ? 1.0 : 2.0) / double(N);
    c[(size_t)idx * kTab64Deg + tid] = make_double2(a0 * sc, a1 * sc);
  }
}

struct CoefTable64 { int device; int fn; Tab64Hdr* hdr; double2* c; };
// nullptr when the table cannot be had (allocation failure, stream being captured, option cheb_table = 0): the route then
// reports MIA_ERR_UNSUPPORTED and the caller takes the next kernel.  Built synchronously on first use, one per device and selector.
static const CoefTable64* cheb_coef_table64(hipStream_t stream, int fn) {
  static std::mutex mu;
  static std::vector<CoefTable64*> tabs;
  if (!option(MIA_OPT_CHEB_TABLE)) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lock(mu);
  for (const CoefTable64* t : tabs)
    if (t->device == dev && t->fn == fn) return t;
  if (tabs.size() >= 64) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
  CoefTable64* t = new CoefTable64{dev, fn, nullptr, nullptr};
  if (hipMalloc((void**)&t->hdr, sizeof(Tab64Hdr) * kTabN) != hipSuccess ||
      hipMalloc((void**)&t->c, sizeof(double2) * kTabN * kTab64Deg) != hipSuccess) {
    (void)hipGetLastError();
    if (t->hdr) (void)hipFree(t->hdr);
    delete t;
    return nullptr;
  }
  cheb_table64_kernel<<<dim3(kTabN), dim3(kTab64Deg), 0, stream>>>(t->hdr, t->c, kTab64LogTol, kTab64Margin, fn);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(t->hdr); (void)hipFree(t->c);
    delete t;
    return nullptr;
  }
  tabs.push_back(t);
  return t;
}

// ---- lane helpers of the f64 matrix instruction's layout: lane (lr, h) = (lane & 15, lane >> 4) ------------------------------
using d4t = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ double tile64_add_h(double v) {       // sum over the four lanes (lr, h = 0..3), in every one of them
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ double tile64_max_h(double v) {       // maximum over the same four lanes, NaN wins
  double o = __shfl_xor(v, 16, 64);
  v = (o > v || o != o) ? o : v;
  o = __shfl_xor(v, 32, 64);
  return (o > v || o != o) ? o : v;
}
__device__ __forceinline__ unsigned tile64_wave_max_u32(unsigned u) {     // wave-uniform maximum (DPP, see mia_common.h)
  unsigned t;
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xf, 0xf, false); u = u > t ? u : t;
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x4E, 0xf, 0xf, false); u = u > t ? u : t;
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x124, 0xf, 0xf, false); u = u > t ? u : t;
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x128, 0xf, 0xf, false); u = u > t ? u : t;
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)u, 0), b = (unsigned)__builtin_amdgcn_readlane((int)u, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)u, 32), d = (unsigned)__builtin_amdgcn_readlane((int)u, 48);
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

#define MIA_MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

}  // namespace mia
