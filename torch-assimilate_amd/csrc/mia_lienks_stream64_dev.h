// What the two dense IEnKS tile kernels read of a point's incoming weights, shared: lienks_stream64.hip and
// lienks_patch64.hip (the same kernel under a tile map).  Both functions take the point's k x k matrix as a
// wave-uniform pointer; which point that is -- the tile's p0 + pt, or the map's entry -- is the caller's.
#pragma once
#include "mia_ring64_dev.h"

namespace mia {

// lienks_tile64.hip's threshold: a point of the transform variant is "at the prior" when
// max_ij |W_in[i][j] - w_mean_i - [i == j]| <= kStreamPriorTol.  An accepted deviation perturbs D = Wp^-1 Yl by at most k delta
// relative: 128 * 1e-14 = 1.3e-12 at the largest k of the route, two orders below the 1e-10 contract.
constexpr double kStreamPriorTol = 1e-14;

// Row means of one point's incoming weights, w_mean_i = (sum_j W[i][j] - 1) / k (_split_weights, core/ienks.py:46-54), for
// the four rows i = 16 tm + 4 q + h of member block tm, in lienks64_row_means' summation order: the sixteen lanes (lr) of lane
// group h share row i, lane lr adds columns lr, lr + 16, ... ascending, then the butterfly; all sixteen end up with the mean.
// take: this lane keeps the means in wm4 (0 for rows beyond k: they meet zero A operands in the product).  Four rows a call:
// 4 KT loads in flight, and the caller's loop over points keeps it at that.
template <int KT>
__device__ __forceinline__ void lienks_stream64_row_means(const double* win, int k, int tm, int lr, int h, bool take,
                                                          d4t& wm4) {
  double s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // (a wave-uniform 64-bit row group plus ONE 32-bit lane offset h k + lr, as the stores below: clamped row and column
    //  indices, or a 64-bit address per row, would be registers for the compiler to carry from in front of every loop.  Only
    //  the last row and column blocks are ragged; what lies beyond k is not read.)
    const bool rok = tm < KT - 1 || 16 * tm + 4 * q + h < k;
    const char* row = reinterpret_cast<const char*>(win + (16 * tm + 4 * q) * k);      // wave-uniform
    const unsigned loff = (unsigned)(h * k + lr) * 8u;                                  // 32-bit lane offset in bytes
    s[q] = 0.0;
#pragma unroll
    for (int jj = 0; jj < KT; ++jj) {
      double v = 0.0;
      if (rok && (jj < KT - 1 || lr + 16 * jj < k)) v = *reinterpret_cast<const double*>(row + (loff + 128u * jj));
      s[q] += v;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool rok = tm < KT - 1 || 16 * tm + 4 * q + h < k;
    s[q] += __shfl_xor(s[q], 1, 64);
    s[q] += __shfl_xor(s[q], 2, 64);
    s[q] += __shfl_xor(s[q], 4, 64);
    s[q] += __shfl_xor(s[q], 8, 64);
    const double wm = rok ? (s[q] - 1.0) / double(k) : 0.0;
    wm4[q] = take ? wm : wm4[q];
  }
}

// max_ij |W[i][j] - w_mean_i - [i == j]| over the elements this lane sees (NaN where an element is not a number), the means
// in the order above: the prior test of the transform variant.  Four rows a trip, one per lane group.
template <int KT>
__device__ __forceinline__ double lienks_stream64_prior_dev(const double* win, int k, int lr, int h) {
  double dev = 0.0;
#pragma clang loop unroll(disable)
  for (int i0 = 0; i0 < k; i0 += 4) {
    const int i = i0 + h;
    const bool rok = i < k;
    const char* row = reinterpret_cast<const char*>(win + i0 * k);                     // wave-uniform
    const unsigned loff = (unsigned)(h * k + lr) * 8u;                                  // 32-bit lane offset in bytes
    double wv[KT];
    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < KT; ++jj) {
      double v = 0.0;
      if (rok && (jj < KT - 1 || lr + 16 * jj < k)) v = *reinterpret_cast<const double*>(row + (loff + 128u * jj));
      wv[jj] = v;
      s += v;
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    const double wm = (s - 1.0) / double(k);
#pragma unroll
    for (int jj = 0; jj < KT; ++jj) {
      const int j = lr + 16 * jj;
      const double e = fabs(wv[jj] - wm - (i == j ? 1.0 : 0.0));
      if (rok && j < k) dev = (e > dev || e != e) ? e : dev;
    }
  }
  return dev;
}

}  // namespace mia
