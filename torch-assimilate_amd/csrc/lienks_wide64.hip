// The localised IEnKS weight update with tau = 1 in FLOAT64 for ensembles of 65 .. 128 members (and below, for comparison),
// sixteen grid points per WORKGROUP of NW wavefronts, every contraction on the matrix cores (v_mfma_f64_16x16x4_f64), without
// an eigensolver: what IEnKSTransformModule / IEnKSBundleModule.forward (core/ienks.py:108-141, 167-173) return on the
// localised block under LocalizedIEnKS*.inner_loop (interface/lienks.py:75-118).  With tau = 1, reg = k - 1, D = Yl (transform
// variant, while Wp = I) or D = Yl / eps (bundle variant) and S = D^T D:
//
//     Wp'     = I + D phi(S) D^T,     w_mean' = D psi(S) (d_l + D^T w_mean),     W' = w_mean' 1^T + Wp'
//
// i.e. the LETKF weights at inflation 1 with the innovations shifted by D^T w_mean.
//
// The frame is letkf_wide64w.hip's, statement for statement: per-point lists of any metric, union by rank
// extraction, ONE record image per workgroup with the compile-time pitch 16 KT + 5, the row blocks of the union dealt over the
// NW waves in runs of TW = ceil(UT / NW), G = Yw Yw^T for the wave's block columns, D^2, Gershgorin bound, table row -> alpha,
// degree and decline of every point, the exchange buffer bx in the dead sqrt(rho) table with two barriers per recurrence step,
// one pass per MEMBER c < k, the stores.  (A copy, not a template switch: the weights kernel's code object stays what it was.)
// Lane roles, the canonical summation order -- every sum over the union is ONE ascending accumulator chain over (tk, q), so a
// point's bits depend on neither tile, shard nor NW -- and the instruction discipline (every product step unconditional, no
// branch between a matrix instruction and the first vector read of its result; builtins only) are described in
// letkf_wide64.hip.
//
// What differs is lienks_tile64.hip's, placed into this frame:
//
//     w_mean_i = (sum_j W_in[i][j] - 1) / k    per point (or once, for ONE shared matrix: w_stride = 0), in lienks_tile64.hip's
//                                     order: lane lr adds columns lr, lr + 16, ..., then a butterfly over the sixteen lanes of a
//                                     row -- an order that depends on (i, j) alone.  EVERY wave reads W_in and forms the means
//                                     of all sixteen points itself (the B operand wmv[4 tm + q], 8 KT registers, live through
//                                     the Gram loop only): no LDS, no barrier, and the re-reads come from L2
//     zs[i]    = MFMA(ao[i], wb, zs[i])        the shift z = Yw w_mean for the wave's OWN row blocks: one more accumulator chain
//                                     per block in the Gram loop, on the A operands of G[.][i], unconditional
//     ed[i][r] = (d_b s + zs[i][r]) D^2        s = 1 (transform) or eps (bundle), read off the accumulators before any branch.
//                                     In lienks_tile64.hip e lies over the dead sqrt(rho) table; here that table is bx, so e
//                                     stays in registers (8 TW through the member loop) and costs neither LDS nor a barrier
//     wm_c     = sum_b e_b psi_b      each wave publishes e o Psi of its own blocks through bx (the weights kernel publishes
//                                     D^2 o Psi), and the chain that every wave runs whole takes a block of ONES as the A
//                                     operand (the weights kernel: the innovations in row 0): every row of the result block is
//                                     the sum, in the canonical order
//     sqrt(rho) enters Dl as sqrt(rho) / eps (bundle): bound, table row and degree are those of the scaled S
//     W'[g][c][j] = wm_c + [c == j] + (Yw^T (D^2 o Phi))_j
//
// A point without observations gets its W_in back bit for bit, flag 0 (core/ienks.py:135), copied by the whole workgroup, and
// takes no part in the tile; a tile without an active point returns before the union -- every wave holds the same lists and
// takes the same decision, before the first barrier.  Transform variant: a point with observations whose Wp is not the identity
// (kPriorTol below) is declined whole like a point whose degree exceeds the table's cap: MIA_FLAG_RETRY, counted once, W_out
// untouched; the general kernel redoes them (mia_lienks_update_retry_f64).  Every wave scans every point itself, so the verdict
// is in every wave before the first barrier.  A tile that holds a non-finite record is done point by point, so that
// MIA_FLAG_NONFINITE stays with the points that use the record.  Every barrier is reached by all waves on every path: the
// member loop's trip count is k, degmax is the same in every wave.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

// lienks_tile64.hip's threshold: a point of the transform variant is "at the prior" when
// max_ij |W_in[i][j] - w_mean_i - [i == j]| <= kPriorTol.  An accepted deviation perturbs D = Wp^-1 Yl by at most k delta
// relative: 128 * 1e-14 = 1.3e-12 at the largest k of the route, two orders below the 1e-10 contract.
constexpr double kPriorTol = 1e-14;

struct LienksWide64Params {
  int k; int kp;
  int64_t ng;
  const double* Win; int64_t w_stride;     // [ng][k][k], or one [k][k] for all points when w_stride == 0
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  int transform;                           // 1: transform variant (D = Yl while Wp = I), 0: bundle variant (D = Yl / eps)
  double dscale, dshift;                   // 1 / eps and eps (bundle), 1 and 1 (transform)
  double reg, inv_reg, f0, cs_phi, cs_psi;
  double* W; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// Row means of one point's incoming weights, w_mean_i = (sum_j W[i][j] - 1) / k (_split_weights, core/ienks.py:46-54), for
// the four rows i = 16 tm + 4 q + h of member block tm, in lienks64_row_means' summation order: the sixteen lanes (lr) of lane
// group h share row i, lane lr adds columns lr, lr + 16, ... ascending, then the butterfly; all sixteen end up with the mean.
// take: this lane keeps the means in wm4.  (Rows beyond k give junk: the Gram loop's member predicate keeps it out of the
// product.)  Four rows a call: 4 KT loads in flight, and the caller's loop over points keeps it at that.
template <int KT>
__device__ __forceinline__ void lienks_wide64_row_means(const double* win, int k, int tm, int lr, int h, bool take,
                                                        double (&wm4)[4]) {
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
    s[q] += __shfl_xor(s[q], 1, 64);
    s[q] += __shfl_xor(s[q], 2, 64);
    s[q] += __shfl_xor(s[q], 4, 64);
    s[q] += __shfl_xor(s[q], 8, 64);
    const double wm = (s[q] - 1.0) / double(k);
    wm4[q] = take ? wm : wm4[q];
  }
}

// max_ij |W[i][j] - w_mean_i - [i == j]| over the elements this lane sees (NaN where an element is not a number), the means
// in the order above: the prior test of the transform variant.  Four rows a trip, one per lane group.
template <int KT>
__device__ __forceinline__ double lienks_wide64_prior_dev(const double* win, int k, int lr, int h) {
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

// UT: 16-slot blocks of the union the workgroup holds; KT = ceil(k / 16); NW: wavefronts of the workgroup.  One workgroup's
// waves sit on different SIMDs, one wave per SIMD: up to 512 registers each.
template <int UT, int KT, int NW>
__global__ __launch_bounds__(64 * NW, 1) void lienks_wide64_kernel(LienksWide64Params P) {
  constexpr int UMAX = 16 * UT, NU = 4 * UT, DS = UMAX + 1, TW = (UT + NW - 1) / NW, NT = 64 * NW;
  // odd row pitch (in doubles) of the record image: the largest kp | 1 of this KT, so that every LDS address below is a
  // base register plus an immediate
  constexpr int KS = 16 * KT + 5;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: what depends on it is scalar selects and branches)
  const int k = P.k, kp = P.kp, pm = P.p_max;
  double* Yw = reinterpret_cast<double*>(smem_raw);          // [UMAX][KS] union records, zero rows beyond the union
  double* Dl = Yw + UMAX * KS;                               // [16][DS]   sqrt(rho) [/ eps] of (point, slot), 0 = not local
  double* bx = Dl;                                           // [4 UT][64] the exchange buffer: B operands of steps (tk, q), once Dl is dead
  double* xch = Dl + 16 * DS;                                // [NW][16]   per-column scalars that cross the waves
  int* ukey = reinterpret_cast<int*>(xch + NW * 16);         // [UMAX]     observation index of a slot, -1 = unused
  int* nf = ukey + UMAX;                                     // [NW]       a wave met a non-finite record

  // XCD-aware block -> tile map: blocks b, b + 8, ... share an XCD (and its L2) and take consecutive tiles, whose
  // records overlap
  const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t ntile = (P.ng + 15) >> 4;
  if (bid >= ntile) return;
  const int64_t q8 = ntile >> 3, r8 = ntile & 7, xcd = bid & 7;
  const int64_t tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int64_t p0 = tile << 4;                              // first point of the tile (index into the launch's ng points)
  const int npts = P.ng - p0 < 16 ? (int)(P.ng - p0) : 16;
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;
  const unsigned kk8 = (unsigned)(k * k) * 8u;               // bytes of one point's weights
  const bool shared_w = P.w_stride == 0;

  // the wave's own row blocks (clamped to a block that exists) and whether they are its to publish
  int to[TW];
  bool own[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    own[i] = wv * TW + i < UT;
    to[i] = own[i] ? wv * TW + i : UT - 1;
  }

  // ---- the tile's neighbour lists, in every wave alike: lane (lp, sub) holds entries sub, sub + 4, ... of point lp
  //      (unconditional loads inside the row's storage; entries beyond the count become index -1)
  const int nl = pm < P.p_cap ? pm : P.p_cap;
  int eidx[NU];
  double ew[NU / NW];      // sqrt(rho) of entries u = NW u2 + wv only: the ones this wave lays into the table below
  int lcnt;
  unsigned long long skipmask;       // bit 4 p: point p takes no part in the tile (overflow, no observation, declined here)
  {
    const int64_t row = p0 + (lp < npts ? lp : 0);          // (lists, flags and weights count from the shard's g0)
    lcnt = P.cnt[row];
    const int32_t* ib = P.idx + row * P.p_cap;
    const double* wb = P.w + row * P.p_cap;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int pos = sub + 4 * u;
      eidx[u] = ib[pos < nl ? pos : 0];
    }
#pragma unroll
    for (int u2 = 0; u2 < NU / NW; ++u2) {
      const int pos = sub + 4 * (NW * u2 + wv);
      ew[u2] = wb[pos < nl ? pos : 0];
    }
    const bool pbad = lp < npts && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad && wv == 0) {
      if (sub == 0) P.flags[p0 + lp] = MIA_FLAG_OVERFLOW;
      const double nanv = __builtin_nan("");
      double* wp = P.W + (p0 + lp) * (int64_t)(k * k);
      for (int it = sub; it < k * k; it += 4) wp[it] = nanv;
    }
    if (lp >= npts || pbad) lcnt = 0;
    // ---- no local observation: the weights go back as they came (core/ienks.py:135), the whole workgroup copying a point
    const unsigned long long emask = __ballot(lp < npts && !pbad && lcnt == 0);
    skipmask = __ballot(pbad) | emask;
    for (int pt = 0; pt < npts; ++pt) {
      if (!((emask >> (4 * pt)) & 1ull)) continue;
      const double* win = P.Win + (p0 + pt) * P.w_stride;
      double* wout = P.W + (p0 + pt) * (int64_t)(k * k);
      for (int it = tid; it < k * k; it += NT) wout[it] = win[it];
      if (tid == 0) P.flags[p0 + pt] = 0;
    }
    // ---- transform variant: D = Wp^-1 Yl is Yl only at the prior; any other point with observations is the general
    //      kernel's.  Every wave scans every point: the verdict needs no exchange.
    if (P.transform) {
      unsigned np = 0u;                                      // bit p: point p is not at the prior
      const int nscan = shared_w ? 1 : npts;
      for (int pt = 0; pt < nscan; ++pt) {
        if (!shared_w && ((skipmask >> (4 * pt)) & 1ull)) continue;
        const double dev = lienks_wide64_prior_dev<KT>(P.Win + (p0 + pt) * P.w_stride, k, lr, h);
        if (__any(!(dev <= kPriorTol))) np |= shared_w ? 0xffffu : (1u << pt);
      }
      const bool pnot = lp < npts && lcnt > 0 && ((np >> lp) & 1u);
      if (pnot && sub == 0 && wv == 0) {
        P.flags[p0 + lp] = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
      if (pnot) lcnt = 0;
      skipmask |= __ballot(pnot);
    }
    if (!__any(lcnt > 0)) return;                            // nothing left to update in this tile (in every wave alike)
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (sub + 4 * u >= lcnt) eidx[u] = -1;
  }

  const bool colok = lr < npts && !((skipmask >> (4 * lr)) & 1ull);
  // the flag word of column lr: wave-uniform base + 32-bit lane offset, like the stores of W (no 64-bit address per lane to
  // carry through the loop)
  auto col_flag = [&]() -> int32_t& {
    return *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(P.flags + p0) + (unsigned)lr * 4u);
  };

  int lo = 0;
#pragma clang loop unroll(disable)
  while (lo < npts) {
    // ---- union of the lists of points [lo, hi): slot = RANK of the observation index, found by repeated extraction of
    //      the smallest remaining key (one DPP reduction per slot), in every wave alike (the trip counts and every decision
    //      below are therefore the same in all waves); shrink the range until the union fits
    int n = 16, hi, U;
    int es[NU];            // slot of this lane's entries
    for (;;) {
      hi = lo + n < npts ? lo + n : npts;
      const bool act = lp >= lo && lp < hi;
      unsigned key1[NU];   // index + 1 of an entry that takes part, 0 otherwise
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        es[u] = -1;
        key1[u] = (act && eidx[u] >= 0) ? (unsigned)eidx[u] + 1u : 0u;
      }
      for (int i = tid; i < UMAX; i += NT) ukey[i] = -1;
      __syncthreads();
      U = 0;
      unsigned last = 0u;
#pragma clang loop unroll(disable)
      for (;;) {
        unsigned best = 0u;                       // ~(smallest key above `last`), 0 = none left
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const unsigned cand = key1[u] > last ? ~key1[u] : 0u;
          best = cand > best ? cand : best;
        }
        best = tile64_wave_max_u32(best);
        if (best == 0u) break;
        last = ~best;
        if (U < UMAX) {
#pragma unroll
          for (int u = 0; u < NU; ++u)
            if (key1[u] == last) es[u] = U;
          if (tid == 0) ukey[U] = (int)(last - 1u);
        }
        ++U;
        if (U > UMAX) break;
      }
      if (U > UMAX) { __syncthreads(); n >>= 1; continue; }     // (n = 1 always fits: a single list has at most UMAX entries)
      __syncthreads();
      // ---- the union's records, four rows per wave and trip: lane group h takes row r0 + h, its sixteen lanes the columns
      double fin = 0.0;       // stays 0 while every value is finite (inf * 0 = NaN)
#pragma clang loop unroll_count(2)
      for (int r0 = 4 * wv; r0 < UMAX; r0 += 4 * NW) {
        const int r = r0 + h;
        const int key = ukey[r];
        const double* src = P.rec + (int64_t)(key < 0 ? 0 : key) * kp;
        for (int c = lr; c < kp; c += 16) {
          double v = 0.0;
          if (key >= 0) v = src[c];
          fin = fma(v, 0.0, fin);
          Yw[r * KS + c] = v;
        }
      }
      const int wbad = __any(fin != fin) ? 1 : 0;
      if (lane == 0) nf[wv] = wbad;
      for (int i = tid; i < 16 * DS; i += NT) Dl[i] = 0.0;
      __syncthreads();
      // A non-finite record would reach EVERY column of the tile through the shared Gram matrix (NaN * 0 = NaN), also the
      // points that do not see that observation.  Such a tile is done point by point: the union is then the point's
      // own list and the damage stays where the reference has it.
      int anybad = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) anybad |= nf[w];
      if (anybad && hi - lo > 1) { __syncthreads(); n = 1; continue; }
      break;
    }
#pragma unroll
    for (int u2 = 0; u2 < NU / NW; ++u2) {
      int e = es[NW * u2];                                   // slot of entry NW u2 + wv
#pragma unroll
      for (int w = 1; w < NW; ++w) e = wv == w ? es[NW * u2 + w] : e;
      if (e >= 0) Dl[lp * DS + e] = ew[u2] * P.dscale;
    }
    __syncthreads();
    const bool colact = colok && lr >= lo && lr < hi;
    // ---- w_mean of the points of this pass, in every wave: wmv[4 tm + q] = w_mean[point lr][member 16 tm + 4 q + h], the B
    //      operand of the shift (0 for points that take no part).  Closed before the first matrix instruction of the pass.
    double wmv[4 * KT];
#pragma unroll
    for (int tm = 0; tm < KT; ++tm) {
      double wm4[4] = {0., 0., 0., 0.};
      const int nscan = shared_w ? 1 : hi;
#pragma clang loop unroll(disable)
      for (int pt = shared_w ? 0 : lo; pt < nscan; ++pt) {
        if (!shared_w && ((skipmask >> (4 * pt)) & 1ull)) continue;
        // (lo and hi come out of the union's wave reductions: the same in every lane, but only this tells the compiler so,
        //  and with it that the matrix' address is a scalar)
        const int ptu = __builtin_amdgcn_readfirstlane(pt);
        lienks_wide64_row_means<KT>(P.Win + (p0 + ptu) * P.w_stride, k, tm, lr, h, shared_w || lr == pt, wm4);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) wmv[4 * tm + q] = wm4[q];
    }
    d4t d2[TW];             // D^2 of column lr, slots 16 to[i] + h + 4 r
    // ---- G = Yw Yw^T, the wave's block columns: G[tk][i][r] = Gram[16 tk + h + 4 r][16 to[i] + lr]; beside it the shift
    //      z = Yw w_mean of the wave's own row blocks, zs[i][r] = z[16 to[i] + h + 4 r][point lr], on the same A operands
    d4t G[UT][TW], zs[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i) zs[i] = d4t{0., 0., 0., 0.};
#pragma unroll
    for (int t1 = 0; t1 < UT; ++t1)
#pragma unroll
      for (int i = 0; i < TW; ++i) G[t1][i] = d4t{0., 0., 0., 0.};
#pragma unroll
    for (int tm = 0; tm < KT; ++tm)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mem = 16 * tm + 4 * q + h;
        const bool ok = tm < KT - 1 || mem < k;            // (innovation / pad columns are not members; only the last block is ragged)
        const int col = ok ? mem : 0;
        double av[UT], ao[TW];
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          const double v = Yw[(16 * t + lr) * KS + col];
          av[t] = ok ? v : 0.0;
        }
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          const double v = Yw[(16 * to[i] + lr) * KS + col];
          ao[i] = ok ? v : 0.0;
        }
        const double wb = ok ? wmv[4 * tm + q] : 0.0;
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
          for (int t1 = 0; t1 < UT; ++t1) G[t1][i] = MIA_MFMA64(av[t1], ao[i], G[t1][i]);
#pragma unroll
        for (int i = 0; i < TW; ++i) zs[i] = MIA_MFMA64(ao[i], wb, zs[i]);
      }
    // the shifted innovation of (slot, point), d_b s + z: read off the accumulators before any branch; multiplied by D^2 below
    d4t ed[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) ed[i][r] = Yw[(16 * to[i] + h + 4 * r) * KS + k] * P.dshift + zs[i][r];
    // ---- Gershgorin bound of every point: L_g = max_a w_a sum_b |G_ab| w_b over the wave's rows a, then over the waves
    double alpha;
    int deg, tab_idx, pflag = 0;
    bool decl;
    {
      d4t dreg[UT], dro[TW], R[TW];
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dreg[t][r] = Dl[lr * DS + 16 * t + h + 4 * r];
#pragma unroll
      for (int i = 0; i < TW; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dro[i][r] = Dl[lr * DS + 16 * to[i] + h + 4 * r];
        R[i] = d4t{0., 0., 0., 0.};
      }
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int i = 0; i < TW; ++i) R[i] = MIA_MFMA64(fabs(G[tk][i][q]), dreg[tk][q], R[i]);
      double L = 0.0;
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = dro[i][r] * R[i][r];
          L = (v > L || v != v) ? v : L;
          d2[i][r] = dro[i][r] * dro[i][r];
          ed[i][r] = ed[i][r] * d2[i][r];                  // e = (d s + z) D^2
        }
      L = tile64_max_h(L);
      if (h == 0) xch[wv * 16 + lr] = L;
      __syncthreads();                                     // (every wave has its D in registers: Dl is dead, bx may be written)
      L = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const double v = xch[w * 16 + lr];
        L = (v > L || v != v) ? v : L;
      }
      L = fmax(L, 1e-300 * P.reg) * (1.0 + 1e-12);
      if (!(L == L) || !(fabs(L) < 1e300)) { pflag |= MIA_FLAG_NONFINITE; L = P.reg; }
      tab_idx = (int)ceil(double(kTabPerOctave) * log2(L * P.inv_reg)) + kTabIdx0;
      tab_idx = tab_idx < 0 ? 0 : (tab_idx > kTabN - 1 ? kTabN - 1 : tab_idx);      // (the last entries decline: T = 2^8)
      const Tab64Hdr hd = P.tab_hdr[tab_idx];
      deg = hd.deg;
      decl = colact && (deg > P.dmax || deg > kTab64Deg - 1);
      alpha = (deg > kTab64Deg - 1) ? 0.0 : hd.two_over_T * P.inv_reg;             // (a declined column carries bounded junk)
      if (decl && h == 0 && wv == 0) {
        col_flag() = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
    }
    // (deg, decl and colact are the same in every wave, so degmax is)
    const int degmax = (int)tile64_wave_max_u32((colact && !decl) ? (unsigned)deg : 0u);
    const double2* ctab = P.tab_c + (size_t)tab_idx * kTab64Deg;
    auto coef = [&](int j) -> double2 {                              // (zero beyond a point's own degree)
      const double2 c = ctab[j < kTab64Deg ? j : kTab64Deg - 1];
      return double2{c.x * P.cs_phi, c.y * P.cs_psi};
    };
    // the wave's blocks of dv o tv into the exchange buffer (dv = D^2, or e for the mean weight): the value first, then the
    // store's predicate (4.2); the caller puts a barrier behind it
    auto publish = [&](const d4t (&dv)[TW], const d4t (&tv)[TW]) {
      d4t b[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i) b[i] = dv[i] * tv[i];
#pragma unroll
      for (int i = 0; i < TW; ++i)
        if (own[i]) {
#pragma unroll
          for (int q = 0; q < 4; ++q) bx[(4 * to[i] + q) * 64 + lane] = b[i][q];
        }
    };
    const unsigned olane = (unsigned)lr * kk8 + (unsigned)h * 8u;    // point lr, column h (+ 16 tj + 4 r) of a row of W
    const bool wr = colact && !decl;

#pragma clang loop unroll(disable)
    for (int c = 0; c < k; ++c) {
      // ---- Z = Yw e_c: column c of the record image, the wave's row blocks, in the result layout as it lies
      d4t va[TW], vb[TW], aphi[TW], apsi[TW], y[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) va[i][r] = Yw[(16 * to[i] + h + 4 * r) * KS + c];
      // ---- the recurrence on the 16 columns at once.  v_0 = Z, v_{j+1} = 2 (alpha G (D^2 o v_j) - v_j) - v_{j-1}; D enters as
      //      D^2 in the products' right-hand side and once at the end; slots that are not local to a column (D = 0) carry
      //      bounded junk that D^2 = 0 keeps out of every product.  The right-hand side crosses the waves through bx.
      auto product = [&](const d4t (&tv)[TW]) {
        publish(d2, tv);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TW; ++i) y[i] = d4t{0., 0., 0., 0.};
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double b = bx[(4 * tk + q) * 64 + lane];
#pragma unroll
            for (int i = 0; i < TW; ++i) y[i] = MIA_MFMA64(G[tk][i][q], b, y[i]);
          }
        __syncthreads();        // (one buffer: nobody writes the next right-hand side before every wave has read this one)
      };
      // vnew = 2 (alpha y - vcur) - vold, written over vold; the two weight functions accumulate c_j vnew
      auto advance = [&](d4t (&vold)[TW], const d4t (&vcur)[TW], const double2 cj) {
        product(vcur);
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          vold[i] = 2.0 * (alpha * y[i] - vcur[i]) - vold[i];
          aphi[i] = cj.x * vold[i] + aphi[i];
          apsi[i] = cj.y * vold[i] + apsi[i];
        }
      };
      {
        const double2 c0 = coef(0), c1 = coef(1);
        product(va);
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          vb[i] = alpha * y[i] - va[i];
          aphi[i] = c0.x * va[i] + c1.x * vb[i];
          apsi[i] = c0.y * va[i] + c1.y * vb[i];
        }
      }
      int j = 2;
      double2 cj = coef(2), cj1 = coef(3);
#pragma clang loop unroll(disable)
      for (; j + 1 <= degmax; j += 2) {
        const double2 nj = coef(j + 2), nj1 = coef(j + 3);       // requested one trip ahead
        advance(va, vb, cj);          // va = v_j
        advance(vb, va, cj1);         // vb = v_{j+1}
        cj = nj; cj1 = nj1;
      }
      if (j <= degmax) advance(va, vb, cj);
      // ---- wm_c = sum_b e_b psi_b: e o Psi of the sixteen points, each wave's own blocks through bx, under a block of ones,
      //      the WHOLE chain in every wave (canonical order, no partial sums).  Every row of the result block is the sum:
      //      register 0 of lane (lr, h) is that of point lr.
      publish(ed, apsi);
      __syncthreads();
      d4t zacc = {0., 0., 0., 0.};
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) zacc = MIA_MFMA64(1.0, bx[(4 * tk + q) * 64 + lane], zacc);
      const double wm = zacc[0];
      __syncthreads();
      // ---- row c of W_pert = Yw^T (D^2 o Phi): D o phi(S) z = D^2 o (accumulated v) is the right-hand side, complete in
      //      every wave; output member blocks tj = wv, wv + NW, ...
      publish(d2, aphi);
      __syncthreads();
      d4t bphi[UT];
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) bphi[tk][q] = bx[(4 * tk + q) * 64 + lane];
      // row c of the sixteen points' weights: wave-uniform 64-bit base (tile, row c) + 32-bit lane offset (point lr, column j)
      char* obase = reinterpret_cast<char*>(P.W + (p0 * k + c) * (int64_t)k);
#pragma clang loop unroll(disable)
      for (int tj = wv; tj < KT; tj += NW) {
        d4t acc = {0., 0., 0., 0.};
        const int mcol = 16 * tj + lr < k ? 16 * tj + lr : k - 1;      // the output column this lane supplies to the A operand
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = MIA_MFMA64(Yw[(16 * tk + 4 * q + h) * KS + mcol], bphi[tk][q], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + h + 4 * r;
          const double o = acc[r] + (wm + (mem == c ? P.f0 : 0.0));
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * 8u)) = o;
        }
      }
      __syncthreads();          // (the next member publishes into bx)
    }
    {
      if (!(colact && !decl)) pflag = 0;          // (columns that are not written do not report)
      const unsigned long long fb = __ballot(pflag != 0);
      // (the four lane groups of a column folded on the scalar side: a per-lane 64-bit mask would be carried, and at
      //  <6, 8, 2> spilled, from in front of the loop)
      const unsigned fcol = (unsigned)(fb | (fb >> 16) | (fb >> 32) | (fb >> 48)) & 0xffffu;
      const bool anyf = ((fcol >> lr) & 1u) != 0u;
      if (h == 0) xch[wv * 16 + lr] = anyf ? 1.0 : 0.0;
      __syncthreads();
      if (wv == 0 && h == 0 && colact && !decl) {
        bool bad = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) bad = bad || xch[w * 16 + lr] != 0.0;
        col_flag() = (bad ? MIA_FLAG_NONFINITE : 0) | (deg << 8);
      }
    }
    lo = hi;
    __syncthreads();
  }
}

// launches with the sizes of the wide frame (mia_frames64.h): UT blocks shared by NW wavefronts
template <int UT, int KT, int NW>
static int lienks_wide64_launch_t(const LienksWide64Params& tp, hipStream_t stream) {
  // p_max <= k bounds UT = ceil((p_max + 8) / 16) by KT + 1: the other pairs are never asked for and not built
  if constexpr (UT > KT + 1) return MIA_ERR_UNSUPPORTED;
  else
    return launch_blocks(lienks_wide64_kernel<UT, KT, NW>, (tp.ng + 15) >> 4, 64 * NW, wide64_lds_bytes(UT, KT, NW), stream,
                         [] { note_analysis_kernel("lienks_wide64_kernel<%d, %d, %d>", UT, KT, NW); }, tp);
}

bool lienks_wide64_route_covers(int k, int p_max, int64_t ng) {
  if (k < 2 || k > 128 || p_max < 0 || p_max > k || ng < 0) return false;
  // a pass addresses W as wave-uniform base (tile, row) + 32-bit byte offset inside the tile's sixteen matrices
  if ((int64_t)16 * k * k * 8 >= ((int64_t)1 << 31)) return false;
  const int ut = wide64_ut(p_max);
  if (wide64_lds_bytes(ut, (k + 15) >> 4, wide64_nw(ut)) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int lienks_wide64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec, const int32_t* nbr_cnt,
                         const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max, double epsilon, double* W_out,
                         int32_t* flags, int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !W_in || !W_out || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (w_stride != 0 && w_stride != (int64_t)k * k) return MIA_ERR_UNSUPPORTED;
  if (!lienks_wide64_route_covers(k, p_max, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Dual);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  LienksWide64Params tp;
  tp.k = k; tp.kp = (k + 1 + 3) & ~3;
  tp.ng = ng; tp.Win = W_in; tp.w_stride = w_stride; tp.rec = rec;
  tp.cnt = nbr_cnt; tp.idx = nbr_idx; tp.w = nbr_w; tp.p_cap = p_cap; tp.p_max = p_max;
  tp.transform = epsilon > 0.0 ? 0 : 1;
  tp.dscale = epsilon > 0.0 ? 1.0 / epsilon : 1.0;
  tp.dshift = epsilon > 0.0 ? epsilon : 1.0;
  // the constants of weights_wide64_launch at inf_factor = 1: reg = k - 1, f0 = 1
  const double rg = (double)(k - 1), km = (double)(k - 1);
  tp.reg = rg;
  tp.inv_reg = 1.0 / rg;
  tp.f0 = sqrt(km / rg);
  tp.cs_phi = sqrt(km) / (rg * sqrt(rg));
  tp.cs_psi = 1.0 / rg;
  tp.W = W_out; tp.flags = flags; tp.retry_count = retry_count;
  tp.dmax = kTab64Deg - 1;
  tp.tab_hdr = tab->hdr; tp.tab_c = tab->c;
  const int kt = (k + 15) >> 4;
  return dispatch_upto<8>(wide64_ut(p_max), [&](auto ut) {
    return dispatch_upto<8>(kt, [&](auto kt_c) { return lienks_wide64_launch_t<ut(), kt_c(), wide64_nw(ut())>(tp, stream); });
  });
}

}  // namespace mia
