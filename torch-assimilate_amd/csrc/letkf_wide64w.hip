// The LETKF WEIGHTS in FLOAT64 for ensembles of 65 .. 128 members (and below, for comparison), sixteen grid points per
// WORKGROUP of NW wavefronts, every contraction on the matrix cores (v_mfma_f64_16x16x4_f64): what LETKF.estimate_weights
// returns (interface/letkf.py:127-146, core/etkf.py:57-103), W[g][i][j] = w_mean_i + W_pert_ij, without an eigensolver.
//
// The frame is letkf_wide64.hip's, statement for statement up to and including the Gershgorin bound: per-point
// lists of any metric, union by rank extraction, ONE record image per workgroup with the compile-time pitch 16 KT + 5, the
// row blocks of the union dealt over the NW waves in runs of TW = ceil(UT / NW), G = Yw Yw^T for the wave's block columns,
// D^2, table row -> alpha, degree and decline of every point, the exchange buffer in the dead sqrt(rho) table.  (A copy, not a
// template switch: the analysis kernel's code object stays what it was.)  Lane roles, the canonical summation order -- every
// sum over the union is ONE ascending accumulator chain over (tk, q), so a point's bits depend on neither tile, shard nor NW
// -- and the instruction discipline (every product step unconditional, no branch between a matrix instruction and the first
// vector read of its result; builtins only) are described there.
//
// What differs is letkf_tile64w.hip's: instead of one pass per state row there is one pass per MEMBER c < k,
// with x' = e_c:
//
//     Z_c  = Yw e_c                   column c of the record image for the wave's own row blocks, already in the result
//                                     layout, va[i][r] = Yw[(16 to[i] + h + 4 r) KS + c] -- no product, no state, no mean
//     v'   = 2 (alpha G (D^2 o v) - v) - v''                the frame's recurrence, coefficients and degmax; two barriers a step
//     wm_c = sum_b d_b D^2_b psi_b    the mean weight of member c: the whole chain in every wave
//     W[g][c][j] = wm_c + f0 [c == j] + (Yw^T (D^2 o Phi))_j        row c of the point's weights, member blocks tj round robin
//
// (W_pert is symmetric: its column c, which the recurrence on Z_c produces, is its row c.)  W is [g1 - g0][k][k]: n k^2 8 bytes
// exceed 2^31 at 1e5 points, so a pass addresses it as a 64-bit wave-uniform base (tile, row c) + a 32-bit lane offset
// (16 k^2 8 <= 2^21).  For fixed (tj, r) the four lane groups h hold four consecutive j: one store instruction writes sixteen
// 32-byte segments, one per point.
//
// Declined points (degree above the table's cap): MIA_FLAG_RETRY, counted, W untouched, their columns run with alpha = 0;
// the Jacobi kernel redoes them with weights (mia_letkf_weights_retry_f64).  A tile that holds a non-finite record is done
// point by point, so that MIA_FLAG_NONFINITE stays with the points that use the record.  A point without observations gets
// sqrt(inf) I exactly (D = 0 keeps every product out; etkf.py:91-95).  Every barrier is reached by all waves on every path:
// the member loop's trip count is k, degmax is the same in every wave.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

struct Wide64WParams {
  int k; int kp;
  int64_t ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  double reg, inv_reg, f0, cs_phi, cs_psi;
  double* W; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// UT: 16-slot blocks of the union the workgroup holds; KT = ceil(k / 16); NW: wavefronts of the workgroup.  One workgroup's
// waves sit on different SIMDs, one wave per SIMD: up to 512 registers each.
template <int UT, int KT, int NW>
__global__ __launch_bounds__(64 * NW, 1) void letkf_wide64w_kernel(Wide64WParams P) {
  constexpr int UMAX = 16 * UT, NU = 4 * UT, DS = UMAX + 1, TW = (UT + NW - 1) / NW, NT = 64 * NW;
  // odd row pitch (in doubles) of the record image: the largest kp | 1 of this KT, so that every LDS address below is a
  // base register plus an immediate
  constexpr int KS = 16 * KT + 5;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: what depends on it is scalar selects and branches)
  const int k = P.k, kp = P.kp, pm = P.p_max;
  double* Yw = reinterpret_cast<double*>(smem_raw);          // [UMAX][KS] union records, zero rows beyond the union
  double* Dl = Yw + UMAX * KS;                               // [16][DS]   sqrt(rho) of (point, slot), 0 = not local
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
  unsigned long long badmask;
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
    badmask = __ballot(pbad);
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (sub + 4 * u >= lcnt) eidx[u] = -1;
  }

  const bool colok = lr < npts && !((badmask >> (4 * lr)) & 1ull);

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
      if (e >= 0) Dl[lp * DS + e] = ew[u2];
    }
    __syncthreads();
    const bool colact = colok && lr >= lo && lr < hi;
    d4t d2[TW];             // D^2 of column lr, slots 16 to[i] + h + 4 r
    // ---- G = Yw Yw^T, the wave's block columns: G[tk][i][r] = Gram[16 tk + h + 4 r][16 to[i] + lr]
    d4t G[UT][TW];
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
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
          for (int t1 = 0; t1 < UT; ++t1) G[t1][i] = MIA_MFMA64(av[t1], ao[i], G[t1][i]);
      }
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
        P.flags[p0 + lr] = MIA_FLAG_RETRY;
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
    // the wave's blocks of D^2 o tv into the exchange buffer: the value first, then the store's predicate (4.2); the caller
    // puts a barrier behind it
    auto publish = [&](const d4t (&tv)[TW]) {
      d4t b[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i) b[i] = d2[i] * tv[i];
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
        publish(tv);
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
      // ---- wm_c = sum_b d_b (w_b psi_b): row vector of the innovations (column k of the records) times D^2 o Psi, the
      //      WHOLE chain in every wave (canonical order, no partial sums).  Row 0 of the result block = lanes (lr, h = 0),
      //      register 0; handed to the column's other lanes.
      publish(apsi);
      __syncthreads();
      d4t zacc = {0., 0., 0., 0.};
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dv = Yw[(16 * tk + 4 * q + h) * KS + k];
          zacc = MIA_MFMA64(lr == 0 ? dv : 0.0, bx[(4 * tk + q) * 64 + lane], zacc);
        }
      const double wm = __shfl(zacc[0], lr, 64);
      __syncthreads();
      // ---- row c of W_pert = Yw^T (D^2 o Phi): D o phi(S) z = D^2 o (accumulated v) is the right-hand side, complete in
      //      every wave; output member blocks tj = wv, wv + NW, ...
      publish(aphi);
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
      const bool anyf = ((fb >> lr) & 0x0001000100010001ull) != 0ull;
      if (h == 0) xch[wv * 16 + lr] = anyf ? 1.0 : 0.0;
      __syncthreads();
      if (wv == 0 && h == 0 && colact && !decl) {
        bool bad = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) bad = bad || xch[w * 16 + lr] != 0.0;
        P.flags[p0 + lr] = (bad ? MIA_FLAG_NONFINITE : 0) | (deg << 8);
      }
    }
    lo = hi;
    __syncthreads();
  }
}

// launches with the sizes of the wide frame (mia_frames64.h): UT blocks shared by NW wavefronts
template <int UT, int KT, int NW>
static int wide64w_launch_t(const Wide64WParams& tp, hipStream_t stream) {
  // p_max <= k bounds UT = ceil((p_max + 8) / 16) by KT + 1: the other pairs are never asked for and not built
  if constexpr (UT > KT + 1) return MIA_ERR_UNSUPPORTED;
  else
    return launch_blocks(letkf_wide64w_kernel<UT, KT, NW>, (tp.ng + 15) >> 4, 64 * NW, wide64_lds_bytes(UT, KT, NW), stream,
                         [] { note_analysis_kernel("letkf_wide64w_kernel<%d, %d, %d>", UT, KT, NW); }, tp);
}

bool weights_wide64_route_covers(int k, int p_max, int64_t ng) {
  if (k < 2 || k > 128 || p_max < 0 || p_max > k || ng < 0) return false;
  // a pass addresses W as wave-uniform base (tile, row) + 32-bit byte offset inside the tile's sixteen matrices
  if ((int64_t)16 * k * k * 8 >= ((int64_t)1 << 31)) return false;
  const int ut = wide64_ut(p_max);
  if (wide64_lds_bytes(ut, (k + 15) >> 4, wide64_nw(ut)) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int weights_wide64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                          const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                          int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !W || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!weights_wide64_route_covers(k, p_max, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Dual);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Wide64WParams tp;
  tp.k = k; tp.kp = (k + 1 + 3) & ~3;
  tp.ng = ng; tp.rec = rec;
  tp.cnt = nbr_cnt; tp.idx = nbr_idx; tp.w = nbr_w; tp.p_cap = p_cap; tp.p_max = p_max;
  const double rg = (double)(k - 1) / inf_factor, km = (double)(k - 1);
  tp.reg = rg;
  tp.inv_reg = 1.0 / rg;
  tp.f0 = sqrt(km / rg);
  tp.cs_phi = sqrt(km) / (rg * sqrt(rg));
  tp.cs_psi = 1.0 / rg;
  tp.W = W; tp.flags = flags; tp.retry_count = retry_count;
  tp.dmax = kTab64Deg - 1;
  tp.tab_hdr = tab->hdr; tp.tab_c = tab->c;
  const int kt = (k + 15) >> 4;
  return dispatch_upto<8>(wide64_ut(p_max), [&](auto ut) {
    return dispatch_upto<8>(kt, [&](auto kt_c) { return wide64w_launch_t<ut(), kt_c(), wide64_nw(ut())>(tp, stream); });
  });
}

}  // namespace mia
