// The LETKF WEIGHTS in FLOAT64, sixteen grid points per wavefront, every contraction on the matrix cores
// (v_mfma_f64_16x16x4_f64): what LETKF.estimate_weights returns (interface/letkf.py:127-146, core/etkf.py:57-103) in the
// default working precision of the drop-in classes, W[g][i][j] = w_mean_i + W_pert_ij, without an eigensolver.
//
// The frame is letkf_tile64.hip's, statement for statement up to and including the Gershgorin bound: per-point lists of any
// metric, union by rank extraction, record image in LDS, G = Yw Yw^T, D^2, table row -> alpha, degree and decline of every
// point.  (A copy, not a template switch: the analysis kernels' code objects stay what they were.)  Lane roles, canonical
// summation order and the instruction discipline (every product step unconditional, no branch between a matrix instruction
// and the first vector read of its result; builtins only) are described there.
//
// What differs: instead of one pass per state row there is one pass per MEMBER c < k, with x' = e_c:
//
//     Z_c  = Yw e_c                   column c of the record image, the same for the sixteen points: already in the result
//                                     layout, va[t][r] = Yw[(16 t + h + 4 r) KS + c] -- no product, no state, no mean
//     v'   = 2 (alpha G (D^2 o v) - v) - v''                the recurrence as it stands, same coefficients and degrees
//     wm_c = sum_b d_b D^2_b psi_b    the mean weight of member c (the analysis kernel's x' w_mean with x' = e_c)
//     W[g][c][j] = wm_c + f0 [c == j] + (Yw^T (D^2 o Phi))_j        row c of the point's weights
//
// (W_pert is symmetric: its column c, which the recurrence on Z_c produces, is its row c.)  W is [g1 - g0][k][k]: n k^2 8 bytes
// exceed 2^31 at 1e5 points, so a pass addresses it as a 64-bit wave-uniform base (tile, row c) + a 32-bit lane offset
// (16 k^2 8 <= 2^19).  For fixed (tj, r) the four lane groups h hold four consecutive j: one store instruction writes sixteen
// 32-byte segments, one per point.  Not staged through LDS in this version.
//
// Declined points (degree above the table's cap): MIA_FLAG_RETRY, counted, W untouched; the Jacobi kernel redoes them with
// weights (mia_letkf_weights_retry_f64).  A tile that holds a non-finite record is done point by point, so that
// MIA_FLAG_NONFINITE stays with the points that use the record.  A point without observations gets sqrt(inf) I exactly
// (D = 0 keeps every product out; etkf.py:91-95).
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

struct Tile64WParams {
  int k; int kp;
  int64_t ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  double reg, inv_reg, f0, cs_phi, cs_psi;
  double* W; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};


// UT: 16-slot blocks of the union the wavefront holds (G is UT x UT result blocks of 8 registers); KT = ceil(k / 16).
// Instantiations and launch bounds are letkf_tile64_kernel's.
template <int UT, int KT>
__global__ __launch_bounds__(64, (UT <= 2 ? 2 : 1)) void letkf_weights64_kernel(Tile64WParams P) {
  constexpr int UMAX = 16 * UT, NU = 4 * UT, DS = UMAX + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int k = P.k, kp = P.kp, pm = P.p_max;
  const int KS = kp | 1;                                     // odd row pitch (in doubles) of the record image
  double* Yw = reinterpret_cast<double*>(smem_raw);          // [UMAX][KS] union records, zero rows beyond the union
  double* Dl = Yw + UMAX * KS;                               // [16][DS]   sqrt(rho) of (point, slot), 0 = not local
  int* ukey = reinterpret_cast<int*>(Dl + 16 * DS);          // [UMAX]     observation index of a slot, -1 = unused

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

  // ---- the tile's neighbour lists: lane (lp, sub) holds entries sub, sub + 4, ... of point lp (unconditional loads inside
  //      the row's storage; entries beyond the count become index -1: the one validity test of everything that follows)
  const int nl = pm < P.p_cap ? pm : P.p_cap;
  int eidx[NU];
  double ew[NU];
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
      const int e = pos < nl ? pos : 0;
      eidx[u] = ib[e];
      ew[u] = wb[e];
    }
    const bool pbad = lp < npts && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad) {
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

  int lo = 0;
#pragma clang loop unroll(disable)
  while (lo < npts) {
    // The loop body runs once per tile unless the tile had to be split.  The lane id goes through an opaque copy, so that
    // the compiler does not hoist dozens of address / predicate registers out of a loop that does not loop.
    int lanev = lane;
    asm volatile("" : "+v"(lanev));
    const int lr = lanev & 15, h = lanev >> 4, lp = lanev >> 2;
    const bool colok = lr < npts && !((badmask >> (4 * lr)) & 1ull);
    // ---- union of the lists of points [lo, hi): slot = RANK of the observation index, found by repeated extraction of
    //      the smallest remaining key (one DPP reduction per slot); shrink the range until the union fits
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
      for (int i = lane; i < UMAX; i += 64) ukey[i] = -1;
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
          if (lane == 0) ukey[U] = (int)(last - 1u);
        }
        ++U;
        if (U > UMAX) break;
      }
      if (U > UMAX) { __syncthreads(); n >>= 1; continue; }     // (n = 1 always fits: a single list has at most UMAX entries)
      __syncthreads();
      // ---- the union's records, four rows per trip: lane group h takes row r0 + h, its sixteen lanes the columns
      double fin = 0.0;       // stays 0 while every value is finite (inf * 0 = NaN)
#pragma clang loop unroll_count(2)
      for (int r0 = 0; r0 < UMAX; r0 += 4) {
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
      // A non-finite record would reach EVERY column of the tile through the shared Gram matrix (NaN * 0 = NaN), also the
      // points that do not see that observation.  Such a tile is done point by point: the union is then the point's
      // own list and the damage stays where the reference has it.
      if (__any(fin != fin) && hi - lo > 1) { __syncthreads(); n = 1; continue; }
      break;
    }
    for (int i = lane; i < 16 * DS; i += 64) Dl[i] = 0.0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (es[u] >= 0) Dl[lp * DS + es[u]] = ew[u];
    __syncthreads();
    const bool colact = colok && lr >= lo && lr < hi;
    d4t d2[UT];             // D^2 of column lr, slots 16 t + h + 4 r
    // ---- G = Yw Yw^T: G[t1][t2][r] = Gram[16 t1 + h + 4 r][16 t2 + lr]
    d4t G[UT][UT];
#pragma unroll
    for (int t1 = 0; t1 < UT; ++t1)
#pragma unroll
      for (int t2 = 0; t2 < UT; ++t2) G[t1][t2] = d4t{0., 0., 0., 0.};
#pragma unroll
    for (int tm = 0; tm < KT; ++tm)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mem = 16 * tm + 4 * q + h;
        const bool ok = tm < KT - 1 || mem < k;            // (innovation / pad columns are not members; only the last block is ragged)
        const int col = ok ? mem : 0;
        double av[UT];
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          const double v = Yw[(16 * t + lr) * KS + col];
          av[t] = ok ? v : 0.0;
        }
#pragma unroll
        for (int t2 = 0; t2 < UT; ++t2)
#pragma unroll
          for (int t1 = 0; t1 < UT; ++t1) G[t1][t2] = MIA_MFMA64(av[t1], av[t2], G[t1][t2]);
      }
    // ---- Gershgorin bound of every point: L_g = max_a w_a sum_b |G_ab| w_b, then degree / interval from the table
    double alpha;
    int deg, tab_idx, pflag = 0;
    bool decl;
    {
      d4t dreg[UT], R[UT];
#pragma unroll
      for (int t = 0; t < UT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dreg[t][r] = Dl[lr * DS + 16 * t + h + 4 * r];
        R[t] = d4t{0., 0., 0., 0.};
      }
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < UT; ++t) R[t] = MIA_MFMA64(fabs(G[tk][t][q]), dreg[tk][q], R[t]);
      double L = 0.0;
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = dreg[t][r] * R[t][r];
          L = (v > L || v != v) ? v : L;
          d2[t][r] = dreg[t][r] * dreg[t][r];
        }
      L = tile64_max_h(L);
      L = fmax(L, 1e-300 * P.reg) * (1.0 + 1e-12);
      if (!(L == L) || !(fabs(L) < 1e300)) { pflag |= MIA_FLAG_NONFINITE; L = P.reg; }
      tab_idx = (int)ceil(double(kTabPerOctave) * log2(L * P.inv_reg)) + kTabIdx0;
      tab_idx = tab_idx < 0 ? 0 : (tab_idx > kTabN - 1 ? kTabN - 1 : tab_idx);      // (the last entries decline: T = 2^8)
      const Tab64Hdr hd = P.tab_hdr[tab_idx];
      deg = hd.deg;
      decl = colact && (deg > P.dmax || deg > kTab64Deg - 1);
      alpha = (deg > kTab64Deg - 1) ? 0.0 : hd.two_over_T * P.inv_reg;             // (a declined column carries bounded junk)
      if (decl && h == 0) {
        P.flags[p0 + lr] = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
    }
    const int degmax = (int)tile64_wave_max_u32((colact && !decl) ? (unsigned)deg : 0u);
    const double2* ctab = P.tab_c + (size_t)tab_idx * kTab64Deg;
    auto coef = [&](int j) -> double2 {                              // (zero beyond a point's own degree)
      const double2 c = ctab[j < kTab64Deg ? j : kTab64Deg - 1];
      return double2{c.x * P.cs_phi, c.y * P.cs_psi};
    };

    for (int c = 0; c < k; ++c) {
      // (lane roles through opaque copies once more: what is invariant in this loop -- addresses, predicates -- would
      //  otherwise be hoisted in front of it and spilled there)
      int hv = h, lrv = lr;
      asm volatile("" : "+v"(hv), "+v"(lrv));
      // ---- Z = Yw e_c: column c of the record image, in the result layout as it lies
      d4t va[UT], vb[UT], aphi[UT], apsi[UT], y[UT];
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) va[t][r] = Yw[(16 * t + hv + 4 * r) * KS + c];
      // ---- the recurrence on the 16 columns at once; vectors stay in the result layout.  v_0 = Z,
      //      v_{j+1} = 2 (alpha G (D^2 o v_j) - v_j) - v_{j-1}; D enters as D^2 in the products' right-hand side and once at
      //      the end; slots that are not local to a column (D = 0) carry bounded junk that D^2 = 0 keeps out of every product
      auto product = [&](const d4t (&tv)[UT]) {
#pragma unroll
        for (int t = 0; t < UT; ++t) y[t] = d4t{0., 0., 0., 0.};
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double b = d2[tk][q] * tv[tk][q];
#pragma unroll
            for (int t = 0; t < UT; ++t) y[t] = MIA_MFMA64(G[tk][t][q], b, y[t]);
          }
      };
      // vnew = 2 (alpha y - vcur) - vold, written over vold; the two weight functions accumulate c_j vnew
      auto advance = [&](d4t (&vold)[UT], const d4t (&vcur)[UT], const double2 cj) {
        product(vcur);
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          vold[t] = 2.0 * (alpha * y[t] - vcur[t]) - vold[t];
          aphi[t] = cj.x * vold[t] + aphi[t];
          apsi[t] = cj.y * vold[t] + apsi[t];
        }
      };
      {
        const double2 c0 = coef(0), c1 = coef(1);
        product(va);
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          vb[t] = alpha * y[t] - va[t];
          aphi[t] = c0.x * va[t] + c1.x * vb[t];
          apsi[t] = c0.y * va[t] + c1.y * vb[t];
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
      // ---- wm_c = sum_b d_b (w_b psi_b): one more product, row vector of the innovations (column k of the records)
      //      times D^2 o Psi -- on the matrix cores like everything else, because their enumeration IS the canonical
      //      summation order.  Row 0 of the result block = lanes (lrv, hv = 0), register 0; handed to the column's other lanes.
      d4t zacc = {0., 0., 0., 0.};
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dv = Yw[(16 * tk + 4 * q + hv) * KS + k];
          zacc = MIA_MFMA64(lrv == 0 ? dv : 0.0, d2[tk][q] * apsi[tk][q], zacc);
        }
      const double wm = __shfl(zacc[0], lrv, 64);
#pragma unroll
      for (int t = 0; t < UT; ++t) aphi[t] *= d2[t];          // D o phi(S) z = D^2 o (accumulated v): right-hand side of the last product
      // row c of the sixteen points' weights: wave-uniform 64-bit base (tile, row c) + 32-bit lane offset (point lrv, column j)
      char* obase = reinterpret_cast<char*>(P.W + (p0 * k + c) * (int64_t)k);
      const unsigned olane = (unsigned)lrv * kk8 + (unsigned)hv * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj) {
        d4t acc = {0., 0., 0., 0.};
        const int mcol = 16 * tj + lrv < k ? 16 * tj + lrv : k - 1;      // the output column this lane supplies to the A operand
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = MIA_MFMA64(Yw[(16 * tk + 4 * q + hv) * KS + mcol], aphi[tk][q], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + hv + 4 * r;
          const double o = acc[r] + (wm + (mem == c ? P.f0 : 0.0));
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * 8u)) = o;
        }
      }
    }
    {
      if (!(colact && !decl)) pflag = 0;          // (columns that are not written do not report)
      const unsigned long long fb = __ballot(pflag != 0);
      const bool anyf = ((fb >> lr) & 0x0001000100010001ull) != 0ull;
      if (h == 0 && colact && !decl) P.flags[p0 + lr] = (anyf ? MIA_FLAG_NONFINITE : 0) | (deg << 8);
    }
    lo = hi;
    __syncthreads();
  }
}

// launches with the sizes of the resident image (mia_frames64.h): UT blocks of records of kp doubles
template <int UT, int KT>
static int tile64w_launch_t(const Tile64WParams& tp, hipStream_t stream) {
  return launch_blocks(letkf_weights64_kernel<UT, KT>, (tp.ng + 15) >> 4, 64, resident64_lds_bytes(UT, tp.kp), stream,
                       [] { note_analysis_kernel("letkf_weights64_kernel<%d, %d>", UT, KT); }, tp);
}

bool weights64_route_covers(int k, int p_max, int64_t ng) {
  if (k < 2 || k > 64 || p_max < 0 || p_max > k || ng < 0) return false;
  if (resident64_lds_bytes(resident64_ut(p_max), (k + 1 + 3) & ~3) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int weights64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                     const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                     int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !W || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!weights64_route_covers(k, p_max, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Dual);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Tile64WParams tp;
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
  return dispatch_upto<4>(resident64_ut(p_max), [&](auto ut) {
    return dispatch_upto<4>(kt, [&](auto kt_c) { return tile64w_launch_t<ut(), kt_c()>(tp, stream); });
  });
}

}  // namespace mia
