// Fused LETKF analysis in FLOAT64, sixteen grid points per wavefront, every contraction on the matrix cores
// (v_mfma_f64_16x16x4_f64).  The default working precision of the drop-in classes (interface.py, after
// pytassim/interface/base.py:68,73,106-118) arrives here instead of at the one-point-per-wavefront Jacobi kernel.
//
// Mathematics of letkf_tile.hip (reference: core/etkf.py:57-103 + interface/wrapper.py:86-98 +
// base.py:257-278): in the index space of the UNION of a tile's sixteen per-point lists
//
//     S_g = D_g G D_g,      G = Yw Yw^T  (U x U),   D_g = diag(sqrt(rho_g)) (0 = not local)
//     Z   = Yw X'                     (U x k)(k x 16)
//     R   = |G| D                     Gershgorin bounds -> table row -> degree and interval of every point
//     v'  = 2 (alpha G (D^2 o v) - v) - v''                the three-term Chebyshev recurrence, 16 points at a time
//     Xa' = Yw^T (D^2 o Phi)          (k x U)(U x 16)
//
// all in float64: no split operands, no per-record scale.  Input is what mia_letkf_analysis_packed_f64 takes -- float64
// records [P][kp] and the per-point lists with their float64 sqrt(rho) -- so the route does not depend on the metric that
// made the lists; union, ranks and slots are formed here.
//
// Lane roles follow v_mfma_f64_16x16x4_f64: A and B carry ONE f64 per lane, lane (lr, h) = (lane & 15, lane >> 4) supplies
// A[i = lr][k = h] and B[k = h][j = lr]; of a 16 x 16 result block the lane holds COLUMN lr (= grid point lr of the tile),
// rows h + 4 r in register r = 0..3 (not the f32 form's 4 h + r).  Step (t, q) of a product over the union therefore sums
// slots 16 t + 4 q + h, h = 0..3: register q of result block t IS the B operand of that step where it sits, so the vectors
// of the recurrence never leave the registers; by symmetry the Gram blocks are the A operands of those steps as they
// stand.  Members are enumerated the same way (member 16 tm + 4 q + h), which puts x' where the output block needs it.
//
// Summation order is canonical: slot = RANK of the observation index inside the union, steps ascend, so a point's own
// observations are always summed in ascending index order with exact zeros in between, whatever else is in the tile: a
// point's result does not depend on tile composition, shard boundaries or launch geometry.
//
// Every step of every product is unconditional (all 4 UT steps, slots beyond the union hold zero records and D = 0): there
// is NO branch between a matrix instruction and the first vector read of its result, and builtins only.
//
// A tile whose union exceeds the 16 UT slots of its instantiation is processed in halves (quarters, ...): one point
// always fits (p_max <= 16 UT is checked on the host).  A tile that holds a non-finite record is analysed point by point,
// so that the damage stays with the points that use the observation.  Points whose degree exceeds the table's cap are
// DECLINED (MIA_FLAG_RETRY, counted, Xa untouched) and redone by letkf_wave_kernel<double>.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

// the coefficient table (dual pair), the lane helpers and MIA_MFMA64: mia_cheb_table64.h, shared with letkf_dense64.hip

struct Tile64Params {
  const double* X; int64_t ldx; int m; int k; int kp;
  int64_t g0, ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  double reg, inv_reg, f0, inv_k, cs_phi, cs_psi;
  double* Xa; int64_t ldo, o0; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};


// UT: 16-slot blocks of the union the wavefront holds (G is UT x UT result blocks of 8 registers); KT = ceil(k / 16).
// UT <= 2: two wavefronts per SIMD (256 registers each); above: one, up to 512.
template <int UT, int KT>
__global__ __launch_bounds__(64, (UT <= 2 ? 2 : 1)) void letkf_tile64_kernel(Tile64Params P) {
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
  const int64_t oc0 = P.o0 + p0;                             // output column of the tile's first point
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;

  // ---- the tile's neighbour lists: lane (lp, sub) holds entries sub, sub + 4, ... of point lp (unconditional loads inside
  //      the row's storage; entries beyond the count become index -1: the one validity test of everything that follows)
  const int nl = pm < P.p_cap ? pm : P.p_cap;
  int eidx[NU];
  double ew[NU];
  int lcnt;
  unsigned long long badmask;
  {
    const int64_t row = p0 + (lp < npts ? lp : 0);          // (lists, flags and output columns count from the shard's g0)
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
      for (int it = sub; it < P.m * k; it += 4) P.Xa[(int64_t)it * P.ldo + oc0 + lp] = nanv;
    }
    if (lp >= npts || pbad) lcnt = 0;
    badmask = __ballot(pbad);
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (sub + 4 * u >= lcnt) eidx[u] = -1;
  }

  // a state row of the tile: member (tm, q) of lane group h = 16 tm + 4 q + h, column lr (clamped to an existing member)
  // (wave-uniform base + 32-bit lane offset in bytes: k ld 8 < 2^31 is checked on the host)
  const unsigned ldxb = (unsigned)P.ldx * 8u, ldob = (unsigned)P.ldo * 8u;
  auto load_x = [&](int mi, int hh, int col, double (&xr)[KT][4]) {
    const char* xbase = reinterpret_cast<const char*>(P.X + (int64_t)mi * k * P.ldx + P.g0 + p0);
    const unsigned xlane = (unsigned)hh * ldxb + (unsigned)col * 8u;
#pragma unroll
    for (int tm = 0; tm < KT; ++tm)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned off = xlane + (unsigned)(16 * tm + 4 * q) * ldxb;
        if (tm == KT - 1) {                               // (only the last member block is ragged)
          const int mem = 16 * tm + 4 * q + hh;
          off = (unsigned)(mem < k ? mem : k - 1) * ldxb + (unsigned)col * 8u;
        }
        xr[tm][q] = *reinterpret_cast<const double*>(xbase + off);
      }
  };

  int lo = 0;
#pragma clang loop unroll(disable)
  while (lo < npts) {
    // The loop body runs once per tile unless the tile had to be split.  The lane id goes through an opaque copy, so that
    // the compiler does not hoist dozens of address / predicate registers out of a loop that does not loop.
    int lanev = lane;
    asm volatile("" : "+v"(lanev));
    const int lr = lanev & 15, h = lanev >> 4, lp = lanev >> 2;
    const bool colok = lr < npts && !((badmask >> (4 * lr)) & 1ull);
    const int lrc = lr < npts ? lr : npts - 1;               // a column that exists (clamped, unconditional loads)
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
      // points that do not see that observation.  Such a tile is analysed point by point: the union is then the point's
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

    for (int mi = 0; mi < P.m; ++mi) {
      // (lane roles through opaque copies once more: what is invariant in this loop -- addresses, predicates -- would
      //  otherwise be hoisted in front of it and spilled there)
      int hv = h, lrv = lr, lrcv = lrc;
      asm volatile("" : "+v"(hv), "+v"(lrv), "+v"(lrcv));
      double xb[KT][4];
      load_x(mi, hv, lrcv, xb);
      double xs = 0.0;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + hv < k);
          xb[tm][q] = live ? xb[tm][q] : 0.0;
          xs += xb[tm][q];
        }
      const double xm = tile64_add_h(xs) * P.inv_k;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + hv < k);
          xb[tm][q] = live ? xb[tm][q] - xm : 0.0;
        }
      // ---- Z = Yw X'
      d4t va[UT], vb[UT], aphi[UT], apsi[UT], y[UT];
#pragma unroll
      for (int t = 0; t < UT; ++t) va[t] = d4t{0., 0., 0., 0.};
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int mem = 16 * tm + 4 * q + hv;
          const bool ok = tm < KT - 1 || mem < k;
          const int col = ok ? mem : 0;
#pragma unroll
          for (int t = 0; t < UT; ++t) {
            const double v = Yw[(16 * t + lrv) * KS + col];
            va[t] = MIA_MFMA64(ok ? v : 0.0, xb[tm][q], va[t]);
          }
        }
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
      // ---- x' w_mean = sum_b d_b (w_b psi_b): one more product, row vector of the innovations (column k of the records)
      //      times D^2 o Psi -- on the matrix cores like everything else, because their enumeration IS the canonical
      //      summation order.  Row 0 of the result block = lanes (lrv, hv = 0), register 0; handed to the column's other lanes.
      double xre[KT][4];
      load_x(mi, hv, lrcv, xre);
      d4t zacc = {0., 0., 0., 0.};
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dv = Yw[(16 * tk + 4 * q + hv) * KS + k];
          zacc = MIA_MFMA64(lrv == 0 ? dv : 0.0, d2[tk][q] * apsi[tk][q], zacc);
        }
      const double zu = __shfl(zacc[0], lrv, 64);
#pragma unroll
      for (int t = 0; t < UT; ++t) aphi[t] *= d2[t];          // D o phi(S) z = D^2 o (accumulated v): right-hand side of the last product
      const double mterm = xm + zu;
      char* obase = reinterpret_cast<char*>(P.Xa + (int64_t)mi * k * P.ldo + oc0);
      const unsigned olane = (unsigned)hv * ldob + (unsigned)lrv * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj) {
        d4t acc = {0., 0., 0., 0.};
        const int mcol = 16 * tj + lrv < k ? 16 * tj + lrv : k - 1;      // the output row this lane supplies to the A operand
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = MIA_MFMA64(Yw[(16 * tk + 4 * q + hv) * KS + mcol], aphi[tk][q], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + hv + 4 * r;
          const double o = acc[r] + (mterm + P.f0 * (xre[tj][r] - xm));
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * ldob)) = o;
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
static int tile64_launch_t(const Tile64Params& tp, hipStream_t stream) {
  return launch_blocks(letkf_tile64_kernel<UT, KT>, (tp.ng + 15) >> 4, 64, resident64_lds_bytes(UT, tp.kp), stream,
                       [] { note_analysis_kernel("letkf_tile64_kernel<%d, %d>", UT, KT); }, tp);
}

bool tile64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng) {
  if (m < 1 || k < 2 || k > 64 || p_max < 0 || p_max > k || ldx < 1 || ldo < 1 || ng < 0) return false;
  // the state and the output are addressed as wave-uniform base + 32-bit byte offset of a column of one state row block
  if ((int64_t)k * ldx * 8 >= ((int64_t)1 << 31) || (int64_t)k * ldo * 8 >= ((int64_t)1 << 31)) return false;
  if (resident64_lds_bytes(resident64_ut(p_max), (k + 1 + 3) & ~3) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int tile64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                           hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!tile64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Dual);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Tile64Params tp;
  tp.X = X; tp.ldx = ldx; tp.m = m; tp.k = k; tp.kp = (k + 1 + 3) & ~3;
  tp.g0 = g0; tp.ng = ng; tp.rec = rec;
  tp.cnt = nbr_cnt; tp.idx = nbr_idx; tp.w = nbr_w; tp.p_cap = p_cap; tp.p_max = p_max;
  const double rg = (double)(k - 1) / inf_factor, km = (double)(k - 1);
  tp.reg = rg;
  tp.inv_reg = 1.0 / rg;
  tp.f0 = sqrt(km / rg);
  tp.inv_k = 1.0 / (double)k;
  tp.cs_phi = sqrt(km) / (rg * sqrt(rg));
  tp.cs_psi = 1.0 / rg;
  tp.Xa = Xa; tp.ldo = ldo; tp.o0 = o0; tp.flags = flags; tp.retry_count = retry_count;
  tp.dmax = kTab64Deg - 1;
  tp.tab_hdr = tab->hdr; tp.tab_c = tab->c;
  const int kt = (k + 15) >> 4;
  return dispatch_upto<4>(resident64_ut(p_max), [&](auto ut) {
    return dispatch_upto<4>(kt, [&](auto kt_c) { return tile64_launch_t<ut(), kt_c()>(tp, stream); });
  });
}

}  // namespace mia
