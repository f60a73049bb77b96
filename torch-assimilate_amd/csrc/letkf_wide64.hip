// Fused LETKF analysis in FLOAT64 for ensembles of 65 .. 128 members (and below, for comparison), sixteen grid points per
// WORKGROUP of NW wavefronts, every contraction on the matrix cores (v_mfma_f64_16x16x4_f64).
//
// The mathematics, the input, the prologue and the lane roles are letkf_tile64.hip's: in the index space of the
// UNION of a tile's sixteen per-point lists
//
//     S_g = D_g G D_g,      G = Yw Yw^T  (U x U),   D_g = diag(sqrt(rho_g)) (0 = not local)
//     Z   = Yw X'                     (U x k)(k x 16)
//     R   = |G| D                     Gershgorin bounds -> table row -> degree and interval of every point
//     v'  = 2 (alpha G (D^2 o v) - v) - v''                the three-term Chebyshev recurrence, 16 points at a time
//     Xa' = Yw^T (D^2 o Phi)          (k x U)(U x 16)
//
// What is new is the distribution (after letkf_tile2p.hip): one wavefront holds 8 UT^2 registers of Gram matrix,
// which ends at UT = 4.  Here the UT sixteen-slot ROW BLOCKS of the union are split over the NW waves of a workgroup, which
// share one record image in LDS.  Wave w owns the contiguous blocks t = w TW .. w TW + TW - 1 (TW = ceil(UT / NW); the last
// wave may own fewer) and keeps for them G[tk][t] (all tk) and the vectors va / vb / aphi / apsi / y / d2.  Per recurrence
// step a wave forms b = D^2 o v for its own blocks, lays them into LDS in the B-operand layout (which IS the result layout:
// lane for lane the same value), and after a workgroup barrier reads the complete right-hand side and runs
// y[t] = sum_tk sum_q MFMA(G[tk][t][q], b[tk][q], y[t]) for its own t.  One exchange buffer, two barriers per step; it lies
// in the space of the sqrt(rho) table, which is dead once d2 sits in registers.  Otherwise only the Gershgorin maximum (a
// max: exact in any order), D^2 o Psi (for x' w_mean) and D^2 o Phi (for the output product) cross the waves; the output
// member blocks tj are dealt round robin.
//
// Summation order is canonical: slot = RANK of the observation index inside the union, and EVERY sum over the union is one
// chain of matrix instructions through one accumulator, ascending over (tk, q) -- never per-wave partial sums (x' w_mean
// included: every wave runs that whole chain).  A point's bits therefore do not depend on its tile, the shard boundary, or NW.
//
// Every step of every product is unconditional; a wave that owns fewer than TW blocks computes its missing blocks as copies of
// block UT - 1 and does not publish them.  There is NO branch between a matrix instruction and the first vector read of its
// result: published values are formed before the (wave-uniform) predicate of their store.  Builtins only.
//
// The wave index is a scalar (readfirstlane); degmax derives from per-column values every wave holds identically, and every
// barrier is reached by all waves: the union loop, the halves path, the point-by-point path of a tile with a non-finite record
// and the recurrence of a tile whose columns are all declined run the same trips in every wave.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

struct Wide64Params {
  const double* X; int64_t ldx; int m; int k; int kp;
  int64_t g0, ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  double reg, inv_reg, f0, inv_k, cs_phi, cs_psi;
  double* Xa; int64_t ldo, o0; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// UT: 16-slot blocks of the union the workgroup holds; KT = ceil(k / 16); NW: wavefronts of the workgroup.  One workgroup's
// waves sit on different SIMDs, one wave per SIMD: up to 512 registers each.
template <int UT, int KT, int NW>
__global__ __launch_bounds__(64 * NW, 1) void letkf_wide64_kernel(Wide64Params P) {
  constexpr int UMAX = 16 * UT, NU = 4 * UT, DS = UMAX + 1, TW = (UT + NW - 1) / NW, NT = 64 * NW;
  // odd row pitch (in doubles) of the record image: the largest kp | 1 of this KT, so that every LDS address below is a
  // base register plus an immediate (kp | 1 itself wherever k >= 16 KT - 3, e.g. k = 80, 96, 128)
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
  const int64_t oc0 = P.o0 + p0;                             // output column of the tile's first point
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;

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
    const int64_t row = p0 + (lp < npts ? lp : 0);          // (lists, flags and output columns count from the shard's g0)
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
      for (int it = sub; it < P.m * k; it += 4) P.Xa[(int64_t)it * P.ldo + oc0 + lp] = nanv;
    }
    if (lp >= npts || pbad) lcnt = 0;
    badmask = __ballot(pbad);
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (sub + 4 * u >= lcnt) eidx[u] = -1;
  }

  const unsigned ldxb = (unsigned)P.ldx * 8u, ldob = (unsigned)P.ldo * 8u;   // (k ld 8 < 2^31 is checked on the host)
  const bool colok = lr < npts && !((badmask >> (4 * lr)) & 1ull);
  const int lrc = lr < npts ? lr : npts - 1;                 // a column that exists (clamped, unconditional loads)

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
      // points that do not see that observation.  Such a tile is analysed point by point: the union is then the point's
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

    for (int mi = 0; mi < P.m; ++mi) {
      // ---- the state row: member (tm, q) of lane group h = 16 tm + 4 q + h, column lr (clamped to an existing member)
      const char* xbase = reinterpret_cast<const char*>(P.X + (int64_t)mi * k * P.ldx + P.g0 + p0);
      const unsigned xlane = (unsigned)h * ldxb + (unsigned)lrc * 8u;
      double xb[KT][4];
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (wave-uniform 64-bit row address + ONE 32-bit lane offset: the rows' addresses are scalars, not 4 KT vector registers)
          const char* xrow = xbase + (size_t)(16 * tm + 4 * q) * ldxb;
          unsigned off = xlane;
          if (tm == KT - 1) {                               // (only the last member block is ragged)
            const int mem = 16 * tm + 4 * q + h;
            xrow = xbase;
            off = (unsigned)(mem < k ? mem : k - 1) * ldxb + (unsigned)lrc * 8u;
          }
          xb[tm][q] = *reinterpret_cast<const double*>(xrow + off);
        }
      double xs = 0.0;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + h < k);
          xb[tm][q] = live ? xb[tm][q] : 0.0;
          xs += xb[tm][q];
        }
      const double xm = tile64_add_h(xs) * P.inv_k;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + h < k);
          xb[tm][q] = live ? xb[tm][q] - xm : 0.0;
        }
      // ---- Z = Yw X', the wave's row blocks
      d4t va[TW], vb[TW], aphi[TW], apsi[TW], y[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i) va[i] = d4t{0., 0., 0., 0.};
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int mem = 16 * tm + 4 * q + h;
          const bool ok = tm < KT - 1 || mem < k;
          const int col = ok ? mem : 0;
#pragma unroll
          for (int i = 0; i < TW; ++i) {
            const double v = Yw[(16 * to[i] + lr) * KS + col];
            va[i] = MIA_MFMA64(ok ? v : 0.0, xb[tm][q], va[i]);
          }
        }
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
      // ---- x' w_mean = sum_b d_b (w_b psi_b): row vector of the innovations (column k of the records) times D^2 o Psi, the
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
      const double zu = __shfl(zacc[0], lr, 64);
      const double mterm = xm + zu;
      __syncthreads();
      // ---- Xa' = Yw^T (D^2 o Phi): D o phi(S) z = D^2 o (accumulated v) is the right-hand side, complete in every wave;
      //      output member blocks tj = wv, wv + NW, ...
      publish(aphi);
      __syncthreads();
      d4t bphi[UT];
#pragma unroll
      for (int tk = 0; tk < UT; ++tk)
#pragma unroll
        for (int q = 0; q < 4; ++q) bphi[tk][q] = bx[(4 * tk + q) * 64 + lane];
      char* obase = reinterpret_cast<char*>(P.Xa + (int64_t)mi * k * P.ldo + oc0);
      const bool wr = colact && !decl;
#pragma clang loop unroll(disable)
      for (int tj = wv; tj < KT; tj += NW) {
        d4t acc = {0., 0., 0., 0.};
        const int mcol = 16 * tj + lr < k ? 16 * tj + lr : k - 1;      // the output row this lane supplies to the A operand
        double xre[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + h + 4 * r;
          const double xv = *reinterpret_cast<const double*>(xbase + ((unsigned)(mem < k ? mem : k - 1) * ldxb + (unsigned)lrc * 8u));
          xre[r] = (colact && mem < k) ? xv : 0.0;
        }
#pragma unroll
        for (int tk = 0; tk < UT; ++tk)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = MIA_MFMA64(Yw[(16 * tk + 4 * q + h) * KS + mcol], bphi[tk][q], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + h + 4 * r;
          const double o = acc[r] + (mterm + P.f0 * (xre[r] - xm));
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + ((unsigned)mem * ldob + (unsigned)lr * 8u)) = o;
        }
      }
      __syncthreads();          // (the next state row publishes into bx)
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
static int wide64_launch_t(const Wide64Params& tp, hipStream_t stream) {
  // p_max <= k bounds UT = ceil((p_max + 8) / 16) by KT + 1: the other pairs are never asked for and not built
  if constexpr (UT > KT + 1) return MIA_ERR_UNSUPPORTED;
  else
    return launch_blocks(letkf_wide64_kernel<UT, KT, NW>, (tp.ng + 15) >> 4, 64 * NW, wide64_lds_bytes(UT, KT, NW), stream,
                         [] { note_analysis_kernel("letkf_wide64_kernel<%d, %d, %d>", UT, KT, NW); }, tp);
}

bool wide64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng) {
  if (m < 1 || k < 2 || k > 128 || p_max < 0 || p_max > k || ldx < 1 || ldo < 1 || ng < 0) return false;
  // the state and the output are addressed as wave-uniform base + 32-bit byte offset of a column of one state row block
  if ((int64_t)k * ldx * 8 >= ((int64_t)1 << 31) || (int64_t)k * ldo * 8 >= ((int64_t)1 << 31)) return false;
  const int ut = wide64_ut(p_max);
  if (wide64_lds_bytes(ut, (k + 15) >> 4, wide64_nw(ut)) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int wide64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                           hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!wide64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Dual);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Wide64Params tp;
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
  return dispatch_upto<8>(wide64_ut(p_max), [&](auto ut) {
    return dispatch_upto<8>(kt, [&](auto kt_c) { return wide64_launch_t<ut(), kt_c(), wide64_nw(ut())>(tp, stream); });
  });
}

}  // namespace mia
