// Localised kernel ETKF (RBF / Gauss kernel) in FLOAT64, sixteen grid points per workgroup of four wavefronts: the default
// working precision of LKETKF(RBFKernel(gamma), localization) / LETKF with a GaussKernel arrives here instead of at the
// one-point-per-wavefront Jacobi kernel (a 40 x 40 eigensolve per grid point).
//
// Reference: KETKFModule._estimate_weights (pytassim/core/ketkf.py:65-94) with RBFKernel / GaussKernel
// (pytassim/kernels/rbf.py:75-81,110-111) under wrapper_localization (pytassim/interface/wrapper.py:86-98) and the
// transform of interface/base.py:257-278; the float32 twin is lketkf_tile.hip, whose header states the mathematics.  Per
// grid point g, members a, b and the point's local observations s with Gaspari-Cohn weights rho_sg:
//     Dist[(a, b), g] = sum_s (y_as - y_bs)^2 rho_sg      (and the k member / observation pairs (y_as - d_s)^2)
//     K = exp(-gamma Dist), ko likewise;   Kc = C K C,   koc = ko - mean(ko) - (rowmean(K) - mean(K))
//     xa = mean + x'^T (Kc + reg)^-1 koc + sqrt(k-1) (Kc + reg)^-1/2 x',      reg = (k-1) / inf
//
// Input is what mia_letkf_analysis_matfun_f64 takes -- float64 records [P][kp] and the per-point lists with their float64
// sqrt(rho) -- so the route does not depend on the metric that made the lists.  The union of a tile's sixteen lists is
// formed here exactly as in letkf_tile64.hip: slot = RANK of the observation index in the union, steps ascending, zero
// records and rho = 0 beyond the union.  (Every wavefront forms the union for itself from the same lists: the four copies
// are equal, so is every branch taken on them, and the workgroup's barriers stay in uniform control flow.)
//
// Matrix-core part.  Dist is ONE product per tile on v_mfma_f64_16x16x4_f64: rows = pairs in blocks of sixteen (the upper
// triangle of K with its diagonal, T(a, b) = a k - a (a - 1) / 2 + b - a for a <= b, then the k observation pairs), columns =
// the sixteen points, depth = the union's slots.  Lane (lr, h) forms the A operand (y_as - y_bs)^2 of pair 16 blk + lr, slot
// 16 t + 4 q + h from the record image in LDS; the B operand is rho = D^2 as the lists give it.  The pair blocks are dealt
// round-robin to the four wavefronts.  The result layout hands lane (lr, h) point lr's pairs h + 4 r of the block: it takes the
// float64 library exp and stores K[pair][point] to LDS (110 KB at k = 40).  Every step of the product is unconditional (all
// 4 UT steps; slots beyond the union hold zero records and rho = 0): there is NO branch between a matrix instruction and the
// first vector read of its result, builtins only.  The diagonal pairs give exp(-gamma 0) = 1 exactly.
//
// Per-point part.  K belongs to one point, so its matrix-vector products are float64 vector multiply-adds.  Thread t of the
// 256 owns point t & 15 and rows t >> 4, + 16, + 32 of that point's matrix; the current vector of every point is exchanged
// through two LDS buffers [k][16], one barrier per step.  The matrix functions come from the three-term Chebyshev recurrence
// with the primal pair of mia_cheb_table64.h (1 / u, 1 / u^2, u = sqrt(1 + t)) on Kc, applied implicitly: x' is centred and
// every K u is centred again through mean(K u) = r^T u / k, r = K 1 the row sums.  One Krylov sequence per state row, read
// with both coefficient sets.  The spectral bound is the largest row sum of K (K > 0 entrywise, ||C K C|| <= ||K|| <= k).
//
// Summation order is canonical: slots by rank with exact zeros in between, members ascending in every matrix-vector product,
// row sum, mean and dot product (each thread sums all k terms itself, no tree over threads): a point's result does not
// depend on tile composition, shard boundaries or launch geometry.
//
// A tile whose union exceeds the 16 UT slots of its instantiation is processed in halves (quarters, ...): one point always
// fits (p_max <= 16 UT is checked on the host).  A tile that holds a non-finite record is analysed point by point; the
// points that see the record are DECLINED (MIA_FLAG_RETRY, counted, Xa untouched), as are points whose degree exceeds the
// table's cap, and redone by letkf_wave_kernel<double>.  A point without local observations gets the prior branch, whatever
// its degree would be, and does not count towards the tile's largest degree.
//
// Kernel expressions (template parameter ST != 0; instantiated in lketkf_kern64.hip, which includes this file).  Every other
// reference kernel and every +, *, ** composition is a function of three pair statistics (mia_kernel_prog.h), and each of them
// is the same product with other operands:
//     x.y        A = y_as y_bs,       B = rho
//     |x - y|^2  A = (y_as - y_bs)^2, B = rho
//     |x - y|_1  A = |y_as - y_bs|,   B = sqrt(rho)     (letkf_wave.hip takes the statistics of the sqrt(rho)-scaled block)
// ST is the set of statistics an instantiation forms (kStatDot | kStatSq | kStatL1), one accumulator chain each over the same
// 4 UT unconditional steps.  The accumulators are then copied into ordinary registers by unconditional additions BEFORE the
// interpreter's first (wave-uniform) branch -- DESIGN 4.2 -- and lane (lr, h) evaluates the program (kprog_eval) on its four
// (pair h + 4 r, point lr) results.  `same` (DiagKernel) belongs to the RESULT row: it is true exactly for the pairs T(a, a),
// read from the pair table, and false for the k observation pairs (diag.py:65-66).  Everything after K is in LDS is the RBF
// form's, with one difference: a dot-product kernel has negative entries, so the spectral bound is the largest ABSOLUTE row
// sum (||C K C|| <= ||K||_2 <= ||K||_inf for a symmetric K); the signed row sums still centre.  The recurrence is right only for a
// positive semidefinite K -- the reference clamps negative eigenvalues, a polynomial cannot --: the caller vouches for that
// (kernels.py, kernel_is_psd).
#include "mia_cheb_table64.h"
#include "mia_kernel_prog.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"

namespace mia {

struct Rbf64Params {
  const double* X; int64_t ldx; int m; int k; int kp;
  int64_t g0, ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  double reg, inv_reg, f0, inv_k, cs_phi, cs_psi, ngamma;
  double* Xa; int64_t ldo, o0; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
  KernelProgram<double> prog;                                // (ST != 0 only)
};

// pair statistics an instantiation forms for a kernel expression; 0 = none: the RBF form, exp(ngamma Dist)
constexpr int kStatDot = 1, kStatSq = 2, kStatL1 = 4;

constexpr int kRbf64MaxK = 40;

// pairs of a k-member ensemble (upper triangle with diagonal + observation pairs), in blocks of sixteen
static inline int rbf64_pair_blocks(int k) { return (k * (k + 1) / 2 + k + 15) >> 4; }
// doubles of the region that holds the record image and sqrt(rho) during the Dist product, and the vectors afterwards
__host__ __device__ static inline size_t rbf64_region(int ut, int k, int kp) {
  const size_t a = (size_t)16 * ut * (kp | 1) + 16 * (size_t)(16 * ut + 1), b = (size_t)4 * 16 * k;
  return a > b ? a : b;
}

// UT: 16-slot blocks of the union an instantiation holds; NR = ceil(k / 16): rows of a point's matrix a thread owns;
// ST: statistics set of a kernel expression (0: RBF)
template <int UT, int NR, int ST>
__global__ __launch_bounds__(256, 2) void lketkf_tile64_kernel(Rbf64Params P) {
  constexpr int UMAX = 16 * UT, NU = 4 * UT, DS = UMAX + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = P.k, kp = P.kp, pm = P.p_max;
  const int KS = kp | 1;                                     // odd row pitch (in doubles) of the record image
  const int NT = k * (k + 1) / 2, NPB = (NT + k + 15) >> 4;
  double* Kt = reinterpret_cast<double*>(smem_raw);          // [16 NPB][16]  K of (pair, point); rows NT .. NT + k - 1: ko
  double* Yw = Kt + (size_t)NPB * 256;                       // [UMAX][KS]    union records, zero rows beyond the union
  double* Dl = Yw + UMAX * KS;                               // [16][DS]      sqrt(rho) of (point, slot), 0 = not local
  double* V0 = Yw;                                           // (after the Dist product) [k][16] vectors of the recurrence,
  double* V1 = V0 + 16 * k;
  double* Rs = V1 + 16 * k;                                  //   row sums of K,
  double* Kc = Rs + 16 * k;                                  //   centred kernel vector koc
  int* ukey = reinterpret_cast<int*>(Yw + rbf64_region(UT, k, kp));   // [UMAX] observation index of a slot, -1 = unused
  int* PA = ukey + UMAX;                                     // [16 NPB] members (a | b << 8) of a pair
  int* pcnt = PA + 16 * NPB;                                 // [16] list length of a point (0: none, absent or overflown)
  int* pfl = pcnt + 16;                                      // [16] output flags of a point
  int* sflag = pfl + 16;                                     // [1]  the record image holds a non-finite value

  // XCD-aware block -> tile map, as letkf_tile64.hip
  const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t ntile = (P.ng + 15) >> 4;
  if (bid >= ntile) return;
  const int64_t q8 = ntile >> 3, r8 = ntile & 7, xcd = bid & 7;
  const int64_t tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int64_t p0 = tile << 4;                              // first point of the tile (index into the launch's ng points)
  const int npts = P.ng - p0 < 16 ? (int)(P.ng - p0) : 16;
  const int64_t oc0 = P.o0 + p0;                             // output column of the tile's first point
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;

  // ---- the pair table (padding pairs: (0, 0))
  for (int i = tid; i < 16 * NPB; i += 256) PA[i] = 0;
  __syncthreads();
  for (int a = tid; a < k; a += 256) {
    const int base = a * k - a * (a - 1) / 2;
    for (int b = a; b < k; ++b) PA[base + b - a] = a | (b << 8);
    PA[NT + a] = a | (k << 8);                               // (column k of a record is the innovation)
  }

  // ---- the tile's neighbour lists, in every wavefront: lane (lp, sub) holds entries sub, sub + 4, ... of point lp
  //      (unconditional loads inside the row's storage; entries beyond the count become index -1)
  const int nl = pm < P.p_cap ? pm : P.p_cap;
  int eidx[NU];
  double ew[ST == 0 ? NU : 1];   // (a kernel expression reads sqrt(rho) again where it fills Dl: the interpreter needs the registers)
  int lcnt;
  unsigned long long badmask;
  {
    const int64_t row = p0 + (lp < npts ? lp : 0);
    lcnt = P.cnt[row];
    const int32_t* ib = P.idx + row * P.p_cap;
    const double* wb = P.w + row * P.p_cap;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int pos = sub + 4 * u;
      const int e = pos < nl ? pos : 0;
      eidx[u] = ib[e];
      if constexpr (ST == 0) ew[u] = wb[e];
    }
    const bool pbad = lp < npts && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad && wave == 0) {
      if (sub == 0) P.flags[p0 + lp] = MIA_FLAG_OVERFLOW;
      const double nanv = __builtin_nan("");
      for (int it = sub; it < P.m * k; it += 4) P.Xa[(int64_t)it * P.ldo + oc0 + lp] = nanv;
    }
    if (lp >= npts || pbad) lcnt = 0;
    badmask = __ballot(pbad);
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (sub + 4 * u >= lcnt) eidx[u] = -1;
    if (wave == 0 && sub == 0) pcnt[lp] = lcnt;
  }

  // this thread in the per-point part: point p, rows r0 + 16 i
  const int p = tid & 15, r0 = tid >> 4;
  const bool colok = p < npts && !((badmask >> (4 * p)) & 1ull);
  const int pc = p < npts ? p : npts - 1;                    // a column that exists (clamped, unconditional loads)

  int lo = 0;
#pragma clang loop unroll(disable)
  while (lo < npts) {
    // ---- union of the lists of points [lo, hi): slot = RANK of the observation index, found by repeated extraction of
    //      the smallest remaining key; shrink the range until the union fits and, where a record is not finite, to one point
    int n = 16, hi, U;
    int es[NU];            // slot of this lane's entries
    bool badrec;
    for (;;) {
      hi = lo + n < npts ? lo + n : npts;
      const bool act = lp >= lo && lp < hi;
      unsigned key1[NU];   // index + 1 of an entry that takes part, 0 otherwise
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        es[u] = -1;
        key1[u] = (act && eidx[u] >= 0) ? (unsigned)eidx[u] + 1u : 0u;
      }
      for (int i = tid; i < UMAX; i += 256) ukey[i] = -1;
      if (tid == 0) *sflag = 0;
      if (tid < 16) pfl[tid] = 0;
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
          if (lane == 0) ukey[U] = (int)(last - 1u);          // (the four wavefronts write the same value)
        }
        ++U;
        if (U > UMAX) break;
      }
      if (U > UMAX) { __syncthreads(); n >>= 1; continue; }     // (n = 1 always fits: a single list has at most UMAX entries)
      __syncthreads();
      // ---- the union's records, sixteen rows per trip: thread (tid >> 4) takes a row, its sixteen neighbours the columns
      double fin = 0.0;       // stays 0 while every value is finite (inf * 0 = NaN)
      for (int rr = 0; rr < UMAX; rr += 16) {
        const int r = rr + (tid >> 4);
        const int key = ukey[r];
        const double* src = P.rec + (int64_t)(key < 0 ? 0 : key) * kp;
        for (int c = tid & 15; c < kp; c += 16) {
          double v = 0.0;
          if (key >= 0) v = src[c];
          fin = fma(v, 0.0, fin);
          Yw[r * KS + c] = v;
        }
      }
      for (int i = tid; i < 16 * DS; i += 256) Dl[i] = 0.0;
      if (fin != fin) *sflag = 1;
      __syncthreads();
      badrec = *sflag != 0;
      // A non-finite record would reach EVERY column of the tile through the shared product (NaN * 0 = NaN), also the
      // points that do not see that observation.  Such a tile is analysed point by point.
      if (badrec && hi - lo > 1) { __syncthreads(); n = 1; continue; }
      break;
    }
    if (badrec) {            // one point, and it sees a non-finite record: the eigensolver kernel's business
      if (tid == 0) { P.flags[p0 + lo] = MIA_FLAG_RETRY; atomicAdd(P.retry_count, 1); }
      lo = hi;
      __syncthreads();
      continue;
    }
    if constexpr (ST == 0) {
#pragma unroll
      for (int u = 0; u < NU; ++u)
        if (es[u] >= 0) Dl[lp * DS + es[u]] = ew[u];           // (the four wavefronts write the same value)
    } else {
      const double* wb = P.w + (p0 + (lp < npts ? lp : 0)) * P.p_cap;
#pragma unroll
      for (int u = 0; u < NU; ++u)
        if (es[u] >= 0) Dl[lp * DS + es[u]] = wb[sub + 4 * u];   // (es >= 0: entry sub + 4 u lies inside the point's list)
    }
    __syncthreads();

    // ---- Dist on the matrix cores, exp, K to LDS: the pair blocks round-robin over the wavefronts
    if constexpr (ST == 0) {
      double rho[UT][4];      // B operand: rho of (slot 16 t + 4 q + h, point lr)
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dv = Dl[lr * DS + 16 * t + 4 * q + h];
          rho[t][q] = dv * dv;
        }
#pragma clang loop unroll(disable)
      for (int blk = wave; blk < NPB; blk += 4) {
        const int pa = PA[16 * blk + lr];
        const int ca = pa & 255, cb = pa >> 8;
        d4t acc = {0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < UT; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double* yr = Yw + (16 * t + 4 * q + h) * KS;
            const double df = yr[ca] - yr[cb];
            acc = MIA_MFMA64(df * df, rho[t][q], acc);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) Kt[(16 * blk + h + 4 * r) * 16 + lr] = exp(P.ngamma * acc[r]);
      }
    } else {
      // a kernel expression: one chain per statistic of the set.  sqrt(rho) is read from LDS at every step: 4 UT values of rho
      // (and of sqrt(rho)) held in registers beside three accumulators and the interpreter's pow spill to scratch at UT >= 3
#pragma clang loop unroll(disable)
      for (int blk = wave; blk < NPB; blk += 4) {
        const int pa = PA[16 * blk + lr];
        const int ca = pa & 255, cb = pa >> 8;
        d4t ad = {0., 0., 0., 0.}, as = {0., 0., 0., 0.}, al = {0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < UT; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int slot = 16 * t + 4 * q + h;
            const double* yr = Yw + slot * KS;
            const double ya = yr[ca], yb = yr[cb], df = ya - yb;
            const double dv = Dl[lr * DS + slot], rh = dv * dv;
            if constexpr ((ST & kStatDot) != 0) ad = MIA_MFMA64(ya * yb, rh, ad);
            if constexpr ((ST & kStatSq) != 0) as = MIA_MFMA64(df * df, rh, as);
            if constexpr ((ST & kStatL1) != 0) al = MIA_MFMA64(fabs(df), dv, al);
          }
        // the accumulators' first vector reads: unconditional, ahead of the interpreter's branches (x + 0.0 is not folded)
        double sd[4], ss[4], sl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sd[r] = (ST & kStatDot) ? ad[r] + 0.0 : 0.0;
          ss[r] = (ST & kStatSq) ? as[r] + 0.0 : 0.0;
          sl[r] = (ST & kStatL1) ? al[r] + 0.0 : 0.0;
        }
#pragma clang loop unroll(disable)
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * blk + h + 4 * r;               // the RESULT row's pair decides `same`, not the operand row's
          const int pr = PA[row];
          const bool same = row < NT && (pr & 255) == (pr >> 8);
          const double vd = r == 0 ? sd[0] : (r == 1 ? sd[1] : (r == 2 ? sd[2] : sd[3]));
          const double vs = r == 0 ? ss[0] : (r == 1 ? ss[1] : (r == 2 ? ss[2] : ss[3]));
          const double vl = r == 0 ? sl[0] : (r == 1 ? sl[1] : (r == 2 ? sl[2] : sl[3]));
          Kt[row * 16 + lr] = kprog_eval<double>(P.prog, vd, vs, vl, same);
        }
      }
    }
    __syncthreads();          // K complete; the record image is dead from here on

    // ---- row sums r = K 1 of this thread's rows, members ascending
    int ra[NR];               // row (clamped to an existing one)
    bool rok[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      rok[i] = r0 + 16 * i < k;
      ra[i] = rok[i] ? r0 + 16 * i : 0;
    }
    //      (a kernel expression: the absolute row sums beside them, parked in V1 until the recurrence's first barrier)
    {
      double rs[NR], rab[NR];
      int ix[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) { rs[i] = 0.0; rab[i] = 0.0; ix[i] = ra[i]; }
      for (int b = 0; b < k; ++b) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const double kv = Kt[ix[i] * 16 + p];
          rs[i] += kv;
          if constexpr (ST != 0) rab[i] += fabs(kv);
          ix[i] += b < ra[i] ? k - b - 1 : 1;
        }
      }
#pragma unroll
      for (int i = 0; i < NR; ++i)
        if (rok[i]) {
          Rs[ra[i] * 16 + p] = rs[i];
          if constexpr (ST != 0) V1[ra[i] * 16 + p] = rab[i];
        }
    }
    __syncthreads();
    // ---- spectral bound (largest row sum; of |K| for a kernel expression), degree and interval from the table; the centred
    //      kernel vector
    const bool colact = colok && p >= lo && p < hi;
    const bool noobs = pcnt[p] == 0;
    double alpha;
    int deg, tab_idx, pflag = 0;
    bool decl;
    {
      double L = 0.0, rsum = 0.0, kosum = 0.0;
      for (int b = 0; b < k; ++b) {
        const double v = Rs[b * 16 + p];
        const double bv = ST != 0 ? V1[b * 16 + p] : v;
        L = (bv > L || bv != bv) ? bv : L;
        rsum += v;
        kosum += Kt[(NT + b) * 16 + p];
      }
      const double rmean = rsum * P.inv_k * P.inv_k, komean = kosum * P.inv_k;
#pragma unroll
      for (int i = 0; i < NR; ++i)
        if (rok[i]) Kc[ra[i] * 16 + p] = Kt[(NT + ra[i]) * 16 + p] - komean - (Rs[ra[i] * 16 + p] * P.inv_k - rmean);
      L = fmax(L, 1e-300 * P.reg) * (1.0 + 1e-12);
      if (!(L == L) || !(fabs(L) < 1e300)) { pflag |= MIA_FLAG_NONFINITE; L = P.reg; }
      tab_idx = (int)ceil(double(kTabPerOctave) * log2(L * P.inv_reg)) + kTabIdx0;
      tab_idx = tab_idx < 0 ? 0 : (tab_idx > kTabN - 1 ? kTabN - 1 : tab_idx);
      const Tab64Hdr hd = P.tab_hdr[tab_idx];
      deg = hd.deg;
      // (a point without local observations takes the prior branch: its degree -- K = 1, L = k -- neither declines it nor
      //  lengthens the tile's recurrence)
      decl = colact && !noobs && (deg > P.dmax || deg > kTab64Deg - 1);
      alpha = (deg > kTab64Deg - 1) ? 0.0 : hd.two_over_T * P.inv_reg;             // (a declined column carries bounded junk)
      if (decl && r0 == 0) {
        P.flags[p0 + p] = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
    }
    // (every wavefront holds all sixteen points: the maximum is the same in the four)
    const int degmax = (int)tile64_wave_max_u32((colact && !decl && !noobs) ? (unsigned)deg : 0u);
    const double2* ctab = P.tab_c + (size_t)tab_idx * kTab64Deg;
    auto coef = [&](int j) -> double2 {                              // (zero beyond a point's own degree)
      return ctab[j < kTab64Deg ? j : kTab64Deg - 1];
    };
    const bool wr = colact && !decl;

    for (int mi = 0; mi < P.m; ++mi) {
      const double* xbase = P.X + (int64_t)mi * k * P.ldx + P.g0 + p0 + pc;
      double xr[NR], vcur[NR], vold[NR], aphi[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        xr[i] = xbase[(int64_t)ra[i] * P.ldx];
        if (rok[i]) V0[ra[i] * 16 + p] = xr[i];
      }
      __syncthreads();        // (also: koc and the row sums are complete)
      double xs = 0.0;
      for (int b = 0; b < k; ++b) xs += V0[b * 16 + p];
      const double xm = xs * P.inv_k;
      const double2 c0 = coef(0);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        vcur[i] = xr[i] - xm;
        vold[i] = 0.0;
        aphi[i] = c0.x * vcur[i];
      }
      double zacc = 0.0;
      // step j reads v_j (all members, ascending) from one buffer, writes this thread's rows of v_{j+1} into the other:
      // v_1 = alpha Kc v_0 - v_0, v_{j+1} = 2 (alpha Kc v_j - v_j) - v_{j-1}, Kc u = K u - r^T u / k for a centred u
      double shift = xm;      // (buffer 0 holds the state row itself: v_0 = x - mean)
      double2 cj = c0;
#pragma clang loop unroll(disable)
      for (int j = 0; j < degmax; ++j) {
        const double* Vs = (j & 1) ? V1 : V0;
        double* Vd = (j & 1) ? V0 : V1;
        const double2 cn = coef(j + 1);
        double y[NR], ru = 0.0, kd = 0.0;
        int ix[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) { y[i] = 0.0; ix[i] = ra[i]; }
        for (int b = 0; b < k; ++b) {
          const double vb = Vs[b * 16 + p] - shift;
          ru = fma(Rs[b * 16 + p], vb, ru);
          kd = fma(Kc[b * 16 + p], vb, kd);
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            y[i] = fma(Kt[ix[i] * 16 + p], vb, y[i]);
            ix[i] += b < ra[i] ? k - b - 1 : 1;
          }
        }
        zacc = fma(cj.y, kd, zacc);
        const double am = ru * P.inv_k;
        const double two = j == 0 ? 1.0 : 2.0;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const double vn = two * (alpha * (y[i] - am) - vcur[i]) - vold[i];
          vold[i] = vcur[i];
          vcur[i] = vn;
          aphi[i] = fma(cn.x, vn, aphi[i]);
          if (rok[i]) Vd[ra[i] * 16 + p] = vn;
        }
        shift = 0.0;
        cj = cn;
        __syncthreads();
      }
      {                       // koc . v of the last vector
        const double* Vs = (degmax & 1) ? V1 : V0;
        double kd = 0.0;
        for (int b = 0; b < k; ++b) kd = fma(Kc[b * 16 + p], Vs[b * 16 + p] - shift, kd);
        zacc = fma(cj.y, kd, zacc);
      }
      const double mterm = xm + P.cs_psi * zacc;
      double* obase = P.Xa + (int64_t)mi * k * P.ldo + oc0 + p;
      int pf = 0;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        // a point without local observations: the prior branch, mean + sqrt(inf) x' (core/etkf.py:91-95)
        const double o = noobs ? xm + P.f0 * (xr[i] - xm) : fma(P.cs_phi, aphi[i], mterm);
        if (wr && rok[i]) {
          if (!(fabs(o) <= 1e300)) pf = MIA_FLAG_NONFINITE;
          obase[(int64_t)ra[i] * P.ldo] = o;
        }
      }
      pflag |= pf;
      __syncthreads();        // (the next state row overwrites buffer 0)
    }
    if (wr && pflag) atomicOr(&pfl[p], pflag);
    __syncthreads();
    if (wr && r0 == 0) P.flags[p0 + p] = pfl[p] | ((deg < kTab64Deg ? deg : kTab64Deg - 1) << 8);
    lo = hi;
    __syncthreads();
  }
}

static size_t rbf64_lds_bytes(int ut, int k) {
  const int kp = (k + 1 + 3) & ~3, npb = rbf64_pair_blocks(k);
  return align_up(((size_t)npb * 256 + rbf64_region(ut, k, kp)) * sizeof(double) + ((size_t)16 * ut + 16 * (size_t)npb + 48) * sizeof(int), 16);
}

// (a frame of its own: pair blocks and statistic region above; UT from p_max as the resident image, resident64_ut)
template <int UT, int NR, int ST>
static int rbf64_launch_t(const Rbf64Params& tp, hipStream_t stream) {
  return launch_blocks(lketkf_tile64_kernel<UT, NR, ST>, (tp.ng + 15) >> 4, 256, rbf64_lds_bytes(UT, tp.k), stream,
                       [] { note_analysis_kernel("lketkf_tile64_kernel<%d, %d, %d>", UT, NR, ST); }, tp);     // (ST: 0 RBF; 1 dot, 2 sq, 7 dot + sq + l1)
}

template <int ST>
static int rbf64_launch_s(const Rbf64Params& tp, hipStream_t stream) {
  return dispatch_upto<4>(resident64_ut(tp.p_max), [&](auto ut) {
    return dispatch_upto<3>((tp.k + 15) >> 4, [&](auto nr) { return rbf64_launch_t<ut(), nr(), ST>(tp, stream); });
  });
}

// the parameter block of both forms (ngamma and prog are the caller's)
static Rbf64Params rbf64_params(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                                const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                                double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                                const CoefTable64* tab) {
  Rbf64Params tp;
  tp.X = X; tp.ldx = ldx; tp.m = m; tp.k = k; tp.kp = (k + 1 + 3) & ~3;
  tp.g0 = g0; tp.ng = ng; tp.rec = rec;
  tp.cnt = nbr_cnt; tp.idx = nbr_idx; tp.w = nbr_w; tp.p_cap = p_cap; tp.p_max = p_max;
  const double rg = (double)(k - 1) / inf_factor, km = (double)(k - 1);
  tp.reg = rg;
  tp.inv_reg = 1.0 / rg;
  tp.f0 = sqrt(km / rg);
  tp.inv_k = 1.0 / (double)k;
  tp.cs_phi = sqrt(km) / sqrt(rg);
  tp.cs_psi = 1.0 / rg;
  tp.ngamma = 0.0;
  tp.Xa = Xa; tp.ldo = ldo; tp.o0 = o0; tp.flags = flags; tp.retry_count = retry_count;
  tp.dmax = kTab64Deg - 1;
  tp.tab_hdr = tab->hdr; tp.tab_c = tab->c;
  tp.prog.n = 0;
  return tp;
}

#ifndef MIA_KERN64_TU
// RBF kernel, float64, 2 <= k <= 40 members, lists of at most 64 observations (no p_max <= k condition: the matrix is k x k)
bool rbf64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng) {
  if (m < 1 || k < 2 || k > kRbf64MaxK || p_max < 0 || p_max > 64 || ldx < 1 || ldo < 1 || ng < 0) return false;
  if (rbf64_lds_bytes(resident64_ut(p_max), k) > kMaxDynamicLds) return false;
  return grid_covers((ng + 15) >> 4);
}

int rbf64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                          const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                          double inf_factor, double gamma, double* Xa, int64_t ldo, int64_t o0, int32_t* flags,
                          int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count || !(gamma > 0.0)) return MIA_ERR_UNSUPPORTED;
  if (!rbf64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Rbf64Params tp = rbf64_params(X, ldx, m, k, g0, ng, rec, nbr_cnt, nbr_idx, nbr_w, p_cap, p_max, inf_factor, Xa, ldo, o0, flags,
                                retry_count, tab);
  tp.ngamma = -gamma;
  return rbf64_launch_s<0>(tp, stream);
}
#else
// (this translation unit = lketkf_kern64.hip: the kernel-expression instantiations, compiled beside the RBF ones)
// The cover is the RBF form's (same LDS layout).  A program's statistics are rounded up to one of three compiled sets:
// {dot}, {sq}, {dot, sq, l1}; tanh and sin make no positive semidefinite kernel the package knows: MIA_ERR_UNSUPPORTED.
int kern64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, const mia_kernel_op_t* prog, int n_ops, double* Xa, int64_t ldo, int64_t o0,
                           int32_t* flags, int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (kernel_program_check(prog, n_ops) != MIA_OK) return MIA_ERR_UNSUPPORTED;
  if (!rbf64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  int need = 0;
  for (int i = 0; i < n_ops; ++i) {
    const int op = prog[i].op;
    if (op == MIA_KOP_TANH || op == MIA_KOP_SIN) return MIA_ERR_UNSUPPORTED;
    if (op == MIA_KOP_DOT) need |= kStatDot;
    if (op == MIA_KOP_SQDIST) need |= kStatSq;
    if (op == MIA_KOP_L1DIST) need |= kStatL1;
  }
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Rbf64Params tp = rbf64_params(X, ldx, m, k, g0, ng, rec, nbr_cnt, nbr_idx, nbr_w, p_cap, p_max, inf_factor, Xa, ldo, o0, flags,
                                retry_count, tab);
  tp.prog.n = n_ops;
  for (int i = 0; i < n_ops; ++i) { tp.prog.op[i] = (unsigned char)prog[i].op; tp.prog.val[i] = prog[i].value; }
  if (need == kStatDot) return rbf64_launch_s<kStatDot>(tp, stream);
  if (need == kStatSq || need == 0) return rbf64_launch_s<kStatSq>(tp, stream);      // (a constant kernel needs none)
  return rbf64_launch_s<kStatDot | kStatSq | kStatL1>(tp, stream);
}
#endif

}  // namespace mia
