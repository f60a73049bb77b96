// The LETKF WEIGHTS in FLOAT64 for DENSE local networks (p_max > k) of ensembles up to 128 members, sixteen grid points per
// wavefront, every contraction on the matrix cores (v_mfma_f64_16x16x4_f64): what LETKF.estimate_weights returns
// (interface/letkf.py:127-146, core/etkf.py:57-103), W[g][i][j] = w_mean_i + W_pert_ij, without an eigensolver.
//
// The frame is the ring family's (csrc/mia_ring64_dev.h: mathematics of the products, lane roles, summation order, the ring
// and the rules of the run-time loops) and, block for block, letkf_stream64.hip's up to and including the degree
// and decline of every point: per-point lists of any metric, union by rank extraction, the union's records streamed through
// a ring of two sixteen-slot blocks in LDS, rhs in LDS, the streamed Gershgorin bound, the primal table.  What stays in LDS
// per wave is the sqrt(rho) table, the slot table, the ring and the tile's rhs: 256 slots at every 2 <= k <= 128.
//
// What differs is letkf_tile64w.hip's: instead of one pass per state row there is one pass per MEMBER c < k
// with x' = e_c -- no state load, no mean.  With reg = (k - 1) / inf, C_g = Yw^T diag(rho_g) Yw (k x k, what the reference
// decomposes), rhs_g = Yw^T (rho_g o d), f0 = sqrt((k - 1) / reg), phi(t) = 1 / sqrt(1 + t), psi(t) = 1 / (1 + t), t = lambda / reg:
//
//     W[g][c][j] = wm_c + f0 (phi(C_g) e_c)_j,        wm_c = (psi(C_g) e_c) . rhs_g / reg
//
// (both matrices are symmetric: column c, which the recurrence on e_c produces, is row c), both functions from ONE Chebyshev
// recurrence on e_c.  W is [g1 - g0][k][k]: n k^2 8 bytes exceed 2^31 at 1e5 points, so a pass addresses it as a 64-bit
// wave-uniform base (tile, row c) + a 32-bit lane offset (16 k^2 8 <= 2^21).  For fixed (tj, r) the four lane groups h hold
// four consecutive j: one store instruction writes sixteen 32-byte segments, one per point.  A point WITHOUT observations
// gets sqrt(inf) I exactly (etkf.py:91-95): the truncated series at C = 0 is only about 1, so such a column is written
// directly, takes no part in the tile's degree and reports flag 0.
//
// A tile whose union exceeds the slots of the launch is processed in halves (quarters, ...): one point always fits.  A tile
// that holds a non-finite record is done point by point.  Points whose degree exceeds the table's cap are DECLINED
// (MIA_FLAG_RETRY, counted, their k x k block of W untouched) and redone with weights by letkf_wave_kernel<double>
// (mia_letkf_weights_retry_f64) where that kernel holds the shape.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_ring64_dev.h"
#include "mia_tile_launch.h"

namespace mia {

struct Stream64WParams {
  int k; int kp;
  int64_t ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  int ub;                                                    // sixteen-slot blocks of the slot table of the launch
  double reg, inv_reg, cs_phi, cs_psi, f_id;                 // f_id = sqrt(inf): the diagonal of a point without observations
  double* W; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// KT = ceil(k / 16).  One wavefront per workgroup; its LDS bounds how many share a compute unit.
template <int KT>
__global__ __launch_bounds__(64, 1) void letkf_stream64w_kernel(Stream64WParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int k = P.k, kp = P.kp, pm = P.p_max;
  const int UMAX = 16 * P.ub, DS = UMAX + 1;
  const int KS = kp | 1;                                     // odd row pitch (in doubles) of a staged block
  double* Ring = reinterpret_cast<double*>(smem_raw);        // [2][16][KS] two sixteen-slot blocks of union records
  double* Rl = Ring + 2 * 16 * KS;                           // [4 KT][64]  rhs of the tile, every lane its own registers' worth
  double* Dl = Rl + 4 * KT * 64;                             // [16][DS]    sqrt(rho) of (point, slot), 0 = not local
  int* ukey = reinterpret_cast<int*>(Dl + 16 * DS);          // [UMAX]      observation index of a slot, ascending; -1 = none
  unsigned* Kl = reinterpret_cast<unsigned*>(Dl);            // [16][nl]    index + 1 of the lists' entries while the union is formed

  const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t ntile = (P.ng + 15) >> 4;
  if (bid >= ntile) return;
  const int64_t tile = ring64_tile_of_block(bid, ntile);
  const int64_t p0 = tile << 4;                              // first point of the tile (index into the launch's ng points)
  const int npts = P.ng - p0 < 16 ? (int)(P.ng - p0) : 16;
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;
  const unsigned kk8 = (unsigned)(k * k) * 8u;               // bytes of one point's weights

  // ---- the tile's neighbour lists stay in memory: lane (lp, sub) walks entries sub, sub + 4, ... of point lp
  int nl = pm < P.p_cap ? pm : P.p_cap;
  nl = nl < UMAX ? nl : UMAX;
  const int64_t lrow = p0 + (lp < npts ? lp : 0);            // (lists, flags and weights count from the shard's g0)
  const int32_t* ib = P.idx + lrow * P.p_cap;
  const double* wb = P.w + lrow * P.p_cap;
  int lcnt = P.cnt[lrow];
  unsigned long long badmask;
  {
    const bool pbad = lp < npts && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad) {
      if (sub == 0) P.flags[p0 + lp] = MIA_FLAG_OVERFLOW;
      const double nanv = __builtin_nan("");
      double* wp = P.W + (p0 + lp) * (int64_t)(k * k);
      for (int it = sub; it < k * k; it += 4) wp[it] = nanv;
    }
    if (lp >= npts || pbad) lcnt = 0;
    badmask = __ballot(pbad);
  }
  // a point without observations: sqrt(inf) I, written directly (lanes 4 lr .. 4 lr + 3 hold point lr's count)
  const bool cempty = __shfl(lcnt, 4 * lr, 64) == 0;

  // ---- the ring (mia_ring64_dev.h); st holds the block this lane has staged
  int UB = 1;
  int cur = 0;                                               // the half that holds the block of the trip
  double st[4][Ring64<KT>::NC];
  const Ring64<KT> ring{Ring, P.rec, ukey, k, kp, KS, lr, h, cur, st};

  int lo = 0;
  bool single = false;                                       // a non-finite record was met: the rest of the tile goes point by point
#pragma clang loop unroll(disable)
  while (lo < npts) {
    const bool colok = lr < npts && !((badmask >> (4 * lr)) & 1ull);
    const double* Dcol = Dl + lr * DS + h;                    // + 16 t + 4 r: slot 16 t + h + 4 r of column lr
    // ---- union of the lists of points [lo, hi): slot = RANK of the observation index, found by repeated extraction of
    //      the smallest remaining key (one sweep over the keys in LDS and one DPP reduction per slot); shrink the range
    //      until the union fits
    int n = single ? 1 : 16, hi, U;
    bool act;
    for (;;) {
      hi = lo + n < npts ? lo + n : npts;
      act = lp >= lo && lp < hi;
      for (int pos = sub; pos < nl; pos += 4) {
        int e = -1;
        if (act && pos < lcnt) e = ib[pos];
        Kl[lp * nl + pos] = e >= 0 ? (unsigned)e + 1u : 0u;
      }
      for (int i = lane; i < UMAX; i += 64) ukey[i] = -1;
      __syncthreads();
      U = 0;
      unsigned last = 0u;
      const int e0 = lo * nl, e1 = hi * nl;
#pragma clang loop unroll(disable)
      for (;;) {
        unsigned best = 0u;                       // ~(smallest key above `last`), 0 = none left
        for (int e = e0 + lane; e < e1; e += 64) {
          const unsigned key1 = Kl[e];
          const unsigned cand = key1 > last ? ~key1 : 0u;
          best = cand > best ? cand : best;
        }
        best = tile64_wave_max_u32(best);
        if (best == 0u) break;
        last = ~best;
        if (U < UMAX && lane == 0) ukey[U] = (int)(last - 1u);
        ++U;
        if (U > UMAX) break;
      }
      if (U > UMAX) { __syncthreads(); n >>= 1; continue; }     // (n = 1 always fits: a single list has at most UMAX entries)
      __syncthreads();
      UB = (U + 15) >> 4;
      UB = UB < 1 ? 1 : UB;                                      // blocks in use; slots up to 16 UB are staged
      // ---- sqrt(rho) of (point, slot): the slot of an entry is the place of its index in the sorted slot table
      for (int i = lane; i < 16 * DS; i += 64) Dl[i] = 0.0;     // (over the keys: every lane is past the barrier behind their last read)
      __syncthreads();
      if (act)
        for (int pos = sub; pos < lcnt; pos += 4) {
          const int key = ib[pos];
          if (key < 0) continue;
          int a = 0, b = U;
          while (a < b) {
            const int mid = (a + b) >> 1;
            if (ukey[mid] < key) a = mid + 1; else b = mid;
          }
          Dl[lp * DS + a] = wb[pos];
        }
      // ---- block 0 into the ring
      double fin = 0.0;
      ring.stage(0);
      ring.commit(cur, fin);
      __syncthreads();
      // ---- rhs_g = Yw^T (rho_g o d), once per tile (d = column k of the records); this first pass over the union also
      //      looks at every record (blocks 1 .. UB - 1 and block 0 again pass through commit)
      d4t rhs[KT];
#pragma unroll
      for (int tj = 0; tj < KT; ++tj) rhs[tj] = d4t{0., 0., 0., 0.};
      {
        int tb = 0;
#pragma clang loop unroll(disable)
        do {
          ring.stage(tb + 1 < UB ? tb + 1 : 0);
          double s[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double dv = Dcol[16 * tb + 4 * q];
            s[q] = dv * dv * Ring[cur * 16 * KS + (4 * q + h) * KS + k];
          }
          ring.fold(s, rhs);
          ring.turn(fin);
        } while (++tb < UB);
      }
      // A non-finite record would reach EVERY column of the tile through the shared products (NaN * 0 = NaN), also the
      // points that do not see that observation.  Such a tile is analysed point by point: the union is then the point's
      // own list and the damage stays where the reference has it.
      if (__any(fin != fin) && hi - lo > 1) { __syncthreads(); n = 1; single = true; continue; }
#pragma unroll
      for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rl[(4 * tj + r) * 64 + lane] = rhs[tj][r];
      break;
    }
    const bool colact = colok && lr >= lo && lr < hi;
    double nofin = 0.0;                                       // (the later passes do not look at the records again)
    // ---- Gershgorin bound of every point, streamed: L_g = max_a w_a sum_b |G_ab| w_b.  Row block t is read from memory as
    //      B operands (slot 16 t + lr, member 16 tm + 4 q + h); every Gram block (tk, t) is formed (4 KT instructions),
    //      folded into the row sums (4) and dropped
    double L = 0.0;
    {
      int t = 0;
#pragma clang loop unroll(disable)
      do {
        double at[KT][4];
        {
          const int key = ukey[16 * t + lr];
          const double* src = P.rec + ((int64_t)(key < 0 ? 0 : key) * kp + h);
#pragma unroll
          for (int tm = 0; tm < KT; ++tm)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              double v = 0.0;
              if (key >= 0 && (tm < KT - 1 || 16 * tm + 4 * q + h < k)) v = src[16 * tm + 4 * q];
              at[tm][q] = v;
            }
        }
        d4t R = {0., 0., 0., 0.};
        int tk = 0;
#pragma clang loop unroll(disable)
        do {
          ring.stage(tk + 1 < UB ? tk + 1 : 0);
          __builtin_amdgcn_sched_barrier(0);
          const d4t Gb = ring.chain(at);
          double dk[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) dk[q] = Dcol[16 * tk + 4 * q];
#pragma unroll
          for (int q = 0; q < 4; ++q) R = MIA_MFMA64(fabs(Gb[q]), dk[q], R);
          ring.turn(nofin);
        } while (++tk < UB);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = Dcol[16 * t + 4 * r] * R[r];
          L = (v > L || v != v) ? v : L;
        }
      } while (++t < UB);
    }
    // ---- degree and interval of every point from the table
    double alpha;
    int deg, tab_idx, pflag = 0;
    bool decl;
    {
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
    // (a column without observations is written directly: its series is not looked at and asks for no step)
    const int degmax = (int)tile64_wave_max_u32((colact && !decl && !cempty) ? (unsigned)deg : 0u);
    const Coef64 coef{P.tab_c + (size_t)tab_idx * kTab64Deg, P.cs_phi, P.cs_psi};

#pragma clang loop unroll(disable)
    for (int c = 0; c < k; ++c) {
      // (lane roles through opaque copies, as in letkf_tile64.hip: what is invariant in this loop -- the member numbers of the
      // start vector, the 4 KT offsets of the output, their predicates -- would otherwise be hoisted and held in registers
      // across the recurrence, which has none to spare)
      int hv = h, lrv = lr;
      asm volatile("" : "+v"(hv), "+v"(lrv));
      d4t va[KT], vb[KT], aphi[KT], apsi[KT];
      // ---- the recurrence on the 16 columns at once: v_0 = e_c on live columns (member c < k always exists), v_1 = alpha C v_0 - v_0,
      //      v_{j+1} = 2 (alpha C v_j - v_j) - v_{j-1}
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) va[tm][q] = (colact && 16 * tm + 4 * q + hv == c) ? 1.0 : 0.0;
      const Recur64<KT> step{ring, Dcol, UB, nofin, alpha, aphi, apsi};     // product / advance of the recurrence
      {
        const double2 c0 = coef(0), c1 = coef(1);
#pragma unroll
        for (int t = 0; t < KT; ++t) vb[t] = -va[t];
        step.product(va, vb, alpha);                 // vb = v_1 = alpha C v_0 - v_0
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          aphi[t] = c0.x * va[t] + c1.x * vb[t];
          apsi[t] = c0.y * va[t] + c1.y * vb[t];
        }
      }
      int j = 2;
      double2 cj = coef(2), cj1 = coef(3);
#pragma clang loop unroll(disable)
      for (; j + 1 <= degmax; j += 2) {
        const double2 nj = coef(j + 2), nj1 = coef(j + 3);       // requested one trip ahead
        step.advance(va, vb, cj);          // va = v_j
        step.advance(vb, va, cj1);         // vb = v_{j+1}
        cj = nj; cj1 = nj1;
      }
      if (j <= degmax) step.advance(va, vb, cj);
      // ---- wm_c = (psi(C) e_c) . rhs / reg: members in the lane's registers first, then the four lane groups
      double zs = 0.0;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) zs = fma(apsi[tm][r], Rl[(4 * tm + r) * 64 + lane], zs);
      const double wm = tile64_add_h(zs);
      // row c of the sixteen points' weights: wave-uniform 64-bit base (tile, row c) + 32-bit lane offset (point lr, column j)
      char* obase = reinterpret_cast<char*>(P.W + (p0 * k + c) * (int64_t)k);
      const unsigned olane = (unsigned)lrv * kk8 + (unsigned)hv * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + hv + 4 * r;
          double o = aphi[tj][r] + wm;
          if (cempty) o = mem == c ? P.f_id : 0.0;
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * 8u)) = o;
        }
    }
    {
      if (!(colact && !decl)) pflag = 0;          // (columns that are not written do not report)
      const unsigned long long fb = __ballot(pflag != 0);
      const bool anyf = ((fb >> lr) & 0x0001000100010001ull) != 0ull;
      if (h == 0 && colact && !decl) P.flags[p0 + lr] = cempty ? 0 : ((anyf ? MIA_FLAG_NONFINITE : 0) | (deg << 8));
    }
    lo = hi;
    __syncthreads();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr int kStream64WMaxK = 128;

bool weights_stream64_route_covers(int k, int p_max, int64_t ng) {
  if (k < 2 || k > kStream64WMaxK || p_max <= k || ng < 0) return false;                // p_max <= k: the dual routes
  if (p_max > 16 * kRing64MaxBlocks) return false;
  // a pass addresses W as wave-uniform base (tile, row) + 32-bit byte offset inside the tile's sixteen matrices
  if ((int64_t)16 * k * k * 8 >= ((int64_t)1 << 31)) return false;
  if (ring64_lds_bytes(ring64_blocks(p_max), k) > kMaxDynamicLds) return false;   // (holds at every k: tests/test_stream64w_cover.py)
  return grid_covers((ng + 15) >> 4);
}

// launches with the sizes of the ring frame (mia_frames64.h)
template <int KT>
static int stream64w_launch_t(const Stream64WParams& dp, hipStream_t stream) {
  return launch_blocks(letkf_stream64w_kernel<KT>, (dp.ng + 15) >> 4, 64, ring64_lds_bytes(dp.ub, dp.k), stream,
                       [] { note_analysis_kernel("letkf_stream64w_kernel<%d>", KT); }, dp);
}

int weights_stream64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                            const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                            int32_t* retry_count, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !W || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!weights_stream64_route_covers(k, p_max, ng)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Stream64WParams dp;
  dp.k = k; dp.kp = (k + 1 + 3) & ~3;
  dp.ng = ng; dp.rec = rec;
  dp.cnt = nbr_cnt; dp.idx = nbr_idx; dp.w = nbr_w; dp.p_cap = p_cap; dp.p_max = p_max;
  dp.ub = ring64_blocks(p_max);
  const double rg = (double)(k - 1) / inf_factor, km = (double)(k - 1);
  dp.reg = rg;
  dp.inv_reg = 1.0 / rg;
  dp.cs_phi = sqrt(km / rg);                                  // f0
  dp.cs_psi = 1.0 / rg;
  dp.f_id = sqrt(inf_factor);
  dp.W = W; dp.flags = flags; dp.retry_count = retry_count;
  dp.dmax = kTab64Deg - 1;
  dp.tab_hdr = tab->hdr; dp.tab_c = tab->c;
  return dispatch_upto<8>((k + 15) >> 4, [&](auto kt) { return stream64w_launch_t<kt()>(dp, stream); });
}

}  // namespace mia
