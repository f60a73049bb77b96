// lienks_stream64.hip's IEnKS weight UPDATE (tau = 1, FLOAT64, dense local networks p_max > k, ensembles up to 128 members,
// sixteen grid points per wavefront, every contraction a v_mfma_f64_16x16x4_f64, the union's records streamed through a ring of
// two sixteen-slot blocks) with letkf_patch64w.hip's three changes to the FRAME; mathematics, lane roles,
// summation order, the ring and its stage / chain / fold / turn discipline and the run-time loops are the ring family's
// (csrc/mia_ring64_dev.h, shared), the row means, the rhs pass with the shift D^T w_mean, the streamed bound, table, decline,
// the bundle scaling and the prior test of the transform variant lienks_stream64.hip's (reference:
// core/ienks.py:108-141, 167-173 under interface/lienks.py:75-118) and are not restated here.
//
// 1. TILE MAP.  The sixteen points of tile t are tile_pts[16 t + s], s = 0 .. 15: indices into the launch's range [0, ng),
//    -1 = empty slot.  On a row-major 2-D mesh sixteen CONSECUTIVE points are a 16 x 1 strip whose lists have a union of 200
//    observations at radius 3 against 176 of a 4 x 4 patch: the strip runs in parts, the patch in one pass.  Through the map
//    go the list row, the count, the flag, the point's k x k block of W_out -- and the point's block of W_IN, which the
//    weights twin does not have: the row means, the prior test of the transform variant and the copy-back of a point without
//    observations (bit for bit, by the whole wavefront) read W_in + tile_pts[slot] w_stride; with w_stride = 0 there is ONE
//    shared matrix and no map on it.  Live slots need not be a prefix: a dead slot is clamped to the tile's first live point
//    for loads, takes no part (its bit of skipmask is set from the start) and every store is predicated.  The range loop
//    runs over SLOTS, starts a range at a live slot and ends at the last live one.  A tile without a live slot returns
//    before the union, as does a tile whose live points all lack observations, after their copy-back; an entry outside
//    [0, ng) is an empty slot.  Lists and flags stay in natural point order, so the redo of declined points
//    (mia_lienks_update_retry_f64) needs no map.
// 2. IMAGE SIZED BY THE CALLER.  `ub` sixteen-slot blocks of the sqrt(rho) table and the slot table, 1 <= ub <= 16 at every
//    ensemble size (the records are not resident); the caller has it from tile_union_census_kernel (letkf_patch64.hip).  A tile
//    whose union exceeds it runs in halves of its SLOTS, quarters, ...; a single list longer than the image, p_max or p_cap is
//    MIA_FLAG_OVERFLOW and NaN weights, never a truncated list.
// 3. THE STORES.  lienks_stream64.hip addresses W_out as a wave-uniform base (the tile's first point, row c) + a 32-bit lane
//    offset point k^2 8 + j 8, which needs a tile's points to be consecutive.  Under a map they lie anywhere in n k^2 8 bytes (more
//    than 2^31 at 1e5 points): every lane owns one column = one point, so it forms a 64-bit base W_out + tile_pts[slot] k^2 (once
//    per member pass, behind the recurrence: see there) and keeps the 32-bit part to c k 8 + j 8 < k^2 8 <= 2^17.  The per-point reads of W_in were wave-uniform per
//    point already (a 64-bit scalar base + a 32-bit lane offset inside the matrix): they take the point from the map.
//
// A point's observations are summed in ascending index order with exact zeros in between whatever else is in the tile, and its
// row means depend on its own matrix alone, so W and flags are lienks_stream64_kernel's bit for bit under any map
// (tests/test_gpu_ienks_patch64.py).
//
// The kernel keeps its own text for everything the map reaches (DESIGN 2.18 on letkf_patch64.hip: the map reaches every
// address the frame forms); what it does not reach is mia_ring64_dev.h's and mia_lienks_stream64_dev.h's.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_lienks_stream64_dev.h"
#include "mia_ring64_dev.h"
#include "mia_tile_launch.h"

namespace mia {

struct LienksPatch64Params {
  int k; int kp;
  int64_t ng;
  const double* Win; int64_t w_stride;     // [ng][k][k], or one [k][k] for all points when w_stride == 0
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  const int32_t* tile_pts; int64_t n_tiles;                  // [n_tiles][16] point of a slot, -1 = none
  int ub;                                                    // sixteen-slot blocks of the slot table of the launch: the caller's
  int transform;                           // 1: transform variant (D = Yl while Wp = I), 0: bundle variant (D = Yl / eps)
  double dscale, dshift;                   // 1 / eps and eps (bundle), 1 and 1 (transform)
  double reg, inv_reg, cs_phi, cs_psi;
  double* W; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// KT = ceil(k / 16).  One wavefront per workgroup; its LDS bounds how many share a compute unit.
template <int KT>
__global__ __launch_bounds__(64, 1) void lienks_patch64_kernel(LienksPatch64Params P) {
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
  const int64_t ntile = P.n_tiles;
  if (bid >= ntile) return;
  const int64_t tile = ring64_tile_of_block(bid, ntile);
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;
  const int64_t kk = (int64_t)(k * k);                       // doubles of one point's weights

  // ---- the tile's points: slot lr is this lane's column, slot lp the list it walks.  An entry outside [0, ng) is an empty
  //      slot (the census refuses such a map; nothing is ever indexed by one)
  const int32_t* tp = P.tile_pts + tile * 16;
  int ptc = tp[lr], ptl = tp[lp];
  ptc = (ptc >= 0 && ptc < P.ng) ? ptc : -1;
  ptl = (ptl >= 0 && ptl < P.ng) ? ptl : -1;
  const unsigned livemask = (unsigned)(__ballot(ptc >= 0) & 0xffffull);       // (lanes 0 .. 15 are slots 0 .. 15)
  if (livemask == 0u) return;
  const int nslot = 32 - __builtin_clz(livemask);             // one past the last live slot
  const int pfirst = tp[__builtin_ctz(livemask)];             // a point that exists: what dead slots load from
  const bool live_c = ptc >= 0, live_l = ptl >= 0;
  const int colpt = live_c ? ptc : pfirst;                    // (from here on the column's point: ptc is not used again)

  // ---- the tile's neighbour lists stay in memory: lane (lp, sub) walks entries sub, sub + 4, ... of slot lp's point
  int nl = pm < P.p_cap ? pm : P.p_cap;
  nl = nl < UMAX ? nl : UMAX;
  const int64_t lrow = live_l ? ptl : pfirst;                // (lists, flags and weights count from the shard's g0)
  const int32_t* ib = P.idx + lrow * P.p_cap;
  const double* wb = P.w + lrow * P.p_cap;
  int lcnt = P.cnt[lrow];
  const bool shared_w = P.w_stride == 0;
  unsigned long long skipmask;       // bit 4 s: slot s takes no part in the tile (dead, overflow, no observation, declined here)
  {
    const bool pbad = live_l && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad) {
      if (sub == 0) P.flags[ptl] = MIA_FLAG_OVERFLOW;
      const double nanv = __builtin_nan("");
      double* wp = P.W + (int64_t)ptl * kk;
      for (int it = sub; it < k * k; it += 4) wp[it] = nanv;
    }
    if (!live_l || pbad) lcnt = 0;
    // ---- no local observation: the weights go back as they came (core/ienks.py:135), the whole wavefront copying a point
    const unsigned long long emask = __ballot(live_l && !pbad && lcnt == 0);
    skipmask = __ballot(pbad || !live_l) | emask;
    for (int s = 0; s < nslot; ++s) {
      if (!((emask >> (4 * s)) & 1ull)) continue;
      const int64_t pt = tp[s];                              // (a live slot: wave-uniform, inside [0, ng))
      const double* win = P.Win + pt * P.w_stride;
      double* wout = P.W + pt * kk;
      for (int it = lane; it < k * k; it += 64) wout[it] = win[it];
      if (lane == 0) P.flags[pt] = 0;
    }
    // ---- transform variant: D = Wp^-1 Yl is Yl only at the prior; any other point with observations is the general kernel's
    if (P.transform) {
      unsigned np = 0u;                                      // bit s: slot s' point is not at the prior
      const int nscan = shared_w ? 1 : nslot;
      for (int s = 0; s < nscan; ++s) {
        if (!shared_w && ((skipmask >> (4 * s)) & 1ull)) continue;
        const int64_t pt = shared_w ? 0 : tp[s];             // (one shared matrix: no map on W_in)
        const double dev = lienks_stream64_prior_dev<KT>(P.Win + pt * P.w_stride, k, lr, h);
        if (__any(!(dev <= kStreamPriorTol))) np |= shared_w ? 0xffffu : (1u << s);
      }
      const bool pnot = live_l && lcnt > 0 && ((np >> lp) & 1u);
      if (pnot && sub == 0) {
        P.flags[ptl] = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
      if (pnot) lcnt = 0;
      skipmask |= __ballot(pnot);
    }
    if (!__any(lcnt > 0)) return;                            // nothing left to update in this tile
  }

  // ---- the ring (mia_ring64_dev.h); st holds the block this lane has staged
  int UB = 1;
  int cur = 0;                                               // the half that holds the block of the trip
  double st[4][Ring64<KT>::NC];
  const Ring64<KT> ring{Ring, P.rec, ukey, k, kp, KS, lr, h, cur, st};

  int lo = 0;
  bool single = false;                                       // a non-finite record was met: the rest of the tile goes point by point
#pragma clang loop unroll(disable)
  while (lo < nslot) {
    if (!((livemask >> lo) & 1u)) { ++lo; continue; }        // a range starts at a live slot, so it is never empty
    const bool colok = live_c && !((skipmask >> (4 * lr)) & 1ull);
    const double* Dcol = Dl + lr * DS + h;                    // + 16 t + 4 r: slot 16 t + h + 4 r of column lr
    // ---- union of the lists of slots [lo, hi): slot of the union = RANK of the observation index, found by repeated extraction of
    //      the smallest remaining key (one sweep over the keys in LDS and one DPP reduction per slot); shrink the range
    //      until the union fits
    int n = single ? 1 : 16, hi, U;
    bool act;
    for (;;) {
      hi = lo + n < nslot ? lo + n : nslot;
      act = lp >= lo && lp < hi && live_l;
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
          Dl[lp * DS + a] = wb[pos] * P.dscale;
        }
      // ---- w_mean of the points of this pass: wmean[tm][q] = w_mean[point lr][member 16 tm + 4 q + h], the B operand of
      //      the shift (0 for points that take no part).  Closed before the first matrix instruction of the pass.
      d4t wmean[KT];
#pragma unroll
      for (int tm = 0; tm < KT; ++tm) {
        d4t wm4 = {0., 0., 0., 0.};
        const int nscan = shared_w ? 1 : hi;
#pragma clang loop unroll(disable)
        for (int s = shared_w ? 0 : lo; s < nscan; ++s) {
          if (!shared_w && ((skipmask >> (4 * s)) & 1ull)) continue;
          // (lo and hi come out of the union's wave reductions: the same in every lane, but only this tells the compiler so,
          //  and with it that the map's entry and the matrix' address are scalars)
          const int su = __builtin_amdgcn_readfirstlane(s);
          const int64_t pt = shared_w ? 0 : tp[su];
          lienks_stream64_row_means<KT>(P.Win + pt * P.w_stride, k, tm, lr, h, shared_w || lr == s, wm4);
        }
        wmean[tm] = wm4;
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
          __builtin_amdgcn_sched_barrier(0);
          const d4t Tb = ring.chain(wmean);            // T = Yw w_mean: slot 4 q + h of the block in register q, column = point
          double s[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double dv = Dcol[16 * tb + 4 * q];
            s[q] = (dv * dv) * (Ring[cur * 16 * KS + (4 * q + h) * KS + k] * P.dshift + Tb[q]);
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
        P.flags[colpt] = MIA_FLAG_RETRY;                       // (colact: the slot is live, colpt is its point)
        atomicAdd(P.retry_count, 1);
      }
    }
    // (a column without observations has its W_in back already: it is not active and asks for no step)
    const int degmax = (int)tile64_wave_max_u32((colact && !decl) ? (unsigned)deg : 0u);
    const Coef64 coef{P.tab_c + (size_t)tab_idx * kTab64Deg, P.cs_phi, P.cs_psi};

#pragma clang loop unroll(disable)
    for (int c = 0; c < k; ++c) {
      // (lane roles through opaque copies, as in letkf_tile64.hip: what is invariant in this loop -- the member numbers of the
      // start vector, the 4 KT offsets of the output, their predicates -- would otherwise be hoisted and held in registers
      // across the recurrence, which has none to spare)
      int hv = h, cpv = colpt;
      asm volatile("" : "+v"(hv), "+v"(cpv));
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
      // row c of the sixteen points' weights: the lane's 64-bit base (its point) + 32-bit offset (row c, column j) < k^2 8.
      // This lane's column is one point (a dead slot: the tile's first live point, never stored to); the base of its k x k
      // block is formed here, behind the recurrence, from the point's index: ONE register lives across the recurrence, not the
      // base's two, which KT = 8 does not have (256 + 256 registers and four spills with the base formed once per range)
      char* obase = reinterpret_cast<char*>(P.W + (int64_t)cpv * kk);
      const unsigned olane = (unsigned)(c * k) * 8u + (unsigned)hv * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + hv + 4 * r;
          const double o = aphi[tj][r] + wm;
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * 8u)) = o;
        }
    }
    {
      if (!(colact && !decl)) pflag = 0;          // (columns that are not written do not report)
      const unsigned long long fb = __ballot(pflag != 0);
      const bool anyf = ((fb >> lr) & 0x0001000100010001ull) != 0ull;
      if (h == 0 && colact && !decl) P.flags[colpt] = (anyf ? MIA_FLAG_NONFINITE : 0) | (deg << 8);
    }
    lo = hi;
    __syncthreads();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr int kLienksPatch64MaxBlocks = kRing64MaxBlocks;       // union_blocks of the caller: 256 slots, at every ensemble size of the route
constexpr int kLienksPatch64MaxK = 128;

// weights_patch64_route_covers' arithmetic
bool lienks_patch64_route_covers(int k, int p_max, int64_t ng) {
  if (k < 2 || k > kLienksPatch64MaxK || p_max <= k || ng < 0) return false;            // p_max <= k: the dual routes
  if (p_max > 16 * kLienksPatch64MaxBlocks) return false;
  // a lane addresses W_out as its point's 64-bit base + a 32-bit byte offset inside that point's k x k block; map entries are int32
  if ((int64_t)k * k * 8 >= ((int64_t)1 << 31) || ng >= ((int64_t)1 << 31)) return false;
  if (ring64_lds_bytes(kLienksPatch64MaxBlocks, k) > kMaxDynamicLds) return false;   // (the largest image; holds at every k: tests/test_ienks_patch64_cover.py)
  return true;
}

// launches with the sizes of the ring frame (mia_frames64.h)
template <int KT>
static int lienks_patch64_launch_t(const LienksPatch64Params& dp, hipStream_t stream) {
  return launch_blocks(lienks_patch64_kernel<KT>, dp.n_tiles, 64, ring64_lds_bytes(dp.ub, dp.k), stream,
                       [] { note_analysis_kernel("lienks_patch64_kernel<%d>", KT); }, dp);
}

int lienks_patch64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec,
                          const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                          double epsilon, double* W_out, int32_t* flags, int32_t* retry_count, const int32_t* tile_pts,
                          int64_t n_tiles, int union_blocks, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !W_in || !W_out || !flags || !retry_count || !tile_pts) return MIA_ERR_UNSUPPORTED;
  if (w_stride != 0 && w_stride != (int64_t)k * k) return MIA_ERR_UNSUPPORTED;
  if (!lienks_patch64_route_covers(k, p_max, ng)) return MIA_ERR_UNSUPPORTED;
  if (union_blocks < 1 || union_blocks > kLienksPatch64MaxBlocks || n_tiles < 1 || !grid_covers(n_tiles)) return MIA_ERR_UNSUPPORTED;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  LienksPatch64Params dp;
  dp.k = k; dp.kp = (k + 1 + 3) & ~3;
  dp.ng = ng; dp.Win = W_in; dp.w_stride = w_stride; dp.rec = rec;
  dp.cnt = nbr_cnt; dp.idx = nbr_idx; dp.w = nbr_w; dp.p_cap = p_cap; dp.p_max = p_max;
  dp.tile_pts = tile_pts; dp.n_tiles = n_tiles;
  dp.ub = union_blocks;
  dp.transform = epsilon > 0.0 ? 0 : 1;
  dp.dscale = epsilon > 0.0 ? 1.0 / epsilon : 1.0;
  dp.dshift = epsilon > 0.0 ? epsilon : 1.0;
  // the constants of lienks_stream64_launch: reg = k - 1, f0 = 1
  const double rg = (double)(k - 1), km = (double)(k - 1);
  dp.reg = rg;
  dp.inv_reg = 1.0 / rg;
  dp.cs_phi = sqrt(km / rg);                                  // f0
  dp.cs_psi = 1.0 / rg;
  dp.W = W_out; dp.flags = flags; dp.retry_count = retry_count;
  dp.dmax = kTab64Deg - 1;
  dp.tab_hdr = tab->hdr; dp.tab_c = tab->c;
  return dispatch_upto<8>((k + 15) >> 4, [&](auto kt) { return lienks_patch64_launch_t<kt()>(dp, stream); });
}

}  // namespace mia
