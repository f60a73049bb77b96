// letkf_stream64.hip's ANALYSIS (FLOAT64, dense local networks p_max > k, ensembles up to 128 members, sixteen grid points per
// wavefront, every contraction a v_mfma_f64_16x16x4_f64, the union's records streamed through a ring of two sixteen-slot blocks)
// with letkf_patch64.hip's two changes to the FRAME, as letkf_patch64w.hip has them for the weights; mathematics,
// lane roles, summation order, the ring and its stage / chain / fold / turn discipline and the run-time loops are the ring
// family's (csrc/mia_ring64_dev.h, shared), the streamed bound, table, decline and the point-by-point mode after a non-finite
// record letkf_stream64.hip's (reference: core/etkf.py:57-103 + interface/wrapper.py:86-98 + base.py:257-278) and
// are not restated here.
//
// 1. TILE MAP.  The sixteen points of tile t are tile_pts[16 t + s], s = 0 .. 15: indices into the launch's range [0, ng),
//    -1 = empty slot.  On a row-major 2-D mesh sixteen CONSECUTIVE points are a 16 x 1 strip whose lists have a union of 200
//    observations at radius 3 against 176 of a 4 x 4 patch: the strip overflows the slot table of the launch without a map
//    (ring64_blocks(p_max): 128 slots at p_max 101) and runs in parts, the patch runs in one pass.  List row, count, flag, the
//    state column read from X and the output column written to Xa are addressed through the map; state and output as
//    letkf_patch64.hip has them (the wave-uniform base of the state row block + a 32-bit byte offset member ld 8 + point 8:
//    the host's check k ld 8 < 2^31 covers it, since every mapped column lies inside the leading dimension).  Live slots need
//    not be a prefix: a dead slot is clamped to the tile's first live point for loads and every store is predicated.  The
//    range loop runs over SLOTS, starts a range at a live slot and ends at the last live one.  A tile without a live slot
//    returns before the union; an entry outside [0, ng) is an empty slot.  Lists, flags and outputs stay in natural point
//    order, so the redo of declined points (letkf_wave_kernel<double>) needs no map.
// 2. SLOT TABLES SIZED BY THE CALLER.  `ub` sixteen-slot blocks of the sqrt(rho) table and the slot table, 1 <= ub <= 16 at
//    every ensemble size (the records are not resident); the caller has it from tile_union_census_kernel (letkf_patch64.hip).
//    A tile whose union exceeds it runs in halves of its SLOTS, quarters, ...; a single list longer than the image, p_max or
//    p_cap is MIA_FLAG_OVERFLOW and NaN output for that point, never a truncated list.
//
// A point's observations are summed in ascending index order with exact zeros in between whatever else is in the tile, so Xa
// and flags are letkf_stream64_kernel's bit for bit under any map, any ub, any shard and any number of state rows
// (tests/test_gpu_patch64s.py).
//
// The kernel keeps its own text for everything the map reaches (DESIGN 2.18 on letkf_patch64.hip: the map reaches every
// address the frame forms); what it does not reach is mia_ring64_dev.h's.
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_ring64_dev.h"
#include "mia_tile_launch.h"

namespace mia {

struct Patch64SParams {
  const double* X; int64_t ldx; int m; int k; int kp;
  int64_t g0, ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  const int32_t* tile_pts; int64_t n_tiles;                  // [n_tiles][16] point of a slot, -1 = none
  int ub;                                                    // sixteen-slot blocks of the slot table of the launch: the caller's
  double reg, inv_reg, inv_k, cs_phi, cs_psi;
  double* Xa; int64_t ldo, o0; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// KT = ceil(k / 16).  One wavefront per workgroup; its LDS bounds how many share a compute unit.
template <int KT>
__global__ __launch_bounds__(64, 1) void letkf_patch64s_kernel(Patch64SParams P) {
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
  const int colpt = live_c ? ptc : pfirst;

  // ---- the tile's neighbour lists stay in memory: lane (lp, sub) walks entries sub, sub + 4, ... of slot lp's point
  int nl = pm < P.p_cap ? pm : P.p_cap;
  nl = nl < UMAX ? nl : UMAX;
  const int64_t lrow = live_l ? ptl : pfirst;                // (lists, flags and output columns count from the shard's g0)
  const int32_t* ib = P.idx + lrow * P.p_cap;
  const double* wb = P.w + lrow * P.p_cap;
  int lcnt = P.cnt[lrow];
  unsigned long long badmask;
  {
    const bool pbad = live_l && (lcnt > pm || lcnt > P.p_cap || lcnt > UMAX);   // loud failure, never truncate
    if (pbad) {
      if (sub == 0) P.flags[ptl] = MIA_FLAG_OVERFLOW;
      const double nanv = __builtin_nan("");
      for (int it = sub; it < P.m * k; it += 4) P.Xa[(int64_t)it * P.ldo + P.o0 + ptl] = nanv;
    }
    if (!live_l || pbad) lcnt = 0;
    badmask = __ballot(pbad);
  }

  // a state row of the tile: member (tm, q) of lane group h = 16 tm + 4 q + h, the column of slot lr's point (clamped to an
  // existing member) (wave-uniform base + 32-bit lane offset in bytes: k ld 8 < 2^31 is checked on the host, g0 + column < ld)
  const unsigned ldxb = (unsigned)P.ldx * 8u, ldob = (unsigned)P.ldo * 8u;
  auto load_x = [&](int mi, int hh, int col, double (&xr)[KT][4]) {
    const char* xbase = reinterpret_cast<const char*>(P.X + (int64_t)mi * k * P.ldx + P.g0);
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
    const bool colok = live_c && !((badmask >> (4 * lr)) & 1ull);
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
          Dl[lp * DS + a] = wb[pos];
        }
      // ---- block 0 into the ring
      double fin = 0.0;
      ring.stage(0);
      ring.commit(cur, fin);
      __syncthreads();
      // ---- rhs_g = Yw^T (rho_g o d), once per range (d = column k of the records); this first pass over the union also
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
        P.flags[colpt] = MIA_FLAG_RETRY;                                            // (an active column is live: colpt is its point)
        atomicAdd(P.retry_count, 1);
      }
    }
    const int degmax = (int)tile64_wave_max_u32((colact && !decl) ? (unsigned)deg : 0u);
    const Coef64 coef{P.tab_c + (size_t)tab_idx * kTab64Deg, P.cs_phi, P.cs_psi};

    for (int mi = 0; mi < P.m; ++mi) {
      // (lane roles through opaque copies, as in letkf_tile64.hip: what is invariant in this loop -- the 4 KT offsets of a
      // state row, those of the output, their predicates -- would otherwise be hoisted and held in registers across the
      // recurrence, which has none to spare)
      int hv = h, cv = colpt;
      asm volatile("" : "+v"(hv), "+v"(cv));
      d4t va[KT], vb[KT], aphi[KT], apsi[KT];
      double xm;
      {
        double xb[KT][4];
        load_x(mi, hv, cv, xb);
        double xs = 0.0;
#pragma unroll
        for (int tm = 0; tm < KT; ++tm)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + hv < k);
            xb[tm][q] = live ? xb[tm][q] : 0.0;
            xs += xb[tm][q];
          }
        xm = tile64_add_h(xs) * P.inv_k;
        // ---- the recurrence on the 16 columns at once: v_0 = x', v_1 = alpha C v_0 - v_0, v_{j+1} = 2 (alpha C v_j - v_j) - v_{j-1}
#pragma unroll
        for (int tm = 0; tm < KT; ++tm)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + hv < k);
            va[tm][q] = live ? xb[tm][q] - xm : 0.0;
          }
      }
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
      // ---- x' w_mean = (psi(C) x') . rhs / reg: members in the lane's registers first, then the four lane groups
      double zs = 0.0;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) zs = fma(apsi[tm][r], Rl[(4 * tm + r) * 64 + lane], zs);
      const double mterm = xm + tile64_add_h(zs);
      char* obase = reinterpret_cast<char*>(P.Xa + (int64_t)mi * k * P.ldo + P.o0);
      const unsigned olane = (unsigned)hv * ldob + (unsigned)cv * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + hv + 4 * r;
          const double o = aphi[tj][r] + mterm;
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * ldob)) = o;
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
constexpr int kPatch64SMaxBlocks = kRing64MaxBlocks;            // union_blocks of the caller: 256 slots, at every ensemble size of the route

// launches with the sizes of the ring frame (mia_frames64.h)
template <int KT>
static int patch64s_launch_t(const Patch64SParams& dp, hipStream_t stream) {
  return launch_blocks(letkf_patch64s_kernel<KT>, dp.n_tiles, 64, ring64_lds_bytes(dp.ub, dp.k), stream,
                       [] { note_analysis_kernel("letkf_patch64s_kernel<%d>", KT); }, dp);
}

int patch64s_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                             const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                             double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                             const int32_t* tile_pts, int64_t n_tiles, int union_blocks, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!stream64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  if (ng >= ((int64_t)1 << 31) || !grid_covers(n_tiles)) return MIA_ERR_UNSUPPORTED;   // (map entries are int32)
  if (union_blocks < 1 || union_blocks > kPatch64SMaxBlocks || n_tiles < 1) return MIA_ERR_SIZE;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Patch64SParams dp;
  dp.X = X; dp.ldx = ldx; dp.m = m; dp.k = k; dp.kp = (k + 1 + 3) & ~3;
  dp.g0 = g0; dp.ng = ng; dp.rec = rec;
  dp.cnt = nbr_cnt; dp.idx = nbr_idx; dp.w = nbr_w; dp.p_cap = p_cap; dp.p_max = p_max;
  dp.tile_pts = tile_pts; dp.n_tiles = n_tiles;
  dp.ub = union_blocks;
  const double rg = (double)(k - 1) / inf_factor, km = (double)(k - 1);
  dp.reg = rg;
  dp.inv_reg = 1.0 / rg;
  dp.inv_k = 1.0 / (double)k;
  dp.cs_phi = sqrt(km / rg);                                  // f0
  dp.cs_psi = 1.0 / rg;
  dp.Xa = Xa; dp.ldo = ldo; dp.o0 = o0; dp.flags = flags; dp.retry_count = retry_count;
  dp.dmax = kTab64Deg - 1;
  dp.tab_hdr = tab->hdr; dp.tab_c = tab->c;
  return dispatch_upto<8>((k + 15) >> 4, [&](auto kt) { return patch64s_launch_t<kt()>(dp, stream); });
}

}  // namespace mia
