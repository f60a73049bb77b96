// letkf_dense64.hip's analysis (FLOAT64, dense local networks p_max > k, sixteen grid points per wavefront, every contraction
// a v_mfma_f64_16x16x4_f64) with two changes to its FRAME; mathematics, lane roles, summation order, table,
// decline and the run-time loops are that file's (reference: core/etkf.py:57-103 + interface/wrapper.py:86-98 +
// base.py:257-278) and are not restated here.
//
// 1. TILE MAP.  The sixteen points of tile t are tile_pts[16 t + s], s = 0 .. 15: indices into the launch's range [0, ng),
//    -1 = empty slot.  On a row-major 2-D mesh sixteen CONSECUTIVE points are a 16 x 1 strip whose lists have a union of
//    175 - 250 observations at radius 3; a 4 x 4 patch has 116 - 184 and fits one record image.  Lists, counts, flags, state
//    columns and output columns are addressed through the map (a per-lane 32-bit byte offset from a wave-uniform base: the
//    host's check k ld 8 < 2^31 covers it, since every mapped column lies inside the leading dimension).  Live slots need not
//    be a prefix: a dead slot is clamped to the tile's first live point for loads and every store is predicated.  A tile
//    without a live slot returns before the union.  Lists and flags stay in natural point order, so the redo of declined points
//    (letkf_wave_kernel<double>) needs no map.
// 2. IMAGE SIZED BY THE CALLER.  `ub` sixteen-slot blocks, 1 <= ub <= the capacity at this ensemble size; the caller has it from
//    tile_union_census_kernel below (largest union of a tile).  A tile whose union exceeds the image runs in halves of its
//    SLOTS (the first eight slots of a 4 x 4 patch are a 2 x 4 patch), quarters, ...; a single list longer than the image,
//    p_max or p_cap is MIA_FLAG_OVERFLOW and NaN output, never a truncated list.
//
// A point's observations are summed in ascending index order with exact zeros in between whatever else is in the tile, so the
// output is letkf_dense64_kernel's bit for bit under any map (tests/test_gpu_patch64.py).
//
// The kernel is a copy of letkf_dense64_kernel with the frame changed, not a shared body: the map reaches every address the
// frame forms (lists, flags, loads, stores, the range loop), so a shared body would be parametrised in each of them and the
// dense route's code generation -- registers, the placement of loads beside matrix instructions -- would have to be
// re-verified; the project's precedent is the same (letkf_stream64.hip, lketkf_kern64.hip).
#include "mia_cheb_table64.h"
#include "mia_frames64.h"
#include "mia_tile_launch.h"
#include "mia_kernels.h"

namespace mia {

struct Patch64Params {
  const double* X; int64_t ldx; int m; int k; int kp;
  int64_t g0, ng;
  const double* rec;
  const int32_t* cnt; const int32_t* idx; const double* w; int p_cap; int p_max;
  const int32_t* tile_pts; int64_t n_tiles;                  // [n_tiles][16] point of a slot, -1 = none
  int ub;                                                    // sixteen-slot blocks of the record image in LDS
  double reg, inv_reg, inv_k, cs_phi, cs_psi;
  double* Xa; int64_t ldo, o0; int32_t* flags; int32_t* retry_count;
  int dmax;
  const Tab64Hdr* tab_hdr; const double2* tab_c;
};

// KT = ceil(k / 16).  One wavefront per workgroup; the LDS image bounds how many share a compute unit.
template <int KT>
__global__ __launch_bounds__(64, 1) void letkf_patch64_kernel(Patch64Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int k = P.k, kp = P.kp, pm = P.p_max;
  const int UMAX = 16 * P.ub, DS = UMAX + 1;
  const int KS = kp | 1;                                     // odd row pitch (in doubles) of the record image
  double* Yw = reinterpret_cast<double*>(smem_raw);          // [UMAX][KS] union records, zero rows beyond the union
  double* Dl = Yw + UMAX * KS;                               // [16][DS]   sqrt(rho) of (slot of the tile, slot of the union), 0 = not local
  int* ukey = reinterpret_cast<int*>(Dl + 16 * DS);          // [UMAX]     observation index of a slot, ascending
  unsigned* Kl = reinterpret_cast<unsigned*>(Dl);            // [16][nl]   index + 1 of the lists' entries while the union is formed

  // XCD-aware block -> tile map: blocks b, b + 8, ... share an XCD (and its L2) and take consecutive tiles, whose
  // records overlap (consecutive tiles of a patch row)
  const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t ntile = P.n_tiles;
  if (bid >= ntile) return;
  const int64_t q8 = ntile >> 3, r8 = ntile & 7, xcd = bid & 7;
  const int64_t tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int lr = lane & 15, h = lane >> 4, lp = lane >> 2, sub = lane & 3;

  // ---- the tile's points: slot lr is this lane's column, slot lp the list it walks.  An entry outside [0, ng) is an empty
  //      slot (the census has refused such a map already; nothing is ever indexed by one)
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

  // a state row of the tile: member (tm, q) of lane group h = 16 tm + 4 q + h, the column of slot lr (clamped to an existing
  // member) (wave-uniform base + 32-bit lane offset in bytes: k ld 8 < 2^31 is checked on the host, g0 + column < ld)
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

  int lo = 0;
  bool single = false;                                       // a non-finite record was met: the rest of the tile goes point by point
#pragma clang loop unroll(disable)
  while (lo < nslot) {
    if (!((livemask >> lo) & 1u)) { ++lo; continue; }        // a range starts at a live slot, so it is never empty
    const bool colok = live_c && !((badmask >> (4 * lr)) & 1ull);
    // ---- union of the lists of slots [lo, hi): slot of the union = RANK of the observation index, found by repeated
    //      extraction of the smallest remaining key (one sweep over the keys in LDS and one DPP reduction per slot); shrink
    //      the range until the union fits
    int n = single ? 1 : 16, hi, U, UB;
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
      UB = UB < 1 ? 1 : UB;                                      // blocks in use; rows up to 16 UB are written
      // ---- the union's records, four rows per trip: lane group h takes row r0 + h, its sixteen lanes the columns
      double fin = 0.0;       // stays 0 while every value is finite (inf * 0 = NaN)
#pragma clang loop unroll_count(2)
      for (int r0 = 0; r0 < 16 * UB; r0 += 4) {
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
      // A non-finite record would reach EVERY column of the tile through the shared products (NaN * 0 = NaN), also the
      // points that do not see that observation.  Such a tile is analysed point by point: the union is then the point's
      // own list and the damage stays where the reference has it.
      if (__any(fin != fin) && hi - lo > 1) { __syncthreads(); n = 1; single = true; continue; }
      break;
    }
    // ---- sqrt(rho) of (slot of the tile, slot of the union): the slot of an entry is the place of its index in the sorted table
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
    __syncthreads();
    const bool colact = colok && lr >= lo && lr < hi;
    const double* Dcol = Dl + lr * DS + h;                    // + 16 t + 4 r: slot 16 t + h + 4 r of column lr
    // A operands.  First product / Gram: record row 16 tb + lr, member 16 tm + 4 q + h; second product: record row
    // 16 tb + 4 q + h, member 16 tj + lr.  Innovation and pad columns are not members (only the last block is ragged).
    auto a_in = [&](int tb, int tm, int q) -> double {
      const int mem = 16 * tm + 4 * q + h;
      const bool ok = tm < KT - 1 || mem < k;
      const double v = Yw[(16 * tb + lr) * KS + (ok ? mem : 0)];
      return ok ? v : 0.0;
    };
    auto a_out = [&](int tb, int q, int tj) -> double {
      const int mem = 16 * tj + lr;
      const bool ok = tj < KT - 1 || mem < k;
      const double v = Yw[(16 * tb + 4 * q + h) * KS + (ok ? mem : 0)];
      return ok ? v : 0.0;
    };
    // ---- Gershgorin bound of every point, streamed: L_g = max_a w_a sum_b |G_ab| w_b.  Row block t: every Gram block
    //      (tk, t) is formed (4 KT instructions), folded into the row sums (4) and dropped
    double L = 0.0;
    {
      int t = 0;
#pragma clang loop unroll(disable)
      do {
        d4t R = {0., 0., 0., 0.};
        int tk = 0;
#pragma clang loop unroll(disable)
        do {
          d4t Gb = {0., 0., 0., 0.};
#pragma unroll
          for (int tm = 0; tm < KT; ++tm)
#pragma unroll
            for (int q = 0; q < 4; ++q) Gb = MIA_MFMA64(a_in(tk, tm, q), a_in(t, tm, q), Gb);
          double dk[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) dk[q] = Dcol[16 * tk + 4 * q];
#pragma unroll
          for (int q = 0; q < 4; ++q) R = MIA_MFMA64(fabs(Gb[q]), dk[q], R);
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
        P.flags[ptc] = MIA_FLAG_RETRY;
        atomicAdd(P.retry_count, 1);
      }
    }
    const int degmax = (int)tile64_wave_max_u32((colact && !decl) ? (unsigned)deg : 0u);
    const double2* ctab = P.tab_c + (size_t)tab_idx * kTab64Deg;
    auto coef = [&](int j) -> double2 {                              // (zero beyond a point's own degree)
      const double2 c = ctab[j < kTab64Deg ? j : kTab64Deg - 1];
      return double2{c.x * P.cs_phi, c.y * P.cs_psi};
    };
    // y += Yw^T (s o .) over one block: the second product's steps (tb, q), B = the scaled block
    auto fold = [&](int tb, const double (&s)[4], d4t (&y)[KT]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int tj = 0; tj < KT; ++tj) y[tj] = MIA_MFMA64(a_out(tb, q, tj), s[q], y[tj]);
    };
    // ---- rhs_g = Yw^T (rho_g o d), once per range (d = column k of the records)
    d4t rhs[KT];
#pragma unroll
    for (int tj = 0; tj < KT; ++tj) rhs[tj] = d4t{0., 0., 0., 0.};
    {
      int tb = 0;
#pragma clang loop unroll(disable)
      do {
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dv = Dcol[16 * tb + 4 * q];
          s[q] = dv * dv * Yw[(16 * tb + 4 * q + h) * KS + k];
        }
        fold(tb, s, rhs);
      } while (++tb < UB);
    }

    for (int mi = 0; mi < P.m; ++mi) {
      double xb[KT][4];
      load_x(mi, h, colpt, xb);
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
      // ---- the recurrence on the 16 columns at once: v_0 = x', v_{j+1} = 2 (alpha C v_j - v_j) - v_{j-1}
      d4t va[KT], vb[KT], aphi[KT], apsi[KT], y[KT];
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool live = colact && (tm < KT - 1 || 16 * tm + 4 * q + h < k);
          va[tm][q] = live ? xb[tm][q] - xm : 0.0;
        }
      // y = C u = Yw^T (rho o (Yw u)), one sixteen-slot block of the union per trip
      auto product = [&](const d4t (&u)[KT]) {
#pragma unroll
        for (int tj = 0; tj < KT; ++tj) y[tj] = d4t{0., 0., 0., 0.};
        int tb = 0;
#pragma clang loop unroll(disable)
        do {
          d4t Tb = {0., 0., 0., 0.};
#pragma unroll
          for (int tm = 0; tm < KT; ++tm)
#pragma unroll
            for (int q = 0; q < 4; ++q) Tb = MIA_MFMA64(a_in(tb, tm, q), u[tm][q], Tb);
          double s[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double dv = Dcol[16 * tb + 4 * q];
            s[q] = (dv * dv) * Tb[q];
          }
          fold(tb, s, y);
        } while (++tb < UB);
      };
      // vnew = 2 (alpha y - vcur) - vold, written over vold; the two functions accumulate c_j vnew
      auto advance = [&](d4t (&vold)[KT], const d4t (&vcur)[KT], const double2 cj) {
        product(vcur);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          vold[t] = 2.0 * (alpha * y[t] - vcur[t]) - vold[t];
          aphi[t] = cj.x * vold[t] + aphi[t];
          apsi[t] = cj.y * vold[t] + apsi[t];
        }
      };
      {
        const double2 c0 = coef(0), c1 = coef(1);
        product(va);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
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
      // ---- x' w_mean = (psi(C) x') . rhs / reg: members in the lane's registers first, then the four lane groups
      double zs = 0.0;
#pragma unroll
      for (int tm = 0; tm < KT; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) zs = fma(apsi[tm][r], rhs[tm][r], zs);
      const double mterm = xm + tile64_add_h(zs);
      char* obase = reinterpret_cast<char*>(P.Xa + (int64_t)mi * k * P.ldo + P.o0);
      const unsigned olane = (unsigned)h * ldob + (unsigned)colpt * 8u;
      const bool wr = colact && !decl;
#pragma unroll
      for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mem = 16 * tj + h + 4 * r;
          const double o = aphi[tj][r] + mterm;
          if (!(fabs(o) <= 1e300) && mem < k) pflag |= MIA_FLAG_NONFINITE;
          if (wr && mem < k) *reinterpret_cast<double*>(obase + (olane + (unsigned)(16 * tj + 4 * r) * ldob)) = o;
        }
    }
    {
      if (!(colact && !decl)) pflag = 0;          // (columns that are not written do not report)
      const unsigned long long fb = __ballot(pflag != 0);
      const bool anyf = ((fb >> lr) & 0x0001000100010001ull) != 0ull;
      if (h == 0 && colact && !decl) P.flags[ptc] = (anyf ? MIA_FLAG_NONFINITE : 0) | (deg << 8);
    }
    lo = hi;
    __syncthreads();
  }
}

// ---- the census of a tile map: validation and the largest union -------------------------------------------------------------
// One wavefront per tile.  (1) Every entry must lie in [-1, ng) and every point of [0, ng) must occur exactly once: a counter
// per point (seen[pt], zeroed by the entry) finds an entry met twice, the sum of live entries a point that is missing (no
// entry out of range, none twice and ng of them: every point once); the last tile to finish compares the sum.  Nothing is
// indexed by an entry out of range.  (2) The distinct observation indices of the tile's lists, counted through a hash set in
// LDS (at most 16 x 256 list entries are looked at -- a longer list is the analysis kernel's overflow, whatever the image --
// in 8192 places, so a free place always exists), folded into out[1] by atomicMax.
constexpr int kCensusHash = 8192;
constexpr int kCensusMaxList = 256;

__global__ __launch_bounds__(64) void tile_union_census_kernel(const int32_t* tile_pts, int64_t n_tiles, int64_t ng,
                                                               const int32_t* cnt, const int32_t* idx, int p_cap, int p_max,
                                                               int count_unions, int32_t* seen /* [ng] + live sum + tiles done */,
                                                               int32_t* out /* [0] error bits, [1] largest union */) {
  __shared__ unsigned tab[kCensusHash];
  __shared__ int ndistinct;
  const int lane = threadIdx.x, lp = lane >> 2, sub = lane & 3;
  const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (tile >= n_tiles) return;
  const int pt = tile_pts[tile * 16 + lp];
  const bool inrange = pt >= -1 && pt < ng;
  const bool live = inrange && pt >= 0;
  int err = inrange ? 0 : MIA_TILEMAP_RANGE;
  if (live && sub == 0 && atomicAdd(&seen[pt], 1) != 0) err |= MIA_TILEMAP_TWICE;
  if (count_unions) {
    for (int i = lane; i < kCensusHash; i += 64) tab[i] = 0u;
    if (lane == 0) ndistinct = 0;
    __syncthreads();
    if (live) {
      int nl = p_max < p_cap ? p_max : p_cap;
      nl = nl < kCensusMaxList ? nl : kCensusMaxList;
      int lcnt = cnt[pt];
      lcnt = lcnt < nl ? lcnt : nl;
      const int32_t* ib = idx + (int64_t)pt * p_cap;
      for (int pos = sub; pos < lcnt; pos += 4) {
        const int e = ib[pos];
        if (e < 0) continue;
        const unsigned key1 = (unsigned)e + 1u;
        unsigned hpos = (key1 * 2654435761u) >> 19;              // 13 bits
        for (;;) {
          const unsigned old = atomicCAS(&tab[hpos], 0u, key1);
          if (old == 0u) { atomicAdd(&ndistinct, 1); break; }
          if (old == key1) break;
          hpos = (hpos + 1u) & (unsigned)(kCensusHash - 1);
        }
      }
    }
    __syncthreads();
    if (lane == 0) atomicMax(&out[1], ndistinct);
  }
  const unsigned long long lv = __ballot(live && sub == 0);
  const bool anyerr = __any(err != 0);
  if (anyerr && err != 0) atomicOr(&out[0], err);
  if (lane == 0) {
    atomicAdd(&seen[ng], __popcll(lv));
    __threadfence();
    if (atomicAdd(&seen[ng + 1], 1) == (int)(n_tiles - 1)) {     // the last tile: have all ng points been met?
      __threadfence();
      if ((int64_t)atomicAdd(&seen[ng], 0) != ng) atomicOr(&out[0], MIA_TILEMAP_MISSING);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// launches with the sizes of the resident image (mia_frames64.h), as letkf_dense64.hip: the same bytes, the same capacity; the
// caller chooses the blocks
template <int KT>
static int patch64_launch_t(const Patch64Params& dp, hipStream_t stream) {
  return launch_blocks(letkf_patch64_kernel<KT>, dp.n_tiles, 64, resident64_lds_bytes(dp.ub, dp.kp), stream,
                       [] { note_analysis_kernel("letkf_patch64_kernel<%d>", KT); }, dp);
}

int patch64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                            const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                            double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                            const int32_t* tile_pts, int64_t n_tiles, int union_blocks, hipStream_t stream) {
  if (!option(MIA_OPT_TILE) || !flags || !retry_count) return MIA_ERR_UNSUPPORTED;
  if (!dense64_route_covers(m, k, p_max, ldx, ldo, ng)) return MIA_ERR_UNSUPPORTED;
  if (ng >= ((int64_t)1 << 31) || !grid_covers(n_tiles)) return MIA_ERR_UNSUPPORTED;   // (map entries are int32)
  if (union_blocks < 1 || union_blocks > resident64_capacity_blocks(k) || n_tiles < 1) return MIA_ERR_SIZE;
  const CoefTable64* tab = cheb_coef_table64(stream, kTab64Primal);
  if (!tab) return MIA_ERR_UNSUPPORTED;
  Patch64Params dp;
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
  return dispatch_upto<4>((k + 15) >> 4, [&](auto kt) { return patch64_launch_t<kt()>(dp, stream); });
}

int tile_union_census_launch(const int32_t* tile_pts, int64_t n_tiles, int64_t ng, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                             int p_cap, int p_max, int count_unions, int32_t* out2, int32_t* ws, hipStream_t stream) {
  dim3 grid;
  if (ng >= ((int64_t)1 << 31) - 2 || n_tiles >= ((int64_t)1 << 31) || !launch_grid(n_tiles, &grid)) return MIA_ERR_UNSUPPORTED;
  MIA_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)(ng + 2) * sizeof(int32_t), stream));
  MIA_HIP_TRY(hipMemsetAsync(out2, 0, 2 * sizeof(int32_t), stream));
  tile_union_census_kernel<<<grid, dim3(64), 0, stream>>>(tile_pts, n_tiles, ng, nbr_cnt, nbr_idx, p_cap, p_max, count_unions, ws,
                                                          out2);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

}  // namespace mia
