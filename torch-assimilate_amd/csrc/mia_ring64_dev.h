// The device frame of the streamed ("ring") float64 tile kernels for DENSE local networks (p_max > k) of ensembles up to 128
// members: letkf_stream64.hip (analysis), letkf_stream64w.hip (weights, 2.19), lienks_stream64.hip (IEnKS update,
// 2.20), letkf_patch64w.hip (weights under a tile map, 2.22), lienks_patch64.hip (IEnKS update under a tile map, 2.23) and letkf_patch64s.hip (analysis under a tile map, 2.24).  Each of them keeps its __global__ kernel, its head (lists,
// overflow, map, prior scan), the passes over the union written out in its body, the start vector of a pass and its stores;
// what they share stands here once: the block -> tile map, the ring, the table's coefficient pair and the two
// steps of the recurrence.
//
// Sixteen grid points per wavefront, every contraction on the matrix cores (v_mfma_f64_16x16x4_f64).  With C_g = Yw^T diag(rho_g)
// Yw (k x k, what the reference decomposes) the kernels need phi(C_g) u and psi(C_g) u from ONE Chebyshev recurrence on u.
// C_g is never formed:
//
//     C_g u = Yw^T (rho_g o (Yw u))          T = Yw . U   (16 slots x k)(k x 16 points),   y += Yw^T . (rho o T)
//
// two thin products per sixteen-slot block whose left factors belong to the tile and whose sixteen columns are the sixteen
// points; both read their A operands from the staged block, which is therefore fetched once per trip and read twice.  The
// recurrence keeps FOUR k-vectors, not letkf_dense64.hip's five: the accumulator of the second product starts at the step's
// other terms, -2 v_j - v_{j-1}, and the column's 2 alpha rides on rho o T, so that the chain leaves v_{j+1} in place.  The
// spectral bound is the dual route's: L_g = max_a w_a sum_b |G_ab| w_b; row block t is held as operands in registers (read
// straight from memory, once per t) while the blocks tk stream through the ring.
//
// Lane roles follow v_mfma_f64_16x16x4_f64 as in letkf_tile64.hip: lane (lr, h) = (lane & 15, lane >> 4) supplies A[lr][h]
// and B[h][lr]; of a result block it holds column lr (= grid point lr), rows h + 4 r in register r.  A k-vector of the
// sixteen points is KT result blocks (member 16 tm + h + 4 r in register r): register q of block tm IS the B operand of
// step (tm, q) of the first product, the scaled block of T the B operand of steps (tb, q) of the second.
//
// Summation order is canonical: slot = RANK of the observation index inside the union, blocks and steps ascend, every sum
// over the union is ONE chain of matrix instructions through its accumulator (never partial sums per block), so a point's
// own observations are summed in ascending index order with exact zeros in between, whatever else is in the tile.
//
// The ring.  Every pass over the union (rhs, the rows of the bound, every product of the recurrence) finds block 0 in the
// ring's current half and leaves it there: trip tb asks memory for block tb + 1 (block 0 in the last trip) at its top,
// multiplies block tb out of the current half, writes the staged registers to the other half, passes the barrier and swaps
// the halves.  A lane stages rows 4 j + h, columns lr + 16 i: one base address per row, the columns are immediate offsets.
// A slot beyond the union has key -1: it is never turned into an address, its row is written as zeros.
//
// The loops over union blocks are run-time loops.  What they rely on: builtins only; every such loop is a
// do-while that runs at least once, so that it is left on the fall-through side of its closing branch; an accumulator that
// lives across the back edge is touched by matrix instructions only until the loop has been left; a block of T (or of the
// Gram matrix) is fresh in every trip and its vector read is followed by the trip's remaining matrix instructions.  The
// ring's loads stand at the top of a trip, before its first matrix instruction; its LDS writes and barrier behind the last.
//
// The form.  Every struct here holds REFERENCES to the kernel's own locals and is aggregate-initialised once those are
// declared, and its members are plain __device__ functions, not __forceinline__ ones: exactly what the [&] closures were that
// each kernel used to spell out, so the four code objects are those closures' byte for byte (HISTORY.md).  Held by value the
// same members build a different, longer code object; forced inline, the kernels of 17 .. 32 members come out differently.
// What a kernel has INLINE in its body (the union, the rhs pass, the bound, the degree lookup, the series) stays there for
// the same reason: made a function, a block is optimised on its own before it is inlined, and every instantiation changes.
#pragma once
#include "mia_cheb_table64.h"

namespace mia {

// XCD-aware block -> tile map: blocks b, b + 8, ... share an XCD (and its L2) and take consecutive tiles, whose records overlap
__device__ __forceinline__ int64_t ring64_tile_of_block(int64_t bid, int64_t ntile) {
  const int64_t q8 = ntile >> 3, r8 = ntile & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// ---- the ring of two sixteen-slot blocks of union records in LDS
template <int KT>
struct Ring64 {
  static constexpr int NC = KT + 1;                          // column trips of a staged row: kp <= 16 KT + 4
  double* const& Ring; const double* const& rec; int* const& ukey;
  const int& k; const int& kp; const int& KS; const int& lr; const int& h;
  int& cur;                                                  // the half that holds the block of the trip
  double (&st)[4][NC];

  // stage() asks memory for block tb of the union (rows 4 j + h, columns lr + 16 i of this lane), commit() writes the staged
  // registers to one half.  Rows beyond the union (key -1) are zeros and touch no memory
  __device__ void stage(int tb) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = ukey[16 * tb + 4 * j + h];
      const double* src = rec + ((int64_t)(key < 0 ? 0 : key) * kp + lr);
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        double v = 0.0;
        if (key >= 0 && (i < KT - 1 || lr + 16 * i < kp)) v = src[16 * i];
        st[j][i] = v;
      }
    }
  }
  __device__ void commit(int half, double& fin) const {   // fin stays 0 while every value is finite (inf * 0 = NaN)
    double* dst = Ring + half * 16 * KS + h * KS + lr;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        fin = fma(st[j][i], 0.0, fin);
        if (i < KT - 1 || lr + 16 * i < kp) dst[4 * j * KS + 16 * i] = st[j][i];
      }
  }
  // A operands out of the current half.  First product / Gram: record row lr of the block, member 16 tm + 4 q + h; second
  // product: record row 4 q + h, member 16 tj + lr.  Innovation and pad columns are not members (only the last block is ragged).
  __device__ double a_in(int tm, int q) const {
    const int mem = 16 * tm + 4 * q + h;
    const bool ok = tm < KT - 1 || mem < k;
    const double v = Ring[cur * 16 * KS + lr * KS + (ok ? mem : 0)];
    return ok ? v : 0.0;
  }
  __device__ double a_out(int q, int tj) const {
    const int mem = 16 * tj + lr;
    const bool ok = tj < KT - 1 || mem < k;
    const double v = Ring[cur * 16 * KS + (4 * q + h) * KS + (ok ? mem : 0)];
    return ok ? v : 0.0;
  }
  // The A operands of four matrix instructions are read from LDS while the four before them run, and the scheduler is
  // held to that order: left alone it reads a trip's 8 KT operands ahead of its first instruction, which the 40 KT
  // registers of the recurrence vectors and the staged block leave no room for above 80 members.
  // T (or Gram) block of the trip: steps (tm, q) ascending through ONE accumulator; b[tm][q] = the B operands
  template <class B>
  __device__ d4t chain(const B& b) const {
    d4t acc = {0., 0., 0., 0.};
    double an[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) an[q] = a_in(0, q);
#pragma unroll
    for (int tm = 0; tm < KT; ++tm) {
      double ac[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) ac[q] = an[q];
      if (tm + 1 < KT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) an[q] = a_in(tm + 1, q);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = MIA_MFMA64(ac[q], b[tm][q], acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
  }
  // y += Yw^T (s o .) over the block of the trip: the second product's steps (tb, q), B = the scaled block; step
  // e = KT q + tj, four steps per group
  __device__ void fold(const double (&s)[4], d4t (&y)[KT]) const {
    double an[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) an[i] = a_out(i / KT, i % KT);
#pragma unroll
    for (int g = 0; g < KT; ++g) {
      double ac[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ac[i] = an[i];
      if (g + 1 < KT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) an[i] = a_out((4 * g + 4 + i) / KT, (4 * g + 4 + i) % KT);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) y[(4 * g + i) % KT] = MIA_MFMA64(ac[i], s[(4 * g + i) / KT], y[(4 * g + i) % KT]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the end of a trip: the staged block into the other half, which becomes the current one
  __device__ void turn(double& fin) const {
    commit(cur ^ 1, fin);
    __syncthreads();
    cur ^= 1;
  }
};

// the table row's coefficient pair j, scaled (zero beyond a point's own degree)
struct Coef64 {
  const double2* ctab; const double& cs_phi; const double& cs_psi;
  __device__ double2 operator()(int j) const {
    const double2 c = ctab[j < kTab64Deg ? j : kTab64Deg - 1];
    return double2{c.x * cs_phi, c.y * cs_psi};
  }
};

// ---- the recurrence on the 16 columns at once: v_0 = the pass' start vector, v_1 = alpha C v_0 - v_0,
//      v_{j+1} = 2 (alpha C v_j - v_j) - v_{j-1}; aphi = sum_j c_j.x v_j and apsi = sum_j c_j.y v_j
template <int KT>
struct Recur64 {
  const Ring64<KT>& ring; const double* const& Dcol; const int& UB; double& nofin;
  const double& alpha; d4t (&aphi)[KT]; d4t (&apsi)[KT];

  // acc += sc C u = Yw^T (sc rho o (Yw u)), one sixteen-slot block of the union per trip; sc = alpha or 2 alpha of the
  // column.  The caller has put the recurrence's other terms into acc: the step needs no vector of its own for C u,
  // which at 128 members is the 64 registers that decide between spilling and not
  __device__ void product(const d4t (&u)[KT], d4t (&acc)[KT], const double sc) const {
    int tb = 0;
#pragma clang loop unroll(disable)
    do {
      ring.stage(tb + 1 < UB ? tb + 1 : 0);
      __builtin_amdgcn_sched_barrier(0);
      const d4t Tb = ring.chain(u);
      double s[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double dv = Dcol[16 * tb + 4 * q];
        s[q] = (sc * (dv * dv)) * Tb[q];
      }
      ring.fold(s, acc);
      ring.turn(nofin);
    } while (++tb < UB);
  }
  // vnew = 2 alpha C vcur - 2 vcur - vold, accumulated over vold; the two functions accumulate c_j vnew
  __device__ void advance(d4t (&vold)[KT], const d4t (&vcur)[KT], const double2 cj) const {
#pragma unroll
    for (int t = 0; t < KT; ++t) vold[t] = -2.0 * vcur[t] - vold[t];
    product(vcur, vold, 2.0 * alpha);
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      aphi[t] = cj.x * vold[t] + aphi[t];
      apsi[t] = cj.y * vold[t] + apsi[t];
    }
  }
};

}  // namespace mia
