// The ensemble transform in FLOAT64 on tiles of sixteen grid points, every product a v_mfma_f64_16x16x4_f64: _apply_weights
// (pytassim/interface/base.py:257-278) in the default working precision of the drop-in classes, with per-grid-point weights
// (dims (grid, ensemble, ensemble_new): update_state after estimate_weights, the weight-file flow, every iteration of the
// localised IEnKS) and with one weight matrix for all points (the global ETKF / KETKF):
//     xa[v][j][g] = mean_vg + sum_i (x[v][i][g] - mean_vg) W[g][i][j]          mean_vg = (1 / k) sum_i x[v][i][g]
// The float32 twins are apply_local.hip; the frame is theirs.  The one-point-per-wavefront kernel of ienks.hip
// and the one-point-per-thread kernel of etkf_global.hip stay as the fallback outside the cover below and as the baseline.
//
// apply_local64_tile_kernel<KT> (KT = ceil(k / 16) <= 8, 2 <= k <= 128, any m >= 1): a workgroup of four wavefronts owns a tile
// of sixteen consecutive points.
//   * The tile's state rows arrive EIGHT rows at a time as whole 128-byte segments (row v, member i, the sixteen points) in an
//     LDS image [row][member][point]; wavefront w transforms points 4 w .. 4 w + 3 as xa_g^T (k x rows) = W_g^T x_g'^T:
//     the A operand is W_g read straight from memory (lane (lr, h) supplies A[lr][h] = W_g[4 ks + h][16 jb + lr]: 128-byte
//     runs of a row of W), one block row of sixteen new members held and the next requested ahead; the B operand is the
//     point's column of the image with the row mean removed in registers (lane (lr, h): B[h][lr] = x'[row lr][member
//     4 ks + h]); the result block (rows h + 4 r in register r, column = state row lr) goes back into column g of the image
//     in place -- the column belongs to this wavefront alone and its B fragments are in registers by then -- and the image
//     leaves as whole segments.
//   * ROWS PER PASS: eight.  Sixteen rows of doubles are 2048 kp + 128 bytes: 82 KB at k = 40 (one workgroup = four
//     wavefronts per CU, where the kernel waits on memory) and more than a workgroup may ask for above k = 76.  Eight rows are
//     1024 kp + 64 bytes: 41 024 at k = 40 (three workgroups per CU, the float32 kernel's footprint), 131 136 at k = 128, so
//     ONE frame serves every 2 <= k <= 128.  The price: columns 8..15 of every matrix instruction carry zeros (the products
//     are a tenth of the memory time: 2 m k^2 flops per point against 8 k^2 + 16 k m bytes), and W_g is read once per eight
//     rows instead of once per sixteen.  profiles/apply64_resource_usage.txt has the registers and LDS of every instantiation.
//   * ROW PITCH: 16 kp + 1 doubles (kp = k rounded up to 4).  ds_read_b64 is served per half wave on 64 four-byte banks: the
//     B-fragment read of lanes (lr, h) touches doubles lr pitch + 16 h + const, and 16 kp is a multiple of 32 doubles, so the
//     double-bank index is (lr + 16 (h & 1)) mod 32 -- the sixteen lanes lr < 8 of a half hit sixteen different bank pairs
//     and lanes lr >= 8 read the address of lane lr - 8 (a broadcast).  The result writes (sixteen contiguous lanes = one h,
//     bank pair lr mod 16) and the staging accesses (sixteen contiguous doubles per group) are conflict-free as well.
//   * REGISTER SETS: two sets of a[KS] (the block row in use and the one requested ahead) in every instantiation.  Above
//     KT = 4 the image alone keeps a CU at one workgroup, i.e. one wavefront per SIMD with 512 registers to its name; two sets
//     at KT = 8 are 128 of them.  No instantiation uses scratch.
// apply_global64_tile_kernel<KT>: xa_v (k x G) = W^T x_v' + mean with the sixteen POINTS as the columns of the product, so
// the B operand (128-byte runs of a member's row) and the result go straight between memory and registers: no LDS.  One
// wavefront per tile and all state rows; W^T stays in registers for KT <= 3 (72 registers) and is reloaded per block row
// (from the cache: 8 k^2 bytes in all) above.
//
// PADDING AND NON-FINITE INPUT.  A column of the product (a state row of a point; a point in the global kernel) sums only
// its own B column, so a NaN in x[v][.][g] stays in outputs (v, ., g), and W_g is used by point g alone.  Padding never
// meets a non-finite mean: B entries of members beyond k, of rows beyond the pass and of points beyond the tile are SELECTED
// to exact zero after the mean is removed (not left as 0 - mean against zero rows of W), and A entries beyond k are selected
// zeros as well; padding rows and points of the image are zeros and are never stored.
//
// A point's sums run in a fixed order that depends on nothing but k (members 4 ks + h, ks ascending inside the matrix
// instruction chain; the mean: per lane ks ascending, then the two cross-lane steps), so a point's bits do not depend on its
// tile, its neighbours or the shard it is launched in.  Builtins only; the first vector read of a result block (+ mean)
// precedes every branch.
#include "mia_common.h"
#include "mia_kernels.h"
#include "mia_options.h"
#include "mia_tile_launch.h"

namespace mia {

using d4a = __attribute__((ext_vector_type(4))) double;

constexpr int kApply64Rows = 8;       // state rows per pass of the per-point kernel (see above)
constexpr int kApply64KMax = 128;

struct Apply64Params {
  const double* X; int64_t ldx; int m, k; int64_t g0, ng; const double* W; double* Xa; int64_t ldo, o0;
  int kp;        // members rounded up to a multiple of 4 (depth of one matrix instruction)
  int pitch;     // doubles per state row of the LDS image: 16 kp + 1
};

__device__ __forceinline__ double apply64_add_h(double v) {          // sum over the four lanes (lr, h = 0..3), in every one of them
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// workgroups per CU the image allows (= wavefronts per SIMD the registers have to allow)
template <int KT>
__global__ __launch_bounds__(256, KT <= 2 ? 4 : (KT == 3 ? 3 : (KT == 4 ? 2 : 1))) void apply_local64_tile_kernel(Apply64Params P) {
  extern __shared__ __attribute__((aligned(16))) double img64[];       // [8 rows][kp members][16 points], row pitch P.pitch
  constexpr int KS = 4 * KT;                                           // depth steps of four members
  constexpr int RP = kApply64Rows;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, h = lane >> 4;
  const int rl = lr & (RP - 1);                                        // the state row whose image this lane reads
  const bool rowlane = lr < RP;                                        // columns 8..15 of the product: zeros
  const int k = P.k, kp = P.kp, pitch = P.pitch;
  const int64_t p0 = (int64_t)blockIdx.x << 4;
  const int npts = P.ng - p0 < 16 ? (int)(P.ng - p0) : 16;
  const int nks = kp >> 2;                                             // depth steps that hold members
  const int sg = tid & 15, s0 = tid >> 4;                              // staging: member s0 + 16 it, point sg of its segments
  const double dk = (double)k;
  const int64_t xrow = (int64_t)k * P.ldx, orow = (int64_t)k * P.ldo;  // doubles between two state rows
  for (int r0 = 0; r0 < P.m; r0 += RP) {
    const int nrows = P.m - r0 < RP ? P.m - r0 : RP;
    // ---- the tile's next eight state rows into the image (rows / points / members that do not exist: zeros): thread (s0, sg)
    //      takes point sg of the segments (row v, member s0 + 16 it), eight loads in flight.  A row's base is uniform and
    //      64-bit; the lane offset (member i, point sg) is 32-bit: (k + 3) ldx 8 < 2^32 is checked on the host.
    {
      const double* xb = P.X + (int64_t)r0 * xrow + P.g0 + p0;
      for (int i = s0; i < kp; i += 16) {
        const unsigned off = ((unsigned)i * (unsigned)P.ldx + (unsigned)sg) * 8u;
        const bool keep = i < k && sg < npts;
        double val[RP];
#pragma unroll
        for (int u = 0; u < RP; ++u)
          val[u] = (keep && u < nrows) ? *reinterpret_cast<const double*>(reinterpret_cast<const char*>(xb + (int64_t)u * xrow) + off) : 0.0;
#pragma unroll
        for (int u = 0; u < RP; ++u) img64[u * pitch + i * 16 + sg] = val[u];
      }
    }
    __syncthreads();
    // ---- this wavefront's four points, one block row (sixteen new members j) of one point at a time: its slice of W_g is the
    //      A operand, requested one unit ahead of its products
    auto load_w = [&](int g, int jb, double (&a)[KS]) {               // a[ks] = W_g[4 ks + h][16 jb + lr]
      const double* wg = P.W + (p0 + g) * (int64_t)k * k;
      const int j = 16 * jb + lr;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int i = 4 * ks + h;
        a[ks] = (g < npts && i < k && j < k) ? wg[i * k + j] : 0.0;
      }
    };
    double a[KS], an[KS], b[KS];
    double mean = 0.0;
    load_w(4 * wave, 0, an);
#pragma unroll 1
    for (int u = 0; u < 4 * KT; ++u) {
      const int pp = u / KT, jb = u - pp * KT, g = 4 * wave + pp;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
      if (u + 1 < 4 * KT) {
        const int un = u + 1, ppn = un / KT;
        load_w(4 * wave + ppn, un - ppn * KT, an);
      }
      if (g >= npts || 16 * jb >= k) continue;                         // (wave-uniform)
      if (jb == 0) {
        // B fragments: b[ks] = x[row lr][member 4 ks + h] of point g; the row's mean over the members (its four lanes hold
        // disjoint quarters of them; members k .. kp - 1 of the image are zeros), removed before the products.  What is
        // not a member of an existing row becomes an exact zero whatever the mean is.
        double part = 0.0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          b[ks] = ks < nks ? img64[rl * pitch + (4 * ks + h) * 16 + g] : 0.0;
          part += b[ks];
        }
        mean = apply64_add_h(part) / dk;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = (rowlane && 4 * ks + h < k) ? b[ks] - mean : 0.0;
      }
      // the block row of the result: new members j = 16 jb + 4 q + h of state row lr, back into column g of the image (all KS
      // depth steps run: beyond the members both operands are zero)
      d4a acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks], acc, 0, 0, 0);
      double out[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) out[q] = acc[q] + mean;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 16 * jb + 4 * q + h;
        if (rowlane && j < k) img64[lr * pitch + j * 16 + g] = out[q];
      }
    }
    __syncthreads();
    // ---- the image leaves as whole segments
    {
      double* ob = P.Xa + (int64_t)r0 * orow + P.o0 + p0;
      for (int i = s0; i < k; i += 16) {
        const unsigned off = ((unsigned)i * (unsigned)P.ldo + (unsigned)sg) * 8u;
        if (sg < npts) {
#pragma unroll 4
          for (int v = 0; v < nrows; ++v)
            *reinterpret_cast<double*>(reinterpret_cast<char*>(ob + (int64_t)v * orow) + off) = img64[v * pitch + i * 16 + sg];
        }
      }
    }
    __syncthreads();
  }
}

// ONE weight matrix for all grid points: sixteen consecutive points are the N dimension of the matrix instruction.
template <int KT>
__global__ __launch_bounds__(256) void apply_global64_tile_kernel(Apply64Params P) {
  constexpr int KS = 4 * KT;
  constexpr bool kWholeW = KT <= 3;
  const int lane = threadIdx.x & 63, lr = lane & 15, h = lane >> 4;
  const int k = P.k;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t p0 = tile << 4;
  if (p0 >= P.ng) return;
  const int npts = P.ng - p0 < 16 ? (int)(P.ng - p0) : 16;
  const double dk = (double)k;
  auto load_w = [&](int jb, double (&a)[KS]) {                         // a[ks] = W[4 ks + h][16 jb + lr]
    const int j = 16 * jb + lr;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = 4 * ks + h;
      a[ks] = (i < k && j < k) ? P.W[i * k + j] : 0.0;
    }
  };
  double aw[kWholeW ? KT : 1][KS];
  if constexpr (kWholeW) {
#pragma unroll
    for (int jb = 0; jb < KT; ++jb) load_w(jb, aw[jb]);
  }
  const bool col = lr < npts;
  // 32-bit lane offsets (member i or j, point lr) on a row's uniform 64-bit base: (k + 3) ld 8 < 2^32 is checked on the host
  const unsigned xoff = (unsigned)lr * 8u, xstep = (unsigned)P.ldx * 8u, ostep = (unsigned)P.ldo * 8u;
  for (int v = 0; v < P.m; ++v) {
    const char* xb = reinterpret_cast<const char*>(P.X + (int64_t)v * k * P.ldx + P.g0 + p0);
    char* ob = reinterpret_cast<char*>(P.Xa + (int64_t)v * k * P.ldo + P.o0 + p0);
    double b[KS];
    double part = 0.0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = 4 * ks + h;
      b[ks] = (col && i < k) ? *reinterpret_cast<const double*>(xb + (xoff + (unsigned)i * xstep)) : 0.0;
      part += b[ks];
    }
    const double mean = apply64_add_h(part) / dk;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = (col && 4 * ks + h < k) ? b[ks] - mean : 0.0;   // (padding: exact zeros, whatever the mean)
#pragma unroll
    for (int jb = 0; jb < KT; ++jb) {
      if (16 * jb < k) {                                               // (uniform)
        d4a acc = {0.0, 0.0, 0.0, 0.0};
        if constexpr (kWholeW) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aw[jb][ks], b[ks], acc, 0, 0, 0);
        } else {
          double one[KS];
          load_w(jb, one);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(one[ks], b[ks], acc, 0, 0, 0);
        }
        double out[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = acc[q] + mean;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = 16 * jb + 4 * q + h;
          if (col && j < k) *reinterpret_cast<double*>(ob + (xoff + (unsigned)j * ostep)) = out[q];
        }
      }
    }
  }
}

// ---- cover (host only) -----------------------------------------------------------------------------------------------------
size_t apply_local64_lds_bytes(int k) { return (size_t)kApply64Rows * (16 * (size_t)((k + 3) & ~3) + 1) * sizeof(double); }

static bool apply64_shape_ok(int m, int k, int64_t ldx, int64_t ldo, int64_t ng) {
  if (k < 2 || k > kApply64KMax || m < 1 || ng < 1 || ldx < 1 || ldo < 1) return false;
  // 32-bit lane offsets (i ld + sg) 8: member i <= kp - 1 <= k + 2 (staging walks the padded members too, their loads switched
  // off), point sg <= 15
  if ((int64_t)(k + 3) * ldx * 8 >= ((int64_t)1 << 32) || (int64_t)(k + 3) * ldo * 8 >= ((int64_t)1 << 32)) return false;
  return true;
}
bool apply_local64_covers(int m, int k, int64_t ldx, int64_t ldo, int64_t ng) {
  if (!apply64_shape_ok(m, k, ldx, ldo, ng)) return false;
  if (((ng + 15) >> 4) > 2147483647LL) return false;
  return apply_local64_lds_bytes(k) <= kMaxDynamicLds;
}
bool apply_global64_covers(int m, int k, int64_t ldx, int64_t ldo, int64_t ng) {
  if (!apply64_shape_ok(m, k, ldx, ldo, ng)) return false;
  return ((((ng + 15) >> 4) + 3) >> 2) <= 2147483647LL;
}

// ---- hand-over under the default option (apply64 = -1) ---------------------------------------------------------------------
// The tile kernel takes a shape class by default where its slowest round beat the fallback's fastest by more than the larger
// spread (tools/time_apply64.py, profiles/apply64_time.json; MI355X, 1e5 points, ms fallback -> tile):
//   per point   k = 20: m = 1 0.132 -> 0.113, 8 0.731 -> 0.133, 16 1.41 -> 0.250, 64 5.35 -> 0.938
//               k = 40: m = 1 0.321 -> 0.283, 8 1.71 -> 0.372, 16 3.28 -> 0.625, 64 12.8 -> 2.37
//               k = 64: m = 1 0.650 -> 0.627, 8 4.21 -> 0.821, 16 8.37 -> 1.58,  64 34.1 -> 5.87
//               k = 80: m = 1 1.191 -> 1.122, 8 9.79 -> 1.30,  16 19.8 -> 2.34,  64 73.1 -> 8.22
//               k = 128: m = 1 2.36 -> 4.94 (LOST), 8 18.7 -> 5.09, 16 37.8 -> 10.1, 64 173 -> 40.2
//   global      k = 40: m = 1 0.094 -> 0.022, 16 1.08 -> 0.228, 64 4.22 -> 0.880;  k = 128: 1.56 -> 0.174, 19.7 -> 2.37, 83.4 -> 9.37
// Above eighty members the image keeps a CU at one workgroup and a single state row does not pay for it (k = 128, m = 1:
// 0.48 x); between the measured points -- 80 < k, m < 8 -- nothing was measured, so the fallback keeps them.
constexpr int kApplyLocal64AnyRowsKMax = 80;    // up to here every m >= 1 won
constexpr int kApplyLocal64WideMinRows = 8;     // 80 < k <= 128: from eight state rows on (k = 128, m = 1 lost: 2.36 against 4.94 ms)
static bool apply_local64_default(int m, int k) { return k <= kApplyLocal64AnyRowsKMax || m >= kApplyLocal64WideMinRows; }
static bool apply_global64_default(int, int) { return true; }      // every measured class won (4.3 x .. 9 x)

static bool apply64_route_open(bool by_default) {
  if (!option(MIA_OPT_TILE)) return false;
  const int o = option_apply64();
  return o > 0 || (o < 0 && by_default);
}

int apply_global64_tile_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* W, double* Xa,
                               int64_t ldo, int64_t o0, hipStream_t stream) {
  if (!apply_global64_covers(m, k, ldx, ldo, ng) || !apply64_route_open(apply_global64_default(m, k))) return MIA_ERR_UNSUPPORTED;
  const int64_t nb = (((ng + 15) >> 4) + 3) >> 2;
  Apply64Params p{X, ldx, m, k, g0, ng, W, Xa, ldo, o0, (k + 3) & ~3, 0};
  const int kt = (k + 15) >> 4;
  void (*kern)(Apply64Params) = nullptr;
  if (dispatch_upto<8>(kt, [&](auto kt_c) { kern = apply_global64_tile_kernel<kt_c()>; return MIA_OK; }) != MIA_OK) return MIA_ERR_UNSUPPORTED;
  kern<<<dim3((unsigned)nb), dim3(256), 0, stream>>>(p);
  MIA_LAUNCH_CHECK();
  note_transform_kernel("apply_global64_tile_kernel<%d>", kt);
  return MIA_OK;
}

int apply_local64_tile_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* W, double* Xa,
                              int64_t ldo, int64_t o0, hipStream_t stream) {
  if (!apply_local64_covers(m, k, ldx, ldo, ng) || !apply64_route_open(apply_local64_default(m, k))) return MIA_ERR_UNSUPPORTED;
  const int64_t ntile = (ng + 15) >> 4;
  Apply64Params p{X, ldx, m, k, g0, ng, W, Xa, ldo, o0, (k + 3) & ~3, 0};
  p.pitch = 16 * p.kp + 1;
  const size_t lds = apply_local64_lds_bytes(k);
  const int kt = (k + 15) >> 4;
  void (*kern)(Apply64Params) = nullptr;
  if (dispatch_upto<8>(kt, [&](auto kt_c) { kern = apply_local64_tile_kernel<kt_c()>; return MIA_OK; }) != MIA_OK) return MIA_ERR_UNSUPPORTED;
  if (lds > 48 * 1024) MIA_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<dim3((unsigned)ntile), dim3(256), lds, stream>>>(p);
  MIA_LAUNCH_CHECK();
  note_transform_kernel("apply_local64_tile_kernel<%d>", kt);
  return MIA_OK;
}

}  // namespace mia

extern "C" int mia_apply_local_f64_cover(int m, int k, int64_t ldx, int64_t ldo, int64_t n_points) {
  return mia::apply_local64_covers(m, k, ldx, ldo, n_points) ? 1 : 0;
}
extern "C" int mia_apply_f64_cover(int m, int k, int64_t ldx, int64_t ldo, int64_t n_points) {
  return mia::apply_global64_covers(m, k, ldx, ldo, n_points) ? 1 : 0;
}
