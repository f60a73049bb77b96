// Internal launchers shared between translation units (not part of the C ABI).
#pragma once
#include "mia_common.h"
#include "mia_localize_dev.h"

namespace mia {

// a segment's 64 slot counters sit kSlotStride ints apart (one per 256 bytes): atomics that share a cache line
// are serialised by the L2 channel that owns it (25 000 on one line cost more than the whole analysis)
constexpr int kSlotStride = 64;

// IEnKS update (tau = 1) through the weights variant of the matfun kernel: variant 1 transform (points whose Wp is not the
// identity are declined), 2 bundle (inv_eps = 1 / epsilon)
struct IenksOpts { int variant; const float* W_in; int64_t w_stride; float inv_eps; };

// letkf_cheb.hip.  MIA_ERR_UNSUPPORTED when the shape is outside the matfun route.
// seg_len > 0: one segmented launch over the ng points (native step driver): segment s = points
// [s*seg_len, (s+1)*seg_len) writes the (m*k, seg_len) buffer at Xa + s*seg_stride (ldo = seg_len) and counts
// its finished points in the 64 slot counters done[(s*64 + j) * kSlotStride] (zeroed by the caller); needs seg_len % 8 == 0.
int cheb_analysis_launch(const float* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const float* rec,
                         const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                         float inf_factor, int kernel_mode, float gamma, float* Xa, int64_t ldo, int64_t o0,
                         int32_t* flags, int32_t* retry_count, const ScanParams* scan, int32_t* stats,
                         hipStream_t stream, int seg_len = 0, int64_t seg_stride = 0, int32_t* done = nullptr,
                         float* W_out = nullptr /* weights-output variant: [ng][k][k] */, const IenksOpts* ienks = nullptr);

// apply_local.hip: the per-grid-point weight transform on tiles of sixteen points (float32, k <= 96; MIA_ERR_UNSUPPORTED otherwise)
int apply_local_tile_launch(const float* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const float* W, float* Xa,
                            int64_t ldo, int64_t o0, hipStream_t stream);

// ... and with ONE weight matrix for all points (the global ETKF's transform): grid points as the columns of a plain product
int apply_global_tile_launch(const float* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const float* W, float* Xa,
                             int64_t ldo, int64_t o0, hipStream_t stream);

// apply_local64.hip: both transforms in float64 on the same frame (v_mfma_f64_16x16x4_f64, 2 <= k <= 128, any m).
// apply_*64_covers: shape test (host only; the 32-bit lane offsets and, per point, the LDS of the instantiation);
// apply_*64_tile_launch: MIA_ERR_UNSUPPORTED outside it, with the option tile = 0, with apply64 = 0, and with apply64 = -1
// where the round-1 kernel is kept by default (the caller then runs apply_local_weights_kernel / apply_weights_kernel)
bool apply_local64_covers(int m, int k, int64_t ldx, int64_t ldo, int64_t ng);
bool apply_global64_covers(int m, int k, int64_t ldx, int64_t ldo, int64_t ng);
size_t apply_local64_lds_bytes(int k);
int apply_local64_tile_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* W, double* Xa,
                              int64_t ldo, int64_t o0, hipStream_t stream);
int apply_global64_tile_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* W, double* Xa,
                               int64_t ldo, int64_t o0, hipStream_t stream);
// The transform kernel an entry point has just put on a stream, under the name rocprofv3 records for it: read back by
// mia_last_transform_kernel.  A slot of its own: mia_last_analysis_kernel keeps naming the analysis.  printf-style.
void note_transform_kernel(const char* fmt, ...);

// Chebyshev coefficient tables of the matfun kernels (letkf_cheb.hip, cheb_coef_table): geometric grid of scaled
// spectral bounds T = L / reg, 32 per octave over 2^-24 .. 2^8; entry i holds {degree, bits of 2 / T} and 64 (phi, psi)
// coefficient pairs, zero beyond the degree.
constexpr int kTabPerOctave = 32, kTabIdx0 = 24 * kTabPerOctave, kTabN = 32 * kTabPerOctave, kTabDeg = 64;

// letkf_tile.hip: the same analysis with sixteen grid points per wavefront (dual route, k <= 64, few state rows).
// tile_route_covers: shape test; tile_analysis_launch: MIA_ERR_UNSUPPORTED outside it.  nbr_w is float64 or (w_f32)
// float32 lists.
bool tile_route_covers(int m, int k, int p_max);
int tile_analysis_launch(const float* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const float* rec,
                         const int32_t* nbr_cnt, const int32_t* nbr_idx, const void* nbr_w, int w_f32, int p_cap,
                         int p_max, float inf_factor, float* Xa, int64_t ldo, int64_t o0, int32_t* flags,
                         int32_t* retry_count, int dmax, const int2* tab_hdr, const float2* tab_c, hipStream_t stream,
                         int seg_len = 0, int64_t seg_stride = 0, int32_t* done = nullptr);
// (letkf_tile_split.hip) the same launch on the split-precision instantiations: every product on v_mfma_f32_16x16x32_f16
// with operands carried as pairs of halves; tile_analysis_launch forwards here when the option tile_split is on
int tile_split_analysis_launch(const float* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const float* rec,
                               const int32_t* nbr_cnt, const int32_t* nbr_idx, const void* nbr_w, int w_f32, int p_cap,
                               int p_max, float inf_factor, float* Xa, int64_t ldo, int64_t o0, int32_t* flags,
                               int32_t* retry_count, int dmax, const int2* tab_hdr, const float2* tab_c, hipStream_t stream,
                               int seg_len, int64_t seg_stride, int32_t* done);

// letkf_tile64.hip: the float64 analysis with sixteen grid points per wavefront, every product a v_mfma_f64_16x16x4_f64
// (dual route, 2 <= k <= 64, p_max <= k, any number of state rows), from float64 records and per-point lists.
// tile64_route_covers: shape test (host only); tile64_analysis_launch: MIA_ERR_UNSUPPORTED outside it, with the option
// tile = 0, and when the float64 coefficient table cannot be had (stream being captured).
bool tile64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng);
int tile64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                           hipStream_t stream);

// letkf_tile64w.hip: the float64 WEIGHTS [ng][k][k] on the same frame (what LETKF.estimate_weights returns,
// interface/letkf.py:127-146): one pass of the recurrence per member instead of per state row, no state and no analysis.
// weights64_route_covers: shape test (host only; 2 <= k <= 64, p_max <= k); weights64_launch: MIA_ERR_UNSUPPORTED outside
// it, with the option tile = 0, and when the float64 coefficient table cannot be had.
bool weights64_route_covers(int k, int p_max, int64_t ng);
int weights64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                     const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                     int32_t* retry_count, hipStream_t stream);

// lienks_tile64.hip: the float64 localised IEnKS weight update with tau = 1 on the same frame (core/ienks.py:108-141 without an
// eigensolver): the weights at inflation 1 with the innovations shifted by D^T w_mean; epsilon > 0 = bundle variant, else the
// transform variant, which declines every point whose Wp is not the identity.  lienks64_route_covers: shape test (host only;
// weights64_route_covers' bounds); lienks64_launch: MIA_ERR_UNSUPPORTED outside it, with the option tile = 0, and when the
// float64 coefficient table cannot be had.
bool lienks64_route_covers(int k, int p_max, int64_t ng);
int lienks64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec, const int32_t* nbr_cnt,
                    const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max, double epsilon, double* W_out,
                    int32_t* flags, int32_t* retry_count, hipStream_t stream);

// letkf_dense64.hip: the float64 analysis on tiles for dense local networks (primal form, 2 <= k <= 64, k < p_max <= the
// slots of the LDS record image, any number of state rows): the union streams through the wave block by block, C_g is never
// formed.  dense64_route_covers: shape test (host only; false for p_max <= k, which is letkf_tile64.hip's);
// dense64_analysis_launch: MIA_ERR_UNSUPPORTED outside it, with the option tile = 0, and when its coefficient table cannot
// be had.
bool dense64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng);
int dense64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                            const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                            double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                            hipStream_t stream);

// letkf_patch64.hip: letkf_dense64.hip's analysis with a tile's sixteen points taken from a map (4 x 4 patches of a 2-D mesh)
// and the record image sized by the caller; the cover is dense64_route_covers.  patch64_analysis_launch: MIA_ERR_UNSUPPORTED
// outside it, with the option tile = 0, and when the coefficient table cannot be had; MIA_ERR_SIZE for union_blocks outside
// 1 .. resident64_capacity_blocks(k) (mia_frames64.h).  tile_union_census_launch: validates the map and counts the largest union of a tile (ws:
// ng + 2 int32, zeroed here; out2: error bits MIA_TILEMAP_*, largest union).
int patch64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                            const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                            double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                            const int32_t* tile_pts, int64_t n_tiles, int union_blocks, hipStream_t stream);
int tile_union_census_launch(const int32_t* tile_pts, int64_t n_tiles, int64_t ng, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                             int p_cap, int p_max, int count_unions, int32_t* out2, int32_t* ws, hipStream_t stream);

// letkf_stream64.hip: letkf_dense64.hip's analysis with the union's records streamed through a ring of two sixteen-slot blocks
// in LDS instead of a resident image (primal form, 2 <= k <= 128, k < p_max <= 256, any number of state rows): what dense
// networks of 65 .. 128 members run.  stream64_route_covers: shape test (host only; false for p_max <= k, which is the dual
// routes'); stream64_analysis_launch: MIA_ERR_UNSUPPORTED outside it, with the option tile = 0, and when its coefficient
// table cannot be had.
bool stream64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng);
int stream64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                             const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                             double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                             hipStream_t stream);

// letkf_wide64.hip: letkf_tile64.hip's analysis for ensembles up to 128 members (dual route, 2 <= k <= 128, p_max <= k, any
// number of state rows): the row blocks of the union are split over the two or four wavefronts of a workgroup, which share
// one record image.  wide64_route_covers: shape test (host only, the LDS of the chosen instantiation included);
// wide64_analysis_launch: MIA_ERR_UNSUPPORTED outside it, with the option tile = 0, and when the float64 coefficient table
// cannot be had.
bool wide64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng);
int wide64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                           hipStream_t stream);

// letkf_wide64w.hip: letkf_tile64w.hip's float64 WEIGHTS [ng][k][k] for ensembles up to 128 members on letkf_wide64.hip's
// frame (2 <= k <= 128, p_max <= k): one pass of the recurrence per member, the row blocks of the union split over two or
// four wavefronts.  weights_wide64_route_covers: shape test (host only: the LDS of the chosen instantiation, the launch grid,
// the 32-bit offsets inside a tile's weights); weights_wide64_launch: MIA_ERR_UNSUPPORTED outside it, with the option
// tile = 0, and when the float64 coefficient table cannot be had.
bool weights_wide64_route_covers(int k, int p_max, int64_t ng);
int weights_wide64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                          const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                          int32_t* retry_count, hipStream_t stream);

// letkf_stream64w.hip: the float64 WEIGHTS [ng][k][k] for dense local networks on letkf_stream64.hip's frame (primal form,
// 2 <= k <= 128, k < p_max <= 256): one pass of the recurrence per member on e_c, the union's records streamed through the ring.
// weights_stream64_route_covers: shape test (host only: the LDS of the launch, the launch grid, the 32-bit offsets inside a
// tile's weights; false for p_max <= k, which is the dual routes'); weights_stream64_launch: MIA_ERR_UNSUPPORTED outside it,
// with the option tile = 0, and when its coefficient table cannot be had.
bool weights_stream64_route_covers(int k, int p_max, int64_t ng);
int weights_stream64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                            const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                            int32_t* retry_count, hipStream_t stream);

// letkf_patch64w.hip: letkf_stream64w.hip's weights with a tile's sixteen points taken from a map (4 x 4 patches of a 2-D mesh)
// and the slot tables sized by the caller, 1 <= union_blocks <= 16 at every ensemble size.  weights_patch64_route_covers: shape
// test (host only: 2 <= k <= 128, k < p_max <= 256, ng < 2^31 for the int32 map entries, k^2 8 < 2^31 for the 32-bit offset
// inside a point's weights, the LDS of the largest image); weights_patch64_launch: MIA_ERR_UNSUPPORTED outside it, with
// union_blocks outside 1 .. 16, more tiles than a launch grid holds, the option tile = 0, and when its coefficient table
// cannot be had.  The map is validated by tile_union_census_launch (letkf_patch64.hip).
bool weights_patch64_route_covers(int k, int p_max, int64_t ng);
int weights_patch64_launch(int k, int64_t ng, const double* rec, const int32_t* nbr_cnt, const int32_t* nbr_idx,
                           const double* nbr_w, int p_cap, int p_max, double inf_factor, double* W, int32_t* flags,
                           int32_t* retry_count, const int32_t* tile_pts, int64_t n_tiles, int union_blocks, hipStream_t stream);

// letkf_patch64s.hip: letkf_stream64.hip's analysis with a tile's sixteen points taken from a map (4 x 4 patches of a 2-D mesh)
// and the slot tables sized by the caller; the cover is stream64_route_covers.  patch64s_analysis_launch: MIA_ERR_UNSUPPORTED
// outside it, with ng >= 2^31 (the map's entries are int32), more tiles than a launch grid holds, the option tile = 0, and when
// the coefficient table cannot be had; MIA_ERR_SIZE for union_blocks outside 1 .. 16, at every ensemble size.  The map is
// validated by tile_union_census_launch (letkf_patch64.hip).
int patch64s_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                             const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                             double inf_factor, double* Xa, int64_t ldo, int64_t o0, int32_t* flags, int32_t* retry_count,
                             const int32_t* tile_pts, int64_t n_tiles, int union_blocks, hipStream_t stream);

// lienks_wide64.hip: lienks_tile64.hip's float64 IEnKS weight update with tau = 1 for ensembles up to 128 members on
// letkf_wide64w.hip's frame (2 <= k <= 128, p_max <= k): the weights at inflation 1 with the innovations shifted by
// D^T w_mean, the row blocks of the union split over two or four wavefronts.  lienks_wide64_route_covers: shape test (host
// only; weights_wide64_route_covers' arithmetic); lienks_wide64_launch: MIA_ERR_UNSUPPORTED outside it, with the option
// tile = 0, and when the float64 coefficient table cannot be had.
bool lienks_wide64_route_covers(int k, int p_max, int64_t ng);
int lienks_wide64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec, const int32_t* nbr_cnt,
                         const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max, double epsilon, double* W_out,
                         int32_t* flags, int32_t* retry_count, hipStream_t stream);

// lienks_stream64.hip: the same update for DENSE local networks on letkf_stream64w.hip's frame (2 <= k <= 128,
// k < p_max <= 256), the union's records streamed through a ring in LDS.  lienks_stream64_route_covers: shape test (host
// only; weights_stream64_route_covers' arithmetic); lienks_stream64_launch: MIA_ERR_UNSUPPORTED outside it, with the option
// tile = 0, and when the float64 coefficient table cannot be had.
bool lienks_stream64_route_covers(int k, int p_max, int64_t ng);
int lienks_stream64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec, const int32_t* nbr_cnt,
                           const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max, double epsilon, double* W_out,
                           int32_t* flags, int32_t* retry_count, hipStream_t stream);

// lienks_patch64.hip: lienks_stream64.hip's update with a tile's sixteen points taken from a map (4 x 4 patches of a 2-D mesh;
// W_in, W_out, lists and flags all go through it) and the slot tables sized by the caller, 1 <= union_blocks <= 16 at every
// ensemble size.  lienks_patch64_route_covers: shape test (host only; weights_patch64_route_covers' arithmetic);
// lienks_patch64_launch: MIA_ERR_UNSUPPORTED outside it, with union_blocks outside 1 .. 16, more tiles than a launch grid, the
// option tile = 0, and when the float64 coefficient table cannot be had.
bool lienks_patch64_route_covers(int k, int p_max, int64_t ng);
int lienks_patch64_launch(const double* W_in, int64_t w_stride, int k, int64_t ng, const double* rec, const int32_t* nbr_cnt,
                          const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max, double epsilon, double* W_out,
                          int32_t* flags, int32_t* retry_count, const int32_t* tile_pts, int64_t n_tiles, int union_blocks,
                          hipStream_t stream);

// lketkf_tile64.hip: the float64 RBF-kernelised analysis on tiles (2 <= k <= 40, lists of at most 64 observations, any number
// of state rows; no p_max <= k condition): one workgroup of four wavefronts per tile, the pair statistic on the matrix
// cores, a point's k x k matrix in LDS.  rbf64_route_covers: shape test (host only, the LDS of the chosen instantiation
// included); rbf64_analysis_launch: MIA_ERR_UNSUPPORTED outside it, without gamma > 0, with the option tile = 0, and when the
// float64 coefficient table cannot be had.
bool rbf64_route_covers(int m, int k, int p_max, int64_t ldx, int64_t ldo, int64_t ng);
int rbf64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                          const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                          double inf_factor, double gamma, double* Xa, int64_t ldo, int64_t o0, int32_t* flags,
                          int32_t* retry_count, hipStream_t stream);

// lketkf_kern64.hip (the ST != 0 instantiations of lketkf_tile64.hip): the same analysis with K from a kernel expression
// (host array `prog`, checked here again); the cover is rbf64_route_covers.  MIA_ERR_UNSUPPORTED outside it, for a malformed
// program or one with tanh / sin, with the option tile = 0, and when the float64 coefficient table cannot be had.
int kern64_analysis_launch(const double* X, int64_t ldx, int m, int k, int64_t g0, int64_t ng, const double* rec,
                           const int32_t* nbr_cnt, const int32_t* nbr_idx, const double* nbr_w, int p_cap, int p_max,
                           double inf_factor, const mia_kernel_op_t* prog, int n_ops, double* Xa, int64_t ldo, int64_t o0,
                           int32_t* flags, int32_t* retry_count, hipStream_t stream);

// Completion event for the next tile-kernel launch of this thread (set by the step driver around the analysis call of a
// step in flight): the launch then carries the event in its own dispatch packet (hipExtLaunchKernel) instead of the caller
// recording a marker packet behind it -- one packet less between two kernels of the analysis queue.  Cleared by the launch
// that takes it.
hipEvent_t& launch_stop_event();
hipEvent_t& launch_start_event();     // optional timing partner of the above (the dispatch's own start time)
// The analysis kernel a launch function has just put on a stream, under the name rocprofv3 records for it (template arguments
// included): read back by mia_last_analysis_kernel, so that bench lines and tools label their figures with the kernel that
// ran, not with a guess from the route options.  printf-style.
void note_analysis_kernel(const char* fmt, ...);
// launches of the tile kernel made by this thread so far; whether a launch with these sizes would be accepted by it
unsigned long long& tile_launch_count();
bool tile_launch_would_serve(int m, int k, int p_max, int p_cap, int64_t ldx, int64_t ldo, int64_t ng, int seg_len);
// (letkf_cheb.hip) whether mia_letkf_analysis_matfun_f32 with these arguments ends in the tile kernel -- the dispatch rule
// of cheb_analysis_launch, evaluated without launching (builds the coefficient table on `stream` if it does not exist yet)
bool cheb_tile_will_serve(int m, int k, int p_max, int p_cap, float gamma, int64_t ldx, int64_t ldo, int64_t ng, hipStream_t stream);

// (letkf_cheb.hip) coefficient table of the dual route at the default truncation target (built on first use, per device)
bool cheb_dual_table(hipStream_t stream, const int2** hdr, const float2** c);
// ... and of the primal route (the RBF-kernelised tile kernel, lketkf_tile.hip)
bool cheb_primal_table(hipStream_t stream, const int2** hdr, const float2** c);

// one-wave kernel on `stream` that returns once the 64 slot counters at done64[j * kSlotStride] sum to `expected` (bounded
// polling: after ~seconds it sets bit 0 of *err and returns, so the grid always drains)
int segment_wait_launch(const int32_t* done64, int expected, int32_t* err, hipStream_t stream);

}  // namespace mia
