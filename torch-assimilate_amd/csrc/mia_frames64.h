// Sizing rules of the three float64 tile frames, each once: what a launch asks for in LDS, how many sixteen-slot blocks it
// takes for a longest list of p_max, and what an ensemble size can hold.  The kernel of a frame lays its LDS out by the same
// arithmetic (each kernel file says which frame it launches with); tests/test_*_cover.py restate the rules independently.
// Host only: nothing here is device code.
#pragma once
#include "mia_common.h"

namespace mia {

// ---- resident image (letkf_tile64, letkf_tile64w, lienks_tile64; letkf_dense64, letkf_patch64): the records of a tile's union in LDS.
// image [16 blocks][kp | 1] + sqrt(rho) [16][16 blocks + 1] doubles, slot table [16 blocks] ints; kp = round_up(k + 1, 4)
static inline size_t resident64_lds_bytes(int blocks, int kp) {
  const int umax = 16 * blocks;
  return align_up(((size_t)umax * (kp | 1) + 16 * (size_t)(umax + 1)) * sizeof(double) + (size_t)umax * sizeof(int), 16);
}
// dual routes (p_max <= k <= 64): slots an instantiation offers a tile beyond the longest single list (as letkf_tile.hip: sixteen
// consecutive points of a regular network add ~one observation per second point), up to the four blocks the kernels are built for
static inline int resident64_ut(int p_max) {
  const int ut = (p_max + 8 + 15) >> 4;
  return ut < 1 ? 1 : (ut > 4 ? 4 : ut);
}
// primal routes (p_max > k): sixteen-slot blocks the record image of this ensemble size may have (256 slots where they fit) ...
constexpr int kResident64MaxBlocks = 16;
static inline int resident64_capacity_blocks(int k) {
  const int kp = (k + 1 + 3) & ~3;
  int ub = kResident64MaxBlocks;
  while (ub > 0 && resident64_lds_bytes(ub, kp) > kMaxDynamicLds) --ub;
  return ub;
}
// ... and the blocks a launch takes: the longest list plus what sixteen consecutive points of a regular network add (one
// observation per point at stride 1).  Fewer slots = more workgroups per compute unit; a tile that needs more is halved.
static inline int resident64_blocks(int k, int p_max) {
  const int cap = resident64_capacity_blocks(k), want = (p_max + 16 + 15) >> 4;
  return want < cap ? want : cap;
}

// ---- wide (letkf_wide64, letkf_wide64w, lienks_wide64): one record image per workgroup of NW wavefronts, k <= 128.
// UT = ceil((p_max + 8) / 16) as the resident image, up to eight blocks
static inline int wide64_ut(int p_max) {
  const int ut = (p_max + 8 + 15) >> 4;
  return ut < 1 ? 1 : (ut > 8 ? 8 : ut);
}
// two wavefronts hold up to six row blocks (three each: 8 * 6 * 3 = 144 registers of Gram matrix), four the rest
constexpr int wide64_nw(int ut) { return ut <= 6 ? 2 : 4; }
static inline size_t wide64_lds_bytes(int ut, int kt, int nw) {
  const int umax = 16 * ut;
  return align_up(((size_t)umax * (16 * kt + 5) + 16 * (size_t)(umax + 1) + 16 * (size_t)nw) * sizeof(double) +
                  (size_t)(umax + nw) * sizeof(int), 16);
}

// ---- ring (letkf_stream64, letkf_stream64w, lienks_stream64, letkf_patch64w, lienks_patch64, letkf_patch64s): the union's records streamed, k <= 128.
// ring [2][16][kp | 1] + rhs [4 KT][64] + sqrt(rho) [16][16 ub + 1] doubles, slot table [16 ub] ints
constexpr int kRing64MaxBlocks = 16;                            // 256 slots, at every ensemble size of the routes
static inline size_t ring64_lds_bytes(int ub, int k) {
  const int umax = 16 * ub, kp = (k + 1 + 3) & ~3, kt = (k + 15) >> 4;
  return align_up(((size_t)2 * 16 * (kp | 1) + (size_t)4 * kt * 64 + 16 * (size_t)(umax + 1)) * sizeof(double) +
                  (size_t)umax * sizeof(int), 16);
}
// the blocks a launch takes: resident64_blocks' rule without a capacity that depends on k
static inline int ring64_blocks(int p_max) {
  const int want = (p_max + 16 + 15) >> 4;
  return want < kRing64MaxBlocks ? want : kRing64MaxBlocks;
}

}  // namespace mia
