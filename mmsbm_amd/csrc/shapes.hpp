// shapes.hpp -- sizes and limits every translation unit of the library agrees on: the padding of K and L, workgroup
// sizes, unit lengths and the LDS footprints the kernels are launched with (host arithmetic only: no kernels, no HIP type)
#pragma once

namespace {

inline int pad_dim(int d) {  // multiples of 4: 32-byte row granules, whole chunks of 4 outputs
  if (d <= 256) return (d + 3) / 4 * 4;
  if (d <= 512) return (d + 7) / 8 * 8;
  if (d <= 1024) return (d + 15) / 16 * 16;
  return (d + 31) / 32 * 32;  // (whole lanes of the 64 x 32 instantiation of the triple passes)
}

// (G, VEC) instantiation for a padded row length: code 0..6
// Four doubles (32 bytes) per lane: fewer lanes per row means more rows per wave instruction,
// i.e. less vector-ALU work (dot product, DPP reduction, division) per triple.
inline int group_code(int dp) {
  if (dp <= 16) return 0;   // G=4  VEC=4
  if (dp <= 32) return 1;   // G=8  VEC=4
  if (dp <= 64) return 2;   // G=16 VEC=4
  if (dp <= 128) return 3;  // G=32 VEC=4
  if (dp <= 256) return 4;  // G=64 VEC=4
  if (dp <= 512) return 5;  // G=64 VEC=8
  return 6;                 // G=64 VEC=16 (up to 1,024 groups)
}
constexpr int kMaxGroupRow = 1024;  // columns the widest (G, VEC) covers; wider rows: seg_wide_kernel / block loops
inline int group_lanes(int code) {
  static const int g[7] = {4, 8, 16, 32, 64, 64, 64};
  return g[code];
}

constexpr int kBlock = 256;          // threads of a workgroup, where nothing else is said
constexpr int kUnitPairs = 64;      // pairs of one rating a pair-stage workgroup multiplies at a time
constexpr int kPairBlockMax = 512;   // threads of the pair stage's big workgroups

constexpr int kQuadUnits = 4;  // 64-pair units a workgroup of pair_quad_a_kernel multiplies jointly
constexpr int kQuadMaxL = 56;  // its input rows at most (14 double2 per thread and chunk; beyond: pair_block like every other shape)

constexpr size_t kLdsBudget = 64 * 1024;  // dynamic LDS a launch may use without hipFuncSetAttribute
constexpr size_t kLdsMax = 160 * 1024;    // with hipFuncAttributeMaxDynamicSharedMemorySize

// dynamic LDS of pair_block: transposed rows + output rows (shared with the eta rows)
constexpr size_t kScalarTileBytes = 8 * 1024;  // larger tiles thrash the scalar cache: stage in LDS
inline bool tile_in_lds(int dinp, int doutp) {
  return static_cast<size_t>(dinp) * doutp * sizeof(double) > kScalarTileBytes;
}
// A rating tile beyond the scalar cache (kp * lp > 1024: 1,024 doubles are kScalarTileBytes): the shapes whose pair stage
// leaves the lane-per-pair form with its tile in scalar loads -- matrix cores, longer unit runs, direct stores, the quad A launch
inline bool tile_beyond_scalar_cache(int kp, int lp) { return static_cast<size_t>(kp) * lp * sizeof(double) > kScalarTileBytes; }
inline size_t pair_block_lds(int dinp, int doutp, bool tile_lds) {
  // transposed input rows + one region shared by the eta rows and the output rows [+ the tile]
  const size_t d = static_cast<size_t>(dinp) * (kUnitPairs + 1) + static_cast<size_t>(kUnitPairs) * doutp +
                   (tile_lds ? static_cast<size_t>(dinp) * doutp : 0);
  return d * sizeof(double);  // the S hand-over area reuses it (create() bounds the copies by it)
}
// dynamic LDS of pass_dense_kernel: pair_block's two regions, the first with max(kp, lp) rows -- it holds the unit's eta
// rows, transposed (lp rows), before the A rows and then the C rows (kp rows each) take their place
inline size_t pass_dense_lds(int kp, int lp) { return pair_block_lds(kp > lp ? kp : lp, lp, false); }

// ---- the pair stage on the matrix cores (pair_mfma.hpp) ----
constexpr int kMfmaMaxDim = 64;       // <= 4 tiles of 16 per side
constexpr int kMfmaChunkPairs = 1024;  // pairs per workgroup at most (their item ids are parked in LDS)
static_assert(kMfmaChunkPairs >= 4 * mmsbm::kMvChunkPairs, "pair_mfma_kernel parks a whole chunk's item ids in LDS");
constexpr int kMfmaBlk = 64;          // block of the blocked forms (mfma_rows_kernel, mfma_slab_kernel)
constexpr int kRowsUnits = 2;  // 64-pair units per workgroup of mfma_rows_kernel: one staged tile block serves them all
constexpr size_t kMfmaRowsLds = (kMfmaBlk * (kUnitPairs + 1) + kMfmaBlk * kMfmaBlk) * sizeof(double) + kRowsUnits * kUnitPairs * sizeof(int);
constexpr size_t kMfmaSlabLds = (kMfmaBlk * (kUnitPairs + 1) + kUnitPairs * kMfmaBlk) * sizeof(double) + kMfmaChunkPairs * sizeof(int);
inline size_t pair_mfma_lds(int dinp, int doutp, bool with_s) {
  return (static_cast<size_t>(dinp) * (kUnitPairs + 1) + static_cast<size_t>(dinp) * doutp +
          (with_s ? static_cast<size_t>(kUnitPairs) * doutp : 0)) * sizeof(double) + kMfmaChunkPairs * sizeof(int);
}

// The 4 x 4 blocks of the A launch (the T + S launch keeps padded tiles: its 128 registers do not hold them; measured,
// EXPERIMENTS.md).  An output side of 16 f + 4 r groups: f full 16-tiles; a remainder of 4 or 8 (r = 1, 2) runs as 4 x 4
// blocks on v_mfma_f64_4x4x4_4b_f64, a remainder of 12 stays a padded tile.  Packed for PairBlockArgs::mg0 / mg1.
inline void mfma_geometry(int dinp, int doutp, int *mg0, int *mg1) {
  const int fo = doutp >> 4, ro0 = (doutp & 15) >> 2;
  const int ro = (ro0 == 1 || ro0 == 2) ? ro0 : 0;
  const int nto = fo + ((ro0 && !ro) ? 1 : 0), mti = (dinp + 15) >> 4;      // (padded) 16-tiles per side
  const int rows_t = std::min(16 * mti, dinp), cols_t = std::min(16 * nto, doutp);   // rows / columns the tiles cover
  *mg0 = ro | (nto << 4) | (mti << 7);
  *mg1 = rows_t | (cols_t << 7);
}

// ---- wide rows (pair_quad.hpp: wide_matvec_kernel, wide_slab_kernel) ----
constexpr int kWidePairs = 8, kWideChunkPairs = 1024;
constexpr int kWideKG = 8;  // (16: the C values no longer fit the scalar registers, 921 vs 477 us)
inline size_t wide_matvec_lds(int dinp) { return static_cast<size_t>(kWidePairs) * dinp * sizeof(double); }

// ---- small problems: the two-launch iteration (fused_small.hpp) ----
inline size_t pairs_fused_lds(int kp, int lp, int split_parts = 0) {  // split_parts: partial rows of a unit's split pairs
  return (static_cast<size_t>(lp) * (kUnitPairs + 1) + static_cast<size_t>(kUnitPairs) * lp +
          static_cast<size_t>(kUnitPairs) * kp + static_cast<size_t>(kp) * (kUnitPairs + 1) +
          static_cast<size_t>(split_parts) * kp) * sizeof(double);
}
constexpr size_t kFusedSplitLds = 96 * 1024;  // partial rows of a workgroup's split user segments, at most

}  // namespace
