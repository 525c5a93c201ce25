// pair_plan.hpp -- the launch plan of the pair stage (T = P^T C, the K x L slabs, the A rows) as ONE value: which of the
// stage's forms runs, and with which geometry.  Host arithmetic on plain numbers only -- no HIP type, no context -- so
// that the rules tying the fields together are checked on the CPU over every shape (tests/native/pair_plan_check.cpp).
// Included after layout.hpp and shapes.hpp.  create() builds the plan (plan_pair_shape, then plan_pair_forms once the CU
// count and the pair count are known), options "mfma" and "quad" change it through set_mfma / set_quad, and the
// launching units (tu_pair.hip, tu_mfma.hip) read form_t() / form_a() and the instantiation keys: nothing else decides.
#pragma once

namespace mmsbm_hip_impl {  // (PairPlan is a member of mmsbm_hip_ctx: one type in every translation unit)

// pair_block_kernel<GATHER, DO_S, NACC, TLDS, NT, KT, DIRECT>: the plan ties three of the switches to ONE fact about the
// shape -- the padded tile holds more than 1,024 entries (8 KB, the scalar cache's share):
//   small tile: KT = 2, rows through LDS (DIRECT off), tile in scalar registers (TLDS off), NACC = 1
//   big tile:   KT = 4, rows straight from registers (DIRECT on), tile in LDS unless it does not fit beside the rows
// (four slots per thread, NACC = 4: only where 512 threads are too few for the tile's slots, (K/4)(L/4) > 1,024 -- such a
// tile does not fit the LDS beside the rows, and a 256-thread launch (L <= 24) runs out of LDS for its K rows first)
// so only these combinations are instantiated.  X(NACC, TLDS, NT, KT, DIRECT); the dispatch of tu_pair.hip and
// pair_block_t_listed / pair_block_a_listed below are all made from these two lists.
#define MMSBM_PAIR_BLOCK_T_LIST(X)                                                                                     \
  X(1, false, 256, 2, false) X(1, false, 512, 2, false)                                                                \
  X(1, false, 256, 4, true) X(1, false, 512, 4, true) X(1, true, 256, 4, true) X(1, true, 512, 4, true)                \
  X(2, false, 256, 4, true) X(2, false, 512, 4, true) X(2, true, 256, 4, true) X(2, true, 512, 4, true)                \
  X(4, false, 512, 4, true)
// ... and of the A launch (GATHER on, DO_S off: no slots, NACC = 1 and KT = 4 always)
#define MMSBM_PAIR_BLOCK_A_LIST(X)                                                                                     \
  X(1, false, 256, 4, false) X(1, false, 512, 4, false)                                                                \
  X(1, false, 256, 4, true) X(1, false, 512, 4, true) X(1, true, 256, 4, true) X(1, true, 512, 4, true)

// one integer per (NACC, TLDS, NT, KT, DIRECT): what the dispatch switches on
constexpr int pair_block_key(int nacc, bool tlds, int nt, int kt, bool direct) {
  return nacc | (kt << 4) | (tlds ? 1 << 8 : 0) | (direct ? 1 << 9 : 0) | (nt << 10);
}
#define MMSBM_PB_LISTED(N, TL, NT, KT, D) case pair_block_key(N, TL, NT, KT, D):
inline bool pair_block_t_listed(int key) {
  switch (key) { MMSBM_PAIR_BLOCK_T_LIST(MMSBM_PB_LISTED) return true; default: return false; }
}
inline bool pair_block_a_listed(int key) {
  switch (key) { MMSBM_PAIR_BLOCK_A_LIST(MMSBM_PB_LISTED) return true; default: return false; }
}
#undef MMSBM_PB_LISTED

// The kernels of one launch of the stage: the wide-row kernels, lane-per-pair pair_block_kernel, pair_quad_a_kernel (A
// launch only), pair_mfma_kernel, or the blocked mfma_rows_kernel (+ mfma_slab_kernel in the T + S launch)
enum class PairForm { Wide, Block, Quad, Mfma, MfmaBig };

struct PairPlan {
  int kp = 0, lp = 0;  // the padded shape the plan is for
  // ---- the lane-per-pair form (pair_block_kernel), both launches ----
  int threads_t = kBlock, threads_a = kBlock;  // workgroup sizes (T + S launch, A launch)
  int kt = 4;                                  // S phase: k-rows per register tile (2 when K x L is small)
  int spb = kBlock, nacc = 1, nsub = 1;        // S phase: threads per slot-grid copy, slots per thread, copies
  bool tl_t = false, tl_a = false;             // rating tile staged in LDS (T + S launch / A launch)
  size_t lds_t = 0, lds_a = 0;
  bool direct_out = false;  // output rows stored straight from registers (no LDS transpose)
  // ---- the other forms ----
  bool wide = false;      // K, L beyond the LDS stage: wide_matvec / wide_slab kernels (any size)
  bool mfma = false;      // both launches run pair_mfma_kernel (tiles beyond the scalar cache, K, L <= 64)
  bool mfma_big = false;  // K or L beyond 64, skinny tiles: the blocked forms (mfma_rows_kernel + mfma_slab_kernel)
  bool quad_a = false;    // the A launch runs pair_quad_a_kernel (long rows)
  size_t lds_mt = 0, lds_ma = 0, lds_qa = 0;  // LDS of pair_mfma_kernel (T + S, A) and of pair_quad_a_kernel
  int chunk_pairs = mmsbm::kMvChunkPairs;     // pairs per workgroup of the stage at most (the unit list is cut to it)

  bool big_tile() const { return tile_beyond_scalar_cache(kp, lp); }
  // (`mfma` is never set while `wide` is: both writers go through here, and `wide` is decided first)
  bool mfma_possible() const {
    return !wide && kp <= kMfmaMaxDim && lp <= kMfmaMaxDim && lds_mt <= kLdsMax && lds_ma <= kLdsMax;
  }
  // The A launch as pair_quad_a_kernel: the tile in LDS, 512-thread workgroups, four units' rows and the tile inside the LDS
  bool quad_possible() const {
    return !wide && big_tile() && tl_a && threads_a == kPairBlockMax && lds_qa <= kLdsMax - 2048 && lp <= kQuadMaxL;
  }
  // The stage runs on the matrix cores (`mfma_big` may be set while `wide` is, and then takes wide shapes too)
  bool on_mfma() const { return mfma || mfma_big; }
  // The plan's share of "the two-launch iteration exists for this shape" (fused_small.hpp): rows of up to 24 groups --
  // beyond that the four-launch stage runs 512-thread workgroups, whose split of a unit's pairs among the copies of the
  // slab grid (hence the association order of S) 256 threads cannot mirror
  bool two_shape_ok() const {
    return threads_t == kBlock && threads_a == kBlock && !tl_t && !tl_a && nacc == 1 && kt == 2 && spb * nsub <= kBlock &&
           !wide && !mfma && !mfma_big && !direct_out && chunk_pairs == mmsbm::kMvChunkPairs &&
           pairs_fused_lds(kp, lp) <= kLdsBudget;
  }
  // The plan's share of "the triple passes and the T + S stage run as one launch" (pass_dense.hpp): the T + S launch is
  // pair_block_kernel<false, true, 1, false, 256, 2, false> over single units -- small tile through scalar loads, one
  // slot per thread, 256 threads (so rows of up to 24 groups: three double2 of eta rows per thread).  The pair units
  // compute their A rows themselves in the multiply-add order of pair_block_kernel's A mode (the same for 256 and 512
  // threads, tile in scalar loads or in LDS), so the A launch, which still fills the table for the user pass, must be that
  // kernel too: it is for every small tile, and the condition says so
  bool pass_dense_shape_ok() const {
    return form_t() == PairForm::Block && form_a() == PairForm::Block && threads_t == kBlock && !tl_t && nacc == 1 && kt == 2 && spb * nsub <= kBlock &&
           !direct_out && chunk_pairs == mmsbm::kMvChunkPairs && kUnitPairs * lp <= 3 * 2 * kBlock && pass_dense_lds(kp, lp) <= kLdsBudget;
  }

  // ---- which kernel the plan selects ----
  PairForm form_t() const {
    return mfma_big ? PairForm::MfmaBig : mfma ? PairForm::Mfma : wide ? PairForm::Wide : PairForm::Block;
  }
  PairForm form_a() const { return (!on_mfma() && !wide && quad_a) ? PairForm::Quad : form_t(); }
  int key_t() const { return pair_block_key(nacc, tl_t, threads_t, kt, direct_out); }
  int key_a() const { return pair_block_key(1, tl_a, threads_a, 4, direct_out); }
  // pair_quad_a_kernel<NL>: double2 per thread and chunk for input rows of lp (15 or 16 spill at 256 registers: kQuadMaxL)
  int quad_nl() const {
    const int nl = (lp + 3) / 4;
    return nl <= 8 ? 8 : nl <= 10 ? 10 : nl <= 12 ? 12 : nl <= 13 ? 13 : 14;
  }

  // ---- the option transitions ----
  // Option "mfma": 0 off, 1 on (one-block form if possible, else the blocked form), 2 the blocked form whatever the shape,
  // wide shapes included.  The A launch's own runs (a_chunks) are not rebuilt: they serve whenever `mfma` is on again.
  void set_mfma(double value) {
    mfma = value == 1.0 && mfma_possible();
    mfma_big = value != 0.0 && !mfma && chunk_pairs <= kMfmaChunkPairs;
  }
  // Option "quad": on wherever quad_possible holds -- also where plan_pair_forms left it off because the chunk is not four units.
  void set_quad(bool on) { quad_a = on && quad_possible(); }
};

// The geometry of the lane-per-pair form, and whether the shape has outgrown it: arithmetic on kp and lp only.
// `wide` is decided here, once, from the shape and force_wide (MMSBM_HIP_FORCE_WIDE): no option changes it.
inline PairPlan plan_pair_shape(int kp, int lp, bool force_wide) {
  PairPlan p;
  p.kp = kp; p.lp = lp;
  // four waves share the chunks of 4 outputs of a short row; long rows get up to 8 waves
  // (measured: 320 threads do not beat 256 at L = 20, 512 beat 256 by 15 % at L = 50)
  auto threads_for = [](int nch) { return nch <= 6 ? kBlock : kPairBlockMax; };
  p.threads_t = threads_for(lp / 4);
  p.threads_a = threads_for(kp / 4);
  const int nthr = p.threads_t;
  p.kt = ((kp / 2) * (lp / 4) <= kBlock / 2) ? 2 : 4;
  const int nslot = (kp / p.kt) * (lp / 4);
  if (nslot <= nthr / 2) {
    p.spb = nslot; p.nacc = 1;
    const int room = (kp * (kUnitPairs + 1) + kUnitPairs * lp) / (nslot * 4 * p.kt);  // hand-over area
    p.nsub = std::max(1, std::min(std::min(nthr / nslot, 8), 1 + room));
  } else {
    p.spb = nthr;
    int n = 1;
    while (n * nthr < nslot) n *= 2;
    p.nacc = n;
  }
  // the rating tile sits in LDS when it is too big for the scalar cache -- unless that does not fit beside the rows:
  // then it is read through scalar loads after all (slower, but it runs)
  p.tl_t = tile_in_lds(kp, lp);
  p.tl_a = tile_in_lds(lp, kp);
  p.lds_t = pair_block_lds(kp, lp, p.tl_t);
  p.lds_a = pair_block_lds(lp, kp, p.tl_a);
  if (p.lds_t > kLdsMax) { p.tl_t = false; p.lds_t = pair_block_lds(kp, lp, false); }
  if (p.lds_a > kLdsMax) { p.tl_a = false; p.lds_a = pair_block_lds(lp, kp, false); }
  // still too large for the 64-pair LDS stage (roughly K + L > 300): the plain wide-row kernels
  p.wide = p.lds_t > kLdsMax || p.lds_a > kLdsMax || p.nacc > 4 || force_wide;
  return p;
}

// Which form the shape gets and how many pairs a workgroup of it takes, from the plan of plan_pair_shape, the number of
// pairs, the device's CU count and the knobs no_mfma (MMSBM_HIP_NO_MFMA) and mfma_chunk (MMSBM_HIP_MFMA_CHUNK; 0: not set)
inline PairPlan plan_pair_forms(PairPlan p, int n_pairs, int n_cus, bool no_mfma, int mfma_chunk) {
  const bool big_tile = p.big_tile();
  // both launches on the matrix cores where the tile has left the scalar cache (pair_mfma_kernel)
  p.lds_mt = pair_mfma_lds(p.kp, p.lp, true);
  p.lds_ma = pair_mfma_lds(p.lp, p.kp, false);
  p.mfma = p.mfma_possible() && big_tile && !no_mfma;
  // K or L beyond 64: the blocked matrix-core kernels take over from the lane-per-pair stage with its tile in
  // scalar loads and from the wide-row kernels
  // Skinny tiles too (a side below 16 groups, e.g. 600 x 5 or 3 x 1,024): three quarters of a 16-wide tile are
  // padding there, and it is still several times faster than the alternatives -- the wide-row kernels have one
  // thread per output column (8 of 256 threads busy at L = 5), the lane-per-pair stage streams a 38 KB tile
  // through the scalar cache.  1M ratings, T+S / A launch: 600 x 5 2,336 / 124 -> 380 / 115 us, 1,024 x 3
  // 5,822 / 152 -> 621 / 171, 8 x 520 471 / 927 -> 247 / 191, 3 x 1,024 470 / 3,219 -> 430 / 346, 300 x 8
  // 310 / 91 -> 197 / 53 (scripts/skinny_time.py, round 3).
  p.mfma_big = !p.mfma && big_tile && !no_mfma;
  // big K x L tiles: four 64-pair units per pair_block workgroup (4x fewer slabs to write + add); on the matrix cores
  // eight -- only for `mfma`, and only while that still leaves every CU a few rounds of workgroups (C5: T+S 358 -> 342
  // us, half the slabs for eta_p: 123 -> 111 us; 768 or 1,024 pairs per workgroup are slower).  mfma_chunk overrides it.
  int big_chunk = 4 * mmsbm::kMvChunkPairs;
  if (p.mfma && n_pairs >= 2 * big_chunk * 4 * n_cus) big_chunk *= 2;
  if (mfma_chunk > 0) big_chunk = mfma_chunk;
  p.chunk_pairs = p.wide ? kWideChunkPairs : (big_tile ? big_chunk : mmsbm::kMvChunkPairs);
  // long rows: the mat-vec's outputs go to memory straight from registers (C5: -6 % on both
  // pair_block launches); short rows are cheaper transposed through LDS and copied out flat
  // (C3: direct stores cost +1.1 / +1.7 us)
  p.direct_out = big_tile;
  // ... and the A launch as a persistent four-unit pipeline where the tile sits in LDS and
  // everything fits (C5: 312 -> 259 us)
  p.lds_qa = (static_cast<size_t>(kQuadUnits) * p.lp * (kUnitPairs + 1) + static_cast<size_t>(p.lp) * p.kp) * sizeof(double);
  p.quad_a = p.quad_possible() && big_chunk == 4 * mmsbm::kMvChunkPairs;
  return p;
}

}  // namespace mmsbm_hip_impl
