// Host-only check of mmsbm_amd/csrc/pair_plan.hpp, built with -fsanitize=address,undefined by
// tests/test_pair_plan_cpu.py.  Builds the pair stage's launch plan for every padded shape of K, L = 1 .. 1,199, under
// every creation knob and option sequence, and checks the rules that tie the plan's fields together -- among them that
// the pair_block_kernel instantiation a plan selects is on the list tu_pair.hip's dispatch is made from.
#include <cstddef>
#include <cstdio>
#include <set>
#include <vector>

#include "../../mmsbm_amd/csrc/layout.hpp"
#include "../../mmsbm_amd/csrc/shapes.hpp"
#include "../../mmsbm_amd/csrc/pair_plan.hpp"

using namespace mmsbm_hip_impl;

static long fails = 0;
static int g_kp = 0, g_lp = 0, g_knob = 0, g_seq = 0;
#define CHECK(x)                                                                                                       \
  do {                                                                                                                 \
    if (!(x) && ++fails <= 20)                                                                                         \
      std::printf("FAILED %s (kp %d, lp %d, knob %d, sequence %d) line %d\n", #x, g_kp, g_lp, g_knob, g_seq, __LINE__); \
  } while (0)

static void apply_sequence(PairPlan &p, int seq) {
  switch (seq) {
    case 1: p.set_mfma(0); break;
    case 2: p.set_mfma(2); break;
    case 3: p.set_mfma(0); p.set_mfma(1); break;
    case 4: p.set_quad(false); break;
    case 5: p.set_quad(true); break;
    default: break;
  }
}

static void check_block_geometry(const PairPlan &p) {  // the lane-per-pair form: what pair_block_kernel is compiled for
  const bool big = tile_beyond_scalar_cache(p.kp, p.lp);
  CHECK((p.kt == 4) == p.direct_out && p.direct_out == big);
  CHECK((!p.tl_t && !p.tl_a) || p.direct_out);
  CHECK(p.nacc == 1 || p.nacc == 2 || p.nacc == 4);
  CHECK(p.nacc != 4 || (p.threads_t == kPairBlockMax && !p.tl_t));
  CHECK(p.threads_t == kBlock || p.threads_t == kPairBlockMax);
  CHECK(p.threads_a == kBlock || p.threads_a == kPairBlockMax);
}

static void check_plan(const PairPlan &p) {
  const PairForm ft = p.form_t(), fa = p.form_a();
  CHECK(!p.mfma || (!p.wide && p.kp <= kMfmaMaxDim && p.lp <= kMfmaMaxDim));
  CHECK(!(p.mfma && p.mfma_big));
  CHECK(!p.quad_a || (p.lp <= kQuadMaxL && p.lds_qa <= kLdsMax - 2048));
  CHECK(!p.on_mfma() || p.chunk_pairs <= kMfmaChunkPairs);
  CHECK(p.chunk_pairs >= kUnitPairs && p.chunk_pairs % kUnitPairs == 0);
  switch (ft) {
    case PairForm::Block:
      check_block_geometry(p);
      CHECK(pair_block_t_listed(p.key_t()));
      CHECK(p.lds_t <= kLdsMax);
      break;
    case PairForm::Wide: CHECK(p.wide && wide_matvec_lds(p.kp) <= kLdsMax); break;
    case PairForm::Mfma: CHECK(p.mfma && p.lds_mt <= kLdsMax); break;
    case PairForm::MfmaBig: CHECK(p.mfma_big && kMfmaRowsLds <= kLdsMax && kMfmaSlabLds <= kLdsMax); break;
    default: CHECK(!"a T + S form");
  }
  switch (fa) {
    case PairForm::Block:
      check_block_geometry(p);
      CHECK(pair_block_a_listed(p.key_a()));
      CHECK(p.lds_a <= kLdsMax);
      break;
    case PairForm::Quad: {
      check_block_geometry(p);
      const int nl = p.quad_nl();
      CHECK(p.quad_a && ft == PairForm::Block && p.lds_qa <= kLdsMax);
      CHECK((nl == 8 || nl == 10 || nl == 12 || nl == 13 || nl == 14) && 4 * nl >= p.lp);
      break;
    }
    case PairForm::Wide: CHECK(ft == PairForm::Wide && wide_matvec_lds(p.lp) <= kLdsMax); break;
    case PairForm::Mfma: CHECK(ft == PairForm::Mfma && p.lds_ma <= kLdsMax); break;
    case PairForm::MfmaBig: CHECK(ft == PairForm::MfmaBig); break;
  }
  CHECK(!p.two_shape_ok() || (ft == PairForm::Block && fa == PairForm::Block && !p.direct_out));
}

int main() {
  std::set<int> padded;
  for (int d = 1; d <= 1199; ++d) padded.insert(pad_dim(d));
  const std::vector<int> dims(padded.begin(), padded.end());
  const int n_cus = 256;
  // the chunk doubles at 2 * (4 * kMvChunkPairs) * 4 * n_cus pairs; twice that as well
  const int doubling = 2 * 4 * mmsbm::kMvChunkPairs * 4 * n_cus;
  const int pair_counts[4] = {doubling - 1, doubling, 2 * doubling - 1, 2 * doubling};
  long shapes = 0, plans = 0, n_wide = 0, n_big = 0, n_mfma = 0, n_block = 0;
  for (int kp : dims)
    for (int lp : dims) {
      g_kp = kp; g_lp = lp;
      ++shapes;
      for (int knob = 0; knob < 3; ++knob) {  // none, no_mfma, force_wide
        g_knob = knob;
        const PairPlan shape = plan_pair_shape(kp, lp, knob == 2);
        for (int n_pairs : pair_counts) {
          const PairPlan made = plan_pair_forms(shape, n_pairs, n_cus, knob == 1, 0);
          CHECK(made.wide == shape.wide && (knob != 2 || made.wide));
          CHECK(knob != 1 || !made.on_mfma());
          CHECK(!made.mfma || made.chunk_pairs == (n_pairs >= doubling ? 512 : 256));
          CHECK(made.mfma || made.chunk_pairs == (made.wide ? kWideChunkPairs : made.big_tile() ? 256 : mmsbm::kMvChunkPairs));
          if (knob == 0 && n_pairs == pair_counts[0]) {
            const PairForm f = made.form_t();   // (wide shapes apart: the blocked matrix-core form takes them too)
            if (made.wide) ++n_wide;
            else if (f == PairForm::MfmaBig) ++n_big;
            else if (f == PairForm::Mfma) ++n_mfma;
            else ++n_block;
          }
          for (int seq = 0; seq < 6; ++seq) {
            g_seq = seq;
            PairPlan p = made;
            apply_sequence(p, seq);
            CHECK(p.wide == made.wide && p.chunk_pairs == made.chunk_pairs);   // no option changes either
            CHECK(seq != 1 || !p.on_mfma());
            CHECK(seq != 2 || (p.mfma_big && !p.mfma));
            CHECK(seq != 3 || p.on_mfma());
            CHECK(seq != 4 || !p.quad_a);
            CHECK(seq != 5 || p.quad_a == p.quad_possible());
            check_plan(p);
            ++plans;
          }
        }
      }
    }
  // the library's own choice over the default shapes, as counted from the rules before they moved into pair_plan.hpp
  std::printf("shapes %ld, plans %ld; default plans: wide %ld, blocked mfma %ld, mfma %ld, block %ld\n", shapes, plans,
              n_wide, n_big, n_mfma, n_block);
  if (n_wide != 15001 || n_big != 2561 || n_mfma != 114 || n_block != 280) { std::printf("FAILED: the default plans' counts\n"); ++fails; }
  if (dims.size() != 134 || shapes != 17956) { std::printf("FAILED: %zu padded values, %ld shapes\n", dims.size(), shapes); ++fails; }
  if (fails) { std::printf("pair plan check: %ld failure(s)\n", fails); return 1; }
  std::printf("pair plan check: ok\n");
  return 0;
}
