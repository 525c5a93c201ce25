// tu_pair.hip -- translation unit of the pair stage on the vector ALUs: pair_block_kernel (T + S launch, A launch;
// pair_block.hpp), pair_quad_a_kernel and the wide-row kernels (pair_quad.hpp), with the host code that chooses among them
#include "prelude.hpp"
#include "pair_block.hpp"
#include "pair_quad.hpp"

namespace mmsbm_hip_impl {

// Both launches dispatch on the plan (pair_plan.hpp): its form, and for pair_block_kernel the instantiation key, one case
// per entry of the plan header's lists -- which are therefore the instantiations this unit compiles.
void stage_dense_valu(mmsbm_hip_ctx *c) {  // T = P^T C  and the K x L slabs for p
  const PairPlan &pp = c->pp;
  const int nb = static_cast<int>(c->lay.mv_chunks.size());
  const PairBlockArgs pa = pair_block_t_args(c);
  if (pp.form_t() == PairForm::Wide) {
    LaunchScope ls(c, K_DENSE);
    const int subs = kWideChunkPairs / kWidePairs;
    const int kgs = (c->kp + kWideKG - 1) / kWideKG, lbs = (c->lp + kBlock - 1) / kBlock;
    const size_t lds = wide_matvec_lds(c->kp);
    allow_big_lds(wide_matvec_kernel<false>, lds);
    LAUNCH((wide_matvec_kernel<false>), slot_grid(c, nb * subs), kBlock, lds, c->stream, pa, subs);
    LAUNCH(wide_slab_kernel, slot_grid(c, nb * kgs * lbs), kBlock, 0, c->stream, pa, kgs, lbs);
    ls.done();
    return;
  }
  LaunchScope ls(c, K_DENSE, true);
#define PB_CASE(N, TL, NT, KT, D)                                                           \
  case pair_block_key(N, TL, NT, KT, D):                                                    \
    allow_big_lds(pair_block_kernel<false, true, N, TL, NT, KT, D>, pp.lds_t);              \
    LAUNCH_IN(ls, (pair_block_kernel<false, true, N, TL, NT, KT, D>), slot_grid(c, nb), NT, pp.lds_t, c->stream, pa, pa.tiles); \
    break;
  switch (pp.key_t()) {
    MMSBM_PAIR_BLOCK_T_LIST(PB_CASE)
    default: throw ApiError(MMSBM_E_INTERNAL, "pair_block (T + S): no such instantiation");
  }
#undef PB_CASE
  ls.done();
}

void stage_matvec_a_valu(mmsbm_hip_ctx *c, int slot, int a_slot, bool grid) {
  const PairPlan &pp = c->pp;
  int nb = 0;
  const PairBlockArgs pa = matvec_a_args(c, slot, a_slot, grid, &nb);
  if (nb == 0) return;
  LaunchScope ls(c, K_MATVEC_A, true);
  bool found = true;
  switch (pp.form_a()) {
    case PairForm::Wide: {
      const int subs = kWideChunkPairs / kWidePairs;
      const size_t lds = wide_matvec_lds(c->lp);
      allow_big_lds(wide_matvec_kernel<true>, lds);
      LAUNCH_IN(ls, (wide_matvec_kernel<true>), slot_grid(c, nb * subs), kBlock, lds, c->stream, pa, subs);
      break;
    }
    case PairForm::Quad: {
      const dim3 grid_q = slot_grid(c, std::min(nb, c->n_cus));
#define QA_CASE(NL)                                                                               \
  case NL:                                                                                        \
    allow_big_lds(pair_quad_a_kernel<NL>, pp.lds_qa);                                             \
    LAUNCH_IN(ls, (pair_quad_a_kernel<NL>), grid_q, kPairBlockMax, pp.lds_qa, c->stream, pa, pa.tiles, nb); \
    break;
      switch (pp.quad_nl()) {
        QA_CASE(8) QA_CASE(10) QA_CASE(12) QA_CASE(13) QA_CASE(14)   // (every value of quad_nl)
      }
#undef QA_CASE
      break;
    }
    case PairForm::Block:
#define PA_CASE(N, TL, NT, KT, D)                                                           \
  case pair_block_key(N, TL, NT, KT, D):                                                    \
    allow_big_lds(pair_block_kernel<true, false, N, TL, NT, KT, D>, pp.lds_a);              \
    LAUNCH_IN(ls, (pair_block_kernel<true, false, N, TL, NT, KT, D>), slot_grid(c, nb), NT, pp.lds_a, c->stream, pa, pa.tiles); \
    break;
      switch (pp.key_a()) {
        MMSBM_PAIR_BLOCK_A_LIST(PA_CASE)
        default: found = false;
      }
#undef PA_CASE
      break;
    default: found = false;  // (the matrix-core forms: tu_mfma.hip)
  }
  if (!found) throw ApiError(MMSBM_E_INTERNAL, "pair stage (A): no such instantiation");
  ls.done();
}

}  // namespace mmsbm_hip_impl
