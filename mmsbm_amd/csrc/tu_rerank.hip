// tu_rerank.hip -- translation unit of the queries of the recommend session that add a stage of their own to the frame of
// serve_frame.hpp: another tile kernel in front of the exclusions, a stage over the batch buffer behind them, or a stage
// over the selected pool
//   explore.hpp    randomised top-N with propensities: the batch buffer moved to a second one and perturbed with Gumbel
//                  noise from a counter-based PCG64 stream, the same selection over the keys, then each position's
//                  probability from the unperturbed scores; the propensities of given lists
//   ensemble.hpp   ensemble-aware queries: the restarts' scores reduced per pair (min, max, mean - risk std), then the
//                  same selection; the spread of given pairs
//   group.hpp      group queries: the members' score tiles reduced per group, then the same selection
//   diverse.hpp    diversified top-N: the pool kept on the device, then a greedy kernel; reads the similarity session; the
//                  distance of given pairs of that session
// (recommend.hpp and top_pairs.hpp: the device helpers these kernels share -- the tile accumulation, the sorted list; the
// smallest accumulator at or above a bar, gtop_floor_acc.  Nothing of theirs is launched here.)
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "top_pairs.hpp"
#include "explore.hpp"
#include "ensemble.hpp"
#include "group.hpp"
#include "diverse.hpp"

namespace mmsbm_hip_impl {

// ---- randomised top-N with propensities (explore.hpp) ---------------------------------------------------------------------
namespace {

// The PCG64 stream of a call: its four words and the jump table on the device (the host copy is held: the upload is
// asynchronous)
struct ExploreStream {
  uint64_t st[4];
  std::vector<uint64_t> tab_h;
  DevBuf<uint64_t> tab;
  ExploreStream(const uint64_t state[4], hipStream_t stream) : tab_h(64 * 4) {
    std::copy(state, state + 4, st);
    explore_jump_table(st, tab_h.data());
    tab.upload(tab_h, stream);
  }
};

}  // namespace

// recommend_query_within's batches with two stages of its own around the unchanged selection: behind the exclusions the
// row maxima and the perturbation (the scores move to `raw`, the keys take their place), behind the selection the
// propensities from `raw` -- per batch, before the next one overwrites it (top_n_device's `each`).
void recommend_query_explore(mmsbm_hip_ctx *c, const UserQuery &q, int n, double temperature, const uint64_t state[4],
                             const TopNOut &out, double *propensity) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int64_t n_users = q.users.n;
  top_n_blank(n_users, n, out);
  const size_t outs = static_cast<size_t>(n_users) * n;
  for (size_t e = 0; propensity && e < outs; ++e) propensity[e] = 0.0;
  c->last_ms[T_RECOMMEND] = 0.f;
  const int C = q.cand.columns(rc.items);
  if (C == 0 || n_users == 0) return;  // (no column to score: every row is empty)
  hipStream_t st = c->stream;
  const int64_t bu = rec_batch_users(C, n_users);  // (the batches top_n_device will form)
  const size_t ld = static_cast<size_t>(C);
  require_free_mem(static_cast<size_t>(bu) * ld * sizeof(double) + static_cast<size_t>(bu) * 24 + outs * 16 + 2048,
                   "recommend_explore: the unperturbed scores of a batch of users");
  ExploreStream rng(state, st);
  DevBuf<double> raw, mx, ps, pp;
  DevBuf<uint64_t> base;
  raw.alloc(static_cast<size_t>(bu) * ld);
  mx.alloc(static_cast<size_t>(bu));
  base.alloc(static_cast<size_t>(bu) * 2);
  ps.alloc(outs);
  pp.alloc(outs);
  const unsigned spans = static_cast<unsigned>((C + kExpSpan - 1) / kExpSpan);
  rec_within_device(
      c, q, rc.seen_lists(), n, 0, rec_tiles(c, rc.x.ptr, rc.x_stride()),
      [&](const TopNDev &dev, EventPair &ev, const int32_t *, float prep_ms) {  // the scores are `raw`'s, not the keys
        top_n_copy_out(c, TopNDev{ps.ptr, dev.oi, dev.on}, ev, n_users, n, T_RECOMMEND, out, q.cand.items, pp.ptr, propensity);
        c->last_ms[T_RECOMMEND] += prep_ms;
      },
      [&](const WithinPrep &w, const int32_t *ub, int nb, double *sc) {
        LAUNCH(explore_norm_kernel, nb, kBlock, 0, st, sc, ld, C, ub, rng.tab.ptr, rng.st[0], rng.st[1], mx.ptr, base.ptr);
        LAUNCH(explore_perturb_kernel, dim3(spans, static_cast<unsigned>(nb)), kBlock, 0, st, sc, raw.ptr, ld, C, w.dcand(),
               rng.tab.ptr, base.ptr, rng.st[2], rng.st[3], temperature);
      },
      [&](const TopNDev &batch, int nb, int64_t b0) {
        LAUNCH(explore_finish_kernel, nb, kRecWave, 0, st, raw.ptr, ld, C, mx.ptr, temperature, batch.oi, batch.on, n,
               ps.ptr + b0 * n, pp.ptr + b0 * n);
      });
}

// The propensities of caller-given lists: recommend_query_within's score tiles and exclusions per batch (within_fill),
// the row maxima, then explore_list_kernel over the batch buffer itself -- no noise, no selection.
void recommend_list_propensity(mmsbm_hip_ctx *c, const UserQuery &q, double temperature, const RowCsr &asked, double *scores,
                               double *propensity) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int64_t n_users = q.users.n;
  const size_t total = static_cast<size_t>(DevCsr::entries(asked, n_users));  // (checked: below 2^31)
  for (size_t e = 0; e < total; ++e) {
    if (scores) scores[e] = -INFINITY;
    propensity[e] = 0.0;
  }
  c->last_ms[T_RECOMMEND] = 0.f;
  const int C = q.cand.columns(rc.items);
  if (C == 0 || total == 0) return;  // (no candidate anywhere, or nothing asked)
  hipStream_t st = c->stream;
  WithinPrep w;
  within_prepare(c, q, w);
  BatchFrame fr(C, n_users);
  const size_t ld = static_cast<size_t>(C);
  require_free_mem(fr.bytes() + static_cast<size_t>(fr.bu) * 8 + (static_cast<size_t>(n_users) + 1) * 4 + total * 20,
                   "recommend_list_propensity: a batch of users and the lists");
  DevBuf<double> mx, os, op;
  DevCsr lists;
  mx.alloc(static_cast<size_t>(fr.bu));
  os.alloc(total);
  op.alloc(total);
  lists.upload(asked, n_users, st);
  const auto tiles = rec_tiles(c, rc.x.ptr, rc.x_stride());
  const int32_t *col_of = w.has_cand ? w.ct.col.ptr : nullptr;
  fr.run(st, q.users.ids, [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
    within_fill(c, w, tiles, rc.seen_lists(), ub, nb, b0, sc);
    LAUNCH(explore_norm_kernel, nb, kBlock, 0, st, sc, ld, C, ub, nullptr, uint64_t(0), uint64_t(0), mx.ptr, nullptr);
    LAUNCH(explore_list_kernel, nb, kRecWave, 0, st, sc, ld, C, mx.ptr, temperature, lists.off.ptr + b0, lists.val.ptr, col_of,
           os.ptr, op.ptr);
  });
  if (scores) HIP_CHECK(hipMemcpyAsync(scores, os.ptr, sizeof(double) * total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(propensity, op.ptr, sizeof(double) * total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_RECOMMEND] = fr.ev.ms() + w.ct.ms;
}

void explore_noise(mmsbm_hip_ctx *c, const uint64_t state[4], int64_t n_pairs, const int32_t *users, const int32_t *items,
                   double *r, double *g) {
  use_device(c);
  if (n_pairs == 0) return;
  hipStream_t st = c->stream;
  const int64_t per = std::min<int64_t>(n_pairs, int64_t(1) << 24);  // pairs per launch (24 bytes each)
  require_free_mem(static_cast<size_t>(per) * 24 + 2048, "explore_noise: a batch of pairs");
  ExploreStream rng(state, st);
  DevBuf<int32_t> du, di;
  DevBuf<double> dr, dg;
  du.alloc(static_cast<size_t>(per));
  di.alloc(static_cast<size_t>(per));
  dr.alloc(static_cast<size_t>(per));
  dg.alloc(static_cast<size_t>(per));
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(du.ptr, users + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(di.ptr, items + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    LAUNCH(explore_noise_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, rng.tab.ptr, rng.st[0],
           rng.st[1], rng.st[2], rng.st[3], du.ptr, di.ptr, np, dr.ptr, dg.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(r + p0, dr.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(g + p0, dg.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
}

// ---- ensemble-aware queries (ensemble.hpp) ------------------------------------------------------------------------------
// rec_run_within with the score tile replaced by the aggregate over the restarts (rec_within_run: the same candidate
// table, the same exclusions, the same batches and selection)
void recommend_query_ensemble(mmsbm_hip_ctx *c, const UserQuery &q, int mode, double risk, int n, const TopNOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(q.users.n, n, out);
  rec_within_run(c, q, rc.seen_lists(), n,
                 [&](const double *y, size_t ys, int C, const int32_t *ub, int nb, double *sc) {
                   auto tile = [&](auto kernel) {
                     LAUNCH(kernel, tile_grid(C, nb, kEnsTile), kBlock, 0, c->stream, rc.x.ptr, rc.x_stride(), y, ys, ub, nb, C, rc.rank, rc.slots, risk, sc,
                            static_cast<size_t>(C));
                   };
                   if (mode == MMSBM_HIP_ENSEMBLE_MIN) tile(ens_tile_kernel<kEnsMin>);
                   else if (mode == MMSBM_HIP_ENSEMBLE_MAX) tile(ens_tile_kernel<kEnsMax>);
                   else tile(ens_tile_kernel<kEnsLcb>);
                 },
                 T_ENSEMBLE, out);
}

void recommend_pair_spread(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *users, const int32_t *items, double *stats,
                           double *per_slot) {
  use_device(c);
  const RecSession &rc = *c->rc;
  c->last_ms[T_ENSEMBLE] = 0.f;
  if (n_pairs == 0) return;
  const int S = rc.slots;
  hipStream_t st = c->stream;
  const int64_t per = ens_pairs_per_launch(n_pairs, S, per_slot != nullptr);
  require_free_mem(static_cast<size_t>(per) * ens_pair_bytes(S, per_slot != nullptr), "recommend_pair_spread: a batch of pairs");
  DevBuf<int32_t> du, di;
  DevBuf<double> ds, dp;
  du.alloc(static_cast<size_t>(per));
  di.alloc(static_cast<size_t>(per));
  ds.alloc(static_cast<size_t>(per) * 4);
  if (per_slot) dp.alloc(static_cast<size_t>(per) * S);
  float ms = 0.f;  // device time of the call's kernels (option "ensemble_ms")
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(du.ptr, users + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(di.ptr, items + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    EventPair ev;
    ev.start(st);
    LAUNCH(ens_pairs_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, rc.x_stride(),
           rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.rank, S, du.ptr, di.ptr, np, ds.ptr, dp.ptr);
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(stats + p0 * 4, ds.ptr, sizeof(double) * np * 4, hipMemcpyDeviceToHost, st));
    for (int s = 0; s < S && per_slot; ++s)  // the batch's [S][np] into the caller's [S][n_pairs]
      HIP_CHECK(hipMemcpyAsync(per_slot + static_cast<size_t>(s) * n_pairs + p0, dp.ptr + static_cast<size_t>(s) * np,
                               sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  c->last_ms[T_ENSEMBLE] = ms;
}

// ---- group queries (group.hpp) ------------------------------------------------------------------------------------------
// plan (plan_groups: the member blocks, the batches' runs and fragments), memory check, uploads, top_n_run, scatter
void recommend_query_groups(mmsbm_hip_ctx *c, int64_t n_groups, const RowCsr &members, int mode, double bar,
                            const Subset &sub, int n, const TopNOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int32_t *cand = sub.items;  // (null: the columns are the items)
  top_n_blank(n_groups, n, out);
  c->last_ms[T_GROUP] = 0.f;
  const int NI = rc.items, rank = rc.rank, S = rc.slots;
  const int C = sub.columns(NI);
  const bool tiles = mode != MMSBM_HIP_GROUP_MEAN;
  const GroupPlan p = plan_groups(members.offsets, members.values, n_groups, C, c->n_cus, c->grp_run, tiles);
  const int64_t G = p.groups();
  if (G == 0 || C == 0) return;  // (no row or no column to score: every row is empty)
  if (p.too_large())
    throw ApiError(MMSBM_E_TOOLARGE, "recommend_query_groups: " + std::to_string(p.n_blocks) + " blocks of member rows in one query");
  const size_t ycs = static_cast<size_t>(C) * rank, bs = static_cast<size_t>(G) * rank;
  require_free_mem(CatTable::bytes(rc, sub) +
                       (p.rows.size() + 3 * p.info.size() + p.run_off.size() + 2 * p.cut_off.size() + 2 * static_cast<size_t>(G) + 1) * 4 +
                       (tiles ? static_cast<size_t>(p.most_frag) * C : S * bs) * sizeof(double),
                   "recommend_query_groups: the member rows, the groups' lists and the candidates' rows");
  hipStream_t st = c->stream;
  DevBuf<int32_t> d_rows, d_info, d_grp, d_out, d_run, d_cut_grp, d_cut_off, d_gblk, d_size;
  DevBuf<double> xbar, part;
  CatTable ct;
  d_rows.upload(p.rows, st);
  d_info.upload(p.info, st);
  d_grp.upload(p.grp, st);
  if (tiles) {
    d_out.upload(p.out, st);
    d_run.upload(p.run_off, st);
    if (p.most_frag > 0) {
      d_cut_grp.upload(p.cut_grp, st);
      d_cut_off.upload(p.cut_off, st);
      part.alloc(static_cast<size_t>(p.most_frag) * C);
    }
  } else {
    d_gblk.upload(p.gblk, st);
    d_size.upload(p.gsize, st);
    xbar.alloc(S * bs);
  }
  if (cand) cat_table(c, sub, ct);
  const double *y = cand ? ct.y.ptr : rc.y.ptr;
  const size_t ys = cand ? ycs : static_cast<size_t>(NI) * rank, xs = rc.x_stride();
  const SeenLists seen = rc.seen_lists();
  const int32_t *col_of = cand ? ct.col.ptr : nullptr;
  std::vector<int32_t> ti(static_cast<size_t>(G) * n), tc(static_cast<size_t>(G));
  std::vector<double> ts(static_cast<size_t>(G) * n);
  top_n_run(c, C, G, p.ids.data(), n, "recommend_query_groups: a batch of groups",
            [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
              const int g0 = static_cast<int>(b0);
              const unsigned it = static_cast<unsigned>(p.item_tiles);
              if (tiles) {
                const size_t k = static_cast<size_t>(b0 / p.bu);
                const dim3 g(it, static_cast<unsigned>(p.batch_run[k + 1] - p.batch_run[k]));
                const int32_t *ro = d_run.ptr + p.batch_run[k];
                const int n_cut = p.batch_cut[k + 1] - p.batch_cut[k], p0 = p.cut_off[static_cast<size_t>(p.batch_cut[k])];
                auto tile = [&](auto kernel) {
                  LAUNCH(kernel, g, kBlock, 0, st, rc.x.ptr, xs, y, ys, d_rows.ptr, d_info.ptr, d_out.ptr, ro, g0, p0, C, rank,
                         S, bar, sc, part.ptr, static_cast<size_t>(C));
                };
                if (mode == MMSBM_HIP_GROUP_MIN) tile(grp_tile_kernel<kGrpMin>);
                else if (mode == MMSBM_HIP_GROUP_MAX) tile(grp_tile_kernel<kGrpMax>);
                else tile(grp_tile_kernel<kGrpCount>);
                if (n_cut > 0)
                  LAUNCH(grp_combine_kernel, dim3(static_cast<unsigned>((C + kBlock - 1) / kBlock), static_cast<unsigned>(n_cut)),
                         kBlock, 0, st, part.ptr, d_cut_grp.ptr + p.batch_cut[k], d_cut_off.ptr + p.batch_cut[k], g0, p0, C, mode, S,
                         sc, static_cast<size_t>(C));
              } else {
                const size_t e = static_cast<size_t>(nb) * rank * S;
                LAUNCH(grp_mean_kernel, static_cast<unsigned>((e + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, xs, rank,
                       S, d_rows.ptr, d_gblk.ptr, d_size.ptr, g0, nb, xbar.ptr, bs);
                score_tiles(c, xbar.ptr, bs, y, ys, C, ub, nb, SeenLists{}, sc);
              }
              if (seen.off) {
                const int blk0 = p.gblk[static_cast<size_t>(g0)];
                LAUNCH(grp_exclude_kernel, static_cast<unsigned>(p.gblk[static_cast<size_t>(g0) + nb] - blk0), kBlock, 0, st,
                       d_rows.ptr, d_info.ptr, d_grp.ptr, blk0, g0, seen.off, seen.items, col_of, sc, static_cast<size_t>(C));
              }
            },
            T_GROUP, TopNOut{ti.data(), ts.data(), tc.data()});
  c->last_ms[T_GROUP] += ct.ms;
  for (int64_t r = 0; r < G; ++r) {  // the rows to their places in the request, columns -> item ids
    const size_t o = static_cast<size_t>(p.at[r]) * n, t = static_cast<size_t>(r) * n;
    const int cnt = tc[static_cast<size_t>(r)];
    if (out.counts) out.counts[p.at[r]] = cnt;
    for (int k = 0; k < cnt; ++k) {
      out.items[o + k] = item_of(cand, ti[t + k]);
      if (out.scores) out.scores[o + k] = ts[t + k];
    }
  }
}

// ---- diversified top-N and the distance of given pairs (diverse.hpp) --------------------------------------------------
void similar_pairs(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *a, const int32_t *b, double *distance) {
  use_device(c);
  const SimSession &sm = *c->sm;
  c->last_ms[T_DIVERSE] = 0.f;
  if (n_pairs == 0) return;
  const double denom = static_cast<double>(sm.slots) * static_cast<double>(sm.others);
  hipStream_t st = c->stream;
  const int64_t per = std::min<int64_t>(n_pairs, int64_t(1) << 24);  // pairs per launch (16 bytes each)
  require_free_mem(static_cast<size_t>(per) * 16, "similar_pairs: a batch of pairs");
  DevBuf<int32_t> da, db;
  DevBuf<double> dd;
  da.alloc(static_cast<size_t>(per));
  db.alloc(static_cast<size_t>(per));
  dd.alloc(static_cast<size_t>(per));
  float ms = 0.f;  // device time of the call's kernels (option "diverse_ms")
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(da.ptr, a + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(db.ptr, b + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    EventPair ev;
    ev.start(st);
    LAUNCH(div_pairs_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, sm.q.ptr,
           static_cast<size_t>(sm.rows) * sm.width, sm.mf.ptr, sm.width, sm.slots, denom, da.ptr, db.ptr, np, dd.ptr);
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(distance + p0, dd.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  c->last_ms[T_DIVERSE] = ms;
}

void recommend_diverse(mmsbm_hip_ctx *c, const UserQuery &q, int n, int pool, double trade_off, const TopNOut &out,
                       double *distances) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const SimSession &sm = *c->sm;
  const int64_t n_users = q.users.n;
  top_n_blank(n_users, n, out);
  for (size_t e = 0; distances && e < static_cast<size_t>(n_users) * n; ++e) distances[e] = INFINITY;
  c->last_ms[T_DIVERSE] = 0.f;
  if (q.cand.columns(rc.items) == 0 || n_users == 0) return;  // (no column to score: every row is empty)
  hipStream_t st = c->stream;
  const double denom = static_cast<double>(sm.slots) * static_cast<double>(sm.others);
  const size_t lds = (static_cast<size_t>(pool) * 21 + 7) / 8 * 8;  // score, m, id, picked flag per place
  size_t free_b = 0, total_b = 0;
  if (c->div_rows <= 0) HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const int64_t rows_per = div_rows_per_call(c->div_rows, n_users, free_b, div_row_bytes(pool, n));
  const SeenLists seen = rc.seen_lists();
  float ms = 0.f;  // device time of the query's kernels (option "diverse_ms")
  std::vector<int64_t> rebased;  // (the rows' own lists, offsets from the first of them)
  for (int64_t b0 = 0; b0 < n_users; b0 += rows_per) {
    const int64_t nb = std::min(rows_per, n_users - b0);
    const size_t outs = static_cast<size_t>(nb) * n;
    rec_within_device(
        c, q.rows(b0, nb, rebased), seen, pool, outs * 20 + static_cast<size_t>(nb) * 4, rec_tiles(c, rc.x.ptr, rc.x_stride()),
        [&](const TopNDev &dev, EventPair &ev, const int32_t *dcand, float prep_ms) {
          DevBuf<int32_t> ri, rn;
          DevBuf<double> rs, rd;
          ri.alloc(outs); rs.alloc(outs); rd.alloc(outs); rn.alloc(static_cast<size_t>(nb));
          EventPair ev2;
          ev2.start(st);
          if (dcand)  // the pool as columns of the compact table -> item ids
            LAUNCH(div_ids_kernel, static_cast<unsigned>((static_cast<size_t>(nb) * pool + kBlock - 1) / kBlock), kBlock, 0,
                   st, dcand, q.cand.n, dev.on, static_cast<int>(nb), pool, dev.oi);
          LAUNCH(div_greedy_kernel, static_cast<unsigned>(nb), kDivWave, lds, st, sm.q.ptr,
                 static_cast<size_t>(sm.rows) * sm.width, sm.mf.ptr, sm.width, sm.slots, sm.rows, denom, dev.os, dev.oi, dev.on, pool, n, trade_off, ri.ptr, rs.ptr, rd.ptr, rn.ptr);
          HIP_CHECK(hipGetLastError());
          ev2.stop(st);
          const size_t o = static_cast<size_t>(b0) * n;  // (the kernel wrote the padding too: straight into the caller's rows)
          HIP_CHECK(hipMemcpyAsync(out.items + o, ri.ptr, sizeof(int32_t) * outs, hipMemcpyDeviceToHost, st));
          if (out.scores) HIP_CHECK(hipMemcpyAsync(out.scores + o, rs.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
          if (distances) HIP_CHECK(hipMemcpyAsync(distances + o, rd.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
          if (out.counts) HIP_CHECK(hipMemcpyAsync(out.counts + b0, rn.ptr, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
          HIP_CHECK(hipStreamSynchronize(st));
          ms += ev.ms() + ev2.ms() + prep_ms;
        });
  }
  c->last_ms[T_DIVERSE] = ms;
}

}  // namespace mmsbm_hip_impl
