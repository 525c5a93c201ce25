// tu_pairs.hip -- translation unit of the m best pairs of the whole model: queries of the recommend session with kernels
// of their own
//   top_pairs.hpp  the m best pairs: one fused launch over the score tiles and the merge levels of the workgroups' lists
//   pairs_bulk.hpp the m best pairs beyond 1,024: a radix select of the bar over the score tiles, count-then-write, then
//                  the sorts of tu_pairs_bulk.hip; the host steps are pairs_bulk_plan.hpp
// (recommend.hpp: the device helpers these kernels share -- the tile accumulation, the sorted list)
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "top_pairs.hpp"
#include "pairs_bulk.hpp"

namespace mmsbm_hip_impl {

// The m best pairs over users[0 .. n_users) (host ids, ascending and distinct) x the session's catalogue
// (top_pairs.hpp).  The launches of a query: one fused launch and the merge levels of G lists -- whatever U and I.
void recommend_top_pairs(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int m, int32_t *out_users,
                         int32_t *out_items, double *out_scores, int32_t *count) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int I = rc.items, rank = rc.rank;
  for (int k = 0; k < m; ++k) {
    out_users[k] = -1;
    out_items[k] = -1;
    out_scores[k] = -INFINITY;
  }
  *count = 0;
  c->last_ms[T_TOP_PAIRS] = 0.f;
  if (n_users == 0 || I == 0) return;
  hipStream_t st = c->stream;
  const int64_t tiles = ((n_users + kRecTile - 1) / kRecTile) * ((static_cast<int64_t>(I) + kRecTile - 1) / kRecTile);
  // G: two workgroups per CU (what the LDS of gtop_fused_kernel allows), one resident set that walks all tiles
  const int G = static_cast<int>(std::min<int64_t>(c->top_groups > 0 ? c->top_groups : 2 * c->n_cus, tiles));
  const size_t per_list = static_cast<size_t>(m) * (sizeof(double) + sizeof(uint64_t)) + sizeof(int32_t);
  const int G1 = (G + kTopFan - 1) / kTopFan;  // lists after the first merge level
  require_free_mem((static_cast<size_t>(G) + G1) * per_list + static_cast<size_t>(n_users) * 4, "top_pairs: the workgroups' lists");
  DevBuf<int32_t> du, na, nb2;
  DevBuf<double> sa, sb;
  DevBuf<uint64_t> ka, kb;
  du.alloc(n_users);
  sa.alloc(static_cast<size_t>(G) * m); ka.alloc(static_cast<size_t>(G) * m); na.alloc(G);
  sb.alloc(static_cast<size_t>(G1) * m); kb.alloc(static_cast<size_t>(G1) * m); nb2.alloc(G1);
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  EventPair ev;  // device time of the query's kernels (option "top_pairs_ms")
  ev.start(st);
  const SeenLists seen = rc.seen_lists();
  LAUNCH(gtop_fused_kernel, G, kBlock, 0, st, rc.x.ptr, rc.x_stride(), rc.y.ptr, static_cast<size_t>(I) * rank, du.ptr,
         static_cast<int>(n_users), I, rank, rc.slots, seen.off, seen.items, m, sa.ptr, ka.ptr, na.ptr);
  // merge levels: a -> b -> a ... until one list is left (G = 1: one level, so that the merge is always part of a query)
  double *is = sa.ptr, *os = sb.ptr;
  uint64_t *ik = ka.ptr, *ok = kb.ptr;
  int32_t *in = na.ptr, *on = nb2.ptr;
  int lists = G;
  do {
    const int out_lists = (lists + kTopFan - 1) / kTopFan;
    LAUNCH(gtop_merge_kernel, out_lists, kBlock, 0, st, is, ik, in, lists, kTopFan, m, os, ok, on);
    std::swap(is, os);
    std::swap(ik, ok);
    std::swap(in, on);
    lists = out_lists;
  } while (lists > 1);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<double> hs(static_cast<size_t>(m));
  std::vector<uint64_t> hk(static_cast<size_t>(m));
  int32_t hn = 0;
  HIP_CHECK(hipMemcpyAsync(hs.data(), is, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hk.data(), ik, sizeof(uint64_t) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&hn, in, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_TOP_PAIRS] = ev.ms();
  *count = hn;
  for (int k = 0; k < hn; ++k) {
    out_users[k] = static_cast<int32_t>(hk[static_cast<size_t>(k)] >> 32);
    out_items[k] = static_cast<int32_t>(hk[static_cast<size_t>(k)] & 0xffffffffu);
    out_scores[k] = hs[static_cast<size_t>(k)];
  }
}

// ---- the m best pairs beyond a workgroup's list (pairs_bulk.hpp) ---------------------------------------------------------
// users ascending and distinct.  out_* null: phase 1 alone (mmsbm_hip_recommend_pair_bar).  counts: above, ties,
// candidates.  The host steps between the launches are pairs_bulk_plan.hpp's.
void recommend_top_pairs_bulk(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int64_t m, int32_t *out_users,
                              int32_t *out_items, double *out_scores, int64_t *count, double *bar, int64_t counts[3]) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int I = rc.items, rank = rc.rank, S = rc.slots;
  const bool fill = out_users != nullptr;
  if (fill) {
    for (int64_t k = 0; k < m; ++k) {
      out_users[k] = -1;
      out_items[k] = -1;
      out_scores[k] = -INFINITY;
    }
    *count = 0;
  }
  *bar = -INFINITY;
  counts[0] = counts[1] = counts[2] = 0;
  c->last_ms[T_TOP_PAIRS_BULK] = 0.f;
  c->pb_passes = 0;
  c->pb_collected = 0;
  int64_t cand = n_users * static_cast<int64_t>(I);
  if (rc.excl)
    for (int64_t b = 0; b < n_users; ++b) cand -= rc.seen_off_h[static_cast<size_t>(users[b]) + 1] - rc.seen_off_h[static_cast<size_t>(users[b])];
  counts[2] = cand;
  if (cand <= 0) return;
  const PbPlan plan = plan_pairs_bulk(n_users, I, cand, m, c->n_cus, c->pb_groups, c->pb_bits, c->pb_collect);
  require_free_mem(fill ? plan.bytes() : plan.bytes() - plan.out_bytes, "top_pairs_bulk: the entries, the histograms and the counts");
  hipStream_t st = c->stream;
  const int nb = static_cast<int>(n_users), G = plan.groups;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(I) * rank;
  const SeenLists seen = rc.seen_lists();
  DevBuf<int32_t> du, tie_row, cut_item;
  DevBuf<unsigned long long> hist, n_buf;
  DevBuf<long long> grp;  // [4][G]: above, ties, admitted, bases
  DevBuf<double> d_bar;
  du.alloc(n_users);
  tie_row.alloc(n_users);
  cut_item.alloc(1);
  hist.alloc(2 * static_cast<size_t>(plan.bins));
  n_buf.alloc(1);
  grp.alloc(4 * static_cast<size_t>(G));
  d_bar.alloc(1);
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  EventPair ev;  // device time of the whole query, the host steps between its launches included (option "pairs_bulk_ms")
  ev.start(st);
  // ---- phase 1: the m-th accumulator ----
  PbState sel = pb_begin(cand, plan.m_out);
  std::vector<unsigned long long> hh(2 * static_cast<size_t>(plan.bins));
  std::vector<int64_t> h(static_cast<size_t>(plan.bins));
  const unsigned seen_grid = static_cast<unsigned>(std::min<int64_t>((n_users + 3) / 4, 64LL * std::max(c->n_cus, 1)));
  for (int pass = 0; sel.done_bits < 64 && !pb_collect_now(sel, plan.collect); ++pass) {
    const PbDigit dg = pb_digit(plan.bits, pass);
    const int bins = 1 << dg.width;
    const PbulkDigit d{sel.prefix, sel.done_bits == 0 ? 1 : 0, sel.done_bits == 0 ? 0 : 64 - sel.done_bits, dg.shift,
                       static_cast<uint32_t>(bins - 1)};
    HIP_CHECK(hipMemsetAsync(hist.ptr, 0, sizeof(unsigned long long) * 2 * plan.bins, st));
    LAUNCH(pbulk_tile_kernel<false>, G, kBlock, sizeof(uint32_t) * bins, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank,
           S, d, hist.ptr, nullptr, nullptr, nullptr, 0ull, nullptr);
    if (seen.off)
      LAUNCH(pbulk_seen_kernel, seen_grid, kBlock, sizeof(uint32_t) * bins, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, rank,
             S, d, seen.off, seen.items, hist.ptr + plan.bins);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hh.data(), hist.ptr, sizeof(unsigned long long) * 2 * plan.bins, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < bins; ++b) {
      h[b] = static_cast<int64_t>(hh[b]) - static_cast<int64_t>(hh[static_cast<size_t>(plan.bins) + b]);
      if (h[b] < 0) throw std::runtime_error("top_pairs_bulk: more seen pairs than pairs in a bin");
    }
    if (!pb_advance(sel, dg, h.data())) throw std::runtime_error("top_pairs_bulk: the histogram holds fewer than m candidates");
    ++c->pb_passes;
  }
  uint64_t key_m = sel.prefix;
  if (sel.done_bits < 64) {  // a small bin: its candidates' keys, sorted; the key of rank k
    const size_t n = static_cast<size_t>(sel.in_bin);
    DevBuf<uint64_t> buf, sorted;
    buf.alloc(n);
    sorted.alloc(n);
    const PbulkDigit d{sel.prefix, sel.done_bits == 0 ? 1 : 0, sel.done_bits == 0 ? 0 : 64 - sel.done_bits, 0, 0u};
    HIP_CHECK(hipMemsetAsync(n_buf.ptr, 0, sizeof(unsigned long long), st));
    LAUNCH(pbulk_tile_kernel<true>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, d, nullptr, seen.off,
           seen.items, buf.ptr, static_cast<unsigned long long>(n), n_buf.ptr);
    HIP_CHECK(hipGetLastError());
    unsigned long long got = 0;
    HIP_CHECK(hipMemcpyAsync(&got, n_buf.ptr, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (got != n) throw std::runtime_error("top_pairs_bulk: the collected bin does not hold what its histogram counted");
    pairs_bulk_sort_desc(c, buf.ptr, sorted.ptr, n);
    HIP_CHECK(hipMemcpyAsync(&key_m, sorted.ptr + (sel.k - 1), sizeof key_m, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    c->pb_collected = sel.in_bin;
  }
  const double acc_m = pb_value(key_m);
  // ---- the bar, the counts above and at it, the ties per user ----
  long long *g_above = grp.ptr, *g_tie = grp.ptr + G, *g_adm = grp.ptr + 2 * static_cast<size_t>(G), *g_base = grp.ptr + 3 * static_cast<size_t>(G);
  HIP_CHECK(hipMemsetAsync(tie_row.ptr, 0, sizeof(int32_t) * n_users, st));
  LAUNCH(pbulk_count_kernel, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
         seen.items, g_above, g_tie, tie_row.ptr, d_bar.ptr);
  HIP_CHECK(hipGetLastError());
  std::vector<long long> hg(2 * static_cast<size_t>(G));
  std::vector<int32_t> ties(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(hg.data(), grp.ptr, sizeof(long long) * 2 * G, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(ties.data(), tie_row.ptr, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(bar, d_bar.ptr, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  int64_t above = 0, at_bar = 0;
  for (int g = 0; g < G; ++g) {
    above += hg[g];
    at_bar += hg[static_cast<size_t>(G) + g];
  }
  counts[0] = above;
  counts[1] = at_bar;
  if (!(above < plan.m_out && plan.m_out <= above + at_bar))
    throw std::runtime_error("top_pairs_bulk: the bar does not hold the m-th pair");
  if (fill) {
    // ---- phase 2: the pairs above the bar and the ties the order admits ----
    const int64_t quota = plan.m_out - above;
    const PbCut cut = pb_tie_cut(ties.data(), n_users, quota);
    const int32_t none = -1;
    HIP_CHECK(hipMemcpyAsync(cut_item.ptr, &none, sizeof none, hipMemcpyHostToDevice, st));
    if (cut.part > 0)
      LAUNCH(pbulk_cut_kernel, 1, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, static_cast<int>(users[cut.row]), I, rank, S,
             acc_m, static_cast<long long>(cut.part), seen.off, seen.items, cut_item.ptr);
    std::vector<long long> adm(static_cast<size_t>(G)), base(static_cast<size_t>(G));
    if (quota == at_bar) {  // every tie is in: the count's numbers
      for (int g = 0; g < G; ++g) adm[g] = hg[g] + hg[static_cast<size_t>(G) + g];
    } else {
      LAUNCH(pbulk_emit_kernel<false>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
             seen.items, static_cast<long long>(cut.row), cut_item.ptr, g_adm, nullptr, nullptr, nullptr, 0ll);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(adm.data(), g_adm, sizeof(long long) * G, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
    long long run = 0;
    for (int g = 0; g < G; ++g) {
      base[g] = run;
      run += adm[g];
    }
    if (run != plan.m_out) throw std::runtime_error("top_pairs_bulk: the admitted pairs are not min(m, candidates)");
    const size_t n = static_cast<size_t>(plan.m_out);
    DevBuf<uint64_t> ok, fk;
    DevBuf<double> os, fs;
    ok.alloc(n); os.alloc(n); fk.alloc(n); fs.alloc(n);
    HIP_CHECK(hipMemcpyAsync(g_base, base.data(), sizeof(long long) * G, hipMemcpyHostToDevice, st));
    LAUNCH(pbulk_emit_kernel<true>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
           seen.items, static_cast<long long>(cut.row), cut_item.ptr, g_adm, g_base, ok.ptr, os.ptr, static_cast<long long>(n));
    HIP_CHECK(hipGetLastError());
    // ---- phase 3: the order ----
    pairs_bulk_order(c, ok.ptr, os.ptr, n, fk.ptr, fs.ptr);
    std::vector<uint64_t> hk(n);
    HIP_CHECK(hipMemcpyAsync(hk.data(), fk.ptr, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(out_scores, fs.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k) {
      out_users[k] = static_cast<int32_t>(hk[k] >> 32);
      out_items[k] = static_cast<int32_t>(hk[k] & 0xffffffffu);
    }
    *count = plan.m_out;
  }
  ev.stop(st);
  ev.wait();
  c->last_ms[T_TOP_PAIRS_BULK] = ev.ms();
}

}  // namespace mmsbm_hip_impl
