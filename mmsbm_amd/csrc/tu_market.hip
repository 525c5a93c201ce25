// tu_market.hip -- translation unit of the item side and of capacity: the queries of the recommend session that score
// items against users or share items out among them, in the frame of serve_frame.hpp
//   audience.hpp   item-side queries: the n best users of an item, and an item's audience above a bar (fused kernel)
//   allocate.hpp   capacity-aware allocation: rounds of the user-side and the item-side batches with a threshold epilogue
//                  on the score tile, the same exclusions and selection; the lists and the keys stay on the device
//   assign.hpp     welfare-maximising assignment: rounds of a forward auction over the compacted active users -- the
//                  score tile less a price per column, the same exclusions and selection with n = 2, the bids sorted
//                  (tu_pairs_bulk.hip) and merged into the items' slots by one wave per item
//   assortment.hpp greedy assortment selection: rounds of a gain pass over the score tiles against a per-user state, an
//                  arg-max over the catalogue and a state update, chained on the stream behind a stop flag
// (recommend.hpp and top_pairs.hpp: the device helpers these kernels share -- the tile accumulation, the sorted list; the
// smallest accumulator at or above a bar, gtop_floor_acc.  Nothing of theirs is launched here.)
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "top_pairs.hpp"
#include "audience.hpp"
#include "allocate.hpp"
#include "assign.hpp"
#include "assortment.hpp"

namespace mmsbm_hip_impl {

// ---- item-side queries (audience.hpp) -----------------------------------------------------------------------------------
namespace {

// The item -> users lists of the session: the transpose of seen_off / seen, so each item's users are ascending and
// distinct by construction.  Built by the first item-side query, dropped by recommend_add_items.
void rec_item_lists(mmsbm_hip_ctx *c) {
  RecSession &rc = *c->rc;
  if (!rc.excl || rc.by_item_built) return;
  const int U = c->ext_users, NI = rc.items;
  hipStream_t st = c->stream;
  const size_t n = static_cast<size_t>(rc.seen_off_h[U]);
  std::vector<int32_t> seen(n);
  if (n > 0) HIP_CHECK(hipMemcpyAsync(seen.data(), rc.seen.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int32_t> off(static_cast<size_t>(NI) + 1, 0), user(n);
  for (size_t e = 0; e < n; ++e) ++off[static_cast<size_t>(seen[e]) + 1];
  for (int i = 0; i < NI; ++i) off[i + 1] += off[i];
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (int u = 0; u < U; ++u)  // (users ascending: so is every item's list)
    for (int32_t e = rc.seen_off_h[u]; e < rc.seen_off_h[u + 1]; ++e) user[static_cast<size_t>(at[seen[e]]++)] = u;
  require_free_mem((off.size() + n) * sizeof(int32_t), "recommend: the items' excluded users");
  DevBuf<int32_t> d_off, d_user;
  d_off.upload(off, st);
  d_user.upload(user, st);
  HIP_CHECK(hipStreamSynchronize(st));  // (host vectors are locals)
  rc.by_item_off.swap(d_off);
  rc.by_item.swap(d_user);
  rc.by_item_built = true;
}

}  // namespace

void recommend_query_items(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, int n, const TopNOut &out) {
  use_device(c);
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  const SeenLists ex{rc.excl ? rc.by_item_off.ptr : nullptr, rc.by_item.ptr};  // (by item id: the users left out)
  top_n_run(c, rc.users, n_items, items, n, "recommend: a batch of items",
            [&](const int32_t *ib, int nb, int64_t, double *sc) {  // rec_score_batch with the sides exchanged
              score_tiles(c, rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.x.ptr, rc.x_stride(), rc.users, ib, nb, ex, sc);
            },
            T_RECOMMEND, out);
}

void recommend_audience(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, double min_score, int64_t capacity,
                        int64_t *offsets, int32_t *users, double *scores) {
  use_device(c);
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  std::fill(offsets, offsets + n_items + 1, int64_t(0));
  c->last_ms[T_AUDIENCE] = 0.f;
  const int U = c->ext_users, rank = rc.rank, S = rc.slots;
  if (n_items == 0 || U == 0) return;
  hipStream_t st = c->stream;
  const int64_t n_ut = (static_cast<int64_t>(U) + kRecTile - 1) / kRecTile;
  const int64_t rb = aud_count_rows(U, c->aud_rows, n_items);  // items per COUNT batch
  const size_t table = static_cast<size_t>(rb) * n_ut;
  require_free_mem(table * 4 + static_cast<size_t>(n_items) * 8 + static_cast<size_t>(rb) * 8,
                   "audience: the counts of a batch of items");
  DevBuf<int32_t> di, cnt, tot;
  di.alloc(n_items);
  cnt.alloc(table);
  tot.alloc(n_items);
  HIP_CHECK(hipMemcpyAsync(di.ptr, items, sizeof(int32_t) * n_items, hipMemcpyHostToDevice, st));
  const int32_t *ex_off = rc.excl ? rc.by_item_off.ptr : nullptr, *ex = rc.by_item.ptr;
  const size_t xs = static_cast<size_t>(rc.items) * rank, ys = rc.x_stride();
  // tiles are dealt to at most 8 workgroups per CU (what the staging tiles' LDS allows twice over)
  auto groups = [&](int nb) {
    return static_cast<unsigned>(std::min<int64_t>(n_ut * ((nb + kRecTile - 1) / kRecTile), 8LL * c->n_cus));
  };
  // COUNT + offsets of rows [r0, r0 + nb): cnt [user tile][nb], tot[r0 ...]
  auto count_batch = [&](int64_t r0, int nb) {
    LAUNCH(aud_tile_kernel<false>, groups(nb), kBlock, 0, st, rc.y.ptr, xs, rc.x.ptr, ys, di.ptr + r0, nb, U, rank, S,
           ex_off, ex, min_score, cnt.ptr, static_cast<size_t>(nb), nullptr, int64_t(0), nullptr, nullptr, int64_t(0));
    LAUNCH(aud_offsets_kernel, static_cast<unsigned>((nb + kBlock - 1) / kBlock), kBlock, 0, st, cnt.ptr,
           static_cast<size_t>(nb), static_cast<int>(n_ut), nb, tot.ptr + r0);
  };
  float ms = 0.f;  // device time of the call's kernels (option "audience_ms")
  std::vector<int32_t> ht(static_cast<size_t>(n_items));
  {
    EventPair ev;
    ev.start(st);
    for (int64_t r0 = 0; r0 < n_items; r0 += rb) count_batch(r0, static_cast<int>(std::min(rb, n_items - r0)));
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(ht.data(), tot.ptr, sizeof(int32_t) * n_items, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  int64_t largest = 0;
  for (int64_t b = 0; b < n_items; ++b) {
    offsets[b + 1] = offsets[b] + ht[static_cast<size_t>(b)];
    largest = std::max<int64_t>(largest, ht[static_cast<size_t>(b)]);
  }
  c->last_ms[T_AUDIENCE] = ms;
  const int64_t total = offsets[n_items];
  if (!users || total == 0) return;
  if (capacity < total)
    throw ApiError(MMSBM_E_TOOLARGE, "audience: " + std::to_string(total) + " entries, room for " + std::to_string(capacity));
  // WRITE: runs of rows whose entries stay under the cap (a larger row goes alone), inside the COUNT batches; a batch's
  // counts are formed again unless the request was one batch, whose offsets are still there
  const int64_t cap = c->aud_entries > 0 ? c->aud_entries : kAudEntries;
  const int64_t out_cap = std::min(total, std::max(cap, largest));
  require_free_mem(static_cast<size_t>(out_cap) * 12 + static_cast<size_t>(rb) * 8, "audience: the entries of a batch of items");
  DevBuf<int32_t> ou;
  DevBuf<double> os;
  DevBuf<int64_t> rbase;
  ou.alloc(static_cast<size_t>(out_cap));
  os.alloc(static_cast<size_t>(out_cap));
  rbase.alloc(static_cast<size_t>(rb));
  const bool one_batch = rb >= n_items;
  std::vector<int64_t> hb(static_cast<size_t>(rb));
  for (int64_t r0 = 0; r0 < n_items; r0 += rb) {
    const int nb = static_cast<int>(std::min(rb, n_items - r0));
    if (offsets[r0 + nb] == offsets[r0]) continue;
    for (int j = 0; j < nb; ++j) hb[static_cast<size_t>(j)] = offsets[r0 + j] - offsets[r0];
    HIP_CHECK(hipMemcpyAsync(rbase.ptr, hb.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (hb is written again for the next batch)
    if (!one_batch) {
      EventPair ev;
      ev.start(st);
      count_batch(r0, nb);
      ev.stop(st);
      HIP_CHECK(hipStreamSynchronize(st));
      ms += ev.ms();
    }
    for (const AudRun &run : aud_write_runs(ht.data() + r0, nb, cap)) {
      if (run.entries == 0) continue;
      const int s0 = run.first;
      EventPair ev;
      ev.start(st);
      LAUNCH(aud_tile_kernel<true>, groups(run.rows), kBlock, 0, st, rc.y.ptr, xs, rc.x.ptr, ys, di.ptr + r0 + s0, run.rows,
             U, rank, S, ex_off, ex, min_score, cnt.ptr + s0, static_cast<size_t>(nb), rbase.ptr + s0,
             hb[static_cast<size_t>(s0)], ou.ptr, os.ptr, out_cap);
      HIP_CHECK(hipGetLastError());
      ev.stop(st);
      const int64_t o = offsets[r0 + s0];
      HIP_CHECK(hipMemcpyAsync(users + o, ou.ptr, sizeof(int32_t) * run.entries, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipMemcpyAsync(scores + o, os.ptr, sizeof(double) * run.entries, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      ms += ev.ms();
    }
  }
  c->last_ms[T_AUDIENCE] = ms;
}

// ---- capacity-aware allocation (allocate.hpp) ----------------------------------------------------------------------------
// The rounds of deferred acceptance: per round the batches of recommend_query (user pass) and of recommend_query_items
// over the capped items (item pass), both with alloc_score_kernel in place of rec_score_kernel; P, sigma and tau stay on
// the device, and the host reads one int per round.  users: distinct ids (checked by the C ABI); plan: the caps.
void recommend_allocate(mmsbm_hip_ctx *c, const UserRows &users, int n, const AllocPlan &plan, int max_rounds,
                        const TopNOut &out, int32_t *rounds, int32_t *converged) {
  use_device(c);
  const int64_t n_users = users.n;
  top_n_blank(n_users, n, out);
  *rounds = 0;
  *converged = 1;
  c->last_ms[T_ALLOCATE] = 0.f;
  c->alloc_rounds = 0;
  if (n_users == 0) return;
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  const int U = rc.users, NI = rc.items, rank = rc.rank;
  const int64_t NC = plan.capped();
  hipStream_t st = c->stream;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(NI) * rank;
  // user pass: batches of bu users over NI columns; item pass: batches of plan.bi capped items over U columns
  const int64_t bu = rec_batch_users(NI, n_users), bi = plan.bi;
  const int nsel = plan.most_n;
  const SelectPlan up = select_plan(c, NI, bu, n), ip = NC > 0 ? select_plan(c, U, bi, nsel) : SelectPlan{};
  const size_t buf = std::max(static_cast<size_t>(bu) * NI, static_cast<size_t>(bi) * U);
  const size_t outs = static_cast<size_t>(n_users) * n, lists = static_cast<size_t>(bi) * nsel;
  require_free_mem(buf * sizeof(double) + SelectStage::bytes(up, ip) + outs * 12 + static_cast<size_t>(n_users) * 8 +
                       lists * 12 + static_cast<size_t>(bi) * 4 + (static_cast<size_t>(NI) + U) * 12 +
                       static_cast<size_t>(NC) * 9 + 4,
                   "recommend_allocate: a batch of scores, the users' lists and the items' keys");
  // tau by item: -inf (everything is acceptable), +inf for a closed item (nothing is); sigma by user: +inf outside the
  // request (nothing stands in front of it), written for the request's users by every round
  std::vector<double> tau_h(static_cast<size_t>(NI), -INFINITY), sig_h(static_cast<size_t>(U), INFINITY);
  for (int32_t i : plan.closed) tau_h[static_cast<size_t>(i)] = INFINITY;
  const std::vector<int32_t> tau_uh(static_cast<size_t>(NI), -1), sig_ih(static_cast<size_t>(U), -1);
  DevBuf<double> sc, ps, ls, tau_s, sig_s;
  DevBuf<int32_t> du, pi, pn, lu, ln, tau_u, sig_i, d_item, d_cap, d_total;
  DevBuf<unsigned char> d_changed;
  sc.alloc(buf);
  const SelectStage sel(up, ip);  // (the two passes follow each other: one scratch)
  ps.alloc(outs); pi.alloc(outs); pn.alloc(static_cast<size_t>(n_users));
  du.alloc(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(du.ptr, users.ids, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  tau_s.upload(tau_h, st); tau_u.upload(tau_uh, st);
  if (NC > 0) {
    ls.alloc(lists); lu.alloc(lists); ln.alloc(static_cast<size_t>(bi));
    sig_s.upload(sig_h, st); sig_i.upload(sig_ih, st);
    d_item.upload(plan.item, st); d_cap.upload(plan.cap, st);
    d_changed.alloc(static_cast<size_t>(NC));
    d_total.alloc(1);
  }
  const SeenLists seen = rc.seen_lists();
  const SeenLists by_item{rc.excl ? rc.by_item_off.ptr : nullptr, rc.by_item.ptr};
  const unsigned row_blocks = static_cast<unsigned>((n_users + kBlock - 1) / kBlock);
  EventPair ev;  // device time of the whole call (option "allocate_ms"): the host's reads between the rounds included
  ev.start(st);
  int round = 0;
  bool done = false;
  while (!done) {
    ++round;
    for_batches(n_users, bu, [&](int64_t b0, int nb) {  // the user pass
      const int32_t *ub = du.ptr + b0;
      LAUNCH(alloc_score_kernel, tile_grid(NI, nb), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, ub, nb, NI, rank, rc.slots,
             nullptr, nullptr, tau_s.ptr, tau_u.ptr, sc.ptr, static_cast<size_t>(NI));
      exclude_seen(st, ub, nb, seen, sc.ptr, static_cast<size_t>(NI));
      sel.run(st, up, sc.ptr, nb, n, ps.ptr + b0 * n, pi.ptr + b0 * n, pn.ptr + b0);
    });
    HIP_CHECK(hipGetLastError());
    if (NC == 0) break;  // (no cap binds: the answer is the user pass)
    LAUNCH(alloc_sigma_kernel, row_blocks, kBlock, 0, st, du.ptr, static_cast<int>(n_users), n, ps.ptr, pi.ptr, pn.ptr,
           sig_s.ptr, sig_i.ptr);
    for_batches(NC, bi, [&](int64_t r0, int nb) {  // the item pass: the sides exchanged
      const int32_t *ib = d_item.ptr + r0;
      const int bn = plan.batch_n[static_cast<size_t>(r0 / bi)];
      LAUNCH(alloc_score_kernel, tile_grid(U, nb), kBlock, 0, st, rc.y.ptr, ys, rc.x.ptr, xs, ib, nb, U, rank, rc.slots,
             tau_s.ptr, tau_u.ptr, sig_s.ptr, sig_i.ptr, sc.ptr, static_cast<size_t>(U));
      exclude_seen(st, ib, nb, by_item, sc.ptr, static_cast<size_t>(U));
      sel.run(st, ip, sc.ptr, nb, bn, ls.ptr, lu.ptr, ln.ptr);
      LAUNCH(alloc_tau_kernel, static_cast<unsigned>((nb + kBlock - 1) / kBlock), kBlock, 0, st, ib, d_cap.ptr + r0, nb, bn,
             ls.ptr, lu.ptr, ln.ptr, tau_s.ptr, tau_u.ptr, d_changed.ptr + r0);
    });
    LAUNCH(alloc_changed_kernel, 1, kBlock, 0, st, d_changed.ptr, static_cast<int>(NC), d_total.ptr);
    HIP_CHECK(hipGetLastError());
    int32_t changed = 0;
    HIP_CHECK(hipMemcpyAsync(&changed, d_total.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (the round's only wait)
    if (changed == 0) {
      done = true;
    } else if (round == max_rounds) {
      *converged = 0;
      done = true;
    }
  }
  LAUNCH(alloc_cut_kernel, row_blocks, kBlock, 0, st, du.ptr, static_cast<int>(n_users), n, tau_s.ptr, tau_u.ptr, ps.ptr,
         pi.ptr, pn.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  top_n_copy_out(c, TopNDev{ps.ptr, pi.ptr, pn.ptr}, ev, n_users, n, T_ALLOCATE, out);
  *rounds = round;
  c->alloc_rounds = round;
}

// ---- welfare-maximising assignment (assign.hpp) -------------------------------------------------------------------------
// The rounds of the forward auction over the compacted list of active rows, then the certificate pass over all rows; the
// row state, the slots and the prices stay on the device, and the host reads one int per round: the next round's active
// rows.  users: distinct ids (checked by the C ABI), any order -- the device works in id order.
void recommend_assign(mmsbm_hip_ctx *c, const UserRows &rows, const AssignPlan &plan, double reserve, double eps,
                      int max_rounds, const AssignOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int64_t n_users = rows.n;
  const int NI = rc.items, rank = rc.rank;
  for (int64_t b = 0; b < n_users; ++b) {
    out.items[b] = -1;
    out.scores[b] = -INFINITY;
    out.paid[b] = 0.0;
    out.pi[b] = reserve;
  }
  for (int i = 0; i < NI; ++i) {
    const int32_t q = plan.cap[static_cast<size_t>(i)];
    out.price[i] = q == 0 ? INFINITY : 0.0;
    out.price_sum[i] = 0.0;
    out.load[i] = 0;
  }
  *out.rounds = 0;
  *out.converged = 1;
  c->last_ms[T_ASSIGN] = 0.f;
  c->asg_rounds = 0;
  c->asg_bids = 0;
  if (n_users == 0 || NI == 0) return;
  hipStream_t st = c->stream;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(NI) * rank;
  const size_t nu = static_cast<size_t>(n_users), n_slots = plan.slots();
  // the request in id order: row r is request row at[r]
  std::vector<int64_t> at(nu);
  for (size_t b = 0; b < nu; ++b) at[b] = static_cast<int64_t>(b);
  std::sort(at.begin(), at.end(), [&](int64_t a, int64_t b) { return rows.ids[a] < rows.ids[b]; });
  std::vector<int32_t> ids(nu);
  for (size_t r = 0; r < nu; ++r) ids[r] = rows.ids[at[r]];
  const int64_t bu = rec_batch_users(NI, n_users);
  const SelectPlan sp = select_plan(c, NI, bu, 2);
  const int nblk = static_cast<int>((n_users + kBlock - 1) / kBlock);
  const size_t sort_bytes = assign_sort_bytes(nu);
  require_free_mem(static_cast<size_t>(bu) * NI * sizeof(double) + sp.bytes() +
                       nu * (2 * 8 + 2 * 4 + 2 * 12 + 4 + 3 * 4 + 2 * 8 + 2 * 4) + n_slots * 12 +
                       static_cast<size_t>(NI) * (3 * 8 + 2 * 4) + static_cast<size_t>(nblk) * 8 + sort_bytes + 4,
                   "recommend_assign: a batch of scores, the users' state, the bids and the items' slots");
  std::vector<double> p1_h(static_cast<size_t>(NI)), p2_h(static_cast<size_t>(NI));
  for (int i = 0; i < NI; ++i) {
    const int32_t q = plan.cap[static_cast<size_t>(i)];
    p1_h[static_cast<size_t>(i)] = q == 0 ? INFINITY : 0.0;
    p2_h[static_cast<size_t>(i)] = q < 0 || q >= 2 ? 0.0 : INFINITY;
  }
  DevBuf<double> sc, vs, row_paid, row_score, price, p1, p2, bid, bid_score, psum;
  DevBuf<int32_t> du, vi, vn, row_item, dropped, holder, d_cap, d_off, act_r, act_u, bid_item, blk_cnt, blk_base,
      d_total;
  DevBuf<uint32_t> place, ord;
  DevBuf<char> tmp;
  sc.alloc(static_cast<size_t>(bu) * NI);
  const SelectStage sel(sp);
  vs.alloc(2 * nu); vi.alloc(2 * nu); vn.alloc(nu);
  du.upload(ids, st);
  act_u.upload(ids, st);  // the first round: every row is active
  std::vector<int32_t> iota(nu);
  for (size_t r = 0; r < nu; ++r) iota[r] = static_cast<int32_t>(r);
  act_r.upload(iota, st);
  // nobody holds anything, every slot is free at price 0 (+0.0 and -1 are one byte repeated)
  const std::vector<double> ninf_d(nu, -INFINITY);
  row_item.alloc(nu); dropped.alloc(nu); row_paid.alloc(nu); row_score.upload(ninf_d, st);
  price.alloc(n_slots); holder.alloc(n_slots); psum.alloc(static_cast<size_t>(NI));
  HIP_CHECK(hipMemsetAsync(row_item.ptr, 0xFF, sizeof(int32_t) * nu, st));
  HIP_CHECK(hipMemsetAsync(dropped.ptr, 0, sizeof(int32_t) * nu, st));
  HIP_CHECK(hipMemsetAsync(row_paid.ptr, 0, sizeof(double) * nu, st));
  if (n_slots > 0) {
    HIP_CHECK(hipMemsetAsync(price.ptr, 0, sizeof(double) * n_slots, st));
    HIP_CHECK(hipMemsetAsync(holder.ptr, 0xFF, sizeof(int32_t) * n_slots, st));
  }
  p1.upload(p1_h, st); p2.upload(p2_h, st);
  d_cap.upload(plan.cap, st); d_off.upload(plan.slot_off, st);
  bid.alloc(nu); bid_score.alloc(nu); bid_item.alloc(nu); place.alloc(nu); ord.alloc(nu);
  blk_cnt.alloc(static_cast<size_t>(nblk)); blk_base.alloc(static_cast<size_t>(nblk)); d_total.alloc(1);
  tmp.alloc(sort_bytes);
  HIP_CHECK(hipStreamSynchronize(st));  // (the uploads' host vectors are temporaries)
  const SeenLists seen = rc.seen_lists();
  const size_t accept_lds = static_cast<size_t>(plan.lds_places()) * (sizeof(double) + sizeof(int32_t));
  // the values of the rows ids[0 .. n_rows) (device) at the prices p1, the exclusions, and the n best of every row to
  // vs / vi / vn, batch by batch
  auto value_pass = [&](const int32_t *ids, int64_t n_rows, int n) {
    for_batches(n_rows, bu, [&](int64_t b0, int nb) {
      const int32_t *ub = ids + b0;
      LAUNCH(assign_value_kernel, tile_grid(NI, nb), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, ub, nb, NI, rank, rc.slots,
             p1.ptr, sc.ptr, static_cast<size_t>(NI));
      exclude_seen(st, ub, nb, seen, sc.ptr, static_cast<size_t>(NI));
      sel.run(st, sp, sc.ptr, nb, n, vs.ptr + b0 * n, vi.ptr + b0 * n, vn.ptr + b0);
    });
  };
  EventPair ev;  // device time of the whole call (option "assign_ms"): the host's reads between the rounds included
  ev.start(st);
  int round = 0;
  int64_t na = n_users, active_sum = 0;
  while (na > 0) {
    if (round == max_rounds) {
      *out.converged = 0;
      break;
    }
    ++round;
    active_sum += na;
    value_pass(act_u.ptr, na, 2);
    const int n_act = static_cast<int>(na);
    LAUNCH(assign_bid_kernel, static_cast<unsigned>((na + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys,
           rank, rc.slots, act_u.ptr, act_r.ptr, n_act, vs.ptr, vi.ptr, vn.ptr, p1.ptr, p2.ptr, reserve, eps, bid_item.ptr,
           bid.ptr, bid_score.ptr, place.ptr, dropped.ptr);
    assign_sort_bids(st, tmp.ptr, sort_bytes, bid_item.ptr, bid.ptr, place.ptr, ord.ptr, static_cast<size_t>(na));
    LAUNCH(assign_accept_kernel, static_cast<unsigned>(NI), kRecWave, accept_lds, st, d_cap.ptr, d_off.ptr, plan.lds_places(),
           bid_item.ptr, bid.ptr, bid_score.ptr, ord.ptr, n_act, act_r.ptr, price.ptr, holder.ptr, p1.ptr, p2.ptr,
           row_item.ptr, row_paid.ptr, row_score.ptr);
    LAUNCH(assign_count_kernel, static_cast<unsigned>(nblk), kBlock, 0, st, row_item.ptr, dropped.ptr,
           static_cast<int>(n_users), blk_cnt.ptr);
    LAUNCH(assign_scan_kernel, 1, kBlock, 0, st, blk_cnt.ptr, nblk, blk_base.ptr, d_total.ptr);
    LAUNCH(assign_list_kernel, static_cast<unsigned>(nblk), kBlock, 0, st, row_item.ptr, dropped.ptr, du.ptr,
           static_cast<int>(n_users), blk_base.ptr, act_r.ptr, act_u.ptr);
    HIP_CHECK(hipGetLastError());
    int32_t next = 0;
    HIP_CHECK(hipMemcpyAsync(&next, d_total.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (the round's only wait)
    na = next;
  }
  // the certificate: every row's best value at the final prices
  value_pass(du.ptr, n_users, 1);
  LAUNCH(assign_price_sum_kernel, static_cast<unsigned>((NI + kBlock - 1) / kBlock), kBlock, 0, st, d_off.ptr, price.ptr, NI,
         psum.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<int32_t> h_item(nu), h_drop(nu), h_vn(nu);
  std::vector<double> h_paid(nu), h_score(nu), h_vs(nu);
  HIP_CHECK(hipMemcpyAsync(h_item.data(), row_item.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_drop.data(), dropped.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_vn.data(), vn.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_paid.data(), row_paid.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_score.data(), row_score.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_vs.data(), vs.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(out.price_sum, psum.ptr, sizeof(double) * NI, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(out.price, p1.ptr, sizeof(double) * NI, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_ASSIGN] = ev.ms();
  int64_t n_dropped = 0;
  for (size_t r = 0; r < nu; ++r) {
    const size_t b = static_cast<size_t>(at[r]);
    const double best = h_vn[r] > 0 ? h_vs[r] : -INFINITY;
    out.pi[b] = best > reserve ? best : reserve;
    n_dropped += h_drop[r] != 0;
    if (h_item[r] < 0) continue;
    out.items[b] = h_item[r];
    out.scores[b] = h_score[r];
    out.paid[b] = h_paid[r];
    ++out.load[h_item[r]];
  }
  *out.rounds = round;
  c->asg_rounds = round;
  c->asg_bids = active_sum - n_dropped;  // every active row of a round bids or drops out, and drops out once
}

// ---- greedy assortment selection (assortment.hpp) -------------------------------------------------------------------------
// plan (plan_assortment: the runs of user rows, the batches of item tiles), memory check, uploads; the given items one
// by one (their gain over the state before them, then the state); then n_pick rounds of gain / join / pick / update
// enqueued back to back -- no host wait and no copy between them: once the stop flag is set on the device the launches
// that follow return at once -- and ONE read-back at the end.  users: ascending, distinct.
void recommend_assortment(mmsbm_hip_ctx *c, const UserRows &asked, int mode, double level, const int32_t *given,
                          int n_given, const Subset &sub, int n_pick, int32_t *items, double *gains, int32_t *count,
                          int32_t *stop, double *given_gains, int32_t *served_items, double *served_scores) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int32_t *users = asked.ids, *cand = sub.items;  // (cand null: the columns are the items)
  for (float *t : {&c->last_ms[T_ASSORT], &c->asrt_ms[0], &c->asrt_ms[1], &c->asrt_ms[2]}) *t = 0.f;
  const int NI = rc.items, rank = rc.rank, S = rc.slots;
  const int C = sub.columns(NI);
  for (int k = 0; k < n_pick; ++k) {
    items[k] = -1;
    gains[k] = 0.0;
  }
  for (int g = 0; g < n_given; ++g) given_gains[g] = 0.0;
  *count = 0;
  *stop = n_pick == 0 ? MMSBM_HIP_ASSORT_STOP_C : C == 0 ? MMSBM_HIP_ASSORT_STOP_NO_CANDIDATES : MMSBM_HIP_ASSORT_STOP_NO_GAIN;
  if (asked.n == 0) return;  // (nobody to serve: no item gains anything)
  const int nu = static_cast<int>(asked.n);
  const AssortPlan p = plan_assortment(asked.n, C, c->n_cus, c->asrt_run,
                                       c->asrt_part > 0 ? static_cast<size_t>(c->asrt_part) : kAsrtPartBytes);
  // a given item: its one tile of the catalogue, in the runs of the rounds -- a column's sum is the same additions in the
  // same order whether the item is given or chosen, so a set valued as given items gets the greedy's bits
  const AssortPlan pg = plan_assortment(asked.n, kRecTile, c->n_cus, C > 0 ? p.run_blocks : c->asrt_run);
  const bool rounds = n_pick > 0 && C > 0;
  const size_t ycs = static_cast<size_t>(C) * rank;
  const size_t n_res = static_cast<size_t>(n_pick) + static_cast<size_t>(n_given);
  require_free_mem(CatTable::bytes(rc, sub) + static_cast<size_t>(nu) * (4 + 8 + 4 + 8) + static_cast<size_t>(C) * 4 + n_res * 12 +
                       (rounds ? p.part_doubles() * sizeof(double) + static_cast<size_t>(p.n_blk()) * 12 : 0) +
                       (n_given > 0 ? pg.part_doubles() * sizeof(double) : 0),
                   "recommend_assortment: the users' state, the runs' partial sums and the candidates' rows");
  hipStream_t st = c->stream;
  // the state: best[u] = level x S undivided (BEST; REACH fills it when a user is covered), nobody served
  std::vector<double> h_best(static_cast<size_t>(nu), mode == kAsrtBest ? level * static_cast<double>(S) : 0.0);
  std::vector<int32_t> h_served(static_cast<size_t>(nu), -1), h_users(users, users + nu);
  std::vector<int32_t> h_taken(static_cast<size_t>(C), 0);
  for (int g = 0; g < n_given; ++g) {  // a given item is never chosen: its column, where it has one
    if (cand) {
      const int32_t *at = std::lower_bound(cand, cand + C, given[g]);
      if (at != cand + C && *at == given[g]) h_taken[static_cast<size_t>(at - cand)] = 1;
    } else {
      h_taken[static_cast<size_t>(given[g])] = 1;
    }
  }
  DevBuf<double> best, score, part, part_g, blk_v, res_gain;
  DevBuf<int32_t> rows, served, taken, blk_i, res_col, flags;
  CatTable ct;
  rows.upload(h_users, st);
  best.upload(h_best, st);
  served.upload(h_served, st);
  taken.upload(h_taken, st);
  score.alloc(static_cast<size_t>(nu));
  res_col.alloc(static_cast<size_t>(n_pick));
  res_gain.alloc(n_res);
  flags.alloc(2);  // the stop flag, the count
  HIP_CHECK(hipMemsetAsync(res_gain.ptr, 0, sizeof(double) * std::max<size_t>(n_res, 1), st));
  HIP_CHECK(hipMemsetAsync(flags.ptr, 0, sizeof(int32_t) * 2, st));
  if (rounds) {
    part.alloc(p.part_doubles());
    blk_v.alloc(static_cast<size_t>(p.n_blk()));
    blk_i.alloc(static_cast<size_t>(p.n_blk()));
    if (cand) cat_table(c, sub, ct);
  }
  if (n_given > 0) part_g.alloc(pg.part_doubles());
  const double *y = cand && rounds ? ct.y.ptr : rc.y.ptr;
  const size_t yfs = static_cast<size_t>(NI) * rank, ys = cand && rounds ? ycs : yfs, xs = rc.x_stride();
  const SeenLists seen = rc.seen_lists();
  const int32_t *dcand = cand && rounds ? ct.cand.ptr : nullptr;
  int32_t *d_stop = flags.ptr, *d_count = flags.ptr + 1;
  double *d_given = res_gain.ptr + n_pick;
  const unsigned user_grid = static_cast<unsigned>((nu + kBlock - 1) / kBlock);
  auto gain = [&](const AssortPlan &pl, const double *yy, size_t yys, int ni, int tile0, unsigned tiles, const int32_t *cols,
                  double *out) {
    const dim3 g(tiles, static_cast<unsigned>(pl.runs));
    auto tile = [&](auto kernel) {
      LAUNCH(kernel, g, kBlock, 0, st, rc.x.ptr, xs, yy, yys, rows.ptr, nu, static_cast<int>(pl.run_rows), ni, tile0, rank, S,
             level, best.ptr, served.ptr, seen.off, seen.items, cols, d_stop, out, static_cast<size_t>(pl.ld));
    };
    if (mode == kAsrtBest) tile(asrt_gain_kernel<kAsrtBest>);
    else tile(asrt_gain_kernel<kAsrtReach>);
  };
  auto update = [&](int k, int item) {
    auto go = [&](auto kernel) {
      LAUNCH(kernel, user_grid, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, yfs, rows.ptr, nu, rank, S, level, k, item, res_col.ptr,
             dcand, seen.off, seen.items, d_stop, best.ptr, served.ptr);
    };
    if (mode == kAsrtBest) go(asrt_update_kernel<kAsrtBest>);
    else go(asrt_update_kernel<kAsrtReach>);
  };
  // the phases' device times (option "assortment_timing"): one event at every border between two phases of a round
  std::vector<std::unique_ptr<EventPair::Event>> marks;
  auto mark = [&] {
    if (!c->asrt_timing) return;
    marks.push_back(std::make_unique<EventPair::Event>());
    HIP_CHECK(hipEventRecord(marks.back()->e, st));
  };
  EventPair ev;  // device time of the query's kernels (option "assortment_ms")
  ev.start(st);
  for (int g = 0; g < n_given; ++g) {
    gain(pg, rc.y.ptr, yfs, NI, given[g] / kRecTile, 1u, nullptr, part_g.ptr);
    LAUNCH(asrt_given_kernel, 1, kRecWave, 0, st, part_g.ptr, static_cast<size_t>(pg.ld), static_cast<int>(pg.runs),
           given[g] % kRecTile, g, d_given);
    update(-1, given[g]);
  }
  HIP_CHECK(hipGetLastError());
  for (int k = 0; rounds && k < n_pick; ++k) {  // (rounds follow each other on the stream: no host wait in between)
    mark();
    for (int64_t b = 0; b < p.batches; ++b) {
      const auto [col0, n_cols] = p.batch_cols(b, C);
      gain(p, y, ys, C, static_cast<int>(b * p.batch_tiles), static_cast<unsigned>((n_cols + kRecTile - 1) / kRecTile), dcand,
           part.ptr);
      LAUNCH(asrt_join_kernel, static_cast<unsigned>((n_cols + kAsrtJoin - 1) / kAsrtJoin), kBlock, 0, st, part.ptr,
             static_cast<size_t>(p.ld), static_cast<int>(p.runs), static_cast<int>(col0), static_cast<int>(n_cols), taken.ptr,
             p.batch_blk[static_cast<size_t>(b)], d_stop, blk_v.ptr, blk_i.ptr);
    }
    mark();
    LAUNCH(asrt_pick_kernel, 1, kBlock, 0, st, blk_v.ptr, blk_i.ptr, static_cast<int>(p.n_blk()), k, taken.ptr, res_col.ptr,
           res_gain.ptr, d_count, d_stop);
    mark();
    update(k, 0);
    HIP_CHECK(hipGetLastError());
  }
  mark();
  LAUNCH(asrt_finish_kernel, static_cast<unsigned>((std::max<size_t>(n_res, static_cast<size_t>(nu)) + kBlock - 1) / kBlock),
         kBlock, 0, st, res_gain.ptr, static_cast<int>(n_res), mode == kAsrtBest, best.ptr, served.ptr, nu, S, score.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<int32_t> h_col(static_cast<size_t>(n_pick)), h_flags(2);
  std::vector<double> h_gain(n_res);
  if (n_pick > 0) HIP_CHECK(hipMemcpyAsync(h_col.data(), res_col.ptr, sizeof(int32_t) * n_pick, hipMemcpyDeviceToHost, st));
  if (n_res > 0) HIP_CHECK(hipMemcpyAsync(h_gain.data(), res_gain.ptr, sizeof(double) * n_res, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_flags.data(), flags.ptr, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(served_items, served.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(served_scores, score.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_ASSORT] = ev.ms() + ct.ms;
  for (size_t m = 0; m + 1 < marks.size(); ++m) {  // gain + join, pick, update: in turn
    float v = 0.f;
    HIP_CHECK(hipEventElapsedTime(&v, marks[m]->e, marks[m + 1]->e));
    c->asrt_ms[m % 3] += v;
  }
  const int cnt = rounds ? h_flags[1] : 0;
  *count = cnt;
  if (rounds) *stop = h_flags[0];  // (0: all n_pick rounds ran)
  for (int k = 0; k < cnt; ++k) {
    items[k] = item_of(cand, h_col[static_cast<size_t>(k)]);
    gains[k] = h_gain[static_cast<size_t>(k)];
  }
  for (int g = 0; g < n_given; ++g) given_gains[g] = h_gain[static_cast<size_t>(n_pick) + g];
}

}  // namespace mmsbm_hip_impl
