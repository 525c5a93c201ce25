// serve_plan.hpp -- the launch plans of the serving queries (serve_frame.hpp) as plain values: the batches of a top-N
// query and its item split, the selection's list and scratch (SelectPlan), the blocks / runs / fragments of a group query, the COUNT batches and
// WRITE runs of an audience query, the rows per call of a diversified query.  Host arithmetic on plain numbers only -- no
// HIP type, no context -- so that the rules a kernel's block index depends on are checked on the CPU over every shape
// (tests/native/serve_plan_check.cpp).  The shape constants the plans share with the kernels are defined here, once.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mmsbm_hip_impl {

constexpr int kRecTile = 128;     // users x items of one score workgroup (recommend.hpp)
constexpr int kRecTm = 8;         // outputs per thread along each side (16 x 16 threads)
constexpr int kRecWave = 64;      // rec_select_kernel: one wave per workgroup
constexpr int kRecPerLane = 4;    // elements a lane examines per round
constexpr int kGrpBlock = kRecTm;               // group.hpp: member rows per block, the rows one thread of the tile holds
constexpr int kGrpStep = kRecTile / kGrpBlock;  // blocks per step of the walk (16)
constexpr int kGrpLast = 16;      // blk_info: bit set on the last block of a group (of a fragment of a cut group); low
                                  // bits: the block's members
constexpr int kGrpPart = 32;      // blk_info: the block belongs to a fragment of a cut group

constexpr size_t kRecBatchBytes = size_t(128) << 20;  // score buffer of one batch of users (stays in the 256 MB MALL)
constexpr size_t kAudTableBytes = size_t(64) << 20;   // recommend_audience: the (row, user tile) counts of one batch
constexpr size_t kFreeMargin = size_t(64) << 20;      // device memory a query leaves free (require_free_mem)
constexpr int kRecMinPerPart = 1024;                  // items a selecting wave gets at least
constexpr int kPosMinPerPart = 2048;                  // items a counting workgroup gets at least
constexpr int64_t kAudEntries = int64_t(16) << 20;    // recommend_audience: the entries of one WRITE batch (12 bytes each)

// ---- the batches of a top-N query and the selection ------------------------------------------------------------------
// users per batch: a score buffer of ~128 MB, whole 128-user tiles where that allows
inline int64_t rec_batch_users(int I, int64_t n_users) {
  int64_t bu = std::max<int64_t>(1, static_cast<int64_t>(kRecBatchBytes / (static_cast<size_t>(I) * sizeof(double))));
  bu = std::min<int64_t>(bu, 32768);
  if (bu >= kRecTile) bu = bu / kRecTile * kRecTile;
  return std::min(bu, n_users);
}

// (parts, per): the I items split into parts of at least min_per items each until about `target` (batch rows x
// parts) are in flight; few users: one user over 100k items
inline std::pair<int, int> item_parts(int I, int64_t bu, int64_t target, int min_per) {
  int parts = 1;
  if (bu < target) parts = static_cast<int>(std::min<int64_t>((target + bu - 1) / bu, (I + min_per - 1) / min_per));
  parts = std::max(parts, 1);
  const int per = (I + parts - 1) / parts;
  return {I > 0 ? (I + per - 1) / per : 1, per};
}

// The sorted list of a selecting wave (rec_select_kernel, cat_rank_kernel): the next power of two >= n + one round of
// the wave, a score and an id per place in LDS
inline std::pair<int, size_t> select_list(int n) {  // (places, LDS bytes)
  int cap = 1;
  while (cap < n + kRecWave * kRecPerLane) cap <<= 1;
  return {cap, static_cast<size_t>(cap) * (sizeof(double) + sizeof(int32_t))};
}

// The selection of one batch (rec_select_kernel): the n best of every one of `rows` batch rows over `cols` columns.  The
// columns are split into `parts` parts of `per` (item_parts) until about `target` selecting waves are in flight; with
// more than one part every (row, part) leaves a list of n places (`entries` in all, a score and an id each) and a count
// (`lists`) that a second launch merges; one part selects straight into the result and needs no places.
struct SelectPlan {
  int cols = 0, parts = 1, per = 0;
  size_t entries = 0, lists = 0;
  SelectPlan() = default;  // (a selection that never runs: no scratch)
  SelectPlan(int cols_, int64_t rows, int n, int min_per, int64_t target) : cols(cols_) {
    const std::pair<int, int> split = item_parts(cols, rows, target, min_per);
    parts = split.first;
    per = split.second;
    lists = static_cast<size_t>(rows) * parts;
    entries = parts > 1 ? lists * n : 0;
  }
  size_t bytes() const { return entries * (sizeof(double) + sizeof(int32_t)) + lists * sizeof(int32_t); }
};

// ---- per-category caps (quota.hpp) -------------------------------------------------------------------------------------
// What a query with capped categories uploads and launches with.  The categories are the caller's, as catalogue items
// (each strictly ascending, no item in two of them: checked by the C ABI); here they become COLUMNS of the query's batch
// buffer -- the item itself, or its place in the ascending candidate list (an item that is no candidate is dropped) --
// and a category that cannot change the answer is dropped: one with m <= q columns (never full) or with q >= n (never
// full within n picks).  The form of a kept category follows from (m, q) alone:
//   short  m <= kQuotaShortMax: a sub-wave group of quota_width(m) lanes, 64 / width categories to a wave.  The short
//          categories stand first, by ascending width, so that a wave's categories share one width;
//   long   m >  kQuotaShortMax: one wave per (row, category) with a sorted list of q places.
constexpr int kQuotaShortMax = kRecWave;  // columns of the largest category that shares a wave with others
enum QuotaForm { kQuotaDropped = 0, kQuotaShort = 1, kQuotaLong = 2 };

inline int quota_width(int m) {  // lanes of a short category: the next power of two >= m
  int w = 1;
  while (w < m) w <<= 1;
  return w;
}
inline QuotaForm quota_form(int m, int q, int n) {
  if (m <= q || q >= n) return kQuotaDropped;
  return m <= kQuotaShortMax ? kQuotaShort : kQuotaLong;
}

struct QuotaPlan {
  std::vector<int32_t> cat;             // per kept category: its place in the caller's request
  std::vector<int32_t> off, col, cap;   // the kept categories' columns (CSR, ascending inside a category) and caps
  int n_short = 0;                      // the first n_short kept categories take the short form, the others the long one
  std::vector<int32_t> wave_first, wave_info;  // short form, per wave: its first category; width | categories << 8
  int long_cap = 0;                     // the largest cap of a long category (sizes the waves' list)
  int kept() const { return static_cast<int>(cat.size()); }
  int n_long() const { return kept() - n_short; }
  size_t bytes() const { return (off.size() + col.size() + cap.size() + wave_first.size() + wave_info.size()) * sizeof(int32_t); }
};

// cand: the query's ascending candidate list (null: the columns are the items)
inline QuotaPlan plan_quota(const int32_t *cand, int n_cand, int64_t n_cats, const int64_t *cat_off,
                            const int32_t *cat_items, const int32_t *caps, int n) {
  QuotaPlan p;
  std::vector<int32_t> cols;                // every category's columns, in request order
  std::vector<int64_t> begin(static_cast<size_t>(n_cats) + 1, 0);
  std::vector<int> form(static_cast<size_t>(n_cats), kQuotaDropped);
  for (int64_t g = 0; g < n_cats; ++g) {
    for (int64_t e = cat_off[g]; e < cat_off[g + 1]; ++e) {
      if (!cand) {
        cols.push_back(cat_items[e]);
      } else {
        const int32_t *at = std::lower_bound(cand, cand + n_cand, cat_items[e]);
        if (at != cand + n_cand && *at == cat_items[e]) cols.push_back(static_cast<int32_t>(at - cand));
      }
    }
    begin[static_cast<size_t>(g) + 1] = static_cast<int64_t>(cols.size());
    const int64_t m = begin[static_cast<size_t>(g) + 1] - begin[static_cast<size_t>(g)];
    form[static_cast<size_t>(g)] = quota_form(static_cast<int>(std::min<int64_t>(m, INT32_MAX)), caps[g], n);
  }
  auto keep = [&](int64_t g) {
    p.cat.push_back(static_cast<int32_t>(g));
    p.off.push_back(static_cast<int32_t>(p.col.size()));
    p.col.insert(p.col.end(), cols.begin() + begin[static_cast<size_t>(g)], cols.begin() + begin[static_cast<size_t>(g) + 1]);
    p.cap.push_back(caps[g]);
  };
  for (int w = 1; w <= kQuotaShortMax; w <<= 1) {  // the short categories by ascending width, 64 / w of them to a wave
    const int first = p.kept();
    for (int64_t g = 0; g < n_cats; ++g)
      if (form[static_cast<size_t>(g)] == kQuotaShort &&
          quota_width(static_cast<int>(begin[static_cast<size_t>(g) + 1] - begin[static_cast<size_t>(g)])) == w)
        keep(g);
    const int per = kRecWave / w;
    for (int g0 = first; g0 < p.kept(); g0 += per) {
      p.wave_first.push_back(g0);
      p.wave_info.push_back(w | (std::min(per, p.kept() - g0) << 8));
    }
  }
  p.n_short = p.kept();
  for (int64_t g = 0; g < n_cats; ++g)
    if (form[static_cast<size_t>(g)] == kQuotaLong) {
      keep(g);
      p.long_cap = std::max(p.long_cap, caps[g]);
    }
  p.off.push_back(static_cast<int32_t>(p.col.size()));
  return p;
}

// ---- category-level recommendation (shelves.hpp) ---------------------------------------------------------------------------
// What a shelves query uploads and launches with.  The categories are the caller's, as catalogue items (each strictly
// ascending, no item in two of them: checked by the C ABI); here they become COLUMNS of the query's batch buffer as in
// plan_quota (an item that is no candidate is dropped), and a category left without a column is dropped: no row can show
// it.  The kept categories stand in plan_quota's order -- the short ones (m <= kQuotaShortMax) by ascending width,
// 64 / width to a wave, the long ones behind them -- but their VALUE COLUMNS (slot) follow the caller's order, so that
// the selection's tie rule over the value buffer, ascending column, is "ascending category index of the call".
struct ShelfPlan {
  std::vector<int64_t> cat;             // per kept category: its place in the caller's request
  std::vector<int32_t> slot;            // per kept category: its column of the value buffer
  std::vector<int32_t> of_slot;         // per value column: the kept category that writes it
  std::vector<int32_t> off, col;        // the kept categories' columns (CSR, ascending inside a category)
  int n_short = 0;                      // the first n_short kept categories take the short form, the others the long one
  std::vector<int32_t> wave_first, wave_info;  // short form, per wave: its first category; width | categories << 8
  int kept() const { return static_cast<int>(cat.size()); }
  int n_long() const { return kept() - n_short; }
  size_t bytes() const {
    return (slot.size() + of_slot.size() + off.size() + col.size() + wave_first.size() + wave_info.size()) * sizeof(int32_t);
  }
};

// cand: the query's ascending candidate list (null: the columns are the items)
inline ShelfPlan plan_shelves(const int32_t *cand, int n_cand, int64_t n_cats, const int64_t *cat_off,
                              const int32_t *cat_items) {
  ShelfPlan p;
  std::vector<int32_t> cols;                // every category's columns, in request order
  std::vector<int64_t> begin(static_cast<size_t>(n_cats) + 1, 0);
  std::vector<int32_t> rank(static_cast<size_t>(n_cats), -1);  // a category's place among those with a column
  int32_t n_kept = 0;
  for (int64_t g = 0; g < n_cats; ++g) {
    for (int64_t e = cat_off[g]; e < cat_off[g + 1]; ++e) {
      if (!cand) {
        cols.push_back(cat_items[e]);
      } else {
        const int32_t *at = std::lower_bound(cand, cand + n_cand, cat_items[e]);
        if (at != cand + n_cand && *at == cat_items[e]) cols.push_back(static_cast<int32_t>(at - cand));
      }
    }
    begin[static_cast<size_t>(g) + 1] = static_cast<int64_t>(cols.size());
    if (begin[static_cast<size_t>(g) + 1] > begin[static_cast<size_t>(g)]) rank[static_cast<size_t>(g)] = n_kept++;
  }
  auto size_of = [&](int64_t g) { return begin[static_cast<size_t>(g) + 1] - begin[static_cast<size_t>(g)]; };
  p.of_slot.resize(static_cast<size_t>(n_kept));
  auto keep = [&](int64_t g) {
    p.of_slot[static_cast<size_t>(rank[static_cast<size_t>(g)])] = p.kept();
    p.cat.push_back(g);
    p.slot.push_back(rank[static_cast<size_t>(g)]);
    p.off.push_back(static_cast<int32_t>(p.col.size()));
    p.col.insert(p.col.end(), cols.begin() + begin[static_cast<size_t>(g)], cols.begin() + begin[static_cast<size_t>(g) + 1]);
  };
  for (int w = 1; w <= kQuotaShortMax; w <<= 1) {  // the short categories by ascending width, 64 / w of them to a wave
    const int first = p.kept();
    for (int64_t g = 0; g < n_cats; ++g)
      if (size_of(g) > 0 && size_of(g) <= kQuotaShortMax && quota_width(static_cast<int>(size_of(g))) == w) keep(g);
    const int per = kRecWave / w;
    for (int g0 = first; g0 < p.kept(); g0 += per) {
      p.wave_first.push_back(g0);
      p.wave_info.push_back(w | (std::min(per, p.kept() - g0) << 8));
    }
  }
  p.n_short = p.kept();
  for (int64_t g = 0; g < n_cats; ++g)
    if (size_of(g) > kQuotaShortMax) keep(g);
  p.off.push_back(static_cast<int32_t>(p.col.size()));
  return p;
}

// ---- capacity-aware allocation (allocate.hpp) ----------------------------------------------------------------------------
// What recommend_allocate makes of the caller's caps, one per catalogue item, for a request of n_users users: a negative
// cap and a cap >= n_users never bind (every user of the request may hold the item), cap 0 closes the item, and the
// items in between are the CAPPED ones -- the rows of the item pass, in batches of rec_batch_users over the U user
// columns, each batch selecting with n = its largest cap.  A cap that binds beyond max_n places is not supported.
struct AllocPlan {
  std::vector<int32_t> item, cap;  // the capped items, ascending, and their caps (1 .. min(max_n, n_users - 1))
  std::vector<int32_t> closed;     // the items with cap 0
  int64_t refused = -1;            // the first item whose cap lies in (max_n, n_users); nothing below is filled in
  int64_t bi = 0;                  // capped items per batch of the item pass
  std::vector<int32_t> batch_n;    // per batch: its largest cap
  int most_n = 0;                  // the largest cap of all
  int64_t capped() const { return static_cast<int64_t>(item.size()); }
};

// force_bi > 0: that many items per batch instead of rec_batch_users (the CPU check: batches without 128 MB shapes)
inline AllocPlan plan_allocate(const int32_t *caps, int n_items, int64_t n_users, int U, int max_n, int64_t force_bi = 0) {
  AllocPlan p;
  for (int i = 0; i < n_items; ++i) {
    const int64_t q = caps[i];
    if (q < 0 || q >= n_users) continue;
    if (q > max_n) {
      AllocPlan none;
      none.refused = i;
      return none;
    }
    if (q == 0) {
      p.closed.push_back(i);
    } else {
      p.item.push_back(i);
      p.cap.push_back(static_cast<int32_t>(q));
    }
  }
  if (p.item.empty()) return p;
  p.bi = force_bi > 0 ? std::min(force_bi, p.capped()) : rec_batch_users(U, p.capped());
  for (int64_t r0 = 0; r0 < p.capped(); r0 += p.bi) {
    const int64_t r1 = std::min(p.capped(), r0 + p.bi);
    p.batch_n.push_back(*std::max_element(p.cap.begin() + r0, p.cap.begin() + r1));
    p.most_n = std::max(p.most_n, p.batch_n.back());
  }
  return p;
}

// ---- welfare-maximising assignment (assign.hpp) -------------------------------------------------------------------------
// What recommend_assign makes of the caller's caps (plan_allocate's reading of them): per item -1 (unlimited: negative
// or >= n_users), 0 (closed) or its cap, and the binding items' slots one after the other.
struct AssignPlan {
  std::vector<int32_t> cap;       // per catalogue item: -1, 0, or 1 .. min(max_n, n_users - 1)
  std::vector<int32_t> slot_off;  // [items + 1]: the item's slots (none for -1 and 0)
  int64_t refused = -1;           // the first item whose cap lies in (max_n, n_users); nothing else is filled in
  int most = 0;                   // the largest binding cap
  int lds_places() const {        // assign_accept_kernel's list: a power of two >= most, at least 2
    int p = 2;
    while (p < most) p <<= 1;
    return p;
  }
  size_t slots() const { return slot_off.empty() ? 0 : static_cast<size_t>(slot_off.back()); }
};

inline AssignPlan plan_assign(const int32_t *caps, int n_items, int64_t n_users, int max_n) {
  AssignPlan p;
  p.cap.assign(static_cast<size_t>(n_items), -1);
  p.slot_off.assign(static_cast<size_t>(n_items) + 1, 0);
  int64_t total = 0;
  for (int i = 0; i < n_items; ++i) {
    const int64_t q = caps[i];
    if (q >= 0 && q < n_users) {
      if (q > max_n) {
        AssignPlan none;
        none.refused = i;
        return none;
      }
      p.cap[static_cast<size_t>(i)] = static_cast<int32_t>(q);
      p.most = std::max(p.most, static_cast<int>(q));
      total += q;
    }
    if (total > INT32_MAX) {  // (n_items x max_n slots: beyond int32 offsets)
      AssignPlan none;
      none.refused = i;
      return none;
    }
    p.slot_off[static_cast<size_t>(i) + 1] = static_cast<int32_t>(total);
  }
  return p;
}

// ---- group queries (group.hpp) -----------------------------------------------------------------------------------------
// What recommend_query_groups uploads and launches with.  The rows of the device request are the groups that have
// members (an empty group has no candidate); their members stand in blocks of kGrpBlock rows, a group's last block
// filled up with its first member's id (a row that can be loaded; the kernels never look at it: `info` holds the number
// of members).  With `tiles` (every mode but the mean) each batch of `bu` rows is walked in runs of about `want` blocks
// -- whole steps of the walk, about 8 workgroups per CU over the item tiles (option "group_run_blocks") -- made of whole
// groups; a group longer than that is cut into fragments of `want` blocks, one run each, whose values meet in
// grp_combine_kernel.
struct GroupPlan {
  std::vector<int64_t> at;    // per row: its place in the caller's request
  std::vector<int32_t> ids;   // 0 .. G - 1: the rows as top_n_run's request
  size_t n_blocks = 0;        // more than 2^31 - 1 member rows (too_large): nothing below is filled in
  bool too_large() const { return n_blocks * kGrpBlock > static_cast<size_t>(INT32_MAX); }
  std::vector<int32_t> rows, info, grp;  // [block][kGrpBlock] member ids; per block: members | kGrpLast | kGrpPart; its row
  std::vector<int32_t> out;              // per block: the row the tile kernel writes (a group, or a fragment)
  std::vector<int32_t> gblk, gsize;      // per row: its first block (G + 1 entries), its members
  int64_t bu = 0, item_tiles = 0;        // rows per batch (what top_n_device will form); 128-column tiles of the C columns
  std::vector<int32_t> want;             // per batch: blocks per run
  std::vector<int32_t> run_off, batch_run;            // the runs' first blocks; the batches' first runs
  std::vector<int32_t> cut_grp, cut_off, batch_cut;   // the cut groups, their first fragments; the batches' first cut groups
  int32_t most_frag = 0;                 // fragments of the batch with the most
  int64_t groups() const { return static_cast<int64_t>(at.size()); }
};

// force_bu > 0: that many rows per batch instead of rec_batch_users (the CPU check: batches without 128 MB shapes)
inline GroupPlan plan_groups(const int64_t *offsets, const int32_t *members, int64_t n_groups, int C, int n_cus,
                             int64_t run_blocks, bool tiles, int64_t force_bu = 0) {
  GroupPlan p;
  for (int64_t g = 0; g < n_groups; ++g)
    if (offsets[g + 1] > offsets[g]) {
      p.ids.push_back(static_cast<int32_t>(p.at.size()));
      p.at.push_back(g);
    }
  const int64_t G = p.groups();
  if (G == 0 || C == 0) return p;  // (no row or no column to score)
  for (int64_t r = 0; r < G; ++r)
    p.n_blocks += static_cast<size_t>((offsets[p.at[r] + 1] - offsets[p.at[r]] + kGrpBlock - 1) / kGrpBlock);
  if (p.too_large()) return p;
  p.gblk.resize(static_cast<size_t>(G) + 1);
  p.gsize.resize(static_cast<size_t>(G));
  p.rows.reserve(p.n_blocks * kGrpBlock);
  for (int64_t r = 0; r < G; ++r) {
    const int32_t *m = members + offsets[p.at[r]];
    const int64_t sz = offsets[p.at[r] + 1] - offsets[p.at[r]];
    p.gblk[static_cast<size_t>(r)] = static_cast<int32_t>(p.info.size());
    p.gsize[static_cast<size_t>(r)] = static_cast<int32_t>(sz);
    for (int64_t k = 0; k < sz; k += kGrpBlock) {
      const int in = static_cast<int>(std::min<int64_t>(kGrpBlock, sz - k));
      for (int a = 0; a < kGrpBlock; ++a) p.rows.push_back(a < in ? m[k + a] : m[0]);
      p.info.push_back(in | (k + kGrpBlock >= sz ? kGrpLast : 0));
      p.grp.push_back(static_cast<int32_t>(r));
    }
  }
  p.gblk[static_cast<size_t>(G)] = static_cast<int32_t>(p.info.size());
  p.out = p.grp;
  p.bu = force_bu > 0 ? std::min(force_bu, G) : rec_batch_users(C, G);
  p.item_tiles = (static_cast<int64_t>(C) + kRecTile - 1) / kRecTile;
  if (!tiles) return p;
  int32_t n_frag = 0;  // fragments so far
  for (int64_t b0 = 0; b0 < G; b0 += p.bu) {
    const int64_t b1 = std::min(G, b0 + p.bu);
    const int64_t blocks = p.gblk[static_cast<size_t>(b1)] - p.gblk[static_cast<size_t>(b0)];
    const int64_t most = std::max<int64_t>(1, 8LL * n_cus / p.item_tiles);
    const int64_t ask = run_blocks > 0 ? run_blocks : (blocks + most - 1) / most;
    const int32_t want = static_cast<int32_t>(
        std::max<int64_t>(kGrpStep, (std::min<int64_t>(ask, blocks) + kGrpStep - 1) / kGrpStep * kGrpStep));
    p.want.push_back(want);
    p.batch_run.push_back(static_cast<int32_t>(p.run_off.size()));
    p.batch_cut.push_back(static_cast<int32_t>(p.cut_grp.size()));
    const int32_t frag0 = n_frag;
    int32_t first = p.gblk[static_cast<size_t>(b0)];
    p.run_off.push_back(first);
    auto begin_run = [&](int32_t blk) {  // (nothing where a run begins there already)
      if (blk > first) p.run_off.push_back(first = blk);
    };
    for (int64_t r = b0; r < b1; ++r) {
      const int32_t g_lo = p.gblk[static_cast<size_t>(r)], g_hi = p.gblk[static_cast<size_t>(r) + 1];
      if (g_hi - g_lo > want) {
        p.cut_grp.push_back(static_cast<int32_t>(r));
        p.cut_off.push_back(n_frag);
        for (int32_t lo = g_lo; lo < g_hi; lo += want, ++n_frag) {
          const int32_t hi = std::min(g_hi, lo + want);
          begin_run(lo);
          for (int32_t b = lo; b < hi; ++b) {
            p.info[static_cast<size_t>(b)] |= kGrpPart;
            p.out[static_cast<size_t>(b)] = n_frag;
          }
          p.info[static_cast<size_t>(hi) - 1] |= kGrpLast;
        }
        if (r + 1 < b1) begin_run(g_hi);
      } else if (g_hi - first >= want && r + 1 < b1) {
        begin_run(g_hi);
      }
    }
    p.most_frag = std::max(p.most_frag, n_frag - frag0);
  }
  p.batch_run.push_back(static_cast<int32_t>(p.run_off.size()));
  p.run_off.push_back(p.gblk[static_cast<size_t>(G)]);  // (one past the last run; a batch's last run ends where the next batch's first begins)
  p.batch_cut.push_back(static_cast<int32_t>(p.cut_grp.size()));
  p.cut_off.push_back(n_frag);
  return p;
}

// ---- greedy assortment selection (assortment.hpp) --------------------------------------------------------------------------
// What recommend_assortment launches with.  The request's users stand as ONE list of rows, ascending by id; the gain
// kernel walks it in runs of `run_rows` rows -- whole 128-row steps, about 8 workgroups per CU over the item tiles
// (option "assortment_run_blocks": 8-row blocks per run, rounded up to whole steps of 16) -- and never more runs than a
// grid's second dimension holds.  A run's carry goes to a row of the partial buffer [runs][cols]; where runs x columns
// is beyond kAsrtPartBytes the item tiles are walked in batches of `batch_tiles`, each joined before the next overwrites
// the buffer.  The join leaves one entry per 256 columns (n_blk in all), the pick reads them.
constexpr int kAsrtNoGain = 1, kAsrtNoCand = 2;           // the stop flag (0: running); MMSBM_HIP_ASSORT_STOP_*
constexpr size_t kAsrtPartBytes = size_t(64) << 20;       // the partial buffer of one batch of item tiles
constexpr int64_t kAsrtMaxRuns = 65535;                   // gridDim.y
constexpr int kAsrtJoin = 256;                            // columns per workgroup of asrt_join_kernel (kBlock)

struct AssortPlan {
  int64_t n_rows = 0, n_blocks = 0, item_tiles = 0;  // users; their 8-row blocks; 128-column tiles of the C columns
  int64_t run_blocks = 0, run_rows = 0, runs = 0;    // per run: blocks (a multiple of kGrpStep), rows; the runs
  int64_t batch_tiles = 0, batches = 0;              // item tiles per launch of the gain kernel; launches per round
  int64_t ld = 0;                                    // columns of the partial buffer: batch_tiles x 128
  std::vector<int32_t> batch_blk;                    // per batch: its first entry of the join's output (batches + 1)
  int64_t n_blk() const { return batch_blk.empty() ? 0 : batch_blk.back(); }
  size_t part_doubles() const { return static_cast<size_t>(runs) * static_cast<size_t>(ld); }
  // columns of batch b of a table of C columns: [col0, col0 + n)
  std::pair<int64_t, int64_t> batch_cols(int64_t b, int64_t C) const {
    const int64_t col0 = b * batch_tiles * kRecTile;
    return {col0, std::min<int64_t>(C, col0 + batch_tiles * kRecTile) - col0};
  }
};

// part_bytes: kAsrtPartBytes (the CPU check: batches without 64 MB shapes).  n_rows == 0 or C == 0: nothing to launch.
inline AssortPlan plan_assortment(int64_t n_rows, int64_t C, int n_cus, int64_t run_blocks_option,
                                  size_t part_bytes = kAsrtPartBytes) {
  AssortPlan p;
  p.n_rows = n_rows;
  if (n_rows <= 0 || C <= 0) return p;
  p.n_blocks = (n_rows + kGrpBlock - 1) / kGrpBlock;
  p.item_tiles = (C + kRecTile - 1) / kRecTile;
  const int64_t most = std::max<int64_t>(1, 8LL * n_cus / p.item_tiles);
  int64_t ask = run_blocks_option > 0 ? run_blocks_option : (p.n_blocks + most - 1) / most;
  ask = std::max(ask, (p.n_blocks + kAsrtMaxRuns - 1) / kAsrtMaxRuns);
  p.run_blocks = std::max<int64_t>(kGrpStep, (std::min(ask, p.n_blocks) + kGrpStep - 1) / kGrpStep * kGrpStep);
  p.run_rows = p.run_blocks * kGrpBlock;
  p.runs = (p.n_blocks + p.run_blocks - 1) / p.run_blocks;
  const int64_t fit = static_cast<int64_t>(part_bytes / sizeof(double)) / p.runs / kRecTile;
  p.batch_tiles = std::min(p.item_tiles, std::max<int64_t>(1, fit));
  p.batches = (p.item_tiles + p.batch_tiles - 1) / p.batch_tiles;
  p.ld = p.batch_tiles * kRecTile;
  p.batch_blk.push_back(0);
  for (int64_t b = 0; b < p.batches; ++b)
    p.batch_blk.push_back(p.batch_blk.back() + static_cast<int32_t>((p.batch_cols(b, C).second + kAsrtJoin - 1) / kAsrtJoin));
  return p;
}

// ---- the spread of given pairs (ensemble.hpp) ----------------------------------------------------------------------------
// pairs per launch of recommend_pair_spread: the batch's ids, four numbers a pair and, when wanted, the S slots' values
// stay within kEnsPairBytes (at least one pair)
constexpr size_t kEnsPairBytes = size_t(256) << 20;
inline size_t ens_pair_bytes(int slots, bool per_slot) { return 8 + 32 + (per_slot ? static_cast<size_t>(slots) * 8 : 0); }
inline int64_t ens_pairs_per_launch(int64_t n_pairs, int slots, bool per_slot) {
  return std::min<int64_t>(n_pairs, std::max<int64_t>(1, static_cast<int64_t>(kEnsPairBytes / ens_pair_bytes(slots, per_slot))));
}

// ---- item-side queries (audience.hpp) ----------------------------------------------------------------------------------
// items per COUNT batch of recommend_audience: option "audience_rows", else whole 128-row tiles while the batch's
// (row, user tile) counts stay within kAudTableBytes
inline int64_t aud_count_rows(int U, int64_t rows_option, int64_t n_items) {
  const int64_t n_ut = (static_cast<int64_t>(U) + kRecTile - 1) / kRecTile;
  int64_t rb = rows_option;
  if (rb <= 0)
    rb = std::max<int64_t>(kRecTile, static_cast<int64_t>(kAudTableBytes / sizeof(int32_t)) / n_ut / kRecTile * kRecTile);
  return std::min(rb, n_items);
}

// The WRITE runs of one COUNT batch: consecutive rows whose entries stay under the cap (a larger row goes alone).  A
// run without entries has nothing to write.
struct AudRun {
  int first, rows;
  int64_t entries;
};
inline std::vector<AudRun> aud_write_runs(const int32_t *counts, int nb, int64_t cap) {
  std::vector<AudRun> runs;
  for (int s0 = 0; s0 < nb;) {
    int64_t e = counts[s0];
    int s1 = s0 + 1;
    while (s1 < nb && e + counts[s1] <= cap) e += counts[s1++];
    runs.push_back({s0, s1 - s0, e});
    s0 = s1;
  }
  return runs;
}

// ---- diversified top-N (diverse.hpp) -------------------------------------------------------------------------------------
// bytes a request row of recommend_diverse holds on the device: the pool list (12 bytes a place) and the picks (20 an entry)
inline size_t div_row_bytes(int pool, int n) { return static_cast<size_t>(pool) * 12 + static_cast<size_t>(n) * 20 + 16; }

// rows per call: option "diverse_rows", else all of them unless that is not free beside a batch's score buffer -- then
// halves of the request until it is (a row's answer does not depend on the other rows)
inline int64_t div_rows_per_call(int64_t rows_option, int64_t n_users, size_t free_bytes, size_t per_row) {
  if (rows_option > 0) return std::min(rows_option, n_users);
  int64_t rows_per = n_users;
  while (rows_per > 1 && static_cast<size_t>(rows_per) * per_row + kRecBatchBytes + kFreeMargin > free_bytes)
    rows_per = (rows_per + 1) / 2;
  return rows_per;
}

}  // namespace mmsbm_hip_impl
