// Host-only check of mmsbm_amd/csrc/serve_plan.hpp, built with -fsanitize=address,undefined by
// tests/test_serve_plan_cpu.py.  Sweeps the serving queries' plans -- the batches and item parts of a top-N query, the
// selection's list, the blocks / runs / fragments of a group query, the WRITE runs of an audience query, the rows per call
// of a diversified query -- and checks each against a restatement of what the kernels rely on, written from the sizes of
// the request and not from the plan's own loops.  A few plans are pinned value by value.
#include <cstdio>

#include "../../mmsbm_amd/csrc/serve_plan.hpp"

using namespace mmsbm_hip_impl;

static long fails = 0;
static long g_case = 0;   // counts the plans checked; printed with a failure
#define CHECK(x)                                                                                                       \
  do {                                                                                                                 \
    if (!(x) && ++fails <= 20) std::printf("FAILED %s (case %ld) line %d\n", #x, g_case, __LINE__);                     \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- 1. batches, item parts, the selection's list ---------------------------------------------------------------------
static void check_batch(int I, int64_t n_users, int n_cus) {
  ++g_case;
  const int64_t bu = rec_batch_users(I, n_users);
  CHECK(bu >= 1 && bu <= std::min<int64_t>(n_users, 32768));
  const int64_t fit = std::min<int64_t>((int64_t(128) << 20) / (int64_t(I) * 8), 32768);  // rows the buffer holds
  if (fit >= 128) {
    const int64_t whole = fit - fit % 128;
    if (n_users >= whole) CHECK(bu == whole && bu % 128 == 0);
    else CHECK(bu == n_users);
  } else {
    CHECK(bu == std::min<int64_t>(std::max<int64_t>(fit, 1), n_users));
  }
  CHECK(bu * int64_t(I) * 8 <= (int64_t(128) << 20) || bu == 1);
  const int64_t targets[2] = {32LL * n_cus, 8LL * n_cus};
  const int min_pers[2] = {1024, 2048};
  for (int t = 0; t < 2; ++t) {
    const auto [parts, per] = item_parts(I, bu, targets[t], min_pers[t]);
    CHECK(parts >= 1 && per >= 1);
    CHECK(int64_t(parts) * per >= I && int64_t(parts - 1) * per < I);
    if (bu >= targets[t]) CHECK(parts == 1);
    CHECK(parts <= ceil_div(I, min_pers[t]) && parts <= std::max<int64_t>(1, ceil_div(targets[t], bu)));
    // the selection's plan: item_parts' split, and a scratch of n places per (row, part) exactly when the parts are merged
    for (int n : {1, 2, 10, 1024}) {
      const SelectPlan sp(I, bu, n, min_pers[t], targets[t]);
      CHECK(sp.cols == I && sp.parts == parts && sp.per == per);
      CHECK(int64_t(sp.parts) * sp.per >= I);
      CHECK(sp.lists == size_t(bu) * size_t(parts));
      CHECK((sp.entries == 0) == (sp.parts == 1));
      if (sp.parts > 1) CHECK(sp.entries == sp.lists * size_t(n));
      CHECK(sp.bytes() == 12 * sp.entries + 4 * size_t(bu) * size_t(parts));
    }
  }
}

static void check_batches() {
  const int64_t users[] = {1, 2, 127, 128, 129, 3328, 3329, 1000000};
  const int cus[] = {1, 64, 256};
  auto over = [&](int I) {
    for (int64_t u : users)
      for (int n_cus : cus) check_batch(I, u, n_cus);
  };
  for (int I = 1; I <= 5000; ++I) over(I);
  over(70000);
  over(1 << 24);
  for (int n = 1; n <= 1024; ++n) {
    const auto [cap, lds] = select_list(n);
    CHECK(cap >= n + 256 && (cap & (cap - 1)) == 0 && cap / 2 < n + 256);
    CHECK(lds == size_t(cap) * 12);
  }
  // pinned: worked from the formulas of the commit before the plans moved here
  CHECK(rec_batch_users(5000, 1000000) == 3328);
  CHECK(rec_batch_users(70000, 129) == 128);
  CHECK(rec_batch_users(30, 5) == 5);
  CHECK(item_parts(5000, 2, 8192, 1024) == std::make_pair(5, 1000));
  CHECK(item_parts(5000, 3328, 8192, 1024) == std::make_pair(3, 1667));
  CHECK(item_parts(2049, 1, 8192, 1024) == std::make_pair(3, 683));
  CHECK(item_parts(2048, 1, 8192, 1024) == std::make_pair(2, 1024));
  CHECK(SelectPlan(5000, 3, 10, 1024, 8192).bytes() == size_t(3 * 5 * 10 * 12 + 3 * 5 * 4));  // 5 parts of 1,000
  CHECK(SelectPlan(129, 32768, 3, 1024, 8192).bytes() == size_t(32768 * 4));                 // one part: the counts alone
  CHECK(SelectPlan().bytes() == 0 && SelectPlan().parts == 1);
  CHECK(select_list(256) == std::make_pair(512, size_t(6144)));
  CHECK(select_list(257) == std::make_pair(1024, size_t(12288)));
  CHECK(select_list(769) == std::make_pair(2048, size_t(24576)));
}

// ---- 2. the group plan ------------------------------------------------------------------------------------------------
struct GroupRequest {
  std::vector<int64_t> off{0};
  std::vector<int32_t> mem;
  void add(int size) {  // distinct ids, not in ascending order: 1000 g + 7, then downwards from 1000 g + 999
    const int32_t g = static_cast<int32_t>(off.size()) - 1;
    for (int j = 0; j < size; ++j) mem.push_back(j == 0 ? 1000 * g + 7 : 1000 * g + 1000 - j);
    off.push_back(static_cast<int64_t>(mem.size()));
  }
  int64_t groups() const { return static_cast<int64_t>(off.size()) - 1; }
  int64_t size(int64_t g) const { return off[g + 1] - off[g]; }
};

static void check_group_plan(const GroupRequest &q, int C, int n_cus, int64_t opt, bool tiles, int64_t force_bu) {
  ++g_case;
  const GroupPlan p = plan_groups(q.off.data(), q.mem.data(), q.groups(), C, n_cus, opt, tiles, force_bu);
  // the rows: the groups that have members, ascending
  std::vector<int64_t> at;
  for (int64_t g = 0; g < q.groups(); ++g)
    if (q.size(g) > 0) at.push_back(g);
  CHECK(p.at == at);
  const int64_t G = static_cast<int64_t>(at.size());
  CHECK(static_cast<int64_t>(p.ids.size()) == G);
  for (int64_t r = 0; r < G; ++r) CHECK(p.ids[r] == r);
  if (G == 0) {
    CHECK(p.rows.empty() && p.info.empty() && p.run_off.empty());
    return;
  }
  CHECK(!p.too_large());
  // the blocks
  CHECK(static_cast<int64_t>(p.gblk.size()) == G + 1 && static_cast<int64_t>(p.gsize.size()) == G && p.gblk[0] == 0);
  int64_t nblk = 0;
  for (int64_t r = 0; r < G; ++r) {
    const int64_t sz = q.size(at[r]);
    CHECK(p.gsize[r] == sz && p.gblk[r] == nblk && p.gblk[r + 1] - p.gblk[r] == ceil_div(sz, 8));
    nblk += ceil_div(sz, 8);
  }
  CHECK(p.gblk[G] == nblk && static_cast<int64_t>(p.n_blocks) == nblk);
  CHECK(static_cast<int64_t>(p.info.size()) == nblk && static_cast<int64_t>(p.grp.size()) == nblk &&
        static_cast<int64_t>(p.out.size()) == nblk && static_cast<int64_t>(p.rows.size()) == nblk * 8);
  if (static_cast<int64_t>(p.info.size()) != nblk || static_cast<int64_t>(p.rows.size()) != nblk * 8 ||
      static_cast<int64_t>(p.out.size()) != nblk || static_cast<int64_t>(p.grp.size()) != nblk)
    return;
  // the batches
  const int64_t bu = force_bu > 0 ? std::min(force_bu, G) : G;  // (the sweep's shapes fit one 128 MB batch)
  CHECK(p.bu == bu && p.item_tiles == ceil_div(C, 128));
  const int64_t n_batch = ceil_div(G, bu);
  if (!tiles) {
    CHECK(p.run_off.empty() && p.batch_run.empty() && p.cut_grp.empty() && p.cut_off.empty() && p.batch_cut.empty() &&
          p.want.empty() && p.most_frag == 0);
  } else {
    CHECK(static_cast<int64_t>(p.want.size()) == n_batch && static_cast<int64_t>(p.batch_run.size()) == n_batch + 1 &&
          static_cast<int64_t>(p.batch_cut.size()) == n_batch + 1);
    if (static_cast<int64_t>(p.want.size()) != n_batch || static_cast<int64_t>(p.batch_run.size()) != n_batch + 1 ||
        static_cast<int64_t>(p.batch_cut.size()) != n_batch + 1)
      return;
  }
  // per block: what the kernels read, from the sizes alone
  std::vector<int32_t> cut_grp, cut_off;
  std::vector<int64_t> frag_blocks;  // blocks per fragment
  int32_t n_frag = 0, most_frag = 0;
  for (int64_t k = 0; k < n_batch; ++k) {
    const int64_t b0 = k * bu, b1 = std::min(G, b0 + bu);
    int32_t want = 0;
    if (tiles) {
      want = p.want[k];
      const int64_t blocks = p.gblk[b1] - p.gblk[b0], most = std::max<int64_t>(1, 8LL * n_cus / ceil_div(C, 128));
      const int64_t ask = std::min(opt > 0 ? opt : ceil_div(blocks, most), blocks);
      CHECK(want > 0 && want % 16 == 0 && want == std::max<int64_t>(16, ceil_div(ask, 16) * 16));
      if (want <= 0) return;
      CHECK(p.batch_cut[k] == static_cast<int32_t>(cut_grp.size()));
    }
    const int32_t frag0 = n_frag;
    for (int64_t r = b0; r < b1; ++r) {
      const int64_t sz = q.size(at[r]), gb = ceil_div(sz, 8);
      const bool cut = tiles && gb > want;
      if (cut) {
        cut_grp.push_back(static_cast<int32_t>(r));
        cut_off.push_back(n_frag);
      }
      const int32_t *m = q.mem.data() + q.off[at[r]];
      for (int64_t j = 0; j < gb; ++j) {
        const int64_t b = p.gblk[r] + j;
        const int live = static_cast<int>(std::min<int64_t>(8, sz - 8 * j));
        CHECK(live >= 1 && live <= 8 && (p.info[b] & 15) == live && p.grp[b] == r);
        for (int a = 0; a < 8; ++a) CHECK(p.rows[b * 8 + a] == (a < live ? m[8 * j + a] : m[0]));
        const bool last = cut ? (j % want == want - 1 || j == gb - 1) : j == gb - 1;
        CHECK(p.info[b] == (live | (last ? kGrpLast : 0) | (cut ? kGrpPart : 0)));
        CHECK(p.out[b] == (cut ? n_frag + static_cast<int32_t>(j / want) : static_cast<int32_t>(r)));
        if (cut && j % want == 0) frag_blocks.push_back(std::min<int64_t>(want, gb - j));
      }
      if (cut) n_frag += static_cast<int32_t>(ceil_div(gb, want));
    }
    most_frag = std::max(most_frag, n_frag - frag0);
  }
  if (!tiles) return;
  cut_off.push_back(n_frag);
  CHECK(p.cut_grp == cut_grp && p.cut_off == cut_off && p.most_frag == most_frag);
  CHECK(p.batch_cut[n_batch] == static_cast<int32_t>(cut_grp.size()) && p.cut_off.back() == n_frag);
  for (size_t i = 0; i + 1 < p.cut_off.size(); ++i) CHECK(p.cut_off[i] <= p.cut_off[i + 1]);
  CHECK(static_cast<int64_t>(frag_blocks.size()) == n_frag);
  // the runs: within each batch they partition the batch's blocks; whole uncut groups, or exactly one fragment
  CHECK(p.batch_run[0] == 0 && static_cast<int64_t>(p.run_off.size()) == p.batch_run[n_batch] + 1);
  if (static_cast<int64_t>(p.run_off.size()) != p.batch_run[n_batch] + 1) return;
  for (int64_t k = 0; k < n_batch; ++k) {
    const int64_t b0 = k * bu, b1 = std::min(G, b0 + bu);
    const int32_t r0 = p.batch_run[k], r1 = p.batch_run[k + 1];
    CHECK(r1 > r0 && p.run_off[r0] == p.gblk[b0] && p.run_off[r1] == p.gblk[b1]);
    for (int32_t r = r0; r < r1; ++r) {
      const int32_t lo = p.run_off[r], hi = p.run_off[r + 1];
      CHECK(lo < hi && lo >= p.gblk[b0] && hi <= p.gblk[b1]);
      if (!(lo < hi && lo >= 0 && hi <= nblk)) return;
      if (p.info[lo] & kGrpPart) {  // one fragment, all of it
        const int32_t f = p.out[lo];
        for (int32_t b = lo; b < hi; ++b) CHECK((p.info[b] & kGrpPart) && p.out[b] == f);
        CHECK(hi - lo == frag_blocks[f] && hi - lo <= p.want[k]);
        CHECK(lo == 0 || !(p.info[lo - 1] & kGrpPart) || p.out[lo - 1] != f);
        CHECK(hi == nblk || !(p.info[hi] & kGrpPart) || p.out[hi] != f);
      } else {  // whole groups, none of them cut
        for (int32_t b = lo; b < hi; ++b) CHECK(!(p.info[b] & kGrpPart));
        CHECK(lo == p.gblk[p.grp[lo]] && hi == p.gblk[p.grp[hi - 1] + 1]);
      }
    }
  }
}

static bool same(const std::vector<int32_t> &v, std::initializer_list<int32_t> w) { return v == std::vector<int32_t>(w); }

static void check_groups() {
  const int sizes[] = {0, 1, 7, 8, 9, 127, 128, 129, 300};
  const int cs[] = {1, 100, 5000}, cus[] = {1, 256};
  const int64_t opts[] = {0, 16, 32}, bus[] = {1, 2, 0};
  for (int n_groups = 1; n_groups <= 4; ++n_groups) {
    int total = 1;
    for (int g = 0; g < n_groups; ++g) total *= 9;
    for (int code = 0; code < total; ++code) {
      GroupRequest q;
      for (int g = 0, rest = code; g < n_groups; ++g, rest /= 9) q.add(sizes[rest % 9]);
      for (int C : cs)
        for (int n_cus : cus)
          for (int64_t opt : opts)
            for (int64_t bu : bus) check_group_plan(q, C, n_cus, opt, true, bu);
      for (int64_t bu : bus) check_group_plan(q, 100, 256, 0, false, bu);  // the mean: blocks only
    }
  }
  {  // pinned: worked from the loop of the commit before the plan moved here
    GroupRequest q;
    for (int s : {1, 2, 7, 8, 9, 127, 128, 129}) q.add(s);
    const GroupPlan p = plan_groups(q.off.data(), q.mem.data(), q.groups(), 5000, 256, 0, true);
    CHECK(same(p.want, {16}) && same(p.gblk, {0, 1, 2, 3, 4, 6, 22, 38, 55}) && same(p.run_off, {0, 22, 38, 54, 55}));
    CHECK(same(p.batch_run, {0, 4}) && same(p.cut_grp, {7}) && same(p.cut_off, {0, 2}) && same(p.batch_cut, {0, 1}));
    CHECK(p.most_frag == 2 && p.bu == 8);
  }
  {
    GroupRequest q;
    for (int s : {129, 1, 300}) q.add(s);
    const GroupPlan p = plan_groups(q.off.data(), q.mem.data(), q.groups(), 100, 256, 16, true);
    CHECK(same(p.gblk, {0, 17, 18, 56}) && same(p.run_off, {0, 16, 17, 18, 34, 50, 56}));
    CHECK(same(p.cut_grp, {0, 2}) && same(p.cut_off, {0, 2, 5}) && p.most_frag == 5);
  }
  {  // no column: the rows only
    GroupRequest q;
    q.add(3);
    const GroupPlan p = plan_groups(q.off.data(), q.mem.data(), q.groups(), 0, 256, 0, true);
    CHECK(p.groups() == 1 && p.rows.empty() && p.run_off.empty());
  }
}

// ---- 3. the audience plan -----------------------------------------------------------------------------------------------
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // [0, n)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>((g_rng >> 33) % n);
}

static void check_audience() {
  for (int64_t cap : {int64_t(1), int64_t(7), int64_t(100)})
    for (int rep = 0; rep < 400; ++rep) {
      ++g_case;
      const int nb = 1 + static_cast<int>(rnd(300));
      std::vector<int32_t> cnt(static_cast<size_t>(nb));
      for (int32_t &v : cnt) v = rnd(20) == 0 ? 1000 + static_cast<int32_t>(rnd(100000)) : static_cast<int32_t>(rnd(41));
      const std::vector<AudRun> runs = aud_write_runs(cnt.data(), nb, cap);
      int next = 0;
      for (size_t i = 0; i < runs.size(); ++i) {
        const AudRun &r = runs[i];
        CHECK(r.first == next && r.rows >= 1 && r.first + r.rows <= nb);
        if (r.first != next || r.rows < 1 || r.first + r.rows > nb) return;
        int64_t sum = 0;
        for (int j = 0; j < r.rows; ++j) sum += cnt[static_cast<size_t>(r.first + j)];
        CHECK(r.entries == sum);
        CHECK(sum <= cap || r.rows == 1);
        next = r.first + r.rows;
        if (next < nb) CHECK(sum + cnt[static_cast<size_t>(next)] > cap);
      }
      CHECK(next == nb);
    }
  // the COUNT batch: the option as it is, else whole 128-row tiles whose counts stay within the 64 MB table -- at least one
  for (int U : {1, 128, 129, 5000, 1000000, 40000000})
    for (int64_t n_items : {int64_t(1), int64_t(3), int64_t(129), int64_t(1) << 20}) {
      ++g_case;
      for (int64_t opt : {int64_t(1), int64_t(3), int64_t(5000)}) CHECK(aud_count_rows(U, opt, n_items) == std::min(opt, n_items));
      const int64_t rb = aud_count_rows(U, 0, n_items), n_ut = ceil_div(U, 128);
      CHECK(rb >= 1 && rb <= n_items);
      if (rb < n_items) CHECK(rb % 128 == 0 && (rb * n_ut * 4 <= (int64_t(64) << 20) || rb == 128));
      if (rb < n_items && rb > 128) CHECK((rb + 128) * n_ut * 4 > (int64_t(64) << 20));
    }
}

// ---- 4. the diverse plan ------------------------------------------------------------------------------------------------
static int64_t halved_until_free(int64_t rows, size_t free_b, size_t per_row) {
  const size_t fixed = (size_t(128) << 20) + (size_t(64) << 20);  // a batch's score buffer and the margin kept free
  if (rows <= 1 || static_cast<size_t>(rows) * per_row + fixed <= free_b) return rows;
  return halved_until_free((rows + 1) / 2, free_b, per_row);
}

static void check_diverse() {
  CHECK(div_row_bytes(50, 10) == 50 * 12 + 10 * 20 + 16);
  for (int64_t n_users : {int64_t(1), int64_t(2), int64_t(5), int64_t(1000), int64_t(1000000)})
    for (size_t free_b : {size_t(0), size_t(100) << 20, (size_t(192) << 20) + 5000, size_t(1) << 30, size_t(1) << 40})
      for (size_t per_row : {div_row_bytes(1, 1), div_row_bytes(50, 10), div_row_bytes(1024, 1024)}) {
        ++g_case;
        for (int64_t opt : {int64_t(1), int64_t(2), int64_t(100)})
          CHECK(div_rows_per_call(opt, n_users, free_b, per_row) == std::min(opt, n_users));
        const int64_t got = div_rows_per_call(0, n_users, free_b, per_row);
        CHECK(got >= 1 && got <= n_users && got == halved_until_free(n_users, free_b, per_row));
      }
}

int main() {
  check_batches();
  check_groups();
  check_audience();
  check_diverse();
  if (fails) {
    std::printf("serve plan check: %ld FAILED of %ld cases\n", fails, g_case);
    return 1;
  }
  std::printf("serve plan check: ok (%ld cases)\n", g_case);
  return 0;
}
