// Host-only check of mmsbm_amd/csrc/abi_request.hpp, built with -fsanitize=address,undefined by
// tests/test_abi_request_cpu.py.  For the requests of tests/abi_request_cases.py that depend on no session state it
// builds the same faulty and empty requests on plain arrays, runs them through the header's checks in the order the
// entry runs them, and prints `label<TAB>code<TAB>message`: the pytest holds every line against the table recorded from
// the library (tests/gpu_abi_requests_parent.json).  Then it sweeps each checker's legal extremes, which must pass
// without a refusal and without a read outside the arrays given.  The sizes are the table's: 64 users, 48 items, K = 3,
// rating weights 0, 1, 2.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "../../mmsbm_amd/csrc/abi_request.hpp"

using namespace mmsbm_hip_impl;
using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;

constexpr int32_t kUsers = 64, kItems = 48, kK = 3;
constexpr double kWMin = 0.0, kWMax = 2.0;
static long fails = 0;

template <class F>
static void note(const std::string &label, F &&f) {
  int code = 0;
  std::string text;
  try {
    f();
  } catch (const ApiError &e) {
    code = e.code, text = e.what();
  } catch (const std::invalid_argument &e) {
    code = 1, text = e.what();
  }
  std::printf("%s\t%d\t%s\n", label.c_str(), code, text.c_str());
}
template <class F>
static void legal(const char *what, F &&f) {   // an extreme that every checker must let through
  try {
    f();
  } catch (const std::exception &e) {
    if (++fails <= 20) std::printf("FAILED legal %s: %s\n", what, e.what());
  }
}
static const int32_t *ptr(const I32 &v, bool given) { return given ? v.data() : nullptr; }
static const int64_t *ptr(const I64 &v, bool given) { return given ? v.data() : nullptr; }
[[noreturn]] static void null_argument() { throw std::invalid_argument("null argument"); }

// A request as the cases build it: the defaults are a small valid one
struct Request {
  int64_t n_users = 2;
  I32 users{0, 1};
  bool has_users = true;
  int32_t n = 2, n_cand = 0;
  I32 cand;
  bool has_cand = false;
  I64 off;          // the exclusion or seen lists
  I32 val;
  bool has_off = false, has_val = false;
  std::vector<double> theta = std::vector<double>(2 * kK, 1.0 / kK);
  bool has_theta = true;
  int64_t n_cats = 2;
  I64 cat_off{0, 2, 4};
  I32 cat_items{0, 1, 2, 3}, caps{1, 1};
  bool has_cat_off = true, has_cat_items = true, has_caps = true;
  ShelfAsk ask{1, 1, 1, 1};
  bool has_shelf_cats = true, has_shelf_items = true;
  double temperature = 0.5;
  I64 list_off{0, 1, 2};
  I32 list_items{3, 4};
};

// An entry as mmsbm_hip.hip runs the header's checks for it, after its session is open
struct Entry {
  const char *name, *user_prefix, *who;   // user_prefix null: theta rows
  const char *n_who, *n_noun;             // null: no n, or an n of the entry's own
  int32_t top;                            // items of the catalogue the session holds
  bool subset, lists, quota, shelves, explore;
  const char *seen_who;
  const char *vals = nullptr, *val_name = nullptr;   // set: the lists are the entry's own "offsets" CSR, and required
  bool rank = false;                                  // ... whose rows are candidate lists
};
static void run(const Entry &e, const Request &r) {
  static int32_t out_i[8];
  static double out_d[8];
  require_rows(r.n_users);
  if (e.n_who) require_n(r.n, e.n_who, e.n_noun);
  const ShelfOut out{r.has_shelf_cats ? out_i : nullptr, out_d, out_i, out_i, r.has_shelf_items ? out_i : nullptr, out_d, out_i};
  if (e.shelves) require_shelf_ask(r.n_users, r.n_cats, r.ask, out, e.who);
  if (e.explore) require_temperature(r.temperature, kWMin, kWMax, e.who);
  const int32_t n_cand = e.subset ? r.n_cand : 0, *cand = e.subset ? ptr(r.cand, r.has_cand) : nullptr;
  if (e.user_prefix) {
    if (r.n_users > 0 && (!r.has_users || (e.vals && !r.has_off))) null_argument();
    if (e.vals) {
      require_ids(ptr(r.users, r.has_users), r.n_users, kUsers, e.user_prefix);
      RowCsr{ptr(r.off, r.has_off), ptr(r.val, r.has_val), "offsets", "user", e.vals, e.val_name}.check(r.n_users, e.top, e.who);
      for (int64_t b = 0; e.rank && b < r.n_users; ++b)
        require_candidates(r.val.data() + r.off[b], r.off[b], r.off[b + 1] - r.off[b], e.top, e.who);
      return;
    }
    const UserQuery q = user_query(r.n_users, ptr(r.users, r.has_users), n_cand, cand, ptr(r.off, e.lists && r.has_off),
                                   ptr(r.val, e.lists && r.has_val));
    q.check(kUsers, e.user_prefix, e.top, e.who);
  } else {
    if (r.n_users > 0 && !r.has_theta) null_argument();
    if (std::string(e.seen_who) == "inform") require_theta_entries(r.theta.data(), r.has_theta ? size_t(r.n_users) * kK : 0, "inform");
    const ThetaQuery q = theta_query(r.n_users, r.has_theta ? r.theta.data() : nullptr, ptr(r.off, r.has_off),
                                     ptr(r.val, r.has_val), n_cand, cand);
    q.check(e.top, e.who, e.seen_who);
  }
  if (e.quota || e.shelves)
    Categories{r.n_cats, ptr(r.cat_off, r.has_cat_off), ptr(r.cat_items, r.has_cat_items), ptr(r.caps, r.has_caps && e.quota)}
        .check(e.top, e.who, e.quota);
}

struct Named {
  const char *what;
  std::function<void(Request &)> set;
};

int main() {
  const std::vector<Named> bad_cand = {
      {"candidate out of range at entry 1", [](Request &r) { r.cand = {0, kItems}; }},
      {"candidates descending", [](Request &r) { r.cand = {3, 2}; }},
      {"candidate repeated", [](Request &r) { r.cand = {2, 2}; }},
      {"n_cand = items + 1", [](Request &r) { r.cand.resize(kItems + 1); for (int i = 0; i <= kItems; ++i) r.cand[i] = i; }}};
  auto with_cand = [](Request &r) { r.has_cand = true, r.n_cand = static_cast<int32_t>(r.cand.size()); };
  const std::vector<Named> bad_csr = {
      {"offsets[0] = 1", [](Request &r) { r.off = {1, 1, 1}, r.val = {0}; }},
      {"offsets decrease at row 1", [](Request &r) { r.off = {0, 1, 0}, r.val = {}; }},
      {"value out of range", [](Request &r) { r.off = {0, 1, 2}, r.val = {0, kItems}; }}};
  auto with_lists = [](Request &r) { r.has_off = r.has_val = true; };
  auto empty = [](Request &r) { r.n_users = 0, r.has_users = r.has_theta = false, r.has_shelf_cats = r.has_shelf_items = false; };

  // ---- the users / candidate subset / exclusion prefix ----------------------------------------------------------------
  const std::vector<Entry> user_entries = {
      {"recommend_query_within", "recommend: user", "recommend_query_within", "recommend", "items", kItems, 1, 1, 0, 0, 0, 0},
      {"recommend_query_explore", "recommend: user", "recommend_query_explore", "recommend_explore", "items", kItems, 1, 1, 0, 0, 1, 0},
      {"recommend_list_propensity", "recommend: user", "recommend_list_propensity", nullptr, nullptr, kItems, 1, 1, 0, 0, 1, 0},
      {"recommend_query_quota", "recommend: user", "recommend_query_quota", "recommend", "items", kItems, 1, 1, 1, 0, 0, 0},
      {"recommend_query_shelves", "recommend: user", "recommend_query_shelves", nullptr, nullptr, kItems, 1, 1, 0, 1, 0, 0},
      {"recommend_diverse", "recommend_diverse: user", "recommend_diverse", nullptr, nullptr, kItems, 1, 1, 0, 0, 0, 0},
      {"recommend_query_ensemble", "recommend_query_ensemble: user", "recommend_query_ensemble", "recommend_query_ensemble",
       "items", kItems, 1, 1, 0, 0, 0, 0},
      {"inform_query", "inform: user", "inform_query", "inform", "items", kItems, 1, 1, 0, 0, 0, 0}};
  for (const Entry &e : user_entries) {
    const std::string name = std::string(e.name) + ": ";
    auto row = [&](const std::string &what, const std::function<void(Request &)> &set) {
      Request r;
      set(r);
      note(name + what, [&] { run(e, r); });
    };
    if (e.n_who)
      for (int n : {0, 1025}) row("n = " + std::to_string(n), [&](Request &r) { r.n = n; });
    row("user id = n_users at row 1", [](Request &r) { r.users = {0, kUsers}; });
    row("user id = -1 at row 1", [](Request &r) { r.users = {0, -1}; });
    row("n_users = -1", [](Request &r) { r.n_users = -1; });
    row("null users", [](Request &r) { r.has_users = false; });
    for (const Named &c : bad_cand) row(c.what, [&](Request &r) { c.set(r), with_cand(r); });
    row("n_cand = -1", [](Request &r) { r.cand = {0, 1}, r.has_cand = true, r.n_cand = -1; });
    row("no users, n_cand = -1 without candidates", [&](Request &r) { empty(r), r.n_cand = -1; });
    for (const Named &c : bad_csr) row(std::string("exclusion ") + c.what, [&](Request &r) { c.set(r), with_lists(r); });
    row("exclusion total 2^31", [](Request &r) { r.off = {0, 0, int64_t(1) << 31}, r.has_off = true; });
    row("exclusion without values", [](Request &r) { r.off = {0, 1, 2}, r.has_off = true; });
    row("no users, exclusion offsets given", [&](Request &r) { empty(r), r.off = {0}, r.has_off = true; });
    row("no users, null arrays", empty);
  }
  {
    const Entry &explore = user_entries[1], &lists = user_entries[2], &quota = user_entries[3],
                &shelves = user_entries[4];
    auto two = [&](const Entry &e, const char *label, const std::function<void(Request &)> &set) {
      Request r;
      set(r);
      note(label, [&] { run(e, r); });
    };
    two(explore, "recommend_query_explore: temperature 0 and n = 0", [](Request &r) { r.temperature = 0.0, r.n = 0; });
    two(explore, "recommend_query_explore: temperature 0 and a bad user id", [](Request &r) { r.temperature = 0.0, r.users = {0, kUsers}; });
    two(lists, "recommend_list_propensity: temperature 0 and null users", [](Request &r) { r.temperature = 0.0, r.has_users = false; });
    two(shelves, "recommend_query_shelves: depth = 0 and a bad user id", [](Request &r) { r.ask.depth = 0, r.users = {0, kUsers}; });
    two(quota, "recommend_query_quota: a bad exclusion and a bad category", [&](Request &r) {
      r.off = {1, 1, 1}, r.val = {0}, with_lists(r), r.cat_items = {1, 0, 2, 3};
    });
    const double inf = std::numeric_limits<double>::infinity();
    for (const auto &[text, t] : std::vector<std::pair<const char *, double>>{
             {"0.0", 0.0}, {"nan", std::nan("")}, {"inf", inf}, {"-1.0", -1.0}, {"0.002857", 0.002857}}) {
      two(explore, ("recommend_query_explore: temperature " + std::string(text)).c_str(), [t = t](Request &r) { r.temperature = t; });
      two(lists, ("recommend_list_propensity: temperature " + std::string(text)).c_str(), [t = t](Request &r) { r.temperature = t; });
    }
  }

  const std::vector<Entry> csr_entries = {
      {"recommend_rank", "recommend_rank: user", "recommend_rank", "recommend", "items", kItems, 0, 1, 0, 0, 0, 0, "candidate items",
       "candidate item id", true},
      {"explain_query", "explain: user", "explain", "explain", "rows", kItems, 0, 1, 0, 0, 0, 0, "pairs", "item id"},
      {"recommend_positions", "recommend_positions: user", "recommend_positions", nullptr, nullptr, kItems, 0, 1, 0, 0, 0, 0, "items",
       "item id"}};
  for (const Entry &e : csr_entries) {
    const std::string name = std::string(e.name) + ": ";
    auto row = [&](const std::string &what, const std::function<void(Request &)> &set) {
      Request r;
      r.off = {0, 1, 2}, r.val = {3, 4}, r.has_off = r.has_val = true;
      set(r);
      note(name + what, [&] { run(e, r); });
    };
    if (e.n_who)
      for (int n : {0, 1025}) row("n = " + std::to_string(n), [&](Request &r) { r.n = n; });
    row("user id = n_users at row 1", [](Request &r) { r.users = {0, kUsers}; });
    row("user id = -1 at row 1", [](Request &r) { r.users = {0, -1}; });
    row("n_users = -1", [](Request &r) { r.n_users = -1; });
    row("null users", [](Request &r) { r.has_users = false; });
    row("null offsets", [](Request &r) { r.has_off = false; });
    for (const Named &c : bad_csr) row(c.what, c.set);
    row("total 2^31", [](Request &r) { r.off = {0, 0, int64_t(1) << 31}, r.has_val = false; });
    row("without values", [](Request &r) { r.has_val = false; });
    row("no users, null arrays", [&](Request &r) { empty(r), r.has_off = r.has_val = false; });
  }
  {
    Request r;
    r.off = {0, 2, 4}, r.has_off = r.has_val = true, r.val = {0, 1, 3, 2};
    note("recommend_rank: not ascending in the second row", [&] { run(csr_entries[0], r); });
    r.val = {0, 1, 3, 3};
    note("recommend_rank: repeated in the second row", [&] { run(csr_entries[0], r); });
  }

  // ---- theta rows ---------------------------------------------------------------------------------------------------------
  const std::vector<Entry> theta_entries = {
      {"recommend_query_theta", nullptr, "recommend_query_theta", "recommend", "items", kItems, 0, 1, 0, 0, 0, "recommend"},
      {"recommend_query_theta_within", nullptr, "recommend_query_theta_within", "recommend", "items", kItems, 1, 1, 0, 0, 0, "recommend"},
      {"recommend_query_theta_quota", nullptr, "recommend_query_theta_quota", "recommend", "items", kItems, 1, 1, 1, 0, 0, "recommend"},
      {"recommend_query_theta_shelves", nullptr, "recommend_query_theta_shelves", nullptr, nullptr, kItems, 1, 1, 0, 1, 0, "recommend"},
      {"inform_query_theta", nullptr, "inform_query_theta", "inform", "items", kItems, 1, 1, 0, 0, 0, "inform"}};
  for (const Entry &e : theta_entries) {
    const std::string name = std::string(e.name) + ": ";
    auto row = [&](const std::string &what, const std::function<void(Request &)> &set) {
      Request r;
      set(r);
      note(name + what, [&] { run(e, r); });
    };
    if (e.n_who)
      for (int n : {0, 1025}) row("n = " + std::to_string(n), [&](Request &r) { r.n = n; });
    for (const Named &c : bad_csr) row(std::string("seen ") + c.what, [&](Request &r) { c.set(r), with_lists(r); });
    row("seen total 2^31", [](Request &r) { r.off = {0, 0, int64_t(1) << 31}, r.has_off = true; });
    row("seen without values", [](Request &r) { r.off = {0, 1, 2}, r.has_off = true; });
    if (e.subset) {
      for (const Named &c : bad_cand) row(c.what, [&](Request &r) { c.set(r), with_cand(r); });
      row("n_cand = -1", [](Request &r) { r.cand = {0, 1}, r.has_cand = true, r.n_cand = -1; });
    }
    row("n_users = -1", [](Request &r) { r.n_users = -1; });
    row("null theta", [](Request &r) { r.has_theta = false; });
    row("no users, null arrays", empty);
  }
  {
    const Entry &inform = theta_entries[4], &within = theta_entries[1];
    Request r;
    r.theta[kK + 1] = -0.25;
    note("inform_query_theta: a negative theta entry", [&] { run(inform, r); });
    r.theta[kK + 1] = std::nan("");
    note("inform_query_theta: a NaN theta entry", [&] { run(inform, r); });
    r.cand = {3, 2}, with_cand(r);
    note("inform_query_theta: a NaN theta entry and a bad candidate", [&] { run(inform, r); });
    Request w;
    w.cand = {3, 2}, with_cand(w), w.off = {1, 1, 1}, w.val = {0}, with_lists(w);
    note("recommend_query_theta_within: a bad candidate and a bad seen list", [&] { run(within, w); });
  }

  // ---- categories and shelves -----------------------------------------------------------------------------------------------
  const std::vector<Named> bad_cats = {
      {"category not ascending", [](Request &r) { r.cat_items = {1, 0, 2, 3}; }},
      {"item in two categories", [](Request &r) { r.cat_items = {0, 1, 1, 2}; }},
      {"cat_offsets[0] = 1", [](Request &r) { r.cat_off = {1, 2, 4}; }},
      {"cat_offsets decrease", [](Request &r) { r.cat_off = {0, 2, 1}, r.cat_items = {0}; }},
      {"category item out of range", [](Request &r) { r.cat_items = {0, 1, 2, kItems}; }}};
  for (const Entry *e : {&user_entries[3], &theta_entries[2], &user_entries[4], &theta_entries[3]}) {
    const std::string name = std::string(e->name) + ": ";
    auto row = [&](const std::string &what, const std::function<void(Request &)> &set) {
      Request r;
      set(r);
      note(name + what, [&] { run(*e, r); });
    };
    for (const Named &c : bad_cats) row(c.what, c.set);
    row("n_cats = -1", [](Request &r) { r.n_cats = -1; });
    row("null cat_offsets", [](Request &r) { r.has_cat_off = false; });
    if (e->quota) {
      row("a negative cap", [](Request &r) { r.caps = {1, -1}; });
      row("null cat_caps", [](Request &r) { r.has_caps = false; });
      row("null cat_items", [](Request &r) { r.has_cat_items = false; });
    } else {
      const std::vector<std::pair<const char *, std::function<void(Request &)>>> asks = {
          {"depth = 0", [](Request &r) { r.ask.depth = 0; }},           {"min_items = 0", [](Request &r) { r.ask.min_items = 0; }},
          {"n_shelves = 0", [](Request &r) { r.ask.n_shelves = 0; }},   {"per_shelf = -1", [](Request &r) { r.ask.per_shelf = -1; }},
          {"depth = 1025", [](Request &r) { r.ask.depth = 1025; }},     {"n_shelves = 1025", [](Request &r) { r.ask.n_shelves = 1025; }},
          {"per_shelf = 1025", [](Request &r) { r.ask.per_shelf = 1025; }}};
      for (const auto &[what, set] : asks) row(what, set);
      row("depth = 0 and a category not ascending", [](Request &r) { r.ask.depth = 0, r.cat_items = {1, 0, 2, 3}; });
      row("n_cats = 2^31", [](Request &r) { r.n_cats = int64_t(1) << 31; });
      row("null shelf_cats", [](Request &r) { r.has_shelf_cats = false; });
      row("null items at per_shelf 1", [](Request &r) { r.has_shelf_items = false; });
    }
  }

  // ---- lists, groups, user sets ------------------------------------------------------------------------
  {
    const char *who = "recommend_list_propensity";
    auto lists = [&](const char *label, const I64 &off, const I32 &items) {
      note(std::string(who) + ": " + label, [&] {
        const RowCsr l = listed_items(off.data(), items.data());
        l.check(2, kItems, who);
        require_lists(l, 2, who);
      });
    };
    lists("an item twice in a list", {0, 2, 2}, {3, 3});
    I32 many(1025);
    for (int i = 0; i < 1025; ++i) many[i] = i % kItems;
    lists("a list of 1025 items", {0, 1025, 1025}, many);
    lists("list offsets[0] = 1", {1, 1, 1}, {0});
    lists("list offsets decrease at row 1", {0, 1, 0}, {});
    lists("list value out of range", {0, 1, 2}, {0, kItems});

    auto groups = [&](const char *label, int64_t n_groups, const I64 &off, const I32 &members) {
      note(std::string("recommend_query_groups: ") + label, [&] {
        RowCsr{off.data(), members.data(), "offsets", "group", "members", "member"}.check(n_groups, kUsers, "recommend_query_groups");
        require_distinct_members(off.data(), members.data(), n_groups, kUsers, "recommend_query_groups");
      });
    };
    groups("a member repeated in a group", 2, {0, 1, 3}, {0, 1, 1});
    groups("offsets[0] = 1", 2, {1, 1, 1}, {0});
    groups("offsets decrease at row 1", 2, {0, 1, 0}, {});
    groups("value out of range", 2, {0, 1, 2}, {0, kUsers});

    for (const auto &names : std::vector<std::pair<const char *, const char *>>{
             {"recommend_top_pairs", "top_pairs"}, {"recommend_top_pairs_bulk", "top_pairs_bulk"}, {"recommend_pair_bar", "top_pairs_bulk"}}) {
      const char *entry = names.first, *who2 = names.second;
      const I32 twice{1, 0, 1}, beyond{0, kUsers};
      note(std::string(entry) + ": a repeated id", [&] { sorted_user_set(twice.data(), 3, kUsers, who2); });
      note(std::string(entry) + ": user id = n_users at row 1", [&] { sorted_user_set(beyond.data(), 2, kUsers, who2); });
    }
    for (const char *entry : {"recommend_allocate", "recommend_assign"}) {
      const I32 twice{1, 0, 1}, beyond{0, kUsers};
      I32 all;
      note(std::string(entry) + ": a user asked twice", [&] { asked_once_user_set(twice.data(), 3, kUsers, entry, all); });
      note(std::string(entry) + ": user id = n_users at row 1", [&] { asked_once_user_set(beyond.data(), 2, kUsers, entry, all); });
      note(std::string(entry) + ": users left out, n_users = 3", [&] { asked_once_user_set(nullptr, 3, kUsers, entry, all); });
    }
  }

  // ---- legal extremes: nothing refused, nothing read outside the arrays --------------------------------------------------------
  legal("n = 1, 1024", [] { require_n(1, "x", "items"), require_n(kQueryMaxN, "x", "items"); });
  legal("an empty CSR with null values", [] {
    const I64 off{0, 0, 0};
    check_csr(off.data(), nullptr, 2, kItems, "x", "o", "row", "vals", "val");
    check_csr(nullptr, nullptr, 2, kItems, "x", "o", "row", "vals", "val");
    check_csr(off.data(), nullptr, 0, kItems, "x", "o", "row", "vals", "val");
  });
  // (a total of 2^31 - 1 passes the offsets' checks, and check_csr then reads every value: 8 GiB, not swept)
  legal("n_cand = 0, n_cand = top", [] {
    I32 all(kItems);
    for (int i = 0; i < kItems; ++i) all[i] = i;
    Subset{0, all.data()}.check(kItems, "x");
    Subset{kItems, all.data()}.check(kItems, "x");
    Subset{-5, nullptr}.check(kItems, "x");
    // the columns of a null subset (the catalogue, whatever n says), an empty one and a full one
    if (Subset{-5, nullptr}.columns(kItems) != kItems || Subset{0, nullptr}.columns(0) != 0) throw std::runtime_error("null subset");
    if (Subset{0, all.data()}.columns(kItems) != 0) throw std::runtime_error("empty subset");
    if (Subset{kItems, all.data()}.columns(kItems) != kItems) throw std::runtime_error("full subset");
  });
  legal("ids at both ends, no ids", [] {
    const I32 ends{0, kUsers - 1};
    require_ids(ends.data(), 2, kUsers, "x");
    require_ids(nullptr, 0, kUsers, "x");
  });
  legal("every item in a category of its own, caps 0; no categories", [] {
    I64 off(kItems + 1);
    I32 items(kItems), caps(kItems, 0);
    for (int i = 0; i <= kItems; ++i) off[i] = i;
    for (int i = 0; i < kItems; ++i) items[i] = i;
    Categories{kItems, off.data(), items.data(), caps.data()}.check(kItems, "x");
    Categories{kItems, off.data(), items.data(), nullptr}.check(kItems, "x", false);
    Categories{0, nullptr, nullptr, nullptr}.check(kItems, "x");
  });
  legal("a temperature at the floor; equal weights", [] {
    require_temperature(0.00286, kWMin, kWMax, "x");
    require_temperature(5e-324, 1.0, 1.0, "x");
  });
  legal("a shelf ask at its limits", [] {
    int32_t i[1];
    double d[1];
    require_shelf_ask(1, INT32_MAX, ShelfAsk{1024, 1024, 1024, 1024}, ShelfOut{i, d, i, i, i, d, i}, "x");
    require_shelf_ask(1, 0, ShelfAsk{1, 1, 1, 0}, ShelfOut{i, d, i, i, nullptr, nullptr, nullptr}, "x");
    require_shelf_ask(0, 0, ShelfAsk{1, 1, 1, 1}, ShelfOut{}, "x");
  });
  legal("a list of 1024 distinct items; every user in one group and in two", [] {
    I32 items(1024);
    for (int i = 0; i < 1024; ++i) items[i] = i;
    const I64 off{0, 1024};
    require_lists(listed_items(off.data(), items.data()), 1, "x");
    I32 members(2 * kUsers);
    for (int i = 0; i < 2 * kUsers; ++i) members[i] = i % kUsers;
    const I64 goff{0, kUsers, 2 * kUsers};
    require_distinct_members(goff.data(), members.data(), 2, kUsers, "x");
  });
  legal("user sets: all users either way, the users reversed", [] {
    I32 all, rev(kUsers);
    for (int i = 0; i < kUsers; ++i) rev[i] = kUsers - 1 - i;
    const I32 ids = sorted_user_set(nullptr, 0, kUsers, "x");
    if (ids.size() != size_t(kUsers) || ids.front() != 0 || ids.back() != kUsers - 1) throw std::runtime_error("all users");
    if (sorted_user_set(rev.data(), kUsers, kUsers, "x") != ids) throw std::runtime_error("sorted");
    if (asked_once_user_set(rev.data(), kUsers, kUsers, "x", all) != rev.data()) throw std::runtime_error("in order");
    if (asked_once_user_set(nullptr, kUsers, kUsers, "x", all) != all.data() || all != ids) throw std::runtime_error("all");
    if (sorted_user_set(rev.data(), 0, kUsers, "x").size() != 0) throw std::runtime_error("none");
  });
  // ---- the request values: the normalising constructors, the rows of a query --------------------------------------------------
  legal("an empty request loses its offsets, any other keeps them", [] {
    const I64 off0{0}, off2{0, 1, 2};
    const I32 ids{0, 1}, val{3, 4};
    const std::vector<double> theta(2 * kK, 1.0 / kK);
    const UserQuery none = user_query(0, nullptr, 0, nullptr, off0.data(), nullptr);
    const ThetaQuery none_t = theta_query(0, nullptr, off0.data(), nullptr, 0, nullptr);
    if (none.excl.offsets || none_t.seen.offsets) throw std::runtime_error("no rows: offsets kept");
    none.check(kUsers, "x: user", kItems, "x");
    none_t.check(kItems, "x", "x");
    const UserQuery two = user_query(2, ids.data(), 2, val.data(), off2.data(), val.data());
    const ThetaQuery two_t = theta_query(2, theta.data(), off2.data(), val.data(), 2, val.data());
    if (two.excl.offsets != off2.data() || two.excl.values != val.data() || two.users.ids != ids.data() || two.users.n != 2 ||
        two.cand.items != val.data() || two.cand.n != 2)
      throw std::runtime_error("two rows: the user query moved");
    if (two_t.seen.offsets != off2.data() || two_t.seen.values != val.data() || two_t.theta != theta.data() || two_t.n_users != 2 ||
        two_t.cand.items != val.data() || two_t.cand.n != 2)
      throw std::runtime_error("two rows: the theta query moved");
    two.check(kUsers, "x: user", kItems, "x");
    two_t.check(kItems, "x", "x");
    if (listed_items(off0.data(), nullptr).of_rows(0).offsets || listed_items(off2.data(), val.data()).of_rows(2).offsets != off2.data())
      throw std::runtime_error("of_rows");
  });
  legal("the rows [b0, b0 + nb) of a query: ids from b0, the subset as it is, own lists counted from the first", [] {
    // requests of 0, 1 and 5 rows: no lists; lists; empty lists at the first and the last row -- each with and without
    // a subset.  Every array is exactly as long as the request says, so a read beyond one is the sanitizer's.
    const I32 sub{1, 3, 5};
    for (int64_t rows : {0, 1, 5})
      for (int shape = 0; shape < 3; ++shape)
        for (int with_sub = 0; with_sub < 2; ++with_sub) {
          I32 ids(static_cast<size_t>(rows));
          for (int64_t b = 0; b < rows; ++b) ids[static_cast<size_t>(b)] = static_cast<int32_t>(7 * b % kUsers);
          I64 off(static_cast<size_t>(rows) + 1, 0);
          for (int64_t b = 0; b < rows; ++b) {
            const bool hollow = shape == 2 && (b == 0 || b == rows - 1);
            off[static_cast<size_t>(b) + 1] = off[static_cast<size_t>(b)] + (hollow ? 0 : 1 + b % 3);
          }
          I32 val(static_cast<size_t>(off.back()));
          for (size_t e = 0; e < val.size(); ++e) val[e] = static_cast<int32_t>(5 * e % kItems);
          const bool lists = shape > 0;
          const UserQuery q{{rows, ptr(ids, rows > 0)}, {with_sub ? 3 : 0, ptr(sub, with_sub != 0)},
                            excluded_lists(ptr(off, lists), ptr(val, lists && !val.empty()))};
          for (int64_t b0 = 0; b0 <= rows; ++b0)
            for (int64_t nb = 0; b0 + nb <= rows; ++nb) {
              I64 rebased{-7};   // (a previous call's contents must not show)
              const UserQuery part = q.rows(b0, nb, rebased);
              if (part.users.n != nb || part.cand.n != q.cand.n || part.cand.items != q.cand.items)
                throw std::runtime_error("rows: the users or the subset");
              for (int64_t k = 0; k < nb; ++k)
                if (part.users.ids[k] != ids[static_cast<size_t>(b0 + k)]) throw std::runtime_error("rows: an id");
              if (!lists) {
                if (part.excl.offsets || part.excl.values) throw std::runtime_error("rows: lists from none");
                continue;
              }
              // the restatement: offsets minus the first, values from the first
              if (!part.excl.offsets || part.excl.off_name != q.excl.off_name) throw std::runtime_error("rows: no lists");
              for (int64_t k = 0; k <= nb; ++k)
                if (part.excl.offsets[k] != off[static_cast<size_t>(b0 + k)] - off[static_cast<size_t>(b0)])
                  throw std::runtime_error("rows: an offset");
              for (int64_t e = 0; e < part.excl.offsets[nb]; ++e)
                if (part.excl.values[e] != val[static_cast<size_t>(off[static_cast<size_t>(b0)] + e)])
                  throw std::runtime_error("rows: a value");
              part.check(kUsers, "x: user", kItems, "x");   // (reads every offset and every value to the end)
            }
        }
  });
  if (refused_cap("recommend_allocate", 3, 1500, 2000) !=
      "recommend_allocate: the cap of item 3, 1500, is above 1024 and below the 2000 users of the request")
    ++fails, std::printf("FAILED refused_cap\n");
  std::printf(fails ? "abi request check: %ld FAILED\n" : "abi request check: ok\n", fails);
  return fails ? 1 : 0;
}
