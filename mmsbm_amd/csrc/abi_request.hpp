// abi_request.hpp -- the request checks of the C ABI (mmsbm_hip.hip) as host-only code: what a query's users, candidate
// subset, exclusion lists, theta rows, categories, shelves, temperature and user set must satisfy before a kernel reads
// them, and the refusal each fault gets -- and the values a checked request crosses into the serving units as (launch.hpp
// declares the units' entry points over them): UserRows, Subset, RowCsr, UserQuery, ThetaQuery, Categories in; TopNOut,
// ShelfOut, AssignOut out.  user_query / theta_query are where an empty request loses its offsets, UserQuery::rows where a
// slice of a request's own lists is re-based: the only arithmetic on the caller's list pointers in front of the uploads.
// Plain values only -- counts, tops, pointers, the session's weights' range --
// no HIP type, no context, no session: the checks decide which pointers the kernels will dereference, so they run on
// the CPU under the sanitizers over faulty and extreme requests (tests/native/abi_request_check.cpp), against the texts
// recorded from the library (tests/gpu_abi_requests_parent.json).  A fault throws std::invalid_argument (MMSBM_E_INVALID
// at the ABI) or ApiError with the code; the order of the checks inside a function is part of what it promises.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace mmsbm_hip_impl {

struct ApiError : std::runtime_error {
  int code;
  ApiError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

constexpr int kErrUnsupported = 4, kErrTooLarge = 5;   // MMSBM_E_UNSUPPORTED, MMSBM_E_TOOLARGE
constexpr int kQueryMaxN = 1024;                       // MMSBM_HIP_RECOMMEND_MAX_N

// ---- single checks ----------------------------------------------------------------------------------------------------
// ids[0 .. n) in [0, top), or "<prefix> id out of range at row m"
inline void require_ids(const int32_t *ids, int64_t n, int32_t top, const std::string &prefix) {
  for (int64_t m = 0; m < n; ++m)
    if (ids[m] < 0 || ids[m] >= top) throw std::invalid_argument(prefix + " id out of range at row " + std::to_string(m));
}

// The n of a top-N query of `who` ("recommend", "similar"), which returns `noun` ("items", "rows")
inline void require_n(int32_t n, const char *who, const char *noun) {
  if (n < 1) throw std::invalid_argument(std::string(who) + ": n must be at least 1");
  if (n > kQueryMaxN)
    throw ApiError(kErrUnsupported, std::string(who) + ": n = " + std::to_string(n) + " is beyond the " +
                                        std::to_string(kQueryMaxN) + " " + noun + " a query returns at most");
}

// A CSR argument of `rows` ranges (none when off is null): off[0] == 0, never decreasing, a total below 2^31 and
// val[0 .. total) in [0, top).  Messages "<who>: <off_name>[0] must be 0", "<who>: <off_name> decrease at <row> b",
// "<who>: more than 2^31 - 1 <vals>", "<who>: <val_name> out of range at entry e".
inline void check_csr(const int64_t *off, const int32_t *val, int64_t rows, int32_t top, const char *who,
                      const char *off_name, const char *row, const char *vals, const char *val_name) {
  if (!off || rows == 0) return;
  const std::string w = std::string(who) + ": ";
  if (off[0] != 0) throw std::invalid_argument(w + off_name + "[0] must be 0");
  for (int64_t b = 0; b < rows; ++b)
    if (off[b + 1] < off[b])
      throw std::invalid_argument(w + off_name + " decrease at " + row + " " + std::to_string(b));
  const int64_t total = off[rows];
  if (total > INT32_MAX) throw std::invalid_argument(w + "more than 2^31 - 1 " + vals);
  if (total > 0 && !val) throw std::invalid_argument("null argument");
  for (int64_t e = 0; e < total; ++e)
    if (val[e] < 0 || val[e] >= top)
      throw std::invalid_argument(w + val_name + " out of range at entry " + std::to_string(e));
}

// A candidate list of `who`: v[0 .. n) strictly ascending (so distinct) ids in [0, top); `first`: the entry index of v[0]
inline void require_candidates(const int32_t *v, int64_t first, int64_t n, int32_t top, const char *who) {
  for (int64_t e = 0; e < n; ++e) {
    if (v[e] < 0 || v[e] >= top)
      throw std::invalid_argument(std::string(who) + ": candidate item id out of range at entry " + std::to_string(first + e));
    if (e > 0 && v[e] <= v[e - 1])
      throw std::invalid_argument(std::string(who) + ": candidate items must be ascending and distinct (entry " +
                                  std::to_string(first + e) + ")");
  }
}

// The temperature of the two explore entries: finite, > 0 and not below the floor of a session whose rating weights
// span [w_min, w_max] (explore.hpp: a score lies between them, and no exp((s - m) / T) may underflow)
inline void require_temperature(double t, double w_min, double w_max, const char *who) {
  const std::string w = std::string(who) + ": ";
  if (!std::isfinite(t) || t <= 0.0) throw std::invalid_argument(w + "the temperature must be finite and > 0");
  if ((w_max - w_min) / t > 700.0)
    throw std::invalid_argument(w + "temperature " + std::to_string(t) + " is below the floor " +
                                std::to_string((w_max - w_min) / 700.0) + " of the session's weights ((max w - min w) / 700)");
}

// What a *_shelves entry asks of each row, and the caller's output arrays (mmsbm_hip.h; the last three null when
// per_shelf = 0)
struct ShelfAsk {
  int depth, min_items, n_shelves, per_shelf;
};
struct ShelfOut {
  int32_t *shelf_cats;
  double *shelf_values;
  int32_t *shelf_available, *shelf_counts, *items;
  double *scores;
  int32_t *item_counts;
};
inline void require_shelf_ask(int64_t n_users, int64_t n_cats, const ShelfAsk &ask, const ShelfOut &out, const char *who) {
  const std::string w = std::string(who) + ": ";
  if (ask.depth < 1) throw std::invalid_argument(w + "depth must be at least 1");
  if (ask.min_items < 1) throw std::invalid_argument(w + "min_items must be at least 1");
  if (ask.n_shelves < 1) throw std::invalid_argument(w + "n_shelves must be at least 1");
  if (ask.per_shelf < 0) throw std::invalid_argument(w + "negative per_shelf");
  auto within_max = [&](int v, const char *name) {
    if (v > kQueryMaxN)
      throw ApiError(kErrUnsupported, w + name + " = " + std::to_string(v) + " is beyond the " + std::to_string(kQueryMaxN) +
                                          " a query holds");
  };
  within_max(ask.depth, "depth");
  within_max(ask.n_shelves, "n_shelves");
  within_max(ask.per_shelf, "per_shelf");
  if (n_cats > INT32_MAX) throw ApiError(kErrTooLarge, w + "more than 2^31 - 1 categories");
  if (n_users > 0 && (!out.shelf_cats || !out.shelf_values || !out.shelf_available || !out.shelf_counts ||
                      (ask.per_shelf > 0 && (!out.items || !out.scores || !out.item_counts))))
    throw std::invalid_argument("null argument");
}

// The members of a group query, a CSR check_csr has passed over `top` users: distinct within a group
inline void require_distinct_members(const int64_t *offsets, const int32_t *members, int64_t n_groups, int32_t top,
                                     const char *who) {
  std::vector<int64_t> last(static_cast<size_t>(top), -1);   // last[u] = the last group that named user u
  for (int64_t g = 0; g < n_groups; ++g)
    for (int64_t e = offsets[g]; e < offsets[g + 1]; ++e) {
      if (last[static_cast<size_t>(members[e])] == g)
        throw std::invalid_argument(std::string(who) + ": member repeated in group " + std::to_string(g) + " at entry " +
                                    std::to_string(e));
      last[static_cast<size_t>(members[e])] = g;
    }
}

// The theta entries of inform_query_theta (a NaN gain has no place in the order, and the entropy of a negative weight
// is not one)
inline void require_theta_entries(const double *theta, size_t n, const char *who) {
  for (size_t e = 0; e < n; ++e)
    if (!std::isfinite(theta[e]) || theta[e] < 0.0)
      throw std::invalid_argument(std::string(who) + ": theta entry " + std::to_string(e) + " is not a finite number >= 0");
}

// ---- the values a request crosses into the units as --------------------------------------------------------------------
// A row CSR: per request row a list of ids, with the names its messages use (null inside the units: checked already)
struct RowCsr {
  const int64_t *offsets;
  const int32_t *values;
  const char *off_name, *row, *vals, *val_name;
  void check(int64_t rows, int32_t top, const char *who) const {
    check_csr(offsets, values, rows, top, who, off_name, row, vals, val_name);
  }
  // the lists of a request of `rows` rows: an empty request reads no offsets, given or not
  RowCsr of_rows(int64_t rows) const {
    RowCsr r = *this;
    if (rows <= 0) r.offsets = nullptr;
    return r;
  }
};
inline RowCsr excluded_lists(const int64_t *off, const int32_t *val) {
  return {off, val, "excl_offsets", "user", "excluded items", "excluded item"};
}
inline RowCsr seen_lists(const int64_t *off, const int32_t *val) {
  return {off, val, "seen_offsets", "user", "seen items", "seen item"};
}
inline RowCsr listed_items(const int64_t *off, const int32_t *val) {
  return {off, val, "list_offsets", "user", "listed items", "listed item"};
}

// The caller-given lists of recommend_list_propensity, a CSR check has passed: no list beyond kQueryMaxN items, no item
// twice in one
inline void require_lists(const RowCsr &lists, int64_t rows, const char *who) {
  std::vector<int32_t> row;
  for (int64_t b = 0; b < rows; ++b) {
    const int64_t len = lists.offsets[b + 1] - lists.offsets[b];
    if (len > kQueryMaxN)
      throw ApiError(kErrUnsupported, std::string(who) + ": the list of row " + std::to_string(b) + " holds " +
                                          std::to_string(len) + " items, beyond the " + std::to_string(kQueryMaxN) +
                                          " a list holds at most");
    row.assign(lists.values + lists.offsets[b], lists.values + lists.offsets[b + 1]);
    std::sort(row.begin(), row.end());
    const auto twice = std::adjacent_find(row.begin(), row.end());
    if (twice != row.end())
      throw std::invalid_argument(std::string(who) + ": item " + std::to_string(*twice) + " is twice in the list of row " +
                                  std::to_string(b));
  }
}

// User rows: encoded ids of training users, one per request row
struct UserRows {
  int64_t n;
  const int32_t *ids;
  void check(int32_t top, const std::string &prefix) const { require_ids(ids, n, top, prefix); }
};

// A candidate subset of the catalogue: n ascending, distinct item ids (items null: all of it, n ignored)
struct Subset {
  int32_t n;
  const int32_t *items;
  void check(int32_t top, const char *who) const {
    if (!items) return;
    if (n < 0 || n > top) throw std::invalid_argument(std::string(who) + ": n_cand outside [0, items of the catalogue]");
    require_candidates(items, 0, n, top, who);
  }
  // the columns a query over it scores, of a catalogue of `catalogue` items
  int columns(int catalogue) const { return items ? n : catalogue; }
};

inline void require_rows(int64_t n_users) {
  if (n_users < 0) throw std::invalid_argument("negative n_users");
}

// The users / candidate subset / exclusion prefix of a query of `who` over `n_users_top` users and `top` items, after
// the entry's null checks: ids ("<user_prefix> id ..."), then the subset, then the exclusion lists
struct UserQuery {
  UserRows users;
  Subset cand;
  RowCsr excl;
  void check(int32_t n_users_top, const std::string &user_prefix, int32_t top, const char *who) const {
    users.check(n_users_top, user_prefix);
    cand.check(top, who);
    excl.check(users.n, top, who);
  }
  // the query of the request rows [b0, b0 + nb): their ids, the same subset, their own lists with the offsets counted
  // from the first of them (held by `rebased`)
  UserQuery rows(int64_t b0, int64_t nb, std::vector<int64_t> &rebased) const {
    UserQuery q{{nb, users.ids ? users.ids + b0 : nullptr}, cand, excl};
    if (!excl.offsets) return q;
    const int64_t first = excl.offsets[b0];
    rebased.resize(static_cast<size_t>(nb) + 1);
    for (int64_t k = 0; k <= nb; ++k) rebased[static_cast<size_t>(k)] = excl.offsets[b0 + k] - first;
    q.excl.offsets = rebased.data();
    if (excl.values) q.excl.values = excl.values + first;
    return q;
  }
};
inline UserQuery user_query(int64_t n_users, const int32_t *users, int32_t n_cand, const int32_t *cand_items,
                            const int64_t *excl_offsets, const int32_t *excl_items) {
  return {{n_users, users}, {n_cand, cand_items}, excluded_lists(excl_offsets, excl_items).of_rows(n_users)};
}

// Theta rows: caller-given users -- theta [slot][n_users][K] -- with their seen lists and the candidate subset; the
// subset first (under `who`), then the seen lists (under `seen_who`: "recommend", "inform")
struct ThetaQuery {
  int64_t n_users;
  const double *theta;
  Subset cand;
  RowCsr seen;
  void check(int32_t top, const char *who, const char *seen_who) const {
    cand.check(top, who);
    seen.check(n_users, top, seen_who);
  }
};
inline ThetaQuery theta_query(int64_t n_users, const double *theta, const int64_t *seen_offsets, const int32_t *seen_items,
                              int32_t n_cand, const int32_t *cand_items) {
  return {n_users, theta, {n_cand, cand_items}, seen_lists(seen_offsets, seen_items).of_rows(n_users)};
}

// The categories of the *_quota and *_shelves entries: a CSR of n categories over the catalogue's items with a cap each
// (caps null: the shelves entries)
struct Categories {
  int64_t n;
  const int64_t *offsets;
  const int32_t *items, *caps;
  // over the catalogue's `top` items: each category strictly ascending, no item in two of them, no negative cap.
  // capped = false (the two *_shelves entries): the same categories without caps, `caps` is not read.
  void check(int32_t top, const char *who, bool capped = true) const {
    const std::string w = std::string(who) + ": ";
    if (n < 0) throw std::invalid_argument(w + "negative n_cats");
    if (n == 0) return;
    if (!offsets || (capped && !caps)) throw std::invalid_argument("null argument");
    check_csr(offsets, items, n, top, who, "cat_offsets", "category", "category items", "category item");
    std::vector<bool> taken(static_cast<size_t>(top), false);
    for (int64_t g = 0; g < n; ++g) {
      if (capped && caps[g] < 0) throw std::invalid_argument(w + "negative cap of category " + std::to_string(g));
      for (int64_t e = offsets[g]; e < offsets[g + 1]; ++e) {
        if (e > offsets[g] && items[e] <= items[e - 1])
          throw std::invalid_argument(w + "the items of a category must be ascending and distinct (entry " +
                                      std::to_string(e) + ")");
        if (taken[static_cast<size_t>(items[e])])
          throw std::invalid_argument(w + "item " + std::to_string(items[e]) + " is in two categories (entry " +
                                      std::to_string(e) + ")");
        taken[static_cast<size_t>(items[e])] = true;
      }
    }
  }
};

// The caller's output arrays of a top-N query: items and scores [rows][n], counts [rows] (scores, counts: null allowed)
struct TopNOut {
  int32_t *items;
  double *scores;
  int32_t *counts;
};
// ... and of recommend_assign (mmsbm_hip.h)
struct AssignOut {
  int32_t *items;
  double *scores, *paid, *pi, *price, *price_sum;
  int32_t *load, *rounds, *converged;
};

// ---- user sets ---------------------------------------------------------------------------------------------------------
// top_pairs, top_pairs_bulk, pair_bar: the request in id order (ties go by user id; the kernel walks the users in this
// order), every training user when `users` is null; a repeated id would put its pairs into the order twice
inline std::vector<int32_t> sorted_user_set(const int32_t *users, int64_t n_users, int32_t top, const std::string &who) {
  std::vector<int32_t> ids;
  if (users) {
    require_ids(users, n_users, top, who + ": user");
    ids.assign(users, users + n_users);
    std::sort(ids.begin(), ids.end());
    const auto twice = std::adjacent_find(ids.begin(), ids.end());
    if (twice != ids.end()) throw std::invalid_argument(who + ": user id " + std::to_string(*twice) + " is repeated");
  } else {
    ids.resize(static_cast<size_t>(top));
    for (int32_t u = 0; u < top; ++u) ids[static_cast<size_t>(u)] = u;
  }
  return ids;
}

// allocate, assign: the request in the caller's order, no user asked twice; every training user (written to `all`)
// when `users` is null, and then n_users must say so
inline const int32_t *asked_once_user_set(const int32_t *users, int64_t n_users, int32_t top, const std::string &who,
                                          std::vector<int32_t> &all) {
  if (!users) {
    if (n_users != top) throw std::invalid_argument(who + ": without users, n_users must be the number of training users");
    all.resize(static_cast<size_t>(n_users));
    for (int64_t b = 0; b < n_users; ++b) all[static_cast<size_t>(b)] = static_cast<int32_t>(b);
    return all.data();
  }
  require_ids(users, n_users, top, who + ": user");
  std::vector<bool> asked(static_cast<size_t>(top), false);
  for (int64_t b = 0; b < n_users; ++b) {
    if (asked[static_cast<size_t>(users[b])])
      throw std::invalid_argument(who + ": user " + std::to_string(users[b]) + " is asked twice (row " + std::to_string(b) + ")");
    asked[static_cast<size_t>(users[b])] = true;
  }
  return users;
}

// allocate, assign: the cap the plan refused (above what one selection holds, below the request's users)
inline std::string refused_cap(const std::string &who, int item, int32_t cap, int64_t n_users, const char *tail = "") {
  return who + ": the cap of item " + std::to_string(item) + ", " + std::to_string(cap) + ", is above " +
         std::to_string(kQueryMaxN) + " and below the " + std::to_string(n_users) + " users of the request" + tail;
}

}  // namespace mmsbm_hip_impl
