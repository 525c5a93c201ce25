// pairs_bulk_plan.hpp -- the host side of the radix select behind mmsbm_hip_recommend_top_pairs_bulk (pairs_bulk.hpp) as
// plain values: the order key of a score, the digits of the passes, the step between two passes (which bin holds the
// m-th key, how many keys lie above it, the new prefix) and the plan of a query (digit width, passes, workgroups, buffer
// sizes, when to stop and collect a small bin).  Host arithmetic on plain numbers only -- no HIP type, no context -- so
// that every rule is swept on the CPU against a sorted restatement (tests/native/pairs_bulk_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define MMSBM_PB_HD __host__ __device__
#else
#define MMSBM_PB_HD
#endif

namespace mmsbm_hip_impl {

constexpr int64_t kPbMaxM = int64_t(1) << 26;         // largest m of a query (MMSBM_HIP_TOP_PAIRS_BULK_MAX_M)
constexpr int kPbMaxBits = 16;                        // widest digit the select step is defined for
constexpr int kPbDevMaxBits = 12;                     // widest digit of a launch: 4,096 bins of 4 bytes in LDS
constexpr int kPbDefaultBits = 12;                    // option "pairs_bulk_bits" = 0
constexpr int kPbMaxGroups = 4096;                    // largest value of option "pairs_bulk_groups"
constexpr int64_t kPbDefaultCollect = int64_t(1) << 20;  // option "pairs_bulk_collect": a bin of at most this many keys
constexpr int64_t kPbMaxCollect = int64_t(1) << 24;      // is collected and sorted outright (0: never, every pass runs)
constexpr int kPbFlushTiles = 1 << 15;                // tiles between two flushes of a workgroup's 32-bit bins: a bin
                                                      // gains at most 2^14 per tile, so it stays below 2^29
constexpr size_t kPbEntryBytes = 96;                  // device bytes per returned entry: the two (key, score) arrays, the
                                                      // sort keys, the permutation and the sorts' own storage

// The order key of a double given by its bits: key(a) < key(b) exactly when a < b, -0.0 and +0.0 share one key (the
// scores' equality is fp64 equality).  Not for NaN.  The one definition: the kernels call it too.
MMSBM_PB_HD inline uint64_t pb_key_of_bits(uint64_t bits) {
  if ((bits << 1) == 0) bits = 0;  // -0.0 -> +0.0
  return (bits >> 63) ? ~bits : (bits | (uint64_t(1) << 63));
}
inline uint64_t pb_bits_of_key(uint64_t key) { return (key >> 63) ? (key & ~(uint64_t(1) << 63)) : ~key; }
inline uint64_t pb_key(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return pb_key_of_bits(b);
}
inline double pb_value(uint64_t key) {
  const uint64_t b = pb_bits_of_key(key);
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

// Pass p of a select with digits of `bits` bits looks at key bits [shift, shift + width): the top digit first; the last
// digit is narrower when bits does not divide 64
struct PbDigit {
  int shift, width;
};
inline int pb_passes(int bits) { return (64 + bits - 1) / bits; }
inline PbDigit pb_digit(int bits, int pass) {
  const int hi = 64 - bits * pass;
  const int shift = std::max(hi - bits, 0);
  return {shift, hi - shift};
}

// One step: hist[0 .. n_bins) counts the keys inside the current prefix by their next digit, k (1-based) is the rank
// from the top, among them, of the key looked for.  found: k <= the sum; bin: the digit of that key; above: the keys in
// higher bins; in_bin: the keys of that bin.
struct PbStep {
  bool found;
  int bin;
  int64_t above, in_bin;
};
inline PbStep pb_select_step(const int64_t *hist, int n_bins, int64_t k) {
  int64_t above = 0;
  if (k >= 1)
    for (int b = n_bins - 1; b >= 0; --b) {
      if (hist[b] >= k - above) return {true, b, above, hist[b]};  // (no sum is formed that could pass 2^63)
      above += hist[b];
    }
  return {false, -1, above, 0};
}

// The select between its passes: the first `done_bits` bits of the key looked for are `prefix`, `k` is its rank from
// the top among the `in_bin` keys that share them, `above` keys lie above them all
struct PbState {
  uint64_t prefix = 0;
  int done_bits = 0;
  int64_t k = 0, above = 0, in_bin = 0;
};
inline PbState pb_begin(int64_t total, int64_t k) {
  PbState s;
  s.k = k;
  s.in_bin = total;
  return s;
}
// false: the histogram does not hold k keys (the state is left as it was)
inline bool pb_advance(PbState &s, PbDigit d, const int64_t *hist) {
  const PbStep st = pb_select_step(hist, 1 << d.width, s.k);
  if (!st.found) return false;
  s.prefix = (s.done_bits == 0 ? 0 : s.prefix << d.width) | static_cast<uint64_t>(st.bin);
  s.done_bits += d.width;
  s.k -= st.above;
  s.above += st.above;
  s.in_bin = st.in_bin;
  return true;
}
// The select stops before its next pass and collects the bin: it is small enough (collect = 0: never), or no bit is left
inline bool pb_collect_now(const PbState &s, int64_t collect) {
  return s.done_bits < 64 && collect > 0 && s.in_bin <= collect;
}
// Whether a key belongs to the state's prefix
inline bool pb_in_prefix(const PbState &s, uint64_t key) {
  return s.done_bits == 0 || (key >> (64 - s.done_bits)) == s.prefix;
}

// The plan of a query over n_users x n_items pairs, `candidates` of them candidates, for the m best
struct PbPlan {
  int bits = 0, passes = 0, bins = 0;   // digit width, passes at most, bins of the widest digit
  int groups = 0;                       // workgroups of every tile launch (each a contiguous run of tiles)
  int64_t tiles = 0;                    // 128 x 128 tiles of the request
  int64_t collect = 0;                  // early-stop size
  int64_t m_out = 0;                    // entries of the answer: min(m, candidates)
  size_t lds_bytes = 0;                 // a workgroup's bins
  size_t hist_bytes = 0;                // the two global histograms (all pairs, seen pairs)
  size_t collect_bytes = 0;             // the collected bin and its sorted copy
  size_t out_bytes = 0;                 // everything of size m_out
  size_t group_bytes = 0;               // per workgroup: counts above, at the bar, admitted, and the bases
  size_t user_bytes = 0;                // the request's ids and the ties per user
  size_t bytes() const { return hist_bytes + collect_bytes + out_bytes + group_bytes + user_bytes; }
};
// opt_*: the options "pairs_bulk_groups" / "pairs_bulk_bits" (0: the library's choice) and "pairs_bulk_collect"
inline PbPlan plan_pairs_bulk(int64_t n_users, int64_t n_items, int64_t candidates, int64_t m, int n_cus, int opt_groups,
                              int opt_bits, int64_t opt_collect) {
  PbPlan p;
  p.bits = opt_bits > 0 ? std::min(opt_bits, kPbDevMaxBits) : kPbDefaultBits;
  p.passes = pb_passes(p.bits);
  p.bins = 1 << p.bits;
  p.tiles = ((n_users + 127) / 128) * ((n_items + 127) / 128);
  const int64_t want = opt_groups > 0 ? opt_groups : 2LL * std::max(n_cus, 1);
  p.groups = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, kPbMaxGroups), p.tiles)));
  p.collect = std::max<int64_t>(0, std::min(opt_collect, kPbMaxCollect));
  p.m_out = std::max<int64_t>(0, std::min(m, candidates));
  p.lds_bytes = static_cast<size_t>(p.bins) * sizeof(uint32_t);
  p.hist_bytes = 2 * static_cast<size_t>(p.bins) * sizeof(int64_t);
  p.collect_bytes = 3 * static_cast<size_t>(std::min(p.collect, std::max<int64_t>(candidates, 0))) * sizeof(uint64_t);
  p.out_bytes = static_cast<size_t>(p.m_out) * kPbEntryBytes;
  p.group_bytes = 4 * static_cast<size_t>(p.groups) * sizeof(int64_t);
  p.user_bytes = 2 * static_cast<size_t>(std::max<int64_t>(n_users, 0)) * sizeof(int32_t);
  return p;
}
// Workgroup g's run of tiles [t0, t1): the first tiles % groups workgroups one more than the others (the kernels hold
// the same two lines)
inline void pb_tile_run(int64_t tiles, int64_t groups, int64_t g, int64_t &t0, int64_t &t1) {
  t0 = (tiles / groups) * g + std::min(g, tiles % groups);
  t1 = t0 + tiles / groups + (g < tiles % groups ? 1 : 0);
}

// Which ties enter the answer: ties[b] candidates of request row b (ascending user id) score exactly the bar, `quota`
// of all of them are admitted in (user, item) order.  Rows below `row` are admitted whole, row `row` gives its first
// `part` ties (0 < part < ties[row], or part = 0: none of it), rows beyond none.  quota <= the sum.
struct PbCut {
  int64_t row, part;
};
inline PbCut pb_tie_cut(const int32_t *ties, int64_t n_rows, int64_t quota) {
  int64_t run = 0;
  for (int64_t b = 0; b < n_rows; ++b) {
    if (run + ties[b] > quota) return {b, quota - run};
    run += ties[b];
  }
  return {n_rows, 0};
}

}  // namespace mmsbm_hip_impl
