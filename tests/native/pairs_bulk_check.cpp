// Host-only check of mmsbm_amd/csrc/pairs_bulk_plan.hpp, built with -fsanitize=address,undefined by
// tests/test_pairs_bulk_plan_cpu.py.  Sweeps the host side of the radix select behind top_pairs_bulk -- the order key, the
// digits, the step between two passes, the early stop, the tie cut, the plan and the tile runs -- against restatements
// written from sorted lists and plain counts, not from the header's own loops.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <random>
#include <vector>

#include "../../mmsbm_amd/csrc/pairs_bulk_plan.hpp"

using namespace mmsbm_hip_impl;

static long fails = 0;
static long g_case = 0;
#define CHECK(x)                                                                                                       \
  do {                                                                                                                 \
    if (!(x) && ++fails <= 20) std::printf("FAILED %s (case %ld) line %d\n", #x, g_case, __LINE__);                     \
  } while (0)

// ---- 1. the key ---------------------------------------------------------------------------------------------------------
static void check_keys() {
  const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
  std::vector<double> v = {-inf, -1e300, -2.5, -1.0, -den, -0.0, 0.0, den, 1e-300, 0.5, 1.0, 1.0 + 2.3e-16, 3.0, 1e300, inf};
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> u(-5.0, 5.0);
  for (int t = 0; t < 2000; ++t) v.push_back(u(rng));
  for (size_t a = 0; a < v.size(); ++a)
    for (size_t b = 0; b < v.size(); ++b) {
      ++g_case;
      CHECK((v[a] < v[b]) == (pb_key(v[a]) < pb_key(v[b])));
      CHECK((v[a] == v[b]) == (pb_key(v[a]) == pb_key(v[b])));  // fp64 equality: -0.0 and +0.0 share a key
    }
  for (double x : v) {
    const double back = pb_value(pb_key(x));
    CHECK(back == x && (x != 0.0 || !std::signbit(back)));      // the bits come back, a zero as +0.0
  }
  CHECK(pb_key(0.0) == (uint64_t(1) << 63) && pb_key(-0.0) == pb_key(0.0));
}

// ---- 2. digits ----------------------------------------------------------------------------------------------------------
static void check_digits() {
  for (int bits = 1; bits <= kPbMaxBits; ++bits) {
    ++g_case;
    const int passes = pb_passes(bits);
    CHECK(passes * bits >= 64 && (passes - 1) * bits < 64);
    int hi = 64;
    for (int p = 0; p < passes; ++p) {
      const PbDigit d = pb_digit(bits, p);
      CHECK(d.width >= 1 && d.width <= bits && d.shift + d.width == hi && d.shift >= 0);
      if (p + 1 < passes) CHECK(d.width == bits);
      hi = d.shift;
    }
    CHECK(hi == 0);  // every bit belongs to exactly one digit
  }
}

// ---- 3. the select against a sorted list ---------------------------------------------------------------------------------
// The select over `keys` for rank k with digits of `bits` bits, histograms counted here key by key; collect: the early
// stop.  Every state between two passes is checked against plain counts.
static uint64_t run_select(const std::vector<uint64_t> &keys, int bits, int64_t k, int64_t collect, int &passes_run,
                           bool &collected) {
  PbState s = pb_begin(static_cast<int64_t>(keys.size()), k);
  passes_run = 0;
  collected = false;
  std::vector<int64_t> hist;
  for (int pass = 0; s.done_bits < 64 && !pb_collect_now(s, collect); ++pass) {
    const PbDigit d = pb_digit(bits, pass);
    hist.assign(size_t(1) << d.width, 0);
    for (uint64_t key : keys)
      if (pb_in_prefix(s, key)) ++hist[(key >> d.shift) & ((uint64_t(1) << d.width) - 1)];
    const PbState before = s;
    CHECK(pb_advance(s, d, hist.data()));
    ++passes_run;
    CHECK(s.done_bits == before.done_bits + d.width && s.done_bits + d.shift == 64);
    int64_t inside = 0, above = 0;
    for (uint64_t key : keys) {
      const uint64_t top = s.done_bits == 64 ? key : key >> (64 - s.done_bits);
      inside += top == s.prefix;
      above += top > s.prefix;
    }
    CHECK(inside == s.in_bin && above == s.above && s.k >= 1 && s.k <= s.in_bin && s.above + s.k == k);
  }
  if (s.done_bits == 64) return s.prefix;
  collected = true;
  std::vector<uint64_t> bin;
  for (uint64_t key : keys)
    if (pb_in_prefix(s, key)) bin.push_back(key);
  CHECK(static_cast<int64_t>(bin.size()) == s.in_bin && s.in_bin <= collect);
  std::sort(bin.begin(), bin.end(), std::greater<uint64_t>());
  return bin[static_cast<size_t>(s.k - 1)];
}

static void check_select() {
  std::mt19937_64 rng(11);
  for (int shape = 0; shape < 6; ++shape) {
    std::vector<uint64_t> keys;
    const int n = shape == 5 ? 1 : 160;
    for (int t = 0; t < n; ++t) {
      uint64_t key = rng();
      if (shape == 1) key = pb_key(static_cast<double>(static_cast<int>(rng() % 9)) - 4.0);  // nine levels, both signs, zero
      if (shape == 2) key = 0x4014000000000000ull;                                           // all mass in one bin
      if (shape == 3) key = (rng() & 0xffffull) | 0xabcdef0000000000ull;                     // one long common prefix
      if (shape == 4) key = t % 2 ? ~uint64_t(0) - (rng() % 3) : rng() % 3;                  // both ends of the range
      keys.push_back(key);
    }
    std::vector<uint64_t> sorted = keys;
    std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
    for (int bits = 1; bits <= kPbMaxBits; ++bits) {
      // m at 1, at the total, and at the first and the last entry of every bin of the first digit
      std::vector<int64_t> ks = {1, static_cast<int64_t>(n)};
      const PbDigit d0 = pb_digit(bits, 0);
      for (size_t j = 0; j < sorted.size(); ++j) {
        const bool first = j == 0 || (sorted[j - 1] >> d0.shift) != (sorted[j] >> d0.shift);
        const bool last = j + 1 == sorted.size() || (sorted[j + 1] >> d0.shift) != (sorted[j] >> d0.shift);
        if (first || last) ks.push_back(static_cast<int64_t>(j) + 1);
      }
      for (int64_t k : ks)
        for (int64_t collect : {int64_t(0), int64_t(1), int64_t(7), int64_t(1000)}) {
          ++g_case;
          int passes_run;
          bool collected;
          const uint64_t got = run_select(keys, bits, k, collect, passes_run, collected);
          CHECK(got == sorted[static_cast<size_t>(k - 1)]);
          if (collect == 0) CHECK(!collected && passes_run == pb_passes(bits));  // prefixes through all 64 bits
          if (collect >= n) CHECK(collected && passes_run == 0);                 // small from the start: no pass at all
        }
    }
  }
}

// ---- 4. one step on counts no 32-bit number holds ---------------------------------------------------------------------------
static void check_steps() {
  for (int bits = 1; bits <= kPbMaxBits; ++bits) {
    const int n_bins = 1 << bits;
    std::vector<int64_t> hist(static_cast<size_t>(n_bins), 0);
    ++g_case;
    CHECK(!pb_select_step(hist.data(), n_bins, 1).found);              // empty
    CHECK(!pb_select_step(hist.data(), n_bins, 0).found);
    PbState s = pb_begin(0, 1);
    CHECK(!pb_advance(s, pb_digit(bits, 0), hist.data()) && s.done_bits == 0 && s.k == 1 && s.above == 0);
    for (int form = 0; form < 3; ++form) {
      for (int b = 0; b < n_bins; ++b) {
        hist[static_cast<size_t>(b)] = 0;
        if (form == 0 && b % 3 != 1) hist[static_cast<size_t>(b)] = (int64_t(1) << 33) + b;   // bins beyond 2^32, gaps
        if (form == 1 && b == n_bins / 2) hist[static_cast<size_t>(b)] = int64_t(2400000000);  // all mass in one bin
        if (form == 2) hist[static_cast<size_t>(b)] = b % 2;                                   // ones and gaps
      }
      // the restatement: walk the bins from the top with running first / last ranks
      int64_t run = 0;
      for (int b = n_bins - 1; b >= 0; --b) {
        const int64_t c = hist[static_cast<size_t>(b)];
        if (c == 0) continue;
        const bool probe = n_bins <= 1024 || b % 251 == 0 || b >= n_bins - 3 || b <= 2;  // (wide digits: a sample of bins)
        for (int64_t k : {run + 1, run + c, run + (c + 1) / 2}) {
          if (!probe) break;
          ++g_case;
          const PbStep st = pb_select_step(hist.data(), n_bins, k);
          CHECK(st.found && st.bin == b && st.above == run && st.in_bin == c);
        }
        run += c;
      }
      CHECK(!pb_select_step(hist.data(), n_bins, run + 1).found);      // beyond the total
      if (run > 0) CHECK(pb_select_step(hist.data(), n_bins, run).found);
    }
  }
}

// ---- 5. the tie cut -----------------------------------------------------------------------------------------------------
static void check_cut() {
  std::mt19937_64 rng(5);
  for (int t = 0; t < 3000; ++t) {
    ++g_case;
    const int n = static_cast<int>(rng() % 12);
    std::vector<int32_t> ties(static_cast<size_t>(n));
    int64_t total = 0;
    for (auto &x : ties) {
      x = static_cast<int32_t>(rng() % 4 == 0 ? 0 : rng() % 9);
      total += x;
    }
    for (int64_t quota = 0; quota <= total; ++quota) {
      const PbCut cut = pb_tie_cut(ties.data(), n, quota);
      // the restatement: the ties one by one in (row, place) order; the first `quota` are in
      int64_t seen = 0;
      bool ok = true;
      for (int b = 0; b < n; ++b)
        for (int e = 0; e < ties[static_cast<size_t>(b)]; ++e, ++seen) {
          const bool in = seen < quota;
          const bool says = b < cut.row || (b == cut.row && e < cut.part);
          ok = ok && in == says;
        }
      CHECK(ok && cut.row >= 0 && cut.row <= n && cut.part >= 0);
      if (cut.row < n) CHECK(cut.part < ties[static_cast<size_t>(cut.row)]);
      else CHECK(cut.part == 0 && quota == total);
    }
  }
}

// ---- 6. the plan and the tile runs ------------------------------------------------------------------------------------------
static void check_plans() {
  const int64_t users[] = {1, 128, 129, 300, 120000, 1000000};
  const int64_t items[] = {1, 128, 997, 20000, 2000000};
  const int64_t ms[] = {1, 1025, 100000, kPbMaxM};
  const int cus[] = {1, 256};
  const int groups[] = {0, 1, 2, 7, 4096};
  const int64_t collects[] = {0, 1, 5000, kPbDefaultCollect, kPbMaxCollect};
  for (int64_t U : users)
    for (int64_t I : items)
      for (int64_t m : ms)
        for (int n_cus : cus)
          for (int og : groups)
            for (int ob : {0, 1, 4, 8, 11, 12})
              for (int64_t oc : collects) {
                ++g_case;
                const int64_t cand = U * I - std::min<int64_t>(U, 5);
                const PbPlan p = plan_pairs_bulk(U, I, cand, m, n_cus, og, ob, oc);
                CHECK(p.bits == (ob ? ob : kPbDefaultBits) && p.bits >= 1 && p.bits <= kPbDevMaxBits);
                CHECK(p.bins == 1 << p.bits && p.passes == pb_passes(p.bits));
                CHECK(p.lds_bytes == size_t(p.bins) * 4 && p.lds_bytes <= 16384);     // beside the two staging tiles
                CHECK(p.tiles == ((U + 127) / 128) * ((I + 127) / 128));
                CHECK(p.groups >= 1 && p.groups <= kPbMaxGroups && p.groups <= p.tiles);
                if (og) CHECK(p.groups == std::min<int64_t>(og, p.tiles));
                else CHECK(p.groups == std::min<int64_t>(std::min<int64_t>(2 * n_cus, kPbMaxGroups), p.tiles));
                CHECK(p.collect == oc && p.collect <= kPbMaxCollect);
                CHECK(p.m_out == std::min(m, cand) && p.m_out <= kPbMaxM);
                CHECK(p.out_bytes == size_t(p.m_out) * kPbEntryBytes && p.hist_bytes == size_t(p.bins) * 16);
                CHECK(p.collect_bytes <= 3 * size_t(kPbMaxCollect) * 8 && p.group_bytes == size_t(p.groups) * 32);
                CHECK(p.bytes() <= size_t(kPbMaxM) * kPbEntryBytes + (size_t(1) << 30));  // whatever the request
                // the runs: contiguous, in order, all tiles, lengths one apart at most
                int64_t at = 0, shortest = p.tiles, longest = 0;
                const int64_t probe[] = {0, 1, p.groups / 2, p.groups - 2, p.groups - 1};
                for (int64_t g = 0; g < p.groups; ++g) {
                  if (p.groups > 64 && g != probe[0] && g != probe[1] && g != probe[2] && g != probe[3] && g != probe[4]) {
                    int64_t t0, t1;
                    pb_tile_run(p.tiles, p.groups, g, t0, t1);
                    at = t1;
                    continue;
                  }
                  int64_t t0, t1;
                  pb_tile_run(p.tiles, p.groups, g, t0, t1);
                  if (g == 0) CHECK(t0 == 0);
                  if (p.groups <= 64) CHECK(t0 == at);
                  CHECK(t1 > t0);
                  shortest = std::min(shortest, t1 - t0);
                  longest = std::max(longest, t1 - t0);
                  at = t1;
                }
                CHECK(at == p.tiles && longest - shortest <= 1);
              }
  // a bin of a workgroup between two flushes stays inside 32 bits
  CHECK(int64_t(kPbFlushTiles) * 128 * 128 < (int64_t(1) << 31));
  CHECK(kPbDevMaxBits <= kPbMaxBits && kPbDefaultBits <= kPbDevMaxBits && kPbDefaultCollect <= kPbMaxCollect);
}

int main() {
  check_keys();
  check_digits();
  check_select();
  check_steps();
  check_cut();
  check_plans();
  if (fails) {
    std::printf("pairs bulk check: %ld FAILED\n", fails);
    return 1;
  }
  std::printf("pairs bulk check: ok (%ld cases)\n", g_case);
  return 0;
}
