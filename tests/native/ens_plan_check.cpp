// Host-only check of the one plan ensemble.hpp adds to mmsbm_amd/csrc/serve_plan.hpp -- the pairs per launch of
// recommend_pair_spread -- built with -fsanitize=address,undefined by tests/test_ens_plan_cpu.py: every launch holds
// at least one pair and at most the request, a launch's buffers stay within kEnsPairBytes unless it holds one pair, and
// the launches cover the request exactly.
#include <cstdio>

#include "../../mmsbm_amd/csrc/serve_plan.hpp"

using namespace mmsbm_hip_impl;

static long fails = 0;
#define CHECK(x)                                                                     \
  do {                                                                               \
    if (!(x) && ++fails <= 20) std::printf("FAILED %s line %d\n", #x, __LINE__);     \
  } while (0)

int main() {
  const int64_t pairs[] = {1, 2, 255, 256, 257, 999970, int64_t(1) << 24, (int64_t(1) << 31) - 1, int64_t(1) << 33};
  const int slots[] = {1, 2, 3, 8, 64, 1 << 20, 1 << 26};
  for (int64_t n : pairs)
    for (int S : slots)
      for (int each = 0; each < 2; ++each) {
        const size_t row = ens_pair_bytes(S, each != 0);
        CHECK(row == size_t(40) + (each ? size_t(S) * 8 : 0));  // two ids, four numbers, the slots' values
        const int64_t per = ens_pairs_per_launch(n, S, each != 0);
        CHECK(per >= 1 && per <= n);
        CHECK(static_cast<size_t>(per) * row <= kEnsPairBytes || per == 1);
        if (per < n) CHECK(static_cast<size_t>(per + 1) * row > kEnsPairBytes);  // (as many as fit)
        int64_t covered = 0, launches = 0;
        for (int64_t p0 = 0; p0 < n && launches < 1000; p0 += per, ++launches) covered += std::min(per, n - p0);
        if (launches < 1000) CHECK(covered == n);
        CHECK((per + 255) / 256 <= int64_t(1) << 31);  // the grid of ens_pairs_kernel
      }
  CHECK(ens_pairs_per_launch(999970, 8, true) == 999970);  // C3's top-10 lists: one launch
  if (fails) {
    std::printf("ens plan check: %ld failures\n", fails);
    return 1;
  }
  std::printf("ens plan check: ok\n");
  return 0;
}
