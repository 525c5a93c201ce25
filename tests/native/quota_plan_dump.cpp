// quota_plan_dump.cpp -- the host plan of a query with capped categories (mmsbm_amd/csrc/serve_plan.hpp: plan_quota,
// quota_form, quota_width) as text, for tests/test_quota_cpu.py: a CPU program, no HIP.
// stdin: n_cand (-1: no candidate list) cand[n_cand]  n_cats off[n_cats + 1] items[off[n_cats]] caps[n_cats]  n
//        then any number of triples m q n.
// stdout: one line per array of the plan ("name v v v ..."), then "form f width w" per triple.
#include <cstdio>
#include <iostream>

#include "../../mmsbm_amd/csrc/serve_plan.hpp"

using namespace mmsbm_hip_impl;

template <class V>
static void line(const char *name, const V &v) {
  std::printf("%s", name);
  for (auto x : v) std::printf(" %lld", static_cast<long long>(x));
  std::printf("\n");
}

int main() {
  long long n_cand = 0, n_cats = 0;
  if (!(std::cin >> n_cand)) return 2;
  std::vector<int32_t> cand(static_cast<size_t>(std::max<long long>(n_cand, 0)));
  for (auto &x : cand) std::cin >> x;
  cand.reserve(1);  // (an empty candidate list is still a list: data() is not null)
  std::cin >> n_cats;
  std::vector<int64_t> off(static_cast<size_t>(n_cats) + 1);
  for (auto &x : off) std::cin >> x;
  std::vector<int32_t> items(static_cast<size_t>(off.back())), caps(static_cast<size_t>(n_cats));
  for (auto &x : items) std::cin >> x;
  for (auto &x : caps) std::cin >> x;
  int n = 0;
  if (!(std::cin >> n)) return 2;
  const QuotaPlan p = plan_quota(n_cand < 0 ? nullptr : cand.data(), static_cast<int>(cand.size()), n_cats, off.data(),
                                 items.data(), caps.data(), n);
  line("cat", p.cat);
  line("off", p.off);
  line("col", p.col);
  line("cap", p.cap);
  line("wave_first", p.wave_first);
  line("wave_info", p.wave_info);
  std::printf("n_short %d\nn_long %d\nlong_cap %d\n", p.n_short, p.n_long(), p.long_cap);
  int m = 0, q = 0, nn = 0;
  while (std::cin >> m >> q >> nn) std::printf("form %d width %d\n", static_cast<int>(quota_form(m, q, nn)), quota_width(m));
  return 0;
}
