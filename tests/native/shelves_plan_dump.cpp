// shelves_plan_dump.cpp -- the host plan of a shelves query (mmsbm_amd/csrc/serve_plan.hpp: plan_shelves) as text, for
// tests/test_shelves_cpu.py: a CPU program, no HIP.
// stdin: n_cand (-1: no candidate list) cand[n_cand]  n_cats off[n_cats + 1] items[off[n_cats]]
// stdout: one line per array of the plan ("name v v v ...").
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
  if (!(std::cin >> n_cats)) return 2;
  std::vector<int64_t> off(static_cast<size_t>(n_cats) + 1);
  for (auto &x : off) std::cin >> x;
  std::vector<int32_t> items(static_cast<size_t>(off.back()));
  for (auto &x : items) std::cin >> x;
  if (!std::cin) return 2;
  const ShelfPlan p = plan_shelves(n_cand < 0 ? nullptr : cand.data(), static_cast<int>(cand.size()), n_cats, off.data(),
                                   items.data());
  line("cat", p.cat);
  line("slot", p.slot);
  line("of_slot", p.of_slot);
  line("off", p.off);
  line("col", p.col);
  line("wave_first", p.wave_first);
  line("wave_info", p.wave_info);
  std::printf("n_short %d\nn_long %d\n", p.n_short, p.n_long());
  return 0;
}
