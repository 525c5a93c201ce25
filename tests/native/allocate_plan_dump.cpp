// allocate_plan_dump.cpp -- the host plan of a capacity-aware allocation (mmsbm_amd/csrc/serve_plan.hpp: plan_allocate)
// as text, for tests/test_allocate_cpu.py: a CPU program, no HIP.
// stdin: n_items caps[n_items] n_users U max_n force_bi (0: the batches of rec_batch_users).
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
  long long n_items = 0, n_users = 0, U = 0, max_n = 0, force_bi = 0;
  if (!(std::cin >> n_items)) return 2;
  std::vector<int32_t> caps(static_cast<size_t>(n_items));
  for (auto &x : caps) std::cin >> x;
  caps.reserve(1);  // (no item is still a list: data() is not null)
  if (!(std::cin >> n_users >> U >> max_n >> force_bi)) return 2;
  const AllocPlan p = plan_allocate(caps.data(), static_cast<int>(n_items), n_users, static_cast<int>(U),
                                    static_cast<int>(max_n), force_bi);
  line("item", p.item);
  line("cap", p.cap);
  line("closed", p.closed);
  line("batch_n", p.batch_n);
  std::printf("refused %lld\nbi %lld\nmost_n %d\n", static_cast<long long>(p.refused), static_cast<long long>(p.bi), p.most_n);
  return 0;
}
