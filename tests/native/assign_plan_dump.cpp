// assign_plan_dump.cpp -- the host plan of a welfare-maximising assignment (mmsbm_amd/csrc/serve_plan.hpp: plan_assign) as
// text, for tests/test_assign_cpu.py: a CPU program, no HIP.
// stdin: n_items caps[n_items] n_users max_n.  stdout: one line per array of the plan ("name v v v ...").
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
  long long n_items = 0, n_users = 0, max_n = 0;
  if (!(std::cin >> n_items)) return 2;
  std::vector<int32_t> caps(static_cast<size_t>(n_items));
  for (auto &x : caps) std::cin >> x;
  caps.reserve(1);  // (no item is still a list: data() is not null)
  if (!(std::cin >> n_users >> max_n)) return 2;
  const AssignPlan p = plan_assign(caps.data(), static_cast<int>(n_items), n_users, static_cast<int>(max_n));
  line("cap", p.cap);
  line("slot_off", p.slot_off);
  std::printf("refused %lld\nmost %d\nlds_places %d\nslots %lld\n", static_cast<long long>(p.refused), p.most,
              p.lds_places(), static_cast<long long>(p.slots()));
  return 0;
}
