// Host-only check of plan_assortment (mmsbm_amd/csrc/serve_plan.hpp), built and run by tests/test_assortment_cpu.py.
// Without arguments: sweeps the plan over users x columns x CU counts x forced run lengths x partial-buffer sizes and
// checks each against what asrt_gain_kernel / asrt_join_kernel / asrt_pick_kernel rely on, restated from the sizes of
// the request and not from the plan's own arithmetic; prints "assort plan check: ok".
// With arguments `n_rows C n_cus run_blocks part_bytes`: prints that plan, one "name value ..." line per field.
#include <cstdio>
#include <cstdlib>

#include "../../mmsbm_amd/csrc/serve_plan.hpp"

using namespace mmsbm_hip_impl;

static long fails = 0;
static long g_case = 0;
#define CHECK(x)                                                                                                       \
  do {                                                                                                                 \
    if (!(x) && ++fails <= 20) std::printf("FAILED %s (case %ld) line %d\n", #x, g_case, __LINE__);                     \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static void check_plan(int64_t n, int64_t C, int n_cus, int64_t force, size_t part_bytes) {
  ++g_case;
  const AssortPlan p = plan_assortment(n, C, n_cus, force, part_bytes);
  if (n == 0 || C == 0) {
    CHECK(p.runs == 0 && p.batches == 0 && p.n_blk() == 0 && p.part_doubles() == 0);
    return;
  }
  // the runs: whole 128-row steps, every row in exactly one run, no run without a row, a grid's second dimension
  CHECK(p.n_rows == n && p.n_blocks == ceil_div(n, 8) && p.item_tiles == ceil_div(C, 128));
  CHECK(p.run_blocks >= 16 && p.run_blocks % 16 == 0 && p.run_rows == p.run_blocks * 8 && p.run_rows % 128 == 0);
  CHECK(p.runs >= 1 && p.runs <= 65535);
  CHECK(p.runs * p.run_rows >= n && (p.runs - 1) * p.run_rows < n);
  if (force > 0 && ceil_div(ceil_div(n, 8), 65535) <= force)  // the forced length, rounded up to whole steps
    CHECK(p.run_blocks == std::max<int64_t>(16, ceil_div(std::min<int64_t>(force, ceil_div(n, 8)), 16) * 16));
  if (force == 0) {  // about 8 workgroups per CU over the item tiles: never more runs, and no run a step longer than that takes
    const int64_t most = std::max<int64_t>(1, 8LL * n_cus / ceil_div(C, 128));
    const int64_t ask = std::max(ceil_div(ceil_div(n, 8), most), ceil_div(ceil_div(n, 8), 65535));
    CHECK(p.runs <= most);
    CHECK(p.run_blocks == 16 || p.run_blocks < std::min(ask, ceil_div(n, 8)) + 16);
  }
  // the batches: whole item tiles, every column in exactly one batch, the partial buffer within its size (or one tile)
  CHECK(p.batch_tiles >= 1 && p.batch_tiles <= p.item_tiles && p.ld == p.batch_tiles * 128);
  CHECK(p.batches == ceil_div(p.item_tiles, p.batch_tiles));
  CHECK(p.part_doubles() * 8 <= part_bytes || p.batch_tiles == 1);
  CHECK(static_cast<int64_t>(p.batch_blk.size()) == p.batches + 1 && p.batch_blk[0] == 0);
  int64_t cols = 0, blks = 0;
  for (int64_t b = 0; b < p.batches; ++b) {
    const auto [col0, nc] = p.batch_cols(b, C);
    CHECK(col0 == cols && nc >= 1 && nc <= p.ld && col0 % 128 == 0);
    CHECK(p.batch_blk[static_cast<size_t>(b)] == blks);
    cols += nc;
    blks += ceil_div(nc, 256);
  }
  CHECK(cols == C && p.n_blk() == blks);
}

int main(int argc, char **argv) {
  if (argc == 6) {
    const AssortPlan p = plan_assortment(std::atoll(argv[1]), std::atoll(argv[2]), std::atoi(argv[3]), std::atoll(argv[4]),
                                         static_cast<size_t>(std::atoll(argv[5])));
    std::printf("n_blocks %lld\nitem_tiles %lld\nrun_blocks %lld\nrun_rows %lld\nruns %lld\nbatch_tiles %lld\nbatches %lld\nld %lld\n",
                (long long)p.n_blocks, (long long)p.item_tiles, (long long)p.run_blocks, (long long)p.run_rows,
                (long long)p.runs, (long long)p.batch_tiles, (long long)p.batches, (long long)p.ld);
    std::printf("batch_blk");
    for (int32_t v : p.batch_blk) std::printf(" %d", v);
    std::printf("\npart_doubles %lld\n", (long long)p.part_doubles());
    return 0;
  }
  const int64_t users[] = {0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300, 1000, 99997, 1000000, 9000000};
  const int64_t cols[] = {0, 1, 127, 128, 129, 255, 256, 257, 997, 1021, 10000, 100000, 1 << 22};
  const int cus[] = {1, 64, 256, 304};
  const int64_t forced[] = {0, 1, 16, 17, 48, 1 << 20};
  const size_t bytes[] = {size_t(64) << 20, size_t(1) << 20, 4096, 1};
  for (int64_t n : users)
    for (int64_t C : cols)
      for (int n_cus : cus)
        for (int64_t f : forced)
          for (size_t b : bytes) check_plan(n, C, n_cus, f, b);
  // pinned: worked by hand from the rules in the header's comment
  {
    const AssortPlan p = plan_assortment(99997, 100000, 256, 0);   // 782 item tiles: 2 runs of 6,256 blocks
    CHECK(p.item_tiles == 782 && p.n_blocks == 12500 && p.run_blocks == 6256 && p.runs == 2 && p.batches == 1);
    const AssortPlan q = plan_assortment(300, 997, 256, 16);       // forced: one step a run
    CHECK(q.run_rows == 128 && q.runs == 3 && q.item_tiles == 8 && q.n_blk() == 4);
    const AssortPlan r = plan_assortment(300, 997, 256, 1 << 20);  // forced: one run with a carry over every step
    CHECK(r.runs == 1 && r.run_blocks == 48);
    const AssortPlan s = plan_assortment(300, 997, 256, 16, 3 * 256 * 8);  // a buffer of two tiles per run
    CHECK(s.batch_tiles == 2 && s.batches == 4 && s.batch_blk.back() == 4 && s.batch_cols(3, 997).second == 229);
  }
  if (fails) {
    std::printf("assort plan check: %ld failures\n", fails);
    return 1;
  }
  std::printf("assort plan check: ok (%ld plans)\n", g_case);
  return 0;
}
