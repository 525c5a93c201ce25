// shelves.hpp -- category-level recommendation (mmsbm_hip_recommend_query_shelves / _query_theta_shelves): which
// categories ("shelves") to show a row, and each shelf's best items.
//
// Semantics (the one definition): a query's categories are disjoint sets of catalogue items.  For a row take
// recommend_query_within's candidates with their scores (recommend_query's bits) and, for category g, its candidates'
// scores s_1, s_2, ... in recommend.hpp's order -- score descending, equal scores by ascending item id; a of them.
// a < min_items: the category is no candidate.  Otherwise t = min(depth, a) and its VALUE is
// ((..((s_1 + s_2) + s_3) + ..) + s_t) / t: additions left to right from s_1, one IEEE division.  The row's shelves are
// the n_shelves categories of largest value, equal values by ascending category index of the call; a shelf's items are
// the first min(per_shelf, a) of s_1, s_2, ...  A row's answer depends on that row alone.
//
// Per batch of rows (tu_recommend.hip: rec_shelves_run, a BatchFrame over the item columns and a SelectStage over val),
// between the exclusions and the next batch's score tiles (the batch buffer sc [rows][columns] is only read):
//   shelf_value_short_kernel  categories of m <= 64 columns, in quota_short_kernel's geometry: a category is a group of
//                             w = the next power of two >= m lanes, 64 / w categories of one width to a wave.  A lane
//                             holds one column's (score, column) and finds its rank among the finite ones of its group
//                             by shuffles and rec_better; then for j = 0 .. min(depth, w) - 1 the group reads the lane of
//                             rank j (a ballot restricted to the group, a shuffle) and adds: the sum runs in rank order.
//                             No LDS, no barrier.
//   shelf_value_long_kernel   m > 64: one wave per (row, category): quota_long_kernel's first pass with n = depth, which
//                             also counts the finite columns; after the last rec_sort_cut one lane adds the list's
//                             entries in order and divides.
// Both write val [row][G] at the category's value column (serve_plan.hpp: the kept categories in the caller's order, so
// that the selection's "equal values by ascending column" IS the tie rule above), -inf when fewer than min_items columns
// are finite -- which rec_select_kernel, run as it is over val with I = G and n = n_shelves, never takes.
//   shelf_items_kernel        grid (n_shelves, rows), one wave: the chosen category's columns of the batch buffer through
//                             RecList with n = per_shelf; writes the columns and scores best first, their count and the
//                             category's finite columns (`available`).  Not launched when per_shelf = 0;
//   shelf_avail_kernel        per_shelf = 0 only: the value kernels then also write the finite counts avail [row][G],
//                             and this gathers the chosen categories' counts.
// No atomics; the only arithmetic on a score is the sum and the division above.
#pragma once

namespace {

// grid (waves / kQuotaWaves, rows of the batch).  wave_first / wave_info as quota_short_kernel's (ShelfPlan); off / col:
// the kept categories' columns; slot: their value columns.  avail: null unless per_shelf = 0.
__global__ __launch_bounds__(kBlock) void shelf_value_short_kernel(const int32_t *__restrict__ wave_first,
                                                                   const int32_t *__restrict__ wave_info, int n_waves,
                                                                   const int32_t *__restrict__ off,
                                                                   const int32_t *__restrict__ col,
                                                                   const int32_t *__restrict__ slot, int depth,
                                                                   int min_items, const double *__restrict__ scores,
                                                                   size_t ld, double *__restrict__ val,
                                                                   int32_t *__restrict__ avail, size_t G) {
  const int lane = threadIdx.x % kRecWave, wv = blockIdx.x * kQuotaWaves + threadIdx.x / kRecWave;
  if (wv >= n_waves) return;  // (whole waves leave: the shuffles below stay inside one wave)
  const int info = wave_info[wv], w = info & 0xff, cats = info >> 8;
  const int pos = lane & (w - 1), first = lane - pos, g = first / w;
  const double *row = scores + static_cast<size_t>(blockIdx.y) * ld;
  double s = -INFINITY;  // (a lane without a column: never counted, never read)
  int c = INT_MAX, cat = -1;
  if (g < cats) {
    cat = wave_first[wv] + g;
    const int lo = off[cat];
    if (pos < off[cat + 1] - lo) {
      c = col[lo + pos];
      s = row[c];
    }
  }
  const bool fin = s != -INFINITY;
  int before = 0;  // the finite columns of the category that come before this one in the order: its rank
  for (int j = 1; j < w; ++j) {
    const int src = first + ((pos + j) & (w - 1));
    const double so = __shfl(s, src, kRecWave);
    const int co = __shfl(c, src, kRecWave);
    before += (so != -INFINITY && rec_better(so, co, s, c)) ? 1 : 0;
  }
  const uint64_t group = w == kRecWave ? ~uint64_t(0) : (uint64_t(1) << w) - 1;
  const int a = __popcll((__ballot(fin) >> first) & group);
  double sum = 0.0;
  const int steps = min(depth, w);
  for (int j = 0; j < steps; ++j) {
    // the group's lane of rank j (the order is strict: at most one); none: the category has no j-th candidate
    const uint64_t m = (__ballot(fin && before == j) >> first) & group;
    const int src = m ? first + __ffsll(static_cast<unsigned long long>(m)) - 1 : lane;
    const double v = __shfl(s, src, kRecWave);
    if (m) sum = j == 0 ? v : sum + v;
  }
  if (pos == 0 && cat >= 0) {
    const size_t at = static_cast<size_t>(blockIdx.y) * G + slot[cat];
    val[at] = a >= min_items && a > 0 ? sum / static_cast<double>(min(depth, a)) : -INFINITY;
    if (avail) avail[at] = a;
  }
}

// One pass over the columns col[lo .. hi) of `row` through the list L (places places) that keeps the n best; returns
// the finite columns.  All lanes of the one-wave workgroup; the list is sorted, cut to n and safe to read on return.
__device__ __forceinline__ int shelf_list_pass(RecList<int> &L, int n, int places, const int32_t *__restrict__ col,
                                               int lo, int hi, const double *__restrict__ row) {
  const int lane = threadIdx.x;
  int a = 0;
  for (int base = lo; base < hi; base += kRecWave * kRecPerLane) {
    // no room for a whole round: keep the n best, raise the threshold
    if (L.cnt + kRecWave * kRecPerLane > places) rec_sort_cut<kRecWave>(L, n);
    double sv[kRecPerLane];
    int iv[kRecPerLane];
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const int at = base + e * kRecWave + lane;
      sv[e] = -INFINITY;
      iv[e] = INT_MAX;
      if (at < hi) {
        iv[e] = col[at];
        sv[e] = row[iv[e]];
      }
    }
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const bool fin = sv[e] != -INFINITY;
      a += __popcll(__ballot(fin));
      const bool ok = fin && L.admits(sv[e], iv[e]);
      const uint64_t mask = __ballot(ok);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (ok) {
        const int at = L.cnt + __popcll(below);
        L.ks[at] = sv[e];
        L.kk[at] = iv[e];
      }
      L.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kRecWave>(L, n);
  return a;
}

// grid (long categories, rows of the batch), one wave per workgroup.  Category first + blockIdx.x of off / col / slot;
// `places`: the list's places (select_list(depth)), a score and a column each in LDS.
__global__ __launch_bounds__(kRecWave) void shelf_value_long_kernel(const int32_t *__restrict__ off,
                                                                    const int32_t *__restrict__ col,
                                                                    const int32_t *__restrict__ slot, int first,
                                                                    int depth, int min_items, int places,
                                                                    const double *__restrict__ scores, size_t ld,
                                                                    double *__restrict__ val,
                                                                    int32_t *__restrict__ avail, size_t G) {
  extern __shared__ double shelf_lds[];
  RecList<int> L{shelf_lds, reinterpret_cast<int *>(shelf_lds + places)};
  const int cat = first + blockIdx.x;
  const double *row = scores + static_cast<size_t>(blockIdx.y) * ld;
  const int a = shelf_list_pass(L, depth, places, col, off[cat], off[cat + 1], row);
  if (threadIdx.x != 0) return;
  double sum = 0.0;  // (L.cnt = min(depth, a) entries, best first)
  for (int k = 0; k < L.cnt; ++k) sum = k == 0 ? L.ks[0] : sum + L.ks[k];
  const size_t at = static_cast<size_t>(blockIdx.y) * G + slot[cat];
  val[at] = a >= min_items && a > 0 ? sum / static_cast<double>(L.cnt) : -INFINITY;
  if (avail) avail[at] = a;
}

// grid (n_shelves, rows of the batch), one wave per workgroup.  sel [row][n_shelves] / sel_n [row]: the rows' chosen
// value columns (the selection's output); of_slot: a value column's category of off / col.  Output, by (row, shelf):
// out_col / out_s [..][per_shelf] best first, out_n their count, out_avail the category's finite columns.
__global__ __launch_bounds__(kRecWave) void shelf_items_kernel(const int32_t *__restrict__ sel,
                                                               const int32_t *__restrict__ sel_n,
                                                               const int32_t *__restrict__ of_slot,
                                                               const int32_t *__restrict__ off,
                                                               const int32_t *__restrict__ col, int per_shelf,
                                                               int places, const double *__restrict__ scores, size_t ld,
                                                               int32_t *__restrict__ out_col, double *__restrict__ out_s,
                                                               int32_t *__restrict__ out_n,
                                                               int32_t *__restrict__ out_avail) {
  extern __shared__ double shelf_lds[];
  const int k = blockIdx.x, b = blockIdx.y;
  if (k >= sel_n[b]) return;  // (the row has fewer shelves: the whole wave leaves)
  RecList<int> L{shelf_lds, reinterpret_cast<int *>(shelf_lds + places)};
  const size_t o = static_cast<size_t>(b) * gridDim.x + k;
  const int cat = of_slot[sel[o]];
  const double *row = scores + static_cast<size_t>(b) * ld;
  const int a = shelf_list_pass(L, per_shelf, places, col, off[cat], off[cat + 1], row);
  for (int e = threadIdx.x; e < L.cnt; e += kRecWave) {
    out_col[o * per_shelf + e] = L.kk[e];
    out_s[o * per_shelf + e] = L.ks[e];
  }
  if (threadIdx.x == 0) {
    out_n[o] = L.cnt;
    out_avail[o] = a;
  }
}

// per_shelf = 0: out_avail [row][n_shelves] = avail [row][G] at the row's chosen value columns.  grid (rows of the batch).
__global__ __launch_bounds__(kRecWave) void shelf_avail_kernel(const int32_t *__restrict__ sel,
                                                               const int32_t *__restrict__ sel_n, int n_shelves,
                                                               const int32_t *__restrict__ avail, size_t G,
                                                               int32_t *__restrict__ out_avail) {
  const size_t b = blockIdx.x;
  for (int k = threadIdx.x; k < sel_n[b]; k += kRecWave)
    out_avail[b * n_shelves + k] = avail[b * G + sel[b * n_shelves + k]];
}

}  // namespace
