// catalogue.hpp -- recommendation inside a part of the catalogue, within an open recommend session (recommend.hpp):
// the n best of a caller-given SUBSET of the items (shared by the users of a query), with extra excluded items per
// request row, and the order of caller-given candidate LISTS, one per user (the second stage of a two-stage system).
//
//   mmsbm_hip_recommend_query_within / _query_theta_within   the candidates are ascending, distinct item ids of the
//                       session's catalogue.
//     cat_gather_kernel   the candidates' rows of the session's item table into a compact table [slot][C][rank];
//     cat_cols_kernel     col_of[item] = the item's column in that table, or -1 (a binary search per item of the
//                       catalogue: every entry written once, by one thread);
//     rec_score_kernel    (recommend.hpp, as it is) on the compact table with ni = C into a batch buffer of C columns;
//     cat_exclude_kernel  -inf at col_of[item] for every listed item that is a candidate: once over the session's seen
//                       lists (indexed by user id) when the session excludes, once over the query's own lists
//                       (indexed by the row's place in the request, so a user asked twice may carry two lists);
//     rec_select_kernel   (recommend.hpp, as it is; top_n_run of serve_frame.hpp) with I = C: the batch size and the
//                       split across waves follow C.  The host maps the returned columns through the candidate list.
//                       A null candidate list is the whole catalogue: recommend_query's own launches, then
//                       cat_exclude_kernel without col_of over the query's own lists.
//   mmsbm_hip_recommend_rank   per-user candidate lists (CSR by request row, each ascending and distinct).
//     cat_rank_kernel     one wave per request row, in rounds of kRecWave * kRecPerLane candidates: a lane forms its
//                       candidate's score from the user's and the item's rows, drops it when the user's sorted seen
//                       list holds the item (binary search), and the survivors go through RecList / rec_sort_cut exactly
//                       as in rec_select_kernel<false>.  No score buffer, no atomics.
// Bit for bit: a score is ONE fma chain over f = s * rank + j ascending from +0.0 and one division by S -- the
// operations of rec_tile_acc / rec_score_kernel in their order, which do not depend on the column a candidate has or on
// the other candidates -- so a pair's score is recommend_query's.  (rec_tile_acc pads ROWS beyond nb / ni with zeros,
// never the chain of a real output: kc = min(kRecKc, F - f0) ends it at F.)
// Order: the candidate list is ascending, so "equal scores by ascending column" IS "equal scores by ascending item
// id": the one total order of recommend.hpp, cut to the candidates.  The answer is therefore the rows of
// recommend_query(n = all) filtered to the candidates and cut to n.
#pragma once

namespace {

// out[(s * C + c) * rank + j] = y[s * ys + cand[c] * rank + j]
__global__ __launch_bounds__(kBlock) void cat_gather_kernel(const double *__restrict__ y, size_t ys,
                                                            const int32_t *__restrict__ cand, int C, int rank,
                                                            int slots, double *__restrict__ out) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const size_t per = static_cast<size_t>(C) * rank;
  if (e >= per * slots) return;
  const size_t s = e / per, r = e - s * per;
  const size_t c = r / rank;
  const int j = static_cast<int>(r - c * rank);
  out[e] = y[s * ys + static_cast<size_t>(cand[c]) * rank + j];
}

// The place of `item` in the ascending list v[lo, hi), or -1
__device__ __forceinline__ int cat_find(const int32_t *__restrict__ v, int lo, int hi, int item) {
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    const int at = v[mid];
    if (at == item) return mid;
    if (at < item) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// col_of[item] = c where cand[c] == item, else -1, for every item of the session's catalogue (cand ascending, distinct)
__global__ __launch_bounds__(kBlock) void cat_cols_kernel(const int32_t *__restrict__ cand, int C, int items,
                                                          int32_t *__restrict__ col_of) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= items) return;
  col_of[i] = cat_find(cand, 0, C, i);
}

// Row b of the batch: scores[b * ld + col] = -inf for every item of list g = (ids ? ids[b] : first + b), items
// item[off[g] .. off[g + 1]), col = col_of[item] (skipped when -1), or the item itself without col_of.  One workgroup
// per row; a repeated item writes the same value twice.
__global__ __launch_bounds__(kBlock) void cat_exclude_kernel(const int32_t *__restrict__ ids, int first,
                                                             const int32_t *__restrict__ off,
                                                             const int32_t *__restrict__ item,
                                                             const int32_t *__restrict__ col_of,
                                                             double *__restrict__ scores, size_t ld) {
  const int b = blockIdx.x;
  const int g = ids ? ids[b] : first + b;
  double *row = scores + static_cast<size_t>(b) * ld;
  for (int e = off[g] + threadIdx.x; e < off[g + 1]; e += kBlock) {
    const int col = col_of ? col_of[item[e]] : item[e];
    if (col >= 0) row[col] = -INFINITY;
  }
}

// The n best of request row b's candidate list cand[off[b] .. off[b + 1]) (ascending, distinct ids of the catalogue)
// for user users[b].  One wave per workgroup, grid (rows).  x / y: `slots` tables [rows][rank], xs / ys doubles apart.
// seen_off / seen: the sorted excluded items per user id, or null.  Output: out_s / out_i [b * n + k], k < out_n[b].
__global__ __launch_bounds__(kRecWave) void cat_rank_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys, int rank,
                                                            int slots, const int32_t *__restrict__ users,
                                                            const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ cand,
                                                            const int32_t *__restrict__ seen_off,
                                                            const int32_t *__restrict__ seen, int n, int cap,
                                                            double *__restrict__ out_s, int32_t *__restrict__ out_i,
                                                            int32_t *__restrict__ out_n) {
  extern __shared__ double cat_lds[];
  RecList<int> L{cat_lds, reinterpret_cast<int *>(cat_lds + cap)};
  const int lane = threadIdx.x, b = blockIdx.x;
  const int u = users[b];
  const int lo = off[b], hi = off[b + 1];
  const int s_lo = seen_off ? seen_off[u] : 0, s_hi = seen_off ? seen_off[u + 1] : 0;
  const double *xu = x + static_cast<size_t>(u) * rank;
  const double n_slots = static_cast<double>(slots);
  for (int base = lo; base < hi; base += kRecWave * kRecPerLane) {
    // no room for a whole round: keep the N best, raise the threshold
    if (L.cnt + kRecWave * kRecPerLane > cap) rec_sort_cut<kRecWave>(L, n);
    double sv[kRecPerLane];
    int iv[kRecPerLane];
    bool ok[kRecPerLane];
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const int pos = base + e * kRecWave + lane;
      ok[e] = false;
      sv[e] = -INFINITY;
      iv[e] = INT_MAX;
      if (pos < hi) {
        const int item = cand[pos];
        const double *yi = y + static_cast<size_t>(item) * rank;
        double acc = 0.0;  // THE chain of rec_tile_acc: f = s * rank + j ascending
        for (int s = 0; s < slots; ++s)
          for (int j = 0; j < rank; ++j) acc = fma(xu[static_cast<size_t>(s) * xs + j], yi[static_cast<size_t>(s) * ys + j], acc);
        sv[e] = acc / n_slots;
        iv[e] = item;
        ok[e] = sv[e] != -INFINITY && cat_find(seen, s_lo, s_hi, item) < 0;
      }
    }
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const bool q = ok[e] && L.admits(sv[e], iv[e]);
      const uint64_t mask = __ballot(q);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (q) {
        const int at = L.cnt + __popcll(below);
        L.ks[at] = sv[e];
        L.kk[at] = iv[e];
      }
      L.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kRecWave>(L, n);
  const size_t o = static_cast<size_t>(b) * n;
  for (int k = lane; k < L.cnt; k += kRecWave) {
    out_s[o + k] = L.ks[k];
    out_i[o + k] = L.kk[k];
  }
  if (lane == 0) out_n[b] = L.cnt;
}

}  // namespace
