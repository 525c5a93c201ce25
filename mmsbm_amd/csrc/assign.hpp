// assign.hpp -- welfare-maximising assignment (mmsbm_hip_recommend_assign): every user of a request gets at most one item,
// item i at most cap[i] users, and the sum of the assigned scores plus `reserve` per unassigned user is as large as it
// can be, within (assigned users) x epsilon.  allocate.hpp answers the same capacities with the one STABLE assignment
// (a walk in score order); this is the assignment of largest total, and it prices every item.
//
// The algorithm (the one definition; tests/assign_reference.py restates it in numpy): a forward auction in Jacobi rounds,
// every price 0 at first.  An item of cap c has c slots (price, holder), kept sorted by price ascending, then holder
// ascending (-1: nobody); p1 / p2 of the item are the prices of its two cheapest slots (p2 = +inf for c = 1, p1 = +inf
// for c = 0, p1 = p2 = 0 for ever for an unlimited item, which holds no slots and takes every bid at price 0).
//   bid     every active user (no item, not dropped out) forms v[i] = score(u, i) - p1[i] over its candidates; (v1, i1)
//           the best in recommend's order, v2' the second value.  Not v1 > reserve: the user drops out for good (prices
//           only rise).  Else v2 = max(reserve, v2', score(u, i1) - p2[i1]) and the bid is (p1[i1] + (v1 - v2)) + eps.
//   accept  per item the bids descending (equal bids by ascending user), the slots ascending: the k-th bid takes the
//           k-th slot while bid > price; its holder becomes active again, the winner holds the slot at its bid; the
//           slots are sorted again.
//   stop    when nobody is active, or after max_rounds rounds (the holdings are feasible after every round).
// Additions, subtractions and comparisons of doubles in that order only: the prices are the reference's bits.
// At the end one more pass over all users at the final prices gives pi_u = max(reserve, max_i (score - p1)), and
// sum pi + sum of all slot prices bounds the optimum from above whatever the prices are.
//
// On the device the request's users stand in id order (row r), and a round runs over the COMPACTED list of active rows:
//   assign_value_kernel   rec_tile_acc, the single division of rec_score_kernel, then s - p1[column] stored; rows = the
//                         active users.  recommend's exclusion and selection kernels follow unchanged with n = 2
//                         (on the host: exclude_seen and the SelectStage of serve_frame.hpp, batch by batch).
//   assign_bid_kernel     one thread per active row: score(u, i1) by the tile's own fma chain (the same bits), the
//                         bid or the drop-out flag, and the row's place for the sort
//   (rocPRIM merge sort of the places by (item, bid descending, place): tu_pairs_bulk.hip)
//   assign_accept_kernel  one wave per item: its segment of the sorted bids by bisection, the bids against the slots,
//                         winners and displaced holders written, the slots sorted again in LDS (rec_sort)
//   assign_count_kernel / assign_scan_kernel / assign_list_kernel   the rows' flags -> the next active list, ascending:
//                         counts per block of rows, one workgroup scans them, every block writes its rows; the host
//                         reads the total, one int per round
//   assign_price_sum_kernel  at the end: every item's slot prices added in slot order
// No atomics; every row and every slot has one writer per launch; nothing depends on the batch or grid shape.
#pragma once

namespace {

constexpr int kAsgDropped = INT_MAX;  // the item key of a row that dropped out: behind every item in the sort

// values[b * ld + i] = score(rows[b], i) - p1[i] for b < nb, i < ni: the score as rec_score_kernel stores it.  The
// tile's padding is masked by index.  grid (column tiles, row tiles).
__global__ __launch_bounds__(kBlock) void assign_value_kernel(const double *__restrict__ x, size_t xs,
                                                              const double *__restrict__ y, size_t ys,
                                                              const int32_t *__restrict__ rows, int nb, int ni, int rank,
                                                              int slots, const double *__restrict__ p1,
                                                              double *__restrict__ values, size_t ld) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kRecTile, b0 = blockIdx.y * kRecTile;
  double acc[kRecTm][kRecTm];
  rec_tile_acc(x, xs, y, ys, rows, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
  const double n_slots = static_cast<double>(slots);
  double pc[kRecTm];
#pragma unroll
  for (int c = 0; c < kRecTm; ++c) {
    const int i = i0 + tx + 16 * c;
    pc[c] = i < ni ? p1[i] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    const int b = b0 + ty * kRecTm + a;
    if (b >= nb) continue;
    double *row = values + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i < ni) row[i] = acc[a][c] / n_slots - pc[c];
    }
  }
}

// The bid of active row a < na (user act_u[a], request row act_r[a]) from its two best values vs / vi [a * 2 + k],
// k < vn[a]: bid_item[a] = i1, bid[a], bid_score[a] = score(u, i1); or bid_item[a] = kAsgDropped and dropped[row] = 1.
// place[a] = a: what the sort orders.
__global__ __launch_bounds__(kBlock) void assign_bid_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys, int rank, int slots,
                                                            const int32_t *__restrict__ act_u,
                                                            const int32_t *__restrict__ act_r, int na,
                                                            const double *__restrict__ vs, const int32_t *__restrict__ vi,
                                                            const int32_t *__restrict__ vn,
                                                            const double *__restrict__ p1, const double *__restrict__ p2,
                                                            double reserve, double eps, int32_t *__restrict__ bid_item,
                                                            double *__restrict__ bid, double *__restrict__ bid_score,
                                                            uint32_t *__restrict__ place, int32_t *__restrict__ dropped) {
  const int a = blockIdx.x * kBlock + threadIdx.x;
  if (a >= na) return;
  place[a] = static_cast<uint32_t>(a);
  const int cnt = vn[a];
  const double v1 = cnt > 0 ? vs[2 * static_cast<size_t>(a)] : -INFINITY;
  if (!(v1 > reserve)) {
    bid_item[a] = kAsgDropped;
    bid[a] = 0.0;
    bid_score[a] = -INFINITY;
    dropped[act_r[a]] = 1;
    return;
  }
  const int i1 = vi[2 * static_cast<size_t>(a)];
  const int u = act_u[a];
  double acc = 0.0;  // (rec_tile_acc's chain: f = s * rank + j ascending from +0.0, one division)
  for (int s = 0; s < slots; ++s) {
    const double *xr = x + static_cast<size_t>(s) * xs + static_cast<size_t>(u) * rank;
    const double *yr = y + static_cast<size_t>(s) * ys + static_cast<size_t>(i1) * rank;
    for (int j = 0; j < rank; ++j) acc = fma(xr[j], yr[j], acc);
  }
  const double s1 = acc / static_cast<double>(slots);
  double v2 = reserve;
  const double v2p = cnt > 1 ? vs[2 * static_cast<size_t>(a) + 1] : -INFINITY;
  if (v2p > v2) v2 = v2p;
  const double alt = s1 - p2[i1];
  if (alt > v2) v2 = alt;
  bid_item[a] = i1;
  bid[a] = (p1[i1] + (v1 - v2)) + eps;
  bid_score[a] = s1;
}

// The first place k of [0, n) with bid_item[ord[k]] >= key (n: none)
__device__ __forceinline__ int asg_lower(const int32_t *__restrict__ bid_item, const uint32_t *__restrict__ ord, int n,
                                         int64_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (bid_item[ord[mid]] >= key) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One wave per item i < ni (grid ni, kRecWave threads; LDS: lds_places doubles + lds_places ints, a power of two >= the
// largest cap, >= 2).  cap[i]: -1 unlimited, 0 closed, else the slots price / holder [slot_off[i] .. + cap[i]).  ord:
// the nbid places sorted by (item, bid descending, place).  Row state by request row: row_item / row_paid / row_score.
__global__ __launch_bounds__(kRecWave) void assign_accept_kernel(const int32_t *__restrict__ cap,
                                                                 const int32_t *__restrict__ slot_off, int lds_places,
                                                                 const int32_t *__restrict__ bid_item,
                                                                 const double *__restrict__ bid,
                                                                 const double *__restrict__ bid_score,
                                                                 const uint32_t *__restrict__ ord, int nbid,
                                                                 const int32_t *__restrict__ act_r,
                                                                 double *__restrict__ price, int32_t *__restrict__ holder,
                                                                 double *__restrict__ p1, double *__restrict__ p2,
                                                                 int32_t *__restrict__ row_item,
                                                                 double *__restrict__ row_paid,
                                                                 double *__restrict__ row_score) {
  extern __shared__ double asg_lds[];
  const int i = blockIdx.x, lane = threadIdx.x;
  const int c = cap[i];
  if (c == 0) return;
  const int lo = asg_lower(bid_item, ord, nbid, i), hi = asg_lower(bid_item, ord, nbid, static_cast<int64_t>(i) + 1);
  if (lo == hi) return;
  if (c < 0) {  // unlimited: every bid is taken, at price 0
    for (int k = lo + lane; k < hi; k += kRecWave) {
      const uint32_t a = ord[k];
      const int r = act_r[a];
      row_item[r] = i;
      row_paid[r] = 0.0;
      row_score[r] = bid_score[a];
    }
    return;
  }
  double *pr = price + slot_off[i];
  int32_t *ho = holder + slot_off[i];
  // m: the bids taken -- the first k at which bid_k > price_k fails (bids descend, prices ascend: it fails from there on)
  const int most = min(hi - lo, c);
  int m = most;
  for (int k0 = 0; k0 < most; k0 += kRecWave) {
    const int k = k0 + lane;
    const bool fails = k < most && !(bid[ord[lo + k]] > pr[k]);
    const uint64_t mask = __ballot(fails);
    if (mask) {
      m = k0 + __ffsll(static_cast<long long>(mask)) - 1;
      break;
    }
  }
  if (m == 0) return;
  __syncthreads();  // (every lane has read the prices it compares before any is written)
  for (int k = lane; k < m; k += kRecWave) {
    const uint32_t a = ord[lo + k];
    const int r = act_r[a], was = ho[k];
    if (was >= 0) {
      row_item[was] = -1;
      row_paid[was] = 0.0;
      row_score[was] = -INFINITY;
    }
    const double b = bid[a];
    pr[k] = b;
    ho[k] = r;
    row_item[r] = i;
    row_paid[r] = b;
    row_score[r] = bid_score[a];
  }
  __syncthreads();
  if (c > 1) {  // the slots by (price ascending, holder ascending): rec_sort's order over (-price, holder)
    double *ks = asg_lds;
    int *kk = reinterpret_cast<int *>(asg_lds + lds_places);
    for (int k = lane; k < c; k += kRecWave) {
      ks[k] = -pr[k];
      kk[k] = ho[k];
    }
    rec_sort<kRecWave>(ks, kk, c);
    for (int k = lane; k < c; k += kRecWave) {
      pr[k] = -ks[k];
      ho[k] = kk[k];
    }
    __syncthreads();
  }
  if (lane == 0) {
    p1[i] = pr[0];
    if (c > 1) p2[i] = pr[1];
  }
}

// price_sum[i] = the prices of item i's slots added in slot order from +0.0 (an item without slots: 0); one thread per item
__global__ __launch_bounds__(kBlock) void assign_price_sum_kernel(const int32_t *__restrict__ slot_off,
                                                                  const double *__restrict__ price, int ni,
                                                                  double *__restrict__ price_sum) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= ni) return;
  double t = 0.0;
  for (int e = slot_off[i]; e < slot_off[i + 1]; ++e) t += price[e];
  price_sum[i] = t;
}

// ---- the next active list: the rows with no item that have not dropped out, ascending -----------------------------------
__device__ __forceinline__ bool asg_active(const int32_t *row_item, const int32_t *dropped, int r, int n) {
  return r < n && row_item[r] < 0 && dropped[r] == 0;
}

// blk_cnt[block] = the active rows among rows [block * kBlock, + kBlock)
__global__ __launch_bounds__(kBlock) void assign_count_kernel(const int32_t *__restrict__ row_item,
                                                              const int32_t *__restrict__ dropped, int n,
                                                              int32_t *__restrict__ blk_cnt) {
  __shared__ int red[kBlock / kRecWave];
  const int r = blockIdx.x * kBlock + threadIdx.x;
  const uint64_t mask = __ballot(asg_active(row_item, dropped, r, n));
  if (threadIdx.x % kRecWave == 0) red[threadIdx.x / kRecWave] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kBlock / kRecWave; ++w) t += red[w];
    blk_cnt[blockIdx.x] = t;
  }
}

// blk_base[b] = blk_cnt[0] + .. + blk_cnt[b - 1] for b < nblk, total[0] = the sum of all.  One workgroup.
__global__ __launch_bounds__(kBlock) void assign_scan_kernel(const int32_t *__restrict__ blk_cnt, int nblk,
                                                             int32_t *__restrict__ blk_base, int32_t *__restrict__ total) {
  __shared__ int sh[kBlock];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nblk; b0 += kBlock) {
    const int b = b0 + threadIdx.x;
    const int v = b < nblk ? blk_cnt[b] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {  // inclusive scan (Hillis-Steele)
      const int add = static_cast<int>(threadIdx.x) >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    if (b < nblk) blk_base[b] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += sh[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = carry;
}

// act_r / act_u [blk_base[block] + rank within the block] = the active rows of the block and their user ids
__global__ __launch_bounds__(kBlock) void assign_list_kernel(const int32_t *__restrict__ row_item,
                                                             const int32_t *__restrict__ dropped,
                                                             const int32_t *__restrict__ users, int n,
                                                             const int32_t *__restrict__ blk_base,
                                                             int32_t *__restrict__ act_r, int32_t *__restrict__ act_u) {
  __shared__ int red[kBlock / kRecWave];
  const int r = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x % kRecWave, wave = threadIdx.x / kRecWave;
  const bool on = asg_active(row_item, dropped, r, n);
  const uint64_t mask = __ballot(on);
  if (lane == 0) red[wave] = __popcll(mask);
  __syncthreads();
  if (!on) return;
  int at = blk_base[blockIdx.x];
  for (int w = 0; w < wave; ++w) at += red[w];
  at += __popcll(lane == 0 ? uint64_t(0) : (mask & ((~uint64_t(0)) >> (64 - lane))));
  act_r[at] = r;
  act_u[at] = users[r];
}

}  // namespace
