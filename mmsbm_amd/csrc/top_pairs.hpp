// top_pairs.hpp -- the m best (user, item) pairs of the whole model (mmsbm_hip_recommend_top_pairs): one order over all
// |Q| x I pairs of a request, inside an open recommend session (recommend.hpp), without a score buffer.
//
// Order: score descending, equal scores (exact fp64 equality) by ascending user id, then ascending item id -- a strict
// total order on finite scores.  The m best of a union of sets are among the m best of each set, so ANY split of the
// pairs into workgroups and any order inside a workgroup gives the same m pairs: the answer does not depend on G.
//
//   gtop_fused_kernel   G workgroups, each owning a contiguous run of 128 x 128 (user, item) tiles (tile t = user tile
//                       t / item tiles, item tile t % item tiles; 64-bit tile numbers).  Per tile the 8 x 8 accumulators
//                       per thread are formed by rec_tile_acc (recommend.hpp), the function rec_score_kernel calls:
//                       the same fma chain over f = s * rank + j from +0.0, then one division by S, so a pair's score
//                       is bit for bit recommend_query's -- by construction -- and stay in registers:
//                         1. pre-filter, 64 compares per thread: acc >= lo, where lo is the smallest accumulator whose
//                            QUOTIENT reaches the threshold score (the correctly rounded division by S is monotone, so
//                            acc < lo implies acc / S < threshold; lo is searched among the neighbours of threshold * S
//                            and verified, -inf when the search fails: the pre-filter may only pass too much).  Lanes
//                            outside the request (b >= nb, i >= ni) are masked by index;
//                         2. the lanes that pass divide, compare (score, user, item) with the workgroup's threshold --
//                            its m-th best accepted pair so far -- and only then search the user's ascending seen list;
//                         3. survivors are appended to the candidate list in LDS at positions from a workgroup prefix
//                            sum of the per-thread counts (no atomics); what does not fit waits in the thread's bit mask
//                            while the list is sorted and cut to m (rec_sort_cut, 256 threads), which raises the threshold,
//                            and is then judged again.  The first tile (no threshold, 16,384 candidates) goes through
//                            the same loop in pieces of at most kTopCap - m.
//                       The workgroup writes its <= m best (score, user << 32 | item), best first.
//   gtop_merge_kernel   workgroup j merges `fan` consecutive lists into one, same order, same list code; entries are
//                       visited k-major (entry k of every list before entry k + 1 of any), so a round of 256 without a
//                       survivor ends the merge: every list is sorted and each of its later entries is worse still.
//                       Launched until one list is left (G <= kTopMaxGroups: at most two levels).
// Device memory of a query: 2 x G x m x 16 bytes + the request's ids; nothing of size |Q| x I.
// LDS of gtop_fused_kernel: the two staging tiles (33,280 B) + the list (kTopCap x 16 = 32,768 B) + 64 B.
#pragma once

namespace {

constexpr int kTopMaxM = MMSBM_HIP_TOP_PAIRS_MAX_M;  // largest m a query may ask for (include/mmsbm_hip.h)
constexpr int kTopCap = 2048;                        // candidate list entries (a power of two >= kTopMaxM + kBlock)
constexpr int kTopMaxGroups = 4096;                  // largest G (option "top_pairs_groups")
constexpr int kTopFan = 64;                          // lists one merging workgroup takes (<= kBlock, see above)
constexpr int kTopWaves = kBlock / kRecWave;
static_assert(kTopCap >= kTopMaxM + kBlock && (kTopCap & (kTopCap - 1)) == 0, "list room for one round of the merge");
static_assert(kTopFan <= kBlock, "a round of the merge visits every list");

__device__ __forceinline__ uint64_t gtop_key(int u, int i) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(u)) << 32) | static_cast<uint32_t>(i);
}

// The neighbour of x towards +inf (up) or -inf
__device__ __forceinline__ double gtop_next(double x, bool up) {
  if (x == 0.0) return up ? __longlong_as_double(1LL) : -__longlong_as_double(1LL);
  const long long b = __double_as_longlong(x);
  return __longlong_as_double((x > 0.0) == up ? b + 1 : b - 1);
}

// The smallest accumulator a with a / n_slots >= thr (verified: the one below it gives less), or -inf when it is not
// among the neighbours of thr * n_slots.
__device__ double gtop_floor_acc(double thr, double n_slots) {
  double a = thr * n_slots;
  for (int t = 0; t < 4 && !(a / n_slots >= thr); ++t) a = gtop_next(a, true);
  if (!(a / n_slots >= thr) || !(a > -INFINITY)) return -INFINITY;
  for (int t = 0; t < 6; ++t) {
    const double below = gtop_next(a, false);
    if (!(below / n_slots >= thr)) return a;
    a = below;
  }
  return -INFINITY;
}

// row[c] for a lane's own c, by the bits of c: the accumulators stay in registers (an index the compiler sees as one
// would send the whole tile to scratch memory)
__device__ __forceinline__ double gtop_pick(const double (&row)[kRecTm], int c) {
  static_assert(kRecTm == 8, "three bits");
  const bool b0 = c & 1, b1 = c & 2, b2 = c & 4;
  // (values first: a conditional between two array elements is a conditional between two ADDRESSES)
  const double r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4], r5 = row[5], r6 = row[6], r7 = row[7];
  const double p0 = b0 ? r1 : r0, p1 = b0 ? r3 : r2, p2 = b0 ? r5 : r4, p3 = b0 ? r7 : r6;
  const double q0 = b1 ? p1 : p0, q1 = b1 ? p3 : p2;
  return b2 ? q1 : q0;
}

// The candidate list of a workgroup: recommend.hpp's list, order and sort with the pair key (user << 32 | item)
using GtopList = RecList<uint64_t>;

// Exclusive prefix of k over the workgroup's threads (thread order) and the total.  All 256 threads.
__device__ __forceinline__ int gtop_scan(int k, int *wtot, int &total) {
  const int lane = threadIdx.x % kRecWave, wave = threadIdx.x / kRecWave;
  int v = k;
#pragma unroll
  for (int o = 1; o < kRecWave; o <<= 1) {
    const int t = __shfl_up(v, o, kRecWave);
    if (lane >= o) v += t;
  }
  if (lane == kRecWave - 1) wtot[wave] = v;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kTopWaves; ++w) {
    const int t = wtot[w];
    if (w < wave) base += t;
    sum += t;
  }
  __syncthreads();  // (wtot is written again by the next scan)
  total = sum;
  return base + v - k;
}

// The list's first cnt entries to out_s / out_k [g * m ...], out_n[g]
__device__ __forceinline__ void gtop_write(const GtopList &L, int m, size_t g, double *__restrict__ out_s,
                                           uint64_t *__restrict__ out_k, int32_t *__restrict__ out_n) {
  for (int k = threadIdx.x; k < L.cnt; k += kBlock) {
    out_s[g * m + k] = L.ks[k];
    out_k[g * m + k] = L.kk[k];
  }
  if (threadIdx.x == 0) out_n[g] = L.cnt;
}

// The m best pairs of workgroup g's run of tiles.  x / y / users / nb / ni / rank / slots as rec_score_kernel;
// seen_off / seen: the session's excluded items per user id (ascending), or null.  grid G, 256 threads.
__global__ __launch_bounds__(kBlock) void gtop_fused_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys,
                                                            const int32_t *__restrict__ users, int nb, int ni, int rank,
                                                            int slots, const int32_t *__restrict__ seen_off,
                                                            const int32_t *__restrict__ seen, int m,
                                                            double *__restrict__ out_s, uint64_t *__restrict__ out_k,
                                                            int32_t *__restrict__ out_n) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  __shared__ double list_s[kTopCap];
  __shared__ uint64_t list_k[kTopCap];
  __shared__ int wtot[kTopWaves + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  GtopList L{list_s, list_k};
  double lo = -INFINITY;  // the pre-filter's bound on the accumulator
  const double n_slots = static_cast<double>(slots);
  // this workgroup's tiles: [t0, t1) of n_ut * n_it, the first T % G workgroups one more than the others
  const long long n_it = (ni + kRecTile - 1) / kRecTile, n_ut = (nb + kRecTile - 1) / kRecTile;
  const long long T = n_it * n_ut, G = gridDim.x, g = blockIdx.x;
  const long long t0 = (T / G) * g + min(g, T % G), t1 = t0 + T / G + (g < T % G ? 1 : 0);
  for (long long t = t0; t < t1; ++t) {
    const int b0 = static_cast<int>(t / n_it) * kRecTile, i0 = static_cast<int>(t % n_it) * kRecTile;
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, users, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    // ---- bit e = a * 8 + c of `todo`: the pairs of this thread still to be judged; lanes outside the request
    // (b >= nb, i >= ni: accumulators of 0.0) are masked by index ----
    uint32_t cols = 0;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) cols |= (i0 + tx + 16 * c < ni ? 1u : 0u) << c;
    uint64_t todo = 0;
#pragma unroll
    for (int a = 0; a < kRecTm; ++a)
      if (b0 + ty * kRecTm + a < nb) todo |= static_cast<uint64_t>(cols) << (kRecTm * a);
    // ---- judge, append, and cut when the list is full, until nothing of the tile waits ----
    bool first = true;  // (the seen lists are searched once per pair)
    for (;;) {
      // 1. the pre-filter against the current bound
      uint64_t pre = 0;
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        uint32_t row = 0;
#pragma unroll
        for (int c = 0; c < kRecTm; ++c) row |= (acc[a][c] >= lo ? 1u : 0u) << c;
        pre |= static_cast<uint64_t>(row) << (kRecTm * a);
      }
      todo &= pre;
      // 2. the exact comparison, then the seen list (row by row: the row index stays a constant, see gtop_pick)
      uint64_t surv = 0;
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        uint32_t rb = static_cast<uint32_t>(todo >> (kRecTm * a)) & 0xffu, keep = 0;
        if (rb == 0) continue;
        const int u = users[b0 + ty * kRecTm + a];
        for (; rb != 0; rb &= rb - 1) {
          const int c = __ffs(static_cast<int>(rb)) - 1, i = i0 + tx + 16 * c;
          const double sc = gtop_pick(acc[a], c) / n_slots;
          bool ok = L.admits(sc, gtop_key(u, i));
          if (ok && first && seen_off) {  // survivors only: binary search in the user's ascending list
            const int end = seen_off[u + 1];
            int p = seen_off[u], q = end;
            while (p < q) {
              const int mid = (p + q) >> 1;
              if (seen[mid] < i) p = mid + 1; else q = mid;
            }
            ok = !(p < end && seen[p] == i);
          }
          if (ok) keep |= 1u << c;
        }
        surv |= static_cast<uint64_t>(keep) << (kRecTm * a);
      }
      first = false;
      // 3. append at the positions of a workgroup prefix sum
      int total;
      const int k = __popcll(surv);
      const int off = gtop_scan(k, wtot, total);
      if (total == 0) break;
      const int room = kTopCap - L.cnt;
      const int take = max(0, min(k, room - off));
      uint64_t left = 0;  // what did not fit
      int n = 0;
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        uint32_t rb = static_cast<uint32_t>(surv >> (kRecTm * a)) & 0xffu;
        if (rb == 0) continue;
        const int u = users[b0 + ty * kRecTm + a];
        for (; rb != 0 && n < take; rb &= rb - 1, ++n) {
          const int c = __ffs(static_cast<int>(rb)) - 1;
          list_s[L.cnt + off + n] = gtop_pick(acc[a], c) / n_slots;
          list_k[L.cnt + off + n] = gtop_key(u, i0 + tx + 16 * c);
        }
        left |= static_cast<uint64_t>(rb) << (kRecTm * a);
      }
      todo = left;
      L.cnt += min(total, room);
      if (total <= room) break;
      __syncthreads();
      rec_sort_cut<kBlock>(L, m);
      if (L.have_thr) lo = gtop_floor_acc(L.thr_s, n_slots);
    }
    // the threshold as early as m candidates exist: the next tile is filtered against it
    if (!L.have_thr && L.cnt >= m) {
      __syncthreads();
      rec_sort_cut<kBlock>(L, m);
      if (L.have_thr) lo = gtop_floor_acc(L.thr_s, n_slots);
    }
  }
  __syncthreads();
  rec_sort_cut<kBlock>(L, m);
  gtop_write(L, m, blockIdx.x, out_s, out_k, out_n);
}

// Workgroup j: the m best of lists [j * fan, min(n_lists, j * fan + fan)) of in_s / in_k [list * m + k], k < in_n[list],
// each sorted best first, into out_s / out_k [j * m ...], out_n[j].  grid ceil(n_lists / fan), 256 threads.
__global__ __launch_bounds__(kBlock) void gtop_merge_kernel(const double *__restrict__ in_s,
                                                            const uint64_t *__restrict__ in_k,
                                                            const int32_t *__restrict__ in_n, int n_lists, int fan,
                                                            int m, double *__restrict__ out_s,
                                                            uint64_t *__restrict__ out_k, int32_t *__restrict__ out_n) {
  __shared__ double list_s[kTopCap];
  __shared__ uint64_t list_k[kTopCap];
  __shared__ int wtot[kTopWaves + 1];
  GtopList L{list_s, list_k};
  const int l0 = blockIdx.x * fan, nl = min(fan, n_lists - l0);
  const int n_pos = nl * m;  // (<= kTopFan * kTopMaxM)
  for (int base = 0; base < n_pos; base += kBlock) {
    if (L.cnt + kBlock > kTopCap) {  // no room for a whole round
      __syncthreads();
      rec_sort_cut<kBlock>(L, m);
    }
    const int pos = base + static_cast<int>(threadIdx.x);
    bool ok = false;
    double sc = 0.0;
    uint64_t key = 0;
    if (pos < n_pos) {
      const int k = pos / nl;
      const size_t list = static_cast<size_t>(l0 + (pos - k * nl));
      if (k < in_n[list]) {
        sc = in_s[list * m + k];
        key = in_k[list * m + k];
        ok = L.admits(sc, key);
      }
    }
    int total;
    const int off = gtop_scan(ok ? 1 : 0, wtot, total);
    if (total == 0) break;  // every list's next entry is out (or the lists are used up): so is what follows it
    if (ok) {
      list_s[L.cnt + off] = sc;
      list_k[L.cnt + off] = key;
    }
    L.cnt += total;
  }
  __syncthreads();
  rec_sort_cut<kBlock>(L, m);
  gtop_write(L, m, blockIdx.x, out_s, out_k, out_n);
}

}  // namespace
