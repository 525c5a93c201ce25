// pairs_bulk.hpp -- the m best (user, item) pairs beyond what a workgroup's list holds (mmsbm_hip_recommend_top_pairs_bulk,
// mmsbm_hip_recommend_pair_bar): top_pairs.hpp's definition -- the same candidates, the same score bits, the same order
// (score descending, equal scores by ascending user id, then item id) -- for m up to 2^26, inside an open recommend
// session, without a score buffer.  The |Q| x I matrix is never stored: every kernel below that walks it forms the
// 128 x 128 tiles with rec_tile_acc (recommend.hpp), so a pair's accumulator, and its score acc / S, are recommend_query's
// bits by construction.  Plain launches with host steps in between (pairs_bulk_plan.hpp); no persistent kernel, no flags.
//
// Phase 1, the bar: a radix select of the m-th largest ACCUMULATOR over an order-preserving 64-bit key (-0.0 as +0.0,
//   sign bit flipped, negatives inverted).  The correctly rounded division by S > 0 is monotone, so the m-th score is
//   the m-th accumulator's quotient.
//   pbulk_tile_kernel<false>  one pass: G workgroups, each a contiguous run of tiles; per pair inside the chosen prefix,
//                       one digit of the key into the workgroup's 32-bit bins in LDS (integer atomics; a thread adds
//                       runs of equal digits at once), flushed into the 64-bit global histogram (integer atomics) every
//                       kPbFlushTiles tiles and at the end.  ALL pairs are counted: no seen list is searched.
//   pbulk_seen_kernel   the same digit of the request's SEEN pairs into a second histogram, each scored by one fma
//                       chain over f ascending from +0.0 -- rec_tile_acc's chain for that pair, the same bits.  The host
//                       subtracts, finds the bin of the m-th key and the new prefix (pb_advance).
//   pbulk_tile_kernel<true>   as soon as the prefix's bin is small: its candidates' keys (seen lists searched here, for
//                       pairs inside the prefix only) appended to a buffer, which is sorted; the key of rank k is read.
//                       The places come from an integer atomic: only the sorted multiset is used.
//   An integer sum does not depend on its order, so every histogram, and with it every decision of the select, is
//   bitwise reproducible whatever the number of workgroups.  These are the only atomics of the library, none on floats.
//   pbulk_count_kernel  bar = the m-th accumulator / S; lo = gtop_floor_acc(bar): the smallest accumulator whose quotient
//                       reaches the bar (top_pairs.hpp), so acc >= lo pre-filters as in aud_decide and only what passes
//                       divides.  Counts per workgroup the candidates with score > bar and == bar (plain stores), and the
//                       ties per request row (integer atomics: a row's tiles belong to several workgroups).
// Phase 2, collect: the pairs above the bar and the first `quota` ties in (user, item) order: every tie of the rows
//   below `cut_row`, and of row cut_row those with item <= *cut_item (pb_tie_cut on the host; pbulk_cut_kernel finds the
//   item at which row cut_row's share is used up).
//   pbulk_emit_kernel<false>  the admitted pairs per workgroup (skipped when every tie is admitted: phase 1's counts)
//   pbulk_emit_kernel<true>   writes them: place = the workgroup's base (host scan) + the tiles before + a workgroup
//                       prefix sum inside the tile (gtop_scan) -- functions of the ids and G; no atomics.
// Phase 3, order: two stable rocPRIM radix sorts of the m entries (tu_pairs_bulk.hip): by (user << 32 | item)
//   ascending, then by the score's key descending.  The order is strict and total, so the sorted answer does not depend
//   on the places phase 2 gave, hence not on G; the digit width and the early stop change the route to the same bar.
// Device memory: O(m + bins + G + |Q|).
#pragma once

namespace {

static_assert(kPbMaxM == MMSBM_HIP_TOP_PAIRS_BULK_MAX_M, "one bound");

__device__ __forceinline__ uint64_t pbulk_key(double v) {
  return pb_key_of_bits(static_cast<uint64_t>(__double_as_longlong(v)));
}

// What a pass looks at: keys whose bits above `pshift` equal `prefix` (any: every key), digit (key >> shift) & mask
struct PbulkDigit {
  uint64_t prefix;
  int any, pshift, shift;
  uint32_t mask;
};
__device__ __forceinline__ bool pbulk_inside(const PbulkDigit &d, uint64_t key) {
  return d.any || (key >> d.pshift) == d.prefix;
}

// The accumulator of one pair: rec_tile_acc's chain for it
__device__ __forceinline__ double pbulk_pair_acc(const double *__restrict__ x, size_t xs, const double *__restrict__ y,
                                                 size_t ys, int u, int i, int rank, int slots) {
  double acc = 0.0;
  for (int s = 0; s < slots; ++s) {
    const double *xr = x + static_cast<size_t>(s) * xs + static_cast<size_t>(u) * rank;
    const double *yr = y + static_cast<size_t>(s) * ys + static_cast<size_t>(i) * rank;
    for (int j = 0; j < rank; ++j) acc = fma(xr[j], yr[j], acc);
  }
  return acc;
}

// Whether item i is in user u's ascending seen list
__device__ __forceinline__ bool pbulk_seen(const int32_t *__restrict__ seen_off, const int32_t *__restrict__ seen, int u,
                                           int i) {
  const int end = seen_off[u + 1];
  int p = seen_off[u], q = end;
  while (p < q) {
    const int mid = (p + q) >> 1;
    if (seen[mid] < i) p = mid + 1; else q = mid;
  }
  return p < end && seen[p] == i;
}

// The workgroup's bins into the global histogram, and zero again.  All threads; barriers around it are the caller's.
__device__ __forceinline__ void pbulk_flush(uint32_t *lh, int bins, unsigned long long *__restrict__ hist) {
  for (int b = threadIdx.x; b < bins; b += kBlock) {
    const uint32_t v = lh[b];
    if (v != 0) {
      atomicAdd(&hist[b], static_cast<unsigned long long>(v));
      lh[b] = 0;
    }
  }
}

// This workgroup's run of tiles (pb_tile_run)
__device__ __forceinline__ void pbulk_run(long long T, long long &t0, long long &t1) {
  const long long G = gridDim.x, g = blockIdx.x;
  t0 = (T / G) * g + min(g, T % G);
  t1 = t0 + T / G + (g < T % G ? 1 : 0);
}

// COLLECT = false: hist[digit] += 1 for every pair of the request inside the prefix (dynamic LDS: (mask + 1) x 4 bytes).
// COLLECT = true:  the keys of the CANDIDATES inside the prefix to buf[atomic place] (cap places; *n_buf counts them all).
// x / y / users / nb / ni / rank / slots as rec_score_kernel; grid G, 256 threads.
template <bool COLLECT>
__global__ __launch_bounds__(kBlock) void pbulk_tile_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys,
                                                            const int32_t *__restrict__ users, int nb, int ni, int rank,
                                                            int slots, PbulkDigit d,
                                                            unsigned long long *__restrict__ hist,
                                                            const int32_t *__restrict__ seen_off,
                                                            const int32_t *__restrict__ seen, uint64_t *__restrict__ buf,
                                                            unsigned long long cap, unsigned long long *__restrict__ n_buf) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  extern __shared__ uint32_t pbulk_lds[];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int bins = static_cast<int>(d.mask) + 1;
  if (!COLLECT) {
    for (int b = tid; b < bins; b += kBlock) pbulk_lds[b] = 0;
    __syncthreads();
  }
  const long long n_it = (ni + kRecTile - 1) / kRecTile, n_ut = (nb + kRecTile - 1) / kRecTile;
  long long t0, t1;
  pbulk_run(n_it * n_ut, t0, t1);
  int since = 0;  // tiles since the last flush
  for (long long t = t0; t < t1; ++t) {
    const int b0 = static_cast<int>(t / n_it) * kRecTile, i0 = static_cast<int>(t % n_it) * kRecTile;
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, users, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    uint32_t cur = 0, run = 0;  // a run of equal digits: one atomic
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {
      const int b = b0 + ty * kRecTm + a;
      if (b >= nb) continue;  // (masked by index: the accumulators outside are 0.0)
      int u = 0;
      if (COLLECT) u = users[b];
#pragma unroll
      for (int c = 0; c < kRecTm; ++c) {
        const int i = i0 + tx + 16 * c;
        if (i >= ni) continue;
        const uint64_t key = pbulk_key(acc[a][c]);
        if (!pbulk_inside(d, key)) continue;
        if (COLLECT) {
          if (seen_off && pbulk_seen(seen_off, seen, u, i)) continue;
          const unsigned long long at = atomicAdd(n_buf, 1ull);
          if (at < cap) buf[at] = key;
        } else {
          const uint32_t dg = static_cast<uint32_t>(key >> d.shift) & d.mask;
          if (dg == cur) {
            ++run;
          } else {
            if (run != 0) atomicAdd(&pbulk_lds[cur], run);
            cur = dg;
            run = 1;
          }
        }
      }
    }
    if (!COLLECT) {
      if (run != 0) atomicAdd(&pbulk_lds[cur], run);
      if (++since == kPbFlushTiles) {
        __syncthreads();
        pbulk_flush(pbulk_lds, bins, hist);
        __syncthreads();
        since = 0;
      }
    }
  }
  if (!COLLECT) {
    __syncthreads();
    pbulk_flush(pbulk_lds, bins, hist);
  }
}

// hist[digit] += 1 for every seen pair (users[b], seen item) of the request inside the prefix.  One wave per request row
// at a time; any grid; dynamic LDS as pbulk_tile_kernel<false>.
__global__ __launch_bounds__(kBlock) void pbulk_seen_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys,
                                                            const int32_t *__restrict__ users, int nb, int rank,
                                                            int slots, PbulkDigit d,
                                                            const int32_t *__restrict__ seen_off,
                                                            const int32_t *__restrict__ seen,
                                                            unsigned long long *__restrict__ hist) {
  extern __shared__ uint32_t pbulk_lds[];
  const int tid = threadIdx.x, lane = tid % kRecWave, wave = tid / kRecWave;
  const int bins = static_cast<int>(d.mask) + 1;
  for (int b = tid; b < bins; b += kBlock) pbulk_lds[b] = 0;
  __syncthreads();
  constexpr int kWaves = kBlock / kRecWave;
  for (long long b = static_cast<long long>(blockIdx.x) * kWaves + wave; b < nb; b += static_cast<long long>(gridDim.x) * kWaves) {
    const int u = users[b];
    for (int e = seen_off[u] + lane; e < seen_off[u + 1]; e += kRecWave) {
      const uint64_t key = pbulk_key(pbulk_pair_acc(x, xs, y, ys, u, seen[e], rank, slots));
      if (pbulk_inside(d, key)) atomicAdd(&pbulk_lds[static_cast<uint32_t>(key >> d.shift) & d.mask], 1u);
    }
  }
  __syncthreads();  // (a seen list holds fewer than 2^31 entries in all: no flush on the way)
  pbulk_flush(pbulk_lds, bins, hist);
}

// ---- the bar and what lies above it ---------------------------------------------------------------------------------
struct PbulkBar {
  double bar, lo, n_slots;
};
// bar = acc_m / S (+0.0 for a zero of either sign), lo: gtop_floor_acc's bound or -inf
__device__ __forceinline__ PbulkBar pbulk_bar(double acc_m, int slots) {
  PbulkBar r;
  r.n_slots = static_cast<double>(slots);
  r.bar = acc_m / r.n_slots;
  if (r.bar == 0.0) r.bar = 0.0;
  r.lo = gtop_floor_acc(r.bar, r.n_slots);
  return r;
}

// One tile's decisions: bit a * 8 + c of `above` / `tie`: pair (row b0 + ty * 8 + a, item i0 + tx + 16 c) is a candidate
// with score > bar / == bar.  The seen lists are searched only for pairs that reach the bar.
__device__ __forceinline__ void pbulk_decide(const double (&acc)[kRecTm][kRecTm], const int32_t *__restrict__ users,
                                             int nb, int ni, int b0, int i0, int tx, int ty, const PbulkBar &br,
                                             const int32_t *__restrict__ seen_off, const int32_t *__restrict__ seen,
                                             uint64_t &above, uint64_t &tie) {
  uint32_t cols = 0;
#pragma unroll
  for (int c = 0; c < kRecTm; ++c) cols |= (i0 + tx + 16 * c < ni ? 1u : 0u) << c;
  above = 0;
  tie = 0;
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    if (b0 + ty * kRecTm + a >= nb) continue;
    uint32_t ra = 0, rt = 0;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      if (acc[a][c] >= br.lo) {  // (lo = -inf: everything divides)
        const double sc = acc[a][c] / br.n_slots;
        ra |= (sc > br.bar ? 1u : 0u) << c;
        rt |= (sc == br.bar ? 1u : 0u) << c;
      }
    }
    above |= static_cast<uint64_t>(ra & cols) << (kRecTm * a);
    tie |= static_cast<uint64_t>(rt & cols) << (kRecTm * a);
  }
  if (!seen_off) return;
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    uint32_t rb = static_cast<uint32_t>((above | tie) >> (kRecTm * a)) & 0xffu;
    if (rb == 0) continue;
    const int u = users[b0 + ty * kRecTm + a];
    if (seen_off[u] == seen_off[u + 1]) continue;
    uint32_t drop = 0;
    for (; rb != 0; rb &= rb - 1) {
      const int c = __ffs(static_cast<int>(rb)) - 1;
      if (pbulk_seen(seen_off, seen, u, i0 + tx + 16 * c)) drop |= 1u << c;
    }
    const uint64_t keep = ~(static_cast<uint64_t>(drop) << (kRecTm * a));
    above &= keep;
    tie &= keep;
  }
}

// The sum of v over the workgroup, in thread 0.  All threads; red: kBlock / kRecWave places.
__device__ __forceinline__ long long pbulk_block_sum(long long v, long long *red) {
  for (int o = kRecWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kRecWave);
  if (threadIdx.x % kRecWave == 0) red[threadIdx.x / kRecWave] = v;
  __syncthreads();
  long long s = 0;
  for (int w = 0; w < kBlock / kRecWave; ++w) s += red[w];
  __syncthreads();
  return s;
}

// acc_m: the m-th accumulator.  n_above[g] / n_tie[g]: workgroup g's candidates above / at the bar; tie_row[b] += the
// ties of request row b (zeroed by the caller); *bar_out: the bar.  grid G, 256 threads.
__global__ __launch_bounds__(kBlock) void pbulk_count_kernel(const double *__restrict__ x, size_t xs,
                                                             const double *__restrict__ y, size_t ys,
                                                             const int32_t *__restrict__ users, int nb, int ni, int rank,
                                                             int slots, double acc_m,
                                                             const int32_t *__restrict__ seen_off,
                                                             const int32_t *__restrict__ seen,
                                                             long long *__restrict__ n_above,
                                                             long long *__restrict__ n_tie, int32_t *__restrict__ tie_row,
                                                             double *__restrict__ bar_out) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  __shared__ long long red[kBlock / kRecWave];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const PbulkBar br = pbulk_bar(acc_m, slots);
  if (blockIdx.x == 0 && tid == 0) *bar_out = br.bar;
  const long long n_it = (ni + kRecTile - 1) / kRecTile, n_ut = (nb + kRecTile - 1) / kRecTile;
  long long t0, t1;
  pbulk_run(n_it * n_ut, t0, t1);
  long long na = 0, nt = 0;
  for (long long t = t0; t < t1; ++t) {
    const int b0 = static_cast<int>(t / n_it) * kRecTile, i0 = static_cast<int>(t % n_it) * kRecTile;
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, users, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    uint64_t above, tie;
    pbulk_decide(acc, users, nb, ni, b0, i0, tx, ty, br, seen_off, seen, above, tie);
    na += __popcll(above);
    nt += __popcll(tie);
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {  // the row's ties over the 16 lanes of the ty group
      int v = __popc(static_cast<uint32_t>(tie >> (kRecTm * a)) & 0xffu);
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      const int b = b0 + ty * kRecTm + a;
      if (tx == 0 && v != 0 && b < nb) atomicAdd(&tie_row[b], v);
    }
  }
  const long long sa = pbulk_block_sum(na, red), st = pbulk_block_sum(nt, red);
  if (tid == 0) {
    n_above[blockIdx.x] = sa;
    n_tie[blockIdx.x] = st;
  }
}

// *cut_item = the item of request row `row`'s (user u) part-th tie in item order (part >= 1; the row holds more).  One
// workgroup.
__global__ __launch_bounds__(kBlock) void pbulk_cut_kernel(const double *__restrict__ x, size_t xs,
                                                           const double *__restrict__ y, size_t ys, int u, int ni,
                                                           int rank, int slots, double acc_m, long long part,
                                                           const int32_t *__restrict__ seen_off,
                                                           const int32_t *__restrict__ seen,
                                                           int32_t *__restrict__ cut_item) {
  __shared__ int wtot[kTopWaves + 1];
  const PbulkBar br = pbulk_bar(acc_m, slots);
  long long before = 0;
  for (int i0 = 0; i0 < ni; i0 += kBlock) {
    const int i = i0 + static_cast<int>(threadIdx.x);
    bool is_tie = false;
    if (i < ni) {
      const double sc = pbulk_pair_acc(x, xs, y, ys, u, i, rank, slots) / br.n_slots;
      is_tie = sc == br.bar && !(seen_off && pbulk_seen(seen_off, seen, u, i));
    }
    int total;
    const int off = gtop_scan(is_tie ? 1 : 0, wtot, total);
    if (is_tie && before + off + 1 == part) *cut_item = i;
    before += total;
    if (before >= part) break;  // (uniform)
  }
}

// The admitted pairs: above the bar, or at it and (row < cut_row, or row == cut_row and item <= *cut_item).
// WRITE = false: n_adm[g] = workgroup g's.  WRITE: they go to out_k / out_s [base[g] + ...] (out_cap places).
// grid G (the count's), 256 threads.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void pbulk_emit_kernel(const double *__restrict__ x, size_t xs,
                                                            const double *__restrict__ y, size_t ys,
                                                            const int32_t *__restrict__ users, int nb, int ni, int rank,
                                                            int slots, double acc_m,
                                                            const int32_t *__restrict__ seen_off,
                                                            const int32_t *__restrict__ seen, long long cut_row,
                                                            const int32_t *__restrict__ cut_item,
                                                            long long *__restrict__ n_adm,
                                                            const long long *__restrict__ base,
                                                            uint64_t *__restrict__ out_k, double *__restrict__ out_s,
                                                            long long out_cap) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  __shared__ long long red[kBlock / kRecWave];
  __shared__ int wtot[kTopWaves + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const PbulkBar br = pbulk_bar(acc_m, slots);
  const int last_item = *cut_item;
  const long long n_it = (ni + kRecTile - 1) / kRecTile, n_ut = (nb + kRecTile - 1) / kRecTile;
  long long t0, t1;
  pbulk_run(n_it * n_ut, t0, t1);
  long long mine = 0;                                  // !WRITE: this thread's admitted pairs
  long long at = WRITE ? base[blockIdx.x] : 0;         // WRITE: the workgroup's next free place (uniform)
  for (long long t = t0; t < t1; ++t) {
    const int b0 = static_cast<int>(t / n_it) * kRecTile, i0 = static_cast<int>(t % n_it) * kRecTile;
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, users, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    uint64_t above, tie;
    pbulk_decide(acc, users, nb, ni, b0, i0, tx, ty, br, seen_off, seen, above, tie);
    uint32_t low = 0;  // columns of this thread with item <= the cut's
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) low |= (i0 + tx + 16 * c <= last_item ? 1u : 0u) << c;
    uint64_t adm = above;
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {
      const long long b = b0 + ty * kRecTm + a;
      const uint32_t rt = static_cast<uint32_t>(tie >> (kRecTm * a)) & 0xffu;
      const uint32_t in = b < cut_row ? rt : (b == cut_row ? rt & low : 0u);
      adm |= static_cast<uint64_t>(in) << (kRecTm * a);
    }
    if (!WRITE) {
      mine += __popcll(adm);
      continue;
    }
    int total;
    const int off = gtop_scan(__popcll(adm), wtot, total);
    long long o = at + off;
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {
      uint32_t rb = static_cast<uint32_t>(adm >> (kRecTm * a)) & 0xffu;
      if (rb == 0) continue;
      const int u = users[b0 + ty * kRecTm + a];
      for (; rb != 0; rb &= rb - 1, ++o) {
        const int c = __ffs(static_cast<int>(rb)) - 1;
        if (o < out_cap) {  // (always: the bases are this code's own counts; the buffer's bound all the same)
          out_k[o] = gtop_key(u, i0 + tx + 16 * c);
          out_s[o] = gtop_pick(acc[a], c) / br.n_slots;
        }
      }
    }
    at += total;
  }
  if (!WRITE) {
    const long long s = pbulk_block_sum(mine, red);
    if (tid == 0) n_adm[blockIdx.x] = s;
  }
}

}  // namespace
