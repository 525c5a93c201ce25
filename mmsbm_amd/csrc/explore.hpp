// explore.hpp -- randomised top-N with logged propensities (mmsbm_hip_recommend_query_explore /
// _recommend_list_propensity / _explore_noise): a row's list is drawn without replacement from the Plackett-Luce
// distribution over its candidates with utilities score / T, and every position comes with its probability.
//
// Semantics (the one definition).  Request row b, user u, candidates C_u = recommend_query_within's (the same subset,
// the same exclusions), s(u, i) = recommend_query's bits, temperature T > 0, a PCG64 stream (pcg64.hpp):
//   uniform  r(u, i) = draw number u * 2^32 + i of the stream, counting from 0: numpy's bg.advance(u << 32 | i), then
//            Generator.random().  A function of (stream, u, i) alone -- not of the catalogue's size, the candidates,
//            the batch or the other rows;
//   noise    E = -log(1 - r)  (1 - r is exact), E = 2^-54 where r = 0;  g = -log(E): standard Gumbel, always finite;
//   key      key(u, i) = s + T * g: the product rounded, then the sum rounded (no fma); -inf stays -inf;
//   list     the n candidates of largest key, key descending, equal keys by ascending item id: rec_select_kernel as it
//            is over the keys (Gumbel-top-n: the order of the keys IS a Plackett-Luce draw).  The SCORES are returned;
//   propensity of position t = 1 .. count:  m = max over C_u of s,  e_i = exp((s_i - m) / T) (difference and
//            quotient rounded, then the exp),  R_t = sum of e_i over the candidates not ranked above t,  p_t = e_t / R_t.
// R_t is accumulated from what remains, in a fixed order: the candidates outside the list first (a lane's columns
// ascending into four running sums, the four added left to right, a butterfly over the 64 lanes), then the list from
// its end: R_count = tail + e_count, R_t = R_(t+1) + e_t.  Only positive terms are ever added, never a full-row sum
// minus the head; the last remaining candidate of a row has tail = +0.0, so R = e and its propensity is exactly 1.0.
//
// Per batch of rows, between the exclusions and the unchanged selection, and after it:
//   explore_norm_kernel     one workgroup per row: m over the filled, excluded buffer (-inf: no candidate), and the row's
//                           stream jumped to u * 2^32 (one thread, at most 31 table steps);
//   explore_perturb_kernel  grid (spans of kExpSpan columns, rows): the score moves to a second batch buffer, the key
//                           takes its place.  A thread jumps once from the row's state to its first column and then
//                           walks its columns kBlock apart with ONE 128-bit multiply-add each (the table's 2^8-step
//                           map); under a candidate list the columns are no run of items, and every column jumps from
//                           the row's state by its item id (the candidate array);
//   explore_finish_kernel   one wave per row, after the selection: the selected columns' scores from the second buffer,
//                           their e into LDS, -inf over them in the second buffer (it is scratch), the tail over what is
//                           left, the suffix sums by one lane, the quotients by all;
//   explore_list_kernel     the same finish (explore_finish_row: one copy) over caller-given lists: an item that is no
//                           candidate of the row gets 0 / -inf and e = 0, which leaves every R as it is.
//   explore_noise_kernel    r and g of caller-given (user, item) pairs: explore_noise_at, the function the perturbation
//                           calls.
// The jumps: the state after n steps of s <- s M + c is an affine map of s; the host tabulates the maps of 2^b steps,
// b = 0 .. 63, once per call (2 KB), and a jump by delta applies the maps of delta's set bits -- they are powers of one
// map, so their order is free.  No atomics anywhere.
#pragma once
#include "pcg64.hpp"

namespace {

constexpr int kExpSpan = 8192;     // columns of one perturbing workgroup: 32 per thread
constexpr int kExpBlockLog2 = 8;   // the table entry whose map steps a thread from one of its columns to the next
static_assert((1 << kExpBlockLog2) == kBlock, "explore_perturb_kernel steps kBlock columns with one table entry");
constexpr double kExploreFloor = 700.0;  // (max w - min w) / T beyond this is refused: no e underflows below it

// tab[b * 4 ..]: {mult_hi, mult_lo, plus_hi, plus_lo} of the map of 2^b steps of the stream st = {state, inc} words
inline void explore_jump_table(const uint64_t st[4], uint64_t *tab) {
  pcg64::u128 mult = pcg64::multiplier(), plus = pcg64::make128(st[2], st[3]);
  for (int b = 0; b < 64; ++b) {
    tab[b * 4 + 0] = static_cast<uint64_t>(mult >> 64);
    tab[b * 4 + 1] = static_cast<uint64_t>(mult);
    tab[b * 4 + 2] = static_cast<uint64_t>(plus >> 64);
    tab[b * 4 + 3] = static_cast<uint64_t>(plus);
    plus = (mult + 1) * plus;
    mult *= mult;
  }
}

// the state `delta` steps on
__device__ __forceinline__ pcg64::u128 explore_jump(const uint64_t *__restrict__ tab, pcg64::u128 s, uint64_t delta) {
  while (delta) {
    const uint64_t *e = tab + 4 * (__ffsll(static_cast<unsigned long long>(delta)) - 1);
    delta &= delta - 1;
    s = s * pcg64::make128(e[0], e[1]) + pcg64::make128(e[2], e[3]);
  }
  return s;
}

// g of the uniform r
__device__ __forceinline__ double explore_gumbel(double r) {
  const double E = r == 0.0 ? 0x1p-54 : -log(1.0 - r);
  return -log(E);
}

// r and g of the draw that follows state `s` of the stream with increment `inc`
__device__ __forceinline__ void explore_noise_at(pcg64::u128 s, pcg64::u128 inc, double &r, double &g) {
  pcg64::Stream st{s, inc};
  r = pcg64::next_double(st);
  g = explore_gumbel(r);
}

__device__ __forceinline__ double explore_key(double s, double T, double g) {
#pragma clang fp contract(off)
  const double t = T * g;
  return s + t;
}

__device__ __forceinline__ double explore_e(double s, double m, double T) {
#pragma clang fp contract(off)
  const double d = s - m;
  const double q = d / T;
  return exp(q);
}

// grid (rows of the batch).  mx[b] = the largest entry of row b of scores (-inf: no candidate); base (null: not wanted)
// [b * 2 ..] = {hi, lo} of the stream's state users[b] * 2^32 steps on from s0.
__global__ __launch_bounds__(kBlock) void explore_norm_kernel(const double *__restrict__ scores, size_t ld, int C,
                                                              const int32_t *__restrict__ users,
                                                              const uint64_t *__restrict__ tab, uint64_t s0_hi,
                                                              uint64_t s0_lo, double *__restrict__ mx,
                                                              uint64_t *__restrict__ base) {
  __shared__ double red[kBlock / kRecWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double *row = scores + static_cast<size_t>(b) * ld;
  double m = -INFINITY;
  for (int i = tid; i < C; i += kBlock) m = fmax(m, row[i]);
  for (int o = kRecWave / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, kRecWave));
  if (tid % kRecWave == 0) red[tid / kRecWave] = m;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kBlock / kRecWave; ++w) m = fmax(m, red[w]);
  mx[b] = m;
  if (base) {
    const pcg64::u128 s = explore_jump(tab, pcg64::make128(s0_hi, s0_lo), static_cast<uint64_t>(users[b]) << 32);
    base[static_cast<size_t>(b) * 2] = static_cast<uint64_t>(s >> 64);
    base[static_cast<size_t>(b) * 2 + 1] = static_cast<uint64_t>(s);
  }
}

// grid (spans of kExpSpan columns, rows of the batch).  raw[b][i] = scores[b][i], then scores[b][i] = its key; column i
// is item cand[i], or item i without cand.  base: explore_norm_kernel's; inc: the stream's increment.
__global__ __launch_bounds__(kBlock) void explore_perturb_kernel(double *__restrict__ scores, double *__restrict__ raw,
                                                                 size_t ld, int C, const int32_t *__restrict__ cand,
                                                                 const uint64_t *__restrict__ tab,
                                                                 const uint64_t *__restrict__ base, uint64_t inc_hi,
                                                                 uint64_t inc_lo, double T) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lo = blockIdx.x * kExpSpan, hi = min(C, lo + kExpSpan);
  double *row = scores + static_cast<size_t>(b) * ld, *keep = raw + static_cast<size_t>(b) * ld;
  const pcg64::u128 inc = pcg64::make128(inc_hi, inc_lo);
  const pcg64::u128 s_row = pcg64::make128(base[static_cast<size_t>(b) * 2], base[static_cast<size_t>(b) * 2 + 1]);
  const uint64_t *e = tab + 4 * kExpBlockLog2;
  const pcg64::u128 mult = pcg64::make128(e[0], e[1]), plus = pcg64::make128(e[2], e[3]);
  int i = lo + tid;
  if (i >= hi) return;
  pcg64::u128 st = cand ? 0 : explore_jump(tab, s_row, static_cast<uint64_t>(i));
  for (; i < hi; i += kBlock) {
    const double s = row[i];
    keep[i] = s;
    if (s != -INFINITY) {  // (-inf stays -inf: its noise is never formed)
      double r, g;
      explore_noise_at(cand ? explore_jump(tab, s_row, static_cast<uint64_t>(cand[i])) : st, inc, r, g);
      row[i] = explore_key(s, T, g);
    }
    st = st * mult + plus;
  }
}

// The propensities of one row's list, all lanes of a one-wave workgroup.  row [C]: the row's unperturbed scores (-inf:
// no candidate), written: -inf over the list's columns; m: their largest.  Entry k < cnt of the list is ent[k]: a column,
// or with col_of an item whose column is col_of[item] (-1: none).  out_s / out_p [k]: its score and propensity, -inf / 0
// where it is no candidate of the row.  es / rs: kRecMaxN doubles of LDS each.
__device__ __forceinline__ void explore_finish_row(double *__restrict__ row, int C, double m, double T,
                                                   const int32_t *__restrict__ ent, const int32_t *__restrict__ col_of,
                                                   int cnt, double *__restrict__ out_s, double *__restrict__ out_p,
                                                   double *es, double *rs) {
  const int lane = threadIdx.x;
  for (int k = lane; k < cnt; k += kRecWave) {
    const int col = col_of ? col_of[ent[k]] : ent[k];
    const double s = col >= 0 ? row[col] : -INFINITY;
    out_s[k] = s;
    es[k] = s != -INFINITY ? explore_e(s, m, T) : 0.0;
    if (s != -INFINITY) row[col] = -INFINITY;  // (the list's entries are distinct: one lane per column)
  }
  __syncthreads();  // (the row's -inf and es are written before they are read)
  double acc[kRecPerLane] = {0.0, 0.0, 0.0, 0.0};
  static_assert(kRecPerLane == 4, "explore_finish_row adds four running sums left to right");
  for (int base = 0; base < C; base += kRecWave * kRecPerLane) {
    double sv[kRecPerLane];
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const int i = base + e * kRecWave + lane;
      sv[e] = i < C ? row[i] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e)
      if (sv[e] != -INFINITY) acc[e] += explore_e(sv[e], m, T);
  }
  double tail = ((acc[0] + acc[1]) + acc[2]) + acc[3];
  for (int o = kRecWave / 2; o > 0; o >>= 1) tail += __shfl_xor(tail, o, kRecWave);  // (the same bits in every lane)
  if (lane == 0) {
    double R = tail;
    for (int k = cnt - 1; k >= 0; --k) {
      R += es[k];
      rs[k] = R;
    }
  }
  __syncthreads();
  for (int k = lane; k < cnt; k += kRecWave) out_p[k] = es[k] > 0.0 ? es[k] / rs[k] : 0.0;
}

// grid (rows of the batch), one wave per workgroup.  sel / sel_n: the selection's output of the batch ([b * n + k],
// k < sel_n[b]: columns of raw); out_s / out_p [b * n + k].
__global__ __launch_bounds__(kRecWave) void explore_finish_kernel(double *__restrict__ raw, size_t ld, int C,
                                                                  const double *__restrict__ mx, double T,
                                                                  const int32_t *__restrict__ sel,
                                                                  const int32_t *__restrict__ sel_n, int n,
                                                                  double *__restrict__ out_s,
                                                                  double *__restrict__ out_p) {
  __shared__ double es[kRecMaxN], rs[kRecMaxN];
  const size_t b = blockIdx.x, o = b * n;
  explore_finish_row(raw + b * ld, C, mx[b], T, sel + o, nullptr, sel_n[b], out_s + o, out_p + o, es, rs);
}

// grid (rows of the batch), one wave per workgroup.  Row b's list is item[off[b] .. off[b + 1]) (at most kRecMaxN
// distinct items of the catalogue; off counted from the call's first row); col_of: every item's column of raw, or null
// where the columns are the items.  out_s / out_p [off[b] + k].
__global__ __launch_bounds__(kRecWave) void explore_list_kernel(double *__restrict__ raw, size_t ld, int C,
                                                                const double *__restrict__ mx, double T,
                                                                const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ item,
                                                                const int32_t *__restrict__ col_of,
                                                                double *__restrict__ out_s,
                                                                double *__restrict__ out_p) {
  __shared__ double es[kRecMaxN], rs[kRecMaxN];
  const size_t b = blockIdx.x;
  const int lo = off[b], cnt = off[b + 1] - lo;
  explore_finish_row(raw + b * ld, C, mx[b], T, item + lo, col_of, cnt, out_s + lo, out_p + lo, es, rs);
}

// r[p], g[p] of the pair (users[p], items[p]), p < n_pairs
__global__ __launch_bounds__(kBlock) void explore_noise_kernel(const uint64_t *__restrict__ tab, uint64_t s0_hi,
                                                               uint64_t s0_lo, uint64_t inc_hi, uint64_t inc_lo,
                                                               const int32_t *__restrict__ users,
                                                               const int32_t *__restrict__ items, int64_t n_pairs,
                                                               double *__restrict__ r, double *__restrict__ g) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= n_pairs) return;
  const uint64_t at = (static_cast<uint64_t>(users[p]) << 32) | static_cast<uint64_t>(items[p]);
  explore_noise_at(explore_jump(tab, pcg64::make128(s0_hi, s0_lo), at), pcg64::make128(inc_hi, inc_lo), r[p], g[p]);
}

}  // namespace
