// overlap.hpp -- the overlap of the restarts' groups (mmsbm_hip_overlap_*): the Gram matrix of the added slots'
// membership tables of one side, on the device.
//
// Users (side 1; items, side 0, are the same with eta, L and I): the S added slots' theta tables side by side are
// X [rows][F], F = S G, column f = s G + a = group a of the s-th slot added, and
//   out[f][g] = sum_row X[row, f] X[row, g]                                       (F x F, row-major)
// -- how much of the population two groups share.  align.py matches the groups of two restarts on its blocks.
// Per slot added, rec_fold_kernel (recommend.hpp) with no matrix copies the slot's rows, external sides, into the
// session table [slot][rows][G].  Per query:
//   ovl_gram_kernel     one workgroup per (tile pair on or above the diagonal, slab of rows): a 64 x 64 output tile, 4 x 4
//                       outputs per thread on the vector ALU, both operand tiles staged through LDS 16 rows at a time
//                       (plain copies of pieces of table rows: the contraction runs over the rows; the next step's
//                       values are loaded into registers while this step is multiplied), into the slab's partial tile;
//   ovl_combine_kernel  one thread per output: the slabs' partial results added in place in a fixed tree, the sum written
//                       to out[f][g] and to out[g][f].
// Operation order -- the contract:
//   * the rows are cut into slabs of kOvlSlab rows (a compile-time constant; the last slab may be shorter);
//   * inside a slab an output is ONE fma chain over the slab's rows in ascending order from +0.0 (rows beyond the
//     table take no part: no padding term);
//   * the slabs' partial results p[0 .. n) are combined pairwise in slab order: p[s] += p[s + d] for every s that is a
//     multiple of 2 d with s + d < n, for d = 1, 2, 4, ...; the sum is p[0];
//   * no atomics.
// So an output depends on its two columns and on the number of rows only -- not on S, on the tile the columns fall
// into, on the number of CUs, on the side layout (a swapped context gives the same bits: the session table is read
// through ext_slot) or on slots the context holds beyond those added.  x y and y x are the same product, so the two
// halves of a diagonal tile agree bit for bit, and every tile below the diagonal is the written mirror of the one
// above: out[f][g] and out[g][f] are the same bits.
// No v_mfma_f64 form: the fp64 matrix rate equals the vector rate on gfx950, and the fma form keeps every output's
// operation order explicit.
#pragma once

namespace {

constexpr int kOvlTile = 64;                // columns x columns of one output tile
constexpr int kOvlTm = 4;                   // outputs per thread along each side (16 x 16 threads)
constexpr int kOvlRc = 16;                  // rows staged in LDS per step
constexpr int kOvlLdsRow = kOvlTile + 2;    // (padded LDS row, 16-byte aligned rows)
constexpr int kOvlSlab = 2048;              // B: rows of one slab

// The tile pair (ti <= tj) of workgroup `idx` among the nt (nt + 1) / 2 pairs, row by row of the upper triangle
__device__ __forceinline__ void ovl_tile_pair(int idx, int nt, int &ti, int &tj) {
  ti = 0;
  while (idx >= nt - ti) {
    idx -= nt - ti;
    ++ti;
  }
  tj = ti + idx;
}

// part[(slab * pairs + pair) * 64 * 64 + i * 64 + j] = sum over the slab's rows of X[row, ti * 64 + i] X[row, tj * 64 + j]
// tab: `slots` tables [rows][G], qs doubles apart; column f of X is column f % G of table f / G.
// One workgroup per (slab, tile pair): blockIdx.x = slab * pairs + pair.
__global__ __launch_bounds__(kBlock) void ovl_gram_kernel(const double *__restrict__ tab, size_t qs, int rows, int G,
                                                          int F, int nt, int pairs, double *__restrict__ part) {
  __shared__ double xt[kOvlRc][kOvlLdsRow];
  __shared__ double yt[kOvlRc][kOvlLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  int ti, tj;
  ovl_tile_pair(static_cast<int>(blockIdx.x % pairs), nt, ti, tj);
  const int row0 = static_cast<int>(blockIdx.x / pairs) * kOvlSlab;  // (< rows: no overflow)
  const int row1 = rows - row0 > kOvlSlab ? row0 + kOvlSlab : rows;
  double acc[kOvlTm][kOvlTm];
#pragma unroll
  for (int a = 0; a < kOvlTm; ++a)
#pragma unroll
    for (int c = 0; c < kOvlTm; ++c) acc[a][c] = 0.0;
  // the column this thread stages in both tiles: j = tid % 64, of rows tid / 64 + 4 m of the step
  const int j = tid % kOvlTile, fx = ti * kOvlTile + j, fy = tj * kOvlTile + j;
  const double *xcol = fx < F ? tab + static_cast<size_t>(fx / G) * qs + fx % G : nullptr;
  const double *ycol = fy < F ? tab + static_cast<size_t>(fy / G) * qs + fy % G : nullptr;
  // the step's values wait in registers while the step before is multiplied out of the LDS: the loads of step n + 1
  // are in flight during the fmas of step n (the order of the fmas is untouched)
  constexpr int kPer = kOvlTile * kOvlRc / kBlock;
  double xn[kPer], yn[kPer];
  auto fetch = [&](int r0) {
    const int rc = min(kOvlRc, row1 - r0);
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int rr = tid / kOvlTile + (kBlock / kOvlTile) * m;
      const size_t at = static_cast<size_t>(r0 + rr) * G;
      const bool in = rr < rc;
      xn[m] = in && xcol ? xcol[at] : 0.0;
      yn[m] = in && ycol ? ycol[at] : 0.0;
    }
  };
  if (row0 < row1) fetch(row0);
  for (int r0 = row0; r0 < row1; r0 += kOvlRc) {
    const int rc = min(kOvlRc, row1 - r0);
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int rr = tid / kOvlTile + (kBlock / kOvlTile) * m;
      xt[rr][j] = xn[m];
      yt[rr][j] = yn[m];
    }
    __syncthreads();
    if (r0 + kOvlRc < row1) fetch(r0 + kOvlRc);
    for (int rr = 0; rr < rc; ++rr) {
      double xa[kOvlTm], yc[kOvlTm];
#pragma unroll
      for (int a = 0; a < kOvlTm; ++a) xa[a] = xt[rr][ty * kOvlTm + a];
#pragma unroll
      for (int c = 0; c < kOvlTm; ++c) yc[c] = yt[rr][tx + 16 * c];  // (neighbouring lanes: neighbouring columns)
#pragma unroll
      for (int a = 0; a < kOvlTm; ++a)
#pragma unroll
        for (int c = 0; c < kOvlTm; ++c) acc[a][c] = fma(xa[a], yc[c], acc[a][c]);
    }
    __syncthreads();
  }
  double *tile = part + static_cast<size_t>(blockIdx.x) * (kOvlTile * kOvlTile);
#pragma unroll
  for (int a = 0; a < kOvlTm; ++a)
#pragma unroll
    for (int c = 0; c < kOvlTm; ++c) tile[(ty * kOvlTm + a) * kOvlTile + tx + 16 * c] = acc[a][c];
}

// out[f * F + g] = out[g * F + f] = the slabs' partial results of (f, g) combined in the fixed tree (header), in place
// in `part`; f = ti * 64 + i <= g = tj * 64 + j.  One thread per entry of every tile pair: blockIdx.x = pair * 16 + the
// sixteenth of the tile.
__global__ __launch_bounds__(kBlock) void ovl_combine_kernel(double *__restrict__ part, int slabs, int F, int nt,
                                                             int pairs, double *__restrict__ out) {
  constexpr int kPer = kOvlTile * kOvlTile / kBlock;
  const int pair = static_cast<int>(blockIdx.x / kPer);
  const int e = static_cast<int>(blockIdx.x % kPer) * kBlock + threadIdx.x, i = e / kOvlTile, j = e % kOvlTile;
  int ti, tj;
  ovl_tile_pair(pair, nt, ti, tj);
  const int f = ti * kOvlTile + i, g = tj * kOvlTile + j;
  if (f >= F || g >= F || f > g) return;  // (the lower half of a diagonal tile holds the same bits as the upper)
  const size_t step = static_cast<size_t>(pairs) * (kOvlTile * kOvlTile);  // from a slab's tile to the next slab's
  double *p = part + static_cast<size_t>(pair) * (kOvlTile * kOvlTile) + e;
  for (int d = 1; d < slabs; d *= 2)
    for (int s = 0; s + d < slabs; s += 2 * d) p[s * step] += p[(s + d) * step];
  const double v = p[0];
  out[static_cast<size_t>(f) * F + g] = v;
  out[static_cast<size_t>(g) * F + f] = v;
}

}  // namespace
