// The float64 Gram tile loop shared by the last-layer kernels (lip_lastlayer.hip) and the subnetwork kernels
// (lip_subnetwork.hip): a 32 x 32 tile of sum_i row_i col_i^T over a range of examples on v_mfma_f64_16x16x4_f64, the
// operands supplied by a functor, and the split of the examples over blocks that goes with it.
#ifndef LIP_GRAMTILE_H
#define LIP_GRAMTILE_H
#include "lip_internal.h"

namespace lip {

constexpr int LL_B = 32;                    // tile edge
constexpr int LL_TILE = LL_B * LL_B;
constexpr int LL_CHUNK = 16;                // examples per wave step (four MFMA k-steps of 4)
constexpr int LL_SPAN = 4 * LL_CHUNK;       // examples the four waves of a block cover per round
typedef double ll_f64x4 __attribute__((ext_vector_type(4)));

// split n examples over ys ranges of nper (whole spans) until a launch of `tiles` tiles has ~4 blocks per CU
static void ll_split(int n, long long tiles, int& ys_out, int& nper) {
  long long spans = ((long long)n + LL_SPAN - 1) / LL_SPAN, ys = (1024 + tiles - 1) / tiles;
  if (ys > spans) ys = spans;
  if (ys > 4096) ys = 4096;
  if (ys < 1) ys = 1;
  nper = (int)((spans + ys - 1) / ys) * LL_SPAN;
  ys_out = (int)(((long long)n + nper - 1) / nper);
}

// One 32 x 32 partial tile sum_{i in [ib, ie)} row_i col_i^T of a block: its four waves take every fourth 16-example
// chunk on v_mfma_f64_16x16x4_f64, meet in LDS (red, 3 tiles) in wave order, and wave 0 writes the tile to mine.
template <class Operands>
__device__ __forceinline__ void ll_gram_tile(const Operands& op, int ib, int ie, double* __restrict__ red,
                                             double* __restrict__ mine) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  ll_f64x4 acc[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int i0 = ib + LL_CHUNK * wave; i0 < ie; i0 += LL_SPAN) {
    double a[4][2], b[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int i = i0 + 4 * s + q;                  // k-step s of the chunk: this lane's example
      const bool ok = i < ie;
      const int ic = ok ? i : ie - 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double av = op.row(ic, t);
        const double bv = op.col(ic, t);
        a[s][t] = ok ? av : 0.0;
        b[s][t] = ok ? bv : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][0], b[s][0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][0], b[s][1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][1], b[s][0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][1], b[s][1], acc[1][1], 0, 0, 0);
    }
  }
  // C/D map of v_mfma_f64_16x16x4_f64: register r of lane l holds (row = (l >> 4) + 4 r, col = l & 15)
  if (wave > 0) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave - 1) * LL_TILE + (16 * tm + q + 4 * r) * LL_B + 16 * tn + i16] = acc[tm][tn][r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = (16 * tm + q + 4 * r) * LL_B + 16 * tn + i16;
          mine[e] = ((acc[tm][tn][r] + red[e]) + red[LL_TILE + e]) + red[2 * LL_TILE + e];
        }
  }
}

// (row, column) of lower-triangle tile number `tile`, rows first: tile = tr (tr + 1) / 2 + tc, tc <= tr
__device__ __forceinline__ void ll_tri_tile(int tile, int& tr, int& tc) {
  tr = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((tr + 1) * (tr + 2) / 2 <= tile) ++tr;
  while (tr * (tr + 1) / 2 > tile) --tr;
  tc = tile - tr * (tr + 1) / 2;
}

// The Gram of a compact float32 (R, S) panel's columns (lip_subnetwork.hip: sub_gram_kernel, then sub_assemble_kernel),
// for the translation units that Gram-multiply panels of their own: G (S, S) += panel^T panel through `part`
// (>= panel_gram_scratch(R, S) doubles), and the assemble step alone for partial tiles a caller's own kernel wrote with
// ll_gram_tile (ys ranges of `tiles` lower-triangle tiles each, added in index order, both triangles from the same sums).
bool panel_gram_fits(int R, int S);
long long panel_gram_scratch(int R, int S);
hipError_t launch_panel_gram(const float* panel, int R, int S, double* G, double* part, hipStream_t st);
hipError_t launch_gram_assemble(const double* part, long long tiles, int ys, int S, double* G, hipStream_t st);

}  // namespace lip

#endif  // LIP_GRAMTILE_H
