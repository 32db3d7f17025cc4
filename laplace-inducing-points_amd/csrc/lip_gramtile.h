// The float64 Gram tile loop shared by the last-layer kernels (lip_lastlayer.hip) and the subnetwork kernels
// (lip_subnetwork.hip): a 32 x 32 tile of sum_i row_i col_i^T over a range of examples on v_mfma_f64_16x16x4_f64, the
// operands supplied by a functor, and the split of the examples over blocks that goes with it; and the float64 tile
// product of a wave, out = A B in k order (ll_tile_mac, ll_tile_store, ll_tile16_mac), that the predictives and the two
// projections of the EIGEN sweep share (ll_project_kernel).
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

// The operands of the tile products below are functors: a Row handle a lane prepares once per output row or column, and
// at(handle, l), the float64 value of its element l, which never reads outside its tensor for 0 <= l < L.
// float32 rows, row r at P + r ld, up-cast before any multiplication
struct F32Rows {
  const float* __restrict__ P;
  long long ld;
  typedef const float* Row;
  __device__ __forceinline__ Row row(long long r) const { return P + r * ld; }
  __device__ __forceinline__ double at(Row r, int l) const { return (double)r[l]; }
};

// float64 columns of a row-major matrix with leading dimension ld: the handle points at the column's first element
struct F64Cols {
  int ld;
  typedef const double* Row;
  __device__ __forceinline__ double at(Row c, int l) const { return c[(long long)l * ld]; }
};

// acc[tm][tn] += sum_{l < L} A.at(ra[tm], l) B.at(rb[tn], l) for the 32 x 32 tile of one wave, four 16 x 16 accumulators
// of v_mfma_f64_16x16x4_f64: lane (i16, q) holds row / column i16 of each half and k-step q.  The sum runs in l order.
template <class AOp, class BOp>
__device__ __forceinline__ void ll_tile_mac(const AOp& A, const typename AOp::Row (&ra)[2], const BOp& B,
                                            const typename BOp::Row (&rb)[2], int L, int q, ll_f64x4 (&acc)[2][2]) {
  int l0 = 0;
  // four k-steps per round, every load issued before the first product
  for (; l0 + 16 <= L; l0 += 16) {
    double a[4][2], b[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int l = l0 + 4 * s + q;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[s][t] = A.at(ra[t], l);
        b[s][t] = B.at(rb[t], l);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][tm], b[s][tn], acc[tm][tn], 0, 0, 0);
  }
  for (; l0 < L; l0 += 4) {
    const int l = l0 + q;
    const bool ok = l < L;
    const int lc = ok ? l : L - 1;
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const double av = A.at(ra[t], lc), bv = B.at(rb[t], lc);
      a[t] = ok ? av : 0.0;
      b[t] = ok ? bv : 0.0;
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
  }
}

// the tile of ll_tile_mac at (r0, c0) into row-major out (rows, cols), rounded to Out: register r of lane (i16, q) is
// (row q + 4 r, col i16) of its 16 x 16 accumulator; entries past the matrix are never stored.  Idx is the width of the
// row arithmetic: int where rows fits one, long long otherwise.
template <class Idx, class Out>
__device__ __forceinline__ void ll_tile_store(const ll_f64x4 (&acc)[2][2], Idx r0, Idx rows, int c0, int cols,
                                              int i16, int q, Out* __restrict__ out) {
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const Idx row = r0 + 16 * tm + q + 4 * r;
        const int col = c0 + 16 * tn + i16;
        if (row < rows && col < cols) out[(long long)row * cols + col] = (Out)acc[tm][tn][r];
      }
}

// The single-accumulator form: acc += sum_{l < L} a(l) b(l) for the 16 x 16 tile of one wave, a and b the lane's own row
// and column as callables, STEPS k-steps per round with every load issued before the first product, the sum in l order.
template <int STEPS, class AFn, class BFn>
__device__ __forceinline__ ll_f64x4 ll_tile16_mac(const AFn& a, const BFn& b, int L, int q) {
  ll_f64x4 acc = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  int l0 = 0;
  for (; l0 + 4 * STEPS <= L; l0 += 4 * STEPS) {
    double av[STEPS], bv[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      av[s] = a(l0 + 4 * s + q);
      bv[s] = b(l0 + 4 * s + q);
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
  }
  for (; l0 < L; l0 += 4) {
    const int l = l0 + q;
    const bool ok = l < L;
    const int lc = ok ? l : L - 1;
    const double av = a(lc), bv = b(lc);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ok ? av : 0.0, ok ? bv : 0.0, acc, 0, 0, 0);
  }
  return acc;
}

// out (rows, cols) = A (rows, L) B (L, cols): A's elements come from a functor (float32 values, up-cast before any
// multiplication), B is float64 row-major, the sum runs in l order on v_mfma_f64_16x16x4_f64 and is rounded ONCE on the
// store (Out = float), or not at all (Out = double).  A wave per 32 x 32 tile of out, a block per row tile and four
// column tiles: grid = (ceil(rows / 32), ceil(cols / 128)).  Rows and columns past the matrix are clamped on the loads
// and never stored; A.row(r) prepares a row once per lane, A.at(row, l) reads one element and never reads outside its
// tensor.
template <class AOp, class Out>
__global__ __launch_bounds__(256) void ll_project_kernel(const AOp A, long long rows, int L, const double* __restrict__ B,
                                                         int cols, Out* __restrict__ out) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (ct * 32 >= cols) return;
  const long long r0 = (long long)blockIdx.x * 32;
  typename AOp::Row ra[2];
  const double* pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long long r = r0 + 16 * t + i16;
    ra[t] = A.row(r < rows ? r : rows - 1);                                                  // clamped: never written back
    pb[t] = B + min(ct * 32 + 16 * t + i16, cols - 1);
  }
  ll_f64x4 acc[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  ll_tile_mac(A, ra, F64Cols{cols}, pb, L, q, acc);
  ll_tile_store(acc, r0, rows, ct * 32, cols, i16, q, out);
}

// can ll_project_kernel's grid take a (rows, cols) output?
inline bool ll_project_fits(long long rows, int cols) { return (rows + 31) / 32 <= 0x7fffffffll && (cols + 127) / 128 <= 65535; }

// (row, column) of lower-triangle tile number `tile`, rows first: tile = tr (tr + 1) / 2 + tc, tc <= tr
__device__ __forceinline__ void ll_tri_tile(int tile, int& tr, int& tc) {
  tr = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((tr + 1) * (tr + 2) / 2 <= tile) ++tr;
  while (tr * (tr + 1) / 2 > tile) --tr;
  tc = tile - tr * (tr + 1) / 2;
}

// The lower triangle of 32 x 32 tiles of an (S, S) Gram over R rows, the rows split over ys ranges
struct TriPlan {
  int T;                 // tiles per edge
  long long tiles;       // lower-triangle tiles
  int ys, nper;          // row ranges and rows per range (a multiple of LL_SPAN)
};

static TriPlan tri_plan(int R, int S) {
  TriPlan p;
  p.T = (S + LL_B - 1) / LL_B;
  p.tiles = (long long)p.T * (p.T + 1) / 2;
  ll_split(R, p.tiles, p.ys, p.nper);
  return p;
}

// The Gram of a compact float32 (R, S) panel's columns (lip_subnetwork.hip: sub_gram_kernel, then sub_assemble_kernel),
// for the translation units that Gram-multiply panels of their own: G (S, S) += panel^T panel through `part`
// (>= panel_gram_scratch(R, S) doubles), and the assemble step alone for partial tiles a caller's own kernel wrote with
// ll_gram_tile (ys ranges of `tiles` lower-triangle tiles each, added in index order, both triangles from the same sums).
bool panel_gram_fits(int R, int S);
long long panel_gram_scratch(int R, int S);
hipError_t launch_panel_gram(const float* panel, int R, int S, double* G, double* part, hipStream_t st);
hipError_t launch_gram_assemble(const double* part, long long tiles, int ys, int S, double* G, hipStream_t st);

// The two projections of the EIGEN sweep of lip_engine.hip, on operands the caller has checked (the entry points
// lip_kfac_project_patches / lip_rows_project check and then call these):
//   AV ((n OH OW), Mt) = patches(X) V      (lip_kfac.hip; the geometry arguments of lip_kfac_input_gram)
//   GU ((P R), N)      = G Ub              (lip_subnetwork.hip; row r of probe p at G + p pstride + r ldg)
// and the fold of a pass's float32 sums into a block's float64 second moments, Lam[e] += y[e].
hipError_t launch_project_patches(const float* X, int n, int IH, int IW, int C, int KH, int KW, int stride, int pad_h,
                                  int pad_w, int OH, int OW, int bias, const double* V, float* AV, hipStream_t st);
hipError_t launch_rows_project(const float* G, long long ldg, long long pstride, int P, int R, int N, const double* Ub,
                               float* GU, hipStream_t st);
hipError_t launch_eigen_fold(const float* y, long long E, double* Lam, hipStream_t st);

}  // namespace lip

#endif  // LIP_GRAMTILE_H
