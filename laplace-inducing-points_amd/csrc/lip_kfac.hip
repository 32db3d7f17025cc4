// Kronecker-factored Laplace over every layer (KFAC; KFC for convolutions): the input factor of one layer
// (lip_kfac_input_gram) and the closed-form predictive of one layer block (lip_kfac_predict).  The output factors come
// from the KRON sweep of lip_engine.hip (lip_vjp_kron).  Everything after the float32 loads in float64.
//
//   A[e][f]       += sum_{i < n} sum_{t < OH OW} at_{i,t}[e] at_{i,t}[f]
//   out[b][k][m]  += sum_{j,l} R[j][l] T_{(k,b)}[j][l] T_{(m,b)}[j][l],   T_r = V^T J_r Ub
//
// at_{i,t} is the im2col patch of image i at output position t in (kh, kw, ci) order, zero outside the image, with a
// leading 1 when the layer has a bias; J_r is the (Mt, N) block at flat offset `off` of Jacobian row r.
//
// Input Gram: ll_gram_tile (lip_gramtile.h) with an operand functor that gathers patch elements, over the lower triangle
// of 32 x 32 tiles x ranges of Gram rows (image, oh, ow); partial tiles go to scratch and the assemble step of
// lip_subnetwork.hip adds the ranges in index order, both triangles from the same sums: no atomics, bitwise
// reproducible, exactly symmetric.  The gather clamps the address and selects zero: it never reads outside the tensor.
//
// Predict: W = J Ub and T = V^T W on v_mfma_f64_16x16x4_f64 (ll_tile_mac of lip_gramtile.h), both in the caller's
// scratch, for chunks of test points that fit it; then one block per output entry walks R o T_k o T_m.  The diag form
// runs the k == m entries through the same function, so it equals the diagonal of the full form bitwise.
//
// Eigenbasis square sums (lip_kfac_eigen_sqsum, the fit-time twin of the predictive, for EKFAC):
//   Lam[j][l]     += sum_{r < R} T_r[j][l]^2
// Stage one is the predictive's (KfacBlockRows with Kc = 1); stage two forms V^T W_r tile by tile, squares it in
// registers and sums over groups of rows, so T is never written; the groups' partial sums are folded in group order.
//
// Patch projection (lip_kfac_project_patches, for the EIGEN sweep of lip_engine.hip, which forms the same Lam without
// factor rows):  AV[(i,t)][j] = sum_e at_{i,t}[e] V[e][j], float32, rounded once.  ll_project_kernel (lip_gramtile.h)
// with an operand functor that gathers the patch entries as the input Gram's does.
//
// Grid predictive (lip_kfac_predict_grid, the marginal variances at G multiples s_g of the fitted prior in one pass):
//   out[g][b][k]  += sum_{j,l} T_{(k,b)}[j][l]^2 / (Ev[j][l] + s_g)
// The weights 1 / (Ev + s_g) are divided once per call into scratch; stage one is the predictive's; stage two is the
// square-sum kernel's tile product, reduced in registers against every weight tile, one partial sum per
// (row, tile, scale); a fold adds the tiles in tile order.  T is never written, no atomics.
#include <algorithm>
#include <cmath>
#include "lip_internal.h"
#include "lip_gramtile.h"

namespace lip {

struct KfacGeom {
  int IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias, Mt;
};

// The operand pair of one lane of the patch Gram: Gram row i = (image, oh, ow), column = patch element
struct KfacPatchOperands {
  const float* __restrict__ X;
  int IH, IW, C, stride, pad_h, pad_w, OHW, OW;
  unsigned mOHW, sOHW, mOW, sOW;                     // FastDiv magic numbers of OH OW and OW
  int rh[2], rw[2], rc[2], ch[2], cw[2], cc[2];      // (kh, kw, ci) of the lane's row / column elements; kh < 0: the constant 1
  __device__ __forceinline__ void element(int e, int bias, int KW, int& kh, int& kw, int& ci) const {
    e -= bias;
    if (e < 0) { kh = -1; kw = 0; ci = 0; return; }
    ci = e % C;
    const int k = e / C;
    kw = k % KW;
    kh = k / KW;
  }
  __device__ __forceinline__ double at(int i, int kh, int kw, int ci) const {
    const int img = (int)((__umulhi((unsigned)i, mOHW) + (unsigned)i) >> sOHW), t = i - img * OHW;
    const int oh = (int)((__umulhi((unsigned)t, mOW) + (unsigned)t) >> sOW), ow = t - oh * OW;
    const int ih = oh * stride - pad_h + kh, iw = ow * stride - pad_w + kw;
    const bool in = kh >= 0 && ih >= 0 && ih < IH && iw >= 0 && iw < IW;
    const int ihc = min(max(ih, 0), IH - 1), iwc = min(max(iw, 0), IW - 1);                   // clamped: the load stays inside
    const float v = X[(((long long)img * IH + ihc) * IW + iwc) * C + ci];
    return kh < 0 ? 1.0 : (in ? (double)v : 0.0);
  }
  __device__ __forceinline__ double row(int i, int t) const { return at(i, rh[t], rw[t], rc[t]); }
  __device__ __forceinline__ double col(int i, int t) const { return at(i, ch[t], cw[t], cc[t]); }
};

__global__ __launch_bounds__(256) void kfac_input_gram_kernel(const float* __restrict__ X, KfacGeom g, int R, TriPlan pl,
                                                              FastDiv dOHW, FastDiv dOW, double* __restrict__ part) {
  __shared__ double red[3 * LL_TILE];
  const int i16 = threadIdx.x & 15;
  const int tile = blockIdx.x;
  int tr, tc;
  ll_tri_tile(tile, tr, tc);
  KfacPatchOperands op;
  op.X = X, op.IH = g.IH, op.IW = g.IW, op.C = g.C, op.stride = g.stride, op.pad_h = g.pad_h, op.pad_w = g.pad_w;
  op.OHW = g.OH * g.OW, op.OW = g.OW, op.mOHW = dOHW.m, op.sOHW = dOHW.s, op.mOW = dOW.m, op.sOW = dOW.s;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    op.element(min(tr * LL_B + 16 * t + i16, g.Mt - 1), g.bias, g.KW, op.rh[t], op.rw[t], op.rc[t]);   // clamped: never read back
    op.element(min(tc * LL_B + 16 * t + i16, g.Mt - 1), g.bias, g.KW, op.ch[t], op.cw[t], op.cc[t]);
  }
  const int ib = blockIdx.y * pl.nper;
  ll_gram_tile(op, ib, min(ib + pl.nper, R), red, part + ((long long)blockIdx.y * pl.tiles + tile) * LL_TILE);
}

// The A operand of ll_project_kernel for W (rows Mt, N) = J Ub: local row rho = (lr, j), lr = bl Kc + k the row of point
// b0 + bl and class k (source row k B + b0 + bl of Jr), j the row of its (Mt, N) block at flat offset off
struct KfacBlockRows {
  const float* __restrict__ Jr;
  long long ldj, off;
  int B, Kc, b0, Mt, N;
  typedef const float* Row;
  __device__ __forceinline__ Row row(long long r) const {
    const long long lr = r / Mt;
    const int j = (int)(r - lr * Mt), bl = (int)(lr / Kc), k = (int)(lr - (long long)bl * Kc);
    return Jr + ((long long)k * B + b0 + bl) * ldj + off + (long long)j * N;
  }
  __device__ __forceinline__ double at(Row r, int l) const { return (double)r[l]; }
};

// T_lr (Mt, N) = V^T W_lr for every local row lr: T[j][l] = sum_f V[f][j] W[f][l].  blockIdx.x = (lr, row tile), a wave
// per 32 x 32 tile, a block per four column tiles; the sum stays in f order.
__global__ __launch_bounds__(256) void kfac_vt_kernel(const double* __restrict__ V, const double* __restrict__ W, int Mt, int N,
                                                      int MT32, double* __restrict__ T) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (ct * 32 >= N) return;
  const long long lr = blockIdx.x / MT32;
  const int rt = (int)(blockIdx.x - lr * MT32);
  const double* Wr = W + lr * Mt * N;
  const double* pa[2];
  const double* pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    pa[t] = V + min(rt * 32 + 16 * t + i16, Mt - 1);                                         // clamped: never written back
    pb[t] = Wr + min(ct * 32 + 16 * t + i16, N - 1);
  }
  ll_f64x4 acc[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  ll_tile_mac(F64Cols{Mt}, pa, F64Cols{N}, pb, Mt, q, acc);
  ll_tile_store(acc, rt * 32, Mt, ct * 32, N, i16, q, T + lr * Mt * N);
}

// One entry sum_e R[e] tk[e] tm[e] by one block: a thread per e (every 256th), the threads' sums met by a fixed tree in
// LDS.  Both forms go through it, so the diag form equals the diagonal of the full form bitwise.
__device__ __forceinline__ double kfac_quad_entry(const double* __restrict__ R, const double* __restrict__ tk,
                                                  const double* __restrict__ tm, int E, double* red) {
  double t = 0.0;
  for (int e = threadIdx.x; e < E; e += 256) t = fma(R[e] * tk[e], tm[e], t);
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// block = (local point bl, pair): the full form takes the pairs k <= m and mirrors, the diag form the pairs k == m
__global__ __launch_bounds__(256) void kfac_quad_kernel(const double* __restrict__ R, const double* __restrict__ T, int Kc,
                                                        int E, int b0, int pairs, double* __restrict__ out, int diag) {
  __shared__ double red[256];
  const int bl = blockIdx.x / pairs, pair = blockIdx.x - bl * pairs;
  int k, m;
  if (diag) k = m = pair;
  else ll_tri_tile(pair, m, k);                                                              // m >= k
  const double* base = T + (long long)bl * Kc * E;
  const double t = kfac_quad_entry(R, base + (long long)k * E, base + (long long)m * E, E, red);
  if (threadIdx.x != 0) return;
  const long long b = b0 + bl;
  if (diag) {
    out[b * Kc + k] += t;
  } else {
    out[(b * Kc + k) * Kc + m] += t;
    if (m != k) out[(b * Kc + m) * Kc + k] += t;
  }
}

// The row groups of the eigenbasis square sums: each block of kfac_sqsum_kernel owns a row tile and four column tiles of
// Lam, so a small block has few of them; the local rows are split over ~1024 / blocks groups of nper consecutive rows.
struct KfacSqPlan {
  int groups, nper;
};

static long long kfac_sq_max_groups(int Mt, int N) {
  const long long blocks = (long long)((Mt + 31) / 32) * ((N + 127) / 128);
  return std::min<long long>((1024 + blocks - 1) / blocks, 1024);
}

static KfacSqPlan kfac_sq_plan(long long lrows, int Mt, int N) {
  const long long gz = std::max<long long>(1, std::min(kfac_sq_max_groups(Mt, N), lrows));
  KfacSqPlan p;
  p.nper = (int)((lrows + gz - 1) / gz);
  p.groups = (int)((lrows + p.nper - 1) / p.nper);
  return p;
}

// part_g (Mt, N) = sum_{lr in group g} T_lr o T_lr, T_lr = V^T W_lr: the product of kfac_vt_kernel (same lane map, the
// sum in f order) per local row, squared in registers and accumulated over the group's rows in row order; T is never
// written.  blockIdx = (row tile, four column tiles, group), a wave per 32 x 32 tile of Lam.
__global__ __launch_bounds__(256) void kfac_sqsum_kernel(const double* __restrict__ V, const double* __restrict__ W, int Mt,
                                                         int N, long long lrows, int nper, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (ct * 32 >= N) return;
  const int rt = blockIdx.x;
  const long long E = (long long)Mt * N;
  const long long lr0 = (long long)blockIdx.z * nper, lr1 = min(lr0 + nper, lrows);
  const double* pa[2];
  int cb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    pa[t] = V + min(rt * 32 + 16 * t + i16, Mt - 1);                                         // clamped: never written back
    cb[t] = min(ct * 32 + 16 * t + i16, N - 1);
  }
  ll_f64x4 sq[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) sq[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  for (long long lr = lr0; lr < lr1; ++lr) {
    const double* pb[2] = {W + lr * E + cb[0], W + lr * E + cb[1]};
    ll_f64x4 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
    ll_tile_mac(F64Cols{Mt}, pa, F64Cols{N}, pb, Mt, q, acc);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) sq[tm][tn][r] = fma(acc[tm][tn][r], acc[tm][tn][r], sq[tm][tn][r]);
  }
  ll_tile_store(sq, rt * 32, Mt, ct * 32, N, i16, q, part + (long long)blockIdx.z * E);
}

// Lam[e] += part_0[e] + part_1[e] + ... in group order: a thread per entry
__global__ __launch_bounds__(256) void kfac_sqsum_fold_kernel(const double* __restrict__ part, int groups, long long E,
                                                              double* __restrict__ Lam) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double t = part[e];
  for (int g = 1; g < groups; ++g) t += part[(long long)g * E + e];
  Lam[e] += t;
}

// The scales of one grid call, passed by value: every block reads its own s_g from the kernel arguments
struct KfacGridScales {
  double s[LIP_GRID_MAX];
};

// Wt[g][e] = 1 / (Ev[e] + s_g), one correctly rounded division per entry and scale: blockIdx = (256 entries, g)
__global__ __launch_bounds__(256) void kfac_grid_weights_kernel(const double* __restrict__ Ev, int E, KfacGridScales sc,
                                                                double* __restrict__ Wt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  Wt[(long long)blockIdx.y * E + e] = 1.0 / (Ev[e] + sc.s[blockIdx.y]);
}

// part[(lr, tile, g)] = sum over the tile of T_lr o T_lr o Wt_g, T_lr = V^T W_lr: the product of kfac_vt_kernel (same
// grid, same lane map, the sum in f order) squared in registers, entries past the matrix set to zero, then one pass per
// scale over the weight tile, which is read from Wt where it lies (a tile is owned by one wave, so no weight is read
// twice by a block).  A lane sums its 16 entries in register order and the wave meets in a fixed butterfly, so a slice
// depends on its own weights alone.  T is never written.
__global__ __launch_bounds__(256) void kfac_grid_kernel(const double* __restrict__ V, const double* __restrict__ W,
                                                        const double* __restrict__ Wt, int Mt, int N, int MT32, int NT32, int G,
                                                        double* __restrict__ part) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (ct * 32 >= N) return;
  const long long lr = blockIdx.x / MT32;
  const int rt = (int)(blockIdx.x - lr * MT32);
  const int E = Mt * N;
  const double* Wr = W + lr * E;
  const double* pa[2];
  const double* pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    pa[t] = V + min(rt * 32 + 16 * t + i16, Mt - 1);                                         // clamped: zeroed below
    pb[t] = Wr + min(ct * 32 + 16 * t + i16, N - 1);
  }
  ll_f64x4 acc[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = ll_f64x4{0.0, 0.0, 0.0, 0.0};
  ll_tile_mac(F64Cols{Mt}, pa, F64Cols{N}, pb, Mt, q, acc);
  // register r of lane (i16, q) is (row q + 4 r, col i16) of its 16 x 16 accumulator (ll_tile_store)
  double sq[16];
  int at[16];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 32 + 16 * tm + q + 4 * r, col = ct * 32 + 16 * tn + i16;
        const int i = (2 * tm + tn) * 4 + r;
        sq[i] = (row < Mt && col < N) ? acc[tm][tn][r] * acc[tm][tn][r] : 0.0;
        at[i] = min(row, Mt - 1) * N + min(col, N - 1);                                      // clamped: times zero
      }
  double* mine = part + ((lr * MT32 + rt) * NT32 + ct) * G;
  for (int g = 0; g < G; ++g) {
    const double* __restrict__ w = Wt + (long long)g * E;
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t = fma(sq[i], w[at[i]], t);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    if (lane == 0) mine[g] = t;
  }
}

// out[g][b0 + bl][k] += the tiles' partial sums of local row lr = bl Kc + k in tile order: a thread per (lr, g)
__global__ __launch_bounds__(256) void kfac_grid_fold_kernel(const double* __restrict__ part, long long lrows, int tiles, int G,
                                                             int B, int Kc, int b0, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= lrows * G) return;
  const long long lr = i / G;
  const int g = (int)(i - lr * G);
  const double* p = part + lr * tiles * G + g;
  double t = p[0];
  for (int tile = 1; tile < tiles; ++tile) t += p[(long long)tile * G];
  const long long bl = lr / Kc;
  const int k = (int)(lr - bl * Kc);
  out[((long long)g * B + b0 + bl) * Kc + k] += t;
}

// The A operand of ll_project_kernel for the patch projection AV = patches(X) V: row i = (image, oh, ow), element e the
// patch entry KfacPatchOperands gathers ((kh, kw, ci) order after the leading 1 of a bias; zero outside the image; the
// address clamped, so nothing outside X is read)
struct KfacPatchRows {
  const float* __restrict__ X;
  int IH, IW, C, KW, stride, pad_h, pad_w, bias, OHW, OW;
  FastDiv dOHW, dOW, dC, dKW;
  struct Row {
    long long img;
    int h0, w0;                                       // input row / column of the window's tap (0, 0)
  };
  __device__ __forceinline__ Row row(long long r) const {
    const int i = (int)r, img = dOHW.div(i), t = i - img * OHW;
    const int oh = dOW.div(t), ow = t - oh * OW;
    return Row{(long long)img, oh * stride - pad_h, ow * stride - pad_w};
  }
  __device__ __forceinline__ double at(const Row& r, int e) const {
    e -= bias;
    const int ec = max(e, 0);
    const int k = dC.div(ec), ci = ec - k * C;
    const int kh = dKW.div(k), kw = k - kh * KW;
    const int ih = r.h0 + kh, iw = r.w0 + kw;
    const bool in = ih >= 0 && ih < IH && iw >= 0 && iw < IW;
    const int ihc = min(max(ih, 0), IH - 1), iwc = min(max(iw, 0), IW - 1);                   // clamped: the load stays inside
    const float v = X[((r.img * IH + ihc) * IW + iwc) * C + ci];
    return e < 0 ? 1.0 : (in ? (double)v : 0.0);
  }
};

// Lam[e] += y[e]: a thread per entry
__global__ __launch_bounds__(256) void kfac_eigen_fold_kernel(const float* __restrict__ y, long long E, double* __restrict__ Lam) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < E) Lam[e] += (double)y[e];
}

hipError_t launch_project_patches(const float* X, int n, int IH, int IW, int C, int KH, int KW, int stride, int pad_h,
                                  int pad_w, int OH, int OW, int bias, const double* V, float* AV, hipStream_t st) {
  KfacPatchRows A;
  A.X = X, A.IH = IH, A.IW = IW, A.C = C, A.KW = KW, A.stride = stride, A.pad_h = pad_h, A.pad_w = pad_w;
  A.bias = bias ? 1 : 0, A.OHW = OH * OW, A.OW = OW;
  A.dOHW = FastDiv((unsigned)(OH * OW)), A.dOW = FastDiv((unsigned)OW), A.dC = FastDiv((unsigned)C), A.dKW = FastDiv((unsigned)KW);
  const int Mt = KH * KW * C + A.bias;
  const long long rows = (long long)n * OH * OW;
  hipLaunchKernelGGL((ll_project_kernel<KfacPatchRows, float>), dim3((unsigned)((rows + 31) / 32), (unsigned)((Mt + 127) / 128)), dim3(256),
                     0, st, A, rows, Mt, V, Mt, AV);
  return hipGetLastError();
}

hipError_t launch_eigen_fold(const float* y, long long E, double* Lam, hipStream_t st) {
  hipLaunchKernelGGL(kfac_eigen_fold_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, y, E, Lam);
  return hipGetLastError();
}

}  // namespace lip

using namespace lip;

static bool kfac_geom_ok(int32_t n, const KfacGeom& g) {
  if (n <= 0 || g.IH <= 0 || g.IW <= 0 || g.C <= 0 || g.KH <= 0 || g.KW <= 0 || g.stride <= 0 || g.pad_h < 0 || g.pad_w < 0 ||
      g.OH <= 0 || g.OW <= 0)
    return false;
  // every output position's window starts at or before the last input row / column (its rest may hang over: zeros)
  return (long long)(g.OH - 1) * g.stride - g.pad_h < g.IH && (long long)(g.OW - 1) * g.stride - g.pad_w < g.IW &&
         (long long)g.KH * g.KW * g.C + 1 <= 0x7fffffffll;
}

static KfacGeom kfac_geom(int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW, int32_t stride, int32_t pad_h,
                          int32_t pad_w, int32_t OH, int32_t OW, int32_t bias) {
  KfacGeom g;
  g.IH = IH, g.IW = IW, g.C = C, g.KH = KH, g.KW = KW, g.stride = stride, g.pad_h = pad_h, g.pad_w = pad_w, g.OH = OH, g.OW = OW;
  g.bias = bias ? 1 : 0;
  g.Mt = (int)((long long)KH * KW * C) + g.bias;
  return g;
}

// the tensors the 32-bit row arithmetic of the Gram can take: fewer than 2^31 input elements and Gram rows
static bool kfac_fits(int32_t n, const KfacGeom& g) {
  return (long long)n * g.IH * g.IW * g.C < (1ll << 31) && (long long)n * g.OH * g.OW < (1ll << 31);
}

static bool kfac_block_ok(int32_t B, int32_t Kc, int64_t off, int32_t Mt, int32_t N) {
  return B > 0 && Kc > 0 && Mt > 0 && N > 0 && off >= 0 && (long long)Mt * N < (1ll << 31) && (long long)B * Kc < (1ll << 31);
}

extern "C" {

int lip_kfac_input_gram_scratch(int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW, int32_t stride,
                                int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, int64_t* doubles) {
  const KfacGeom g = kfac_geom(IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias);
  if (!doubles || !kfac_geom_ok(n, g)) { set_error("lip_kfac_input_gram_scratch: bad argument"); return LIP_ERR_ARG; }
  if (!kfac_fits(n, g)) { set_error("lip_kfac_input_gram_scratch: a tensor of 2^31 or more elements; pass fewer images per call"); return LIP_ERR_ARG; }
  const TriPlan pl = tri_plan(n * OH * OW, g.Mt);
  *doubles = pl.tiles * pl.ys * LL_TILE;
  return LIP_OK;
}

int lip_kfac_input_gram(const float* X, int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW, int32_t stride,
                        int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, double* A, double* scratch,
                        int64_t scratch_doubles, void* stream) {
  const KfacGeom g = kfac_geom(IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias);
  if (!X || !A || !scratch || !kfac_geom_ok(n, g)) { set_error("lip_kfac_input_gram: bad argument"); return LIP_ERR_ARG; }
  if (!kfac_fits(n, g)) { set_error("lip_kfac_input_gram: a tensor of 2^31 or more elements; pass fewer images per call"); return LIP_ERR_ARG; }
  const int R = n * OH * OW;
  const TriPlan pl = tri_plan(R, g.Mt);
  const long long need = pl.tiles * pl.ys * LL_TILE;
  if (scratch_doubles < need) {
    set_error("lip_kfac_input_gram: scratch of %lld doubles, %lld needed (lip_kfac_input_gram_scratch)", (long long)scratch_doubles, need);
    return LIP_ERR_ARG;
  }
  if (pl.tiles > 0x7fffffffll || (g.Mt + 15) / 16 > 65535) { set_error("lip_kfac_input_gram: Mt = %d is too large", g.Mt); return LIP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_input_gram_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.ys), dim3(256), 0, st, X, g, R, pl,
                     FastDiv((unsigned)(OH * OW)), FastDiv((unsigned)OW), scratch);
  LIP_CHECK_HIP(hipGetLastError());
  LIP_CHECK_HIP(launch_gram_assemble(scratch, pl.tiles, pl.ys, g.Mt, A, st));
  return LIP_OK;
}

int lip_kfac_project_patches(const float* X, int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW,
                             int32_t stride, int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, const double* V,
                             float* AV, void* stream) {
  const KfacGeom g = kfac_geom(IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias);
  if (!X || !V || !AV || !kfac_geom_ok(n, g)) { set_error("lip_kfac_project_patches: bad argument"); return LIP_ERR_ARG; }
  const long long rows = (long long)n * OH * OW;
  if (!kfac_fits(n, g) || rows * g.Mt >= (1ll << 31) || (long long)g.Mt * g.Mt >= (1ll << 31) || !ll_project_fits(rows, g.Mt)) {
    set_error("lip_kfac_project_patches: a tensor of 2^31 or more elements; pass fewer images per call");
    return LIP_ERR_ARG;
  }
  LIP_CHECK_HIP(launch_project_patches(X, n, IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, g.bias, V, AV, (hipStream_t)stream));
  return LIP_OK;
}

int lip_kfac_predict_scratch(int32_t B, int32_t Kc, int32_t Mt, int32_t N, int64_t* doubles) {
  if (!doubles || !kfac_block_ok(B, Kc, 0, Mt, N)) { set_error("lip_kfac_predict_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = 2ll * B * Kc * Mt * N;                                  // W and T of every row; a (Kc, Mt, N) pair per point at least
  return LIP_OK;
}

int lip_kfac_predict(const float* Jr, int64_t ldj, int32_t B, int32_t Kc, int64_t off, int32_t Mt, int32_t N, const double* V,
                     const double* Ub, const double* R, double* out, int32_t diag, double* scratch, int64_t scratch_doubles,
                     void* stream) {
  if (!Jr || !V || !Ub || !R || !out || !scratch || !kfac_block_ok(B, Kc, off, Mt, N) || ldj < off + (long long)Mt * N) {
    set_error("lip_kfac_predict: bad argument");
    return LIP_ERR_ARG;
  }
  const int E = Mt * N, MT32 = (Mt + 31) / 32;
  const long long per_point = 2ll * Kc * E;
  if (scratch_doubles < per_point) {
    set_error("lip_kfac_predict: scratch of %lld doubles, at least %lld needed for one point (lip_kfac_predict_scratch: all points)",
              (long long)scratch_doubles, per_point);
    return LIP_ERR_ARG;
  }
  const long long pairs = diag ? (long long)Kc : (long long)Kc * (Kc + 1) / 2;
  // points per chunk: what the scratch holds, within the grids' 2^31 - 1 blocks
  long long Bc = scratch_doubles / per_point;
  Bc = std::min<long long>(Bc, B);
  Bc = std::min<long long>(Bc, 0x7fffffffll / ((long long)Kc * std::max(Mt, 32)));
  Bc = std::min<long long>(Bc, 0x7fffffffll / pairs);
  if (Bc < 1 || (N + 127) / 128 > 65535) { set_error("lip_kfac_predict: Kc = %d, Mt = %d, N = %d is too large", (int)Kc, (int)Mt, (int)N); return LIP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)((N + 127) / 128);
  for (long long b0 = 0; b0 < B; b0 += Bc) {
    const long long nb = std::min<long long>(Bc, B - b0), lrows = nb * Kc, rows = lrows * Mt;
    double* W = scratch;
    double* T = scratch + lrows * E;
    hipLaunchKernelGGL((ll_project_kernel<KfacBlockRows, double>), dim3((unsigned)((rows + 31) / 32), gy), dim3(256), 0, st,
                       KfacBlockRows{Jr, (long long)ldj, (long long)off, (int)B, (int)Kc, (int)b0, (int)Mt, (int)N}, rows, (int)N,
                       Ub, (int)N, W);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_vt_kernel, dim3((unsigned)(lrows * MT32), gy), dim3(256), 0, st, V, (const double*)W, (int)Mt, (int)N,
                       MT32, T);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_quad_kernel, dim3((unsigned)(nb * pairs)), dim3(256), 0, st, R, (const double*)T, (int)Kc, E, (int)b0,
                       (int)pairs, out, (int)diag);
    LIP_CHECK_HIP(hipGetLastError());
  }
  return LIP_OK;
}

// the doubles of a grid call that do not depend on the points (the G weight matrices) and those of one point (J Ub of its
// Kc rows and their (tile, g) partial sums)
static long long kfac_grid_fixed(int32_t Mt, int32_t N, int32_t G) { return (long long)G * Mt * N; }

static long long kfac_grid_per_point(int32_t Kc, int32_t Mt, int32_t N, int32_t G) {
  const long long tiles = (long long)((Mt + 31) / 32) * ((N + 31) / 32);
  return (long long)Kc * ((long long)Mt * N + tiles * G);
}

int lip_kfac_predict_grid_scratch(int32_t B, int32_t Kc, int32_t Mt, int32_t N, int32_t G, int64_t* doubles) {
  if (!doubles || !kfac_block_ok(B, Kc, 0, Mt, N) || G < 1 || G > LIP_GRID_MAX) {
    set_error("lip_kfac_predict_grid_scratch: bad argument");
    return LIP_ERR_ARG;
  }
  *doubles = kfac_grid_fixed(Mt, N, G) + (long long)B * kfac_grid_per_point(Kc, Mt, N, G);
  return LIP_OK;
}

int lip_kfac_predict_grid(const float* Jr, int64_t ldj, int32_t B, int32_t Kc, int64_t off, int32_t Mt, int32_t N,
                          const double* V, const double* Ub, const double* Ev, const double* scales, int32_t G, double* out,
                          double* scratch, int64_t scratch_doubles, void* stream) {
  if (!Jr || !V || !Ub || !Ev || !scales || !out || !scratch || !kfac_block_ok(B, Kc, off, Mt, N) || G < 1 || G > LIP_GRID_MAX ||
      ldj < off + (long long)Mt * N) {
    set_error("lip_kfac_predict_grid: bad argument");
    return LIP_ERR_ARG;
  }
  KfacGridScales sc;
  for (int g = 0; g < LIP_GRID_MAX; ++g) {
    sc.s[g] = g < G ? scales[g] : 1.0;
    if (!std::isfinite(sc.s[g]) || sc.s[g] <= 0.0) {
      set_error("lip_kfac_predict_grid: scale %d is not a finite positive number", g);
      return LIP_ERR_ARG;
    }
  }
  const int E = Mt * N, MT32 = (Mt + 31) / 32, NT32 = (N + 31) / 32;
  const long long fixed = kfac_grid_fixed(Mt, N, G), per_point = kfac_grid_per_point(Kc, Mt, N, G);
  if (scratch_doubles < fixed + per_point) {
    set_error("lip_kfac_predict_grid: scratch of %lld doubles, at least %lld needed for one point "
              "(lip_kfac_predict_grid_scratch: all points)", (long long)scratch_doubles, fixed + per_point);
    return LIP_ERR_ARG;
  }
  // points per chunk: what the scratch holds after the weights, within the grids' 2^31 - 1 blocks
  long long Bc = (scratch_doubles - fixed) / per_point;
  Bc = std::min<long long>(Bc, B);
  Bc = std::min<long long>(Bc, 0x7fffffffll / ((long long)Kc * std::max(Mt, 32)));
  if (Bc < 1 || (N + 127) / 128 > 65535) {
    set_error("lip_kfac_predict_grid: Kc = %d, Mt = %d, N = %d is too large", (int)Kc, (int)Mt, (int)N);
    return LIP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)((N + 127) / 128);
  double* Wt = scratch;
  hipLaunchKernelGGL(kfac_grid_weights_kernel, dim3((unsigned)((E + 255) / 256), (unsigned)G), dim3(256), 0, st, Ev, E, sc, Wt);
  LIP_CHECK_HIP(hipGetLastError());
  for (long long b0 = 0; b0 < B; b0 += Bc) {
    const long long nb = std::min<long long>(Bc, B - b0), lrows = nb * Kc, rows = lrows * Mt;
    double* W = scratch + fixed;
    double* part = W + lrows * E;
    hipLaunchKernelGGL((ll_project_kernel<KfacBlockRows, double>), dim3((unsigned)((rows + 31) / 32), gy), dim3(256), 0, st,
                       KfacBlockRows{Jr, (long long)ldj, (long long)off, (int)B, (int)Kc, (int)b0, (int)Mt, (int)N}, rows, (int)N,
                       Ub, (int)N, W);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_grid_kernel, dim3((unsigned)(lrows * MT32), gy), dim3(256), 0, st, V, (const double*)W,
                       (const double*)Wt, (int)Mt, (int)N, MT32, NT32, (int)G, part);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_grid_fold_kernel, dim3((unsigned)((lrows * G + 255) / 256)), dim3(256), 0, st, (const double*)part,
                       lrows, MT32 * NT32, (int)G, (int)B, (int)Kc, (int)b0, out);
    LIP_CHECK_HIP(hipGetLastError());
  }
  return LIP_OK;
}

int lip_kfac_eigen_sqsum_scratch(int32_t R, int32_t Mt, int32_t N, int64_t* doubles) {
  if (!doubles || !kfac_block_ok(R, 1, 0, Mt, N)) { set_error("lip_kfac_eigen_sqsum_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = ((long long)R + kfac_sq_plan(R, Mt, N).groups) * Mt * N;         // J Ub of every row and the groups' partial sums
  return LIP_OK;
}

int lip_kfac_eigen_sqsum(const float* W, int64_t ldw, int32_t R, int64_t off, int32_t Mt, int32_t N, const double* V,
                         const double* Ub, double* Lam, double* scratch, int64_t scratch_doubles, void* stream) {
  if (!W || !V || !Ub || !Lam || !scratch || !kfac_block_ok(R, 1, off, Mt, N) || ldw < off + (long long)Mt * N) {
    set_error("lip_kfac_eigen_sqsum: bad argument");
    return LIP_ERR_ARG;
  }
  const long long E = (long long)Mt * N;
  if (scratch_doubles < 2 * E) {
    set_error("lip_kfac_eigen_sqsum: scratch of %lld doubles, at least %lld needed for one row (lip_kfac_eigen_sqsum_scratch: all rows)",
              (long long)scratch_doubles, 2 * E);
    return LIP_ERR_ARG;
  }
  const int MT32 = (Mt + 31) / 32;
  if ((N + 127) / 128 > 65535) { set_error("lip_kfac_eigen_sqsum: N = %d is too large", (int)N); return LIP_ERR_ARG; }
  // rows per chunk: all R in one chunk when the scratch holds them with their groups and stage one's grid does; else a
  // chunk size under which every chunk, the shorter last one included, fits with its partial sums whatever its group
  // count (never more groups than gmax, or than rows), within the 2^31 - 1 blocks of stage one
  const long long avail = scratch_doubles / E, gmax = kfac_sq_max_groups(Mt, N), cap = 0x7fffffffll / std::max(Mt, 32);
  long long Rc = R;
  if (R > cap || avail < R + kfac_sq_plan(R, Mt, N).groups)
    Rc = std::min(std::min<long long>(R, cap), avail > 2 * gmax ? avail - gmax : avail / 2);
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)((N + 127) / 128);
  for (long long r0 = 0; r0 < R; r0 += Rc) {
    const long long nb = std::min<long long>(Rc, R - r0), rows = nb * Mt;
    const KfacSqPlan pl = kfac_sq_plan(nb, Mt, N);
    double* JU = scratch;
    double* part = scratch + nb * E;
    hipLaunchKernelGGL((ll_project_kernel<KfacBlockRows, double>), dim3((unsigned)((rows + 31) / 32), gy), dim3(256), 0, st,
                       KfacBlockRows{W, (long long)ldw, (long long)off, (int)R, 1, (int)r0, (int)Mt, (int)N}, rows, (int)N, Ub,
                       (int)N, JU);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_sqsum_kernel, dim3((unsigned)MT32, gy, (unsigned)pl.groups), dim3(256), 0, st, V, (const double*)JU,
                       (int)Mt, (int)N, nb, pl.nper, part);
    LIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfac_sqsum_fold_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, (const double*)part, pl.groups, E,
                       Lam);
    LIP_CHECK_HIP(hipGetLastError());
  }
  return LIP_OK;
}

}  // extern "C"
