// Last-layer Laplace: the dense GGN block of the final Dense layer from the cached penultimate features and softmax
// probabilities (lip_ll_ggn), and the matching test-time quadratic form (lip_ll_predict).  Everything in float64.
//
// With phit_i = [1, phi_i] (Ft = F + 1 entries) and theta_L = [bias (K), kernel (F, K) row-major], flat index r = f K + k:
//   G[(f,k)][(g,l)] = sum_i phit_i[f] phit_i[g] H_i[k][l],   H_i = diag(p_i) - p_i p_i^T  (softmax)  or  I  (Gaussian).
// The H = diag - outer split turns the n K rank-one terms of length DL into two plain Grams over the examples:
//   UU[r][c]      = sum_i U_i[r] U_i[c],          U_i[(f,k)] = phit_i[f] p_i[k]    (DL x DL, lower triangle of tiles)
//   D[f][(g,l)]   = sum_i phit_i[f] U_i[(g,l)]                                      (Ft x DL, tiles with f <= g)
//   G[(f,k)][(g,l)] = delta_kl D[min(f,g)][(max(f,g), l)] - UU[max(r,c)][min(r,c)]
// (Gaussian head: D[f][g] = sum_i phit_i[f] phit_i[g] alone, Kc = 1 column per g.)  U_i[r] is a product of two float32
// values, exact in float64, so every term is rounded once where the matrix pipe adds it.  Nothing of size (n, DL) is
// ever written: the operands are rebuilt from Phi and Pr in registers.
//
// Work split: block = one 32 x 32 tile x one range of examples (blockIdx.y); its four waves take every fourth 16-example
// chunk on v_mfma_f64_16x16x4_f64 (the operand and C/D maps of dot_nt_f64_mfma_kernel in lip_krylov.hip) and meet in LDS
// in wave order.  Every block writes its partial tile to the caller's scratch; ll_assemble_kernel adds the ranges in
// index order and applies the formula above.  No atomics anywhere: the summation order is a function of (n, F, K) alone,
// so the result is bitwise reproducible, and both (r, c) and (c, r) read the same partial sums, so G stays symmetric.
//
// The Kronecker-factored posterior (lip_ll_kron_factors, lip_ll_kron_predict; second half of the file) takes the same
// tile loop, ll_gram_tile (lip_gramtile.h), with another operand functor: its two factors are plain Grams of [1, phi_i]
// and [1, p_i].
#include "lip_internal.h"
#include "lip_gramtile.h"

namespace lip {

struct LLPlan {
  int DL, Ft, Kc;        // Kc: classes per feature in the column space (K for softmax, 1 for the Gaussian head)
  int T, Tuu;            // tiles per edge of the DL space; lower-triangle tiles of UU (0 for the Gaussian head)
  int TF, Tc;            // row tiles of D (over Ft), column tiles of D (over Ft * Kc)
  long long tiles;       // Tuu + TF * Tc
  int ys, nper;          // example ranges and examples per range (a multiple of LL_SPAN)
};

static LLPlan ll_plan(int n, int F, int K, bool softmax) {
  LLPlan p;
  p.Ft = F + 1;
  p.DL = p.Ft * K;
  p.Kc = softmax ? K : 1;
  p.T = (p.DL + LL_B - 1) / LL_B;
  p.Tuu = softmax ? (int)((long long)p.T * (p.T + 1) / 2) : 0;
  p.TF = (p.Ft + LL_B - 1) / LL_B;
  p.Tc = (p.Ft * p.Kc + LL_B - 1) / LL_B;
  p.tiles = (long long)p.Tuu + (long long)p.TF * p.Tc;
  ll_split(n, p.tiles, p.ys, p.nper);
  return p;
}

// one operand element: phit_i[f] (* p_i[k] when weighted); f == 0 is the bias feature
__device__ __forceinline__ double ll_operand(const float* __restrict__ Phi, long long ldphi, const float* __restrict__ Pr,
                                             int K, int i, int f, int k, bool weighted) {
  double v = f == 0 ? 1.0 : (double)Phi[(long long)i * ldphi + (f - 1)];
  if (weighted) v *= (double)Pr[(long long)i * K + k];
  return v;
}

// The operand pair of one lane of ll_gram_kernel: rows are flat (f, k) of the DL space for a UU tile and features for a
// D tile; columns are flat (g, l) with Kc classes per feature.  t picks the 16-wide half of the 32-wide tile.
struct LLHeadOperands {
  const float* __restrict__ Phi;
  long long ldphi;
  const float* __restrict__ Pr;
  int K;
  bool uu, softmax;
  int rf[2], rk[2], cf[2], ck[2];
  __device__ __forceinline__ double row(int i, int t) const { return ll_operand(Phi, ldphi, Pr, K, i, rf[t], rk[t], uu); }
  __device__ __forceinline__ double col(int i, int t) const { return ll_operand(Phi, ldphi, Pr, K, i, cf[t], ck[t], softmax); }
};

// The operand pair of one lane of a plain Gram of the augmented rows xt_i = [1, X[i][0..C)]: index 0 is the constant.
struct LLAugOperands {
  const float* __restrict__ X;
  long long ld;
  int r[2], c[2];
  __device__ __forceinline__ double at(int i, int j) const { return j == 0 ? 1.0 : (double)X[(long long)i * ld + (j - 1)]; }
  __device__ __forceinline__ double row(int i, int t) const { return at(i, r[t]); }
  __device__ __forceinline__ double col(int i, int t) const { return at(i, c[t]); }
};

__global__ __launch_bounds__(256) void ll_gram_kernel(const float* __restrict__ Phi, long long ldphi,
                                                      const float* __restrict__ Pr, int n, int K, LLPlan pl,
                                                      double* __restrict__ part) {
  __shared__ double red[3 * LL_TILE];
  const int i16 = threadIdx.x & 15;
  const int tile = blockIdx.x;
  LLHeadOperands op;
  op.Phi = Phi, op.ldphi = ldphi, op.Pr = Pr, op.K = K;
  op.softmax = Pr != nullptr;
  op.uu = tile < pl.Tuu;
  int r0, c0;
  if (op.uu) {
    int tr, tc;
    ll_tri_tile(tile, tr, tc);
    r0 = tr * LL_B;
    c0 = tc * LL_B;
  } else {
    const int t = tile - pl.Tuu;
    r0 = (t / pl.Tc) * LL_B;
    c0 = (t % pl.Tc) * LL_B;
    // only f <= g is ever read: a tile whose smallest f lies above its largest g has nothing to compute
    const int cmax = min(c0 + LL_B - 1, pl.Ft * pl.Kc - 1);
    if (r0 > cmax / pl.Kc) return;
  }
  const int rows = op.uu ? pl.DL : pl.Ft, cols = pl.Ft * pl.Kc;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = min(r0 + 16 * t + i16, rows - 1), c = min(c0 + 16 * t + i16, cols - 1);   // clamped: never read back
    op.rf[t] = op.uu ? r / K : r;
    op.rk[t] = op.uu ? r % K : 0;
    op.cf[t] = c / pl.Kc;
    op.ck[t] = c % pl.Kc;
  }
  const int ib = blockIdx.y * pl.nper;
  ll_gram_tile(op, ib, min(ib + pl.nper, n), red, part + ((long long)blockIdx.y * pl.tiles + tile) * LL_TILE);
}

// G[r][c] += delta_kl D[min(f,g)][(max(f,g), l)] - UU[max(r,c)][min(r,c)], each a sum over the example ranges in order
__global__ __launch_bounds__(256) void ll_assemble_kernel(const double* __restrict__ part, int K, LLPlan pl,
                                                          double* __restrict__ G) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (r >= pl.DL || c >= pl.DL) return;
  const int hi = max(r, c), lo = min(r, c);
  const int f = hi / K, k = hi % K, g = lo / K, l = lo % K;                 // g <= f
  double uu = 0.0, d = 0.0;
  if (pl.Tuu > 0) {
    const int th = hi / LL_B, tl = lo / LL_B;
    const double* src = part + (long long)(th * (th + 1) / 2 + tl) * LL_TILE + (hi % LL_B) * LL_B + lo % LL_B;
    for (int y = 0; y < pl.ys; ++y) uu += src[(long long)y * pl.tiles * LL_TILE];
  }
  if (k == l) {
    const int col = f * pl.Kc + (pl.Kc > 1 ? l : 0);
    const double* src = part + ((long long)pl.Tuu + (long long)(g / LL_B) * pl.Tc + col / LL_B) * LL_TILE +
                        (g % LL_B) * LL_B + col % LL_B;
    for (int y = 0; y < pl.ys; ++y) d += src[(long long)y * pl.tiles * LL_TILE];
  }
  G[(long long)r * pl.DL + c] += d - uu;
}

// out[b][k][l] = sum_g phit_b[g] (sum_f phit_b[f] S[(f,k)][(g,l)]),  l >= k, mirrored.  Block = (b, k); a wave per l; a
// lane per g (every 64th), the inner sum over f serial per lane, the lanes' partial sums met by a fixed butterfly.  The
// diag form runs l = k alone through the same code, so it equals the diagonal of the full form bitwise.
__global__ __launch_bounds__(256) void ll_predict_kernel(const float* __restrict__ Phi, long long ldphi, int F, int K,
                                                         const double* __restrict__ S, double* __restrict__ out, int diag) {
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Ft = F + 1;
  const long long DL = (long long)Ft * K;
  const float* phi = Phi + (long long)b * ldphi;
  const int lend = diag ? k + 1 : K;
  for (int l = k + wave; l < lend; l += 4) {
    double s = 0.0;
    for (int g = lane; g < Ft; g += 64) {
      const double* col = S + (long long)k * DL + (long long)g * K + l;       // S[(f, k)][(g, l)], f = 0
      double t = col[0];
      for (int f = 1; f < Ft; ++f) t = fma((double)phi[f - 1], col[(long long)f * K * DL], t);
      s = fma(g == 0 ? 1.0 : (double)phi[g - 1], t, s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) {
      if (diag) out[(long long)b * K + k] = s;
      else {
        out[((long long)b * K + k) * K + l] = s;
        out[((long long)b * K + l) * K + k] = s;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- Kronecker factors
// A = sum_i phit_i phit_i^T and Bf = sum_i diag(p_i) - p_i p_i^T are both read off plain Grams of augmented rows:
// phit_i = [1, phi_i] is one already, and with pt_i = [1, p_i] the Gram P = sum_i pt_i pt_i^T holds sum_i p_i[k] in
// P[k + 1][0] and sum_i p_i[k] p_i[l] in P[k + 1][l + 1].  One launch computes the lower-triangle tiles of both.
struct LLKronPlan {
  int Ft, Kt;            // edge of the two Grams; Kt = K + 1, or 0 for the Gaussian head (Bf = n I needs no Gram)
  int tilesA, tilesB;    // lower-triangle 32 x 32 tiles of each
  long long tiles;
  int ys, nper;
};

static LLKronPlan ll_kron_plan(int n, int F, int K, bool softmax) {
  LLKronPlan p;
  p.Ft = F + 1;
  p.Kt = softmax ? K + 1 : 0;
  const long long ta = (p.Ft + LL_B - 1) / LL_B, tb = (p.Kt + LL_B - 1) / LL_B;
  p.tilesA = (int)(ta * (ta + 1) / 2);
  p.tilesB = (int)(tb * (tb + 1) / 2);
  p.tiles = (long long)p.tilesA + p.tilesB;
  ll_split(n, p.tiles, p.ys, p.nper);
  return p;
}

__global__ __launch_bounds__(256) void ll_kron_gram_kernel(const float* __restrict__ Phi, long long ldphi,
                                                           const float* __restrict__ Pr, int n, int K, LLKronPlan pl,
                                                           double* __restrict__ part) {
  __shared__ double red[3 * LL_TILE];
  const int i16 = threadIdx.x & 15;
  const int tile = blockIdx.x;
  const bool isA = tile < pl.tilesA;
  int tr, tc;
  ll_tri_tile(isA ? tile : tile - pl.tilesA, tr, tc);
  LLAugOperands op;
  op.X = isA ? Phi : Pr;
  op.ld = isA ? ldphi : (long long)K;
  const int dim = isA ? pl.Ft : pl.Kt;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    op.r[t] = min(tr * LL_B + 16 * t + i16, dim - 1);                                        // clamped: never read back
    op.c[t] = min(tc * LL_B + 16 * t + i16, dim - 1);
  }
  const int ib = blockIdx.y * pl.nper;
  ll_gram_tile(op, ib, min(ib + pl.nper, n), red, part + ((long long)blockIdx.y * pl.tiles + tile) * LL_TILE);
}

// Bf[r][c] += delta_rc P[r + 1][0] - P[max + 1][min + 1], P = the Gram of [1, p]: the lower-triangle tiles starting at
// tile0, each entry a sum over the example ranges in index order
__global__ __launch_bounds__(256) void ll_kron_assemble_kernel(const double* __restrict__ part, long long tiles, int ys,
                                                               int tile0, int dim, double* __restrict__ out) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (r >= dim || c >= dim) return;
  const int hi = max(r, c) + 1, lo = min(r, c) + 1;
  const int th = hi / LL_B, tl = lo / LL_B;
  const double* src = part + ((long long)tile0 + th * (th + 1) / 2 + tl) * LL_TILE + (hi % LL_B) * LL_B + lo % LL_B;
  double v = 0.0, d = 0.0;
  for (int y = 0; y < ys; ++y) v += src[(long long)y * tiles * LL_TILE];
  if (r == c) {
    const double* sd = part + ((long long)tile0 + th * (th + 1) / 2) * LL_TILE + (hi % LL_B) * LL_B;
    for (int y = 0; y < ys; ++y) d += sd[(long long)y * tiles * LL_TILE];
  }
  out[(long long)r * dim + c] += d - v;
}

__global__ void ll_diag_add_kernel(double* __restrict__ M, int dim, double v) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < dim) M[(long long)k * dim + k] += v;
}

// ------------------------------------------------------------------------------------------- Kronecker predictive
// C[b][c] = sum_j a(b, j) Bm[j][c], b < B, j < J, c < N (Bm row-major); a(b, j) = phit_b[j] from Phi, or U[b][j]^2 with
// SQUARED.  A wave per 16 x 16 tile of C on v_mfma_f64_16x16x4_f64: lane l holds a(row l & 15, j0 + (l >> 4)) and
// Bm[j0 + (l >> 4)][col l & 15]; result register r of lane l is (row (l >> 4) + 4 r, col l & 15).
template <bool SQUARED>
__global__ __launch_bounds__(256) void ll_kron_gemm_kernel(const float* __restrict__ Phi, long long ldphi,
                                                           const double* __restrict__ U, int B, int J,
                                                           const double* __restrict__ Bm, int N, double* __restrict__ C) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int ct = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), rt = blockIdx.y;
  if (ct * 16 >= N) return;
  const int b = min(rt * 16 + i16, B - 1), c = min(ct * 16 + i16, N - 1);      // clamped: never written back
  auto a_of = [&](int j) -> double {
    if (SQUARED) {
      const double u = U[(long long)b * J + j];
      return u * u;
    }
    return j == 0 ? 1.0 : (double)Phi[(long long)b * ldphi + (j - 1)];
  };
  // eight k-steps per round, every load issued before the first product; the sum stays in j order
  const ll_f64x4 acc = ll_tile16_mac<8>(a_of, [&](int j) { return Bm[(long long)j * N + c]; }, J, q);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = rt * 16 + q + 4 * r, col = ct * 16 + i16;
    if (row < B && col < N) C[(long long)row * N + col] = acc[r];
  }
}

// One entry out[b][k][m] = sum_l Ub[k][l] Ub[m][l] s_b[l] by one wave: a lane per l (every 64th), the lanes' partial sums
// met by a fixed butterfly.  Both forms below go through it, so the diag form equals the diagonal of the full form bitwise.
__device__ __forceinline__ double ll_kron_cov_entry(const double* __restrict__ uk, const double* __restrict__ um,
                                                    const double* __restrict__ s, int K, int lane) {
  double t = 0.0;
  for (int l = lane; l < K; l += 64) t = fma(uk[l] * um[l], s[l], t);
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) t += __shfl_xor(t, w, 64);
  return t;
}

// full form: block = (b, k), a wave per m >= k, mirrored
__global__ __launch_bounds__(256) void ll_kron_cov_kernel(const double* __restrict__ Ub, const double* __restrict__ S, int K,
                                                          double* __restrict__ out) {
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int m = k + wave; m < K; m += 4) {
    const double t = ll_kron_cov_entry(Ub + (long long)k * K, Ub + (long long)m * K, S + (long long)b * K, K, lane);
    if (lane == 0) {
      out[((long long)b * K + k) * K + m] = t;
      out[((long long)b * K + m) * K + k] = t;
    }
  }
}

// diag form: block = (four test points, k), a wave per test point, m = k
__global__ __launch_bounds__(256) void ll_kron_var_kernel(const double* __restrict__ Ub, const double* __restrict__ S, int B,
                                                          int K, double* __restrict__ out) {
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= B) return;
  const double t = ll_kron_cov_entry(Ub + (long long)k * K, Ub + (long long)k * K, S + (long long)b * K, K, lane);
  if (lane == 0) out[(long long)b * K + k] = t;
}

}  // namespace lip

using namespace lip;

static bool ll_shape_ok(int32_t n, int32_t F, int32_t K) {
  return n > 0 && F > 0 && K > 0 && ((long long)F + 1) * K <= 0x7fffffffll;
}

extern "C" {

int lip_ll_ggn_scratch(int32_t n, int32_t F, int32_t K, int64_t* doubles) {
  if (!doubles || !ll_shape_ok(n, F, K)) { set_error("lip_ll_ggn_scratch: bad argument"); return LIP_ERR_ARG; }
  // the larger of the two heads' plans, so one buffer serves either
  const LLPlan a = ll_plan(n, F, K, true), b = ll_plan(n, F, K, false);
  const long long da = a.tiles * a.ys * LL_TILE, db = b.tiles * b.ys * LL_TILE;
  *doubles = da > db ? da : db;
  return LIP_OK;
}

int lip_ll_ggn(const float* Phi, int64_t ldphi, const float* Pr, int32_t n, int32_t F, int32_t K, double* G,
               double* scratch, int64_t scratch_doubles, void* stream) {
  if (!Phi || !G || !scratch || !ll_shape_ok(n, F, K) || ldphi < F) { set_error("lip_ll_ggn: bad argument"); return LIP_ERR_ARG; }
  const LLPlan pl = ll_plan(n, F, K, Pr != nullptr);
  const long long need = pl.tiles * pl.ys * LL_TILE;
  if (scratch_doubles < need) {
    set_error("lip_ll_ggn: scratch of %lld doubles, %lld needed (lip_ll_ggn_scratch)", (long long)scratch_doubles, need);
    return LIP_ERR_ARG;
  }
  if (pl.tiles > 0x7fffffffll || (pl.DL + 15) / 16 > 65535) { set_error("lip_ll_ggn: (F + 1) K = %d is too large", pl.DL); return LIP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ll_gram_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.ys), dim3(256), 0, st, Phi, (long long)ldphi, Pr,
                     n, K, pl, scratch);
  LIP_CHECK_HIP(hipGetLastError());
  const unsigned gb = (unsigned)((pl.DL + 15) / 16);
  hipLaunchKernelGGL(ll_assemble_kernel, dim3(gb, gb), dim3(256), 0, st, (const double*)scratch, K, pl, G);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_ll_predict(const float* Phi, int64_t ldphi, int32_t B, int32_t F, int32_t K, const double* S, double* out,
                   int32_t diag, void* stream) {
  if (!Phi || !S || !out || !ll_shape_ok(B, F, K) || ldphi < F || K > 65535) { set_error("lip_ll_predict: bad argument"); return LIP_ERR_ARG; }
  hipLaunchKernelGGL(ll_predict_kernel, dim3((unsigned)B, (unsigned)K), dim3(256), 0, (hipStream_t)stream, Phi,
                     (long long)ldphi, F, K, S, out, (int)diag);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_ll_kron_factors_scratch(int32_t n, int32_t F, int32_t K, int64_t* doubles) {
  if (!doubles || !ll_shape_ok(n, F, K)) { set_error("lip_ll_kron_factors_scratch: bad argument"); return LIP_ERR_ARG; }
  // the softmax plan has the tiles of the Gaussian one and more, but the split differs: take the larger
  const LLKronPlan a = ll_kron_plan(n, F, K, true), b = ll_kron_plan(n, F, K, false);
  const long long da = a.tiles * a.ys * LL_TILE, db = b.tiles * b.ys * LL_TILE;
  *doubles = da > db ? da : db;
  return LIP_OK;
}

int lip_ll_kron_factors(const float* Phi, int64_t ldphi, const float* Pr, int32_t n, int32_t F, int32_t K, double* A,
                        double* Bf, double* scratch, int64_t scratch_doubles, void* stream) {
  if (!Phi || !A || !Bf || !scratch || !ll_shape_ok(n, F, K) || ldphi < F) {
    set_error("lip_ll_kron_factors: bad argument");
    return LIP_ERR_ARG;
  }
  const LLKronPlan pl = ll_kron_plan(n, F, K, Pr != nullptr);
  const long long need = pl.tiles * pl.ys * LL_TILE;
  if (scratch_doubles < need) {
    set_error("lip_ll_kron_factors: scratch of %lld doubles, %lld needed (lip_ll_kron_factors_scratch)",
              (long long)scratch_doubles, need);
    return LIP_ERR_ARG;
  }
  const unsigned ga = (unsigned)((pl.Ft + 15) / 16), gb = (unsigned)((K + 15) / 16);
  if (pl.tiles > 0x7fffffffll || ga > 65535 || gb > 65535) {
    set_error("lip_ll_kron_factors: F = %d, K = %d is too large", (int)F, (int)K);
    return LIP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ll_kron_gram_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.ys), dim3(256), 0, st, Phi, (long long)ldphi,
                     Pr, n, K, pl, scratch);
  LIP_CHECK_HIP(hipGetLastError());
  LIP_CHECK_HIP(launch_gram_assemble(scratch, pl.tiles, pl.ys, pl.Ft, A, st));   // A: the Gram of phit, its tiles from tile 0
  if (Pr)
    hipLaunchKernelGGL(ll_kron_assemble_kernel, dim3(gb, gb), dim3(256), 0, st, (const double*)scratch, pl.tiles, pl.ys,
                       pl.tilesA, (int)K, Bf);
  else
    hipLaunchKernelGGL(ll_diag_add_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, Bf, (int)K, (double)n);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_ll_kron_predict_scratch(int32_t B, int32_t F, int32_t K, int64_t* doubles) {
  if (!doubles || !ll_shape_ok(B, F, K)) { set_error("lip_ll_kron_predict_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = (long long)B * ((long long)F + 1 + K);                 // u (B, F + 1) and s (B, K)
  return LIP_OK;
}

int lip_ll_kron_predict(const float* Phi, int64_t ldphi, int32_t B, int32_t F, int32_t K, const double* V, const double* R,
                        const double* Ub, double* out, int32_t diag, double* scratch, int64_t scratch_doubles, void* stream) {
  if (!Phi || !V || !R || !Ub || !out || !scratch || !ll_shape_ok(B, F, K) || ldphi < F || K > 65535 ||
      ((long long)B + 15) / 16 > 65535) {
    set_error("lip_ll_kron_predict: bad argument");
    return LIP_ERR_ARG;
  }
  const int Ft = F + 1;
  const long long need = (long long)B * ((long long)Ft + K);
  if (scratch_doubles < need) {
    set_error("lip_ll_kron_predict: scratch of %lld doubles, %lld needed (lip_ll_kron_predict_scratch)",
              (long long)scratch_doubles, need);
    return LIP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double* u = scratch;
  double* s = scratch + (long long)B * Ft;
  const unsigned gy = (unsigned)((B + 15) / 16);
  // u = phit V, then s = (u o u) R
  hipLaunchKernelGGL(ll_kron_gemm_kernel<false>, dim3((unsigned)((Ft + 63) / 64), gy), dim3(256), 0, st, Phi, (long long)ldphi,
                     (const double*)nullptr, (int)B, Ft, V, Ft, u);
  LIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ll_kron_gemm_kernel<true>, dim3((unsigned)((K + 63) / 64), gy), dim3(256), 0, st, (const float*)nullptr,
                     0ll, (const double*)u, (int)B, Ft, R, (int)K, s);
  LIP_CHECK_HIP(hipGetLastError());
  if (diag)
    hipLaunchKernelGGL(ll_kron_var_kernel, dim3((unsigned)((B + 3) / 4), (unsigned)K), dim3(256), 0, st, Ub, (const double*)s,
                       (int)B, (int)K, out);
  else
    hipLaunchKernelGGL(ll_kron_cov_kernel, dim3((unsigned)B, (unsigned)K), dim3(256), 0, st, Ub, (const double*)s, (int)K, out);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

}  // extern "C"
