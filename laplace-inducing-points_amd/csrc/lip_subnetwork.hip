// Subnetwork Laplace: the dense GGN block over an arbitrary index set idx (S entries of the flat parameter vector) from
// the per-example rows lip_vjp_rows writes (lip_sub_gram), and the matching test-time quadratic form (lip_sub_predict).
// Everything after the gather in float64.
//
//   G[a][c]        += sum_{r < R} W[r][idx[a]] W[r][idx[c]]
//   out[b][k][l]    = sum_{a,c} Jr[k B + b][idx[a]] Sigma[a][c] Jr[l B + b][idx[c]]
//
// Both start with sub_gather_kernel: the S scattered 4-byte columns of every row are read ONCE and written as a compact
// (rows, S) float32 panel in the caller's scratch, coalesced.  Every later stage reads the panel: the 16 lanes of a
// k-step of the Gram read 64 contiguous bytes.  Gathering inside the tile loop instead would re-read each scattered
// column once per tile row of G (S / 32 times).  The gather clamps every index into [0, D): a bad index gives a wrong
// number, never an out-of-bounds read.
//
// Gram: ll_gram_tile (lip_gramtile.h, the tile loop of lip_ll_ggn) over the lower triangle of 32 x 32 tiles x ranges of
// rows; every block writes its partial tile to scratch and sub_assemble_kernel adds the ranges in index order, both
// (a, c) and (c, a) from the same partial sums: no atomics, bitwise reproducible, exactly symmetric.
//
// Predict: T = panel Sigma ((K B, S) float64, in scratch; a wave per 32 x 32 tile on v_mfma_f64_16x16x4_f64), then per
// test point the K x K product T_b panel_b^T on the same instruction, tiles with k-tile <= l-tile, entries k <= l written
// and mirrored.  The diag form runs the diagonal tiles of the same kernel and keeps k == l, so it equals the diagonal of
// the full form bitwise.  The panel rows are stored point-major (b K + k) so that a point's K rows are adjacent.
#include "lip_internal.h"
#include "lip_gramtile.h"

namespace lip {

// panel[(row map)(r)][a] = W[r][clamp(idx[a])];  KB == 0: rows in place;  KB = (K, B): source row k B + b -> b K + k
__global__ __launch_bounds__(256) void sub_gather_kernel(const float* __restrict__ W, long long ldw, long long D,
                                                         long long R, const long long* __restrict__ idx, int S, int K,
                                                         int B, float* __restrict__ panel) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= S) return;
  long long j = idx[a];
  j = j < 0 ? 0 : (j >= D ? D - 1 : j);
  for (long long r = blockIdx.y; r < R; r += gridDim.y) {
    const long long dst = K > 0 ? (r % B) * K + r / B : r;
    panel[dst * S + a] = W[r * ldw + j];
  }
}

// The operand pair of one lane of a plain Gram of the panel's columns
struct SubPanelOperands {
  const float* __restrict__ P;
  long long ld;
  int r[2], c[2];
  __device__ __forceinline__ double row(int i, int t) const { return (double)P[(long long)i * ld + r[t]]; }
  __device__ __forceinline__ double col(int i, int t) const { return (double)P[(long long)i * ld + c[t]]; }
};

__global__ __launch_bounds__(256) void sub_gram_kernel(const float* __restrict__ panel, int R, int S, TriPlan pl,
                                                       double* __restrict__ part) {
  __shared__ double red[3 * LL_TILE];
  const int i16 = threadIdx.x & 15;
  const int tile = blockIdx.x;
  int tr, tc;
  ll_tri_tile(tile, tr, tc);
  SubPanelOperands op;
  op.P = panel, op.ld = S;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    op.r[t] = min(tr * LL_B + 16 * t + i16, S - 1);                                          // clamped: never read back
    op.c[t] = min(tc * LL_B + 16 * t + i16, S - 1);
  }
  const int ib = blockIdx.y * pl.nper;
  ll_gram_tile(op, ib, min(ib + pl.nper, R), red, part + ((long long)blockIdx.y * pl.tiles + tile) * LL_TILE);
}

// G[a][c] += P[max(a, c)][min(a, c)], P the lower-triangle tiles, each entry a sum over the row ranges in index order
__global__ __launch_bounds__(256) void sub_assemble_kernel(const double* __restrict__ part, long long tiles, int ys, int S,
                                                           double* __restrict__ G) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (r >= S || c >= S) return;
  const int hi = max(r, c), lo = min(r, c);
  const int th = hi / LL_B, tl = lo / LL_B;
  const double* src = part + ((long long)th * (th + 1) / 2 + tl) * LL_TILE + (hi % LL_B) * LL_B + lo % LL_B;
  double v = 0.0;
  for (int y = 0; y < ys; ++y) v += src[(long long)y * tiles * LL_TILE];
  G[(long long)r * S + c] += v;
}

// out[b][k][l] = sum_a T[b K + k][a] panel[b K + l][a].  Block = (test point b, four tile pairs); a wave per 16 x 16 tile
// (kt, lt), kt <= lt (diag: kt == lt), of the K x K product.  Entries k <= l are written and mirrored; diag keeps k == l.
__global__ __launch_bounds__(256) void sub_quad_kernel(const double* __restrict__ T, const float* __restrict__ panel, int K,
                                                       int S, double* __restrict__ out, int diag) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4;
  const int b = blockIdx.x;
  const int pair = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int KT = (K + 15) / 16;
  int kt, lt;
  if (diag) {
    if (pair >= KT) return;
    kt = lt = pair;
  } else {
    if (pair >= KT * (KT + 1) / 2) return;
    ll_tri_tile(pair, lt, kt);                                                               // lt >= kt
  }
  const double* ta = T + ((long long)b * K + min(kt * 16 + i16, K - 1)) * S;                 // clamped: never written back
  const float* pb = panel + ((long long)b * K + min(lt * 16 + i16, K - 1)) * S;
  const ll_f64x4 acc = ll_tile16_mac<4>([&](int a) { return ta[a]; }, [&](int a) { return (double)pb[a]; }, S, q);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = kt * 16 + q + 4 * r, l = lt * 16 + i16;
    if (k >= K || l >= K) continue;
    if (diag) {
      if (k == l) out[(long long)b * K + k] = acc[r];
    } else if (k <= l) {
      out[((long long)b * K + k) * K + l] = acc[r];
      out[((long long)b * K + l) * K + k] = acc[r];
    }
  }
}

static long long sub_panel_doubles(long long rows, int S) { return (rows * S + 1) / 2; }

// The Gram stages on their own (declared in lip_gramtile.h): lip_kfac.hip and the KRON sweep of lip_engine.hip run them too
hipError_t launch_gram_assemble(const double* part, long long tiles, int ys, int S, double* G, hipStream_t st) {
  const unsigned gb = (unsigned)((S + 15) / 16);
  hipLaunchKernelGGL(sub_assemble_kernel, dim3(gb, gb), dim3(256), 0, st, part, tiles, ys, S, G);
  return hipGetLastError();
}

bool panel_gram_fits(int R, int S) {
  if (R <= 0 || S <= 0) return false;
  return tri_plan(R, S).tiles <= 0x7fffffffll && (S + 15) / 16 <= 65535;
}

long long panel_gram_scratch(int R, int S) {
  const TriPlan pl = tri_plan(R, S);
  return pl.tiles * pl.ys * LL_TILE;
}

hipError_t launch_panel_gram(const float* panel, int R, int S, double* G, double* part, hipStream_t st) {
  const TriPlan pl = tri_plan(R, S);
  hipLaunchKernelGGL(sub_gram_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.ys), dim3(256), 0, st, panel, R, S, pl, part);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_gram_assemble(part, pl.tiles, pl.ys, S, G, st);
}

static void sub_gather(const float* W, long long ldw, long long D, long long R, const int64_t* idx, int S, int K, int B,
                       float* panel, hipStream_t st) {
  const unsigned gy = (unsigned)(R < 65535 ? R : 65535);
  hipLaunchKernelGGL(sub_gather_kernel, dim3((unsigned)((S + 255) / 256), gy), dim3(256), 0, st, W, ldw, D, R,
                     (const long long*)idx, S, K, B, panel);
}

// One launch over all P R rows when the probes are adjacent (one probe, or the per-probe stride is the row block), else
// one launch per probe: the rule of the KRON sweep's Grams
hipError_t launch_rows_project(const float* G, long long ldg, long long pstride, int P, int R, int N, const double* Ub,
                               float* GU, hipStream_t st) {
  const bool packed = P == 1 || pstride == (long long)R * ldg;
  const long long rows = packed ? (long long)P * R : R;
  const dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((N + 127) / 128));
  for (int p = 0; p < (packed ? 1 : P); ++p) {
    hipLaunchKernelGGL((ll_project_kernel<F32Rows, float>), grid, dim3(256), 0, st, F32Rows{G + p * pstride, ldg}, rows, N, Ub, N,
                       GU + (long long)p * R * N);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace lip

using namespace lip;

static bool sub_rows_ok(int32_t B, int32_t K, int32_t S) {
  return B > 0 && K > 0 && S > 0 && (long long)B * K <= 0x7fffffffll;
}

extern "C" {

int lip_sub_gather(const float* W, int64_t ldw, int64_t D, int32_t R, const int64_t* idx, int32_t S, float* panel,
                   void* stream) {
  if (!W || !idx || !panel || R <= 0 || S <= 0 || D <= 0 || ldw < D) { set_error("lip_sub_gather: bad argument"); return LIP_ERR_ARG; }
  sub_gather(W, (long long)ldw, (long long)D, R, idx, S, 0, 0, panel, (hipStream_t)stream);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_rows_project(const float* G, int64_t ldg, int64_t pstride, int32_t P, int32_t R, int32_t N, const double* Ub, float* GU,
                     void* stream) {
  if (!G || !Ub || !GU || P <= 0 || R <= 0 || N <= 0 || ldg < N || (P > 1 && pstride < (long long)(R - 1) * ldg + N)) {
    set_error("lip_rows_project: bad argument");
    return LIP_ERR_ARG;
  }
  if ((long long)P * R * N >= (1ll << 31) || (long long)N * N >= (1ll << 31) || !ll_project_fits((long long)P * R, N)) {
    set_error("lip_rows_project: a tensor of 2^31 or more elements; pass fewer rows per call");
    return LIP_ERR_ARG;
  }
  LIP_CHECK_HIP(launch_rows_project(G, (long long)ldg, (long long)pstride, P, R, N, Ub, GU, (hipStream_t)stream));
  return LIP_OK;
}

int lip_sub_gram_scratch(int32_t R, int32_t S, int64_t* doubles) {
  if (!doubles || R <= 0 || S <= 0) { set_error("lip_sub_gram_scratch: bad argument"); return LIP_ERR_ARG; }
  const TriPlan pl = tri_plan(R, S);
  *doubles = sub_panel_doubles(R, S) + pl.tiles * pl.ys * LL_TILE;
  return LIP_OK;
}

int lip_sub_gram(const float* W, int64_t ldw, int64_t D, int32_t R, const int64_t* idx, int32_t S, double* G,
                 double* scratch, int64_t scratch_doubles, void* stream) {
  if (!W || !idx || !G || !scratch || R <= 0 || S <= 0 || D <= 0 || ldw < D) {
    set_error("lip_sub_gram: bad argument");
    return LIP_ERR_ARG;
  }
  const TriPlan pl = tri_plan(R, S);
  const long long pd = sub_panel_doubles(R, S), need = pd + pl.tiles * pl.ys * LL_TILE;
  if (scratch_doubles < need) {
    set_error("lip_sub_gram: scratch of %lld doubles, %lld needed (lip_sub_gram_scratch)", (long long)scratch_doubles, need);
    return LIP_ERR_ARG;
  }
  if (pl.tiles > 0x7fffffffll || (S + 15) / 16 > 65535) { set_error("lip_sub_gram: S = %d is too large", (int)S); return LIP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  float* panel = (float*)scratch;
  double* part = scratch + pd;
  sub_gather(W, (long long)ldw, (long long)D, R, idx, S, 0, 0, panel, st);
  LIP_CHECK_HIP(hipGetLastError());
  LIP_CHECK_HIP(launch_panel_gram(panel, (int)R, (int)S, G, part, st));
  return LIP_OK;
}

int lip_sub_predict_scratch(int32_t B, int32_t K, int32_t S, int64_t* doubles) {
  if (!doubles || !sub_rows_ok(B, K, S)) { set_error("lip_sub_predict_scratch: bad argument"); return LIP_ERR_ARG; }
  const long long rows = (long long)B * K;
  *doubles = sub_panel_doubles(rows, S) + rows * S;                  // the float32 panel and T (K B, S)
  return LIP_OK;
}

int lip_sub_predict(const float* Jr, int64_t ldj, int64_t D, int32_t B, int32_t K, const int64_t* idx, int32_t S,
                    const double* Sigma, double* out, int32_t diag, double* scratch, int64_t scratch_doubles, void* stream) {
  if (!Jr || !idx || !Sigma || !out || !scratch || !sub_rows_ok(B, K, S) || D <= 0 || ldj < D) {
    set_error("lip_sub_predict: bad argument");
    return LIP_ERR_ARG;
  }
  const long long rows = (long long)B * K, pd = sub_panel_doubles(rows, S), need = pd + rows * S;
  if (scratch_doubles < need) {
    set_error("lip_sub_predict: scratch of %lld doubles, %lld needed (lip_sub_predict_scratch)", (long long)scratch_doubles,
              need);
    return LIP_ERR_ARG;
  }
  const long long KT = ((long long)K + 15) / 16, pairs = diag ? KT : KT * (KT + 1) / 2;
  if ((rows + 31) / 32 > 65535 || (pairs + 3) / 4 > 65535) {
    set_error("lip_sub_predict: B = %d, K = %d is too large", (int)B, (int)K);
    return LIP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  float* panel = (float*)scratch;
  double* T = scratch + pd;
  sub_gather(Jr, (long long)ldj, (long long)D, rows, idx, S, K, B, panel, st);
  LIP_CHECK_HIP(hipGetLastError());
  // T (rows, S) = panel Sigma
  hipLaunchKernelGGL((ll_project_kernel<F32Rows, double>), dim3((unsigned)((rows + 31) / 32), (unsigned)((S + 127) / 128)), dim3(256),
                     0, st, F32Rows{panel, (long long)S}, rows, (int)S, Sigma, (int)S, T);
  LIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sub_quad_kernel, dim3((unsigned)B, (unsigned)((pairs + 3) / 4)), dim3(256), 0, st, (const double*)T,
                     (const float*)panel, (int)K, (int)S, out, (int)diag);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

}  // extern "C"
