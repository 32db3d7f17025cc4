// MAP training: the HBM-bound streaming kernels a training step adds to the engine's primal and backward passes
// (include/lip.h, "MAP training"; replaces src/train_map.py's jitted _map_step around the convolutions).
//
//   batch statistics      z (R, N) -> mean, biased var, rsqrt(var + eps), s = gamma rstd, running averages
//   BN train backward     g' = g - (dbeta + xhat dgamma) / R
//   transposed kernels    Wt[t][co][ci] = W[t][ci][co] s[co]
//   loss head             logits, labels -> (p - e_y) / n and the summed NLL;  Gaussian NLL for the regressor
//   Adam with the prior   theta, m, v updated in one pass, 0.5 sum a theta^2 returned
//
// No atomics anywhere: every sum is taken in a fixed order (per-thread strided sums, the halving tree of a 64-lane wave,
// waves / row groups in index order through LDS, partials in index order), so equal inputs give equal bits.
#include "lip_internal.h"

namespace lip {
namespace {

constexpr int TRAIN_STATS_ROWS = 256;    // rows of z per partial sum of the statistics kernel
constexpr int ADAM_MAX_BLOCKS = 2048;    // 8 blocks per CU on the 256 CUs of an MI355X
constexpr int LOSS_THREADS = 1024;       // the loss head is ONE block: its sums need no second launch

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                              // lane 0 holds the sum
}

// sum of one double per thread over a block of NT threads (NT a multiple of 64): the wave tree, then the waves in index
// order; valid in thread 0
template <int NT>
__device__ __forceinline__ double block_sum_f64(double v, double* lds /*[NT / 64]*/) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// ---- batch statistics ------------------------------------------------------------------------------------------------
// Shifted float64 sums: with sh[c] = z[0][c], block (x, y) sums d = z[r][c] - sh[c] and d^2 over the rows of chunk y for
// the channels of column tile x, and stores the pair.  d is of the size of the channel's spread, not of its mean, so
// sum d^2 - (sum d)^2 / R does not cancel (the float32 E[z^2] - E[z]^2 loses every digit at mean 1e3, spread 1e-1).
// A thread owns VEC adjacent channels (one 16-byte load when VEC = 4) and every (256 / CW)-th row of the chunk.
template <int VEC>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ z, int R, int N, int CG, int CW,
                                                               double2* __restrict__ partial) {
  __shared__ double red[2 * VEC * 256];
  const int cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW, RP = 256 / CW;
  const int cg = blockIdx.x * CW + cl;
  const int r0 = blockIdx.y * TRAIN_STATS_ROWS;
  const int r1 = r0 + TRAIN_STATS_ROWS < R ? r0 + TRAIN_STATS_ROWS : R;
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { s1[k] = 0.0; s2[k] = 0.0; }
  if (cg < CG) {
    const int c0 = cg * VEC;
    if (VEC == 4) {
      const float4 sh = *reinterpret_cast<const float4*>(z + c0);
      const double h0 = sh.x, h1 = sh.y, h2 = sh.z, h3 = sh.w;
#pragma unroll 4
      for (int r = r0 + rl; r < r1; r += RP) {
        const float4 v = *reinterpret_cast<const float4*>(z + (long long)r * N + c0);
        const double d0 = (double)v.x - h0, d1 = (double)v.y - h1, d2 = (double)v.z - h2, d3 = (double)v.w - h3;
        s1[0] += d0; s2[0] = fma(d0, d0, s2[0]);
        s1[1 % VEC] += d1; s2[1 % VEC] = fma(d1, d1, s2[1 % VEC]);
        s1[2 % VEC] += d2; s2[2 % VEC] = fma(d2, d2, s2[2 % VEC]);
        s1[3 % VEC] += d3; s2[3 % VEC] = fma(d3, d3, s2[3 % VEC]);
      }
    } else {
      const double h = z[c0];
#pragma unroll 4
      for (int r = r0 + rl; r < r1; r += RP) {
        const double d = (double)z[(long long)r * N + c0] - h;
        s1[0] += d; s2[0] = fma(d, d, s2[0]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    red[(2 * k) * 256 + threadIdx.x] = s1[k];
    red[(2 * k + 1) * 256 + threadIdx.x] = s2[k];
  }
  __syncthreads();
  if (rl == 0 && cg < CG) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      double a = 0.0, b = 0.0;
      for (int j = 0; j < RP; ++j) { a += red[(2 * k) * 256 + j * CW + cl]; b += red[(2 * k + 1) * 256 + j * CW + cl]; }
      partial[(long long)blockIdx.y * N + cg * VEC + k] = make_double2(a, b);
    }
  }
}

struct BnFoldP {
  const float* z; const double2* partial; int R, N, chunks;
  const float* bias; const float* gamma; float eps, momentum;
  float* mean; float* var; float* rstd; float* s; float* run_mean; float* run_var;
};

// one wave per channel: the chunk pairs in lane-strided order, the wave tree, then the statistics in float64, each
// rounded once on its store.  The conv bias shifts the mean only.
__global__ __launch_bounds__(256) void bn_stats_fold_kernel(const BnFoldP p) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= p.N) return;
  double a = 0.0, b = 0.0;
  for (int j = lane; j < p.chunks; j += 64) {
    const double2 q = p.partial[(long long)j * p.N + c];
    a += q.x; b += q.y;
  }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (lane != 0) return;
  const double R = (double)p.R;
  double mean = (double)p.z[c] + a / R;
  double m2 = b - a * a / R;
  if (m2 < 0.0) m2 = 0.0;
  const double var = m2 / R;
  if (p.bias) mean += (double)p.bias[c];
  const float rstd = (float)(1.0 / sqrt(var + (double)p.eps));
  if (p.mean) p.mean[c] = (float)mean;
  if (p.var) p.var[c] = (float)var;
  if (p.rstd) p.rstd[c] = rstd;
  if (p.s) p.s[c] = (p.gamma ? p.gamma[c] : 1.f) * rstd;       // float32, as engine.build_consts forms it
  const double mom = (double)p.momentum;
  if (p.run_mean) p.run_mean[c] = (float)(mom * (double)p.run_mean[c] + (1.0 - mom) * mean);
  if (p.run_var) p.run_var[c] = (float)(mom * (double)p.run_var[c] + (1.0 - mom) * var);
}

inline int pow2_at_least(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// ---- BN train backward: g' = g - (dbeta + xhat dgamma) / R, per probe ---------------------------------------------------
struct BnBwdP {
  const float* g; long long g_ps;
  const float* xhat;
  const float* dbeta; const float* dgamma; long long d_ps;
  float* out; long long out_ps;
  long long count; int N; float inv;
};

template <int VEC>
__global__ __launch_bounds__(256) void bn_train_bwd_kernel(const BnBwdP p) {
  const float* g = p.g + (long long)blockIdx.y * p.g_ps;
  float* out = p.out + (long long)blockIdx.y * p.out_ps;
  const float* db = p.dbeta + (long long)blockIdx.y * p.d_ps;
  const float* dg = p.dgamma + (long long)blockIdx.y * p.d_ps;
  const long long step = (long long)gridDim.x * 256;
  if (VEC == 4) {
    const long long quads = p.count >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += step) {
      const int c = (int)((unsigned)(q * 4) % (unsigned)p.N);      // count < 2^31 (checked by the callers)
      const float4 gv = *reinterpret_cast<const float4*>(g + 4 * q);
      const float4 xv = *reinterpret_cast<const float4*>(p.xhat + 4 * q);
      float4 o;
      o.x = gv.x - (db[c] + xv.x * dg[c]) * p.inv;
      o.y = gv.y - (db[c + 1] + xv.y * dg[c + 1]) * p.inv;
      o.z = gv.z - (db[c + 2] + xv.z * dg[c + 2]) * p.inv;
      o.w = gv.w - (db[c + 3] + xv.w * dg[c + 3]) * p.inv;
      *reinterpret_cast<float4*>(out + 4 * q) = o;
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.count; i += step) {
      const int c = (int)((unsigned)i % (unsigned)p.N);
      out[i] = g[i] - (db[c] + p.xhat[i] * dg[c]) * p.inv;
    }
  }
}

// ---- transposed, BN-scaled kernels: Wt[t][co][ci] = W[t][ci][co] s[co], one 32 x 32 tile per block through LDS ------------
__global__ __launch_bounds__(256) void wt_refresh_kernel(const float* __restrict__ W, const float* __restrict__ s,
                                                         float* __restrict__ Wt, int cin, int cout) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long long base = (long long)blockIdx.z * cin * cout;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    if (ci < cin && co < cout) tile[j][tx] = W[base + (long long)ci * cout + co] * (s ? s[co] : 1.f);
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int co = co0 + j, ci = ci0 + tx;
    if (ci < cin && co < cout) Wt[base + (long long)co * cin + ci] = tile[tx][j];
  }
}

// ---- loss head ---------------------------------------------------------------------------------------------------------
// classifier: one wave per example, the examples of a wave in index order; u = (softmax(f) - e_y) / n through a
// log-sum-exp about the row maximum (every exponent <= 0: finite for any finite logits), the example's NLL
// lse - f[y] in float64.  A label outside [0, K) gives a NaN loss and the row softmax(f) / n.
__global__ __launch_bounds__(LOSS_THREADS) void loss_head_classifier_kernel(const float* __restrict__ logits,
                                                                            const long long* __restrict__ labels, int n, int K,
                                                                            float* __restrict__ U, double* __restrict__ out) {
  __shared__ double lds[LOSS_THREADS / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float invn = 1.f / (float)n;
  double acc = 0.0;
  for (int i = wave; i < n; i += LOSS_THREADS / 64) {
    const float* f = logits + (long long)i * K;
    float* u = U + (long long)i * K;
    float mx = -3.0e38f;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, f[k]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k = lane; k < K; k += 64) sum += expf(f[k] - mx);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    const long long y = labels[i];
    for (int k = lane; k < K; k += 64) u[k] = (expf(f[k] - mx) * inv - (k == y ? 1.f : 0.f)) * invn;
    if (lane == 0) {
      const double fy = (y >= 0 && y < K) ? (double)f[y] : __longlong_as_double(0x7ff8000000000000ll);
      acc += (double)mx + log((double)sum) - fy;
    }
  }
  if (lane == 0) lds[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < LOSS_THREADS / 64; ++w) s += lds[w];
    out[0] = s;
    out[1] = 0.0;
  }
}

// regressor: u = (f - y) exp(-logvar) / count over the count = n K outputs; out[0] = the summed Gaussian NLL
// 0.5 sum (log(2 pi) + logvar + (f - y)^2 exp(-logvar)), out[1] = d(mean NLL)/d logvar = 0.5 (1 - mean (f - y)^2 exp(-logvar))
__global__ __launch_bounds__(LOSS_THREADS) void loss_head_regressor_kernel(const float* __restrict__ f, const float* __restrict__ y,
                                                                           long long count, float logvar, float* __restrict__ U,
                                                                           double* __restrict__ out) {
  __shared__ double lds[LOSS_THREADS / 64];
  const float prec = expf(-logvar), w = prec / (float)count;
  double se = 0.0;
  for (long long i = threadIdx.x; i < count; i += LOSS_THREADS) {
    const float d = f[i] - y[i];
    U[i] = d * w;
    se = fma((double)d, (double)d, se);
  }
  se = block_sum_f64<LOSS_THREADS>(se, lds);
  if (threadIdx.x == 0) {
    const double lv = (double)logvar, pr = exp(-lv), cnt = (double)count;
    out[0] = 0.5 * (cnt * (1.8378770664093453 + lv) + se * pr);
    out[1] = 0.5 * (1.0 - se * pr / cnt);
  }
}

// ---- Adam with the prior folded in ---------------------------------------------------------------------------------------
struct AdamP {
  float* theta; float* m; float* v; const float* g; const float* a; float a_s;
  float lr, b1, b2, eps, inv_bc1, inv_bc2;
  long long D;
};

__device__ __forceinline__ void adam_one(const AdamP& p, float& th, float& m, float& v, float g, float a, double& reg) {
  reg = fma(0.5 * (double)a * (double)th, (double)th, reg);
  const float gt = g + a * th;
  m = p.b1 * m + (1.f - p.b1) * gt;
  v = p.b2 * v + (1.f - p.b2) * gt * gt;
  th -= p.lr * (m * p.inv_bc1) / (sqrtf(v * p.inv_bc2) + p.eps);
}

// float4 body (the five vectors are 16-byte aligned allocations), scalar tail by block 0; one partial per block
template <bool VECA>
__global__ __launch_bounds__(256) void adam_kernel(const AdamP p, double* __restrict__ partial) {
  __shared__ double lds[4];
  const long long quads = p.D >> 2, step = (long long)gridDim.x * 256;
  double reg = 0.0;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += step) {
    float4 th = *reinterpret_cast<float4*>(p.theta + 4 * q);
    float4 m = *reinterpret_cast<float4*>(p.m + 4 * q);
    float4 v = *reinterpret_cast<float4*>(p.v + 4 * q);
    const float4 g = *reinterpret_cast<const float4*>(p.g + 4 * q);
    float4 a = make_float4(p.a_s, p.a_s, p.a_s, p.a_s);
    if (VECA) a = *reinterpret_cast<const float4*>(p.a + 4 * q);
    adam_one(p, th.x, m.x, v.x, g.x, a.x, reg);
    adam_one(p, th.y, m.y, v.y, g.y, a.y, reg);
    adam_one(p, th.z, m.z, v.z, g.z, a.z, reg);
    adam_one(p, th.w, m.w, v.w, g.w, a.w, reg);
    *reinterpret_cast<float4*>(p.theta + 4 * q) = th;
    *reinterpret_cast<float4*>(p.m + 4 * q) = m;
    *reinterpret_cast<float4*>(p.v + 4 * q) = v;
  }
  if (blockIdx.x == 0) {
    const long long i = 4 * quads + threadIdx.x;
    if (i < p.D) {
      float th = p.theta[i], m = p.m[i], v = p.v[i];
      adam_one(p, th, m, v, p.g[i], VECA ? p.a[i] : p.a_s, reg);
      p.theta[i] = th; p.m[i] = m; p.v[i] = v;
    }
  }
  reg = block_sum_f64<256>(reg, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = reg;
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) s += partial[i];
  s = block_sum_f64<256>(s, lds);
  if (threadIdx.x == 0) out[0] = s;
}

inline int adam_blocks(long long D) {
  const long long b = (D / 4 + 255) / 256;
  return (int)(b < 1 ? 1 : b > ADAM_MAX_BLOCKS ? ADAM_MAX_BLOCKS : b);
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------------
long long bn_stats_scratch(int R, int N) {
  return 2ll * ((R + TRAIN_STATS_ROWS - 1) / TRAIN_STATS_ROWS) * N;
}

hipError_t launch_bn_stats(const BnStatsP& p, hipStream_t st) {
  const int chunks = (p.R + TRAIN_STATS_ROWS - 1) / TRAIN_STATS_ROWS;
  double2* partial = reinterpret_cast<double2*>(p.scratch);
  const bool vec = (p.N & 3) == 0 && aligned16(p.z);
  const int CG = vec ? p.N / 4 : p.N;
  const int CW = pow2_at_least(CG) < 256 ? pow2_at_least(CG) : 256;
  const dim3 grid((unsigned)((CG + CW - 1) / CW), (unsigned)chunks);
  if (vec) { hipLaunchKernelGGL(bn_stats_partial_kernel<4>, grid, dim3(256), 0, st, p.z, p.R, p.N, CG, CW, partial); }
  else { hipLaunchKernelGGL(bn_stats_partial_kernel<1>, grid, dim3(256), 0, st, p.z, p.R, p.N, CG, CW, partial); }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  BnFoldP f;
  f.z = p.z; f.partial = partial; f.R = p.R; f.N = p.N; f.chunks = chunks;
  f.bias = p.bias; f.gamma = p.gamma; f.eps = p.eps; f.momentum = p.momentum;
  f.mean = p.mean; f.var = p.var; f.rstd = p.rstd; f.s = p.s; f.run_mean = p.run_mean; f.run_var = p.run_var;
  hipLaunchKernelGGL(bn_stats_fold_kernel, dim3((unsigned)((p.N + 3) / 4)), dim3(256), 0, st, f);
  return hipGetLastError();
}

hipError_t launch_bn_train_bwd(const BnTrainBwdP& q, int P, hipStream_t st) {
  BnBwdP p;
  p.g = q.g; p.g_ps = q.g_ps; p.xhat = q.xhat; p.dbeta = q.dbeta; p.dgamma = q.dgamma; p.d_ps = q.d_ps;
  p.out = q.out; p.out_ps = q.out_ps; p.N = q.N; p.count = (long long)q.R * q.N; p.inv = 1.f / (float)q.R;
  const bool vec = (q.N & 3) == 0 && aligned16(q.g, q.xhat, q.out) && ((q.g_ps | q.out_ps) & 3) == 0;
  const long long items = vec ? p.count / 4 : p.count;
  const long long blocks = (items + 255) / 256;
  const dim3 grid((unsigned)(blocks < 2048 ? (blocks < 1 ? 1 : blocks) : 2048), (unsigned)P);
  if (vec) { hipLaunchKernelGGL(bn_train_bwd_kernel<4>, grid, dim3(256), 0, st, p); }
  else { hipLaunchKernelGGL(bn_train_bwd_kernel<1>, grid, dim3(256), 0, st, p); }
  return hipGetLastError();
}

hipError_t launch_wt_refresh(const float* W, const float* s, float* Wt, int taps, int cin, int cout, hipStream_t st) {
  hipLaunchKernelGGL(wt_refresh_kernel, dim3((unsigned)((cin + 31) / 32), (unsigned)((cout + 31) / 32), (unsigned)taps), dim3(256), 0,
                     st, W, s, Wt, cin, cout);
  return hipGetLastError();
}

}  // namespace lip

using namespace lip;

extern "C" {

int lip_train_bn_stats_scratch(int32_t R, int32_t N, int64_t* doubles) {
  if (R <= 0 || N <= 0 || !doubles) { set_error("lip_train_bn_stats_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = bn_stats_scratch(R, N);
  return LIP_OK;
}

int lip_train_bn_stats(const float* z, int32_t R, int32_t N, const float* bias, const float* gamma, float eps, float momentum,
                       float* mean, float* var, float* rstd, float* s, float* run_mean, float* run_var, double* scratch,
                       int64_t scratch_doubles, void* stream) {
  if (!z || R <= 0 || N <= 0 || !scratch || scratch_doubles < bn_stats_scratch(R, N) || (long long)R * N >= (1ll << 31) ||
      !(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f) || (((uintptr_t)scratch) & 15)) {
    set_error("lip_train_bn_stats: bad argument");
    return LIP_ERR_ARG;
  }
  BnStatsP p;
  p.z = z; p.R = R; p.N = N; p.bias = bias; p.gamma = gamma; p.eps = eps; p.momentum = momentum;
  p.mean = mean; p.var = var; p.rstd = rstd; p.s = s; p.run_mean = run_mean; p.run_var = run_var; p.scratch = scratch;
  LIP_CHECK_HIP(launch_bn_stats(p, (hipStream_t)stream));
  return LIP_OK;
}

int lip_train_bn_backward(const float* g, const float* xhat, const float* dbeta, const float* dgamma, int32_t R, int32_t N,
                          float* out, void* stream) {
  if (!g || !xhat || !dbeta || !dgamma || !out || R <= 0 || N <= 0 || (long long)R * N >= (1ll << 31) || out == g) {
    set_error("lip_train_bn_backward: bad argument");
    return LIP_ERR_ARG;
  }
  BnTrainBwdP p;
  p.g = g; p.g_ps = 0; p.xhat = xhat; p.dbeta = dbeta; p.dgamma = dgamma; p.d_ps = 0; p.out = out; p.out_ps = 0; p.R = R; p.N = N;
  LIP_CHECK_HIP(launch_bn_train_bwd(p, 1, (hipStream_t)stream));
  return LIP_OK;
}

int lip_train_wt_refresh(const float* W, const float* s, float* Wt, int32_t taps, int32_t cin, int32_t cout, void* stream) {
  if (!W || !Wt || W == Wt || taps <= 0 || taps > 65535 || cin <= 0 || cout <= 0 || (cout + 31) / 32 > 65535) {
    set_error("lip_train_wt_refresh: bad argument");
    return LIP_ERR_ARG;
  }
  LIP_CHECK_HIP(launch_wt_refresh(W, s, Wt, taps, cin, cout, (hipStream_t)stream));
  return LIP_OK;
}

int lip_train_loss_head(const float* outputs, const void* targets, int32_t n, int32_t K, int32_t classifier, float logvar, float* U,
                        double* out, void* stream) {
  if (!outputs || !targets || !U || !out || n <= 0 || K <= 0 || (long long)n * K >= (1ll << 31)) {
    set_error("lip_train_loss_head: bad argument");
    return LIP_ERR_ARG;
  }
  if (classifier) {
    hipLaunchKernelGGL(loss_head_classifier_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, outputs,
                       (const long long*)targets, n, K, U, out);
  } else {
    hipLaunchKernelGGL(loss_head_regressor_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, outputs,
                       (const float*)targets, (long long)n * K, logvar, U, out);
  }
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_train_adam_scratch(int64_t D, int64_t* doubles) {
  if (D <= 0 || !doubles) { set_error("lip_train_adam_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = adam_blocks(D);
  return LIP_OK;
}

int lip_train_adam(float* theta, float* m, float* v, const float* g, const float* a, float a_scalar, float lr, float b1, float b2,
                   float eps, int64_t t, int64_t D, double* reg, double* scratch, int64_t scratch_doubles, void* stream) {
  if (!theta || !m || !v || !g || !reg || !scratch || D <= 0 || t < 1 || scratch_doubles < adam_blocks(D) ||
      !(b1 >= 0.f && b1 < 1.f) || !(b2 >= 0.f && b2 < 1.f) ||
      !aligned16(theta, m, v, g) || (a && !aligned16(a))) {
    set_error("lip_train_adam: bad argument (null pointer, t < 1, betas outside [0, 1), scratch too small or a vector that is not 16-byte aligned)");
    return LIP_ERR_ARG;
  }
  AdamP p;
  p.theta = theta; p.m = m; p.v = v; p.g = g; p.a = a; p.a_s = a_scalar; p.lr = lr; p.b1 = b1; p.b2 = b2; p.eps = eps; p.D = D;
  p.inv_bc1 = (float)(1.0 / (1.0 - pow((double)b1, (double)t)));
  p.inv_bc2 = (float)(1.0 / (1.0 - pow((double)b2, (double)t)));
  const int blocks = adam_blocks(D);
  if (a) { hipLaunchKernelGGL(adam_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, scratch); }
  else { hipLaunchKernelGGL(adam_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, scratch); }
  LIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, blocks, reg);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

}  // extern "C"
