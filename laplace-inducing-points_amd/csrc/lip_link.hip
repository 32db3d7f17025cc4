// Monte-Carlo softmax link of the closed-form predictives (lip_link_mc) and the semidefinite Cholesky factor that feeds
// it a full covariance (lip_link_chol).  include/lip.h defines both; this file is the launch geometry.
//
// lip_link_mc is one fused draw -> softmax -> accumulate kernel: no logit sample is ever written.  The work is Philox
// integer multiplies (about 40 quarter-rate v_mul per four normals) plus one v_exp per class, with next to no memory
// traffic, so the three shapes below only differ in how they keep lanes busy.  One workgroup of 256 threads owns one
// example in all of them, so a row's sums depend on (K, S) alone: chunk-invariant and repeatable, no atomics.
//   lane per draw  (link_lane_kernel, K <= 64; the factor form always): lane t runs the draws t, t + 256, ... whole, its
//                  logits and float64 sums in registers (KR = K rounded up to 4, 8, 16, 32 or 64), the factor read as LDS
//                  broadcasts.  The 256 lanes' sums meet in a xor butterfly per wave and in wave order through LDS.
//   wave per draw  (link_wave_kernel<GW, QPL, false>, K <= 2048): a group of GW = 16, 32 or 64 lanes runs one draw, lane l
//                  of it owning the quads l, l + GW, ... (QPL of them) of classes; max and sum are butterflies inside the
//                  group, no __syncthreads per draw; the float64 sums stay in registers, lane-private, and the groups
//                  of a block add up at the end in a fixed order.
//   block per draw (link_wave_kernel<64, QPL, true>, 2048 < K <= 8192): the 256 lanes share one draw, thread t owning the
//                  quads t, t + 256, ...; max and sum cross the four waves through LDS (two barriers per draw, against
//                  some 2000 cycles of Philox and v_exp per lane).  Per-wave sums in LDS would take 12 K bytes per wave:
//                  at K = 8192 one wave per CU, three SIMDs idle; here every class has one owner and the sums need no
//                  final reduction at all.
#include <cmath>
#include "lip_internal.h"

namespace lip {

constexpr unsigned LINK_TAG = 0x4C4E4B31u;           // fourth Philox counter word ("LNK1"): no stream shared with lip_head_sample
constexpr int LINK_NT = 256;
constexpr int LINK_FACTOR_MAX_K = 64, LINK_DIAG_MAX_K = 8192;
constexpr int LINK_WAVE_MAX_K = 2048;                // 64 lanes x 8 quads x 4 classes
// largest K of the diagonal form on the lane-per-draw path: measured on MI355X at (n, S) = (256, 1000), the lane path
// wins through K = 48 (18.8 against 19.6 ms per 200 calls) and loses at K = 64 (20.6 against 19.5); DESIGN.md section 4
constexpr int LINK_LANE_DEFAULT_K = 48;
static std::atomic<int> link_lane_max_k{LINK_LANE_DEFAULT_K};

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7FF8000000000000ll); }

// the four normals of quad q of draw s of example g
__device__ __forceinline__ void link_normals(unsigned g, unsigned s, unsigned q, unsigned long long seed, float* e) {
  unsigned int w[4];
  philox4x32(g, s, q, LINK_TAG, seed, w);
  box_muller_pair(w[0], w[1], e[0], e[1]);
  box_muller_pair(w[2], w[3], e[2], e[3]);
}

// a dead row: NaN probabilities and entropy, flag 1 (every thread of the block calls it)
__device__ __forceinline__ void link_dead_row(int i, int K, double* probs, double* ment, int* flags) {
  for (int k = threadIdx.x; k < K; k += blockDim.x) probs[(long long)i * K + k] = nan64();
  if (threadIdx.x == 0) { flags[i] = 1; if (ment) ment[i] = nan64(); }
}

// ---- lane per draw ---------------------------------------------------------------------------------------------------
template <int KR, bool FACTOR>
__global__ __launch_bounds__(LINK_NT) void link_lane_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                           const float* __restrict__ L, int K, int S, unsigned long long seed,
                                                           unsigned long long g0, double* __restrict__ probs,
                                                           double* __restrict__ ment, int* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) float s_m[KR];
  __shared__ __attribute__((aligned(16))) float s_a[FACTOR ? KR * KR : KR];   // sd, or the factor at row stride KR
  __shared__ double s_red[LINK_NT / 64][KR + 1];
  const int i = blockIdx.x, t = threadIdx.x;
  int bad = 0;
  for (int k = t; k < KR; k += LINK_NT) {
    float m = 0.f, sd = 0.f;
    if (k < K) {
      m = (float)mean[(long long)i * K + k];
      bad |= !isfinite(m);
      if (!FACTOR) {
        const double v = var[(long long)i * K + k];
        sd = (float)sqrt(v);
        bad |= !(v >= 0.0) || !isfinite(sd);
      }
    }
    s_m[k] = m;
    if (!FACTOR) s_a[k] = sd;
  }
  if (FACTOR) {
    for (int e = t; e < KR * KR; e += LINK_NT) {
      const int r = e / KR, c = e - r * KR;
      float v = 0.f;
      if (r < K && c <= r) {                                       // the lower triangle is all that a draw reads
        v = L[((long long)i * K + r) * K + c];
        bad |= !isfinite(v);
      }
      s_a[e] = v;
    }
  }
  bad = __syncthreads_or(bad);
  if (bad) { link_dead_row(i, K, probs, ment, flags); return; }

  double acc[KR], hacc = 0.0;
#pragma unroll
  for (int k = 0; k < KR; ++k) acc[k] = 0.0;
  const unsigned g = (unsigned)(g0 + (unsigned long long)i);
  for (int s = t; s < S; s += LINK_NT) {
    // the means, scales and factor stay in LDS (broadcast reads): hoisted out of this loop they would take up to KR^2 / 2
    // registers and spill
    asm volatile("" ::: "memory");
    float z[KR];
#pragma unroll
    for (int q = 0; q < KR / 4; ++q)
      if (4 * q < K) link_normals(g, (unsigned)s, (unsigned)q, seed, &z[4 * q]);
    if (FACTOR) {
      // z_k = m_k + sum_{j <= k} L_kj eps_j in place, k descending: the rows below k no longer need eps_k
#pragma unroll
      for (int k = KR - 1; k >= 0; --k)
        if (k < K) {
          float a = s_m[k];
#pragma unroll
          for (int j = 0; j <= k; ++j) a = fmaf(s_a[k * KR + j], z[j], a);
          z[k] = a;
        }
    } else {
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) z[k] = fmaf(s_a[k], z[k], s_m[k]);
    }
    float mx = z[0];
#pragma unroll
    for (int k = 1; k < KR; ++k)
      if (k < K) mx = fmaxf(mx, z[k]);
    float sum = 0.f, tt = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (k < K) {
        const float x = z[k] - mx, e = __expf(x);
        z[k] = e; sum += e; tt = fmaf(e, x, tt);
      }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (k < K) acc[k] += (double)(z[k] * inv);
    hacc += (double)(__logf(sum) - tt * inv);                      // H(p) = log sum - sum_k e_k x_k / sum
  }
  const int lane = t & 63, w = t >> 6;
#pragma unroll
  for (int k = 0; k <= KR; ++k)
    if (k < K || k == KR) {
      double v = k == KR ? hacc : acc[k < KR ? k : 0];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) s_red[w][k] = v;
    }
  __syncthreads();
  for (int k = t; k < K; k += LINK_NT)
    probs[(long long)i * K + k] = (((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k]) / (double)S;
  if (t == 0) {
    flags[i] = 0;
    if (ment) ment[i] = (((s_red[0][KR] + s_red[1][KR]) + s_red[2][KR]) + s_red[3][KR]) / (double)S;
  }
}

// ---- wave per draw / block per draw (diagonal form) -----------------------------------------------------------------
// A group (GW lanes, or with BLOCK the whole workgroup) shares a draw; member l owns the quads l, l + G, ... < QPL of them.
template <int GW, int QPL, bool BLOCK>
__global__ __launch_bounds__(LINK_NT) void link_wave_kernel(const double* __restrict__ mean, const double* __restrict__ var, int K,
                                                           int S, unsigned long long seed, unsigned long long g0,
                                                           double* __restrict__ probs, double* __restrict__ ment,
                                                           int* __restrict__ flags) {
  constexpr int NW = LINK_NT / 64;
  constexpr int G = BLOCK ? LINK_NT : GW;                          // members of a group
  constexpr int NG = BLOCK ? 1 : LINK_NT / GW;                     // groups of the block
  constexpr int NC = 4 * QPL;                                      // classes a member owns
  __shared__ float s_x[3][NW];                                     // BLOCK: per-wave max / sum / sum e x
  __shared__ double s_tot[BLOCK ? 1 : 4 * GW * QPL];               // !BLOCK: the groups' sums meet here, class-indexed
  __shared__ double s_h[NW];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l = BLOCK ? t : (t & (GW - 1)), grp = BLOCK ? 0 : t / GW;
  const int Q = (K + 3) >> 2;
  int bad = 0;
  for (int k = t; k < K; k += LINK_NT) {
    const float m = (float)mean[(long long)i * K + k];
    const double v = var[(long long)i * K + k];
    bad |= !isfinite(m) || !(v >= 0.0) || !isfinite((float)sqrt(v));
  }
  bad = __syncthreads_or(bad);
  if (bad) { link_dead_row(i, K, probs, ment, flags); return; }

  float m[NC], sd[NC];
  double acc[NC], hacc = 0.0;
#pragma unroll
  for (int r = 0; r < QPL; ++r)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int k = 4 * (l + G * r) + h, j = 4 * r + h;
      m[j] = 0.f; sd[j] = 0.f; acc[j] = 0.0;
      if (k < K) { m[j] = (float)mean[(long long)i * K + k]; sd[j] = (float)sqrt(var[(long long)i * K + k]); }
    }
  const unsigned g = (unsigned)(g0 + (unsigned long long)i);
  for (int s0 = 0; s0 < S; s0 += NG) {                             // the same trip count for every lane: the butterflies
    const bool live = s0 + grp < S;                                // below always run with whole groups
    const unsigned s = (unsigned)(live ? s0 + grp : s0);
    float z[NC];
#pragma unroll
    for (int r = 0; r < QPL; ++r) {
      const int q = l + G * r;
      z[4 * r] = z[4 * r + 1] = z[4 * r + 2] = z[4 * r + 3] = 0.f;
      if (q < Q) link_normals(g, s, (unsigned)q, seed, &z[4 * r]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < QPL; ++r)
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int j = 4 * r + h;
        z[j] = fmaf(sd[j], z[j], m[j]);
        if (4 * (l + G * r) + h < K) mx = fmaxf(mx, z[j]);
      }
#pragma unroll
    for (int off = (BLOCK ? 64 : GW) / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (BLOCK) {
      if (lane == 0) s_x[0][w] = mx;
      __syncthreads();
      mx = fmaxf(fmaxf(s_x[0][0], s_x[0][1]), fmaxf(s_x[0][2], s_x[0][3]));
    }
    float sum = 0.f, tt = 0.f;
#pragma unroll
    for (int r = 0; r < QPL; ++r)
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int j = 4 * r + h;
        const bool ok = 4 * (l + G * r) + h < K;
        const float x = ok ? z[j] - mx : 0.f, e = ok ? __expf(x) : 0.f;
        z[j] = e; sum += e; tt = fmaf(e, x, tt);
      }
#pragma unroll
    for (int off = (BLOCK ? 64 : GW) / 2; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, 64);
      tt += __shfl_xor(tt, off, 64);
    }
    if (BLOCK) {
      if (lane == 0) { s_x[1][w] = sum; s_x[2][w] = tt; }
      __syncthreads();                                             // s_x[0] is rewritten only behind this barrier, s_x[1..2] only
      sum = ((s_x[1][0] + s_x[1][1]) + s_x[1][2]) + s_x[1][3];     // behind the next draw's first one
      tt = ((s_x[2][0] + s_x[2][1]) + s_x[2][2]) + s_x[2][3];
    }
    const float inv = 1.0f / sum;
    if (live) {
#pragma unroll
      for (int j = 0; j < NC; ++j) acc[j] += (double)(z[j] * inv);
      hacc += (double)(__logf(sum) - tt * inv);
    }
  }
  const double dS = (double)S;
  if (BLOCK) {                                                     // every class has one owner, every thread the same hacc
#pragma unroll
    for (int r = 0; r < QPL; ++r)
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int k = 4 * (l + G * r) + h;
        if (k < K) probs[(long long)i * K + k] = acc[4 * r + h] / dS;
      }
    if (t == 0) { flags[i] = 0; if (ment) ment[i] = hacc / dS; }
    return;
  }
  // the groups of a wave in a xor butterfly (every lane ends with the wave's sum), then the waves in index order
#pragma unroll
  for (int off = GW; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
    hacc += __shfl_xor(hacc, off, 64);
  }
  for (int ww = 0; ww < NW; ++ww) {
    if (w == ww && lane < GW) {
#pragma unroll
      for (int r = 0; r < QPL; ++r)
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int c = 4 * (l + GW * r) + h;                      // < 4 GW QPL
          s_tot[c] = ww ? s_tot[c] + acc[4 * r + h] : acc[4 * r + h];
        }
      if (lane == 0) s_h[0] = ww ? s_h[0] + hacc : hacc;
    }
    __syncthreads();
  }
  for (int k = t; k < K; k += LINK_NT) probs[(long long)i * K + k] = s_tot[k] / dS;
  if (t == 0) { flags[i] = 0; if (ment) ment[i] = s_h[0] / dS; }
}

// ---- semidefinite Cholesky: one wave per matrix, the float64 working copy in LDS (row stride K | 1) ---------------------
__global__ __launch_bounds__(64) void link_chol_kernel(const double* __restrict__ cov, int K, float* __restrict__ Lout,
                                                       int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) double ch_a[];   // [K][ld]
  __shared__ double s_w[64];
  const int i = blockIdx.x, t = threadIdx.x, ld = K | 1;
  const double* C = cov + (long long)i * K * K;
  float* Lo = Lout + (long long)i * K * K;
  int bad = 0;
  for (int e = t; e < K * K; e += 64) {
    const int r = e / K, c = e - r * K;
    if (c <= r) {
      const double v = C[e];
      bad |= !isfinite(v);
      ch_a[r * ld + c] = v;
    }
  }
  __syncthreads();
  double dmax = t < K ? ch_a[t * ld + t] : -INFINITY;              // NaN-free unless bad
  s_w[t] = dmax;
  __syncthreads();
  if (!bad) {
    dmax = s_w[0];
    for (int k = 1; k < K; ++k) dmax = fmax(dmax, s_w[k]);
  }
  const double tol = 9.5367431640625e-07 * dmax;                   // 2^-20 max_i C_ii
  if (!bad && t < K) bad = ch_a[t * ld + t] < -tol;
  bad = __syncthreads_or(bad);
  if (bad) {
    for (int e = t; e < K * K; e += 64) Lo[e] = 0.f;
    if (t == 0) flags[i] = 1;
    return;
  }
  for (int j = 0; j < K; ++j) {
    // left-looking column j: row t >= j forms C_tj - sum_{k < j} L_tk L_jk, k ascending
    if (t >= j && t < K) {
      double sum = 0.0;
      for (int k = 0; k < j; ++k) sum += ch_a[t * ld + k] * ch_a[j * ld + k];
      ch_a[t * ld + j] -= sum;
    }
    __syncthreads();
    const double d = ch_a[j * ld + j];
    __syncthreads();                                               // row j reads d before it overwrites it
    if (t >= j && t < K) {
      const double piv = sqrt(d);
      ch_a[t * ld + j] = d > tol ? (t == j ? piv : ch_a[t * ld + j] / piv) : 0.0;
    }
    __syncthreads();
  }
  for (int e = t; e < K * K; e += 64) {
    const int r = e / K, c = e - r * K;
    Lo[e] = c <= r ? (float)ch_a[r * ld + c] : 0.f;
  }
  if (t == 0) flags[i] = 0;
}

}  // namespace lip

using namespace lip;

extern "C" {

int lip_link_chol(const double* cov, int32_t n, int32_t K, float* L, int32_t* flags, void* stream) {
  if (!cov || !L || !flags || n < 1 || K < 1 || K > LINK_FACTOR_MAX_K) {
    set_error("lip_link_chol: bad argument (null cov / L / flags, n < 1 or K outside 1..%d)", LINK_FACTOR_MAX_K);
    return LIP_ERR_ARG;
  }
  const size_t shmem = (size_t)K * (K | 1) * sizeof(double);
  hipLaunchKernelGGL(link_chol_kernel, dim3((unsigned)n), dim3(64), shmem, (hipStream_t)stream, cov, K, L, flags);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_link_mc(const double* mean, const double* var, const float* L, int32_t n, int32_t K, int32_t S, uint64_t seed,
                int64_t example_offset, double* probs, double* mean_entropy, int32_t* flags, void* stream) {
  if (!mean || !probs || !flags || (var != nullptr) == (L != nullptr) || n < 1 || S < 1 || K < 1) {
    set_error("lip_link_mc: bad argument (null mean / probs / flags, both or neither of var and L, n < 1, S < 1 or K < 1)");
    return LIP_ERR_ARG;
  }
  if (K > (L ? LINK_FACTOR_MAX_K : LINK_DIAG_MAX_K)) {
    set_error("lip_link_mc: bad argument (K = %d, at most %d with %s)", K, L ? LINK_FACTOR_MAX_K : LINK_DIAG_MAX_K,
              L ? "a factor" : "variances");
    return LIP_ERR_ARG;
  }
  if (example_offset < 0 || example_offset + (int64_t)n > (1ll << 32)) {
    set_error("lip_link_mc: bad argument (example_offset %lld with n = %d leaves 0 .. 2^32)", (long long)example_offset, n);
    return LIP_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;                      // like lip_head_sample, no entry in the route census
  const unsigned long long g0 = (unsigned long long)example_offset;
  const dim3 grid((unsigned)n), block(LINK_NT);
#define LINK_LANE(KR, F) \
  hipLaunchKernelGGL((link_lane_kernel<KR, F>), grid, block, 0, st, mean, var, L, K, S, (unsigned long long)seed, g0, probs, mean_entropy, flags)
#define LINK_WAVE(GW, QPL, B) \
  hipLaunchKernelGGL((link_wave_kernel<GW, QPL, B>), grid, block, 0, st, mean, var, K, S, (unsigned long long)seed, g0, probs, mean_entropy, flags)
  if (L || K <= link_lane_max_k.load(std::memory_order_relaxed)) {
    with_flag(L != nullptr, [&](auto f) {
      constexpr bool F = decltype(f)::value;
      if (K <= 4) LINK_LANE(4, F);
      else if (K <= 8) LINK_LANE(8, F);
      else if (K <= 16) LINK_LANE(16, F);
      else if (K <= 32) LINK_LANE(32, F);
      else LINK_LANE(64, F);
    });
  } else if (K <= 64) LINK_WAVE(16, 1, false);
  else if (K <= 128) LINK_WAVE(32, 1, false);
  else if (K <= 256) LINK_WAVE(64, 1, false);
  else if (K <= 512) LINK_WAVE(64, 2, false);
  else if (K <= 1024) LINK_WAVE(64, 4, false);
  else if (K <= LINK_WAVE_MAX_K) LINK_WAVE(64, 8, false);
  else if (K <= 4096) LINK_WAVE(64, 4, true);
  else LINK_WAVE(64, 8, true);
#undef LINK_LANE
#undef LINK_WAVE
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

int lip_debug_link_lane_max_k(int32_t K) {
  const int before = link_lane_max_k.load(std::memory_order_relaxed);
  if (K >= 0) link_lane_max_k.store(K > LINK_FACTOR_MAX_K ? LINK_FACTOR_MAX_K : K, std::memory_order_relaxed);
  return before;
}

}  // extern "C"
