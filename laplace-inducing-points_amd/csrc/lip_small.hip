// Non-GEMM kernels of the linearised-network engine: all HBM-bound, coalesced along the channel
// (innermost NHWC) dimension, wavefront reductions where a sum is needed.
#include "lip_internal.h"

namespace lip {

// ---- per-channel column sums: red0[p][c] += sum_r g[p][r][c] ; red1[p][c] += sum_r g*xhat --------
// (bias / BN-parameter cotangents that could not be fused into an igemm epilogue)
// Blocks take `rpb` rows (512, fewer when the grid would not fill the chip: at 128 a block of the CIFAR sweep lived for
// one memory latency and its set-up and LDS / global atomics weighed as much as its loads).  Whenever N % 4 == 0 and the rows are 16-byte
// aligned a thread owns one column quad: float4 loads, private sums, four LDS atomics at the end.  (The first version
// did one LDS atomic and a 64-bit modulo per ELEMENT once N > 256: 0.3 - 0.4 TB/s on ResNet-50's 512 - 2048-channel
// layers, 4.6 ms of its 173 ms sweep.)
__global__ __launch_bounds__(256) void reduce_kernel(const ReduceP prm) {
  extern __shared__ float sm[];           // [2*N]
  const int N = prm.N, p = blockIdx.y;
  float* s0 = sm; float* s1 = sm + N;
  for (int i = threadIdx.x; i < 2 * N; i += 256) sm[i] = 0.f;
  __syncthreads();
  const int rbeg = blockIdx.x * prm.rpb;
  const int rows = min(prm.rpb, prm.R - rbeg);
  const long long seg0 = (long long)blockIdx.z * prm.R * N;      // per-example rows: segment z of R rows
  const float* g = prm.g + (long long)p * prm.g_ps + seg0 + (long long)rbeg * N;
  const float* xh = prm.xhat ? prm.xhat + seg0 + (long long)rbeg * N : nullptr;
  const long long cnt = (long long)rows * N;
  const int path = reduce_path(N, g, xh);
  if (path == SP_QUAD || path == SP_QUAD_WIDE) {
    const int nq = N >> 2;
    const int groups = nq <= 256 ? 256 / nq : 1;                 // row groups working side by side
    const int rg = nq <= 256 ? (int)threadIdx.x / nq : 0;
    for (int cq = nq <= 256 ? (int)threadIdx.x - rg * nq : (int)threadIdx.x; cq < nq && rg < groups; cq += 256) {
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
#pragma unroll 4
      for (int r = rg; r < rows; r += groups) {
        const float4 v = *reinterpret_cast<const float4*>(g + (long long)r * N + 4 * cq);
        a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
        if (xh) {
          const float4 x = *reinterpret_cast<const float4*>(xh + (long long)r * N + 4 * cq);
          a1.x += v.x * x.x; a1.y += v.y * x.y; a1.z += v.z * x.z; a1.w += v.w * x.w;
        }
      }
      atomicAdd(&s0[4 * cq], a0.x); atomicAdd(&s0[4 * cq + 1], a0.y); atomicAdd(&s0[4 * cq + 2], a0.z); atomicAdd(&s0[4 * cq + 3], a0.w);
      if (xh) { atomicAdd(&s1[4 * cq], a1.x); atomicAdd(&s1[4 * cq + 1], a1.y); atomicAdd(&s1[4 * cq + 2], a1.z); atomicAdd(&s1[4 * cq + 3], a1.w); }
    }
  } else if (path == SP_FIXED) {
    // fixed channel per thread: accumulate privately, one LDS atomic per thread
    const int c = threadIdx.x % N;
    float a0 = 0.f, a1 = 0.f;
    for (long long idx = threadIdx.x; idx < cnt; idx += 256) {
      const float v = g[idx];
      a0 += v;
      if (xh) a1 += v * xh[idx];
    }
    atomicAdd(&s0[c], a0);
    if (xh) atomicAdd(&s1[c], a1);
  } else {
    for (long long idx = threadIdx.x; idx < cnt; idx += 256) {
      const int c = (int)(idx % N);
      const float v = g[idx];
      atomicAdd(&s0[c], v);
      if (xh) atomicAdd(&s1[c], v * xh[idx]);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += 256) {
    if (prm.red0) atomicAdd(prm.red0 + (long long)p * prm.red0_ps + blockIdx.z * prm.red_seg + c, s0[c]);
    if (prm.red1) atomicAdd(prm.red1 + (long long)p * prm.red1_ps + blockIdx.z * prm.red_seg + c, s1[c]);
  }
}

hipError_t launch_reduce(const ReduceP& p0, int P, hipStream_t st) {
  ReduceP p = p0;
  const long long segs = (long long)P * (p.nseg > 0 ? p.nseg : 1);
  p.rpb = 512;
  while (p.rpb > 16 && (long long)((p.R + p.rpb - 1) / p.rpb) * segs < 2048) p.rpb >>= 1;
  dim3 grid((p.R + p.rpb - 1) / p.rpb, P, p.nseg > 0 ? p.nseg : 1);
  // with N % 4 == 0 every row block and segment of a probe starts on the alignment of the probe's first row
  int path = reduce_path(p.N, p.g, p.xhat);
  for (int q = 1; q < P && q < 4; ++q)
    if (reduce_path(p.N, p.g + (long long)q * p.g_ps, p.xhat) != path) path = SP_MIXED;
  LIP_ROUTE_PATH("reduce", path);
  if (p.nseg > 0) LIP_ROUTE("reduce/rows");
  hipLaunchKernelGGL(reduce_kernel, grid, dim3(256), 2 * p.N * sizeof(float), st, p);
  return hipGetLastError();
}

// ---- per-pair segmented reduces (lip_vjp_sqsum, lip_vjp_wnorm) -----------------------------------------------------
// Per (probe p, example i) pair the column sums  u0[c] = sum_{r < R} g[p][i][r][c],  u1[c] = sum_r g[p][i][r][c] xhat[i][r][c].
// Block = `cb` columns x (256 / cb) row lanes and the pairs of its group (PairGroupP), taken in order: per pair the row
// lanes sum strided rows and leave their sums in LDS; fold(q, sums) then runs on every thread between two barriers, and
// sums(u0, u1) adds the row lanes of the caller's column in lane order.  The kernels below differ in the fold only.
struct RedGroupP : PairGroupP {
  int cb;
};

template <class Fold>
__device__ __forceinline__ void reduce_pair_walk(const ReduceP& prm, const RedGroupP& pg, float* s0, float* s1, Fold&& fold) {
  const int N = prm.N, cb = pg.cb, RL = 256 / cb;
  const int cl = threadIdx.x % cb, rl = threadIdx.x / cb;
  const int c = blockIdx.x * cb + cl;
  const int q0 = blockIdx.y * pg.per, q1 = min(pg.pairs, q0 + pg.per);
  const bool on = c < N;
  for (int q = q0; q < q1; ++q) {
    const int p = q / pg.n_img, i = q - p * pg.n_img;
    const long long seg = (long long)i * prm.R * N;
    const float* g = prm.g + (long long)p * prm.g_ps + seg;
    const float* xh = prm.xhat ? prm.xhat + seg : nullptr;
    float t0 = 0.f, t1 = 0.f;
    if (on)
      for (int r = rl; r < prm.R; r += RL) {
        const float v = g[(long long)r * N + c];
        t0 += v;
        if (xh) t1 = fmaf(v, xh[(long long)r * N + c], t1);
      }
    s0[threadIdx.x] = t0; s1[threadIdx.x] = t1;
    __syncthreads();
    fold(q, [&](float& u0, float& u1) {
      u0 = u1 = 0.f;
      for (int k = 0; k < RL; ++k) { u0 += s0[k * cb + cl]; u1 += s1[k * cb + cl]; }
    });
    __syncthreads();                    // the next pair's lane sums overwrite s0 / s1
  }
}

// square-accumulating:  red0[c] += sum_{(p, i)} u0[c]^2 ,  red1[c] += sum_{(p, i)} u1[c]^2.  Row lane 0 squares and
// accumulates; one partial per group (plain stores) or, for a single group, added into the output directly.
struct SqRedP : RedGroupP {
  float* part0; float* part1;           // [groups][N] each, or null: one group
};

__global__ __launch_bounds__(256) void reduce_sqsum_kernel(const ReduceP prm, const SqRedP sq) {
  __shared__ float s0[256], s1[256];
  const int N = prm.N, grp = blockIdx.y;
  const int c = blockIdx.x * sq.cb + threadIdx.x % sq.cb, rl = threadIdx.x / sq.cb;
  float a0 = 0.f, a1 = 0.f;
  reduce_pair_walk(prm, sq, s0, s1, [&](int, auto sums) {
    if (rl == 0) {
      float u0, u1;
      sums(u0, u1);
      a0 = fmaf(u0, u0, a0); a1 = fmaf(u1, u1, a1);
    }
  });
  if (rl != 0 || c >= N) return;
  if (sq.part0) {
    if (prm.red0) sq.part0[(long long)grp * N + c] = a0;
    if (prm.red1) sq.part1[(long long)grp * N + c] = a1;
  } else {
    if (prm.red0) prm.red0[c] += a0;
    if (prm.red1) prm.red1[c] += a1;
  }
}

static int sq_cb(int N) {
  int cb = 64;
  while (cb > 1 && cb / 2 >= N) cb >>= 1;
  return cb;
}
static long long sq_colblocks(int N) { return (N + sq_cb(N) - 1) / sq_cb(N); }

long long reduce_sqsum_scratch(int N, long long pairs) {
  if (N <= 0 || pairs <= 0) return 0;
  const long long bound = pair_groups(sq_colblocks(N), pairs).bound;
  return bound > 1 ? 2ll * bound * N : 0;
}

hipError_t launch_reduce_sqsum(const ReduceP& p, int P, float* scratch, long long scratch_floats, hipStream_t st) {
  if (!p.red0 && !p.red1) return hipSuccess;
  if (p.N <= 0 || !pair_launch_ok(P, p.nseg, p.R)) return hipErrorInvalidValue;
  SqRedP sq;
  sq.cb = sq_cb(p.N);
  const long long tiles = sq_colblocks(p.N);
  const int G = pair_launch_groups(sq, tiles, P, p.nseg);
  if (!scratch_fits(G > 1 ? 2ll * G * p.N : 0, scratch, scratch_floats)) return hipErrorInvalidValue;
  sq.part0 = G > 1 ? scratch : nullptr;
  sq.part1 = G > 1 ? scratch + (long long)G * p.N : nullptr;
  LIP_ROUTE("reduce_sqsum");
  hipLaunchKernelGGL(reduce_sqsum_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(256), 0, st, p, sq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || G == 1) return e;
  if (p.red0 && (e = launch_sqsum_finish(sq.part0, G, p.N, p.red0, st)) != hipSuccess) return e;
  if (p.red1) e = launch_sqsum_finish(sq.part1, G, p.N, p.red1, st);
  return e;
}

// y[j] += sum_g partial[g][j] in group order (the fixed-order second pass of the square-accumulating reductions)
__global__ __launch_bounds__(256) void sqsum_finish_kernel(const float* __restrict__ partial, int G, long long len,
                                                           float* __restrict__ y) {
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < len; j += (long long)gridDim.x * 256) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += partial[(long long)g * len + j];
    y[j] += s;
  }
}

hipError_t launch_sqsum_finish(const float* partial, int G, long long len, float* y, hipStream_t st) {
  if (len <= 0 || G <= 0) return hipSuccess;
  const long long blocks = (len + 255) / 256;
  hipLaunchKernelGGL(sqsum_finish_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, partial, G, len, y);
  return hipGetLastError();
}

// weighted square norm:  out[(p, i)] += sum_c  w0[c] u0[c]^2 + w1[c] u1[c]^2.  Per pair the column sums are squared,
// weighted and summed over the block's columns (they sit in wave 0: shuffles) to one float, stored to
// partial[column block][pair].  wnorm_finish adds the column blocks of a pair in order.
struct WnRedP : RedGroupP {
  const float* w0; const float* w1;     // the (N,) weight slices of red0 / red1, or null (all ones)
  int has0, has1;
  float* partial;                       // [column blocks][pairs]
};

__global__ __launch_bounds__(256) void reduce_wnorm_kernel(const ReduceP prm, const WnRedP wn) {
  __shared__ float s0[256], s1[256];
  const int c = blockIdx.x * wn.cb + threadIdx.x % wn.cb;
  const bool lead = threadIdx.x / wn.cb == 0 && c < prm.N;      // (row lane 0: threads 0 .. cb - 1, cb <= 64 — all in wave 0)
  const float w0 = (lead && wn.has0) ? (wn.w0 ? wn.w0[c] : 1.f) : 0.f;
  const float w1 = (lead && wn.has1) ? (wn.w1 ? wn.w1[c] : 1.f) : 0.f;
  float* part = wn.partial + (long long)blockIdx.x * wn.pairs;
  reduce_pair_walk(prm, wn, s0, s1, [&](int q, auto sums) {
    if (threadIdx.x < 64) {
      float v = 0.f;
      if (lead) {
        float u0, u1;
        sums(u0, u1);
        v = fmaf(w0 * u0, u0, w1 * u1 * u1);
      }
      v = wave_sum(v);
      if (threadIdx.x == 0) part[q] = v;
    }
  });
}

long long reduce_wnorm_tiles(int N) { return N > 0 ? sq_colblocks(N) : 0; }

hipError_t launch_reduce_wnorm(const ReduceP& p, int P, bool ones, float* out, float* scratch, long long scratch_floats,
                               hipStream_t st) {
  if (!p.red0 && !p.red1) return hipSuccess;
  if (p.N <= 0 || !out || !pair_launch_ok(P, p.nseg, p.R)) return hipErrorInvalidValue;
  WnRedP wn;
  wn.cb = sq_cb(p.N);
  const long long tiles = sq_colblocks(p.N), pairs = (long long)P * p.nseg;
  const int G = pair_launch_groups(wn, tiles, P, p.nseg);
  if (!scratch_fits(tiles * pairs, scratch, scratch_floats)) return hipErrorInvalidValue;
  wn.has0 = p.red0 != nullptr; wn.has1 = p.red1 != nullptr;
  wn.w0 = ones ? nullptr : p.red0; wn.w1 = ones ? nullptr : p.red1;
  wn.partial = scratch;
  wnorm_route_hit(WN_REDUCE);
  hipLaunchKernelGGL(reduce_wnorm_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(256), 0, st, p, wn);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_wnorm_finish(scratch, (int)tiles, pairs, out, st);
}

// out[q] += sum_t partial[t][q], t ascending, the tiles added in float64 (one rounding per op and pair)
__global__ __launch_bounds__(256) void wnorm_finish_kernel(const float* __restrict__ partial, int T, long long pairs,
                                                           float* __restrict__ out) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= pairs) return;
  double s = 0.0;
  for (int t = 0; t < T; ++t) s += (double)partial[(long long)t * pairs + q];
  out[q] = (float)((double)out[q] + s);
}

hipError_t launch_wnorm_finish(const float* partial, int T, long long pairs, float* out, hipStream_t st) {
  if (pairs <= 0 || T <= 0) return hipSuccess;
  wnorm_route_hit(WN_FINISH);
  hipLaunchKernelGGL(wnorm_finish_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, partial, T, pairs, out);
  return hipGetLastError();
}

// launch census of the lip_vjp_wnorm kernels (lip_debug_wnorm_routes): a table of its own, apart from the route census
static const char* const kWnormRoutes[WN_ROUTES] = {
    "wgrad_wnorm<2,2,1,2>", "wgrad_wnorm<2,2,2,2>", "wgrad_wnorm<2,2,1,1>", "wgrad_wnorm<4,1,1,2>", "wgrad_wnorm<2,1,1,1>",
    "wgrad_wnorm<4,1,1,1>", "wgrad_wnorm_dense", "reduce_wnorm", "wnorm_finish",
};
static std::atomic<long long> g_wnorm_counts[WN_ROUTES];

void wnorm_route_hit(int id) {
  if (id >= 0 && id < WN_ROUTES) g_wnorm_counts[id].fetch_add(1, std::memory_order_relaxed);
}

int wnorm_routes_read(int64_t* counts, int n, const char** names) {
  const int m = n < WN_ROUTES ? n : (int)WN_ROUTES;
  for (int i = 0; i < m; ++i) {
    if (counts) counts[i] = g_wnorm_counts[i].load(std::memory_order_relaxed);
    if (names) names[i] = kWnormRoutes[i];
  }
  for (int i = 0; i < WN_ROUTES; ++i) g_wnorm_counts[i].store(0, std::memory_order_relaxed);
  return m;
}

// ---- mean pool over pixels: out[p][i][c] = inv * sum_pix in[p][i][pix][c]  (jnp.mean(x,(1,2))) ------
__global__ __launch_bounds__(256) void pool_fwd_kernel(const PoolP prm) {
  extern __shared__ float sm[];           // [C + 1024]: the sums, then the partial sums of SP_FIXED [256] / narrow SP_QUAD [G][C]
  const int C = prm.C, i = blockIdx.x, p = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += 256) sm[c] = 0.f;
  __syncthreads();
  const float* in = prm.in + (long long)p * prm.in_ps + (long long)i * prm.HW * C;
  const long long cnt = (long long)prm.HW * C;
  const int path = pool_fwd_path(C, in);
  if (path == SP_QUAD && (C >> 2) < 256) {
    // fewer than 256 channel quads: 256 / Q pixel groups side by side (as reduce_kernel's row groups), thread (cq, g)
    // adds pixels g, g + G, ... of its quad; the groups' partial sums meet in LDS and are added in group order (no float
    // atomics: the tangent stays the same from run to run)
    const int Q = C >> 2, G = 256 / Q, cq = threadIdx.x % Q, g = threadIdx.x / Q;
    float* part = sm + C;                 // [G][C]
    if (g < G) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int px = g; px < prm.HW; px += G) {
        const float4 v = *reinterpret_cast<const float4*>(in + (long long)px * C + 4 * cq);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
      *reinterpret_cast<float4*>(part + g * C + 4 * cq) = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float t = 0.f;
      for (int k = 0; k < G; ++k) t += part[k * C + c];
      sm[c] = t;
    }
  } else if (path == SP_QUAD) {
    // a thread owns whole channel quads: float4 loads down the pixels, no LDS traffic (wide layers: the per-element
    // LDS atomic + modulo of the general branch ran ResNet-50's 2048-channel pool at 0.3 TB/s)
    for (int cq = threadIdx.x; cq < (C >> 2); cq += 256) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int px = 0; px < prm.HW; ++px) {
        const float4 v = *reinterpret_cast<const float4*>(in + (long long)px * C + 4 * cq);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
      sm[4 * cq] = a.x; sm[4 * cq + 1] = a.y; sm[4 * cq + 2] = a.z; sm[4 * cq + 3] = a.w;
    }
  } else if (path == SP_FIXED) {
    // a thread keeps one channel; the 256 / C partial sums of a channel meet in LDS and are added in thread order (LDS
    // float atomics here made the tangent differ from run to run)
    float* part = sm + C;                 // [256]
    float a = 0.f;
    for (long long idx = threadIdx.x; idx < cnt; idx += 256) a += in[idx];
    part[threadIdx.x] = a;
    __syncthreads();
    if ((int)threadIdx.x < C) {
      float t = 0.f;
      for (int k = threadIdx.x; k < 256; k += C) t += part[k];
      sm[threadIdx.x] = t;
    }
  } else {
    // any other channel count or alignment: one channel per thread, pixels in order
    for (int c = threadIdx.x; c < C; c += 256) {
      float a = 0.f;
      for (int px = 0; px < prm.HW; ++px) a += in[(long long)px * C + c];
      sm[c] = a;
    }
  }
  __syncthreads();
  float* out = prm.out + (long long)p * prm.out_ps + (long long)i * C;
  for (int c = threadIdx.x; c < C; c += 256) out[c] = sm[c] * prm.inv;
}

hipError_t launch_pool_fwd(const PoolP& p, int P, hipStream_t st) {
  int path = pool_fwd_path(p.C, p.in);                 // C % 4 == 0: every example of a probe starts on the probe's alignment
  for (int q = 1; q < P && q < 4; ++q)
    if (pool_fwd_path(p.C, p.in + (long long)q * p.in_ps) != path) path = SP_MIXED;
  LIP_ROUTE_PATH("pool_fwd", path);
  hipLaunchKernelGGL(pool_fwd_kernel, dim3(p.n, P, 1), dim3(256), (p.C + 1024) * sizeof(float), st, p);
  return hipGetLastError();
}

// ---- pool backward: out[p][i][pix][c] = dphi[i][pix][c] * inv * in[p][i][c], plus reductions ------------
constexpr int PB_PIX = 16;
__global__ __launch_bounds__(256) void pool_bwd_kernel(const PoolP prm) {
  extern __shared__ float sm[];           // [2*C], and [2][1024] partial sums behind them when C / 4 < 256
  const int C = prm.C, i = blockIdx.y, p = blockIdx.z;
  float* s0 = sm; float* s1 = sm + C;
  const bool red = prm.red0 || prm.red1;
  if (red) {
    for (int c = threadIdx.x; c < 2 * C; c += 256) sm[c] = 0.f;
    __syncthreads();
  }
  const int pbeg = blockIdx.x * PB_PIX;
  const int npix = min(PB_PIX, prm.HW - pbeg);
  const float* in = prm.in + (long long)p * prm.in_ps + (long long)i * C;
  const long long base = ((long long)i * prm.HW + pbeg) * C;
  float* out = prm.out + (long long)p * prm.out_ps + base;
  const long long cnt = (long long)npix * C;
  // 256 % C == 0: a thread keeps ONE channel for all its pixels, so the column sums accumulate in registers and
  // reach LDS once per thread (an LDS atomic per element made this broadcast kernel run at 0.4 TB/s)
  const int path = pool_bwd_path(C, in, out, prm.dphi ? prm.dphi + base : nullptr, prm.xhat ? prm.xhat + base : nullptr);
  const bool fixed_c = path == SP_FIXED;
  float a0 = 0.f, a1 = 0.f;
  if (path == SP_QUAD) {
    // a thread owns a channel quad; sums stay in registers (no per-element atomics).  256 or more quads: a thread walks
    // all the block's pixels and adds to the per-probe totals directly.  Fewer: G = 256 / Q pixel groups side by side,
    // thread (cq, g) takes pixels g, g + G, ..., the groups leave their sums in LDS and one thread per channel adds them
    // (in group order) to the per-probe totals: as many global atomics as before
    const int Q = C >> 2;
    const bool narrow = Q < 256;
    const int G = narrow ? 256 / Q : 1, g = narrow ? (int)threadIdx.x / Q : 0;
    const int Gn = min(G, npix);                                 // groups that have a pixel
    const bool via_lds = red && Gn > 1;
    float* part0 = sm + 2 * C; float* part1 = part0 + 1024;      // [Gn][C] each, G C <= 1024
    for (int cq = narrow ? (int)threadIdx.x - g * Q : (int)threadIdx.x; cq < Q && g < Gn; cq += 256) {
      const float4 u = *reinterpret_cast<const float4*>(in + 4 * cq);
      float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
      for (int px = g; px < npix; px += G) {
        const long long o = (long long)px * C + 4 * cq;
        float4 v = make_float4(u.x * prm.inv, u.y * prm.inv, u.z * prm.inv, u.w * prm.inv);
        if (prm.dphi) {
          const float4 d = *reinterpret_cast<const float4*>(prm.dphi + base + o);
          v.x *= d.x; v.y *= d.y; v.z *= d.z; v.w *= d.w;
        }
        *reinterpret_cast<float4*>(out + o) = v;
        if (red) {
          r0.x += v.x; r0.y += v.y; r0.z += v.z; r0.w += v.w;
          if (prm.red1) {
            const float4 x = *reinterpret_cast<const float4*>(prm.xhat + base + o);
            r1.x += v.x * x.x; r1.y += v.y * x.y; r1.z += v.z * x.z; r1.w += v.w * x.w;
          }
        }
      }
      if (via_lds) {
        *reinterpret_cast<float4*>(part0 + g * C + 4 * cq) = r0;
        if (prm.red1) *reinterpret_cast<float4*>(part1 + g * C + 4 * cq) = r1;
        continue;
      }
      if (prm.red0) { float* d0 = prm.red0 + (long long)p * prm.red0_ps + 4 * cq;
        atomicAdd(d0, r0.x); atomicAdd(d0 + 1, r0.y); atomicAdd(d0 + 2, r0.z); atomicAdd(d0 + 3, r0.w); }
      if (prm.red1) { float* d1 = prm.red1 + (long long)p * prm.red1_ps + 4 * cq;
        atomicAdd(d1, r1.x); atomicAdd(d1 + 1, r1.y); atomicAdd(d1 + 2, r1.z); atomicAdd(d1 + 3, r1.w); }
    }
    if (!via_lds) return;
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float t0 = 0.f, t1 = 0.f;
      for (int k = 0; k < Gn; ++k) { t0 += part0[k * C + c]; if (prm.red1) t1 += part1[k * C + c]; }
      if (prm.red0) atomicAdd(prm.red0 + (long long)p * prm.red0_ps + c, t0);
      if (prm.red1) atomicAdd(prm.red1 + (long long)p * prm.red1_ps + c, t1);
    }
    return;
  }
  for (long long idx = threadIdx.x; idx < cnt; idx += 256) {
    const int c = (int)(idx % C);
    float v = in[c] * prm.inv;
    if (prm.dphi) v *= prm.dphi[base + idx];
    out[idx] = v;
    if (red) {
      const float x = prm.red1 ? v * prm.xhat[base + idx] : 0.f;
      if (fixed_c) { a0 += v; a1 += x; }
      else {
        atomicAdd(&s0[c], v);
        if (prm.red1) atomicAdd(&s1[c], x);
      }
    }
  }
  if (red && fixed_c && threadIdx.x < cnt) {
    const int c = threadIdx.x % C;
    atomicAdd(&s0[c], a0);
    if (prm.red1) atomicAdd(&s1[c], a1);
  }
  if (red) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      if (prm.red0) atomicAdd(prm.red0 + (long long)p * prm.red0_ps + c, s0[c]);
      if (prm.red1) atomicAdd(prm.red1 + (long long)p * prm.red1_ps + c, s1[c]);
    }
  }
}

hipError_t launch_pool_bwd(const PoolP& p, int P, hipStream_t st) {
  dim3 grid((p.HW + PB_PIX - 1) / PB_PIX, p.n, P);
  int path = pool_bwd_path(p.C, p.in, p.out, p.dphi, p.xhat);   // C % 4 == 0: blocks keep their probe's alignment
  for (int q = 1; q < P && q < 4; ++q)
    if (pool_bwd_path(p.C, p.in + (long long)q * p.in_ps, p.out + (long long)q * p.out_ps, p.dphi, p.xhat) != path) path = SP_MIXED;
  LIP_ROUTE_PATH("pool_bwd", path);
  const bool groups = (path == SP_QUAD || path == SP_MIXED) && (p.C >> 2) < 256;     // the quad path's pixel groups leave partial sums in LDS
  hipLaunchKernelGGL(pool_bwd_kernel, grid, dim3(256), (2 * p.C + (groups ? 2048 : 0)) * sizeof(float), st, p);
  return hipGetLastError();
}

// ---- window pools (max / average) ----------------------------------------------------------------------------
// A null argmax buffer selects the window AVERAGE (sum / (KH*KW), padding counted: flax.linen.avg_pool's default).
// primal: out = max over the window, argmax cached as the linear pixel index of the winning input (first max wins)
__global__ __launch_bounds__(256) void maxpool_primal_kernel(const MaxPoolP prm) {
  const long long total = (long long)prm.n * prm.OH * prm.OW * prm.C;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % prm.C);
    long long t = idx / prm.C;
    const int ow = (int)(t % prm.OW); t /= prm.OW;
    const int oh = (int)(t % prm.OH);
    const int i = (int)(t / prm.OH);
    const bool avg = prm.amax_w == nullptr;
    float best = avg ? 0.f : -3.0e38f; int bi = -1;
    for (int kh = 0; kh < prm.KH; ++kh) {
      const int ih = oh * prm.stride + kh - prm.pad_h;
      if (ih < 0 || ih >= prm.IH) continue;
      for (int kw = 0; kw < prm.KW; ++kw) {
        const int iw = ow * prm.stride + kw - prm.pad_w;
        if (iw < 0 || iw >= prm.IW) continue;
        const float v = prm.in[(((long long)i * prm.IH + ih) * prm.IW + iw) * prm.C + c];
        if (avg) best += v;
        else if (v > best) { best = v; bi = ih * prm.IW + iw; }
      }
    }
    if (avg) { prm.out[idx] = best * (1.f / (float)(prm.KH * prm.KW)); continue; }
    prm.out[idx] = best;
    prm.amax_w[idx] = (float)bi;
  }
}

hipError_t launch_maxpool_primal(const MaxPoolP& p, hipStream_t st) {
  const long long total = (long long)p.n * p.OH * p.OW * p.C;
  const long long blocks = (total + 255) / 256;
  if (p.amax_w) LIP_ROUTE("maxpool_primal/max"); else LIP_ROUTE("maxpool_primal/avg");
  hipLaunchKernelGGL(maxpool_primal_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, p);
  return hipGetLastError();
}

// tangent: out[p][i][oh][ow][c] = in[p][i][argmax][c]
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const MaxPoolP prm) {
  const int p = blockIdx.y;
  const long long per_img_out = (long long)prm.OH * prm.OW * prm.C, per_img_in = (long long)prm.IH * prm.IW * prm.C;
  const long long total = prm.n * per_img_out;
  const float* in = prm.in + (long long)p * prm.in_ps;
  float* out = prm.out + (long long)p * prm.out_ps;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % prm.C);
    const long long i = idx / per_img_out;
    if (!prm.amax) {
      long long t = (idx % per_img_out) / prm.C;
      const int ow = (int)(t % prm.OW), oh = (int)(t / prm.OW);
      float acc = 0.f;
      for (int kh = 0; kh < prm.KH; ++kh) {
        const int ih = oh * prm.stride + kh - prm.pad_h;
        if (ih < 0 || ih >= prm.IH) continue;
        for (int kw = 0; kw < prm.KW; ++kw) {
          const int iw = ow * prm.stride + kw - prm.pad_w;
          if (iw < 0 || iw >= prm.IW) continue;
          acc += in[i * per_img_in + ((long long)ih * prm.IW + iw) * prm.C + c];
        }
      }
      out[idx] = acc * (1.f / (float)(prm.KH * prm.KW));
      continue;
    }
    const int pix = (int)prm.amax[idx];
    out[idx] = pix >= 0 ? in[i * per_img_in + (long long)pix * prm.C + c] : 0.f;
  }
}

hipError_t launch_maxpool_fwd(const MaxPoolP& p, int P, hipStream_t st) {
  const long long total = (long long)p.n * p.OH * p.OW * p.C;
  const long long blocks = (total + 255) / 256;
  if (p.amax) LIP_ROUTE("maxpool_fwd/max"); else LIP_ROUTE("maxpool_fwd/avg");
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), P), dim3(256), 0, st, p);
  return hipGetLastError();
}

// cotangent: out[p][i][ih][iw][c] = dphi * sum over windows (oh, ow) covering (ih, iw) whose argmax is (ih, iw)
// of in[p][i][oh][ow][c]; plus the reductions of LIP_OP_POOL_BWD.  A gather, so no atomics on the tensor.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const MaxPoolP prm) {
  extern __shared__ float sm[];           // [2*C]
  const int C = prm.C, p = blockIdx.y;
  float* s0 = sm; float* s1 = sm + C;
  const bool red = prm.red0 || prm.red1;
  if (red) {
    for (int c = threadIdx.x; c < 2 * C; c += 256) sm[c] = 0.f;
    __syncthreads();
  }
  const long long per_img_in = (long long)prm.IH * prm.IW * C, per_img_g = (long long)prm.OH * prm.OW * C;
  const long long total = prm.n * per_img_in;
  const float* g = prm.in + (long long)p * prm.in_ps;
  float* out = prm.out + (long long)p * prm.out_ps;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % C);
    long long t = idx / C;
    const int iw = (int)(t % prm.IW); t /= prm.IW;
    const int ih = (int)(t % prm.IH);
    const long long i = t / prm.IH;
    const float me = (float)(ih * prm.IW + iw);
    float v = 0.f;
    for (int kh = 0; kh < prm.KH; ++kh) {
      const int th = ih + prm.pad_h - kh;
      if (th < 0 || (th % prm.stride) != 0) continue;
      const int oh = th / prm.stride;
      if (oh >= prm.OH) continue;
      for (int kw = 0; kw < prm.KW; ++kw) {
        const int tw = iw + prm.pad_w - kw;
        if (tw < 0 || (tw % prm.stride) != 0) continue;
        const int ow = tw / prm.stride;
        if (ow >= prm.OW) continue;
        const long long o = i * per_img_g + ((long long)oh * prm.OW + ow) * C + c;
        if (!prm.amax || prm.amax[o] == me) v += g[o];
      }
    }
    if (!prm.amax) v *= 1.f / (float)(prm.KH * prm.KW);
    if (prm.dphi) v *= prm.dphi[idx];
    out[idx] = v;
    if (red) {
      atomicAdd(&s0[c], v);
      if (prm.red1) atomicAdd(&s1[c], v * prm.xhat[idx]);
    }
  }
  if (red) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      if (prm.red0) atomicAdd(prm.red0 + (long long)p * prm.red0_ps + c, s0[c]);
      if (prm.red1) atomicAdd(prm.red1 + (long long)p * prm.red1_ps + c, s1[c]);
    }
  }
}

// Same gather, one channel QUAD per thread (C = 4, 8, ..., 1024: the grid stride is a multiple of C / 4, so a thread
// keeps its channels): 32-bit index arithmetic once per quad, float4 loads / stores, the reduction sums private in
// registers.  The scalar kernel above spends a 64-bit div / mod chain and two LDS atomics per element: 4.2 ms for
// ResNet-50's stem pool at 8 images x 64 probes (0.5 TB/s); it stays for the other channel counts.
__global__ __launch_bounds__(256) void maxpool_bwd_quad_kernel(const MaxPoolP prm) {
  extern __shared__ float sm[];           // [2*C]
  const int C = prm.C, nq = C >> 2, p = blockIdx.y;
  float* s0 = sm; float* s1 = sm + C;
  const bool red = prm.red0 || prm.red1;
  if (red) {
    for (int c = threadIdx.x; c < 2 * C; c += 256) sm[c] = 0.f;
    __syncthreads();
  }
  const unsigned total = (unsigned)prm.n * prm.IH * prm.IW * nq;
  const unsigned per_img_g = (unsigned)prm.OH * prm.OW * C;
  const float* g = prm.in + (long long)p * prm.in_ps;
  float* out = prm.out + (long long)p * prm.out_ps;
  const unsigned first = blockIdx.x * 256u + threadIdx.x;
  const int c = (int)(first % (unsigned)nq) * 4;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
  const float scale = prm.amax ? 1.f : 1.f / (float)(prm.KH * prm.KW);
  for (unsigned q = first; q < total; q += gridDim.x * 256u) {
    unsigned t = q / (unsigned)nq;
    const int iw = (int)(t % (unsigned)prm.IW); t /= (unsigned)prm.IW;
    const int ih = (int)(t % (unsigned)prm.IH);
    const unsigned i = t / (unsigned)prm.IH;
    const float me = (float)(ih * prm.IW + iw);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kh = 0; kh < prm.KH; ++kh) {
      const int th = ih + prm.pad_h - kh;
      if (th < 0 || (th % prm.stride) != 0) continue;
      const int oh = th / prm.stride;
      if (oh >= prm.OH) continue;
      for (int kw = 0; kw < prm.KW; ++kw) {
        const int tw = iw + prm.pad_w - kw;
        if (tw < 0 || (tw % prm.stride) != 0) continue;
        const int ow = tw / prm.stride;
        if (ow >= prm.OW) continue;
        const unsigned o = i * per_img_g + (unsigned)(oh * prm.OW + ow) * C + c;
        const float4 gv = *reinterpret_cast<const float4*>(g + o);
        if (prm.amax) {
          const float4 am = *reinterpret_cast<const float4*>(prm.amax + o);
          v.x += am.x == me ? gv.x : 0.f; v.y += am.y == me ? gv.y : 0.f;
          v.z += am.z == me ? gv.z : 0.f; v.w += am.w == me ? gv.w : 0.f;
        } else {
          v.x += gv.x; v.y += gv.y; v.z += gv.z; v.w += gv.w;
        }
      }
    }
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    const long long idx = (long long)q * 4;
    if (prm.dphi) {
      const float4 d = *reinterpret_cast<const float4*>(prm.dphi + idx);
      v.x *= d.x; v.y *= d.y; v.z *= d.z; v.w *= d.w;
    }
    *reinterpret_cast<float4*>(out + idx) = v;
    if (red) {
      r0.x += v.x; r0.y += v.y; r0.z += v.z; r0.w += v.w;
      if (prm.red1) {
        const float4 x = *reinterpret_cast<const float4*>(prm.xhat + idx);
        r1.x += v.x * x.x; r1.y += v.y * x.y; r1.z += v.z * x.z; r1.w += v.w * x.w;
      }
    }
  }
  if (red) {
    atomicAdd(&s0[c], r0.x); atomicAdd(&s0[c + 1], r0.y); atomicAdd(&s0[c + 2], r0.z); atomicAdd(&s0[c + 3], r0.w);
    if (prm.red1) { atomicAdd(&s1[c], r1.x); atomicAdd(&s1[c + 1], r1.y); atomicAdd(&s1[c + 2], r1.z); atomicAdd(&s1[c + 3], r1.w); }
    __syncthreads();
    for (int cc = threadIdx.x; cc < C; cc += 256) {
      if (prm.red0) atomicAdd(prm.red0 + (long long)p * prm.red0_ps + cc, s0[cc]);
      if (prm.red1) atomicAdd(prm.red1 + (long long)p * prm.red1_ps + cc, s1[cc]);
    }
  }
}

hipError_t launch_maxpool_bwd(const MaxPoolP& p, int P, hipStream_t st) {
  const long long total = (long long)p.n * p.IH * p.IW * p.C;
  const int nq = p.C >> 2;
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const bool quad = (p.C & 3) == 0 && nq <= 256 && 256 % nq == 0 && total < (1ll << 31) && (long long)p.n * p.OH * p.OW * p.C < (1ll << 31) &&
                    al16(p.in) && al16(p.out) && al16(p.amax) && al16(p.dphi) && al16(p.xhat) && (p.in_ps & 3) == 0 && (p.out_ps & 3) == 0;
  if (quad) {
    // few, long-lived blocks per probe: every block ends in 2 C global atomics on the same per-probe sums (4 096 blocks
    // per probe: 33 M contended atomics, 3.97 ms; 128 per probe: 0.4 ms)
    const long long blocks = (total / 4 + 255) / 256, want = 8192 / (P > 0 ? P : 1) > 8 ? 8192 / (P > 0 ? P : 1) : 8;
    if (p.amax) LIP_ROUTE("maxpool_bwd/quad"); else LIP_ROUTE("maxpool_bwd/quad/avg");
    hipLaunchKernelGGL(maxpool_bwd_quad_kernel, dim3((unsigned)(blocks < want ? blocks : want), P), dim3(256),
                       2 * p.C * sizeof(float), st, p);
    return hipGetLastError();
  }
  const long long blocks = (total + 255) / 256;
  if (p.amax) LIP_ROUTE("maxpool_bwd/scalar"); else LIP_ROUTE("maxpool_bwd/scalar/avg");
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048), P), dim3(256),
                     2 * p.C * sizeof(float), st, p);
  return hipGetLastError();
}

// ---- primal post-processing: z -> (xhat, a = act(y), dphi = act'(y)),  y = BN(z + bias) + res --------
__device__ __forceinline__ void act_eval(int act, float y, float& a, float& d) {
  if (act == 1) { a = y > 0.f ? y : 0.f; d = y > 0.f ? 1.f : 0.f; }
  else if (act == 2) { const float t = tanhf(y); a = t; d = 1.f - t * t; }
  else if (act == 3) {  // tanh-form GELU (flax.linen.gelu default approximate=True; src/toymodels.py:11)
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float u = k0 * (y + k1 * y * y * y);
    const float t = tanhf(u);
    a = 0.5f * y * (1.f + t);
    d = 0.5f * (1.f + t) + 0.5f * y * (1.f - t * t) * k0 * (1.f + 3.f * k1 * y * y);
  } else { a = y; d = 1.f; }
}

__global__ __launch_bounds__(256) void primal_post_kernel(const PrimalPostP prm) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < prm.count;
       idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % prm.N);
    float y = prm.z[idx];
    if (prm.bias) y += prm.bias[c];
    if (prm.gamma) {
      const float xh = (y - prm.mean[c]) * prm.rstd[c];
      if (prm.xhat) prm.xhat[idx] = xh;
      y = xh * prm.gamma[c] + prm.beta[c];
    }
    if (prm.res) y += prm.res[idx];
    float a, d;
    act_eval(prm.act, y, a, d);
    prm.a[idx] = a;
    if (prm.dphi) prm.dphi[idx] = d;
  }
}

hipError_t launch_primal_post(const PrimalPostP& p, hipStream_t st) {
  const long long blocks = (p.count + 255) / 256;
  static const char* const kAct[4] = {"none", "relu", "tanh", "gelu"};
  if (p.act >= 0 && p.act < 4) LIP_ROUTE_KEYED(p.act * 2 + (p.gamma ? 1 : 0), 8, "primal_post/%s%s", kAct[p.act], p.gamma ? "/bn" : "");
  hipLaunchKernelGGL(primal_post_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, p);
  return hipGetLastError();
}

// ---- softmax of the primal logits (one wave per example): p and sqrt(p)  (src/ggn.py:23-24,127) ------
__global__ __launch_bounds__(64) void softmax_kernel(const float* logits, float* prob, float* sqrtp, int n, int K) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const float* f = logits + (long long)i * K;
  float mx = -3.0e38f;
  for (int k = lane; k < K; k += 64) mx = fmaxf(mx, f[k]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += expf(f[k] - mx);
  s = wave_sum(s);
  const float inv = 1.f / s;
  for (int k = lane; k < K; k += 64) {
    const float pk = expf(f[k] - mx) * inv;
    prob[(long long)i * K + k] = pk;
    sqrtp[(long long)i * K + k] = sqrtf(pk);
  }
}

hipError_t launch_softmax(const float* logits, float* prob, float* sqrtp, int n, int K, hipStream_t st) {
  LIP_ROUTE("softmax");
  hipLaunchKernelGGL(softmax_kernel, dim3(n), dim3(64), 0, st, logits, prob, sqrtp, n, K);
  return hipGetLastError();
}

// ---- output-space head: Hessian / square-root-factor action per (probe, example) ----------------------
//   GGN : g = c (p.u - p (p^T u))                 src/ggn.py:125-131
//   LT  : U = c (s.u - (p^T u) s)                 src/ggn.py:29-39
//   L   : g = c (s.u - (s^T u) p)                 src/ggn.py:16-27
//   regressor: every mode multiplies by c (c carries exp(-logvar) or its square root, src/ggn.py:17-19,112-113)
__global__ __launch_bounds__(64) void head_kernel(const HeadP prm) {
  const int i = blockIdx.x, p = blockIdx.y, lane = threadIdx.x, K = prm.K;
  const float* u = prm.in + (long long)p * prm.in_ps + (long long)i * K;
  float* o = prm.out + (long long)p * prm.out_ps + (long long)i * K;
  if (head_scales(prm.classifier, prm.mode)) {
    for (int k = lane; k < K; k += 64) o[k] = prm.c * u[k];
    return;
  }
  const float* pp = prm.p + (long long)i * K;
  const float* ss = prm.s + (long long)i * K;
  float dot = 0.f;
  if (prm.mode == LIP_HEAD_L) { for (int k = lane; k < K; k += 64) dot += ss[k] * u[k]; }
  else                        { for (int k = lane; k < K; k += 64) dot += pp[k] * u[k]; }
  dot = wave_sum(dot);
  for (int k = lane; k < K; k += 64) {
    float v;
    if (prm.mode == LIP_HEAD_GGN)      v = pp[k] * (u[k] - dot);
    else if (prm.mode == LIP_HEAD_LT)  v = ss[k] * (u[k] - dot);
    else                               v = ss[k] * u[k] - dot * pp[k];
    o[k] = prm.c * v;
  }
}

hipError_t launch_head(const HeadP& p, int P, hipStream_t st) {
  if (head_scales(p.classifier, p.mode)) LIP_ROUTE("head/scale");
  else if (p.mode == LIP_HEAD_GGN) LIP_ROUTE("head/ggn");
  else if (p.mode == LIP_HEAD_LT) LIP_ROUTE("head/lt");
  else LIP_ROUTE("head/l");
  hipLaunchKernelGGL(head_kernel, dim3(p.n, P, 1), dim3(64), 0, st, p);
  return hipGetLastError();
}

// ---- y = a * x (initialises the output block with the prior-precision term alpha*V, src/lla.py:21-22) --
__global__ __launch_bounds__(256) void scale_copy_kernel(float* y, const float* x, float a, long long count) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (long long)gridDim.x * 256)
    y[idx] = a * x[idx];
}

__global__ void scale_copy_range_kernel(float* __restrict__ y, const float* __restrict__ x, float a, long long off, long long len,
                                        long long ld) {
  const long long base = (long long)blockIdx.y * ld + off;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
    y[base + i] = x ? a * x[base + i] : 0.f;
}

hipError_t launch_scale_copy_range(float* y, const float* x, float a, long long off, long long len, int P, long long ld, hipStream_t st) {
  if (len <= 0 || P <= 0) return hipSuccess;
  const long long blocks = (len + 255) / 256;
  hipLaunchKernelGGL(scale_copy_range_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)P), dim3(256), 0, st, y, x, a, off, len, ld);
  return hipGetLastError();
}

hipError_t launch_scale_copy(float* y, const float* x, float a, long long count, hipStream_t st) {
  const long long blocks = (count + 255) / 256;
  hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, y, x, a, count);
  return hipGetLastError();
}

// ---- y[p] += a (.) x[p]: the prior term of lip_ggn_vp_diag (a vector prior precision A = diag(a) in place of
// alpha I, src/lla.py:21-22), added after a sweep that ran with alpha = 0.  A row whose three operands share their
// alignment modulo 16 bytes streams as scalar head | float4 body | scalar tail; any other row runs on dwords (rows of an
// odd-D block differ from one another, so the choice is per row).  Grid-stride in both axes, no atomics: every element
// has one writer. ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_diag_kernel(float* __restrict__ Y, const float* __restrict__ X,
                                                       const float* __restrict__ a, long long N, int P) {
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    float* y = Y + (long long)p * N;
    const float* x = X + (long long)p * N;
    const unsigned long long ya = (unsigned long long)y, xa = (unsigned long long)x, aa = (unsigned long long)a;
    if ((((ya ^ xa) | (ya ^ aa)) & 15ull) == 0) {
      long long h = (4 - (long long)((ya >> 2) & 3)) & 3;      // scalars up to the first 16-byte boundary
      if (h > N) h = N;
      const long long G = (N - h) >> 2;
      for (long long g = t0; g < G; g += step) {
        const long long o = h + 4 * g;
        const float4 xv = *reinterpret_cast<const float4*>(x + o), av = *reinterpret_cast<const float4*>(a + o);
        float4 yv = *reinterpret_cast<const float4*>(y + o);
        yv.x += av.x * xv.x; yv.y += av.y * xv.y; yv.z += av.z * xv.z; yv.w += av.w * xv.w;
        *reinterpret_cast<float4*>(y + o) = yv;
      }
      if (blockIdx.x == 0) {
        for (long long i = threadIdx.x; i < h; i += 256) y[i] += a[i] * x[i];
        for (long long i = h + 4 * G + threadIdx.x; i < N; i += 256) y[i] += a[i] * x[i];
      }
    } else {
      for (long long i = t0; i < N; i += step) y[i] += a[i] * x[i];
    }
  }
}

hipError_t launch_add_diag(float* y, const float* x, const float* a, int P, long long N, hipStream_t st) {
  if (P <= 0 || N <= 0) return hipSuccess;
  const long long blocks = (N + 1023) / 1024;                   // one quad per thread and pass
  hipLaunchKernelGGL(add_diag_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)(P < 1024 ? P : 1024)), dim3(256),
                     0, st, y, x, a, N, P);
  return hipGetLastError();
}

}  // namespace lip
