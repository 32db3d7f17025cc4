// Layer-wise evidence terms of the structured Laplace posteriors (lip_evidence_terms): for every prior group g the pair
//   L_g = sum_{x in g} log1p(r x / alpha_g),    T_g = sum_{x in g} (r x / alpha_g) / (1 + r x / alpha_g),
// x the curvature eigenvalues that belong to the group, alpha_g = exp(log_alphas[g]) read from device memory.  Everything
// in float64.
//
// The eigenvalues are never written out: a segment of the table names them inside one value pool,
//   KRON: scale * max(lam_i, 0) * max(mu_j, 0), lam (rows) at off, mu (cols) right behind it: rows * cols terms,
//   LIST: scale * max(vals[off + i], 0), i < rows,
// so a Kronecker-factored block of Mt N eigenvalues costs Mt + N reads.  A term is s max(lam_i, 0) max(mu_j, 0) with
// s = scale * (r / alpha_g) formed once per workgroup: four roundings after exp(log_alpha_g) (three for LIST).
//
// Work split: the host cuts every segment into chunks of chunk_terms consecutive terms (the last one shorter); block c
// reduces chunk c: thread t takes the terms t, t + 256, ... of the chunk in ascending order into its own pair of sums, a
// wave adds its 64 lanes by the fixed halving tree, and thread 0 adds the four waves in index order through LDS and
// writes the pair to scratch[2 c .. 2 c + 1] with ordinary stores.  evidence_fold_kernel (one 64-lane block per group)
// then adds the partial pairs of the group's chunks in the order of the group-to-chunks table.  No atomics: the order of
// every addition is a function of the tables alone, so the result is bitwise reproducible.
//
// The host validates the host copy of the segment table before any launch.  The kernels check every index they read
// from the device tables against the extents they are given as well, and answer a broken table with NaN instead of an
// out-of-bounds access.
#include <cmath>

#include "lip_internal.h"

namespace lip {

constexpr int EV_T = 256;                      // threads of a chunk block (four waves)
constexpr long long EV_MAX_EDGE = 0x7fffffffll;

// the checks of one segment, shared by the entry point (host copy) and the chunk kernel (device copy)
__host__ __device__ inline bool ev_seg_ok(const lip_ev_seg_t& s, long long n_vals, int G) {
  if (s.kind != LIP_EV_KRON && s.kind != LIP_EV_LIST) return false;
  if (s.group < 0 || s.group >= G) return false;
  if (s.off < 0 || s.rows <= 0 || s.cols <= 0 || s.off > n_vals) return false;
  if (!(s.scale >= 0.0) || !(s.scale <= 1.79769313486231570815e308)) return false;       // finite, not negative, not NaN
  if (s.kind == LIP_EV_KRON) {
    if (s.rows > EV_MAX_EDGE || s.cols > EV_MAX_EDGE) return false;                      // rows * cols stays below 2^62
    return s.rows + s.cols <= n_vals - s.off;
  }
  return s.cols == 1 && s.rows <= n_vals - s.off;
}

__host__ __device__ inline long long ev_seg_terms(const lip_ev_seg_t& s) {
  return s.kind == LIP_EV_KRON ? (long long)s.rows * (long long)s.cols : (long long)s.rows;
}

__device__ __forceinline__ double ev_clamp(double v) { return v < 0.0 ? 0.0 : v; }       // a NaN stays a NaN

__device__ __forceinline__ void ev_add(double x, double& L, double& T) {
  L += log1p(x);
  T += x / (1.0 + x);
}

__global__ __launch_bounds__(EV_T) void evidence_chunk_kernel(const double* __restrict__ vals, long long n_vals,
                                                              const lip_ev_seg_t* __restrict__ segs, int n_seg,
                                                              const lip_ev_chunk_t* __restrict__ chunks, long long chunk_terms,
                                                              const double* __restrict__ log_alphas, int G, double r,
                                                              double* __restrict__ scratch) {
  __shared__ double sh[2][EV_T / 64];
  const long long c = blockIdx.x;
  const int tid = threadIdx.x;
  const lip_ev_chunk_t ch = chunks[c];
  bool ok = ch.seg >= 0 && ch.seg < n_seg;
  lip_ev_seg_t sg = {};
  long long total = 0;
  if (ok) {
    sg = segs[ch.seg];
    ok = ev_seg_ok(sg, n_vals, G);
    total = ok ? ev_seg_terms(sg) : 0;
    ok = ok && ch.start >= 0 && ch.start < total;
  }
  if (!ok) {                                                       // block-uniform: every thread read the same words
    if (tid == 0) { scratch[2 * c] = NAN; scratch[2 * c + 1] = NAN; }
    return;
  }
  const long long left = total - ch.start;
  const int count = (int)(left < chunk_terms ? left : chunk_terms);      // chunk_terms <= 2^30 (entry point)
  const double s = sg.scale * (r / exp(log_alphas[sg.group]));
  double L = 0.0, T = 0.0;
  if (sg.kind == LIP_EV_LIST) {
    const double* __restrict__ p = vals + sg.off + ch.start;
#pragma unroll 4
    for (int u = tid; u < count; u += EV_T) ev_add(ev_clamp(p[u]) * s, L, T);
  } else {
    const double* __restrict__ lam = vals + sg.off;
    const double* __restrict__ mu = lam + sg.rows;
    const long long cols = sg.cols;
    const long long t0 = ch.start + tid;                           // this thread's first term: (i, j) = divmod(t0, cols)
    long long i = t0 / cols, j = t0 - i * cols;
    const long long qi = EV_T / cols, qj = EV_T - qi * cols;       // one step of EV_T terms moves (i, j) by (qi, qj)
    for (int u = tid; u < count; u += EV_T) {
      ev_add((ev_clamp(lam[i]) * ev_clamp(mu[j])) * s, L, T);
      i += qi;
      j += qj;
      if (j >= cols) { j -= cols; ++i; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {                         // lane l += lane l + off: the fixed halving tree
    L += __shfl_down(L, off, 64);
    T += __shfl_down(T, off, 64);
  }
  if ((tid & 63) == 0) { sh[0][tid >> 6] = L; sh[1][tid >> 6] = T; }
  __syncthreads();
  if (tid == 0) {
    double l = sh[0][0], t = sh[1][0];
#pragma unroll
    for (int w = 1; w < EV_T / 64; ++w) { l += sh[0][w]; t += sh[1][w]; }
    scratch[2 * c] = l;
    scratch[2 * c + 1] = t;
  }
}

// out[g] = the partial pairs of the chunks group_chunks[group_ptr[g] .. group_ptr[g + 1]) added in that order
__global__ __launch_bounds__(64) void evidence_fold_kernel(const double* __restrict__ scratch, long long n_chunks,
                                                           const long long* __restrict__ group_ptr,
                                                           const int* __restrict__ group_chunks, double* __restrict__ out) {
  __shared__ double sh[2][64];
  const int g = blockIdx.x, lane = threadIdx.x;
  const long long p0 = group_ptr[g], p1 = group_ptr[g + 1];
  const bool ok = p0 >= 0 && p0 <= p1 && p1 <= n_chunks;
  double l = ok ? 0.0 : NAN, t = l;
  for (long long base = p0; ok && base < p1; base += 64) {         // ok, p0, p1 are block-uniform
    const long long rest = p1 - base;
    const int m = (int)(rest < 64 ? rest : 64);
    if (lane < m) {
      const long long c = group_chunks[base + lane];
      const bool in = c >= 0 && c < n_chunks;
      sh[0][lane] = in ? scratch[2 * c] : NAN;
      sh[1][lane] = in ? scratch[2 * c + 1] : NAN;
    }
    __syncthreads();
    if (lane == 0)
      for (int k = 0; k < m; ++k) { l += sh[0][k]; t += sh[1][k]; }
    __syncthreads();
  }
  if (lane == 0) { out[2 * g] = l; out[2 * g + 1] = t; }
}

}  // namespace lip

using namespace lip;

extern "C" {

int lip_evidence_terms_scratch(int64_t n_chunks, int64_t* doubles) {
  if (!doubles || n_chunks <= 0 || n_chunks > EV_MAX_EDGE) { set_error("lip_evidence_terms_scratch: bad argument"); return LIP_ERR_ARG; }
  *doubles = 2 * n_chunks;
  return LIP_OK;
}

int lip_evidence_terms(const double* vals, int64_t n_vals, const lip_ev_seg_t* segs_host, const lip_ev_seg_t* segs, int32_t n_seg,
                       const lip_ev_chunk_t* chunks, int64_t n_chunks, int64_t chunk_terms, const int64_t* group_ptr,
                       const int32_t* group_chunks, const double* log_alphas, int32_t G, double r, double* out,
                       double* scratch, int64_t scratch_doubles, void* stream) {
  if (!vals || !segs_host || !segs || !chunks || !group_ptr || !group_chunks || !log_alphas || !out || !scratch || n_vals <= 0 ||
      n_seg <= 0 || n_chunks <= 0 || n_chunks > EV_MAX_EDGE || chunk_terms <= 0 || chunk_terms > (1ll << 30) || G <= 0) {
    set_error("lip_evidence_terms: bad argument");
    return LIP_ERR_ARG;
  }
  if (!std::isfinite(r) || r < 0.0) { set_error("lip_evidence_terms: bad argument: r must be finite and not negative"); return LIP_ERR_ARG; }
  long long need = 0;
  for (int k = 0; k < n_seg; ++k) {
    if (!ev_seg_ok(segs_host[k], (long long)n_vals, G)) {
      const lip_ev_seg_t& s = segs_host[k];
      set_error("lip_evidence_terms: bad argument: segment %d (kind %d, offset %lld, rows %lld, cols %lld, scale %g, group %d) "
                "with a pool of %lld values and %d groups", k, (int)s.kind, (long long)s.off, (long long)s.rows, (long long)s.cols,
                s.scale, (int)s.group, (long long)n_vals, (int)G);
      return LIP_ERR_ARG;
    }
    const long long terms = ev_seg_terms(segs_host[k]);
    need += (terms + chunk_terms - 1) / chunk_terms;
  }
  if (need != n_chunks) {
    set_error("lip_evidence_terms: bad argument: %lld chunks given, the segments cut into %lld of %lld terms", (long long)n_chunks,
              need, (long long)chunk_terms);
    return LIP_ERR_ARG;
  }
  if (scratch_doubles < 2 * n_chunks) {
    set_error("lip_evidence_terms: scratch of %lld doubles, %lld needed (lip_evidence_terms_scratch)", (long long)scratch_doubles,
              (long long)(2 * n_chunks));
    return LIP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;                            // like lip_head_sample, no entry in the route census
  hipLaunchKernelGGL(evidence_chunk_kernel, dim3((unsigned)n_chunks), dim3(EV_T), 0, st, vals, (long long)n_vals, segs, (int)n_seg,
                     chunks, (long long)chunk_terms, log_alphas, (int)G, r, scratch);
  hipLaunchKernelGGL(evidence_fold_kernel, dim3((unsigned)G), dim3(64), 0, st, (const double*)scratch, (long long)n_chunks,
                     (const long long*)group_ptr, (const int*)group_chunks, out);
  LIP_CHECK_HIP(hipGetLastError());
  return LIP_OK;
}

}  // extern "C"
