/*
 * lip.h — C ABI of the MI355X-native linearised-Laplace engine (liblip_hip.so).
 *
 * The reference (nrholm1/Laplace-Inducing-Points) has no FFI: its hot path is a set of
 * Python closures over jax.jvp / jax.vjp (src/ggn.py:9-146).  This header is the build-defined
 * drop-in boundary underneath the same Python call surface (last bullet):
 * plain pointers and sizes, integer status codes, a hipStream_t passed as void*, no torch
 * types, no exceptions across the boundary.  All pointers are DEVICE pointers borrowed from
 * the caller (who owns them) unless stated otherwise.  Thread-compatible, not thread-safe.
 *
 * Each entry point cites the reference code it replaces.
 */
#ifndef LIP_H
#define LIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIP_OK 0
#define LIP_ERR_ARG 1       /* bad argument / shape the kernels do not support */
#define LIP_ERR_HIP 2       /* a HIP runtime call failed; see lip_last_error() */
#define LIP_ERR_STATE 3     /* engine not bound / tape missing */

/* ---- address spaces an op operand can live in -------------------------------------- */
enum {
  LIP_SP_NONE = -1,
  LIP_SP_THETA = 0,  /* flat MAP parameters theta (D floats)        src/utils.py:12-17     */
  LIP_SP_CONST = 1,  /* per-handle constants (BN factors, W^T)                              */
  LIP_SP_PRIM = 2,   /* cached primal tensors, one copy per example (never per probe)       */
  LIP_SP_WORK = 3,   /* tangent / cotangent workspace, [probe][example][H][W][C]            */
  LIP_SP_VIN = 4,    /* caller's input block V  (P, D) row-major                            */
  LIP_SP_YOUT = 5,   /* caller's output block Y (P, D) row-major                            */
  LIP_SP_HEAD = 6    /* caller's output-space block (P, n, K)                               */
};

/* operand = base[space] + off + probe * pstride   (all in floats) */
typedef struct {
  int32_t space;
  int32_t reserved;
  int64_t off;
  int64_t pstride;
} lip_ref_t;

/* one K-segment of an implicit GEMM:  acc[r][co] += sum_{kh,kw,c} A[img][ih][iw][c] * B[(kh*KW+kw)*C + c][co]
 * mode 0 (conv):            ih = oh*stride + kh - pad_h
 * mode 1 (transposed conv): t = oh + pad_h - kh, valid iff t >= 0 && t % stride == 0, ih = t/stride   */
typedef struct {
  lip_ref_t a;
  lip_ref_t b;
  int32_t IH, IW, C, KH, KW, stride, pad_h, pad_w, mode;
  int32_t flags;       /* LIP_SEG_B_TRANS: B is read as  B[(tap*C + c)][n] = b[(tap*N + n)*C + c]  — the HWIO kernel of the
                          convolution being transposed, used in place (per-probe weight tangents have no transposed copy) */
} lip_seg_t;
#define LIP_SEG_B_TRANS 1

enum {
  LIP_OP_IGEMM = 1,       /* implicit-GEMM conv / dense, fused epilogue (tangent fwd, data-grad, primal) */
  LIP_OP_WGRAD = 2,       /* weight-gradient GEMM reduced over examples and pixels, per probe            */
  LIP_OP_REDUCE = 3,      /* per-channel column sums (bias / BN-parameter cotangents)                    */
  LIP_OP_POOL_FWD = 4,    /* mean over pixels                                                            */
  LIP_OP_POOL_BWD = 5,    /* broadcast/HW, times dphi, plus parameter reductions                         */
  LIP_OP_PRIMAL_POST = 6, /* z -> xhat, y, a = act(y), dphi = act'(y)   (primal pass, once per binding)  */
  LIP_OP_SOFTMAX = 7,     /* logits -> p, sqrt(p)                        (primal pass)                   */
  LIP_OP_HEAD = 8,        /* output-space Hessian / square-root factor action  src/ggn.py:16-39,125-131  */
  /* window pools: with a NONE aux0 ref the three ops below compute the window AVERAGE (sum / (KH*KW), padding
     counted -- flax.linen.avg_pool, used by the reference's LeNet5 src/scalemodels.py:28,34) and its transpose */
  LIP_OP_MAXPOOL_PRIMAL = 9,  /* max pool of the primal activations + cached argmax (aux0)             */
  LIP_OP_MAXPOOL_FWD = 10,    /* tangent of max pool: gather at the cached argmax                      */
  LIP_OP_MAXPOOL_BWD = 11,    /* cotangent of max pool (gather over the covering windows), times dphi,
                                 plus parameter reductions — same epilogue fields as LIP_OP_POOL_BWD   */
  /* train tapes only (MAP training, below).  Both reuse fields of lip_op_t under the meaning given here:
     BN_STATS     between a BN unit's IGEMM and its PRIMAL_POST: the batch statistics of z = seg[0].a ([R][N]) with the
                  conv bias e0 (or NONE) and the BN scale e1, eps = bn_eps: aux0 <- mean, aux1 <- rsqrt(var + eps),
                  scale <- s = gamma * rstd (CONST space, written through the binding's writable constants), and the
                  running averages out (mean) / out2 (var) <- fscale * old + (1 - fscale) * batch, fscale the momentum
     BN_TRAIN_BWD after the op that forms a BN unit's cotangent g = seg[0].a and its reductions: out <- g - (e0 + xhat * e1) / R
                  with e0 = d beta, e1 = d gamma as reduced into YOUT; out is a tensor of its own (a residual consumer
                  upstream keeps reading g)                                                           */
  LIP_OP_BN_STATS = 12,
  LIP_OP_BN_TRAIN_BWD = 13
};

/* head modes */
enum {
  LIP_HEAD_GGN = 0,  /* g = c * (diag p - p p^T) Jv         src/ggn.py:125-131 (classifier), :112-113 (regressor: c*Jv) */
  LIP_HEAD_LT = 1,   /* U = c * L^T Jv  -> HEAD space       src/ggn.py:29-39  (W^T)   */
  LIP_HEAD_L = 2,    /* g = c * L U     <- HEAD space       src/ggn.py:16-27  (W)     */
  LIP_HEAD_OUT = 3,  /* U = Jv          -> HEAD space       raw JVP  (src/lla.py:153) */
  LIP_HEAD_IN = 4    /* g = U           <- HEAD space       raw VJP  (src/lla.py:66)  */
};

typedef struct {
  int32_t kind;
  int32_t nseg;
  lip_seg_t seg[3];
  int32_t n_img, OH, OW, N;      /* rows R = n_img*OH*OW, N output channels                       */
  int32_t act;                   /* PRIMAL_POST: activation id (0 none,1 relu,2 tanh,3 gelu-tanh) */
  int32_t ksplit;                /* WGRAD: split of the row reduction (atomics when > 1)          */
  int32_t M;                     /* WGRAD: KH*KW*Cin ; REDUCE/POOL: unused                        */
  int32_t classifier;            /* HEAD: 1 softmax-CE, 0 Gaussian regression                     */
  float   fscale;                /* POOL: 1/HW ; others unused                                    */
  float   bn_eps;
  lip_ref_t out;                 /* [probe][R][N]                                                 */
  lip_ref_t out2;                /* PRIMAL_POST: dphi ; SOFTMAX: sqrt(p)                          */
  lip_ref_t out3;                /* PRIMAL_POST: xhat                                             */
  lip_ref_t scale;               /* per-channel multiplier of the accumulator                     */
  lip_ref_t e0;                  /* per-channel addend (per probe if pstride != 0)                */
  lip_ref_t e1;                  /* per-channel multiplier of xhat, added                         */
  lip_ref_t xhat;                /* [R][N] primal                                                 */
  lip_ref_t res;                 /* residual addend [probe][R][N]                                 */
  lip_ref_t dphi;                /* [R][N] primal, multiplies the result                          */
  lip_ref_t red0;                /* += column sums of the result            (YOUT)                */
  lip_ref_t red1;                /* += column sums of result * xhat2        (YOUT)                */
  lip_ref_t xhat2;               /* [R][N] primal used by red1                                    */
  lip_ref_t aux0, aux1;          /* PRIMAL_POST: BN mean / rsqrt(var+eps) ; HEAD: p / sqrt(p)     */
} lip_op_t;

typedef struct lip_engine lip_engine_t;

/* ---- library ----------------------------------------------------------------------- */
int lip_abi_version(void);                 /* bumps on incompatible changes of this header (added entry points keep it) */
const char* lip_last_error(void);          /* text of the last failure on this thread            */
int lip_sizeof_op(void);                   /* sizeof(lip_op_t): lets the ctypes mirror self-check */
/* The route of a product: precision, split-K, Winograd and the Winograd probe walk, four process-wide modes with the
 * setters below.  An entry point that launches kernels reads the four ONCE, before its first launch, and uses that
 * snapshot for every pass and every launch it makes:
 *   - a setter takes effect at the next entry-point call;
 *   - a call in flight, on this or another thread, keeps the route it started with (the modes are atomic words: a
 *     setter may run at any time without tearing a call's plan).
 * A launch whose route needs per-stream scratch that cannot be had (the library keeps scratch for 16 (device, stream)
 * pairs; or the allocation fails) runs on the direct kernels instead, with the same result to rounding.
 *
 * arithmetic of the MFMA kernels: 0 = exact f32 MFMA (default, dtype "f32");
 * 1 = split-precision operands x = hi + lo in bf16, three bf16 MFMAs per product with f32 accumulation
 *     ("bf16x3": ~1e-5 relative error per product, ~5x fewer matrix-pipe cycles).                     */
int lip_set_precision(int32_t mode);
int lip_get_precision(void);
/* split-K implicit GEMM of under-filled launches (few probes): 1 = on (default), 0 = off.  The
 * results differ only in the summation order of the K axis; the switch exists so that a test can compare the two
 * orders in one process (the environment variable LIP_NOKSPLIT is read once).                          */
int lip_set_split_k(int32_t on);
/* Winograd F(2x2, 3x3) route of the 3x3 / stride-1 / pad-1 layers of the tangent and backward tapes (2.25x fewer
 * matrix-pipe multiplications, f32 in / f32 accumulate; the transforms move a layer's result by ~2e-7 relative;
 * DESIGN.md section 4): 0 = off (the direct implicit GEMMs everywhere), 1 = on (default: every eligible launch),
 * 2 = on (the value the tests set; the same launches as 1).  Never applied to the primal tape.  The environment
 * variable LIP_NOWINO is read once; this call overrides it.                                             */
int lip_set_winograd(int32_t mode);
int lip_get_winograd(void);
/* Probe walk of the Winograd conv kernel: a block handles w consecutive probes of its (tile block, column block).
 * 0 = automatic (default: the largest w in {1, 2, 4} that leaves the launch enough blocks; 1 for launches of at most
 * 8 probes), 1 / 2 / 4 = forced (capped by the probe count of the launch).  Every output except the float-atomic
 * column sums is bit-identical for every w.  lip_wino_walk_plan: what the automatic rule takes for a launch of gx
 * blocks per probe and P probes (a pure query).                                                        */
int lip_set_wino_walk(int32_t w);
int lip_get_wino_walk(void);
int lip_wino_walk_plan(int64_t gx, int32_t P);

/* ---- engine: one per (network, theta_MAP, data slice Z) binding on one device --------
 * Replaces the closure factories compute_ggn_vp / compute_W_vps (src/ggn.py:97,9): they
 * snapshot flat_params and Z at factory time; so does the engine (theta/consts/prim are
 * fixed until the next lip_engine_bind).                                                */
enum { LIP_TAPE_PRIMAL = 0, LIP_TAPE_TANGENT = 1, LIP_TAPE_BACKWARD = 2,
       LIP_TAPE_TRAIN_PRIMAL = 3, LIP_TAPE_TRAIN_BACKWARD = 4 };   /* the last two: MAP training only, optional */

int lip_engine_create(lip_engine_t** out, int64_t D, int32_t n_img, int32_t K);
int lip_engine_destroy(lip_engine_t* e);
int lip_engine_set_tape(lip_engine_t* e, int32_t which /*LIP_TAPE_*/, const lip_op_t* ops /*host*/, int32_t nops);
int lip_engine_bind(lip_engine_t* e, const float* theta, const float* consts, float* prim,
                    float* work, int64_t work_floats_per_probe, int32_t max_probes_per_chunk);
/* run the primal tape once (caches activations, BN-normalised values, act', softmax).   */
int lip_engine_primal(lip_engine_t* e, void* stream);

/* measurement hook: when enabled every op launch is bracketed by HIP events recorded on the launch
 * stream; lip_engine_profile_read sums elapsed ms and launch counts per op kind (index = LIP_OP_*)
 * and clears the log.  Used by bench.py for the live per-kernel roofline figure.                 */
int lip_engine_profile(lip_engine_t* e, int32_t enable);
int lip_engine_profile_read(lip_engine_t* e, double* ms_by_kind, int64_t* launches_by_kind, int32_t nkinds);

/* run ONE host-supplied op on a single probe chunk (P <= chunk size) against the engine's bound buffers and the
 * caller's V / Y / H blocks.  The second-order pass of the inducing-point gradient (reverse over the tangent tape,
 * src/train_inducing.py:195-232) is driven from the host op by op through this entry point.                    */
int lip_engine_run_op(lip_engine_t* e, const lip_op_t* op /*host*/, const float* V, float* Y, float* H, int32_t P,
                      int32_t head_mode, float head_c, void* stream);
/* test hook: run ops [first, first+count) of one tape on a single probe chunk (P <= chunk size) */
int lip_debug_run_ops(lip_engine_t* e, int32_t which, int32_t first, int32_t count, const float* V, float* Y,
                      float* H, int32_t P, int32_t head_mode, float head_c, void* stream);

/* test hook: launch-route census of the conv GEMM dispatchers and the square-sum kernels.  Every launch adds one to
 * a host-side counter of its route (kernel instantiation and the flags that picked it, e.g. "igemm_fast<4,1,1,2>/par/bv4");
 * no GPU work.  lip_debug_route_count: the number of routes known so far.  lip_debug_routes fills counts[i] and
 * names[i] (static strings) for i < min(n, count), either may be NULL, then clears every count.               */
int lip_debug_route_count(void);
int lip_debug_routes(int64_t* counts, int32_t n, const char** names);

/* Y[p] = scale * sum_i J_i^T H_i J_i V[p] + alpha * V[p]      src/ggn.py:133-144, src/lla.py:21-22
 * (scale carries N/M and, for the regressor, exp(-logvar): src/ggn.py:111-113)           */
int lip_ggn_vp(lip_engine_t* e, const float* V, float* Y, int32_t P, float scale, float alpha, void* stream);
/* Y[p] = scale * sum_i J_i^T H_i J_i V[p] + a (.) V[p]: lip_ggn_vp with a VECTOR prior precision A = diag(a) in place of
 * alpha I (generalises src/lla.py:21-22; one precision per layer is a = alpha_{g(j)}).  a is a (D,) device vector in
 * flat-parameter order.  Chunking, checks and status codes are those of lip_ggn_vp (not bound: LIP_ERR_STATE before Y is
 * touched; a null V / Y / a: LIP_ERR_ARG): the sweep runs as lip_ggn_vp's with alpha = 0, then one streaming pass adds
 * a (.) V over the probe chunk (no float atomics; V is not written).                                            */
int lip_ggn_vp_diag(lip_engine_t* e, const float* V, float* Y, int32_t P, float scale, const float* a, void* stream);
/* U[p,i,:] = c * L_i^T J_i V[p]   (mode LIP_HEAD_LT, src/ggn.py:55-62,84-85) or J_i V[p] (LIP_HEAD_OUT) */
int lip_jvp(lip_engine_t* e, const float* V, float* U, int32_t P, int32_t head_mode, float c, void* stream);
/* Y[p] = sum_i J_i^T (c * L_i U[p,i,:])  (LIP_HEAD_L, src/ggn.py:64-76,87-91) or raw (LIP_HEAD_IN) */
int lip_vjp(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float c, void* stream);
/* per-example rows of the same product: Y[(p*n + i)] = J_i^T (c * L_i U[p,i,:]), Y is (P*n, D) — no reduction
 * crosses examples, so a probe that holds e_k on every example yields the n rows J_i^T L_i e_k of the GGN's
 * square-root factor in ONE sweep (the reference builds them column by column: src/ggn.py:64-93, 207-219) */
int lip_vjp_rows(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float c, void* stream);
/* Square sum of those rows, ADDED into Y (D,):
 *   Y[j] += sum_p sum_i ( J_i^T (c * L_i U[p,i,:]) )_j^2   (LIP_HEAD_L)   or   sum_p sum_i ( J_i^T U[p,i,:] )_j^2  (LIP_HEAD_IN)
 * without the (P n, D) rows: every per-(probe, example) parameter cotangent is squared where it is formed.  With
 * U[p,i,:] = e_p (P = K one-hot probes on every example) and c = 1 this is the GGN diagonal before the N/M (and
 * exp(-logvar)) factor.  Y accumulates, so probe and example chunks add up; the result is bitwise reproducible (no
 * float atomics).  `scratch` (device, caller-owned) holds >= lip_vjp_sqsum_scratch(e, P) floats; a bad head mode, a
 * null pointer or too small a scratch returns LIP_ERR_ARG and leaves Y untouched.                              */
int lip_vjp_sqsum(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float c, float* scratch,
                  int64_t scratch_floats, void* stream);
/* scratch floats lip_vjp_sqsum needs for P probes on this engine's binding; bounded by the tape geometry (independent
 * of the example count and of P beyond a fixed group bound) and never more than for P = the bound chunk size      */
int lip_vjp_sqsum_scratch(lip_engine_t* e, int32_t P, int64_t* floats);

/* Weighted square norm of those rows, ADDED into out (P*n,):
 *   out[p*n + i] += sum_d w[d] * r_{p,i}[d]^2 ,   r_{p,i} = the row lip_vjp_rows writes for probe p and example i
 * (same head modes, same c) — the other reduction of the squares lip_vjp_sqsum forms: over the parameters, keeping the
 * (probe, example) pair.  w is a (D,) device vector in flat-parameter order (NULL: all ones).  With one-hot probes e_k
 * and w = the variances of a diagonal posterior this is the linearised predictive variance of output k at example i;
 * with w = NULL it is the diagonal of J J^T.  No rows are written, no float atomics: bitwise reproducible.  `scratch`
 * (device, caller-owned) holds >= lip_vjp_wnorm_scratch(e, P) floats: (pairs of one pass) x (output tiles of the
 * largest op).  A bad head mode, a null U / out or too small a scratch returns LIP_ERR_ARG and leaves out untouched. */
int lip_vjp_wnorm(lip_engine_t* e, const float* U, const float* w, float* out, int32_t P, int32_t head_mode, float c,
                  float* scratch, int64_t scratch_floats, void* stream);
int lip_vjp_wnorm_scratch(lip_engine_t* e, int32_t P, int64_t* floats);
/* test hook: launch census of the lip_vjp_wnorm kernels, a table of its own (they are not part of lip_debug_routes);
 * same calling convention as lip_debug_route_count / lip_debug_routes.                                          */
int lip_debug_wnorm_route_count(void);
int lip_debug_wnorm_routes(int64_t* counts, int32_t n, const char** names);

/* ---- Krylov / trace primitives on blocks of vectors: X is (P, N) row-major -----------
 * They replace what XLA emits for matfree's tridiag_sym (called at src/sample.py:114-126),
 * jax.scipy.sparse.linalg.cg (src/stochtrace.py:146,192; src/sample.py:71) and the
 * Hutchinson quadratic forms (src/stochtrace.py:30-34).                                 */
int lip_bdot(const float* X, const float* Y, float* out /*[P], overwritten*/, int32_t P, int64_t N, void* stream);
/* out[p] = sum_j w[j] X[p][j] Y[p][j], w (N,): lip_bdot in the metric diag(w) — the prior term v^T A v of the quadratic
 * forms of lip_ggn_vp_diag's operator (generalises alpha <v, v>, src/lla.py:21-22) without a (P, N) temporary.  X, Y as
 * for lip_bdot (shared alignment modulo 16 bytes); w at any 4-byte alignment.  Same order of the sums as lip_bdot.  */
int lip_bdot_w(const float* X, const float* Y, const float* w, float* out /*[P], overwritten*/, int32_t P, int64_t N,
               void* stream);
int lip_axpby(float* Y, const float* X, const float* a /*[P] or NULL*/, float a_s, const float* b /*[P] or NULL*/,
              float b_s, int32_t P, int64_t N, void* stream);      /* Y[p] = (a_s*a[p]) X[p] + (b_s*b[p]) Y[p] */
/* Lanczos basis Q is (P, kmax, ldq): row stride ldq >= N with ldq % 4 == 0 and a 16-byte aligned base, so the
 * basis — (j+1) x the traffic of w — streams with aligned 16-byte loads; w stays (P, N).
 * c[p][j] = <Q[p][j], w[p]>, j < k.                                                       */
int lip_multi_dot(const float* Q, const float* w, float* c /*[P][kmax], first k overwritten*/, int32_t P,
                  int32_t k, int32_t kmax, int64_t N, int64_t ldq, void* stream);
/* w[p] -= sum_j c[p][j] Q[p][j];  nrm2[p] = ||w[p]||^2 after the update.                 */
int lip_multi_axpy_norm(const float* Q, const float* c, float* w, float* nrm2 /*[P], overwritten*/, int32_t P,
                        int32_t k, int32_t kmax, int64_t N, int64_t ldq, void* stream);
/* Q[p][j] = w[p] * rsqrt(nrm2[p])   (next Lanczos vector; the row padding is zeroed)     */
int lip_scale_store(const float* w, const float* nrm2, float* Q, int32_t j, int32_t P, int32_t kmax, int64_t N,
                    int64_t ldq, void* stream);
/* fused CG update (one pass): x += a p; r -= a Ap; rr[p] = <r,r>, a[p] = rr_old[p]/pAp[p]; the rows x[p], r[p] of
 * inactive probes (active[p]==0; active == NULL: every probe is active) are left untouched and their rr_new[p] is
 * set to 0 (rr_new is zeroed before the pass): a caller keeps its own rr of an inactive probe.  The four blocks must
 * share their alignment modulo 16 bytes (any 4-byte alignment), as must X, Y of lip_bdot / lip_axpby and p, r of
 * lip_cg_direction.                                                                       */
int lip_cg_update(float* x, float* r, const float* p, const float* Ap, const float* rr_old, const float* pAp,
                  const int32_t* active, float* rr_new /*[P], overwritten*/, int32_t P, int64_t N, void* stream);
/* p = r + (rr_new/rr_old) p                                                              */
int lip_cg_direction(float* p, const float* r, const float* rr_new, const float* rr_old, const int32_t* active,
                     int32_t P, int64_t N, void* stream);
/* C (m, n) float64, overwritten = A B^T with A (m, K), B (n, K) float32 rows (row strides lda / ldb >= K, 4-byte
 * alignment suffices) accumulated in float64: the tall-skinny inner products whose float32 accumulation is too coarse —
 * the sampler's stiff-direction coefficients (src/sample.py:130-139 at cond 3e9), the Gram of Hutch++'s tall-skinny
 * orthonormalisation and its projections G Q^T (src/stochtrace.py:124-131).  Uses one partial-sum buffer per (device,
 * stream), so calls on different streams may overlap; without a buffer (a 17th (device, stream) pair, a failed
 * allocation) the partial tiles are added with float64 atomics instead.                                        */
int lip_dot_nt_f64(const float* A, int64_t lda, int32_t m, const float* B, int64_t ldb, int32_t n, int64_t K, double* C,
                   void* stream);
/* C (m, n) float32, overwritten = A B^T, same operand layout as lip_dot_nt_f64, float32 MFMA with the long reduction
 * axis split over the grid (partial tiles added by float atomics: the summation order, hence the last bits, vary from
 * run to run).  W^T applied to a block of draws on a materialised factor (src/sample.py:130-139).             */
int lip_gemm_nt(const float* A, int64_t lda, int32_t m, const float* B, int64_t ldb, int32_t n, int64_t K, float* C,
                void* stream);
/* Out (m, N) = T (m, k) B (k, N) + beta V (m, N): float32 MFMA, short reduction k (rows of a materialised factor), very
 * long N (= D); row strides ldt >= k, ldb / ldv / ldo >= N.  V may be NULL (no addend) or Out itself (in place); Out must
 * not alias T or B.  The second pass of a block of posterior draws, x = alpha^(-1/2) eps + (coefficients) Qm
 * (src/sample.py:139-143 in the Gram's eigenbasis), and the second product of the factor-mode GGN-vp.        */
int lip_gemm_nn_axpy(const float* T, int64_t ldt, int32_t m, int32_t k, const float* B, int64_t ldb, int64_t N, const float* V,
                     int64_t ldv, float beta, float* Out, int64_t ldo, void* stream);
/* Out[i] = zscale * Z[i] + sum_j Cm[i][j] Y[j],  i < r: r combinations of the s rows of Y (s, N) in one streaming pass
 * per 12 output rows; Cm (r, s) float64 row-major on the device, Z (r, N) optional (NULL: no addend).  Replaces
 * jnp.linalg.qr's Q of src/stochtrace.py:128 (as L^-1 Y after a Gram factorisation) and the deflation
 * G - (G Q) Q^T of :131.  Out must not alias Y or Z.                                                      */
int lip_rows_combine(const double* Cm, const float* Y, int64_t ldy, int32_t s, const float* Z, int64_t ldz, float zscale,
                     float* Out, int64_t ldo, int32_t r, int64_t N, void* stream);
/* out[d] += sum_{j<k} w[j] U[j][d]^2,  d < N: the weighted column square sums of the float32 rows U (k, N), row stride
 * ldu >= N, in float64; w (k) float64 on the device or NULL (all ones); out (N) float64 is ADDED into.  The marginal
 * variance of a low-rank posterior, diag(U^T diag(s) U), in one read of U and without a (k, N) temporary.  Every column
 * is owned by one thread that takes the rows in ascending order (no atomics, no scratch): out0 + sum, the sum started at
 * zero, each term one fused multiply-add of the exact square, so the result is bitwise reproducible and independent of
 * the grid.  16-byte loads when ldu % 4 == 0 and U is 16-byte aligned, dword loads otherwise.  A null U / out,
 * k or N <= 0 or ldu < N returns LIP_ERR_ARG and leaves out untouched.                                         */
int lip_cols_wsqsum(const float* U, int64_t ldu, int32_t k, int64_t N, const double* w /*[k], NULL = ones*/,
                    double* out /*[N], added into*/, void* stream);
/* Last-layer Laplace: the dense GGN block over theta_L = [bias (K), kernel (F, K) row-major] of a final Dense layer,
 * from the penultimate features and the softmax probabilities alone (no backward sweep).  G (DL, DL) float64
 * row-major, DL = (F + 1) K, ADDED into (example chunks sum into one G):
 *   G[(f K + k)][(g K + l)] += sum_i phit_i[f] phit_i[g] H_i[k][l],   phit_i = [1, Phi[i][0..F)],
 *   H_i = diag(p_i) - p_i p_i^T (Pr (n, K) float32 given)  or  I (Pr NULL: the Gaussian head).
 * Phi (n, F) float32, row stride ldphi >= F.  Operands are up-cast before any multiplication and accumulated in
 * float64 on the float64 matrix pipe; H is split as diag - outer, so the work is K weighted (F + 1)^2 Grams minus one
 * n-term Gram of the rows phit_i (x) p_i, rebuilt in registers: nothing of size (n, DL) is written.  The examples are
 * split over blocks whose partial tiles go to scratch (device, caller-owned, >= lip_ll_ggn_scratch(n, F, K) doubles;
 * the query covers both heads) and are added in index order by a second kernel: no atomics, so the result is bitwise
 * reproducible, and one triangle of tiles is computed and mirrored, so a symmetric G stays exactly symmetric.  A null
 * Phi / G / scratch, n, F or K <= 0, ldphi < F or too small a scratch returns LIP_ERR_ARG and leaves G untouched. */
int lip_ll_ggn(const float* Phi, int64_t ldphi, const float* Pr, int32_t n, int32_t F, int32_t K, double* G,
               double* scratch, int64_t scratch_doubles, void* stream);
int lip_ll_ggn_scratch(int32_t n, int32_t F, int32_t K, int64_t* doubles);
/* The matching test-time quadratic form, float64, out overwritten; S (DL, DL) float64 row-major (the posterior covariance):
 *   diag == 0: out (B, K, K), out[b][k][l] = sum_{f,g} phit_b[f] phit_b[g] S[(f K + k)][(g K + l)], computed for k <= l
 *              and mirrored (exactly symmetric);
 *   diag != 0: out (B, K), the k == l entries only, bitwise those of the full form.
 * No (B, K, DL) intermediate is written.  A null Phi / S / out, B, F or K <= 0 or ldphi < F returns LIP_ERR_ARG and
 * leaves out untouched. */
int lip_ll_predict(const float* Phi, int64_t ldphi, int32_t B, int32_t F, int32_t K, const double* S, double* out,
                   int32_t diag, void* stream);
/* Kronecker-factored last layer: the two factors of G_kron = c A (x) Bf over theta_L (flat index f K + k), ADDED into
 * A (F + 1, F + 1) and Bf (K, K), float64 row-major (example chunks sum into one pair):
 *   A[f][g] += sum_i phit_i[f] phit_i[g],   phit_i = [1, Phi[i][0..F)]   (the bias is feature 0),
 *   Bf[k][l] += sum_i delta_kl p_i[k] - p_i[k] p_i[l]   (Pr (n, K) float32 given)  or  n delta_kl   (Pr NULL).
 * Both are read off plain Grams of the augmented rows [1, phi_i] and [1, p_i], up-cast before any multiplication and
 * accumulated on the float64 matrix pipe by the tile loop of lip_ll_ggn: nothing of size (n, F + 1) or (n, K) in float64
 * is written, the examples are split over blocks whose partial tiles go to scratch (>= lip_ll_kron_factors_scratch
 * doubles; the query covers both heads) and are added in index order, no atomics: bitwise reproducible, and one triangle
 * of tiles is computed and mirrored, so symmetric factors stay exactly symmetric.  A null Phi / A / Bf / scratch, n, F
 * or K <= 0, ldphi < F or too small a scratch returns LIP_ERR_ARG and leaves A and Bf untouched. */
int lip_ll_kron_factors(const float* Phi, int64_t ldphi, const float* Pr, int32_t n, int32_t F, int32_t K, double* A,
                        double* Bf, double* scratch, int64_t scratch_doubles, void* stream);
int lip_ll_kron_factors_scratch(int32_t n, int32_t F, int32_t K, int64_t* doubles);
/* The predictive of the factored posterior S = sum_{j,l} (V_j V_j^T) (x) (Ub_l Ub_l^T) R[j][l]; V (F + 1, F + 1),
 * R (F + 1, K), Ub (K, K) float64 row-major.  Per test point: u = V^T phit, s_l = sum_j u_j^2 R[j][l] (both on the float64
 * matrix pipe, kept in scratch: B (F + 1 + K) doubles, lip_ll_kron_predict_scratch), then
 *   diag == 0: out (B, K, K), out[b][k][m] = sum_l Ub[k][l] Ub[m][l] s_b[l], computed for k <= m and mirrored;
 *   diag != 0: out (B, K), the k == m entries only, bitwise those of the full form.
 * Nothing of size (B, K, DL) and no (DL, DL) matrix is formed.  A null pointer, B, F or K <= 0, ldphi < F or too small
 * a scratch returns LIP_ERR_ARG and leaves out untouched. */
int lip_ll_kron_predict(const float* Phi, int64_t ldphi, int32_t B, int32_t F, int32_t K, const double* V, const double* R,
                        const double* Ub, double* out, int32_t diag, double* scratch, int64_t scratch_doubles, void* stream);
int lip_ll_kron_predict_scratch(int32_t B, int32_t F, int32_t K, int64_t* doubles);
/* Subnetwork Laplace: the dense GGN block over an index set idx (S entries of the flat parameter vector, device int64)
 * from per-example factor rows W (R, ldw) float32, ldw >= D: the rows lip_vjp_rows writes for one-hot probes in
 * LIP_HEAD_L mode.  G (S, S) float64 row-major, ADDED into (example chunks and class chunks sum into one G):
 *   G[a][c] += sum_{r < R} W[r][idx[a]] W[r][idx[c]].
 * A gather kernel first writes the compact (R, S) float32 panel into scratch (every scattered column read once, the
 * writes coalesced); the tile loop of lip_ll_ggn then runs over the panel: operands up-cast before any multiplication,
 * accumulated on the float64 matrix pipe, the rows split over blocks whose partial tiles go to scratch (device,
 * caller-owned, >= lip_sub_gram_scratch(R, S) doubles) and are added in index order by a second kernel: no atomics, so
 * the result is bitwise reproducible, and one triangle of tiles is computed and mirrored, so a symmetric G stays exactly
 * symmetric.  The gather clamps every index into [0, D): an index outside gives a wrong number, never an out-of-bounds
 * read (callers validate).  A null W / idx / G / scratch, R, S or D <= 0, ldw < D or too small a scratch returns
 * LIP_ERR_ARG and leaves G untouched. */
int lip_sub_gram_scratch(int32_t R, int32_t S, int64_t* doubles);
/* The first stage of lip_sub_gram on its own: panel (R, S) float32 row-major, overwritten, panel[r][a] = W[r][idx[a]]
 * with the same clamp.  Same argument checks; panel is left untouched on LIP_ERR_ARG. */
int lip_sub_gather(const float* W, int64_t ldw, int64_t D, int32_t R, const int64_t* idx, int32_t S, float* panel,
                   void* stream);
int lip_sub_gram(const float* W, int64_t ldw, int64_t D, int32_t R, const int64_t* idx, int32_t S, double* G, double* scratch,
                 int64_t scratch_doubles, void* stream);
/* The matching test-time quadratic form, float64, out overwritten.  Jr (K B, ldj) float32, ldj >= D, row k B + b the
 * Jacobian row of output k at test point b (the (P = K, n = B, D) block lip_vjp_rows writes for one-hot probes in
 * LIP_HEAD_IN mode); Sigma (S, S) float64 row-major (the posterior covariance over theta[idx]):
 *   diag == 0: out (B, K, K), out[b][k][l] = sum_{a,c} Jr[k B + b][idx[a]] Sigma[a][c] Jr[l B + b][idx[c]], computed for
 *              k <= l and mirrored (exactly symmetric);
 *   diag != 0: out (B, K), the k == l entries only, bitwise those of the full form.
 * The gathered float32 panel and T = panel Sigma ((K B, S) float64) live in scratch (>= lip_sub_predict_scratch(B, K, S)
 * doubles); nothing larger is written.  Both products run on the float64 matrix pipe.  Indices are clamped as in
 * lip_sub_gram.  A null pointer, B, K, S or D <= 0, ldj < D or too small a scratch returns LIP_ERR_ARG and leaves out
 * untouched. */
int lip_sub_predict_scratch(int32_t B, int32_t K, int32_t S, int64_t* doubles);
int lip_sub_predict(const float* Jr, int64_t ldj, int64_t D, int32_t B, int32_t K, const int64_t* idx, int32_t S,
                    const double* Sigma, double* out, int32_t diag, double* scratch, int64_t scratch_doubles, void* stream);

/* ---- Kronecker-factored curvature of every layer (KFAC / KFC; not reference functions) ------------------------
 * A layer block is the flat slice [bias (N)] + kernel (M x N row-major), M = KH KW C in (kh, kw, ci) order, read as an
 * (Mt, N) matrix with the bias as row 0 when there is one (Mt = M + 1).  Its curvature is approximated by
 * (recal / (n T)) A (x) S with the two float64 Grams below, T = OH OW.
 *
 * Input factor of one layer, ADDED into A (Mt, Mt) float64 row-major:
 *   A += sum_{i < n} sum_{t < OH OW} at_{i,t} at_{i,t}^T
 * X is the layer's float32 NHWC input (n, IH, IW, C); at_{i,t} the im2col patch of image i at output position t, zero
 * outside the image (the high-side padding of SAME included), with a leading 1 when bias != 0.  Lower-triangle 32 x 32
 * tiles x row ranges write partial tiles to scratch (>= lip_kfac_input_gram_scratch doubles), added in index order: no
 * atomics, bitwise reproducible, exactly symmetric; chunks of images add up.  The gather clamps its address and selects
 * zero: nothing outside X is read.  A null pointer, a non-positive extent, too small a scratch, or 2^31 or more input
 * elements or Gram rows returns LIP_ERR_ARG and leaves A untouched. */
int lip_kfac_input_gram_scratch(int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW, int32_t stride,
                                int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, int64_t* doubles);
int lip_kfac_input_gram(const float* X, int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW, int32_t stride,
                        int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, double* A, double* scratch,
                        int64_t scratch_doubles, void* stream);
/* Output factors of every layer from one backward sweep, ADDED into S: the sweep of lip_vjp_sqsum (same U, head modes
 * and c) in which every WGRAD op, instead of a weight gradient, Gram-multiplies the (P n OH OW, N) float32 rows g of its
 * cotangent operand, S_l += sum g g^T, and no bias / BN reduction is launched.  S holds the (N_l, N_l) float64 blocks of
 * the WGRAD ops in tape order; lip_vjp_kron_layout gives, per op, the flat offset of its kernel in theta, the offset of
 * its block in S and N_l (up to `cap` entries; *count the number of ops, *total the doubles of S).  The cotangent is
 * that of the layer's output after BN: the caller applies the frozen BN scale s s^T o S_l.  Probe passes add in order:
 * bitwise reproducible for a given chunking.  scratch holds >= lip_vjp_kron_scratch(e, P) doubles for the P of the call
 * (the largest need over every pass size the call can run; it is not monotone in P).  Every Gram of every pass is
 * checked before the first launch.  Status codes as
 * lip_vjp_sqsum; S is untouched on LIP_ERR_ARG / LIP_ERR_STATE. */
int lip_vjp_kron_scratch(lip_engine_t* e, int32_t P, int64_t* doubles);
int lip_vjp_kron_layout(lip_engine_t* e, int32_t cap, int64_t* kernel_off, int64_t* out_off, int32_t* N, int32_t* count,
                        int64_t* total);
int lip_vjp_kron(lip_engine_t* e, const float* U, double* S, int32_t P, int32_t head_mode, float c, double* scratch,
                 int64_t scratch_doubles, void* stream);
/* Closed-form predictive of one layer block under the factored posterior, float64, ADDED into out.  Jr (Kc B, ldj)
 * float32, row k B + b the Jacobian row of output k at test point b (lip_vjp_rows, LIP_HEAD_IN); the block is the
 * (Mt, N) matrix at flat offset off of a row, ldj >= off + Mt N; V (Mt, Mt), Ub (N, N), R (Mt, N) the fitted factors
 * (covariance sum_{j,l} V[f][j] V[g][j] Ub[k][l] Ub[m][l] R[j][l]).  With T_r = V^T J_r Ub,
 *   diag == 0: out (B, Kc, Kc), out[b][k][m] += sum_{j,l} R[j][l] T_{(k,b)}[j][l] T_{(m,b)}[j][l], computed for k <= m
 *              and mirrored (a symmetric out stays exactly symmetric);
 *   diag != 0: out (B, Kc), the k == m entries only, bitwise those of the full form.
 * J Ub and T live in scratch; lip_kfac_predict_scratch gives the doubles for all B points at once, a smaller scratch
 * (at least 2 Kc Mt N doubles, one point) makes the call run in chunks of points.  A null pointer, a non-positive
 * extent, ldj < off + Mt N, Mt N >= 2^31 or a scratch below one point returns LIP_ERR_ARG and leaves out untouched. */
int lip_kfac_predict_scratch(int32_t B, int32_t Kc, int32_t Mt, int32_t N, int64_t* doubles);
int lip_kfac_predict(const float* Jr, int64_t ldj, int32_t B, int32_t Kc, int64_t off, int32_t Mt, int32_t N, const double* V,
                     const double* Ub, const double* R, double* out, int32_t diag, double* scratch, int64_t scratch_doubles,
                     void* stream);
/* The marginal predictive variances of one layer block at G multiples of the fitted prior, float64, ADDED into out
 * (G, B, Kc).  With a prior s a (a the fitted prior, s > 0) the whitened factor only scales, so the fitted (V, Ub) serve
 * every s and, with Ev (Mt, N) the block's eigenvalues in the fitted whitened basis (R = 1 / (Ev + 1) at the fit) and
 * T_r = V^T J_r Ub,
 *   out[g][b][k] += sum_{j,l} T_{(k,b)}[j][l]^2 / (Ev[j][l] + scales[g]).
 * Jr, ldj, off, V, Ub and the row order are those of lip_kfac_predict; Ev is a device (Mt, N) float64 row-major matrix
 * with entries >= 0 (exact zeros included); scales is a HOST array of G finite values > 0, 1 <= G <= LIP_GRID_MAX.  The
 * weights 1 / (Ev + s_g) are correctly rounded divisions done once per call into scratch; J Ub lives in scratch, V^T (J Ub)
 * is formed tile by tile on the float64 matrix pipe, squared in registers and reduced against the G weight tiles, and the
 * (row, tile, g) partial sums (also in scratch) are folded in tile order: T is never written, no atomics.  Two calls with
 * identical arguments agree bitwise, a result does not depend on the scratch size, and slice g depends on scales[g]
 * alone, not on G or the other scales.  lip_kfac_predict_grid_scratch gives the doubles for all B points at once; a
 * smaller scratch, at least G Mt N + Kc (Mt N + ceil(Mt / 32) ceil(N / 32) G) doubles (the weights and one point), makes
 * the call run in chunks of points.  A null pointer, a non-positive extent, G < 1 or G > LIP_GRID_MAX, a scale that is
 * not finite or is <= 0, off < 0, ldj < off + Mt N, Mt N >= 2^31 or a scratch below one point returns LIP_ERR_ARG and
 * leaves out untouched; every check runs on the host before any launch. */
#define LIP_GRID_MAX 32
int lip_kfac_predict_grid_scratch(int32_t B, int32_t Kc, int32_t Mt, int32_t N, int32_t G, int64_t* doubles);
int lip_kfac_predict_grid(const float* Jr, int64_t ldj, int32_t B, int32_t Kc, int64_t off, int32_t Mt, int32_t N,
                          const double* V, const double* Ub, const double* Ev, const double* scales, int32_t G, double* out,
                          double* scratch, int64_t scratch_doubles, void* stream);
/* Second moments of the factor rows in a block's Kronecker eigenbasis (EKFAC), float64, ADDED into Lam (Mt, N):
 *   Lam[j][l] += sum_{r < R} ( sum_{f,k} V[f][j] W_r[f][k] Ub[k][l] )^2
 * W (R, ldw) float32, the rows lip_vjp_rows writes for one-hot probes in LIP_HEAD_L mode; W_r the (Mt, N) row-major
 * block at flat offset off of row r, ldw >= off + Mt N; V (Mt, Mt) and Ub (N, N) float64 row-major.  Chunks of examples
 * and of classes add into one Lam.  W_r Ub lives in scratch (stage one of lip_kfac_predict); V^T (W_r Ub) is formed tile
 * by tile on the float64 matrix pipe, squared in registers and summed over groups of rows, whose partial sums (also in
 * scratch) are folded in group order: V^T W_r Ub is never written, no atomics, and two calls with identical arguments
 * give bitwise identical results.  lip_kfac_eigen_sqsum_scratch gives the doubles for all R rows at once; a smaller
 * scratch (at least 2 Mt N doubles, one row) makes the call run in chunks of rows.  A null pointer, a non-positive
 * extent, off < 0, ldw < off + Mt N, Mt N >= 2^31 or a scratch below one row returns LIP_ERR_ARG and leaves Lam
 * untouched. */
int lip_kfac_eigen_sqsum_scratch(int32_t R, int32_t Mt, int32_t N, int64_t* doubles);
int lip_kfac_eigen_sqsum(const float* W, int64_t ldw, int32_t R, int64_t off, int32_t Mt, int32_t N, const double* V,
                         const double* Ub, double* Lam, double* scratch, int64_t scratch_doubles, void* stream);
/* The same second moments from one backward sweep, without factor rows.  The slice of a factor row that belongs to a
 * layer block is a per-example weight gradient, mat_l(J_i^T u) = At_i^T G_i diag(s) (At_i the (OH OW, Mt) im2col patches of
 * example i with the leading 1 of a bias, G_i the (OH OW, N) cotangent rows of the block's WGRAD op, s the frozen BN
 * scale), so V^T mat_l(.) Ub = (At_i V)^T (G_i Ub') with Ub' = diag(s) Ub: a per-example weight gradient of a 1x1
 * convolution with Mt input channels on the OH x OW map, both operands projected first.
 *
 * lip_kfac_project_patches: AV ((n OH OW), Mt) float32 row-major, overwritten, AV[(i,t)][j] = sum_e at_{i,t}[e] V[e][j];
 * X, the geometry and the patch order are those of lip_kfac_input_gram, V (Mt, Mt) float64 row-major.  The sum runs in
 * e order on the float64 matrix pipe and is rounded once, on the store; rows of AV are 16-byte aligned when Mt % 4 == 0
 * and AV is.  No scratch, no atomics, bitwise reproducible, nothing outside X is read.  A null pointer, a non-positive
 * extent, or 2^31 or more elements of X, AV or V returns LIP_ERR_ARG and leaves AV untouched.
 *
 * lip_rows_project: GU ((P R), N) float32 row-major, overwritten, GU[p R + r][m] = sum_c G[p pstride + r ldg + c] Ub[c][m];
 * G the float32 cotangent rows of a WGRAD op (R rows of N per probe, row stride ldg >= N, per-probe stride pstride),
 * Ub (N, N) float64 row-major (the caller folds diag(s) into it).  One launch when the probes are adjacent
 * (P == 1 or pstride == R ldg), one per probe otherwise; the same accumulation and single rounding.  A null pointer, a
 * non-positive extent, ldg < N, pstride < (R - 1) ldg + N with P > 1, or 2^31 or more elements of GU or Ub returns
 * LIP_ERR_ARG and leaves GU untouched. */
int lip_kfac_project_patches(const float* X, int32_t n, int32_t IH, int32_t IW, int32_t C, int32_t KH, int32_t KW,
                             int32_t stride, int32_t pad_h, int32_t pad_w, int32_t OH, int32_t OW, int32_t bias, const double* V,
                             float* AV, void* stream);
int lip_rows_project(const float* G, int64_t ldg, int64_t pstride, int32_t P, int32_t R, int32_t N, const double* Ub, float* GU,
                     void* stream);
/* The sweep that joins them, ADDED into Lam: the backward sweep of lip_vjp_kron (same U, head modes and c, no weight
 * gradient into parameter space, no bias / BN reduction) in which every WGRAD op projects its activation operand with
 * V[k] (once per op and pass) and the cotangent rows of the pass's probes with Ub[k], runs the square-accumulating
 * per-(probe, example) weight gradient of lip_vjp_sqsum on the projected pair (C = Mt, 1x1, stride 1, no padding, no
 * scale) into a zeroed (Mt, N) float32 block, and adds that block to Lam[k] in float64:
 *   Lam[k][j][m] += sum_{p < P} sum_{i < n} ( ((At_i V[k])^T (G_pi Ub[k]))[j][m] )^2.
 * V, Ub, Lam, Mt are HOST arrays of nblocks entries, one per WGRAD op in tape order (the order of lip_vjp_kron_layout):
 * device pointers to V (Mt, Mt), Ub (N, N) and Lam (Mt, N), float64 row-major, and the block's rows Mt[k] = KH KW C of
 * the op, plus 1 for a block with a bias row.  scratch: device, 16-byte aligned, >= lip_vjp_eigen_scratch(e, P) floats
 * (per op n OH OW Mt + P' n OH OW N + Mt N floats and the square sums' own scratch, P' the probes of a pass).  Passes
 * add in order and every kernel sums in a fixed order: bitwise reproducible for a given binding, probe count and
 * chunking.  Every op of every pass is checked before the first launch: a null operand, nblocks other than the number of
 * WGRAD ops, an Mt[k] that is not the op's KH KW C (+ 1), 2^31 or more elements of an operand on a pass, or too small a
 * scratch returns LIP_ERR_ARG and leaves every Lam untouched; LIP_ERR_STATE as lip_vjp_sqsum. */
int lip_vjp_eigen_scratch(lip_engine_t* e, int32_t P, int64_t* floats);
int lip_vjp_eigen(lip_engine_t* e, const float* U, const double* const* V, const double* const* Ub, double* const* Lam,
                  const int32_t* Mt, int32_t nblocks, int32_t P, int32_t head_mode, float c, float* scratch,
                  int64_t scratch_floats, void* stream);
/* The other reduction of the same products, ADDED into out (P n,) float32 like lip_vjp_wnorm: the predictive of a
 * Kronecker-factored posterior without any D-wide row,
 *   out[p n + i] += sum_k sum_{j,m} Rw[k][j][m] ( ((At_i V[k])^T (G_pi Ub[k]))[j][m] )^2  +  sum_{d in reductions} w_rem[d] (J_i^T u_p)_d^2.
 * Every WGRAD op projects its operands exactly as lip_vjp_eigen does and hands the projected pair (C = Mt, 1x1, stride
 * 1, no padding, no scale) to the weighted-norm weight gradient of lip_vjp_wnorm with the block's weights Rw[k]: a
 * device (Mt, N) row-major FLOAT32 matrix (at OH OW = 1 the bilinear route (av^2)^T Rw (gu^2)).  V, Ub, Rw, Mt: host
 * arrays of nblocks entries in tape order, as in lip_vjp_eigen.  w_rem: a (D,) float32 device vector addressed as the w
 * of lip_vjp_wnorm and read ONLY at the slices of the bias / BN reductions; the bias of a block with a bias row is
 * already counted by the block (its row 0), so the caller passes w_rem = 0 on every parameter inside a block.  w_rem
 * may be NULL: then no reduction is launched at all.  head_mode: LIP_HEAD_IN or LIP_HEAD_L.  scratch: device, 16-byte
 * aligned, >= lip_vjp_eigen_wnorm_scratch(e, P) floats (per op n OH OW Mt + P' n OH OW N floats and one float per
 * (output tile, pair) of the weighted norm, P' the probes of a pass; the largest op, against the reductions' need).
 * No atomics; the tiles of an op and the ops of the tape add in a fixed order and probe passes write disjoint slices:
 * bitwise reproducible.  Every op of every pass is checked before the first launch: a null operand, nblocks other than
 * the number of WGRAD ops, an Mt[k] that is not the op's KH KW C (+ 1), 2^31 or more elements of an operand on a pass,
 * or a scratch below the query returns LIP_ERR_ARG and leaves out untouched; LIP_ERR_STATE as lip_vjp_sqsum. */
int lip_vjp_eigen_wnorm_scratch(lip_engine_t* e, int32_t P, int64_t* floats);
int lip_vjp_eigen_wnorm(lip_engine_t* e, const float* U, const double* const* V, const double* const* Ub,
                        const float* const* Rw, const int32_t* Mt, int32_t nblocks, const float* w_rem, float* out, int32_t P,
                        int32_t head_mode, float c, float* scratch, int64_t scratch_floats, void* stream);
/* ---- MAP training (replaces the jitted _map_step of src/train_map.py:52-88) ---------------------------------------------
 * One step is a fixed number of calls whatever the depth: (load the batch into PRIM), lip_train_primal,
 * lip_train_refresh, lip_train_loss_head, lip_train_backward, lip_train_adam.  The kernels are streaming passes over
 * NHWC float32 without atomics: every sum runs in a fixed order, so equal inputs give equal bits.
 *
 * lip_engine_train_bind: the WRITABLE view of the constants of a bound engine (consts must be the pointer given to
 * lip_engine_bind) and a float64 scratch of >= the largest lip_train_bn_stats_scratch(R, N) over the BN_STATS ops of the
 * train primal tape (16-byte aligned; may be NULL for a net without BN).  Re-binding the engine drops it.
 * lip_engine_set_refresh: the transposed kernels the backward tapes read, `count` rows of 6 int64 (host):
 * (offset of W in THETA, offset of Wt in CONST, offset of s in CONST or -1, taps KH KW, Cin, Cout).
 * lip_train_primal: the train primal tape (batch statistics instead of the constants' running ones; updates the running
 * averages in CONST).  PRIM then holds train-mode activations: the sweeps of the other tapes refuse to run until the next
 * lip_engine_primal.  lip_train_refresh: Wt[t][co][ci] = W[t][ci][co] * s[co] for every row of the table, from the
 * current THETA and the s the train primal pass wrote.  lip_train_backward: Y (D,) = sum_i J_i^T U[i] through the train
 * backward tape (Y is overwritten; U (n, K) are raw head cotangents), J the Jacobian of the train-mode network, the
 * batch statistics differentiated through.  Status codes as lip_vjp; LIP_ERR_STATE without the train tapes, the
 * writable constants or a train primal pass. */
int lip_engine_train_bind(lip_engine_t* e, float* consts, double* scratch, int64_t scratch_doubles);
int lip_engine_set_refresh(lip_engine_t* e, const int64_t* table /*host, count x 6*/, int32_t count);
int lip_train_primal(lip_engine_t* e, void* stream);
int lip_train_refresh(lip_engine_t* e, void* stream);
int lip_train_backward(lip_engine_t* e, const float* U, float* Y, void* stream);
/* The kernels on their own.
 * lip_train_bn_stats: per channel c < N of z (R, N), with Flax BatchNorm's defaults: mean[c] = E[z] + bias[c],
 * var[c] = E[(z - E z)^2] (biased), rstd[c] = rsqrt(var + eps), s[c] = gamma[c] * rstd[c] (float32 product; gamma NULL: 1),
 * run_mean / run_var <- momentum * old + (1 - momentum) * (mean / var), in place.  Any output may be NULL.  The sums are
 * float64 sums of d = z[r][c] - z[0][c] and d^2 over chunks of rows, folded in chunk order: no E[z^2] - E[z]^2 in
 * float32.  scratch: >= lip_train_bn_stats_scratch(R, N) doubles, 16-byte aligned.  A null z / scratch, R or N <= 0,
 * R N >= 2^31, a negative eps, a momentum outside [0, 1] or too small a scratch returns LIP_ERR_ARG, nothing written. */
int lip_train_bn_stats_scratch(int32_t R, int32_t N, int64_t* doubles);
int lip_train_bn_stats(const float* z, int32_t R, int32_t N, const float* bias, const float* gamma, float eps, float momentum,
                       float* mean, float* var, float* rstd, float* s, float* run_mean, float* run_var, double* scratch,
                       int64_t scratch_doubles, void* stream);
/* out[r][c] = g[r][c] - (dbeta[c] + xhat[r][c] * dgamma[c]) / R; out must not be g. */
int lip_train_bn_backward(const float* g, const float* xhat, const float* dbeta, const float* dgamma, int32_t R, int32_t N,
                          float* out, void* stream);
/* Wt[t][co][ci] = W[t][ci][co] * s[co], t < taps (s NULL: no scale): engine.build_consts' "wt" entries on the device. */
int lip_train_wt_refresh(const float* W, const float* s, float* Wt, int32_t taps, int32_t cin, int32_t cout, void* stream);
/* Loss head, one launch.  classifier != 0: outputs (n, K) logits, targets (n,) int64 labels; U (n, K) = (softmax - e_y) / n,
 * out[0] = sum_i (logsumexp(f_i) - f_i[y_i]) in float64 (the caller divides by n), out[1] = 0; the log-sum-exp is taken
 * about the row maximum, so logits of any finite size give finite results; a label outside [0, K) makes out[0] NaN.
 * classifier == 0: outputs, targets (n, K) float32; U = (f - y) exp(-logvar) / (n K), out[0] = 0.5 sum (log(2 pi) + logvar
 * + (f - y)^2 exp(-logvar)) (src/train_map.py:73-77 before its mean), out[1] = d(mean NLL)/d logvar.  out: 2 doubles. */
int lip_train_loss_head(const float* outputs, const void* targets, int32_t n, int32_t K, int32_t classifier, float logvar, float* U,
                        double* out, void* stream);
/* One Adam step with the prior folded in (optax.adam, eps_root = 0), D entries, step t >= 1:
 *   gt = g + a theta;  m = b1 m + (1 - b1) gt;  v = b2 v + (1 - b2) gt^2;
 *   theta -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
 * a: a (D,) precision vector, or NULL for the scalar a_scalar.  reg[0] = 0.5 sum a theta^2 of the theta BEFORE the step,
 * float64.  One read and one write of theta, m, v; one read of g and a.  The five vectors must be 16-byte aligned.
 * scratch: >= lip_train_adam_scratch(D) doubles. */
int lip_train_adam_scratch(int64_t D, int64_t* doubles);
int lip_train_adam(float* theta, float* m, float* v, const float* g, const float* a, float a_scalar, float lr, float b1, float b2,
                   float eps, int64_t t, int64_t D, double* reg, double* scratch, int64_t scratch_doubles, void* stream);
/* counter-based Rademacher (+-1) / standard-normal fill of a (P, N) block               */
int lip_fill_rademacher(float* X, int32_t P, int64_t N, uint64_t seed, void* stream);
int lip_fill_normal(float* X, int32_t P, int64_t N, uint64_t seed, void* stream);
/* Monte-Carlo Fisher head cotangents: for sample s < S and example i < n of the softmax rows probs (n, K), draw a class
 * yhat ~ p_i and write U[s][i][k] = (k == yhat ? 1 : 0) - p_i[k] (one float32 subtraction), labels[s][i] = yhat when
 * labels is not null.  U is (S, n, K) row-major and is overwritten.  The draw is defined in integers, so it does not
 * depend on the launch geometry and a host can replay it: q_k = floor((double)p_i[k] * 2^40) as a 64-bit unsigned
 * integer, pre_k = q_0 + ... + q_k, Q = pre_{K-1} (Q = 0 for a row with an entry outside [0, 1], NaN included); Philox4x32-10
 * with the counter words (g, s, 0x9E3779B9, 0xBB67AE85), g = example_offset + i, keyed by the two words of seed (the
 * generator of lip_fill_normal) gives w0..w3; t = mulhi64((w1 << 32) | w0, Q); yhat = min{k : pre_k > t}, so a class
 * with q_k = 0 is never drawn.  A row with Q = 0 gets label -1 and the row -p_i.  Sampling the rows [a, b) of a block
 * with example_offset = a gives the rows [a, b) of the draw of the whole block.  A null probs / U, n < 1, S < 1, K < 1,
 * K > 8192, example_offset < 0 or example_offset + n > 2^32 returns LIP_ERR_ARG and writes nothing. */
int lip_head_sample(const float* probs, int32_t n, int32_t K, int32_t S, uint64_t seed, int64_t example_offset, float* U,
                    int32_t* labels, void* stream);
/* Layer-wise evidence of the structured posteriors: for every prior group g < G, with alpha_g = exp(log_alphas[g]),
 *   out[g][0] = L_g = sum_x log1p(r x / alpha_g),   out[g][1] = T_g = sum_x (r x / alpha_g) / (1 + r x / alpha_g),
 * x over the curvature eigenvalues of the group; out (G, 2) float64 is overwritten.  The eigenvalues are named by a
 * segment table over one float64 value pool vals (n_vals) on the device and are never written out:
 *   LIP_EV_KRON: x = scale * max(lam_i, 0) * max(mu_j, 0), lam = vals[off .. off + rows), mu = vals[off + rows ..
 *                off + rows + cols): rows * cols terms, term t = i cols + j;
 *   LIP_EV_LIST: x = scale * max(vals[off + i], 0), i < rows (cols = 1).
 * A group may own any number of segments of either kind.  The caller cuts every segment, in table order, into chunks of
 * chunk_terms consecutive terms (the last one of a segment shorter): chunks[c] = (first term, segment), n_chunks of them;
 * group_ptr (G + 1) / group_chunks (n_chunks) list every group's chunks in the order in which their partial sums are
 * added.  segs, chunks, group_ptr, group_chunks and log_alphas are device arrays (log_alphas is read by the kernel, so
 * an optimiser loop launches without a host round trip); segs_host is the host copy of segs, which the entry point
 * checks before any launch.  One workgroup reduces one chunk in a fixed order (per-lane strided sums, the halving tree
 * of a 64-lane wave, waves in index order through LDS) and stores its pair to scratch (device, >=
 * lip_evidence_terms_scratch(n_chunks) doubles); a second launch adds each group's pairs in table order.  No atomics,
 * two launches whatever G is: bitwise reproducible and a function of the tables alone.  A term is
 * (scale * (r / alpha_g)) * (max(lam_i, 0) * max(mu_j, 0)): four roundings after exp.  A null pointer, n_vals, n_seg,
 * n_chunks, chunk_terms or G <= 0, chunk_terms > 2^30, a non-finite or negative r, a segment with an unknown kind, a
 * group outside [0, G), non-positive rows or cols (cols != 1 for a list, rows or cols >= 2^31 for a product), a
 * negative or non-finite scale or an end past the pool, an n_chunks other than what the segments cut into, or too small
 * a scratch returns LIP_ERR_ARG and leaves out untouched.  A device table that differs from the checked host copy
 * cannot make the kernels read outside vals, the tables or scratch: they answer it with NaN. */
#define LIP_EV_KRON 0
#define LIP_EV_LIST 1
typedef struct {
  int32_t kind, group;
  int64_t off, rows, cols;
  double scale;
} lip_ev_seg_t;
typedef struct {
  int64_t start;               /* first term of the chunk inside its segment */
  int32_t seg, reserved;
} lip_ev_chunk_t;
int lip_evidence_terms_scratch(int64_t n_chunks, int64_t* doubles);
int lip_evidence_terms(const double* vals, int64_t n_vals, const lip_ev_seg_t* segs_host, const lip_ev_seg_t* segs, int32_t n_seg,
                       const lip_ev_chunk_t* chunks, int64_t n_chunks, int64_t chunk_terms, const int64_t* group_ptr,
                       const int32_t* group_chunks, const double* log_alphas, int32_t G, double r, double* out,
                       double* scratch, int64_t scratch_doubles, void* stream);
/* Semidefinite Cholesky factors for lip_link_mc: for each of the n covariances cov (n, K, K) float64, K <= 64, a lower
 * factor L (n, K, K) float32 with L L^T = C, computed in float64.  Predictive covariances can be rank-deficient and
 * come from float32 sums, so the factor is defined for semidefinite input, column by column: with tol = 2^-20 max_i C_ii
 * and d_j = C_jj - sum_{k<j} L_jk^2, a column with d_j > tol gets L_jj = sqrt(d_j), L_ij = (C_ij - sum_{k<j} L_ik L_jk) /
 * L_jj (i > j); any other column is zero.  Only the lower triangle of C is read; the strict upper triangle of L is
 * written as zeros.  An example with a non-finite entry in its lower triangle or a C_ii < -tol is dead: flags[i] = 1 and
 * an all-zero L; live examples get flags[i] = 0.  L and flags are overwritten.  A null cov / L / flags, n < 1, K < 1 or
 * K > 64 returns LIP_ERR_ARG and writes nothing. */
int lip_link_chol(const double* cov, int32_t n, int32_t K, float* L, int32_t* flags, void* stream);
/* Monte-Carlo softmax link: the class probabilities of a Gaussian over the logits, integrated by S draws per example
 * without writing a draw.  Exactly one of var (n, K), marginal variances, K <= 8192, and L (n, K, K), a lower factor
 * (lip_link_chol), K <= 64, is non-null.  For example i < n, draw s < S and class k < K
 *   z_k = mean_k + sqrt(var_k) eps_k     or     z_k = mean_k + sum_{j<=k} L_kj eps_j,      p^s = softmax(z),
 *   probs[i] = (1/S) sum_s p^s  (n, K) float64,    mean_entropy[i] = (1/S) sum_s H(p^s)  (n,) float64, in nats,
 * mean_entropy when not null; both are overwritten.  The normals are defined by their bits, so a host can replay them:
 * Philox4x32-10 keyed by the two words of seed (the generator of lip_fill_normal) at the counter words (g, s, k >> 2,
 * 0x4C4E4B31), g = example_offset + i, gives w0..w3; the fourth word differs from lip_head_sample's 0xBB67AE85, so an
 * MC Fisher fit and an MC link with one seed share no stream.  (eps_{4j}, eps_{4j+1}) is the Box-Muller pair of (w0, w1)
 * and (eps_{4j+2}, eps_{4j+3}) that of (w2, w3), as in lip_fill_normal: u = ((w >> 8) + 0.5) 2^-24 in float32, rad =
 * sqrt(-2 ln u1) (__logf, __fsqrt_rn), the pair (rad cos, rad sin)(2 pi u2) (__sincosf).  mean, sqrt(var) and the draws
 * are float32; the softmax subtracts the row maximum and uses __expf; H = log sum - sum_k e_k x_k / sum.  The sums over
 * the draws run in float64 in an order that depends on (K, S) alone and end in one division by S: results repeat bit
 * for bit, and the rows [a, b) computed with example_offset = a equal the rows [a, b) of the whole call.  No atomics.
 * var_k = 0 or an all-zero L gives softmax(mean) for every draw, whatever S.  A row with a mean that is not finite in
 * float32, a negative or non-finite var, or a non-finite entry in the lower triangle of L is dead: flags[i] = 1, NaN
 * probabilities and entropy; it does not touch the other rows, which get flags[i] = 0.  A null mean / probs / flags, both
 * or neither of var and L, n < 1, S < 1 (as an int32_t: 2^31 and more included), K < 1, K over the cap of the form,
 * example_offset < 0 or example_offset + n > 2^32 returns LIP_ERR_ARG and writes nothing. */
int lip_link_mc(const double* mean, const double* var, const float* L, int32_t n, int32_t K, int32_t S, uint64_t seed,
                int64_t example_offset, double* probs, double* mean_entropy, int32_t* flags, void* stream);
/* Measurement only: the largest K at which the variance form of lip_link_mc runs a whole draw per lane instead of one
 * per group of lanes (0..64; negative: leave it).  Returns the previous value.  Results are a function of the setting. */
int lip_debug_link_lane_max_k(int32_t K);

#ifdef __cplusplus
}
#endif
#endif /* LIP_H */
