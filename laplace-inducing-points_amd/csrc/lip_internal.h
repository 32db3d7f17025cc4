// Internal (non-ABI) declarations shared by the HIP translation units of liblip_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include "lip.h"
#include "lip_bindcache.h"

namespace lip {

// ---- division by a run-time constant without the ~40-instruction software divide --------------
// q = (umulhi(n, m) + n) >> s  (round-up magic number; exact for 0 <= n < 2^31, d >= 1)
struct FastDiv {
  unsigned m, s, d;
  FastDiv() : m(1), s(0), d(1) {}
  explicit FastDiv(unsigned dd) : d(dd) {
    s = 0;
    while ((1ull << s) < dd) ++s;
    m = (unsigned)((((1ull << s) - dd) << 32) / dd + 1);
  }
  __host__ __device__ __forceinline__ int div(int n) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)((__umulhi((unsigned)n, m) + (unsigned)n) >> s);
#else
    return (int)((unsigned)n / d);
#endif
  }
};

// ---- resolved (device-pointer) parameter blocks handed to the kernels -------------------
struct SegP {
  const float* a; long long a_ps;
  const float* b; long long b_ps;
  int IH, IW, C, KH, KW, stride, pad_h, pad_w, mode, Ktot;
  int b_trans;                          // LIP_SEG_B_TRANS (generic kernel only)
  FastDiv dC, dKW;
  // branch-free gather coordinate (fast kernel; stride in {1, 2}):
  //   t0 = o * mul + sgn * k + off ;  valid iff (t0 & mask) == 0 && 0 <= (t0 >> sh) < lim
  int mul, sgn, off_h, off_w, mask, sh;
};

struct IgemmP {
  int nseg;
  SegP seg[3];
  int R, OHW, OW, N;
  FastDiv dOHW, dOW;
  float* out; long long out_ps;
  const float* scale;
  const float* e0; long long e0_ps;
  const float* e1; long long e1_ps;
  const float* xhat;
  const float* res; long long res_ps;
  const float* dphi;
  float* red0; long long red0_ps;
  float* red1; long long red1_ps;
  const float* xhat2;
  const float* zeros;                   // >= 16 floats of device zeros (masked gather rows)
  unsigned long long* dbg;              // diagnostic s_memtime stamps (null in every real run)
  // split-K launches (few probes, under-filled grids): block z of gridDim.z accumulates its share of the K-tiles and
  // stores the raw sums to partial + z * partial_zs + p * R * N; igemm_finish_kernel adds the shares and runs the epilogue
  float* partial; long long partial_zs;
  int no_ksplit;                        // outputs of the primal tape: ReLU gates / pooling arg-maxima are taken from these sums,
                                        // so their summation order stays the one-block order whatever the launch geometry
  // parity-class row order of a stride-2 data gradient (fast kernel, OH and OW even): the rows of one block all
  // share (oh & 1, ow & 1), so the taps whose parity cannot match are skipped instead of gathered as zeros
  int Rc, OHW2, OW2;                    // rows per class n*(OH/2)*(OW/2), (OH/2)*(OW/2), OW/2
  FastDiv dOHW2, dOW2;
};

struct WgradP {
  const float* a;                       // primal activations [n][IH][IW][C]
  int IH, IW, C, KH, KW, stride, pad_h, pad_w;
  const float* g; long long g_ps;       // cotangent [P][R][N]
  int R, OHW, OW, N, M;                 // M = KH*KW*C
  FastDiv dOHW, dOW;
  float* y; long long y_ps;             // Y + param offset, element [m*N + co]
  const float* scale;                   // per-channel [N] or null
  int ksplit;
  const float* zeros;
  int P;                                // probe-batched variant: probes in this launch (columns = P*N)
  // per-example rows (lip_vjp_rows): grid.z = example, the row reduction of block z covers only that example's
  // seg_rows = OH*OW rows and lands in Y row (p, z): y + p*y_ps + z*seg_ys
  int seg_rows; long long seg_ys;
  // fused output of a weight gradient whose launch reduces all R rows in one block (no row split):
  //   overwrite == 1:  y = s * acc + alpha * v     (v = the probe's own slice of V at the same offset, or null)
  // instead of y += s * acc on a block the caller initialised with alpha * V — the initialisation pass over these
  // parameters is then skipped (lip_ggn_vp).  Set by the engine only for the ops whose range its initialisation skipped,
  // which it decides with wgrad_will_overwrite().
  int overwrite; const float* v; long long v_ps; float alpha;
  int sk_mg0, sk_tiles, sk_tn0;         // wgrad_skinny_kernel: first m-group of the launch, column tiles per probe it walks, first of them
};

struct ReduceP {
  const float* g; long long g_ps; int R, N;
  const float* xhat;
  float* red0; long long red0_ps;
  float* red1; long long red1_ps;
  // per-example rows: nseg > 0 -> grid.z = example, R rows per example, outputs at + z*red_seg
  int nseg; long long red_seg;
  int rpb;                              // rows per block: set by launch_reduce
};

struct PoolP {
  const float* in; long long in_ps;     // fwd: [P][n][HW][C]   bwd: [P][n][C]
  float* out; long long out_ps;         // fwd: [P][n][C]       bwd: [P][n][HW][C]
  int n, HW, C; float inv;
  const float* dphi;                    // bwd: [n][HW][C] or null
  const float* xhat;                    // bwd: for red1
  float* red0; long long red0_ps;
  float* red1; long long red1_ps;
};

struct MaxPoolP {
  const float* in; long long in_ps;     // [P][n][IH][IW][C]   (bwd: cotangent of the pooled tensor [P][n][OH][OW][C])
  float* out; long long out_ps;         // [P][n][OH][OW][C]   (bwd: [P][n][IH][IW][C])
  float* amax_w; const float* amax;     // [n][OH][OW][C] argmax as linear pixel index ih*IW+iw (float)
  int n, IH, IW, OH, OW, C, KH, KW, stride, pad_h, pad_w;
  const float* dphi; const float* xhat;
  float* red0; long long red0_ps;
  float* red1; long long red1_ps;
};

struct PrimalPostP {
  const float* z; float* a; float* dphi; float* xhat;   // all [R][N]
  const float* bias;                    // [N] or null          (THETA)
  const float* gamma; const float* beta;                 // BN   (THETA) or null
  const float* mean; const float* rstd;                  // BN   (CONST)
  const float* res;                     // [R][N] or null
  long long count; int N; int act;
};

struct HeadP {
  const float* in; long long in_ps;     // [P][n][K]
  float* out; long long out_ps;         // [P][n][K]
  const float* p; const float* s;       // softmax probs / sqrt [n][K]
  int n, K, mode, classifier; float c;
};

// ---- MAP training (lip_train.hip) ---------------------------------------------------------------------------------------
struct BnStatsP {
  const float* z; int R, N;             // raw conv output [R][N]
  const float* bias; const float* gamma;                 // conv bias / BN scale (THETA) or null
  float eps, momentum;
  float* mean; float* var; float* rstd; float* s;        // per channel; any may be null
  float* run_mean; float* run_var;      // running averages, updated in place; or null
  double* scratch;                      // >= bn_stats_scratch(R, N) doubles, 16-byte aligned
};

struct BnTrainBwdP {
  const float* g; long long g_ps;       // cotangent of the BN output [P][R][N]
  const float* xhat;                    // [R][N] primal
  const float* dbeta; const float* dgamma; long long d_ps;   // the reduced BN cotangents, per probe
  float* out; long long out_ps;         // corrected cotangent [P][R][N], not g
  int R, N;
};

// ---- code path of the non-GEMM kernels that pick one from the channel count and the pointer alignment ----------
// One predicate per kernel, used by the kernel (per block, on the block's own pointers) and by its launcher (per probe,
// for the route census), so a census label cannot drift from the branch that ran.
enum SmallPath { SP_QUAD = 0, SP_QUAD_WIDE = 1, SP_FIXED = 2, SP_ATOMIC = 3, SP_MIXED = 4 };

__host__ __device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
// reduce_kernel: g, xh are the first row of the block (xh may be null)
__host__ __device__ __forceinline__ int reduce_path(int N, const float* g, const float* xh) {
  if ((N & 3) == 0 && aligned16(g, xh)) return (N >> 2) <= 256 ? SP_QUAD : SP_QUAD_WIDE;
  return (N <= 256 && (256 % N) == 0) ? SP_FIXED : SP_ATOMIC;
}
// pool_fwd_kernel: in is the first pixel of the (probe, example) map
__host__ __device__ __forceinline__ int pool_fwd_path(int C, const float* in) {
  if (C <= 256 && (256 % C) == 0) return SP_FIXED;
  return ((C & 3) == 0 && aligned16(in)) ? SP_QUAD : SP_ATOMIC;
}
// pool_bwd_kernel: in / out / dphi / xhat at the block's first element (dphi, xhat may be null)
__host__ __device__ __forceinline__ int pool_bwd_path(int C, const float* in, const float* out, const float* dphi, const float* xhat) {
  if ((256 % C) == 0) return SP_FIXED;
  return ((C & 3) == 0 && aligned16(in, out, dphi, xhat)) ? SP_QUAD : SP_ATOMIC;
}
// head_kernel: plain scaling (regressor, or the OUT / IN modes) against the softmax factor actions
__host__ __device__ __forceinline__ bool head_scales(int classifier, int mode) {
  return !classifier || mode == LIP_HEAD_OUT || mode == LIP_HEAD_IN;
}

// ---- the arithmetic route of a call ---------------------------------------------------------------------------------------
// The four process-wide modes with setters (lip_set_precision / lip_set_winograd / lip_set_wino_walk / lip_set_split_k),
// as ONE value.  An entry point takes current_route() once, before its first launch, and hands that value to every
// predicate and launcher of the call: a setter takes effect at the next entry-point call, and a call in flight, on this or
// another thread, keeps the route it started with.
struct Route {
  int precision;   // 0: exact f32 MFMA; 1: split-precision bf16x3 operands
  int wino;        // Winograd route of the 3x3 / stride-1 layers: 0 off, 1 on, 2 on (same launches as 1)
  int walk;        // probes per block of igemm_wino_kernel: 0 = the rule wino_walk_plan(), or 1 / 2 / 4 forced
  bool split_k;    // split-K of under-filled implicit GEMMs
};
Route current_route();     // the only function that reads the four process-wide modes

// ---- launchers (return hipError_t of the launch) ------------------------------------------
// route: the call's route (above).  cache: the engine's cache of binding-fixed Winograd transforms, or null (per-launch transforms).  launch_igemm takes
// the transformed weights of segment s from it when bit s of fixed_b is set (the engine sets it where the segment's
// shared B operand lives in THETA / CONST); launch_wgrad is handed a cache only when p.a lives in PRIM / CONST.  The
// cache never changes the route of a launch, only where the Winograd kernels' transformed operand comes from.
hipError_t launch_igemm(const IgemmP& p, int P, hipStream_t st, const Route& route, BindCache* cache = nullptr, unsigned fixed_b = 0);
// An op with p.overwrite set whose fused launch cannot be made for want of scratch (a 17th (device, stream) pair, a failed
// allocation) has its block of Y initialised here (alpha * v, or 0) and then takes the accumulating direct kernels.
hipError_t launch_wgrad(const WgradP& p, int P, hipStream_t st, const Route& route, BindCache* cache = nullptr);
// a cache with the device allocator and the per-engine cap of bind_cache_policy(), or null when the policy is off
BindCache* new_bind_cache();
hipError_t launch_reduce(const ReduceP& p, int P, hipStream_t st);
hipError_t launch_pool_fwd(const PoolP& p, int P, hipStream_t st);
hipError_t launch_pool_bwd(const PoolP& p, int P, hipStream_t st);
hipError_t launch_primal_post(const PrimalPostP& p, hipStream_t st);
hipError_t launch_maxpool_primal(const MaxPoolP& p, hipStream_t st);
hipError_t launch_maxpool_fwd(const MaxPoolP& p, int P, hipStream_t st);
hipError_t launch_maxpool_bwd(const MaxPoolP& p, int P, hipStream_t st);
hipError_t launch_softmax(const float* logits, float* prob, float* sqrtp, int n, int K, hipStream_t st);
hipError_t launch_head(const HeadP& p, int P, hipStream_t st);
// MAP training: batch statistics of a BN unit (two launches: chunk partials, fold), the train-mode correction of its
// cotangent, and one transposed, BN-scaled kernel Wt[t][co][ci] = W[t][ci][co] s[co] (s null: no scale)
long long bn_stats_scratch(int R, int N);
hipError_t launch_bn_stats(const BnStatsP& p, hipStream_t st);
hipError_t launch_bn_train_bwd(const BnTrainBwdP& p, int P, hipStream_t st);
hipError_t launch_wt_refresh(const float* W, const float* s, float* Wt, int taps, int cin, int cout, hipStream_t st);
hipError_t launch_gemm_nt(const float* A, long long lda, int m, const float* B, long long ldb, int n, long long K, float* C,
                          hipStream_t st);
hipError_t launch_gemm_nn_axpy(const float* T, long long ldt, int m, int k, const float* B, long long ldb, long long N,
                               const float* V, long long ldv, float beta, float* Out, long long ldo, hipStream_t st);
hipError_t launch_scale_copy(float* y, const float* x, float a, long long count, hipStream_t st);
// y[p][off + i] = a * x[p][off + i] (x null: 0) for i < len, p < P, row stride ld: the parameters a fused weight gradient
// does NOT write (biases, BN parameters, layers on the accumulate path)
hipError_t launch_scale_copy_range(float* y, const float* x, float a, long long off, long long len, int P, long long ld, hipStream_t st);
// y[p][j] += a[j] * x[p][j], p < P, j < N (rows of N floats): the vector-prior term of lip_ggn_vp_diag
hipError_t launch_add_diag(float* y, const float* x, const float* a, int P, long long N, hipStream_t st);
// true when launch_wgrad(p, P, st, route) takes the one-block-per-tile kernel that honours WgradP::overwrite
bool wgrad_will_overwrite(const WgradP& p, int P, const Route& route);

// ---- square-accumulating reductions of lip_vjp_sqsum ----------------------------------------
// y[j] += sum_{p < P} sum_{i < n} (per-(probe, example) partial product)_j^2, no (P, n, .) intermediate and no float
// atomics: a block owns one output tile and a fixed group of (probe, example) pairs and writes one partial per group;
// sqsum_finish adds the partials to y in group order.  A launch of one group adds into y directly.
// Scratch: the caller's, `*_sqsum_scratch` floats (0 when the launch needs none); bounded by the target grid
// (SQ_TARGET_BLOCKS), independent of n and of the probe count.
constexpr int SQ_TARGET_BLOCKS = 512;                  // 2 blocks per CU on the 256 CUs of an MI355X

// The pair walk shared by the per-pair kernels (wgrad_sqsum / wgrad_wnorm tiles, reduce_sqsum / reduce_wnorm): pair
// q = p * n_img + i; the blocks of group g (blockIdx.y) take pairs [g * per, min(pairs, (g + 1) * per)) in order.
struct PairGroupP {
  int pairs, per, n_img;
};
// Groups of a launch with `blocks_per_group` blocks per group, enough of them to fill SQ_TARGET_BLOCKS.
// bound = min(pairs, ceil(SQ_TARGET_BLOCKS / blocks_per_group)) is monotone in `pairs`, so a scratch sized with it for the
// largest pass serves every smaller one; the launch's G <= bound after rounding to whole groups of `per` pairs.
struct PairGroups {
  long long bound;
  int G, per;
};
inline PairGroups pair_groups(long long blocks_per_group, long long pairs) {
  PairGroups r;
  r.bound = (SQ_TARGET_BLOCKS + blocks_per_group - 1) / blocks_per_group;
  if (r.bound > pairs) r.bound = pairs;
  if (r.bound < 1) r.bound = 1;
  r.per = (int)((pairs + r.bound - 1) / r.bound);
  r.G = (int)((pairs + r.per - 1) / r.per);
  return r;
}
// The argument checks of the four per-pair launchers: P > 0 probes of n_img > 0 examples with `rows` > 0 rows each,
// fewer than 2^31 pairs; a weight gradient also passes its row total R, which the examples must make up (a reduce is
// given its rows per segment and has no total to check); and a scratch of `need` floats is there when need > 0.
inline bool pair_launch_ok(int P, int n_img, long long rows) {
  return P > 0 && n_img > 0 && rows > 0 && (long long)P * n_img < (1ll << 31);
}
inline bool pair_launch_ok(int P, int n_img, long long rows, long long R) {
  return pair_launch_ok(P, n_img, rows) && rows * n_img == R;
}
inline bool scratch_fits(long long need, const float* scratch, long long scratch_floats) {
  return need <= scratch_floats && (need == 0 || scratch);
}
// fills `pg` for a checked launch of `blocks_per_group` blocks per group and returns its number of groups G
inline int pair_launch_groups(PairGroupP& pg, long long blocks_per_group, int P, int n_img) {
  const PairGroups g = pair_groups(blocks_per_group, (long long)P * n_img);
  pg.pairs = P * n_img; pg.per = g.per; pg.n_img = n_img;
  return g.G;
}

// weight gradient (p as built for the per-example rows, p.seg_rows = OH*OW): the MFMA kernel per (probe, example)
// tile, or, when OH*OW == 1, the rank-1 route  y[m][c] += sum_i a_i[m]^2 sum_p (s[c] g_pi[c])^2
long long wgrad_sqsum_scratch(int M, int N, int OHW, long long pairs);
hipError_t launch_wgrad_sqsum(const WgradP& p, int P, int n_img, float* scratch, long long scratch_floats, hipStream_t st);
// bias / BN cotangents: p.R rows per (probe, example) segment, p.nseg = n; red0 / red1 point into the (D,) output
long long reduce_sqsum_scratch(int N, long long pairs);
hipError_t launch_reduce_sqsum(const ReduceP& p, int P, float* scratch, long long scratch_floats, hipStream_t st);
// y[j] += sum_{g < G} partial[g * len + j], g ascending
hipError_t launch_sqsum_finish(const float* partial, int G, long long len, float* y, hipStream_t st);

// ---- weighted square norms of lip_vjp_wnorm --------------------------------------------------
// out[p * n + i] += sum_j w_j (per-(probe, example) partial product)_j^2: the same per-pair tiles and segmented sums as
// the square-accumulating reductions above, reduced over the parameters instead of over the pairs.  Every launch
// writes one float per (output tile, pair) to scratch[tile * pairs + pair] (plain stores) and wnorm_finish adds the
// tiles of a pair, in tile order, into out: no float atomics.  w: the op's slice of the weight vector in the layout of
// the op's output (null: all ones).  Scratch floats of a launch: `*_wnorm_tiles` x pairs.
long long wgrad_wnorm_tiles(int M, int N, int OHW);
hipError_t launch_wgrad_wnorm(const WgradP& p, int P, int n_img, const float* w, float* out, float* scratch,
                              long long scratch_floats, hipStream_t st);
// p.red0 / p.red1: which reductions the op has and (unless `ones`) their (N,) weight slices — read, never written
long long reduce_wnorm_tiles(int N);
hipError_t launch_reduce_wnorm(const ReduceP& p, int P, bool ones, float* out, float* scratch, long long scratch_floats,
                               hipStream_t st);
hipError_t launch_wnorm_finish(const float* partial, int T, long long pairs, float* out, hipStream_t st);
// launch census of these kernels (lip_debug_wnorm_routes), kept apart from the route census below
enum WnormRoute { WN_WGRAD_2212 = 0, WN_WGRAD_2222, WN_WGRAD_2211, WN_WGRAD_4112, WN_WGRAD_2111, WN_WGRAD_4111,
                  WN_WGRAD_DENSE, WN_REDUCE, WN_FINISH, WN_ROUTES };
void wnorm_route_hit(int id);
int wnorm_routes_read(int64_t* counts, int n, const char** names);

// ---- route census (lip_debug_routes): one host-side counter per launch route -----------------
// A route is one kernel instantiation as launched, with the flags that picked it, e.g. "igemm_fast<4,1,1,2>/par/bv4".
// route_id() formats the name and returns its slot (the table of known routes in lip_mfma.hip, or a new slot appended
// after it); LIP_ROUTE caches the slot per launch site and adds one with a relaxed atomic.  No GPU work.
int route_id(const char* fmt, ...);
void route_hit(int id);
int route_count();
// copies min(n, route_count()) counts and names (names stay valid for the life of the process), then clears the counts
int routes_read(int64_t* counts, int n, const char** names);
#define LIP_ROUTE(...)                                                  \
  do {                                                                  \
    static const int lip_route_slot_ = ::lip::route_id(__VA_ARGS__);    \
    ::lip::route_hit(lip_route_slot_);                                  \
  } while (0)

// a launch site whose name depends on a run-time key in [0, nkeys): one cached slot per key
#define LIP_ROUTE_KEYED(key, nkeys, ...)                                \
  do {                                                                  \
    static std::atomic<int> lip_route_slots_[nkeys];                    \
    int lip_slot_ = lip_route_slots_[key].load(std::memory_order_relaxed) - 1;             \
    if (lip_slot_ < 0) { lip_slot_ = ::lip::route_id(__VA_ARGS__); lip_route_slots_[key].store(lip_slot_ + 1, std::memory_order_relaxed); } \
    ::lip::route_hit(lip_slot_);                                        \
  } while (0)
// "<kernel>/quad | quad_wide | fixed | atomic | mixed" from a SmallPath (mixed: the probes of one launch differ)
#define LIP_ROUTE_PATH(kernel, path)                                    \
  do {                                                                  \
    static const char* const lip_pn_[5] = {"quad", "quad_wide", "fixed", "atomic", "mixed"};  \
    LIP_ROUTE_KEYED(path, 5, kernel "/%s", lip_pn_[path]);              \
  } while (0)

// ---- environment switches ----------------------------------------------------------------------
// Every LIP_* variable the library reads, one field each.  switches() reads them all on its first call and never again:
// "once per process" is a contract (tests/test_ab_switches.py starts one child process per setting because of it).
// Unless a field says otherwise it is true when the variable is set to anything.  All but the first four are A/B switches.
struct Switches {
  bool precision_x3;   // LIP_PRECISION: first letter b or 1 -> the precision mode starts as 1 (bf16x3 operands), else 0 (exact f32)
  bool noksplit;       // LIP_NOKSPLIT: split-K of under-filled implicit GEMMs starts off
  bool nowino;         // LIP_NOWINO: the Winograd mode starts as 0 (off); overrides LIP_WINO
  bool wino_f;         // LIP_WINO: first letter f -> the Winograd mode starts as 2, else 1
  bool generic;        // LIP_GENERIC: igemm / wgrad instead of every specialised direct kernel (the Winograd test precedes it)
  bool nofirst;        // LIP_NOFIRST: no first-layer kernels (igemm_first, wgrad_first)
  bool noskinny;       // LIP_NOSKINNY: no wgrad_skinny on the dense layers
  bool nopb;           // LIP_NOPB: no probe-batched weight gradient (wgrad_pb)
  bool nopb96;         // LIP_NOPB96: no 96-row probe-batched tile for N = 64, M = 576
  bool wgrad3;         // LIP_WGRAD3: the three-wave wgrad_pb<3,1,1,4> also in f32 mode
  bool nopar;          // LIP_NOPAR: plain row order for even-grid stride-2 data gradients
  bool nobv4;          // LIP_NOBV4: dword instead of dwordx4 B / cotangent loads (igemm_fast, igemm_adirect, wgrad_fast)
  bool noadirect;      // LIP_NOADIRECT: igemm_fast<4,1,*,*> instead of igemm_adirect
  bool wino_novepi;    // LIP_WINO_NOVEPI: the scalar Winograd epilogue on aligned operands
  bool nosmallp;       // LIP_NOSMALLP: the 128-row tiles also at few probes
  int smallp_factor;   // LIP_SMALLP_FACTOR: few probes = fewer 128-row blocks than this many per CU (default 2)
  int wgw_minblocks;   // LIP_WGW_MINBLOCKS: fewest (probe, c tile, n tile) blocks that take wgrad_wino (default 2)
  int tile;            // LIP_TILE: experiment tiles of launch_igemm, 1..4 (default -1: none)
  bool dbg;            // LIP_DBG: cycle stamps of igemm_fast, reported on stderr after a stream synchronisation (never timed)
  bool dot_nt_valu;    // LIP_DOT_NT_VALU: the VALU / LDS kernel of lip_dot_nt_f64
  bool dot_nt_noquad;  // LIP_DOT_NT_NOQUAD: lip_dot_nt_f64 with one tile per block, the waves splitting K
};
const Switches& switches();
// LIP_WGW_NOSTAGE: wgrad_wino/rowq fetches the cotangent per wave, without the block's LDS stage.  It picks an
// instantiation, not a route (the name stays wgrad_wino/rowq), so it is read here, as lip_bindcache.h reads its policy;
// its A/B test is tests/test_wgrad_wino_stage.py, which starts one child process per setting.
inline bool wgw_nostage() {
  static const bool off = getenv("LIP_WGW_NOSTAGE") != nullptr;
  return off;
}

// ---- one record per (device, stream) ---------------------------------------------------------------
// with(st, f) finds or creates the record of (current device, st) and returns f(record), run under the table's lock.
// It returns a value-initialised result (a null pointer) when hipGetDevice fails or all CAP records belong to other
// (device, stream) pairs; records live for the life of the process.
template <class Rec, int CAP = 16>
class PerStream {
  struct Slot { int dev; hipStream_t st; Rec rec; };
  Slot slots_[CAP];
  int used_ = 0;
  std::mutex mu_;
 public:
  template <class F> auto with(hipStream_t st, F&& f) -> decltype(f(std::declval<Rec&>())) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return {};
    std::lock_guard<std::mutex> lock(mu_);
    for (int i = 0; i < used_; ++i)
      if (slots_[i].dev == dev && slots_[i].st == st) return f(slots_[i].rec);
    if (used_ == CAP) return {};
    Slot& s = slots_[used_++];
    s.dev = dev; s.st = st; s.rec = Rec();
    return f(s.rec);
  }
};

// f(std::true_type()) or f(std::false_type()): a run-time flag as a template argument.  LIP_ROUTE inside a generic
// lambda caches one slot per instantiation, so a name formatted from the flag types is the route of the kernel launched.
template <class F> auto with_flag(bool on, F&& f) {
  if (on) return f(std::true_type());
  return f(std::false_type());
}

void set_error(const char* fmt, ...);
// a failed HIP runtime call inside an entry point (code that is `using namespace lip`): record it, return LIP_ERR_HIP
#define LIP_CHECK_HIP(expr)                                                        \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) { set_error("%s: %s", #expr, hipGetErrorString(_e)); return LIP_ERR_HIP; } \
  } while (0)
// the setters of the four modes of a Route (read back by current_route() alone)
void set_precision_mode(int m);
void set_split_k_mode(int on);
void set_wino_mode(int m);
void set_wino_walk(int w);
int wino_walk_plan(long long gx, int P);

// ---- wave / block reductions (wave = 64 lanes on gfx950) --------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- counter-based RNG: Philox4x32-10 on four counter words, key = the two words of the seed --------------------
__device__ __forceinline__ void philox4x32(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                           unsigned long long key, unsigned int (&out)[4]) {
  unsigned int k0 = (unsigned int)key, k1 = (unsigned int)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long m0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long m1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned int n0 = (unsigned int)(m1 >> 32) ^ c1 ^ k0;
    const unsigned int n1 = (unsigned int)m1;
    const unsigned int n2 = (unsigned int)(m0 >> 32) ^ c3 ^ k1;
    const unsigned int n3 = (unsigned int)m0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the fills and the head sampler: a 64-bit counter in words 0 and 1, two constants in words 2 and 3
__device__ __forceinline__ void philox4x32(unsigned long long ctr, unsigned long long key, unsigned int (&out)[4]) {
  philox4x32((unsigned int)ctr, (unsigned int)(ctr >> 32), 0x9E3779B9u, 0xBB67AE85u, key, out);
}

// Box-Muller on one pair of Philox words: u = ((w >> 8) + 0.5) 2^-24, (a, b) = sqrt(-2 ln u1) (cos, sin)(2 pi u2).
// Hardware transcendentals (v_log_f32 / v_sin_f32 / v_cos_f32, ~1e-6 relative): the library versions made the normal
// fill ALU-bound at 3.8 TB/s; u1 >= 2^-25, so the logarithm stays far from its denormal range
__device__ __forceinline__ void box_muller_pair(unsigned int w1, unsigned int w2, float& a, float& b) {
  const float u1 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(w2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float rad = __fsqrt_rn(-2.0f * __logf(u1));
  float sn, cs;
  __sincosf(6.283185307179586f * u2, &sn, &cs);
  a = rad * cs; b = rad * sn;
}

}  // namespace lip
