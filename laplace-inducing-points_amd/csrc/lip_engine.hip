// Op-tape interpreter + C ABI of the linearised-network engine (see include/lip.h).
//
// The Python host compiles a NetSpec into three tapes of lip_op_t (primal, tangent-forward,
// backward).  The engine resolves operand references against the bound device buffers and
// launches the HIP kernels on the caller's stream, chunking the probe dimension so that the
// tangent workspace fits the budget the caller allocated.  No allocation, no synchronisation
// and no host<->device copy happens inside a run (hipGraph-capturable).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "lip_internal.h"
#include "lip_gramtile.h"

namespace lip {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace lip

using namespace lip;

struct lip_engine {
  int64_t D = 0;
  int32_t n_img = 0, K = 0;
  std::vector<lip_op_t> tape[5];         // LIP_TAPE_*: primal, tangent, backward; train primal, train backward
  const float* theta = nullptr;
  const float* consts = nullptr;
  // MAP training (lip_engine_train_bind / lip_engine_set_refresh): the writable view of consts, the float64 scratch of the
  // batch statistics, the table of transposed kernels, and whether PRIM holds a train primal pass
  float* consts_rw = nullptr;
  double* train_scratch = nullptr;
  int64_t train_scratch_doubles = 0;
  struct Refresh { int64_t w_off, wt_off, s_off; int taps, cin, cout; };
  std::vector<Refresh> refresh;
  bool train_primal_done = false;
  float* prim = nullptr;
  float* work = nullptr;
  int64_t work_pp = 0;      // workspace floats per probe
  int32_t max_chunk = 0;    // probes per chunk
  bool primal_done = false;
  // optional per-op timing (HIP events recorded on the launch stream); a run records into it through its const engine
  bool prof = false;
  mutable std::vector<hipEvent_t> ev_pool;
  mutable size_t ev_used = 0;
  mutable std::vector<int> ev_kind;   // kind of the op bracketed by events (2i, 2i+1)
  // Winograd transforms of the binding's shared kernels and primal activations (lip_bindcache.h): filled lazily by the
  // sweeps' launches, stale after a primal pass, freed on re-binding and destruction; null with LIP_NOBINDCACHE
  BindCache* cache = new_bind_cache();
  // lip_vjp_kron: doubles before the (N, N) block of backward op i in its output (WGRAD ops, in tape order), and the
  // total; filled when the backward tape is set
  std::vector<int64_t> kron_off;
  int64_t kron_total = 0;
  // lip_vjp_eigen: the number of WGRAD ops before backward op i (the index of its block in the call's host arrays)
  std::vector<int> wgrad_index;
  ~lip_engine() { delete cache; }
};

namespace {

// What a backward sweep does with the parameter cotangents (weight gradients, bias / BN reductions) it forms
enum class Sweep {
  SUMMED,   // lip_ggn_vp / lip_vjp: summed over the examples into the (P, D) block Y
  ROWS,     // lip_vjp_rows: Y holds one row per (probe, example); no reduction crosses examples
  SQSUM,    // lip_vjp_sqsum: formed per (probe, example) as in ROWS, squared and summed into ONE (D,) vector Y
  WNORM,    // lip_vjp_wnorm: formed per (probe, example); Y is the (D,) WEIGHT vector, read only, and the weighted square
            // norm of every cotangent is added to wout[p * n + i]
  KRON,     // lip_vjp_kron: no parameter cotangent is formed; every WGRAD op Gram-multiplies the rows of its cotangent
            // operand into its (N, N) float64 block of kron (the output factors of a Kronecker-factored curvature)
  EIGEN,    // lip_vjp_eigen: no parameter cotangent is formed; every WGRAD op projects its activation patches with the
            // block's V and its cotangent rows with the block's Ub, and the per-(probe, example) products of the projected
            // pair are squared and summed into the block's (Mt, N) float64 Lam (the second moments EKFAC needs)
  EWNORM,   // lip_vjp_eigen_wnorm: the projections of EIGEN, then the other reduction of the per-(probe, example) products:
            // squared, weighted by the block's (Mt, N) float32 Rw and added to wout[p * n + i]; no parameter cotangent of a
            // block tensor is formed.  The reductions (bias / BN cotangents) run as in WNORM against the weight vector Y,
            // or not at all when Y is null
};

// The operands of one WGRAD op in an EIGEN / EWNORM sweep: the block's bases, its output (EIGEN) or its weights (EWNORM),
// and its rows Mt = KH KW C (+ 1: a bias row)
struct EigenBlock {
  const double* V;
  const double* Ub;
  double* Lam;
  int Mt;
  const float* Rw = nullptr;
};

// The overwrite plan of one pass of a summed product (lip_ggn_vp / lip_vjp): the parameter ranges of Y, ascending, that
// init_output left unwritten because a fused weight gradient of the backward tape writes them outright.  Made once per
// pass; make_wgrad sets overwrite for exactly the ops whose range is in it, so the two cannot disagree.
struct SkipRange { int64_t off, len; };
using OverwritePlan = std::vector<SkipRange>;
inline bool planned(const OverwritePlan& plan, int64_t off) {
  const auto it = std::lower_bound(plan.begin(), plan.end(), off, [](const SkipRange& r, int64_t o) { return r.off < o; });
  return it != plan.end() && it->off == off;
}

struct RunCtx {
  const lip_engine* e;
  const float* V;   // chunk-shifted
  float* Y;
  float* H;         // HEAD space, chunk-shifted
  int P;            // probes in this chunk
  int head_mode;
  float head_c;
  Route route;      // taken once per entry-point call (current_route()), before its first pass
  hipStream_t st;
  Sweep mode = Sweep::SUMMED;
  float* scratch = nullptr;       // SQSUM / WNORM: the square-accumulating kernels' scratch
  long long scratch_floats = 0;
  bool wones = false;             // WNORM: every weight is 1 and Y is a placeholder of the right extent that is never read
  float* wout = nullptr;
  double* kron = nullptr;         // KRON: the (N, N) block of the op being run (run_tape shifts the output buffer per op)
  double* kron_scratch = nullptr; // ... and the partial tiles of one Gram
  long long kron_doubles = 0;
  const EigenBlock* eigen = nullptr;  // EIGEN / EWNORM: the blocks of the WGRAD ops in tape order (run_tape picks the op's), scratch as SQSUM's
  // summed products (lip_ggn_vp / lip_vjp): a weight gradient that reduces all rows in one block WRITES
  // y = s acc + alpha v instead of adding to an initialised block where the pass's plan says the initialisation skipped
  // its parameters; a context without a plan never overwrites
  const OverwritePlan* plan = nullptr;
  float alpha = 0.f;

  bool per_example() const { return mode != Sweep::SUMMED; }      // cotangents are taken per example
  // no parameter cotangent is formed (an EWNORM sweep without a weight vector launches no reduction either)
  bool no_params() const { return mode == Sweep::KRON || mode == Sweep::EIGEN || (mode == Sweep::EWNORM && !Y); }
};

// The kinds of sweep, from the operands of one pass (a plain RunCtx{..., route, st} is summed and not fused)
inline RunCtx fused_sum(RunCtx c, float alpha, const OverwritePlan* plan) { c.alpha = alpha; c.plan = plan; return c; }
inline RunCtx example_rows(RunCtx c) { c.mode = Sweep::ROWS; return c; }
inline RunCtx square_sum(RunCtx c, float* scratch, long long floats) {
  c.mode = Sweep::SQSUM; c.scratch = scratch; c.scratch_floats = floats;
  return c;
}
inline RunCtx weighted_norm(RunCtx c, float* scratch, long long floats, bool wones, float* wout) {
  c.mode = Sweep::WNORM; c.scratch = scratch; c.scratch_floats = floats; c.wones = wones; c.wout = wout;
  return c;
}

inline RunCtx kron_factors(RunCtx c, double* out, double* scratch, long long doubles) {
  c.mode = Sweep::KRON; c.kron = out; c.kron_scratch = scratch; c.kron_doubles = doubles;
  return c;
}
inline RunCtx eigen_moments(RunCtx c, const EigenBlock* blocks, float* scratch, long long floats) {
  c.mode = Sweep::EIGEN; c.eigen = blocks; c.scratch = scratch; c.scratch_floats = floats;
  return c;
}
inline RunCtx eigen_weighted_norm(RunCtx c, const EigenBlock* blocks, float* scratch, long long floats, float* wout) {
  c.mode = Sweep::EWNORM; c.eigen = blocks; c.scratch = scratch; c.scratch_floats = floats; c.wout = wout;
  return c;
}

// an operand the binding fixes between two primal passes: the weights / constants, or the primal tape's activations
inline bool bound_space(const lip_ref_t& r) { return (r.space == LIP_SP_THETA || r.space == LIP_SP_CONST || r.space == LIP_SP_PRIM) && r.pstride == 0; }

inline float* resolve(const RunCtx& c, const lip_ref_t& r) {
  switch (r.space) {
    case LIP_SP_THETA: return const_cast<float*>(c.e->theta) + r.off;
    case LIP_SP_CONST: return const_cast<float*>(c.e->consts) + r.off;
    case LIP_SP_PRIM: return c.e->prim + r.off;
    case LIP_SP_WORK: return c.e->work + r.off * (int64_t)c.e->max_chunk;
    case LIP_SP_VIN: return c.V ? const_cast<float*>(c.V) + r.off : nullptr;
    case LIP_SP_YOUT: return c.Y ? c.Y + r.off : nullptr;
    case LIP_SP_HEAD: return c.H ? c.H + r.off : nullptr;
    default: return nullptr;
  }
}

#define RUN_CHECK(expr, what)                                                                  \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(_e)); return LIP_ERR_HIP; } \
  } while (0)

constexpr int MAX_REDUCED_WIDTH = 8192;   // columns of a parameter reduction (bias / BN cotangents) the kernels take

// Scratch floats ONE backward op needs in a sweep over `pairs` (probe, example) pairs: lip_vjp_sqsum's are bounded by the
// target grid, lip_vjp_wnorm's are pairs x output tiles
long long wgrad_scratch(Sweep mode, int M, int N, int OHW, long long pairs) {
  return mode == Sweep::WNORM ? wgrad_wnorm_tiles(M, N, OHW) * pairs : mode == Sweep::SQSUM ? wgrad_sqsum_scratch(M, N, OHW, pairs) : 0;
}
long long reduce_scratch(Sweep mode, int N, long long pairs) {
  return mode == Sweep::WNORM || mode == Sweep::EWNORM ? reduce_wnorm_tiles(N) * pairs : mode == Sweep::SQSUM ? reduce_sqsum_scratch(N, pairs) : 0;
}

template <class Prm>
void resolve_reductions(const RunCtx& c, const lip_op_t& op, Prm& p) {
  p.red0 = resolve(c, op.red0); p.red0_ps = op.red0.pstride;
  p.red1 = resolve(c, op.red1); p.red1_ps = op.red1.pstride;
}

// per-example form of a reduction over [P][n][rows][N]: one output row per (probe, example) instead of one per probe
void per_example(ReduceP& r, int n_img, int rows) {
  r.R = rows; r.nseg = n_img; r.red_seg = r.red0 ? r.red0_ps : r.red1_ps;
  r.red0_ps *= n_img; r.red1_ps *= n_img;
}

// The parameter reductions of a filled ReduceP, as the sweep takes them: summed or per example (ROWS), squared into the
// (D,) output (SQSUM), or weighted into wout (WNORM)
int reduce_params(const RunCtx& c, const ReduceP& r, int n_img, const char* who) {
  if (!r.g || r.N <= 0 || r.N > MAX_REDUCED_WIDTH || (r.red1 && !r.xhat)) { set_error("%s: bad reduction operands", who); return LIP_ERR_ARG; }
  if (reduce_scratch(c.mode, r.N, (long long)c.P * n_img) > c.scratch_floats) { set_error("%s: reduction scratch too small", who); return LIP_ERR_ARG; }
  switch (c.mode) {
    case Sweep::WNORM:
    case Sweep::EWNORM: RUN_CHECK(launch_reduce_wnorm(r, c.P, c.wones, c.wout, c.scratch, c.scratch_floats, c.st), who); break;
    case Sweep::SQSUM: RUN_CHECK(launch_reduce_sqsum(r, c.P, c.scratch, c.scratch_floats, c.st), who); break;
    default: RUN_CHECK(launch_reduce(r, c.P, c.st), who);
  }
  return LIP_OK;
}

// Launch an op that fuses parameter reductions (column sums over ALL rows of a probe).  A per-example sweep launches it
// without them and takes them by a segmented reduce over the op's freshly written output [P][n][rows][N] instead.
template <class Prm, class Launch>
int launch_with_reductions(const RunCtx& c, Prm& p, Launch launch, const char* who, int n_img, int rows, int N, const float* xhat) {
  if (c.no_params()) { p.red0 = nullptr; p.red1 = nullptr; }
  if (!c.per_example() || (!p.red0 && !p.red1)) { RUN_CHECK(launch(p), who); return LIP_OK; }
  ReduceP r;
  memset(&r, 0, sizeof(r));
  r.g = p.out; r.g_ps = p.out_ps; r.N = N; r.xhat = xhat;
  r.red0 = p.red0; r.red0_ps = p.red0_ps; r.red1 = p.red1; r.red1_ps = p.red1_ps;
  per_example(r, n_img, rows);
  p.red0 = nullptr; p.red1 = nullptr;
  RUN_CHECK(launch(p), who);
  return reduce_params(c, r, n_img, who);
}

int check_space(const RunCtx& c, const lip_ref_t& r, const char* what) {
  if (r.space == LIP_SP_NONE) return LIP_OK;
  if (resolve(c, r) == nullptr) { set_error("op operand '%s' refers to an unbound space %d", what, r.space); return LIP_ERR_STATE; }
  return LIP_OK;
}

// resolved parameter block of a WGRAD op in this context (init_output makes it too, in a context that has no plan yet, to
// ask wgrad_will_overwrite about the op)
int make_wgrad(const RunCtx& c, const lip_op_t& op, WgradP& p) {
  const lip_seg_t& g = op.seg[0];
  p = WgradP();
  p.a = resolve(c, g.a);
  p.IH = g.IH; p.IW = g.IW; p.C = g.C; p.KH = g.KH; p.KW = g.KW;
  p.stride = g.stride; p.pad_h = g.pad_h; p.pad_w = g.pad_w;
  p.g = resolve(c, g.b); p.g_ps = g.b.pstride;
  p.R = op.n_img * op.OH * op.OW; p.OHW = op.OH * op.OW; p.OW = op.OW; p.N = op.N;
  p.M = g.KH * g.KW * g.C;
  if (op.OH <= 0 || op.OW <= 0) { set_error("WGRAD: bad geometry"); return LIP_ERR_ARG; }
  p.dOHW = FastDiv((unsigned)p.OHW); p.dOW = FastDiv((unsigned)p.OW);
  p.y = resolve(c, op.out); p.y_ps = op.out.pstride;
  p.scale = resolve(c, op.scale);
  p.ksplit = op.ksplit > 0 ? op.ksplit : 0;           // 0: the launcher picks the row split for the probe count
  if (c.mode == Sweep::ROWS) {
    p.ksplit = op.n_img; p.seg_rows = p.OHW; p.seg_ys = p.y_ps; p.y_ps *= op.n_img;
  } else if (c.per_example()) {
    p.ksplit = 1; p.seg_rows = p.OHW; p.seg_ys = 0;     // per-example row geometry; the square-accumulating launchers walk the examples
  }
  if (!p.a || !p.g || !p.y || p.R <= 0 || p.N <= 0 || p.M <= 0) { set_error("WGRAD: bad operands"); return LIP_ERR_ARG; }
  if ((long long)p.R * p.N >= (1ll << 31) || (long long)op.n_img * p.IH * p.IW * p.C >= (1ll << 31) || (long long)p.M * p.N >= (1ll << 31)) {
    set_error("WGRAD: a tensor of this binding has 2^31 or more elements; bind fewer examples per engine (ExampleChunkedGGN)");
    return LIP_ERR_ARG;
  }
  if ((p.C & 3) == 0 && (((uintptr_t)p.a) & 15)) { set_error("WGRAD: activations not 16-byte aligned"); return LIP_ERR_ARG; }
  if (c.plan && op.out.space == LIP_SP_YOUT && planned(*c.plan, op.out.off)) {
    p.overwrite = 1;
    p.v = c.V ? c.V + op.out.off : nullptr; p.v_ps = op.out.pstride; p.alpha = c.alpha;
  }
  return LIP_OK;
}

// Gram rows of a WGRAD op's cotangent operand on a pass of pc probes, and the launches they take: one over all probes
// when the probes are adjacent (the per-probe stride is the row block), else one per probe
long long kron_rows(const lip_op_t& op, int pc, int* launches) {
  const long long Rp = (long long)op.n_img * op.OH * op.OW;
  const bool packed = pc == 1 || op.seg[0].b.pstride == Rp * op.N;
  if (launches) *launches = packed ? 1 : pc;
  return packed ? Rp * pc : Rp;
}

// can the Gram of a WGRAD op's cotangent rows run on a pass of pc probes?
bool kron_op_fits(const lip_op_t& op, int pc) {
  const long long R = kron_rows(op, pc, nullptr);
  return R > 0 && R < (1ll << 31) && op.N > 0 && panel_gram_fits((int)R, op.N);
}

// KRON: S_l += sum over the (probe, example, position) rows g of the op's cotangent operand of g g^T (the panel Gram of
// lip_subnetwork.hip on the (rows, N) float32 block in place)
int kron_wgrad(const RunCtx& c, const lip_op_t& op) {
  const lip_ref_t& b = op.seg[0].b;
  const float* rows = resolve(c, b);
  int launches = 1;
  const long long R = kron_rows(op, c.P, &launches);
  if (!rows || !c.kron || !c.kron_scratch || R <= 0 || op.N <= 0) { set_error("WGRAD (kron): bad operands"); return LIP_ERR_ARG; }
  if (!kron_op_fits(op, c.P)) {       // lip_vjp_kron has checked every op before its first launch
    set_error("WGRAD (kron): 2^31 or more cotangent rows on a pass; bind fewer examples per engine");
    return LIP_ERR_ARG;
  }
  if (panel_gram_scratch((int)R, op.N) > c.kron_doubles) { set_error("WGRAD (kron): scratch too small"); return LIP_ERR_ARG; }
  double* S = c.kron;
  for (int l = 0; l < launches; ++l)
    RUN_CHECK(launch_panel_gram(rows + (int64_t)l * b.pstride, (int)R, op.N, S, c.kron_scratch, c.st), "kron gram launch");
  return LIP_OK;
}

// EIGEN: the scratch floats of one WGRAD op with Mt rows on a pass of pc probes, in the order eigen_wgrad lays them out
// (every part a whole number of float4): the projected patches AV (n OH OW, Mt), the projected rows GU (pc n OH OW, N),
// the pass's (Mt, N) float32 sums, and the scratch of the square-accumulating weight gradient on the projected pair
struct EigenLayout {
  long long av, gu, y, sq;
  long long total() const { return av + gu + y + sq; }
};
inline long long round4(long long x) { return (x + 3) / 4 * 4; }
EigenLayout eigen_layout(const lip_op_t& op, int Mt, int pc) {
  const long long Rp = (long long)op.n_img * op.OH * op.OW;
  EigenLayout l;
  l.av = round4(Rp * Mt); l.gu = round4(Rp * pc * op.N); l.y = round4((long long)Mt * op.N);
  l.sq = wgrad_sqsum_scratch(Mt, op.N, op.OH * op.OW, (long long)pc * op.n_img);
  return l;
}

// can the op run in an EIGEN sweep with Mt rows on a pass of pc probes?  (the 32-bit index arithmetic of the weight
// gradient on the projected pair, the projections' grids, and a window geometry whose clamped gather stays in the tensor)
bool eigen_op_fits(const lip_op_t& op, int Mt, int pc) {
  const lip_seg_t& g = op.seg[0];
  if (op.n_img <= 0 || op.OH <= 0 || op.OW <= 0 || op.N <= 0 || pc <= 0 || g.IH <= 0 || g.IW <= 0 || g.C <= 0 || g.KH <= 0 ||
      g.KW <= 0 || g.stride <= 0 || g.pad_h < 0 || g.pad_w < 0)
    return false;
  const long long M = (long long)g.KH * g.KW * g.C, Rp = (long long)op.n_img * op.OH * op.OW, lim = 1ll << 31;
  if (Mt != M && Mt != M + 1) return false;
  if (pc > 1 && g.b.pstride < Rp * op.N) return false;                  // the probes' row blocks would overlap
  if ((long long)(op.OH - 1) * g.stride - g.pad_h >= g.IH || (long long)(op.OW - 1) * g.stride - g.pad_w >= g.IW) return false;
  return Rp * Mt < lim && Rp * pc * op.N < lim && (long long)Mt * op.N < lim && (long long)Mt * Mt < lim &&
         (long long)op.N * op.N < lim && (long long)op.n_img * g.IH * g.IW * g.C < lim && (long long)pc * op.n_img < lim &&
         ll_project_fits(Rp, Mt) && ll_project_fits(Rp * pc, op.N);
}

// EIGEN: Lam_l += sum over the (probe, example) pairs of ((At_i V)^T (G_pi Ub))^2, At_i the example's patches, G_pi the
// pair's cotangent rows.  The patches are projected once for the pass, the rows of all its probes next; the projected
// pair is a 1x1 convolution with Mt input channels on the OH x OW map, whose per-pair weight gradients the
// square-accumulating launcher of lip_vjp_sqsum forms, squares and sums into the pass's float32 block.
int eigen_wgrad(const RunCtx& c, const lip_op_t& op) {
  const lip_seg_t& g = op.seg[0];
  const float* a = resolve(c, g.a);
  const float* rows = resolve(c, g.b);
  const EigenBlock* b = c.eigen;
  if (!a || !rows || !b || !b->V || !b->Ub || !b->Lam || !c.scratch || g.a.pstride != 0) { set_error("WGRAD (eigen): bad operands"); return LIP_ERR_ARG; }
  if (!eigen_op_fits(op, b->Mt, c.P)) {       // lip_vjp_eigen has checked every op before its first launch
    set_error("WGRAD (eigen): the block does not match the op, or a tensor of 2^31 or more elements");
    return LIP_ERR_ARG;
  }
  const EigenLayout l = eigen_layout(op, b->Mt, c.P);
  if (l.total() > c.scratch_floats) { set_error("WGRAD (eigen): scratch too small"); return LIP_ERR_ARG; }
  float* AV = c.scratch;
  float* GU = AV + l.av;
  float* y = GU + l.gu;
  float* sq = y + l.y;
  const int Mt = b->Mt, OHW = op.OH * op.OW, Rp = op.n_img * OHW;
  RUN_CHECK(launch_project_patches(a, op.n_img, g.IH, g.IW, g.C, g.KH, g.KW, g.stride, g.pad_h, g.pad_w, op.OH, op.OW,
                                   Mt - g.KH * g.KW * g.C, b->V, AV, c.st), "patch projection launch");
  RUN_CHECK(launch_rows_project(rows, op.N, g.b.pstride, c.P, Rp, op.N, b->Ub, GU, c.st), "row projection launch");
  RUN_CHECK(hipMemsetAsync(y, 0, sizeof(float) * (size_t)Mt * op.N, c.st), "memset eigen sums");
  WgradP p = WgradP();
  p.a = AV; p.IH = op.OH; p.IW = op.OW; p.C = Mt; p.KH = 1; p.KW = 1; p.stride = 1; p.pad_h = 0; p.pad_w = 0;
  p.g = GU; p.g_ps = (long long)Rp * op.N;
  p.R = Rp; p.OHW = OHW; p.OW = op.OW; p.N = op.N; p.M = Mt;
  p.dOHW = FastDiv((unsigned)OHW); p.dOW = FastDiv((unsigned)op.OW);
  p.y = y; p.y_ps = 0; p.scale = nullptr;
  p.ksplit = 1; p.seg_rows = OHW; p.seg_ys = 0;
  RUN_CHECK(launch_wgrad_sqsum(p, c.P, op.n_img, sq, l.sq, c.st), "square-sum wgrad launch (eigen)");
  RUN_CHECK(launch_eigen_fold(y, (long long)Mt * op.N, b->Lam, c.st), "eigen fold launch");
  return LIP_OK;
}

// EWNORM: the scratch floats of one WGRAD op with Mt rows on a pass of pc probes, in the order ewnorm_wgrad lays them out:
// the AV and GU of EigenLayout, then the (output tile, pair) partials of the weighted-norm weight gradient
struct EwnormLayout {
  long long av, gu, wn;
  long long total() const { return av + gu + wn; }
};
EwnormLayout ewnorm_layout(const lip_op_t& op, int Mt, int pc) {
  const EigenLayout e = eigen_layout(op, Mt, pc);
  return EwnormLayout{e.av, e.gu, wgrad_wnorm_tiles(Mt, op.N, op.OH * op.OW) * pc * op.n_img};
}

// EWNORM: wout[p n + i] += sum_{j,m} Rw[j][m] (((At_i V)^T (G_pi Ub))[j][m])^2.  The projections of eigen_wgrad; the
// projected pair goes to the weighted-norm weight gradient of lip_vjp_wnorm as the same 1x1 convolution with Mt input
// channels, its weights the block's Rw (at OH OW = 1 the launcher's bilinear route: the product is an outer product still).
int ewnorm_wgrad(const RunCtx& c, const lip_op_t& op) {
  const lip_seg_t& g = op.seg[0];
  const float* a = resolve(c, g.a);
  const float* rows = resolve(c, g.b);
  const EigenBlock* b = c.eigen;
  if (!a || !rows || !b || !b->V || !b->Ub || !b->Rw || !c.wout || !c.scratch || g.a.pstride != 0) { set_error("WGRAD (eigen wnorm): bad operands"); return LIP_ERR_ARG; }
  if (!eigen_op_fits(op, b->Mt, c.P)) {       // lip_vjp_eigen_wnorm has checked every op before its first launch
    set_error("WGRAD (eigen wnorm): the block does not match the op, or a tensor of 2^31 or more elements");
    return LIP_ERR_ARG;
  }
  const EwnormLayout l = ewnorm_layout(op, b->Mt, c.P);
  if (l.total() > c.scratch_floats) { set_error("WGRAD (eigen wnorm): scratch too small"); return LIP_ERR_ARG; }
  float* AV = c.scratch;
  float* GU = AV + l.av;
  float* part = GU + l.gu;
  const int Mt = b->Mt, OHW = op.OH * op.OW, Rp = op.n_img * OHW;
  RUN_CHECK(launch_project_patches(a, op.n_img, g.IH, g.IW, g.C, g.KH, g.KW, g.stride, g.pad_h, g.pad_w, op.OH, op.OW,
                                   Mt - g.KH * g.KW * g.C, b->V, AV, c.st), "patch projection launch");
  RUN_CHECK(launch_rows_project(rows, op.N, g.b.pstride, c.P, Rp, op.N, b->Ub, GU, c.st), "row projection launch");
  WgradP p = WgradP();
  p.a = AV; p.IH = op.OH; p.IW = op.OW; p.C = Mt; p.KH = 1; p.KW = 1; p.stride = 1; p.pad_h = 0; p.pad_w = 0;
  p.g = GU; p.g_ps = (long long)Rp * op.N;
  p.R = Rp; p.OHW = OHW; p.OW = op.OW; p.N = op.N; p.M = Mt;
  p.dOHW = FastDiv((unsigned)OHW); p.dOW = FastDiv((unsigned)op.OW);
  p.y = nullptr; p.y_ps = 0; p.scale = nullptr;
  p.ksplit = 1; p.seg_rows = OHW; p.seg_ys = 0;
  RUN_CHECK(launch_wgrad_wnorm(p, c.P, op.n_img, b->Rw, c.wout, part, l.wn, c.st), "weighted-norm wgrad launch (eigen)");
  return LIP_OK;
}

int run_op(const RunCtx& c, const lip_op_t& op) {
  switch (op.kind) {
    case LIP_OP_IGEMM: {
      if (op.nseg < 1 || op.nseg > 3) { set_error("IGEMM: nseg=%d", op.nseg); return LIP_ERR_ARG; }
      IgemmP p = IgemmP();
      p.nseg = op.nseg;
      for (int s = 0; s < op.nseg; ++s) {
        const lip_seg_t& g = op.seg[s];
        int rc;
        if ((rc = check_space(c, g.a, "seg.a")) || (rc = check_space(c, g.b, "seg.b"))) return rc;
        SegP& q = p.seg[s];
        q.a = resolve(c, g.a); q.a_ps = g.a.pstride;
        q.b = resolve(c, g.b); q.b_ps = g.b.pstride;
        q.IH = g.IH; q.IW = g.IW; q.C = g.C; q.KH = g.KH; q.KW = g.KW;
        q.stride = g.stride; q.pad_h = g.pad_h; q.pad_w = g.pad_w; q.mode = g.mode;
        q.Ktot = g.KH * g.KW * g.C;
        q.b_trans = (g.flags & LIP_SEG_B_TRANS) ? 1 : 0;
        q.dC = FastDiv((unsigned)(g.C > 0 ? g.C : 1)); q.dKW = FastDiv((unsigned)(g.KW > 0 ? g.KW : 1));
        if (g.mode == 0) { q.mul = g.stride; q.sgn = 1; q.off_h = -g.pad_h; q.off_w = -g.pad_w; q.mask = 0; q.sh = 0; }
        else { q.mul = 1; q.sgn = -1; q.off_h = g.pad_h; q.off_w = g.pad_w; q.mask = g.stride - 1; q.sh = (g.stride == 2) ? 1 : 0; }
        if (!q.a || !q.b || q.Ktot <= 0 || q.stride <= 0) { set_error("IGEMM: bad segment %d", s); return LIP_ERR_ARG; }
        if ((q.C & 3) == 0 && ((((uintptr_t)q.a) & 15) || (q.a_ps & 3))) { set_error("IGEMM: segment %d activations not 16-byte aligned", s); return LIP_ERR_ARG; }
      }
      p.R = op.n_img * op.OH * op.OW; p.OHW = op.OH * op.OW; p.OW = op.OW; p.N = op.N;
      if (op.OH <= 0 || op.OW <= 0) { set_error("IGEMM: bad geometry"); return LIP_ERR_ARG; }
      p.dOHW = FastDiv((unsigned)p.OHW); p.dOW = FastDiv((unsigned)p.OW);
      p.out = resolve(c, op.out); p.out_ps = op.out.pstride;
      p.no_ksplit = op.out.space == LIP_SP_PRIM;
      p.scale = resolve(c, op.scale);
      p.e0 = resolve(c, op.e0); p.e0_ps = op.e0.pstride;
      p.e1 = resolve(c, op.e1); p.e1_ps = op.e1.pstride;
      p.xhat = resolve(c, op.xhat);
      p.res = resolve(c, op.res); p.res_ps = op.res.pstride;
      p.dphi = resolve(c, op.dphi);
      resolve_reductions(c, op, p);
      p.xhat2 = resolve(c, op.xhat2);
      if (!p.out || p.R <= 0 || p.N <= 0) { set_error("IGEMM: bad output"); return LIP_ERR_ARG; }
      {   // the kernels index tensors with 32-bit arithmetic: refuse bindings that do not fit instead of wrapping
        const long long lim = 1ll << 31;
        bool fits = (long long)p.R * p.N < lim;
        for (int s = 0; s < op.nseg; ++s)
          fits = fits && (long long)op.n_img * p.seg[s].IH * p.seg[s].IW * p.seg[s].C < lim && (long long)p.seg[s].Ktot * p.N < lim;
        if (!fits) { set_error("IGEMM: a tensor of this binding has 2^31 or more elements; bind fewer examples per engine (ExampleChunkedGGN)"); return LIP_ERR_ARG; }
      }
      if (p.e1 && !p.xhat) { set_error("IGEMM: e1 without xhat"); return LIP_ERR_ARG; }
      if (p.red1 && !p.xhat2) { set_error("IGEMM: red1 without xhat2"); return LIP_ERR_ARG; }
      unsigned fixed_b = 0;
      for (int s = 0; s < op.nseg; ++s) fixed_b |= bound_space(op.seg[s].b) ? 1u << s : 0u;
      return launch_with_reductions(c, p, [&](const IgemmP& q) { return launch_igemm(q, c.P, c.st, c.route, c.e->cache, fixed_b); }, "IGEMM launch",
                                    op.n_img, p.OHW, p.N, p.xhat2);
    }
    case LIP_OP_WGRAD: {
      if (c.mode == Sweep::KRON) return kron_wgrad(c, op);
      if (c.mode == Sweep::EIGEN) return eigen_wgrad(c, op);
      if (c.mode == Sweep::EWNORM) return ewnorm_wgrad(c, op);
      WgradP p;
      const int rc = make_wgrad(c, op, p);
      if (rc) return rc;
      if (wgrad_scratch(c.mode, p.M, p.N, p.OHW, (long long)c.P * op.n_img) > c.scratch_floats) { set_error("WGRAD: scratch too small"); return LIP_ERR_ARG; }
      switch (c.mode) {
        case Sweep::WNORM:
          RUN_CHECK(launch_wgrad_wnorm(p, c.P, op.n_img, c.wones ? nullptr : p.y, c.wout, c.scratch, c.scratch_floats, c.st), "weighted-norm wgrad launch");
          break;
        case Sweep::SQSUM: RUN_CHECK(launch_wgrad_sqsum(p, c.P, op.n_img, c.scratch, c.scratch_floats, c.st), "square-sum wgrad launch"); break;
        default: RUN_CHECK(launch_wgrad(p, c.P, c.st, c.route, bound_space(op.seg[0].a) ? c.e->cache : nullptr), "wgrad launch");
      }
      return LIP_OK;
    }
    case LIP_OP_REDUCE: {
      if (c.no_params()) return LIP_OK;
      ReduceP p;
      memset(&p, 0, sizeof(p));
      p.g = resolve(c, op.seg[0].a); p.g_ps = op.seg[0].a.pstride;
      p.R = op.n_img * op.OH * op.OW; p.N = op.N;
      p.xhat = resolve(c, op.xhat2);
      resolve_reductions(c, op, p);
      if (c.per_example()) per_example(p, op.n_img, op.OH * op.OW);
      return reduce_params(c, p, op.n_img, "REDUCE");
    }
    case LIP_OP_POOL_FWD:
    case LIP_OP_POOL_BWD: {
      PoolP p;
      memset(&p, 0, sizeof(p));
      p.in = resolve(c, op.seg[0].a); p.in_ps = op.seg[0].a.pstride;
      p.out = resolve(c, op.out); p.out_ps = op.out.pstride;
      p.n = op.n_img; p.HW = op.OH * op.OW; p.C = op.N; p.inv = op.fscale;
      p.dphi = resolve(c, op.dphi);
      p.xhat = resolve(c, op.xhat2);
      resolve_reductions(c, op, p);
      if (!p.in || !p.out || p.C <= 0 || p.C > MAX_REDUCED_WIDTH || (p.red1 && !p.xhat)) { set_error("POOL: bad operands"); return LIP_ERR_ARG; }
      if (op.kind == LIP_OP_POOL_BWD)
        return launch_with_reductions(c, p, [&](const PoolP& q) { return launch_pool_bwd(q, c.P, c.st); }, "POOL_BWD launch", p.n, p.HW, p.C, p.xhat);
      RUN_CHECK(launch_pool_fwd(p, c.P, c.st), "pool_fwd launch");
      return LIP_OK;
    }
    case LIP_OP_MAXPOOL_PRIMAL:
    case LIP_OP_MAXPOOL_FWD:
    case LIP_OP_MAXPOOL_BWD: {
      const lip_seg_t& g = op.seg[0];
      MaxPoolP p;
      memset(&p, 0, sizeof(p));
      p.in = resolve(c, g.a); p.in_ps = g.a.pstride;
      p.out = resolve(c, op.out); p.out_ps = op.out.pstride;
      p.amax_w = resolve(c, op.aux0); p.amax = p.amax_w;
      p.n = op.n_img; p.IH = g.IH; p.IW = g.IW; p.OH = op.OH; p.OW = op.OW; p.C = op.N;
      p.KH = g.KH; p.KW = g.KW; p.stride = g.stride; p.pad_h = g.pad_h; p.pad_w = g.pad_w;
      p.dphi = resolve(c, op.dphi);
      p.xhat = resolve(c, op.xhat2);
      resolve_reductions(c, op, p);
      if (!p.in || !p.out || p.C <= 0 || p.C > MAX_REDUCED_WIDTH || p.stride <= 0 || (p.red1 && !p.xhat)) { set_error("MAXPOOL: bad operands"); return LIP_ERR_ARG; }
      if (op.kind == LIP_OP_MAXPOOL_PRIMAL) RUN_CHECK(launch_maxpool_primal(p, c.st), "maxpool_primal launch");
      else if (op.kind == LIP_OP_MAXPOOL_FWD) RUN_CHECK(launch_maxpool_fwd(p, c.P, c.st), "maxpool_fwd launch");
      else return launch_with_reductions(c, p, [&](const MaxPoolP& q) { return launch_maxpool_bwd(q, c.P, c.st); }, "MAXPOOL_BWD launch",
                                         p.n, p.IH * p.IW, p.C, p.xhat);
      return LIP_OK;
    }
    case LIP_OP_PRIMAL_POST: {
      PrimalPostP p;
      memset(&p, 0, sizeof(p));
      p.z = resolve(c, op.seg[0].a);
      p.a = resolve(c, op.out); p.dphi = resolve(c, op.out2); p.xhat = resolve(c, op.out3);
      p.bias = resolve(c, op.e0);
      p.gamma = resolve(c, op.e1); p.beta = resolve(c, op.scale);
      p.mean = resolve(c, op.aux0); p.rstd = resolve(c, op.aux1);
      p.res = resolve(c, op.res);
      p.count = (long long)op.n_img * op.OH * op.OW * op.N; p.N = op.N; p.act = op.act;
      if (!p.z || !p.a || (p.gamma && (!p.beta || !p.mean || !p.rstd))) { set_error("PRIMAL_POST: bad operands"); return LIP_ERR_ARG; }
      RUN_CHECK(launch_primal_post(p, c.st), "primal_post launch");
      return LIP_OK;
    }
    case LIP_OP_SOFTMAX: {
      const float* in = resolve(c, op.seg[0].a);
      float* pr = resolve(c, op.out); float* sq = resolve(c, op.out2);
      if (!in || !pr || !sq) { set_error("SOFTMAX: bad operands"); return LIP_ERR_ARG; }
      RUN_CHECK(launch_softmax(in, pr, sq, op.n_img, op.N, c.st), "softmax launch");
      return LIP_OK;
    }
    case LIP_OP_BN_STATS: {
      if (!c.e->consts_rw) { set_error("BN_STATS: the binding has no writable constants (lip_engine_train_bind)"); return LIP_ERR_STATE; }
      for (const lip_ref_t* r : {&op.aux0, &op.aux1, &op.scale, &op.out, &op.out2})
        if (r->space != LIP_SP_CONST) { set_error("BN_STATS: statistics must live in the CONST space"); return LIP_ERR_ARG; }
      BnStatsP p;
      p.z = resolve(c, op.seg[0].a); p.R = op.n_img * op.OH * op.OW; p.N = op.N;
      p.bias = resolve(c, op.e0); p.gamma = resolve(c, op.e1);
      p.eps = op.bn_eps; p.momentum = op.fscale;
      p.mean = resolve(c, op.aux0); p.var = nullptr; p.rstd = resolve(c, op.aux1); p.s = resolve(c, op.scale);
      p.run_mean = resolve(c, op.out); p.run_var = resolve(c, op.out2);
      p.scratch = c.e->train_scratch;
      if (!p.z || !p.gamma || op.n_img <= 0 || op.OH <= 0 || op.OW <= 0 || p.N <= 0 || (long long)op.n_img * op.OH * op.OW * p.N >= (1ll << 31) ||
          !(p.eps >= 0.f) || !(p.momentum >= 0.f && p.momentum <= 1.f)) { set_error("BN_STATS: bad operands"); return LIP_ERR_ARG; }
      if (!p.scratch || bn_stats_scratch(p.R, p.N) > c.e->train_scratch_doubles) { set_error("BN_STATS: statistics scratch too small"); return LIP_ERR_ARG; }
      RUN_CHECK(launch_bn_stats(p, c.st), "bn_stats launch");
      return LIP_OK;
    }
    case LIP_OP_BN_TRAIN_BWD: {
      BnTrainBwdP p;
      p.g = resolve(c, op.seg[0].a); p.g_ps = op.seg[0].a.pstride;
      p.xhat = resolve(c, op.xhat);
      p.dbeta = resolve(c, op.e0); p.dgamma = resolve(c, op.e1); p.d_ps = op.e0.pstride;
      p.out = resolve(c, op.out); p.out_ps = op.out.pstride;
      p.R = op.n_img * op.OH * op.OW; p.N = op.N;
      if (!p.g || !p.xhat || !p.dbeta || !p.dgamma || !p.out || p.out == p.g || op.n_img <= 0 || op.OH <= 0 || op.OW <= 0 || p.N <= 0 ||
          (long long)op.n_img * op.OH * op.OW * p.N >= (1ll << 31) || op.e1.pstride != op.e0.pstride || c.per_example()) {
        set_error("BN_TRAIN_BWD: bad operands");
        return LIP_ERR_ARG;
      }
      RUN_CHECK(launch_bn_train_bwd(p, c.P, c.st), "bn_train_bwd launch");
      return LIP_OK;
    }
    case LIP_OP_HEAD: {
      HeadP p;
      memset(&p, 0, sizeof(p));
      p.n = op.n_img; p.K = op.N; p.mode = c.head_mode; p.classifier = op.classifier; p.c = c.head_c;
      p.p = resolve(c, op.aux0); p.s = resolve(c, op.aux1);
      const lip_ref_t* in; const lip_ref_t* out;
      switch (c.head_mode) {
        case LIP_HEAD_GGN: in = &op.seg[0].a; out = &op.out; break;
        case LIP_HEAD_LT: case LIP_HEAD_OUT: in = &op.seg[0].a; out = &op.out2; break;
        case LIP_HEAD_L: case LIP_HEAD_IN: in = &op.out2; out = &op.out; break;
        default: set_error("HEAD: bad mode %d", c.head_mode); return LIP_ERR_ARG;
      }
      p.in = resolve(c, *in); p.in_ps = in->pstride;
      p.out = resolve(c, *out); p.out_ps = out->pstride;
      if (!p.in || !p.out || (p.classifier && (!p.p || !p.s))) { set_error("HEAD: bad operands (mode %d)", c.head_mode); return LIP_ERR_ARG; }
      RUN_CHECK(launch_head(p, c.P, c.st), "head launch");
      return LIP_OK;
    }
    default:
      set_error("unknown op kind %d", op.kind);
      return LIP_ERR_ARG;
  }
}

hipEvent_t next_event(const lip_engine* e) {
  if (e->ev_used == e->ev_pool.size()) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    e->ev_pool.push_back(ev);
  }
  return e->ev_pool[e->ev_used++];
}

int run_tape(const RunCtx& c, int which, bool skip_head) {
  const std::vector<lip_op_t>& t = c.e->tape[which];
  if (t.empty()) { set_error("tape %d is empty", which); return LIP_ERR_STATE; }
  for (size_t i = 0; i < t.size(); ++i) {
    if (skip_head && t[i].kind == LIP_OP_HEAD) continue;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c.e->prof) {
      e0 = next_event(c.e); e1 = next_event(c.e);
      if (e0 && e1) { c.e->ev_kind.push_back(t[i].kind); (void)hipEventRecord(e0, c.st); }
    }
    int rc;
    if (c.mode == Sweep::KRON && t[i].kind == LIP_OP_WGRAD) {
      RunCtx ck = c;                                   // this op's block of the output buffer
      ck.kron = c.kron + c.e->kron_off[i];
      rc = run_op(ck, t[i]);
    } else if ((c.mode == Sweep::EIGEN || c.mode == Sweep::EWNORM) && t[i].kind == LIP_OP_WGRAD) {
      RunCtx ck = c;                                   // this op's block of the call's arrays
      ck.eigen = c.eigen + c.e->wgrad_index[i];
      rc = run_op(ck, t[i]);
    } else {
      rc = run_op(c, t[i]);
    }
    if (c.e->prof && e0 && e1) (void)hipEventRecord(e1, c.st);
    if (rc != LIP_OK) {
      char buf[400];
      snprintf(buf, sizeof(buf), "%s", g_err);
      set_error("tape %d op %zu (kind %d): %s", which, i, t[i].kind, buf);
      return rc;
    }
  }
  return LIP_OK;
}

// Initialise the (pc, D) output block of a summed product: alpha * V (or 0) everywhere EXCEPT the parameters a fused
// weight gradient of the backward tape will write outright.  c is the pass's plain context; the ranges left out are
// returned in `skip`, the plan that the pass's fused context (fused_sum) then runs the tapes with.  This is the one place
// where a pass asks wgrad_will_overwrite, once per WGRAD op.
int init_output(const RunCtx& c, float alpha, int64_t D, OverwritePlan& skip) {
  skip.clear();
  for (const lip_op_t& op : c.e->tape[LIP_TAPE_BACKWARD]) {
    if (op.kind != LIP_OP_WGRAD) continue;
    WgradP p;
    const int rc = make_wgrad(c, op, p);
    if (rc) return rc;
    if (op.out.space == LIP_SP_YOUT && wgrad_will_overwrite(p, c.P, c.route)) skip.push_back({op.out.off, (int64_t)p.M * p.N});
  }
  const float* v = alpha != 0.f ? c.V : nullptr;
  if (skip.empty()) {
    if (v) RUN_CHECK(launch_scale_copy(c.Y, v, alpha, (long long)c.P * D, c.st), "scale_copy");
    else RUN_CHECK(hipMemsetAsync(c.Y, 0, sizeof(float) * (size_t)c.P * D, c.st), "memset Y");
    return LIP_OK;
  }
  std::sort(skip.begin(), skip.end(), [](const SkipRange& a, const SkipRange& b) { return a.off < b.off; });
  int64_t pos = 0;
  for (const SkipRange& r : skip) {
    if (r.off < pos) { set_error("init_output: overlapping weight-gradient outputs"); return LIP_ERR_STATE; }
    RUN_CHECK(launch_scale_copy_range(c.Y, v, alpha, pos, r.off - pos, c.P, D, c.st), "scale_copy_range");
    pos = r.off + r.len;
  }
  RUN_CHECK(launch_scale_copy_range(c.Y, v, alpha, pos, D - pos, c.P, D, c.st), "scale_copy_range");
  return LIP_OK;
}

// What every sweep entry point checks first, in this order: the engine, its binding, the primal pass, its own arguments
int ready(const lip_engine* e, const char* who, bool args_ok) {
  if (!e) { set_error("%s: null engine", who); return LIP_ERR_ARG; }
  if (!e->theta || !e->prim || !e->work || e->max_chunk <= 0) { set_error("%s: engine not bound", who); return LIP_ERR_STATE; }
  if (!e->primal_done) { set_error("%s: primal pass not run", who); return LIP_ERR_STATE; }
  if (!args_ok) { set_error("%s: bad argument", who); return LIP_ERR_ARG; }
  return LIP_OK;
}

// ... of a backward sweep from the head cotangents U (lip_vjp and its per-example variants)
int ready_vjp(const lip_engine* e, const char* who, const float* U, const void* out, int P, int head_mode, bool more_ok = true) {
  return ready(e, who, U && out && P > 0 && (head_mode == LIP_HEAD_L || head_mode == LIP_HEAD_IN) && more_ok);
}

// Probes per pass when P exceeds the workspace: equal passes (256 probes on an 85-probe workspace run 4 x 64, not
// 85 + 85 + 85 + 1 — a one-probe pass costs 2 ms of under-filled launches, a quarter of a 64-probe pass)
inline int balanced_chunk(int P, int max_chunk) {
  const int passes = (P + max_chunk - 1) / max_chunk;
  return (P + passes - 1) / passes;
}

// The probe-chunk loop of every sweep: body(c0, pc) runs the pass over probes [c0, c0 + pc) and returns its status.
// Probe c0 of a block with `stride` floats per probe starts at block + c0 * stride.
template <class Body>
int for_each_pass(const lip_engine* e, int P, Body body) {
  for (int c0 = 0, step = balanced_chunk(P, e->max_chunk); c0 < P; c0 += step) {
    const int rc = body(c0, std::min(step, P - c0));
    if (rc) return rc;
  }
  return LIP_OK;
}

inline float* head_block(const lip_engine* e, const float* U, int c0) { return const_cast<float*>(U) + (int64_t)c0 * e->n_img * e->K; }

// lip_ggn_vp, and lip_ggn_vp_diag (a != null): the same sweep with alpha = 0, its overwrite plan unchanged, then the
// prior term a (.) V over the pass
int ggn_sweep(const lip_engine* e, const float* V, float* Y, int P, float scale, float alpha, const float* a, hipStream_t st) {
  const Route route = current_route();
  OverwritePlan plan;
  return for_each_pass(e, P, [&](int c0, int pc) {
    const float* v = V + c0 * e->D;
    float* y = Y + c0 * e->D;
    const RunCtx plain{e, v, y, nullptr, pc, LIP_HEAD_GGN, scale, route, st};
    int rc = init_output(plain, alpha, e->D, plan);
    const RunCtx c = fused_sum(plain, alpha, &plan);
    if (rc || (rc = run_tape(c, LIP_TAPE_TANGENT, false)) || (rc = run_tape(c, LIP_TAPE_BACKWARD, true))) return rc;
    if (a) RUN_CHECK(launch_add_diag(y, v, a, pc, (long long)e->D, st), "add_diag");
    return LIP_OK;
  });
}

// does the op form bias / BN cotangents (a REDUCE op, or reductions fused into another op)?
inline bool has_reductions(const lip_op_t& op) {
  return (op.kind == LIP_OP_IGEMM || op.kind == LIP_OP_REDUCE || op.kind == LIP_OP_POOL_BWD || op.kind == LIP_OP_MAXPOOL_BWD) &&
         (op.red0.space != LIP_SP_NONE || op.red1.space != LIP_SP_NONE);
}

// Scratch floats of a lip_vjp_sqsum / lip_vjp_wnorm call of P probes (doubles of a lip_vjp_kron call): the largest need
// of one backward op on one pass (ops run in stream order and reuse it).  Depends on the tape geometry and the probes
// per pass only.
int64_t sweep_scratch(const lip_engine* e, Sweep mode, int P) {
  const int pc = e->max_chunk > 0 ? balanced_chunk(P, e->max_chunk) : P;
  int64_t need = 0;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD]) {
    const long long pairs = (long long)pc * op.n_img;
    int64_t k = 0;
    if (mode == Sweep::KRON) {
      // The last pass may be shorter, and the partial tiles of a Gram are not monotone in its rows (ll_split trades
      // ranges for rows per range): the largest need over every pass size up to pc
      if (op.kind == LIP_OP_WGRAD)
        for (int q = 1; q <= pc; ++q)
          if (kron_op_fits(op, q)) k = std::max<int64_t>(k, panel_gram_scratch((int)kron_rows(op, q, nullptr), op.N));
    } else if (op.kind == LIP_OP_WGRAD)
      k = wgrad_scratch(mode, op.seg[0].KH * op.seg[0].KW * op.seg[0].C, op.N, op.OH * op.OW, pairs);
    else if (has_reductions(op))
      k = reduce_scratch(mode, op.N, pairs);
    need = std::max(need, k);
  }
  return need;
}

// Scratch floats of a lip_vjp_eigen_wnorm call of P probes: the largest need of one backward op on a full pass (every
// part grows with the probes, so it bounds the shorter last pass), a WGRAD op with either row count a block can have,
// against the reductions' own need
int64_t ewnorm_scratch(const lip_engine* e, int P) {
  const int pc = e->max_chunk > 0 ? balanced_chunk(P, e->max_chunk) : P;
  int64_t need = 0;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD]) {
    if (op.kind == LIP_OP_WGRAD) {
      const int M = op.seg[0].KH * op.seg[0].KW * op.seg[0].C;
      for (int Mt = M; Mt <= M + 1; ++Mt) need = std::max<int64_t>(need, ewnorm_layout(op, Mt, pc).total());
    } else if (has_reductions(op)) {
      need = std::max<int64_t>(need, reduce_scratch(Sweep::EWNORM, op.N, (long long)pc * op.n_img));
    }
  }
  return need;
}

// lip_vjp_sqsum_scratch / lip_vjp_wnorm_scratch
int scratch_query(const lip_engine* e, const char* who, Sweep mode, int P, int64_t* floats) {
  if (!e || !floats || P <= 0) { set_error("%s: bad argument", who); return LIP_ERR_ARG; }
  if (e->tape[LIP_TAPE_BACKWARD].empty()) { set_error("%s: backward tape missing", who); return LIP_ERR_STATE; }
  *floats = sweep_scratch(e, mode, P);
  return LIP_OK;
}

// ... and the refusal of a call whose scratch is smaller than the query says
int scratch_fits(const lip_engine* e, const char* who, Sweep mode, int P, const void* scratch, int64_t scratch_floats) {
  const int64_t need = sweep_scratch(e, mode, P);
  if (scratch_floats >= need && (need == 0 || scratch)) return LIP_OK;
  set_error("%s: scratch of %lld %s, %lld needed (%s_scratch)", who, (long long)scratch_floats,
            mode == Sweep::KRON ? "doubles" : "floats", (long long)need, who);
  return LIP_ERR_ARG;
}

}  // namespace

extern "C" {

int lip_abi_version(void) { return 8; }
const char* lip_last_error(void) { return g_err; }
int lip_sizeof_op(void) { return (int)sizeof(lip_op_t); }
int lip_set_precision(int32_t mode) { if (mode != 0 && mode != 1) { set_error("lip_set_precision: mode must be 0 (f32) or 1 (bf16x3)"); return LIP_ERR_ARG; } set_precision_mode(mode); return LIP_OK; }
int lip_set_split_k(int32_t on) { set_split_k_mode(on != 0); return LIP_OK; }
int lip_set_winograd(int32_t mode) { if (mode < 0 || mode > 2) { set_error("lip_set_winograd: mode must be 0 (off), 1 (auto) or 2 (every eligible launch)"); return LIP_ERR_ARG; } set_wino_mode(mode); return LIP_OK; }
int lip_get_winograd(void) { return current_route().wino; }
int lip_set_wino_walk(int32_t w) { if (w != 0 && w != 1 && w != 2 && w != 4) { set_error("lip_set_wino_walk: w must be 0 (automatic), 1, 2 or 4"); return LIP_ERR_ARG; } set_wino_walk(w); return LIP_OK; }
int lip_get_wino_walk(void) { return current_route().walk; }
int lip_wino_walk_plan(int64_t gx, int32_t P) { return wino_walk_plan((long long)gx, P); }
int lip_get_precision(void) { return current_route().precision; }

int lip_engine_create(lip_engine_t** out, int64_t D, int32_t n_img, int32_t K) {
  if (!out || D <= 0 || n_img <= 0 || K <= 0) { set_error("lip_engine_create: bad argument"); return LIP_ERR_ARG; }
  lip_engine* e = new lip_engine();
  e->D = D; e->n_img = n_img; e->K = K;
  *out = e;
  return LIP_OK;
}

int lip_engine_destroy(lip_engine_t* e) {
  if (e) for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  delete e;
  return LIP_OK;
}

int lip_engine_set_tape(lip_engine_t* e, int32_t which, const lip_op_t* ops, int32_t nops) {
  if (!e || which < 0 || which > LIP_TAPE_TRAIN_BACKWARD || !ops || nops <= 0) { set_error("lip_engine_set_tape: bad argument"); return LIP_ERR_ARG; }
  e->tape[which].assign(ops, ops + nops);
  if (which == LIP_TAPE_BACKWARD) {
    e->kron_off.assign(nops, 0);
    e->wgrad_index.assign(nops, 0);
    e->kron_total = 0;
    int wgrads = 0;
    for (int i = 0; i < nops; ++i) {
      e->kron_off[i] = e->kron_total;
      e->wgrad_index[i] = wgrads;
      if (ops[i].kind == LIP_OP_WGRAD) { e->kron_total += (int64_t)ops[i].N * ops[i].N; ++wgrads; }
    }
  }
  if (which == LIP_TAPE_PRIMAL) e->primal_done = false;
  if (which == LIP_TAPE_TRAIN_PRIMAL) e->train_primal_done = false;
  return LIP_OK;
}

int lip_engine_bind(lip_engine_t* e, const float* theta, const float* consts, float* prim, float* work,
                    int64_t work_floats_per_probe, int32_t max_probes_per_chunk) {
  if (!e || !theta || !prim || !work || work_floats_per_probe <= 0 || max_probes_per_chunk <= 0) {
    set_error("lip_engine_bind: bad argument");
    return LIP_ERR_ARG;
  }
  if ((((uintptr_t)prim) & 15) || (((uintptr_t)work) & 15) || (consts && (((uintptr_t)consts) & 15))) {
    set_error("lip_engine_bind: buffers must be 16-byte aligned");
    return LIP_ERR_ARG;
  }
  // re-binding only a (grown) workspace keeps the cached primal pass valid
  if (e->theta != theta || e->consts != consts || e->prim != prim) e->primal_done = false;
  e->train_primal_done = false;
  e->consts_rw = nullptr; e->train_scratch = nullptr; e->train_scratch_doubles = 0;
  if (e->cache) e->cache->release();
  e->theta = theta; e->consts = consts; e->prim = prim; e->work = work;
  e->work_pp = work_floats_per_probe; e->max_chunk = max_probes_per_chunk;
  return LIP_OK;
}

int lip_engine_primal(lip_engine_t* e, void* stream) {
  if (!e || !e->theta || !e->prim) { set_error("lip_engine_primal: engine not bound"); return LIP_ERR_STATE; }
  // the pass rewrites PRIM from a THETA that may have changed in place: whatever the cache holds is stale from here on
  // (dropped before the launches and after them, so nothing a failed pass left half-written is taken for current)
  if (e->cache) e->cache->invalidate();
  const int rc = run_tape(RunCtx{e, nullptr, nullptr, nullptr, 1, 0, 1.f, current_route(), (hipStream_t)stream}, LIP_TAPE_PRIMAL, false);
  if (e->cache) e->cache->invalidate();
  if (rc == LIP_OK) e->primal_done = true;
  e->train_primal_done = false;          // PRIM holds eval-mode activations again
  return rc;
}

int lip_engine_train_bind(lip_engine_t* e, float* consts, double* scratch, int64_t scratch_doubles) {
  if (!e || !consts || scratch_doubles < 0 || (scratch_doubles > 0 && !scratch) || (((uintptr_t)scratch) & 15)) {
    set_error("lip_engine_train_bind: bad argument");
    return LIP_ERR_ARG;
  }
  if (!e->theta || !e->prim || e->consts != consts) { set_error("lip_engine_train_bind: consts is not the bound constants buffer"); return LIP_ERR_STATE; }
  e->consts_rw = consts; e->train_scratch = scratch; e->train_scratch_doubles = scratch_doubles;
  return LIP_OK;
}

int lip_engine_set_refresh(lip_engine_t* e, const int64_t* table, int32_t count) {
  if (!e || count < 0 || (count > 0 && !table)) { set_error("lip_engine_set_refresh: bad argument"); return LIP_ERR_ARG; }
  std::vector<lip_engine::Refresh> rows;
  for (int i = 0; i < count; ++i) {
    const int64_t* r = table + 6 * (int64_t)i;
    if (r[0] < 0 || r[1] < 0 || r[2] < -1 || r[3] <= 0 || r[3] > 65535 || r[4] <= 0 || r[5] <= 0 || r[4] >= (1ll << 31) || (r[5] + 31) / 32 > 65535 ||
        r[0] + r[3] * r[4] * r[5] > e->D) {
      set_error("lip_engine_set_refresh: bad row %d", i);
      return LIP_ERR_ARG;
    }
    rows.push_back({r[0], r[1], r[2], (int)r[3], (int)r[4], (int)r[5]});
  }
  e->refresh.swap(rows);
  return LIP_OK;
}

// the engine is bound for training: the train tapes, the writable constants
static int ready_train(const lip_engine* e, const char* who, bool args_ok) {
  if (!e) { set_error("%s: null engine", who); return LIP_ERR_ARG; }
  if (!e->theta || !e->prim || !e->work || e->max_chunk <= 0) { set_error("%s: engine not bound", who); return LIP_ERR_STATE; }
  if (!e->consts_rw) { set_error("%s: no writable constants (lip_engine_train_bind)", who); return LIP_ERR_STATE; }
  if (e->tape[LIP_TAPE_TRAIN_PRIMAL].empty() || e->tape[LIP_TAPE_TRAIN_BACKWARD].empty()) { set_error("%s: train tapes missing", who); return LIP_ERR_STATE; }
  if (!args_ok) { set_error("%s: bad argument", who); return LIP_ERR_ARG; }
  return LIP_OK;
}

int lip_train_primal(lip_engine_t* e, void* stream) {
  int rc = ready_train(e, "lip_train_primal", true);
  if (rc) return rc;
  // THETA may have changed in place and PRIM is rewritten: as in lip_engine_primal, whatever the cache holds is stale
  e->primal_done = false; e->train_primal_done = false;
  if (e->cache) e->cache->invalidate();
  rc = run_tape(RunCtx{e, nullptr, nullptr, nullptr, 1, 0, 1.f, current_route(), (hipStream_t)stream}, LIP_TAPE_TRAIN_PRIMAL, false);
  if (e->cache) e->cache->invalidate();
  if (rc == LIP_OK) e->train_primal_done = true;
  return rc;
}

int lip_train_refresh(lip_engine_t* e, void* stream) {
  const int rc = ready_train(e, "lip_train_refresh", true);
  if (rc) return rc;
  if (e->cache) e->cache->invalidate();       // the transformed copies of the transposed kernels are stale
  for (const lip_engine::Refresh& r : e->refresh)
    RUN_CHECK(launch_wt_refresh(e->theta + r.w_off, r.s_off >= 0 ? e->consts_rw + r.s_off : nullptr, e->consts_rw + r.wt_off, r.taps, r.cin,
                                r.cout, (hipStream_t)stream), "wt_refresh launch");
  return LIP_OK;
}

int lip_train_backward(lip_engine_t* e, const float* U, float* Y, void* stream) {
  int rc = ready_train(e, "lip_train_backward", U && Y);
  if (rc) return rc;
  if (!e->train_primal_done) { set_error("lip_train_backward: train primal pass not run"); return LIP_ERR_STATE; }
  RUN_CHECK(hipMemsetAsync(Y, 0, sizeof(float) * (size_t)e->D, (hipStream_t)stream), "memset Y");
  return run_tape(RunCtx{e, nullptr, Y, const_cast<float*>(U), 1, LIP_HEAD_IN, 1.f, current_route(), (hipStream_t)stream}, LIP_TAPE_TRAIN_BACKWARD, false);
}

int lip_engine_profile(lip_engine_t* e, int32_t enable) {
  if (!e) { set_error("lip_engine_profile: null engine"); return LIP_ERR_ARG; }
  e->prof = enable != 0;
  e->ev_used = 0;
  e->ev_kind.clear();
  return LIP_OK;
}

int lip_engine_profile_read(lip_engine_t* e, double* ms_by_kind, int64_t* launches_by_kind, int32_t nkinds) {
  if (!e || !ms_by_kind || !launches_by_kind || nkinds <= 0) { set_error("lip_engine_profile_read: bad argument"); return LIP_ERR_ARG; }
  for (int k = 0; k < nkinds; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
  for (size_t i = 0; i < e->ev_kind.size(); ++i) {
    hipEvent_t a = e->ev_pool[2 * i], b = e->ev_pool[2 * i + 1];
    RUN_CHECK(hipEventSynchronize(b), "hipEventSynchronize");
    float ms = 0.f;
    RUN_CHECK(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
    const int k = e->ev_kind[i];
    if (k >= 0 && k < nkinds) { ms_by_kind[k] += ms; launches_by_kind[k] += 1; }
  }
  e->ev_used = 0;
  e->ev_kind.clear();
  return LIP_OK;
}

int lip_engine_run_op(lip_engine_t* e, const lip_op_t* op, const float* V, float* Y, float* H, int32_t P, int32_t head_mode,
                      float head_c, void* stream) {
  if (!e || !op || P <= 0 || P > e->max_chunk) { set_error("lip_engine_run_op: bad argument"); return LIP_ERR_ARG; }
  if (!e->theta || !e->prim) { set_error("lip_engine_run_op: engine not bound"); return LIP_ERR_STATE; }
  return run_op(RunCtx{e, V, Y, H, P, head_mode, head_c, current_route(), (hipStream_t)stream}, *op);
}

int lip_debug_run_ops(lip_engine_t* e, int32_t which, int32_t first, int32_t count, const float* V, float* Y,
                      float* H, int32_t P, int32_t head_mode, float head_c, void* stream) {
  if (!e || which < 0 || which > LIP_TAPE_TRAIN_BACKWARD || P <= 0 || P > e->max_chunk) { set_error("lip_debug_run_ops: bad argument"); return LIP_ERR_ARG; }
  const std::vector<lip_op_t>& t = e->tape[which];
  if (first < 0 || count < 0 || (size_t)(first + count) > t.size()) { set_error("lip_debug_run_ops: bad op range"); return LIP_ERR_ARG; }
  const RunCtx c{e, V, Y, H, P, head_mode, head_c, current_route(), (hipStream_t)stream};
  for (int i = first; i < first + count; ++i) {
    const int rc = run_op(c, t[i]);
    if (rc) return rc;
  }
  return LIP_OK;
}

int lip_debug_route_count(void) { return route_count(); }

int lip_debug_routes(int64_t* counts, int32_t n, const char** names) {
  if (n < 0) { set_error("lip_debug_routes: bad argument"); return LIP_ERR_ARG; }
  routes_read(counts, n, names);
  return LIP_OK;
}

int lip_ggn_vp(lip_engine_t* e, const float* V, float* Y, int32_t P, float scale, float alpha, void* stream) {
  const int rc = ready(e, "lip_ggn_vp", V && Y && P > 0);
  return rc ? rc : ggn_sweep(e, V, Y, P, scale, alpha, nullptr, (hipStream_t)stream);
}

int lip_ggn_vp_diag(lip_engine_t* e, const float* V, float* Y, int32_t P, float scale, const float* a, void* stream) {
  const int rc = ready(e, "lip_ggn_vp_diag", V && Y && a && P > 0);
  return rc ? rc : ggn_sweep(e, V, Y, P, scale, 0.f, a, (hipStream_t)stream);
}

int lip_jvp(lip_engine_t* e, const float* V, float* U, int32_t P, int32_t head_mode, float cc, void* stream) {
  const int rc = ready(e, "lip_jvp", V && U && P > 0 && (head_mode == LIP_HEAD_LT || head_mode == LIP_HEAD_OUT));
  if (rc) return rc;
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    return run_tape(RunCtx{e, V + c0 * e->D, nullptr, head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream}, LIP_TAPE_TANGENT, false);
  });
}

int lip_vjp(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float cc, void* stream) {
  const int rc = ready_vjp(e, "lip_vjp", U, Y, P, head_mode);
  if (rc) return rc;
  const Route route = current_route();
  OverwritePlan plan;
  return for_each_pass(e, P, [&](int c0, int pc) {
    const RunCtx plain{e, nullptr, Y + c0 * e->D, head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    const int rc = init_output(plain, 0.f, e->D, plan);
    return rc ? rc : run_tape(fused_sum(plain, 0.f, &plan), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_rows(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float cc, void* stream) {
  const int rc = ready_vjp(e, "lip_vjp_rows", U, Y, P, head_mode);
  if (rc) return rc;
  const int64_t ystride = (int64_t)e->n_img * e->D;
  hipStream_t st = (hipStream_t)stream;
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    float* y = Y + c0 * ystride;
    RUN_CHECK(hipMemsetAsync(y, 0, sizeof(float) * (size_t)pc * ystride, st), "memset Y");
    return run_tape(example_rows(RunCtx{e, nullptr, y, head_block(e, U, c0), pc, head_mode, cc, route, st}), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_sqsum_scratch(lip_engine_t* e, int32_t P, int64_t* floats) {
  return scratch_query(e, "lip_vjp_sqsum_scratch", Sweep::SQSUM, P, floats);
}

int lip_vjp_sqsum(lip_engine_t* e, const float* U, float* Y, int32_t P, int32_t head_mode, float cc, float* scratch,
                  int64_t scratch_floats, void* stream) {
  int rc = ready_vjp(e, "lip_vjp_sqsum", U, Y, P, head_mode, scratch_floats >= 0);
  if (rc || (rc = scratch_fits(e, "lip_vjp_sqsum", Sweep::SQSUM, P, scratch, scratch_floats))) return rc;
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    const RunCtx c{e, nullptr, Y, head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    return run_tape(square_sum(c, scratch, scratch_floats), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_wnorm_scratch(lip_engine_t* e, int32_t P, int64_t* floats) {
  return scratch_query(e, "lip_vjp_wnorm_scratch", Sweep::WNORM, P, floats);
}

int lip_vjp_wnorm(lip_engine_t* e, const float* U, const float* w, float* out, int32_t P, int32_t head_mode, float cc,
                  float* scratch, int64_t scratch_floats, void* stream) {
  int rc = ready_vjp(e, "lip_vjp_wnorm", U, out, P, head_mode, scratch_floats >= 0);
  if (rc || (rc = scratch_fits(e, "lip_vjp_wnorm", Sweep::WNORM, P, scratch, scratch_floats))) return rc;
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    // (w == NULL: theta stands in for the weight vector — a (D,) device block whose slices are addressed, never read)
    const RunCtx c{e, nullptr, const_cast<float*>(w ? w : e->theta), head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    return run_tape(weighted_norm(c, scratch, scratch_floats, w == nullptr, out + (int64_t)c0 * e->n_img), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_kron_scratch(lip_engine_t* e, int32_t P, int64_t* doubles) {
  return scratch_query(e, "lip_vjp_kron_scratch", Sweep::KRON, P, doubles);
}

int lip_vjp_kron_layout(lip_engine_t* e, int32_t cap, int64_t* kernel_off, int64_t* out_off, int32_t* N, int32_t* count,
                        int64_t* total) {
  if (!e || cap < 0 || !count || !total || (cap > 0 && (!kernel_off || !out_off || !N))) { set_error("lip_vjp_kron_layout: bad argument"); return LIP_ERR_ARG; }
  if (e->tape[LIP_TAPE_BACKWARD].empty()) { set_error("lip_vjp_kron_layout: backward tape missing"); return LIP_ERR_STATE; }
  int32_t k = 0;
  const std::vector<lip_op_t>& t = e->tape[LIP_TAPE_BACKWARD];
  for (size_t i = 0; i < t.size(); ++i) {
    if (t[i].kind != LIP_OP_WGRAD) continue;
    if (k < cap) { kernel_off[k] = t[i].out.off; out_off[k] = e->kron_off[i]; N[k] = t[i].N; }
    ++k;
  }
  *count = k;
  *total = e->kron_total;
  return LIP_OK;
}

int lip_vjp_kron(lip_engine_t* e, const float* U, double* S, int32_t P, int32_t head_mode, float cc, double* scratch,
                 int64_t scratch_doubles, void* stream) {
  int rc = ready_vjp(e, "lip_vjp_kron", U, S, P, head_mode, scratch_doubles >= 0);
  if (rc || (rc = scratch_fits(e, "lip_vjp_kron", Sweep::KRON, P, scratch, scratch_doubles))) return rc;
  // every Gram of every pass is checked before the first launch, so that a refusal leaves S untouched
  const int step = balanced_chunk(P, e->max_chunk), last = P - (P - 1) / step * step;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD])
    if (op.kind == LIP_OP_WGRAD && !(kron_op_fits(op, step) && kron_op_fits(op, last))) {
      set_error("lip_vjp_kron: 2^31 or more cotangent rows on a pass; bind fewer examples per engine");
      return LIP_ERR_ARG;
    }
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    const RunCtx c{e, nullptr, nullptr, head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    return run_tape(kron_factors(c, S, scratch, scratch_doubles), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_eigen_scratch(lip_engine_t* e, int32_t P, int64_t* floats) {
  if (!e || !floats || P <= 0) { set_error("lip_vjp_eigen_scratch: bad argument"); return LIP_ERR_ARG; }
  if (e->tape[LIP_TAPE_BACKWARD].empty()) { set_error("lip_vjp_eigen_scratch: backward tape missing"); return LIP_ERR_STATE; }
  // every part of an op's scratch grows with the probes of a pass, so the full pass bounds the shorter last one; the
  // square sums' part is not monotone in the rows, so both row counts a block can have (with and without a bias row)
  const int pc = e->max_chunk > 0 ? balanced_chunk(P, e->max_chunk) : P;
  int64_t need = 0;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD]) {
    if (op.kind != LIP_OP_WGRAD) continue;
    const int M = op.seg[0].KH * op.seg[0].KW * op.seg[0].C;
    for (int Mt = M; Mt <= M + 1; ++Mt) need = std::max<int64_t>(need, eigen_layout(op, Mt, pc).total());
  }
  *floats = need;
  return LIP_OK;
}

int lip_vjp_eigen(lip_engine_t* e, const float* U, const double* const* V, const double* const* Ub, double* const* Lam,
                  const int32_t* Mt, int32_t nblocks, int32_t P, int32_t head_mode, float cc, float* scratch,
                  int64_t scratch_floats, void* stream) {
  int rc = ready_vjp(e, "lip_vjp_eigen", U, Lam, P, head_mode, V && Ub && Mt && nblocks > 0 && scratch && scratch_floats > 0);
  if (rc) return rc;
  if (((uintptr_t)scratch) & 15) { set_error("lip_vjp_eigen: scratch must be 16-byte aligned"); return LIP_ERR_ARG; }
  // every op of every pass is checked before the first launch, so that a refusal leaves every Lam untouched
  const int step = balanced_chunk(P, e->max_chunk), last = P - (P - 1) / step * step;
  std::vector<EigenBlock> blocks;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD]) {
    if (op.kind != LIP_OP_WGRAD) continue;
    const size_t k = blocks.size();
    if (k >= (size_t)nblocks) { set_error("lip_vjp_eigen: %d blocks, the backward tape has more weight gradients", (int)nblocks); return LIP_ERR_ARG; }
    if (!V[k] || !Ub[k] || !Lam[k]) { set_error("lip_vjp_eigen: block %zu has a null operand", k); return LIP_ERR_ARG; }
    if (op.seg[0].a.pstride != 0 || !eigen_op_fits(op, Mt[k], step) || !eigen_op_fits(op, Mt[k], last)) {
      set_error("lip_vjp_eigen: block %zu (Mt = %d) does not match its weight gradient, or a tensor of 2^31 or more "
                "elements on a pass; bind fewer examples per engine", k, (int)Mt[k]);
      return LIP_ERR_ARG;
    }
    const long long need = eigen_layout(op, Mt[k], step).total();
    if (need > scratch_floats) {
      set_error("lip_vjp_eigen: scratch of %lld floats, %lld needed (lip_vjp_eigen_scratch)", (long long)scratch_floats, need);
      return LIP_ERR_ARG;
    }
    blocks.push_back(EigenBlock{V[k], Ub[k], Lam[k], (int)Mt[k]});
  }
  if (blocks.size() != (size_t)nblocks) { set_error("lip_vjp_eigen: %d blocks, the backward tape has %zu weight gradients", (int)nblocks, blocks.size()); return LIP_ERR_ARG; }
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    const RunCtx c{e, nullptr, nullptr, head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    return run_tape(eigen_moments(c, blocks.data(), scratch, scratch_floats), LIP_TAPE_BACKWARD, false);
  });
}

int lip_vjp_eigen_wnorm_scratch(lip_engine_t* e, int32_t P, int64_t* floats) {
  if (!e || !floats || P <= 0) { set_error("lip_vjp_eigen_wnorm_scratch: bad argument"); return LIP_ERR_ARG; }
  if (e->tape[LIP_TAPE_BACKWARD].empty()) { set_error("lip_vjp_eigen_wnorm_scratch: backward tape missing"); return LIP_ERR_STATE; }
  *floats = ewnorm_scratch(e, P);
  return LIP_OK;
}

int lip_vjp_eigen_wnorm(lip_engine_t* e, const float* U, const double* const* V, const double* const* Ub, const float* const* Rw,
                        const int32_t* Mt, int32_t nblocks, const float* w_rem, float* out, int32_t P, int32_t head_mode,
                        float cc, float* scratch, int64_t scratch_floats, void* stream) {
  int rc = ready_vjp(e, "lip_vjp_eigen_wnorm", U, out, P, head_mode, V && Ub && Rw && Mt && nblocks > 0 && scratch && scratch_floats > 0);
  if (rc) return rc;
  if (((uintptr_t)scratch) & 15) { set_error("lip_vjp_eigen_wnorm: scratch must be 16-byte aligned"); return LIP_ERR_ARG; }
  // every op of every pass is checked before the first launch, so that a refusal leaves out untouched
  const int64_t need = ewnorm_scratch(e, P);
  if (scratch_floats < need) {
    set_error("lip_vjp_eigen_wnorm: scratch of %lld floats, %lld needed (lip_vjp_eigen_wnorm_scratch)", (long long)scratch_floats, (long long)need);
    return LIP_ERR_ARG;
  }
  const int step = balanced_chunk(P, e->max_chunk), last = P - (P - 1) / step * step;
  std::vector<EigenBlock> blocks;
  for (const lip_op_t& op : e->tape[LIP_TAPE_BACKWARD]) {
    if (w_rem && has_reductions(op) && !(op.N > 0 && op.N <= MAX_REDUCED_WIDTH && (long long)step * op.n_img < (1ll << 31))) {
      set_error("lip_vjp_eigen_wnorm: a parameter reduction of %d columns, or 2^31 or more pairs on a pass", (int)op.N);
      return LIP_ERR_ARG;
    }
    if (op.kind != LIP_OP_WGRAD) continue;
    const size_t k = blocks.size();
    if (k >= (size_t)nblocks) { set_error("lip_vjp_eigen_wnorm: %d blocks, the backward tape has more weight gradients", (int)nblocks); return LIP_ERR_ARG; }
    if (!V[k] || !Ub[k] || !Rw[k]) { set_error("lip_vjp_eigen_wnorm: block %zu has a null operand", k); return LIP_ERR_ARG; }
    if (op.seg[0].a.pstride != 0 || !eigen_op_fits(op, Mt[k], step) || !eigen_op_fits(op, Mt[k], last)) {
      set_error("lip_vjp_eigen_wnorm: block %zu (Mt = %d) does not match its weight gradient, or a tensor of 2^31 or more "
                "elements on a pass; bind fewer examples per engine", k, (int)Mt[k]);
      return LIP_ERR_ARG;
    }
    EigenBlock b{V[k], Ub[k], nullptr, (int)Mt[k]};
    b.Rw = Rw[k];
    blocks.push_back(b);
  }
  if (blocks.size() != (size_t)nblocks) { set_error("lip_vjp_eigen_wnorm: %d blocks, the backward tape has %zu weight gradients", (int)nblocks, blocks.size()); return LIP_ERR_ARG; }
  const Route route = current_route();
  return for_each_pass(e, P, [&](int c0, int pc) {
    // (Y is the remainder's weight vector, read at the slices of the reductions only; null: no reduction runs)
    const RunCtx c{e, nullptr, const_cast<float*>(w_rem), head_block(e, U, c0), pc, head_mode, cc, route, (hipStream_t)stream};
    return run_tape(eigen_weighted_norm(c, blocks.data(), scratch, scratch_floats, out + (int64_t)c0 * e->n_img), LIP_TAPE_BACKWARD, false);
  });
}

int lip_debug_wnorm_route_count(void) { return (int)WN_ROUTES; }

int lip_debug_wnorm_routes(int64_t* counts, int32_t n, const char** names) {
  if (n < 0) { set_error("lip_debug_wnorm_routes: bad argument"); return LIP_ERR_ARG; }
  wnorm_routes_read(counts, n, names);
  return LIP_OK;
}

}  // extern "C"
