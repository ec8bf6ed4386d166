// gpx_api.hip — host side of libgpx.so: the C ABI of include/gpx.h.
//
// Implements the fit()/predict() hot path of SURVEY.md §8 (rows a1-a6) on one MI355X:
//   fit:     K = sf2 k(X,X) + (sn2+jitter) I  ->  blocked Cholesky (in place, lower)
//            (with gpx_set_noise_weights: + diag(sn2 w_i + jitter) — DESIGN.md §3.4f)
//            ->  alpha = L^-T L^-1 y  ->  logdet
//            (with gpx_set_basis: H^T rides in the bordered rows beside y^T, then beta and z' = z - Z_H beta — DESIGN.md §3.4m)
//   predict: K* = sf2 k(Xs,X) -> mean = K* alpha -> V^T = K* L^-T -> var = sf2 - rowsumsq(V^T)
// The reference has no such path (GPmap.py has no fit/predict/linalg beyond
// np.linalg.norm at GPmap.py:120); the arithmetic follows oracle/gp_oracle.py
// (R&W Alg. 2.1).
//
// Data layout in HBM (element type T = double, or float for the fp32 / mixed handles; row-major):
//   K / L   [Npad+64][ld]  ld = Npad + one 128-byte line (skew against power-of-two strides; rows
//                          128-byte aligned); only the lower triangle is referenced; rows/cols >= N
//                          are identity; rows [Npad, Npad+64) carry the right-hand sides ("bordered").
//                          After gpx_reserve / a gpx_append that outgrew the buffer: ld = capacity rows + that line,
//                          and Npad grows inside the buffer (append_room, append_restart)
//   Winv    [Npad/64][64][64]   inverses of the 64x64 diagonal blocks of L
//   Wblk    [Npad/nb][nb][nb]   explicit inverses of the nb x nb diagonal blocks (panel / block solves
//                               are dense products with them), built beside the factorisation
//   P       2 x [Npad+64][nb+skew]  compact copies of the current / next panel (SYRK operand)
//   VT      [MB][ld]            K* and, after the forward solve, V^T — one batch of MB <= 8192 query points
//   ZT      [Npad][ld]          L^-T, on demand, for gpx_lml_grad
//                               (gpx_fit_predict: Mpad more rows below the right-hand sides carry K* -> V^T)
// Streams: st (main: the throughput work — rows below the next diagonal block, REST, the rows of the panel
// solve nobody on the chain needs, bordered / query rows), st2 (look-ahead CHAIN, high priority: update of the
// next diagonal block, its factorisation, the panel solve of the rows of the diagonal block after it), st3
// (side: block-inverse extension, parked on the POTF2's device flag), st4 (copies of solved panels / blocks
// back into their matrices).  Schedule: chol_enqueue.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/gpx.h"
#include "gpx_cov.h"
#include "gpx_env.h"
#include "gpx_internal.h"

using namespace gpx;

namespace {

thread_local std::string g_create_error;

// No exception crosses the C ABI (include/gpx.h): every extern "C" entry point that can
// allocate (std::string / std::vector / std::thread) is a function-try-block ending in this.
#define GPX_CATCH_ALL                                  \
  catch (const std::bad_alloc&) { return GPX_E_NOMEM; } \
  catch (...) { return GPX_E_HIP; }

constexpr int RHS_ROWS = 64;  // right-hand sides are padded to one 64-row MFMA slab

struct Phase {
  hipEvent_t a, b;
  double* target;
};

// One device allocation.  It frees itself: whoever destroys it has selected its device and drained the streams that
// used it (gpx_destroy, gpx_release_scratch, the unit-test entry points' Scratch).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {  // the old allocation leaves with `o`
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

struct Comm;   // gpx_shard.inc
struct Group;  // gpx_group.inc

}  // namespace

struct gpx_handle {
  gpx_config cfg{};
  int nb = 1024;       // Cholesky panel width
  int nb_solve = 256;  // block width of the alpha solves (one 64-row slab: latency-bound)
  int nb_pred = 1024;  // block width of the variance TRSM (follows the panel width when the library chooses that — auto_panel_width — unless GPX_NB_PRED is given: env.nb_pred >= 0)
  EnvKnobs env;        // the environment switches (gpx_env.h): create entries from gpx_create, call entries as of the start of this call (begin_call)
  hipStream_t st = nullptr;   // main stream
  hipStream_t st2 = nullptr;  // look-ahead (panel) stream, high priority
  hipStream_t st3 = nullptr;  // side stream of the diagonal chain: in-block SYRKs, block inverses
  hipStream_t st4 = nullptr;  // copy stream: solved panels / blocks back into their matrices
  hipStream_t st5 = nullptr;  // sharded factorisation: the owner's diagonal chain beside the all-gather of the previous panel (created by the first sharded fit)
  std::string err;
  gpx_timings tm{};
  // fitted state
  bool fitted = false;
  int64_t N = 0, Npad = 0, ld = 0, ldp = 0;
  int d = 0, k = 0, n_ls = 1;
  double sf2 = 0, sn2 = 0, jitter = 0;
  double logdet = 0;
  DevBuf X, Xs, ls, K, Winv, P, YT, Y, scalars, info;
  DevBuf var, meanout;  // predict's results on the device
  // Scratch: everything gpx_release_scratch frees (`h->scr = {}`) — buffers that any later call allocates again when it
  // needs them and that no fitted state lives in.  A buffer is scratch by being declared here, and only so.
  struct ScratchBufs {
    DevBuf Q, Qs, VT, MT;  // predict: query points (raw, scaled), K* -> V^T of one batch, mean^T
    DevBuf Qg, Qz;         // the *_paths calls: the query points' path ids (-1 up to the padded size), a zeroed diagonal vector
    DevBuf Tsol;           // predict: compact solved blocks of V^T (2 x batch x (nb + skew))
    DevBuf MTpart;         // split-K partial tiles of the posterior-mean product
    DevBuf ZT, gpart;      // gpx_lml_grad: L^-T (Npad x ld) and the per-tile partial sums
    DevBuf ZTloc, ZTpack;  // sharded gradient: own row blocks of L^-T (stacked), one packed block in flight
    DevBuf Sv;             // sharded solves: two broadcast buffers of solved blocks
    DevBuf Q64, Qs64, Q32, M64;             // GPX_MIXED predict
    DevBuf GatherS, GatherR, outM, outV;    // sharded predict: the all-gather of the ranks' slices
    // joint posterior (gpx_predict_cov / gpx_sample_posterior): scratch of their own, never the fit's buffers
    DevBuf JVT, JTsol, JSig, JSigF, JWinv, JP, JWblk, JUblk, JInfo, JZT, JST, JZin, JOut;
    // posterior gradient (gpx_predict_grad): scratch of its own as well
    DevBuf GV, GTsol, GMT, GMTpart, GVN, GPart, GOut;
    // block scoring (gpx_score_blocks, gpx_forecast_blocks): targets, per-slice Gram partials, batch mean^T, results + the bad-block word
    DevBuf SY, SPart, SMT, SOut;
    DevBuf SW;  // gpx_score_blocks_weighted: the query points' weights
    DevBuf BG, BU;  // a fit with basis functions: per-slice Gram of the bordered rows; u = L_A^-1 (h - Z_H^T v*) per query row (rows x 64, fp64)
    DevBuf UW, UQ;  // gpx_remove_rows: per pass in flight (two) the carry ((N + 64) x UPD_W) and the panel's orthogonal factor (2 UPD_W square)
    DevBuf LOO;     // gpx_loo: q (N) | var (N) | mean (N x k) | logp (N x k), fp64
    DevBuf SV1, SV2, SS2;  // gpx_sparse_predict(_cov): T1^T and T2^T of one batch of query rows; T2^T T2
    // gpx_sparse_elbo_grad: [H | ch^T], LB^-T -> LB -> L^-T M, M -> Guu, L^-T, H' = L^-T [H | ch], a chunk of T, partials + sums
    DevBuf SGH, SGZ, SGM, SGZL, SGHp, SGT, SGpart;
    DevBuf PWZ, PWpart, PWout, PWres;  // gpx_pathwise_*: a host caller's normals, the splits' partials, OutT of one batch, results for a host caller
  } scr;
  // row-block shard (world > 1)
  Comm* comm = nullptr;  // RCCL, in-process or host-callback transport (gpx_shard.inc)
  Group* group = nullptr;    // ndev > 1: this handle only fronts per-device member handles (gpx_group.inc)
  bool in_group = false;     // a member of a group: inputs may live on another device of the process
  bool discard_out = false;  // a member with rank > 0: rank 0 delivers the (identical) results
  void* zT = nullptr;      // z^T = (L^-1 y)^T (64 x ld): the bordered rows of the K buffer
  void* alphaT = nullptr;  // alpha^T (64 x ld): AT (computed on demand from z^T) or YT (shard)
  bool alpha_ready = false;
  DevBuf AT;
  // GPX_MIXED: fp64 side of the mixed-precision mode (the fp32 engine uses the buffers above)
  DevBuf RTloc, P32out;  // GPX_MIXED on a distributed shard: local columns of the refinement's right-hand sides; fp32 predict outputs
  DevBuf X64, Y64, Xs64, A64, Aprev, R64, X32, Y32, RT32, rn, Zfew;
  int refine = 0;    // GPX_MIXED: 0 = adaptive, > 0 = fixed iteration count
  DevBuf resv_ring;  // device counters of the self-reserving trailing updates ([1024][8] unsigned; GPX_CU_SELF_RESERVE)
  DevBuf strassen2;  // temporaries of strassen_nt's second level (chol_two_level_enqueue: the deep update and the deferred product share it)
  DevBuf Wblk, Ublk; // explicit inverses of the nb x nb diagonal blocks of L ([Npad/nb][nb][nb]) + scratch
  int nbw = 0;       // block width of Wblk (0: not built)
  int nb_shard = 512;  // distribution block = panel width of the sharded factorisation (chosen per fit)
  int64_t nloc = 0, ldy = 0;
  DevBuf G, Dbuf, Sbuf, YTloc, Cneg;
  // replicated-factor mode of the shard: every rank keeps the whole L (the panels pass through
  // it anyway), so solves and predictions need no per-panel exchange (gpx_shard.inc)
  bool repl = false;
  DevBuf Lfull;
  const void* Lfac = nullptr;  // the factor the single-GPU solves read: K (unsharded) or Lfull
  // device-flag hand-overs between this handle's streams (diag_enqueue, fused strip): -1 not probed yet, 1 a kernel parked
  // on one stream sees the store of a kernel launched later on another (flag_handover_probe), 0 it does not: hipEvents
  int shard_snake = 1;  // the dealing of row blocks the last sharded fit used (gpx_internal.h: Deal)
  int64_t fq_rows = 0;  // gpx_fit_predict on a shard: padded rows of this rank's slice of the query points (bordered rows of its K buffer)
  int flag_ok = -1;
  int flag_retries = 0;  // fits of this handle that were run again with hipEvents after a parked stream timed out
  int64_t reserve = 0;   // gpx_reserve: points the layout of the next fit / append leaves room for (0: what the fit needs)
  // per-observation noise weights (gpx_set_noise_weights).  Nothing here is allocated, and no kernel
  // reads any of it, while no weights are set.
  DevBuf Wset;           // the weights of the next fits, in the handle's element type (double for GPX_MIXED)
  int64_t nw_set = 0;    // how many (0: none set)
  DevBuf Wfit, Wfit64;   // the weights of the CURRENT fit: in the fit engine's element type, with room for the layout's
                         // capacity (appends); GPX_MIXED: and in fp64 (refinement, gpx_get_noise_weights)
  bool weighted = false; // the current fit was built with Wfit
  // observation kinds (gpx_set_observation_kinds): -1 a value of f, j a value of d f / d x_j.  Nothing here
  // is allocated, and no kernel reads any of it, while no kinds are set.
  std::vector<int32_t> kinds_set;  // the kinds of the next fits (empty: none set)
  double sn2_deriv_set = 0.0;      // ... and the noise variance of their derivative rows
  std::vector<int32_t> kinds_fit;  // the kinds of the CURRENT fit (kinded only)
  DevBuf Kfit, Dfit;               // the same on the device, -1 up to the layout's capacity; the finished diagonal terms
  double sn2_deriv = 0.0;
  bool kinded = false;             // the current fit was built by the KINDS builders: every K* against it is, too
  bool has_deriv = false;          // ... and has at least one derivative row
  // path ids (gpx_set_path_groups): id >= 0 the path of an observation, -1 none; a same-path pair gets
  // + sg2 k(., .; ls_path).  Nothing here is allocated, and no kernel reads any of it, while no ids are set.
  std::vector<int32_t> groups_set;  // the ids of the next fits (empty: none set)
  double sg2_set = 0.0;             // ... their within-path variance
  std::vector<double> lsp_set;      // ... and lengthscales (1 or d)
  std::vector<int32_t> groups_fit;  // the ids of the CURRENT fit (grouped only)
  std::vector<double> q_fit;        // q_c = (l_c / l_path,c)^2 of the current fit (d entries; the source of Gq)
  DevBuf Gfit, Gdiag, Gq;           // the ids on the device, -1 up to the layout's capacity; the finished diagonal terms; q
  double sg2 = 0.0;
  int n_lsp = 0;                    // the number of path lengthscales of the current fit (1 or d; grouped only)
  bool grouped = false;             // the current fit was built by the GROUPS builder (ids set, one >= 0, sg2 > 0)
  // explicit basis functions (gpx_set_basis).  Nothing here is allocated, and no kernel of gpx_basis.hip
  // is launched, while no basis is set.
  int basis_set = 0;  // the basis of the next fits (GPX_BASIS_*; 0: none)
  int basis = 0;      // the basis of the CURRENT fit and its number of functions p (0: a plain fit)
  int bp = 0;
  DevBuf Bst;         // the current fit's beta | L_A | A^-1 (fp64; gpx_internal.h: BASIS_STATE)
  // pathwise posterior function samples (gpx_pathwise_draw): the stored draw of the CURRENT fit — state,
  // not scratch.  S == 0: none.  Whatever changes the factor drops it (drop_pathwise).
  struct Pathwise {
    DevBuf Om, W, V;  // Omega (F x d, fp64), W (Cpad x ldw), V = R K_y^-1 (Cpad x ld, rows as alphaT's)
    int64_t S = 0, F = 0, ldw = 0, n_normals = 0;
  } pw;
  // inducing-point fit (gpx_sparse_fit; gpx_sparse.inc).  A handle holds a dense fit (`fitted`) or a sparse
  // one (`sp.fitted`), never both: begin_fit drops this state, gpx_sparse_fit drops the dense factor.  Every matrix here has
  // the leading dimension ld = mpad + 64 + skew (the chunk carries 64 bordered columns, and the solves take one ld).
  struct Sparse {
    bool fitted = false;
    int64_t N = 0, m = 0, mpad = 0, chunk = 0, ld = 0;
    double elbo[8] = {};
    double sum_inv_s2 = 0;    // sum_n 1 / s_n^2 of the fit's observations (the gradient's sf2 and sn2 entries)
    DevBuf Z, Zs;             // inducing points: raw (m x d), scaled (mpad x d)
    DevBuf L, WinvL;          // chol(Kuu) and its 64-block inverses
    DevBuf B, WinvB;          // chol(I + A A^T) with c^T as bordered rows [mpad, mpad + 64), and its 64-block inverses
    DevBuf P, Wblk, Ublk, info, scal;  // the factorisations' panels, block inverses, two info blocks, the bound's scalars
    DevBuf Xc, Xsc, Yc, Wc, Kc, part;  // one chunk: points (raw, scaled), targets, weights, bordered rows; the TN partials
  } sp;
  // event pool
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<Phase> phases;
  // Drains the streams, then destroys the communicator, the events and the streams; the DevBuf members free themselves
  // after that.  The caller has selected the device (gpx_destroy does).
  ~gpx_handle();
};

namespace {

#define HIPCHK(h, call)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      char buf_[512];                                                                      \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
               __FILE__, __LINE__);                                                        \
      (h)->err = buf_;                                                                     \
      return e_ == hipErrorOutOfMemory ? GPX_E_NOMEM : GPX_E_HIP;                          \
    }                                                                                      \
  } while (0)

int fail(gpx_handle* h, int code, const char* msg) {
  if (h) h->err = msg; else g_create_error = msg;
  // a dense entry point that finds no dense fit on a handle with a sparse one: say where that fit is served
  if (h && h->sp.fitted && code == GPX_E_ARG && (strstr(msg, "no successful fit") || strstr(msg, "no fit")))
    h->err += " (the handle holds an inducing-point fit: use the gpx_sparse_* calls)";
  return code;
}

// the same with the message "<fn>: <what>", fn the exported name of the call
int fail(gpx_handle* h, int code, const char* fn, const char* what) {
  return fail(h, code, (std::string(fn) + ": " + what).c_str());
}

bool bad_mem_kind(int32_t mem_kind) { return !(mem_kind == GPX_MEM_HOST || mem_kind == GPX_MEM_DEVICE); }

// n int32 side values (kinds, path ids) from host or device memory into `out` (on the handle's device unless it fronts a group)
int fetch_ids(gpx_handle* h, const int32_t* src, int64_t n, int32_t mem_kind, std::vector<int32_t>& out) {
  out.resize((size_t)n);
  if (mem_kind == GPX_MEM_HOST) {
    std::copy(src, src + n, out.begin());
    return GPX_OK;
  }
  if (!h->group) HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipMemcpy(out.data(), src, (size_t)n * sizeof(int32_t), hipMemcpyDefault));
  return GPX_OK;
}

// the first of n ids below -1 (the only values no id or kind may take), or n
int64_t first_below_minus_one(const int32_t* ids, int64_t n) {
  return std::find_if(ids, ids + n, [](int32_t v) { return v < -1; }) - ids;
}

// a variance a caller may set (sg2, sn2_deriv): finite and >= 0; n path lengthscales: each finite and > 0
bool variance_ok(double v) { return v >= 0.0 && std::isfinite(v); }
bool path_ls_ok(const double* ls_path, int32_t n) {
  return std::all_of(ls_path, ls_path + n, [](double l) { return l > 0.0 && std::isfinite(l); });
}

// the refusal of gpx_predict_grad / gpx_kernel_deriv_matrix: k = sf2 e^-r has a kink at r = 0
#define MATERN12_NO_GRAD "Matern-1/2 is not differentiable (its sample paths have no derivative)"
// the refusals of gpx_predict_hess / gpx_kernel_hess_matrix
#define NOT_TWICE_DIFFERENTIABLE \
  "the kernel is not twice differentiable (only RBF and Matern-5/2 sample paths have a second derivative)"
#define HESS_D_LIMIT "second derivatives are built for at most 8 input dimensions (d > 8)"

#define LAUNCHCHK(h)                                                                                  \
  do {                                                                                                \
    if (take_launch_error())                                                                          \
      return fail(h, GPX_E_ARG, "internal error: a triangular-solve operand was not 128-byte aligned"); \
  } while (0)

int ensure(gpx_handle* h, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return GPX_OK;
  if (b.p) HIPCHK(h, hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  HIPCHK(h, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return GPX_OK;
}

// the same for a buffer the caller can do without: false, and no error on the handle, when the memory is not there
bool try_ensure(gpx_handle* h, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return true;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return false;
  }
  b.cap = bytes;
  return true;
}

hipEvent_t next_event(gpx_handle* h) {
  if (h->ev_used == h->ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    h->ev_pool.push_back(e);
  }
  return h->ev_pool[h->ev_used++];
}

// "what stream a has been given so far": a pooled event recorded on a, in *e — for a wait that comes later.  `site`
// names the caller in the message of a call that fails here.
int record_event(gpx_handle* h, hipStream_t a, const char* site, hipEvent_t* e) {
  if (!(*e = next_event(h))) {
    char msg[64];
    snprintf(msg, sizeof msg, "hipEventCreate failed (%s)", site);
    return fail(h, GPX_E_HIP, msg);
  }
  HIPCHK(h, hipEventRecord(*e, a));
  return GPX_OK;
}

// stream b waits for what stream a has been given so far
int stream_waits(gpx_handle* h, hipStream_t b, hipStream_t a, const char* site) {
  hipEvent_t e;
  if (int rc = record_event(h, a, site, &e)) return rc;
  HIPCHK(h, hipStreamWaitEvent(b, e, 0));
  return GPX_OK;
}

// roctx ranges around the phases (SURVEY.md §5 "tracing"): `rocprofv3 --marker-trace --kernel-trace` then shows which
// phase of a fit / predict enqueued which kernels.  librocprofiler-sdk-roctx.so is resolved at run time — the copy a
// profiler already mapped if there is one — and everything is a no-op when it is absent or GPX_ROCTX=0.  The ranges
// bracket the HOST-side enqueue of a phase (roctx marks host time; the per-phase GPU time is gpx_timings').
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
const Roctx& roctx() {
  static const Roctx r = [] {
    Roctx x;
    EnvKnobs env;
    env_read(env, EnvAt::process);
    if (!env.roctx) return x;
    void* lib = nullptr;
    for (const char* n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"})
      if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!lib)
      for (const char* n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so"})
        if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) return x;
    x.push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
    x.pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
    if (!x.push || !x.pop) x.push = nullptr, x.pop = nullptr;
    return x;
  }();
  return r;
}

// the range name of a phase = the gpx_timings field its time goes to
const char* phase_name(const gpx_handle* h, const double* t) {
  const gpx_timings& tm = h->tm;
#define GPX_PHASE(f) \
  if (t == &tm.f) return "gpx:" #f;
  GPX_PHASE(h2d) GPX_PHASE(kbuild) GPX_PHASE(chol) GPX_PHASE(solve) GPX_PHASE(logdet) GPX_PHASE(fit_total)
  GPX_PHASE(kstar) GPX_PHASE(mean) GPX_PHASE(trsm) GPX_PHASE(var) GPX_PHASE(d2h) GPX_PHASE(predict_total)
  GPX_PHASE(comm) GPX_PHASE(chol_diag) GPX_PHASE(chol_trsm) GPX_PHASE(chol_strip) GPX_PHASE(chol_syrk)
  GPX_PHASE(grad_trtri) GPX_PHASE(grad_trace) GPX_PHASE(grad_total) GPX_PHASE(refine)
#undef GPX_PHASE
  return "gpx:phase";
}

struct PhaseScope {
  gpx_handle* h;
  Phase ph;
  bool on;
  hipStream_t s;
  bool ranged = false;
  PhaseScope(gpx_handle* h_, double* target, bool enable = true, hipStream_t stream = nullptr)
      : h(h_), on(enable), s(stream ? stream : h_->st) {
    if (roctx().push) ranged = roctx().push(phase_name(h, target)) >= 0;
    if (!on) return;
    ph.a = next_event(h);
    ph.b = next_event(h);
    ph.target = target;
    if (ph.a) (void)hipEventRecord(ph.a, s);
  }
  ~PhaseScope() {
    if (ranged) (void)roctx().pop();
    if (!on) return;
    if (ph.b) (void)hipEventRecord(ph.b, s);
    if (ph.a && ph.b) h->phases.push_back(ph);
  }
};

// after the stream is idle: fold event pairs into their targets
void collect_phases(gpx_handle* h) {
  for (auto& p : h->phases) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) *p.target += ms;
  }
  h->phases.clear();
  h->ev_used = 0;
}

// EnvKnobs::counters_collected: rocprofv3 --pmc (or a counter input file) exports ROCPROF_COUNTER_COLLECTION=1 into the
// profiled process.  Counter collection serialises kernels across streams in an order of its own, which a stream parked on a
// device flag (wait_counter_kernel) does not survive — it would spin until its time-out — so the device-side
// hand-overs switch themselves off there and the schedule falls back to hipEvents (same kernels otherwise).

// Self-test of the device-flag hand-over, once per handle: a wait kernel on the side stream, then a
// one-thread store on the main stream.  With concurrent queues the waiter sees the flag within microseconds; where
// kernels are serialised across streams (AMD_SERIALIZE_KERNEL, counter collection, a debugger or tool funnelling the
// streams into one hardware queue in submission order) it runs out of its ~50 ms of polls first, and the handle hands
// over by hipEvents (same kernels, same arithmetic: bit-identical, tests/test_gp_parity_gpu.py) instead of meeting
// wait_counter_kernel's 15 s time-out inside a fit.  GPX_CHAIN_FLAG=0|1 overrides (and skips the probe).
int flag_handover_probe(gpx_handle* h) {
  if (h->flag_ok >= 0) return GPX_OK;
  if (h->env.chain_flag >= 0) return GPX_OK;  // explicit override (chain_flag_enabled looks at it per call): nothing cached
  if (h->env.counters_collected || !h->st3) {
    h->flag_ok = 0;
    return GPX_OK;
  }
  unsigned* d = nullptr;
  unsigned seen = 0;
  HIPCHK(h, hipMalloc(&d, 64));
  hipError_t e = hipMemsetAsync(d, 0, 64, h->st);
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  if (e == hipSuccess) {
    launch_flag_probe_wait(d, d + 1, 1u << 15, h->st3);  // ~2 us per poll: gives up after ~50-70 ms
    launch_flag_probe_set(d, h->st);
    e = hipStreamSynchronize(h->st3);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  if (e == hipSuccess) e = hipMemcpy(&seen, d + 1, sizeof(unsigned), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIPCHK(h, e);
  h->flag_ok = seen ? 1 : 0;
  return GPX_OK;
}

// device-flag hand-overs for this handle's schedule?  (per call: tests switch GPX_CHAIN_FLAG between fits)
bool chain_flag_enabled(const gpx_handle* h) {
  if (h->env.chain_flag >= 0) return h->env.chain_flag != 0;
  return !h->env.counters_collected && h->flag_ok == 1;
}

// the trailing update of chol_enqueue: one fused launch (GPX_FUSED_STRIP, device-flag hand-overs only), else the split
// schedule (the default), else the round-2 look-ahead
bool fused_strip_in_force(const gpx_handle* h) { return h->env.fused_strip && chain_flag_enabled(h); }
bool split_strip_in_force(const gpx_handle* h) { return h->env.split_strip && !fused_strip_in_force(h); }

// A stream parked on a device flag timed out (a negative info word) although the handle's self-test passed — a tool
// attached later, or one that reorders rather than serialises.  True: the handle hands over by hipEvents from now on and
// the caller runs its work once more (same kernels, same bits).  False — a second failure, or the user forced the flag
// with GPX_CHAIN_FLAG — is the caller's error.  The decision uses nothing that differs between the ranks of a shard (not
// the rank-local h->flag_ok: with it at 0 and the flag not forced no stream of THIS handle parks, but a peer's may have
// timed out, and the ranks must retry — or leave — together).
bool retry_with_events(gpx_handle* h, bool retried) {
  if (retried || h->env.chain_flag >= 0) return false;
  h->flag_ok = 0;
  h->flag_retries += 1;
  return true;
}

constexpr int RESV_RING = 1024;  // self-reserving launches per factorisation (more: plain kernels)

// ---- blocked right-looking Cholesky, in place on the lower triangle -------------------
// A [n][ld]; Winv [n/64][64*64]; P = two compact panel buffers [n][ldp]; n multiple of
// 64 (128 when n > nb).  Two levels: panels of width nb; inside a panel's diagonal block,
// 64-wide sub-panels whose diagonal is factorised by the one-workgroup POTF2.
//
// One-panel look-ahead: the trailing update of step p is split into the STRIP (the nb
// columns that form panel p+1) and the REST.  As soon as the strip is done, the
// high-priority stream st2 factorises diagonal block p+1 and solves panel p+1 (into the
// other P buffer) while the main stream runs the rest of update p; the two streams
// touch disjoint columns of A.

// Explicit inverses W_p = L_pp^-1 of the nb x nb diagonal blocks, built BESIDE the factorisation
// of each block on the auxiliary stream: with them a panel solve X <- X L_pp^-T is ONE dense
// product X W_p^T on the MFMA tile engine instead of 64-row slabs each walking the nb/64 column
// blocks in sequence (a latency chain of ~0.7 ms per panel whatever the number of rows — the
// largest single item of a small-N fit: BASELINE.json configs[1]).
template <typename T>
struct InvWork {
  T* W = nullptr;   // [n / nbw][nbw][nbw], row-major, lower triangular (strictly upper part zero)
  T* U = nullptr;   // scratch: (L_pp^-1)^T of the block in flight, [nbw][ldu]
  int64_t ldu = 0;
  int nbw = 0;
  hipStream_t aux = nullptr;
  hipEvent_t ready = nullptr;      // recorded on aux when the inverse of the last enqueued block is complete
  hipEvent_t copied[2] = {};       // copy-back of the panel last written into P buffer 0 / 1 (copy stream)
  unsigned seq = 0;                // step flag's last value (info[9]): counts on from block to block of one factorisation
};

// diagonal block [o, o+nbp) on stream s.  iw != null: after the POTF2 of every 64-column step the
// auxiliary stream extends the block's inverse by one column block of U / row block of W
// (launch_inv_extend) — one event per step, nothing on the critical chain.
// lm: how every launch of the block goes out (the POTF2 and the slab solves read its chain side, the rest `latency`).
template <typename T>
int diag_enqueue(gpx_handle* h, T* A, int64_t ld, int64_t o, int nbp, T* Winv, int* info, int64_t gidx0,
                 hipStream_t s, InvWork<T>* iw = nullptr, LaunchMode lm = {}) {
  T* Wp = nullptr;
  // Hand-over to the side stream WITHOUT events on the chain (round 3): POTF2 of step i publishes i + 1 in
  // info[9] after a device-scope release; the side stream is parked on wait_counter_kernel in front of each
  // inverse extension.  The extension of column blocks [q, q + w) needs the rows of L of those blocks, which
  // are complete with the step's POTF2 (their off-diagonal part came from earlier steps' solves).  A hipEvent
  // per step cost the chain ~7 us of every 70 (record + the gap it opens).
  // The hipEvent per step comes back (GPX_CHAIN_FLAG=0, or by itself: flag_handover_probe) where kernels of different
  // streams do not run concurrently, e.g. under `rocprofv3 --pmc` (counter collection serialises kernels across queues
  // in an order of its own; the parked wait kernel then runs before the POTF2 it waits for and only its time-out ends
  // the stand-off — measured in round 3: the bench died after 15 s).
  unsigned* dflag = reinterpret_cast<unsigned*>(info + 9);  // `info` is a 64-byte buffer: [0] pivot, [8] strip counter, [9] step flag
  unsigned seq = iw ? iw->seq : 0;
  const bool use_flag = chain_flag_enabled(h);  // the handle's self-test (flag_handover_probe) or GPX_CHAIN_FLAG
  if (iw) {
    Wp = iw->W + (o / iw->nbw) * (int64_t)iw->nbw * iw->nbw;
    // the side stream starts behind everything already queued on s: the W block may live in a
    // buffer that earlier work on s (or, through its waits, on other ranks) is still reading
    hipEvent_t e0 = next_event(h);  // (taken in front of the memset: not record_event)
    if (!e0) return fail(h, GPX_E_HIP, "hipEventCreate failed (block inverse)");
    // the step flag (info[9]) is reset in front of the FIRST block only; later blocks count on (one memset and
    // the gaps around it less on the chain per block; every stream that polls the flag starts behind e0)
    if (seq == 0) HIPCHK(h, hipMemsetAsync(dflag, 0, sizeof(unsigned), s));
    HIPCHK(h, hipEventRecord(e0, s));
    HIPCHK(h, hipStreamWaitEvent(iw->aux, e0, 0));
    HIPCHK(h, hipMemsetAsync(iw->U, 0, (size_t)iw->nbw * iw->ldu * sizeof(T), iw->aux));
    launch_set_diag_one_t<T>(iw->U, iw->ldu, nbp, iw->aux);
    HIPCHK(h, hipMemsetAsync(Wp, 0, (size_t)iw->nbw * iw->nbw * sizeof(T), iw->aux));
  }
  // The serial chain — POTF2, solve of the 64 columns below, SYRK inside the block — stays on ONE
  // stream: moving the SYRK to a side stream (so that it would run beside the next POTF2) made
  // the chain 40 % LONGER (measured at N = 8192: 49 -> 73 us per step), because every cross-stream
  // event wait costs more than the 6 us launch it hides.  The inverse extension only ever waits
  // FOR the chain (never the other way round), one event per step: batching the events four steps
  // at a time saved 0.3 ms of chain at N = 8192 but let the inverse lag behind the block's last
  // POTF2, and the panel solve waiting for it lost 0.7 ms.
  // Round 3: the chain advances 128 columns per step — ONE launch factors the 128 x 128 diagonal tile
  // (POTF2 of 64, the 64 x 64 block below it, its update, POTF2 of the second 64: potf2_128_kernel),
  // then one solve of the rows below, one update inside the block and one inverse-extension event
  // per 128 columns instead of per 64 (GPX_DIAG_STEP=64 selects the old stepping: A/B measurement).
  const int diag_step = h->env.diag_step;
  const int nq = nbp / KB;
  for (int q = 0; q < nq;) {
    const int w = (diag_step == 128 && q + 1 < nq) ? 2 : 1;  // 64-blocks factored by this step
    const int64_t oq = o + (int64_t)q * KB;
    T* Aqq = A + oq * ld + oq;
    T* Wq = Winv + (oq / KB) * (KB * KB);
    seq += 2;  // POTF2 writes seq - 1 when it starts ("everything before it on the chain is complete") and seq when it is done
    if (w == 2)
      launch_potf2_128<T>(Aqq, ld, Wq, gidx0 + oq, info, s, iw && use_flag ? dflag : nullptr, seq, lm);
    else
      launch_potf2_64<T>(Aqq, ld, Wq, gidx0 + oq, info, s, iw && use_flag ? dflag : nullptr, seq);
    const int64_t rem = o + nbp - (oq + w * KB);
    if (rem > 0) {
      T* panel = A + (oq + w * KB) * ld + oq;
      launch_trsm_rlt<T>(panel, ld, rem, Aqq, ld, Wq, w * KB, nullptr, 0, s, lm);
      launch_gemm_nt<T>(64, A + (oq + w * KB) * ld + (oq + w * KB), ld, panel, ld, panel, ld, rem, rem, w * KB, 1, 0, s, lm);
    }
    if (iw) {  // column blocks q .. q + w - 1 of the inverse, behind this step's POTF2
      if (use_flag) {
        // the part of the extension's walk that lies left of this step's columns needs nothing of this step:
        // it starts with the step's POTF2 and runs beside it; the rest follows the POTF2
        if (q > 0) {
          launch_wait_counter(dflag, seq - 1, info, iw->aux);
          launch_inv_extend<T>(iw->U, iw->ldu, A + o * ld + o, ld, Winv + (o / KB) * (KB * KB), q, q + w, Wp,
                               iw->nbw, iw->aux, 1, lm);
        }
        launch_wait_counter(dflag, seq, info, iw->aux);
      } else {  // the same two launches (the same arithmetic, bit for bit), both behind the step's event
        if (int rc = stream_waits(h, iw->aux, s, "block inverse")) return rc;
        launch_inv_extend<T>(iw->U, iw->ldu, A + o * ld + o, ld, Winv + (o / KB) * (KB * KB), q, q + w, Wp, iw->nbw,
                             iw->aux, 1, lm);
      }
      launch_inv_extend<T>(iw->U, iw->ldu, A + o * ld + o, ld, Winv + (o / KB) * (KB * KB), q, q + w, Wp, iw->nbw,
                           iw->aux, 2, lm);
    }
    q += w;
  }
  if (iw) {
    iw->seq = seq;
    if (int rc = record_event(h, iw->aux, "block inverse", &iw->ready)) return rc;
  }
  return GPX_OK;
}

// Panel solve below diagonal block [o, o+nbp): P (rows x nbp, ldp) = A[t.., o..] * L_pp^-T, also
// stored back into A.  With the block inverse: two dense products (main rows / bordered rows) into
// P on stream s, and the copy back into A on the auxiliary stream (nobody reads the panel from A
// before the factorisation is over: the trailing updates read P).  Without: the slab kernel.
// row0 / prev / last (round 3): the rows [row0, row0 + rows_main + nx) of the panel only — the split schedule solves
// the rows of the next diagonal block on the chain and the rest on the main stream.  `prev` is the copy-back event
// of the panel that last lived in P[set] (every part waits for it before it writes); the part with `last` set
// records the new one (both parts' copies run in order on the copy stream).
template <typename T>
int panel_solve_enqueue(gpx_handle* h, T* A, int64_t ld, int64_t o, int nbp, int64_t rows_main, int64_t nx,
                        const T* Winv, T* P, int64_t ldp, hipStream_t s, InvWork<T>* iw, int set, LaunchMode lm,
                        int64_t row0 = 0, hipEvent_t prev = nullptr, bool last = true) {
  T* Apanel = A + (o + nbp + row0) * ld + o;
  P += row0 * ldp;
  const int64_t rows = rows_main + nx;
  if (rows <= 0) {
    if (iw && last && row0 > 0) {  // nothing in this part: the first part's copy is the panel's
      if (int rc = record_event(h, h->st4, "panel copy", &iw->copied[set])) return rc;
    }
    return GPX_OK;
  }
  if (!iw) {
    launch_trsm_rlt<T>(Apanel, ld, rows, A + o * ld + o, ld, Winv + (o / KB) * (KB * KB), nbp, P, ldp, s, lm);
    return GPX_OK;
  }
  const T* Wp = iw->W + (o / iw->nbw) * (int64_t)iw->nbw * iw->nbw;
  HIPCHK(h, hipStreamWaitEvent(s, iw->ready, 0));
  if (row0 == 0 && last) prev = iw->copied[set];
  if (prev) HIPCHK(h, hipStreamWaitEvent(s, prev, 0));  // P[set] is about to be overwritten
  const int tile_main = gemm_nt_tile((rows_main % 128 == 0 && nbp % 128 == 0) ? 128 : 64, rows_main, nbp, 4);
  if (rows_main > 0 && nx > 0 && tile_main == 64) {
    // the bordered rows lie directly below the matrix rows, in A and in P: with 64-tiles on both, ONE launch
    // (as a launch of its own the 64-row product is a serial K = nb walk of ~37 us on the chain)
    launch_gemm_nt_fixed<T>(64, P, ldp, Apanel, ld, Wp, iw->nbw, rows, nbp, nbp, 4, 1, s, lm);
  } else {
    if (rows_main > 0) launch_gemm_nt_fixed<T>(tile_main, P, ldp, Apanel, ld, Wp, iw->nbw, rows_main, nbp, nbp, 4, 1, s, lm);
    if (nx > 0)
      launch_gemm_nt<T>(64, P + rows_main * ldp, ldp, Apanel + rows_main * ld, ld, Wp, iw->nbw, nx, nbp, nbp, 4, 1,
                        s, lm);
  }
  if (int rc = stream_waits(h, h->st4, s, "panel copy")) return rc;
  launch_copy2d<T>(Apanel, ld, P, ldp, rows, nbp, h->st4);
  if (last) return record_event(h, h->st4, "panel copy", &iw->copied[set]);
  return GPX_OK;
}

// nx extra rows (0 or a multiple of 64) directly below row n-1 ride along through every
// panel solve and trailing update without being factorised: with the right-hand sides
// stored there as rows ("bordered matrix"), they leave the factorisation as
// z^T = (L^-1 y)^T — the forward substitution costs no serial pass of its own.
// Round 3 — FUSED trailing update (GPX_FUSED_STRIP=1; the default stays the two-launch form: on the
// bench both take the same time — the boundary between STRIP and REST costs nothing measurable, the
// "gaps" of the round-2 trace were the strips' own work — and the fused form must not run under
// rocprofv3 --pmc, which serialises kernels and would starve the parked stream until its time-out):
// STRIP and REST are ONE launch (gemm_nt_fused_kernel) with the strip's tiles enumerated first.  Each strip slot bumps a device counter (info[8]) when its tile is released; the look-ahead
// stream is parked on wait_counter_kernel until the strip of this panel is complete and then runs
// the next diagonal block and panel solve beside the rest of the same launch.  The bordered rows'
// update of panel p+1 moves behind the panel solve on the look-ahead stream (it touches no row of
// the matrix proper), i.e. off the chain and inside the previous update.
// of nr bordered rows (x nc columns), those that go out in 128-tiles when nr is no multiple of 128: all but the remainder
inline int64_t split_rows_128(int64_t nr, int64_t nc) {
  return (nr > 128 && nr % 128 != 0 && nc % 128 == 0) ? nr / 128 * 128 : nr;
}

// The two-level factorisation's deferred product (chol_two_level_enqueue), split schedule only:
// while o < c1 the 128-multiple of the side rows is updated in columns [t0, c1) only, and right behind the side step of
// the last panel left of c1 ONE product at K = c1 gives their columns [c1, n) what those panels owe them.
struct DeferLeft {
  int64_t c1 = 0;    // a panel boundary in (0, n)
  int64_t smin = 0;  // strassen_nt from quadrants of this size on; 0: one classical launch
  size_t temp = 0;   // elements of ONE panel buffer: the level's temporaries live in the buffer of that last panel
  int64_t smin2 = 0;        // strassen_nt's second level from quadrants of this size on; 0: one level
  void* temp2 = nullptr;    // its temporaries (the handle's strassen2) and their size in elements
  size_t temp2_elems = 0;
};

// The panel at offset o of an n x n factorisation in panels of nb, and what lies behind it.
struct PanelGeom {
  int64_t o;
  int nbp;         // width of the panel
  int64_t t0;      // first trailing row/col
  int64_t ntrail;  // trailing rows (<= 0: the last panel; o >= n: 0)
  int nbn;         // width of the next panel
  int64_t nrest;   // trailing rows beyond the next panel
  int tile;        // of the trailing update's launches
  PanelGeom(int64_t n, int nb, int64_t o_)
      : o(o_), nbp((int)std::min<int64_t>(nb, n - o)), t0(o + nbp), ntrail(n - t0), nbn((int)std::min<int64_t>(nb, ntrail)),
        nrest(ntrail - nbn), tile((ntrail % 128 == 0 && nbn % 128 == 0) ? 128 : 64) {}
  // does a 128-tile trailing update run beside the look-ahead chain of the panel behind this one?  If not,
  // the chain's small launches are alone on the GPU and take the latency mode of the 64-tile engine.
  bool update_is_big() const { return nrest > 0 && tile == 128 && gemm_nt_tile(128, nrest, nrest, 1) == 128; }
  // can the trailing update of this panel be one fused launch?  (128-tiles for strip and rest)
  bool fusable() const { return update_is_big() && gemm_nt_tile(128, ntrail, nbn, 2) == 128; }
};

// What the three per-panel schedules of chol_enqueue share: its arguments, the streams, and what one panel hands to the
// next.  Built once per factorisation.  Every launch names its LaunchMode; the launchers remember nothing.
template <typename T>
struct CholSched {
  gpx_handle* h;
  T* A;
  int64_t ld, n;
  int nb;
  T* Winv;
  int64_t ldp;
  int* info;
  int64_t gidx0;
  bool profile;
  int64_t nx;
  InvWork<T>* iw;
  const DeferLeft* defer;
  hipStream_t s0, s1;
  T* Pbuf[2];
  bool fuse_env;    // default OFF: measured equal, see DESIGN.md §5.2
  bool top_env;     // GPX_SOLVE_TOP=0: the whole panel solve on the chain (A/B)
  int rest_split;   // trailing rows (in panels) up to which the REST hands its first column block over early
  int64_t nxs, nxc;  // side rows (the main stream's business alone) and the chain's bordered rows: nx = nxc + nxs
  int64_t dna, dc1;  // the deferred product: its rows and the column it starts at (0: none)
  unsigned* ctr;     // the info buffer is 64 bytes: [0] pivot, [8] strip counter
  unsigned target;   // strip slots released so far (fused step)
  hipEvent_t e_main;  // split strip: "the main stream's work on the trailing matrix so far is complete"
  int resv_k;         // GPX_CU_SELF_RESERVE, and the ring of this factorisation (null: off)
  ReserveRing* ring;

  // is the trailing update of the panel g one fused launch?
  bool is_fused(const PanelGeom& g) const { return fuse_env && g.fusable(); }
  // bordered rows [n, n+nx) x trailing columns of the panel g (solved panel in Pc)
  void bordered_update(const PanelGeom& g, const T* Pc, hipStream_t s, LaunchMode lm) const {
    if (nx <= 0 || g.ntrail <= 0) return;
    launch_gemm_nt<T>(nx % 128 == 0 && g.ntrail % 128 == 0 ? 128 : 64, A + n * ld + g.t0, ld, Pc + g.ntrail * ldp, ldp, Pc,
                      ldp, nx, g.ntrail, g.nbp, 0, 0, s, lm);
  }
  // bordered rows [n + r0, n + r0 + nr) x matrix columns [c0, c0 + nc), panel g (split schedule)
  void bordered_block(const PanelGeom& g, const T* Pc, hipStream_t s, int64_t c0, int64_t nc, int64_t r0, int64_t nr,
                      LaunchMode lm) const {
    if (nr <= 0 || nc <= 0) return;
    // many rows plus a 64-row remainder (the left block column of the two-level factorisation with the right-hand
    // sides below it): the 128-multiple in 128-tiles, the remainder in a launch of its own
    const int64_t na = split_rows_128(nr, nc);
    launch_gemm_nt<T>(na % 128 == 0 && nc % 128 == 0 ? 128 : 64, A + (n + r0) * ld + c0, ld, Pc + (g.ntrail + r0) * ldp, ldp,
                      Pc + (c0 - g.t0) * ldp, ldp, na, nc, g.nbp, 0, 0, s, lm);
    if (na < nr)
      launch_gemm_nt<T>(64, A + (n + r0 + na) * ld + c0, ld, Pc + (g.ntrail + r0 + na) * ldp, ldp, Pc + (c0 - g.t0) * ldp, ldp,
                        nr - na, nc, g.nbp, 0, 0, s, lm);
  }
  // side rows of the panel g -> P and back into A
  int side_solve(const PanelGeom& g, T* Pp, hipStream_t s, LaunchMode lm) const {
    if (nxs <= 0) return GPX_OK;
    const int64_t o = g.o;
    const int nbp = g.nbp;
    T* Aside = A + (n + nxc) * ld + o;
    T* Pside = Pp + ((n - o - nbp) + nxc) * ldp;
    if (!iw) {
      launch_trsm_rlt<T>(Aside, ld, nxs, A + o * ld + o, ld, Winv + (o / KB) * (KB * KB), nbp, Pside, ldp, s, lm);
      return GPX_OK;
    }
    HIPCHK(h, hipStreamWaitEvent(s, iw->ready, 0));
    const T* Wp = iw->W + (o / iw->nbw) * (int64_t)iw->nbw * iw->nbw;
    const int64_t na = split_rows_128(nxs, nbp);  // (as bordered_block)
    launch_gemm_nt<T>(na % 128 == 0 && nbp % 128 == 0 ? 128 : 64, Pside, ldp, Aside, ld, Wp, iw->nbw, na, nbp, nbp, 4, 1, s, lm);
    if (na < nxs)
      launch_gemm_nt<T>(64, Pside + na * ldp, ldp, Aside + na * ld, ld, Wp, iw->nbw, nxs - na, nbp, nbp, 4, 1, s, lm);
    launch_copy2d<T>(Aside, ld, Pside, ldp, nxs, nbp, s);
    return GPX_OK;
  }
  // The deferred product (DeferLeft): A[side rows, c1:n) -= L[side rows, 0:c1) L[c1:n, 0:c1)^T for the dna side rows that go
  // out in 128-tiles; the remainder (the right-hand sides) stays right-looking.  lm reaches the classical launches: the
  // one below and strassen_nt's peeled parts, not the level's products.
  void deferred_product(T* Tbuf, hipStream_t s, LaunchMode lm) const {
    T* Cd = A + (n + nxc) * ld + dc1;
    const T *Ad = A + (n + nxc) * ld, *Bd = A + dc1 * ld;
    const int64_t nd = n - dc1, kd = dc1, ldt = kd / 2 + ld_skew<T>();
    // through a Strassen level in row chunks, in a fixed order: the fewest chunks whose temporaries fit the panel buffer,
    // as long as their quadrants are large enough for a level; else one classical launch
    int64_t mch = 0;
    for (int64_t parts = 1; defer->smin > 0 && parts <= dna / 256; ++parts) {
      const int64_t m = round_up((dna + parts - 1) / parts, 256);
      if (std::min(m, nd) / 256 * 128 < defer->smin) break;
      if (strassen_temp_elems(m, nd, kd, ld_skew<T>()) <= defer->temp) {
        mch = m;
        break;
      }
    }
    if (mch == 0) {
      launch_gemm_nt<T>(128, Cd, ld, Ad, ld, Bd, ld, dna, nd, kd, 0, 0, s, lm);
      return;
    }
    const StrassenL2<T> l2{defer->smin2, (T*)defer->temp2, defer->temp2_elems};
    for (int64_t r = 0; r < dna; r += mch) {
      const int64_t m = std::min(mch, dna - r);
      strassen_nt<T>(Cd + r * ld, ld, Ad + r * ld, ld, Bd, ld, m, nd, kd, Tbuf, Tbuf + (m / 256 * 128) * ldt, ldt, s, &l2, nullptr,
                     lm);
    }
  }

  int fused_step(const PanelGeom& g, int step, hipEvent_t e_panel);
  int split_step(const PanelGeom& g, int step, hipEvent_t e_panel);
  int lookahead_step(const PanelGeom& g, int step, hipEvent_t e_panel);
};

// FUSED step (GPX_FUSED_STRIP=1): STRIP and REST of the panel g are one launch; the look-ahead stream is parked on the
// strip counter and then runs diagonal block p+1 and panel p+1 beside the rest of the same launch.
template <typename T>
int CholSched<T>::fused_step(const PanelGeom& g, int step, hipEvent_t e_panel) {
  const int64_t t0 = g.t0, ntrail = g.ntrail, nrest = g.nrest;
  const int nbp = g.nbp, nbn = g.nbn;
  T *Pc = Pbuf[step & 1], *Pn = Pbuf[(step + 1) & 1];  // panel of this step, rows [t0, n + nx), and the next
  const LaunchMode beside{!g.update_is_big()};  // for everything this step enqueues (chain, solve, bordered rows)
  int rc;
  {  // main stream: the whole trailing update, strip first
    PhaseScope ps(h, &h->tm.chol_syrk, profile);
    target += launch_gemm_nt_fused<T>(A + t0 * ld + t0, ld, Pc, ldp, ntrail, nbn, nbp, ctr, s0);
    h->tm.syrk_flops += (double)ntrail * (double)(ntrail + 1) * (double)nbp;
    h->tm.syrk_launches += 1;
  }
  // look-ahead stream: parked until the strip is released, then diagonal block p+1, panel p+1
  launch_wait_counter(ctr, target, info, s1);
  {
    PhaseScope ps(h, &h->tm.chol_diag, profile, s1);
    if ((rc = diag_enqueue(h, A, ld, t0, nbn, Winv, info, gidx0, s1, iw, beside))) return rc;
  }
  {
    PhaseScope ps(h, &h->tm.chol_trsm, profile, s1);
    if ((rc = panel_solve_enqueue(h, A, ld, t0, nbn, nrest, nx, Winv, Pn, ldp, s1, iw, (step + 1) & 1, beside))) return rc;
  }
  HIPCHK(h, hipEventRecord(e_panel, s1));
  const PanelGeom gn(n, nb, t0);
  if (is_fused(gn)) bordered_update(gn, Pn, s1, beside);  // for update p+1: off the chain, beside the rest of update p
  HIPCHK(h, hipStreamWaitEvent(s0, e_panel, 0));
  return GPX_OK;
}

// SPLIT step (round 3, the default), with the deferred product of the two-level factorisation's left block column.
template <typename T>
int CholSched<T>::split_step(const PanelGeom& g, int step, hipEvent_t e_panel) {
  const EnvKnobs& env = h->env;
  const int64_t t0 = g.t0, ntrail = g.ntrail, nrest = g.nrest;
  const int nbp = g.nbp, nbn = g.nbn, tile = g.tile;
  T *Pc = Pbuf[step & 1], *Pn = Pbuf[(step + 1) & 1];  // panel of this step, rows [t0, n + nx), and the next
  hipStream_t sm = s0;
  int rc;
  // self-reserving main-stream products where the chain sets the pace (the criterion of the REST's early hand-over)
  const int resv_it = (resv_k > 0 && (env.resv_all || ntrail <= (int64_t)(rest_split + 1) * nb)) ? resv_k : 0;
  // The modes of this step.  Does a large update run beside its small launches (PanelGeom::update_is_big)?
  const bool latency = !g.update_is_big();
  const LaunchMode beside{latency};                     // the look-ahead stream's products
  const LaunchMode on_main{latency, resv_it, 0, ring};  // everything the main stream runs beside the next diagonal chain
  const LaunchMode on_chain{latency, 0, resv_it > 0 ? env.resv_chain : 0, ring};  // the diagonal chain beside such products
  // SPLIT STRIP (round 3, the default): of the strip only the next DIAGONAL block is on the chain.  It is
  // updated on the look-ahead stream itself, right behind the panel solve that produced its operand (no
  // hand-over between streams on the chain; 64-tiles in latency mode: a K = nb walk of a 64-tile is a
  // quarter of a 128-tile's), after the previous panel's REST (which also touched the block) is complete.
  // The rows BELOW it are needed only by the next panel solve, one diagonal chain later: they are updated
  // on the main stream, beside that chain, followed by the REST.
  if (e_main) HIPCHK(h, hipStreamWaitEvent(s1, e_main, 0));
  {
    PhaseScope ps(h, &h->tm.chol_strip, profile, s1);
    launch_gemm_nt<T>(tile, A + t0 * ld + t0, ld, Pc, ldp, Pc, ldp, nbn, nbn, nbp, 1, 0, s1, beside);
  }
  // the deferred product takes this panel's buffer for its temporaries: behind this launch, its reader on the chain
  hipEvent_t e_stripd = nullptr;
  if (t0 == dc1 && (rc = record_event(h, s1, "deferred product", &e_stripd))) return rc;
  // The host enqueues the main stream's whole iteration BEFORE the diagonal chain's ~50 small launches: the
  // GPU runs the chain about as fast as the host can enqueue it (N = 8192: the update used to reach the GPU
  // 0.5 ms after the panel it needs, and then collided with the NEXT panel solve and diagonal-block update).
  {  // rows below the diagonal block in the next panel's columns; the chain's bordered rows in a small launch
    PhaseScope ps(h, &h->tm.chol_strip, profile, sm);
    if (nrest > 0)
      launch_gemm_nt<T>(tile, A + (t0 + nbn) * ld + t0, ld, Pc + (int64_t)nbn * ldp, ldp, Pc, ldp, nrest, nbn, nbp, 0,
                        0, sm, on_main);
    bordered_block(g, Pc, sm, t0, nbn, 0, nxc, on_main);
  }
  hipEvent_t e_below;
  if ((rc = record_event(h, sm, "look-ahead", &e_below))) return rc;
  // REST.  Where the chain, not the update, sets the pace (the last `rest_split` panels' worth of trailing
  // rows: all of N = 8192, the tail of N = 65536), the column block of the panel AFTER next goes first, as a
  // launch of its own, and the look-ahead stream's next diagonal-block update waits for that launch only:
  // the chain then never waits for the bulk of an update (it used to, for every early panel of N = 8192,
  // where update and chain take about the same time).  The panel buffer this update reads is rewritten two
  // panel solves later, behind the next "rows below" event of this stream, i.e. behind all of this update.
  const int nbn2 = (int)std::min<int64_t>(nb, nrest);
  const bool ahead = nrest > nbn2 && nrest <= (int64_t)rest_split * nb;
  T* Cr = A + (t0 + nbn) * ld + (t0 + nbn);
  const T* Pr = Pc + (int64_t)nbn * ldp;
  if (ahead) {
    {
      PhaseScope ps(h, &h->tm.chol_strip, profile, sm);
      launch_gemm_nt<T>(tile, Cr, ld, Pr, ldp, Pr, ldp, nrest, nbn2, nbp, 2, 0, sm, on_main);
    }
    if ((rc = record_event(h, sm, "look-ahead", &e_main))) return rc;
  }
  const int64_t nr = ahead ? nrest - nbn2 : nrest, off = ahead ? nbn2 : 0;
  if (nr > 0) {
    const bool big = gemm_nt_tile(tile, nr, nr, 1) == 128;
    PhaseScope ps(h, big ? &h->tm.chol_syrk : &h->tm.chol_strip, profile, sm);
    launch_gemm_nt<T>(tile, Cr + off * ld + off, ld, Pr + off * ldp, ldp, Pr + off * ldp, ldp, nr, nr, nbp, 1, 0, sm, on_main);
    if (big) {
      h->tm.syrk_flops += (double)nr * (double)(nr + 1) * (double)nbp;
      h->tm.syrk_launches += 1;
    }
  }
  if (!ahead && (rc = record_event(h, sm, "look-ahead", &e_main))) return rc;
  {  // the bordered rows' share of the REST (columns beyond the next panel); the side rows' whole step — their
     // panel solve and the update of every column to the right — behind everything the chain waits for
    PhaseScope ps(h, &h->tm.chol_strip, profile, sm);
    bordered_block(g, Pc, sm, t0 + nbn, nrest, 0, nxc, on_main);
    if ((rc = side_solve(g, Pc, sm, on_main))) return rc;
    if (g.o < dc1) {
      // deferral: the 128-tile rows only in columns [t0, c1) — in the tiles the whole launch would take, so that
      // those columns receive the same addends bit for bit — and the remainder's launch as it is
      if (dc1 > t0)
        launch_gemm_nt_fixed<T>(gemm_nt_tile(128, dna, ntrail, 0), A + (n + nxc) * ld + t0, ld, Pc + (ntrail + nxc) * ldp, ldp,
                                Pc, ldp, dna, dc1 - t0, nbp, 0, 0, sm, on_main);
      bordered_block(g, Pc, sm, t0, ntrail, nxc + dna, nxs - dna, on_main);
      if (t0 == dc1) {
        // B operand: rows [c1, n) of the panels so far are in A once this panel's copy-back is (the copy stream
        // runs in order).  Temporaries: this panel's buffer, behind its copy-back and behind STRIP_D on the chain;
        // its next writer, the solve of the panel after next, waits for the next "rows below" event of this stream.
        if (iw->copied[step & 1]) HIPCHK(h, hipStreamWaitEvent(sm, iw->copied[step & 1], 0));
        HIPCHK(h, hipStreamWaitEvent(sm, e_stripd, 0));
        deferred_product(Pc, sm, on_main);
      }
    } else {
      bordered_block(g, Pc, sm, t0, ntrail, nxc, nxs, on_main);
    }
  }
  {
    PhaseScope ps(h, &h->tm.chol_diag, profile, s1);
    if ((rc = diag_enqueue(h, A, ld, t0, nbn, Winv, info, gidx0, s1, iw, on_chain))) return rc;
  }
  HIPCHK(h, hipStreamWaitEvent(s1, e_below, 0));
  // Panel solve p+1: only the rows of the NEXT diagonal block (what STRIP_D(p+1) and the B operands need) on the
  // chain; the rows below them, and the chain's bordered rows, on the main stream in front of its next update
  // (their inputs are the main stream's own work plus W_{p+1}) — with the block inverse only.
  const int64_t top = (iw && top_env) ? std::min<int64_t>(nrest, nb) : nrest;
  hipEvent_t prev_copied = iw ? iw->copied[(step + 1) & 1] : nullptr;
  {
    PhaseScope ps(h, &h->tm.chol_trsm, profile, s1);
    if (top < nrest || (iw && top_env)) {
      if ((rc = panel_solve_enqueue(h, A, ld, t0, nbn, top, 0, Winv, Pn, ldp, s1, iw, (step + 1) & 1, beside, 0, prev_copied,
                                    false)))
        return rc;
    } else if ((rc = panel_solve_enqueue(h, A, ld, t0, nbn, nrest, nxc, Winv, Pn, ldp, s1, iw, (step + 1) & 1, beside))) {
      return rc;
    }
  }
  HIPCHK(h, hipEventRecord(e_panel, s1));
  HIPCHK(h, hipStreamWaitEvent(sm, e_panel, 0));
  if (top < nrest || (iw && top_env)) {  // runs beside the NEXT diagonal chain
    PhaseScope ps(h, &h->tm.chol_trsm, profile, sm);
    if ((rc = panel_solve_enqueue(h, A, ld, t0, nbn, nrest - top, nxc, Winv, Pn, ldp, sm, iw, (step + 1) & 1, on_main, top,
                                  prev_copied, true)))
      return rc;
  }
  return GPX_OK;
}

// Round-2 LOOK-AHEAD step (GPX_SPLIT_STRIP=0): the whole STRIP on the main stream, then diagonal block p+1 and panel
// p+1 on the look-ahead stream beside the REST.
template <typename T>
int CholSched<T>::lookahead_step(const PanelGeom& g, int step, hipEvent_t e_panel) {
  const int64_t t0 = g.t0, ntrail = g.ntrail, nrest = g.nrest;
  const int nbp = g.nbp, nbn = g.nbn, tile = g.tile;
  T *Pc = Pbuf[step & 1], *Pn = Pbuf[(step + 1) & 1];  // panel of this step, rows [t0, n + nx), and the next
  const LaunchMode alone{true};                 // the strip runs alone (the look-ahead stream waits for it)
  const LaunchMode beside{!g.update_is_big()};  // everything else this step enqueues (chain, solve, rest)
  int rc;
  {  // STRIP: rows [t0, n) x cols [t0, t0+nbn), tiles on/below the diagonal
    PhaseScope ps(h, &h->tm.chol_strip, profile);
    launch_gemm_nt<T>(tile, A + t0 * ld + t0, ld, Pc, ldp, Pc, ldp, ntrail, nbn, nbp, 2, 0, s0, alone);
    // bordered rows [n, n+nx) x all trailing cols: their own small launch, so that the
    // SYRK grids (and their XCD balance) stay exactly those of the plain factorisation
    bordered_update(g, Pc, s0, beside);
  }
  // the two streams touch the same matrix: an event that cannot be created / recorded /
  // waited on must fail the call, never let the streams run unordered
  if ((rc = stream_waits(h, s1, s0, "look-ahead"))) return rc;
  {  // look-ahead stream: factor diagonal block p+1, solve panel p+1
    {
      PhaseScope ps(h, &h->tm.chol_diag, profile, s1);
      if ((rc = diag_enqueue(h, A, ld, t0, nbn, Winv, info, gidx0, s1, iw, beside))) return rc;
    }
    {
      PhaseScope ps(h, &h->tm.chol_trsm, profile, s1);
      if ((rc = panel_solve_enqueue(h, A, ld, t0, nbn, nrest, nx, Winv, Pn, ldp, s1, iw, (step + 1) & 1, beside))) return rc;
    }
  }
  HIPCHK(h, hipEventRecord(e_panel, s1));
  if (nrest > 0) {  // REST: lower triangle of the trailing matrix beyond the strip
    // the roofline bookkeeping (time, flops, launches) follows ONE kernel, the 128-tile triangular
    // update; the last few, under-filled updates run as 64-tiles and are booked with the strips
    const bool big = gemm_nt_tile(tile, nrest, nrest, 1) == 128;
    PhaseScope ps(h, big ? &h->tm.chol_syrk : &h->tm.chol_strip, profile);
    launch_gemm_nt<T>(tile, A + (t0 + nbn) * ld + (t0 + nbn), ld, Pc + (int64_t)nbn * ldp, ldp,
                      Pc + (int64_t)nbn * ldp, ldp, nrest, nrest, nbp, 1, 0, s0, beside);
    if (big) {
      h->tm.syrk_flops += (double)nrest * (double)(nrest + 1) * (double)nbp;
      h->tm.syrk_launches += 1;
    }
  }
  HIPCHK(h, hipStreamWaitEvent(s0, e_panel, 0));
  return GPX_OK;
}

template <typename T>
int chol_enqueue(gpx_handle* h, T* A, int64_t ld, int64_t n, int nb, T* Winv, T* P0, T* P1,
                 int64_t ldp, int* info, int64_t gidx0, bool profile, int64_t nx = 0,
                 InvWork<T>* iw = nullptr, int64_t nx_side = 0, int rest_split_arg = -1,
                 const DeferLeft* defer = nullptr) {
  hipStream_t s0 = h->st, s1 = h->st2;
  int rc;
  // The schedule is a function of the arguments and the handle: its switches are h->env, the snapshot the call took
  // when it began (gpx_env.h), and nothing below reads the environment.
  const EnvKnobs& env = h->env;
  const bool split_env = split_strip_in_force(h);  // (the fused update keeps its own hand-over)
  CholSched<T> c{};
  c.h = h, c.A = A, c.ld = ld, c.n = n, c.nb = nb, c.Winv = Winv, c.ldp = ldp, c.info = info, c.gidx0 = gidx0;
  c.profile = profile, c.nx = nx, c.iw = iw, c.defer = defer, c.s0 = s0, c.s1 = s1, c.Pbuf[0] = P0, c.Pbuf[1] = P1;
  c.fuse_env = fused_strip_in_force(h);
  c.top_env = env.solve_top;
  // (a caller's own rest_split: the two-level schedule)
  c.rest_split = rest_split_arg >= 0 ? rest_split_arg : env.rest_split;
  c.ctr = reinterpret_cast<unsigned*>(info + 8);
  // The LAST nx_side bordered rows (the query points of gpx_fit_predict: a multiple of 128) are the main stream's
  // business alone in the split schedule: their panel solves, like their updates, are throughput work no step of the
  // chain waits for (tried: a stream of their own that trails the factorisation panel by panel, reading L from A —
  // slower, N = 8192: 12.4 against 11.6 ms; one more stream's worth of serial block solves).  The other bordered
  // rows (the right-hand sides) ride in the chain's panel solves as before.
  c.nxs = split_env ? nx_side : 0, c.nxc = nx - c.nxs;
  // the deferred product's rows: the side rows that go out in 128-tiles (CholSched::deferred_product)
  const int64_t dna0 = (defer && iw && c.nxs > 0 && !c.fuse_env && defer->c1 > 0 && defer->c1 < n && defer->c1 % nb == 0 && n % 128 == 0)
                           ? split_rows_128(c.nxs, n - defer->c1)
                           : 0;
  c.dna = dna0 % 128 == 0 ? dna0 : 0, c.dc1 = c.dna > 0 ? defer->c1 : 0;
  const LaunchMode alone{true};  // panel 0, and the last panel's side rows: nothing runs beside them
  // GPX_CU_SELF_RESERVE = k (round 4): where the chain sets the pace, the main stream's products leave k CUs per XCD to it
  // by themselves (gemm_nt_resv_kernel: persistent grids that exit on the reserved CUs).  Split schedule only.
  // GPX_RESV_ALL=1 (experiment): every panel's main-stream products, not only the chain-bound ones.  GPX_RESV_CHAIN: 0
  // chain untouched, 1 (default) POTF2 padded to 130 KB of LDS, 2 also its slab launches.  GPX_RESV_FORM: the grid of the
  // self-reserving launches (launch_gemm_nt).
  c.resv_k = env.cu_self_reserve;
  ReserveRing ring;  // this factorisation's: `used` counts from 0
  if (c.resv_k > 0 && split_env) {
    if ((rc = ensure(h, h->resv_ring, (size_t)RESV_RING * 8 * sizeof(unsigned)))) return rc;
    HIPCHK(h, hipMemsetAsync(h->resv_ring.p, 0, (size_t)RESV_RING * 8 * sizeof(unsigned), s0));
    ring.ctr = (unsigned*)h->resv_ring.p, ring.cap = RESV_RING, ring.form = env.resv_form;
    c.ring = &ring;
  }
  const PanelGeom g0(n, nb, 0);
  const bool any_fused = c.is_fused(g0);
  if (any_fused) HIPCHK(h, hipMemsetAsync(c.ctr, 0, sizeof(unsigned), s0));
  // prologue: panel 0 on the main stream
  {
    const int nb0 = g0.nbp;
    {
      PhaseScope ps(h, &h->tm.chol_diag, profile);
      if ((rc = diag_enqueue(h, A, ld, 0, nb0, Winv, info, gidx0, s0, iw, alone))) return rc;
    }
    {
      PhaseScope ps(h, &h->tm.chol_trsm, profile);
      if ((rc = panel_solve_enqueue(h, A, ld, 0, nb0, n - nb0, c.nxc, Winv, P0, ldp, s0, iw, 0, alone))) return rc;
    }
    if (any_fused) {
      c.bordered_update(g0, P0, s0, alone);
      if ((rc = stream_waits(h, s1, s0, "look-ahead"))) return rc;  // counter reset + panel 0 before the parked stream's first poll
    }
  }
  if (split_env && n > nb && (rc = record_event(h, s0, "look-ahead", &c.e_main))) return rc;  // panel 0 ran on the main stream
  int step = 0;
  for (int64_t o = 0; o < n; o += nb, ++step) {
    const PanelGeom g(n, nb, o);
    if (g.ntrail <= 0) {  // the last panel: nothing to update, but the side rows still take their solve
      // (alone: the step before it had no REST, and a single panel follows the prologue)
      if ((rc = c.side_solve(g, c.Pbuf[step & 1], s0, alone))) return rc;
      break;
    }
    hipEvent_t e_panel = next_event(h);
    if (!e_panel) return fail(h, GPX_E_HIP, "hipEventCreate failed (look-ahead)");
    rc = c.is_fused(g) ? c.fused_step(g, step, e_panel) : split_env ? c.split_step(g, step, e_panel) : c.lookahead_step(g, step, e_panel);
    if (rc) return rc;
  }
  if (iw) {  // join the side and copy streams: the last inverse and every panel copy-back are in W / A
    for (hipStream_t sj : {iw->aux, h->st4})
      if ((rc = stream_waits(h, s0, sj, "join"))) return rc;
  }
  return GPX_OK;
}

// ---- two-level Cholesky: the arguments of chol_enqueue ---------------------------------------
// The matrix is split at the panel boundary c nearest n / 2, and from n >= GPX_TWO_LEVEL_FROM on (0: never) the
// factorisation runs as
//   1. chol_enqueue of the left block column: A11 = L11 L11^T with rows [c, n + nx) — A21 and the bordered rows — as
//      its bordered rows.  They go in as SIDE rows (nx_side: all of them): the side rows' panel solves and updates are
//      the main stream's throughput work that no step of the chain waits for, which is what A21 is; the chain's rows
//      must come first among the bordered rows and the right-hand sides lie BELOW A21, so those ride as side rows too.
//   2. A22 -= L21 L21^T in ONE update at K = c (the deep update: main stream), beside it on the look-ahead stream the
//      bordered rows' columns [c, n) (a long serial walk of few tiles), joined before 3.
//   3. chol_enqueue of A22 with the bordered rows, pivots counted from gidx0 + c; block inverses, panel buffers and the
//      step flag as gpx_append's restart takes them (a fresh InvWork: the flag is reset in front of its first block).
// With GPX_STRASSEN_MIN > 0 the off-diagonal block of the deep update — rows [hh, np) x columns [0, hh) of A22, hh = half
// of np = n - c in whole 128-tiles — goes through strassen_nt when its quadrants are at least that large, the two
// diagonal halves stay classical triangular launches; GPX_STRASSEN_DIAG splits the two halves once more in the same way.
// The deep update is booked under chol_syrk, syrk_flops counting the flops executed.
template <typename T>
int chol_two_level_enqueue(gpx_handle* h, T* A, int64_t ld, int64_t n, int nb, T* Winv, T* P0, T* P1, int64_t ldp,
                           int* info, int64_t gidx0, bool profile, int64_t nx = 0, InvWork<T>* iw = nullptr,
                           int64_t nx_side = 0) {
  const EnvKnobs& env = h->env;
  const int64_t c = std::max<int64_t>(1, (n / 2 + nb / 2) / nb) * nb, np = n - c;
  // The temporaries of the Strassen levels are the two panel buffers — P0 and P1 are the halves of ONE allocation
  // [P0, P0 + 2 (P1 - P0)), idle between phase 1 and phase 3 (everything that read or wrote them is ordered in front of
  // the main stream's next launch when chol_enqueue returns) — so the level costs no memory.  They hold the level of
  // Npad = 65536 at 2048-wide panels and nothing larger (Npad <= 32 nb): beyond that, and in fp32 unless
  // GPX_STRASSEN_SINGLE says otherwise (the variance at full size), the one-level schedule, as
  // wherever the split has no level to enable (by itself it only costs).
  const int64_t smin = env.strassen_min;
  const int depth = smin > 0 ? (env.strassen_diag ? 2 : 1) : 0;
  const int64_t hh = np / 2 / 128 * 128, ldt = c / 2 + ld_skew<T>();
  const bool fits = P1 > P0 && strassen_temp_elems(np - hh, hh, c, ld_skew<T>()) <= 2 * (size_t)(P1 - P0);
  const bool wanted = depth == 0 || (fits && (sizeof(T) == 8 || env.strassen_f32));
  if (env.two_level_from <= 0 || n < env.two_level_from || !iw || nx_side != 0 || np < 256 || n % 128 != 0 || nb % 128 != 0 ||
      (nx != 0 && nx != RHS_ROWS) || !wanted)
    return chol_enqueue<T>(h, A, ld, n, nb, Winv, P0, P1, ldp, info, gidx0, profile, nx, iw, nx_side);
  int rc;
  hipStream_t s0 = h->st, s1 = h->st2;
  T *TA = P0, *TB = nullptr;
  // 1. the left block column
  // (each phase has half the panels, and in phase 1 the side rows keep the main stream busy beside the chain: the REST's
  //  early hand-over — GPX_REST_SPLIT, tuned on the one-level schedule — from half as many trailing panels on; N = 65536:
  //  1513.3 against 1521.6 ms)
  const int rs = env.rest_split / 2;
  // GPX_DEFER_LEFT: the panels left of c1 — the panel boundary nearest c / 2, at least one panel on each side — leave
  // A21's columns [c1, c) alone, and one product at K = c1 (large in all three dimensions: a Strassen level pays, which
  // it cannot at K = nb) makes up for it.  Unset: on where the level is; 1 with the level off: a classical product.
  DeferLeft defer;
  defer.c1 = std::min<int64_t>(std::max<int64_t>(1, (c / 2 + nb / 2) / nb) * nb, c - nb);
  defer.smin = depth > 0 ? smin : 0;
  defer.temp = (size_t)(P1 - P0);
  const bool defer_on = (env.defer_left < 0 ? depth > 0 : env.defer_left != 0) && defer.c1 > 0;
  // The second level's temporaries (GPX_STRASSEN_MIN_TWO): ONE buffer of the handle's, sized here, before anything is
  // enqueued, for the larger of its two users — the deep update's off-diagonal block and the deferred product's largest
  // chunk run on the main stream one after the other.  Without it (no memory left) the second level does not run.
  StrassenL2<T> l2;
  if (depth > 0 && env.strassen_min2 > 0 && sizeof(T) == 8) {  // (fp64 only, whatever GPX_STRASSEN_SINGLE says)
    auto quadrants2 = [](int64_t m, int64_t nn) { return std::min(m, nn) / 256 * 128 / 256 * 128; };
    size_t need = 0;
    if (quadrants2(np - hh, hh) >= env.strassen_min2) need = strassen_temp2_elems<T>(np - hh, hh, c);
    if (defer_on && quadrants2(np, c - defer.c1) >= env.strassen_min2)
      need = std::max(need, strassen_temp2_elems<T>(round_up(np, 256), c - defer.c1, defer.c1));
    if (need > 0 && try_ensure(h, h->strassen2, need * sizeof(T))) {
      l2.min2 = env.strassen_min2;
      l2.buf = (T*)h->strassen2.p;
      l2.elems = h->strassen2.cap / sizeof(T);
    }
  }
  defer.smin2 = l2.min2;
  defer.temp2 = l2.buf;
  defer.temp2_elems = l2.elems;
  if ((rc = chol_enqueue<T>(h, A, ld, c, nb, Winv, P0, P1, ldp, info, gidx0, profile, np + nx, iw, np + nx, rs,
                            defer_on ? &defer : nullptr)))
    return rc;
  // 2. the deep update
  T* A22 = A + c * ld + c;
  const T* L21 = A + c * ld;
  hipEvent_t e_rows = nullptr;
  if (nx > 0) {
    if ((rc = stream_waits(h, s1, s0, "deep update"))) return rc;
    PhaseScope ps(h, &h->tm.chol_strip, profile, s1);
    launch_gemm_nt<T>(64, A + n * ld + c, ld, A + n * ld, ld, L21, ld, nx, np, c, 0, 0, s1);
    if ((rc = record_event(h, s1, "deep update", &e_rows))) return rc;
  }
  {
    PhaseScope ps(h, &h->tm.chol_syrk, profile);
    // rows and columns [o, o + sz) of A22, lower triangle; `lv` levels of splitting left
    std::function<void(int64_t, int64_t, int)> deep = [&](int64_t o, int64_t sz, int lv) {
      const int64_t s1z = sz / 2 / 128 * 128, s2z = sz - s1z;
      if (lv <= 0 || s1z < 256 || std::min(s1z, s2z) / 256 * 128 < smin) {
        launch_gemm_nt<T>(128, A22 + o * ld + o, ld, L21 + o * ld, ld, L21 + o * ld, ld, sz, sz, c, 1, 0, s0);
        h->tm.syrk_flops += (double)sz * (double)(sz + 1) * (double)c;
        h->tm.syrk_launches += 1;
        return;
      }
      deep(o, s1z, lv - 1);
      TB = TA + (s2z / 256 * 128) * ldt;
      bool two = false;
      h->tm.syrk_flops += strassen_nt<T>(A22 + (o + s1z) * ld + o, ld, L21 + (o + s1z) * ld, ld, L21 + o * ld, ld, s2z, s1z,
                                         c, TA, TB, ldt, s0, &l2, &two);
      h->tm.syrk_launches += two ? 49 : 7;
      deep(o + s1z, s2z, lv - 1);
    };
    deep(0, np, depth);
  }
  if (e_rows) HIPCHK(h, hipStreamWaitEvent(s0, e_rows, 0));
  // 3. the right block
  InvWork<T> iw2;
  iw2.W = iw->W + (c / iw->nbw) * (int64_t)iw->nbw * iw->nbw;
  iw2.U = iw->U;
  iw2.ldu = iw->ldu;
  iw2.nbw = iw->nbw;
  iw2.aux = iw->aux;
  rc = chol_enqueue<T>(h, A22, ld, np, nb, Winv + (c / KB) * (KB * KB), P0, P0 + (np + nx) * ldp, ldp, info, gidx0 + c, profile,
                       nx, &iw2, 0, rs);
  iw->seq = iw2.seq;
  return rc;
}

// XT (rows x n, ld) <- XT * L^-T   (i.e. X <- L^-1 X for X = XT^T), block forward substitution.
// With many right-hand sides (rows >= 128: the variance TRSM) the same one-panel
// look-ahead as the factorisation: the update of block p is split into the STRIP (the
// columns of block p+1) and the REST; the high-priority stream solves block p+1 while
// the main stream runs the rest of update p (disjoint columns of XT).
template <typename T>
struct SolveWork {       // optional: explicit block inverses + two compact result buffers (rows x ldt)
  const T* W = nullptr;
  int nbw = 0;
  T *T0 = nullptr, *T1 = nullptr;
  int64_t ldt = 0;
};

template <typename T>
int solve_fwd_enqueue(gpx_handle* h, T* XT, int64_t rows, const T* L, int64_t ld, int64_t n, int nb,
                      const T* Winv, const SolveWork<T>* wb = nullptr) {
  hipStream_t s0 = h->st, s1 = h->st2;
  const int tile = (rows % 128 == 0) ? 128 : 64;
  const LaunchMode alone{true};  // one stream, nothing beside it; below: until a large update runs beside the block solves
  if (rows < 128 || !s1) {
    for (int64_t o = 0; o < n; o += nb) {
      const int nbp = (int)std::min<int64_t>(nb, n - o);
      launch_trsm_rlt<T>(XT + o, ld, rows, L + o * ld + o, ld, Winv + (o / KB) * (KB * KB), nbp, nullptr,
                         0, s0, alone);
      const int64_t ntrail = n - (o + nbp);
      if (ntrail > 0)
        launch_gemm_nt<T>((ntrail % 128 == 0) ? tile : 64, XT + o + nbp, ld, XT + o, ld,
                          L + (o + nbp) * ld + o, ld, rows, ntrail, nbp, 0, 0, s0, alone);
    }
    return GPX_OK;
  }
  // With the explicit block inverses of the factorisation (h->Wblk, same block width) a block
  // solve is one dense product into a compact buffer Ts (which then also serves as the A operand
  // of the updates) instead of the slab kernel's serial walk; the copy back into XT runs on the
  // auxiliary stream.
  const bool dense = wb && wb->nbw == nb && wb->T0 && h->st4;
  T* Ts[2] = {dense ? wb->T0 : nullptr, dense ? wb->T1 : nullptr};
  hipEvent_t e_copy[2] = {nullptr, nullptr};
  const int64_t ldt = dense ? wb->ldt : 0;
  auto block_solve = [&](int64_t o, int nbp, int set, hipStream_t s, LaunchMode lm) -> int {
    if (!dense) {
      launch_trsm_rlt<T>(XT + o, ld, rows, L + o * ld + o, ld, Winv + (o / KB) * (KB * KB), nbp, nullptr, 0, s, lm);
      return GPX_OK;
    }
    if (e_copy[set]) HIPCHK(h, hipStreamWaitEvent(s, e_copy[set], 0));  // Ts[set] is free again
    launch_gemm_nt<T>((rows % 128 == 0 && nbp % 128 == 0) ? 128 : 64, Ts[set], ldt, XT + o, ld,
                      wb->W + (o / nb) * (int64_t)nb * nb, nb, rows, nbp, nbp, 4, 1, s, lm);
    hipEvent_t e = next_event(h);
    e_copy[set] = next_event(h);
    if (!e || !e_copy[set]) return fail(h, GPX_E_HIP, "hipEventCreate failed (block solve)");
    HIPCHK(h, hipEventRecord(e, s));
    HIPCHK(h, hipStreamWaitEvent(h->st4, e, 0));
    launch_copy2d<T>(XT + o, ld, Ts[set], ldt, rows, nbp, h->st4);
    HIPCHK(h, hipEventRecord(e_copy[set], h->st4));
    return GPX_OK;
  };
  int rc;
  if ((rc = block_solve(0, (int)std::min<int64_t>(nb, n), 0, s0, alone))) return rc;
  int step = 0;
  for (int64_t o = 0; o < n; o += nb, ++step) {
    const int nbp = (int)std::min<int64_t>(nb, n - o);
    const int64_t t0 = o + nbp, ntrail = n - t0;
    if (ntrail <= 0) break;
    const int nbn = (int)std::min<int64_t>(nb, ntrail);
    const int64_t nrest = ntrail - nbn;
    const int tl = (nbn % 128 == 0 && nrest % 128 == 0) ? tile : 64;
    const int cur = step & 1;
    const T* Ablk = dense ? Ts[cur] : XT + o;  // the solved block o (rows x nbp)
    const int64_t lda = dense ? ldt : ld;
    // the STRIP runs alone: the look-ahead stream waits for it, the previous REST is over
    launch_gemm_nt<T>(tl, XT + t0, ld, Ablk, lda, L + t0 * ld + o, ld, rows, nbn, nbp, 0, 0, s0, alone);  // STRIP
    const LaunchMode beside{!(nrest > 0 && gemm_nt_tile(tl, rows, nrest, 0) == 128)};  // a 128-tile REST runs beside block p+1's solve
    hipEvent_t e_strip = next_event(h), e_panel = next_event(h);
    if (!e_strip || !e_panel) return fail(h, GPX_E_HIP, "hipEventCreate failed (look-ahead)");
    HIPCHK(h, hipEventRecord(e_strip, s0));
    HIPCHK(h, hipStreamWaitEvent(s1, e_strip, 0));
    if ((rc = block_solve(t0, nbn, cur ^ 1, s1, beside))) return rc;
    HIPCHK(h, hipEventRecord(e_panel, s1));
    if (nrest > 0)  // REST
      launch_gemm_nt<T>(tl, XT + t0 + nbn, ld, Ablk, lda, L + (t0 + nbn) * ld + o, ld, rows, nrest, nbp, 0, 0,
                        s0, beside);
    HIPCHK(h, hipStreamWaitEvent(s0, e_panel, 0));
  }
  if (dense) {  // every block is back in XT
    for (int set = 0; set < 2; ++set)
      if (e_copy[set]) HIPCHK(h, hipStreamWaitEvent(s0, e_copy[set], 0));
  }
  return GPX_OK;
}

// XT (rows x n, ld) <- XT * L^-1   (X <- L^-T X), block back substitution; rows multiple of 64
template <typename T>
void solve_bwd_enqueue(gpx_handle* h, T* XT, int64_t rows, const T* L, int64_t ld, int64_t n, int nb,
                       const T* Winv) {
  hipStream_t st = h->st;
  int64_t last = ((n - 1) / nb) * nb;
  for (int64_t o = last; o >= 0; o -= nb) {
    const int nbp = (int)std::min<int64_t>(nb, n - o);
    launch_trsm_rln<T>(XT + o, ld, rows, L + o * ld + o, ld, Winv + (o / KB) * (KB * KB), nbp, st);
    if (o > 0) launch_gemm_nn<T>(XT, ld, XT + o, ld, L + o * ld, ld, rows, o, nbp, st);
  }
}

int copy_in(gpx_handle* h, void* dst, const void* src, size_t bytes, int mem_kind) {
  if (bytes == 0) return GPX_OK;
  // group members: a device pointer of the caller lives on ONE of the group's devices
  const hipMemcpyKind kind = mem_kind == GPX_MEM_HOST ? hipMemcpyHostToDevice
                             : h->in_group            ? hipMemcpyDefault
                                                      : hipMemcpyDeviceToDevice;
  HIPCHK(h, hipMemcpyAsync(dst, src, bytes, kind, h->st));
  return GPX_OK;
}

int copy_out(gpx_handle* h, void* dst, const void* src, size_t bytes, int mem_kind) {
  if (bytes == 0) return GPX_OK;
  HIPCHK(h, hipMemcpyAsync(dst, src, bytes,
                           mem_kind == GPX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           h->st));
  return GPX_OK;
}

// Rows of K* / V^T per batch of query points.  Query rows are independent, so predicting in
// batches is numerically identical to one pass; the V^T buffer is the only O(M N) allocation
// of predict (M = 65536 at N = 131072 would be 69 GB beside the 137 GB factor), so it is capped:
// GPX_PRED_BATCH rows (default 8192, a multiple of 128), and — where every rank decides for
// itself (no collective inside the batch loop) — shrunk to what the card has left.
int64_t pred_batch_rows(gpx_handle* h, int64_t Mpad, size_t row_bytes, bool may_shrink) {
  int64_t cap = h->env.pred_batch;
  if (may_shrink) {
    size_t freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
      const double avail = 0.8 * ((double)freeb + (double)h->scr.VT.cap);
      const int64_t fit = (int64_t)(avail / (double)row_bytes) / 128 * 128;
      cap = std::max<int64_t>(128, std::min(cap, fit));
    }
  }
  return std::min(cap, Mpad);
}

// Panel width the library picks when gpx_config.block == 0 (round 4).  Rounds 1-3 swept 256 ... 2048 and found a plateau
// from 1024 — with the diagonal chain partly exposed.  On the round-3/4 schedule nothing of the chain is exposed at large
// N, and a 2048-wide panel halves the number of trailing updates (K = 2048 per tile: the per-tile prologue + epilogue
// weigh half as much, 72.4 against 71.7 TF) and of block steps of the variance solve: C3 1602-1605 -> 1579-1584 ms, C5 fp32
// 881 -> 859 ms; equal at N = 16384 ... 32768, slower at N = 8192 where the chain sets the pace (12.5 vs 13.2 ms):
// tools/r04_nb_sweep.sh, profiles/r04_panel_width.txt.  GPX_NB_WIDE_FROM = rows from which 2048 is used (0: never).
int auto_panel_width(const gpx_handle* h, int64_t Npad) {
  const int64_t from = h->env.nb_wide_from;
  return (from > 0 && Npad >= from) ? 2048 : 1024;
}

// ---- stages every entry point is built from --------------------------------------------------------
// None of them reads the environment — begin_call has taken the call's snapshot of it, h->env, and that is what they and
// everything below them consult — allocates beyond the ensure() it names or synchronises beyond what it says.

// The call entries of the environment (gpx_env.h) into the handle: by begin_call — the rank handles of a device group
// and handles with a communicator come through it as well (their entry points are the single-device ones) — and by
// the three places that enqueue without it: gpx_get_alpha, the unit-test entry points' Scratch, create_group.
void refresh_env(gpx_handle* h) { env_read(h->env, EnvAt::call); }

// the start of a call on one handle (a single-device one, a rank of a device group, one with a communicator)
int begin_call(gpx_handle* h) {
  refresh_env(h);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  h->err.clear();
  h->phases.clear();  // an earlier call that failed mid-way must not leak its event pairs
  h->ev_used = 0;
  return GPX_OK;
}

int begin_fit(gpx_handle* h) {  // ... of a call that replaces the fit
  const int rc = begin_call(h);
  if (rc == GPX_OK) {
    h->fitted = false;
    h->basis = h->bp = 0;  // (fit_impl decides; the other engines never fit with a basis: check_fit_basis)
    h->pw = {};            // a stored pathwise draw belongs to the fit it was drawn against
    if (h->sp.fitted || h->sp.L.p) {  // a dense fit replaces an inducing-point fit: its state leaves with it
      HIPCHK(h, hipDeviceSynchronize());
      h->sp = {};
    }
  }
  return rc;
}

// the end of a call: the main stream idle, nothing failed on the way, the phase clocks folded into gpx_timings
int finish_call(gpx_handle* h) {
  HIPCHK(h, hipStreamSynchronize(h->st));
  HIPCHK(h, hipGetLastError());
  LAUNCHCHK(h);
  collect_phases(h);
  return GPX_OK;
}

void reset_predict_clocks(gpx_timings& tm) { tm.kstar = tm.mean = tm.trsm = tm.var = tm.d2h = tm.predict_total = 0; }

// T = float for GPX_F32 handles, double otherwise (GPX_MIXED is dispatched before: its entry points are not templates)
#define BY_DTYPE(h, fn, ...) ((h)->cfg.dtype == GPX_F32 ? fn<float>(__VA_ARGS__) : fn<double>(__VA_ARGS__))

// room for M query points: Q (M x d, as given) and Qs (padded to whole tiles, scaled by the length scales)
template <typename T>
int ensure_queries(gpx_handle* h, int64_t M) {
  int rc;
  if ((rc = ensure(h, h->scr.Q, (size_t)M * h->d * sizeof(T)))) return rc;
  return ensure(h, h->scr.Qs, (size_t)round_up(M, TILE) * h->d * sizeof(T));
}

// the query points into Q and, scaled, into Qs — inside the caller's phase (predict books it under kstar, a fit that
// carries query rows under kbuild)
template <typename T>
int upload_queries(gpx_handle* h, const void* Xq, int64_t M, int32_t mem_kind) {
  int rc;
  if ((rc = copy_in(h, h->scr.Q.p, Xq, (size_t)M * h->d * sizeof(T), mem_kind))) return rc;
  launch_scale_points<T>((const T*)h->scr.Q.p, M, round_up(M, TILE), h->d, (const double*)h->ls.p, h->n_ls, (T*)h->scr.Qs.p,
                         h->st);
  return GPX_OK;
}

// The query points' path ids (the *_paths calls; gq in the memory kind of the query points) into Qg next to Qs, -1 from M
// to the padded size: the GROUPS builders read the ids of whole tiles.  Inside the caller's phase, as upload_queries.
int upload_query_ids(gpx_handle* h, const int32_t* gq, int64_t M, int32_t mem_kind) {
  const int64_t Mpad = round_up(M, TILE);
  int rc;
  if ((rc = ensure(h, h->scr.Qg, (size_t)Mpad * sizeof(int32_t)))) return rc;
  HIPCHK(h, hipMemsetAsync(h->scr.Qg.p, 0xFF, (size_t)Mpad * sizeof(int32_t), h->st));  // -1
  return copy_in(h, h->scr.Qg.p, gq, (size_t)M * sizeof(int32_t), mem_kind);
}

// Dense block solves for solve_fwd_enqueue over `rows` rows: the fit's explicit block inverses and two compact result
// buffers in `buf`.  *sw stays empty (slab solves) when the solve's block width is not the inverses' or the handle keeps
// no whole factor.
template <typename T>
int dense_solve_work(gpx_handle* h, DevBuf& buf, int64_t rows, SolveWork<T>* sw) {
  if (h->nbw != h->nb_pred || (h->comm && !h->repl)) return GPX_OK;
  int rc;
  sw->ldt = h->nbw + ld_skew<T>();
  if ((rc = ensure(h, buf, (size_t)2 * rows * sw->ldt * sizeof(T)))) return rc;
  sw->W = (const T*)h->Wblk.p;
  sw->nbw = h->nbw;
  sw->T0 = (T*)buf.p;
  sw->T1 = sw->T0 + rows * sw->ldt;
  return GPX_OK;
}

// mean^T (64 x cols, ldm) = rhs^T (64 x Npad) * V for V^T (cols x Npad), both with the factor's leading dimension: a
// 64-row product with K = N, so the contraction is split when that fills the chip (part: [splits][64][ldpart])
template <typename T>
void mean_product(gpx_handle* h, T* MT, int64_t ldm, const T* rhsT, const T* VT, int64_t cols, T* part, int64_t ldpart) {
  const int ksplit = splitk_splits(h->Npad);
  if (ksplit > 1)
    launch_gemm_nt_splitk<T>(MT, ldm, rhsT, h->ld, VT, h->ld, RHS_ROWS, cols, h->Npad, ksplit, part, ldpart, h->st);
  else
    launch_gemm_nt<T>(64, MT, ldm, rhsT, h->ld, VT, h->ld, RHS_ROWS, cols, h->Npad, 0, 1, h->st);
}

template <typename T>
int ensure_mean_partials(gpx_handle* h, DevBuf& part, int64_t ldpart) {  // (nothing when mean_product does not split)
  const int ksplit = splitk_splits(h->Npad);
  return ksplit > 1 ? ensure(h, part, (size_t)ksplit * RHS_ROWS * ldpart * sizeof(T)) : GPX_OK;
}

// The predict half of a fit that carried query points as bordered rows: V^T (rows valid of rows_pad, leading dimension
// h->ld) is in place; what is left is the mean V^T z (h->meanout) and, with want_var, the row norms (h->var).  The caller
// has ensured MT / MTpart (leading dimension ldm) and the two outputs.
template <typename T>
void bordered_mean_var(gpx_handle* h, const T* VT, int64_t rows, int64_t rows_pad, int64_t ldm, bool want_var) {
  {
    PhaseScope ps(h, &h->tm.mean);
    mean_product<T>(h, (T*)h->scr.MT.p, ldm, (const T*)h->zT, VT, rows_pad, (T*)h->scr.MTpart.p, ldm);
    launch_unpack_rhs<T>((const T*)h->scr.MT.p, ldm, rows, h->k, 1.0, (T*)h->meanout.p, h->st);
  }
  if (want_var) {
    PhaseScope ps(h, &h->tm.var);
    launch_var_rows<T>(VT, h->ld, rows, h->Npad, h->sf2, (T*)h->var.p, h->st);
  }
  if (h->bp) {  // (single-device fits only; the query points of the fused predict sit in scr.Q)
    PhaseScope ps(h, want_var ? &h->tm.var : &h->tm.mean);
    launch_basis_epilogue<T>((const double*)h->Bst.p, h->bp, h->k, h->d, (const T*)h->scr.MT.p, ldm, (const T*)h->scr.Q.p, rows,
                             (T*)h->meanout.p, want_var ? (T*)h->var.p : nullptr, nullptr, h->st);
  }
}

// h->meanout (M x k) and, if asked for, h->var (M) to the caller
template <typename T>
int deliver_mean_var(gpx_handle* h, void* mean, void* var, int64_t M, int32_t mem_kind) {
  PhaseScope ps(h, &h->tm.d2h);
  int rc;
  if ((rc = copy_out(h, mean, h->meanout.p, (size_t)M * h->k * sizeof(T), mem_kind))) return rc;
  return var ? copy_out(h, var, h->var.p, (size_t)M * sizeof(T), mem_kind) : GPX_OK;
}

template <typename T>
int predict_core(gpx_handle* h, const void* Xq, int64_t M, bool want_var, int32_t mem_kind, const int32_t* gq = nullptr);
bool few_solver_applies(const gpx_handle* h);
template <typename T>
int solve_few(gpx_handle* h, T* RT, int k, const T* L, int64_t ld, int64_t n, const T* W, int nb, bool forward = true,
              bool backward = true);

}  // namespace

#include "gpx_shard.inc"
#include "gpx_group.inc"

namespace {

// The weights of the fit that begins: a copy of what gpx_set_noise_weights stored (the fit keeps its own: a later
// gpx_set_noise_weights does not touch it), in the engine's element type T; none set: nothing happens here.
template <typename T>
int stage_fit_weights(gpx_handle* h, int64_t N, int64_t cap) {
  h->weighted = false;
  if (h->nw_set == 0) return GPX_OK;
  int rc;
  if ((rc = ensure(h, h->Wfit, (size_t)cap * sizeof(T)))) return rc;
  if (h->cfg.dtype == GPX_MIXED) {  // T = float: the fp32 factorisation; the fp64 copy serves the refinement
    if ((rc = ensure(h, h->Wfit64, (size_t)cap * 8))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->Wfit64.p, h->Wset.p, (size_t)N * 8, hipMemcpyDeviceToDevice, h->st));
    launch_f64_to_f32((const double*)h->Wfit64.p, (float*)h->Wfit.p, N, h->st);
  } else {
    HIPCHK(h, hipMemcpyAsync(h->Wfit.p, h->Wset.p, (size_t)N * sizeof(T), hipMemcpyDeviceToDevice, h->st));
  }
  h->weighted = true;
  return GPX_OK;
}

// The kinds of the fit that begins, as stage_fit_weights: the fit keeps its own copy (host and device, -1 beyond N up to the
// capacity) and the finished diagonal terms (kind_i < 0 ? sn2 : sn2_deriv) w_i + jitter; none set: nothing happens here.
// Matern-1/2 (all kinds are -1 then: check_fit_kinds) has no KINDS builders and needs none: it is the plain model.
template <typename T>
int stage_fit_kinds(gpx_handle* h, int64_t N, int64_t cap, double sn2, double jitter) {
  h->kinded = h->has_deriv = false;
  if (h->kinds_set.empty() || !cov::differentiable(h->cfg.kernel)) return GPX_OK;
  int rc;
  if ((rc = ensure(h, h->Kfit, (size_t)cap * sizeof(int32_t)))) return rc;
  if ((rc = ensure(h, h->Dfit, (size_t)cap * sizeof(T)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->st));  // (kinds_fit is the source of an asynchronous copy of the fit before)
  h->kinds_fit = h->kinds_set;
  h->sn2_deriv = h->sn2_deriv_set;
  HIPCHK(h, hipMemsetAsync(h->Kfit.p, 0xFF, (size_t)cap * sizeof(int32_t), h->st));  // -1
  HIPCHK(h, hipMemcpyAsync(h->Kfit.p, h->kinds_fit.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
  launch_kinds_diag<T>((const int32_t*)h->Kfit.p, h->weighted ? (const T*)h->Wfit.p : nullptr, N, sn2, h->sn2_deriv, jitter,
                       (T*)h->Dfit.p, h->st);
  h->kinded = true;
  for (int32_t kk : h->kinds_fit) h->has_deriv |= kk >= 0;
  return GPX_OK;
}

// does the next fit take the GROUPS builder?  Path ids set, one of them >= 0, and sg2 > 0: anything else is the plain model
bool groups_effective(const gpx_handle* h) {
  if (h->groups_set.empty() || !(h->sg2_set > 0.0)) return false;
  for (int32_t g : h->groups_set)
    if (g >= 0) return true;
  return false;
}

// The path ids of the fit that begins, as stage_fit_kinds: the fit keeps its own copy (host and device, -1 beyond N up to
// the capacity), q_c = (l_c / l_path,c)^2 and the finished diagonal terms sn2 w_i + jitter; not effective: nothing happens here.
template <typename T>
int stage_fit_groups(gpx_handle* h, int64_t N, int64_t cap, int d, const double* lengthscale, int n_ls, double sn2,
                     double jitter) {
  h->grouped = false;
  if (!groups_effective(h)) return GPX_OK;
  int rc;
  if ((rc = ensure(h, h->Gfit, (size_t)cap * sizeof(int32_t)))) return rc;
  if ((rc = ensure(h, h->Gdiag, (size_t)cap * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Gq, MAX_D * 8))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->st));  // (groups_fit and q_fit are the sources of asynchronous copies of the fit before)
  h->groups_fit = h->groups_set;
  h->sg2 = h->sg2_set;
  h->n_lsp = (int)h->lsp_set.size();
  h->q_fit.assign((size_t)d, 0.0);
  for (int c = 0; c < d; ++c) {
    const double r = lengthscale[n_ls == 1 ? 0 : c] / h->lsp_set[h->lsp_set.size() == 1 ? 0 : c];
    h->q_fit[c] = r * r;
  }
  HIPCHK(h, hipMemsetAsync(h->Gfit.p, 0xFF, (size_t)cap * sizeof(int32_t), h->st));  // -1
  HIPCHK(h, hipMemcpyAsync(h->Gfit.p, h->groups_fit.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(h->Gq.p, h->q_fit.data(), (size_t)d * 8, hipMemcpyHostToDevice, h->st));
  launch_kinds_diag<T>((const int32_t*)h->Gfit.p, h->weighted ? (const T*)h->Wfit.p : nullptr, N, sn2, sn2, jitter,
                       (T*)h->Gdiag.p, h->st);
  h->grouped = true;
  return GPX_OK;
}

// K* of value rows As (m valid of mpad) against the training set of the current fit: the KINDS builder on a fit with kinds
// (a fit with path ids takes the plain builder: query rows are values of f, and Cov[f(x*), y_i] = sf2 k(x*, x_i)).
// ga != null (a fit with path ids; readable up to mpad, -1 beyond m): row i with ga[i] >= 0 is a value of f + g_p of that
// path, and the GROUPS builder adds sg2 k(x*, x_i; l_path) where the ids match.
template <typename T>
void kbuild_cross_fit(gpx_handle* h, const T* As, int64_t m, int64_t mpad, T* K, int64_t ld, const int32_t* ga = nullptr) {
  if (ga)
    launch_kbuild_cross_g<T>(h->cfg.kernel, As, ga, m, mpad, (const T*)h->Xs.p, (const int32_t*)h->Gfit.p, h->N, h->Npad,
                             h->d, h->sf2, (const double*)h->Gq.p, h->sg2, K, ld, h->st);
  else if (h->kinded)
    launch_kbuild_cross_k<T>(h->cfg.kernel, As, m, mpad, (const T*)h->Xs.p, h->N, h->Npad, h->d, h->sf2,
                             (const int32_t*)h->Kfit.p, (const double*)h->ls.p, h->n_ls, K, ld, h->st);
  else
    launch_kbuild_cross<T>(h->cfg.kernel, As, m, mpad, (const T*)h->Xs.p, h->N, h->Npad, h->d, h->sf2, K, ld, h->st);
}

// Xq != null (gpx_fit_predict): the M query points' cross-kernel rows K* ride through the factorisation as
// bordered rows too — below the right-hand sides — and leave it as
// V^T = (L^-1 K*^T)^T: the variance solve of predict costs no pass of its own (its M N^2 flops are rows of
// the trailing updates, which at small N fill the CUs the serial diagonal chain leaves idle).
template <typename T>
int fit_impl(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
             const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
             int32_t mem_kind, int64_t* info, const void* Xq = nullptr, int64_t M = 0, bool retried = false) {
  const int64_t Npad = round_up(N, TILE);
  const int64_t Mpad = Xq ? round_up(M, TILE) : 0;
  // rows the buffers are laid out for: the fit's own, or what gpx_reserve asked for (appends then happen in place)
  const int64_t cap = h->reserve > 0 ? std::max(Npad, round_up(h->reserve, TILE)) : Npad;
  const int64_t capN = h->reserve > 0 ? cap : N;
  const int64_t ld = cap + ld_skew<T>();
  if (h->cfg.block == 0) {  // the library's choice; predict's block solves use the fit's block inverses: same width
    h->nb = auto_panel_width(h, Npad);
    if (h->env.nb_pred < 0) h->nb_pred = h->nb;
  }
  const int64_t ldp = h->nb + ld_skew<T>();
  h->N = N; h->Npad = Npad; h->ld = ld; h->ldp = ldp; h->d = d; h->k = k; h->n_ls = n_ls;
  h->sf2 = sf2; h->sn2 = sn2; h->jitter = jitter;
  const bool profile = (h->cfg.flags & GPX_FLAG_PROFILE) != 0;
  gpx_timings& tm = h->tm;
  tm.h2d = tm.kbuild = tm.chol = tm.solve = tm.logdet = tm.fit_total = 0;
  tm.chol_diag = tm.chol_trsm = tm.chol_strip = tm.chol_syrk = tm.syrk_flops = tm.comm = 0;
  tm.syrk_launches = 0;
  tm.kbuild_bytes = (double)sizeof(T) * ((double)N * (double)(N + 1) / 2.0 + (double)N * d);

  int rc;
  if ((rc = flag_handover_probe(h))) return rc;  // once per handle: device flags or hipEvents between the streams
  if ((rc = ensure(h, h->X, (size_t)capN * d * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Y, (size_t)capN * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Xs, (size_t)cap * d * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->ls, MAX_D * 8))) return rc;
  const int64_t NX = RHS_ROWS + Mpad;  // bordered rows: [K* rows of a fused predict] + the right-hand sides
  if (Xq && (rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->K, (size_t)(cap + NX) * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Winv, (size_t)(cap / KB) * KB * KB * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->P, (size_t)2 * (cap + NX) * ldp * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scalars, 64))) return rc;
  if ((rc = ensure(h, h->info, 64))) return rc;
  const int64_t nblk = (cap + h->nb - 1) / h->nb;
  const int64_t ldu = h->nb + ld_skew<T>();
  if ((rc = ensure(h, h->Wblk, (size_t)nblk * h->nb * h->nb * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Ublk, (size_t)h->nb * ldu * sizeof(T)))) return rc;
  if ((rc = stage_fit_weights<T>(h, N, cap))) return rc;
  if ((rc = stage_fit_kinds<T>(h, N, cap, sn2, jitter))) return rc;
  if ((rc = stage_fit_groups<T>(h, N, cap, d, lengthscale, n_ls, sn2, jitter))) return rc;
  const int bp = basis_count(h->basis_set, d);  // (k + bp <= 64 and N >= bp: check_fit_basis)
  h->basis = h->basis_set;
  h->bp = bp;
  if (bp && (rc = ensure(h, h->Bst, (size_t)BASIS_STATE * 8))) return rc;
  if (bp && (rc = ensure(h, h->scr.BG, (size_t)basis_gram_slices(Npad) * RHS_ROWS * RHS_ROWS * 8))) return rc;
  InvWork<T> iw;
  iw.W = (T*)h->Wblk.p;
  iw.U = (T*)h->Ublk.p;
  iw.ldu = ldu;
  iw.nbw = h->nb;
  iw.aux = h->st3;
  h->nbw = 0;  // valid again once this fit has finished

  T* dK = (T*)h->K.p;
  h->Lfac = dK;
  h->repl = false;
  T* dYT = dK + Npad * ld;  // rows [Npad, Npad + RHS_ROWS) of the K buffer: y^T, then z^T = (L^-1 y)^T
  h->zT = dYT;
  h->alphaT = nullptr;
  h->alpha_ready = false;
  int* dInfo = (int*)h->info.p;
  {
    PhaseScope total(h, &tm.fit_total);
    {
      PhaseScope ps(h, &tm.h2d);
      if ((rc = copy_in(h, h->X.p, X, (size_t)N * d * sizeof(T), mem_kind))) return rc;
      if ((rc = copy_in(h, h->Y.p, y, (size_t)N * k * sizeof(T), mem_kind))) return rc;
      if ((rc = copy_in(h, h->ls.p, lengthscale, (size_t)n_ls * 8, GPX_MEM_HOST))) return rc;
      const int init = INT_MAX;
      HIPCHK(h, hipMemcpyAsync(dInfo, &init, sizeof(int), hipMemcpyHostToDevice, h->st));
    }
    {
      PhaseScope ps(h, &tm.kbuild);
      launch_scale_points<T>((const T*)h->X.p, N, Npad, d, (const double*)h->ls.p, n_ls,
                          (T*)h->Xs.p, h->st);
      if (h->grouped)  // (never with kinds set: check_fit_groups)
        launch_kbuild_sym_g<T>(h->cfg.kernel, (const T*)h->Xs.p, N, Npad, d, sf2, (const int32_t*)h->Gfit.p,
                               (const double*)h->Gq.p, h->sg2, (const T*)h->Gdiag.p, dK, ld, h->st);
      else if (h->kinded)
        launch_kbuild_sym_k<T>(h->cfg.kernel, (const T*)h->Xs.p, N, Npad, d, sf2, (const int32_t*)h->Kfit.p,
                               (const double*)h->ls.p, n_ls, (const T*)h->Dfit.p, dK, ld, h->st);
      else if (h->weighted)
        launch_kbuild_sym_w<T>(h->cfg.kernel, (const T*)h->Xs.p, N, Npad, d, sf2, (const T*)h->Wfit.p, sn2, jitter, dK, ld,
                               h->st);
      else
        launch_kbuild_sym<T>(h->cfg.kernel, (const T*)h->Xs.p, N, Npad, d, sf2, sn2 + jitter, dK, ld, h->st);
      if (Xq) {  // rows [Npad + RHS_ROWS, ... + Mpad): K(Xq, X)
        if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
        kbuild_cross_fit<T>(h, (const T*)h->scr.Qs.p, M, Mpad, dK + (Npad + RHS_ROWS) * ld, ld);
      }
    }
    {
      PhaseScope ps(h, &tm.chol);
      launch_pack_rhs<T>((const T*)h->Y.p, N, k, dYT, ld, Npad, RHS_ROWS, h->st);
      if (bp) launch_basis_rows<T>((const T*)h->X.p, N, Npad, d, k, bp, dYT, ld, h->st);  // rows [k, k + bp): H^T -> Z_H^T
      // gpx_fit proper on two levels from GPX_TWO_LEVEL_FROM rows on (chol_two_level_enqueue); gpx_fit_predict's query
      // rows and the mixed mode's fp32 fit keep the one-level schedule
      if (!Xq && h->cfg.dtype != GPX_MIXED)
        rc = chol_two_level_enqueue<T>(h, dK, ld, Npad, h->nb, (T*)h->Winv.p, (T*)h->P.p, (T*)h->P.p + (Npad + NX) * ldp, ldp,
                                       dInfo, 0, profile, NX, &iw, Mpad);
      else
        rc = chol_enqueue<T>(h, dK, ld, Npad, h->nb, (T*)h->Winv.p, (T*)h->P.p, (T*)h->P.p + (Npad + NX) * ldp, ldp, dInfo, 0,
                             profile, NX, &iw, Mpad);
      if (rc) return rc;
    }
    if (bp) {  // beta = (Z_H^T Z_H)^-1 Z_H^T z, then z' = z - Z_H beta in place: every reader of zT from here on sees z'
      PhaseScope ps(h, &tm.solve);
      launch_bordered_gram<T>(dYT, ld, Npad, (double*)h->scr.BG.p, h->st);
      launch_beta_solve((const double*)h->scr.BG.p, Npad, k, bp, N, (double*)h->Bst.p, dInfo, h->st);
      launch_basis_project<T>(dYT, ld, Npad, k, bp, (const double*)h->Bst.p, h->st);
    }
    // The forward substitution happened inside the factorisation (bordered rows).  The
    // back substitution alpha = L^-T z is NOT on the fit+predict path: the posterior mean is
    // K* K^-1 y = V^T z with V = L^-1 K*^T, which the variance path computes anyway;
    // alpha is produced on demand (gpx_get_alpha, mean-only predict): ensure_alpha().
    {
      PhaseScope ps(h, &tm.logdet);
      launch_logdet<T>(dK, ld, Npad, (double*)h->scalars.p, h->st);
    }
  }
  int hinfo = 0;
  HIPCHK(h, hipMemcpyAsync(&hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(&h->logdet, h->scalars.p, sizeof(double), hipMemcpyDeviceToHost, h->st));
  if ((rc = finish_call(h))) return rc;
  if (hinfo < 0) {
    // wait_counter_kernel gave up although the self-test passed (a tool attached later, or one that reorders rather than
    // serialises): this handle hands over by hipEvents from now on and the fit runs once more — same kernels, same bits.
    // Only a forced GPX_CHAIN_FLAG=1, or a second failure, is an error.
    if (retry_with_events(h, retried))
      return fit_impl<T>(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info, Xq, M, true);
    return fail(h, GPX_E_HIP,
                "a stream parked on a device flag timed out: kernels are being serialised across streams — "
                "set GPX_CHAIN_FLAG=0 (and leave GPX_FUSED_STRIP unset) to hand over by hipEvents instead");
  }
  tm.handover_flags = chain_flag_enabled(h) ? 1.0 : 0.0;
  tm.handover_retries = (double)h->flag_retries;
  *info = (hinfo == INT_MAX) ? 0 : (int64_t)hinfo;
  h->fitted = (*info == 0);
  if (h->fitted) h->nbw = h->nb;
  return GPX_OK;
}

// ---- gpx_append: more observations without a new factorisation of the old ones -------------------------
// Rows [0, R0) of L, R0 = the last panel boundary inside the old data, do not change when rows are added below them, and
// neither do columns [0, R0) of z^T.  An append is the right-looking factorisation restarted at R0: the left part of the
// new rows (one forward solve against the R0 columns), the trailing square [R0, Npad')^2 rebuilt and reduced by the Schur
// term of those columns in one product, then chol_enqueue on it with the right-hand sides as bordered rows.

// Room for `Nnew` points.  Within the layout's capacity nothing of the factor moves; beyond it the factor's lower triangle
// and columns [0, R0) of z^T move into a buffer with room for one more panel width of points (or what gpx_reserve asked
// for), and the point, block-inverse and panel buffers grow with it.  Every allocation happens before anything is touched:
// on GPX_E_NOMEM the fit is as it was.
// with_weights: the fit has noise weights, or the new points bring some — the weight vector follows the same capacity.
// So do the kinds or path ids of a fit that has them and its finished diagonal terms: the N entries of the fit are kept,
// and the kinds / ids are -1 from there to the new capacity (the builders read them up to the padded size).
template <typename T>
int append_room(gpx_handle* h, int64_t Nnew, bool with_weights) {
  const int64_t skew = ld_skew<T>(), cap0 = h->ld - skew, NpadNew = round_up(Nnew, TILE), want = round_up(h->reserve, TILE);
  const int64_t N = h->N, Npad = h->Npad, nb = h->nb, d = h->d, k = h->k;
  const bool relayout = NpadNew > cap0 || want > cap0;
  const int64_t cap = !relayout ? cap0 : NpadNew <= want ? want : round_up(Nnew + nb, TILE);
  const int64_t ld = cap + skew, R0 = N / nb * nb;
  struct Grow {
    DevBuf* buf;
    size_t need, keep;
    DevBuf fresh;
    bool minus_one = false;  // kinds / ids: the fresh buffer holds -1 before the kept entries are copied in
  } g[] = {{&h->X, (size_t)cap * d * sizeof(T), (size_t)N * d * sizeof(T), {}},
           {&h->Y, (size_t)cap * k * sizeof(T), (size_t)N * k * sizeof(T), {}},
           {&h->Xs, (size_t)cap * d * sizeof(T), (size_t)Npad * d * sizeof(T), {}},
           {&h->Winv, (size_t)(cap / KB) * KB * KB * sizeof(T), (size_t)(Npad / KB) * KB * KB * sizeof(T), {}},
           {&h->Wblk, (size_t)((cap + nb - 1) / nb) * nb * nb * sizeof(T), (size_t)(R0 / nb) * nb * nb * sizeof(T), {}},
           {&h->Wfit, with_weights ? (size_t)cap * sizeof(T) : 0, h->weighted ? (size_t)N * sizeof(T) : 0, {}},
           {&h->Kfit, h->kinded ? (size_t)cap * sizeof(int32_t) : 0, (size_t)N * sizeof(int32_t), {}, true},
           {&h->Dfit, h->kinded ? (size_t)cap * sizeof(T) : 0, (size_t)N * sizeof(T), {}},
           {&h->Gfit, h->grouped ? (size_t)cap * sizeof(int32_t) : 0, (size_t)N * sizeof(int32_t), {}, true},
           {&h->Gdiag, h->grouped ? (size_t)cap * sizeof(T) : 0, (size_t)N * sizeof(T), {}}};
  const size_t kbytes = (size_t)(cap + RHS_ROWS) * ld * sizeof(T);
  const size_t pbytes = (size_t)2 * (cap + RHS_ROWS) * h->ldp * sizeof(T);
  const bool newK = relayout || h->K.cap < kbytes, newP = h->P.cap < pbytes;
  double need = (newK ? (double)kbytes : 0.0) + (newP ? (double)pbytes : 0.0);
  for (Grow& x : g)
    if (x.buf->cap < x.need) need += (double)x.need;
  if (need == 0.0) return GPX_OK;
  size_t freeb = 0, totalb = 0;
  HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
  const double avail = (double)freeb + (newP ? (double)h->P.cap : 0.0);  // the panel buffers are scratch: freed first
  char msg[256];
  snprintf(msg, sizeof msg, "gpx_append: %.0f bytes of device memory needed for %lld points (beside the fit), %.0f available",
           need, (long long)Nnew, avail);
  if (need > avail) return fail(h, GPX_E_NOMEM, msg);
  DevBuf Knew;
  if (newP) h->P = DevBuf();
  bool ok = !newK || hipMalloc(&Knew.p, kbytes) == hipSuccess;
  if (ok && newK) Knew.cap = kbytes;
  for (Grow& x : g)
    if (ok && x.buf->cap < x.need) {
      ok = hipMalloc(&x.fresh.p, x.need) == hipSuccess;
      if (ok) x.fresh.cap = x.need;
    }
  if (ok && newP) {
    ok = hipMalloc(&h->P.p, pbytes) == hipSuccess;
    if (ok) h->P.cap = pbytes;
  }
  if (!ok) {
    (void)hipGetLastError();
    return fail(h, GPX_E_NOMEM, msg);  // (the fresh buffers free themselves; the fit is untouched)
  }
  for (Grow& x : g) {
    if (x.fresh.p && x.minus_one) HIPCHK(h, hipMemsetAsync(x.fresh.p, 0xFF, x.need, h->st));
    if (x.fresh.p && x.keep) HIPCHK(h, hipMemcpyAsync(x.fresh.p, x.buf->p, x.keep, hipMemcpyDeviceToDevice, h->st));
  }
  T* zT = (T*)h->zT;
  if (newK) {  // the factor's lower triangle; z^T keeps its row (append_restart moves it when Npad changes)
    T* dst = (T*)Knew.p;
    launch_copy_lower<T>(dst, ld, (const T*)h->K.p, h->ld, Npad, h->st);
    zT = dst + Npad * ld;
    HIPCHK(h, hipMemsetAsync(zT, 0, (size_t)RHS_ROWS * ld * sizeof(T), h->st));
    launch_copy2d<T>(zT, ld, (const T*)h->zT, h->ld, RHS_ROWS, R0, h->st);
  }
  HIPCHK(h, hipStreamSynchronize(h->st));
  for (Grow& x : g)
    if (x.fresh.p) *x.buf = std::move(x.fresh);  // the old allocation leaves with x.fresh
  if (newK) {
    h->K = std::move(Knew);
    h->ld = ld;
    h->Lfac = h->K.p;
    h->zT = zT;
  }
  return GPX_OK;
}

// The restart itself, from what is resident: points [0, Nnew) in h->X / h->Y (Xnew != null: the last m of them are copied
// in first), the factor of the first Nold.  Nnew == Nold rebuilds the fit of Nold points from its first R0 columns — what
// a failed append runs to hand the previous model back.  *hinfo: the device's pivot word (INT_MAX: positive definite).
template <typename T>
int append_restart(gpx_handle* h, int64_t Nold, int64_t Nnew, const void* Xnew, const void* ynew, int32_t mem_kind,
                   int* hinfo) {
  const int64_t ld = h->ld, ldp = h->ldp, nb = h->nb;
  const int d = h->d, k = h->k;
  const int64_t R0 = Nold / nb * nb, R1 = Nold / TILE * TILE;  // first column / first row that is computed again
  const int64_t Npad = round_up(Nnew, TILE), np = Npad - R0, rows = Npad - R1, m = Nnew - Nold;
  const bool profile = (h->cfg.flags & GPX_FLAG_PROFILE) != 0;
  gpx_timings& tm = h->tm;
  T* dK = (T*)h->K.p;
  T* Xs = (T*)h->Xs.p;
  T* Winv = (T*)h->Winv.p;
  T* dYT = dK + Npad * ld;
  int* dInfo = (int*)h->info.p;
  int rc;
  SolveWork<T> sw;
  if (R0 > 0 && (rc = dense_solve_work<T>(h, h->scr.Tsol, rows, &sw))) return rc;
  InvWork<T> iw;
  iw.W = (T*)h->Wblk.p + (R0 / nb) * nb * nb;
  iw.U = (T*)h->Ublk.p;
  iw.ldu = nb + ld_skew<T>();
  iw.nbw = (int)nb;
  iw.aux = h->st3;
  {
    PhaseScope total(h, &tm.fit_total);
    {
      PhaseScope ps(h, &tm.h2d);
      if (m > 0 && Xnew) {
        if ((rc = copy_in(h, (T*)h->X.p + Nold * d, Xnew, (size_t)m * d * sizeof(T), mem_kind))) return rc;
        if ((rc = copy_in(h, (T*)h->Y.p + Nold * k, ynew, (size_t)m * k * sizeof(T), mem_kind))) return rc;
      }
      const int init = INT_MAX;
      HIPCHK(h, hipMemcpyAsync(dInfo, &init, sizeof(int), hipMemcpyHostToDevice, h->st));
    }
    {
      PhaseScope ps(h, &tm.kbuild);
      if (dYT != (T*)h->zT) {  // Npad changes: columns [0, R0) of z^T to their new rows before those rows are built
        HIPCHK(h, hipMemsetAsync(dYT, 0, (size_t)RHS_ROWS * ld * sizeof(T), h->st));
        launch_copy2d<T>(dYT, ld, (const T*)h->zT, ld, RHS_ROWS, R0, h->st);
        h->zT = dYT;
      }
      launch_scale_points<T>((const T*)h->X.p + R1 * d, Nnew - R1, rows, d, (const double*)h->ls.p, h->n_ls, Xs + R1 * d,
                             h->st);
      // A fit with kinds or path ids: the same two builds by the KINDS / GROUPS builders, with the side channel of the rows
      // ([R1, Nnew) of the left part, [R0, Nnew) of the square: both offsets are multiples of 128, and the entries from Nnew
      // to the capacity are -1) and the finished diagonal terms of rows [R0, Nnew) from the stored and the new weights.
      const T* wfit = h->weighted ? (const T*)h->Wfit.p + R0 : nullptr;
      if (h->grouped) {
        const int32_t* G = (const int32_t*)h->Gfit.p;
        launch_kinds_diag<T>(G + R0, wfit, Nnew - R0, h->sn2, h->sn2, h->jitter, (T*)h->Gdiag.p + R0, h->st);
        if (R0 > 0)  // (a tile of new rows whose ids meet none of its columns' skips the path term)
          launch_kbuild_cross_g<T>(h->cfg.kernel, Xs + R1 * d, G + R1, Nnew - R1, rows, Xs, G, R0, R0, d, h->sf2,
                                   (const double*)h->Gq.p, h->sg2, dK + R1 * ld, ld, h->st);
        launch_kbuild_sym_g<T>(h->cfg.kernel, Xs + R0 * d, Nnew - R0, np, d, h->sf2, G + R0, (const double*)h->Gq.p, h->sg2,
                               (const T*)h->Gdiag.p + R0, dK + R0 * ld + R0, ld, h->st);
      } else if (h->kinded) {
        const int32_t* Kd = (const int32_t*)h->Kfit.p;
        launch_kinds_diag<T>(Kd + R0, wfit, Nnew - R0, h->sn2, h->sn2_deriv, h->jitter, (T*)h->Dfit.p + R0, h->st);
        if (R0 > 0)
          launch_kbuild_cross_kk<T>(h->cfg.kernel, Xs + R1 * d, Kd + R1, Nnew - R1, rows, Xs, Kd, R0, R0, d, h->sf2,
                                    (const double*)h->ls.p, h->n_ls, dK + R1 * ld, ld, h->st);
        launch_kbuild_sym_k<T>(h->cfg.kernel, Xs + R0 * d, Nnew - R0, np, d, h->sf2, Kd + R0, (const double*)h->ls.p, h->n_ls,
                               (const T*)h->Dfit.p + R0, dK + R0 * ld + R0, ld, h->st);
      } else {
        if (R0 > 0)  // left part of the 128-row tiles that hold a new point: K(x_i, x_j), j < R0
          launch_kbuild_cross<T>(h->cfg.kernel, Xs + R1 * d, Nnew - R1, rows, Xs, R0, R0, d, h->sf2, dK + R1 * ld, ld, h->st);
        if (h->weighted)  // the rebuilt square needs the stored weights of rows [R0, Nold) beside the new points'
          launch_kbuild_sym_w<T>(h->cfg.kernel, Xs + R0 * d, Nnew - R0, np, d, h->sf2, (const T*)h->Wfit.p + R0, h->sn2,
                                 h->jitter, dK + R0 * ld + R0, ld, h->st);
        else
          launch_kbuild_sym<T>(h->cfg.kernel, Xs + R0 * d, Nnew - R0, np, d, h->sf2, h->sn2 + h->jitter, dK + R0 * ld + R0,
                               ld, h->st);
      }
    }
    {
      PhaseScope ps(h, &tm.chol);
      if (R0 > 0 && (rc = solve_fwd_enqueue<T>(h, dK + R1 * ld, rows, dK, ld, R0, h->nb_pred, Winv, &sw))) return rc;
      launch_pack_rhs<T>((const T*)h->Y.p + R0 * k, Nnew - R0, k, dYT + R0, ld, np, RHS_ROWS, h->st);
      if (R0 > 0) {  // Schur term of the R0 columns already factorised: the square, then the bordered rows
        launch_gemm_nt<T>(128, dK + R0 * ld + R0, ld, dK + R0 * ld, ld, dK + R0 * ld, ld, np, np, R0, 1, 0, h->st);
        launch_gemm_nt<T>(64, dYT + R0, ld, dYT, ld, dK + R0 * ld, ld, RHS_ROWS, np, R0, 0, 0, h->st);
      }
      if ((rc = chol_enqueue<T>(h, dK + R0 * ld + R0, ld, np, (int)nb, Winv + (R0 / KB) * (KB * KB), (T*)h->P.p,
                                (T*)h->P.p + (np + RHS_ROWS) * ldp, ldp, dInfo, R0, profile, RHS_ROWS, &iw, 0)))
        return rc;
    }
    {
      PhaseScope ps(h, &tm.logdet);
      launch_logdet<T>(dK, ld, Npad, (double*)h->scalars.p, h->st);
    }
  }
  HIPCHK(h, hipMemcpyAsync(hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(&h->logdet, h->scalars.p, sizeof(double), hipMemcpyDeviceToHost, h->st));
  return finish_call(h);
}

// side (gpx_append_rows on a fit with kinds or path ids; host, m entries, checked): the new rows' kinds (h->kinded) or path
// ids (h->grouped).  They are staged behind the fit's own on the device before the restart; the host copies and has_deriv
// follow once the restart has gone through, and a failed append takes the staged entries back (-1).
template <typename T>
int append_impl(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, int64_t m, int32_t mem_kind,
                int64_t* info, const int32_t* side = nullptr) {
  const int64_t Nold = h->N, Nnew = Nold + m;
  gpx_timings& tm = h->tm;
  tm.h2d = tm.kbuild = tm.chol = tm.solve = tm.logdet = tm.fit_total = 0;
  tm.chol_diag = tm.chol_trsm = tm.chol_strip = tm.chol_syrk = tm.syrk_flops = tm.comm = 0;
  tm.syrk_launches = 0;
  tm.kbuild_bytes = (double)sizeof(T) * ((double)m * (double)(Nold + Nnew + 1) / 2.0 + (double)m * h->d);
  int rc;
  if ((rc = flag_handover_probe(h))) return rc;
  const bool was_weighted = h->weighted;
  if ((rc = append_room<T>(h, Nnew, was_weighted || wnew))) return rc;  // nothing of the fit has been touched yet
  {  // ... nor by the block-solve buffers of the new rows' forward solve
    SolveWork<T> sw;
    if ((rc = dense_solve_work<T>(h, h->scr.Tsol, round_up(Nnew, TILE) - Nold / TILE * TILE, &sw))) return rc;
  }
  // The weight vector has the factor's capacity (append_room grew it with the layout, keeping the N weights of the fit).
  // A fit without weights that is given some gets ones for its own points first.
  if (was_weighted || wnew) {
    if (!was_weighted) launch_fill<T>((T*)h->Wfit.p, Nold, 1.0, h->st);
    if (wnew) {
      if ((rc = copy_in(h, (T*)h->Wfit.p + Nold, wnew, (size_t)m * sizeof(T), mem_kind))) return rc;
    } else {
      launch_fill<T>((T*)h->Wfit.p + Nold, m, 1.0, h->st);
    }
    h->weighted = true;
  }
  int32_t* dside = !side ? nullptr : (int32_t*)(h->grouped ? h->Gfit.p : h->Kfit.p);
  if (side) {  // (the caller's host copy is only read inside this block: an early return below leaves no copy in flight)
    HIPCHK(h, hipMemcpyAsync(dside + Nold, side, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
  }
  h->fitted = false;  // until the restart (or the restart back) has gone through
  h->alphaT = nullptr;
  h->alpha_ready = false;
  // the restart; a parked stream that timed out: once more with hipEvents, as fit_impl does (same kernels, same bits)
  auto restart = [&](int64_t n1, const void* Xa, const void* ya, int* hinfo) -> int {
    for (int attempt = 0;; ++attempt) {
      int r = append_restart<T>(h, Nold, n1, Xa, ya, mem_kind, hinfo);
      if (r != GPX_OK || *hinfo >= 0) return r;
      if (!retry_with_events(h, attempt > 0))
        return fail(h, GPX_E_HIP,
                    "a stream parked on a device flag timed out: kernels are being serialised across streams — "
                    "set GPX_CHAIN_FLAG=0 (and leave GPX_FUSED_STRIP unset) to hand over by hipEvents instead");
      if ((r = begin_call(h))) return r;
    }
  };
  int hinfo = 0;
  if ((rc = restart(Nnew, Xnew, ynew, &hinfo))) return rc;
  *info = (hinfo == INT_MAX) ? 0 : (int64_t)hinfo;
  int64_t Nfit = Nnew;
  if (*info > 0) {  // not positive definite with the new points: the same restart with none of them is the previous fit
    int back = 0;
    if ((rc = begin_call(h))) return rc;
    if (side) HIPCHK(h, hipMemsetAsync(dside + Nold, 0xFF, (size_t)m * sizeof(int32_t), h->st));  // -1 beyond the fit again
    if ((rc = restart(Nold, nullptr, nullptr, &back))) return rc;
    if (back != INT_MAX) return fail(h, GPX_E_HIP, "gpx_append: the previous fit could not be restored");
    Nfit = Nold;
    h->weighted = was_weighted;  // (the weights of the first Nold points were never touched)
  } else if (side) {  // (the restart has finished: nothing reads the host vectors asynchronously any more)
    std::vector<int32_t>& host = h->grouped ? h->groups_fit : h->kinds_fit;
    host.insert(host.end(), side, side + m);
    if (h->kinded)
      for (int64_t i = 0; i < m; ++i) h->has_deriv |= side[i] >= 0;
  }
  h->N = Nfit;
  h->Npad = round_up(Nfit, TILE);
  tm.handover_flags = chain_flag_enabled(h) ? 1.0 : 0.0;
  tm.handover_retries = (double)h->flag_retries;
  h->fitted = true;
  return GPX_OK;
}

// ---- gpx_remove_rows: fewer observations without a new factorisation of the others -------------------
// One pass takes rows [a, a + m) (m <= UPD_W) out of a factor of N rows (csrc/gpx_update.hip has the algebra).  Nothing is
// evaluated: the factor, z^T and the carry are all the pass reads.  The bordered rows stay at `zT` (their place for the
// N0 points the call started with) through every pass; remove_impl moves them once at the end.
//
// Who may write where (the overwrite hazard).  Panel j of a pass reads columns [b + j w, b + (j + 1) w) of L33 and of z^T
// (b = a + m, w = UPD_W) and its new columns belong m to the left: [a + j w, a + (j + 1) w), rows m up.
//   - Later launches read columns >= b + (j + 1) w only: to the right of everything panel j writes, for every m >= 0.
//   - Inside panel j's own launch the written columns meet the read ones iff m < w, and then a band's destination rows
//     are the unread source of the band above it.  So for m < w the strip writes into the panel buffer (h->P) and a
//     second launch moves the panel into place: by then panel j has been consumed.  For m == w the two column ranges are
//     disjoint — the strip writes columns [p0 - w, p0), which hold panel j - 1's source (consumed by the launch before) or
//     the removed columns themselves — and the strip writes the factor directly.
//   - The carry is a buffer of its own; a workgroup overwrites only the carry rows it has read itself.
//   - L31 (columns [0, a), no arithmetic) moves m rows up through the panel buffer, a slab of rows at a time: copy out,
//     then copy in — two launches in stream order, so a slab's destination may overlap any source row.
// Two full passes (m == UPD_W) in a row run as a two-stage pipeline: the second pass, on st2, is one panel behind the
// first.  Its panel j reads columns [a1 + j w, a1 + (j + 1) w) — exactly what panel j of the first pass has written
// (lead->done[j] is recorded behind that strip) — and writes the w columns left of them; panels j' > j of the first pass
// read and write columns from a1 + (j + 1) w on.  The second pass starts (carry, L31) once the first has moved its L31
// (lead->moved), which holds the second's removed columns and its own L31; each pass has a carry and a Q of its own
// (`slot`), and only the L31 moves touch the panel buffer (full passes write the factor directly).
struct PassLink {
  hipEvent_t moved = nullptr;
  std::vector<hipEvent_t> done;
};

template <typename T>
int remove_pass(gpx_handle* h, int64_t a, int64_t m, int64_t N, T* zT, int* dInfo, hipStream_t st, int slot,
                PassLink* record, const PassLink* follow) {
  const int64_t ld = h->ld, b = a + m, n3 = N - b;
  if (n3 <= 0) return GPX_OK;  // the tail: a truncation
  T* dK = (T*)h->K.p;
  T* W = (T*)h->scr.UW.p + (size_t)slot * (h->scr.UW.cap / sizeof(T) / 2);
  T* Q = (T*)h->scr.UQ.p + (size_t)slot * 4 * UPD_W * UPD_W;
  T* P = (T*)h->P.p;
  const int64_t pcap = (int64_t)(h->P.cap / sizeof(T));
  if (follow) HIPCHK(h, hipStreamWaitEvent(st, follow->moved, 0));
  launch_upd_carry_init<T>(dK, ld, a, (int)m, n3, zT, W, st);
  if (a > 0) {
    const int64_t R = std::max<int64_t>(1, pcap / a);
    for (int64_t r0 = 0; r0 < n3; r0 += R) {
      const int64_t rows = std::min(R, n3 - r0);
      launch_upd_copy<T>(P, a, dK + (b + r0) * ld, ld, rows, a, st);
      launch_upd_copy<T>(dK + (a + r0) * ld, ld, P, a, rows, a, st);
    }
  }
  int rc;
  if (record && (rc = record_event(h, st, "gpx_remove_rows", &record->moved))) return rc;
  const bool direct = m == UPD_W;
  for (int64_t j0 = 0; j0 < n3; j0 += UPD_W) {
    const int64_t p0 = b + j0, nrows = n3 - j0;
    const int nv = (int)std::min<int64_t>(UPD_W, nrows);
    T* Wp = W + j0 * UPD_W;
    T* Wz = W + n3 * UPD_W;
    T* dstL = dK + (p0 - m) * ld + (p0 - m);
    T* dstZ = zT + (p0 - m);
    if (follow) HIPCHK(h, hipStreamWaitEvent(st, follow->done[(size_t)(j0 / UPD_W)], 0));
    launch_upd_small<T>(dK, ld, p0, nv, Wp, Q, a + j0, dInfo, st);
    if (direct) {
      launch_upd_strip<T>(dK, ld, p0, nrows, nv, zT, Wp, Wz, Q, dstL, ld, dstZ, ld, st);
    } else {
      launch_upd_strip<T>(dK, ld, p0, nrows, nv, zT, Wp, Wz, Q, P, UPD_W, P + nrows * UPD_W, UPD_W, st);
      launch_upd_unstage<T>(P, nrows, nv, dstL, ld, dstZ, ld, st);
    }
    if (record) {
      hipEvent_t e;
      if ((rc = record_event(h, st, "gpx_remove_rows", &e))) return rc;
      record->done.push_back(e);
    }
  }
  return GPX_OK;
}

// `bytes` bytes from byte offset `from` of buf to offset `to` < from (the ranges may overlap: through the panel buffer)
int shift_down(gpx_handle* h, void* buf, size_t to, size_t from, size_t bytes) {
  if (!bytes) return GPX_OK;
  HIPCHK(h, hipMemcpyAsync(h->P.p, (const char*)buf + from, bytes, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync((char*)buf + to, h->P.p, bytes, hipMemcpyDeviceToDevice, h->st));
  return GPX_OK;
}

template <typename T>
int remove_impl(gpx_handle* h, int64_t start, int64_t count, int64_t* info) {
  const int64_t N0 = h->N, Npad0 = h->Npad, ld = h->ld, N1 = N0 - count, Npad1 = round_up(N1, TILE);
  const int64_t stop = start + count, tail = N0 - stop;
  const int d = h->d, k = h->k;
  gpx_timings& tm = h->tm;
  tm.h2d = tm.kbuild = tm.chol = tm.solve = tm.logdet = tm.fit_total = 0;
  tm.chol_diag = tm.chol_trsm = tm.chol_strip = tm.chol_syrk = tm.syrk_flops = tm.comm = 0;
  tm.syrk_launches = 0;
  tm.kbuild_bytes = 0;
  int rc;
  if ((rc = ensure(h, h->scr.UW, (size_t)2 * (N0 + 64) * UPD_W * sizeof(T)))) return rc;  // (the fit is untouched so far)
  if ((rc = ensure(h, h->scr.UQ, (size_t)2 * 4 * UPD_W * UPD_W * sizeof(T)))) return rc;  // (two passes in flight)
  T* dK = (T*)h->K.p;
  T* zT = (T*)h->zT;
  int* dInfo = (int*)h->info.p;
  h->fitted = false;  // until the update has gone through: it cannot be taken back in place
  h->alphaT = nullptr;
  h->alpha_ready = false;
  h->nbw = 0;  // the explicit inverses of the panel-wide diagonal blocks belong to the old rows' grid
  {
    PhaseScope total(h, &tm.fit_total);
    {
      PhaseScope ps(h, &tm.chol);
      const int init = INT_MAX;
      HIPCHK(h, hipMemcpyAsync(dInfo, &init, sizeof(int), hipMemcpyHostToDevice, h->st));
      int64_t N = N0;
      for (int64_t hi = stop; hi > start;) {  // from the highest rows down, one update width at a time
        const int64_t lo = std::max(start, hi - UPD_W);
        if (hi - start >= 2 * UPD_W && N > hi && h->st2) {  // two full passes with rows below them: the pipeline
          PassLink link;
          if ((rc = remove_pass<T>(h, lo, UPD_W, N, zT, dInfo, h->st, 0, &link, nullptr))) return rc;
          if ((rc = remove_pass<T>(h, lo - UPD_W, UPD_W, N - UPD_W, zT, dInfo, h->st2, 1, nullptr, &link))) return rc;
          if ((rc = stream_waits(h, h->st, h->st2, "gpx_remove_rows"))) return rc;
          N -= 2 * UPD_W;
          hi = lo - UPD_W;
          continue;
        }
        if ((rc = remove_pass<T>(h, lo, hi - lo, N, zT, dInfo, h->st, 0, nullptr, nullptr))) return rc;
        N -= hi - lo;
        hi = lo;
      }
      // what a fit of N1 points leaves beyond them, the bordered rows at their place below Npad1 rows
      launch_upd_pad<T>(dK, ld, N1, Npad1, zT, Npad0, h->st);
      if (Npad1 != Npad0) {
        T* z1 = dK + Npad1 * ld;
        HIPCHK(h, hipMemsetAsync(z1, 0, (size_t)RHS_ROWS * ld * sizeof(T), h->st));
        launch_upd_copy<T>(z1, ld, zT, ld, RHS_ROWS, N1, h->st);
        h->zT = z1;
      }
      launch_upd_trinv<T>(dK, ld, start / KB, Npad1 / KB, (T*)h->Winv.p, h->st);
      // the stored rows follow: points, scaled points (zero beyond N1), targets, weights, kinds / ids (-1 beyond N1)
      // and their finished diagonal terms
      if ((rc = shift_down(h, h->X.p, (size_t)start * d * sizeof(T), (size_t)stop * d * sizeof(T), (size_t)tail * d * sizeof(T)))) return rc;
      if ((rc = shift_down(h, h->Y.p, (size_t)start * k * sizeof(T), (size_t)stop * k * sizeof(T), (size_t)tail * k * sizeof(T)))) return rc;
      if ((rc = shift_down(h, h->Xs.p, (size_t)start * d * sizeof(T), (size_t)stop * d * sizeof(T), (size_t)tail * d * sizeof(T)))) return rc;
      HIPCHK(h, hipMemsetAsync((T*)h->Xs.p + N1 * d, 0, (size_t)(Npad0 - N1) * d * sizeof(T), h->st));
      if (h->weighted &&
          (rc = shift_down(h, h->Wfit.p, (size_t)start * sizeof(T), (size_t)stop * sizeof(T), (size_t)tail * sizeof(T))))
        return rc;
      for (int side = 0; side < 2; ++side) {
        if (!(side ? h->grouped : h->kinded)) continue;
        DevBuf& ids = side ? h->Gfit : h->Kfit;
        DevBuf& dg = side ? h->Gdiag : h->Dfit;
        if ((rc = shift_down(h, ids.p, (size_t)start * 4, (size_t)stop * 4, (size_t)tail * 4))) return rc;
        HIPCHK(h, hipMemsetAsync((int32_t*)ids.p + N1, 0xFF, (size_t)count * 4, h->st));
        if ((rc = shift_down(h, dg.p, (size_t)start * sizeof(T), (size_t)stop * sizeof(T), (size_t)tail * sizeof(T)))) return rc;
      }
    }
    {
      PhaseScope ps(h, &tm.logdet);
      launch_logdet<T>(dK, ld, Npad1, (double*)h->scalars.p, h->st);
    }
  }
  int hinfo = 0;
  HIPCHK(h, hipMemcpyAsync(&hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(&h->logdet, h->scalars.p, sizeof(double), hipMemcpyDeviceToHost, h->st));
  if ((rc = finish_call(h))) return rc;
  if (h->kinded && (int64_t)h->kinds_fit.size() == N0) {
    h->kinds_fit.erase(h->kinds_fit.begin() + start, h->kinds_fit.begin() + stop);
    h->has_deriv = false;
    for (int32_t v : h->kinds_fit) h->has_deriv |= v >= 0;
  }
  if (h->grouped && (int64_t)h->groups_fit.size() == N0) h->groups_fit.erase(h->groups_fit.begin() + start, h->groups_fit.begin() + stop);
  h->N = N1;
  h->Npad = Npad1;
  *info = (hinfo == INT_MAX) ? 0 : (int64_t)hinfo;
  h->fitted = (*info == 0);
  return GPX_OK;
}

// RT (k <= 8 rows of ld) <- (L L^T)^-1 RT (or only L^-T RT) with the fit's explicit block inverses: a forward and a
// backward block substitution as streams over the factor (gpx_mixed.hip: rowdot / coldot kernels), one stream, in order.
template <typename T>
int solve_few(gpx_handle* h, T* RT, int k, const T* L, int64_t ld, int64_t n, const T* W, int nbw, bool forward, bool backward) {
  // W: [n / nbw][nbw][nbw] explicit inverses of the nbw-wide diagonal blocks.  The sweeps run in blocks of nb = min(nbw,
  // 1024): the diagonal nb-sub-blocks of a lower-triangular inverse ARE the inverses of the diagonal nb-sub-blocks of
  // the factor, so a 2048-wide W serves 1024-blocks through a pointer and its leading dimension (round 4).
  const int nb = std::min(nbw, 1024);
  auto Wsub = [&](int64_t o) -> const T* {
    return W + (o / nbw) * (int64_t)nbw * nbw + ((o % nbw) / nb) * ((int64_t)nb * nbw + nb);
  };
  int rc;
  if ((rc = ensure(h, h->Zfew, (size_t)8 * nb * sizeof(T)))) return rc;
  T* Zs = (T*)h->Zfew.p;
  hipStream_t st = h->st;
  for (int64_t o = 0; forward && o < n; o += nb) {  // L z = r
    const int nbp = (int)std::min<int64_t>(nb, n - o);
    const int64_t t0 = o + nbp;
    launch_few_product<T>(false, true, Zs, nb, Wsub(o), nbw, nbp, nbp, RT + o, ld, k, st);
    HIPCHK(h, hipMemcpy2DAsync(RT + o, (size_t)ld * sizeof(T), Zs, (size_t)nb * sizeof(T), (size_t)nbp * sizeof(T), k,
                               hipMemcpyDeviceToDevice, st));
    launch_few_product<T>(false, false, RT + t0, ld, L + t0 * ld + o, ld, n - t0, nbp, Zs, nb, k, st);
  }
  for (int64_t o = ((n - 1) / nb) * nb; backward && o >= 0; o -= nb) {  // L^T x = z
    const int nbp = (int)std::min<int64_t>(nb, n - o);
    launch_few_product<T>(true, true, Zs, nb, Wsub(o), nbw, nbp, nbp, RT + o, ld, k, st);
    HIPCHK(h, hipMemcpy2DAsync(RT + o, (size_t)ld * sizeof(T), Zs, (size_t)nb * sizeof(T), (size_t)nbp * sizeof(T), k,
                               hipMemcpyDeviceToDevice, st));
    launch_few_product<T>(true, false, RT, ld, L + o * ld, ld, o, nbp, Zs, nb, k, st);
  }
  return GPX_OK;
}

// the streaming solver needs the fit's explicit block inverses (h->Wblk, blocks of width h->nbw up to 1024 or a multiple
// of 1024, which solve_few serves in 1024-sub-blocks; other widths above 1024 take the slab path: every block of an
// unsharded fit, or of a shard that keeps the whole factor), at most 8 right-hand sides (GPX_FEW_SOLVE=0: always the
// slab path)
bool few_solver_applies(const gpx_handle* h) {
  return h->env.few_solve && h->nbw > 0 && (h->nbw <= 1024 ? h->nbw % 128 == 0 : h->nbw % 1024 == 0) && h->k <= 8 &&
         (!h->comm || h->repl) && h->Wblk.p;
}

// alpha^T = z^T L^-1 on a copy of the bordered rows (z stays available for V^T z)
template <typename T>
int ensure_alpha(gpx_handle* h) {
  if (h->alpha_ready) return GPX_OK;
  int rc;
  if ((rc = ensure(h, h->AT, (size_t)RHS_ROWS * h->ld * sizeof(T)))) return rc;
  PhaseScope ps(h, &h->tm.solve);
  HIPCHK(h, hipMemcpyAsync(h->AT.p, h->zT, (size_t)RHS_ROWS * h->ld * sizeof(T), hipMemcpyDeviceToDevice,
                           h->st));
  if (few_solver_applies(h)) {  // k <= 8 targets: the back substitution as a stream over the factor (round 3)
    if ((rc = solve_few<T>(h, (T*)h->AT.p, h->k, (const T*)h->Lfac, h->ld, h->Npad, (const T*)h->Wblk.p, h->nbw, false)))
      return rc;
  } else
    solve_bwd_enqueue<T>(h, (T*)h->AT.p, RHS_ROWS, (const T*)h->Lfac, h->ld, h->Npad, h->nb_solve,
                         (const T*)h->Winv.p);
  h->alphaT = h->AT.p;
  h->alpha_ready = true;
  return GPX_OK;
}

// K*, variance solve, mean and variance of M query points; results stay on the device in
// h->meanout (M x k) and h->var (M).  Reads the factor through h->Lfac (whole L).
// gq != null (gpx_predict_paths; a fit with path ids): the query points' path ids, staged in scr.Qg; a batch reads its own.
template <typename T>
int predict_core(gpx_handle* h, const void* Xq, int64_t M, bool want_var, int32_t mem_kind, const int32_t* gq) {
  if (M <= 0) return GPX_OK;  // a rank whose slice of the query points is empty
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld;
  const int d = h->d, k = h->k;
  const int64_t Mpad = round_up(M, TILE);
  const int64_t ldm = Mpad + ld_skew<T>();
  const int64_t MB = pred_batch_rows(h, Mpad, (size_t)ld * sizeof(T), true);
  gpx_timings& tm = h->tm;
  int rc;
  if ((rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.VT, (size_t)MB * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * sizeof(T)))) return rc;
  const int64_t ldpm = std::min(MB, Mpad) + ld_skew<T>();  // split-K partial tiles of ONE batch
  if ((rc = ensure_mean_partials<T>(h, h->scr.MTpart, ldpm))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->var, (size_t)Mpad * sizeof(T)))) return rc;
  SolveWork<T> sw;  // block inverses of this fit (a shard: of the factor it keeps whole)
  if (want_var && (rc = dense_solve_work<T>(h, h->scr.Tsol, MB, &sw))) return rc;
  T* dVT = (T*)h->scr.VT.p;
  const T* dK = (const T*)h->Lfac;
  const T* dWinv = (const T*)h->Winv.p;
  if (!want_var && (rc = ensure_alpha<T>(h))) return rc;  // mean only: K* alpha with the cached alpha
  const T* rhsT = (const T*)(want_var ? h->zT : h->alphaT);
  {
    PhaseScope ps(h, &tm.kstar);
    if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
    if (gq && (rc = upload_query_ids(h, gq, M, mem_kind))) return rc;
  }
  const int32_t* dg = gq ? (const int32_t*)h->scr.Qg.p : nullptr;
  for (int64_t m0 = 0; m0 < Mpad; m0 += MB) {  // batches of query points through one V^T buffer
    const int64_t mp = std::min(MB, Mpad - m0);       // padded rows of this batch
    const int64_t mv = std::min<int64_t>(mp, M - m0);  // valid rows
    {
      PhaseScope ps(h, &tm.kstar);
      kbuild_cross_fit<T>(h, (const T*)h->scr.Qs.p + m0 * d, mv, mp, dVT, ld, dg ? dg + m0 : nullptr);
    }
    if (want_var) {
      PhaseScope ps(h, &tm.trsm);
      if ((rc = solve_fwd_enqueue<T>(h, dVT, mp, dK, ld, Npad, h->nb_pred, dWinv, &sw))) return rc;
    }
    {  // with the variance: mean^T (64 x mp) = z^T (64 x Npad) * V   (mu = K* K^-1 y = V^T z);
       // mean only: alpha^T * K*^T
      PhaseScope ps(h, &tm.mean);
      mean_product<T>(h, (T*)h->scr.MT.p + m0, ldm, rhsT, dVT, mp, (T*)h->scr.MTpart.p, ldpm);
    }
    if (want_var) {
      PhaseScope ps(h, &tm.var);
      launch_var_rows<T>(dVT, ld, mv, Npad, h->sf2, (T*)h->var.p + m0, h->st, dg ? dg + m0 : nullptr, h->sg2);
    }
  }
  {
    PhaseScope ps(h, &tm.mean);
    launch_unpack_rhs<T>((const T*)h->scr.MT.p, ldm, M, k, 1.0, (T*)h->meanout.p, h->st);
  }
  if (h->bp) {  // + h^T beta, + |u|^2 (rows [k, k + bp) of MT are Z_H^T v* on the variance route)
    PhaseScope ps(h, want_var ? &tm.var : &tm.mean);
    launch_basis_epilogue<T>((const double*)h->Bst.p, h->bp, k, d, (const T*)h->scr.MT.p, ldm, (const T*)h->scr.Q.p, M,
                             (T*)h->meanout.p, want_var ? (T*)h->var.p : nullptr, nullptr, h->st);
  }
  return GPX_OK;
}

template <typename T>
int predict_impl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind,
                 const int32_t* gq = nullptr) {
  reset_predict_clocks(h->tm);
  int rc;
  {
    PhaseScope total(h, &h->tm.predict_total);
    if ((rc = predict_core<T>(h, Xq, M, var != nullptr, mem_kind, gq))) return rc;
    if ((rc = deliver_mean_var<T>(h, mean, var, M, mem_kind))) return rc;
  }
  return finish_call(h);
}

// The predict half of gpx_fit_predict: V^T already sits in the Mpad rows below the right-hand sides in the factor's buffer
// (fit_impl with query points); what is left is the mean V^T z and the row norms.
template <typename T>
int fused_predict_tail(gpx_handle* h, int64_t M, void* mean, void* var, int32_t mem_kind) {
  const int64_t Mpad = round_up(M, TILE), ldm = Mpad + ld_skew<T>();
  reset_predict_clocks(h->tm);
  int rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * sizeof(T)))) return rc;
  if ((rc = ensure_mean_partials<T>(h, h->scr.MTpart, ldm))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * h->k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->var, (size_t)Mpad * sizeof(T)))) return rc;
  {
    PhaseScope total(h, &h->tm.predict_total);
    bordered_mean_var<T>(h, (const T*)h->Lfac + (h->Npad + RHS_ROWS) * h->ld, M, Mpad, ldm, var != nullptr);
    if ((rc = deliver_mean_var<T>(h, mean, var, M, mem_kind))) return rc;
  }
  return finish_call(h);
}

// ---- joint posterior (ABI v6: gpx_predict_cov, gpx_sample_posterior) ----------------------------------------------------
// Sigma = K(Xs, Xs) - V^T V with V^T = K* L^-T for ALL M query rows in one buffer (Sigma needs every pair of rows), then
// for samples L_S = chol(Sigma + (diag_add + j) I) and S^T = Z^T L_S^T.  Every buffer is scratch of its own (J*): the
// fit's factor, block inverses and z^T are only read, so a predict afterwards is bit for bit what it was before.
constexpr int POST_NB = 1024;         // panel width of the factorisation of Sigma
constexpr int64_t POST_ROWS = 8192;   // rows of Z^T per transform batch

// device bytes the call needs beyond the fit (the J* buffers and predict's small mean buffers); `have` = what those buffers
// hold already (ensure() frees and replaces them)
template <typename T>
size_t posterior_need(const gpx_handle* h, int64_t M, int64_t S, bool sample, bool z_host, bool out_host, size_t* have) {
  const size_t E = sizeof(T);
  const int64_t Mpad = round_up(M, TILE), lds = Mpad + ld_skew<T>(), k = h->k;
  double b = (double)Mpad * h->ld + (double)Mpad * lds;                                          // V^T, Sigma
  if (h->nbw == h->nb_pred) b += 2.0 * Mpad * (h->nbw + ld_skew<T>());                            // block-solve buffers
  b += (double)RHS_ROWS * (Mpad + ld_skew<T>()) * (1 + splitk_splits(h->Npad)) + (double)M * k;   // mean
  *have = h->scr.JVT.cap + h->scr.JTsol.cap + h->scr.JSig.cap;
  if (sample) {
    const int64_t ldp = POST_NB + ld_skew<T>(), nblk = (Mpad + POST_NB - 1) / POST_NB;
    const int64_t R = std::min<int64_t>(round_up(std::max<int64_t>(POST_ROWS / k, 1) * k, TILE), round_up(S * k, TILE));
    b += (double)Mpad * lds + (double)(Mpad / KB) * KB * KB + 2.0 * Mpad * ldp + (double)nblk * POST_NB * POST_NB +
         (double)POST_NB * ldp + 2.0 * R * lds;
    if (z_host) b += (double)S * M * k;
    if (out_host) b += (double)S * M * k;
    *have += h->scr.JSigF.cap + h->scr.JWinv.cap + h->scr.JP.cap + h->scr.JWblk.cap + h->scr.JUblk.cap + h->scr.JZT.cap + h->scr.JST.cap + h->scr.JZin.cap +
             h->scr.JOut.cap;
  }
  return (size_t)(b * E) + 4096;
}

// refused handles and the memory check: GPX_OK or the error (nothing computed yet)
template <typename T>
int posterior_check(gpx_handle* h, const char* fn, int64_t M, int64_t S, bool sample, bool z_host, bool out_host) {
  char buf[256];
  size_t have = 0;
  const size_t need = posterior_need<T>(h, M, S, sample, z_host, out_host, &have);
  size_t freeb = 0, totalb = 0;
  HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
  if ((double)need > (double)freeb + (double)have) {
    snprintf(buf, sizeof buf, "%s: M = %lld query points need %.3f GB of device memory, %.3f GB are free", fn, (long long)M,
             need / 1e9, ((double)freeb + (double)have) / 1e9);
    return fail(h, GPX_E_NOMEM, buf);
  }
  return GPX_OK;
}

// mean (h->meanout, M x k) and the LOWER triangle of Sigma (h->scr.JSig, Mpad x lds; padded rows identity).
// gq != null (the *_paths calls; a fit with path ids): the query points' path ids — K* and K(Xs, Xs) by the GROUPS builders.
template <typename T>
int posterior_cov_core(gpx_handle* h, const void* Xq, int64_t M, int32_t mem_kind, const int32_t* gq = nullptr) {
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld;
  const int d = h->d, k = h->k;
  const int64_t Mpad = round_up(M, TILE), lds = Mpad + ld_skew<T>(), ldm = Mpad + ld_skew<T>();
  gpx_timings& tm = h->tm;
  int rc;
  if ((rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.JVT, (size_t)Mpad * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JSig, (size_t)Mpad * lds * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * sizeof(T)))) return rc;
  if ((rc = ensure_mean_partials<T>(h, h->scr.MTpart, ldm))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * sizeof(T)))) return rc;
  SolveWork<T> sw;  // dense block solves, as predict
  if ((rc = dense_solve_work<T>(h, h->scr.JTsol, Mpad, &sw))) return rc;
  if (gq && (rc = ensure(h, h->scr.Qz, (size_t)Mpad * sizeof(T)))) return rc;
  if (h->bp && (rc = ensure(h, h->scr.BU, (size_t)M * RHS_ROWS * 8))) return rc;
  T* dVT = (T*)h->scr.JVT.p;
  T* dSig = (T*)h->scr.JSig.p;
  const int32_t* dg = nullptr;
  {
    PhaseScope ps(h, &tm.kstar);
    if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
    if (gq) {
      if ((rc = upload_query_ids(h, gq, M, mem_kind))) return rc;
      dg = (const int32_t*)h->scr.Qg.p;
    }
    kbuild_cross_fit<T>(h, (const T*)h->scr.Qs.p, M, Mpad, dVT, ld, dg);
  }
  {
    PhaseScope ps(h, &tm.trsm);
    if ((rc = solve_fwd_enqueue<T>(h, dVT, Mpad, (const T*)h->Lfac, ld, Npad, h->nb_pred, (const T*)h->Winv.p, &sw)))
      return rc;
  }
  {  // mean^T (64 x Mpad) = z^T V
    PhaseScope ps(h, &tm.mean);
    mean_product<T>(h, (T*)h->scr.MT.p, ldm, (const T*)h->zT, dVT, Mpad, (T*)h->scr.MTpart.p, ldm);
    launch_unpack_rhs<T>((const T*)h->scr.MT.p, ldm, M, k, 1.0, (T*)h->meanout.p, h->st);
    if (h->bp)
      launch_basis_epilogue<T>((const double*)h->Bst.p, h->bp, k, d, (const T*)h->scr.MT.p, ldm, (const T*)h->scr.Q.p, M,
                               (T*)h->meanout.p, nullptr, (double*)h->scr.BU.p, h->st);
  }
  {  // Sigma = K(Xs, Xs) - (V^T)(V^T)^T: lower 64-tiles of the kernel (the block above the diagonal inside a 128-tile is
     // not built: zero it first), then one SYRK over the lower triangle
    PhaseScope ps(h, &tm.var);
    HIPCHK(h, hipMemsetAsync(dSig, 0, (size_t)Mpad * lds * sizeof(T), h->st));
    if (dg) {  // (the GROUPS builder reads a finished per-row diagonal term: none here)
      HIPCHK(h, hipMemsetAsync(h->scr.Qz.p, 0, (size_t)Mpad * sizeof(T), h->st));
      launch_kbuild_sym_g<T>(h->cfg.kernel, (const T*)h->scr.Qs.p, M, Mpad, d, h->sf2, dg, (const double*)h->Gq.p, h->sg2,
                             (const T*)h->scr.Qz.p, dSig, lds, h->st);
    } else {
      launch_kbuild_sym<T>(h->cfg.kernel, (const T*)h->scr.Qs.p, M, Mpad, d, h->sf2, 0.0, dSig, lds, h->st);
    }
    launch_gemm_nt<T>(128, dSig, lds, dVT, ld, dVT, ld, Mpad, Mpad, Npad, 1, 0, h->st);
    if (h->bp) launch_cov_add_uut<T>(dSig, lds, M, h->bp, (const double*)h->scr.BU.p, h->st);  // + U U^T (lower; mirrored later)
  }
  return GPX_OK;
}

template <typename T>
int predict_cov_impl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* cov, int32_t mem_kind,
                     const int32_t* gq = nullptr) {
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  int rc;
  if ((rc = posterior_check<T>(h, "gpx_predict_cov", M, 0, false, false, false))) return rc;
  const int64_t Mpad = round_up(M, TILE), lds = Mpad + ld_skew<T>();
  {
    PhaseScope total(h, &tm.predict_total);
    if ((rc = posterior_cov_core<T>(h, Xq, M, mem_kind, gq))) return rc;
    {
      PhaseScope ps(h, &tm.var);
      launch_mirror_lower<T>((T*)h->scr.JSig.p, lds, Mpad, 0, h->st);  // bit-symmetric copy-out
    }
    PhaseScope ps(h, &tm.d2h);
    if (mean && (rc = copy_out(h, mean, h->meanout.p, (size_t)M * h->k * sizeof(T), mem_kind))) return rc;
    HIPCHK(h, hipMemcpy2DAsync(cov, (size_t)M * sizeof(T), h->scr.JSig.p, (size_t)lds * sizeof(T), (size_t)M * sizeof(T),
                               (size_t)M, mem_kind == GPX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               h->st));
  }
  return finish_call(h);
}

template <typename T>
int sample_posterior_impl(gpx_handle* h, const void* Xq, int64_t M, int64_t S, uint64_t seed, const void* z,
                          double diag_add, double jitter, int32_t max_tries, void* out, double* jitter_used, int64_t* info,
                          int32_t mem_kind, const int32_t* gq = nullptr) {
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  const bool host = mem_kind == GPX_MEM_HOST;
  int rc;
  if ((rc = posterior_check<T>(h, "gpx_sample_posterior", M, S, true, z && host, host))) return rc;
  const int k = h->k;
  const int64_t Mpad = round_up(M, TILE), lds = Mpad + ld_skew<T>(), ldp = POST_NB + ld_skew<T>();
  const int64_t total = S * k;                                                   // rows of Z^T / S^T
  const int64_t Rb = std::max<int64_t>(POST_ROWS / k, 1) * k;                    // whole samples per batch
  const int64_t Rpad = std::min(round_up(Rb, TILE), round_up(total, TILE));      // buffer rows
  const size_t outn = (size_t)S * M * k;
  const int64_t nblk = (Mpad + POST_NB - 1) / POST_NB;
  if ((rc = ensure(h, h->scr.JSigF, (size_t)Mpad * lds * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JWinv, (size_t)(Mpad / KB) * KB * KB * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JP, (size_t)2 * Mpad * ldp * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JWblk, (size_t)nblk * POST_NB * POST_NB * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JUblk, (size_t)POST_NB * ldp * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JInfo, 64))) return rc;
  if ((rc = ensure(h, h->scr.JZT, (size_t)Rpad * lds * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.JST, (size_t)Rpad * lds * sizeof(T)))) return rc;
  if (z && host && (rc = ensure(h, h->scr.JZin, outn * sizeof(T)))) return rc;
  if (host && (rc = ensure(h, h->scr.JOut, outn * sizeof(T)))) return rc;
  T* dF = (T*)h->scr.JSigF.p;
  int* dInfo = (int*)h->scr.JInfo.p;
  const T* dz = (const T*)z;
  T* dout = host ? (T*)h->scr.JOut.p : (T*)out;
  // the factorisation books its trailing updates into the fit's counters: they stay the fit's, on every way out
  struct KeepFitClocks {
    gpx_timings& tm;
    const gpx_timings saved;
    ~KeepFitClocks() {
      tm.syrk_flops = saved.syrk_flops, tm.syrk_launches = saved.syrk_launches;
      tm.chol_diag = saved.chol_diag, tm.chol_trsm = saved.chol_trsm, tm.chol_strip = saved.chol_strip;
      tm.chol_syrk = saved.chol_syrk;
    }
  } keep_fit_clocks{tm, tm};
  double j = jitter;
  int hinfo = INT_MAX;
  {
    PhaseScope total_ps(h, &tm.predict_total);
    if ((rc = posterior_cov_core<T>(h, Xq, M, mem_kind, gq))) return rc;
    const T* dSig = (const T*)h->scr.JSig.p;  // (allocated by the core)
    if (z && host) {
      PhaseScope ps(h, &tm.kstar);
      if ((rc = copy_in(h, h->scr.JZin.p, z, outn * sizeof(T), GPX_MEM_HOST))) return rc;
      dz = (const T*)h->scr.JZin.p;
    }
    {  // factorisation (jitter escalation) and transform
      PhaseScope ps(h, &tm.var);
      for (int t = 0; t < max_tries; ++t) {  // Sigma stays as built: every attempt starts from a fresh copy of it
        if (t > 0) j = std::max(j, 1e-12 * h->sf2) * 10.0;
        launch_copy2d<T>(dF, lds, dSig, lds, Mpad, Mpad, h->st);
        launch_fix_diag<T>(dF, lds, (int)Mpad, (int)M, diag_add + j, h->st);
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)dInfo, INT_MAX, 1, h->st));
        InvWork<T> iw;
        iw.W = (T*)h->scr.JWblk.p;
        iw.U = (T*)h->scr.JUblk.p;
        iw.ldu = ldp;
        iw.nbw = POST_NB;
        iw.aux = h->st3;
        if ((rc = chol_enqueue<T>(h, dF, lds, Mpad, POST_NB, (T*)h->scr.JWinv.p, (T*)h->scr.JP.p, (T*)h->scr.JP.p + Mpad * ldp, ldp,
                                  dInfo, 0, false, 0, &iw)))
          return rc;
        HIPCHK(h, hipMemcpyAsync(&hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        LAUNCHCHK(h);
        if (hinfo < 0)
          return fail(h, GPX_E_HIP,
                      "gpx_sample_posterior: a stream parked on a device flag timed out: kernels are being serialised "
                      "across streams — set GPX_CHAIN_FLAG=0 to hand over by hipEvents instead");
        if (hinfo == INT_MAX) break;
      }
      if (hinfo == INT_MAX) {
        launch_mirror_lower<T>(dF, lds, Mpad, 1, h->st);  // the product reads B's diagonal tiles whole: zero above L_S
        for (int64_t r0 = 0; r0 < total; r0 += Rb) {
          const int64_t rows = std::min(Rb, total - r0), rpad = round_up(rows, TILE);
          launch_normals<T>((T*)h->scr.JZT.p, lds, r0, rpad, total, M, Mpad, k, seed, dz, h->st);
          launch_gemm_nt<T>(128, (T*)h->scr.JST.p, lds, (const T*)h->scr.JZT.p, lds, dF, lds, rpad, Mpad, Mpad, 4, 1, h->st);
          launch_sample_epilogue<T>((const T*)h->scr.JST.p, lds, r0, rows, (const T*)h->meanout.p, M, k, dout, h->st);
        }
      }
    }
    if (hinfo == INT_MAX && host) {
      PhaseScope ps2(h, &tm.d2h);
      if ((rc = copy_out(h, out, dout, outn * sizeof(T), mem_kind))) return rc;
    }
  }
  *jitter_used = j;
  *info = hinfo == INT_MAX ? 0 : (int64_t)hinfo;
  return finish_call(h);
}

// ---- joint density of blocks of query points (gpx_score_blocks) -------------------------------------------
// predict_core's batch loop with whole blocks per batch: floor(MB / Lg) blocks, their rows padded to 128 for the solve, so
// no block straddles two V^T buffers; the row norms of predict give way to the per-block Gram of V^T and the block
// factorisation (gpx_score.hip).  V^T, its solve buffers and the mean product's buffers are predict's own scratch; the fit
// is only read.

// device bytes per row of a batch beyond the fit: V^T, the two compact solve buffers, the Gram partials of its share of a block
template <typename T>
size_t score_row_bytes(const gpx_handle* h, int Lg) {
  const int LP = score_lp(Lg);
  size_t b = (size_t)h->ld * sizeof(T);
  if (h->nbw == h->nb_pred) b += (size_t)2 * (h->nbw + ld_skew<T>()) * sizeof(T);
  return b + ((size_t)score_slices(h->Npad) * LP * LP * sizeof(double) + Lg - 1) / Lg;
}

// gpx_forecast_blocks is the same batch loop with Lg = Lo + Lp rows per block, of which the first Lo carry targets, and
// block_forecast_kernel in place of block_score_kernel: `fc` says so (null: scoring).
struct ForecastOut {
  int Lp;                          // rows to forecast per block (Lo = Lg - Lp observed ones before them)
  void *mean, *cov, *var, *logp;   // the caller's outputs (cov, var, logp may be null)
};

template <typename T>
int score_impl(gpx_handle* h, const void* Xq, const void* yq, const void* wq, int64_t G, int32_t Lg, double diag_add,
               void* logp, void* maha, void* logdet, int32_t mem_kind, int64_t* info, const ForecastOut* fc = nullptr) {
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld, M = G * Lg;
  const int d = h->d, k = h->k;
  const int Lp = fc ? fc->Lp : 0, Lo = Lg - Lp;  // rows of a block that carry targets: Lo (scoring: all Lg)
  const int64_t My = G * Lo;
  const double sg2 = h->grouped ? h->sg2 : 0.0;  // a fit with path ids: every block is a new path
  const double* dq = h->grouped ? (const double*)h->Gq.p : nullptr;
  const int64_t Mpad = round_up(M, TILE);
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  int rc;
  {  // not one 128-row batch beside what the call keeps per query point: refused before anything is allocated
    const size_t row_bytes = score_row_bytes<T>(h, Lg);
    const size_t E = sizeof(T);
    const double small = (double)(M + 2 * TILE) * d * 2 * E + (double)M * (2 * k + (wq ? 1 : 0)) * E + (double)G * (2 * k + 1) * E +
                         (double)G * Lp * (k + Lp + 1) * E + (double)RHS_ROWS * (TILE + ld_skew<T>()) * (1 + splitk_splits(Npad)) * E + 4096;
    const double need = (double)TILE * row_bytes + small;
    const double have = (double)h->scr.VT.cap + h->scr.Tsol.cap + h->scr.SPart.cap + h->scr.Q.cap + h->scr.Qs.cap + h->scr.SY.cap +
                        h->scr.SOut.cap + h->scr.SMT.cap + h->scr.MTpart.cap + h->meanout.cap +
                        (wq ? h->scr.SW.cap : 0);
    size_t freeb = 0, totalb = 0;
    HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
    if (need > (double)freeb + have) {
      char buf[256];
      snprintf(buf, sizeof buf, "%s: one batch of 128 rows needs %.3f GB of device memory, %.3f GB are free",
               fc ? "gpx_forecast_blocks" : "gpx_score_blocks", need / 1e9, ((double)freeb + have) / 1e9);
      return fail(h, GPX_E_NOMEM, buf);
    }
  }
  const int64_t MB = pred_batch_rows(h, Mpad, score_row_bytes<T>(h, Lg), true);
  const int64_t bpb = std::min<int64_t>(G, MB / Lg);  // whole blocks per batch (MB >= 128 >= 2 Lg)
  const int64_t rows_b = round_up(bpb * Lg, TILE);     // <= MB
  const int64_t ldmb = rows_b + ld_skew<T>();
  const int S = score_slices(Npad), LP = score_lp(Lg);
  // a batch reads rows_b rows of Qs from its first block on: up to 127 rows beyond M
  if ((rc = ensure_queries<T>(h, M + TILE))) return rc;
  if ((rc = ensure(h, h->scr.SY, (size_t)My * k * sizeof(T)))) return rc;
  if (wq && (rc = ensure(h, h->scr.SW, (size_t)M * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.VT, (size_t)rows_b * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.SMT, (size_t)RHS_ROWS * ldmb * sizeof(T)))) return rc;
  if ((rc = ensure_mean_partials<T>(h, h->scr.MTpart, ldmb))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.SPart, (size_t)bpb * S * LP * LP * sizeof(double)))) return rc;
  if (h->bp && (rc = ensure(h, h->scr.BU, (size_t)bpb * Lg * RHS_ROWS * 8))) return rc;
  const double* dU = h->bp ? (const double*)h->scr.BU.p : nullptr;  // a batch's u rows, from its first row
  const size_t out_elems = fc ? (size_t)G * Lp * (k + Lp + 1) + (size_t)G * k : (size_t)G * (2 * k + 1);
  const size_t bad_off = round_up((int64_t)(out_elems * sizeof(T)), 16);
  DevBuf& outbuf = h->scr.SOut;
  if ((rc = ensure(h, outbuf, bad_off + 16))) return rc;
  SolveWork<T> sw;
  if ((rc = dense_solve_work<T>(h, h->scr.Tsol, rows_b, &sw))) return rc;
  T* dVT = (T*)h->scr.VT.p;
  T* dMT = (T*)h->scr.SMT.p;
  // the results of a call, one layout per kind of call (out_elems above), the bad-block word behind either:
  //   scoring   logp (G, k) | maha (G, k) | logdet (G)
  //   forecast  logp (G, k) | mean (G Lp, k) | cov (G, Lp, Lp) | var (G Lp)
  T* dLogp = (T*)outbuf.p;
  T* dMaha = dLogp + G * k;
  T* dLogdet = dMaha + G * k;
  T* dFmean = dLogp + G * k;
  T* dFcov = dFmean + G * Lp * k;
  T* dFvar = dFcov + G * Lp * Lp;
  int* dBad = (int*)((char*)outbuf.p + bad_off);
  const T* dQs = (const T*)h->scr.Qs.p;
  int hbad = INT_MAX;
  {
    PhaseScope total(h, &tm.predict_total);
    {
      PhaseScope ps(h, &tm.kstar);
      if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
      HIPCHK(h, hipMemsetAsync((T*)h->scr.Qs.p + Mpad * d, 0, (size_t)TILE * d * sizeof(T), h->st));
      if ((rc = copy_in(h, h->scr.SY.p, yq, (size_t)My * k * sizeof(T), mem_kind))) return rc;
      if (wq && (rc = copy_in(h, h->scr.SW.p, wq, (size_t)M * sizeof(T), mem_kind))) return rc;
      const int init = INT_MAX;
      HIPCHK(h, hipMemcpyAsync(dBad, &init, sizeof(int), hipMemcpyHostToDevice, h->st));
    }
    for (int64_t g0 = 0; g0 < G; g0 += bpb) {  // batches of whole blocks through one V^T buffer
      const int64_t nb = std::min(bpb, G - g0), m0 = g0 * Lg;
      const int64_t mv = nb * Lg, mp = round_up(mv, TILE);
      {
        PhaseScope ps(h, &tm.kstar);
        kbuild_cross_fit<T>(h, dQs + m0 * d, mv, mp, dVT, ld);
      }
      {
        PhaseScope ps(h, &tm.trsm);
        if ((rc = solve_fwd_enqueue<T>(h, dVT, mp, (const T*)h->Lfac, ld, Npad, h->nb_pred, (const T*)h->Winv.p, &sw))) return rc;
      }
      {  // mean^T (64 x mp) = z^T V, then the batch's rows of the mean (M, k)
        PhaseScope ps(h, &tm.mean);
        mean_product<T>(h, dMT, ldmb, (const T*)h->zT, dVT, mp, (T*)h->scr.MTpart.p, ldmb);
        launch_unpack_rhs<T>(dMT, ldmb, mv, k, 1.0, (T*)h->meanout.p + m0 * k, h->st);
        if (h->bp)
          launch_basis_epilogue<T>((const double*)h->Bst.p, h->bp, k, d, dMT, ldmb, (const T*)h->scr.Q.p + m0 * d, mv,
                                   (T*)h->meanout.p + m0 * k, nullptr, (double*)h->scr.BU.p, h->st);
      }
      {
        PhaseScope ps(h, &tm.var);
        launch_block_gram<T>(dVT, ld, nb, Lg, Npad, (double*)h->scr.SPart.p, h->st);
        if (fc)
          launch_block_forecast<T>(h->cfg.kernel, (const double*)h->scr.SPart.p, nb, Lo, Lp, Npad, dQs + m0 * d, d,
                                   (const T*)h->scr.SY.p + g0 * Lo * k, (const T*)h->meanout.p + m0 * k, k, h->sf2, sg2, dq,
                                   diag_add, dFmean, dFcov, dFvar, dLogp, g0, dBad, h->st, dU, h->bp);
        else
          launch_block_score<T>(h->cfg.kernel, (const double*)h->scr.SPart.p, nb, Lg, Npad, dQs + m0 * d, d,
                                (const T*)h->scr.SY.p + m0 * k, (const T*)h->meanout.p + m0 * k, k, h->sf2, diag_add, dLogp,
                                dMaha, dLogdet, g0, dBad, h->st, wq ? (const T*)h->scr.SW.p + m0 : nullptr, sg2, dq, dU,
                                h->bp);
      }
    }
    PhaseScope ps(h, &tm.d2h);
    if (fc) {
      if ((rc = copy_out(h, fc->mean, dFmean, (size_t)G * Lp * k * sizeof(T), mem_kind))) return rc;
      if (fc->cov && (rc = copy_out(h, fc->cov, dFcov, (size_t)G * Lp * Lp * sizeof(T), mem_kind))) return rc;
      if (fc->var && (rc = copy_out(h, fc->var, dFvar, (size_t)G * Lp * sizeof(T), mem_kind))) return rc;
      if (fc->logp && (rc = copy_out(h, fc->logp, dLogp, (size_t)G * k * sizeof(T), mem_kind))) return rc;
    } else if ((rc = copy_out(h, logp, dLogp, (size_t)G * k * sizeof(T), mem_kind))) {
      return rc;
    }
    if (maha && (rc = copy_out(h, maha, dMaha, (size_t)G * k * sizeof(T), mem_kind))) return rc;
    if (logdet && (rc = copy_out(h, logdet, dLogdet, (size_t)G * sizeof(T), mem_kind))) return rc;
    HIPCHK(h, hipMemcpyAsync(&hbad, dBad, sizeof(int), hipMemcpyDeviceToHost, h->st));
  }
  if ((rc = finish_call(h))) return rc;
  *info = hbad == INT_MAX ? 0 : (int64_t)hbad;
  return GPX_OK;
}

// ---- posterior gradient (gpx_predict_grad) -------------------------------------------------------------------------
// Mean only (var and dvar NULL): dmean = dK* alpha with the cached alpha, matrix-free (launch_kgrad_matvec); no solve,
// nothing of size M N is stored; `mean` comes from predict's own mean-only path.
// Otherwise, per batch of MB query points (GPX_PRED_BATCH, shrunk to what the card holds): V = [K*;] d_1 K*; ...; d_d K*
// (nblk row blocks of mp rows each) -> ONE forward solve over the nblk mp rows -> ONE split-K z^T V (mean and dmean
// together) -> row norms against the per-block prior -> unpack.  Every buffer is scratch of its own (G*): the fit is only
// read, so gpx_predict afterwards is bit-identical.
// gpx_predict_hess is the same two routes with `order` = 2: the hess_pairs(d) second derivatives per query
// point in place of the d first ones (nd below), no value rows, gpx_hess.hip's build and matrix-free product.

// prior[b] of the row blocks: sf2 (value rows), then Var[d f / d x_j] = cov::grad_prior sf2 / l_j^2.
// prior_path != null (a fit with path ids): what a query point with a path id adds, sg2 and
// Var[d g_p / d x_j] = cov::grad_prior sg2 / l_path,j^2 = cov::grad_prior sg2 q_j / l_j^2.
// order 2 (gpx_predict_hess): the pairs (i, j), i <= j, instead: Var[d_i d_j f] = c2 sf2 / (l_i^2 l_j^2), three
// times that for i == j, c2 = cov::hess_prior; a path id adds the same in sg2 and l_path (1 / l_path,j^2 = q_j / l_j^2).
int grad_priors(gpx_handle* h, bool with_value, double* prior, double* prior_path = nullptr, int order = 1) {
  double ls[MAX_D];
  HIPCHK(h, hipMemcpyAsync(ls, h->ls.p, (size_t)h->n_ls * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  int b = 0;
  if (order == 2) {
    const double c2 = cov::hess_prior(h->cfg.kernel);
    for (int i = 0; i < h->d; ++i)
      for (int j = i; j < h->d; ++j) {
        const double li = ls[h->n_ls == 1 ? 0 : i], lj = ls[h->n_ls == 1 ? 0 : j];
        const double w = (i == j ? 3.0 : 1.0) * c2 / (li * li * lj * lj);
        if (prior_path) prior_path[b] = w * h->sg2 * h->q_fit[(size_t)i] * h->q_fit[(size_t)j];
        prior[b++] = w * h->sf2;
      }
    return GPX_OK;
  }
  if (with_value) {
    if (prior_path) prior_path[b] = h->sg2;
    prior[b++] = h->sf2;
  }
  const double c = cov::grad_prior(h->cfg.kernel);
  for (int j = 0; j < h->d; ++j) {
    const double l = ls[h->n_ls == 1 ? 0 : j];
    if (prior_path) prior_path[b] = c * h->sg2 * h->q_fit[(size_t)j] / (l * l);
    prior[b++] = c * h->sf2 / (l * l);
  }
  return GPX_OK;
}

template <typename T>
int predict_grad_mean_only(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* dmean, int32_t mem_kind, int order) {
  const int d = h->d, k = h->k;
  const int nd = order == 2 ? hess_pairs(d) : d;  // derivatives per query point and target
  gpx_timings& tm = h->tm;
  int rc;
  int KC = 1, S = 1;
  int64_t chunk = 0;
  kgrad_matvec_shape(M, h->Npad, d, k, &KC, &S, &chunk);
  if (mean) {
    if ((rc = predict_core<T>(h, Xq, M, false, mem_kind))) return rc;  // gpx_predict's mean; leaves Qs scaled
  } else {
    if ((rc = ensure_alpha<T>(h))) return rc;
    if ((rc = ensure_queries<T>(h, M))) return rc;
    PhaseScope ps(h, &tm.kstar);
    if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
  }
  if ((rc = ensure(h, h->scr.GPart, (size_t)S * k * nd * round_up(M, 64) * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.GOut, (size_t)M * nd * k * sizeof(T)))) return rc;
  {
    PhaseScope ps(h, &tm.mean);
    const auto matvec = order == 2 ? launch_khess_matvec<T> : launch_kgrad_matvec<T>;  // (one signature)
    matvec(h->cfg.kernel, (const T*)h->scr.Qs.p, M, (const T*)h->Xs.p, h->Npad, d, h->sf2, (const T*)h->alphaT, h->ld, k,
           (const double*)h->ls.p, h->n_ls, (T*)h->scr.GPart.p, (T*)h->scr.GOut.p, h->st);
  }
  PhaseScope ps(h, &tm.d2h);
  if (mean && (rc = copy_out(h, mean, h->meanout.p, (size_t)M * k * sizeof(T), mem_kind))) return rc;
  return copy_out(h, dmean, h->scr.GOut.p, (size_t)M * nd * k * sizeof(T), mem_kind);
}

template <typename T>
int predict_grad_var(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, void* dmean, void* dvar,
                     int32_t mem_kind, const char* fn, const int32_t* gq, int order) {
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld;
  const int d = h->d, k = h->k;
  const int nd = order == 2 ? hess_pairs(d) : d;  // derivatives per query point and target: dmean (M, nd, k), dvar (M, nd)
  const size_t E = sizeof(T);
  const int64_t Mpad = round_up(M, TILE);
  const bool with_value = mean || var;  // (never with order 2)
  const int nblk = nd + (with_value ? 1 : 0);
  const int ksplit = splitk_splits(Npad);
  const bool dense = h->nbw == h->nb_pred;  // the fit's block inverses, same block width: dense block solves
  const int64_t ldt = h->nbw + ld_skew<T>();
  // device bytes per padded query point of a batch (V, block-solve buffers, z^T V and its split-K partials, norms),
  // and the fixed part (queries, outputs, the skew columns of the product buffers)
  const double per_pt = (double)E * nblk * ((double)ld + (dense ? 2.0 * ldt : 0.0) + RHS_ROWS * (1.0 + ksplit) + 1.0);
  const double fixed = (double)E * ((double)M * d + (double)Mpad * d + (double)M * (k + 1) * (nd + 1) +
                                    (double)RHS_ROWS * ld_skew<T>() * (1 + ksplit)) + 4096.0;
  const size_t have = h->scr.GV.cap + h->scr.GTsol.cap + h->scr.GMT.cap + h->scr.GMTpart.cap + h->scr.GVN.cap + h->scr.GOut.cap;
  size_t freeb = 0, totalb = 0;
  HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
  const double avail = (double)freeb + (double)have;
  if (128.0 * per_pt + fixed > avail) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: one batch of 128 query points needs %.3f GB of device memory, %.3f GB are free", fn,
             (128.0 * per_pt + fixed) / 1e9, avail / 1e9);
    return fail(h, GPX_E_NOMEM, buf);
  }
  const int64_t fit = (int64_t)((0.8 * avail - fixed) / per_pt) / 128 * 128;
  const int64_t MB = std::min(pred_batch_rows(h, Mpad, 0, false), std::max<int64_t>(128, fit));
  const int64_t RB = nblk * MB;                 // rows of the largest batch
  const int64_t ldm = RB + ld_skew<T>();        // z^T V of one batch
  double prior[PRIOR_SLOTS], prior_path[PRIOR_SLOTS];
  int rc;
  if ((rc = grad_priors(h, with_value, prior, gq ? prior_path : nullptr, order))) return rc;
  if ((rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.GV, (size_t)RB * ld * E))) return rc;
  if ((rc = ensure(h, h->scr.GMT, (size_t)RHS_ROWS * ldm * E))) return rc;
  if ((rc = ensure_mean_partials<T>(h, h->scr.GMTpart, ldm))) return rc;
  if ((rc = ensure(h, h->scr.GVN, (size_t)RB * E))) return rc;
  const int64_t o_dvar = M * nd * k, o_mean = o_dvar + M * nd, o_var = o_mean + M * k;
  if ((rc = ensure(h, h->scr.GOut, (size_t)(o_var + M) * E))) return rc;
  SolveWork<T> sw;
  if ((rc = dense_solve_work<T>(h, h->scr.GTsol, RB, &sw))) return rc;
  T* dV = (T*)h->scr.GV.p;
  T* out = (T*)h->scr.GOut.p;
  gpx_timings& tm = h->tm;
  {
    PhaseScope ps(h, &tm.kstar);
    if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
    if (gq && (rc = upload_query_ids(h, gq, M, mem_kind))) return rc;
  }
  const int32_t* dg = gq ? (const int32_t*)h->scr.Qg.p : nullptr;  // (a fit with path ids: the query points' own)
  for (int64_t m0 = 0; m0 < Mpad; m0 += MB) {
    const int64_t mp = std::min(MB, Mpad - m0);        // padded rows of this batch (a multiple of 128)
    const int64_t mv = std::min<int64_t>(mp, M - m0);  // valid rows
    const int64_t R = nblk * mp;                       // rows of V in this batch
    const int64_t ldb = R + ld_skew<T>();
    {
      PhaseScope ps(h, &tm.kstar);
      const int32_t* kfit = h->kinded ? (const int32_t*)h->Kfit.p : nullptr;
      if (order == 2)
        launch_khess_build<T>(h->cfg.kernel, (const T*)h->scr.Qs.p + m0 * d, dg ? dg + m0 : nullptr, mv, mp, (const T*)h->Xs.p,
                              dg ? (const int32_t*)h->Gfit.p : kfit, N, Npad, d, h->sf2, (const double*)h->ls.p, h->n_ls,
                              dg ? (const double*)h->Gq.p : nullptr, h->sg2, dV, ld, h->st);
      else if (dg)
        launch_kgrad_build_g<T>(h->cfg.kernel, (const T*)h->scr.Qs.p + m0 * d, dg + m0, mv, mp, (const T*)h->Xs.p,
                                (const int32_t*)h->Gfit.p, N, Npad, d, h->sf2, (const double*)h->ls.p, h->n_ls,
                                (const double*)h->Gq.p, h->sg2, with_value ? 1 : 0, dV, ld, h->st);
      else
        launch_kgrad_build<T>(h->cfg.kernel, (const T*)h->scr.Qs.p + m0 * d, mv, mp, (const T*)h->Xs.p, N, Npad, d, h->sf2,
                              (const double*)h->ls.p, h->n_ls, with_value ? 1 : 0, dV, ld, h->st, kfit);
    }
    {
      PhaseScope ps(h, &tm.trsm);
      if ((rc = solve_fwd_enqueue<T>(h, dV, R, (const T*)h->Lfac, ld, Npad, h->nb_pred, (const T*)h->Winv.p, &sw)))
        return rc;
    }
    {  // (mean | dmean)^T (64 x R) = z^T V
      PhaseScope ps(h, &tm.mean);
      mean_product<T>(h, (T*)h->scr.GMT.p, ldb, (const T*)h->zT, dV, R, (T*)h->scr.GMTpart.p, ldb);
    }
    {
      PhaseScope ps(h, &tm.var);
      launch_grad_norms<T>(dV, ld, mp, mv, nblk, Npad, prior, (T*)h->scr.GVN.p, h->st, dg ? dg + m0 : nullptr, prior_path);
    }
    {
      PhaseScope ps(h, &tm.mean);
      launch_grad_unpack<T>((const T*)h->scr.GMT.p, ldb, (const T*)h->scr.GVN.p, mp, mv, nblk, nd, k, with_value ? 1 : 0,
                            out + o_mean + m0 * k, out + o_var + m0, out + m0 * nd * k, out + o_dvar + m0 * nd, h->st);
    }
  }
  PhaseScope ps(h, &tm.d2h);
  if ((rc = copy_out(h, dmean, out, (size_t)M * nd * k * E, mem_kind))) return rc;
  if (dvar && (rc = copy_out(h, dvar, out + o_dvar, (size_t)M * nd * E, mem_kind))) return rc;
  if (mean && (rc = copy_out(h, mean, out + o_mean, (size_t)M * k * E, mem_kind))) return rc;
  if (var && (rc = copy_out(h, var, out + o_var, (size_t)M * E, mem_kind))) return rc;
  return GPX_OK;
}

template <typename T>
int predict_grad_impl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, void* dmean, void* dvar,
                      int32_t mem_kind, const int32_t* gq, const char* fn, int order) {
  reset_predict_clocks(h->tm);
  int rc;
  {
    PhaseScope total(h, &h->tm.predict_total);
    // (the matrix-free product knows neither derivative columns nor path ids: the batch route then)
    if (!var && !dvar && !h->has_deriv && !gq)
      rc = predict_grad_mean_only<T>(h, Xq, M, mean, dmean, mem_kind, order);
    else
      rc = predict_grad_var<T>(h, Xq, M, mean, var, dmean, dvar, mem_kind, fn, gq, order);
    if (rc) return rc;
  }
  return finish_call(h);
}

// ZT <- ZT * L^-T = L^-T restricted to the rows this rank owns: the forward substitution of
// solve_fwd_enqueue on the rows that are not structurally zero.  Row r of L^-T is zero left of
// column r and the rows are independent (a right-hand multiplication), so the row blocks of
// height nb are dealt block-cyclically over P ranks with no exchange: rank `rank` keeps its blocks
// b = rank, rank + P, ... stacked in ZT (local block j = global block j P + rank, the identity at
// columns [b nb, b nb + nb) on entry), and column block [o, o + nb) only involves the local rows of
// the blocks below o / nb — a prefix of the stack.  P = 1: the whole L^-T in place, N^3/3 flops;
// same STRIP / REST look-ahead as the factorisation.
int trtri_enqueue(gpx_handle* h, double* ZT, const double* L, int64_t ld, int64_t n, int nb,
                  const double* Winv, int P, int rank) {
  hipStream_t s0 = h->st, s1 = h->st2;
  auto rows_below = [&](int64_t t) -> int64_t {  // local rows of the own blocks with index < t / nb
    const int64_t q = t / nb;
    return q > rank ? (q - rank + P - 1) / P * nb : 0;
  };
  auto own = [&](int64_t t) { return (int)((t / nb) % P) == rank; };
  if (own(0))
    launch_trsm_rlt<double>(ZT, ld, std::min<int64_t>(nb, n), L, ld, Winv, (int)std::min<int64_t>(nb, n), nullptr, 0, s0);
  for (int64_t o = 0; o < n; o += nb) {
    const int nbp = (int)std::min<int64_t>(nb, n - o);
    const int64_t t0 = o + nbp, ntrail = n - t0;
    if (ntrail <= 0) break;
    const int nbn = (int)std::min<int64_t>(nb, ntrail);
    const int64_t nrest = ntrail - nbn;
    const int64_t R = rows_below(t0);                    // local rows that are non-zero in column block o
    const int64_t Rn = R + (own(t0) ? nbn : 0);          // ... plus the identity rows of block t0 / nb
    const int tl = (R % 128 == 0 && nbn % 128 == 0 && nrest % 128 == 0) ? 128 : 64;
    if (R > 0) launch_gemm_nt<double>(tl, ZT + t0, ld, ZT + o, ld, L + t0 * ld + o, ld, R, nbn, nbp, 0, 0, s0);  // STRIP
    hipEvent_t e_strip = next_event(h), e_blk = next_event(h);
    if (!e_strip || !e_blk) return fail(h, GPX_E_HIP, "hipEventCreate failed (look-ahead)");
    HIPCHK(h, hipEventRecord(e_strip, s0));
    HIPCHK(h, hipStreamWaitEvent(s1, e_strip, 0));
    if (Rn > 0)
      launch_trsm_rlt<double>(ZT + t0, ld, Rn, L + t0 * ld + t0, ld, Winv + (t0 / KB) * (KB * KB), nbn, nullptr, 0, s1);
    HIPCHK(h, hipEventRecord(e_blk, s1));
    if (nrest > 0 && R > 0)  // REST
      launch_gemm_nt<double>(tl, ZT + t0 + nbn, ld, ZT + o, ld, L + (t0 + nbn) * ld + o, ld, R, nrest, nbp, 0, 0,
                             s0);
    HIPCHK(h, hipStreamWaitEvent(s0, e_blk, 0));
  }
  return GPX_OK;
}

// the block width of the L^-T sweeps: their measured 1024-blocks whatever the fit's panel width (GPX_NB_GRAD overrides: A/B)
int zt_block(const gpx_handle* h) { return h->env.nb_grad ? h->env.nb_grad : std::min(h->nb_pred, 1024); }

// scr.ZT <- L^-T of the current fit, whole, on one device (lml_grad_impl with P = 1, loo_impl): N^3 / 3 flops on the tile
// engine.  Always built anew — the handle does not remember that it holds one — and scratch afterwards.
int build_zt(gpx_handle* h) {
  const int64_t Npad = h->Npad, ld = h->ld;
  int rc;
  if ((rc = ensure(h, h->scr.ZT, (size_t)Npad * ld * 8))) return rc;
  double* ZT = (double*)h->scr.ZT.p;
  HIPCHK(h, hipMemsetAsync(ZT, 0, (size_t)Npad * ld * 8, h->st));
  launch_set_diag_one(ZT, ld, Npad, h->st);
  return trtri_enqueue(h, ZT, (const double*)h->Lfac, ld, Npad, zt_block(h), (const double*)h->Winv.p, 1, 0);
}

// Gradient of the log marginal likelihood.  Sharded handles (replicated factor: every rank holds
// the whole L): L^-T in row blocks dealt over the ranks (no exchange), one all-gather of its
// non-zero part (block b: rows x columns >= b nb, packed), the fused K^-1 trace pass with the
// tile groups dealt over the ranks, one all-reduce of ntheta sums.  alpha and its quadratic
// form are replicated work (O(N^2)), identical on every rank.
// kinds (gpx_lml_grad_full on a fit with derivative observations; one device): the KINDS instantiations of both passes,
// theta = (lengthscales..., sf2, sn2, sn2_deriv).
// grad_path (gpx_lml_grad_paths on a fit with path ids; one device): the GROUPS instantiations of both passes, theta =
// (lengthscales..., sf2, sn2, sg2, l_path...); the last 1 + n_lsp entries go to grad_path.
int lml_grad_impl(gpx_handle* h, double* lml, double* grad, bool kinds = false, double* grad_path = nullptr) {
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld;
  const bool paths = grad_path != nullptr;
  const int d = h->d, k = h->k, ntheta = h->n_ls + (kinds ? 3 : paths ? 3 + h->n_lsp : 2), ard = h->n_ls > 1;
  Comm* cm = h->comm;
  const int P = cm ? cm->world : 1, rank = cm ? cm->rank : 0;
  const int nb = zt_block(h);
  gpx_timings& tm = h->tm;
  tm.grad_trtri = tm.grad_trace = tm.grad_total = 0;
  const int64_t s1n = kinv_trace_slots(Npad), s2n = alpha_quad_slots(Npad);
  const int64_t nblk = (Npad + nb - 1) / nb;
  int64_t nloc = 0;  // rows of the own blocks (the last block may be ragged)
  for (int64_t b = rank; b < nblk; b += P) nloc += std::min<int64_t>(nb, Npad - b * nb);
  int rc;
  if ((rc = ensure_alpha<double>(h))) return rc;
  if ((rc = ensure(h, h->scr.ZT, (size_t)Npad * ld * 8))) return rc;
  if (P > 1) {
    if ((rc = ensure(h, h->scr.ZTloc, (size_t)std::max<int64_t>(nloc, 1) * ld * 8))) return rc;
    if ((rc = ensure(h, h->scr.ZTpack, (size_t)nb * Npad * 8))) return rc;
  }
  if ((rc = ensure(h, h->scr.gpart, (size_t)((s1n + s2n) * ntheta + 2 * ntheta + 1) * 8))) return rc;
  double* ZT = (double*)h->scr.ZT.p;
  double* Zl = P > 1 ? (double*)h->scr.ZTloc.p : ZT;
  double* part1 = (double*)h->scr.gpart.p;
  double* part2 = part1 + s1n * ntheta;
  double* outv = part2 + s2n * ntheta;  // [ntheta] K^-1 sums, [ntheta] alpha sums, [1] y . alpha
  // per-observation noise: dK / dlog sn2 = sn2 diag(w), so the noise entry of both passes takes w_i per row
  const double* wv = h->weighted ? (const double*)h->Wfit.p : nullptr;
  hipStream_t st = h->st;
  {
    PhaseScope total(h, &tm.grad_total);
    {
      PhaseScope ps(h, &tm.grad_trtri);
      if (P == 1) {
        if ((rc = build_zt(h))) return rc;
      } else {
        HIPCHK(h, hipMemsetAsync(Zl, 0, (size_t)nloc * ld * 8, st));
        int64_t j = 0;
        for (int64_t b = rank; b < nblk; b += P, ++j)
          launch_set_diag_one(Zl + j * nb * ld + b * nb, ld, std::min<int64_t>(nb, Npad - b * nb), st);
        if ((rc = trtri_enqueue(h, Zl, (const double*)h->Lfac, ld, Npad, nb, (const double*)h->Winv.p, P, rank)))
          return rc;
        // all-gather: block b from rank b % P, only the columns right of its zeros
        double* pack = (double*)h->scr.ZTpack.p;
        HIPCHK(h, hipMemsetAsync(ZT, 0, (size_t)Npad * ld * 8, st));
        for (int64_t b = 0; b < nblk; ++b) {
          const int64_t r0 = b * nb, hb = std::min<int64_t>(nb, Npad - r0), w = Npad - r0;
          const int root = (int)(b % P);
          if (root == rank) launch_copy2d<double>(pack, w, Zl + (b / P) * nb * ld + r0, ld, hb, w, st);
          if ((rc = cm->bcast(h, pack, (size_t)(hb * w), root, st))) return rc;
          launch_copy2d<double>(ZT + r0 * ld + r0, ld, pack, w, hb, w, st);
        }
      }
    }
    {
      PhaseScope ps(h, &tm.grad_trace);
      HIPCHK(h, hipMemsetAsync(part1, 0, (size_t)(s1n + s2n) * ntheta * 8, st));  // ragged-edge / other ranks' slots write nothing
      if (kinds)
        launch_kinv_trace_kinds(h->cfg.kernel, ZT, ld, Npad, N, (const double*)h->Xs.p, d, ard, h->sf2, h->sn2,
                                h->sn2_deriv, (const int32_t*)h->Kfit.p, (const double*)h->ls.p, h->n_ls, part1, ntheta,
                                st, wv);
      else if (paths)
        launch_kinv_trace_groups(h->cfg.kernel, ZT, ld, Npad, N, (const double*)h->Xs.p, d, ard, h->sf2, h->sn2, h->sg2,
                                 (const int32_t*)h->Gfit.p, (const double*)h->Gq.p, h->n_lsp, part1, ntheta, st, wv);
      else
        launch_kinv_trace(h->cfg.kernel, ZT, ld, Npad, N, (const double*)h->Xs.p, d, ard, h->sf2, h->sn2, part1,
                          ntheta, P, rank, st, wv);
    }
    if (kinds)
      launch_alpha_quad_kinds(h->cfg.kernel, (const double*)h->alphaT, ld, k, Npad, N, (const double*)h->Xs.p, d, ard,
                              h->sf2, h->sn2, h->sn2_deriv, (const int32_t*)h->Kfit.p, (const double*)h->ls.p, h->n_ls,
                              part2, ntheta, st, wv);
    else if (paths)
      launch_alpha_quad_groups(h->cfg.kernel, (const double*)h->alphaT, ld, k, Npad, N, (const double*)h->Xs.p, d, ard,
                               h->sf2, h->sn2, h->sg2, (const int32_t*)h->Gfit.p, (const double*)h->Gq.p, h->n_lsp, part2,
                               ntheta, st, wv);
    else
      launch_alpha_quad(h->cfg.kernel, (const double*)h->alphaT, ld, k, Npad, N, (const double*)h->Xs.p, d, ard,
                        h->sf2, h->sn2, part2, ntheta, st, wv);
    launch_reduce_partials(part1, s1n, ntheta, 1.0, outv, st);
    launch_reduce_partials(part2, s2n, ntheta, 1.0, outv + ntheta, st);
    launch_dot_rhs((const double*)h->Y.p, (const double*)h->alphaT, ld, N, k, outv + 2 * ntheta, st);
    if (P > 1 && (rc = cm->allreduce(h, outv, (size_t)ntheta, COMM_SUM))) return rc;
  }
  double host[2 * (2 * MAX_D + 3) + 1];
  HIPCHK(h, hipMemcpyAsync(host, outv, (size_t)(2 * ntheta + 1) * 8, hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  const int nmain = paths ? h->n_ls + 2 : ntheta;
  for (int t = 0; t < nmain; ++t) grad[t] = 0.5 * (host[ntheta + t] - (double)k * host[t]);
  for (int t = nmain; t < ntheta; ++t) grad_path[t - nmain] = 0.5 * (host[ntheta + t] - (double)k * host[t]);
  if (kinds && h->sn2_deriv == 0.0) grad[ntheta - 1] = 0.0;  // (exactly: not -0, and no 0 x inf)
  *lml = -0.5 * host[2 * ntheta] - 0.5 * (double)k * h->logdet -
         0.5 * (double)N * (double)k * 1.8378770664093454835606594728112;  // log(2 pi)
  return GPX_OK;
}

// Leave-one-out predictions of the current fit (gpx_loo; one fp64 device): alpha, L^-T (the gradient's
// stage), one pass over its upper triangle for Q_ii (a fit with basis functions: Q'_ii), the finish kernel, the copies.
// `total` sums logp over the rows on the host, in row order.
int loo_impl(gpx_handle* h, double* mean, double* var, double* logp, double* total) {
  const int64_t N = h->N, ld = h->ld;
  const int k = h->k, p = h->bp;
  int rc;
  if ((rc = ensure_alpha<double>(h))) return rc;
  if ((rc = ensure(h, h->scr.LOO, (size_t)(2 * N + 2 * N * k) * 8))) return rc;
  double* dq = (double*)h->scr.LOO.p;
  double* dvar = dq + N;
  double* dmean = dvar + N;
  double* dlogp = dmean + N * k;
  if ((rc = build_zt(h))) return rc;
  hipStream_t st = h->st;
  launch_loo_rows((const double*)h->scr.ZT.p, ld, N, p ? (const double*)h->zT + (int64_t)k * ld : nullptr, p,
                  (const double*)h->Bst.p, dq, st);
  launch_loo_finish(dq, (const double*)h->alphaT, ld, (const double*)h->Y.p, N, k, dmean, dvar, dlogp, st);
  std::vector<double> lp;  // total without logp: the terms still come to the host
  if (total && !logp) {
    lp.resize((size_t)N * k);
    logp = lp.data();
  }
  if (mean) HIPCHK(h, hipMemcpyAsync(mean, dmean, (size_t)N * k * 8, hipMemcpyDeviceToHost, st));
  if (var) HIPCHK(h, hipMemcpyAsync(var, dvar, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  if (logp) HIPCHK(h, hipMemcpyAsync(logp, dlogp, (size_t)N * k * 8, hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  if (total)
    for (int c = 0; c < k; ++c) {
      double s = 0.0;
      for (int64_t i = 0; i < N; ++i) s += logp[i * k + c];
      total[c] = s;
    }
  return GPX_OK;
}

// ---- pathwise posterior function samples (gpx_pathwise_draw / _eval) -------------------------------------
// The draw: Omega and W from the stream, the prior draws at the training points by the evaluation kernel with its V term
// off (written straight into the rows that become V), the residual rows in place, and V = R K_y^-1 by the rows-layout
// solves against the fit's factor — one 64-row slab at a time, so that a column's bits do not depend on how many columns
// the draw has (the solves pick their tiles by the row count).  Built aside and moved into the handle at the end: a call
// that fails keeps the draw of the call before.
constexpr int64_t PW_ROWS = 8192;  // training points per launch of the draw's feature pass (bounds the partial buffer)

template <typename T>
int pathwise_draw_impl(gpx_handle* h, int64_t S, int64_t F, uint64_t seed, const void* z, int32_t mem_kind) {
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld;
  const int d = h->d, k = h->k, q = pathwise_chi_dof(h->cfg.kernel);
  const int64_t C = S * k, Cpad = round_up(C, RHS_ROWS), ldw = round_up(2 * F, 64) + ld_skew<T>();
  const int64_t nn = F * (d + q) + C * (2 * F + N);
  const int64_t MB = std::min(PW_ROWS, Npad);
  const int nz = pathwise_splits(Npad, F, false);
  gpx_handle::Pathwise fresh;
  int rc;
  if ((rc = ensure(h, fresh.Om, (size_t)F * d * sizeof(double)))) return rc;
  if ((rc = ensure(h, fresh.W, (size_t)Cpad * ldw * sizeof(T)))) return rc;
  if ((rc = ensure(h, fresh.V, (size_t)Cpad * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.PWpart, (size_t)nz * Cpad * MB * sizeof(T)))) return rc;
  const T* dz = (const T*)z;
  T* dV = (T*)fresh.V.p;
  {
    PhaseScope total(h, &tm.predict_total);
    {
      PhaseScope ps(h, &tm.kstar);  // the feature half of the draw
      if (z && mem_kind == GPX_MEM_HOST) {
        if ((rc = ensure(h, h->scr.PWZ, (size_t)nn * sizeof(T)))) return rc;
        if ((rc = copy_in(h, h->scr.PWZ.p, z, (size_t)nn * sizeof(T), GPX_MEM_HOST))) return rc;
        dz = (const T*)h->scr.PWZ.p;
      }
      launch_pathwise_draw<T>(dz, seed, F, d, q, C, Cpad, N, (double*)fresh.Om.p, (T*)fresh.W.p, ldw, h->st);
      for (int64_t m0 = 0; m0 < Npad; m0 += MB)
        launch_pathwise_eval<T>(h->cfg.kernel, (const T*)h->Xs.p + m0 * d, std::min(MB, Npad - m0), (const T*)h->Xs.p, Npad, d,
                                h->sf2, nullptr, 0, (const double*)fresh.Om.p, F, (const T*)fresh.W.p, ldw, Cpad,
                                (T*)h->scr.PWpart.p, dV + m0, ld, h->st);
      launch_pathwise_resid<T>((const T*)h->Y.p, dV, ld, h->weighted ? (const T*)h->Wfit.p : nullptr, h->sn2, dz, seed,
                               F * (d + q), F, N, Npad, k, C, Cpad, dV, ld, h->st);
    }
    {
      PhaseScope ps(h, &tm.trsm);
      for (int64_t r = 0; r < Cpad; r += RHS_ROWS) {
        if ((rc = solve_fwd_enqueue<T>(h, dV + r * ld, RHS_ROWS, (const T*)h->Lfac, ld, Npad, h->nb_solve, (const T*)h->Winv.p)))
          return rc;
        solve_bwd_enqueue<T>(h, dV + r * ld, RHS_ROWS, (const T*)h->Lfac, ld, Npad, h->nb_solve, (const T*)h->Winv.p);
      }
    }
  }
  if ((rc = finish_call(h))) return rc;
  fresh.S = S, fresh.F = F, fresh.ldw = ldw, fresh.n_normals = nn;
  h->pw = std::move(fresh);
  return GPX_OK;
}

// Samples [s0, s0 + S) of the stored draw at M query points, in batches of query rows (rows are independent and the
// kernel's splits do not depend on M: batching changes no bit).  Only the 64-column blocks the samples touch are evaluated.
template <typename T>
int pathwise_eval_impl(gpx_handle* h, const void* Xq, int64_t M, int64_t s0, int64_t S, void* out, int32_t mem_kind) {
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  const int64_t Npad = h->Npad, ld = h->ld, F = h->pw.F, ldw = h->pw.ldw;
  const int d = h->d, k = h->k;
  const int64_t cb0 = s0 * k / RHS_ROWS * RHS_ROWS, csel = round_up((s0 + S) * k, RHS_ROWS) - cb0;
  const int nz = pathwise_splits(Npad, F, true);
  const int64_t Mpad = round_up(M, TILE);
  const int64_t MB = pred_batch_rows(h, Mpad, (size_t)(nz + 1) * csel * sizeof(T), true);
  const bool host = mem_kind == GPX_MEM_HOST;
  const size_t outn = (size_t)S * M * k;
  int rc;
  if ((rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.PWpart, (size_t)nz * csel * MB * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.PWout, (size_t)csel * MB * sizeof(T)))) return rc;
  if (host && (rc = ensure(h, h->scr.PWres, outn * sizeof(T)))) return rc;
  T* dout = host ? (T*)h->scr.PWres.p : (T*)out;
  {
    PhaseScope total(h, &tm.predict_total);
    {
      PhaseScope ps(h, &tm.kstar);
      if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
    }
    {
      PhaseScope ps(h, &tm.mean);
      for (int64_t m0 = 0; m0 < Mpad; m0 += MB) {
        const int64_t mv = std::min<int64_t>(std::min(MB, Mpad - m0), M - m0);
        if (mv <= 0) break;
        launch_pathwise_eval<T>(h->cfg.kernel, (const T*)h->scr.Qs.p + m0 * d, round_up(mv, 64), (const T*)h->Xs.p, Npad, d,
                                h->sf2, (const T*)h->pw.V.p + cb0 * ld, ld, (const double*)h->pw.Om.p, F,
                                (const T*)h->pw.W.p + cb0 * ldw, ldw, csel, (T*)h->scr.PWpart.p, (T*)h->scr.PWout.p, MB, h->st);
        launch_pathwise_unpack<T>((const T*)h->scr.PWout.p, MB, cb0, s0, S, M, m0, mv, k, dout, h->st);
      }
    }
    if (host) {
      PhaseScope ps(h, &tm.d2h);
      if ((rc = copy_out(h, out, dout, outn * sizeof(T), mem_kind))) return rc;
    }
  }
  return finish_call(h);
}

// ---- GPX_MIXED: fp32 factorisation, fp64 refinement of alpha, fp64 mean --------------------------
constexpr int MIXED_KMAX = 8;
constexpr int MIXED_MAX_ITERS = 12;   // refine == 0: cap of the adaptive refinement
// relative residual at which the adaptive refinement stops.  At N = 65536 (C5) the largest elementwise
// relative error of the posterior mean is ~2000x the relative residual (means near zero count with a
// floor of 1e-6: profiles/r02_c5_mixed_precision_study.json), so north_star's 1e-6 needs <= 4e-10.
constexpr double MIXED_TOL = 1e-10;

void launch_rows_sumsq_y(gpx_handle* h, double* out) {  // ||y||^2: y (N x k) is one row of N k values
  launch_rows_sumsq((const double*)h->Y64.p, 0, 1, h->N * h->k, out, h->st);
}

int mixed_fit(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
              const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, int32_t mem_kind,
              int64_t* info) {
  if (k > MIXED_KMAX) return fail(h, GPX_E_ARG, "gpx_fit: the mixed-precision mode takes at most 8 target columns");
  int rc;
  if ((rc = ensure(h, h->X64, (size_t)N * d * 8))) return rc;
  if ((rc = ensure(h, h->Y64, (size_t)N * k * 8))) return rc;
  if ((rc = ensure(h, h->X32, (size_t)N * d * 4))) return rc;
  if ((rc = ensure(h, h->Y32, (size_t)N * k * 4))) return rc;
  if ((rc = ensure(h, h->ls, MAX_D * 8))) return rc;
  hipStream_t st = h->st;
  if ((rc = copy_in(h, h->X64.p, X, (size_t)N * d * 8, mem_kind))) return rc;
  if ((rc = copy_in(h, h->Y64.p, y, (size_t)N * k * 8, mem_kind))) return rc;
  launch_f64_to_f32((const double*)h->X64.p, (float*)h->X32.p, N * d, st);
  launch_f64_to_f32((const double*)h->Y64.p, (float*)h->Y32.p, N * k, st);
  // the whole fp32 fit (kernel build, blocked Cholesky, z = L^-1 y) on the device copies — on a shard (round 4) the
  // sharded fp32 fit: every rank holds the same fp64 inputs and runs the same refinement (replicated fp64 work)
  if (h->comm)
    rc = shard_fit<float>(h, h->X32.p, h->Y32.p, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, GPX_MEM_DEVICE, info);
  else
    rc = fit_impl<float>(h, h->X32.p, h->Y32.p, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, GPX_MEM_DEVICE, info);
  if (rc) return rc;
  gpx_timings& tm = h->tm;
  tm.refine = tm.refine_resid0 = tm.refine_resid = tm.refine_iters = 0;
  if (*info != 0) return GPX_OK;
  const int64_t Npad = h->Npad;  // the fp32 side's padding (a shard pads to its block height): the fp64 side follows it
  if ((rc = ensure(h, h->Xs64, (size_t)Npad * d * 8))) return rc;
  if ((rc = ensure(h, h->A64, (size_t)MIXED_KMAX * Npad * 8))) return rc;
  if ((rc = ensure(h, h->R64, (size_t)MIXED_KMAX * Npad * 8))) return rc;
  if ((rc = ensure(h, h->Aprev, (size_t)MIXED_KMAX * Npad * 8))) return rc;
  if ((rc = ensure(h, h->rn, 64))) return rc;
  const bool dist = h->comm && !h->repl;  // factor only held distributed: the refinement's solves are collective
  if (dist && (rc = ensure(h, h->RTloc, (size_t)RHS_ROWS * h->ldy * 4))) return rc;
  const int64_t ld32 = h->ld;
  if ((rc = ensure(h, h->RT32, (size_t)RHS_ROWS * ld32 * 4))) return rc;
  const bool few = !dist && few_solver_applies(h);
  if (!dist && (rc = ensure_alpha<float>(h))) return rc;  // (distributed: the fit left alpha^T replicated in YT)
  double* A64 = (double*)h->A64.p;
  double* R64 = (double*)h->R64.p;
  double* rn = (double*)h->rn.p;
  const double* Xs64 = (const double*)h->Xs64.p;
  const float* L32 = (const float*)h->Lfac;
  double hn[3] = {0, 0, 0};
  {
    PhaseScope ps(h, &tm.refine);
    launch_scale_points<double>((const double*)h->X64.p, N, Npad, d, (const double*)h->ls.p, n_ls, (double*)h->Xs64.p,
                                st);
    HIPCHK(h, hipMemsetAsync(A64, 0, (size_t)MIXED_KMAX * Npad * 8, st));
    launch_rows_add_f32_to_f64((const float*)h->alphaT, ld32, A64, Npad, k, N, Npad, 0, st);
    launch_rows_sumsq_y(h, rn + 2);  // ||y||^2
  }
  // refine == 0: iterate until the fp64 residual ||y - K alpha|| falls below MIXED_TOL ||y|| or stops
  // contracting (the fp32 factor is no preconditioner for this matrix), at most MIXED_MAX_ITERS
  // times — the residual norm is read back once per iteration (one 31 ms pass at N = 65536 each).
  // A fixed count runs without reading anything back until the end.
  const bool adaptive = h->refine <= 0;
  const int max_it = adaptive ? MIXED_MAX_ITERS : h->refine;
  double prev = 0, restored_res = -1.0;
  int iters = 0;
  for (int it = 0;; ++it) {
    PhaseScope ps(h, &tm.refine);
    // r = y - (K + diag I) alpha  (fp64, matrix-free; per-observation noise: diag(sn2 w_i + jitter))
    launch_kmatvec(h->cfg.kernel, Xs64, N, Npad, Xs64, Npad, d, sf2, sn2 + jitter, (const double*)h->Y64.p, A64,
                   Npad, k, -1.0, R64, Npad, st, h->weighted ? (const double*)h->Wfit64.p : nullptr, sn2, jitter);
    bool last = it == max_it;
    if (it == 0 || last || adaptive) launch_rows_sumsq(R64, Npad, k, N, rn + (it == 0 ? 0 : 1), st);
    if (adaptive) {
      HIPCHK(h, hipMemcpyAsync(hn, rn, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      const double res = hn[2] > 0 ? std::sqrt(hn[it == 0 ? 0 : 1] / hn[2]) : 0.0;
      if (it > 0 && !(res <= prev)) {
        // the last correction made the residual WORSE (or not finite): the fp32 factor is no contraction for this
        // matrix.  alpha goes back to the iterate before it, and that iterate's residual and count are what is reported.
        HIPCHK(h, hipMemcpyAsync(A64, h->Aprev.p, (size_t)MIXED_KMAX * Npad * 8, hipMemcpyDeviceToDevice, st));
        restored_res = prev;
        iters = it - 1;
        break;
      }
      if (res <= MIXED_TOL || (it > 0 && res > 0.5 * prev)) last = true;
      prev = res;
    }
    if (last) {
      if (it == 0) HIPCHK(h, hipMemcpyAsync(rn + 1, rn, 8, hipMemcpyDeviceToDevice, st));
      iters = it;
      break;
    }
    // delta = (L L^T)^-1 r in fp32; alpha += delta in fp64 (adaptive: the iterate before the correction is kept)
    if (adaptive) HIPCHK(h, hipMemcpyAsync(h->Aprev.p, A64, (size_t)MIXED_KMAX * Npad * 8, hipMemcpyDeviceToDevice, st));
    launch_rows_f64_to_f32(R64, Npad, (float*)h->RT32.p, ld32, k, RHS_ROWS, N, Npad, st);
    if (dist) {  // own column blocks of the residual rows -> the distributed solve -> delta replicated in RT32 again
      const int nb = h->nb_shard;
      const Shard sh{h->comm->world, h->comm->rank, nb, Npad / nb, h->shard_snake};
      float* Rl = (float*)h->RTloc.p;
      for (int64_t lb = 0; lb < sh.nlb(sh.r); ++lb)
        HIPCHK(h, hipMemcpy2DAsync(Rl + lb * nb, (size_t)h->ldy * 4, (const float*)h->RT32.p + sh.global(sh.r, lb) * nb,
                                   (size_t)ld32 * 4, (size_t)nb * 4, RHS_ROWS, hipMemcpyDeviceToDevice, st));
      if ((rc = shard_solve_dist<float>(h, sh, Rl, (float*)h->RT32.p))) return rc;
    } else if (few) {
      if ((rc = solve_few<float>(h, (float*)h->RT32.p, k, L32, ld32, Npad, (const float*)h->Wblk.p, h->nbw))) return rc;
    } else {
      if ((rc = solve_fwd_enqueue<float>(h, (float*)h->RT32.p, RHS_ROWS, L32, ld32, Npad, h->nb_solve,
                                         (const float*)h->Winv.p)))
        return rc;
      solve_bwd_enqueue<float>(h, (float*)h->RT32.p, RHS_ROWS, L32, ld32, Npad, h->nb_solve, (const float*)h->Winv.p);
    }
    launch_rows_add_f32_to_f64((const float*)h->RT32.p, ld32, A64, Npad, k, N, Npad, 1, st);
  }
  HIPCHK(h, hipMemcpyAsync(hn, rn, 24, hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  tm.fit_total += tm.refine;
  tm.refine_iters = iters;
  if (hn[2] > 0) {
    tm.refine_resid0 = std::sqrt(hn[0] / hn[2]);
    tm.refine_resid = restored_res >= 0 ? restored_res : std::sqrt(hn[1] / hn[2]);
  }
  return GPX_OK;
}

int mixed_predict(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) {
  const int64_t N = h->N, Npad = h->Npad;
  const int d = h->d, k = h->k;
  const int64_t Mpad = round_up(M, TILE);
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  int rc;
  if ((rc = ensure(h, h->scr.Q64, (size_t)M * d * 8))) return rc;
  if ((rc = ensure(h, h->scr.Qs64, (size_t)Mpad * d * 8))) return rc;
  if ((rc = ensure(h, h->scr.Q32, (size_t)M * d * 4))) return rc;
  if ((rc = ensure(h, h->scr.M64, (size_t)(MIXED_KMAX * Mpad + (size_t)M * k + Mpad) * 8))) return rc;
  double* MT64 = (double*)h->scr.M64.p;            // [8][Mpad] transposed means
  double* mout = MT64 + MIXED_KMAX * Mpad;     // (M x k)
  double* vout = mout + (size_t)M * k;         // (M)
  hipStream_t st = h->st;
  double shard_ms[6] = {0, 0, 0, 0, 0, 0};  // a sharded variance predict is a call of its own: its clocks are added below
  if (var && h->comm) {
    // Variance through the sharded fp32 factor (round 4): the whole sharded predict — collective, every rank — into
    // device scratch, before this call's own phases (it synchronises and folds its own clocks).  Its fp32 mean is not
    // used: the mean comes from the refined fp64 alpha below, replicated work on every rank.
    if ((rc = ensure(h, h->P32out, (size_t)M * (k + 1) * 4))) return rc;
    if ((rc = copy_in(h, h->scr.Q64.p, Xq, (size_t)M * d * 8, mem_kind))) return rc;
    launch_f64_to_f32((const double*)h->scr.Q64.p, (float*)h->scr.Q32.p, M * d, st);
    float* m32 = (float*)h->P32out.p;
    float* v32 = m32 + (size_t)M * k;
    const bool discard = h->discard_out;
    h->discard_out = false;  // the scratch outputs are wanted on every rank
    rc = shard_predict<float>(h, h->scr.Q32.p, M, m32, v32, GPX_MEM_DEVICE);
    h->discard_out = discard;
    if (rc) return rc;
    const double keep[6] = {tm.kstar, tm.trsm, tm.var, tm.mean, tm.predict_total, tm.comm};
    for (int i = 0; i < 6; ++i) shard_ms[i] = keep[i];
    reset_predict_clocks(tm);
    launch_f32_to_f64(v32, vout, M, st);
  }
  {
    PhaseScope total(h, &tm.predict_total);
    if ((rc = copy_in(h, h->scr.Q64.p, Xq, (size_t)M * d * 8, mem_kind))) return rc;
    if (var && !h->comm) {  // variance through the fp32 factor (its own K*, V^T = K* L^-T, row sums)
      launch_f64_to_f32((const double*)h->scr.Q64.p, (float*)h->scr.Q32.p, M * d, st);
      if ((rc = predict_core<float>(h, h->scr.Q32.p, M, true, GPX_MEM_DEVICE))) return rc;
      launch_f32_to_f64((const float*)h->var.p, vout, M, st);
    }
    {
      PhaseScope ps(h, &tm.mean);
      launch_scale_points<double>((const double*)h->scr.Q64.p, M, Mpad, d, (const double*)h->ls.p, h->n_ls,
                                  (double*)h->scr.Qs64.p, st);
      launch_kmatvec(h->cfg.kernel, (const double*)h->scr.Qs64.p, M, Mpad, (const double*)h->Xs64.p, Npad, d, h->sf2,
                     0.0, nullptr, (const double*)h->A64.p, Npad, k, 1.0, MT64, Mpad, st);
      launch_unpack_rhs<double>(MT64, Mpad, M, k, 1.0, mout, st);
    }
    PhaseScope ps(h, &tm.d2h);
    if (!h->discard_out) {  // a group's ranks > 0 hold the same result; rank 0 delivers it
      if ((rc = copy_out(h, mean, mout, (size_t)M * k * 8, mem_kind))) return rc;
      if (var && (rc = copy_out(h, var, vout, (size_t)M * 8, mem_kind))) return rc;
    }
  }
  if ((rc = finish_call(h))) return rc;
  tm.kstar += shard_ms[0];
  tm.trsm += shard_ms[1];
  tm.var += shard_ms[2];
  tm.predict_total += shard_ms[4];
  (void)N;
  return GPX_OK;
}

int mixed_alpha(gpx_handle* h, void* out) {
  int rc;
  if ((rc = ensure(h, h->scr.M64, (size_t)h->N * h->k * 8))) return rc;
  launch_unpack_rhs<double>((const double*)h->A64.p, h->Npad, h->N, h->k, 1.0, (double*)h->scr.M64.p, h->st);
  HIPCHK(h, hipMemcpyAsync(out, h->scr.M64.p, (size_t)h->N * h->k * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return GPX_OK;
}

template <typename T>
int alpha_impl(gpx_handle* h, void* out) {
  int rc;
  if ((!h->comm || h->repl) && (rc = ensure_alpha<T>(h))) return rc;  // the distributed shard solves alpha in fit
  if ((rc = ensure(h, h->meanout, (size_t)h->N * h->k * sizeof(T)))) return rc;
  launch_unpack_rhs<T>((const T*)h->alphaT, h->ld, h->N, h->k, 1.0, (T*)h->meanout.p, h->st);
  HIPCHK(h, hipMemcpyAsync(out, h->meanout.p, (size_t)h->N * h->k * sizeof(T), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return GPX_OK;
}

}  // namespace

gpx_handle::~gpx_handle() {
  for (hipStream_t s : {st, st2, st3, st4, st5})
    if (s) (void)hipStreamSynchronize(s);
  destroy_comm(this);
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
  for (hipStream_t s : {st, st2, st3, st4, st5})
    if (s) (void)hipStreamDestroy(s);
}

extern "C" {

int gpx_abi_version(void) { return GPX_ABI_VERSION; }

int gpx_device_count(int* count) try {
  if (!count) return GPX_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    *count = 0;
    return GPX_E_HIP;
  }
  *count = n;
  return GPX_OK;
}
GPX_CATCH_ALL

const char* gpx_last_error(gpx_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int gpx_create(gpx_handle** out, const gpx_config* cfg) try {
  if (!out || !cfg) return fail(nullptr, GPX_E_ARG, "gpx_create: null argument");
  *out = nullptr;
  if (!cov::known(cfg->kernel)) return fail(nullptr, GPX_E_ARG, "gpx_create: unknown kernel id");
  if (cfg->dtype != GPX_F64 && cfg->dtype != GPX_F32 && cfg->dtype != GPX_MIXED)
    return fail(nullptr, GPX_E_ARG, "gpx_create: unknown dtype id");
  if (cfg->refine < 0 || cfg->refine > 50) return fail(nullptr, GPX_E_ARG, "gpx_create: need 0 <= refine <= 50");
  if (cfg->world < 1 || cfg->world > 64 || cfg->rank < 0 || cfg->rank >= cfg->world)
    return fail(nullptr, GPX_E_ARG, "gpx_create: need 1 <= world <= 64 and 0 <= rank < world");
  if (cfg->ndev < 0 || cfg->ndev > GPX_MAX_GROUP)
    return fail(nullptr, GPX_E_ARG, "gpx_create: need 0 <= ndev <= GPX_MAX_GROUP");
  const int nb = cfg->block == 0 ? 1024 : cfg->block;
  if (nb < 128 || nb > 4096 || nb % 128 != 0)
    return fail(nullptr, GPX_E_ARG, "gpx_create: block must be a multiple of 128 in [128, 4096]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, GPX_E_HIP, "gpx_create: no HIP device visible (libgpx has no CPU fallback)");
  // ndev == 1 with an EXPLICIT transport is a one-rank group: the group code (rank threads' entry,
  // ncclCommInitAll / LocalComm, the sharded schedule) on one device — how a one-GPU box exercises
  // the RCCL device-group path at all; ndev == 1 with GPX_TRANSPORT_AUTO stays the plain handle
  if (cfg->ndev > 1 || (cfg->ndev == 1 && cfg->transport != GPX_TRANSPORT_AUTO)) {
    for (int i = 0; i < cfg->ndev; ++i)
      if (cfg->devices[i] < 0 || cfg->devices[i] >= ndev)
        return fail(nullptr, GPX_E_ARG, "gpx_create: group device ordinal out of range");
    return create_group(out, cfg);
  }
  const int device = cfg->ndev == 1 ? cfg->devices[0] : cfg->device;
  if (device < 0 || device >= ndev)
    return fail(nullptr, GPX_E_ARG, "gpx_create: device ordinal out of range");
  gpx_handle* h = new (std::nothrow) gpx_handle();
  if (!h) return fail(nullptr, GPX_E_NOMEM, "gpx_create: out of host memory");
  h->cfg = *cfg;
  h->cfg.device = device;
  h->nb = nb;
  h->refine = cfg->refine;  // 0: adaptive
  env_read(h->env, EnvAt::create);  // tuning overrides: GPX_NB_SHARD, GPX_NB_SOLVE, GPX_NB_PRED (gpx_env.h)
  h->nb_solve = h->env.nb_solve;
  if (h->env.nb_pred >= 0) h->nb_pred = h->env.nb_pred;
  int prio_lo = 0, prio_hi = 0;
  if (hipSetDevice(device) != hipSuccess ||
      hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
      hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&h->st2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(&h->st3, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithFlags(&h->st4, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(nullptr, GPX_E_HIP, "gpx_create: hipSetDevice/hipStreamCreate failed");
  }
  *out = h;
  return GPX_OK;
}
GPX_CATCH_ALL

void gpx_destroy(gpx_handle* h) {
  if (!h) return;
  if (h->group)
    destroy_group(h);
  else
    (void)hipSetDevice(h->cfg.device);
  delete h;
}

namespace {
// the argument checks of gpx_fit and gpx_fit_predict (with_queries: Xq, mean and M as well); `fn` heads the messages
int check_fit_args(gpx_handle* h, const char* fn, bool with_queries, bool any_null, int64_t N, int64_t M, int32_t d, int32_t k,
                   const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, int32_t mem_kind) {
  auto bad = [&](const char* what) { return fail(h, GPX_E_ARG, fn, what); };
  if (any_null) return bad("null argument");
  if (N <= 0 || d <= 0 || d > MAX_D || (with_queries && M <= 0))
    return bad(with_queries ? "need N, M > 0 and 1 <= d <= 32" : "need N > 0 and 1 <= d <= 32");
  if (k <= 0 || k > RHS_ROWS) return bad("need 1 <= k <= 64 target columns");
  if (n_ls != 1 && n_ls != d) return bad("n_ls must be 1 or d");
  if (bad_mem_kind(mem_kind)) return bad("bad mem_kind");
  if (!(sf2 > 0.0) || sn2 < 0.0 || jitter < 0.0) return bad("need sf2 > 0, sn2 >= 0, jitter >= 0");
  for (int i = 0; i < n_ls; ++i)
    if (!(lengthscale[i] > 0.0)) return bad("lengthscale must be > 0");
  if (N > (int64_t)INT_MAX - 4096) return bad("N too large");
  return GPX_OK;
}

// Per-observation noise weights (or query weights) must be finite and >= 0.  Host arrays are read here; device arrays by
// one small reduction kernel whose verdict (a word of h->scalars) is the only thing copied back.  es = element size (4 / 8).  `stream` null (the
// front handle of a device group owns none): the device array is read back and checked on the host.
int check_weights(gpx_handle* h, const char* fn, const void* w, int64_t n, int32_t mem_kind, size_t es, hipStream_t stream) {
  auto bad = [&]() { return fail(h, GPX_E_ARG, (std::string(fn) + ": weights must be finite and >= 0").c_str()); };
  auto host_ok = [&](const void* p) {
    for (int64_t i = 0; i < n; ++i) {
      const double v = es == 4 ? (double)((const float*)p)[i] : ((const double*)p)[i];
      if (!(v >= 0.0) || !std::isfinite(v)) return false;
    }
    return true;
  };
  if (mem_kind == GPX_MEM_HOST) return host_ok(w) ? GPX_OK : bad();
  if (!stream) {
    std::vector<char> tmp((size_t)n * es);
    HIPCHK(h, hipMemcpy(tmp.data(), w, tmp.size(), hipMemcpyDefault));
    return host_ok(tmp.data()) ? GPX_OK : bad();
  }
  int rc, hbad = 0;
  if ((rc = ensure(h, h->scalars, 64))) return rc;  // the fit's own 64 bytes ([0, 16): logdet, info): the verdict at byte 32
  int* flag = (int*)((char*)h->scalars.p + 32);
  if (es == 4)
    launch_check_weights<float>((const float*)w, n, flag, stream);
  else
    launch_check_weights<double>((const double*)w, n, flag, stream);
  HIPCHK(h, hipMemcpyAsync(&hbad, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCHK(h, hipStreamSynchronize(stream));
  HIPCHK(h, hipGetLastError());
  return hbad ? bad() : GPX_OK;
}

// a fit on a handle with weights set: refused on device groups, shards and handles that own a communicator, and when the
// weights are not one per observation — before anything is computed or exchanged
int check_fit_weights(gpx_handle* h, const char* fn, int64_t N) {
  if (h->nw_set == 0) return GPX_OK;
  char buf[256];
  if (h->group || h->cfg.world > 1 || h->comm) {
    snprintf(buf, sizeof buf, "%s: per-observation noise weights are not supported on %s (single-device handles only; "
             "clear them with gpx_set_noise_weights(h, NULL, 0, ...))", fn, h->group ? "device groups" : "sharded handles");
    return fail(h, GPX_E_UNSUPPORTED, buf);
  }
  if (N != h->nw_set) {
    snprintf(buf, sizeof buf, "%s: %lld noise weights are set for a fit of %lld observations", fn, (long long)h->nw_set,
             (long long)N);
    return fail(h, GPX_E_ARG, buf);
  }
  return GPX_OK;
}

// a fit on a handle with observation kinds set, before anything is computed or exchanged: GPX_E_ARG for kinds that do not
// fit the call (not one per observation, a dimension >= d), GPX_E_UNSUPPORTED where no KINDS builder runs
int check_fit_kinds(gpx_handle* h, const char* fn, int64_t N, int32_t d) {
  if (h->kinds_set.empty()) return GPX_OK;
  char buf[320];
  const char* where = h->group ? "device groups" : (h->cfg.world > 1 || h->comm) ? "sharded handles"
                      : h->cfg.dtype == GPX_MIXED ? "GPX_MIXED handles" : nullptr;
  if (where) {
    snprintf(buf, sizeof buf, "%s: observation kinds are not supported on %s (single-device GPX_F64 / GPX_F32 handles "
             "only; clear them with gpx_set_observation_kinds(h, NULL, 0, ...))", fn, where);
    return fail(h, GPX_E_UNSUPPORTED, buf);
  }
  if (N != (int64_t)h->kinds_set.size()) {
    snprintf(buf, sizeof buf, "%s: %lld observation kinds are set for a fit of %lld observations", fn,
             (long long)h->kinds_set.size(), (long long)N);
    return fail(h, GPX_E_ARG, buf);
  }
  bool deriv = false;
  for (int64_t i = 0; i < N; ++i) {
    if (h->kinds_set[i] >= d) {
      snprintf(buf, sizeof buf, "%s: observation %lld has kind %d, the inputs have %d dimensions", fn, (long long)i,
               (int)h->kinds_set[i], (int)d);
      return fail(h, GPX_E_ARG, buf);
    }
    deriv |= h->kinds_set[i] >= 0;
  }
  if (deriv && !cov::differentiable(h->cfg.kernel)) {
    snprintf(buf, sizeof buf, "%s: derivative observations: " MATERN12_NO_GRAD, fn);
    return fail(h, GPX_E_UNSUPPORTED, buf);
  }
  return GPX_OK;
}

// a fit on a handle with path ids set, before anything is computed or exchanged: GPX_E_ARG for ids or lengthscales that do
// not fit the call, GPX_E_UNSUPPORTED where no GROUPS builder runs (only when the ids take effect: groups_effective)
int check_fit_groups(gpx_handle* h, const char* fn, int64_t N, int32_t d) {
  if (h->groups_set.empty()) return GPX_OK;
  char buf[320];
  if (N != (int64_t)h->groups_set.size()) {
    snprintf(buf, sizeof buf, "%s: %lld path ids are set for a fit of %lld observations", fn,
             (long long)h->groups_set.size(), (long long)N);
    return fail(h, GPX_E_ARG, buf);
  }
  if (h->lsp_set.size() != 1 && (int64_t)h->lsp_set.size() != d) {
    snprintf(buf, sizeof buf, "%s: %d path lengthscales are set, the inputs have %d dimensions (need 1 or d)", fn,
             (int)h->lsp_set.size(), (int)d);
    return fail(h, GPX_E_ARG, buf);
  }
  if (!groups_effective(h)) return GPX_OK;
  const char* where = h->group ? "device groups" : (h->cfg.world > 1 || h->comm) ? "sharded handles"
                      : h->cfg.dtype == GPX_MIXED ? "GPX_MIXED handles"
                      : !h->kinds_set.empty() ? "handles that also have observation kinds set" : nullptr;
  if (where) {
    snprintf(buf, sizeof buf, "%s: path ids are not supported on %s (no builder of the within-path covariance runs there; "
             "single-device GPX_F64 / GPX_F32 handles only; clear them with gpx_set_path_groups(h, NULL, 0, ...))", fn, where);
    return fail(h, GPX_E_UNSUPPORTED, buf);
  }
  return GPX_OK;
}

// a fit on a handle with a basis set (gpx_set_basis), before anything is computed or exchanged and with the previous fit
// still valid: GPX_E_UNSUPPORTED where the basis steps do not run, GPX_E_ARG for a basis that does not fit the call
int check_fit_basis(gpx_handle* h, const char* fn, int64_t N, int32_t d, int32_t k) {
  if (!h->basis_set) return GPX_OK;
  char buf[320];
  const char* where = h->group ? "device groups" : (h->cfg.world > 1 || h->comm) ? "sharded handles"
                      : h->cfg.dtype == GPX_MIXED ? "GPX_MIXED handles"
                      : !h->kinds_set.empty() ? "handles that also have observation kinds set"
                      : groups_effective(h) ? "handles that also have path ids set" : nullptr;
  if (where) {
    snprintf(buf, sizeof buf, "%s: basis functions are not supported on %s (single-device GPX_F64 / GPX_F32 handles with "
             "plain or weighted observations only; clear the basis with gpx_set_basis(h, GPX_BASIS_NONE))", fn, where);
    return fail(h, GPX_E_UNSUPPORTED, buf);
  }
  const int p = basis_count(h->basis_set, d);
  if (k + p > RHS_ROWS) {
    snprintf(buf, sizeof buf, "%s: k = %d target columns and p = %d basis functions need k + p <= 64 bordered rows", fn, (int)k,
             p);
    return fail(h, GPX_E_ARG, buf);
  }
  if (N < p) {
    snprintf(buf, sizeof buf, "%s: %lld observations cannot determine p = %d basis coefficients (need N >= p)", fn,
             (long long)N, p);
    return fail(h, GPX_E_ARG, buf);
  }
  return GPX_OK;
}

// what a fit with basis functions refuses (`what`: the call's own reason), before anything is computed
int basis_refused(gpx_handle* h, const char* fn, const char* what) {
  if (!h->fitted || !h->bp) return GPX_OK;
  char buf[320];
  snprintf(buf, sizeof buf, "%s: the fit has basis functions (gpx_set_basis): %s", fn, what);
  return fail(h, GPX_E_UNSUPPORTED, buf);
}
#define BASIS_NO_UPDATE "beta and the projected right-hand sides are not updated in place: fit the changed data instead"

// gpx_fit on one handle, behind its argument checks and begin_fit
int fit_begun(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k, const double* lengthscale,
              int32_t n_ls, double sf2, double sn2, double jitter, int32_t mem_kind, int64_t* info) {
  h->grouped = false;  // (fit_impl decides; the other engines never build with path ids: check_fit_groups)
  if (h->cfg.dtype == GPX_MIXED) return mixed_fit(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
  if (h->cfg.world > 1 || h->comm) {  // a 1-rank communicator also takes the sharded schedule
    h->weighted = false;
    return BY_DTYPE(h, shard_fit, h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
  }
  return BY_DTYPE(h, fit_impl, h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
}

// gpx_fit_predict on a handle with a communicator: do the query rows ride through the sharded factorisation, as bordered
// rows of every rank's local row set?  In the split schedule only (GPX_SPLIT_STRIP), up to 8192 rows per rank, unless
// GPX_SHARD_FUSED=0.  Decided here, once per call, from the call's snapshot; shard_fit relies on it (query rows that reach
// it outside the split schedule are GPX_E_UNSUPPORTED).
bool queries_ride_through_shard(const gpx_handle* h, int64_t M) {
  if (!h->comm || h->cfg.dtype == GPX_MIXED || !h->env.split_strip || !h->env.shard_fused) return false;
  const int P = h->comm->world;
  return round_up((M + P - 1) / P, TILE) <= 8192;
}
}  // namespace

int gpx_fit(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
            const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
            int32_t mem_kind, int64_t* info) try {
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = check_fit_args(h, "gpx_fit", false, !X || !y || !lengthscale || !info, N, 0, d, k, lengthscale, n_ls, sf2, sn2,
                           jitter, mem_kind)))
    return rc;
  if ((rc = check_fit_weights(h, "gpx_fit", N))) return rc;
  if ((rc = check_fit_kinds(h, "gpx_fit", N, d))) return rc;
  if ((rc = check_fit_groups(h, "gpx_fit", N, d))) return rc;
  if ((rc = check_fit_basis(h, "gpx_fit", N, d, k))) return rc;
  if (h->group) return group_fit(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
  if ((rc = begin_fit(h))) return rc;
  return fit_begun(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
}
GPX_CATCH_ALL

int gpx_fit_predict(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
                    const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, const void* Xq,
                    int64_t M, void* mean, void* var, int32_t mem_kind, int64_t* info) try {
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = check_fit_args(h, "gpx_fit_predict", true, !X || !y || !lengthscale || !info || !Xq || !mean, N, M, d, k,
                           lengthscale, n_ls, sf2, sn2, jitter, mem_kind)))
    return rc;
  if ((rc = check_fit_weights(h, "gpx_fit_predict", N))) return rc;
  if ((rc = check_fit_kinds(h, "gpx_fit_predict", N, d))) return rc;
  if ((rc = check_fit_groups(h, "gpx_fit_predict", N, d))) return rc;
  if ((rc = check_fit_basis(h, "gpx_fit_predict", N, d, k))) return rc;
  if (h->group) return group_fit_predict(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, Xq, M, mean, var, mem_kind, info);
  // Shards (round 4): every rank's slice of the query points rides through the sharded factorisation as bordered rows of
  // its local row set (shard_fit with query points + shard_fused_tail) — in the split schedule, up to 8192 rows per rank.
  // Otherwise, and in the mixed mode (its refinement needs the factor first), the call IS the two calls (same results;
  // ABI v5 — it was GPX_E_UNSUPPORTED).  *info > 0: not positive definite, nothing predicted.
  if ((rc = begin_fit(h))) return rc;  // (the call's snapshot of the environment: what is decided below reads it)
  if (h->cfg.world > 1 || h->comm || h->cfg.dtype == GPX_MIXED) {
    if (!queries_ride_through_shard(h, M)) {
      rc = fit_begun(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info);
      if (rc != GPX_OK || *info != 0) return rc;
      return gpx_predict(h, Xq, M, mean, var, mem_kind);
    }
    h->grouped = false;
    rc = BY_DTYPE(h, shard_fit, h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info, false, Xq, M);
    if (rc != GPX_OK || !h->fitted) return rc;
    return BY_DTYPE(h, shard_fused_tail, h, M, mean, var, mem_kind);
  }
  // one batch of query points rides through the factorisation; more than that (ABI v5: it was GPX_E_UNSUPPORTED): the
  // first batch rides, the others go through the ordinary predict against the factor the pass leaves behind — query
  // rows are independent, so the split changes no bit of either part
  const int64_t Mb = std::min<int64_t>(M, pred_batch_rows(h, round_up(M, TILE), 0, false));
  const size_t es = h->cfg.dtype == GPX_F32 ? sizeof(float) : sizeof(double);
  rc = BY_DTYPE(h, fit_impl, h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info, Xq, Mb);
  if (rc != GPX_OK || !h->fitted) return rc;  // *info > 0: not positive definite, nothing predicted
  rc = BY_DTYPE(h, fused_predict_tail, h, Mb, mean, var, mem_kind);
  if (rc != GPX_OK || Mb == M) return rc;
  const gpx_timings first = h->tm;  // the rest through predict; its clocks are added to the pass's
  const void* Xr = (const char*)Xq + (size_t)Mb * d * es;
  void* mr = (char*)mean + (size_t)Mb * k * es;
  void* vr = var ? (char*)var + (size_t)Mb * es : nullptr;
  rc = BY_DTYPE(h, predict_impl, h, Xr, M - Mb, mr, vr, mem_kind);
  h->tm.kstar += first.kstar;
  h->tm.mean += first.mean;
  h->tm.trsm += first.trsm;
  h->tm.var += first.var;
  h->tm.d2h += first.d2h;
  h->tm.predict_total += first.predict_total;
  return rc;
}
GPX_CATCH_ALL

namespace {
// the joint-posterior calls run on single-device fp64 / fp32 handles; anything else is refused before any work
int posterior_refused(gpx_handle* h, const char* fn) {
  char buf[256];
  const char* why = h->group                                  ? "device groups"
                    : (h->cfg.world > 1 || h->comm)           ? "sharded handles"
                    : h->cfg.dtype == GPX_MIXED               ? "GPX_MIXED handles"
                                                              : nullptr;
  if (!why) return GPX_OK;
  snprintf(buf, sizeof buf, "%s: not supported on %s (single-device GPX_F64 / GPX_F32 handles only)", fn, why);
  return fail(h, GPX_E_UNSUPPORTED, buf);
}

// What the *_paths calls refuse beyond their plain twins' argument checks, before anything is computed: handles the
// joint-posterior calls refuse, a fit without effective path ids, a null gq or an id below -1 (ids on the device are read
// back for the check).
int query_ids_refused(gpx_handle* h, const char* fn, const int32_t* gq, int64_t M, int32_t mem_kind) {
  if (!gq) return fail(h, GPX_E_ARG, fn, "bad argument");
  if (int rc = posterior_refused(h, fn)) return rc;
  if (int rc = basis_refused(h, fn, "a basis together with path ids is not supported")) return rc;
  if (!h->grouped)
    return fail(h, GPX_E_UNSUPPORTED, fn,
                "the current fit has no path ids (gpx_set_path_groups with an id >= 0 and sg2 > 0 before the fit)");
  std::vector<int32_t> ids;
  if (int rc = fetch_ids(h, gq, M, mem_kind, ids)) return rc;
  const int64_t i = first_below_minus_one(ids.data(), M);
  if (i == M) return GPX_OK;
  char buf[256];
  snprintf(buf, sizeof buf, "%s: path id %d of query point %lld is below -1", fn, (int)ids[i], (long long)i);
  return fail(h, GPX_E_ARG, buf);
}
}  // namespace

// ---- the four posterior calls and their *_paths twins (the path itself, f + g_p: a path id per query point; DESIGN.md
// §3.4k): one body per call.  `fn`, the exported name, heads every message; `paths`: the call takes gq, and query_ids_refused
// stands in for posterior_refused.
extern "C++" {
namespace {
// What the three joint-posterior families refuse, in their common order, then begin_call: the family's argument test, the
// mem_kind, its value test (bad_values: the message, or null), a handle without a fit, its size limit (too_large: the
// message, or null), a kernel without the derivatives of `order` (1: gradient, 2: second derivatives, which also stop at
// MAX_HESS_D dimensions), the handle's kind or — paths — the ids.
int posterior_begin(gpx_handle* h, const char* fn, bool paths, const int32_t* gq, int64_t M, int32_t mem_kind, bool bad_args,
                    const char* bad_values, const char* too_large, int order = 0) {
  if (!h) return GPX_E_ARG;
  if (bad_args) return fail(h, GPX_E_ARG, fn, "bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, fn, "bad mem_kind");
  if (bad_values) return fail(h, GPX_E_ARG, fn, bad_values);
  if (!h->fitted) return fail(h, GPX_E_ARG, fn, "handle has no successful fit");
  if (too_large) return fail(h, GPX_E_ARG, fn, too_large);
  if (order == 2 && !cov::twice_differentiable(h->cfg.kernel)) return fail(h, GPX_E_UNSUPPORTED, fn, NOT_TWICE_DIFFERENTIABLE);
  if (order && !cov::differentiable(h->cfg.kernel)) return fail(h, GPX_E_UNSUPPORTED, fn, MATERN12_NO_GRAD);
  if (order == 2 && h->d > MAX_HESS_D) return fail(h, GPX_E_UNSUPPORTED, fn, HESS_D_LIMIT);
  if (order)
    if (int rc = basis_refused(h, fn, order == 2 ? "the posterior second derivatives do not include the basis terms yet"
                                                 : "the posterior gradient does not include the basis terms yet"))
      return rc;
  const int rc = paths ? query_ids_refused(h, fn, gq, M, mem_kind) : posterior_refused(h, fn);
  return rc ? rc : begin_call(h);
}

// (gpx_predict alone tests the fit before the arguments, serves groups, shards and GPX_MIXED handles, and has no limit on M)
int predict_entry(gpx_handle* h, const char* fn, bool paths, const void* Xq, const int32_t* gq, int64_t M, void* mean,
                  void* var, int32_t mem_kind) {
  if (!h) return GPX_E_ARG;
  if (!h->fitted) return fail(h, GPX_E_ARG, fn, "handle has no successful fit");
  if (!Xq || !mean || M <= 0) return fail(h, GPX_E_ARG, fn, "bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, fn, "bad mem_kind");
  int rc;
  if (paths) {
    if (M > (int64_t)INT_MAX - 4096) return fail(h, GPX_E_ARG, fn, "M too large");
    if ((rc = query_ids_refused(h, fn, gq, M, mem_kind)) || (rc = begin_call(h))) return rc;
    return BY_DTYPE(h, predict_impl, h, Xq, M, mean, var, mem_kind, gq);
  }
  if (h->group) return group_predict(h, Xq, M, mean, var, mem_kind);
  if ((rc = begin_call(h))) return rc;
  if (h->cfg.dtype == GPX_MIXED) return mixed_predict(h, Xq, M, mean, var, mem_kind);
  if (h->cfg.world > 1 || h->comm) return BY_DTYPE(h, shard_predict, h, Xq, M, mean, var, mem_kind);
  return BY_DTYPE(h, predict_impl, h, Xq, M, mean, var, mem_kind);
}

int predict_cov_entry(gpx_handle* h, const char* fn, bool paths, const void* Xq, const int32_t* gq, int64_t M, void* mean,
                      void* cov, int32_t mem_kind) {
  const int rc = posterior_begin(h, fn, paths, gq, M, mem_kind, !Xq || !cov || M <= 0, nullptr,
                                 M > (int64_t)INT_MAX - 4096 ? "M too large" : nullptr);
  return rc ? rc : BY_DTYPE(h, predict_cov_impl, h, Xq, M, mean, cov, mem_kind, gq);
}

int sample_posterior_entry(gpx_handle* h, const char* fn, bool paths, const void* Xq, const int32_t* gq, int64_t M, int64_t S,
                           uint64_t seed, const void* z, double diag_add, double jitter, int32_t max_tries, void* out,
                           double* jitter_used, int64_t* info, int32_t mem_kind) {
  const bool values_ok = diag_add >= 0.0 && jitter >= 0.0 && max_tries >= 1;
  const int rc = posterior_begin(h, fn, paths, gq, M, mem_kind, !Xq || !out || !info || !jitter_used || M <= 0 || S <= 0,
                                 values_ok ? nullptr : "need diag_add >= 0, jitter >= 0, max_tries >= 1",
                                 M > (int64_t)INT_MAX - 4096 || S > (int64_t)1 << 40 ? "M or S too large" : nullptr);
  if (rc) return rc;
  return BY_DTYPE(h, sample_posterior_impl, h, Xq, M, S, seed, z, diag_add, jitter, max_tries, out, jitter_used, info,
                  mem_kind, gq);
}

int predict_grad_entry(gpx_handle* h, const char* fn, bool paths, const void* Xq, const int32_t* gq, int64_t M, void* mean,
                       void* var, void* dmean, void* dvar, int32_t mem_kind) {
  const int rc = posterior_begin(h, fn, paths, gq, M, mem_kind, !Xq || !dmean || M <= 0, nullptr,
                                 M > (int64_t)INT_MAX - 4096 ? "M too large" : nullptr, 1);
  return rc ? rc : BY_DTYPE(h, predict_grad_impl, h, Xq, M, mean, var, dmean, dvar, mem_kind, gq, fn, 1);
}

// gpx_predict_hess and its twin: the gradient's stages on the d (d + 1) / 2 second derivatives, no value rows
int predict_hess_entry(gpx_handle* h, const char* fn, bool paths, const void* Xq, const int32_t* gq, int64_t M, void* hmean,
                       void* hvar, int32_t mem_kind) {
  const int rc = posterior_begin(h, fn, paths, gq, M, mem_kind, !Xq || !hmean || M <= 0, nullptr,
                                 M > ((int64_t)INT_MAX - 4096) / hess_pairs(MAX_HESS_D) ? "M too large" : nullptr, 2);
  return rc ? rc : BY_DTYPE(h, predict_grad_impl, h, Xq, M, nullptr, nullptr, hmean, hvar, mem_kind, gq, fn, 2);
}
}  // namespace
}  // extern "C++"

int gpx_predict(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) try {
  return predict_entry(h, "gpx_predict", false, Xq, nullptr, M, mean, var, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_paths(gpx_handle* h, const void* Xq, const int32_t* gq, int64_t M, void* mean, void* var,
                      int32_t mem_kind) try {
  return predict_entry(h, "gpx_predict_paths", true, Xq, gq, M, mean, var, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_cov(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* cov, int32_t mem_kind) try {
  return predict_cov_entry(h, "gpx_predict_cov", false, Xq, nullptr, M, mean, cov, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_cov_paths(gpx_handle* h, const void* Xq, const int32_t* gq, int64_t M, void* mean, void* cov,
                          int32_t mem_kind) try {
  return predict_cov_entry(h, "gpx_predict_cov_paths", true, Xq, gq, M, mean, cov, mem_kind);
}
GPX_CATCH_ALL

int gpx_sample_posterior(gpx_handle* h, const void* Xq, int64_t M, int64_t S, uint64_t seed, const void* z,
                         double diag_add, double jitter, int32_t max_tries, void* out, double* jitter_used, int64_t* info,
                         int32_t mem_kind) try {
  return sample_posterior_entry(h, "gpx_sample_posterior", false, Xq, nullptr, M, S, seed, z, diag_add, jitter, max_tries, out,
                                jitter_used, info, mem_kind);
}
GPX_CATCH_ALL

int gpx_sample_posterior_paths(gpx_handle* h, const void* Xq, const int32_t* gq, int64_t M, int64_t S, uint64_t seed,
                               const void* z, double diag_add, double jitter, int32_t max_tries, void* out,
                               double* jitter_used, int64_t* info, int32_t mem_kind) try {
  return sample_posterior_entry(h, "gpx_sample_posterior_paths", true, Xq, gq, M, S, seed, z, diag_add, jitter, max_tries,
                                out, jitter_used, info, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_grad(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, void* dmean, void* dvar,
                     int32_t mem_kind) try {
  return predict_grad_entry(h, "gpx_predict_grad", false, Xq, nullptr, M, mean, var, dmean, dvar, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_grad_paths(gpx_handle* h, const void* Xq, const int32_t* gq, int64_t M, void* mean, void* var, void* dmean,
                           void* dvar, int32_t mem_kind) try {
  return predict_grad_entry(h, "gpx_predict_grad_paths", true, Xq, gq, M, mean, var, dmean, dvar, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_hess(gpx_handle* h, const void* Xq, int64_t M, void* hmean, void* hvar, int32_t mem_kind) try {
  return predict_hess_entry(h, "gpx_predict_hess", false, Xq, nullptr, M, hmean, hvar, mem_kind);
}
GPX_CATCH_ALL

int gpx_predict_hess_paths(gpx_handle* h, const void* Xq, const int32_t* gq, int64_t M, void* hmean, void* hvar,
                           int32_t mem_kind) try {
  return predict_hess_entry(h, "gpx_predict_hess_paths", true, Xq, gq, M, hmean, hvar, mem_kind);
}
GPX_CATCH_ALL

namespace {
// gpx_score_blocks (wq null) and gpx_score_blocks_weighted: one body, so the refusals are the same
int score_blocks_entry(gpx_handle* h, const void* Xs, const void* ys, const void* wq, int64_t G, int32_t Lg, double diag_add,
                       void* logp, void* maha, void* logdet, int32_t mem_kind, int64_t* info) {
  if (!h) return GPX_E_ARG;
  if (!Xs || !ys || !logp || !info || G <= 0) return fail(h, GPX_E_ARG, "gpx_score_blocks: bad argument");
  if (Lg < 1 || Lg > 64) return fail(h, GPX_E_ARG, "gpx_score_blocks: need 1 <= Lg <= 64");
  if (!(diag_add >= 0.0)) return fail(h, GPX_E_ARG, "gpx_score_blocks: need diag_add >= 0");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_score_blocks: bad mem_kind");
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_score_blocks: handle has no successful fit");
  if (G > ((int64_t)INT_MAX - 4096) / Lg) return fail(h, GPX_E_ARG, "gpx_score_blocks: G * Lg too large");
  int rc;
  if ((rc = posterior_refused(h, "gpx_score_blocks"))) return rc;
  if ((rc = begin_call(h))) return rc;
  if (wq && (rc = check_weights(h, "gpx_score_blocks_weighted", wq, G * Lg, mem_kind, h->cfg.dtype == GPX_F32 ? 4 : 8, h->st)))
    return rc;
  return BY_DTYPE(h, score_impl, h, Xs, ys, wq, G, Lg, diag_add, logp, maha, logdet, mem_kind, info);
}

int append_entry(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, int64_t m, int32_t mem_kind,
                 int64_t* info) {
  if (!h) return GPX_E_ARG;
  if (!Xnew || !ynew || !info || m <= 0) return fail(h, GPX_E_ARG, "gpx_append: bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_append: bad mem_kind");
  int rc;
  if ((rc = posterior_refused(h, "gpx_append"))) return rc;
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_append: handle has no successful fit");
  if ((rc = basis_refused(h, "gpx_append", BASIS_NO_UPDATE))) return rc;
  if (m > (int64_t)INT_MAX - 4096 - h->N) return fail(h, GPX_E_ARG, "gpx_append: N + m too large");
  if (h->has_deriv)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_append: the fit has derivative observations (gpx_set_observation_kinds): fit the "
                                      "concatenated data instead");
  if (h->grouped)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_append: the fit has path ids (gpx_set_path_groups) and the appended rows would be "
                                      "built without the within-path covariance: fit the concatenated data instead");
  h->kinded = false;  // (kinds all -1: the plain model, and from here on the plain builders' — the same numbers)
  if ((rc = begin_call(h))) return rc;
  h->pw = {};  // the factor changes: a stored pathwise draw goes
  if (wnew && (rc = check_weights(h, "gpx_append_weighted", wnew, m, mem_kind, h->cfg.dtype == GPX_F32 ? 4 : 8, h->st)))
    return rc;
  return BY_DTYPE(h, append_impl, h, Xnew, ynew, wnew, m, mem_kind, info);
}
}  // namespace

int gpx_score_blocks(gpx_handle* h, const void* Xs, const void* ys, int64_t G, int32_t Lg, double diag_add, void* logp,
                     void* maha, void* logdet, int32_t mem_kind, int64_t* info) try {
  return score_blocks_entry(h, Xs, ys, nullptr, G, Lg, diag_add, logp, maha, logdet, mem_kind, info);
}
GPX_CATCH_ALL

int gpx_score_blocks_weighted(gpx_handle* h, const void* Xs, const void* ys, const void* wq, int64_t G, int32_t Lg,
                              double diag_add, void* logp, void* maha, void* logdet, int32_t mem_kind, int64_t* info) try {
  return score_blocks_entry(h, Xs, ys, wq, G, Lg, diag_add, logp, maha, logdet, mem_kind, info);
}
GPX_CATCH_ALL

int gpx_append(gpx_handle* h, const void* Xnew, const void* ynew, int64_t m, int32_t mem_kind, int64_t* info) try {
  return append_entry(h, Xnew, ynew, nullptr, m, mem_kind, info);
}
GPX_CATCH_ALL

int gpx_append_weighted(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, int64_t m, int32_t mem_kind,
                        int64_t* info) try {
  return append_entry(h, Xnew, ynew, wnew, m, mem_kind, info);
}
GPX_CATCH_ALL

int gpx_remove_rows(gpx_handle* h, int64_t start, int64_t count, int64_t* info) try {
  if (!h) return GPX_E_ARG;
  if (!info) return fail(h, GPX_E_ARG, "gpx_remove_rows: bad argument");
  int rc;
  if ((rc = posterior_refused(h, "gpx_remove_rows"))) return rc;
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_remove_rows: handle has no successful fit");
  if ((rc = basis_refused(h, "gpx_remove_rows", BASIS_NO_UPDATE))) return rc;
  if (start < 0 || count < 0 || start > h->N || count > h->N - start)
    return fail(h, GPX_E_ARG, "gpx_remove_rows: rows [start, start + count) must lie inside the fit");
  if (count >= h->N) return fail(h, GPX_E_ARG, "gpx_remove_rows: a fit keeps at least one point");
  *info = 0;
  if (count == 0) return GPX_OK;
  if ((rc = begin_call(h))) return rc;
  h->pw = {};  // the factor changes: a stored pathwise draw goes
  return BY_DTYPE(h, remove_impl, h, start, count, info);
}
GPX_CATCH_ALL

int gpx_append_rows(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, const int32_t* kind_new,
                    const int32_t* group_new, int64_t m, int32_t mem_kind, int64_t* info) try {
  if (!h) return GPX_E_ARG;
  if (!Xnew || !ynew || !info || m <= 0) return fail(h, GPX_E_ARG, "gpx_append_rows: bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_append_rows: bad mem_kind");
  int rc;
  if ((rc = posterior_refused(h, "gpx_append_rows"))) return rc;
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_append_rows: handle has no successful fit");
  if ((rc = basis_refused(h, "gpx_append_rows", BASIS_NO_UPDATE))) return rc;
  if (m > (int64_t)INT_MAX - 4096 - h->N) return fail(h, GPX_E_ARG, "gpx_append_rows: N + m too large");
  // the kinds and the ids are checked in host copies (NULL: all -1), which also feed the fit's host vectors afterwards
  std::vector<int32_t> kinds((size_t)m, -1), ids((size_t)m, -1);
  if ((kind_new && (rc = fetch_ids(h, kind_new, m, mem_kind, kinds))) ||
      (group_new && (rc = fetch_ids(h, group_new, m, mem_kind, ids))))
    return rc;
  bool deriv = false, path = false;
  for (int64_t i = 0; i < m; ++i) {
    if (kinds[i] < -1 || kinds[i] >= h->d)
      return fail(h, GPX_E_ARG, "gpx_append_rows: a kind is -1 (a value) or a dimension in [0, d)");
    if (ids[i] < -1) return fail(h, GPX_E_ARG, "gpx_append_rows: a path id is -1 (no path) or >= 0");
    deriv |= kinds[i] >= 0;
    path |= ids[i] >= 0;
  }
  if (deriv && !cov::differentiable(h->cfg.kernel))
    return fail(h, GPX_E_UNSUPPORTED, "gpx_append_rows: derivative observations: " MATERN12_NO_GRAD);
  if (deriv && !h->kinded)
    return fail(h, GPX_E_ARG, "gpx_append_rows: a derivative row needs a fit made with observation kinds set "
                              "(gpx_set_observation_kinds): this fit has no sn2_deriv");
  if (path && !h->grouped)
    return fail(h, GPX_E_ARG, "gpx_append_rows: a path id >= 0 needs a fit made with path ids (gpx_set_path_groups, sg2 > 0)");
  // a plain or weighted fit (then every kind and id is -1): gpx_append_weighted itself.  A fit made with kinds set stays
  // one, also when neither it nor the new rows hold a derivative: it keeps its sn2_deriv for the rows of a later append.
  if (!h->kinded && !h->grouped) return append_entry(h, Xnew, ynew, wnew, m, mem_kind, info);
  if ((rc = begin_call(h))) return rc;
  h->pw = {};  // the factor changes: a stored pathwise draw goes
  if (wnew && (rc = check_weights(h, "gpx_append_rows", wnew, m, mem_kind, h->cfg.dtype == GPX_F32 ? 4 : 8, h->st)))
    return rc;
  const int32_t* side = h->grouped ? ids.data() : kinds.data();
  return BY_DTYPE(h, append_impl, h, Xnew, ynew, wnew, m, mem_kind, info, side);
}
GPX_CATCH_ALL

int gpx_set_noise_weights(gpx_handle* h, const void* w, int64_t n, int32_t mem_kind) try {
  if (!h) return GPX_E_ARG;
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_set_noise_weights: bad mem_kind");
  if (n < 0 || (n == 0) != (w == nullptr) || n > (int64_t)INT_MAX - 4096)
    return fail(h, GPX_E_ARG, "gpx_set_noise_weights: need n weights, or NULL and 0 to clear them");
  const size_t es = h->cfg.dtype == GPX_F32 ? 4 : 8;
  int rc;
  if (h->group) {  // a group's fit with weights is refused (check_fit_weights): only their count is kept
    if (n > 0 && (rc = check_weights(h, "gpx_set_noise_weights", w, n, mem_kind, es, nullptr))) return rc;
    h->nw_set = n;
    return GPX_OK;
  }
  if (n == 0 && h->nw_set == 0) return GPX_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  h->pw = {};  // the noise model the draw's eps was sampled under is being replaced: a stored pathwise draw goes
  if (n == 0) {
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->Wset = DevBuf();
    h->nw_set = 0;
    return GPX_OK;
  }
  // validated where the caller holds them, before the handle's copy is overwritten: a refused call leaves the weights of
  // the call before in place.  The buffer is kept from call to call (an optimiser sets the same n before every fit).
  if ((rc = check_weights(h, "gpx_set_noise_weights", w, n, mem_kind, es, h->st))) return rc;
  if (h->Wset.cap < (size_t)n * es) {
    DevBuf fresh;  // (allocated before the old one is let go: GPX_E_NOMEM leaves the previous weights too)
    if (hipMalloc(&fresh.p, (size_t)n * es) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, GPX_E_NOMEM, "gpx_set_noise_weights: out of device memory");
    }
    fresh.cap = (size_t)n * es;
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->Wset = std::move(fresh);
  }
  if ((rc = copy_in(h, h->Wset.p, w, (size_t)n * es, mem_kind))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->st));
  h->nw_set = n;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_set_basis(gpx_handle* h, int32_t basis) try {
  if (!h) return GPX_E_ARG;
  if (basis < GPX_BASIS_NONE || basis > GPX_BASIS_QUADRATIC)
    return fail(h, GPX_E_ARG, "gpx_set_basis: need GPX_BASIS_NONE, _CONSTANT, _LINEAR or _QUADRATIC");
  h->basis_set = basis;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_basis(gpx_handle* h, int32_t* basis, int32_t* p, double* beta, double* beta_cov) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !basis || !p) return fail(h, GPX_E_ARG, "gpx_get_basis: no fit or null output");
  *basis = h->basis;
  *p = h->bp;
  if (!h->bp || (!beta && !beta_cov)) return GPX_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  std::vector<double> st((size_t)BASIS_STATE);
  HIPCHK(h, hipMemcpyAsync(st.data(), h->Bst.p, st.size() * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  const int bp = h->bp, k = h->k;
  for (int j = 0; j < bp; ++j) {  // the state block's rows are 64 wide (gpx_internal.h: BASIS_STATE)
    if (beta) std::copy(&st[(size_t)j * 64], &st[(size_t)j * 64 + k], beta + (size_t)j * k);
    if (beta_cov) std::copy(&st[2 * 4096 + (size_t)j * 64], &st[2 * 4096 + (size_t)j * 64 + bp], beta_cov + (size_t)j * bp);
  }
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_noise_weights(gpx_handle* h, void* out) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !out) return fail(h, GPX_E_ARG, "gpx_get_noise_weights: no fit or null output");
  const bool f32 = h->cfg.dtype == GPX_F32;
  const int64_t N = h->group ? h->group->members[0]->N : h->N;
  if (!h->weighted) {
    for (int64_t i = 0; i < N; ++i)
      if (f32) ((float*)out)[i] = 1.0f; else ((double*)out)[i] = 1.0;
    return GPX_OK;
  }
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const void* src = h->cfg.dtype == GPX_MIXED ? h->Wfit64.p : h->Wfit.p;
  HIPCHK(h, hipMemcpyAsync(out, src, (size_t)N * (f32 ? 4 : 8), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_set_observation_kinds(gpx_handle* h, const int32_t* kind, int64_t n, double sn2_deriv, int32_t mem_kind) try {
  if (!h) return GPX_E_ARG;
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_set_observation_kinds: bad mem_kind");
  if (n < 0 || (n == 0) != (kind == nullptr) || n > (int64_t)INT_MAX - 4096)
    return fail(h, GPX_E_ARG, "gpx_set_observation_kinds: need n kinds, or NULL and 0 to clear them");
  if (n == 0) {
    h->kinds_set.clear();
    h->sn2_deriv_set = 0.0;
    return GPX_OK;
  }
  if (!variance_ok(sn2_deriv)) return fail(h, GPX_E_ARG, "gpx_set_observation_kinds: sn2_deriv must be finite and >= 0");
  // validated in a copy of the caller's array, before the handle's is replaced: a refused call leaves the kinds of the
  // call before in place
  std::vector<int32_t> fresh;
  if (int rc = fetch_ids(h, kind, n, mem_kind, fresh)) return rc;
  if (first_below_minus_one(fresh.data(), n) < n)
    return fail(h, GPX_E_ARG, "gpx_set_observation_kinds: a kind is -1 (a value) or a dimension >= 0");
  h->kinds_set = std::move(fresh);
  h->sn2_deriv_set = sn2_deriv;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_observation_kinds(gpx_handle* h, int32_t* out) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !out) return fail(h, GPX_E_ARG, "gpx_get_observation_kinds: no fit or null output");
  const int64_t N = h->group ? h->group->members[0]->N : h->N;
  if (h->kinded && (int64_t)h->kinds_fit.size() == N)
    std::copy(h->kinds_fit.begin(), h->kinds_fit.end(), out);
  else
    std::fill(out, out + N, (int32_t)-1);
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_set_path_groups(gpx_handle* h, const int32_t* group, int64_t n, double sg2, const double* ls_path,
                        int32_t n_ls_path, int32_t mem_kind) try {
  if (!h) return GPX_E_ARG;
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_set_path_groups: bad mem_kind");
  if (n < 0 || (n == 0) != (group == nullptr) || n > (int64_t)INT_MAX - 4096)
    return fail(h, GPX_E_ARG, "gpx_set_path_groups: need n path ids, or NULL and 0 to clear them");
  if (n == 0) {
    h->groups_set.clear();
    h->lsp_set.clear();
    h->sg2_set = 0.0;
    return GPX_OK;
  }
  if (!variance_ok(sg2)) return fail(h, GPX_E_ARG, "gpx_set_path_groups: sg2 must be finite and >= 0");
  if (!ls_path || n_ls_path < 1 || n_ls_path > MAX_D)
    return fail(h, GPX_E_ARG, "gpx_set_path_groups: need 1 or d path lengthscales");
  if (!path_ls_ok(ls_path, n_ls_path))
    return fail(h, GPX_E_ARG, "gpx_set_path_groups: path lengthscales must be finite and > 0");
  // validated in a copy of the caller's array, before the handle's is replaced: a refused call leaves the setting of the
  // call before in place
  std::vector<int32_t> fresh;
  if (int rc = fetch_ids(h, group, n, mem_kind, fresh)) return rc;
  if (first_below_minus_one(fresh.data(), n) < n)
    return fail(h, GPX_E_ARG, "gpx_set_path_groups: a path id is -1 (no path) or >= 0");
  h->groups_set = std::move(fresh);
  h->lsp_set.assign(ls_path, ls_path + n_ls_path);
  h->sg2_set = sg2;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_path_groups(gpx_handle* h, int32_t* out) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !out) return fail(h, GPX_E_ARG, "gpx_get_path_groups: no fit or null output");
  const int64_t N = h->group ? h->group->members[0]->N : h->N;
  if (h->grouped && (int64_t)h->groups_fit.size() == N)
    std::copy(h->groups_fit.begin(), h->groups_fit.end(), out);
  else
    std::fill(out, out + N, (int32_t)-1);
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_forecast_blocks(gpx_handle* h, const void* Xb, const void* yo, int64_t G, int32_t Lo, int32_t Lp, double diag_add,
                        void* mean, void* cov, void* var, void* logp, int32_t mem_kind, int64_t* info) try {
  if (!h) return GPX_E_ARG;
  if (!Xb || !yo || !mean || !info || G <= 0) return fail(h, GPX_E_ARG, "gpx_forecast_blocks: bad argument");
  if (Lo < 1 || Lp < 1 || (int64_t)Lo + Lp > 64)
    return fail(h, GPX_E_ARG, "gpx_forecast_blocks: need 1 <= Lo, 1 <= Lp and Lo + Lp <= 64");
  if (!(diag_add >= 0.0)) return fail(h, GPX_E_ARG, "gpx_forecast_blocks: need diag_add >= 0");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_forecast_blocks: bad mem_kind");
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_forecast_blocks: handle has no successful fit");
  const int32_t Lg = Lo + Lp;
  if (G > ((int64_t)INT_MAX - 4096) / (Lg * (int64_t)Lp)) return fail(h, GPX_E_ARG, "gpx_forecast_blocks: G too large");
  int rc;
  if ((rc = posterior_refused(h, "gpx_forecast_blocks"))) return rc;
  if ((rc = begin_call(h))) return rc;
  const ForecastOut fc{Lp, mean, cov, var, logp};
  return BY_DTYPE(h, score_impl, h, Xb, yo, nullptr, G, Lg, diag_add, nullptr, nullptr, nullptr, mem_kind, info, &fc);
}
GPX_CATCH_ALL

int gpx_reserve(gpx_handle* h, int64_t capacity) try {
  if (!h) return GPX_E_ARG;
  if (capacity < 0 || capacity > (int64_t)INT_MAX - 4096) return fail(h, GPX_E_ARG, "gpx_reserve: bad capacity");
  int rc;
  if ((rc = posterior_refused(h, "gpx_reserve"))) return rc;
  // (0 takes a reservation back: nothing of the current fit depends on it, an append without one grows the layout itself)
  if (h->fitted && capacity > 0 && capacity < h->N)
    return fail(h, GPX_E_ARG, "gpx_reserve: the handle already holds more points");
  h->reserve = capacity;  // laid out by the next gpx_fit / gpx_append
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_factor_info(gpx_handle* h, const void** factor, int64_t* ld, int64_t* capacity) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_factor_info: handle has no successful fit");
  int rc;
  if ((rc = posterior_refused(h, "gpx_factor_info"))) return rc;
  const int64_t skew = h->cfg.dtype == GPX_F32 ? ld_skew<float>() : ld_skew<double>();
  if (factor) *factor = h->K.p;
  if (ld) *ld = h->ld;
  if (capacity) *capacity = h->ld - skew;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_alpha(gpx_handle* h, void* out) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !out) return fail(h, GPX_E_ARG, "gpx_get_alpha: no fit or null output");
  if (h->group) {  // alpha is replicated (or solved on demand from the replicated factor): rank 0 has it
    gpx_handle* m0 = h->group->members[0];
    const int rc = gpx_get_alpha(m0, out);
    if (rc != GPX_OK) h->err = m0->err;
    return rc;
  }
  refresh_env(h);  // (not begin_call: the clocks and the message of the call before stay)
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (h->cfg.dtype == GPX_MIXED) return mixed_alpha(h, out);
  return BY_DTYPE(h, alpha_impl, h, out);
}
GPX_CATCH_ALL

int gpx_lml_grad(gpx_handle* h, double* lml, double* grad) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !lml || !grad) return fail(h, GPX_E_ARG, "gpx_lml_grad: no fit or null output");
  if (h->cfg.dtype != GPX_F64) return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad: fp64 handles only");
  if (h->grouped)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad: the fit has path ids (gpx_set_path_groups); the gradient passes evaluate "
                                      "dK / dtheta matrix-free without the within-path covariance (difference the LML instead)");
  if (h->has_deriv)  // (n_ls + 2 entries have no room for d / dlog sn2_deriv)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad: the fit has derivative observations (gpx_set_observation_kinds): "
                                      "call gpx_lml_grad_full, whose gradient has the n_ls + 3 entries of such a fit");
  if (h->group) return group_lml_grad(h, lml, grad);
  if (h->cfg.world > 1 && !h->comm) return fail(h, GPX_E_ARG, "gpx_lml_grad: sharded handle without a communicator");
  int rc;
  if ((rc = begin_call(h))) return rc;
  if (h->comm && !h->repl) return shard_lml_grad_dist(h, lml, grad);  // factor only held distributed
  return lml_grad_impl(h, lml, grad);
}
GPX_CATCH_ALL

int gpx_lml_grad_full(gpx_handle* h, double* lml, double* grad) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !lml || !grad) return fail(h, GPX_E_ARG, "gpx_lml_grad_full: no fit or null output");
  if (h->cfg.dtype != GPX_F64) return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_full: fp64 handles only");
  if (h->group || h->comm || h->cfg.world > 1)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_full: single-device handles only (gpx_lml_grad on shards and groups)");
  if (h->grouped)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_full: the fit has path ids (gpx_set_path_groups); the gradient passes "
                                      "evaluate dK / dtheta matrix-free without the within-path covariance (difference the "
                                      "LML instead)");
  int rc;
  if ((rc = begin_call(h))) return rc;
  if (h->has_deriv) return lml_grad_impl(h, lml, grad, true);
  if ((rc = lml_grad_impl(h, lml, grad))) return rc;  // no derivative row: gpx_lml_grad's numbers
  grad[h->n_ls + 2] = 0.0;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_lml_grad_paths(gpx_handle* h, double* lml, double* grad, double* grad_path, int32_t n_path) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !lml || !grad || n_path < 0 || (n_path > 0 && !grad_path))
    return fail(h, GPX_E_ARG, "gpx_lml_grad_paths: no fit, null output or n_path < 0");
  if (h->cfg.dtype != GPX_F64) return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_paths: fp64 handles only");
  if (h->group || h->comm || h->cfg.world > 1)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_paths: single-device handles only (no fit with path ids exists on shards "
                                      "and groups; gpx_lml_grad there)");
  if (h->has_deriv)
    return fail(h, GPX_E_UNSUPPORTED, "gpx_lml_grad_paths: the fit has derivative observations (gpx_set_observation_kinds), "
                                      "which exclude path ids: call gpx_lml_grad_full");
  if (h->grouped && n_path != 1 + h->n_lsp) {
    char buf[200];
    snprintf(buf, sizeof buf, "gpx_lml_grad_paths: the fit has %d path lengthscale(s): grad_path needs n_path = %d, not %d",
             h->n_lsp, 1 + h->n_lsp, (int)n_path);
    return fail(h, GPX_E_ARG, buf);
  }
  int rc;
  if ((rc = begin_call(h))) return rc;
  if (h->grouped) return lml_grad_impl(h, lml, grad, false, grad_path);
  if ((rc = lml_grad_impl(h, lml, grad))) return rc;  // no effective path ids: gpx_lml_grad's launches and numbers
  for (int32_t t = 0; t < n_path; ++t) grad_path[t] = 0.0;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_loo(gpx_handle* h, double* mean, double* var, double* logp, double* total) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || (!mean && !var && !logp && !total)) return fail(h, GPX_E_ARG, "gpx_loo: no fit or no output");
  if (h->cfg.dtype != GPX_F64) return fail(h, GPX_E_UNSUPPORTED, "gpx_loo: fp64 handles only");
  if (h->group || h->comm || h->cfg.world > 1) return fail(h, GPX_E_UNSUPPORTED, "gpx_loo: single-device handles only");
  int rc;
  if ((rc = begin_call(h))) return rc;
  return loo_impl(h, mean, var, logp, total);
}
GPX_CATCH_ALL

namespace {
// what the pathwise calls refuse beyond their arguments, before anything is computed: the handles the joint-posterior calls
// refuse, and the fits whose covariance is not the plain k(x, x') the features approximate
int pathwise_refused(gpx_handle* h, const char* fn) {
  if (int rc = posterior_refused(h, fn)) return rc;
  if (h->has_deriv)
    return fail(h, GPX_E_UNSUPPORTED, fn, "the fit has derivative observations (gpx_set_observation_kinds): not supported");
  if (h->grouped) return fail(h, GPX_E_UNSUPPORTED, fn, "the fit has path ids (gpx_set_path_groups): not supported");
  return basis_refused(h, fn, "the sampled functions do not include the basis terms");
}
}  // namespace

int gpx_pathwise_draw(gpx_handle* h, int64_t S, int64_t F, uint64_t seed, const void* z, int32_t mem_kind) try {
  if (!h) return GPX_E_ARG;
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_pathwise_draw", "bad mem_kind");
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_pathwise_draw", "handle has no successful fit");
  if (S < 0 || (S > 0 && F < 1)) return fail(h, GPX_E_ARG, "gpx_pathwise_draw", "need S >= 0 samples and F >= 1 frequencies");
  int rc;
  if ((rc = pathwise_refused(h, "gpx_pathwise_draw"))) return rc;
  if (S > 0 && (S > ((int64_t)1 << 20) / h->k || F > (int64_t)1 << 24))
    return fail(h, GPX_E_ARG, "gpx_pathwise_draw", "S k (at most 2^20 columns) or F (at most 2^24) too large");
  if ((rc = begin_call(h))) return rc;
  if (S == 0) {
    h->pw = {};
    return GPX_OK;
  }
  return BY_DTYPE(h, pathwise_draw_impl, h, S, F, seed, z, mem_kind);
}
GPX_CATCH_ALL

int gpx_pathwise_eval(gpx_handle* h, const void* Xs, int64_t M, int64_t s0, int64_t S, void* out, int32_t mem_kind) try {
  if (!h) return GPX_E_ARG;
  if (!Xs || !out || M <= 0 || S <= 0 || s0 < 0) return fail(h, GPX_E_ARG, "gpx_pathwise_eval", "bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, "gpx_pathwise_eval", "bad mem_kind");
  if (!h->fitted) return fail(h, GPX_E_ARG, "gpx_pathwise_eval", "handle has no successful fit");
  int rc;
  if ((rc = pathwise_refused(h, "gpx_pathwise_eval"))) return rc;
  if (h->pw.S == 0)
    return fail(h, GPX_E_ARG, "gpx_pathwise_eval",
                "no live draw: call gpx_pathwise_draw first (a fit, append, removal or new noise weights drops the draw)");
  if (s0 > h->pw.S || S > h->pw.S - s0)
    return fail(h, GPX_E_ARG, "gpx_pathwise_eval", "samples [s0, s0 + S) must lie inside the draw");
  if (M > (int64_t)INT_MAX - 4096) return fail(h, GPX_E_ARG, "gpx_pathwise_eval", "M too large");
  if ((rc = begin_call(h))) return rc;
  return BY_DTYPE(h, pathwise_eval_impl, h, Xs, M, s0, S, out, mem_kind);
}
GPX_CATCH_ALL

int gpx_pathwise_info(gpx_handle* h, int64_t* S, int64_t* F, int64_t* n_normals) try {
  if (!h) return GPX_E_ARG;
  if (S) *S = h->pw.S;
  if (F) *F = h->pw.F;
  if (n_normals) *n_normals = h->pw.n_normals;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_release_scratch(gpx_handle* h) try {
  if (!h) return GPX_E_ARG;
  std::vector<gpx_handle*> hs;
  if (h->group)
    hs = h->group->members;
  else
    hs.push_back(h);
  for (gpx_handle* m : hs) {
    HIPCHK(h, hipSetDevice(m->cfg.device));
    for (hipStream_t sx : {m->st, m->st2, m->st3, m->st4, m->st5})
      if (sx) HIPCHK(h, hipStreamSynchronize(sx));
    m->scr = {};  // every scratch buffer moves into a temporary that frees it
  }
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_logdet(gpx_handle* h, double* out) try {
  if (!h) return GPX_E_ARG;
  if (!h->fitted || !out) return fail(h, GPX_E_ARG, "gpx_logdet: no fit or null output");
  *out = h->group ? h->group->members[0]->logdet : h->logdet;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_set_flags(gpx_handle* h, int32_t flags) try {
  if (!h || (flags & ~GPX_FLAG_PROFILE)) return GPX_E_ARG;
  h->cfg.flags = flags;
  if (h->group)
    for (gpx_handle* m : h->group->members) m->cfg.flags = flags;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_get_timings(gpx_handle* h, gpx_timings* out) try {
  if (!h || !out) return GPX_E_ARG;
  *out = h->group ? h->group->members[0]->tm : h->tm;  // a group reports rank 0's clocks
  return GPX_OK;
}
GPX_CATCH_ALL

// ---- kernel unit-test entry points -------------------------------------------------------
// Every HIP failure of these entry points is GPX_E_HIP, a failed allocation included, with the failing call in
// gpx_last_error(NULL).  A call's Dev buffers are declared after its Scratch, so they free themselves before the streams go.
#define UCHK(call)                                                              \
  do {                                                                          \
    if ((call) != hipSuccess) return fail(nullptr, GPX_E_HIP, #call " failed"); \
  } while (0)

extern "C++" {
namespace {
struct Scratch {  // a throw-away handle-like context for the host-buffer entry points
  gpx_handle h;
  hipStream_t& st = h.st;  // the main stream: what an entry point enqueues goes here
  bool ok = false;
  Scratch() {
    int dev = 0;
    refresh_env(&h);  // the schedulers a unit-test entry point runs read h.env like any call
    if (hipGetDevice(&dev) != hipSuccess) return;
    h.cfg.device = dev;
    ok = true;
    for (hipStream_t* s : {&h.st, &h.st2, &h.st3, &h.st4})
      ok = ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess;
  }
  int finish() {  // what the call enqueued on the main stream has run, and without an error
    UCHK(hipStreamSynchronize(st));
    UCHK(hipGetLastError());
    return GPX_OK;
  }
};  // (~gpx_handle tears down streams, events and whatever buffer a scheduler function allocated)

template <typename T>
struct Dev : DevBuf {  // a DevBuf of `count` elements that reads as the T* it holds
  operator T*() const { return (T*)p; }
  int alloc(size_t count) {
    UCHK(hipMalloc(&p, count * sizeof(T)));
    return GPX_OK;
  }
  int upload(const T* src, size_t count, hipStream_t st, size_t room = 0) {  // room for max(count, room); count from the host
    UCHK(hipMalloc(&p, std::max(count, room) * sizeof(T)));
    UCHK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return GPX_OK;
  }
};

// What the kernel-matrix calls check alike, all of it GPX_E_ARG without a message: na x nb points of 1 <= d <= MAX_D
// dimensions with n_ls = 1 or d lengthscales; the element type; path ids >= -1 with lengthscales and sg2 as
// gpx_set_path_groups takes them.
bool sizes_ok(int64_t na, int64_t nb, int32_t d, int32_t n_ls) {
  return na > 0 && nb > 0 && d > 0 && d <= MAX_D && (n_ls == 1 || n_ls == d);
}
bool unit_dtype_ok(int32_t dtype) { return dtype == GPX_F64 || dtype == GPX_F32; }
bool path_args_ok(const int32_t* ga, int64_t na, const int32_t* gb, int64_t nb, const double* ls_path, int32_t n_ls_path,
                  double sg2) {
  return variance_ok(sg2) && path_ls_ok(ls_path, n_ls_path) && first_below_minus_one(ga, na) == na &&
         first_below_minus_one(gb, nb) == nb;
}
// the kinds of both sides (null: all values) lie in [-1, d); a derivative among them on Matern-1/2 is refused under fn
int kinds_refused(const char* fn, int32_t kernel, const int32_t* ka, int64_t na, const int32_t* kb, int64_t nb, int32_t d) {
  bool deriv = false;
  for (auto [kind, n] : {std::pair{ka, na}, std::pair{kb, nb}})
    for (int64_t i = 0; kind && i < n; ++i) {
      if (kind[i] < -1 || kind[i] >= d) return GPX_E_ARG;
      deriv |= kind[i] >= 0;
    }
  if (deriv && !cov::differentiable(kernel)) return fail(nullptr, GPX_E_UNSUPPORTED, fn, MATERN12_NO_GRAD);
  return GPX_OK;
}

// The staging the seven kernel-matrix calls share, on a Scratch of its own: the points scaled by the lengthscales, the side
// arrays and the output on the device, the result back in the caller's dense array.  An entry point is its argument
// checks, these calls, its one launch, fetch.
template <typename T>
struct KernelCall {
  Scratch sc;
  hipStream_t st = sc.st;
  int d = 0;
  int64_t na = 0, nb = 0, napad = 0, nbpad = 0, ld = 0, nblk = 0;
  std::vector<T> hA, hB, host;  // the points rounded to T, the padded result (the sources live until fetch has synchronised)
  Dev<T> A, B, As, Bs, K;      // points raw and scaled (n x d, round_up(n, 64) x d), nblk blocks of napad x ld
  Dev<double> ls, q;            // MAX_D entries each
  Dev<int32_t> ga, gb;
  int scaled(Dev<T>& raw, Dev<T>& scl, const std::vector<T>& h, int64_t n, int64_t npad, int32_t n_ls) {
    if (int rc; (rc = raw.upload(h.data(), h.size(), st)) || (rc = scl.alloc((size_t)npad * d))) return rc;
    launch_scale_points<T>(raw, n, npad, d, ls, n_ls, scl, st);
    return GPX_OK;
  }
  // A (na x d) and B (nb x d; null: the symmetric call, nb = na) scaled by the n_ls lengthscales
  int points(const double* A_, int64_t na_, const double* B_, int64_t nb_, int32_t d_, const double* lengthscale, int32_t n_ls) {
    if (!sc.ok) return GPX_E_HIP;
    d = d_, na = na_, nb = B_ ? nb_ : na_, napad = round_up(na, 64), nbpad = round_up(nb, 64), ld = nbpad;
    hA.assign(A_, A_ + na * d);
    if (B_) hB.assign(B_, B_ + nb * d);
    if (int rc; (rc = ls.upload(lengthscale, n_ls, st, MAX_D)) || (rc = scaled(A, As, hA, na, napad, n_ls)) || !B_) return rc;
    return scaled(B, Bs, hB, nb, nbpad, n_ls);
  }
  // One int32 array per side (ids or kinds).  padded: at the padded length, -1 beyond the values and on a side without any;
  // else at n, and a null device pointer for a side without any.
  int side(Dev<int32_t>& g, const int32_t* src, int64_t n, int64_t npad, bool padded) {
    if (!padded) return src ? g.upload(src, n, st) : GPX_OK;
    if (int rc = g.alloc(npad)) return rc;
    UCHK(hipMemsetAsync(g, 0xFF, (size_t)npad * 4, st));
    if (src) UCHK(hipMemcpyAsync(g, src, (size_t)n * 4, hipMemcpyHostToDevice, st));
    return GPX_OK;
  }
  int sides(const int32_t* a, const int32_t* b, bool padded, const double* q_ = nullptr) {  // q_: the caller's d entries of q
    int rc;
    if (q_ && (rc = q.upload(q_, d, st, MAX_D))) return rc;
    return (rc = side(ga, a, na, napad, padded)) ? rc : side(gb, b, nb, nbpad, padded);
  }
  int output(int64_t nblk_, bool zero) {
    host.resize((size_t)(nblk = nblk_) * napad * ld);
    if (int rc = K.alloc(host.size())) return rc;
    if (zero) UCHK(hipMemsetAsync(K, 0, host.size() * sizeof(T), st));
    return GPX_OK;
  }
  int fetch(double* out) {  // -> (nblk, na, nb), dense
    UCHK(hipMemcpyAsync(host.data(), K, host.size() * sizeof(T), hipMemcpyDeviceToHost, st));
    if (int rc = sc.finish()) return rc;
    for (int64_t b = 0; b < nblk; ++b)
      for (int64_t i = 0; i < na; ++i)
        for (int64_t j = 0; j < nb; ++j) out[(b * na + i) * nb + j] = (double)host[(size_t)(b * napad + i) * ld + j];
    return GPX_OK;
  }
};

// gpx_kernel_path_matrix, K (na, nb), and gpx_kernel_path_grad_matrix (grad), K (d, na, nb) = the d derivative matrices by
// A: one body; fn names the call in the message
int kernel_path_entry(const char* fn, bool grad, int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na,
                      const double* B, const int32_t* gb, int64_t nb_, int32_t d, const double* lengthscale, int32_t n_ls,
                      double sf2, const double* ls_path, int32_t n_ls_path, double sg2, double* K) {
  if (!A || !B || !ga || !gb || !K || !lengthscale || !ls_path || !sizes_ok(na, nb_, d, n_ls) ||
      (n_ls_path != 1 && n_ls_path != d))
    return GPX_E_ARG;
  if (!cov::known(kernel) || !unit_dtype_ok(dtype) || !path_args_ok(ga, na, gb, nb_, ls_path, n_ls_path, sg2)) return GPX_E_ARG;
  if (grad && !cov::differentiable(kernel)) return fail(nullptr, GPX_E_UNSUPPORTED, fn, MATERN12_NO_GRAD);
  std::vector<double> q((size_t)d);
  for (int c = 0; c < d; ++c) q[c] = lengthscale[n_ls == 1 ? 0 : c] / ls_path[n_ls_path == 1 ? 0 : c];
  for (double& r : q) r *= r;
  auto run = [&](auto t) {
    using T = decltype(t);
    KernelCall<T> kc;
    if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) || (rc = kc.sides(ga, gb, true, q.data())) ||
        (rc = kc.output(grad ? d : 1, false)))
      return rc;
    if (grad)
      launch_kgrad_build_g<T>(kernel, kc.As, kc.ga, na, kc.napad, kc.Bs, kc.gb, nb_, kc.nbpad, d, sf2, kc.ls, n_ls, kc.q, sg2, 0,
                              kc.K, kc.ld, kc.st);
    else
      launch_kbuild_cross_g<T>(kernel, kc.As, kc.ga, na, kc.napad, kc.Bs, kc.gb, nb_, kc.nbpad, d, sf2, kc.q, sg2, kc.K, kc.ld,
                               kc.st);
    return kc.fetch(K);
  };
  return dtype == GPX_F32 ? run(float()) : run(double());
}

// the two MFMA probes: D (16 x 16) from A, B (64 entries each), in one buffer of 64 + 64 + 256 elements
template <typename T>
int mfma_probe_t(const T* A, const T* B, T* D, void (*launch)(const T*, const T*, T*, hipStream_t)) {
  if (!A || !B || !D) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  Dev<T> d;
  if (int rc = d.upload(A, 64, sc.st, 64 + 64 + 256)) return rc;
  UCHK(hipMemcpyAsync(d + 64, B, 64 * sizeof(T), hipMemcpyHostToDevice, sc.st));
  launch(d, d + 64, d + 128, sc.st);
  UCHK(hipMemcpyAsync(D, d + 128, 256 * sizeof(T), hipMemcpyDeviceToHost, sc.st));
  return sc.finish();
}
}  // namespace
}  // extern "C++"

int gpx_kernel_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb_,
                      int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                      double diag_add, double* K) try {
  if (!A || !K || !lengthscale || !sizes_ok(na, B ? nb_ : na, d, n_ls) || !cov::known(kernel)) return GPX_E_ARG;
  KernelCall<double> kc;
  if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) || (rc = kc.output(1, true))) return rc;
  if (B)
    launch_kbuild_cross<double>(kernel, kc.As, na, kc.napad, kc.Bs, nb_, kc.nbpad, d, sf2, kc.K, kc.ld, kc.st);
  else  // (the upper part is not built: it stays zero)
    launch_kbuild_sym<double>(kernel, kc.As, na, kc.napad, d, sf2, diag_add, kc.K, kc.ld, kc.st);
  return kc.fetch(K);
}
GPX_CATCH_ALL

// the original entry point keeps its original kernel set (RBF, Matern-5/2); every family: gpx_kernel_deriv_matrix
int gpx_kernel_grad_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb_, int32_t d,
                           const double* lengthscale, int32_t n_ls, double sf2, double* G) {
  if (kernel != GPX_KERNEL_RBF && kernel != GPX_KERNEL_MATERN52) return GPX_E_ARG;
  return gpx_kernel_deriv_matrix(kernel, A, na, B, nb_, d, lengthscale, n_ls, sf2, G);
}

int gpx_kernel_deriv_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb_, int32_t d,
                            const double* lengthscale, int32_t n_ls, double sf2, double* G) try {
  if (!A || !B || !G || !lengthscale || !sizes_ok(na, nb_, d, n_ls) || !cov::known(kernel)) return GPX_E_ARG;
  if (!cov::differentiable(kernel)) return fail(nullptr, GPX_E_UNSUPPORTED, "gpx_kernel_deriv_matrix", MATERN12_NO_GRAD);
  KernelCall<double> kc;
  if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) || (rc = kc.output(d, false))) return rc;
  launch_kgrad_build<double>(kernel, kc.As, na, kc.napad, kc.Bs, nb_, kc.nbpad, d, sf2, kc.ls, n_ls, 0, kc.K, kc.ld, kc.st);
  return kc.fetch(G);
}
GPX_CATCH_ALL

int gpx_kernel_path_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na, const double* B,
                           const int32_t* gb, int64_t nb_, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                           const double* ls_path, int32_t n_ls_path, double sg2, double* K) try {
  return kernel_path_entry("gpx_kernel_path_matrix", false, kernel, dtype, A, ga, na, B, gb, nb_, d, lengthscale, n_ls, sf2,
                           ls_path, n_ls_path, sg2, K);
}
GPX_CATCH_ALL

int gpx_kernel_path_grad_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na,
                                const double* B, const int32_t* gb, int64_t nb_, int32_t d, const double* lengthscale,
                                int32_t n_ls, double sf2, const double* ls_path, int32_t n_ls_path, double sg2,
                                double* G) try {
  return kernel_path_entry("gpx_kernel_path_grad_matrix", true, kernel, dtype, A, ga, na, B, gb, nb_, d, lengthscale, n_ls, sf2,
                           ls_path, n_ls_path, sg2, G);
}
GPX_CATCH_ALL

int gpx_kernel_mixed_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ka, int64_t na, const double* B,
                            const int32_t* kb, int64_t nb_, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                            double* K) try {
  if (!A || !B || !K || !lengthscale || !sizes_ok(na, nb_, d, n_ls)) return GPX_E_ARG;
  if (!cov::known(kernel) || !unit_dtype_ok(dtype)) return GPX_E_ARG;
  if (int rc = kinds_refused("gpx_kernel_mixed_matrix", kernel, ka, na, kb, nb_, d)) return rc;
  auto run = [&](auto t) {
    using T = decltype(t);
    KernelCall<T> kc;
    if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) || (rc = kc.sides(ka, kb, true)) || (rc = kc.output(1, false)))
      return rc;
    if (cov::differentiable(kernel))
      launch_kbuild_cross_kk<T>(kernel, kc.As, kc.ga, na, kc.napad, kc.Bs, kc.gb, nb_, kc.nbpad, d, sf2, kc.ls, n_ls, kc.K,
                                kc.ld, kc.st);
    else  // (Matern-1/2: values only, and the fit builds them with the plain builder)
      launch_kbuild_cross<T>(kernel, kc.As, na, kc.napad, kc.Bs, nb_, kc.nbpad, d, sf2, kc.K, kc.ld, kc.st);
    return kc.fetch(K);
  };
  return dtype == GPX_F32 ? run(float()) : run(double());
}
GPX_CATCH_ALL

int gpx_kernel_hess_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na, const double* B,
                           const int32_t* side_b, int64_t nb_, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                           const double* ls_path, int32_t n_ls_path, double sg2, double* G) try {
  const char* fn = "gpx_kernel_hess_matrix";
  if (!A || !B || !G || !lengthscale || !sizes_ok(na, nb_, d, n_ls) || !cov::known(kernel) || !unit_dtype_ok(dtype))
    return GPX_E_ARG;
  std::vector<double> q;
  if (ga) {  // path ids on both sides
    if (!side_b || !ls_path || (n_ls_path != 1 && n_ls_path != d) || !path_args_ok(ga, na, side_b, nb_, ls_path, n_ls_path, sg2))
      return GPX_E_ARG;
    for (int c = 0; c < d; ++c) q.push_back(lengthscale[n_ls == 1 ? 0 : c] / ls_path[n_ls_path == 1 ? 0 : c]);
    for (double& r : q) r *= r;
  } else if (side_b) {  // kinds of the columns
    if (int rc = kinds_refused(fn, kernel, nullptr, 0, side_b, nb_, d)) return rc;
  }
  if (!cov::twice_differentiable(kernel)) return fail(nullptr, GPX_E_UNSUPPORTED, fn, NOT_TWICE_DIFFERENTIABLE);
  if (d > MAX_HESS_D) return fail(nullptr, GPX_E_UNSUPPORTED, fn, HESS_D_LIMIT);
  auto run = [&](auto t) {
    using T = decltype(t);
    KernelCall<T> kc;
    if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) ||
                (rc = kc.sides(ga, side_b, true, ga ? q.data() : nullptr)) || (rc = kc.output(hess_pairs(d), false)))
      return rc;
    launch_khess_build<T>(kernel, kc.As, ga ? (const int32_t*)kc.ga : nullptr, na, kc.napad, kc.Bs,
                          side_b ? (const int32_t*)kc.gb : nullptr, nb_, kc.nbpad, d, sf2, kc.ls, n_ls,
                          ga ? (const double*)kc.q : nullptr, sg2, kc.K, kc.ld, kc.st);
    return kc.fetch(G);
  };
  return dtype == GPX_F32 ? run(float()) : run(double());
}
GPX_CATCH_ALL

int gpx_kernel_dl_matrix(int32_t kernel, const double* A, const int32_t* ka, int64_t na, const double* B,
                         const int32_t* kb, int64_t nb_, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                         double* G) try {
  if (!A || !B || !G || !lengthscale || !sizes_ok(na, nb_, d, n_ls) || !cov::known(kernel)) return GPX_E_ARG;
  if (int rc = kinds_refused("gpx_kernel_dl_matrix", kernel, ka, na, kb, nb_, d)) return rc;
  KernelCall<double> kc;
  if (int rc; (rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) || (rc = kc.sides(ka, kb, false)) || (rc = kc.output(n_ls, true)))
    return rc;
  launch_dl_matrix(kernel, kc.As, kc.ga, na, kc.napad, kc.Bs, kc.gb, nb_, d, kc.ls, n_ls, sf2, kc.K, kc.ld, kc.st);
  return kc.fetch(G);
}
GPX_CATCH_ALL

int gpx_kernel_path_dtheta_matrix(int32_t kernel, const double* A, const int32_t* ga, int64_t na, const double* B,
                                  const int32_t* gb, int64_t nb_, int32_t d, const double* ls_path, int32_t n_ls_path,
                                  double sg2, double* G) try {
  if (!A || !B || !ga || !gb || !G || !ls_path || !sizes_ok(na, nb_, d, n_ls_path)) return GPX_E_ARG;
  if (!cov::known(kernel) || !path_args_ok(ga, na, gb, nb_, ls_path, n_ls_path, sg2)) return GPX_E_ARG;
  // the points are scaled by l_path itself, so q = 1: r_p^2 = sum_c ((x_ic - x_jc) / l_path,c)^2 as in a fit with l = l_path
  KernelCall<double> kc;
  const std::vector<double> q((size_t)d, 1.0);
  if (int rc; (rc = kc.points(A, na, B, nb_, d, ls_path, n_ls_path)) || (rc = kc.sides(ga, gb, false, q.data())) ||
      (rc = kc.output(1 + n_ls_path, true)))
    return rc;
  launch_path_dtheta_matrix(kernel, kc.As, kc.ga, na, kc.napad, kc.Bs, kc.gb, nb_, d, kc.q, n_ls_path, sg2, kc.K, kc.ld, kc.st);
  return kc.fetch(G);
}
GPX_CATCH_ALL

int gpx_pathwise_eval_raw(int32_t kernel, int32_t dtype, const double* Xq, int64_t M, const double* X, int64_t N, int32_t d,
                          const double* ls, int32_t n_ls, double sf2, const double* Omega, int64_t F, const double* W,
                          const double* V, int64_t C, double* out) try {
  if (!Xq || !X || !ls || !Omega || !W || !V || !out || !sizes_ok(M, N, d, n_ls) || F < 1 || C < 1) return GPX_E_ARG;
  if (!cov::known(kernel) || !unit_dtype_ok(dtype) || M > (1 << 24) || N > (1 << 24) || F > (1 << 24) || C > (1 << 20))
    return GPX_E_ARG;
  auto run = [&](auto t) -> int {
    using T = decltype(t);
    KernelCall<T> kc;  // the points scaled as the fit's and the queries' are; its output block is not used
    if (int rc = kc.points(Xq, M, X, N, d, ls, n_ls)) return rc;
    const int64_t cpad = round_up(C, 64), ldw = round_up(2 * F, 64), ldv = kc.nbpad, mpad = kc.napad;
    const int nz = pathwise_splits(kc.nbpad, F, true);
    std::vector<T> hW((size_t)cpad * ldw, (T)0), hV((size_t)cpad * ldv, (T)0), hO((size_t)cpad * mpad);
    for (int64_t c = 0; c < C; ++c) {
      for (int64_t j = 0; j < 2 * F; ++j) hW[c * ldw + j] = (T)W[c * 2 * F + j];
      for (int64_t n = 0; n < N; ++n) hV[c * ldv + n] = (T)V[c * N + n];
    }
    Dev<T> dW, dV, part, outT;
    Dev<double> dOm;
    if (int rc; (rc = dW.upload(hW.data(), hW.size(), kc.st)) || (rc = dV.upload(hV.data(), hV.size(), kc.st)) ||
                (rc = dOm.upload(Omega, (size_t)F * d, kc.st)) || (rc = part.alloc((size_t)nz * cpad * mpad)) ||
                (rc = outT.alloc((size_t)cpad * mpad)))
      return rc;
    launch_pathwise_eval<T>(kernel, kc.As, mpad, kc.Bs, kc.nbpad, d, sf2, dV, ldv, dOm, F, dW, ldw, cpad, part, outT, mpad,
                            kc.st);
    UCHK(hipMemcpyAsync(hO.data(), outT, hO.size() * sizeof(T), hipMemcpyDeviceToHost, kc.st));
    if (int rc = kc.sc.finish()) return rc;
    for (int64_t c = 0; c < C; ++c)
      for (int64_t m = 0; m < M; ++m) out[c * M + m] = (double)hO[c * mpad + m];
    return GPX_OK;
  };
  return dtype == GPX_F32 ? run(float()) : run(double());
}
GPX_CATCH_ALL

int gpx_potrf(double* A, int64_t n, int32_t block, int64_t* info) try {
  if (!A || !info || n <= 0 || n % 64 != 0) return GPX_E_ARG;
  const int nb = block == 0 ? 1024 : block;
  if (nb % 128 != 0 || nb < 128) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ld = n + LD_SKEW, ldp = nb + LD_SKEW;
  Dev<double> dA, dW, dP, dWb, dUb;
  Dev<int> dInfo;
  int hinfo = INT_MAX, rc;
  if ((rc = dA.alloc((size_t)n * ld)) || (rc = dW.alloc((size_t)(n / 64) * 4096)) || (rc = dP.alloc((size_t)2 * n * ldp)) ||
      (rc = dInfo.alloc(16)) || (rc = dWb.alloc((size_t)((n + nb - 1) / nb) * nb * nb)) || (rc = dUb.alloc((size_t)nb * ldp)))
    return rc;
  InvWork<double> iw{dWb, dUb, ldp, nb, sc.h.st3};  // W, U, ldu, nbw, aux
  if ((rc = flag_handover_probe(&sc.h))) return fail(nullptr, rc, sc.h.err.c_str());
  UCHK(hipMemcpy2DAsync(dA, (size_t)ld * 8, A, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpyAsync(dInfo, &hinfo, sizeof(int), hipMemcpyHostToDevice, sc.st));
  if ((rc = chol_two_level_enqueue(&sc.h, (double*)dA, ld, n, nb, (double*)dW, (double*)dP, dP + n * ldp, ldp, dInfo, 0, false,
                                   0, &iw)))
    return rc;
  UCHK(hipMemcpy2DAsync(A, (size_t)n * 8, dA, (size_t)ld * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost, sc.st));
  UCHK(hipMemcpyAsync(&hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, sc.st));
  if ((rc = sc.finish())) return rc;
  if (hinfo < 0)
    return fail(nullptr, GPX_E_HIP,
                "a stream parked on a device flag timed out (kernels serialised across streams? set GPX_CHAIN_FLAG=0)");
  *info = (hinfo == INT_MAX) ? 0 : hinfo;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_trsm(double* X, int64_t m, const double* L, int64_t nb) try {
  if (!X || !L || m <= 0 || nb <= 0 || m % 64 != 0 || nb % 64 != 0) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ldx = nb + LD_SKEW, ldl = nb + LD_SKEW;
  Dev<double> dX, dL, dL2, dW;
  Dev<int> dInfo;
  int hinfo = INT_MAX, rc;
  if ((rc = dX.alloc((size_t)m * ldx)) || (rc = dL.alloc((size_t)nb * ldl)) || (rc = dL2.alloc((size_t)nb * ldl)) ||
      (rc = dW.alloc((size_t)(nb / 64) * 4096)) || (rc = dInfo.alloc(16)))
    return rc;
  UCHK(hipMemcpy2DAsync(dX, (size_t)ldx * 8, X, (size_t)nb * 8, (size_t)nb * 8, (size_t)m, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpy2DAsync(dL, (size_t)ldl * 8, L, (size_t)nb * 8, (size_t)nb * 8, (size_t)nb, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpyAsync(dInfo, &hinfo, sizeof(int), hipMemcpyHostToDevice, sc.st));
  // inverse diagonal blocks of the GIVEN factor: potf2 of (L_qq L_qq^T) reproduces L_qq up to
  // rounding, so build them from a scratch copy of the products instead.
  std::vector<double> G((size_t)nb / 64 * 4096);
  for (int64_t q = 0; q < nb / 64; ++q)
    for (int i = 0; i < 64; ++i)
      for (int j = 0; j < 64; ++j) {
        double s = 0.0;
        for (int t = 0; t <= std::min(i, j); ++t)
          s += L[(q * 64 + i) * nb + q * 64 + t] * L[(q * 64 + j) * nb + q * 64 + t];
        G[(size_t)q * 4096 + i * 64 + j] = s;
      }
  UCHK(hipMemcpyAsync(dL2, G.data(), G.size() * 8, hipMemcpyHostToDevice, sc.st));
  UCHK(hipStreamSynchronize(sc.st));
  for (int64_t q = 0; q < nb / 64; ++q)
    launch_potf2_64<double>(dL2 + q * 4096, 64, dW + q * 4096, q * 64, dInfo, sc.st);
  launch_trsm_rlt<double>(dX, ldx, m, dL, ldl, dW, (int)nb, nullptr, 0, sc.st);
  if (take_launch_error()) return GPX_E_ARG;
  UCHK(hipMemcpy2DAsync(X, (size_t)nb * 8, dX, (size_t)ldx * 8, (size_t)nb * 8, (size_t)m, hipMemcpyDeviceToHost, sc.st));
  return sc.finish();
}
GPX_CATCH_ALL

int gpx_gemm_nt(double* C, int64_t m, int64_t n, const double* A, const double* B, int64_t k,
                int32_t lower) try {
  if (!C || !A || !B || m <= 0 || n <= 0 || k <= 0 || m % 64 || n % 64 || k % 16) return GPX_E_ARG;
  if (lower && m != n) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ldc = n + LD_SKEW, lda = k + LD_SKEW;
  const int tile = (m % 128 == 0 && n % 128 == 0) ? 128 : 64;
  Dev<double> dC, dA, dB;
  if (int rc; (rc = dC.alloc((size_t)m * ldc)) || (rc = dA.alloc((size_t)m * lda)) || (rc = dB.alloc((size_t)n * lda))) return rc;
  UCHK(hipMemcpy2DAsync(dC, (size_t)ldc * 8, C, (size_t)n * 8, (size_t)n * 8, (size_t)m, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpy2DAsync(dA, (size_t)lda * 8, A, (size_t)k * 8, (size_t)k * 8, (size_t)m, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpy2DAsync(dB, (size_t)lda * 8, B, (size_t)k * 8, (size_t)k * 8, (size_t)n, hipMemcpyHostToDevice, sc.st));
  // GPX_STRASSEN_MIN > 0: a rectangular product whose quadrants are at least that large takes one Strassen level
  const int64_t smin = sc.h.env.strassen_min;
  if (!lower && smin > 0 && std::min(m, n) >= 256 && std::min(m, n) / 256 * 128 >= smin) {
    Dev<double> dT;
    const int64_t ldt = k / 2 + LD_SKEW;
    if (int rc = dT.alloc(strassen_temp_elems(m, n, k, LD_SKEW))) return rc;
    // GPX_STRASSEN_MIN_TWO > 0: its seven products take a second level by the same rule
    Dev<double> dT2;
    StrassenL2<double> l2;
    l2.min2 = sc.h.env.strassen_min2;
    l2.elems = strassen_temp2_elems<double>(m, n, k);
    if (l2.min2 > 0 && l2.elems > 0) {
      if (int rc = dT2.alloc(l2.elems)) return rc;
      l2.buf = dT2;
    }
    strassen_nt<double>(dC, ldc, dA, lda, dB, lda, m, n, k, dT, dT + (m / 256 * 128) * ldt, ldt, sc.st, &l2);
    UCHK(hipStreamSynchronize(sc.st));  // (dT goes out of scope)
  } else {
    launch_gemm_nt_fixed<double>(tile, dC, ldc, dA, lda, dB, lda, m, n, k, lower, 0, sc.st);
  }
  UCHK(hipMemcpy2DAsync(C, (size_t)n * 8, dC, (size_t)ldc * 8, (size_t)n * 8, (size_t)m, hipMemcpyDeviceToHost, sc.st));
  return sc.finish();
}
GPX_CATCH_ALL

int gpx_mfma_probe(const double* A, const double* B, double* D) try { return mfma_probe_t(A, B, D, launch_mfma_probe); }
GPX_CATCH_ALL

int gpx_mfma_probe_f32(const float* A, const float* B, float* D) try { return mfma_probe_t(A, B, D, launch_mfma_probe_f32); }
GPX_CATCH_ALL

int gpx_path_distance(const double* paths, int64_t P, const double* cents, int64_t C, int32_t L,
                      double* D, int32_t mem_kind) try {
  if (!paths || !cents || !D || P <= 0 || C <= 0 || L <= 0 || L > 64) return GPX_E_ARG;
  if (bad_mem_kind(mem_kind)) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const bool host = mem_kind == GPX_MEM_HOST;
  Dev<double> dp, dc, dD;
  if (int rc = dc.alloc((size_t)C * L * 2)) return rc;
  UCHK(hipMemcpyAsync(dc, cents, (size_t)C * L * 16, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, sc.st));
  if (int rc; host && ((rc = dp.upload(paths, (size_t)P * L * 2, sc.st)) || (rc = dD.alloc((size_t)P * C)))) return rc;
  for (int64_t c0 = 0; c0 < C; c0 += 64)
    launch_path_distance(host ? dp : paths, P, dc + c0 * L * 2, (int)std::min<int64_t>(64, C - c0), L,
                         (host ? dD : D) + c0, C, sc.st);
  if (host) UCHK(hipMemcpyAsync(D, dD, (size_t)P * C * 8, hipMemcpyDeviceToHost, sc.st));
  return sc.finish();
}
GPX_CATCH_ALL

// The tile engine alone, operands resident: C (n x n) op= A (n x k) A'(n x k)^T on zero-filled device
// buffers, `iters` back-to-back launches after one warm-up; *ms = mean launch time.
extern "C++" {
template <typename T>
int gemm_bench_t(int64_t n, int64_t k, int32_t lower, int32_t mode, int32_t iters, double* ms) {
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ldc = n + ld_skew<T>(), lda = k + ld_skew<T>();
  Dev<T> dC, dA;
  float t = 0.f;
  if (int rc; (rc = dC.alloc((size_t)n * ldc)) || (rc = dA.alloc((size_t)2 * n * lda))) return rc;
  UCHK(hipMemsetAsync(dC, 0, (size_t)n * ldc * sizeof(T), sc.st));
  UCHK(hipMemsetAsync(dA, 0, (size_t)2 * n * lda * sizeof(T), sc.st));
  hipEvent_t e0 = next_event(&sc.h), e1 = next_event(&sc.h);  // (the Scratch handle's pool destroys them)
  if (!e0 || !e1) return fail(nullptr, GPX_E_HIP, "hipEventCreate failed");
  Dev<T> dT;  // mode 2: C -= A A'^T through strassen_nt (one launch = the whole level: ten sums, seven products)
  Dev<T> dT2;  // mode 3: the same with the second level in each of the seven, whatever the size of their quadrants
  StrassenL2<T> l2;
  const int64_t ldt = k / 2 + ld_skew<T>();
  if (mode >= 2) {
    if (int rc = dT.alloc(strassen_temp_elems(n, n, k, ld_skew<T>()))) return rc;
  }
  if (mode == 3) {
    l2.min2 = 128;
    l2.elems = strassen_temp2_elems<T>(n, n, k);
    if (int rc = dT2.alloc(l2.elems)) return rc;
    l2.buf = dT2;
  }
  auto once = [&] {
    if (mode >= 2)
      strassen_nt<T>(dC, ldc, dA, lda, dA + n * lda, lda, n, n, k, dT, dT + (n / 256 * 128) * ldt, ldt, sc.st, &l2);
    else
      launch_gemm_nt_fixed<T>(128, dC, ldc, dA, lda, dA + n * lda, lda, n, n, k, lower, mode, sc.st);
  };
  once();
  UCHK(hipEventRecord(e0, sc.st));
  for (int i = 0; i < iters; ++i) once();
  UCHK(hipEventRecord(e1, sc.st));
  if (int rc = sc.finish()) return rc;
  UCHK(hipEventElapsedTime(&t, e0, e1));
  *ms = (double)t / iters;
  return GPX_OK;
}
}  // extern "C++"

int gpx_debug_gemm_bench(int32_t dtype, int64_t n, int64_t k, int32_t lower, int32_t mode, int32_t iters,
                         double* ms_per_launch) try {
  if (!ms_per_launch || n <= 0 || n % 128 || k <= 0 || k % 32 || iters <= 0 || (lower != 0 && lower != 1) ||
      mode < 0 || mode > 3 || (mode == 2 && (lower != 0 || n % 256 || k % 64)) || (mode == 3 && (lower != 0 || n % 512 || k % 128)) ||
      n > 131072 || k > 32768)
    return GPX_E_ARG;
  if (dtype == GPX_F64) return gemm_bench_t<double>(n, k, lower, mode, iters, ms_per_launch);
  if (dtype == GPX_F32) return gemm_bench_t<float>(n, k, lower, mode, iters, ms_per_launch);
  return GPX_E_ARG;
}
GPX_CATCH_ALL

int gpx_debug_set_delay(uint64_t seed) {
  debug_set_delay(seed);
  return GPX_OK;
}

int gpx_debug_tile_map(int32_t kind, int64_t tm, int64_t tn, int32_t P, int32_t tpb, int32_t c, int32_t* out,
                       int64_t cap, int64_t* count) try {
  if (!out || !count || tm <= 0 || cap <= 0 || kind < 0 || kind > 2) return GPX_E_ARG;
  if (kind == 1 && (tn <= 0 || P <= 0 || tpb <= 0 || c < 0)) return GPX_E_ARG;
  BcMask bc{P, tpb};  // cyclic dealing in its old shorthand: row block of local block j = j P + c
  bc.gc0 = -c;
  const int64_t n = debug_tile_map(kind, tm, tn, bc, out, cap);
  if (n < 0) return GPX_E_ARG;
  *count = n;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_debug_stair_map(int64_t tm, int64_t tn, int32_t P, int32_t tpb, int32_t r, int32_t lbf, int32_t gc0,
                        int32_t snake, int32_t* out, int64_t cap, int64_t* count) try {
  if (!out || !count || tm <= 0 || tn <= 0 || cap <= 0 || P <= 0 || tpb <= 0 || r < 0 || r >= P || lbf < 0 || gc0 < 0)
    return GPX_E_ARG;
  BcMask bc{P, tpb};
  bc.r = r;
  bc.lbf = lbf;
  bc.gc0 = gc0;
  bc.snake = snake ? 1 : 0;
  if (bc.row_tile(0) < 0) return GPX_E_ARG;  // the first local row block must not lie left of the first column block
  const int64_t n = debug_tile_map(1, tm, tn, bc, out, cap);
  if (n < 0) return GPX_E_ARG;
  *count = n;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_debug_deal(int32_t P, int32_t snake, int64_t nblk, int32_t* owner, int64_t* local, int64_t* upto) try {
  if (P <= 0 || nblk <= 0 || !owner || !local || !upto) return GPX_E_ARG;
  const Deal dl{P, snake ? 1 : 0};
  for (int64_t g = 0; g < nblk; ++g) {
    owner[g] = dl.owner(g);
    local[g] = dl.local(g);
    if (dl.global(owner[g], local[g]) != g) return GPX_E_ARG;  // the two directions must agree
    for (int r = 0; r < P; ++r) upto[g * P + r] = dl.upto(g, r);
  }
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_debug_env(char* buf, int32_t n) try {
  EnvKnobs env;  // a fresh snapshot of every moment; the create entries as gpx_create resolves them
  for (EnvAt at : {EnvAt::create, EnvAt::call, EnvAt::process}) env_read(env, at);
  return env_print(env, buf, n);
}
GPX_CATCH_ALL

int gpx_microbench(double* mfma_tflops, double* copy_gbs) try {
  if (!mfma_tflops || !copy_gbs) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  Dev<double> sink, src, dst;
  const int64_t count = (int64_t)1 << 28;  // 2 GiB per buffer
  const int64_t skew = 0;  // (round 3: a skewed destination measured slower than an aligned one: tools/copy_bw.hip)
  // 65536 iterations, ~0.23 s: long enough to be past the clock ramp (a 14 ms loop read 75 TF, the sustained rate is
  // 77.8); GPX_MICROBENCH_ITERS overrides
  const int iters = sc.h.env.microbench_iters;
  const int blocks = 256 * 8;
  float ms = 0.f;
  if (int rc; (rc = sink.alloc(8)) || (rc = src.alloc((size_t)count)) || (rc = dst.alloc((size_t)(count + skew)))) return rc;
  hipEvent_t e0 = next_event(&sc.h), e1 = next_event(&sc.h);  // (the Scratch handle's pool destroys them)
  if (!e0 || !e1) return fail(nullptr, GPX_E_HIP, "hipEventCreate failed");
  UCHK(hipMemsetAsync(src, 0x11, (size_t)count * 8, sc.st));
  launch_mfma_loop(sink, 64, blocks, sc.st);  // warm-up
  UCHK(hipEventRecord(e0, sc.st));
  launch_mfma_loop(sink, iters, blocks, sc.st);
  UCHK(hipEventRecord(e1, sc.st));
  UCHK(hipEventSynchronize(e1));
  UCHK(hipEventElapsedTime(&ms, e0, e1));
  *mfma_tflops = (double)blocks * 4 * (double)iters * 16 * 2048.0 / (ms * 1e-3) / 1e12;
  for (int r = 0; r < 4; ++r) launch_copy(src, dst + skew, count, sc.st);  // warm-up
  UCHK(hipEventRecord(e0, sc.st));
  for (int r = 0; r < 20; ++r) launch_copy(src, dst + skew, count, sc.st);
  UCHK(hipEventRecord(e1, sc.st));
  UCHK(hipEventSynchronize(e1));
  UCHK(hipEventElapsedTime(&ms, e0, e1));
  *copy_gbs = 20.0 * 2.0 * (double)count * 8.0 / (ms * 1e-3) / 1e9;
  UCHK(hipGetLastError());
  return GPX_OK;
}
GPX_CATCH_ALL

#include "gpx_sparse.inc"

}  // extern "C"
