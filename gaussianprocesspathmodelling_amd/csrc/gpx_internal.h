// gpx_internal.h — launcher prototypes shared by the kernel TUs and the C-ABI TU.
// All launchers enqueue on `st` and never synchronise.  Every launcher is a template on
// the element type T, explicitly instantiated for double and float in its .hip file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpx {

constexpr int KB = 64;      // innermost Cholesky block (one-workgroup POTF2 + inverse)
constexpr int TILE = 128;   // trailing-update tile; every padded dimension is a multiple
constexpr int MAX_D = 32;   // max input dimension d (the kernels stage points in LDS arrays of this width)
constexpr int MAX_HESS_D = 8;  // ... of the posterior second derivatives (gpx_hess.hip): d (d + 1) / 2 row blocks per point
constexpr int hess_pairs(int d) { return d * (d + 1) / 2; }  // the pairs (i, j), i <= j, row-major
// row blocks with a prior of their own in launch_grad_norms: value + d of the gradient, the pairs of the Hessian
constexpr int PRIOR_SLOTS = hess_pairs(MAX_HESS_D) > MAX_D + 1 ? hess_pairs(MAX_HESS_D) : MAX_D + 1;
// Leading-dimension skew against power-of-two strides: ONE 128-byte line, so that every row of
// every matrix starts on a 128-byte boundary (hipMalloc bases are 256-byte aligned; all padded
// dimensions are multiples of 64 elements).  trsm_rlt_kernel DEPENDS on this: it round-trips a
// 64x64 tile through global memory inside one workgroup — L2-side atomics, then LDS-DMA loads
// through the CU's L1 — which is only coherent because no 128-byte line of the tile can already
// sit in that L1: lines never straddle a tile edge (this alignment) and the earlier loads of the
// walk touch only columns left of the tile.  Keep skew * sizeof(T) a multiple of 128.
template <typename T>
constexpr int ld_skew() {
  return 128 / (int)sizeof(T);
}
constexpr int LD_SKEW = ld_skew<double>();  // fp64 buffers (16 elements)
static_assert(ld_skew<double>() * sizeof(double) % 128 == 0 && ld_skew<float>() * sizeof(float) % 128 == 0,
              "row starts must stay 128-byte aligned (trsm_rlt_kernel's L1 invariant)");

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// Dealing of the row blocks of the Gram matrix over the P ranks of a shard (csrc/gpx_shard.inc).
//   cyclic (rounds 1-3): block g on rank g mod P — rank P-1 holds the lowest block of every round of P, and a row block's
//     share of every trailing update grows with its index: the last rank carries 8.4 % more than the mean at P = 8 /
//     nb = 512 (N = 65536), 17 % at nb = 1024, in EVERY panel (the ranks meet at each panel, so that is the fit's time).
//   snake (round 4, default): rounds of 2 P blocks dealt 0, 1, ..., P-1, P-1, ..., 1, 0 — every rank gets one block of the
//     ascending and one of the descending half, the sums agree: 0.65 % / 2.6 % in the same cases (tools/scaling_model.py).
// Everything that depends on the dealing asks this struct (host and device).
struct Deal {
  int P, snake;
  __host__ __device__ __forceinline__ int owner(int64_t g) const {
    if (!snake) return (int)(g % P);
    const int pos = (int)(g % (2 * P));
    return pos < P ? pos : 2 * P - 1 - pos;
  }
  __host__ __device__ __forceinline__ int64_t local(int64_t g) const {  // index of block g among its owner's blocks
    if (!snake) return g / P;
    return 2 * (g / (2 * P)) + ((g % (2 * P)) >= P ? 1 : 0);
  }
  __host__ __device__ __forceinline__ int64_t global(int r, int64_t lb) const {  // block number lb of rank r
    if (!snake) return lb * P + r;
    return (lb >> 1) * (2 * P) + ((lb & 1) ? 2 * P - 1 - r : r);
  }
  __host__ __device__ __forceinline__ int64_t upto(int64_t p, int r) const {  // blocks of rank r with index <= p (p >= -1)
    if (!snake) return p >= r ? (p - r) / P + 1 : 0;
    const int64_t n = p + 1, c = n / (2 * P), rem = n % (2 * P);
    return 2 * c + (rem > r ? 1 : 0) + (rem > 2 * P - 1 - r ? 1 : 0);
  }
};

struct BcMask {   // row map of the sharded trailing update (P == 0: unused)
  int P, tpb;     // ranks, tiles per block
  int r = 0, lbf = 0, gc0 = 0, snake = 0;  // local tile row ti belongs to row block Deal.global(r, lbf + ti / tpb) of the matrix,
                                           // tile column 0 to block gc0: row tile (that block - gc0) * tpb + ti % tpb of the launch
  // B operand read straight from the ALL-GATHERED panel (round 4; piece == 0: B is contiguous): rank-major pieces of
  // `piece` rows, every rank's own blocks beyond panel p in order.  Tile column tj is block g = gc0 + tj / tpb of the
  // matrix: block number local(g) - upto(p, owner(g)) of the piece of rank owner(g).
  int p = 0;
  int64_t piece = 0;
  __host__ __device__ __forceinline__ Deal deal() const { return Deal{P, snake}; }
  __host__ __device__ __forceinline__ int row_tile(int ti) const {  // launch-relative tile row of local tile row ti
    return (int)(deal().global(r, lbf + ti / tpb) - gc0) * tpb + ti % tpb;
  }
};

// first row of B's tile column tj (BT rows per tile; tpb counts BT-tiles per block)
template <int BT>
__host__ __device__ __forceinline__ int64_t bc_brow(const BcMask& bc, int tj) {
  if (bc.piece == 0) return (int64_t)tj * BT;
  const Deal dl = bc.deal();
  const int64_t g = bc.gc0 + tj / bc.tpb;
  const int rr = dl.owner(g);
  return (int64_t)rr * bc.piece + ((dl.local(g) - dl.upto(bc.p, rr)) * bc.tpb + tj % bc.tpb) * BT;
}


// ---- kernel-matrix build (gpx_kbuild.hip) ---------------------------------------
// Xs = X / lengthscale (per-dimension), rows >= n zero-filled up to npad.
template <typename T>
void launch_scale_points(const T* X, int64_t n, int64_t npad, int d, const double* ls, int n_ls, T* Xs,
                         hipStream_t st);
// Lower tiles (64x64) of K[npad, npad] (ld): sf2*k(xi,xj), + diag_add on the diagonal;
// padded rows/cols (>= n) become identity rows.
template <typename T>
void launch_kbuild_sym(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2,
                       double diag_add, T* K, int64_t ld, hipStream_t st);
// The same with per-observation noise: + (sn2 w[i] + jitter) on the diagonal of row i < n, w (n) on the device
// (w = 1 everywhere: the bits of launch_kbuild_sym with diag_add = sn2 + jitter).
template <typename T>
void launch_kbuild_sym_w(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const T* w, double sn2,
                         double jitter, T* K, int64_t ld, hipStream_t st);
// Rectangular K*[mpad, npad] (ld) = sf2*k(As_i, Bs_j); rows >= m or cols >= n are zero.
template <typename T>
void launch_kbuild_cross(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n,
                         int64_t npad, int d, double sf2, T* K, int64_t ld, hipStream_t st);
// Observations with kinds (gpx_cov.h: kind -1 a value of f, j a value of d f / d x_j; the arrays are readable up to the
// padded sizes and hold -1 there; ls (n_ls = 1 or d) on the device; differentiable families only).
// diag[i] = (kind[i] < 0 ? sn2 : sn2_deriv) (w ? w[i] : 1) + jitter for i < n, formed in fp64 and rounded once
template <typename T>
void launch_kinds_diag(const int32_t* kind, const T* w, int64_t n, double sn2, double sn2_deriv, double jitter, T* diag,
                       hipStream_t st);
// launch_kbuild_sym over such observations: cov::element per pair, + diag[i] on the diagonal of row i < n
template <typename T>
void launch_kbuild_sym_k(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const int32_t* kind,
                         const double* ls, int n_ls, const T* diag, T* K, int64_t ld, hipStream_t st);
// launch_kbuild_cross with value rows (As) against such observations as columns (Bs, kind_b)
template <typename T>
void launch_kbuild_cross_k(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d,
                           double sf2, const int32_t* kind_b, const double* ls, int n_ls, T* K, int64_t ld, hipStream_t st);
// ... with kinds on the rows too (kind_a: readable up to mpad, -1 beyond m): the left part of appended rows
// (append_restart), gpx_kernel_mixed_matrix
template <typename T>
void launch_kbuild_cross_kk(int kernel, const T* As, const int32_t* kind_a, int64_t m, int64_t mpad, const T* Bs,
                            const int32_t* kind_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                            T* K, int64_t ld, hipStream_t st);

// Observations with path ids (id >= 0 names the path of an observation, -1 none; the arrays are readable up
// to the padded sizes and hold -1 there): + sg2 k(x, x'; l_path) where the ids of a pair match.  q (d entries, device) =
// (l_c / l_path,c)^2: the scaled points' differences times sqrt(q_c) are the path kernel's.  diag as launch_kinds_diag's.
template <typename T>
void launch_kbuild_sym_g(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const int32_t* group,
                         const double* q, double sg2, const T* diag, T* K, int64_t ld, hipStream_t st);
// the rectangular build over two sets of such observations (gpx_kernel_path_matrix)
template <typename T>
void launch_kbuild_cross_g(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                           const int32_t* group_b, int64_t n, int64_t npad, int d, double sf2, const double* q, double sg2,
                           T* K, int64_t ld, hipStream_t st);

// ---- dense blocks (gpx_blas.hip) ---------------------------------------------------
// How a launch goes out — the last argument of the launchers below that have variants (default: the plain kernels).
// Nothing is remembered between launches: what a launch gets is what its call site says.
struct ReserveRing {  // [cap][8] device counters, owned by the factorisation that zeroed them (gemm_nt_resv_kernel in gpx_blas.hip)
  unsigned* ctr = nullptr;
  int cap = 0, used = 0;  // launches beyond cap are the plain kernels
  int form = 1;           // grid of the self-reserving launches: 1 turnover, 0 persistent (GPX_RESV_FORM)
};
struct LaunchMode {
  // The caller knows nothing large runs beside this launch: the 64-tile launches (launch_gemm_nt with an under-filled
  // 128-grid, launch_trsm_rlt / launch_inv_extend with few slabs) then stage several k-steps per barrier — 64 or 128 KB
  // of LDS per workgroup instead of 32 — which shortens every latency-bound K walk when the GPU is otherwise idle and
  // must NOT be used beside a large trailing update (see gpx_blas.hip).
  bool latency = false;
  // > 0 (round 4), with a ring: the products of launch_gemm_nt go out as persistent grids whose workgroups leave resv_k
  // CUs per XCD alone (they exit at once there) and take their tiles from the next 8 counters of *ring.
  int resv_k = 0;
  // with a ring, the chain's side (GPX_RESV_CHAIN): != 0 — launch_potf2_128 asks for 130 KB of LDS; > 1 — the narrow slab
  // launches too (launch_trsm_rlt, <= 16 slabs) ask for a whole CU's LDS, so that they land on the CUs the update leaves alone.
  int resv_chain = 0;
  ReserveRing* ring = nullptr;  // null: resv_k and resv_chain count for nothing
};
// In-place Cholesky of one 64x64 diagonal block (lower) + its inverse Winv (64x64,
// row-major, upper part zero).  gidx0 = global index of the block's first row (info).
template <typename T>
void launch_potf2_64(T* A, int64_t lda, T* Winv, int64_t gidx0, int* info, hipStream_t st, unsigned* flag = nullptr,
                     unsigned flag_val = 0);
// The same for a 128x128 diagonal tile in one launch: L11, L21, L22 in place and the TWO 64x64 inverses
// of its diagonal blocks (Winv[0..4096), Winv[4096..8192)); the 64 x 64 block above the diagonal is
// not touched.
// flag != null (both kernels): *flag = flag_val after a device-scope release of the results — what a stream parked
// on launch_wait_counter(flag, flag_val) waits for.
template <typename T>
void launch_potf2_128(T* A, int64_t lda, T* Winv, int64_t gidx0, int* info, hipStream_t st, unsigned* flag = nullptr,
                      unsigned flag_val = 0, LaunchMode lm = {});
// X (rows x nb, ldx) <- X * L^-T; L (nb x nb, ldl) lower, Winv = nb/64 inverse diag
// blocks.  rows, nb multiples of 64.  If P != null the result is also written to the
// compact panel P (rows x nb, ldp).
template <typename T>
void launch_trsm_rlt(T* X, int64_t ldx, int64_t rows, const T* L, int64_t ldl, const T* Winv, int nb,
                     T* P, int64_t ldp, hipStream_t st, LaunchMode lm = {});
// Building the explicit inverse of a diagonal block L (nbw x nbw, ldl) next to its
// factorisation: U (ldu) holds (L^-1)^T column blocks [0, q0) already and the identity elsewhere;
// this solves column blocks [q0, q1) of U for row blocks 0..q1-1 and writes them transposed into
// row blocks [q0, q1) of W = L^-1 (ldw).  Needs the 64-block inverses and rows of L up to q1.
template <typename T>
void launch_inv_extend(T* U, int64_t ldu, const T* L, int64_t ldl, const T* Winv, int q0, int q1, T* W,
                       int64_t ldw, hipStream_t st, int phase = 0,  // 0 whole, 1 "pre" (left of block q0 only), 2 "post"
                       LaunchMode lm = {});
// 1 if a launcher CALLED BY THIS HOST THREAD since the last call refused misaligned operands (and launched nothing);
// clears the flag.  Thread-local: an API call enqueues and checks on one thread, so a handle only ever sees its own
// launches' errors (distinct handles on distinct threads: include/gpx.h)
int take_launch_error();
// X (rows x nb, ldx) <- X * L^-1 (right, lower, no-transpose; descending blocks).
template <typename T>
void launch_trsm_rln(T* X, int64_t ldx, int64_t rows, const T* L, int64_t ldl, const T* Winv, int nb,
                     hipStream_t st);
// C (m x n, ldc) op= A (m x k, lda) * B (n x k, ldb)^T.
//   mode 0: C -= A B^T      mode 1: C = A B^T
//   lower 0: every tile;  1: lower triangle (m == n), triangular super-tile order;
//         2: rectangle masked to tile_col <= tile_row (look-ahead strip);
//         4: every tile, B lower triangular (k limited to the tile's own column range).
//   tile = 128 (m,n multiples of 128) or 64 (multiples of 64); k multiple of 64.
template <typename T>
void launch_gemm_nt(int tile, T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb,
                    int64_t m, int64_t n, int64_t k, int lower, int mode, hipStream_t st, LaunchMode lm = {});
// the tile size launch_gemm_nt really uses for (tile, m, n, lower): 64 when the 128-grid is under-filled
int gemm_nt_tile(int tile, int64_t m, int64_t n, int lower);
// the same with the tile size taken literally (unit-test entry point, engine benchmark)
template <typename T>
void launch_gemm_nt_fixed(int tile, T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb,
                    int64_t m, int64_t n, int64_t k, int lower, int mode, hipStream_t st, LaunchMode lm = {});
// C (m x n) -= A B^T with one Strassen level on the part with m, n multiples of 256 (gpx_blas.hip: the order of its
// launches, and why the result is repeatable bit for bit); m, n multiples of 64, k a multiple of the k-step.  TA | TB:
// strassen_temp_elems(m, n, k, skew) elements, TB = TA + (m / 256 * 128) * ldt, ldt = k / 2 + skew.  Null temporaries,
// or a shape with nothing for the level: the classical launch.  Returns the flops executed.
// l2 (optional): the seven products take a second level where their own quadrants are at least l2->min2 rows and columns
// (GPX_STRASSEN_MIN_TWO) and l2->buf holds strassen_temp2_elems<T>(m, n, k) of l2->elems elements; otherwise — null, min2 = 0,
// no or too small a buffer — exactly the one-level launches.  *two_levels (optional) says whether it ran.
// lm reaches the classical launches only (the no-level fallback and the three peeled parts), not the level's products.
size_t strassen_temp_elems(int64_t m, int64_t n, int64_t k, int skew);
template <typename T>
size_t strassen_temp2_elems(int64_t m, int64_t n, int64_t k);
template <typename T>
struct StrassenL2 {
  int64_t min2 = 0;
  T* buf = nullptr;
  size_t elems = 0;
};
template <typename T>
double strassen_nt(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t m, int64_t n,
                   int64_t k, T* TA, T* TB, int64_t ldt, hipStream_t st, const StrassenL2<T>* l2 = nullptr,
                   bool* two_levels = nullptr, LaunchMode lm = {});
// The whole trailing update of a panel in one launch: C (n x n, 128-tiles, lower) -= P P^T (P: n x k, ldp)
// with the first ns columns (the strip that becomes the next panel) enumerated first; every strip slot
// adds 1 to *ctr once its tile is released at device scope.  Returns the number of strip slots.
template <typename T>
unsigned launch_gemm_nt_fused(T* C, int64_t ldc, const T* P, int64_t ldp, int64_t n, int64_t ns, int64_t k,
                              unsigned* ctr, hipStream_t st);
// One wave that returns once *ctr >= target (polled at device scope, ~2 us period).  Bounded: after
// ~15 s it gives up, sets *info = INT_MIN (the caller reports it) and returns — never a hung queue.
void launch_wait_counter(const unsigned* ctr, unsigned target, int* info, hipStream_t st);
// the two halves of the hand-over self-test: *seen = 1 iff the waiting kernel saw *flag != 0 within max_polls x ~2 us
void launch_flag_probe_wait(const unsigned* flag, unsigned* seen, unsigned max_polls, hipStream_t st);
void launch_flag_probe_set(unsigned* flag, hipStream_t st);
// Sharded trailing update: C (m local rows x n, 128-tiles) -= A B^T restricted to tiles with
//   tile_col <= bc.row_tile(tile_row)   (the row blocks' places in the dealing: Deal / BcMask above);
//   bc.piece > 0: B is the all-gathered panel bc.p in rank-major pieces (bc_brow).
// test hook: random spin kernels in front of launches (gpx_debug_set_delay; gpx_misc.hip)
void debug_set_delay(uint64_t seed);
void debug_delay(hipStream_t st);
// C (m x n) = A (m x k) B(n x k)^T for skinny C with a long contraction (m, n multiples of 64): S
// splits of k into partial tiles part[s] (m x ldp each, back to back), summed in split order
int splitk_splits(int64_t k);  // depends on k only: batching the columns must not change the bits
template <typename T>
void launch_gemm_nt_splitk(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t m,
                           int64_t n, int64_t k, int S, T* part, int64_t ldp, hipStream_t st);
template <typename T>
void launch_gemm_nt_bc(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t m,
                       int64_t n, int64_t k, const BcMask& bc, hipStream_t st);
// C (m x n, ldc) -= A (m x k, lda) * B (k x n, ldb); 64x64 tiles.
template <typename T>
void launch_gemm_nn(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t m,
                    int64_t n, int64_t k, hipStream_t st);

// ---- small helpers (gpx_misc.hip) ------------------------------------------------------
// YT (R x npad, ld) <- transpose of y (n x k) into rows [0,k), everything else zero.
template <typename T>
void launch_pack_rhs(const T* y, int64_t n, int k, T* YT, int64_t ld, int64_t npad, int R,
                     hipStream_t st);
// out (n x k) <- rows [0,k) of YT (R x *, ld), scaled by `scale`.
template <typename T>
void launch_unpack_rhs(const T* YT, int64_t ld, int64_t n, int k, double scale, T* out, hipStream_t st);
// var[i] = sf2 - sum_j VT[i, j]^2, i < m  (accumulated in fp64).  ids != null (device, m entries): the prior of a row i with
// ids[i] >= 0 is sf2 + sg2, summed in fp64.
template <typename T>
void launch_var_rows(const T* VT, int64_t ld, int64_t m, int64_t ncols, double sf2, T* var,
                     hipStream_t st, const int32_t* ids = nullptr, double sg2 = 0.0);
// dst (rows x cols, ldd) = src (rows x cols, lds), streaming; cols * sizeof(T) multiple of 16, 16-byte aligned rows
template <typename T>
void launch_copy2d(T* dst, int64_t ldd, const T* src, int64_t lds, int64_t rows, int64_t cols, hipStream_t st);
// lower triangle of dst (n x n, ldd) = that of src (lds), whole 128-tiles (the diagonal tiles included); n a multiple of
// 128, rows 16-byte aligned.  Half the traffic of launch_copy2d on the square: moving a factor into a larger buffer.
template <typename T>
void launch_copy_lower(T* dst, int64_t ldd, const T* src, int64_t lds, int64_t n, hipStream_t st);
// A[i][i] = 1 for i < n
template <typename T>
void launch_set_diag_one_t(T* A, int64_t lda, int64_t n, hipStream_t st);
// out[0] = 2 * sum_{i<n} log(A[i, i])  (fp64 accumulation and result).
template <typename T>
void launch_logdet(const T* A, int64_t lda, int64_t n, double* out, hipStream_t st);
void launch_mfma_probe(const double* A, const double* B, double* D, hipStream_t st);
void launch_mfma_probe_f32(const float* A, const float* B, float* D, hipStream_t st);
void launch_mfma_loop(double* sink, int iters, int blocks, hipStream_t st);
int64_t debug_tile_map(int kind, int64_t tm, int64_t tn, const BcMask& bc, int32_t* out,
                       int64_t cap);
void launch_copy(const double* src, double* dst, int64_t count, hipStream_t st);

// ---- log-marginal-likelihood gradient (gpx_grad.hip, fp64) -------------------------------------
// theta = (lengthscale[0..n_ls), sf2, sn2), ntheta = n_ls + 2, ard = n_ls > 1.  Both passes write
// one partial per (tile slot, theta); reduce_partials sums them in a fixed order.
int64_t kinv_trace_slots(int64_t npad);  // slots of the 128-tile triangular map
int64_t alpha_quad_slots(int64_t npad);  // 64-tiles of the lower triangle
void launch_set_diag_one(double* A, int64_t lda, int64_t n, hipStream_t st);
// part[slot][t] = sum over the tile of (ZT ZT^T)_ij (dK/dlog theta_t)_ij, ZT = L^-T (npad x npad, ld);
// rank `rank` of P covers every P-th octet of 64-slot groups (P = 1: all of them)
void launch_kinv_trace(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                       int ard, double sf2, double sn2, double* part, int ntheta, int P, int rank, hipStream_t st,
                       const double* wv = nullptr);  // wv (n): the noise entry sums w_i (K^-1)_ii (null: w = 1)
// the same for a factor that is only held distributed: ZTc (npad rows x ncols, ldc) = the columns of L^-T
// that belong to this rank's row blocks of L (height nb, block-cyclic over P ranks, local order); every
// rank visits every tile and contracts over its own columns: the ranks' partial sums add up
void launch_kinv_trace_cols(int kernel, const double* ZTc, int64_t ldc, int64_t npad, int64_t n, const double* Xs,
                            int d, int ard, double sf2, double sn2, double* part, int ntheta, int nb, int P, int rank,
                            int64_t ncols, int snake, hipStream_t st);
// part[slot][t] = sum over the tile of (sum_c alpha_ic alpha_jc) (dK/dlog theta_t)_ij, alphaT (k x npad, ld)
void launch_alpha_quad(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                       const double* Xs, int d, int ard, double sf2, double sn2, double* part, int ntheta,
                       hipStream_t st, const double* wv = nullptr);  // wv (n): the noise entry sums w_i sum_c alpha_ic^2
// Both passes for a fit with derivative observations (differentiable families; kind readable up to npad, -1 there; ls
// (n_ls) on the device): theta = (lengthscale[0..n_ls), sf2, sn2, sn2_deriv), ntheta = n_ls + 3; one device
void launch_kinv_trace_kinds(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                             int ard, double sf2, double sn2, double sn2_deriv, const int32_t* kind, const double* ls,
                             int n_ls, double* part, int ntheta, hipStream_t st, const double* wv = nullptr);
void launch_alpha_quad_kinds(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                             const double* Xs, int d, int ard, double sf2, double sn2, double sn2_deriv,
                             const int32_t* kind, const double* ls, int n_ls, double* part, int ntheta, hipStream_t st,
                             const double* wv = nullptr);
// Both passes for a fit with path ids (every family; group: the ids, readable up to npad, -1 there; q (d entries) on the
// device): theta = (lengthscale[0..n_ls), sf2, sn2, sg2, l_path[0..n_lsp)), ntheta = n_ls + 3 + n_lsp; one device
void launch_kinv_trace_groups(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                              int ard, double sf2, double sn2, double sg2, const int32_t* group, const double* q,
                              int n_lsp, double* part, int ntheta, hipStream_t st, const double* wv = nullptr);
void launch_alpha_quad_groups(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                              const double* Xs, int d, int ard, double sf2, double sn2, double sg2, const int32_t* group,
                              const double* q, int n_lsp, double* part, int ntheta, hipStream_t st,
                              const double* wv = nullptr);
// G (1 + n_lsp blocks of napad x ld): [0] the within-path term m sg2 k(r_p) of ids ga at As against gb at Bs, [1 + c] its
// derivative by log l_path,c (cov::path_dtheta); scaled points, q (d entries) on the device
void launch_path_dtheta_matrix(int kernel, const double* As, const int32_t* ga, int64_t na, int64_t napad, const double* Bs,
                               const int32_t* gb, int64_t nb, int d, const double* q, int n_lsp, double sg2, double* G,
                               int64_t ld, hipStream_t st);
// G (n_ls blocks of napad x ld)[c][i][j] = d cov(obs of kind ka[i] at As_i, obs of kind kb[j] at Bs_j) / d log l_c, i < na,
// j < nb (cov::element_dl); scaled points, ka / kb null: values; a kind >= 0 needs a differentiable family
void launch_dl_matrix(int kernel, const double* As, const int32_t* ka, int64_t na, int64_t napad, const double* Bs,
                      const int32_t* kb, int64_t nb, int d, const double* ls, int n_ls, double sf2, double* G, int64_t ld,
                      hipStream_t st);
void launch_reduce_partials(const double* part, int64_t ntile, int ntheta, double scale, double* out,
                            hipStream_t st);
// out[0] = sum_i sum_c y[i*k + c] * alphaT[c*ld + i]
void launch_dot_rhs(const double* y, const double* alphaT, int64_t ld, int64_t n, int k, double* out,
                    hipStream_t st);

// ---- mixed precision (gpx_mixed.hip) ------------------------------------------------------------
// outT[c][i] = (y ? y[i*k+c] : 0) + sign * (sum_j sf2 k(a_i, b_j) alphaT[c][j] + diag * alphaT[c][i]), i < m;
// fp64, matrix-free (K regenerated from the scaled points As (mpad x d) / Bs (npad x d)); k <= 8;
// alphaT (k x lda) zero beyond the valid columns.
void launch_kmatvec(int kernel, const double* As, int64_t m, int64_t mpad, const double* Bs, int64_t npad, int d,
                    double sf2, double diag, const double* y, const double* alphaT, int64_t lda, int k,
                    double sign, double* outT, int64_t ldo, hipStream_t st, const double* wv = nullptr, double wsn2 = 0.0,
                    double wjit = 0.0);  // wv (m) != null: row i's diagonal term is (wsn2 wv[i] + wjit) alphaT[c][i], not diag
void launch_f64_to_f32(const double* in, float* out, int64_t count, hipStream_t st);
void launch_f32_to_f64(const float* in, double* out, int64_t count, hipStream_t st);
// dst (R x ldd, float) = rows [0, rows) x [0, n) of src (double), zero elsewhere up to npad
void launch_rows_f64_to_f32(const double* src, int64_t lds, float* dst, int64_t ldd, int rows, int R, int64_t n,
                            int64_t npad, hipStream_t st);
// dst (rows x ldd, double) (+)= src (float) on [0, n), (acc ? unchanged : 0) beyond
void launch_rows_add_f32_to_f64(const float* src, int64_t lds, double* dst, int64_t ldd, int rows, int64_t n,
                                int64_t npad, int acc, hipStream_t st);
void launch_rows_sumsq(const double* src, int64_t lds, int rows, int64_t n, double* out, hipStream_t st);
// few right-hand sides (k <= 8): out[c][i] (= | -=) sum_j M[i][j] v[c][j]  (cols: M[j][i]); nj <= 1024, cols: ni % 128 == 0
template <typename T>
void launch_few_product(bool cols, bool assign, T* out, int64_t ldo, const T* M, int64_t ldm, int64_t ni, int nj,
                        const T* v, int64_t ldv, int k, hipStream_t st);

// ---- path distance (gpx_paths.hip) -----------------------------------------------------------
// D (P, ldd)[p][c] = sum_i ||paths[p][i] - cents[c][i]||, paths (P, L, 2), cents (C <= 64, L <= 64, 2)
void launch_path_distance(const double* paths, int64_t P, const double* cents, int C, int L, double* D,
                          int64_t ldd, hipStream_t st);

// ---- joint posterior (gpx_posterior.hip) -----------------------------------------------------
// Z^T rows [r0, r0 + rows_pad) (ld) of a call with `total` = S k rows (row r = s k + c) and M columns (mpad, a multiple of
// 64): element (r, m) = normal number (s M + m) k + c of the Philox stream `seed` (z == null; include/gpx.h specifies it),
// or z[(s M + m) k + c] of the caller's (S, M, k) array; zero beyond `total` rows and M columns
template <typename T>
void launch_normals(T* ZT, int64_t ld, int64_t r0, int64_t rows_pad, int64_t total, int64_t M, int64_t mpad, int k,
                    uint64_t seed, const T* z, hipStream_t st);
// A (n x n, lda; n multiple of 64): strict upper triangle <- transpose of the strict lower one (zero_upper: <- 0)
template <typename T>
void launch_mirror_lower(T* A, int64_t lda, int64_t n, int zero_upper, hipStream_t st);
// out[(s M + m) k + c] = mean[m k + c] + ST[r - r0][m] (lds) for the rows r = s k + c in [r0, r0 + rows) (whole samples)
template <typename T>
void launch_sample_epilogue(const T* ST, int64_t lds, int64_t r0, int64_t rows, const T* mean, int64_t M, int k, T* out,
                            hipStream_t st);

// ---- posterior gradient (gpx_deriv.hip) --------------------------------------------------------
// Row blocks of V (each mpad rows, ld; mpad a multiple of 64): [sf2 k(As, Bs) if with_value — launch_kbuild_cross's
// numbers] then d k(As, Bs) / d As_j for j < d; zero beyond m rows / n columns.  ls (n_ls = 1 or d) on the device.
// kind_b != null: the columns are observations with kinds (as launch_kbuild_cross_k's).
template <typename T>
void launch_kgrad_build(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d,
                        double sf2, const double* ls, int n_ls, int with_value, T* V, int64_t ld, hipStream_t st,
                        const int32_t* kind_b = nullptr);
// The same over rows and columns with path ids (launch_kbuild_cross_g's arguments): a same-path pair gets the value and the
// derivative of sg2 k(., .; l_path) as well; a tile that can hold no such pair gives launch_kgrad_build's numbers.
template <typename T>
void launch_kgrad_build_g(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                          const int32_t* group_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                          const double* q, double sg2, int with_value, T* V, int64_t ld, hipStream_t st);
// grid of the matrix-free product: KC targets per workgroup, S splits of `chunk` training columns; the partial buffer
// holds S * k * d * round_up(M, 64) elements
void kgrad_matvec_shape(int64_t M, int64_t npad, int d, int k, int* KC, int* S, int64_t* chunk);
// dmean (M, d, k)[m][j][c] = sum_n d k(As_m, Bs_n) / d As_mj alphaT[c][n], matrix-free (neither K* nor its derivative
// is stored); As readable up to round_up(M, 64) rows, alphaT (k x lda) zero beyond the valid columns
template <typename T>
void launch_kgrad_matvec(int kernel, const T* As, int64_t M, const T* Bs, int64_t npad, int d, double sf2,
                         const T* alphaT, int64_t lda, int k, const double* ls, int n_ls, T* part, T* dmean,
                         hipStream_t st);
// out[b mp + i] = prior[b] - sum_{j < ncols} V[b mp + i][j]^2 for i < mv, b < nblk (<= PRIOR_SLOTS; prior on the host).
// ids != null (device, mv entries): the prior of a row i with ids[i] >= 0 is prior[b] + prior_path[b], summed in fp64
template <typename T>
void launch_grad_norms(const T* V, int64_t ld, int64_t mp, int64_t mv, int nblk, int64_t ncols, const double* prior,
                       T* out, hipStream_t st, const int32_t* ids = nullptr, const double* prior_path = nullptr);
// one batch of the variance route: column b mp + i of MT (RHS rows = targets) and entry b mp + i of VN, i < mv, into
// mean (mv, k) / var (mv) (row block 0 when with_value) and dmean (mv, d, k) / dvar (mv, d); mean, var, dvar may be null
template <typename T>
void launch_grad_unpack(const T* MT, int64_t ldm, const T* VN, int64_t mp, int64_t mv, int nblk, int d, int k,
                        int with_value, T* mean, T* var, T* dmean, T* dvar, hipStream_t st);

// ---- posterior second derivatives (gpx_hess.hip) -----------------------------------------------
// hess_pairs(d) row blocks of V (each mpad rows, ld; mpad a multiple of 64), block (i, j), i <= j, row-major =
// d^2 k(As, Bs) / d As_i d As_j; zero beyond m rows / n columns.  RBF and Matern-5/2, d <= MAX_HESS_D (nothing is launched
// otherwise).  group_a == null, side_b == null: the plain build; side_b alone: the columns' kinds (launch_kgrad_build's
// kind_b; a derivative column holds the third derivative); both: path ids of rows and columns with q and sg2
// (launch_kgrad_build_g's).  A tile without a derivative column / a possible same-path pair gives the plain build's numbers.
template <typename T>
void launch_khess_build(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                        const int32_t* side_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                        const double* q, double sg2, T* V, int64_t ld, hipStream_t st);
// hmean (M, hess_pairs(d), k)[m][(i, j)][c] = sum_n d^2 k(As_m, Bs_n) / d As_mi d As_mj alphaT[c][n], matrix-free:
// launch_kgrad_matvec's arguments and grid (kgrad_matvec_shape), part of S * k * hess_pairs(d) * round_up(M, 64) elements
template <typename T>
void launch_khess_matvec(int kernel, const T* As, int64_t M, const T* Bs, int64_t npad, int d, double sf2,
                         const T* alphaT, int64_t lda, int k, const double* ls, int n_ls, T* part, T* hmean,
                         hipStream_t st);

// ---- joint density of blocks of query points (gpx_score.hip) -----------------------------------
// Column slices of V^T per block in launch_block_gram: a function of npad ONLY (a block's partial sums, and with them its
// results, may not depend on how many blocks a call or a batch holds).
int score_slices(int64_t npad);
inline int score_lp(int Lg) { return 16 * ((Lg + 15) / 16); }  // Gram edge: Lg rounded up to whole 16 x 16 MFMA tiles
// part [nblk][score_slices(npad)][LP][LP] (fp64; only the lower 16 x 16 tiles are written): per-slice Gram of the rows
// [b Lg, (b + 1) Lg) of VT (ld) over the columns [0, npad), block b < nblk, 1 <= Lg <= 64
template <typename T>
void launch_block_gram(const T* VT, int64_t ld, int64_t nblk, int Lg, int64_t npad, double* part, hipStream_t st);
// Block b < nblk of a batch (global number g0 + b): S = sf2 k(Qs_b, Qs_b) + diag_add I - sum of its partials, Cholesky,
// r = ys_b - mean_b (each (Lg, k)), then maha[g][c] = |L^-1 r_c|^2, logdet[g] = log|S|, logp[g][c]; Qs, ys, mean start at
// the batch's first row, the outputs at block 0 of the call.  A pivot that is not > 0: NaN outputs, *bad = min(*bad, g + 1).
template <typename T>
void launch_block_score(int kernel, const double* part, int64_t nblk, int Lg, int64_t npad, const T* Qs, int d,
                        const T* ys, const T* mean, int k, double sf2, double diag_add, T* logp, T* maha, T* logdet,
                        int64_t g0, int* bad, hipStream_t st, const T* wq = nullptr,  // wq (nblk Lg), from the batch's first
                        double sg2 = 0.0, const double* q = nullptr,                  // row: + diag_add wq[i] per point
                        const double* U = nullptr, int pu = 0);
// U != null (a fit with basis functions; (nblk Lg) x 64 fp64 from the batch's first row, launch_basis_epilogue's): S gains
// u_i . u_j over pu entries, and `mean` already includes h^T beta; null: today's bits.  The same for launch_block_forecast.
// sg2 > 0 (a fit with path ids): every block is a new path, S gains sg2 k(Qs_b, Qs_b; l_path); q (d, device) = (l_c / l_path,c)^2
// Block b < nblk of a batch of gpx_forecast_blocks: Lo observed rows, then Lp rows to forecast (Lo + Lp <= 64); part as
// above with Lg = Lo + Lp; Qs and mean ((Lo + Lp) rows per block) and yo (Lo rows per block) start at the batch's first
// block, the outputs at block 0 of the call: fmean (G Lp, k), fcov (G, Lp, Lp) | null, fvar (G Lp) | null, flogp (G, k) | null.
// diag_add goes on the observed rows only.  A pivot that is not > 0: NaN outputs, *bad = min(*bad, g + 1).
template <typename T>
void launch_block_forecast(int kernel, const double* part, int64_t nblk, int Lo, int Lp, int64_t npad, const T* Qs, int d,
                           const T* yo, const T* mean, int k, double sf2, double sg2, const double* q, double diag_add,
                           T* fmean, T* fcov, T* fvar, T* flogp, int64_t g0, int* bad, hipStream_t st,
                           const double* U = nullptr, int pu = 0);

// ---- explicit basis functions (gpx_basis.hip) -------------------------------------
// basis 1 | 2 | 3 (include/gpx.h): h(x) = [1] | [1, x_c] | [1, x_c, x_c^2] of the RAW inputs, p = 1 | 1 + d | 1 + 2 d functions
inline int basis_count(int basis, int d) { return basis == 1 ? 1 : basis == 2 ? 1 + d : basis == 3 ? 1 + 2 * d : 0; }
// the handle's state block (fp64, on the device): beta[j * 64 + c] | L_A[i * 64 + j] (lower) | A^-1[i * 64 + j]
constexpr int BASIS_STATE = 3 * 64 * 64;
// rows [k, k + p) of the bordered block YT (ld) = H^T over the columns < n, zero up to npad; X (n x d) the raw points
template <typename T>
void launch_basis_rows(const T* X, int64_t n, int64_t npad, int d, int k, int p, T* YT, int64_t ld, hipStream_t st);
// Column slices of the bordered rows' Gram: a function of npad ONLY, one fp64 partial per slice, summed in slice order
int basis_gram_slices(int64_t npad);
// part [basis_gram_slices(npad)][64][64] (fp64) = per-slice zT zT^T of the 64 bordered rows zT (ld) over the columns [0, npad)
template <typename T>
void launch_bordered_gram(const T* zT, int64_t ld, int64_t npad, double* part, hipStream_t st);
// one workgroup: A = G[k:k+p, k:k+p], L_A = chol A, beta = A^-1 G[k:k+p, 0:k], A^-1 into `state`.  A pivot j (1-based) of A
// that is not > 0 or not finite: atomicMin(info, n + j), state left as it was.
void launch_beta_solve(const double* part, int64_t npad, int k, int p, int64_t n, double* state, int* info, hipStream_t st);
// zT[c] -= sum_j beta[j][c] zT[k + j] for c < k over the columns [0, npad), formed in fp64 and rounded once
template <typename T>
void launch_basis_project(T* zT, int64_t ld, int64_t npad, int k, int p, const double* state, hipStream_t st);
// Query point m < rows (raw points Q, rows x d): mean[m][c] += h^T beta_c; with var or U: u = L_A^-1 (h - MT[k .. k + p, m]),
// var[m] += |u|^2 (var may be null), U[m * 64 + j] = u_j (U may be null).  Neither: MT is not read (the mean-only route).
template <typename T>
void launch_basis_epilogue(const double* state, int p, int k, int d, const T* MT, int64_t ldm, const T* Q, int64_t rows,
                           T* mean, T* var, double* U, hipStream_t st);
// lower triangle of Sig (M x M, lds) += U U^T, U (M x 64, fp64) as launch_basis_epilogue leaves it
template <typename T>
void launch_cov_add_uut(T* Sig, int64_t lds, int64_t M, int p, const double* U, hipStream_t st);

// ---- leave-one-out predictions (gpx_loo.hip; fp64) --------------------------------
// q[i] = sum_{i <= j < n} ZT[i][j]^2 for i < n, ZT = L^-T (row-major, ld; rows 128-byte aligned).  p > 0 (a fit with basis
// functions): ZHT = Z_H^T (p rows, ld: rows [k, k + p) of the bordered block), state the handle's basis state block;
// q[i] = q_i - |L_A^-1 b_i|^2 with b_i = sum_j ZT[i][j] Z_H[j][:], or 0 where that is <= 64 * 2^-52 * q_i (a row the basis
// coefficients alone determine).  Columns >= n are not read.  p = 0: neither ZHT nor state is read.
void launch_loo_rows(const double* ZT, int64_t ld, int64_t n, const double* ZHT, int p, const double* state, double* q,
                     hipStream_t st);
// var[i] = 1 / q[i], mean[i k + c] = Y[i k + c] - alphaT[c ld + i] / q[i], logp[i k + c] = -1/2 log(2 pi / q[i]) -
// alphaT[c ld + i]^2 / (2 q[i]) for i < n, c < k; q[i] = 0: var +inf, mean NaN, logp -inf
void launch_loo_finish(const double* q, const double* alphaT, int64_t ld, const double* Y, int64_t n, int k, double* mean,
                       double* var, double* logp, hipStream_t st);

// ---- pathwise posterior function samples (gpx_pathwise.hip) ------------------------
// q of include/gpx.h: the chi-square degrees of freedom of the family's spectral density (0: RBF, Gaussian frequencies)
int pathwise_chi_dof(int kernel);
// splits of launch_pathwise_eval's contraction: feature chunks, then (with_v) training chunks — functions of (npad, F) only
int pathwise_splits(int64_t npad, int64_t F, bool with_v);
// outT (cpad x mpad, ldo) = W Phi(As)^T + V K(As, Bs)^T, matrix-free on the MFMA units.  As (mpad x d, mpad a multiple of
// 64) and Bs (npad x d, npad a multiple of 64): scaled points, rows beyond the valid ones zero; V (cpad x ldv, cpad a
// multiple of 64, zero beyond the valid columns; null: the feature term alone); Om (F x d, fp64); W (cpad x ldw, ldw >=
// round_up(2 F, 64), zero beyond 2 F); part: pathwise_splits(npad, F, V != null) * cpad * mpad elements.
template <typename T>
void launch_pathwise_eval(int kernel, const T* As, int64_t mpad, const T* Bs, int64_t npad, int d, double sf2, const T* V,
                          int64_t ldv, const double* Om, int64_t F, const T* W, int64_t ldw, int64_t cpad, T* part, T* outT,
                          int64_t ldo, hipStream_t st);
// Om and W (every element of cpad x ldw) from the call's stream of normals: z (the caller's, device) or Philox `seed`
template <typename T>
void launch_pathwise_draw(const T* z, uint64_t seed, int64_t F, int d, int q, int64_t C, int64_t cpad, int64_t N, double* Om,
                          T* W, int64_t ldw, hipStream_t st);
// R (cpad x npad of ldr) = y^T - FT - sqrt(sn2 w) E for col < C, n < N, zero elsewhere; ebase = F (d + q); R may be FT
template <typename T>
void launch_pathwise_resid(const T* y, const T* FT, int64_t ldf, const T* wv, double sn2, const T* z, uint64_t seed,
                           int64_t ebase, int64_t F, int64_t N, int64_t npad, int k, int64_t C, int64_t cpad, T* R,
                           int64_t ldr, hipStream_t st);
// out (S, M, k)[s][m0 + mm][c] = outT[(s0 + s) k + c - r0][mm] for mm < mv
template <typename T>
void launch_pathwise_unpack(const T* outT, int64_t ldo, int64_t r0, int64_t s0, int64_t S, int64_t M, int64_t m0, int64_t mv,
                            int k, T* out, hipStream_t st);

// ---- inducing-point GP (gpx_sparse.hip; fp64) --------------------------------------
// The TN product: lower 64-tiles of C (n x n, ldc; n a multiple of 64) (+)= X^T X, X (rows x n, ldx; 16-byte aligned rows)
// row-major — the contraction runs over the ROWS.  The rows are dealt to syrk_tn_splits(n, rows_nominal) splits of equal
// length (a function of those two only; rows <= rows_nominal), each tile's partial sums (part: syrk_tn_part_elems
// elements) are added in split order, each split walks its rows in ascending order.  Nothing above the diagonal is written.
int syrk_tn_splits(int64_t n, int64_t rows_nominal);
int64_t syrk_tn_part_elems(int64_t n, int64_t rows_nominal);
void launch_syrk_tn(double* C, int64_t ldc, int64_t n, const double* X, int64_t ldx, int64_t rows, int64_t rows_nominal,
                    double* part, int accumulate, hipStream_t st);
// XT (cols x rows, ldt) = X (rows x cols, ldx)^T; rows, cols multiples of 32 (gpx_debug_syrk_tn_bench's transpose + NT route)
void launch_transpose(const double* X, int64_t ldx, int64_t rows, int64_t cols, double* XT, int64_t ldt, hipStream_t st);
// A chunk Kc (rows valid of rows_pad, ld) of cross-kernel rows over mpad columns: row r / s_r, s_r = sqrt(sn2 w[r]) (w null:
// 1), and columns [mpad, mpad + 64) = y[r][0..k) / s_r, zero beyond k and on the padded rows
void launch_sparse_border(double* Kc, int64_t ld, int64_t rows, int64_t rows_pad, int64_t mpad, const double* y, int k,
                          const double* w, double sn2, hipStream_t st);
// scal[0] = trace of B[0:mpad, 0:mpad], scal[1 + c] = B[mpad + c][mpad + c] (c < k), then B[j][j] += 1 for j < mpad
void launch_sparse_close(double* B, int64_t ld, int64_t mpad, int k, double* scal, hipStream_t st);
// var[i] = (sf2 - |V1[i]|^2) + |V2[i]|^2 + add over ncols columns, i < m
void launch_sparse_var(const double* V1, const double* V2, int64_t ld, int64_t m, int64_t ncols, double sf2, double add,
                       double* var, hipStream_t st);
// The rectangular derivative contraction of the bound's gradient: acc[t] += sum_{n < na, i < nb} W[n][i] r_n (dK / dlog
// theta_t)(As_n, Bs_i) for theta = (lengthscale[0..n_ls), sf2), r_n = 1 / sqrt(rsn2 rw[n]) (rw null: 1 / sqrt(rsn2); rsn2 = 1
// without rw: W as it is).  W (napad x ldw, ldw even, rows 16-byte aligned) is readable over napad x nbpad (multiples of 64)
// and may hold anything beyond na x nb; As (napad x d) and Bs (nbpad x d) are scaled points.  part: cross_dtheta_part_elems
// elements, one partial per (64-tile, theta), summed in tile order: two calls agree bit for bit.
int64_t cross_dtheta_part_elems(int64_t rows_pad, int64_t cols_pad, int n_ls);
void launch_cross_dtheta(int kernel, const double* W, int64_t ldw, int64_t na, int64_t napad, int64_t nb, int64_t nbpad,
                         const double* As, const double* Bs, int d, int n_ls, double sf2, const double* rw, double rsn2,
                         double* part, double* acc, hipStream_t st);
// H (in: B^-1) and M (in: B), both mpad x mpad at ld, become H = k (I - B^-1) - ch ch^T and M = H - k (B - I); chT (k rows, ld)
void launch_sparse_grad_weights(double* H, double* M, int64_t ld, int64_t mpad, const double* chT, int k, hipStream_t st);
// out[0] = trace of Binv over its mpad rows, out[1] = sum of squares of the k rows of chT over mpad columns
void launch_sparse_grad_scalars(const double* Binv, int64_t ld, int64_t mpad, const double* chT, int k, double* out,
                                hipStream_t st);

// ---- removal of observations (gpx_update.hip) -----------------------------------
constexpr int UPD_W = 64;  // panel width of the rank-m update of the trailing factor = most columns m one pass removes
// carry W ((n3 + 64) x UPD_W, compact): row i < n3 = columns [a, a + m) of row a + m + i of L, rows n3 + r those columns of
// the 64 bordered rows zT; zero from column m on
template <typename T>
void launch_upd_carry_init(const T* L, int64_t ld, int64_t a, int m, int64_t n3, const T* zT, T* W, hipStream_t st);
// the small step of the panel whose diagonal block sits at (p0, p0) of L (nv <= UPD_W valid rows) with carry rows Wj:
// Q (2 UPD_W square, row-major, formed in fp64 and rounded once).  A pivot that is not > 0: atomicMin(info, gidx0 + its
// 1-based place), gidx0 the 0-based index of the panel's first row in the remaining data.
template <typename T>
void launch_upd_small(const T* L, int64_t ld, int64_t p0, int nv, const T* Wj, T* Q, int64_t gidx0, int* info,
                      hipStream_t st);
// [ panel' | carry' ] = [ panel | carry ] Q over the nrows rows of L from p0 down (carry rows Wp) and the 64 bordered rows zT
// (carry rows Wz): panel' to outL (ldo) / outZ (ldz) under the lower-triangle / nv masks, carry' over the carry
template <typename T>
void launch_upd_strip(const T* L, int64_t ld, int64_t p0, int64_t nrows, int nv, const T* zT, T* Wp, T* Wz, const T* Q,
                      T* outL, int64_t ldo, T* outZ, int64_t ldz, hipStream_t st);
// a staged panel ((nrows + 64) x UPD_W, compact) into its place under the same masks
template <typename T>
void launch_upd_unstage(const T* P, int64_t nrows, int nv, T* dstL, int64_t ldl, T* dstZ, int64_t ldz, hipStream_t st);
// dst (rows x cols, ldd) = src (lds): any alignment; the two may not overlap
template <typename T>
void launch_upd_copy(T* dst, int64_t ldd, const T* src, int64_t lds, int64_t rows, int64_t cols, hipStream_t st);
// what a fit leaves beyond n points: rows [n, npad) of A zero up to column npad with a one on the diagonal, columns
// [n, nz) of the 64 rows of zT zero
template <typename T>
void launch_upd_pad(T* A, int64_t ld, int64_t n, int64_t npad, T* zT, int64_t nz, hipStream_t st);
// Winv[q] = inverse of the 64 x 64 diagonal block q of L for q0 <= q < q1 (launch_potf2_64's layout)
template <typename T>
void launch_upd_trinv(const T* L, int64_t ld, int64_t q0, int64_t q1, T* Winv, hipStream_t st);

// ---- row-block-cyclic shard helpers (gpx_misc.hip; T = double | float) ------------------------
// A[i][i] = i < nvalid ? A[i][i] + add : 1   for i < n (diagonal of one local row block)
template <typename T>
void launch_fix_diag(T* A, int64_t lda, int n, int nvalid, double add, hipStream_t st);
// Gathered panel G [P][maxcnt][ldp] (rank-major, each rank's trailing rows in local order)
// -> dst [(nblk-p-1)*nb][ldd] in global row order (the replicated factor's column block p: the update kernels read
// the gathered panel in place, bc_brow in gpx_tile.h).
template <typename T>
void launch_unpermute_panel(const T* G, int64_t ldp, T* dst, int64_t ldd, int nb, Deal dl, int p, int nblk, int64_t maxcnt,
                            hipStream_t st);
// YTloc[r][lb*nb + i] = y[(g*nb+i)*k + r] for the blocks g = dl.global(rank, lb) owned by `rank`.
template <typename T>
void launch_pack_rhs_local(const T* y, int64_t n, int k, T* YTloc, int64_t ldy, int nb, int nlb, Deal dl, int rank, int R,
                           hipStream_t st);
// Full[r][g*nb + i] = Loc[r][lb*nb + i] (own blocks), rest untouched.
template <typename T>
void launch_scatter_local(const T* Loc, int64_t ldl, T* Full, int64_t ldf, int nb, int nlb, Deal dl, int rank, int R,
                          hipStream_t st);
// dst (rows x cols, ldd) += sign * src (rows x cols, lds)
template <typename T>
void launch_add_block(T* dst, int64_t ldd, const T* src, int64_t lds, int rows, int cols, double sign, hipStream_t st);
template <typename T>
void launch_add_scalar(T* p, int64_t count, double v, hipStream_t st);
// p[i] = v, i < count
template <typename T>
void launch_fill(T* p, int64_t count, double v, hipStream_t st);
// *bad = 1 if any of w[0..n) is negative or not finite, else 0 (one workgroup; per-observation noise weights that
// arrive as device pointers)
template <typename T>
void launch_check_weights(const T* w, int64_t n, int* bad, hipStream_t st);
// dst[i] = op over q < P of src[q*count + i] in rank order (op 0 sum, 1 min); dst may not alias src
template <typename T>
void launch_reduce_ranks(const T* src, T* dst, int P, int64_t count, int op, hipStream_t st);
// out[0] += 2 * sum_i log(A[i][i]), i < n (one diagonal block)
template <typename T>
void launch_logdet_acc(const T* A, int64_t lda, int n, double* out, hipStream_t st);

}  // namespace gpx
