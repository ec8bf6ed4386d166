/* gpx.h — C ABI of libgpx.so: exact Gaussian-process regression on MI355X (gfx950).
 *
 * Drop-in boundary for the GP fit/predict hot path.  The upstream
 * reference (/root/reference/GPmap.py) has NO fit/predict, no kernel matrix and no
 * Cholesky (its only linalg call is np.linalg.norm, GPmap.py:120), so there is no
 * reference FFI to mirror: each entry point below cites the SURVEY.md §8 row that
 * defines it and, where one exists, the nearest reference code.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ types, no exceptions, no abort().
 *   - return 0 = ok, <0 = API misuse / HIP / RCCL error (text via gpx_last_error).
 *   - numerical failure is NOT an error code: *info > 0 is the 1-based index of the
 *     first non-positive pivot (LAPACK potrf convention) and the call returns 0.
 *   - all matrices are row-major, C-contiguous unless a leading dimension is given.
 *   - the caller owns every pointer it passes; the library owns every device
 *     allocation inside a handle and frees it in gpx_destroy.
 *   - a handle is not thread-safe; distinct handles may be used from distinct threads.
 *   - calls are synchronous at return.
 */
#ifndef GPX_H_
#define GPX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_ABI_VERSION 6 /* v6: gpx_predict_cov, gpx_sample_posterior, later gpx_predict_grad, gpx_kernel_grad_matrix, gpx_append, gpx_reserve and gpx_factor_info (additive: no existing call, struct or layout changed); v5: gpx_timings.handover_*, fp32 / mixed shards; v4: + gpx_fit_predict (v3: gpx_set_flags, refine, one-rank groups) */

/* kernel family — SURVEY.md §8 row a1 (nearest reference code: the pairwise
 * distance loop trajectories.calc_distance, GPmap.py:114-121, and the unused
 * scipy.spatial.distance import, GPmap.py:10). */
#define GPX_KERNEL_RBF 0      /* sf2 * exp(-r^2/2)                            */
#define GPX_KERNEL_MATERN52 1 /* sf2 * (1 + sqrt5 r + 5 r^2/3) exp(-sqrt5 r)  */
#define GPX_KERNEL_MATERN32 2 /* sf2 * (1 + sqrt3 r) exp(-sqrt3 r)            */
#define GPX_KERNEL_MATERN12 3 /* sf2 * exp(-r)  (exponential, Ornstein-Uhlenbeck) */
/* r^2 = sum_j ((x_j - x'_j) / l_j)^2, d_c = (x_c - x'_c) / l_c.  gpx_lml_grad: dK / dlog l_c = kd d_c^2 with
 *   RBF kd = k,  Matern-5/2 kd = sf2 (5/3) (1 + sqrt5 r) e^(-sqrt5 r),  Matern-3/2 kd = 3 sf2 e^(-sqrt3 r),
 *   Matern-1/2 kd = sf2 e^(-r) / r, and 0 at r = 0 (kd d_c^2 <= sf2 r -> 0).
 * Matern-1/2 is not differentiable: gpx_predict_grad and gpx_kernel_deriv_matrix return GPX_E_UNSUPPORTED for it. */

#define GPX_F64 0
#define GPX_F32 1
#define GPX_MIXED 2 /* inputs / outputs double; factorisation in fp32, alpha refined in fp64 against the  \
                       matrix-free fp64 kernel until ||y - K alpha|| <= 1e-10 ||y||: fp64-GRADE posterior \
                       MEAN, fp32-GRADE VARIANCE (sf2 - ||L^-1 k*||^2 through the fp32 factor, never      \
                       refined: errors of ~1e-6 sf2 absolute, i.e. percents of a small variance) (configs[4]) */

#define GPX_MEM_HOST 0   /* pointers are host memory; library copies H2D/D2H   */
#define GPX_MEM_DEVICE 1 /* pointers are device memory on the handle's device  */

#define GPX_FLAG_PROFILE 1 /* per-launch hipEvent timing of the Cholesky sub-phases */

/* error codes */
#define GPX_OK 0
#define GPX_E_ARG (-1)     /* bad argument / state                               */
#define GPX_E_HIP (-2)     /* HIP runtime error                                  */
#define GPX_E_COMM (-3)    /* RCCL / communicator error                          */
#define GPX_E_UNSUPPORTED (-4)
#define GPX_E_NOMEM (-5)

typedef struct gpx_handle gpx_handle;

/* transport of a single-process device group (gpx_config.ndev > 1) */
#define GPX_TRANSPORT_AUTO 0  /* RCCL when the listed devices are distinct, else LOCAL          */
#define GPX_TRANSPORT_RCCL 1  /* ncclCommInitAll inside the process, one communicator per device */
#define GPX_TRANSPORT_LOCAL 2 /* stream-ordered peer copies between the ranks' device buffers,   \
                                 hipEvents between their streams; no library besides HIP.  Also   \
                                 valid with one device listed several times (ranks share it).    */
#define GPX_MAX_GROUP 8

typedef struct gpx_config {
  int32_t kernel;  /* GPX_KERNEL_*                                   */
  int32_t dtype;   /* GPX_F64 | GPX_F32 | GPX_MIXED                  */
  int32_t device;  /* HIP device ordinal this handle computes on (ndev <= 1)                 */
  int32_t block;   /* Cholesky panel width nb (multiple of 128, <= 4096), 0 = the library's choice: 1024; 2048 from N = 40960 on */
  int32_t rank;    /* process-per-GPU shard: this process' rank (0 if world==1)              */
  int32_t world;   /* process-per-GPU shard: number of processes sharing the Gram matrix     */
  int32_t flags;   /* GPX_FLAG_*                                     */
  /* Single-process multi-GPU (SURVEY.md §8b "Threading"): ndev > 1 makes the handle a GROUP —
   * one rank per entry of devices[], one worker thread per rank inside the calling process,
   * the same row-block-cyclic schedule as the process-per-GPU shard.  gpx_fit / gpx_predict /
   * gpx_get_alpha / ... on the group handle are ordinary blocking calls of a plain caller (no
   * launcher, no torch.distributed); rank/world must be 0/1 then. */
  int32_t ndev;                     /* 0 or 1: one device (`device`);  2..GPX_MAX_GROUP: group; 1 with an explicit \
                                       transport (not AUTO): a ONE-rank group on devices[0] (the group / RCCL   \
                                       code path on a single GPU: tests)                                        */
  int32_t devices[GPX_MAX_GROUP];   /* HIP ordinals of the group's ranks                       */
  int32_t transport;                /* GPX_TRANSPORT_*                                         */
  int32_t refine;                   /* GPX_MIXED: 0 = refine until the relative residual is <= 1e-10 or stops  \
                                       contracting (at most 12 iterations); > 0 = exactly that many      */
  int32_t reserved[2];
} gpx_config;

/* per-phase wall times (ms, hipEvent on the handle's stream) of the LAST
 * gpx_fit / gpx_predict — SURVEY.md §8(d). */
typedef struct gpx_timings {
  double h2d, kbuild, chol, solve, logdet, fit_total;          /* gpx_fit     */
  double kstar, mean, trsm, var, d2h, predict_total;           /* gpx_predict */
  double comm;                                                 /* RCCL time inside chol (sharded) */
  /* Cholesky sub-phases, filled only with GPX_FLAG_PROFILE: */
  double chol_diag, chol_trsm, chol_strip, chol_syrk; /* summed ms (diag/trsm run on the look-ahead stream) */
  double syrk_flops;                       /* algorithmic flops n(n+1) nb of the 128-tile trailing-update launches \
                                              (chol_syrk / syrk_launches cover the same launches; the last few,     \
                                              under-filled updates run as 64-tiles and are booked under chol_strip) */
  int64_t syrk_launches;
  double kbuild_bytes;                     /* algorithmic bytes of the kernel build */
  double grad_trtri, grad_trace, grad_total; /* gpx_lml_grad: L^-T build, fused K^-1 trace pass, whole call */
  double refine;                           /* GPX_MIXED: ms spent refining alpha in fp64 */
  double refine_resid0, refine_resid;      /* ||y - K alpha|| / ||y|| before / after the refinement */
  double refine_iters;                     /* GPX_MIXED: refinement iterations the last fit ran */
  /* ABI v5: how the streams of the last fit handed over inside the diagonal chain.  1 = device flags (a kernel parked  \
     on the side stream polls a word the POTF2 publishes), 0 = hipEvents — chosen by a ~100 us self-test at the handle's \
     first fit (does a parked kernel see a store launched later on another stream?), by GPX_CHAIN_FLAG=0|1, or because    \
     rocprofv3 counter collection is on.  Same kernels and bit-identical results either way. */
  double handover_flags;
  double handover_retries;                 /* fits of this handle re-run with hipEvents after a parked stream timed out */
} gpx_timings;

/* ---- lifecycle ------------------------------------------------------------- */
int gpx_abi_version(void);
int gpx_device_count(int* count);
int gpx_create(gpx_handle** out, const gpx_config* cfg);
void gpx_destroy(gpx_handle* h);
const char* gpx_last_error(gpx_handle* h); /* h may be NULL: last error of gpx_create */

/* ---- hot path (SURVEY.md §8 rows a1,a3,a4 = fit; a2,a5,a6 = predict) --------- */
/* K = sf2 k(X,X) + (sn2+jitter) I;  L = chol(K);  alpha = L^-T L^-1 y.
 * X (N,d), y (N,k) row-major, in the dtype of the handle (GPX_F64 and GPX_MIXED: double,
 * GPX_F32: float — everything including the factorisation then runs in fp32: config 5, the
 * precision study; GPX_MIXED: fp32 factorisation + fp64 refinement, k <= 8).  ABI v5: every dtype also on
 * a shard / device group (the row-block shard runs in the handle's element type; the mixed mode's fp64
 * refinement is replicated work on every rank, its fp32 solves local on a replicated factor and collective
 * on a factor that is only held distributed).  lengthscale: n_ls = 1 or d.
 * *info (written when the call returns 0; never negative): 0 = fitted.  p > 0 = K is not positive definite, LAPACK's potrf
 * convention: p is the 1-based index of the first failing pivot, i.e. the leading minor of order p is the first that is
 * not positive definite; rows [0, p - 1) of the factor are valid (the factor of the leading minor of order p - 1), nothing
 * else is, and the handle holds no fit.  A non-finite input row counts as failing: a NaN in row r of X makes pivot r NaN
 * and *info = r + 1 (with a Strassen level of the two-level schedule on and r right of its split c: c < *info <= r + 1,
 * DESIGN.md §3.2 item 6). */
int gpx_fit(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
            const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
            int32_t mem_kind, int64_t* info);

/* mean (M,k) = K* alpha;  var (M) = sf2 - colsumsq(L^-1 K*^T)  (latent variance,
 * raw — not clamped).  var may be NULL (mean only). */
int gpx_predict(gpx_handle* h, const void* Xs, int64_t M, void* mean, void* var,
                int32_t mem_kind);

/* gpx_fit and gpx_predict (with variance) of ONE batch of query points as one call (ABI v4): the M cross-kernel
 * rows K(Xs, X) ride through the blocked factorisation as bordered rows — the way the right-hand sides already
 * do — and leave it as V^T = (L^-1 K*^T)^T, so the variance solve costs no pass of its own: its M N^2 flops are
 * rows of the trailing updates (at small N they run on the CUs the serial diagonal chain leaves idle; N = 8192,
 * M = 4096: 12.6 -> 11.5 ms per step).  Same results as the two calls up to the rounding of a different
 * summation order; the handle is fitted afterwards exactly as after gpx_fit (gpx_predict, gpx_get_alpha,
 * gpx_lml_grad ... work on it).  *info > 0: not positive definite, nothing was predicted.  ABI v5: every handle
 * accepts the call (v4: GPX_E_UNSUPPORTED beyond single-device fp64 / fp32 handles and one batch).  Single device,
 * GPX_F64 / GPX_F32: one predict batch (8192 rows) rides, further batches go through the ordinary predict against the
 * factor the pass leaves behind.  Shards and device groups (GPX_F64 / GPX_F32): rank r's slice of the query points —
 * ceil(M / world) rounded up to 128 — rides through ITS part of the sharded factorisation as bordered rows of its local
 * row set (up to 8192 rows per rank; a collective call: every rank of a shard makes it with the same arguments), in
 * both solve modes; GPX_SHARD_FUSED=0 runs the two calls instead.  GPX_MIXED handles run the call as gpx_fit +
 * gpx_predict (the refinement needs the factor first).  Mirrors the reference-side usage `gp.fit(X, y);
 * gp.predict(Xs)`. */
int gpx_fit_predict(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
                    const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, const void* Xs,
                    int64_t M, void* mean, void* var /* may be NULL */, int32_t mem_kind, int64_t* info);

/* ---- joint posterior (ABI v6) ---------------------------------------------------------------------------------------
 * Both calls: single-device GPX_F64 / GPX_F32 handles after a successful fit, element type the handle's (as gpx_predict).
 * GPX_MIXED handles, shards and device groups return GPX_E_UNSUPPORTED (nothing computed, the fit stays valid).  A query
 * set too large for the card returns GPX_E_NOMEM (gpx_last_error names the bytes) before anything is allocated.  Neither
 * call changes the fit: gpx_predict afterwards is bit-identical to gpx_predict before.  Their device buffers are scratch
 * (gpx_release_scratch frees them).  Timings: kstar, trsm, mean, d2h, predict_total as for gpx_predict; var = assembling
 * Sigma (and for sampling its factorisation and the transform).
 *
 * mean (M,k) = K* alpha (may be NULL);  cov (M,M) = K(Xs,Xs) - V^T V,  V = L^-1 K*^T: the latent (noise-free) joint
 * covariance, full and bit-symmetric, row-major, the same for every target column.  Its diagonal is gpx_predict's var up
 * to rounding (a different summation order). */
int gpx_predict_cov(gpx_handle* h, const void* Xs, int64_t M, void* mean, void* cov, int32_t mem_kind);

/* S joint posterior samples per target:  out[s,:,c] = mean[:,c] + L_S z[s,:,c],  L_S = chol(cov + (diag_add + j) I),
 * out (S,M,k) row-major.  z (S,M,k): the caller's standard normals (same memory kind and element type as out), or NULL:
 * generated on the device from `seed`.  j starts at `jitter`; after a failed factorisation j <- max(j, 1e-12 sf2) * 10,
 * at most max_tries attempts; *jitter_used = the j of the last attempt (the one that succeeded).  *info > 0: still not
 * positive definite (first bad pivot, LAPACK convention); the call returns 0 and `out` is undefined.
 *
 * The device normals (fixed, so that results can be reproduced anywhere): normal number i = (s M + m) k + c of the call
 * comes from Philox4x32-10 (Random123 constants) with counter (n & 0xffffffff, n >> 32, 0, 0), n = i >> 1, and key
 * (seed & 0xffffffff, seed >> 32); its output words w0..w3 give
 *     u1 = (((w0 << 32 | w1) >> 11) + 1) 2^-53,   u2 = ((w2 << 32 | w3) >> 11) 2^-53,   r = sqrt(-2 ln u1),
 *     z[2n] = r cos(2 pi u2),   z[2n+1] = r sin(2 pi u2)     (fp64; GPX_F32 handles round these to fp32).
 * Sample s depends on (seed, s, M, k) only: the first S' samples of a call with S > S' are those of the call with S'.
 * Known answers: key 0, counter 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all-ones key and counter -> 408f276d
 * 41c83b0e a20bc7c6 6d5451fd. */
int gpx_sample_posterior(gpx_handle* h, const void* Xs, int64_t M, int64_t S, uint64_t seed, const void* z,
                         double diag_add, double jitter, int32_t max_tries, void* out /* (S,M,k) */,
                         double* jitter_used, int64_t* info, int32_t mem_kind);

/* ---- posterior gradient (ABI v6, additive) ---------------------------------------------------------------------------
 * The derivative of the posterior with respect to the query point (for a path model: the velocity).  With u = x / l
 * (per dimension for ARD), r^2 = sum_j (u*_j - u_j)^2:
 *   RBF         d k(x*, x) / d x*_j = -(sf2 / l_j) (u*_j - u_j) e^(-r^2/2),                        prior Var = sf2 / l_j^2
 *   Matern-5/2  d k(x*, x) / d x*_j = -(sf2 / l_j) (5/3) (1 + sqrt5 r) e^(-sqrt5 r) (u*_j - u_j),  prior Var = 5 sf2 / (3 l_j^2)
 *   Matern-3/2  d k(x*, x) / d x*_j = -(sf2 / l_j) 3 e^(-sqrt3 r) (u*_j - u_j),                    prior Var = 3 sf2 / l_j^2
 * (smooth at r = 0, where it is 0).  Matern-1/2 is not differentiable: its handles return GPX_E_UNSUPPORTED
 * (gpx_last_error says why), nothing is computed and the fit stays valid.  With d_j K* the (M, N) matrix of d k(x*_m, x_n) / d x*_mj:
 *   dmean[m, j, c] = (d_j K* alpha)[m, c] = ((L^-1 d_j K*^T)^T z)[m, c]
 *   dvar[m, j]     = prior_j - ||L^-1 (d_j K*)_m^T||^2   (latent: no noise term; raw, not clamped; the same for every
 *                                                         target column, as gpx_predict's var)
 * Same handles, refusals (GPX_E_UNSUPPORTED for GPX_MIXED, shards, device groups; the fit stays valid), element type and
 * memory kinds as gpx_predict_cov; the fit is only read (gpx_predict afterwards is bit-identical); its device buffers are
 * scratch (gpx_release_scratch frees them).  var and dvar both NULL: dmean is computed matrix-free from the cached alpha
 * (one exponential per query / training pair, no solve, nothing of size M N stored) and mean, if requested, by
 * gpx_predict's mean-only path.  Otherwise the query points go in batches (GPX_PRED_BATCH, shrunk to the card): the rows
 * [K*;] d_1 K*; ...; d_d K* of a batch are built by one fused kernel, solved by ONE forward substitution, and one z^T V
 * product gives mean and dmean together; GPX_E_NOMEM (before any allocation, gpx_last_error names the bytes) when not
 * even one batch of 128 points fits.  Timings: kstar (builds), trsm, mean, var, d2h, predict_total as for gpx_predict.
 * Layouts (row-major): dmean (M,d,k), dvar (M,d), mean (M,k), var (M). */
/* gradient of the posterior at M query points (single-device GPX_F64 / GPX_F32 handles after a successful fit):
 * dmean (M,d,k) = d mean / d x*,  dvar (M,d) = latent variance of each partial derivative (may be NULL);
 * mean (M,k) and var (M) (each may be NULL) = gpx_predict's, from the same pass. */
int gpx_predict_grad(gpx_handle* h, const void* Xs, int64_t M, void* mean, void* var, void* dmean, void* dvar,
                     int32_t mem_kind);

/* ---- joint density of blocks of query points (additive to ABI v6) --------------------------------------------------------
 * How likely is a whole path under the fitted model: the query points come in G blocks of Lg consecutive points (a path =
 * a block), and each block is scored under its JOINT posterior — the Lg x Lg diagonal block of gpx_predict_cov's matrix,
 * never the (G Lg)^2 matrix itself.  Per batch of query points the call runs gpx_predict's K* build, variance solve and
 * mean product, then ONE more pass over V^T = K* L^-T (the traffic of gpx_predict's variance pass): the lower 16 x 16 tiles
 * of each block's Gram through the fp64 MFMA (fp32 rows are widened on the way in), one fp64 partial per column slice — the
 * slice count depends on N only, nothing is accumulated atomically — and per block, in fp64 whatever the element type,
 * S_g = sf2 k(X_g, X_g) + diag_add I - Gram, its Cholesky, and the forward solve of the k residual columns.  A block's
 * results therefore do not depend on G, on its position in the call or on the batch size (GPX_PRED_BATCH; batches hold whole
 * blocks).  Same handles, refusals (GPX_E_UNSUPPORTED for GPX_MIXED, shards, device groups: nothing computed, the fit stays
 * valid), element type and memory kinds as gpx_predict_cov; every family, Matern-1/2 included (no derivative is involved).
 * The fit is only read (gpx_predict afterwards is bit-identical); the device buffers are scratch (gpx_release_scratch frees
 * them).  GPX_E_NOMEM (before any allocation, gpx_last_error names the bytes) when not even one batch of 128 rows fits.
 * Bad arguments: GPX_E_ARG; *info is written only when the call returns 0.  Timings: kstar, trsm, mean, d2h, predict_total as
 * for gpx_predict; var = the Gram pass plus the block factorisations. */
/* Joint log predictive density of G blocks of Lg consecutive query points each (a path = a block).
 * Xs (G*Lg, d), ys (G*Lg, k) row-major in the handle's element type, d and k as fitted.  For block g with
 * m_g = K*_g alpha (Lg,k), S_g = K(X_g,X_g) - V_g^T V_g + diag_add I (the same for every target), r_c = ys_g[:,c] - m_g[:,c]:
 *   maha[g,c] = r_c^T S_g^-1 r_c,  logdet[g] = log|S_g|,
 *   logp[g,c] = -1/2 maha[g,c] - 1/2 logdet[g] - Lg/2 log 2 pi.
 * diag_add >= 0: sn2 for the density of noisy observations, 0 for the latent function.  1 <= Lg <= 64, G >= 1.
 * maha, logdet may be NULL.  *info > 0: 1-based index of the FIRST block whose S_g has a non-positive pivot; that
 * block's outputs are NaN, every other block is valid; the call returns 0.  The fit is only read. */
int gpx_score_blocks(gpx_handle* h, const void* Xs, const void* ys, int64_t G, int32_t Lg, double diag_add,
                     void* logp /* (G,k) */, void* maha /* (G,k) */, void* logdet /* (G) */,
                     int32_t mem_kind, int64_t* info);

/* ---- appending observations (additive to ABI v6) ------------------------------------------------------------------------
 * gpx_append: m more observations into a fitted handle without factorising the old ones again.  Xnew (m,d), ynew (m,k)
 * row-major in the handle's element type, d and k as fitted.  Afterwards the handle is, to rounding, what gpx_fit of the
 * concatenated N + m points with the same hyper-parameters and the fit's jitter would have left: every other call
 * (gpx_predict, _cov, _grad, gpx_sample_posterior, gpx_get_alpha, gpx_logdet, gpx_lml_grad, a further gpx_append) works on
 * N + m points.  With nb the fit's panel width (kept for the life of the fit) and R0 = floor(N / nb) nb, rows [0, R0) of L
 * and columns [0, R0) of z^T = (L^-1 y)^T stay as they are; the call solves the left part of the 128-row tiles that hold a
 * new point against those R0 columns, rebuilds K on [R0, N + m)^2, subtracts the Schur term of the R0 columns in one product
 * and restarts the blocked factorisation there (the right-hand sides ride as bordered rows, as in gpx_fit):
 * m' R0^2 + n'^2 R0 + n'^3 / 3 flops, m' the rows solved again and n' the padded trailing size, against N^3 / 3.
 * *info > 0: 1-based index, in the concatenated data, of the first non-positive pivot; the call returns 0 and the handle
 * holds the previous fit again (N points, every call valid): the same restart with no new point rebuilds it.
 * Timings: the fit fields (h2d, kbuild, chol, logdet, fit_total), zeroed at the start of the call.
 * Single-device GPX_F64 / GPX_F32 handles after a successful fit (else GPX_E_ARG); GPX_MIXED handles, shards and device
 * groups return GPX_E_UNSUPPORTED (nothing computed, the fit stays valid).
 * Memory: within the capacity of the layout (gpx_reserve; without it the padding up to the next multiple of 128) nothing
 * is reallocated or copied.  Beyond it the factor's lower triangle moves into a buffer with room for one more panel
 * width of points, so a stream of small appends reallocates at most once per nb points; old and new buffer exist side by
 * side for that moment.  GPX_E_NOMEM (gpx_last_error names the bytes) comes before anything is touched: the fit stays valid. */
int gpx_append(gpx_handle* h, const void* Xnew, const void* ynew, int64_t m, int32_t mem_kind, int64_t* info);
/* The next gpx_fit and later gpx_append lay the factor buffer out for up to `capacity` points (leading dimension from
 * round_up(capacity, 128)); appends within it happen in place.  0 (the default): what the fit itself needs — a handle
 * that never calls this fits exactly as before, and 0 on a fitted handle takes a reservation back for the fits that
 * follow (the current layout stays).  On a fitted handle any other capacity below its N is GPX_E_ARG; a larger one
 * takes effect with the next append (one move of the factor).  Refusals as for gpx_append. */
int gpx_reserve(gpx_handle* h, int64_t capacity);
/* Where the factor lives (single-device GPX_F64 / GPX_F32 handles after a successful fit): its device pointer (row-major,
 * lower triangle), leading dimension in elements and the points the layout has room for.  Any output may be NULL.  The
 * pointer changes only when a fit or an append has to reallocate. */
int gpx_factor_info(gpx_handle* h, const void** factor, int64_t* ld, int64_t* capacity);

/* ---- per-observation noise weights (additive to ABI v6) ---------------------------------------------------------------
 * Model: K = sf2 k(X,X) + diag(sn2 w_i + jitter), one weight w_i >= 0 per observation, shared by the k targets.  w = 1
 * everywhere is the model of a handle that never calls this, bit for bit; w_i = 0 is an exact observation (only the jitter
 * on its diagonal entry).  sn2 stays the level gpx_lml_grad differentiates: dK / dlog sn2 = sn2 diag(w), so its noise entry
 * is 1/2 sn2 sum_i w_i (sum_c alpha_ic^2 - k (K^-1)_ii); the weights are fixed data.  Absolute variances: sn2 = 1, w = them.
 *
 * gpx_set_noise_weights copies n weights (the handle's element type: double for GPX_F64 / GPX_MIXED, float for GPX_F32;
 * host or device memory as mem_kind says) into the handle.  They apply to every later gpx_fit / gpx_fit_predict — a
 * jitter-escalation loop, the repeated fits of an optimiser — until they are replaced or cleared (w == NULL with n == 0).
 * A negative or non-finite weight: GPX_E_ARG, nothing is stored and the weights of the call before stay.  A fit with
 * N != n returns GPX_E_ARG before anything is computed.  An existing fit is not touched: it keeps the weights it was made
 * with, for every call, until the next fit.
 * Single-device GPX_F64, GPX_F32 and GPX_MIXED handles (GPX_MIXED: the fp64 refinement runs against the weighted
 * matrix-free kernel; gpx_lml_grad stays GPX_F64 only).  On device groups, shards and handles that own a communicator
 * the call itself succeeds, and a fit with weights set returns GPX_E_UNSUPPORTED before anything is computed or
 * exchanged (gpx_last_error says why); once they are cleared the handle fits as before.
 * With no weights set a handle launches no additional kernel and allocates nothing more. */
int gpx_set_noise_weights(gpx_handle* h, const void* w, int64_t n, int32_t mem_kind);
/* The weights of the current fit (appended points included), all ones when it had none.  GPX_E_ARG without a fit. */
int gpx_get_noise_weights(gpx_handle* h, void* out /* (N) host, the handle's element type */);
/* gpx_append with weights wnew (m) for the new points (NULL: ones — what plain gpx_append does on a weighted fit too).
 * Validated like gpx_set_noise_weights, before the fit is touched.  The weight vector follows the factor's capacity rules
 * (gpx_reserve): nothing is reallocated within capacity.  A failed append (*info > 0) hands back the previous weights with
 * the previous fit.  Refusals as for gpx_append. */
int gpx_append_weighted(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, int64_t m, int32_t mem_kind,
                        int64_t* info);
/* gpx_score_blocks with S_g = K(X_g,X_g) - V_g^T V_g + diag_add diag(wq_g): wq (G*Lg) weights of the query points in the
 * handle's element type, validated like gpx_set_noise_weights; wq == NULL is gpx_score_blocks exactly.  The weights of
 * the FIT play no part here beyond the factor they went into.  Refusals as for gpx_score_blocks. */
int gpx_score_blocks_weighted(gpx_handle* h, const void* Xs, const void* ys, const void* wq, int64_t G, int32_t Lg,
                              double diag_add, void* logp /* (G,k) */, void* maha /* (G,k) */, void* logdet /* (G) */,
                              int32_t mem_kind, int64_t* info);

/* ---- derivative observations (additive to ABI v6) ----------------------------------------------------------------------
 * Model: row i of a fit is an observation at x_i with a kind: -1 a value of f, j (0 <= j < d) a value of d f / d x_j — a
 * velocity along input j.  A derivative of a GP is jointly Gaussian with it, so both enter one Gram matrix, one Cholesky
 * factor and the same prediction stages.  With u = (x_a - x_b) / l per dimension and v, g, h of the family (csrc/gpx_cov.h;
 * RBF: g = h = v) the entry for kinds (a, b) is
 *   (-1, -1)  v               ( i, -1)  -g u_i / l_i
 *   (-1,  j)  g u_j / l_j     ( i,  j)  (g delta_ij - h u_i u_j) / (l_i l_j)
 * and the diagonal term is (kind_i < 0 ? sn2 : sn2_deriv) w_i + jitter: sn2_deriv >= 0 is the noise variance of the
 * derivative rows (a level of its own: its unit is target / input), w the noise weights (ones when none are set).  A value
 * with w_i = 0 and a derivative with sn2_deriv = 0 at the same point say "pass through here with this velocity".
 * Query points stay values (gpx_predict, gpx_predict_cov, gpx_sample_posterior, gpx_score_blocks) or values and
 * derivatives (gpx_predict_grad); their prior variances do not change.
 *
 * gpx_set_observation_kinds copies n kinds (host or device memory as mem_kind says) and sn2_deriv into the handle.  They
 * apply to every later gpx_fit / gpx_fit_predict until they are replaced or cleared (kind == NULL with n == 0).  A kind
 * below -1, or a negative or non-finite sn2_deriv: GPX_E_ARG, nothing is stored and the kinds of the call before stay.  A
 * fit with N != n, or with a kind >= d, returns GPX_E_ARG before anything is computed.  An existing fit is not touched: it
 * keeps the kinds it was made with, for every call, until the next fit.
 * Single-device GPX_F64 / GPX_F32 handles, RBF, Matern-5/2 and Matern-3/2.  GPX_E_UNSUPPORTED before anything is computed
 * or exchanged, with the previous fit still valid and gpx_last_error saying why: a fit with a derivative kind on a
 * Matern-1/2 handle (not differentiable; kinds that are all -1 fit as the plain model there); a fit with kinds set on
 * GPX_MIXED handles, device groups, shards and handles that own a communicator (the set call itself succeeds, and once
 * the kinds are cleared the handle fits as before); gpx_lml_grad (gpx_lml_grad_full is the gradient of such a fit),
 * gpx_append and gpx_append_weighted on a fit that has a derivative row (gpx_append_rows appends to such a fit).  gpx_predict_grad without variances takes the batch route on such a fit (its matrix-free product knows
 * value columns only).  With no kinds set a handle launches the kernels it launched before and allocates nothing more. */
int gpx_set_observation_kinds(gpx_handle* h, const int32_t* kind, int64_t n, double sn2_deriv, int32_t mem_kind);
/* The kinds of the current fit, all -1 when it was made without any.  GPX_E_ARG without a fit. */
int gpx_get_observation_kinds(gpx_handle* h, int32_t* out /* (N) host */);

/* ---- within-path deviations: path ids on the observations (additive to ABI v6) ---------------------------------------------
 * Model (hierarchical GP): y_p(t) = f(t) + g_p(t) + noise — f the function the handle models, g_p a GP of its own for every
 * path p, independent between paths, of the handle's covariance family with variance sg2 and lengthscales ls_path:
 *   K[(x, p), (x', p')] = sf2 k(x, x'; l) + [p == p' and p >= 0] sg2 k(x, x'; l_path)      (+ (sn2 w_i + jitter) on the diagonal)
 * group[i] >= 0 names the path of observation i (ids need be neither contiguous nor sorted), -1 says "no path": that
 * observation gets f alone.  EVERY PREDICTION CALL KEEPS ITS CODE AND MEANING: gpx_predict, gpx_predict_cov,
 * gpx_predict_grad, gpx_sample_posterior and the mean-only route use K* = sf2 k(Xq, X) against the new factor, which is
 * exactly the posterior of the cluster mean f.  gpx_score_blocks(_weighted) on such a fit treats every block as a NEW path:
 * its covariance gains sg2 k(X_g, X_g; l_path).  gpx_forecast_blocks conditions a new path on its first points.
 *
 * gpx_set_path_groups copies n ids (host or device memory as mem_kind says), sg2 and the n_ls_path (1 or d; checked
 * against d at the fit) lengthscales into the handle, for every later gpx_fit / gpx_fit_predict until replaced or cleared
 * (group == NULL with n == 0).  GPX_E_ARG — nothing stored, the previous setting stays — for an id below -1, sg2 negative
 * or not finite, a lengthscale not > 0 or not finite, n_ls_path < 1 or > 32.  A fit with N != n, or n_ls_path not 1 or d:
 * GPX_E_ARG before anything is computed.  With every id -1, or sg2 == 0, a fit is the plain (or weighted) fit bit for bit.
 * Otherwise GPX_E_UNSUPPORTED before anything is computed or exchanged, the previous fit still valid: a fit on device
 * groups, shards, handles with a communicator, GPX_MIXED handles, and handles that also have observation kinds set; on a
 * fit made with path ids: gpx_append / gpx_append_weighted (the rows would come without ids: gpx_append_rows takes them),
 * gpx_lml_grad and
 * gpx_lml_grad_full (these evaluate training-pair covariances matrix-free, without the path term; gpx_lml_grad_paths is
 * the gradient of such a fit). */
int gpx_set_path_groups(gpx_handle* h, const int32_t* group, int64_t n, double sg2, const double* ls_path,
                        int32_t n_ls_path, int32_t mem_kind);
/* The path ids of the current fit, all -1 when it was made without any (or with sg2 == 0).  GPX_E_ARG without a fit. */
int gpx_get_path_groups(gpx_handle* h, int32_t* out /* (N) host */);
/* ---- appending rows with kinds or path ids (additive to ABI v6) -----------------------------------------------------------
 * gpx_append_weighted for every fit: the m new rows bring their weights wnew, kinds kind_new and path ids group_new (m
 * entries each; mem_kind says where all five arrays live).  wnew, kind_new and group_new may each be NULL: ones for the
 * weights, all -1 for the kinds and the ids.  Afterwards the handle is, to rounding, what gpx_fit of the concatenated rows
 * would have left — with the concatenated weights, kinds and ids in the same row order and the fit's hyper-parameters,
 * sn2_deriv, sg2, l_path and jitter — and every later call works on N + m rows: the predict family,
 * gpx_score_blocks(_weighted), gpx_forecast_blocks, gpx_get_alpha, gpx_logdet, gpx_lml_grad_full / gpx_lml_grad_paths,
 * gpx_get_observation_kinds, gpx_get_path_groups, gpx_get_noise_weights, a further append.
 * The restart is gpx_append's, through the builders of the fit: on a fit with kinds the left part of the new rows is the
 * rectangular KINDS build with kinds on rows and columns and the rebuilt square [R0, N + m)^2 the symmetric one; on a fit
 * with path ids the GROUPS builds, whose per-tile test "can this tile hold a same-path pair" skips the path term wherever
 * the ids of the new rows meet none of the columns'.  The kinds / ids and the finished diagonal terms follow the factor's
 * capacity rules (gpx_reserve) as the weights do.
 * Plain and weighted fits (made without kinds and without effective path ids): every kind and id is then NULL or -1 and
 * the call is gpx_append_weighted — the same launches, the same bits.  A fit made with kinds set stays one, also when
 * neither it nor the new rows hold a derivative: it keeps sn2_deriv, and gpx_get_observation_kinds returns N + m entries.
 * Kinds: a kind >= 0 needs a fit made with kinds set (gpx_set_observation_kinds; kinds that were all -1 count), else
 * GPX_E_ARG: the fit has no sn2_deriv.  A kind outside [-1, d): GPX_E_ARG.  A kind >= 0 on a GPX_KERNEL_MATERN12 handle:
 * GPX_E_UNSUPPORTED.  On a fit with a derivative row, kinds that are all -1 append values of f.
 * Path ids: an id >= 0 needs a fit built with path ids (one id >= 0 and sg2 > 0 at the fit), else GPX_E_ARG; an id below
 * -1: GPX_E_ARG.  An id may be new (a new path) or one the fit holds already (more points of a known path).
 * Every check, and the GPX_E_NOMEM of a layout that has to grow, comes before anything of the fit is touched.  Refusals
 * as for gpx_append (GPX_MIXED handles, shards, device groups, handles with a communicator).
 * *info > 0: as gpx_append — the call returns 0 and the handle holds the previous fit again, with its kinds, ids, weights
 * and finished diagonal terms; the getters return the old N entries. */
int gpx_append_rows(gpx_handle* h, const void* Xnew, const void* ynew, const void* wnew, const int32_t* kind_new,
                    const int32_t* group_new, int64_t m, int32_t mem_kind, int64_t* info);
/* ---- removing observations (additive to ABI v6) -------------------------------------------------------------------------
 * gpx_remove_rows: rows [start, start + count) of the fitted data leave the handle without a new factorisation of the
 * others.  Afterwards the handle is, to rounding, what gpx_fit of the remaining N - count rows (in their order, with the
 * same hyper-parameters, the fit's jitter and their own weights, kinds and path ids) would have left: every other call
 * (gpx_predict, _cov, _grad and their _paths forms, gpx_sample_posterior, gpx_score_blocks, gpx_forecast_blocks,
 * gpx_get_alpha, gpx_logdet, the three gpx_lml_grad*, a further append or remove) works on N - count points.
 * Nothing of the covariance is evaluated, so every kind of fit is served alike (plain, weighted, with observation kinds,
 * with path ids).  With a = start and b = start + count, rows [0, a) of L and the rows' columns [0, a) stay as they are
 * and the trailing factor takes the positive update L33' L33'^T = L33 L33^T + L32 L32^T, at most 64 removed columns per
 * pass (a longer range goes in chunks from its highest rows down), as orthogonal transformations of [L33 | L32] in column
 * panels of 64; z^T = (L^-1 y)^T rides through them as bordered rows.  About n3^2 (w + 2 m + m^2 / w) flops per pass of m
 * columns over n3 = N - b trailing rows (w = 64); removing the last rows is a truncation, the first rows the worst case:
 * taking out more than about N / 12 of the first rows costs as much as gpx_fit.
 * The factor is compacted inside its buffer: pointer, ld and capacity (gpx_factor_info) are unchanged and a later append
 * reuses the room.  The stored points, targets, weights, kinds, ids and diagonal terms follow; has_deriv is taken again
 * from the remaining kinds; the 64-block inverses are taken again from block start / 64 on; the explicit inverses of the
 * panel-wide diagonal blocks are dropped (solves then go through the 64-block inverses) and alpha is solved on demand.
 * count == 0: GPX_OK, nothing changes.  start < 0, count < 0, start + count > N or count == N (a fit keeps one point):
 * GPX_E_ARG, the fit stays valid.
 * *info: 0 on success.  The update is backward stable and in exact arithmetic meets no non-positive pivot; if one appears
 * all the same (non-finite numbers in the factor), *info is its 1-based index in the remaining data, the call returns 0
 * and the handle is left WITHOUT a fit (every later call but gpx_fit: GPX_E_ARG): the update works in place and cannot
 * be taken back.
 * Timings: the fit fields (chol, logdet, fit_total), zeroed at the start of the call.
 * Single-device GPX_F64 / GPX_F32 handles after a successful fit (else GPX_E_ARG); GPX_MIXED handles, shards and device
 * groups return GPX_E_UNSUPPORTED (nothing computed, the fit stays valid). */
int gpx_remove_rows(gpx_handle* h, int64_t start, int64_t count, int64_t* info);
/* Forecast of partly observed new paths.  Xb (G (Lo + Lp), d): per block its Lo observed points, then its Lp points to
 * forecast (1 <= Lo, 1 <= Lp, Lo + Lp <= 64); yo (G Lo, k) the observed targets; diag_add >= 0 goes on the diagonal of the
 * observed part only (the observation noise).  The block prior is posterior(f) [+ sg2 k(., .; l_path) on a fit with path
 * ids]; with S the joint (Lo + Lp)^2 covariance of a block, L_oo = chol(S_oo + diag_add I), B = S_po L_oo^-T and
 * w = L_oo^-1 (yo - mean_o):
 *   mean (G Lp, k) = mean_p + B w;   cov (G, Lp, Lp), may be NULL = S_pp - B B^T (latent, shared by the targets, exactly
 *   symmetric);   var (G Lp), may be NULL = its diagonal;   logp (G, k), may be NULL = the joint log-density of the
 *   observed prefix (gpx_score_blocks' number for the Lo points alone).
 * *info = 1-based index of the first block whose conditioning matrix is not positive definite (its outputs are NaN, the
 * others unaffected), 0 if none.  A block's numbers do not depend on G, its position or GPX_PRED_BATCH.  Single-device
 * GPX_F64 / GPX_F32 handles (GPX_E_UNSUPPORTED otherwise, as gpx_score_blocks); any fit, with or without path ids. */
int gpx_forecast_blocks(gpx_handle* h, const void* Xb, const void* yo, int64_t G, int32_t Lo, int32_t Lp, double diag_add,
                        void* mean, void* cov, void* var, void* logp, int32_t mem_kind, int64_t* info);
/* ---- predicting an observed path itself, f + g_p (additive to ABI v6) ------------------------------------
 * The four posterior calls with one more argument: gq, M path ids (int32, in the memory kind of Xs, every entry >= -1), one
 * per query point.  gq[i] == -1 asks for f(x_i), the plain call's meaning; gq[i] = p >= 0 asks for f(x_i) + g_p(x_i), the
 * path p itself:
 *   Cov[value(x*, p*), y_i]           = sf2 k(x*, x_i; l) + [p* == p_i and p* >= 0] sg2 k(x*, x_i; l_path)
 *   Cov[value(x*, p*), value(x', p')] = sf2 k(x*, x'; l)  + [p* == p'  and p* >= 0] sg2 k(x*, x'; l_path)
 * so the prior variance is sf2 + [p* >= 0] sg2, and that of d / d x_j is c sf2 / l_j^2 + [p* >= 0] c sg2 / l_path,j^2 (c the
 * family's dpoly(0)).  An id no training row carries is a path nobody has seen: the mean of f, the (co)variance of f plus
 * the prior sg2 k(., .; l_path).  Ids may be mixed freely in one call.  Outputs, batching, results on the device and every
 * other argument are the plain call's; a call whose ids are all -1 returns the plain call's bits wherever it takes the
 * plain call's route (gpx_predict_grad_paths without var and dvar takes the batch route, not the matrix-free product).  A
 * point's results do not depend on M, its position or GPX_PRED_BATCH.  The fit and the results of plain calls afterwards
 * are unchanged.
 * Refusals, before anything is computed: GPX_E_ARG for gq == NULL, an id below -1, and what the plain call refuses;
 * GPX_E_UNSUPPORTED ("path ids") when the current fit was not built with path ids (a plain, weighted or derivative fit, or
 * sg2 == 0 or every id -1 at the fit); GPX_E_UNSUPPORTED on device groups, shards, handles with a communicator and
 * GPX_MIXED handles; gpx_predict_grad_paths on GPX_KERNEL_MATERN12: GPX_E_UNSUPPORTED as gpx_predict_grad. */
int gpx_predict_paths(gpx_handle* h, const void* Xs, const int32_t* gq, int64_t M, void* mean, void* var, int32_t mem_kind);
int gpx_predict_cov_paths(gpx_handle* h, const void* Xs, const int32_t* gq, int64_t M, void* mean, void* cov,
                          int32_t mem_kind);
int gpx_sample_posterior_paths(gpx_handle* h, const void* Xs, const int32_t* gq, int64_t M, int64_t S, uint64_t seed,
                               const void* z, double diag_add, double jitter, int32_t max_tries, void* out,
                               double* jitter_used, int64_t* info, int32_t mem_kind);
int gpx_predict_grad_paths(gpx_handle* h, const void* Xs, const int32_t* gq, int64_t M, void* mean, void* var, void* dmean,
                           void* dvar, int32_t mem_kind);

/* ---- posterior second derivatives (additive to ABI v6) --------------------------------------------------
 * The second derivatives of the posterior by the query point (for a path model: the acceleration).  The pairs (i, j),
 * i <= j, are numbered row-major, D2 = d (d + 1) / 2 of them.  With u = (x* - x) / l and g, h, p of the family (v = sf2 k):
 *   d^2 k(x*, x) / d x*_i d x*_j          = (h u_i u_j - g delta_ij) / (l_i l_j)
 *   d^3 k(x*, x) / d x*_i d x*_j d x_c    = (p u_i u_j u_c - h (delta_ic u_j + delta_jc u_i + delta_ij u_c)) / (l_i l_j l_c)
 *                                           (against a derivative observation of kind c, gpx_set_observation_kinds)
 *   prior Var[d_i d_j f] = h(0) / (l_i^2 l_j^2) for i != j, 3 h(0) / l_i^4 for i == j;  h(0) = sf2 (RBF), (25/3) sf2 (Matern-5/2)
 *   RBF: g = h = p = v;  Matern-5/2: g = sf2 (5/3)(1 + s) e^-s, h = sf2 (25/3) e^-s, p = sf2 (125/3) e^-s / s, s = sqrt5 r
 * With d_ij K* the (M, N) matrix of those entries:
 *   hmean[m, (i,j), c] = (d_ij K* alpha)[m, c]
 *   hvar[m, (i,j)]     = prior_ij - ||L^-1 (d_ij K*)_m^T||^2     (latent, raw, not clamped; the same for every target)
 * hvar == NULL on a fit without derivative rows: hmean is computed matrix-free from the cached alpha (one exponential per
 * query / training pair, no solve).  Otherwise the query points go in batches (GPX_PRED_BATCH, shrunk to the card) through
 * gpx_predict_grad's stages: the D2 row blocks of a batch by one fused kernel, ONE forward substitution, one z^T V, row
 * norms; GPX_E_NOMEM before any allocation when not even one batch of 128 points fits.  A point's results do not depend on
 * M, its position or GPX_PRED_BATCH.  Handles, element type, memory kinds, scratch (gpx_release_scratch) and timings are
 * gpx_predict_grad's; the fit is only read (gpx_predict afterwards is bit-identical).
 * gpx_predict_hess_paths: gq as gpx_predict_grad_paths' — a query point with gq >= 0 is a point of f + g_p, whose
 * covariance with a same-path row gains the second derivative of sg2 k(., .; l_path) and whose prior gains the same formula in
 * sg2 and l_path; always the batch route; every id -1: the bits of gpx_predict_hess's batch route.
 * GPX_E_UNSUPPORTED before anything is computed (gpx_last_error says why; the fit stays valid): GPX_KERNEL_MATERN32 and
 * GPX_KERNEL_MATERN12 (not twice differentiable), d > 8, a fit with a basis, GPX_MIXED handles, shards, device groups and
 * handles with a communicator; gpx_predict_hess_paths on a fit without effective path ids.  GPX_E_ARG as gpx_predict_grad. */
int gpx_predict_hess(gpx_handle* h, const void* Xs, int64_t M, void* hmean /* (M, D2, k) */, void* hvar /* (M, D2), may be NULL */,
                     int32_t mem_kind);
int gpx_predict_hess_paths(gpx_handle* h, const void* Xs, const int32_t* gq, int64_t M, void* hmean, void* hvar,
                           int32_t mem_kind);

int gpx_get_alpha(gpx_handle* h, void* out /* (N,k) host */);
/* Log marginal likelihood of the last fit and its gradient w.r.t. the LOG hyper-parameters —
 * SURVEY.md §8(f) row 1 ("log marginal likelihood + hyper-parameter gradient hooks"; no anchor
 * in GPmap.py):  *lml = -1/2 sum_c y_c^T alpha_c - k/2 log|K| - N k/2 log 2 pi,
 * grad[0..n_ls) = d lml / d log lengthscale, grad[n_ls] = d / d log sf2, grad[n_ls+1] = d / d log sn2
 * (n_ls as passed to gpx_fit).  Costs about two more factorisations' worth of MFMA work
 * (L^-T, then K^-1 = L^-T L^-1 consumed tile by tile as it is formed) and one extra N x N
 * buffer; K^-1 itself is never stored.  fp64 handles.  Sharded handles and groups: collective
 * (every rank calls it, every rank gets the same numbers).  Replicated-factor mode: both passes are
 * split over the ranks with one all-gather of L^-T between them.  Factor only held distributed
 * (C4-sized problems): L^-T is built by the distributed forward substitution of the variance path,
 * each rank keeps the columns that belong to its own row blocks (N^2 / P numbers), contracts the
 * trace over them, and ntheta numbers are all-reduced (round 3; was GPX_E_UNSUPPORTED). */
int gpx_lml_grad(gpx_handle* h, double* lml, double* grad);
/* The same with one more entry (additive to ABI v6), for fits with derivative observations (gpx_set_observation_kinds) as
 * well: grad[n_ls + 2] = d lml / d log sn2_deriv, with dK / dlog sn2_deriv = sn2_deriv w_i on the derivative rows and
 * dK / dlog sn2 = sn2 w_i on the value rows.  The entry is exactly 0 when the fit has no derivative row or sn2_deriv = 0.
 * The derivative of a Gram entry of kinds (ka, kb) by a log lengthscale is the table of csrc/gpx_cov.h (element_dl),
 * evaluated in the epilogue of the same fused K^-1 trace pass: the cost is gpx_lml_grad's.  Single-device GPX_F64 handles,
 * with or without kinds or noise weights; on a fit without a derivative row *lml and grad[0 .. n_ls + 2) are gpx_lml_grad's
 * bit for bit.  GPX_E_UNSUPPORTED on other element types and on shards, device groups and handles that own a communicator
 * (no fit with a derivative row exists there: gpx_lml_grad is their call).  A failed call writes nothing and leaves the
 * fit valid. */
int gpx_lml_grad_full(gpx_handle* h, double* lml, double* grad /* n_ls + 3 */);
/* The gradient of a fit with path ids (gpx_set_path_groups; additive to ABI v6): grad as gpx_lml_grad's, and grad_path[0] =
 * d lml / d log sg2, grad_path[1 + c] = d lml / d log l_path,c.  With e_c = (x_ic - x_jc) / l_c, q_c = (l_c / l_path,c)^2,
 * r_p^2 = sum_c q_c e_c^2 and m_ij = [id_i == id_j >= 0]:  dK / dlog sg2 = m sg2 k(r_p),  dK / dlog l_path,c = m kd(r_p; sg2)
 * q_c e_c^2 (kd of the family, csrc/gpx_cov.h: path_dtheta; n_ls_path == 1: the sum over c);  dK / dlog sf2 = sf2 k(r), the f
 * part alone, and dK / dlog l_c is the plain one: the path term does not depend on l.  Evaluated in the epilogue of the same
 * fused K^-1 trace pass, only in tiles that can hold a same-path pair: the cost is gpx_lml_grad's.  On a fit made by the
 * path builder n_path must be 1 + n_ls_path of that fit (GPX_E_ARG otherwise).  On any other fit — no ids, every id -1 or
 * sg2 == 0 — *lml and grad are gpx_lml_grad's bit for bit, by the same launches, and the n_path >= 0 entries of grad_path
 * are set to exactly 0 (grad_path may be NULL when n_path == 0).  Single-device GPX_F64 handles, with or without noise
 * weights.  GPX_E_UNSUPPORTED on other element types, on shards, device groups and handles that own a communicator (no fit
 * with path ids exists there) and on a fit with derivative rows (gpx_lml_grad_full is its gradient).  A failed call writes
 * nothing and leaves the fit valid.  Timings: grad_trtri, grad_trace, grad_total, as for the other two. */
int gpx_lml_grad_paths(gpx_handle* h, double* lml, double* grad /* n_ls + 2, as gpx_lml_grad */,
                       double* grad_path /* n_path: d/dlog sg2, then d/dlog l_path,c */, int32_t n_path);
/* Leave-one-out predictive distribution of every observation of the current fit (R&W 5.10-5.12).  Host buffers, fp64;
 * any of them may be NULL, not all.  total: k sums of logp over the rows, in row order.
 * With Q = K^-1 of the fit as it stands (noise, weights, jitter, derivative rows and the path term included) and
 * q_i = Q_ii: var_i = 1 / q_i is the predictive variance of OBSERVATION i given all the others, its own noise included;
 * mean_ic = y_ic - alpha_ic / q_i; logp_ic = -1/2 log(2 pi / q_i) - alpha_ic^2 / (2 q_i).  A derivative row's entries are
 * about that derivative observation.  A fit with basis functions marginalises the coefficients (flat prior):
 * q'_i = q_i - |L_A^-1 (K^-1 H)_i|^2 replaces q_i, and h^T beta is inside mean.  A row that the basis coefficients alone
 * determine (q'_i <= 64 * 2^-52 * q_i; every row when N = p) is undetermined: var = +inf, mean = NaN, logp = -inf, and
 * total = -inf.
 * Cost: one L^-T (N^3 / 3 flops: the grad_trtri phase of a gradient, and its N^2 * 8 bytes of scratch, which
 * gpx_release_scratch frees) and one pass over it; every kernel family.  The sums have one order: two calls return the
 * same bits.  GPX_E_ARG without a fit or with four NULL outputs; GPX_E_UNSUPPORTED on GPX_F32 / GPX_MIXED handles and on
 * shards, device groups and handles that own a communicator.  A failed call writes nothing and leaves the fit valid. */
int gpx_loo(gpx_handle* h, double* mean /* (N,k) */, double* var /* (N) */, double* logp /* (N,k) */, double* total /* (k) */);

/* ---- pathwise posterior function samples (additive to ABI v6) ------------------------------------------
 * Matheron's rule with a random-Fourier-feature prior (Wilson et al. 2020): a posterior sample is a FUNCTION, drawn once
 * and evaluated anywhere, again and again.  With u = x / l (per dimension for ARD), F frequencies, C = S k columns,
 * col = s k + c, and K_y the matrix the fit factorised (noise, weights and jitter included):
 *   q                 = 2 nu of the family: 5 Matern-5/2, 3 Matern-3/2, 1 Matern-1/2; 0 for RBF
 *   Omega (F, d)      scaled frequencies shared by all columns: Omega_f = g_f sqrt(q / chi_f), g_f d standard normals, chi_f
 *                     the sum of squares of q further normals, in order (a Student-t draw; chi_f = 0, which only a
 *                     caller's all-zero z produces: Omega_f = 0); RBF: Omega_f = g_f
 *   theta_f(x)        = sum_j Omega_fj u_j
 *   f~_col(x)         = sqrt(sf2 / F) sum_f [ W[col, f] cos theta_f(x) + W[col, F + f] sin theta_f(x) ],  W (C, 2F) normals
 *   R[col, n]         = y[n, c] - f~_col(x_n) - sqrt(sn2 w_n) E[col, n],  E (C, N) normals, w_n the noise weight (1 without
 *                     weights); the factor's jitter is not sampled
 *   V                 = R K_y^-1, rows as alpha^T
 *   out[s, m, c]      = f~_col(x_m) + sum_n sf2 k(x_m, x_n) V[col, n]
 * The conditioning on the data is exact; only the prior draw is approximate: its covariance Phi Phi^T misses sf2 k by
 * O(1 / sqrt(F)) (profiles/pathwise_bias.json tabulates the effect on the posterior variance).
 *
 * One flat stream of n_normals = F (d + q) + C (2F + N) standard normals feeds a draw: numbers [f (d + q), (f + 1)(d + q))
 * are g_f followed by the chi normals of frequency f; after that block every column has 2F + N numbers, W[col, :] then
 * E[col, :].  z == NULL: number i is normal number i of the Philox stream `seed` that gpx_sample_posterior specifies.
 * Otherwise z holds the n_normals values, in the handle's element type and the memory kind of the call.  Consequence:
 * sample s depends on (seed, s, F, N, d, k, kernel) only — the first S' samples of a larger draw are the draw with S'.
 *
 * gpx_pathwise_draw stores Omega, W and V in the handle: state of the fit, not scratch (gpx_release_scratch keeps it).
 * S = 0 drops the stored draw.  Whatever changes the factor drops it too: gpx_fit, gpx_fit_predict, gpx_append(_weighted,
 * _rows), gpx_remove_rows; and gpx_set_noise_weights.  Cost: one pass of the evaluation kernel over the training points and
 * one pair of triangular solves per 64 columns (a column's bits do not depend on how many columns the draw has).
 * gpx_pathwise_eval writes samples [s0, s0 + S) of the stored draw at the M query points Xs into out (S, M, k), element
 * type and memory kind as gpx_predict; nothing of size M N or M M is stored, query points go in batches (any M), and
 * evaluating the same point again — alone, in another batch, with other samples — returns the same bits.  Without a live
 * draw: GPX_E_ARG, and gpx_last_error says so.  It only reads the fit: gpx_predict afterwards is bit-identical.
 * gpx_pathwise_info: the stored draw's S, F and n_normals (0, 0, 0 without one); each pointer may be NULL.
 * Single-device GPX_F64 / GPX_F32 handles, every family, scalar or ARD lengthscales, with or without noise weights.
 * GPX_E_UNSUPPORTED with a message, nothing computed and the fit still valid: GPX_MIXED handles, shards, device groups,
 * fits with derivative observations, with path ids or with a basis.  Timings: kstar (the draw: normals, features, residual
 * rows; eval: the query points), trsm (the draw's solves), mean (eval's kernel), d2h, predict_total. */
int gpx_pathwise_draw(gpx_handle* h, int64_t S, int64_t F, uint64_t seed, const void* z, int32_t mem_kind);
int gpx_pathwise_eval(gpx_handle* h, const void* Xs, int64_t M, int64_t s0, int64_t S, void* out /* (S,M,k) */,
                      int32_t mem_kind);
int gpx_pathwise_info(gpx_handle* h, int64_t* S, int64_t* F, int64_t* n_normals);

/* ---- inducing-point GP: the collapsed variational bound of Titsias 2009 ("SGPR") ----------------------
 * For data with more observations than a dense factor can hold: m inducing points Z stand for the N observations, the cost
 * is O(N m^2) and the memory O(m^2 + chunk m).  With s_n^2 = sn2 w_n (w_n = 1 when w == NULL), S = diag(s^2), yt = S^-1/2 y:
 *   Kuu = sf2 k(Z,Z) + jitter I,  L = chol(Kuu);   A = L^-1 sf2 k(Z,X) S^-1/2;   B = I + A A^T,  LB = chol(B);   c = LB^-1 A yt
 *   ELBO_c = -N/2 log 2 pi - sum log LB_ii - 1/2 sum log s_n^2 - 1/2 |yt_c|^2 + 1/2 |c_c|^2 - 1/2 sum sf2 / s_n^2 + 1/2 tr(A A^T)
 *   predict: T1 = L^-1 sf2 k(Z,Xs), T2 = LB^-1 T1;  mean = T2^T c,  var = sf2 - colsumsq(T1) + colsumsq(T2),
 *            cov = sf2 k(Xs,Xs) - T1^T T1 + T2^T T2   (the latent f: no noise term)
 * The cross-kernel rows are whitened by L^-1 BEFORE the contraction over the observations (the cheaper order loses the
 * result: DESIGN.md).  jitter is added to Kuu only: it is a (tiny) change of the model, not of the noise.
 * gpx_sparse_fit streams X, y, w in chunks of `chunk` observations (rounded up to a multiple of 128; 0: the library's
 * choice, a function of m alone); results depend on (m, chunk) but on nothing else of the machine, and two calls with the
 * same arguments agree bit for bit.  1 <= d <= 32, 1 <= k <= 8, 1 <= m <= 65536, n_ls 1 or d, sf2 > 0, sn2 > 0, jitter >= 0.
 * w: per-observation noise weights, finite and > 0 (GPX_E_ARG otherwise: a waypoint, w = 0, has no place in S^-1; the
 * weights of gpx_set_noise_weights are not used here).  X, y, w, Z, Xs and the outputs are fp64 in the memory kind given.
 * *info = 0, or the 1-based pivot of Kuu that was not > 0, or m + the pivot of B (which cannot happen in exact arithmetic);
 * the call returns 0 then and the handle is left without a fit.  Single-device GPX_F64 handles only: GPX_F32 / GPX_MIXED
 * handles, shards, handles with a communicator and device groups return GPX_E_UNSUPPORTED.  A size the card cannot hold
 * returns GPX_E_NOMEM before anything is allocated.
 * A handle holds a dense fit or a sparse fit, never both: either fit call replaces the other state, every other dense entry
 * point refuses a sparse-fitted handle with GPX_E_ARG (gpx_last_error names gpx_sparse_*), and the sparse entry points refuse
 * a dense-fitted handle the same way; the existing fit stays valid.  Not available on a sparse fit: the gradient of the
 * bound with respect to Z, update / remove / loo, derivative observations, path ids, basis functions.
 * Timings: kbuild (Kuu and the chunks' cross-kernel rows), chol (both factorisations), solve (whitening and contraction),
 * logdet, fit_total; kstar, trsm, mean, var, d2h, predict_total.
 *
 * gpx_sparse_elbo_grad: grad (n_ls + 2) = the gradient of F = sum_c ELBO_c by the LOG parameters, ordered as gpx_lml_grad's
 * (lengthscale[0..n_ls), sf2, sn2); elbo (k; may be NULL) = gpx_sparse_elbo's values.  Z and jitter are constants.  With
 *   ch = LB^-T c,   H = k (I - B^-1) - ch ch^T,   Guu = 1/2 L^-T [k (2 I - B^-1 - B) - ch ch^T] L^-1,
 *   t_n = L^-T (H a_n + ch yt_n^T) / s_n   (a_n: column n of A; row n of T = dF / dKuf^T):
 *   dF/dlog l_c = sum T . dKfu/dlog l_c + sum Guu . dKuu/dlog l_c          (dk/dlog l_c = kd ((x_c - z_c) / l_c)^2)
 *   dF/dlog sf2 = sum T . Kfu + sum Guu . sf2 k(Z,Z) - 1/2 k sf2 sum_n 1 / s_n^2
 *   dF/dlog sn2 = 1/2 k (m - tr B^-1) - 1/2 k N + 1/2 |yt|^2 - |c|^2 + 1/2 (|c|^2 - |ch|^2) + 1/2 k sf2 sum_n 1 / s_n^2
 *                 - 1/2 k tr(A A^T)
 * The fit does not keep the observations: the caller passes the X, y, w (and N) of the gpx_sparse_fit the handle holds, in
 * one memory kind; N != the fit's is GPX_E_ARG, and other data of the same N is the caller's error (the result is then the
 * gradient of nothing).  The observations stream once more in the fit's chunks; the cost is O(m^3) + one more pass of the
 * fit's build and whitening + 2 N m^2 flops of one product, the memory five m x m temporaries and one more chunk buffer
 * (scratch: gpx_release_scratch frees them), checked before anything is allocated (GPX_E_NOMEM).  Refusals as the other
 * gpx_sparse_* calls.  A call that fails writes neither output; the fit stays valid either way, and a later
 * gpx_sparse_predict returns the bits it returned before.  Two calls agree bit for bit.  Timings: grad_trtri (the O(m^3)
 * stage), grad_trace (the streamed pass), grad_total. */
int gpx_sparse_fit(gpx_handle* h, const void* X, const void* y, const void* w /* (N) or NULL */, int64_t N, int32_t d, int32_t k,
                   const void* Z, int64_t m, const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
                   int64_t chunk /* 0: library's choice */, int32_t mem_kind, int64_t* info);
int gpx_sparse_predict(gpx_handle* h, const void* Xs, int64_t M, void* mean /* (M,k) */, void* var /* (M) | NULL */,
                       int32_t mem_kind);
int gpx_sparse_predict_cov(gpx_handle* h, const void* Xs, int64_t M, void* mean /* (M,k) | NULL */, void* cov /* (M,M) */,
                           int32_t mem_kind);
int gpx_sparse_elbo(gpx_handle* h, double* elbo /* (k) */);
int gpx_sparse_info(gpx_handle* h, int64_t* N, int64_t* m, int64_t* k, int64_t* chunk);
int gpx_sparse_elbo_grad(gpx_handle* h, const void* X, const void* y, const void* w /* (N) or NULL */, int64_t N,
                         int32_t mem_kind, double* elbo /* (k) | NULL */, double* grad /* n_ls + 2 */);
int gpx_logdet(gpx_handle* h, double* out);
/* Frees what only the NEXT predict / gradient call would use (the V^T batch, the L^-T buffer of
 * gpx_lml_grad, per-tile partials, compact block buffers, the buffers of the joint-posterior calls); the fit itself (factor, alpha, block
 * inverses) stays valid.  Buffers grow on demand and are otherwise kept for reuse: call this
 * between a gradient and a large predict when N is close to what the card holds (at N = 131072 the
 * factor and L^-T are 137 GB each). */
int gpx_release_scratch(gpx_handle* h);
int gpx_get_timings(gpx_handle* h, gpx_timings* out);
/* Replaces gpx_config.flags of an existing handle (GPX_FLAG_PROFILE on / off between calls: bench.py
 * prices the flag on ONE handle, same buffers).  Groups: applied to every member. */
int gpx_set_flags(gpx_handle* h, int32_t flags);

/* ---- explicit basis functions: a constant, linear or quadratic mean (additive to ABI v6) -------------------
 * Model (Rasmussen & Williams §2.7): y = f(x) + h(x)^T beta + noise, f the zero-mean GP of the handle, beta with a flat
 * prior and marginalised: its uncertainty reaches every predictive variance.  h is evaluated on the RAW inputs the caller
 * passes (not on x / l), and beta is in their units:
 *   GPX_BASIS_CONSTANT  h = [1]                               p = 1
 *   GPX_BASIS_LINEAR    h = [1, x_1 .. x_d]                    p = 1 + d
 *   GPX_BASIS_QUADRATIC h = [1, x_1 .. x_d, x_1^2 .. x_d^2]    p = 1 + 2 d
 * With H = h(X) (N x p) and K = L L^T the matrix the fit factorises anyway:
 *   Z_H = L^-1 H,  z = L^-1 y,  A = Z_H^T Z_H,  beta = A^-1 Z_H^T z  (generalised least squares),  cov(beta) = A^-1
 *   z' = z - Z_H beta,  alpha' = L^-T z' = K^-1 (y - H beta)   (H^T alpha' = 0)
 *   mean(x*) = k*^T alpha' + h(x*)^T beta
 *   cov(x*, x') = k(x*, x') - v*^T v' + u*^T u',   v* = L^-1 k*,  u* = L_A^-1 (h(x*) - Z_H^T v*),  L_A = chol A
 * H^T occupies p of the 64 bordered right-hand-side rows of the fit next to the k targets: k + p <= 64.  beta, L_A, A^-1 and
 * u are fp64 whatever the handle's element type.  gpx_get_alpha returns alpha'; gpx_logdet stays log|K|; gpx_lml_grad
 * returns the PROFILE likelihood -1/2 (y - H beta)^T alpha' - k/2 log|K| - N k / 2 log 2 pi at beta and its exact gradient
 * (the derivative through beta vanishes because H^T alpha' = 0); gpx_lml_grad_full and gpx_lml_grad_paths are gpx_lml_grad
 * on such a fit, as on any plain fit.  Noise weights compose freely (only K changes).
 *
 * gpx_set_basis stores the basis for every later gpx_fit / gpx_fit_predict until it is replaced; GPX_BASIS_NONE clears it.
 * Any other value, or a NULL handle: GPX_E_ARG, the previous setting stays.  An existing fit is not touched.
 * At the fit, before anything is computed and with the previous fit still valid: k + p > 64 or N < p is GPX_E_ARG.  *info
 * of the fit: 0 < *info <= N a pivot of K as before; *info = N + j: pivot j (1-based) of A was not > 0 or not finite (the
 * columns of H are linearly dependent on this data) — the call returns 0 and the handle holds no fit.
 * Served on a fit with a basis: gpx_predict (both routes), gpx_predict_cov, gpx_sample_posterior (around the corrected mean,
 * from the corrected covariance), gpx_score_blocks(_weighted), gpx_forecast_blocks, gpx_get_alpha, gpx_logdet, the three
 * gradient calls.  GPX_E_UNSUPPORTED with "basis" in gpx_last_error, before anything is computed or exchanged and with the
 * previous fit still valid: a fit with a basis set on GPX_MIXED handles, device groups, shards and handles that own a
 * communicator (the set call itself succeeds there), or together with observation kinds or effective path ids; on a fit
 * with a basis: gpx_append, gpx_append_weighted, gpx_append_rows, gpx_remove_rows, gpx_predict_grad and every *_paths
 * posterior call.
 * With no basis set a handle launches the kernels it launched before, allocates nothing more and returns the same bits. */
#define GPX_BASIS_NONE 0
#define GPX_BASIS_CONSTANT 1
#define GPX_BASIS_LINEAR 2
#define GPX_BASIS_QUADRATIC 3
int gpx_set_basis(gpx_handle* h, int32_t basis);
/* The basis of the current fit: its id, p, and — each may be NULL — beta and cov(beta) = A^-1.  A fit without a basis:
 * basis = 0, p = 0, nothing else written.  GPX_E_ARG without a fit. */
int gpx_get_basis(gpx_handle* h, int32_t* basis, int32_t* p, double* beta /* (p,k) host, fp64 */,
                  double* beta_cov /* (p,p) host, fp64 */);

/* ---- row-block sharding over RCCL ------------------------------ */
/* Two process models run the same schedule: the single-process device group above
 * (gpx_config.ndev) and one process per GPU (below).
 * One process per GPU.  Rank 0 calls gpx_comm_unique_id and ships the 128 bytes to
 * the other ranks by any means (the Python host uses torch.distributed); every rank
 * then calls gpx_comm_init on its handle (created with the same world, own rank).  A
 * handle that owns a communicator — even a 1-rank one — runs the sharded schedule. */
int gpx_comm_unique_id(void* id128);
int gpx_comm_init(gpx_handle* h, const void* id128);

/* Portable transport for the same shard schedule: collectives on HOST buffers supplied
 * by the caller (e.g. torch.distributed/gloo); the library stages device<->host around
 * each call.  Used by the multi-process tests that share one GPU (RCCL refuses duplicate
 * devices) and for fabrics without RCCL.  op: 0 = sum, 1 = min.  Return 0 on success. */
typedef struct gpx_host_comm {
  void* ctx;
  int (*bcast)(void* ctx, void* buf, int64_t bytes, int32_t root);
  int (*allgather)(void* ctx, const void* send, void* recv, int64_t bytes_per_rank);
  int (*reduce)(void* ctx, const double* send, double* recv, int64_t count, int32_t root, int32_t op);
  int (*allreduce)(void* ctx, double* buf, int64_t count, int32_t op);
} gpx_host_comm;
int gpx_comm_init_host(gpx_handle* h, const gpx_host_comm* vt);

/* ---- batched path distance (reference: trajectories.calc_distance,
 * GPmap.py:114-121, the inner loop of kmeansclustering GPmap.py:72-80) ---------------- */
/* D (P,C)[p][c] = sum_{i<L} || paths[p][i] - cents[c][i] ||_2 with paths (P,L,2) and cents
 * (C,L,2) arrays of (x,y), fp64, L <= 64.  mem_kind as in gpx_fit (device pointers must
 * live on the current HIP device). */
int gpx_path_distance(const double* paths, int64_t P, const double* cents, int64_t C, int32_t L,
                      double* D, int32_t mem_kind);

/* ---- kernel unit-test entry points (host buffers, fp64) ------------------------- */
/* K (na,nb) = sf2 k(A,B) (+ diag_add on the diagonal when B == NULL, i.e. B = A). */
int gpx_kernel_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb,
                      int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                      double diag_add, double* K /* (na, nb or na) */);
/* kernel unit-test entry point (host buffers, fp64): G (d, na, nb)[j][a][b] = d k(A_a, B_b) / d A_aj.
 * GPX_KERNEL_RBF and GPX_KERNEL_MATERN52 only (its kernel set as first published; any other id is GPX_E_ARG). */
int gpx_kernel_grad_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                           const double* lengthscale, int32_t n_ls, double sf2, double* G);
/* The same for every kernel family (additive to ABI v6): RBF, Matern-5/2, Matern-3/2; GPX_KERNEL_MATERN12 returns
 * GPX_E_UNSUPPORTED (gpx_last_error(NULL) says why) and leaves G untouched. */
int gpx_kernel_deriv_matrix(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                            const double* lengthscale, int32_t n_ls, double sf2, double* G);
/* kernel unit-test entry point (host buffers, fp64; additive to ABI v6): G (n_ls, na, nb)[c][a][b] = the derivative by
 * log lengthscale[c] of the covariance between an observation of kind ka[a] at A_a and one of kind kb[b] at B_b (kinds as
 * in gpx_set_observation_kinds; ka / kb == NULL: all values) — what gpx_lml_grad_full contracts with K^-1.  n_ls == 1: the
 * one lengthscale of every dimension.  A kind outside [-1, d): GPX_E_ARG.  GPX_KERNEL_MATERN12 with any kind >= 0 returns
 * GPX_E_UNSUPPORTED (gpx_last_error(NULL) says why) and leaves G untouched. */
int gpx_kernel_dl_matrix(int32_t kernel, const double* A, const int32_t* ka, int64_t na, const double* B,
                         const int32_t* kb, int64_t nb, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                         double* G /* (n_ls, na, nb) */);
/* K (na, nb) host, fp64 = sf2 k(A_i, B_j; l) + [ga_i == gb_j and ga_i >= 0] sg2 k(A_i, B_j; l_path): the covariance of
 * observations with path ids (gpx_set_path_groups), by the fit's builder; no diagonal term.  n_ls, n_ls_path: 1 or d.
 * dtype GPX_F64 or GPX_F32 (the fp32 builder on the rounded inputs, returned widened). */
int gpx_kernel_path_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na, const double* B,
                           const int32_t* gb, int64_t nb, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                           const double* ls_path, int32_t n_ls_path, double sg2, double* K);
/* kernel unit-test entry point (host buffers; additive to ABI v6): G (d, na, nb), G[j][a][b] = d / d A_aj of the entry
 * K[a][b] of gpx_kernel_path_matrix — the d K* rows of gpx_predict_grad_paths, by its builder.  Arguments and GPX_E_ARG as
 * gpx_kernel_path_matrix; GPX_KERNEL_MATERN12: GPX_E_UNSUPPORTED (not differentiable), as gpx_kernel_deriv_matrix.  G is
 * written only on success. */
int gpx_kernel_path_grad_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na,
                                const double* B, const int32_t* gb, int64_t nb, int32_t d, const double* lengthscale,
                                int32_t n_ls, double sf2, const double* ls_path, int32_t n_ls_path, double sg2,
                                double* G /* (d, na, nb) */);
/* K (na, nb) host, fp64 = the covariance between an observation of kind ka[a] at A_a and one of kind kb[b] at B_b (kinds as
 * in gpx_set_observation_kinds; ka / kb == NULL: all values), by the fit's rectangular builder with kinds on rows and
 * columns — the left part of rows appended by gpx_append_rows; no diagonal term.  n_ls: 1 or d.  dtype GPX_F64 or GPX_F32
 * (the fp32 builder on the rounded inputs, returned widened).  Refusals as gpx_kernel_dl_matrix's. */
int gpx_kernel_mixed_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ka, int64_t na, const double* B,
                            const int32_t* kb, int64_t nb, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                            double* K);
/* kernel unit-test entry point (host buffers; additive to ABI v6): G (D2, na, nb), G[(i,j)][a][b] = the second derivative by
 * A_ai and A_aj of the covariance of a value at A_a with the observation b — the row blocks of gpx_predict_hess(_paths), by
 * its builder (pairs i <= j row-major, D2 = d (d + 1) / 2).  What the observation b is:
 *   ga == NULL, side_b == NULL   a value: the plain build (ls_path, n_ls_path, sg2 are not read)
 *   ga == NULL, side_b != NULL   an observation of kind side_b[b] in [-1, d) (gpx_set_observation_kinds): the KINDS build
 *   ga != NULL                   a value with path id side_b[b], the rows' ids in ga (all >= -1; ls_path, n_ls_path = 1 or d
 *                                and sg2 as gpx_kernel_path_matrix's): the build with path ids
 * n_ls: 1 or d; dtype GPX_F64 or GPX_F32 (the fp32 builder on the rounded inputs, returned widened).  GPX_E_ARG as
 * gpx_kernel_path_grad_matrix / gpx_kernel_mixed_matrix; GPX_E_UNSUPPORTED (gpx_last_error(NULL) says why) for
 * GPX_KERNEL_MATERN32, GPX_KERNEL_MATERN12 and d > 8.  G is written only on success. */
int gpx_kernel_hess_matrix(int32_t kernel, int32_t dtype, const double* A, const int32_t* ga, int64_t na, const double* B,
                           const int32_t* side_b, int64_t nb, int32_t d, const double* lengthscale, int32_t n_ls, double sf2,
                           const double* ls_path, int32_t n_ls_path, double sg2, double* G /* (D2, na, nb) */);
/* kernel unit-test entry point (host buffers, fp64; additive to ABI v6): G (1 + n_ls_path, na, nb): G[0][a][b] = [ga_a == gb_b
 * and ga_a >= 0] sg2 k(A_a, B_b; l_path), the within-path term of gpx_kernel_path_matrix, and G[1 + c] its derivative by
 * log l_path,c (n_ls_path == 1: by the one l_path) — what gpx_lml_grad_paths contracts with K^-1, by the device function its
 * epilogues call.  Every family, GPX_KERNEL_MATERN12 included (its derivative is 0 at coincident points).  GPX_E_ARG, before
 * any device call: a NULL pointer, na or nb < 1, d outside [1, 32], n_ls_path not 1 or d, an unknown family, sg2 negative or
 * not finite, a lengthscale not > 0 or not finite, an id below -1. */
int gpx_kernel_path_dtheta_matrix(int32_t kernel, const double* A, const int32_t* ga, int64_t na, const double* B,
                                  const int32_t* gb, int64_t nb, int32_t d, const double* ls_path, int32_t n_ls_path,
                                  double sg2, double* G /* (1 + n_ls_path, na, nb) */);
/* kernel unit-test entry point (host buffers; additive to ABI v6): the evaluation kernel of gpx_pathwise_eval apart from any
 * factor.  out (C, M)[c][m] = sqrt(sf2 / F) sum_f (W[c][f] cos theta_f(Xq_m) + W[c][F + f] sin theta_f(Xq_m))
 * + sum_n sf2 k(Xq_m, X_n) V[c][n], with Omega (F, d), W (C, 2F), V (C, N) as given.  dtype GPX_F64 or GPX_F32 (the fp32
 * kernel on the rounded inputs, phases still in fp64, returned widened).  GPX_E_ARG, before any device call: a NULL
 * pointer, a size < 1, d outside [1, 32], n_ls not 1 or d, an unknown family or dtype. */
int gpx_pathwise_eval_raw(int32_t kernel, int32_t dtype, const double* Xq, int64_t M, const double* X, int64_t N, int32_t d,
                          const double* ls, int32_t n_ls, double sf2, const double* Omega, int64_t F,
                          const double* W /* (C,2F) */, const double* V /* (C,N) */, int64_t C, double* out /* (C,M) */);
/* in-place lower Cholesky of A (n,n), lda = n; n multiple of 64.  The strictly upper
 * triangle is never read and is scratch on return (diagonal tiles are updated whole).
 * block = panel width (0 = default).  *info = p > 0: the first failing pivot, 1-based (LAPACK: the leading minor of
 * order p is the first that is not positive definite; a NaN pivot counts as failing); rows [0, p - 1) of the factor are
 * valid.  Never negative. */
int gpx_potrf(double* A, int64_t n, int32_t block, int64_t* info);
/* X (m,nb) <- X L^-T, L (nb,nb) lower; m, nb multiples of 64. */
int gpx_trsm(double* X, int64_t m, const double* L, int64_t nb);
/* C (m,n) -= A (m,k) B(n,k)^T.  lower != 0: only tiles on/below the diagonal
 * (m == n required).  m,n multiples of 128, k multiple of 16. */
int gpx_gemm_nt(double* C, int64_t m, int64_t n, const double* A, const double* B, int64_t k,
                int32_t lower);
/* The TN product of the inducing-point fit: the lower triangle of C (n,n) = X^T X (accumulate == 0) or += X^T X, X (rows,n)
 * row-major; nothing above the diagonal is written.  n a multiple of 64, rows >= 1. */
int gpx_syrk_tn(double* C, int64_t n, const double* X, int64_t rows, int32_t accumulate);
/* That contraction alone on zero-filled resident operands, `iters` repeats after a warm-up; *ms_per_call = the mean time.
 * route 0: the TN kernel as the fit launches it; 1: a transpose of X, then the NT tile engine (128-tiles, lower); 2: that NT
 * launch alone.  n a multiple of 128 (<= 16384), rows a multiple of 64.  tools/sparse_bench.py. */
int gpx_debug_syrk_tn_bench(int64_t n, int64_t rows, int32_t route, int32_t iters, double* ms_per_call);
/* The derivative contraction of gpx_sparse_elbo_grad alone (its kernel's unit entry; host buffers, as gpx_kernel_dl_matrix):
 * out[t] = sum_{i < na, j < nb} W[i][j] (dK / dlog theta_t)(A_i, B_j) for theta = (lengthscale[0..n_ls), sf2), K = sf2 k(A, B);
 * W (na,nb) row-major, out n_ls + 1 entries.  Two calls agree bit for bit; a coincident pair contributes its finite value. */
int gpx_cross_dtheta_contract(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                              const double* W /* (na, nb) */, const double* lengthscale, int32_t n_ls, double sf2,
                              double* out /* n_ls + 1 */);
/* That kernel and its reduction alone on zero-filled resident operands (W at the leading dimension of a fit with m = cols),
 * `iters` repeats after a warm-up; *ms_per_call = the mean time.  rows (<= 2^22) and cols (<= 65536) multiples of 64.
 * tools/sparse_grad_bench.py. */
int gpx_debug_cross_dtheta_bench(int32_t kernel, int64_t rows, int64_t cols, int32_t d, int32_t n_ls, int32_t iters,
                                 double* ms_per_call);
/* fp64 MFMA layout probe: D (16,16) = A (16,4) B (4,16) through one
 * v_mfma_f64_16x16x4_f64. */
int gpx_mfma_probe(const double* A, const double* B, double* D);
/* the same through one v_mfma_f32_16x16x4_f32 (different accumulator row map). */
int gpx_mfma_probe_f32(const float* A, const float* B, float* D);
/* microbenchmarks quoted beside the rooflines: sustained fp64 MFMA
 * TFLOP/s of a register-resident loop and HBM GB/s of a streaming copy. */
int gpx_microbench(double* mfma_tflops, double* copy_gbs);
/* host-only replay of the tile maps of the trailing-update kernels (no GPU needed): kind 0 =
 * lower triangle of a tm x tm grid of 128x128 tiles (unsharded SYRK), kind 1 = the
 * block-cyclic staircase of a rank's tm x tn grid (P ranks, tpb tiles per row block, offset
 * c: local tile row ti owns tj <= ((ti/tpb)*P + c)*tpb + ti%tpb), kind 2 = the fused trailing
 * update (strip of tn tile columns first, then the triangle beyond it; tm x tm lower).  Writes (ti, tj) int32
 * pairs in launch order into out[2*cap]; returns their count through *count.  Test hook:
 * every owned tile must appear exactly once. */
int gpx_debug_tile_map(int32_t kind, int64_t tm, int64_t tn, int32_t P, int32_t tpb, int32_t c,
                       int32_t* out, int64_t cap, int64_t* count);
/* the staircase of a rank under either dealing of the row blocks (round 4; cyclic: block g on rank g mod P; snake: rounds
 * of 2 P blocks dealt 0 .. P-1, P-1 .. 0 — balanced row work): local tile row ti belongs to block number lbf + ti / tpb of
 * rank r, tile column 0 to block gc0 of the matrix.  Same output as gpx_debug_tile_map kind 1. */
int gpx_debug_stair_map(int64_t tm, int64_t tn, int32_t P, int32_t tpb, int32_t r, int32_t lbf, int32_t gc0,
                        int32_t snake, int32_t* out, int64_t cap, int64_t* count);
/* the dealing itself: owner[g], local[g] (index of block g among its owner's blocks) for g < nblk, and
 * upto[g * P + r] = number of blocks of rank r with index <= g.  Test hook (tests/test_tile_maps.py). */
int gpx_debug_deal(int32_t P, int32_t snake, int64_t nblk, int32_t* owner, int64_t* local, int64_t* upto);
/* host-only exercise of the rendezvous the LOCAL transport's rank threads use (no GPU needed):
 * P threads run `rounds` barrier rounds, each checking that every rank published the round
 * number; if abort_rank >= 0 that rank leaves at round abort_round and aborts the hub instead
 * of arriving.  *completed = rounds every surviving rank finished; returns 0 when all threads
 * came back (no deadlock) and saw consistent data, GPX_E_COMM otherwise. */
int gpx_debug_local_hub(int32_t P, int32_t rounds, int32_t abort_rank, int32_t abort_round,
                        int32_t* completed);

/* Test hook (process-wide): seed != 0 puts a short bounded spin kernel in front of a random third
 * of the library's launches, on the stream of that launch, so that its streams race each other
 * differently per seed; 0 turns it off.  Results must not change by a bit — every cross-stream
 * dependency is an event (tests/test_delay_gpu.py). */
int gpx_debug_set_delay(uint64_t seed);
/* Diagnostics: the dense tile engine alone, operands resident in HBM (zero-filled): C (n,n) -= / =
 * A (n,k) B(n,k)^T, lower != 0: the triangular (SYRK-shaped) launch of the trailing update; mode 0:
 * C -= (atomic epilogue), 1: C = (plain stores), 2: C -= through one Strassen level (lower 0, n multiple of 256, k of
 * 64), 3: through two levels (lower 0, n multiple of 512, k of 128).  dtype GPX_F64 / GPX_F32; n multiple of 128,
 * k of 32.  One warm-up launch, then the mean of `iters` back-to-back launches in ms. */
int gpx_debug_gemm_bench(int32_t dtype, int64_t n, int64_t k, int32_t lower, int32_t mode, int32_t iters,
                         double* ms_per_launch);
/* The environment switches as the library resolves them right now (additive to ABI v6; no device needed, none touched):
 * a fresh snapshot of every switch of INTEGRATION.md §7 — the ones a handle reads when it is created as gpx_create
 * would resolve them — as one "NAME=value\n" line each; an unset switch whose default is a rule of its own (tri-states,
 * GPX_NB_PRED, GPX_RCCL_PATH) prints as "unset".  Writes at most n - 1 characters and a terminating 0 into buf (nothing
 * when buf is NULL or n <= 0) and returns the length of the whole text, as snprintf does. */
int gpx_debug_env(char* buf, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H_ */
