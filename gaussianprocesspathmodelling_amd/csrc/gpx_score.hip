// gpx_score.hip — joint log predictive density of blocks of query points (gpx_score_blocks, include/gpx.h): a path is a
// block of Lg consecutive query points, and its density under the fitted GP needs the Lg x Lg posterior covariance
//     S_g = K(X_g, X_g) - V_g^T V_g + diag_add I,    V^T = K* L^-T  (the rows predict's variance solve leaves behind),
// not the M x M joint covariance of all query points.  Two kernels per batch of V^T:
//
//   block_gram_kernel   grid (blocks of the batch) x (column slices of V^T).  A workgroup streams the Lg rows of one block
//                       over its slice in chunks of 64 columns: 16-byte global loads into registers (the next chunk is in
//                       flight while this one is multiplied), converted to fp64 and staged in LDS, then the lower 16 x 16
//                       tiles of the LP x LP Gram (LP = 16 ceil(Lg / 16)) accumulate through v_mfma_f64_16x16x4_f64.  The
//                       A operand of tile row I and the B operand of tile column J are the same LDS read (a Gram), so a
//                       k-step costs LP/16 ds_read_b64 per lane for up to 10 MFMAs.  The four waves split the 64 columns
//                       of a chunk; their sums meet in LDS in wave order and leave as ONE fp64 partial per slice.  The slice
//                       count depends on Npad only and nothing is accumulated atomically, so a block's numbers do not
//                       depend on the number of blocks, on its position or on the batch it falls in.
//   block_score_kernel  one workgroup per block, fp64 whatever the element type: partials summed in slice order,
//                       S = sf2 k(X_g, X_g) + diag_add I - Gram from the scaled queries (gpx_cov.h), Cholesky of S in
//                       LDS, r = ys - mean, forward solve of the k columns, maha / logdet / logp.  A pivot that is not
//                       > 0 makes the block's outputs NaN and lowers *bad to its 1-based index.  On a fit with path ids
//                       the block is a new path: S gains sg2 k(X_g, X_g; l_path).
//   block_forecast_kernel  gpx_forecast_blocks: the same S for Lo observed + Lp forecast rows, the same Cholesky stopped
//                       after Lo columns, one Schur update (built from the same device functions).
//
// LDS row slab: row stride 66 doubles (= 2 mod 32), so the 16 rows x 2 columns a half-wave reads for one MFMA operand
// (ds_read_b64, 64 four-byte banks) fall on 32 distinct bank pairs.
#include <algorithm>
#include <climits>

#include "gpx_cov.h"
#include "gpx_internal.h"

namespace gpx {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int GC = 64;         // columns of V^T per staged chunk (every padded N is a multiple of 128)
constexpr int GLD = GC + 2;    // row stride of the slab in doubles
constexpr int MAX_SLICES = 8;  // column slices of V^T per block
constexpr int SLD = 65;        // row stride of S and of the residuals in block_score_kernel

template <typename T>
struct Piece {  // 16 bytes of a row of V^T
  typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

template <typename T, int NT>
__global__ __launch_bounds__(256) void block_gram_kernel(const T* __restrict__ VT, int64_t ld, int Lg, int cps, int nch,
                                                        double* __restrict__ part) {
  constexpr int LP = 16 * NT, NTILES = NT * (NT + 1) / 2;
  constexpr int PER = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr int PPR = GC / PER;             // pieces per row of a chunk (32 | 16)
  constexpr int RPP = 256 / PPR;            // rows per pass of the workgroup (8 | 16)
  constexpr int NPASS = LP / RPP;
  typedef typename Piece<T>::type piece_t;
  __shared__ __attribute__((aligned(16))) double slab[LP * GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pc = tid % PPR, pr = tid / PPR;
  const int c0 = (int)blockIdx.y * cps, c1 = min(nch, c0 + cps);
  const T* base = VT + (int64_t)blockIdx.x * Lg * ld;

  for (int e = Lg * GLD + tid; e < LP * GLD; e += 256) slab[e] = 0.0;  // rows [Lg, LP): never staged
  __syncthreads();

  piece_t pre[NPASS];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int r = pr + RPP * i;
      if (r < Lg) pre[i] = *reinterpret_cast<const piece_t*>(base + (int64_t)r * ld + (int64_t)c * GC + pc * PER);
    }
  };
  v4d acc[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

  if (c0 < c1) fetch(c0);
  for (int c = c0; c < c1; ++c) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int r = pr + RPP * i;
      if (r < Lg) {
        double* dst = slab + r * GLD + pc * PER;
#pragma unroll
        for (int u = 0; u < PER; u += 2)
          *reinterpret_cast<v2d*>(dst + u) = (v2d){(double)pre[i][u], (double)pre[i][u + 1]};
      }
    }
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
#pragma unroll
    for (int ks = 0; ks < GC / 16; ++ks) {
      const int kk = wave * (GC / 4) + 4 * ks + (lane >> 4);
      double a[NT];
#pragma unroll
      for (int I = 0; I < NT; ++I) a[I] = slab[(I * 16 + (lane & 15)) * GLD + kk];
      int t = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], a[J], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }

  // the four waves' sums, in wave order, through the (now free) slab: NTILES * 256 <= LP * GLD doubles
  double* red = slab;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < NTILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = t * 256 + r * 64 + lane;
          red[e] = w == 0 ? acc[t][r] : red[e] + acc[t][r];
        }
    }
    __syncthreads();
  }
  // accumulator register r of lane l = element ((l >> 4) + 4 r, l & 15) of its tile (gpx_mfma_probe pins this)
  double* out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (LP * LP);
  for (int e = tid; e < NTILES * 256; e += 256) {
    const int t = e >> 8, r = (e >> 6) & 3, l = e & 63;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    const int J = t - I * (I + 1) / 2;
    out[(I * 16 + (l >> 4) + 4 * r) * LP + J * 16 + (l & 15)] = red[e];
  }
}

// sum of the four lanes of a quad, the same bits in each of them
__device__ __forceinline__ double quad_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// ---- the device code block_score_kernel and block_forecast_kernel share ----------------------------------------------------

// Lower triangle of S (Lg x Lg, stride SLD) of the block whose first row is row0: sf2 k + [sg2 k(., .; l_path)] - Gram, the
// partials summed in slice order; + diag_add (times wq[i] if given) on the diagonal of the rows i < nd.  sg2 > 0 (a fit with
// path ids: the block is a new path) adds the within-path term from the scaled queries with q_c = (l_c / l_path,c)^2.
// U != null (a fit with basis functions, gpx_basis.hip): + u_i . u_j over pu entries; null: the same bits as without it.
template <typename T, int KERNEL>
__device__ __forceinline__ void block_build_s(double* Sm, const double* pb, int S, int LP, const T* __restrict__ Qs,
                                              int64_t row0, int d, int Lg, int nd, double sf2, double sg2,
                                              const double* __restrict__ q, double diag_add, const T* __restrict__ wq,
                                              const double* __restrict__ U, int pu) {
  for (int e = threadIdx.x; e < Lg * Lg; e += 256) {
    const int i = e / Lg, j = e - i * Lg;
    if (j > i) continue;
    double gram = 0.0;
    for (int s = 0; s < S; ++s) gram += pb[(int64_t)s * (LP * LP) + i * LP + j];
    double r2 = 0.0;
    for (int c = 0; c < d; ++c) {
      const double df = (double)Qs[(row0 + i) * d + c] - (double)Qs[(row0 + j) * d + c];
      r2 += df * df;
    }
    double v = cov::value<KERNEL, double>(r2, sf2);
    if (sg2 > 0.0) {  // (the same for every thread)
      double rp2 = 0.0;
      for (int c = 0; c < d; ++c) {
        const double df = (double)Qs[(row0 + i) * d + c] - (double)Qs[(row0 + j) * d + c];
        rp2 += q[c] * (df * df);
      }
      v += cov::value<KERNEL, double>(rp2, sg2);
    }
    if (i == j && i < nd) v += wq ? diag_add * (double)wq[row0 + i] : diag_add;  // per-point weight of the added diagonal
    v -= gram;
    if (U) {  // a fit with basis functions: + u_i . u_j (U: 64 fp64 per query row, from the batch's first row)
      double uu = 0.0;
      for (int c = 0; c < pu; ++c) uu += U[(row0 + i) * 64 + c] * U[(row0 + j) * 64 + c];
      v += uu;
    }
    Sm[i * SLD + j] = v;
  }
}

// Left-looking Cholesky of the columns j < nc over ALL Lg rows: row ci of column j by the four lanes of a quad (the
// contraction index dealt mod 4).  nc == Lg: the factor of S.  nc < Lg: L_oo in the leading nc x nc block,
// B = S_po L_oo^-T in the rows below it, the trailing block untouched.  false: a pivot was not > 0 (the same for every thread).
__device__ __forceinline__ bool block_chol_cols(double* Sm, int Lg, int nc, double* piv, double& half_logdet) {
  const int tid = threadIdx.x, ci = tid >> 2, q = tid & 3;
  for (int j = 0; j < nc; ++j) {
    const bool mine = ci >= j && ci < Lg;
    double acc = 0.0;
    if (mine)
      for (int p = q; p < j; p += 4) acc += Sm[ci * SLD + p] * Sm[j * SLD + p];
    acc = quad_sum(acc);
    const double v = mine ? Sm[ci * SLD + j] - acc : 0.0;
    if (ci == j && q == 0) *piv = v;
    __syncthreads();
    const double dj = *piv;
    if (!(dj > 0.0)) return false;
    const double lj = sqrt(dj);
    if (mine && q == 0) Sm[ci * SLD + j] = ci == j ? lj : v / lj;
    half_logdet += log(lj);
    __syncthreads();
  }
  return true;
}

// w = L^-1 r for the leading n x n block of the factor: column ci by the lanes of quad ci (all in one wave); returns this
// thread's |w_ci|^2 (ci < k)
__device__ __forceinline__ double block_forward(const double* Sm, double* Wm, int n, int k) {
  const int tid = threadIdx.x, ci = tid >> 2, q = tid & 3;
  double mh = 0.0;
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
    if (ci < k)
      for (int p = q; p < i; p += 4) acc += Sm[i * SLD + p] * Wm[p * SLD + ci];
    acc = quad_sum(acc);
    double w = 0.0;
    if (ci < k) {
      w = (Wm[i * SLD + ci] - acc) / Sm[i * SLD + i];
      mh += w * w;
    }
    if (ci < k && q == 0) Wm[i * SLD + ci] = w;
    __syncthreads();
  }
  return mh;
}

constexpr double LOG_2PI = 1.83787706640934548356065947281;

template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void block_score_kernel(const double* __restrict__ part, int S, int LP,
                                                         const T* __restrict__ Qs, int d, const T* __restrict__ ys,
                                                         const T* __restrict__ mean, int k, int Lg, double sf2,
                                                         double diag_add, T* __restrict__ logp, T* __restrict__ maha,
                                                         T* __restrict__ logdet, int64_t g0, int* __restrict__ bad,
                                                         const T* __restrict__ wq, double sg2,
                                                         const double* __restrict__ q, const double* __restrict__ U,
                                                         int pu) {
  __shared__ double Sm[64 * SLD];  // S, then its Cholesky factor (lower)
  __shared__ double Wm[64 * SLD];  // residuals r (Lg x k), then L^-1 r
  __shared__ double piv;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, row0 = b * Lg;
  block_build_s<T, KERNEL>(Sm, part + b * S * (int64_t)(LP * LP), S, LP, Qs, row0, d, Lg, Lg, sf2, sg2, q, diag_add, wq, U,
                           pu);
  for (int e = tid; e < Lg * k; e += 256) {
    const int i = e / k, c = e - i * k;
    Wm[i * SLD + c] = (double)ys[row0 * k + e] - (double)mean[row0 * k + e];
  }
  __syncthreads();

  const int ci = tid >> 2, qd = tid & 3;
  double half_logdet = 0.0;
  const bool ok = block_chol_cols(Sm, Lg, Lg, &piv, half_logdet);
  double mh = 0.0;
  if (ok) mh = block_forward(Sm, Wm, Lg, k);
  const double nan = __builtin_nan("");
  const int64_t g = g0 + b;
  if (ci < k && qd == 0) {
    maha[g * k + ci] = (T)(ok ? mh : nan);
    logp[g * k + ci] = (T)(ok ? -0.5 * mh - half_logdet - 0.5 * Lg * LOG_2PI : nan);
  }
  if (tid == 0) {
    logdet[g] = (T)(ok ? 2.0 * half_logdet : nan);
    if (!ok) atomicMin(bad, (int)(g + 1));
  }
}

// gpx_forecast_blocks: one workgroup per block of Lo observed rows, then Lp rows to forecast (Lg = Lo + Lp <= 64).  The score
// kernel stopped after Lo columns plus one Schur update: the joint S with diag_add on the observed rows only, the Cholesky
// of its first Lo columns over all rows (L_oo and B = S_po L_oo^-T in place), w = L_oo^-1 (yo - mean_o), then
//   fmean = mean_p + B w,   fcov = S_pp - B B^T (the lower triangle computed, both halves written),   fvar = diag(fcov),
//   flogp = the joint log-density of the observed rows (what block_score_kernel gives for them alone).
// Every sum runs in index order inside one thread (or one quad): nothing depends on G, the position or the batch.
template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void block_forecast_kernel(const double* __restrict__ part, int S, int LP,
                                                            const T* __restrict__ Qs, int d, const T* __restrict__ yo,
                                                            const T* __restrict__ mean, int k, int Lo, int Lp, double sf2,
                                                            double sg2, const double* __restrict__ q, double diag_add,
                                                            T* __restrict__ fmean, T* __restrict__ fcov,
                                                            T* __restrict__ fvar, T* __restrict__ flogp, int64_t g0,
                                                            int* __restrict__ bad, const double* __restrict__ U,
                                                            int pu) {
  __shared__ double Sm[64 * SLD];  // S; then L_oo, B below it, S_pp
  __shared__ double Wm[64 * SLD];  // rows < Lo: yo - mean_o, then w; rows >= Lo: mean_p
  __shared__ double piv;
  const int tid = threadIdx.x, Lg = Lo + Lp;
  const int64_t b = blockIdx.x, row0 = b * Lg;
  block_build_s<T, KERNEL>(Sm, part + b * S * (int64_t)(LP * LP), S, LP, Qs, row0, d, Lg, Lo, sf2, sg2, q, diag_add,
                           (const T*)nullptr, U, pu);
  for (int e = tid; e < Lg * k; e += 256) {
    const int i = e / k, c = e - i * k;
    const double m = (double)mean[row0 * k + e];
    Wm[i * SLD + c] = i < Lo ? (double)yo[b * Lo * k + e] - m : m;
  }
  __syncthreads();

  const int ci = tid >> 2, qd = tid & 3;
  double half_logdet = 0.0;
  const bool ok = block_chol_cols(Sm, Lg, Lo, &piv, half_logdet);
  double mh = 0.0;
  if (ok) mh = block_forward(Sm, Wm, Lo, k);
  const double nan = __builtin_nan("");
  const int64_t g = g0 + b;
  for (int e = tid; e < Lp * k; e += 256) {
    const int i = e / k, c = e - i * k;
    double acc = Wm[(Lo + i) * SLD + c];
    for (int p = 0; p < Lo; ++p) acc += Sm[(Lo + i) * SLD + p] * Wm[p * SLD + c];
    fmean[(g * Lp + i) * k + c] = (T)(ok ? acc : nan);
  }
  for (int e = tid; e < Lp * Lp; e += 256) {
    const int i = e / Lp, j = e - i * Lp;
    if (j > i) continue;
    double acc = Sm[(Lo + i) * SLD + Lo + j];
    for (int p = 0; p < Lo; ++p) acc -= Sm[(Lo + i) * SLD + p] * Sm[(Lo + j) * SLD + p];
    const T v = (T)(ok ? acc : nan);
    if (fcov) {
      fcov[(g * Lp + i) * Lp + j] = v;
      fcov[(g * Lp + j) * Lp + i] = v;
    }
    if (fvar && i == j) fvar[g * Lp + i] = v;
  }
  if (flogp && ci < k && qd == 0) flogp[g * k + ci] = (T)(ok ? -0.5 * mh - half_logdet - 0.5 * Lo * LOG_2PI : nan);
  if (tid == 0 && !ok) atomicMin(bad, (int)(g + 1));
}

}  // namespace

int score_slices(int64_t npad) {
  const int64_t nch = npad / GC;
  return (int)std::min<int64_t>(MAX_SLICES, std::max<int64_t>(1, (nch + 7) / 8));
}

template <typename T>
void launch_block_gram(const T* VT, int64_t ld, int64_t nblk, int Lg, int64_t npad, double* part, hipStream_t st) {
  debug_delay(st);
  const int nch = (int)(npad / GC), S = score_slices(npad), cps = (nch + S - 1) / S;
  const dim3 grid((unsigned)nblk, (unsigned)S), block(256);
  switch ((Lg + 15) / 16) {
    case 1: hipLaunchKernelGGL((block_gram_kernel<T, 1>), grid, block, 0, st, VT, ld, Lg, cps, nch, part); break;
    case 2: hipLaunchKernelGGL((block_gram_kernel<T, 2>), grid, block, 0, st, VT, ld, Lg, cps, nch, part); break;
    case 3: hipLaunchKernelGGL((block_gram_kernel<T, 3>), grid, block, 0, st, VT, ld, Lg, cps, nch, part); break;
    default: hipLaunchKernelGGL((block_gram_kernel<T, 4>), grid, block, 0, st, VT, ld, Lg, cps, nch, part); break;
  }
}

template <typename T>
void launch_block_score(int kernel, const double* part, int64_t nblk, int Lg, int64_t npad, const T* Qs, int d,
                        const T* ys, const T* mean, int k, double sf2, double diag_add, T* logp, T* maha, T* logdet,
                        int64_t g0, int* bad, hipStream_t st, const T* wq, double sg2, const double* q, const double* U,
                        int pu) {
  debug_delay(st);
  const int S = score_slices(npad), LP = score_lp(Lg);
  cov::dispatch(kernel, [&](auto fam) {
    hipLaunchKernelGGL((block_score_kernel<T, fam>), dim3((unsigned)nblk), dim3(256), 0, st, part, S, LP, Qs, d, ys, mean,
                       k, Lg, sf2, diag_add, logp, maha, logdet, g0, bad, wq, sg2, q, U, pu);
  });
}

template <typename T>
void launch_block_forecast(int kernel, const double* part, int64_t nblk, int Lo, int Lp, int64_t npad, const T* Qs, int d,
                           const T* yo, const T* mean, int k, double sf2, double sg2, const double* q, double diag_add,
                           T* fmean, T* fcov, T* fvar, T* flogp, int64_t g0, int* bad, hipStream_t st, const double* U,
                           int pu) {
  debug_delay(st);
  const int S = score_slices(npad), LP = score_lp(Lo + Lp);
  cov::dispatch(kernel, [&](auto fam) {
    hipLaunchKernelGGL((block_forecast_kernel<T, fam>), dim3((unsigned)nblk), dim3(256), 0, st, part, S, LP, Qs, d, yo,
                       mean, k, Lo, Lp, sf2, sg2, q, diag_add, fmean, fcov, fvar, flogp, g0, bad, U, pu);
  });
}

#define GPX_INSTANTIATE_SCORE(T)                                                                                       \
  template void launch_block_gram<T>(const T*, int64_t, int64_t, int, int64_t, double*, hipStream_t);                 \
  template void launch_block_score<T>(int, const double*, int64_t, int, int64_t, const T*, int, const T*, const T*,  \
                                      int, double, double, T*, T*, T*, int64_t, int*, hipStream_t, const T*, double,  \
                                      const double*, const double*, int);                                              \
  template void launch_block_forecast<T>(int, const double*, int64_t, int, int, int64_t, const T*, int, const T*,      \
                                         const T*, int, double, double, const double*, double, T*, T*, T*, T*, int64_t, \
                                         int*, hipStream_t, const double*, int);
GPX_INSTANTIATE_SCORE(double)
GPX_INSTANTIATE_SCORE(float)

}  // namespace gpx
