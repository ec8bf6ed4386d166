// gpx_basis.hip — explicit basis functions with marginalised coefficients (gpx_set_basis, include/gpx.h; DESIGN.md §3.4m;
// Rasmussen & Williams §2.7).  With h(x) the basis (p functions of the RAW inputs: 1 | 1, x_c | 1, x_c, x_c^2), H = h(X) and
// K = L L^T the factor of the fit:
//     Z_H = L^-1 H,  z = L^-1 y,  A = Z_H^T Z_H,  beta = A^-1 Z_H^T z,  z' = z - Z_H beta,
//     mean(x*) = k*^T K^-1 (y - H beta) + h(x*)^T beta,   cov(x*, x') = k(x*, x') - v*^T v' + u*^T u',
//     u* = L_A^-1 (h(x*) - Z_H^T v*),  v* = L^-1 k*,  L_A = chol A.
// H^T rides through the factorisation in rows [k, k + p) of the 64 bordered right-hand-side rows (they are solved whether
// they hold anything or not) and comes out as Z_H^T; Z_H^T v* is rows [k, k + p) of the mean product predict makes anyway.
// What is left for this file is small and memory- or latency-bound, plain vector code in fp64 whatever the element type:
//
//   basis_rows_kernel      H^T into rows [k, k + p) of the bordered block (beside launch_pack_rhs)
//   bordered_gram_kernel   G = zT zT^T (64 x 64) per column slice of 1024; the slices are a function of Npad only and are
//                          summed in slice order by the solve — no atomics, the same bits on every run
//   beta_solve_kernel      one workgroup: A and Z_H^T z out of G, L_A, beta, A^-1 into the handle's state block; a pivot
//                          of A that is not > 0 or not finite goes to the fit's info word as N + its 1-based place
//   basis_project_kernel   zT[c] -= sum_j beta[j][c] zT[k + j] for c < k: every later reader of zT sees z'
//   basis_epilogue_kernel  per query point: mean += h^T beta, var += |u|^2, u kept for the joint calls
//   cov_add_uut_kernel     lower triangle of Sigma += U U^T (the caller mirrors it)
//
// State block (fp64, BASIS_STATE doubles): beta[j * 64 + c] | L_A[i * 64 + j] (lower) | A^-1[i * 64 + j].
#include "gpx_internal.h"

namespace gpx {
namespace {

constexpr int BR = 64;           // bordered rows = stride of the state block's three matrices
constexpr int GRAM_COLS = 1024;  // columns of zT per slice of the Gram
constexpr int GSLD = 65;         // LDS row stride of a staged 64 x 64 chunk

__host__ __device__ __forceinline__ int packed(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// h_j of one raw point x (d entries): 1, then x_c, then x_c^2
template <typename T>
__device__ __forceinline__ double basis_elem(int j, int d, const T* __restrict__ x) {
  if (j == 0) return 1.0;
  if (j <= d) return (double)x[j - 1];
  const double v = (double)x[j - 1 - d];
  return v * v;
}

template <typename T>
__global__ __launch_bounds__(256) void basis_rows_kernel(const T* __restrict__ X, int64_t n, int64_t npad, int d, int k,
                                                        T* __restrict__ YT, int64_t ld) {
  const int j = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npad; i += (int64_t)gridDim.x * 256)
    YT[(int64_t)(k + j) * ld + i] = i < n ? (T)basis_elem<T>(j, d, X + i * d) : (T)0;
}

// part[s][r * 64 + c] = sum over the columns of slice s of zT[r][.] zT[c][.]: thread (ty, tx) of 16 x 16 owns a 4 x 4 patch
template <typename T>
__global__ __launch_bounds__(256) void bordered_gram_kernel(const T* __restrict__ zT, int64_t ld, int64_t npad,
                                                           double* __restrict__ part) {
  __shared__ double slab[BR * GSLD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * GRAM_COLS, c1 = c0 + GRAM_COLS < npad ? c0 + GRAM_COLS : npad;
  double acc[4][4] = {};
  for (int64_t cc = c0; cc < c1; cc += 64) {  // (npad is a multiple of 128: whole chunks)
    for (int e = tid; e < BR * 64; e += 256) {
      const int r = e >> 6, c = e & 63;
      slab[r * GSLD + c] = (double)zT[(int64_t)r * ld + cc + c];
    }
    __syncthreads();
    for (int kk = 0; kk < 64; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = slab[(ty * 4 + i) * GSLD + kk], b[i] = slab[(tx * 4 + i) * GSLD + kk];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
    __syncthreads();
  }
  double* out = part + (int64_t)blockIdx.x * (BR * BR);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(ty * 4 + i) * BR + tx * 4 + j] = acc[i][j];
}

__global__ __launch_bounds__(256) void beta_solve_kernel(const double* __restrict__ part, int S, int k, int p, int64_t n,
                                                        double* __restrict__ state, int* __restrict__ info) {
  __shared__ double A[BR * GSLD];          // A, then L_A (lower)
  __shared__ double Li[BR * (BR + 1) / 2];  // L_A^-1, packed lower
  __shared__ double Bm[1024];              // Z_H^T z (p x k, p k <= 1024 because k + p <= 64), then beta
  __shared__ double piv;
  const int tid = threadIdx.x;
  double* beta = state;
  double* La = state + BR * BR;
  double* Ainv = state + 2 * BR * BR;
  for (int e = tid; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    double s = 0.0;
    for (int q = 0; q < S; ++q) s += part[(int64_t)q * (BR * BR) + (k + i) * BR + k + j];
    A[i * GSLD + j] = s;
  }
  for (int e = tid; e < p * k; e += 256) {
    const int j = e / k, c = e - j * k;
    double s = 0.0;
    for (int q = 0; q < S; ++q) s += part[(int64_t)q * (BR * BR) + (k + j) * BR + c];
    Bm[j * k + c] = s;
  }
  __syncthreads();
  for (int j = 0; j < p; ++j) {  // right-looking Cholesky of A
    if (tid == 0) piv = A[j * GSLD + j];
    __syncthreads();
    const double dj = piv;
    if (!(dj > 0.0) || !(dj <= 1.79769313486231570815e308)) {  // (the same for every thread)
      if (tid == 0) atomicMin(info, (int)(n + j + 1));
      return;
    }
    const double lj = sqrt(dj);
    for (int i = j + tid; i < p; i += 256) A[i * GSLD + j] = i == j ? lj : A[i * GSLD + j] / lj;
    __syncthreads();
    const int m = p - j - 1;  // trailing block, lower triangle
    for (int e = tid; e < m * m; e += 256) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) A[i * GSLD + c] -= A[i * GSLD + j] * A[c * GSLD + j];
    }
    __syncthreads();
  }
  if (tid < k) {  // beta_c = L_A^-T L_A^-1 (Z_H^T z)_c, in place
    const int c = tid;
    for (int i = 0; i < p; ++i) {
      double s = Bm[i * k + c];
      for (int q = 0; q < i; ++q) s -= A[i * GSLD + q] * Bm[q * k + c];
      Bm[i * k + c] = s / A[i * GSLD + i];
    }
    for (int i = p - 1; i >= 0; --i) {
      double s = Bm[i * k + c];
      for (int q = i + 1; q < p; ++q) s -= A[q * GSLD + i] * Bm[q * k + c];
      Bm[i * k + c] = s / A[i * GSLD + i];
    }
  } else if (tid >= 64 && tid - 64 < p) {  // column j of L_A^-1 (another wave than the beta columns)
    const int j = tid - 64;
    for (int i = j; i < p; ++i) {
      double s = i == j ? 1.0 : 0.0;
      for (int q = j; q < i; ++q) s -= A[i * GSLD + q] * Li[packed(q, j)];
      Li[packed(i, j)] = s / A[i * GSLD + i];
    }
  }
  __syncthreads();
  for (int e = tid; e < p * k; e += 256) beta[(e / k) * BR + e % k] = Bm[e];
  for (int e = tid; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    La[i * BR + j] = j <= i ? A[i * GSLD + j] : 0.0;
    double s = 0.0;  // A^-1 = L_A^-T L_A^-1
    for (int q = i > j ? i : j; q < p; ++q) s += Li[packed(q, i)] * Li[packed(q, j)];
    Ainv[i * BR + j] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void basis_project_kernel(T* __restrict__ zT, int64_t ld, int64_t npad, int k, int p,
                                                           const double* __restrict__ state) {
  __shared__ double Bm[1024];
  for (int e = threadIdx.x; e < p * k; e += 256) Bm[e] = state[(e / k) * BR + e % k];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  for (int c = 0; c < k; ++c) {
    double s = (double)zT[(int64_t)c * ld + i];
    for (int j = 0; j < p; ++j) s -= Bm[j * k + c] * (double)zT[(int64_t)(k + j) * ld + i];
    zT[(int64_t)c * ld + i] = (T)s;
  }
}

// One query point per thread.  r = h(x*) - Z_H^T v* (rows [k, k + p) of MT), u = L_A^-1 r by forward substitution with the
// point's vector in LDS (column tid of a 64 x 64 slab: conflict-free) and L_A read as a broadcast.
template <typename T>
__global__ __launch_bounds__(64) void basis_epilogue_kernel(const double* __restrict__ state, int p, int k, int d,
                                                           const T* __restrict__ MT, int64_t ldm, const T* __restrict__ Q,
                                                           int64_t rows, T* __restrict__ mean, T* __restrict__ var,
                                                           double* __restrict__ U) {
  __shared__ double La[BR * (BR + 1) / 2];
  __shared__ double Bm[1024];
  __shared__ double r[BR * 64];
  const int tid = threadIdx.x;
  const bool want_u = var != nullptr || U != nullptr;
  for (int e = tid; e < p * k; e += 64) Bm[e] = state[(e / k) * BR + e % k];
  if (want_u)
    for (int e = tid; e < p * p; e += 64) {
      const int i = e / p, j = e - i * p;
      if (j <= i) La[packed(i, j)] = state[BR * BR + i * BR + j];
    }
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * 64 + tid;
  if (m >= rows) return;  // (no barrier below)
  const T* x = Q + m * d;
  for (int c = 0; c < k; ++c) {
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += basis_elem<T>(j, d, x) * Bm[j * k + c];
    mean[m * k + c] = (T)((double)mean[m * k + c] + s);
  }
  if (!want_u) return;
  double uu = 0.0;
  for (int i = 0; i < p; ++i) {
    double s = basis_elem<T>(i, d, x) - (double)MT[(int64_t)(k + i) * ldm + m];
    for (int q = 0; q < i; ++q) s -= La[packed(i, q)] * r[q * 64 + tid];
    s /= La[packed(i, i)];
    r[i * 64 + tid] = s;
    uu += s * s;
    if (U) U[m * BR + i] = s;
  }
  if (var) var[m] = (T)((double)var[m] + uu);
}

// 16 x 16 elements of the lower triangle per workgroup: Sig[i][j] += u_i . u_j, i, j < M
template <typename T>
__global__ __launch_bounds__(256) void cov_add_uut_kernel(T* __restrict__ Sig, int64_t lds, int64_t M, int p,
                                                         const double* __restrict__ U) {
  if (blockIdx.x > blockIdx.y) return;  // a tile above the diagonal
  __shared__ double Ui[16 * GSLD], Uj[16 * GSLD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)blockIdx.y * 16, j0 = (int64_t)blockIdx.x * 16;
  for (int e = tid; e < 16 * p; e += 256) {
    const int rr = e / p, q = e - rr * p;
    Ui[rr * GSLD + q] = i0 + rr < M ? U[(i0 + rr) * BR + q] : 0.0;
    Uj[rr * GSLD + q] = j0 + rr < M ? U[(j0 + rr) * BR + q] : 0.0;
  }
  __syncthreads();
  const int64_t i = i0 + ty, j = j0 + tx;
  if (i >= M || j > i) return;
  double s = 0.0;
  for (int q = 0; q < p; ++q) s += Ui[ty * GSLD + q] * Uj[tx * GSLD + q];
  Sig[i * lds + j] = (T)((double)Sig[i * lds + j] + s);
}

}  // namespace

int basis_gram_slices(int64_t npad) { return (int)((npad + GRAM_COLS - 1) / GRAM_COLS); }

template <typename T>
void launch_basis_rows(const T* X, int64_t n, int64_t npad, int d, int k, int p, T* YT, int64_t ld, hipStream_t st) {
  const int64_t bx = (npad + 255) / 256;
  hipLaunchKernelGGL(basis_rows_kernel<T>, dim3((unsigned)(bx > 1024 ? 1024 : bx), (unsigned)p), dim3(256), 0, st, X, n, npad,
                     d, k, YT, ld);
}

template <typename T>
void launch_bordered_gram(const T* zT, int64_t ld, int64_t npad, double* part, hipStream_t st) {
  hipLaunchKernelGGL(bordered_gram_kernel<T>, dim3((unsigned)basis_gram_slices(npad)), dim3(256), 0, st, zT, ld, npad, part);
}

void launch_beta_solve(const double* part, int64_t npad, int k, int p, int64_t n, double* state, int* info, hipStream_t st) {
  hipLaunchKernelGGL(beta_solve_kernel, dim3(1), dim3(256), 0, st, part, basis_gram_slices(npad), k, p, n, state, info);
}

template <typename T>
void launch_basis_project(T* zT, int64_t ld, int64_t npad, int k, int p, const double* state, hipStream_t st) {
  hipLaunchKernelGGL(basis_project_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, zT, ld, npad, k, p,
                     state);
}

template <typename T>
void launch_basis_epilogue(const double* state, int p, int k, int d, const T* MT, int64_t ldm, const T* Q, int64_t rows,
                           T* mean, T* var, double* U, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(basis_epilogue_kernel<T>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, state, p, k, d, MT, ldm,
                     Q, rows, mean, var, U);
}

template <typename T>
void launch_cov_add_uut(T* Sig, int64_t lds, int64_t M, int p, const double* U, hipStream_t st) {
  const unsigned t = (unsigned)((M + 15) / 16);
  hipLaunchKernelGGL(cov_add_uut_kernel<T>, dim3(t, t), dim3(256), 0, st, Sig, lds, M, p, U);
}

#define GPX_INSTANTIATE_BASIS(T)                                                                                        \
  template void launch_basis_rows<T>(const T*, int64_t, int64_t, int, int, int, T*, int64_t, hipStream_t);              \
  template void launch_bordered_gram<T>(const T*, int64_t, int64_t, double*, hipStream_t);                              \
  template void launch_basis_project<T>(T*, int64_t, int64_t, int, int, const double*, hipStream_t);                    \
  template void launch_basis_epilogue<T>(const double*, int, int, int, const T*, int64_t, const T*, int64_t, T*, T*,    \
                                         double*, hipStream_t);                                                         \
  template void launch_cov_add_uut<T>(T*, int64_t, int64_t, int, const double*, hipStream_t);
GPX_INSTANTIATE_BASIS(double)
GPX_INSTANTIATE_BASIS(float)

}  // namespace gpx
