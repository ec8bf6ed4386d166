// gpx_loo.hip — leave-one-out predictions of the current fit (gpx_loo, include/gpx.h; Rasmussen &
// Williams §5.4.2, eqs. 5.10-5.12).  With K = L L^T the factor of the fit, ZT = L^-T (upper triangular, built by the
// gradient's trtri stage) and Q = K^-1 = ZT ZT^T:
//     q_i = Q_ii = sum_{j >= i} ZT[i][j]^2,   var_i = 1 / q_i,   mean_ic = y_ic - alpha_ic / q_i,
//     logp_ic = -1/2 log(2 pi / q_i) - alpha_ic^2 / (2 q_i).
// A fit with basis functions marginalises beta under a flat prior: its precision is
//     Q' = Q - B A^-1 B^T,  B = K^-1 H = ZT Z_H,  A = Z_H^T Z_H = L_A L_A^T,
// so q'_i = q_i - |L_A^-1 b_i|^2 with b_i = sum_j ZT[i][j] Z_H[j][:] takes the place of q_i (alpha is alpha' already).
//
//   loo_rows_kernel        q_i: one workgroup per row of ZT, 16-byte loads from the 64-aligned column at or below i, the
//                          columns < i of that chunk masked; lanes, then waves through LDS, in a fixed order
//   loo_rows_basis_kernel  q_i and the p dot products b_i in the same pass: RW rows per wave, the Z_H^T column chunk of
//                          all of them staged once in LDS; then u = L_A^-1 b_i by forward substitution, lane j holding
//                          entry j, and q'_i = q_i - |u|^2 (0 for a row the basis alone determines: see below)
//   loo_finish_kernel      mean, var, logp of every row and target from q, alpha^T and y
//
// No atomics anywhere: every sum has one order, a function of (N, ld, p) only, so two calls return the same bits.  No
// kernel reads a column >= N of ZT or Z_H^T: what the padding holds does not matter.
//
// Undetermined rows: q'_i <= 64 * 2^-52 * q_i means that the basis coefficients alone reproduce observation i (every row
// when N = p) — the difference is rounding.  The row pass stores q = 0 for such a row and the finish kernel turns q = 0
// into var = +inf, mean = NaN, logp = -inf.
#include "gpx_internal.h"

namespace gpx {
namespace {

constexpr int LOO_T = 256;        // threads per workgroup (4 waves)
constexpr int LOO_CH = 128;       // columns per staged chunk of the basis pass: one double2 per lane
constexpr double LOO_UNDET = 64.0 * 2.220446049250313e-16;

// sum over the 64 lanes; every lane gets the same bits (the two operands of each step are exchanged, not reordered)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// Rows of ZT start on 128-byte boundaries (ld_skew) and every chunk starts at an even column: the double2 loads are aligned.
__global__ __launch_bounds__(LOO_T) void loo_rows_kernel(const double* __restrict__ ZT, int64_t ld, int64_t n,
                                                        double* __restrict__ q) {
  __shared__ double wsum[LOO_T / 64];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const double* __restrict__ row = ZT + i * ld;
  const int64_t c0 = i & ~(int64_t)63, nev = n & ~(int64_t)1;  // (pairs of columns wholly below n)
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
  for (int64_t c = c0 + 2 * tid; c < nev; c += 2 * LOO_T) {
    const double2 v = *reinterpret_cast<const double2*>(row + c);
    const double x = c >= i ? v.x : 0.0, y = c + 1 >= i ? v.y : 0.0;
    s0 += x * x;
    s1 += y * y;
  }
  if (tid == 0 && (n & 1)) {  // the last column of an odd n (n - 1 >= i)
    const double x = row[n - 1];
    s0 += x * x;
  }
  const double s = wave_sum(s0 + s1);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) q[i] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// PB: bound of p (the accumulators live in registers); RW rows per wave, 4 RW rows per workgroup (a divisor of 64: the rows
// of a workgroup share their first chunk).  Dynamic LDS: p * LOO_CH doubles — the staged chunk of Z_H^T, afterwards L_A by
// columns (p * 64 doubles).
template <int PB, int RW>
__global__ __launch_bounds__(LOO_T) void loo_rows_basis_kernel(const double* __restrict__ ZT, int64_t ld, int64_t n,
                                                              const double* __restrict__ ZHT, int p,
                                                              const double* __restrict__ state, double* __restrict__ q) {
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * (4 * RW), iw = i0 + w * RW;  // first row of the workgroup, of this wave
  const int64_t c0 = i0 & ~(int64_t)63;
  double acc[RW][PB], s0[RW], s1[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    s0[r] = s1[r] = 0.0;
#pragma unroll
    for (int j = 0; j < PB; ++j) acc[r][j] = 0.0;
  }
  for (int64_t c = c0; c < n; c += LOO_CH) {
    for (int e = tid; e < p * LOO_CH; e += LOO_T) {
      const int j = e / LOO_CH, cc = e % LOO_CH;
      sm[e] = c + cc < n ? ZHT[(int64_t)j * ld + c + cc] : 0.0;
    }
    __syncthreads();
    const int64_t col = c + 2 * lane;
    double x[RW], y[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int64_t i = iw + r;
      x[r] = y[r] = 0.0;
      if (i < n) {
        const double* __restrict__ row = ZT + i * ld;
        if (col + 1 < n) {
          const double2 v = *reinterpret_cast<const double2*>(row + col);
          x[r] = v.x, y[r] = v.y;
        } else if (col < n) {
          x[r] = row[col];
        }
        if (col < i) x[r] = 0.0;
        if (col + 1 < i) y[r] = 0.0;
      }
      s0[r] += x[r] * x[r];
      s1[r] += y[r] * y[r];
    }
#pragma unroll
    for (int j = 0; j < PB; ++j)
      if (j < p) {
        const double2 hv = *reinterpret_cast<const double2*>(&sm[j * LOO_CH + 2 * lane]);
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r][j] += x[r] * hv.x + y[r] * hv.y;
      }
    __syncthreads();
  }
  // (the loop ran at least once and ended on a barrier: nobody reads the staged chunk any more)
  for (int e = tid; e < p * 64; e += LOO_T) {  // sm[c * 64 + r] = L_A[r][c] for c <= r < p, 0 elsewhere
    const int c = e >> 6, r = e & 63;
    sm[e] = (r < p && r >= c) ? state[64 * 64 + r * 64 + c] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const double qi = wave_sum(s0[r] + s1[r]);
    double b = 0.0;  // lane j: entry j of b_i, then of the running right-hand side
#pragma unroll
    for (int j = 0; j < PB; ++j)
      if (j < p) {
        const double t = wave_sum(acc[r][j]);
        if (lane == j) b = t;
      }
    double uu = 0.0;
    for (int c = 0; c < p; ++c) {
      const double u = __shfl(b, c) / sm[c * 64 + c];
      uu += u * u;
      if (lane > c) b -= sm[c * 64 + lane] * u;
    }
    const int64_t i = iw + r;
    if (lane == 0 && i < n) {
      const double qp = qi - uu;
      q[i] = qp > LOO_UNDET * qi ? qp : 0.0;
    }
  }
}

__global__ __launch_bounds__(LOO_T) void loo_finish_kernel(const double* __restrict__ q, const double* __restrict__ alphaT,
                                                          int64_t ld, const double* __restrict__ Y, int64_t n, int k,
                                                          double* __restrict__ mean, double* __restrict__ var,
                                                          double* __restrict__ logp) {
  const int64_t i = (int64_t)blockIdx.x * LOO_T + threadIdx.x;
  if (i >= n) return;
  const double qi = q[i];
  if (!(qi > 0.0)) {  // undetermined (the row pass stored 0)
    var[i] = __longlong_as_double(0x7ff0000000000000LL);
    for (int c = 0; c < k; ++c) {
      mean[i * k + c] = __longlong_as_double(0x7ff8000000000000LL);
      logp[i * k + c] = __longlong_as_double(0xfff0000000000000LL);
    }
    return;
  }
  const double v = 1.0 / qi;
  const double lc = -0.5 * log(6.283185307179586476925286766559 * v);
  var[i] = v;
  for (int c = 0; c < k; ++c) {
    const double a = alphaT[(int64_t)c * ld + i];
    mean[i * k + c] = Y[i * k + c] - a * v;
    logp[i * k + c] = lc - 0.5 * a * a * v;
  }
}

}  // namespace

void launch_loo_rows(const double* ZT, int64_t ld, int64_t n, const double* ZHT, int p, const double* state, double* q,
                     hipStream_t st) {
  if (n <= 0) return;
  if (p <= 0) {
    hipLaunchKernelGGL(loo_rows_kernel, dim3((unsigned)n), dim3(LOO_T), 0, st, ZT, ld, n, q);
    return;
  }
  const size_t lds = (size_t)p * LOO_CH * sizeof(double);
  if (p <= 8)
    hipLaunchKernelGGL((loo_rows_basis_kernel<8, 4>), dim3((unsigned)((n + 15) / 16)), dim3(LOO_T), lds, st, ZT, ld, n, ZHT, p,
                       state, q);
  else
    hipLaunchKernelGGL((loo_rows_basis_kernel<64, 1>), dim3((unsigned)((n + 3) / 4)), dim3(LOO_T), lds, st, ZT, ld, n, ZHT, p,
                       state, q);
}

void launch_loo_finish(const double* q, const double* alphaT, int64_t ld, const double* Y, int64_t n, int k, double* mean,
                       double* var, double* logp, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(loo_finish_kernel, dim3((unsigned)((n + LOO_T - 1) / LOO_T)), dim3(LOO_T), 0, st, q, alphaT, ld, Y, n, k,
                     mean, var, logp);
}

}  // namespace gpx
