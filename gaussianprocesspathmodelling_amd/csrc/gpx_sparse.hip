// gpx_sparse.hip — kernels of the inducing-point GP (gpx_sparse_*; fp64).
//
// The one heavy kernel is the TN product  C += X^T X  over the ROWS of a row-major chunk X (rows x n): the whitened
// cross-kernel rows of a chunk of observations, with the scaled targets as bordered columns, contracted over the
// observations.  The tile engine of gpx_tile.h is NT (k contiguous); here k runs down the rows, so a 128-byte line of the
// LDS image is 16 consecutive COLUMNS of one k-row, and lane l of a wave fetches its MFMA operand with one ds_read_b64 at
// [k = (l >> 4) + 4 s][i = l & 15]  (gpx_tile.h: A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15]).
//
// LDS image: TN_K = 16 k-rows of 64 columns per operand, k-rows TN_LDS = 80 doubles apart — 640 bytes = 160 banks of four
// bytes, i.e. a stagger of 32 banks (one 128-byte line) per k-row.  With a stride of 64 doubles (512 bytes = 0 mod 64
// banks) the two k-rows that a 32-lane half of a ds_read_b64 covers would share their banks; with the stagger they take
// banks [0, 32) and [32, 64).  (Derived from the bank rule bank = (addr / 4) mod 64, not measured.)
//
// Determinism: one workgroup owns one (tile, split) pair and walks its rows in ascending order; the splits of a tile are
// summed in split order by a second launch.  The number of splits is a function of (n, rows_nominal) only — for a fit: of
// (m, chunk) — never of the device, the free memory or the number of valid rows.  No atomics.
//
// The gradient of the bound (gpx_sparse_elbo_grad) adds the rectangular derivative contraction, cross_dtheta_kernel:
//   part[tile][t] = sum over a 64 x 64 tile of  W[n][i] r_n (dK / dlog theta_t)(a_n, b_i),   theta = (lengthscales..., sf2)
// with the weights LOADED from a row-major matrix W (one read of rows x cols doubles: the kernel is bound by that read) and
// dK regenerated from the two staged point sets exactly as alpha_quad_kernel (gpx_grad.hip) does — without its symmetry
// factor and its diagonal: the grid is the whole rectangle.  r_n = 1 / sqrt(rsn2 rw_n) is the row scale 1 / s_n of the
// streamed pass (rw null: 1; rsn2 = 1 and no rw: the weights as they are, exactly).  One partial per (tile, theta) through the
// workgroup reduction in fixed order; partials_acc_kernel adds a launch's partials onto a device accumulator, launch after
// launch in chunk order.  Rows >= na and columns >= nb contribute exact zeros whatever W holds there; a coincident pair
// contributes its finite value (cov::value_kd: Matern-1/2 has kd = 0 at r = 0).
#include "gpx_cov.h"
#include "gpx_internal.h"

namespace gpx {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int TN_T = 64;    // output tile edge
constexpr int TN_K = 16;    // k-rows per LDS stage
constexpr int TN_LDS = 80;  // doubles between k-rows of the LDS image (64 + one 128-byte line of stagger)

// lower-triangle tile t -> (ti, tj), tj <= ti, row-major over the triangle
__device__ __forceinline__ void tri_tile(int t, int* ti, int* tj) {
  int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  while (i * (i + 1) / 2 > t) --i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

// one thread's share of a stage: four consecutive columns of row `row` of both operands (zero from row r1 on)
__device__ __forceinline__ void tn_fetch(const double* pa, const double* pb, int64_t ldx, int64_t row, int64_t r1, double2& a0,
                                         double2& a1, double2& b0, double2& b1) {
  if (row < r1) {
    const double2* qa = reinterpret_cast<const double2*>(pa + row * ldx);
    const double2* qb = reinterpret_cast<const double2*>(pb + row * ldx);
    a0 = qa[0], a1 = qa[1], b0 = qb[0], b1 = qb[1];
  } else {
    a0 = a1 = b0 = b1 = double2{0.0, 0.0};
  }
}

// part[(s * ntile + t)][64][64] = X[r0_s : r1_s, ti-block]^T X[r0_s : r1_s, tj-block], r0_s = s * split_rows
__global__ __launch_bounds__(256) void syrk_tn_kernel(const double* __restrict__ X, int64_t ldx, int64_t rows,
                                                      int64_t split_rows, double* __restrict__ part, int ntile) {
  __shared__ double As[TN_K * TN_LDS];
  __shared__ double Bs[TN_K * TN_LDS];
  const int t = blockIdx.x, s = blockIdx.y;
  int ti, tj;
  tri_tile(t, &ti, &tj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t r0 = (int64_t)s * split_rows;
  const int64_t r1 = r0 + split_rows < rows ? r0 + split_rows : rows;
  // loader: thread -> k-row lr of the stage, four consecutive columns from lc
  const int lr = tid >> 4, lc = (tid & 15) * 4;
  const double* pa = X + (int64_t)ti * TN_T + lc;
  const double* pb = X + (int64_t)tj * TN_T + lc;
  v4d acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = v4d{0.0, 0.0, 0.0, 0.0};
  double2 a0, a1, b0, b1;
  if (r0 < r1) tn_fetch(pa, pb, ldx, r0 + lr, r1, a0, a1, b0, b1);
  for (int64_t r = r0; r < r1; r += TN_K) {
    __syncthreads();  // the previous stage has been read
    double* da = As + lr * TN_LDS + lc;
    double* db = Bs + lr * TN_LDS + lc;
    da[0] = a0.x, da[1] = a0.y, da[2] = a1.x, da[3] = a1.y;
    db[0] = b0.x, db[1] = b0.y, db[2] = b1.x, db[3] = b1.y;
    __syncthreads();
    // the next stage's loads fly beside this stage's MFMAs
    if (r + TN_K < r1) tn_fetch(pa, pb, ldx, r + TN_K + lr, r1, a0, a1, b0, b1);
#pragma unroll
    for (int q = 0; q < TN_K / 4; ++q) {
      const int krow = (4 * q + l4) * TN_LDS;
      const double a = As[krow + 16 * wave + l15];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double b = Bs[krow + 16 * j + l15];
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
      }
    }
  }
  // D reg r of lane l = D[(l >> 4) + 4 r][l & 15]
  double* out = part + ((int64_t)s * ntile + t) * (TN_T * TN_T);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(16 * wave + l4 + 4 * r) * TN_T + 16 * j + l15] = acc[j][r];
}

// C[tile] (+)= sum over the splits, in split order; elements above the diagonal are not touched
__global__ __launch_bounds__(256) void syrk_tn_reduce_kernel(const double* __restrict__ part, int ntile, int S,
                                                             double* __restrict__ C, int64_t ldc, int accumulate) {
  const int t = blockIdx.x;
  int ti, tj;
  tri_tile(t, &ti, &tj);
  for (int idx = threadIdx.x; idx < TN_T * TN_T; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    const int64_t gi = (int64_t)ti * TN_T + i, gj = (int64_t)tj * TN_T + j;
    if (gj > gi) continue;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += part[((int64_t)s * ntile + t) * (TN_T * TN_T) + idx];
    double* c = C + gi * ldc + gj;
    *c = accumulate ? *c + sum : sum;
  }
}

// row r of a chunk: the cross-kernel row over s_r = sqrt(sn2 w_r), and y_r / s_r beside it
__global__ __launch_bounds__(256) void sparse_border_kernel(double* __restrict__ Kc, int64_t ld, int64_t rows, int64_t mpad,
                                                            const double* __restrict__ y, int k,
                                                            const double* __restrict__ w, double sn2) {
  const int64_t r = blockIdx.x;
  double* row = Kc + r * ld;
  if (r >= rows) {  // (the cross-kernel part of a padded row is zero already)
    if (threadIdx.x < 64) row[mpad + threadIdx.x] = 0.0;
    return;
  }
  const double s = sqrt(sn2 * (w ? w[r] : 1.0));
  for (int64_t j = threadIdx.x; j < mpad; j += 256) row[j] = row[j] / s;
  if (threadIdx.x < 64) row[mpad + threadIdx.x] = threadIdx.x < k ? y[r * k + threadIdx.x] / s : 0.0;
}

// one workgroup: scal[0] = trace of the leading mpad x mpad block (summed in a fixed tree), scal[1 + c] = B[mpad + c][mpad + c]
// for c < k, then + 1 on that block's diagonal
__global__ __launch_bounds__(256) void sparse_close_kernel(double* __restrict__ B, int64_t ld, int64_t mpad, int k,
                                                           double* __restrict__ scal) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < mpad; j += 256) {
    const double v = B[j * ld + j];
    s += v;
    B[j * ld + j] = v + 1.0;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) scal[0] = red[0];
  if ((int)threadIdx.x < k) scal[1 + threadIdx.x] = B[(mpad + threadIdx.x) * ld + mpad + threadIdx.x];
}

// var[i] = (sf2 - |V1[i]|^2) + |V2[i]|^2 + add, one wave per row
__global__ __launch_bounds__(256) void sparse_var_kernel(const double* __restrict__ V1, const double* __restrict__ V2,
                                                         int64_t ld, int64_t m, int64_t ncols, double sf2, double add,
                                                         double* __restrict__ var) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t j = lane; j < ncols; j += 64) {
    const double a = V1[i * ld + j], b = V2[i * ld + j];
    s1 += a * a;
    s2 += b * b;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_down(s1, o);
    s2 += __shfl_down(s2, o);
  }
  if (lane == 0) var[i] = (sf2 - s1) + s2 + add;
}

// XT (cols x rows, ldt) = X (rows x cols, ldx)^T through a 32 x 33 LDS tile; rows, cols multiples of 32 (the benchmark's
// "transpose, then the NT engine" route: gpx_debug_syrk_tn_bench)
__global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ X, int64_t ldx, double* __restrict__ XT,
                                                        int64_t ldt) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  for (int i = ty; i < 32; i += 8) tile[i][tx] = X[(r0 + i) * ldx + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8) XT[(c0 + i) * ldt + r0 + tx] = tile[tx][i];
}

// sum over the 256 threads of a workgroup in a fixed order, every thread gets the result (gpx_grad.hip's wg_sum)
__device__ __forceinline__ double wg_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red[] may still be read from the previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (column tiles, row tiles); As (>= 64 gridDim.y rows) and Bs (>= 64 gridDim.x rows): scaled points, d columns;
// W readable over the whole padded rectangle, rows 16-byte aligned (ldw even).  part[(by * gridDim.x + bx) * nth + t],
// nth = (ard ? d : 1) + 1.  D > 0: the dimension at compile time (the LDS image is 64 D doubles per side instead of 64 MAX_D).
template <int KERNEL, int D>
__global__ __launch_bounds__(256) void cross_dtheta_kernel(const double* __restrict__ W, int64_t ldw, int64_t na, int64_t nb,
                                                          const double* __restrict__ As, const double* __restrict__ Bs,
                                                          int d_rt, int ard, double sf2, const double* __restrict__ rw,
                                                          double rsn2, double* __restrict__ part) {
  constexpr int KT = 64, DL = D > 0 ? D : MAX_D;
  __shared__ double xa[KT * DL];
  __shared__ double xb[KT * DL];
  __shared__ double rs[KT];
  __shared__ double red[4];
  const int d = (D > 0) ? D : d_rt;
  const int64_t i0 = (int64_t)blockIdx.y * KT, j0 = (int64_t)blockIdx.x * KT;
  const int tid = threadIdx.x;
  for (int e = tid; e < KT * d; e += 256) {
    xa[e] = As[i0 * d + e];
    xb[e] = Bs[j0 * d + e];
  }
  if (tid < KT) {
    const int64_t gi = i0 + tid;
    rs[tid] = gi < na ? 1.0 / sqrt(rsn2 * (rw ? rw[gi] : 1.0)) : 0.0;
  }
  __syncthreads();
  const int jl0 = (tid & 31) * 2, rg = tid >> 5;  // this thread's 8 rows x 2 columns: a wave reads 2 rows x 512 bytes of W
  const bool c0 = j0 + jl0 < nb, c1 = j0 + jl0 + 1 < nb;
  double wt[8][2];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int il = rg + 8 * r;
    const double2 w2 = *reinterpret_cast<const double2*>(W + (i0 + il) * ldw + j0 + jl0);
    const bool row = i0 + il < na;
    wt[r][0] = (row && c0) ? w2.x * rs[il] : 0.0;
    wt[r][1] = (row && c1) ? w2.y * rs[il] : 0.0;
  }
  double Sf = 0.0, Sl = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int il = rg + 8 * r;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int jl = jl0 + q;
      double r2 = 0.0;
      for (int c = 0; c < d; ++c) {
        const double e = xa[il * d + c] - xb[jl * d + c];
        r2 += e * e;
      }
      double kf, kd;
      cov::value_kd<KERNEL>(r2, sf2, kf, kd);
      const double v = wt[r][q];
      Sf += v * kf;
      const double t = v * kd;
      Sl += t * r2;
      wt[r][q] = t;
    }
  }
  const int nls = ard ? d : 1;
  double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (nls + 1);
  if (!ard) {
    const double s = wg_sum(Sl, red);
    if (tid == 0) out[0] = s;
  } else {
    for (int c = 0; c < d; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const double e = xa[(rg + 8 * r) * d + c] - xb[(jl0 + q) * d + c];
          s += wt[r][q] * e * e;
        }
      }
      s = wg_sum(s, red);
      if (tid == 0) out[c] = s;
    }
  }
  const double sf = wg_sum(Sf, red);
  if (tid == 0) out[nls] = sf;
}

// acc[t] += sum_tile part[tile * nth + t]; one workgroup per theta, fixed order (reduce_partials_kernel's, accumulating)
__global__ __launch_bounds__(256) void partials_acc_kernel(const double* __restrict__ part, int64_t ntile, int nth,
                                                          double* __restrict__ acc) {
  __shared__ double red[4];
  const int t = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < ntile; i += 256) s += part[i * nth + t];
  s = wg_sum(s, red);
  if (threadIdx.x == 0) acc[t] += s;
}

// The two m x m weights of the gradient from B^-1 (in H), the rebuilt B = LB LB^T (in M) and ch^T (64 rows, ld):
//   H = kk (I - B^-1) - ch ch^T        M = H - kk (B - I)  =  kk (2 I - B^-1 - B) - ch ch^T
// element by element over the padded square (padded rows and columns of both come out exactly zero: B = B^-1 = I, ch = 0 there)
__global__ __launch_bounds__(256) void sparse_grad_weights_kernel(double* __restrict__ H, double* __restrict__ M, int64_t ld,
                                                                 int64_t mpad, const double* __restrict__ chT, int k) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= mpad * mpad) return;
  const int64_t i = e / mpad, j = e - i * mpad;
  const double kk = (double)k, dij = i == j ? 1.0 : 0.0;
  double cc = 0.0;
  for (int c = 0; c < k; ++c) cc += chT[c * ld + i] * chT[c * ld + j];
  const double h = kk * (dij - H[i * ld + j]) - cc;
  H[i * ld + j] = h;
  M[i * ld + j] = h - kk * (M[i * ld + j] - dij);
}

// one workgroup, fixed trees: out[0] = trace of Binv over mpad (a padded row adds exactly 1), out[1] = sum over the k rows
// of chT of their squares
__global__ __launch_bounds__(256) void sparse_grad_scalars_kernel(const double* __restrict__ Binv, int64_t ld, int64_t mpad,
                                                                 const double* __restrict__ chT, int k,
                                                                 double* __restrict__ out) {
  __shared__ double red[4];
  double tr = 0.0, ss = 0.0;
  for (int64_t j = threadIdx.x; j < mpad; j += 256) {
    tr += Binv[j * ld + j];
    for (int c = 0; c < k; ++c) ss += chT[c * ld + j] * chT[c * ld + j];
  }
  tr = wg_sum(tr, red);
  ss = wg_sum(ss, red);
  if (threadIdx.x == 0) out[0] = tr, out[1] = ss;
}

}  // namespace

int syrk_tn_splits(int64_t n, int64_t rows_nominal) {
  const int64_t nt = n / TN_T, ntile = nt * (nt + 1) / 2;
  int64_t S = 1024 / ntile;                                  // about four workgroups per CU when the tiles alone are few
  S = S < rows_nominal / 128 ? S : rows_nominal / 128;      // ... but at least 128 rows per split
  return (int)(S < 1 ? 1 : S > 64 ? 64 : S);
}

int64_t syrk_tn_part_elems(int64_t n, int64_t rows_nominal) {
  const int64_t nt = n / TN_T;
  return (int64_t)syrk_tn_splits(n, rows_nominal) * (nt * (nt + 1) / 2) * (TN_T * TN_T);
}

void launch_syrk_tn(double* C, int64_t ldc, int64_t n, const double* X, int64_t ldx, int64_t rows, int64_t rows_nominal,
                    double* part, int accumulate, hipStream_t st) {
  const int64_t nt = n / TN_T;
  const int ntile = (int)(nt * (nt + 1) / 2);
  const int S = syrk_tn_splits(n, rows_nominal);
  const int64_t split_rows = round_up((rows_nominal + S - 1) / S, TN_K);
  hipLaunchKernelGGL(syrk_tn_kernel, dim3((unsigned)ntile, (unsigned)S), dim3(256), 0, st, X, ldx, rows, split_rows, part,
                     ntile);
  hipLaunchKernelGGL(syrk_tn_reduce_kernel, dim3((unsigned)ntile), dim3(256), 0, st, (const double*)part, ntile, S, C, ldc,
                     accumulate);
}

void launch_transpose(const double* X, int64_t ldx, int64_t rows, int64_t cols, double* XT, int64_t ldt, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(cols / 32), (unsigned)(rows / 32)), dim3(256), 0, st, X, ldx, XT, ldt);
}

void launch_sparse_border(double* Kc, int64_t ld, int64_t rows, int64_t rows_pad, int64_t mpad, const double* y, int k,
                          const double* w, double sn2, hipStream_t st) {
  hipLaunchKernelGGL(sparse_border_kernel, dim3((unsigned)rows_pad), dim3(256), 0, st, Kc, ld, rows, mpad, y, k, w, sn2);
}

void launch_sparse_close(double* B, int64_t ld, int64_t mpad, int k, double* scal, hipStream_t st) {
  hipLaunchKernelGGL(sparse_close_kernel, dim3(1), dim3(256), 0, st, B, ld, mpad, k, scal);
}

void launch_sparse_var(const double* V1, const double* V2, int64_t ld, int64_t m, int64_t ncols, double sf2, double add,
                       double* var, hipStream_t st) {
  hipLaunchKernelGGL(sparse_var_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, V1, V2, ld, m, ncols, sf2, add, var);
}

int64_t cross_dtheta_part_elems(int64_t rows_pad, int64_t cols_pad, int n_ls) {
  return (rows_pad / 64) * (cols_pad / 64) * (n_ls + 1);
}

void launch_cross_dtheta(int kernel, const double* W, int64_t ldw, int64_t na, int64_t napad, int64_t nb, int64_t nbpad,
                         const double* As, const double* Bs, int d, int n_ls, double sf2, const double* rw, double rsn2,
                         double* part, double* acc, hipStream_t st) {
  const dim3 grid((unsigned)(nbpad / 64), (unsigned)(napad / 64)), block(256);
  const int ard = n_ls > 1;
  cov::dispatch(kernel, [&](auto fam) {
    if (d == 1)
      hipLaunchKernelGGL((cross_dtheta_kernel<fam, 1>), grid, block, 0, st, W, ldw, na, nb, As, Bs, d, ard, sf2, rw, rsn2, part);
    else if (d == 3)
      hipLaunchKernelGGL((cross_dtheta_kernel<fam, 3>), grid, block, 0, st, W, ldw, na, nb, As, Bs, d, ard, sf2, rw, rsn2, part);
    else
      hipLaunchKernelGGL((cross_dtheta_kernel<fam, 0>), grid, block, 0, st, W, ldw, na, nb, As, Bs, d, ard, sf2, rw, rsn2, part);
  });
  hipLaunchKernelGGL(partials_acc_kernel, dim3((unsigned)(n_ls + 1)), dim3(256), 0, st, (const double*)part,
                     (napad / 64) * (nbpad / 64), n_ls + 1, acc);
}

void launch_sparse_grad_weights(double* H, double* M, int64_t ld, int64_t mpad, const double* chT, int k, hipStream_t st) {
  hipLaunchKernelGGL(sparse_grad_weights_kernel, dim3((unsigned)(mpad * mpad / 256)), dim3(256), 0, st, H, M, ld, mpad, chT, k);
}

void launch_sparse_grad_scalars(const double* Binv, int64_t ld, int64_t mpad, const double* chT, int k, double* out,
                                hipStream_t st) {
  hipLaunchKernelGGL(sparse_grad_scalars_kernel, dim3(1), dim3(256), 0, st, Binv, ld, mpad, chT, k, out);
}

}  // namespace gpx
