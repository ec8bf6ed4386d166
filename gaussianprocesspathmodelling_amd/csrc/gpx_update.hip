// gpx_update.hip — removing observations from a factor (gpx_remove_rows).
//
// Taking rows [a, b) out of the data (m = b - a <= UPD_W per pass) leaves L11 and L31 of
//        | L11          |
//    L = | L21 L22      |      rows / cols  [0, a) [a, b) [b, N)
//        | L31 L32 L33  |
// as they are; the new trailing block satisfies L33' L33'^T = L33 L33^T + L32 L32^T: a rank-m POSITIVE update.  With
// the carry W = L32 (n3 x m) it runs over L33 in column panels of width UPD_W.  Per panel with diagonal block Ljj and
// carry rows Wj, one workgroup (upd_small_kernel, fp64 whatever the handle's type) forms
//    Ljj' = chol(Ljj Ljj^T + Wj Wj^T)     V = Ljj^-1 Wj     C = chol(I + V^T V)
//    Q    = | Ljj^T Ljj'^-T    -V C^-T |        (orthogonal, 2 UPD_W square; rounded once to T)
//           | Wj^T  Ljj'^-T     C^-T   |
// and upd_strip_kernel applies it on the MFMA units to every row at and below the panel and to the bordered right-hand
// side rows:  [ Lij' | Wi' ] = [ Lij | Wi ] Q,  [ z3^T[:, panel] | z2^T ] <- the same product.
//
// Lane-owns-row idiom of the small step: a lane keeps one row of 64 doubles in registers (every loop unrolled, all
// indices compile-time) and reads the triangular factor from LDS as wave-wide broadcasts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "gpx_tile.h"

namespace gpx {
namespace {

constexpr int UW = UPD_W;   // 64
constexpr int SLD = UW + 1;  // LDS row stride of the small step's fp64 matrices
constexpr int UQ = 2 * UW;   // edge of Q
typedef Num<double>::v4 v4d;

// y L^T = x in place, L (UW x UW, lower) in LDS with row stride SLD: y_c = (x_c - sum_{k<c} y_k L[c][k]) / L[c][c],
// right-looking so that the UW - 1 - c updates of a step are independent; rinv[c] = 1 / L[c][c] (LDS) keeps the division
// out of the chain of UW dependent steps.  With x = e_c: y = column c of L^-1.
__device__ __forceinline__ void row_solve(double (&x)[UW], const double* __restrict__ Lm, const double* __restrict__ rinv) {
#pragma unroll
  for (int c = 0; c < UW; ++c) {
    x[c] = x[c] * rinv[c];
#pragma unroll
    for (int c2 = c + 1; c2 < UW; ++c2) x[c2] -= x[c] * Lm[c2 * SLD + c];
  }
}

// Cholesky of a UW x UW matrix whose row `lane` (lower part) the lanes of ONE wave hold in a[]; col: [2][UW] doubles of
// LDS for this matrix.  Every wave of the workgroup calls it (one barrier per step); waves with !active only keep the
// barriers company.  On return a[] = row `lane` of the factor (zero above the diagonal).  *bad: 1-based index of the
// first pivot that is not > 0 (unchanged if none); the factorisation goes on with 1 in its place.  rinv[k] = 1 / L[k][k].
__device__ __forceinline__ void chol_rows(double (&a)[UW], int lane, double* __restrict__ col, double* __restrict__ rinv,
                                          bool active, int* bad) {
#pragma unroll
  for (int k = 0; k < UW; ++k) {
    double* cb = col + (k & 1) * UW;
    if (active) cb[lane] = a[k];
    __syncthreads();
    if (active) {
      double d = cb[k];
      if (!(d > 0.0)) {
        if (*bad == 0) *bad = k + 1;
        d = 1.0;
      }
      const double rs = 1.0 / sqrt(d);
      const double lk = lane >= k ? a[k] * rs : 0.0;  // L[lane][k]; the update below: a_ck L[lane][k] / L[k][k]
      const double t = lk * rs;
      a[k] = lk;
      if (lane == k) rinv[k] = rs;
#pragma unroll
      for (int c = k + 1; c < UW; ++c) a[c] -= t * cb[c];
    }
  }
}

// The per-panel small step.  L: the factor, the panel's diagonal block at (p0, p0), nv <= UW valid rows (beyond: the
// identity); Wj: the panel's carry rows (UW wide, compact); Q (UQ x UQ, row-major) out.  gidx0: 0-based index of the
// panel's first row in the remaining data (info).
template <typename T>
__global__ __launch_bounds__(256) void upd_small_kernel(const T* __restrict__ L, int64_t ld, int64_t p0, int nv,
                                                        const T* __restrict__ Wj, T* __restrict__ Q, int64_t gidx0,
                                                        int* __restrict__ info) {
  __shared__ double LaH[UW * SLD];  // Ljj, later H = I + V^T V -> C
  __shared__ double Wb[UW * SLD];   // Wj
  __shared__ double Vt[UW * SLD];   // V^T
  __shared__ double G[UW * SLD];    // Ljj Ljj^T + Wj Wj^T -> Ljj'
  __shared__ double col[2 * 2 * UW];
  __shared__ double rinv[3 * UW];  // 1 / diagonal of Ljj, Ljj', C
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const T* Ljj = L + p0 * ld + p0;
#pragma unroll
  for (int u = 0; u < UW * UW / 256; ++u) {
    const int e = tid + 256 * u, r = e >> 6, c = e & 63;
    double lv = r == c ? 1.0 : 0.0, wv = 0.0;
    if (r < nv) {
      lv = c <= r ? (double)Ljj[(int64_t)r * ld + c] : 0.0;
      wv = (double)Wj[r * UW + c];
    }
    LaH[r * SLD + c] = lv;
    Wb[r * SLD + c] = wv;
    if (r == c) rinv[r] = 1.0 / lv;
  }
  __syncthreads();
  double x[UW];
  if (wave == 0) {  // V^T = Wj^T Ljj^-T, one row per lane
#pragma unroll
    for (int c = 0; c < UW; ++c) x[c] = Wb[c * SLD + lane];
    row_solve(x, LaH, rinv);
#pragma unroll
    for (int c = 0; c < UW; ++c) Vt[lane * SLD + c] = x[c];
  } else {  // beside it: the ten lower 16-tiles of G on the MFMA units, dealt over waves 1-3 (Ljj's image is zero above
            // the diagonal, so the full-length product is the triangular one)
    for (int t = wave - 1; t < 10; t += 3) {
      const int i = t < 1 ? 0 : t < 3 ? 1 : t < 6 ? 2 : 3, j = t - i * (i + 1) / 2;
      const double* Ai = LaH + (16 * i + l15) * SLD + l4;
      const double* Aj = LaH + (16 * j + l15) * SLD + l4;
      const double* Bi = Wb + (16 * i + l15) * SLD + l4;
      const double* Bj = Wb + (16 * j + l15) * SLD + l4;
      v4d accL = {0.0, 0.0, 0.0, 0.0}, accW = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < UW / 4; ++ks) {
        accL = Num<double>::mfma(Ai[4 * ks], Aj[4 * ks], accL);
        accW = Num<double>::mfma(Bi[4 * ks], Bj[4 * ks], accW);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) G[(16 * i + l4 + 4 * r) * SLD + 16 * j + l15] = accL[r] + accW[r];
    }
  }
  __syncthreads();
  {  // H = I + V^T V over Ljj's image (Ljj: global from here on): wave w the 16-tiles (w, 0..w)
    const int i = wave;
    const double* Ai = Vt + (16 * i + l15) * SLD + l4;
    for (int j = 0; j <= i; ++j) {
      const double* Aj = Vt + (16 * j + l15) * SLD + l4;
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = (i == j && l4 + 4 * r == l15) ? 1.0 : 0.0;
#pragma unroll
      for (int ks = 0; ks < UW / 4; ++ks) acc = Num<double>::mfma(Ai[4 * ks], Aj[4 * ks], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) LaH[(16 * i + l4 + 4 * r) * SLD + 16 * j + l15] = acc[r];
    }
  }
  __syncthreads();
  double* M = wave == 0 ? G : LaH;
  const bool active = wave < 2;
#pragma unroll
  for (int c = 0; c < UW; ++c) x[c] = (active && c <= lane) ? M[lane * SLD + c] : 0.0;
  int bad = 0;
  chol_rows(x, lane, col + (wave & 1) * 2 * UW, rinv + (1 + (wave & 1)) * UW, active, &bad);
  if (active) {
#pragma unroll
    for (int c = 0; c < UW; ++c) M[lane * SLD + c] = x[c];
    if (bad && lane == 0) atomicMin(info, (int)(gidx0 + (wave == 0 ? bad : 1)));
  }
  __syncthreads();
  // the four blocks of Q, one per wave, one row per lane
  const double* Lm = wave < 2 ? G : LaH;
  if (wave == 0) {  // row `lane` of Ljj^T
#pragma unroll
    for (int c = 0; c < UW; ++c)
      x[c] = c < nv ? (c >= lane ? (double)Ljj[(int64_t)c * ld + lane] : 0.0) : (c == lane ? 1.0 : 0.0);
  } else if (wave == 1) {  // of Wj^T
#pragma unroll
    for (int c = 0; c < UW; ++c) x[c] = Wb[c * SLD + lane];
  } else if (wave == 2) {  // of -V
#pragma unroll
    for (int c = 0; c < UW; ++c) x[c] = -Vt[c * SLD + lane];
  } else {  // of I
#pragma unroll
    for (int c = 0; c < UW; ++c) x[c] = c == lane ? 1.0 : 0.0;
  }
  row_solve(x, Lm, rinv + (wave < 2 ? 1 : 2) * UW);
  T* q = Q + ((wave & 1) * UW + lane) * UQ + (wave >> 1) * UW;
#pragma unroll
  for (int c = 0; c < UW; ++c) q[c] = (T)x[c];
}

// [ out | carry' ] = [ panel | carry ] Q for a band of 64 rows per workgroup.  Rows i < nrows are rows p0 + i of the
// factor (columns [p0, p0 + UW), lower triangle only), rows nrows + r (r < 64) the bordered rows zT (columns < nv of the
// panel).  Each workgroup reads its band once, K = 2 UW in two halves through one LDS image, and every wave owns 32 of
// the 128 output columns: waves 0-1 the new panel, 2-3 the new carry (written over the band's own carry rows, which
// it has read itself).  outL / outZ: where the new panel goes — the staging buffer, or (m == UW only) its compacted
// place in the factor; see remove_pass in gpx_api.hip for why that is safe.
template <typename T>
__global__ __launch_bounds__(256) void upd_strip_kernel(const T* __restrict__ L, int64_t ld, int64_t p0, int64_t nrows,
                                                        int nv, const T* __restrict__ zT, T* __restrict__ Wp,
                                                        T* __restrict__ Wz, const T* __restrict__ Q,
                                                        T* __restrict__ outL, int64_t ldo, T* __restrict__ outZ,
                                                        int64_t ldz) {
  using v4 = typename Num<T>::v4;
  constexpr int AL = UW + 1;
  __shared__ T As[64 * AL];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * 64, total = nrows + 64;
  v4 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (v4){0, 0, 0, 0};
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    T bq[UW / 4][2];
#pragma unroll
    for (int ks = 0; ks < UW / 4; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bq[ks][nt] = Q[(half * UW + 4 * ks + l4) * UQ + 32 * wave + 16 * nt + l15];
    T v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u, r = e >> 6, c = e & 63;
      const int64_t i = i0 + r;
      v[u] = (T)0;
      if (half == 0) {
        if (i < nrows) {
          if (i >= UW || c <= i) v[u] = L[(p0 + i) * ld + p0 + c];
        } else if (i < total) {
          if (c < nv) v[u] = zT[(i - nrows) * ld + p0 + c];
        }
      } else {
        if (i < nrows)
          v[u] = Wp[i * UW + c];
        else if (i < total)
          v[u] = Wz[(i - nrows) * UW + c];
      }
    }
    if (half) __syncthreads();  // the first half's fragments have been read
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u;
      As[(e >> 6) * AL + (e & 63)] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < UW / 4; ++ks) {
      T a[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) a[mt] = As[(16 * mt + l15) * AL + 4 * ks + l4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = Num<T>::mfma(a[mt], bq[ks][nt], acc[mt][nt]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + 16 * mt + Num<T>::drow(l4, r);
        const int cc = (wave & 1) * 32 + 16 * nt + l15;  // column inside the panel / the carry
        const T val = acc[mt][nt][r];
        if (wave < 2) {
          if (i < nrows) {
            if (i >= UW || cc <= i) outL[i * ldo + cc] = val;
          } else if (i < total) {
            if (cc < nv) outZ[(i - nrows) * ldz + cc] = val;
          }
        } else {
          if (i < nrows)
            Wp[i * UW + cc] = val;
          else if (i < total)
            Wz[(i - nrows) * UW + cc] = val;
        }
      }
}

// the staged panel (the strip's outL / outZ images, UW wide, back to back) into its place, under the strip's masks
template <typename T>
__global__ __launch_bounds__(256) void upd_unstage_kernel(const T* __restrict__ P, int64_t nrows, int nv, T* __restrict__ dstL,
                                                          int64_t ldl, T* __restrict__ dstZ, int64_t ldz) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, i = e >> 6;
  const int c = (int)(e & 63);
  if (i < nrows) {
    if (i >= UW || c <= i) dstL[i * ldl + c] = P[e];
  } else if (i < nrows + 64) {
    if (c < nv) dstZ[(i - nrows) * ldz + c] = P[e];
  }
}

// W ((n3 + 64) x UW): row i < n3 = columns [a, a + m) of row a + m + i of the factor, row n3 + r the same columns of
// zT's row r; zero from column m on
template <typename T>
__global__ __launch_bounds__(256) void upd_carry_init_kernel(const T* __restrict__ L, int64_t ld, int64_t a, int m, int64_t n3,
                                                             const T* __restrict__ zT, T* __restrict__ W) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, i = e >> 6;
  const int c = (int)(e & 63);
  if (i >= n3 + 64) return;
  T v = (T)0;
  if (c < m) v = i < n3 ? L[(a + m + i) * ld + a + c] : zT[(i - n3) * ld + a + c];
  W[e] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void upd_copy_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds,
                                                       int64_t rows, int64_t cols) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) dst[r * ldd + c] = src[r * lds + c];
}

// rows [n, npad) of the factor: zero up to column npad, one on the diagonal; columns [n, nz) of the 64 rows of zT: zero
template <typename T>
__global__ __launch_bounds__(256) void upd_pad_kernel(T* __restrict__ A, int64_t ld, int64_t n, int64_t npad, T* __restrict__ zT,
                                                      int64_t nz) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (r < npad - n) {
    const int64_t row = n + r;
    if (c < npad) A[row * ld + c] = c == row ? (T)1 : (T)0;
  } else {
    const int64_t zr = r - (npad - n);
    if (c >= n && c < nz) zT[zr * ld + c] = (T)0;
  }
}

// Winv[q] = inverse of the 64 x 64 diagonal block q of L (lower), row-major, zero above the diagonal; fp64 inside
template <typename T>
__global__ __launch_bounds__(64) void upd_trinv_kernel(const T* __restrict__ L, int64_t ld, int64_t q0, T* __restrict__ Winv) {
  __shared__ double Lm[UW * SLD];
  __shared__ double rinv[UW];
  const int lane = threadIdx.x;
  const int64_t q = q0 + blockIdx.x;
  const T* B = L + q * UW * ld + q * UW;
  for (int r = 0; r < UW; ++r) Lm[r * SLD + lane] = lane <= r ? (double)B[(int64_t)r * ld + lane] : 0.0;
  rinv[lane] = 1.0 / (double)B[(int64_t)lane * ld + lane];
  __syncthreads();
  double x[UW];
#pragma unroll
  for (int c = 0; c < UW; ++c) x[c] = c == lane ? 1.0 : 0.0;
  row_solve(x, Lm, rinv);
  T* out = Winv + q * (UW * UW);
#pragma unroll
  for (int c = 0; c < UW; ++c) out[c * UW + lane] = (T)x[c];
}

}  // namespace

template <typename T>
void launch_upd_carry_init(const T* L, int64_t ld, int64_t a, int m, int64_t n3, const T* zT, T* W, hipStream_t st) {
  const int64_t total = (n3 + 64) * UW;
  hipLaunchKernelGGL(upd_carry_init_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, L, ld, a, m, n3, zT, W);
}

template <typename T>
void launch_upd_small(const T* L, int64_t ld, int64_t p0, int nv, const T* Wj, T* Q, int64_t gidx0, int* info,
                      hipStream_t st) {
  hipLaunchKernelGGL(upd_small_kernel<T>, dim3(1), dim3(256), 0, st, L, ld, p0, nv, Wj, Q, gidx0, info);
}

template <typename T>
void launch_upd_strip(const T* L, int64_t ld, int64_t p0, int64_t nrows, int nv, const T* zT, T* Wp, T* Wz, const T* Q,
                      T* outL, int64_t ldo, T* outZ, int64_t ldz, hipStream_t st) {
  hipLaunchKernelGGL(upd_strip_kernel<T>, dim3((unsigned)((nrows + 64 + 63) / 64)), dim3(256), 0, st, L, ld, p0, nrows, nv,
                     zT, Wp, Wz, Q, outL, ldo, outZ, ldz);
}

template <typename T>
void launch_upd_unstage(const T* P, int64_t nrows, int nv, T* dstL, int64_t ldl, T* dstZ, int64_t ldz, hipStream_t st) {
  const int64_t total = (nrows + 64) * UW;
  hipLaunchKernelGGL(upd_unstage_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, nrows, nv, dstL, ldl,
                     dstZ, ldz);
}

template <typename T>
void launch_upd_copy(T* dst, int64_t ldd, const T* src, int64_t lds, int64_t rows, int64_t cols, hipStream_t st) {
  if (rows <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(upd_copy_kernel<T>, dim3((unsigned)((cols + 255) / 256), (unsigned)std::min<int64_t>(rows, 4096)),
                     dim3(256), 0, st, dst, ldd, src, lds, rows, cols);
}

template <typename T>
void launch_upd_pad(T* A, int64_t ld, int64_t n, int64_t npad, T* zT, int64_t nz, hipStream_t st) {
  const int64_t width = std::max(npad, nz);
  hipLaunchKernelGGL(upd_pad_kernel<T>, dim3((unsigned)((width + 255) / 256), (unsigned)(npad - n + 64)), dim3(256), 0, st, A,
                     ld, n, npad, zT, nz);
}

template <typename T>
void launch_upd_trinv(const T* L, int64_t ld, int64_t q0, int64_t q1, T* Winv, hipStream_t st) {
  if (q1 <= q0) return;
  hipLaunchKernelGGL(upd_trinv_kernel<T>, dim3((unsigned)(q1 - q0)), dim3(64), 0, st, L, ld, q0, Winv);
}

#define GPX_UPD_INST(T)                                                                                                  \
  template void launch_upd_carry_init<T>(const T*, int64_t, int64_t, int, int64_t, const T*, T*, hipStream_t);           \
  template void launch_upd_small<T>(const T*, int64_t, int64_t, int, const T*, T*, int64_t, int*, hipStream_t);          \
  template void launch_upd_strip<T>(const T*, int64_t, int64_t, int64_t, int, const T*, T*, T*, const T*, T*, int64_t,   \
                                    T*, int64_t, hipStream_t);                                                           \
  template void launch_upd_unstage<T>(const T*, int64_t, int, T*, int64_t, T*, int64_t, hipStream_t);                    \
  template void launch_upd_copy<T>(T*, int64_t, const T*, int64_t, int64_t, int64_t, hipStream_t);                       \
  template void launch_upd_pad<T>(T*, int64_t, int64_t, int64_t, T*, int64_t, hipStream_t);                              \
  template void launch_upd_trinv<T>(const T*, int64_t, int64_t, int64_t, T*, hipStream_t);
GPX_UPD_INST(double)
GPX_UPD_INST(float)
#undef GPX_UPD_INST

}  // namespace gpx
