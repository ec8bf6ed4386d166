// gpx_posterior.hip — the kernels of the joint posterior (gpx_predict_cov / gpx_sample_posterior, include/gpx.h).
//
// Everything heavy is the existing engine (gpx_api.hip strings it together):
//   V^T = K* L^-T  (cross kernel build + blocked forward solve, as in predict)
//   Sigma = K(Xs, Xs) - V^T V        (symmetric kernel build, then ONE lower-triangle SYRK on the MFMA engine)
//   L_S = chol(Sigma + (diag_add + j) I)  (the blocked Cholesky of the fit on buffers of its own)
//   S^T = Z^T L_S^T                  (the engine's lower-triangular-B product)
// What is new here is the glue:
//   philox_normal_kernel   standard normals of a fixed, documented stream (Philox4x32-10 + Box-Muller), written as Z^T
//   pack_normals_kernel    the caller's normals (S, M, k) transposed into Z^T
//   mirror_lower_kernel    Sigma's lower triangle copied (or zeros written) into its upper triangle, 64 x 64 LDS tiles
//   sample_epilogue_kernel mean + S^T scattered into the (S, M, k) output
// All stores are plain vector stores.
#include "gpx_internal.h"

namespace gpx {
namespace {

// ---- Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) ------------------------------------------------
struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// normal number i of the stream `seed`: block n = i / 2 of Philox (counter (n lo, n hi, 0, 0), key (seed lo, seed hi)),
// Box-Muller on its two 53-bit uniforms, cosine branch for even i, sine branch for odd i (fp64)
__device__ __forceinline__ double philox_normal(uint64_t seed, uint64_t i) {
  const uint64_t n = i >> 1;
  const Philox4 b = philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = (double)((((uint64_t)b.w[0] << 32 | b.w[1]) >> 11) + 1) * 0x1.0p-53;  // (0, 1]
  const double u2 = (double)(((uint64_t)b.w[2] << 32 | b.w[3]) >> 11) * 0x1.0p-53;        // [0, 1)
  const double r = sqrt(-2.0 * log(u1));
  const double a = 6.283185307179586 * u2;
  return (i & 1) ? r * sin(a) : r * cos(a);
}

// Z^T rows [r0, r0 + rows_pad) of a call with `total` = S k normals rows (row r = s k + c) and M columns, into ZT
// (rows_pad x ld): ZT[r - r0][m] = z_(s, m, c), element number i = (s M + m) k + c of the call; zero beyond the valid
// rows / columns (mpad columns).  Every element is a function of its own index only: the result does not depend on the
// grid.  One lane writes 16 bytes of one row (VEC adjacent columns).
template <typename T, bool GEN>
__device__ __forceinline__ void fill_zt(T* __restrict__ ZT, int64_t ld, int64_t r0, int64_t rows_pad, int64_t total,
                                        int64_t M, int64_t mpad, int k, uint64_t seed, const T* __restrict__ z) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  const int64_t groups = mpad / VEC, n = rows_pad * groups;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lr = e / groups, m0 = (e % groups) * VEC, r = r0 + lr;
    const int64_t s = r / k, c = r % k;
    vec_t v;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int64_t m = m0 + j;
      T x = (T)0;
      if (r < total && m < M) {
        const int64_t i = (s * M + m) * k + c;
        x = GEN ? (T)philox_normal(seed, (uint64_t)i) : z[i];
      }
      v[j] = x;
    }
    *reinterpret_cast<vec_t*>(ZT + lr * ld + m0) = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void philox_normal_kernel(T* ZT, int64_t ld, int64_t r0, int64_t rows_pad,
                                                            int64_t total, int64_t M, int64_t mpad, int k, uint64_t seed) {
  fill_zt<T, true>(ZT, ld, r0, rows_pad, total, M, mpad, k, seed, nullptr);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_normals_kernel(T* ZT, int64_t ld, int64_t r0, int64_t rows_pad, int64_t total,
                                                           int64_t M, int64_t mpad, int k, const T* z) {
  fill_zt<T, false>(ZT, ld, r0, rows_pad, total, M, mpad, k, 0, z);
}

// A (n x n, lda; n multiple of 64): upper triangle <- transpose of the lower one (zero_upper: <- 0), tile (ti, tj),
// tj <= ti, per workgroup through LDS (one padded 64 x 64 tile): rows are read and written 64 elements at a time.
template <typename T>
__global__ __launch_bounds__(256) void mirror_lower_kernel(T* A, int64_t lda, int zero_upper) {
  __shared__ T tile[64][65];
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const T* src = A + (int64_t)ti * 64 * lda + (int64_t)tj * 64;  // lower tile (ti, tj)
  T* dst = A + (int64_t)tj * 64 * lda + (int64_t)ti * 64;        // upper tile (tj, ti)
  if (!zero_upper) {
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) tile[r][tx] = src[(int64_t)r * lda + tx];
    __syncthreads();
  }
#pragma unroll 4
  for (int r = ty; r < 64; r += 4) {  // dst[r][tx] = src[tx][r]; on the diagonal tile only above its diagonal
    if (ti == tj && tx <= r) continue;
    dst[(int64_t)r * lda + tx] = zero_upper ? (T)0 : tile[tx][r];
  }
}

// rows [r0, r0 + rows) of S^T (rows a multiple of k, r0 too: whole samples) -> out[(s M + m) k + c] = mean[m k + c] +
// ST[r - r0][m], r = s k + c; the batch's part of `out` is contiguous, written in order
template <typename T>
__global__ __launch_bounds__(256) void sample_epilogue_kernel(const T* __restrict__ ST, int64_t lds, int64_t r0, int64_t rows,
                                                              const T* __restrict__ mean, int64_t M, int k,
                                                              T* __restrict__ out) {
  const int64_t per = M * k, n = (rows / k) * per;
  T* o = out + (r0 / k) * per;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sl = e / per, rem = e % per, m = rem / k, c = rem % k;
    o[e] = mean[rem] + ST[(sl * k + c) * lds + m];
  }
}

unsigned grid_for(int64_t work) {
  const int64_t b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

}  // namespace

template <typename T>
void launch_normals(T* ZT, int64_t ld, int64_t r0, int64_t rows_pad, int64_t total, int64_t M, int64_t mpad, int k,
                    uint64_t seed, const T* z, hipStream_t st) {
  if (rows_pad <= 0) return;
  const unsigned g = grid_for(rows_pad * (mpad / (16 / (int64_t)sizeof(T))));
  if (z)
    hipLaunchKernelGGL(pack_normals_kernel<T>, dim3(g), dim3(256), 0, st, ZT, ld, r0, rows_pad, total, M, mpad, k, z);
  else
    hipLaunchKernelGGL(philox_normal_kernel<T>, dim3(g), dim3(256), 0, st, ZT, ld, r0, rows_pad, total, M, mpad, k, seed);
}

template <typename T>
void launch_mirror_lower(T* A, int64_t lda, int64_t n, int zero_upper, hipStream_t st) {
  if (n <= 0) return;
  const unsigned t = (unsigned)(n / 64);
  hipLaunchKernelGGL(mirror_lower_kernel<T>, dim3(t, t), dim3(256), 0, st, A, lda, zero_upper);
}

template <typename T>
void launch_sample_epilogue(const T* ST, int64_t lds, int64_t r0, int64_t rows, const T* mean, int64_t M, int k, T* out,
                            hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(sample_epilogue_kernel<T>, dim3(grid_for((rows / k) * M * k)), dim3(256), 0, st, ST, lds, r0, rows,
                     mean, M, k, out);
}

#define GPX_INSTANTIATE_POSTERIOR(T)                                                                                  \
  template void launch_normals<T>(T*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int, uint64_t, const T*, \
                                  hipStream_t);                                                                     \
  template void launch_mirror_lower<T>(T*, int64_t, int64_t, int, hipStream_t);                                      \
  template void launch_sample_epilogue<T>(const T*, int64_t, int64_t, int64_t, const T*, int64_t, int, T*, hipStream_t);
GPX_INSTANTIATE_POSTERIOR(double)
GPX_INSTANTIATE_POSTERIOR(float)

}  // namespace gpx
