// gpx_pathwise.hip — pathwise posterior function samples (gpx_pathwise_draw / _eval, include/gpx.h; DESIGN.md §3.4q;
// Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors").  A sample is a function
//     f_col(x) = f~_col(x) + sum_n k(x, x_n) V[col][n],   f~_col(x) = sum_j W[col][j] phi_j(x),
//     phi_j(x) = amp cos(theta_j(x)) for j < F,  amp sin(theta_(j - F)(x)) for F <= j < 2 F,
//     theta_f(x) = sum_c Omega[f][c] u_c,  u = x / l,  amp = sqrt(sf2 / F).
//
//   pw_eval_kernel     the hot path: one split of  OutT (Cpad x mpad) = W Phi(Xq)^T + V K(Xq, X)^T.  Neither Phi nor K is
//                      stored: lane l of a wave owns the pair (contraction item l >> 4, query l & 15) of a 4 x 16 slice,
//                      forms its feature or kernel value in registers (cov::value) and hands it to the MFMA as the B operand
//                      (B lane l = B[l >> 4][l & 15], one element per lane, as A: gpx_tile.h); the A operand is a 16-column
//                      tile of the V / W slab in LDS.  One value serves the four 16-column tiles of the workgroup's 64
//                      columns; the four waves own 16 query points each.  Values as B put the query index on the
//                      accumulator's lane axis: the partial stores run along m.
//   pw_finish_kernel   OutT = the splits' partials summed in split order
//   pw_draw_kernel     normals -> Omega (F x d, fp64) and W (Cpad x ldw, zero beyond C rows / 2 F columns)
//   pw_resid_kernel    R[col][n] = y[n][c] - F~T[col][n] - sqrt(sn2 w_n) E[col][n] in right-hand-side layout
//   pw_unpack_kernel   rows [s0 k, (s0 + S) k) of OutT -> out (S, M, k)
//
// Splits: the 2 F feature items in chunks of PW_FCHUNK, the training points in chunks of PW_NCHUNK — functions of nothing
// (constants), so a query point's bits do not depend on M, on the batch it rides in or on how many columns the call has.
// No atomics: every sum has one order.  Phases are accumulated in fp64 on both element types and, for float, reduced to
// [-pi, pi] in fp64 before the fp32 sincos (Student-t frequencies make |theta| reach 1e4 and beyond).
// The kernels read the points up to the padded sizes (rows zero-filled) and V / W up to whole 64-item stages: V is zero
// beyond N and W beyond 2 F, so those items add nothing.  All stores are plain vector stores.
#include "gpx_cov.h"
#include "gpx_tile.h"

namespace gpx {
namespace {

constexpr int PW_MQ = 64;          // query points per workgroup: 16 per wave
constexpr int PW_CB = 64;          // columns per workgroup: four 16-column MFMA tiles
constexpr int PW_ST = 64;          // contraction items per LDS stage: 16 MFMA k-steps
constexpr int PW_LDS = PW_ST + 4;  // row stride of the slab in LDS: 16 rows x 4 k of a fragment read hit distinct banks
constexpr int64_t PW_NCHUNK = 2048;  // training points per split
constexpr int64_t PW_FCHUNK = 2048;  // feature items (of 2 F) per split

// ---- Philox4x32-10 and the normals of include/gpx.h (the stream of gpx_sample_posterior, gpx_posterior.hip) ---------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* w) {
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
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

__device__ __forceinline__ double philox_normal(uint64_t seed, uint64_t i) {
  const uint64_t n = i >> 1;
  uint32_t w[4];
  philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const double u1 = (double)((((uint64_t)w[0] << 32 | w[1]) >> 11) + 1) * 0x1.0p-53;  // (0, 1]
  const double u2 = (double)(((uint64_t)w[2] << 32 | w[3]) >> 11) * 0x1.0p-53;        // [0, 1)
  const double r = sqrt(-2.0 * log(u1));
  const double a = 6.283185307179586 * u2;
  return (i & 1) ? r * sin(a) : r * cos(a);
}

// number i of the call's flat stream: the caller's z (element type T) or the Philox stream `seed`
template <typename T>
__device__ __forceinline__ double stream_normal(const T* __restrict__ z, uint64_t seed, int64_t i) {
  return z ? (double)z[i] : philox_normal(seed, (uint64_t)i);
}

// the feature of one (item, point) pair: cosine half for item < F, sine half beyond; theta in fp64
template <typename T>
__device__ __forceinline__ T feature(double theta, bool sine, double amp) {
  if constexpr (std::is_same<T, double>::value) {
    double s, c;
    sincos(theta, &s, &c);
    return amp * (sine ? s : c);
  } else {
    const double t = theta - 6.283185307179586476925286766559 * rint(theta * 0.15915494309189533576888376337251);
    float s, c;
    sincosf((float)t, &s, &c);
    return (float)amp * (sine ? s : c);
  }
}

// One split (blockIdx.z) of the product for the 64 query points of blockIdx.x and the 64 columns of blockIdx.y:
//   z <  SF   feature items [z FCHUNK, (z + 1) FCHUNK) of the 2 F, against W
//   z >= SF   training points [(z - SF) NCHUNK, ...) of the npad, against V
// part[(z cpad + col) ldp + m].  As (mpad x d) and Bs (npad x d) are the scaled points, rows beyond the valid ones zero.
template <typename T, int KERNEL, int D>
__global__ __launch_bounds__(256) void pw_eval_kernel(const T* __restrict__ As, const T* __restrict__ Bs, int64_t npad,
                                                     int d_rt, T sf2, const T* __restrict__ V, int64_t ldv,
                                                     const double* __restrict__ Om, int64_t F, int SF,
                                                     const T* __restrict__ W, int64_t ldw, double amp,
                                                     T* __restrict__ part, int64_t ldp, int64_t cpad) {
  using N_ = Num<T>;
  constexpr int DD = D > 0 ? D : MAX_D;  // D = 0: any d <= MAX_D, loops over d at run time
  constexpr int DR = D > 0 ? D : 1;      // query coordinates held in registers (D = 0: none, re-read through the cache)
  const int d = (D > 0) ? D : d_rt;
  __shared__ double pts[PW_ST * DD];  // the stage's training points (as T) or frequencies (fp64)
  __shared__ T slab[PW_CB * PW_LDS];  // the stage's 64 columns x 64 items of V or W
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l4 = lane >> 4, l15 = lane & 15;
  const int64_t m = (int64_t)blockIdx.x * PW_MQ + w * 16 + l15;  // this lane's query point
  const int64_t cb = (int64_t)blockIdx.y * PW_CB;
  const int z = (int)blockIdx.z;
  const bool feat = z < SF;
  const T* __restrict__ xq = As + m * d;  // padded rows are readable
  T xa[DR];
#pragma unroll
  for (int c = 0; c < DR; ++c) xa[c] = xq[c];
  typename N_::v4 acc[PW_CB / 16];
#pragma unroll
  for (int t = 0; t < PW_CB / 16; ++t) acc[t] = (typename N_::v4){(T)0, (T)0, (T)0, (T)0};

  const int64_t total = feat ? 2 * F : npad;
  const int64_t jbeg = feat ? (int64_t)z * PW_FCHUNK : (int64_t)(z - SF) * PW_NCHUNK;
  const int64_t jend = jbeg + (feat ? PW_FCHUNK : PW_NCHUNK) < total ? jbeg + (feat ? PW_FCHUNK : PW_NCHUNK) : total;
  const T* __restrict__ src = feat ? W : V;
  const int64_t lds_ = feat ? ldw : ldv;
  T* ptsT = reinterpret_cast<T*>(pts);

  for (int64_t j0 = jbeg; j0 < jend; j0 += PW_ST) {
    if (feat) {
      for (int e = tid; e < PW_ST * d; e += 256) {
        const int64_t j = j0 + e / d;
        pts[e] = j < 2 * F ? Om[(j < F ? j : j - F) * d + e % d] : 0.0;
      }
    } else {
      for (int e = tid; e < PW_ST * d; e += 256) ptsT[e] = Bs[j0 * d + e];
    }
    for (int e = tid; e < PW_CB * PW_ST; e += 256) {
      const int c = e >> 6, jj = e & 63;
      slab[c * PW_LDS + jj] = src[(cb + c) * lds_ + j0 + jj];  // (zero beyond N / 2 F: see the head of the file)
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < PW_ST / 4; ++t) {
      const int jj = 4 * t + l4;
      T val;
      if (feat) {
        double th = 0.0;
        if constexpr (D > 0) {
#pragma unroll
          for (int c = 0; c < D; ++c) th += pts[jj * D + c] * (double)xa[c];
        } else {
          for (int c = 0; c < d; ++c) th += pts[jj * d + c] * (double)xq[c];
        }
        val = feature<T>(th, j0 + jj >= F, amp);
      } else {
        T r2 = (T)0;
        if constexpr (D > 0) {
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const T df = xa[c] - ptsT[jj * D + c];
            r2 += df * df;
          }
        } else {
          for (int c = 0; c < d; ++c) {
            const T df = xq[c] - ptsT[jj * d + c];
            r2 += df * df;
          }
        }
        val = cov::value<KERNEL>(r2, sf2);
      }
#pragma unroll
      for (int q = 0; q < PW_CB / 16; ++q) acc[q] = N_::mfma(slab[(q * 16 + l15) * PW_LDS + jj], val, acc[q]);
    }
    __syncthreads();
  }
  // accumulator register r of lane l = element (drow(l >> 4, r), l & 15) of its tile: column x query point
#pragma unroll
  for (int q = 0; q < PW_CB / 16; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[((int64_t)z * cpad + cb + q * 16 + N_::drow(l4, r)) * ldp + m] = acc[q][r];
}

// outT[c ldo + m] = sum over the splits, in order, of part[(z cpad + c) ldp + m], c < cpad, m < mpad
template <typename T>
__global__ __launch_bounds__(256) void pw_finish_kernel(const T* __restrict__ part, int64_t ldp, int nz, int64_t cpad,
                                                       int64_t mpad, T* __restrict__ outT, int64_t ldo) {
  const int64_t total = cpad * mpad;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t c = e / mpad, mm = e - c * mpad;
    T acc = (T)0;
    for (int q = 0; q < nz; ++q) acc += part[((int64_t)q * cpad + c) * ldp + mm];
    outT[c * ldo + mm] = acc;
  }
}

// Omega and W from the flat stream (include/gpx.h): numbers [f (d + q), (f + 1)(d + q)) are g_f then the q chi normals of
// frequency f; then per column a block of 2 F + N numbers, W[col][:] first.  Omega_f = g_f sqrt(q / chi_f) (q = 0: g_f).
template <typename T>
__global__ __launch_bounds__(256) void pw_draw_kernel(const T* __restrict__ z, uint64_t seed, int64_t F, int d, int q,
                                                     int64_t C, int64_t cpad, int64_t N, double* __restrict__ Om,
                                                     T* __restrict__ W, int64_t ldw) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cpad * ldw; i += (int64_t)gridDim.x * 256) {
    const int64_t col = i / ldw, j = i - col * ldw;
    W[i] = (col < C && j < 2 * F) ? (T)stream_normal(z, seed, F * (d + q) + col * (2 * F + N) + j) : (T)0;
  }
  // one lane per entry of Omega (each forms its frequency's chi again: q <= 5 numbers)
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < F * d; e += (int64_t)gridDim.x * 256) {
    const int64_t f = e / d, base = f * (d + q);
    double chi = 0.0;
    for (int j = 0; j < q; ++j) {
      const double x = stream_normal(z, seed, base + d + j);
      chi += x * x;
    }
    const double g = stream_normal(z, seed, base + (e - f * d));
    Om[e] = q == 0 ? g : chi > 0.0 ? g * sqrt((double)q / chi) : 0.0;  // (chi = 0: only a caller's all-zero z)
  }
}

// R[col ldr + n] = y[n k + c] - FT[col ldf + n] - sqrt(sn2 w_n) E[col][n] for col = s k + c < C, n < N; zero elsewhere up
// to cpad rows and npad columns (what the triangular solves read).  R may be FT: an element is read, then written, by one lane.
template <typename T>
__global__ __launch_bounds__(256) void pw_resid_kernel(const T* __restrict__ y, const T* FT, int64_t ldf,
                                                      const T* __restrict__ wv, double sn2, const T* __restrict__ z,
                                                      uint64_t seed, int64_t ebase, int64_t F, int64_t N, int64_t npad,
                                                      int k, int64_t C, int64_t cpad, T* R, int64_t ldr) {
  const int64_t total = cpad * npad;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t col = e / npad, n = e - col * npad;
    T r = (T)0;
    if (col < C && n < N) {
      const double sd = sqrt(sn2 * (wv ? (double)wv[n] : 1.0));
      const double eps = sd * stream_normal(z, seed, ebase + col * (2 * F + N) + 2 * F + n);
      r = (T)((double)y[n * k + col % k] - (double)FT[col * ldf + n] - eps);
    }
    R[col * ldr + n] = r;
  }
}

// out[((s - s0) M + m) k + c] = outT[(s k + c - r0) ldo + m] for s0 <= s < s0 + S (r0: the first row outT holds)
template <typename T>
__global__ __launch_bounds__(256) void pw_unpack_kernel(const T* __restrict__ outT, int64_t ldo, int64_t r0, int64_t s0,
                                                       int64_t S, int64_t M, int64_t m0, int64_t mv, int k,
                                                       T* __restrict__ out) {
  const int64_t total = S * mv * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t s = e / (mv * k), rem = e - s * mv * k, mm = rem / k, c = rem - mm * k;
    out[(s * M + m0 + mm) * k + c] = outT[((s0 + s) * k + c - r0) * ldo + mm];
  }
}

unsigned grid_for(int64_t work) {
  const int64_t b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

template <typename T, int KERNEL>
void eval_d(dim3 grid, const T* As, const T* Bs, int64_t npad, int d, double sf2, const T* V, int64_t ldv, const double* Om,
            int64_t F, int SF, const T* W, int64_t ldw, double amp, T* part, int64_t ldp, int64_t cpad, hipStream_t st) {
#define PW_LAUNCH(DV)                                                                                                    \
  hipLaunchKernelGGL((pw_eval_kernel<T, KERNEL, DV>), grid, dim3(256), 0, st, As, Bs, npad, d, (T)sf2, V, ldv, Om, F, SF, W, \
                     ldw, amp, part, ldp, cpad)
  switch (d) {
    case 1: PW_LAUNCH(1); break;
    case 2: PW_LAUNCH(2); break;
    case 3: PW_LAUNCH(3); break;
    default: PW_LAUNCH(0); break;
  }
#undef PW_LAUNCH
}

}  // namespace

int pathwise_chi_dof(int kernel) {
  return kernel == GPX_KERNEL_MATERN52 ? 5 : kernel == GPX_KERNEL_MATERN32 ? 3 : kernel == GPX_KERNEL_MATERN12 ? 1 : 0;
}

int pathwise_splits(int64_t npad, int64_t F, bool with_v) {
  const int64_t sf = (2 * F + PW_FCHUNK - 1) / PW_FCHUNK, sn = with_v ? (npad + PW_NCHUNK - 1) / PW_NCHUNK : 0;
  return (int)(sf + sn);
}

template <typename T>
void launch_pathwise_eval(int kernel, const T* As, int64_t mpad, const T* Bs, int64_t npad, int d, double sf2, const T* V,
                          int64_t ldv, const double* Om, int64_t F, const T* W, int64_t ldw, int64_t cpad, T* part, T* outT,
                          int64_t ldo, hipStream_t st) {
  if (mpad <= 0 || cpad <= 0) return;
  const int SF = pathwise_splits(npad, F, false), nz = pathwise_splits(npad, F, V != nullptr);
  const dim3 grid((unsigned)(mpad / PW_MQ), (unsigned)(cpad / PW_CB), (unsigned)nz);
  const double amp = sqrt(sf2 / (double)F);
  cov::dispatch(kernel, [&](auto fam) { eval_d<T, fam>(grid, As, Bs, npad, d, sf2, V, ldv, Om, F, SF, W, ldw, amp, part, mpad, cpad, st); });
  hipLaunchKernelGGL(pw_finish_kernel<T>, dim3(grid_for(cpad * mpad)), dim3(256), 0, st, part, mpad, nz, cpad, mpad, outT, ldo);
}

template <typename T>
void launch_pathwise_draw(const T* z, uint64_t seed, int64_t F, int d, int q, int64_t C, int64_t cpad, int64_t N, double* Om,
                          T* W, int64_t ldw, hipStream_t st) {
  hipLaunchKernelGGL(pw_draw_kernel<T>, dim3(grid_for(F + cpad * ldw)), dim3(256), 0, st, z, seed, F, d, q, C, cpad, N, Om, W,
                     ldw);
}

template <typename T>
void launch_pathwise_resid(const T* y, const T* FT, int64_t ldf, const T* wv, double sn2, const T* z, uint64_t seed,
                           int64_t ebase, int64_t F, int64_t N, int64_t npad, int k, int64_t C, int64_t cpad, T* R,
                           int64_t ldr, hipStream_t st) {
  hipLaunchKernelGGL(pw_resid_kernel<T>, dim3(grid_for(cpad * npad)), dim3(256), 0, st, y, FT, ldf, wv, sn2, z, seed, ebase, F,
                     N, npad, k, C, cpad, R, ldr);
}

template <typename T>
void launch_pathwise_unpack(const T* outT, int64_t ldo, int64_t r0, int64_t s0, int64_t S, int64_t M, int64_t m0, int64_t mv,
                            int k, T* out, hipStream_t st) {
  if (S <= 0 || mv <= 0) return;
  hipLaunchKernelGGL(pw_unpack_kernel<T>, dim3(grid_for(S * mv * k)), dim3(256), 0, st, outT, ldo, r0, s0, S, M, m0, mv, k,
                     out);
}

#define GPX_INSTANTIATE_PATHWISE(T)                                                                                        \
  template void launch_pathwise_eval<T>(int, const T*, int64_t, const T*, int64_t, int, double, const T*, int64_t,        \
                                        const double*, int64_t, const T*, int64_t, int64_t, T*, T*, int64_t, hipStream_t); \
  template void launch_pathwise_draw<T>(const T*, uint64_t, int64_t, int, int, int64_t, int64_t, int64_t, double*, T*,    \
                                        int64_t, hipStream_t);                                                           \
  template void launch_pathwise_resid<T>(const T*, const T*, int64_t, const T*, double, const T*, uint64_t, int64_t,      \
                                         int64_t, int64_t, int64_t, int, int64_t, int64_t, T*, int64_t, hipStream_t);     \
  template void launch_pathwise_unpack<T>(const T*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int,   \
                                          T*, hipStream_t);
GPX_INSTANTIATE_PATHWISE(double)
GPX_INSTANTIATE_PATHWISE(float)

}  // namespace gpx
