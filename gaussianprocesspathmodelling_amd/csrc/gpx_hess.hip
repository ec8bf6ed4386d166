// gpx_hess.hip — the kernels of the posterior second derivatives (gpx_predict_hess / gpx_kernel_hess_matrix, include/gpx.h;
// DESIGN.md §3.4p).
//
// With g and h of the family (gpx_cov.h), u = x* / l - x / l:  d^2 k / d x*_i d x*_j = (h u_i u_j - g delta_ij) / (l_i l_j),
// the negative of cov::element(i, j): one exponential per (query, training) pair serves all D2 = d (d + 1) / 2 pairs
// (i, j), i <= j, row-major.  Only the twice differentiable families (RBF, Matern-5/2) are instantiated: the launchers
// below do nothing for the others (gpx_api.hip refuses the calls before any launch).  The two routes are the gradient's
// (gpx_deriv.hip):
//   mean only:      hmean = (d_i d_j K*) alpha, matrix-free (khess_matvec_kernel + khess_finish_kernel), no solve
//   with variance:  V = [d_i d_j K*] (khess_build_kernel) -> the gradient's forward solve, z^T V, row norms and unpack
// All stores are plain vector stores; every reduction runs in a fixed order (bit-reproducible).
#include <algorithm>
#include <climits>

#include "gpx_cov.h"
#include "gpx_internal.h"

namespace gpx {
namespace {

constexpr int GT = 64;  // tile edge of the build, query rows per workgroup of the matrix-free product

// D2 row blocks of V (each mpad rows, ld), block (i, j) = d^2 k(As, Bs) / d As_i d As_j: kgrad_build_kernel's tiling, lane
// map, padding (zero beyond m rows / n columns) and non-temporal 16-byte stores; r^2 and the exponential once per pair,
// D2 stores of it.  HBM-write-bound.
// KINDS: the columns are observations with a kind (kcol readable up to the padded size, -1 there): against a derivative
// column of kind c the entry is the third derivative d^3 k / d x*_i d x*_j d x_c (cov::hess_element, needs p).  A tile whose
// 64 column kinds are all -1 — decided once per workgroup — takes the path, and gives the numbers, of the plain build.
// GROUPS (never with KINDS): rows and columns carry path ids (krow / kcol, -1 up to the padded sizes), q holds
// q_c = (l_c / l_path,c)^2, and a same-path pair gains the Hessian of sg2 k(., .; l_path): with e = u* - u and
// 1 / l_path,c = sqrt(q_c) / l_c that is (h_p (q_i e_i) (q_j e_j) - g_p q_i delta_ij) / (l_i l_j), g_p and h_p at
// r_path^2 = sum_c q_c e_c^2.  Whether the tile can hold a same-path pair is decided once per workgroup, as
// kgrad_build_kernel does; a tile that cannot takes the path, and gives the numbers, of the plain build.
template <typename T, int KERNEL, int D, bool KINDS = false, bool GROUPS = false>
__global__ __launch_bounds__(256) void khess_build_kernel(const T* __restrict__ As, int64_t m, const T* __restrict__ Bs,
                                                         int64_t n, int d_rt, int tiles_n, T sf2,
                                                         const double* __restrict__ ls, int n_ls, T* __restrict__ V,
                                                         int64_t ld, int64_t mpad,
                                                         const int32_t* __restrict__ kcol = nullptr,
                                                         const int32_t* __restrict__ krow = nullptr,
                                                         const double* __restrict__ q = nullptr, T sg2 = (T)0) {
  static_assert(!(KINDS && GROUPS), "a fit has kinds or path ids, never both");
  constexpr int DD = D > 0 ? D : MAX_HESS_D;
  const int d = (D > 0) ? D : d_rt;
  __shared__ T xa[GT * DD];
  __shared__ T xb[GT * DD];
  __shared__ T il[DD];
  const int ti = (int)(blockIdx.x / tiles_n), tj = (int)(blockIdx.x - (int64_t)ti * tiles_n);
  const int64_t i0 = (int64_t)ti * GT, j0 = (int64_t)tj * GT;
  const int tid = threadIdx.x;
  for (int e = tid; e < GT * d; e += 256) {
    xa[e] = As[i0 * d + e];  // rows of the padded point arrays are always readable
    xb[e] = Bs[j0 * d + e];
  }
  if (tid < d) il[tid] = (T)(1.0 / ls[n_ls == 1 ? 0 : tid]);
  bool mixed = false;
  const int* skb = nullptr;
  [[maybe_unused]] const T* sq = nullptr;
  if constexpr (KINDS) {
    __shared__ int kbs[GT];
    int deriv = 0;
    if (tid >= 256 - GT) {  // (the last wave: the first ones stage 1 / l)
      const int kk = kcol[j0 + tid - (256 - GT)];
      kbs[tid - (256 - GT)] = kk;
      deriv = kk >= 0;
    }
    mixed = __syncthreads_or(deriv) != 0;
    skb = kbs;
  } else if constexpr (GROUPS) {
    __shared__ int gab[2 * GT];
    __shared__ int rng[4];  // lowest / highest non-negative id of the rows, of the columns
    __shared__ T qv[DD];
    if (tid >= 256 - 2 * GT) {  // wave 2: the rows, wave 3: the columns (the first ones stage 1 / l)
      const int t = tid - (256 - 2 * GT);
      const int id = t < GT ? krow[i0 + t] : kcol[j0 + t - GT];
      gab[t] = id;
      int lo = id >= 0 ? id : INT_MAX, hi = id;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
      }
      if ((t & 63) == 0) rng[2 * (t >> 6)] = lo, rng[2 * (t >> 6) + 1] = hi;
    } else if (tid >= GT && tid - GT < d) {
      qv[tid - GT] = (T)q[tid - GT];
    }
    __syncthreads();
    mixed = rng[0] <= rng[3] && rng[2] <= rng[1];  // (no id >= 0 on a side: lo = INT_MAX, hi < 0)
    skb = gab;
    sq = qv;
  } else {
    __syncthreads();
  }
  const int c2 = (tid & 31) * 2;
  const int rg = tid >> 5;
  const int64_t col0 = j0 + c2, col1 = col0 + 1;
  const int64_t blk = mpad * ld;  // elements per row block
  typedef T pair_t __attribute__((ext_vector_type(2)));
  if constexpr (GROUPS) {
    // a loop of its own, so that the last loop stays, statement for statement, the plain build's (kgrad_build_kernel)
    if (mixed) {
#pragma unroll 1
      for (int r = 0; r < 8; ++r) {
        const int ir = rg + 8 * r;
        const int64_t row = i0 + ir;
        const T* pa = xa + ir * d;
        const T *pb0 = xb + c2 * d, *pb1 = pb0 + d;
        T s0 = (T)0, s1 = (T)0, p0 = (T)0, p1 = (T)0;  // r^2 and r_path^2 of the lane's two pairs
        for (int c = 0; c < d; ++c) {
          const T e0 = pa[c] - pb0[c], e1 = pa[c] - pb1[c];
          s0 += e0 * e0;
          s1 += e1 * e1;
          p0 += sq[c] * (e0 * e0);
          p1 += sq[c] * (e1 * e1);
        }
        T v0, g0, h0, v1, g1, h1;
        cov::value_gh<KERNEL>(s0, sf2, v0, g0, h0);
        cov::value_gh<KERNEL>(s1, sf2, v1, g1, h1);
        const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
        T* out = V + row * ld + col0;
        const int ga = skb[ir];
        // one branch for the lane's two pairs (kgrad_build_kernel); a pair of two paths keeps pg = ph = 0
        T pv, pg0 = (T)0, ph0 = (T)0, pg1 = (T)0, ph1 = (T)0;
        const bool m0 = ga >= 0 && ga == skb[GT + c2], m1 = ga >= 0 && ga == skb[GT + c2 + 1];
        if (m0 || m1) {
          cov::value_gh<KERNEL>(p0, sg2, pv, pg0, ph0);
          cov::value_gh<KERNEL>(p1, sg2, pv, pg1, ph1);
          if (!m0) pg0 = ph0 = (T)0;
          if (!m1) pg1 = ph1 = (T)0;
        }
        int b = 0;
        for (int i = 0; i < d; ++i) {
          const T ui0 = pa[i] - pb0[i], ui1 = pa[i] - pb1[i];
          for (int j = i; j < d; ++j, ++b) {
            const T uj0 = pa[j] - pb0[j], uj1 = pa[j] - pb1[j];
            const T qd = i == j ? sq[i] : (T)0;
            const T w0 = -cov::element<T>(i, j, v0, g0, h0, ui0, uj0, il[i], il[j]) +
                         (ph0 * ((sq[i] * ui0) * (sq[j] * uj0)) - pg0 * qd) * (il[i] * il[j]);
            const T w1 = -cov::element<T>(i, j, v1, g1, h1, ui1, uj1, il[i], il[j]) +
                         (ph1 * ((sq[i] * ui1) * (sq[j] * uj1)) - pg1 * qd) * (il[i] * il[j]);
            pair_t w = {ok0 ? w0 : (T)0, ok1 ? w1 : (T)0};
            __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + b * blk));
          }
        }
      }
      return;
    }
  }
  if constexpr (KINDS) {
    // a tile with a derivative column has a loop of its own as well: sharing the plain loop, the compiler formed g of
    // Matern-5/2 from operands the third derivative also uses and gave the value columns other last bits
    if (mixed) {
#pragma unroll 1
      for (int r = 0; r < 8; ++r) {
        const int ir = rg + 8 * r;
        const int64_t row = i0 + ir;
        const T* pa = xa + ir * d;
        const T *pb0 = xb + c2 * d, *pb1 = pb0 + d;
        T s0 = (T)0, s1 = (T)0;
        for (int c = 0; c < d; ++c) {
          const T e0 = pa[c] - pb0[c], e1 = pa[c] - pb1[c];
          s0 += e0 * e0;
          s1 += e1 * e1;
        }
        const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
        T* out = V + row * ld + col0;
        T v0, g0, h0, t0, v1, g1, h1, t1;
        cov::value_ghp<KERNEL>(s0, sf2, v0, g0, h0, t0);
        cov::value_ghp<KERNEL>(s1, sf2, v1, g1, h1, t1);
        const int kb0 = skb[c2], kb1 = skb[c2 + 1];
        const int cb0 = kb0 < 0 ? 0 : kb0, cb1 = kb1 < 0 ? 0 : kb1;  // (kinds < d: the API checks)
        const T ub0 = pa[cb0] - pb0[cb0], ub1 = pa[cb1] - pb1[cb1], ilb0 = il[cb0], ilb1 = il[cb1];
        int b = 0;
        for (int i = 0; i < d; ++i) {
          const T ui0 = pa[i] - pb0[i], ui1 = pa[i] - pb1[i];
          for (int j = i; j < d; ++j, ++b) {
            const T uj0 = pa[j] - pb0[j], uj1 = pa[j] - pb1[j];
            pair_t w = {ok0 ? cov::hess_element<T>(i, j, kb0, v0, g0, h0, t0, ui0, uj0, ub0, il[i], il[j], ilb0) : (T)0,
                        ok1 ? cov::hess_element<T>(i, j, kb1, v1, g1, h1, t1, ui1, uj1, ub1, il[i], il[j], ilb1) : (T)0};
            __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + b * blk));
          }
        }
      }
      return;
    }
  }
  constexpr int ROWS_IN_FLIGHT = D > 0 ? 2 : 1;
#pragma unroll ROWS_IN_FLIGHT
  for (int r = 0; r < 8; ++r) {
    const int ir = rg + 8 * r;
    const int64_t row = i0 + ir;
    const T* pa = xa + ir * d;
    const T *pb0 = xb + c2 * d, *pb1 = pb0 + d;
    T s0 = (T)0, s1 = (T)0;
    for (int c = 0; c < d; ++c) {
      const T e0 = pa[c] - pb0[c], e1 = pa[c] - pb1[c];
      s0 += e0 * e0;
      s1 += e1 * e1;
    }
    const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
    T* out = V + row * ld + col0;
    T v0, g0, h0, v1, g1, h1;
    cov::value_gh<KERNEL>(s0, sf2, v0, g0, h0);
    cov::value_gh<KERNEL>(s1, sf2, v1, g1, h1);
    int b = 0;
    for (int i = 0; i < d; ++i) {
      const T ui0 = pa[i] - pb0[i], ui1 = pa[i] - pb1[i];
      for (int j = i; j < d; ++j, ++b) {
        const T uj0 = pa[j] - pb0[j], uj1 = pa[j] - pb1[j];
        pair_t w = {ok0 ? -cov::element<T>(i, j, v0, g0, h0, ui0, uj0, il[i], il[j]) : (T)0,
                    ok1 ? -cov::element<T>(i, j, v1, g1, h1, ui1, uj1, il[i], il[j]) : (T)0};
        __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + b * blk));
      }
    }
  }
}

// Matrix-free mean Hessian, partial over the training columns [s chunk, (s + 1) chunk) of split s = blockIdx.z:
//   part[((s k + c) D2 + b) ldp + i] = sum_n (h u_i' u_j' - g delta_i'j')(x*_i, x_n) alphaT[c][n],   b = pair (i', j')
// for the 64 query rows of blockIdx.x and the targets [KC blockIdx.y, KC blockIdx.y + KC): kgrad_matvec_kernel's structure
// (LDS-broadcast columns, each wave 16 of every 64, the four waves summed in a fixed order; no atomics).  One exponential
// per pair serves all D2 second derivatives and the KC targets of the workgroup; 1 / (l_i' l_j') waits for the finish.
template <typename T, int KERNEL, int D, int KC>
__global__ __launch_bounds__(256) void khess_matvec_kernel(const T* __restrict__ As, const T* __restrict__ Bs,
                                                          int64_t npad, int64_t chunk, int d_rt, T sf2,
                                                          const T* __restrict__ alphaT, int64_t lda, int k,
                                                          T* __restrict__ part, int64_t ldp) {
  constexpr int DD = D > 0 ? D : MAX_HESS_D;
  constexpr int PP = DD * (DD + 1) / 2;
  const int d = (D > 0) ? D : d_rt;
  const int d2 = d * (d + 1) / 2;
  __shared__ T xb[GT * DD];
  __shared__ T ab[KC * GT];
  __shared__ T red[3 * GT];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * GT + lane;
  const int cb = (int)blockIdx.y * KC;
  const int s = (int)blockIdx.z;
  const int64_t jbeg = (int64_t)s * chunk, jend = jbeg + chunk < npad ? jbeg + chunk : npad;
  T xa[DD];
#pragma unroll
  for (int c = 0; c < DD; ++c)
    if (D > 0 || c < d) xa[c] = As[i * d + c];  // padded rows are readable
  T acc[KC][PP];
#pragma unroll
  for (int t = 0; t < KC; ++t)
#pragma unroll
    for (int b = 0; b < PP; ++b) acc[t][b] = (T)0;
  for (int64_t j0 = jbeg; j0 < jend; j0 += GT) {
    for (int e = tid; e < GT * d; e += 256) xb[e] = Bs[j0 * d + e];
    for (int e = tid; e < KC * GT; e += 256) {
      const int t = e >> 6;
      ab[e] = (cb + t < k) ? alphaT[(int64_t)(cb + t) * lda + j0 + (e & 63)] : (T)0;
    }
    __syncthreads();
    for (int jj = g * 16; jj < g * 16 + 16; ++jj) {
      T df[DD];
      T r2 = (T)0;
#pragma unroll
      for (int c = 0; c < DD; ++c) {
        df[c] = (T)0;
        if (D > 0 || c < d) {
          df[c] = xa[c] - xb[jj * d + c];
          r2 += df[c] * df[c];
        }
      }
      T v, gf, hf;
      cov::value_gh<KERNEL>(r2, sf2, v, gf, hf);
      // the pairs in the full-width order (a, b), a <= b < DD: static register indices; finish maps them to d's own
      T w[PP];
      {
        int b = 0;
#pragma unroll
        for (int a = 0; a < DD; ++a)
#pragma unroll
          for (int c = a; c < DD; ++c, ++b) w[b] = hf * (df[a] * df[c]) - (a == c ? gf : (T)0);
      }
#pragma unroll
      for (int t = 0; t < KC; ++t) {
        const T al = ab[t * GT + jj];
#pragma unroll
        for (int b = 0; b < PP; ++b) acc[t][b] += al * w[b];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < KC; ++t) {
    int b = 0, bo = 0;  // pair number at width DD, at width d
#pragma unroll
    for (int a = 0; a < DD; ++a)
#pragma unroll
      for (int c = a; c < DD; ++c, ++b) {
        if (D == 0 && c >= d) continue;  // d is uniform: every wave skips the same barriers
        if (g > 0) red[(g - 1) * GT + lane] = acc[t][b];
        __syncthreads();
        if (g == 0 && cb + t < k) {
          const T v = ((acc[t][b] + red[lane]) + red[GT + lane]) + red[2 * GT + lane];
          part[(((int64_t)s * k + cb + t) * d2 + bo) * ldp + i] = v;
        }
        __syncthreads();
        ++bo;
      }
  }
}

// hmean (M, D2, k)[m][b][c] = (sum over the S splits, in order, of part) / (l_i l_j), b = pair (i, j)
template <typename T>
__global__ __launch_bounds__(256) void khess_finish_kernel(const T* __restrict__ part, int64_t ldp, int S, int64_t M,
                                                          int d, int k, const double* __restrict__ ls, int n_ls,
                                                          T* __restrict__ out) {
  const int d2 = d * (d + 1) / 2;
  const int64_t total = M * d2 * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / ((int64_t)d2 * k);
    const int rem = (int)(e - m * d2 * k);
    const int b = rem / k, c = rem - b * k;
    int i = 0, first = 0;  // row i of the upper triangle holds the pairs [first, first + d - i)
    while (b >= first + d - i) first += d - i, ++i;
    const int j = i + b - first;
    T acc = (T)0;
    for (int t = 0; t < S; ++t) acc += part[(((int64_t)t * k + c) * d2 + b) * ldp + m];
    out[e] = acc * ((T)(1.0 / ls[n_ls == 1 ? 0 : i]) * (T)(1.0 / ls[n_ls == 1 ? 0 : j]));
  }
}

unsigned grid_for(int64_t work) {
  const int64_t b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

template <typename T, int KERNEL, int D>
void build_kg(dim3 grid, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int d, int tn, double sf2,
              const double* ls, int n_ls, T* V, int64_t ld, hipStream_t st, const int32_t* kcol, const int32_t* grow,
              const double* q, double sg2) {
  const dim3 block(256);
  const T s = (T)sf2, sg = (T)sg2;
  if (grow)  // rows and columns with path ids (kcol: the columns')
    hipLaunchKernelGGL((khess_build_kernel<T, KERNEL, D, false, true>), grid, block, 0, st, As, m, Bs, n, d, tn, s, ls, n_ls, V, ld, mpad, kcol, grow, q, sg);
  else if (kcol)  // observations with kinds
    hipLaunchKernelGGL((khess_build_kernel<T, KERNEL, D, true>), grid, block, 0, st, As, m, Bs, n, d, tn, s, ls, n_ls, V, ld, mpad, kcol);
  else
    hipLaunchKernelGGL((khess_build_kernel<T, KERNEL, D>), grid, block, 0, st, As, m, Bs, n, d, tn, s, ls, n_ls, V, ld, mpad);
}

template <typename T, int KERNEL>
void build_d(const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d, double sf2,
             const double* ls, int n_ls, T* V, int64_t ld, hipStream_t st, const int32_t* kcol, const int32_t* grow,
             const double* q, double sg2) {
  const int64_t tm = mpad / GT, tn = npad / GT;
  const dim3 grid((unsigned)(tm * tn));
  switch (d) {
    case 1: build_kg<T, KERNEL, 1>(grid, As, m, mpad, Bs, n, d, (int)tn, sf2, ls, n_ls, V, ld, st, kcol, grow, q, sg2); break;
    case 2: build_kg<T, KERNEL, 2>(grid, As, m, mpad, Bs, n, d, (int)tn, sf2, ls, n_ls, V, ld, st, kcol, grow, q, sg2); break;
    case 3: build_kg<T, KERNEL, 3>(grid, As, m, mpad, Bs, n, d, (int)tn, sf2, ls, n_ls, V, ld, st, kcol, grow, q, sg2); break;
    default: build_kg<T, KERNEL, 0>(grid, As, m, mpad, Bs, n, d, (int)tn, sf2, ls, n_ls, V, ld, st, kcol, grow, q, sg2); break;
  }
}

template <typename T, int KERNEL, int D, int KC>
void matvec_launch(dim3 grid, const T* As, const T* Bs, int64_t npad, int64_t chunk, int d, double sf2, const T* alphaT,
                   int64_t lda, int k, T* part, int64_t ldp, hipStream_t st) {
  hipLaunchKernelGGL((khess_matvec_kernel<T, KERNEL, D, KC>), grid, dim3(256), 0, st, As, Bs, npad, chunk, d, (T)sf2,
                     alphaT, lda, k, part, ldp);
}

template <typename T, int KERNEL, int D>
void matvec_kc(dim3 grid, int KC, const T* As, const T* Bs, int64_t npad, int64_t chunk, int d, double sf2,
               const T* alphaT, int64_t lda, int k, T* part, int64_t ldp, hipStream_t st) {
  if (KC == 1)
    matvec_launch<T, KERNEL, D, 1>(grid, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st);
  else if (KC == 2)
    matvec_launch<T, KERNEL, D, 2>(grid, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st);
  else
    matvec_launch<T, KERNEL, D, 4>(grid, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st);
}

template <typename T, int KERNEL>
void matvec_d(dim3 grid, int KC, const T* As, const T* Bs, int64_t npad, int64_t chunk, int d, double sf2,
              const T* alphaT, int64_t lda, int k, T* part, int64_t ldp, hipStream_t st) {
  switch (d) {
    case 1: matvec_kc<T, KERNEL, 1>(grid, KC, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st); break;
    case 2: matvec_kc<T, KERNEL, 2>(grid, KC, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st); break;
    case 3: matvec_kc<T, KERNEL, 3>(grid, KC, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st); break;
    default: matvec_launch<T, KERNEL, 0, 1>(grid, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, ldp, st); break;
  }
}

// f over the twice differentiable families: not instantiated for the others, whose ids call nothing
template <typename F>
void dispatch_twice(int kernel, F&& f) {
  cov::dispatch(kernel, [&](auto K) {
    if constexpr (cov::twice_differentiable(K)) f(K);
  });
}

}  // namespace

template <typename T>
void launch_khess_build(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                        const int32_t* side_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                        const double* q, double sg2, T* V, int64_t ld, hipStream_t st) {
  if (d < 1 || d > MAX_HESS_D) return;
  dispatch_twice(kernel, [&](auto fam) { build_d<T, fam>(As, m, mpad, Bs, n, npad, d, sf2, ls, n_ls, V, ld, st, side_b, group_a, q, sg2); });
}

template <typename T>
void launch_khess_matvec(int kernel, const T* As, int64_t M, const T* Bs, int64_t npad, int d, double sf2,
                         const T* alphaT, int64_t lda, int k, const double* ls, int n_ls, T* part, T* hmean,
                         hipStream_t st) {
  if (d < 1 || d > MAX_HESS_D) return;
  int KC = 1, S = 1;
  int64_t chunk = npad;
  kgrad_matvec_shape(M, npad, d, k, &KC, &S, &chunk);
  const int64_t mpad = round_up(M, GT);
  const dim3 grid((unsigned)(mpad / GT), (unsigned)((k + KC - 1) / KC), (unsigned)S);
  dispatch_twice(kernel, [&](auto fam) {
    matvec_d<T, fam>(grid, KC, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, mpad, st);
    hipLaunchKernelGGL(khess_finish_kernel<T>, dim3(grid_for(M * hess_pairs(d) * k)), dim3(256), 0, st, part, mpad, S, M,
                       d, k, ls, n_ls, hmean);
  });
}

#define GPX_INSTANTIATE_HESS(T)                                                                                        \
  template void launch_khess_build<T>(int, const T*, const int32_t*, int64_t, int64_t, const T*, const int32_t*,      \
                                      int64_t, int64_t, int, double, const double*, int, const double*, double, T*,   \
                                      int64_t, hipStream_t);                                                          \
  template void launch_khess_matvec<T>(int, const T*, int64_t, const T*, int64_t, int, double, const T*, int64_t, int, \
                                       const double*, int, T*, T*, hipStream_t);
GPX_INSTANTIATE_HESS(double)
GPX_INSTANTIATE_HESS(float)

}  // namespace gpx
