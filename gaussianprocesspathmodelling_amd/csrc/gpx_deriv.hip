// gpx_deriv.hip — the kernels of the posterior gradient (gpx_predict_grad / gpx_kernel_grad_matrix / gpx_kernel_deriv_matrix, include/gpx.h).
//
// With g of the family (gpx_cov.h), d k / d x*_j = -g (u*_j - u_j) / l_j and u = x / l: one exponential per
// (query, training) pair.  Matern-1/2 has no derivative at r = 0: the launchers below do nothing for it (gpx_api.hip
// refuses the calls before any launch).  Everything heavy beyond these kernels is the existing engine (gpx_api.hip):
//   mean only:      dmean = dK* alpha, matrix-free (kgrad_matvec_kernel + kgrad_finish_kernel), no solve
//   with variance:  V = [K*; d_1 K*; ...; d_d K*] (kgrad_build_kernel) -> ONE forward solve over all rows -> ONE split-K
//                   z^T V (mean and dmean together) -> row norms with a per-row-block prior -> unpack
// All stores are plain vector stores; every reduction runs in a fixed order (bit-reproducible).
#include <algorithm>
#include <climits>

#include "gpx_cov.h"
#include "gpx_internal.h"

namespace gpx {
namespace {

constexpr int GT = 64;      // tile edge of the build, query rows per workgroup of the matrix-free product

// Row blocks of V (each mpad rows, ld): [K* if with_value] then d_1 K* ... d_d K*; tile (ti, tj) of 64 x 64 per
// workgroup, the same lane map, padding (zero beyond m rows / n columns) and non-temporal 16-byte stores as
// kbuild_kernel; r^2 and the exponential once per pair, 1 + d stores of it.  HBM-write-bound.
// KINDS: the columns are observations with a kind (gpx_cov.h; kcol readable up to the padded size, -1 there): against a
// derivative column the value rows hold the (-1, j) element and the d_i K* rows the (i, j) element (cov::element).  A tile
// whose 64 column kinds are all -1 — decided once per workgroup — takes the path, and gives the numbers, of the plain build.
// GROUPS (never with KINDS): rows and columns carry path ids (krow / kcol, readable up to the padded sizes, -1 there) and a
// same-path pair gets + sg2 k(., .; l_path) and its derivative; q holds q_c = (l_c / l_path,c)^2 (d
// entries).  The 64 + 64 ids and q are staged beside the points; whether the tile can hold a same-path pair — the ranges of
// the non-negative row and column ids overlap — is decided once per workgroup, wave-uniform, as kbuild_kernel does.  A tile
// that cannot takes the path, and gives the numbers, of the plain build.  Otherwise r_path^2 = sum_c q_c e_c^2 beside r^2, from
// the same differences e_c, and where the ids match the value row gains cov::value_g's v and row block j gains -g_path q_j e_j / l_j: with u' = x / l_path, u'_j - u'_j' = sqrt(q_j) e_j and
// d / d x_j = -g_path (u'_j - u'_j') / l_path,j.  One more exponential per matching pair, none for the others.
template <typename T, int KERNEL, int D, bool KINDS = false, bool GROUPS = false>
__global__ __launch_bounds__(256) void kgrad_build_kernel(const T* __restrict__ As, int64_t m, const T* __restrict__ Bs,
                                                         int64_t n, int d_rt, int tiles_n, T sf2,
                                                         const double* __restrict__ ls, int n_ls, int with_value,
                                                         T* __restrict__ V, int64_t ld, int64_t mpad,
                                                         const int32_t* __restrict__ kcol = nullptr,
                                                         const int32_t* __restrict__ krow = nullptr,
                                                         const double* __restrict__ q = nullptr, T sg2 = (T)0) {
  static_assert(!(KINDS && GROUPS), "a fit has kinds or path ids, never both");
  const int d = (D > 0) ? D : d_rt;
  __shared__ T xa[GT * (D > 0 ? D : MAX_D)];
  __shared__ T xb[GT * (D > 0 ? D : MAX_D)];
  __shared__ T il[MAX_D];
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
    __shared__ T qv[D > 0 ? D : MAX_D];
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
    // A tile that can hold a same-path pair has a loop of its own, so that the loop below stays, statement for statement,
    // the plain build's: the compiler contracts (1 + s) e and its like by what else uses the operands, and a shared body
    // gave the value rows of Matern-3/2 other last bits than the plain kernel's.  One row in flight: two hold the path
    // term's registers twice.
    if (mixed) {
#pragma unroll 1
      for (int r = 0; r < 8; ++r) {
        const int ir = rg + 8 * r;
        const int64_t row = i0 + ir;
        T s0 = (T)0, s1 = (T)0, p0 = (T)0, p1 = (T)0;  // r^2 and r_path^2 of the lane's two pairs
        for (int c = 0; c < d; ++c) {
          const T a = xa[ir * d + c];
          const T e0 = a - xb[c2 * d + c], e1 = a - xb[(c2 + 1) * d + c];
          s0 += e0 * e0;
          s1 += e1 * e1;
          p0 += sq[c] * (e0 * e0);
          p1 += sq[c] * (e1 * e1);
        }
        T v0, g0, v1, g1;
        cov::value_g<KERNEL>(s0, sf2, v0, g0);
        cov::value_g<KERNEL>(s1, sf2, v1, g1);
        const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
        T* out = V + row * ld + col0;
        const int ga = skb[ir];
        // One branch for the lane's two pairs, not one each: two divergent regions cost 8 - 20 VGPRs and an occupancy step
        // (compiler's resource report).  A pair of two paths keeps pv = pg = 0: -g e - 0 below.
        T pv0 = (T)0, pg0 = (T)0, pv1 = (T)0, pg1 = (T)0;
        const bool m0 = ga >= 0 && ga == skb[GT + c2], m1 = ga >= 0 && ga == skb[GT + c2 + 1];
        if (m0 || m1) {
          cov::value_g<KERNEL>(p0, sg2, pv0, pg0);
          cov::value_g<KERNEL>(p1, sg2, pv1, pg1);
          if (!m0) pv0 = pg0 = (T)0;
          if (!m1) pv1 = pg1 = (T)0;
        }
        if (with_value) {
          pair_t w = {ok0 ? v0 + pv0 : (T)0, ok1 ? v1 + pv1 : (T)0};
          __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out));
          out += blk;
        }
        for (int c = 0; c < d; ++c) {
          const T a = xa[ir * d + c];
          const T e0 = (a - xb[c2 * d + c]) * il[c], e1 = (a - xb[(c2 + 1) * d + c]) * il[c];
          pair_t w = {ok0 ? -g0 * e0 - pg0 * (sq[c] * e0) : (T)0, ok1 ? -g1 * e1 - pg1 * (sq[c] * e1) : (T)0};
          __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + c * blk));
        }
      }
      return;
    }
  }
#pragma unroll 2
  for (int r = 0; r < 8; ++r) {
    const int ir = rg + 8 * r;
    const int64_t row = i0 + ir;
    T s0 = (T)0, s1 = (T)0;
    for (int c = 0; c < d; ++c) {
      const T a = xa[ir * d + c];
      const T e0 = a - xb[c2 * d + c], e1 = a - xb[(c2 + 1) * d + c];
      s0 += e0 * e0;
      s1 += e1 * e1;
    }
    if constexpr (KINDS) {
      if (mixed) {
        const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
        T* out = V + row * ld + col0;
        T v0, g0, h0, v1, g1, h1;
        cov::value_gh<KERNEL>(s0, sf2, v0, g0, h0);
        cov::value_gh<KERNEL>(s1, sf2, v1, g1, h1);
        const int kb0 = skb[c2], kb1 = skb[c2 + 1];
        const int cb0 = kb0 < 0 ? 0 : kb0, cb1 = kb1 < 0 ? 0 : kb1;  // (kinds < d: the API checks)
        const T* pa = xa + ir * d;
        const T *pb0 = xb + c2 * d, *pb1 = pb0 + d;
        const T ub0 = pa[cb0] - pb0[cb0], ub1 = pa[cb1] - pb1[cb1], ilb0 = il[cb0], ilb1 = il[cb1];
        if (with_value) {
          pair_t w = {ok0 ? cov::element<T>(-1, kb0, v0, g0, h0, (T)0, ub0, (T)0, ilb0) : (T)0,
                      ok1 ? cov::element<T>(-1, kb1, v1, g1, h1, (T)0, ub1, (T)0, ilb1) : (T)0};
          __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out));
          out += blk;
        }
        for (int c = 0; c < d; ++c) {
          pair_t w = {ok0 ? cov::element<T>(c, kb0, v0, g0, h0, pa[c] - pb0[c], ub0, il[c], ilb0) : (T)0,
                      ok1 ? cov::element<T>(c, kb1, v1, g1, h1, pa[c] - pb1[c], ub1, il[c], ilb1) : (T)0};
          __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + c * blk));
        }
        continue;
      }
    }
    T v0, g0, v1, g1;
    cov::value_g<KERNEL>(s0, sf2, v0, g0);
    cov::value_g<KERNEL>(s1, sf2, v1, g1);
    const bool ok0 = row < m && col0 < n, ok1 = row < m && col1 < n;
    T* out = V + row * ld + col0;
    if (with_value) {
      pair_t w = {ok0 ? v0 : (T)0, ok1 ? v1 : (T)0};
      __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out));
      out += blk;
    }
    for (int c = 0; c < d; ++c) {
      const T a = xa[ir * d + c];
      const T e0 = (a - xb[c2 * d + c]) * il[c], e1 = (a - xb[(c2 + 1) * d + c]) * il[c];
      pair_t w = {ok0 ? -g0 * e0 : (T)0, ok1 ? -g1 * e1 : (T)0};
      __builtin_nontemporal_store(w, reinterpret_cast<pair_t*>(out + c * blk));
    }
  }
}

// Matrix-free mean gradient, partial over the training columns [s chunk, (s + 1) chunk) of split s = blockIdx.z:
//   part[((s k + c) d + j) ldp + i] = sum_n g(x*_i, x_n) (u*_ij - u_nj) alphaT[c][n]
// for the 64 query rows of blockIdx.x and the targets [KC blockIdx.y, KC blockIdx.y + KC) (kmatvec_kernel's
// structure: LDS-broadcast columns, each wave 16 of every 64, the four waves summed in a fixed order; no atomics).
// One exponential per pair serves all d partial derivatives and the KC targets of the workgroup.
template <typename T, int KERNEL, int D, int KC>
__global__ __launch_bounds__(256) void kgrad_matvec_kernel(const T* __restrict__ As, const T* __restrict__ Bs,
                                                          int64_t npad, int64_t chunk, int d_rt, T sf2,
                                                          const T* __restrict__ alphaT, int64_t lda, int k,
                                                          T* __restrict__ part, int64_t ldp) {
  constexpr int DD = D > 0 ? D : MAX_D;
  const int d = (D > 0) ? D : d_rt;
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
  T acc[KC][DD];
#pragma unroll
  for (int q = 0; q < KC; ++q)
#pragma unroll
    for (int c = 0; c < DD; ++c) acc[q][c] = (T)0;
  for (int64_t j0 = jbeg; j0 < jend; j0 += GT) {
    for (int e = tid; e < GT * d; e += 256) xb[e] = Bs[j0 * d + e];
    for (int e = tid; e < KC * GT; e += 256) {
      const int q = e >> 6;
      ab[e] = (cb + q < k) ? alphaT[(int64_t)(cb + q) * lda + j0 + (e & 63)] : (T)0;
    }
    __syncthreads();
    for (int jj = g * 16; jj < g * 16 + 16; ++jj) {
      T df[DD];
      T r2 = (T)0;
#pragma unroll
      for (int c = 0; c < DD; ++c)
        if (D > 0 || c < d) {
          df[c] = xa[c] - xb[jj * d + c];
          r2 += df[c] * df[c];
        }
      T v, gf;
      cov::value_g<KERNEL>(r2, sf2, v, gf);
#pragma unroll
      for (int q = 0; q < KC; ++q) {
        const T ga = gf * ab[q * GT + jj];
#pragma unroll
        for (int c = 0; c < DD; ++c)
          if (D > 0 || c < d) acc[q][c] += ga * df[c];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < KC; ++q)
#pragma unroll
    for (int c = 0; c < DD; ++c) {
      if (D == 0 && c >= d) continue;  // d is uniform: every wave skips the same barriers
      if (g > 0) red[(g - 1) * GT + lane] = acc[q][c];
      __syncthreads();
      if (g == 0 && cb + q < k) {
        const T v = ((acc[q][c] + red[lane]) + red[GT + lane]) + red[2 * GT + lane];
        part[(((int64_t)s * k + cb + q) * d + c) * ldp + i] = v;
      }
      __syncthreads();
    }
}

// dmean (M, d, k)[m][j][c] = -(sum over the S splits, in order, of part) / l_j
template <typename T>
__global__ __launch_bounds__(256) void kgrad_finish_kernel(const T* __restrict__ part, int64_t ldp, int S, int64_t M,
                                                          int d, int k, const double* __restrict__ ls, int n_ls,
                                                          T* __restrict__ out) {
  const int64_t total = M * d * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / ((int64_t)d * k);
    const int rem = (int)(e - m * d * k);
    const int j = rem / k, c = rem - j * k;
    T acc = (T)0;
    for (int q = 0; q < S; ++q) acc += part[(((int64_t)q * k + c) * d + j) * ldp + m];
    out[e] = -acc * (T)(1.0 / ls[n_ls == 1 ? 0 : j]);
  }
}

struct Priors {
  double p[PRIOR_SLOTS];
};

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + (red[2] + red[3]));
  __syncthreads();
  return s;
}

// one workgroup per valid row i of row block b = blockIdx.y:  out[b mp + i] = prior[b] - sum_j V[b mp + i][j]^2
// (fp64 accumulation, var_rows_kernel's fixed order).  ids != null: query point i with a path id >= 0 is a value of f + g_p,
// and its prior is pr[b] + pg[b], the sum formed in fp64 before the same subtraction.
template <typename T>
__global__ __launch_bounds__(256) void grad_norms_kernel(const T* __restrict__ V, int64_t ld, int64_t mp, int64_t ncols,
                                                        Priors pr, T* __restrict__ out,
                                                        const int32_t* __restrict__ ids = nullptr, Priors pg = {}) {
  typedef T pair_t __attribute__((ext_vector_type(2)));
  __shared__ double red[4];
  const int64_t r = (int64_t)blockIdx.y * mp + blockIdx.x;
  const T* row = V + r * ld;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t j = (int64_t)threadIdx.x * 2; j < ncols; j += 512) {
    const pair_t v = *reinterpret_cast<const pair_t*>(row + j);
    s0 += (double)v.x * (double)v.x;
    s1 += (double)v.y * (double)v.y;
  }
  const double s = block_sum(s0 + s1, red);
  if (threadIdx.x == 0) {
    const double prior = (ids && ids[blockIdx.x] >= 0) ? pr.p[blockIdx.y] + pg.p[blockIdx.y] : pr.p[blockIdx.y];
    out[r] = (T)(prior - s);
  }
}

// the permuting unpack of one batch: column b mp + i of MT (row c = target) and entry b mp + i of VN (norms) go to
//   b = 0 with a value block: mean[i k + c], var[i];   else j = b - off: dmean[(i d + j) k + c], dvar[i d + j]
template <typename T>
__global__ __launch_bounds__(256) void grad_unpack_kernel(const T* __restrict__ MT, int64_t ldm, const T* __restrict__ VN,
                                                         int64_t mp, int64_t mv, int nblk, int d, int k, int with_value,
                                                         T* __restrict__ mean, T* __restrict__ var,
                                                         T* __restrict__ dmean, T* __restrict__ dvar) {
  const int64_t total = mv * nblk * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / ((int64_t)nblk * k);
    const int rem = (int)(e - i * nblk * k);
    const int b = rem / k, c = rem - b * k;
    const int64_t col = (int64_t)b * mp + i;
    const T v = MT[(int64_t)c * ldm + col];
    if (with_value && b == 0) {
      if (mean) mean[i * k + c] = v;
      if (var && c == 0) var[i] = VN[col];
    } else {
      const int j = b - (with_value ? 1 : 0);
      dmean[(i * d + j) * k + c] = v;
      if (dvar && c == 0) dvar[i * d + j] = VN[col];
    }
  }
}

unsigned grid_for(int64_t work) {
  const int64_t b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

template <typename T, int KERNEL>
void build_d(const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d, double sf2,
             const double* ls, int n_ls, int with_value, T* V, int64_t ld, hipStream_t st, const int32_t* kcol,
             const int32_t* grow, const double* q, double sg2) {
  const int64_t tm = mpad / GT, tn = npad / GT;
  dim3 grid((unsigned)(tm * tn)), block(256);
  const T s = (T)sf2;
  const int tnn = (int)tn;
  if (grow) {  // rows and columns with path ids (kcol: the columns')
    const T sg = (T)sg2;
    switch (d) {
      case 1: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 1, false, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol, grow, q, sg); break;
      case 2: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 2, false, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol, grow, q, sg); break;
      case 3: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 3, false, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol, grow, q, sg); break;
      default: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 0, false, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol, grow, q, sg); break;
    }
    return;
  }
  if (kcol) {  // observations with kinds
    switch (d) {
      case 1: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 1, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol); break;
      case 2: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 2, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol); break;
      case 3: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 3, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol); break;
      default: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 0, true>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad, kcol); break;
    }
    return;
  }
  switch (d) {
    case 1: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 1>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad); break;
    case 2: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 2>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad); break;
    case 3: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 3>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad); break;
    default: hipLaunchKernelGGL((kgrad_build_kernel<T, KERNEL, 0>), grid, block, 0, st, As, m, Bs, n, d, tnn, s, ls, n_ls, with_value, V, ld, mpad); break;
  }
}

template <typename T, int KERNEL, int D, int KC>
void matvec_launch(dim3 grid, const T* As, const T* Bs, int64_t npad, int64_t chunk, int d, double sf2, const T* alphaT,
                   int64_t lda, int k, T* part, int64_t ldp, hipStream_t st) {
  hipLaunchKernelGGL((kgrad_matvec_kernel<T, KERNEL, D, KC>), grid, dim3(256), 0, st, As, Bs, npad, chunk, d, (T)sf2,
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

}  // namespace

template <typename T>
void launch_kgrad_build(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d,
                        double sf2, const double* ls, int n_ls, int with_value, T* V, int64_t ld, hipStream_t st,
                        const int32_t* kind_b) {
  cov::dispatch_differentiable(kernel, [&](auto fam) { build_d<T, fam>(As, m, mpad, Bs, n, npad, d, sf2, ls, n_ls, with_value, V, ld, st, kind_b, nullptr, nullptr, 0.0); });
}

template <typename T>
void launch_kgrad_build_g(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                          const int32_t* group_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                          const double* q, double sg2, int with_value, T* V, int64_t ld, hipStream_t st) {
  cov::dispatch_differentiable(kernel, [&](auto fam) { build_d<T, fam>(As, m, mpad, Bs, n, npad, d, sf2, ls, n_ls, with_value, V, ld, st, group_b, group_a, q, sg2); });
}

void kgrad_matvec_shape(int64_t M, int64_t npad, int d, int k, int* KC, int* S, int64_t* chunk) {
  const int kc = d > 3 ? 1 : (k == 1 ? 1 : k == 2 ? 2 : 4);
  const int64_t wgs = (round_up(M, GT) / GT) * ((k + kc - 1) / kc);
  // split the N contraction until the grid holds ~1024 workgroups (4 per CU), chunks of at least 1024 columns
  int64_t s = (1024 + wgs - 1) / wgs;
  s = std::max<int64_t>(1, std::min<int64_t>(s, npad / 1024));
  const int64_t ch = round_up((npad + s - 1) / s, GT);
  *KC = kc;
  *chunk = ch;
  *S = (int)((npad + ch - 1) / ch);
}

template <typename T>
void launch_kgrad_matvec(int kernel, const T* As, int64_t M, const T* Bs, int64_t npad, int d, double sf2,
                         const T* alphaT, int64_t lda, int k, const double* ls, int n_ls, T* part, T* dmean,
                         hipStream_t st) {
  int KC = 1, S = 1;
  int64_t chunk = npad;
  kgrad_matvec_shape(M, npad, d, k, &KC, &S, &chunk);
  const int64_t mpad = round_up(M, GT);
  const dim3 grid((unsigned)(mpad / GT), (unsigned)((k + KC - 1) / KC), (unsigned)S);
  cov::dispatch_differentiable(kernel, [&](auto fam) {
    matvec_d<T, fam>(grid, KC, As, Bs, npad, chunk, d, sf2, alphaT, lda, k, part, mpad, st);
    hipLaunchKernelGGL(kgrad_finish_kernel<T>, dim3(grid_for(M * d * k)), dim3(256), 0, st, part, mpad, S, M, d, k, ls,
                       n_ls, dmean);
  });
}

template <typename T>
void launch_grad_norms(const T* V, int64_t ld, int64_t mp, int64_t mv, int nblk, int64_t ncols, const double* prior,
                       T* out, hipStream_t st, const int32_t* ids, const double* prior_path) {
  if (mv <= 0 || nblk <= 0) return;
  Priors pr{}, pg{};
  for (int b = 0; b < nblk && b < PRIOR_SLOTS; ++b) pr.p[b] = prior[b];
  if (ids)
    for (int b = 0; b < nblk && b < PRIOR_SLOTS; ++b) pg.p[b] = prior_path[b];
  hipLaunchKernelGGL(grad_norms_kernel<T>, dim3((unsigned)mv, (unsigned)nblk), dim3(256), 0, st, V, ld, mp, ncols, pr,
                     out, ids, pg);
}

template <typename T>
void launch_grad_unpack(const T* MT, int64_t ldm, const T* VN, int64_t mp, int64_t mv, int nblk, int d, int k,
                        int with_value, T* mean, T* var, T* dmean, T* dvar, hipStream_t st) {
  if (mv <= 0) return;
  hipLaunchKernelGGL(grad_unpack_kernel<T>, dim3(grid_for(mv * nblk * k)), dim3(256), 0, st, MT, ldm, VN, mp, mv, nblk,
                     d, k, with_value, mean, var, dmean, dvar);
}

#define GPX_INSTANTIATE_DERIV(T)                                                                                       \
  template void launch_kgrad_build<T>(int, const T*, int64_t, int64_t, const T*, int64_t, int64_t, int, double,       \
                                      const double*, int, int, T*, int64_t, hipStream_t, const int32_t*);             \
  template void launch_kgrad_matvec<T>(int, const T*, int64_t, const T*, int64_t, int, double, const T*, int64_t, int, \
                                       const double*, int, T*, T*, hipStream_t);                                      \
  template void launch_kgrad_build_g<T>(int, const T*, const int32_t*, int64_t, int64_t, const T*, const int32_t*,    \
                                        int64_t, int64_t, int, double, const double*, int, const double*, double,    \
                                        int, T*, int64_t, hipStream_t);                                               \
  template void launch_grad_norms<T>(const T*, int64_t, int64_t, int64_t, int, int64_t, const double*, T*,            \
                                     hipStream_t, const int32_t*, const double*);                                     \
  template void launch_grad_unpack<T>(const T*, int64_t, const T*, int64_t, int64_t, int, int, int, int, T*, T*, T*,  \
                                      T*, hipStream_t);
GPX_INSTANTIATE_DERIV(double)
GPX_INSTANTIATE_DERIV(float)

}  // namespace gpx
