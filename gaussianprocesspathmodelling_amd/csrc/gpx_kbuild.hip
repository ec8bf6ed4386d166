// gpx_kbuild.hip — kernel-matrix builder (SURVEY.md §8 rows a1 "K1" and a2 "K1'").
//
// The reference has no kernel-matrix code; its nearest relative is the pairwise
// distance loop trajectories.calc_distance (GPmap.py:114-121).  Formula and
// operation order follow oracle/gp_oracle.py:kernel_matrix.
//
// HBM-write-bound: one 64x64 tile of K per 256-thread workgroup, input points staged
// once in LDS, each lane writes 16-byte (2 x f64) pieces so a half-wave covers 512
// contiguous bytes of one row.  Algorithmic traffic: 8 B per entry written, the
// points (N*d*8 B) read once per tile row/column from L2.
#include <climits>

#include "gpx_cov.h"
#include "gpx_internal.h"

namespace gpx {
namespace {

constexpr int KT = 64;      // tile edge

template <typename T>
__global__ __launch_bounds__(256) void scale_points_kernel(const T* __restrict__ X, int64_t n,
                                                          int64_t npad, int d,
                                                          const double* __restrict__ ls, int n_ls,
                                                          T* __restrict__ Xs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npad * d) return;
  const int64_t i = idx / d;
  const int c = (int)(idx - i * d);
  Xs[idx] = (i < n) ? X[idx] / (T)ls[n_ls == 1 ? 0 : c] : (T)0;
}

// linear index over the lower triangle (row-major) -> (ti, tj), tj <= ti
__device__ __forceinline__ void tri_coords(int64_t t, int& ti, int& tj) {
  int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = (int)i;
  tj = (int)(t - i * (i + 1) / 2);
}

// SYM: lower tiles of a square matrix built from one point set (As == Bs), diagonal
// gets + diag_add, padding becomes identity.  !SYM: all tiles, padding is zero.
// WEIGHTED (SYM only): row i < m of the diagonal gets + (wsn2 w[i] + wjit) instead of diag_add — per-observation noise;
// the sum is formed in fp64 and rounded once, as the host forms sn2 + jitter for the scalar form (w = 1: the same bits).
// KINDS: the columns (SYM: and the rows) are observations with a kind (gpx_cov.h: -1 a value, j a derivative along x_j);
// krow (null: all values) / kcol are readable up to the padded sizes and hold -1 there, ls (n_ls) are the lengthscales.
// The 64 + 64 kinds and 1 / l are staged beside the points.  A tile whose kinds are all -1 — decided once per workgroup,
// wave-uniform — takes the value-only path, whose numbers are those of the plain build; a mixed tile evaluates cov::element,
// still one exponential per pair.  SYM: w is the finished per-row diagonal term (launch_kinds_diag), read on diagonal tiles.
// GROUPS (never with KINDS): the observations carry path ids (-1: no path) and a same-path pair gets + sg2 k(., .; l_path),
// the within-path deviation of the hierarchical model.  The side channels are reused: krow / kcol are
// the row / column ids (readable up to the padded sizes, -1 there), ls (n_ls == d) holds q_c = (l_c / l_path,c)^2 and wsn2
// is sg2; SYM: w is the finished per-row diagonal term, as for KINDS.  The 64 + 64 ids and q are staged beside the points.
// Whether the tile can hold a same-path pair — the ranges of the non-negative row and column ids overlap — is decided once
// per workgroup, wave-uniform; a tile that cannot takes the value-only path, whose numbers are those of the plain build.
// Otherwise r_path^2 = sum_c q_c e_c^2 from the scaled differences e_c the loop forms anyway, and cov::value(r_path^2, sg2)
// is added where the ids match (SYM: the diagonal gets sg2 this way).
template <typename T, int KERNEL, bool SYM, int D, bool WEIGHTED = false, bool KINDS = false, bool GROUPS = false>
__global__ __launch_bounds__(256) void kbuild_kernel(const T* __restrict__ As, int64_t m,
                                                    const T* __restrict__ Bs, int64_t n, int d_rt,
                                                    int tiles_n, T sf2, T diag_add, T* __restrict__ K,
                                                    int64_t ld, const T* __restrict__ w = nullptr,
                                                    double wsn2 = 0.0, double wjit = 0.0,
                                                    const int32_t* __restrict__ krow = nullptr,
                                                    const int32_t* __restrict__ kcol = nullptr,
                                                    const double* __restrict__ ls = nullptr, int n_ls = 0) {
  const int d = (D > 0) ? D : d_rt;
  // LDS sized by the instantiation (d = 3: 2 x 1.5 KB, not 2 x 16 KB): the occupancy is then the waves', not the LDS's
  __shared__ T xa[KT * (D > 0 ? D : MAX_D)];
  __shared__ T xb[KT * (D > 0 ? D : MAX_D)];
  int ti, tj;
  if (SYM) {
    tri_coords((int64_t)blockIdx.x, ti, tj);
  } else {
    ti = (int)(blockIdx.x / tiles_n);
    tj = (int)(blockIdx.x - (int64_t)ti * tiles_n);
  }
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  const int tid = threadIdx.x;
  for (int e = tid; e < KT * d; e += 256) {
    xa[e] = As[i0 * d + e];  // rows of the padded point array are always readable
    xb[e] = Bs[j0 * d + e];
  }
  bool mixed = false;
  const int* ska = nullptr;
  const int* skb = nullptr;
  const T* sil = nullptr;
  if constexpr (KINDS) {
    __shared__ int kab[2 * KT];
    __shared__ T ilv[D > 0 ? D : MAX_D];
    int deriv = 0;
    if (tid < 2 * KT) {
      const int kk = tid < KT ? (krow ? krow[i0 + tid] : -1) : kcol[j0 + tid - KT];
      kab[tid] = kk;
      deriv = kk >= 0;
    } else if (tid - 2 * KT < d) {
      ilv[tid - 2 * KT] = (T)(1.0 / ls[n_ls == 1 ? 0 : tid - 2 * KT]);
    }
    mixed = __syncthreads_or(deriv) != 0;
    ska = kab, skb = kab + KT, sil = ilv;
  } else if constexpr (GROUPS) {
    static_assert(!WEIGHTED, "the GROUPS build takes its diagonal from the finished per-row vector");
    __shared__ int gab[2 * KT];
    __shared__ int rng[4];  // lowest / highest non-negative id of the rows, of the columns
    __shared__ T qv[D > 0 ? D : MAX_D];
    if (tid < 2 * KT) {  // wave 0: the rows, wave 1: the columns
      const int id = tid < KT ? krow[i0 + tid] : kcol[j0 + tid - KT];
      gab[tid] = id;
      int lo = id >= 0 ? id : INT_MAX, hi = id;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
      }
      if ((tid & 63) == 0) rng[2 * (tid >> 6)] = lo, rng[2 * (tid >> 6) + 1] = hi;
    } else if (tid - 2 * KT < d) {
      qv[tid - 2 * KT] = (T)ls[tid - 2 * KT];
    }
    __syncthreads();
    mixed = rng[0] <= rng[3] && rng[2] <= rng[1];  // (no id >= 0 on a side: lo = INT_MAX, hi < 0)
    ska = gab, skb = gab + KT, sil = qv;
  } else {
    __syncthreads();
  }
  const int c2 = (tid & 31) * 2;
  const int rg = tid >> 5;
  T bj0[D > 0 ? D : MAX_D], bj1[D > 0 ? D : MAX_D];
  if (D > 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      bj0[c] = xb[c2 * D + c];
      bj1[c] = xb[(c2 + 1) * D + c];
    }
  }
  const int64_t col0 = j0 + c2, col1 = col0 + 1;
#pragma unroll 2
  for (int r = 0; r < 8; ++r) {
    const int il = rg + 8 * r;
    const int64_t row = i0 + il;
    T s0 = (T)0, s1 = (T)0;
    [[maybe_unused]] T p0 = (T)0, p1 = (T)0;  // GROUPS, on a tile that can hold a same-path pair: r_path^2
    if (D > 0) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const T a = xa[il * D + c];
        const T e0 = a - bj0[c], e1 = a - bj1[c];
        s0 += e0 * e0;
        s1 += e1 * e1;
        if constexpr (GROUPS) {
          if (mixed) p0 += sil[c] * (e0 * e0), p1 += sil[c] * (e1 * e1);
        }
      }
    } else {
      for (int c = 0; c < d; ++c) {
        const T a = xa[il * d + c];
        const T e0 = a - xb[c2 * d + c], e1 = a - xb[(c2 + 1) * d + c];
        s0 += e0 * e0;
        s1 += e1 * e1;
        if constexpr (GROUPS) {
          if (mixed) p0 += sil[c] * (e0 * e0), p1 += sil[c] * (e1 * e1);
        }
      }
    }
    T v0, v1;
    if constexpr (KINDS) {
      if (mixed) {
        T g0, h0, g1, h1;
        cov::value_gh<KERNEL>(s0, sf2, v0, g0, h0);
        cov::value_gh<KERNEL>(s1, sf2, v1, g1, h1);
        const int ka = ska[il], kb0 = skb[c2], kb1 = skb[c2 + 1];
        const int ca = ka < 0 ? 0 : ka, cb0 = kb0 < 0 ? 0 : kb0, cb1 = kb1 < 0 ? 0 : kb1;  // (kinds < d: the API checks)
        const T* pa = xa + il * d;
        const T *pb0 = xb + c2 * d, *pb1 = pb0 + d;
        v0 = cov::element<T>(ka, kb0, v0, g0, h0, pa[ca] - pb0[ca], pa[cb0] - pb0[cb0], sil[ca], sil[cb0]);
        v1 = cov::element<T>(ka, kb1, v1, g1, h1, pa[ca] - pb1[ca], pa[cb1] - pb1[cb1], sil[ca], sil[cb1]);
      } else {
        v0 = cov::value<KERNEL>(s0, sf2), v1 = cov::value<KERNEL>(s1, sf2);
      }
    } else {
      v0 = cov::value<KERNEL>(s0, sf2), v1 = cov::value<KERNEL>(s1, sf2);
      if constexpr (GROUPS) {
        if (mixed) {
          const int ga = ska[il];
          if (ga >= 0 && ga == skb[c2]) v0 += cov::value<KERNEL>(p0, (T)wsn2);
          if (ga >= 0 && ga == skb[c2 + 1]) v1 += cov::value<KERNEL>(p1, (T)wsn2);
        }
      }
    }
    if (SYM) {
      if (KINDS || GROUPS) {  // the finished diagonal term of row `row` (only diagonal tiles read it)
        if (ti == tj && row < m) {
          const T da = w[row];
          if (row == col0) v0 += da;
          if (row == col1) v1 += da;
        }
      } else if (WEIGHTED) {  // (only diagonal tiles read w: one load per row there)
        if (ti == tj && row < m) {
          const T da = (T)(wsn2 * (double)w[row] + wjit);
          if (row == col0) v0 += da;
          if (row == col1) v1 += da;
        }
      } else {
        if (row == col0) v0 += diag_add;
        if (row == col1) v1 += diag_add;
      }
      if (row >= m || col0 >= n) v0 = (row == col0) ? (T)1 : (T)0;
      if (row >= m || col1 >= n) v1 = (row == col1) ? (T)1 : (T)0;
    } else {
      if (row >= m || col0 >= n) v0 = (T)0;
      if (row >= m || col1 >= n) v1 = (T)0;
    }
    typedef T pair_t __attribute__((ext_vector_type(2)));
    pair_t out = {v0, v1};
    // Non-temporal 16-byte stores: nothing re-reads a tile before the whole matrix (17 GB) has gone by.  Round 4,
    // tools/kbuild_variants.hip, twelve variants side by side in one process at N = 65536 (profiles/r04_kbuild_variants.txt):
    // this kernel 3.36 ms = 5.1 TB/s against 3.52 with plain stores and 3.58 with the 2 x 16 KB static LDS of rounds 1-3;
    // unrolling (1 / 2 / 4 / 8 rows), persistent tile walks, row strips and an occupancy hint all land within 3.4-3.9 ms.
    __builtin_nontemporal_store(out, reinterpret_cast<pair_t*>(K + row * ld + col0));
  }
}

// the weighted symmetric build (launch_kbuild_sym_w)
template <typename T, int KERNEL>
void dispatch_d_w(const T* Xs, int64_t n, int d, int64_t nblocks, int tiles_n, double sf2, const T* w, double sn2,
                  double jitter, T* K, int64_t ld, hipStream_t st) {
  dim3 grid((unsigned)nblocks), block(256);
  const T s = (T)sf2, z = (T)0;
  switch (d) {
    case 1: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, true, 1, true>), grid, block, 0, st, Xs, n, Xs, n, d, tiles_n, s, z, K, ld, w, sn2, jitter); break;
    case 2: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, true, 2, true>), grid, block, 0, st, Xs, n, Xs, n, d, tiles_n, s, z, K, ld, w, sn2, jitter); break;
    case 3: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, true, 3, true>), grid, block, 0, st, Xs, n, Xs, n, d, tiles_n, s, z, K, ld, w, sn2, jitter); break;
    default: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, true, 0, true>), grid, block, 0, st, Xs, n, Xs, n, d, tiles_n, s, z, K, ld, w, sn2, jitter); break;
  }
}

// the builds over observations with kinds (launch_kbuild_sym_k / launch_kbuild_cross_k)
template <typename T, int KERNEL, bool SYM>
void dispatch_d_k(const T* As, int64_t m, const T* Bs, int64_t n, int d, int64_t nblocks, int tiles_n, double sf2,
                  const int32_t* krow, const int32_t* kcol, const double* ls, int n_ls, const T* diag, T* K, int64_t ld,
                  hipStream_t st) {
  dim3 grid((unsigned)nblocks), block(256);
  const T s = (T)sf2, z = (T)0;
  switch (d) {
    case 1: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 1, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, 0.0, 0.0, krow, kcol, ls, n_ls); break;
    case 2: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 2, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, 0.0, 0.0, krow, kcol, ls, n_ls); break;
    case 3: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 3, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, 0.0, 0.0, krow, kcol, ls, n_ls); break;
    default: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 0, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, 0.0, 0.0, krow, kcol, ls, n_ls); break;
  }
}

// the builds over observations with path ids (launch_kbuild_sym_g / launch_kbuild_cross_g)
template <typename T, int KERNEL, bool SYM>
void dispatch_d_g(const T* As, int64_t m, const T* Bs, int64_t n, int d, int64_t nblocks, int tiles_n, double sf2,
                  const int32_t* grow, const int32_t* gcol, const double* q, double sg2, const T* diag, T* K, int64_t ld,
                  hipStream_t st) {
  dim3 grid((unsigned)nblocks), block(256);
  const T s = (T)sf2, z = (T)0;
  switch (d) {
    case 1: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 1, false, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, sg2, 0.0, grow, gcol, q, d); break;
    case 2: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 2, false, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, sg2, 0.0, grow, gcol, q, d); break;
    case 3: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 3, false, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, sg2, 0.0, grow, gcol, q, d); break;
    default: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 0, false, false, true>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, z, K, ld, diag, sg2, 0.0, grow, gcol, q, d); break;
  }
}

// diag[i] = (kind[i] < 0 ? sn2 : sn2_deriv) (w ? w[i] : 1) + jitter, i < n: formed in fp64 and rounded once
template <typename T>
__global__ __launch_bounds__(256) void kinds_diag_kernel(const int32_t* __restrict__ kind, const T* __restrict__ w,
                                                        int64_t n, double sn2, double sn2_deriv, double jitter,
                                                        T* __restrict__ diag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  diag[i] = (T)((kind[i] < 0 ? sn2 : sn2_deriv) * (w ? (double)w[i] : 1.0) + jitter);
}

template <typename T, int KERNEL, bool SYM>
void dispatch_d(const T* As, int64_t m, const T* Bs, int64_t n, int d, int64_t nblocks, int tiles_n,
                double sf2, double diag_add, T* K, int64_t ld, hipStream_t st) {
  dim3 grid((unsigned)nblocks), block(256);
  const T s = (T)sf2, da = (T)diag_add;
  switch (d) {
    case 1: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 1>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, da, K, ld); break;
    case 2: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 2>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, da, K, ld); break;
    case 3: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 3>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, da, K, ld); break;
    default: hipLaunchKernelGGL((kbuild_kernel<T, KERNEL, SYM, 0>), grid, block, 0, st, As, m, Bs, n, d, tiles_n, s, da, K, ld); break;
  }
}

}  // namespace

template <typename T>
void launch_scale_points(const T* X, int64_t n, int64_t npad, int d, const double* ls, int n_ls, T* Xs,
                         hipStream_t st) {
  const int64_t total = npad * d;
  hipLaunchKernelGGL(scale_points_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X,
                     n, npad, d, ls, n_ls, Xs);
}

template <typename T>
void launch_kbuild_sym(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2,
                       double diag_add, T* K, int64_t ld, hipStream_t st) {
  const int64_t TT = npad / KT;
  const int64_t nblocks = TT * (TT + 1) / 2;
  cov::dispatch(kernel, [&](auto fam) { dispatch_d<T, fam, true>(Xs, n, Xs, n, d, nblocks, (int)TT, sf2, diag_add, K, ld, st); });
}

template <typename T>
void launch_kbuild_sym_w(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const T* w, double sn2,
                         double jitter, T* K, int64_t ld, hipStream_t st) {
  const int64_t TT = npad / KT;
  const int64_t nblocks = TT * (TT + 1) / 2;
  cov::dispatch(kernel, [&](auto fam) { dispatch_d_w<T, fam>(Xs, n, d, nblocks, (int)TT, sf2, w, sn2, jitter, K, ld, st); });
}

template <typename T>
void launch_kbuild_cross(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n,
                         int64_t npad, int d, double sf2, T* K, int64_t ld, hipStream_t st) {
  const int64_t tm = mpad / KT, tn = npad / KT;
  cov::dispatch(kernel, [&](auto fam) { dispatch_d<T, fam, false>(As, m, Bs, n, d, tm * tn, (int)tn, sf2, 0.0, K, ld, st); });
}

template <typename T>
void launch_kinds_diag(const int32_t* kind, const T* w, int64_t n, double sn2, double sn2_deriv, double jitter, T* diag,
                       hipStream_t st) {
  hipLaunchKernelGGL(kinds_diag_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kind, w, n, sn2, sn2_deriv,
                     jitter, diag);
}

template <typename T>
void launch_kbuild_sym_k(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const int32_t* kind,
                         const double* ls, int n_ls, const T* diag, T* K, int64_t ld, hipStream_t st) {
  const int64_t TT = npad / KT;
  const int64_t nblocks = TT * (TT + 1) / 2;
  cov::dispatch_differentiable(kernel, [&](auto fam) {
    dispatch_d_k<T, fam, true>(Xs, n, Xs, n, d, nblocks, (int)TT, sf2, kind, kind, ls, n_ls, diag, K, ld, st);
  });
}

template <typename T>
void launch_kbuild_cross_k(int kernel, const T* As, int64_t m, int64_t mpad, const T* Bs, int64_t n, int64_t npad, int d,
                           double sf2, const int32_t* kind_b, const double* ls, int n_ls, T* K, int64_t ld, hipStream_t st) {
  const int64_t tm = mpad / KT, tn = npad / KT;
  cov::dispatch_differentiable(kernel, [&](auto fam) {
    dispatch_d_k<T, fam, false>(As, m, Bs, n, d, tm * tn, (int)tn, sf2, nullptr, kind_b, ls, n_ls, nullptr, K, ld, st);
  });
}

// as launch_kbuild_cross_k with kinds on the rows too (kind_a: readable up to mpad, -1 beyond m): the left part of appended
// rows, whose new observations may be derivatives
template <typename T>
void launch_kbuild_cross_kk(int kernel, const T* As, const int32_t* kind_a, int64_t m, int64_t mpad, const T* Bs,
                            const int32_t* kind_b, int64_t n, int64_t npad, int d, double sf2, const double* ls, int n_ls,
                            T* K, int64_t ld, hipStream_t st) {
  const int64_t tm = mpad / KT, tn = npad / KT;
  cov::dispatch_differentiable(kernel, [&](auto fam) {
    dispatch_d_k<T, fam, false>(As, m, Bs, n, d, tm * tn, (int)tn, sf2, kind_a, kind_b, ls, n_ls, nullptr, K, ld, st);
  });
}

template <typename T>
void launch_kbuild_sym_g(int kernel, const T* Xs, int64_t n, int64_t npad, int d, double sf2, const int32_t* group,
                         const double* q, double sg2, const T* diag, T* K, int64_t ld, hipStream_t st) {
  const int64_t TT = npad / KT;
  const int64_t nblocks = TT * (TT + 1) / 2;
  cov::dispatch(kernel, [&](auto fam) {
    dispatch_d_g<T, fam, true>(Xs, n, Xs, n, d, nblocks, (int)TT, sf2, group, group, q, sg2, diag, K, ld, st);
  });
}

template <typename T>
void launch_kbuild_cross_g(int kernel, const T* As, const int32_t* group_a, int64_t m, int64_t mpad, const T* Bs,
                           const int32_t* group_b, int64_t n, int64_t npad, int d, double sf2, const double* q, double sg2,
                           T* K, int64_t ld, hipStream_t st) {
  const int64_t tm = mpad / KT, tn = npad / KT;
  cov::dispatch(kernel, [&](auto fam) {
    dispatch_d_g<T, fam, false>(As, m, Bs, n, d, tm * tn, (int)tn, sf2, group_a, group_b, q, sg2, nullptr, K, ld, st);
  });
}

#define GPX_INSTANTIATE_KBUILD(T)                                                                     \
  template void launch_scale_points<T>(const T*, int64_t, int64_t, int, const double*, int, T*,       \
                                       hipStream_t);                                                  \
  template void launch_kbuild_sym<T>(int, const T*, int64_t, int64_t, int, double, double, T*,        \
                                     int64_t, hipStream_t);                                           \
  template void launch_kbuild_sym_w<T>(int, const T*, int64_t, int64_t, int, double, const T*, double, double, T*, \
                                       int64_t, hipStream_t);                                         \
  template void launch_kbuild_cross<T>(int, const T*, int64_t, int64_t, const T*, int64_t, int64_t,   \
                                       int, double, T*, int64_t, hipStream_t);                        \
  template void launch_kinds_diag<T>(const int32_t*, const T*, int64_t, double, double, double, T*, hipStream_t); \
  template void launch_kbuild_sym_k<T>(int, const T*, int64_t, int64_t, int, double, const int32_t*, const double*, int, \
                                       const T*, T*, int64_t, hipStream_t);                           \
  template void launch_kbuild_sym_g<T>(int, const T*, int64_t, int64_t, int, double, const int32_t*, const double*, double, \
                                       const T*, T*, int64_t, hipStream_t);                           \
  template void launch_kbuild_cross_g<T>(int, const T*, const int32_t*, int64_t, int64_t, const T*, const int32_t*, int64_t, \
                                         int64_t, int, double, const double*, double, T*, int64_t, hipStream_t); \
  template void launch_kbuild_cross_k<T>(int, const T*, int64_t, int64_t, const T*, int64_t, int64_t, int, double, \
                                         const int32_t*, const double*, int, T*, int64_t, hipStream_t); \
  template void launch_kbuild_cross_kk<T>(int, const T*, const int32_t*, int64_t, int64_t, const T*, const int32_t*, \
                                          int64_t, int64_t, int, double, const double*, int, T*, int64_t, hipStream_t);
GPX_INSTANTIATE_KBUILD(double)
GPX_INSTANTIATE_KBUILD(float)

}  // namespace gpx
