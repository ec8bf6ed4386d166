// gpx_grad.hip — analytic gradient of the log marginal likelihood w.r.t. the log
// hyper-parameters ("hyper-parameter gradient hooks"; the reference has
// no counterpart — GPmap.py contains no GP code).  Restated on the CPU by
// oracle/gp_oracle.py:OracleGP.lml_gradient (R&W eq. 5.9):
//
//     dLML/dlog(theta) = 1/2 sum_ij (sum_c alpha_ic alpha_jc - k K^-1_ij) (dK/dlog theta)_ij
//
//   dK/dlog l_c  = kd_ij * ((x_ic - x_jc) / l_c)^2   (kd of the family: gpx_cov.h)
//   dK/dlog sf2  = Kf_ij = sf2 k(r_ij)
//   dK/dlog sn2  = sn2 delta_ij
//
// K^-1 is never stored.  With ZT = L^-T (upper triangular, built from the factor already held
// by a forward substitution on the identity that skips the structural zeros: N^3/3 flops),
// K^-1 = ZT ZT^T is an NT product on the MFMA tile engine whose k-range starts at the tile's
// first row (another N^3/3), and each 128x128 tile of it is consumed in the epilogue of the
// very workgroup that produced it: the dK/dtheta tile is regenerated from the scaled points
// (as the kernel build does), multiplied in, reduced over the workgroup and written as one
// partial sum per (tile, theta).  The alpha alpha^T term is a separate O(N^2 k) pass of the
// same epilogue over 64x64 tiles.  Partials are summed in a fixed order: deterministic.
//
// Fits with derivative observations (KINDS instantiations of both kernels; gpx_lml_grad_full): an element of K of kinds
// (ka, kb) is cov::element and its d / dlog l_c is A u_c^2 + (delta(ka, c) + delta(kb, c)) B (cov::element_dl, the table in
// gpx_cov.h).  W A stays in the accumulators for the per-dimension pass exactly as W kd does; W B is summed per row (the
// rows of kind >= 0) and per column of the thread's elements and goes to the dimension that row's / column's kind names.
// theta = (lengthscales..., sf2, sn2, sn2_deriv): the diagonal sum is split by the row's kind.
//
// Fits with path ids (GROUPS instantiations of both kernels; gpx_lml_grad_paths): K = sf2 k(r) + m sg2 k(r_p)
// + diag with m_ij = [id_i == id_j >= 0] and r_p^2 = sum_c q_c e_c^2 (gpx_cov.h: path_dtheta).  The path term does not depend
// on l (q_c e_c^2 = ((x_ic - x_jc) / l_path,c)^2), so the entries of l, sf2 (the f part alone) and sn2 are the plain ones;
// theta = (lengthscales..., sf2, sn2, sg2, l_path...) gets  dK/dlog sg2 = m sg2 k(r_p),  dK/dlog l_path,c = m kd(r_p; sg2) q_c e_c^2.
// The accumulators have no room for a second retained set, so the path passes run FIRST, while the accumulators still hold
// W: one pass for sg2 (and the single l_path), then one per path dimension with r_p and kd recomputed per element — only
// in tiles that can hold a same-path pair (the ranges of the non-negative row and column ids overlap: workgroup-uniform, as
// kbuild_kernel's), the others write exact zeros and evaluate no extra exponential.
#include <climits>

#include "gpx_cov.h"
#include "gpx_internal.h"
#include "gpx_tile.h"

namespace gpx {
namespace {

// sum over the 256 threads of a workgroup, every thread gets the result (fixed order)
__device__ __forceinline__ double wg_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red[] may still be read from the previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- fused K^-1 tile + trace epilogue -------------------------------------------------------
// grid: the hole-free triangular super-tile map of the SYRK (tile_coords<true>), 128x128 tiles.
// part[lin * ntheta + t], t = (lengthscales..., sf2, sn2): sum over the tile of
// K^-1_ij (dK/dlog theta_t)_ij, off-diagonal tiles counted twice (symmetry).
// WEIGHTED: per-observation noise, dK/dlog sn2 = sn2 diag(wv) — the noise entry sums wv[i] K^-1_ii.  An instantiation of
// its own: the epilogue sits at the edge of the register file (see the scheduling barrier below), and one more load in it
// changes what the unweighted kernel spills.
// KINDS: the fit has derivative observations — kind (readable up to npad, -1 there), ls (n_ls) and sn2_deriv are read, wv
// may be null (WEIGHTED is not used), ntheta = n_ls + 3.  Instantiations of their own for the same reason.
// GROUPS (never with KINDS or WEIGHTED): the fit has path ids — the side channels are reused as kbuild_kernel's are: kind
// holds the ids (readable up to npad, -1 there), ls the d entries of q, n_ls is n_ls_path (1 or d) and sn2_deriv is sg2; wv
// may be null.  part[..] = (l_0.., sf2, sn2, sg2, l_path,0..), ntheta = (ard ? d : 1) + 3 + n_ls_path.
template <int KERNEL, int D, bool WEIGHTED, bool KINDS = false, bool GROUPS = false>
__global__ __launch_bounds__(256, 2) void kinv_trace_kernel(const double* __restrict__ ZT, int64_t ld,
                                                            int tiles, int64_t npad, int64_t n,
                                                            const double* __restrict__ Xs, int d_rt, int ard,
                                                            double sf2, double sn2, double* __restrict__ part,
                                                            int ntheta, int64_t nslots, int P, int rank,
                                                            int dc_nb, int dc_P, int dc_r, int64_t dc_cols, int dc_snake,
                                                            const double* __restrict__ wv,
                                                            const int32_t* __restrict__ kind = nullptr,
                                                            const double* __restrict__ ls = nullptr, int n_ls = 0,
                                                            double sn2_deriv = 0.0) {
  constexpr int BT = 128;
  __shared__ __attribute__((aligned(16))) double smem[TileShapeG<double, BT, BT>::SMEM_ELEMS];
  __shared__ double red[4];
  const int d = (D > 0) ? D : d_rt;
  // Tile (ti, tj) costs (tiles - ti) k-ranges, so handing each XCD one contiguous eighth of the
  // tile order (xcd_chunk_id, right for the uniform SYRK) gives the first XCD 29 % of the work
  // and the kernel ran at 31.6 TF.  Deal whole 64-slot groups (one super-tile: what an XCD runs
  // concurrently, so the L2 sharing inside a group is kept) round-robin over the XCDs instead:
  // neighbouring groups cost about the same, and the heavy ones still come first.
  // Sharded call (P ranks, each holding the whole L^-T): whole octets of groups — one group per
  // XCD — are dealt round-robin over the ranks, so every rank keeps all eight XCDs busy and its
  // share of heavy and light tiles; rank r launches only its own octets.
  const int64_t b = blockIdx.x, xl = b >> 3;
  const int64_t lin = ((((xl >> 6) * P + rank) << 3) + (b & 7)) * 64 + (xl & 63);
  int ti, tj;
  if (lin >= nslots || !tile_coords<true>(lin, tiles, tiles, 8, 0, BcMask{0, 1, 0}, ti, tj)) return;
  Num<double>::v4 acc[4][4];
  zero_acc(acc);
  // rows ti, tj of ZT are zero left of column ti*BT (tj <= ti): start the contraction there.
  // Distributed-column mode (dc_P > 0; the factor is only held distributed): this rank holds the
  // columns of L^-T that belong to ITS row blocks of L (height dc_nb, its block number lb — Deal.global(dc_r, lb) —
  // at local column lb dc_nb) for ALL rows, and contributes the part of the contraction over those
  // columns; the first own block that is not left of the tile's rows starts it.  The partial sums of
  // the ranks add up to the trace (one all-reduce of ntheta numbers).
  int64_t koff = (int64_t)ti * BT, klen = npad - koff;
  if (dc_P > 0) {
    const int64_t gi = koff / dc_nb;                                        // block of the tile's first row
    const int64_t before = Deal{dc_P, dc_snake}.upto(gi - 1, dc_r);         // own blocks with index < gi
    koff = before * dc_nb;
    klen = dc_cols - koff;
    if (klen <= 0) return;  // nothing of this tile lives here (its slot of `part` was zeroed)
  }
  gemm_tile_g<double, BT, BT>(ZT + (int64_t)ti * BT * ld + koff, ld, ZT + (int64_t)tj * BT * ld + koff, ld,
                              (int)klen, acc, smem);
  // gemm_tile_g ends with a barrier: the staging buffers are free -> scaled points of the
  // tile's rows and columns
  double* xa = smem;
  double* xb = smem + BT * MAX_D;
  const int tid = threadIdx.x;
  for (int e = tid; e < BT * d; e += 256) {
    xa[e] = Xs[(int64_t)ti * BT * d + e];
    xb[e] = Xs[(int64_t)tj * BT * d + e];
  }
  const int* ska = nullptr;
  const int* skb = nullptr;
  const double* sil = nullptr;
  [[maybe_unused]] const int* srng = nullptr;
  if constexpr (KINDS) {  // the tile's row and column kinds and 1 / l, beside the points
    __shared__ int kab[2 * BT];
    __shared__ double ilv[MAX_D];
    kab[tid] = kind[(tid < BT ? (int64_t)ti * BT : (int64_t)tj * BT - BT) + tid];
    if (tid < d) ilv[tid] = 1.0 / ls[n_ls == 1 ? 0 : tid];
    ska = kab, skb = kab + BT, sil = ilv;
  }
  if constexpr (GROUPS) {  // the tile's row and column ids and q, beside the points; the id ranges of the two sides
    static_assert(!KINDS && !WEIGHTED, "a fit has path ids or kinds, and the GROUPS instantiation reads wv when it is set");
    __shared__ int gab[2 * BT];
    __shared__ int rng[8];  // per wave (0, 1: the rows, 2, 3: the columns) the lowest / highest non-negative id
    __shared__ double qv[MAX_D];
    const int id = kind[(tid < BT ? (int64_t)ti * BT : (int64_t)tj * BT - BT) + tid];
    gab[tid] = id;
    int lo = id >= 0 ? id : INT_MAX, hi = id;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    if ((tid & 63) == 0) rng[2 * (tid >> 6)] = lo, rng[2 * (tid >> 6) + 1] = hi;
    if (tid < d) qv[tid] = ls[tid];
    ska = gab, skb = gab + BT, sil = qv, srng = rng;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
  if constexpr (GROUPS) {  // the path entries, while the accumulators hold W (the loop below overwrites them)
    const int nlp = n_ls;
    double* outp = part + lin * ntheta + (ntheta - nlp - 1);  // (sg2, l_path...)
    const double wp = (ti == tj) ? 1.0 : 2.0;
    // The noise entry first, and here rather than in the loop below: its load of wv is what makes the WEIGHTED loop spill
    // half as much again as the plain one, and every scratch access of that loop is a round trip to memory (measured:
    // the trace pass of this instantiation ran 8 % behind the plain one at d = 3 with the entry formed there).  Only a
    // diagonal tile holds diagonal elements, at il == jl.
    double sdiag = 0.0;
    if (ti == tj) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int il = wr * 64 + m * 16 + l4 + 4 * r;
          const int64_t gi = (int64_t)ti * BT + il;
#pragma unroll
          for (int nn = 0; nn < 4; ++nn)
            if (il == wc * 64 + nn * 16 + l15 && gi < n) sdiag += wv ? acc[m][nn][r] * wv[gi] : acc[m][nn][r];
        }
      sdiag = wg_sum(sdiag, red);
    }
    if (tid == 0) outp[-1] = sdiag * sn2;
    // can the tile hold a same-path pair?  (no id >= 0 on a side: lo = INT_MAX, hi < 0)
    const bool mixed = min(srng[0], srng[2]) <= max(srng[5], srng[7]) && min(srng[4], srng[6]) <= max(srng[1], srng[3]);
    if (!mixed) {
      if (tid <= nlp) outp[tid] = 0.0;
    } else {
      // pass 0: sg2 and, with one l_path, its entry (the sum over the dimensions); pass 1 + c: l_path,c
      for (int pass = 0; pass <= (nlp > 1 ? d : 0); ++pass) {
        double s = 0.0, s1 = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int il = wr * 64 + m * 16 + l4 + 4 * r;
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) {
              const int jl = wc * 64 + nn * 16 + l15;
              double pv, pdl;  // (padded rows and columns have id -1: no pair)
              if (cov::path_dtheta<KERNEL>(ska[il], skb[jl], xa + il * d, xb + jl * d, sil, d, sn2_deriv, pass - 1, pv, pdl)) {
                s += acc[m][nn][r] * (pass == 0 ? pv : pdl);
                s1 += acc[m][nn][r] * pdl;
              }
              __builtin_amdgcn_sched_barrier(0);  // (as below)
            }
          }
        s = wg_sum(s, red);
        if (pass == 0) {
          if (nlp == 1) s1 = wg_sum(s1, red);
          if (tid == 0) {
            outp[0] = wp * s;
            if (nlp == 1) outp[1] = wp * s1;
          }
        } else if (tid == 0) {
          outp[pass] = wp * s;
        }
      }
    }
  }
  double Sf = 0.0, Sn = 0.0, Sl = 0.0;
  // KINDS: the diagonal sum of the derivative rows, and W B summed over the thread's elements of a row / of a column
  [[maybe_unused]] double Sd = 0.0, RB[4][4] = {}, CB[4] = {};
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int il = wr * 64 + m * 16 + l4 + 4 * r;
      const int64_t gi = (int64_t)ti * BT + il;
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) {
        const int jl = wc * 64 + nn * 16 + l15;
        const int64_t gj = (int64_t)tj * BT + jl;
        double r2 = 0.0;
        if (D > 0) {
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const double e = xa[il * D + c] - xb[jl * D + c];
            r2 += e * e;
          }
        } else {
          for (int c = 0; c < d; ++c) {
            const double e = xa[il * d + c] - xb[jl * d + c];
            r2 += e * e;
          }
        }
        double v = acc[m][nn][r];
        if (gi >= n || gj >= n) v = 0.0;  // padded rows / columns are not part of K
        if constexpr (KINDS) {
          if constexpr (cov::differentiable(KERNEL)) {
            double kf, g, h, p, A, B;
            cov::value_ghp<KERNEL>(r2, sf2, kf, g, h, p);
            const int ka = ska[il], kb = skb[jl];
            const int ca = ka < 0 ? 0 : ka, cb = kb < 0 ? 0 : kb;  // (kinds < d: the fit checked)
            const double ua = xa[il * d + ca] - xb[jl * d + ca], ub = xa[il * d + cb] - xb[jl * d + cb];
            Sf += v * cov::element<double>(ka, kb, kf, g, h, ua, ub, sil[ca], sil[cb]);
            if (gi == gj && gi < n) {
              const double vw = wv ? v * wv[gi] : v;
              if (ka < 0) Sn += vw;
              else Sd += vw;
            }
            cov::element_dl<double>(ka, kb, g, h, p, ua, ub, sil[ca], sil[cb], A, B);
            const double t = v * A, tb = v * B;
            Sl += t * r2;
            if (ka >= 0) RB[m][r] += tb;
            if (kb >= 0) CB[nn] += tb;
            acc[m][nn][r] = t;  // kept for the per-dimension pass (ARD)
          }
        } else {
          double kf, kd;
          cov::value_kd<KERNEL>(r2, sf2, kf, kd);
          Sf += v * kf;
          if constexpr (GROUPS) {
            // (the noise entry is formed before the path passes)
          } else if (WEIGHTED) {
            if (gi == gj && gi < n) Sn += v * wv[gi];
          } else {
            if (gi == gj) Sn += v;
          }
          const double t = v * kd;
          Sl += t * r2;
          acc[m][nn][r] = t;  // kept for the per-dimension pass (ARD)
        }
        // one element at a time: left alone, the scheduler interleaves all 64 evaluations of
        // this fully unrolled nest (the accumulators must stay in registers) and spills hundreds
        // of VGPRs; the epilogue is < 1 % of the tile's time either way
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  const double w = (ti == tj) ? 1.0 : 2.0;
  double* out = part + lin * ntheta;
  const int nls = ntheta - (KINDS ? 3 : GROUPS ? 3 + n_ls : 2);
  if (!ard) {
    if constexpr (KINDS) {  // one lengthscale: every dimension a kind names is that one
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) Sl += RB[m][r];
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) Sl += CB[nn];
    }
    const double s = wg_sum(Sl, red);
    if (tid == 0) out[0] = w * s;
  } else {
    for (int c = 0; c < d; ++c) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int il = wr * 64 + m * 16 + l4 + 4 * r;
#pragma unroll
          for (int nn = 0; nn < 4; ++nn) {
            const int jl = wc * 64 + nn * 16 + l15;
            const double e = xa[il * d + c] - xb[jl * d + c];
            s += acc[m][nn][r] * e * e;
          }
          if constexpr (KINDS) {
            if (ska[il] == c) s += RB[m][r];
          }
        }
      if constexpr (KINDS) {
#pragma unroll
        for (int nn = 0; nn < 4; ++nn)
          if (skb[wc * 64 + nn * 16 + l15] == c) s += CB[nn];
      }
      s = wg_sum(s, red);
      if (tid == 0) out[c] = w * s;
    }
  }
  if constexpr (GROUPS) {
    const double sf = wg_sum(Sf, red);
    if (tid == 0) out[nls] = w * sf;
    return;
  }
  const double sf = wg_sum(Sf, red), sn = wg_sum(Sn, red);
  if (tid == 0) {
    out[nls] = w * sf;
    out[nls + 1] = sn * sn2;  // only diagonal tiles hold diagonal elements (w = 1 there)
  }
  if constexpr (KINDS) {
    const double sd = wg_sum(Sd, red);
    if (tid == 0) out[nls + 2] = sd * sn2_deriv;
  }
}

// ---- the alpha alpha^T term: sum_ij (sum_c alpha_ic alpha_jc) (dK/dlog theta)_ij -------------
// 64x64 tiles over the lower triangle (row-major triangular enumeration as the kernel build);
// alphaT (64 x ld): row c = target c.  Same partial layout as above.
__device__ __forceinline__ void tri_coords64(int64_t t, int& ti, int& tj) {
  int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = (int)i;
  tj = (int)(t - i * (i + 1) / 2);
}

// KINDS, GROUPS: as kinv_trace_kernel's.
template <int KERNEL, int D, bool KINDS = false, bool GROUPS = false>
__global__ __launch_bounds__(256) void alpha_quad_kernel(const double* __restrict__ alphaT, int64_t ld, int k,
                                                        int64_t n, const double* __restrict__ Xs, int d_rt,
                                                        int ard, double sf2, double sn2,
                                                        double* __restrict__ part, int ntheta,
                                                        const double* __restrict__ wv,
                                                        const int32_t* __restrict__ kind = nullptr,
                                                        const double* __restrict__ ls = nullptr, int n_ls = 0,
                                                        double sn2_deriv = 0.0) {
  constexpr int KT = 64;
  __shared__ double xa[KT * MAX_D];
  __shared__ double xb[KT * MAX_D];
  __shared__ double red[4];
  const int d = (D > 0) ? D : d_rt;
  int ti, tj;
  tri_coords64((int64_t)blockIdx.x, ti, tj);
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  const int tid = threadIdx.x;
  for (int e = tid; e < KT * d; e += 256) {
    xa[e] = Xs[i0 * d + e];
    xb[e] = Xs[j0 * d + e];
  }
  const int* ska = nullptr;
  const int* skb = nullptr;
  const double* sil = nullptr;
  if constexpr (KINDS) {
    __shared__ int kab[2 * KT];
    __shared__ double ilv[MAX_D];
    if (tid < 2 * KT) kab[tid] = kind[(tid < KT ? i0 : j0 - KT) + tid];
    else if (tid - 2 * KT < d) ilv[tid - 2 * KT] = 1.0 / ls[n_ls == 1 ? 0 : tid - 2 * KT];
    ska = kab, skb = kab + KT, sil = ilv;
  }
  [[maybe_unused]] const int* srng = nullptr;
  if constexpr (GROUPS) {  // wave 0: the row ids, wave 1: the column ids, and their ranges; q
    static_assert(!KINDS, "a fit has path ids or kinds");
    __shared__ int gab[2 * KT];
    __shared__ int rng[4];
    __shared__ double qv[MAX_D];
    if (tid < 2 * KT) {
      const int id = kind[(tid < KT ? i0 : j0 - KT) + tid];
      gab[tid] = id;
      int lo = id >= 0 ? id : INT_MAX, hi = id;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
      }
      if ((tid & 63) == 0) rng[2 * (tid >> 6)] = lo, rng[2 * (tid >> 6) + 1] = hi;
    } else if (tid - 2 * KT < d) {
      qv[tid - 2 * KT] = ls[tid - 2 * KT];
    }
    ska = gab, skb = gab + KT, sil = qv, srng = rng;
  }
  __syncthreads();
  const int jl0 = (tid & 31) * 2, rg = tid >> 5;
  // weights of this thread's 8 rows x 2 columns
  double wt[8][2];
#pragma unroll
  for (int r = 0; r < 8; ++r) wt[r][0] = wt[r][1] = 0.0;
  for (int c = 0; c < k; ++c) {
    const double* a = alphaT + (int64_t)c * ld;
    const double b0 = a[j0 + jl0], b1 = a[j0 + jl0 + 1];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const double ai = a[i0 + rg + 8 * r];
      wt[r][0] += ai * b0;
      wt[r][1] += ai * b1;
    }
  }
  if constexpr (GROUPS) {  // the path entries, while wt holds the weights (kinv_trace_kernel's passes)
    const int nlp = n_ls;
    double* outp = part + (int64_t)blockIdx.x * ntheta + (ntheta - nlp - 1);  // (sg2, l_path...)
    const double wp = (ti == tj) ? 1.0 : 2.0;
    const bool mixed = srng[0] <= srng[3] && srng[2] <= srng[1];  // (no id >= 0 on a side: lo = INT_MAX, hi < 0)
    if (!mixed) {
      if (tid <= nlp) outp[tid] = 0.0;
    } else {
      for (int pass = 0; pass <= (nlp > 1 ? d : 0); ++pass) {
        double s = 0.0, s1 = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int il = rg + 8 * r;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int jl = jl0 + q;
            double pv, pdl;  // (padded rows and columns have id -1: no pair)
            if (cov::path_dtheta<KERNEL>(ska[il], skb[jl], xa + il * d, xb + jl * d, sil, d, sn2_deriv, pass - 1, pv, pdl)) {
              s += wt[r][q] * (pass == 0 ? pv : pdl);
              s1 += wt[r][q] * pdl;
            }
          }
        }
        s = wg_sum(s, red);
        if (pass == 0) {
          if (nlp == 1) s1 = wg_sum(s1, red);
          if (tid == 0) {
            outp[0] = wp * s;
            if (nlp == 1) outp[1] = wp * s1;
          }
        } else if (tid == 0) {
          outp[pass] = wp * s;
        }
      }
    }
  }
  double Sf = 0.0, Sn = 0.0, Sl = 0.0;
  [[maybe_unused]] double Sd = 0.0, RB[8] = {}, CB[2] = {};
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int il = rg + 8 * r;
    const int64_t gi = i0 + il;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int jl = jl0 + q;
      const int64_t gj = j0 + jl;
      double r2 = 0.0;
      for (int c = 0; c < d; ++c) {
        const double e = xa[il * d + c] - xb[jl * d + c];
        r2 += e * e;
      }
      double v = wt[r][q];
      if (gi >= n || gj >= n) v = 0.0;
      if constexpr (KINDS) {
        if constexpr (cov::differentiable(KERNEL)) {
          double kf, g, h, p, A, B;
          cov::value_ghp<KERNEL>(r2, sf2, kf, g, h, p);
          const int ka = ska[il], kb = skb[jl];
          const int ca = ka < 0 ? 0 : ka, cb = kb < 0 ? 0 : kb;
          const double ua = xa[il * d + ca] - xb[jl * d + ca], ub = xa[il * d + cb] - xb[jl * d + cb];
          Sf += v * cov::element<double>(ka, kb, kf, g, h, ua, ub, sil[ca], sil[cb]);
          if (gi == gj && gi < n) {
            const double vw = wv ? v * wv[gi] : v;
            if (ka < 0) Sn += vw;
            else Sd += vw;
          }
          cov::element_dl<double>(ka, kb, g, h, p, ua, ub, sil[ca], sil[cb], A, B);
          const double t = v * A, tb = v * B;
          Sl += t * r2;
          if (ka >= 0) RB[r] += tb;
          if (kb >= 0) CB[q] += tb;
          wt[r][q] = t;
        }
      } else {
        double kf, kd;
        cov::value_kd<KERNEL>(r2, sf2, kf, kd);
        Sf += v * kf;
        if (gi == gj) Sn += (wv && gi < n) ? v * wv[gi] : v;
        const double t = v * kd;
        Sl += t * r2;
        wt[r][q] = t;
      }
    }
  }
  const double w = (ti == tj) ? 1.0 : 2.0;
  double* out = part + (int64_t)blockIdx.x * ntheta;
  const int nls = ntheta - (KINDS ? 3 : GROUPS ? 3 + n_ls : 2);
  if (!ard) {
    if constexpr (KINDS) {
#pragma unroll
      for (int r = 0; r < 8; ++r) Sl += RB[r];
      Sl += CB[0];
      Sl += CB[1];
    }
    const double s = wg_sum(Sl, red);
    if (tid == 0) out[0] = w * s;
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
        if constexpr (KINDS) {
          if (ska[rg + 8 * r] == c) s += RB[r];
        }
      }
      if constexpr (KINDS) {
        if (skb[jl0] == c) s += CB[0];
        if (skb[jl0 + 1] == c) s += CB[1];
      }
      s = wg_sum(s, red);
      if (tid == 0) out[c] = w * s;
    }
  }
  const double sf = wg_sum(Sf, red), sn = wg_sum(Sn, red);
  if (tid == 0) {
    out[nls] = w * sf;
    out[nls + 1] = sn * sn2;
  }
  if constexpr (KINDS) {
    const double sd = wg_sum(Sd, red);
    if (tid == 0) out[nls + 2] = sd * sn2_deriv;
  }
}

// out[t] = scale * sum_tile part[tile * ntheta + t]; one workgroup per theta, fixed order
__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ part, int64_t ntile,
                                                             int ntheta, double scale, double* __restrict__ out) {
  __shared__ double red[4];
  const int t = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < ntile; i += 256) s += part[i * ntheta + t];
  s = wg_sum(s, red);
  if (threadIdx.x == 0) out[t] = scale * s;
}

// out[0] = sum_i sum_c y[i*k + c] * alphaT[c*ld + i]
__global__ __launch_bounds__(256) void dot_rhs_kernel(const double* __restrict__ y, const double* __restrict__ alphaT,
                                                     int64_t ld, int64_t n, int k, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t e = threadIdx.x; e < n * k; e += 256) {
    const int64_t i = e / k;
    const int c = (int)(e - i * k);
    s += y[e] * alphaT[(int64_t)c * ld + i];
  }
  s = wg_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(256) void set_diag_one_kernel(double* A, int64_t lda, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) A[i * lda + i] = 1.0;
}

// ---- d K / d log l_c as a matrix (gpx_kernel_dl_matrix: the unit test of cov::element_dl) --------------------------------
// G[c][i][j] (n_ls blocks of napad x ld) for observations of kinds ka (null: values) at As against kinds kb at Bs; scaled
// points.  Matern-1/2 (values only: the API checks) has A = kd.
template <int KERNEL>
__global__ __launch_bounds__(256) void dl_matrix_kernel(const double* __restrict__ As, const int32_t* __restrict__ ka,
                                                       int64_t na, int64_t napad, const double* __restrict__ Bs,
                                                       const int32_t* __restrict__ kb, int64_t nb, int d,
                                                       const double* __restrict__ ls, int n_ls, double sf2,
                                                       double* __restrict__ G, int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= na * nb) return;
  const int64_t i = e / nb, j = e - i * nb;
  const double* pa = As + i * d;
  const double* pb = Bs + j * d;
  double r2 = 0.0;
  for (int c = 0; c < d; ++c) {
    const double u = pa[c] - pb[c];
    r2 += u * u;
  }
  const int kia = ka ? ka[i] : -1, kib = kb ? kb[j] : -1;
  double A, B = 0.0;
  if constexpr (cov::differentiable(KERNEL)) {
    double v, g, h, p;
    cov::value_ghp<KERNEL>(r2, sf2, v, g, h, p);
    const int ca = kia < 0 ? 0 : kia, cb = kib < 0 ? 0 : kib;
    cov::element_dl<double>(kia, kib, g, h, p, pa[ca] - pb[ca], pa[cb] - pb[cb], 1.0 / ls[n_ls == 1 ? 0 : ca],
                            1.0 / ls[n_ls == 1 ? 0 : cb], A, B);
  } else {
    double v;
    cov::value_kd<KERNEL>(r2, sf2, v, A);
  }
  if (n_ls == 1) {
    G[i * ld + j] = A * r2 + (double)((kia >= 0) + (kib >= 0)) * B;
  } else {
    for (int c = 0; c < d; ++c) {
      const double u = pa[c] - pb[c];
      G[((int64_t)c * napad + i) * ld + j] = A * (u * u) + (double)((kia == c) + (kib == c)) * B;
    }
  }
}

// ---- d (within-path term) / d log (sg2, l_path,c) as a matrix (gpx_kernel_path_dtheta_matrix: the unit test of
// cov::path_dtheta) -----
// G[t][i][j] (1 + n_lsp blocks of napad x ld): t = 0 the term m sg2 k(r_p) itself, t = 1 + c its derivative by log l_path,c
// (n_lsp == 1: by the one l_path); ids ga at the scaled points As against gb at Bs, q (d entries).
template <int KERNEL>
__global__ __launch_bounds__(256) void path_dtheta_matrix_kernel(const double* __restrict__ As, const int32_t* __restrict__ ga,
                                                                int64_t na, int64_t napad, const double* __restrict__ Bs,
                                                                const int32_t* __restrict__ gb, int64_t nb, int d,
                                                                const double* __restrict__ q, int n_lsp, double sg2,
                                                                double* __restrict__ G, int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= na * nb) return;
  const int64_t i = e / nb, j = e - i * nb;
  double v, dl;
  for (int t = 0; t < n_lsp; ++t) {
    cov::path_dtheta<KERNEL>(ga[i], gb[j], As + i * d, Bs + j * d, q, d, sg2, n_lsp == 1 ? -1 : t, v, dl);
    if (t == 0) G[i * ld + j] = v;
    G[((int64_t)(1 + t) * napad + i) * ld + j] = dl;
  }
}

template <int KERNEL>
void launch_kinv_trace_k(const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d, int ard,
                         double sf2, double sn2, double* part, int ntheta, int P, int rank, int dc_nb, int dc_P,
                         int dc_r, int64_t dc_cols, int dc_snake, const double* wv, hipStream_t st,
                         const int32_t* kind = nullptr, const double* ls = nullptr, int n_ls = 0, double sn2_deriv = 0.0,
                         bool groups = false) {
  const int tiles = (int)(npad / 128);
  const int64_t ts = (tiles + 7) / 8;
  const int64_t nslots = ts * (ts - 1) / 2 * 64 + ts * 36;
  const int64_t octets = (nslots + 511) / 512, mine = octets > rank ? (octets - rank + P - 1) / P : 0;
  if (mine == 0) return;
  dim3 grid((unsigned)(mine * 512)), block(256);  // whole octets of 8 x 64 slots
  if (groups) {  // kind: the path ids, ls: q, n_ls: n_ls_path, sn2_deriv: sg2
    switch (d) {
      case 1: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 1, false, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
      case 2: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 2, false, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
      case 3: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 3, false, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
      default: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 0, false, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
    }
    return;
  }
  if (kind) {
    if constexpr (cov::differentiable(KERNEL)) {
      switch (d) {
        case 1: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 1, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
        case 2: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 2, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
        case 3: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 3, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
        default: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 0, false, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv, kind, ls, n_ls, sn2_deriv); break;
      }
    }
    return;
  }
  if (wv) {
    switch (d) {
      case 1: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 1, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
      case 2: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 2, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
      case 3: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 3, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
      default: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 0, true>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
    }
    return;
  }
  switch (d) {
    case 1: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 1, false>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
    case 2: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 2, false>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
    case 3: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 3, false>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
    default: hipLaunchKernelGGL((kinv_trace_kernel<KERNEL, 0, false>), grid, block, 0, st, ZT, ld, tiles, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, nslots, P, rank, dc_nb, dc_P, dc_r, dc_cols, dc_snake, wv); break;
  }
}

template <int KERNEL>
void launch_alpha_quad_k(const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n, const double* Xs, int d,
                         int ard, double sf2, double sn2, double* part, int ntheta, const double* wv, hipStream_t st,
                         const int32_t* kind = nullptr, const double* ls = nullptr, int n_ls = 0, double sn2_deriv = 0.0,
                         bool groups = false) {
  const int64_t T = npad / 64;
  dim3 grid((unsigned)(T * (T + 1) / 2)), block(256);
  if (groups) {
    if (d == 3)
      hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 3, false, true>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, kind, ls, n_ls, sn2_deriv);
    else
      hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 0, false, true>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, kind, ls, n_ls, sn2_deriv);
    return;
  }
  if (kind) {
    if constexpr (cov::differentiable(KERNEL)) {
      if (d == 3)
        hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 3, true>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, kind, ls, n_ls, sn2_deriv);
      else
        hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 0, true>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, kind, ls, n_ls, sn2_deriv);
    }
    return;
  }
  if (d == 3)
    hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 3>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv);
  else
    hipLaunchKernelGGL((alpha_quad_kernel<KERNEL, 0>), grid, block, 0, st, alphaT, ld, k, n, Xs, d, ard, sf2, sn2, part, ntheta, wv);
}

}  // namespace

int64_t kinv_trace_slots(int64_t npad) {
  const int64_t ts = (npad / 128 + 7) / 8;
  return ts * (ts - 1) / 2 * 64 + ts * 36;
}

int64_t alpha_quad_slots(int64_t npad) {
  const int64_t T = npad / 64;
  return T * (T + 1) / 2;
}

void launch_set_diag_one(double* A, int64_t lda, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(set_diag_one_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, lda, n);
}

void launch_kinv_trace(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                       int ard, double sf2, double sn2, double* part, int ntheta, int P, int rank, hipStream_t st,
                       const double* wv) {
  cov::dispatch(kernel, [&](auto fam) { launch_kinv_trace_k<fam>(ZT, ld, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, P, rank, 0, 0, 0, 0, 0, wv, st); });
}

void launch_kinv_trace_kinds(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                             int ard, double sf2, double sn2, double sn2_deriv, const int32_t* kind, const double* ls,
                             int n_ls, double* part, int ntheta, hipStream_t st, const double* wv) {
  cov::dispatch_differentiable(kernel, [&](auto fam) { launch_kinv_trace_k<fam>(ZT, ld, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, 1, 0, 0, 0, 0, 0, 0, wv, st, kind, ls, n_ls, sn2_deriv); });
}

void launch_alpha_quad_kinds(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                             const double* Xs, int d, int ard, double sf2, double sn2, double sn2_deriv,
                             const int32_t* kind, const double* ls, int n_ls, double* part, int ntheta, hipStream_t st,
                             const double* wv) {
  cov::dispatch_differentiable(kernel, [&](auto fam) { launch_alpha_quad_k<fam>(alphaT, ld, k, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, st, kind, ls, n_ls, sn2_deriv); });
}

void launch_kinv_trace_groups(int kernel, const double* ZT, int64_t ld, int64_t npad, int64_t n, const double* Xs, int d,
                              int ard, double sf2, double sn2, double sg2, const int32_t* group, const double* q,
                              int n_lsp, double* part, int ntheta, hipStream_t st, const double* wv) {
  cov::dispatch(kernel, [&](auto fam) { launch_kinv_trace_k<fam>(ZT, ld, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, 1, 0, 0, 0, 0, 0, 0, wv, st, group, q, n_lsp, sg2, true); });
}

void launch_alpha_quad_groups(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                              const double* Xs, int d, int ard, double sf2, double sn2, double sg2, const int32_t* group,
                              const double* q, int n_lsp, double* part, int ntheta, hipStream_t st, const double* wv) {
  cov::dispatch(kernel, [&](auto fam) { launch_alpha_quad_k<fam>(alphaT, ld, k, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, st, group, q, n_lsp, sg2, true); });
}

void launch_path_dtheta_matrix(int kernel, const double* As, const int32_t* ga, int64_t na, int64_t napad, const double* Bs,
                               const int32_t* gb, int64_t nb, int d, const double* q, int n_lsp, double sg2, double* G,
                               int64_t ld, hipStream_t st) {
  cov::dispatch(kernel, [&](auto fam) {
    hipLaunchKernelGGL(path_dtheta_matrix_kernel<fam>, dim3((unsigned)((na * nb + 255) / 256)), dim3(256), 0, st, As, ga, na,
                       napad, Bs, gb, nb, d, q, n_lsp, sg2, G, ld);
  });
}

void launch_dl_matrix(int kernel, const double* As, const int32_t* ka, int64_t na, int64_t napad, const double* Bs,
                      const int32_t* kb, int64_t nb, int d, const double* ls, int n_ls, double sf2, double* G, int64_t ld,
                      hipStream_t st) {
  cov::dispatch(kernel, [&](auto fam) {
    hipLaunchKernelGGL(dl_matrix_kernel<fam>, dim3((unsigned)((na * nb + 255) / 256)), dim3(256), 0, st, As, ka, na, napad, Bs,
                       kb, nb, d, ls, n_ls, sf2, G, ld);
  });
}

void launch_kinv_trace_cols(int kernel, const double* ZTc, int64_t ldc, int64_t npad, int64_t n, const double* Xs,
                            int d, int ard, double sf2, double sn2, double* part, int ntheta, int nb, int P, int rank,
                            int64_t ncols, int snake, hipStream_t st) {
  cov::dispatch(kernel, [&](auto fam) { launch_kinv_trace_k<fam>(ZTc, ldc, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, 1, 0, nb, P, rank, ncols, snake, nullptr, st); });
}

void launch_alpha_quad(int kernel, const double* alphaT, int64_t ld, int k, int64_t npad, int64_t n,
                       const double* Xs, int d, int ard, double sf2, double sn2, double* part, int ntheta,
                       hipStream_t st, const double* wv) {
  cov::dispatch(kernel, [&](auto fam) { launch_alpha_quad_k<fam>(alphaT, ld, k, npad, n, Xs, d, ard, sf2, sn2, part, ntheta, wv, st); });
}

void launch_reduce_partials(const double* part, int64_t ntile, int ntheta, double scale, double* out,
                            hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ntheta), dim3(256), 0, st, part, ntile, ntheta, scale, out);
}

void launch_dot_rhs(const double* y, const double* alphaT, int64_t ld, int64_t n, int k, double* out,
                    hipStream_t st) {
  hipLaunchKernelGGL(dot_rhs_kernel, dim3(1), dim3(256), 0, st, y, alphaT, ld, n, k, out);
}

}  // namespace gpx
