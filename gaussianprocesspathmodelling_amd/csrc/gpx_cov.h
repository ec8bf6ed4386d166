// gpx_cov.h — the covariance families (GPX_KERNEL_*, include/gpx.h), defined once for every HIP kernel that evaluates
// k(r) and for the host.  With u = x / l (per dimension), r^2 = sum_j (u_j - u'_j)^2 and d_c = (x_c - x'_c) / l_c:
//
//   id  family      s        poly(s)          dpoly(s)        e
//   0   RBF         -        1                1               exp(-r^2 / 2)
//   1   Matern-5/2  sqrt5 r  1 + s + s^2/3    (5/3)(1 + s)    exp(-s)
//   2   Matern-3/2  sqrt3 r  1 + s            3               exp(-s)
//   3   Matern-1/2  r        1                -               exp(-s)
//
//   v  = sf2 (poly(s) e)    the value sf2 k(r)
//   g  = sf2 (dpoly(s) e)   d k / d x*_j = -g (u*_j - u_j) / l_j   (RBF: g = v)
//   kd = g                  d K / d log l_c = kd d_c^2;  Matern-1/2: kd = v / r, 0 at r = 0 (kd d_c^2 <= sf2 r -> 0)
//   h                       d g / d x'_j = h (u_j - u'_j) / l_j: the second-derivative block (derivative observations)
//        RBF         v
//        Matern-5/2  sf2 (25/3) e
//        Matern-3/2  9 sf2 e / s, taken as 0 at r = 0 (h only ever multiplies u_i u_j, and h u_i u_j <= 9 sf2 r / sqrt3 -> 0)
//        Matern-1/2  -
//
// Observation kinds (element): a row of a fit is a value of f (kind -1) or of d f / d x_j (kind j); with u = (x_a - x_b) / l
//   (-1, -1)  v                 ( i, -1)  -g u_i / l_i
//   (-1,  j)  +g u_j / l_j      ( i,  j)  (g delta_ij - h u_i u_j) / (l_i l_j)      at r = 0: (j, j) = grad_prior sf2 / l_j^2
//
// Derivative of an element E of kinds (ka, kb) by a log lengthscale (element_dl; the LML gradient of a fit with derivative
// observations): d E / d log l_c = A u_c^2 + (delta(ka, c) + delta(kb, c)) B, with p = -2 d h / d (r^2):
//        RBF         v
//        Matern-5/2  sf2 (125/3) e / s, taken as 0 at r = 0          (p only ever multiplies u_i u_j u_c^2 -> 0)
//        Matern-3/2  27 sf2 e (1 + s) / s^3, taken as 0 at r = 0
//   (-1, -1)  A = g                B = 0
//   (-1,  j)  A = +h u_j / l_j     B = -2 g u_j / l_j
//   ( i, -1)  A = -h u_i / l_i     B = +2 g u_i / l_i
//   ( i,  j)  A = (h delta_ij - p u_i u_j) / (l_i l_j)      B = (2 h u_i u_j - g delta_ij) / (l_i l_j)
// One lengthscale for all dimensions sums over c: A r^2 + ((ka >= 0) + (kb >= 0)) B.
//
// Every kernel evaluates these in this one operation order (value / value_g / value_gh / value_ghp / value_kd): for one element type and
// exponential, the value rows of the derivative build and the kf of the LML gradient are bit for bit the kernel build's
// K.  Matern-1/2 has no derivative at r = 0: it has no g, and no derivative kernel is instantiated for it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/gpx.h"

namespace gpx {
namespace cov {

constexpr bool known(int kernel) { return kernel >= GPX_KERNEL_RBF && kernel <= GPX_KERNEL_MATERN12; }
constexpr bool differentiable(int kernel) { return known(kernel) && kernel != GPX_KERNEL_MATERN12; }
// prior Var[d f / d x_j] = grad_prior sf2 / l_j^2, i.e. dpoly(0), of a differentiable family
constexpr double grad_prior(int kernel) {
  return kernel == GPX_KERNEL_MATERN52 ? 5.0 / 3.0 : kernel == GPX_KERNEL_MATERN32 ? 3.0 : 1.0;
}

constexpr double SQRT5 = 2.23606797749978969640917366873128;
constexpr double SQRT3 = 1.73205080756887729352744634150587;

struct Exp {
  template <typename T>
  __device__ __forceinline__ T operator()(T x) const { return exp(x); }
};

template <int KERNEL, typename T>
__device__ __forceinline__ T svar(T r2) {  // s (unused by RBF)
  constexpr double scale = KERNEL == GPX_KERNEL_MATERN52 ? SQRT5 : KERNEL == GPX_KERNEL_MATERN32 ? SQRT3 : 1.0;
  return KERNEL == GPX_KERNEL_RBF ? (T)0 : (T)scale * sqrt(r2);
}

template <int KERNEL, typename T>
__device__ __forceinline__ T earg(T r2, T s) {  // the argument of e
  return KERNEL == GPX_KERNEL_RBF ? (T)-0.5 * r2 : -s;
}

template <int KERNEL, typename T>
__device__ __forceinline__ T poly(T s) {
  if constexpr (KERNEL == GPX_KERNEL_MATERN52) return (T)1 + s + s * s / (T)3;
  else if constexpr (KERNEL == GPX_KERNEL_MATERN32) return (T)1 + s;
  else return (T)1;
}

template <int KERNEL, typename T>
__device__ __forceinline__ T dpoly(T s) {
  static_assert(differentiable(KERNEL), "Matern-1/2 is not differentiable");
  if constexpr (KERNEL == GPX_KERNEL_MATERN52) return (T)(5.0 / 3.0) * ((T)1 + s);
  else if constexpr (KERNEL == GPX_KERNEL_MATERN32) return (T)3;
  else return (T)1;
}

template <int KERNEL, typename T, typename E = Exp>
__device__ __forceinline__ T value(T r2, T sf2, E ex = {}) {
  const T s = svar<KERNEL>(r2);
  return sf2 * (poly<KERNEL>(s) * ex(earg<KERNEL>(r2, s)));
}

template <int KERNEL, typename T, typename E = Exp>
__device__ __forceinline__ void value_g(T r2, T sf2, T& v, T& g, E ex = {}) {
  const T s = svar<KERNEL>(r2);
  const T e = ex(earg<KERNEL>(r2, s));
  v = sf2 * (poly<KERNEL>(s) * e);
  g = sf2 * (dpoly<KERNEL>(s) * e);
}

// v and g as value_g forms them (the same bits), and h
template <int KERNEL, typename T, typename E = Exp>
__device__ __forceinline__ void value_gh(T r2, T sf2, T& v, T& g, T& h, E ex = {}) {
  static_assert(differentiable(KERNEL), "Matern-1/2 is not differentiable");
  const T s = svar<KERNEL>(r2);
  const T e = ex(earg<KERNEL>(r2, s));
  v = sf2 * (poly<KERNEL>(s) * e);
  g = sf2 * (dpoly<KERNEL>(s) * e);
  if constexpr (KERNEL == GPX_KERNEL_MATERN52) h = sf2 * ((T)(25.0 / 3.0) * e);
  else if constexpr (KERNEL == GPX_KERNEL_MATERN32) h = s > (T)0 ? sf2 * ((T)9 * e) / s : (T)0;
  else h = v;
}

// The covariance of an observation of kind ka at x_a with one of kind kb at x_b (the table above) — the one place the
// mixed formula exists.  ua = u_ka and ila = 1 / l_ka (anything when ka < 0), ub and ilb the same for kb; u = (x_a - x_b) / l.
// Products of the two sides are formed side by side, so that swapping a and b (u -> -u) gives the same bits.
template <typename T>
__host__ __device__ __forceinline__ T element(int ka, int kb, T v, T g, T h, T ua, T ub, T ila, T ilb) {
  if (ka < 0) return kb < 0 ? v : g * ub * ilb;
  if (kb < 0) return -g * ua * ila;
  return ((ka == kb ? g : (T)0) - h * (ua * ub)) * (ila * ilb);
}

// Second derivatives by the query point (gpx_hess.hip).  k is twice mean-square differentiable for RBF
// and Matern-5/2 only (h(0) is unbounded for Matern-3/2 and absent for Matern-1/2), and there
//   prior Var[d_i d_j f] = hess_prior sf2 / (l_i^2 l_j^2)  (i != j),   3 hess_prior sf2 / l_i^4  (i == j),   hess_prior = h(0) / sf2
constexpr bool twice_differentiable(int kernel) { return kernel == GPX_KERNEL_RBF || kernel == GPX_KERNEL_MATERN52; }
constexpr double hess_prior(int kernel) { return kernel == GPX_KERNEL_MATERN52 ? 25.0 / 3.0 : 1.0; }

// The covariance of d^2 f / d x_i d x_j at x_a with an observation of kind kb at x_b, u = (x_a - x_b) / l:
//   kb < 0   (h u_i u_j - g delta_ij) / (l_i l_j), the negative of element(i, j) — its bits
//   kb = c   (p u_i u_j u_c - h (delta_ic u_j + delta_jc u_i + delta_ij u_c)) / (l_i l_j l_c)
// ub = u_kb and ilb = 1 / l_kb (anything when kb < 0); p as value_ghp forms it.
template <typename T>
__host__ __device__ __forceinline__ T hess_element(int i, int j, int kb, T v, T g, T h, T p, T ui, T uj, T ub, T ili, T ilj,
                                                   T ilb) {
  if (kb < 0) return -element<T>(i, j, v, g, h, ui, uj, ili, ilj);
  const T s = (i == kb ? uj : (T)0) + (j == kb ? ui : (T)0) + (i == j ? ub : (T)0);
  return (p * ((ui * uj) * ub) - h * s) * ((ili * ilj) * ilb);
}

// v, g and h as value_gh forms them (the same bits), and p
template <int KERNEL, typename T, typename E = Exp>
__device__ __forceinline__ void value_ghp(T r2, T sf2, T& v, T& g, T& h, T& p, E ex = {}) {
  static_assert(differentiable(KERNEL), "Matern-1/2 is not differentiable");
  const T s = svar<KERNEL>(r2);
  const T e = ex(earg<KERNEL>(r2, s));
  v = sf2 * (poly<KERNEL>(s) * e);
  g = sf2 * (dpoly<KERNEL>(s) * e);
  if constexpr (KERNEL == GPX_KERNEL_MATERN52) {
    h = sf2 * ((T)(25.0 / 3.0) * e);
    p = s > (T)0 ? sf2 * ((T)(125.0 / 3.0) * e) / s : (T)0;
  } else if constexpr (KERNEL == GPX_KERNEL_MATERN32) {
    h = s > (T)0 ? sf2 * ((T)9 * e) / s : (T)0;
    p = s > (T)0 ? sf2 * ((T)27 * e * ((T)1 + s)) / (s * s * s) : (T)0;
  } else {
    h = v;
    p = v;
  }
}

// d element / d log l_c = A u_c^2 + (delta(ka, c) + delta(kb, c)) B (the table above), arguments as element's.  The same
// discipline: products of the two sides side by side, so that swapping a and b (u -> -u) gives the same bits.
template <typename T>
__host__ __device__ __forceinline__ void element_dl(int ka, int kb, T g, T h, T p, T ua, T ub, T ila, T ilb, T& A, T& B) {
  if (ka < 0) {
    if (kb < 0) {
      A = g, B = (T)0;
    } else {
      A = h * ub * ilb, B = (T)-2 * g * ub * ilb;
    }
  } else if (kb < 0) {
    A = -h * ua * ila, B = (T)2 * g * ua * ila;
  } else {
    const T uu = ua * ub, ll = ila * ilb;
    A = ((ka == kb ? h : (T)0) - p * uu) * ll;
    B = ((T)2 * h * uu - (ka == kb ? g : (T)0)) * ll;
  }
}

template <int KERNEL, typename T, typename E = Exp>
__device__ __forceinline__ void value_kd(T r2, T sf2, T& v, T& kd, E ex = {}) {
  if constexpr (KERNEL == GPX_KERNEL_MATERN12) {
    const T r = svar<KERNEL>(r2);
    v = sf2 * (poly<KERNEL>(r) * ex(earg<KERNEL>(r2, r)));
    kd = r > (T)0 ? v / r : (T)0;
  } else {
    value_g<KERNEL>(r2, sf2, v, kd, ex);
  }
}

// The within-path term sg2 k(r_p) of a pair with path ids (ga, gb) and its derivatives by the log path parameters (the LML
// gradient of a fit with path ids) — the one place they exist.  pa / pb: the pair's SCALED points (x / l), q_c = (l_c /
// l_path,c)^2, so r_p^2 = sum_c q_c e_c^2 with e = pa - pb (the kernel build's own operation order).  A same-path pair
// (ga == gb >= 0) returns true with v = sg2 k(r_p) = d / dlog sg2 and
//   c >= 0:  dl = kd(r_p; sg2) q_c e_c^2 = d / dlog l_path,c        c < 0:  dl = kd r_p^2, their sum (one l_path for all)
// Any other pair returns false with v = dl = 0 and evaluates no exponential.  e enters only squared: swapping the two
// sides gives the same bits.
template <int KERNEL, typename T>
__device__ __forceinline__ bool path_dtheta(int ga, int gb, const T* pa, const T* pb, const T* q, int d, T sg2, int c, T& v,
                                            T& dl) {
  v = dl = (T)0;
  if (ga < 0 || ga != gb) return false;
  T rp2 = (T)0, tc = (T)0;
  for (int j = 0; j < d; ++j) {
    const T e = pa[j] - pb[j];
    const T t = q[j] * (e * e);
    rp2 += t;
    if (j == c) tc = t;
  }
  T kd;
  value_kd<KERNEL>(rp2, sg2, v, kd);
  dl = kd * (c < 0 ? rp2 : tc);
  return true;
}

// f(std::integral_constant<int, id>{}) for the family `kernel` (the API refuses unknown ids before any launch)
template <typename F>
void dispatch(int kernel, F&& f) {
  switch (kernel) {
    case GPX_KERNEL_RBF: f(std::integral_constant<int, GPX_KERNEL_RBF>{}); break;
    case GPX_KERNEL_MATERN52: f(std::integral_constant<int, GPX_KERNEL_MATERN52>{}); break;
    case GPX_KERNEL_MATERN32: f(std::integral_constant<int, GPX_KERNEL_MATERN32>{}); break;
    default: f(std::integral_constant<int, GPX_KERNEL_MATERN12>{}); break;
  }
}

// the same over the differentiable families: f is not instantiated for the others, whose ids call nothing
template <typename F>
void dispatch_differentiable(int kernel, F&& f) {
  dispatch(kernel, [&](auto K) {
    if constexpr (differentiable(K)) f(K);
  });
}

}  // namespace cov
}  // namespace gpx
