// What the two kernels that evaluate oxDNA's `bond` and `mindistance` order parameters share - order_params_kernel on
// stored rows (order_params.hip) and umbrella_decide_kernel on the resident frame (umbrella.hip): one listed pair's
// hydrogen-bonding energy and base-base distance, and the per-lane partials they go into.  One body, so the two kernels'
// values are the same bit for bit on the same (centre, quaternion) words.
#pragma once
#include "mythos_internal.h"
#include "oxdna_gather.h"

namespace mythos {

// A non-negative IEEE number orders as the unsigned integer of its bit pattern: what lets a smallest distance be folded
// with integer minima, in any order, reproducible bit for bit.
template <typename R>
struct OrderedBits;
template <>
struct OrderedBits<float> {
  using type = unsigned int;
  static __device__ __forceinline__ type of(float v) { return __float_as_uint(v); }
  static __device__ __forceinline__ float back(type b) { return __uint_as_float(b); }
};
template <>
struct OrderedBits<double> {
  using type = unsigned long long;
  static __device__ __forceinline__ type of(double v) { return (type)__double_as_longlong(v); }
  static __device__ __forceinline__ double back(type b) { return __longlong_as_double((long long)b); }
};

// Pair (i, j), i the lower index (role p, the reference's i < j pairs), with its full weight: e_hb - the energy kernel's
// hydrogen-bonding energy (unbonded_angular_geo with TERMS = 1, no gradients; 0 unless want_hb) - and r, the base-base
// distance.  The energy takes the minimum image of the CENTRE displacement, as the energy kernel does; the distance that
// of the displacement between the SITES, as the reference's displacement function does - the same vector for any pair
// close enough to bind, and the shorter one where a component of the displacement is near half a box edge.
template <typename R, int MODEL, class Loader>
__device__ __forceinline__ void order_param_pair(const ConstParams<R, false>& P, const UniGeo<R, MODEL>& geo, const Loader& ld,
                                                 const BoxT<R>& box, int i, int j, bool want_hb, R& e_hb, R& r) {
  Nuc<R> p, q;
  R q4[4];
  ld.load(i, p, q4);
  ld.load(j, q, q4);
  const V3<R> raw = q.c - p.c;
  const V3<R> dco = min_image(raw, box);
  const V3<R> d = min_image(geo.base_base(raw, p, q), box);
  r = m_sqrt(dot(d, d));
  R e[T_COUNT];
#pragma unroll
  for (int t = 0; t < T_COUNT; ++t) e[t] = R(0);
  if (want_hb) {
    SelfGrad<R> sg;
    NoPG pg;
    unbonded_angular_geo<R, MODEL, false, NoPG, 1>(P, p, q, dco, true, R(1), e, sg, pg, geo);
  }
  e_hb = e[T_HB];
}

// a lane's partials of one order parameter: the count of pairs below the cutoff and the smallest distance as ordered bits
template <typename R>
__device__ __forceinline__ void order_param_accumulate(R e_hb, R r, double hb_cutoff, int& count, typename OrderedBits<R>::type& nearest) {
  count += (double(e_hb) < hb_cutoff) ? 1 : 0;
  const typename OrderedBits<R>::type b = OrderedBits<R>::of(r);
  nearest = b < nearest ? b : nearest;
}

}  // namespace mythos
