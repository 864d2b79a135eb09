// The MARTINI energy terms, spelled out once: minimum image, shifted-cut-off 12-6 Lennard-Jones, harmonic bond, G96
// cosine / harmonic angle (mythos/energy/martini/m2/lj.py:55-88, m2/bond.py:34-40, m2/angle.py:35-93, m3/angle.py:8-11,
// martini/base.py:15-17).  Instantiated by the energy and parameter-gradient kernels (martini.hip), by the step kernel
// (martini_md.hip) and, at double for the host, by oracle/cpu_port/martini_cpu.cpp - the build the sanitizers run.
//
// The units are compiled with -ffp-contract=on: a multiply-add is fused where ONE source expression has that shape, and
// the tests hold the callers' results bitwise.  So the functions return factors (x, the gradient coefficient, the powers)
// and the callers keep their accumulations - `gx += g * dx`, 1/2 k x^2 in double or in R, their sums of squares.
#pragma once
#include "oxdna_math.h"

namespace mythos {

__device__ __forceinline__ float m_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double m_atan2(double y, double x) { return atan2(y, x); }

// minimum image in an orthorhombic box; il = 1 / l
template <typename R>
__device__ __forceinline__ R wrap(R d, R l, R il) {
  return d - l * m_rint(d * il);
}

// Fused multiply-add spelled out.  The squared distance of the row walk decides which entries the pruned rows keep: every
// instantiation of the step kernel has to round it the same way, whatever contraction the compiler would choose for it
// (the energy-trace and the plain instantiation disagreed in the last bit of r^2 in fp64, kept different entries at
// the edge of the pruned range, and the sums behind that entry fell into other lanes).
__device__ __forceinline__ float m_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double m_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename R>
__device__ __forceinline__ R wrap_fma(R d, R l, R il) {
  return m_fma(-l, m_rint(d * il), d);
}

// ---- Lennard-Jones, V = 4 eps [(s12 - s6) - (c12 - c6)] inside r_c, s6 = (sigma / r)^6, c6 = (sigma / r_c)^6
template <typename R>
struct LjPair {
  R s6, s12, g;  // the two powers and (dV/dr) / r
};
// (sigma^2 x)^3: s6 for x = 1 / r^2, c6 for x = 1 / r_c^2
template <typename R>
__device__ __forceinline__ R lj_pow6(R sig2, R x) {
  const R s2 = sig2 * x;
  return s2 * s2 * s2;
}
template <typename R>
__device__ __forceinline__ LjPair<R> lj_pair(R sig2, R ep, R r2) {
  const R ir2 = R(1) / r2;
  const R s6 = lj_pow6(sig2, ir2), s12 = s6 * s6;
  return {s6, s12, R(-24) * ep * (R(2) * s12 - s6) * ir2};
}
// the shifted pair energy in units of 4 eps
template <typename R>
__device__ __forceinline__ R lj_shifted(const LjPair<R>& t, R c6) {
  return (t.s12 - t.s6) - (c6 * c6 - c6);
}

// ---- reaction-field Coulomb with the potential shifted to 0 at r_c (GROMACS, coulombtype = reaction-field under the
// Verlet scheme): V = qq (1/r + k_rf r^2 - c_rf) for a pair inside r_c, V = qq (k_rf r^2 - c_rf) for an excluded (bonded)
// pair inside r_c, qq = (f / eps_r) q_i q_j.  The factors are per unit qq; 1/r^3 from one reciprocal square root.
template <typename R>
struct RfPair {
  R v, g;  // V / qq and (dV/dr) / (r qq)
};
template <typename R>
__device__ __forceinline__ RfPair<R> rf_pair(R r2, R k_rf, R c_rf) {
  const R ir = m_rsqrt(r2);
  return {ir + k_rf * r2 - c_rf, R(2) * k_rf - ir * ir * ir};
}
template <typename R>
__device__ __forceinline__ RfPair<R> rf_excluded(R r2, R k_rf, R c_rf) {
  return {k_rf * r2 - c_rf, R(2) * k_rf};
}

// ---- harmonic bond, E = 1/2 k x^2, from the squared length of the wrapped displacement d; dE/dd = c d
template <typename R>
struct BondTerm {
  R x, c;  // r - r0 and k x / r
};
template <typename R>
__device__ __forceinline__ BondTerm<R> bond_term(R r2, R k, R r0) {
  const R r = m_sqrt(r2), x = r - r0;
  return {x, k * x / r};
}

// ---- angle i - j - k, E = 1/2 k x^2 with x = cos(theta) - cos(theta0) (kind 0, G96) or theta - theta0 (kind 1, harmonic)
template <typename R>
struct AngleGeom {
  R c, iu, iv;  // cos(theta), 1 / |u|, 1 / |v|
  R sn;         // |uhat x vhat| for the atan2 form of the reference (m2/angle.py:49-58); kind 1 only
};
// geometry from the wrapped arms u = r_i - r_j, v = r_k - r_j and their products u2 = u.u, v2 = v.v, uv = u.v
template <typename R>
__device__ __forceinline__ AngleGeom<R> angle_geometry(const R (&u)[3], const R (&v)[3], R u2, R v2, R uv, int kind) {
  const R iu = R(1) / m_sqrt(u2), iv = R(1) / m_sqrt(v2);
  const R c = uv * iu * iv;
  R sn = 0;
  if (kind != 0) {
    const R cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    sn = m_sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) * iu * iv;
  }
  return {c, iu, iv, sn};
}
template <typename R>
struct AngleTerm {
  R x, dEdc;  // dEdc = dE / dcos(theta)
};
// ref: cos(theta0) for kind 0, theta0 for kind 1
template <typename R>
__device__ __forceinline__ AngleTerm<R> angle_term(int kind, const AngleGeom<R>& g, R k, R ref) {
  if (kind == 0) {
    const R x = g.c - ref;
    return {x, k * x};
  }
  const R x = m_atan2(g.sn, g.c) - ref;
  // d(theta)/d(cos) = -1/sin; (theta - pi)/sin(theta) -> -1 at theta = pi
  return {x, (g.sn > R(1e-6)) ? -k * x / g.sn : k};
}
// one component of dcos/dr of the bead in `role` (0: first bead, 1: centre, 2: last bead), from that component of u and v:
// dc/du = (vhat - c uhat)/|u|, dc/dv = (uhat - c vhat)/|v|
template <typename R>
__device__ __forceinline__ R angle_role_grad(int role, const AngleGeom<R>& g, R uk, R vk) {
  const R du = (vk * g.iv - g.c * uk * g.iu) * g.iu, dv = (uk * g.iu - g.c * vk * g.iv) * g.iv;
  return (role == 0) ? du : ((role == 2) ? dv : -(du + dv));
}

}  // namespace mythos
