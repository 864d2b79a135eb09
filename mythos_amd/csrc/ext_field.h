// Position-dependent external forces of the oxDNA Langevin integrator (mythos_langevin_set_restraints): harmonic tethers
// of single nucleotides, harmonic restraints of the SUM of a group's positions, and a torque on a group applied as forces
// on its members' centres (LAMMPS' spring/self, addforce with a variable of the summed coordinates, addtorque - the
// stretch-torsion protocol) - and the point terms of mythos_langevin_set_point_forces, oxDNA's
// moving `string`, `trap`, `mutual_trap`, `repulsion_plane` and `repulsion_sphere`, one term on one nucleotide each.  All
// act on centres of mass; none is a body torque.
//
// Time: the moving laws take the step count s of the frame whose positions the force is taken at - the integrator's
// step counter (mythos_langevin_get_step) when that frame was reached.  The kick in front of launch k of a queue gets
// s = step_at_queue_start + k as a double computed on the host, the number its stamp is made of: the same whether the
// launch runs once, is halted and resumed behind a rebuilt list, or belongs to the second of two advances.  Both half
// kicks around frame s (the closing one of step s - 1 and the opening one of step s) use F(x_s, s).
//
// Two launches in the queue slot of ext_kick_kernel (langevin_frame.h), in front of a step launch:
//   ext_group_kernel       one workgroup of 256 per group: the group's sum / centroid and S in double, an LDS tree in
//                          fixed order, into the group's row of 8 doubles.  A pure function of the positions, which no
//                          kick writes, so it needs no stamp and no skip: run twice it writes the same row.
//   ext_field_kick_kernel  one thread per restrained nucleotide (an `entry`): it gathers the terms that name the
//                          nucleotide - its tether, then its groups in the order of the group list, then its point
//                          terms in the order they were given - adds them in double in that order and kicks the
//                          momentum once.  No two threads write one momentum, so there is no
//                          atomic and no order between workgroups to fix; a nucleotide in a tether and two groups gets
//                          the same bits whatever the schedule.  Every workgroup follows ext_kick_kernel's protocol with
//                          a stamp word of its OWN (workgroups do not synchronise): every thread reads it in front of a
//                          barrier, thread 0 replaces it behind the kick.
// Coordinates are taken as the frame stores them - p0, plus the low parts pl of the fp32 hi + lo form - without a minimum
// image: the integrator never folds a coordinate into the box (langevin_step.h applies the minimum image to differences
// only), so a restrained nucleotide's coordinate is continuous along a run.  The one difference taken is a mutual
// trap's, x_ref - x, and that one gets the minimum image where its term asks for it (PBC = 1).
#pragma once
#include "langevin_step.h"

namespace mythos {

enum : int { EXT_GROUP_SUM = 0, EXT_GROUP_TORQUE = 1 };
// enum mythos_point_force_kind of include/mythos_hip.h; the rows of pt_param (d: dir / |dir|, normalised by the host):
//   STRING       F0, rate, d.xyz, origin.xyz      F = (F0 + rate s) d                     U = -(F0 + rate s) d.(x - origin)
//   TRAP         stiff, rate, d.xyz, pos0.xyz     F = -stiff (x - pos0 - rate s d)        U = stiff / 2 |...|^2
//   MUTUAL_TRAP  stiff, r0, rate                  F = stiff (r - r0 - rate s) D / r       U = stiff / 2 (r - r0 - rate s)^2
//                                                 D = x_ref - x (minimum image under EXT_POINT_PBC), r = |D|; r = 0: no force
//   PLANE        stiff, position, d.xyz           h = d.x + position < 0: F = -stiff h d  U = stiff / 2 h^2
//   SPHERE       stiff, r0, rate, center.xyz      |rho| > R = r0 + rate s: F = -stiff (1 - R / |rho|) rho, rho = x - center
//                                                                                         U = stiff / 2 (|rho| - R)^2
enum : int { EXT_POINT_STRING = 0, EXT_POINT_TRAP = 1, EXT_POINT_MUTUAL_TRAP = 2, EXT_POINT_PLANE = 3, EXT_POINT_SPHERE = 4, EXT_POINT_KINDS = 5 };
enum : int { EXT_POINT_PBC = 1 };
constexpr int kExtPointParams = 8;  // doubles per point term
constexpr int kExtEnergies = 3 + EXT_POINT_KINDS;  // mythos_langevin_eval_external_at: constant, tether, sum, then one per point kind
constexpr int kExtRow = 8;  // doubles per group row: sum (F.x, F.y, F.z, U, ...); torque (centroid.xyz, 1 / S, ...)

// device arrays of one set of restraints and one set of point terms (mythos_sim owns them)
struct ExtFieldView {
  int n_tethers = 0, n_groups = 0, n_entries = 0;
  const int* t_index = nullptr;      // [n_tethers] distinct nucleotides
  const double* t_k = nullptr;       // [n_tethers]
  const double* t_anchor = nullptr;  // [n_tethers][3]
  const int* t_mask = nullptr;       // [n_tethers] bit a: axis a is restrained
  const int* g_kind = nullptr;       // [n_groups] EXT_GROUP_*
  const int* g_first = nullptr;      // [n_groups + 1] member range
  const int* g_member = nullptr;     // members, distinct within a group
  const double* g_vec = nullptr;     // [n_groups][3] sum: (k, -, -); torque: T
  const double* g_target = nullptr;  // [n_groups][3] sum: s0
  const int* g_mask = nullptr;       // [n_groups] sum: axis bits
  double* g_row = nullptr;           // [n_groups][kExtRow] written by ext_group_kernel
  const int* e_index = nullptr;      // [n_entries] the restrained nucleotides, ascending
  const int* e_first = nullptr;      // [n_entries + 1] term range of an entry
  const int* e_term = nullptr;       // t >= 0: tether t; ~g < 0: group g; per entry the tether first, then groups ascending
  // point terms (mythos_langevin_set_point_forces), stored sorted by nucleotide and, within one, in the order given: the
  // terms of entry e are pt_first[e] .. pt_first[e + 1).  n_points = 0: the arrays below are null and never read.
  int n_points = 0;
  const int* pt_first = nullptr;     // [n_entries + 1]
  const int* pt_kind = nullptr;      // [n_points] EXT_POINT_*
  const int* pt_particle = nullptr;  // [n_points] the nucleotide the term acts on (the energy sum reads it)
  const int* pt_ref = nullptr;       // [n_points] mutual trap: the partner, which needs no entry of its own
  const int* pt_flags = nullptr;     // [n_points] EXT_POINT_PBC
  const double* pt_param = nullptr;  // [n_points][kExtPointParams]
  double box[3] = {1, 1, 1};         // the system's box, for the minimum image of a mutual trap with EXT_POINT_PBC
};

// centre of nucleotide i in double (pl: the low parts of an fp32 frame, or null)
template <typename R>
__device__ inline void ext_centre(const typename Vec4T<R>::type* __restrict__ p0, const typename Vec4T<R>::type* __restrict__ pl, int i,
                                  double (&x)[3]) {
  const auto a = p0[i];
  x[0] = double(a.x), x[1] = double(a.y), x[2] = double(a.z);
  if (pl) {
    const auto l = pl[i];
    x[0] += double(l.x), x[1] += double(l.y), x[2] += double(l.z);
  }
}

// v[k] <- the sum of v[k] over the 256 threads of the workgroup, in the fixed order of a binary tree; every thread gets it
template <int K>
__device__ inline void ext_block_sum(double (&red)[4][256], double (&v)[K]) {
  static_assert(K <= 4, "red has four rows");
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][t] += red[k][t + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = red[k][0];
  __syncthreads();  // (red is used again)
}

// A torque group whose members all lie on the axis through their centroid has S = 0 and gets no force.  In floating
// point the centroid carries the rounding of the coordinates it was summed from, so S of such a group is of the order
// (eps |x|)^2, not 0: S at or below 1e-24 sum |x_j|^2 - a spread across the axis under 1e-12 of the coordinates, four
// digits above the rounding of a double and far under any spread of matter - counts as zero.
constexpr double kExtTorqueFloor = 1e-24;

template <typename R>
__global__ __launch_bounds__(256) void ext_group_kernel(const ExtFieldView v, const typename Vec4T<R>::type* __restrict__ p0,
                                                        const typename Vec4T<R>::type* __restrict__ pl) {
  __shared__ double red[4][256];
  const int g = blockIdx.x;
  const int b = v.g_first[g], e = v.g_first[g + 1];
  double acc[4] = {0, 0, 0, 0};  // sum of the positions, and of their squares (the scale of the torque floor)
  for (int m = b + (int)threadIdx.x; m < e; m += 256) {
    double x[3];
    ext_centre<R>(p0, pl, v.g_member[m], x);
    acc[0] += x[0], acc[1] += x[1], acc[2] += x[2];
    acc[3] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  }
  ext_block_sum(red, acc);
  double* row = v.g_row + (size_t)g * kExtRow;
  if (v.g_kind[g] == EXT_GROUP_SUM) {
    if (threadIdx.x == 0) {
      const double k = v.g_vec[3 * g];
      const int mask = v.g_mask[g];
      double u = 0;
      for (int a = 0; a < 3; ++a) {
        const double d = ((mask >> a) & 1) ? acc[a] - v.g_target[3 * g + a] : 0.0;
        row[a] = -k * d;
        u += d * d;
      }
      row[3] = 0.5 * k * u;
    }
    return;
  }
  const double inv_m = 1.0 / double(e - b);
  const double c[3] = {acc[0] * inv_m, acc[1] * inv_m, acc[2] * inv_m};
  const double scale2 = acc[3];
  double T[3] = {v.g_vec[3 * g], v.g_vec[3 * g + 1], v.g_vec[3 * g + 2]};
  const double inv_t = 1.0 / sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
  T[0] *= inv_t, T[1] *= inv_t, T[2] *= inv_t;
  double s[1] = {0};
  for (int m = b + (int)threadIdx.x; m < e; m += 256) {
    double x[3];
    ext_centre<R>(p0, pl, v.g_member[m], x);
    const double d[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
    const double along = d[0] * T[0] + d[1] * T[1] + d[2] * T[2];
    const double px = d[0] - along * T[0], py = d[1] - along * T[1], pz = d[2] - along * T[2];
    s[0] += px * px + py * py + pz * pz;
  }
  ext_block_sum(red, s);
  if (threadIdx.x == 0) {
    row[0] = c[0], row[1] = c[1], row[2] = c[2];
    row[3] = s[0] > kExtTorqueFloor * scale2 ? 1.0 / s[0] : 0.0;
  }
}

// Point term j on a nucleotide at x, at step count s: its force added to F, its energy returned.  The one evaluation of
// the five laws (table at EXT_POINT_*): the kick and the energy sum both come here.
template <typename R>
__device__ inline double ext_point_term(const ExtFieldView& v, int j, const typename Vec4T<R>::type* __restrict__ p0,
                                        const typename Vec4T<R>::type* __restrict__ pl, const double (&x)[3], double s, double (&F)[3]) {
  const double* q = v.pt_param + (size_t)j * kExtPointParams;
  switch (v.pt_kind[j]) {
    case EXT_POINT_STRING: {
      const double f = q[0] + q[1] * s;
      F[0] += f * q[2], F[1] += f * q[3], F[2] += f * q[4];
      return -f * (q[2] * (x[0] - q[5]) + q[3] * (x[1] - q[6]) + q[4] * (x[2] - q[7]));
    }
    case EXT_POINT_TRAP: {
      const double k = q[0], shift = q[1] * s;
      double u = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double d = x[a] - q[5 + a] - shift * q[2 + a];
        F[a] -= k * d;
        u += d * d;
      }
      return 0.5 * k * u;
    }
    case EXT_POINT_MUTUAL_TRAP: {
      double y[3], D[3];
      ext_centre<R>(p0, pl, v.pt_ref[j], y);
      const bool wrap = (v.pt_flags[j] & EXT_POINT_PBC) != 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        D[a] = y[a] - x[a];
        if (wrap) D[a] -= v.box[a] * rint(D[a] / v.box[a]);
      }
      const double r = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
      const double stretch = r - q[1] - q[2] * s;
      if (r > 0.0) {
        const double g = q[0] * stretch / r;
        F[0] += g * D[0], F[1] += g * D[1], F[2] += g * D[2];
      }
      return 0.5 * q[0] * stretch * stretch;
    }
    case EXT_POINT_PLANE: {
      const double h = q[2] * x[0] + q[3] * x[1] + q[4] * x[2] + q[1];
      if (!(h < 0.0)) return 0.0;
      const double g = -q[0] * h;
      F[0] += g * q[2], F[1] += g * q[3], F[2] += g * q[4];
      return 0.5 * q[0] * h * h;
    }
    default: {  // EXT_POINT_SPHERE (the host admits no other kind)
      const double rho[3] = {x[0] - q[3], x[1] - q[4], x[2] - q[5]};
      const double dist = sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]);
      const double Rs = q[1] + q[2] * s;
      if (!(dist > Rs) || !(dist > 0.0)) return 0.0;
      const double g = -q[0] * (1.0 - Rs / dist);
      F[0] += g * rho[0], F[1] += g * rho[1], F[2] += g * rho[2];
      return 0.5 * q[0] * (dist - Rs) * (dist - Rs);
    }
  }
}

// The force of the whole set on the nucleotide of entry e (x: its centre) at step count s, terms added in the entry's
// order: its tether, its groups ascending, its point terms as given.  The one evaluation of every law: the kick and
// mythos_langevin_eval_external(_at) both come here.  (p0, pl): the frame x is taken from, for a mutual trap's partner.
template <typename R>
__device__ inline void ext_field_force(const ExtFieldView& v, int e, const typename Vec4T<R>::type* __restrict__ p0,
                                       const typename Vec4T<R>::type* __restrict__ pl, const double (&x)[3], double s, double (&F)[3]) {
  F[0] = F[1] = F[2] = 0.0;
  for (int t = v.e_first[e]; t < v.e_first[e + 1]; ++t) {
    const int code = v.e_term[t];
    if (code >= 0) {  // tether: -k A (x - a)
      const double k = v.t_k[code];
      const int mask = v.t_mask[code];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if ((mask >> a) & 1) F[a] -= k * (x[a] - v.t_anchor[3 * code + a]);
      continue;
    }
    const int g = ~code;
    const double* row = v.g_row + (size_t)g * kExtRow;
    if (v.g_kind[g] == EXT_GROUP_SUM) {  // -k A (s - s0), the same on every member
      F[0] += row[0], F[1] += row[1], F[2] += row[2];
    } else {  // (T x d) / S
      const double d[3] = {x[0] - row[0], x[1] - row[1], x[2] - row[2]};
      const double* T = v.g_vec + 3 * g;
      const double inv_s = row[3];
      F[0] += (T[1] * d[2] - T[2] * d[1]) * inv_s;
      F[1] += (T[2] * d[0] - T[0] * d[2]) * inv_s;
      F[2] += (T[0] * d[1] - T[1] * d[0]) * inv_s;
    }
  }
  if (v.n_points > 0)
    for (int j = v.pt_first[e]; j < v.pt_first[e + 1]; ++j) (void)ext_point_term<R>(v, j, p0, pl, x, s, F);
}

// p_i += c dt F_i(x) on the frame step launch k is about to read, F of the positions of that same frame: both half kicks
// of BAOAB around x_k use the force at x_k, and this kick writes no position, so it commutes with the interaction kick
// exactly as the constant one does.  Behind ext_group_kernel of the same frame.  Protocol: ext_kick_kernel's, with
// stamp[blockIdx.x].  s: the step count of that frame (see Time, above); only point terms read it.
template <typename R>
__global__ __launch_bounds__(256) void ext_field_kick_kernel(const ExtFieldView v, const typename Vec4T<R>::type* __restrict__ p0,
                                                             const typename Vec4T<R>::type* __restrict__ pl, double c_dt, double s,
                                                             typename Vec4T<R>::type* __restrict__ mom, const int* __restrict__ flags,
                                                             const int* __restrict__ list_overflow, int k_index,
                                                             unsigned long long this_stamp, unsigned long long* __restrict__ stamp) {
  const int hw = flags[1], aw = flags[3];
  const int halt = ((hw != 0 && hw <= k_index) ? 1 : 0) | ((aw != 0 && aw <= k_index) ? 1 : 0) |
                   (list_overflow ? (list_overflow[0] | list_overflow[1]) : 0);
  const unsigned long long seen = stamp[blockIdx.x];
  __syncthreads();  // everybody has read the stamp before thread 0 replaces it
  if (halt != 0 || seen == this_stamp) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < v.n_entries) {
    const int i = v.e_index[e];
    double x[3], F[3];
    ext_centre<R>(p0, pl, i, x);
    ext_field_force<R>(v, e, p0, pl, x, s, F);
    auto p = mom[i];
    p.x += R(c_dt * F[0]), p.y += R(c_dt * F[1]), p.z += R(c_dt * F[2]);
    mom[i] = p;
  }
  if (threadIdx.x == 0) stamp[blockIdx.x] = this_stamp;
}

// ------------------------------------------------------------------ mythos_langevin_eval_external
// packed (N,3) centres -> the p0 words of a frame and zero momenta; momenta -> packed (N,3) forces
template <typename R>
__global__ void ext_eval_pack_kernel(int n, const R* __restrict__ c, typename Vec4T<R>::type* __restrict__ p0,
                                     typename Vec4T<R>::type* __restrict__ mom) {
  using V4 = typename Vec4T<R>::type;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  p0[i] = V4{c[3 * i], c[3 * i + 1], c[3 * i + 2], R(0)};
  mom[i] = V4{R(0), R(0), R(0), R(0)};
}
template <typename R>
__global__ void ext_eval_unpack_kernel(int n, const typename Vec4T<R>::type* __restrict__ mom, R* __restrict__ f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const auto m = mom[i];
  f[3 * i] = m.x, f[3 * i + 1] = m.y, f[3 * i + 2] = m.z;
}

// out[0] = -sum F.x of the constant forces, out[1] = the tether energy, out[2] = the sum-restraint energy (the rows of
// ext_group_kernel), and with n_out = kExtEnergies out[3 + kind] = the energy of the point terms of each kind at step
// count s; n_out = 3 writes the first three words only.  One workgroup, fixed order.
template <typename R>
__global__ __launch_bounds__(256) void ext_energy_kernel(int ext_count, const int* __restrict__ ext_index,
                                                         const typename Vec4T<R>::type* __restrict__ ext_force, const ExtFieldView v,
                                                         const typename Vec4T<R>::type* __restrict__ p0, double s, int n_out,
                                                         double* __restrict__ out) {
  __shared__ double red[4][256];
  double acc[4] = {0, 0, 0, 0};
  for (int e = threadIdx.x; e < ext_count; e += 256) {
    double x[3];
    ext_centre<R>(p0, nullptr, ext_index[e], x);
    const auto f = ext_force[e];
    acc[0] -= double(f.x) * x[0] + double(f.y) * x[1] + double(f.z) * x[2];
  }
  for (int t = threadIdx.x; t < v.n_tethers; t += 256) {
    double x[3];
    ext_centre<R>(p0, nullptr, v.t_index[t], x);
    const int mask = v.t_mask[t];
    double u = 0;
    for (int a = 0; a < 3; ++a) {
      const double d = ((mask >> a) & 1) ? x[a] - v.t_anchor[3 * t + a] : 0.0;
      u += d * d;
    }
    acc[1] += 0.5 * v.t_k[t] * u;
  }
  for (int g = threadIdx.x; g < v.n_groups; g += 256)
    if (v.g_kind[g] == EXT_GROUP_SUM) acc[2] += v.g_row[(size_t)g * kExtRow + 3];
  // point terms: acc[3] the strings', pt[0 .. 3] the traps', mutual traps', planes' and spheres'
  double pt[4] = {0, 0, 0, 0};
  for (int j = threadIdx.x; j < v.n_points; j += 256) {
    double x[3], F[3] = {0, 0, 0};
    ext_centre<R>(p0, nullptr, v.pt_particle[j], x);
    const double u = ext_point_term<R>(v, j, p0, nullptr, x, s, F);
    const int kind = v.pt_kind[j];
    acc[3] += kind == EXT_POINT_STRING ? u : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) pt[k] += kind == EXT_POINT_TRAP + k ? u : 0.0;
  }
  ext_block_sum(red, acc);
  ext_block_sum(red, pt);
  if (threadIdx.x == 0) {
    out[0] = acc[0], out[1] = acc[1], out[2] = acc[2];
    if (n_out == kExtEnergies) {
      out[3] = acc[3];
      for (int k = 0; k < 4; ++k) out[4 + k] = pt[k];
    }
  }
}

}  // namespace mythos
