// External forces of the MARTINI Langevin integrator (mythos_martini_langevin_set_restraints): harmonic position
// restraints (GROMACS' [ position_restraints ] funct 1), flat-bottomed position restraints (funct 2: sphere, cylinder,
// layer, each invertible) and pull coordinates between the centres of mass of two groups (GROMACS' pull code: umbrella and
// constant-force, geometries distance and direction, an absolute reference, pbcatom).  The structure is ext_field.h's, on
// the MARTINI frame: positions x, y, z of a bead (stride 4 in a frame, 3 in a caller's array), vel = (v, 1 / m).
// Units nm, ps, kJ/mol, amu; every sum in double, in both precisions.
//
// Laws (d: the distance the shape names, X the reference, t = s dt with s the step count of the frame the force is taken at):
//   position restraint   U = 1/2 sum_a k_a (x_a - X_a)^2
//   flat-bottom          U = 1/2 k (d - r)^2 where d > r (invert: where d < r); sphere d = |x - X|, cylinder(axis) the distance
//                        from the axis through X, layer(axis) d = |x_a - X_a|; no force at d = 0
//   pull coordinate      D = X_B - X_A (COMs weighted with the integrator's masses; A = -1: X_A = origin), minimum image in
//                        the replica's box when periodic; distance: xi = |D| over the axes of dim, no force at xi = 0;
//                        direction: xi = D . n.  umbrella U = 1/2 k (xi - init - rate t)^2, constant-force U = k xi.
//                        Member j of B gets -U'(xi) e m_j / M_B, member j of A +U'(xi) e m_j / M_A.
// Coordinates are taken as the frame stores them - the integrator never folds one into the box.  A group with a pbc_ref
// bead takes its members at their minimum image relative to that bead.
//
// Two launches in the queue slot in front of step launch k (martini_md_step_kernel takes the force at x_k and applies
// (kick_close + do_step / 2) dt F / m, writes nothing when it halts and never folds a coordinate):
//   mr_com_kernel   one workgroup of 256 per (frame, replica, group): members strided over the threads, a fixed-order LDS
//                   tree, sum m x / M and M in double into the group's row.  A pure function of the positions: no stamp.
//   mr_kick_kernel  one thread per (replica, restrained bead): the bead's terms in the order of its list, added in double,
//                   one kick of its velocity.  A pull coordinate's xi and U' are recomputed by the thread from the two COM
//                   rows through mr_pull_eval - the one evaluation every path uses.  No atomics; no two threads write one
//                   velocity.  Every workgroup follows ext_kick_kernel's protocol (langevin_frame.h) with a stamp word of
//                   its own: it skips exactly when step launch k skips, reads the stamp in front of a barrier, and thread 0
//                   replaces it behind the kick.
#pragma once
#include <hip/hip_runtime.h>

#include "martini_restraint_checks.h"

namespace mythos {

constexpr int kMrRow = 4;       // doubles per group row: COM.xyz, M
constexpr int kMrEnergies = 4;  // position, flat-bottom, umbrella, constant-force

// device arrays of one set (MmRestraints owns them); integer topology is one replica's, parameters are per replica
struct MrView {
  int n = 0, n_rep = 1;  // beads of one replica, replicas
  int n_posres = 0, n_flat = 0, n_groups = 0, n_pull = 0, n_entries = 0;
  const int* pr_index = nullptr;
  const double* pr_k = nullptr;
  const double* pr_ref = nullptr;
  const int* fb_index = nullptr;
  const int* fb_flags = nullptr;
  const double* fb_param = nullptr;
  const int* g_first = nullptr;
  const int* g_member = nullptr;
  const int* g_pbc_ref = nullptr;
  const int* p_flags = nullptr;
  const int* p_groups = nullptr;
  const double* p_param = nullptr;
  const double* boxes = nullptr;  // [n_rep][3] (ones when the set takes no minimum image)
  const double* mass = nullptr;   // [n] the integrator's masses
  const int* e_index = nullptr;   // [n_entries] restrained beads, ascending
  const int* e_first = nullptr;   // [n_entries + 1]
  const int* e_term = nullptr;    // mr_term_code
  double dt = 0.0;
};

__device__ inline void mr_block_sum4(double (&red)[4][256], double (&v)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = red[k][0];
  __syncthreads();
}

// rows[(frame * n_rep + rep) * n_groups + g] <- COM and mass of group g.  pos: frame-major, replica-major, `stride` reals
// per bead.  Grid: n_frames * n_rep * n_groups.
template <typename R>
__global__ __launch_bounds__(256) void mr_com_kernel(const MrView v, const R* __restrict__ pos, int stride, double* __restrict__ rows) {
  __shared__ double red[4][256];
  const int g = blockIdx.x % v.n_groups, fr = blockIdx.x / v.n_groups;  // fr: frame * n_rep + rep
  const int rep = fr % v.n_rep;
  const R* x = pos + (size_t)fr * v.n * stride;
  const double* L = v.boxes + 3 * (size_t)rep;
  const int b = v.g_first[g], e = v.g_first[g + 1];
  const int pr = v.g_pbc_ref[g];
  double ref[3] = {0, 0, 0};
  if (pr >= 0)
    for (int a = 0; a < 3; ++a) ref[a] = double(x[(size_t)pr * stride + a]);
  double acc[4] = {0, 0, 0, 0};
  for (int m = b + (int)threadIdx.x; m < e; m += 256) {
    const int i = v.g_member[m];
    const double w = v.mass[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double q = double(x[(size_t)i * stride + a]);
      if (pr >= 0) {
        const double d = q - ref[a];
        q = ref[a] + (d - L[a] * rint(d / L[a]));
      }
      acc[a] += w * q;
    }
    acc[3] += w;
  }
  mr_block_sum4(red, acc);
  if (threadIdx.x == 0) {
    double* row = rows + (size_t)blockIdx.x * kMrRow;
    row[0] = acc[0] / acc[3], row[1] = acc[1] / acc[3], row[2] = acc[2] / acc[3], row[3] = acc[3];
  }
}

struct MrPull {
  double xi, u, du;  // the coordinate, its energy and U'(xi)
  double e[3];       // d xi / d X_B (zero where the coordinate has no direction)
};

// Pull coordinate p of replica rep from the COM rows of that replica (rows: its n_groups rows) at time t, with the
// parameters of row prow - rep itself everywhere but in the window-exchange event, which evaluates a configuration under
// another replica's window; minimum images are always the configuration's, in the box of rep.  The one evaluation of the
// law: the kick, the energy sum, the stored-frames launch and the exchange event all come here.
__device__ inline MrPull mr_pull_eval(const MrView& v, int p, int rep, int prow, const double* __restrict__ rows, double t) {
  const int f = v.p_flags[p], A = v.p_groups[2 * p], B = v.p_groups[2 * p + 1];
  const double* q = v.p_param + ((size_t)prow * v.n_pull + p) * kMrPullParams;
  const double* L = v.boxes + 3 * (size_t)rep;
  const double* xb = rows + (size_t)B * kMrRow;
  double D[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double xa = A >= 0 ? rows[(size_t)A * kMrRow + a] : q[6 + a];
    D[a] = xb[a] - xa;
    if (mr_pull_periodic(f)) D[a] -= L[a] * rint(D[a] / L[a]);
  }
  MrPull r;
  if (mr_pull_direction(f)) {
    r.xi = D[0] * q[3] + D[1] * q[4] + D[2] * q[5];
    r.e[0] = q[3], r.e[1] = q[4], r.e[2] = q[5];
  } else {
    const int dim = mr_pull_dim(f);
    double s = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((dim >> a) & 1)) D[a] = 0.0;
      s += D[a] * D[a];
    }
    r.xi = sqrt(s);
    const double inv = r.xi > 0.0 ? 1.0 / r.xi : 0.0;
    r.e[0] = D[0] * inv, r.e[1] = D[1] * inv, r.e[2] = D[2] * inv;
  }
  if (mr_pull_constant(f)) {
    r.u = q[0] * r.xi, r.du = q[0];
  } else {
    const double dev = r.xi - q[1] - q[2] * t;
    r.u = 0.5 * q[0] * dev * dev, r.du = q[0] * dev;
  }
  return r;
}

// position restraint t with the reference of parameter row prow (the bead's own replica, or in the window-exchange event
// the other window's row) on a bead at x: its force added to F, its energy returned
__device__ inline double mr_posres_term(const MrView& v, int t, int prow, const double (&x)[3], double (&F)[3]) {
  const double* k = v.pr_k + 3 * (size_t)t;
  const double* X = v.pr_ref + ((size_t)prow * v.n_posres + t) * 3;
  double u = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = x[a] - X[a];
    F[a] -= k[a] * d;
    u += k[a] * d * d;
  }
  return 0.5 * u;
}

// flat-bottom term t with the parameters of row prow on a bead at x
__device__ inline double mr_flat_term(const MrView& v, int t, int prow, const double (&x)[3], double (&F)[3]) {
  const int f = v.fb_flags[t], shape = mr_flat_shape(f), axis = mr_flat_axis(f);
  const double* q = v.fb_param + ((size_t)prow * v.n_flat + t) * kMrFlatParams;
  double rho[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    rho[a] = x[a] - q[2 + a];
    if (shape == MR_FLAT_CYLINDER && a == axis) rho[a] = 0.0;
    if (shape == MR_FLAT_LAYER && a != axis) rho[a] = 0.0;
  }
  const double d = sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]);
  const bool on = mr_flat_invert(f) ? d < q[1] : d > q[1];
  if (!on) return 0.0;
  const double s = d - q[1];
  if (d > 0.0) {
    const double g = -q[0] * s / d;
    F[0] += g * rho[0], F[1] += g * rho[1], F[2] += g * rho[2];
  }
  return 0.5 * q[0] * s * s;
}

// v_i += factor F_i(x) on the frame step launch k is about to read, for every restrained bead of every replica;
// factor = c_dt / m_i, or 1 when c_dt < 0 (the evaluation path: forces into zeroed velocities).  rows: the COM rows of
// mr_com_kernel on the same positions, [n_rep][n_groups].  s: the step count of that frame.  Protocol: see the head.
template <typename R, typename V4>
__global__ __launch_bounds__(256) void mr_kick_kernel(const MrView v, const R* __restrict__ pos, int stride, const double* __restrict__ rows,
                                                      double c_dt, double s, V4* __restrict__ vel, const int* __restrict__ flags,
                                                      const int* __restrict__ list_overflow, int k_index,
                                                      unsigned long long this_stamp, unsigned long long* __restrict__ stamp) {
  const int hw = flags[1];
  const int halt = ((hw != 0 && hw <= k_index) ? 1 : 0) | (list_overflow ? (list_overflow[0] | list_overflow[1]) : 0);
  const unsigned long long seen = stamp[blockIdx.x];
  __syncthreads();  // everybody has read the stamp before thread 0 replaces it
  if (halt != 0 || seen == this_stamp) return;
  const long long ge = (long long)blockIdx.x * 256 + threadIdx.x;
  if (ge < (long long)v.n_rep * v.n_entries) {
    const int rep = (int)(ge / v.n_entries), e = (int)(ge % v.n_entries);
    const int il = v.e_index[e];
    const size_t i = (size_t)rep * v.n + il;
    const double x[3] = {double(pos[i * stride]), double(pos[i * stride + 1]), double(pos[i * stride + 2])};
    const double* rw = rows + (size_t)rep * v.n_groups * kMrRow;
    const double t = s * v.dt;
    double F[3] = {0, 0, 0};
    for (int c = v.e_first[e]; c < v.e_first[e + 1]; ++c) {
      const int code = v.e_term[c], kind = code & 3, idx = code >> 3;
      if (kind == MR_TERM_POSRES) {
        (void)mr_posres_term(v, idx, rep, x, F);
      } else if (kind == MR_TERM_FLAT) {
        (void)mr_flat_term(v, idx, rep, x, F);
      } else {
        const int side = (code >> 2) & 1;
        const MrPull pc = mr_pull_eval(v, idx, rep, rep, rw, t);
        const int g = v.p_groups[2 * idx + side];
        const double w = (side ? -pc.du : pc.du) * (v.mass[il] / rw[(size_t)g * kMrRow + 3]);
        F[0] += w * pc.e[0], F[1] += w * pc.e[1], F[2] += w * pc.e[2];
      }
    }
    const double fac = c_dt < 0.0 ? 1.0 : c_dt / v.mass[il];
    V4 p = vel[i];
    p.x += R(fac * F[0]), p.y += R(fac * F[1]), p.z += R(fac * F[2]);
    vel[i] = p;
  }
  if (threadIdx.x == 0) stamp[blockIdx.x] = this_stamp;
}

// energies[rep][kMrEnergies] and xi[rep][n_pull] of the set at pos (one frame), from the COM rows.  One workgroup per replica.
template <typename R>
__global__ __launch_bounds__(256) void mr_energy_kernel(const MrView v, const R* __restrict__ pos, int stride, const double* __restrict__ rows,
                                                        double s, double* __restrict__ energies, double* __restrict__ xi) {
  __shared__ double red[4][256];
  const int rep = blockIdx.x;
  const R* x0 = pos + (size_t)rep * v.n * stride;
  const double* rw = rows + (size_t)rep * v.n_groups * kMrRow;
  double acc[4] = {0, 0, 0, 0};
  for (int t = threadIdx.x; t < v.n_posres; t += 256) {
    const size_t i = v.pr_index[t];
    const double x[3] = {double(x0[i * stride]), double(x0[i * stride + 1]), double(x0[i * stride + 2])};
    double F[3] = {0, 0, 0};
    acc[0] += mr_posres_term(v, t, rep, x, F);
  }
  for (int t = threadIdx.x; t < v.n_flat; t += 256) {
    const size_t i = v.fb_index[t];
    const double x[3] = {double(x0[i * stride]), double(x0[i * stride + 1]), double(x0[i * stride + 2])};
    double F[3] = {0, 0, 0};
    acc[1] += mr_flat_term(v, t, rep, x, F);
  }
  for (int p = threadIdx.x; p < v.n_pull; p += 256) {
    const MrPull pc = mr_pull_eval(v, p, rep, rep, rw, s * v.dt);
    acc[mr_pull_constant(v.p_flags[p]) ? 3 : 2] += pc.u;
    if (xi) xi[(size_t)rep * v.n_pull + p] = pc.xi;
  }
  mr_block_sum4(red, acc);
  if (threadIdx.x == 0)
    for (int k = 0; k < kMrEnergies; ++k) energies[(size_t)rep * kMrEnergies + k] = acc[k];
}

// xi of every (frame, replica, coordinate) of a stored trajectory from its COM rows [n_frames][n_rep][n_groups]
__global__ __launch_bounds__(256) void mr_pull_values_kernel(const MrView v, int n_frames, const double* __restrict__ rows,
                                                             double* __restrict__ out) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= (long long)n_frames * v.n_rep * v.n_pull) return;
  const int p = (int)(j % v.n_pull);
  const long long fr = j / v.n_pull;
  const int rep = (int)(fr % v.n_rep);
  out[j] = mr_pull_eval(v, p, rep, rep, rows + (size_t)fr * v.n_groups * kMrRow, 0.0).xi;
}

// caller's (n_all, 3) positions need no packing (stride 3); the velocities of the scratch frame -> (n_all, 3) forces
template <typename R, typename V4>
__global__ void mr_unpack_force_kernel(int n_all, const V4* __restrict__ vel, R* __restrict__ f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_all) return;
  const V4 m = vel[i];
  f[3 * (size_t)i] = m.x, f[3 * (size_t)i + 1] = m.y, f[3 * (size_t)i + 2] = m.z;
}

}  // namespace mythos
