// Duplex-mechanics observables of oxDNA trajectories, ONE workgroup per frame (duplex_obs.hip): what the reference's
// force-extension and stretch-torsion workflows measure per state, function by function:
//   [0] backbone distance  mythos/observables/diameter.py:23-46          mean over the listed base pairs of the distance of
//                                                                        their backbone sites (sigma_backbone and the
//                                                                        Angstrom factor are the caller's)
//   [1] extension          mythos/observables/stretch_torsion.py:77-95   |z| between the midpoints of two base pairs
//   [2] twist              mythos/observables/stretch_torsion.py:16-35   sum over quartets of the angle between the
//                                                                        base-base vectors of adjacent pairs, z dropped
//   [3] RMSD               mythos/observables/rmse.py:19-67              to a centred target after optimal superposition
// in oxDNA length units and radians.  Arithmetic in fp64 whatever the frames' precision; fixed-order reductions
// (block_sum of wave_ops.h; the sites, minimum image and clamp are those of observables.h).
#pragma once
#include "observables.h"

namespace mythos {

struct DuplexView {
  const int* bps = nullptr;       // [n_bp][2] hydrogen-bonded pairs of the backbone distance
  const int* quartets = nullptr;  // [n_q][2][2] adjacent base pairs ((a1, b1), (a2, b2)) of the twist
  const double* target = nullptr; // [n][3] centred target of the RMSD, or null
  int n_bp = 0, n_q = 0;
  int has_ends = 0;
  int ends[4] = {0, 0, 0, 0};     // a1, b1, a2, b2 of the extension
  SiteGeo geo;                    // site offsets and box (host_checks.h)
};

// The proper rotation that takes the centred frame x onto the target t in the least-squares sense, from
// S[3 a + b] = sum_i x_ia t_ib: Horn's unit quaternion, the eigenvector of the largest eigenvalue of the symmetric 4 x 4
// matrix below, by cyclic Jacobi sweeps (the rotations keep the eigenvectors orthonormal to rounding, so a frame that IS
// the target, rotated, comes back to it to ~1e-15).  The same rotation as the reference's SVD with its reflection fix
// (rmse.py:38-47: the sign of the smallest singular direction flipped when det < 0) wherever that is unique.
// rot: row-major, (rot x)_a = sum_b rot[3 a + b] x_b.
__host__ __device__ inline void horn_rotation(const double* S, double* rot) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      diag += a[p][p] * a[p][p];
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off += a[p][q] * a[p][q];
    }
    if (!(off > 1e-60 * diag)) break;  // (also: NaN input, all zeros)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double at = fabs(theta);
        const double t = (at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0))) * (theta < 0.0 ? -1.0 : 1.0);
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // columns p, q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq, a[k][q] = s * akp + c * akq;
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq, v[k][q] = s * vkp + c * vkq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // rows p, q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk, a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = a[q][p] = 0.0;
      }
    }
  }
  double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (a[k][k] > best) best = a[k][k], q0 = v[0][k], q1 = v[1][k], q2 = v[2][k], q3 = v[3][k];
  const double inv = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 *= inv, q1 *= inv, q2 *= inv, q3 *= inv;
  rot[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, rot[1] = 2 * (q1 * q2 - q0 * q3), rot[2] = 2 * (q1 * q3 + q0 * q2);
  rot[3] = 2 * (q1 * q2 + q0 * q3), rot[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, rot[5] = 2 * (q2 * q3 - q0 * q1);
  rot[6] = 2 * (q1 * q3 - q0 * q2), rot[7] = 2 * (q2 * q3 + q0 * q1), rot[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}

}  // namespace mythos
