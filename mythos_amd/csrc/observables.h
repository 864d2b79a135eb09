// Per-frame structural observables of oxDNA duplex trajectories, evaluated by ONE workgroup per frame:
// propeller twist, helical rise, pitch angle and the persistence-length partials (mean base-pair spacing and the
// autocorrelation of the local helical axes).  Launched from two places: mythos_observables_eval, and
// mythos_oxdna_energy_obs (behind its energy launch, while the frames are still in L2), so that a DiffTRe evaluation -
// energies, dU/dtheta and the observable it reweights - is one call.
//
// What is computed follows the reference function by function:
//   propeller twist  mythos/observables/propeller.py:19-71   mean over the listed base pairs of 180 - acos(a3_i . a3_j) [deg]
//   local axis       mythos/observables/base.py:24-45        unit vector between the base-site midpoints of two adjacent pairs
//   rise             mythos/observables/rise.py:21-39        (midpoint displacement) . axis, in Angstrom
//   pitch angle      mythos/observables/pitch.py:33-59       angle between the backbone-backbone vectors of the two pairs
//                                                            after projecting out the axis [rad]
//   persistence      mythos/observables/persistence_length.py:47-91  C(d) = mean_i l_i . l_(i+d), <l0>; skip_ends drops two
//                                                            quartets at either end
// Arithmetic in fp64 whatever the state's precision (a few hundred flops per base pair); fixed-order reductions.
//
// Output row of a frame, `width` = 4 + n_corr doubles:
//   [0] propeller twist (deg)  [1] rise (Angstrom)  [2] pitch angle (rad)  [3] <l0> (oxDNA length units)  [4 + d] C(d)
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"
#include "host_checks.h"
#include "oxdna_math.h"
#include "wave_ops.h"

namespace mythos {

constexpr double kAngstromPerOxdnaLength = 8.518;  // mythos/utils/units.py:5-8

struct ObsView {
  const int* bps = nullptr;       // [n_bp][2] hydrogen-bonded pairs of the propeller twist
  const int* quartets = nullptr;  // [n_q][2][2] adjacent base pairs ((a1, b1), (a2, b2))
  double* axis = nullptr;         // scratch [frames][n_q][3]: the local axes of a frame (autocorrelation input)
  int n_bp = 0, n_q = 0;
  int skip = 0;                   // quartets dropped at either end for the persistence-length partials (0 or 2)
  int n_corr = 0;                 // n_q - 2 * skip (>= 0)
  int width = 0;                  // 4 + n_corr; 0 = no observables
  SiteGeo geo;                    // site offsets and box (host_checks.h)
};

using D3 = V3<double>;

// The sites of a nucleotide (SiteGeo) from its centre and axes, and the minimum image of a displacement between sites:
// the one statement of them for every frame-observable kernel.
__device__ __forceinline__ D3 base_site(const SiteGeo& g, D3 c, D3 a1) { return c + g.g_hb * a1; }
__device__ __forceinline__ D3 back_site(const SiteGeo& g, D3 c, D3 a1, D3 a2, D3 a3) {
  return c + g.g_k1 * a1 + g.g_k2 * (g.model == 3 ? a3 : a2);  // oxRNA2: second coefficient on a3 (rna2/nucleotide.py:56)
}
__device__ __forceinline__ D3 obs_min_image(D3 d, const SiteGeo& g) {
  if (g.box_on) {
    d.x -= g.box[0] * rint(d.x / g.box[0]);
    d.y -= g.box[1] * rint(d.y / g.box[1]);
    d.z -= g.box[2] * rint(d.z / g.box[2]);
  }
  return d;
}

__device__ __forceinline__ double obs_clamp(double c) { return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c); }

// centre and axes of nucleotide i of one frame, in double whatever the frame's precision
template <typename R>
__device__ __forceinline__ D3 obs_centre(const R* __restrict__ center, int i) {
  return D3{(double)center[3 * i], (double)center[3 * i + 1], (double)center[3 * i + 2]};
}
template <typename R>
__device__ __forceinline__ void obs_axes(const R* __restrict__ quat, int i, D3& a1, D3& a2, D3& a3) {
  quat_axes<double>(quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3], a1, a2, a3);
}

// center [n][3], quat [n][4] of ONE frame; out [width]; axis scratch [n_q][3] of this frame.
template <typename R>
__device__ __forceinline__ void frame_observables(const ObsView& v, const R* __restrict__ center, const R* __restrict__ quat,
                                                  double* __restrict__ out, double* __restrict__ axis, double* red) {
  const SiteGeo& g = v.geo;
  // ---- propeller twist
  double pt = 0.0;
  for (int k = threadIdx.x; k < v.n_bp; k += blockDim.x) {
    D3 a1, a2, n1, n2;
    obs_axes(quat, v.bps[2 * k], a1, a2, n1);
    obs_axes(quat, v.bps[2 * k + 1], a1, a2, n2);
    pt += 180.0 - acos(obs_clamp(dot(n1, n2))) * (180.0 / kPi);
  }
  pt = block_sum(pt, red);
  // ---- quartets: axis, rise, pitch angle, spacing
  double rise = 0.0, ang = 0.0, l0 = 0.0;
  for (int k = threadIdx.x; k < v.n_q; k += blockDim.x) {
    const int ia1 = v.quartets[4 * k], ib1 = v.quartets[4 * k + 1], ia2 = v.quartets[4 * k + 2], ib2 = v.quartets[4 * k + 3];
    D3 x1, y1, z1, x2, y2, z2, x3, y3, z3, x4, y4, z4;
    obs_axes(quat, ia1, x1, y1, z1), obs_axes(quat, ib1, x2, y2, z2), obs_axes(quat, ia2, x3, y3, z3), obs_axes(quat, ib2, x4, y4, z4);
    const D3 c1 = obs_centre(center, ia1), c2 = obs_centre(center, ib1), c3 = obs_centre(center, ia2), c4 = obs_centre(center, ib2);
    const D3 m1 = 0.5 * (base_site(g, c1, x1) + base_site(g, c2, x2));
    const D3 m2 = 0.5 * (base_site(g, c3, x3) + base_site(g, c4, x4));
    const D3 dr = obs_min_image(m2 - m1, g);
    const double norm = sqrt(dot(dr, dr));
    const D3 ax = (1.0 / norm) * dr;
    axis[3 * k] = ax.x, axis[3 * k + 1] = ax.y, axis[3 * k + 2] = ax.z;
    rise += dot(dr, ax) * kAngstromPerOxdnaLength;
    if (k >= v.skip && k < v.n_q - v.skip) l0 += norm;
    // backbone-backbone vectors of the two pairs, helical component removed
    D3 bb1 = obs_min_image(back_site(g, c2, x2, y2, z2) - back_site(g, c1, x1, y1, z1), g);
    D3 bb2 = obs_min_image(back_site(g, c4, x4, y4, z4) - back_site(g, c3, x3, y3, z3), g);
    bb1 = obs_min_image(bb1 - dot(ax, bb1) * ax, g);
    bb2 = obs_min_image(bb2 - dot(ax, bb2) * ax, g);
    const double c = dot(bb1, bb2) / sqrt(dot(bb1, bb1) * dot(bb2, bb2));
    ang += acos(obs_clamp(c));
  }
  rise = block_sum(rise, red);
  ang = block_sum(ang, red);
  l0 = block_sum(l0, red);  // (its barriers also publish the axes of this frame to the whole workgroup)
  __threadfence_block();
  if (threadIdx.x == 0) {
    out[0] = v.n_bp > 0 ? pt / v.n_bp : 0.0;
    out[1] = v.n_q > 0 ? rise / v.n_q : 0.0;
    out[2] = v.n_q > 0 ? ang / v.n_q : 0.0;
    out[3] = v.n_corr > 0 ? l0 / v.n_corr : 0.0;
  }
  // ---- autocorrelation of the kept axes: C(d) = mean over the n_corr - d pairs at lag d
  const double* a = axis + 3 * v.skip;
  for (int d = threadIdx.x; d < v.n_corr; d += blockDim.x) {
    double s = 0.0;
    for (int i = 0; i + d < v.n_corr; ++i)
      s += a[3 * i] * a[3 * (i + d)] + a[3 * i + 1] * a[3 * (i + d) + 1] + a[3 * i + 2] * a[3 * (i + d) + 2];
    out[4 + d] = s / (v.n_corr - d);
  }
}

}  // namespace mythos

// host side of an observable set (observables.hip)
struct mythos_obs {
  int n = 0, dtype = 0, device = 0;
  mythos::ObsView view;     // device pointers filled in; view.axis is (re)allocated per call
  mythos::DeviceBuf<int> d_bps, d_quartets;
  mythos::DeviceBuf<double> d_axis;
  ~mythos_obs() { (void)hipSetDevice(device); }  // the members free themselves, on the set's device
};

namespace mythos {
// makes sure the axis scratch covers n_frames and returns the view to pass to observables_launch
int obs_view_for(mythos_obs* o, int n_frames, ObsView* out);
// the stand-alone kernel on frames f0 .. f0 + nf of the arrays obs_view_for sized the scratch for: center, quat, out and
// the view's axis scratch are those of frame 0, the launch offsets all four
int observables_launch(mythos_obs* o, ObsView view, const void* center, const void* quat, int f0, int nf, double* out,
                       hipStream_t stream);
}  // namespace mythos
