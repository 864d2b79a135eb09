// Lateral pressure profile of stored MARTINI frames: the diagonal virial of every frame resolved in slabs along z, every
// frame of a trajectory in one call (mythos_martini_stress_profile; definitions in DESIGN section 3.5q).  The reference has
// no such observable; its GROMACS runs report one pressure per frame, never its profile.
//
// Per-bead virial.  Bead i of a frame gets w_i = (w_ix, w_iy, w_iz), martini_pressure_kernel's decomposition term for term
// (martini_npt.inc): an LJ pair, a bond, a reaction-field pair and an excluded reaction-field pair give -1/2 g dx_d^2 to
// either bead (g = (dV/dr) / r), an angle -u_d dU/dx_id to its first and -v_d dU/dx_kd to its last bead, nothing to its
// centre; all over minimum-image vectors, from the term functions of martini_terms.h.  sum_i w_i is the W of
// mythos_martini_langevin_pressure for the same configuration.  A Harasima-type assignment: the share sits at the bead's
// own z.  Its lateral components are what the profile is for; P_zz(z) of this contour is not constant in z, only its sum
// over the slabs is physical.
//
// Four kernels per chunk of frames, none with an atomic:
//   stress_pair_kernel    the non-bonded part on lj_tile_sweep (martini_internal.h; no neighbour list for stored frames),
//                         the partner range split over blockIdx.y as in the energy kernels.  LJ, and with charges the
//                         reaction-field pair and excluded-pair terms: the sweep meets every excluded partner once, which is
//                         the pressure kernel's duplicate-partner rule.  A tile's sum in R, the tiles' sums in double; one
//                         row of 3 (6 with charges) doubles per bead and partner range.
//   stress_mid_kernel     (centred profiles) the frame's midpoint: the mean stored z of the centre selection, summed as
//                         membrane_kernel sums its midpoint.
//   stress_bonded_kernel  bonds and angles gathered per bead from the incidence lists, as martini_bonded_kernel gathers
//                         them, and the bead's slab, in double from the position promoted on load.
//   stress_slab_kernel    one wavefront per slab and frame: lane l walks the beads l, l + 64, ... in index order, adds the
//                         shares of those that lie in the slab - the partner ranges of a bead in range order -, then the
//                         wavefront's tree.  The order of every addition depends on n and the bead's slab alone.
// Reproducibility: the partner split depends on n only (stress_n_js), never on the number of frames, and a frame's row is
// made from that frame's data alone - the same bits alone, in any batch, across launch chunks and call after call.  The
// slab sums keep full double precision (no fixed-point scale), which is why the fixed-order reduction was chosen over
// integer LDS atomics; it costs F n_bins n / 64 bin reads, small against the F n^2 pair sweep.
// The un-split W of a slab is ((lj + bond) + angle) + coulomb of the by_term columns, in that order: bitwise the same.
// Scratch per frame: n (8 n_js (3 or 6) + 52) bytes; frames go in chunks of at most 65 535 (grid.z) and 512 MB.
#include <algorithm>
#include <cmath>
#include <string>

#include "martini_internal.h"
#include "stress_profile_checks.h"
#include "wave_ops.h"

namespace mythos {

constexpr int kSpBlock = 256;
constexpr int kSpWaves = kSpBlock / 64;

// partner ranges of the sweep: a function of the tile count alone (a frame's sums must not depend on the batch it is in)
static int stress_n_js(int n_tiles) { return std::min(n_tiles, std::max(1, 192 / std::max(1, n_tiles))); }

template <typename R, bool COUL>
__global__ __launch_bounds__(kLjBlock) void stress_pair_kernel(
    int n, const R* __restrict__ pos, const R* __restrict__ box, const int* __restrict__ types, const R* __restrict__ sigma,
    const R* __restrict__ eps, const R* __restrict__ charge, const int* __restrict__ excl, MartiniConst<R> K, RfConst<R> C,
    int n_tiles, double* __restrict__ part /* [frame][js][n][3 or 6] */) {
  constexpr int CP = COUL ? 6 : 3;
  extern __shared__ unsigned char smem_raw[];
  const int tt = K.n_types * K.n_types;
  R* s_sig2 = reinterpret_cast<R*>(smem_raw);
  R* s_eps = s_sig2 + tt;
  R* s_x = s_eps + tt;
  const int frame = blockIdx.z;
  const int js = blockIdx.y, n_js = gridDim.y;
  const int i = blockIdx.x * kLjBlock + threadIdx.x;
  for (int k = threadIdx.x; k < tt; k += kLjBlock) {
    const R sg = sigma[k];
    s_sig2[k] = sg * sg;
    s_eps[k] = eps[k];
  }
  R qi = 0;
  (void)qi;
  if constexpr (COUL) qi = i < n ? C.pref * charge[i] : R(0);
  R lx = 0, ly = 0, lz = 0, cx = 0, cy = 0, cz = 0;  // one tile in R, the tiles in double
  double wl[3] = {0.0, 0.0, 0.0}, wc[3] = {0.0, 0.0, 0.0};
  (void)cx, (void)cy, (void)cz, (void)wc;
  lj_tile_sweep<R>(
      n, pos + (size_t)frame * n * 3, box + (size_t)frame * 3, types, excl, K.rc2, K.n_types, n_tiles, s_x,
      [&](int tp, int j, bool excluded, R dx, R dy, R dz, R r2) {
        if (!excluded) {
          const R h = R(-0.5) * lj_pair(s_sig2[tp], s_eps[tp], r2).g;
          lx += h * dx * dx, ly += h * dy * dy, lz += h * dz * dz;
        }
        if constexpr (COUL) {
          const R qq = qi * charge[j];
          if (qq != R(0)) {
            const RfPair<R> t = excluded ? rf_excluded(r2, C.k_rf, C.c_rf) : rf_pair(r2, C.k_rf, C.c_rf);
            const R hc = R(-0.5) * qq * t.g;
            cx += hc * dx * dx, cy += hc * dy * dy, cz += hc * dz * dz;
          }
        }
      },
      [&] {
        wl[0] += double(lx), wl[1] += double(ly), wl[2] += double(lz);
        lx = 0, ly = 0, lz = 0;
        if constexpr (COUL) {
          wc[0] += double(cx), wc[1] += double(cy), wc[2] += double(cz);
          cx = 0, cy = 0, cz = 0;
        }
      });
  if (i < n) {
    double* __restrict__ o = part + (((size_t)frame * n_js + js) * n + i) * CP;
    o[0] = wl[0], o[1] = wl[1], o[2] = wl[2];
    if constexpr (COUL) o[3] = wc[0], o[4] = wc[1], o[5] = wc[2];
  }
}

// mid[frame] = mean stored z of the centre selection: thread-strided partials in double, then block_sum
template <typename R>
__global__ __launch_bounds__(kSpBlock) void stress_mid_kernel(int n, int n_sel, const int* __restrict__ sel, const R* __restrict__ pos,
                                                              double* __restrict__ mid) {
  __shared__ double s_w[kSpWaves];
  const int frame = blockIdx.x;
  const R* __restrict__ p = pos + (size_t)frame * n * 3;
  double zs = 0.0;
  for (int k = threadIdx.x; k < n_sel; k += kSpBlock) zs += double(p[3 * (size_t)sel[k] + 2]);
  const double s = block_sum(zs, s_w);
  if (threadIdx.x == 0) mid[frame] = s / double(n_sel);
}

// the slab of a stored z, in double; always inside [0, n_bins) whatever z and lz hold
__device__ __forceinline__ int stress_slab(double z, double lz, const double* __restrict__ mid, int frame, int n_bins) {
  double s;
  if (mid) {
    const double t = (z - mid[frame]) / lz;
    const double u = t - floor(t + 0.5);
    s = (u + 0.5) * double(n_bins);
  } else {
    const double t = z / lz;
    const double u = t - floor(t);
    s = u * double(n_bins);
  }
  const int b = (int)floor(s);
  return max(0, min(n_bins - 1, b));
}

// bonded[frame][i] = bond share xyz | angle share xyz of bead i; bin[frame][i] = its slab
template <typename R>
__global__ __launch_bounds__(kSpBlock) void stress_bonded_kernel(
    int n, const R* __restrict__ pos, const R* __restrict__ box, const int* __restrict__ bead_bonds, const int* __restrict__ bead_angles,
    const int* __restrict__ bonds, const R* __restrict__ bond_k, const R* __restrict__ bond_r0, const int* __restrict__ angles,
    const R* __restrict__ angle_k, const R* __restrict__ angle_t0, int angle_kind, const double* __restrict__ mid, int n_bins,
    double* __restrict__ bonded, int* __restrict__ bin) {
  const int frame = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R* __restrict__ p = pos + (size_t)frame * n * 3;
  const R l[3] = {box[(size_t)frame * 3], box[(size_t)frame * 3 + 1], box[(size_t)frame * 3 + 2]};
  const R il[3] = {R(1) / l[0], R(1) / l[1], R(1) / l[2]};
  R wb[3] = {0, 0, 0}, wa[3] = {0, 0, 0};
  for (int s = 0; s < kMaxBeadBonds; ++s) {
    const int ent = bead_bonds[(size_t)i * kMaxBeadBonds + s];
    if (ent < 0) break;
    const int b = ent >> 1, side = ent & 1;
    const int o = bonds[2 * b + (1 - side)];
    R d[3], r2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d[k] = wrap(p[3 * (size_t)i + k] - p[3 * (size_t)o + k], l[k], il[k]);
      r2 += d[k] * d[k];
    }
    const R h = R(-0.5) * bond_term(r2, bond_k[b], bond_r0[b]).c;
#pragma unroll
    for (int k = 0; k < 3; ++k) wb[k] += h * d[k] * d[k];
  }
  for (int s = 0; s < kMaxBeadAngles; ++s) {
    const int ent = bead_angles[(size_t)i * kMaxBeadAngles + s];
    if (ent < 0) break;
    const int a = ent >> 2, role = ent & 3;  // 0: first bead, 1: centre, 2: last bead
    if (role == 1) continue;                 // (the centre's arms are counted at their far ends)
    const int bi = angles[3 * a], bj = angles[3 * a + 1], bk = angles[3 * a + 2];
    R u[3], v[3], u2 = 0, v2 = 0, uv = 0;  // u = r_i - r_j, v = r_k - r_j
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u[k] = wrap(p[3 * (size_t)bi + k] - p[3 * (size_t)bj + k], l[k], il[k]);
      v[k] = wrap(p[3 * (size_t)bk + k] - p[3 * (size_t)bj + k], l[k], il[k]);
      u2 += u[k] * u[k], v2 += v[k] * v[k], uv += u[k] * v[k];
    }
    const AngleGeom<R> ag = angle_geometry(u, v, u2, v2, uv, angle_kind);
    R ref = angle_t0[a];
    if (angle_kind == 0) {
      if constexpr (sizeof(R) == 4) ref = cosf(ref); else ref = cos(ref);
    }
    const R h = -angle_term(angle_kind, ag, angle_k[a], ref).dEdc;
    // (times this bead's own arm)
#pragma unroll
    for (int k = 0; k < 3; ++k) wa[k] += h * angle_role_grad(role, ag, u[k], v[k]) * (role == 0 ? u[k] : v[k]);
  }
  double* __restrict__ o = bonded + ((size_t)frame * n + i) * 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = double(wb[k]), o[3 + k] = double(wa[k]);
  bin[(size_t)frame * n + i] = stress_slab(double(p[3 * (size_t)i + 2]), double(box[(size_t)frame * 3 + 2]), mid, frame, n_bins);
}

// row[frame0 + frame][slab] = count, W (4 doubles), or count, W_lj, W_bond, W_angle, W_coulomb (13 doubles)
template <bool COUL>
__global__ __launch_bounds__(kSpBlock) void stress_slab_kernel(int n, int n_js, int n_bins, int by_term, const double* __restrict__ part,
                                                               const double* __restrict__ bonded, const int* __restrict__ bin, int frame0,
                                                               double* __restrict__ out) {
  constexpr int CP = COUL ? 6 : 3;
  constexpr int NV = 1 + 3 * kStressTerms;
  const int frame = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int* __restrict__ fb = bin + (size_t)frame * n;
  const double* __restrict__ fbo = bonded + (size_t)frame * n * 6;
  const double* __restrict__ fp = part + (size_t)frame * n_js * n * CP;
  const int width = by_term ? MYTHOS_STRESS_ROW_BY_TERM : MYTHOS_STRESS_ROW;
  for (int slab = blockIdx.x * kSpWaves + wave; slab < n_bins; slab += gridDim.x * kSpWaves) {  // (uniform per wavefront)
    double v[NV];  // count | lj | bond | angle | coulomb
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = 0.0;
    for (int i = lane; i < n; i += 64) {
      if (fb[i] != slab) continue;
      v[0] += 1.0;
      for (int js = 0; js < n_js; ++js) {
        const double* __restrict__ q = fp + ((size_t)js * n + i) * CP;
        v[1] += q[0], v[2] += q[1], v[3] += q[2];
        if constexpr (COUL) v[10] += q[3], v[11] += q[4], v[12] += q[5];
      }
      const double* __restrict__ q = fbo + (size_t)i * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) v[4 + c] += q[c];
    }
#pragma unroll
    for (int c = 0; c < NV; ++c)
      for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, 64);
    if (lane == 0) {
      double* __restrict__ row = out + ((size_t)(frame0 + frame) * n_bins + slab) * width;
      if (by_term) {
#pragma unroll
        for (int c = 0; c < NV; ++c) row[c] = v[c];
      } else {
        row[0] = v[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) row[1 + d] = ((v[1 + d] + v[4 + d]) + v[7 + d]) + v[10 + d];
      }
    }
  }
}

template <typename R>
static int stress_profile_typed(mythos_martini* m, const R* pos, const R* box, int n_frames, int n_center, int n_bins, bool by_term,
                                double* out, hipStream_t st) {
  const int n = m->n;
  const int nbx = (n + kLjBlock - 1) / kLjBlock, n_js = stress_n_js(nbx), nbb = (n + kSpBlock - 1) / kSpBlock;
  const bool coul = m->has_charge;
  const int cp = coul ? 6 : 3;
  const size_t per_frame = (size_t)n * ((size_t)n_js * cp * sizeof(double) + 6 * sizeof(double) + sizeof(int));
  const int chunk = (int)std::min<size_t>(65535, std::max<size_t>(1, (size_t(512) << 20) / per_frame));
  const size_t nf_max = (size_t)std::min(chunk, n_frames);
  if (int rc = m->d_sp_part.grow(nf_max * n_js * n * cp)) return rc;
  if (int rc = m->d_sp_bonded.grow(nf_max * n * 6)) return rc;
  if (int rc = m->d_sp_bin.grow(nf_max * n)) return rc;
  if (n_center > 0)
    if (int rc = m->d_sp_mid.grow(nf_max)) return rc;
  const MartiniConst<R> K{R(m->r_cut * m->r_cut), m->n_types, m->angle_kind};
  const size_t lds = (size_t)2 * m->n_types * m->n_types * sizeof(R) + 3 * kLjBlock * sizeof(R) + kLjBlock * sizeof(int);
  auto pair_kernel = coul ? stress_pair_kernel<R, true> : stress_pair_kernel<R, false>;
  auto slab_kernel = coul ? stress_slab_kernel<true> : stress_slab_kernel<false>;
  MYTHOS_HIP_TRY(hipFuncSetAttribute((const void*)pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const double* mid = n_center > 0 ? m->d_sp_mid.get() : nullptr;
  const int slab_blocks = std::min((n_bins + kSpWaves - 1) / kSpWaves, 64);
  return for_frame_chunks(n_frames, chunk, [&](int f0, int nf) {
    const R* p = pos + (size_t)f0 * n * 3;
    const R* b = box + (size_t)f0 * 3;
    hipLaunchKernelGGL(pair_kernel, dim3(nbx, n_js, nf), dim3(kLjBlock), lds, st, n, p, b, m->d_types.get(), (const R*)m->d_sigma.get(),
                       (const R*)m->d_eps.get(), (const R*)m->d_charge.get(), m->d_excl.get(), K, m->rf<R>(), nbx, m->d_sp_part.get());
    if (n_center > 0)
      hipLaunchKernelGGL(stress_mid_kernel<R>, dim3(nf), dim3(kSpBlock), 0, st, n, n_center, m->d_sp_center.get(), p, m->d_sp_mid.get());
    hipLaunchKernelGGL(stress_bonded_kernel<R>, dim3(nbb, nf), dim3(kSpBlock), 0, st, n, p, b, m->d_bead_bonds.get(), m->d_bead_angles.get(),
                       m->d_bonds.get(), (const R*)m->d_bond_k.get(), (const R*)m->d_bond_r0.get(), m->d_angles.get(),
                       (const R*)m->d_angle_k.get(), (const R*)m->d_angle_t0.get(), m->angle_kind, mid, n_bins, m->d_sp_bonded.get(),
                       m->d_sp_bin.get());
    hipLaunchKernelGGL(slab_kernel, dim3(slab_blocks, nf), dim3(kSpBlock), 0, st, n, n_js, n_bins, by_term ? 1 : 0,
                       (const double*)m->d_sp_part.get(), (const double*)m->d_sp_bonded.get(), (const int*)m->d_sp_bin.get(), f0, out);
    MYTHOS_HIP_TRY(hipGetLastError());
    return 0;
  });
}

}  // namespace mythos

using namespace mythos;

extern "C" {

double mythos_martini_bar_per_kj_mol_nm3(void) { return kBarPerKjMolNm3; }

int mythos_martini_stress_profile_check(int n, double r_cut, int n_frames, const double* boxes, int n_center, const int32_t* center,
                                        int n_bins) {
  return stress_profile_check("mythos_martini_stress_profile_check", n, r_cut, n_frames, boxes, n_center, center, n_bins);
}

int mythos_martini_stress_profile(mythos_martini_t* m, const void* pos, const void* box, int n_frames, int n_center,
                                  const int32_t* center, int n_bins, int by_term, double* out, mythos_stream_t stream) {
  if (!m || !pos || !box || !out || n_frames < 0) {
    set_error("mythos_martini_stress_profile: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = stress_profile_check("mythos_martini_stress_profile", m->n, m->r_cut, n_frames, nullptr, n_center, center, n_bins)) return rc;
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  if (n_center > 0 && (m->h_sp_center.size() != (size_t)n_center || !std::equal(center, center + n_center, m->h_sp_center.begin()))) {
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));  // (a launch that still reads the list replaced below)
    if (int rc = m->d_sp_center.upload(center, (size_t)n_center)) return rc;
    m->h_sp_center.assign(center, center + n_center);
  }
  return with_real(m->dtype, [&](auto r) {
    using R = decltype(r);
    return stress_profile_typed<R>(m, (const R*)pos, (const R*)box, n_frames, n_center, n_bins, by_term != 0, out, st);
  });
}

}  // extern "C"
