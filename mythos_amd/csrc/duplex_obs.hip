// Duplex-mechanics observables behind the C ABI (mythos_duplex_obs_*): see duplex_obs.h for what is computed and where
// the reference defines it.  One workgroup per frame, three passes of the workgroup over the centres for the RMSD
// (centroid, the nine sums of the correlation matrix, the residual after the rotation one thread has solved for).
#include "duplex_obs.h"

#include <memory>

#include "mythos_internal.h"

struct mythos_duplex_obs {
  int n = 0, device = 0;
  mythos::DuplexView view;  // device pointers filled in
  mythos::DeviceBuf<int> d_bps, d_quartets;
  mythos::DeviceBuf<double> d_target;
  ~mythos_duplex_obs() { (void)hipSetDevice(device); }  // the members free themselves, on the set's device
};

namespace mythos {

template <typename R>
__global__ __launch_bounds__(256) void duplex_obs_kernel(const DuplexView v, int n, const R* __restrict__ center_all,
                                                         const R* __restrict__ quat_all, int frame0, double* __restrict__ out_all) {
  __shared__ double red[4];
  __shared__ double s_rot[9];
  const size_t f = (size_t)frame0 + blockIdx.x;
  const R* __restrict__ center = center_all + f * n * 3;
  const R* __restrict__ quat = quat_all + f * n * 4;
  double* __restrict__ out = out_all + f * MYTHOS_DUPLEX_ROW;
  const SiteGeo& geo = v.geo;
  auto centre = [&](int i) { return obs_centre(center, i); };
  auto back = [&](int i) {
    D3 a1, a2, a3;
    obs_axes(quat, i, a1, a2, a3);
    return back_site(geo, centre(i), a1, a2, a3);
  };
  auto base = [&](int i) {
    D3 a1, a2, a3;
    obs_axes(quat, i, a1, a2, a3);
    return base_site(geo, centre(i), a1);
  };
  // ---- [0] backbone distance (diameter.py:37-41)
  double bd = 0.0;
  for (int k = threadIdx.x; k < v.n_bp; k += blockDim.x) {
    const D3 d = obs_min_image(back(v.bps[2 * k]) - back(v.bps[2 * k + 1]), geo);
    bd += sqrt(dot(d, d));
  }
  bd = block_sum(bd, red);
  // ---- [2] twist in the x-y plane (stretch_torsion.py:19-35); 0 / 0 = NaN for a pair along z, as the reference
  double tw = 0.0;
  for (int k = threadIdx.x; k < v.n_q; k += blockDim.x) {
    const int a1 = v.quartets[4 * k], b1 = v.quartets[4 * k + 1], a2 = v.quartets[4 * k + 2], b2 = v.quartets[4 * k + 3];
    const D3 d1 = obs_min_image(base(b1) - base(a1), geo);
    const D3 d2 = obs_min_image(base(b2) - base(a2), geo);
    const double n1 = sqrt(d1.x * d1.x + d1.y * d1.y), n2 = sqrt(d2.x * d2.x + d2.y * d2.y);
    tw += acos(obs_clamp((d1.x / n1) * (d2.x / n2) + (d1.y / n1) * (d2.y / n2)));
  }
  tw = block_sum(tw, red);
  // ---- [3] RMSD to the centred target (rmse.py:19-67): raw coordinates, no minimum image
  double rmsd = 0.0;
  if (v.target) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const D3 c = centre(i);
      sx += c.x, sy += c.y, sz += c.z;
    }
    sx = block_sum(sx, red), sy = block_sum(sy, red), sz = block_sum(sz, red);
    const D3 mean{sx / n, sy / n, sz / n};
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const D3 x = centre(i) - mean;
      const double t0 = v.target[3 * (size_t)i], t1 = v.target[3 * (size_t)i + 1], t2 = v.target[3 * (size_t)i + 2];
      S[0] += x.x * t0, S[1] += x.x * t1, S[2] += x.x * t2;
      S[3] += x.y * t0, S[4] += x.y * t1, S[5] += x.y * t2;
      S[6] += x.z * t0, S[7] += x.z * t1, S[8] += x.z * t2;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = block_sum(S[k], red);
    if (threadIdx.x == 0) horn_rotation(S, s_rot);
    __syncthreads();
    // second pass: the residual itself (the identity |x|^2 + |t|^2 - 2 sum sigma cancels to nothing near the target)
    double r2 = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const D3 x = centre(i) - mean;
      const double d0 = s_rot[0] * x.x + s_rot[1] * x.y + s_rot[2] * x.z - v.target[3 * (size_t)i];
      const double d1 = s_rot[3] * x.x + s_rot[4] * x.y + s_rot[5] * x.z - v.target[3 * (size_t)i + 1];
      const double d2 = s_rot[6] * x.x + s_rot[7] * x.y + s_rot[8] * x.z - v.target[3 * (size_t)i + 2];
      r2 += d0 * d0 + d1 * d1 + d2 * d2;
    }
    rmsd = sqrt(block_sum(r2, red) / n);
  }
  if (threadIdx.x == 0) {
    out[0] = v.n_bp > 0 ? bd / v.n_bp : 0.0;
    // ---- [1] extension (stretch_torsion.py:84-95)
    double ext = 0.0;
    if (v.has_ends) {
      const D3 ca1 = centre(v.ends[0]), ca2 = centre(v.ends[2]);
      const D3 m1 = ca1 + 0.5 * obs_min_image(centre(v.ends[1]) - ca1, geo);
      const D3 m2 = ca2 + 0.5 * obs_min_image(centre(v.ends[3]) - ca2, geo);
      ext = fabs(obs_min_image(m2 - m1, geo).z);
    }
    out[1] = ext;
    out[2] = v.n_q > 0 ? tw : 0.0;
    out[3] = rmsd;
  }
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_duplex_obs_t* mythos_duplex_obs_create(int model, int n, const double* geometry, const double* box, int n_bp,
                                              const int32_t* base_pairs, int n_quartets, const int32_t* quartets,
                                              const int32_t* end_pairs, const double* target_center, int device) {
  if ((model < 1 || model > 3) || n <= 0 || !geometry || n_bp < 0 || n_quartets < 0 || (n_bp > 0 && !base_pairs) ||
      (n_quartets > 0 && !quartets)) {
    set_error("mythos_duplex_obs_create: invalid argument");
    return nullptr;
  }
  SiteGeo geo;
  if (!indices_in_range(base_pairs, 2 * (size_t)n_bp, n, "mythos_duplex_obs_create: base-pair index out of range") ||
      !indices_in_range(quartets, 4 * (size_t)n_quartets, n, "mythos_duplex_obs_create: quartet index out of range") ||
      !indices_in_range(end_pairs, end_pairs ? 4 : 0, n, "mythos_duplex_obs_create: end-pair index out of range") ||
      !site_geo_from(model, geometry, box, "mythos_duplex_obs_create", &geo))
    return nullptr;
  if (select_device(device, "mythos_duplex_obs_create")) return nullptr;
  auto o = std::make_unique<mythos_duplex_obs>();
  o->n = n, o->device = device;
  DuplexView& v = o->view;
  v.n_bp = n_bp, v.n_q = n_quartets, v.geo = geo;
  if (end_pairs) {
    v.has_ends = 1;
    for (int k = 0; k < 4; ++k) v.ends[k] = end_pairs[k];
  }
  if ((n_bp > 0 && o->d_bps.upload(base_pairs, 2 * (size_t)n_bp)) ||
      (n_quartets > 0 && o->d_quartets.upload(quartets, 4 * (size_t)n_quartets)) ||
      (target_center && o->d_target.upload(target_center, 3 * (size_t)n))) {
    set_error("mythos_duplex_obs_create: device allocation failed");
    return nullptr;
  }
  v.bps = o->d_bps.get(), v.quartets = o->d_quartets.get(), v.target = o->d_target.get();
  return o.release();
}

void mythos_duplex_obs_destroy(mythos_duplex_obs_t* o) { delete o; }

int mythos_duplex_obs_eval(mythos_duplex_obs_t* o, const void* center, const void* quat, int dtype, int n_frames, double* out,
                           mythos_stream_t stream) {
  if (!o || n_frames < 0 || (dtype != MYTHOS_F32 && dtype != MYTHOS_F64) || (n_frames > 0 && (!center || !quat || !out))) {
    set_error("mythos_duplex_obs_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipSetDevice(o->device));
  const DuplexView& v = o->view;
  // workgroup size as observables_launch chooses it: one wavefront when every list fits one (the centres are the
  // RMSD's list), four otherwise
  const int threads = (v.n_bp <= 64 && v.n_q <= 64 && (!v.target || o->n <= 64)) ? 64 : 256;
  return with_real(dtype, [&](auto r) {
    using R = decltype(r);
    return for_frame_chunks(n_frames, kFramesPerLaunch, [&](int f0, int nf) {
      hipLaunchKernelGGL(duplex_obs_kernel<R>, dim3(nf), dim3(threads), 0, (hipStream_t)stream, v, o->n, (const R*)center,
                         (const R*)quat, f0, out);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

}  // extern "C"
