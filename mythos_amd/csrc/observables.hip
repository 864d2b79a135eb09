// Observable sets behind the C ABI (mythos_observables_*): see observables.h for what is computed and where the
// reference defines it.  One workgroup per frame; mythos_oxdna_energy_obs (oxdna_kernels.hip) queues the same kernel behind
// its energy launch, through the same observables_launch that mythos_observables_eval calls per chunk of frames.
#include "observables.h"

#include <memory>

#include "mythos_internal.h"

namespace mythos {

template <typename R>
__global__ __launch_bounds__(256) void observables_kernel(const ObsView v, int n, const R* __restrict__ center,
                                                          const R* __restrict__ quat, double* __restrict__ out) {
  __shared__ double red[4];
  const size_t f = blockIdx.x;
  frame_observables<R>(v, center + f * n * 3, quat + f * n * 4, out + f * v.width, v.axis + f * (size_t)v.n_q * 3, red);
}

int obs_view_for(mythos_obs* o, int n_frames, ObsView* out) {
  const size_t need = (size_t)std::max(n_frames, 1) * std::max(o->view.n_q, 1) * 3;
  if (int rc = o->d_axis.grow(need)) return rc;
  o->view.axis = o->d_axis.get();
  *out = o->view;
  return 0;
}

int observables_launch(mythos_obs* o, ObsView v, const void* center, const void* quat, int f0, int nf, double* out,
                       hipStream_t st) {
  // one workgroup per frame; a frame whose lists fit one wavefront (the DiffTRe systems: 30 base pairs, 31 quartets) gets
  // a workgroup of one - its sums are the first wavefront's sums of the wider workgroup bit for bit (the other partials
  // are zeros), its barriers cost nothing, and four times as many frames are in flight
  const int threads = (v.n_bp <= 64 && v.n_q <= 64) ? 64 : 256;
  v.axis += (size_t)f0 * v.n_q * 3;
  with_real(o->dtype, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL(observables_kernel<R>, dim3(nf), dim3(threads), 0, st, v, o->n, (const R*)center + (size_t)f0 * o->n * 3,
                       (const R*)quat + (size_t)f0 * o->n * 4, out + (size_t)f0 * v.width);
  });
  MYTHOS_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_obs_t* mythos_observables_create(int model, int n, const double* geometry, const double* box, int n_bp,
                                        const int32_t* base_pairs, int n_quartets, const int32_t* quartets, int skip_ends,
                                        int dtype, int device) {
  if ((model < 1 || model > 3) || n <= 0 || !geometry || n_bp < 0 || n_quartets < 0 || (n_bp > 0 && !base_pairs) ||
      (n_quartets > 0 && !quartets) || (dtype != MYTHOS_F32 && dtype != MYTHOS_F64)) {
    set_error("mythos_observables_create: invalid argument");
    return nullptr;
  }
  SiteGeo geo;
  if (!indices_in_range(base_pairs, 2 * (size_t)n_bp, n, "mythos_observables_create: base-pair index out of range") ||
      !indices_in_range(quartets, 4 * (size_t)n_quartets, n, "mythos_observables_create: quartet index out of range") ||
      !site_geo_from(model, geometry, box, "mythos_observables_create", &geo))
    return nullptr;
  if (select_device(device, "mythos_observables_create")) return nullptr;
  auto o = std::make_unique<mythos_obs>();
  o->n = n, o->dtype = dtype, o->device = device;
  ObsView& v = o->view;
  v.n_bp = n_bp, v.n_q = n_quartets;
  v.skip = skip_ends ? 2 : 0;
  v.n_corr = std::max(0, n_quartets - 2 * v.skip);
  v.width = 4 + v.n_corr;
  v.geo = geo;
  if ((n_bp > 0 && o->d_bps.upload(base_pairs, 2 * (size_t)n_bp)) ||
      (n_quartets > 0 && o->d_quartets.upload(quartets, 4 * (size_t)n_quartets))) {
    set_error("mythos_observables_create: device allocation failed");
    return nullptr;
  }
  v.bps = o->d_bps.get(), v.quartets = o->d_quartets.get();
  return o.release();
}

void mythos_observables_destroy(mythos_obs_t* o) { delete o; }

int mythos_observables_width(const mythos_obs_t* o) { return o ? o->view.width : -1; }

int mythos_observables_eval(mythos_obs_t* o, const void* center, const void* quat, int n_frames, double* out,
                            mythos_stream_t stream) {
  if (!o || n_frames < 0 || (n_frames > 0 && (!center || !quat || !out))) {
    set_error("mythos_observables_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipSetDevice(o->device));
  ObsView v;
  if (int rc = obs_view_for(o, n_frames, &v)) return rc;
  return for_frame_chunks(n_frames, kFramesPerLaunch, [&](int f0, int nf) {
    return observables_launch(o, v, center, quat, f0, nf, out, (hipStream_t)stream);
  });
}

}  // extern "C"
