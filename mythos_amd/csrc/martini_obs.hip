// MARTINI structural observables: the lengths of named bonds and the angles of named triplets of every frame, one launch
// for all names.  Replaces mythos/observables/bond_distances.py:15-17, 51-69 and triplet_angles.py:15-31, 73-92 (a
// jax.vmap over frames of a vmap over the matching pairs / triplets, once per name) with the angle of
// mythos/energy/martini/m2/angle.py:35-58.
//
// A group is every bond, or every angle, that shares one topology name.  One thread per (item, frame): 2 - 3 beads of
// 24 B gathered through an index list on the device, a handful of double operations, one 8-B store.  The kernel is
// gather bound; the index lists (32 B per item) stay in L2 across the frames of a launch.  No atomics.
// Output, dev double, group-major: group g with m_g members occupies the (S, m_g) row-major block that starts at
// S * (m_0 + ... + m_{g-1}) - the layout the distribution plan of w1.hip reads.
// Arithmetic is always double: fp32 positions and boxes are promoted on load.
#include <memory>
#include <vector>

#include "host_checks.h"
#include "mythos_internal.h"

struct mythos_martini_obs {
  int n = 0, n_groups = 0, device = 0;
  long long n_items = 0;    // sum of the groups' members
  mythos::DeviceBuf<int4> d_beads;  // [n_items] i, j, k (k = -1: a bond)
  mythos::DeviceBuf<int4> d_place;  // [n_items] members before this group, members of this group, column inside the group
  ~mythos_martini_obs() { (void)hipSetDevice(device); }  // the members free themselves, on the set's device
};

namespace mythos {

constexpr int kObsBlock = 256;

__device__ __forceinline__ double obs_wrap(double d, double l) { return d - l * rint(d / l); }

template <typename R>
__global__ __launch_bounds__(kObsBlock) void martini_obs_kernel(int n, long long n_items, const int4* __restrict__ beads,
                                                                const int4* __restrict__ place,
                                                                const R* __restrict__ pos, const R* __restrict__ box,
                                                                int frame0, int n_frames, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * kObsBlock + threadIdx.x;
  if (t >= n_items) return;
  const int frame = frame0 + blockIdx.y;
  const R* __restrict__ p = pos + (size_t)frame * n * 3;
  const double l[3] = {double(box[(size_t)frame * 3]), double(box[(size_t)frame * 3 + 1]), double(box[(size_t)frame * 3 + 2])};
  const int4 b = beads[t], w = place[t];
  double u[3], u2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u[k] = obs_wrap(double(p[3 * (size_t)b.x + k]) - double(p[3 * (size_t)b.y + k]), l[k]);
    u2 += u[k] * u[k];
  }
  double val;
  if (b.z < 0) {
    val = sqrt(u2);  // bond_distances.py:15-17: |minimum image of x_i - x_j|
  } else {
    double v[3], v2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = obs_wrap(double(p[3 * (size_t)b.z + k]) - double(p[3 * (size_t)b.y + k]), l[k]);
      v2 += v[k] * v[k];
    }
    // m2/angle.py:49-58: unit vectors first, then atan2(|cross|, dot)
    const double nu = sqrt(u2), nv = sqrt(v2);
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] /= nu, v[k] /= nv;
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    const double dot = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    val = atan2(sqrt(cx * cx + cy * cy + cz * cz), dot);
  }
  out[(size_t)n_frames * w.x + (size_t)frame * w.y + w.z] = val;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_martini_obs_t* mythos_martini_obs_create(int n, int n_groups, const int32_t* beads_per_item, const int32_t* members,
                                                const int32_t* index, int device) {
  if (n < 1 || n_groups < 1 || !beads_per_item || !members || !index) {
    set_error("mythos_martini_obs_create: invalid argument");
    return nullptr;
  }
  std::vector<int4> beads, place;
  long long before = 0;
  const int32_t* ix = index;
  for (int g = 0; g < n_groups; ++g) {
    const int w = beads_per_item[g];
    if ((w != 2 && w != 3) || members[g] < 1) {
      set_error("mythos_martini_obs_create: a group has 2 (bond) or 3 (angle) beads per item and at least one member");
      return nullptr;
    }
    for (int b = 0; b < members[g]; ++b, ix += w) {
      if (!indices_in_range(ix, (size_t)w, n, "mythos_martini_obs_create: bead index out of range")) return nullptr;
      beads.push_back(make_int4(ix[0], ix[1], w == 3 ? ix[2] : -1, 0));
      place.push_back(make_int4((int)before, members[g], b, 0));
    }
    before += members[g];
    if (before > (1ll << 30)) {
      set_error("mythos_martini_obs_create: more than 2^30 items per frame");
      return nullptr;
    }
  }
  if (select_device(device, "mythos_martini_obs_create")) return nullptr;
  auto h = std::make_unique<mythos_martini_obs>();
  h->n = n, h->n_groups = n_groups, h->device = device, h->n_items = before;
  if (h->d_beads.upload(beads) || h->d_place.upload(place)) {
    set_error("mythos_martini_obs_create: device allocation failed");
    return nullptr;
  }
  return h.release();
}

void mythos_martini_obs_destroy(mythos_martini_obs_t* h) { delete h; }

int64_t mythos_martini_obs_count(const mythos_martini_obs_t* h) { return h ? (int64_t)h->n_items : 0; }

int mythos_martini_obs_eval(mythos_martini_obs_t* h, const void* pos, const void* box, int dtype, int n_frames, double* out,
                            mythos_stream_t stream) {
  if (!h || !pos || !box || !out || n_frames < 0 || (dtype != MYTHOS_F32 && dtype != MYTHOS_F64)) {
    set_error("mythos_martini_obs_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  const unsigned nbx = (unsigned)((h->n_items + kObsBlock - 1) / kObsBlock);
  return with_real(dtype, [&](auto r) {
    using R = decltype(r);
    return for_frame_chunks(n_frames, 32768, [&](int f0, int nf) {  // the frame is blockIdx.y: grid.y <= 65535
      hipLaunchKernelGGL(martini_obs_kernel<R>, dim3(nbx, nf), dim3(kObsBlock), 0, (hipStream_t)stream, h->n, h->n_items,
                         h->d_beads.get(), h->d_place.get(), (const R*)pos, (const R*)box, f0, n_frames, out);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

}  // extern "C"
