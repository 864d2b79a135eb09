// Membrane observables of a lipid bilayer: leaflet assignment, thickness and area per lipid of every frame, one launch.
// Replaces mythos/observables/membrane_thickness.py:33-43 and area_per_lipid.py:31-41 (LiPyphilic's AssignLeaflets,
// MembThickness and AreaPerLipid at their defaults, n_bins = 1, run on the host through MDAnalysis once per objective
// per optimisation step).
//
// Definitions.  A lipid is a residue that owns beads of the lipid selection; its z is the
// unweighted mean z of those beads.  The midpoint of a frame is the mean z of ALL beads of the lipid selection (over
// beads, not over lipids).  Leaflet +1 if z_lipid > midpoint, else -1 (a tie goes to -1).  Thickness is the mean z of the
// thickness beads whose lipid is in leaflet +1 minus the same mean of leaflet -1, NaN if either is empty; coordinates
// are used as stored (no re-wrapping in z).  Area per lipid is Lx Ly (occupied leaflets) / n_lipids: the mean of the
// Voronoi cells of a periodic tessellation, which tile the box.
//
// One workgroup per frame, three passes of the workgroup over the index lists: the selection's beads for the midpoint,
// the lipids for the leaflets, the thickness beads for the two means.  A thickness bead recomputes its lipid's z by the
// same function the leaflet pass used (same operations in the same order: the same bits), so nothing is kept per
// lipid and their number has no limit.  Sums are double and in a fixed order: thread-strided partials, then block_sum
// of wave_ops.h (the wavefront's tree, the wavefronts' totals in order through LDS).  No atomics: a frame's row depends
// on that frame only.  The kernel is launch and gather bound (3 - 4 gathered z per lipid and frame).
#include <memory>
#include <vector>

#include "host_checks.h"
#include "mythos_internal.h"
#include "wave_ops.h"

struct mythos_membrane {
  int n = 0, n_lipids = 0, n_sel = 0, n_thick = 0, device = 0;
  mythos::DeviceBuf<int> d_start;        // [n_lipids + 1] CSR offsets into d_sel
  mythos::DeviceBuf<int> d_sel;          // [n_sel] beads of the lipid selection, grouped by lipid
  mythos::DeviceBuf<int> d_thick;        // [n_thick] beads of the thickness selection
  mythos::DeviceBuf<int> d_thick_lipid;  // [n_thick] the lipid of each
  ~mythos_membrane() { (void)hipSetDevice(device); }  // the members free themselves, on the set's device
};

namespace mythos {

constexpr int kMemBlock = 256;

template <typename R>
__device__ __forceinline__ double lipid_z(const R* __restrict__ p, const int* __restrict__ start, const int* __restrict__ sel, int l) {
  const int a = start[l], b = start[l + 1];
  double s = 0.0;
  for (int k = a; k < b; ++k) s += double(p[3 * (size_t)sel[k] + 2]);
  return s / double(b - a);
}

template <typename R>
__global__ __launch_bounds__(kMemBlock) void membrane_kernel(int n, int n_lipids, int n_sel, int n_thick,
                                                             const int* __restrict__ start, const int* __restrict__ sel,
                                                             const int* __restrict__ thick, const int* __restrict__ thick_lipid,
                                                             const R* __restrict__ pos, const R* __restrict__ box, int frame0,
                                                             double* __restrict__ out, int8_t* __restrict__ leaflets) {
  __shared__ double s_w[kMemBlock / 64];
  const unsigned int block = blockDim.x;
  __builtin_assume(block == kMemBlock);  // (the one launch site; block_sum then adds its four totals unrolled)
  const int frame = frame0 + blockIdx.x;
  const R* __restrict__ p = pos + (size_t)frame * n * 3;
  // midpoint: over beads
  double zs = 0.0;
  for (int k = threadIdx.x; k < n_sel; k += kMemBlock) zs += double(p[3 * (size_t)sel[k] + 2]);
  const double mid = block_sum(zs, s_w) / double(n_sel);
  // leaflets
  double up = 0.0;
  for (int l = threadIdx.x; l < n_lipids; l += kMemBlock) {
    const bool upper = lipid_z(p, start, sel, l) > mid;
    up += upper ? 1.0 : 0.0;
    if (leaflets) leaflets[(size_t)frame * n_lipids + l] = upper ? 1 : -1;
  }
  const double n_up = block_sum(up, s_w), n_lo = double(n_lipids) - n_up;  // counts: exact in double
  // thickness beads by the leaflet of their lipid
  double zu = 0.0, zl = 0.0, cu = 0.0;
  for (int t = threadIdx.x; t < n_thick; t += kMemBlock) {
    const double z = double(p[3 * (size_t)thick[t] + 2]);
    if (lipid_z(p, start, sel, thick_lipid[t]) > mid)
      zu += z, cu += 1.0;
    else
      zl += z;
  }
  zu = block_sum(zu, s_w), zl = block_sum(zl, s_w), cu = block_sum(cu, s_w);
  if (threadIdx.x == 0) {
    const double cl = double(n_thick) - cu, nan = __builtin_nan("");
    const double mu = cu > 0.0 ? zu / cu : nan, ml = cl > 0.0 ? zl / cl : nan;
    const double lx = double(box[(size_t)frame * 3]), ly = double(box[(size_t)frame * 3 + 1]);
    const double occupied = (n_up > 0.0 ? 1.0 : 0.0) + (n_lo > 0.0 ? 1.0 : 0.0);
    double* __restrict__ row = out + (size_t)frame * MYTHOS_MEMBRANE_ROW;
    row[0] = mu - ml;  // NaN if a leaflet has no thickness bead (and with it: no lipid)
    row[1] = lx * ly * occupied / double(n_lipids);
    row[2] = mid;
    row[3] = n_up;
    row[4] = n_lo;
    row[5] = mu;
    row[6] = ml;
  }
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_membrane_t* mythos_membrane_create(int n, int n_lipids, const int32_t* lipid_start, const int32_t* lipid_beads, int n_thick,
                                          const int32_t* thick_beads, const int32_t* thick_lipid, int device) {
  if (n < 1 || n_lipids < 1 || n_thick < 0 || !lipid_start || !lipid_beads || (n_thick > 0 && (!thick_beads || !thick_lipid))) {
    set_error("mythos_membrane_create: invalid argument");
    return nullptr;
  }
  if (lipid_start[0] != 0) {
    set_error("mythos_membrane_create: lipid_start[0] must be 0");
    return nullptr;
  }
  for (int l = 0; l < n_lipids; ++l)
    if (lipid_start[l + 1] <= lipid_start[l]) {
      set_error("mythos_membrane_create: every lipid owns at least one bead of the selection");
      return nullptr;
    }
  const int n_sel = lipid_start[n_lipids];
  if (!indices_in_range(lipid_beads, (size_t)n_sel, n, "mythos_membrane_create: bead index out of range") ||
      !indices_in_range(thick_beads, (size_t)n_thick, n, "mythos_membrane_create: thickness bead or its lipid out of range") ||
      !indices_in_range(thick_lipid, (size_t)n_thick, n_lipids, "mythos_membrane_create: thickness bead or its lipid out of range"))
    return nullptr;
  if (select_device(device, "mythos_membrane_create")) return nullptr;
  auto h = std::make_unique<mythos_membrane>();
  h->n = n, h->n_lipids = n_lipids, h->n_sel = n_sel, h->n_thick = n_thick, h->device = device;
  if (h->d_start.upload(lipid_start, (size_t)n_lipids + 1) || h->d_sel.upload(lipid_beads, (size_t)n_sel) ||
      h->d_thick.upload(thick_beads, (size_t)n_thick) || h->d_thick_lipid.upload(thick_lipid, (size_t)n_thick)) {
    set_error("mythos_membrane_create: device allocation failed");
    return nullptr;
  }
  return h.release();
}

void mythos_membrane_destroy(mythos_membrane_t* h) { delete h; }

int mythos_membrane_n_lipids(const mythos_membrane_t* h) { return h ? h->n_lipids : 0; }

int mythos_membrane_eval(mythos_membrane_t* h, const void* pos, const void* box, int dtype, int n_frames, double* out,
                         int8_t* leaflets, mythos_stream_t stream) {
  if (!h || !pos || !box || !out || n_frames < 0 || (dtype != MYTHOS_F32 && dtype != MYTHOS_F64)) {
    set_error("mythos_membrane_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  return with_real(dtype, [&](auto r) {
    using R = decltype(r);
    return for_frame_chunks(n_frames, kFramesPerLaunch, [&](int f0, int nf) {
      hipLaunchKernelGGL(membrane_kernel<R>, dim3(nf), dim3(kMemBlock), 0, (hipStream_t)stream, h->n, h->n_lipids, h->n_sel,
                         h->n_thick, h->d_start.get(), h->d_sel.get(), h->d_thick.get(), h->d_thick_lipid.get(), (const R*)pos,
                         (const R*)box, f0, out, leaflets);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

}  // extern "C"
