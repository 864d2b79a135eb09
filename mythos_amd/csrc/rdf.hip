// Pair-distance histograms of stored MARTINI frames: the counts behind the radial distribution function g(r) of named
// pairs of bead selections, every frame and every pair of selections in one launch.  The reference has no such
// observable; the definition is that of MDAnalysis' InterRDF (ordered pairs, exclusion blocks), restated in DESIGN
// section 3.5m.
//
// A group is two bead lists A and B.  counts[frame][group][bin] += 1 for every ordered pair (i in A, j in B) with
// block[i] != block[j] (block = the bead's own index where the caller gave none, so i != j is the same test) whose
// minimum-image distance r over the masked dimensions is below r_max; bin = floor(r n_bins / r_max), at most n_bins - 1.
// Where A and B are the same list the kernel walks the positions p < q of the list and adds 2.
//
// One workgroup per (frame, group, tile of 256 beads of A): a thread owns one bead of A in registers, the workgroup
// walks B in strips of 256 beads staged in LDS as doubles with their block ids (every lane reads the same strip entry: a
// broadcast, no bank conflict), r^2 is compared with r_max^2 in front of the square root, hits go into a workgroup
// histogram in LDS (uint32, LDS atomic adds) and the non-zero bins leave once per workgroup as 64-bit atomic adds into
// the zeroed output.  Integer adds: the result has the same bits whatever the order, run after run.
// LDS: 256 x 32 B strip + 4 n_bins B histogram = 8 - 24 KB, all of it dynamic (16-byte aligned base).
// Arithmetic is always double: fp32 positions and boxes are promoted on load.  The image is d - L rint(d (1 / L)):
// rint's argument differs from d / L by an ulp, which picks the other image only at |d| = L / 2 - where both images are
// equally long, and no pair inside r_max <= L / 2 is.
// Brute force over the two lists, no cell list: F |A| |B| distances.  Sized for what this project stores (1 280 to about
// 20 000 beads, hundreds of frames); a list holds at most 2^22 beads, which also keeps a workgroup's uint32 bins exact.
#include <cmath>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "host_checks.h"
#include "mythos_internal.h"

struct mythos_rdf {
  int n = 0, n_groups = 0, n_bins = 0, dims = 3, device = 0;
  double r_max = 0.0;
  unsigned n_tiles = 0;
  std::vector<int64_t> n_pairs;      // [n_groups] admissible ordered pairs
  mythos::DeviceBuf<int> d_index;    // the lists back to back: A_0 B_0 A_1 B_1 ...
  mythos::DeviceBuf<int> d_block;    // [n] exclusion id of a bead (its own index where the caller gave none)
  mythos::DeviceBuf<int4> d_groups;  // [n_groups] start of A in d_index, |A|, start of B, |B|
  mythos::DeviceBuf<int4> d_tiles;   // [n_tiles] group, first position of A, 1 if A and B are the same list
  ~mythos_rdf() { (void)hipSetDevice(device); }  // the members free themselves, on the set's device
};

namespace mythos {

constexpr int kRdfBlock = 256;      // threads of a workgroup = beads of a tile of A = beads of a strip of B
constexpr int kRdfMaxBins = 4096;
constexpr int kRdfMaxList = 1 << 22;

struct RdfBead {  // 32 B: two 16-byte LDS reads
  double x, y, z;
  int block, pad;
};

template <typename R, int DIMS>
__global__ __launch_bounds__(kRdfBlock) void rdf_kernel(int n, int n_groups, int n_bins, double r_max, double bins_per_length,
                                                        const int4* __restrict__ tiles, const int4* __restrict__ groups,
                                                        const int* __restrict__ index, const int* __restrict__ block,
                                                        const R* __restrict__ pos, const R* __restrict__ box, int frame0,
                                                        unsigned long long* __restrict__ counts, unsigned int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rdf_lds[];
  RdfBead* __restrict__ s_strip = reinterpret_cast<RdfBead*>(rdf_lds);
  unsigned int* __restrict__ s_hist = reinterpret_cast<unsigned int*>(rdf_lds + kRdfBlock * sizeof(RdfBead));
  const int frame = frame0 + blockIdx.y;
  const int4 tile = tiles[blockIdx.x], g = groups[tile.x];
  const bool same = tile.z != 0;
  const R* __restrict__ p = pos + (size_t)frame * n * 3;
  double l[DIMS], inv_l[DIMS];
  bool short_edge = false;
#pragma unroll
  for (int k = 0; k < DIMS; ++k) {
    l[k] = double(box[(size_t)frame * 3 + k]);
    inv_l[k] = 1.0 / l[k];
    short_edge |= !(l[k] >= 2.0 * r_max);  // (a NaN edge too)
  }
  if (short_edge && blockIdx.x == 0 && threadIdx.x == 0) atomicMin(flags, (unsigned int)frame);
  for (int b = threadIdx.x; b < n_bins; b += kRdfBlock) s_hist[b] = 0u;

  const int ia = tile.y + (int)threadIdx.x;  // position in A
  const bool own = ia < g.y;
  double a[3] = {0.0, 0.0, 0.0};
  int a_block = 0;
  if (own) {
    const int bead = index[g.x + ia];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = double(p[3 * (size_t)bead + k]);
    a_block = block[bead];
  }
  const double r_max2 = r_max * r_max;
  const unsigned int inc = same ? 2u : 1u;
  // the same list: positions q > p only, so the strips in front of this tile hold nothing for it
  for (int b0 = same ? tile.y : 0; b0 < g.w; b0 += kRdfBlock) {
    __syncthreads();  // the strip before this one is used up (first pass: the histogram is zero)
    const int jb = b0 + (int)threadIdx.x;
    if (jb < g.w) {
      const int bead = index[g.z + jb];
      RdfBead q;
      q.x = double(p[3 * (size_t)bead]), q.y = double(p[3 * (size_t)bead + 1]), q.z = double(p[3 * (size_t)bead + 2]);
      q.block = block[bead], q.pad = 0;
      s_strip[threadIdx.x] = q;
    }
    __syncthreads();
    if (!own) continue;
    const int m = min(kRdfBlock, g.w - b0);
    const int first = same ? max(ia - b0 + 1, 0) : 0;
    for (int j = first; j < m; ++j) {
      const RdfBead q = s_strip[j];
      if (q.block == a_block) continue;
      const double qv[3] = {q.x, q.y, q.z};
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < DIMS; ++k) {
        const double d = a[k] - qv[k];
        const double w = d - l[k] * rint(d * inv_l[k]);
        r2 += w * w;
      }
      if (r2 < r_max2) {
        const int bin = min((int)(sqrt(r2) * bins_per_length), n_bins - 1);
        atomicAdd(&s_hist[bin], inc);
      }
    }
  }
  __syncthreads();
  unsigned long long* __restrict__ row = counts + ((size_t)frame * n_groups + tile.x) * n_bins;
  for (int b = threadIdx.x; b < n_bins; b += kRdfBlock) {
    const unsigned int c = s_hist[b];
    if (c) atomicAdd(&row[b], (unsigned long long)c);
  }
}

// |A| |B| minus the ordered pairs (p, q) whose beads share an exclusion id (block, or the bead itself)
static int64_t rdf_admissible_pairs(const int32_t* a, int n_a, const int32_t* b, int n_b, const int32_t* block) {
  std::unordered_map<int32_t, int64_t> in_b;
  for (int q = 0; q < n_b; ++q) ++in_b[block ? block[b[q]] : b[q]];
  int64_t shared = 0;
  for (int p = 0; p < n_a; ++p) {
    const auto it = in_b.find(block ? block[a[p]] : a[p]);
    if (it != in_b.end()) shared += it->second;
  }
  return (int64_t)n_a * n_b - shared;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_rdf_t* mythos_rdf_create(int n, int n_groups, const int32_t* n_a, const int32_t* n_b, const int32_t* index,
                                const int32_t* block, int n_bins, double r_max, int dims, int device) {
  if (n < 1 || !n_a || !n_b || !index) {
    set_error("mythos_rdf_create: invalid argument");
    return nullptr;
  }
  if (n_groups < 1) {
    set_error("mythos_rdf_create: at least one group");
    return nullptr;
  }
  if (n_bins < 1 || n_bins > kRdfMaxBins) {
    set_error("mythos_rdf_create: n_bins must be in [1, 4096]");
    return nullptr;
  }
  if (!(r_max > 0.0) || !std::isfinite(r_max)) {
    set_error("mythos_rdf_create: r_max must be positive and finite");
    return nullptr;
  }
  if (dims != MYTHOS_RDF_XY && dims != MYTHOS_RDF_XYZ) {
    set_error("mythos_rdf_create: dims must be MYTHOS_RDF_XY or MYTHOS_RDF_XYZ");
    return nullptr;
  }
  auto h = std::make_unique<mythos_rdf>();
  std::vector<int4> groups, tiles;
  size_t at = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (n_a[g] < 1 || n_b[g] < 1) {
      set_error("mythos_rdf_create: every list holds at least one bead");
      return nullptr;
    }
    if (n_a[g] > kRdfMaxList || n_b[g] > kRdfMaxList) {
      set_error("mythos_rdf_create: a list holds more than 2^22 beads");
      return nullptr;
    }
    const int32_t *a = index + at, *b = a + n_a[g];
    if (!indices_in_range(a, (size_t)n_a[g] + (size_t)n_b[g], n, "mythos_rdf_create: bead index out of range")) return nullptr;
    h->n_pairs.push_back(rdf_admissible_pairs(a, n_a[g], b, n_b[g], block));
    if (h->n_pairs.back() == 0) {
      set_error("mythos_rdf_create: a group has no admissible pair");
      return nullptr;
    }
    const int same = n_a[g] == n_b[g] && std::memcmp(a, b, sizeof(int32_t) * (size_t)n_a[g]) == 0;
    groups.push_back(make_int4((int)at, n_a[g], (int)at + n_a[g], n_b[g]));
    for (int a0 = 0; a0 < n_a[g]; a0 += kRdfBlock) tiles.push_back(make_int4(g, a0, same, 0));
    at += (size_t)n_a[g] + (size_t)n_b[g];
    if (at > (size_t)1 << 30 || tiles.size() > (size_t)1 << 30) {
      set_error("mythos_rdf_create: more than 2^30 list entries");
      return nullptr;
    }
  }
  std::vector<int> ids((size_t)n);
  for (int i = 0; i < n; ++i) ids[i] = block ? block[i] : i;
  if (select_device(device, "mythos_rdf_create")) return nullptr;
  h->n = n, h->n_groups = n_groups, h->n_bins = n_bins, h->dims = dims, h->device = device, h->r_max = r_max;
  h->n_tiles = (unsigned)tiles.size();
  if (h->d_index.upload(index, at) || h->d_block.upload(ids) || h->d_groups.upload(groups) || h->d_tiles.upload(tiles)) {
    set_error("mythos_rdf_create: device allocation failed");
    return nullptr;
  }
  return h.release();
}

void mythos_rdf_destroy(mythos_rdf_t* h) { delete h; }

int mythos_rdf_n_pairs(const mythos_rdf_t* h, int64_t* n_pairs) {
  if (!h || !n_pairs) {
    set_error("mythos_rdf_n_pairs: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  std::copy(h->n_pairs.begin(), h->n_pairs.end(), n_pairs);
  return MYTHOS_OK;
}

int mythos_rdf_eval(mythos_rdf_t* h, const void* pos, const void* box, int dtype, int n_frames, int64_t* counts, int32_t* flags,
                    mythos_stream_t stream) {
  if (!h || !pos || !box || !counts || !flags || n_frames < 0 || (dtype != MYTHOS_F32 && dtype != MYTHOS_F64)) {
    set_error("mythos_rdf_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  MYTHOS_HIP_TRY(hipMemsetAsync(flags, 0xff, sizeof(int32_t), (hipStream_t)stream));  // -1: every frame holds 2 r_max
  if (n_frames == 0) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)n_frames * h->n_groups * h->n_bins, (hipStream_t)stream));
  const size_t lds = kRdfBlock * sizeof(RdfBead) + sizeof(unsigned int) * (size_t)h->n_bins;
  const double bins_per_length = double(h->n_bins) / h->r_max;
  return with_real(dtype, [&](auto r) {
    using R = decltype(r);
    auto kernel = h->dims == MYTHOS_RDF_XY ? rdf_kernel<R, 2> : rdf_kernel<R, 3>;
    return for_frame_chunks(n_frames, 32768, [&](int f0, int nf) {  // the frame is blockIdx.y: grid.y <= 65535
      hipLaunchKernelGGL(kernel, dim3(h->n_tiles, nf), dim3(kRdfBlock), lds, (hipStream_t)stream, h->n, h->n_groups, h->n_bins,
                         h->r_max, bins_per_length, h->d_tiles.get(), h->d_groups.get(), h->d_index.get(), h->d_block.get(),
                         (const R*)pos, (const R*)box, f0, (unsigned long long*)counts, (unsigned int*)flags);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

}  // extern "C"
