// Weighted 1-D Wasserstein distance between sample distributions and reference distributions, and its derivative with
// respect to the per-frame weights.  Replaces mythos/observables/wasserstein.py:42-78, which sorts u, v and their
// concatenation on every evaluation (and again under jax.grad).
//
// Inside a DiffTRe optimisation the samples of a stored trajectory do not change between optimisation steps, only the
// frame weights do.  So the sort happens once: a PLAN holds, per group (one named bond / angle), the merged ascending
// support of concat(u.flatten(), v) as
//   dx[k]   = x[k+1] - x[k]                               (0 for the last entry)
//   src[k]  = the frame index s (>= 0) of a u entry, or the bits of the double -v_weight (sign bit set) of a v entry
//   rank[t] = the merged position of the u sample t = s * m + b  (the inverse of the merge order on the u entries)
// and an evaluation is
//   a_k = weights[s_k] / m | -v_weight,   D_k = sum_{j <= k} a_j,   W = sum_k dx_k |D_k|          (wasserstein.py:58-63)
//   dW/da_j = sum_{k >= j} dx_k sign(D_k)  (sign(0) = 0),   dW/dweights[s] = (1 / m) sum_b dW/da_{rank[s m + b]}
//
// Layout: every group's merged entries start at a multiple of kW1Chunk and are padded to one (dx = 0, a = -0.0), so a
// chunk belongs to one group and all groups share the launches.  A workgroup of 256 threads owns a chunk of 2048 entries,
// 8 consecutive entries per thread (64 B of dx, 64 B of src: four 16-B loads each), scanned serially in registers, then
// across the wavefront (wave_ops.h group_scan) and across the four wavefronts through one LDS exchange.
// Carries between chunks come from chunk totals written by an earlier LAUNCH and added in index order - no workgroup
// waits for another one.  Launches of an evaluation (all groups together):
//   w1_chunk_sum      src                      -> chunk totals of a                              8 B / entry
//   w1_scan           dx, src, chunk totals    -> dx sign(D) per entry, chunk totals of it and of W   16 B + 8 B
//   w1_suffix         dx sign(D), chunk totals -> dW/da per entry, in place                      8 B + 8 B   (gradient only)
//   w1_frame_sum      rank, dW/da              -> dW/dweights[g][s]: a wavefront or a workgroup per frame   12 B / sample (gradient only)
//   w1_total          chunk totals of W        -> W[g]
// Every sum has a fixed order and no atomic is used: two evaluations of the same inputs agree bit for bit.  The
// per-frame gradient gathers through rank instead of scattering dW/da to sample order and summing rows: 8-B accesses at
// sorted positions either way (uncoalesced reads here, uncoalesced writes there), plain coalesced stores in w1_suffix,
// and nothing is written through an index.  DESIGN.md 3.5b has what w1_frame_sum costs.
#include <memory>
#include <vector>

#include "mythos_internal.h"
#include "wave_ops.h"

namespace mythos {

constexpr int kW1Block = 256;
constexpr int kW1Per = 8;
constexpr int kW1Chunk = kW1Block * kW1Per;

struct W1Group {
  long long u_off;  // first sample of the group in the sample block
  long long v_off;  // first reference sample of the group in the concatenated reference samples
  long long o_off;  // first entry of the group in the concatenated merge order
  long long n_u, n_v;
  int chunk0, n_chunks;
  int m;            // members per frame
  int frames;       // n_u = frames * m
  int has_vw, pad;
  double uniform;   // 1 / (frames m): the coefficient of a u entry without frame weights (wasserstein.py:19-20)
};

}  // namespace mythos

struct mythos_w1_plan {
  int n_groups = 0, max_frames = 0, max_members = 0, device = 0, n_chunks = 0;
  long long n_u_total = 0;
  mythos::DeviceBuf<mythos::W1Group> d_groups;
  mythos::DeviceBuf<int> d_chunk_group;  // [n_chunks]
  mythos::DeviceBuf<double> d_dx;        // [n_chunks * kW1Chunk]
  mythos::DeviceBuf<long long> d_src;    // [n_chunks * kW1Chunk]
  mythos::DeviceBuf<int> d_rank;         // [n_u_total]
  mythos::DeviceBuf<double> d_g;         // [n_chunks * kW1Chunk] dx sign(D), then dW/da
  mythos::DeviceBuf<double> d_part;      // [3][n_chunks]: chunk totals of a | of dx |D| | of dx sign(D)
  mythos::DeviceBuf<int> d_flag;
  ~mythos_w1_plan() { (void)hipSetDevice(device); }  // the members free themselves, on the plan's device
};

namespace mythos {

// sum over the workgroup, every thread gets it: xor butterfly inside the wavefront, wavefront totals added in order
__device__ __forceinline__ double w1_block_sum(double v, double* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kW1Block / 64; ++w) s += s_w[w];
  return s;
}

// what the threads before this one hold in total (thread order)
__device__ __forceinline__ double w1_block_scan_exclusive(double v, double* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double inc = group_scan<64>(v);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  double before = 0.0;
#pragma unroll
  for (int w = 0; w < kW1Block / 64 - 1; ++w)
    if (w < wave) before += s_w[w];
  double ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.0;
  return before + ex;
}

__device__ __forceinline__ double w1_coef(long long src, const double* __restrict__ weights, const W1Group& g) {
  if (src < 0) return __builtin_bit_cast(double, src);
  return weights ? weights[src] / double(g.m) : g.uniform;
}

template <typename T>
__device__ __forceinline__ void w1_load8(const T* __restrict__ p, T (&v)[kW1Per]) {
  static_assert(sizeof(T) == 8, "two entries per 16-B load");
  const int4* q = reinterpret_cast<const int4*>(p);
#pragma unroll
  for (int k = 0; k < kW1Per / 2; ++k) {
    const int4 w = q[k];
    v[2 * k] = __builtin_bit_cast(T, ((long long)w.y << 32) | (long long)(unsigned int)w.x);
    v[2 * k + 1] = __builtin_bit_cast(T, ((long long)w.w << 32) | (long long)(unsigned int)w.z);
  }
}

__device__ __forceinline__ void w1_store8(double* __restrict__ p, const double (&v)[kW1Per]) {
  double2* q = reinterpret_cast<double2*>(p);
#pragma unroll
  for (int k = 0; k < kW1Per / 2; ++k) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
}

// plan build: one thread per padded merged entry
__global__ __launch_bounds__(kW1Block) void w1_plan_kernel(const W1Group* __restrict__ groups, const int* __restrict__ chunk_group,
                                                           const double* __restrict__ u, const double* __restrict__ v,
                                                           const double* __restrict__ vw, const long long* __restrict__ order,
                                                           double* __restrict__ dx, long long* __restrict__ src,
                                                           int* __restrict__ rank, int* __restrict__ flag) {
  const int c = blockIdx.x / kW1Per;
  const W1Group g = groups[chunk_group[c]];
  const long long p = (long long)blockIdx.x * kW1Block + threadIdx.x;  // padded position
  const long long k = p - (long long)g.chunk0 * kW1Chunk;              // position inside the group
  const long long len = g.n_u + g.n_v;
  double d = 0.0;
  long long word = (long long)0x8000000000000000ull;  // -0.0: padding
  if (k < len) {
    const long long i0 = order[g.o_off + k];
    const long long i1 = k + 1 < len ? order[g.o_off + k + 1] : i0;
    if (i0 < 0 || i0 >= len || i1 < 0 || i1 >= len) {
      *flag = 1;  // (every writer stores the same value)
    } else {
      const double x0 = i0 < g.n_u ? u[g.u_off + i0] : v[g.v_off + i0 - g.n_u];
      const double x1 = i1 < g.n_u ? u[g.u_off + i1] : v[g.v_off + i1 - g.n_u];
      d = x1 - x0;
      if (!(d >= 0.0)) *flag = 2;  // not ascending, or NaN samples
      if (i0 < g.n_u) {
        word = i0 / g.m;
        rank[g.u_off + i0] = (int)p;
      } else {
        const double wv = g.has_vw ? vw[g.v_off + i0 - g.n_u] : 1.0 / double(g.n_v);
        if (!(wv >= 0.0)) *flag = 3;  // a reference weight is a mass
        word = __builtin_bit_cast(long long, -wv) | (long long)0x8000000000000000ull;
      }
    }
  }
  dx[p] = d;
  src[p] = word;
}

__global__ __launch_bounds__(kW1Block) void w1_chunk_sum_kernel(const W1Group* __restrict__ groups, const int* __restrict__ chunk_group,
                                                                const long long* __restrict__ src,
                                                                const double* __restrict__ weights, double* __restrict__ a_tot) {
  __shared__ double s_w[kW1Block / 64];
  const int c = blockIdx.x;
  const W1Group g = groups[chunk_group[c]];
  long long s[kW1Per];
  w1_load8(src + (size_t)c * kW1Chunk + threadIdx.x * kW1Per, s);
  double t = 0.0;
#pragma unroll
  for (int j = 0; j < kW1Per; ++j) t += w1_coef(s[j], weights, g);
  t = w1_block_sum(t, s_w);
  if (threadIdx.x == 0) a_tot[c] = t;
}

__global__ __launch_bounds__(kW1Block) void w1_scan_kernel(const W1Group* __restrict__ groups, const int* __restrict__ chunk_group,
                                                           const double* __restrict__ dx, const long long* __restrict__ src,
                                                           const double* __restrict__ weights, const double* __restrict__ a_tot,
                                                           double* __restrict__ gbuf, double* __restrict__ w_tot,
                                                           double* __restrict__ g_tot) {
  __shared__ double s_w[4][kW1Block / 64];
  const int c = blockIdx.x;
  const W1Group g = groups[chunk_group[c]];
  // carry-in: the totals of the group's earlier chunks, in a fixed order
  double cin = 0.0;
  for (int k = g.chunk0 + threadIdx.x; k < c; k += kW1Block) cin += a_tot[k];
  cin = w1_block_sum(cin, s_w[0]);
  const size_t at = (size_t)c * kW1Chunk + threadIdx.x * kW1Per;
  long long s[kW1Per];
  double d[kW1Per], p[kW1Per];
  w1_load8(src + at, s);
  w1_load8(dx + at, d);
  double run = 0.0;
#pragma unroll
  for (int j = 0; j < kW1Per; ++j) {
    run += w1_coef(s[j], weights, g);
    p[j] = run;
  }
  const double base = cin + w1_block_scan_exclusive(run, s_w[1]);
  double wl = 0.0, gl = 0.0;
#pragma unroll
  for (int j = 0; j < kW1Per; ++j) {
    const double D = base + p[j];
    wl += d[j] * fabs(D);
    p[j] = D > 0.0 ? d[j] : (D < 0.0 ? -d[j] : 0.0);  // dx sign(D)
    gl += p[j];
  }
  wl = w1_block_sum(wl, s_w[2]);
  if (threadIdx.x == 0) w_tot[c] = wl;
  if (gbuf) {
    w1_store8(gbuf + at, p);
    gl = w1_block_sum(gl, s_w[3]);
    if (threadIdx.x == 0) g_tot[c] = gl;
  }
}

// dW/da_j = sum_{k >= j} dx_k sign(D_k): the scan of w1_scan_kernel run from the far end (thread t owns the 8 entries
// that end 8 t entries before the end of the chunk); in place
__global__ __launch_bounds__(kW1Block) void w1_suffix_kernel(const W1Group* __restrict__ groups, const int* __restrict__ chunk_group,
                                                             const double* __restrict__ g_tot, double* __restrict__ gbuf) {
  __shared__ double s_w[2][kW1Block / 64];
  const int c = blockIdx.x;
  const W1Group g = groups[chunk_group[c]];
  double cin = 0.0;
  for (int k = c + 1 + threadIdx.x; k < g.chunk0 + g.n_chunks; k += kW1Block) cin += g_tot[k];
  cin = w1_block_sum(cin, s_w[0]);
  const size_t at = (size_t)c * kW1Chunk + (size_t)(kW1Block - 1 - threadIdx.x) * kW1Per;
  double p[kW1Per];
  w1_load8(gbuf + at, p);
#pragma unroll
  for (int j = kW1Per - 2; j >= 0; --j) p[j] += p[j + 1];
  const double base = cin + w1_block_scan_exclusive(p[0], s_w[1]);
#pragma unroll
  for (int j = 0; j < kW1Per; ++j) p[j] = base + p[j];
  w1_store8(gbuf + at, p);
}

// dW/dweights[g][s] = (1 / m) sum_b dW/da at the merged position of sample (s, b).  The reads are 8-B gathers at sorted
// positions, so the kernel lives on loads in flight: WAVES = 1, one wavefront per frame, for short rows; WAVES = 4, the
// whole workgroup on one frame (wavefront sums added in wavefront order), when rows are long and frames alone would
// leave the chip with a few wavefronts per CU.  The choice depends on the plan only, so results stay reproducible.
template <int WAVES>
__global__ __launch_bounds__(kW1Block) void w1_frame_sum_kernel(const W1Group* __restrict__ groups, const int* __restrict__ rank,
                                                                const double* __restrict__ gbuf, int row_stride,
                                                                double* __restrict__ dw) {
  static_assert(WAVES == 1 || WAVES == kW1Block / 64, "a wavefront or the workgroup per frame");
  __shared__ double s_w[kW1Block / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long s = WAVES == 1 ? (long long)blockIdx.x * (kW1Block / 64) + wave : (long long)blockIdx.x;
  const W1Group g = groups[blockIdx.y];
  if (s >= g.frames) return;  // (uniform per wavefront; per workgroup when WAVES == 4)
  const int* __restrict__ r = rank + g.u_off + s * g.m;
  double a = 0.0;
#pragma unroll 4
  for (int b = WAVES == 1 ? lane : (int)threadIdx.x; b < g.m; b += 64 * WAVES) a += gbuf[r[b]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if constexpr (WAVES == 1) {
    if (lane == 0) dw[(size_t)blockIdx.y * row_stride + s] = a / double(g.m);
  } else {
    if (lane == 0) s_w[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = s_w[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) t += s_w[w];
      dw[(size_t)blockIdx.y * row_stride + s] = t / double(g.m);
    }
  }
}

__global__ __launch_bounds__(64) void w1_total_kernel(const W1Group* __restrict__ groups, const double* __restrict__ w_tot,
                                                      double* __restrict__ w1) {
  const W1Group g = groups[blockIdx.x];
  double a = 0.0;
  for (int k = threadIdx.x; k < g.n_chunks; k += 64) a += w_tot[g.chunk0 + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) w1[blockIdx.x] = a;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

mythos_w1_plan_t* mythos_w1_plan_create(int n_groups, const int32_t* n_frames, const int32_t* members, const double* samples,
                                        const int64_t* n_ref, const double* ref, const double* ref_weights,
                                        const uint8_t* has_ref_weights, const int64_t* order, int device,
                                        mythos_stream_t stream) {
  if (n_groups < 1 || n_groups > 65535 || !n_frames || !members || !samples || !n_ref || !ref || !order ||
      (has_ref_weights && !ref_weights)) {
    set_error("mythos_w1_plan_create: invalid argument (1 <= n_groups <= 65535)");
    return nullptr;
  }
  std::vector<W1Group> groups(n_groups);
  std::vector<int> chunk_group;
  long long u_off = 0, v_off = 0, o_off = 0, chunks = 0;
  int max_frames = 0, max_members = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (n_frames[g] < 1 || members[g] < 1 || n_ref[g] < 1) {
      set_error("mythos_w1_plan_create: every group needs at least one frame, one member and one reference sample");
      return nullptr;
    }
    W1Group& G = groups[g];
    G.m = members[g], G.frames = n_frames[g], G.pad = 0;
    G.n_u = (long long)n_frames[g] * members[g], G.n_v = n_ref[g];
    G.u_off = u_off, G.v_off = v_off, G.o_off = o_off;
    G.has_vw = (has_ref_weights && has_ref_weights[g]) ? 1 : 0;
    G.uniform = 1.0 / double(G.n_u);
    const long long nc = (G.n_u + G.n_v + kW1Chunk - 1) / kW1Chunk;
    G.chunk0 = (int)chunks, G.n_chunks = (int)nc;
    chunks += nc;
    if (chunks * kW1Chunk >= (1ll << 31)) {
      set_error("mythos_w1_plan_create: more than 2^31 merged entries");
      return nullptr;
    }
    chunk_group.insert(chunk_group.end(), (size_t)nc, g);
    u_off += G.n_u, v_off += G.n_v, o_off += G.n_u + G.n_v;
    max_frames = std::max(max_frames, n_frames[g]);
    max_members = std::max(max_members, members[g]);
  }
  if (select_device(device, "mythos_w1_plan_create")) return nullptr;
  auto p = std::make_unique<mythos_w1_plan>();
  p->n_groups = n_groups, p->max_frames = max_frames, p->max_members = max_members, p->device = device, p->n_chunks = (int)chunks;
  p->n_u_total = u_off;
  const size_t padded = (size_t)chunks * kW1Chunk;
  hipStream_t st = (hipStream_t)stream;
  bool ok = !(p->d_groups.upload(groups) || p->d_chunk_group.upload(chunk_group) || p->d_dx.alloc(padded) || p->d_src.alloc(padded) ||
              p->d_rank.alloc((size_t)p->n_u_total) || p->d_g.alloc(padded) || p->d_part.alloc((size_t)3 * chunks) || p->d_flag.alloc(1));
  // a merge order that is no permutation leaves ranks unwritten: they then point at entry 0, not anywhere
  ok = ok && hipMemsetAsync(p->d_rank.get(), 0, (size_t)p->n_u_total * sizeof(int), st) == hipSuccess &&
       hipMemsetAsync(p->d_flag.get(), 0, sizeof(int), st) == hipSuccess;
  int flag = 0;
  if (ok) {
    hipLaunchKernelGGL(w1_plan_kernel, dim3((unsigned)(chunks * kW1Per)), dim3(kW1Block), 0, st, p->d_groups.get(), p->d_chunk_group.get(),
                       samples, ref, ref_weights, (const long long*)order, p->d_dx.get(), p->d_src.get(), p->d_rank.get(), p->d_flag.get());
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(&flag, p->d_flag.get(), sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
  }
  if (!ok || flag != 0) {
    set_error(!ok ? "mythos_w1_plan_create: device allocation or launch failed"
                  : (flag == 1 ? "mythos_w1_plan_create: the merge order holds an index outside its group"
                     : flag == 3 ? "mythos_w1_plan_create: a reference weight is negative or NaN"
                                 : "mythos_w1_plan_create: the merge order is not ascending (or a sample is NaN)"));
    return nullptr;
  }
  return p.release();
}

void mythos_w1_plan_destroy(mythos_w1_plan_t* p) { delete p; }

int mythos_w1_eval(mythos_w1_plan_t* p, const double* weights, double* w1, double* dw1_dweights, mythos_stream_t stream) {
  if (!p || !w1) {
    set_error("mythos_w1_eval: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int nc = p->n_chunks;
  double *a_tot = p->d_part.get(), *w_tot = p->d_part.get() + nc, *g_tot = p->d_part.get() + 2 * (size_t)nc;
  hipLaunchKernelGGL(w1_chunk_sum_kernel, dim3(nc), dim3(kW1Block), 0, st, p->d_groups.get(), p->d_chunk_group.get(), p->d_src.get(), weights, a_tot);
  hipLaunchKernelGGL(w1_scan_kernel, dim3(nc), dim3(kW1Block), 0, st, p->d_groups.get(), p->d_chunk_group.get(), p->d_dx.get(), p->d_src.get(), weights,
                     a_tot, dw1_dweights ? p->d_g.get() : nullptr, w_tot, g_tot);
  if (dw1_dweights) {
    hipLaunchKernelGGL(w1_suffix_kernel, dim3(nc), dim3(kW1Block), 0, st, p->d_groups.get(), p->d_chunk_group.get(), g_tot, p->d_g.get());
    if (p->max_members >= 512)
      hipLaunchKernelGGL(w1_frame_sum_kernel<kW1Block / 64>, dim3((unsigned)p->max_frames, p->n_groups), dim3(kW1Block), 0, st,
                         p->d_groups.get(), p->d_rank.get(), p->d_g.get(), p->max_frames, dw1_dweights);
    else
      hipLaunchKernelGGL(w1_frame_sum_kernel<1>, dim3((unsigned)((p->max_frames + kW1Block / 64 - 1) / (kW1Block / 64)), p->n_groups),
                         dim3(kW1Block), 0, st, p->d_groups.get(), p->d_rank.get(), p->d_g.get(), p->max_frames, dw1_dweights);
  }
  hipLaunchKernelGGL(w1_total_kernel, dim3(p->n_groups), dim3(64), 0, st, p->d_groups.get(), w_tot, w1);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

}  // extern "C"
