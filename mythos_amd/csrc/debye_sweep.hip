// Debye-Hueckel energy of F frames at T temperatures in one launch: the kernel behind mythos_oxdna_debye_sweep().
//
// Replaces the Debye part of the reference's temperature sweep, vmap(lambda kt: energy_fn.with_params(kt=kt).map(traj))
// (mythos/observables/melting_temp.py:127-140 over mythos/energy/dna2/debye.py:47-110).  kT reaches an oxDNA energy in two
// places only: the stacking strength (affine in kT, the term linear in it - a host-side scale) and the four
// Debye-Hueckel constants.  So the sweep needs one ordinary energy launch plus this: every backbone-backbone distance
// computed ONCE and T constant sets evaluated on it.
//
// Layout: grid = (ceil(N / 32), frames), 256 threads; a group of 8 lanes owns one nucleotide of the tile, as in the
// energy kernel.  Per segment of kSweepCap row entries:
//   1. the groups walk their rows and keep (distance, charge multiplier) of the entries closer than the largest r_cut of
//      the table in their own LDS list (ballot compaction, as gather_row), then the lists are packed into one;
//   2. wavefront w takes the temperatures t = w, w + 4, ...; its 64 lanes stride over the packed list, the sums are folded
//      over the wavefront in a fixed order and added to the tile's accumulator row of that temperature (LDS, touched by
//      that one wavefront only).
// The tile's rows go to HBM as partials; a second small kernel adds the tiles in index order.  No floating-point
// atomics anywhere: results are reproducible bit for bit.  Every pair is met from both of its row entries, so each entry
// carries half of the pair's energy - the weighting of the energy kernel (oxdna_gather.h).
#include "mythos_internal.h"
#include "oxdna_gather.h"

namespace mythos {

constexpr int kSweepBlock = 256;
constexpr int kSweepG = 8;                         // lanes per nucleotide
constexpr int kSweepPPB = kSweepBlock / kSweepG;   // nucleotides per tile
constexpr int kSweepCap = 32;                      // row entries per nucleotide walked at a time
constexpr int kSweepMaxT = 128;                    // temperatures per launch (the host loops over longer tables)
constexpr int kSweepConsts = MYTHOS_DEBYE_SWEEP_CONSTS;  // kappa, prefactor, bsmooth, rcut, rhigh
constexpr int kSweepList = kSweepPPB * kSweepCap;

// PGRAD: also the partials with respect to the five constants (debye_pgrad's, per temperature); row width 1 or 6
template <typename R, int MODEL, bool PGRAD>
__global__ __launch_bounds__(kSweepBlock) void debye_sweep_kernel(
    const R* __restrict__ Pg, const BoxT<R> box, int n, const R* __restrict__ center, const R* __restrict__ quat,
    const int* __restrict__ meta, const int* __restrict__ rows, const int* __restrict__ row_len, int row_stride, int half_ends,
    const double* __restrict__ consts, int n_kt, R r_max, double* __restrict__ part) {
  static_assert(MODEL == 2 || MODEL == 3, "oxDNA2 and oxRNA2 carry the term in one parameter vector");
  constexpr int W = PGRAD ? 1 + kSweepConsts : 1;
  __shared__ R c_lds[kSweepMaxT][kSweepConsts];
  __shared__ double acc_lds[kSweepMaxT][W];
  __shared__ R grp_r[kSweepPPB][kSweepCap];
  __shared__ float grp_m[kSweepPPB][kSweepCap];
  __shared__ R list_r[kSweepList];
  __shared__ float list_m[kSweepList];
  __shared__ int cnt_lds[kSweepPPB];
  __shared__ int off_lds[kSweepPPB + 1];
  __shared__ int max_len;

  const int frame = blockIdx.y;
  const int grp = threadIdx.x / kSweepG, lane = threadIdx.x % kSweepG;
  const int wave = threadIdx.x >> 6, wlane = threadIdx.x & 63;
  const int i = blockIdx.x * kSweepPPB + grp;
  const size_t fo = (size_t)frame * n;
  const int len = i < n ? row_len[i] : 0;

  for (int k = threadIdx.x; k < n_kt * kSweepConsts; k += kSweepBlock) (&c_lds[0][0])[k] = R(consts[k]);
  for (int k = threadIdx.x; k < n_kt * W; k += kSweepBlock) (&acc_lds[0][0])[k] = 0.0;
  if (threadIdx.x == 0) max_len = 0;
  __syncthreads();
  if (lane == 0) atomicMax(&max_len, len);  // (an integer maximum: the same whatever the order)
  __syncthreads();
  const int tile_len = max_len;

  const ConstParams<R, false> P(Pg);
  const UniGeo<R, MODEL> geo(P);
  const PackedLoader<R> ld{center + fo * 3, quat + fo * 4, meta};
  Nuc<R> self;
  if (i < n) {
    R qs[4];
    ld.load(i, self, qs);
  }
  const int* __restrict__ row = rows + (size_t)(i < n ? i : 0) * row_stride;
  const int gshift = wlane & ~(kSweepG - 1);
  constexpr unsigned int kGroupMask = (1u << kSweepG) - 1u;
  const unsigned int below = (1u << lane) - 1u;

  for (int seg0 = ROW_BONDED_SLOTS; seg0 < tile_len; seg0 += kSweepCap) {
    // 1. this group's entries of the segment inside the largest cut-off
    const int seg_end = min(len, seg0 + kSweepCap);
    int n_in = 0;
    for (int s0 = seg0; s0 < seg_end; s0 += kSweepG) {
      const int s = s0 + lane;
      const int entry = (s < seg_end) ? row[s] : -1;
      bool in = false;
      R r = R(0);
      float mult = 1.0f;
      if (entry >= 0) {
        Nuc<R> other;
        R q4[4];
        ld.load(entry & ROW_INDEX_MASK, other, q4);
        const V3<R> d = geo.back_back(min_image(other.c - self.c, box), self, other);
        r = m_sqrt(dot(d, d));
        in = r < r_max;
        if (half_ends) mult = (self.is_end ? 0.5f : 1.0f) * (other.is_end ? 0.5f : 1.0f);
      }
      const unsigned int m = (unsigned int)(__ballot(in) >> gshift) & kGroupMask;
      if (in) {
        const int at = n_in + __popc(m & below);  // < kSweepCap: a segment has that many entries
        grp_r[grp][at] = r;
        grp_m[grp][at] = mult;
      }
      n_in += __popc(m);
    }
    if (lane == 0) cnt_lds[grp] = n_in;
    __syncthreads();
    if (threadIdx.x <= kSweepPPB) {  // where each group's entries start in the packed list (and, last, its length)
      int o = 0;
      for (int g = 0; g < (int)threadIdx.x; ++g) o += cnt_lds[g];
      off_lds[threadIdx.x] = o;
    }
    __syncthreads();
    for (int k = lane; k < n_in; k += kSweepG) {
      list_r[off_lds[grp] + k] = grp_r[grp][k];
      list_m[off_lds[grp] + k] = grp_m[grp][k];
    }
    __syncthreads();
    // 2. every temperature on the packed list
    const int total = off_lds[kSweepPPB];
    for (int t = wave; t < n_kt; t += kSweepBlock / 64) {
      const DebyeP<R> p{c_lds[t][3], c_lds[t][4], c_lds[t][0], c_lds[t][1], c_lds[t][2]};  // rcut, rhigh, kappa, prefactor, bsmooth
      double e = 0.0, g_kappa = 0.0, g_pref = 0.0, g_bs = 0.0, g_rcut = 0.0;
      for (int k = wlane; k < total; k += 64) {
        const R r = list_r[k], mult = R(list_m[k]);
        e += double(mult * debye_eval(r, p).f);
        if constexpr (PGRAD) {  // debye_pgrad (oxdna_math.h)
          if (r < p.rcut) {
            if (r < p.rhigh) {
              const R ex = m_exp(-p.kappa * r) / r;
              g_kappa += double(-mult * r * ex * p.prefactor);
              g_pref += double(mult * ex);
            } else {
              const R dr = r - p.rcut;
              g_bs += double(mult * dr * dr);
              g_rcut += double(-mult * R(2) * p.bsmooth * dr);
            }
          }
        }
      }
      e = group_sum<64>(e);
      if constexpr (PGRAD) {
        g_kappa = group_sum<64>(g_kappa), g_pref = group_sum<64>(g_pref), g_bs = group_sum<64>(g_bs), g_rcut = group_sum<64>(g_rcut);
      }
      if (wlane == 0) {
        acc_lds[t][0] += e;
        if constexpr (PGRAD) {
          acc_lds[t][1] += g_kappa, acc_lds[t][2] += g_pref, acc_lds[t][3] += g_bs, acc_lds[t][4] += g_rcut;  // [5], rhigh: 0
        }
      }
    }
    __syncthreads();  // the lists are rewritten by the next segment
  }
  __syncthreads();
  double* __restrict__ out = part + ((size_t)frame * gridDim.x + blockIdx.x) * n_kt * W;
  for (int k = threadIdx.x; k < n_kt * W; k += kSweepBlock) out[k] = 0.5 * (&acc_lds[0][0])[k];  // half a pair per row entry
}

// e_dh[t][frame] = sum over tiles of part[frame][tile][t][0]; de[t][frame][k] likewise of [1 + k].  One thread per output,
// the tiles added in index order (the reduce_partials_few_kernel pattern of the energy call: a melting-temperature duplex
// is a tile or two per frame).
__global__ __launch_bounds__(256) void debye_sweep_reduce_kernel(const double* __restrict__ part, int n_frames, int n_tiles, int n_kt,
                                                                  int width, size_t frames_total, int frame0,
                                                                  double* __restrict__ e_dh, double* __restrict__ de) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t count = (size_t)n_frames * n_kt * width;
  if (idx >= count) return;
  const int k = (int)(idx % width);
  const int t = (int)((idx / width) % n_kt);
  const int f = (int)(idx / ((size_t)width * n_kt));
  const double* p = part + ((size_t)f * n_tiles * n_kt + t) * width + k;
  double s = 0.0;
  for (int b = 0; b < n_tiles; ++b) s += p[(size_t)b * n_kt * width];
  const size_t row = (size_t)t * frames_total + frame0 + f;
  if (k == 0) e_dh[row] = s;
  else de[row * kSweepConsts + (k - 1)] = s;
}

template <typename R, int MODEL>
static int sweep_typed(mythos_system* sys, const R* center, const R* quat, int n_frames, int n_kt, const double* dh_consts,
                       double* e_dh, double* de_dconsts, hipStream_t stream) {
  const int n = sys->n;
  const int tiles = (n + kSweepPPB - 1) / kSweepPPB;
  const int width = de_dconsts ? 1 + kSweepConsts : 1;
  // the table goes up in the stream's order: a sweep still running on it has read its own before this one lands
  if (int rc = sys->d_sweep_consts.grow((size_t)n_kt * kSweepConsts)) return rc;
  MYTHOS_HIP_TRY(hipMemcpyAsync(sys->d_sweep_consts.get(), dh_consts, (size_t)n_kt * kSweepConsts * sizeof(double), hipMemcpyHostToDevice, stream));
  // frames per launch: the 65535 limit of grid.y and at most 64 MB of tile partials
  const int kt_chunk = std::min(n_kt, kSweepMaxT);
  const size_t per_frame = (size_t)tiles * kt_chunk * width * sizeof(double);
  int chunk = (int)std::min<size_t>(65535, std::max<size_t>(1, (size_t(64) << 20) / per_frame));
  chunk = std::min(chunk, n_frames);
  if (int rc = sys->d_sweep_part.grow((size_t)chunk * tiles * kt_chunk * width)) return rc;
  const BoxT<R> box = make_box<R>(sys);
  const int half_ends = sys->pd.v[DH_HALF_CHARGED_ENDS] != 0.0 ? 1 : 0;
  for (int t0 = 0; t0 < n_kt; t0 += kSweepMaxT) {
    const int nt = std::min(kSweepMaxT, n_kt - t0);
    double r_max = 0.0;
    for (int t = t0; t < t0 + nt; ++t) r_max = std::max(r_max, dh_consts[(size_t)t * kSweepConsts + 3]);
    const double* consts = sys->d_sweep_consts.get() + (size_t)t0 * kSweepConsts;
    const int rc = for_frame_chunks(n_frames, chunk, [&](int f0, int nf) {
      const R* c = center + (size_t)f0 * n * 3;
      const R* q = quat + (size_t)f0 * n * 4;
      auto launch = [&](auto pgrad) {
        hipLaunchKernelGGL((debye_sweep_kernel<R, MODEL, decltype(pgrad)::value>), dim3(tiles, nf), dim3(kSweepBlock), 0, stream,
                           device_params_of<R>(sys), box, n, c, q, sys->d_meta.get(), sys->list.d_rows.get(), sys->d_row_len.get(),
                           sys->list.stride, half_ends, consts, nt, R(r_max), sys->d_sweep_part.get());
      };
      if (de_dconsts) launch(std::true_type{}); else launch(std::false_type{});
      MYTHOS_HIP_TRY(hipGetLastError());
      const size_t count = (size_t)nf * nt * width;
      hipLaunchKernelGGL(debye_sweep_reduce_kernel, dim3((unsigned int)((count + 255) / 256)), dim3(256), 0, stream, sys->d_sweep_part.get(),
                         nf, tiles, nt, width, (size_t)n_frames, f0, e_dh + (size_t)t0 * n_frames,
                         de_dconsts ? de_dconsts + (size_t)t0 * n_frames * kSweepConsts : nullptr);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
    if (rc) return rc;
  }
  return MYTHOS_OK;
}

}  // namespace mythos

using namespace mythos;

extern "C" int mythos_oxdna_debye_sweep(mythos_system_t* s, const void* center, const void* quat, int n_frames, int n_kt,
                                        const double* dh_consts, double* e_dh, double* de_dconsts, mythos_stream_t stream) {
  if (!s || n_frames < 0 || n_kt < 0 || (n_frames > 0 && n_kt > 0 && (!center || !quat || !dh_consts || !e_dh))) {
    set_error("mythos_oxdna_debye_sweep: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (s->model != 2 && s->model != 3) {
    set_error(s->model == 4 ? "mythos_oxdna_debye_sweep: an oxNA system has three Debye-Hueckel constant sets per temperature; "
                              "evaluate it once per temperature (mythos_oxdna_energy)"
                            : "mythos_oxdna_debye_sweep: oxDNA1 has no Debye-Hueckel term");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->params_set || !s->nbrs_set) {
    set_error("mythos_oxdna_debye_sweep: parameters and neighbours must be set first");
    return MYTHOS_ERR_NOT_READY;
  }
  if (n_frames == 0 || n_kt == 0) return MYTHOS_OK;  // an empty batch or table (its buffers may be null) is not an error
  for (size_t k = 0; k < (size_t)n_kt * kSweepConsts; ++k)
    if (!std::isfinite(dh_consts[k])) {
      set_error("mythos_oxdna_debye_sweep: the constant table holds a NaN or an infinity");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  return with_real(s->dtype, [&](auto r) {
    using R = decltype(r);
    if (s->model == 2) return sweep_typed<R, 2>(s, (const R*)center, (const R*)quat, n_frames, n_kt, dh_consts, e_dh, de_dconsts, st);
    return sweep_typed<R, 3>(s, (const R*)center, (const R*)quat, n_frames, n_kt, dh_consts, e_dh, de_dconsts, st);
  });
}
