// MBAR, the binless form of WHAM: per-frame unbiasing weights of N frames pooled from K biased windows, and the binned
// sums behind a free-energy profile over them.  Definitions and the measured timings: DESIGN section 3.5o.  The reference
// has no such estimator; the equations are those of Shirts and Chodera (J. Chem. Phys. 129, 124105, 2008), iterated as
//
//     L_n  = ln sum_j N_j exp(f_j - b_j(n))            t_kn = N_k exp(f_k - b_k(n) - L_n)  in (0, 1],  sum_k t_kn = 1
//     f_k' = f_k - ln(sum_n t_kn / N_k)                gauge f_0 = 0
//
// which is f_k' = -ln sum_n exp(-b_k(n) - L_n) written with the responsibilities t_kn: only L_n needs a running maximum,
// the per-window sums are plain sums of numbers <= 1.  All arithmetic is double.
//
// mbar_iterate_kernel<SRC>: a workgroup of 256 threads takes chunks of 1024 frames, four per thread (four independent
// exp chains: the kernel is bound by K N exponentials, twice per iteration), at most 1024 workgroups striding the chunks.
// SRC = 0 forms b_k(n) = sum_p A_kp (xi_np - C_kp)^2 + B_kp xi_np from the frames' coordinates and the lowered window
// table in LDS - umbrella: A = beta k / 2, C = init, B = 0; constant force: A = 0, B = beta k - and never stores the K x N
// matrix; SRC = 1 reads the caller's u[k][n].  Pass 1 over k is an online log-sum-exp per frame and writes L_n; pass 2
// forms t_kn again and sums it per window: over the four frames of a thread, over the wavefront in a fixed DPP / readlane
// order, into the wavefront's own LDS row chunk after chunk, and at the end the four rows in order into one partial per
// (workgroup, window).  No atomics: the same bits run after run.  No per-thread array indexed by k: no scratch.
// mbar_finish_kernel: one workgroup of 1024; a wavefront adds the partials of a window - lane l those of workgroups l,
// l + 64, ... in order, then the wavefront sum above - and the workgroup writes f' with f'_0 = 0 in place and
// max_k |f' - f| into one device word - the only thing the host reads, once per check_every iterations.
// mbar_binned_sum_kernel: one workgroup per bin sums w_n exp(lw_n - shift) over the bin's segment of a frame order sorted
// by bin, thread-strided then block_sum; one more workgroup sums every frame the same way (the normalisation).
//
// The Gram matrix G = W^T W of the window weights W_nk = exp(f_k - b_k(n) - L_n) = t_kn / N_k - the Hessian of a Newton step
// and the asymptotic covariance both are functions of it - and the segment moments sum_{n in segment} v_n W_nk.  W is N x K
// and, like the bias matrix, never stored.  Both entry points queue the L-pass (the iterate kernel without partials) first.
// mbar_gram_kernel<SRC>: the windows in tiles of 64, the upper-triangle tile pairs only.  A workgroup of 256 takes one tile
// pair (blockIdx.y) and the frame chunks blockIdx.x, blockIdx.x + gridDim.x, ...; per step of F <= 32 frames it forms the two
// 64-column strips of W in LDS (one strip on a diagonal pair) - entry e of the step is frame e % F, column e / F, so xi, L
// and the matrix rows are read along the frames and the table row of a column is an LDS broadcast; the strip rows are padded
// by two doubles against the bank conflict of that store - and then every thread adds the F outer products into its 4 x 4
// block of the tile, in registers, by fma in frame order (a diagonal tile is exactly symmetric: the product commutes).  Only
// the table rows of the pair's windows are staged, so F follows from what K (3 P + 1) leaves of the 64 KB.  One partial
// tile per (frame block, tile pair); the number of frame blocks is at most 1024 / pairs: the partials stay below 32 MB.
// mbar_gram_finish_kernel: a thread per tile entry adds the frame blocks' partials in index order and writes the entry and,
// off the diagonal tiles, its mirror image.
// mbar_segment_kernel<SRC>: the iterate kernel's pass 2 over a segment of a frame order - 256 x 4 frames per round, per
// window the threads' four terms v_n W_nk, mbar_wave_sum, the wavefront's LDS row, the four rows in order.  blockIdx.x is the
// segment; the rounds of a segment are dealt to gridDim.y workgroups (as many as keep segments x splits <= 1024: one segment
// over all frames - the column sums a Newton step needs at every candidate - is not left to one workgroup), whose partials
// mbar_segment_finish_kernel adds in index order.  The split is a function of N and the number of segments alone.
//
// The block bootstrap's weighted sums (mythos_mbar_boot_colsums, mythos_mbar_boot_binned).  Replicate b weights frame n by an
// integer multiplicity m_bn and solves sum_n m_bn W_bnk = 1; about the solved f^ with delta_b = f_b - f^ and the
// responsibilities t^_jn = N_j exp(f^_j - b_j(n) - L^_n) at f^ (sum_j t^_jn = 1),
//     D_bn = sum_j t^_jn e^{delta_bj}       W_bnk = t^_kn e^{delta_bk} / (N_k D_bn)       e^{lw_bn} = e^{-L^_n} / D_bn
// mbar_boot_kernel<SRC, MODE>: a workgroup of 256 takes a tile of 32 replicates and walks its frames 32 at a time.  Per step
// it forms the 32 x K strip of t^ in LDS - the step's only exponentials, shared by the tile's replicates: K / 32 per frame
// and replicate -, then D of its 32 x 32 (replicate, frame) pairs, four per thread over one read of the strip, a dot
// product of K fmas in window order against the tile's e^{delta} rows in LDS, and q_bn = m_bn / D_bn into LDS.  MODE 0 (the
// column sums): thread (window k of a tile of 64, eight replicates) adds q_bn t^_kn of the step's frames into eight registers
// by fma in frame order; the k tiles and the replicate tiles are blockIdx.z.  MODE 1 (the binned sums): thread (replicate,
// column e) adds q_bn e^{-L^_n - shift} v_ne.  Frames are dealt in rounds of 1 024 to gridDim.y workgroups as in the segment
// kernel, whose partials the finish kernels add in index order (and scale by e^{delta_bk} / N_k).  Plain fma, no MFMA: see
// DESIGN.  W, D and the bias matrix are never stored; no atomics, no per-thread array indexed at run time.
#include <cmath>
#include <memory>
#include <vector>

#include "device_buf.h"
#include "mbar_checks.h"
#include "wave_ops.h"

struct mythos_mbar {
  int K = 0, P = 0, device = 0, src = -1;  // src: -1 nothing set, 0 window table + xi, 1 matrix
  int64_t N = 0;
  int n_chunks = 0, n_blocks = 0;
  const double* xi = nullptr;  // borrowed: dev double[N][P]
  const double* u = nullptr;   // borrowed: dev double[K][N]
  mythos::DeviceBuf<double> d_table;    // [K][P][3] A, B, C
  mythos::DeviceBuf<double> d_ln_nk;    // [K]
  mythos::DeviceBuf<double> d_L;        // [N]
  mythos::DeviceBuf<double> d_partial;  // [K][n_blocks]
  mythos::DeviceBuf<double> d_gram_partial;  // [frame blocks][tile pairs][64][64]: allocated by the first mythos_mbar_gram
  mythos::DeviceBuf<double> d_seg_partial;   // [segments][splits][K]: grown by mythos_mbar_segment_moments where splits > 1
  mythos::DeviceBuf<double> d_boot_exp;      // [B][K] e^{delta}: grown by the bootstrap entry points
  mythos::DeviceBuf<double> d_boot_partial;  // [splits][B][K] or [B][segments][splits][E]
  ~mythos_mbar() { (void)hipSetDevice(device); }  // the members free themselves, on the handle's device
};

namespace mythos {

constexpr int kMbarBlock = 256;
constexpr int kMbarFpt = 4;                         // frames per thread and chunk
constexpr int kMbarChunk = kMbarBlock * kMbarFpt;   // frames per chunk
constexpr int kMbarMaxBlocks = 1024;                // the grid's cap: four workgroups per CU; the rest is strided
constexpr int kMbarWaves = kMbarBlock / 64;
constexpr int kMbarFinishBlock = 1024;              // the one workgroup of the finish kernel: sixteen windows at a time
constexpr int kGramTile = 64;                       // windows per tile: 16 x 16 threads own 4 x 4 entries each
constexpr int kGramTileSize = kGramTile * kGramTile;
constexpr int kGramPad = 2;                         // doubles behind a strip row in LDS
constexpr int kGramLog2Frames = 5;                  // at most 32 frames per strip step
constexpr int kGramMaxPartials = 1024;              // (frame block, tile pair) partial tiles of 32 KB each
constexpr int kSegMaxSplits = 1024;                 // segments x splits of the segment kernel

// Sum over the wavefront, wave-uniform, in a fixed order: DPP butterfly inside each row of 16, then the four rows in order.
// Every lane must be enabled.
__device__ __forceinline__ double mbar_wave_sum(double v) {
  v = group_sum<16>(v);
  return ((read_lane(v, 0) + read_lane(v, 16)) + read_lane(v, 32)) + read_lane(v, 48);
}

// max that keeps a NaN once it has one (a diverged iteration must not look converged)
__device__ __forceinline__ double mbar_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

template <int SRC>
__global__ __launch_bounds__(kMbarBlock) void mbar_iterate_kernel(int K, int P, long long N, int n_chunks, const double* __restrict__ xi,
                                                                   const double* __restrict__ table, const double* __restrict__ u,
                                                                   const double* __restrict__ ln_nk, const double* __restrict__ f,
                                                                   double* __restrict__ L_out, double* __restrict__ lw_out,
                                                                   double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double mbar_lds[];
  double* __restrict__ s_tab = mbar_lds;                  // [K][P][3]
  double* __restrict__ s_a = s_tab + 3 * (size_t)K * P;   // [K] ln N_k + f_k
  double* __restrict__ s_part = s_a + K;                  // [kMbarWaves][K]
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if (SRC == 0)
    for (int i = tid; i < 3 * K * P; i += kMbarBlock) s_tab[i] = table[i];
  for (int k = tid; k < K; k += kMbarBlock) s_a[k] = ln_nk[k] + f[k];
  for (int i = tid; i < kMbarWaves * K; i += kMbarBlock) s_part[i] = 0.0;
  __syncthreads();

  // b_k(n) of frame slot j: its first coordinate from a register, further ones through the cache
  auto bias = [&](int k, long long n, double x0) {
    if constexpr (SRC == 1) return u[(size_t)k * (size_t)N + (size_t)n];
    const double* __restrict__ q = s_tab + 3 * (size_t)k * P;
    double b = 0.0;
    for (int p = 0; p < P; ++p) {
      const double x = p == 0 ? x0 : xi[(size_t)n * P + p];
      const double d = x - q[3 * p + 2];
      b += q[3 * p] * d * d + q[3 * p + 1] * x;
    }
    return b;
  };

  for (int chunk = (int)blockIdx.x; chunk < n_chunks; chunk += (int)gridDim.x) {
    long long n[kMbarFpt];
    bool own[kMbarFpt];
    double x0[kMbarFpt], m[kMbarFpt], s[kMbarFpt], L[kMbarFpt];
#pragma unroll
    for (int j = 0; j < kMbarFpt; ++j) {
      const long long at = (long long)chunk * kMbarChunk + j * kMbarBlock + tid;
      own[j] = at < N;
      n[j] = own[j] ? at : N - 1;  // a slot past the end reads the last frame and adds nothing
      x0[j] = SRC == 0 ? xi[(size_t)n[j] * P] : 0.0;
      m[j] = s_a[0] - bias(0, n[j], x0[j]);
      s[j] = 1.0;
    }
    for (int k = 1; k < K; ++k) {
      const double a0 = s_a[k];
#pragma unroll
      for (int j = 0; j < kMbarFpt; ++j) {
        const double a = a0 - bias(k, n[j], x0[j]);
        const double e = exp(-fabs(a - m[j]));
        s[j] = a > m[j] ? s[j] * e + 1.0 : s[j] + e;
        m[j] = fmax(a, m[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kMbarFpt; ++j) {
      L[j] = m[j] + log(s[j]);
      if (own[j]) {
        L_out[n[j]] = L[j];
        if (lw_out) lw_out[n[j]] = -L[j];
      }
    }
    if (!partial) continue;  // the log-weights alone (uniform over the launch)
    for (int k = 0; k < K; ++k) {
      const double a0 = s_a[k];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kMbarFpt; ++j) {
        const double t = exp(a0 - bias(k, n[j], x0[j]) - L[j]);
        acc += own[j] ? t : 0.0;
      }
      const double w = mbar_wave_sum(acc);
      if ((tid & 63) == 0) s_part[(size_t)wave * K + k] += w;
    }
  }
  if (!partial) return;
  __syncthreads();
  for (int k = tid; k < K; k += kMbarBlock) {
    double t = s_part[k];
#pragma unroll
    for (int w = 1; w < kMbarWaves; ++w) t += s_part[(size_t)w * K + k];
    partial[(size_t)k * gridDim.x + blockIdx.x] = t;  // window-major: the finish kernel reads a window's row
  }
}

__global__ __launch_bounds__(kMbarFinishBlock) void mbar_finish_kernel(int K, int n_blocks, const double* __restrict__ partial,
                                                                        const double* __restrict__ ln_nk, double* __restrict__ f,
                                                                        double* __restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) double s_raw[];  // [K] f' before the gauge
  __shared__ double s_max[kMbarFinishBlock];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  // a wavefront per window: its lanes stride the window's row of workgroup partials (independent, coalesced loads - one
  // thread per window was a chain of n_blocks dependent loads, as long as the iterate kernel itself), then the fixed-order sum
  for (int k = tid >> 6; k < K; k += kMbarFinishBlock / 64) {
    double t = 0.0;
    for (int b = lane; b < n_blocks; b += 64) t += partial[(size_t)k * n_blocks + b];
    t = mbar_wave_sum(t);
    if (lane == 0) s_raw[k] = f[k] - (log(t) - ln_nk[k]);  // f_k - ln(sum_n t_kn / N_k)
  }
  __syncthreads();
  const double f0 = s_raw[0];
  double d = 0.0;
  for (int k = tid; k < K; k += kMbarFinishBlock) {
    const double g = s_raw[k] - f0;
    d = mbar_max_nan(d, fabs(g - f[k]));
    f[k] = g;
  }
  s_max[tid] = d;
  __syncthreads();
  for (int o = kMbarFinishBlock / 2; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = mbar_max_nan(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  if (tid == 0) *delta = s_max[0];
}

__global__ __launch_bounds__(kMbarBlock) void mbar_binned_sum_kernel(int n_bins, long long N, const long long* __restrict__ seg,
                                                                      const long long* __restrict__ order, const double* __restrict__ lw,
                                                                      const double* __restrict__ weights, double shift,
                                                                      double* __restrict__ out) {
  __shared__ double s_red[kMbarWaves];
  const int b = (int)blockIdx.x;
  long long lo = 0, hi = N;  // workgroup n_bins: every frame
  if (b < n_bins) lo = min(max(seg[b], 0ll), N), hi = min(max(seg[b + 1], lo), N);
  double acc = 0.0;
  for (long long i = lo + (int)threadIdx.x; i < hi; i += kMbarBlock) {
    const long long n = order[i];
    if (n < 0 || n >= N) continue;  // (not a permutation: the caller's fault, memory stays in bounds)
    acc += (weights ? weights[n] : 1.0) * exp(lw[n] - shift);
  }
  const double total = block_sum(acc, s_red);
  if (threadIdx.x == 0) out[b] = total;
}

// b_k(n) for the Gram and segment kernels: q the window's table row [P][3] in LDS, x0 the frame's first coordinate
template <int SRC>
__device__ __forceinline__ double mbar_bias(const double* __restrict__ q, const double* __restrict__ xi, const double* __restrict__ u,
                                            int P, long long N, int k, long long n, double x0) {
  if constexpr (SRC == 1) return u[(size_t)k * (size_t)N + (size_t)n];
  double b = 0.0;
  for (int p = 0; p < P; ++p) {
    const double x = p == 0 ? x0 : xi[(size_t)n * P + p];
    const double d = x - q[3 * p + 2];
    b += q[3 * p] * d * d + q[3 * p + 1] * x;
  }
  return b;
}

// tile pair `pair` of the upper triangle, row by row: (0,0) (0,1) ... (0,T-1) (1,1) ...
__device__ __forceinline__ void mbar_tile_pair(int T, int pair, int& ti, int& tj) {
  ti = 0;
  while (pair >= T - ti) pair -= T - ti, ++ti;
  tj = ti + pair;
}

// what the host and the kernel agree on: columns of a strip step, staged table rows, doubles in front of the strips (even)
constexpr int mbar_gram_width(int K) { return K > kGramTile ? 2 * kGramTile : kGramTile; }
constexpr int mbar_gram_rows(int K) { return K < mbar_gram_width(K) ? K : mbar_gram_width(K); }
constexpr size_t mbar_gram_head(int K, int P, int src) {
  const size_t d = (size_t)mbar_gram_rows(K) * ((src == 0 ? 3 * (size_t)P : 0) + 1);
  return d + (d & 1);
}

template <int SRC>
__global__ __launch_bounds__(kMbarBlock) void mbar_gram_kernel(int K, int P, long long N, int n_chunks, int log2_frames,
                                                                const double* __restrict__ xi, const double* __restrict__ table,
                                                                const double* __restrict__ u, const double* __restrict__ f,
                                                                const double* __restrict__ L, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double mbar_lds[];
  const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int ti, tj;
  mbar_tile_pair((K + kGramTile - 1) / kGramTile, (int)blockIdx.y, ti, tj);
  const bool diag = ti == tj;
  // a pair's valid columns are the first n_cols: only the last tile is short, and it is tile j or the diagonal's own
  const int n_cols = min(kGramTile, K - kGramTile * ti) + (diag ? 0 : min(kGramTile, K - kGramTile * tj));
  const int width = diag ? kGramTile : 2 * kGramTile, stride = mbar_gram_width(K) + kGramPad, frames = 1 << log2_frames;
  const int row = SRC == 0 ? 3 * P : 0;
  double* __restrict__ s_tab = mbar_lds;                               // [rows][P][3]
  double* __restrict__ s_f = s_tab + (size_t)mbar_gram_rows(K) * row;  // [rows]
  double* __restrict__ s_w = mbar_lds + mbar_gram_head(K, P, SRC);     // [frames][stride]
  auto window = [&](int c) { return c < kGramTile ? kGramTile * ti + c : kGramTile * tj + c - kGramTile; };
  if constexpr (SRC == 0)
    for (int i = tid; i < n_cols * row; i += kMbarBlock) s_tab[i] = table[(size_t)window(i / row) * row + i % row];
  for (int c = tid; c < n_cols; c += kMbarBlock) s_f[c] = f[window(c)];
  __syncthreads();

  double acc[4][4] = {};
  for (int chunk = (int)blockIdx.x; chunk < n_chunks; chunk += (int)gridDim.x) {
    const long long end = min((long long)(chunk + 1) * kMbarChunk, N);
    for (long long base = (long long)chunk * kMbarChunk; base < end; base += frames) {
      for (int e = tid; e < width << log2_frames; e += kMbarBlock) {
        const int fr = e & (frames - 1), c = e >> log2_frames;
        const long long n = base + fr;
        double w = 0.0;  // a column past K, a frame past N: a zero that adds nothing
        if (c < n_cols && n < N) {
          const double x0 = SRC == 0 ? xi[(size_t)n * P] : 0.0;
          w = exp(s_f[c] - mbar_bias<SRC>(s_tab + (size_t)c * row, xi, u, P, N, window(c), n, x0) - L[n]);
        }
        s_w[fr * stride + c] = w;
      }
      __syncthreads();
      const int n_fr = (int)min((long long)frames, end - base);
      for (int fr = 0; fr < n_fr; ++fr) {
        const double* __restrict__ a = s_w + fr * stride + 4 * ty;
        const double* __restrict__ b = s_w + fr * stride + (diag ? 0 : kGramTile) + 4 * tx;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
  }
  double* __restrict__ dst = partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * kGramTileSize;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(4 * ty + i) * kGramTile + 4 * tx + j] = acc[i][j];
}

// grid (tile pairs, kGramTileSize / kMbarBlock)
__global__ __launch_bounds__(kMbarBlock) void mbar_gram_finish_kernel(int K, int n_fb, const double* __restrict__ partial,
                                                                       double* __restrict__ gram) {
  int ti, tj;
  mbar_tile_pair((K + kGramTile - 1) / kGramTile, (int)blockIdx.x, ti, tj);
  const int e = (int)blockIdx.y * kMbarBlock + (int)threadIdx.x;
  double t = 0.0;
  for (int b = 0; b < n_fb; ++b) t += partial[((size_t)b * gridDim.x + blockIdx.x) * kGramTileSize + e];
  const int gi = kGramTile * ti + e / kGramTile, gj = kGramTile * tj + e % kGramTile;
  if (gi >= K || gj >= K) return;
  gram[(size_t)gi * K + gj] = t;
  if (ti != tj) gram[(size_t)gj * K + gi] = t;  // (a diagonal tile holds both of its triangles, bit for bit)
}

// grid (segments, splits); dst [segment][split][K]
template <int SRC>
__global__ __launch_bounds__(kMbarBlock) void mbar_segment_kernel(int K, int P, long long N, const long long* __restrict__ seg,
                                                                   const long long* __restrict__ order, const double* __restrict__ v,
                                                                   const double* __restrict__ xi, const double* __restrict__ table,
                                                                   const double* __restrict__ u, const double* __restrict__ f,
                                                                   const double* __restrict__ L, double* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double mbar_lds[];
  double* __restrict__ s_tab = mbar_lds;                  // [K][P][3]
  double* __restrict__ s_a = s_tab + 3 * (size_t)K * P;   // [K] f_k
  double* __restrict__ s_part = s_a + K;                  // [kMbarWaves][K]
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if (SRC == 0)
    for (int i = tid; i < 3 * K * P; i += kMbarBlock) s_tab[i] = table[i];
  for (int k = tid; k < K; k += kMbarBlock) s_a[k] = f[k];
  for (int i = tid; i < kMbarWaves * K; i += kMbarBlock) s_part[i] = 0.0;
  __syncthreads();
  long long lo = 0, hi = N;  // no order: every frame, in natural order
  if (order) lo = min(max(seg[blockIdx.x], 0ll), N), hi = min(max(seg[blockIdx.x + 1], lo), N);
  for (long long at = lo + (long long)blockIdx.y * kMbarChunk; at < hi; at += (long long)gridDim.y * kMbarChunk) {
    long long n[kMbarFpt];
    double x0[kMbarFpt], vn[kMbarFpt], Ln[kMbarFpt];
#pragma unroll
    for (int j = 0; j < kMbarFpt; ++j) {
      const long long i = at + j * kMbarBlock + tid;
      long long m = i < hi ? (order ? order[i] : i) : -1;
      const bool own = m >= 0 && m < N;  // (not a permutation: the entry is skipped, memory stays in bounds)
      n[j] = own ? m : 0;                // a slot without a frame reads frame 0 and adds 0 times its weight
      vn[j] = own ? (v ? v[n[j]] : 1.0) : 0.0;
      x0[j] = SRC == 0 ? xi[(size_t)n[j] * P] : 0.0;
      Ln[j] = L[n[j]];
    }
    for (int k = 0; k < K; ++k) {
      const double a0 = s_a[k];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kMbarFpt; ++j)
        acc += vn[j] * exp(a0 - mbar_bias<SRC>(s_tab + 3 * (size_t)k * P, xi, u, P, N, k, n[j], x0[j]) - Ln[j]);
      const double w = mbar_wave_sum(acc);
      if ((tid & 63) == 0) s_part[(size_t)wave * K + k] += w;
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += kMbarBlock) {
    double t = s_part[k];
#pragma unroll
    for (int w = 1; w < kMbarWaves; ++w) t += s_part[(size_t)w * K + k];
    dst[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * K + k] = t;
  }
}

// grid (segments)
__global__ __launch_bounds__(kMbarBlock) void mbar_segment_finish_kernel(int K, int splits, const double* __restrict__ partial,
                                                                          double* __restrict__ out) {
  for (int k = (int)threadIdx.x; k < K; k += kMbarBlock) {
    double t = 0.0;
    for (int s = 0; s < splits; ++s) t += partial[((size_t)blockIdx.x * splits + s) * K + k];
    out[(size_t)blockIdx.x * K + k] = t;
  }
}

// ---- the block bootstrap's weighted sums ------------------------------------------------------------------------------
constexpr int kBootTile = 32;     // replicates per workgroup
constexpr int kBootFrames = 32;   // frames per step
constexpr int kBootCols = 64;     // windows per workgroup of the column sums
constexpr int kBootMaxE = 8;      // columns of v per call of the binned sums: kBootTile * kBootMaxE threads own one sum each
constexpr int kBootMaxB = 1 << 16;
constexpr int boot_stride(int K) { return K | 1; }  // odd: the strip's rows start in different banks
// doubles of LDS: table, ln N + f^, e^{delta} rows, strip, q, e^{-L - shift}, v, and the step's frame indices
constexpr size_t mbar_boot_lds_doubles(int K, int P, int src) {
  return (size_t)K * ((src == 0 ? 3 * (size_t)P : 0) + 1) + (size_t)kBootTile * K + (size_t)kBootFrames * boot_stride(K) +
         (size_t)kBootTile * kBootFrames + kBootFrames + (size_t)kBootFrames * kBootMaxE + kBootFrames;
}

__global__ __launch_bounds__(kMbarBlock) void mbar_boot_exp_kernel(long long count, const double* __restrict__ delta, double* __restrict__ ed) {
  const long long i = (long long)blockIdx.x * kMbarBlock + threadIdx.x;
  if (i < count) ed[i] = exp(delta[i]);
}

// grid (segments, splits, tiles).  MODE 0: dst [split][B][K], tiles = replicate tiles x window tiles, one segment;
// MODE 1: dst [B][segments][splits][E], tiles = replicate tiles.
template <int SRC, int MODE>
__global__ __launch_bounds__(kMbarBlock) void mbar_boot_kernel(int K, int P, long long N, int B, int E, const long long* __restrict__ seg,
                                                                const long long* __restrict__ order, const double* __restrict__ v,
                                                                double shift, const double* __restrict__ xi,
                                                                const double* __restrict__ table, const double* __restrict__ u,
                                                                const double* __restrict__ ln_nk, const double* __restrict__ f,
                                                                const double* __restrict__ L, const double* __restrict__ ed,
                                                                const unsigned short* __restrict__ mult, double* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double mbar_lds[];
  const int row = SRC == 0 ? 3 * P : 0, stride = boot_stride(K);
  double* __restrict__ s_tab = mbar_lds;                               // [K][P][3]
  double* __restrict__ s_a = s_tab + (size_t)K * row;                  // [K] ln N_k + f^_k
  double* __restrict__ s_e = s_a + K;                                  // [kBootTile][K] e^{delta}
  double* __restrict__ s_w = s_e + (size_t)kBootTile * K;              // [kBootFrames][stride] t^
  double* __restrict__ s_q = s_w + (size_t)kBootFrames * stride;       // [kBootTile][kBootFrames] m / D
  double* __restrict__ s_x = s_q + kBootTile * kBootFrames;            // [kBootFrames] e^{-L - shift}
  double* __restrict__ s_v = s_x + kBootFrames;                        // [kBootFrames][E]
  long long* __restrict__ s_n = (long long*)(s_v + kBootFrames * kBootMaxE);  // [kBootFrames] the frames, -1 for none
  const int tid = (int)threadIdx.x;
  const int k_tiles = (K + kBootCols - 1) / kBootCols;
  const int b0 = kBootTile * (MODE == 0 ? (int)blockIdx.z / k_tiles : (int)blockIdx.z);
  const int k0 = MODE == 0 ? kBootCols * ((int)blockIdx.z % k_tiles) : 0;
  if constexpr (SRC == 0)
    for (int i = tid; i < K * row; i += kMbarBlock) s_tab[i] = table[i];
  for (int k = tid; k < K; k += kMbarBlock) s_a[k] = ln_nk[k] + f[k];
  for (int i = tid; i < kBootTile * K; i += kMbarBlock) s_e[i] = b0 + i / K < B ? ed[(size_t)b0 * K + i] : 0.0;
  long long lo = 0, hi = N;  // no order: every frame, in natural order
  if (order) lo = min(max(seg[blockIdx.x], 0ll), N), hi = min(max(seg[blockIdx.x + 1], lo), N);
  double acc[8] = {};  // MODE 0: replicates (tid >> 6) + 4 i of window k0 + (tid & 63); MODE 1: acc[0] of (replicate, column)
  for (long long at = lo + (long long)blockIdx.y * kMbarChunk; at < hi; at += (long long)gridDim.y * kMbarChunk) {
    const long long end = min(at + kMbarChunk, hi);
    for (long long base = at; base < end; base += kBootFrames) {
      if (tid < kBootFrames) {
        const long long i = base + tid;
        const long long m = i < end ? (order ? order[i] : i) : -1;
        const bool own = m >= 0 && m < N;  // (not a permutation: the entry is skipped, memory stays in bounds)
        s_n[tid] = own ? m : -1;
        if constexpr (MODE == 1) s_x[tid] = own ? exp(-L[m] - shift) : 0.0;
      }
      __syncthreads();
      for (int e = tid; e < kBootFrames * K; e += kMbarBlock) {
        const int fr = e & (kBootFrames - 1), c = e / kBootFrames;
        const long long n = s_n[fr];
        double w = 0.0;  // a slot without a frame: a zero that adds nothing
        if (n >= 0) {
          const double x0 = SRC == 0 ? xi[(size_t)n * P] : 0.0;
          w = exp(s_a[c] - mbar_bias<SRC>(s_tab + (size_t)c * row, xi, u, P, N, c, n, x0) - L[n]);
        }
        s_w[fr * stride + c] = w;
      }
      if constexpr (MODE == 1)
        for (int i = tid; i < kBootFrames * E; i += kMbarBlock) {
          const long long n = s_n[i / E];
          s_v[i] = n >= 0 ? (v ? v[(size_t)n * E + i % E] : 1.0) : 0.0;
        }
      __syncthreads();
      {
        const int fr = tid & (kBootFrames - 1), r0 = tid / kBootFrames;  // replicates r0 + 8 i of the tile
        const double* __restrict__ w = s_w + fr * stride;
        const double* __restrict__ e = s_e + (size_t)r0 * K;
        const size_t step = (size_t)(kMbarBlock / kBootFrames) * K;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
        for (int j = 0; j < K; ++j) {
          const double t = w[j];
          d0 = fma(t, e[j], d0), d1 = fma(t, e[step + j], d1), d2 = fma(t, e[2 * step + j], d2), d3 = fma(t, e[3 * step + j], d3);
        }
        const double d[4] = {d0, d1, d2, d3};
        const long long n = s_n[fr];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = r0 + (kMbarBlock / kBootFrames) * i;
          const unsigned m = (n >= 0 && b0 + r < B) ? mult[(size_t)(b0 + r) * (size_t)N + (size_t)n] : 0u;
          double q = m ? (double)m / d[i] : 0.0;
          if constexpr (MODE == 1) q *= s_x[fr];
          s_q[r * kBootFrames + fr] = q;
        }
      }
      __syncthreads();
      if constexpr (MODE == 0) {
        const double* __restrict__ w = s_w + min(k0 + (tid & (kBootCols - 1)), K - 1);  // a window past K: computed, not written
        const double* __restrict__ q = s_q + (tid / kBootCols) * kBootFrames;
        for (int fr = 0; fr < kBootFrames; ++fr) {
          const double t = w[fr * stride];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = fma(q[(kMbarBlock / kBootCols) * kBootFrames * i + fr], t, acc[i]);
        }
      } else if (tid < kBootTile * E) {
        const double* __restrict__ q = s_q + (tid / E) * kBootFrames;
        const double* __restrict__ c = s_v + tid % E;
        for (int fr = 0; fr < kBootFrames; ++fr) acc[0] = fma(q[fr], c[fr * E], acc[0]);
      }
      // (the next step writes s_n and s_x, which nobody reads behind the last barrier, and the rest behind its own first barrier)
    }
  }
  if constexpr (MODE == 0) {
    const int k = k0 + (tid & (kBootCols - 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int b = b0 + tid / kBootCols + (kMbarBlock / kBootCols) * i;
      if (k < K && b < B) dst[((size_t)blockIdx.y * B + b) * K + k] = acc[i];
    }
  } else if (tid < kBootTile * E && b0 + tid / E < B) {
    dst[(((size_t)(b0 + tid / E) * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * E + tid % E] = acc[0];
  }
}

// s_bk = e^{delta_bk} / N_k times the splits' partials in index order; a thread per (b, k)
__global__ __launch_bounds__(kMbarBlock) void mbar_boot_colsums_finish_kernel(long long count, int K, int splits,
                                                                               const double* __restrict__ partial,
                                                                               const double* __restrict__ delta,
                                                                               const double* __restrict__ ln_nk, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kMbarBlock + threadIdx.x;
  if (i >= count) return;
  double t = 0.0;
  for (int s = 0; s < splits; ++s) t += partial[(size_t)s * count + i];
  out[i] = t * exp(delta[i] - ln_nk[i % K]);
}

// out[i] = the splits' partials of entry i = (b, segment, e) in index order, E values each
__global__ __launch_bounds__(kMbarBlock) void mbar_boot_binned_finish_kernel(long long count, int E, int splits,
                                                                              const double* __restrict__ partial, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kMbarBlock + threadIdx.x;
  if (i >= count) return;
  const long long cell = i / E;
  double t = 0.0;
  for (int s = 0; s < splits; ++s) t += partial[((size_t)cell * splits + s) * E + i % E];
  out[i] = t;
}

static int mbar_ready(const mythos_mbar* h, const char* who) {
  if (h->src < 0) {
    set_error(std::string(who) + ": neither windows nor a matrix are set");
    return MYTHOS_ERR_NOT_READY;
  }
  return MYTHOS_OK;
}

static int mbar_set_counts(mythos_mbar* h, const int64_t* n_k) {
  std::vector<double> ln((size_t)h->K);
  for (int k = 0; k < h->K; ++k) ln[k] = std::log((double)n_k[k]);
  return h->d_ln_nk.upload(ln);
}

static void mbar_launch(const mythos_mbar* h, const double* f, double* lw_out, double* partial, hipStream_t st) {
  const size_t lds = sizeof(double) * mbar_lds_doubles(h->K, h->P);
  auto kernel = h->src == 0 ? mbar_iterate_kernel<0> : mbar_iterate_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(h->n_blocks), dim3(kMbarBlock), lds, st, h->K, h->P, (long long)h->N, h->n_chunks, h->xi,
                     h->d_table.get(), h->u, h->d_ln_nk.get(), f, h->d_L.get(), lw_out, partial);
}

// The segment kernel and, where a segment's rounds are split, its finish.  d_L must be current on the stream.
static int mbar_segment_launch(mythos_mbar* h, const double* f, int n_seg, const int64_t* seg_start, const int64_t* order,
                               const double* v, double* out, hipStream_t st) {
  const int splits = std::min(h->n_chunks, std::max(1, kSegMaxSplits / n_seg));
  double* dst = out;
  if (splits > 1) {
    if (int rc = h->d_seg_partial.grow((size_t)n_seg * splits * h->K)) return rc;
    dst = h->d_seg_partial.get();
  }
  const size_t lds = sizeof(double) * mbar_lds_doubles(h->K, h->P);
  auto kernel = h->src == 0 ? mbar_segment_kernel<0> : mbar_segment_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(n_seg, splits), dim3(kMbarBlock), lds, st, h->K, h->P, (long long)h->N, (const long long*)seg_start,
                     (const long long*)order, v, h->xi, h->d_table.get(), h->u, f, h->d_L.get(), dst);
  if (splits > 1)
    hipLaunchKernelGGL(mbar_segment_finish_kernel, dim3(n_seg), dim3(kMbarBlock), 0, st, h->K, splits, dst, out);
  return MYTHOS_OK;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

int mythos_mbar_check(int n_windows, int64_t n_frames, int n_coords, const double* table, const double* kT, const int64_t* n_k,
                      const double* xi, int n_edges, const double* edges) {
  return mbar_check("mythos_mbar_check", n_windows, n_frames, n_coords, table, kT, n_k, xi, n_edges, edges);
}

mythos_mbar_t* mythos_mbar_create(int64_t n_frames, int n_windows, int device) {
  if (n_windows < 1) {
    set_error("mythos_mbar_create: K < 1 (at least one window)");
    return nullptr;
  }
  if (n_frames < 1 || n_frames >= ((int64_t)1 << 31) || mbar_lds_doubles(n_windows, 0) > (size_t)kMbarLdsDoubles) {
    set_error("mythos_mbar_create: 1 <= N < 2^31 frames and at most " + std::to_string(kMbarLdsDoubles / 6) + " windows");
    return nullptr;
  }
  if (select_device(device, "mythos_mbar_create")) return nullptr;
  auto h = std::make_unique<mythos_mbar>();
  h->K = n_windows, h->N = n_frames, h->device = device;
  h->n_chunks = (int)((n_frames + kMbarChunk - 1) / kMbarChunk);
  h->n_blocks = std::min(h->n_chunks, kMbarMaxBlocks);
  if (h->d_L.alloc((size_t)n_frames) || h->d_partial.alloc((size_t)h->n_blocks * n_windows) ||
      h->d_ln_nk.alloc((size_t)n_windows) || h->d_table.alloc(1)) {
    set_error("mythos_mbar_create: device allocation failed");
    return nullptr;
  }
  return h.release();
}

void mythos_mbar_destroy(mythos_mbar_t* h) { delete h; }

int mythos_mbar_set_windows(mythos_mbar_t* h, int n_coords, const double* table, const double* kT, const int64_t* n_k, const double* xi) {
  if (!h || !table || !kT || !n_k || !xi) {
    set_error("mythos_mbar_set_windows: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_check("mythos_mbar_set_windows", h->K, h->N, n_coords, table, kT, n_k, nullptr, 0, nullptr)) return rc;
  const double beta = 1.0 / kT[0];
  std::vector<double> abc(3 * (size_t)h->K * n_coords);
  for (size_t i = 0; i < (size_t)h->K * n_coords; ++i) {
    const double* q = table + i * kMbarRow;
    const bool umbrella = q[0] == MBAR_UMBRELLA;
    abc[3 * i] = umbrella ? 0.5 * beta * q[1] : 0.0;
    abc[3 * i + 1] = umbrella ? 0.0 : beta * q[1];
    abc[3 * i + 2] = umbrella ? q[2] : 0.0;
  }
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());  // no launch in flight reads a table that is being replaced
  if (int rc = h->d_table.upload(abc)) return rc;
  if (int rc = mbar_set_counts(h, n_k)) return rc;
  h->P = n_coords, h->xi = xi, h->u = nullptr, h->src = 0;
  return MYTHOS_OK;
}

int mythos_mbar_set_matrix(mythos_mbar_t* h, const double* u_kn, const int64_t* n_k) {
  if (!h || !u_kn || !n_k) {
    set_error("mythos_mbar_set_matrix: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_check("mythos_mbar_set_matrix", h->K, h->N, 0, nullptr, nullptr, n_k, nullptr, 0, nullptr)) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());
  if (int rc = mbar_set_counts(h, n_k)) return rc;
  h->P = 0, h->xi = nullptr, h->u = u_kn, h->src = 1;
  return MYTHOS_OK;
}

int mythos_mbar_iterate(mythos_mbar_t* h, double* f_inout, int n_iter, double* delta_out, mythos_stream_t stream) {
  if (!h || !f_inout || !delta_out || n_iter < 0) {
    set_error("mythos_mbar_iterate: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_ready(h, "mythos_mbar_iterate")) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  for (int it = 0; it < n_iter; ++it) {
    mbar_launch(h, f_inout, nullptr, h->d_partial.get(), st);
    hipLaunchKernelGGL(mbar_finish_kernel, dim3(1), dim3(kMbarFinishBlock), sizeof(double) * (size_t)h->K, st, h->K, h->n_blocks,
                       h->d_partial.get(), h->d_ln_nk.get(), f_inout, delta_out);
  }
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_mbar_log_weights(mythos_mbar_t* h, const double* f, double* log_weights, mythos_stream_t stream) {
  if (!h || !f || !log_weights) {
    set_error("mythos_mbar_log_weights: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_ready(h, "mythos_mbar_log_weights")) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  mbar_launch(h, f, log_weights, nullptr, (hipStream_t)stream);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_mbar_binned_sum(mythos_mbar_t* h, int n_bins, const int64_t* seg_start, const int64_t* order, const double* log_weights,
                           const double* weights, double shift, double* sums, mythos_stream_t stream) {
  if (!h || n_bins < 1 || n_bins > (1 << 20) || !seg_start || !order || !log_weights || !sums || !std::isfinite(shift)) {
    set_error("mythos_mbar_binned_sum: invalid argument (1 <= n_bins <= 2^20, a finite shift)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(mbar_binned_sum_kernel, dim3(n_bins + 1), dim3(kMbarBlock), 0, (hipStream_t)stream, n_bins, (long long)h->N,
                     (const long long*)seg_start, (const long long*)order, log_weights, weights, shift, sums);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_mbar_gram(mythos_mbar_t* h, const double* f, double* gram, double* colsum, mythos_stream_t stream) {
  if (!h || !f || !gram) {
    set_error("mythos_mbar_gram: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_ready(h, "mythos_mbar_gram")) return rc;
  const int tiles = (h->K + kGramTile - 1) / kGramTile, pairs = tiles * (tiles + 1) / 2;
  const size_t head = mbar_gram_head(h->K, h->P, h->src), step = (size_t)mbar_gram_width(h->K) + kGramPad;
  int log2_frames = kGramLog2Frames;
  while (log2_frames >= 0 && head + (step << log2_frames) > (size_t)kMbarLdsDoubles) --log2_frames;
  if (log2_frames < 0) {
    set_error("mythos_mbar_gram: the window table leaves no LDS for a strip of W (" + std::to_string(head) + " + " +
              std::to_string(step) + " doubles do not fit 64 KB)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int n_fb = std::min(h->n_chunks, std::max(1, kGramMaxPartials / pairs));
  if (int rc = h->d_gram_partial.grow((size_t)n_fb * pairs * kGramTileSize)) return rc;
  mbar_launch(h, f, nullptr, nullptr, st);  // L_n at this f
  auto kernel = h->src == 0 ? mbar_gram_kernel<0> : mbar_gram_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(n_fb, pairs), dim3(kMbarBlock), sizeof(double) * (head + (step << log2_frames)), st, h->K, h->P,
                     (long long)h->N, h->n_chunks, log2_frames, h->xi, h->d_table.get(), h->u, f, h->d_L.get(), h->d_gram_partial.get());
  hipLaunchKernelGGL(mbar_gram_finish_kernel, dim3(pairs, kGramTileSize / kMbarBlock), dim3(kMbarBlock), 0, st, h->K, n_fb,
                     h->d_gram_partial.get(), gram);
  if (colsum)
    if (int rc = mbar_segment_launch(h, f, 1, nullptr, nullptr, nullptr, colsum, st)) return rc;
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_mbar_segment_moments(mythos_mbar_t* h, const double* f, int n_seg, const int64_t* seg_start, const int64_t* order,
                                const double* v, double* out, mythos_stream_t stream) {
  if (!h || !f || !out || n_seg < 1 || n_seg > (1 << 20) || (order && !seg_start) || (!order && n_seg != 1)) {
    set_error("mythos_mbar_segment_moments: invalid argument (1 <= n_seg <= 2^20; seg_start with an order, one segment without)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_ready(h, "mythos_mbar_segment_moments")) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  mbar_launch(h, f, nullptr, nullptr, st);  // L_n at this f
  if (int rc = mbar_segment_launch(h, f, n_seg, seg_start, order, v, out, st)) return rc;
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

// What both bootstrap entry points check and queue first: L^ at f^ and e^{delta}.
static int mbar_boot_begin(mythos_mbar* h, const char* who, const double* f_hat, int B, const double* delta, const uint16_t* mult,
                           const void* out, hipStream_t st) {
  if (!h || !f_hat || !delta || !mult || !out || B < 1 || B > kBootMaxB) {
    set_error(std::string(who) + ": invalid argument (1 <= B <= " + std::to_string(kBootMaxB) + " replicates)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mbar_ready(h, who)) return rc;
  if (mbar_boot_lds_doubles(h->K, h->P, h->src) > (size_t)kMbarLdsDoubles) {
    set_error(std::string(who) + ": the window table, " + std::to_string(kBootTile) + " rows of e^delta and a strip of " +
              std::to_string(kBootFrames) + " frames (" + std::to_string(mbar_boot_lds_doubles(h->K, h->P, h->src)) +
              " doubles) do not fit 64 KB of LDS");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(h->device));
  const long long count = (long long)B * h->K;
  if (int rc = h->d_boot_exp.grow((size_t)count)) return rc;
  mbar_launch(h, f_hat, nullptr, nullptr, st);  // L_n at f^
  hipLaunchKernelGGL(mbar_boot_exp_kernel, dim3((unsigned)((count + kMbarBlock - 1) / kMbarBlock)), dim3(kMbarBlock), 0, st, count, delta,
                     h->d_boot_exp.get());
  return MYTHOS_OK;
}

int mythos_mbar_boot_colsums(mythos_mbar_t* h, const double* f_hat, int n_boot, const double* delta, const uint16_t* mult, double* out_s,
                             mythos_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mbar_boot_begin(h, "mythos_mbar_boot_colsums", f_hat, n_boot, delta, mult, out_s, st)) return rc;
  const int tiles = ((n_boot + kBootTile - 1) / kBootTile) * ((h->K + kBootCols - 1) / kBootCols);
  const int splits = std::min(h->n_chunks, std::max(1, kSegMaxSplits / tiles));
  const long long count = (long long)n_boot * h->K;
  if (int rc = h->d_boot_partial.grow((size_t)splits * count)) return rc;
  auto kernel = h->src == 0 ? mbar_boot_kernel<0, 0> : mbar_boot_kernel<1, 0>;
  hipLaunchKernelGGL(kernel, dim3(1, splits, tiles), dim3(kMbarBlock), sizeof(double) * mbar_boot_lds_doubles(h->K, h->P, h->src), st, h->K,
                     h->P, (long long)h->N, n_boot, 0, (const long long*)nullptr, (const long long*)nullptr, (const double*)nullptr, 0.0,
                     h->xi, h->d_table.get(), h->u, h->d_ln_nk.get(), f_hat, h->d_L.get(), h->d_boot_exp.get(), mult,
                     h->d_boot_partial.get());
  hipLaunchKernelGGL(mbar_boot_colsums_finish_kernel, dim3((unsigned)((count + kMbarBlock - 1) / kMbarBlock)), dim3(kMbarBlock), 0, st, count,
                     h->K, splits, h->d_boot_partial.get(), delta, h->d_ln_nk.get(), out_s);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_mbar_boot_binned(mythos_mbar_t* h, const double* f_hat, int n_boot, const double* delta, const uint16_t* mult, int n_seg,
                            const int64_t* seg_start, const int64_t* order, int n_cols, const double* v, double shift, double* out,
                            mythos_stream_t stream) {
  if (n_seg < 1 || n_seg > (1 << 20) || (order && !seg_start) || (!order && n_seg != 1) || n_cols < 0 || n_cols > kBootMaxE ||
      (n_cols > 0 && !v) || !std::isfinite(shift)) {
    set_error("mythos_mbar_boot_binned: invalid argument (1 <= n_seg <= 2^20; seg_start with an order, one segment without; 0 <= E <= " +
              std::to_string(kBootMaxE) + " with v where E > 0; a finite shift)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mbar_boot_begin(h, "mythos_mbar_boot_binned", f_hat, n_boot, delta, mult, out, st)) return rc;
  const int E = std::max(n_cols, 1), tiles = (n_boot + kBootTile - 1) / kBootTile;
  const int splits = (int)std::min<long long>(h->n_chunks, std::max<long long>(1, kSegMaxSplits / ((long long)n_seg * tiles)));
  const long long count = (long long)n_boot * n_seg * E;
  if (int rc = h->d_boot_partial.grow((size_t)count * splits)) return rc;
  auto kernel = h->src == 0 ? mbar_boot_kernel<0, 1> : mbar_boot_kernel<1, 1>;
  hipLaunchKernelGGL(kernel, dim3(n_seg, splits, tiles), dim3(kMbarBlock), sizeof(double) * mbar_boot_lds_doubles(h->K, h->P, h->src), st,
                     h->K, h->P, (long long)h->N, n_boot, E, (const long long*)seg_start, (const long long*)order, n_cols > 0 ? v : nullptr,
                     shift, h->xi, h->d_table.get(), h->u, h->d_ln_nk.get(), f_hat, h->d_L.get(), h->d_boot_exp.get(), mult,
                     h->d_boot_partial.get());
  hipLaunchKernelGGL(mbar_boot_binned_finish_kernel, dim3((unsigned)((count + kMbarBlock - 1) / kMbarBlock)), dim3(kMbarBlock), 0, st, count,
                     E, splits, h->d_boot_partial.get(), out);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

}  // extern "C"
