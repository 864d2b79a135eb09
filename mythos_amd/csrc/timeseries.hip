// Normalised autocorrelation functions of K time series, the input of the statistical inefficiency g (DESIGN section 3.5o;
// the definition is pymbar's, Chodera et al., J. Chem. Theory Comput. 3, 26, 2007).  Series k is the rows offsets[k] ...
// offsets[k + 1] - 1 of an (N, E) double array, each of the E columns a series of its own, T = its length:
//
//     mu = mean x,  v = mean (x - mu)^2,  C(t) = sum_{i < T - t} (x_i - mu)(x_{i+t} - mu) / ((T - t) v)
//
// ts_moments_kernel: one workgroup of 256 per (series, column): mu, then v, each thread-strided and block_sum.
// ts_autocorr_kernel: a workgroup of 256 takes one (series, column) and a tile of 64 lags t and walks the series in tiles
// of 256 positions i.  Per tile it stages the centred x_i (256 doubles) and the centred window x_{i + t} of the tile's lags
// (256 + 64 doubles, zeros past the end of the series) in LDS; thread (lag l, quarter q) adds its 64 products of the tile
// by fma in index order - x_i is an LDS broadcast, the window is read at consecutive addresses - into one register over
// all tiles, and at the end the four quarters of a lag are added in order.  A zero past the end adds nothing (fma(a, 0, s) =
// s).  No atomics, a fixed order: the same bits run after run.  A lag t >= T, and every lag of a constant series, is 0.
#include <algorithm>
#include <vector>

#include "device_buf.h"
#include "timeseries_checks.h"
#include "wave_ops.h"

namespace mythos {

constexpr int kTsBlock = 256;   // threads, and positions per tile
constexpr int kTsLags = 64;     // lags per workgroup

__global__ __launch_bounds__(kTsBlock) void ts_moments_kernel(int E, const double* __restrict__ x, const long long* __restrict__ offsets,
                                                               double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double s_red[kTsBlock / 64];
  const int series = (int)blockIdx.x / E, e = (int)blockIdx.x % E;
  const long long lo = offsets[series], T = offsets[series + 1] - lo;
  double acc = 0.0;
  for (long long i = threadIdx.x; i < T; i += kTsBlock) acc += x[(size_t)(lo + i) * E + e];
  const double mu = block_sum(acc, s_red) / (double)T;
  acc = 0.0;
  for (long long i = threadIdx.x; i < T; i += kTsBlock) {
    const double d = x[(size_t)(lo + i) * E + e] - mu;
    acc = fma(d, d, acc);
  }
  const double v = block_sum(acc, s_red) / (double)T;
  if (threadIdx.x == 0) mean[blockIdx.x] = mu, var[blockIdx.x] = v;
}

// grid (K E, lag tiles); out [K E][n_lags], out[.][j] = C(t0 + j)
__global__ __launch_bounds__(kTsBlock) void ts_autocorr_kernel(int E, const double* __restrict__ x, const long long* __restrict__ offsets,
                                                                const double* __restrict__ mean, const double* __restrict__ var,
                                                                long long t0, int n_lags, double* __restrict__ out) {
  __shared__ double s_a[kTsBlock];            // x_i - mu of the tile; the quarters' sums at the end
  __shared__ double s_b[kTsBlock + kTsLags];  // x_{i0 + tl0 + j} - mu
  const int tid = (int)threadIdx.x, l = tid & (kTsLags - 1), q = tid / kTsLags;
  const int series = (int)blockIdx.x / E, e = (int)blockIdx.x % E;
  const long long lo = offsets[series], T = offsets[series + 1] - lo;
  const long long tl0 = t0 + (long long)blockIdx.y * kTsLags;  // the tile's first lag
  const double mu = mean[blockIdx.x], v = var[blockIdx.x];
  const double* __restrict__ col = x + (size_t)lo * E + e;
  double acc = 0.0;
  for (long long i0 = 0; i0 + tl0 < T; i0 += kTsBlock) {  // (uniform over the workgroup)
    const long long i = i0 + tid;
    s_a[tid] = i < T ? col[(size_t)i * E] - mu : 0.0;
    for (int j = tid; j < kTsBlock + kTsLags; j += kTsBlock) {
      const long long p = i0 + tl0 + j;
      s_b[j] = p < T ? col[(size_t)p * E] - mu : 0.0;
    }
    __syncthreads();
    const double* __restrict__ a = s_a + q * kTsLags;
    const double* __restrict__ b = s_b + q * kTsLags + l;
#pragma unroll 8
    for (int k = 0; k < kTsLags; ++k) acc = fma(a[k], b[k], acc);
    __syncthreads();
  }
  s_a[tid] = acc;
  __syncthreads();
  const int j = (int)blockIdx.y * kTsLags + l;
  if (q == 0 && j < n_lags) {
    const double total = ((s_a[l] + s_a[kTsLags + l]) + s_a[2 * kTsLags + l]) + s_a[3 * kTsLags + l];
    const long long t = tl0 + l;
    out[(size_t)blockIdx.x * n_lags + j] = (t < T && v > 0.0) ? total / ((double)(T - t) * v) : 0.0;
  }
}

static int ts_args(const char* who, int64_t N, int E, int K, const int64_t* offsets, const void* a, const void* b, const void* c,
                   const void* d) {
  if (!a || !b || !c || !d) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = timeseries_check(who, N, E, K, offsets, nullptr)) return rc;
  if ((int64_t)K * E > (int64_t)0x7fffffff) {
    set_error(std::string(who) + ": K E >= 2^31 series");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  return MYTHOS_OK;
}

}  // namespace mythos

using namespace mythos;

extern "C" {

int mythos_timeseries_check(int64_t n_rows, int n_cols, int n_series, const int64_t* offsets, const double* x) {
  return timeseries_check("mythos_timeseries_check", n_rows, n_cols, n_series, offsets, x);
}

int mythos_timeseries_moments(const double* x, int64_t n_rows, int n_cols, int n_series, const int64_t* offsets,
                              const int64_t* offsets_dev, double* mean, double* var, int device, mythos_stream_t stream) {
  if (int rc = ts_args("mythos_timeseries_moments", n_rows, n_cols, n_series, offsets, x, offsets_dev, mean, var)) return rc;
  if (int rc = select_device(device, "mythos_timeseries_moments")) return rc;
  hipLaunchKernelGGL(ts_moments_kernel, dim3(n_series * n_cols), dim3(kTsBlock), 0, (hipStream_t)stream, n_cols, x,
                     (const long long*)offsets_dev, mean, var);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

int mythos_timeseries_autocorr(const double* x, int64_t n_rows, int n_cols, int n_series, const int64_t* offsets,
                               const int64_t* offsets_dev, const double* mean, const double* var, int64_t t0, int n_lags,
                               double* out, int device, mythos_stream_t stream) {
  if (int rc = ts_args("mythos_timeseries_autocorr", n_rows, n_cols, n_series, offsets, x, offsets_dev, mean, var)) return rc;
  if (!out || t0 < 0 || n_lags < 1 || n_lags > kTsMaxLagBlock) {
    set_error("mythos_timeseries_autocorr: invalid argument (t0 >= 0, 1 <= n_lags <= " + std::to_string(kTsMaxLagBlock) + ")");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = select_device(device, "mythos_timeseries_autocorr")) return rc;
  hipLaunchKernelGGL(ts_autocorr_kernel, dim3(n_series * n_cols, (n_lags + kTsLags - 1) / kTsLags), dim3(kTsBlock), 0,
                     (hipStream_t)stream, n_cols, x, (const long long*)offsets_dev, mean, var, (long long)t0, n_lags, out);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

}  // extern "C"
