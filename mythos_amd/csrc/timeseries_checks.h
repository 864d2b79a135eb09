// Host-side checks of a set of time series (mythos_timeseries_check, mythos_timeseries_moments,
// mythos_timeseries_autocorr): every refusal named.  In the style of mbar_checks.h - the standard library, the public
// header and set_error alone, in front of any device call, so a bad set is refused without a GPU.
// Definitions: DESIGN section 3.5o.  K series are segments of an (N, E) array: series k holds the rows
// offsets[k] ... offsets[k + 1] - 1, time-ordered; each of the E columns is a series of its own.
#ifndef MYTHOS_TIMESERIES_CHECKS_H
#define MYTHOS_TIMESERIES_CHECKS_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);

constexpr int kTsMaxLagBlock = 1 << 16;  // lags per call of mythos_timeseries_autocorr

// MYTHOS_OK, or INVALID_ARGUMENT with "<who>: <why>" as the message.  x (host double[N][E]) may be NULL: values that stay
// on the device are the caller's to check.
inline int timeseries_check(const char* who, int64_t N, int E, int K, const int64_t* offsets, const double* x) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (E < 1) return refuse("E < 1 (at least one column)");
  if (K < 1 || N < 1 || !offsets) return refuse("invalid argument (K >= 1 series, N >= 1 rows, offsets)");
  if (N >= ((int64_t)1 << 31)) return refuse("N >= 2^31 rows");
  if (offsets[0] != 0) return refuse("offsets do not increase to N (offsets[0] != 0)");
  for (int k = 0; k < K; ++k)
    if (!(offsets[k + 1] > offsets[k]) || offsets[k + 1] > N)
      return refuse("offsets do not increase to N (series " + std::to_string(k) + " is empty or runs past the " + std::to_string(N) + " rows)");
  if (offsets[K] != N) return refuse("offsets do not increase to N (offsets[K] = " + std::to_string(offsets[K]) + ", N = " + std::to_string(N) + ")");
  if (x)
    for (int64_t i = 0; i < N * E; ++i)
      if (!std::isfinite(x[i])) return refuse("non-finite value (row " + std::to_string(i / E) + ", column " + std::to_string(i % E) + ")");
  return MYTHOS_OK;
}

}  // namespace mythos

#endif  // MYTHOS_TIMESERIES_CHECKS_H
