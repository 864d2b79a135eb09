// Host-side checks of an MBAR problem (mythos_mbar_check, mythos_mbar_set_windows, mythos_mbar_set_matrix,
// mythos_mbar_binned_sum): every refusal named.  In the style of martini_restraint_checks.h - the standard library, the
// public header and set_error alone, in front of any device call, so a bad problem is refused without a GPU.
// Definitions: DESIGN section 3.5o.  The window table is host double[K][P][kMbarRow] = {kind, k, init, rate} with kind 0
// for an umbrella U = 1/2 k (xi - init)^2 and 1 for a constant force U = k xi, as MartiniRestraints.lower delivers the
// pull coordinates of replica k.
#ifndef MYTHOS_MBAR_CHECKS_H
#define MYTHOS_MBAR_CHECKS_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);

constexpr int kMbarRow = 4;             // doubles per (window, coordinate) of the table: kind, k, init, rate
constexpr int kMbarLdsDoubles = 8192;   // 64 KB of LDS: K (3 P + 6) doubles of the iterate kernel fit below it
enum : int { MBAR_UMBRELLA = 0, MBAR_CONSTANT_FORCE = 1 };

// doubles of LDS the iterate kernel takes: the lowered table (3 per window and coordinate), ln N_k, f_k and one sum per
// wavefront and window
constexpr size_t mbar_lds_doubles(int K, int P) { return (size_t)K * (3 * (size_t)P + 2 + 4); }

// MYTHOS_OK, or INVALID_ARGUMENT with "<who>: <why>" as the message.  Every array may be NULL where its count is 0 or the
// caller has nothing to check there: table and kT (the matrix path has neither), xi (frames that stay on the device), edges.
inline int mbar_check(const char* who, int K, int64_t N, int P, const double* table, const double* kT, const int64_t* n_k,
                      const double* xi, int n_edges, const double* edges) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (K < 1) return refuse("K < 1 (at least one window)");
  if (N < 1 || P < 0 || n_edges < 0 || !n_k) return refuse("invalid argument");
  if (N >= ((int64_t)1 << 31)) return refuse("N >= 2^31 frames");
  if (mbar_lds_doubles(K, P) > (size_t)kMbarLdsDoubles)
    return refuse("K (3 P + 6) = " + std::to_string(mbar_lds_doubles(K, P)) + " doubles of window table do not fit 64 KB of LDS");
  int64_t sum = 0;
  for (int k = 0; k < K; ++k) {
    if (n_k[k] < 1) return refuse("N_k < 1 for window " + std::to_string(k) + " (states without frames are not built)");
    sum += n_k[k];
    if (sum > N) break;
  }
  if (sum != N) return refuse("sum N_k != N (the windows' frame counts do not add up to the " + std::to_string(N) + " frames)");
  if (table) {
    if (P < 1) return refuse("the window table needs at least one coordinate");
    for (int k = 0; k < K; ++k)
      for (int p = 0; p < P; ++p) {
        const double* q = table + ((size_t)k * P + p) * kMbarRow;
        const std::string w = "window " + std::to_string(k) + ", coordinate " + std::to_string(p) + ": ";
        if (q[0] != MBAR_UMBRELLA && q[0] != MBAR_CONSTANT_FORCE) return refuse(w + "unknown kind");
        if (!std::isfinite(q[1])) return refuse(w + "non-finite k");
        if (!std::isfinite(q[2])) return refuse(w + "non-finite init");
        if (!(q[3] == 0.0)) return refuse(w + "rate != 0 (moving windows are not built)");
      }
    if (!kT) return refuse("the window table needs kT");
  }
  if (kT)
    for (int k = 0; k < K; ++k) {
      if (!std::isfinite(kT[k]) || !(kT[k] > 0.0)) return refuse("kT of window " + std::to_string(k) + " is not positive and finite");
      if (kT[k] != kT[0])
        return refuse("windows at different kT (" + std::to_string(k) + " and 0): the table path takes one temperature, "
                      "a temperature ladder needs the matrix path");
    }
  if (xi)
    for (int64_t i = 0; i < N * P; ++i)
      if (!std::isfinite(xi[i])) return refuse("non-finite xi (frame " + std::to_string(i / P) + ", coordinate " + std::to_string(i % P) + ")");
  if (n_edges > 0) {
    if (!edges || n_edges < 2) return refuse("edges: at least two are needed");
    for (int b = 0; b < n_edges; ++b) {
      if (!std::isfinite(edges[b])) return refuse("non-finite edge " + std::to_string(b));
      if (b > 0 && !(edges[b] > edges[b - 1])) return refuse("non-increasing edges (edge " + std::to_string(b) + ")");
    }
  }
  return MYTHOS_OK;
}

}  // namespace mythos

#endif  // MYTHOS_MBAR_CHECKS_H
