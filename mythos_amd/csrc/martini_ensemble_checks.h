// Host bookkeeping of the MARTINI temperature ensemble that needs no device: what mythos_martini_langevin_create_ensemble and
// load refuse.  (How an advance with events is cut into chunks: mm_event_chunk, martini_exchange_checks.h.)  In the style
// of host_checks.h - it stands on the standard library and set_error alone, so tests/host/martini_ensemble_checks_main.cpp
// compiles it as it is, under the host sanitizers.
#ifndef MYTHOS_MARTINI_ENSEMBLE_CHECKS_H
#define MYTHOS_MARTINI_ENSEMBLE_CHECKS_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace mythos {

void set_error(const std::string& msg);

constexpr int kMmStride0 = 256;  // the row stride a new MARTINI integrator starts from

// 0, or -1 (MYTHOS_ERR_INVALID_ARGUMENT) with "<who>: ..." as the error message: three positive edges, none shorter than 2 rl
inline int mm_box_fits(const double* box, double rl, const std::string& who) {
  if (!box || !(box[0] > 0) || !(box[1] > 0) || !(box[2] > 0)) {
    set_error(who + ": invalid argument");
    return -1;
  }
  if (2.0 * rl > std::min(box[0], std::min(box[1], box[2]))) {
    set_error(who + ": the box is smaller than twice (r_cut + skin): minimum image breaks down");
    return -1;
  }
  return 0;
}

// n beads per replica, kT[n_rep], boxes [n_rep][3] or null (not checked then): 0 or -1 as above, the message naming the replica
inline int mm_ensemble_check(int n, int n_rep, const double* kT, double r_cut, double skin, const double* boxes, const char* who) {
  if (n < 1 || n_rep < 1 || !kT) {
    set_error(std::string(who) + ": at least one replica (n_rep >= 1) of at least one bead, and one kT per replica required");
    return -1;
  }
  for (int r = 0; r < n_rep; ++r)
    if (!(kT[r] > 0) || !std::isfinite(kT[r])) {
      set_error(std::string(who) + ": kT of replica " + std::to_string(r) + " must be finite and positive");
      return -1;
    }
  if ((long long)n_rep * n > (long long)(INT_MAX / kMmStride0)) {
    set_error(std::string(who) + ": " + std::to_string(n_rep) + " replicas of " + std::to_string(n) + " beads are more than the " +
              std::to_string(INT_MAX / kMmStride0) + " rows the neighbour store indexes");
    return -1;
  }
  for (int r = 0; boxes && r < n_rep; ++r)
    if (int rc = mm_box_fits(boxes + 3 * (size_t)r, r_cut + skin, std::string(who) + ": replica " + std::to_string(r))) return rc;
  return 0;
}

}  // namespace mythos

#endif  // MYTHOS_MARTINI_ENSEMBLE_CHECKS_H
