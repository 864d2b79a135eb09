// Host-side checks of a stress-profile call (mythos_martini_stress_profile, mythos_martini_stress_profile_check): every
// refusal named.  In the style of mbar_checks.h - the standard library, the public header and set_error alone, in front of
// any device call, so a bad call is refused without a GPU.  Definitions: DESIGN section 3.5q.
#ifndef MYTHOS_STRESS_PROFILE_CHECKS_H
#define MYTHOS_STRESS_PROFILE_CHECKS_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);

// Slabs per frame.  The slab kernel keeps nothing per slab in LDS (a wavefront owns a slab and sums it in bead order), so the
// cap is not a capacity of the kernel: it is the count at which the raw row of a frame - 13 doubles per slab with by_term -
// is 104 KB, and beyond which a slab of a 20 000-bead frame holds a handful of beads.
constexpr int kStressMaxBins = 1024;
constexpr int kStressTerms = 4;  // lj, bond, angle, coulomb: the order of the by_term columns
constexpr int stress_row_width(bool by_term) { return by_term ? MYTHOS_STRESS_ROW_BY_TERM : MYTHOS_STRESS_ROW; }

// MYTHOS_OK, or INVALID_ARGUMENT with "<who>: <why>" as the message.  boxes: HOST double[n_frames][3], or NULL where the
// caller has the boxes on the device only (nothing about them is checked then); center may be NULL where n_center is 0.
inline int stress_profile_check(const char* who, int n, double r_cut, int n_frames, const double* boxes, int n_center,
                                const int32_t* center, int n_bins) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (n < 1 || n_frames < 0 || n_center < 0 || (n_center > 0 && !center) || !(r_cut > 0.0)) return refuse("invalid argument");
  if (n_bins < 1) return refuse("n_bins < 1 (at least one slab)");
  if (n_bins > kStressMaxBins) return refuse("n_bins = " + std::to_string(n_bins) + " is above the cap of " + std::to_string(kStressMaxBins) + " slabs");
  for (int k = 0; k < n_center; ++k)
    if (center[k] < 0 || center[k] >= n)
      return refuse("centre index " + std::to_string(center[k]) + " (entry " + std::to_string(k) + ") is outside [0, " + std::to_string(n) + ")");
  if (boxes)
    for (int f = 0; f < n_frames; ++f)
      for (int d = 0; d < 3; ++d) {
        const double l = boxes[3 * (size_t)f + d];
        if (!std::isfinite(l) || !(l > 0.0))
          return refuse("frame " + std::to_string(f) + ": box edge " + std::to_string(d) + " is not positive and finite");
        if (l < 2.0 * r_cut)
          return refuse("frame " + std::to_string(f) + ": box edge " + std::to_string(d) + " = " + std::to_string(l) + " is shorter than 2 r_cut = " +
                        std::to_string(2.0 * r_cut) + "; the minimum image does not find the closest pair there");
      }
  return MYTHOS_OK;
}

}  // namespace mythos

#endif  // MYTHOS_STRESS_PROFILE_CHECKS_H
