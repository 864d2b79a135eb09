// Host-side checks of a set of point forces (mythos_langevin_set_point_forces, mythos_point_forces_check): every term
// named by its place in the list and its kind.  In the style of host_checks.h - it stands on the standard library, the
// public header's enum and set_error alone and runs in front of any device call, so a bad term is refused without a GPU.
// The rows of `param` are those of the table at enum mythos_point_force_kind (include/mythos_hip.h).
#ifndef MYTHOS_POINT_FORCE_CHECKS_H
#define MYTHOS_POINT_FORCE_CHECKS_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);

constexpr int kPointForceParams = 8;  // doubles per term

// where the three components of a kind's direction are in its row (-1: it has none).  A string and a plane need one
// always, a trap only when it moves (rate != 0).
inline int point_force_dir_at(int kind) {
  return (kind == MYTHOS_POINT_STRING || kind == MYTHOS_POINT_TRAP || kind == MYTHOS_POINT_PLANE) ? 2 : -1;
}

// where a kind's rate is in its row (-1: the kind cannot move): word 1 of a string and a trap, word 2 of a mutual trap and
// a sphere.  A kind this does not know is an error of whoever added it, not a resting term.
inline int point_force_rate_at(int kind) {
  static_assert(MYTHOS_POINT_KINDS == 5, "a new point-force kind: say where its rate is");
  switch (kind) {
    case MYTHOS_POINT_STRING:
    case MYTHOS_POINT_TRAP: return 1;
    case MYTHOS_POINT_MUTUAL_TRAP:
    case MYTHOS_POINT_SPHERE: return 2;
    default: return -1;  // (a plane)
  }
}

// true: every term is one the kernel evaluates.  false, with "<who>: term <t> (<kind>): ..." as the error message.
// n: nucleotides of the system; has_box: whether a minimum image exists.  n_terms = 0 reads nothing.
inline bool point_forces_valid(const char* who, int n, bool has_box, int n_terms, const int32_t* kind, const int32_t* particle,
                               const int32_t* ref_particle, const int32_t* flags, const double* param) {
  static const char* const names[] = {"string", "trap", "mutual_trap", "repulsion_plane", "repulsion_sphere"};
  for (int t = 0; t < n_terms; ++t) {
    const int k = kind[t];
    const std::string where = std::string(who) + ": term " + std::to_string(t);
    auto refuse = [&](const std::string& why) {
      set_error(where + (k >= 0 && k < MYTHOS_POINT_KINDS ? " (" + std::string(names[k]) + ")" : std::string()) + ": " + why);
      return false;
    };
    if (k < 0 || k >= MYTHOS_POINT_KINDS) return refuse("kind " + std::to_string(k) + " is not a mythos_point_force_kind");
    const std::string range = " out of range [0, " + std::to_string(n) + ")";
    if (particle[t] < 0 || particle[t] >= n) return refuse("particle " + std::to_string(particle[t]) + range);
    const double* q = param + (size_t)t * kPointForceParams;
    for (int a = 0; a < kPointForceParams; ++a)
      if (!std::isfinite(q[a])) return refuse("parameter " + std::to_string(a) + " is not finite");
    if (flags[t] != 0 && !(k == MYTHOS_POINT_MUTUAL_TRAP && flags[t] == MYTHOS_POINT_PBC))
      return refuse("flags = " + std::to_string(flags[t]) + " (only a mutual trap takes MYTHOS_POINT_PBC)");
    if (k != MYTHOS_POINT_STRING && q[0] < 0) return refuse("stiff is negative (stiff >= 0)");
    if (k == MYTHOS_POINT_MUTUAL_TRAP) {
      if (ref_particle[t] < 0 || ref_particle[t] >= n) return refuse("ref_particle " + std::to_string(ref_particle[t]) + range);
      if (ref_particle[t] == particle[t]) return refuse("ref_particle is the particle itself (" + std::to_string(particle[t]) + ")");
      if (flags[t] == MYTHOS_POINT_PBC && !has_box) return refuse("PBC = 1 on a system without a box");
    }
    if ((k == MYTHOS_POINT_MUTUAL_TRAP || k == MYTHOS_POINT_SPHERE) && q[1] < 0) return refuse("r0 is negative (r0 >= 0)");
    const int d = point_force_dir_at(k);
    if (d >= 0 && !(q[d] * q[d] + q[d + 1] * q[d + 1] + q[d + 2] * q[d + 2] > 0) && !(k == MYTHOS_POINT_TRAP && q[1] == 0.0))
      return refuse("dir is zero (a direction is needed)");
  }
  return true;
}

}  // namespace mythos

#endif  // MYTHOS_POINT_FORCE_CHECKS_H
