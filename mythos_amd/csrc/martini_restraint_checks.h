// Host-side checks and lowering of a set of MARTINI restraints (mythos_martini_langevin_set_restraints,
// mythos_martini_restraints_check): every term named by its kind and its place in the list.  In the style of
// point_force_checks.h - the standard library, the public header and set_error alone, in front of any device call, so a bad
// set is refused without a GPU.  The layouts are those of the prototype in include/mythos_hip.h.
#ifndef MYTHOS_MARTINI_RESTRAINT_CHECKS_H
#define MYTHOS_MARTINI_RESTRAINT_CHECKS_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);

constexpr int kMrFlatParams = 5;  // doubles per flat-bottom term and replica: k, r, X.xyz
constexpr int kMrPullParams = 9;  // doubles per pull coordinate and replica: k, init, rate, vec.xyz, origin.xyz
// flat-bottom flags: shape in bits 0-1, axis in bits 2-3, invert in bit 4
enum : int { MR_FLAT_SPHERE = 0, MR_FLAT_CYLINDER = 1, MR_FLAT_LAYER = 2 };
constexpr int mr_flat_shape(int f) { return f & 3; }
constexpr int mr_flat_axis(int f) { return (f >> 2) & 3; }
constexpr bool mr_flat_invert(int f) { return ((f >> 4) & 1) != 0; }
// pull flags: bit 0 constant-force (else umbrella), bit 1 direction (else distance), bit 2 periodic, bits 4-6 dim
constexpr bool mr_pull_constant(int f) { return (f & 1) != 0; }
constexpr bool mr_pull_direction(int f) { return (f & 2) != 0; }
constexpr bool mr_pull_periodic(int f) { return (f & 4) != 0; }
constexpr int mr_pull_dim(int f) { return (f >> 4) & 7; }
// term codes of a restrained bead's list: kind in bits 0-1, (pull) side in bit 2 - 0: member of A, 1: member of B -, index above
enum : int { MR_TERM_POSRES = 0, MR_TERM_FLAT = 1, MR_TERM_PULL = 2 };
constexpr int mr_term_code(int kind, int side, int index) { return (index << 3) | (side << 2) | kind; }

// the flat arrays of one set, as the entry points take them
struct MrArrays {
  int n_posres = 0;
  const int32_t* pr_index = nullptr;  // [n_posres]
  const double* pr_k = nullptr;       // [n_posres][3]
  const double* pr_ref = nullptr;     // [n_rep][n_posres][3]
  int n_flat = 0;
  const int32_t* fb_index = nullptr;  // [n_flat]
  const int32_t* fb_flags = nullptr;  // [n_flat]
  const double* fb_param = nullptr;   // [n_rep][n_flat][kMrFlatParams]
  int n_groups = 0;
  const int32_t* g_first = nullptr;    // [n_groups + 1]
  const int32_t* g_member = nullptr;   // members, group after group
  const int32_t* g_pbc_ref = nullptr;  // [n_groups] a member, or -1
  int n_pull = 0;
  const int32_t* p_flags = nullptr;   // [n_pull]
  const int32_t* p_groups = nullptr;  // [n_pull][2]: A (-1: the absolute reference `origin`), B
  const double* p_param = nullptr;    // [n_rep][n_pull][kMrPullParams]
  const double* boxes = nullptr;      // [n_rep][3], or NULL when no term takes a minimum image
  bool empty() const { return n_posres == 0 && n_flat == 0 && n_pull == 0; }
};

// MYTHOS_OK, or INVALID_ARGUMENT with "<who>: <term>: <why>" as the error message.  n: beads of one replica.
inline int mr_check(const char* who, int n, int n_rep, const MrArrays& a, bool barostat, bool exchange) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (n < 1 || n_rep < 1 || a.n_posres < 0 || a.n_flat < 0 || a.n_groups < 0 || a.n_pull < 0) return refuse("invalid argument");
  if ((a.n_posres > 0 && (!a.pr_index || !a.pr_k || !a.pr_ref)) || (a.n_flat > 0 && (!a.fb_index || !a.fb_flags || !a.fb_param)) ||
      (a.n_groups > 0 && (!a.g_first || !a.g_member || !a.g_pbc_ref)) || (a.n_pull > 0 && (!a.p_flags || !a.p_groups || !a.p_param)))
    return refuse("invalid argument (a list without its arrays)");
  if (!a.empty() && barostat)
    return refuse("restraints together with a barostat are refused: the restraint virial and reference scaling are not built");
  if (!a.empty() && exchange)
    return refuse("restraints together with replica exchange are refused: the restraint energy is not in the exchange's H");
  const std::string range = " out of range [0, " + std::to_string(n) + ")";
  bool need_box = false;
  std::vector<char> seen((size_t)n, 0);
  for (int t = 0; t < a.n_posres; ++t) {
    const std::string w = "position restraint " + std::to_string(t) + ": ";
    const int i = a.pr_index[t];
    if (i < 0 || i >= n) return refuse(w + "index " + std::to_string(i) + range);
    if (seen[i]) return refuse(w + "duplicate position restraint of bead " + std::to_string(i));
    seen[i] = 1;
    for (int d = 0; d < 3; ++d) {
      const double k = a.pr_k[3 * (size_t)t + d];
      if (!std::isfinite(k)) return refuse(w + "non-finite value (k)");
      if (k < 0) return refuse(w + "k < 0");
    }
    for (int r = 0; r < n_rep; ++r)
      for (int d = 0; d < 3; ++d)
        if (!std::isfinite(a.pr_ref[((size_t)r * a.n_posres + t) * 3 + d])) return refuse(w + "non-finite value (reference)");
  }
  for (int t = 0; t < a.n_flat; ++t) {
    const std::string w = "flat-bottom restraint " + std::to_string(t) + ": ";
    const int i = a.fb_index[t], f = a.fb_flags[t];
    if (i < 0 || i >= n) return refuse(w + "index " + std::to_string(i) + range);
    if (f < 0 || f >= 32 || mr_flat_shape(f) > MR_FLAT_LAYER || mr_flat_axis(f) > 2) return refuse(w + "unknown shape or axis (flags " + std::to_string(f) + ")");
    for (int r = 0; r < n_rep; ++r) {
      const double* q = a.fb_param + ((size_t)r * a.n_flat + t) * kMrFlatParams;
      for (int d = 0; d < kMrFlatParams; ++d)
        if (!std::isfinite(q[d])) return refuse(w + "non-finite value");
      if (q[0] < 0) return refuse(w + "k < 0");
      if (q[1] < 0) return refuse(w + "r < 0");
    }
  }
  for (int g = 0; g < a.n_groups; ++g) {
    const std::string w = "pull group " + std::to_string(g) + ": ";
    const int b = a.g_first[g], e = a.g_first[g + 1];
    if (b < 0 || e < b || (g == 0 && b != 0)) return refuse(w + "invalid member range");
    if (e == b) return refuse(w + "empty group");
    std::fill(seen.begin(), seen.end(), 0);
    for (int m = b; m < e; ++m) {
      const int i = a.g_member[m];
      if (i < 0 || i >= n) return refuse(w + "index " + std::to_string(i) + range);
      if (seen[i]) return refuse(w + "duplicate member " + std::to_string(i));
      seen[i] = 1;
    }
    const int pr = a.g_pbc_ref[g];
    if (pr >= 0) need_box = true;
    if (pr != -1 && (pr < 0 || pr >= n || !seen[pr])) return refuse(w + "pbc_ref " + std::to_string(pr) + " is not a member of the group");
  }
  for (int p = 0; p < a.n_pull; ++p) {
    const std::string w = "pull coordinate " + std::to_string(p) + ": ";
    const int f = a.p_flags[p], A = a.p_groups[2 * p], B = a.p_groups[2 * p + 1];
    if (f < 0 || f >= 128 || (f & 8)) return refuse(w + "unknown flags " + std::to_string(f));
    if (A < -1 || A >= a.n_groups || B < 0 || B >= a.n_groups)
      return refuse(w + "group index out of range [0, " + std::to_string(a.n_groups) + ")");
    if (A == B) return refuse(w + "A = B (the two groups are the same)");
    if (mr_pull_periodic(f)) need_box = true;
    if (!mr_pull_direction(f) && mr_pull_dim(f) == 0) return refuse(w + "empty dim (a distance needs at least one axis)");
    for (int r = 0; r < n_rep; ++r) {
      const double* q = a.p_param + ((size_t)r * a.n_pull + p) * kMrPullParams;
      for (int d = 0; d < kMrPullParams; ++d)
        if (!std::isfinite(q[d])) return refuse(w + "non-finite value");
      if (!mr_pull_constant(f) && q[0] < 0) return refuse(w + "k < 0");
      if (mr_pull_direction(f) && !(q[3] * q[3] + q[4] * q[4] + q[5] * q[5] > 0)) return refuse(w + "zero vec (a direction is needed)");
    }
  }
  if (a.boxes)
    for (int k = 0; k < 3 * n_rep; ++k)
      if (!std::isfinite(a.boxes[k]) || !(a.boxes[k] > 0)) return refuse("box of replica " + std::to_string(k / 3) + ": non-finite value or an edge <= 0");
  if (need_box && !a.boxes) return refuse("periodic coordinates and pbc_ref need the replicas' boxes");
  return MYTHOS_OK;
}

// The term lists of the restrained beads of one replica (the set passed mr_check): beads ascending; per bead its position
// restraint first, then its flat-bottom terms in the order given, then the pull coordinates ascending (within one, A's
// membership before B's).
struct MrEntries {
  std::vector<int32_t> index, first, term;
};
inline MrEntries mr_entries(int n, const MrArrays& a) {
  std::vector<std::vector<int32_t>> per((size_t)n);
  for (int t = 0; t < a.n_posres; ++t) per[a.pr_index[t]].push_back(mr_term_code(MR_TERM_POSRES, 0, t));
  for (int t = 0; t < a.n_flat; ++t) per[a.fb_index[t]].push_back(mr_term_code(MR_TERM_FLAT, 0, t));
  for (int p = 0; p < a.n_pull; ++p)
    for (int side = 0; side < 2; ++side) {
      const int g = a.p_groups[2 * p + side];
      if (g < 0) continue;
      for (int m = a.g_first[g]; m < a.g_first[g + 1]; ++m) per[a.g_member[m]].push_back(mr_term_code(MR_TERM_PULL, side, p));
    }
  MrEntries e;
  e.first.push_back(0);
  for (int i = 0; i < n; ++i) {
    if (per[i].empty()) continue;
    e.index.push_back(i);
    e.term.insert(e.term.end(), per[i].begin(), per[i].end());
    e.first.push_back((int32_t)e.term.size());
  }
  return e;
}

}  // namespace mythos

#endif  // MYTHOS_MARTINI_RESTRAINT_CHECKS_H
