// Host bookkeeping of window exchange in the MARTINI ensemble (mythos_martini_langevin_set_window_exchange): Hamiltonian
// replica exchange between the per-replica parameter rows of a set of restraints ("windows") at equal temperature.  What
// needs no device is here: the decision, the refusals, the permutation check of an assignment and the plan that carries
// the rows from one assignment to another.  In the style of martini_exchange_checks.h, whose pair schedule, acceptance
// rule and chunking it shares - the standard library and set_error alone, so tests/host/martini_window_exchange_main.cpp
// compiles it as it is under the host sanitizers.
#ifndef MYTHOS_MARTINI_WINDOW_EXCHANGE_CHECKS_H
#define MYTHOS_MARTINI_WINDOW_EXCHANGE_CHECKS_H

#include "martini_exchange_checks.h"

namespace mythos {

constexpr int kWxRec = 11;  // step, t, slot A, slot B, E_t(x_A), E_t+1(x_A), E_t(x_B), E_t+1(x_B), d, u, accepted
constexpr uint32_t kWxStream = 6;  // Philox stream (5: temperature exchange)
constexpr int kWxPullParams = 9;   // kMrPullParams of martini_restraint_checks.h: k, init, rate, vec.xyz, origin.xyz

// ---- the decision for slot A in window t and slot B in window t + 1, both at kT: the physical energy cancels, what is
// left are the restraint energies of the two configurations under the two windows
MYTHOS_XHD inline double mm_wx_delta(double kT, double e_t_a, double e_t1_a, double e_t_b, double e_t1_b) {
  return -(1.0 / kT) * ((e_t1_a + e_t_b) - (e_t_a + e_t1_b));
}

// ---- rows from one assignment to another: slot s takes the row that slot plan[s] holds now.  cur and want are
// permutations (window_of_slot); the window want[s] lies in the slot q with cur[q] == want[s].
inline std::vector<int32_t> mm_wx_row_plan(const int32_t* cur, const int32_t* want, int n_rep) {
  std::vector<int32_t> slot_of((size_t)n_rep, -1), plan((size_t)n_rep, -1);
  for (int q = 0; q < n_rep; ++q) slot_of[(size_t)cur[q]] = q;
  for (int s = 0; s < n_rep; ++s) plan[(size_t)s] = slot_of[(size_t)want[s]];
  return plan;
}
// rows [n_rep][row_len] gathered through a plan, in place
inline void mm_wx_permute_rows(std::vector<double>& rows, size_t row_len, const std::vector<int32_t>& plan) {
  if (row_len == 0) return;
  const std::vector<double> old(rows);
  for (size_t s = 0; s < plan.size(); ++s)
    std::copy(old.begin() + (size_t)plan[s] * row_len, old.begin() + ((size_t)plan[s] + 1) * row_len, rows.begin() + s * row_len);
}

// ---- refusals: 0, or -1 (MYTHOS_ERR_INVALID_ARGUMENT) with "<who>: ..." as the error message
inline int mm_wx_check_settings(int n_rep, int every, const char* who) {
  if (n_rep < 2) {
    set_error(std::string(who) + ": window exchange needs an ensemble handle with at least two replicas (n_rep >= 2)");
    return -1;
  }
  if (every < 0) {
    set_error(std::string(who) + ": window exchange every >= 0 required (0 switches window exchange off)");
    return -1;
  }
  return 0;
}
inline int mm_wx_check_kT(int n_rep, const double* kT, const char* who) {
  for (int r = 1; r < n_rep; ++r)
    if (kT[r] != kT[0]) {
      set_error(std::string(who) + ": window exchange needs every replica at the same kT (replica " + std::to_string(r) + " has " +
                std::to_string(kT[r]) + ", replica 0 " + std::to_string(kT[0]) +
                "): exchange with different kT and windows is not built");
      return -1;
    }
  return 0;
}
inline int mm_wx_check_partners(bool temperature_exchange, bool barostat, const char* who) {
  if (temperature_exchange) {
    set_error(std::string(who) + ": window exchange together with temperature replica exchange is refused: exchange with "
              "different kT and windows is not built");
    return -1;
  }
  if (barostat) {
    set_error(std::string(who) + ": window exchange together with a barostat is refused: restraints under pressure coupling "
              "are not built");
    return -1;
  }
  return 0;
}
// windows may differ in k, init, rate (and in the position-restraint references and flat-bottom parameters); vec and origin
// of a pull coordinate are the coordinate's: xi is then a function of the configuration alone
inline int mm_wx_check_set(int n_rep, int n_pull, const double* p_param, const char* who) {
  if (n_pull <= 0 || !p_param) return 0;
  for (int r = 1; r < n_rep; ++r)
    for (int p = 0; p < n_pull; ++p)
      for (int d = 3; d < kWxPullParams; ++d)
        if (p_param[((size_t)r * n_pull + p) * kWxPullParams + d] != p_param[(size_t)p * kWxPullParams + d]) {
          set_error(std::string(who) + ": pull coordinate " + std::to_string(p) + ": window exchange needs the same " +
                    (d < 6 ? "vec" : "origin") + " in every replica (replica " + std::to_string(r) +
                    " differs): windows may differ in k, init and rate only");
          return -1;
        }
  return 0;
}
inline int mm_wx_check_windows(int n_rep, const int32_t* window_of_slot, const char* who) {
  if (n_rep < 2) return mm_wx_check_settings(n_rep, 0, who);
  if (!mm_is_permutation(window_of_slot, n_rep)) {
    set_error(std::string(who) + ": window_of_slot must be a permutation of 0 .. " + std::to_string(n_rep - 1));
    return -1;
  }
  return 0;
}
// every refusal that needs no handle; kT, p_param and window_of_slot may be NULL (not checked)
inline int mm_wx_check(int n_rep, int every, const double* kT, bool temperature_exchange, bool barostat, int n_pull, const double* p_param,
                       const int32_t* window_of_slot, const char* who) {
  if (int rc = mm_wx_check_settings(n_rep, every, who)) return rc;
  if (kT)
    if (int rc = mm_wx_check_kT(n_rep, kT, who)) return rc;
  if (every > 0)
    if (int rc = mm_wx_check_partners(temperature_exchange, barostat, who)) return rc;
  if (n_pull < 0) {
    set_error(std::string(who) + ": invalid argument (n_pull < 0)");
    return -1;
  }
  if (every > 0)
    if (int rc = mm_wx_check_set(n_rep, n_pull, p_param, who)) return rc;
  return window_of_slot ? mm_wx_check_windows(n_rep, window_of_slot, who) : 0;
}

}  // namespace mythos

#endif  // MYTHOS_MARTINI_WINDOW_EXCHANGE_CHECKS_H
