// Stand-alone host program for mythos_amd/csrc/martini_window_exchange_checks.h, built with -fsanitize=address,undefined by
// tests/test_martini_window_exchange_cpu.py: the decision of window exchange, every refusal, the permutation check of an
// assignment, and the row plan of set_windows for R = 2 .. 5 over every pair of permutations.  Exit code 0 and "ok" on
// success.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "martini_window_exchange_checks.h"

namespace mythos {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mythos

using namespace mythos;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static bool has(const char* part) { return g_error.find(part) != std::string::npos; }

int main() {
  // ---- the decision: two harmonic windows at 0 and 1 (k = 2, kT = 1), x_A = 1 in window t, x_B = 0 in window t + 1:
  // E_t(x_A) = 1, E_t+1(x_A) = 0, E_t(x_B) = 0, E_t+1(x_B) = 1 -> d = +2, always swapped; the mirror image has d = -2
  CHECK(mm_wx_delta(1.0, 1.0, 0.0, 0.0, 1.0) == 2.0);
  CHECK(mm_wx_delta(1.0, 0.0, 1.0, 1.0, 0.0) == -2.0);
  CHECK(mm_wx_delta(2.5, 3.0, 3.0, 7.0, 7.0) == 0.0 && mm_xchg_accept(mm_wx_delta(2.5, 3.0, 3.0, 7.0, 7.0), 0.999999));
  CHECK(mm_wx_delta(0.5, 1.0, 0.0, 0.0, 1.0) == 4.0);
  CHECK(kWxStream == 6 && kWxStream != kXchgStream && kWxRec == 11);

  // ---- settings
  CHECK(mm_wx_check_settings(2, 0, "t") == 0 && mm_wx_check_settings(64, 100, "t") == 0);
  CHECK(mm_wx_check_settings(1, 4, "t") == -1 && has("t: window exchange needs an ensemble handle with at least two replicas"));
  CHECK(mm_wx_check_settings(0, 4, "t") == -1 && has("at least two replicas"));
  CHECK(mm_wx_check_settings(3, -1, "t") == -1 && has("window exchange every >= 0"));
  // ---- equal kT
  {
    const double same[3] = {2.5, 2.5, 2.5}, differ[3] = {2.5, 2.5, 2.6};
    CHECK(mm_wx_check_kT(3, same, "t") == 0);
    CHECK(mm_wx_check_kT(3, differ, "t") == -1 && has("the same kT") && has("replica 2"));
  }
  // ---- the partners
  CHECK(mm_wx_check_partners(false, false, "t") == 0);
  CHECK(mm_wx_check_partners(true, false, "t") == -1 && has("together with temperature replica exchange"));
  CHECK(mm_wx_check_partners(false, true, "t") == -1 && has("together with a barostat"));
  // ---- the set: k, init, rate may differ, vec and origin may not
  {
    const int R = 3, P = 2;
    std::vector<double> q((size_t)R * P * kWxPullParams);
    for (int r = 0; r < R; ++r)
      for (int p = 0; p < P; ++p) {
        double* row = &q[((size_t)r * P + p) * kWxPullParams];
        row[0] = 500.0 + r, row[1] = 0.5 + 0.07 * r, row[2] = 1e-3 * r;
        row[3] = 0, row[4] = 0, row[5] = 1, row[6] = 0.1 * p, row[7] = 0.2, row[8] = 0.3;
      }
    CHECK(mm_wx_check_set(R, P, q.data(), "t") == 0);
    CHECK(mm_wx_check_set(R, 0, nullptr, "t") == 0 && mm_wx_check_set(R, P, nullptr, "t") == 0);
    std::vector<double> bad = q;
    bad[((size_t)2 * P + 1) * kWxPullParams + 4] = 0.5;
    CHECK(mm_wx_check_set(R, P, bad.data(), "t") == -1 && has("pull coordinate 1") && has("the same vec") && has("replica 2"));
    bad = q;
    bad[((size_t)1 * P + 0) * kWxPullParams + 8] = 0.31;
    CHECK(mm_wx_check_set(R, P, bad.data(), "t") == -1 && has("pull coordinate 0") && has("the same origin") && has("replica 1"));
    // ---- everything through the one check
    const double kT[3] = {2.5, 2.5, 2.5}, kT_bad[3] = {2.5, 2.0, 2.5};
    const int32_t perm[3] = {2, 0, 1}, twice[3] = {0, 0, 1};
    CHECK(mm_wx_check(R, 10, kT, false, false, P, q.data(), perm, "t") == 0);
    CHECK(mm_wx_check(R, 10, nullptr, false, false, 0, nullptr, nullptr, "t") == 0);
    CHECK(mm_wx_check(1, 10, nullptr, false, false, 0, nullptr, nullptr, "t") == -1 && has("at least two replicas"));
    CHECK(mm_wx_check(R, -2, nullptr, false, false, 0, nullptr, nullptr, "t") == -1 && has("every >= 0"));
    CHECK(mm_wx_check(R, 10, kT_bad, false, false, 0, nullptr, nullptr, "t") == -1 && has("the same kT"));
    CHECK(mm_wx_check(R, 10, kT, true, false, 0, nullptr, nullptr, "t") == -1 && has("temperature replica exchange"));
    CHECK(mm_wx_check(R, 10, kT, false, true, 0, nullptr, nullptr, "t") == -1 && has("barostat"));
    CHECK(mm_wx_check(R, 0, kT, true, true, 0, nullptr, nullptr, "t") == 0);  // off: nothing to clash with
    CHECK(mm_wx_check(R, 10, kT, false, false, P, bad.data(), nullptr, "t") == -1 && has("origin"));
    CHECK(mm_wx_check(R, 10, kT, false, false, -1, nullptr, nullptr, "t") == -1 && has("n_pull"));
    CHECK(mm_wx_check(R, 10, kT, false, false, P, q.data(), twice, "t") == -1 && has("window_of_slot must be a permutation of 0 .. 2"));
  }
  // ---- the permutation check of an assignment
  {
    const int32_t id[4] = {0, 1, 2, 3}, perm[4] = {2, 0, 3, 1}, twice[4] = {0, 1, 1, 3}, high[4] = {0, 1, 2, 4}, neg[4] = {0, -1, 2, 3};
    CHECK(mm_wx_check_windows(4, id, "t") == 0 && mm_wx_check_windows(4, perm, "t") == 0);
    CHECK(mm_wx_check_windows(4, twice, "t") == -1 && has("t: window_of_slot must be a permutation of 0 .. 3"));
    CHECK(mm_wx_check_windows(4, high, "t") == -1 && mm_wx_check_windows(4, neg, "t") == -1 && mm_wx_check_windows(4, nullptr, "t") == -1);
    CHECK(mm_wx_check_windows(1, id, "t") == -1 && has("at least two replicas"));
  }
  // ---- the row plan: for R = 2 .. 5, from every assignment to every other.  Row w starts as {w, w + 0.5} in slot w; after a
  // move to `want` slot s must hold the row of window want[s], whatever the assignment before.
  long plans = 0;
  for (int R = 2; R <= 5; ++R) {
    std::vector<int32_t> cur((size_t)R), want((size_t)R);
    std::iota(cur.begin(), cur.end(), 0);
    do {
      std::vector<double> rows((size_t)R * 2);
      for (int s = 0; s < R; ++s) rows[2 * (size_t)s] = cur[(size_t)s], rows[2 * (size_t)s + 1] = cur[(size_t)s] + 0.5;
      std::iota(want.begin(), want.end(), 0);
      do {
        const std::vector<int32_t> plan = mm_wx_row_plan(cur.data(), want.data(), R);
        CHECK((int)plan.size() == R && mm_is_permutation(plan.data(), R));
        std::vector<double> moved = rows;
        mm_wx_permute_rows(moved, 2, plan);
        for (int s = 0; s < R; ++s) CHECK(moved[2 * (size_t)s] == want[(size_t)s] && moved[2 * (size_t)s + 1] == want[(size_t)s] + 0.5);
        if (cur == want)
          for (int s = 0; s < R; ++s) CHECK(plan[(size_t)s] == s);
        ++plans;
      } while (std::next_permutation(want.begin(), want.end()));
    } while (std::next_permutation(cur.begin(), cur.end()));
  }
  CHECK(plans == 2L * 2 + 6L * 6 + 24L * 24 + 120L * 120);
  {  // rows of length zero (a set without that kind of term) stay empty
    std::vector<double> none;
    mm_wx_permute_rows(none, 0, {1, 0});
    CHECK(none.empty());
  }
  std::printf("ok (%ld plans)\n", plans);
  return 0;
}
