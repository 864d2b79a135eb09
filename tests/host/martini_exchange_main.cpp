// Stand-alone host program for mythos_amd/csrc/martini_exchange_checks.h, built with -fsanitize=address,undefined by
// tests/test_martini_exchange_cpu.py: the pair schedule of replica exchange, the chunking of an advance with coupling and
// exchange events against a step-by-step loop, what mm_chunk_plan hands the integrator for every chunk, the permutation check, the choice of the reference pressure, every refusal,
// and detailed balance through the real mm_xchg_accept.  Exit code 0 and "ok" on success.
// With the argument "flip" the detailed-balance chain negates d before it asks mm_xchg_accept: the program then has to fail.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "martini_exchange_checks.h"

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

// what one call of the chunked advance does, as (step, what) records: 's' a saved row, 'x' an exchange, 'c' a coupling event
struct Mark {
  int64_t step;
  char what;
  bool operator==(const Mark& o) const { return step == o.step && what == o.what; }
};

static int walk_chunks(int64_t& step, int couple, int exchange, int n_steps, int save_every, std::vector<Mark>& out, long& chunks) {
  int done = 0;
  while (done < n_steps) {
    const MmEventChunk c = mm_event_chunk(step, couple, exchange, done, n_steps, save_every);
    CHECK(c.len >= 1 && done + c.len <= n_steps);
    step += c.len, done += c.len, ++chunks;
    CHECK(c.last == (done == n_steps));
    // the order inside a step: the row (the state before both events), the exchange, the coupling
    if (c.save) out.push_back({step, 's'});
    if (c.exchange) out.push_back({step, 'x'});
    if (c.couple) out.push_back({step, 'c'});
  }
  return 0;
}

// the plan of every chunk of one call against its rules, written out; kind none: a call without exchange events
static int walk_plans(int64_t& step, int couple, int exchange, int n_steps, int save_every, MmExchangeKind kind, bool close, bool energies,
                      long& plans) {
  int done = 0;
  while (done < n_steps) {
    const MmEventChunk c = mm_event_chunk(step, couple, kind == kMmNoExchange ? 0 : exchange, done, n_steps, save_every);
    const MmChunkPlan p = mm_chunk_plan(c, close, kind, energies);
    step += c.len, done += c.len, ++plans;
    CHECK(p.close == (c.couple || c.exchange || (c.last && close)));
    CHECK(p.save_every == ((c.save || (c.exchange && kind == kMmTemperatureExchange)) ? c.len : 0));
    CHECK((p.energy == kMmCallerRow) == (c.save && energies));
    CHECK((p.energy == kMmScratchRow) == (kind == kMmTemperatureExchange && c.exchange && !(c.save && energies)));
    CHECK(p.energy == kMmNoEnergyRow || p.save_every == c.len);  // an energy row is a saved row of the chunk's call
    if (kind != kMmTemperatureExchange) CHECK(p.energy == kMmNoEnergyRow || (c.save && energies));  // never a row the caller did not ask for
  }
  return 0;
}

static void walk_steps(int64_t& step, int couple, int exchange, int n_steps, int save_every, std::vector<Mark>& out) {
  for (int k = 1; k <= n_steps; ++k) {
    ++step;
    if (save_every > 0 && k % save_every == 0) out.push_back({step, 's'});
    if (exchange > 0 && step % exchange == 0) out.push_back({step, 'x'});
    if (couple > 0 && step % couple == 0) out.push_back({step, 'c'});
  }
}

int main(int argc, char** argv) {
  const bool flip = argc > 1 && std::strcmp(argv[1], "flip") == 0;
  // ---- the pair schedule, R = 2 .. 5 over consecutive attempts
  for (int n_rep = 2; n_rep <= 5; ++n_rep)
    for (int64_t a = 1; a <= 9; ++a) {
      std::vector<int> want;
      for (int t = (int)(a % 2); t + 1 < n_rep; t += 2) want.push_back(t);
      CHECK(mm_xchg_n_pairs(n_rep, a) == (int)want.size());
      std::vector<int> in_pair((size_t)n_rep, -1);
      for (int p = 0; p < (int)want.size(); ++p) {
        CHECK(mm_xchg_pair_rung(a, p) == want[(size_t)p]);
        in_pair[(size_t)want[(size_t)p]] = in_pair[(size_t)want[(size_t)p] + 1] = want[(size_t)p];  // disjoint: written once
      }
      for (int g = 0; g < n_rep; ++g) CHECK(mm_xchg_pair_of_rung(n_rep, a, g) == in_pair[(size_t)g]);
    }
  CHECK(mm_xchg_n_pairs(2, 1) == 0 && mm_xchg_n_pairs(2, 2) == 1 && mm_xchg_n_pairs(5, 1) == 2 && mm_xchg_n_pairs(5, 2) == 2);
  CHECK(mm_xchg_n_pairs(1, 1) == 0 && mm_xchg_n_pairs(1, 2) == 0);

  // ---- chunks against the step loop: (coupling every, exchange every, save_every), one call and split calls
  long chunks = 0, plans = 0;
  const int combos[4][3] = {{3, 6, 3}, {4, 6, 5}, {0, 4, 0}, {3, 4, 1}};
  const std::vector<std::vector<int>> calls = {{48}, {10, 14, 24}, {1, 1, 46}, {12, 12, 12, 12}};
  for (const auto& cb : combos)
    for (const auto& split : calls)
      for (int64_t step0 : {0, 5, 12, 1000003}) {
        std::vector<Mark> got, want;
        int64_t sa = step0, sb = step0;
        for (int n : split) {
          if (walk_chunks(sa, cb[0], cb[1], n, cb[2], got, chunks)) return 1;
          walk_steps(sb, cb[0], cb[1], n, cb[2], want);
        }
        CHECK(sa == sb && got.size() == want.size());
        for (size_t k = 0; k < got.size(); ++k) CHECK(got[k] == want[k]);
        for (MmExchangeKind kind : {kMmNoExchange, kMmTemperatureExchange, kMmWindowExchange})
          for (int flags = 0; flags < 4; ++flags) {
            int64_t sp = step0;
            for (int n : split)
              if (walk_plans(sp, cb[0], cb[1], n, cb[2], kind, (flags & 1) != 0, (flags & 2) != 0, plans)) return 1;
            CHECK(sp == sb);
          }
        if (step0 == 0 && cb[0] == 3 && cb[1] == 6 && cb[2] == 3 && split.size() == 1) {
          // steps 6, 12, ...: a row, an exchange and a coupling event together, in that order
          size_t k = 0;
          while (k < got.size() && got[k].step < 6) ++k;
          CHECK(k + 2 < got.size() && got[k] == (Mark{6, 's'}) && got[k + 1] == (Mark{6, 'x'}) && got[k + 2] == (Mark{6, 'c'}));
        }
      }
  {  // neither event: the chunks of a plain call with rows; and no rows at all: one chunk
    const MmEventChunk c = mm_event_chunk(7, 0, 0, 0, 20, 0);
    CHECK(c.len == 20 && !c.couple && !c.exchange && !c.save && c.last);
    const MmEventChunk e = mm_event_chunk(7, 0, 0, 4, 20, 4);
    CHECK(e.len == 4 && !e.couple && !e.exchange && e.save && !e.last);
  }

  // ---- the permutation check
  {
    const int32_t id[4] = {0, 1, 2, 3}, perm[4] = {2, 0, 3, 1}, twice[4] = {0, 1, 1, 3}, high[4] = {0, 1, 2, 4}, neg[4] = {0, -1, 2, 3};
    CHECK(mm_is_permutation(id, 4) && mm_is_permutation(perm, 4) && mm_is_permutation(id, 1));
    CHECK(!mm_is_permutation(twice, 4) && !mm_is_permutation(high, 4) && !mm_is_permutation(neg, 4));
    CHECK(!mm_is_permutation(nullptr, 4) && !mm_is_permutation(id, 0));
    CHECK(mm_xchg_check_ladder(4, perm, "t") == 0);
    CHECK(mm_xchg_check_ladder(4, twice, "t") == -1 && has("t: rung_of_slot must be a permutation of 0 .. 3"));
    CHECK(mm_xchg_check_ladder(4, nullptr, "t") == -1 && has("permutation"));
    CHECK(mm_xchg_check_ladder(1, id, "t") == -1 && has("at least two replicas"));
  }
  // ---- settings
  CHECK(mm_xchg_check_settings(2, 0, "t") == 0 && mm_xchg_check_settings(8, 100, "t") == 0);
  CHECK(mm_xchg_check_settings(1, 4, "t") == -1 && has("at least two replicas"));
  CHECK(mm_xchg_check_settings(0, 4, "t") == -1 && has("at least two replicas"));
  CHECK(mm_xchg_check_settings(3, -1, "t") == -1 && has("every >= 0"));
  // ---- the reference pressure of the work term
  {
    double p = -1.0;
    const double ref[2] = {1.0, 2.0}, same[2] = {3.0, 3.0};
    const double both[2] = {3e-4, 3e-4}, xy[2] = {3e-4, 0.0}, z[2] = {0.0, 4.5e-5};
    CHECK(mm_xchg_pressure(false, 1, ref, both, &p, "t") == 0 && p == 0.0);
    CHECK(mm_xchg_pressure(true, 0, ref, both, &p, "t") == 0 && p == 1.0 / 16.6053907);
    CHECK(mm_xchg_pressure(true, 1, ref, xy, &p, "t") == 0 && p == 1.0 / 16.6053907);
    CHECK(mm_xchg_pressure(true, 1, ref, z, &p, "t") == 0 && p == 2.0 / 16.6053907);
    CHECK(mm_xchg_pressure(true, 1, same, both, &p, "t") == 0 && p == 3.0 / 16.6053907);
    p = -1.0;
    CHECK(mm_xchg_pressure(true, 1, ref, both, &p, "t") == -1 && has("no scalar work term") && has("ref_p[0] == ref_p[1]") && p == -1.0);
  }
  // ---- the decision
  CHECK(mm_xchg_accept(0.0, 0.999999) && mm_xchg_accept(1e-300, 0.999999) && mm_xchg_accept(700.0, 0.5));
  CHECK(mm_xchg_accept(-1.0, 0.36) && !mm_xchg_accept(-1.0, 0.37) && !mm_xchg_accept(-800.0, 1e-300));
  CHECK(!mm_xchg_accept(std::nan(""), 0.5));
  CHECK(mm_xchg_delta(1.0, 2.0, 5.0, 0.0, 3.0, 0.0, 0.0) == 1.0);  // the colder slot holds more energy: always swapped
  CHECK(mm_xchg_delta(1.0, 2.0, 3.0, 10.0, 3.0, 6.0, 0.5) == 1.0);
  CHECK(mm_xchg_vel_factor(1.0, 4.0) == 2.0 && mm_xchg_vel_factor(2.5, 2.5) == 1.0);

  // ---- detailed balance: four rungs, every slot's U drawn afresh and exactly from its rung's law at each attempt
  // (U = kT Gamma(k / 2, 1), k = 30); the swaps must leave every rung's law alone
  {
    constexpr int R = 4, k = 30;
    const double kT[R] = {1.0, 1.3, 1.7, 2.2};
    const long n_attempts = 200000;
    std::mt19937_64 gen(20260317);
    std::gamma_distribution<double> gamma(0.5 * k, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    int rung_of_slot[R] = {0, 1, 2, 3};
    bool visited[R][R] = {};
    double sum[R] = {0, 0, 0, 0};
    long accepted = 0, attempted = 0;
    for (long a = 1; a <= n_attempts; ++a) {
      double U[R];
      int slot_of_rung[R];
      for (int s = 0; s < R; ++s) U[s] = kT[rung_of_slot[s]] * gamma(gen), slot_of_rung[rung_of_slot[s]] = s;
      for (int p = 0; p < mm_xchg_n_pairs(R, a); ++p) {
        const int t = mm_xchg_pair_rung(a, p), A = slot_of_rung[t], B = slot_of_rung[t + 1];
        double d = mm_xchg_delta(kT[t], kT[t + 1], U[A], 0.0, U[B], 0.0, 0.0);
        if (flip) d = -d;
        ++attempted;
        if (mm_xchg_accept(d, uni(gen))) rung_of_slot[A] = t + 1, rung_of_slot[B] = t, ++accepted;
      }
      for (int s = 0; s < R; ++s) sum[rung_of_slot[s]] += U[s], visited[s][rung_of_slot[s]] = true;
    }
    double worst = 0.0;
    for (int t = 0; t < R; ++t) {
      const double mean = sum[t] / n_attempts, want = 0.5 * k * kT[t];
      const double se = kT[t] * std::sqrt(0.5 * k) / std::sqrt((double)n_attempts);
      worst = std::max(worst, std::fabs(mean - want) / se);
    }
    std::printf("detailed balance%s: %ld of %ld accepted, worst rung mean %.2f standard errors off\n", flip ? " (d flipped)" : "", accepted,
                attempted, worst);
    CHECK(worst < 4.0);
    for (int s = 0; s < R; ++s)
      for (int t = 0; t < R; ++t) CHECK(visited[s][t]);
  }
  std::printf("ok (%ld chunks, %ld plans)\n", chunks, plans);
  return 0;
}
