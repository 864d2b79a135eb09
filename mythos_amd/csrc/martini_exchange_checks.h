// Host bookkeeping of temperature replica exchange in the MARTINI ensemble (mythos_martini_langevin_set_exchange) that needs
// no device: which rung pairs an event attempts, the decision, how every advance with events - coupling, temperature
// exchange, window exchange - is cut at them and at saved rows and what the one loop passes on for each chunk
// (mm_event_chunk, mm_chunk_plan), the permutation check of a ladder, the scalar reference pressure of the work term, and what is refused.  In the
// style of martini_ensemble_checks.h - the standard library and set_error alone, so tests/host/martini_exchange_main.cpp
// compiles it as it is under the host sanitizers.  What mm_exchange_kernel shares with the host (the pair schedule, the
// decision) is marked MYTHOS_XHD: __host__ __device__ under hipcc, nothing otherwise.
#ifndef MYTHOS_MARTINI_EXCHANGE_CHECKS_H
#define MYTHOS_MARTINI_EXCHANGE_CHECKS_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MYTHOS_XHD __host__ __device__
#else
#define MYTHOS_XHD
#endif

namespace mythos {

void set_error(const std::string& msg);

constexpr int kXchgRec = 11;  // step, t, slot A, slot B, U_A, U_B, V_A, V_B, d, u, accepted
constexpr uint32_t kXchgStream = 5;  // Philox stream (0/1 thermostat, 2/3 barostat, 4 umbrella, 7/8 initial velocities)
constexpr double kXchgBarPerKjMolNm3 = 16.6053907;

// ---- the pair schedule: attempt a tries the rung pairs (t, t + 1), t = a mod 2, a mod 2 + 2, ... while t + 1 < n_rep
MYTHOS_XHD inline int mm_xchg_first_rung(int64_t attempt) { return (int)(attempt & 1); }
MYTHOS_XHD inline int mm_xchg_n_pairs(int n_rep, int64_t attempt) {
  const int left = n_rep - mm_xchg_first_rung(attempt);
  return left > 0 ? left / 2 : 0;
}
MYTHOS_XHD inline int mm_xchg_pair_rung(int64_t attempt, int p) { return mm_xchg_first_rung(attempt) + 2 * p; }
// the lower rung of the pair that rung g belongs to at this attempt, or -1: g sits out
MYTHOS_XHD inline int mm_xchg_pair_of_rung(int n_rep, int64_t attempt, int g) {
  const int f = mm_xchg_first_rung(attempt);
  if (g < f) return -1;
  const int t = g - ((g - f) & 1);
  return t + 1 < n_rep ? t : -1;
}

// ---- the decision: d = (beta_t - beta_t+1) (H_A - H_B), H = U + p V, for slot A on rung t and slot B on rung t + 1
MYTHOS_XHD inline double mm_xchg_delta(double kT_t, double kT_t1, double U_A, double V_A, double U_B, double V_B, double p) {
  const double H_A = U_A + p * V_A, H_B = U_B + p * V_B;
  return (1.0 / kT_t - 1.0 / kT_t1) * (H_A - H_B);
}
MYTHOS_XHD inline bool mm_xchg_accept(double d, double u) { return d >= 0.0 || u < exp(d); }
// what a slot's velocities are multiplied by when its kT goes from kT_old to kT_new (rounded once more to the system's reals)
MYTHOS_XHD inline double mm_xchg_vel_factor(double kT_old, double kT_new) { return sqrt(kT_new / kT_old); }

// ---- chunks of an advance with events (mm_advance_chunked, martini_md.hip: under a barostat, temperature exchange or
// window exchange): the next chunk ends at the next coupling event, the next exchange event (both on the absolute step
// counter; every == 0: none), the next saved row (counted from the call's first step) or the end of the call, whichever
// comes first
struct MmEventChunk {
  int len;
  bool couple, exchange, save, last;
};
inline MmEventChunk mm_event_chunk(int64_t step, int couple_every, int exchange_every, int done, int n_steps, int save_every) {
  const int never = n_steps + 1;
  const int to_couple = couple_every > 0 ? couple_every - (int)(step % couple_every) : never;
  const int to_exchange = exchange_every > 0 ? exchange_every - (int)(step % exchange_every) : never;
  const int to_save = save_every > 0 ? save_every - done % save_every : never;
  const int len = std::min(std::min(to_couple, to_exchange), std::min(to_save, n_steps - done));
  return {len, len == to_couple, len == to_exchange, len == to_save, done + len == n_steps};
}

// What the integrator's one call for a chunk is given.  An event needs the closed state, so a chunk that ends at one
// closes; the last chunk closes if the caller's call does.  A temperature event needs U(x_s) of every slot, so its chunk
// ends on an energy row whether the caller saves that step or not: the caller's row if it saves the step with energies,
// the exchange's scratch row otherwise.  A window event needs no energy row.
enum MmExchangeKind { kMmNoExchange = 0, kMmTemperatureExchange, kMmWindowExchange };
enum MmEnergyRow { kMmNoEnergyRow = 0, kMmCallerRow, kMmScratchRow };
struct MmChunkPlan {
  bool close;
  int save_every;      // c.len: the chunk's last step is a row; 0: the chunk saves nothing
  MmEnergyRow energy;  // where that row's energies go
};
inline MmChunkPlan mm_chunk_plan(const MmEventChunk& c, bool close, MmExchangeKind kind, bool caller_energies) {
  const bool needs_u = c.exchange && kind == kMmTemperatureExchange;
  const MmEnergyRow energy = (c.save && caller_energies) ? kMmCallerRow : (needs_u ? kMmScratchRow : kMmNoEnergyRow);
  return {c.couple || c.exchange || (c.last && close), (c.save || needs_u) ? c.len : 0, energy};
}

// Row r of a per-row array of `copies` records of `width` values each: where chunked output lands
inline size_t mm_row_offset(int row, int copies, size_t width) { return (size_t)row * copies * width; }

inline bool mm_is_permutation(const int32_t* p, int n) {
  if (!p || n < 1) return false;
  std::vector<char> seen((size_t)n, 0);
  for (int r = 0; r < n; ++r) {
    if (p[r] < 0 || p[r] >= n || seen[(size_t)p[r]]) return false;
    seen[(size_t)p[r]] = 1;
  }
  return true;
}

// ---- refusals: 0, or -1 (MYTHOS_ERR_INVALID_ARGUMENT) with "<who>: ..." as the error message
inline int mm_xchg_check_settings(int n_rep, int every, const char* who) {
  if (n_rep < 2) {
    set_error(std::string(who) + ": replica exchange needs an ensemble handle with at least two replicas (n_rep >= 2)");
    return -1;
  }
  if (every < 0) {
    set_error(std::string(who) + ": exchange every >= 0 required (0 switches exchange off)");
    return -1;
  }
  return 0;
}
inline int mm_xchg_check_ladder(int n_rep, const int32_t* rung_of_slot, const char* who) {
  if (n_rep < 2) return mm_xchg_check_settings(n_rep, 0, who);
  if (!mm_is_permutation(rung_of_slot, n_rep)) {
    set_error(std::string(who) + ": rung_of_slot must be a permutation of 0 .. " + std::to_string(n_rep - 1));
    return -1;
  }
  return 0;
}

// The pressure of the work term p V (kJ/mol/nm^3) under the barostat that is set: 0 without coupling, ref_p[0] for isotropic
// coupling, for semi-isotropic coupling the reference pressure of the axis set that is compressible.  Both compressible
// with different reference pressures is refused: an anisotropic reference stress has no scalar work term.
inline int mm_xchg_pressure(bool barostat_on, int coupling, const double ref_p[2], const double beta[2], double* p, const char* who) {
  double p_ref = 0.0;
  if (!barostat_on) {
    *p = 0.0;
    return 0;
  }
  if (coupling == 0) {
    p_ref = ref_p[0];
  } else if (beta[0] > 0 && beta[1] > 0) {
    if (ref_p[0] != ref_p[1]) {
      set_error(std::string(who) + ": replica exchange under semi-isotropic coupling with both compressibilities non-zero needs "
                "ref_p[0] == ref_p[1] (" + std::to_string(ref_p[0]) + " != " + std::to_string(ref_p[1]) +
                "): an anisotropic reference stress has no scalar work term p V");
      return -1;
    }
    p_ref = ref_p[0];
  } else {
    p_ref = beta[0] > 0 ? ref_p[0] : ref_p[1];
  }
  *p = p_ref / kXchgBarPerKjMolNm3;
  return 0;
}

}  // namespace mythos

#endif  // MYTHOS_MARTINI_EXCHANGE_CHECKS_H
