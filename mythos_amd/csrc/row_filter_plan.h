// The schedule of the oxDNA integrator's candidate rows (neighbors.hip: filter_rows_kernel): which list
// rebuilds of a run start with a WIDE build - the cell builder at list range + margin, centre criterion only, into the
// candidate store - and which only FILTER the candidates they find there into the rows.  Every rebuild ends in a filter,
// and a filter either writes the rows the full builder would have written at that frame or halts the launches behind
// it, so a wrong choice here fails no parity test and only loses speed (a wide build too many) or costs a recovery
// (one too few).  The choice is therefore plain host arithmetic with no HIP in it, as md_plan.h is; the CPU suite pins
// its boundaries (tests/test_row_filter_plan_cpu.py).
#pragma once

namespace mythos {

// Rebuilds per candidate build: the wide build of rebuild 0 serves the filters of rebuilds 0 .. kCandEvery - 1.
constexpr int kCandEvery = 8;
// How far beyond the list range (r_cut + skin) the candidates reach, in thousandths of a length unit.  A candidate row
// vouches for a filtered row while no centre has moved more than half the margin since the wide build; the rule is
// margin >= 1.15 * 2 * (largest centre displacement over kCandEvery rebuild intervals), the cushion the skin keeps over
// one interval.  The thermalised 12 kbp duplex moves 0.76 at most in 400 steps (1.75 by the rule); a scan on the GPU
// has 172 / 57 / 1 / 0 out-of-turn rebuilds in 60 000 steps at margins of 1.4 / 1.6 / 1.8 / 2.0, and none at 2.0 in
// fp64 or at 100 kbp.  profiles/r07_row_filter.md has the curve and the scan.
constexpr int kCandMarginMilli = 2000;

// debug_every / debug_margin_milli: mythos_debug_set(MYTHOS_DEBUG_ROWS_CAND_EVERY / _CAND_MARGIN), 0 = the constants
inline int cand_every_for(long long debug_every) { return debug_every > 0 ? (int)(debug_every > 1 << 20 ? 1 << 20 : debug_every) : kCandEvery; }
inline double cand_margin_for(long long debug_margin_milli) { return 1e-3 * double(debug_margin_milli > 0 ? debug_margin_milli : kCandMarginMilli); }

// The squared displacement beyond which a nucleotide's candidate row no longer vouches for its row.  Half the margin
// each for the two nucleotides of a pair is the triangle inequality in exact arithmetic; the distances are computed
// in the system's precision, so the filter gives up a five-hundredth of the half margin early (fp32 rounding of a
// squared distance of ~25 is 3e-6: three orders below what is given up).
inline double cand_stale_sq(double margin) {
  const double h = 0.5 * margin * (1.0 - 1.0 / 512.0);
  return h * h;
}

// What an integrator carries of the schedule from one call to the next, next to MdRun::since_build.
struct CandState {
  int age = -1;          // rebuilds filtered from the candidates in the store, the wide build's own included; < 0: none valid
  int margin_milli = 0;  // the margin they were built with
};

// The next rebuild (scheduled, or the first of a list) is wide: no valid candidates - the first build after a load, a
// new neighbour policy, a dropped list (list_valid false) or a build by the full builder -, another margin than they
// were built with, or kCandEvery rebuilds served.
inline bool cand_rebuild_is_wide(const CandState& c, bool list_valid, int every, int margin_milli) {
  return !list_valid || c.age < 0 || c.margin_milli != margin_milli || c.age >= every;
}

// ... and the state behind it.  A recovery (the synchronising build after a halt) is always wide: cand_after(true, ..).
inline CandState cand_after(bool wide, const CandState& c, int margin_milli) {
  return wide ? CandState{1, margin_milli} : CandState{c.age + 1, c.margin_milli};
}

// a build by the full builder (rows_filter = 0, or a system the cell path does not take): the store vouches for nothing
inline CandState cand_none() { return CandState{}; }

}  // namespace mythos
