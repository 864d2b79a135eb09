// The host loop that drives a Langevin step kernel over the resident state, shared by the oxDNA integrator
// (advance_typed, langevin_core.inc) and the MARTINI one (martini_md.hip): per-run state, the segmented launch loop with its
// halt / rebuild / resume protocol, HIP-event timing, and the two small kernels behind it.
#ifndef MYTHOS_MD_DRIVER_H
#define MYTHOS_MD_DRIVER_H

#include <algorithm>
#include <string>

#include "mythos_internal.h"

namespace mythos {

// What an integrator carries from one call to the next, apart from its model's frames and lists.
struct MdRun {
  static constexpr int kCtlWords = 4;    // d_flags: [0] error bits (2 NaN), [1] halt, [2] progress, [3] aborted launch + 1
  static constexpr int kMaxSamples = 16;
  uint64_t seed = 0;
  int64_t step = 0;
  int cur = 0;              // the frame that holds the current state
  bool open = false;        // the frame holds x_n and momenta short of the closing half kick of step n (md_drive)
  bool resident = false;    // the frames hold a state (load, or the last run)
  bool list_valid = false;  // the rows were built from this state's history and the rebuild schedule continues
  bool list_fitted = false; // a synchronising, growing build has sized rows and buckets for this integrator
  int since_build = 0;      // steps taken since the rows were built
  int rebuild_every = 0;    // scheduled list rebuilds (0: a static list, oxDNA only)
  int timing_samples = 0;   // dispatches per run timed with their own event pair (set_timing; ~8 us each)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket a whole run
  hipEvent_t sa[kMaxSamples] = {}, sb[kMaxSamples] = {};
  DeviceBuf<int> d_flags;
  // control words as the device published them at the end of a segment: [0..3] d_flags, [4..6] the list builder's
  // overflow words.  Pinned host memory the publishing kernel writes directly: one stream synchronisation per segment
  // and no copy commands.
  PinnedBuf<int> ctl;
  double last_avg_ms = 0;     // (ev1 - ev0) / launches: includes rebuilds and inter-kernel gaps
  double last_kernel_ms = 0;  // mean over the sampled single-launch intervals
  int last_launches = 0, last_samples = 0;
  int last_recoveries = 0;  // halts of the last run that were rebuilt and resumed
  int last_rebuilds = 0;    // scheduled list rebuilds inside the last advance (the first build of a list not counted)

  MdRun() = default;
  MdRun(const MdRun&) = delete;
  MdRun& operator=(const MdRun&) = delete;
  // (the owner's destructor has selected the device; what md_run_create did not get to is null)
  ~MdRun() {
    for (hipEvent_t e : {ev0, ev1})
      if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < kMaxSamples; ++k) {
      if (sa[k]) (void)hipEventDestroy(sa[k]);
      if (sb[k]) (void)hipEventDestroy(sb[k]);
    }
  }
};

// events, control words (cleared) and their pinned host copy; false on failure (the destructor frees what was made)
inline bool md_run_create(MdRun& r) {
  bool ok = r.d_flags.alloc(MdRun::kCtlWords) == 0 && hipMemset(r.d_flags.get(), 0, MdRun::kCtlWords * sizeof(int)) == hipSuccess &&
            r.ctl.alloc(8) == 0 && hipEventCreate(&r.ev0) == hipSuccess && hipEventCreate(&r.ev1) == hipSuccess;
  if (ok) std::fill(r.ctl.host(), r.ctl.host() + 8, 0);
  for (int k = 0; ok && k < MdRun::kMaxSamples; ++k)
    ok = hipEventCreate(&r.sa[k]) == hipSuccess && hipEventCreate(&r.sb[k]) == hipSuccess;
  return ok;
}

// End of a segment: hand the control words to the host (pinned memory) and clear the ones a later segment starts
// from, so that neither a copy command nor a memset sits between two runs.
static __global__ void publish_ctl_kernel(int* __restrict__ flags, const int* __restrict__ overflow, int* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out[0] = flags[0], out[1] = flags[1], out[2] = flags[2], out[3] = flags[3];
  out[4] = overflow ? overflow[0] : 0, out[5] = overflow ? overflow[1] : 0, out[6] = overflow ? overflow[2] : 0;
  flags[0] = 0, flags[2] = 0;  // the halt word stays until the host has recovered (later launches must see it)
}

// Energy-trace row of a saved step: the step kernel's per-workgroup partials [n_blocks][WIDTH] summed.  256 threads =
// 16 columns x 16 groups of workgroup partials, the group sums added in a fixed order (one thread per column was a
// chain of n_blocks dependent loads: 110 us per saved step at 12 kbp)
template <int WIDTH>
static __global__ __launch_bounds__(256) void reduce_trace_kernel(const double* __restrict__ part, int n_blocks, double* __restrict__ out) {
  static_assert(WIDTH <= 16, "one column per trace entry");
  __shared__ double acc[16][17];
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  double s = 0.0;
  if (k < WIDTH)
    for (int b = g; b < n_blocks; b += 16) s += part[(size_t)b * WIDTH + k];
  acc[g][k] = s;
  __syncthreads();
  if (g == 0 && k < WIDTH && out) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) t += acc[j][k];
    out[k] = t;
  }
}

// One call of md_drive.
struct MdDrive {
  const char* who;  // error-message prefix
  int n_steps, save_every;
  bool close;        // end on a closing-only launch (see md_drive)
  bool energy_rows;  // saved rows carry energies (energy-trace instantiation at x_k plus a reduction)
  bool plain_rows;   // saved rows without energies (written by the launch that produces the saved state)
  bool dynamic_list; // the rows follow the state: scheduled rebuilds, halts and recoveries (false: static rows)
  int* halt_words;   // the list builder's overflow words, which the step kernels watch (null with static rows)
  const int* row_stride;  // current row capacity (the overflow test hook claims one more)
  double skin;
  std::string give_up_hint;  // appended to the error that ends a run after kMaxRecoveries
  hipStream_t st;
};

// What one step launch does, besides its index k.
struct LaunchRow {
  int cur;           // the frame the launch reads (it writes cur ^ 1)
  bool save;         // energy-trace row sidx at x_k (a reduction launch follows)
  bool save_next;    // the launch's output, x_{k+1}, is row sidx
  int sidx;
  float kick_close;  // 0 on the first launch of a closed frame, 1/2 otherwise
  int do_step;       // 0: the closing-only launch
  int built_at;      // k index at which the rows in use were built (negative: so many steps before this call)
  hipEvent_t ea, eb; // the dispatch's own begin / end time stamps (null: not sampled)
};

// n_steps on the resident state and ONE stream synchronisation per segment of kSegment launches - the host has to see
// the halt word before it can say the steps were taken.  Nothing else is between two calls: the list and its rebuild
// schedule carry over, the control words are published and cleared by a one-thread kernel, events are recorded only
// when timing was asked for.
// Launch k evaluates the forces at x_k, closes step k - 1 with them (the second half kick) and takes step k up to its
// first half kick and drift.  close = true: n_steps + 1 launches, the last one only closes (momenta p_n in the frame).
// close = false (advance): n_steps launches; the frame is left OPEN - x_n with momenta short of their closing half
// kick - and whoever comes next supplies it with the force evaluation it needs anyway: the next advance in its first
// launch (which is then the same launch as launch n of one longer call: advance(a); advance(b) is advance(a + b) launch
// for launch), store through a zero-step closing call.  A call whose last step saves an energy row evaluates at x_n
// for that row and closes while it is there.
// The model comes in as callables:
//   launch(k, const LaunchRow&)  the step launch (and the trace reduction behind a saving one)
//   rebuild(buf)                 scheduled list build from frame buf (cannot stop to grow: an overflow halts the launches)
//   rebuild_until_fit(buf)       synchronising build from frame buf that grows rows and buckets until they fit
//   on_abort()                   a launch aborted (its work lists were too short): 0 to run it again wider, or an error
// each build returning 0 or an error code.
template <class Launch, class Rebuild, class RebuildUntilFit, class OnAbort>
static int md_drive(MdRun& run, const MdDrive& d, Launch&& launch, Rebuild&& rebuild, RebuildUntilFit&& rebuild_until_fit,
                    OnAbort&& on_abort) {
  const bool closes = d.close || (d.energy_rows && d.n_steps > 0 && d.n_steps % d.save_every == 0);
  const int n_launch = closes ? d.n_steps + 1 : d.n_steps;
  if (n_launch == 0) return MYTHOS_OK;  // (advance(0) on an open or a closed frame: nothing to do)
  const hipStream_t st = d.st;
  const bool was_open = run.open;
  const int cur0 = run.cur;
  int built_at = 0;
  if (d.dynamic_list) {
    if (!run.list_fitted) {
      // the first build of this integrator sizes rows (a quarter of headroom) and cell buckets (none more than half
      // full) with a synchronising build; later ones just rebuild - should that overflow, the next step kernel
      // halts and the recovery below grows what is needed
      if (int rc = rebuild_until_fit(cur0)) return rc;
      run.list_fitted = true;
    } else if (!run.list_valid) {
      if (int rc = rebuild(cur0)) return rc;
    } else {
      built_at = -run.since_build;
    }
    run.list_valid = true;
  }
  const bool timing = run.timing_samples > 0;
  if (timing) MYTHOS_HIP_TRY(hipEventRecord(run.ev0, st));
  int launches = 0, samples = 0, recoveries = 0, scheduled = 0;
  const int max_samples = std::min(run.timing_samples, MdRun::kMaxSamples);  // 0: no dispatch is bracketed
  const int sample_stride = std::max(1, n_launch / std::max(1, max_samples));
  // An error ends the call with rows that belong to no state - the next call builds them again - and clean halt and
  // overflow words ...
  auto drop_list = [&]() {
    run.list_valid = false;
    run.since_build = 0;
    run.last_recoveries = recoveries;
    run.last_rebuilds = scheduled;
    (void)hipMemsetAsync(run.d_flags.get() + 1, 0, 3 * sizeof(int), st);
    if (d.halt_words) (void)hipMemsetAsync(d.halt_words, 0, kOverflowWords * sizeof(int), st);
  };
  // ... and the state that kernels 0 .. ran - 1 left: positions after the last step that counted, momenta short of its
  // closing half kick
  auto fail = [&](int ran, int rc) -> int {
    run.cur = cur0 ^ (ran & 1);
    run.step += ran;
    run.open = was_open || ran > 0;
    drop_list();
    return rc;
  };
  // The kernels of a run are queued in segments of kSegment; after each the host looks at the halt word.  A step that
  // moves a particle out of its skin, or a rebuild that overflows its rows or spill list, halts the launches behind it
  // (they return at once); the host then rebuilds at the last valid state - growing what overflowed - and resumes
  // there.  A run never integrates on a stale or truncated list, and neither condition is an error; what it costs is
  // the empty launches behind the halt (at most a segment) and a synchronisation.
  constexpr int kMaxRecoveries = 64;
  const long long dbg_seg = debug_value(MYTHOS_DEBUG_MD_SEGMENT);
  const int kSegment = dbg_seg > 0 ? (int)std::min<long long>(dbg_seg, 1 << 20) : 8192;
  int k = 0, seg_len = kSegment;  // a run that has halted once looks more often: less queued behind the next halt
  int cur = cur0;
  while (k < n_launch) {
    // The device's progress word (flags[2], cleared by publish_ctl_kernel after every segment) says nothing when the
    // FIRST launch of a segment halts before writing it (a scheduled rebuild in front of it overflowed): the launches
    // of the earlier segments count all the same.
    const int seg_start = k, seg_end = std::min(n_launch - 1, k + seg_len - 1);
    for (; k <= seg_end; ++k) {
      const bool last = (k == d.n_steps);  // (reached only by a call that closes)
      LaunchRow row;
      row.cur = cur;
      row.save = d.energy_rows && k > 0 && (k % d.save_every == 0);
      row.save_next = d.plain_rows && !last && ((k + 1) % d.save_every == 0);
      row.sidx = row.save ? (k / d.save_every - 1) : (row.save_next ? ((k + 1) / d.save_every - 1) : 0);
      // (a closing-only launch rebuilds too when the schedule says so: the launch a longer call would issue at this index
      // does, and the forces that close step n must come off the same rows either way - sums over rows built at different
      // states differ in their last bits)
      if (d.dynamic_list && k - built_at >= run.rebuild_every) {
        if (int rc = rebuild(cur)) return fail(k, rc);
        built_at = k;
        ++scheduled;
        if (debug_value(MYTHOS_DEBUG_MD_OVERFLOW_AT) == k + 1) {  // test hook: this build claims a row did not fit
          debug_clear(MYTHOS_DEBUG_MD_OVERFLOW_AT);
          MYTHOS_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d.halt_words, *d.row_stride + 1, 1, st));
        }
      }
      row.kick_close = (k == 0 && !was_open) ? 0.0f : 0.5f;
      row.do_step = last ? 0 : 1;
      row.built_at = built_at;
      row.ea = row.eb = nullptr;
      if (!row.save && (k % sample_stride == sample_stride / 2) && samples < max_samples)
        row.ea = run.sa[samples], row.eb = run.sb[samples], ++samples;
      launch(k, row);
      ++launches;
      cur ^= 1;
    }
    if (timing && k >= n_launch) MYTHOS_HIP_TRY(hipEventRecord(run.ev1, st));
    hipLaunchKernelGGL(publish_ctl_kernel, dim3(1), dim3(1), 0, st, run.d_flags.get(), (const int*)d.halt_words, run.ctl.dev());
    MYTHOS_HIP_TRY(hipGetLastError());
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
    const int* ctl = run.ctl.host();
    if (ctl[0] & 2) {  // NaN: the state is lost
      drop_list();
      run.resident = false;
      run.step += d.n_steps;
      run.last_avg_ms = run.last_kernel_ms = 0.0;  // (ev1 is recorded only behind the last segment)
      run.last_launches = launches;
      run.last_samples = samples;
      set_error(std::string(d.who) + ": NaN in the state (time step too large or overlapping start configuration)");
      return MYTHOS_ERR_NUMERIC;
    }
    const int aborted = ctl[3];  // launch index + 1 whose angular work lists were too short (its output does not count)
    if (ctl[1] == 0 && ctl[4] == 0 && ctl[5] == 0 && aborted == 0) continue;  // nothing halted
    if (aborted != 0) {
      if (int rc = on_abort()) return fail(aborted - 1, rc);
    } else if (!d.dynamic_list) {
      break;  // (a static list cannot halt; defensive)
    }
    // kernels 0 .. ran-1 count; the state they left is in the frame kernel `ran` reads (an aborted launch and
    // everything behind it do not count: their inputs are untouched)
    const int progressed = std::max(ctl[2], seg_start);
    const int ran = aborted != 0 ? std::min(progressed, aborted - 1) : progressed;
    if (++recoveries > kMaxRecoveries) {
      set_error(std::string(d.who) + ": the neighbour list had to be rebuilt out of turn more than " + std::to_string(kMaxRecoveries) +
                " times in one run: the skin (" + std::to_string(d.skin) + ") is too small for a rebuild every " +
                std::to_string(run.rebuild_every) + " steps" + d.give_up_hint);
      return fail(ran, MYTHOS_ERR_OVERFLOW);
    }
    cur = cur0 ^ (ran & 1);
    k = ran;
    seg_len = std::max(std::min(256, kSegment), seg_len / 4);
    MYTHOS_HIP_TRY(hipMemsetAsync(run.d_flags.get() + 1, 0, 3 * sizeof(int), st));
    if (d.dynamic_list) {
      if (int rc = rebuild_until_fit(cur)) return fail(ran, rc);
      built_at = k;
    }
  }
  run.last_recoveries = recoveries;
  run.last_rebuilds = scheduled;
  run.cur = cur;
  run.open = !closes;
  run.since_build = d.n_steps - built_at;
  if (timing) {
    float ms = 0;
    MYTHOS_HIP_TRY(hipEventElapsedTime(&ms, run.ev0, run.ev1));
    run.last_avg_ms = launches ? double(ms) / launches : 0.0;
    double acc = 0;
    for (int s = 0; s < samples; ++s) {
      float t = 0;
      MYTHOS_HIP_TRY(hipEventElapsedTime(&t, run.sa[s], run.sb[s]));
      acc += t;
    }
    run.last_kernel_ms = samples ? acc / samples : 0.0;
  } else {
    run.last_avg_ms = run.last_kernel_ms = 0.0;
  }
  run.last_launches = launches;
  run.last_samples = samples;
  run.step += d.n_steps;
  return MYTHOS_OK;
}

// ---- the C entry points both integrators share (mythos_langevin_* / mythos_martini_langevin_*)
inline int md_set_timing(MdRun* r, int samples, const char* who) {
  if (!r || samples < 0) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  r->timing_samples = std::min(samples, MdRun::kMaxSamples);
  return MYTHOS_OK;
}

inline int md_last_kernel_ms(const MdRun* r, double* kernel_ms, double* loop_ms_per_launch, int* launches, int* samples,
                             const char* who) {
  if (!r) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (kernel_ms) *kernel_ms = r->last_kernel_ms;
  if (loop_ms_per_launch) *loop_ms_per_launch = r->last_avg_ms;
  if (launches) *launches = r->last_launches;
  if (samples) *samples = r->last_samples;
  return MYTHOS_OK;
}

// *out = r->*field: last_recoveries, last_rebuilds
inline int md_last_count(const MdRun* r, int MdRun::*field, int* out, const char* who) {
  if (!r || !out) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  *out = r->*field;
  return MYTHOS_OK;
}

inline int64_t md_get_step(const MdRun* r) { return r ? r->step : -1; }

}  // namespace mythos

#endif  // MYTHOS_MD_DRIVER_H
