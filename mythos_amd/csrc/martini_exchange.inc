// Temperature replica exchange between the replicas of a MARTINI ensemble; included by martini_md.hip behind martini_npt.inc.
//
// The rule is stated in include/mythos_hip.h (mythos_martini_langevin_set_exchange) and DESIGN.md section 3.5l; what needs
// no device - the pair schedule, the decision, the chunking and its plan, the refusals - is martini_exchange_checks.h.
// Here: the decision kernel, the velocity rescale, the event, and what the event and the C entry points share with window
// exchange (MmPairExchange, martini_md.hip).  The loop that cuts an advance at the events is mm_advance_chunked (martini_md.hip).
//
// Slots are the replicas as they lie in memory; an exchange swaps the TEMPERATURES of two slots, no bead data moves.  An
// event needs U(x_s) of every slot: the chunk in front of it ends on a closing launch of the energy-trace instantiation and
// mm_reduce_trace_ens_kernel, into the caller's row if step s is saved with energies, into MmLadder::d_etrace otherwise
// (mm_chunk_plan).

namespace mythos {

struct MmXchgArgs {
  int n_rep, width;  // replicas; columns of an energy row (4, or 5 with the Coulomb column)
  double p;          // kJ/mol/nm^3: reference pressure of the work term, 0 without a barostat
  uint64_t seed;     // the exchange seed
  int64_t step, attempt;
};

// U of a slot from its energy row: lj + bond + angle (+ coulomb), added in that order (column 3 is the kinetic energy)
__device__ __forceinline__ double mm_xchg_potential(const double* __restrict__ row, int width) {
  double u = row[0] + row[1];
  u += row[2];
  if (width > 4) u += row[4];
  return u;
}

// One workgroup; slot s decides for itself.  It finds the pair its rung belongs to at this attempt and the slot that holds
// the other rung, evaluates the pair's decision - both members do, on the same numbers in the same order, so they agree -
// and writes its own new rung and velocity factor; the member on the lower rung writes the pair's log record.  Every word of
// the outputs is written once.  in_d: boxes [n_rep][3], then the ladder's kT [n_rep], and rung_in, all pinned host memory
// the host fills while the stream is idle; fac goes to device memory for mm_rescale_vel_ens_kernel, rung_out and log to
// pinned host memory, read behind the event's one synchronisation (the mm_barostat_kernel / publish_ctl_kernel pattern).
static __global__ __launch_bounds__(256) void mm_exchange_kernel(const double* __restrict__ e_rows, const double* __restrict__ in_d,
                                                                 const int* __restrict__ rung_in, const MmXchgArgs a,
                                                                 double* __restrict__ fac, int* __restrict__ rung_out,
                                                                 double* __restrict__ log) {
  const int n_rep = a.n_rep;
  const double* __restrict__ boxes = in_d;
  const double* __restrict__ kT = in_d + 3 * (size_t)n_rep;
  const int first = mm_xchg_first_rung(a.attempt);
  for (int s = threadIdx.x; s < n_rep; s += blockDim.x) {
    const int g = rung_in[s];
    const int t = mm_xchg_pair_of_rung(n_rep, a.attempt, g);
    int new_rung = g;
    double f = 1.0;
    if (t >= 0) {
      const int other = (g == t) ? t + 1 : t;
      int o = -1;
      for (int q = 0; q < n_rep; ++q)
        if (rung_in[q] == other) o = q;
      if (o >= 0) {  // (a permutation: always)
        const int A = (g == t) ? s : o, B = (g == t) ? o : s;  // A holds rung t, B rung t + 1
        const double U_A = mm_xchg_potential(e_rows + (size_t)A * a.width, a.width);
        const double U_B = mm_xchg_potential(e_rows + (size_t)B * a.width, a.width);
        const double V_A = (boxes[3 * A] * boxes[3 * A + 1]) * boxes[3 * A + 2];
        const double V_B = (boxes[3 * B] * boxes[3 * B + 1]) * boxes[3 * B + 2];
        const double d = mm_xchg_delta(kT[t], kT[t + 1], U_A, V_A, U_B, V_B, a.p);
        uint32_t c[4] = {(uint32_t)t, uint32_t((uint64_t)a.step), uint32_t((uint64_t)a.step >> 32), kXchgStream};
        philox4x32(c, uint32_t(a.seed), uint32_t(a.seed >> 32));
        const double u = (double(c[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
        const bool acc = mm_xchg_accept(d, u);
        if (acc) {
          new_rung = other;
          f = mm_xchg_vel_factor(kT[g], kT[other]);
        }
        if (g == t) {
          double* __restrict__ r = log + (size_t)((t - first) >> 1) * kXchgRec;
          r[0] = double(a.step), r[1] = double(t), r[2] = double(A), r[3] = double(B), r[4] = U_A, r[5] = U_B, r[6] = V_A, r[7] = V_B;
          r[8] = d, r[9] = u, r[10] = acc ? 1.0 : 0.0;
        }
      }
    }
    rung_out[s] = new_rung;
    fac[s] = f;
  }
}

// Bead i of slot i / n times that slot's factor, rounded once to the system's reals; a slot whose factor is exactly 1 - it
// sat out, or its pair was rejected - is not touched
template <typename R>
__global__ __launch_bounds__(256) void mm_rescale_vel_ens_kernel(int n, int n_rep, const double* __restrict__ fac,
                                                                 typename Real4<R>::type* __restrict__ vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_rep) return;
  const double f = fac[i / n];
  if (f == 1.0) return;
  const R s = R(f);
  auto v = vel[i];
  v.x *= s, v.y *= s, v.z *= s;  // (.w: the inverse mass)
  vel[i] = v;
}

static bool mm_exchange_on(const mythos_martini_sim* sim) { return sim->n_rep >= 2 && sim->xchg.every > 0; }

static int mm_exchange_buffers(mythos_martini_sim* sim) {
  const size_t nr = (size_t)sim->n_rep;  // (fixed at create)
  if (int rc = sim->ladder.d_etrace.grow(nr * kMmTraceCoul)) return rc;
  if (int rc = sim->ladder.d_fac.grow(nr)) return rc;
  if (int rc = sim->xchg.h_d.grow(4 * nr + (nr / 2) * kXchgRec)) return rc;  // in: boxes 3 R, kT R; out: R / 2 records
  return sim->xchg.h_i.grow(2 * nr);                                        // in: rung R; out: rung R
}

// the ladder as it stands -> every slot's kT; the replica table follows at the next mm_upload_reps
static void mm_apply_ladder(mythos_martini_sim* sim) {
  for (int r = 0; r < sim->n_rep; ++r) sim->rep_kT[r] = sim->ladder.kT[(size_t)sim->xchg.of_slot[r]];
}

// The host half of an exchange event of either kind, behind the event's synchronisation: the permutation the kernel left
// in the upper half of h_i and the n_pairs records at h_log, both pinned, become the slots' permutation, the call's log
// and the counts per rung pair.  what: "exchange" or "window-exchange", as the message names the event.
static int mm_pair_exchange_take(mythos_martini_sim* sim, MmPairExchange& x, const double* h_log, int n_pairs, const char* what) {
  const int nr = sim->n_rep;
  const int* out = x.h_i.host() + nr;
  if (!mm_is_permutation(out, nr)) {  // (defensive: the kernel swaps pairs of a permutation)
    set_error(std::string("mythos_martini_langevin_run: the ") + what + " event at step " + std::to_string(sim->step) + " did not return a permutation");
    return MYTHOS_ERR_HIP;
  }
  std::copy(out, out + nr, x.of_slot.begin());
  x.last_log.insert(x.last_log.end(), h_log, h_log + (size_t)n_pairs * kXchgRec);
  for (int q = 0; q < n_pairs; ++q) {
    const int t = (int)h_log[(size_t)q * kXchgRec + 1];
    ++x.attempts[(size_t)t];
    if (h_log[(size_t)q * kXchgRec + 10] != 0.0) ++x.accepts[(size_t)t];
  }
  return MYTHOS_OK;
}

// The exchange event at the closed state of step sim->step, from the energy rows e_rows [n_rep][width] queued on st:
// decision and rescale on the device, ONE synchronisation, then the host takes the ladder and the log from pinned memory,
// gives every slot its kT, queues the replica table and drops the neighbour rows - as after a coupling event, which makes
// what follows the run of an ensemble loaded with this state.
template <typename R>
static int mm_exchange_event(mythos_martini_sim* sim, const double* e_rows, double p, hipStream_t st) {
  using V4 = typename Real4<R>::type;
  MmPairExchange& x = sim->xchg;
  const int nr = sim->n_rep, n = sim->sys->n;
  const int64_t attempt = sim->step / x.every;
  const int n_pairs = mm_xchg_n_pairs(nr, attempt);
  // (the stream is idle behind the last event's synchronisation, or nothing queued on it reads these)
  std::copy(sim->rep_box.begin(), sim->rep_box.end(), x.h_d.host());
  std::copy(sim->ladder.kT.begin(), sim->ladder.kT.end(), x.h_d.host() + 3 * (size_t)nr);
  std::copy(x.of_slot.begin(), x.of_slot.end(), x.h_i.host());
  MmXchgArgs a;
  a.n_rep = nr, a.width = sim->trace_width(), a.p = p, a.seed = x.seed, a.step = sim->step, a.attempt = attempt;
  hipLaunchKernelGGL(mm_exchange_kernel, dim3(1), dim3(256), 0, st, e_rows, (const double*)x.h_d.dev(), (const int*)x.h_i.dev(), a,
                     sim->ladder.d_fac.get(), x.h_i.dev() + nr, x.h_d.dev() + 4 * (size_t)nr);
  hipLaunchKernelGGL(mm_rescale_vel_ens_kernel<R>, dim3((sim->n_all() + 255) / 256), dim3(256), 0, st, n, nr, (const double*)sim->ladder.d_fac.get(),
                     (V4*)sim->vel.get());
  MYTHOS_HIP_TRY(hipGetLastError());
  MYTHOS_HIP_TRY(hipStreamSynchronize(st));
  if (int rc = mm_pair_exchange_take(sim, x, x.h_d.host() + 4 * (size_t)nr, n_pairs, "exchange")) return rc;
  mm_apply_ladder(sim);
  if (int rc = mm_upload_reps(sim, st)) return rc;
  sim->list_valid = false;
  sim->since_build = 0;
  return MYTHOS_OK;
}

// ---- what the C entry points of the two exchanges share; `which` is &mythos_martini_sim::xchg or ::wx
using MmWhich = MmPairExchange mythos_martini_sim::*;
static int mm_pair_get(const mythos_martini_sim* s, MmWhich which, int32_t* of_slot, const char* who) {
  if (!s || !of_slot || s->n_rep < 1) {
    set_error(std::string(who) + ": an ensemble handle and an array of n_rep entries required");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  std::copy((s->*which).of_slot.begin(), (s->*which).of_slot.end(), of_slot);
  return MYTHOS_OK;
}
static int mm_pair_last_rows(const mythos_martini_sim* s, MmWhich which, int32_t* rows, int* n_rows, const char* who) {
  if (!s || s->n_rep < 1 || (!rows && !n_rows)) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const std::vector<int32_t>& last = (s->*which).last_rows;
  if (n_rows) *n_rows = (int)(last.size() / (size_t)s->n_rep);
  if (rows) std::copy(last.begin(), last.end(), rows);
  return MYTHOS_OK;
}
static int mm_pair_last_log(const mythos_martini_sim* s, MmWhich which, double* rec, int* n, const char* who) {
  if (!s || (!rec && !n)) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const std::vector<double>& log = (s->*which).last_log;
  if (n) *n = (int)(log.size() / kXchgRec);
  if (rec) std::copy(log.begin(), log.end(), rec);
  return MYTHOS_OK;
}
static int mm_pair_counts(const mythos_martini_sim* s, MmWhich which, int64_t* attempts, int64_t* accepts, const char* who) {
  if (!s || s->n_rep < 2 || !attempts || !accepts) {
    set_error(std::string(who) + ": an ensemble handle with n_rep >= 2 and two arrays of n_rep - 1 entries required");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  std::copy((s->*which).attempts.begin(), (s->*which).attempts.end(), attempts);
  std::copy((s->*which).accepts.begin(), (s->*which).accepts.end(), accepts);
  return MYTHOS_OK;
}

}  // namespace mythos

extern "C" {

int mythos_martini_exchange_check(int n_rep, int every, const int32_t* rung_of_slot) {
  if (int rc = mm_xchg_check_settings(n_rep, every, "mythos_martini_exchange_check")) return rc;
  return rung_of_slot ? mm_xchg_check_ladder(n_rep, rung_of_slot, "mythos_martini_exchange_check") : MYTHOS_OK;
}

int mythos_martini_langevin_set_exchange(mythos_martini_sim_t* s, int every, uint64_t seed) {
  if (!s) {
    set_error("mythos_martini_langevin_set_exchange: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_xchg_check_settings(s->n_rep, every, "mythos_martini_langevin_set_exchange")) return rc;
  if (every > 0 && s->wx.every > 0)  // (martini_window_exchange_checks.h)
    return mm_wx_check_partners(true, false, "mythos_martini_langevin_set_exchange");
  if (every > 0 && s->rst.installed) {
    set_error("mythos_martini_langevin_set_exchange: replica exchange together with restraints is refused: the restraint energy is not "
              "in the exchange's H (clear the set with mythos_martini_langevin_set_restraints first)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->xchg.every = every;
  s->xchg.seed = seed;
  return MYTHOS_OK;
}

int mythos_martini_langevin_set_ladder(mythos_martini_sim_t* s, const int32_t* rung_of_slot) {
  const char* who = "mythos_martini_langevin_set_ladder";
  if (!s) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_xchg_check_ladder(s->n_rep, rung_of_slot, who)) return rc;
  if (s->resident && s->open) {
    set_error(std::string(who) + ": the resident frame is open - its momenta wait for a closing half kick at the old kT (store or load first)");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());  // (launches that read the replica table)
  std::copy(rung_of_slot, rung_of_slot + s->n_rep, s->xchg.of_slot.begin());
  mm_apply_ladder(s);
  if (int rc = mm_upload_reps(s, nullptr)) return rc;
  MYTHOS_HIP_TRY(hipStreamSynchronize(nullptr));
  return MYTHOS_OK;
}

int mythos_martini_langevin_get_ladder(const mythos_martini_sim_t* s, int32_t* rung_of_slot) {
  return mm_pair_get(s, &mythos_martini_sim::xchg, rung_of_slot, "mythos_martini_langevin_get_ladder");
}

int mythos_martini_langevin_last_ladder(const mythos_martini_sim_t* s, int32_t* rows, int* n_rows) {
  return mm_pair_last_rows(s, &mythos_martini_sim::xchg, rows, n_rows, "mythos_martini_langevin_last_ladder");
}

int mythos_martini_langevin_last_exchanges(const mythos_martini_sim_t* s, double* rec, int* n) {
  return mm_pair_last_log(s, &mythos_martini_sim::xchg, rec, n, "mythos_martini_langevin_last_exchanges");
}

int mythos_martini_langevin_exchange_counts(const mythos_martini_sim_t* s, int64_t* attempts, int64_t* accepts) {
  return mm_pair_counts(s, &mythos_martini_sim::xchg, attempts, accepts, "mythos_martini_langevin_exchange_counts");
}

}  // extern "C"
