// Window exchange between the replicas of a MARTINI ensemble: Hamiltonian replica exchange between the per-replica
// parameter rows of the installed set of restraints, at equal kT; included by martini_md.hip behind martini_restraints.inc.
//
// The rule is stated in include/mythos_hip.h (mythos_martini_langevin_set_window_exchange) and DESIGN.md section 3.5p; what
// needs no device - the decision, the refusals, the row plan of set_windows - is martini_window_exchange_checks.h; pair
// schedule, acceptance and chunking are those of temperature exchange (martini_exchange_checks.h), and so are the record
// (MmPairExchange, martini_md.hip), the host half of an event and the bodies of the C entry points (martini_exchange.inc).
// The loop that cuts an advance at the events is mm_advance_chunked (martini_md.hip).
//
// Slots are the replicas as they lie in memory and keep beads, box, seed and kT.  The window of rung w is the parameter row
// set_restraints was given for replica w: pr_ref[w], fb_param[w], p_param[w].  An accepted exchange SWAPS THE TWO ROWS in
// device memory, so that slot s always runs under row s: mr_kick_kernel and its load chain know nothing of the exchange.
// At equal kT the physical energy cancels: an event needs no energy row, no closing energy launch and no rescale.

namespace mythos {

struct MmWxArgs {
  int n_rep;
  double kT, s;  // the common kT; the step count of the resident frame as the restraints' time base takes it
  uint64_t seed;
  int64_t step, attempt;
};

// One workgroup of 256 per attempted pair (t, t + 1), t = first + 2 blockIdx.x.  Slot A holds window t, slot B window t + 1;
// since rows move with their windows, window t's parameters are row A and window t + 1's row B.  The four cross energies -
// each the sum of the position, flat-bottom, umbrella and constant-force energies of one configuration under one row, in
// the configuration's own box - are strided over the threads and summed in double through the fixed-order LDS tree.
// Thread 0 decides and writes the pair's record and both slots' new window to pinned host memory; behind a barrier, on
// acceptance, all threads swap the two rows.  No other workgroup of the launch reads or writes rows A and B: the pairs of
// one attempt are disjoint.  window_in / window_out / log: pinned host memory; the host fills window_out with window_in
// before the launch, so slots that sit out keep theirs.
template <typename R>
__global__ __launch_bounds__(256) void mr_window_exchange_kernel(const MrView v, const R* __restrict__ pos, int stride,
                                                                 const double* __restrict__ rows, const MmWxArgs a,
                                                                 const int* __restrict__ window_in, double* pr_ref, double* fb_param,
                                                                 double* p_param, int* __restrict__ window_out, double* __restrict__ log) {
  __shared__ double red[4][256];
  __shared__ int s_slot[2];
  __shared__ int s_acc;
  const int first = mm_xchg_first_rung(a.attempt);
  const int t = first + 2 * (int)blockIdx.x;
  if (t + 1 >= a.n_rep) return;  // (the grid is mm_xchg_n_pairs: never)
  if (threadIdx.x < 2) s_slot[threadIdx.x] = -1;
  __syncthreads();
  for (int q = threadIdx.x; q < a.n_rep; q += 256) {
    const int w = window_in[q];
    if (w == t) s_slot[0] = q;
    if (w == t + 1) s_slot[1] = q;
  }
  __syncthreads();
  const int slot[2] = {s_slot[0], s_slot[1]};
  if (slot[0] < 0 || slot[1] < 0) return;  // (a permutation: never; uniform over the workgroup)
  // acc[2 c + w]: configuration of slot[c] under the row of slot[w] - E_t(x_A), E_t+1(x_A), E_t(x_B), E_t+1(x_B)
  double acc[4] = {0, 0, 0, 0};
  const double time = a.s * v.dt;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const R* x0 = pos + (size_t)slot[c] * v.n * stride;
    const double* rw = rows + (size_t)slot[c] * v.n_groups * kMrRow;
    for (int k = threadIdx.x; k < v.n_posres; k += 256) {
      const size_t i = v.pr_index[k];
      const double x[3] = {double(x0[i * stride]), double(x0[i * stride + 1]), double(x0[i * stride + 2])};
      double F[3] = {0, 0, 0};
      acc[2 * c] += mr_posres_term(v, k, slot[0], x, F);
      acc[2 * c + 1] += mr_posres_term(v, k, slot[1], x, F);
    }
    for (int k = threadIdx.x; k < v.n_flat; k += 256) {
      const size_t i = v.fb_index[k];
      const double x[3] = {double(x0[i * stride]), double(x0[i * stride + 1]), double(x0[i * stride + 2])};
      double F[3] = {0, 0, 0};
      acc[2 * c] += mr_flat_term(v, k, slot[0], x, F);
      acc[2 * c + 1] += mr_flat_term(v, k, slot[1], x, F);
    }
    for (int p = threadIdx.x; p < v.n_pull; p += 256) {
      acc[2 * c] += mr_pull_eval(v, p, slot[c], slot[0], rw, time).u;
      acc[2 * c + 1] += mr_pull_eval(v, p, slot[c], slot[1], rw, time).u;
    }
  }
  mr_block_sum4(red, acc);  // (ends on a barrier: every read of the two rows is behind us)
  if (threadIdx.x == 0) {
    const double d = mm_wx_delta(a.kT, acc[0], acc[1], acc[2], acc[3]);
    uint32_t c[4] = {(uint32_t)t, uint32_t((uint64_t)a.step), uint32_t((uint64_t)a.step >> 32), kWxStream};
    philox4x32(c, uint32_t(a.seed), uint32_t(a.seed >> 32));
    const double u = (double(c[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
    const bool ok = mm_xchg_accept(d, u);
    double* __restrict__ r = log + (size_t)blockIdx.x * kWxRec;
    r[0] = double(a.step), r[1] = double(t), r[2] = double(slot[0]), r[3] = double(slot[1]);
    r[4] = acc[0], r[5] = acc[1], r[6] = acc[2], r[7] = acc[3], r[8] = d, r[9] = u, r[10] = ok ? 1.0 : 0.0;
    window_out[slot[0]] = ok ? t + 1 : t;
    window_out[slot[1]] = ok ? t : t + 1;
    s_acc = ok ? 1 : 0;
  }
  __syncthreads();
  if (s_acc == 0) return;
  const size_t n_pr = (size_t)v.n_posres * 3, n_fb = (size_t)v.n_flat * kMrFlatParams, n_pp = (size_t)v.n_pull * kMrPullParams;
  for (size_t k = threadIdx.x; k < n_pr; k += 256) {
    const double x = pr_ref[slot[0] * n_pr + k], y = pr_ref[slot[1] * n_pr + k];
    pr_ref[slot[0] * n_pr + k] = y, pr_ref[slot[1] * n_pr + k] = x;
  }
  for (size_t k = threadIdx.x; k < n_fb; k += 256) {
    const double x = fb_param[slot[0] * n_fb + k], y = fb_param[slot[1] * n_fb + k];
    fb_param[slot[0] * n_fb + k] = y, fb_param[slot[1] * n_fb + k] = x;
  }
  for (size_t k = threadIdx.x; k < n_pp; k += 256) {
    const double x = p_param[slot[0] * n_pp + k], y = p_param[slot[1] * n_pp + k];
    p_param[slot[0] * n_pp + k] = y, p_param[slot[1] * n_pp + k] = x;
  }
}

static bool mm_window_exchange_on(const mythos_martini_sim* sim) { return sim->n_rep >= 2 && sim->wx.every > 0; }

static int mm_wx_buffers(mythos_martini_sim* sim) {
  const size_t nr = (size_t)sim->n_rep;  // (fixed at create)
  if (int rc = sim->wx.h_d.grow((nr / 2) * kWxRec)) return rc;  // out: R / 2 records
  return sim->wx.h_i.grow(2 * nr);                              // in: window R; out: window R
}

// The window-exchange event at the closed state of step sim->step: the centres of mass of the resident frame, the decision
// kernel, ONE synchronisation; the host then takes the assignment and the log from pinned memory and drops the neighbour
// rows, as the temperature event does - what follows is the run of an ensemble loaded with this state and these rows.
template <typename R>
static int mm_window_exchange_event(mythos_martini_sim* sim, hipStream_t st) {
  MmPairExchange& w = sim->wx;
  MmRestraints& q = sim->rst;
  const MrView& v = q.view;
  const int nr = sim->n_rep;
  const int64_t attempt = sim->step / w.every;
  const int n_pairs = mm_xchg_n_pairs(nr, attempt);
  if (n_pairs > 0) {
    // (the stream is idle behind the last event's synchronisation, or nothing queued on it reads these)
    std::copy(w.of_slot.begin(), w.of_slot.end(), w.h_i.host());
    std::copy(w.of_slot.begin(), w.of_slot.end(), w.h_i.host() + nr);
    const R* frame = (const R*)sim->frame[sim->cur].get();
    if (v.n_pull > 0) hipLaunchKernelGGL(mr_com_kernel<R>, dim3(v.n_rep * v.n_groups), dim3(256), 0, st, v, frame, 4, q.d_rows.get());
    MmWxArgs a;
    a.n_rep = nr, a.kT = sim->rep_kT[0], a.s = double(sim->step), a.seed = w.seed, a.step = sim->step, a.attempt = attempt;
    hipLaunchKernelGGL(mr_window_exchange_kernel<R>, dim3(n_pairs), dim3(256), 0, st, v, frame, 4, (const double*)q.d_rows.get(), a,
                       (const int*)w.h_i.dev(), q.d_pr_ref.get(), q.d_fb_param.get(), q.d_p_param.get(), w.h_i.dev() + nr, w.h_d.dev());
    MYTHOS_HIP_TRY(hipGetLastError());
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
    if (int rc = mm_pair_exchange_take(sim, w, w.h_d.host(), n_pairs, "window-exchange")) return rc;
  }
  sim->list_valid = false;
  sim->since_build = 0;
  return MYTHOS_OK;
}

// rows of the installed set from the current assignment to `want` (host round trip: a rare call)
static int mm_wx_move_rows(mythos_martini_sim* sim, const int32_t* want) {
  MmRestraints& q = sim->rst;
  const MrView& v = q.view;
  const int nr = sim->n_rep;
  const std::vector<int32_t> plan = mm_wx_row_plan(sim->wx.of_slot.data(), want, nr);
  struct Rows {
    double* d;
    size_t len;
  } all[3] = {{q.d_pr_ref.get(), (size_t)v.n_posres * 3}, {q.d_fb_param.get(), (size_t)v.n_flat * kMrFlatParams},
              {q.d_p_param.get(), (size_t)v.n_pull * kMrPullParams}};
  for (const Rows& r : all) {
    if (r.len == 0) continue;
    std::vector<double> h((size_t)nr * r.len);
    MYTHOS_HIP_TRY(hipMemcpy(h.data(), r.d, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    mm_wx_permute_rows(h, r.len, plan);
    MYTHOS_HIP_TRY(hipMemcpy(r.d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return MYTHOS_OK;
}

}  // namespace mythos

extern "C" {

int mythos_martini_window_exchange_check(int n_rep, int every, const double* kT, int temperature_exchange, int barostat, int n_pull,
                                         const double* p_param, const int32_t* window_of_slot) {
  return mm_wx_check(n_rep, every, kT, temperature_exchange != 0, barostat != 0, n_pull, p_param, window_of_slot,
                     "mythos_martini_window_exchange_check");
}

int mythos_martini_langevin_set_window_exchange(mythos_martini_sim_t* s, int every, uint64_t seed) {
  const char* who = "mythos_martini_langevin_set_window_exchange";
  if (!s) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_wx_check_settings(s->n_rep, every, who)) return rc;
  if (every > 0) {
    if (int rc = mm_wx_check_kT(s->n_rep, s->ladder.kT.data(), who)) return rc;
    if (int rc = mm_wx_check_partners(mm_exchange_on(s), s->baro.kind != 0, who)) return rc;
    if (s->rst.installed && s->rst.view.n_pull > 0) {
      // (the set is on the device; the rows may have moved, which changes nothing in what is compared)
      std::vector<double> h((size_t)s->n_rep * s->rst.view.n_pull * kMrPullParams);
      MYTHOS_HIP_TRY(hipSetDevice(s->device));
      MYTHOS_HIP_TRY(hipDeviceSynchronize());
      MYTHOS_HIP_TRY(hipMemcpy(h.data(), s->rst.d_p_param.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost));
      if (int rc = mm_wx_check_set(s->n_rep, s->rst.view.n_pull, h.data(), who)) return rc;
    }
  }
  s->wx.every = every;
  s->wx.seed = seed;
  return MYTHOS_OK;
}

int mythos_martini_langevin_set_windows(mythos_martini_sim_t* s, const int32_t* window_of_slot) {
  const char* who = "mythos_martini_langevin_set_windows";
  if (!s) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_wx_check_windows(s->n_rep, window_of_slot, who)) return rc;
  if (!s->rst.installed) {
    set_error(std::string(who) + ": no set of restraints is installed: there are no rows to assign");
    return MYTHOS_ERR_NOT_READY;
  }
  if (s->resident && s->open) {
    set_error(std::string(who) + ": the resident frame is open - its velocities wait for a closing half kick under the old windows (store or load first)");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());  // (launches that read the rows)
  if (int rc = mm_wx_move_rows(s, window_of_slot)) return rc;
  std::copy(window_of_slot, window_of_slot + s->n_rep, s->wx.of_slot.begin());
  return MYTHOS_OK;
}

int mythos_martini_langevin_get_windows(const mythos_martini_sim_t* s, int32_t* window_of_slot) {
  return mm_pair_get(s, &mythos_martini_sim::wx, window_of_slot, "mythos_martini_langevin_get_windows");
}

int mythos_martini_langevin_last_windows(const mythos_martini_sim_t* s, int32_t* rows, int* n_rows) {
  return mm_pair_last_rows(s, &mythos_martini_sim::wx, rows, n_rows, "mythos_martini_langevin_last_windows");
}

int mythos_martini_langevin_last_window_exchanges(const mythos_martini_sim_t* s, double* rec, int* n) {
  return mm_pair_last_log(s, &mythos_martini_sim::wx, rec, n, "mythos_martini_langevin_last_window_exchanges");
}

int mythos_martini_langevin_window_exchange_counts(const mythos_martini_sim_t* s, int64_t* attempts, int64_t* accepts) {
  return mm_pair_counts(s, &mythos_martini_sim::wx, attempts, accepts, "mythos_martini_langevin_window_exchange_counts");
}

}  // extern "C"
