// Host side of the MARTINI integrator's external forces (included by martini_md.hip; kernels: martini_restraints.h; the
// checks and the lowering to per-bead term lists, which need no device: martini_restraint_checks.h).  Here: the upload of a
// set, the evaluation path and the stored-frames launch.  The kick itself is queued by mm_advance_typed's launches, so it runs
// the same in the plain call and in every chunk of mm_advance_chunked (martini_md.hip).

namespace mythos {

// the set is lowered for the boxes it was given: a load into other boxes would take minimum images in the wrong cell
static int mr_check_load_box(const mythos_martini_sim* sim, const double* box) {
  const MmRestraints& q = sim->rst;
  if (!q.installed || !q.uses_box || !box) return MYTHOS_OK;
  for (int k = 0; k < 3 * sim->copies(); ++k)
    if (box[k] != q.h_boxes[k]) {
      set_error("mythos_martini_langevin_load: the restraints were installed for another box (replica " + std::to_string(k / 3) +
                "): install them again with the boxes of this state");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
  return MYTHOS_OK;
}

static MrArrays mr_arrays(int n_posres, const int32_t* pr_index, const double* pr_k, const double* pr_ref, int n_flat, const int32_t* fb_index,
                          const int32_t* fb_flags, const double* fb_param, int n_groups, const int32_t* g_first, const int32_t* g_member,
                          const int32_t* g_pbc_ref, int n_pull, const int32_t* p_flags, const int32_t* p_groups, const double* p_param,
                          const double* boxes) {
  MrArrays a;
  a.n_posres = n_posres, a.pr_index = pr_index, a.pr_k = pr_k, a.pr_ref = pr_ref;
  a.n_flat = n_flat, a.fb_index = fb_index, a.fb_flags = fb_flags, a.fb_param = fb_param;
  a.n_groups = n_groups, a.g_first = g_first, a.g_member = g_member, a.g_pbc_ref = g_pbc_ref;
  a.n_pull = n_pull, a.p_flags = p_flags, a.p_groups = p_groups, a.p_param = p_param;
  a.boxes = boxes;
  return a;
}

static int mr_install(mythos_martini_sim* sim, const MrArrays& a) {
  MmRestraints& q = sim->rst;
  const int n = sim->sys->n, nr = sim->copies();
  q.installed = false;
  q.stamp_stale = true;
  q.view = MrView();
  if (a.empty()) return MYTHOS_OK;
  const MrEntries e = mr_entries(n, a);
  const int n_members = a.n_groups > 0 ? a.g_first[a.n_groups] : 0;
  std::vector<double> boxes((size_t)3 * nr, 1.0);
  if (a.boxes) boxes.assign(a.boxes, a.boxes + 3 * (size_t)nr);
  const int n_entries = (int)e.index.size();
  const size_t blocks = ((size_t)nr * n_entries + 255) / 256;
  if (q.d_pr_index.upload(a.pr_index, a.n_posres) || q.d_pr_k.upload(a.pr_k, 3 * (size_t)a.n_posres) ||
      q.d_pr_ref.upload(a.pr_ref, 3 * (size_t)nr * a.n_posres) || q.d_fb_index.upload(a.fb_index, a.n_flat) ||
      q.d_fb_flags.upload(a.fb_flags, a.n_flat) || q.d_fb_param.upload(a.fb_param, (size_t)nr * a.n_flat * kMrFlatParams) ||
      q.d_g_first.upload(a.g_first, a.n_groups > 0 ? a.n_groups + 1 : 0) || q.d_g_member.upload(a.g_member, n_members) ||
      q.d_g_pbc_ref.upload(a.g_pbc_ref, a.n_groups) || q.d_p_flags.upload(a.p_flags, a.n_pull) ||
      q.d_p_groups.upload(a.p_groups, 2 * (size_t)a.n_pull) || q.d_p_param.upload(a.p_param, (size_t)nr * a.n_pull * kMrPullParams) ||
      q.d_boxes.upload(boxes) || q.d_mass.upload(sim->h_mass) || q.d_e_index.upload(e.index) || q.d_e_first.upload(e.first) ||
      q.d_e_term.upload(e.term) || q.d_rows.alloc((size_t)nr * a.n_groups * kMrRow) || q.d_stamp.alloc(blocks) ||
      hipMemset(q.d_rows.get(), 0, q.d_rows.capacity() * sizeof(double)) != hipSuccess) {
    set_error("mythos_martini_langevin_set_restraints: device allocation failed");
    return MYTHOS_ERR_HIP;
  }
  MrView& v = q.view;
  v.n = n, v.n_rep = nr;
  v.n_posres = a.n_posres, v.n_flat = a.n_flat, v.n_groups = a.n_groups, v.n_pull = a.n_pull, v.n_entries = n_entries;
  v.pr_index = q.d_pr_index.get(), v.pr_k = q.d_pr_k.get(), v.pr_ref = q.d_pr_ref.get();
  v.fb_index = q.d_fb_index.get(), v.fb_flags = q.d_fb_flags.get(), v.fb_param = q.d_fb_param.get();
  v.g_first = q.d_g_first.get(), v.g_member = q.d_g_member.get(), v.g_pbc_ref = q.d_g_pbc_ref.get();
  v.p_flags = q.d_p_flags.get(), v.p_groups = q.d_p_groups.get(), v.p_param = q.d_p_param.get();
  v.boxes = q.d_boxes.get(), v.mass = q.d_mass.get();
  v.e_index = q.d_e_index.get(), v.e_first = q.d_e_first.get(), v.e_term = q.d_e_term.get();
  v.dt = sim->dt;
  q.h_boxes = boxes;
  q.uses_box = a.boxes != nullptr;
  q.installed = true;
  return MYTHOS_OK;
}

// forces (copies n, 3), energies [copies][kMrEnergies] and xi [copies][n_pull] at pos (copies n, 3) and step count `step`:
// the kick's kernels with factor 1 on a scratch array of zero velocities, then the energy sum
template <typename R>
static int mr_eval_typed(mythos_martini_sim* sim, const R* pos, double step, R* force, double* energies, double* xi, hipStream_t st) {
  using V4 = typename Real4<R>::type;
  MmRestraints& q = sim->rst;
  const int n_all = sim->n_all(), nr = sim->copies();
  if (!q.installed) {  // no set: no field
    if (force) MYTHOS_HIP_TRY(hipMemsetAsync(force, 0, (size_t)n_all * 3 * sizeof(R), st));
    if (energies) MYTHOS_HIP_TRY(hipMemsetAsync(energies, 0, (size_t)nr * kMrEnergies * sizeof(double), st));
    return MYTHOS_OK;
  }
  const MrView& v = q.view;
  if (int rc = q.d_eval_vel.grow((size_t)n_all * sizeof(V4))) return rc;
  if (int rc = q.d_eval_rows.grow((size_t)nr * v.n_groups * kMrRow)) return rc;
  if (int rc = q.d_eval_stamp.grow((size_t)std::max(1, q.kick_blocks()))) return rc;
  if (int rc = q.d_eval_flags.grow((size_t)MdRun::kCtlWords)) return rc;
  MYTHOS_HIP_TRY(hipMemsetAsync(q.d_eval_vel.get(), 0, (size_t)n_all * sizeof(V4), st));
  MYTHOS_HIP_TRY(hipMemsetAsync(q.d_eval_stamp.get(), 0, (size_t)std::max(1, q.kick_blocks()) * sizeof(unsigned long long), st));
  MYTHOS_HIP_TRY(hipMemsetAsync(q.d_eval_flags.get(), 0, MdRun::kCtlWords * sizeof(int), st));
  V4* vel = (V4*)q.d_eval_vel.get();
  mr_launch_kick<R>(v, pos, 3, q.d_eval_rows.get(), -1.0, step, vel, q.d_eval_flags.get(), nullptr, 0, 1ull, q.d_eval_stamp.get(), st);
  if (force) hipLaunchKernelGGL((mr_unpack_force_kernel<R, V4>), dim3((n_all + 255) / 256), dim3(256), 0, st, n_all, (const V4*)vel, force);
  if (energies)
    hipLaunchKernelGGL(mr_energy_kernel<R>, dim3(nr), dim3(256), 0, st, v, pos, 3, (const double*)q.d_eval_rows.get(), step, energies, xi);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

template <typename R>
static int mr_pull_values_typed(mythos_martini_sim* sim, const R* pos, int n_frames, double* out, hipStream_t st) {
  MmRestraints& q = sim->rst;
  const MrView& v = q.view;
  const long long blocks = (long long)n_frames * v.n_rep * v.n_groups;
  const long long items = (long long)n_frames * v.n_rep * v.n_pull;
  if (items == 0) return MYTHOS_OK;
  if (blocks > INT_MAX || items > INT_MAX) {
    set_error("mythos_martini_langevin_pull_values: too many frames for one launch");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = q.d_eval_rows.grow((size_t)blocks * kMrRow)) return rc;
  hipLaunchKernelGGL(mr_com_kernel<R>, dim3((unsigned)blocks), dim3(256), 0, st, v, pos, 3, q.d_eval_rows.get());
  hipLaunchKernelGGL(mr_pull_values_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, v, n_frames, (const double*)q.d_eval_rows.get(), out);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

}  // namespace mythos

extern "C" {

int mythos_martini_restraints_check(int n, int n_rep, int n_posres, const int32_t* pr_index, const double* pr_k, const double* pr_ref,
                                    int n_flat, const int32_t* fb_index, const int32_t* fb_flags, const double* fb_param, int n_groups,
                                    const int32_t* g_first, const int32_t* g_member, const int32_t* g_pbc_ref, int n_pull,
                                    const int32_t* p_flags, const int32_t* p_groups, const double* p_param, const double* boxes,
                                    int barostat, int exchange) {
  return mr_check("mythos_martini_restraints_check", n, n_rep,
                  mr_arrays(n_posres, pr_index, pr_k, pr_ref, n_flat, fb_index, fb_flags, fb_param, n_groups, g_first, g_member, g_pbc_ref,
                            n_pull, p_flags, p_groups, p_param, boxes),
                  barostat != 0, exchange != 0);
}

int mythos_martini_langevin_set_restraints(mythos_martini_sim_t* s, int n_posres, const int32_t* pr_index, const double* pr_k,
                                           const double* pr_ref, int n_flat, const int32_t* fb_index, const int32_t* fb_flags,
                                           const double* fb_param, int n_groups, const int32_t* g_first, const int32_t* g_member,
                                           const int32_t* g_pbc_ref, int n_pull, const int32_t* p_flags, const int32_t* p_groups,
                                           const double* p_param, const double* boxes) {
  const char* who = "mythos_martini_langevin_set_restraints";
  if (!s) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const MrArrays a = mr_arrays(n_posres, pr_index, pr_k, pr_ref, n_flat, fb_index, fb_flags, fb_param, n_groups, g_first, g_member,
                               g_pbc_ref, n_pull, p_flags, p_groups, p_param, boxes);
  if (int rc = mr_check(who, s->sys->n, s->copies(), a, s->baro.kind != 0, mm_exchange_on(s))) return rc;
  if (s->wx.every > 0)  // window exchange: vec and origin are the coordinate's, not a window's (martini_window_exchange_checks.h)
    if (int rc = mm_wx_check_set(s->n_rep, a.n_pull, a.p_param, who)) return rc;
  if (s->resident && s->open) {
    set_error(std::string(who) + ": the resident frame is open - its velocities wait for a closing half kick by the old field (store or load first)");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());  // (launches that read the arrays replaced below)
  // the rows are the caller's again: window w lies in slot w, the window-exchange counts start over
  s->wx.identity();
  return mr_install(s, a);
}

int mythos_martini_langevin_n_pull(const mythos_martini_sim_t* s) { return s && s->rst.installed ? s->rst.view.n_pull : 0; }

int mythos_martini_langevin_eval_external(mythos_martini_sim_t* s, const void* pos, double step, void* force, double* energies, double* xi,
                                          mythos_stream_t stream) {
  if (!s || !pos || !std::isfinite(step)) {
    set_error("mythos_martini_langevin_eval_external: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return s->sys->dtype == MYTHOS_F32 ? mr_eval_typed<float>(s, (const float*)pos, step, (float*)force, energies, xi, (hipStream_t)stream)
                                     : mr_eval_typed<double>(s, (const double*)pos, step, (double*)force, energies, xi, (hipStream_t)stream);
}

int mythos_martini_langevin_pull_values(mythos_martini_sim_t* s, const void* pos, int n_frames, double* out, mythos_stream_t stream) {
  if (!s || n_frames < 0 || (n_frames > 0 && (!pos || !out))) {
    set_error("mythos_martini_langevin_pull_values: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->rst.installed || s->rst.view.n_pull == 0) return MYTHOS_OK;  // no coordinate: nothing to write
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return s->sys->dtype == MYTHOS_F32 ? mr_pull_values_typed<float>(s, (const float*)pos, n_frames, out, (hipStream_t)stream)
                                     : mr_pull_values_typed<double>(s, (const double*)pos, n_frames, out, (hipStream_t)stream);
}

}  // extern "C"
