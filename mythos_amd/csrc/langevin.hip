// Langevin integrator, translation unit 1 of 2: the fp32 instantiations of langevin_core.inc and the C entry points
// (mythos_langevin_*).  The fp64 instantiations are in langevin_f64.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "langevin_core.inc"
#include "point_force_checks.h"

namespace {
// the entry points of the system's precision: this unit's own, or langevin_f64.hip's
MdEntries md_entries_of(const mythos_sim* s) { return s->sys->dtype == MYTHOS_F32 ? md_entries<float>() : md_entries_f64(); }

// the point terms' half of a view (mythos_langevin_set_point_forces), everything of the restraints' half unset
ExtFieldView ext_point_part(const ExtFieldView& v) {
  ExtFieldView o;
  o.n_points = v.n_points;
  o.pt_kind = v.pt_kind, o.pt_particle = v.pt_particle, o.pt_ref = v.pt_ref, o.pt_flags = v.pt_flags, o.pt_param = v.pt_param;
  for (int a = 0; a < 3; ++a) o.box[a] = v.box[a];
  return o;
}

// The entries of s->rst - the nucleotides a restraint or a point term names, ascending - from what the two sets
// contribute (the host copies in mythos_sim), with each entry's range of restraint terms and of point terms; one stamp
// word per workgroup of the kick.  Both setters end here, after the device has gone idle.  With no point terms the
// entries are the restraints' own, as they were uploaded before there were any.
int ext_entries_merge(mythos_sim* s) {
  const std::vector<int>&ri = s->h_rst_index, &rf = s->h_rst_first, &rt = s->h_rst_term, &pp = s->h_pt_particle;
  ExtFieldView& v = s->rst;
  v.n_entries = v.n_points = 0;  // (nothing half replaced counts)
  v.e_index = v.e_first = v.e_term = v.pt_first = nullptr;
  std::vector<int> e_index, e_first{0}, e_term, pt_first{0};
  size_t a = 0, b = 0;
  while (a < ri.size() || b < pp.size()) {
    const int i = (b >= pp.size() || (a < ri.size() && ri[a] <= pp[b])) ? ri[a] : pp[b];
    e_index.push_back(i);
    if (a < ri.size() && ri[a] == i) {
      e_term.insert(e_term.end(), rt.begin() + rf[a], rt.begin() + rf[a + 1]);
      ++a;
    }
    e_first.push_back((int)e_term.size());
    while (b < pp.size() && pp[b] == i) ++b;
    pt_first.push_back((int)b);
  }
  if (e_index.empty()) return MYTHOS_OK;
  int rc = s->d_rst_e_index.upload(e_index);
  if (!rc) rc = s->d_rst_e_first.upload(e_first);
  if (!rc) rc = s->d_rst_e_term.upload(e_term);
  if (!rc && !pp.empty()) rc = s->d_pt_first.upload(pt_first);
  if (!rc) rc = s->d_rst_stamp.alloc((e_index.size() + 255) / 256);
  if (rc) return rc;
  v.e_index = s->d_rst_e_index.get(), v.e_first = s->d_rst_e_first.get(), v.e_term = s->d_rst_e_term.get();
  if (!pp.empty()) v.pt_first = s->d_pt_first.get();
  v.n_points = (int)pp.size();
  v.n_entries = (int)e_index.size();
  return MYTHOS_OK;
}
}  // namespace

extern "C" {

mythos_sim_t* mythos_langevin_create(mythos_system_t* sys, double dt, double kT, double gamma_t, double gamma_r,
                                     double mass, const double* inertia, uint64_t seed) {
  if (!sys || !(dt > 0) || !(kT >= 0) || gamma_t < 0 || gamma_r < 0 || !(mass > 0)) {
    set_error("mythos_langevin_create: invalid argument");
    return nullptr;
  }
  if (select_device(sys->device, "mythos_langevin_create")) return nullptr;
  auto s = std::make_unique<mythos_sim>();
  s->sys = sys;
  s->device = sys->device;
  s->dt = dt;
  s->kT = kT;
  s->gamma_t = gamma_t;
  s->gamma_r = gamma_r;
  s->mass = mass;
  for (int k = 0; k < 3; ++k) s->inertia[k] = inertia ? inertia[k] : 1.0;
  s->seed = seed;
  const size_t v4 = (sys->dtype == MYTHOS_F32 ? sizeof(float4) : sizeof(double4)) * (size_t)sys->n;
  bool ok = md_run_create(*s);
  for (int k = 0; k < 2; ++k)
    for (int a = 0; a < mythos_sim::kFrameArrays; ++a) ok = ok && s->frame[k][a].alloc(v4) == 0;
  // (d_epart: one row of partials per workgroup of the narrowest launch, 16 lanes per nucleotide)
  ok = ok && s->keep_hi.alloc(v4) == 0 && s->keep_lo.alloc(v4) == 0 &&
       s->d_epart.alloc((size_t)((sys->n + 15) / 16) * kTraceWidth) == 0 && sys->reserve_refs() == 0;
  if (!ok) {
    set_error("mythos_langevin_create: device allocation failed");
    return nullptr;
  }
  return s.release();
}

void mythos_langevin_destroy(mythos_sim_t* s) { delete s; }

int mythos_langevin_set_neighbor_policy(mythos_sim_t* s, double r_cut, double skin, int every) {
  if (!s || (every > 0 && (!(r_cut > 0) || !(skin > 0)))) {
    set_error("mythos_langevin_set_neighbor_policy: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->r_cut = r_cut;
  s->skin = skin;
  s->rebuild_every = every;
  s->list_fitted = false;  // another list range: size rows and buckets again at the next run
  s->list_valid = false;
  s->sys->cand_unfit = false;  // (and find out again whether its candidate rows fit)
  return MYTHOS_OK;
}

int mythos_langevin_init_momenta(mythos_sim_t* s, void* p_lin, void* p_ang, mythos_stream_t stream) {
  if (!s || !p_lin || !p_ang) {
    set_error("mythos_langevin_init_momenta: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return md_entries_of(s).init_momenta(s, p_lin, p_ang, (hipStream_t)stream);
}

namespace {

// what a state needs before it can be packed into frames: the site geometry (parameters) and, for oxNA, the types that
// choose between the two geometries
int md_ready_state(mythos_sim_t* s, const char* who) {
  mythos_system* sys = s->sys;
  if (!sys->params_set) {
    set_error(std::string(who) + ": parameters must be set first");
    return MYTHOS_ERR_NOT_READY;
  }
  if (sys->model == 4 && !sys->types_set) {
    set_error(std::string(who) + ": an oxNA system needs its nucleotide types (mythos_oxdna_set_nucleotide_types)");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(sys->device));
  return MYTHOS_OK;
}

// what every entry that launches step kernels checks first
int md_ready(mythos_sim_t* s, const char* who) {
  mythos_system* sys = s->sys;
  if (int rc = md_ready_state(s, who)) return rc;
  if (!sys->nbrs_set && s->rebuild_every <= 0) {
    set_error(std::string(who) + ": parameters and neighbours (or a neighbour policy) must be set first");
    return MYTHOS_ERR_NOT_READY;
  }
  if (s->rebuild_every > 0 && sys->list.stride == 0)
    if (int rc = rows_reserve(sys->list, sys->n, 64)) return rc;
  if (s->list_epoch != sys->list_epoch) {  // parameters or rows were replaced behind the integrator's back
    s->list_valid = false;
    s->list_epoch = sys->list_epoch;
  }
  return MYTHOS_OK;
}

// oxNA systems step through the fused kernel's MODEL 4 instantiation; mythos_langevin_set_option(MYTHOS_LANGEVIN_UNFUSED)
// selects the two-launch path (the energy kernel's forces + unfused_integrate_kernel) instead - a second implementation
// the tests hold the first to.  The choice is made when a state is loaded and holds while that state is resident.

int md_load(mythos_sim_t* s, void* c, void* q, void* p, void* l, hipStream_t st) {
  s->unfused.active = s->unfused.want && s->sys->model == 4;
  s->umb.primed = false;  // (another state: the snapshot and the weights held are not its)
  s->umb.frame_loaded = true;
  return md_entries_of(s).load(s, c, q, p, l, st);
}

int md_advance(mythos_sim_t* s, int n_steps, int save_every, bool close, void* tc, void* tq, double* e_trace, hipStream_t st) {
  if (s->ext_count > 0 && s->unfused.active) {
    set_error("mythos_langevin_run / advance: external forces are not applied on the unfused oxNA path "
              "(MYTHOS_LANGEVIN_UNFUSED); clear them or step through the fused kernel");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (s->rst.n_entries > 0 && s->unfused.active) {
    set_error("mythos_langevin_run / advance: restraints and point forces are not applied on the unfused oxNA path "
              "(MYTHOS_LANGEVIN_UNFUSED); clear them or step through the fused kernel");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  // quaternion rows are written as one 4-vector per nucleotide
  const size_t q_align = s->sys->dtype == MYTHOS_F32 ? sizeof(float4) : sizeof(double4);
  if (save_every > 0 && tq && (reinterpret_cast<uintptr_t>(tq) % q_align) != 0) {
    set_error("mythos_langevin_run / advance: traj_quat must be aligned to 4 elements (" + std::to_string(q_align) + " bytes)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->umb.frame_loaded = false;
  return md_entries_of(s).advance(s, n_steps, save_every, close, tc, tq, e_trace, st);
}

int md_store(mythos_sim_t* s, void* c, void* q, void* p, void* l, hipStream_t st) {
  return md_entries_of(s).store(s, c, q, p, l, st);
}

}  // namespace

int mythos_langevin_run(mythos_sim_t* s, void* center, void* quat, void* p_lin, void* p_ang, int n_steps,
                        int save_every, void* traj_center, void* traj_quat, double* e_trace,
                        mythos_stream_t stream) {
  if (!s || !center || !quat || !p_lin || !p_ang || n_steps < 0 || save_every < 0) {
    set_error("mythos_langevin_run: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = md_ready(s, "mythos_langevin_run")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = md_load(s, center, quat, p_lin, p_ang, st)) return rc;
  const int rc = md_advance(s, n_steps, save_every, true, traj_center, traj_quat, e_trace, st);
  // the state of the last valid step goes back to the caller whatever the run reported
  if (int rs = md_store(s, center, quat, p_lin, p_ang, st)) return rc ? rc : rs;
  return rc;
}

int mythos_langevin_load(mythos_sim_t* s, const void* center, const void* quat, const void* p_lin, const void* p_ang,
                         mythos_stream_t stream) {
  if (!s || !center || !quat || !p_lin || !p_ang) {
    set_error("mythos_langevin_load: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = md_ready_state(s, "mythos_langevin_load")) return rc;
  return md_load(s, (void*)center, (void*)quat, (void*)p_lin, (void*)p_ang, (hipStream_t)stream);
}

int mythos_langevin_advance(mythos_sim_t* s, int n_steps, int save_every, void* traj_center, void* traj_quat,
                            double* e_trace, mythos_stream_t stream) {
  if (!s || n_steps < 0 || save_every < 0) {
    set_error("mythos_langevin_advance: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->resident) {
    set_error("mythos_langevin_advance: no resident state (call mythos_langevin_load first; a run that ended in a numeric "
              "error drops its state)");
    return MYTHOS_ERR_NOT_READY;
  }
  if (int rc = md_ready(s, "mythos_langevin_advance")) return rc;
  if (n_steps > 0) s->umb.primed = false;  // (unbiased steps: the snapshot and the weights held are no longer this state's)
  return md_advance(s, n_steps, save_every, false, traj_center, traj_quat, e_trace, (hipStream_t)stream);
}

int mythos_langevin_store(mythos_sim_t* s, void* center, void* quat, void* p_lin, void* p_ang, mythos_stream_t stream) {
  if (!s || !center || !quat || !p_lin || !p_ang) {
    set_error("mythos_langevin_store: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->resident) {
    set_error("mythos_langevin_store: no resident state");
    return MYTHOS_ERR_NOT_READY;
  }
  if (s->open) {  // one more launch closes the frame: what a launch needs has to be there (it was, for the advance before)
    if (int rc = md_ready(s, "mythos_langevin_store")) return rc;
  } else {  // a copy: load; store round-trips a state whether or not neighbours were ever set
    MYTHOS_HIP_TRY(hipSetDevice(s->device));
  }
  return md_store(s, center, quat, p_lin, p_ang, (hipStream_t)stream);
}

int64_t mythos_langevin_get_step(const mythos_sim_t* s) { return md_get_step(s); }

int mythos_langevin_set_step(mythos_sim_t* s, int64_t step) {
  if (!s || step < 0) {
    set_error("mythos_langevin_set_step: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->step = step;
  s->ext_stamp_stale = s->rst_stamp_stale = true;  // (the stamp of the last external kick names a step index)
  return MYTHOS_OK;
}

int mythos_langevin_set_external_forces(mythos_sim_t* s, int count, const int32_t* index, const double* force) {
  const char* who = "mythos_langevin_set_external_forces";
  if (!s || count < 0 || (count > 0 && (!index || !force))) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (s->resident && s->open) {
    set_error(std::string(who) + ": the resident frame is open (its pending closing half kick would mix two forces); call "
              "mythos_langevin_store first");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const int n = s->sys->n;
  std::vector<char> seen((size_t)n, 0);
  for (int e = 0; e < count; ++e) {
    if (index[e] < 0 || index[e] >= n) {
      set_error(std::string(who) + ": nucleotide index " + std::to_string(index[e]) + " out of range [0, " + std::to_string(n) + ")");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
    if (seen[index[e]]) {
      set_error(std::string(who) + ": nucleotide " + std::to_string(index[e]) + " is listed twice (sum its forces first)");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
    seen[index[e]] = 1;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(force[3 * (size_t)e + k])) {
        set_error(std::string(who) + ": a force component is not finite");
        return MYTHOS_ERR_INVALID_ARGUMENT;
      }
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  s->ext_stamp_stale = true;
  if (count == 0) {
    s->ext_count = 0;
    return MYTHOS_OK;
  }
  // an earlier advance may still be reading the old list on its stream: wait before replacing it
  MYTHOS_HIP_TRY(hipDeviceSynchronize());
  std::vector<double> f4((size_t)count * 4, 0.0);
  for (int e = 0; e < count; ++e)
    for (int k = 0; k < 3; ++k) f4[4 * (size_t)e + k] = force[3 * (size_t)e + k];
  s->ext_count = 0;  // (nothing half replaced counts)
  if (int rc = s->d_ext_index.upload(index, (size_t)count)) return rc;
  if (int rc = s->d_ext_force.upload_real(s->sys->dtype, f4.data(), f4.size())) return rc;
  if (!s->d_ext_stamp)
    if (int rc = s->d_ext_stamp.alloc(1)) return rc;
  s->ext_count = count;
  return MYTHOS_OK;
}

int mythos_langevin_set_restraints(mythos_sim_t* s, int n_tethers, const int32_t* t_index, const double* t_k, const double* t_anchor,
                                   const int32_t* t_mask, int n_groups, const int32_t* g_kind, const int32_t* g_first,
                                   const int32_t* g_member, const double* g_vec, const double* g_target, const int32_t* g_mask) {
  const std::string who = "mythos_langevin_set_restraints";
  auto refuse = [&](const std::string& why) {
    set_error(who + ": " + why);
    return MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (!s || n_tethers < 0 || n_groups < 0 || (n_tethers > 0 && (!t_index || !t_k || !t_anchor || !t_mask)) ||
      (n_groups > 0 && (!g_kind || !g_first || !g_member || !g_vec || !g_target || !g_mask)))
    return refuse("invalid argument");
  if (s->resident && s->open)
    return refuse("the resident frame is open (its pending closing half kick would mix two forces); call mythos_langevin_store first");
  const int n = s->sys->n;
  auto in_range = [&](int i) { return i >= 0 && i < n; };
  auto finite3 = [](const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
  const std::string range = " out of range [0, " + std::to_string(n) + ")";
  // terms[i]: the terms that name nucleotide i, the tether first, then the groups ascending (the order the kick adds in)
  std::vector<std::vector<int>> terms((size_t)n);
  for (int t = 0; t < n_tethers; ++t) {
    const int i = t_index[t];
    if (!in_range(i)) return refuse("nucleotide index " + std::to_string(i) + range);
    if (!terms[i].empty()) return refuse("nucleotide " + std::to_string(i) + " is listed twice among the tethers");
    if (!std::isfinite(t_k[t]) || !finite3(t_anchor + 3 * (size_t)t)) return refuse("a tether's stiffness or anchor is not finite");
    if (t_k[t] < 0) return refuse("a tether's stiffness is negative (k >= 0)");
    if (t_mask[t] < 0 || t_mask[t] > 7) return refuse("an axis mask is not a combination of the bits 1, 2, 4");
    terms[i].push_back(t);
  }
  if (n_groups > 0 && g_first[0] != 0) return refuse("the member ranges start at 0");
  std::vector<int> last_group((size_t)n, -1);
  for (int g = 0; g < n_groups; ++g) {
    const int b = g_first[g], e = g_first[g + 1];
    const bool torque = g_kind[g] == EXT_GROUP_TORQUE;
    if (g_kind[g] != EXT_GROUP_SUM && !torque) return refuse("group kind " + std::to_string(g_kind[g]) + " (0: sum restraint, 1: torque)");
    if (e < b) return refuse("the member ranges must not decrease");
    if (e - b < (torque ? 2 : 1))
      return refuse("group " + std::to_string(g) + " has " + std::to_string(e - b) + " members (a sum restraint needs at least one, a torque group two)");
    const double* vec = g_vec + 3 * (size_t)g;
    if (torque) {
      if (!finite3(vec)) return refuse("a torque is not finite");
      if (!(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2] > 0)) return refuse("a torque is zero (|T| > 0)");
    } else {
      if (!std::isfinite(vec[0]) || !finite3(g_target + 3 * (size_t)g)) return refuse("a sum restraint's stiffness or target is not finite");
      if (vec[0] < 0) return refuse("a sum restraint's stiffness is negative (k >= 0)");
      if (g_mask[g] < 0 || g_mask[g] > 7) return refuse("an axis mask is not a combination of the bits 1, 2, 4");
    }
    for (int m = b; m < e; ++m) {
      const int i = g_member[m];
      if (!in_range(i)) return refuse("nucleotide index " + std::to_string(i) + range);
      if (last_group[i] == g) return refuse("nucleotide " + std::to_string(i) + " is listed twice in group " + std::to_string(g));
      last_group[i] = g;
      terms[i].push_back(~g);
    }
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  s->rst_stamp_stale = true;
  // an earlier advance may still be reading the old arrays on its stream: wait before replacing them
  if (s->rst.n_entries > 0 || n_tethers > 0 || n_groups > 0) MYTHOS_HIP_TRY(hipDeviceSynchronize());
  s->rst = ext_point_part(s->rst);  // (nothing half replaced counts; the point terms are not this call's)
  s->h_rst_index.clear(), s->h_rst_term.clear(), s->h_rst_first.assign(1, 0);
  if (n_tethers == 0 && n_groups == 0) return ext_entries_merge(s);
  std::vector<int> e_index, e_first{0}, e_term;
  for (int i = 0; i < n; ++i) {
    if (terms[i].empty()) continue;
    e_index.push_back(i);
    e_term.insert(e_term.end(), terms[i].begin(), terms[i].end());
    e_first.push_back((int)e_term.size());
  }
  const size_t nt = (size_t)n_tethers, ng = (size_t)n_groups, nm = n_groups > 0 ? (size_t)g_first[n_groups] : 0;
  int rc = 0;
  auto up = [&](auto& buf, const auto* host, size_t count) {
    if (!rc) rc = buf.upload(host, count);
  };
  up(s->d_rst_t_index, t_index, nt), up(s->d_rst_t_k, t_k, nt), up(s->d_rst_t_anchor, t_anchor, 3 * nt), up(s->d_rst_t_mask, t_mask, nt);
  up(s->d_rst_g_kind, g_kind, ng), up(s->d_rst_g_first, g_first, n_groups > 0 ? ng + 1 : 0), up(s->d_rst_g_member, g_member, nm);
  up(s->d_rst_g_vec, g_vec, 3 * ng), up(s->d_rst_g_target, g_target, 3 * ng), up(s->d_rst_g_mask, g_mask, ng);
  if (!rc) rc = s->d_rst_g_row.alloc(ng * kExtRow);
  if (rc) return ext_entries_merge(s), rc;
  ExtFieldView& v = s->rst;
  v.n_tethers = n_tethers, v.n_groups = n_groups;
  v.t_index = s->d_rst_t_index.get(), v.t_k = s->d_rst_t_k.get(), v.t_anchor = s->d_rst_t_anchor.get(), v.t_mask = s->d_rst_t_mask.get();
  v.g_kind = s->d_rst_g_kind.get(), v.g_first = s->d_rst_g_first.get(), v.g_member = s->d_rst_g_member.get();
  v.g_vec = s->d_rst_g_vec.get(), v.g_target = s->d_rst_g_target.get(), v.g_mask = s->d_rst_g_mask.get(), v.g_row = s->d_rst_g_row.get();
  s->h_rst_index = std::move(e_index), s->h_rst_first = std::move(e_first), s->h_rst_term = std::move(e_term);
  return ext_entries_merge(s);
}

int mythos_point_forces_check(int n, int has_box, int n_terms, const int32_t* kind, const int32_t* particle, const int32_t* ref_particle,
                              const int32_t* flags, const double* param) {
  const char* who = "mythos_point_forces_check";
  if (n < 0 || n_terms < 0 || (n_terms > 0 && (!kind || !particle || !ref_particle || !flags || !param))) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  return point_forces_valid(who, n, has_box != 0, n_terms, kind, particle, ref_particle, flags, param) ? MYTHOS_OK : MYTHOS_ERR_INVALID_ARGUMENT;
}

int mythos_langevin_set_point_forces(mythos_sim_t* s, int n_terms, const int32_t* kind, const int32_t* particle, const int32_t* ref_particle,
                                     const int32_t* flags, const double* param) {
  const char* who = "mythos_langevin_set_point_forces";
  if (!s || n_terms < 0 || (n_terms > 0 && (!kind || !particle || !ref_particle || !flags || !param))) {
    set_error(std::string(who) + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (s->resident && s->open) {
    set_error(std::string(who) + ": the resident frame is open (its pending closing half kick would mix two forces); call "
              "mythos_langevin_store first");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const mythos_system* sys = s->sys;
  if (!point_forces_valid(who, sys->n, sys->has_box, n_terms, kind, particle, ref_particle, flags, param)) return MYTHOS_ERR_INVALID_ARGUMENT;
  static_assert(kPointForceParams == kExtPointParams && (int)MYTHOS_POINT_KINDS == (int)EXT_POINT_KINDS && (int)MYTHOS_POINT_PBC == (int)EXT_POINT_PBC &&
                    (int)MYTHOS_POINT_SPHERE == (int)EXT_POINT_SPHERE,
                "the public enum is the kernel's");
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  s->rst_stamp_stale = true;
  // an earlier advance may still be reading the old arrays on its stream: wait before replacing them
  if (s->rst.n_entries > 0 || n_terms > 0) MYTHOS_HIP_TRY(hipDeviceSynchronize());
  ExtFieldView& v = s->rst;
  v.n_entries = v.n_points = 0;  // (nothing half replaced counts)
  v.pt_first = v.pt_kind = v.pt_particle = v.pt_ref = v.pt_flags = nullptr, v.pt_param = nullptr;
  s->h_pt_particle.clear();
  s->pt_moving = false;
  for (int t = 0; t < n_terms; ++t) {
    const int at = point_force_rate_at(kind[t]);
    if (at >= 0 && param[(size_t)t * kPointForceParams + at] != 0.0) s->pt_moving = true;
  }
  if (n_terms == 0) return ext_entries_merge(s);
  // by nucleotide, and within one in the order given: the order the kick adds in
  std::vector<int> order((size_t)n_terms);
  for (int t = 0; t < n_terms; ++t) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return particle[a] < particle[b]; });
  std::vector<int> k_s, p_s, r_s, f_s;
  std::vector<double> q_s;
  for (int t : order) {
    k_s.push_back(kind[t]), p_s.push_back(particle[t]), f_s.push_back(flags[t]);
    r_s.push_back(kind[t] == MYTHOS_POINT_MUTUAL_TRAP ? ref_particle[t] : particle[t]);  // (read by a mutual trap alone)
    double q[kPointForceParams];
    for (int a = 0; a < kPointForceParams; ++a) q[a] = param[(size_t)t * kPointForceParams + a];
    const int d = point_force_dir_at(kind[t]);
    if (d >= 0) {  // dir -> dir / |dir| (a resting trap may have none: zeros stay)
      const double len = std::sqrt(q[d] * q[d] + q[d + 1] * q[d + 1] + q[d + 2] * q[d + 2]);
      if (len > 0) q[d] /= len, q[d + 1] /= len, q[d + 2] /= len;
    }
    q_s.insert(q_s.end(), q, q + kPointForceParams);
  }
  int rc = s->d_pt_kind.upload(k_s);
  if (!rc) rc = s->d_pt_particle.upload(p_s);
  if (!rc) rc = s->d_pt_ref.upload(r_s);
  if (!rc) rc = s->d_pt_flags.upload(f_s);
  if (!rc) rc = s->d_pt_param.upload(q_s);
  if (rc) return ext_entries_merge(s), rc;
  v.pt_kind = s->d_pt_kind.get(), v.pt_particle = s->d_pt_particle.get(), v.pt_ref = s->d_pt_ref.get(), v.pt_flags = s->d_pt_flags.get();
  v.pt_param = s->d_pt_param.get();
  for (int a = 0; a < 3; ++a) v.box[a] = sys->has_box ? sys->box[a] : 1.0;
  s->h_pt_particle = std::move(p_s);
  return ext_entries_merge(s);
}

int mythos_langevin_eval_external_at(mythos_sim_t* s, const void* center, double step, void* force_out, double* energy_out,
                                     mythos_stream_t stream) {
  if (!s || !center || !force_out || !energy_out || !std::isfinite(step)) {
    set_error("mythos_langevin_eval_external_at: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return md_entries_of(s).eval_external(s, center, step, force_out, energy_out, kExtEnergies, (hipStream_t)stream);
}

int mythos_langevin_eval_external(mythos_sim_t* s, const void* center, void* force_out, double* energy_out, mythos_stream_t stream) {
  if (!s || !center || !force_out || !energy_out) {
    set_error("mythos_langevin_eval_external: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return md_entries_of(s).eval_external(s, center, 0.0, force_out, energy_out, 3, (hipStream_t)stream);
}

int mythos_langevin_set_seed(mythos_sim_t* s, uint64_t seed) {
  if (!s) {
    set_error("mythos_langevin_set_seed: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->seed = seed;
  return MYTHOS_OK;
}

int mythos_langevin_last_kernel_ms(const mythos_sim_t* s, double* kernel_ms, double* loop_ms_per_launch,
                                   int* launches, int* samples) {
  return md_last_kernel_ms(s, kernel_ms, loop_ms_per_launch, launches, samples, "mythos_langevin_last_kernel_ms");
}

int mythos_langevin_last_recoveries(const mythos_sim_t* s, int* recoveries) {
  return md_last_count(s, &MdRun::last_recoveries, recoveries, "mythos_langevin_last_recoveries");
}

int mythos_langevin_last_rebuilds(const mythos_sim_t* s, int* scheduled) {
  return md_last_count(s, &MdRun::last_rebuilds, scheduled, "mythos_langevin_last_rebuilds");
}

int mythos_langevin_set_option(mythos_sim_t* s, int option, int64_t value) {
  if (!s || option != MYTHOS_LANGEVIN_UNFUSED || (value != 0 && value != 1)) {
    set_error("mythos_langevin_set_option: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (value == 1 && s->sys->model != 4) {
    set_error("mythos_langevin_set_option: the unfused path exists for oxNA systems (model 4) only");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->unfused.want = value == 1;
  return MYTHOS_OK;
}

int mythos_langevin_set_timing(mythos_sim_t* s, int samples) { return md_set_timing(s, samples, "mythos_langevin_set_timing"); }

// ---- umbrella sampling (umbrella.h; mythos/simulators/oxdna/oxdna.py:225-275, utils.py:348-429)
namespace {
// what neither set_umbrella nor advance_umbrella steps with, by name
int umbrella_refusals(const mythos_sim* s, const std::string& who) {
  auto refuse = [&](const std::string& why) {
    set_error(who + ": " + why);
    return (int)MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (s->sys->model == 4)
    return refuse("an oxNA system (model 4) has three hydrogen-bonding parameter sets and two site geometries; the order "
                  "parameters are built for oxDNA1, oxDNA2 and oxRNA2");
  if (s->unfused.want || s->unfused.active) return refuse("the unfused oxNA path (MYTHOS_LANGEVIN_UNFUSED) is not sampled under a bias");
  if (s->sys->pseq_terms != 0)
    return refuse("the system carries a probabilistic sequence (mythos_oxdna_set_pseq): an expected hydrogen-bonding energy "
                  "below the cutoff is not oxDNA's order parameter");
  if (s->pt_moving)
    return refuse("a point force moves (rate != 0): its force depends on the step count, which breaks the reversibility the "
                  "acceptance rule rests on; clear it (mythos_langevin_set_point_forces) or give it rate = 0");
  return MYTHOS_OK;
}
}  // namespace

int mythos_langevin_set_umbrella(mythos_sim_t* s, int n_rep, int n_ops, const int32_t* op_kind, const int32_t* op_first, const int32_t* pairs,
                                 int n_pairs, const int32_t* iface_first, const double* interfaces, const int32_t* table_shape,
                                 const double* table, double hb_cutoff, int segment_steps) {
  const std::string who = "mythos_langevin_set_umbrella";
  auto refuse = [&](const std::string& why) {
    set_error(who + ": " + why);
    return (int)MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (!s || n_ops < 0) return refuse("invalid argument");
  if (s->resident && s->open)
    return refuse("the resident frame is open (a segment starts from a closed frame); call mythos_langevin_store first");
  UmbrellaState& u = s->umb;
  if (n_ops == 0) {  // no bias: every other call issues the launches it issued before one was set
    u.n_ops = 0;
    u.primed = false;
    return MYTHOS_OK;
  }
  if (int rc = umbrella_refusals(s, who)) return rc;
  if (!std::isfinite(hb_cutoff)) return refuse("hb_cutoff is not finite");
  if (n_rep < 1) return refuse("invalid argument");
  const mythos_system* sys = s->sys;
  const int n = sys->n, n_one = n / n_rep;
  std::vector<int32_t> bonded;  // the backbone neighbours inside the first replica
  for (int i = 0; i < n_one; ++i)
    for (int k = 0; k < ROW_BONDED_SLOTS; ++k) {
      const int j = sys->h_partners[(size_t)ROW_BONDED_SLOTS * i + k];
      if (j > i && j < n_one) bonded.push_back(i), bonded.push_back(j);
    }
  if (!umbrella_valid(who, n, n_rep, sys->model, (int)(bonded.size() / 2), bonded.data(), n_ops, op_kind, op_first, pairs, n_pairs,
                      iface_first, interfaces, table_shape, table, segment_steps))
    return MYTHOS_ERR_INVALID_ARGUMENT;
  std::vector<int> list;
  for (int k = 0; k < n_pairs; ++k) list.push_back(std::min(pairs[2 * k], pairs[2 * k + 1])), list.push_back(std::max(pairs[2 * k], pairs[2 * k + 1]));
  list.insert(list.end(), op_first, op_first + n_ops + 1);
  list.insert(list.end(), op_kind, op_kind + n_ops);
  list.insert(list.end(), iface_first, iface_first + n_ops + 1);
  list.insert(list.end(), table_shape, table_shape + n_ops);
  size_t cells = 1;
  for (int k = 0; k < n_ops; ++k) cells *= (size_t)table_shape[k];
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());  // an earlier advance may still be reading the old arrays on its stream
  u.n_ops = 0;  // (nothing half replaced counts)
  u.primed = false;
  const size_t real = sys->dtype == MYTHOS_F32 ? sizeof(float) : sizeof(double);
  int rc = u.d_list.upload(list);
  if (!rc) rc = u.d_iface.upload(interfaces, (size_t)iface_first[n_ops]);
  if (!rc) rc = u.d_table.upload(table, cells);
  if (!rc) rc = u.d_w_cur.alloc((size_t)n_rep);
  if (!rc) rc = u.d_accept.alloc((size_t)n_rep);
  if (!rc) rc = u.d_state.alloc(2 * (size_t)n_rep * n_ops);
  if (!rc) rc = u.d_counts.alloc(2);
  if (!rc) rc = u.d_err.alloc(1);
  if (!rc) rc = u.d_prime_rec.alloc((size_t)n_rep * umbrella_record_width(n_ops));
  for (int w = 0; w < 8 && !rc; ++w) rc = u.snap[w].grow(4 * real * (size_t)n);
  if (!rc) rc = u.stage_c.grow(3 * real * (size_t)n);
  if (!rc) rc = u.stage_q.grow(4 * real * (size_t)n);
  if (!rc) rc = u.stage_p.grow(3 * real * (size_t)n);
  if (!rc) rc = u.stage_l.grow(3 * real * (size_t)n);
  if (rc) return rc;
  MYTHOS_HIP_TRY(hipMemset(u.d_counts.get(), 0, 2 * sizeof(unsigned long long)));
  u.n_pairs = n_pairs, u.n_rep = n_rep, u.n_one = n_one, u.segment_steps = segment_steps, u.hb_cutoff = hb_cutoff;
  u.n_ops = n_ops;
  return MYTHOS_OK;
}

int mythos_langevin_advance_umbrella(mythos_sim_t* s, int n_segments, int sample_every, void* traj_center, void* traj_quat, void* prop_center,
                                     void* prop_quat, double* record, mythos_stream_t stream) {
  const std::string who = "mythos_langevin_advance_umbrella";
  if (!s || n_segments < 0 || sample_every < 0) {
    set_error(who + ": invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  UmbrellaState& u = s->umb;
  if (u.n_ops == 0) {
    set_error(who + ": no bias is set (call mythos_langevin_set_umbrella first)");
    return MYTHOS_ERR_NOT_READY;
  }
  if (!s->resident) {
    set_error(who + ": no resident state (call mythos_langevin_load first; a run that ended in a numeric error drops its state)");
    return MYTHOS_ERR_NOT_READY;
  }
  if (int rc = md_ready(s, who.c_str())) return rc;
  if (int rc = umbrella_refusals(s, who)) return rc;
  mythos_system* sys = s->sys;
  if (sys->n != u.n_rep * u.n_one) {
    set_error(who + ": the bias was set for another system size");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const size_t q_align = sys->dtype == MYTHOS_F32 ? sizeof(float4) : sizeof(double4);
  for (const void* tq : {traj_quat, prop_quat})
    if (tq && (reinterpret_cast<uintptr_t>(tq) % q_align) != 0) {
      set_error(who + ": traj_quat and prop_quat must be aligned to 4 elements (" + std::to_string(q_align) + " bytes)");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
  hipStream_t st = (hipStream_t)stream;
  const MdEntries entries = md_entries_of(s);
  if (s->open)  // a segment starts from a closed frame
    if (int rc = md_advance(s, 0, 0, true, nullptr, nullptr, nullptr, st)) return rc;
  const UmbrellaView v{u.n_ops,         u.n_pairs,       u.n_rep,          u.n_one,          u.hb_cutoff,     u.d_list.get(),   u.d_iface.get(),
                       u.d_table.get(), u.d_w_cur.get(), u.d_accept.get(), u.d_state.get(), u.d_counts.get(), u.d_err.get()};
  const int width = umbrella_record_width(u.n_ops);
  void* snap[8];
  for (int w = 0; w < 8; ++w) snap[w] = u.snap[w].get();
  // the boundary at the resident (closed) frame: decide, then commit with the rows of sample `row` (negative: none)
  auto boundary = [&](bool prime, double* rec, long long row) -> int {
    void* frame[8];
    for (int w = 0; w < 8; ++w) frame[w] = s->frame[s->cur][w].get();
    if (int rc = umbrella_decide_launch(sys, v, frame[0], frame[4], s->seed, (uint64_t)s->step, prime, rec, st)) return rc;
    const size_t real = sys->dtype == MYTHOS_F32 ? sizeof(float) : sizeof(double);
    auto at = [&](void* base, int w) -> void* { return (base && row >= 0) ? (char*)base + (size_t)row * sys->n * w * real : nullptr; };
    return umbrella_commit_launch(sys->dtype, sys->n, u.n_one, frame, snap, u.d_accept.get(), at(traj_center, 3), at(traj_quat, 4),
                                  at(prop_center, 3), at(prop_quat, 4), st);
  };
  // parameters replaced since the weights held were looked up (mythos_oxdna_set_params): the states are evaluated again
  if (u.param_epoch != sys->param_epoch) u.primed = false;
  if (!u.primed) {
    // the first boundary: the resident state becomes the snapshot whatever its weight, and a weight of 0 is an error
    MYTHOS_HIP_TRY(hipMemsetAsync(u.d_err.get(), 0x7f, sizeof(int), st));
    if (int rc = boundary(true, u.d_prime_rec.get(), -1)) return rc;
    int bad = 0;
    MYTHOS_HIP_TRY(hipMemcpyAsync(&bad, u.d_err.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
    if (bad >= 0 && bad < u.n_rep) {
      std::vector<double> row((size_t)width);
      MYTHOS_HIP_TRY(hipMemcpy(row.data(), u.d_prime_rec.get() + (size_t)bad * width, width * sizeof(double), hipMemcpyDeviceToHost));
      std::string state;
      for (int k = 0; k < u.n_ops; ++k) state += (k ? ", " : "") + std::to_string((long long)row[u.n_ops + k]);
      set_error(who + ": replica " + std::to_string(bad) + " starts in state (" + state + "), which has weight 0 in the table");
      return MYTHOS_ERR_INVALID_ARGUMENT;
    }
    u.primed = true;
    u.param_epoch = sys->param_epoch;
  }
  for (int b = 0; b < n_segments; ++b) {
    // The neighbour rows are rebuilt at the start of every segment exactly as after mythos_langevin_load - by loading: the
    // closed frame goes out and comes back through the kernels of store and load (a frame that load has just left is
    // theirs already).  One build per segment, whichever replicas were rejected, and a run that is bit for bit the loop
    // load; advance(L); store of the plain integrator where every proposal is accepted.
    if (!u.frame_loaded) {
      if (int rc = entries.store(s, u.stage_c.get(), u.stage_q.get(), u.stage_p.get(), u.stage_l.get(), st)) return rc;
      if (int rc = entries.load(s, u.stage_c.get(), u.stage_q.get(), u.stage_p.get(), u.stage_l.get(), st)) return rc;
    }
    if (int rc = md_advance(s, u.segment_steps, 0, true, nullptr, nullptr, nullptr, st)) return rc;
    const bool sample = sample_every > 0 && (b + 1) % sample_every == 0;
    if (int rc = boundary(false, record ? record + (size_t)b * u.n_rep * width : nullptr, sample ? (b + 1) / sample_every - 1 : -1)) return rc;
  }
  return MYTHOS_OK;
}

int mythos_langevin_umbrella_counts(mythos_sim_t* s, int64_t* accepted, int64_t* decided) {
  if (!s || !accepted || !decided) {
    set_error("mythos_langevin_umbrella_counts: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  *accepted = *decided = 0;
  if (!s->umb.d_counts) return MYTHOS_OK;
  unsigned long long c[2] = {0, 0};
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());
  MYTHOS_HIP_TRY(hipMemcpy(c, s->umb.d_counts.get(), sizeof(c), hipMemcpyDeviceToHost));
  *accepted = (int64_t)c[0], *decided = (int64_t)c[1];
  return MYTHOS_OK;
}

}  // extern "C"
