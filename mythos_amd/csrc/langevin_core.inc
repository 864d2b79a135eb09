// (langevin_core.inc: the host driver of the oxDNA Langevin integrator, included by langevin.hip - the fp32 instantiations
// and the C entry points - and by langevin_f64.hip - the fp64 instantiations; two translation units because the two
// precisions want different compiler switches, see the Makefile)
//
// The parts, by concern:
//   langevin_step.h      the fused step kernel md_step_kernel and its device helpers (device code only)
//   langevin_frame.h     pack / unpack / rederive / init-momenta / external-kick kernels
//   ext_field.h          the position-dependent external kick: tethers, sum restraints, group torques, point terms
//   langevin_sim.h       struct mythos_sim and the host helpers that only read it
//   langevin_unfused.inc the oxNA cross-check path, a second integrator with its own state and step loop
//   md_plan.h            which instantiation a launch takes (pure host arithmetic, checked by the CPU suite)
// Here: load_typed, unpack_typed, advance_typed - the one place md_step_kernel is launched - and the per-precision entry
// points (MdEntries).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include <hip/hip_ext.h>

// The fp32 stepping kernels evaluate the piecewise modulation functions (f1, f2, f4, f5) in their branch-free forms
// and read the sequence weights with one indexed load (oxdna_math.h: MYTHOS_LEAN_MATH).  Measured on MI355X (round 3,
// A/B of one build against the other on one box): 12 kbp 61.4 k -> 63.9 k steps/s, 100 kbp 10.7 k -> 11.3 k, 256
// replicas of 64 nt 62.7 k -> 65.4 k; the base-pair item of the angular pass 949 VALU + 434 SALU -> 744 + 151.  fp64
// keeps the branchy forms: with the branch-free ones the three-per-CU instantiation spilled more (29.4 k -> 25.7 k).
#ifndef MYTHOS_LEAN_MATH
#define MYTHOS_LEAN_MATH 1
#endif

#include "cell_list.h"
#include "chunk_order.h"
#include "md_driver.h"
#include "md_plan.h"
#include "oxdna_gather.h"
#include "philox.h"

#include "langevin_step.h"
#include "langevin_frame.h"
#include "ext_field.h"
#include "langevin_unfused.inc"  // (UnfusedState, then langevin_sim.h, then the path's host side)

using namespace mythos;

namespace mythos {

static_assert(kMdPlanBlock == kMdBlock, "md_plan.h plans for the step kernel's workgroup");

// compute units of the system's device (256 where the runtime does not say)
inline int device_cus(const mythos_system* sys) {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sys->device);
  return cus;
}

// Spatial order of the workgroups' chunks (chunk_order.h): two small kernels on the run's stream, at every load and
// every 64th scheduled list rebuild (molecules drift slowly, and a stale order costs speed, not correctness).
// Systems under 64 chunks do not bother.
template <typename R>
static int update_chunk_order(mythos_sim* sim, const typename Vec4T<R>::type* p0, int blocks, hipStream_t st) {
  if (blocks < 64) {  // (index order; a stale order of another chunk size must not survive a change of lanes)
    sim->d_chunk_order.reset(), sim->d_chunk_keys.reset();
    return 0;
  }
  if (int rc = sim->d_chunk_keys.grow((size_t)blocks)) return rc;
  if (int rc = sim->d_chunk_order.grow((size_t)blocks)) return rc;
  MYTHOS_HIP_TRY(chunk_order_device(p0, blocks, kMdBlock / sim->lanes, std::max(1.0, sim->r_cut > 0 ? sim->r_cut : 4.0), sim->d_chunk_keys.get(),
                                    sim->d_chunk_order.get(), st));
  return 0;
}

// The position-dependent external kick (ext_field.h) of view v on the momenta `mom`, forces taken at (p0, pl): the group
// rows, then the gather-and-kick with one stamp word per workgroup.  The one place these two kernels are launched - in
// front of a step launch, and by mythos_langevin_eval_external(_at) with c_dt = 1 on zeroed momenta.  The point terms
// (mythos_langevin_set_point_forces) are terms of the same entries: they add no launch.  step: the step count of the
// frame (p0, pl), which the moving laws take as their time (ext_field.h).
inline int ext_field_blocks(const ExtFieldView& v) { return (v.n_entries + 255) / 256; }
template <typename R>
static void launch_ext_field_kick(const ExtFieldView& v, const typename Vec4T<R>::type* p0, const typename Vec4T<R>::type* pl, double c_dt,
                                  double step, typename Vec4T<R>::type* mom, const int* flags, const int* halt_words, int k,
                                  unsigned long long stamp, unsigned long long* stamps, hipStream_t st) {
  if (v.n_groups > 0) hipLaunchKernelGGL(ext_group_kernel<R>, dim3(v.n_groups), dim3(256), 0, st, v, p0, pl);
  hipLaunchKernelGGL(ext_field_kick_kernel<R>, dim3(ext_field_blocks(v)), dim3(256), 0, st, v, p0, pl, c_dt, step, mom, flags, halt_words,
                     k, stamp, stamps);
}

// Caller's (N,3)/(N,4) arrays -> the resident frames.  The list of a previous state does not carry over.
template <typename R, int MODEL>
static int load_typed(mythos_sim* sim, const R* center, const R* quat, const R* p_lin, const R* p_ang, hipStream_t st) {
  mythos_system* sys = sim->sys;
  const int n = sys->n;
  const int tb = (n + 255) / 256;
  const OxParams<R>& P = params_of<R>(sys);
  const R g_k1 = P[GEO_BACK_A1], g_k2 = (MODEL >= 2) ? P[GEO_BACK_A2] : R(0);
  sim->cur = 0;
  const Frame<R> f0 = frame_of<R>(sim, 0);
  // (oxNA: the RNA nucleotides take the oxRNA2 vector's backbone site)
  const double* Prna = oxdna_param_set(sys, sys->param_sets() == 1 ? 0 : 1);
  hipLaunchKernelGGL((pack_state_kernel<R, (MODEL == 4 ? 0 : back_axis<MODEL>())>), dim3(tb), dim3(256), 0, st, n, g_k1, g_k2,
                     R(Prna[GEO_BACK_A1]), R(Prna[GEO_BACK_A2]), center, quat, p_lin, p_ang,
                     sys->d_meta.get(), f0, sim->keep_valid ? (const R*)sim->keep_hi.get() : nullptr,
                     (const R*)sim->keep_lo.get());
  MYTHOS_HIP_TRY(hipGetLastError());
  sim->resident = true;
  sim->list_valid = false;
  sim->since_build = 0;
  sim->items_big = false;
  sim->open = false;
  sim->ext_stamp_stale = true;
  sim->rst_stamp_stale = true;
  sim->param_epoch = sys->param_epoch;
  const int cus = device_cus(sys);
  sim->lanes = md_lanes_for(n, cus, debug_value(MYTHOS_DEBUG_MD_LANES));  // (the debug value is read here, at load)
  return update_chunk_order<R>(sim, f0.p0, md_plan_for(n, sim->lanes, cus, sizeof(R), 0).blocks, st);
}

// The resident frames -> caller's arrays (asynchronous on st; the state stays resident).
template <typename R>
static int unpack_typed(mythos_sim* sim, R* center, R* quat, R* p_lin, R* p_ang, hipStream_t st) {
  const int n = sim->sys->n;
  hipLaunchKernelGGL(unpack_state_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, st, n, frame_of<R>(sim, sim->cur),
                     center, quat, p_lin, p_ang, (R*)sim->keep_hi.get(), (R*)sim->keep_lo.get());
  MYTHOS_HIP_TRY(hipGetLastError());
  sim->keep_valid = true;
  return 0;
}

// n_steps on the resident state: md_drive (md_driver.h) runs the launches, the list's rebuild schedule and the recovery
// from a halt; what is oxDNA's is here - the frame's site offsets after a parameter change, the choice of instantiation
// per launch, the chunk order, and the wider work lists after an aborted launch.
// Rows with energies (e_trace != NULL) come from the energy-trace instantiation: launch k evaluates at x_k, writes row
// k / save_every - 1 (positions, term and kinetic energies) and a reduction launch follows.  Rows WITHOUT energies - the
// reference's own semantics of run - cost two stores in the plain instantiation: launch k, which produces x_{k+1}, writes
// it to its row as well; such a call needs no closing launch for its last row and leaves the frame open like any other.
template <typename R, int MODEL>
static int advance_typed(mythos_sim* sim, int n_steps, int save_every, bool close, R* traj_center, R* traj_quat, double* e_trace,
                         hipStream_t st) {
  using V4 = typename Vec4T<R>::type;
  mythos_system* sys = sim->sys;
  const int n = sys->n;
  // which instantiation and grid (md_plan.h); MYTHOS_DEBUG_MD_DENSE is read here, at every advance
  const MdPlan plan = md_plan_for(n, sim->lanes, device_cus(sys), sizeof(R), debug_value(MYTHOS_DEBUG_MD_DENSE));
  const int blocks = plan.blocks;
  const R* Pdev = device_params_of<R>(sys);
  const BoxT<R> box = make_box<R>(sys);
  const LangevinConst<R> K = make_const<R>(sim);
  const MdCut<R> cut = make_cut<R>(sys);
  const Frame<R> fr[2] = {frame_of<R>(sim, 0), frame_of<R>(sim, 1)};
  if (sim->param_epoch != sys->param_epoch) {  // mythos_oxdna_set_params / set_nucleotide_types since the load
    const OxParams<R>& Ph = params_of<R>(sys);
    const double* Prna = oxdna_param_set(sys, sys->param_sets() == 1 ? 0 : 1);
    hipLaunchKernelGGL((rederive_frame_kernel<R, (MODEL == 4 ? 0 : back_axis<MODEL>())>), dim3((n + 255) / 256), dim3(256), 0, st, n,
                       Ph[GEO_BACK_A1], (MODEL >= 2) ? Ph[GEO_BACK_A2] : R(0), R(Prna[GEO_BACK_A1]), R(Prna[GEO_BACK_A2]),
                       (const int*)sys->d_meta.get(), fr[sim->cur]);
    MYTHOS_HIP_TRY(hipGetLastError());
    sim->param_epoch = sys->param_epoch;
  }
  const bool dynamic_list = sim->rebuild_every > 0;
  // a probabilistic sequence (mythos_oxdna_set_pseq): the PSEQ instantiations - since round 4 with the short work lists
  // too (ITEMS = 16, abort -> wide fallback as the plain path), so such a run steps at the plain rate's occupancy
  PseqView<R> pseq;
  const bool use_pseq = sys->pseq_terms != 0;
  if (debug_value(MYTHOS_DEBUG_MD_ITEMS_BIG) == 1) sim->items_big = true;  // (tests: the wide instantiations without a crowded system)
  if (use_pseq) pseq.marg = (const R*)sys->d_ps_marg.get(), pseq.unit = sys->d_ps_unit.get(), pseq.bp = (const R*)sys->d_ps_bp.get(), pseq.terms = sys->pseq_terms;
  int* halt_words = dynamic_list ? sys->list.d_overflow.get() : nullptr;
  auto launch_step = [&](int k, const LaunchRow& row) {
    const int cur = row.cur;
    const bool save = row.save;
    const R kick_close = R(row.kick_close);
    R* tc = ((save || row.save_next) && traj_center) ? traj_center + (size_t)row.sidx * n * 3 : nullptr;
    R* tq = ((save || row.save_next) && traj_quat) ? traj_quat + (size_t)row.sidx * n * 4 : nullptr;
    const V4* ref = (const V4*)sys->d_ref_pos.get();
    const V4* ref_off = (const V4*)sys->d_ref_off.get();
    const V4* ref_a1 = (const V4*)sys->d_ref_a1.get();
    if (sim->ext_count > 0) {  // the external kick of this launch (ext_kick_kernel); outside the dispatch's event pair
      if (sim->ext_stamp_stale) {
        (void)hipMemsetAsync(sim->d_ext_stamp.get(), 0, sizeof(unsigned long long), st);
        sim->ext_stamp_stale = false;
      }
      const double c = double(row.kick_close) + 0.5 * row.do_step;
      const unsigned long long stamp = 2ull * (unsigned long long)(sim->step + k) + (row.kick_close != 0.0f ? 1ull : 0ull) + 1ull;
      hipLaunchKernelGGL(ext_kick_kernel<R>, dim3(1), dim3(256), 0, st, sim->ext_count, (const int*)sim->d_ext_index.get(),
                         (const V4*)sim->d_ext_force.get(), R(c * sim->dt), fr[cur].mom, (const int*)sim->d_flags.get(),
                         (const int*)halt_words, k, stamp, sim->d_ext_stamp.get());
    }
    if (sim->rst.n_entries > 0) {  // the position-dependent kick of this launch (ext_field.h), same slot, same stamp value
      if (sim->rst_stamp_stale) {
        (void)hipMemsetAsync(sim->d_rst_stamp.get(), 0, sizeof(unsigned long long) * (size_t)ext_field_blocks(sim->rst), st);
        sim->rst_stamp_stale = false;
      }
      const double c = double(row.kick_close) + 0.5 * row.do_step;
      const unsigned long long stamp = 2ull * (unsigned long long)(sim->step + k) + (row.kick_close != 0.0f ? 1ull : 0ull) + 1ull;
      launch_ext_field_kick<R>(sim->rst, fr[cur].p0, kHiLo<R> ? fr[cur].pl : nullptr, c * sim->dt, double(sim->step + k), fr[cur].mom,
                               (const int*)sim->d_flags.get(), (const int*)halt_words, k, stamp, sim->d_rst_stamp.get(), st);
    }
    // The one launch of md_step_kernel, its arguments written once.  With events: the pair receives the begin / end time
    // stamps of THIS dispatch (the same stamps a profiler's kernel trace reports), not the time between two markers in
    // the queue.
    auto launch = [&](auto save_tag, auto items_tag, auto pseq_tag, auto dense_tag, auto lanes_tag) {
      hipExtLaunchKernelGGL((md_step_kernel<R, MODEL, decltype(save_tag)::value, decltype(items_tag)::value, decltype(pseq_tag)::value,
                                            decltype(dense_tag)::value, decltype(lanes_tag)::value>),
                            dim3(plan.grid), dim3(kMdBlock), 0, st, row.ea, row.eb, 0,
                            Pdev, box, K, cut, n, fr[cur], fr[cur ^ 1], sys->list.d_rows.get(), sys->d_row_len.get(), row_close_of(sys),
                            sys->list.stride, sys->extra_bonds ? 1 : 0, kick_close, row.do_step, sim->seed, (uint64_t)(sim->step + k), ref,
                            ref_off, ref_a1, sim->d_flags.get(), tc, tq, sim->d_epart.get(), sim->d_chunk_order.get(), halt_words, k, 0,
                            plan.prio_on, pseq);
    };
    // ... reached through the tags save, items, pseq, dense, lanes.  DENSE exists for fp32 stepping of oxDNA1 / oxDNA2 with
    // the short work lists, a discrete sequence and 8 lanes only (md_blocks_per_cu); everything else, a PSEQ run on a dense
    // grid included, takes the plain instantiation.
    with_bool(save, [&](auto save_tag) {
      with_bool(sim->items_big, [&](auto big_tag) {
        constexpr bool SV = decltype(save_tag)::value;
        using Items = std::integral_constant<int, decltype(big_tag)::value ? md_items_big<R, SV>() : kMdItems>;
        with_bool(use_pseq, [&](auto pseq_tag) {
          using L8 = std::integral_constant<int, 8>;
          using L16 = std::integral_constant<int, 16>;
          // (plan.dense_grid - fp32, 8 lanes, a large grid - is necessary, not sufficient: SAVE, PSEQ, ITEMS and MODEL decide here)
          constexpr bool dense_exists = sizeof(R) == 4 && !SV && !decltype(pseq_tag)::value && Items::value == kMdItems && MODEL <= 2;
          if (sim->lanes == 16) {
            launch(save_tag, Items{}, pseq_tag, std::false_type{}, L16{});
          } else if constexpr (dense_exists) {
            with_bool(plan.dense_grid, [&](auto dense_tag) { launch(save_tag, Items{}, pseq_tag, dense_tag, L8{}); });
          } else {
            launch(save_tag, Items{}, pseq_tag, std::false_type{}, L8{});
          }
        });
      });
    });
    if (save)
      hipLaunchKernelGGL(reduce_trace_kernel<kTraceWidth>, dim3(1), dim3(256), 0, st, sim->d_epart.get(), blocks,
                         e_trace + (size_t)row.sidx * kTraceWidth);
  };
  // Where the cell builder makes the rows, a rebuild filters candidate rows instead (neighbors.hip: filter_rows_kernel),
  // behind a wide build where row_filter_plan.h says so: the first build of a list, every kCandEvery-th rebuild, every
  // recovery.  The rows are the builder's either way; mythos_debug_set(MYTHOS_DEBUG_ROWS_FILTER, 0) has the builder make
  // them all, as do systems the all-pairs kernel serves.
  const int cand_every = cand_every_for(debug_value(MYTHOS_DEBUG_ROWS_CAND_EVERY));
  const double cand_margin = cand_margin_for(debug_value(MYTHOS_DEBUG_ROWS_CAND_MARGIN));
  const int cand_margin_milli = (int)std::lround(1e3 * cand_margin);
  bool filter_rows = dynamic_list && debug_value(MYTHOS_DEBUG_ROWS_FILTER) != 0 && !sys->cand_unfit &&
                     rows_filter_applies(sys, sim->r_cut, sim->skin, cand_margin);
  auto rebuild = [&](int buf) -> int {
    if ((++sim->builds & 63) == 0)
      if (int rc = update_chunk_order<R>(sim, fr[buf].p0, blocks, st)) return rc;
    if (!filter_rows) {
      sim->cand = cand_none();
      return rows_build_device(sys, fr[buf].p0, true, sim->r_cut, sim->skin, fr[buf].p3, fr[buf].p1, true, st);
    }
    const bool wide = cand_rebuild_is_wide(sim->cand, sim->list_valid, cand_every, cand_margin_milli);
    if (wide) {
      sim->cand = cand_none();  // (should the build fail)
      if (int rc = rows_wide_build_device(sys, fr[buf].p0, sim->r_cut, sim->skin, cand_margin, st)) return rc;
    }
    sim->cand = cand_after(wide, sim->cand, cand_margin_milli);
    return rows_filter_device(sys, fr[buf].p0, fr[buf].p3, fr[buf].p1, sim->r_cut, sim->skin, cand_margin, st);
  };
  auto rebuild_until_fit = [&](int buf) -> int {
    sim->cand = cand_none();
    if (filter_rows) {
      const int rc = rows_filter_until_fit(sys, fr[buf].p0, fr[buf].p3, fr[buf].p1, sim->r_cut, sim->skin, cand_margin, st);
      if (rc == MYTHOS_OK) sim->cand = cand_after(true, sim->cand, cand_margin_milli);
      if (!sys->cand_unfit) return rc;
      filter_rows = false;  // (candidate rows too long for this system: the full builder from here on)
    }
    return rows_build_until_fit(sys, fr[buf].p0, true, sim->r_cut, sim->skin, fr[buf].p3, fr[buf].p1, true, true, st);
  };
  auto on_abort = [&]() -> int {
    if (!sim->items_big) {
      sim->items_big = true;  // run that step again, and the rest of the run, with the wider instantiation
      return 0;
    }
    set_error("mythos_langevin_run: more than " + std::to_string(md_items_big<R, false>()) + " (" + std::to_string(md_items_big<R, true>()) +
              " on steps that save energies)"
              " neighbours of one nucleotide are inside the range of an angular term (overlapping bases?)");
    return MYTHOS_ERR_OVERFLOW;
  };
  MdDrive d;
  d.who = "mythos_langevin_run";
  d.n_steps = n_steps, d.save_every = save_every, d.close = close;
  d.energy_rows = save_every > 0 && e_trace != nullptr;
  d.plain_rows = save_every > 0 && e_trace == nullptr && (traj_center != nullptr || traj_quat != nullptr);
  d.dynamic_list = dynamic_list;
  d.halt_words = halt_words;
  d.row_stride = &sys->list.stride;
  d.skin = sim->skin;
  d.st = st;
  return md_drive(*sim, d, launch_step, rebuild, rebuild_until_fit, on_abort);
}

// ---- per-precision entry points of the integrator: templates here, instantiated by name in the translation unit of their
//      precision alone (langevin.hip: float, langevin_f64.hip: double), so neither unit holds a kernel of the other's
template <typename R>
static int entry_load(mythos_sim* s, void* c, void* q, void* p, void* l, hipStream_t st) {
  if (s->unfused.active) return unfused_load<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);
  return with_model(s->sys->model, [&](auto m) { return load_typed<R, decltype(m)::value>(s, (R*)c, (R*)q, (R*)p, (R*)l, st); });
}

template <typename R>
static int entry_advance(mythos_sim* s, int n_steps, int save_every, bool close, void* tc, void* tq, double* e_trace, hipStream_t st) {
  if (s->unfused.active) return unfused_advance<R>(s, n_steps, save_every, (R*)tc, (R*)tq, e_trace, st);
  return with_model(s->sys->model, [&](auto m) {
    return advance_typed<R, decltype(m)::value>(s, n_steps, save_every, close, (R*)tc, (R*)tq, e_trace, st);
  });
}

template <typename R>
static int entry_store(mythos_sim* s, void* c, void* q, void* p, void* l, hipStream_t st) {
  if (s->unfused.active) return unfused_store<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);
  // an open frame (mythos_langevin_advance) gets its closing half kick first; should that fail, the open state goes
  // back all the same, with the error
  const int rc = s->open ? entry_advance<R>(s, 0, 0, true, nullptr, nullptr, nullptr, st) : MYTHOS_OK;
  const int ru = unpack_typed<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);
  return rc ? rc : ru;
}

template <typename R>
static int entry_init_momenta(mythos_sim* s, void* p_lin, void* p_ang, hipStream_t st) {
  const double sd_t = std::sqrt(s->mass * s->kT);
  double sd_r[3];
  for (int k = 0; k < 3; ++k) sd_r[k] = std::sqrt(s->inertia[k] * s->kT);
  hipLaunchKernelGGL(init_momenta_kernel<R>, dim3(1), dim3(256), 0, st, s->sys->n, R(sd_t), R(sd_r[0]), R(sd_r[1]), R(sd_r[2]), s->seed,
                     (R*)p_lin, (R*)p_ang);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

// mythos_langevin_eval_external_at: the caller's packed centres become the p0 words of a scratch frame with zero momenta,
// the kick kernels of the integrator run on it with c dt = 1 at step count `step`, and the momenta go out as the forces.
// n_energies: kExtEnergies, or 3 for the first three words alone (mythos_langevin_eval_external).
template <typename R>
static int entry_eval_external(mythos_sim* s, const void* center, double step, void* force_out, double* energy_out, int n_energies,
                               hipStream_t st) {
  using V4 = typename Vec4T<R>::type;
  const int n = s->sys->n;
  const int blocks = std::max(1, ext_field_blocks(s->rst));
  const size_t ctl_bytes = MdRun::kCtlWords * sizeof(int) + sizeof(unsigned long long) * (size_t)(1 + blocks);
  if (int rc = s->d_eval_p0.grow(sizeof(V4) * (size_t)n)) return rc;
  if (int rc = s->d_eval_mom.grow(sizeof(V4) * (size_t)n)) return rc;
  if (int rc = s->d_eval_ctl.grow(ctl_bytes)) return rc;
  if (int rc = s->d_eval_group_row.grow((size_t)std::max(1, s->rst.n_groups) * kExtRow)) return rc;
  MYTHOS_HIP_TRY(hipMemsetAsync(s->d_eval_ctl.get(), 0, ctl_bytes, st));
  V4* p0 = (V4*)s->d_eval_p0.get();
  V4* mom = (V4*)s->d_eval_mom.get();
  const int* flags = (const int*)s->d_eval_ctl.get();
  unsigned long long* stamps = (unsigned long long*)((char*)s->d_eval_ctl.get() + MdRun::kCtlWords * sizeof(int));
  static_assert(MdRun::kCtlWords * sizeof(int) % sizeof(unsigned long long) == 0, "the stamps follow the control words aligned");
  hipLaunchKernelGGL(ext_eval_pack_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, st, n, (const R*)center, p0, mom);
  if (s->ext_count > 0)
    hipLaunchKernelGGL(ext_kick_kernel<R>, dim3(1), dim3(256), 0, st, s->ext_count, (const int*)s->d_ext_index.get(),
                       (const V4*)s->d_ext_force.get(), R(1), mom, flags, (const int*)nullptr, 0, 1ull, stamps);
  ExtFieldView v = s->rst;
  v.g_row = s->d_eval_group_row.get();  // (the rows of a resident run are not disturbed)
  if (v.n_entries > 0) launch_ext_field_kick<R>(v, p0, nullptr, 1.0, step, mom, flags, nullptr, 0, 1ull, stamps + 1, st);
  hipLaunchKernelGGL(ext_eval_unpack_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, st, n, (const V4*)mom, (R*)force_out);
  hipLaunchKernelGGL(ext_energy_kernel<R>, dim3(1), dim3(256), 0, st, s->ext_count, (const int*)s->d_ext_index.get(),
                     (const V4*)s->d_ext_force.get(), v, (const V4*)p0, step, n_energies, energy_out);
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

// One precision's entry points as a table; langevin.hip chooses between its own and langevin_f64.hip's by the system's dtype.
struct MdEntries {
  int (*load)(mythos_sim*, void*, void*, void*, void*, hipStream_t);
  int (*advance)(mythos_sim*, int, int, bool, void*, void*, double*, hipStream_t);
  int (*store)(mythos_sim*, void*, void*, void*, void*, hipStream_t);
  int (*init_momenta)(mythos_sim*, void*, void*, hipStream_t);
  int (*eval_external)(mythos_sim*, const void*, double, void*, double*, int, hipStream_t);
};
template <typename R>
constexpr MdEntries md_entries() {
  return {entry_load<R>, entry_advance<R>, entry_store<R>, entry_init_momenta<R>, entry_eval_external<R>};
}
MdEntries md_entries_f64();  // langevin_f64.hip

}  // namespace mythos
