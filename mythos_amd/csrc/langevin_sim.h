// The oxDNA Langevin integrator's handle, struct mythos_sim, and the host helpers that only read it: the constants, the
// cut-offs and the frames a launch is given.  Reached through langevin_unfused.inc, which defines the one member type
// that is not the driver's or a buffer (UnfusedState) in front of its include of this file.
#pragma once
#ifndef MYTHOS_UNFUSED_STATE_DEFINED
#error "langevin_sim.h needs UnfusedState: include langevin_unfused.inc (or langevin_core.inc), which defines it and then includes this file"
#endif
#include <cmath>
#include <vector>

#include "ext_field.h"
#include "langevin_step.h"
#include "md_driver.h"
#include "row_filter_plan.h"
#include "umbrella.h"

struct mythos_sim : mythos::MdRun {
  mythos_system* sys = nullptr;
  int device = 0;  // the system's, copied at create: the integrator may outlive its system, to be destroyed only
  double dt = 0, kT = 0, gamma_t = 0, gamma_r = 0, mass = 1, inertia[3] = {1, 1, 1};
  // neighbour policy (MdRun::rebuild_every: 0 = the system's static rows)
  double r_cut = 0, skin = 0;
  // device state: two ping-pong frames of 8 vec4 arrays each (p0, p1, p2, p3, q, pl, mom, ang)
  static constexpr int kFrameArrays = 8;
  mythos::DeviceBytes frame[2][kFrameArrays];
  int builds = 0;          // scheduled rebuilds so far (the chunk order is refreshed every 64th)
  int list_epoch = 0;      // sys->list_epoch the rows in use belong to
  mythos::CandState cand;  // the candidate rows behind the scheduled rebuilds (row_filter_plan.h); carries over like since_build
  // centres as the last run handed them out (hi) and the low parts that went with them (fp32 systems)
  mythos::DeviceBytes keep_hi, keep_lo;
  bool keep_valid = false;
  bool items_big = false;              // the ITEMS = 32 instantiation is in use (a launch of this load found 16 too few)
  int param_epoch = 0;                 // sys->param_epoch the packed site offsets of the resident frames were derived from
  int lanes = mythos::kMdG;      // lanes per nucleotide of the step launches of this load (8, or 16 for small systems: md_lanes_for)
  mythos::DeviceBuf<int> d_chunk_order;  // [blocks] spatial order of the workgroups' chunks of nucleotides (null: index order)
  mythos::DeviceBuf<unsigned long long> d_chunk_keys;
  mythos::DeviceBuf<double> d_epart;     // [blocks][kTraceWidth] energy-trace partials of a saving launch
  mythos::UnfusedState unfused;  // oxNA (model 4): the cross-check path's switch and its own buffers (langevin_unfused.inc)
  // constant external forces (mythos_langevin_set_external_forces), in the system's precision
  int ext_count = 0;
  mythos::DeviceBuf<int> d_ext_index;                  // [ext_count] distinct nucleotides
  mythos::DeviceBytes d_ext_force;                     // [ext_count] Vec4T<R>: (F, 0)
  mythos::DeviceBuf<unsigned long long> d_ext_stamp;   // [1] the last kick applied (ext_kick_kernel)
  bool ext_stamp_stale = true;                 // load / set_step / set_external_forces: cleared in front of the next kick
  // position-dependent external forces (mythos_langevin_set_restraints; ext_field.h), held in double in both precisions
  mythos::ExtFieldView rst;                            // the counts and the device arrays below (all zero / null: none set)
  mythos::DeviceBuf<int> d_rst_t_index, d_rst_t_mask, d_rst_g_kind, d_rst_g_first, d_rst_g_member, d_rst_g_mask;
  mythos::DeviceBuf<int> d_rst_e_index, d_rst_e_first, d_rst_e_term;
  mythos::DeviceBuf<double> d_rst_t_k, d_rst_t_anchor, d_rst_g_vec, d_rst_g_target, d_rst_g_row;
  mythos::DeviceBuf<unsigned long long> d_rst_stamp;   // [workgroups of ext_field_kick_kernel] each one's last kick applied
  bool rst_stamp_stale = true;                         // as ext_stamp_stale, for d_rst_stamp
  // point terms (mythos_langevin_set_point_forces), the other half of `rst`: sorted by nucleotide, in the order given
  mythos::DeviceBuf<int> d_pt_first, d_pt_kind, d_pt_particle, d_pt_ref, d_pt_flags;
  mythos::DeviceBuf<double> d_pt_param;
  // The two sets are set and cleared independently and share the entries of `rst`: the host keeps what each contributes
  // - the restraints' entries (index, term range, terms) and the point terms' nucleotides - and merges them when either
  // changes (ext_entries_merge, langevin.hip).
  std::vector<int> h_rst_index, h_rst_first{0}, h_rst_term, h_pt_particle;
  bool pt_moving = false;  // a point term has rate != 0: its force depends on the step count
  // umbrella sampling (mythos_langevin_set_umbrella; umbrella.h): the bias, the snapshot and the decisions' words
  mythos::UmbrellaState umb;
  // scratch of mythos_langevin_eval_external: p0 and momentum words, zeroed control words and stamps
  mythos::DeviceBytes d_eval_p0, d_eval_mom, d_eval_ctl;
  mythos::DeviceBuf<double> d_eval_group_row;
  ~mythos_sim() { (void)hipSetDevice(device); }  // the members, MdRun's too, free themselves on that device
};

namespace mythos {

template <typename R>
static LangevinConst<R> make_const(const mythos_sim* s) {
  LangevinConst<R> K;
  K.dt = R(s->dt);
  K.half_dt = R(0.5 * s->dt);
  K.inv_mass = R(1.0 / s->mass);
  const double c1t = std::exp(-s->gamma_t * s->dt), c1r = std::exp(-s->gamma_r * s->dt);
  K.c1_t = R(c1t);
  K.c2_t = R(std::sqrt(s->kT * (1.0 - c1t * c1t) * s->mass));
  K.c1_r = R(c1r);
  for (int k = 0; k < 3; ++k) {
    K.inv_inertia[k] = R(1.0 / s->inertia[k]);
    K.c2_r[k] = R(std::sqrt(s->kT * (1.0 - c1r * c1r) * s->inertia[k]));
  }
  K.skin_half_sq = R(s->rebuild_every > 0 ? 0.25 * s->skin * s->skin : -1.0);
  return K;
}

template <typename R>
static MdCut<R> make_cut(const mythos_system* sys) {
  const OxParams<double>& P = sys->pd;
  // (oxNA: rbb2 and rcom2 - the coarse tests - cover all three vectors; the kernel derives the supports of each vector itself)
  double rbb = oxdna_param_max(sys, NEXC_BACKBONE_RC);
  if (sys->model >= 2) rbb = std::max(rbb, oxdna_param_max(sys, DH_RCUT));
  const double rcom = oxdna_close_range(sys);
  MdCut<R> c;
  c.rbb2 = R(rbb * rbb);
  c.rcom2 = R(rcom * rcom);
  auto sq = [](double v) { return R(v * v); };
  c.hb_lo2 = sq(P[HYDR_RCLOW]), c.hb_hi2 = sq(P[HYDR_RCHIGH]);
  c.cr_lo2 = sq(P[CRST_RCLOW]), c.cr_hi2 = sq(P[CRST_RCHIGH]);
  c.cx_lo2 = sq(P[CXST_RCLOW]), c.cx_hi2 = sq(P[CXST_RCHIGH]);
  c.hb_mask = 0;
  for (int k = 0; k < 16; ++k)
    if (P[HYDR_EPS_00 + k] != 0.0) c.hb_mask |= 1u << k;
  return c;
}

template <typename R>
static Frame<R> frame_of(const mythos_sim* sim, int k) {
  using V4 = typename Vec4T<R>::type;
  auto a = [&](int i) { return (V4*)sim->frame[k][i].get(); };
  return Frame<R>{a(0), a(1), a(2), a(3), a(4), a(5), a(6), a(7)};
}

}  // namespace mythos
