// Internal definitions shared by the translation units of libmythos_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mythos_hip.h"
#include "device_buf.h"
#include "oxdna_math.h"

namespace mythos {

// (set_error, hip_fail and MYTHOS_HIP_TRY: device_buf.h)
// test / diagnostic switches (mythos_debug_set): process-wide, 0 = default
long long debug_value(int key);
void debug_clear(int key);

// Row entry encoding of the per-nucleotide neighbour rows:
//   slot 0 : bonded partner on the 3' side  (bond (j, self): self plays nn_j)   or -1
//   slot 1 : bonded partner on the 5' side  (bond (self, j): self plays nn_i)   or -1
//   slot 2, 3: a second partner in the nn_j / nn_i role, or -1.  Only the two ends of a circular strand have one:
//           the reference closes a ring with the pair (first, last) in that order (mythos/input/topology.py:178-180),
//           so `first` is nn_i of two bonds and `last` is nn_j of two.  Even slots: self is nn_j; odd: self is nn_i.
//   slot>=4: unbonded neighbour index | ROLE_Q if self plays op_j of the ordered pair
constexpr int ROW_ROLE_Q = 1 << 30;
constexpr int ROW_INDEX_MASK = ROW_ROLE_Q - 1;
constexpr int ROW_BONDED_SLOTS = 4;

template <typename R>
struct BoxT {
  R l[3];
  R il[3];
  int on;
};

// d_overflow words: [0] longest row if over the stride, [1] fullest bucket if over its capacity, [2] fullest bucket if
// over half its capacity (headroom hint, not an error)
constexpr int kOverflowWords = 3;

// The Verlet rows of one system (oxDNA: mythos_system, MARTINI: mythos_martini_sim) and what their builds keep from one
// to the next: the overflow words and the cell table (cell_list.h, which has the host helpers around them).  The row
// lengths stay with each owner: their layouts differ.
struct VerletRows {
  DeviceBuf<int> d_rows;  // [n][stride]
  int stride = 0;
  DeviceBuf<int> d_overflow;  // [kOverflowWords] largest demands seen since last cleared (list_build_until_fit)
  DeviceBuf<int> d_cell;      // cell table (cell_list.h CellBins): counters [2][H], buckets [H][cell_bucket_cap]
  int cell_H = 0;             // table slots of the current layout
  int cell_alloc_bucket_cap = 0;  // places per slot the current layout was made for
  bool cell_sites = false;    // the layout carries the two site streams (cell_list.h CellBins::sites)
  int cell_bucket_cap;        // places per slot (the owner's default, grown by list_build_until_fit)
  int cell_phase = 0;         // which counter half the next build counts into
  explicit VerletRows(int bucket_cap) : cell_bucket_cap(bucket_cap) {}
};

}  // namespace mythos

struct mythos_obs;

struct mythos_system {
  int model = 0;
  int n = 0;
  int dtype = 0;
  int device = 0;
  int n_bonded = 0;
  bool has_box = false;
  double box[3] = {0, 0, 0};

  // topology (device)
  mythos::DeviceBuf<int> d_meta;  // [n] seq | is_end << 2

  // neighbour rows: the rows, their overflow words and cell table (cell buckets start at 32 places; the rows reserve a
  // stride of 64 at first use, rows_build_device)
  mythos::VerletRows list{32};
  mythos::DeviceBuf<int> d_row_len;  // [n] used slots (>= 2) | [2n] bonded partners | [n] end of the "close" segment
  bool nbrs_set = false;
  int list_epoch = 0;  // bumped when parameters or rows are replaced through the ABI (integrators re-validate their list)
  int param_epoch = 0; // bumped when parameters or nucleotide types are replaced (integrators re-derive the site offsets they carry)
  // host copy of the bonded partners, [n][2]
  std::vector<int> h_partners;
  bool extra_bonds = false;  // some nucleotide uses slot 2 or 3 (circular strands)

  // Verlet build scratch of an MD run (neighbors.hip writes it): allocated by reserve_refs, which an integrator's
  // create calls
  mythos::DeviceBytes d_ref_pos;  // [n] real4 positions at the last build (MD displacement check)
  mythos::DeviceBytes d_ref_off;  // [n] real4 backbone offsets at the last build
  mythos::DeviceBytes d_ref_a1;   // [n] real4 base vectors at the last build
  // Candidate store of an MD run (neighbors.hip: rows_wide_build_device fills it, filter_rows_kernel reads it): rows of
  // every unbonded neighbour whose centre lay within list range + margin at the candidate frame, one index-sorted
  // segment each, with their own stride, overflow words and cell table, and the centres they were built from.
  // Allocated at the first wide build.
  mythos::VerletRows cand{32};
  mythos::DeviceBuf<int> d_cand_len;   // [n] used slots | [n] end of the close segment (= used slots: one segment)
  mythos::DeviceBytes d_cand_ref;      // [n] real4 centres at the candidate frame
  bool cand_unfit = false;             // the candidates of this system need longer rows than the builder's LDS holds: no filter
  int reserve_refs() {
    const size_t v4 = (dtype == MYTHOS_F32 ? sizeof(float4) : sizeof(double4)) * (size_t)n;
    for (mythos::DeviceBytes* b : {&d_ref_pos, &d_ref_off, &d_ref_a1})
      if (int rc = b->grow(v4)) return rc;
    return 0;
  }

  // parameters
  bool params_set = false;
  mythos::OxParams<float> pf;
  mythos::OxParams<double> pd;
  // oxNA (model 4): three vectors - oxDNA2 (also in pf / pd), oxRNA2, hybrid - one after the other, host and device
  std::vector<double> pd_sets;
  int param_sets() const { return model == 4 ? 3 : 1; }
  bool types_set = false;  // model 4: mythos_oxdna_set_nucleotide_types has run
  std::vector<int> h_meta;  // seq | is_end << 2 | is_rna << 3, as uploaded to d_meta
  mythos::DeviceBuf<float> d_pf;   // the same vectors in device memory (read by the MD kernel as scalar loads)
  mythos::DeviceBuf<double> d_pd;

  // probabilistic sequence (mythos_oxdna_set_pseq); pseq_terms == 0: discrete sequence
  mythos::DeviceBytes d_ps_marg;  // [n][4] real: marginal base probabilities
  mythos::DeviceBuf<int> d_ps_unit;   // [n] 2 * base pair + member, or -1
  mythos::DeviceBytes d_ps_bp;    // [max(n_bp, 1)][4] real: base-pair type probabilities
  int pseq_terms = 0;         // bit 0 stacking, bit 1 hydrogen bonding
  int ps_n_bp = 0;            // constrained base pairs of the distribution
  double* ps_gmarg = nullptr; // caller's dU/d(marginals) and dU/d(type probabilities) buffers, set for the duration of
  double* ps_gbp = nullptr;   // one mythos_oxdna_energy_dpseq call

  // energy-pass scratch
  mythos::DeviceBuf<double> d_epart;   // [frames_chunk][blocks][8]
  mythos::DeviceBuf<double> d_pgpart;  // [frames_chunk][blocks][OXP_COUNT]
  // temperature-sweep scratch (debye_sweep.hip)
  mythos::DeviceBuf<double> d_sweep_consts;  // [n_kt][5] the caller's constant table
  mythos::DeviceBuf<double> d_sweep_part;    // [frames_chunk][tiles][n_kt_chunk][1 or 6]
  // order-parameter lists of the last mythos_oxdna_order_params call (order_params.hip), kept between calls:
  // [n_pairs][2] pairs, lower index first | [n_ops + 1] op_first | [n_ops] op_kind
  std::vector<int> h_op_list;
  mythos::DeviceBuf<int> d_op_list;

  // the members free themselves, on the system's device
  ~mythos_system() { (void)hipSetDevice(device); }
};

namespace mythos {

template <typename R>
BoxT<R> make_box(const mythos_system* s) {
  BoxT<R> b;
  b.on = s->has_box ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    b.l[k] = R(s->has_box ? s->box[k] : 1.0);
    b.il[k] = R(s->has_box ? 1.0 / s->box[k] : 1.0);
  }
  return b;
}

template <typename R>
const OxParams<R>& params_of(const mythos_system* s);
template <>
inline const OxParams<float>& params_of<float>(const mythos_system* s) { return s->pf; }
template <>
inline const OxParams<double>& params_of<double>(const mythos_system* s) { return s->pd; }
template <typename R>
const R* device_params_of(const mythos_system* s);
template <>
inline const float* device_params_of<float>(const mythos_system* s) { return s->d_pf.get(); }
template <>
inline const double* device_params_of<double>(const mythos_system* s) { return s->d_pd.get(); }

// A run-time model number, or a run-time switch, as the compile-time tag a kernel template takes: f is a generic lambda and
// is called with std::integral_constant<int, M>, M = 1 ... 4 (the entry points checked the range; 2 otherwise), or with
// std::true_type / std::false_type.
template <class F>
auto with_model(int model, F&& f) {
  switch (model) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 2>{});
  }
}
template <class F>
auto with_bool(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}
// A run-time precision (MYTHOS_F32 / MYTHOS_F64; the entry points checked it) as the type a kernel template takes: f is
// called with float{} or double{}.
template <class F>
auto with_real(int dtype, F&& f) {
  return dtype == MYTHOS_F32 ? f(float{}) : f(double{});
}
// The frames of a call in launches of at most `chunk`: f(f0, nf) -> 0 or an error code, which ends the loop.
template <class F>
int for_frame_chunks(int n_frames, int chunk, F&& f) {
  for (int f0 = 0; f0 < n_frames; f0 += chunk)
    if (int rc = f(f0, std::min(chunk, n_frames - f0))) return rc;
  return 0;
}
// frames per launch of the kernels that give a frame one workgroup, blockIdx.x + frame0: far below the grid limit
constexpr int kFramesPerLaunch = 1 << 20;

// d_row_len holds three arrays back to back: row length [n] | bonded partners [n][ROW_BONDED_SLOTS] | end of the
// "close" segment of the row [n]
static_assert(ROW_BONDED_SLOTS == 4, "the row builders copy four partner slots");
inline int* row_close_of(const mythos_system* sys) { return sys->d_row_len.get() + (size_t)(1 + ROW_BONDED_SLOTS) * sys->n; }

// Largest centre-centre distance at which anything other than the backbone-backbone terms (excluded
// volume between base / backbone sites, H-bond, cross- and coaxial stacking) can act.  Rows keep the
// neighbours inside this range (+ skin) in a leading "close" segment so the MD kernel's radial pass
// runs its heavy and its Debye-only code on homogeneous wavefronts.
// One flat vector of the system: the only one, or (oxNA) vector k of oxDNA2, oxRNA2, hybrid.
inline const double* oxdna_param_set(const mythos_system* sys, int k) {
  return sys->param_sets() == 1 ? sys->pd.v : sys->pd_sets.data() + (size_t)k * OXP_COUNT;
}
// max over the system's vectors of one entry, or of a function of a vector
inline double oxdna_param_max(const mythos_system* sys, int idx) {
  double m = oxdna_param_set(sys, 0)[idx];
  for (int k = 1; k < sys->param_sets(); ++k) m = std::max(m, oxdna_param_set(sys, k)[idx]);
  return m;
}

inline double oxdna_close_range(const mythos_system* sys) {
  // (oxNA: ranges from whichever vector is largest, site offsets from whichever geometry reaches farthest)
  double off_back = 0.0, off_base = 0.0, off_stack = 0.0;
  for (int k = 0; k < std::min(sys->param_sets(), 2); ++k) {  // the hybrid vector carries no geometry of its own
    const double* P = oxdna_param_set(sys, k);
    off_back = std::max(off_back, std::sqrt(P[GEO_BACK_A1] * P[GEO_BACK_A1] + (sys->model >= 2 ? P[GEO_BACK_A2] * P[GEO_BACK_A2] : 0.0)));
    off_base = std::max(off_base, std::fabs(P[GEO_BASE]));
    off_stack = std::max(off_stack, std::fabs(P[GEO_STACK]));
  }
  auto mx = [&](int idx) { return oxdna_param_max(sys, idx); };
  double rcom = std::max(mx(NEXC_BACK_BASE_RC), mx(NEXC_BASE_BACK_RC)) + off_back + off_base;
  rcom = std::max(rcom, mx(NEXC_BASE_RC) + 2 * off_base);
  rcom = std::max(rcom, std::max(mx(HYDR_RCHIGH), mx(CRST_RCHIGH)) + 2 * off_base);
  rcom = std::max(rcom, mx(CXST_RCHIGH) + 2 * off_stack);
  return rcom * (1.0 + 1e-6);
}

// oxdna_kernels.hip
int oxdna_energy_launch(mythos_system* sys, const void* center, const void* quat, int n_frames, double* e_terms,
                        void* dU_dcenter, void* dU_dquat, double* dU_dparams, mythos_obs* obs, double* obs_out,
                        hipStream_t stream);
// neighbors.hip
int rows_from_pairs(mythos_system* sys, const int32_t* pairs, int n_pairs);
// backbone_offsets, base_vectors: real4 per nucleotide (MD frames) to select the segments by site distances, or null
// write_refs: also store the positions / backbone offsets / base vectors the list was built from in
// d_ref_pos / d_ref_off / d_ref_a1 (the MD kernel's displacement check compares against them)
int rows_build_device(mythos_system* sys, const void* center, bool center_is_vec4, double r_cut, double skin,
                      const void* backbone_offsets, const void* base_vectors, bool write_refs, hipStream_t stream);
// rows_build_device inside list_build_until_fit (cell_list.h): grows rows and buckets until the build fits, synchronising
int rows_build_until_fit(mythos_system* sys, const void* center, bool center_is_vec4, double r_cut, double skin,
                         const void* backbone_offsets, const void* base_vectors, bool write_refs, bool headroom,
                         hipStream_t stream);
// The candidate rows of an MD run and the rows filtered from them (row_filter_plan.h).  p0, p3, p1: the
// frame's centres, backbone offsets and base vectors, real4 per nucleotide.
// rows_filter_applies: the cell builder would build both the rows and the candidates (cell_grid at either range).
bool rows_filter_applies(const mythos_system* sys, double r_cut, double skin, double margin);
// wide build: the cell builder at r_cut + skin + margin, centre criterion only, into sys->cand
int rows_wide_build_device(mythos_system* sys, const void* p0, double r_cut, double skin, double margin, hipStream_t stream);
// filter: sys->cand -> sys->list at the frame (p0, p3, p1), entry for entry what rows_build_device writes there - or a
// non-zero first overflow word of sys->list, which halts the step launches (stale candidates, rows over a stride)
int rows_filter_device(mythos_system* sys, const void* p0, const void* p3, const void* p1, double r_cut, double skin, double margin,
                       hipStream_t stream);
// wide build until the candidates fit, then filter until the rows fit (synchronising; both with headroom).  Candidate rows
// beyond kCandStrideMax slots (a system far denser than a duplex) set sys->cand_unfit and fail: the caller builds in full
int rows_filter_until_fit(mythos_system* sys, const void* p0, const void* p3, const void* p1, double r_cut, double skin, double margin,
                          hipStream_t stream);

}  // namespace mythos
