// Umbrella sampling on the resident Langevin state (umbrella.hip): what the integrator's handle keeps of a bias, the
// checks of its lists, and the two launches of a segment boundary.  The segment loop itself is the integrator's
// (mythos_langevin_advance_umbrella, langevin.hip).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "device_buf.h"

struct mythos_system;

namespace mythos {

// record row of one (boundary, replica), doubles: [n_ops] proposed values | [n_ops] proposed states | W_old | W_new | u | accept |
// [n_ops] the states the replica holds after the decision
inline int umbrella_record_width(int n_ops) { return 3 * n_ops + 4; }

// The bias of one integrator.  n_ops == 0: none set.
struct UmbrellaState {
  int n_ops = 0, n_pairs = 0, n_rep = 1, n_one = 0, segment_steps = 0;
  double hb_cutoff = -0.1;
  // [n_pairs][2] pairs of ONE replica, lower index first | [n_ops + 1] op_first | [n_ops] op_kind | [n_ops + 1] iface_first |
  // [n_ops] table_shape
  DeviceBuf<int> d_list;
  DeviceBuf<double> d_iface;  // the interfaces of the mindistance parameters, one after the other
  DeviceBuf<double> d_table;  // dense, row-major, one axis per order parameter
  DeviceBuf<double> d_w_cur;  // [n_rep] weight of the state each replica holds
  DeviceBuf<int> d_accept;    // [n_rep] the last decision
  DeviceBuf<int> d_state;     // [n_rep][n_ops] the state each replica holds | [n_rep][n_ops] the last proposal's
  DeviceBuf<unsigned long long> d_counts;  // accepted, decided
  DeviceBuf<int> d_err;       // [1] lowest replica whose initial state has weight 0 (INT_MAX: none)
  DeviceBuf<double> d_prime_rec;  // [n_rep][record width] the record rows of the priming boundary
  DeviceBytes snap[8];        // the snapshot: a frame's eight arrays
  DeviceBytes stage_c, stage_q, stage_p, stage_l;  // the packed state between the store and the load that open a segment
  bool primed = false;        // the snapshot holds the resident state, d_w_cur its weights and d_state its states
  int param_epoch = 0;        // sys->param_epoch the weights held were looked up under
  bool frame_loaded = false;  // the resident frame is what mythos_langevin_load left (nothing has stepped it since)
};

// what the decide launch reads and writes besides the frame
struct UmbrellaView {
  int n_ops, n_pairs, n_rep, n_one;
  double hb_cutoff;
  const int* list;
  const double* iface;
  const double* table;
  double* w_cur;
  int* accept;
  int* state;
  unsigned long long* counts;
  int* err;
};

// The checks of a bias on their own (mythos_umbrella_check, mythos_langevin_set_umbrella): true, or false with
// "<who>: ..." as the error message.  bonded: [n_bonded][2] backbone neighbours, indices of one replica.
bool umbrella_valid(const std::string& who, int n, int n_rep, int model, int n_bonded, const int32_t* bonded, int n_ops,
                    const int32_t* op_kind, const int32_t* op_first, const int32_t* pairs, int n_pairs, const int32_t* iface_first,
                    const double* interfaces, const int32_t* table_shape, const double* table, int segment_steps);

// One workgroup per replica on the frame words (p0, q) of the system's precision: the order parameters of the proposal,
// its weight, the uniform of (replica, step) and the decision.  prime: accept whatever the weight, and name a replica of
// weight 0 in v.err.  record: [n_rep][record width] or null.
int umbrella_decide_launch(const mythos_system* sys, const UmbrellaView& v, const void* p0, const void* q, uint64_t seed, uint64_t step,
                           bool prime, double* record, hipStream_t st);

// One thread per nucleotide: accepted replicas frame -> snapshot, rejected ones snapshot -> frame with the momenta
// negated, in the snapshot as well; then the post-decision packed row (traj_*) and the proposal's (prop_*), each or all null.  frame, snap: the
// eight arrays of a Frame<R> in its order (p0, p1, p2, p3, q, pl, mom, ang).
int umbrella_commit_launch(int dtype, int n, int n_one, void* const* frame, void* const* snap, const int* accept, void* traj_center,
                           void* traj_quat, void* prop_center, void* prop_quat, hipStream_t st);

}  // namespace mythos
