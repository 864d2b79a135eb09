// Umbrella sampling on the resident Langevin state: the two launches of a segment boundary and the checks of a bias.
//
// Replaces the external oxDNA run of the reference's oxDNAUmbrellaSampler (mythos/simulators/oxdna/oxdna.py:225-275; the
// order-parameter and weight columns it reads back, utils.py:348-429) by segment-Metropolis on the integrator: a segment
// of L steps from a closed frame (x, p) is a proposal (x', p'), accepted iff W(s') > 0 and u W(s) < W(s'), s the state of
// the order parameters; a rejected replica goes back to (x, -p).  The Langevin map is reversible with respect to the
// Boltzmann density under momentum reversal up to the integrator's own O(dt^2) error, so the chain leaves
// pi(x, p) W(Q(x)) invariant.  The segment loop is the integrator's (mythos_langevin_advance_umbrella, langevin.hip).
//
// umbrella_decide_kernel: one workgroup per replica reads the frame words (p0.xyz, q) of the replica's nucleotides - the
// values mythos_langevin_store hands out - and evaluates the listed pairs exactly as order_params_kernel does on a
// stored row (same loader arithmetic, same pair functions, same minimum images): the values are bitwise those of
// mythos_oxdna_order_params.  Counts and the ordered-bits minimum are folded with integer adds and minima, in the
// wavefront by shuffles and across the (at most four) wavefronts through LDS in a fixed order; thread 0 forms the table
// index, reads W, draws u from Philox stream 4 of (replica, step) and decides, all in double in both precisions.
// umbrella_commit_kernel: one thread per nucleotide copies the eight frame words frame -> snapshot (accepted) or
// snapshot -> frame with mom and ang negated (rejected; the negated momenta go into the snapshot too - it is the state the
// replica holds), 16-byte accesses consecutive over the lanes, and writes the packed rows.  Neither kernel uses scratch;
// the decide kernel's LDS is eight words written by lane 0 of each wavefront.
#include <climits>
#include <cmath>

#include "mythos_internal.h"
#include "order_param_pair.h"
#include "oxdna_gather.h"
#include "philox.h"
#include "umbrella.h"

namespace mythos {

constexpr int kUmbBlock = 256;

template <typename R, int MODEL>
__global__ __launch_bounds__(kUmbBlock) void umbrella_decide_kernel(const R* __restrict__ Pg, const BoxT<R> box,
                                                                    const typename Vec4T<R>::type* __restrict__ p0,
                                                                    const typename Vec4T<R>::type* __restrict__ qf,
                                                                    const int* __restrict__ meta, const UmbrellaView v, uint64_t seed,
                                                                    uint64_t step, int prime, double* __restrict__ record) {
  static_assert(MODEL >= 1 && MODEL <= 3, "one site geometry per system");
  using Bits = OrderedBits<R>;
  using BitsT = typename Bits::type;
  __shared__ int s_count[kUmbBlock / 64];
  __shared__ BitsT s_near[kUmbBlock / 64];
  const int* __restrict__ pairs = v.list;
  const int* __restrict__ op_first = pairs + 2 * (size_t)v.n_pairs;
  const int* __restrict__ op_kind = op_first + v.n_ops + 1;
  const int* __restrict__ iface_first = op_kind + v.n_ops;
  const int* __restrict__ shape = iface_first + v.n_ops + 1;
  const int rep = blockIdx.x;
  const int base = rep * v.n_one;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
  const int width = 3 * v.n_ops + 4;
  int* __restrict__ held = v.state + (size_t)rep * v.n_ops;                               // the state the replica holds
  int* __restrict__ proposed = v.state + ((size_t)v.n_rep + rep) * v.n_ops;                // the proposal's, for thread 0 below
  double* __restrict__ row = record ? record + (size_t)rep * width : nullptr;

  const ConstParams<R, false> P(Pg);
  const UniGeo<R, MODEL> geo(P);
  const Vec4Loader<R> ld{p0, qf, meta};
  size_t index = 0;      // (thread 0) row-major index of the proposal's state in the table
  bool in_table = true;  // every state so far is on its axis
  for (int op = 0; op < v.n_ops; ++op) {
    const int k0 = op_first[op], k1 = op_first[op + 1];
    const int kind = op_kind[op];
    const bool want_hb = kind == MYTHOS_OP_BOND;
    int count = 0;
    BitsT nearest = ~(BitsT)0;
    for (int k = k0 + (int)threadIdx.x; k < k1; k += blockDim.x) {
      R e_hb, r;
      order_param_pair<R, MODEL>(P, geo, ld, box, base + pairs[2 * k], base + pairs[2 * k + 1], want_hb, e_hb, r);
      order_param_accumulate<R>(e_hb, r, v.hb_cutoff, count, nearest);
    }
    for (int o = 32; o > 0; o >>= 1) {
      count += __shfl_xor(count, o);
      const BitsT other = __shfl_xor(nearest, o);
      nearest = other < nearest ? other : nearest;
    }
    if (lane == 0) s_count[wave] = count, s_near[wave] = nearest;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < n_waves; ++w) {
        count += s_count[w];
        nearest = s_near[w] < nearest ? s_near[w] : nearest;
      }
      double value;
      int state;
      if (kind == MYTHOS_OP_BOND) {
        value = double(count);
        state = count;
      } else {
        value = double(Bits::back(nearest));
        state = 0;
        for (int j = iface_first[op]; j < iface_first[op + 1]; ++j) state += (value > v.iface[j]) ? 1 : 0;
      }
      in_table = in_table && state < shape[op];
      index = index * (size_t)shape[op] + (size_t)state;
      proposed[op] = state;
      if (row) row[op] = value, row[v.n_ops + op] = double(state);
    }
    __syncthreads();  // the words are written again for the next order parameter
  }
  if (threadIdx.x != 0) return;
  uint32_t c[4] = {(uint32_t)rep, uint32_t(step), uint32_t(step >> 32), 4u};
  philox4x32(c, uint32_t(seed), uint32_t(seed >> 32));
  const double u = (double(c[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32: (0, 1)
  const double w_new = in_table ? v.table[index] : 0.0;
  const double w_old = prime ? w_new : v.w_cur[rep];
  int acc;
  if (prime) {
    acc = 1;
    if (!(w_new > 0.0)) atomicMin(v.err, rep);
  } else {
    const double lhs = u * w_old;
    acc = (w_new > 0.0 && lhs < w_new) ? 1 : 0;
    atomicAdd(v.counts + 1, 1ull);
    if (acc) atomicAdd(v.counts, 1ull);
  }
  if (acc) v.w_cur[rep] = w_new;
  v.accept[rep] = acc;
  for (int op = 0; op < v.n_ops; ++op) {  // (thread 0 wrote `proposed` itself)
    const int now = acc ? proposed[op] : held[op];
    held[op] = now;
    if (row) row[2 * v.n_ops + 4 + op] = double(now);
  }
  if (row) row[2 * v.n_ops] = w_old, row[2 * v.n_ops + 1] = w_new, row[2 * v.n_ops + 2] = u, row[2 * v.n_ops + 3] = double(acc);
}

// the eight arrays of a frame, in Frame<R>'s order (langevin_step.h)
template <typename R>
struct FrameWords {
  typename Vec4T<R>::type* w[8];
};
constexpr int kWordP0 = 0, kWordQ = 4, kWordPl = 5, kWordMom = 6;

template <typename R>
__global__ __launch_bounds__(256) void umbrella_commit_kernel(int n, int n_one, const FrameWords<R> f, const FrameWords<R> s,
                                                              const int* __restrict__ accept, R* __restrict__ traj_c, R* __restrict__ traj_q,
                                                              R* __restrict__ prop_c, R* __restrict__ prop_q) {
  using V4 = typename Vec4T<R>::type;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool acc = accept[i / n_one] != 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    if (w == kWordPl && sizeof(R) != 4) continue;  // (the low parts of the centres exist in fp32 frames alone)
    V4 now = f.w[w][i];
    if (w == kWordP0 && prop_c) prop_c[3 * (size_t)i] = now.x, prop_c[3 * (size_t)i + 1] = now.y, prop_c[3 * (size_t)i + 2] = now.z;
    if (w == kWordQ && prop_q) reinterpret_cast<V4*>(prop_q)[i] = now;
    if (acc) {
      s.w[w][i] = now;
    } else {
      now = s.w[w][i];
      if (w >= kWordMom) {  // the state the replica holds from here on is (x, -p): the snapshot follows, so a second rejection in a row gives (x, p)
        now.x = -now.x, now.y = -now.y, now.z = -now.z;
        s.w[w][i] = now;
      }
      f.w[w][i] = now;
    }
    if (w == kWordP0 && traj_c) traj_c[3 * (size_t)i] = now.x, traj_c[3 * (size_t)i + 1] = now.y, traj_c[3 * (size_t)i + 2] = now.z;
    if (w == kWordQ && traj_q) reinterpret_cast<V4*>(traj_q)[i] = now;
  }
}

int umbrella_decide_launch(const mythos_system* sys, const UmbrellaView& v, const void* p0, const void* q, uint64_t seed, uint64_t step,
                           bool prime, double* record, hipStream_t st) {
  const int block = v.n_pairs <= 64 ? 64 : kUmbBlock;
  return with_model(sys->model, [&](auto m) {
    constexpr int M = decltype(m)::value == 4 ? 2 : decltype(m)::value;  // (model 4 is refused when the bias is set)
    return with_real(sys->dtype, [&](auto r) {
      using R = decltype(r);
      using V4 = typename Vec4T<R>::type;
      hipLaunchKernelGGL((umbrella_decide_kernel<R, M>), dim3((unsigned int)v.n_rep), dim3(block), 0, st, device_params_of<R>(sys),
                         make_box<R>(sys), (const V4*)p0, (const V4*)q, (const int*)sys->d_meta.get(), v, seed, step, prime ? 1 : 0, record);
      MYTHOS_HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

int umbrella_commit_launch(int dtype, int n, int n_one, void* const* frame, void* const* snap, const int* accept, void* traj_center,
                           void* traj_quat, void* prop_center, void* prop_quat, hipStream_t st) {
  return with_real(dtype, [&](auto r) {
    using R = decltype(r);
    using V4 = typename Vec4T<R>::type;
    FrameWords<R> f, s;
    for (int w = 0; w < 8; ++w) f.w[w] = (V4*)frame[w], s.w[w] = (V4*)snap[w];
    hipLaunchKernelGGL(umbrella_commit_kernel<R>, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, st, n, n_one, f, s, accept,
                       (R*)traj_center, (R*)traj_quat, (R*)prop_center, (R*)prop_quat);
    MYTHOS_HIP_TRY(hipGetLastError());
    return 0;
  });
}

bool umbrella_valid(const std::string& who, int n, int n_rep, int model, int n_bonded, const int32_t* bonded, int n_ops,
                    const int32_t* op_kind, const int32_t* op_first, const int32_t* pairs, int n_pairs, const int32_t* iface_first,
                    const double* interfaces, const int32_t* table_shape, const double* table, int segment_steps) {
  auto refuse = [&](const std::string& why) {
    set_error(who + ": " + why);
    return false;
  };
  if (n <= 0 || n_rep < 1 || n_ops < 1 || n_pairs < 1 || n_bonded < 0 || !op_kind || !op_first || !pairs || !iface_first || !table_shape ||
      !table || (n_bonded > 0 && !bonded))
    return refuse("invalid argument");
  if (model == 4)
    return refuse("an oxNA system (model 4) has three hydrogen-bonding parameter sets and two site geometries; the order "
                  "parameters are built for oxDNA1, oxDNA2 and oxRNA2");
  if (model < 1 || model > 4) return refuse("model must be 1 (oxDNA1), 2 (oxDNA2) or 3 (oxRNA2)");
  if (n % n_rep != 0) return refuse(std::to_string(n) + " nucleotides are not " + std::to_string(n_rep) + " replicas of one system");
  if (segment_steps < 1) return refuse("segment_steps must be at least 1 (a segment is a proposal of that many steps)");
  const int n_one = n / n_rep;
  if (op_first[0] != 0 || op_first[n_ops] != n_pairs) return refuse("op_first must start at 0 and end at n_pairs");
  if (iface_first[0] != 0) return refuse("iface_first must start at 0");
  size_t cells = 1;
  for (int k = 0; k < n_ops; ++k) {
    if (op_kind[k] != MYTHOS_OP_BOND && op_kind[k] != MYTHOS_OP_MINDISTANCE) return refuse("op_kind must be 0 (bond) or 1 (mindistance)");
    if (op_first[k + 1] <= op_first[k])
      return refuse("order parameter " + std::to_string(k) + " has an empty slice of pairs (op_first must increase)");
    const int n_if = iface_first[k + 1] - iface_first[k];
    if (n_if < 0) return refuse("iface_first must not decrease");
    if (n_if > 0 && !interfaces) return refuse("invalid argument");
    if (op_kind[k] == MYTHOS_OP_BOND && n_if != 0) return refuse("a bond order parameter has no interfaces");
    for (int j = iface_first[k]; j < iface_first[k + 1]; ++j)
      if (!std::isfinite(interfaces[j])) return refuse("an interface is not finite");
    const int reachable = (op_kind[k] == MYTHOS_OP_BOND ? op_first[k + 1] - op_first[k] : n_if) + 1;
    if (table_shape[k] < reachable)
      return refuse("axis " + std::to_string(k) + " of the weights table holds " + std::to_string(table_shape[k]) + " states; order parameter " +
                    std::to_string(k) + " reaches " + std::to_string(reachable) + " (a missing row is given as weight 0, not left out)");
    cells *= (size_t)table_shape[k];
    if (cells > (size_t)1 << 28) return refuse("the weights table has more than 2^28 entries");
  }
  for (int k = 0; k < n_pairs; ++k) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || b < 0 || a >= n_one || b >= n_one || a == b)
      return refuse("pair " + std::to_string(k) + " names a nucleotide outside one replica [0, " + std::to_string(n_one) +
                    "), or one nucleotide twice");
    for (int e = 0; e < n_bonded; ++e)
      if ((bonded[2 * e] == a && bonded[2 * e + 1] == b) || (bonded[2 * e] == b && bonded[2 * e + 1] == a))
        return refuse("pair " + std::to_string(k) + " (" + std::to_string(a) + ", " + std::to_string(b) +
                      ") lists backbone neighbours: oxDNA evaluates no hydrogen bond between them");
  }
  bool any = false;
  for (size_t c = 0; c < cells; ++c) {
    if (!std::isfinite(table[c]) || table[c] < 0)
      return refuse("weight " + std::to_string(c) + " of the table is negative or not finite (a state that must not be visited has weight 0)");
    any = any || table[c] > 0;
  }
  if (!any) return refuse("every weight of the table is 0");
  return true;
}

}  // namespace mythos

using namespace mythos;

extern "C" int mythos_umbrella_check(int n, int n_rep, int model, int n_bonded, const int32_t* bonded, int n_ops, const int32_t* op_kind,
                                     const int32_t* op_first, const int32_t* pairs, int n_pairs, const int32_t* iface_first,
                                     const double* interfaces, const int32_t* table_shape, const double* table, int segment_steps) {
  return umbrella_valid("mythos_umbrella_check", n, n_rep, model, n_bonded, bonded, n_ops, op_kind, op_first, pairs, n_pairs, iface_first,
                        interfaces, table_shape, table, segment_steps)
             ? MYTHOS_OK
             : MYTHOS_ERR_INVALID_ARGUMENT;
}
