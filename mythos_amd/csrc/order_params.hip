// oxDNA's `bond` and `mindistance` order parameters of stored frames: the kernel behind mythos_oxdna_order_params().
//
// Replaces what an oxDNA umbrella-sampling run writes into its energy file per configuration (the order-parameter
// columns the reference reads back, mythos/simulators/oxdna/utils.py:348-384) for the two kinds every order-parameter
// file of the reference uses:
//   bond         the number of listed pairs whose hydrogen-bonding energy is below hb_cutoff (oxDNA's HB_CUTOFF, -0.1;
//                the comparison is strict);
//   mindistance  the smallest minimum-image distance between the base (hydrogen-bonding) sites of the listed pairs.
// The H-bond energy is the energy kernel's: unbonded_angular_geo with TERMS = 1 (oxdna_pair.h), no gradients, on the
// system's flat parameters, sequence weights, box and precision.  A pair is evaluated once, from its lower index in
// role p (the reference's i < j pairs), with its full weight - a row entry of the energy kernel carries half.
//
// Layout: a group of G lanes owns one (frame, order parameter); G is the power of two that covers the longest slice,
// 64 at most, so a wavefront holds 64 / G groups and the 6 - 12 pairs per frame of a melting run fill its lanes with
// several frames.  The lanes of a group stride over the slice; each keeps an integer count and the smallest distance
// as its bit pattern (a non-negative IEEE number orders as an unsigned integer), and the group folds both with
// integer adds and minima: the result does not depend on the order and is reproducible bit for bit.  No atomics, no
// LDS, no second launch; where a slice of op_first begins or ends never matters, since no group sees another's pairs.
#include "mythos_internal.h"
#include "order_param_pair.h"
#include "oxdna_gather.h"

namespace mythos {

constexpr int kOpBlock = 256;
constexpr int kOpFramesPerLaunch = 65535;  // frames per launch, as the energy entry points split theirs

// list: [n_pairs][2] pairs, lower index first | [n_ops + 1] op_first | [n_ops] op_kind
template <typename R, int MODEL>
__global__ __launch_bounds__(kOpBlock) void order_params_kernel(
    const R* __restrict__ Pg, const BoxT<R> box, int n, const R* __restrict__ center, const R* __restrict__ quat,
    const int* __restrict__ meta, const int* __restrict__ list, int n_pairs, int n_ops, int n_frames, int g_log2, double hb_cutoff,
    double* __restrict__ op_out, double* __restrict__ hb_out, double* __restrict__ dist_out) {
  static_assert(MODEL >= 1 && MODEL <= 3, "one site geometry per system");
  using Bits = OrderedBits<R>;
  const int* __restrict__ pairs = list;
  const int* __restrict__ op_first = list + 2 * (size_t)n_pairs;
  const int* __restrict__ op_kind = op_first + n_ops + 1;
  const int G = 1 << g_log2;
  const int lane = threadIdx.x & (G - 1);
  const long long gid = ((long long)blockIdx.x * kOpBlock + threadIdx.x) >> g_log2;
  const bool live = gid < (long long)n_frames * n_ops;
  const int frame = live ? (int)(gid / n_ops) : 0;
  const int op = live ? (int)(gid % n_ops) : 0;
  const int k0 = op_first[op];
  const int k1 = live ? op_first[op + 1] : k0;  // (a group past the end walks nothing and still takes part in the folds)
  const int kind = op_kind[op];
  const bool want_hb = kind == MYTHOS_OP_BOND || hb_out != nullptr;

  const ConstParams<R, false> P(Pg);
  const UniGeo<R, MODEL> geo(P);
  const size_t fo = (size_t)frame * n;
  const PackedLoader<R> ld{center + fo * 3, quat + fo * 4, meta};
  int count = 0;
  typename Bits::type nearest = ~(typename Bits::type)0;
  for (int k = k0 + lane; k < k1; k += G) {
    R e_hb, r;
    order_param_pair<R, MODEL>(P, geo, ld, box, pairs[2 * k], pairs[2 * k + 1], want_hb, e_hb, r);
    order_param_accumulate<R>(e_hb, r, hb_cutoff, count, nearest);
    const size_t at = (size_t)frame * n_pairs + k;
    if (hb_out) hb_out[at] = double(e_hb);
    if (dist_out) dist_out[at] = double(r);
  }
  for (int o = G >> 1; o > 0; o >>= 1) {
    count += __shfl_xor(count, o);
    const typename Bits::type other = __shfl_xor(nearest, o);
    nearest = other < nearest ? other : nearest;
  }
  if (live && lane == 0) op_out[gid] = kind == MYTHOS_OP_BOND ? double(count) : double(Bits::back(nearest));
}

template <typename R, int MODEL>
static int order_params_typed(mythos_system* sys, const R* center, const R* quat, int n_frames, int n_ops, int n_pairs, int g_log2,
                              double hb_cutoff, double* op_out, double* hb_out, double* dist_out, hipStream_t stream) {
  const int n = sys->n;
  const BoxT<R> box = make_box<R>(sys);
  const size_t groups_per_block = (size_t)kOpBlock >> g_log2;
  // frames per launch: the chunk of the energy entry points, fewer where that many would be more blocks than a grid takes
  const int chunk = (int)std::min<size_t>(kOpFramesPerLaunch, std::max<size_t>(1, (size_t(0x7fffffff) * groups_per_block) / (size_t)n_ops));
  return for_frame_chunks(n_frames, chunk, [&](int f0, int nf) {
    const size_t blocks = ((size_t)nf * n_ops + groups_per_block - 1) / groups_per_block;
    hipLaunchKernelGGL((order_params_kernel<R, MODEL>), dim3((unsigned int)blocks), dim3(kOpBlock), 0, stream, device_params_of<R>(sys),
                       box, n, center + (size_t)f0 * n * 3, quat + (size_t)f0 * n * 4, sys->d_meta.get(), sys->d_op_list.get(), n_pairs,
                       n_ops, nf, g_log2, hb_cutoff, op_out + (size_t)f0 * n_ops, hb_out ? hb_out + (size_t)f0 * n_pairs : nullptr,
                       dist_out ? dist_out + (size_t)f0 * n_pairs : nullptr);
    MYTHOS_HIP_TRY(hipGetLastError());
    return 0;
  });
}

}  // namespace mythos

using namespace mythos;

extern "C" int mythos_oxdna_order_params(mythos_system_t* s, const void* center, const void* quat, int n_frames, int n_ops,
                                         const int32_t* op_kind, const int32_t* op_first, const int32_t* pairs, int n_pairs,
                                         double hb_cutoff, double* op_out, double* hb_out, double* dist_out, mythos_stream_t stream) {
  const char* who = "mythos_oxdna_order_params: ";
  auto refuse = [&](const std::string& why) {
    set_error(who + why);
    return (int)MYTHOS_ERR_INVALID_ARGUMENT;
  };
  if (!s || n_frames < 0 || n_ops < 0 || n_pairs < 0) return refuse("invalid argument");
  if (n_frames > 0 && n_ops > 0 && (!center || !quat || !op_kind || !op_first || !pairs || !op_out)) return refuse("invalid argument");
  if (s->model == 4)
    return refuse("an oxNA system has three hydrogen-bonding parameter sets and two site geometries; the order parameters are "
                  "built for oxDNA1, oxDNA2 and oxRNA2");
  if (s->pseq_terms != 0)
    return refuse("the system carries a probabilistic sequence (mythos_oxdna_set_pseq): an expected hydrogen-bonding energy "
                  "below the cutoff is not oxDNA's order parameter");
  if (!s->params_set) {
    set_error(std::string(who) + "parameters must be set first");
    return MYTHOS_ERR_NOT_READY;
  }
  if (n_frames == 0 || n_ops == 0) return MYTHOS_OK;  // an empty batch or list (its buffers may be null) is not an error
  if (!std::isfinite(hb_cutoff)) return refuse("hb_cutoff is not finite");
  // the lists, checked: every index the kernel forms from them is inside its array
  if (op_first[0] != 0 || op_first[n_ops] != n_pairs) return refuse("op_first must start at 0 and end at n_pairs");
  int longest = 0;
  for (int k = 0; k < n_ops; ++k) {
    if (op_kind[k] != MYTHOS_OP_BOND && op_kind[k] != MYTHOS_OP_MINDISTANCE) return refuse("op_kind must be 0 (bond) or 1 (mindistance)");
    if (op_first[k + 1] <= op_first[k]) return refuse("an order parameter without pairs (op_first must increase)");
    longest = std::max(longest, op_first[k + 1] - op_first[k]);
  }
  std::vector<int> packed((size_t)2 * n_pairs + 2 * (size_t)n_ops + 1);
  for (int k = 0; k < n_pairs; ++k) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || b < 0 || a >= s->n || b >= s->n || a == b) return refuse("a pair names a nucleotide outside the system, or one nucleotide twice");
    packed[2 * (size_t)k] = std::min(a, b), packed[2 * (size_t)k + 1] = std::max(a, b);
  }
  std::copy(op_first, op_first + n_ops + 1, packed.begin() + 2 * (size_t)n_pairs);
  std::copy(op_kind, op_kind + n_ops, packed.begin() + 2 * (size_t)n_pairs + n_ops + 1);
  int g_log2 = 0;
  while ((1 << g_log2) < std::min(longest, 64)) ++g_log2;

  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  // The lists stay on the device between calls; a call with other lists waits for the launches that still read the old ones.
  if (packed != s->h_op_list) {
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
    if (int rc = s->d_op_list.grow(packed.size())) return rc;
    MYTHOS_HIP_TRY(hipMemcpy(s->d_op_list.get(), packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice));
    s->h_op_list.swap(packed);
  }
  return with_model(s->model, [&](auto m) {
    constexpr int M = decltype(m)::value == 4 ? 2 : decltype(m)::value;  // (model 4 was refused above)
    return with_real(s->dtype, [&](auto r) {
      using R = decltype(r);
      return order_params_typed<R, M>(s, (const R*)center, (const R*)quat, n_frames, n_ops, n_pairs, g_log2, hb_cutoff, op_out, hb_out,
                                      dist_out, st);
    });
  });
}
