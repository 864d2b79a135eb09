// Wavefront-level helpers shared by the oxDNA and MARTINI kernels.
#ifndef MYTHOS_WAVE_OPS_H
#define MYTHOS_WAVE_OPS_H

#include <hip/hip_runtime.h>

namespace mythos {

// Optimisation barrier on a register value: whatever produced it stays before this point, its uses after.
template <typename T>
__device__ __forceinline__ void pin_vgpr(T& v) {
  asm volatile("" : "+v"(v));
}

// Cross-lane moves inside a 16-lane row as DPP modifiers (full-rate VALU, no trip through the LDS
// crossbar that __shfl's ds_bpermute takes): quad_perm [1,0,3,2] / [2,3,0,1] exchange with lane^1 /
// lane^2, row_half_mirror and row_mirror reflect inside 8 / 16 lanes.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}

// Sum over the G lanes of a group (G <= 16: butterfly in a fixed order, every lane gets the total).
template <int G, typename R>
__device__ __forceinline__ R group_sum(R v) {
  if constexpr (G <= 16) {
    if constexpr (G >= 2) v += dpp_move<0xB1>(v);   // lane ^ 1
    if constexpr (G >= 4) v += dpp_move<0x4E>(v);   // lane ^ 2: quads now hold their sum
    if constexpr (G >= 8) v += dpp_move<0x141>(v);  // row_half_mirror: the other quad of the 8
    if constexpr (G >= 16) v += dpp_move<0x140>(v); // row_mirror: the other half of the 16
  } else {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  }
  return v;
}

// Sum over the workgroup in a fixed order, to every thread: wavefront shuffles, then the wavefronts' totals in order.
// red: shared scratch of blockDim.x / 64 doubles.  Every thread of the workgroup must call it.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}

// The value a given lane holds, as a wave-uniform (v_readlane: no LDS trip); `lane` must be uniform.
__device__ __forceinline__ double read_lane(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}

// Inclusive prefix sum over the G lanes of a group, G = 16 (one DPP row) or 64 (the wavefront), every lane enabled.
// Inside a row: row_shr 1 / 2 / 4 / 8, lanes whose source would lie before the row read 0 (bound_ctrl).  Across the
// four rows of a wavefront: the row totals sit in lanes 15 / 31 / 47 and are added in row order.  The order of the
// additions is fixed, so the result is reproducible.
template <int G, typename R>
__device__ __forceinline__ R group_scan(R v) {
  static_assert(G == 16 || G == 64, "group_scan: one DPP row or one wavefront");
  v += dpp_move<0x111>(v);  // row_shr:1
  v += dpp_move<0x112>(v);  // row_shr:2
  v += dpp_move<0x114>(v);  // row_shr:4
  v += dpp_move<0x118>(v);  // row_shr:8
  if constexpr (G == 64) {
    const R r0 = read_lane(v, 15), r1 = read_lane(v, 31), r2 = read_lane(v, 47);
    const int row = (int)(__lane_id() >> 4);
    const R before = row == 0 ? R(0) : (row == 1 ? r0 : (row == 2 ? r0 + r1 : (r0 + r1) + r2));
    v += before;
  }
  return v;
}

}  // namespace mythos

#endif  // MYTHOS_WAVE_OPS_H
