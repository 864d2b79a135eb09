// The small kernels around the frames of the oxDNA Langevin integrator (Frame<R>, langevin_step.h): the caller's packed
// (N,3) / (N,4) arrays to a frame and back, the frame's derived words again after a parameter change, Maxwell-Boltzmann
// momenta, and the kick of the constant external forces.
#pragma once
#include "langevin_step.h"

namespace mythos {

// ------------------------------------------------------------------ packed (N,3)/(N,4) <-> frame
// BX: the axis of the second backbone coefficient (2: a2, 3: a3), or 0 = by the nucleotide's type (oxNA: g_* for DNA on
// a1 / a2, r_* for RNA on a1 / a3)
template <typename R, int BX>
__global__ void pack_state_kernel(int n, R g_k1, R g_k2, R r_k1, R r_k2, const R* __restrict__ c, const R* __restrict__ q,
                                  const R* __restrict__ p, const R* __restrict__ l, const int* __restrict__ meta,
                                  const Frame<R> f, const R* __restrict__ keep_hi, const R* __restrict__ keep_lo) {
  using V4 = typename Vec4T<R>::type;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (kHiLo<R>) {
    // the caller holds fp32 centres; where they are still the values the last run handed out, the low parts that
    // run kept are restored, so a trajectory advanced in several run() calls loses nothing at the seams
    R lo[3] = {R(0), R(0), R(0)};
    if (keep_hi) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (c[3 * i + k] == keep_hi[3 * i + k]) lo[k] = keep_lo[3 * i + k];
    }
    f.pl[i] = V4{lo[0], lo[1], lo[2], R(0)};
  }
  // the kernels assume unit quaternions (torque form); normalise on entry
  R q0 = q[4 * i], q1 = q[4 * i + 1], q2 = q[4 * i + 2], q3 = q[4 * i + 3];
  const R inv = m_rsqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 *= inv, q1 *= inv, q2 *= inv, q3 *= inv;
  V3<R> a1, a2, a3;
  quat_axes(q0, q1, q2, q3, a1, a2, a3);
  f.p0[i] = V4{c[3 * i], c[3 * i + 1], c[3 * i + 2], R(meta[i])};
  f.p1[i] = V4{a1.x, a1.y, a1.z, R(0)};
  f.p2[i] = V4{a3.x, a3.y, a3.z, R(0)};
  const bool rna = BX == 0 && ((meta[i] >> 3) & 1);
  const V3<R> ab = (BX == 3 || rna) ? a3 : a2;  // second axis of the backbone site
  const R k1 = rna ? r_k1 : g_k1, k2 = rna ? r_k2 : g_k2;
  f.p3[i] = V4{k1 * a1.x + k2 * ab.x, k1 * a1.y + k2 * ab.y, k1 * a1.z + k2 * ab.z, R(0)};
  f.q[i] = V4{q0, q1, q2, q3};
  f.mom[i] = V4{p[3 * i], p[3 * i + 1], p[3 * i + 2], R(0)};
  f.ang[i] = V4{l[3 * i], l[3 * i + 1], l[3 * i + 2], R(0)};
}
template <typename R>
__global__ void unpack_state_kernel(int n, const Frame<R> f, R* __restrict__ c, R* __restrict__ q,
                                    R* __restrict__ p, R* __restrict__ l, R* __restrict__ keep_hi,
                                    R* __restrict__ keep_lo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const auto a = f.p0[i];
  if constexpr (kHiLo<R>) {
    const auto lo = f.pl[i];
    keep_hi[3 * i] = a.x, keep_hi[3 * i + 1] = a.y, keep_hi[3 * i + 2] = a.z;
    keep_lo[3 * i] = lo.x, keep_lo[3 * i + 1] = lo.y, keep_lo[3 * i + 2] = lo.z;
  }
  const auto b = f.q[i];
  const auto m = f.mom[i];
  const auto w = f.ang[i];
  c[3 * i] = a.x, c[3 * i + 1] = a.y, c[3 * i + 2] = a.z;
  q[4 * i] = b.x, q[4 * i + 1] = b.y, q[4 * i + 2] = b.z, q[4 * i + 3] = b.w;
  p[3 * i] = m.x, p[3 * i + 1] = m.y, p[3 * i + 2] = m.z;
  l[3 * i] = w.x, l[3 * i + 1] = w.y, l[3 * i + 2] = w.z;
}

// Parameters (site geometry) or nucleotide types were replaced while a state is resident: the words of the frame that
// were derived from them - the meta word and the backbone offset - are derived again from the quaternion.
template <typename R, int BX>
__global__ void rederive_frame_kernel(int n, R g_k1, R g_k2, R r_k1, R r_k2, const int* __restrict__ meta, const Frame<R> f) {
  using V4 = typename Vec4T<R>::type;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V4 q = f.q[i];
  V3<R> a1, a2, a3;
  quat_axes(q.x, q.y, q.z, q.w, a1, a2, a3);
  V4 c = f.p0[i];
  c.w = R(meta[i]);
  f.p0[i] = c;
  const bool rna = BX == 0 && ((meta[i] >> 3) & 1);
  const V3<R> ab = (BX == 3 || rna) ? a3 : a2;
  const R k1 = rna ? r_k1 : g_k1, k2 = rna ? r_k2 : g_k2;
  f.p3[i] = V4{k1 * a1.x + k2 * ab.x, k1 * a1.y + k2 * ab.y, k1 * a1.z + k2 * ab.z, R(0)};
}

// Maxwell-Boltzmann momenta; the centre-of-mass momentum is removed (jax_md initialize_momenta
// with center_velocity=True).  Single block: n is at most a few 10^4 and this runs once.
template <typename R>
__global__ void init_momenta_kernel(int n, R sd_t, R sd_r0, R sd_r1, R sd_r2, uint64_t seed, R* __restrict__ p,
                                    R* __restrict__ l) {
  __shared__ double sum[3][256];
  double s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    R z[6];
    normals6(seed, (uint32_t)i, 0xFFFFFFFFFFFFFFFFull, 7u, z);
    p[3 * i] = sd_t * z[0], p[3 * i + 1] = sd_t * z[1], p[3 * i + 2] = sd_t * z[2];
    l[3 * i] = sd_r0 * z[3], l[3 * i + 1] = sd_r1 * z[4], l[3 * i + 2] = sd_r2 * z[5];
    s0 += p[3 * i], s1 += p[3 * i + 1], s2 += p[3 * i + 2];
  }
  sum[0][threadIdx.x] = s0, sum[1][threadIdx.x] = s1, sum[2][threadIdx.x] = s2;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 3; ++k) sum[k][threadIdx.x] += sum[k][threadIdx.x + o];
    __syncthreads();
  }
  const R m0 = R(sum[0][0] / n), m1 = R(sum[1][0] / n), m2 = R(sum[2][0] / n);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    p[3 * i] -= m0, p[3 * i + 1] -= m1, p[3 * i + 2] -= m2;
  }
}

// Constant external forces (mythos_langevin_set_external_forces; oxDNA's `string` force with rate = 0): the kick
// p_i += c dt F_ext,i on the frame step launch k is about to read, c = kick_close + do_step / 2 - the multiple of dt F
// that launch applies itself.  A kick by a constant force commutes with the kick by the interaction force (both translate
// momenta at fixed positions), so the launch that follows is BAOAB with the total force.  One workgroup, entries strided
// (indices are distinct: the host checked), queued in front of the step launch and behind the scheduled list rebuild.
// It honours the driver's protocol (md_driver.h):
//   - it skips exactly when step launch k skips: the test of md_step_kernel on flags[1], flags[3] and the list
//     builder's overflow words;
//   - it is idempotent per launch.  The kick is in place, so the frames' invariant - a launch never modifies the state it
//     read, which is what lets an aborted launch run again wider from intact inputs - holds only if a second application
//     is a no-op: `stamp` holds 2 (step + k) + (kick_close != 0) + 1 of the last kick applied, every thread reads it in
//     front of a barrier, and a workgroup that finds its own stamp there returns.  The closed / open bit tells a
//     closing-only launch from the first launch of the next call, which carries the same step index;
//   - it writes the momenta and the stamp, nothing else; never the control words.
template <typename R>
__global__ __launch_bounds__(256) void ext_kick_kernel(int count, const int* __restrict__ index,
                                                       const typename Vec4T<R>::type* __restrict__ force, R c_dt,
                                                       typename Vec4T<R>::type* __restrict__ mom, const int* __restrict__ flags,
                                                       const int* __restrict__ list_overflow, int k_index,
                                                       unsigned long long this_stamp, unsigned long long* __restrict__ stamp) {
  const int hw = flags[1], aw = flags[3];
  const int halt = ((hw != 0 && hw <= k_index) ? 1 : 0) | ((aw != 0 && aw <= k_index) ? 1 : 0) |
                   (list_overflow ? (list_overflow[0] | list_overflow[1]) : 0);
  const unsigned long long seen = *stamp;
  __syncthreads();  // everybody has read the stamp before thread 0 replaces it
  if (halt != 0 || seen == this_stamp) return;
  for (int e = threadIdx.x; e < count; e += blockDim.x) {
    const int i = index[e];
    const auto f = force[e];
    auto p = mom[i];
    p.x += c_dt * f.x, p.y += c_dt * f.y, p.z += c_dt * f.z;
    mom[i] = p;
  }
  if (threadIdx.x == 0) *stamp = this_stamp;
}

}  // namespace mythos
