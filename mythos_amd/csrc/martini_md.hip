// Langevin MD of a MARTINI system: one fused kernel per time step (BASELINE configs[2]).
//
// The reference has no MARTINI integrator of its own - it drives GROMACS as an external process
// (mythos/simulators/gromacs/) and only re-evaluates energies (mythos/energy/martini/m2/*.py).  This file
// is the device-resident counterpart for the same force field: shifted-cut-off Lennard-Jones over a Verlet
// list, harmonic bonds, G96 / harmonic angles (the terms of martini_terms.h, as in martini.hip), and the BAOAB
// Langevin splitting used for oxDNA (langevin_step.h) specialised to point particles:
//   B  v += h F / m      A  x += h v      O  v = c1 v + sqrt(kT (1 - c1^2) / m) xi,  c1 = exp(-gamma dt)
// While the system holds charges (mythos_martini_set_charges) the COUL instantiations add reaction-field Coulomb.
// Units are GROMACS': nm, ps, amu, kJ/mol (1 kJ/mol = 1 amu nm^2 / ps^2), kT = 0.0083144626 T.
//
// Work decomposition (as md_step_kernel): 16 lanes per bead (kMmG), 16 beads per 256-thread workgroup; the lanes stride
// over the bead's neighbour row (partners inside r_c + skin, bonded partners already excluded), then over the
// bead's bonds and angles; DPP fold; one wavefront integrates the workgroup's beads.  The kernel that
// evaluates F(x_k) closes step k-1 and opens step k; frames ping-pong.  No atomics in the force path.
// Roofline: as for oxDNA the state is cache resident; algorithmic bytes per bead per step =
// 2 x (pos 3 + vel 3) words + 4 B type + 4 B x nbar.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "cell_list.h"
#include "martini_ensemble_checks.h"
#include "martini_exchange_checks.h"
#include "martini_internal.h"
#include "martini_restraints.h"
#include "martini_window_exchange_checks.h"
#include "md_driver.h"
#include "philox.h"
#include "wave_ops.h"

namespace mythos {

// (threads per workgroup, scanned in round 4 at 20 480 beads: 128 / 256 / 512 / 1 024 -> 81.4 k / 84.5 k / 83.2 k / 76.6 k steps/s)
#ifndef MYTHOS_MM_BLOCK
#define MYTHOS_MM_BLOCK 256
#endif
constexpr int kMmBlock = MYTHOS_MM_BLOCK;
// Lanes per bead.  Sixteen since round 4: the kernel needs 28 VGPRs, so twice the wavefronts (1 280 workgroups of 16 beads
// for 20 480 beads, five per CU) fit without any trade, and a lane's chain through the row is half as long - the kernel
// was latency-bound at 2.5 wavefronts per SIMD (65 % of its wave cycles waiting).  20 480 beads, events, loop rate
// (scripts/exp_martini_lanes_r04.sh, two alternations): 8 lanes 12.05 us / 68.7 k steps/s; 16 lanes with 4 / 3 / 2 row
// entries per lane in flight 10.6 / 11.1 / 11.1 us, 76.0 k / 75.6 k / 74.7 k; 32 lanes 14.3 us / 59.7 k.
#ifndef MYTHOS_MM_G
#define MYTHOS_MM_G 16
#endif
#ifndef MYTHOS_MM_BATCH
#define MYTHOS_MM_BATCH 4
#endif
constexpr int kMmG = MYTHOS_MM_G;
constexpr int kMmPPB = kMmBlock / kMmG;
constexpr int kMmTrace = 4;      // lj, bond, angle, kinetic
constexpr int kMmTraceCoul = 5;  // and the reaction-field Coulomb energy, while the system holds charges

template <typename R>
struct Real4;
template <>
struct Real4<float> {
  using type = float4;
};
template <>
struct Real4<double> {
  using type = double4;
};

template <typename R>
struct MmConst {
  R lx, ly, lz, ilx, ily, ilz;
  R rc2;
  R dt, half_dt, c1, kT;
  R skin_half_sq;  // (skin/2)^2, <= 0 disables the displacement check
  R rin2;          // (r_c + inner margin)^2: range of the pruned rows (EMIT); <= 0: no pruned rows
  R step_max_sq;   // a bead may move (margin / 2) / (inner_every - 1) per step while pruned rows are in use; <= 0: no check
  int n_types, angle_kind;
};

// Reaction-field Coulomb in the step and pressure kernels (COUL instantiations; mythos_martini_set_charges).  A frame's .w
// carries type + kMaxTypes x charge class while charges are set (class 0: no charge, so .w is the plain type otherwise).
// The kernels' arguments are those of the instantiations without charges: the Coulomb record travels behind the
// epsilon table, eps[n_types^2 + ...] = f / eps_r, k_rf, c_rf, the self term -1/2 (f / eps_r) c_rf sum q^2, then the
// charge of every class - staged in LDS with the type tables, so a neighbour's charge costs no second gather.
constexpr int kCoulPref = 0, kCoulKrf = 1, kCoulCrf = 2, kCoulSelf = 3, kCoulQ = 4;
constexpr int kCoulRec = kCoulQ + kMaxChargeClasses;

// Temperature ensemble (ENS instantiations; mythos_martini_langevin_create_ensemble): R copies of the system, replica r
// owning beads [r n, (r + 1) n) of every per-bead array, rows in LOCAL indices, topology and type tables those of one copy.
// As for COUL the kernels' arguments do not change: the replica table travels behind the Coulomb record, at the next
// multiple of 8 bytes - the number of replicas, then one record per replica with what MmConst and `seed` hold for a
// single copy.  A workgroup belongs to one replica, so its record is scalar data.
template <typename R>
struct MmRep {
  R lx, ly, lz, ilx, ily, ilz, kT, pad;
  uint64_t seed;
};
constexpr size_t kMmRepHead = 8;  // bytes: int n_rep, int unused
__host__ __device__ constexpr size_t mm_rep_offset(int tt, size_t real_bytes) {
  return (((size_t)tt + kCoulRec) * real_bytes + 7) & ~size_t(7);
}
// the replica record of workgroup `rep`, K's box and kT replaced by it
template <typename R>
__device__ __forceinline__ const MmRep<R>& mm_rep_record(const R* eps, int tt, int rep, int& n_rep) {
  const unsigned char* t = reinterpret_cast<const unsigned char*>(eps) + mm_rep_offset(tt, sizeof(R));
  n_rep = *reinterpret_cast<const int*>(t);
  return reinterpret_cast<const MmRep<R>*>(t + kMmRepHead)[rep];
}
template <typename R>
__device__ __forceinline__ void mm_rep_apply(MmConst<R>& K, const MmRep<R>& r) {
  K.lx = r.lx, K.ly = r.ly, K.lz = r.lz, K.ilx = r.ilx, K.ily = r.ily, K.ilz = r.ilz, K.kT = r.kT;
}

// Wave priority by phase (see md_step_kernel, langevin_step.h): MYTHOS_MM_PRIO_MAP = three decimal digits, the s_setprio
// level of the row loop, the bonded lists, and everything behind the barrier (0 = no s_setprio)
// (20 480 beads: 64.7 k -> 65.3 k steps/s with 310)
#ifndef MYTHOS_MM_PRIO_MAP
#define MYTHOS_MM_PRIO_MAP 310
#endif
#if MYTHOS_MM_PRIO_MAP != 0
constexpr int mm_prio_digit(int phase) {
  int v = MYTHOS_MM_PRIO_MAP;
  for (int k = 2; k > phase; --k) v /= 10;
  return v % 10;
}
#define MM_PRIO(phase) __builtin_amdgcn_s_setprio(mm_prio_digit(phase))
#else
#define MM_PRIO(phase) do { } while (0)
#endif

// EMIT (pruned rows, round 4): the launch walks the Verlet rows (range r_c + skin) and, as a by-product of the distances it
// computes anyway, writes for every bead the entries inside r_c + margin to a second set of rows, in row order.  The next
// inner_every - 1 launches walk those instead - 78 entries for 135 at the bilayer's policy - while no bead moves more
// than margin / 2 in total (checked per step, conservatively; a violation halts like a bead that leaves its skin, and
// the recovery rebuilds both lists).  GROMACS prunes its pair list the same way between searches ("dynamic pruning").
// Which list a launch walks is a function of the steps since the Verlet rows were built, so split calls stay bitwise equal.
// COUL: reaction-field Coulomb on top (the record behind eps, above): the pair term inside the row walk's cut-off test,
// the excluded-pair term on the bond slots.  The instantiations without it are, instruction for instruction, those from
// before the flag existed (scripts/isa_diff.py --alias).
// ENS: n is the bead count of ONE replica; workgroup bid serves beads [lb PPB, (lb + 1) PPB) of replica rep, through
// per-bead pointers moved to that replica in the prologue - the body below is the single copy's.
template <typename R, bool SAVE, bool EMIT = false, bool COUL = false, bool ENS = false>
__global__ __launch_bounds__(kMmBlock, 1024 / kMmBlock) void martini_md_step_kernel(
    int n, const MmConst<R> K0, const typename Real4<R>::type* __restrict__ in, typename Real4<R>::type* __restrict__ out,
    typename Real4<R>::type* __restrict__ vel, const int* __restrict__ rows, const int* __restrict__ row_len,
    int row_stride, const R* __restrict__ sigma, const R* __restrict__ eps, const int* __restrict__ bead_bonds,
    const int* __restrict__ bead_angles, const int* __restrict__ bonds, const R* __restrict__ bond_k,
    const R* __restrict__ bond_r0, const int* __restrict__ angles, const R* __restrict__ angle_k,
    const R* __restrict__ angle_t0, R kick_close, int do_step, uint64_t seed, uint64_t step,
    const typename Real4<R>::type* __restrict__ ref_pos, int* __restrict__ flags, R* __restrict__ traj,
    double* __restrict__ e_part, const int* __restrict__ list_overflow, int k_index, int* __restrict__ emit_rows,
    int* __restrict__ emit_len, const int* __restrict__ bb_partner, const int2* __restrict__ ba_partner) {
  using V4 = typename Real4<R>::type;
  constexpr int G = kMmG, PPB = kMmPPB;
  constexpr int NT = COUL ? kMmTraceCoul : kMmTrace;
  extern __shared__ unsigned char smem_raw[];
  MmConst<R> K = K0;
  R* s_sig2 = reinterpret_cast<R*>(smem_raw);
  R* s_eps = s_sig2 + K.n_types * K.n_types;
  R* s_c = s_eps + K.n_types * K.n_types;  // (COUL) the Coulomb record
  (void)s_c;
  __shared__ R s_f[PPB][4];
  __shared__ double s_e[SAVE ? PPB : 1][NT];

  int n_blocks = (n + PPB - 1) / PPB;
  int n_rep = 1;
  (void)n_rep;
  if constexpr (ENS) {
    (void)mm_rep_record<R>(eps, K.n_types * K.n_types, 0, n_rep);
    n_blocks *= n_rep;
  }
  const int bid = (int)(blockIdx.x & 7) * ((n_blocks + 7) >> 3) + (int)(blockIdx.x >> 3);  // XCD-aware order
  if (bid >= n_blocks) return;
  int lb = bid;  // the workgroup's index inside its replica
  if constexpr (ENS) {
    const int bpr = (n + PPB - 1) / PPB;
    const int rep = bid / bpr;
    lb = bid - rep * bpr;
    const MmRep<R>& rr = mm_rep_record<R>(eps, K.n_types * K.n_types, rep, n_rep);
    mm_rep_apply(K, rr);
    seed = rr.seed;
    const size_t b0 = (size_t)rep * n;
    in += b0, out += b0, vel += b0, ref_pos += b0;
    rows += b0 * row_stride, row_len += b0;
    if (traj) traj += 3 * b0;
    if constexpr (EMIT) emit_rows += b0 * row_stride, emit_len += b0;
  }
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int i = lb * PPB + grp;
  const bool valid = i < n;
  const int ii = valid ? i : n - 1;
  // Halt word (see md_drive, md_driver.h): set by the step that moved a bead out of its skin, or by a
  // rebuild that overflowed.  One lane requests it here; everybody looks at it behind the barrier in front of the
  // integration, before which nothing is written to global memory.
  __shared__ int s_halt;
  int halt_word = 0;
  // the word holds the index of the first launch that must not run: late workgroups of the launch that set it go on
  if (threadIdx.x == 0) {
    const int hw = flags[1];
    halt_word = ((hw != 0 && hw <= k_index) ? 1 : 0) | (list_overflow ? (list_overflow[0] | list_overflow[1]) : 0);
  }

  const int tt = K.n_types * K.n_types;
  for (int k = threadIdx.x; k < tt; k += kMmBlock) {  // (sigma: squared already, mm compact tables)
    s_sig2[k] = sigma[k];
    s_eps[k] = eps[k];
  }
  if constexpr (COUL)
    if (threadIdx.x < kCoulRec) s_c[threadIdx.x] = eps[tt + threadIdx.x];
  const V4 me = in[ii];
  // the bead type travels as an integer-valued real in .w (COUL: with the charge class above it, see kCoulRec)
  const int type_i = (COUL ? ((int)me.w & (kMaxTypes - 1)) : (int)me.w) * K.n_types;
  const int* __restrict__ row = rows + (size_t)ii * row_stride;
  const int len = valid ? row_len[ii] : 0;
  // bonds and angles: the lane's incidence entry and the partner beads it names are requested here, in front of the row
  // walk, so that behind it ONE round of gathers (the partners' positions) is left.  (Until round 4: entry -> bond /
  // angle record -> positions, three dependent reads behind the walk, 2.2 us of a 10.6 us kernel.)
  int ent_b0 = -1, par_b0 = -1, ent_a0 = -1;
  int2 par_a0{-1, -1};
  if (valid) {
    if (lane < kMaxBeadBonds) ent_b0 = bead_bonds[(size_t)i * kMaxBeadBonds + lane], par_b0 = bb_partner[(size_t)i * kMaxBeadBonds + lane];
    if (lane < kMaxBeadAngles) ent_a0 = bead_angles[(size_t)i * kMaxBeadAngles + lane], par_a0 = ba_partner[(size_t)i * kMaxBeadAngles + lane];
  }
  // (COUL) The excluded-pair term counts a partner once, as the exclusion table does, however many bonds join the pair:
  // a slot that repeats the partner of a lower slot of this bead does not carry it.
  bool coul_dup = false;
  (void)coul_dup;
  if constexpr (COUL) {
    static_assert(kMaxBeadBonds <= G, "one bond slot per lane");
#pragma unroll
    for (int t = 0; t < kMaxBeadBonds - 1; ++t) {
      const int pt = __shfl(par_b0, t, G);
      coul_dup = coul_dup || (t < lane && pt == par_b0);
    }
  }
  __syncthreads();

  MM_PRIO(0);
  R gx = 0, gy = 0, gz = 0;  // dU/dx_i
  R e_lj = 0, e_b = 0, e_a = 0, e_c = 0;
  (void)e_c;
  const R irc2 = R(1) / K.rc2;
  // (COUL) f / eps_r times this bead's charge; 0 for most beads, whose groups skip the Coulomb arithmetic
  R qi = 0, k_rf = 0, c_rf = 0;
  const R* s_q = s_c + kCoulQ;
  (void)qi, (void)k_rf, (void)c_rf, (void)s_q;
  if constexpr (COUL) {
    qi = valid ? s_c[kCoulPref] * s_q[(int)me.w >> 6] : R(0);
    k_rf = s_c[kCoulKrf], c_rf = s_c[kCoulCrf];
  }
  static_assert(kMaxTypes == 64, "the charge class sits above six bits of type");
  // ---- Lennard-Jones over the row, kLjBatch entries per lane at a time: their neighbour positions are requested
  //      together and the next batch's row entries before this batch is evaluated.  20 480 beads x 8 lanes are 2.5
  //      wavefronts per SIMD, too few to hide a gather per iteration (one-ahead prefetch: 14 exposed round trips per
  //      row of 112; batches of four: four).  The order of the sums over a lane's entries is unchanged.
  {
    constexpr int kLjBatch = MYTHOS_MM_BATCH;
    int jn[kLjBatch];
    int n_in = 0;  // (EMIT) entries of the pruned row so far: the same number in every lane of the group
    int* __restrict__ emit_row = EMIT ? emit_rows + (size_t)ii * row_stride : nullptr;
    const int gshift = (int)(threadIdx.x & 63) & ~(G - 1);
    constexpr unsigned int kGroupMask = (G >= 32) ? 0xffffffffu : ((1u << (G & 31)) - 1u);
    (void)n_in, (void)emit_row, (void)gshift;
#pragma unroll
    for (int u = 0; u < kLjBatch; ++u) jn[u] = (u * G + lane < len) ? row[u * G + lane] : -1;
#pragma unroll 1
    for (int s0 = 0; s0 < len; s0 += kLjBatch * G) {
      int j[kLjBatch];
      V4 o[kLjBatch];
#pragma unroll
      for (int u = 0; u < kLjBatch; ++u) {
        j[u] = jn[u];
        o[u] = in[j[u] >= 0 ? j[u] : ii];
      }
#pragma unroll
      for (int u = 0; u < kLjBatch; ++u) {
        const int idx = s0 + (kLjBatch + u) * G + lane;
        jn[u] = (idx < len) ? row[idx] : -1;
      }
#pragma unroll
      for (int u = 0; u < kLjBatch; ++u) {
        const bool have = j[u] >= 0;
        const R dx = wrap_fma(me.x - o[u].x, K.lx, K.ilx), dy = wrap_fma(me.y - o[u].y, K.ly, K.ily), dz = wrap_fma(me.z - o[u].z, K.lz, K.ilz);
        const R r2 = m_fma(dz, dz, m_fma(dy, dy, dx * dx));
        if constexpr (EMIT) {
          const bool keep = have && r2 < K.rin2;
          const unsigned int gm = (unsigned int)(__ballot(keep) >> gshift) & kGroupMask;
          if (keep) emit_row[n_in + __popc(gm & ((1u << lane) - 1u))] = j[u];
          n_in += __popc(gm);
        }
        if (have && r2 < K.rc2) {
          const int tp = type_i + (COUL ? ((int)o[u].w & (kMaxTypes - 1)) : (int)o[u].w);
          const R ep = s_eps[tp];
          const LjPair<R> t = lj_pair(s_sig2[tp], ep, r2);
          gx += t.g * dx, gy += t.g * dy, gz += t.g * dz;
          if constexpr (SAVE) e_lj += R(0.5) * R(4) * ep * lj_shifted(t, lj_pow6(s_sig2[tp], irc2));
          if constexpr (COUL) {
            if (qi != R(0)) {
              const R qq = qi * s_q[(int)o[u].w >> 6];
              const RfPair<R> c = rf_pair(r2, k_rf, c_rf);
              const R cg = qq * c.g;
              gx += cg * dx, gy += cg * dy, gz += cg * dz;
              if constexpr (SAVE) e_c += R(0.5) * qq * c.v;
            }
          }
        }
      }
    }
    if constexpr (EMIT)
      if (valid && lane == 0) emit_len[i] = n_in;
  }
  // ---- bonds and angles of this bead (incidence lists, one entry per lane)
  MM_PRIO(1);
  if (valid) {
    for (int s = lane; s < kMaxBeadBonds; s += G) {
      const int ent = (s == lane) ? ent_b0 : bead_bonds[(size_t)i * kMaxBeadBonds + s];
      if (ent < 0) continue;
      const int partner = (s == lane) ? par_b0 : bb_partner[(size_t)i * kMaxBeadBonds + s];
      const int b = ent >> 1, side = ent & 1;
      const V4 o = in[partner];
      const R dx = wrap(me.x - o.x, K.lx, K.ilx), dy = wrap(me.y - o.y, K.ly, K.ily), dz = wrap(me.z - o.z, K.lz, K.ilz);
      const BondTerm<R> t = bond_term(dx * dx + dy * dy + dz * dz, bond_k[b], bond_r0[b]);
      gx += t.c * dx, gy += t.c * dy, gz += t.c * dz;
      if constexpr (SAVE)
        if (side == 0) e_b += R(0.5) * bond_k[b] * t.x * t.x;
      if constexpr (COUL) {  // the excluded pair's reaction-field term, once per pair and owner
        const R r2 = dx * dx + dy * dy + dz * dz;
        if (qi != R(0) && !coul_dup && r2 < K.rc2) {
          const R qq = qi * s_q[(int)o.w >> 6];
          const RfPair<R> c = rf_excluded(r2, k_rf, c_rf);
          const R cg = qq * c.g;
          gx += cg * dx, gy += cg * dy, gz += cg * dz;
          if constexpr (SAVE) e_c += R(0.5) * qq * c.v;
        }
      }
    }
    for (int s = lane; s < kMaxBeadAngles; s += G) {
      const int ent = (s == lane) ? ent_a0 : bead_angles[(size_t)i * kMaxBeadAngles + s];
      if (ent < 0) continue;
      const int2 others = (s == lane) ? par_a0 : ba_partner[(size_t)i * kMaxBeadAngles + s];
      const int a = ent >> 2, role = ent & 3;  // 0: first bead, 1: centre, 2: last bead
      // (the other two beads of the angle, in its order; this bead's own position is in registers)
      const V4 q0 = in[others.x], q1 = in[others.y];
      const V4 pi = role == 0 ? me : q0, pj = role == 0 ? q0 : (role == 1 ? me : q1), pk = role == 2 ? me : q1;
      const R u[3] = {wrap(pi.x - pj.x, K.lx, K.ilx), wrap(pi.y - pj.y, K.ly, K.ily), wrap(pi.z - pj.z, K.lz, K.ilz)};
      const R v[3] = {wrap(pk.x - pj.x, K.lx, K.ilx), wrap(pk.y - pj.y, K.ly, K.ily), wrap(pk.z - pj.z, K.lz, K.ilz)};
      const R u2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      const R uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
      const AngleGeom<R> ag = angle_geometry(u, v, u2, v2, uv, K.angle_kind);
      const AngleTerm<R> t = angle_term(K.angle_kind, ag, angle_k[a], angle_t0[a]);  // (d_angle_ref: cos(theta0) for G96)
      const R en = R(0.5) * angle_k[a] * t.x * t.x;
      if constexpr (SAVE)
        if (role == 0) e_a += en;
      const R gk[3] = {angle_role_grad(role, ag, u[0], v[0]), angle_role_grad(role, ag, u[1], v[1]), angle_role_grad(role, ag, u[2], v[2])};
      gx += t.dEdc * gk[0], gy += t.dEdc * gk[1], gz += t.dEdc * gk[2];
    }
  }
  gx = group_sum<G>(gx);
  gy = group_sum<G>(gy);
  gz = group_sum<G>(gz);
  if constexpr (SAVE) {
    e_lj = group_sum<G>(e_lj);
    e_b = group_sum<G>(e_b);
    e_a = group_sum<G>(e_a);
    if constexpr (COUL) e_c = group_sum<G>(e_c);
  }
  if (lane == 0) {
    s_f[grp][0] = gx, s_f[grp][1] = gy, s_f[grp][2] = gz;
    if constexpr (SAVE) {
      s_e[grp][0] = valid ? double(e_lj) : 0.0;
      s_e[grp][1] = valid ? double(e_b) : 0.0;
      s_e[grp][2] = valid ? double(e_a) : 0.0;
      s_e[grp][3] = 0.0;
      if constexpr (COUL) s_e[grp][4] = valid ? double(e_c) : 0.0;
    }
  }
  // ---- integrator prologue, before the barrier: the integrating wavefront draws its thermostat noise and fetches
  //      position, velocity and list reference here, so the tail of the kernel behind the barrier is arithmetic only
  //      (the oxDNA step kernel's arrangement, langevin_step.h).  pin_vgpr keeps the values on this side of the barrier.
  const int int_wave = (bid >> 2) & (kMmBlock / 64 - 1) & 3;
  const int il = threadIdx.x & 63;
  const int ib = lb * PPB + il;
  const bool integrates = (int)(threadIdx.x >> 6) == int_wave && il < PPB && ib < n;
  R z[6] = {R(0), R(0), R(0), R(0), R(0), R(0)};
  V4 x0{}, vv{}, r0{};
  if (integrates) {
    x0 = in[ib];
    vv = vel[ib];
    if (do_step && K.skin_half_sq > R(0)) r0 = ref_pos[ib];
    if (do_step) normals6(seed, (uint32_t)ib, step, 0u, z);
    pin_vgpr(z[0]), pin_vgpr(z[1]), pin_vgpr(z[2]);
    pin_vgpr(x0.x), pin_vgpr(x0.y), pin_vgpr(x0.z), pin_vgpr(vv.x), pin_vgpr(vv.y), pin_vgpr(vv.z), pin_vgpr(vv.w);
  }
  if (threadIdx.x == 0) s_halt = halt_word;
  __syncthreads();
  if (s_halt != 0) return;  // halted: the state stays at the last valid step
  MM_PRIO(2);
  if (bid == 0 && threadIdx.x == 0) flags[2] = k_index + 1;
  // ---- one wavefront integrates the beads of the workgroup, one per lane
  if (integrates) {
    const R im = vv.w;  // inverse mass
    const R F[3] = {-s_f[il][0], -s_f[il][1], -s_f[il][2]};
    R x[3] = {x0.x, x0.y, x0.z}, v[3] = {vv.x, vv.y, vv.z};
    const R kc = kick_close * K.dt * im;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += kc * F[k];
    if constexpr (SAVE) {
      s_e[il][3] = 0.5 * (double(v[0]) * v[0] + double(v[1]) * v[1] + double(v[2]) * v[2]) / double(im);
      if (traj) traj[3 * (size_t)ib] = x[0], traj[3 * (size_t)ib + 1] = x[1], traj[3 * (size_t)ib + 2] = x[2];
    }
    if (do_step) {
      const R hk = K.half_dt * im;
      const R c2 = m_sqrt(K.kT * im * (R(1) - K.c1 * K.c1));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] += hk * F[k];
        x[k] += K.half_dt * v[k];
        v[k] = K.c1 * v[k] + c2 * z[k];
        x[k] += K.half_dt * v[k];
      }
      if (K.skin_half_sq > R(0)) {
        const R dx = x[0] - r0.x, dy = x[1] - r0.y, dz = x[2] - r0.z;
        if (dx * dx + dy * dy + dz * dz > K.skin_half_sq) atomicMax(flags + 1, k_index + 1);  // stale for the NEXT forces: launch k + 1 halts
      }
      if (K.step_max_sq > R(0)) {  // pruned rows in use: see EMIT
        const R dx = x[0] - x0.x, dy = x[1] - x0.y, dz = x[2] - x0.z;
        if (dx * dx + dy * dy + dz * dz > K.step_max_sq) atomicMax(flags + 1, k_index + 1);
      }
      if (!(x[0] == x[0]) || !(v[0] == v[0])) atomicOr(flags, 2);
    }
    out[ib] = V4{x[0], x[1], x[2], x0.w};
    vel[ib] = V4{v[0], v[1], v[2], im};
    if constexpr (!SAVE) {
      // positions-only trajectory (e_trace == NULL): the launch that produces x_{k+1} writes it to the caller's row too
      // (md_step_kernel does the same, langevin_step.h) - no energy-trace instantiation, no reduction, no closing launch
      if (traj) traj[3 * (size_t)ib] = x[0], traj[3 * (size_t)ib + 1] = x[1], traj[3 * (size_t)ib + 2] = x[2];
    }
  }
  if constexpr (SAVE) {
    __syncthreads();
    if (threadIdx.x < NT) {
      double s = 0.0;
      for (int g = 0; g < PPB; ++g) s += s_e[g][threadIdx.x];
      if constexpr (COUL)
        if (lb == 0 && threadIdx.x == 4) s += double(s_c[kCoulSelf]);
      e_part[(size_t)bid * NT + threadIdx.x] = s;
    }
  }
}

template <typename R>
__global__ void mm_pack_kernel(int n, const R* __restrict__ pos, const R* __restrict__ v, const int* __restrict__ types,
                               const R* __restrict__ inv_mass, typename Real4<R>::type* __restrict__ frame,
                               typename Real4<R>::type* __restrict__ vel) {
  using V4 = typename Real4<R>::type;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  frame[i] = V4{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], R(types[i])};  // (types: with the charge class, see kCoulRec)
  vel[i] = V4{v[3 * i], v[3 * i + 1], v[3 * i + 2], inv_mass[i]};
}

// the charges changed under a resident frame (mm_sync_charges): its .w takes the new packed types
template <typename R>
__global__ void mm_retype_kernel(int n, const int* __restrict__ types, typename Real4<R>::type* __restrict__ frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) frame[i].w = R(types[i]);
}

// Ensemble forms of the two kernels above: n beads per replica, types and inverse masses those of one copy
template <typename R>
__global__ void mm_pack_ens_kernel(int n, int n_rep, const R* __restrict__ pos, const R* __restrict__ v, const int* __restrict__ types,
                                   const R* __restrict__ inv_mass, typename Real4<R>::type* __restrict__ frame,
                                   typename Real4<R>::type* __restrict__ vel) {
  using V4 = typename Real4<R>::type;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_rep) return;
  const int l = i % n;
  frame[i] = V4{pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], R(types[l])};
  vel[i] = V4{v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2], inv_mass[l]};
}

template <typename R>
__global__ void mm_retype_ens_kernel(int n, int n_rep, const int* __restrict__ types, typename Real4<R>::type* __restrict__ frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * n_rep) frame[i].w = R(types[i % n]);
}

// Energy-trace rows of an ensemble: workgroup r sums the blocks_per_rep partials of replica r into row r, in the order
// reduce_trace_kernel (md_driver.h) sums those of a single copy
template <int WIDTH>
static __global__ __launch_bounds__(256) void mm_reduce_trace_ens_kernel(const double* __restrict__ part, int blocks_per_rep,
                                                                         double* __restrict__ out) {
  __shared__ double acc[16][17];
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  part += (size_t)blockIdx.x * blocks_per_rep * WIDTH;
  double s = 0.0;
  if (k < WIDTH)
    for (int b = g; b < blocks_per_rep; b += 16) s += part[(size_t)b * WIDTH + k];
  acc[g][k] = s;
  __syncthreads();
  if (g == 0 && k < WIDTH && out) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) t += acc[j][k];
    out[(size_t)blockIdx.x * WIDTH + k] = t;
  }
}

template <typename R>
__global__ void mm_unpack_kernel(int n, const typename Real4<R>::type* __restrict__ frame,
                                 const typename Real4<R>::type* __restrict__ vel, R* __restrict__ pos, R* __restrict__ v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pos[3 * i] = frame[i].x, pos[3 * i + 1] = frame[i].y, pos[3 * i + 2] = frame[i].z;
  v[3 * i] = vel[i].x, v[3 * i + 1] = vel[i].y, v[3 * i + 2] = vel[i].z;
}

// Maxwell-Boltzmann velocities with the centre-of-mass momentum removed (single workgroup, runs once)
template <typename R>
__global__ void mm_init_velocities_kernel(int n, R kT, const R* __restrict__ inv_mass, uint64_t seed, R* __restrict__ v) {
  __shared__ double sum[4][256];
  double s0 = 0, s1 = 0, s2 = 0, sm = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    R z[6];
    normals6(seed, (uint32_t)i, 0xFFFFFFFFFFFFFFFFull, 7u, z);
    const R sd = m_sqrt(kT * inv_mass[i]);
    v[3 * i] = sd * z[0], v[3 * i + 1] = sd * z[1], v[3 * i + 2] = sd * z[2];
    const double m = 1.0 / double(inv_mass[i]);
    s0 += m * v[3 * i], s1 += m * v[3 * i + 1], s2 += m * v[3 * i + 2], sm += m;
  }
  sum[0][threadIdx.x] = s0, sum[1][threadIdx.x] = s1, sum[2][threadIdx.x] = s2, sum[3][threadIdx.x] = sm;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 4; ++k) sum[k][threadIdx.x] += sum[k][threadIdx.x + o];
    __syncthreads();
  }
  const R c0 = R(sum[0][0] / sum[3][0]), c1 = R(sum[1][0] / sum[3][0]), c2 = R(sum[2][0] / sum[3][0]);
  for (int i = threadIdx.x; i < n; i += blockDim.x) v[3 * i] -= c0, v[3 * i + 1] -= c1, v[3 * i + 2] -= c2;
}

// ------------------------------------------------------------------------------------------------
// Verlet rows for point particles in a periodic orthorhombic box.  One wavefront per bead; candidates come
// from the 27 surrounding cells of the hashed cell list (cell_list.h) or, for boxes under three cells per edge
// and tiny systems, from a sweep over all beads.  Directly bonded partners are left out (the reference masks
// them, mythos/energy/martini/m2/lj.py:137-157).  Rows are in ascending (cell, index) order: reproducible.
// ------------------------------------------------------------------------------------------------
template <typename R>
__device__ __forceinline__ bool mm_excluded(const int* __restrict__ ex, int j) {
  bool hit = false;
#pragma unroll
  for (int q = 0; q < kMaxExcl; ++q) hit = hit || (ex[q] == j);
  return hit;
}

// G lanes per bead (kMmRowG): the rows of 64 / G beads are built side by side in one wavefront.  The kernel is
// VALU-bound (SQ_ACTIVE_INST_VALU x 4 clocks / SIMDs = 75 % of its time): ~2.2 instructions per candidate, but a bead
// has 400-750 candidates in its 27 cells of which ~112 are inside the list range (cells of the full range: the
// sphere is 15 % of the 27-cell volume).  16, 32 and 64 lanes per bead take the same time; 8 is slower.
#ifndef MYTHOS_MM_ROW_G
#define MYTHOS_MM_ROW_G 16
#endif
constexpr int kMmRowG = MYTHOS_MM_ROW_G;

// (Round 4 tried cells of HALF the list range again - 125 around a bead, those whose nearest point lies beyond the range
// dropped before the sweep: 2.6 times fewer candidates, and 41.9 us against 36.1 us for this kernel at 20 480 beads
// (rocprofv3, scripts/exp_martini_r04.sh; the loop 66.0 k against 68.6 k steps/s).  A sweep of 16 candidates then spans
// four or five cells and every lane walks the prefix table through them - five dependent LDS reads per sweep where the
// 27-cell grid needs one every other sweep - and 125 table look-ups per bead replace 27.  The kernel is not bound by its
// candidate count alone; the variant is not in the source.)
template <typename R, int G>
__global__ __launch_bounds__(256) void mm_build_rows_cells_kernel(
    int n, const typename Real4<R>::type* __restrict__ pos, const MmConst<R> K, const CellGrid<R> g, R rl2,
    const int* __restrict__ excl, const int* __restrict__ cell_cnt,
    const typename CellPlace<R>::type* __restrict__ place, int cell_cap, const int* __restrict__ spill, int cell_H,
    int* __restrict__ rows, int* __restrict__ row_len, int row_stride, int* __restrict__ overflow,
    typename Real4<R>::type* __restrict__ ref_pos) {
  constexpr int NG = 256 / G;  // beads per workgroup
  __shared__ int s_pre[NG][29], s_st[NG][28], s_c[NG][28][3];
  const int grp = threadIdx.x / G, l = threadIdx.x % G;
  const int gshift = (threadIdx.x & 63) & ~(G - 1);  // first lane of this group inside its wavefront
  const int i = blockIdx.x * NG + grp;
  if (i >= n) return;
  const auto pi = pos[i];
  const int total = cell_candidates<R, G>(g, pi.x, pi.y, pi.z, cell_cnt, cell_cap, cell_H, s_pre[grp], s_st[grp], s_c[grp], l);
  int ex[kMaxExcl];
#pragma unroll
  for (int q = 0; q < kMaxExcl; ++q) ex[q] = excl[(size_t)i * kMaxExcl + q];
  // excluded partners are beads of the same molecule, whose indices lie in a short window around i: the eight
  // comparisons run only in sweeps where some candidate falls inside it
  int ex_lo = 0x7fffffff, ex_hi = -1;
#pragma unroll
  for (int q = 0; q < kMaxExcl; ++q)
    if (ex[q] >= 0) ex_lo = min(ex_lo, ex[q]), ex_hi = max(ex_hi, ex[q]);
  int* row = rows + (size_t)i * row_stride;
  constexpr unsigned int kGroupMask = (G == 32) ? 0xffffffffu : ((1u << G) - 1u);
  const unsigned int below = (1u << l) - 1u;
  int out = 0;
  int lo = 0;  // cell of this lane's candidate: only ever advances, t grows by G per sweep
  // The sweep body is written without nested branches (clamped reads, predicates folded into `hit`): as nested ifs it
  // compiled to a dozen exec-mask branches per sweep, and the kernel is bound by the instructions of its ~164 k
  // wave-sweeps (10.5 M candidates / 64), not by their memory traffic.
  const int n_direct = s_pre[grp][27];  // candidates that come from buckets; the rest is the spill list
  // kSweeps sweeps per iteration: their (clamped, unconditional) reads are issued together and waited for once.  With
  // four beads per wavefront a dense cell is ~47 sweeps of 16 for its group, and a group's chain of sweeps - each a
  // table look-up and a read away from its test - is what the kernel's duration follows.
#ifndef MYTHOS_MM_SWEEPS
#define MYTHOS_MM_SWEEPS 4
#endif
  constexpr int kSweeps = MYTHOS_MM_SWEEPS;
  for (int t0 = 0; t0 < total; t0 += kSweeps * G) {
    typename CellPlace<R>::type pj[kSweeps];
    int cell[kSweeps], tcs[kSweeps];
#pragma unroll
    for (int u = 0; u < kSweeps; ++u) {
      const int t = t0 + u * G + l;
      const int tc = t < total ? t : total - 1;
      while (s_pre[grp][lo + 1] <= tc) ++lo;
      cell[u] = lo;
      tcs[u] = tc;
      // position and index of the candidate arrive together, a contiguous stream per cell
      pj[u] = place[tc < n_direct ? s_st[grp][lo] + (tc - s_pre[grp][lo]) : 0];
    }
#pragma unroll
    for (int u = 0; u < kSweeps; ++u) {
      const int t = t0 + u * G + l;
      const bool live = t < total;
      const bool from_bucket = tcs[u] < n_direct;
      int j = cell_index_of(pj[u].w);
      if (!from_bucket) {  // spill list (rare): index, then a gather
        j = spill[tcs[u] - n_direct];
        const auto q = pos[j];
        pj[u].x = q.x, pj[u].y = q.y, pj[u].z = q.z;
      }
      bool keep = live & (j != i);
      if (j >= ex_lo && j <= ex_hi) keep = keep & !mm_excluded<R>(ex, j);  // one or two sweeps of a row
      if (!g.direct) {  // hashed table: a bucket may mix cells that collide, a candidate counts only for the cell it lies in
        int jx, jy, jz;
        cell_of(g, pj[u].x, pj[u].y, pj[u].z, jx, jy, jz);
        const int c = cell[u];
        keep = keep & (!from_bucket | (jx == s_c[grp][c][0] & jy == s_c[grp][c][1] & jz == s_c[grp][c][2]));
      }
      const R dx = wrap(pj[u].x - pi.x, K.lx, K.ilx), dy = wrap(pj[u].y - pi.y, K.ly, K.ily), dz = wrap(pj[u].z - pi.z, K.lz, K.ilz);
      const bool hit = keep & (dx * dx + dy * dy + dz * dz < rl2);
      const unsigned int m = (unsigned int)(__ballot(hit) >> gshift) & kGroupMask;
      const int slot = out + __popc(m & below);
      if (hit & (slot < row_stride)) row[slot] = j;
      out += __popc(m);
    }
  }
  if (l == 0) {
    if (out > row_stride) {
      atomicMax(overflow, out);
      out = row_stride;
    }
    row_len[i] = out;
    ref_pos[i] = pi;  // what the displacement check of the step kernel compares against
  }
}

template <typename R>
__global__ __launch_bounds__(256) void mm_build_rows_allpairs_kernel(
    int n, const typename Real4<R>::type* __restrict__ pos, const MmConst<R> K, R rl2, const int* __restrict__ excl,
    int* __restrict__ rows, int* __restrict__ row_len, int row_stride, int* __restrict__ overflow,
    typename Real4<R>::type* __restrict__ ref_pos) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + w;
  if (i >= n) return;
  const auto pi = pos[i];
  int ex[kMaxExcl];
#pragma unroll
  for (int q = 0; q < kMaxExcl; ++q) ex[q] = excl[(size_t)i * kMaxExcl + q];
  int* row = rows + (size_t)i * row_stride;
  int out = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    if (j < n && j != i && !mm_excluded<R>(ex, j)) {
      const auto pj = pos[j];
      const R dx = wrap(pj.x - pi.x, K.lx, K.ilx), dy = wrap(pj.y - pi.y, K.ly, K.ily), dz = wrap(pj.z - pi.z, K.lz, K.ilz);
      hit = dx * dx + dy * dy + dz * dz < rl2;
    }
    const unsigned long long m = __ballot(hit);
    if (hit) {
      const int slot = out + __popcll(m & ((1ull << lane) - 1ull));
      if (slot < row_stride) row[slot] = j;
    }
    out += __popcll(m);
  }
  if (lane == 0) {
    if (out > row_stride) {
      atomicMax(overflow, out);
      out = row_stride;
    }
    row_len[i] = out;
    ref_pos[i] = pi;  // what the displacement check of the step kernel compares against
  }
}

}  // namespace mythos

using namespace mythos;

// Pressure coupling of the resident state (martini_npt.inc): what mythos_martini_langevin_set_barostat set, the device and
// pinned records of the last pressure evaluation / coupling event, and the box of every row the last call saved.
struct MmBarostat {
  int kind = 0;      // 0 off, 1 Berendsen, 2 stochastic cell rescaling
  int coupling = 0;  // 0 isotropic, 1 semi-isotropic (xy, z)
  double ref_p[2] = {1.0, 1.0}, beta[2] = {0.0, 0.0}, tau_p = 1.0;  // bar, 1/bar, ps
  int every = 10;
  mythos::DeviceBuf<double> d_part, d_rec;  // per-workgroup partials [blocks][6]; the record the scale kernel reads
  mythos::PinnedBuf<double> rec;            // the same record in pinned host memory, written by the device
  std::vector<double> last_boxes;           // [rows][3] of the last run / advance
};

// An exchange between the replicas of an ensemble, temperature exchange (xchg, martini_exchange.inc) and window exchange
// (wx, martini_window_exchange.inc) alike: what set_exchange / set_window_exchange set, the permutation - which rung's kT
// every slot runs at, which window's parameter row it holds -, the counts since restart / set_restraints, and the
// permutation rows and attempt log of the last call.
static_assert(kXchgRec == 11 && kWxRec == kXchgRec, "one log record for both exchanges: column 1 the rung, column 10 accepted");
struct MmPairExchange {
  int every = 0;      // 0: off
  uint64_t seed = 0;  // of the decisions' uniforms, a Philox stream of its own
  std::vector<int32_t> of_slot;            // [n_rep]: rung_of_slot / window_of_slot, the identity at creation
  std::vector<int64_t> attempts, accepts;  // [n_rep - 1], per rung pair (t, t + 1)
  std::vector<int32_t> last_rows;          // [rows][n_rep]: of_slot at every row the last call saved
  std::vector<double> last_log;            // [attempted pairs][kXchgRec]
  // pinned, allocated at the first advance with the exchange on.  h_d: out the log [n_rep / 2][kXchgRec]; temperature
  // exchange has in boxes [n_rep][3], kT [n_rep] in front of it.  h_i: in of_slot [n_rep], out the new one [n_rep].
  mythos::PinnedBuf<double> h_d;
  mythos::PinnedBuf<int> h_i;
  void identity() {
    for (size_t r = 0; r < of_slot.size(); ++r) of_slot[r] = (int32_t)r;
    std::fill(attempts.begin(), attempts.end(), 0);
    std::fill(accepts.begin(), accepts.end(), 0);
  }
};
// what temperature exchange needs on top: the ladder, and the device buffers of an event
struct MmLadder {
  std::vector<double> kT;                     // [n_rep]: the kT given at creation, in their order
  mythos::DeviceBuf<double> d_etrace, d_fac;  // energy rows of an event whose step is not saved [n_rep][5]; velocity factors [n_rep]
};

// External forces of the resident state (martini_restraints.h, martini_restraints.inc): the device arrays of the set
// mythos_martini_langevin_set_restraints installed, the COM rows and the kick's stamp words.  installed = false: the
// integrator launches nothing it did not launch before the set existed.
struct MmRestraints {
  bool installed = false;
  bool uses_box = false;      // a periodic coordinate or a pbc_ref: the set holds the boxes it was lowered for
  bool stamp_stale = true;    // the stamp words are cleared in front of the next kick (load, restart, set_restraints)
  mythos::MrView view;
  std::vector<double> h_boxes;
  mythos::DeviceBuf<int> d_pr_index, d_fb_index, d_fb_flags, d_g_first, d_g_member, d_g_pbc_ref, d_p_flags, d_p_groups, d_e_index, d_e_first, d_e_term;
  mythos::DeviceBuf<double> d_pr_k, d_pr_ref, d_fb_param, d_p_param, d_boxes, d_mass, d_rows, d_eval_rows;
  mythos::DeviceBuf<unsigned long long> d_stamp, d_eval_stamp;
  mythos::DeviceBuf<int> d_eval_flags;
  mythos::DeviceBytes d_eval_vel;
  int kick_blocks() const { return (int)(((long long)view.n_rep * view.n_entries + 255) / 256); }
};

struct mythos_martini_sim : mythos::MdRun {
  mythos_martini* sys = nullptr;
  double dt = 0.02, kT = 2.27, gamma = 1.0;
  double skin = 0.2;  // (MdRun::rebuild_every: 10 until set_neighbor_policy)
  int device = 0;  // the system's, copied at create: the integrator may outlive its system, to be destroyed only
  DeviceBytes frame[2], vel, ref_pos, d_inv_mass;
  // Type tables of the step kernel: only the types that occur, renumbered 0 .. n_ctypes - 1 (the DMPC bilayer uses 4 of
  // the force field's 37: every workgroup filled 2 x 37^2 LDS entries per launch, 0.9 us of a 10.6 us kernel), sigma
  // already squared.  d_ctypes: the compact type of every bead (what the frames carry in .w).
  int n_ctypes = 0;
  DeviceBuf<int> d_ctypes;
  // Reaction-field Coulomb: derived from the system's charges whenever its charge_gen moved (mm_sync_charges).  d_ctypes
  // then holds h_ctypes + kMaxTypes x charge class, d_ceps the Coulomb record behind h_ceps (kCoulRec reals, always there).
  std::vector<int> h_ctypes;
  std::vector<double> h_ceps;
  int charge_gen = 0;
  int param_gen = 0;         // the system's at the time the tables below were derived (mythos_martini_set_params, mm_sync_params)
  std::vector<int> h_used;   // the force field's type of every compact type
  bool coul = false;
  int trace_width() const { return coul ? kMmTraceCoul : kMmTrace; }
  DeviceBytes d_csig2, d_ceps;
  // per incidence slot of a bead: the partner of the bond, the two other beads of the angle (see the step kernel)
  DeviceBuf<int> d_bb_partner;
  DeviceBuf<int2> d_ba_partner;
  DeviceBytes d_angle_ref;  // per angle: cos(theta0) for the G96 form (once, instead of a cosine per lane and step), theta0 for the harmonic one
  mythos::VerletRows list{64};  // cell buckets start at 64 places; the rows at a stride of 256 (allocated at create)
  DeviceBuf<int> d_row_len;
  // pruned rows (martini_md_step_kernel, EMIT): entries of the Verlet rows inside r_c + inner_margin, rewritten every
  // inner_every steps by the step launch itself; inner_margin <= 0 or inner_every < 2: not used
  DeviceBuf<int> d_rows_in, d_row_len_in;
  double inner_margin = 0.0;  // off until mythos_martini_langevin_set_inner_list asks for them
  int inner_every = 4;
  DeviceBuf<double> d_epart;
  double box[3] = {0, 0, 0};  // of the resident state (mythos_martini_langevin_load / advance / store)
  MmBarostat baro;            // off until mythos_martini_langevin_set_barostat: box is then constant between two loads
  // Temperature ensemble (mythos_martini_langevin_create_ensemble): n_rep copies of the system in one set of arrays,
  // replica-major; 0: the single copy above, whose kT, seed and box are then the only ones.  The replica table of the
  // kernels sits behind d_ceps' Coulomb record; it is staged in pinned memory (h_reps) and uploaded by mm_upload_reps
  // whenever a box moved.
  int n_rep = 0;
  std::vector<double> rep_kT, rep_box;  // [n_rep], [n_rep][3]
  std::vector<uint64_t> rep_seed;
  mythos::PinnedBuf<unsigned char> h_reps;
  MmPairExchange xchg;  // off until mythos_martini_langevin_set_exchange
  MmLadder ladder;
  MmRestraints rst;   // none until mythos_martini_langevin_set_restraints
  MmPairExchange wx;  // off until mythos_martini_langevin_set_window_exchange
  std::vector<double> h_mass;  // [n] as given at creation (the COM weights of the pull groups)
  int copies() const { return n_rep > 0 ? n_rep : 1; }
  int n_all() const { return copies() * sys->n; }  // beads of all copies
  const double* box_of(int r) const { return n_rep > 0 ? &rep_box[3 * (size_t)r] : box; }
  ~mythos_martini_sim() { (void)hipSetDevice(device); }  // the members, MdRun's too, free themselves on that device
};

namespace mythos {

template <typename R>
static MmConst<R> mm_const(const mythos_martini_sim* sim, const double* box);

// the rows of copy `rep` (0 for a single copy) from its n beads at pos, in its box: local indices, its slice of the row store
template <typename R>
static int mm_rebuild_one(mythos_martini_sim* sim, int rep, const typename Real4<R>::type* pos, hipStream_t st) {
  mythos_martini* m = sim->sys;
  VerletRows& L = sim->list;
  const int n = m->n;
  const double rl = m->r_cut + sim->skin;
  const double* box = sim->box_of(rep);
  const MmConst<R> K = mm_const<R>(sim, box);
  const size_t b0 = (size_t)rep * n;
  int* d_rows = L.d_rows.get() + b0 * L.stride;
  int* d_row_len = sim->d_row_len.get() + b0;
  typename Real4<R>::type* d_ref = (typename Real4<R>::type*)sim->ref_pos.get() + b0;
  pos += b0;
  CellGrid<R> g;
  if (!cell_grid(g, n, rl, box)) {
    hipLaunchKernelGGL(mm_build_rows_allpairs_kernel<R>, dim3((n + 3) / 4), dim3(256), 0, st, n, pos, K, R(rl * rl), m->d_excl.get(),
                       d_rows, d_row_len, L.stride, L.d_overflow.get(), d_ref);
    return 0;
  }
  // one table slot per cell (no hashing) whenever the grid is not much larger than the system
  const long long n_cells = (long long)g.nc[0] * g.nc[1] * g.nc[2];
  g.direct = n_cells <= 8LL * n ? 1 : 0;
  CellBins bins;
  if (int rc = cell_table<R>(L, g.direct ? (int)n_cells : next_pow2(2 * n), false, st, bins)) return rc;
  // buckets sorted by bead index: the row builder copies candidates in bucket order, and rows must not depend on
  // the order in which the binning atomics landed
  cell_bins_build<R, true>(n, reinterpret_cast<const R*>(pos), g, bins, L.d_overflow.get(), true, st);
  hipLaunchKernelGGL((mm_build_rows_cells_kernel<R, kMmRowG>), dim3((n + 256 / kMmRowG - 1) / (256 / kMmRowG)), dim3(256), 0, st, n, pos, K, g,
                     R(rl * rl), m->d_excl.get(), bins.cnt_cur, (const typename CellPlace<R>::type*)bins.place, bins.cap, bins.spill, bins.H,
                     d_rows, d_row_len, L.stride, L.d_overflow.get(), d_ref);
  return 0;
}

// Every copy's rows, one after the other through the one cell table: each build is the single copy's, so are its rows.
template <typename R>
static int mm_rebuild(mythos_martini_sim* sim, const typename Real4<R>::type* pos, hipStream_t st) {
  for (int r = 0; r < sim->copies(); ++r)
    if (int rc = mm_rebuild_one<R>(sim, r, pos, st)) return rc;
  return 0;
}

// pruned rows make sense inside the skin and when at least one launch walks them between two prunings
static bool mm_inner_on(const mythos_martini_sim* sim) {
  return sim->inner_margin > 0 && sim->inner_margin < sim->skin && sim->inner_every >= 2;
}

// (an ensemble's step and pressure kernels take box and kT from the replica table instead: box_of(0) stands in)
template <typename R>
static MmConst<R> mm_const(const mythos_martini_sim* sim, const double* box) {
  const mythos_martini* m = sim->sys;
  MmConst<R> K;
  K.lx = R(box[0]), K.ly = R(box[1]), K.lz = R(box[2]);
  K.ilx = R(1.0 / box[0]), K.ily = R(1.0 / box[1]), K.ilz = R(1.0 / box[2]);
  K.rc2 = R(m->r_cut * m->r_cut);
  K.dt = R(sim->dt), K.half_dt = R(0.5 * sim->dt), K.c1 = R(std::exp(-sim->gamma * sim->dt)), K.kT = R(sim->kT);
  K.skin_half_sq = R(0.25 * sim->skin * sim->skin);
  const bool inner = mm_inner_on(sim);
  const double rin = m->r_cut + sim->inner_margin, smax = 0.5 * sim->inner_margin / std::max(1, sim->inner_every - 1);
  K.rin2 = inner ? R(rin * rin) : R(0);
  K.step_max_sq = inner ? R(smax * smax) : R(0);
  K.n_types = sim->n_ctypes, K.angle_kind = m->angle_kind;
  return K;
}

// Ensemble: the replica table (box, 1 / box, kT, seed per replica, as mm_const rounds them for a single copy) from the
// pinned staging buffer to the device, behind st.  The host writes the staging buffer only while st is idle: at create,
// at load, and behind the synchronisation of a coupling event.
static int mm_upload_reps(mythos_martini_sim* sim, hipStream_t st) {
  const int nr = sim->n_rep;
  const bool f32 = sim->sys->dtype == MYTHOS_F32;
  const size_t rec = f32 ? sizeof(MmRep<float>) : sizeof(MmRep<double>), tab = kMmRepHead + nr * rec;
  if (int rc = sim->h_reps.grow(tab)) return rc;  // (the number of replicas is fixed at create)
  unsigned char* h = sim->h_reps.host();
  const int head[2] = {nr, 0};
  std::memcpy(h, head, kMmRepHead);
  for (int r = 0; r < nr; ++r) {
    const double* b = sim->box_of(r);
    const double kT = sim->rep_kT[r];
    if (f32) {
      const MmRep<float> q{float(b[0]), float(b[1]), float(b[2]), float(1.0 / b[0]), float(1.0 / b[1]), float(1.0 / b[2]), float(kT), 0.0f, sim->rep_seed[r]};
      std::memcpy(h + kMmRepHead + r * rec, &q, rec);
    } else {
      const MmRep<double> q{b[0], b[1], b[2], 1.0 / b[0], 1.0 / b[1], 1.0 / b[2], kT, 0.0, sim->rep_seed[r]};
      std::memcpy(h + kMmRepHead + r * rec, &q, rec);
    }
  }
  const size_t off = mm_rep_offset(sim->n_ctypes * sim->n_ctypes, f32 ? sizeof(float) : sizeof(double));
  MYTHOS_HIP_TRY(hipMemcpyAsync((unsigned char*)sim->d_ceps.get() + off, h, tab, hipMemcpyHostToDevice, st));
  return MYTHOS_OK;
}

// The epsilon table with the Coulomb record behind it (ce: n_ctypes^2 + kCoulRec doubles) in the system's precision; for
// an ensemble with room for the replica table behind that, filled at once.
static int mm_upload_ceps(mythos_martini_sim* sim, const std::vector<double>& ce) {
  const int dtype = sim->sys->dtype;
  if (sim->n_rep == 0) return sim->d_ceps.upload_real(dtype, ce.data(), ce.size());
  const bool f32 = dtype == MYTHOS_F32;
  const size_t w = f32 ? sizeof(float) : sizeof(double), rec = f32 ? sizeof(MmRep<float>) : sizeof(MmRep<double>);
  if (int rc = sim->d_ceps.alloc(mm_rep_offset(sim->n_ctypes * sim->n_ctypes, w) + kMmRepHead + sim->n_rep * rec)) return rc;
  if (f32) {
    const std::vector<float> tmp(ce.begin(), ce.end());
    MYTHOS_HIP_TRY(hipMemcpy(sim->d_ceps.get(), tmp.data(), tmp.size() * w, hipMemcpyHostToDevice));
  } else {
    MYTHOS_HIP_TRY(hipMemcpy(sim->d_ceps.get(), ce.data(), ce.size() * w, hipMemcpyHostToDevice));
  }
  if (int rc = mm_upload_reps(sim, nullptr)) return rc;
  MYTHOS_HIP_TRY(hipStreamSynchronize(nullptr));
  return MYTHOS_OK;
}

// What the step kernels read in place of the system's own tables, derived from the system's reals AS THE DEVICE HOLDS
// THEM (the caller's doubles rounded to the system's precision): sigma^2 and epsilon of the types that occur (cs, ce:
// [C][C], C = max(1, used.size())), and per angle cos(theta0) for the G96 form, theta0 for the harmonic one.
static void mm_param_tables(const mythos_martini* sys, const std::vector<int>& used, std::vector<double>& cs, std::vector<double>& ce,
                            std::vector<double>& ref) {
  const int dtype = sys->dtype, T = sys->n_types;
  auto rounded = [dtype](double v) { return dtype == MYTHOS_F32 ? double(float(v)) : v; };
  const size_t C = std::max<size_t>(1, used.size());
  cs.assign(C * C, 0.0), ce.assign(C * C, 0.0);
  for (size_t p = 0; p < used.size(); ++p)
    for (size_t q = 0; q < used.size(); ++q) {
      // (squared in the kernel's own precision, as the kernel did)
      const double sg = rounded(sys->h_sigma[(size_t)used[p] * T + used[q]]);
      cs[p * C + q] = dtype == MYTHOS_F32 ? double(float(sg) * float(sg)) : sg * sg;
      ce[p * C + q] = rounded(sys->h_eps[(size_t)used[p] * T + used[q]]);
    }
  ref.resize(sys->h_angle_t0.size());
  for (size_t a = 0; a < ref.size(); ++a) {
    const double t0 = rounded(sys->h_angle_t0[a]);
    ref[a] = sys->angle_kind == 0 ? std::cos(t0) : t0;
  }
}

static int mm_upload_ceps(mythos_martini_sim* sim, const std::vector<double>& ce);

// mythos_martini_set_params replaced the system's parameter tables: the integrator's own follow at the head of its next
// call, in place - the handle, its resident state and its lists stay.  The epsilon table travels with the Coulomb record
// (and an ensemble's replica table), so mm_sync_charges is made to lay all of it out again.  Rare: synchronises.
static int mm_sync_params(mythos_martini_sim* sim, hipStream_t st) {
  const mythos_martini* m = sim->sys;
  if (sim->param_gen == m->param_gen) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipStreamSynchronize(st));
  std::vector<double> cs, ce, ref;
  mm_param_tables(m, sim->h_used, cs, ce, ref);
  if (sim->d_csig2.upload_real(m->dtype, cs.data(), cs.size()) || sim->d_angle_ref.upload_real(m->dtype, ref.data(), ref.size())) {
    set_error("mythos_martini_langevin: device allocation failed");
    return MYTHOS_ERR_HIP;
  }
  sim->h_ceps = ce;
  sim->charge_gen = m->charge_gen - 1;
  sim->param_gen = m->param_gen;
  return MYTHOS_OK;
}

// The integrator's view of the system's charges, brought up to date at the head of every call (load, advance, store,
// pressure) when mythos_martini_set_charges has changed them since: the charge classes, the packed types and the Coulomb
// record behind the epsilon table.  A resident frame is retyped in place.  Rare: synchronises.
static int mm_sync_charges(mythos_martini_sim* sim, hipStream_t st) {
  const mythos_martini* m = sim->sys;
  if (int rc = mm_sync_params(sim, st)) return rc;
  if (sim->charge_gen == m->charge_gen) return MYTHOS_OK;
  MYTHOS_HIP_TRY(hipStreamSynchronize(st));  // (launches that read the tables replaced below)
  const int n = m->n;
  std::vector<int> packed = sim->h_ctypes;
  std::vector<double> tab(kMaxChargeClasses, 0.0), ce = sim->h_ceps;
  double self = 0.0;  // sum q^2
  if (m->has_charge) {
    const std::vector<double>& q = m->h_charge;
    int n_cls = 1;  // class 0: no charge
    for (int i = 0; i < n; ++i) {
      int c = 0;
      while (c < n_cls && tab[c] != q[i]) ++c;
      if (c == n_cls) {
        if (n_cls == kMaxChargeClasses) {  // (mythos_martini_set_charges refuses such a system)
          set_error("mythos_martini_langevin: more distinct charge values than the charge table holds");
          return MYTHOS_ERR_INVALID_ARGUMENT;
        }
        tab[n_cls++] = q[i];
      }
      packed[i] += kMaxTypes * c;
      self += q[i] * q[i];
    }
    const RfConst<double> c = m->rf<double>();
    const double rec[4] = {c.pref, c.k_rf, c.c_rf, -0.5 * c.pref * c.c_rf * self};
    ce.insert(ce.end(), rec, rec + 4);
    ce.insert(ce.end(), tab.begin(), tab.end());
  }
  ce.resize(sim->h_ceps.size() + kCoulRec, 0.0);
  if (sim->d_ctypes.upload(packed) || mm_upload_ceps(sim, ce)) {
    set_error("mythos_martini_langevin: device allocation failed");
    return MYTHOS_ERR_HIP;
  }
  sim->coul = m->has_charge;
  if (sim->resident && sim->n_rep > 0) {
    const int tb = (sim->n_all() + 255) / 256;
    if (m->dtype == MYTHOS_F32)
      hipLaunchKernelGGL(mm_retype_ens_kernel<float>, dim3(tb), dim3(256), 0, st, n, sim->n_rep, sim->d_ctypes.get(), (float4*)sim->frame[sim->cur].get());
    else
      hipLaunchKernelGGL(mm_retype_ens_kernel<double>, dim3(tb), dim3(256), 0, st, n, sim->n_rep, sim->d_ctypes.get(), (double4*)sim->frame[sim->cur].get());
    MYTHOS_HIP_TRY(hipGetLastError());
  } else if (sim->resident) {
    const int tb = (n + 255) / 256;
    if (m->dtype == MYTHOS_F32)
      hipLaunchKernelGGL(mm_retype_kernel<float>, dim3(tb), dim3(256), 0, st, n, sim->d_ctypes.get(), (float4*)sim->frame[sim->cur].get());
    else
      hipLaunchKernelGGL(mm_retype_kernel<double>, dim3(tb), dim3(256), 0, st, n, sim->d_ctypes.get(), (double4*)sim->frame[sim->cur].get());
    MYTHOS_HIP_TRY(hipGetLastError());
  }
  if (int rc = sim->d_epart.grow((size_t)sim->copies() * ((n + kMmPPB - 1) / kMmPPB) * kMmTraceCoul)) return rc;
  sim->charge_gen = m->charge_gen;
  return MYTHOS_OK;
}

// The external kick of view v on the velocities `vel`, forces taken at pos: the COM rows of the pull groups, then the
// gather-and-kick with one stamp word per workgroup.  The one place these two kernels are launched - in front of a step
// launch, and by mythos_martini_langevin_eval_external with c_dt < 0 (factor 1) on zeroed velocities.  A set without pull
// coordinates has no COM launch.
template <typename R>
static void mr_launch_kick(const MrView& v, const R* pos, int stride, double* rows, double c_dt, double step, typename Real4<R>::type* vel,
                           const int* flags, const int* halt_words, int k, unsigned long long stamp, unsigned long long* stamps,
                           hipStream_t st) {
  if (v.n_pull > 0) hipLaunchKernelGGL(mr_com_kernel<R>, dim3(v.n_rep * v.n_groups), dim3(256), 0, st, v, pos, stride, rows);
  const int blocks = (int)(((long long)v.n_rep * v.n_entries + 255) / 256);
  if (blocks > 0)
    hipLaunchKernelGGL((mr_kick_kernel<R, typename Real4<R>::type>), dim3(blocks), dim3(256), 0, st, v, pos, stride, (const double*)rows, c_dt,
                       step, vel, flags, halt_words, k, stamp, stamps);
}

// caller's (n, 3) arrays -> the resident frame; the list of a previous state does not carry over
template <typename R>
static int mm_load_typed(mythos_martini_sim* sim, const R* pos, const R* v, const double* box, hipStream_t st) {
  using V4 = typename Real4<R>::type;
  mythos_martini* m = sim->sys;
  const int n = m->n, tb = (n + 255) / 256;
  if (sim->n_rep > 0) {  // box: [n_rep][3]
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));  // (the staging buffer of the replica tables)
    sim->rep_box.assign(box, box + 3 * (size_t)sim->n_rep);
    if (int rc = mm_upload_reps(sim, st)) return rc;
    hipLaunchKernelGGL(mm_pack_ens_kernel<R>, dim3((sim->n_all() + 255) / 256), dim3(256), 0, st, n, sim->n_rep, pos, v, sim->d_ctypes.get(),
                       (const R*)sim->d_inv_mass.get(), (V4*)sim->frame[0].get(), (V4*)sim->vel.get());
  } else {
    for (int k = 0; k < 3; ++k) sim->box[k] = box[k];
    hipLaunchKernelGGL(mm_pack_kernel<R>, dim3(tb), dim3(256), 0, st, n, pos, v, sim->d_ctypes.get(), (const R*)sim->d_inv_mass.get(),
                       (V4*)sim->frame[0].get(), (V4*)sim->vel.get());
  }
  MYTHOS_HIP_TRY(hipGetLastError());
  sim->cur = 0;
  sim->resident = true;
  sim->list_valid = false;
  sim->open = false;
  sim->since_build = 0;
  sim->rst.stamp_stale = true;
  return MYTHOS_OK;
}

// n_steps on the resident state: md_drive (md_driver.h) runs the launches, the list's rebuild schedule and the recovery
// from a halt, as for oxDNA.  What is MARTINI's is here: the list builds and the pruned rows.  Rows with energies
// (e_trace != NULL) come from the energy-trace instantiation at x_k plus a reduction launch; rows without are written by
// the launch that produces the saved state.
template <typename R>
static int mm_advance_typed(mythos_martini_sim* sim, int n_steps, int save_every, bool close, R* traj_pos, double* e_trace,
                            hipStream_t st) {
  using V4 = typename Real4<R>::type;
  mythos_martini* m = sim->sys;
  const int n = m->n, n_all = sim->n_all();  // (the kernels take n, the beads of one copy)
  const bool ens = sim->n_rep > 0;
  const int blocks_per_rep = (n + kMmPPB - 1) / kMmPPB;
  const int blocks = sim->copies() * blocks_per_rep, grid = 8 * ((blocks + 7) / 8);
  const MmConst<R> K = mm_const<R>(sim, sim->box_of(0));
  V4* fr[2] = {(V4*)sim->frame[0].get(), (V4*)sim->frame[1].get()};
  V4* vel = (V4*)sim->vel.get();
  const bool inner_on = mm_inner_on(sim);
  // the pruned rows share the Verlet rows' stride (a pruned row is a subset of its row: it cannot overflow)
  auto ensure_inner = [&]() -> int {
    if (!inner_on) return 0;
    if (int rc = sim->d_row_len_in.grow((size_t)n_all)) return rc;
    return sim->d_rows_in.grow((size_t)n_all * sim->list.stride);  // (a stride only grows)
  };
  if (int rc = ensure_inner()) return rc;
  const bool coul = sim->coul;
  const size_t lds = ((size_t)2 * sim->n_ctypes * sim->n_ctypes + (coul ? kCoulRec : 0)) * sizeof(R);
  auto launch_step = [&](int k, const LaunchRow& row) {
    const int cur = row.cur;
    R kick_close = R(row.kick_close);
    int do_step = row.do_step;
    R* tp = ((row.save || row.save_next) && traj_pos) ? traj_pos + (size_t)row.sidx * n_all * 3 : nullptr;
    // pruned rows: the launch d steps after the Verlet rows were built prunes when d is a multiple of inner_every (so
    // the first launch on new rows does) and walks the pruned rows otherwise
    const bool emit = inner_on && ((k - row.built_at) % sim->inner_every == 0);
    const int* walk_rows = (inner_on && !emit) ? sim->d_rows_in.get() : sim->list.d_rows.get();
    const int* walk_len = (inner_on && !emit) ? sim->d_row_len_in.get() : sim->d_row_len.get();
    int* emit_rows = emit ? sim->d_rows_in.get() : nullptr;
    int* emit_len = emit ? sim->d_row_len_in.get() : nullptr;
    // the external kick c dt F_ext / m of this launch (martini_restraints.h), queued in front of it, outside the dispatch's event pair
    auto ext_kick = [&](double c, bool closing) {
      MmRestraints& q = sim->rst;
      if (q.stamp_stale) {
        (void)hipMemsetAsync(q.d_stamp.get(), 0, sizeof(unsigned long long) * (size_t)q.kick_blocks(), st);
        q.stamp_stale = false;
      }
      const unsigned long long stamp = 2ull * (unsigned long long)(sim->step + k) + (closing ? 1ull : 0ull) + 1ull;
      mr_launch_kick<R>(q.view, (const R*)fr[cur], 4, q.d_rows.get(), c * sim->dt, double(sim->step + k), vel, sim->d_flags.get(),
                        sim->list.d_overflow.get(), k, stamp, q.d_stamp.get(), st);
    };
    // A launch that saves an energy row takes the row's kinetic energy behind its closing half kick.  Under a set of
    // restraints the external kick of a whole launch - closing and opening half together - would already be in those
    // velocities, so such a launch is issued as the two launches a call that closes and the call behind it issue at this
    // step index: close with the row (kick_close, no step), then open (no closing kick, the step), each behind its own
    // external half kick, whose stamps differ in the closing bit as they do across two calls.  The forces are evaluated
    // twice, on rows with energies only; both launches walk the same rows, read frame cur and test the same halt words.
    const bool split = sim->rst.installed && row.save && row.do_step != 0;
    if (sim->rst.installed) ext_kick(split ? double(row.kick_close) : double(row.kick_close) + 0.5 * row.do_step, row.kick_close != 0.0f);
    if (split) do_step = 0;
#define MM_ARGS                                                                                                           \
  n, K, (const V4*)fr[cur], fr[cur ^ 1], vel, walk_rows, walk_len, sim->list.stride, (const R*)sim->d_csig2.get(),        \
      (const R*)sim->d_ceps.get(), m->d_bead_bonds.get(), m->d_bead_angles.get(), m->d_bonds.get(),                       \
      (const R*)m->d_bond_k.get(), (const R*)m->d_bond_r0.get(), m->d_angles.get(), (const R*)m->d_angle_k.get(),         \
      (const R*)sim->d_angle_ref.get(), kick_close, do_step, sim->seed, (uint64_t)(sim->step + k),                        \
      (const V4*)sim->ref_pos.get(), sim->d_flags.get(), tp, sim->d_epart.get(), sim->list.d_overflow.get(), k,           \
      emit_rows, emit_len, sim->d_bb_partner.get(), sim->d_ba_partner.get()
    auto go_ens = [&](auto save_tag, auto emit_tag, auto coul_tag, auto ens_tag) {
      constexpr bool SV = decltype(save_tag)::value, EM = decltype(emit_tag)::value, CL = decltype(coul_tag)::value;
      constexpr bool EN = decltype(ens_tag)::value;
      if (row.ea) {
        hipExtLaunchKernelGGL((martini_md_step_kernel<R, SV, EM, CL, EN>), dim3(grid), dim3(kMmBlock), lds, st, row.ea, row.eb, 0, MM_ARGS);
      } else {
        hipLaunchKernelGGL((martini_md_step_kernel<R, SV, EM, CL, EN>), dim3(grid), dim3(kMmBlock), lds, st, MM_ARGS);
      }
    };
#undef MM_ARGS
    // an ensemble: the instantiations that read the replica table
    auto go_coul = [&](auto save_tag, auto emit_tag, auto coul_tag) {
      if (ens) go_ens(save_tag, emit_tag, coul_tag, std::true_type{}); else go_ens(save_tag, emit_tag, coul_tag, std::false_type{});
    };
    // the system holds charges: the instantiations with reaction-field Coulomb
    auto go = [&](auto save_tag, auto emit_tag) {
      if (coul) go_coul(save_tag, emit_tag, std::true_type{}); else go_coul(save_tag, emit_tag, std::false_type{});
    };
    if (row.save) {
      if (emit) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{});
      if (ens && coul)
        hipLaunchKernelGGL(mm_reduce_trace_ens_kernel<kMmTraceCoul>, dim3(sim->n_rep), dim3(256), 0, st, sim->d_epart.get(), blocks_per_rep,
                           e_trace + (size_t)row.sidx * sim->n_rep * kMmTraceCoul);
      else if (ens)
        hipLaunchKernelGGL(mm_reduce_trace_ens_kernel<kMmTrace>, dim3(sim->n_rep), dim3(256), 0, st, sim->d_epart.get(), blocks_per_rep,
                           e_trace + (size_t)row.sidx * sim->n_rep * kMmTrace);
      else if (coul)
        hipLaunchKernelGGL(reduce_trace_kernel<kMmTraceCoul>, dim3(1), dim3(256), 0, st, sim->d_epart.get(), blocks,
                           e_trace + (size_t)row.sidx * kMmTraceCoul);
      else
        hipLaunchKernelGGL(reduce_trace_kernel<kMmTrace>, dim3(1), dim3(256), 0, st, sim->d_epart.get(), blocks,
                           e_trace + (size_t)row.sidx * kMmTrace);
    } else {
      if (emit) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{});
    }
    if (split) {
      ext_kick(0.5, false);
      kick_close = R(0), do_step = 1, tp = nullptr;
      if (emit) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{});
    }
  };
  MdDrive d;
  d.who = "mythos_martini_langevin_run";
  d.n_steps = n_steps, d.save_every = save_every, d.close = close;
  d.energy_rows = save_every > 0 && e_trace != nullptr;
  d.plain_rows = save_every > 0 && e_trace == nullptr && traj_pos != nullptr;
  d.dynamic_list = true;
  d.halt_words = sim->list.d_overflow.get();
  d.row_stride = &sim->list.stride;
  d.skin = sim->skin;
  if (inner_on)
    d.give_up_hint = ", or the margin of the pruned rows (" + std::to_string(sim->inner_margin) + ") for one pruning in " +
                     std::to_string(sim->inner_every) + " steps";
  d.st = st;
  return md_drive(
      *sim, d, launch_step, [&](int buf) { return mm_rebuild<R>(sim, fr[buf], st); },
      [&](int buf) -> int {
        auto build = [&] { return mm_rebuild<R>(sim, fr[buf], st); };
        if (int rc = list_build_until_fit(sim->list, n_all, build, true, "mythos_martini_langevin_run: neighbour build", st)) return rc;
        return ensure_inner();  // (the rows may have grown)
      },
      [] { return 0; });  // (no MARTINI launch aborts)
}

// the resident frame -> caller's arrays (asynchronous on st); an open frame gets its closing half kick first
template <typename R>
static int mm_store_typed(mythos_martini_sim* sim, R* pos, R* v, hipStream_t st) {
  using V4 = typename Real4<R>::type;
  const int n = sim->n_all();
  const int rc = sim->open ? mm_advance_typed<R>(sim, 0, 0, true, nullptr, nullptr, st) : MYTHOS_OK;
  hipLaunchKernelGGL(mm_unpack_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, st, n, (const V4*)sim->frame[sim->cur].get(), (const V4*)sim->vel.get(), pos, v);
  MYTHOS_HIP_TRY(hipGetLastError());
  return rc;
}

}  // namespace mythos

#include "martini_npt.inc"
#include "martini_exchange.inc"
#include "martini_restraints.inc"
#include "martini_window_exchange.inc"

namespace mythos {

// n_steps with events - coupling under a barostat, and temperature or window exchange: chunks that end at the next event
// step (absolute step counter), the next saved row (counted from the call's first step) or the end of the call
// (mm_event_chunk), each one call of mm_advance_typed - md_drive as it is - with what mm_chunk_plan says.  A chunk that
// ends at an event closes (the event needs the closed state; a temperature event U(x_s) too); every other boundary
// leaves the frame open, and the launches on either side of it are those of one longer call.  Inside a step: the saved
// row - the state BEFORE the step's events, with the box, ladder and windows it was integrated under -, then the exchange
// on U and the box of (x_s, box_s), then the coupling with the new kT' and the rescaled velocities, each event with its own
// synchronisation.  What is refused comes first, then the events' buffers, allocated at the first call that needs them.
template <typename R>
static int mm_advance_chunked(mythos_martini_sim* sim, int n_steps, int save_every, bool close, R* traj_pos, double* e_trace, hipStream_t st) {
  MmBarostat& b = sim->baro;
  const bool baro = mm_barostat_on(sim);
  const MmExchangeKind kind = mm_window_exchange_on(sim) ? kMmWindowExchange : (mm_exchange_on(sim) ? kMmTemperatureExchange : kMmNoExchange);
  const int exchange_every = kind == kMmWindowExchange ? sim->wx.every : (kind == kMmTemperatureExchange ? sim->xchg.every : 0);
  double p = 0.0;  // of the temperature exchange's work term
  if (kind == kMmWindowExchange) {
    if (!sim->rst.installed) {
      set_error("mythos_martini_langevin_advance: window exchange is on and no set of restraints is installed: there are no windows to "
                "exchange (mythos_martini_langevin_set_restraints first, or switch window exchange off)");
      return MYTHOS_ERR_NOT_READY;
    }
    if (int rc = mm_wx_buffers(sim)) return rc;
  } else if (kind == kMmTemperatureExchange) {
    if (int rc = mm_xchg_pressure(baro, b.coupling, b.ref_p, b.beta, &p, "mythos_martini_langevin_advance")) return rc;
    if (int rc = mm_exchange_buffers(sim)) return rc;
  }
  if (n_steps == 0) return mm_advance_typed<R>(sim, 0, save_every, close, traj_pos, e_trace, st);
  const size_t row_reals = (size_t)sim->n_all() * 3;
  int done = 0, rows = 0, rebuilds = 0, recoveries = 0, launches = 0;
  while (done < n_steps) {
    const MmEventChunk c = mm_event_chunk(sim->step, baro ? b.every : 0, exchange_every, done, n_steps, save_every);
    const MmChunkPlan plan = mm_chunk_plan(c, close, kind, e_trace != nullptr);
    double* e_row = plan.energy == kMmCallerRow    ? e_trace + mm_row_offset(rows, sim->copies(), sim->trace_width())
                    : plan.energy == kMmScratchRow ? sim->ladder.d_etrace.get()
                                                   : nullptr;
    const int rc = mm_advance_typed<R>(sim, c.len, plan.save_every, plan.close, (c.save && traj_pos) ? traj_pos + rows * row_reals : nullptr, e_row, st);
    rebuilds += sim->last_rebuilds, recoveries += sim->last_recoveries, launches += sim->last_launches;
    sim->last_rebuilds = rebuilds, sim->last_recoveries = recoveries, sim->last_launches = launches;
    if (rc) return rc;
    if (c.save) mm_push_row(sim), ++rows;
    if (c.exchange)
      if (int re = kind == kMmWindowExchange ? mm_window_exchange_event<R>(sim, st) : mm_exchange_event<R>(sim, e_row, p, st)) return re;
    if (c.couple)
      if (int re = mm_pressure_typed<R>(sim, true, st)) return re;
    done += c.len;
  }
  return MYTHOS_OK;
}

}  // namespace mythos

extern "C" {

void mythos_martini_langevin_destroy(mythos_martini_sim_t* s) { delete s; }

}  // extern "C"

namespace {

// n_rep = 0: the single copy of mythos_martini_langevin_create (kT, seeds: one value each)
mythos_martini_sim_t* mm_create(mythos_martini_t* sys, int n_rep, double dt, const double* kTs, double gamma, const double* mass,
                                const uint64_t* seeds, const char* who) {
  const double kT = kTs[0];
  const uint64_t seed = seeds ? seeds[0] : 0;
  if (select_device(sys->device, who)) return nullptr;
  auto s = std::make_unique<mythos_martini_sim>();
  s->sys = sys, s->device = sys->device, s->dt = dt, s->kT = kT, s->gamma = gamma, s->seed = seed;
  s->rebuild_every = 10;
  if (n_rep > 0) {
    s->n_rep = n_rep;
    s->rep_kT.assign(kTs, kTs + n_rep);
    s->rep_box.assign(3 * (size_t)n_rep, 0.0);
    s->rep_seed.assign((size_t)n_rep, 0);
    for (int r = 0; seeds && r < n_rep; ++r) s->rep_seed[r] = seeds[r];
    s->ladder.kT = s->rep_kT;
    for (MmPairExchange* x : {&s->xchg, &s->wx}) {
      x->of_slot.resize((size_t)n_rep);
      x->attempts.resize((size_t)std::max(0, n_rep - 1));
      x->accepts.resize((size_t)std::max(0, n_rep - 1));
      x->identity();
    }
  }
  const int copies = s->copies();
  const int n = sys->n, dtype = sys->dtype;
  const size_t w = dtype == MYTHOS_F32 ? sizeof(float) : sizeof(double);
  std::vector<double> im(n);
  for (int i = 0; i < n; ++i) {
    const double mi = mass ? mass[i] : 72.0;  // MARTINI's standard bead mass (amu)
    if (!(mi > 0)) {
      set_error(std::string(who) + ": masses must be positive");
      return nullptr;
    }
    im[i] = 1.0 / mi;
    s->h_mass.push_back(mi);
  }
  // partners per incidence slot
  const std::vector<int>&bb = sys->h_bead_bonds, &ba = sys->h_bead_angles;
  std::vector<int> pb(bb.size(), -1);
  std::vector<int2> pa(ba.size(), int2{-1, -1});
  for (size_t k = 0; k < bb.size(); ++k)
    if (bb[k] >= 0) pb[k] = sys->h_bonds[2 * (size_t)(bb[k] >> 1) + (1 - (bb[k] & 1))];
  for (size_t k = 0; k < ba.size(); ++k)
    if (ba[k] >= 0) {
      const int* t = &sys->h_angles[3 * (size_t)(ba[k] >> 2)];
      const int role = ba[k] & 3;
      pa[k] = role == 0 ? int2{t[1], t[2]} : (role == 1 ? int2{t[0], t[2]} : int2{t[0], t[1]});
    }
  // the compact type tables (mm_param_tables)
  const int T = sys->n_types;
  std::vector<int> types = sys->h_types, cmap(T, -1), used;
  for (int t : types)
    if (t >= 0 && t < T && cmap[t] < 0) cmap[t] = 0;
  for (int t = 0; t < T; ++t)
    if (cmap[t] == 0) cmap[t] = (int)used.size(), used.push_back(t);
  const int C = std::max<int>(1, (int)used.size());
  std::vector<double> cs, ce, ref;
  mm_param_tables(sys, used, cs, ce, ref);
  for (int& t : types) t = (t >= 0 && t < T) ? cmap[t] : 0;
  s->n_ctypes = C;
  s->h_ctypes = types;
  s->h_used = used;
  s->h_ceps = ce;
  s->param_gen = sys->param_gen;
  ce.resize(ce.size() + kCoulRec, 0.0);  // the Coulomb record, all zero until the system holds charges (mm_sync_charges)
  const size_t na = (size_t)copies * n;  // per-bead state: every copy's
  const int blocks = copies * ((n + kMmPPB - 1) / kMmPPB);
  if (!md_run_create(*s) || s->frame[0].alloc(na * 4 * w) || s->frame[1].alloc(na * 4 * w) || s->vel.alloc(na * 4 * w) ||
      s->ref_pos.alloc(na * 4 * w) || rows_reserve(s->list, (int)na, kMmStride0) || s->d_row_len.alloc(na) ||
      s->list.d_overflow.alloc(kOverflowWords) || s->d_epart.alloc((size_t)blocks * kMmTrace) ||
      s->d_inv_mass.upload_real(dtype, im.data(), im.size()) || s->d_bb_partner.upload(pb) || s->d_ba_partner.upload(pa) ||
      s->d_ctypes.upload(types) || s->d_csig2.upload_real(dtype, cs.data(), cs.size()) ||
      mm_upload_ceps(s.get(), ce) || s->d_angle_ref.upload_real(dtype, ref.data(), ref.size()) ||
      hipMemset(s->list.d_overflow.get(), 0, kOverflowWords * sizeof(int)) != hipSuccess) {
    set_error(std::string(who) + ": device allocation failed");
    return nullptr;
  }
  return s.release();
}

}  // namespace

extern "C" {

mythos_martini_sim_t* mythos_martini_langevin_create(mythos_martini_t* sys, double dt, double kT, double gamma,
                                                     const double* mass, uint64_t seed) {
  if (!sys || !(dt > 0) || !(kT > 0) || !(gamma >= 0)) {
    set_error("mythos_martini_langevin_create: invalid argument");
    return nullptr;
  }
  return mm_create(sys, 0, dt, &kT, gamma, mass, &seed, "mythos_martini_langevin_create");
}

int mythos_martini_ensemble_check(int n, int n_rep, const double* kT, double r_cut, double skin, const double* boxes) {
  return mm_ensemble_check(n, n_rep, kT, r_cut, skin, boxes, "mythos_martini_ensemble_check");
}

mythos_martini_sim_t* mythos_martini_langevin_create_ensemble(mythos_martini_t* sys, int n_rep, double dt, const double* kT, double gamma,
                                                              const double* mass, const uint64_t* seeds) {
  const char* who = "mythos_martini_langevin_create_ensemble";
  if (!sys || !(dt > 0) || !(gamma >= 0)) {
    set_error(std::string(who) + ": invalid argument");
    return nullptr;
  }
  if (mm_ensemble_check(sys->n, n_rep, kT, sys->r_cut, 0.0, nullptr, who)) return nullptr;
  return mm_create(sys, n_rep, dt, kT, gamma, mass, seeds, who);
}

int mythos_martini_langevin_set_neighbor_policy(mythos_martini_sim_t* s, double skin, int rebuild_every) {
  if (!s || !(skin > 0) || rebuild_every < 1) {
    set_error("mythos_martini_langevin_set_neighbor_policy: skin > 0 and rebuild_every >= 1 required");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->skin = skin;
  s->rebuild_every = rebuild_every;
  s->list_fitted = false;  // another list range: size rows and buckets again at the next run
  s->list_valid = false;
  return MYTHOS_OK;
}

int mythos_martini_langevin_set_inner_list(mythos_martini_sim_t* s, double margin, int every) {
  if (!s || every < 0) {
    set_error("mythos_martini_langevin_set_inner_list: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->inner_margin = margin;
  s->inner_every = every;
  s->list_valid = false;  // the schedule of pruning starts again with the next build
  return MYTHOS_OK;
}

int mythos_martini_langevin_init_velocities(mythos_martini_sim_t* s, void* vel, mythos_stream_t stream) {
  if (!s || !vel) {
    set_error("mythos_martini_langevin_init_velocities: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  // (an ensemble: replica r's slice of vel [n_rep][n][3] is what a single integrator with its kT and seed draws)
  for (int r = 0; r < s->copies(); ++r) {
    const double kT = s->n_rep > 0 ? s->rep_kT[r] : s->kT;
    const uint64_t seed = s->n_rep > 0 ? s->rep_seed[r] : s->seed;
    const size_t off = 3 * (size_t)r * s->sys->n;
    if (s->sys->dtype == MYTHOS_F32)
      hipLaunchKernelGGL(mm_init_velocities_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream, s->sys->n, float(kT),
                         (const float*)s->d_inv_mass.get(), seed, (float*)vel + off);
    else
      hipLaunchKernelGGL(mm_init_velocities_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, s->sys->n, kT,
                         (const double*)s->d_inv_mass.get(), seed, (double*)vel + off);
  }
  MYTHOS_HIP_TRY(hipGetLastError());
  return MYTHOS_OK;
}

namespace {

// (an ensemble: box [n_rep][3], every replica's checked, the message names the replica)
int mm_check_box(const mythos_martini_sim_t* s, const double* box, const char* who) {
  const double rl = s->sys->r_cut + s->skin;
  if (s->n_rep == 0) return mm_box_fits(box, rl, who);
  for (int r = 0; r < s->n_rep; ++r)
    if (int rc = mm_box_fits(box ? box + 3 * (size_t)r : nullptr, rl, std::string(who) + ": replica " + std::to_string(r))) return rc;
  return MYTHOS_OK;
}

int mm_load(mythos_martini_sim_t* s, const void* pos, const void* vel, const double* box, hipStream_t st) {
  if (int rc = mr_check_load_box(s, box)) return rc;
  if (int rc = mm_sync_charges(s, st)) return rc;
  return s->sys->dtype == MYTHOS_F32 ? mm_load_typed<float>(s, (const float*)pos, (const float*)vel, box, st)
                                     : mm_load_typed<double>(s, (const double*)pos, (const double*)vel, box, st);
}

// Without events the call is ONE mm_advance_typed - one md_drive - with the caller's save_every; its rows all have the box,
// ladder and windows of the load, and a call that failed has none.
int mm_advance(mythos_martini_sim_t* s, int n_steps, int save_every, bool close, void* traj, double* e_trace, hipStream_t st) {
  if (int rc = mm_sync_charges(s, st)) return rc;
  mm_clear_logs(s);
  const bool f32 = s->sys->dtype == MYTHOS_F32;
  if (mm_barostat_on(s) || mm_exchange_on(s) || mm_window_exchange_on(s))
    return f32 ? mm_advance_chunked<float>(s, n_steps, save_every, close, (float*)traj, e_trace, st)
               : mm_advance_chunked<double>(s, n_steps, save_every, close, (double*)traj, e_trace, st);
  const int rc = f32 ? mm_advance_typed<float>(s, n_steps, save_every, close, (float*)traj, e_trace, st)
                     : mm_advance_typed<double>(s, n_steps, save_every, close, (double*)traj, e_trace, st);
  for (int r = 0; rc == MYTHOS_OK && save_every > 0 && r < n_steps / save_every; ++r) mm_push_row(s);
  return rc;
}
int mm_store(mythos_martini_sim_t* s, void* pos, void* vel, hipStream_t st) {
  if (int rc = mm_sync_charges(s, st)) return rc;
  return s->sys->dtype == MYTHOS_F32 ? mm_store_typed<float>(s, (float*)pos, (float*)vel, st) : mm_store_typed<double>(s, (double*)pos, (double*)vel, st);
}

}  // namespace

int mythos_martini_langevin_run(mythos_martini_sim_t* s, void* pos, void* vel, const double* box, int n_steps,
                                int save_every, void* traj_pos, double* e_trace, mythos_stream_t stream) {
  if (!s || !pos || !vel || n_steps < 0 || save_every < 0) {
    set_error("mythos_martini_langevin_run: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_check_box(s, box, "mythos_martini_langevin_run")) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mm_load(s, pos, vel, box, st)) return rc;
  const int rc = mm_advance(s, n_steps, save_every, true, traj_pos, e_trace, st);
  // the state of the last valid step goes back to the caller whatever the run reported
  if (s->resident) {
    if (int rs = mm_store(s, pos, vel, st)) return rc ? rc : rs;
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
  }
  return rc;
}

int mythos_martini_langevin_load(mythos_martini_sim_t* s, const void* pos, const void* vel, const double* box, mythos_stream_t stream) {
  if (!s || !pos || !vel) {
    set_error("mythos_martini_langevin_load: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = mm_check_box(s, box, "mythos_martini_langevin_load")) return rc;
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return mm_load(s, pos, vel, box, (hipStream_t)stream);
}

int mythos_martini_langevin_advance(mythos_martini_sim_t* s, int n_steps, int save_every, void* traj_pos, double* e_trace,
                                    mythos_stream_t stream) {
  if (!s || n_steps < 0 || save_every < 0) {
    set_error("mythos_martini_langevin_advance: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->resident) {
    set_error("mythos_martini_langevin_advance: no resident state (call mythos_martini_langevin_load first; a run that ended in a "
              "numeric error drops its state)");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return mm_advance(s, n_steps, save_every, false, traj_pos, e_trace, (hipStream_t)stream);
}

int mythos_martini_langevin_store(mythos_martini_sim_t* s, void* pos, void* vel, mythos_stream_t stream) {
  if (!s || !pos || !vel) {
    set_error("mythos_martini_langevin_store: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->resident) {
    set_error("mythos_martini_langevin_store: no resident state");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return mm_store(s, pos, vel, (hipStream_t)stream);
}

int64_t mythos_martini_langevin_get_step(const mythos_martini_sim_t* s) { return md_get_step(s); }

int mythos_martini_langevin_restart(mythos_martini_sim_t* s, const uint64_t* seeds, int64_t step) {
  if (!s || !seeds || step < 0) {
    set_error("mythos_martini_langevin_restart: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  s->seed = seeds[0];
  for (int r = 0; r < s->n_rep; ++r) s->rep_seed[r] = seeds[r];
  if (s->n_rep > 0) {  // the ladder back to the identity, every slot at the kT it was created with; the counts to zero
    s->xchg.identity();
    mm_apply_ladder(s);
  }
  s->step = step;
  s->rst.stamp_stale = true;
  s->resident = false;  // (an ensemble's replica table takes the seeds at the load that has to follow)
  s->list_valid = false;
  s->open = false;
  return MYTHOS_OK;
}

int mythos_martini_langevin_last_rebuilds(const mythos_martini_sim_t* s, int* scheduled) {
  return md_last_count(s, &MdRun::last_rebuilds, scheduled, "mythos_martini_langevin_last_rebuilds");
}

int mythos_martini_langevin_last_kernel_ms(const mythos_martini_sim_t* s, double* kernel_ms, double* loop_ms_per_launch,
                                           int* launches, int* samples) {
  return md_last_kernel_ms(s, kernel_ms, loop_ms_per_launch, launches, samples, "mythos_martini_langevin_last_kernel_ms");
}

int mythos_martini_langevin_neighbor_stats(const mythos_martini_sim_t* s, int* max_row, double* mean_row) {
  if (!s) {
    set_error("mythos_martini_langevin_neighbor_stats: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  return row_stats(s->d_row_len.get(), s->n_all(), 0, max_row, mean_row);
}

int mythos_martini_langevin_get_rows(const mythos_martini_sim_t* s, int which, int32_t* rows, int32_t* row_len, int* stride) {
  if (!s || (which != 0 && which != 1)) {
    set_error("mythos_martini_langevin_get_rows: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const int* d_rows = which == 0 ? s->list.d_rows.get() : s->d_rows_in.get();
  const int* d_len = which == 0 ? s->d_row_len.get() : s->d_row_len_in.get();
  if (stride) *stride = s->list.stride;
  if (!rows && !row_len) return MYTHOS_OK;
  if (!d_rows || !d_len || !s->list_valid) {
    set_error(which == 0 ? "mythos_martini_langevin_get_rows: no list has been built"
                         : "mythos_martini_langevin_get_rows: no pruned rows (switched off, or no step taken yet)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  MYTHOS_HIP_TRY(hipDeviceSynchronize());
  if (rows) MYTHOS_HIP_TRY(hipMemcpy(rows, d_rows, (size_t)s->n_all() * s->list.stride * sizeof(int), hipMemcpyDeviceToHost));
  if (row_len) MYTHOS_HIP_TRY(hipMemcpy(row_len, d_len, (size_t)s->n_all() * sizeof(int), hipMemcpyDeviceToHost));
  return MYTHOS_OK;
}

int mythos_martini_langevin_last_recoveries(const mythos_martini_sim_t* s, int* recoveries) {
  return md_last_count(s, &MdRun::last_recoveries, recoveries, "mythos_martini_langevin_last_recoveries");
}

int mythos_martini_langevin_set_timing(mythos_martini_sim_t* s, int samples) {
  return md_set_timing(s, samples, "mythos_martini_langevin_set_timing");
}

}  // extern "C"
