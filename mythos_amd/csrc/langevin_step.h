// The fused step kernel of the oxDNA Langevin integrator and its device helpers: device code only.  The host side - which
// instantiation a launch takes, and its arguments - is advance_typed (langevin_core.inc) with md_plan.h.
//
// Rigid-body Langevin MD for oxDNA: one fused kernel per time step.
//
// Replaces the hot loop of the reference, jax.lax.scan(step_fn) with
// step_fn = jax_md.simulate.nvt_langevin on RigidBody states
// (mythos/simulators/jax_md/jaxmd.py:73-94).  jax_md (third party, not in the reference tree)
// advances one step as  B(dt/2) A(dt/2) O(dt) A(dt/2) [force] B(dt/2):
//   B  p += h F,  Pi += h F_q            (F_q = -dU/dq, quaternion conjugate momentum Pi)
//   A  x += h p/m, free rotor by the NO_SQUISH splitting R3(h/2) R2(h/2) R1(h) R2(h/2) R3(h/2)
//   O  p = c1 p + c2 sqrt(m) xi,  body angular momentum L = c1 L + c2 sqrt(I) xi,
//      c1 = exp(-gamma dt), c2 = sqrt(kT (1 - c1^2))
// Here the rotational state is the body-frame angular momentum L_k = 1/2 (P_k q).Pi, for which
// the kick is the body torque and the free rotor is a rotation about a principal axis; the two
// forms are the same map for a unit quaternion.
//
// Fusion: the kernel that evaluates F(x_k) first closes step k-1 (second half kick), optionally
// emits the snapshot / energies of x_k, then opens step k (half kick, A, O, A) and writes
// x_{k+1} to the other buffer of a ping-pong pair (other workgroups are still reading x_k).
// One launch per MD step; a run of K steps costs K+1 force evaluations.
//
// Per nucleotide per step (fp32): read + write the expanded frame (centre hi + lo, a1, a3, backbone
// offset, quaternion) and the momenta, read the neighbour row and the neighbours' frames through L2.
// Algorithmic HBM bytes are stated in DESIGN.md; the working set of a 12 kbp duplex (a few MB) is
// L2 / Infinity-Cache resident, the kernel is bound by VALU issue and latency, not by bytes.
//
// (MYTHOS_LEAN_MATH, which langevin_core.inc sets in front of every include, chooses the forms oxdna_math.h gives these
// kernels.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "oxdna_gather.h"
#include "philox.h"

namespace mythos {

template <typename R>
struct LangevinConst {
  R dt, half_dt;
  R inv_mass;
  R inv_inertia[3];
  R c1_t, c2_t;     // translational OU: p = c1 p + c2 xi   (c2 includes sqrt(m))
  R c1_r, c2_r[3];  // rotational OU per principal axis     (c2 includes sqrt(I_k))
  R skin_half_sq;   // (skin/2)^2 for the displacement check, <= 0 disables
};

// rotation about body axis K by angle phi = h L_K / I_K  (one NO_SQUISH factor)
template <int K, typename R>
__device__ __forceinline__ void free_rotor(R* q, R* L, R h, const R* inv_I) {
  const R phi = h * L[K] * inv_I[K];
  R s, c;
  if constexpr (sizeof(R) == 4) {
    // native v_sin / v_cos: |phi| is a few 1e-2, the precise sincosf (argument reduction, private out-pointers) costs an
    // order of magnitude more instructions for digits fp32 MD cannot use.  (The series used for fp64 below is more
    // accurate than the native pair - 1e-7 relative instead of 1e-7 absolute - but 8 - 10 % slower per STEP, cut at
    // x^7 / x^8 with per-lane loops (67.1 k -> 60.0 k steps/s at 12 kbp) or at x^5 / x^4 behind one uniform branch
    // (67.2 k -> 62.0 k): ten of these are in the tail of every workgroup, and there the transcendental unit's two
    // instructions are cheaper than five multiply-adds.)
    s = __sinf(R(0.5) * phi);
    c = __cosf(R(0.5) * phi);
  } else {
    // fp64: a sub-step turns a nucleotide by ~1e-3 rad, where a short Taylor series is exact to the last bit (to x^7 for
    // the sine, x^6 for the cosine: remainders 2.5e-18 and 2.3e-17 for |x| < 1/32) at a twentieth of the instructions of
    // the library's sincos - ten of these per step sit in the integrating wavefront's chain, behind the last barrier of
    // the kernel, where nothing hides them: 12 kbp 35.7 k -> 39.0 k steps/s, 100 kbp 5.16 k -> 5.71 k with the first
    // version (x^11 / x^12 below 1/8, per-lane loops).  A larger angle (nothing thermal gets there: the margin is a
    // factor of fifteen) is halved until it fits and the result doubled back, behind ONE wave-uniform branch; the
    // library's sin / cos are not called at all (their large-argument reduction keeps a private array: scratch for a
    // path never taken).
    R x = R(0.5) * phi;
    int halvings = 0;
    const bool large = __ballot(fabs(x) >= R(0.03125)) != 0ull;
    if (large)
      while (fabs(x) >= R(0.03125) && halvings < 64) x *= R(0.5), ++halvings;
    const R x2 = x * x;
    s = x * (R(1) + x2 * (R(-1.0 / 6) + x2 * (R(1.0 / 120) + x2 * R(-1.0 / 5040))));
    c = R(1) + x2 * (R(-0.5) + x2 * (R(1.0 / 24) + x2 * R(-1.0 / 720)));
    if (large)
      for (; halvings > 0; --halvings) {
        const R s2 = R(2) * s * c;
        c = c * c - s * s;
        s = s2;
      }
  }
  // q <- q (x) (c, s e_K) = c q + s P_K q
  const R q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  if constexpr (K == 0) {
    q[0] = c * q0 - s * q1;
    q[1] = c * q1 + s * q0;
    q[2] = c * q2 + s * q3;
    q[3] = c * q3 - s * q2;
  } else if constexpr (K == 1) {
    q[0] = c * q0 - s * q2;
    q[1] = c * q1 - s * q3;
    q[2] = c * q2 + s * q0;
    q[3] = c * q3 + s * q1;
  } else {
    q[0] = c * q0 - s * q3;
    q[1] = c * q1 + s * q2;
    q[2] = c * q2 - s * q1;
    q[3] = c * q3 + s * q0;
  }
  // body components of the (lab-fixed) angular momentum rotate by -phi about e_K
  const R cf = c * c - s * s, sf = R(2) * s * c;
  constexpr int A = (K + 1) % 3, B = (K + 2) % 3;
  const R la = L[A], lb = L[B];
  L[A] = cf * la + sf * lb;
  L[B] = -sf * la + cf * lb;
}

template <typename R>
__device__ __forceinline__ void drift(R* x, R* q, const R* p, R* L, R h, const LangevinConst<R>& K) {
  x[0] += h * p[0] * K.inv_mass;
  x[1] += h * p[1] * K.inv_mass;
  x[2] += h * p[2] * K.inv_mass;
  free_rotor<2>(q, L, R(0.5) * h, K.inv_inertia);
  free_rotor<1>(q, L, R(0.5) * h, K.inv_inertia);
  free_rotor<0>(q, L, h, K.inv_inertia);
  free_rotor<1>(q, L, R(0.5) * h, K.inv_inertia);
  free_rotor<2>(q, L, R(0.5) * h, K.inv_inertia);
}

constexpr int kMdBlock = 256;
constexpr int kMdG = 8;                    // lanes per nucleotide
constexpr int kMdPPB = kMdBlock / kMdG;    // nucleotides per workgroup
#ifndef MYTHOS_MD_ITEMS  // (dev A/B: scripts/build_variant.sh)
#define MYTHOS_MD_ITEMS 16
#endif
#ifndef MYTHOS_MD_F64_BLOCKS  // workgroups per CU the register allocator is asked to make room for, by variant
#define MYTHOS_MD_F64_BLOCKS 3
#endif
#ifndef MYTHOS_MD_F64S_BLOCKS
#define MYTHOS_MD_F64S_BLOCKS 2
#endif
#ifndef MYTHOS_MD_F32_BLOCKS
#define MYTHOS_MD_F32_BLOCKS 3
#endif
#ifndef MYTHOS_MD_F32S_BLOCKS
#define MYTHOS_MD_F32S_BLOCKS 2
#endif
constexpr int kMdItems = MYTHOS_MD_ITEMS;  // flagged unbonded neighbours per nucleotide (phase 2) the stepping kernel has room for
// ... and the variant a run falls back to when a nucleotide has more (see md_step_kernel): 32, or what the 160 KB of LDS
// leave for the fp64 energy-trace instantiation, whose result rows carry the 8 term energies as well
template <typename R, bool SAVE>
constexpr int md_items_big() {
  return (sizeof(R) == 8 && SAVE) ? 22 : 32;
}
// Result rows (one per evaluated bonded slot / angular item) come out of ONE pool per workgroup, handed out by a prefix
// sum over the 32 nucleotides' counts: a duplex uses 2 + ~5 rows per nucleotide, a fixed 4 + 16 per nucleotide was two
// thirds empty and its 33 KB (fp32) / 66 KB (fp64) of LDS decided how many workgroups a CU holds.  A workgroup whose
// nucleotides need more rows than the pool has aborts the launch like one whose work lists are too short (ITEMS), and
// the run goes on with the big instantiation, whose pool is the full 32 x (4 + ITEMS).
#ifndef MYTHOS_MD_POOL  // (dev A/B)
#define MYTHOS_MD_POOL 320
#endif
constexpr int kMdPool = MYTHOS_MD_POOL;
constexpr int kTraceWidth = T_COUNT + 2;   // 8 energy terms + KE_trans + KE_rot

// Expanded per-nucleotide state of one time level ("frame"), written by the kernel that
// produced the positions so that neighbour visits never redo the quaternion -> axes algebra:
//   p0 = (centre, meta)   p1 = (a1, 0)   p2 = (a3, 0)   p3 = (backbone offset k1 a1 + k2 a2, 0)
//   pl = (centre_lo, 0)   fp32 only: the centre is the unevaluated sum p0.xyz + pl.xyz (|lo| <= ulp(hi)/2), which
//        keeps ~48 bits of position however large the coordinates are (a 12 kbp duplex is 4 800 length units long,
//        where a bare fp32 coordinate resolves 5e-4).  Differences of nearby centres are then exact to fp32
//        round-off of the DIFFERENCE: (hi_j - hi_i) is exact (Sterbenz), (lo_j - lo_i) is tiny.
//   q  = quaternion
//   mom = (p, 0), ang = (L_body, 0): the momenta of the same time level.  They ping-pong with the positions, so a
//        launch never modifies the state it read: whatever it discovers on the way (a work list that does not fit),
//        the host can discard what it wrote and run that step again from intact inputs.
template <typename R>
struct Frame {
  typename Vec4T<R>::type *p0, *p1, *p2, *p3, *q, *pl, *mom, *ang;
};

template <typename R>
constexpr bool kHiLo = sizeof(R) == 4;

// centre(o) - centre(s) from the hi (and, in fp32, lo) parts
template <typename R>
__device__ __forceinline__ V3<R> centre_diff(const typename Vec4T<R>::type& o_hi, const typename Vec4T<R>::type& o_lo,
                                             const V3<R>& s_hi, const V3<R>& s_lo) {
  V3<R> d{o_hi.x - s_hi.x, o_hi.y - s_hi.y, o_hi.z - s_hi.z};
  if constexpr (kHiLo<R>) {
    d.x += o_lo.x - s_lo.x;
    d.y += o_lo.y - s_lo.y;
    d.z += o_lo.z - s_lo.z;
  }
  return d;
}

// squared cut-offs of the radial pass, derived on the host from the parameter vector
template <typename R>
struct MdCut {
  R rbb2;    // backbone-backbone: max(Debye r_cut, excluded-volume r_c)^2
  R rcom2;   // centre-centre distance below which the base / stack site terms can act
  // squared supports of the angular terms' radial factors (base-base for H-bond and cross-stacking,
  // stack-stack for coaxial stacking): the radial pass flags a neighbour without taking a square root
  R hb_lo2, hb_hi2, cr_lo2, cr_hi2, cx_lo2, cx_hi2;
  // bit (4 * seq_p + seq_q) set where the H-bond weight table is non-zero (only complementary pairs by default):
  // the radial pass tests one bit instead of walking the 16-entry table
  unsigned int hb_mask;
};

template <typename R>
__device__ __forceinline__ V3<R> xyz(const typename Vec4T<R>::type& v) {
  return V3<R>{v.x, v.y, v.z};
}

// radial f3 from r^2: returns the energy and, in coef, tw * V'(r) / r (0 outside the support)
template <typename R>
__device__ __forceinline__ R f3_coef(R eps, R tw, const F3P<R>& fp, R r2, R& coef) {
  coef = R(0);
  if (r2 >= fp.rc * fp.rc) return R(0);
  const R r = m_sqrt(r2);
  const FD<R> v = f3_eval(r, eps, fp);
  coef = tw * v.d / r;
  return v.f;
}

template <typename R>
__device__ __forceinline__ R f3_radial(R eps, R tw, const F3P<R>& fp, V3<R> d, R r2, V3<R>& g) {
  if (r2 >= fp.rc * fp.rc) return R(0);
  const R r = m_sqrt(r2);
  const FD<R> v = f3_eval(r, eps, fp);
  axpy(g, tw * v.d / r, d);
  return v.f;
}

// Wave priority by phase: the further a wavefront is from the end of the kernel, the higher its s_setprio level.
// The SIMD's arbiter serves the older wavefront first, so of the three workgroups that share a CU the first to arrive
// ran ahead (done after 9.2 us) and the last one finished alone, with one wavefront per SIMD and nothing to hide its
// latencies behind (11.7 us; cycle stamps of a diagnostic build, since removed).  With the priority tied to progress the
// workgroup that lags wins the arbitration, the three advance together and the CU is busy to the end: 12 kbp 65.8 k -> 69.3 k steps/s,
// 256 replicas 68.0 k -> 72.1 k, 100 kbp 12.8 k -> 13.0 k.  Five decimal digits = the level of the phases radial-close,
// radial-far, angular, fold, integrate; 33210 against its neighbours on one box: 32210 69.1 k (100 kbp 12.7 k),
// 33200 / 32100 / 33100 / 33211 67.3 - 67.5 k, the reverse order 65.8 k (= none); the wavefront with the short angular
// role (coaxial) one level below the others: 67.1 k.  0 = no s_setprio at all.
// fp64 at 12 kbp gains more (33.3 k -> 36.2 k) but LOSES 3.4 % at 100 kbp, where a CU works through eight rounds of three
// workgroups and finishing the oldest first is what lets the next one in: the host passes prio_on = 0 for fp64 grids that
// are not resident at once (advance_typed).
#ifndef MYTHOS_MD_PRIO_MAP
#define MYTHOS_MD_PRIO_MAP 33210
#endif
#if MYTHOS_MD_PRIO_MAP != 0
constexpr int md_prio_digit(int phase) {
  int v = MYTHOS_MD_PRIO_MAP;
  for (int k = 4; k > phase; --k) v /= 10;
  return v % 10;
}
#define MD_PRIO(phase)                                                     \
  do {                                                                     \
    if (prio_on) __builtin_amdgcn_s_setprio(md_prio_digit(phase));        \
  } while (0)
#else
#define MD_PRIO(phase) do { } while (0)
#endif

// One MD step (see file header).  kick_close: multiple of dt*F that closes the previous step
// (0 for the first kernel of a run, 1/2 otherwise); do_step = 0 for the closing-only kernel.
//
// Work decomposition: 8 lanes per nucleotide, 32 nucleotides per 256-thread workgroup.
//   phase 1 (radial): the lanes stride over the nucleotide's unbonded row - in ONE pipelined sweep over [4, len) whose
//           strides run the close body while any lane of the wavefront has a slot in its close segment and the far body
//           after that; oxNA and the 16-lane instantiations walk the close segment, then the far segment, as two
//           pipelines.  Either way one set of helpers evaluates an entry (close_entry, far_entry, backbone_term) and one
//           fetches the next neighbour's state (NbrState): per neighbour the centre (hi, lo), the backbone offset and -
//           in a close stride - a1; Debye-Hueckel and the excluded-volume site pairs with early-outs on squared
//           distances; the few neighbours whose base-base / stack-stack distance lies in the support of an angular
//           term are flagged (two LDS lists per nucleotide: base-pair terms, coaxial stacking);
//   phase 2 (angular): work items of the whole workgroup, one code path per wavefront: the bonded
//           neighbours (FENE, bonded excluded volume, stacking), the two halves of the base-pair list
//           (H-bond + cross-stacking evaluated together), the coaxial list; results go to LDS rows;
//   fold:   each group sums its rows (DPP reductions over the 8 lanes);
//   integrate: one wavefront advances the 32 nucleotides of the workgroup and writes the next frame.
// workgroups per CU the register allocator is asked to make room for: what the LDS footprint of the
// variant allows (fp32 stepping 43 KB; the trace and fp64 variants carry wider result rows)
// fp64 stepping asks for three: all 750 workgroups of 12 kbp resident at once.  (Until round 3 that bound cost 116 B of
// scratch - 168 VGPRs - and a second instantiation with the looser bound served grids that fit anyway; compiled without
// machine LICM, see the Makefile, the kernel needs 149 VGPRs and no scratch under either bound, so there is one.)
// DENSE (fp32 stepping, oxDNA1 / oxDNA2): a grid of more workgroups than the chip holds at once.  There the step rate
// is what a CU gets through, not one workgroup's chain, and a fifth resident workgroup per CU pays: result rows out of
// the pool as in fp64 (24.6 KB of LDS instead of 37.5) and a register bound of five per CU (96 VGPRs, no scratch) -
// 100 kbp 11.55 k -> 12.65 k steps/s; at 12 kbp, where all 750 workgroups are resident anyway, the same build is 1.7 %
// slower than the fixed rows (the pool's second prefix scan), so it is chosen by grid size (advance_typed).
template <typename R, bool SAVE, int ITEMS, bool DENSE = false, int MODEL = 2, bool PSEQ = false>
constexpr int md_blocks_per_cu() {
  if (DENSE) return 5;
  // (oxNA and oxRNA2-pseq in fp64 spill 52 - 88 B under the three-per-CU bound of 168 VGPRs.  Late in round 4 a change
  // elsewhere in the unit moved the allocation and the 16-lane oxNA instantiation's forces came out wrong by 2.6e-5 from the
  // first step on; two workgroups per CU - no spills - were exact, and so is three per CU once the unit is compiled with
  // -mllvm -amdgpu-remove-redundant-endcf=0: the same compiler fault as in the energy kernel (oxdna_energy_core.inc,
  // MYTHOS_EN_PARK_FROM), in a shape the EXEC = 0 scan does not see.  The flag is on for every unit since - Makefile.)
  if (ITEMS > kMdItems) return sizeof(R) == 4 ? (SAVE ? 1 : 2) : 1;  // a pool of 32 x 36 rows: 64 - 100 KB (fp32), 125 - 150 KB (fp64) of LDS
  return sizeof(R) == 4 ? (SAVE ? MYTHOS_MD_F32S_BLOCKS : MYTHOS_MD_F32_BLOCKS) : (SAVE ? MYTHOS_MD_F64S_BLOCKS : MYTHOS_MD_F64_BLOCKS);
}

// What the radial pass reads of the parameters, gathered so that the oxNA instantiation (MODEL 4) can hold one set per
// kind of pair - DNA-DNA, RNA-RNA, hybrid - and choose per row entry; every other instantiation has ONE set, built from
// the values it always used (scalar registers; the compiler sees the same operands as before).
template <typename R>
struct RadSet {
  F3P<R> f_bb, f_base, f_bkba, f_babk;
  R eps_n, tw_n, tw_dh;
  DebyeP<R> dhp;
  bool half_ends;
  R rbb2, hb_lo2, hb_hi2, cr_lo2, cr_hi2, cx_lo2, cx_hi2;
  unsigned int hb_mask;
};
template <typename R, int MODEL, class PT>
__device__ __forceinline__ RadSet<R> radset_from(const PT& P, const MdCut<R>& cut) {
  RadSet<R> s;
  s.f_bb = f3_params<R>(P, NEXC_BACKBONE_RSTAR), s.f_base = f3_params<R>(P, NEXC_BASE_RSTAR);
  s.f_bkba = f3_params<R>(P, NEXC_BACK_BASE_RSTAR), s.f_babk = f3_params<R>(P, NEXC_BASE_BACK_RSTAR);
  s.eps_n = P[NEXC_EPS];
  s.tw_n = P[TW_NEXC], s.tw_dh = (MODEL >= 2) ? P[TW_DH] : R(0);
  s.half_ends = (MODEL >= 2) && (P[DH_HALF_CHARGED_ENDS] != R(0));
  s.dhp = (MODEL >= 2) ? debye_params<R>(P) : DebyeP<R>{};
  s.rbb2 = cut.rbb2, s.hb_lo2 = cut.hb_lo2, s.hb_hi2 = cut.hb_hi2, s.cr_lo2 = cut.cr_lo2, s.cr_hi2 = cut.cr_hi2;
  s.cx_lo2 = cut.cx_lo2, s.cx_hi2 = cut.cx_hi2, s.hb_mask = cut.hb_mask;
  return s;
}
// oxNA: the supports of one parameter vector, derived on the device (scalar arithmetic, once per workgroup) the way
// make_cut derives them on the host for the single-vector models
template <typename R, class PT>
__device__ __forceinline__ MdCut<R> cut_from(const PT& P, R rcom2) {
  MdCut<R> c;
  const R rbb = fmax(P[NEXC_BACKBONE_RC], P[DH_RCUT]);
  c.rbb2 = rbb * rbb, c.rcom2 = rcom2;
  c.hb_lo2 = P[HYDR_RCLOW] * P[HYDR_RCLOW], c.hb_hi2 = P[HYDR_RCHIGH] * P[HYDR_RCHIGH];
  c.cr_lo2 = P[CRST_RCLOW] * P[CRST_RCLOW], c.cr_hi2 = P[CRST_RCHIGH] * P[CRST_RCHIGH];
  c.cx_lo2 = P[CXST_RCLOW] * P[CXST_RCLOW], c.cx_hi2 = P[CXST_RCHIGH] * P[CXST_RCHIGH];
  c.hb_mask = 0u;
#pragma unroll
  for (int k = 0; k < 16; ++k) c.hb_mask |= (P[HYDR_EPS_00 + k] != R(0)) ? (1u << k) : 0u;
  return c;
}
template <typename R>
__device__ __forceinline__ F3P<R> pick3(const F3P<R>& a, const F3P<R>& b, const F3P<R>& c, int k) {
  return {k == 0 ? a.rstar : (k == 1 ? b.rstar : c.rstar), k == 0 ? a.sigma : (k == 1 ? b.sigma : c.sigma),
          k == 0 ? a.b : (k == 1 ? b.b : c.b), k == 0 ? a.rc : (k == 1 ? b.rc : c.rc), a.base};
}
#define MD_PICK3(f) (k == 0 ? a.f : (k == 1 ? b.f : c.f))
template <typename R>
__device__ __forceinline__ RadSet<R> pick3(const RadSet<R>& a, const RadSet<R>& b, const RadSet<R>& c, int k) {
  RadSet<R> s;
  s.f_bb = pick3(a.f_bb, b.f_bb, c.f_bb, k), s.f_base = pick3(a.f_base, b.f_base, c.f_base, k);
  s.f_bkba = pick3(a.f_bkba, b.f_bkba, c.f_bkba, k), s.f_babk = pick3(a.f_babk, b.f_babk, c.f_babk, k);
  s.eps_n = MD_PICK3(eps_n), s.tw_n = MD_PICK3(tw_n), s.tw_dh = MD_PICK3(tw_dh);
  s.dhp = {MD_PICK3(dhp.rcut), MD_PICK3(dhp.rhigh), MD_PICK3(dhp.kappa), MD_PICK3(dhp.prefactor), MD_PICK3(dhp.bsmooth)};
  s.half_ends = a.half_ends;  // one switch for the whole system (na1/debye.py:25)
  s.rbb2 = MD_PICK3(rbb2), s.hb_lo2 = MD_PICK3(hb_lo2), s.hb_hi2 = MD_PICK3(hb_hi2), s.cr_lo2 = MD_PICK3(cr_lo2);
  s.cr_hi2 = MD_PICK3(cr_hi2), s.cx_lo2 = MD_PICK3(cx_lo2), s.cx_hi2 = MD_PICK3(cx_hi2), s.hb_mask = MD_PICK3(hb_mask);
  return s;
}
#undef MD_PICK3

// the parameter set of the row entry being evaluated: the one set of the model, or (oxNA) the set of the pair's kind -
// 0 DNA-DNA, 1 RNA-RNA, 2 hybrid - from the type bits of the two meta words
#define MD_RADSET_OF_ENTRY                                                                                         \
  const int md_kind = (MODEL == 4) ? na1_kind(self.rna, meta_of(o0.w).rna) : 0;                                    \
  const RadSet<R> rs_picked = (MODEL == 4) ? pick3(rs0, rs1, rs2, md_kind) : rs0;                                  \
  const RadSet<R>& rs = (MODEL == 4) ? rs_picked : rs0;
__device__ __forceinline__ int na1_kind(int self_rna, int other_rna) { return (self_rna && other_rna) ? 1 : ((self_rna || other_rna) ? 2 : 0); }

// The meta word of a nucleotide as a frame carries it (p0.w): bits 0 - 1 the base, bit 2 strand end, bit 3 RNA (oxNA)
struct Meta {
  int seq, is_end, rna;
};
template <typename R>
__device__ __forceinline__ Meta meta_of(R w) {
  const int m = (int)w;
  return Meta{m & 3, (m >> 2) & 1, (m >> 3) & 1};
}
template <typename R>
__device__ __forceinline__ void set_meta(Nuc<R>& nuc, R w) {
  const Meta m = meta_of(w);
  nuc.seq = m.seq, nuc.is_end = m.is_end, nuc.rna = m.rna;
}
// centre and axes of a workgroup's own nucleotide from its self_lds row (words 0 - 8).  The meta word (9) and the low
// part of the centre (10 - 12) stay with the caller: read here, the meta word was kept in a register from the head of the
// integrator to the frame store at its end, which reads it again.  (seq, is_end, rna and idx are the caller's to set.)
template <typename R>
__device__ __forceinline__ Nuc<R> nuc_from_lds(const R* ms) {
  Nuc<R> nuc;
  nuc.c = V3<R>{ms[0], ms[1], ms[2]};
  nuc.a1 = V3<R>{ms[3], ms[4], ms[5]};
  nuc.a3 = V3<R>{ms[6], ms[7], ms[8]};
  nuc.a2 = cross(nuc.a3, nuc.a1);
  return nuc;
}

// Neighbour state in flight for the radial pass: centre and meta word, backbone offset, a1 (close strides only) and, in
// fp32, the low part of the centre.  with_a1 is a constant or wave-uniform.
template <typename R>
struct NbrState {
  typename Vec4T<R>::type n0{}, n3{}, n1{}, nl{};
  __device__ __forceinline__ void fetch(const Frame<R>& in, int j, bool with_a1) {
    n0 = in.p0[j];
    n3 = in.p3[j];
    if (with_a1) n1 = in.p1[j];
    if constexpr (kHiLo<R>) nl = in.pl[j];
  }
};

// ITEMS: result rows per nucleotide for the angular work lists.  16 is enough for any duplex, junction or origami
// at physical density (a base has 3 - 5 partners inside the range of an angular term); a nucleotide with more makes
// the launch ABORT: it raises flags[3], the host discards what that launch wrote (its inputs are intact: frames and
// momenta ping-pong) and runs the step again with the ITEMS = 32 instantiation, which stays in use for the rest of
// the run.  More than 32 is reported as an error (sterically that takes overlapping bases).
// PSEQ: the system carries a probabilistic sequence (mythos_oxdna_set_pseq): the two sequence-weight look-ups of the
// angular pass are expectations (ConstParams<R, true>, as in the energy kernel) and the radial pass flags every pair
// inside the hydrogen-bonding range, whatever the discrete sequence says.  Its own instantiations (both list widths since
// round 4): the plain ones keep their registers and instruction counts.
// GL: lanes per nucleotide.  8 (32 nucleotides per workgroup) for grids that fill the chip; 16 (16 per workgroup, twice
// the workgroups) for small systems - 1 kbp, the DiffTRe replicas - where a launch lasts as long as one workgroup's
// chain and occupancy is not the constraint: a nucleotide's ~12 close and ~13 far row entries are then ONE iteration of
// each radial loop instead of two, and round 4 measured the second iterations at 30 % of the kernel.
// At 12 kbp the doubled grid (1 500 workgroups of 116 VGPRs) would not be resident at once; the host chooses (advance_typed).
template <typename R, int MODEL, bool SAVE, int ITEMS, bool PSEQ = false, bool DENSE = false, int GL = kMdG>
__global__ __launch_bounds__(kMdBlock, (md_blocks_per_cu<R, SAVE, ITEMS, DENSE, MODEL, PSEQ>())) void md_step_kernel(
    const R* __restrict__ Pg, const BoxT<R> box, const LangevinConst<R> K, const MdCut<R> cut, int n, const Frame<R> in,
    const Frame<R> out,
    const int* __restrict__ rows, const int* __restrict__ row_len, const int* __restrict__ row_close, int row_stride,
    int extra_bonds, R kick_close, int do_step, uint64_t seed, uint64_t step, const typename Vec4T<R>::type* __restrict__ ref_pos,
    const typename Vec4T<R>::type* __restrict__ ref_off, const typename Vec4T<R>::type* __restrict__ ref_a1,
    int* __restrict__ flags,
    R* __restrict__ traj_c, R* __restrict__ traj_q, double* __restrict__ e_part, const int* __restrict__ chunk_order,
    const int* __restrict__ list_overflow, int k_index, int /* unused */, int prio_on, const PseqView<R> pseq) {
  // (the unused word keeps the kernel-argument layout the register allocation of these kernels was measured with:
  // without it prio_on and pseq move up and the fp32 12 kbp kernel spills its scalars differently, 1 % slower)
  using V4 = typename Vec4T<R>::type;
  constexpr int G = GL, PPB = kMdBlock / GL;
  static_assert(GL == 8 || GL == 16, "lanes per nucleotide");
  static_assert(!DENSE || GL == kMdG, "DENSE serves large grids");
  constexpr int RW = (SAVE ? 12 + T_COUNT : 12) + 1;  // result row: dc, g1, g2, g3 (+ energies), padded to odd
  // rows of one nucleotide: its two bonded slots + ITEMS flagged neighbours (in a system with circular strands the two
  // second-bond slots come out of the ITEMS).  Two rows fewer per nucleotide than four bonded slots + ITEMS: 3.3 KB of
  // LDS under the fp32 stepping instantiation (37.5 KB now).  LDS decides the residency earlier than 160 KB / size
  // suggests: at 44 KB per workgroup a CU held 2.2 workgroups on average where it holds 2.7 at 41 KB (100 kbp: 11.2 k
  // -> 9.3 k steps/s; found in round 3 through two experiments that each grew the footprint by a few KB).
  constexpr int kSlots = 2 + ITEMS;
  // two work lists per nucleotide: 0 = base-pair terms (H-bond and / or cross-stacking: they share the base-base
  // vector and all six angles, so one evaluation serves both), 1 = coaxial stacking
  // Wave-dense lists (the fixed-row instantiations of the single sweep, ITEMS = 16: the 12 kbp kernel): every wavefront
  // appends what its groups flag to ONE list per kind while the radial pass runs - position = the wavefront's running
  // count + the flagged lanes below, both out of the ballot the per-nucleotide slot needs anyway - so the angular pass
  // finds its items with two LDS round trips (the four counts, the item) where the per-nucleotide lists take a prefix
  // scan over the 32 counts and a binary search: fourteen dependent round trips in front of the first neighbour load of
  // the base-pair wavefronts, the longest chain of the kernel.  An item is 8 bytes: the row entry, and p | k << 8 - the
  // owner and the slot within the owner's list, which fix the result row exactly as the per-nucleotide lists do.
  // kWaveCap per wavefront and kind (a duplex has 25 - 35 base-pair items per wavefront); a fuller wavefront aborts the
  // launch like an over-full nucleotide, and the ITEMS = 32 instantiation (per-nucleotide lists: 8 x ITEMS items per
  // wavefront would take 16 KB) repeats the step.  2 x 4 x 64 x 8 B = 4 KB in place of items (4 KB) + item_pre (0.5 KB).
  // (oxRNA2, MODEL 3, keeps the per-nucleotide lists: with the dense ones md_step_kernel<float, 3, false, 16> took 52 B of
  // scratch where it had none; oxNA, MODEL 4, and the 16-lane instantiations walk their rows in two pipelines whose trip
  // counts differ between the groups of a wavefront, so a wavefront-wide running count has no place there)
  constexpr bool kWaveLists = sizeof(R) == 4 && !DENSE && ITEMS == kMdItems && MODEL <= 2 && GL == kMdG;
  constexpr int kWaveCap = 64;
  __shared__ int items[kWaveLists ? 1 : 2][kWaveLists ? 1 : PPB][kWaveLists ? 1 : ITEMS];  // the flagged row ENTRIES (index | role bit), not their slots
  __shared__ int item_cnt[2][PPB];
  __shared__ int item_pre[kWaveLists ? 1 : 4][kWaveLists ? 1 : PPB + 1];  // per WAVEFRONT: the prefix of the list that wavefront will walk
  __shared__ int2 wave_items[kWaveLists ? 2 : 1][kWaveLists ? 4 : 1][kWaveLists ? kWaveCap : 1];
  __shared__ __attribute__((aligned(16))) int wave_cnt[2][4];  // items of every wavefront's list, final at the barrier
  __shared__ R self_lds[PPB][13];
  __shared__ R rad_lds[PPB][7];  // radial-pass site gradients (backbone, base) of each nucleotide
  // result rows, [nucleotide][slot][RW] with the nucleotide stride padded to an odd word count: the 32
  // nucleotides' rows then start in 32 different banks (20 x 13 = 260 words would alias p and p + 8)
  // fp64: rows out of the workgroup's pool (see kMdPool).  fp32 keeps a fixed block of kSlots rows per nucleotide: its
  // LDS never decided the residency (2.9 workgroups per CU at 12 kbp), and the pool's second prefix scan and base-row
  // look-ups cost it 1.2 % (61.3 k against 62.1 k steps/s, A/B on one box).
  static_assert(!DENSE || (sizeof(R) == 4 && !SAVE && !PSEQ && ITEMS == kMdItems && MODEL <= 2), "DENSE: see md_blocks_per_cu");
  constexpr bool kPooled = sizeof(R) == 8 || DENSE;
  constexpr int kPool = (ITEMS > kMdItems || !kPooled) ? PPB * kSlots : kMdPool * PPB / kMdPPB;  // (320 rows per 32 nucleotides)
  static_assert(kPool >= PPB * ROW_BONDED_SLOTS, "the pool holds at least the bonded rows");
  static_assert(ITEMS > ROW_BONDED_SLOTS, "room for the second-bond slots of circular strands");
  __shared__ R res_flat[kPool * RW + (kPooled ? 0 : PPB)];
  __shared__ int row_base[kPooled ? 4 : 1][PPB + 1];  // per WAVEFRONT (like item_pre): first pool row of every nucleotide
  // fixed layout: the nucleotide stride padded to an odd word count, so the 32 nucleotides' blocks start in 32 banks
  constexpr int kFixedStride = (kSlots * RW) | 1;
  auto pool_row = [&](int row) -> R* { return res_flat + row * RW; };
  auto fixed_row = [&](int pp, int slot) -> R* { return res_flat + pp * kFixedStride + slot * RW; };
  __shared__ double e_lds[SAVE ? PPB : 1][kTraceWidth];
  using CP = ConstParams<R, PSEQ>;
  const auto make_cp = [&](const R* g) {
    if constexpr (PSEQ) return CP(g, pseq); else return CP(g);
  };
  const CP P = make_cp(Pg);  // scalar loads at the point of use; an LDS copy was measured 2.4x slower
  const int grp = threadIdx.x / G;
  const int lane = threadIdx.x % G;
  // XCD-aware order: the hardware deals consecutive workgroups round-robin to the 8 XCDs, so workgroup b
  // takes chunk (b % 8) * ceil(n_blocks / 8) + b / 8 - every XCD then owns one contiguous eighth of the
  // nucleotide index range and neighbouring chunks (same strand, adjacent cells) share its L2.
  const int n_blocks = (n + PPB - 1) / PPB;
  const int vb = (int)(blockIdx.x & 7) * ((n_blocks + 7) >> 3) + (int)(blockIdx.x >> 3);
  if (vb >= n_blocks) return;  // grid is padded to a multiple of 8; whole workgroup leaves together
  // Halted (flags[1], set by the previous step when a site left its skin; or a rebuild overflowed its rows or spill
  // list): this and every later launch of the segment do nothing, the state stays at the last valid step, and the
  // host rebuilds and resumes from flags[2] (kernel index after the last one that ran).
  // One lane requests the words here; everybody looks at them behind the first barrier (LDS), before which the
  // kernel writes nothing to global memory.  (Every thread loading and testing them up front cost 1.7 % of the step.)
  __shared__ int s_halt;
  int halt_word = 0;  // requested now, parked in LDS just before the barrier: nobody waits for it on the way
  // The halt word carries the index of the first launch that must not run (set by launch k: k + 1): a workgroup of
  // the SAME launch that starts after the word was set keeps going - on a grid larger than what is resident at once
  // the late workgroups of launch k would otherwise skip a step the early ones took.
  if (threadIdx.x == 0) {
    const int hw = flags[1], aw = flags[3];  // aw: an earlier launch aborted (work lists too short, see ITEMS)
    halt_word = ((hw != 0 && hw <= k_index) ? 1 : 0) | ((aw != 0 && aw <= k_index) ? 1 : 0) |
                (list_overflow ? (list_overflow[0] | list_overflow[1]) : 0);
  }
  // chunk_order (host, from the positions at the start of a run): the chunks of 32 nucleotides in spatial order, so
  // the contiguous eighth an XCD works on is also contiguous in space - in a duplex the two complementary
  // stretches of the strands, which are far apart in index, land on the same XCD and share its L2
  const int bid = chunk_order ? chunk_order[vb] : vb;
  const int i = bid * PPB + grp;
  const bool valid = i < n;
  const int ii = valid ? i : n - 1;  // out-of-range groups shadow the last nucleotide and discard

  const R g_ba = P[GEO_BASE], g_st = P[GEO_STACK];
  // oxNA: the oxRNA2 vector (sites of an RNA nucleotide) and the hybrid one; P itself is the oxDNA2 vector there
  const CP Prna = make_cp(Pg + ((MODEL == 4) ? OXP_COUNT : 0)), Pdrh = make_cp(Pg + ((MODEL == 4) ? 2 * OXP_COUNT : 0));
  const Na1Params<CP> P4{P, Prna, Pdrh};

  // ---- owner state (also parked in LDS for the block-wide angular pass)
  Nuc<R> self;
  V3<R> offb_s, self_lo{R(0), R(0), R(0)};
  {
    const V4 s0 = in.p0[ii], s1 = in.p1[ii], s2 = in.p2[ii], s3 = in.p3[ii];
    if constexpr (kHiLo<R>) self_lo = xyz<R>(in.pl[ii]);
    self.c = xyz<R>(s0);
    self.a1 = xyz<R>(s1);
    self.a3 = xyz<R>(s2);
    self.a2 = cross(self.a3, self.a1);
    offb_s = xyz<R>(s3);
    set_meta(self, s0.w);
    if (lane == 0) {
      R* sl = self_lds[grp];
      sl[0] = s0.x, sl[1] = s0.y, sl[2] = s0.z, sl[3] = s1.x, sl[4] = s1.y, sl[5] = s1.z;
      sl[6] = s2.x, sl[7] = s2.y, sl[8] = s2.z, sl[9] = s0.w;
      sl[10] = self_lo.x, sl[11] = self_lo.y, sl[12] = self_lo.z;
    }
  }
  const int* __restrict__ row = rows + (size_t)ii * row_stride;
  const int len = valid ? row_len[ii] : 0;
  const int close_end = min(len, row_close[ii]);  // [2, close_end): any term may act; [close_end, len): backbone only

  R e[T_COUNT];
#pragma unroll
  for (int k = 0; k < T_COUNT; ++k) e[k] = R(0);
  V3<R> gbk{R(0), R(0), R(0)}, gba{R(0), R(0), R(0)};  // sum of dV/dd acting on self's backbone / base site

  MD_PRIO(0);
  // ---- phase 1: radial pass over the unbonded slots
  const RadSet<R> rs0 = (MODEL == 4) ? radset_from<R, 2>(P, cut_from<R>(P, cut.rcom2)) : radset_from<R, MODEL>(P, cut);
  // (oxNA: the oxRNA2 and the hybrid vector follow the oxDNA2 one; the other models never read rs1 / rs2)
  const RadSet<R> rs1 = (MODEL == 4) ? radset_from<R, 2>(Prna, cut_from<R>(Prna, cut.rcom2)) : rs0;
  const RadSet<R> rs2 = (MODEL == 4) ? radset_from<R, 2>(Pdrh, cut_from<R>(Pdrh, cut.rcom2)) : rs0;
  int n_items[2] = {0, 0};
  const int wave_s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int wave_n[2] = {0, 0};  // (wave-dense lists) items of this wavefront's two lists so far: wave-uniform
  const int row_room = ITEMS - (extra_bonds ? ROW_BONDED_SLOTS - 2 : 0);  // result rows left for flagged neighbours
  const int lane64 = threadIdx.x & 63;
  const int gshift = lane64 & ~(G - 1);
  // Software pipeline: ONE sweep over the unbonded slots [ROW_BONDED_SLOTS, len) in strides of G - lane l of a group takes
  // slots ROW_BONDED_SLOTS + l + G t, so the close entries sit on the lanes and in the iterations of their own (the flagged
  // lists keep their order) and the far segment follows on without a second prologue: its first entries and their state
  // are in flight while the last close stride is evaluated.  Row entries are fetched two strides ahead, and the neighbour
  // state (centre, backbone offset, a1) of stride t + 1 is requested before stride t is evaluated, so the
  // L2 / Infinity-Cache round trips overlap the arithmetic instead of serialising with it.
  // (rolled: keeping the body once in the instruction stream matters more than unrolling - the whole
  // kernel has to stay inside the instruction cache that two CUs share)
  // (within a stride the prefetches are unconditional per lane: an entry past the end of the row is read from the row's
  // last slot and replaced by -1, a missing neighbour's state is read from the lane's OWN nucleotide and never used -
  // lines that are in the cache anyway; a load behind a lane-dependent branch made the compiler wait for ALL outstanding
  // loads at the join, the one just issued included.  WHETHER a stride is fetched at all is a question to the whole
  // wavefront - a scalar compare, a scalar branch: no load is issued for a stride in which no lane has an entry, and a1
  // only if one of those entries is in a close segment, so the last iteration of the sweep issues no load.  Until the two
  // segments were one sweep each of them ended on a full set of prefetches nobody read: 7 of a wavefront's 54.5 read
  // instructions per launch at 12 kbp, on the L1 port the three workgroups of a CU contend for in this pass.)
  // The body of an iteration is chosen per wavefront as well: the close body while any lane has a slot below its
  // close_end - a far entry that shares such a stride goes through it with `close` forced false and gets exactly the
  // backbone terms of the far body - and the far body (backbone - backbone only) from the first all-far stride on.
  auto row_at = [&](int s, int end) -> int {
    const int v = row[max(min(s, end - 1), 0)];
    return s < end ? v : -1;
  };
  auto row_word = [&](int s) -> int { return row[max(min(s, len - 1), 0)]; };
  auto slot_of_entry = [&](int e) -> int { return e >= 0 ? (e & ROW_INDEX_MASK) : ii; };
  // The radial terms of ONE row entry, written once for the two loop structures below.  o: the neighbour's state as the
  // pipeline delivered it - the loops take the four vectors out of the prefetch struct first and hand the helpers a
  // temporary built from them: with `const NbrState<R> o = nb;` as the loop's copy md_step_kernel<double, 2, false, 16,
  // false, false, 16> took 36 B of scratch where it had none (profiles/r06_radial_entry.md has the shapes that were tried:
  // the compiler inlines these helpers only after its first scalar-replacement pass, so what crosses a helper's boundary
  // is allocated differently, and no shape reproduces the hand-written copies' code instruction for instruction).
  // backbone - backbone: excluded volume + Debye-Hueckel
  auto backbone_term = [&](const RadSet<R>& rs, const V3<R>& dco, const V3<R>& offb_o, const V4& o0) __attribute__((always_inline)) {
    const V3<R> d = dco + offb_o - offb_s;
    const R r2 = dot(d, d);
    if (r2 < rs.rbb2) {
      const R r = m_sqrt(r2);
      const FD<R> v = f3_eval(r, rs.eps_n, rs.f_bb);
      R dVdr = rs.tw_n * v.d;
      R en = v.f;
      if constexpr (MODEL >= 2) {
        const FD<R> dh = debye_eval(r, rs.dhp);
        R mult = R(1);
        if (rs.half_ends) mult = (self.is_end ? R(0.5) : R(1)) * (meta_of(o0.w).is_end ? R(0.5) : R(1));
        dVdr += rs.tw_dh * mult * dh.d;
        if constexpr (SAVE) e[T_DH] += R(0.5) * mult * dh.f;
      }
      if constexpr (SAVE) e[T_NEXC] += R(0.5) * en;
      axpy(gbk, dVdr / r, d);
    }
  };
  // an entry of the far segment: only the backbone - backbone terms can act
  auto far_entry = [&](const NbrState<R>& o) __attribute__((always_inline)) {
    const V4& o0 = o.n0;
    MD_RADSET_OF_ENTRY
    const V3<R> dco = min_image(centre_diff<R>(o0, o.nl, self.c, self_lo), box);
    backbone_term(rs, dco, xyz<R>(o.n3), o0);
  };
  // an entry of a stride that holds close entries.  in_close: the slot lies in the close segment, so any term may act and
  // the entry may be flagged for the angular lists (flag[0] base-pair terms, flag[1] coaxial stacking); an entry of the
  // far segment that shares the stride gets exactly the backbone terms of far_entry
  auto close_entry = [&](int entry, const NbrState<R>& o, bool in_close, bool (&flag)[2]) __attribute__((always_inline)) {
    const V4 &o0 = o.n0, &o1 = o.n1;
    const bool role_p = (entry & ROW_ROLE_Q) == 0;
    MD_RADSET_OF_ENTRY
    const bool o_rna = (MODEL == 4) && meta_of(o0.w).rna;
    const R gba_s = (MODEL == 4 && self.rna) ? Prna[GEO_BASE] : g_ba, gba_o = o_rna ? Prna[GEO_BASE] : g_ba;
    const R gst_s = (MODEL == 4 && self.rna) ? Prna[GEO_STACK] : g_st, gst_o = o_rna ? Prna[GEO_STACK] : g_st;
    (void)gst_s, (void)gst_o;
    const V3<R> dco = min_image(centre_diff<R>(o0, o.nl, self.c, self_lo), box);
    const V3<R> offb_o = xyz<R>(o.n3);
    const bool close = in_close && dot(dco, dco) < cut.rcom2;
    backbone_term(rs, dco, offb_o, o0);
    if (close) {
      const V3<R> a1o = xyz<R>(o1);
      R en = R(0);
      // self backbone - other base and self base - other backbone: which of the two is the reference's
      // "back_p - base_q" / "base_p - back_q" depends on the role; the squared distances are routed by
      // role so both parameter blocks stay scalar operands
      {
        V3<R> dA = dco - offb_s;
        axpy(dA, gba_o, a1o);
        V3<R> dB = dco + offb_o;
        axpy(dB, -gba_s, self.a1);
        const R ra2 = dot(dA, dA), rb2 = dot(dB, dB);
        R c1, c2;
        en += f3_coef(rs.eps_n, rs.tw_n, rs.f_bkba, role_p ? ra2 : rb2, c1);
        en += f3_coef(rs.eps_n, rs.tw_n, rs.f_babk, role_p ? rb2 : ra2, c2);
        axpy(gbk, role_p ? c1 : c2, dA);
        axpy(gba, role_p ? c2 : c1, dB);
      }
      const V3<R> da = a1o - self.a1;
      {
        V3<R> d = dco;
        if constexpr (MODEL == 4) {  // each nucleotide's base site at the offset of its own type
          axpy(d, gba_o, a1o);
          axpy(d, -gba_s, self.a1);
        } else {
          axpy(d, g_ba, da);
        }
        const R r2 = dot(d, d);
        en += f3_radial(rs.eps_n, rs.tw_n, rs.f_base, d, r2, gba);
        // (& and not &&, here and for flag[1]: written to a flag the caller owns, the short-circuit forms stayed branches -
        // twelve instructions and a saved EXEC per entry in place of the parent's five; 12 kbp fp32 0.2 - 0.4 % slower)
        flag[0] = (rs.cr_lo2 < r2) & (r2 < rs.cr_hi2);
        if (!flag[0] & (rs.hb_lo2 < r2) & (r2 < rs.hb_hi2)) {  // H-bond only for pairs with a non-zero weight
          const int so = meta_of(o0.w).seq;
          if (PSEQ && (pseq.terms & 2) != 0)
            flag[0] = rs.hb_mask != 0u;  // the weight is an expectation over both bases: any non-zero table entry may count
          else
            flag[0] = (rs.hb_mask >> (role_p ? (self.seq * 4 + so) : (so * 4 + self.seq))) & 1u;
        }
      }
      {
        V3<R> d = dco;
        if constexpr (MODEL == 4) {
          axpy(d, gst_o, a1o);
          axpy(d, -gst_s, self.a1);
        } else {
          axpy(d, g_st, da);
        }
        const R r2 = dot(d, d);
        flag[1] = (rs.cx_lo2 < r2) & (r2 < rs.cx_hi2);
      }
      if constexpr (SAVE) e[T_NEXC] += R(0.5) * en;
    }
  };
  // append the flagged slots of this group to its two LDS lists, in slot order
  auto append_flagged = [&](const bool (&flag)[2], int entry) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const unsigned long long bal = __ballot(flag[t]);
      const unsigned int gm = (unsigned int)(bal >> gshift) & ((1u << G) - 1u);
      if (flag[t]) {
        const int pos = n_items[t] + __popc(gm & ((1u << lane) - 1u));
        if constexpr (kWaveLists) {
          const int wpos = wave_n[t] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          if (wpos < kWaveCap) wave_items[t][wave_s][wpos] = make_int2(entry, grp | (pos << 8));  // (a fuller list aborts the launch below)
        } else {
          if (pos < ITEMS) items[t][grp][pos] = entry;  // (row_room <= ITEMS; an over-full nucleotide aborts the launch below)
        }
      }
      n_items[t] += __popc(gm);
      if constexpr (kWaveLists) wave_n[t] = __builtin_amdgcn_readfirstlane(wave_n[t] + __popcll(bal));  // (a scalar register, not one per lane)
    }
  };
  // oxNA (MODEL 4) keeps the two separate pipelines - close segment, then far segment - it had before the single sweep:
  // with the sweep, hipcc's register allocation of md_step_kernel<double, 4, true, *, false, false, 8> parks the
  // kernel-argument tuple {flags, traj_c, traj_q, e_part} in spill lanes AFTER two later scalar loads have overwritten
  // three quarters of it, and the launch writes its trajectory rows through the wrong pointers (seen on the GPU: dynamics
  // exact, saved rows never written; read in the -S output: s_load_dwordx8 s[12:19] at 0x1d0, s_load s[14:15] / s[16:23],
  // then v_writelane of s12 .. s19).  Its instantiations compile to what they were; DESIGN section 8.
  // So do the 16-lane instantiations (GL == 16, small systems): a row of ~25 entries is two strides either way, and the
  // 1 kbp run measured the sweep 1.4 % SLOWER there (86.2 k against 87.5 k steps/s, three alternations).
  if constexpr (MODEL == 4 || GL != kMdG) {
    {
      int e_cur = -1, e_nxt = -1;
      NbrState<R> nb;
      {
        const int s = ROW_BONDED_SLOTS + lane;
        e_cur = row_at(s, close_end);
        e_nxt = row_at(s + G, close_end);
        nb.fetch(in, slot_of_entry(e_cur), true);
      }
#pragma unroll 1
      for (int s0 = ROW_BONDED_SLOTS; s0 < close_end; s0 += G) {
        const int s = s0 + lane;
        const int entry = e_cur;
        const V4 o0 = nb.n0, o3 = nb.n3, o1 = nb.n1, ol = nb.nl;
        e_cur = e_nxt;
        e_nxt = row_at(s + 2 * G, close_end);
        nb.fetch(in, slot_of_entry(e_cur), true);  // the close segment reads a1 as well: nearly all of its entries need it
        bool flag[2] = {false, false};
        if (entry >= 0) close_entry(entry, NbrState<R>{o0, o3, o1, ol}, true, flag);
        append_flagged(flag, entry);
      }
    }
    // far segment: only the backbone-backbone terms (excluded volume + Debye-Hueckel) can act
    MD_PRIO(1);
    {
      int e_cur = -1, e_nxt = -1;
      NbrState<R> nb;
      {
        const int s = close_end + lane;
        e_cur = row_at(s, len);
        e_nxt = row_at(s + G, len);
        nb.fetch(in, slot_of_entry(e_cur), false);
      }
#pragma unroll 1
      for (int s0 = close_end; s0 < len; s0 += G) {
        const int s = s0 + lane;
        const int entry = e_cur;
        const V4 o0 = nb.n0, o3 = nb.n3, o1 = nb.n1, ol = nb.nl;
        e_cur = e_nxt;
        e_nxt = row_at(s + 2 * G, len);
        nb.fetch(in, slot_of_entry(e_cur), false);
        if (entry >= 0) far_entry(NbrState<R>{o0, o3, o1, ol});
      }
    }
  } else {
    {
      // (e_nxt is the word as it was read: whether the lane has an entry there is decided from the slot when the word moves
      // up to e_cur, an iteration later - a select right behind the conditional load would wait for it on the spot)
      int e_cur = -1, e_nxt = -1;
      NbrState<R> nb;
      // the longest row and the longest close segment of the wavefront, as scalars: the lanes of a group hold the same two
      // numbers, so one lane per group is read.  "Some lane has an entry in the stride at s0" is then s0 < wlen and "some
      // lane's slot there is in its close segment" s0 < wclose - scalar loop control and no mask to carry.  (The same
      // questions as ballots over s < len, carried from iteration to iteration or asked again at each use, cost scratch:
      // 36 B in md_step_kernel<double, 2> under a probabilistic sequence, 20 - 36 B in the DENSE instantiation.)
      int wlen = 0, wclose = 0;
#pragma unroll
      for (int k = 0; k < 64 / G; ++k) {
        wlen = max(wlen, __builtin_amdgcn_readlane(len, k * G));
        wclose = max(wclose, __builtin_amdgcn_readlane(close_end, k * G));
      }
      int s0 = ROW_BONDED_SLOTS;
      if (s0 < wlen) {
        const int s = s0 + lane;
        e_cur = row_at(s, len);
        if (s0 + G < wlen) e_nxt = row_word(s + G);
        nb.fetch(in, slot_of_entry(e_cur), s0 < wclose);
      }
#pragma unroll 1
      for (; s0 < wlen; s0 += G) {
        const int s = s0 + lane;
        const int entry = e_cur;
        const V4 o0 = nb.n0, o3 = nb.n3, o1 = nb.n1, ol = nb.nl;
        e_cur = s + G < len ? e_nxt : -1;
        if (s0 + G < wlen) {
          if (s0 + 2 * G < wlen) e_nxt = row_word(s + 2 * G);
          nb.fetch(in, slot_of_entry(e_cur), s0 + G < wclose);  // the close segment reads a1 as well: nearly all of its entries need it
        }
        if (s0 < wclose) {
          bool flag[2] = {false, false};
          if (entry >= 0) close_entry(entry, NbrState<R>{o0, o3, o1, ol}, s < close_end, flag);  // (a far entry in a mixed stride: backbone terms only)
          append_flagged(flag, entry);
        } else {
          // all-far stride: only the backbone-backbone terms (excluded volume + Debye-Hueckel) can act
          MD_PRIO(1);
          if (entry >= 0) far_entry(NbrState<R>{o0, o3, o1, ol});
        }
      }
    }
  }
  bool lists_over = n_items[0] + n_items[1] > row_room;  // result rows of one nucleotide exhausted: this launch does not count
  // (wave-dense lists: ... or a wavefront's list is full.  Either way the WHOLE wavefront hands in nothing: its items
  // cannot be told apart by owner any more, and an item of an over-full nucleotide would point past its result rows)
  if constexpr (kWaveLists) lists_over = __any(lists_over) || wave_n[0] > kWaveCap || wave_n[1] > kWaveCap;
  if (lists_over) {
    if (lane == 0) atomicMax(flags + 3, k_index + 1);
    n_items[0] = n_items[1] = 0;
    wave_n[0] = wave_n[1] = 0;
  }
  // The radial sums are folded over the group now and parked in LDS: nothing computed so far stays in
  // registers across the angular pass (whose pair functions need the whole register budget).
  group_reduce_v3<G>(gbk);
  group_reduce_v3<G>(gba);
  if (lane == 0) {
    R* rl = rad_lds[grp];
    rl[0] = gbk.x, rl[1] = gbk.y, rl[2] = gbk.z, rl[3] = gba.x, rl[4] = gba.y, rl[5] = gba.z;
#pragma unroll
    for (int t = 0; t < 2; ++t) item_cnt[t][grp] = valid ? n_items[t] : 0;
  }
  if constexpr (kWaveLists) {
    if (lane64 == 0) wave_cnt[0][wave_s] = wave_n[0], wave_cnt[1][wave_s] = wave_n[1];
  }
  if (threadIdx.x == 0) s_halt = halt_word;
  __syncthreads();  // self_lds, rad_lds and item_cnt are visible
  MD_PRIO(2);
  if (s_halt != 0) return;  // halted: nothing has been written to global memory yet
  if (vb == 0 && threadIdx.x == 0) flags[2] = k_index + 1;

  // ---- phase 2: angular pass, work items spread over the whole workgroup so that every wavefront
  //      runs ONE code path (roles below).  Results go to the owner's result rows in LDS.
  {
    NoPG pg;
    // role of this wavefront: 0 bonded, 1 and 2 the two halves of the base-pair list (~100 items per workgroup
    // in a duplex: one sweep of 64 each instead of two sweeps on one wavefront), 3 coaxial list; rotated with the
    // workgroup index so the heavy and the light roles spread over the four SIMDs of a CU
    const int wave = ((threadIdx.x >> 6) + bid) & 3;
    const bool bonded_wave = wave == 0;
    const int lst = wave == 3 ? 1 : 0;
    // exclusive prefix of the 32 per-nucleotide counts of this wavefront's list, so the list is dense over the
    // workgroup; every wavefront scans for itself (5 DPP-free shuffle steps) instead of meeting at a second barrier
    const int pw = threadIdx.x >> 6;
    // rows 2, 3 (second-bond slots) exist only in systems with circular strands
    const int n_bonded_rows = extra_bonds ? ROW_BONDED_SLOTS : 2;
    // wave-dense lists: the list of this wavefront's role is the four wavefronts' lists one after the other - item q is
    // found from the four counts (one 16-byte read) with three compares; no scan, no search, no second barrier
    int wl_b1 = 0, wl_b2 = 0, wl_b3 = 0, wl_n = 0;
    if constexpr (kWaveLists) {
      const int4 wc = *reinterpret_cast<const int4*>(wave_cnt[lst]);
      const int c0 = __builtin_amdgcn_readfirstlane(wc.x), c1 = __builtin_amdgcn_readfirstlane(wc.y);
      const int c2 = __builtin_amdgcn_readfirstlane(wc.z), c3 = __builtin_amdgcn_readfirstlane(wc.w);
      wl_b1 = c0, wl_b2 = wl_b1 + c1, wl_b3 = wl_b2 + c2, wl_n = wl_b3 + c3;  // (scalars: the pair functions need every vector register)
    } else {
      const int l = threadIdx.x & 63;
      int inc = (l < PPB) ? item_cnt[lst][l] : 0;
      // ... and (pooled rows) of the rows every nucleotide takes from the result pool: its bonded slots, then its two lists
      int rows_inc = (kPooled && l < PPB) ? n_bonded_rows + item_cnt[0][l] + item_cnt[1][l] : 0;
#pragma unroll
      for (int o = 1; o < PPB; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (l >= o) inc += u;
        if constexpr (kPooled) {
          const int v = __shfl_up(rows_inc, o, 64);
          if (l >= o) rows_inc += v;
        }
      }
      if (l < PPB) item_pre[pw][l + 1] = inc;
      if (l == 0) item_pre[pw][0] = 0;
      if constexpr (kPooled) {
        if (l < PPB) row_base[pw][l + 1] = rows_inc;
        if (l == 0) row_base[pw][0] = 0;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // more rows than the pool holds (every wavefront computes the same number): nothing of the angular pass is
    // evaluated or folded, the launch is marked as not counting and the host goes on with the big instantiation
    const bool pool_over = kPooled && row_base[kPooled ? pw : 0][PPB] > kPool;
    if (pool_over && threadIdx.x == 0) atomicMax(flags + 3, k_index + 1);
    const int n_list = kWaveLists ? wl_n : (pool_over ? 0 : item_pre[kWaveLists ? 0 : pw][kWaveLists ? 0 : PPB]);
    const int half = (n_list + 1) >> 1;
    const int q_lo = wave == 2 ? half : 0;                      // this wavefront's slice [q_lo, q_hi) of the list
    const int q_hi = wave == 1 ? half : n_list;
    const int n_total = q_hi - q_lo;
    const int n_sweeps = (n_total + 63) / 64;
    // bonded wave: one sweep over slots 0 / 1 of the 32 nucleotides, and a second over slots 2 / 3 only in
    // systems with circular strands (a ring's two ends carry a second bond in one role)
    const int my_sweeps = bonded_wave ? (pool_over ? 0 : (extra_bonds ? 2 : 1)) : n_sweeps;
    for (int sweep = 0; sweep < my_sweeps; ++sweep) {
      int p, idx, sl;
      bool active;
      if (bonded_wave) {
        p = (threadIdx.x & 63) >> 1;
        idx = (threadIdx.x & 1) + 2 * sweep;
        sl = idx;
        active = p < PPB;  // (16 lanes per nucleotide: the workgroup has 16 nucleotides, half a wavefront of bonded slots)
      } else {
        const int q = q_lo + sweep * 64 + (threadIdx.x & 63);
        active = q < q_hi;
        int k;
        if constexpr (kWaveLists) {
          const int src = (q >= wl_b1) + (q >= wl_b2) + (q >= wl_b3);  // the wavefront that appended item q
          const int at = q - (q >= wl_b3 ? wl_b3 : q >= wl_b2 ? wl_b2 : q >= wl_b1 ? wl_b1 : 0);
          const int2 it = wave_items[lst][src][at & (kWaveCap - 1)];  // (a lane past the end reads a slot nobody uses)
          p = it.y & (PPB - 1), k = it.y >> 8;  // (masked: what a lane past the end read is not an owner)
          sl = active ? it.x : -1;
        } else {
        int lo = 0, hi = PPB;  // owner: largest p with item_pre[pw][p] <= q
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (item_pre[pw][mid] <= q) lo = mid; else hi = mid;
        }
        p = lo;
        k = q - item_pre[pw][lo];
        sl = active ? items[lst][p][k] : -1;  // for these waves sl carries the row entry itself
        }
        // result row: the bonded slots, then the nucleotide's H-bond, cross-stacking and coaxial items
        idx = n_bonded_rows + k + (lst >= 1 ? item_cnt[0][p] : 0);
      }
      const int ip = bid * PPB + p;
      if (!active || ip >= n) continue;
      const int entry = bonded_wave ? rows[(size_t)ip * row_stride + sl] : sl;
      R* out_r = kPooled ? pool_row(row_base[kPooled ? pw : 0][p] + idx) : fixed_row(p, idx);
      SelfGrad<R> g;
      g.dc = g.g1 = g.g2 = g.g3 = V3<R>{R(0), R(0), R(0)};
      R ee[T_COUNT];
#pragma unroll
      for (int k = 0; k < T_COUNT; ++k) ee[k] = R(0);
      if (entry >= 0) {
        const int j = entry & ROW_INDEX_MASK;
        const bool role_p = bonded_wave ? ((sl & 1) == 1) : ((entry & ROW_ROLE_Q) == 0);
        const R* ms = self_lds[p];
        Nuc<R> me = nuc_from_lds(ms), o;
        set_meta(me, ms[9]);
        me.idx = ip, o.idx = j;  // (read only by the expectation of a probabilistic sequence)
        const V4 o0 = in.p0[j], o1 = in.p1[j], o2 = in.p2[j];
        V4 ol{};
        if constexpr (kHiLo<R>) ol = in.pl[j];
        o.c = xyz<R>(o0);
        o.a1 = xyz<R>(o1);
        o.a3 = xyz<R>(o2);
        o.a2 = cross(o.a3, o.a1);
        set_meta(o, o0.w);
        const V3<R> dco = min_image(centre_diff<R>(o0, ol, me.c, V3<R>{ms[10], ms[11], ms[12]}), box);
        // (oxNA: the pair templates pick vector, form and sites by the kind of the pair from the three vectors)
        const auto& PP = [&]() -> const auto& {
          if constexpr (MODEL == 4) return P4; else return P;
        }();
        if (wave == 0) {
          bonded_pair<R, MODEL, true, NoPG>(PP, me, o, dco, role_p, R(0.5), ee, g, pg);
        } else if (wave != 3) {
          unbonded_angular<R, MODEL, true, NoPG, 3>(PP, me, o, dco, role_p, R(0.5), ee, g, pg);
        } else {
          unbonded_angular<R, MODEL, true, NoPG, 4>(PP, me, o, dco, role_p, R(0.5), ee, g, pg);
        }
      }
      out_r[0] = g.dc.x, out_r[1] = g.dc.y, out_r[2] = g.dc.z;
      out_r[3] = g.g1.x, out_r[4] = g.g1.y, out_r[5] = g.g1.z;
      out_r[6] = g.g2.x, out_r[7] = g.g2.y, out_r[8] = g.g2.z;
      out_r[9] = g.g3.x, out_r[10] = g.g3.y, out_r[11] = g.g3.z;
      if constexpr (SAVE) {
#pragma unroll
        for (int k = 0; k < T_COUNT; ++k) out_r[12 + k] = ee[k];
      }
    }
  }
  // ---- integrator prologue, early: the wavefront with the coaxial role is the first to leave the angular pass
  //      (few items) and would idle at the barrier; it is also the one that integrates below, so it draws the
  //      thermostat noise and fetches momenta, quaternion and list-reference rows here, off the tail of the kernel
  //      where nothing else is left to hide their latency.  pin_vgpr keeps the values on this side of the barriers.
  const int int_wave = (3 - bid) & 3;  // the wavefront whose role above was 3
  const int il = threadIdx.x & 63;     // nucleotide of this lane in the integrating wave
  const int i_int = bid * PPB + il;
  const bool integrates = (int)(threadIdx.x >> 6) == int_wave && il < PPB && i_int < n;
  R z[6] = {R(0), R(0), R(0), R(0), R(0), R(0)};
  V4 pm{}, lm{}, qv{}, r0{}, f0{}, a0{};
  if (integrates) {
    pm = in.mom[i_int], lm = in.ang[i_int], qv = in.q[i_int];
    if (do_step && K.skin_half_sq > R(0)) r0 = ref_pos[i_int], f0 = ref_off[i_int], a0 = ref_a1[i_int];
    if (do_step) normals6(seed, (uint32_t)i_int, step, 0u, z);
#pragma unroll
    for (int k = 0; k < 6; ++k) pin_vgpr(z[k]);
    pin_vgpr(pm.x), pin_vgpr(pm.y), pin_vgpr(pm.z);
    pin_vgpr(lm.x), pin_vgpr(lm.y), pin_vgpr(lm.z);
    pin_vgpr(qv.x), pin_vgpr(qv.y), pin_vgpr(qv.z), pin_vgpr(qv.w);
  }
  __syncthreads();
  MD_PRIO(3);

  // ---- fold: each group gathers its owner's result rows (one per lane), adds the radial-pass
  //      site gradients, and reduces over its 8 lanes in a fixed order
  SelfGrad<R> sg;
  sg.dc = sg.g1 = sg.g2 = sg.g3 = V3<R>{R(0), R(0), R(0)};
  // (any wavefront's copy of row_base: they are identical, and complete since the barrier above)
  const int fw = kPooled ? (int)(threadIdx.x >> 6) : 0;
  const int rb = kPooled ? row_base[fw][grp] : 0;
  const bool pool_ok = !kPooled || row_base[fw][PPB] <= kPool;
  const int n_bonded_fold = extra_bonds ? ROW_BONDED_SLOTS : 2;  // rows 2, 3 exist only in systems with circular strands
  if (valid && pool_ok) {
    const int total = kPooled ? row_base[fw][grp + 1] - rb : n_bonded_fold + item_cnt[0][grp] + item_cnt[1][grp];
    for (int u = lane; u < total; u += G) {
      const R* rr = kPooled ? pool_row(rb + u) : fixed_row(grp, u);
      sg.dc = sg.dc + V3<R>{rr[0], rr[1], rr[2]};
      sg.g1 = sg.g1 + V3<R>{rr[3], rr[4], rr[5]};
      sg.g2 = sg.g2 + V3<R>{rr[6], rr[7], rr[8]};
      sg.g3 = sg.g3 + V3<R>{rr[9], rr[10], rr[11]};
      if constexpr (SAVE) {
#pragma unroll
        for (int k = 0; k < T_COUNT; ++k) e[k] += rr[12 + k];
      }
    }
  }
  if (lane == 0) {  // radial-pass sums (already folded over the group)
    const R* rl = rad_lds[grp];
    const V3<R> rbk{rl[0], rl[1], rl[2]}, rba{rl[3], rl[4], rl[5]};
    sg.dc = sg.dc - (rbk + rba);
    if constexpr (MODEL == 4) {  // the sites of this nucleotide's own type
      const bool r = self.rna != 0;
      axpy(sg.g1, -(r ? Prna[GEO_BACK_A1] : P[GEO_BACK_A1]), rbk);
      axpy(sg.g1, -(r ? Prna[GEO_BASE] : P[GEO_BASE]), rba);
      axpy(sg.g2, r ? R(0) : -P[GEO_BACK_A2], rbk);
      axpy(sg.g3, r ? -Prna[GEO_BACK_A2] : R(0), rbk);
    } else {
    axpy(sg.g1, -P[GEO_BACK_A1], rbk);
    axpy(sg.g1, -P[GEO_BASE], rba);
    if constexpr (MODEL == 2) axpy(sg.g2, -P[GEO_BACK_A2], rbk);
    if constexpr (MODEL == 3) axpy(sg.g3, -P[GEO_BACK_A2], rbk);  // oxRNA2: the backbone site's second axis is a3
    }
  }
  if constexpr (SAVE) {
    group_reduce<G, R, true>(e, sg);
  } else {
    group_reduce_v3<G>(sg.dc);
    group_reduce_v3<G>(sg.g1);
    group_reduce_v3<G>(sg.g2);
    group_reduce_v3<G>(sg.g3);
  }

  // the folded gradient of every nucleotide goes back to LDS (row 0 of its own result block, which only
  // this group has read) so that ONE wavefront integrates all 32 nucleotides of the workgroup, one per
  // lane: the integrator is ~0.6 k instructions per lane whatever the lane count, and run by lane 0 of
  // every group it occupied all four SIMDs at 1/8 lane use.  What goes back is the force and the body torque, not the
  // four gradients: the conversion (three cross products, three projections) is done here, by 32 lanes of four
  // wavefronts at once, instead of at the head of the integrating wavefront's stream behind the last barrier.
  if (lane == 0) {
    const Nuc<R> own = nuc_from_lds(self_lds[grp]);  // (the axes are read; the loads of the centre and the meta word are dropped)
    const V3<R> tl = axes_grad_to_torque(own, sg);
    R* fr = kPooled ? pool_row(pool_ok ? rb : grp * 2) : fixed_row(grp, 0);  // (pool exhausted: the launch does not count; any free row will do)
    fr[0] = -sg.dc.x, fr[1] = -sg.dc.y, fr[2] = -sg.dc.z;
    fr[3] = dot(own.a1, tl), fr[4] = dot(own.a2, tl), fr[5] = dot(own.a3, tl);
  }
  __syncthreads();
  MD_PRIO(4);
  double ke_t = 0.0, ke_r = 0.0;
  if (integrates) {
    const int i = i_int;
    const Nuc<R> self = nuc_from_lds(self_lds[il]);
    // force and body torque of this nucleotide, as the fold left them
    const R* fr = kPooled ? pool_row(row_base[fw][PPB] <= kPool ? row_base[fw][il] : il * 2) : fixed_row(il, 0);
    const V3<R> F{fr[0], fr[1], fr[2]};
    const R tb[3] = {fr[3], fr[4], fr[5]};
    const bool int_rna = (MODEL == 4) && meta_of(self_lds[il][9]).rna;  // oxNA: this nucleotide's own geometry
    const R g_k1 = int_rna ? Prna[GEO_BACK_A1] : P[GEO_BACK_A1];
    const R g_k2 = (MODEL >= 2) ? (int_rna ? Prna[GEO_BACK_A2] : P[GEO_BACK_A2]) : R(0);
    R p[3] = {pm.x, pm.y, pm.z}, L[3] = {lm.x, lm.y, lm.z};
    R qs[4] = {qv.x, qv.y, qv.z, qv.w};
    const R kc = kick_close * K.dt;
    p[0] += kc * F.x;
    p[1] += kc * F.y;
    p[2] += kc * F.z;
    L[0] += kc * tb[0];
    L[1] += kc * tb[1];
    L[2] += kc * tb[2];
    if constexpr (SAVE) {
      ke_t = 0.5 * double(K.inv_mass) * (double(p[0]) * p[0] + double(p[1]) * p[1] + double(p[2]) * p[2]);
      ke_r = 0.5 * (double(K.inv_inertia[0]) * L[0] * L[0] + double(K.inv_inertia[1]) * L[1] * L[1] +
                    double(K.inv_inertia[2]) * L[2] * L[2]);
      if (traj_c) {
        traj_c[3 * i + 0] = self.c.x;
        traj_c[3 * i + 1] = self.c.y;
        traj_c[3 * i + 2] = self.c.z;
      }
      if (traj_q) {
        traj_q[4 * i + 0] = qs[0];
        traj_q[4 * i + 1] = qs[1];
        traj_q[4 * i + 2] = qs[2];
        traj_q[4 * i + 3] = qs[3];
      }
    }
    R x[3] = {self.c.x, self.c.y, self.c.z};
    R xl[3] = {self_lds[il][10], self_lds[il][11], self_lds[il][12]};  // low part of the centre (fp32 runs)
    R dxa[3] = {R(0), R(0), R(0)};                                      // this step's displacement
    R* const xd = kHiLo<R> ? dxa : x;
    V3<R> n1 = self.a1, n2 = self.a2, n3 = self.a3;
    // second axis of the backbone site (a2; a3 in oxRNA2), selected by VALUE (a select between the two locals' addresses
    // kept both in scratch memory in the oxNA instantiations)
    const bool bk3 = MODEL == 3 || int_rna;
    V3<R> nbk{bk3 ? n3.x : n2.x, bk3 ? n3.y : n2.y, bk3 ? n3.z : n2.z};
    if (do_step) {
      p[0] += K.half_dt * F.x;
      p[1] += K.half_dt * F.y;
      p[2] += K.half_dt * F.z;
      L[0] += K.half_dt * tb[0];
      L[1] += K.half_dt * tb[1];
      L[2] += K.half_dt * tb[2];
      drift(xd, qs, p, L, K.half_dt, K);
      p[0] = K.c1_t * p[0] + K.c2_t * z[0];
      p[1] = K.c1_t * p[1] + K.c2_t * z[1];
      p[2] = K.c1_t * p[2] + K.c2_t * z[2];
      L[0] = K.c1_r * L[0] + K.c2_r[0] * z[3];
      L[1] = K.c1_r * L[1] + K.c2_r[1] * z[4];
      L[2] = K.c1_r * L[2] + K.c2_r[2] * z[5];
      drift(xd, qs, p, L, K.half_dt, K);
      if constexpr (kHiLo<R>) {
        // centre += displacement in (hi, lo) form: the displacement goes to the low part, then one fast two-sum
        // re-normalises (|hi| >= |lo + d| always holds here)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const R sdl = xl[k] + dxa[k];
          const R t = x[k] + sdl;
          xl[k] = sdl - (t - x[k]);
          x[k] = t;
        }
      }
      // keep the quaternion on the unit sphere (fp32 round-off)
      const R inv = m_rsqrt(qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3]);
      qs[0] *= inv;
      qs[1] *= inv;
      qs[2] *= inv;
      qs[3] *= inv;
      if (!(x[0] == x[0]) || !(qs[0] == qs[0])) atomicOr(flags, 2);
      quat_axes(qs[0], qs[1], qs[2], qs[3], n1, n2, n3);
      nbk = V3<R>{bk3 ? n3.x : n2.x, bk3 ? n3.y : n2.y, bk3 ? n3.z : n2.z};
      if (K.skin_half_sq > R(0)) {
        // the list is valid while neither the centre nor the backbone and base sites (the segments are selected
        // by site distances, and a rotation moves the sites) have travelled more than skin / 2 since the build
        const R dx = x[0] - r0.x, dy = x[1] - r0.y, dz = x[2] - r0.z;
        const R bx = dx + (g_k1 * n1.x + g_k2 * nbk.x - f0.x), by = dy + (g_k1 * n1.y + g_k2 * nbk.y - f0.y),
                bz = dz + (g_k1 * n1.z + g_k2 * nbk.z - f0.z);
        // base site c + g_base a1 (the stacking site lies between it and the centre)
        const R gb = int_rna ? Prna[GEO_BASE] : P[GEO_BASE];
        const R sx = dx + gb * (n1.x - a0.x), sy = dy + gb * (n1.y - a0.y), sz = dz + gb * (n1.z - a0.z);
        if (dx * dx + dy * dy + dz * dz > K.skin_half_sq || bx * bx + by * by + bz * bz > K.skin_half_sq ||
            sx * sx + sy * sy + sz * sz > K.skin_half_sq)
          atomicMax(flags + 1, k_index + 1);  // the list is stale for the NEXT force evaluation: launch k + 1 halts
      }
    }
    if constexpr (!SAVE) {
      // Positions-only trajectory (the reference's run: every step's state.position and nothing else,
      // simulators/jax_md/jaxmd.py:84-99): the launch that PRODUCES x_{k+1} also writes it to the caller's row - the
      // values it has just put into the next frame (fp32: the high part of the centre, what store hands out), behind a
      // wave-uniform test.  No energy-trace instantiation, no reduction launch, no closing launch for the last row.
      if (traj_c) {
        traj_c[3 * i + 0] = x[0];
        traj_c[3 * i + 1] = x[1];
        traj_c[3 * i + 2] = x[2];
      }
      if (traj_q) reinterpret_cast<V4*>(traj_q)[i] = V4{qs[0], qs[1], qs[2], qs[3]};
    }
    out.p0[i] = V4{x[0], x[1], x[2], self_lds[il][9]};
    if constexpr (kHiLo<R>) out.pl[i] = V4{xl[0], xl[1], xl[2], R(0)};
    out.p1[i] = V4{n1.x, n1.y, n1.z, R(0)};
    out.p2[i] = V4{n3.x, n3.y, n3.z, R(0)};
    // (a closing-only launch hands the frame on unchanged, bit for bit: the offset is copied, not re-derived from
    // axes whose cross product may round differently - advance(a); advance(b) then equals advance(a + b) exactly)
    out.p3[i] = do_step ? V4{g_k1 * n1.x + g_k2 * nbk.x, g_k1 * n1.y + g_k2 * nbk.y, g_k1 * n1.z + g_k2 * nbk.z, R(0)} : in.p3[i];
    out.q[i] = V4{qs[0], qs[1], qs[2], qs[3]};
    out.mom[i] = V4{p[0], p[1], p[2], R(0)};
    out.ang[i] = V4{L[0], L[1], L[2], R(0)};
  }
  if constexpr (SAVE) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < T_COUNT; ++k) e_lds[grp][k] = valid ? double(e[k]) : 0.0;
    }
    if ((int)(threadIdx.x >> 6) == int_wave && il < PPB) {
      e_lds[il][T_COUNT] = ke_t;
      e_lds[il][T_COUNT + 1] = ke_r;
    }
    __syncthreads();
    if (threadIdx.x < kTraceWidth) {
      double s = 0.0;
      for (int g = 0; g < PPB; ++g) s += e_lds[g][threadIdx.x];
      e_part[(size_t)bid * kTraceWidth + threadIdx.x] = s;
    }
  }
}

}  // namespace mythos
