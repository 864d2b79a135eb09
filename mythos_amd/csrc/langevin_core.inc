// (langevin_core.inc: the kernels and host templates of the oxDNA Langevin integrator, included by langevin.hip - the
// fp32 instantiations and the C entry points - and by langevin_f64.hip - the fp64 instantiations; two translation units
// because the two precisions want different compiler switches, see the Makefile)
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
//   phase 1 (radial): the lanes stride over the nucleotide's unbonded row, close segment then far segment;
//           per neighbour they read the centre (hi, lo), the backbone offset and - in the close segment -
//           a1, evaluate Debye-Hueckel and the excluded-volume site pairs with early-outs on squared
//           distances, and flag the few neighbours whose base-base / stack-stack distance lies in the
//           support of an angular term (two LDS lists per nucleotide: base-pair terms, coaxial stacking);
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
  const int md_kind = (MODEL == 4) ? na1_kind(self.rna, ((int)o0.w >> 3) & 1) : 0;                                 \
  const RadSet<R> rs_picked = (MODEL == 4) ? pick3(rs0, rs1, rs2, md_kind) : rs0;                                  \
  const RadSet<R>& rs = (MODEL == 4) ? rs_picked : rs0;
__device__ __forceinline__ int na1_kind(int self_rna, int other_rna) { return (self_rna && other_rna) ? 1 : ((self_rna || other_rna) ? 2 : 0); }

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
// each radial loop instead of two, and round 4 measured the second iterations at 30 % of the kernel (DESIGN section 8).
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
  __shared__ int items[2][PPB][ITEMS];  // the flagged row ENTRIES (index | role bit), not their slots
  __shared__ int item_cnt[2][PPB];
  __shared__ int item_pre[4][PPB + 1];  // per WAVEFRONT: the prefix of the list that wavefront will walk
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
    const int m = (int)s0.w;
    self.seq = m & 3;
    self.is_end = (m >> 2) & 1;
    self.rna = (m >> 3) & 1;
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
  const int row_room = ITEMS - (extra_bonds ? ROW_BONDED_SLOTS - 2 : 0);  // result rows left for flagged neighbours
  const int lane64 = threadIdx.x & 63;
  const int gshift = lane64 & ~(G - 1);
  // Software pipeline: the lane's row entries are fetched kEnt at a time, and the neighbour
  // state (centre, backbone offset) of entry k+1 is requested before entry k is evaluated, so the
  // L2 / Infinity-Cache round trips overlap the arithmetic instead of serialising with it.
  // (rolled: keeping the body once in the instruction stream matters more than unrolling - the whole
  // kernel has to stay inside the instruction cache that two CUs share)
  // (the prefetches are unconditional: an entry past the end of the segment is read from the segment's last slot and
  // replaced by -1, a missing neighbour's state is read from the lane's OWN nucleotide and never used - lines that are
  // in the cache anyway; a load behind a lane-dependent branch made the compiler wait for ALL outstanding loads at
  // the join, the one just issued included)
  auto row_at = [&](int s, int end) -> int {
    const int v = row[max(min(s, end - 1), 0)];
    return s < end ? v : -1;
  };
  auto slot_of_entry = [&](int e) -> int { return e >= 0 ? (e & ROW_INDEX_MASK) : ii; };
  {
    int e_cur = -1, e_nxt = -1;
    V4 n0{}, n3{}, n1{}, nl{};
    {
      const int s = ROW_BONDED_SLOTS + lane;
      e_cur = row_at(s, close_end);
      e_nxt = row_at(s + G, close_end);
      const int j = slot_of_entry(e_cur);
      n0 = in.p0[j];
      n3 = in.p3[j];
      n1 = in.p1[j];
      if constexpr (kHiLo<R>) nl = in.pl[j];
    }
#pragma unroll 1
    for (int s0 = ROW_BONDED_SLOTS; s0 < close_end; s0 += G) {
      const int s = s0 + lane;
      const int entry = e_cur;
      const V4 o0 = n0, o3 = n3, o1 = n1, ol = nl;
      e_cur = e_nxt;
      e_nxt = row_at(s + 2 * G, close_end);
      {  // the close segment reads a1 as well: nearly all of its entries need it
        const int jn = slot_of_entry(e_cur);
        n0 = in.p0[jn];
        n3 = in.p3[jn];
        n1 = in.p1[jn];
        if constexpr (kHiLo<R>) nl = in.pl[jn];
      }
      bool flag[2] = {false, false};
      if (entry >= 0) {
        const bool role_p = (entry & ROW_ROLE_Q) == 0;
        MD_RADSET_OF_ENTRY
        const bool o_rna = (MODEL == 4) && ((((int)o0.w) >> 3) & 1);
        const R gba_s = (MODEL == 4 && self.rna) ? Prna[GEO_BASE] : g_ba, gba_o = o_rna ? Prna[GEO_BASE] : g_ba;
        const R gst_s = (MODEL == 4 && self.rna) ? Prna[GEO_STACK] : g_st, gst_o = o_rna ? Prna[GEO_STACK] : g_st;
        (void)gst_s, (void)gst_o;
        const V3<R> dco = min_image(centre_diff<R>(o0, ol, self.c, self_lo), box);
        const V3<R> offb_o = xyz<R>(o3);
        const bool close = dot(dco, dco) < cut.rcom2;
        // backbone - backbone: excluded volume + Debye-Hueckel
        {
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
              if (rs.half_ends) {
                const int mo = (int)o0.w;
                mult = (self.is_end ? R(0.5) : R(1)) * (((mo >> 2) & 1) ? R(0.5) : R(1));
              }
              dVdr += rs.tw_dh * mult * dh.d;
              if constexpr (SAVE) e[T_DH] += R(0.5) * mult * dh.f;
            }
            if constexpr (SAVE) e[T_NEXC] += R(0.5) * en;
            axpy(gbk, dVdr / r, d);
          }
        }
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
            flag[0] = rs.cr_lo2 < r2 && r2 < rs.cr_hi2;
            if (!flag[0] && rs.hb_lo2 < r2 && r2 < rs.hb_hi2) {  // H-bond only for pairs with a non-zero weight
              const int so = (int)o0.w & 3;
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
            flag[1] = rs.cx_lo2 < r2 && r2 < rs.cx_hi2;
          }
          if constexpr (SAVE) e[T_NEXC] += R(0.5) * en;
        }
      }
      // append the flagged slots of this group to its two LDS lists, in slot order
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const unsigned long long bal = __ballot(flag[t]);
        const unsigned int gm = (unsigned int)(bal >> gshift) & ((1u << G) - 1u);
        if (flag[t]) {
          const int pos = n_items[t] + __popc(gm & ((1u << lane) - 1u));
          if (pos < ITEMS) items[t][grp][pos] = entry;  // (row_room <= ITEMS; an over-full nucleotide aborts the launch below)
        }
        n_items[t] += __popc(gm);
      }
    }
  }
  // far segment: only the backbone-backbone terms (excluded volume + Debye-Hueckel) can act
  MD_PRIO(1);
  {
    int e_cur = -1, e_nxt = -1;
    V4 n0{}, n3{}, nl{};
    {
      const int s = close_end + lane;
      e_cur = row_at(s, len);
      e_nxt = row_at(s + G, len);
      const int j = slot_of_entry(e_cur);
      n0 = in.p0[j];
      n3 = in.p3[j];
      if constexpr (kHiLo<R>) nl = in.pl[j];
    }
#pragma unroll 1
    for (int s0 = close_end; s0 < len; s0 += G) {
      const int s = s0 + lane;
      const int entry = e_cur;
      const V4 o0 = n0, o3 = n3, ol = nl;
      e_cur = e_nxt;
      e_nxt = row_at(s + 2 * G, len);
      {
        const int jn = slot_of_entry(e_cur);
        n0 = in.p0[jn];
        n3 = in.p3[jn];
        if constexpr (kHiLo<R>) nl = in.pl[jn];
      }
      if (entry >= 0) {
        MD_RADSET_OF_ENTRY
        const V3<R> dco = min_image(centre_diff<R>(o0, ol, self.c, self_lo), box);
        const V3<R> d = dco + xyz<R>(o3) - offb_s;
        const R r2 = dot(d, d);
        if (r2 < rs.rbb2) {
          const R r = m_sqrt(r2);
          const FD<R> v = f3_eval(r, rs.eps_n, rs.f_bb);
          R dVdr = rs.tw_n * v.d;
          if constexpr (MODEL >= 2) {
            const FD<R> dh = debye_eval(r, rs.dhp);
            R mult = R(1);
            if (rs.half_ends) {
              const int mo = (int)o0.w;
              mult = (self.is_end ? R(0.5) : R(1)) * (((mo >> 2) & 1) ? R(0.5) : R(1));
            }
            dVdr += rs.tw_dh * mult * dh.d;
            if constexpr (SAVE) e[T_DH] += R(0.5) * mult * dh.f;
          }
          if constexpr (SAVE) e[T_NEXC] += R(0.5) * v.f;
          axpy(gbk, dVdr / r, d);
        }
      }
    }
  }
  if (n_items[0] + n_items[1] > row_room) {  // result rows of one nucleotide exhausted: this launch does not count
    if (lane == 0) atomicMax(flags + 3, k_index + 1);
    n_items[0] = n_items[1] = 0;
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
    {
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
    const int n_list = pool_over ? 0 : item_pre[pw][PPB];
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
        int lo = 0, hi = PPB;  // owner: largest p with item_pre[pw][p] <= q
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (item_pre[pw][mid] <= q) lo = mid; else hi = mid;
        }
        p = lo;
        const int k = q - item_pre[pw][lo];
        sl = active ? items[lst][p][k] : -1;  // for these waves sl carries the row entry itself
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
        Nuc<R> me, o;
        const R* ms = self_lds[p];
        me.c = V3<R>{ms[0], ms[1], ms[2]};
        me.a1 = V3<R>{ms[3], ms[4], ms[5]};
        me.a3 = V3<R>{ms[6], ms[7], ms[8]};
        me.a2 = cross(me.a3, me.a1);
        const int mm = (int)ms[9];
        me.seq = mm & 3;
        me.is_end = (mm >> 2) & 1;
        me.rna = (mm >> 3) & 1;
        me.idx = ip, o.idx = j;  // (read only by the expectation of a probabilistic sequence)
        const V4 o0 = in.p0[j], o1 = in.p1[j], o2 = in.p2[j];
        V4 ol{};
        if constexpr (kHiLo<R>) ol = in.pl[j];
        o.c = xyz<R>(o0);
        o.a1 = xyz<R>(o1);
        o.a3 = xyz<R>(o2);
        o.a2 = cross(o.a3, o.a1);
        const int mo = (int)o0.w;
        o.seq = mo & 3;
        o.is_end = (mo >> 2) & 1;
        o.rna = (mo >> 3) & 1;
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
    Nuc<R> own;
    const R* ms = self_lds[grp];
    own.a1 = V3<R>{ms[3], ms[4], ms[5]};
    own.a3 = V3<R>{ms[6], ms[7], ms[8]};
    own.a2 = cross(own.a3, own.a1);
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
    Nuc<R> self;
    {
      const R* ms = self_lds[il];
      self.c = V3<R>{ms[0], ms[1], ms[2]};
      self.a1 = V3<R>{ms[3], ms[4], ms[5]};
      self.a3 = V3<R>{ms[6], ms[7], ms[8]};
      self.a2 = cross(self.a3, self.a1);
    }
    // force and body torque of this nucleotide, as the fold left them
    const R* fr = kPooled ? pool_row(row_base[fw][PPB] <= kPool ? row_base[fw][il] : il * 2) : fixed_row(il, 0);
    const V3<R> F{fr[0], fr[1], fr[2]};
    const R tb[3] = {fr[3], fr[4], fr[5]};
    const bool int_rna = (MODEL == 4) && ((((int)self_lds[il][9]) >> 3) & 1);  // oxNA: this nucleotide's own geometry
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

using namespace mythos;

struct mythos_sim : mythos::MdRun {
  mythos_system* sys = nullptr;
  int device = 0;  // the system's, copied at create: the integrator may outlive its system, to be destroyed only
  double dt = 0, kT = 0, gamma_t = 0, gamma_r = 0, mass = 1, inertia[3] = {1, 1, 1};
  // neighbour policy (MdRun::rebuild_every: 0 = the system's static rows)
  double r_cut = 0, skin = 0;
  // device state: two ping-pong frames of 8 vec4 arrays each (p0, p1, p2, p3, q, pl, mom, ang)
  static constexpr int kFrameArrays = 8;
  DeviceBytes frame[2][kFrameArrays];
  int builds = 0;          // scheduled rebuilds so far (the chunk order is refreshed every 64th)
  int list_epoch = 0;      // sys->list_epoch the rows in use belong to
  // centres as the last run handed them out (hi) and the low parts that went with them (fp32 systems)
  DeviceBytes keep_hi, keep_lo;
  bool keep_valid = false;
  bool items_big = false;              // the ITEMS = 32 instantiation is in use (a launch of this load found 16 too few)
  bool want_unfused = false;           // mythos_langevin_set_option(MYTHOS_LANGEVIN_UNFUSED): takes effect at the next load
  bool unfused = false;                // the resident state lives in the unfused path's buffers (decided by load)
  int param_epoch = 0;                 // sys->param_epoch the packed site offsets of the resident frames were derived from
  int lanes = kMdG;              // lanes per nucleotide of the step launches of this load (8, or 16 for small systems: md_lanes_for)
  DeviceBuf<int> d_chunk_order;  // [blocks] spatial order of the workgroups' chunks of nucleotides (null: index order)
  DeviceBuf<unsigned long long> d_chunk_keys;
  DeviceBuf<double> d_epart;     // [blocks][kTraceWidth] energy-trace partials of a saving launch
  // oxNA (model 4), unfused path: packed state + gradients of the energy kernel + list reference (see unfused_*)
  DeviceBytes u_c, u_q, u_p, u_l, u_gc, u_gq, u_ref;
  DeviceBuf<double> u_e;  // [8] term energies of the last force evaluation + [2] kinetic energies
  bool u_forces_valid = false;
  // constant external forces (mythos_langevin_set_external_forces), in the system's precision
  int ext_count = 0;
  DeviceBuf<int> d_ext_index;                  // [ext_count] distinct nucleotides
  DeviceBytes d_ext_force;                     // [ext_count] Vec4T<R>: (F, 0)
  DeviceBuf<unsigned long long> d_ext_stamp;   // [1] the last kick applied (ext_kick_kernel)
  bool ext_stamp_stale = true;                 // load / set_step / set_external_forces: cleared in front of the next kick
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

// Lanes per nucleotide for this system (see md_step_kernel, GL): 16 where the doubled grid is at most two workgroups per CU
// (all resident with room to spare: n <= 8 192 on 256 CUs), 8 otherwise.  mythos_debug_set(MYTHOS_DEBUG_MD_LANES, 8 | 16) overrides.
static int md_lanes_for(const mythos_system* sys) {
  const long long dbg = debug_value(MYTHOS_DEBUG_MD_LANES);
  if (dbg == 8 || dbg == 16) return (int)dbg;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sys->device);
  const int grid16 = (sys->n + 15) / 16;
  return 2 * grid16 <= 3 * cus ? 16 : 8;  // measured (r04_experiments.md): 16 lanes win to 6 k nt, lose from 10 k nt
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
  sim->param_epoch = sys->param_epoch;
  sim->lanes = md_lanes_for(sys);
  const int ppb = kMdBlock / sim->lanes;
  return update_chunk_order<R>(sim, f0.p0, (n + ppb - 1) / ppb, st);
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
  const bool lanes16 = sim->lanes == 16;
  const int ppb = kMdBlock / sim->lanes;
  const int blocks = (n + ppb - 1) / ppb;
  const int grid = 8 * ((blocks + 7) / 8);  // padded for the kernel's XCD-aware workgroup order
  int sim_cus = 256;  // compute units of the device: a grid of more than four workgroups per CU takes the DENSE instantiation
  (void)hipDeviceGetAttribute(&sim_cus, hipDeviceAttributeMultiprocessorCount, sys->device);
  const long long dbg_dense = debug_value(MYTHOS_DEBUG_MD_DENSE);  // (tests: 1 forces the DENSE instantiation, 2 forbids it)
  const bool dense_grid = !lanes16 && (dbg_dense == 1 || (dbg_dense != 2 && grid > 4 * sim_cus));
  const int prio_on = (sizeof(R) == 8 && grid > 3 * sim_cus) ? 0 : 1;  // (see MYTHOS_MD_PRIO_MAP)
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
    auto launch_pseq = [&](auto save_tag, auto items_tag, hipEvent_t ea, hipEvent_t eb) {
      constexpr bool SV = decltype(save_tag)::value;
      constexpr int IT = decltype(items_tag)::value;
      auto go = [&](auto lanes_tag) {
        hipExtLaunchKernelGGL((md_step_kernel<R, MODEL, SV, IT, true, false, decltype(lanes_tag)::value>), dim3(grid), dim3(kMdBlock), 0, st, ea, eb, 0,
                              Pdev, box, K, cut, n, fr[cur], fr[cur ^ 1], sys->list.d_rows.get(), sys->d_row_len.get(), row_close_of(sys),
                              sys->list.stride, sys->extra_bonds ? 1 : 0, kick_close, row.do_step, sim->seed, (uint64_t)(sim->step + k), ref,
                              ref_off, ref_a1, sim->d_flags.get(), tc, tq, sim->d_epart.get(), sim->d_chunk_order.get(), halt_words, k, 0, prio_on, pseq);
      };
      if (lanes16) go(std::integral_constant<int, 16>{}); else go(std::integral_constant<int, 8>{});
    };
    auto launch = [&](auto save_tag, auto items_tag, hipEvent_t ea, hipEvent_t eb) {
      constexpr bool SV = decltype(save_tag)::value;
      constexpr int IT = decltype(items_tag)::value;
      // with events: the pair receives the begin / end time stamps of THIS dispatch (the same stamps a profiler's
      // kernel trace reports), not the time between two markers in the queue
      auto go = [&](auto dense_tag, auto lanes_tag) {
        hipExtLaunchKernelGGL((md_step_kernel<R, MODEL, SV, IT, false, decltype(dense_tag)::value, decltype(lanes_tag)::value>), dim3(grid), dim3(kMdBlock), 0, st, ea, eb, 0,
                              Pdev, box, K, cut, n, fr[cur], fr[cur ^ 1], sys->list.d_rows.get(), sys->d_row_len.get(), row_close_of(sys),
                              sys->list.stride, sys->extra_bonds ? 1 : 0, kick_close, row.do_step, sim->seed, (uint64_t)(sim->step + k), ref,
                              ref_off, ref_a1, sim->d_flags.get(), tc, tq, sim->d_epart.get(), sim->d_chunk_order.get(), halt_words, k, 0, prio_on, PseqView<R>{});
      };
      using L8 = std::integral_constant<int, 8>;
      using L16 = std::integral_constant<int, 16>;
      if (lanes16) {
        go(std::false_type{}, L16{});
      } else if constexpr (sizeof(R) == 4 && !SV && IT == kMdItems && MODEL <= 2) {
        if (dense_grid) go(std::true_type{}, L8{}); else go(std::false_type{}, L8{});
      } else {
        go(std::false_type{}, L8{});
      }
    };
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
    using T = std::true_type;
    using F = std::false_type;
    using Small = std::integral_constant<int, kMdItems>;
    using BigS = std::integral_constant<int, md_items_big<R, true>()>;
    using BigN = std::integral_constant<int, md_items_big<R, false>()>;
    const hipEvent_t ea = row.ea, eb = row.eb;
    if (use_pseq) {
      if (save) {
        if (sim->items_big) launch_pseq(T{}, BigS{}, ea, eb); else launch_pseq(T{}, Small{}, ea, eb);
      } else {
        if (sim->items_big) launch_pseq(F{}, BigN{}, ea, eb); else launch_pseq(F{}, Small{}, ea, eb);
      }
    } else if (save) {
      if (sim->items_big) launch(T{}, BigS{}, ea, eb); else launch(T{}, Small{}, ea, eb);
    } else {
      if (sim->items_big) launch(F{}, BigN{}, ea, eb); else launch(F{}, Small{}, ea, eb);
    }
    if (save)
      hipLaunchKernelGGL(reduce_trace_kernel<kTraceWidth>, dim3(1), dim3(256), 0, st, sim->d_epart.get(), blocks,
                         e_trace + (size_t)row.sidx * kTraceWidth);
  };
  auto rebuild = [&](int buf) -> int {
    if ((++sim->builds & 63) == 0)
      if (int rc = update_chunk_order<R>(sim, fr[buf].p0, blocks, st)) return rc;
    return rows_build_device(sys, fr[buf].p0, true, sim->r_cut, sim->skin, fr[buf].p3, fr[buf].p1, true, st);
  };
  auto rebuild_until_fit = [&](int buf) -> int {
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

// ------------------------------------------------------------------------------------------------
// oxNA (model 4): the UNFUSED path, behind MYTHOS_NA1_UNFUSED=1 - a second implementation of a hybrid system's dynamics
// that the tests hold md_step_kernel<R, 4, ...> to (it came first and stayed as the cross-check).  Two launches per step:
// the energy kernel's forces instantiation (dU/dcentre, dU/dquaternion of the packed state), then this integrator
// kernel, one thread per nucleotide: the same B A O A | B map, Philox stream and free-rotor drift as md_step_kernel's
// integrator (shared device functions), so a trajectory is held to the same oracle.
// The list: static rows (mythos_oxdna_set_neighbors), or the integrator's policy - rows of range r_cut + skin rebuilt
// every rebuild_every steps from the centres; the host looks at the skin flag at every rebuild (it synchronises there
// anyway) and a violation is an error (no halt-and-resume on this path): shorten the interval or widen the skin.
// ------------------------------------------------------------------------------------------------
template <typename R>
__global__ void unfused_integrate_kernel(int n, const LangevinConst<R> K, R* __restrict__ c, R* __restrict__ q, R* __restrict__ p,
                                         R* __restrict__ L, const R* __restrict__ gc, const R* __restrict__ gq, R kick_close,
                                         int do_step, uint64_t seed, uint64_t step, const R* __restrict__ ref, R site_reach,
                                         int* __restrict__ flags, R* __restrict__ traj_c, R* __restrict__ traj_q,
                                         double* __restrict__ ke /* [2], atomics; null: not wanted */) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double ke_t = 0.0, ke_r = 0.0;
  if (i < n) {
    R x[3] = {c[3 * i], c[3 * i + 1], c[3 * i + 2]};
    R qs[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
    R pp[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]}, LL[3] = {L[3 * i], L[3 * i + 1], L[3 * i + 2]};
    const R F[3] = {-gc[3 * i], -gc[3 * i + 1], -gc[3 * i + 2]};
    const R g0 = gq[4 * i], g1 = gq[4 * i + 1], g2 = gq[4 * i + 2], g3 = gq[4 * i + 3];
    // body torque from the quaternion gradient: tau_k = -1/2 (P_k q) . dU/dq (NO_SQUISH permutations)
    const R tb[3] = {R(-0.5) * (-qs[1] * g0 + qs[0] * g1 + qs[3] * g2 - qs[2] * g3),
                     R(-0.5) * (-qs[2] * g0 - qs[3] * g1 + qs[0] * g2 + qs[1] * g3),
                     R(-0.5) * (-qs[3] * g0 + qs[2] * g1 - qs[1] * g2 + qs[0] * g3)};
    const R kc = kick_close * K.dt;
#pragma unroll
    for (int k = 0; k < 3; ++k) pp[k] += kc * F[k], LL[k] += kc * tb[k];
    if (ke) {
      ke_t = 0.5 * double(K.inv_mass) * (double(pp[0]) * pp[0] + double(pp[1]) * pp[1] + double(pp[2]) * pp[2]);
      ke_r = 0.5 * (double(K.inv_inertia[0]) * LL[0] * LL[0] + double(K.inv_inertia[1]) * LL[1] * LL[1] +
                    double(K.inv_inertia[2]) * LL[2] * LL[2]);
    }
    if (traj_c) traj_c[3 * i] = x[0], traj_c[3 * i + 1] = x[1], traj_c[3 * i + 2] = x[2];
    if (traj_q) traj_q[4 * i] = qs[0], traj_q[4 * i + 1] = qs[1], traj_q[4 * i + 2] = qs[2], traj_q[4 * i + 3] = qs[3];
    if (do_step) {
      R z[6];
      normals6(seed, (uint32_t)i, step, 0u, z);
#pragma unroll
      for (int k = 0; k < 3; ++k) pp[k] += K.half_dt * F[k], LL[k] += K.half_dt * tb[k];
      drift(x, qs, pp, LL, K.half_dt, K);
#pragma unroll
      for (int k = 0; k < 3; ++k) pp[k] = K.c1_t * pp[k] + K.c2_t * z[k], LL[k] = K.c1_r * LL[k] + K.c2_r[k] * z[3 + k];
      drift(x, qs, pp, LL, K.half_dt, K);
      const R inv = m_rsqrt(qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k) qs[k] *= inv;
      if (!(x[0] == x[0]) || !(qs[0] == qs[0])) atomicOr(flags, 2);
      if (ref != nullptr) {
        // no site may have moved more than skin / 2 since the build: |d site| <= |d centre| + sum_k |coef_k| |d a_k|
        // (site_reach bounds the sum of the offset coefficients of any site in either geometry)
        V3<R> a1, a2, a3;
        quat_axes(qs[0], qs[1], qs[2], qs[3], a1, a2, a3);
        const R* rr = ref + 12 * (size_t)i;
        const V3<R> dx{x[0] - rr[0], x[1] - rr[1], x[2] - rr[2]};
        const V3<R> d1{a1.x - rr[3], a1.y - rr[4], a1.z - rr[5]}, d2{a2.x - rr[6], a2.y - rr[7], a2.z - rr[8]},
            d3{a3.x - rr[9], a3.y - rr[10], a3.z - rr[11]};
        const R da = m_sqrt(fmax(dot(d1, d1), fmax(dot(d2, d2), dot(d3, d3))));
        const R moved = m_sqrt(dot(dx, dx)) + site_reach * da;
        if (moved * moved > K.skin_half_sq) atomicOr(flags + 1, 1);
      }
      c[3 * i] = x[0], c[3 * i + 1] = x[1], c[3 * i + 2] = x[2];
      q[4 * i] = qs[0], q[4 * i + 1] = qs[1], q[4 * i + 2] = qs[2], q[4 * i + 3] = qs[3];
    }
    p[3 * i] = pp[0], p[3 * i + 1] = pp[1], p[3 * i + 2] = pp[2];
    L[3 * i] = LL[0], L[3 * i + 1] = LL[1], L[3 * i + 2] = LL[2];
  }
  if (ke) {  // one atomic pair per wavefront
    for (int o = 32; o > 0; o >>= 1) ke_t += __shfl_down(ke_t, o, 64), ke_r += __shfl_down(ke_r, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(ke, ke_t), atomicAdd(ke + 1, ke_r);
  }
}

// list reference of the unfused path: centre and the three axes at build time
template <typename R>
__global__ void unfused_ref_kernel(int n, const R* __restrict__ c, const R* __restrict__ q, R* __restrict__ ref) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3<R> a1, a2, a3;
  quat_axes(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3], a1, a2, a3);
  R* rr = ref + 12 * (size_t)i;
  rr[0] = c[3 * i], rr[1] = c[3 * i + 1], rr[2] = c[3 * i + 2];
  rr[3] = a1.x, rr[4] = a1.y, rr[5] = a1.z, rr[6] = a2.x, rr[7] = a2.y, rr[8] = a2.z, rr[9] = a3.x, rr[10] = a3.y, rr[11] = a3.z;
}

static __global__ void unfused_trace_kernel(const double* __restrict__ e, double* __restrict__ row) {
  if (threadIdx.x < kTraceWidth) row[threadIdx.x] = e[threadIdx.x];
}

template <typename R>
static int unfused_alloc(mythos_sim* sim) {
  if (sim->u_e) return 0;  // (the last of them: a partly failed attempt is made again)
  const size_t n = (size_t)sim->sys->n;
  for (DeviceBytes* b : {&sim->u_c, &sim->u_p, &sim->u_l, &sim->u_gc})
    if (int rc = b->alloc(3 * n * sizeof(R))) return rc;
  for (DeviceBytes* b : {&sim->u_q, &sim->u_gq})
    if (int rc = b->alloc(4 * n * sizeof(R))) return rc;
  if (int rc = sim->u_ref.alloc(12 * n * sizeof(R))) return rc;
  return sim->u_e.alloc(kTraceWidth);
}

template <typename R>
static int unfused_load(mythos_sim* sim, const R* c, const R* q, const R* p, const R* l, hipStream_t st) {
  if (int rc = unfused_alloc<R>(sim)) return rc;
  const size_t n = (size_t)sim->sys->n;
  MYTHOS_HIP_TRY(hipMemcpyAsync(sim->u_c.get(), c, 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(sim->u_q.get(), q, 4 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(sim->u_p.get(), p, 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(sim->u_l.get(), l, 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  sim->resident = true;
  sim->list_valid = false;
  sim->since_build = 0;
  sim->u_forces_valid = false;
  return 0;
}

template <typename R>
static int unfused_store(mythos_sim* sim, R* c, R* q, R* p, R* l, hipStream_t st) {
  const size_t n = (size_t)sim->sys->n;
  MYTHOS_HIP_TRY(hipMemcpyAsync(c, sim->u_c.get(), 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(q, sim->u_q.get(), 4 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(p, sim->u_p.get(), 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  MYTHOS_HIP_TRY(hipMemcpyAsync(l, sim->u_l.get(), 3 * n * sizeof(R), hipMemcpyDeviceToDevice, st));
  return 0;
}

template <typename R>
static int unfused_advance(mythos_sim* sim, int n_steps, int save_every, R* traj_c, R* traj_q, double* e_trace, hipStream_t st) {
  mythos_system* sys = sim->sys;
  const int n = sys->n, tb = (n + 255) / 256;
  const LangevinConst<R> K = make_const<R>(sim);
  R *c = (R*)sim->u_c.get(), *q = (R*)sim->u_q.get(), *p = (R*)sim->u_p.get(), *l = (R*)sim->u_l.get(), *gc = (R*)sim->u_gc.get(), *gq = (R*)sim->u_gq.get();
  R* ref = (R*)sim->u_ref.get();
  const bool dynamic = sim->rebuild_every > 0;
  sim->last_recoveries = 0;
  // the sum of the offset coefficients of the farthest site, over both geometries (bounds a site's motion under rotation)
  double reach = 0.0;
  for (int k = 0; k < 2; ++k) {
    const double* P = sys->pd_sets.data() + (size_t)k * OXP_COUNT;
    reach = std::max({reach, std::fabs(P[GEO_BACK_A1]) + std::fabs(P[GEO_BACK_A2]), std::fabs(P[GEO_BASE]), std::fabs(P[GEO_STACK]),
                      std::fabs(P[GEO_STACK3_A1]) + std::fabs(P[GEO_STACK3_A2]), std::fabs(P[GEO_STACK5_A1]) + std::fabs(P[GEO_STACK5_A2])});
  }
  auto build = [&]() -> int {
    if (int rc = rows_build_until_fit(sys, c, false, sim->r_cut, sim->skin, nullptr, nullptr, false, true, st)) return rc;
    hipLaunchKernelGGL(unfused_ref_kernel<R>, dim3(tb), dim3(256), 0, st, n, (const R*)c, (const R*)q, ref);
    sim->since_build = 0;
    sim->list_valid = true;
    sim->list_epoch = ++sys->list_epoch;
    return 0;
  };
  auto forces = [&]() -> int {
    return oxdna_energy_launch(sys, c, q, 1, sim->u_e.get(), gc, gq, nullptr, nullptr, nullptr, st);
  };
  auto check_flags = [&](const char* when) -> int {
    int fl[2] = {0, 0};
    MYTHOS_HIP_TRY(hipMemcpyAsync(fl, sim->d_flags.get(), sizeof(fl), hipMemcpyDeviceToHost, st));
    MYTHOS_HIP_TRY(hipStreamSynchronize(st));
    MYTHOS_HIP_TRY(hipMemsetAsync(sim->d_flags.get(), 0, 2 * sizeof(int), st));
    if (fl[0] & 2) {
      sim->resident = false;
      set_error(std::string("mythos_langevin_run (oxNA, unfused): NaN in the state ") + when);
      return MYTHOS_ERR_NUMERIC;
    }
    if (fl[1] != 0) {
      sim->resident = false;
      set_error("mythos_langevin_run (oxNA, unfused): a site moved more than skin / 2 between two list rebuilds; shorten "
                "rebuild_every or widen the skin (this path does not halt and resume)");
      return MYTHOS_ERR_OVERFLOW;
    }
    return 0;
  };
  MYTHOS_HIP_TRY(hipMemsetAsync(sim->d_flags.get(), 0, mythos_sim::kCtlWords * sizeof(int), st));
  if (!sim->list_valid) sim->u_forces_valid = false;  // parameters or rows were replaced since the last force evaluation
  if (dynamic && !sim->list_valid)
    if (int rc = build()) return rc;
  if (!sim->u_forces_valid) {
    if (int rc = forces()) return rc;
    sim->u_forces_valid = true;
  }
  int saved = 0;
  for (int k = 0; k <= n_steps; ++k) {
    // launch k: close the kick of step k - 1 (the forces at x_k are in gc / gq), record x_k, then step k -> k + 1
    const bool do_step = k < n_steps;
    const bool save = save_every > 0 && k > 0 && k % save_every == 0;
    if (k == 0 && !do_step) break;  // zero steps: nothing to close
    R* tc = (save && traj_c) ? traj_c + (size_t)saved * n * 3 : nullptr;
    R* tq = (save && traj_q) ? traj_q + (size_t)saved * n * 4 : nullptr;
    double* ke = save ? sim->u_e.get() + T_COUNT : nullptr;
    if (save) MYTHOS_HIP_TRY(hipMemsetAsync(sim->u_e.get() + T_COUNT, 0, 2 * sizeof(double), st));
    hipLaunchKernelGGL(unfused_integrate_kernel<R>, dim3(tb), dim3(256), 0, st, n, K, c, q, p, l, (const R*)gc, (const R*)gq,
                       R(k > 0 ? 0.5 : 0.0), do_step ? 1 : 0, sim->seed, (uint64_t)(sim->step + k), dynamic ? (const R*)ref : nullptr,
                       R(reach), sim->d_flags.get(), tc, tq, ke);
    if (save) {
      if (e_trace) hipLaunchKernelGGL(unfused_trace_kernel, dim3(1), dim3(64), 0, st, (const double*)sim->u_e.get(), e_trace + (size_t)saved * kTraceWidth);
      ++saved;
    }
    if (!do_step) break;
    ++sim->since_build;
    if (dynamic && sim->since_build >= sim->rebuild_every) {
      if (int rc = check_flags("before a list rebuild")) return rc;
      if (int rc = build()) return rc;
    }
    if (int rc = forces()) return rc;
  }
  MYTHOS_HIP_TRY(hipGetLastError());
  if (int rc = check_flags("at the end of the run")) return rc;
  sim->step += n_steps;
  return 0;
}

}  // namespace mythos


// ---- per-precision entry points of the integrator: mythos_md_*<R> is defined (explicitly instantiated) in the translation
//      unit of its precision and only declared in the other
template <typename R>
int mythos_md_load(mythos_sim* s, void* c, void* q, void* p, void* l, hipStream_t st);
template <typename R>
int mythos_md_advance(mythos_sim* s, int n_steps, int save_every, bool close, void* tc, void* tq, double* e_trace, hipStream_t st);
template <typename R>
int mythos_md_store(mythos_sim* s, void* c, void* q, void* p, void* l, hipStream_t st);
template <typename R>
int mythos_md_init_momenta(mythos_sim* s, void* p_lin, void* p_ang, hipStream_t st);

#define MYTHOS_MD_DEFINE_PRECISION(R)                                                                                        \
  template <>                                                                                                                 \
  int mythos_md_load<R>(mythos_sim * s, void* c, void* q, void* p, void* l, hipStream_t st) {                                  \
    mythos_system* sys = s->sys;                                                                                              \
    if (s->unfused) return mythos::unfused_load<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);                                        \
    return sys->model == 1   ? mythos::load_typed<R, 1>(s, (R*)c, (R*)q, (R*)p, (R*)l, st)                                   \
           : sys->model == 2 ? mythos::load_typed<R, 2>(s, (R*)c, (R*)q, (R*)p, (R*)l, st)                                   \
           : sys->model == 3 ? mythos::load_typed<R, 3>(s, (R*)c, (R*)q, (R*)p, (R*)l, st)                                   \
                             : mythos::load_typed<R, 4>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);                                  \
  }                                                                                                                           \
  template <>                                                                                                                 \
  int mythos_md_advance<R>(mythos_sim * s, int n_steps, int save_every, bool close, void* tc, void* tq, double* e_trace,      \
                           hipStream_t st) {                                                                                  \
    mythos_system* sys = s->sys;                                                                                              \
    if (s->unfused) return mythos::unfused_advance<R>(s, n_steps, save_every, (R*)tc, (R*)tq, e_trace, st);                   \
    return sys->model == 1   ? mythos::advance_typed<R, 1>(s, n_steps, save_every, close, (R*)tc, (R*)tq, e_trace, st)        \
           : sys->model == 2 ? mythos::advance_typed<R, 2>(s, n_steps, save_every, close, (R*)tc, (R*)tq, e_trace, st)        \
           : sys->model == 3 ? mythos::advance_typed<R, 3>(s, n_steps, save_every, close, (R*)tc, (R*)tq, e_trace, st)        \
                             : mythos::advance_typed<R, 4>(s, n_steps, save_every, close, (R*)tc, (R*)tq, e_trace, st);       \
  }                                                                                                                           \
  template <>                                                                                                                 \
  int mythos_md_store<R>(mythos_sim * s, void* c, void* q, void* p, void* l, hipStream_t st) {                                 \
    if (s->unfused) return mythos::unfused_store<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);                                       \
    /* an open frame (mythos_langevin_advance) gets its closing half kick first; should that fail, the open state goes */     \
    /* back all the same, with the error                                                                              */     \
    const int rc = s->open ? mythos_md_advance<R>(s, 0, 0, true, nullptr, nullptr, nullptr, st) : MYTHOS_OK;                   \
    const int ru = mythos::unpack_typed<R>(s, (R*)c, (R*)q, (R*)p, (R*)l, st);                                                \
    return rc ? rc : ru;                                                                                                      \
  }                                                                                                                           \
  template <>                                                                                                                 \
  int mythos_md_init_momenta<R>(mythos_sim * s, void* p_lin, void* p_ang, hipStream_t st) {                                    \
    const double sd_t = std::sqrt(s->mass * s->kT);                                                                           \
    double sd_r[3];                                                                                                           \
    for (int k = 0; k < 3; ++k) sd_r[k] = std::sqrt(s->inertia[k] * s->kT);                                                   \
    hipLaunchKernelGGL(mythos::init_momenta_kernel<R>, dim3(1), dim3(256), 0, st, s->sys->n, R(sd_t), R(sd_r[0]), R(sd_r[1]), \
                       R(sd_r[2]), s->seed, (R*)p_lin, (R*)p_ang);                                                            \
    MYTHOS_HIP_TRY(hipGetLastError());                                                                                        \
    return MYTHOS_OK;                                                                                                         \
  }
