// Pressure and pressure coupling of the MARTINI integrator; included by martini_md.hip behind mm_store_typed.
//
// The reference runs its MARTINI dynamics in GROMACS with semi-isotropic coupling (data/templates/martini/m2/DMPC/273K/
// md.mdp: pcoupltype = semiisotropic, compressibility = 3e-4 0.0, ref-p = 1.0 1.0); this is the device-resident
// counterpart: the diagonal pressure of the resident state and a first-order cell-rescaling barostat, deterministic
// (Berendsen) or with the noise term of stochastic cell rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107, 2020).
//
//   K_d = sum_i m_i v_id^2,   W_d = -sum_terms r_d dU/dr_d over relative (minimum-image) vectors = -dU/dln s_d under
//   x -> s o x, box -> s o box,   P_d = (K_d + W_d) / V x 16.6053907 bar  (kJ/mol/nm^3 -> bar)
//
// A coupling event at the closed state (x_s, v_s) of every absolute step s > 0 with s % every == 0, with
// f_d = beta_d every dt / tau_p, kT' = 16.6053907 kT and xi = normals6(seed, particle 0, step s, stream 2)[0, 1]:
//   isotropic       ln mu   = [-f (P0 - P) + sqrt(2 kT' f / V) xi0] / 3,                 P = (Px + Py + Pz) / 3
//   semi-isotropic  ln mu_xy = -f_xy (P0_xy - P_xy) / 3 + sqrt(kT' f_xy / (3 V)) xi0,    P_xy = (Px + Py) / 2
//                   ln mu_z  = -f_z (P0_z - P_z) / 3 + sqrt(2 kT' f_z / (3 V)) xi1
//   c-rescale: x <- mu o x, box <- mu o box, v <- v / mu.   Berendsen: no noise terms, velocities untouched.
// mu = exp(ln mu): GROMACS' Berendsen scales by the linear 1 - f (P0 - P) / 3, which differs from this at O(f^2).
//
// The pressure kernel reads a CLOSED frame (velocities after the closing half kick) and writes nothing but its partials:
// the chunk in front of an event ends on the step kernel's closing launch (md_drive, close = true).  The loop that cuts an
// advance at the events is mm_advance_chunked (martini_md.hip), one for coupling and both exchanges; the row logs it keeps
// are mm_clear_logs / mm_push_row below.

namespace mythos {

// (kBarPerKjMolNm3: martini_internal.h)
constexpr int kMmVir = 6;    // Kx Ky Kz Wx Wy Wz
constexpr int kNptRec = 20;  // box[3] mu[3] P[3] K[3] W[3] V ok
enum { kRecBox = 0, kRecMu = 3, kRecP = 6, kRecK = 9, kRecW = 12, kRecV = 15, kRecOk = 16 };

// The step kernel's decomposition (16 lanes per bead over its Verlet row, then its bond and angle incidence slots, DPP
// fold) with the strain derivative in place of the force: an LJ pair or a bond gives -1/2 g dx_d^2 to either bead, an
// angle -u_d dU/dx_id at its first and -v_d dU/dx_kd at its last bead.  Sums in R inside a lane, in double across groups.
// COUL (the system holds charges; the record behind eps, martini_md.hip): the reaction-field pair term on the row walk and the excluded-pair term on the bond
// slots that carry it, both central: -1/2 (dV/dr) / r dx_d^2 to either bead, as LJ and bonds.
// ENS (the replica table behind the Coulomb record, martini_md.hip): n beads per replica, blocks_per_rep workgroups each,
// pointers moved to the workgroup's replica; partials stay in workgroup order, so replica-major.
template <typename R, bool COUL, bool ENS = false>
__global__ __launch_bounds__(kMmBlock, 1024 / kMmBlock) void martini_pressure_kernel(
    int n, const MmConst<R> K0, const typename Real4<R>::type* __restrict__ in, const typename Real4<R>::type* __restrict__ vel,
    const int* __restrict__ rows, const int* __restrict__ row_len, int row_stride, const R* __restrict__ sigma,
    const R* __restrict__ eps, const int* __restrict__ bead_bonds, const int* __restrict__ bead_angles,
    const R* __restrict__ bond_k, const R* __restrict__ bond_r0, const R* __restrict__ angle_k, const R* __restrict__ angle_t0,
    const int* __restrict__ bb_partner, const int2* __restrict__ ba_partner, double* __restrict__ part) {
  using V4 = typename Real4<R>::type;
  constexpr int G = kMmG, PPB = kMmPPB;
  extern __shared__ unsigned char smem_raw[];
  MmConst<R> K = K0;
  R* s_sig2 = reinterpret_cast<R*>(smem_raw);
  R* s_eps = s_sig2 + K.n_types * K.n_types;
  R* s_c = s_eps + K.n_types * K.n_types;  // (COUL) the Coulomb record
  (void)s_c;
  __shared__ double s_p[PPB][kMmVir];

  const int bid = (int)blockIdx.x;  // (the grid is exactly the workgroups that hold beads)
  int lb = bid;
  if constexpr (ENS) {
    const int bpr = (n + PPB - 1) / PPB;
    const int rep = bid / bpr;
    int n_rep;
    lb = bid - rep * bpr;
    mm_rep_apply(K, mm_rep_record<R>(eps, K.n_types * K.n_types, rep, n_rep));
    const size_t b0 = (size_t)rep * n;
    in += b0, vel += b0, rows += b0 * row_stride, row_len += b0;
  }
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int i = lb * PPB + grp;
  const bool valid = i < n;
  const int ii = valid ? i : n - 1;
  const int tt = K.n_types * K.n_types;
  for (int k = threadIdx.x; k < tt; k += kMmBlock) {
    s_sig2[k] = sigma[k];
    s_eps[k] = eps[k];
  }
  if constexpr (COUL)
    if (threadIdx.x < kCoulRec) s_c[threadIdx.x] = eps[tt + threadIdx.x];
  const V4 me = in[ii];
  const int type_i = (COUL ? ((int)me.w & (kMaxTypes - 1)) : (int)me.w) * K.n_types;
  const int* __restrict__ row = rows + (size_t)ii * row_stride;
  const int len = valid ? row_len[ii] : 0;
  __syncthreads();

  R wx = 0, wy = 0, wz = 0;
  R qi = 0, k_rf = 0, c_rf = 0;
  const R* s_q = s_c + kCoulQ;
  (void)qi, (void)k_rf, (void)c_rf, (void)s_q;
  if constexpr (COUL) {
    qi = valid ? s_c[kCoulPref] * s_q[(int)me.w >> 6] : R(0);
    k_rf = s_c[kCoulKrf], c_rf = s_c[kCoulCrf];
  }
  {
    constexpr int kB = MYTHOS_MM_BATCH;
#pragma unroll 1
    for (int s0 = 0; s0 < len; s0 += kB * G) {
      int j[kB];
      V4 o[kB];
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const int idx = s0 + u * G + lane;
        j[u] = (idx < len) ? row[idx] : -1;
      }
#pragma unroll
      for (int u = 0; u < kB; ++u) o[u] = in[j[u] >= 0 ? j[u] : ii];
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const R dx = wrap_fma(me.x - o[u].x, K.lx, K.ilx), dy = wrap_fma(me.y - o[u].y, K.ly, K.ily), dz = wrap_fma(me.z - o[u].z, K.lz, K.ilz);
        const R r2 = m_fma(dz, dz, m_fma(dy, dy, dx * dx));
        if (j[u] >= 0 && r2 < K.rc2) {
          const int tp = type_i + (COUL ? ((int)o[u].w & (kMaxTypes - 1)) : (int)o[u].w);
          const R h = R(-0.5) * lj_pair(s_sig2[tp], s_eps[tp], r2).g;
          wx += h * dx * dx, wy += h * dy * dy, wz += h * dz * dz;
          if constexpr (COUL) {
            if (qi != R(0)) {
              const R hc = R(-0.5) * qi * s_q[(int)o[u].w >> 6] * rf_pair(r2, k_rf, c_rf).g;
              wx += hc * dx * dx, wy += hc * dy * dy, wz += hc * dz * dz;
            }
          }
        }
      }
    }
  }
  // (COUL) a bond slot that repeats the partner of a lower slot carries no excluded-pair term (see the step kernel)
  bool coul_dup = false;
  (void)coul_dup;
  if constexpr (COUL) {
    const int par = (valid && lane < kMaxBeadBonds) ? bb_partner[(size_t)i * kMaxBeadBonds + lane] : -1;
#pragma unroll
    for (int t = 0; t < kMaxBeadBonds - 1; ++t) {
      const int pt = __shfl(par, t, G);
      coul_dup = coul_dup || (t < lane && pt == par);
    }
  }
  if (valid) {
    for (int s = lane; s < kMaxBeadBonds; s += G) {
      const int ent = bead_bonds[(size_t)i * kMaxBeadBonds + s];
      if (ent < 0) continue;
      const int b = ent >> 1;
      const V4 o = in[bb_partner[(size_t)i * kMaxBeadBonds + s]];
      const R dx = wrap(me.x - o.x, K.lx, K.ilx), dy = wrap(me.y - o.y, K.ly, K.ily), dz = wrap(me.z - o.z, K.lz, K.ilz);
      const R h = R(-0.5) * bond_term(dx * dx + dy * dy + dz * dz, bond_k[b], bond_r0[b]).c;
      wx += h * dx * dx, wy += h * dy * dy, wz += h * dz * dz;
      if constexpr (COUL) {
        const R r2 = dx * dx + dy * dy + dz * dz;
        if (qi != R(0) && !coul_dup && r2 < K.rc2) {
          const R hc = R(-0.5) * qi * s_q[(int)o.w >> 6] * rf_excluded(r2, k_rf, c_rf).g;
          wx += hc * dx * dx, wy += hc * dy * dy, wz += hc * dz * dz;
        }
      }
    }
    for (int s = lane; s < kMaxBeadAngles; s += G) {
      const int ent = bead_angles[(size_t)i * kMaxBeadAngles + s];
      if (ent < 0) continue;
      const int a = ent >> 2, role = ent & 3;  // 0: first bead, 1: centre, 2: last bead
      if (role == 1) continue;                 // (the centre's arms are counted at their far ends)
      const int2 others = ba_partner[(size_t)i * kMaxBeadAngles + s];
      const V4 q0 = in[others.x], q1 = in[others.y];
      const V4 pi = role == 0 ? me : q0, pj = role == 0 ? q0 : q1, pk = role == 2 ? me : q1;
      const R u[3] = {wrap(pi.x - pj.x, K.lx, K.ilx), wrap(pi.y - pj.y, K.ly, K.ily), wrap(pi.z - pj.z, K.lz, K.ilz)};
      const R v[3] = {wrap(pk.x - pj.x, K.lx, K.ilx), wrap(pk.y - pj.y, K.ly, K.ily), wrap(pk.z - pj.z, K.lz, K.ilz)};
      const R u2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      const R uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
      const AngleGeom<R> ag = angle_geometry(u, v, u2, v2, uv, K.angle_kind);
      const R h = -angle_term(K.angle_kind, ag, angle_k[a], angle_t0[a]).dEdc;
      // (times this bead's own arm)
      wx += h * angle_role_grad(role, ag, u[0], v[0]) * (role == 0 ? u[0] : v[0]);
      wy += h * angle_role_grad(role, ag, u[1], v[1]) * (role == 0 ? u[1] : v[1]);
      wz += h * angle_role_grad(role, ag, u[2], v[2]) * (role == 0 ? u[2] : v[2]);
    }
  }
  wx = group_sum<G>(wx);
  wy = group_sum<G>(wy);
  wz = group_sum<G>(wz);
  if (lane == 0) {
    double kx = 0.0, ky = 0.0, kz = 0.0;
    if (valid) {
      const V4 vv = vel[i];
      const double m = 1.0 / double(vv.w);  // (.w: the inverse mass)
      kx = m * double(vv.x) * double(vv.x), ky = m * double(vv.y) * double(vv.y), kz = m * double(vv.z) * double(vv.z);
    }
    s_p[grp][0] = kx, s_p[grp][1] = ky, s_p[grp][2] = kz;
    s_p[grp][3] = valid ? double(wx) : 0.0, s_p[grp][4] = valid ? double(wy) : 0.0, s_p[grp][5] = valid ? double(wz) : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kMmVir) {
    double s = 0.0;
    for (int g = 0; g < PPB; ++g) s += s_p[g][threadIdx.x];
    part[(size_t)bid * kMmVir + threadIdx.x] = s;
  }
}

struct MmBaroArgs {
  double box[3];
  double ref_p[2], f[2];  // bar; beta every dt / tau_p per bar ([0]: all axes or xy, [1]: z)
  double kTp;             // 16.6053907 kT: bar nm^3
  double min_edge;        // 2 (r_cut + skin)
  uint64_t seed, step;
  int kind, coupling;     // kind 0: pressure only, mu = 1
};

// The partials summed as reduce_trace_kernel sums them (16 columns x 16 groups, fixed order), then one thread in double:
// P, mu and the new box, to the device record (for mm_scale_kernel) and to pinned host memory (for the host, behind its
// one synchronisation per event) - the publish_ctl_kernel pattern.  rec[kRecOk] = 0: the new box would be too small for
// the minimum image, or is not finite; nothing is scaled then.
static __global__ __launch_bounds__(256) void mm_barostat_kernel(const double* __restrict__ part, int n_blocks, const MmBaroArgs a,
                                                                 double* __restrict__ rec, double* __restrict__ host_rec) {
  __shared__ double acc[16][17];
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  double s = 0.0;
  if (k < kMmVir)
    for (int b = g; b < n_blocks; b += 16) s += part[(size_t)b * kMmVir + k];
  acc[g][k] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[kMmVir];
  for (int c = 0; c < kMmVir; ++c) {
    t[c] = 0.0;
    for (int j = 0; j < 16; ++j) t[c] += acc[j][c];
  }
  const double V = a.box[0] * a.box[1] * a.box[2];
  double P[3], ln_mu[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < 3; ++d) P[d] = (t[d] + t[3 + d]) / V * kBarPerKjMolNm3;
  if (a.kind != 0) {
    double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.kind == 2) normals6(a.seed, 0u, a.step, 2u, z);  // (the thermostat draws from streams 0 and 1)
    if (a.coupling == 0) {
      const double p = (P[0] + P[1] + P[2]) / 3.0;
      const double l = (-a.f[0] * (a.ref_p[0] - p) + sqrt(2.0 * a.kTp * a.f[0] / V) * z[0]) / 3.0;
      ln_mu[0] = ln_mu[1] = ln_mu[2] = l;
    } else {
      const double pxy = 0.5 * (P[0] + P[1]);
      ln_mu[0] = ln_mu[1] = -a.f[0] * (a.ref_p[0] - pxy) / 3.0 + sqrt(a.kTp * a.f[0] / (3.0 * V)) * z[0];
      ln_mu[2] = -a.f[1] * (a.ref_p[1] - P[2]) / 3.0 + sqrt(2.0 * a.kTp * a.f[1] / (3.0 * V)) * z[1];
    }
  }
  double out[kNptRec];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double mu = ln_mu[d] == 0.0 ? 1.0 : exp(ln_mu[d]), edge = a.box[d] * mu;
    ok = ok && (edge >= a.min_edge) && (edge < 1e300);  // (false for a NaN too)
    out[kRecBox + d] = edge, out[kRecMu + d] = mu, out[kRecP + d] = P[d], out[kRecK + d] = t[d], out[kRecW + d] = t[3 + d];
  }
  out[kRecV] = V, out[kRecOk] = ok ? 1.0 : 0.0;
#pragma unroll
  for (int c = kRecOk + 1; c < kNptRec; ++c) out[c] = 0.0;
#pragma unroll
  for (int c = 0; c < kNptRec; ++c) rec[c] = out[c], host_rec[c] = out[c];
}

// Ensemble: bead i of replica i / n by that replica's mu; an event at which ANY replica's new box fails scales nobody
// (the call ends there with every replica at the state of that step)
template <typename R>
__global__ void mm_scale_ens_kernel(int n, int n_rep, const double* __restrict__ rec, int scale_vel,
                                    typename Real4<R>::type* __restrict__ frame, typename Real4<R>::type* __restrict__ vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_rep) return;
  for (int r = 0; r < n_rep; ++r)
    if (rec[(size_t)r * kNptRec + kRecOk] == 0.0) return;
  const double* mu = rec + (size_t)(i / n) * kNptRec + kRecMu;
  auto x = frame[i];
  x.x *= R(mu[0]), x.y *= R(mu[1]), x.z *= R(mu[2]);
  frame[i] = x;
  if (scale_vel) {
    auto v = vel[i];
    v.x *= R(1.0 / mu[0]), v.y *= R(1.0 / mu[1]), v.z *= R(1.0 / mu[2]);
    vel[i] = v;
  }
}

template <typename R>
__global__ void mm_scale_kernel(int n, const double* __restrict__ rec, int scale_vel, typename Real4<R>::type* __restrict__ frame,
                                typename Real4<R>::type* __restrict__ vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || rec[kRecOk] == 0.0) return;
  auto x = frame[i];
  x.x *= R(rec[kRecMu]), x.y *= R(rec[kRecMu + 1]), x.z *= R(rec[kRecMu + 2]);
  frame[i] = x;
  if (scale_vel) {
    auto v = vel[i];
    v.x *= R(1.0 / rec[kRecMu]), v.y *= R(1.0 / rec[kRecMu + 1]), v.z *= R(1.0 / rec[kRecMu + 2]);
    vel[i] = v;
  }
}

static bool mm_barostat_on(const mythos_martini_sim* sim) {
  const MmBarostat& b = sim->baro;
  return b.kind != 0 && (b.beta[0] > 0 || (b.coupling == 1 && b.beta[1] > 0));
}

// The row logs of an advance - last_boxes, and for an ensemble handle the rows of ladder and windows - are kept here and
// nowhere else: cleared, with both attempt logs, at the head of every advance, and pushed together at the moment a row is
// saved, so all three always hold the same number of rows.
static void mm_clear_logs(mythos_martini_sim* sim) {
  sim->baro.last_boxes.clear();
  for (MmPairExchange* x : {&sim->xchg, &sim->wx}) x->last_rows.clear(), x->last_log.clear();
}
static void mm_push_row(mythos_martini_sim* sim) {
  const double* b = sim->box_of(0);  // (an ensemble's are contiguous)
  sim->baro.last_boxes.insert(sim->baro.last_boxes.end(), b, b + 3 * (size_t)sim->copies());
  if (sim->n_rep == 0) return;  // a single copy has neither ladder nor windows
  for (MmPairExchange* x : {&sim->xchg, &sim->wx}) x->last_rows.insert(x->last_rows.end(), x->of_slot.begin(), x->of_slot.end());
}

static int mm_npt_buffers(mythos_martini_sim* sim) {
  MmBarostat& b = sim->baro;
  const int blocks = sim->copies() * ((sim->sys->n + kMmPPB - 1) / kMmPPB);
  if (int rc = b.d_part.grow((size_t)blocks * kMmVir)) return rc;
  if (int rc = b.d_rec.grow((size_t)sim->copies() * kNptRec)) return rc;
  return b.rec.grow((size_t)sim->copies() * kNptRec);  // (the number of copies is fixed at create)
}

// Pressure of the resident frame - closed, with rows built for it - into the records; with `event` the coupling
// on top: mu on the device, frame and velocities scaled, then the ONE synchronisation, after which the host takes the new box
// and drops the list (the next launch rebuilds it, which resets ref_pos).
template <typename R>
static int mm_pressure_typed(mythos_martini_sim* sim, bool event, hipStream_t st) {
  using V4 = typename Real4<R>::type;
  mythos_martini* m = sim->sys;
  MmBarostat& b = sim->baro;
  if (int rc = mm_npt_buffers(sim)) return rc;
  const bool ens = sim->n_rep > 0;
  const int n = m->n, blocks_per_rep = (n + kMmPPB - 1) / kMmPPB, blocks = sim->copies() * blocks_per_rep;
  const MmConst<R> K = mm_const<R>(sim, sim->box_of(0));
  const size_t lds = ((size_t)2 * sim->n_ctypes * sim->n_ctypes + (sim->coul ? kCoulRec : 0)) * sizeof(R);
  V4* frame = (V4*)sim->frame[sim->cur].get();
#define MM_P_ARGS                                                                                                          \
  n, K, (const V4*)frame, (const V4*)sim->vel.get(), sim->list.d_rows.get(), sim->d_row_len.get(), sim->list.stride,        \
      (const R*)sim->d_csig2.get(), (const R*)sim->d_ceps.get(), m->d_bead_bonds.get(), m->d_bead_angles.get(),             \
      (const R*)m->d_bond_k.get(), (const R*)m->d_bond_r0.get(), (const R*)m->d_angle_k.get(),                              \
      (const R*)sim->d_angle_ref.get(), sim->d_bb_partner.get(), sim->d_ba_partner.get(), b.d_part.get()
  if (ens && sim->coul)
    hipLaunchKernelGGL((martini_pressure_kernel<R, true, true>), dim3(blocks), dim3(kMmBlock), lds, st, MM_P_ARGS);
  else if (ens)
    hipLaunchKernelGGL((martini_pressure_kernel<R, false, true>), dim3(blocks), dim3(kMmBlock), lds, st, MM_P_ARGS);
  else if (sim->coul)
    hipLaunchKernelGGL((martini_pressure_kernel<R, true>), dim3(blocks), dim3(kMmBlock), lds, st, MM_P_ARGS);
  else
    hipLaunchKernelGGL((martini_pressure_kernel<R, false>), dim3(blocks), dim3(kMmBlock), lds, st, MM_P_ARGS);
#undef MM_P_ARGS
  MmBaroArgs a;
  for (int d = 0; d < 3; ++d) a.box[d] = sim->box_of(0)[d];  // (an ensemble: box, kTp and seed per replica, below)
  for (int d = 0; d < 2; ++d) a.ref_p[d] = b.ref_p[d], a.f[d] = b.beta[d] * b.every * sim->dt / b.tau_p;
  a.kTp = kBarPerKjMolNm3 * sim->kT;
  a.min_edge = 2.0 * (m->r_cut + sim->skin);
  a.seed = sim->seed, a.step = (uint64_t)sim->step;
  a.kind = event ? b.kind : 0, a.coupling = b.coupling;
  if (ens) {
    // One launch of the single copy's kernel per replica, over that replica's partials, with its box, kT' and seed: the
    // record is the single integrator's by construction, and so is the kernel's code (a second kernel around the same
    // body changed the inlining of the first).  R tiny launches per event, next to the 3 R of the list build behind it.
    for (int r = 0; r < sim->n_rep; ++r) {
      for (int d = 0; d < 3; ++d) a.box[d] = sim->box_of(r)[d];
      a.kTp = kBarPerKjMolNm3 * sim->rep_kT[r], a.seed = sim->rep_seed[r];
      hipLaunchKernelGGL(mm_barostat_kernel, dim3(1), dim3(256), 0, st, (const double*)b.d_part.get() + (size_t)r * blocks_per_rep * kMmVir,
                         blocks_per_rep, a, b.d_rec.get() + (size_t)r * kNptRec, b.rec.dev() + (size_t)r * kNptRec);
    }
    if (event)
      hipLaunchKernelGGL(mm_scale_ens_kernel<R>, dim3((sim->n_all() + 255) / 256), dim3(256), 0, st, n, sim->n_rep, (const double*)b.d_rec.get(),
                         b.kind == 2 ? 1 : 0, frame, (V4*)sim->vel.get());
  } else {
    hipLaunchKernelGGL(mm_barostat_kernel, dim3(1), dim3(256), 0, st, (const double*)b.d_part.get(), blocks, a, b.d_rec.get(), b.rec.dev());
    if (event)
      hipLaunchKernelGGL(mm_scale_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, st, n, (const double*)b.d_rec.get(), b.kind == 2 ? 1 : 0, frame,
                         (V4*)sim->vel.get());
  }
  MYTHOS_HIP_TRY(hipGetLastError());
  MYTHOS_HIP_TRY(hipStreamSynchronize(st));
  if (!event) return MYTHOS_OK;
  const double* h_rec = b.rec.host();
  if (ens) {  // R boxes behind the one synchronisation; the replica tables follow them, queued in front of the next launch
    for (int r = 0; r < sim->n_rep; ++r) {
      const double* h = h_rec + (size_t)r * kNptRec;
      if (h[kRecOk] == 0.0) {
        set_error("mythos_martini_langevin_run: the pressure coupling at step " + std::to_string(sim->step) + " would make the box of replica " +
                  std::to_string(r) + " smaller than twice (r_cut + skin), or not finite - edges " + std::to_string(h[kRecBox]) + ", " +
                  std::to_string(h[kRecBox + 1]) + ", " + std::to_string(h[kRecBox + 2]) +
                  ": minimum image breaks down (the state of that step stays resident, no replica scaled)");
        return MYTHOS_ERR_INVALID_ARGUMENT;
      }
    }
    for (int r = 0; r < sim->n_rep; ++r)
      for (int d = 0; d < 3; ++d) sim->rep_box[3 * (size_t)r + d] = h_rec[(size_t)r * kNptRec + kRecBox + d];
    if (int rc = mm_upload_reps(sim, st)) return rc;
    sim->list_valid = false;
    sim->since_build = 0;
    return MYTHOS_OK;
  }
  if (h_rec[kRecOk] == 0.0) {
    set_error("mythos_martini_langevin_run: the pressure coupling at step " + std::to_string(sim->step) +
              " would make the box smaller than twice (r_cut + skin), or not finite - edges " + std::to_string(h_rec[kRecBox]) + ", " +
              std::to_string(h_rec[kRecBox + 1]) + ", " + std::to_string(h_rec[kRecBox + 2]) +
              ": minimum image breaks down (the state of that step stays resident, unscaled)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  for (int d = 0; d < 3; ++d) sim->box[d] = h_rec[kRecBox + d];
  sim->list_valid = false;
  sim->since_build = 0;
  return MYTHOS_OK;
}

}  // namespace mythos

extern "C" {

/* pcoupl (kind), pcoupltype (coupling), ref-p, compressibility, tau-p, nstpcouple (every) of the reference's md.mdp */
int mythos_martini_langevin_set_barostat(mythos_martini_sim_t* s, int kind, int coupling, const double ref_p[2],
                                         const double compressibility[2], double tau_p, int every) {
  if (!s || kind < 0 || kind > 2 || (kind != 0 && (coupling < 0 || coupling > 1 || !ref_p || !compressibility))) {
    set_error("mythos_martini_langevin_set_barostat: kind 0 (off), 1 (berendsen) or 2 (c-rescale), coupling 0 (isotropic) or 1 (semiisotropic)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  MmBarostat& b = s->baro;
  if (kind == 0) {
    b.kind = 0;
    return MYTHOS_OK;
  }
  if (s->wx.every > 0)  // (martini_window_exchange_checks.h)
    return mm_wx_check_partners(false, true, "mythos_martini_langevin_set_barostat");
  if (s->rst.installed) {
    set_error("mythos_martini_langevin_set_barostat: a barostat together with restraints is refused: the restraint virial and reference "
              "scaling are not built (clear the set with mythos_martini_langevin_set_restraints first)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  const bool finite = std::isfinite(ref_p[0]) && std::isfinite(ref_p[1]) && std::isfinite(compressibility[0]) && std::isfinite(compressibility[1]);
  if (!finite || !(compressibility[0] >= 0) || !(compressibility[1] >= 0) || !(tau_p > 0) || !std::isfinite(tau_p) || every < 1) {
    set_error("mythos_martini_langevin_set_barostat: finite ref_p, compressibility >= 0, tau_p > 0 and every >= 1 required");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  b.kind = kind, b.coupling = coupling, b.tau_p = tau_p, b.every = every;
  for (int d = 0; d < 2; ++d) b.ref_p[d] = ref_p[d], b.beta[d] = compressibility[d];
  return MYTHOS_OK;
}

/* out[copies][10]: one record per replica (a single-copy handle: one) */
int mythos_martini_langevin_pressure_ensemble(mythos_martini_sim_t* s, double* out, mythos_stream_t stream) {
  if (!s || !out) {
    set_error("mythos_martini_langevin_pressure: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (!s->resident) {
    set_error("mythos_martini_langevin_pressure: no resident state");
    return MYTHOS_ERR_NOT_READY;
  }
  MYTHOS_HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  const bool f32 = s->sys->dtype == MYTHOS_F32;
  if (int rc = mm_sync_charges(s, st)) return rc;
  // an open frame gets its closing half kick, a state without rows its rows: the zero-step closing call of store
  if (s->open || !s->list_valid || !s->list_fitted)
    if (int rc = f32 ? mm_advance_typed<float>(s, 0, 0, true, nullptr, nullptr, st) : mm_advance_typed<double>(s, 0, 0, true, nullptr, nullptr, st))
      return rc;
  if (int rc = f32 ? mm_pressure_typed<float>(s, false, st) : mm_pressure_typed<double>(s, false, st)) return rc;
  for (int c = 0; c < s->copies(); ++c, out += 10) {
    const double* r = s->baro.rec.host() + (size_t)c * kNptRec;
    for (int d = 0; d < 3; ++d) out[d] = r[kRecK + d], out[3 + d] = r[kRecW + d], out[6 + d] = r[kRecP + d];
    out[9] = r[kRecV];
  }
  return MYTHOS_OK;
}

int mythos_martini_langevin_pressure(mythos_martini_sim_t* s, double out[10], mythos_stream_t stream) {
  if (s && s->n_rep > 0) {
    set_error("mythos_martini_langevin_pressure: an ensemble handle has one record per replica (mythos_martini_langevin_pressure_ensemble)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  return mythos_martini_langevin_pressure_ensemble(s, out, stream);
}

/* boxes[copies][3] */
int mythos_martini_langevin_get_box_ensemble(const mythos_martini_sim_t* s, double* boxes) {
  if (!s || !boxes) {
    set_error("mythos_martini_langevin_get_box: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  std::copy(s->box_of(0), s->box_of(0) + 3 * (size_t)s->copies(), boxes);
  return MYTHOS_OK;
}

int mythos_martini_langevin_get_box(const mythos_martini_sim_t* s, double box[3]) {
  if (s && s->n_rep > 0) {
    set_error("mythos_martini_langevin_get_box: an ensemble handle has one box per replica (mythos_martini_langevin_get_box_ensemble)");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  return mythos_martini_langevin_get_box_ensemble(s, box);
}

int mythos_martini_langevin_n_replicas(const mythos_martini_sim_t* s) { return s ? s->copies() : -1; }

int mythos_martini_langevin_last_boxes(const mythos_martini_sim_t* s, double* boxes, int* n_rows) {
  if (!s || (!boxes && !n_rows)) {
    set_error("mythos_martini_langevin_last_boxes: invalid argument");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (n_rows) *n_rows = (int)(s->baro.last_boxes.size() / (3 * (size_t)s->copies()));  // (an ensemble: rows of [n_rep][3])
  if (boxes) std::copy(s->baro.last_boxes.begin(), s->baro.last_boxes.end(), boxes);
  return MYTHOS_OK;
}

}  // extern "C"
