// Shared by martini.hip (energy path), martini_md.hip (Langevin MD) and stress_profile.hip (stress profile of stored
// frames): limits, constants, the all-pairs tile sweep, the system struct.
#ifndef MYTHOS_MARTINI_INTERNAL_H
#define MYTHOS_MARTINI_INTERNAL_H

#include <algorithm>
#include <vector>

#include "martini_terms.h"
#include "mythos_internal.h"

namespace mythos {

constexpr int kLjBlock = 256;
constexpr int kMaxExcl = 8;
constexpr int kMaxBeadBonds = 8;
constexpr int kMaxBeadAngles = 12;
constexpr int kMaxTypes = 64;
// Distinct charge values of a system, 0 included (class 0).  The step kernel's frames carry type + kMaxTypes x class in
// .w and look the neighbour's charge up in a table of this size in LDS (martini_md.hip); DMPC in water uses three.
constexpr int kMaxChargeClasses = 8;
constexpr double kCoulombF = 138.935458;  // kJ mol^-1 nm e^-2 (GROMACS' ONE_4PI_EPS0)
constexpr double kBarPerKjMolNm3 = 16.6053907;  // kJ mol^-1 nm^-3 -> bar (martini_npt.inc, mythos_martini_bar_per_kj_mol_nm3)

// Reaction-field constants in the kernels' precision: pref = f / eps_r, V = pref q_i q_j (1/r + k_rf r^2 - c_rf)
template <typename R>
struct RfConst {
  R pref, k_rf, c_rf;
};

template <typename R>
struct MartiniConst {
  R rc2;
  int n_types;
  int angle_kind;  // 0 = G96 cosine, 1 = harmonic
};

// The sweep of one thread over its share of the partner tiles (tile js, js + n_js, ...): stages each tile in LDS
// (s_x: 3 kLjBlock reals and kLjBlock ints behind the caller's tables; the first barrier also publishes those), wraps,
// tests the cut-off, and calls pair(tp, j, excluded, dx, dy, dz, r2) for every partner j != i inside it - tp indexes the
// type-pair tables, excluded: j is on the bead's exclusion list (LJ drops those, reaction-field Coulomb has a term for
// them) - and tile_done() behind each tile.
template <typename R, typename Pair, typename TileDone>
__device__ __forceinline__ void lj_tile_sweep(int n, const R* __restrict__ p, const R* __restrict__ box,
                                              const int* __restrict__ types, const int* __restrict__ excl, R rc2,
                                              int n_types, int n_tiles, R* s_x, Pair pair, TileDone tile_done) {
  R *s_y = s_x + kLjBlock, *s_z = s_y + kLjBlock;
  int* s_t = reinterpret_cast<int*>(s_z + kLjBlock);
  const int js = blockIdx.y, n_js = gridDim.y;
  const int i = blockIdx.x * kLjBlock + threadIdx.x;
  const R lx = box[0], ly = box[1], lz = box[2];
  const R ilx = R(1) / lx, ily = R(1) / ly, ilz = R(1) / lz;
  R xi = 0, yi = 0, zi = 0;
  int ti = 0;
  int ex[kMaxExcl];
#pragma unroll
  for (int k = 0; k < kMaxExcl; ++k) ex[k] = -1;
  if (i < n) {
    xi = p[3 * i], yi = p[3 * i + 1], zi = p[3 * i + 2];
    ti = types[i] * n_types;
#pragma unroll
    for (int k = 0; k < kMaxExcl; ++k) ex[k] = excl[(size_t)i * kMaxExcl + k];
  }
  for (int tile = js; tile < n_tiles; tile += n_js) {
    __syncthreads();
    const int j0 = tile * kLjBlock, jl = j0 + threadIdx.x;
    if (jl < n) {
      s_x[threadIdx.x] = p[3 * jl], s_y[threadIdx.x] = p[3 * jl + 1], s_z[threadIdx.x] = p[3 * jl + 2];
      s_t[threadIdx.x] = types[jl];
    }
    __syncthreads();
    const int cnt = min(kLjBlock, n - j0);
    if (i < n) {
      for (int k = 0; k < cnt; ++k) {
        const R dx = wrap(xi - s_x[k], lx, ilx), dy = wrap(yi - s_y[k], ly, ily), dz = wrap(zi - s_z[k], lz, ilz);
        const R r2 = dx * dx + dy * dy + dz * dz;
        if (r2 < rc2) {
          const int j = j0 + k;
          bool excluded = false;
#pragma unroll
          for (int q = 0; q < kMaxExcl; ++q) excluded = excluded || (ex[q] == j);
          if (j != i) pair(ti + s_t[k], j, excluded, dx, dy, dz, r2);
        }
      }
      tile_done();
    }
  }
}

}  // namespace mythos

struct mythos_martini {
  int n = 0, n_types = 0, n_bonds = 0, n_angles = 0, angle_kind = 0, dtype = 0, device = 0;
  double r_cut = 1.1;
  mythos::DeviceBuf<int> d_types, d_excl, d_bead_bonds, d_bead_angles, d_bonds, d_angles;
  mythos::DeviceBytes d_sigma, d_eps, d_bond_k, d_bond_r0, d_angle_k, d_angle_t0;  // reals of the system's precision
  // host copies of what an integrator derives its own tables from (mythos_martini_langevin_create); the reals as the
  // caller's doubles: what the device holds is these rounded to the system's precision
  std::vector<int> h_types, h_bead_bonds, h_bead_angles, h_bonds, h_angles;
  std::vector<double> h_sigma, h_eps, h_angle_t0;
  int param_gen = 0;  // counts mythos_martini_set_params: an integrator compares it with the value its tables were derived at
  // Reaction-field Coulomb (mythos_martini_set_charges): off while no bead carries a charge.  charge_gen counts the calls
  // that changed anything: an integrator compares it with the value it last derived its own tables from.
  bool has_charge = false;
  int charge_gen = 0;
  double eps_r = 15.0, eps_rf = 0.0;
  std::vector<double> h_charge;   // [n], empty when off
  mythos::DeviceBytes d_charge;   // [n] reals
  template <typename R>
  mythos::RfConst<R> rf() const {
    const double rc3 = r_cut * r_cut * r_cut;
    const double k = eps_rf == 0.0 ? 0.5 / rc3 : (eps_rf - eps_r) / ((2.0 * eps_rf + eps_r) * rc3);
    return {R(mythos::kCoulombF / eps_r), R(k), R(1.0 / r_cut + k * r_cut * r_cut)};
  }
  mythos::DeviceBytes d_fpart;
  mythos::DeviceBuf<double> d_epart, d_ebpart, d_ljpart;  // d_ljpart: per-workgroup dU/dsigma | dU/deps tables
  // stress profile of stored frames (stress_profile.hip), allocated at its first call: per-bead virial shares of the sweep
  // [frames][n_js][n][3 or 6], of bonds and angles [frames][n][6], slab of every bead [frames][n], midpoints [frames], and
  // the centre selection of the last call with its host copy
  mythos::DeviceBuf<double> d_sp_part, d_sp_bonded, d_sp_mid;
  mythos::DeviceBuf<int> d_sp_bin, d_sp_center;
  std::vector<int> h_sp_center;
  ~mythos_martini() { (void)hipSetDevice(device); }  // the members free themselves, on the system's device
};

#endif  // MYTHOS_MARTINI_INTERNAL_H
