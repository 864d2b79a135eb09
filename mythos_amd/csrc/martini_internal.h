// Shared by martini.hip (energy path) and martini_md.hip (Langevin MD): limits, constants, the system struct.
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
  ~mythos_martini() { (void)hipSetDevice(device); }  // the members free themselves, on the system's device
};

#endif  // MYTHOS_MARTINI_INTERNAL_H
