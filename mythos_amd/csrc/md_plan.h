// The launch plan of the oxDNA step kernel (md_step_kernel, langevin_step.h): which of its instantiations a system of n
// nucleotides on a device of `cus` compute units takes, and on what grid.  Every instantiation computes the same
// numbers, so a wrong choice here fails no parity test and only loses speed; the choice is therefore plain host
// arithmetic with no HIP in it, and the CPU suite pins its boundaries (oracle/cpu_port/selftest.cpp --md-plan).
#pragma once
#include <cstddef>

namespace mythos {

constexpr int kMdPlanBlock = 256;  // threads of a step workgroup (= kMdBlock, which langevin_core.inc asserts)

// Lanes per nucleotide (see md_step_kernel, GL): 16 where the grid of 16-lane workgroups is at most one and a half per CU
// (all resident with room to spare: n <= 6 144 on 256 CUs), 8 otherwise.  debug_lanes = 8 | 16
// (mythos_debug_set(MYTHOS_DEBUG_MD_LANES), read when a state is loaded) overrides.
inline int md_lanes_for(int n, int cus, long long debug_lanes) {
  if (debug_lanes == 8 || debug_lanes == 16) return (int)debug_lanes;
  const int grid16 = (n + 15) / 16;
  return 2 * grid16 <= 3 * cus ? 16 : 8;  // measured (r04_experiments.md): 16 lanes win to 6 k nt, lose from 10 k nt
}

struct MdPlan {
  int ppb;          // nucleotides per workgroup
  int blocks;       // workgroups that hold nucleotides
  int grid;         // ... padded to a multiple of 8 for the kernel's XCD-aware workgroup order
  bool dense_grid;  // more than four workgroups per CU: the DENSE instantiation, where it exists (fp32, 8 lanes)
  int prio_on;      // wave priority by phase (MYTHOS_MD_PRIO_MAP): off for fp64 grids that are not resident at once
};

// real_bytes = sizeof(R).  debug_dense (mythos_debug_set(MYTHOS_DEBUG_MD_DENSE), read at every advance): 1 forces the
// DENSE instantiation, 2 forbids it.
inline MdPlan md_plan_for(int n, int lanes, int cus, std::size_t real_bytes, long long debug_dense) {
  MdPlan p;
  p.ppb = kMdPlanBlock / lanes;
  p.blocks = (n + p.ppb - 1) / p.ppb;
  p.grid = 8 * ((p.blocks + 7) / 8);
  p.dense_grid = real_bytes == 4 && lanes == 8 && (debug_dense == 1 || (debug_dense != 2 && p.grid > 4 * cus));
  p.prio_on = (real_bytes == 8 && p.grid > 3 * cus) ? 0 : 1;
  return p;
}

}  // namespace mythos
