// Energy kernel, translation unit 2 of 2: the fp64 instantiations of oxdna_energy_core.inc (the reference's precision,
// and the one its DiffTRe gradients are validated in).  Compiled without machine LICM (Makefile: ENERGY_F64_FLAGS),
// which the fp32 unit keeps.
#include "oxdna_energy_core.inc"

namespace mythos {

int oxdna_energy_launch_f64(mythos_system* sys, const void* center, const void* quat, int n_frames, double* e_terms, void* dU_dcenter,
                            void* dU_dquat, double* dU_dparams, mythos_obs* oset, double* obs_out, hipStream_t stream) {
  return oxdna_energy_launch_typed<double>(sys, center, quat, n_frames, e_terms, dU_dcenter, dU_dquat, dU_dparams, oset, obs_out, stream);
}

}  // namespace mythos
