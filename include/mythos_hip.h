/*
 * mythos_hip.h  --  C ABI of libmythos_hip.so: the MI355X (gfx950) force-evaluation and
 * Langevin-integrator core for oxDNA1/2 (and MARTINI 2/3) energy functions.
 *
 * The reference (mythos-bio/mythos) has no FFI: its plugin surface is the Python protocol
 *   EnergyFunction.__call__/map/with_params        mythos/energy/base.py:24-93, 215-434
 *   JaxMDSimulator.run -> scan(step_fn)            mythos/simulators/jax_md/jaxmd.py:45-103
 *   jax.value_and_grad over the energy             mythos/optimization/objective.py:198-235
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, no torch / HIP types: streams are passed as void* (a hipStream_t, NULL = default).
 *   - stream order: an entry that takes a stream reads its device inputs and writes its device outputs in the order of
 *     THAT stream (the caller orders its inputs on it and consumes the outputs on it, or waits for it); its comment says
 *     whether the call is asynchronous or synchronises the stream.  An entry without a stream parameter that replaces
 *     or reads back device data synchronises the DEVICE first, so it is safe against launches queued on any stream,
 *     non-blocking ones included; entries that only touch host numbers say so.  INTEGRATION.md, "Streams", has the table.
 *   - "dev" pointers are device memory owned by the caller (PyTorch tensors) and only borrowed;
 *     "host" pointers are read during the call and may be freed afterwards.
 *   - dtype: 0 = float32 state/arithmetic, 1 = float64.  Energies and dU/dparams are always
 *     float64.
 *   - every function returning int returns 0 on success or a negative mythos_status; the text
 *     is available from mythos_last_error() (thread-local).
 *   - handles are independent: one handle per thread / stream.  The one piece of process-wide state is the table of
 *     test switches behind mythos_debug_set (tests only; all zero by default, never read per launch).
 *   - nucleotides are in oxDNA-classic 3'->5' memory order; quaternions are [w, x, y, z].
 */
#ifndef MYTHOS_HIP_H
#define MYTHOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mythos_system mythos_system_t;   /* one oxDNA system: topology + parameters + neighbours */
typedef struct mythos_sim mythos_sim_t;         /* Langevin integrator state bound to a system */
typedef struct mythos_martini mythos_martini_t; /* one MARTINI system */
typedef struct mythos_martini_sim mythos_martini_sim_t; /* Langevin integrator state bound to a MARTINI system */
typedef struct mythos_obs mythos_obs_t;         /* a set of per-frame structural observables (index lists on the device) */
typedef void* mythos_stream_t;                  /* hipStream_t */

enum mythos_status {
  MYTHOS_OK = 0,
  MYTHOS_ERR_INVALID_ARGUMENT = -1,
  MYTHOS_ERR_HIP = -2,
  MYTHOS_ERR_NO_DEVICE = -3,
  MYTHOS_ERR_NOT_READY = -4,   /* parameters or neighbours not set */
  MYTHOS_ERR_OVERFLOW = -5,    /* a static neighbour list too short, or more out-of-turn rebuilds in one run than a
                                  sane skin / rebuild interval produces (see mythos_langevin_last_recoveries) */
  MYTHOS_ERR_NUMERIC = -6      /* NaN / Inf detected */
};

enum mythos_dtype { MYTHOS_F32 = 0, MYTHOS_F64 = 1 };

/* number of energy terms reported per frame (dna1 leaves the Debye slot 0):
 * fene, bonded_excluded_volume, stacking, unbonded_excluded_volume, hydrogen_bonding,
 * cross_stacking, coaxial_stacking, debye  -- the order of dna2.default_energy_fns()
 * (mythos/energy/dna2/__init__.py:74-85). */
#define MYTHOS_OXDNA_N_TERMS 8

const char* mythos_version(void);
/* last error text of the calling thread ("" if none) */
const char* mythos_last_error(void);
/* number of visible HIP devices (0 if none); never initialises a context beyond the count */
int mythos_device_count(void);

/* ---- flat parameter vector ------------------------------------------------------------------
 * Replaces the per-term frozen dataclasses (*Configuration, mythos/energy/configuration.py:16-123)
 * at the kernel boundary: independent AND dependent constants, one double each, in the order
 * reported here.  The host-side shim derives the dependent ones (init_params) and applies the
 * chain rule to dU_dparams. */
int mythos_oxdna_param_count(void);
const char* mythos_oxdna_param_name(int index); /* NULL if out of range */

/* ---- system ---------------------------------------------------------------------------------
 * Replaces BaseEnergyFunction.__post_init__ topology capture (mythos/energy/base.py:133-140).
 *   model     1 = oxDNA1, 2 = oxDNA2, 3 = oxRNA2 (mythos/energy/rna2/: backbone site on a1 and a3, stacking between the
 *             3' / 5' sites with theta9 / theta10, cross-stacking without theta4, oxDNA1-form coaxial term, Debye-Hueckel)
 *             4 = oxNA, hybrid DNA / RNA systems (mythos/energy/na1/): every pair takes the parameter vector and the
 *             functional forms of its kind - DNA-DNA: oxDNA2, RNA-RNA: oxRNA2, DNA-RNA: the hybrid numbers in the oxDNA1
 *             forms - and every nucleotide the sites of its own type.  Such a system needs
 *             mythos_oxdna_set_nucleotide_types, takes 3 x mythos_oxdna_param_count() parameters (the oxDNA2, oxRNA2 and
 *             hybrid vectors one after the other; dU_dparams rows have the same layout).  No structural observables for it;
 *             a probabilistic sequence for hydrogen bonding only (mythos_oxdna_set_pseq terms = 2), with dU/d(distribution)
 *             through mythos_oxdna_energy_dpseq like the other models.  The Langevin integrator has an oxNA instantiation of its fused step kernel
 *             (two thirds of the oxDNA2 rate: a parameter set is chosen per row entry).  A probabilistic sequence and its gradient reach
 *             an oxNA system through the hydrogen-bonding term (mythos_oxdna_set_pseq, mythos_oxdna_energy_dpseq).
 *   seq       host int32[n]  bases A,C,G,T -> 0..3 (mythos/utils/constants.py:5-11)
 *   is_end    host uint8[n]  1 for strand-terminal nucleotides (Debye half charges), may be NULL
 *   bonded    host int32[n_bonded][2] rows (nn_i, nn_j) as mythos/input/topology.py:166-183
 *   box       host double[3] periodic box (jax_md.space.periodic), or NULL for free space
 */
mythos_system_t* mythos_oxdna_create(int model, int n, const int32_t* seq, const uint8_t* is_end, int n_bonded,
                                     const int32_t* bonded, const double* box, int dtype, int device);
void mythos_oxdna_destroy(mythos_system_t* sys);

/* host double[n_params] in mythos_oxdna_param_name() order (oxNA: three such vectors); replaces with_params() at the boundary.
 * Synchronises the device before the tables are replaced: a launch queued earlier, on any stream, sees the old vector whole. */
int mythos_oxdna_set_params(mythos_system_t* sys, const double* flat_params, int n_params);

/* oxNA (model 4) only: which nucleotides are RNA - the `nt_type` every na1 *Configuration carries
 * (mythos/energy/na1/fene.py:22, mythos/input/topology.py NucleotideType; is_rna_pair / is_dna_rna_pair in
 * mythos/energy/na1/utils.py:9-16).  host uint8[n], 1 = RNA, 0 = DNA.  Synchronises the device before the table is replaced. */
int mythos_oxdna_set_nucleotide_types(mythos_system_t* sys, const uint8_t* is_rna);

/* Probabilistic sequence: replaces `pseq` / `pseq_constraints` of StackingConfiguration and
 * HydrogenBondingConfiguration (mythos/energy/dna1/stacking.py:54-55, 261-287, dna1/hydrogen_bonding.py:94-95, 308-333)
 * and compute_seq_dep_weight (mythos/energy/utils.py:45-132).  The sequence-dependent weight of a pair becomes its
 * expectation; the energy entry point (energies, forces, dU/dparams incl. the 4x4 weight tables) honours it.
 *   marginals  host double[n][4]   probability of A, C, G, T per nucleotide (for a base-paired nucleotide: the marginal
 *              of its pair's type distribution)
 *   unit       host int32[n]       2 * base_pair + position_in_pair for constrained base pairs, -1 for unpaired
 *   bp_probs   host double[n_bp][4] probability of the types AT, TA, GC, CG (mythos/utils/constants.py:13) per base pair
 *   terms      bit 0: stacking, bit 1: hydrogen bonding use the expectation; 0 switches back to the discrete sequence
 * The Langevin integrator steps such a system too (since round 3): the stepping kernel has instantiations whose two
 * weight look-ups are the expectations (md_step_kernel<..., PSEQ>), as the reference's configurations carry pseq into
 * any energy function, the one a simulator steps with included (dna1/stacking.py:284-285, hydrogen_bonding.py:330-331).
 * Synchronises the device before the tables are replaced: a launch queued earlier, on any stream, sees the old distribution whole. */
int mythos_oxdna_set_pseq(mythos_system_t* sys, const double* marginals, const int32_t* unit, int n_bp,
                          const double* bp_probs, int terms);

/* dU/d(sequence distribution): what jax.grad of the reference's energy function returns for the `pseq` leaves
 * (compute_seq_dep_weight is differentiable in them, mythos/energy/utils.py:45-132).  The energy call with parameter
 * partials, plus, per frame,
 *   dU_dmarginals  device double[n_frames][n][4]        dU/d(marginal base probabilities) through the pairs whose two
 *                                                        nucleotides are independent (different units)
 *   dU_dbp         device double[n_frames][max(n_bp,1)][4]  dU/d(type probabilities) through the pairs that ARE a
 *                                                        constrained base pair
 * in the layout mythos_oxdna_set_pseq took; the host carries them to the reference's (unpaired, base-pair) arrays - a
 * paired nucleotide's marginal is a sum of its pair's type probabilities.  Accumulated with fp64 atomics: equal to
 * rounding between runs, not bit for bit.  Needs mythos_oxdna_set_pseq with terms != 0.  Asynchronous on the stream, as
 * mythos_oxdna_energy. */
int mythos_oxdna_energy_dpseq(mythos_system_t* sys, const void* center, const void* quat, int n_frames, double* e_terms,
                              void* dU_dcenter, void* dU_dquat, double* dU_dparams, double* dU_dmarginals, double* dU_dbp,
                              mythos_stream_t stream);

/* Unbonded pair list, reference semantics (NoNeighborList.idx, simulators/jax_md/utils.py:48-67):
 * host int32[n_pairs][2], rows (op_i, op_j) in that role order.  Converted to per-nucleotide rows.  Synchronises the device
 * before the rows are replaced, as the other setters of a system do: an energy or MD launch queued earlier, on any stream,
 * walks the old rows. */
int mythos_oxdna_set_neighbors(mythos_system_t* sys, const int32_t* pairs, int n_pairs);

/* GPU Verlet list with bonded exclusions from positions (replaces mythos/utils/neighbors.py:12-59):
 * center dev real[n][3]; pairs with |c_i - c_j| < r_cut + skin are kept.  The build runs on the stream and the call
 * synchronises it at least once (rows and cell buckets grow until the build fits): launches queued on that stream before the
 * call have finished with the old rows, launches on other streams are the caller's to order. */
int mythos_oxdna_build_neighbors(mythos_system_t* sys, const void* center, double r_cut, double skin,
                                 mythos_stream_t stream);
/* max and mean row length of the current list (directed neighbours per nucleotide); synchronises the device, as
 * mythos_oxdna_get_rows does */
int mythos_oxdna_neighbor_stats(mythos_system_t* sys, int* max_row, double* mean_row);
/* The rows the device holds (diagnostics / tests; synchronises): host int32 rows[n][*stride] - the bonded slots, then the
 * close segment, then the far segment, an entry = neighbour index | role bit - row_len[n] (bonded slots included) and
 * row_close[n] (end of the close segment).  Call with all three null to learn *stride, then with buffers of that size;
 * any of the three may be null. */
int mythos_oxdna_get_rows(mythos_system_t* sys, int32_t* rows, int32_t* row_len, int32_t* row_close, int* stride);

/* Energy of n_frames configurations; replaces ComposedEnergyFunction.compute_terms / map
 * (mythos/energy/base.py:312-319, 90-93) and the jax.grad of them.
 *   center      dev real[n_frames][n][3]
 *   quat        dev real[n_frames][n][4]
 *   e_terms     dev double[n_frames][8]                      (required)
 *   dU_dcenter  dev real[n_frames][n][3] or NULL
 *   dU_dquat    dev real[n_frames][n][4] or NULL             (gradient w.r.t. the un-normalised quaternion,
 *                                                            as jax.grad of mythos/energy/utils.py:18-36 gives)
 *   dU_dparams  dev double[n_frames][n_params] or NULL       (flat vector; dependent entries treated as free)
 * Asynchronous on the stream: launches only, no synchronisation, no host read.
 */
int mythos_oxdna_energy(mythos_system_t* sys, const void* center, const void* quat, int n_frames, double* e_terms,
                        void* dU_dcenter, void* dU_dquat, double* dU_dparams, mythos_stream_t stream);

/* Debye-Hueckel energy of n_frames configurations at n_kt temperatures: the part of a temperature sweep of the energy
 * that is not a host-side scale of one ordinary energy call.  Replaces the Debye term of the reference's
 * vmap(lambda kt: energy_fn.with_params(kt=kt).map(trajectory)) (mythos/observables/melting_temp.py:127-140,
 * mythos/energy/dna2/debye.py:47-110): every backbone-backbone distance is computed once and the n_kt constant sets are
 * evaluated on it.  Uses the system's current neighbour rows, box, precision, end flags and DH_HALF_CHARGED_ENDS; the
 * term weight is not applied (row t at the system's own constants equals e_terms[:, 7] of mythos_oxdna_energy).
 *   center, quat  as mythos_oxdna_energy
 *   dh_consts     host double[n_kt][MYTHOS_DEBYE_SWEEP_CONSTS]: DH_KAPPA, DH_PREFACTOR, DH_BSMOOTH, DH_RCUT, DH_RHIGH
 *   e_dh          dev double[n_kt][n_frames]
 *   de_dconsts    dev double[n_kt][n_frames][MYTHOS_DEBYE_SWEEP_CONSTS] or NULL: partials with respect to the constants
 *                 (the DH_* columns of dU_dparams at each temperature, without the term weight)
 * Models 2 (oxDNA2) and 3 (oxRNA2); model 1 has no such term and model 4 (oxNA: three constant sets per temperature) is
 * refused with MYTHOS_ERR_INVALID_ARGUMENT.  n_frames = 0 or n_kt = 0 returns MYTHOS_OK.  Reproducible bit for bit.
 * Asynchronous on the stream; dh_consts is copied in stream order and must stay alive until the stream has passed the call. */
#define MYTHOS_DEBYE_SWEEP_CONSTS 5
int mythos_oxdna_debye_sweep(mythos_system_t* sys, const void* center, const void* quat, int n_frames, int n_kt,
                             const double* dh_consts, double* e_dh, double* de_dconsts, mythos_stream_t stream);

/* oxDNA's `bond` and `mindistance` order parameters of n_frames configurations: what an oxDNA umbrella-sampling run
 * writes per configuration into the order-parameter columns of its energy file, which the reference reads back
 * (mythos/simulators/oxdna/utils.py:348-384) as the bind_states of mythos/observables/melting_temp.py:109-140.
 *   bond         number of listed pairs whose hydrogen-bonding energy is < hb_cutoff (oxDNA's HB_CUTOFF is -0.1)
 *   mindistance  smallest minimum-image distance between the base (hydrogen-bonding) sites of the listed pairs
 * The hydrogen-bonding energy of a pair is the one mythos_oxdna_energy sums: the system's current parameters, sequence
 * and sequence-dependent weights, box and precision; the lower index takes the reference's role op_i, so (j, i) gives
 * what (i, j) gives.  A pair listed twice counts twice.  Needs parameters, not neighbour rows.
 *   center, quat  as mythos_oxdna_energy
 *   op_kind       host int32[n_ops]: MYTHOS_OP_BOND or MYTHOS_OP_MINDISTANCE
 *   op_first      host int32[n_ops + 1]: order parameter k owns pairs[op_first[k] .. op_first[k + 1]); no empty slice
 *   pairs         host int32[n_pairs][2]: two different nucleotides each
 *   op_out        dev double[n_frames][n_ops]: the count, or the distance (interfaces are the caller's)
 *   hb_out        dev double[n_frames][n_pairs] or NULL: hydrogen-bonding energy of every listed pair
 *   dist_out      dev double[n_frames][n_pairs] or NULL: base-base distance of every listed pair
 * The lists are kept on the device between calls; a call with other lists first waits for `stream`.  Models 1, 2 and 3;
 * model 4 (oxNA) and a system with a probabilistic sequence (an expected energy below the cutoff is not oxDNA's order
 * parameter) are refused with MYTHOS_ERR_INVALID_ARGUMENT.  n_frames = 0 or n_ops = 0 returns MYTHOS_OK.  Reproducible
 * bit for bit. */
#define MYTHOS_OP_BOND 0
#define MYTHOS_OP_MINDISTANCE 1
int mythos_oxdna_order_params(mythos_system_t* sys, const void* center, const void* quat, int n_frames, int n_ops,
                              const int32_t* op_kind, const int32_t* op_first, const int32_t* pairs, int n_pairs,
                              double hb_cutoff, double* op_out, double* hb_out, double* dist_out, mythos_stream_t stream);

/* ---- per-frame structural observables ------------------------------------------------------------
 * Replaces mythos/observables/propeller.py:19-71, pitch.py:33-102, rise.py:21-80 and the per-state part of
 * persistence_length.py:47-91, 168-185 (base.py:24-66 for the local helical axis and the quartets).
 *   geometry    host double[3]: com_to_hb, backbone offset along a1, backbone offset along a2 (0 for oxDNA1; for
 *               oxRNA2, model 3, the offset along a3)
 *   box         host double[3] periodic box of the displacement function, or NULL (free space); a box with an edge
 *               that is not positive is refused (NULL, "box edges must be positive"), as mythos_duplex_obs_create does
 *   base_pairs  host int32[n_bp][2]       hydrogen-bonded pairs of the propeller twist
 *   quartets    host int32[n_q][2][2]     adjacent base pairs ((a1, b1), (a2, b2)) of rise / pitch / persistence length
 *   skip_ends   drop two quartets at either end in the persistence-length partials (persistence_length.py:84-87)
 * Output row per frame, mythos_observables_width() = 4 + n_corr doubles (n_corr = n_q - 4 with skip_ends, else n_q):
 *   [0] propeller twist (deg)  [1] rise (Angstrom)  [2] pitch angle (rad)  [3] mean base-pair spacing <l0>
 *   [4 + d] autocorrelation C(d) of the local helical axes.   Entries whose list is empty are 0.
 * mythos_observables_eval is the stand-alone launch; mythos_oxdna_energy_obs returns the same rows with the energies - the
 * same kernel, queued behind the energy launch of that call while the frames are still in L2 (energies, dU/dparams and
 * observables from one call: the DiffTRe data path). */
mythos_obs_t* mythos_observables_create(int model, int n, const double* geometry, const double* box, int n_bp,
                                        const int32_t* base_pairs, int n_quartets, const int32_t* quartets, int skip_ends,
                                        int dtype, int device);
void mythos_observables_destroy(mythos_obs_t* obs);
int mythos_observables_width(const mythos_obs_t* obs);
/* center dev real[n_frames][n][3], quat dev real[n_frames][n][4], out dev double[n_frames][width]; asynchronous on the stream */
int mythos_observables_eval(mythos_obs_t* obs, const void* center, const void* quat, int n_frames, double* out,
                            mythos_stream_t stream);
/* mythos_oxdna_energy with observables in the same launch: obs may be NULL (then identical to mythos_oxdna_energy);
 * obs_out dev double[n_frames][width].  Asynchronous on the stream, as both are. */
int mythos_oxdna_energy_obs(mythos_system_t* sys, const void* center, const void* quat, int n_frames, double* e_terms,
                            void* dU_dcenter, void* dU_dquat, double* dU_dparams, mythos_obs_t* obs, double* obs_out,
                            mythos_stream_t stream);

/* ---- Langevin integrator ----------------------------------------------------------------------
 * Replaces jax_md.simulate.nvt_langevin on RigidBody states as driven by
 * mythos/simulators/jax_md/jaxmd.py:73-94: BAOAB, rigid-body rotation with body-frame angular
 * momentum (equivalent to the quaternion-momentum NO_SQUISH form), counter-based RNG.
 *   gamma_t/gamma_r   friction of the translational / rotational thermostat
 *   inertia           host double[3] principal moments
 */
mythos_sim_t* mythos_langevin_create(mythos_system_t* sys, double dt, double kT, double gamma_t, double gamma_r,
                                     double mass, const double* inertia, uint64_t seed);
/* Order of destruction: an integrator may be destroyed after the system it was created on, but must not be USED after
 * it - every other entry point of an integrator reads its system. */
void mythos_langevin_destroy(mythos_sim_t* sim);

/* neighbour-list policy of the MD loop: rebuild every `every` steps with cut-off r_cut + skin
 * (every <= 0: keep the list given by set_neighbors for the whole run) */
int mythos_langevin_set_neighbor_policy(mythos_sim_t* sim, double r_cut, double skin, int every);

/* draw Maxwell-Boltzmann momenta at kT (init_fn of nvt_langevin); one launch, asynchronous on the stream */
int mythos_langevin_init_momenta(mythos_sim_t* sim, void* p_lin, void* p_ang, mythos_stream_t stream);

/* Run n_steps; state arrays are updated in place.
 *   center dev real[n][3], quat dev real[n][4], p_lin dev real[n][3], p_ang dev real[n][3] (body frame)
 *   save_every > 0: traj_center dev real[n_steps/save_every][n][3], traj_quat [..][n][4] (aligned to 4 elements)
 *   receive the state after steps save_every, 2*save_every, ...; e_trace dev double[n_steps/save_every][10] receives
 *   the 8 term energies + translational + rotational kinetic energy (any of the three may be NULL).
 *   e_trace == NULL is the reference's own run (mythos/simulators/jax_md/jaxmd.py:84-99 stores state.position of every
 *   step and nothing else): the step launch that produces a saved state writes it to its row too - 7 more words per
 *   nucleotide and saved step, no other cost.  e_trace != NULL selects the energy-trace instantiation of the step
 *   kernel for the saved steps plus one small reduction launch per row.
 * A site that outruns the Verlet skin before the scheduled rebuild, or rows / cell buckets that outgrow their
 * allocation, halt the queued launches; the run rebuilds at the last valid state and resumes (not an error; counted
 * by mythos_langevin_last_recoveries).  MYTHOS_ERR_OVERFLOW only after 64 such rebuilds in one run, or when one
 * nucleotide has more than 32 neighbours inside the range of an angular term (up to 16 the fast instantiation runs; a
 * launch that finds more aborts, nothing it wrote counts, and the step is repeated with 32 result rows per nucleotide).
 * After an error the arrays hold the positions of the last step that counted and momenta short of that step's closing
 * half kick; mythos_langevin_get_step tells how many steps that was.
 * The call synchronises the stream (load; advance; store - at least the one synchronisation of advance); the copy back to
 * the caller's arrays is queued behind it, asynchronous on the stream. */
int mythos_langevin_run(mythos_sim_t* sim, void* center, void* quat, void* p_lin, void* p_ang, int n_steps,
                        int save_every, void* traj_center, void* traj_quat, double* e_trace,
                        mythos_stream_t stream);
/* Resident form of the same loop: the state stays in the integrator's own layout on the device between calls, as
 * the carry of the reference's jax.lax.scan stays on its device (mythos/simulators/jax_md/jaxmd.py:87-94).
 *   load     caller's arrays -> resident state (asynchronous); the neighbour list is rebuilt at the next advance
 *   advance  n_steps on the resident state; the list and its rebuild schedule carry over from the previous advance;
 *            outputs as mythos_langevin_run.  One stream synchronisation per call (the halt-and-resume protocol
 *            needs the host to see the control words before the steps count as taken), nothing else between calls
 *   store    resident state -> caller's arrays (asynchronous on the stream; an OPEN frame is closed first by one more
 *            launch through the loop of advance, with its synchronisation); the state stays resident
 * mythos_langevin_run(...) == load; advance; store.  advance after advance continues bit for bit like one advance
 * of the summed length.  An advance that ends in MYTHOS_ERR_NUMERIC drops the resident state.
 * One force evaluation per step: advance(n) is n launches of the step kernel and leaves the resident momenta short of
 * the closing half kick of step n, which needs the forces at x_n - the evaluation the next advance starts with anyway
 * (as the reference's carry holds the force of the last step for the next one, jax_md simulate.nvt_langevin).  store
 * supplies it with one more launch when the frame is still open, so what store hands back is always (x_n, p_n); an
 * advance whose last step saves an ENERGY row (e_trace != NULL) closes while it evaluates that row.  An open frame is
 * closed with the parameters / sequence distribution in force WHEN IT IS CLOSED: a caller that replaces them between
 * two advances (mythos_oxdna_set_params, mythos_oxdna_set_pseq) and wants step n finished under the old ones calls store
 * first.  The mythos_langevin_last_* figures
 * describe the last call that launched step kernels, store's closing launch included. */
int mythos_langevin_load(mythos_sim_t* sim, const void* center, const void* quat, const void* p_lin, const void* p_ang,
                         mythos_stream_t stream);
int mythos_langevin_advance(mythos_sim_t* sim, int n_steps, int save_every, void* traj_center, void* traj_quat,
                            double* e_trace, mythos_stream_t stream);
int mythos_langevin_store(mythos_sim_t* sim, void* center, void* quat, void* p_lin, void* p_ang, mythos_stream_t stream);

/* absolute step counter (RNG stream position); settable for checkpoint/resume.  A host number, read when a launch is
 * queued: neither call synchronises or touches the device, and a launch queued earlier keeps the value it was queued with. */
int64_t mythos_langevin_get_step(const mythos_sim_t* sim);
int mythos_langevin_set_step(mythos_sim_t* sim, int64_t step);
/* the key of the noise (Philox key; init_momenta draws from it too): what a new `key` argument of the reference's
 * run(opt_params, init_state, n_steps, key) is (mythos/simulators/jax_md/jaxmd.py:60-68), without a new integrator.
 * A host number passed by value to every launch: does not synchronise; launches queued earlier keep the old key. */
int mythos_langevin_set_seed(mythos_sim_t* sim, uint64_t seed);

/* Constant external forces: oxDNA's external force of `type = string` with `rate = 0` (the reference ships the
 * experiment as data/templates/force-ext/: a 220-nt duplex and eight force files, +-z on the two end pairs), a constant
 * force on the centre of mass of each listed nucleotide, no torque.
 *   index   host int32[count]     nucleotides, each in [0, n) and listed once (a caller with repeats sums them first)
 *   force   host double[count][3] stored on the device in the system's precision
 *   count = 0 clears the forces; a run without forces issues exactly the launches it issued before this entry existed.
 * With forces set every step launch is preceded by one small launch that kicks the listed momenta by the multiple of
 * dt F_ext the step launch itself applies of dt F (1/2 on the first launch of a closed frame and on a closing-only one,
 * 1 otherwise): a kick by a constant force commutes with the kick by the interaction force, so the pair is BAOAB with
 * the total force.  The kick follows the halt / abort / resume protocol of the step launches (it skips when they skip
 * and is applied once however often a launch is repeated).
 * MYTHOS_ERR_INVALID_ARGUMENT while the resident frame is open (after mythos_langevin_advance: the pending closing half
 * kick would mix two forces) - valid before mythos_langevin_load and after mythos_langevin_store; also for an index out
 * of range or listed twice.  mythos_langevin_run / _advance refuse to step with forces on the unfused oxNA path
 * (MYTHOS_LANGEVIN_UNFUSED); the fused oxNA kernel is supported.
 * The energy-trace rows stay what they are: the external potential -sum F.x is not part of them (it does not depend on
 * the model parameters and cancels in DiffTRe weights), and the kinetic energies of a row are taken after the external
 * kick of that launch, i.e. with the external part of the NEXT step's opening half kick already in the momenta.
 * Synchronises the device before a list is replaced (count > 0); count = 0 only clears a host number. */
int mythos_langevin_set_external_forces(mythos_sim_t* sim, int count, const int32_t* index, const double* force);

/* Position-dependent external forces on centres of mass - the three fixes of the reference's stretch-torsion protocol
 * (data/templates/lammps-stretch-tors/: LAMMPS' spring/self, addforce with a variable of summed coordinates, addtorque).
 * None is a body torque.  Coordinates are the integrator's own, unfolded and without a minimum image.
 *   tethers  F_i = -k_i A_i (x_i - a_i),  U = sum k_i / 2 |A_i (x_i - a_i)|^2
 *     t_index  host int32[n_tethers]      nucleotides, each in [0, n) and listed once
 *     t_k      host double[n_tethers]     k_i >= 0
 *     t_anchor host double[n_tethers][3]  a_i
 *     t_mask   host int32[n_tethers]      A_i: bit 0 / 1 / 2 set = x / y / z restrained
 *   groups, a CSR list: group g has the members g_member[g_first[g] .. g_first[g + 1]), distinct within the group; a
 *   nucleotide may be in several groups and have a tether as well
 *     g_kind   host int32[n_groups]       MYTHOS_RESTRAINT_SUM or MYTHOS_RESTRAINT_TORQUE
 *     g_first  host int32[n_groups + 1]   g_first[0] = 0
 *     g_member host int32[g_first[n_groups]]
 *     g_vec    host double[n_groups][3]   sum: (k, unused, unused), k >= 0;  torque: T, |T| > 0
 *     g_target host double[n_groups][3]   sum: s0 (torque: unused)
 *     g_mask   host int32[n_groups]       sum: A as above (torque: unused)
 *   sum restraint:  s = sum_{j in G} x_j,  F_i = -k A (s - s0) on every member,  U = k / 2 |A (s - s0)|^2  (at least 1 member)
 *   torque:         d_i = x_i - centroid(G),  t = T / |T|,  S = sum_j |d_j - (d_j.t) t|^2,  F_i = (T x d_i) / S: the forces
 *                   add up to zero and their torque about the centroid along t is |T| (at least 2 members).  A group
 *                   whose members all lie on the axis (S = 0; in floating point S <= 1e-24 sum |x_j|^2) gets no force.
 *                   The torque has no potential.
 * Everything is held and summed in double in both precisions, in a fixed order: a run is reproducible to the bit.
 * n_tethers = n_groups = 0 clears the restraints; a run without restraints issues no launch for them, and constant
 * forces (mythos_langevin_set_external_forces) keep exactly their own launch.  With restraints set every step launch is
 * preceded by two more small launches - the groups' sums, then the kick of every restrained momentum by the multiple of
 * dt F(x) that step launch applies of dt F, F taken at the positions that launch reads, which the kick does not write:
 * the pair is BAOAB with the total force.  The kick follows the halt / abort / resume protocol as the constant one does.
 * MYTHOS_ERR_INVALID_ARGUMENT: while the resident frame is open (as mythos_langevin_set_external_forces); an index out of
 * range; a nucleotide listed twice among the tethers or within one group; a value that is not finite; k < 0; T = 0; too
 * few members.  mythos_langevin_run / _advance refuse to step with restraints on the unfused oxNA path.
 * The energy-trace rows stay what they are: neither the tether nor the sum-restraint energy is part of them (nor the
 * work of the torque, which has no potential), and the kinetic energies of a row are taken after the external kicks of
 * that launch - see mythos_langevin_set_external_forces.  mythos_langevin_eval_external returns the energies.
 * Synchronises the device before the arrays are replaced (not when an empty set replaces an empty one). */
enum mythos_restraint_kind { MYTHOS_RESTRAINT_SUM = 0, MYTHOS_RESTRAINT_TORQUE = 1 };
int mythos_langevin_set_restraints(mythos_sim_t* sim, int n_tethers, const int32_t* t_index, const double* t_k, const double* t_anchor,
                                   const int32_t* t_mask, int n_groups, const int32_t* g_kind, const int32_t* g_first,
                                   const int32_t* g_member, const double* g_vec, const double* g_target, const int32_t* g_mask);

/* The external field of the integrator - constant forces, tethers, sum restraints and torques - at the caller's centres,
 * through the kernels the integrator kicks with (c dt = 1 on zeroed momenta).  Needs no resident state and changes none.
 *   center     device (N,3), the system's precision
 *   force_out  device (N,3), the system's precision
 *   energy_out device double[3]: -sum F.x of the constant forces, the tether energy, the sum-restraint energy
 * Asynchronous on `stream`; the scratch arrays belong to the integrator, so one call at a time per integrator. */
int mythos_langevin_eval_external(mythos_sim_t* sim, const void* center, void* force_out, double* energy_out, mythos_stream_t stream);

/* Point forces: oxDNA's external forces that act on ONE nucleotide's centre of mass each - the moving `string`, `trap`,
 * `mutual_trap`, `repulsion_plane`, `repulsion_sphere` of an external_forces_file, by oxDNA's definitions.  A set of
 * its own beside the restraints: either is set or cleared without the other, and both add up with the constant forces.
 *   kind         host int32[n_terms]     enum mythos_point_force_kind
 *   particle     host int32[n_terms]     the nucleotide the term acts on; any number of terms may name one nucleotide
 *   ref_particle host int32[n_terms]     mutual trap: the partner (!= particle), which gets no force from this term and
 *                                        needs none of its own; other kinds: ignored
 *   flags        host int32[n_terms]     mutual trap: MYTHOS_POINT_PBC = the minimum image of the system's box; others: 0
 *   param        host double[n_terms][8] by kind, unused words finite (0); dir is normalised here, d = dir / |dir|
 *     STRING       F0, rate, dir.xyz, origin.xyz   F = (F0 + rate s) d                  U = -(F0 + rate s) d.(x - origin)
 *     TRAP         stiff, rate, dir.xyz, pos0.xyz  F = -stiff (x - pos0 - rate s d)     U = stiff / 2 |x - pos0 - rate s d|^2
 *     MUTUAL_TRAP  stiff, r0, rate                 D = x_ref - x, r = |D|: F = stiff (r - r0 - rate s) D / r (r = 0: none)
 *                                                                                       U = stiff / 2 (r - r0 - rate s)^2
 *     PLANE        stiff, position, dir.xyz        h = d.x + position < 0: F = -stiff h d,  U = stiff / 2 h^2;  else 0
 *     SPHERE       stiff, r0, rate, center.xyz     rho = x - center, R = r0 + rate s, |rho| > R:
 *                                                  F = -stiff (1 - R / |rho|) rho,     U = stiff / 2 (|rho| - R)^2;  else 0
 * Time.  s is the step count of the frame whose positions the force is taken at: mythos_langevin_get_step when the
 * integrator stood at that frame.  The kick in front of launch k of a call uses (step at the call's start) + k, a double
 * computed on the host per launch - the same number when a launch is halted, the list rebuilt and the run resumed, and
 * when one advance(a + b) is advance(a) then advance(b); both half kicks around a frame use the force of that frame's
 * s.  mythos_langevin_set_step moves the clock.  Agreement with oxDNA's own trajectories is statistical, as for the
 * rest of the integrator: the laws are oxDNA's, the noise and the splitting are not.
 * The terms join the restraint kick (mythos_langevin_set_restraints): per nucleotide its tether, its groups ascending,
 * then its point terms in the order given, added in double and kicked once - reproducible to the bit, no launch added to
 * the group launch and the kick launch of a step.  A set without point terms launches what it launched before there
 * were any; with neither restraints nor point terms nothing is launched for them.  A STRING with rate = 0 is better
 * given to mythos_langevin_set_external_forces, which keeps its own launch.
 * n_terms = 0 clears the set.  MYTHOS_ERR_INVALID_ARGUMENT, the message naming the term: while the resident frame is
 * open; an index out of range; ref_particle == particle; a value that is not finite; stiff < 0; r0 < 0; dir = 0 on a
 * string, a plane or a moving trap; MYTHOS_POINT_PBC on a system without a box, or on another kind.
 * mythos_langevin_run / _advance refuse to step with point forces on the unfused oxNA path.  The energy-trace rows do
 * not hold these energies; mythos_langevin_eval_external_at returns them.
 * Synchronises the device before the arrays are replaced (not when an empty set replaces an empty one). */
enum mythos_point_force_kind {
  MYTHOS_POINT_STRING = 0,
  MYTHOS_POINT_TRAP = 1,
  MYTHOS_POINT_MUTUAL_TRAP = 2,
  MYTHOS_POINT_PLANE = 3,
  MYTHOS_POINT_SPHERE = 4,
  MYTHOS_POINT_KINDS = 5
};
enum mythos_point_force_flag { MYTHOS_POINT_PBC = 1 };
int mythos_langevin_set_point_forces(mythos_sim_t* sim, int n_terms, const int32_t* kind, const int32_t* particle,
                                     const int32_t* ref_particle, const int32_t* flags, const double* param);

/* The checks of mythos_langevin_set_point_forces on their own, for a system of n nucleotides with (has_box != 0) or
 * without a box: MYTHOS_OK, or MYTHOS_ERR_INVALID_ARGUMENT and the message.  Touches no device. */
int mythos_point_forces_check(int n, int has_box, int n_terms, const int32_t* kind, const int32_t* particle, const int32_t* ref_particle,
                              const int32_t* flags, const double* param);

/* mythos_langevin_eval_external at step count `step`, with the point forces' energies:
 *   energy_out device double[8]: the three words of mythos_langevin_eval_external, then the energy of the point terms
 *                                of each kind in the enum's order (string, trap, mutual trap, plane, sphere)
 * mythos_langevin_eval_external is this function at step = 0 with the first three words.  Asynchronous on `stream`, and one
 * call at a time per integrator, as that one. */
int mythos_langevin_eval_external_at(mythos_sim_t* sim, const void* center, double step, void* force_out, double* energy_out,
                                     mythos_stream_t stream);

/* Integrator options.  MYTHOS_LANGEVIN_UNFUSED (oxNA systems only, value 0 / 1): step through the two-launch path -
 * the energy kernel's forces launch + a one-thread-per-nucleotide integrator - instead of the fused step kernel.  A
 * second implementation of the same map (same Philox stream), kept as the cross-check of the fused oxNA instantiation;
 * it has no halt-and-resume (a skin violation is an error).  Takes effect at the next mythos_langevin_load / _run and
 * holds while that state is resident. */
enum mythos_langevin_option { MYTHOS_LANGEVIN_UNFUSED = 0 };
int mythos_langevin_set_option(mythos_sim_t* sim, int option, int64_t value);

/* timing hook for bench.py, HIP events on the launch stream of the last run / advance (all zero unless
 * mythos_langevin_set_timing asked for samples: an untimed run records no events at all):
 *   kernel_ms            mean duration of the step kernel over up to 16 launches spread evenly over the
 *                        run, each timed by its own event pair attached to the dispatch
 *                        (hipExtLaunchKernelGGL start/stop events = the dispatch's begin/end stamps)
 *   loop_ms_per_launch   (last event - first event) / launches: includes neighbour rebuilds and
 *                        inter-kernel gaps */
/* samples: how many dispatches of a run get their own event pair (0 = none, the default; at most 16).  A bracketed
 * dispatch costs ~8 us of queue time, so timing is something the caller switches on (bench.py does).
 * Host numbers: set_timing is read by the next run / advance, last_kernel_ms returns what the last one stored after its
 * own stream synchronisation; neither call synchronises. */
int mythos_langevin_set_timing(mythos_sim_t* sim, int samples);
int mythos_langevin_last_kernel_ms(const mythos_sim_t* sim, double* kernel_ms, double* loop_ms_per_launch,
                                   int* launches, int* samples);

/* How often the last run halted and resumed: a site left its skin before the scheduled rebuild, or a rebuild
 * overflowed its rows / cell buckets.  The launches behind such an event do nothing; the run rebuilds at the last
 * valid state (growing what overflowed) and continues there, so neither is an error - the reference's neighbour
 * list signals `did_buffer_overflow` and leaves the reallocation to the caller (jax_md partition, used at
 * mythos/simulators/jax_md/utils.py:70-126).  More than 64 in one run fails with MYTHOS_ERR_OVERFLOW.
 * A host number, stored by the call it describes behind that call's own stream synchronisation: the getter does not synchronise. */
int mythos_langevin_last_recoveries(const mythos_sim_t* sim, int* recoveries);
/* scheduled list rebuilds (every rebuild_every steps) that fell inside the last run / advance; the build that creates a
 * list and the out-of-turn ones above are not counted.  bench.py reports it next to the timed region.  A host number, as
 * mythos_langevin_last_recoveries: the getter does not synchronise. */
int mythos_langevin_last_rebuilds(const mythos_sim_t* sim, int* scheduled);

/* ---- umbrella sampling on the resident Langevin state ---------------------------------------------
 * Replaces the external oxDNA run behind the reference's oxDNAUmbrellaSampler (mythos/simulators/oxdna/oxdna.py:225-275)
 * and the order-parameter and weight columns it reads back (mythos/simulators/oxdna/utils.py:348-429) for the `bond` and
 * `mindistance` order parameters of mythos_oxdna_order_params, per replica of a batched free-space system (replica r
 * owns the nucleotides [r n / n_rep, (r + 1) n / n_rep)) or for one periodic system (n_rep = 1).
 * Method: segment-Metropolis on the integrator.  A segment is segment_steps ordinary steps from a closed frame (x, p),
 * closed again by the launch mythos_langevin_store uses; the replica's proposal (x', p') has order-parameter state s' and
 * is accepted iff W(s') > 0 and u W(s) < W(s'), s the state it holds; a rejected replica goes back to (x, -p) - linear and
 * body-frame angular momenta negated.  The Langevin map is reversible with respect to the Boltzmann density under
 * momentum reversal up to the integrator's O(dt^2) error, so the chain leaves pi(x, p) W(Q(x)) invariant.  Weights and the
 * decision are double in both precisions; u = (c[0] + 0.5) 2^-32 from Philox4x32-10 with the integrator's seed as key and
 * the counter {replica, step lo, step hi, 4}, step the absolute step count at the boundary.  The neighbour rows are
 * rebuilt at the start of every segment exactly as after mythos_langevin_load (the closed frame passes through the
 * kernels of store and load), so a run does not depend on which replicas were rejected, and with a flat table it is bit
 * for bit the loop load; advance(segment_steps); store.
 *   op_kind, op_first, pairs  as mythos_oxdna_order_params; pairs name nucleotides of ONE replica, [0, n / n_rep)
 *   iface_first   host int32[n_ops + 1]: a mindistance parameter k owns interfaces[iface_first[k] .. iface_first[k + 1]), its
 *                 state is the number of them the distance exceeds (strictly); a bond parameter owns none, its state is
 *                 the count
 *   table_shape   host int32[n_ops]; table host double[prod(table_shape)], dense and row-major, one axis per order
 *                 parameter, every weight finite and >= 0 (a missing row is weight 0).  An axis holds every reachable
 *                 state: slice length + 1 for bond, interfaces + 1 for mindistance; a shorter one is refused
 * mythos_umbrella_check: the checks alone, for a system of n nucleotides of `model` whose backbone neighbours inside one
 * replica are bonded[n_bonded][2] (a listed pair must not be one).  Touches no device.
 * mythos_langevin_set_umbrella: n_ops = 0 clears the bias; with none set every other call issues exactly the launches it
 * issued before.  Refused (MYTHOS_ERR_INVALID_ARGUMENT, by name) while the resident frame is open, for moving point forces
 * (rate != 0: the force depends on the step count, which breaks reversibility), the unfused oxNA path, model 4 and a
 * probabilistic sequence - advance_umbrella refuses the same should they appear later.
 * mythos_langevin_advance_umbrella: n_segments segments on the resident state (an open frame is closed first).  The first
 * call after a load or a set_umbrella primes: the resident state becomes every replica's snapshot, and a replica whose
 * state has weight 0 is an error naming it.  So does the first call after anything else that moved the state or its
 * weights away from the snapshot: unbiased steps (mythos_langevin_advance with n_steps > 0, mythos_langevin_run, which
 * loads) and new parameters (mythos_oxdna_set_params) - the chain starts again from the state as it stands, and no
 * rejection reaches back across them.  One stream synchronisation per segment.  All outputs are device arrays,
 * any may be NULL:
 *   traj_center, traj_quat  real[n_segments / sample_every][n][3 | 4]: the state after the decision of boundaries
 *                           sample_every, 2 sample_every, ... (sample_every = 0: none); quaternion rows aligned to 4 elements
 *   prop_center, prop_quat  the same rows of the proposals, before the decision
 *   record        double[n_segments][n_rep][3 n_ops + 4]: the proposal's values (as mythos_oxdna_order_params returns
 *                 them for the proposal row, bit for bit), its states, W_old, W_new, u, accept (0 / 1), then the states
 *                 the replica holds after the decision (the sample row's)
 * advance_umbrella(a) then (b) continues bit for bit like one call of a + b segments.
 * mythos_langevin_umbrella_counts: decisions accepted and taken since set_umbrella (the priming boundary is not one).
 * Streams: set_umbrella synchronises the device before its arrays are replaced; advance_umbrella returns with the decision
 * and commit launches of its last boundary still queued on the stream (its outputs are in stream order, as everywhere);
 * umbrella_counts reads the device's counters and synchronises the device first. */
int mythos_umbrella_check(int n, int n_rep, int model, int n_bonded, const int32_t* bonded, int n_ops, const int32_t* op_kind,
                          const int32_t* op_first, const int32_t* pairs, int n_pairs, const int32_t* iface_first,
                          const double* interfaces, const int32_t* table_shape, const double* table, int segment_steps);
int mythos_langevin_set_umbrella(mythos_sim_t* sim, int n_rep, int n_ops, const int32_t* op_kind, const int32_t* op_first,
                                 const int32_t* pairs, int n_pairs, const int32_t* iface_first, const double* interfaces,
                                 const int32_t* table_shape, const double* table, double hb_cutoff, int segment_steps);
int mythos_langevin_advance_umbrella(mythos_sim_t* sim, int n_segments, int sample_every, void* traj_center, void* traj_quat,
                                     void* prop_center, void* prop_quat, double* record, mythos_stream_t stream);
int mythos_langevin_umbrella_counts(mythos_sim_t* sim, int64_t* accepted, int64_t* decided);

/* ---- oxDNA text trajectories (host only) -----------------------------------------------------
 * Replaces the Python parse of mythos/input/trajectory.py:192-320 (frames of `t = / b = / E =` header lines and
 * n rows of 15 numbers: com, a1, a3, v, L).  Call once with frames == NULL to count (n_frames out), then with
 * host buffers times[F], box[F][3], energies[F][3], frames[F][n][15]; at most max_frames are stored.  Rows stay in
 * file order (the 5'->3' reversal of new-format files is the caller's, trajectory.py:309-313). */
int mythos_oxdna_read_trajectory(const char* path, int n, int max_frames, double* times, double* box, double* energies,
                                 double* frames, int* n_frames);

/* Writer for the same format (mythos/input/trajectory.py:322-331, mythos/simulators/io.py:146-170): host buffers
 * times[F], box[F][3], energies[F][3], frames[F][n][15]; every number as the shortest text that parses back to the
 * same double (what the reference's str(float) prints); append != 0 adds to an existing file. */
int mythos_oxdna_write_trajectory(const char* path, int n, int n_frames, const double* times, const double* box,
                                  const double* energies, const double* frames, int append);

/* ---- test and diagnostic switches ---------------------------------------------------------------
 * No counterpart in the reference.  The GPU tests use them to reach code paths that physical inputs reach only by
 * chance (a cell bucket that overflows, a row walk in several segments, a list rebuild that overflows in front of the
 * first launch of a segment).  Process-wide, read when a list is built / a call starts (never per launch); a value of 0
 * restores the default (MYTHOS_DEBUG_ROWS_FILTER excepted: its default is 1).  Nothing in the library reads the environment. */
enum mythos_debug_key {
  MYTHOS_DEBUG_CELL_BUCKET_CAP = 0, /* places per cell bucket, fixed (no growth): exercises the spill list */
  MYTHOS_DEBUG_ENERGY_LIST_CAP = 1, /* entries per segment of the energy kernel's row walk (8 ... 192); used by
                                       tests/test_gpu_energy_shapes.py: rows of 13 - 118 entries in two to fifteen segments */
  MYTHOS_DEBUG_MD_SEGMENT = 2,      /* step launches queued between two looks at the halt word (default 8192) */
  MYTHOS_DEBUG_MD_OVERFLOW_AT = 3,  /* k + 1: the scheduled list rebuild in front of step launch k reports a row
                                       overflow although its rows fit (one shot: cleared when it fires) */
  MYTHOS_DEBUG_MD_DENSE = 4,        /* 1: every fp32 oxDNA1/2 stepping launch takes the DENSE instantiation (normally
                                       grids of more than four workgroups per CU), 2: none does */
  MYTHOS_DEBUG_MD_ITEMS_BIG = 5,    /* 1: oxDNA step launches start on the wide work lists (ITEMS = 32) instead of reaching them
                                       through an aborted launch */
  MYTHOS_DEBUG_MD_LANES = 6,        /* 8 | 16: lanes per nucleotide of the oxDNA step launches, fixed when a state is loaded
                                       (normally 16 where n / 16 workgroups are at most two per CU, 8 otherwise) */
  MYTHOS_DEBUG_ROWS_FILTER = 7,     /* DEFAULT 1 (the one key whose default is not 0): scheduled oxDNA list rebuilds filter candidate
                                       rows where the cell builder makes the rows; 0: the full builder makes every one */
  MYTHOS_DEBUG_ROWS_CAND_EVERY = 8, /* list rebuilds per candidate (wide) build; 0: kCandEvery (csrc/row_filter_plan.h) */
  MYTHOS_DEBUG_ROWS_CAND_MARGIN = 9, /* how far beyond the list range the candidates reach, in thousandths; 0: kCandMarginMilli */
  MYTHOS_DEBUG_KEYS = 10
};
int mythos_debug_set(int key, int64_t value);
int64_t mythos_debug_get(int key);

/* ---- MARTINI 2/3 ------------------------------------------------------------------------------
 * Replaces mythos/energy/martini/m2/{lj,bond,angle}.py and m3/angle.py.
 *   types        host int32[n]            bead type index
 *   sigma, eps   host double[n_types][n_types]
 *   bonds        host int32[n_bonds][2], bond_k / bond_r0 host double[n_bonds]
 *   angles       host int32[n_angles][3], angle_k / angle_t0 host double[n_angles] (t0 in radians)
 *   angle_kind   0 = G96 cosine (MARTINI 2), 1 = harmonic (MARTINI 3)
 *   r_cut        LJ cut-off (1.1 nm in the reference), potential shifted to 0 at r_cut
 * Energy terms per frame: [lj, bond, angle].  box dev real[n_frames][3] (per-frame periodic box).
 */
#define MYTHOS_MARTINI_N_TERMS 3
mythos_martini_t* mythos_martini_create(int n, const int32_t* types, int n_types, const double* sigma,
                                        const double* eps, int n_bonds, const int32_t* bonds, const double* bond_k,
                                        const double* bond_r0, int n_angles, const int32_t* angles,
                                        const double* angle_k, const double* angle_t0, int angle_kind, double r_cut,
                                        int dtype, int device);
void mythos_martini_destroy(mythos_martini_t* m);
/* New values for the parameter tables of mythos_martini_create, shapes as there, in place: the handle, and every integrator
 * bound to it with its resident state and lists, stay (an integrator takes the new tables at the head of its next call).
 * A NULL table keeps its values.  What the reference does by writing new GROMACS parameter files before every run
 * (mythos/simulators/gromacs/gromacs.py:70-131).  Synchronises the device. */
int mythos_martini_set_params(mythos_martini_t* m, const double* sigma, const double* eps, const double* bond_k, const double* bond_r0,
                              const double* angle_k, const double* angle_t0);
/* Energies [lj, bond, angle] per frame and optionally dU/dpos; all-pairs sweep, fixed-order reduction.  Asynchronous on the stream. */
int mythos_martini_energy(mythos_martini_t* m, const void* pos, const void* box, int n_frames, double* e_terms,
                          void* dU_dpos, mythos_stream_t stream);

/* Parameter gradients per frame (the reference: jax.grad of the same energy functions with respect to the
 * configuration values, mythos/energy/martini/m2/lj.py:137-157, bond.py:60-71, angle.py:113-129).
 * All outputs are dev double and optional (NULL = skip), except that d_sigma and d_eps come as a pair:
 *   d_sigma, d_eps   [n_frames][n_types][n_types]  dU_lj/dsigma[a][b], dU_lj/deps[a][b] for the ORDERED type
 *                    pair (owner, partner), each unordered bead pair contributing half to either order: the
 *                    derivative with respect to a symmetric entry is out[a][b] + out[b][a]
 *   d_bond_k/_r0     [n_frames][n_bonds]     d_angle_k/_t0  [n_frames][n_angles]   (one value per bond / angle;
 *                    the host sums the bonds that share a named parameter)
 * Asynchronous on the stream. */
int mythos_martini_param_grads(mythos_martini_t* m, const void* pos, const void* box, int n_frames, double* d_sigma,
                               double* d_eps, double* d_bond_k, double* d_bond_r0, double* d_angle_k,
                               double* d_angle_t0, mythos_stream_t stream);

/* Reaction-field Coulomb (GROMACS' coulombtype = reaction-field with the Verlet scheme's potential shift, the setting of
 * every MARTINI run the reference drives: data/templates/martini/m2/DMPC/<T>/md.mdp, epsilon_r = 15, epsilon_rf = 0).  The reference
 * itself evaluates no Coulomb term and ships no Coulomb energies: the formula below is the pin.  Units nm, kJ/mol, e.
 *   f = 138.935458, k_rf = (eps_rf - eps_r) / ((2 eps_rf + eps_r) r_c^3) (eps_rf = 0 means infinity: 1 / (2 r_c^3)),
 *   c_rf = 1 / r_c + k_rf r_c^2, r_c = the system's r_cut (one list, one cut-off)
 *   pair inside r_c, not excluded   V = (f / eps_r) q_i q_j (1 / r + k_rf r^2 - c_rf)
 *   excluded (bonded) pair inside r_c   V = (f / eps_r) q_i q_j (k_rf r^2 - c_rf), with its force
 *   self term                       -1/2 (f / eps_r) c_rf sum q_i^2
 * mythos_martini_set_charges: q host double[n] or NULL.  NULL or all zeros clears the charges - the system then behaves
 * exactly as one that never had any.  Refused: epsilon_r <= 0, epsilon_rf < 0, non-finite input, and more than 8 distinct
 * charge values (0 included): the step kernel keeps them in a table of that size.  mythos_martini_energy,
 * mythos_martini_param_grads and MYTHOS_MARTINI_N_TERMS do not see the charges.  An integrator bound to the system
 * takes the charges in force when a call of it begins (load, run, advance, store, pressure).
 * mythos_martini_coulomb: e_coul dev double[n_frames] (pairs + excluded pairs + self term), dU_dpos dev real[n_frames][n][3]
 * or NULL, written (not accumulated); all-pairs sweep and fixed-order reduction of mythos_martini_energy.  Without charges
 * both are zero.
 * Streams: set_charges synchronises the device before the charge table is replaced; coulomb is asynchronous on the stream. */
int mythos_martini_set_charges(mythos_martini_t* m, const double* q, double epsilon_r, double epsilon_rf);
int mythos_martini_coulomb(mythos_martini_t* m, const void* pos, const void* box, int n_frames, double* e_coul,
                           void* dU_dpos, mythos_stream_t stream);

/* ---- MARTINI Langevin MD ----------------------------------------------------------------------
 * BASELINE configs[2].  The reference runs MARTINI dynamics in GROMACS as an external process
 * (mythos/simulators/gromacs/) and has no integrator of its own for it; this is the device-resident
 * integrator for the same force field (LJ over a Verlet list rebuilt on the device, bonds, angles) with the
 * BAOAB Langevin splitting of mythos_langevin_run for point particles.  Units: nm, ps, amu, kJ/mol.
 *   gamma    friction rate 1/ps (GROMACS sd integrator: 1 / tau_t);  mass host double[n] or NULL (72 amu)
 *   pos, vel dev real[n][3], updated in place;  box host double[3] (orthorhombic, fixed during the run)
 *   traj_pos dev real[n_steps/save_every][n][3] or NULL;  e_trace dev double[.][4] = lj, bond, angle, kinetic
 *   While the system holds charges (mythos_martini_set_charges) the forces include reaction-field Coulomb and a row of
 *   e_trace has FIVE columns: lj, bond, angle, kinetic, coulomb (self term included); the caller allocates for that.
 * Errors and the halt-and-resume protocol as mythos_langevin_run (NUMERIC: NaN). */
mythos_martini_sim_t* mythos_martini_langevin_create(mythos_martini_t* sys, double dt, double kT, double gamma,
                                                     const double* mass, uint64_t seed);
/* (may be destroyed after its system, but must not be used after it: see mythos_langevin_destroy) */
void mythos_martini_langevin_destroy(mythos_martini_sim_t* sim);
int mythos_martini_langevin_set_neighbor_policy(mythos_martini_sim_t* sim, double skin, int rebuild_every);
/* Pruned rows (round 4; no counterpart in the reference - GROMACS, which runs its MARTINI dynamics, prunes its pair list
 * between searches in the same way): every `every` steps the step launch writes, as a by-product of the distances it
 * computes, the entries of each Verlet row inside r_cut + margin to a second set of rows, and the launches in between walk
 * those.  Safe while no bead moves more than margin / 2 between two prunings: checked per step (a step longer than
 * margin / (2 (every - 1)) halts and rebuilds like a bead that leaves its skin).  Off by default; bench.py runs the
 * bilayer with margin 0.2 nm, every 4.  margin <= 0, margin >= skin or every < 2 switches the pruned rows off.  The forces are those of the Verlet rows up to the
 * order of the sums. */
int mythos_martini_langevin_set_inner_list(mythos_martini_sim_t* sim, double margin, int every);
/* Maxwell-Boltzmann velocities at the integrator's kT (an ensemble: every slot at its current kT, with its seed); one
 * launch per copy, asynchronous on the stream */
int mythos_martini_langevin_init_velocities(mythos_martini_sim_t* sim, void* vel, mythos_stream_t stream);
/* load; advance; store in one call: synchronises the stream (the synchronisation of advance, and one more behind the copy
 * back: pos and vel are complete when the call returns) */
int mythos_martini_langevin_run(mythos_martini_sim_t* sim, void* pos, void* vel, const double* box, int n_steps,
                                int save_every, void* traj_pos, double* e_trace, mythos_stream_t stream);
/* Resident form, as mythos_langevin_load / advance / store: the state stays in the integrator's layout on the device
 * between calls, the list and its rebuild schedule carry over, advance(n) is n launches of the step kernel and leaves the
 * frame open (velocities short of the closing half kick of step n; the next advance or store supplies it).
 * mythos_martini_langevin_run == load; advance; store.  advance(a); advance(b) == advance(a + b), bit for bit.
 * e_trace == NULL with traj_pos != NULL: positions-only rows, written by the step launch that produces the saved state.
 * Streams, as for oxDNA: load is asynchronous for a single copy (an ensemble's load first waits for the stream: the staging
 * buffer of its replica table is reused); advance synchronises the stream once per call, and once more per coupling or
 * exchange event; store is asynchronous on a closed frame and closes an open one through the loop of advance first.  The
 * first of these calls after mythos_martini_set_params / _set_charges waits for the stream before it replaces the
 * integrator's own tables. */
int mythos_martini_langevin_load(mythos_martini_sim_t* sim, const void* pos, const void* vel, const double* box,
                                 mythos_stream_t stream);
int mythos_martini_langevin_advance(mythos_martini_sim_t* sim, int n_steps, int save_every, void* traj_pos, double* e_trace,
                                    mythos_stream_t stream);
int mythos_martini_langevin_store(mythos_martini_sim_t* sim, void* pos, void* vel, mythos_stream_t stream);
/* the absolute step counter: a host number, the call does not synchronise */
int64_t mythos_martini_langevin_get_step(const mythos_martini_sim_t* sim);
/* scheduled list rebuilds inside the last advance (as mythos_langevin_last_rebuilds).  This and the three entries below
 * return host numbers the last run / advance stored behind its own stream synchronisation; set_timing sets one the next
 * call reads: none of them synchronises. */
int mythos_martini_langevin_last_rebuilds(const mythos_martini_sim_t* sim, int* scheduled);
int mythos_martini_langevin_last_kernel_ms(const mythos_martini_sim_t* sim, double* kernel_ms,
                                           double* loop_ms_per_launch, int* launches, int* samples);
int mythos_martini_langevin_set_timing(mythos_martini_sim_t* sim, int samples); /* as mythos_langevin_set_timing */
/* out-of-turn rebuilds of the last run (same protocol as mythos_langevin_last_recoveries; a host number, the getter does not
 * synchronise) */
int mythos_martini_langevin_last_recoveries(const mythos_martini_sim_t* sim, int* recoveries);
/* longest and mean Verlet row (an ensemble: over the n_rep n rows); reads the device's row lengths and synchronises the
 * device first, as mythos_martini_langevin_get_rows */
int mythos_martini_langevin_neighbor_stats(const mythos_martini_sim_t* sim, int* max_row, double* mean_row);
/* Diagnostics / tests: the neighbour rows as the device holds them, which = 0 the Verlet rows, 1 the pruned rows
 * (mythos_martini_langevin_set_inner_list).  rows host int32[n][*stride], row_len host int32[n]; with both NULL only
 * *stride is set.  Synchronises the device. */
int mythos_martini_langevin_get_rows(const mythos_martini_sim_t* sim, int which, int32_t* rows, int32_t* row_len, int* stride);

/* ---- MARTINI NPT: pressure and cell-rescaling pressure coupling ------------------------------------------------
 * Stands in for the pressure coupling of the GROMACS runs the reference drives (data/templates/martini/m2/DMPC/273K/
 * md.mdp): kind <- pcoupl, coupling <- pcoupltype, tau_p <- tau-p, compressibility <- compressibility, ref_p <- ref-p,
 * every <- nstpcouple.  First-order cell rescaling only: kind 1 is Berendsen, kind 2 stochastic cell rescaling (C-rescale,
 * Bernetti & Bussi 2020: Berendsen's drift plus its fluctuation-dissipation noise, velocities scaled by 1 / mu); kind 0
 * switches coupling off (the default: every call then runs exactly as without this entry point).  The reference's own
 * choice, Parrinello-Rahman, is not built; neither are anisotropic / off-diagonal coupling or a barostat for oxDNA.
 *   coupling         0 isotropic (ref_p[0], compressibility[0]), 1 semi-isotropic ([0]: xy, [1]: z; compressibility[1] = 0
 *                    fixes the box height, the reference's setting)
 *   ref_p bar, compressibility 1/bar, tau_p ps; compressibility all 0 is "off" as well
 * An event happens at the closed state of every absolute step s > 0 with s % every == 0 (mythos_martini_langevin_get_step
 * counts them), so advance(a); advance(b) stays advance(a + b) bit for bit.  mu = exp(-f (P0 - P) / 3 ...) with
 * f = compressibility every dt / tau_p; GROMACS' Berendsen uses the linear 1 - f (P0 - P) / 3, equal up to O(f^2).
 * The noise is normals6(seed, particle 0, step s, stream 2) of the thermostat's generator.  An event that would make an edge
 * shorter than 2 (r_cut + skin) ends the call with INVALID_ARGUMENT; the state of that step stays resident, unscaled.
 * Each event costs a closing launch, a pressure launch, a list rebuild and one stream synchronisation. */
int mythos_martini_langevin_set_barostat(mythos_martini_sim_t* sim, int kind, int coupling, const double ref_p[2],
                                         const double compressibility[2], double tau_p, int every);
/* Pressure of the resident state (what `gmx energy` reports as Pres-XX / -YY / -ZZ): out = K[3], W[3] (kJ/mol: sum m v_d^2
 * and the virial -dU/dln s_d of LJ + bonds + angles, plus reaction-field Coulomb while the system holds charges), P[3] = (K + W) / V x 16.6053907 (bar), V (nm^3).  Closes an open
 * frame first, as store does; a closed frame is left bitwise as it was.  Synchronises the stream. */
int mythos_martini_langevin_pressure(mythos_martini_sim_t* sim, double out[10], mythos_stream_t stream);
/* the box of the resident state (host double[3]): the one loaded, rescaled by the coupling events since.  A host copy kept up
 * to date behind the synchronisation of every coupling event: the getter does not synchronise. */
int mythos_martini_langevin_get_box(const mythos_martini_sim_t* sim, double box[3]);
/* The box of every row the last run / advance saved, host double[*n_rows][3] (the .gro / .trr box line of a GROMACS
 * trajectory).  A row saved at an event step holds the state before the event and its box.  boxes == NULL: only *n_rows.
 * A host log: the getter does not synchronise. */
int mythos_martini_langevin_last_boxes(const mythos_martini_sim_t* sim, double* boxes, int* n_rows);

/* ---- MARTINI temperature ensemble: n_rep copies of one system, own kT, box, seed and barostat history, one launch per step
 * Replaces the loop of the reference's reparameterisation over its simulation temperatures, one GROMACS run each under
 * the same md.mdp with only ref-t changed (examples/scripts/martini_full_reparameterization.py:347-357 on
 * mythos/simulators/gromacs/gromacs.py:70-131).  Call a copy a replica and n the beads of one (the system's).
 *   kT host double[n_rep], seeds host uint64[n_rep] (NULL: all 0), mass host double[n] or NULL, shared by the replicas
 * The handle is the single integrator's and takes its entry points.  Replica r is, bit for bit, the single integrator
 * made with kT[r] and seeds[r] and loaded with box r, as long as no call reports a recovery (a bead of ANY replica that
 * leaves its skin halts and rebuilds all of them, after which the sums run over rows built at another step).  Shapes:
 *   load / run / store / init_velocities   pos, vel dev real[n_rep][n][3];  box host double[n_rep][3], each checked
 *   advance / run                          traj_pos dev real[rows][n_rep][n][3];  e_trace dev double[rows][n_rep][4 | 5]
 *   last_boxes                             host double[*n_rows][n_rep][3]
 *   get_rows, neighbor_stats               over the n_rep n rows; entries are bead indices inside the replica
 * set_neighbor_policy, set_inner_list, set_barostat, set_timing and the counters apply to all replicas alike; rebuild
 * schedule and halt are global.  mythos_martini_set_charges on the system works as for one copy.  A coupling event is one
 * pressure launch, the single copy's barostat kernel once per replica (noise normals6(seeds[r], 0, step, 2)), one scaling launch
 * and ONE synchronisation; if it would make any replica's box shorter than 2 (r_cut + skin) the call ends with
 * INVALID_ARGUMENT naming the replica, and no replica is scaled.
 * mythos_martini_langevin_pressure / get_box have their shape in the prototype and refuse an ensemble handle; the
 * _ensemble forms take out[n_rep][10] / boxes[n_rep][3], and serve a single-copy handle as n_rep = 1.
 * Refused (NULL / INVALID_ARGUMENT, by name): n_rep < 1, a kT that is not finite and positive, n_rep n beyond
 * INT_MAX / 256 (the initial row stride), at load a box that the single integrator refuses.
 * mythos_martini_ensemble_check: those checks alone for n beads per replica, the cut-off and skin given and boxes
 * host double[n_rep][3] or NULL; touches no device. */
mythos_martini_sim_t* mythos_martini_langevin_create_ensemble(mythos_martini_t* sys, int n_rep, double dt, const double* kT,
                                                              double gamma, const double* mass, const uint64_t* seeds);
int mythos_martini_ensemble_check(int n, int n_rep, const double* kT, double r_cut, double skin, const double* boxes);
int mythos_martini_langevin_n_replicas(const mythos_martini_sim_t* sim); /* 1 for a single-copy handle */
/* A handle made new for another run: seeds host uint64[replicas] (one for a single-copy handle), the step counter set to
 * `step`, the resident state dropped - the next call must be a load or a run.  Settings (list policy, barostat) and buffers stay.
 * After it the handle computes what a handle created with these seeds computes, bit for bit.  An ensemble's ladder goes back
 * to the identity through the path of set_ladder, which synchronises the device; a single copy's restart sets host numbers only. */
int mythos_martini_langevin_restart(mythos_martini_sim_t* sim, const uint64_t* seeds, int64_t step);
/* as mythos_martini_langevin_pressure for every replica: closes an open frame first, synchronises the stream */
int mythos_martini_langevin_pressure_ensemble(mythos_martini_sim_t* sim, double* out, mythos_stream_t stream);
/* as mythos_martini_langevin_get_box for every replica: host copies, the getter does not synchronise */
int mythos_martini_langevin_get_box_ensemble(const mythos_martini_sim_t* sim, double* boxes);

/* ---- MARTINI temperature ensemble: replica exchange between the temperatures -----------------------------------
 * Ensemble handles with n_rep >= 2.  The rule:
 *   Rungs and slots  The ladder's rungs are the kT of create_ensemble in the order given, beta_t = 1 / kT_t in double.
 *                    Slots are the replicas as they lie in memory: slot r keeps its beads, velocities, box, barostat
 *                    history, neighbour rows and thermostat seed for the whole run.  An exchange swaps TEMPERATURES
 *                    between slots; no bead data moves.  rung_of_slot is a permutation of 0 .. n_rep - 1, the identity
 *                    at creation and after restart (load leaves it and the counts alone).
 *   Events           With every = E >= 1 an event happens at the closed state (x_s, v_s) of every absolute step s > 0
 *                    with s % E == 0; its attempt index is a = s / E.  It attempts the rung pairs (t, t + 1) for
 *                    t = a mod 2, a mod 2 + 2, ... while t + 1 < n_rep: disjoint pairs.
 *   Decision         For slot A on rung t and slot B on rung t + 1:  d = (beta_t - beta_t+1) (H_A - H_B),  H = U + p V,
 *                    u = (c[0] + 0.5) 2^-32 of Philox4x32-10 keyed by the 64-bit exchange seed, counter
 *                    {t, s lo, s hi, 5} (stream 5; 0/1 thermostat, 2/3 barostat, 4 umbrella, 7/8 initial velocities);
 *                    accepted iff d >= 0 or u < exp(d).  All in double.
 *   U                lj + bond + angle (+ coulomb while the system holds charges), added in that order, of the values an
 *                    energy row of step s holds: if the call saves one there, U is that row's sum bit for bit.
 *   V, p             V = (lx ly) lz of the slot's box at step s.  p = 0 without a barostat; with one p = p_ref / 16.6053907,
 *                    p_ref = ref_p[0] for isotropic coupling, for semi-isotropic coupling the reference pressure of the
 *                    axis set whose compressibility is non-zero; both non-zero needs ref_p[0] == ref_p[1], otherwise
 *                    advance / run are refused by name (an anisotropic reference stress has no scalar work term).
 *   On acceptance    A takes rung t + 1, B rung t.  A's velocities are multiplied by (real)sqrt(kT_t+1 / kT_t), B's by
 *                    (real)sqrt(kT_t / kT_t+1): quotient and root in double, rounded once to the system's precision,
 *                    the product in that precision.  From the next step on thermostat noise and the barostat's kT' use
 *                    the slot's new kT.
 *   After an event   The neighbour rows are dropped as after a coupling event, accepted or not: the segment behind an event
 *                    is bit for bit the run of a plain ensemble, created with the slots' kT, restarted at step s and loaded
 *                    with the stored state.  One list build per event.
 *   With coupling    At a step with both the exchange comes first, on U and the box of (x_s, box_s); the coupling event
 *                    follows with the new kT' and the rescaled velocities (two synchronisations at such a step).  A row
 *                    saved at step s is the state before both.
 * An event costs a closing launch of the energy-trace instantiation, a reduction, the decision kernel (one workgroup), one
 * rescaling launch, one synchronisation and the list build behind it.  every = 0 switches exchange off: the handle then
 * launches nothing it did not launch before this entry point existed.
 *   set_ladder       rung_of_slot host int32[n_rep], a permutation (anything else is refused); rewrites the slots' kT;
 *                    refused (NOT_READY) while the resident frame is open.  get_ladder: the current one.
 *   last_ladder      host int32[*n_rows][n_rep]: rung_of_slot at every row the last call saved, each the state before the
 *                    events of its step (as last_boxes); rows == NULL: only *n_rows.
 *   last_exchanges   host double[*n][11], the last call's attempts in order: step, t, slot A, slot B, U_A, U_B, V_A, V_B,
 *                    d, u, accepted (0 | 1); rec == NULL: only *n.
 *   exchange_counts  host int64[n_rep - 1] each: attempts and acceptances per rung pair (t, t + 1) since restart.
 * mythos_martini_exchange_check: the refusals that need no handle - n_rep < 2, every < 0, rung_of_slot (host
 * int32[n_rep] or NULL: not checked) not a permutation; touches no device. */
int mythos_martini_langevin_set_exchange(mythos_martini_sim_t* sim, int every, uint64_t seed);
int mythos_martini_langevin_set_ladder(mythos_martini_sim_t* sim, const int32_t* rung_of_slot);
int mythos_martini_langevin_get_ladder(const mythos_martini_sim_t* sim, int32_t* rung_of_slot);
int mythos_martini_langevin_last_ladder(const mythos_martini_sim_t* sim, int32_t* rows, int* n_rows);
int mythos_martini_langevin_last_exchanges(const mythos_martini_sim_t* sim, double* rec, int* n);
int mythos_martini_langevin_exchange_counts(const mythos_martini_sim_t* sim, int64_t* attempts, int64_t* accepts);
int mythos_martini_exchange_check(int n_rep, int every, const int32_t* rung_of_slot);

/* ---- MARTINI integrator: position restraints, flat-bottomed restraints, pulling between centres of mass ----------
 * External forces on the beads of a MARTINI integrator (single copy or ensemble; R = its replicas, 1 for a single copy),
 * applied as a velocity kick queued in front of every step launch: BAOAB with the total force.  Units nm, ps, kJ/mol, amu;
 * every sum in double in both precisions.  s is the step count of the frame the force is taken at, t = s dt.
 *   position restraints  GROMACS' [ position_restraints ] funct 1: U = 1/2 sum_a k_a (x_a - X_a)^2.
 *     pr_index host int32[n_posres] distinct beads; pr_k host double[n_posres][3] >= 0; pr_ref host double[R][n_posres][3].
 *   flat-bottomed restraints  GROMACS' [ position_restraints ] funct 2: U = 1/2 k (d - r)^2 where d > r (inverted: where
 *     d < r), no force at d = 0.  fb_index host int32[n_flat]; fb_flags host int32[n_flat]: shape in bits 0-1 (0 sphere,
 *     d = |x - X|; 1 cylinder, the distance from the axis through X; 2 layer, d = |x_a - X_a|), the axis in bits 2-3,
 *     invert in bit 4; fb_param host double[R][n_flat][5]: k, r, X.xyz.
 *   pull groups  GROMACS' pull-groupN-name / -pbcatom: g_first host int32[n_groups + 1] member ranges, g_member the members
 *     (distinct within a group), g_pbc_ref host int32[n_groups]: a member relative to which the others are taken at their
 *     minimum image, or -1.  Centres of mass are weighted with the integrator's masses.
 *   pull coordinates  GROMACS' pull-coordN-*: p_groups host int32[n_pull][2] = (A, B), A = -1 for the absolute reference
 *     `origin`; p_flags host int32[n_pull]: bit 0 constant-force (else umbrella), bit 1 geometry direction (else distance),
 *     bit 2 periodic (minimum image of D = X_B - X_A in the replica's box), bits 4-6 the axes of dim (distance);
 *     p_param host double[R][n_pull][9]: k, init, rate, vec.xyz (a unit vector), origin.xyz.  distance: xi = |D| over dim, no
 *     force at xi = 0; direction: xi = D . vec.  umbrella U = 1/2 k (xi - init - rate t)^2; constant-force U = k xi (k is
 *     the negative of the force).  Member j of B gets -U'(xi) e m_j / M_B, member j of A +U'(xi) e m_j / M_A.
 *   boxes  host double[R][3], needed when a coordinate is periodic or a group has a pbc_ref (NULL otherwise); a later load
 *     into other boxes is then refused.
 * Coordinates are taken as the frame stores them, unfolded.  All counts zero clears the set: the integrator then launches
 * what it launched before the set existed.  Refused by name (INVALID_ARGUMENT): index out of range, empty group, duplicate
 * member, A = B, k < 0, non-finite value, zero vec, empty dim, r < 0, pbc_ref not a member, a set together with a barostat
 * or with replica exchange in either order of the two calls (the restraint virial and the restraint energy in the
 * exchange's H are not built); NOT_READY while the resident frame is open.
 * mythos_martini_restraints_check: those checks alone for n beads per replica, barostat / exchange saying whether one is
 * set; touches no device.
 * mythos_martini_langevin_eval_external: the field at pos dev real[R][n][3] and step count `step` through the kernels the
 * integrator kicks with: force dev real[R][n][3] (or NULL), energies dev double[R][4] - position, flat-bottom, umbrella,
 * constant-force - (or NULL) and xi dev double[R][n_pull] (or NULL; written with energies).  Needs no resident state.
 * mythos_martini_langevin_pull_values: xi of every coordinate of a stored trajectory, pos dev real[n_frames][R][n][3] ->
 * out dev double[n_frames][R][n_pull]; the same centre-of-mass kernel and the same evaluation as the kick.
 * mythos_martini_langevin_n_pull: coordinates of the installed set (0 without one).
 * Streams: set_restraints synchronises the device before the set is replaced; eval_external and pull_values are asynchronous
 * on the stream (their scratch belongs to the integrator: one call at a time per integrator; a call that needs more of it
 * than any before reallocates it, which waits for the device). */
int mythos_martini_restraints_check(int n, int n_rep, int n_posres, const int32_t* pr_index, const double* pr_k, const double* pr_ref,
                                    int n_flat, const int32_t* fb_index, const int32_t* fb_flags, const double* fb_param, int n_groups,
                                    const int32_t* g_first, const int32_t* g_member, const int32_t* g_pbc_ref, int n_pull,
                                    const int32_t* p_flags, const int32_t* p_groups, const double* p_param, const double* boxes,
                                    int barostat, int exchange);
int mythos_martini_langevin_set_restraints(mythos_martini_sim_t* sim, int n_posres, const int32_t* pr_index, const double* pr_k,
                                           const double* pr_ref, int n_flat, const int32_t* fb_index, const int32_t* fb_flags,
                                           const double* fb_param, int n_groups, const int32_t* g_first, const int32_t* g_member,
                                           const int32_t* g_pbc_ref, int n_pull, const int32_t* p_flags, const int32_t* p_groups,
                                           const double* p_param, const double* boxes);
int mythos_martini_langevin_n_pull(const mythos_martini_sim_t* sim);
int mythos_martini_langevin_eval_external(mythos_martini_sim_t* sim, const void* pos, double step, void* force, double* energies,
                                          double* xi, mythos_stream_t stream);
int mythos_martini_langevin_pull_values(mythos_martini_sim_t* sim, const void* pos, int n_frames, double* out, mythos_stream_t stream);

/* ---- MARTINI ensemble: window exchange (Hamiltonian replica exchange between umbrella windows) -----------------------
 * A mode of its own beside temperature exchange: every replica at the SAME kT, the rungs are the parameter rows of the
 * installed set of restraints.
 *   Windows and slots  The window of rung w is the whole per-replica row set_restraints was given for replica w: pr_ref[w],
 *                    fb_param[w], p_param[w].  Slots are the replicas as they lie in memory and keep beads, velocities,
 *                    box, seed and kT.  window_of_slot is a permutation, the identity after set_restraints.  An accepted
 *                    exchange SWAPS THE TWO ROWS in device memory: slot s always runs under row s, and the step path and the
 *                    restraint kick are what they are without exchange.
 *   Energy           E_w(x_s, t): position + flat-bottom + umbrella + constant-force energy of the configuration of slot s,
 *                    in slot s's box, under window w, at t = step dt (moving windows included); sums in double.
 *   Event            every = E > 0: at the closed state of every absolute step that is a multiple of E.  Attempt a = step / E
 *                    tries the pairs of temperature exchange's schedule.  For slot A in window t and slot B in window t + 1
 *                        d = -(1 / kT) [ (E_t+1(x_A) + E_t(x_B)) - (E_t(x_A) + E_t+1(x_B)) ],   accept iff d >= 0 or u < exp(d),
 *                    u = (c[0] + 0.5) 2^-32 of Philox4x32-10 keyed by the 64-bit seed, counter {t, step lo, step hi, 6}.  The
 *                    physical energy cancels at equal kT: no energy row, no rescale.  One centre-of-mass launch, one
 *                    decision launch (a workgroup per pair), one synchronisation; the neighbour rows are dropped, so what
 *                    follows is bit for bit the run of an ensemble loaded with this state and set_restraints with these
 *                    rows.  A row saved at an event step is the state before the event.  every = 0 switches it off: the
 *                    handle then launches exactly what it launched before.
 * Refused by name (INVALID_ARGUMENT): n_rep < 2, every < 0, replicas whose kT differ, temperature exchange or a barostat in
 * either order of the two calls, a set whose pull vec or origin differ between replicas (windows may differ in k, init,
 * rate, position-restraint references and flat-bottom parameters; xi is then a function of the configuration alone), a
 * window_of_slot that is no permutation.  NOT_READY: advance with window exchange on and no set installed; set_windows on
 * an open resident frame or without a set.
 *   set_windows      window_of_slot host int32[n_rep]: permutes the rows from the current assignment to this one.
 *   get_windows      the current assignment.  set_restraints resets it to the identity and clears the counts.
 *   last_windows     host int32[*n_rows][n_rep]: window_of_slot at every row the last call saved, each before its event.
 *   last_window_exchanges  host double[*n][11], the last call's attempts in order: step, t, slot A, slot B, E_t(x_A),
 *                    E_t+1(x_A), E_t(x_B), E_t+1(x_B), d, u, accepted (0 | 1).  rec / rows NULL: the count alone.
 *   window_exchange_counts  host int64[n_rep - 1] each: attempts and acceptances per rung pair since set_restraints.
 * mythos_martini_window_exchange_check: the refusals that need no handle; kT host double[n_rep], p_param host
 * double[n_rep][n_pull][9] and window_of_slot may be NULL (not checked); temperature_exchange / barostat say whether one is
 * set; touches no device. */
int mythos_martini_window_exchange_check(int n_rep, int every, const double* kT, int temperature_exchange, int barostat, int n_pull,
                                         const double* p_param, const int32_t* window_of_slot);
int mythos_martini_langevin_set_window_exchange(mythos_martini_sim_t* sim, int every, uint64_t seed);
int mythos_martini_langevin_set_windows(mythos_martini_sim_t* sim, const int32_t* window_of_slot);
int mythos_martini_langevin_get_windows(const mythos_martini_sim_t* sim, int32_t* window_of_slot);
int mythos_martini_langevin_last_windows(const mythos_martini_sim_t* sim, int32_t* rows, int* n_rows);
int mythos_martini_langevin_last_window_exchanges(const mythos_martini_sim_t* sim, double* rec, int* n);
int mythos_martini_langevin_window_exchange_counts(const mythos_martini_sim_t* sim, int64_t* attempts, int64_t* accepts);

/* ---- MARTINI observables: named bond lengths and triplet angles ------------------------------
 * Replaces mythos/observables/bond_distances.py:15-17, 51-69 (BondDistances / BondDistancesMapped) and
 * triplet_angles.py:15-31, 73-92 (TripletAngles / TripletAnglesMapped) with the angle of
 * mythos/energy/martini/m2/angle.py:35-58 (atan2 of |cross| and dot of the unit vectors): one launch for every group
 * and every frame.  A group is all bonds, or all angles, that share one topology name.
 *   beads_per_item  host int32[n_groups]   2 = a group of bonds (i, j), 3 = a group of angles (i, j, k), angle at j
 *   members         host int32[n_groups]   items of each group
 *   index           host int32[...]        the bead indices of the groups one after the other, item-major
 *   pos, box        dev real[n_frames][n][3], dev real[n_frames][3] as for the MARTINI energy entry point; dtype is that of pos / box.
 *                   Only the per-frame orthorhombic periodic displacement exists (jax_md.space.periodic).
 *   out             dev double, group-major: group g occupies the (n_frames, members[g]) row-major block that starts
 *                   at n_frames * (members[0] + ... + members[g-1]).  Arithmetic is double for either dtype. */
typedef struct mythos_martini_obs mythos_martini_obs_t;
mythos_martini_obs_t* mythos_martini_obs_create(int n, int n_groups, const int32_t* beads_per_item, const int32_t* members,
                                                const int32_t* index, int device);
void mythos_martini_obs_destroy(mythos_martini_obs_t* obs);
/* items per frame = doubles per frame of the output */
int64_t mythos_martini_obs_count(const mythos_martini_obs_t* obs);
/* one launch over every group and frame, asynchronous on the stream */
int mythos_martini_obs_eval(mythos_martini_obs_t* obs, const void* pos, const void* box, int dtype, int n_frames, double* out,
                            mythos_stream_t stream);

/* ---- weighted 1-D Wasserstein distance ----------------------------------------------------------
 * Replaces wasserstein_1d and its callers (mythos/observables/wasserstein.py:42-78): W between the samples u of a group,
 * weighted per frame, and reference samples v.  The reference sorts u, v and their concatenation on every call and
 * differentiates through the sorts; here a plan is built once per stored trajectory from a merge order the caller
 * supplies (one stable sort of concat(u.flatten(), v) per group), and an evaluation is a prefix sum and, for the
 * gradient, a suffix sum over the plan (csrc/w1.hip).
 *   n_frames, members  host int32[n_groups]  group g has n_frames[g] x members[g] samples, frame-major
 *   samples       dev double   the groups' samples one after the other (with one n_frames: the layout of the observables entry point above)
 *   n_ref         host int64[n_groups];  ref dev double: the groups' reference samples one after the other
 *   ref_weights   dev double, same layout as ref, or NULL;  has_ref_weights host uint8[n_groups] or NULL: groups
 *                 without weights take 1 / n_ref (wasserstein.py:24-25).  Weights are masses: a negative or NaN
 *                 weight fails the call.
 *   order         dev int64, per group n_frames * members + n_ref indices into concat(u.flatten(), v) in ascending
 *                 order of the values.  Checked on the device for range and ascent, NOT for being a permutation: that
 *                 is the caller's duty (a duplicated index leaves the rank of the sample it displaced at entry 0 and
 *                 the gradient wrong, without an error; memory stays in bounds).  The call synchronises the stream.
 * The plan borrows nothing: samples, ref and order may be freed after the call.  It owns scratch for one evaluation at
 * a time (one plan per stream). */
typedef struct mythos_w1_plan mythos_w1_plan_t;
mythos_w1_plan_t* mythos_w1_plan_create(int n_groups, const int32_t* n_frames, const int32_t* members, const double* samples,
                                        const int64_t* n_ref, const double* ref, const double* ref_weights,
                                        const uint8_t* has_ref_weights, const int64_t* order, int device,
                                        mythos_stream_t stream);
void mythos_w1_plan_destroy(mythos_w1_plan_t* plan);
/* weights  dev double[n_frames] per-frame weights shared by all groups (a frame's weight is spread evenly over its
 *          members, wasserstein.py:75-77), or NULL for uniform 1 / (n_frames members); with weights every group has
 *          the same n_frames
 * w1       dev double[n_groups]
 * dw1_dweights  dev double[n_groups][max n_frames] or NULL: dW_g/dweights[s], with sign(0) = 0 where the reference
 *          differentiates jnp.abs.  Bitwise reproducible: fixed summation order, no atomics.
 * Asynchronous on the stream (mythos_w1_plan_create synchronises it: the order is checked on the device). */
int mythos_w1_eval(mythos_w1_plan_t* plan, const double* weights, double* w1, double* dw1_dweights, mythos_stream_t stream);

/* ---- membrane observables: leaflets, thickness, area per lipid ---------------------------------
 * One launch over the stored frames, one workgroup per frame (csrc/membrane.hip; definitions in DESIGN section 3.5c).
 * A lipid is a residue that owns beads of the lipid selection; its z is their unweighted mean, the midpoint is the mean
 * z of all the selection's beads, leaflet +1 is z_lipid > midpoint, -1 otherwise.  Positions in nm, as stored: no
 * re-wrapping in z.
 *   lipid_start  host int32[n_lipids + 1]  CSR offsets into lipid_beads, lipid_start[0] = 0, every lipid non-empty
 *   lipid_beads  host int32[lipid_start[n_lipids]]  the beads of the lipid selection, grouped by lipid
 *   thick_beads  host int32[n_thick]  the beads of the thickness selection (n_thick = 0: area per lipid only)
 *   thick_lipid  host int32[n_thick]  the lipid each of them belongs to */
#define MYTHOS_MEMBRANE_ROW 7 /* doubles per frame of mythos_membrane_eval's out */
typedef struct mythos_membrane mythos_membrane_t;
/* Replaces the constructors of lipyphilic.AssignLeaflets / MembThickness / AreaPerLipid in
 * mythos/observables/membrane_thickness.py:35-42 and area_per_lipid.py:33-40 (selections resolved by the caller). */
mythos_membrane_t* mythos_membrane_create(int n, int n_lipids, const int32_t* lipid_start, const int32_t* lipid_beads, int n_thick,
                                          const int32_t* thick_beads, const int32_t* thick_lipid, int device);
void mythos_membrane_destroy(mythos_membrane_t* mem);
/* Replaces the n_residues of the lipid selection's AtomGroup (mythos/observables/area_per_lipid.py:37-41, the axis the
 * mean runs over). */
int mythos_membrane_n_lipids(const mythos_membrane_t* mem);
/* Replaces the .run() calls and their results of mythos/observables/membrane_thickness.py:37-43 (leaflets.leaflets,
 * thicknesses.memb_thickness) and area_per_lipid.py:35-41 (mean over lipids of area_per_lipid.areas).
 *   pos, box  dev real[n_frames][n][3], dev real[n_frames][3]; dtype is that of both; promoted to double on load
 *   out       dev double[n_frames][MYTHOS_MEMBRANE_ROW]: thickness (nm; NaN if a leaflet has no lipid or no thickness
 *             bead), area per lipid Lx Ly (occupied leaflets) / n_lipids (nm^2), midpoint z, lipids in leaflet +1,
 *             lipids in leaflet -1, mean z of the thickness beads of leaflet +1, of leaflet -1 (NaN if none)
 *   leaflets  dev int8[n_frames][n_lipids] (+1 / -1) or NULL
 * Double sums in a fixed order, no atomics: a frame's row has the same bits whatever else is in the launch.  Asynchronous on
 * the stream. */
int mythos_membrane_eval(mythos_membrane_t* mem, const void* pos, const void* box, int dtype, int n_frames, double* out,
                         int8_t* leaflets, mythos_stream_t stream);

/* ---- duplex-mechanics observables: backbone distance, extension, twist, RMSD -------------------
 * What the reference's force-extension and stretch-torsion workflows measure per state, one launch over the stored
 * frames, one workgroup per frame (csrc/duplex_obs.hip).  Replaces the per-state parts of
 * mythos/observables/diameter.py:23-46, stretch_torsion.py:16-35 and 77-95, rmse.py:19-67.
 *   geometry, box   as mythos_observables_create (site offsets of the model; periodic box of the displacement, or NULL)
 *   base_pairs      host int32[n_bp][2]     hydrogen-bonded pairs of the backbone distance
 *   quartets        host int32[n_q][2][2]   adjacent base pairs ((a1, b1), (a2, b2)) of the twist
 *   end_pairs       host int32[4] a1, b1, a2, b2: the two base pairs of the extension, or NULL
 *   target_center   host double[n][3] target of the RMSD, CENTRED by the caller (rmse.py:110-113), or NULL
 * Output row per frame, MYTHOS_DUPLEX_ROW doubles, oxDNA length units and radians; a column that was not asked for
 * (empty list, NULL) is 0:
 *   [0] mean over base_pairs of the distance between the two backbone sites (diameter.py:37-41; sigma_backbone and the
 *       Angstrom factor are the caller's: they may carry a gradient)
 *   [1] |z| of disp(m2, m1), m = c_a + disp(c_b, c_a) / 2 of the two end pairs (stretch_torsion.py:84-95)
 *   [2] sum over quartets of acos(clamp(b1 . b2)), b = disp(base_b, base_a) with z dropped, then normalised
 *       (stretch_torsion.py:19-35); NaN if a pair's x-y projection vanishes, as the reference's division
 *   [3] sqrt(mean_i |R (x_i - mean x) - t_i|^2) with R the proper rotation that minimises it (rmse.py:29-47: SVD with
 *       the reflection fix; here Horn's quaternion by Jacobi sweeps, then a second pass over the residuals); raw
 *       coordinates, no minimum image (rmse.py:61-65)
 * center dev real[n_frames][n][3], quat dev real[n_frames][n][4] of precision dtype, read as they are; arithmetic in
 * double, sums in a fixed order, no atomics: a frame's row has the same bits whatever else is in the launch.
 * mythos_duplex_obs_eval is asynchronous on the stream. */
#define MYTHOS_DUPLEX_ROW 4
typedef struct mythos_duplex_obs mythos_duplex_obs_t;
mythos_duplex_obs_t* mythos_duplex_obs_create(int model, int n, const double* geometry, const double* box, int n_bp,
                                              const int32_t* base_pairs, int n_quartets, const int32_t* quartets,
                                              const int32_t* end_pairs, const double* target_center, int device);
void mythos_duplex_obs_destroy(mythos_duplex_obs_t* obs);
int mythos_duplex_obs_eval(mythos_duplex_obs_t* obs, const void* center, const void* quat, int dtype, int n_frames, double* out,
                           mythos_stream_t stream);

/* ---- radial distribution functions: pair-distance histograms of stored MARTINI frames ------------
 * The counts behind g(r) of pairs of bead selections, every frame and every pair of selections in one launch
 * (csrc/rdf.hip; definitions in DESIGN section 3.5m).  The reference has no such observable; the counting rule is that
 * of MDAnalysis' InterRDF with an exclusion block.
 *   n_a, n_b   host int32[n_groups]  beads in list A and list B of a group, each at least 1 and at most 2^22
 *   index      host int32[sum (n_a + n_b)]  the lists back to back: A_0 B_0 A_1 B_1 ...; A and B of a group may be the
 *              same list, disjoint or overlapping
 *   block      host int32[n] exclusion id of every bead - a pair of beads that share one is not counted - or NULL
 *   n_bins     1 ... 4096 bins of width r_max / n_bins on [0, r_max); r_max > 0, in the units of the positions
 *   dims       MYTHOS_RDF_XYZ, or MYTHOS_RDF_XY: distances and minimum image in x and y alone (lateral RDF of a membrane)
 * A group whose lists leave no admissible ordered pair is refused, as are indices outside [0, n). */
#define MYTHOS_RDF_XY 2
#define MYTHOS_RDF_XYZ 3
typedef struct mythos_rdf mythos_rdf_t;
mythos_rdf_t* mythos_rdf_create(int n, int n_groups, const int32_t* n_a, const int32_t* n_b, const int32_t* index,
                                const int32_t* block, int n_bins, double r_max, int dims, int device);
void mythos_rdf_destroy(mythos_rdf_t* rdf);
/* n_pairs host int64[n_groups]: the admissible ordered pairs (i in A, j in B) of each group - those with i != j and,
 * with blocks, block[i] != block[j] - the N_pairs of the normalisation g = counts V / (N_pairs v_bin). */
int mythos_rdf_n_pairs(const mythos_rdf_t* rdf, int64_t* n_pairs);
/*   pos, box  dev real[n_frames][n][3], dev real[n_frames][3]; dtype is that of both; promoted to double on load
 *   counts    dev int64[n_frames][n_groups][n_bins], zeroed by the call: +1 for every admissible ordered pair whose
 *             minimum-image distance r (per-frame orthorhombic box, masked dimensions only) is below r_max, in bin
 *             floor(r n_bins / r_max), at most n_bins - 1
 *   flags     dev int32[1]: -1, or the first frame with a box edge of a masked dimension below 2 r_max, where the
 *             minimum image no longer finds the closest pair (the counts of such a frame are not to be used)
 * Integer adds: the counts have the same bits from run to run.  Asynchronous on the stream (the counts are zeroed on it too). */
int mythos_rdf_eval(mythos_rdf_t* rdf, const void* pos, const void* box, int dtype, int n_frames, int64_t* counts,
                    int32_t* flags, mythos_stream_t stream);

/* ---- lateral pressure profile: the diagonal virial of stored MARTINI frames, resolved in slabs along z --------
 * Every frame of a trajectory in one call, on the tables, exclusions, incidence lists and charges the system handle holds
 * (csrc/stress_profile.hip; definitions in DESIGN section 3.5q).  The reference has no such observable.
 * Bead i of a frame gets a diagonal virial share w_i, the decomposition of mythos_martini_langevin_pressure term for term:
 * an LJ pair, a bond, a reaction-field pair and an excluded reaction-field pair give -1/2 (dV/dr) / r dx_d^2 to either bead,
 * an angle -u_d dU/dx_id to its first and -v_d dU/dx_kd to its last bead (nothing to its centre), over minimum-image
 * vectors; sum_i w_i is that entry point's W.  The share sits at the bead's own z (a Harasima-type contour): the lateral
 * components are what the profile is for, P_zz(z) of this contour is not constant in z and only its sum over the slabs is
 * physical.
 *   pos, box   dev real[n_frames][n][3], dev real[n_frames][3] of the SYSTEM's precision; every edge at least 2 r_cut
 *   n_bins     1 ... 1024 slabs of thickness lz / n_bins of the frame's own box
 *   center     host int32[n_center] beads, or n_center = 0.  Without: slab = min(n_bins - 1, floor(u n_bins)) with
 *              u = z / lz - floor(z / lz), fixed to the box.  With: mid = the mean stored z of those beads (the midpoint of
 *              mythos_membrane_eval, and as there wrong for a bilayer that lies across the z boundary),
 *              u = (z - mid) / lz - floor((z - mid) / lz + 1/2), slab = floor((u + 1/2) n_bins) clamped to [0, n_bins - 1]:
 *              slab n_bins / 2 starts at the midplane.  In double from positions promoted on load: an fp32 frame lands in
 *              the slabs of the fp64 call on the same values.
 *   out        dev double[n_frames][n_bins][MYTHOS_STRESS_ROW]: bead count, W_x, W_y, W_z (kJ/mol) of the slab; with by_term
 *              [MYTHOS_STRESS_ROW_BY_TERM]: count, then W_xyz of lj, bond, angle, coulomb (zero without charges).  The
 *              un-split W is ((lj + bond) + angle) + coulomb of those columns, bitwise.
 * The local pressure is P_d = (count kT + W_d) n_bins / (lx ly lz) x mythos_martini_bar_per_kj_mol_nm3() bar: stored frames
 * hold no velocities, the kinetic part is its equipartition value.  The caller forms it.
 * Sums inside a bead's tile of partners in the system's precision, everything behind in double, in a fixed order, no
 * atomics: a frame's row has the same bits alone, in any batch and call after call.  Does not synchronise, except where a
 * new centre list replaces the one of the call before.
 * Refused by name (INVALID_ARGUMENT): n_bins < 1 or > 1024, a centre index outside [0, n).
 * mythos_martini_stress_profile_check: those checks alone for n beads, plus - where boxes (HOST double[n_frames][3]) is given -
 * a box edge that is not positive and finite, or below 2 r_cut, naming the frame.  Touches no device. */
#define MYTHOS_STRESS_ROW 4
#define MYTHOS_STRESS_ROW_BY_TERM 13
double mythos_martini_bar_per_kj_mol_nm3(void);
int mythos_martini_stress_profile_check(int n, double r_cut, int n_frames, const double* boxes, int n_center, const int32_t* center,
                                        int n_bins);
int mythos_martini_stress_profile(mythos_martini_t* martini, const void* pos, const void* box, int n_frames, int n_center,
                                  const int32_t* center, int n_bins, int by_term, double* out, mythos_stream_t stream);

/* ---- MBAR: unbiasing weights of frames pooled from biased windows, and the sums behind a PMF --------
 * The binless multistate estimator (csrc/mbar.hip; definitions in DESIGN section 3.5o).  The reference has none.  N frames
 * are pooled from K windows, window k contributed n_k[k] >= 1 of them (sum = N); b_k(n) is the reduced bias of window k at
 * frame n.  One iteration is
 *     L_n = ln sum_j N_j exp(f_j - b_j(n)),    f_k' = f_k - ln(sum_n t_kn / N_k),  t_kn = N_k exp(f_k - b_k(n) - L_n)
 * re-gauged to f_0 = 0; the per-frame log-weights are -L_n.  All arithmetic is double; fixed summation order, no atomics:
 * the same bits from run to run.
 * The bias comes from one of two sources, whichever was set last:
 *   set_windows  the table path.  table host double[K][P][4] = kind (0 umbrella U = 1/2 k (xi - init)^2, 1 constant force
 *                U = k xi), k, init, rate of every window and coordinate - what p_flags bit 0 and p_param[.][.][0..2] of
 *                the restraints entry point hold for replica k; b_k(n) = sum_p U_kp(xi[n][p]) / kT.  kT host double[K], all
 *                equal.  xi dev double[N][P], BORROWED: it must stay alive and unchanged while the handle uses it.  The
 *                K x N matrix is never stored.
 *   set_matrix   the general path: u_kn dev double[K][N] row-major, BORROWED, any reduced energies (a temperature ladder's
 *                beta_k (U_n + p V_n), for instance).
 * Refused by name (INVALID_ARGUMENT): K < 1, N_k < 1, sum N_k != N, non-finite k or init, rate != 0 (moving windows are not
 * built), windows at different kT in the table path, K (3 P + 6) > 8192 (the table lives in 64 KB of LDS).
 * mythos_mbar_check: those checks alone, plus - where the pointers are given - non-finite xi (host double[N][P]) and
 * non-increasing or non-finite bin edges (host double[n_edges]); table, kT, xi and edges may be NULL.  Touches no device.
 * mythos_mbar_iterate: n_iter iterations queued on the stream without a synchronisation; f_inout dev double[K] is
 * advanced in place, delta_out dev double[1] receives max_k |f' - f| of the last one (NaN if the iteration diverged).
 * mythos_mbar_log_weights: log_weights dev double[N] = -L_n at the given f (dev double[K]).
 * mythos_mbar_binned_sum: order dev int64[N] the frames sorted by bin (a permutation: the caller's duty; memory stays in
 * bounds if it is not), seg_start dev int64[n_bins + 1] the bins' segments of it (frames outside every bin behind the
 * last), weights dev double[N] or NULL for 1.  sums dev double[n_bins + 1]: sum over the bin's frames of
 * weights[n] exp(log_weights[n] - shift), and in the last place the same sum over all N frames.
 * The window weights W_nk = exp(f_k - b_k(n) - L_n) = t_kn / N_k (N x K, never stored) enter two more entry points.  Both
 * take f dev double[K], queue the pass that makes L_n current at this f in front of their own kernels on the caller's
 * stream, work for either source, and do not synchronise (the first call allocates its partial sums on the handle).
 * mythos_mbar_gram: gram dev double[K][K] = the full, exactly symmetric G_ij = sum_n W_ni W_nj - the Hessian of a Newton
 * step is [diag(N_k s_k) - N_i N_j G_ij] / N, the estimator's asymptotic covariance a function of G -; colsum dev double[K]
 * = s_k = sum_n W_nk, or NULL.  Refused by name where the table rows of 128 windows leave no LDS for a strip of W (few
 * windows with some thousand coordinates each).
 * mythos_mbar_segment_moments: out dev double[n_seg][K], out[b][k] = sum over the frames n of segment b of v[n] W_nk;
 * order and seg_start (dev int64[N], dev int64[n_seg + 1]) as for mythos_mbar_binned_sum - an entry of order outside
 * [0, N) is skipped and never dereferenced -; order NULL: one segment (n_seg = 1) over all frames, seg_start unused.  v dev
 * double[N] or NULL for 1.  Refused: NULL handle or output, nothing set (NOT_READY), n_seg < 1 or > 2^20. */
typedef struct mythos_mbar mythos_mbar_t;
int mythos_mbar_check(int n_windows, int64_t n_frames, int n_coords, const double* table, const double* kT, const int64_t* n_k,
                      const double* xi, int n_edges, const double* edges);
mythos_mbar_t* mythos_mbar_create(int64_t n_frames, int n_windows, int device);
void mythos_mbar_destroy(mythos_mbar_t* mbar);
int mythos_mbar_set_windows(mythos_mbar_t* mbar, int n_coords, const double* table, const double* kT, const int64_t* n_k,
                            const double* xi);
int mythos_mbar_set_matrix(mythos_mbar_t* mbar, const double* u_kn, const int64_t* n_k);
int mythos_mbar_iterate(mythos_mbar_t* mbar, double* f_inout, int n_iter, double* delta_out, mythos_stream_t stream);
int mythos_mbar_log_weights(mythos_mbar_t* mbar, const double* f, double* log_weights, mythos_stream_t stream);
int mythos_mbar_binned_sum(mythos_mbar_t* mbar, int n_bins, const int64_t* seg_start, const int64_t* order, const double* log_weights,
                           const double* weights, double shift, double* sums, mythos_stream_t stream);
int mythos_mbar_gram(mythos_mbar_t* mbar, const double* f, double* gram, double* colsum, mythos_stream_t stream);
int mythos_mbar_segment_moments(mythos_mbar_t* mbar, const double* f, int n_seg, const int64_t* seg_start, const int64_t* order,
                                const double* v, double* out, mythos_stream_t stream);
/* The block bootstrap's weighted sums.  Replicate b = 0 ... n_boot - 1 weights frame n by the integer multiplicity
 * mult[b][n] (dev uint16[n_boot][N]) and is delta[b][k] = f_bk - f_hat[k] away from the solved f_hat (dev double[K],
 * dev double[n_boot][K]).  With t_jn = N_j W_nj at f_hat and D_bn = sum_j t_jn exp(delta_bj), the replicate's window weights are
 * W_bnk = W_nk exp(delta_bk) / D_bn and its frame weights exp(-L_n) / D_bn: the exponentials of a frame are formed once
 * for a tile of 32 replicates, W and D are never stored.  Both queue the L-pass at f_hat first, work for either source, do not
 * synchronise, and return the same bits call after call.
 * mythos_mbar_boot_colsums: out_s dev double[n_boot][K], s_bk = sum_n mult[b][n] W_bnk (1 at a replicate's solution).
 * mythos_mbar_boot_binned: out dev double[n_boot][n_seg][max(n_cols, 1)] = sum over the frames n of a segment of
 * mult[b][n] v[n][e] exp(-L_n - shift) / D_bn; v dev double[N][n_cols], or n_cols = 0 for 1; order and seg_start as for
 * mythos_mbar_segment_moments (order NULL: one segment over all frames).
 * Refused by name: n_boot < 1 or > 65 536, n_cols > 8, a non-finite shift, and K (3 P + 65) + 1 376 > 8 192 doubles (the
 * table, 32 rows of exp(delta) and a strip of 32 frames share 64 KB of LDS: about 100 windows of one coordinate). */
int mythos_mbar_boot_colsums(mythos_mbar_t* mbar, const double* f_hat, int n_boot, const double* delta, const uint16_t* mult,
                             double* out_s, mythos_stream_t stream);
int mythos_mbar_boot_binned(mythos_mbar_t* mbar, const double* f_hat, int n_boot, const double* delta, const uint16_t* mult, int n_seg,
                            const int64_t* seg_start, const int64_t* order, int n_cols, const double* v, double shift, double* out,
                            mythos_stream_t stream);

/* ---- time series: autocorrelation functions for the statistical inefficiency (csrc/timeseries.hip) --------
 * K series are the row segments offsets[k] ... offsets[k + 1] - 1 of x, dev double[n_rows][n_cols], time-ordered; every
 * column is a series of its own, T its length.  offsets is given twice, host int64[K + 1] (checked) and dev int64[K + 1].
 *     mu = mean x, v = mean (x - mu)^2, C(t) = sum_{i < T - t} (x_i - mu)(x_{i+t} - mu) / ((T - t) v)
 * mythos_timeseries_moments: mean and var, dev double[K][n_cols].
 * mythos_timeseries_autocorr: out dev double[K][n_cols][n_lags], out[k][e][j] = C(t0 + j); 0 where t0 + j >= T or v = 0.
 * Fixed summation order, no atomics: the same bits call after call.  Neither synchronises.
 * Refused by name (INVALID_ARGUMENT): n_cols < 1, offsets that do not increase from 0 to n_rows, n_lags < 1 or > 65 536.
 * mythos_timeseries_check: those checks alone, plus - where x (HOST double[n_rows][n_cols]) is given - non-finite values.
 * Touches no device. */
int mythos_timeseries_check(int64_t n_rows, int n_cols, int n_series, const int64_t* offsets, const double* x);
int mythos_timeseries_moments(const double* x, int64_t n_rows, int n_cols, int n_series, const int64_t* offsets,
                              const int64_t* offsets_dev, double* mean, double* var, int device, mythos_stream_t stream);
int mythos_timeseries_autocorr(const double* x, int64_t n_rows, int n_cols, int n_series, const int64_t* offsets,
                               const int64_t* offsets_dev, const double* mean, const double* var, int64_t t0, int n_lags,
                               double* out, int device, mythos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MYTHOS_HIP_H */
