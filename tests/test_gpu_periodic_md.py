"""The oxDNA step kernel (md_step_kernel, mythos_amd/csrc/langevin_step.h) and the integrator's own list builder
(build_rows_*_kernel, neighbors.hip; cell_of / cell_candidates, cell_list.h) in periodic boxes whose faces the strands
cross - the configurations of tests/oxdna_periodic_synth.py, which tests/test_oxdna_periodic_synth_cpu.py holds to what
is relied on here (the oracle is translation- and image-invariant to 1e-12; the lattices reach 3 x 10 x 3 cells and
the all-pairs builder; one listed pair in eleven needs an image unwrapped, thousands do folded, where the faces cut duplexes).

 1. six thermostatted fp64 steps of every crossing helix against LangevinOracle on the same Philox stream;
 2. one frictionless step from rest of the 576-nt lattices on the integrator's dynamic list, against oracle forces
    (boxed Verlet pairs), fp64 and every fp32 instantiation, unwrapped and folded coordinates;
 3. 60 steps on the dynamic list == 60 steps on a static all-pairs list, unwrapped == folded;
 4. a thin skin: halts, out-of-turn rebuilds and resumes across faces == the static list;
 5. a helix across three faces evolves like the same helix in the middle of the box (fp64 1e-9; fp32 within twice
    its own deviation from fp64);
 6. HipMDSimulator with space.periodic and a Verlet list: traced energies == energy_fn.map == the oracle.
"""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults
from mythos_amd.simulators.neighbors import verlet_pairs_numpy
from tests import helpers as H
from tests import oxdna_periodic_synth as S

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0
R_CUT, SKIN = S.R_CUT, S.SKIN


def _system(model, top, box, dtype, hce=False):
    from mythos_amd.hip_system import OxdnaSystem

    if model == 4:
        sim, cfg = defaults.default_configs_for("na1")
        flat = fp.pack_flat_na1(fp.derive_flat_na1(cfg["dna"], cfg["rna"], cfg["drh"], kt=sim["kT"], salt_conc=0.5, half_charged_ends=hce),
                                _lib.param_names())
        s = OxdnaSystem(4, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype, is_rna=S.is_rna(top))
    else:
        sim, cfg = defaults.default_configs_for(H.model_dir(model))
        flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=S.SALT[model], half_charged_ends=hce), _lib.param_names())
        s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype)
    s.set_params(torch.as_tensor(flat).detach())
    return s


def _oracle_params(model, hce=False):
    return H.oracle_params_na1(half_charged_ends=hce) if model == 4 else H.oracle_params(model, salt=S.SALT[model], half_charged_ends=hce)


def _dev(a, dtype, s):
    return torch.as_tensor(a, dtype=dtype, device=s.device).contiguous()


def _top_tensors(top, pairs):
    return (torch.as_tensor(top.seq, dtype=torch.long), torch.as_tensor(top.is_end, dtype=torch.long),
            torch.as_tensor(top.bonded_neighbors, dtype=torch.long).reshape(-1, 2), torch.as_tensor(pairs, dtype=torch.long).reshape(-1, 2))


def _mod_box(d, box):
    """d up to lattice vectors (the integrator never folds a centre; two runs may start in different images)."""
    return d - box * np.rint(d / box)


# ---------------------------------------------------------------------------------------------- 1
STEP_CASES = [(m, n, False) for m, n in S.CROSSING] + [(4, "simple-helix-dna-rna", True)]


@pytest.mark.parametrize(("model", "name", "unfused"), STEP_CASES)
def test_crossing_helix_steps_match_the_oracle_fp64(model, name, unfused, md_lanes):
    """The protocol and the tolerances of test_gpu_langevin.py::test_step_by_step_parity_with_oracle_fp64 on helices whose
    strands are images of each other across three faces: every pair between the strands - close radial pass, far pass,
    angular pass - and, in the ring, two bonded pairs go through the minimum image."""
    from mythos_amd.hip_system import LangevinIntegrator
    from oracle.langevin_oracle import LangevinOracle

    top, c0, q0, box = S.crossing_helix(model, name)
    s = _system(model, top, box, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    gam_t, gam_r = KT / 2.5, KT / 7.5
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=gam_t, gamma_r=gam_r, mass=1.0, inertia=(1.0, 1.3, 0.8), seed=0x1234ABCD5678)
    if unfused:
        integ.set_unfused()
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    n_steps = 6
    tc, tq, et = integ.run(c, q, p, L, n_steps, save_every=1)
    orc = LangevinOracle(model, _oracle_params(model), H.topo_tensors(top), box, 0.005, KT, gam_t, gam_r, 1.0, (1.0, 1.3, 0.8),
                         seed=0x1234ABCD5678, is_rna=S.is_rna(top) if model == 4 else None)
    worst = np.zeros(4)
    for k in range(n_steps):
        x, qq, pp, LL, u = orc.step(x, qq, pp, LL)
        ke_t, ke_r = orc.kinetic(pp, LL)
        worst = np.maximum(worst, [np.abs(tc[k].cpu().numpy() - x).max(), np.abs(tq[k].cpu().numpy() - qq).max(),
                                   abs(et[k, :8].sum().item() - u) / abs(u), abs(et[k, 8].item() - ke_t) / ke_t])
        print(f"{model} {name} step {k}: |dx| |dq| dU/U dK/K so far {worst}")
        np.testing.assert_allclose(tc[k].cpu().numpy(), x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(tq[k].cpu().numpy(), qq, rtol=0, atol=1e-10)
        assert abs(et[k, :8].sum().item() - u) < 1e-8 * abs(u)
        assert abs(et[k, 8].item() - ke_t) < 1e-9 * ke_t
        assert abs(et[k, 9].item() - ke_r) < 1e-9 * ke_r
    np.testing.assert_allclose(c.cpu().numpy(), x, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, atol=1e-9)
    assert integ.step == n_steps


# ---------------------------------------------------------------------------------------------- 2
DT1, INERTIA1 = 0.005, (1.0, 1.1, 0.9)


@functools.lru_cache(maxsize=None)
def _one_step_reference(box_x):
    """One frictionless step from rest of a lattice (the protocol of test_gpu_md_at_size.py's 12 kbp steps) with the
    forces and torques of the oracle over the Verlet pairs of the boxed configuration.  Computed once per box."""
    from oracle import oxdna_oracle as orc
    from oracle.langevin_oracle import drift

    top, c0, q0, box = S.duplex_lattice(box_x)
    c0 = c0.astype(np.float32).astype(np.float64)  # the configuration both precisions see
    q0 = q0.astype(np.float32).astype(np.float64)
    qn = q0 / np.linalg.norm(q0, axis=1, keepdims=True)  # the MD kernel normalises the quaternion on entry
    P = H.oracle_params(2, half_charged_ends=True)
    tt = _top_tensors(top, verlet_pairs_numpy(c0, top.bonded_neighbors, 3.9, box=box))

    def forces(x, q):
        _, gc, gq = orc.energy_and_grads(2, P, torch.as_tensor(x), torch.as_tensor(q), *tt, box=box)
        return -gc.numpy(), orc.quat_grad_to_body_torque(torch.as_tensor(q), gq).numpy()

    inertia = np.array(INERTIA1)
    F0, t0 = forces(c0, qn)
    p, L = 0.5 * DT1 * F0, 0.5 * DT1 * t0
    x, q, L = drift(c0, qn, p, L, 0.5 * DT1, 1.0, inertia)
    x, q, L = drift(x, q, p, L, 0.5 * DT1, 1.0, inertia)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    F1, t1 = forces(x, q)
    ref = {"top": top, "box": box, "c0": c0, "q0": q0, "qn": qn, "x": x, "q": q, "p": p + 0.5 * DT1 * F1, "L": L + 0.5 * DT1 * t1}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _one_step(ref, dtype, fold):
    from mythos_amd.hip_system import LangevinIntegrator

    top, box = ref["top"], ref["box"]
    start = S.wrapped(ref["c0"], box) if fold else ref["c0"]
    s = _system(2, top, box, dtype, hce=True)
    integ = LangevinIntegrator(s, dt=DT1, kT=KT, gamma_t=0.0, gamma_r=0.0, mass=1.0, inertia=INERTIA1, seed=1)
    integ.set_neighbor_policy(R_CUT, SKIN, 25)  # the integrator's own builder: cells at box_x = 13, all pairs at 11
    c, qd = _dev(start, dtype, s), _dev(ref["q0"], dtype, s)
    pz, Lz = torch.zeros_like(c), torch.zeros_like(c)
    integ.run(c, qd, pz, Lz, 1)
    assert integ.last_recoveries() == 0
    mx, mean = s.neighbor_stats()
    assert 1.0 < mean < 60.0, (mx, mean)  # a Verlet list (7 100 pairs within 3.9: at most 24.7 entries per row), not all pairs
    return start, c.cpu().double().numpy(), qd.cpu().double().numpy(), pz.cpu().double().numpy(), Lz.cpu().double().numpy()


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("box_x", [13.0, 11.0])
def test_lattice_fp64_step_on_the_dynamic_list_matches_oracle_forces(box_x, fold):
    """Tolerances of test_12kbp_fp64_step_matches_energy_kernel_forces: 1e-9 of the largest momentum, 1e-11 on the state."""
    ref = _one_step_reference(box_x)
    start, c, q, p, L = _one_step(ref, torch.float64, fold)
    for got, want in ((p, ref["p"]), (L, ref["L"])):
        print(f"box_x {box_x} fold {fold}: largest difference {np.abs(got - want).max():.2e} of {np.abs(want).max():.3g}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
    np.testing.assert_allclose(c - start, ref["x"] - ref["c0"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(q, ref["q"], rtol=0, atol=1e-11)


@pytest.mark.parametrize("dense", [0, 1, 2])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("box_x", [13.0, 11.0])
def test_lattice_fp32_step_on_the_dynamic_list_matches_oracle_forces(box_x, fold, dense):
    """Tolerances of test_12kbp_fp32_step_matches_energy_kernel_forces: per nucleotide 1e-3 of its own momentum plus 1e-3
    of the rms.  dense: the instantiation the grid size would choose, the fixed-row one and the DENSE one forced."""
    ref = _one_step_reference(box_x)
    _lib.debug_set("md_dense", dense)
    try:
        start, c, q, p, L = _one_step(ref, torch.float32, fold)
    finally:
        _lib.debug_set("md_dense", 0)
    for got, want in ((p, ref["p"]), (L, ref["L"])):
        rms = np.sqrt((want**2).mean())
        assert rms > 0.005 and np.abs(want).max() < 200 * rms  # there is something to compare, and no singular contact
        err = np.abs(got - want).max(1)
        bound = 1e-3 * (np.abs(want).max(1) + rms)
        print(f"box_x {box_x} fold {fold} dense {dense}: largest err / bound {np.max(err / bound):.3f}, rms {rms:.3g}")
        assert (err <= bound).all(), (err.max(), rms, np.abs(want).max())
    # positions moved by dt^2/2 F ~ 1e-4: the DISPLACEMENT, to the rounding of the caller's fp32 copy of the new centre -
    # 2e-6 where |coordinate| < 32 (the allowance of the 12 kbp test), four times that below 128, where an ulp is four
    # times as large (the unwrapped lattice reaches y = 72; folded, every coordinate is below 39)
    moved = ref["x"] - ref["c0"]
    for lim in (32.0, 128.0):
        near = np.abs(start).max(1) < lim
        assert near.sum() > (100 if fold or lim > 32.0 else -1)
        if near.any():
            assert np.abs((c - start)[near] - moved[near]).max() <= 1e-3 * np.abs(moved).max() + 2e-6 * lim / 32.0
    assert np.abs(q - ref["q"]).max() <= 1e-3 * np.abs(ref["q"] - ref["qn"]).max() + 3e-7


# ---------------------------------------------------------------------------------------------- 3, 4
def _run_lists(model, top, c0, q0, box, policy, n_steps, hce, dt=0.003):
    """The same run on a static list of every non-bonded pair and on the integrator's dynamic list with ``policy`` =
    (r_cut, skin, every): -> [(state vector, saved centres, saved energies, recoveries)] in that order."""
    from mythos_amd.hip_system import LangevinIntegrator

    out = []
    for dynamic in (False, True):
        s = _system(model, top, box, torch.float64, hce=hce)
        integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=99)
        if dynamic:
            integ.set_neighbor_policy(*policy)
        else:
            s.set_neighbors(top.unbonded_neighbors)
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = integ.init_momenta()
        tc, _, et = integ.run(c, q, p, L, n_steps, save_every=15)
        out.append(([t.cpu().numpy() for t in (c, q, p, L)], tc.cpu().numpy(), et.cpu().numpy(), integ.last_recoveries()))
        if dynamic:
            assert s.neighbor_stats()[1] < top.n_nucleotides - 3
    return out


def _assert_same_run(a, b, box=None, what=""):
    worst = max(np.abs(x - y).max() if box is None or k else np.abs(_mod_box(x - y, box)).max() for k, (x, y) in enumerate(zip(a[0], b[0])))
    print(f"{what}: largest difference of the final state {worst:.2e}")
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        d = x - y if (box is None or k) else _mod_box(x - y, box)
        np.testing.assert_allclose(d, 0.0, rtol=0, atol=1e-9)
    d = a[1] - b[1] if box is None else _mod_box(a[1] - b[1], box)
    np.testing.assert_allclose(d, 0.0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("box_x", [13.0, 11.0])
def test_dynamic_list_in_a_box_matches_static_all_pairs_unwrapped_and_folded(box_x):
    """test_gpu_langevin.py::test_dynamic_verlet_list_matches_static_all_pairs in a box: 60 thermostatted fp64 steps with
    a rebuild every 10, final state and the rows saved every 15 steps against the list of every non-bonded pair (1e-9);
    from unwrapped and from folded coordinates, which must agree with each other up to lattice vectors as well."""
    top, c0, q0, box = S.duplex_lattice(box_x)
    runs = {}
    for fold in (False, True):
        start = S.wrapped(c0, box) if fold else c0
        static, dynamic = _run_lists(2, top, start, q0, box, (R_CUT, SKIN, 10), 60, hce=True)
        assert static[3] == 0 and dynamic[3] == 0
        assert np.abs(static[1][-1] - start).max() > 0.02  # they moved
        _assert_same_run(static, dynamic, what=f"box_x {box_x} fold {fold} static / dynamic")
        runs[fold] = (static, dynamic)
    for k, kind in enumerate(("static", "dynamic")):
        _assert_same_run(runs[False][k], runs[True][k], box=box, what=f"box_x {box_x} {kind} unwrapped / folded")


@pytest.mark.parametrize("system", ["helix", "lattice", "lattice-folded"])
def test_a_site_leaving_its_skin_across_a_face_halts_rebuilds_and_resumes_exactly(system):
    """The skin-0.05 protocol of test_gpu_langevin.py::test_a_site_leaving_its_skin_halts_rebuilds_and_resumes_exactly (no
    scheduled rebuild in 90 steps: every rebuild is a halt at the state that left the skin) with its assertions, on the
    oxDNA2 helix across three faces (16 nt: the all-pairs builder with the minimum image) and the 3 x 10 x 3-cell lattice."""
    if system == "helix":
        top, c0, q0, box = S.crossing_helix(2, "simple-helix")
        hce, r_cut = False, 3.3
    else:
        top, c0, q0, box = S.duplex_lattice(13.0)
        c0 = S.wrapped(c0, box) if system == "lattice-folded" else c0
        hce, r_cut = True, R_CUT + SKIN - 0.05  # list range 3.85: the three cells along x and z
        assert S.cells_per_edge(box, r_cut + 0.05) == (3, 10, 3)
    static, dynamic = _run_lists(2, top, c0, q0, box, (r_cut, 0.05, 1000), 90, hce=hce)
    print(f"{system}: {dynamic[3]} recoveries")
    assert static[3] == 0 and 3 <= dynamic[3] <= 64, dynamic[3]
    assert static[1].shape[0] == 6
    _assert_same_run(static, dynamic, what=system)


# ---------------------------------------------------------------------------------------------- 5
def _placements():
    """A: the golden oxDNA2 frame, whole, in the middle of its box; B: the same frame across three faces with its second
    strand an image.  On the grid 2^-11, so both are exact in fp32."""
    top, c, q, box, move = S.placement(2, "simple-helix")
    grid = 2.0**-11
    c = np.round(c / grid) * grid
    return top, c, q, box, move


def _run_placement(top, c0, q0, box, dtype, n_steps=60):
    from mythos_amd.hip_system import LangevinIntegrator

    s = _system(2, top, box, dtype)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=9)
    c, q = _dev(c0, dtype, s), _dev(q0, dtype, s)
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, n_steps)
    return [t.cpu().double().numpy() for t in (c, q, p, L)]


def test_fp64_dynamics_are_invariant_under_lattice_translations():
    top, c0, q0, box, move = _placements()
    a = _run_placement(top, c0, q0, box, torch.float64)
    b = _run_placement(top, c0 + move, q0, box, torch.float64)
    assert np.abs(a[0] - c0).max() > 0.02
    print("A / B differences (x, q, p, L):", [float(np.abs(u - v).max()) for u, v in zip([a[0] + move] + a[1:], b)])
    np.testing.assert_allclose(b[0] - move, a[0], rtol=0, atol=1e-9)
    for u, v in zip(a[1:], b[1:]):
        np.testing.assert_allclose(v, u, rtol=0, atol=1e-9)


def test_fp32_dynamics_across_faces_are_as_accurate_as_in_the_middle_of_the_box():
    """60 steps in fp32 and in fp64 (the oracle's trajectory, test 1) from the same state and seed, in placement A and in
    placement B: B's fp32 momenta may deviate from B's fp64 momenta by at most twice what A's do from A's - the accuracy
    already accepted for fp32 is the measure, and the factor covers the rounding of d - L rint(d / L) at |d| ~ L (the hi + lo
    difference is exact, the product L rint() is exact, the subtraction rounds once more than in the middle of the box).
    Measured on an MI355X, fp32 - fp64 after 60 steps - linear momenta (largest 0.548): A 5.3e-06, B 6.8e-06; angular
    momenta (largest 0.74): A 1.167e-05, B 1.179e-05."""
    top, c0, q0, box, move = _placements()
    dev = {}
    for name, start in (("A", c0), ("B", c0 + move)):
        r64 = _run_placement(top, start, q0, box, torch.float64)
        r32 = _run_placement(top, start, q0, box, torch.float32)
        dev[name] = (np.abs(r32[2] - r64[2]).max(), np.abs(r32[3] - r64[3]).max())
        print(f"placement {name}: fp32 - fp64 momenta differ by {dev[name][0]:.3e} (linear, largest {np.abs(r64[2]).max():.3g}), "
              f"{dev[name][1]:.3e} (angular, largest {np.abs(r64[3]).max():.3g})")
    for k in range(2):
        assert dev["A"][k] > 0.0
        assert dev["B"][k] <= 2.0 * dev["A"][k], (k, dev)


# ---------------------------------------------------------------------------------------------- 6
def test_simulator_in_a_periodic_box_with_a_verlet_list_traces_the_energies_of_its_frames():
    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import Quaternion, RigidBody, space
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList
    from oracle import oxdna_oracle as orc

    top, c0, q0, box = S.crossing_helix(2, "simple-helix")
    disp, shift = space.periodic(box)
    ef = dna2.create_default_energy_fn(topology=top, displacement_fn=disp)
    dev = torch.device("cuda", 0)
    init = RigidBody(center=torch.as_tensor(c0, device=dev), orientation=Quaternion(vec=torch.as_tensor(q0, device=dev)))
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=0.005, kT=KT)
    sim = HipMDSimulator(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin, neighbors=VerletNeighborList(),
                         save_every=5, dtype=torch.float64, trace_energy=True)
    traj = sim.run({}, init, 20, key=17).observables[0]
    assert traj.center.shape == (4, top.n_nucleotides, 3)
    traced = traj.metadata["energy_terms"].sum(1).cpu().numpy()
    mapped = ef.map(RigidBody(traj.center, traj.orientation)).cpu().numpy()
    assert np.ptp(traced) > 1e-3  # the frames differ
    np.testing.assert_allclose(mapped, traced, rtol=1e-9, atol=0)
    u = orc.energy(2, H.oracle_params(2, half_charged_ends=True), traj.center[0].cpu(), traj.orientation.vec[0].cpu(), *H.topo_tensors(top), box).item()
    assert abs(mapped[0] - u) <= 1e-9 * abs(u) and abs(traced[0] - u) <= 1e-9 * abs(u), (mapped[0], traced[0], u)
