"""GPU tests through the reference-shaped Python surface.  They read like the reference's
mythos/energy/dna{1,2}/tests/test_integration.py: build each term with default parameters and a
periodic box of 20, ``energy_fn.map(states)``, divide by N, round to 6 decimals, compare with the
``split_energy.dat`` column."""

import numpy as np
import pytest
import torch

from mythos_amd.energy import dna1, dna2
from mythos_amd.energy.base import Quaternion, RigidBody, space
from mythos_amd.optimization import objective
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0


def _states(traj, dtype=torch.float64):
    dev = torch.device("cuda", 0)
    return RigidBody(
        center=torch.as_tensor(traj.center, dtype=dtype, device=dev),
        orientation=Quaternion(vec=torch.as_tensor(traj.quaternions, dtype=dtype, device=dev)),
    )


def _setup(model, name):
    top, traj, split, energy = H.load_golden(model, name)
    mod = dna1 if model == 1 else dna2
    displacement_fn, _ = space.periodic(20.0)
    return top, traj, split, energy, mod, mod.default_configs()[1], mod.default_transform_fn(), displacement_fn


TERM_CASES = [
    (2, "simple-helix", "Fene", "FeneConfiguration", "fene", {}),
    (2, "simple-helix", "BondedExcludedVolume", "BondedExcludedVolumeConfiguration", "bonded_excluded_volume", {}),
    (2, "simple-helix", "Stacking", "StackingConfiguration", "stacking", {"kt": KT}),
    (2, "simple-helix", "UnbondedExcludedVolume", "UnbondedExcludedVolumeConfiguration", "unbonded_excluded_volume", {}),
    (2, "simple-helix", "HydrogenBonding", "HydrogenBondingConfiguration", "hydrogen_bonding", {}),
    (2, "simple-helix", "CrossStacking", "CrossStackingConfiguration", "cross_stacking", {}),
    (2, "simple-coax", "CoaxialStacking", "CoaxialStackingConfiguration", "coaxial_stacking", {}),
    (2, "simple-helix", "Debye", "DebyeConfiguration", "debye", {"kt": KT, "salt_conc": 0.5, "half_charged_ends": False}),
    (1, "simple-helix", "Stacking", "StackingConfiguration", "stacking", {"kt": KT}),
    (1, "simple-coax", "CoaxialStacking", "CoaxialStackingConfiguration", "coaxial_stacking", {}),
    (1, "simple-helix", "HydrogenBonding", "HydrogenBondingConfiguration", "hydrogen_bonding", {}),
]


@pytest.mark.parametrize(("model", "name", "cls", "cfg_cls", "section", "extra"), TERM_CASES)
def test_single_term_matches_split_energy(model, name, cls, cfg_cls, section, extra):
    top, traj, split, _, mod, default_params, transform_fn, displacement_fn = _setup(model, name)
    energy_config = getattr(mod, cfg_cls)(**{**default_params[section], **extra})
    energy_fn = getattr(mod, cls)(
        displacement_fn=displacement_fn, transform_fn=transform_fn, topology=top, params=energy_config.init_params()
    )
    energy = energy_fn.map(_states(traj)).cpu().numpy()
    energy = np.around(energy / top.n_nucleotides, 6)
    np.testing.assert_allclose(energy, split[:, H.SPLIT_COLUMNS.index(section)], atol=H.TERM_ATOL[section])


@pytest.mark.parametrize(("model", "name", "hce"), [(1, "simple-helix", False), (2, "simple-helix", False), (2, "simple-helix-half-charged-ends", True)])
def test_total_energy_default_fn(model, name, hce):
    top, traj, _, energy, mod, _, _, displacement_fn = _setup(model, name)
    energy_fn = mod.create_default_energy_fn(top, displacement_fn)
    if model == 2:
        energy_fn = energy_fn.with_params(half_charged_ends=hce)
    states = _states(traj)
    e = energy_fn.map(states).cpu().numpy() / top.n_nucleotides
    np.testing.assert_allclose(e, energy, atol=1e-3 if model == 2 else 1e-4)
    terms = energy_fn.compute_terms(states)
    assert terms.shape == (100, len(energy_fn.energy_fns))
    np.testing.assert_allclose(terms.sum(1).cpu().numpy() / top.n_nucleotides, e, atol=1e-12)
    single = energy_fn(states[3])
    assert single.dim() == 0 and abs(single.item() / top.n_nucleotides - e[3]) < 1e-12


def test_kt_is_a_shared_parameter():
    """with_params(kt=...) reaches stacking and Debye (dna2/tests/test_integration.py:366-369)."""
    top, traj, _, _, mod, _, _, displacement_fn = _setup(2, "simple-helix")
    ef = mod.create_default_energy_fn(top, displacement_fn)
    st = _states(traj)[:2]
    a = ef.compute_terms(st)
    b = ef.with_params(kt=0.12).compute_terms(st)
    changed = (a - b).abs().max(0).values.cpu().numpy() > 1e-9
    assert changed.tolist() == [False, False, True, False, False, False, False, True]


def test_weights_and_term_selection():
    top, traj, _, _, mod, _, _, displacement_fn = _setup(2, "simple-helix")
    ef = mod.create_default_energy_fn(top, displacement_fn)
    st = _states(traj)[:3]
    terms = ef.compute_terms(st)
    w = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.0, 1.0, 1.0, 3.0], dtype=torch.float64)
    efw = ef.replace(weights=w)
    torch.testing.assert_close(efw(st).cpu(), (terms.cpu() * w).sum(1), rtol=1e-12, atol=1e-12)
    no_dh = ef.without_terms("Debye")
    torch.testing.assert_close(no_dh(st).cpu(), terms[:, :7].sum(1).cpu(), rtol=1e-12, atol=1e-12)


def test_autograd_positions_orientations_and_parameters():
    """torch.autograd through the HIP op == oracle autograd (stand-in for jax.grad), incl. term weights."""
    from oracle import oxdna_oracle as orc

    top, traj, _, _, mod, _, _, displacement_fn = _setup(2, "simple-helix")
    w = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.7, 1.0, 1.0, 3.0], dtype=torch.float64)
    ef = mod.create_default_energy_fn(top, displacement_fn).replace(weights=w)
    st = _states(traj)[7]
    c = st.center.clone().requires_grad_(True)
    q = st.orientation.vec.clone().requires_grad_(True)
    a_stack = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
    eps_hb = torch.tensor(1.0678, dtype=torch.float64, requires_grad=True)
    u = ef.with_params(a_stack=a_stack, eps_hb=eps_hb)(RigidBody(c, Quaternion(q)))
    gc, gq, ga, ge = torch.autograd.grad(u, (c, q, a_stack, eps_hb))
    # oracle with the same weights
    a2 = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
    e2 = torch.tensor(1.0678, dtype=torch.float64, requires_grad=True)
    P = H.oracle_params(2, overrides={"stacking": {"a_stack": a2}, "hydrogen_bonding": {"eps_hb": e2}}, half_charged_ends=True)
    seq, is_end, b, un = H.topo_tensors(top)
    c2 = torch.as_tensor(traj.center[7]).requires_grad_(True)
    q2 = torch.as_tensor(traj.quaternions[7]).requires_grad_(True)
    u2 = (orc.energy_terms(2, P, c2, q2, seq, is_end, b, un, box=traj.box_size) * w).sum()
    rc, rq, ra, re = torch.autograd.grad(u2, (c2, q2, a2, e2))
    assert abs(u.item() - u2.item()) < 1e-9 * abs(u2.item())
    assert (gc.cpu() - rc).abs().max() < 1e-7 * rc.abs().max()
    assert (gq.cpu() - rq).abs().max() < 1e-7 * rq.abs().max()
    assert abs(ga.item() - ra.item()) < 1e-7 * abs(ra.item())
    assert abs(ge.item() - re.item()) < 1e-7 * abs(re.item())


def test_difftre_loss_and_grad_matches_oracle():
    """compute_loss_and_grad (objective.py:235) on 20 golden frames vs the same math on oracle energies."""
    from oracle import oxdna_oracle as orc

    top, traj, _, _, mod, _, _, displacement_fn = _setup(2, "simple-helix")
    ef = mod.create_default_energy_fn(top, displacement_fn)
    frames = list(range(0, 100, 5))
    st = _states(traj)[frames]
    ref_e = ef.map(st).detach()
    target = torch.tensor(0.2, dtype=torch.float64)

    def observable(states):  # mean COM distance of the first base pair, per frame
        return (states.center[:, 0] - states.center[:, 15]).norm(dim=1).to(torch.float64)

    def loss_fn(states, weights, energy_fn, opt_params, observables):  # noqa: ARG001
        measured = (weights * observable(states)).sum()
        return (measured - target.to(measured.device)) ** 2, (measured, None)

    opt = {"eps_hb": 1.10, "a_stack": 6.2, "k_cross": 47.0}
    (loss, (neff, measured, new_e)), grads = objective.compute_loss_and_grad(opt, ef, 1.0 / KT, loss_fn, st, ref_e, [])
    assert 0.0 < float(neff) <= 1.0 and new_e.shape == (len(frames),)
    # oracle
    leaves = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in opt.items()}
    P = H.oracle_params(2, half_charged_ends=True, overrides={
        "hydrogen_bonding": {"eps_hb": leaves["eps_hb"]}, "stacking": {"a_stack": leaves["a_stack"]}, "cross_stacking": {"k_cross": leaves["k_cross"]}})
    seq, is_end, b, un = H.topo_tensors(top)
    es = torch.stack([
        orc.energy(2, P, torch.as_tensor(traj.center[f]), torch.as_tensor(traj.quaternions[f]), seq, is_end, b, un, box=traj.box_size)
        for f in frames
    ])
    w_o, _ = objective.compute_weights_and_neff(1.0 / KT, es, ref_e.cpu())
    obs = torch.as_tensor(np.linalg.norm(traj.center[frames, 0] - traj.center[frames, 15], axis=1))
    loss_o = ((w_o * obs).sum() - target) ** 2
    g_o = torch.autograd.grad(loss_o, list(leaves.values()))
    assert abs(loss.item() - loss_o.item()) < 1e-8 * max(1.0, abs(loss_o.item()))
    for k, g in zip(leaves, g_o):
        assert abs(grads[k].item() - g.item()) <= 1e-5 * max(abs(g.item()), 1e-8), (k, grads[k].item(), g.item())


def test_simulator_run_surface():
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import NoNeighborList, VerletNeighborList

    top, traj, _, _, mod, _, _, _ = _setup(2, "simple-helix")
    disp, shift = space.free()
    ef = mod.create_default_energy_fn(top, disp)
    params = StaticSimulatorParams(
        seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)),
        gamma=(KT / 2.5, KT / 7.5), bonded_neighbors=top.bonded_neighbors, checkpoint_every=0, dt=5e-3, kT=KT,
    )
    init = _states(traj, torch.float32)[0]
    for nb in (NoNeighborList(unbonded_nbrs=top.unbonded_neighbors), VerletNeighborList(3.25, 0.6, 20)):
        sim = HipMDSimulator(energy_fn=ef, simulator_params=params, space=(disp, shift), simulator_init=nvt_langevin, neighbors=nb,
                             trace_energy=True)
        assert sim.exposes()[0].startswith("trajectory.HipMDSimulator.")
        out = sim.run({"eps_hb": 1.05}, init, 50, key=3)
        tr = out.observables[0]
        assert tr.center.shape == (50, 16, 3) and tr.orientation.vec.shape == (50, 16, 4)
        assert tr.temperature.shape == (50,) and torch.allclose(tr.temperature, torch.full((50,), KT, dtype=torch.float64, device=tr.temperature.device))
        assert torch.isfinite(tr.center).all()
        assert tr.slice(slice(10, 20)).length() == 10
        # the stored frames are consistent with the energy function (same parameters)
        e_traj = ef.with_params(eps_hb=1.05).map(RigidBody(tr.center, tr.orientation))
        torch.testing.assert_close(e_traj.cpu(), tr.metadata["energy_terms"].sum(1).cpu(), rtol=2e-4, atol=1e-3)


def test_integrator_plug_has_the_reference_shape_and_equals_the_one_call_loop():
    """`init_fn, step_fn = simulator_init(energy_fn, shift_fn, dt=, kT=, gamma=)`; `state = init_fn(key, R, mass=)`;
    `state = step_fn(state)`; the loop reads `state.position` (mythos/simulators/jax_md/jaxmd.py:73-92, utils.py:19-28).
    Stepped that way, the states equal the rows of HipMDSimulator.run - the same loop in one call - bit for bit; a state is a
    value: stepping an older one again reproduces its successor."""
    from mythos_amd.simulators.hip_md import HipMDSimulator, NVTLangevinState, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import NoNeighborList

    top, traj, _, _, mod, _, _, _ = _setup(2, "simple-helix")
    disp, shift = space.free()
    ef = mod.create_default_energy_fn(top, disp)
    gamma = RigidBody(center=KT / 2.5, orientation=KT / 7.5)
    mass = RigidBody(center=1.0, orientation=(1.0, 1.0, 1.0))
    init = _states(traj, torch.float64)[0]
    for dtype in (torch.float64, torch.float32):
        plug = nvt_langevin(ef, shift, dt=5e-3, kT=KT, gamma=gamma, dtype=dtype)
        init_fn, step_fn = plug
        state = init_fn(11, init, mass=mass)
        assert isinstance(state, NVTLangevinState) and state.step == 0 and state.mass is mass
        torch.testing.assert_close(state.position.center.double().cpu(), init.center.cpu().double(), rtol=0, atol=1e-6 if dtype == torch.float32 else 0)
        states = [state]
        for _ in range(6):
            states.append(step_fn(states[-1]))
        assert [s.step for s in states] == list(range(7))
        sim = HipMDSimulator(energy_fn=ef, simulator_params=StaticSimulatorParams(seq=top.seq, mass=mass, gamma=gamma, bonded_neighbors=top.bonded_neighbors,
                                                                                  checkpoint_every=0, dt=5e-3, kT=KT),
                             space=(disp, shift), simulator_init=nvt_langevin, neighbors=NoNeighborList(unbonded_nbrs=top.unbonded_neighbors),
                             save_every=1, dtype=dtype)
        rows = sim.run({}, init, 6, key=11).observables[0]
        for k in range(6):
            assert torch.equal(states[k + 1].position.center, rows.center[k]), (dtype, k)
            assert torch.equal(states[k + 1].position.orientation.vec, rows.orientation.vec[k]), (dtype, k)
        # a state is a value: an older one can be stepped again (reloaded, its closing half kick and the next step's opening one
        # are then two roundings where the resident frames have one: equal to rounding, not to the bit)
        tol = dict(rtol=0, atol=1e-12) if dtype == torch.float64 else dict(rtol=0, atol=2e-5)
        again = step_fn(states[2])
        assert again.step == 3
        torch.testing.assert_close(again.position.center, states[3].position.center, **tol)
        torch.testing.assert_close(again.position.orientation.vec, states[3].position.orientation.vec, **tol)
        torch.testing.assert_close(again.momentum.center, states[3].momentum.center, **tol)
        torch.testing.assert_close(again.momentum.orientation, states[3].momentum.orientation, **tol)
        onward = step_fn(again)
        torch.testing.assert_close(onward.position.center, states[4].position.center, **tol)
        plug.close()
    with pytest.raises(NotImplementedError, match="energy function of this package"):
        nvt_langevin(lambda R, **kw: 0.0, shift, dt=5e-3, kT=KT, gamma=gamma)


def test_simulator_batches_independent_replicas_in_one_launch():
    """n_replicas copies of the system advance as one launch per step, far apart in free space.  Cold and frictionless
    (kT -> 0, gamma = 0) the copies follow the same deterministic trajectory as a single run; thermal, they stay where
    they were put relative to their own origin, decorrelate from each other, and hand back (R, n, .) states."""
    import dataclasses as dc

    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import NoNeighborList, VerletNeighborList

    top, traj, _, _, mod, _, _, _ = _setup(2, "simple-helix")
    disp, shift = space.free()
    ef = mod.create_default_energy_fn(top, disp)
    init = _states(traj, torch.float32)[0]
    cold = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(0.0, 0.0),
                                 bonded_neighbors=top.bonded_neighbors, checkpoint_every=0, dt=5e-3, kT=1e-14)
    for nb in (NoNeighborList(unbonded_nbrs=top.unbonded_neighbors), VerletNeighborList(3.25, 0.6, 20)):
        one = HipMDSimulator(energy_fn=ef, simulator_params=cold, space=(disp, shift), simulator_init=nvt_langevin, neighbors=nb,
                             save_every=10)
        ref = one.run({}, init, 60, key=5).observables[0].center  # (6, 16, 3)
        many = dc.replace(one, n_replicas=5)
        out = many.run({}, init, 60, key=5)
        got = out.observables[0].center
        assert got.shape == (5 * 6, 16, 3) and out.observables[0].orientation.vec.shape == (5 * 6, 16, 4)
        for r in range(5):
            torch.testing.assert_close(got[6 * r:6 * (r + 1)], ref, rtol=0, atol=2e-4)
        assert out.state["final_state"].center.shape == (5, 16, 3)
    warm = dc.replace(cold, kT=KT, gamma=(KT / 2.5, KT / 7.5))
    sim = HipMDSimulator(energy_fn=ef, simulator_params=warm, space=(disp, shift), simulator_init=nvt_langevin,
                         neighbors=VerletNeighborList(3.25, 0.6, 20), save_every=50, n_replicas=8)
    out = sim.run({}, init, 400, key=9)
    c = out.observables[0].center.reshape(8, 8, 16, 3)
    assert torch.isfinite(c).all()
    com = c.mean(dim=2)                                      # replicas sit at their own origin again
    assert (com - init.center.mean(0).to(com)).norm(dim=-1).max() < 3.0
    last = c[:, -1]
    assert (last[0] - last[1]).abs().max() > 1e-3            # different noise per replica
    e = ef.map(RigidBody(out.observables[0].center, out.observables[0].orientation))
    assert torch.isfinite(e).all() and e.shape == (64,)
    # the next run continues all replicas from where they are
    again = sim.run({}, **{k: out.state[k] for k in ("init_state", "key")}, n_steps=50)
    assert again.observables[0].center.shape == (8, 16, 3)
    # replicas need free space
    box_disp, box_shift = space.periodic(traj.box_size)
    with pytest.raises(ValueError, match="free space"):
        dc.replace(sim, energy_fn=mod.create_default_energy_fn(top, box_disp), space=(box_disp, box_shift)).run({}, init, 5, key=1)


def _helix_simulator(pairs, ef=None):
    """fp64 simulator of the 16-nt oxDNA2 helix on an explicit pair list, and its initial state."""
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import NoNeighborList

    top, traj, _, _, mod, _, _, _ = _setup(2, "simple-helix")
    disp, shift = space.free()
    params = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5),
                                   bonded_neighbors=top.bonded_neighbors, checkpoint_every=0, dt=5e-3, kT=KT)
    sim = HipMDSimulator(energy_fn=mod.create_default_energy_fn(top, disp) if ef is None else ef, simulator_params=params, space=(disp, shift),
                         simulator_init=nvt_langevin, neighbors=NoNeighborList(unbonded_nbrs=pairs), dtype=torch.float64)
    return sim, _states(traj)[0]


def _four_steps(sim, init):
    tr = sim.run({}, init, 4, key=7).observables[0]
    return tr.center, tr.orientation.vec


def test_equal_pair_lists_share_one_kept_entry():
    """The simulator keys an explicit pair list by content: a second, equal array finds the kept system and integrator."""
    pairs = np.array(H.load_golden(2, "simple-helix")[0].unbonded_neighbors)
    sim, init = _helix_simulator(pairs)
    _four_steps(sim, init)
    sim.neighbors.unbonded_nbrs = pairs.copy()
    second = _four_steps(sim, init)
    assert len(sim._resident) == 1
    fresh = _four_steps(_helix_simulator(pairs.copy())[0], init)
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1])


def test_pair_list_mutated_in_place_is_seen():
    """Base pair (3, 12) leaves the list in place (an entry past the last nucleotide is padding): the next run steps on the
    new list, not on the rows kept from the old one."""
    top = H.load_golden(2, "simple-helix")[0]
    pairs = np.array(top.unbonded_neighbors)
    sim, init = _helix_simulator(pairs)
    before = _four_steps(sim, init)
    drop = ((pairs[:, 0] == 3) & (pairs[:, 1] == 12)) | ((pairs[:, 0] == 12) & (pairs[:, 1] == 3))
    assert drop.sum() == 1
    pairs[drop] = top.n_nucleotides
    mutated = _four_steps(sim, init)
    fresh = _four_steps(_helix_simulator(pairs[~drop])[0], init)
    assert torch.equal(mutated[0], fresh[0]) and torch.equal(mutated[1], fresh[1])
    assert not torch.equal(mutated[0], before[0])


def test_simulator_refuses_a_repeated_term_before_any_launch():
    top, _, _, _, mod, _, _, _ = _setup(2, "simple-helix")
    ef = mod.create_default_energy_fn(top, space.free()[0])
    twice = ef + ef.energy_fns[2]
    sim, init = _helix_simulator(np.array(top.unbonded_neighbors), ef=twice)
    with pytest.raises(ValueError, match="appears twice"):
        sim.run({}, init, 4, key=7)
    assert sim._resident == {}


def test_sequence_dependent_energy_function_from_the_references_file():
    """The drop-in route to sequence-dependent weights, as a user of the reference takes it: `read_ss_weights(file)` into
    `with_params` of the default oxDNA2 energy function (mythos/input/sequence_dependence.py:12-51), evaluated with `map` over
    oxDNA's own sequence-dependent run (tests/golden/regr/simple-helix-oxdna2-ss): oxDNA's total per nucleotide, 25 frames."""
    from mythos_amd.energy import dna2
    from mythos_amd.input.sequence_dependence import read_ss_weights
    from tests import helpers as H

    top, traj, split, _ = H.load_regr("simple-helix-oxdna2-ss")
    disp, _ = space.periodic(traj.box_size)
    w = read_ss_weights(H.GOLDEN / "seq-specific" / "seq_oxdna2.txt")
    ef = dna2.create_default_energy_fn(top, disp).with_params(half_charged_ends=False, **w)
    body = RigidBody(center=torch.as_tensor(traj.center, device="cuda"), orientation=Quaternion(vec=torch.as_tensor(traj.quaternions, device="cuda")))
    e = ef.map(body).cpu().numpy() / top.n_nucleotides
    assert e.shape == (25,) and np.abs(e - split.sum(1)).max() <= 3e-5, np.abs(e - split.sum(1)).max()
    plain = dna2.create_default_energy_fn(top, disp).with_params(half_charged_ends=False).map(body).cpu().numpy() / top.n_nucleotides
    assert np.abs(plain - split.sum(1)).max() > 1e-3  # (the average-sequence model is a different function)


# ---- handle lifetime: an integrator may be destroyed after its system; close() is idempotent ------------------------
DEV = "cuda:0"


def _oxdna_pair():
    """A 16-nt oxDNA2 duplex (fp32) with its integrator, and the two steps every pair takes."""
    from mythos_amd import _lib
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem
    from mythos_amd.input import defaults
    from mythos_amd.utils import generators

    top, c0, q0 = generators.ideal_duplex(8, model=2, seed=3)
    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], half_charged_ends=False), _lib.param_names())
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, dtype=torch.float32, device=DEV)
    s.set_params(flat)
    integ = LangevinIntegrator(s, dt=sim["dt"], kT=sim["kT"], gamma_t=sim["kT"] / 2.5, gamma_r=sim["kT"] / 7.5, seed=11)
    integ.set_neighbor_policy(3.25, 0.3, 5)

    def two_steps():
        c, q = torch.tensor(c0, dtype=torch.float32, device=DEV), torch.tensor(q0, dtype=torch.float32, device=DEV)
        p, ang = integ.init_momenta()
        integ.run(c, q, p, ang, 2)
        return [t.cpu().numpy() for t in (c, q, p, ang)]

    return s, integ, two_steps


def _martini_pair():
    """Two bent four-bead chains (8 beads, two types, fp32) with their integrator, and the two steps every pair takes."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator, MartiniSystem

    x0 = np.array([[0.5 + 0.45 * k, 1.0 + 0.15 * (k % 2), 1.0 + 1.5 * c] for c in range(2) for k in range(4)])
    bonds = [(4 * c + k, 4 * c + k + 1) for c in range(2) for k in range(3)]
    angles = [(4 * c + k, 4 * c + k + 1, 4 * c + k + 2) for c in range(2) for k in range(2)]
    s = MartiniSystem([0, 1, 1, 0, 1, 0, 0, 1], np.array([[0.47, 0.43], [0.43, 0.47]]), np.array([[3.5, 2.7], [2.7, 4.5]]), bonds,
                      np.full(6, 1250.0), np.full(6, 0.47), angles, np.full(4, 25.0), np.full(4, 2.4), dtype=torch.float32, device=DEV)
    integ = MartiniLangevinIntegrator(s, dt=0.01, kT=2.27, gamma=1.0, seed=11)

    def two_steps():
        x = torch.tensor(x0, dtype=torch.float32, device=DEV)
        v = integ.init_velocities()
        integ.run(x, v, [4.0, 4.0, 4.0], 2)
        return [t.cpu().numpy() for t in (x, v)]

    return s, integ, two_steps


@pytest.mark.parametrize("make", [_oxdna_pair, _martini_pair], ids=["oxdna-16nt", "martini-8beads"])
def test_integrator_and_system_close_in_either_order(make):
    """The system closed before its integrator, then a fresh pair the other way round; a third pair with the same seed
    then reproduces the first pair's two steps bit for bit.  close() after close() does nothing."""
    s, integ, two_steps = make()
    first = two_steps()
    s.close()
    integ.close()
    s.close()
    integ.close()
    assert s._h is None and integ._h is None
    s, integ, two_steps = make()
    two_steps()
    integ.close()
    s.close()
    integ.close()
    s.close()
    s, integ, two_steps = make()
    third = two_steps()
    assert all(np.isfinite(a).all() for a in first) and not np.array_equal(first[0], first[0] * 0)
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()


def test_close_is_idempotent_for_every_handle_class():
    """Each class of mythos_amd that owns a handle of the C ABI: the second close() does not reach the library."""
    from mythos_amd import _lib
    from mythos_amd.observables.base import DuplexSet, ObservableSet
    from mythos_amd.observables.martini_geometry import GeometrySet
    from mythos_amd.observables.membrane import MembraneSet
    from mythos_amd.observables.wasserstein import W1Plan

    class Counting:
        def __init__(self, lib):
            self.lib, self.destroyed = lib, []

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if not name.endswith("_destroy"):
                return fn
            return lambda h: (self.destroyed.append(name), fn(h))[1]

    sx, ix, _ = _oxdna_pair()
    sm, im, _ = _martini_pair()
    samples = torch.tensor([0.3, 0.1, 0.2], dtype=torch.float64, device=DEV)
    handles = [ix, sx, im, sm,
               ObservableSet(16, 2, None, None, [[0, 15], [1, 14]], None, True, torch.float32, DEV),
               DuplexSet(16, 2, None, None, end_pairs=[0, 15, 7, 8], device=DEV),
               GeometrySet(8, [2, 3], [np.array([[0, 1], [2, 3]]), np.array([[0, 1, 2]])], DEV),
               MembraneSet(8, [0, 1, 2], [0, 4], [1, 5], [0, 1], DEV),
               W1Plan(samples, [3], [1], [torch.tensor([0.15, 0.25], dtype=torch.float64, device=DEV)], [None])]
    def below(c):  # every class under c, at any depth (the two observable sets and the two integrators share a private base)
        return {s for d in c.__subclasses__() for s in {d} | below(d)}

    owners = {c for c in below(_lib.Handle) if c.__module__.startswith("mythos_amd.") and not c.__name__.startswith("_")}
    assert {type(h) for h in handles} == owners and len(owners) == 9
    for h in handles:
        assert isinstance(h, _lib.Handle) and h._h
        spy = h._lib = Counting(h._lib)
        h.close()
        assert h._h is None and len(spy.destroyed) == 1, type(h).__name__
        h.close()
        h.__del__()
        assert len(spy.destroyed) == 1, type(h).__name__
