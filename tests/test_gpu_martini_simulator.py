"""GPU tests of HipMartiniSimulator (mythos_amd/simulators/hip_martini.py) on the DMPC bilayer fixture: three temperatures,
10 equilibration + 40 production steps, rows every 10, stochastic cell rescaling with the md.mdp's coupling type,
compressibility, reference pressure and tau-p."""

import functools

import numpy as np
import pytest
import torch

from mythos_amd.energy import martini as M
from tests import martini_helpers as MH

pytestmark = pytest.mark.gpu

KB = 0.0083144626
TEMPS = [273.0, 300.0, 320.0]
# data/templates/martini/m2/DMPC/273K/md.mdp: pcoupltype = semiisotropic, tau-p = 8.0, compressibility = 3e-4 0.0, ref-p = 1.0 1.0
# (its pcoupl, Parrinello-Rahman, is not built: c-rescale stands in), given here as the file's own keys and strings
MDP = {"pcoupl": "c-rescale", "pcoupltype": "semiisotropic", "tau-p": "8.0", "compressibility": "3e-4 0.0", "ref-p": "1.0 1.0", "nstpcouple": 10}
OPT = "bond_k_DMPC_GL1_GL2"


def _energy_fn(s):
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    top = s["top"]
    return M.MartiniComposedEnergyFunction([
        M.LJ.from_topology(topology=top, params=M.LJConfiguration(**s["lj_params"])),
        M.Bond.from_topology(topology=top, params=M.BondConfiguration(**s["bond_params"])),
        M.Angle.from_topology(topology=top, params=M.AngleConfiguration(**ap))])


def _simulator(**over):
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator

    s = MH.system()
    x, box, _ = MH.frames("lj")
    kw = dict(energy_fn=_energy_fn(s), topology=s["top"], init_positions=x[3], box=box[3], temperatures=TEMPS, dt=0.02, gamma=1.0,
              equilibration_steps=10, simulation_steps=40, save_every=10, neighbors=(0.4, 5), barostat=MDP, precision="float32", name="bilayer")
    kw.update(over)
    return HipMartiniSimulator(**kw)


@functools.lru_cache(maxsize=None)
def _first_run():
    sim = _simulator()
    return sim, sim.run({}, seed=5)


def test_three_trajectories_of_four_frames_with_temperature_and_boxes():
    sim, out = _first_run()
    s = MH.system()
    assert sim.exposes() == ["trajectory.HipMartiniSimulator.bilayer"]
    assert len(out.observables) == 3
    for t, traj in zip(TEMPS, out.observables):
        assert traj.center.shape == (4, 1280, 3) and traj.center.is_cuda and traj.center.dtype == torch.float32
        assert traj.box_size.shape == (4, 3) and traj.box_size.dtype == torch.float64
        assert torch.equal(traj.temperature.cpu(), torch.full((4,), KB * t, dtype=torch.float64))
        assert torch.isfinite(traj.center).all()
    st = out.state
    assert st["positions"].shape == (3, 1280, 3) and st["velocities"].shape == (3, 1280, 3) and st["boxes"].shape == (3, 3) and st["seed"] == 8
    assert len(s["types"]) == 1280


def test_frames_are_those_of_the_ensemble_driven_by_hand():
    """The same lowering, seeds 5, 6, 7, policy and barostat through MartiniEnsembleIntegrator directly: frames, boxes
    (last_boxes) and the final state bitwise."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniSystem
    from mythos_amd.simulators.hip_martini import lower_martini

    _, out = _first_run()
    s = MH.system()
    x, box, _ = MH.frames("lj")
    low = lower_martini(_energy_fn(s))
    sysm = MartiniSystem(low["types"], low["sigma"], low["eps"], low["bonds"], low["bond_k"], low["bond_r0"], low["angles"], low["angle_k"],
                         low["angle_t0"], angle_kind=low["angle_kind"], dtype=torch.float32)
    integ = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=KB * np.array(TEMPS), gamma=1.0, seeds=5)
    integ.set_neighbor_policy(0.4, 5)
    integ.set_barostat("c-rescale", "semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 0.0), tau_p=8.0, every=10)
    pos = torch.tensor(np.broadcast_to(x[3], (3, 1280, 3)).copy(), dtype=torch.float32, device=sysm.device)
    vel = integ.init_velocities()
    integ.load(pos, vel, box[3])
    integ.advance(10)
    traj, _ = integ.advance(40, save_every=10, want_energy=False)
    lb = integ.last_boxes
    integ.store(pos, vel)
    for r, tr in enumerate(out.observables):
        assert torch.equal(tr.center, traj[:, r]), r
        assert torch.equal(tr.box_size, lb[:, r]), r
    assert torch.equal(out.state["positions"], pos) and torch.equal(out.state["velocities"], vel)
    np.testing.assert_array_equal(out.state["boxes"], integ.box)
    b = lb[-1].cpu().numpy()
    assert not np.array_equal(b[0], b[1]) and not np.array_equal(b[1], b[2])  # every temperature its own box
    assert (b[:, 2] == box[3][2]).all()  # compressibility_z = 0


def test_area_per_lipid_and_the_melting_temperature_grouping():
    """AreaPerLipid on the concatenation; the grouping of MembraneMeltingTemp (frames within temp_rtol of KB T) finds four
    frames per temperature.  The fit itself needs at least five temperatures and is not run."""
    from mythos_amd.observables import AreaPerLipid, MembraneMeltingTemp
    from mythos_amd.simulators.io import SimulatorTrajectory

    _, out = _first_run()
    top = MH.system()["top"]
    cat = SimulatorTrajectory.concat(out.observables)
    assert cat.center.shape == (12, 1280, 3) and cat.box_size.shape == (12, 3) and cat.temperature.shape == (12,)
    apl = AreaPerLipid(topology=top, lipid_sel="name GL1 GL2")(cat).cpu().numpy()
    area = (cat.box_size[:, 0] * cat.box_size[:, 1]).cpu().numpy()
    assert apl.shape == (12,) and np.isfinite(apl).all()
    np.testing.assert_allclose(apl, 100.0 * area / 64, rtol=0.1)
    tm = MembraneMeltingTemp(topology=top, lipid_sel="name GL1 GL2", temperatures=KB * np.array(TEMPS))
    frame_t = cat.temperature.cpu()
    for t in TEMPS:
        assert int(((frame_t - KB * t).abs() < tm.temp_rtol * KB * t).sum()) == 4


def test_a_second_run_with_other_parameters_reuses_the_handles():
    """run(opt_params) after run({}): no new system, the same integrator handle, and the frames of a fresh simulator that
    runs these parameters first - bitwise.  The parameters matter: the frames differ from the first run's."""
    sim, first = _first_run()
    s = MH.system()
    opt = {OPT: 1.3 * float(s["bond_params"][OPT])}
    handle = sim._resident["integrator"]
    again = sim.run(opt, seed=5)
    assert sim.systems_created == 1 and sim._resident["integrator"] is handle
    fresh_sim = _simulator()
    fresh = fresh_sim.run(opt, seed=5)
    assert fresh_sim.systems_created == 1
    for a, b, c in zip(again.observables, fresh.observables, first.observables):
        assert torch.equal(a.center, b.center) and torch.equal(a.box_size, b.box_size)
        assert not torch.equal(a.center, c.center)
    back = sim.run({}, seed=5)  # and back again: the first run's frames
    for a, c in zip(back.observables, first.observables):
        assert torch.equal(a.center, c.center) and torch.equal(a.box_size, c.box_size)
    assert sim.systems_created == 1
    fresh_sim.release()


def test_difftre_objective_over_the_three_trajectories_gives_finite_grads():
    from mythos_amd.observables import AreaPerLipid
    from mythos_amd.optimization import objective as O

    sim, out = _first_run()
    s = MH.system()
    apl = AreaPerLipid(topology=s["top"], lipid_sel="name GL1 GL2")

    def loss_fn(traj, weights, *_):
        expected = (weights * apl(traj)).sum() / weights.sum()
        loss = ((expected - 60.0) ** 2).sqrt()
        return loss, (("apl", expected), ())

    names = tuple(f"t{k}" for k in range(3))
    obj = O.DiffTReObjective(name="apl", required_observables=names, grad_or_loss_fn=loss_fn, energy_fn=sim.energy_fn, min_n_eff_factor=0.1)
    base = {OPT: float(s["bond_params"][OPT])}
    res = obj.calculate(dict(zip(names, out.observables)), opt_params={OPT: 1.002 * base[OPT]}, reference_opt_params=base)
    assert res.is_ready
    g = res.grads[OPT]
    print(f"  loss {float(res.observables['loss']):.6f}, d loss / d {OPT} = {float(g):.6e}")
    assert torch.isfinite(torch.as_tensor(g)).all() and torch.isfinite(torch.as_tensor(res.observables["loss"])).all()
