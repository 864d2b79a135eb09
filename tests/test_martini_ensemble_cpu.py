"""What the MARTINI temperature ensemble refuses, checked without a device: mythos_martini_ensemble_check runs the checks
of mythos_martini_langevin_create_ensemble and of its load on host arguments alone, and MartiniEnsembleIntegrator's
argument helpers are plain functions."""

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.hip_system import MartiniEnsembleIntegrator as Ens

R_CUT, SKIN = 1.1, 0.25


def test_entry_points_exist():
    lib = _lib.load()
    for name in ("mythos_martini_langevin_create_ensemble", "mythos_martini_ensemble_check", "mythos_martini_langevin_n_replicas",
                 "mythos_martini_langevin_pressure_ensemble", "mythos_martini_langevin_get_box_ensemble"):
        assert hasattr(lib, name), name
    assert lib.mythos_martini_langevin_n_replicas(None) == -1


def test_what_passes():
    Ens.check(1280, [2.27, 2.5, 2.66], R_CUT, SKIN)
    Ens.check(1280, [2.27, 2.5], R_CUT, SKIN, boxes=[6.4, 6.5, 10.0])  # one box for every replica
    Ens.check(37, [2.0], R_CUT, SKIN, boxes=[[2.7, 3.0, 3.4]])         # an edge of exactly 2 (r_cut + skin)
    Ens.check((2**31 - 1) // 256 // 4, [1.0] * 4)                      # the last size the row store indexes


@pytest.mark.parametrize("kT,match", [([], "n_rep >= 1"), ([2.27, float("nan")], "kT of replica 1"), ([float("inf")], "kT of replica 0"),
                                      ([2.27, 2.5, 0.0], "kT of replica 2"), ([-1.0, 2.5], "kT of replica 0")])
def test_replica_count_and_temperatures(kT, match):
    with pytest.raises(ValueError, match=match):
        Ens.check(1280, kT, R_CUT, SKIN)


def test_more_rows_than_the_store_indexes():
    with pytest.raises(ValueError, match="4 replicas of 2097152 beads are more than the 8388607 rows"):
        Ens.check(2**21, [1.0] * 4)
    with pytest.raises(ValueError, match="at least one bead"):
        Ens.check(0, [1.0])


@pytest.mark.parametrize("bad,match", [([6.4, 6.5, 2.6], "replica 1: the box is smaller than twice"), ([6.4, 0.0, 10.0], "replica 1: invalid argument"),
                                       ([6.4, float("nan"), 10.0], "replica 1: invalid argument")])
def test_a_replica_box_the_single_copy_check_refuses(bad, match):
    boxes = np.array([[6.4, 6.5, 10.0], bad, [6.4, 6.5, 10.0]])
    with pytest.raises(ValueError, match=match):
        Ens.check(1280, [2.27, 2.5, 2.66], R_CUT, SKIN, boxes=boxes)


def test_box_shapes():
    b = Ens.replica_boxes([6.4, 6.5, 10.0], 3)
    assert b.shape == (3, 3) and b.flags["C_CONTIGUOUS"] and b.dtype == np.float64 and (b == [6.4, 6.5, 10.0]).all()
    b = Ens.replica_boxes(np.arange(6.0).reshape(2, 3), 2)
    assert b.shape == (2, 3)
    for wrong in (np.ones((2, 3)), np.ones((3, 2)), np.ones(4), 6.4):
        with pytest.raises(ValueError, match=r"box must have shape \(3, 3\)"):
            Ens.replica_boxes(wrong, 3)


# ---- HipMartiniSimulator: arguments and the lowering, no device ---------------------------------------------------------
def _bilayer_energy_fn():
    from mythos_amd.energy import martini as M
    from tests import martini_helpers as MH

    s = MH.system()
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    top = s["top"]
    fn = M.MartiniComposedEnergyFunction([
        M.LJ.from_topology(topology=top, params=M.LJConfiguration(**s["lj_params"])),
        M.Bond.from_topology(topology=top, params=M.BondConfiguration(**s["bond_params"])),
        M.Angle.from_topology(topology=top, params=M.AngleConfiguration(**ap))])
    return s, fn


def _sim_kwargs():
    from tests import martini_helpers as MH

    s, fn = _bilayer_energy_fn()
    x, box, _ = MH.frames("lj")
    return dict(energy_fn=fn, topology=s["top"], init_positions=x[3], box=box[3], temperatures=[273.0, 300.0, 320.0], simulation_steps=40,
                save_every=10, equilibration_steps=10)


def test_simulator_arguments():
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator, barostat_settings

    kw = _sim_kwargs()
    sim = HipMartiniSimulator(name="a", **kw)  # builds without a device
    assert sim.exposes() == ["trajectory.HipMartiniSimulator.a"] and sim.systems_created == 0
    x = np.asarray(kw["init_positions"])
    HipMartiniSimulator(**dict(kw, init_positions=np.broadcast_to(x, (3, 1280, 3))))
    HipMartiniSimulator(**dict(kw, temperatures=300.0))  # one temperature: R = 1
    HipMartiniSimulator(**dict(kw, box=np.broadcast_to(kw["box"], (3, 3))))
    with pytest.raises(ValueError, match=r"init_positions must have shape \(1280, 3\) or \(3, 1280, 3\) for 3 temperatures"):
        HipMartiniSimulator(**dict(kw, init_positions=np.broadcast_to(x, (2, 1280, 3))))
    with pytest.raises(ValueError, match="init_positions must have shape"):
        HipMartiniSimulator(**dict(kw, init_positions=x[:100]))
    for wrong in (np.ones((2, 3)), np.ones(4)):
        with pytest.raises(ValueError, match=r"box must have shape \(3, 3\)"):
            HipMartiniSimulator(**dict(kw, box=wrong))
    for temps in ([], [273.0, -1.0], [273.0, float("nan")]):
        with pytest.raises(ValueError, match="temperatures must be"):
            HipMartiniSimulator(**dict(kw, temperatures=temps))
    with pytest.raises(ValueError, match="multiple of save_every"):
        HipMartiniSimulator(**dict(kw, save_every=7))
    with pytest.raises(ValueError, match="precision"):
        HipMartiniSimulator(**dict(kw, precision="float16"))
    # save_every against the barostat's every: the single integrator serves any cadence, and so does the simulator
    for every in (1, 3, 10, 12):
        HipMartiniSimulator(**dict(kw, barostat=dict(kind="c-rescale", coupling="semiisotropic", compressibility=(3e-4, 0.0), every=every)))
    b = barostat_settings({"pcoupl": "C-rescale", "pcoupltype": "semiisotropic", "tau-p": "8.0", "compressibility": "3e-4 0.0",
                           "ref-p": "1.0 1.0", "nstpcouple": 10})
    assert b == dict(kind="c-rescale", coupling="semiisotropic", tau_p=8.0, compressibility=(3e-4, 0.0), ref_p=(1.0, 1.0), every=10)
    assert barostat_settings(None) is None and barostat_settings({"pcoupl": "no"}) is None
    for bad, match in (({"pcoupl": "parrinello-rahman"}, "not built"), ({"kind": "berendsen", "coupling": "anisotropic"}, "not built"),
                       ({"kind": "berendsen", "every": 0}, "every >= 1"), ({"kind": "berendsen", "tau": 1.0}, "unknown key")):
        with pytest.raises(ValueError, match=match):
            HipMartiniSimulator(**dict(kw, barostat=bad))


def test_lowering_follows_with_params_and_equals_the_terms_own_tables():
    from mythos_amd.simulators.hip_martini import lower_martini

    s, fn = _bilayer_energy_fn()
    base = lower_martini(fn)
    names = {"bond_k_DMPC_GL1_GL2": 1.3, "bond_r0_DMPC_NC3_PO4": 1.1, "angle_k_DMPC_PO4_GL1_GL2": 0.7}
    opt = {k: f * float((s["bond_params"] if k.startswith("bond") else s["angle_params"])[k]) for k, f in names.items()}
    new_fn = fn.with_params(opt)
    low = lower_martini(new_fn)
    lj, bond, angle = new_fn.energy_fns
    np.testing.assert_array_equal(low["types"], lj._tables()[0])
    np.testing.assert_array_equal(low["sigma"], lj._theta()[0].numpy())
    np.testing.assert_array_equal(low["eps"], lj._theta()[1].numpy())
    np.testing.assert_array_equal(low["bond_k"], bond._tables()[3])
    np.testing.assert_array_equal(low["bond_r0"], bond._tables()[4])
    np.testing.assert_array_equal(low["angle_k"], angle._tables()[5])
    np.testing.assert_array_equal(low["angle_t0"], angle._tables()[6])
    np.testing.assert_array_equal(low["bonds"], s["top"].bonded_neighbors)
    np.testing.assert_array_equal(low["angles"], s["top"].angles)
    assert low["angle_kind"] == 0 and low["charges"] is None
    top = s["top"]
    hit = np.array([n == "DMPC_GL1_GL2" for n in top.bond_names])
    assert hit.any() and np.array_equal(low["bond_k"][hit], 1.3 * base["bond_k"][hit]) and np.array_equal(low["bond_k"][~hit], base["bond_k"][~hit])
    hit = np.array([n == "DMPC_NC3_PO4" for n in top.bond_names])
    assert hit.any() and np.array_equal(low["bond_r0"][~hit], base["bond_r0"][~hit]) and not np.array_equal(low["bond_r0"][hit], base["bond_r0"][hit])
    hit = np.array([n == "DMPC_PO4_GL1_GL2" for n in top.angle_names])
    assert hit.any() and not np.array_equal(low["angle_k"][hit], base["angle_k"][hit]) and np.array_equal(low["angle_k"][~hit], base["angle_k"][~hit])
    for k in ("sigma", "eps", "angle_t0"):
        np.testing.assert_array_equal(low[k], base[k])
    # the reference values of the fixture, through the terms
    np.testing.assert_allclose(base["bond_k"], s["bond_k"])
    np.testing.assert_allclose(base["angle_t0"], s["angle_t0"])
    with pytest.raises(ValueError, match="lacks the terms"):
        lower_martini(type(fn)(fn.energy_fns[:2]))


def test_host_checks_and_npt_chunking_under_the_host_sanitizers(tmp_path):
    """tests/host/martini_ensemble_checks_main.cpp - a stand-alone program with its own main over
    mythos_amd/csrc/martini_ensemble_checks.h (the refusals) and mm_event_chunk of martini_exchange_checks.h with coupling
    events alone (the chunking of an advance under a barostat over R records per row) - built with -fsanitize=address,undefined and run: exit code 0, nothing reported."""
    import os
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "martini_ensemble_checks_san"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-I", str(root / "mythos_amd" / "csrc"),
                    str(root / "tests" / "host" / "martini_ensemble_checks_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok") and run.stderr == "", (run.stdout, run.stderr)
