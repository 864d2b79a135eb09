"""CPU-side tests of the membrane observables: the NumPy restatement against the reference's known answers, residue
membership of the topology readers, the selection parser, argument errors that arrive before any device work, and the
sigmoid fit of the melting temperature with its implicit gradient."""

import dataclasses as dc

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy.base import Quaternion
from mythos_amd.input import gromacs
from mythos_amd.observables import (AreaPerLipid, MembraneMeltingTemp, MembraneThickness, apl_residual, calculate_apl,
                                    compute_membrane_tm, fit_apl_sigmoid, get_initial_guess)
from mythos_amd.observables import membrane as MB
from mythos_amd.observables import membrane_melting_temp as MT
from mythos_amd.simulators.io import SimulatorTrajectory
from tests import martini_helpers as MH
from tests import membrane_ref as R
from tests import membrane_synth as SY

# mythos/observables/tests/test_membrane_thickness.py:45-58 (Angstrom; lipid_sel "name GL1 GL2", thickness_sel "name PO4")
REF_THICKNESS = np.array([37.21121013, 36.94640994, 37.31411836, 37.03461868, 36.75582552, 36.76741627, 37.21104291, 36.92698368,
                          36.80011913, 36.98599377])
# mythos/observables/tests/test_area_per_lipid.py:45-47 (Angstrom^2; lipid_sel "name GL1 GL2")
REF_AREA = np.array([51.189245, 51.382128, 50.695458, 51.42874, 51.178519, 51.148737, 50.517493, 51.3376, 51.586332, 51.005933])
THICKNESS_ATOL = 1e-6  # the reference's own tolerance
AREA_ATOL = 2e-5       # values printed to six decimals from an fp32 pipeline; five times the measured 3.75e-6

# mythos/observables/tests/test_membrane_melting_temp.py:22-29
TRUE = (47.0, 0.01, 8.0, 0.3, 320.0)
TEMPS = np.linspace(290.0, 350.0, 13)
TRUE_APLS = calculate_apl(TEMPS, *TRUE)


# ---- 1. the restatement ---------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_known_answers():
    top = MH.system()["top"]
    x, box, _ = MH.frames("lj")
    out = R.membrane(x, box, top.residue_index, R.mask(top, ("GL1", "GL2")), R.mask(top, ("PO4",)))
    dt, da = np.abs(10.0 * out["thickness"] - REF_THICKNESS).max(), np.abs(100.0 * out["apl"] - REF_AREA).max()
    print(f"max |thickness - reference| = {dt:.3e} A, max |area - reference| = {da:.3e} A^2")
    assert dt <= THICKNESS_ATOL
    assert da <= AREA_ATOL
    assert np.all(out["n_up"] == 64) and np.all(out["n_lo"] == 64)
    assert np.abs(out["lipid_z"] - out["mid"][:, None]).min() > 0.5  # no lipid near the midpoint


# ---- 2. residue membership --------------------------------------------------------------------------------------------
def test_residue_index_of_the_readers():
    top = MH.system()["top"]
    r = np.asarray(top.residue_index)
    assert r.shape == (1280,) and np.all(np.diff(r) >= 0) and np.array_equal(np.bincount(r), np.full(128, 10))
    r2 = np.asarray(top.tile(2).residue_index)
    assert r2.shape == (2560,) and np.all(np.diff(r2) >= 0) and np.array_equal(np.bincount(r2), np.full(256, 10))
    tpr = gromacs.MartiniTopology.from_tpr(MH.MG / "m3" / "angle" / "test.tpr")
    rt = np.asarray(tpr.residue_index)
    assert rt.shape == (len(tpr.atom_names),) and rt[0] == 0 and np.all(np.diff(rt) >= 0) and np.all(np.diff(rt) <= 1)
    beads_of = {}
    for res in range(int(rt[-1]) + 1):
        idx = np.flatnonzero(rt == res)
        names = {tpr.residue_names[i] for i in idx}
        assert len(names) == 1
        beads_of.setdefault(names.pop(), set()).add(tuple(tpr.atom_names[i] for i in idx))
    assert len(beads_of) >= 2 and all(len(v) == 1 for v in beads_of.values()), {k: len(v) for k, v in beads_of.items()}


def test_a_topology_without_residue_index_is_refused():
    top = dc.replace(MH.system()["top"], residue_index=None)
    old_style = gromacs.MartiniTopology(top.atom_types, top.atom_names, top.residue_names, top.angles, top.bonded_neighbors)
    assert old_style.residue_index is None
    x, box, _ = MH.frames("lj")
    traj = _cpu_traj(x, box)
    with pytest.raises(ValueError, match="residue_index"):
        MembraneThickness(topology=old_style, lipid_sel="name GL1 GL2", thickness_sel="name PO4")(traj)
    with pytest.raises(ValueError, match="residue_index"):
        AreaPerLipid(topology=top, lipid_sel="name GL1 GL2")(traj)


# ---- 3. selections ----------------------------------------------------------------------------------------------------
def test_selection_parser():
    top = SY.get("no_thickness_bead")["top"]  # LIP x4 (ten beads), ONE x2 (GL1), W
    names, res = np.asarray(top.atom_names), np.asarray(top.residue_names)
    assert np.array_equal(MB.select(top, "name GL1 GL2"), np.isin(names, ["GL1", "GL2"]))
    assert np.array_equal(MB.select(top, "resname LIP"), res == "LIP")
    assert np.array_equal(MB.select(top, "resname LIP ONE and name GL1"), names == "GL1")
    assert np.array_equal(MB.select(top, "name GL1 and resname ONE"), (names == "GL1") & (res == "ONE"))
    assert np.array_equal(MB.select(top, ("GL1", "GL2")), np.isin(names, ["GL1", "GL2"]))
    for text, token in (("name GL1 or name GL2", "'or'"), ("not name PO4", "'not'"), ("resid 1:5", "'resid'"), ("name GL*", r"'GL\*'"),
                        ("name GL1 and around 5 name PO4", "'around'"), ("(name GL1)", r"'\(name'"), ("name GL1 name GL2", "'name'")):
        with pytest.raises(ValueError, match="unsupported token " + token):
            MB.select(top, text)
    for empty in ("name XYZ", "resname ONE and name PO4", ("XYZ",)):
        with pytest.raises(ValueError, match="matches no bead"):
            MB.select(top, empty)
    with pytest.raises(ValueError, match="expected 'name A B"):
        MB.select(top, "name GL1 and")


def test_lipids_and_the_stray_thickness_bead():
    d = SY.get("no_thickness_bead")
    top = d["top"]
    obs = MembraneThickness(topology=top, lipid_sel="name GL1 GL2", thickness_sel="name PO4")
    assert np.array_equal(obs.lipid_residues, [0, 1, 2, 3, 4, 5])
    residues, start, sel, thick, thick_lipid = obs.index_lists()
    assert np.array_equal(start, [0, 2, 3, 5, 6, 8, 10]) and np.array_equal(sel, [2, 3, 10, 13, 14, 21, 24, 25, 34, 35])
    assert np.array_equal(thick, [1, 12, 23, 33]) and np.array_equal(thick_lipid, [0, 2, 4, 5])
    assert np.array_equal(AreaPerLipid(topology=top, lipid_sel="resname ONE and name GL1").lipid_residues, [1, 3])
    # W beads (residue 6, beads 42-44) belong to no lipid of "name GL1 GL2": the first of them is named
    with pytest.raises(ValueError, match=r"thickness_sel bead 42 \(W W, residue 6\)"):
        MembraneThickness(topology=top, lipid_sel="name GL1 GL2", thickness_sel="name PO4 W").index_lists()


# ---- 4. argument errors before any device work ------------------------------------------------------------------------
def _cpu_traj(x, box):
    q = torch.zeros((x.shape[0], x.shape[1], 4), dtype=torch.float64)
    q[..., 0] = 1.0
    return SimulatorTrajectory(center=torch.as_tensor(x), orientation=Quaternion(vec=q), box_size=torch.as_tensor(box))


def test_argument_errors_arrive_before_any_device_work():
    d = SY.get("two")
    traj = _cpu_traj(d["x"], d["box"])
    for obs in (MembraneThickness(topology=d["top"], lipid_sel=d["lipid_sel"], thickness_sel=d["thickness_sel"]),
                AreaPerLipid(topology=d["top"], lipid_sel=d["lipid_sel"])):
        with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
            obs(traj)
        with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
            obs.leaflets(traj)
        with pytest.raises(ValueError, match="box_size"):
            obs(dc.replace(traj, box_size=None))
    tm = MembraneMeltingTemp(topology=d["top"], lipid_sel=d["lipid_sel"], temperatures=[300.0])
    with pytest.raises(ValueError, match="trajectory.temperature"):
        tm(traj)
    labelled = dc.replace(traj, temperature=torch.full((3,), 300.0, dtype=torch.float64))
    with pytest.raises(ValueError, match="No frames found for temperature 310.0"):
        MembraneMeltingTemp(topology=d["top"], lipid_sel=d["lipid_sel"], temperatures=[300.0, 310.0])(labelled)
    with pytest.raises(ValueError, match="box_size"):
        tm(dc.replace(labelled, box_size=None))
    with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
        tm(labelled)


def test_row_width_of_the_binding_is_that_of_the_header():
    """The Python side allocates (S, MEMBRANE_ROW) for a kernel that writes MYTHOS_MEMBRANE_ROW doubles per frame."""
    import re
    from pathlib import Path

    header = (Path(__file__).resolve().parent.parent / "include" / "mythos_hip.h").read_text()
    (width,) = re.findall(r"#define\s+MYTHOS_MEMBRANE_ROW\s+(\d+)", header)
    assert int(width) == _lib.MEMBRANE_ROW == 7


# ---- 5. the sigmoid fit -----------------------------------------------------------------------------------------------
def test_sigmoid_model_known_values():
    """test_membrane_melting_temp.py:63-111."""
    assert abs(calculate_apl(320.0, *TRUE).item() - (47.0 + 3.2 + 4.0)) <= 1e-10
    assert abs(calculate_apl(200.0, *TRUE).item() - (47.0 + 2.0)) <= 1e-4
    assert abs(calculate_apl(500.0, *TRUE).item() - (47.0 + 5.0 + 8.0)) <= 1e-4
    assert TRUE_APLS.shape == (13,)
    assert apl_residual(torch.tensor(TRUE, dtype=torch.float64), (TRUE_APLS, TEMPS)).abs().max().item() <= 1e-10
    guess = get_initial_guess(TRUE_APLS, TEMPS)
    assert guess.shape == (5,) and 290.0 <= guess[4].item() <= 350.0 and guess[2].item() > 0 and guess[3].item() == 1.0
    # the literal 1 / (1 + exp(-k (T - Tm))) overflows at the guess's k = 1 in fp32 and saturates in fp64; sigmoid does not
    assert torch.isfinite(calculate_apl(np.array([-1e4, 1e4]), *guess.tolist())).all()


def test_fit_recovers_the_reference_known_answers():
    """test_membrane_melting_temp.py:117-138 and the five-temperature data of :213-259."""
    fitted = fit_apl_sigmoid(TRUE_APLS, TEMPS)
    print("13 temperatures:", fitted.tolist())
    assert abs(fitted[4].item() - 320.0) <= 0.5 and abs(fitted[2].item() - 8.0) <= 0.5
    assert apl_residual(fitted, (TRUE_APLS, TEMPS)).abs().max().item() < 0.01
    assert abs(compute_membrane_tm(TRUE_APLS, TEMPS).item() - 320.0) <= 0.5
    t5 = np.array([300.0, 310.0, 320.0, 330.0, 340.0])
    tm5 = compute_membrane_tm(calculate_apl(t5, *TRUE), t5)
    print("5 temperatures: Tm", tm5.item())
    assert abs(tm5.item() - 320.0) <= 0.5


def test_implicit_gradient_matches_central_differences_off_a_zero_residual_fit():
    """13 temperatures plus noise of sigma = 0.05 (seed 0): the fitted residuals do not vanish, so the Gauss-Newton J^T J
    is not the Hessian.  dTm/dareas (values of order 1) against central differences of the fit, h = 1e-5, within 2e-4.
    Measured: full-Hessian implicit gradient 3.0e-9 from the differences, Gauss-Newton 6.0e-3."""
    noisy = TRUE_APLS + torch.as_tensor(np.random.default_rng(0).normal(0.0, 0.05, size=13))
    y = noisy.clone().requires_grad_(True)
    tm = compute_membrane_tm(y, TEMPS)
    (g,) = torch.autograd.grad(tm, y)
    assert apl_residual(fit_apl_sigmoid(noisy, TEMPS), (noisy, TEMPS)).abs().max().item() > 0.01  # a non-zero residual
    h, fd = 1e-5, np.zeros(13)
    for i in range(13):
        e = torch.zeros(13, dtype=torch.float64)
        e[i] = h
        fd[i] = (compute_membrane_tm(noisy + e, TEMPS).item() - compute_membrane_tm(noisy - e, TEMPS).item()) / (2 * h)
    p = fit_apl_sigmoid(noisy, TEMPS).numpy()
    _, jac = MT._model_and_jacobian(p, TEMPS)
    gauss_newton = jac @ np.linalg.solve(jac.T @ jac, np.eye(5)[4])
    d_full, d_gn = np.abs(g.numpy() - fd).max(), np.abs(gauss_newton - fd).max()
    print(f"max |dTm/dy - central differences|: full Hessian {d_full:.3e}, Gauss-Newton {d_gn:.3e}; max |dTm/dy| {np.abs(fd).max():.3f}")
    assert 0.5 < np.abs(fd).max() < 5.0
    assert d_full <= 2e-4
    assert d_gn > 2e-4  # what the full Hessian is for
    # without implicit differentiation there is no gradient to hand out: refused, not silently dropped
    with pytest.raises(ValueError, match="implicit_diff=False"):
        compute_membrane_tm(y, TEMPS, implicit_diff=False)
    assert compute_membrane_tm(noisy, TEMPS, implicit_diff=False).item() == tm.item()
