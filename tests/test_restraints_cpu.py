"""Restraints of the oxDNA Langevin integrator without a GPU: the NumPy reference of the three force laws
(tests/ext_field_ref.py) against its own definitions, the LAMMPS-input reader against the reference's stretch-torsion
input, and the index convention and units against the frames the reference holds for that input."""

import numpy as np
import pytest

from mythos_amd.input.lammps_restraints import read_lammps_restraints
from mythos_amd.simulators.restraints import GroupTorque, Restraints, SelfTether, SumRestraint
from tests import ext_field_ref as ref
from tests import helpers as H

LAMMPS_IN = H.GOLDEN / "regr" / "lammps-oxdna2-40bp" / "in"
K_LAMMPS, KT_LAMMPS = 1217.58, 0.1


def _numeric_gradient(u, x, h=1e-5):
    g = np.zeros_like(x)
    for i in range(x.shape[0]):
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, a] += h
            xm[i, a] -= h
            g[i, a] = (u(xp) - u(xm)) / (2 * h)
    return g


def test_tether_and_sum_forces_are_minus_the_gradient_of_their_energies():
    """rtol 1e-7.  U is quadratic, so the central difference has no truncation error; what it carries is the rounding of
    the two evaluations of U, each a sum of about 20 products and so good to 20 eps U at the worst, divided by 2 h:
    an absolute 20 eps U / h on every component, which counts on the components that are small."""
    rng = np.random.default_rng(0)
    x = rng.uniform(-3.0, 3.0, size=(9, 3))
    rs = Restraints(
        tethers=[SelfTether([0, 4], 3.5, rng.uniform(-3, 3, (2, 3)), (1, 1, 1)), SelfTether([7], 11.0, rng.uniform(-3, 3, (1, 3)), (1, 0, 1))],
        sums=[SumRestraint([1, 4, 5], 2.25, rng.uniform(-3, 3, 3), (1, 1, 0)), SumRestraint([5, 8], 7.0, rng.uniform(-3, 3, 3), (0, 1, 1))])
    F, e = ref.field(x, rs)
    h = 1e-5
    g = _numeric_gradient(lambda y: ref.field(y, rs)[1][1:].sum(), x, h)
    rounding = 20 * np.finfo(np.float64).eps * e[1:].sum() / h
    print("largest |F + dU/dx| %.2e, rounding bound %.2e, largest |F| %.1f" % (np.abs(F + g).max(), rounding, np.abs(F).max()))
    np.testing.assert_allclose(F, -g, rtol=1e-7, atol=rounding)
    assert e[0] == 0.0 and e[1] > 0 and e[2] > 0
    assert not F[[2, 3, 6]].any()  # nucleotides no term names


@pytest.mark.parametrize("m", [2, 4, 7])
def test_torque_forces_add_up_to_zero_and_carry_the_torque(m):
    rng = np.random.default_rng(m)
    x = rng.uniform(-5.0, 5.0, size=(m + 3, 3))
    index = rng.permutation(m + 3)[:m]
    T = rng.uniform(-1.0, 1.0, 3)
    F = ref.group_torque(x, index, T)
    d = x[index] - x[index].mean(axis=0)
    scale = np.abs(F).max()
    assert np.abs(F.sum(axis=0)).max() <= 1e-13 * scale
    t = T / np.linalg.norm(T)
    assert abs(np.cross(d, F).sum(axis=0) @ t - np.linalg.norm(T)) <= 1e-13


def test_a_torque_group_on_its_axis_gets_no_force():
    x = np.array([[0.3, -1.2, z] for z in (-2.0, 0.5, 1.7)])
    assert not ref.group_torque(x, [0, 1, 2], (0.0, 0.0, 0.4)).any()
    t = np.array([1.0, 2.0, -0.5])
    y = np.array([0.7, 0.1, 3.0]) + np.outer([-1.0, 0.25, 4.0], t)
    F = ref.group_torque(y, [0, 1, 2], 0.3 * t)
    assert np.isfinite(F).all() and not F.any()


def test_the_reader_returns_the_protocol_of_the_reference_input():
    rs, (index, force) = read_lammps_restraints(LAMMPS_IN, n=80)
    assert len(rs.tethers) == 1 and len(rs.sums) == 1 and len(rs.torques) == 1
    t, s, q = rs.tethers[0], rs.sums[0], rs.torques[0]
    assert set(t.index) == {0, 1, 78, 79} and t.k == K_LAMMPS and t.axes == (1, 1, 1) and t.anchor is None
    assert set(s.index) == {38, 41} and s.k == K_LAMMPS and s.axes == (1, 1, 0) and s.target == (0.0, 0.0, 0.0)
    assert q.index == (38, 39, 40, 41) and q.torque == (0.0, 0.0, 0.241412)
    np.testing.assert_array_equal(index, [38, 41])
    np.testing.assert_array_equal(force, [[0, 0, 0.0205634]] * 2)


@pytest.mark.parametrize(("line", "name"), [
    ("fix f1 fB addforce 0.1 v_nothing 0.0", "addforce"),
    ("fix f2 fB addtorque v_t 0 0", "addtorque"),
    ("fix f3 fB spring tether 10.0 0 0 0 0", "spring"),
    ("fix f4 fB spring/rg 10.0 1.0", "spring/rg"),
])
def test_the_reader_names_a_fix_it_does_not_build(tmp_path, line, name):
    path = tmp_path / "in"
    path.write_text("group fB id 39 42\n" + line + "\n")
    with pytest.raises(ValueError, match=name) as err:
        read_lammps_restraints(path, n=80)
    assert ":2:" in str(err.value)
    ok = tmp_path / "in.ok"
    ok.write_text("group a id <= 2\nfix 1 all nve/dotc/langevin 0.1 0.1 100.0 30362 angmom 1000\nfix t a spring/self 3.0\n")
    rs, (index, _) = read_lammps_restraints(ok)
    assert rs.tethers[0].index == (0, 1) and rs.tethers[0].k == 3.0 and index.size == 0


@pytest.mark.parametrize("line", ["group a id 1:4", "group a id <>  3", "group a id <=", "group a id <= 2 5", "group a id 1 x"])
def test_the_reader_names_a_group_line_it_cannot_read(tmp_path, line):
    path = tmp_path / "in"
    path.write_text("units lj\n" + line + "\nfix t a spring/self 3.0\n")
    with pytest.raises(ValueError, match="group id") as err:
        read_lammps_restraints(path, n=80)
    assert ":2:" in str(err.value) and line.split()[-1] in str(err.value)


def test_the_reference_frames_are_held_where_the_parsed_restraints_say():
    """tests/golden/regr/lammps-oxdna2-40bp/data.oxdna: 12 frames of the run the input describes, frame 0 the anchor.  With
    sigma = sqrt(kT / K) = 0.00906: the tethered nucleotides never leave their frame-0 positions by more than 0.0196 in a
    component, their rms deviation over frames 1-11 is 0.855 sigma, the xy sum of 38 and 41 has rms 0.548 sigma.  Asserted:
    rms <= sigma (1 + 3 / sqrt(2 N)), the thermal upper bound with three standard errors of an rms from N samples (132 for
    the tethers, 22 for the sum).  Nucleotides under another index convention, or a stiffness in other units, are not held
    like this: untethered nucleotides of this run move by tenths."""
    rs, _ = read_lammps_restraints(LAMMPS_IN, n=80)
    _, traj, _ = H.load_lammps_regr("lammps-oxdna2-40bp")
    c = np.asarray(traj.center, dtype=np.float64)
    assert c.shape == (12, 80, 3)
    sigma = np.sqrt(KT_LAMMPS / K_LAMMPS)
    t, s = rs.tethers[0], rs.sums[0]
    d = c[1:, list(t.index)] - c[0, list(t.index)]
    assert d.size == 132
    rms_t = np.sqrt((d * d).mean())
    print("tether: max", np.abs(d).max(), "rms / sigma", rms_t / sigma)
    assert np.abs(d).max() <= 0.0196 + 1e-6
    assert rms_t <= sigma * (1 + 3 / np.sqrt(2 * 132))
    ssum = (c[1:, list(s.index)].sum(axis=1) - np.asarray(s.target))[:, :2]
    assert ssum.size == 22
    rms_s = np.sqrt((ssum * ssum).mean())
    print("sum: rms / sigma", rms_s / sigma)
    assert rms_s <= sigma * (1 + 3 / np.sqrt(2 * 22))
    assert abs(rms_t / sigma - 0.855) < 5e-3 and abs(rms_s / sigma - 0.548) < 5e-3  # (the figures the GPU test leans on)
    free = c[1:, 20] - c[0, 20]
    assert np.sqrt((free * free).mean()) > 10 * sigma  # (an untethered nucleotide is not held)


def test_lowering_repeats_the_terms_per_replica():
    rs = Restraints(tethers=[SelfTether([0, 3], 2.0)], sums=[SumRestraint([1, 2], 5.0)], torques=[GroupTorque([0, 1, 2], (0, 0, 1.0))])
    x0 = np.arange(12.0).reshape(4, 3)
    off = np.array([[0.0, 0, 0], [10.0, 20.0, 30.0]])
    a = rs.lower(x0, n_one=4, n_rep=2, offsets=off)
    np.testing.assert_array_equal(a["t_index"], [0, 3, 4, 7])
    np.testing.assert_array_equal(a["t_anchor"], np.concatenate([x0[[0, 3]], x0[[0, 3]] + off[1]]))
    np.testing.assert_array_equal(a["g_kind"], [0, 1, 0, 1])
    np.testing.assert_array_equal(a["g_first"], [0, 2, 5, 7, 10])
    np.testing.assert_array_equal(a["g_member"], [1, 2, 0, 1, 2, 5, 6, 4, 5, 6])
    np.testing.assert_array_equal(a["g_target"][[0, 2]], [x0[1] + x0[2], x0[1] + x0[2] + 2 * off[1]])
    np.testing.assert_array_equal(a["t_mask"], [7] * 4)
    np.testing.assert_array_equal(a["g_mask"], [3, 0, 3, 0])
    with pytest.raises(ValueError, match="reference_center"):
        rs.lower(None, n_one=4)
    with pytest.raises(ValueError, match="out of range"):
        Restraints(torques=[GroupTorque([0, 4], (0, 0, 1.0))]).lower(x0, n_one=4)
