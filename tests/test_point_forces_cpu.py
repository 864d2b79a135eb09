"""Point forces of the oxDNA Langevin integrator without a GPU: the reader of oxDNA external-force files
(read_external_field) on files written here, the lowering per replica, the NumPy reference of the five laws
(tests/point_forces_ref.py) against central differences of its own energies, and every refusal of a term through the C
ABI's host-side check (mythos_point_forces_check, what mythos_langevin_set_point_forces runs first)."""

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.input.external_forces import read_external_field, read_external_forces
from mythos_amd.simulators.restraints import (FLAG_PBC, KIND_MUTUAL_TRAP, KIND_PLANE, KIND_SPHERE, KIND_STRING, KIND_TRAP, MovingString,
                                              MutualTrap, PointForces, RepulsionPlane, RepulsionSphere, Trap)
from tests import point_forces_ref as ref

FILE = """
# a relaxation input's mutual traps, a ramp, a steered trap, a wall and a cage
{
type = mutual_trap
particle = 0
ref_particle = 15
stiff = 0.9
r0 = 1.2
}
{
type = mutual_trap
particle = 15
ref_particle = 0
stiff = 0.9
r0 = 1.2
rate = 1e-6
PBC = 1
}
{
type = string
particle = 3
F0 = 0.5
rate = 1e-5   # a force ramp
dir = 0., 3., 4.
}
{
type = string
particle = 2, 2, 7
F0 = 0.25
rate = 0.
dir = 0., 0., 2.
}
{
type = trap
particle = 4
pos0 = 1., 2., 3.
stiff = 2.5
rate = 2e-4
dir = 2., 0., 0.
}
{
type = repulsion_plane
particle = 1-3
stiff = 4.
dir = 0., 0., 5.
position = 7.5
}
{
type = repulsion_sphere
particle = -1
center = 0.5, -0.5, 1.
r0 = 6.
stiff = 10.
}
{
type = repulsion_sphere
particle = 9
center = 0., 0., 0.
r0 = 6.
stiff = 10.
rate = -1e-4
}
"""


def test_the_reader_returns_every_type_with_its_defaults(tmp_path):
    path = tmp_path / "external.conf"
    path.write_text(FILE)
    pf, (index, force) = read_external_field(path, n=16)
    t = pf.terms
    assert t[0] == MutualTrap(0, 15, 0.9, 1.2, 0.0, False)  # rate and PBC default to 0
    assert t[1] == MutualTrap(15, 0, 0.9, 1.2, 1e-6, True)
    assert t[2] == MovingString(3, 0.5, 1e-5, (0.0, 0.6, 0.8))  # dir normalised
    assert t[3] == Trap(4, (1.0, 2.0, 3.0), 2.5, 2e-4, (1.0, 0.0, 0.0))
    assert t[4:7] == tuple(RepulsionPlane(i, 4.0, (0.0, 0.0, 1.0), 7.5) for i in (1, 2, 3))  # a range
    assert t[7:23] == tuple(RepulsionSphere(i, (0.5, -0.5, 1.0), 6.0, 10.0, 0.0) for i in range(16))  # particle = -1, rate defaults to 0
    assert t[23] == RepulsionSphere(9, (0.0, 0.0, 0.0), 6.0, 10.0, -1e-4) and len(t) == 24
    # the constant string goes to the pair set_external_forces takes, a particle named twice summed
    np.testing.assert_array_equal(index, [2, 7])
    np.testing.assert_array_equal(force, [[0, 0, 0.5], [0, 0, 0.25]])
    assert index.dtype == np.int32 and force.dtype == np.float64
    # read_external_forces stays what it was: it refuses the first block it does not build
    with pytest.raises(ValueError, match="mutual_trap"):
        read_external_forces(path, n=16)
    only = tmp_path / "strings.conf"
    only.write_text("{\ntype = string\nparticle = 5\nF0 = 0.1\nrate = 0\ndir = 1, 0, 0\n}\n")
    pf, const = read_external_field(only)
    assert not pf and pf.terms == ()
    for a, b in zip(const, read_external_forces(only)):
        np.testing.assert_array_equal(a, b)
    empty = tmp_path / "empty.conf"
    empty.write_text("# nothing\n")
    pf, const = read_external_field(empty)
    assert not pf and const[0].shape == (0,) and const[1].shape == (0, 3)


@pytest.mark.parametrize(("body", "match"), [
    ("type = twist\nparticle = 0\nstiff = 1.\nrate = 1e-5\nbase = 0.\npos0 = 0, 0, 0\ncenter = 0, 0, 0\naxis = 0, 0, 1\nmask = 1, 1, 0", "type = twist"),
    ("type = com\ncom_list = 0,1\nref_list = 2,3\nstiff = 1.\nr0 = 2.", "type = com"),
    ("type = repulsion_plane_moving\nparticle = 0\nstiff = 1.\ndir = 0,0,1\nref_particle = 1", "type = repulsion_plane_moving"),
    ("type = trap\nparticle = 0\nstiff = 1.\nrate = 0\ndir = 0,0,1", "missing pos0"),
    ("type = mutual_trap\nparticle = 0\nstiff = 1.\nr0 = 1.", "missing ref_particle"),
    ("type = repulsion_plane\nparticle = 0\nstiff = 1.\ndir = 0,0,0\nposition = 1.", "not a direction"),
    ("type = repulsion_sphere\nparticle = 0\nstiff = 1.\nr0 = 1.\ncenter = 0, 0", "not three numbers"),
    ("type = string\nparticle = 16\nF0 = 1.\nrate = 1e-3\ndir = 0,0,1", "particle 16 out of range"),
])
def test_the_reader_refuses_by_name(tmp_path, body, match):
    path = tmp_path / "external.conf"
    path.write_text("{\ntype = string\nparticle = 1\nF0 = 1.\nrate = 0.\ndir = 1, 0, 0\n}\n{\n" + body + "\n}\n")
    with pytest.raises(ValueError, match=match) as err:
        read_external_field(path, n=16)
    assert "block 1" in str(err.value)


def test_lowering_repeats_the_terms_per_replica():
    """Three replicas against the set shifted by hand: indices by r n_one, pos0 and center by the replica's offset, a
    plane's position by -d.offset, a moving string's energy origin at the offset; a mutual trap has nothing to move."""
    pf = PointForces([MovingString(1, 0.5, 1e-5, (0, 3, 4)), Trap(2, (1.0, 2.0, 3.0), 2.5, 2e-4, (2, 0, 0)), MutualTrap(0, 3, 0.9, 1.2, 1e-6, True),
                      RepulsionPlane(3, 4.0, (0, 0, 5), 7.5), RepulsionSphere(2, (0.5, -0.5, 1.0), 6.0, 10.0, -1e-4), Trap(0, (0, 0, 0), 1.0)])
    off = np.array([[0.0, 0.0, 0.0], [10.0, 20.0, 30.0], [-5.0, 0.25, 8.0]])
    a = pf.lower(n_one=4, n_rep=3, offsets=off)
    kinds = [KIND_STRING, KIND_TRAP, KIND_MUTUAL_TRAP, KIND_PLANE, KIND_SPHERE, KIND_TRAP]
    np.testing.assert_array_equal(a["kind"], kinds * 3)
    np.testing.assert_array_equal(a["particle"], [1, 2, 0, 3, 2, 0, 5, 6, 4, 7, 6, 4, 9, 10, 8, 11, 10, 8])
    np.testing.assert_array_equal(a["ref_particle"][2::6], [3, 7, 11])
    np.testing.assert_array_equal(a["flags"], [0, 0, FLAG_PBC, 0, 0, 0] * 3)
    assert a["param"].shape == (18, 8) and a["param"].dtype == np.float64 and a["kind"].dtype == np.int32
    for r in range(3):
        rows = a["param"][6 * r: 6 * r + 6]
        np.testing.assert_array_equal(rows[0], [0.5, 1e-5, 0.0, 0.6, 0.8, *off[r]])
        np.testing.assert_array_equal(rows[1], [2.5, 2e-4, 1.0, 0.0, 0.0, *(np.array([1.0, 2.0, 3.0]) + off[r])])
        np.testing.assert_array_equal(rows[2], [0.9, 1.2, 1e-6, 0, 0, 0, 0, 0])
        np.testing.assert_array_equal(rows[3], [4.0, 7.5 - off[r][2], 0.0, 0.0, 1.0, 0, 0, 0])
        np.testing.assert_array_equal(rows[4], [10.0, 6.0, -1e-4, *(np.array([0.5, -0.5, 1.0]) + off[r]), 0, 0])
        np.testing.assert_array_equal(rows[5], [1.0, 0.0, 0.0, 0.0, 0.0, *off[r]])  # a resting trap needs no dir
    # the shifted set gives the shifted replica the forces of the original: the reference agrees with the rows
    rng = np.random.default_rng(0)
    x = rng.uniform(-8.0, 8.0, (4, 3))
    F0, e0 = ref.point_field(x, pf, 1000.0)
    shifted = PointForces([MovingString(1, 0.5, 1e-5, (0, 3, 4)), Trap(2, np.array([1.0, 2.0, 3.0]) + off[1], 2.5, 2e-4, (2, 0, 0)), MutualTrap(0, 3, 0.9, 1.2, 1e-6, True),
                           RepulsionPlane(3, 4.0, (0, 0, 5), 7.5 - off[1][2]), RepulsionSphere(2, np.array([0.5, -0.5, 1.0]) + off[1], 6.0, 10.0, -1e-4),
                           Trap(0, off[1], 1.0)])
    F1, e1 = ref.point_field(x + off[1], shifted, 1000.0, origin=off[1])
    np.testing.assert_allclose(F1, F0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(e1, e0, rtol=1e-12, atol=1e-12)
    assert e0[3] > 0 or e0[4] > 0
    with pytest.raises(ValueError, match="out of range"):
        PointForces([MutualTrap(0, 4, 1.0, 1.0)]).lower(n_one=4)
    with pytest.raises(ValueError, match="n_one"):
        pf.lower(n_rep=2)
    with pytest.raises(ValueError, match="not a direction"):
        MovingString(0, 1.0, 1e-3, (0, 0, 0))
    with pytest.raises(ValueError, match="not a direction"):
        Trap(0, (0, 0, 0), 1.0, rate=1e-3)


def _numeric_gradient(u, x, h):
    g = np.zeros_like(x)
    for i in range(x.shape[0]):
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, a] += h
            xm[i, a] -= h
            g[i, a] = (u(xp) - u(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("s", [0.0, 12345.0])
def test_the_reference_forces_are_minus_the_gradient_of_the_reference_energies(s):
    """Every law on the particle it acts on, both branches of the one-sided ones.  The energy of a term is a function of
    its own particle's position (a mutual trap's partner held fixed: the law puts no force on it), so the gradient is
    taken term by term with respect to that particle.  h = 1e-5: the truncation of a central difference is
    h^2 / 6 U''' (zero for the quadratic laws; 1 / r^2-like for the mutual trap and the sphere, under 1e-10 here) and its
    rounding 20 eps U / h, 5e-10 at U of order 100 - rtol 1e-7 with that absolute term."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-3.0, 3.0, (8, 3))
    x[5] = (0.2, -0.1, 0.3)  # inside the sphere
    x[6] = (4.0, 3.0, -5.0)  # outside
    terms = [MovingString(0, 0.5, 1e-4, (1, 2, -2)), Trap(1, (0.5, 0.2, -1.0), 3.0, 1e-4, (0, 1, 0)), Trap(1, (0.0, 0.0, 0.0), 1.5),
             MutualTrap(2, 3, 2.0, 0.5 * np.linalg.norm(x[3] - x[2]), 1e-5), MutualTrap(3, 2, 2.0, 2.0 * np.linalg.norm(x[3] - x[2]), 1e-5),
             RepulsionPlane(4, 5.0, (0, 0, 1), -x[4, 2] - 0.7), RepulsionPlane(4, 5.0, (0, 0, 1), -x[4, 2] + 0.7),
             RepulsionSphere(5, (0, 0, 0), 2.0, 7.0, 1e-5), RepulsionSphere(6, (0, 0, 0), 2.0, 7.0, 1e-5)]
    h = 1e-5
    for t in terms:
        f, u = ref.point_term(x, t, s)
        own = lambda y, t=t: ref.point_term(np.concatenate([x[: t.particle], y, x[t.particle + 1:]]), t, s)[1]  # noqa: E731
        g = _numeric_gradient(own, x[t.particle: t.particle + 1].copy(), h)[0]
        np.testing.assert_allclose(f, -g, rtol=1e-7, atol=20 * np.finfo(np.float64).eps * max(abs(u), 1.0) / h + 1e-10, err_msg=repr(t))
    # both branches were there
    assert ref.point_term(x, terms[5], s)[1] > 0 and ref.point_term(x, terms[6], s)[1] == 0
    assert ref.point_term(x, terms[7], s)[1] == 0 and ref.point_term(x, terms[8], s)[1] > 0
    # a longer trap pulls towards the partner, a shorter pushes away
    assert ref.point_term(x, terms[3], s)[0] @ (x[3] - x[2]) > 0 and ref.point_term(x, terms[4], s)[0] @ (x[2] - x[3]) < 0
    # r = 0: no force, no division by zero
    y = x.copy()
    y[3] = y[2]
    f, u = ref.point_term(y, terms[3], s)
    assert not f.any() and np.isfinite(u)
    # the minimum image
    box = np.array([10.0, 12.0, 14.0])
    z = np.zeros((2, 3))
    z[0], z[1] = (0.5, 1.0, 1.0), (9.5, 1.0, 1.0)
    f_pbc, _ = ref.mutual_trap(z, MutualTrap(0, 1, 1.0, 0.0, 0.0, True), 0.0, box)
    f_free, _ = ref.mutual_trap(z, MutualTrap(0, 1, 1.0, 0.0, 0.0, False), 0.0, box)
    np.testing.assert_allclose(f_pbc, [-1.0, 0, 0], atol=1e-15)
    np.testing.assert_allclose(f_free, [9.0, 0, 0], atol=1e-15)


# ------------------------------------------------------------------ the refusals, through the ABI
def _check(pf_arrays, n=16, has_box=False):
    a = pf_arrays
    ip = lambda v: v.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    rc = _lib.load().mythos_point_forces_check(n, int(has_box), int(a["kind"].shape[0]), ip(a["kind"]), ip(a["particle"]), ip(a["ref_particle"]),
                                               ip(a["flags"]), a["param"].ctypes.data_as(_lib.c_double_p))
    return rc, _lib.last_error()


VALID = PointForces([MovingString(1, 0.5, 1e-5, (0, 3, 4)), Trap(2, (1.0, 2.0, 3.0), 2.5, 2e-4, (2, 0, 0)), MutualTrap(0, 3, 0.9, 1.2, 1e-6),
                     RepulsionPlane(3, 4.0, (0, 0, 5), 7.5), RepulsionSphere(2, (0.5, -0.5, 1.0), 6.0, 10.0, -1e-4), Trap(0, (0, 0, 0), 1.0)])
STRING, TRAP, MUTUAL, PLANE, SPHERE, RESTING = range(6)  # the places of VALID's terms


@pytest.mark.parametrize(("term", "key", "col", "value", "match"), [
    (STRING, "particle", None, -1, r"term 0 \(string\): particle -1 out of range \[0, 16\)"),
    (SPHERE, "particle", None, 16, r"term 4 \(repulsion_sphere\): particle 16 out of range"),
    (MUTUAL, "ref_particle", None, 16, r"term 2 \(mutual_trap\): ref_particle 16 out of range"),
    (MUTUAL, "ref_particle", None, -3, r"term 2 \(mutual_trap\): ref_particle -3 out of range"),
    (MUTUAL, "ref_particle", None, 0, r"term 2 \(mutual_trap\): ref_particle is the particle itself"),
    (TRAP, "param", 6, np.nan, r"term 1 \(trap\): parameter 6 is not finite"),
    (STRING, "param", 1, np.inf, r"term 0 \(string\): parameter 1 is not finite"),
    (TRAP, "param", 0, -2.5, r"term 1 \(trap\): stiff is negative"),
    (MUTUAL, "param", 0, -1.0, r"term 2 \(mutual_trap\): stiff is negative"),
    (PLANE, "param", 0, -1.0, r"term 3 \(repulsion_plane\): stiff is negative"),
    (SPHERE, "param", 0, -1.0, r"term 4 \(repulsion_sphere\): stiff is negative"),
    (MUTUAL, "param", 1, -0.1, r"term 2 \(mutual_trap\): r0 is negative"),
    (SPHERE, "param", 1, -0.1, r"term 4 \(repulsion_sphere\): r0 is negative"),
    (STRING, "param", slice(2, 5), 0.0, r"term 0 \(string\): dir is zero"),
    (TRAP, "param", slice(2, 5), 0.0, r"term 1 \(trap\): dir is zero"),
    (PLANE, "param", slice(2, 5), 0.0, r"term 3 \(repulsion_plane\): dir is zero"),
    (MUTUAL, "flags", None, FLAG_PBC, r"term 2 \(mutual_trap\): PBC = 1 on a system without a box"),
    (PLANE, "flags", None, FLAG_PBC, r"term 3 \(repulsion_plane\): flags = 1"),
    (MUTUAL, "flags", None, 2, r"term 2 \(mutual_trap\): flags = 2"),
    (SPHERE, "kind", None, 5, r"term 4: kind 5 is not"),
    (SPHERE, "kind", None, -1, r"term 4: kind -1 is not"),
])
def test_the_entry_point_refuses_a_bad_term_and_names_it(term, key, col, value, match):
    a = VALID.lower(n_one=16)
    assert _check(a)[0] == 0
    if col is None:
        a[key][term] = value
    else:
        a[key][term, col] = value
    rc, msg = _check(a)
    assert rc == -1, msg
    with pytest.raises(ValueError, match="mythos_point_forces_check: " + match):
        _lib.check(rc, "point_forces_check")


def test_what_the_entry_point_admits():
    a = VALID.lower(n_one=16)
    assert _check(a)[0] == 0
    a["flags"][MUTUAL] = FLAG_PBC
    assert _check(a, has_box=True)[0] == 0  # the minimum image where there is a box
    a = VALID.lower(n_one=16)
    a["param"][STRING, 0] = -0.5  # a string may pull backwards: F0 is no stiffness
    a["param"][MUTUAL, 0] = a["param"][SPHERE, 0] = 0.0  # stiff = 0 is a term without a force
    assert _check(a)[0] == 0
    assert _check(PointForces().lower(n_one=16))[0] == 0  # the empty set, which clears
    lib = _lib.load()
    assert lib.mythos_point_forces_check(16, 0, 1, None, None, None, None, None) == -1
    assert lib.mythos_langevin_set_point_forces(None, 0, None, None, None, None, None) == -1
    assert "mythos_langevin_set_point_forces: invalid argument" in _lib.last_error()
    assert lib.mythos_langevin_eval_external_at(None, None, 0.0, None, None, None) == -1
