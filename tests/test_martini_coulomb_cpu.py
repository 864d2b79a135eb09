"""CPU tests of reaction-field Coulomb: the NumPy reference against itself (forces and virial by central differences,
the shift at the cut-off), the charges the topology readers deliver, and the new entry points in the built library."""

import numpy as np

from mythos_amd import _lib
from mythos_amd.input import gromacs
from tests import martini_helpers as MH
from tests import martini_rf_ref as RF
from tests import martini_synth as S

R_CUT = 1.1


def _charged(name="md37", seed=7):
    """A synthetic system with charges on a third of its beads, both signs, three magnitudes."""
    s = S.get(name)
    rng = np.random.default_rng(seed)
    q = rng.choice([0.0, 0.0, 1.0, -1.0, 0.5, -0.25], size=s["n"])
    q[s["bonds"][0]] = (1.0, -1.0)  # at least one charged bonded pair
    return s, q


def test_potential_and_force_vanish_at_the_cut_off_for_infinite_epsilon_rf():
    for qq in (1.0, -0.5):
        v, dv = RF.pair_v(R_CUT, qq, R_CUT, 15.0, 0.0)
        scale = RF.F_ELEC / 15.0 / R_CUT  # the bare Coulomb term at r_c
        assert abs(v) <= 4e-16 * scale and abs(dv) <= 4e-16 * scale / R_CUT
    # a finite epsilon_rf shifts the potential to zero as well, but leaves a force at the cut-off
    v, dv = RF.pair_v(R_CUT, 1.0, R_CUT, 15.0, 78.0)
    assert abs(v) <= 4e-16 * RF.F_ELEC / 15.0 / R_CUT and abs(dv) > 1e-3
    pref, k_rf, c_rf = RF.constants(R_CUT, 15.0, 0.0)
    assert pref == RF.F_ELEC / 15.0 and k_rf == 1.0 / (2.0 * R_CUT**3) and c_rf == 1.0 / R_CUT + k_rf * R_CUT**2


def test_reference_forces_are_central_differences_of_the_reference_energy():
    s, q = _charged()
    x, box = s["pos"][0], s["box"][0]
    for eps_rf in (0.0, 78.0):
        ref = RF.coulomb(x, box, q, s["bonds"], R_CUT, 15.0, eps_rf)
        assert ref["energy"]["pair"] != 0.0 and ref["energy"]["excluded"] != 0.0 and ref["energy"]["self"] < 0.0
        h = 1e-5
        charged = np.nonzero(q)[0]
        worst = 0.0
        for i in charged[:12]:
            for d in range(3):
                e = []
                for sgn in (1.0, -1.0):
                    y = x.copy()
                    y[i, d] += sgn * h
                    e.append(RF.coulomb(y, box, q, s["bonds"], R_CUT, 15.0, eps_rf)["e"])
                worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - ref["f"][i, d]))
        # central differences: h^2 V''' / 6 ~ 1e-10 x 1e2, and rounding 1e-16 |E| / h ~ 1e-8
        assert worst <= 1e-6 * np.abs(ref["f"]).max(), worst
        assert np.abs(ref["f"].sum(0)).max() <= 1e-12 * np.abs(ref["f"]).max()  # Newton's third law
        assert (ref["f"][q == 0.0] == 0.0).all()


def test_reference_virial_is_the_strain_derivative_of_the_reference_energy():
    s, q = _charged()
    x, box = s["pos"][0], s["box"][0]
    ref = RF.coulomb(x, box, q, s["bonds"], R_CUT)
    h = 1e-6
    for d in range(3):
        e = []
        for sgn in (1.0, -1.0):
            sc = np.ones(3)
            sc[d] = np.exp(sgn * h)
            e.append(RF.coulomb(x * sc, box * sc, q, s["bonds"], R_CUT)["e"])
        w = -(e[0] - e[1]) / (2 * h)
        assert abs(w - ref["w"][d]) <= 1e-6 * np.abs(ref["w"]).max(), (d, w, ref["w"][d])


def test_charges_of_the_golden_bilayer_tpr():
    top = gromacs.MartiniTopology.from_tpr(MH.MG / "m3" / "angle" / "test.tpr")
    q = top.charges
    names = np.array(top.atom_names)
    assert q.shape == (len(top.atom_types),) == (5831,)
    assert q.sum() == 0.0
    assert (q[names == "NC3"] == 1.0).all() and (names == "NC3").sum() == 242
    assert (q[names == "PO4"] == -1.0).all() and (names == "PO4").sum() == 242
    assert (q[(names != "NC3") & (names != "PO4")] == 0.0).all()


def test_charges_of_the_golden_bilayer_top():
    top = MH.system()["top"]
    q = top.charges
    names = np.array(top.atom_names)
    assert q.shape == (1280,) and q.sum() == 0.0
    assert (q[names == "NC3"] == 1.0).all() and (q[names == "PO4"] == -1.0).all()
    assert (q[(names != "NC3") & (names != "PO4")] == 0.0).all() and np.count_nonzero(q) == 256


TOP = """[ moleculetype ]
; name nrexcl
ION 1
[ atoms ]
; nr type resnr residue atom cgnr charge mass
1 Qd 1 ION NA+ 1 1.0 72.0
[ moleculetype ]
LIP 1
[ atoms ]
1 Q0 1 LIP NC3 1  0.75
2 Qa 1 LIP PO4 2 -1.25 ; a comment
3 Na 1 LIP GL1 3  0
4 C1 2 TAIL C1A 4
[ bonds ]
1 2 1 0.47 1250
2 3 1 0.47 1250
[ angles ]
1 2 3 2 120.0 25.0
[ system ]
test
[ molecules ]
LIP 2
ION 1
"""


def test_top_charge_column_round_trips_and_tile_repeats_it(tmp_path):
    path = tmp_path / "topol.top"
    path.write_text(TOP)
    top = gromacs.MartiniTopology.from_top(path)
    expect = np.array([0.75, -1.25, 0.0, 0.0, 0.75, -1.25, 0.0, 0.0, 1.0])
    assert top.charges.dtype == np.float64 and np.array_equal(top.charges, expect)
    assert top.atom_names[-1] == "NA+" and top.bonded_neighbors.shape == (4, 2)
    tiled = top.tile(3)
    assert np.array_equal(tiled.charges, np.tile(expect, 3)) and len(tiled.atom_types) == 27
    # a topology built by hand, as before the field existed, has none - and tiles to none
    bare = gromacs.MartiniTopology(atom_types=top.atom_types, atom_names=top.atom_names, residue_names=top.residue_names,
                                   angles=top.angles, bonded_neighbors=top.bonded_neighbors)
    assert bare.charges is None and bare.tile(2).charges is None


def test_library_exports_the_coulomb_entry_points():
    lib = _lib.load()
    for name in ("mythos_martini_set_charges", "mythos_martini_coulomb"):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(lib, name)
    # no system: both refuse with INVALID_ARGUMENT instead of touching a device
    assert lib.mythos_martini_set_charges(None, None, 15.0, 0.0) != 0
    assert lib.mythos_martini_coulomb(None, None, None, 0, None, None, None) != 0
