"""Pins tests/stress_profile_ref.py, the CPU side of tests/test_gpu_stress_profile.py: the per-bead virial shares against
the strain virial of tests/martini_npt_ref.py (autograd through the oracle's energies) and against central differences,
the slab formulas at their edges, the host-side refusals of mythos_martini_stress_profile_check, the ABI, and the
edge clearance of the systems the GPU tests compare slab counts on."""

import re
from pathlib import Path

import numpy as np
import pytest

from mythos_amd import _lib
from tests import martini_helpers as MH
from tests import martini_npt_ref as NR
from tests import martini_rf_ref as RF
from tests import stress_profile_ref as SR

ROOT = Path(__file__).resolve().parent.parent


def _bilayer():
    s = MH.system()
    x, box, _ = MH.frames("lj")
    top = s["top"]
    ff = (s["types"], s["sigma"], s["eps"], np.asarray(top.bonded_neighbors), s["bond_k"], s["bond_r0"], np.asarray(top.angles),
          s["angle_k"], s["angle_t0"])
    return dict(ff=ff, angle_kind=0, pos=x[3:4].astype(np.float64), box=box[3:4].astype(np.float64), charges=None)


@pytest.mark.parametrize("name", ["bilayer", "n131", "q259", "slab259"])
def test_the_shares_of_all_beads_add_up_to_the_strain_virial(name):
    """sum_i w_i = -dU/ds of the oracle's energies at pos * s, box * s, to 1e-10 of max |W| (the project's NPT bound); the
    Coulomb shares against the virial of martini_rf_ref, which the strain virial does not hold."""
    c = _bilayer() if name == "bilayer" else SR.case(name)
    g96 = c["angle_kind"] == 0
    w = SR.bead_shares(c["pos"][0], c["box"][0], *c["ff"], g96, charges=c["charges"])
    total = w["lj"].sum(0) + w["bond"].sum(0) + w["angle"].sum(0)
    ref = NR.strain_virial(c["pos"][0], c["box"][0], *c["ff"], g96)
    err = np.abs(total - ref).max() / np.abs(ref).max()
    print(f"  {name}: W {total}, strain virial {ref}, rel. error {err:.3e}")
    assert err <= 1e-10
    if c["charges"] is None:
        assert not w["coulomb"].any()
    else:
        rf = RF.coulomb(c["pos"][0], c["box"][0], c["charges"], c["ff"][3], 1.1)
        assert np.abs(rf["virial"]["excluded"]).max() > 0.0  # (the case holds bonded charged pairs)
        assert np.abs(w["coulomb"].sum(0) - rf["w"]).max() <= 1e-10 * np.abs(rf["w"]).max()


def test_the_shares_against_central_differences_of_the_energy():
    c = SR.case("n61")
    w = SR.bead_shares(c["pos"][0], c["box"][0], *c["ff"], True)
    total = w["lj"].sum(0) + w["bond"].sum(0) + w["angle"].sum(0)
    fd = NR.strain_virial_fd(c["pos"][0], c["box"][0], *c["ff"], True)
    err = np.abs(total - fd).max() / np.abs(fd).max()
    print(f"  n61: W {total}, central differences {fd}, rel. error {err:.3e}")
    # h = 1e-6: the rounding of the difference sits just above 1e-10 (measured here: 1.1e-10), so the bound is that of
    # tests/test_martini_npt_cpu.py for the same strain_virial_fd
    assert err <= 1e-8


def test_an_angle_gives_nothing_to_its_centre_bead():
    z = np.zeros(0)
    pos = np.array([[0.1, 0.2, 0.3], [0.5, 0.3, 0.2], [0.7, 0.8, 0.1]])
    w = SR.bead_shares(pos, [5.0, 5.0, 5.0], [0, 0, 0], [[0.47]], [[0.0]], np.zeros((0, 2), int), z, z, [[0, 1, 2]], [25.0], [2.3], True)
    assert not w["angle"][1].any() and w["angle"][0].any() and w["angle"][2].any()
    assert not w["lj"].any() and not w["bond"].any()


def test_slab_formulas_at_their_edges():
    lz, nb = 4.0, 8
    under = np.nextafter(lz, 0.0)
    # fixed to the box: z = 0 and z = Lz open slab 0, just under Lz closes the last one; stored coordinates outside wrap
    assert SR.slab_index([0.0, lz, under, -0.0], lz, nb).tolist() == [0, 0, nb - 1, 0]
    assert SR.slab_index([-0.25, -lz, lz + 0.25, 2 * lz + 0.75, -3 * lz - 0.25], lz, nb).tolist() == [nb - 1, 0, 0, 1, nb - 1]
    assert SR.slab_index([-1e-30], lz, nb).tolist() == [nb - 1]  # (u rounds to 1: the clamp)
    assert SR.slab_index([0.3, 17.0, -5.0], lz, 1).tolist() == [0, 0, 0]
    # centred: slab n_bins / 2 starts at the midplane; half a box away the profile wraps
    mid = 3.9
    z = np.array([mid, np.nextafter(mid, 0.0), mid + 0.5 * lz - 1e-9, mid - 0.5 * lz, mid + 0.5 * lz, mid + lz, mid - 0.3 + 2 * lz])
    assert SR.slab_index(z, lz, nb, mid).tolist() == [nb // 2, nb // 2 - 1, nb - 1, 0, 0, nb // 2, nb // 2 - 1]
    # a midpoint that puts beads on both sides of the wrap: z = 0.1 and z = 3.9 are 0.2 apart across the boundary
    assert SR.slab_index([0.1, 3.9, 0.3], lz, nb, 0.0).tolist() == [nb // 2, nb // 2 - 1, nb // 2]
    assert SR.slab_index([0.5 * lz * (1.0 - 2.0**-53)], lz, nb, 0.0).tolist() in ([nb - 1], [0])  # (t + 1/2 rounds to 1: clamped, in range)
    # odd slab counts: the midplane lies inside slab n_bins // 2
    assert SR.slab_index([mid], lz, 7, mid).tolist() == [3]
    # counts: every bead lands in exactly one slab
    rng = np.random.default_rng(1)
    zz = rng.uniform(-9.0, 9.0, size=500)
    for m in (None, 1.234):
        assert np.bincount(SR.slab_index(zz, lz, 13, m), minlength=13).sum() == 500


def test_raw_rows_add_up_and_the_surface_tension_is_that_of_the_totals():
    c = SR.case("q259")
    kT = 2.27
    args = (c["pos"][1], c["box"][1], 7, *c["ff"], True)
    by = SR.raw_rows(*args, by_term=True, charges=c["charges"], center_index=c["center"])
    row = SR.raw_rows(*args, charges=c["charges"], center_index=c["center"])
    one = SR.raw_rows(c["pos"][1], c["box"][1], 1, *c["ff"], True, charges=c["charges"])
    assert by[:, 0].sum() == c["n"] and np.array_equal(by[:, 0], row[:, 0])
    np.testing.assert_allclose(by[:, 1:].reshape(7, 4, 3).sum(1), row[:, 1:], rtol=0, atol=1e-12 * np.abs(row[:, 1:]).max())
    np.testing.assert_allclose(row[:, 1:].sum(0), one[0, 1:], rtol=0, atol=1e-12 * np.abs(one[0, 1:]).max())
    p = SR.pressures(one, c["box"][1], kT)[0]
    gamma = SR.surface_tension(row, c["box"][1], kT)
    assert gamma == pytest.approx(c["box"][1, 2] * (p[2] - 0.5 * (p[0] + p[1])), rel=1e-12)


def _check(n=10, r_cut=1.1, boxes=None, center=None, n_bins=8):
    from mythos_amd.hip_system import MartiniSystem

    MartiniSystem.check_stress_profile(n, r_cut, boxes, n_bins, center)


def test_the_check_entry_refuses_by_name_without_a_gpu():
    _check()
    _check(boxes=[[2.2, 3.0, 4.0]] * 3, center=[0, 9], n_bins=1024)
    with pytest.raises(ValueError, match=r"n_bins < 1 \(at least one slab\)"):
        _check(n_bins=0)
    with pytest.raises(ValueError, match="n_bins = 1025 is above the cap of 1024 slabs"):
        _check(n_bins=1025)
    with pytest.raises(ValueError, match=r"centre index 10 \(entry 1\) is outside \[0, 10\)"):
        _check(center=[3, 10])
    with pytest.raises(ValueError, match=r"centre index -1 \(entry 0\) is outside \[0, 10\)"):
        _check(center=[-1])
    good = [3.0, 3.0, 3.0]
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="frame 2: box edge 1 is not positive and finite"):
            _check(boxes=[good, good, [3.0, bad, 3.0]])
    with pytest.raises(ValueError, match=r"frame 1: box edge 2 = 2\.1\d* is shorter than 2 r_cut = 2\.2"):
        _check(boxes=[good, [3.0, 3.0, 2.1]])
    assert "mythos_martini_stress_profile_check: " in _lib.last_error()


def test_a_single_term_lowers_to_its_own_tables_with_neutral_values_for_the_others():
    """lower_martini, the one lowering: a lone Bond term keeps its k and r0, carries eps = 0 and angle k = 0; a lone Coulomb
    term brings its charges; anything else is refused by name."""
    from mythos_amd.energy import martini as M
    from mythos_amd.simulators.hip_martini import lower_martini

    s = MH.system()
    low = lower_martini(M.Bond.from_topology(topology=s["top"], params=M.BondConfiguration(**s["bond_params"])))
    np.testing.assert_allclose(low["bond_k"], s["bond_k"])
    np.testing.assert_allclose(low["bond_r0"], s["bond_r0"])
    assert not low["eps"].any() and not low["angle_k"].any() and low["charges"] is None and len(low["types"]) == 1280
    assert np.array_equal(low["bonds"], np.asarray(s["top"].bonded_neighbors)) and low["angle_kind"] == 0
    q = lower_martini(M.Coulomb.from_topology(topology=s["top"]))
    assert np.array_equal(q["charges"], s["top"].charges) and q["epsilon_r"] == 15.0 and not q["bond_k"].any()
    with pytest.raises(TypeError, match="MartiniComposedEnergyFunction or a single MARTINI term"):
        lower_martini(object())


def test_the_abi_declares_and_exports_the_stress_profile():
    """Fails without the feature: the header, the binding and the library all carry the three entry points."""
    header = (ROOT / "include" / "mythos_hip.h").read_text()
    lib = _lib.load()
    for name in ("mythos_martini_stress_profile", "mythos_martini_stress_profile_check", "mythos_martini_bar_per_kj_mol_nm3"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.DECLARED_SYMBOLS and hasattr(lib, name), name
    assert "#define MYTHOS_STRESS_ROW 4" in header and "#define MYTHOS_STRESS_ROW_BY_TERM 13" in header
    assert (_lib.STRESS_ROW, _lib.STRESS_ROW_BY_TERM) == (4, 13)
    assert lib.mythos_martini_bar_per_kj_mol_nm3() == NR.BAR == SR.BAR
    from mythos_amd import observables as O
    from mythos_amd.observables import stress_profile as P

    assert O.StressProfile is P.StressProfile and O.SurfaceTension is P.SurfaceTension and P.to_mN_per_m == 0.1
    assert "StressProfile" in O.__all__ and "SurfaceTension" in O.__all__ and P.MAX_BINS == 1024


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_the_gpu_cases_keep_every_bead_clear_of_the_slab_edges(name):
    c = SR.case(name)  # (asserts the clearance for every slab count, both centrings, fp64 and fp32 values)
    assert c["pos"].shape == (3, c["n"], 3) and c["box"].shape == (3, 3)
    assert np.abs(c["pos"] / c["box"][:, None, :]).max() > 1.0  # stored coordinates outside the box
    SR.assert_clear_of_edges(c, n_bins=(2, 3, 100))
