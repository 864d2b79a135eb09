"""CPU tests of the MARTINI integrator's external forces: the NumPy reference (tests/martini_restraints_ref.py) against
central differences of its own energy, the lowering of a set to the flat arrays of mythos_martini_langevin_set_restraints
(evaluated by a NumPy transcription of the kernels' reading of them), ``from_mdp`` / ``read_ndx``, and every refusal through
mythos_martini_restraints_check, which touches no device."""

import copy

import numpy as np
import pytest

from mythos_amd.simulators import martini_restraints as MR
from mythos_amd.simulators.martini_restraints import (FlatBottomRestraint, MartiniRestraints, PositionRestraint, PullCoordinate,
                                                       PullGroup)
from tests import martini_restraints_cases as CS
from tests import martini_restraints_ref as REF

BOX = np.array([3.0, 3.5, 3.7])
N = 24


def _system(seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.2, 0.8, size=(N, 3)) * BOX, rng.uniform(40.0, 90.0, size=N)


def _gradient_check(rs, x, masses, s=0, dt=0.01, rep=0, ref=None, h=1e-6):
    F, e, _ = REF.field(rs, x, masses, BOX, s, dt, rep, ref)
    num = np.zeros_like(x)
    for i in range(x.shape[0]):
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, a] += h
            xm[i, a] -= h
            num[i, a] = -(REF.energy(rs, xp, masses, BOX, s, dt, rep, ref) - REF.energy(rs, xm, masses, BOX, s, dt, rep, ref)) / (2 * h)
    scale = max(1.0, np.abs(F).max())
    assert np.abs(F - num).max() <= 1e-6 * scale, (np.abs(F - num).max(), scale)
    return F, e


def _coordinate(**kw):
    base = dict(group_a=PullGroup(members=(0, 1, 2)), group_b=PullGroup(members=(5, 6)), k=700.0, init=0.3)
    base.update(kw)
    return PullCoordinate(**base)


TERMS = {
    "position": MartiniRestraints(position=[PositionRestraint(index=3, k=(500.0, 0.0, 120.0), reference=(1.0, 1.2, 1.4)),
                                            PositionRestraint(index=4, k=300.0)]),
    "sphere": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=2, shape="sphere", r=0.2, k=400.0, reference=(1.0, 1.0, 1.0))]),
    "sphere-inverted": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=2, shape="sphere", r=9.0, k=400.0, invert=True, reference=(1.0, 1.0, 1.0))]),
    "cylinder": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=7, shape="cylinder", axis="y", r=0.1, k=400.0, reference=(0.1, 9.0, 0.2))]),
    "cylinder-inverted": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=7, shape="cylinder", axis="x", r=9.0, k=40.0, invert=True, reference=(0.1, 0.3, 0.2))]),
    "layer": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=8, shape="layer", axis="z", r=0.05, k=400.0, reference=(0.0, 0.0, 0.1))]),
    "layer-inverted": MartiniRestraints(flat_bottom=[FlatBottomRestraint(index=8, shape="layer", axis=1, r=9.0, k=40.0, invert=True, reference=(0.0, 0.1, 0.0))]),
    "distance-periodic": MartiniRestraints(pulls=[_coordinate(geometry="distance", dim=(True, False, True), periodic=True)]),
    "distance-plain": MartiniRestraints(pulls=[_coordinate(geometry="distance", periodic=False)]),
    "direction-periodic-image": MartiniRestraints(pulls=[_coordinate(geometry="direction", vec=(1.0, -2.0, 0.5), periodic=True)]),
    "direction-plain": MartiniRestraints(pulls=[_coordinate(geometry="direction", vec=(1.0, -2.0, 0.5), periodic=False)]),
    "absolute": MartiniRestraints(pulls=[_coordinate(group_a=None, origin=(0.4, 0.5, 0.6), geometry="distance", periodic=False)]),
    "absolute-direction": MartiniRestraints(pulls=[_coordinate(group_a=None, origin=(0.4, 0.5, 0.6), geometry="direction", vec=(0, 0, 1), periodic=True)]),
    "constant-force": MartiniRestraints(pulls=[_coordinate(kind="constant-force", k=-55.0, geometry="distance")]),
    "constant-force-direction": MartiniRestraints(pulls=[_coordinate(kind="constant-force", k=35.0, geometry="direction", vec=(0, 1, 1))]),
    "moving": MartiniRestraints(pulls=[_coordinate(geometry="direction", vec=(0, 0, 1), rate=4.0e-3, init=-0.5)]),
}


@pytest.mark.parametrize("name", sorted(TERMS))
def test_reference_forces_are_minus_the_gradient_of_the_reference_energy(name):
    x, masses = _system()
    s = 12345 if name == "moving" else 0
    F, e = _gradient_check(TERMS[name], x, masses, s=s, ref=x + 0.05)
    assert np.abs(F).max() > 1.0 and e.sum() != 0.0, "the case exerts no force: it checks nothing"
    if name == "moving":  # the reference moved by rate * t = 4e-3 * 12345 * 0.01
        _, e0, xi = REF.field(TERMS[name], x, masses, BOX, 0, 0.01)
        assert abs(e[2] - 0.5 * 700.0 * (xi[0] + 0.5 - 4.0e-3 * 123.45) ** 2) < 1e-9 and e0[2] != e[2]


def test_a_periodic_coordinate_takes_the_nearest_image():
    x, masses = _system()
    x[5:7, 0] += 0.55 * BOX[0]  # B beyond half a box from A in x
    x[0:3, 0] -= 0.05 * BOX[0]
    on, off = TERMS["distance-plain"], MartiniRestraints(pulls=[_coordinate(geometry="distance", periodic=True)])
    xi_plain, xi_img = REF.field(on, x, masses, BOX)[2][0], REF.field(off, x, masses, BOX)[2][0]
    assert xi_img < xi_plain - 0.5
    _gradient_check(off, x, masses)


def test_two_group_coordinates_exert_no_net_force():
    x, masses = _system()
    for name, rs in TERMS.items():
        if not rs.pulls or rs.pulls[0].group_a is None:
            continue
        F, _, _ = REF.field(rs, x, masses, BOX, 7, 0.01)
        assert np.abs(F.sum(0)).max() <= 1e-13 * np.abs(F).max(), name


def test_pbc_ref_gives_the_centre_of_the_unwrapped_group():
    rng = np.random.default_rng(8)
    masses = rng.uniform(40.0, 90.0, size=9)
    whole = np.array([3.0, 1.0, 3.7]) + rng.uniform(-0.4, 0.4, size=(9, 3))  # across the x and the z face
    wrapped = np.mod(whole, BOX)
    assert (wrapped != whole).any(0)[[0, 2]].all()
    com_whole, _ = REF.group_com(whole, masses, range(9))
    for ref in (0, 4):
        com, _ = REF.group_com(wrapped, masses, range(9), BOX, pbc_ref=ref)
        d = com - com_whole
        assert np.abs(d - BOX * np.round(d / BOX)).max() < 1e-12
    naive, _ = REF.group_com(wrapped, masses, range(9))
    assert np.abs(naive - com_whole).max() > 0.1
    # and through the lowered arrays
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=None, group_b=PullGroup(members=tuple(range(9)), pbc_ref=4), geometry="direction",
                                                 vec=(1, 0, 0), periodic=False)])
    a = rs.lower(n_rep=1, boxes=BOX)
    xi = CS.lowered_field(a, wrapped, masses, 0, 0.01, 0)[2][0]
    assert abs((xi - com_whole[0]) - BOX[0] * np.round((xi - com_whole[0]) / BOX[0])) < 1e-12


def test_lowering_three_replicas_with_per_replica_init():
    c, sets = CS.n257(), CS.sets()
    rs = sets["full"]
    a = rs.lower(n_rep=3, boxes=c["boxes"], reference_pos=c["ref"], masses=c["masses"])
    MR.check(c["n"], a)
    assert a["p_param"].shape == (3, 4, MR.PULL_PARAMS) and a["p_param"][:, 0, 1].tolist() == [0.4, 0.9, 1.3]
    assert a["p_param"][:, 1, 0].tolist() == [800.0, 1200.0, 50.0] and np.allclose(np.linalg.norm(a["p_param"][:, :, 3:6], axis=-1)[:, 1:3], 1.0)
    assert a["pr_ref"].shape == (3, 257, 3) and np.array_equal(a["pr_ref"][2, 1], c["ref"][2, 1])  # (odd beads: the loaded position)
    assert np.array_equal(a["pr_ref"][2, 0], a["pr_ref"][0, 0])  # (even beads: the reference given)
    sizes = np.diff(a["g_first"]).tolist()
    assert sorted(sizes) == [1, 1, 2, 2, 2, 3, 257] and a["p_groups"][2, 0] == -1
    for rep in range(3):
        x, box = c["pos"][rep], c["boxes"][rep]
        assert CS.minimum_image_margin(rs, x, c["masses"], box) > 0.02, "a minimum image too close to its flip"
        for s in (0, 12345):
            Fr, er, xr = REF.field(rs, x, c["masses"], box, s, CS.DT, rep, c["ref"][rep])
            Fl, el, xl = CS.lowered_field(a, x, c["masses"], s, CS.DT, rep)
            scale = np.abs(Fr).max()
            assert np.abs(Fr - Fl).max() <= 1e-12 * scale and np.abs(er - el).max() <= 1e-12 * np.abs(er).max() and np.abs(xr - xl).max() < 1e-13
            assert (er[:3] > 0).all() and er[3] != 0.0
    x0 = c["pos"][0]
    F0 = REF.field(MartiniRestraints(flat_bottom=rs.flat_bottom[-1:]), x0, c["masses"])
    assert not F0[0].any() and F0[1][1] == 0.5 * 300.0 * 0.2**2  # d = 0: the energy of the inverted sphere, no force
    # every term kind exerts a force somewhere, and HUB carries four kinds of term
    F_hub = [REF.field(MartiniRestraints(position=[p for p in rs.position if p.index == CS.HUB]), c["pos"][0], c["masses"], c["boxes"][0],
                       reference_pos=c["ref"][0])[0][CS.HUB],
             REF.field(MartiniRestraints(flat_bottom=[f for f in rs.flat_bottom if f.index == CS.HUB][:1]), c["pos"][0], c["masses"])[0][CS.HUB],
             REF.field(MartiniRestraints(flat_bottom=[f for f in rs.flat_bottom if f.index == CS.HUB][1:]), c["pos"][0], c["masses"])[0][CS.HUB],
             REF.field(MartiniRestraints(pulls=rs.pulls[:1]), c["pos"][0], c["masses"], c["boxes"][0])[0][CS.HUB],
             REF.field(MartiniRestraints(pulls=rs.pulls[1:2]), c["pos"][0], c["masses"], c["boxes"][0])[0][CS.HUB]]
    assert all(np.abs(f).max() > 0 for f in F_hub)
    # a scalar init serves every replica; a wrong length is refused
    one = MartiniRestraints(pulls=[_coordinate(init=0.7)]).lower(n_rep=3)
    assert one["p_param"][:, 0, 1].tolist() == [0.7] * 3
    with pytest.raises(ValueError, match="one per replica"):
        MartiniRestraints(pulls=[_coordinate(init=(0.1, 0.2))]).lower(n_rep=3)
    with pytest.raises(ValueError, match="no reference"):
        MartiniRestraints(position=[PositionRestraint(index=0)]).lower()


def test_from_mdp_and_read_ndx(tmp_path):
    ndx = tmp_path / "index.ndx"
    ndx.write_text("[ upper ]\n1 2 3\n4 5 ; a comment\n\n[ lower ]\n   11 12\n[ solute ]\n20\n")
    groups = MR.read_ndx(ndx)
    assert list(groups) == ["upper", "lower", "solute"] and groups["upper"].tolist() == [0, 1, 2, 3, 4] and groups["lower"].tolist() == [10, 11]
    mdp = {"pull": "yes", "pull-ngroups": "3", "pull-ncoords": 2, "pull-group1-name": "upper", "pull_group1_pbcatom": "3",
           "pull-group2-name": "lower", "pull-group3-name": "solute",
           "pull-coord1-type": "umbrella", "pull-coord1-geometry": "distance", "pull-coord1-groups": "1 2", "pull-coord1-dim": "N N Y",
           "pull-coord1-init": "1.5", "pull-coord1-rate": "0.001", "pull-coord1-k": "1000",
           "pull-coord2-type": "constant-force", "pull-coord2-geometry": "direction", "pull-coord2-groups": "0 3", "pull-coord2-vec": "0 0 2",
           "pull-coord2-k": "-50", "nsteps": 100}
    rs = MartiniRestraints.from_mdp(mdp, groups)
    c1, c2 = rs.pulls
    assert (c1.kind, c1.geometry, tuple(c1.dim), c1.init, c1.rate, c1.k) == ("umbrella", "distance", (False, False, True), 1.5, 0.001, 1000.0)
    assert c1.group_a.members == (0, 1, 2, 3, 4) and c1.group_a.pbc_ref == 2 and c1.group_b.members == (10, 11) and c1.group_b.pbc_ref is None
    assert c2.group_a is None and c2.group_b.members == (19,) and c2.kind == "constant-force" and c2.vec == (0.0, 0.0, 2.0) and c2.k == -50.0
    a = rs.lower(n_rep=2, boxes=BOX)
    MR.check(N, a)
    assert a["p_param"][0, 1, 3:6].tolist() == [0.0, 0.0, 1.0] and a["p_flags"].tolist() == [4 | (4 << 4), 1 | 2 | 4 | (7 << 4)]
    assert not MartiniRestraints.from_mdp({"pull": "no", "pull-ncoords": 1}, groups)
    for bad in ("pull-coord1-potential-provider", "pull-nstxout", "pull-cylinder-r", "pull-coord1-start"):
        with pytest.raises(ValueError, match=bad):
            MartiniRestraints.from_mdp(dict(mdp, **{bad: "1"}), groups)
    with pytest.raises(ValueError, match="not built"):
        MartiniRestraints.from_mdp(dict(mdp, **{"pull-coord1-geometry": "cylinder"}), groups)
    with pytest.raises(ValueError, match="not a group of the index"):
        MartiniRestraints.from_mdp(dict(mdp, **{"pull-group2-name": "nobody"}), groups)


def _good():
    rs = MartiniRestraints(position=[PositionRestraint(index=1, k=10.0, reference=(0, 0, 0))],
                           flat_bottom=[FlatBottomRestraint(index=2, r=0.5, k=10.0, reference=(0, 0, 0))],
                           pulls=[_coordinate(group_b=PullGroup(members=(5, 6), pbc_ref=6), geometry="direction")])
    return rs.lower(n_rep=2, boxes=BOX)


def test_every_refusal_names_its_reason_without_a_device():
    MR.check(N, _good())
    MR.check(N, MartiniRestraints().lower(n_rep=2), barostat=True, exchange=True)  # an empty set goes with anything

    def refused(match, edit=None, **kw):
        a = copy.deepcopy(_good())
        if edit:
            edit(a)
        with pytest.raises(ValueError, match=match):
            MR.check(N, a, **kw)

    def put(key, index, value):
        def edit(a):
            a[key][index] = value
        return edit

    refused(r"position restraint 0: index 24 out of range \[0, 24\)", put("pr_index", 0, N))
    refused(r"flat-bottom restraint 0: index -1 out of range", put("fb_index", 0, -1))
    refused(r"pull group 0: index 99 out of range", put("g_member", 0, 99))
    refused(r"pull group 1: duplicate member 5", put("g_member", 4, 5))
    refused(r"pull group 1: empty group", put("g_first", 2, 3))
    refused(r"pull coordinate 0: A = B", put("p_groups", (0, 0), 1))
    refused(r"position restraint 0: k < 0", put("pr_k", (0, 1), -1.0))
    refused(r"flat-bottom restraint 0: k < 0", put("fb_param", (1, 0, 0), -1.0))
    refused(r"pull coordinate 0: k < 0", put("p_param", (1, 0, 0), -1.0))
    refused(r"position restraint 0: non-finite value", put("pr_ref", (1, 0, 2), np.nan))
    refused(r"flat-bottom restraint 0: non-finite value", put("fb_param", (0, 0, 3), np.inf))
    refused(r"pull coordinate 0: non-finite value", put("p_param", (0, 0, 1), np.nan))
    refused(r"pull coordinate 0: zero vec", put("p_param", (1, 0, slice(3, 6)), 0.0))
    refused(r"flat-bottom restraint 0: r < 0", put("fb_param", (0, 0, 1), -0.1))
    refused(r"pull group 1: pbc_ref 7 is not a member", put("g_pbc_ref", 1, 7))
    refused(r"together with a barostat", barostat=True)
    refused(r"together with replica exchange", exchange=True)
    refused(r"box of replica 1", put("boxes", (1, 2), 0.0))

    def no_boxes(a):
        a["boxes"] = None
    refused(r"need the replicas' boxes", no_boxes)
    a = MartiniRestraints(pulls=[_coordinate(geometry="distance", dim=(False, False, False))]).lower(n_rep=1, boxes=BOX)
    with pytest.raises(ValueError, match=r"pull coordinate 0: empty dim"):
        MR.check(N, a)
    # a constant force may have either sign; an umbrella's k = 0 and a restraint's k = 0 are allowed
    MR.check(N, MartiniRestraints(pulls=[_coordinate(kind="constant-force", k=-3.0)]).lower(n_rep=1, boxes=BOX))
    MR.check(N, MartiniRestraints(pulls=[_coordinate(k=0.0)], position=[PositionRestraint(index=0, k=0.0, reference=(0, 0, 0))]).lower(n_rep=1, boxes=BOX))


def test_term_lists_of_the_free_bead_window_case_fit_their_box():
    """The shapes of the GPU tests, checked here: the 257-bead replicas fit cut-off + skin, the free beads their 6 nm box."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    c = CS.n257()
    MartiniEnsembleIntegrator.check(c["n"], [2.27] * 3, r_cut=1.1, skin=0.25, boxes=c["boxes"])
    f = CS.free_beads(16)
    MartiniEnsembleIntegrator.check(f["n"], [2.5] * 64, r_cut=1.1, skin=1.0, boxes=f["box"])
    assert (f["pos"] > 1.4).all() and (f["pos"] < 4.6).all()
