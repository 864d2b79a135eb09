"""Host-side behaviour of the MARTINI observables, the Wasserstein argument checks and the composed MARTINI energy
function (no GPU): name matching and the reference's error texts (mythos/observables/bond_distances.py:41-49,
triplet_angles.py:64-71, wasserstein.py:29-40), parameter routing."""

import numpy as np
import pytest
import torch

from mythos_amd.energy import martini as M
from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables import (BondDistances, BondDistancesMapped, TripletAngles, TripletAnglesMapped,
                                    WassersteinDistanceMapped, wasserstein_1d)
from tests import martini_helpers as MH


def _top():
    return MartiniTopology(atom_types=("Q0", "Qa", "Na", "Na"), atom_names=("NC3", "PO4", "GL1", "GL2"),
                           residue_names=("DMPC",) * 4, angles=np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int32),
                           bonded_neighbors=np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int32))


def test_bond_names_select_the_matching_pairs():
    s = MH.system()
    obs = BondDistancesMapped(topology=s["top"], bond_names=("DMPC_GL1_GL2", "DMPC_NC3_PO4"))
    lists = obs.index_lists()
    names = s["top"].bond_names
    for name, idx in zip(obs.names, lists):
        assert idx.shape == (128, 2)
        want = s["top"].bonded_neighbors[[i for i, n in enumerate(names) if n == name]]
        assert np.array_equal(idx, want)
    single = BondDistances(topology=s["top"], bond_name="DMPC_GL1_GL2")
    assert single.names == ("DMPC_GL1_GL2",) and np.array_equal(single.index_lists()[0], lists[0])


def test_angle_names_select_the_matching_triplets():
    s = MH.system()
    names = sorted(set(s["top"].angle_names))
    assert len(names) == 6
    obs = TripletAnglesMapped(topology=s["top"], angle_names=tuple(names))
    assert [ix.shape for ix in obs.index_lists()] == [(128, 3)] * 6
    assert TripletAngles(topology=s["top"], angle_name=names[0]).index_lists()[0].shape == (128, 3)


def test_unknown_names_raise_the_reference_error_text():
    top = _top()
    traj = None  # never reached: the name check comes first
    with pytest.raises(ValueError, match=r"No bonds matching 'DMPC_X_Y' found in the topology\. Available bond names: "
                                         r"\['DMPC_GL1_GL2', 'DMPC_NC3_PO4', 'DMPC_PO4_GL1'\]"):
        BondDistances(topology=top, bond_name="DMPC_X_Y")(traj)
    with pytest.raises(ValueError, match="No bonds matching 'nope'"):
        BondDistancesMapped(topology=top, bond_names=("DMPC_NC3_PO4", "nope"))(traj)
    with pytest.raises(ValueError, match=r"No angles matching 'DMPC_A_B_C' found in the topology\. Available angle names: "
                                         r"\['DMPC_NC3_PO4_GL1', 'DMPC_PO4_GL1_GL2'\]"):
        TripletAngles(topology=top, angle_name="DMPC_A_B_C")(traj)
    with pytest.raises(ValueError, match="No angles matching 'nope'"):
        TripletAnglesMapped(topology=top, angle_names=("nope",))(traj)


def test_trajectory_without_box_raises():
    class T:
        center = torch.zeros((1, 4, 3))
        box_size = None

    with pytest.raises(ValueError, match="box_size"):
        BondDistances(topology=_top(), bond_name="DMPC_NC3_PO4")(T())


def test_wasserstein_argument_errors_come_before_any_device_work():
    """wasserstein.py:29-40, as mythos/observables/tests/test_wasserstein.py:103-126 provokes them."""
    with pytest.raises(ValueError, match="u_weights must have the same shape as u"):
        wasserstein_1d(np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0]), u_weights=np.array([0.5, 0.5]))
    with pytest.raises(ValueError, match="v_weights must have the same shape as v"):
        wasserstein_1d(np.array([1.0, 2.0]), np.array([3.0, 4.0, 5.0]), v_weights=np.array([0.5, 0.5]))
    with pytest.raises(ValueError, match="must sum to the same total mass"):
        wasserstein_1d(np.array([1.0, 2.0]), np.array([3.0, 4.0]), u_weights=np.array([0.3, 0.7]), v_weights=np.array([0.2, 0.2]))
    with pytest.raises(ValueError, match="gradients with respect to the sample values"):
        wasserstein_1d(torch.tensor([1.0, 2.0], requires_grad=True), np.array([3.0, 4.0]))


def test_mapped_v_weights_shape_is_checked_on_the_host():
    wd = WassersteinDistanceMapped(observable=lambda t: {"a": None}, v_distribution_map={"a": np.array([1.0, 2.0, 3.0])},
                                   v_weights_map={"a": np.array([0.5, 0.5])})
    with pytest.raises(ValueError, match="v_weights must have the same shape as v"):
        wd(None)


def _composed(strict=True):
    s = MH.system()
    bond = M.Bond.from_topology(topology=s["top"], params=M.BondConfiguration(**s["bond_params"]))
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    angle = M.Angle.from_topology(topology=s["top"], params=M.AngleConfiguration(**ap))
    return M.MartiniComposedEnergyFunction([bond, angle], strict_params=strict), s


def test_composed_with_params_routes_keys_to_the_terms_that_hold_them():
    fn, s = _composed()
    new = fn.with_params({"bond_k_DMPC_GL1_GL2": 1234.0}, angle_k_DMPC_PO4_GL1_GL2=55.0)
    bond, angle = new.energy_fns
    assert bond.params["bond_k_DMPC_GL1_GL2"] == 1234.0 and "angle_k_DMPC_PO4_GL1_GL2" not in bond.params
    assert angle.params["angle_k_DMPC_PO4_GL1_GL2"] == 55.0 and "bond_k_DMPC_GL1_GL2" not in angle.params
    # the original is untouched, every other value carried over
    assert fn.energy_fns[0].params["bond_k_DMPC_GL1_GL2"] == s["bond_params"]["bond_k_DMPC_GL1_GL2"]
    assert bond.params["bond_r0_DMPC_GL1_GL2"] == s["bond_params"]["bond_r0_DMPC_GL1_GL2"]
    assert set(fn.opt_params()) == set(s["bond_params"]) | set(s["angle_params"])
    assert set(fn.params_dict()) == set(fn.opt_params())
    assert all(f.dtype == torch.float32 for f in fn.with_props(dtype=torch.float32).energy_fns)


def test_composed_unused_keys_raise_only_when_strict():
    fn, _ = _composed(strict=True)
    with pytest.raises(ValueError, match="not used in any energy function"):
        fn.with_params(lj_sigma_Q0_Qa=0.5)
    loose, _ = _composed(strict=False)
    out = loose.with_params(lj_sigma_Q0_Qa=0.5, bond_k_DMPC_GL1_GL2=7.0)
    assert out.energy_fns[0].params["bond_k_DMPC_GL1_GL2"] == 7.0
    with pytest.raises(TypeError):
        M.MartiniComposedEnergyFunction([])
