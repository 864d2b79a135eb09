"""The frame-observable kernels across a launch boundary: a call with more frames than one launch takes is cut by the
shared chunk loop (mythos_amd/csrc/mythos_internal.h, for_frame_chunks), and the frame offset of every later launch
comes from it - for martini_obs through blockIdx.y + frame0 (32 768 frames per launch), for membrane and the duplex
observables through blockIdx.x + frame0 (2^20), for mythos_observables_eval through offset frame, row and axis-scratch
pointers (2^20).

Each test runs the smallest system that has every list, on chunk + 2 or + 3 frames made on the device by a seeded
generator, and takes the rows of frames 0, chunk - 1, chunk and the last one.  They must be, bit for bit, the rows of
those four frames evaluated as a batch of four (one launch, frame0 = 0: another route through the chunk logic), and
match the NumPy / torch restatements at the tolerances of the neighbouring tests of each unit.
"""

import numpy as np
import pytest
import torch

from mythos_amd.energy.base import Quaternion, space
from mythos_amd.input import defaults
from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables import BondDistancesMapped, MembraneThickness, TripletAnglesMapped, get_duplex_quartets
from mythos_amd.observables import base as PB
from mythos_amd.simulators.io import SimulatorTrajectory
from mythos_amd.utils import generators
from oracle import observables_oracle as OO
from tests import duplex_ref as DR
from tests import membrane_ref as MR
from tests.test_gpu_martini_observables import ref_angles, ref_bonds

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MARTINI_CHUNK = 32768  # martini_obs.hip: the frame is blockIdx.y
FRAME_CHUNK = 1 << 20  # kFramesPerLaunch of mythos_internal.h: the frame is blockIdx.x


def _picked(chunk, n_frames):
    return torch.tensor([0, chunk - 1, chunk, n_frames - 1], device=DEV)


def _noise(shape, dtype, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(shape, dtype=dtype, device=DEV, generator=g)


def _martini_traj(x, box):
    q = torch.zeros((x.shape[0], x.shape[1], 4), dtype=x.dtype, device=DEV)
    q[..., 0] = 1.0
    return SimulatorTrajectory(center=x, orientation=Quaternion(vec=q), box_size=box)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_martini_geometry_across_the_launch_boundary(dtype):
    """3 beads, one bond group, one angle group, a box of its own per frame (the bond crosses a face in most of them)."""
    n_frames = MARTINI_CHUNK + 3
    top = MartiniTopology(atom_types=("P",) * 3, atom_names=("A", "B", "C"), residue_names=("MOL",) * 3,
                          angles=np.array([[0, 1, 2]], dtype=np.int32), bonded_neighbors=np.array([[0, 1]], dtype=np.int32))
    bond, angle = top.bond_names[0], top.angle_names[0]
    base = torch.tensor([[0.1, 0.2, 0.3], [0.55, 0.25, 0.2], [0.8, 0.7, 0.1]], dtype=dtype, device=DEV)
    x = base[None] + 0.05 * _noise((n_frames, 3, 3), dtype, 1)
    box = 1.2 + 0.1 * torch.rand((n_frames, 3), dtype=dtype, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    x[:, 1, 0] += box[:, 0]  # the middle bead as its image one box further: bond and angle need the minimum image
    bonds, angles = BondDistancesMapped(topology=top, bond_names=(bond,)), TripletAnglesMapped(topology=top, angle_names=(angle,))
    pick = _picked(MARTINI_CHUNK, n_frames)
    full, four = _martini_traj(x, box), _martini_traj(x[pick].contiguous(), box[pick].contiguous())
    xs, bs = x[pick].double().cpu().numpy(), box[pick].double().cpu().numpy()
    for obs, name, ref in ((bonds, bond, ref_bonds(xs, bs, top.bonded_neighbors)), (angles, angle, ref_angles(xs, bs, top.angles))):
        rows = obs(full)[name]
        assert rows.shape == (n_frames, 1) and rows.dtype == torch.float64
        assert torch.equal(rows[pick], obs(four)[name])
        err = np.abs(rows[pick].cpu().numpy() - ref).max()
        print(f"{name} {dtype}: max |value - restatement| = {err:.3e}")
        assert err <= 1e-12
    assert (np.abs(xs[:, 0, 0] - xs[:, 1, 0]) > 0.5 * bs[:, 0]).all()  # the minimum image is at work in the picked frames


def test_membrane_across_the_launch_boundary():
    """4 beads in 2 lipids (both beads are of the lipid selection, one per lipid of the thickness selection), leaflets."""
    n_frames = FRAME_CHUNK + 2
    top = MartiniTopology(atom_types=("P",) * 4, atom_names=("PO4", "GL1", "PO4", "GL1"), residue_names=("LIP",) * 4,
                          angles=np.zeros((0, 3), dtype=np.int32), bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                          residue_index=np.array([0, 0, 1, 1]))
    base = torch.tensor([[1.0, 1.0, 3.0], [1.0, 1.0, 2.5], [2.0, 2.0, 1.0], [2.0, 2.0, 1.5]], dtype=torch.float32, device=DEV)
    x = base[None] + 0.1 * _noise((n_frames, 4, 3), torch.float32, 3)
    box = 4.0 + torch.rand((n_frames, 3), dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    thick = MembraneThickness(topology=top, lipid_sel="name PO4 GL1", thickness_sel="name PO4")
    pick = _picked(FRAME_CHUNK, n_frames)
    full, four = _martini_traj(x, box), _martini_traj(x[pick].contiguous(), box[pick].contiguous())
    rows, leaf = thick.rows(full), thick.leaflets(full)
    assert rows.shape == (n_frames, 7) and leaf.shape == (n_frames, 2) and leaf.dtype == torch.int8
    assert torch.equal(rows[pick], thick.rows(four)) and torch.equal(leaf[pick], thick.leaflets(four))
    ref = MR.membrane(x[pick].double().cpu().numpy(), box[pick].double().cpu().numpy(), top.residue_index,
                      MR.mask(top, ("PO4", "GL1")), MR.mask(top, ("PO4",)))
    got = rows[pick].cpu().numpy()
    assert np.array_equal(leaf[pick].cpu().numpy(), ref["leaflets"]) and ref["leaflets"].tolist() == [[1, -1]] * 4
    assert np.array_equal(got[:, 3], ref["n_up"]) and np.array_equal(got[:, 4], ref["n_lo"])
    for col, key in ((0, "thickness"), (2, "mid"), (5, "z_up"), (6, "z_lo")):
        err = np.abs(got[:, col] - ref[key]).max()
        print(f"max |{key} - restatement| = {err:.3e} nm")
        assert err <= 1e-10  # Z_ATOL of test_gpu_membrane.py
    assert np.abs(got[:, 1] / ref["apl"] - 1.0).max() <= 1e-12  # its AREA_RTOL


def _duplex_frames(n_frames):
    """A 4-nt duplex (2 base pairs, 1 quartet) with thermal noise, fp32, made on the device; the ideal centres too."""
    top, c0, q0 = generators.ideal_duplex(2, model=2, seed=5)
    c = torch.as_tensor(c0, dtype=torch.float32, device=DEV)[None] + 0.08 * _noise((n_frames, 4, 3), torch.float32, 6)
    q = torch.as_tensor(q0, dtype=torch.float32, device=DEV)[None] + 0.06 * _noise((n_frames, 4, 4), torch.float32, 7)
    q /= q.norm(dim=-1, keepdim=True)
    return c, q, c0


PAIRS = np.array([[0, 3], [1, 2]])


def test_duplex_observables_across_the_launch_boundary():
    n_frames = FRAME_CHUNK + 2
    c, q, c0 = _duplex_frames(n_frames)
    _, cfg = defaults.default_configs_for("dna2")
    quartets = get_duplex_quartets(2).numpy()
    s = PB.DuplexSet(4, 2, cfg["geometry"], None, PAIRS, quartets, end_pairs=[0, 3, 1, 2], target=c0 - c0.mean(0), device=DEV)
    pick = _picked(FRAME_CHUNK, n_frames)
    rows = s.eval(c, q)
    assert rows.shape == (n_frames, PB.DUPLEX_ROW)
    assert torch.equal(rows[pick], s.eval(c[pick].contiguous(), q[pick].contiguous()))
    cs, qs, g3 = c[pick].double().cpu().numpy(), q[pick].double().cpu().numpy(), PB._geometry3(cfg["geometry"], 2)
    want = np.stack([DR.backbone_distance(cs, qs, PAIRS, g3, 2), DR.extension_z(cs, PAIRS[0], PAIRS[1]), DR.twist_xy(cs, qs, quartets, g3, 2),
                     DR.rmsd(c0, cs)], axis=1)
    assert np.abs(want).min() > 1e-3
    err = np.abs(rows[pick].cpu().numpy() - want).max(axis=0)
    print(f"max |row - restatement| per column = {err}")
    assert err.max() <= 1e-10  # the tolerance of test_gpu_duplex_obs.py


def test_observable_set_across_the_launch_boundary():
    """mythos_observables_eval: frames, rows and the axis scratch of the second launch are offset on the host."""
    n_frames = FRAME_CHUNK + 2
    c, q, _ = _duplex_frames(n_frames)
    _, cfg = defaults.default_configs_for("dna2")
    quartets, disp = get_duplex_quartets(2), space.free()[0]
    s = PB.ObservableSet(4, 2, cfg["geometry"], None, PAIRS, quartets, False, torch.float32, DEV)
    assert s.width == 5  # one quartet, skip_ends off: C(0) alone
    pick = _picked(FRAME_CHUNK, n_frames)
    rows = s.eval(c, q)
    assert rows.shape == (n_frames, 5)
    assert torch.equal(rows[pick], s.eval(c[pick].contiguous(), q[pick].contiguous()))
    ref = SimulatorTrajectory(center=c[pick].double().cpu(), orientation=Quaternion(vec=q[pick].double().cpu()))
    corr, l0 = OO.PersistenceLength(quartets, disp, cfg["geometry"], 2, skip_ends=False).get_all_corrs_and_l0s(ref)
    want = torch.stack([OO.PropellerTwist(PAIRS)(ref), OO.Rise(quartets, disp, cfg["geometry"], 2)(ref),
                        OO.PitchAngle(quartets, disp, cfg["geometry"], 2)(ref), l0, corr[:, 0]], dim=1)
    assert want.abs().min() > 1e-3
    err = (rows[pick].cpu() - want).abs().max(dim=0).values
    print(f"max |row - oracle| per column = {err.tolist()}")
    assert err.max().item() <= 1e-10  # the tolerance of test_gpu_observables.py
