"""Duplex-mechanics observables on the GPU (mythos_amd/csrc/duplex_obs.hip) against the numpy restatement of the
reference (tests/duplex_ref.py) and against the reference's own known answers.

 * the numbers of mythos/observables/tests/test_diameter.py:16-103 and test_stretch_torsion.py:17-57, 112-206 through the
   library, with zero site offsets (a site is then the centre, as in the reference's mocks);
 * thermal duplexes, oxDNA1 / oxDNA2 / oxRNA2 site geometry, free and periodic, fp64 and fp32 frames (read as they are,
   arithmetic in fp64: the same tolerance on the same inputs);
 * list sizes either side of one wavefront and of the workgroup; sets that ask for one column only;
 * RMSD: the target itself, a rotated and shifted copy, the mirror image (the reflection branch), noisy frames;
 * sigma_backbone with a gradient; argument errors.
"""

import math

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy.base import Quaternion, RigidBody, space
from mythos_amd.input import defaults
from mythos_amd.observables import RMSE, Diameter, ExtensionZ, TwistXY, get_duplex_quartets
from mythos_amd.observables import base as PB
from mythos_amd.simulators.io import SimulatorTrajectory
from mythos_amd.utils import generators
from tests import duplex_ref as DR
from tests import helpers as H
from tests.test_gpu_observables import _thermal_duplex

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _traj(centers, quats=None, frames=1, dtype=torch.float64):
    c = np.asarray(centers, dtype=np.float64)
    c = np.repeat(c[None], frames, 0) if c.ndim == 2 else c
    if quats is None:
        quats = np.zeros((*c.shape[:2], 4))
        quats[..., 0] = 1.0
    return SimulatorTrajectory(center=torch.as_tensor(c, dtype=dtype, device=DEV), orientation=Quaternion(vec=torch.as_tensor(quats, dtype=dtype, device=DEV)))


def _np64(traj):
    return traj.center.double().cpu().numpy(), traj.orientation.vec.double().cpu().numpy()


def _pairs(bp):
    return np.stack([np.arange(bp), 2 * bp - 1 - np.arange(bp)], axis=1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_references_known_answers_through_the_library(dtype):
    disp = space.free()[0]
    d = Diameter(np.array([[0, 1], [1, 2]]), disp, H.ZERO_GEOMETRY)(_traj([[0, 0, 0], [1, 1, 1], [2, 2, 2]], frames=5, dtype=dtype), 1.0)
    assert d.dtype == torch.float64 and d.shape == (5,)
    np.testing.assert_allclose(d.cpu().numpy(), [23.271608] * 5, rtol=1e-7)
    ext = [([[0, 0, 0], [2, 0, 0], [0, 0, 5], [2, 0, 5]], 5.0), ([[0, 0, 10], [2, 0, 10], [0, 0, 3], [2, 0, 3]], 7.0),
           ([[0, 0, 5], [2, 0, 5], [4, 0, 5], [6, 0, 5]], 0.0), ([[0, 0, 0], [2, 0, 0], [0, 0, 10], [2, 0, 10]], 10.0)]
    for centers, want in ext:
        got = ExtensionZ([0, 1], [2, 3], disp)(_traj(centers, frames=3, dtype=dtype))
        np.testing.assert_allclose(got.cpu().numpy(), [want] * 3, atol=1e-6)
    tw = [([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], 0.0), ([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 1]], math.pi / 2),
          ([[0, 0, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 1]], math.pi)]
    for centers, want in tw:
        got = TwistXY(np.array([[[0, 1], [2, 3]]]), disp, H.ZERO_GEOMETRY)(_traj(centers, frames=2, dtype=dtype))
        np.testing.assert_allclose(got.cpu().numpy(), [want] * 2, atol=1e-6)
    # a pair along z has no direction in the x-y plane: NaN, as the reference's division gives
    nan = TwistXY(np.array([[[0, 1], [2, 3]]]), disp, H.ZERO_GEOMETRY)(_traj([[0, 0, 0], [0, 0, 1], [0, 0, 1], [1, 0, 1]], dtype=dtype))
    assert torch.isnan(nan).all()


def _check_all_columns(top, traj, bp, model, periodic, target):
    _, cfg = defaults.default_configs_for(H.model_dir(model))
    geo = cfg["geometry"]
    g3 = PB._geometry3(geo, model)
    box = 20.0 if periodic else None
    disp = space.periodic(20.0)[0] if periodic else space.free()[0]
    pairs, quartets = _pairs(bp), get_duplex_quartets(bp).numpy()
    bp1, bp2 = pairs[0], pairs[-1]
    c, q = _np64(traj)
    sigma = 0.7
    checks = [
        (Diameter(pairs, disp, geo, model)(traj, sigma), DR.diameter(c, q, pairs, g3, model, sigma, box)),
        (ExtensionZ(bp1, bp2, disp)(traj), DR.extension_z(c, bp1, bp2, box)),
        (TwistXY(quartets, disp, geo, model)(traj), DR.twist_xy(c, q, quartets, g3, model, box)),
        (RMSE(RigidBody(center=torch.as_tensor(target), orientation=None))(traj), DR.rmsd(target, c) * DR.ANGSTROMS_PER_OXDNA_LENGTH),
    ]
    for got, want in checks:
        assert got.dtype == torch.float64 and got.device.type == "cuda" and got.shape == want.shape
        assert np.abs(want).max() > 1e-3
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-10)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("model", [1, 2, 3])
def test_thermal_duplexes_match_the_numpy_restatement(model, periodic, dtype):
    bp = 23
    shift = [19.0, 18.5, 17.0] if periodic else None  # the helix crosses the faces of a 20-unit box (unwrapped coordinates)
    top, traj = _thermal_duplex(bp, 7, model=model, seed=3, dtype=dtype, shift=shift)
    _, c0, _ = generators.ideal_duplex(bp, model=model, seed=3)
    _check_all_columns(top, traj, bp, model, periodic, c0)


@pytest.mark.parametrize(("bp", "frames"), [(2, 4), (70, 2), (300, 3)])
def test_list_sizes_across_the_wavefront_and_the_workgroup(bp, frames):
    """1 quartet (and, below, 1 pair); 70 bp: the first size on 256 threads; 300 bp: strided loops, n = 600."""
    top, traj = _thermal_duplex(bp, frames, seed=11)
    _, c0, _ = generators.ideal_duplex(bp, seed=11)
    _check_all_columns(top, traj, bp, 2, False, c0)
    if bp == 2:
        _, cfg = defaults.default_configs_for("dna2")
        c, q = _np64(traj)
        got = Diameter(np.array([[1, 2]]), space.free()[0], cfg["geometry"])(traj, 0.0)
        np.testing.assert_allclose(got.cpu().numpy(), DR.diameter(c, q, [[1, 2]], PB._geometry3(cfg["geometry"], 2), 2, 0.0), rtol=0, atol=1e-10)


def test_a_set_with_one_column_leaves_the_others_zero():
    bp = 9
    top, traj = _thermal_duplex(bp, 3, seed=2)
    _, cfg = defaults.default_configs_for("dna2")
    disp = space.free()[0]
    _, c0, _ = generators.ideal_duplex(bp, seed=2)
    one = [(Diameter(_pairs(bp), disp, cfg["geometry"]), PB.COL_BACKBONE_DISTANCE), (ExtensionZ(_pairs(bp)[0], _pairs(bp)[-1], disp), PB.COL_EXTENSION),
           (TwistXY(get_duplex_quartets(bp), disp, cfg["geometry"]), PB.COL_TWIST), (RMSE(RigidBody(center=torch.as_tensor(c0), orientation=None)), PB.COL_RMSD)]
    for obs, col in one:
        rows = obs.rows(traj)
        assert rows.shape == (3, PB.DUPLEX_ROW)
        for k in range(PB.DUPLEX_ROW):
            assert (rows[:, k].abs().min() > 1e-3) if k == col else torch.equal(rows[:, k], torch.zeros_like(rows[:, k])), (col, k)
        assert len(obs._sets) == 1
        obs.rows(traj)
        assert len(obs._sets) == 1  # one set per (object, n, device), kept
    empty = PB.DuplexSet(2 * bp, 2, None, None, device=DEV).eval(traj.center, traj.orientation.vec)
    assert torch.equal(empty, torch.zeros_like(empty))
    zero = SimulatorTrajectory(center=traj.center[:0], orientation=Quaternion(vec=traj.orientation.vec[:0]))
    assert one[1][0](zero).shape == (0,)


@pytest.mark.parametrize("bp", [23, 300])
def test_rmsd_after_optimal_superposition(bp):
    """n = 46 and n = 600.  The target itself and a rotated, shifted copy come back to it (<= 1e-10); the mirror image of
    the (chiral) duplex does not - the best PROPER rotation is wanted, the reflection branch of the reference's SVD -
    and equals the restatement; so do noisy frames."""
    _, t, _ = generators.ideal_duplex(bp, seed=5)
    rng = np.random.default_rng(bp)
    a, b = 0.9, -0.4
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    moved = t @ (rz @ rx).T + [5.0, -3.0, 8.0]
    mirror = t * [-1.0, 1.0, 1.0]
    noisy = t[None] + 0.1 * rng.standard_normal((3, *t.shape))
    frames = np.concatenate([t[None], moved[None], mirror[None], noisy])
    rmse = RMSE(RigidBody(center=torch.as_tensor(t), orientation=None))
    got = rmse(_traj(frames)).cpu().numpy() / DR.ANGSTROMS_PER_OXDNA_LENGTH
    want = DR.rmsd(t, frames)
    print("rmsd", got, want)
    assert got[0] <= 1e-10 and got[1] <= 1e-10
    assert got[2] > 0.1 and want[2] > 0.1
    np.testing.assert_allclose(got[2:], want[2:], rtol=0, atol=1e-10)
    # fp32 frames: the same numbers from the same (rounded) inputs
    f32 = _traj(frames, dtype=torch.float32)
    np.testing.assert_allclose(rmse(f32).cpu().numpy() / DR.ANGSTROMS_PER_OXDNA_LENGTH, DR.rmsd(t, f32.center.double().cpu().numpy()), rtol=0, atol=1e-10)


def test_rmse_keeps_the_references_error_messages():
    with pytest.raises(ValueError, match="the target state must be a single conformation"):
        RMSE(RigidBody(center=torch.zeros(2, 5, 3), orientation=None))
    with pytest.raises(ValueError, match=r"center positions in \(x, y, z\) format"):
        RMSE(RigidBody(center=torch.zeros(5, 2), orientation=None))
    with pytest.raises(ValueError, match="displacement function is required"):
        Diameter(np.array([[0, 1]]), None, H.ZERO_GEOMETRY)


def test_diameter_is_differentiable_in_sigma_backbone():
    bp = 12
    top, traj = _thermal_duplex(bp, 5, seed=4)
    _, cfg = defaults.default_configs_for("dna2")
    sigma = torch.tensor(0.7, dtype=torch.float64, device=DEV, requires_grad=True)
    d = Diameter(_pairs(bp), space.free()[0], cfg["geometry"])(traj, sigma)
    (g,) = torch.autograd.grad(d.mean(), sigma)
    assert float(g) == pytest.approx(8.518, rel=1e-14)


def test_argument_errors():
    top, traj = _thermal_duplex(8, 2)
    _, cfg = defaults.default_configs_for("dna2")
    disp = space.free()[0]
    with pytest.raises(_lib.MythosHipError, match="out of range"):
        Diameter(np.array([[0, 99]]), disp, cfg["geometry"])(traj, 0.7)
    with pytest.raises(_lib.MythosHipError, match="out of range"):
        TwistXY(np.array([[[0, 1], [2, 16]]]), disp, cfg["geometry"])(traj)
    with pytest.raises(_lib.MythosHipError, match="out of range"):
        ExtensionZ([0, 15], [7, -1], disp)(traj)
    cpu = SimulatorTrajectory(center=traj.center.cpu(), orientation=Quaternion(vec=traj.orientation.vec.cpu()))
    with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
        ExtensionZ([0, 15], [7, 8], disp)(cpu)
    with pytest.raises(ValueError, match="nucleotides"):
        RMSE(RigidBody(center=torch.zeros(5, 3), orientation=None))(traj)


def test_a_duplex_set_gives_its_handle_back_once():
    """close() any number of times, then the finaliser: one mythos_duplex_obs_destroy, by name (test_gpu_api.py makes
    the check of every handle class; this one reaches Handle through the base it shares with ObservableSet)."""
    s = PB.DuplexSet(16, 2, None, None, end_pairs=[0, 15, 7, 8], device=DEV)
    assert isinstance(s, _lib.Handle) and s._h and s._destroy == "mythos_duplex_obs_destroy"

    class Counting:
        def __init__(self, lib):
            self.lib, self.destroyed = lib, []

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if not name.endswith("_destroy"):
                return fn
            return lambda h: (self.destroyed.append(name), fn(h))[1]

    spy = s._lib = Counting(s._lib)
    s.close()
    assert s._h is None and spy.destroyed == ["mythos_duplex_obs_destroy"]
    s.close()
    s.__del__()
    assert spy.destroyed == ["mythos_duplex_obs_destroy"]


def test_the_energy_call_refuses_a_duplex_set():
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.hip_system import OxdnaSystem

    top, traj = _thermal_duplex(8, 2)
    sim, cfg = defaults.default_configs_for("dna2")
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, dtype=torch.float64)
    s.set_params(fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=True), _lib.param_names()))
    s.set_neighbors(top.unbonded_neighbors)
    with pytest.raises(ValueError, match="not evaluated in the energy call"):
        s.energy(traj.center, traj.orientation.vec, observables=PB.DuplexSet(16, 2, None, None, end_pairs=[0, 15, 7, 8], device=DEV))
