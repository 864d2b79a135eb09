"""GPU tests of the radial distribution function (mythos_amd/csrc/rdf.hip through ``RadialDistribution``): the kernel's
counts against the NumPy brute force of tests/rdf_ref.py, EXACTLY, at the smallest shapes at which the kernel can go
wrong - partial tiles of A and strips of B (256 beads each), the same / disjoint / overlapping lists, exclusion blocks
across a tile boundary, several groups in a handle, 1 to 4096 bins, a box per frame, the xy mask, more frames than a launch
takes - then the normalisation, the physics of an ideal gas, the r_max check and DiffTRe with an RDF loss.

Exact equality is fair because every case first asserts, on the CPU, that no admissible pair lies within 1e-7 bin
widths of a bin edge or of r_max (rdf_ref.MIN_MARGIN): host and device differ by an ulp or two in the image and the
square root, 1e-16 relative.  fp32 inputs are compared with the brute force on the same values cast up to double, which
is what the kernel computes.
"""

import dataclasses as dc
import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import martini as M
from mythos_amd.energy.base import Quaternion
from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables import RadialDistribution, RadialDistributionPair
from mythos_amd.optimization import objective as O
from mythos_amd.simulators.io import SimulatorTrajectory
from tests import martini_helpers as MH
from tests import rdf_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KT = 2.577  # kJ/mol, 310 K

# 300 beads: 37 A, 130 B, 90 C (A + B + C = 257: one bead more than a tile), 43 D
NAMES = ("A",) * 37 + ("B",) * 130 + ("C",) * 90 + ("D",) * 43
BOX = np.array([5.0, 5.3, 6.1])
BOX2 = np.tile(BOX, (2, 1))  # the two frames of _random_frames()


def _traj(x, box, dtype=torch.float64, temperature=None):
    x, box = np.asarray(x), np.asarray(box)
    q = torch.zeros((x.shape[0], x.shape[1], 4), dtype=dtype, device=DEV)
    q[..., 0] = 1.0
    t = None if temperature is None else torch.full((x.shape[0],), float(temperature), dtype=torch.float64, device=DEV)
    return SimulatorTrajectory(center=torch.as_tensor(x, dtype=dtype, device=DEV), orientation=Quaternion(vec=q),
                               box_size=torch.as_tensor(box, dtype=dtype, device=DEV), temperature=t)


def _top(names, block_size=1):
    n = len(names)
    return MartiniTopology(atom_types=("P",) * n, atom_names=tuple(names), residue_names=("MOL",) * n,
                           angles=np.zeros((0, 3), dtype=np.int32), bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                           residue_index=np.arange(n) // block_size)


@functools.lru_cache(maxsize=None)
def _random_frames(n_frames=2, seed=11, jitter=0.0, lz=BOX[2]):
    """Uniform beads in a non-cubic box; with ``jitter`` every frame has a box of its own."""
    rng = np.random.default_rng(seed)
    box = np.array([BOX[0], BOX[1], lz])[None, :] * (1.0 + jitter * rng.uniform(-1.0, 1.0, size=(n_frames, 3)))
    x = rng.uniform(0.0, 1.0, size=(n_frames, len(NAMES), 3)) * box[:, None, :]
    return x, box


def _lists(top, sels):
    from mythos_amd.observables.membrane import select

    return tuple(np.flatnonzero(select(top, s)) for s in sels)


def _check(obs, x, box, dtype=torch.float64):
    """The counts of every pair of ``obs`` on (x, box) equal the brute force's; -> (counts dict, reference dict)."""
    if dtype == torch.float32:
        x, box = np.asarray(x, dtype=np.float32), np.asarray(box, dtype=np.float32)
    got = obs.counts(_traj(x, box, dtype))
    block = None if obs.exclude is None else obs.topology.residue_index
    ref = {}
    for name, sels in obs._pairs().items():
        a, b = _lists(obs.topology, sels)
        ref[name], margin = R.counts(np.asarray(x, dtype=np.float64), np.asarray(box, dtype=np.float64), a, b, obs.n_bins, obs.r_max, block, obs.dims)
        print(f"{name} {dtype} n_bins {obs.n_bins}: {int(ref[name].sum())} counted pairs, margin {margin:.3e} bin widths")
        assert margin > R.MIN_MARGIN, (name, margin)
        c = got[name]
        assert c.dtype == torch.int64 and c.device.type == "cuda" and tuple(c.shape) == ref[name].shape
        assert np.array_equal(c.cpu().numpy(), ref[name]), name
        assert obs.n_pairs[name] == int(R.admissible(a, b, block).sum())
    (handle,) = obs.__dict__["_sets"].values()  # the library counted the same pairs when it made the handle
    assert handle.n_pairs == [obs.n_pairs[name] for name in obs.names]
    return got, ref


# ---- 1. fails without the feature --------------------------------------------------------------------------------------
def test_the_handle_exists_and_counts_one_pair():
    """``RadialDistribution`` imports and ``mythos_rdf_create`` gives a handle (neither exists on the parent commit): two
    beads 0.3 apart across the x face of a box of 4, both orders counted in bin 1 of 8 below 2."""
    lib = _lib.load()
    n_a, n_b, index = (np.array(v, dtype=np.int32) for v in ([2], [2], [0, 1, 0, 1]))
    h = lib.mythos_rdf_create(2, 1, n_a.ctypes.data_as(_lib.c_int_p), n_b.ctypes.data_as(_lib.c_int_p), index.ctypes.data_as(_lib.c_int_p),
                              None, 8, 2.0, 3, 0)
    assert h, _lib.last_error()
    lib.mythos_rdf_destroy(h)
    x, box = np.array([[[0.1, 1.0, 1.0], [3.8, 1.0, 1.0]]]), np.array([[4.0, 4.0, 4.0]])
    obs = RadialDistributionPair(topology=_top(("A", "A")), sel_a="name A", sel_b="name A", r_max=2.0, n_bins=8)
    assert obs.counts(_traj(x, box)).tolist() == [[0, 2, 0, 0, 0, 0, 0, 0]]
    g = obs(_traj(x, box))
    assert g.dtype == torch.float64 and g.shape == (1, 8)
    assert g[0, 1].item() == pytest.approx(2 * 64.0 / (2 * 4.0 / 3.0 * np.pi * (0.5 ** 3 - 0.25 ** 3)), rel=1e-13)


def test_the_handle_is_given_back_once():
    """close() twice and __del__ reach mythos_rdf_destroy once; the observable keeps one handle per device."""
    from mythos_amd.observables.rdf import _RdfSet

    destroyed = []

    class Counting:
        def __init__(self, lib):
            self.lib = lib

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            return fn if not name.endswith("_destroy") else (lambda h: (destroyed.append(name), fn(h))[1])

    rs = _RdfSet(4, [(np.array([0, 1]), np.array([2, 3]))], None, 8, 1.0, "xy", DEV)
    assert isinstance(rs, _lib.Handle) and rs._h and rs.n_pairs == [4]
    rs._lib = Counting(rs._lib)
    rs.close(), rs.close(), rs.__del__()
    assert rs._h is None and destroyed == ["mythos_rdf_destroy"]
    x, box = _random_frames()
    obs = RadialDistributionPair(topology=_top(NAMES), sel_a="name A", sel_b="name B", r_max=2.0, n_bins=50)
    obs.counts(_traj(x, BOX2)), obs.counts(_traj(x, BOX2, torch.float32))
    assert len(obs.__dict__["_sets"]) == 1


# ---- 2. partial tiles and strips, selections, blocks, groups ----------------------------------------------------------------
PAIRS = {"37x130 disjoint": ("name A", "name B"), "257 same": ("name A B C", "name A B C"),
         "167x220 overlapping": ("name A B", "name B C"), "130x37": ("name B", "name A"), "43 same": ("name D", "name D")}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_partial_tiles_and_strips_and_several_groups_in_one_handle(dtype):
    """|A| = 37 against |B| = 130, |A| = |B| = 257 (a second tile and a second strip of one bead), overlapping lists with
    A n B neither empty nor all - five groups of different lengths in one handle, each row its own group's."""
    x, box = _random_frames()
    obs = RadialDistribution(topology=_top(NAMES), pairs=PAIRS, r_max=2.0, n_bins=50)
    got, ref = _check(obs, x, BOX2, dtype)
    assert len({int(r.sum()) for r in ref.values()}) == 4  # the groups differ; the two orders of A, B agree
    assert torch.equal(got["37x130 disjoint"], got["130x37"])
    # each group alone gives the same rows
    for name in ("257 same", "167x220 overlapping"):
        alone = RadialDistributionPair(topology=_top(NAMES), sel_a=PAIRS[name][0], sel_b=PAIRS[name][1], r_max=2.0, n_bins=50)
        xs = x.astype(np.float32) if dtype == torch.float32 else x
        assert torch.equal(alone.counts(_traj(xs, BOX2, dtype)), got[name])


@pytest.mark.parametrize("block_size", [1, 3, 12])
def test_exclusion_blocks(block_size):
    """Residues of 1, 3 and 12 beads; beads 252 ... 263 share one of the 12, and positions 252 ... 256 of the 257-bead
    list lie on both sides of the tile boundary at 256."""
    x, box = _random_frames()
    top = _top(NAMES, block_size)
    obs = RadialDistribution(topology=top, pairs={k: PAIRS[k] for k in ("257 same", "167x220 overlapping", "37x130 disjoint")},
                             r_max=2.0, n_bins=50, exclude="residue")
    if block_size == 12:
        assert top.residue_index[252] == top.residue_index[256] == top.residue_index[263] != top.residue_index[251]
    got, _ = _check(obs, x, BOX2)
    free = dc.replace(obs, exclude=None).counts(_traj(x, BOX2))
    for name in ("257 same", "167x220 overlapping"):  # (the disjoint lists meet in one block only, at beads 36 | 37)
        assert torch.equal(got[name], free[name]) == (block_size == 1), name


# ---- 3. bins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 50, 257, 4096])
def test_bins_and_r_max_of_half_the_shortest_edge(n_bins):
    x, box = _random_frames()
    obs = RadialDistribution(topology=_top(NAMES), pairs={k: PAIRS[k] for k in ("257 same", "37x130 disjoint")},
                             r_max=0.5 * float(BOX.min()), n_bins=n_bins)
    _check(obs, x, BOX2)


def test_an_r_max_no_pair_reaches_gives_zeros():
    x, box = _random_frames()
    a, b = np.arange(37), np.arange(37, 167)
    closest = min(R.distances(x[f], BOX, a, b).min() for f in range(2))
    obs = RadialDistributionPair(topology=_top(NAMES), sel_a="name A", sel_b="name B", r_max=0.5 * float(closest), n_bins=16)
    traj = _traj(x, BOX2)
    assert not obs.counts(traj).any() and obs.counts(traj).shape == (2, 16)
    g = obs(traj)
    assert torch.equal(g, torch.zeros_like(g))


# ---- 4. a box per frame, the xy mask, the r_max check ------------------------------------------------------------------------
def _crossings(x, box, a, b, r_max, dims):
    """Per dimension: is there a counted pair whose raw difference exceeds half the edge (the image is at work)?"""
    k = {"xyz": 3, "xy": 2}[dims]
    seen = np.zeros(k, dtype=bool)
    for f in range(x.shape[0]):
        hit = (R.distances(x[f], box[f], a, b, dims) < r_max) & R.admissible(a, b)
        raw = np.abs(x[f][a][:, None, :k] - x[f][b][None, :, :k])
        seen |= (hit[..., None] & (raw > 0.5 * box[f][:k])).any((0, 1))
    return seen


def test_seventeen_frames_with_boxes_of_their_own():
    x, box = _random_frames(n_frames=17, seed=12, jitter=0.04)
    assert len({tuple(b) for b in box}) == 17
    obs = RadialDistribution(topology=_top(NAMES), pairs={k: PAIRS[k] for k in ("257 same", "37x130 disjoint")}, r_max=2.0, n_bins=50)
    for dtype in (torch.float64, torch.float32):
        _check(obs, x, box, dtype)
    assert _crossings(x, box, np.arange(37), np.arange(37, 167), 2.0, "xyz").all()
    # the normalisation uses each frame's own volume
    g = obs(_traj(x, box))["257 same"].cpu().numpy()
    c = obs.counts(_traj(x, box))["257 same"].cpu().numpy()
    assert np.allclose(g, R.g_of(c, box, obs.n_pairs["257 same"], 2.0), rtol=1e-13, atol=0.0)


def test_the_xy_mask_ignores_z_also_in_the_r_max_check():
    """Lz = 1.2 is far below 2 r_max = 4: the xyz form refuses the frames, the xy form counts them - in x and y alone."""
    x, box = _random_frames(n_frames=17, seed=13, jitter=0.04, lz=1.2)
    obs = RadialDistribution(topology=_top(NAMES), pairs={k: PAIRS[k] for k in ("257 same", "37x130 disjoint")}, r_max=2.0, n_bins=50,
                             dims="xy")
    _, ref = _check(obs, x, box)
    assert _crossings(x, box, np.arange(37), np.arange(37, 167), 2.0, "xy").all()
    a, b = np.arange(37), np.arange(37, 167)
    assert not np.array_equal(ref["37x130 disjoint"], R.counts(x, box, a, b, 50, 2.0)[0])  # z would have mattered
    c = obs.counts(_traj(x, box))["257 same"].cpu().numpy()
    assert np.allclose(obs(_traj(x, box))["257 same"].cpu().numpy(), R.g_of(c, box, obs.n_pairs["257 same"], 2.0, "xy"), rtol=1e-13, atol=0.0)
    with pytest.raises(ValueError, match=r"^frame 0: a box edge \(x, y, z\) is shorter than 2 r_max = 4.0"):
        dc.replace(obs, dims="xyz").counts(_traj(x, box))


@pytest.mark.parametrize("dims,edge", [("xyz", 0), ("xyz", 2), ("xy", 1)])
def test_a_frame_with_an_edge_below_two_r_max_is_an_argument_error(dims, edge):
    x, box = _random_frames(n_frames=17, seed=12, jitter=0.04)
    short = box.copy()
    short[11, edge] = 3.9
    short[14, edge] = 3.5  # the FIRST such frame is named
    obs = RadialDistributionPair(topology=_top(NAMES), sel_a="name A", sel_b="name B", r_max=2.0, n_bins=50, dims=dims)
    with pytest.raises(ValueError, match="^frame 11: a box edge"):
        obs(_traj(x, short))
    obs.counts(_traj(x, box))  # the device is as it was: the next call is served


# ---- 5. more frames than one launch takes -----------------------------------------------------------------------------------
RDF_CHUNK = 32768  # rdf.hip: the frame is blockIdx.y


def test_frames_across_the_launch_boundary():
    """8 beads (4 A, 4 B; A against A + B: overlapping lists), a box per frame, chunk + 3 frames in fp32: frames 0,
    chunk - 1, chunk and the last against the brute force, and equal to those four frames evaluated as a batch."""
    n_frames = RDF_CHUNK + 3
    rng = np.random.default_rng(5)
    box = (2.4 + rng.uniform(0.0, 0.5, size=(n_frames, 3))).astype(np.float32)
    x = (rng.uniform(0.0, 1.0, size=(n_frames, 8, 3)) * box[:, None, :]).astype(np.float32)
    top = _top(("A",) * 4 + ("B",) * 4)
    obs = RadialDistributionPair(topology=top, sel_a="name A", sel_b="name A B", r_max=1.2, n_bins=8)
    pick = np.array([0, RDF_CHUNK - 1, RDF_CHUNK, n_frames - 1])
    c = obs.counts(_traj(x, box, torch.float32))
    assert c.shape == (n_frames, 8)
    ref, margin = R.counts(x[pick].astype(np.float64), box[pick].astype(np.float64), np.arange(4), np.arange(8), 8, 1.2)
    print(f"margin {margin:.3e} bin widths; counted pairs per picked frame {ref.sum(1).tolist()}")
    assert margin > R.MIN_MARGIN and (ref.sum(1) > 0).all() and len({tuple(r) for r in ref.tolist()}) > 1
    assert np.array_equal(c[torch.as_tensor(pick, device=DEV)].cpu().numpy(), ref)
    assert torch.equal(obs.counts(_traj(x[pick], box[pick], torch.float32)), c[torch.as_tensor(pick, device=DEV)])
    assert int(c.sum()) > n_frames  # the frames between them were counted too


# ---- 6. the golden bilayer ----------------------------------------------------------------------------------------------------
GOLDEN_PAIRS = {"PO4-PO4": ("name PO4", "name PO4"), "PO4-GL": ("name PO4", "name GL1 GL2"), "C1-tails": ("name C1A C1B", "name C1A C2A C3A")}


@functools.lru_cache(maxsize=None)
def _golden_reference(exclude):
    top = MH.system()["top"]
    x, box, _ = MH.frames("lj")
    out = {}
    for name, sels in GOLDEN_PAIRS.items():
        a, b = _lists(top, sels)
        block = top.residue_index if exclude else None
        c, margin = R.counts(x, box, a, b, 200, 2.0, block)
        out[name] = (c, margin, int(R.admissible(a, b, block).sum()))
    return out


@pytest.mark.parametrize("exclude", [None, "residue"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_golden_bilayer_counts_and_g(exclude, dtype):
    top = MH.system()["top"]
    x, box, _ = MH.frames("lj")
    obs = RadialDistribution(topology=top, pairs=GOLDEN_PAIRS, r_max=2.0, n_bins=200, exclude=exclude)
    if dtype == torch.float64:
        ref = _golden_reference(exclude)
        got = obs.counts(_traj(x, box))
        g = obs(_traj(x, box))
        for name, (c, margin, n_pairs) in ref.items():
            print(f"{name} exclude={exclude}: {int(c.sum())} counted pairs of {n_pairs} x 10, margin {margin:.3e}")
            assert margin > R.MIN_MARGIN and obs.n_pairs[name] == n_pairs
            assert np.array_equal(got[name].cpu().numpy(), c), name
            assert np.allclose(g[name].cpu().numpy(), R.g_of(c, box, n_pairs, 2.0), rtol=1e-13, atol=0.0), name
        intra = _golden_reference(None)["PO4-GL"][0].sum() - ref["PO4-GL"][0].sum()
        assert (intra == 2 * 128 * 10) == (exclude == "residue")  # PO4 - GL1 and PO4 - GL2 of the same lipid lie inside 2 nm
    else:
        _check(obs, x, box, dtype)


# ---- 7. known physics -----------------------------------------------------------------------------------------------------------
def test_ideal_gas_has_g_of_one():
    """20 000 uniform beads in a box of 10 x 11 x 12, one frame, A = B, 40 bins below 2: the ordered count of a bin is
    twice a Poisson variable of mean m_b = N_pairs v_b / (2 V), so g_b has standard error 1 / sqrt(m_b) and the mean of
    g over the K bins above r = 0.5 has sqrt(sum 1 / m_b) / K.  It is 1 within 4 of those."""
    n = 20000
    rng = np.random.default_rng(2)
    box = np.array([[10.0, 11.0, 12.0]])
    x = rng.uniform(0.0, 1.0, size=(1, n, 3)) * box[:, None, :]
    obs = RadialDistributionPair(topology=_top(("W",) * n), sel_a="name W", sel_b="name W", r_max=2.0, n_bins=40)
    traj = _traj(x, box)
    c, g = obs.counts(traj)[0].cpu().numpy(), obs(traj)[0].cpu().numpy()
    assert obs.n_pairs == {"pair": n * (n - 1)} and (c % 2 == 0).all()
    far = obs.r > 0.5
    m = 0.5 * n * (n - 1) * obs.shell_volumes[far] / box.prod()
    se = np.sqrt((1.0 / m).sum()) / far.sum()
    print(f"mean g above 0.5: {g[far].mean():.6f}, standard error {se:.2e}, counted pairs {int(c.sum())}")
    assert abs(g[far].mean() - 1.0) <= 4.0 * se
    assert np.abs(g[far] - 1.0).max() <= 6.0 / np.sqrt(m.min())  # and no single bin is off


# ---- 8. reproducibility ---------------------------------------------------------------------------------------------------------
def test_counts_are_the_same_bits_from_run_to_run():
    top = MH.system()["top"]
    x, box, _ = MH.frames("lj")
    obs = RadialDistribution(topology=top, pairs=GOLDEN_PAIRS, r_max=2.0, n_bins=200, exclude="residue")
    traj = _traj(x, box, torch.float32)
    first = obs.counts(traj)
    for _ in range(3):
        again = obs.counts(traj)
        assert all(torch.equal(first[k], again[k]) for k in first)
    one = obs.counts(traj.slice(3))  # a frame alone has the rows it has in the batch
    assert all(torch.equal(one[k][0], first[k][3]) for k in first)
    with pytest.raises(ValueError, match="trajectory has 1280 beads, the topology 300"):
        RadialDistributionPair(topology=_top(NAMES), sel_a="name A", sel_b="name B", r_max=2.0, n_bins=50)(traj)


# ---- 9. DiffTRe -------------------------------------------------------------------------------------------------------------------
def test_gradient_of_a_reweighted_rdf_loss_with_respect_to_the_weights():
    top = MH.system()["top"]
    x, box, _ = MH.frames("lj")
    obs = RadialDistributionPair(topology=top, sel_a="name PO4", sel_b="name PO4", r_max=2.0, n_bins=200)
    g = obs(_traj(x, box))
    rng = np.random.default_rng(4)
    w = torch.as_tensor(rng.dirichlet(np.ones(10)), device=DEV).requires_grad_(True)
    target = torch.as_tensor(1.0 + 0.1 * rng.standard_normal(200), device=DEV)
    loss = ((w @ g - target) ** 2).mean()
    (grad,) = torch.autograd.grad(loss, w)
    closed = 2.0 * (w.detach() @ g - target) @ g.T / 200
    err, scale = (grad - closed).abs().max().item(), closed.abs().max().item()
    print(f"max |dloss/dw - closed form| = {err:.3e} of {scale:.3e}")
    assert scale > 1e-3 and err <= 1e-12 * scale


LJ_OPT = ("lj_epsilon_Qa_Qa", "lj_sigma_Qa_Qa", "lj_epsilon_Na_Qa", "lj_epsilon_C1_C1", "lj_sigma_C1_C1")


def test_difftre_objective_with_an_lj_energy_and_an_rdf_loss():
    """One DiffTReObjective.calculate on the golden frames: finite gradients with respect to LJ parameters, equal to those
    of the same objective with g built from the brute force's counts (only the observable differs between the two)."""
    s = MH.system()
    top = s["top"]
    x, box, _ = MH.frames("lj")
    assert all(n in s["lj_params"] for n in LJ_OPT)
    obs = RadialDistributionPair(topology=top, sel_a="name PO4", sel_b="name PO4", r_max=2.0, n_bins=200, exclude="residue")
    c_ref, margin, n_pairs = _golden_reference("residue")["PO4-PO4"]
    assert margin > R.MIN_MARGIN
    g_ref = torch.as_tensor(R.g_of(c_ref, box, n_pairs, 2.0), device=DEV)
    target = torch.as_tensor(np.where(obs.r > 0.45, 1.0, 0.0), device=DEV)

    def make_loss(g_of_traj):
        def loss_fn(traj, weights, *_):
            expected = weights @ g_of_traj(traj)
            return ((expected - target) ** 2).mean(), (("rdf", expected), ())
        return loss_fn

    efn = M.MartiniComposedEnergyFunction([M.LJ.from_topology(topology=top, params=M.LJConfiguration(**s["lj_params"]))])
    base = {n: float(s["lj_params"][n]) for n in LJ_OPT}
    opt = {n: 1.0005 * v for n, v in base.items()}
    traj = _traj(x, box, temperature=KT)
    outs = []
    for g_of_traj in (obs, lambda _traj: g_ref):
        obj = O.DiffTReObjective(name="rdf", required_observables=("traj",), grad_or_loss_fn=make_loss(g_of_traj), energy_fn=efn,
                                 min_n_eff_factor=0.1)
        out = obj.calculate({"traj": traj}, opt_params=opt, reference_opt_params=base)
        assert out.is_ready, out.observables
        outs.append(out)
    kernel, brute = outs
    print(f"loss {kernel.observables['loss'].item():.12e} (brute force {brute.observables['loss'].item():.12e}), n_eff {float(kernel.observables['neff']):.4f}")
    gmax = max(abs(brute.grads[n].item()) for n in LJ_OPT)
    assert gmax > 0.0
    for n in LJ_OPT:
        a, b = kernel.grads[n].item(), brute.grads[n].item()
        print(f"{n}: {a:.12e} brute force {b:.12e}")
        assert np.isfinite(a) and abs(a - b) <= 1e-12 * max(abs(b), gmax), n
    assert abs(kernel.observables["loss"].item() - brute.observables["loss"].item()) <= 1e-12 * abs(brute.observables["loss"].item())
