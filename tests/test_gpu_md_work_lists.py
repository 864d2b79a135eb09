"""The angular pass of md_step_kernel takes its work from two lists the radial pass fills: base-pair items (list 0) and
coaxial-stacking items (list 1).  The fixed-row fp32 instantiations of the single sweep (8 lanes per nucleotide, 16 result
rows) keep them as WAVE-DENSE lists - every wavefront appends what its eight nucleotides flag to one list per kind, and
the role wavefronts walk the four lists one after the other - the others keep one list per nucleotide and find item q
through a prefix scan and a search.  Which lane evaluates an item differs between the two; the result row of an item
(owner, slot within the owner's list) and the order of the fold do not, so nothing computed may depend on it.

What can go wrong sits in the list sizes, not in the system size: a list longer than one sweep of 64 lanes (several sweeps
per role), an odd split between the two base-pair wavefronts, wavefronts and nucleotides that contribute nothing, no item
at all, a last workgroup that is partly empty, and a wavefront's list that is full (64 items) while no nucleotide's is.

List sizes are counted on the CPU the way the radial pass flags entries (as
test_a_crowded_workgroup_exhausts_the_row_pool_and_the_step_reruns does) and asserted before anything runs.

Tolerances.  fp64: those of the existing step tests (tests/test_gpu_langevin.py, tests/test_gpu_edge_cases.py).  fp32 against
the fp64 oracle: per step the bound tests/test_gpu_md_row_sweep.py states for one step - centres and quaternions within two
roundings of their largest value, momenta within 40 (a row of at most 80 terms, each rounding half an ulp of the running
sum, which the largest momentum bounds) - times the number of steps plus one (the fp32 run re-normalises the rounded
quaternions it is handed; the oracle starts from them as they are).
"""

import functools
import types

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults, topology
from mythos_amd.utils import generators
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0
R_CUT = 3.3
SEED = 0x1234ABCD5678
INERTIA = (1.0, 1.3, 0.8)
WAVE_CAP = 64    # items per wavefront and list of the wave-dense lists
ROW_ROOM = 16    # result rows of one nucleotide for its flagged neighbours in the stepping instantiations
DTYPES = (torch.float64, torch.float32)
DT_IDS = ["f64", "f32"]
FP32_ULPS_PER_STEP = (2, 2, 40, 40)  # centres, quaternions, momenta, angular momenta


@functools.lru_cache(maxsize=None)
def _named():
    sim, cfg = defaults.default_configs_for("dna2")
    return fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=False), cfg


def _ball(n, radius, seed):
    """the generator of test_a_crowded_workgroup_exhausts_the_row_pool_and_the_step_reruns"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        v = rng.uniform(-radius, radius, 3)
        if np.linalg.norm(v) <= radius and all(np.linalg.norm(v - w) >= 0.27 for w in pts):
            pts.append(v)
    q0 = rng.standard_normal((n, 4))
    return np.array(pts), q0 / np.linalg.norm(q0, axis=1, keepdims=True)


def _fcc(n, d):
    """the n sites of a face-centred cubic lattice (nearest-neighbour distance d) closest to a point near the origin, inside out"""
    a, pts = d * np.sqrt(2.0), []
    for i in range(-3, 4):
        for j in range(-3, 4):
            for k in range(-3, 4):
                for b in ((0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)):
                    pts.append(a * (np.array([i, j, k], dtype=np.float64) + np.array(b)))
    pts = np.array(pts)
    order = np.argsort(np.linalg.norm(pts - np.array([0.01, 0.02, 0.03]), axis=1), kind="stable")
    return pts[order[:n]]


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(topology, centres, quaternions, dt, device-built rows?)"""
    if kind == "crowded":  # case 1: several sweeps per role
        c, q = _ball(32, 0.9, 21)
    elif kind == "sparse":  # case 2: empty lists among full ones
        c, q = _ball(32, 1.3, 5)
    elif kind == "lattice":  # a wavefront's list over its capacity, no nucleotide over its rows: parallel bases on an fcc
        # lattice of spacing 0.64 - twelve neighbours inside the cross-stacking support (0.45, 0.70), none inside the
        # coaxial one (below 0.622); ordered inside out, so the first wavefront's eight nucleotides hold the most
        c, q = _fcc(32, 0.64), np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (32, 1))
    elif kind == "apart":  # case 3: no item at all
        top = types.SimpleNamespace(seq=np.array([0, 3], dtype=np.int32), is_end=np.ones(2, dtype=np.int32),
                                    bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                                    unbonded_neighbors=np.array([[0, 1]], dtype=np.int32), n_nucleotides=2)
        return top, np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0, 0.0], [0.6, 0.0, 0.8, 0.0]]), 0.005, False
    else:  # case 4: 40 bp, 80 nt - two and a half workgroups of 32, five of 16
        assert kind == "duplex"
        top, c, q = generators.ideal_duplex(40, model=2, seed=3)
        return top, c, q, 0.005, True
    n = c.shape[0]
    # dt: overlapping sites push hard, a step must stay a small perturbation (as in the tests these systems come from)
    return topology.from_arrays(np.arange(n) % 4, [1] * n), c, q, 1e-9, False


def _list_counts(kind):
    """items of every nucleotide in list 0 and list 1, counted as the radial pass flags entries: base-base distance inside the
    cross-stacking support, or inside the H-bond support for a Watson-Crick pair; stacking-site distance inside the coaxial one"""
    from oracle import oxdna_oracle as orc

    top, c0, q0, _, _ = _case(kind)
    named, cfg = _named()
    n, g = c0.shape[0], cfg["geometry"]
    a1 = orc.quat_to_axes(torch.as_tensor(q0))[0].numpy()
    far = 9.0 * np.eye(n)
    db = np.linalg.norm((c0 + g["com_to_hb"] * a1)[:, None] - (c0 + g["com_to_hb"] * a1)[None], axis=-1) + far
    ds = np.linalg.norm((c0 + g["com_to_stacking"] * a1)[:, None] - (c0 + g["com_to_stacking"] * a1)[None], axis=-1) + far
    v = lambda k: float(named[k])  # noqa: E731
    seq = np.asarray(top.seq)
    wc = (seq[:, None] + seq[None]) == 3
    n0 = (((db > v("HYDR_RCLOW")) & (db < v("HYDR_RCHIGH")) & wc) | ((db > v("CRST_RCLOW")) & (db < v("CRST_RCHIGH")))).sum(1)
    n1 = ((ds > v("CXST_RCLOW")) & (ds < v("CXST_RCHIGH"))).sum(1)
    return n0, n1


def _integrator(kind, dtype, seed=SEED):
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    top, c0, q0, dt, device_rows = _case(kind)
    named, _ = _named()
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=None, dtype=dtype)
    s.set_params(fp.pack_flat(named, _lib.param_names()))
    integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, mass=1.0, inertia=INERTIA, seed=seed)
    if device_rows:
        integ.set_neighbor_policy(r_cut=R_CUT, skin=0.9, every=1000)
    else:
        s.set_neighbors(top.unbonded_neighbors)
    c = torch.as_tensor(c0, dtype=dtype, device=s.device).contiguous()
    q = torch.as_tensor(q0, dtype=dtype, device=s.device).contiguous()
    return s, integ, c, q


@functools.lru_cache(maxsize=None)
def _oracle_states(kind, n_steps, state_bytes):
    """the oracle's (x, q, p, L) after each step from the state the GPU run starts from; computed once, never written to"""
    from oracle.langevin_oracle import LangevinOracle

    top, c0, _, dt, _ = _case(kind)
    n = c0.shape[0]
    flat = np.frombuffer(state_bytes, dtype=np.float64)
    x, qq, pp, LL = (a.copy() for a in (flat[:3 * n].reshape(n, 3), flat[3 * n:7 * n].reshape(n, 4), flat[7 * n:10 * n].reshape(n, 3),
                                        flat[10 * n:].reshape(n, 3)))
    orc = LangevinOracle(2, H.oracle_params(2, salt=0.5, half_charged_ends=False), H.topo_tensors(top), None, dt, KT, KT / 2.5, KT / 7.5,
                         1.0, INERTIA, seed=SEED)
    out = []
    for _ in range(n_steps):
        x, qq, pp, LL, _u = orc.step(x, qq, pp, LL)
        out.append(tuple(np.array(a, dtype=np.float64) for a in (x, qq, pp, LL)))
    return out


def _check_against_oracle(kind, dtype, n_steps, recoveries, blob_tolerances=False):
    """n_steps with a saved row per step (the energy-trace instantiation), then the same steps without (the plain one):
    every saved row and both final states against the oracle."""
    finals = []
    for save_every in (1, 0):
        _, integ, c, q = _integrator(kind, dtype)
        p, L = integ.init_momenta()
        start = np.concatenate([t.cpu().numpy().astype(np.float64).ravel() for t in (c, q, p, L)]).tobytes()
        ref = _oracle_states(kind, n_steps, start)
        tc, tq, _ = integ.run(c, q, p, L, n_steps, save_every=save_every)
        assert integ.step == n_steps and integ.last_recoveries() == recoveries, (integ.step, integ.last_recoveries())
        got = [(tc[k], tq[k], None, None) for k in range(n_steps)] if save_every else []
        got.append((c, q, p, L))
        for k, row in zip(list(range(n_steps)) if save_every else [], got[:-1]):
            _compare(row, ref[k], dtype, k + 1, blob_tolerances, f"{kind} saved row {k}")
        _compare(got[-1], ref[-1], dtype, n_steps, blob_tolerances, f"{kind} final, save_every={save_every}")
        finals.append((c, q, p, L))
    for a, b in zip(*finals):  # the two instantiations evaluate the same terms in the same order
        assert torch.equal(a, b)


def _compare(got, ref, dtype, steps, blob_tolerances, what):
    for name, g, r, ulps in zip(("c", "q", "p", "L"), got, ref, FP32_ULPS_PER_STEP):
        if g is None:
            continue
        g = g.cpu().numpy().astype(np.float64)
        err, big = float(np.abs(g - r).max()), float(np.abs(r).max())
        if dtype == torch.float32:
            tol = (steps + 1) * ulps * 2.0**-24 * big  # (+ 1: the start state is rounded to fp32 and its quaternions re-normalised on entry)
            print(f"{what} fp32 {name}: max error {err:.3e}, bound {tol:.3e}")
            assert err <= tol, (what, name, err, tol)
        elif blob_tolerances:  # tests/test_gpu_edge_cases.py, the crowded systems
            print(f"{what} fp64 {name}: max error {err:.3e}")
            if name in ("c", "q"):
                np.testing.assert_allclose(g, r, rtol=1e-11, atol=1e-12)
            else:
                np.testing.assert_allclose(g, r, rtol=1e-8, atol=1e-9 * big)
        else:  # tests/test_gpu_langevin.py, step by step
            print(f"{what} fp64 {name}: max error {err:.3e}")
            np.testing.assert_allclose(g, r, rtol=0, atol=1e-10 if name in ("c", "q") else 1e-9)


@pytest.fixture
def eight_lanes():
    """ONE workgroup of 32 nucleotides (a system this small would take 16 lanes per nucleotide, two workgroups)"""
    _lib.debug_set("md_lanes", 8)
    yield 8
    _lib.debug_set("md_lanes", 0)


# ---- case 1: several sweeps per role ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_lists_of_several_sweeps_per_role(dtype, eight_lanes):
    """148 base-pair items: 74 per half, two sweeps each; 138 coaxial items: three sweeps.  No nucleotide has more than 14
    and no wavefront more than 47 of a kind, so in fp32 (fixed rows, wave-dense lists of 64) nothing aborts: no recovery.
    (The issue this file came with expected this launch to abort on a full wavefront list; counted, the fullest has 47
    items - test_a_full_wavefront_list... below is the system that does abort there.)  fp64 takes its rows from the
    workgroup's pool of 320, needs 350, and recovers once, as in the test the system comes from."""
    n0, n1 = _list_counts("crowded")
    assert n0.sum() == 148 and n1.sum() == 138 and (n0 + n1).max() <= 14 and (n0 > 0).all() and (n1 > 0).all()
    w0, w1 = n0.reshape(4, 8).sum(1), n1.reshape(4, 8).sum(1)
    assert max(w0.max(), w1.max()) <= WAVE_CAP and (2 + n0 + n1).sum() > 320
    _check_against_oracle("crowded", dtype, 3, recoveries=1 if dtype == torch.float64 else 0, blob_tolerances=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_full_wavefront_list_aborts_the_launch_and_the_step_reruns(dtype, eight_lanes):
    """The first wavefront's eight nucleotides flag 84 base-pair items - more than its list of 64 holds - while no nucleotide
    has more than 12: in fp32 the launch aborts, the run repeats the step with the 32-row instantiation (one recovery) and the
    trajectory is the oracle's.  fp64 (per-nucleotide lists, pooled rows: 2 x 32 + 218 rows of 320) runs straight through."""
    n0, n1 = _list_counts("lattice")
    w0 = n0.reshape(4, 8).sum(1)
    assert w0[0] == 84 and (w0[1:] <= WAVE_CAP).all() and n1.sum() == 0 and n0.max() == 12 <= ROW_ROOM and (2 + n0).sum() <= 320
    _check_against_oracle("lattice", dtype, 3, recoveries=1 if dtype == torch.float32 else 0, blob_tolerances=True)


# ---- case 2: empty lists among full ones -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_empty_lists_among_full_ones(dtype, md_lanes):
    """58 and 38 items: one sweep per role, an odd number of coaxial items, nucleotides without any item of a kind"""
    n0, n1 = _list_counts("sparse")
    assert n0.sum() == 58 and n1.sum() == 38 and (n0 == 0).sum() == 10 and (n1 == 0).sum() == 13
    _check_against_oracle("sparse", dtype, 3, recoveries=0, blob_tolerances=True)


# ---- case 3: no item at all ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_no_item_at_all(dtype, md_lanes):
    n0, n1 = _list_counts("apart")
    assert n0.sum() == 0 and n1.sum() == 0
    _check_against_oracle("apart", dtype, 3, recoveries=0)


# ---- case 4: a duplex with a partial last workgroup ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_duplex_with_a_partial_last_workgroup(dtype, md_lanes):
    _check_against_oracle("duplex", dtype, 20, recoveries=0)


# ---- case 5: determinism ---------------------------------------------------------------------------------------------

def _advance(kind, dtype, plan):
    _, integ, c, q = _integrator(kind, dtype)
    p, L = integ.init_momenta()
    integ.load(c, q, p, L)
    for n in plan:
        integ.advance(n)
    integ.store(c, q, p, L)
    torch.cuda.synchronize()
    return c, q, p, L


def _deterministic(kind, dtype):
    a, b = _advance(kind, dtype, (50,)), _advance(kind, dtype, (50,))
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    one, split = _advance(kind, dtype, (20,)), _advance(kind, dtype, (7, 13))
    for x, y in zip(one, split):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_lane_that_evaluates_an_item_does_not_leak_crowded(dtype, eight_lanes):
    _deterministic("crowded", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_lane_that_evaluates_an_item_does_not_leak_duplex(dtype, md_lanes):
    _deterministic("duplex", dtype)
