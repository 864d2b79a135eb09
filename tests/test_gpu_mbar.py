"""GPU tests of MBAR and the umbrella PMF (mythos_amd/csrc/mbar.hip, mythos_amd/observables/mbar.py) against the NumPy
reference tests/mbar_ref.py (checked against the analytic Gaussian case by tests/test_mbar_cpu.py).

  1  one iteration from a given f, table path and matrix path: f' and L_n
  2  the solve: residual under the reference's map, iteration count, bitwise repeatability, max_iter
  3  PMF, expect, n_eff against the reference; empty bins, frames outside the edges, gradcheck, uniform weights
  4  alignment of the pooled frames with SimulatorTrajectory.concat(out.observables)
  5  end to end: umbrella windows on free beads in a harmonic well, the PMF against 1/2 k0 xi^2
  6  _MbarPlan.close() is idempotent
"""

import functools
import importlib

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.simulators.martini_restraints import MartiniRestraints, PositionRestraint, PullCoordinate, PullGroup
from tests import mbar_ref as R

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNK, MAX_BLOCKS = 1024, 1024  # kMbarChunk, kMbarMaxBlocks of csrc/mbar.hip
TOL_ITER = 1e-11


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _windows_case(n_k, P=1, spacing=1.5, seed=0, far=False, k0=2.0, k=8.0):
    """Frames of len(n_k) Gaussian windows (reduced units, kT = 1): dict(table (K, P, 4), xi (N, P), n_k, kT).  P = 2 adds a
    constant-force coordinate with its own per-window k.  ``far``: the last frame sits 40 sigma beyond the last window."""
    n_k = np.asarray(n_k, dtype=np.int64)
    K = len(n_k)
    c = R.gaussian_case(K=K, n_per=1, k0=k0, k=k, spacing_sigma=spacing, seed=seed)
    rng = np.random.default_rng(seed + 100)
    mean = c["k"] * c["c"] / (c["k0"] + c["k"])
    xi = np.concatenate([mean[w] + c["sigma"] * rng.standard_normal(n) for w, n in enumerate(n_k)])[:, None]
    if far:
        xi[-1, 0] = c["c"][-1] + 40.0 * c["sigma"]
    table = c["table"]
    if P == 2:
        second = np.zeros((K, 1, 4))
        second[:, 0, 0], second[:, 0, 1] = 1.0, rng.uniform(-3.0, 3.0, K)
        table = np.concatenate([table, second], axis=1)
        xi = np.concatenate([xi, rng.uniform(0.2, 2.0, size=xi.shape)], axis=1)
    return dict(table=np.ascontiguousarray(table), xi=np.ascontiguousarray(xi), n_k=n_k, kT=1.0)


ITER_CASES = {
    "K1": dict(n_k=(5,)),
    "K2": dict(n_k=(5, 1)),
    "K3": dict(n_k=(5, 1, 7)),
    "K5": dict(n_k=(37, 64, 1, 65, 130)),
    "K5_far": dict(n_k=(37, 64, 1, 65, 130), far=True, spacing=1.0, k0=0.5, k=9.5),
    "K65": dict(n_k=tuple(1 + (7 * i) % 5 for i in range(65)), spacing=0.3),
    "P2": dict(n_k=(37, 64, 1, 65, 130), P=2),
    "chunk_plus_1": dict(n_k=(CHUNK, 1)),
    "stride_plus_1": dict(n_k=(CHUNK * MAX_BLOCKS - 7, 8)),
}


@pytest.mark.parametrize("src", ["table", "matrix"])
@pytest.mark.parametrize("name", list(ITER_CASES))
def test_one_iteration_against_the_reference(name, src):
    """f' and L_n of one iteration from a random f, to 1e-11 absolute in reduced units on inputs with |b| <= 10^3.
    Where the figure comes from: b is formed with at most four roundings (the difference, the square, the product with
    beta k / 2, the sum over coordinates), each at most 2^-53 |b|: 4 * 2^-53 * 10^3 = 4.4e-13 in the exponent, which is an
    absolute error of L_n and of ln sum_n t_kn.  The sums add their depth times 2^-53 relative - which is absolute in the
    logarithm -: four frames of a thread, seven wavefront steps, a chunk per pass of the stride, four wavefronts, then at most 16
    workgroup partials per lane and seven more wavefront steps, about 40 * 2^-53 = 4e-15 (the reference sums pairwise);
    N * 2^-53 bounds any order and is below 1e-11 for N < 9 * 10^4.  exp and log add a few ulp of numbers of order one.  Together under 1e-12: 1e-11 holds a margin
    of ten, and it is the issue's figure."""
    c = _windows_case(**ITER_CASES[name])
    K, N = len(c["n_k"]), int(c["n_k"].sum())
    u = R.bias(c["table"], c["xi"], c["kT"])
    assert np.abs(u).max() <= 1e3
    if name == "K5_far":
        assert u[:, -1].min() > 745.2  # exp(-b) underflows for every window: only the running maximum keeps L finite
    f0 = np.random.default_rng(5).uniform(-2.0, 2.0, K)
    f0 -= f0[0]
    want_f, want_L, _ = R.iterate(u, c["n_k"], f0)
    plan = M._MbarPlan(N, K, DEV)
    try:
        xi_d, u_d = _dev(c["xi"]), _dev(u)
        if src == "table":
            plan.set_windows(c["table"], np.full(K, c["kT"]), c["n_k"], xi_d)
        else:
            plan.set_matrix(u_d, c["n_k"])
        f = _dev(f0)
        L = -plan.log_weights(f)
        assert torch.equal(f, _dev(f0))
        delta = torch.empty(1, dtype=torch.float64, device=DEV)
        plan.iterate(f, 1, delta)
        got_f, got_L, got_d = f.cpu().numpy(), L.cpu().numpy(), float(delta.item())
    finally:
        plan.close()
    err_f, err_L = np.abs(got_f - want_f).max(), np.abs(got_L - want_L).max()
    print(f"  {name} {src}: K = {K}, N = {N}: |f' - ref| {err_f:.2e}, |L - ref| {err_L:.2e}")
    assert np.isfinite(got_L).all() and got_f[0] == 0.0
    assert err_f <= TOL_ITER and err_L <= TOL_ITER
    assert abs(got_d - np.abs(want_f - f0).max()) <= 2 * TOL_ITER


# ------------------------------------------------------------------------------------------------ 2
def _gaussian_set(c, K):
    return MartiniRestraints(pulls=[PullCoordinate(group_a=None, group_b=PullGroup(members=(0,)), geometry="direction", vec=(0, 0, 1),
                                                   k=c["k"], init=c["c"], periodic=False)])


@functools.lru_cache(maxsize=None)
def _solved():
    c = R.gaussian_case(K=8, n_per=100, seed=21)
    rs = _gaussian_set(c, 8)
    xi = _dev(c["xi"])
    res = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], tol=1e-10, check_every=32)
    return c, rs, xi, res, R.bias(c["table"], c["xi"], c["kT"])


def test_the_solve_leaves_a_residual_below_tol_under_the_reference_map():
    c, rs, xi, res, u = _solved()
    f = res.f.cpu().numpy()
    moved = np.abs(R.iterate(u, c["n_k"], f)[0] - f).max()
    print(f"  {res.iterations} iterations, delta {res.delta:.2e}; the reference's map moves the GPU's f by {moved:.2e}")
    assert moved <= 1e-10 + 1e-11 and res.delta <= 1e-10 and f[0] == 0.0
    assert res.iterations % 32 == 0 or res.iterations < 32
    assert res.f.is_cuda and res.log_weights.is_cuda and res.log_weights.shape == (800,)
    assert np.abs(res.log_weights.cpu().numpy() - R.log_weights(u, c["n_k"], f)).max() <= TOL_ITER
    # the window-major (rows, R, P) form is the same problem
    rows = _dev(c["xi"].reshape(8, 100, 1).transpose(1, 0, 2))
    again = M.mbar_umbrella(rows, rs, c["kT"])
    assert torch.equal(again.f, res.f) and torch.equal(again.log_weights, res.log_weights) and again.iterations == res.iterations


def test_two_solves_give_the_same_bits_on_both_paths():
    c, rs, xi, res, u = _solved()
    again = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"])
    assert torch.equal(again.f, res.f) and torch.equal(again.log_weights, res.log_weights) and again.iterations == res.iterations
    a, b = (M.mbar(_dev(u), c["n_k"]) for _ in range(2))
    assert torch.equal(a.f, b.f) and torch.equal(a.log_weights, b.log_weights)
    fa = a.f.cpu().numpy()
    assert np.abs(R.iterate(u, c["n_k"], fa)[0] - fa).max() <= 1e-10 + 1e-11
    assert a.iterations < 32 or a.iterations % 32 == 0


def test_too_few_iterations_raise_with_the_last_delta():
    c, rs, xi, _, _ = _solved()
    with pytest.raises(M.MbarNotConverged, match=r"max_iter = 40.*32 iterations.*delta") as e:
        M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], max_iter=40)
    assert e.value.iterations == 32 and e.value.delta > 1e-10
    with pytest.raises(M.MbarNotConverged) as e:
        M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], max_iter=5)
    assert e.value.iterations == 5
    with pytest.raises(ValueError, match="N_k < 1"):
        M.mbar_umbrella(xi, rs, c["kT"], n_k=[800, 0, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="non-finite u_kn"):
        M.mbar(torch.full((2, 4), float("nan"), dtype=torch.float64, device=DEV), [2, 2])


# ------------------------------------------------------------------------------------------------ 3
def test_pmf_expect_and_n_eff_against_the_reference():
    c, rs, xi, res, u = _solved()
    lw = R.log_weights(u, c["n_k"], res.f.cpu().numpy())
    x = c["xi"][:, 0]
    lo, hi = x.min(), x.max()
    # bins beyond the data on both sides (empty: +inf), and edges that leave the outer frames out
    edges = np.concatenate([[lo - 2.0, lo - 1.0], np.linspace(lo + 0.3, hi - 0.3, 13), [hi + 1.0, hi + 2.0]])
    pmf = M.UmbrellaPMF(restraints=rs, coordinate=0, kT=c["kT"], edges=edges)
    assert pmf.fit(xi, n_k=c["n_k"]).iterations == res.iterations
    w = np.random.default_rng(8).uniform(0.5, 1.5, len(x))
    w /= w.sum()
    for weights in (None, w):
        want = R.pmf(lw, x, edges, c["kT"], weights)
        got = pmf(None if weights is None else _dev(weights)).cpu().numpy()
        assert got.shape == (len(edges) - 1,) and np.isposinf(want[[0, -1]]).all() and ((x < edges[0]) | (x >= edges[-1])).sum() == 0
        assert ((x >= edges[1]) & (x < edges[2])).sum() > 0
        assert (np.isposinf(got) == np.isposinf(want)).all()
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max() <= 1e-10 * np.abs(want[fin]).max()
    uniform = pmf(_dev(np.full(len(x), 1.0 / len(x)))).cpu().numpy()
    fin = np.isfinite(uniform)
    assert np.abs(uniform[fin] - pmf().cpu().numpy()[fin]).max() <= 1e-12 * np.abs(uniform[fin]).max()
    assert np.allclose(pmf.centres, 0.5 * (edges[1:] + edges[:-1]))
    # edges that cover only the middle: the frames outside count in the normalisation alone
    inner = M.UmbrellaPMF(restraints=rs, kT=c["kT"], edges=np.linspace(-0.3, 0.3, 7))
    inner.fit(xi, n_k=c["n_k"])
    want = R.pmf(lw, x, np.linspace(-0.3, 0.3, 7), c["kT"])
    assert ((x < -0.3) | (x >= 0.3)).sum() > 100 and np.abs(inner().cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()
    inner.release(), pmf.release()
    values = np.random.default_rng(9).normal(size=(len(x), 2))
    for weights in (None, w):
        wd = None if weights is None else _dev(weights)
        got = res.expect(_dev(values), wd).cpu().numpy()
        want = R.expect(lw, values, weights)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        assert abs(float(res.n_eff(wd)) - R.n_eff(lw, weights)) <= 1e-10 * R.n_eff(lw, weights)
    with pytest.raises(ValueError, match="non-increasing edges"):
        M.UmbrellaPMF(restraints=rs, kT=1.0, edges=[0.0, 0.0, 1.0])


def test_the_pmf_and_expect_are_differentiable_in_the_weights():
    c = R.gaussian_case(K=3, n_per=12, seed=2)
    rs, xi = _gaussian_set(c, 3), _dev(c["xi"])
    x = c["xi"][:, 0]
    pmf = M.UmbrellaPMF(restraints=rs, kT=0.7 * c["kT"], edges=np.linspace(x.min() + 0.1, x.max() - 0.1, 5))  # frames outside, too
    res = pmf.fit(xi, n_k=c["n_k"])
    assert np.isfinite(pmf().cpu().numpy()).all()
    w = torch.tensor(np.random.default_rng(3).uniform(0.5, 1.5, len(x)) / len(x), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pmf(t), (w,), eps=1e-7, atol=1e-6, rtol=1e-5)
    values = _dev(np.random.default_rng(4).normal(size=(len(x), 2)))
    assert torch.autograd.gradcheck(lambda t: res.expect(values, t), (w,), eps=1e-7, atol=1e-7, rtol=1e-5)
    # an empty bin takes no gradient and leaves the others' alone
    wide = M.UmbrellaPMF(restraints=rs, kT=c["kT"], edges=[x.min() - 2.0, x.min() - 1.0, 0.0, x.max() + 1.0])
    wide.fit(xi, n_k=c["n_k"])
    F = wide(w)
    assert torch.isposinf(F[0]) and torch.isfinite(F[1:]).all()
    (g,) = torch.autograd.grad(F[1:].sum(), w)
    assert torch.isfinite(g).all() and g.abs().max() > 0
    pmf.release(), wide.release()


def test_the_distance_jacobian_adds_kT_d_minus_1_ln_xi():
    c = R.gaussian_case(K=3, n_per=40, seed=6)
    shift = 3.0  # a distance: every frame at xi > 0
    init = c["c"] + shift
    xi = _dev(c["xi"] + shift)
    edges = np.linspace(shift - 1.0, shift + 1.0, 6)
    mk = lambda dim: MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=(1,)), group_b=PullGroup(members=(0,)),  # noqa: E731
                                                             geometry="distance", dim=dim, k=c["k"], init=init, periodic=False)])
    plain = M.UmbrellaPMF(restraints=mk((True, True, True)), kT=c["kT"], edges=edges)
    plain.fit(xi, n_k=c["n_k"])
    for dim, d in (((True, True, True), 3), ((True, True, False), 2), ((False, False, True), 1)):
        jac = M.UmbrellaPMF(restraints=mk(dim), kT=c["kT"], edges=edges, jacobian="distance")
        jac.fit(xi, n_k=c["n_k"])
        assert np.abs((jac() - plain()).cpu().numpy() - c["kT"] * (d - 1) * np.log(jac.centres)).max() <= 1e-12
        jac.release()
    plain.release()
    with pytest.raises(ValueError, match="geometry 'distance'"):
        M.UmbrellaPMF(restraints=_gaussian_set(c, 3), kT=1.0, edges=edges, jacobian="distance")


# ------------------------------------------------------------------------------------------------ 4
@functools.lru_cache(maxsize=None)
def _bilayer():
    from mythos_amd.energy import martini as ME
    from tests import martini_helpers as MH

    s = MH.system()
    x, box, _ = MH.frames("lj")
    top = s["top"]
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    fn = ME.MartiniComposedEnergyFunction([ME.LJ.from_topology(topology=top, params=ME.LJConfiguration(**s["lj_params"])),
                                           ME.Bond.from_topology(topology=top, params=ME.BondConfiguration(**s["bond_params"])),
                                           ME.Angle.from_topology(topology=top, params=ME.AngleConfiguration(**ap))])
    return dict(fn=fn, top=top, x=x[3], box=box[3])


def test_the_pooled_frames_line_up_with_the_concatenated_trajectories():
    """Three windows on the height of one bead above an absolute origin (0.15 nm apart, 0.022 nm wide): xi of pooled frame n, as
    ``pooled`` orders ``state["pull"]``, is the coordinate measured on frame n of SimulatorTrajectory.concat(out.observables)."""
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator
    from mythos_amd.simulators.io import SimulatorTrajectory

    b = _bilayer()
    bead, origin = 5, tuple(float(v) for v in b["x"][5])
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=None, origin=origin, group_b=PullGroup(members=(bead,)), geometry="direction",
                                                 vec=(0, 0, 1), k=5000.0, init=np.array([-0.15, 0.0, 0.15]), periodic=False)])
    sim = HipMartiniSimulator(energy_fn=b["fn"], topology=b["top"], init_positions=b["x"], box=b["box"], temperatures=[300.0] * 3, dt=0.02,
                              gamma=1.0, equilibration_steps=200, simulation_steps=40, save_every=10, neighbors=(0.4, 5), restraints=rs,
                              precision="float32", name="windows")
    out = sim.run({}, seed=3)
    xi = out.state["pull"]
    rows = 4
    assert xi.shape == (rows, 3, 1)
    flat, n_k = M.pooled(xi)
    traj = SimulatorTrajectory.concat(out.observables)
    assert flat.shape == (3 * rows, 1) and list(n_k) == [rows] * 3 and traj.center.shape[0] == 3 * rows
    measured = traj.center[:, bead, 2].double().cpu().numpy() - origin[2]
    got = flat[:, 0].cpu().numpy()
    for n in range(3 * rows):
        assert got[n] == float(xi[n % rows, n // rows, 0])
        assert abs(got[n] - measured[n]) < 1e-5, n
    # the windows are apart by far more than they are wide: the row-major order would not pass
    assert np.abs(xi.reshape(-1).cpu().numpy() - measured).max() > 0.1
    sim.release()


# ------------------------------------------------------------------------------------------------ 5
def test_umbrella_windows_on_a_harmonic_well_recover_its_profile():
    """A free bead of 72 amu under a position restraint k0 = 100 kJ/mol/nm^2 on z and an umbrella k = 500 on its height xi
    above the restraint's reference: the base potential along xi is exactly 1/2 k0 xi^2 and every window an exact Gaussian
    of variance kT / (k0 + k), kT = 2.5 (sigma = 0.0645 nm).  64 replicas = 8 windows 1.5 sigma apart x 8 copies, gamma = 3 / ps,
    dt = 0.02 ps: omega^2 = 600 / 72 = 8.3 / ps^2, autocorrelation time gamma / omega^2 + 1 / gamma = 0.7 ps = 35 steps; frames
    are saved every 100 steps, where the measured lag-1 autocorrelation of xi is -0.04 (asserted below 0.1), 50 per replica
    after 1 000 steps of equilibration.
    The recovered F_b minus 1/2 k0 xi_b^2, mean over the compared bins removed, stays within 4 standard deviations of the
    same quantity over 32 draws of exact Gaussian samples with these counts pushed through tests/mbar_ref.py
    (mbar_ref.e2e_reference: 0.20 ... 0.41 kJ/mol per bin, 0.2 in the middle, 0.3 - 0.4 at the ends), on the bins occupied in
    all 32 draws: all 24 bins of half a sigma on [-6 sigma, 6 sigma], 22 of them inside the windows' range
    (tests/test_mbar_cpu.py checks that count without a GPU).  Measured on an MI355X: largest deviation 3.2 sigma_b, rms 1.08."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniSystem
    from tests import martini_restraints_cases as CS

    e, ref = R.E2E, R.e2e_reference()
    n, n_rep, rows, stride = 16, e["K"] * e["copies"], e["rows"], 100
    case = R.e2e_case(0)
    inits = np.repeat(case["c"], e["copies"])
    means = e["k"] * inits / (e["k0"] + e["k"])
    fb = CS.free_beads(n)
    x_ref = fb["pos"][0].copy()
    rs = MartiniRestraints(position=[PositionRestraint(index=0, k=(0.0, 0.0, e["k0"]), reference=tuple(x_ref))],
                           pulls=[PullCoordinate(group_a=None, origin=tuple(x_ref), group_b=PullGroup(members=(0,)), geometry="direction",
                                                 vec=(0, 0, 1), k=e["k"], init=inits, periodic=False)])
    sysm = MartiniSystem(*fb["ff"], angle_kind=0, dtype=torch.float32)
    integ = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=[e["kT"]] * n_rep, gamma=3.0, mass=np.full(n, 72.0), seeds=list(range(500, 500 + n_rep)))
    integ.set_neighbor_policy(1.0, 10)
    x0 = np.broadcast_to(fb["pos"], (n_rep, n, 3)).copy()
    x0[:, 0, 2] += means
    integ.set_restraints(rs)
    integ.load(torch.tensor(x0, dtype=sysm.dtype, device=sysm.device).contiguous(), integ.init_velocities(), fb["box"])
    integ.advance(1000)
    traj, _ = integ.advance(rows * stride, save_every=stride, want_energy=False)
    xi = integ.pull_values(traj)  # (rows, 64, 1)
    assert xi.shape == (rows, n_rep, 1)
    x = xi[:, :, 0].cpu().numpy()
    d = x - x.mean(axis=0)
    lag1 = float(((d[1:] * d[:-1]).sum(axis=0) / (d * d).sum(axis=0)).mean())
    pmf = M.UmbrellaPMF(restraints=rs, coordinate=0, kT=e["kT"], edges=ref["edges"])
    res = pmf.fit(xi)
    F = pmf().cpu().numpy()
    pmf.release(), integ.close(), sysm.close()
    use = ref["use"]
    assert np.isfinite(F[use]).all()
    err = F[use] - 0.5 * e["k0"] * ref["centres"][use] ** 2
    err -= err.mean()
    print(f"  lag-1 autocorrelation of xi {lag1:.3f}; {res.iterations} iterations; |F_b - k0 xi_b^2 / 2| / sigma_b: max {np.abs(err / ref['sigma'][use]).max():.2f}, "
          f"rms {np.sqrt(((err / ref['sigma'][use]) ** 2).mean()):.2f}; sigma_b {ref['sigma'][use].min():.3f} ... {ref['sigma'][use].max():.3f} kJ/mol")
    assert lag1 < 0.1
    assert (use & ref["inside"]).sum() >= 0.8 * ref["inside"].sum()
    assert (np.abs(err) <= 4.0 * ref["sigma"][use]).all()


# ------------------------------------------------------------------------------------------------ 6
def test_close_of_the_plan_is_idempotent():
    class Counting:
        def __init__(self, lib):
            self.lib, self.destroyed = lib, []

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if not name.endswith("_destroy"):
                return fn
            return lambda h: (self.destroyed.append(name), fn(h))[1]

    plan = M._MbarPlan(10, 2, DEV)
    assert isinstance(plan, _lib.Handle) and plan._h
    with pytest.raises(_lib.MythosHipError, match="neither windows nor a matrix"):
        plan.log_weights(torch.zeros(2, dtype=torch.float64, device=DEV))
    spy = plan._lib = Counting(plan._lib)
    plan.close()
    assert plan._h is None and spy.destroyed == ["mythos_mbar_destroy"]
    plan.close()
    plan.__del__()
    assert spy.destroyed == ["mythos_mbar_destroy"]
    with pytest.raises(_lib.MythosHipError, match="K < 1"):
        M._MbarPlan(10, 0, DEV)
