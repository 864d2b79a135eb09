"""CPU tests of the MBAR estimator's reference, lowering and host checks (no GPU): tests/mbar_ref.py against the analytic
Gaussian case, the identities of the responsibilities, the window table of a MartiniRestraints set against the energies
of tests/martini_restraints_ref.py, every refusal of mythos_mbar_check, and the bins of the end-to-end GPU test."""

import importlib

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.simulators.martini_restraints import MartiniRestraints, PullCoordinate, PullGroup
from tests import martini_restraints_ref as MR
from tests import mbar_ref as R

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)

SEEDS = range(16)


def test_the_symbols_are_there_and_the_names_are_exported():
    lib = _lib.load()
    for name in ("check", "create", "destroy", "set_windows", "set_matrix", "iterate", "log_weights", "binned_sum"):
        assert hasattr(lib, f"mythos_mbar_{name}") and f"mythos_mbar_{name}" in _lib.DECLARED_SYMBOLS
    import mythos_amd.observables as O

    assert O.mbar is M.mbar and O.mbar_umbrella is M.mbar_umbrella and O.UmbrellaPMF is M.UmbrellaPMF and O.MbarResult is M.MbarResult
    assert M._MbarPlan.__name__.startswith("_") and issubclass(M._MbarPlan, _lib.Handle)


def test_the_reference_recovers_the_analytic_free_energies_and_profile():
    """K = 8 windows 1.5 sigma apart, N_k = 400 exact Gaussian samples each, 16 seeds: the mean deviation of every f_k and of
    every PMF bin (mean over the occupied bins removed; bins occupied under all seeds) lies within 4 standard errors of zero.
    Single-seed deviations of f_k reach 0.2 - 0.4 in reduced units here: of order 1 / sqrt(N_k) per window step, statistical.
    The bin average of exp(-beta F) against F at the bin centre is a bias of at most 0.01 kT at these bins (half a sigma
    wide), a twentieth of 4 standard errors."""
    devs, errs, occs = [], [], []
    edges = None
    for seed in SEEDS:
        c = R.gaussian_case(K=8, n_per=400, spacing_sigma=1.5, seed=seed)
        u = R.bias(c["table"], c["xi"], c["kT"])
        f, _, _ = R.solve(u, c["n_k"])
        devs.append(f - c["f"])
        edges = np.linspace(-6.0 * c["sigma"], 6.0 * c["sigma"], 25)
        err, occ = R.gaussian_pmf_error(c, edges)
        errs.append(err), occs.append(occ)
    devs, errs, use = np.asarray(devs), np.asarray(errs), np.all(occs, axis=0)
    se = devs[:, 1:].std(axis=0, ddof=1) / np.sqrt(len(SEEDS))
    print("  f_k: mean deviation", np.round(devs[:, 1:].mean(0), 4), "standard error", np.round(se, 4), "largest single", np.abs(devs).max())
    assert (np.abs(devs[:, 1:].mean(axis=0)) <= 4.0 * se).all()
    assert use.sum() >= 20
    se_b = errs[:, use].std(axis=0, ddof=1) / np.sqrt(len(SEEDS))
    print("  F_b: mean deviation", np.round(errs[:, use].mean(0), 4), "standard error", np.round(se_b, 4))
    assert (np.abs(errs[:, use].mean(axis=0)) <= 4.0 * se_b).all()


def test_the_responsibilities_sum_to_one_per_frame_and_to_the_counts_at_the_fixed_point():
    c = R.gaussian_case(K=5, n_per=1, seed=3)
    n_k = np.array([37, 64, 1, 65, 130])
    rng = np.random.default_rng(4)
    xi = np.concatenate([c["k"] * c["c"][k] / (c["k0"] + c["k"]) + c["sigma"] * rng.standard_normal(n) for k, n in enumerate(n_k)])[:, None]
    u = R.bias(c["table"], xi, c["kT"])
    _, _, t = R.iterate(u, n_k, rng.uniform(-1.0, 1.0, 5))
    assert np.abs(t.sum(axis=0) - 1.0).max() < 1e-14 and t.min() > 0.0 and t.max() <= 1.0
    f, _, _ = R.solve(u, n_k, tol=1e-13)
    _, _, t = R.iterate(u, n_k, f)
    assert np.abs(t.sum(axis=1) - n_k).max() < 1e-10 * n_k.max()
    # the update written with the responsibilities is the textbook one
    g = rng.uniform(-1.0, 1.0, 5)
    new, L, t = R.iterate(u, n_k, g)
    alt = g - np.log(t.sum(axis=1) / n_k)
    assert np.abs((alt - alt[0]) - new).max() < 1e-13


def _two_coordinate_set(K):
    """An umbrella on a direction from an absolute origin (per-replica init and k) and a constant force on a distance between
    two beads (per-replica k): both coordinates bias every window."""
    rng = np.random.default_rng(11)
    return MartiniRestraints(pulls=[
        PullCoordinate(group_a=None, group_b=PullGroup(members=(0,)), kind="umbrella", geometry="direction", vec=(0.0, 0.0, 2.0),
                       origin=(1.0, 1.5, 2.0), k=rng.uniform(200.0, 900.0, K), init=np.linspace(-0.4, 0.6, K), periodic=False),
        PullCoordinate(group_a=PullGroup(members=(1,)), group_b=PullGroup(members=(2,)), kind="constant-force", geometry="distance",
                       k=rng.uniform(-50.0, 50.0, K), periodic=False)])


def test_the_lowered_window_table_gives_the_bias_of_the_restraint_reference():
    K, kT = 4, 2.3
    rs = _two_coordinate_set(K)
    table = M.window_table(rs, K)
    assert table.shape == (K, 2, 4) and (table[:, 0, 0] == 0).all() and (table[:, 1, 0] == 1).all() and (table[:, :, 3] == 0).all()
    rng = np.random.default_rng(12)
    frames = 3.0 * rng.uniform(size=(9, 3, 3))
    masses = np.array([72.0, 50.0, 60.0])
    xi, want = np.zeros((9, 2)), np.zeros((K, 9))
    for n, x in enumerate(frames):
        for k in range(K):
            for p, c in enumerate(rs.pulls):
                xi[n, p], u_p, _, _, _, _ = MR.pull(c, x, masses, None, 0.0, k)
                want[k, n] += u_p / kT
    got = R.bias(table, xi, kT)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    M.check(np.full(K, 9), table=np.tile(table, (1, 1, 1)), kT=kT, xi=np.tile(xi, (K, 1)))  # the library takes it


def _refused(match, **kw):
    with pytest.raises(ValueError, match=match):
        M.check(**kw)


def test_every_refusal_of_the_host_check_without_a_device():
    K, N = 3, 12
    table = np.zeros((K, 1, 4))
    table[:, 0, 1], table[:, 0, 2] = 500.0, [0.0, 0.1, 0.2]
    xi = np.linspace(0.0, 0.2, N)[:, None]
    good = dict(n_k=[4, 4, 4], table=table, kT=2.5, xi=xi, edges=[0.0, 0.1, 0.2])
    M.check(**good)
    M.check(n_k=[5, 1, 7])  # the matrix path: counts alone
    _refused("N_k < 1", **{**good, "n_k": [8, 0, 4]})
    _refused("sum N_k != N", **{**good, "n_k": [4, 4, 5]})
    _refused("sum N_k != N", n_k=[4, 4, 4], n_frames=13)
    lib = _lib.load()
    one = np.ones(1, dtype=np.int64)
    assert lib.mythos_mbar_check(0, 1, 0, None, None, one.ctypes.data_as(M._I64P), None, 0, None) == -1 and "K < 1" in _lib.last_error()
    for col, name in ((1, "non-finite k"), (2, "non-finite init")):
        for bad in (np.nan, np.inf):
            t = table.copy()
            t[1, 0, col] = bad
            _refused(name, **{**good, "table": t})
    x = xi.copy()
    x[7, 0] = np.nan
    _refused("non-finite xi", **{**good, "xi": x})
    t = table.copy()
    t[2, 0, 3] = 1e-3
    _refused("rate != 0", **{**good, "table": t})
    _refused("different kT", **{**good, "kT": [2.5, 2.5, 2.6]})
    _refused("non-increasing edges", **{**good, "edges": [0.0, 0.1, 0.1]})
    _refused("non-increasing edges", **{**good, "edges": [0.0, 0.2, 0.1]})
    _refused("non-finite edge", **{**good, "edges": [0.0, np.inf]})
    _refused("LDS", n_k=np.ones(1400, dtype=np.int64))
    # a set with a moving coordinate is refused through the lowering too
    moving = MartiniRestraints(pulls=[PullCoordinate(group_b=PullGroup(members=(0,)), k=500.0, init=[0.0, 0.1, 0.2], rate=0.01)])
    _refused("rate != 0", **{**good, "table": M.window_table(moving, K)})


def test_the_bins_of_the_end_to_end_test_are_occupied_in_every_reference_draw():
    """The end-to-end GPU test compares on the bins that all 32 exact-Gaussian draws occupy, and asks that these are at least
    80 % of the bins inside the range of the windows' means: the reference alone must meet that, here, without a GPU."""
    ref = R.e2e_reference()
    inside, use = ref["inside"], ref["use"]
    print(f"  bins {len(use)}, inside the windows' range {inside.sum()}, of those occupied in all {R.E2E_SEEDS} draws {(use & inside).sum()}; "
          f"sigma {ref['sigma'][use].min():.3f} ... {ref['sigma'][use].max():.3f} kJ/mol")
    assert inside.sum() >= 20 and (use & inside).sum() >= 0.8 * inside.sum()
    assert np.isfinite(ref["sigma"][use]).all() and (ref["sigma"][use] > 0).all()
