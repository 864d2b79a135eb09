"""CPU tests of the Newton solve and the asymptotic error bars of MBAR (no GPU): the reference tests/mbar_newton_ref.py
against tests/mbar_ref.py and against itself - the Gram route of the covariance against its N x N definition, Newton
against the fixed-point solve, the predicted error bar against the scatter over 200 draws - and the library's host function
``_theta`` against the same definition."""

import functools
import importlib

import numpy as np

from mythos_amd import _lib
from tests import mbar_newton_ref as NR
from tests import mbar_ref as R

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)

CASES = {
    "K5": dict(K=5, n_per=40, seed=1),
    "K8": dict(K=8, n_per=60, seed=2),
    "K4x3": dict(K=4, n_per=25, copies=3, seed=3),
    "K16_wide": dict(K=16, spacing_sigma=2.5),  # 2 761 fixed-point iterations
}
BINS = {"K5": 6, "K8": 12, "K4x3": 6}


@functools.lru_cache(maxsize=None)
def _case(name):
    c = R.gaussian_case(**CASES[name])
    u = R.bias(c["table"], c["xi"], c["kT"])
    f, it, d = NR.newton(u, c["n_k"])
    return c, u, f, it, d


def test_the_symbols_are_there():
    lib = _lib.load()
    for name in ("gram", "segment_moments"):
        assert hasattr(lib, f"mythos_mbar_{name}") and f"mythos_mbar_{name}" in _lib.DECLARED_SYMBOLS


def _augmented_case(name):
    c, u, f, _, _ = _case(name)
    x = c["xi"][:, 0]
    edges = np.linspace(x.min(), x.max() + 1e-9, BINS[name] + 1)
    W = NR.weights_matrix(u, c["n_k"], f)
    occ, cols = NR.bin_columns(R.log_weights(u, c["n_k"], f), x, edges)
    assert len(occ) == BINS[name]
    Wa = NR.augmented(W, cols)
    return Wa, np.concatenate([c["n_k"].astype(np.float64), np.zeros(len(occ))])


def test_the_gram_route_of_the_covariance_agrees_with_the_definition():
    """sigma of every difference of two columns - windows and bin columns - by ``theta_eig`` and by the library's ``_theta``
    against ``theta_direct``: 1e-10 for distinct windows (2e-15 measured), 1e-6 for tripled windows, whose Gram matrix is
    singular (1.5e-8 measured)."""
    for name, tol in (("K5", 1e-10), ("K8", 1e-10), ("K4x3", 1e-6)):
        Wa, n = _augmented_case(name)
        want = NR.sigma(NR.theta_direct(Wa, n))
        G = Wa.T @ Wa
        assert np.abs(G @ n - 1.0).max() < 1e-9  # the columns sum to one and the solve has converged: the null vector
        for route in (NR.theta_eig, M._theta):
            err = np.abs(NR.sigma(route(G, n)) - want).max()
            print(f"  {name} {route.__name__}: |sigma - direct| {err:.2e}, sigma up to {want.max():.3f}")
            assert err <= tol and want.max() > 0.05


def test_newton_matches_the_fixed_point_solve_within_its_iteration_cap():
    for name in CASES:
        c, u, f, it, d = _case(name)
        g, it_fp, _ = R.solve(u, c["n_k"], tol=1e-10)
        moved = np.abs(R.iterate(u, c["n_k"], f)[0] - f).max()
        print(f"  {name}: Newton {it} iterations (fixed point {it_fp}), |f - fixed point| {np.abs(f - g).max():.2e}, residual {moved:.2e}")
        assert np.abs(f - g).max() <= 1e-6 and f[0] == 0.0
        assert moved <= 1e-10 and d <= 1e-10
        assert it <= 25


def test_newton_stays_within_its_cap_at_64_windows():
    c = R.gaussian_case(K=64, n_per=100, seed=4)
    u = R.bias(c["table"], c["xi"], c["kT"])
    f, it, _ = NR.newton(u, c["n_k"])
    print(f"  K = 64: {it} iterations")
    assert it <= 25 and np.abs(R.iterate(u, c["n_k"], f)[0] - f).max() <= 1e-10


def test_the_predicted_error_bar_is_the_scatter_over_independent_draws():
    """200 seeds of K = 8 windows of 100 exact Gaussian frames: the mean predicted sigma(f_k - f_0) over the root mean square
    of f_k - f_0 about the analytic value, per window, within [0.85, 1.15] - the standard error of a standard deviation
    over 200 draws is 5 %, the band three of them."""
    pred, dev = [], []
    for seed in range(200):
        c = R.gaussian_case(K=8, n_per=100, seed=1000 + seed)
        u = R.bias(c["table"], c["xi"], c["kT"])
        f, _, _ = NR.newton(u, c["n_k"], f0=c["f"])
        G, _ = NR.gram(u, c["n_k"], f)
        pred.append(NR.sigma(M._theta(G, c["n_k"]))[1:, 0])
        dev.append(f[1:] - c["f"][1:])
    ratio = np.mean(pred, axis=0) / np.sqrt(np.mean(np.square(dev), axis=0))
    print("  predicted / observed per window:", np.round(ratio, 3))
    assert (ratio >= 0.85).all() and (ratio <= 1.15).all()
