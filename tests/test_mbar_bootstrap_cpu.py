"""CPU tests of the block bootstrap of MBAR and of the statistical inefficiency (no GPU): the reference
tests/mbar_boot_ref.py against hand-computed values, against tests/mbar_newton_ref.py and against the scatter over
independent draws of correlated windows; the library's host side - ``block_resample``, ``auto_block``,
``subsample_correlated``, the refusals - against the reference."""

import importlib

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from tests import mbar_boot_ref as BR
from tests import mbar_newton_ref as NR
from tests import mbar_ref as R

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)


def test_the_symbols_are_there():
    lib = _lib.load()
    for name in ("mbar_boot_colsums", "mbar_boot_binned", "timeseries_check", "timeseries_moments", "timeseries_autocorr"):
        assert hasattr(lib, f"mythos_{name}") and f"mythos_{name}" in _lib.DECLARED_SYMBOLS
    import mythos_amd.observables as O

    for name in ("statistical_inefficiency", "block_resample", "subsample_correlated", "auto_block", "BlockResample"):
        assert name in O.__all__ and getattr(O, name) is getattr(M, name)


def test_reference_g_exact_values():
    """Hand-computed: x = (1, 2, 4, 3): mu = 2.5, v = 1.25, C(1) = (1.5 * 0.5 - 0.5 * 1.5 + 1.5 * 0.5) / (3 * 1.25) = 0.2,
    C(2) = (-1.5 * 1.5 - 0.5 * 0.5) / (2 * 1.25) = -1 - both below mintime = 3, so both enter: g = 1 + 2 (0.2 * 3/4 - 1 * 2/4) =
    0.3 -> 1; with mintime = 1, t* = 2: g = 1 + 2 * 0.2 * 3/4 = 1.3.  x = (0, 1, 2, 3, 4): mu = 2, v = 2, C(1) = (2 + 0 + 0 + 2)
    / (4 * 2) = 0.5, C(2) = (0 - 1 + 0) / (3 * 2) = -1/6, C(3) = (-2 - 2) / (2 * 2) = -1: mintime = 0 stops at t* = 2, g = 1 + 2 * 0.5 * 4/5
    = 1.8; mintime = 3 takes all three, g = 1.8 - 2/6 * 3/5 - 2 * 2/5 = 0.8 -> 1."""
    x4, x5 = [1.0, 2.0, 4.0, 3.0], [0.0, 1.0, 2.0, 3.0, 4.0]
    assert abs(BR.autocorr(x4, 1) - 0.2) < 1e-15 and abs(BR.autocorr(x4, 2) + 1.0) < 1e-15
    assert abs(BR.autocorr(x5, 1) - 0.5) < 1e-15 and abs(BR.autocorr(x5, 2) + 1.0 / 6.0) < 1e-15 and abs(BR.autocorr(x5, 3) + 1.0) < 1e-15
    for fn in (BR.stat_ineff_loops, BR.stat_ineff):
        assert fn(x4) == 1.0 and abs(fn(x4, mintime=1) - 1.3) < 1e-14
        assert abs(fn(x5, mintime=0) - 1.8) < 1e-14 and fn(x5) == 1.0
        assert fn([3.0] * 7) == 1.0                                    # a constant series
        assert fn([5.0]) == 1.0 and fn([1.0, 2.0]) == 1.0              # T = 1, 2
        # T = 3 has the one lag t = 1, and d_1 d_2 + d_2 d_3 = -d_2^2 <= 0 because the deviations sum to zero: always 1
        assert fn([0.0, 1.0, 5.0]) == 1.0 and fn([1.0, 2.0, 3.0]) == 1.0
    assert abs(BR.autocorr([0.0, 1.0, 5.0], 1) - (2.0 - 3.0) / (2.0 * 14.0 / 3.0)) < 1e-15
    x = np.random.default_rng(0).normal(size=40).cumsum()
    assert abs(BR.stat_ineff_loops(x) - BR.stat_ineff(x)) < 1e-12 and BR.stat_ineff(x) > 2.0


def test_reference_g_of_ar1_series_is_the_analytic_value():
    """48 seeds of 4 000 AR(1) frames at phi = 0.5 (g = 3) and phi = 0.8 (g = 9): the mean estimate within 4 standard errors."""
    for phi in (0.5, 0.8):
        z = BR.ar1(np.random.default_rng(7), phi, (48, 4000))
        g = np.array([BR.stat_ineff(row) for row in z])
        want, se = (1.0 + phi) / (1.0 - phi), g.std(ddof=1) / np.sqrt(len(g))
        print(f"  phi = {phi}: g = {g.mean():.3f} +- {se:.3f}, analytic {want:.3f}")
        assert abs(g.mean() - want) <= 4.0 * se and se < 0.05 * want


RESAMPLE_CASES = {
    "l1": dict(n_k=(5, 3), block=1),
    "l_is_N": dict(n_k=(6, 6), block=6),
    "short_last": dict(n_k=(10, 7), block=(3, 4)),   # last blocks of 1 and 3
    "unequal": dict(n_k=(1, 13, 40), block=(5, 13, 7)),
    "longer_than_N": dict(n_k=(4, 9), block=100),
}


@pytest.mark.parametrize("name", list(RESAMPLE_CASES))
def test_block_resample(name):
    c = RESAMPLE_CASES[name]
    n_k, n_boot = np.asarray(c["n_k"]), 6
    r = M.block_resample(n_k, c["block"], n_boot, seed=11)
    block = np.minimum(np.broadcast_to(np.asarray(c["block"]), n_k.shape), n_k)
    assert (r.block == block).all() and r.n_boot == n_boot
    off = np.concatenate([[0], np.cumsum(n_k)])
    for k, (s, length) in enumerate(zip(r.starts, r.lengths)):
        count = -(-n_k[k] // block[k])
        assert s.shape == (n_boot, count) and s.dtype == np.int64 and len(length) == count
        assert (length[:-1] == block[k]).all() and length[-1] == n_k[k] - (count - 1) * block[k] and length.sum() == n_k[k]
        assert (s >= 0).all() and (s + length[None, :] <= n_k[k]).all()
    m = r.multiplicities(0, n_boot, "cpu")
    assert m.dtype == torch.uint16 and tuple(m.shape) == (n_boot, int(n_k.sum()))
    got = m.to(torch.int64).numpy()
    assert (got == BR.multiplicities(n_k, r.starts, r.lengths)).all()
    for k in range(len(n_k)):
        assert (got[:, off[k]:off[k + 1]].sum(axis=1) == n_k[k]).all()
    if name == "l_is_N":
        assert (got == 1).all()
    # the seed decides, batches are slices
    again = M.block_resample(n_k, c["block"], n_boot, seed=11)
    other = M.block_resample(n_k, c["block"], n_boot, seed=12)
    assert all((a == b).all() for a, b in zip(r.starts, again.starts))
    assert (block == n_k).all() or any((a != b).any() for a, b in zip(r.starts, other.starts))
    assert torch.equal(r.multiplicities(2, 5, "cpu"), m[2:5])
    per = 2 * int(n_k.sum())
    assert r.batch_size(3 * per) == 3 and r.batch_size(1) == 1 and r.batch_size(1 << 30) == n_boot
    parts = list(r.batches("cpu", max_bytes=4 * per))
    assert [p.shape[0] for p in parts] == [4, 2] and torch.equal(torch.cat(parts), m)
    # the documented order of the draws
    rng = np.random.default_rng(11)
    for k in range(len(n_k)):
        assert (rng.integers(0, n_k[k] - r.lengths[k] + 1, size=r.starts[k].shape) == r.starts[k]).all()


def test_auto_block_and_subsample():
    assert M.BOOT_BLOCK_FACTOR == 3
    assert (M.auto_block(np.array([[1.0, 2.1], [9.0, 3.0], [50.0, 1.0]]), [100, 20, 1000]) == [7, 20, 150]).all()
    with pytest.raises(ValueError, match="below 1"):
        M.auto_block([0.5], [10])
    keep, kept = M.subsample_indices([10, 5, 3], [2.5, 1.0, 7.0])
    assert list(keep) == [0, 3, 5, 8] + [10, 11, 12, 13, 14] + [15] and list(kept) == [4, 5, 1]
    keep, kept = M.subsample_indices([7], [0.4])  # duplicates dropped: every frame once
    assert list(keep) == list(range(7)) and list(kept) == [7]
    xi = torch.arange(18, dtype=torch.float64)[:, None].contiguous()
    x2, n2 = M.subsample_correlated(xi, g=np.array([2.5, 1.0, 7.0]), n_k=[10, 5, 3])
    assert x2[:, 0].tolist() == [0, 3, 5, 8, 10, 11, 12, 13, 14, 15] and list(n2) == [4, 5, 1]
    x3, n3 = M.subsample_correlated(torch.arange(12, dtype=torch.float64).reshape(4, 3, 1), g=[2.0, 1.0, 3.0])  # (rows, R, P)
    assert x3[:, 0].tolist() == [0, 6, 1, 4, 7, 10, 2, 11] and list(n3) == [2, 4, 2]


def test_refusals():
    with pytest.raises(ValueError, match="non-finite value \\(row 2, column 1\\)"):
        M.check_series([3, 2], x=np.array([[1.0, 0], [2, 0], [0, np.inf], [1, 0], [1, 0]]))
    with pytest.raises(ValueError, match="offsets do not increase to N"):
        M.check_series([3, 2], n_rows=6)
    with pytest.raises(ValueError, match="offsets do not increase to N \\(series 1 is empty"):
        M.check_series([3, 0, 2], n_rows=5)
    with pytest.raises(ValueError, match="E < 1"):
        M.check_series([3, 2], x=np.zeros((5, 0)))
    M.check_series([3, 2], x=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="a block shorter than 1 \\(window 1\\)"):
        M.block_resample([5, 5], [2, 0], 3)
    with pytest.raises(ValueError, match="window 0 has more than 65535 blocks \\(65536\\)"):
        M.block_resample([65_536, 5], 1, 1)
    assert M.block_resample([65_535], 1, 1).starts[0].shape == (1, 65_535)
    with pytest.raises(ValueError, match="n_boot < 1"):
        M.block_resample([5], 1, 0)
    with pytest.raises(ValueError, match="block must be an int"):
        M.block_resample([5, 5], [1.5, 2.0], 2)
    with pytest.raises(ValueError, match="block must be an int"):
        M.block_resample([5, 5], [1, 2, 3], 2)
    u = torch.zeros(2, 4, dtype=torch.float64)
    for solver in ("fixed-point", "bfgs"):
        with pytest.raises(ValueError, match="bootstrap > 0 requires solver='newton'"):
            M.mbar(u, [2, 2], bootstrap=5, solver=solver)
    with pytest.raises(ValueError, match="bootstrap >= 0"):
        M.mbar(u, [2, 2], bootstrap=-1, solver="newton")
    res = M.MbarResult(f=torch.zeros(2), log_weights=torch.zeros(4), iterations=1, delta=0.0)
    with pytest.raises(ValueError, match="without bootstrap"):
        res.f_error("bootstrap")
    with pytest.raises(ValueError, match="method 'jackknife'"):
        res.f_error("jackknife")
    with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
        M.statistical_inefficiency(torch.zeros(5, 1, dtype=torch.float64), n_k=[5])


def test_weighted_reference_against_the_unweighted_one():
    """m = 1 reproduces the Newton reference; m = 2 with N_k doubled gives the same f (the equations are homogeneous)."""
    c = R.gaussian_case(K=5, n_per=40, seed=1)
    u = R.bias(c["table"], c["xi"], c["kT"])
    f, _, _ = NR.newton(u, c["n_k"], tol=1e-12)
    ones = np.ones((1, u.shape[1]))
    got = BR.weighted_newton(u, c["n_k"], ones, tol=1e-12)[0]
    assert got[0] == 0.0 and np.abs(got - f).max() <= 1e-10
    doubled = BR.weighted_newton(u, 2 * c["n_k"], 2.0 * ones, tol=1e-12)[0]
    assert np.abs(doubled - f).max() <= 1e-10
    assert BR.weighted_residual(u, c["n_k"], f, ones[0]) <= 1e-11
    assert np.abs(BR.colsums(u, c["n_k"], f, np.zeros((1, 5)), ones) - 1.0).max() <= 1e-11
    # a resampled replicate solves its own equations, and they differ from the central ones
    r = M.block_resample(c["n_k"], 4, 3, seed=5)
    m = r.multiplicities(0, 3, "cpu").numpy()
    fb = BR.weighted_newton(u, c["n_k"], m, f0=f)
    assert max(BR.weighted_residual(u, c["n_k"], fb[b], m[b]) for b in range(3)) <= 1e-11
    assert np.abs(BR.colsums(u, c["n_k"], f, fb - f, m) - 1.0).max() <= 1e-10 and np.abs(fb - f).max() > 1e-3


STAT = dict(K=8, n_per=800, phi=0.8, draws=110, replicates=32)


def test_the_block_bootstrap_error_bar_is_the_scatter_over_draws_of_correlated_windows():
    """110 draws of K = 8 exact-Gaussian windows 1.5 sigma apart, 800 AR(1) frames each at phi = 0.8 (g = 9).  The mean
    bootstrap sigma(f_7 - f_0) at block="auto" (l = ceil(3 g) from each draw's own estimated g, 32 replicates per draw) over the
    standard deviation of f_7 - f_0 across the draws must lie in [0.80, 1.15]; the asymptotic sigma over the same scatter
    must lie below 0.5, which is what shows that the test tells the two apart.  The standard error of a standard deviation
    over 110 draws is 1 / sqrt(2 * 109) = 6.8 %.  Measured: 0.949 and 0.354 (0.948 and 0.353 at 1 200 frames).  On the reference alone."""
    s = STAT
    boot, asym, diff = [], [], []
    for d in range(s["draws"]):
        c = BR.correlated_gaussian_case(s["K"], s["n_per"], s["phi"], seed=d)
        u = R.bias(c["table"], c["xi"], c["kT"])
        f, _, _ = NR.newton(u, c["n_k"], f0=c["f"])
        block = M.auto_block(BR.stat_ineff_set(c["xi"], c["n_k"]), c["n_k"])
        r = M.block_resample(c["n_k"], block, s["replicates"], seed=d)
        fb = BR.weighted_newton(u, c["n_k"], r.multiplicities(0, s["replicates"], "cpu").numpy(), tol=1e-9, f0=f)
        boot.append(BR.boot_f_sigma(fb)[-1, 0])
        asym.append(NR.sigma(M._theta(NR.gram(u, c["n_k"], f)[0], c["n_k"]))[-1, 0])
        diff.append(f[-1] - f[0])
    scatter = np.std(diff, ddof=1)
    r_boot, r_asym = np.mean(boot) / scatter, np.mean(asym) / scatter
    print(f"  bootstrap / observed {r_boot:.3f}, asymptotic / observed {r_asym:.3f}, scatter {scatter:.4f}")
    assert 1.0 / np.sqrt(2.0 * (s["draws"] - 1)) <= 0.07
    assert 0.80 <= r_boot <= 1.15
    assert r_asym < 0.5
