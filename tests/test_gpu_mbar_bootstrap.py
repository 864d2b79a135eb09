"""GPU tests of the statistical inefficiency (mythos_amd/csrc/timeseries.hip) and of the block bootstrap of MBAR - the
batched weighted sums of mythos_amd/csrc/mbar.hip, the chord solve and the bootstrap error bars of
mythos_amd/observables/mbar.py - against the NumPy reference tests/mbar_boot_ref.py (checked without a GPU by
tests/test_mbar_bootstrap_cpu.py).

  1  autocorrelation functions and g: every length class, mixed lengths, E = 1 and 3, constant and alternating series, a
     lag block that ends at t*; repeatability
  2  mythos_mbar_boot_colsums and mythos_mbar_boot_binned at random delta, both sources; delta = 0 against the unweighted
     entry points; repeatability
  3  the batched solve through mbar_umbrella and mbar; m = 1; MbarNotConverged; bootstrap=0 changes nothing
  4  f_error("bootstrap"), uncertainty, interval and expect_error, with and without weights, with bins that are empty in
     some replicates and occupied in one

Tolerance 1e-11 (1 + |want|) on the sums, as tests/test_gpu_mbar_newton.py derives it for the window weights: the exponent's
error is the same, D_bn is a sum of K <= 65 positive terms (65 * 2^-53 relative) and a sum over frames adds its depth - 32
frames of a step in one fma chain, the steps of a workgroup, at most 1 024 partials - times 2^-53, below 4e-13 in all.
"""

import functools
import importlib

import numpy as np
import pytest
import torch

from tests import mbar_boot_ref as BR
from tests import mbar_newton_ref as NR
from tests import mbar_ref as R
from tests.test_gpu_mbar_newton import _gaussian_set, _Problem, _windows_case

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNK, BOOT_TILE = 1024, 32  # kMbarChunk, kBootTile of csrc/mbar.hip
TOL = 1e-11


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _u16(m):
    """Multiplicities as the (B, N) uint16 device tensor the library takes."""
    return torch.tensor(np.asarray(m).astype(np.uint16).view(np.int16), device=DEV).contiguous().view(torch.uint16)


def _close(got, want, tol=TOL):
    return (np.abs(got - want) <= tol * (1.0 + np.abs(want))).all()


# ------------------------------------------------------------------------------------------------ 1
SERIES_LENGTHS = (1, 2, 3, 255, 256, 257, 1025, 256, 256)  # the last two: a constant and a strictly alternating series


def _series(E, seed=3):
    rng = np.random.default_rng(seed)
    cols = []
    for T in SERIES_LENGTHS:
        phi = rng.uniform(0.3, 0.9, E)
        cols.append(np.stack([2.0 + 0.5 * BR.ar1(rng, p, (T,)) for p in phi], axis=1))
    cols[-2][:] = 1.75
    cols[-1][:] = (1.0 - 2.0 * (np.arange(256) % 2))[:, None] * np.arange(1, E + 1)[None, :]
    return np.ascontiguousarray(np.concatenate(cols)), np.asarray(SERIES_LENGTHS, dtype=np.int64)


@pytest.mark.parametrize("E", [1, 3])
def test_statistical_inefficiency_against_the_reference(E):
    x, n_k = _series(E)
    want = BR.stat_ineff_set(x, n_k)
    got_d = M.statistical_inefficiency(_dev(x), n_k)
    assert torch.equal(got_d, M.statistical_inefficiency(_dev(x), n_k))
    got = got_d.cpu().numpy()
    print(f"  E = {E}: g up to {want.max():.2f}, |got - want| / (1 + |want|) {(np.abs(got - want) / (1 + np.abs(want))).max():.2e}")
    assert got.shape == (len(n_k), E) and got_d.dtype == torch.float64 and got_d.is_cuda
    assert _close(got, want) and want.max() > 3.0
    assert (got[:3] == 1.0).all() and (got[-2:] == 1.0).all()  # T = 1, 2, 3, the constant and the alternating series
    # lag blocks of every size give the same g: one lag per call, blocks that end inside and past the longest series
    for lag_block in (1, 64, 65, 1024, 4096):
        assert _close(M.statistical_inefficiency(_dev(x), n_k, lag_block=lag_block).cpu().numpy(), want)
    for mintime in (0, 10):
        assert _close(M.statistical_inefficiency(_dev(x), n_k, mintime=mintime).cpu().numpy(), BR.stat_ineff_set(x, n_k, mintime))
    # each series alone is what it is in the mixed call
    off = np.concatenate([[0], np.cumsum(n_k)])
    for k in (3, 6):
        alone = M.statistical_inefficiency(_dev(x[off[k]:off[k + 1]]), [n_k[k]])
        assert _close(alone[0].cpu().numpy(), want[k])


def test_a_lag_block_that_ends_at_the_zero_crossing_and_the_pull_layout():
    rng = np.random.default_rng(12)
    x = BR.ar1(rng, 0.8, (1025,))
    g, t_star = BR.stat_ineff(x, return_tstar=True)
    assert 4 < t_star < 1023 and g > 3.0
    for lag_block in (t_star - 1, t_star, t_star + 1):  # the block's last lag is t* - 1, t*, t* + 1
        got = M.statistical_inefficiency(_dev(x[:, None]), [1025], lag_block=lag_block).cpu().numpy()
        assert got.shape == (1, 1) and _close(got[0, 0], g)
    # (rows, R, P) as out.state["pull"]: window r is the rows of column r
    pull = 1.0 + BR.ar1(rng, 0.7, (4, 2, 300)).transpose(2, 0, 1)
    want = np.array([[BR.stat_ineff(pull[:, r, p]) for p in range(2)] for r in range(4)])
    assert _close(M.statistical_inefficiency(_dev(pull)).cpu().numpy(), want)
    with pytest.raises(ValueError, match="non-finite value \\(row 7, column 0\\)"):
        bad = x[:, None].copy()
        bad[7, 0] = np.nan
        M.statistical_inefficiency(_dev(bad), [1025])
    with pytest.raises(ValueError, match="offsets do not increase to N"):
        M.statistical_inefficiency(_dev(x[:, None]), [1000, 24])


def test_autocorrelation_function_values():
    """C(t) itself, t = 0 ... 1 099 of series of 1 025, 257 and 3 rows in one call: C(0) = 1, zeros past the end."""
    rng = np.random.default_rng(4)
    n_k = np.array([1025, 257, 3], dtype=np.int64)
    x = np.ascontiguousarray(rng.normal(size=(int(n_k.sum()), 2)).cumsum(axis=0))
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(n_k)]), dtype=np.int64)
    xd, off_d = _dev(x), _dev(off, torch.int64)
    lib = M._lib.load()
    mean, var = (torch.empty(3, 2, dtype=torch.float64, device=DEV) for _ in range(2))
    head = (M._lib.ptr(xd), int(n_k.sum()), 2, 3, off.ctypes.data_as(M._I64P), M._lib.ptr(off_d))
    M._lib.check(lib.mythos_timeseries_moments(*head, M._lib.ptr(mean), M._lib.ptr(var), 0, M._lib.stream(DEV)))
    outs = []
    for _ in range(2):
        out = torch.full((3, 2, 1100), -7.0, dtype=torch.float64, device=DEV)
        M._lib.check(lib.mythos_timeseries_autocorr(*head, M._lib.ptr(mean), M._lib.ptr(var), 0, 1100, M._lib.ptr(out), 0, M._lib.stream(DEV)))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().numpy()
    for k in range(3):
        for e in range(2):
            s = x[off[k]:off[k + 1], e]
            d = s - s.mean()
            want = np.zeros(1100)
            for t in range(len(s)):
                want[t] = (d[:len(s) - t] @ d[t:]) / ((len(s) - t) * (d * d).mean())
            assert _close(got[k, e], want) and abs(got[k, e, 0] - 1.0) <= 1e-14
            assert abs(mean[k, e].item() - s.mean()) <= 1e-13 * abs(s.mean()) + 1e-15 and abs(var[k, e].item() - (d * d).mean()) <= 1e-12 * (d * d).mean()


# ------------------------------------------------------------------------------------------------ 2
def _mult(rng, B, N):
    """Multiplicities 0 ... 3 with, where the frames allow it: a first chunk of zeros in replicate 0, 300 (the high byte in
    use) and a step across the first chunk boundary."""
    m = rng.integers(0, 4, size=(B, N)).astype(np.int64)
    if N > CHUNK:
        m[0, :CHUNK] = 0
        m[B - 1, CHUNK - 3:CHUNK], m[B - 1, CHUNK:min(N, CHUNK + 3)] = 0, 300
    m[B // 2, N // 2] = 300
    return m


BOOT_CASES = {
    "K1": dict(case=dict(n_k=(5,)), B=1),
    "K2": dict(case=dict(n_k=(5, 1)), B=3),
    "K5": dict(case=dict(n_k=(37, 64, 1, 65, 858)), B=BOOT_TILE + 1),                      # N = 1 025: a chunk and a frame
    "K5_far": dict(case=dict(n_k=(37, 64, 1, 65, 858), far=True, spacing=1.0, k0=0.5, k=9.5), B=3),  # every exp(-b) underflows
    "P2": dict(case=dict(n_k=(37, 64, 1, 65, 858), P=2), B=3),
    "K65": dict(case=dict(n_k=tuple(1 + (7 * i) % 5 for i in range(64)) + (836,), spacing=0.3), B=3),  # a second window tile
    "big": dict(case=dict(n_k=(2**18, 2**18, 2**18, 2**18 - 3, 4)), B=3),                  # N = 2^20 + 1
}


@pytest.mark.parametrize("src", ["table", "matrix"])
@pytest.mark.parametrize("name", list(BOOT_CASES))
def test_boot_sums_against_the_reference(name, src):
    """s_bk = sum_n m_bn W_bnk and sum_n m_bn v_ne e^{-L_bn - shift} over all frames at random delta."""
    c = BOOT_CASES[name]
    B = c["B"]
    with _Problem(_windows_case(**c["case"]), src) as p:
        rng = np.random.default_rng(41)
        delta = rng.uniform(-0.5, 0.5, (B, p.K))
        m = _mult(rng, B, p.N)
        v = rng.uniform(0.5, 1.5, (p.N, 3))
        shift = float(R.log_weights(p.u, p.c["n_k"], p.f).max())
        f, delta_d, m_d = _dev(p.f), _dev(delta), _u16(m)
        got = p.plan.boot_colsums(f, delta_d, m_d)
        assert torch.equal(got, p.plan.boot_colsums(f, delta_d, m_d)) and torch.equal(f, _dev(p.f)) and torch.equal(delta_d, _dev(delta))
        want = BR.colsums(p.u, p.c["n_k"], p.f, delta, m)
        err = (np.abs(got.cpu().numpy() - want) / (1.0 + np.abs(want))).max()
        print(f"  {name} {src}: K = {p.K}, N = {p.N}, B = {B}: s {err:.2e} (of 1 + |want|), largest s {want.max():.3e}")
        assert got.shape == (B, p.K) and _close(got.cpu().numpy(), want)
        for vv in (None, v[:, :1], v):
            whole = p.plan.boot_binned(f, delta_d, m_d, v=None if vv is None else _dev(vv), shift=shift)
            assert torch.equal(whole, p.plan.boot_binned(f, delta_d, m_d, v=None if vv is None else _dev(vv), shift=shift))
            want = BR.binned(p.u, p.c["n_k"], p.f, delta, m, [np.arange(p.N)], vv, shift)
            assert whole.shape == want.shape and _close(whole.cpu().numpy(), want)
        # delta = 0 and m = 1 are the unweighted entry points
        ones, zero = _u16(np.ones((1, p.N))), torch.zeros(1, p.K, dtype=torch.float64, device=DEV)
        plain = p.plan.segment_moments(f).cpu().numpy()
        assert _close(p.plan.boot_colsums(f, zero, ones).cpu().numpy(), plain, 1e-13)
        order = torch.arange(p.N, device=DEV)
        seg = _dev([0, p.N // 2, p.N], torch.int64)
        lw = p.plan.log_weights(f)
        assert _close(p.plan.boot_binned(f, zero, ones, seg, order, None, shift).cpu().numpy()[0, :, 0],
                      p.plan.binned_sum(seg, order, lw, None, shift).cpu().numpy()[:2], 1e-13)


SEG_LENGTHS = (0, 1, 255, 256, 257, 1025)  # then 7 frames behind the last segment
SEG_CASES = {"K5": (400, 400, 400, 400, 201), "K65": (27,) * 64 + (73,)}


@pytest.mark.parametrize("src", ["table", "matrix"])
@pytest.mark.parametrize("name", list(SEG_CASES))
def test_boot_binned_segments_against_the_reference(name, src):
    """Segments of every length class of a random frame order, E = 0, 1 and 3, a replicate tile and one replicate more."""
    n_k = SEG_CASES[name]
    N, B = sum(n_k), BOOT_TILE + 1 if name == "K5" else 3
    assert N == sum(SEG_LENGTHS) + 7
    rng = np.random.default_rng(17)
    order = rng.permutation(N)
    seg = np.concatenate([[0], np.cumsum(SEG_LENGTHS)])
    segments = [order[seg[b]:seg[b + 1]] for b in range(len(SEG_LENGTHS))]
    v = rng.uniform(0.0, 1.0, (N, 3))
    with _Problem(_windows_case(n_k, spacing=1.5 if name == "K5" else 0.3), src) as p:
        delta, m = rng.uniform(-0.5, 0.5, (B, p.K)), _mult(rng, B, N)
        shift = float(R.log_weights(p.u, n_k, p.f).max())
        f, delta_d, m_d = _dev(p.f), _dev(delta), _u16(m)
        order_d, seg_d = _dev(order, torch.int64), _dev(seg, torch.int64)
        for vv in (None, v[:, :1], v):
            vd = None if vv is None else _dev(vv)
            got = p.plan.boot_binned(f, delta_d, m_d, seg_d, order_d, vd, shift)
            assert torch.equal(got, p.plan.boot_binned(f, delta_d, m_d, seg_d, order_d, vd, shift))
            want = BR.binned(p.u, n_k, p.f, delta, m, segments, vv, shift)
            got = got.cpu().numpy()
            assert got.shape == (B, len(SEG_LENGTHS), 1 if vv is None else vv.shape[1]) and (got[:, 0] == 0.0).all() and _close(got, want)
        # entries of the order that name no frame are skipped, never dereferenced
        bad = order.copy()
        at = [seg[3] + 5, seg[5] + 1000]
        bad[at[0]], bad[at[1]] = N + 5, -1
        keep = [np.array([n for i, n in enumerate(s, start=seg[b]) if i not in at], dtype=np.int64) for b, s in enumerate(segments)]
        got = p.plan.boot_binned(f, delta_d, m_d, seg_d, _dev(bad, torch.int64), _dev(v), shift).cpu().numpy()
        assert _close(got, BR.binned(p.u, n_k, p.f, delta, m, keep, v, shift))
        with pytest.raises(ValueError, match="come together"):
            p.plan.boot_binned(f, delta_d, m_d, seg_d, None)
        with pytest.raises(ValueError, match="0 <= E <= 8"):
            p.plan.boot_binned(f, delta_d, m_d, v=torch.ones(N, 9, dtype=torch.float64, device=DEV))
        with pytest.raises(ValueError, match="mult must be a contiguous uint16"):
            p.plan.boot_colsums(f, delta_d, m_d[:, :-1].contiguous())
    fresh = M._MbarPlan(10, 2, DEV)
    with pytest.raises(M._lib.MythosHipError, match="neither windows nor a matrix"):
        fresh.boot_colsums(torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(1, 2, dtype=torch.float64, device=DEV),
                           _u16(np.ones((1, 10))))
    fresh.close()


def test_boot_sums_refuse_windows_that_leave_no_lds():
    n_k = np.ones(130, dtype=np.int64)
    with _Problem(_windows_case(tuple(n_k), spacing=0.1), "matrix") as p:
        with pytest.raises(ValueError, match="do not fit 64 KB of LDS"):
            p.plan.boot_colsums(_dev(p.f), torch.zeros(1, 130, dtype=torch.float64, device=DEV),
                                _u16(np.ones((1, 130))))


# ------------------------------------------------------------------------------------------------ 3
@functools.lru_cache(maxsize=None)
def _correlated():
    c = BR.correlated_gaussian_case(K=6, n_per=150, phi=0.6, seed=3)
    return c, _gaussian_set(c), _dev(c["xi"]), R.bias(c["table"], c["xi"], c["kT"])


def test_the_batched_solve_through_the_public_interface():
    c, rs, xi, u = _correlated()
    n_k, B, tol = c["n_k"], 5, 1e-10
    res = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", tol=tol, bootstrap=B, boot_seed=7)
    g_want = BR.stat_ineff_set(c["xi"], n_k)[:, 0]
    assert res.boot_f.shape == (B, 6) and res.boot_f.is_cuda and _close(res.g, g_want) and (res.block == M.auto_block(g_want, n_k)).all()
    assert g_want.min() > 1.5 and res.block.max() < 150
    by_matrix = M.mbar(_dev(u), n_k, solver="newton", tol=tol, bootstrap=B, block=res.block, boot_seed=7)
    assert by_matrix.g is None and (by_matrix.block == res.block).all()
    m = M.block_resample(n_k, res.block, B, seed=7).multiplicities(0, B, "cpu").numpy()
    want = BR.weighted_newton(u, n_k, m, tol=1e-12, f0=res.f.cpu().numpy())
    for r in (res, by_matrix):
        fb = r.boot_f.cpu().numpy()
        worst = max(BR.weighted_residual(u, n_k, fb[b], m[b]) for b in range(B))
        print(f"  residual under the reference's weighted map {worst:.2e}, |boot_f - reference| {np.abs(fb - want).max():.2e}, "
              f"|boot_f - f| up to {np.abs(fb - r.f.cpu().numpy()).max():.3f}")
        assert worst <= tol + 1e-11 and (fb[:, 0] == r.f[0].item()).all()
        assert np.abs(fb - want).max() <= 1e-8 and np.abs(fb - r.f.cpu().numpy()).max() > 1e-2
        assert _close(r.f_error("bootstrap").cpu().numpy(), BR.boot_f_sigma(fb), 1e-9)
        assert np.abs(r.f_error("bootstrap").cpu().numpy() - BR.boot_f_sigma(want)).max() <= 1e-7
    again = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", tol=tol, bootstrap=B, boot_seed=7)
    assert torch.equal(again.boot_f, res.boot_f)
    other = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", tol=tol, bootstrap=B, boot_seed=8)
    assert not torch.equal(other.boot_f, res.boot_f)
    # bootstrap=0 is today's call, bit for bit, for both solvers
    for solver in M.SOLVERS:
        plain = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver=solver)
        named = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver=solver, bootstrap=0, block=3, boot_seed=5)
        assert torch.equal(plain.f, named.f) and torch.equal(plain.log_weights, named.log_weights)
        assert (plain.iterations, plain.delta) == (named.iterations, named.delta) and named.boot_f is None and named.g is None
    assert torch.equal(plain.f, res.f)
    with pytest.raises(ValueError, match="bootstrap > 0 requires solver='newton'"):
        M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, bootstrap=B)
    with pytest.raises(ValueError, match="block 'long'"):
        M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", bootstrap=B, block="long")


def test_one_replicate_of_ones_is_the_solution_and_the_iteration_cap():
    c, rs, xi, u = _correlated()
    n_k, N = c["n_k"], int(c["n_k"].sum())
    plan = M._MbarPlan(N, 6, DEV)
    plan.set_matrix(_dev(u), n_k)
    f, _, _ = plan.solve(1e-10, 100, 1, solver="newton")
    ones = _u16(np.ones((1, N)))
    delta = plan._bootstrap(f, [ones], 1e-10)
    assert delta.shape == (1, 6) and np.abs(delta.cpu().numpy()).max() <= 1e-10
    m = M.block_resample(n_k, 10, 40, seed=2)
    # two batches are the one batch's replicates
    whole = plan._bootstrap(f, m.batches(DEV), 1e-10)
    parts = plan._bootstrap(f, m.batches(DEV, max_bytes=2 * N * 25), 1e-10)
    assert whole.shape == (40, 6) and np.abs((whole - parts).cpu().numpy()).max() <= 1e-9
    with pytest.raises(M.MbarNotConverged, match=r"bootstrap not converged within max_iter = 1: \d+ of 40 replicates above tol.*worst delta") as e:
        plan._bootstrap(f, m.batches(DEV), 1e-10, max_iter=1)
    assert e.value.iterations == 1 and 1e-10 < e.value.delta < 1.0
    plan.close()
    with pytest.raises(M.MbarNotConverged, match="max_iter = 1"):
        M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", bootstrap=3, max_iter=1)


# ------------------------------------------------------------------------------------------------ 4
PMF_SEED, PMF_B, PMF_BLOCK = 0, 6, 4  # see _pmf_case: the seed is chosen so that the edge bins behave as the test needs


def _pmf_case():
    """K = 5 correlated windows of 60 frames; ten bins, the first and the last holding one frame each (the smallest and the
    largest xi).  A replicate that draws no block over such a frame leaves the bin empty."""
    c = BR.correlated_gaussian_case(K=5, n_per=60, phi=0.5, seed=1)
    x = np.sort(c["xi"][:, 0])
    edges = np.concatenate([[x[0] - 1.0], np.linspace(0.5 * (x[0] + x[1]), 0.5 * (x[-2] + x[-1]), 9), [x[-1] + 1.0]])
    return c, edges


@pytest.mark.parametrize("weighted", [False, True])
def test_bootstrap_error_bars_against_the_reference(weighted):
    c, edges = _pmf_case()
    n_k, x, kT = c["n_k"], c["xi"][:, 0], c["kT"]
    u, rs, xi = R.bias(c["table"], c["xi"], kT), _gaussian_set(c), _dev(c["xi"])
    w = np.random.default_rng(6).uniform(0.5, 1.5, len(x)) if weighted else None
    wd = None if w is None else _dev(w)
    pmf = M.UmbrellaPMF(restraints=rs, kT=kT, edges=edges, solver="newton")
    res = pmf.fit(xi, n_k=n_k, bootstrap=PMF_B, block=PMF_BLOCK, boot_seed=PMF_SEED)
    m = M.block_resample(n_k, PMF_BLOCK, PMF_B, seed=PMF_SEED).multiplicities(0, PMF_B, "cpu").numpy()
    first, last = int(np.argmin(x)), int(np.argmax(x))
    assert (m[:, first] > 0).sum() == 1 and 2 <= (m[:, last] > 0).sum() < PMF_B  # occupied in one replicate; empty in some
    fb = res.boot_f.cpu().numpy()
    F = BR.boot_profiles(u, n_k, fb, m, x, edges, kT, w)
    assert np.isinf(F[:, 0]).sum() == PMF_B - 1 and np.isinf(F[:, -1]).any() and np.isfinite(F[:, 1:-1]).all()
    got_F = pmf.boot_profiles(wd).cpu().numpy()
    assert (np.isinf(got_F) == np.isinf(F)).all() and _close(got_F[np.isfinite(F)], F[np.isfinite(F)], 1e-9)

    central = R.pmf(R.log_weights(u, n_k, res.f.cpu().numpy()), x, edges, kT, w)
    ref = int(np.argmin(central))
    want = BR.profile_sigma(F, ref)
    got = pmf.uncertainty(method="bootstrap", weights=wd).cpu().numpy()
    print(f"  weighted {weighted}: sigma(F_b - F_ref) up to {np.nanmax(want):.3f} kT, |got - want| {np.nanmax(np.abs(got - want)):.2e}")
    assert np.isnan(want[0]) and np.isnan(got[0]) and np.isfinite(want[1:]).all() and want[ref] == 0.0 and got[ref] == 0.0
    assert np.abs(got[1:] - want[1:]).max() <= 1e-9 and np.nanmax(want) > 0.05
    other = 3 if ref != 3 else 4
    assert np.abs(pmf.uncertainty(reference=other, method="bootstrap", weights=wd).cpu().numpy()[1:] - BR.profile_sigma(F, other)[1:]).max() <= 1e-9

    for level in (0.95, 0.5):
        want = BR.profile_interval(F, level)
        got = pmf.interval(level, weights=wd).cpu().numpy()
        assert got.shape == (2, 10) and np.isnan(got[:, 0]).all() and np.isnan(want[:, 0]).all()
        assert np.abs(got[:, 1:] - want[:, 1:]).max() <= 1e-9 and (got[0, 1:] <= got[1, 1:]).all()

    values = np.random.default_rng(9).normal(size=(len(x), 9)) + x[:, None]  # nine columns: two launches
    want = BR.expect_sigma(u, n_k, fb, m, values, w)
    got = pmf.expect_error(_dev(values), method="bootstrap", weights=wd).cpu().numpy()
    assert got.shape == (9,) and np.abs(got - want).max() <= 1e-9 and want.min() > 1e-3
    assert abs(float(pmf.expect_error(_dev(values[:, 0]), method="bootstrap", weights=wd)) - want[0]) <= 1e-9

    # the asymptotic error bars are what they were, and take no weights
    assert torch.equal(pmf.uncertainty()[1:], pmf.uncertainty(method="asymptotic")[1:])
    if weighted:
        with pytest.raises(ValueError, match="use method='bootstrap' with weights"):
            pmf.uncertainty(weights=wd)
        with pytest.raises(ValueError, match="use method='bootstrap' with weights"):
            pmf.expect_error(_dev(values), weights=wd)
    with pytest.raises(ValueError, match="method 'jackknife'"):
        pmf.uncertainty(method="jackknife")
    pmf.fit(xi, n_k=n_k)
    with pytest.raises(ValueError, match="fitted without bootstrap"):
        pmf.uncertainty(method="bootstrap")
    with pytest.raises(ValueError, match="fitted without bootstrap"):
        pmf.interval()
    pmf.release()
