"""GPU tests of the MBAR Gram matrix, segment moments, Newton solve and asymptotic error bars (mythos_amd/csrc/mbar.hip,
mythos_amd/observables/mbar.py) against the NumPy reference tests/mbar_newton_ref.py (checked without a GPU by
tests/test_mbar_newton_cpu.py).

  1  mythos_mbar_gram: G and the column sums at a random f, both sources; symmetry; repeatability
  2  mythos_mbar_segment_moments: segments of every length class, frames behind the last, an out-of-range entry
  3  the Newton solve through mbar_umbrella and mbar; the fixed-point keyword changes nothing
  4  MbarNotConverged and the unknown solver
  5  f_error, UmbrellaPMF.uncertainty and expect_error against the N x N definition
"""

import functools
import importlib

import numpy as np
import pytest
import torch

from mythos_amd.simulators.martini_restraints import MartiniRestraints, PullCoordinate, PullGroup
from tests import mbar_newton_ref as NR
from tests import mbar_ref as R

M = importlib.import_module("mythos_amd.observables.mbar")  # (the package also exports a function of this name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNK, GRAM_MAX_PARTIALS = 1024, 1024  # kMbarChunk, kGramMaxPartials of csrc/mbar.hip
TOL = 1e-11


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


class _Problem:
    """A case on the device through one source, with the reference's bias matrix and a random f (f_0 = 0)."""

    def __init__(self, case, src):
        self.c, self.K, self.N = case, len(case["n_k"]), int(case["n_k"].sum())
        self.u = R.bias(case["table"], case["xi"], case["kT"])
        assert np.abs(self.u).max() <= 1e3
        self.f = np.random.default_rng(5).uniform(-2.0, 2.0, self.K)
        self.f -= self.f[0]
        self.plan = M._MbarPlan(self.N, self.K, DEV)
        self._keep = _dev(case["xi"]) if src == "table" else _dev(self.u)
        if src == "table":
            self.plan.set_windows(case["table"], np.full(self.K, case["kT"]), case["n_k"], self._keep)
        else:
            self.plan.set_matrix(self._keep, case["n_k"])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.plan.close()


def _close(got, want):
    return (np.abs(got - want) <= TOL * (1.0 + np.abs(want))).all()


# ------------------------------------------------------------------------------------------------ 1
GRAM_CASES = {
    "K1": dict(n_k=(5,)),
    "K2": dict(n_k=(5, 1)),
    "K5": dict(n_k=(37, 64, 1, 65, 130)),
    "K5_far": dict(n_k=(37, 64, 1, 65, 130), far=True, spacing=1.0, k0=0.5, k=9.5),
    "P2": dict(n_k=(37, 64, 1, 65, 130), P=2),
    "K65": dict(n_k=tuple(1 + (7 * i) % 5 for i in range(65)), spacing=0.3),     # one window into a second tile
    "K129": dict(n_k=tuple(1 + (7 * i) % 5 for i in range(129)), spacing=0.3),   # three tiles: the pair (0, 2)
    "chunk_plus_1": dict(n_k=(CHUNK, 1)),
    # one tile pair: min(chunks, 1024) frame blocks, so this is one chunk (of one frame) more than a pass of their stride
    "stride_plus_1": dict(n_k=(CHUNK * GRAM_MAX_PARTIALS - 7, 8)),
}


@pytest.mark.parametrize("src", ["table", "matrix"])
@pytest.mark.parametrize("name", list(GRAM_CASES))
def test_gram_and_column_sums_against_the_reference(name, src):
    """G = W^T W and s = W^T 1 at a random f, |got - want| <= 1e-11 (1 + |want|) on inputs with |b| <= 10^3.
    Where the figure comes from: tests/test_gpu_mbar.py bounds the absolute error of the exponent f_k - b_k(n) - L_n below
    1.5e-12, which is a relative error of W_nk and twice that, 3e-12, of a product W_ni W_nj.  The sums are of positive
    terms, so they add their depth times 2^-53 relative.  A Gram entry is one fma chain over the frames of its workgroup - one
    chunk of 1 024 while there are at most 1 024 / pairs chunks, two in the last case - and then a chain over at most 1 024
    frame-block partials: 3 072 * 2^-53 = 3.4e-13.  A column sum is four terms of a thread, seven wavefront steps, the rounds
    of a workgroup (one or two here), four wavefronts and a chain over at most 1 024 splits: 1.2e-13.  The reference (a
    matrix product and a pairwise sum of the materialised W) adds less.  Together 3.4e-12: 1e-11 holds a margin of three."""
    with _Problem(_windows_case(**GRAM_CASES[name]), src) as p:
        want_g, want_s = NR.gram(p.u, p.c["n_k"], p.f)
        f = _dev(p.f)
        g, s = p.plan.gram(f)
        g2, s2 = p.plan.gram(f)
        g3, none = p.plan.gram(f, colsum=False)
        got_g, got_s = g.cpu().numpy(), s.cpu().numpy()
        assert torch.equal(f, _dev(p.f)) and none is None
        assert torch.equal(g, g2) and torch.equal(s, s2) and torch.equal(g, g3)
    err_g = (np.abs(got_g - want_g) / (1.0 + np.abs(want_g))).max()
    err_s = (np.abs(got_s - want_s) / (1.0 + np.abs(want_s))).max()
    print(f"  {name} {src}: K = {p.K}, N = {p.N}: G {err_g:.2e}, s {err_s:.2e} (of 1 + |want|), largest G {want_g.max():.3e}")
    assert np.isfinite(got_g).all() and (got_g == got_g.T).all()
    assert _close(got_g, want_g) and _close(got_s, want_s)
    # the identity behind the covariance's null vector, at any f: sum_k N_k W_nk = 1, so G n = s
    assert np.abs(got_g @ p.c["n_k"] - got_s).max() <= 1e-10 * (1.0 + np.abs(got_s).max())


def test_gram_where_the_table_leaves_room_for_fewer_frames_per_step_and_for_none():
    """The strip step holds 32 frames while K (3 P + 1) + 32 x 130 doubles fit 64 KB; 129 windows of 16 coordinates leave room
    for 8 (128 x 49 + 8 x 130 = 7 312 of 8 192 doubles; 16 frames would need 8 352), and two windows of 1 360 coordinates for
    none, which is refused by name.  Same reference, same tolerance."""
    c = _windows_case(tuple(1 + (7 * i) % 5 for i in range(129)), spacing=0.3)
    K, N, P = 129, int(c["n_k"].sum()), 16
    rng = np.random.default_rng(31)
    more = np.zeros((K, P - 1, 4))
    more[:, :, 1], more[:, :, 2] = rng.uniform(0.0, 2.0, (K, P - 1)), rng.uniform(0.0, 1.0, (K, P - 1))
    c["table"] = np.ascontiguousarray(np.concatenate([c["table"], more], axis=1))
    c["xi"] = np.ascontiguousarray(np.concatenate([c["xi"], rng.uniform(0.0, 1.0, (N, P - 1))], axis=1))
    with _Problem(c, "table") as p:
        want_g, want_s = NR.gram(p.u, c["n_k"], p.f)
        g, s = p.plan.gram(_dev(p.f))
        got_g, got_s = g.cpu().numpy(), s.cpu().numpy()
    assert (got_g == got_g.T).all() and _close(got_g, want_g) and _close(got_s, want_s)
    K, N, P = 2, 3, 1360
    table = np.zeros((K, P, 4))
    table[:, :, 1] = 1.0
    plan = M._MbarPlan(N, K, DEV)
    xi = _dev(rng.uniform(0.0, 1.0, (N, P)))
    plan.set_windows(table, np.ones(K), np.array([2, 1]), xi)
    f = torch.zeros(K, dtype=torch.float64, device=DEV)
    assert plan.segment_moments(f).shape == (1, K)  # the iterate kernel's layout still fits
    with pytest.raises(ValueError, match="leaves no LDS for a strip of W"):
        plan.gram(f)
    plan.close()


# ------------------------------------------------------------------------------------------------ 2
SEG_LENGTHS = (0, 1, 255, 256, 257, 1025)  # then 7 frames behind the last segment
SEG_CASES = {"K5": (400, 400, 400, 400, 201), "K65": (27,) * 64 + (73,)}


@pytest.mark.parametrize("src", ["table", "matrix"])
@pytest.mark.parametrize("name", list(SEG_CASES))
def test_segment_moments_against_the_reference(name, src):
    """out[b][k] = sum over segment b of v_n W_nk to the tolerance of the Gram test (the column sum's reduction: its 1 801
    frames are two rounds, dealt to two workgroups per segment, so the split and its finish kernel run here)."""
    n_k = SEG_CASES[name]
    N = sum(n_k)
    assert N == sum(SEG_LENGTHS) + 7
    rng = np.random.default_rng(17)
    order = rng.permutation(N)
    seg = np.concatenate([[0], np.cumsum(SEG_LENGTHS)])
    segments = [order[seg[b]:seg[b + 1]] for b in range(len(SEG_LENGTHS))]
    v = rng.uniform(0.0, 1.0, N)
    with _Problem(_windows_case(n_k, spacing=1.5 if name == "K5" else 0.3), src) as p:
        f, order_d, seg_d = _dev(p.f), _dev(order, torch.int64), _dev(seg, torch.int64)
        for vv in (None, v):
            want = NR.segment_moments(p.u, n_k, p.f, segments, vv)
            got = p.plan.segment_moments(f, seg_d, order_d, None if vv is None else _dev(vv))
            assert torch.equal(got, p.plan.segment_moments(f, seg_d, order_d, None if vv is None else _dev(vv)))
            got = got.cpu().numpy()
            assert got.shape == (len(SEG_LENGTHS), p.K) and (got[0] == 0.0).all() and _close(got, want)
            whole = p.plan.segment_moments(f, v=None if vv is None else _dev(vv)).cpu().numpy()
            assert whole.shape == (1, p.K) and _close(whole, NR.segment_moments(p.u, n_k, p.f, [np.arange(N)], vv))
        # entries of the order that name no frame are skipped, never dereferenced
        bad = order.copy()
        at = [seg[3] + 5, seg[5] + 1000]
        bad[at[0]], bad[at[1]] = N + 5, -1
        keep = [np.array([n for i, n in enumerate(s, start=seg[b]) if i not in at]) for b, s in enumerate(segments)]
        got = p.plan.segment_moments(f, seg_d, _dev(bad, torch.int64), _dev(v)).cpu().numpy()
        assert _close(got, NR.segment_moments(p.u, n_k, p.f, keep, v))
        with pytest.raises(ValueError, match="come together"):
            p.plan.segment_moments(f, seg_d, None)
    fresh = M._MbarPlan(10, 2, DEV)
    with pytest.raises(M._lib.MythosHipError, match="neither windows nor a matrix"):
        fresh.segment_moments(torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(M._lib.MythosHipError, match="neither windows nor a matrix"):
        fresh.gram(torch.zeros(2, dtype=torch.float64, device=DEV))
    fresh.close()


# ------------------------------------------------------------------------------------------------ 3
def _gaussian_set(c):
    return MartiniRestraints(pulls=[PullCoordinate(group_a=None, group_b=PullGroup(members=(0,)), geometry="direction", vec=(0, 0, 1),
                                                   k=c["k"], init=c["table"][:, 0, 2].copy(), periodic=False)])


@functools.lru_cache(maxsize=None)
def _solved():
    c = R.gaussian_case(K=8, n_per=100, seed=21)
    return c, _gaussian_set(c), _dev(c["xi"]), R.bias(c["table"], c["xi"], c["kT"])


def test_newton_through_the_public_interface():
    c, rs, xi, u = _solved()
    res = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], solver="newton", tol=1e-10)
    by_matrix = M.mbar(_dev(u), c["n_k"], solver="newton")
    for r in (res, by_matrix):
        f = r.f.cpu().numpy()
        moved = np.abs(R.iterate(u, c["n_k"], f)[0] - f).max()
        print(f"  {r.iterations} Newton iterations, delta {r.delta:.2e}; the reference's map moves the GPU's f by {moved:.2e}")
        assert moved <= 1e-10 and r.delta <= 1e-10 and f[0] == 0.0 and r.iterations <= 25 and r.theta is None
        assert np.abs(r.log_weights.cpu().numpy() - R.log_weights(u, c["n_k"], f)).max() <= TOL
    again = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], solver="newton", tol=1e-10)
    assert torch.equal(again.f, res.f) and torch.equal(again.log_weights, res.log_weights) and again.iterations == res.iterations
    # the keyword's default is today's path, bit for bit
    plain = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"])
    named = M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], solver="fixed-point")
    assert torch.equal(plain.f, named.f) and torch.equal(plain.log_weights, named.log_weights)
    assert (plain.iterations, plain.delta) == (named.iterations, named.delta)
    assert np.abs(plain.f.cpu().numpy() - res.f.cpu().numpy()).max() <= 1e-6
    with pytest.raises(ValueError, match="without uncertainties"):
        plain.f_error()


# ------------------------------------------------------------------------------------------------ 4
def test_newton_out_of_iterations_and_an_unknown_solver():
    c, rs, xi, u = _solved()
    with pytest.raises(M.MbarNotConverged, match=r"max_iter = 1.*Newton.*delta") as e:
        M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], solver="newton", max_iter=1)
    assert e.value.iterations == 1 and e.value.delta > 1e-10 and np.isfinite(e.value.delta)
    with pytest.raises(ValueError, match="solver 'bfgs'"):
        M.mbar_umbrella(xi, rs, c["kT"], n_k=c["n_k"], solver="bfgs")
    with pytest.raises(ValueError, match="solver 'bfgs'"):
        M.mbar(_dev(u), c["n_k"], solver="bfgs")
    with pytest.raises(ValueError, match="solver 'bfgs'"):
        M.UmbrellaPMF(restraints=rs, kT=c["kT"], edges=[0.0, 1.0], solver="bfgs")


# ------------------------------------------------------------------------------------------------ 5
def _sigma_tolerance(G, n, pick):
    """Ten times the largest change of any sigma that ``pick`` takes from Theta when the reference Gram matrix is perturbed by
    1e-11 (1 + |G|) times a random symmetric matrix in [-1, 1], 16 draws: what the tolerance of test 1 can do to an error
    bar.  From the reference alone."""
    rng = np.random.default_rng(23)
    base = pick(NR.theta_eig(G, n))
    worst = 0.0
    for _ in range(16):
        r = rng.uniform(-1.0, 1.0, G.shape)
        worst = max(worst, np.abs(pick(NR.theta_eig(G + 1e-11 * (1.0 + np.abs(G)) * 0.5 * (r + r.T), n)) - base).max())
    return 10.0 * worst


@pytest.mark.parametrize("name", ["K5", "K4x3"])
def test_error_bars_against_the_definition(name):
    """f_error, uncertainty and expect_error against theta_direct at the f the GPU solved; the tolerance is computed here from
    the reference (``_sigma_tolerance``; about 1e-9 for distinct windows and 6e-6 for tripled ones, sigma up to 0.87)."""
    c = R.gaussian_case(**(dict(K=5, n_per=40, seed=1) if name == "K5" else dict(K=4, n_per=25, copies=3, seed=3)))
    K, n_k, x = len(c["n_k"]), c["n_k"], c["xi"][:, 0]
    u, rs, xi = R.bias(c["table"], c["xi"], c["kT"]), _gaussian_set(c), _dev(c["xi"])
    # six bins, the first of them empty
    edges = np.concatenate([[x.min() - 1.0], np.linspace(x.min(), x.max() + 1e-9, 6)])
    res = M.mbar_umbrella(xi, rs, c["kT"], n_k=n_k, solver="newton", uncertainties=True)
    f = res.f.cpu().numpy()
    W = NR.weights_matrix(u, n_k, f)
    counts = n_k.astype(np.float64)

    tol_f = _sigma_tolerance(W.T @ W, counts, NR.sigma)
    got = res.f_error().cpu().numpy()
    want = NR.sigma(NR.theta_direct(W, counts))
    print(f"  {name}: f_error |got - want| {np.abs(got - want).max():.2e}, allowed {tol_f:.2e}, sigma up to {want.max():.3f}")
    assert res.theta.shape == (K, K) and res.theta.dtype == torch.float64 and res.theta.is_cuda
    assert np.abs(got - want).max() <= tol_f and (np.diag(got) == 0.0).all()
    by_matrix = M.mbar(_dev(u), n_k, solver="newton", uncertainties=True)
    assert np.abs(by_matrix.f_error().cpu().numpy() - want).max() <= tol_f

    pmf = M.UmbrellaPMF(restraints=rs, kT=c["kT"], edges=edges, solver="newton")
    assert torch.equal(pmf.fit(xi, n_k=n_k).f, res.f)
    F = pmf().cpu().numpy()
    G, n_aug, occ = NR.pmf_gram(u, n_k, f, x, edges)
    ref_bin = int(occ[np.argmin(F[occ])])
    at = K + int(np.searchsorted(occ, ref_bin))
    tol_b = c["kT"] * _sigma_tolerance(G, n_aug, lambda t: NR.sigma(t)[K:, at])
    want = NR.pmf_sigma(u, n_k, f, x, edges, c["kT"])
    got = pmf.uncertainty().cpu().numpy()
    print(f"  {name}: uncertainty |got - want| {np.nanmax(np.abs(got - want)):.2e}, allowed {tol_b:.2e}, sigma up to {np.nanmax(want):.3f}")
    assert list(occ) == [1, 2, 3, 4, 5] and np.isposinf(F[0])
    assert np.isnan(got[0]) and np.isnan(want[0]) and got[ref_bin] == 0.0 and np.isfinite(got[1:]).all()
    assert np.abs(got[1:] - want[1:]).max() <= tol_b and np.nanmax(want) > 0.1
    assert torch.equal(pmf.uncertainty(reference=ref_bin)[1:], pmf.uncertainty()[1:])
    other = int(occ[-1]) if ref_bin != occ[-1] else int(occ[0])
    want = NR.pmf_sigma(u, n_k, f, x, edges, c["kT"], reference=other)
    assert np.abs(pmf.uncertainty(reference=other).cpu().numpy()[1:] - want[1:]).max() <= tol_b
    with pytest.raises(ValueError, match="reference bin 0 is empty"):
        pmf.uncertainty(reference=0)
    with pytest.raises(ValueError, match="expected 'min' or a bin index"):
        pmf.uncertainty(reference=6)

    values = np.random.default_rng(9).normal(size=(len(x), 2))
    got = pmf.expect_error(_dev(values)).cpu().numpy()
    lw = R.log_weights(u, n_k, f)
    for e in range(2):
        cols, mean = NR.expect_columns(lw, values[:, e])
        Wa = NR.augmented(W, cols)
        tol_e = mean * _sigma_tolerance(Wa.T @ Wa, np.concatenate([counts, np.zeros(2)]), lambda t: NR.sigma(t)[K, K + 1])
        want = NR.expect_sigma(u, n_k, f, values[:, e])
        print(f"  {name}: expect_error[{e}] |got - want| {abs(got[e] - want):.2e}, allowed {tol_e:.2e}, sigma {want:.3f}")
        assert abs(got[e] - want) <= tol_e and want > 0.01
    assert got.shape == (2,) and pmf.expect_error(_dev(values[:, 0])).shape == ()
    assert abs(float(pmf.expect_error(_dev(values[:, 0]))) - got[0]) <= 1e-12
    pmf.release()
    with pytest.raises(M._lib.MythosHipError, match="fit"):
        pmf.uncertainty()
