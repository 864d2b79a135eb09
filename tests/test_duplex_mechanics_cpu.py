"""Host side of the duplex-mechanics feature: the closed-form stretch / torsion fits and the worm-like-chain fit against
the reference's own known answers (mythos/observables/tests/test_stretch_torsion.py:210-305, test_wlc.py:13-103), the
derivative of the fit against finite differences, the external-force file parser, and the numpy checker of the GPU
observables (tests/duplex_ref.py) against the numbers of the reference's tests (test_diameter.py:16-103,
test_stretch_torsion.py:17-57, 112-206)."""

import math

import numpy as np
import pytest
import torch

from mythos_amd.input.external_forces import read_external_forces
from mythos_amd.observables import calculate_extension, coth, fit_wlc, loss, stretch, stretch_torsion, torsion
from mythos_amd.utils import units
from tests import duplex_ref as DR

F5 = [0.0, 1.0, 2.0, 3.0, 4.0]
ZERO3 = (0.0, 0.0, 0.0)


def test_stretch_and_torsion_known_answers():
    a1, l0, s_eff = stretch(F5, [10.0, 12.0, 14.0, 16.0, 18.0])
    np.testing.assert_allclose([float(a1), float(l0), float(s_eff)], [2.0, 10.0, 5.0], atol=1e-5)
    a1, l0, s_eff = stretch(F5, [10.0] * 5)
    np.testing.assert_allclose([float(a1), float(l0)], [0.0, 10.0], atol=1e-5)
    assert abs(float(s_eff)) > 1e5
    a3, a4 = torsion(F5, [10.0, 10.5, 11.0, 11.5, 12.0], [1.0, 2.5, 4.0, 5.5, 7.0])
    np.testing.assert_allclose([float(a3), float(a4)], [0.5, 1.5], atol=1e-5)
    a3, a4 = torsion(F5, [10.0] * 5, [5.0] * 5)
    np.testing.assert_allclose([float(a3), float(a4)], [0.0, 0.0], atol=1e-5)
    got = stretch_torsion(F5, [10.0, 12.0, 14.0, 16.0, 18.0], F5, [10.0, 10.5, 11.0, 11.5, 12.0], [1.0, 2.5, 4.0, 5.5, 7.0])
    np.testing.assert_allclose([float(v) for v in got], [5.0, 20.0 / 2.75, -5.0 / 2.75], atol=1e-5)
    got = stretch_torsion(F5, [10.0, 12.0, 14.0, 16.0, 18.0], F5, [10.0] * 5, [1.0, 2.5, 4.0, 5.5, 7.0])
    np.testing.assert_allclose([float(v) for v in got], [5.0, 20.0 / 3.0, 0.0], atol=1e-5)


def test_the_line_fits_are_differentiable():
    ext = torch.tensor([10.0, 12.1, 13.9, 16.2, 18.0], dtype=torch.float64, requires_grad=True)
    a1, l0, s_eff = stretch(torch.tensor(F5, dtype=torch.float64), ext)
    (g,) = torch.autograd.grad(a1, ext)
    f = np.array(F5)
    np.testing.assert_allclose(g.numpy(), (f - f.mean()) / ((f - f.mean()) ** 2).sum(), rtol=1e-12)
    assert s_eff.dtype == torch.float64


def test_coth_and_calculate_extension_against_the_literal_formulas():
    for x in (1.0, 2.0, 3.0):
        np.testing.assert_allclose(float(coth(x)), (np.exp(2 * x) + 1) / (np.exp(2 * x) - 1), rtol=1e-14)

    def literal(force, l0, lp, k, kT):  # noqa: N803
        y = ((force * l0**2) / (lp * kT)) ** (1 / 2)
        return l0 * (1 + force / k - kT / (2 * force * l0) * (1 + y * (np.exp(2 * y) + 1) / (np.exp(2 * y) - 1)))

    np.testing.assert_allclose(float(calculate_extension(1, 1, 1, 1, 1)), literal(1.0, 1.0, 1.0, 1.0, 1.0), rtol=1e-14)
    f = np.array([0.05, 0.3, 0.75])
    np.testing.assert_allclose(calculate_extension(f, 39.87, 50.6, 44.54, 0.0987).numpy(), literal(f, 39.87, 50.6, 44.54, 0.0987), rtol=1e-13)
    np.testing.assert_allclose(loss(np.ones(3), np.ones(3), np.ones(3), 1).numpy(), 1.0 - literal(np.ones(3), 1.0, 1.0, 1.0, 1.0), rtol=1e-13)


# mythos/observables/tests/test_wlc.py:82-103 ("values provided by T. Ouldridge")
WLC_FORCES = np.array([0.025, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.375]) * 2.0
WLC_EXTENSIONS = np.array([35.0, 36.67, 37.84, 38.37, 38.71, 38.98, 39.19, 39.46])
WLC_START = np.array([39.87, 50.60, 44.54])
WLC_KT = units.get_kt(296.15)


def test_fit_wlc_reproduces_the_references_fit():
    res = fit_wlc(WLC_EXTENSIONS, WLC_FORCES, WLC_START, WLC_KT)
    assert res.dtype == torch.float64 and res.shape == (3,)
    got = [float(res[0]) * units.NM_PER_OXDNA_LENGTH, float(res[1]) * units.NM_PER_OXDNA_LENGTH, float(res[2]) * units.PN_PER_OXDNA_FORCE]
    np.testing.assert_allclose(got, [33.951588, 43.467876, 2131.197638], rtol=1e-4)
    # the point returned is stationary: grad_p 1/2 |r|^2 = 0 to rounding
    p = res.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(0.5 * (loss(p, WLC_EXTENSIONS, WLC_FORCES, WLC_KT) ** 2).sum(), p)
    assert float((g.abs() * p.detach().abs()).max()) < 1e-10
    with pytest.raises(ValueError, match="implicit_diff"):
        fit_wlc(torch.tensor(WLC_EXTENSIONS, requires_grad=True), WLC_FORCES, WLC_START, WLC_KT, implicit_diff=False)


def test_fit_wlc_gradient_against_finite_differences():
    """d(fit)/d(extensions) by the implicit function theorem against central differences (h = 1e-5) of the fit itself,
    per parameter as max |difference| / max |derivative|.  Measured: full Hessian 1.1e-9, 6.8e-10, 1.4e-9 for L0, Lp, K;
    the Gauss-Newton J^T J alone 5.0e-4, 3.7e-4, 3.8e-4 (the fitted residuals do not vanish).  Asserted: the full
    Hessian ten times above its measured value, and J^T J where it was measured (a factor of 1e4 away)."""
    h = 1e-5
    fd = np.zeros((3, 8))
    for i in range(8):
        e = np.zeros(8)
        e[i] = h
        fd[:, i] = (fit_wlc(WLC_EXTENSIONS + e, WLC_FORCES, WLC_START, WLC_KT) - fit_wlc(WLC_EXTENSIONS - e, WLC_FORCES, WLC_START, WLC_KT)).numpy() / (2 * h)

    def jac(full):
        x = torch.tensor(WLC_EXTENSIONS, requires_grad=True)
        return np.stack([torch.autograd.grad(fit_wlc(x, WLC_FORCES, WLC_START, WLC_KT, full_hessian=full)[k], x)[0].numpy() for k in range(3)])

    dist = {full: np.abs(jac(full) - fd).max(axis=1) / np.abs(fd).max(axis=1) for full in (True, False)}
    print("full Hessian", dist[True], "J^T J", dist[False])
    assert (dist[True] <= 1.4e-8).all(), dist[True]
    assert (dist[False] > 1e-5).all() and (dist[False] < 5e-3).all(), dist[False]


def _write(tmp_path, text):
    path = tmp_path / "external.conf"
    path.write_text(text)
    return path


BLOCK = "{{\ntype = {type}\nparticle = {particle}\nF0 = {f0}\nrate = {rate}\ndir = {dir}\n}}\n"


def test_external_force_files(tmp_path):
    two = BLOCK.format(type="string", particle="5,214", f0=0.025, rate="0.", dir="0., 0., 1.") + \
        BLOCK.format(type="string", particle="104,115", f0=0.025, rate="0.", dir="0., 0., -1.")
    idx, f = read_external_forces(_write(tmp_path, two))
    assert idx.dtype == np.int32 and f.dtype == np.float64
    np.testing.assert_array_equal(idx, [5, 104, 115, 214])
    np.testing.assert_array_equal(f, [[0, 0, 0.025], [0, 0, -0.025], [0, 0, -0.025], [0, 0, 0.025]])
    # dir is normalised, as oxDNA does
    idx, f = read_external_forces(_write(tmp_path, BLOCK.format(type="string", particle="3", f0=2.0, rate=0, dir="3, 0, 4")))
    np.testing.assert_array_equal(idx, [3])
    np.testing.assert_allclose(f, [[1.2, 0.0, 1.6]], rtol=1e-15)
    # every particle
    everyone = _write(tmp_path, BLOCK.format(type="string", particle="-1", f0=0.5, rate=0, dir="0, 1, 0"))
    idx, f = read_external_forces(everyone, n=6)
    np.testing.assert_array_equal(idx, np.arange(6))
    np.testing.assert_array_equal(f, np.tile([0.0, 0.5, 0.0], (6, 1)))
    with pytest.raises(ValueError, match="needs the number of nucleotides"):
        read_external_forces(everyone)
    # a particle named twice gets the sum
    twice = BLOCK.format(type="string", particle="2,7", f0=1.0, rate=0, dir="1, 0, 0") + BLOCK.format(type="string", particle="7", f0=0.5, rate=0, dir="0, 0, 1")
    idx, f = read_external_forces(_write(tmp_path, twice), n=10)
    np.testing.assert_array_equal(idx, [2, 7])
    np.testing.assert_array_equal(f, [[1.0, 0, 0], [1.0, 0, 0.5]])
    with pytest.raises(ValueError, match="type = trap"):
        read_external_forces(_write(tmp_path, BLOCK.format(type="trap", particle="1", f0=1.0, rate=0, dir="1, 0, 0")))
    with pytest.raises(ValueError, match="rate = 1"):
        read_external_forces(_write(tmp_path, BLOCK.format(type="string", particle="1", f0=1.0, rate=1, dir="1, 0, 0")))
    with pytest.raises(ValueError, match="out of range"):
        read_external_forces(_write(tmp_path, BLOCK.format(type="string", particle="12", f0=1.0, rate=0, dir="1, 0, 0")), n=10)


def _ident(frames, n):
    q = np.zeros((frames, n, 4))
    q[..., 0] = 1.0
    return q


def test_duplex_ref_reproduces_the_reference_tests_numbers():
    c = np.tile(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], dtype=np.float64), (5, 1, 1))
    np.testing.assert_allclose(DR.diameter(c, _ident(5, 3), [[0, 1], [1, 2]], ZERO3, 2, 1.0), [23.271608] * 5, rtol=1e-7)
    ext = [([[0, 0, 0], [2, 0, 0], [0, 0, 5], [2, 0, 5]], 5.0), ([[0, 0, 10], [2, 0, 10], [0, 0, 3], [2, 0, 3]], 7.0),
           ([[0, 0, 5], [2, 0, 5], [4, 0, 5], [6, 0, 5]], 0.0), ([[0, 0, 0], [2, 0, 0], [0, 0, 10], [2, 0, 10]], 10.0)]
    for centers, want in ext:
        np.testing.assert_allclose(DR.extension_z(np.array([centers], dtype=np.float64), (0, 1), (2, 3)), [want], atol=1e-6)
    tw = [([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], 0.0), ([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 1]], math.pi / 2),
          ([[0, 0, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 1]], math.pi)]
    for centers, want in tw:
        np.testing.assert_allclose(DR.twist_xy(np.array([centers], dtype=np.float64), _ident(1, 4), [[[0, 1], [2, 3]]], ZERO3, 2), [want], atol=1e-6)
    # rmsd: a rotated and shifted copy is the target; a mirror image is not
    rng = np.random.default_rng(0)
    t = rng.standard_normal((12, 3)) * [1.0, 2.0, 5.0]
    a = 0.7
    rot = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    np.testing.assert_allclose(DR.rmsd(t, (t @ rot.T + [3.0, -1.0, 2.0])[None]), [0.0], atol=1e-13)
    assert DR.rmsd(t, (t * [-1.0, 1.0, 1.0])[None])[0] > 0.1
