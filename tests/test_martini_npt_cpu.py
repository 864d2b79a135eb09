"""Pins tests/martini_npt_ref.py, the CPU side of tests/test_gpu_martini_npt.py: the strain virial against central
differences, and the statistics of the barostat's noise term on an ideal gas."""

import numpy as np
import pytest

from tests import martini_npt_ref as NR
from tests import martini_synth as S


@pytest.mark.parametrize("name,angle_kind", [("md37", 0), ("md37", 1), ("n257", 0)])
def test_strain_virial_equals_central_differences(name, angle_kind):
    """-dU/ds by autograd through torch.remainder(d + box / 2, box) against (U(1 + h) - U(1 - h)) / 2h, h = 1e-6: the
    truncation error is O(h^2 U''') ~ 1e-12 relative and the round-off ~ 1e-16 |U| / h ~ 1e-10 |U|; bound 1e-8 of max |W|."""
    s = S.get(name)
    a = S.oracle_args(s)
    w = NR.strain_virial(*a, angle_kind == 0)
    w_fd = NR.strain_virial_fd(*a, angle_kind == 0)
    print(f"  {name}: W {w}, central differences {w_fd}")
    assert np.abs(w).max() > 1.0
    np.testing.assert_allclose(w, w_fd, rtol=0, atol=1e-8 * np.abs(w).max())


@pytest.mark.parametrize("coupling,beta_z_on", [("isotropic", True), ("semiisotropic", False), ("semiisotropic", True)],
                         ids=["iso", "semi-z-fixed", "semi"])
def test_ideal_gas_statistics_of_the_numpy_barostat(coupling, beta_z_on):
    """<V> = (N + 1) kT / P0 and Var V / <V>^2 = 1 / (N + 1): the bounds the GPU test uses.  An amplitude of the noise
    wrong by sqrt(2) puts the ratio near 0.5 or 2."""
    n, kT = 64, 2.27
    V, p0 = NR.ideal_gas_volumes(coupling, beta_z_on, 20_000, n=n, kT=kT, seed=7)
    z, ratio = NR.volume_statistics(V, n, kT, p0)
    print(f"  {coupling} beta_z {'on' if beta_z_on else 'off'}: <V> {V[2000:].mean():.2f} of {(n + 1) * kT / p0:.2f}, z {z:+.2f}, ratio {ratio:.3f}")
    assert abs(z) <= 4.0
    assert 0.75 <= ratio <= 1.35
