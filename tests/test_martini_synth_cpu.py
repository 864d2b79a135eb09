"""The synthetic MARTINI systems of tests/martini_synth.py on the host: every named system meets ``check``, and two
independent references agree on them - the torch oracle (oracle/martini_oracle.py, autograd forces) and the double
build of the kernels' term functions (oracle/cpu_port/martini_cpu.cpp) - within the tolerances tests/test_cpu_port.py
holds them to on the bilayer fixture.  What the two differ by is printed per system and term: it is the floor under the
tolerances of tests/test_gpu_martini_shapes.py, whose docstring records the numbers."""

import subprocess

import numpy as np
import pytest

from oracle import cpu_port
from oracle import martini_oracle as mo
from tests import martini_synth as S

KT = 0.0083144626 * 273.0
SMALL = [name for name, kw in S.SYSTEMS.items() if kw["n"] <= 1285]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not cpu_port.LIB.exists():
        subprocess.run(["make", "-C", str(cpu_port.BUILD.parent)], check=True, capture_output=True)


@pytest.mark.parametrize("name", list(S.SYSTEMS))
def test_every_named_system_meets_the_conditions(name):
    s = S.get(name)
    S.check(s)
    kw = S.SYSTEMS[name]
    assert s["pos"].shape == (kw.get("frames", 1), kw["n"], 3) and s["box"].shape == (kw.get("frames", 1), 3)
    occurring = set(np.unique(s["types"]).tolist())
    assert occurring <= {1, 4, 6} and s["sigma"].shape == (7, 7)
    if kw["n"] >= 27:
        assert occurring == {1, 4, 6}
    for tab, lo, hi in ((s["sigma"], 0.43, 0.62), (s["eps"], 2.0, 5.6)):
        assert np.array_equal(tab, tab.T) and np.unique(tab[np.triu_indices(7)]).size == 28 and lo <= tab.min() and tab.max() <= hi
    if kw.get("images"):
        assert np.abs(s["shift"]).max() == kw["images"] or kw["n"] < 3
    again = S.make(**kw) if kw["n"] <= 300 else None  # deterministic
    assert again is None or all(np.array_equal(again[k], s[k]) for k in ("pos", "box", "bonds", "angles", "types", "bond_k"))


def _port(s, angle_kind, mass=None):
    return cpu_port.MartiniCpuPort(s["types"], s["sigma"], s["eps"], s["bonds"], s["bond_k"], s["bond_r0"], s["angles"], s["angle_k"],
                                   s["angle_t0"], angle_kind=angle_kind, mass=mass)


@pytest.mark.parametrize("angle_kind", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_oracle_and_port_agree_on_energies_and_forces(name, angle_kind):
    s = S.get(name)
    S.check(s)
    port = _port(s, angle_kind)
    for f in sorted({0, s["pos"].shape[0] - 1}):
        e_o, g_o = mo.energies_and_forces(*S.oracle_args(s, f), angle_kind == 0)
        e_o, g_o = e_o.numpy(), g_o.numpy()
        e, g = port.energy(s["pos"][f], s["box"][f])
        rel = np.abs(e - e_o) / np.maximum(np.abs(e_o), 1e-300)
        gmax = np.abs(g_o).max()
        print(f"{name} kind {angle_kind} frame {f}: rel. energy difference lj {rel[0]:.1e} bond {rel[1]:.1e} angle {rel[2]:.1e}; "
              f"force difference / max|g| {np.abs(g - g_o).max() / max(gmax, 1e-300):.1e} (max|g| {gmax:.3g})")
        np.testing.assert_allclose(e, e_o, rtol=1e-10)
        np.testing.assert_allclose(g, g_o, rtol=0, atol=1e-9 * gmax)


@pytest.mark.parametrize("name", ["md37", "dilute520"])
def test_oracle_and_port_agree_on_five_langevin_steps(name):
    from oracle.martini_langevin_oracle import MartiniLangevinOracle

    s = S.get(name)
    S.check(s)
    port = _port(s, 0, s["mass"])
    x0, b0 = s["pos"][0].copy(), s["box"][0].copy()
    v0 = 0.3 * np.random.default_rng(5).standard_normal(x0.shape)
    xp, vp = x0.copy(), v0.copy()
    builds, e4 = port.run(xp, vp, b0, 5, dt=0.01, kT=KT, gamma=2.0, seed=0xABCDEF012345, skin=0.25, rebuild_every=2)
    assert builds == 3
    a = S.oracle_args(s)
    orc = MartiniLangevinOracle(*a[2:], True, b0, 0.01, KT, 2.0, s["mass"], seed=0xABCDEF012345)
    xo, vo = x0.copy(), v0.copy()
    e_ref = orc.run(xo, vo, 5)
    print(f"{name}: after 5 steps max |dx| {np.abs(xp - xo).max():.1e} max |dv| {np.abs(vp - vo).max():.1e}; "
          f"energy difference {np.abs(e4 - e_ref[-1]).max():.1e} of {np.abs(e_ref[-1]).max():.3g}; moved {np.abs(xo - x0).max():.3f} nm")
    np.testing.assert_allclose(xp, xo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(vp, vo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(e4, e_ref[-1], rtol=1e-9, atol=1e-7)
