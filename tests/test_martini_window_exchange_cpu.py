"""Window exchange between the umbrella windows of the MARTINI ensemble, checked without a device: the NumPy restatement
(tests/martini_window_exchange_ref.py), the rule on an exactly sampled toy, the host logic of
mythos_amd/csrc/martini_window_exchange_checks.h under the host sanitizers, the new entry points, and every refusal that
needs no handle (mythos_martini_window_exchange_check), raised with the library's message."""

import ctypes as C
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.simulators.martini_restraints import MartiniRestraints, PositionRestraint, PullCoordinate, PullGroup, round_trips
from tests import martini_window_exchange_ref as W

ROOT = Path(__file__).resolve().parent.parent
NEW = {
    "mythos_martini_window_exchange_check": (C.c_int, 8),
    "mythos_martini_langevin_set_window_exchange": (C.c_int, 3),
    "mythos_martini_langevin_set_windows": (C.c_int, 2),
    "mythos_martini_langevin_get_windows": (C.c_int, 2),
    "mythos_martini_langevin_last_windows": (C.c_int, 3),
    "mythos_martini_langevin_last_window_exchanges": (C.c_int, 3),
    "mythos_martini_langevin_window_exchange_counts": (C.c_int, 3),
}


def _need_library():
    if not _lib.lib_path().exists():
        pytest.skip("libmythos_hip.so not built")


# ---- 1: the NumPy reference ---------------------------------------------------------------------------------------------
def test_the_rule_restated_in_numpy():
    """Hand values: the uniform's stream, d's sign on two harmonic windows, a whole event, cross energies with the
    parameter row chosen apart from the configuration, and the row permutation."""
    from tests import martini_exchange_ref as X

    assert W.STREAM == 6 and 0.0 < W.uniform(99, 0, 4) < 1.0 and W.uniform(99, 0, 4) != X.uniform(99, 0, 4)
    assert W.uniform(99, 2, 4) * 2.0 ** 32 % 1.0 == 0.5 and W.uniform(99, 1, 4) != W.uniform(99, 1, 8) != W.uniform(98, 1, 8)
    # windows at 0 and 1, k = 2, kT = 1: x_A = 1 sits in window t's wrong place, x_B = 0 in window t + 1's -> d = +2
    assert W.delta(1.0, 1.0, 0.0, 0.0, 1.0) == 2.0 and W.delta(1.0, 0.0, 1.0, 1.0, 0.0) == -2.0 and W.delta(0.5, 1.0, 0.0, 0.0, 1.0) == 4.0
    assert W.delta(2.5, 3.0, 3.0, 7.0, 7.0) == 0.0
    # one coordinate from the origin to bead 0 along z; per-replica init and k; a position restraint with a per-replica reference
    rs = MartiniRestraints(position=[PositionRestraint(index=1, k=(100.0, 0.0, 0.0))],
                           pulls=[PullCoordinate(group_a=None, group_b=PullGroup(members=(0,)), geometry="direction", vec=(0, 0, 1),
                                                 k=(2.0, 4.0, 2.0), init=(0.0, 1.0, 2.0), rate=0.5, periodic=False)])
    m = np.array([72.0, 72.0])
    x = np.array([[[0.0, 0.0, 1.0], [0.1, 0.0, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[0.0, 0.0, 2.0], [0.3, 0.0, 0.0]]])
    ref = np.zeros((3, 2, 3))
    ref[:, 1, 0] = [0.0, 0.1, 0.3]
    e = lambda s, w, step=0: W.cross_energy(rs, x[s], m, None, step, 0.01, w, ref)  # noqa: E731
    assert e(0, 0) == pytest.approx(0.5 * 2.0 * 1.0 + 0.5 * 100.0 * 0.01) and e(0, 1) == pytest.approx(0.0)
    assert e(1, 0) == pytest.approx(0.0) and e(1, 1) == pytest.approx(0.5 * 4.0 * 1.0 + 0.5 * 100.0 * 0.01)
    assert e(0, 0, step=200) == pytest.approx(0.5 * 100.0 * 0.01)  # the window has moved to xi = 1 at t = 2
    new, recs = W.decide([1, 0, 2], 1.0, lambda s, w: e(s, w, 8), step=8, every=4, seed=1)  # attempt 2: pair (0, 1); slot 1 holds window 0
    assert len(recs) == 1 and recs[0]["slot_a"] == 1 and recs[0]["slot_b"] == 0 and recs[0]["rung"] == 0
    assert recs[0]["d"] == pytest.approx(-(e(1, 1, 8) + e(0, 0, 8) - e(1, 0, 8) - e(0, 1, 8))) and recs[0]["d"] < 0
    assert new.tolist() == ([0, 1, 2] if recs[0]["accepted"] else [1, 0, 2]) and recs[0]["accepted"] == W.accepts(recs[0]["d"], recs[0]["u"])
    assert [r["rung"] for r in W.decide([0, 1, 2], 1.0, e, step=4, every=4, seed=1)[1]] == [1]
    rows = np.arange(12.0).reshape(3, 2, 2)
    assert np.array_equal(W.permute_rows(rows, [2, 0, 1]), rows[[2, 0, 1]])
    a = rs.lower(n_rep=3, reference_pos=ref)
    b = W.lowered_for(a, [2, 0, 1])
    assert np.array_equal(b["p_param"][:, 0, 1], [2.0, 0.0, 1.0]) and np.array_equal(b["pr_ref"][:, 0, 0], [0.3, 0.0, 0.1])
    assert b["p_groups"] is a["p_groups"]


def test_round_trips_on_hand_written_histories():
    up_down = [0, 1, 2, 1, 0]
    cases = {
        "none": ([1, 1, 2, 2, 1, 1], 0),
        "never at the bottom": ([2, 1, 2, 1], 0),
        "one": (up_down, 1),
        "one, starting in the middle": ([1, 2] + up_down, 1),
        "two": (up_down + up_down[1:], 2),
        "cut off at the end": (up_down + [1, 2, 1], 1),
        "half a trip": ([0, 1, 2], 0),
        "bouncing at the bottom": ([0, 1, 0, 1, 0, 1, 2, 1, 0], 1),
    }
    for name, (hist, want) in cases.items():
        col = np.array(hist)
        rows = np.stack([col, (col + 1) % 3, (col + 2) % 3], axis=1)  # three slots; the first is the one under test
        assert round_trips(rows)[0] == want, name
        assert np.array_equal(round_trips(rows), W.round_trips(rows)), name
    rng = np.random.default_rng(5)
    walk = np.clip(np.cumsum(rng.integers(-1, 2, size=(400, 4)), axis=0) % 5, 0, 4)
    assert np.array_equal(round_trips(walk), W.round_trips(walk)) and round_trips(walk).sum() > 0
    assert round_trips(np.zeros((5, 1), dtype=int)).tolist() == [0]
    with pytest.raises(ValueError, match=r"\(rows, R\)"):
        round_trips(np.zeros(5))


# ---- 2: the rule keeps the windows' distributions -----------------------------------------------------------------------
def _toy(sign=1.0, n=400_000, seed=2026):
    """kT = 2.5, k = 500, windows at 0.5 and 0.57: x_A, x_B drawn exactly from their windows' Gaussians, the rule applied once;
    -> (acceptance fraction, the configurations left in window t)."""
    kT, k, c = 2.5, 500.0, (0.5, 0.57)
    sigma = math.sqrt(kT / k)
    rng = np.random.default_rng(seed)
    x_a, x_b, u = rng.normal(c[0], sigma, n), rng.normal(c[1], sigma, n), rng.uniform(size=n)
    e = lambda x, w: 0.5 * k * (x - c[w]) ** 2  # noqa: E731
    d = sign * W.delta(kT, e(x_a, 0), e(x_a, 1), e(x_b, 0), e(x_b, 1))
    acc = (d >= 0.0) | (u < np.exp(np.minimum(d, 0.0)))
    assert all(bool(acc[j]) == W.accepts(d[j], u[j]) for j in range(0, n, 997))  # the vectorised rule is the rule
    return acc.mean(), np.where(acc, x_b, x_a), sigma, c


def test_the_rule_keeps_the_windows_distributions():
    """Exact sampling: the acceptance fraction against erfc(Delta / 2 sigma) = 0.4839 and the mean and variance of what is
    left in window t, each within 4 standard errors (observed when written: 0.48411 accepted, mean - init +0.8e-4 nm with a
    standard error of 1.1e-4; with the sign of d reversed the mean moves by 0.08 nm - the next test)."""
    n = 400_000
    frac, left, sigma, c = _toy()
    want = math.erfc((c[1] - c[0]) / (2.0 * sigma))
    se_p = math.sqrt(want * (1.0 - want) / n)
    dev = left - c[0]
    se_m, se_v = sigma / math.sqrt(n), sigma**2 * math.sqrt(2.0 / n)
    print(f"  accepted {frac:.5f} (erfc {want:.5f}, se {se_p:.1e}); mean - init {dev.mean():+.2e} (se {se_m:.1e}); variance {(dev**2).mean():.5e} "
          f"(kT / k {sigma**2:.5e}, se {se_v:.1e})")
    assert abs(want - 0.4839) < 1e-4
    assert abs(frac - want) <= 4 * se_p
    assert abs(dev.mean()) <= 4 * se_m and abs((dev**2).mean() - sigma**2) <= 4 * se_v


def test_a_reversed_sign_of_d_cannot_pass():
    _, left, sigma, c = _toy(sign=-1.0)
    shift = left.mean() - c[0]
    print(f"  d reversed: the mean of window t moves by {shift:+.4f} nm")
    assert abs(shift) > 100 * sigma / math.sqrt(400_000)


# ---- 3: refusals through the check entry, without a device --------------------------------------------------------------
def _ens():
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    return MartiniEnsembleIntegrator


def _p_param(n_rep=3, n_pull=2):
    q = np.zeros((n_rep, n_pull, 9))
    q[:, :, 0], q[:, :, 1], q[:, :, 2] = 500.0, 0.5 + 0.07 * np.arange(n_rep)[:, None], 1e-3 * np.arange(n_rep)[:, None]
    q[:, :, 3:6], q[:, :, 6:9] = (0.0, 0.0, 1.0), (0.1, 0.2, 0.3)
    return q


def test_entry_points_exist_with_their_prototypes():
    _need_library()
    lib = _lib.load()
    for name, (res, n_args) in NEW.items():
        assert name in _lib.DECLARED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes is not None and len(fn.argtypes) == n_args, name
    header = (ROOT / "include" / "mythos_hip.h").read_text()
    for name in NEW:
        assert f"int {name}(" in header, name


def test_what_passes():
    _need_library()
    E = _ens()
    E.check_window_exchange(2)
    E.check_window_exchange(64, 100, kT=[2.5] * 64)
    E.check_window_exchange(3, 10, kT=[2.5] * 3, p_param=_p_param(), window_of_slot=[2, 0, 1])
    E.check_window_exchange(3, 0, kT=[2.5] * 3, temperature_exchange=True, barostat=True)  # off: nothing to clash with


def test_every_refusal_by_name():
    _need_library()
    E = _ens()
    for n_rep in (1, 0):
        with pytest.raises(ValueError, match=r"window exchange needs an ensemble handle with at least two replicas \(n_rep >= 2\)"):
            E.check_window_exchange(n_rep, 4)
    with pytest.raises(ValueError, match=r"window exchange every >= 0 required \(0 switches window exchange off\)"):
        E.check_window_exchange(3, -1)
    with pytest.raises(ValueError, match=r"every replica at the same kT \(replica 1 has 2\.6"):
        E.check_window_exchange(3, 10, kT=[2.5, 2.6, 2.5])
    with pytest.raises(ValueError, match="window exchange together with temperature replica exchange is refused"):
        E.check_window_exchange(3, 10, kT=[2.5] * 3, temperature_exchange=True)
    with pytest.raises(ValueError, match="window exchange together with a barostat is refused"):
        E.check_window_exchange(3, 10, kT=[2.5] * 3, barostat=True)
    q = _p_param()
    q[2, 1, 4] = 0.5
    with pytest.raises(ValueError, match=r"pull coordinate 1: window exchange needs the same vec in every replica \(replica 2 differs\)"):
        E.check_window_exchange(3, 10, p_param=q)
    q = _p_param()
    q[1, 0, 6] = 0.11
    with pytest.raises(ValueError, match=r"pull coordinate 0: window exchange needs the same origin in every replica \(replica 1 differs\)"):
        E.check_window_exchange(3, 10, p_param=q)
    for bad in ([0, 1, 1], [0, 1, 3], [0, -1, 2]):
        with pytest.raises(ValueError, match=r"window_of_slot must be a permutation of 0 \.\. 2"):
            E.check_window_exchange(3, 10, window_of_slot=bad)
    with pytest.raises(ValueError, match="must hold 3 values"):
        E.check_window_exchange(3, 10, window_of_slot=[0, 1])


def test_null_handles_are_refused_by_name():
    _need_library()
    lib = _lib.load()
    n = C.c_int(0)
    assert lib.mythos_martini_langevin_set_window_exchange(None, 4, 0) == -1 and "set_window_exchange" in _lib.last_error()
    assert lib.mythos_martini_langevin_set_windows(None, None) == -1 and "set_windows" in _lib.last_error()
    assert lib.mythos_martini_langevin_get_windows(None, None) == -1 and "get_windows" in _lib.last_error()
    assert lib.mythos_martini_langevin_last_windows(None, None, C.byref(n)) == -1 and "last_windows" in _lib.last_error()
    assert lib.mythos_martini_langevin_last_window_exchanges(None, None, C.byref(n)) == -1 and "last_window_exchanges" in _lib.last_error()
    assert lib.mythos_martini_langevin_window_exchange_counts(None, None, None) == -1 and "window_exchange_counts" in _lib.last_error()


def test_simulator_arguments():
    """HipMartiniSimulator(window_exchange_every=...) builds without a device and refuses the bad combinations by name."""
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator
    from tests.test_martini_ensemble_cpu import _sim_kwargs

    kw = dict(_sim_kwargs(), temperatures=[300.0] * 3)
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=(0, 1)), group_b=PullGroup(members=(2, 3)), geometry="distance",
                                                 dim=(False, False, True), k=500.0, init=(0.5, 0.57, 0.64), periodic=False)])
    assert HipMartiniSimulator(**kw).window_exchange_every == 0
    assert HipMartiniSimulator(**dict(kw, restraints=rs)).window_exchange_every == 0
    assert HipMartiniSimulator(**dict(kw, restraints=rs, window_exchange_every=10)).window_exchange_every == 10
    for bad in (dict(restraints=rs, window_exchange_every=-1), dict(window_exchange_every=10),
                dict(restraints=rs, window_exchange_every=10, temperatures=[300.0])):
        with pytest.raises(ValueError, match="window_exchange_every >= 0, and restraints with at least two windows"):
            HipMartiniSimulator(**dict(kw, **bad))
    with pytest.raises(ValueError, match="window_exchange_every together with exchange_every is refused"):
        HipMartiniSimulator(**dict(kw, restraints=rs, window_exchange_every=10, exchange_every=10))
    with pytest.raises(ValueError, match="window_exchange_every together with a barostat is refused"):
        HipMartiniSimulator(**dict(kw, restraints=rs, window_exchange_every=10, barostat=dict(kind="berendsen", compressibility=4.5e-5)))
    with pytest.raises(ValueError, match="restraints together with a barostat or replica exchange"):  # (without window exchange: as ever)
        HipMartiniSimulator(**dict(kw, restraints=rs, exchange_every=10))
    with pytest.raises(ValueError, match="window_exchange_every needs every replica at the same temperature"):
        HipMartiniSimulator(**dict(kw, restraints=rs, window_exchange_every=10, temperatures=[300.0, 300.0, 310.0]))


# ---- 4: the host program under the sanitizers ---------------------------------------------------------------------------
def test_host_logic_under_the_host_sanitizers(tmp_path):
    """tests/host/martini_window_exchange_main.cpp - a stand-alone program with its own main over
    martini_window_exchange_checks.h - built with -fsanitize=address,undefined and run: the decision's sign, every refusal,
    the permutation check, and the row plan from every assignment to every other for R = 2 .. 5 (15 016 plans).  Exit code
    0, nothing reported."""
    exe = tmp_path / "martini_window_exchange_san"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-I", str(ROOT / "mythos_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "martini_window_exchange_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.splitlines()[-1] == "ok (15016 plans)" and run.stderr == "", (run.stdout, run.stderr)
