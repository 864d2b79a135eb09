"""Replica exchange between the temperatures of the MARTINI ensemble, checked without a device: the host logic of
mythos_amd/csrc/martini_exchange_checks.h under the host sanitizers, the new entry points, and the refusals that need no
handle (mythos_martini_exchange_check), raised with the library's message."""

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.hip_system import MartiniEnsembleIntegrator as Ens

ROOT = Path(__file__).resolve().parent.parent
NEW = {
    "mythos_martini_langevin_set_exchange": (C.c_int, 3),
    "mythos_martini_langevin_set_ladder": (C.c_int, 2),
    "mythos_martini_langevin_get_ladder": (C.c_int, 2),
    "mythos_martini_langevin_last_ladder": (C.c_int, 3),
    "mythos_martini_langevin_last_exchanges": (C.c_int, 3),
    "mythos_martini_langevin_exchange_counts": (C.c_int, 3),
    "mythos_martini_exchange_check": (C.c_int, 3),
}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("exchange") / "martini_exchange_san"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-I", str(ROOT / "mythos_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "martini_exchange_main.cpp"), "-o", str(exe)], check=True)
    return exe


def test_host_logic_and_detailed_balance_under_the_host_sanitizers(host_program):
    """tests/host/martini_exchange_main.cpp - a stand-alone program with its own main over martini_exchange_checks.h - built
    with -fsanitize=address,undefined and run: the pair schedule for R = 2 .. 5, the two-event chunks against a step loop for
    (coupling every, exchange every, save_every) = (3, 6, 3), (4, 6, 5), (0, 4, 0), (3, 4, 1) as one call and split, the
    permutation check, the reference pressure, every refusal, and detailed balance through the real mm_xchg_accept: four
    rungs kT = 1, 1.3, 1.7, 2.2, U = kT Gamma(15, 1) drawn afresh per attempt, 200 000 attempts, every rung's mean U within 4
    standard errors of 15 kT_t and every slot on every rung.  Exit code 0, nothing reported.
    Observed when written: 142 519 of 300 000 pair attempts accepted, the worst rung mean 1.59 standard errors off.  With the
    sign of d flipped the same chain accepted 266 323 and the worst rung mean was 294 standard errors off - the next test."""
    run = subprocess.run([str(host_program)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.splitlines()[-1].startswith("ok") and run.stderr == "", (run.stdout, run.stderr)
    assert "detailed balance:" in run.stdout


def test_the_detailed_balance_check_fails_when_the_sign_of_d_is_flipped(host_program):
    """The same program with "flip": d is negated before mm_xchg_accept sees it, and the rung means must leave their
    4 standard errors by a wide margin (hundreds, see above) - the check can tell a wrong rule from the right one."""
    run = subprocess.run([str(host_program), "flip"], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 1 and "worst < 4.0" in run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("detailed balance (d flipped)")][0]
    assert float(line.split("worst rung mean")[1].split()[0]) > 100.0


def test_entry_points_exist_with_their_prototypes():
    lib = _lib.load()
    for name, (res, n_args) in NEW.items():
        assert name in _lib.DECLARED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes is not None and len(fn.argtypes) == n_args, name


def test_what_passes():
    Ens.check_exchange(2)
    Ens.check_exchange(8, 100)
    Ens.check_exchange(4, 0, [0, 1, 2, 3])
    Ens.check_exchange(4, 4, [3, 0, 2, 1])


@pytest.mark.parametrize("n_rep", [1, 0])
def test_a_single_copy_is_refused(n_rep):
    with pytest.raises(ValueError, match=r"replica exchange needs an ensemble handle with at least two replicas \(n_rep >= 2\)"):
        Ens.check_exchange(n_rep, 4)


def test_a_negative_every_is_refused():
    with pytest.raises(ValueError, match=r"exchange every >= 0 required \(0 switches exchange off\)"):
        Ens.check_exchange(3, -1)


@pytest.mark.parametrize("ladder", [[0, 1, 1, 3], [0, 1, 2, 4], [0, -1, 2, 3], [1, 2, 3, 4]])
def test_a_ladder_that_is_no_permutation_is_refused(ladder):
    with pytest.raises(ValueError, match=r"rung_of_slot must be a permutation of 0 \.\. 3"):
        Ens.check_exchange(4, 4, ladder)
    with pytest.raises(ValueError, match="must hold 4 values"):
        Ens.check_exchange(4, 4, ladder[:3])


def test_null_handles_are_refused_by_name():
    lib = _lib.load()
    n = C.c_int(0)
    assert lib.mythos_martini_langevin_set_exchange(None, 4, 0) == -1 and "set_exchange" in _lib.last_error()
    assert lib.mythos_martini_langevin_set_ladder(None, None) == -1 and "set_ladder" in _lib.last_error()
    assert lib.mythos_martini_langevin_get_ladder(None, None) == -1 and "get_ladder" in _lib.last_error()
    assert lib.mythos_martini_langevin_last_ladder(None, None, C.byref(n)) == -1 and "last_ladder" in _lib.last_error()
    assert lib.mythos_martini_langevin_last_exchanges(None, None, C.byref(n)) == -1 and "last_exchanges" in _lib.last_error()
    assert lib.mythos_martini_langevin_exchange_counts(None, None, None) == -1 and "exchange_counts" in _lib.last_error()


def test_the_rule_restated_in_numpy():
    """tests/martini_exchange_ref.py against hand values: the schedule, U's order of addition, d with and without p V, the
    rule's two branches, the factor's single rounding, and a whole event."""
    from tests import martini_exchange_ref as X

    assert [X.schedule(r, a) for r, a in ((2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2))] == \
        [[], [0], [1], [0], [1], [0, 2], [1, 3], [0, 2]]
    assert 0.0 < X.uniform(99, 0, 4) < 1.0 and X.uniform(99, 0, 4) != X.uniform(99, 1, 4) != X.uniform(99, 1, 8) != X.uniform(98, 1, 8)
    assert X.uniform(99, 2, 4) * 2.0 ** 32 % 1.0 == 0.5
    assert X.potential([0.1, 0.2, 0.3, 99.0]) == (0.1 + 0.2) + 0.3 and X.potential([0.1, 0.2, 0.3, 99.0, 0.7]) == ((0.1 + 0.2) + 0.3) + 0.7
    assert X.delta(1.0, 2.0, 5.0, 0.0, 3.0, 0.0) == 1.0 and X.delta(1.0, 2.0, 3.0, 10.0, 3.0, 6.0, 0.5) == 1.0
    assert X.accepts(0.0, 0.99) and X.accepts(-1.0, 0.36) and not X.accepts(-1.0, 0.37)
    assert X.factor(1.0, 4.0) == 2.0 and X.factor(2.0, 2.5, np.float32) == np.float32(np.sqrt(1.25))
    assert X.pressure_term(None) == 0.0
    assert X.pressure_term(dict(coupling="semiisotropic", ref_p=(1.0, 2.0), compressibility=(0.0, 1e-5))) == 2.0 / 16.6053907
    kTs = np.array([1.0, 2.0, 3.0])
    e = np.array([[5.0, 0, 0, 0], [0.0, 0, 0, 0], [3.0, 0, 0, 0]])  # slot 0 (rung 0) above slot 2 (rung 1): d > 0
    new, recs, fac = X.decide([0, 2, 1], kTs, e, np.ones((3, 3)), step=8, every=4, seed=1)
    assert new.tolist() == [1, 2, 0] and len(recs) == 1 and recs[0]["slot_a"] == 0 and recs[0]["slot_b"] == 2 and recs[0]["d"] == 1.0
    assert fac.tolist() == [np.sqrt(2.0), 1.0, np.sqrt(0.5)]


def test_simulator_arguments():
    """HipMartiniSimulator(exchange_every=...) builds without a device; a negative cadence, or exchange with one temperature,
    is refused."""
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator
    from tests.test_martini_ensemble_cpu import _sim_kwargs

    kw = _sim_kwargs()
    assert HipMartiniSimulator(**kw).exchange_every == 0
    assert HipMartiniSimulator(**dict(kw, exchange_every=10)).exchange_every == 10
    HipMartiniSimulator(**dict(kw, temperatures=300.0, exchange_every=0))
    for bad in (dict(exchange_every=-1), dict(exchange_every=10, temperatures=300.0)):
        with pytest.raises(ValueError, match="exchange_every >= 0, and at least two temperatures"):
            HipMartiniSimulator(**dict(kw, **bad))
