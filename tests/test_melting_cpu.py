"""Melting temperature without a GPU: the host functions against numpy, the fixture, the kT helpers of flat_params against
``derive_flat`` at each temperature, and the host algebra of the observable on oracle energies."""

import gzip

import numpy as np
import pytest
import torch

from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults, oxdna_energy
from mythos_amd.observables import melting_temp as MT
from mythos_amd.utils.units import get_kt_from_c
from tests import helpers as H
from tests import melting_ref as M


def _sigmoid_curve(n=20, mid=0.1003, width=0.0021):
    kts = np.linspace(0.093, 0.117, n)
    return kts, 1.0 / (1.0 + np.exp((kts - mid) / width))


def test_host_functions_against_numpy():
    ratio = np.array([0.03, 0.5, 1.0, 7.0, 400.0])
    np.testing.assert_allclose(MT.compute_finf(ratio).numpy(), 1 + 1 / (2 * ratio) - np.sqrt((1 + 1 / (2 * ratio)) ** 2 - 1), rtol=1e-15)
    # interp1d sorts by x: the same points in any order, inside and beyond both ends
    rng = np.random.default_rng(3)
    x = np.array([0.3, -1.0, 2.5, 0.9, 1.7])
    y = rng.normal(size=5)
    at = np.array([-3.0, -1.0, -0.2, 0.3, 0.31, 1.0, 2.49, 2.5, 9.0])
    order = np.argsort(x)
    want = np.interp(at, x[order], y[order])
    for perm in (np.arange(5), order, order[::-1], rng.permutation(5)):
        np.testing.assert_allclose(MT.interp1d(x[perm], y[perm], at).numpy(), want, rtol=0, atol=1e-15)
    assert float(MT.interp1d(x, y, 0.9)) == y[3]
    # a melting curve decreases with temperature: the interpolation runs over the ratios as x
    kts, curve = _sigmoid_curve()
    rev = np.argsort(curve)
    assert abs(float(MT.find_melting_temp(kts, curve)) - np.interp(0.5, curve[rev], kts[rev])) < 1e-15
    assert abs(float(MT.find_melting_temp(kts, curve)) - 0.1003) < 2e-5  # the sigmoid's midpoint, to the chord error
    width = np.interp(0.8, curve[rev], kts[rev]) - np.interp(0.2, curve[rev], kts[rev])
    assert abs(float(MT.compute_curve_width(kts, curve)) - width) < 1e-15 and width < 0
    # a curve that never reaches 0.5 pins to the edge of the range
    assert float(MT.find_melting_temp(kts, 0.5 + 0.4 * curve)) == kts[-1]
    assert MT.TARGETS == {"SL_avg_6bp": get_kt_from_c(31.2), "SL_avg_8bp": get_kt_from_c(48.2), "SL_avg_12bp": get_kt_from_c(64.7)}


def test_interp1d_is_differentiable_in_the_curve():
    kts, curve = _sigmoid_curve()
    r = torch.tensor(curve, requires_grad=True)
    tm = MT.find_melting_temp(kts, r)
    (g,) = torch.autograd.grad(tm, r)
    k = int(np.nonzero(g.numpy())[0][0])
    assert np.count_nonzero(g.numpy()) == 2 and curve[k] > 0.5 > curve[k + 1]
    h = 1e-7
    up, dn = curve.copy(), curve.copy()
    up[k] += h
    dn[k] -= h
    fd = (float(MT.find_melting_temp(kts, up)) - float(MT.find_melting_temp(kts, dn))) / (2 * h)
    assert abs(float(g[k]) - fd) < 1e-7 * abs(fd)


def test_fixture_integrity():
    top, traj, en = M.load_run()
    assert top.n_nucleotides == 12 and traj.center.shape == (384, 12, 3) and np.allclose(traj.box_size, 20.0)
    assert list(en) == ["time", "potential_energy", "acc_ratio_trans", "acc_ratio_rot", "acc_ratio_vol", "bond", "mindistance", "weight"]
    assert all(v.shape == (384,) for v in en.values())
    assert en["time"][0] == 10000 and en["time"][1] == 20000  # step 0 dropped: row k is configuration k
    assert int((en["bond"] == 0).sum()) == 229 and (en["weight"] > 0).all()
    inputs = oxdna_energy.read_input(M.FIXTURE / "input")
    assert inputs["T"] == "307.15K" and inputs["umbrella_sampling"] == "1" and inputs["op_file"] == "op.txt"
    assert oxdna_energy.order_parameter_names(M.FIXTURE / "op.txt") == ["bond", "mindistance"]
    # (that the trimmed files are prefixes of the reference's: tests/golden/copy_melting_fixtures.py --check, where it exists)
    assert (M.FIXTURE / "sys.top").read_text().splitlines()[0].split() == ["12", "2"]
    assert len(gzip.decompress((M.FIXTURE / "trajectory.dat.gz").read_bytes()).splitlines()) == 5760
    assert len((M.FIXTURE / "energy.dat").read_text().splitlines()) == 385
    assert max(f.stat().st_size for f in M.FIXTURE.iterdir()) < 1 << 20


def test_read_energy_without_umbrella_sampling(tmp_path):
    (tmp_path / "input").write_text("# a plain run\nenergy_file = e.dat\numbrella_sampling = 0\n")
    (tmp_path / "e.dat").write_text("0 -1.0 0.1 0.2 0.0\n10 -1.5 0.1 0.2 0.0\n20 -1.25 0.1 0.2 0.0\n")
    en = oxdna_energy.read_energy(tmp_path)
    assert list(en) == list(oxdna_energy.BASE_COLUMNS) and en["potential_energy"].tolist() == [-1.5, -1.25]
    (tmp_path / "input").write_text("energy_file = e.dat\numbrella_sampling = 1\nop_file = op.txt\n")
    (tmp_path / "op.txt").write_text("{\norder_parameter = bond\nname = x\n}\n")
    with pytest.raises(ValueError, match="columns"):
        oxdna_energy.read_energy(tmp_path)


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("ss", [False, True])
def test_kt_helpers_equal_derive_flat_at_each_temperature(model, ss):
    """rho_t and the Debye table are the expressions ``derive_flat`` itself evaluates: exact equality, with numbers and
    through the torch graph."""
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    if ss:
        w = np.random.default_rng(model).uniform(0.8, 1.3, (4, 4))
        cfg["stacking"]["ss_stack_weights"] = torch.as_tensor(w)
    kt0, salt = 0.1031, 0.15 if model == 2 else 1.0
    kts = np.array([0.0933, kt0, 0.1, 0.1166, 1e-4])
    rho, table = fp.kt_sweep_tables(model, cfg, kts, kt=kt0, salt_conc=salt)
    eps_g, table_g = fp.kt_sweep_tables(model, cfg, torch.as_tensor(kts), kt=kt0, salt_conc=salt, graph=True)
    base = fp.derive_flat(model, cfg, kt=kt0, salt_conc=salt)
    assert rho[1] == 1.0 and (table is None) == (model == 1)
    for t, kt in enumerate(kts):
        for numbers in (False, True):
            named = fp.derive_flat(model, cfg, kt=kt, salt_conc=salt, numbers_ok=numbers)
            for i in range(4):
                for j in range(4):
                    assert float(named[f"STCK_EPS_{i}{j}"]) == float(eps_g[t, 4 * i + j])
            # rho is the ratio of the scalar factors; the table entries carry one more rounding each (factor x weight): four roundings between the two sides
            ratio = float(named["STCK_EPS_03"]) / float(base["STCK_EPS_03"])
            assert ratio == rho[t] if not ss else abs(ratio - rho[t]) <= 4 * np.spacing(abs(rho[t]))
            if model != 1:
                assert [float(named[n]) for n in fp.DEBYE_KT_NAMES] == table[t].tolist() == table_g[t].tolist()


def test_kt_helpers_carry_the_graph_of_derive_flat():
    """d(eps_stack(kT_t))/d(theta) and d(Debye constants(kT_t))/d(theta) through the batched helpers equal those of
    ``derive_flat`` at that temperature."""
    kts = torch.tensor([0.0933, 0.1166], dtype=torch.float64)
    for t in range(2):
        grads = []
        for batched in (True, False):
            _, cfg, leaves = M.oracle_cfg(2, leaves=True)
            if batched:
                eps, table = fp.kt_sweep_tables(2, cfg, kts, kt=0.1, salt_conc=0.5, graph=True)
                out = eps[t].sum() + (table[t] * torch.arange(1.0, 6.0, dtype=torch.float64)).sum()
            else:
                named = fp.derive_flat(2, cfg, kt=kts[t], salt_conc=0.5)
                out = sum(named[f"STCK_EPS_{i}{j}"] for i in range(4) for j in range(4)) + sum(
                    (k + 1.0) * named[n] for k, n in enumerate(fp.DEBYE_KT_NAMES))
            keys = [("stacking", "eps_stack_base"), ("stacking", "eps_stack_kt_coeff"), ("debye", "q_eff"), ("debye", "lambda_factor"),
                    ("debye", "prefactor_coeff")]
            grads.append([float(g) for g in torch.autograd.grad(out, [leaves[k] for k in keys])])
        np.testing.assert_allclose(grads[0], grads[1], rtol=1e-14)
        assert all(g != 0.0 for g in grads[0])


def test_melting_temperature_from_oracle_energies():
    ref = M.fixture_reference()
    ratios = MT.extrapolated_ratios(ref["e0"], ref["et"], M.KT_SIM, ref["kts"], ref["bind"], ref["weights"])
    assert (np.diff(ratios.numpy()) < 0).all()  # strictly decreasing
    np.testing.assert_allclose(ratios.numpy(), ref["ratios"], rtol=1e-12)
    tm = float(MT.find_melting_temp(ref["kts"], ratios))
    assert abs(tm - ref["tm"]) <= 1e-8 and abs(tm - 0.10144342) <= 1e-8
    assert ref["kts"][0] < tm < ref["kts"][-1]
    assert abs(float(MT.compute_curve_width(ref["kts"], ratios)) - ref["width"]) <= 1e-10


@pytest.mark.skipif(not M.REFERENCE_RUN.exists(), reason="the reference's full 1000-frame run is not on this machine")
def test_full_run_reproduces_the_references_own_number():
    """mythos/observables/tests/test_melting_temp.py asserts isclose(Tm, 0.1009298) on all 1000 configurations."""
    ref = M.fixture_reference(str(M.REFERENCE_RUN))
    assert ref["et"].shape == (20, 1000)
    ratios = MT.extrapolated_ratios(ref["e0"], ref["et"], M.KT_SIM, ref["kts"], ref["bind"], ref["weights"])
    assert np.isclose(float(MT.find_melting_temp(ref["kts"], ratios)), 0.1009298)
    assert np.isclose(ref["tm"], 0.1009298)
