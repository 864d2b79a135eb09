"""GPU tests of the MARTINI integrators' external forces (mythos_martini_langevin_set_restraints, csrc/martini_restraints.h):
position restraints, flat-bottomed restraints and pull coordinates between centres of mass.

The reference is tests/martini_restraints_ref.py (NumPy, float64, checked against central differences of its own energy by
tests/test_martini_restraints_cpu.py); the sets and systems are those of tests/martini_restraints_cases.py, whose shapes -
boxes against cut-off + skin, minimum images clear of their flip - are checked there on the CPU.

  1  field and energies against the reference: 0, 1 and 257 restrained beads (771 in three replicas: four workgroups of the
     kick), groups of 1, 2, 3 and 257 members, fp64 and fp32, step counts 0 and 12 345
  2  pull_values on a stored trajectory: the reference's xi, and bit for bit the xi external_field reports
  3  six steps against the oracle with the reference field added: the 257-bead system with every term kind, and free beads
     with gamma = 0
  4  free beads under an umbrella: 64 replicas, eight windows, mean and variance of xi per window
  5  bitwise: advance(a); advance(b) = advance(a + b) with a moving reference; ensemble replica r = the single integrator
     with replica r's set; a cleared set = an integrator that never had one, launch counts included
  6  a thin skin with k = 10^6 restraints: recoveries happen and the state still matches the oracle
  7  NVE: the drift of U + K + U_ext against the drift of U + K without restraints
  8  refusals through the handle: barostat and exchange, in either order
  9  the bilayer through HipMartiniSimulator: an umbrella on the distance between the leaflets' PO4 centres of mass
"""

import dataclasses as dc
import functools

import numpy as np
import pytest
import torch

from mythos_amd.simulators.martini_restraints import (FlatBottomRestraint, MartiniRestraints, PositionRestraint, PullCoordinate,
                                                       PullGroup)
from tests import martini_restraints_cases as CS
from tests import martini_restraints_ref as REF

pytestmark = pytest.mark.gpu

KB = 0.0083144626
KT = KB * 273.0
SEEDS = [0xABCDEF012345, 7, 2**63 + 11]
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
EPS64 = 2.0**-53


def _ff(s):
    return tuple(s[k] for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0"))


def _system(ff, dtype):
    from mythos_amd.hip_system import MartiniSystem

    return MartiniSystem(*ff, angle_kind=0, dtype=dtype)


def _dev(x, sysm):
    return torch.tensor(np.asarray(x), dtype=sysm.dtype, device=sysm.device).contiguous()


def _rounded(x, dtype):
    """x as the device holds it, widened back to float64"""
    return np.asarray(x, dtype=np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)


def of_replica(rs, r):
    """The set a single integrator carries for replica r: per-replica init and k made scalars."""
    pick = lambda v: float(np.asarray(v, dtype=np.float64).reshape(-1)[r if np.ndim(v) else 0])  # noqa: E731
    return dc.replace(rs, pulls=[dc.replace(c, init=pick(c.init), k=pick(c.k)) for c in rs.pulls])


def static(rs):
    return dc.replace(rs, pulls=[dc.replace(c, rate=0.0) for c in rs.pulls])


def _single(sysm, mass, kT=KT, gamma=2.0, seed=SEEDS[0], dt=CS.DT, policy=(0.25, 2)):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=dt, kT=kT, gamma=gamma, mass=mass, seed=seed)
    integ.set_neighbor_policy(*policy)
    return integ


def _ensemble(sysm, mass, kTs, gamma=2.0, seeds=SEEDS, dt=CS.DT, policy=(0.25, 2)):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    integ = MartiniEnsembleIntegrator(sysm, dt=dt, kT=kTs, gamma=gamma, mass=mass, seeds=list(seeds[:len(kTs)]))
    integ.set_neighbor_policy(*policy)
    return integ


def _tolerances(rs, x, masses, box, s, rep, ref, dtype):
    """(force, energy, xi) tolerances of one replica.  fp64: 1e-12 of the scale plus the bound of the summation order - a
    centre of mass summed in another order differs by at most n eps sum |m x| / M per axis, which moves xi by at most the
    sqrt(3)-fold of both groups' bounds, U' by |k| times that, U by |U'| times that and a distance's direction by |U'| / xi
    times that; the energy sums over n terms by n eps of their sum.  fp32: the reference is fed the rounded positions and everything
    before the result is double, so the force carries one rounding into fp32, 2^-23 of max |F|, on top."""
    F, e, xi = REF.field(rs, x, masses, box, s, CS.DT, rep, ref)
    f_scale, n = np.abs(F).max() if F.any() else 1.0, x.shape[0]
    d_force, d_energy, d_xi = 0.0, 0.0, 0.0
    for c in rs.pulls:
        d = 0.0
        for g in (c.group_a, c.group_b):
            if g is not None:
                mem = g.indices()
                d += len(mem) * EPS64 * (masses[mem][:, None] * np.abs(x[mem])).sum(0).max() / masses[mem].sum()
        d *= np.sqrt(3.0)
        one = MartiniRestraints(pulls=[c])
        _, _, du, _, _, _ = REF.pull(c, x, masses, box, s * CS.DT, rep)
        xi_c = REF.field(one, x, masses, box, s, CS.DT, rep)[2][0]
        k = abs(float(np.asarray(c.k, dtype=np.float64).reshape(-1)[rep if np.ndim(c.k) else 0]))
        d_force += (k if c.kind == "umbrella" else 0.0) * d + (abs(du) / max(abs(xi_c), 1e-3) * d if c.geometry == "distance" else 0.0)
        d_energy += abs(du) * d
        d_xi = max(d_xi, d)
    tol_f = 1e-12 * f_scale + d_force + (2.0**-23 * f_scale if dtype == torch.float32 else 0.0)
    tol_e = (1e-12 + n * EPS64) * max(1.0, np.abs(e).sum()) + d_energy  # (|dU| <= |U'| d_xi)
    return (F, e, xi), (tol_f, tol_e, 1e-12 * max(1.0, np.abs(xi).max(initial=0.0)) + d_xi)


# ------------------------------------------------------------------------------------------------ 1, 2
@DTYPES
def test_field_and_energies_of_three_replicas_against_the_reference(dtype):
    c, rs = CS.n257(), CS.sets()["full"]
    sysm = _system(_ff(c["s"]), dtype)
    integ = _ensemble(sysm, c["masses"], [KT, 1.1 * KT, 1.2 * KT])
    integ.set_restraints(rs, reference_pos=c["ref"], box=c["boxes"])
    pos = _dev(c["pos"], sysm)
    x = _rounded(c["pos"], dtype)
    for s in (0, 12345):
        force, energies, xi = integ.external_field(pos, step=s)
        assert force.shape == (3, 257, 3) and force.dtype == dtype and energies.shape == (3, 4) and xi.shape == (3, 4)
        for r in range(3):
            (F, e, x_ref), (tf, te, tx) = _tolerances(rs, x[r], c["masses"], c["boxes"][r], s, r, c["ref"][r], dtype)
            df, de, dx = np.abs(force[r].double().cpu().numpy() - F).max(), np.abs(energies[r].cpu().numpy() - e).max(), np.abs(xi[r].cpu().numpy() - x_ref).max()
            print(f"  step {s} replica {r}: max |F| {np.abs(F).max():.3e} |dF| {df:.2e} (tol {tf:.2e})  |dE| {de:.2e} (tol {te:.2e})  |dxi| {dx:.2e} (tol {tx:.2e})")
            assert df <= tf and de <= te and dx <= tx
            assert np.count_nonzero(np.abs(F).sum(1)) >= 256


@DTYPES
@pytest.mark.parametrize("name", ["none", "one", "full"])
def test_field_of_the_single_integrator_with_0_1_and_257_restrained_beads(dtype, name):
    c = CS.n257()
    rs = of_replica(CS.sets()[name], 1)
    sysm = _system(_ff(c["s"]), dtype)
    integ = _single(sysm, c["masses"])
    integ.set_restraints(rs, reference_pos=c["ref"][1], box=c["boxes"][1])
    pos, x = _dev(c["pos"][1], sysm), _rounded(c["pos"][1], dtype)
    force, energies, xi = integ.external_field(pos, step=12345)
    (F, e, x_ref), (tf, te, tx) = _tolerances(rs, x, c["masses"], c["boxes"][1], 12345, 0, c["ref"][1], dtype)
    restrained = int(np.count_nonzero(np.abs(F).sum(1)))
    assert restrained == {"none": 0, "one": 1, "full": 257}[name] and xi.shape == (len(rs.pulls),)
    df, de = np.abs(force.double().cpu().numpy() - F).max(), np.abs(energies.cpu().numpy() - e).max()
    print(f"  {name}: max |F| {np.abs(F).max():.3e} |dF| {df:.2e} (tol {tf:.2e})  |dE| {de:.2e} (tol {te:.2e})")
    assert df <= tf and de <= te
    if len(rs.pulls):
        assert np.abs(xi.cpu().numpy() - x_ref).max() <= tx


@DTYPES
def test_pull_values_of_a_stored_trajectory(dtype):
    c, rs = CS.n257(), CS.sets()["full"]
    sysm = _system(_ff(c["s"]), dtype)
    integ = _ensemble(sysm, c["masses"], [KT, 1.1 * KT, 1.2 * KT])
    integ.set_restraints(rs, reference_pos=c["ref"], box=c["boxes"])
    rows = 5
    traj_h = c["pos"][None] + np.random.default_rng(31).uniform(-0.02, 0.02, size=(rows, *c["pos"].shape))
    traj = _dev(traj_h, sysm)
    xi = integ.pull_values(traj)
    assert xi.shape == (rows, 3, 4) and xi.dtype == torch.float64
    x = _rounded(traj_h, dtype)
    for k in range(rows):
        _, _, xi_field = integ.external_field(traj[k].contiguous(), step=3)
        assert torch.equal(xi_field, xi[k]), k
        for r in range(3):
            (_, _, x_ref), (_, _, tx) = _tolerances(rs, x[k, r], c["masses"], c["boxes"][r], 0, r, c["ref"][r], dtype)
            assert np.abs(xi[k, r].cpu().numpy() - x_ref).max() <= tx, (k, r)
    single = _single(sysm, c["masses"])
    single.set_restraints(of_replica(rs, 2), reference_pos=c["ref"][2], box=c["boxes"][2])
    assert torch.equal(single.pull_values(traj[:, 2].contiguous()), xi[:, 2])


# ------------------------------------------------------------------------------------------------ 3
def _steps_against_oracle(ff, rs, x0, ref, box, mass, n_steps, gamma, kT=KT, seed=SEEDS[0], dt=CS.DT, policy=(0.25, 2), atol=1e-10):
    sysm = _system(ff, torch.float64)
    integ = _single(sysm, mass, kT=kT, gamma=gamma, seed=seed, dt=dt, policy=policy)
    integ.set_restraints(rs, reference_pos=ref, box=box)
    pos, vel = _dev(x0, sysm), None
    vel = integ.init_velocities()
    v0 = vel.cpu().numpy().copy()
    traj, et = integ.run(pos, vel, box, n_steps, save_every=1)
    orc = CS.oracle_with_field(rs, ff, True, box, dt, kT, gamma, mass, seed, ref)
    xo, vo = np.array(x0, dtype=np.float64), v0.copy()
    e_ref = orc.run(xo, vo, n_steps)
    dx, dv = np.abs(pos.cpu().numpy() - xo).max(), np.abs(vel.cpu().numpy() - vo).max()
    print(f"  {n_steps} steps: |dx| {dx:.2e} |dv| {dv:.2e} |dE| {np.abs(et.cpu().numpy() - e_ref).max():.2e}; moved {np.abs(xo - x0).max():.3f} nm, "
          f"recoveries {integ.last_recoveries()}")
    assert dx <= atol and dv <= atol
    np.testing.assert_allclose(et.cpu().numpy(), e_ref, rtol=1e-9, atol=1e-7)
    return traj.cpu().numpy(), integ


def test_six_steps_of_the_257_bead_system_with_every_term_kind_against_the_oracle():
    c = CS.n257()
    rs = of_replica(CS.sets()["full"], 0)
    _steps_against_oracle(_ff(c["s"]), rs, c["pos"][0], c["ref"][0], c["boxes"][0], c["masses"], 6, gamma=2.0)
    # the field matters at this tolerance: without it the oracle is elsewhere
    F = REF.field(rs, c["pos"][0], c["masses"], c["boxes"][0], 0, CS.DT, 0, c["ref"][0])[0]
    assert (0.5 * CS.DT**2 * np.abs(F) / c["masses"][:, None]).max() > 1e-6


def _free_set(f, k_pull=500.0, init=0.8, rate=0.0):
    """Free beads: position restraints on beads 0 - 2, a layer wall on bead 3, and a direction umbrella between two groups of
    five (beads 4 - 8 and 9 - 13), not periodic; beads 14 and 15 stay free."""
    x = f["pos"]
    return MartiniRestraints(
        position=[PositionRestraint(index=i, k=(900.0, 400.0 * i, 250.0), reference=tuple(x[i] + 0.05)) for i in range(3)],
        flat_bottom=[FlatBottomRestraint(index=3, shape="layer", axis="z", r=0.01, k=600.0, reference=tuple(x[3] + [0, 0, 0.1]))],
        pulls=[PullCoordinate(group_a=PullGroup(members=tuple(range(4, 9))), group_b=PullGroup(members=tuple(range(9, 14))), geometry="direction",
                              vec=(0.0, 0.0, 1.0), k=k_pull, init=init, rate=rate, periodic=False)])


def test_six_steps_of_free_beads_without_friction_are_the_closed_form_recurrence():
    f = CS.free_beads(16)
    rs = _free_set(f, rate=0.05)
    traj, _ = _steps_against_oracle(f["ff"], rs, f["pos"], f["pos"], f["box"], f["mass"], 6, gamma=0.0, kT=2.5, policy=(0.3, 10))
    # a bead under a position restraint alone: x_{k+1} = 2 x_k - x_{k-1} - dt^2 (k / m) (x_k - X), velocity Verlet's recurrence
    for i in range(3):
        k, X = np.asarray(rs.position[i].k), np.asarray(rs.position[i].reference)
        for s in range(1, 5):
            want = 2 * traj[s, i] - traj[s - 1, i] - CS.DT**2 * k / f["mass"][i] * (traj[s, i] - X)
            assert np.abs(traj[s + 1, i] - want).max() < 1e-12
    assert np.abs(traj[5, 14:] - 2 * traj[4, 14:] + traj[3, 14:]).max() < 1e-13  # the free beads drift


# ------------------------------------------------------------------------------------------------ 4
def test_umbrella_windows_sample_their_mean_and_variance():
    """Free beads of 72 amu, two groups of five (M = 360 each, reduced mass 180 amu), an umbrella on xi = (X_B - X_A) . z with
    k = 500 kJ/mol/nm^2: xi is a harmonic oscillator of omega = sqrt(k / mu) = 1.67 / ps under an Ornstein-Uhlenbeck
    thermostat of the same gamma (the O step of a group's centre is that of a particle of its total mass), for which BAOAB
    samples the configurational distribution exactly: mean init, variance kT / k = 0.005 nm^2.  gamma = 3 / ps is close to
    critical damping, the autocorrelation time gamma / omega^2 + 1 / gamma = 1.4 ps = 70 steps of 0.02 ps is under the
    sampling stride of 100 steps, and blocks of 20 samples (2 000 steps) are independent.  64 replicas, eight windows of
    eight replicas each, 20 000 steps after 1 000 of equilibration: 80 blocks per window, mean and variance within four
    standard errors of the block means.  The list is rebuilt every 10 steps with a skin of 1 nm: a free bead's thermal step
    of 0.04 nm per axis in that time stays far inside skin / 2."""
    n, n_rep, kT, k = 16, 64, 2.5, 500.0
    f = CS.free_beads(n)
    inits = np.repeat(np.linspace(0.5, 1.9, 8), 8)
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=tuple(range(0, 5))), group_b=PullGroup(members=tuple(range(5, 10))),
                                                 geometry="direction", vec=(0, 0, 1), k=k, init=inits, periodic=False)])
    sysm = _system(f["ff"], torch.float32)
    integ = _ensemble(sysm, np.full(n, 72.0), [kT] * n_rep, gamma=3.0, seeds=list(range(100, 100 + n_rep)), dt=0.02, policy=(1.0, 10))
    x0 = np.broadcast_to(f["pos"], (n_rep, n, 3)).copy()
    x0[:, 5:10, 2] += (inits - (x0[:, 5:10, 2].mean(1) - x0[:, 0:5, 2].mean(1)))[:, None]  # start at xi = init
    integ.set_restraints(rs)
    pos, vel = _dev(x0, sysm), integ.init_velocities()
    integ.load(pos, vel, f["box"])
    integ.advance(1000)
    traj, _ = integ.advance(20000, save_every=100, want_energy=False)
    xi = integ.pull_values(traj)[:, :, 0].cpu().numpy()  # (200, 64)
    assert xi.shape == (200, n_rep)
    for w in range(8):
        dev = xi[:, 8 * w:8 * w + 8] - inits[8 * w]
        blocks = dev.T.reshape(8 * 10, 20)
        m, v = blocks.mean(1), (blocks**2).mean(1)
        se_m, se_v = m.std(ddof=1) / np.sqrt(m.size), v.std(ddof=1) / np.sqrt(v.size)
        print(f"  window {w} init {inits[8 * w]:.2f}: mean - init {m.mean():+.2e} (se {se_m:.1e})  variance {v.mean():.3e} (kT / k {kT / k:.3e}, se {se_v:.1e})")
        assert abs(m.mean()) <= 4 * se_m and abs(v.mean() - kT / k) <= 4 * se_v


# ------------------------------------------------------------------------------------------------ 5
def _state(integ, sysm, shape):
    pos, vel = torch.empty(shape, dtype=sysm.dtype, device=sysm.device), torch.empty(shape, dtype=sysm.dtype, device=sysm.device)
    integ.store(pos, vel)
    return pos.cpu(), vel.cpu()


@DTYPES
def test_split_advances_replicas_and_a_cleared_set_are_bitwise(dtype):
    c, full = CS.n257(), CS.sets()["full"]
    assert all(p.rate != 0.0 for p in full.pulls[:2])
    sysm = _system(_ff(c["s"]), dtype)
    kTs = [KT, 1.1 * KT, 1.2 * KT]
    a, b = 7, 6

    def run_ensemble(calls):
        integ = _ensemble(sysm, c["masses"], kTs)
        integ.set_restraints(full, reference_pos=c["ref"], box=c["boxes"])
        vel = integ.init_velocities()
        integ.load(_dev(c["pos"], sysm), vel, c["boxes"])
        rows = [integ.advance(k, save_every=1, want_energy=True) for k in calls]
        assert integ.last_recoveries() == 0
        return torch.cat([r[0] for r in rows]).cpu(), torch.cat([r[1] for r in rows]).cpu(), _state(integ, sysm, (3, 257, 3))

    def run_single(r, calls, rs, cleared=False):
        integ = _single(sysm, c["masses"], kT=kTs[r], seed=SEEDS[r])
        if rs is not None:
            integ.set_restraints(rs, reference_pos=c["ref"][r], box=c["boxes"][r])
        if cleared:
            integ.set_restraints(None)
        vel = integ.init_velocities()
        integ.load(_dev(c["pos"][r], sysm), vel, c["boxes"][r])
        rows = [integ.advance(k, save_every=1, want_energy=True) for k in calls]
        launches = integ.last_kernel_ms()["launches"]
        assert integ.last_recoveries() == 0
        return torch.cat([r_[0] for r_ in rows]).cpu(), torch.cat([r_[1] for r_ in rows]).cpu(), _state(integ, sysm, (257, 3)), launches

    one, split = run_ensemble([a + b]), run_ensemble([a, b])
    assert torch.equal(one[0], split[0]) and torch.equal(one[1], split[1]) and all(torch.equal(p, q) for p, q in zip(one[2], split[2]))
    for r in range(3):
        s_one, s_split = run_single(r, [a + b], of_replica(full, r)), run_single(r, [a, b], of_replica(full, r))
        assert torch.equal(s_one[0], s_split[0]) and torch.equal(s_one[1], s_split[1]) and all(torch.equal(p, q) for p, q in zip(s_one[2], s_split[2]))
        assert torch.equal(one[0][:, r], s_one[0]) and torch.equal(one[1][:, r], s_one[1]), r
        assert torch.equal(one[2][0][r], s_one[2][0]) and torch.equal(one[2][1][r], s_one[2][1]), r
    never, cleared, kept = run_single(0, [a, b], None), run_single(0, [a, b], of_replica(full, 0), cleared=True), run_single(0, [a, b], of_replica(full, 0))
    assert torch.equal(never[0], cleared[0]) and torch.equal(never[1], cleared[1]) and all(torch.equal(p, q) for p, q in zip(never[2], cleared[2]))
    assert never[3] == cleared[3] and never[3] > 0
    assert not torch.equal(never[0], kept[0])


# ------------------------------------------------------------------------------------------------ 6
def test_a_thin_skin_recovers_with_stiff_restraints_and_still_matches_the_oracle():
    """The recipe of tests/test_gpu_martini_ensemble.py::test_a_thin_skin_recovers_and_split_still_equals_unsplit - md1285 x 2
    in fp64, kT and 1.6 kT, dt 1 fs, skin 0.01 nm, no scheduled rebuild inside the call - with a position restraint of
    k = 10^6 kJ/mol/nm^2 on every bead, its reference up to 0.008 nm per axis off the start (forces of 10^4 kJ/mol/nm: the
    beads cross skin / 2 = 0.005 nm within a quarter period of 10 steps).  Halts and resumed launches must neither repeat
    nor drop a kick: one kick of k dt |x - X| / m ~ 1e-1 nm/ps moves a bead by 1e-4 nm within a step, five orders above the
    tolerance."""
    from tests import martini_synth as S

    s = S.get("md1285")
    n, box = s["n"], s["box"][0]
    boxes = np.stack([box, box * 1.02])
    x0 = np.stack([s["pos"][0], s["pos"][0] * 1.02])
    off = np.random.default_rng(61).uniform(-0.008, 0.008, size=(n, 3))
    kTs = [KT, 1.6 * KT]
    sets = [MartiniRestraints(position=[PositionRestraint(index=i, k=1.0e6, reference=tuple(x0[r, i] + off[i])) for i in range(n)]) for r in range(2)]
    # one set for the ensemble: the references are per replica through reference_pos
    rs = MartiniRestraints(position=[PositionRestraint(index=i, k=1.0e6) for i in range(n)])
    sysm = _system(_ff(s), torch.float64)
    integ = _ensemble(sysm, s["mass"], kTs, gamma=1.0, seeds=SEEDS, dt=0.001, policy=(0.01, 1000))
    integ.set_restraints(rs, reference_pos=x0 + off[None])
    pos, vel = _dev(x0, sysm), integ.init_velocities()
    v0 = vel.cpu().numpy().copy()
    integ.run(pos, vel, boxes, 30)
    print(f"  recoveries {integ.last_recoveries()}")
    assert integ.last_recoveries() > 0 and integ.step == 30
    for r in range(2):
        orc = CS.oracle_with_field(sets[r], _ff(s), True, boxes[r], 0.001, kTs[r], 1.0, s["mass"], SEEDS[r], None)
        xo, vo = x0[r].copy(), v0[r].copy()
        orc.run(xo, vo, 30)
        dx, dv = np.abs(pos[r].cpu().numpy() - xo).max(), np.abs(vel[r].cpu().numpy() - vo).max()
        print(f"  replica {r}: |dx| {dx:.2e} |dv| {dv:.2e}, moved {np.abs(xo - x0[r]).max():.4f} nm")
        assert dx <= 1e-9 and dv <= 1e-9


# ------------------------------------------------------------------------------------------------ 7
def test_nve_drift_with_restraints_is_no_larger_than_twice_the_drift_without():
    c = CS.n257()
    rs = static(of_replica(CS.sets()["full"], 0))
    sysm = _system(_ff(c["s"]), torch.float64)
    drift = {}
    for name, restraints in (("plain", None), ("restrained", rs)):
        integ = _single(sysm, c["masses"], gamma=0.0, dt=0.005, policy=(0.25, 5))
        if restraints is not None:
            integ.set_restraints(restraints, reference_pos=c["ref"][0], box=c["boxes"][0])
        pos, vel = _dev(c["pos"][0], sysm), integ.init_velocities()
        traj, et = integ.run(pos, vel, c["boxes"][0], 2000, save_every=100)
        e = et.sum(1).cpu().numpy()
        if restraints is not None:
            e = e + np.array([float(integ.external_field(traj[k].contiguous(), step=0)[1].sum()) for k in range(traj.shape[0])])
        drift[name] = float(np.abs(e - e[0]).max())
        print(f"  {name}: E {e[0]:.4f} -> {e[-1]:.4f} kJ/mol, max |E - E_0| {drift[name]:.3e}, recoveries {integ.last_recoveries()}")
    assert drift["restrained"] <= 2.0 * drift["plain"]


# ------------------------------------------------------------------------------------------------ 8
def test_barostat_and_exchange_refuse_a_set_in_either_order():
    c = CS.n257()
    sysm = _system(_ff(c["s"]), torch.float64)
    rs = CS.sets()["one"]
    baro = dict(kind="berendsen", coupling="isotropic", ref_p=1.0, compressibility=4.5e-5, tau_p=1.0, every=10)
    integ = _single(sysm, c["masses"])
    integ.set_barostat(**baro)
    with pytest.raises(ValueError, match="together with a barostat"):
        integ.set_restraints(rs, reference_pos=c["ref"][0])
    integ.set_barostat(None)
    integ.set_restraints(rs, reference_pos=c["ref"][0])
    with pytest.raises(ValueError, match="barostat together with restraints"):
        integ.set_barostat(**baro)
    integ.set_restraints(None)
    integ.set_barostat(**baro)
    ens = _ensemble(sysm, c["masses"], [KT, 1.1 * KT])
    ens.set_exchange(10, seed=1)
    with pytest.raises(ValueError, match="together with replica exchange"):
        ens.set_restraints(rs, reference_pos=c["ref"][:2])
    ens.set_exchange(0)
    ens.set_restraints(rs, reference_pos=c["ref"][:2])
    with pytest.raises(ValueError, match="exchange together with restraints"):
        ens.set_exchange(10, seed=1)
    ens.set_restraints(None)
    ens.set_exchange(10, seed=1)


# ------------------------------------------------------------------------------------------------ 9
@functools.lru_cache(maxsize=None)
def _bilayer():
    from mythos_amd.energy import martini as M
    from tests import martini_helpers as MH

    s = MH.system()
    x, box, _ = MH.frames("lj")
    top = s["top"]
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    fn = M.MartiniComposedEnergyFunction([M.LJ.from_topology(topology=top, params=M.LJConfiguration(**s["lj_params"])),
                                          M.Bond.from_topology(topology=top, params=M.BondConfiguration(**s["bond_params"])),
                                          M.Angle.from_topology(topology=top, params=M.AngleConfiguration(**ap))])
    po4 = np.flatnonzero(np.asarray(top.atom_names) == "PO4")
    z = x[3][po4, 2]
    lower, upper = po4[z < z.mean()], po4[z >= z.mean()]
    assert len(lower) == len(upper) == 64
    return dict(fn=fn, top=top, x=x[3], box=box[3], lower=lower, upper=upper)


def test_the_bilayer_follows_an_umbrella_on_the_distance_between_its_leaflets():
    from mythos_amd.simulators.hip_martini import HipMartiniSimulator

    b = _bilayer()

    def run(k, init):
        rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=tuple(b["lower"]), pbc_ref=int(b["lower"][0])),
                                                     group_b=PullGroup(members=tuple(b["upper"]), pbc_ref=int(b["upper"][0])),
                                                     geometry="distance", dim=(False, False, True), k=k, init=init, periodic=True)])
        sim = HipMartiniSimulator(energy_fn=b["fn"], topology=b["top"], init_positions=b["x"], box=b["box"], temperatures=[300.0], dt=0.02,
                                  gamma=1.0, equilibration_steps=300, simulation_steps=300, save_every=10, neighbors=(0.4, 5), restraints=rs,
                                  precision="float32", name="pull")
        out = sim.run({}, seed=5)
        integ = sim._resident["integrator"]
        pull = out.state["pull"]
        traj = out.observables[0].center[:, None].contiguous()
        assert pull.shape == (30, 1, 1) and pull.dtype == torch.float64 and pull.is_cuda and torch.equal(pull, integ.pull_values(traj))
        sim.release()
        return float(pull.mean())

    free = run(0.0, 0.0)  # k = 0: the coordinate is measured, nothing is pulled
    init = free + 0.3
    held = run(50000.0, init)
    print(f"  PO4 - PO4 distance in z: unrestrained mean {free:.4f} nm, init {init:.4f} nm, restrained mean {held:.4f} nm")
    assert free < held < init and abs(held - init) < abs(held - free)
