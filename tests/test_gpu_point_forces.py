"""Point forces in the oxDNA Langevin integrator (mythos_langevin_set_point_forces: oxDNA's moving string, trap, mutual
trap, repulsion plane and repulsion sphere), held to

 * tests/point_forces_ref.py, the NumPy reference of the five laws, through mythos_langevin_eval_external_at - every
   branch, the minimum image, three replicas through the layout;
 * the BAOAB recurrence of a free nucleotide under a moving trap and a force ramp, evaluated on the host, which pins the
   time convention s = step at the start of the queue + launch index;
 * oracle/langevin_oracle.py with the reference field added, step by step;
 * bitwise identity across two advances and a forced recovery, and where nothing should change;
 * the refusals that need a resident state;
 * and a repulsion sphere that keeps 64 replicas of two loose strands inside.

The helpers of tests/test_gpu_restraints.py build the systems: the tolerances are that file's, argued there.
"""

import dataclasses as dc

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.simulators.restraints import (GroupTorque, MovingString, MutualTrap, PointForces, RepulsionPlane, RepulsionSphere, Restraints,
                                              SelfTether, SumRestraint, Trap)
from mythos_amd.utils import generators
from tests import helpers as H
from tests import oxdna_periodic_synth as synth
from tests import point_forces_ref as ref
from tests import test_gpu_restraints as R

pytestmark = pytest.mark.gpu

KT = R.KT
EPS32 = R.EPS32
_make, _free_system, _dev, _mixed, _field_atol = R._make, R._free_system, R._dev, R._mixed, R._field_atol


def _integrator(s, **kw):
    from mythos_amd.hip_system import LangevinIntegrator

    args = {"dt": 0.005, "kT": KT, "gamma_t": KT / 2.5, "gamma_r": KT / 7.5, "seed": 7}
    args.update(kw)
    return LangevinIntegrator(s, **args)


def _helix():
    top, traj, _, _ = H.load_golden(2, "simple-helix")
    return top, traj, np.asarray(traj.center[0], dtype=np.float64), np.asarray(traj.quaternions[0], dtype=np.float64)


def _all_kinds(x, rate=1.0):
    """One term of every kind, and then some, on the 16-nt helix at x; every one-sided law in its acting branch.  Nucleotide
    8 carries a moving trap and a ramp (and, in _mixed, a tether, the sum restraint and the torque group)."""
    r = rate
    d_0_15, d_3_12 = np.linalg.norm(x[15] - x[0]), np.linalg.norm(x[12] - x[3])
    centre = x.mean(axis=0)
    return PointForces([
        Trap(8, x[8] + (0.1, -0.2, 0.05), 30.0, 2e-3 * r, (1, 1, 0)), MovingString(8, 0.2, 1e-2 * r, (0, 0, 1)),
        MutualTrap(0, 15, 5.0, 0.8 * d_0_15, 1e-3 * r), MutualTrap(15, 0, 5.0, 0.8 * d_0_15, 1e-3 * r), MutualTrap(3, 12, 4.0, 1.3 * d_3_12, -1e-3 * r),
        RepulsionPlane(5, 20.0, (0, 1, 1), -(x[5, 1] + x[5, 2]) / np.sqrt(2.0) - 0.3), RepulsionPlane(6, 20.0, (0, 1, 1), -(x[6, 1] + x[6, 2]) / np.sqrt(2.0) + 0.3),
        *(RepulsionSphere(i, centre, 0.9 * np.linalg.norm(x[i] - centre), 8.0, -1e-3 * r) for i in (1, 10)), RepulsionSphere(2, centre, 50.0, 8.0, 1e-3 * r),
        Trap(13, x[13] + (0.0, 0.1, 0.0), 12.0), MovingString(4, -0.1, -5e-3 * r, (1, 0, 0))])


# ------------------------------------------------------------------ 1. the field against the NumPy reference
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_external_field_at_against_the_numpy_reference(dtype):
    """The 16-nt helix tiled 17 times (272 free nucleotides); the point terms name nucleotides 0 .. 256, so the kick runs a
    second, partial workgroup of one entry.  In one call: a plane with h < 0 (1) and with h > 0 (2); a sphere with the
    nucleotide outside (3) and inside (4, and the wide one on all of 0 .. 256); mutual traps shorter (5 -> 10) and longer
    (6 -> 11) than r0; nucleotide 7 with a tether, a sum group, a torque group, a moving trap and a ramp; a mutual trap
    whose partner, 270, has no entry; constant forces.  At s = 0 and s = 12345.
    Tolerances, those of test_external_field_against_the_numpy_reference: fp64 rtol 1e-12 plus the summation-order bound
    of the group reductions; fp32 - the reference at the rounded inputs - the two roundings of the output.  The point laws
    are the same double arithmetic added in the same order and rounded once; the mutual trap's D / r is one more square
    root and division in double."""
    _, _, c0, _ = _helix()
    n = 16 * 17
    s = _free_system(n, dtype)
    rng = np.random.default_rng(21)
    x = np.concatenate([c0 + (6.0 * (k % 5), 6.0 * (k // 5), 0.0) for k in range(17)]) + 0.01 * rng.standard_normal((n, 3))
    xd = _dev(x, dtype, s)
    x = xd.double().cpu().numpy()
    centre = x[:257].mean(axis=0)
    dist = lambda i, j: float(np.linalg.norm(x[j] - x[i]))  # noqa: E731
    pf = PointForces([
        RepulsionPlane(1, 20.0, (0, 1, 1), -(x[1, 1] + x[1, 2]) / np.sqrt(2.0) - 0.3), RepulsionPlane(2, 20.0, (0, 1, 1), -(x[2, 1] + x[2, 2]) / np.sqrt(2.0) + 0.3),
        RepulsionSphere(3, x[3] + (0.5, 0.0, 0.0), 0.25, 8.0, 1e-6), RepulsionSphere(4, x[4] + (0.5, 0.0, 0.0), 0.75, 8.0, 1e-6),
        MutualTrap(5, 10, 5.0, 1.25 * dist(5, 10), 1e-6), MutualTrap(6, 11, 5.0, 0.75 * dist(6, 11), 1e-6),
        Trap(7, x[7] + (0.1, -0.2, 0.05), 30.0, 1e-5, (1, 1, 0)), MovingString(7, 0.2, 1e-5, (0, 3, 4)),
        MutualTrap(9, 270, 2.0, 1.0, -1e-6),
        *(RepulsionSphere(i, centre, 11.0, 3.0, -1e-5) for i in range(257))])
    rs = ref.resolved(Restraints(tethers=[SelfTether([7, 20], 40.0)], sums=[SumRestraint([7, 30], 40.0)], torques=[GroupTorque([7, 8, 40, 41], (0.0, 0.03, 0.3))]),
                      x + 0.05 * rng.standard_normal((n, 3)))
    assert sorted({t.particle for t in pf.terms}) == list(range(257)) and 270 not in {t.particle for t in pf.terms}
    const = (np.array([3, 100, 271]), _dev(rng.uniform(-1.0, 1.0, (3, 3)), dtype, s).double().cpu().numpy())
    integ = _integrator(s)
    integ.set_external_forces(*const)
    integ.set_restraints(rs)
    integ.set_point_forces(pf)
    for step in (0, 12345):
        F, e = integ.external_field_at(xd, step)
        Fw, ew = ref.field(x, rs, pf, float(step), const)
        assert torch.isfinite(F).all() and e.shape == (8,)
        assert ew[3] != 0 and all(ew[4:] > 0)
        scale = np.abs(Fw).max()
        atol = _field_atol(x, rs) + (0.0 if dtype == torch.float64 else 2 * EPS32 * scale)
        np.testing.assert_allclose(F.double().cpu().numpy(), Fw, rtol=1e-12 if dtype == torch.float64 else EPS32, atol=atol, err_msg=str(step))
        np.testing.assert_allclose(e.cpu().numpy(), ew, rtol=1e-12, atol=1e-12 * np.abs(ew).max() + 1e-9 * _field_atol(x, rs), err_msg=str(step))
    # every branch was there, and the clock matters
    at = lambda i, step: [ref.point_term(x, t, step)[1] for t in pf.terms[:9]][i]  # noqa: E731
    assert at(0, 0.0) > 0 and at(1, 0.0) == 0 and at(2, 0.0) > 0 and at(3, 0.0) == 0
    outside = [ref.point_term(x, t, 12345.0)[1] > 0 for t in pf.terms[9:]]
    assert any(outside) and not all(outside)
    F0, e0 = integ.external_field_at(xd, 0)
    assert float((F - F0).abs().max()) > 1e-3
    # mythos_langevin_eval_external is the same call at step 0 with the first three words
    F3, e3 = integ.external_field(xd)
    assert torch.equal(F3, F0) and torch.equal(e3, e0[:3])
    # the two sets are independent: either goes without the other
    integ.set_restraints()
    integ.set_external_forces()
    F, e = integ.external_field_at(xd, 12345)
    Fw, ew = ref.point_field(x, pf, 12345.0)
    np.testing.assert_allclose(F.double().cpu().numpy(), Fw, rtol=1e-12 if dtype == torch.float64 else EPS32, atol=0.0 if dtype == torch.float64 else EPS32 * np.abs(Fw).max())
    np.testing.assert_allclose(e.cpu().numpy()[3:], ew, rtol=1e-12)
    assert not e[:3].any()
    integ.set_restraints(rs)
    integ.set_point_forces()
    F, e = integ.external_field_at(xd, 12345)
    Fw, ew = R.ref.field(x, rs)
    np.testing.assert_allclose(F.double().cpu().numpy(), Fw, rtol=1e-12 if dtype == torch.float64 else EPS32,
                               atol=_field_atol(x, rs) + (0.0 if dtype == torch.float64 else EPS32 * np.abs(Fw).max()))
    assert not e[3:].any() and not integ.point_forces
    integ.set_restraints()
    F, e = integ.external_field_at(xd, 12345)
    assert not F.any() and not e.any()


# ------------------------------------------------------------------ 2. the minimum image
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_mutual_trap_across_a_face_takes_the_minimum_image(dtype):
    """The golden helix placed by tests/oxdna_periodic_synth.py: its second strand sits one lattice vector (-L, +L, -L) from
    its first, so the pair 0 - 15 is a base pair only through the image.  PBC = 1 agrees with the reference's minimum
    image; PBC = 0 takes the distance as stored, 20 sqrt(3) away, and differs."""
    top, c, q, box = synth.crossing_helix(2, "simple-helix")
    s = _make(2, top, box, dtype)
    xd = _dev(c, dtype, s)
    x = xd.double().cpu().numpy()
    assert np.abs(np.rint((x[15] - x[0]) / box)).sum() == 3  # (an image in every component)
    integ = _integrator(s)
    out = {}
    for pbc in (True, False):
        pf = PointForces([MutualTrap(0, 15, 5.0, 1.2, 1e-4, pbc), MutualTrap(15, 0, 5.0, 1.2, 1e-4, pbc), MutualTrap(7, 8, 2.0, 0.5, 0.0, pbc)])
        integ.set_point_forces(pf)
        F, e = integ.external_field_at(xd, 100)
        Fw, ew = ref.point_field(x, pf, 100.0, box=box)
        rtol, atol = (1e-12, 0.0) if dtype == torch.float64 else (EPS32, EPS32 * np.abs(Fw).max())
        np.testing.assert_allclose(F.double().cpu().numpy(), Fw, rtol=rtol, atol=atol)
        np.testing.assert_allclose(e.cpu().numpy()[3:], ew, rtol=1e-12)
        out[pbc] = F.double().cpu().numpy()
    assert np.abs(out[True][0]).max() < 10.0 < np.abs(out[False][0]).max()  # a base pair's length against the box diagonal
    np.testing.assert_allclose(out[True][0], -out[True][15], rtol=1e-6)
    # without a box the flag is refused, and names the term
    top0, _, c0, _ = _helix()
    free = _integrator(_make(2, top0, None, dtype))
    with pytest.raises(ValueError, match=r"term 1 \(mutual_trap\): PBC = 1 on a system without a box"):
        free.set_point_forces(PointForces([Trap(0, (0, 0, 0), 1.0), MutualTrap(0, 15, 5.0, 1.2, 0.0, True)]))
    assert not free.point_forces


# ------------------------------------------------------------------ 3. replicas
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_point_forces_of_three_replicas_through_the_layout(dtype):
    """The set repeated per replica by PointForces.lower - pos0 and center moved by the replica's translation, a plane's
    position by -d.offset, a string's energy origin at the offset: every replica gets the field, and the energies, of
    its own frame.  The reference shifts each term by hand."""
    from mythos_amd.simulators.replicas import ReplicaLayout

    _, _, c0, _ = _helix()
    n_one, n_rep = 16, 3
    s = _free_system(n_one * n_rep, dtype)
    rng = np.random.default_rng(9)
    x0 = _dev(c0, dtype, s)
    pf = _all_kinds(x0.double().cpu().numpy())
    layout = ReplicaLayout(n_rep, n_one)
    c, _, offsets = layout.place(x0, torch.zeros((n_one, 4), dtype=dtype, device=s.device), 4.0)
    moved = (c + _dev(0.01 * rng.standard_normal((n_rep * n_one, 3)), dtype, s)).contiguous()
    _, off = layout.restraint_frames(x0, offsets)
    assert np.abs(off[1:]).max() > 4.0
    integ = _integrator(s)
    integ.set_point_forces(pf, n_one=n_one, n_rep=n_rep, offsets=off)
    F, e = integ.external_field_at(moved, 777)
    xs = moved.double().cpu().numpy().reshape(n_rep, n_one, 3)
    want, ew = [], np.zeros(5)
    for r in range(n_rep):
        shifted = []
        for t in pf.terms:
            if isinstance(t, Trap):
                t = dc.replace(t, pos0=np.asarray(t.pos0) + off[r])
            elif isinstance(t, RepulsionSphere):
                t = dc.replace(t, center=np.asarray(t.center) + off[r])
            elif isinstance(t, RepulsionPlane):
                t = dc.replace(t, position=t.position - float(np.dot(t.dir, off[r])))
            shifted.append(t)
        f, u = ref.point_field(xs[r], PointForces(shifted), 777.0, origin=off[r])
        want.append(f)
        ew += u
    want = np.concatenate(want)
    rtol, atol = (1e-12, 0.0) if dtype == torch.float64 else (EPS32, 2 * EPS32 * np.abs(want).max())
    np.testing.assert_allclose(F.double().cpu().numpy(), want, rtol=rtol, atol=atol)
    np.testing.assert_allclose(e.cpu().numpy()[3:], ew, rtol=1e-12, atol=1e-12 * np.abs(ew).max())
    assert np.abs(want).max() > 1.0 and all(ew[1:] > 0)


# ------------------------------------------------------------------ 4. closed form
def _baoab_free(x, p, force, steps, dt, c1, s0=0):
    """B A O A B of free unit masses without noise, F = force(x, s) at the step count of the frame: -> x after every step."""
    h, out = 0.5 * dt, []
    x, p = x.copy(), p.copy()
    for k in range(steps):
        p = p + h * force(x, s0 + k)
        x = x + h * p
        p = c1 * p
        x = x + h * p
        p = p + h * force(x, s0 + k + 1)
        out.append(x.copy())
    return np.array(out)


def _moving_set(n, x0, rng):
    """Moving traps on 0 .. 39, force ramps on 40 .. 79, both on 80 .. 85; the rest of the n flies free."""
    terms = []
    for i in range(40):
        terms.append(Trap(i, x0[i] + 0.3 * rng.standard_normal(3), float(rng.uniform(5.0, 80.0)), float(rng.uniform(1e-3, 5e-3)), rng.standard_normal(3)))
    for i in range(40, 80):
        terms.append(MovingString(i, float(rng.uniform(-0.5, 0.5)), float(rng.uniform(1e-3, 1e-2)), rng.standard_normal(3)))
    for i in range(80, 86):
        terms += [MovingString(i, 0.1, 2e-3, (0, 0, 1)), Trap(i, x0[i], 25.0, 2e-3, (1, 0, 0))]
    return PointForces(terms)


def test_free_nucleotides_under_a_moving_trap_and_a_ramp_follow_the_recurrence():
    """No neighbours, kT = 0 (no noise; friction stays): the integrator is the linear recurrence B A O A B with
    F(x_s, s), which the host evaluates in double.  atol 1e-11, that of
    test_tethered_free_nucleotides_follow_the_closed_form.  The same recurrence with the clock one step late is told
    apart by more than a hundred times that: the test pins s = step at the start of the queue + launch index."""
    n, steps, dt, gamma = 96, 50, 0.005, 0.7
    s = _free_system(n)
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-20.0, 20.0, size=(n, 3))
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    p0, L0 = 0.3 * rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3))
    pf = _moving_set(n, x0, rng)
    integ = _integrator(s, dt=dt, kT=0.0, gamma_t=gamma, gamma_r=gamma)
    integ.set_point_forces(pf)
    state = [_dev(v, torch.float64, s) for v in (x0, q0, p0, L0)]
    tc, _, _ = integ.run(*state, steps, save_every=1, want_energy=False)
    force = lambda x, k: ref.point_field(x, pf, float(k))[0]  # noqa: E731
    want = _baoab_free(x0, p0, force, steps, dt, np.exp(-gamma * dt))
    for k in (1, 2, 17, steps):
        np.testing.assert_allclose(tc[k - 1].cpu().numpy(), want[k - 1], rtol=0, atol=1e-11)
    late = _baoab_free(x0, p0, lambda x, k: force(x, k - 1), steps, dt, np.exp(-gamma * dt))
    assert np.abs(late[-1] - want[-1]).max() > 100 * 1e-11
    assert integ.step == steps


# ------------------------------------------------------------------ 5. the oracle, step by step
def test_step_by_step_parity_with_the_oracle_with_all_eight_kinds(md_lanes):
    """The 16-nt helix in its box under the five point laws, the three restraint laws and constant forces, six steps
    against the CPU integrator with the reference field added at the step count of each force evaluation - the closing
    evaluation of a step is the opening one of the next, at the next count.  The tolerances of
    test_step_by_step_parity_with_the_oracle_with_all_three_kinds."""
    from oracle.langevin_oracle import LangevinOracle

    top, traj, c0, q0 = _helix()
    rs = _mixed(top.n_nucleotides, c0)
    pf = _all_kinds(c0)
    const = (np.array([0, 8]), np.array([[0, 0, 0.3], [0.11, -0.2, 0.07]]))
    s = _make(2, top, traj.box_size, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    gam_t, gam_r, seed, inertia, start = KT / 2.5, KT / 7.5, 0x1234ABCD5678, (1.0, 1.3, 0.8), 40
    integ = _integrator(s, gamma_t=gam_t, gamma_r=gam_r, mass=1.0, inertia=inertia, seed=seed)
    integ.set_external_forces(*const)
    integ.set_restraints(rs, c0)
    integ.set_point_forces(pf)
    integ.step = start

    class Forced(LangevinOracle):
        calls = 0

        def forces(self, x, q):  # (step calls it twice: at the frame it starts from, then at the frame it reaches)
            u, F, tau = super().forces(x, q)
            at = self.step_index + self.calls % 2
            self.calls += 1
            return u, F + ref.field(x, rs, pf, float(at), const)[0], tau

    orc = Forced(2, H.oracle_params(2, salt=0.5, half_charged_ends=False), H.topo_tensors(top), traj.box_size, 0.005, KT, gam_t, gam_r, 1.0, inertia, seed=seed)
    orc.step_index = start
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    n_steps = 6
    tc, tq, et = integ.run(c, q, p, L, n_steps, save_every=1)
    for k in range(n_steps):
        x, qq, pp, LL, u = orc.step(x, qq, pp, LL)
        np.testing.assert_allclose(tc[k].cpu().numpy(), x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(tq[k].cpu().numpy(), qq, rtol=0, atol=1e-10)
        assert abs(et[k, :8].sum().item() - u) < 1e-8 * abs(u)  # the rows hold the model's energy alone
    np.testing.assert_allclose(c.cpu().numpy(), x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(q.cpu().numpy(), qq, rtol=0, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=0, atol=1e-9)
    assert integ.step == start + n_steps
    # the point forces did act, and so did their clock: the field at the first and at the last count differ
    Fa, Fb = ref.point_field(x, pf, float(start))[0], ref.point_field(x, pf, float(start + n_steps))[0]
    assert np.abs(Fa).max() > 0.1 and np.abs(Fa - Fb).max() > 1e-3


# ------------------------------------------------------------------ 6. the clock across launches
def _duplex_with_moving_terms(seed):
    top, c0, q0 = generators.ideal_duplex(24, model=2, seed=seed)
    c0 = c0 + 0.02 * np.random.default_rng(8).standard_normal(c0.shape)
    pf = PointForces([Trap(0, c0[0], 30.0, 5e-4, (0, 0, -1)), Trap(47, c0[47] + (0.1, 0.0, 0.0), 30.0, 0.0), MovingString(23, 0.1, 1e-3, (0, 0, 1)),
                      MovingString(24, 0.1, 1e-3, (0, 0, 1)), MutualTrap(10, 37, 3.0, 1.0, 1e-3), RepulsionSphere(23, c0.mean(axis=0), 3.0, 5.0, -1e-3)])
    return top, c0, q0, pf


@pytest.mark.parametrize("rows", [False, True])
def test_two_advances_continue_the_clock_like_one(rows):
    """advance(3); advance(4) == advance(7), bit for bit, under a moving trap, a ramp and a shrinking sphere beside the
    restraints and constant forces: the second call's kicks take the step count where the first left it."""
    top, c0, q0, pf = _duplex_with_moving_terms(3)
    rs = _mixed(top.n_nucleotides, c0)
    outs = []
    for plan in ((7,), (3, 4)):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = _integrator(s, dt=0.003, seed=99)
        integ.set_neighbor_policy(r_cut=3.3, skin=0.6, every=5)
        integ.set_external_forces([0, 47], [[0, 0, 0.3], [0, 0, -0.3]])
        integ.set_restraints(rs)
        integ.set_point_forces(pf)
        integ.step = 1000
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = integ.init_momenta()
        integ.load(c, q, p, L)
        for n in plan:
            integ.advance(n, save_every=(7 if len(plan) == 1 else 2) if rows else 0)
        integ.store(c, q, p, L)
        assert integ.step == 1007
        outs.append((c, q, p, L))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # (and the clock is in it: the same run from step 0 ends elsewhere)
    s = _make(2, top, None, torch.float64, hce=True)
    integ = _integrator(s, dt=0.003, seed=99)
    integ.set_neighbor_policy(r_cut=3.3, skin=0.6, every=5)
    integ.set_point_forces(pf)
    ends = []
    for start in (0, 1000):
        integ.step = start
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = _dev(np.zeros_like(c0), torch.float64, s), _dev(np.zeros_like(c0), torch.float64, s)
        integ.set_seed(5)
        integ.run(c, q, p, L, 7)
        ends.append(p)
    assert float((ends[0] - ends[1]).abs().max()) > 1e-3


def test_a_forced_recovery_keeps_the_clock():
    """Segments of four launches, the scheduled rebuild in front of launch 8 claims an overflow
    (test_a_forced_recovery_applies_every_kick_once): the kick of launch 8 skips with the launch, the list is rebuilt and the
    run resumes there with the step count that launch had.  Bit for bit the undisturbed run."""
    top, c0, q0, pf = _duplex_with_moving_terms(77)
    rs = _mixed(top.n_nucleotides, c0)
    results = []
    for inject in (False, True):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = _integrator(s, seed=5)
        integ.set_neighbor_policy(3.3, 0.6, 4)
        integ.set_restraints(rs)
        integ.set_point_forces(pf)
        integ.step = 300
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = integ.init_momenta()
        _lib.debug_set("md_segment", 4)
        if inject:
            _lib.debug_set("md_overflow_at", 9)
        try:
            tc, tq, et = integ.run(c, q, p, L, 20, save_every=4)
        finally:
            _lib.debug_set("md_segment", 0)
            _lib.debug_set("md_overflow_at", 0)
        results.append((c, q, p, L, tc, et, integ.last_recoveries(), integ.step))
    plain, hit = results
    assert plain[6] == 0 and hit[6] == 1 and plain[7] == hit[7] == 320
    for a, b in zip(plain[:6], hit[:6]):
        assert torch.equal(a, b)


def test_setting_the_step_moves_the_clock():
    """Free nucleotides at kT = 0 (the noise stream, which also counts steps, is multiplied by zero): a run from
    integ.step = v is the run from step 0 of the terms advanced by v on the host - F0 + rate v, pos0 + rate v d.
    Not bit for bit: (x - pos0) - rate (v + k) d and (x - (pos0 + rate v d)) - rate k d round differently, by an ulp or
    two of coordinates of order 20, 1e-14, times stiff dt^2 = 2e-3 per step over 40 steps - under 1e-14 in a position;
    atol 1e-12.  The run that ignores v is 1e-3 away."""
    n, steps, v = 96, 40, 4096
    s = _free_system(n)
    rng = np.random.default_rng(4)
    x0 = rng.uniform(-20.0, 20.0, size=(n, 3))
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    p0, L0 = 0.3 * rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3))
    pf = _moving_set(n, x0, rng)
    advanced = PointForces([dc.replace(t, F0=t.F0 + t.rate * v) if isinstance(t, MovingString) else dc.replace(t, pos0=np.asarray(t.pos0) + t.rate * v * np.asarray(t.dir))
                            for t in pf.terms])
    ends = {}
    for name, terms, start in (("moved", pf, v), ("advanced", advanced, 0), ("ignored", pf, 0)):
        integ = _integrator(s, kT=0.0, gamma_t=0.7, gamma_r=0.7)
        integ.set_point_forces(terms)
        integ.step = start
        state = [_dev(a, torch.float64, s) for a in (x0, q0, p0, L0)]
        integ.run(*state, steps)
        assert integ.step == start + steps
        ends[name] = state[0].cpu().numpy()
        integ.close()
    np.testing.assert_allclose(ends["moved"], ends["advanced"], rtol=0, atol=1e-12)
    assert np.abs(ends["moved"] - ends["ignored"]).max() > 1e-3


# ------------------------------------------------------------------ 7. bit for bit where nothing should change
def _run_helix(dtype, mode, restraints, steps=50):
    """The 16-nt golden helix for ``steps``; mode: None (set_point_forces never called), "on", "cleared" (set, then cleared),
    "empty" (called with nothing); with or without the restraints and constant forces of tests/test_gpu_restraints.py."""
    top, traj, c0, q0 = _helix()
    s = _make(2, top, traj.box_size, dtype)
    s.set_neighbors(top.unbonded_neighbors)
    integ = _integrator(s)
    c, q = _dev(c0, dtype, s), _dev(q0, dtype, s)
    x = c.double().cpu().numpy()
    if restraints:
        integ.set_external_forces([0, 15, 7, 8, 3], [[0, 0, 0.3], [0, 0, 0.3], [0, 0, -0.3], [0, 0, -0.3], [0.11, -0.2, 0.07]])
        integ.set_restraints(_mixed(top.n_nucleotides, x))
    if mode in ("on", "cleared"):
        integ.set_point_forces(_all_kinds(x))
    if mode in ("cleared", "empty"):
        integ.set_point_forces()
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, steps)
    return c, q, p, L


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nothing_changes_without_point_forces(dtype):
    """With restraints and constant forces, and with neither: an integrator whose point forces were set and cleared, or
    set to nothing, runs what the integrator that never heard of them runs, bit for bit."""
    for restraints in (True, False):
        never = _run_helix(dtype, None, restraints)
        for mode in ("cleared", "empty"):
            got = _run_helix(dtype, mode, restraints)
            for a, b in zip(never, got):
                assert torch.equal(a, b), (mode, restraints)
        on = _run_helix(dtype, "on", restraints)
        assert float((on[0] - never[0]).abs().max()) > 1e-4  # (the point forces do act)


# ------------------------------------------------------------------ 8. refusals that need a resident state
def test_refusals_with_a_resident_state():
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.hip_system import OxdnaSystem
    from mythos_amd.input import defaults

    top, traj, c0, q0 = _helix()
    s = _make(2, top, traj.box_size, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    integ = _integrator(s)
    pf = _all_kinds(c0)
    with pytest.raises(ValueError, match=r"term 0 \(trap\): particle 16 out of range \[0, 16\)"):
        integ.set_point_forces(PointForces([Trap(16, (0, 0, 0), 1.0)]), n_one=10**6)
    with pytest.raises(ValueError, match=r"term 1 \(mutual_trap\): ref_particle is the particle itself"):
        integ.set_point_forces(PointForces([Trap(1, (0, 0, 0), 1.0), MutualTrap(4, 4, 1.0, 1.0)]))
    with pytest.raises(ValueError, match=r"term 0 \(repulsion_sphere\): stiff is negative"):
        integ.set_point_forces(PointForces([RepulsionSphere(1, (0, 0, 0), 1.0, -1.0)]))
    assert not integ.point_forces  # a refused call leaves what was there
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    integ.load(c, q, p, L)
    integ.set_point_forces(pf)
    integ.advance(2)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_point_forces(pf)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_point_forces()
    assert integ.point_forces is pf
    integ.store(c, q, p, L)
    integ.set_point_forces(PointForces(pf.terms[:3]))
    integ.advance(1)
    integ.store(c, q, p, L)
    assert torch.isfinite(c).all() and integ.step == 3
    # the unfused oxNA cross-check path does not apply them
    topn, trajn, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    _, dflt = defaults.default_configs_for("na1")
    simn, _ = defaults.default_configs_for("na1")
    flat = fp.pack_flat_na1(fp.derive_flat_na1(dflt["dna"], dflt["rna"], dflt["drh"], kt=simn["kT"], salt_conc=0.5, half_charged_ends=False), _lib.param_names())
    sn = OxdnaSystem(4, topn.seq, topn.is_end, topn.bonded_neighbors, box=trajn.box_size, dtype=torch.float64, is_rna=is_rna)
    sn.set_params(flat.detach())
    sn.set_neighbors(topn.unbonded_neighbors)
    un = _integrator(sn, dt=0.003, seed=3)
    un.set_unfused()
    cn, qn = _dev(trajn.center[2], torch.float64, sn), _dev(trajn.quaternions[2], torch.float64, sn)
    un.set_point_forces(PointForces([Trap(0, trajn.center[2][0], 5.0, 1e-3, (0, 0, 1))]))
    pn, Ln = un.init_momenta()
    with pytest.raises(ValueError, match="unfused"):
        un.run(cn, qn, pn, Ln, 2)
    un.set_unfused(False)  # the fused oxNA kernel steps with them
    un.run(cn, qn, pn, Ln, 2)
    assert torch.isfinite(cn).all()


# ------------------------------------------------------------------ 9. confinement, end to end
def test_a_repulsion_sphere_keeps_two_loose_strands_inside(tmp_path):
    """64 replicas of the golden helix's two 8-nt strands, the second moved 3 units off the first across the helix axis
    (unpaired: out of hydrogen-bonding range), through HipMDSimulator(point_forces=<an oxDNA external-force file>): one
    repulsion_sphere block on every particle about the centroid, r0 = 2.5 (the farthest nucleotide starts at 2.12),
    stiff = 10, so sigma = sqrt(kT / stiff) = 0.1; 4000 steps of 0.005 at kT = 0.1.  No nucleotide of any replica ends
    farther from the centre than r0 + 5 sigma = 3.0 - five standard deviations of the harmonic wall's thermal penetration
    (exp(-12.5) per nucleotide at the wall) - while the same run without the sphere ends outside that radius.
    The numbers were chosen on the CPU integrator (oracle/langevin_oracle.py with tests/point_forces_ref.py's sphere
    added, six seeds of one replica each): confined, the farthest nucleotide ended at 2.43 ... 2.69 and never passed 2.74
    during a run - 2.4 sigma of the five; free, it ended at 4.27 ... 7.17.
    Observed on the GPU, the farthest nucleotide of 64 replicas at the end: confined 2.736 (2.4 sigma), free 9.65."""
    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import ComposedEnergyFunction, Quaternion, RigidBody, space
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList

    top, _, c0, q0 = _helix()
    n, n_rep, kT, r0, stiff, steps = top.n_nucleotides, 64, 0.1, 2.5, 10.0, 4000
    c0 = c0.copy()
    axis = (c0[7] - c0[0]) / np.linalg.norm(c0[7] - c0[0])
    away = c0[8:].mean(axis=0) - c0[:8].mean(axis=0)
    away -= (away @ axis) * axis
    c0[8:] += 3.0 * away / np.linalg.norm(away)
    centre = c0.mean(axis=0)
    assert np.linalg.norm(c0 - centre, axis=1).max() < r0 - 0.3
    path = tmp_path / "external.conf"
    path.write_text("{\ntype = repulsion_sphere\nparticle = -1\ncenter = %.17g, %.17g, %.17g\nr0 = %g\nstiff = %g\n}\n" % (*centre, r0, stiff))
    disp, shift = space.free()
    ef = ComposedEnergyFunction.from_lists(energy_fns=dna2.default_energy_fns(), energy_configs=dna2.default_energy_configs({"kT": kT}),
                                           transform_fn=dna2.default_transform_fn(), displacement_fn=disp, topology=top)
    dev = torch.device("cuda", 0)
    init = RigidBody(center=torch.as_tensor(c0, device=dev), orientation=Quaternion(vec=torch.as_tensor(q0, device=dev)))
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(kT / 2.5, kT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=0.005, kT=kT)
    caged = HipMDSimulator(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin,
                           neighbors=VerletNeighborList(3.25, 0.6, 10), save_every=steps, n_replicas=n_rep, point_forces=path)
    free = dc.replace(caged, point_forces=None)
    bound = r0 + 5.0 * np.sqrt(kT / stiff)
    far = {}
    for name, sim in (("caged", caged), ("free", free)):
        out = sim.run({}, init, steps, key=3).observables[0]
        assert out.center.shape == (n_rep, n, 3) and torch.isfinite(out.center).all()
        far[name] = float(np.linalg.norm(out.center.double().cpu().numpy() - centre, axis=2).max())
    print("farthest nucleotide: caged %.4f, free %.4f, bound %.4f" % (far["caged"], far["free"], bound))
    assert far["caged"] <= bound < far["free"], far
    _, integ, _ = next(iter(caged._resident.values()))
    assert len(integ.point_forces.terms) == n and integ.step == steps
    caged.release()
    free.release()
