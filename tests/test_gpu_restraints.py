"""Position-dependent external forces in the oxDNA Langevin integrator (mythos_langevin_set_restraints: tethers, sum
restraints, group torques - the stretch-torsion protocol), held to

 * tests/ext_field_ref.py, the NumPy reference of the three laws, through mythos_langevin_eval_external;
 * the closed form of a tethered free nucleotide (position Verlet of a harmonic oscillator) and BAOAB's configurational
   variance in a harmonic well;
 * oracle/langevin_oracle.py with the reference field added, step by step;
 * bitwise identity where nothing should change, and the kick's protocol (two advances, a forced recovery, an aborted and
   repeated launch);
 * the unchanged kernel's own fp32 error;
 * the refusals of the entry point;
 * and, end to end through HipMDSimulator, the frames the reference holds for the protocol.
"""

import dataclasses as dc

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults, topology
from mythos_amd.input.lammps_restraints import read_lammps_restraints
from mythos_amd.simulators.restraints import GroupTorque, Restraints, SelfTether, SumRestraint
from mythos_amd.utils import generators
from tests import ext_field_ref as ref
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0
LAMMPS = "lammps-oxdna2-40bp"
LAMMPS_IN = H.GOLDEN / "regr" / LAMMPS / "in"
EPS64, EPS32 = 2.0**-52, 2.0**-23


def _make(model, top, box, dtype, hce=False, salt=0.5):
    from mythos_amd.hip_system import OxdnaSystem

    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=salt, half_charged_ends=hce), _lib.param_names())
    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype)
    s.set_params(flat)
    return s


def _free_system(n, dtype=torch.float64):
    """n nucleotides without bonds or neighbours."""
    from mythos_amd.hip_system import OxdnaSystem

    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=True), _lib.param_names())
    s = OxdnaSystem(2, np.arange(n, dtype=np.int32) % 4, np.ones(n, dtype=np.int32), np.zeros((0, 2), dtype=np.int32), dtype=dtype)
    s.set_params(flat)
    s.set_neighbors(np.zeros((0, 2), dtype=np.int32))
    return s


def _dev(a, dtype, s):
    return torch.as_tensor(a, dtype=dtype, device=s.device).contiguous()


def _mixed(n, x0, seed=0, k=40.0, torque=0.3):
    """All three kinds on a duplex of n nucleotides; nucleotide n // 2 is in a tether, the sum restraint and the torque group."""
    rng = np.random.default_rng(seed)
    m = n // 2
    rs = Restraints(tethers=[SelfTether([0, n - 1, m], k, x0[[0, n - 1, m]] + 0.05 * rng.standard_normal((3, 3))), SelfTether([2], 0.5 * k, None, (1, 0, 1))],
                    sums=[SumRestraint([m - 1, m], k, None, (1, 1, 0))],
                    torques=[GroupTorque([m - 2, m - 1, m, m + 1], (0.0, 0.1 * torque, torque))])
    return ref.resolved(rs, x0)


def _oracle(model, top, box, dt, gam_t, gam_r, inertia, seed, rs, const=None, salt=0.5, hce=False):
    from oracle.langevin_oracle import LangevinOracle

    class Restrained(LangevinOracle):
        def forces(self, x, q):
            u, F, tau = super().forces(x, q)
            return u, F + ref.field(x, rs, const)[0], tau

    return Restrained(model, H.oracle_params(model, salt=salt, half_charged_ends=hce), H.topo_tensors(top), box, dt, KT, gam_t, gam_r, 1.0, inertia, seed=seed)


# ------------------------------------------------------------------ 1. the field against the NumPy reference
def _sum_bound(xs):
    """Two sums of the same m numbers in different orders (NumPy's pairwise, the kernel's strided tree) differ by at most
    2 ceil(log2 m + 1) eps sum |x_j| per component, to first order."""
    m = xs.shape[0]
    return 2.0 * (np.ceil(np.log2(m)) + 1.0) * EPS64 * np.abs(xs).sum()


def _field_atol(x, rs):
    """Absolute bound on |F_kernel - F_reference| in fp64 from the summation order of the group reductions alone: a sum
    restraint multiplies the difference of the sums by k; a torque group takes its centroid from the sum (d_i off by
    delta = bound / m) and S from the d_j (relative 2 delta sum |d_j| / S), so |dF| <= |T| delta / S (1 + 2 max |d| sum |d_j| / S)."""
    tol = 0.0
    for s in rs.sums:
        tol += s.k * _sum_bound(x[list(s.index)])
    for q in rs.torques:
        xs = x[list(q.index)]
        d = xs - xs.mean(axis=0)
        T = np.asarray(q.torque)
        t = T / np.linalg.norm(T)
        S = ((d - np.outer(d @ t, t)) ** 2).sum()
        if S > ref.TORQUE_FLOOR * (xs * xs).sum():
            delta = _sum_bound(xs) / xs.shape[0]
            dn = np.linalg.norm(d, axis=1)
            tol += np.linalg.norm(T) * delta / S * (1.0 + 2.0 * dn.max() * dn.sum() / S)
    return tol


def _field_cases(n, x, rng):
    pick = lambda m: rng.permutation(n)[:m]  # noqa: E731
    anchors = lambda m: rng.uniform(-2.0, 2.0, (m, 3))  # noqa: E731
    big = pick(257)
    on_axis = np.array([5, 6, 7])
    return {
        "no tethers, groups of 2 and 4": Restraints(sums=[SumRestraint(pick(2), 3.0, rng.uniform(-2, 2, 3))], torques=[GroupTorque(pick(4), (0.1, -0.2, 0.3))]),
        "one tether, a torque group of 2": Restraints(tethers=[SelfTether(pick(1), 7.0, anchors(1), (1, 0, 1))], torques=[GroupTorque(pick(2), (0.0, 0.0, 0.241412))]),
        "257 tethers, groups of 257": Restraints(tethers=[SelfTether(big, 1217.58, anchors(257))],
                                                 sums=[SumRestraint(pick(257), 2.5, rng.uniform(-9, 9, 3), (1, 1, 1)), SumRestraint(pick(4), 1.5, rng.uniform(-2, 2, 3), (0, 1, 1))],
                                                 torques=[GroupTorque(pick(257), (0.3, 0.1, -0.2))]),
        "groups of 65 and 100 (more than one wavefront)": Restraints(sums=[SumRestraint(pick(65), 2.0, rng.uniform(-5, 5, 3), (1, 0, 1))], torques=[GroupTorque(pick(100), (0.2, 0.0, -0.1))]),
        "one nucleotide in a tether and two groups": Restraints(tethers=[SelfTether([11, 3], 9.0, anchors(2))], sums=[SumRestraint([3, 20], 4.0, rng.uniform(-2, 2, 3))],
                                                                 torques=[GroupTorque([1, 3, 8, 9], (0.0, 0.2, 0.1)), GroupTorque([3, 30], (0.5, 0.0, 0.0))]),
        "a torque group on its axis": Restraints(tethers=[SelfTether([5], 2.0, anchors(1))], torques=[GroupTorque(on_axis, (0.0, 0.0, 0.4)), GroupTorque(pick(4), (0.0, 0.0, 0.4))]),
    }


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_external_field_against_the_numpy_reference(dtype):
    """fp64: rtol 1e-12 plus the bound of the summation order (_field_atol).  fp32: the inputs are rounded to fp32 first
    and the reference is evaluated at those values, so what is left is the rounding of the output - the constant kick and
    the restraint kick each round once into the fp32 buffer: 2 eps32 of the largest force."""
    from mythos_amd.hip_system import LangevinIntegrator

    n = 600
    s = _free_system(n, dtype)
    rng = np.random.default_rng(5)
    x = rng.uniform(-2.0, 2.0, (n, 3))
    x[[5, 6, 7], :2] = x[5, :2]  # three nucleotides on a line along z
    xd = _dev(x, dtype, s)
    x = xd.double().cpu().numpy()
    # (constant forces are stored in the system's precision: the reference takes them as stored)
    const = (np.array([3, 100, 599]), _dev(rng.uniform(-1.0, 1.0, (3, 3)), dtype, s).double().cpu().numpy())
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=0.1, gamma_r=0.1, seed=1)
    F, e = integ.external_field(xd)  # nothing set: zeros
    assert not F.any() and not e.any()
    for name, rs in _field_cases(n, x, rng).items():
        for with_const in (False, True):
            integ.set_external_forces(*(const if with_const else ()))
            integ.set_restraints(rs)
            F, e = integ.external_field(xd)
            Fw, ew = ref.field(x, rs, const if with_const else None)
            assert torch.isfinite(F).all(), name
            scale = np.abs(Fw).max()
            atol = _field_atol(x, rs) + (0.0 if dtype == torch.float64 else 2 * EPS32 * scale)
            np.testing.assert_allclose(F.double().cpu().numpy(), Fw, rtol=1e-12 if dtype == torch.float64 else EPS32, atol=atol, err_msg=name)
            np.testing.assert_allclose(e.cpu().numpy(), ew, rtol=1e-12, atol=1e-12 * np.abs(ew).max() + 1e-9 * _field_atol(x, rs), err_msg=name)
    rs = _field_cases(n, x, rng)["a torque group on its axis"]
    integ.set_external_forces()
    integ.set_restraints(Restraints(torques=rs.torques[:1]))
    F, _ = integ.external_field(xd)
    assert not F.any()  # zeros, not NaN
    integ.set_restraints()
    F, e = integ.external_field(xd)
    assert not F.any() and not e.any() and not integ.restraints


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_external_field_of_three_replicas_through_the_layout(dtype):
    """The set repeated per replica by Restraints.lower, anchors and targets moved by each replica's translation: every
    replica gets the field of its own frame."""
    from mythos_amd.hip_system import LangevinIntegrator
    from mythos_amd.simulators.replicas import ReplicaLayout

    n_one, n_rep = 40, 3
    s = _free_system(n_one * n_rep, dtype)
    rng = np.random.default_rng(9)
    x0 = _dev(rng.uniform(-2.0, 2.0, (n_one, 3)), dtype, s)
    rs = Restraints(tethers=[SelfTether([0, 1, 38, 39], 1217.58)], sums=[SumRestraint([18, 21], 1217.58)], torques=[GroupTorque([18, 19, 20, 21], (0, 0, 0.241412))])
    layout = ReplicaLayout(n_rep, n_one)
    c, _, offsets = layout.place(x0, torch.zeros((n_one, 4), dtype=dtype, device=s.device), 4.0)
    moved = (c + _dev(0.01 * rng.standard_normal((n_rep * n_one, 3)), dtype, s)).contiguous()
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=0.1, gamma_r=0.1, seed=1)
    refc, off = layout.restraint_frames(x0, offsets)
    integ.set_restraints(rs, refc, n_one=n_one, n_rep=n_rep, offsets=off)
    F, e = integ.external_field(moved)
    own = ref.resolved(rs, x0.double().cpu().numpy())
    xs = moved.double().cpu().numpy().reshape(n_rep, n_one, 3)
    want, ew, order = [], np.zeros(3), 0.0
    for r in range(n_rep):  # the reference in the replica's frame at its place: anchors and targets shifted by hand
        shifted = dc.replace(own, tethers=[dc.replace(t, anchor=np.asarray(t.anchor) + off[r]) for t in own.tethers],
                             sums=[dc.replace(q, target=np.asarray(q.target) + len(q.index) * off[r]) for q in own.sums])
        f, u = ref.field(xs[r], shifted)
        want.append(f)
        ew += u
        order = max(order, _field_atol(xs[r], shifted))
    want = np.concatenate(want)
    # The reference sees the coordinates as the kernel does (rounded to the system's precision first) and the same anchors
    # and targets (a + off[r], s0 + m off[r], in double), so the bounds are those of the single-system test: fp64 rtol
    # 1e-12 plus the summation order of the four-member centroid; fp32 the one rounding of the output.  The energies are
    # summed in double in both precisions, all terms positive: rtol 1e-12 (the absolute term is for the 0 of the constant forces).
    atol = order + (0.0 if dtype == torch.float64 else 2 * EPS32 * np.abs(want).max())
    np.testing.assert_allclose(F.double().cpu().numpy(), want, rtol=1e-12 if dtype == torch.float64 else EPS32, atol=atol)
    np.testing.assert_allclose(e.cpu().numpy(), ew, rtol=1e-12, atol=1e-12 * np.abs(ew).max())
    assert np.abs(want).max() > 1.0


# ------------------------------------------------------------------ 2. closed forms
def test_tethered_free_nucleotides_follow_the_closed_form():
    """No neighbours, no friction, tethers only: BAOAB is position Verlet, whose map of a harmonic oscillator is exact -
    x_k - a = C cos(k theta) + D sin(k theta) with cos(theta) = 1 - K dt^2 / 2m; an axis the mask leaves out flies free."""
    from mythos_amd.hip_system import LangevinIntegrator

    n, steps, dt = 96, 50, 0.005
    s = _free_system(n)
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-20.0, 20.0, size=(n, 3))
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    p0, L0 = 0.3 * rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3))
    a = x0 + 0.5 * rng.standard_normal((n, 3))
    groups = [(np.arange(0, 40), 1217.58, (1, 1, 1)), (np.arange(40, 80), 55.0, (1, 0, 1)), (np.arange(80, 90), 3.0, (0, 1, 0))]
    rs = Restraints(tethers=[SelfTether(idx, k, a[idx], ax) for idx, k, ax in groups])
    integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=0.0, gamma_r=0.0, seed=7)
    integ.set_restraints(rs)
    state = [_dev(v, torch.float64, s) for v in (x0, q0, p0, L0)]
    tc, _, _ = integ.run(*state, steps, save_every=1, want_energy=False)
    K = np.zeros((n, 3))
    for idx, k, ax in groups:
        K[idx] = k * np.asarray(ax, dtype=np.float64)
    cos = 1.0 - K * dt * dt / 2.0
    theta = np.arccos(cos)
    C = x0 - a
    x1 = C * cos + dt * p0  # one step of position Verlet, m = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.where(K > 0, (x1 - C * cos) / np.sin(theta), 0.0)
    for k in (1, 2, 17, steps):
        want = np.where(K > 0, a + C * np.cos(k * theta) + D * np.sin(k * theta), x0 + k * dt * p0)
        np.testing.assert_allclose(tc[k - 1].cpu().numpy(), want, rtol=0, atol=1e-11)
    assert float(np.abs(tc[steps - 1].cpu().numpy() - (x0 + steps * dt * p0))[:40].max()) > 1e-3  # (the tethers did act)


def _baoab_stationary(K, dt, kT, gamma, m=1.0):
    """Stationary covariance of (x - a, p) under B A O A B in a harmonic well of stiffness K: the map is linear,
    z' = M z + N xi, so the covariance is the fixed point of S = M S M^T + N N^T (iterated to convergence)."""
    h = dt / 2
    B, A = np.array([[1.0, 0.0], [-h * K, 1.0]]), np.array([[1.0, h / m], [0.0, 1.0]])
    c1 = np.exp(-gamma * dt)
    M = B @ A @ np.diag([1.0, c1]) @ A @ B
    N = B @ A @ np.array([0.0, np.sqrt(kT * (1 - c1 * c1) * m)])
    S = np.zeros((2, 2))
    for _ in range(4000):
        S = M @ S @ M.T + np.outer(N, N)
    return S


def test_the_variance_in_a_harmonic_well_is_baoabs():
    """4096 tethered free nucleotides with friction, 2000 steps: <(x - a)^2> per component equals the stationary variance of
    the B A O A B map in a harmonic well within four standard errors.  That variance, from the map itself
    (_baoab_stationary), is kT / K exactly - BAOAB samples a harmonic well's positions without step-size error - and the
    momenta carry the error, <p^2> = m kT (1 - K dt^2 / 4m).  The inflated figure kT / K / (1 - K dt^2 / 4m) is not
    this splitting's: against the fixed point of the map it is 0.0020645 against 0.002
    (K dt^2 / 4 = 0.031 here), and the test asserts that its standard error is small enough to tell the two apart (at least
    eight standard errors between them).  Frames every 50 steps (2.5 time units, gamma = 2: decorrelated) from step 500 on;
    the standard error from 64 blocks of 64 nucleotides."""
    from mythos_amd.hip_system import LangevinIntegrator

    n, dt, K, kT, gamma = 4096, 0.05, 50.0, 0.1, 2.0
    s = _free_system(n)
    rng = np.random.default_rng(2)
    x0 = rng.uniform(-20.0, 20.0, size=(n, 3))
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    integ = LangevinIntegrator(s, dt=dt, kT=kT, gamma_t=gamma, gamma_r=gamma, seed=11)
    integ.set_restraints(Restraints(tethers=[SelfTether(np.arange(n), K)]), x0)
    c, q = _dev(x0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    tc, _, _ = integ.run(c, q, p, L, 2000, save_every=50, want_energy=False)
    S = _baoab_stationary(K, dt, kT, gamma)
    assert abs(S[0, 0] - kT / K) < 1e-12 and abs(S[1, 1] - kT * (1 - K * dt * dt / 4)) < 1e-12
    d2 = ((tc[10:].cpu().numpy() - x0) ** 2).mean(axis=(0, 2))  # per nucleotide
    blocks = d2.reshape(64, 64).mean(axis=1)
    mean, se = blocks.mean(), blocks.std(ddof=1) / np.sqrt(64)
    inflated = kT / K / (1.0 - K * dt * dt / 4.0)
    print("variance %.6e +- %.1e, stationary %.6e, kT / K / (1 - K dt^2 / 4) %.6e" % (mean, se, S[0, 0], inflated))
    assert abs(mean - S[0, 0]) <= 4.0 * se
    assert abs(inflated - S[0, 0]) > 8.0 * se  # (the test has the resolution to tell the two figures apart)
    p2 = (p.cpu().numpy() ** 2).mean(axis=1).reshape(64, 64).mean(axis=1)  # the momenta of the last step
    print("<p^2> %.5f +- %.5f, stationary %.5f" % (p2.mean(), p2.std(ddof=1) / 8, S[1, 1]))
    assert abs(p2.mean() - S[1, 1]) <= 4.0 * p2.std(ddof=1) / 8


# ------------------------------------------------------------------ 3. the oracle, step by step
def _parity(model, top, box, c0, q0, rs, const, salt=0.5):
    from mythos_amd.hip_system import LangevinIntegrator

    s = _make(model, top, box, torch.float64, salt=salt)
    s.set_neighbors(top.unbonded_neighbors)
    gam_t, gam_r, seed, inertia = KT / 2.5, KT / 7.5, 0x1234ABCD5678, (1.0, 1.3, 0.8)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=gam_t, gamma_r=gam_r, mass=1.0, inertia=inertia, seed=seed)
    if const is not None:
        integ.set_external_forces(*const)
    integ.set_restraints(rs, c0)
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    n_steps = 6
    tc, tq, et = integ.run(c, q, p, L, n_steps, save_every=1)
    orc = _oracle(model, top, box, 0.005, gam_t, gam_r, inertia, seed, ref.resolved(rs, c0), const, salt=salt)
    for k in range(n_steps):
        x, qq, pp, LL, u = orc.step(x, qq, pp, LL)
        np.testing.assert_allclose(tc[k].cpu().numpy(), x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(tq[k].cpu().numpy(), qq, rtol=0, atol=1e-10)
        assert abs(et[k, :8].sum().item() - u) < 1e-8 * abs(u)  # the rows hold the model's energy, no restraint energy
    np.testing.assert_allclose(c.cpu().numpy(), x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(q.cpu().numpy(), qq, rtol=0, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=0, atol=1e-9)
    assert integ.step == n_steps
    return c, integ


def test_step_by_step_parity_with_the_oracle_under_the_lammps_protocol(md_lanes):
    """The 80-nt duplex of the reference's LAMMPS run, its frame 0, in its periodic box, under the protocol read from its input."""
    top, traj, _ = H.load_lammps_regr(LAMMPS)
    rs, const = read_lammps_restraints(LAMMPS_IN, n=top.n_nucleotides)
    c0 = np.asarray(traj.center[0], dtype=np.float64) + 0.003 * np.random.default_rng(4).standard_normal((80, 3))  # (off the anchors)
    rs = dc.replace(rs, tethers=[dc.replace(t, anchor=np.asarray(traj.center[0])[list(t.index)]) for t in rs.tethers])
    _parity(2, top, traj.box_size, c0, np.asarray(traj.quaternions[0]), rs, const, salt=0.15)


def test_step_by_step_parity_with_the_oracle_with_all_three_kinds(md_lanes):
    top, traj, _, _ = H.load_golden(2, "simple-helix")
    c0 = np.asarray(traj.center[0], dtype=np.float64)
    rs = _mixed(top.n_nucleotides, c0)
    const = (np.array([0, 8]), np.array([[0, 0, 0.3], [0.11, -0.2, 0.07]]))
    _parity(2, top, traj.box_size, c0, np.asarray(traj.quaternions[0]), rs, const)


# ------------------------------------------------------------------ 4. bit for bit
def _run_helix(dtype, mode, steps=20, const=False):
    """The 16-nt golden helix for ``steps``; mode: None (set_restraints never called), "on", "zero" (k = 0, no torque),
    "cleared" (set, then cleared), "empty" (called with nothing)."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    s = _make(2, top, traj.box_size, dtype)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=7)
    c, q = _dev(traj.center[0], dtype, s), _dev(traj.quaternions[0], dtype, s)
    rs = _mixed(top.n_nucleotides, c.double().cpu().numpy())
    if const:
        integ.set_external_forces([0, 15, 7, 8, 3], [[0, 0, 0.3], [0, 0, 0.3], [0, 0, -0.3], [0, 0, -0.3], [0.11, -0.2, 0.07]])
    if mode in ("on", "cleared"):
        integ.set_restraints(rs)
    if mode == "zero":
        integ.set_restraints(Restraints(tethers=[dc.replace(t, k=0.0) for t in rs.tethers], sums=[dc.replace(x, k=0.0) for x in rs.sums]))
    if mode in ("cleared", "empty"):
        integ.set_restraints()
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, steps)
    return c, q, p, L


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nothing_changes_without_restraints(dtype):
    """k = 0 and no torque, set and cleared, or an empty set: the run that never had any, bit for bit - also with constant
    forces, whose launches a second integrator that never heard of restraints issues alone."""
    for const in (False, True):
        never = _run_helix(dtype, None, steps=50, const=const)
        for mode in ("zero", "cleared", "empty"):
            got = _run_helix(dtype, mode, steps=50, const=const)
            for a, b in zip(never, got):
                assert torch.equal(a, b), (mode, const)
    on = _run_helix(dtype, "on", steps=50)
    assert float((on[0] - never[0]).abs().max()) > 1e-4  # (the restraints do act)


@pytest.mark.parametrize("rows", [False, True])
def test_two_advances_continue_like_one(rows):
    """advance(3); advance(4) == advance(7), bit for bit, with all three kinds and constant forces (the cadences of
    tests/test_gpu_external_forces.py)."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, c0, q0 = generators.ideal_duplex(24, model=2, seed=3)
    rs = _mixed(top.n_nucleotides, c0)
    outs = []
    for plan in ((7,), (3, 4)):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = LangevinIntegrator(s, dt=0.003, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=99)
        integ.set_neighbor_policy(r_cut=3.3, skin=0.6, every=5)
        integ.set_external_forces([0, 47], [[0, 0, 0.3], [0, 0, -0.3]])
        integ.set_restraints(rs)
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = integ.init_momenta()
        integ.load(c, q, p, L)
        for n in plan:
            integ.advance(n, save_every=(7 if len(plan) == 1 else 2) if rows else 0)
        integ.store(c, q, p, L)
        assert integ.step == 7
        outs.append((c, q, p, L))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_a_forced_recovery_applies_every_kick_once():
    """Segments of four launches, the scheduled rebuild in front of launch 8 claims an overflow: the restraint kick of launch
    8 skips with the launch, the run recovers and resumes there.  Bit for bit the undisturbed run."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, c0, q0 = generators.ideal_duplex(24, model=2, seed=77)
    c0 = c0 + 0.02 * np.random.default_rng(8).standard_normal(c0.shape)
    rs = _mixed(top.n_nucleotides, c0)
    results = []
    for inject in (False, True):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=5)
        integ.set_neighbor_policy(3.3, 0.6, 4)
        integ.set_restraints(rs)
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
    assert plain[6] == 0 and hit[6] == 1 and plain[7] == hit[7] == 20
    for a, b in zip(plain[:6], hit[:6]):
        assert torch.equal(a, b)


def test_an_aborted_and_repeated_launch_kicks_once(md_lanes):
    """The crowded blob of tests/test_gpu_external_forces.py (the first launch aborts and is repeated with the wide work
    lists) with a tether on every nucleotide: anchors a distance of order one away and k = 1e9 make forces of 1e9, a kick of
    0.5 per launch against that test's tolerances (4e-4 on a momentum, 1e-12 on a position).  The momenta match the oracle
    only if the repeated launch's restraint kick was a no-op."""
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    def blob(n, radius, seed, min_dist=0.27):
        rng = np.random.default_rng(seed)
        pts = []
        while len(pts) < n:
            v = rng.uniform(-radius, radius, 3)
            if np.linalg.norm(v) <= radius and all(np.linalg.norm(v - w) >= min_dist for w in pts):
                pts.append(v)
        qq = rng.standard_normal((n, 4))
        return np.array(pts), qq / np.linalg.norm(qq, axis=1, keepdims=True)

    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=False), _lib.param_names())
    dt, n = 1e-9, 26
    top = topology.from_arrays(np.arange(n) % 4, [1] * n)
    c0, q0 = blob(n, 0.62, 4)
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=None, dtype=torch.float64)
    s.set_params(flat)
    s.set_neighbors(top.unbonded_neighbors)
    anchor = c0 + np.random.default_rng(3).uniform(-1.0, 1.0, size=(n, 3))
    rs = Restraints(tethers=[SelfTether(np.arange(n), 1e9, anchor)])
    integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=12)
    integ.set_restraints(rs)
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    tc, tq, et = integ.run(c, q, p, L, 4, save_every=2)
    assert integ.last_recoveries() == 1 and integ.step == 4
    lo = _oracle(2, top, None, dt, KT / 2.5, KT / 7.5, (1.0, 1.0, 1.0), 12, rs)
    for k in range(4):
        x, qq, pp, LL, u = lo.step(x, qq, pp, LL)
        if k % 2 == 1:
            np.testing.assert_allclose(tc[k // 2].cpu().numpy(), x, rtol=1e-11, atol=1e-12)
            assert abs(et[k // 2, :8].sum().item() - u) <= 1e-9 * abs(u)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=1e-8, atol=1e-9 * np.abs(pp).max())
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=1e-8, atol=1e-9 * np.abs(LL).max())
    kick = 0.5 * dt * 1e9 * np.abs(anchor - c0).max()  # what the aborted first launch's kick, applied twice, would add
    assert kick > 100 * (1e-8 + 1e-9) * np.abs(pp).max() and dt * kick > 100 * 1e-12


# ------------------------------------------------------------------ 5. fp32
def _run_lammps(dtype, protocol, steps=20):
    from mythos_amd.hip_system import LangevinIntegrator

    top, traj, _ = H.load_lammps_regr(LAMMPS)
    s = _make(2, top, traj.box_size, dtype, salt=0.15)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=7)
    c, q = _dev(traj.center[0], dtype, s), _dev(traj.quaternions[0], dtype, s)
    if protocol:
        rs, const = read_lammps_restraints(LAMMPS_IN, n=top.n_nucleotides)
        integ.set_external_forces(*const)
        integ.set_restraints(rs, c)
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, steps)
    return c, q, p, L


def test_fp32_under_the_protocol_is_as_close_to_fp64_as_without():
    """The distance between the fp32 and the fp64 run under the LAMMPS protocol is at most twice the distance the same two
    runs show unrestrained: the bound is the unchanged kernel's own fp32 error, measured here, not a constant."""
    dist = {}
    for protocol in (False, True):
        a, b = _run_lammps(torch.float64, protocol), _run_lammps(torch.float32, protocol)
        dist[protocol] = [float((x.double() - y.double()).abs().max()) for x, y in zip(a[:2], b[:2])]
    print("fp32 - fp64 (positions, quaternions): unrestrained", dist[False], "protocol", dist[True])
    assert dist[False][0] > 0 and dist[False][1] > 0
    assert dist[True][0] <= 2 * dist[False][0] and dist[True][1] <= 2 * dist[False][1], dist
    moved = (_run_lammps(torch.float64, True)[0] - _run_lammps(torch.float64, False)[0]).abs().max()
    assert float(moved) > 100 * dist[False][0]  # (the protocol did act)


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    n = top.n_nucleotides
    s = _make(2, top, traj.box_size, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=7)
    c0 = np.asarray(traj.center[0], dtype=np.float64)
    a3 = [(0.0, 0.0, 0.0)]

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            integ.set_restraints(Restraints(**kw), c0, n_one=10**6)  # (n_one: the Python side's own range check out of the way)

    def refused_by_the_entry_point(match, key, value, **kw):
        """Restraints.lower refuses a negative index itself, whatever n_one: a valid set is lowered, the index replaced in
        the arrays, and the arrays handed to the C entry point."""
        a = Restraints(**kw).lower(c0, n_one=n)
        a[key][-1] = value
        ip, dp = (lambda x: x.ctypes.data_as(_lib.c_int_p)), (lambda x: x.ctypes.data_as(_lib.c_double_p))
        rc = integ._lib.mythos_langevin_set_restraints(
            integ._h, int(a["t_index"].shape[0]), ip(a["t_index"]), dp(a["t_k"]), dp(a["t_anchor"]), ip(a["t_mask"]),
            int(a["g_kind"].shape[0]), ip(a["g_kind"]), ip(a["g_first"]), ip(a["g_member"]), dp(a["g_vec"]), dp(a["g_target"]), ip(a["g_mask"]))
        with pytest.raises(ValueError, match=match):
            _lib.check(rc, "set_restraints")

    refused("out of range", tethers=[SelfTether([n], 1.0, a3)])
    refused("out of range", sums=[SumRestraint([0, n], 1.0, a3[0])])
    refused("out of range", torques=[GroupTorque([0, n + 1], (0, 0, 1.0))])
    refused_by_the_entry_point(r"index -1 out of range", "t_index", -1, tethers=[SelfTether([1], 1.0, a3)])
    refused_by_the_entry_point(r"index -2 out of range", "g_member", -2, sums=[SumRestraint([0, 1], 1.0, a3[0])])
    refused_by_the_entry_point(r"index -2 out of range", "g_member", -2, torques=[GroupTorque([0, 1], (0, 0, 1.0))])
    refused_by_the_entry_point(r"index %d out of range" % n, "g_member", n, torques=[GroupTorque([0, 1], (0, 0, 1.0))])
    refused("listed twice among the tethers", tethers=[SelfTether([4], 1.0, a3), SelfTether([4], 2.0, a3)])
    refused("listed twice in group", sums=[SumRestraint([1, 2], 1.0, a3[0]), SumRestraint([3, 5, 3], 1.0, a3[0])])
    refused("listed twice in group", torques=[GroupTorque([3, 5, 3], (0, 0, 1.0))])
    refused("finite", tethers=[SelfTether([1], np.nan, a3)])
    refused("finite", tethers=[SelfTether([1], 1.0, [(0.0, np.inf, 0.0)])])
    refused("finite", sums=[SumRestraint([1, 2], 1.0, (0.0, np.nan, 0.0))])
    refused("finite", sums=[SumRestraint([1, 2], np.inf, a3[0])])
    refused("finite", torques=[GroupTorque([1, 2], (0.0, np.nan, 0.0))])
    refused("negative", tethers=[SelfTether([1], -1.0, a3)])
    refused("negative", sums=[SumRestraint([1, 2], -1.0, a3[0])])
    refused("zero", torques=[GroupTorque([1, 2], (0.0, 0.0, 0.0))])
    refused("0 members", sums=[SumRestraint([], 1.0, a3[0])])
    refused("1 members", torques=[GroupTorque([3], (0, 0, 1.0))])
    assert not integ.restraints  # a refused call leaves what was there
    with pytest.raises(ValueError, match="reference_center"):
        integ.set_restraints(Restraints(tethers=[SelfTether([1], 1.0)]))
    # valid before load and after store, refused while the frame is open
    rs = _mixed(n, c0)
    c, q = _dev(traj.center[0], torch.float64, s), _dev(traj.quaternions[0], torch.float64, s)
    p, L = integ.init_momenta()
    integ.load(c, q, p, L)
    integ.set_restraints(rs)
    integ.advance(2)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_restraints(rs)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_restraints()
    assert integ.restraints is rs
    integ.store(c, q, p, L)
    integ.set_restraints(dc.replace(rs, torques=()))
    integ.advance(1)
    integ.store(c, q, p, L)
    assert torch.isfinite(c).all()
    # the unfused oxNA cross-check path does not apply them
    topn, trajn, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    _, dflt = defaults.default_configs_for("na1")
    simn, _ = defaults.default_configs_for("na1")
    flat = fp.pack_flat_na1(fp.derive_flat_na1(dflt["dna"], dflt["rna"], dflt["drh"], kt=simn["kT"], salt_conc=0.5, half_charged_ends=False), _lib.param_names())
    sn = OxdnaSystem(4, topn.seq, topn.is_end, topn.bonded_neighbors, box=trajn.box_size, dtype=torch.float64, is_rna=is_rna)
    sn.set_params(flat.detach())
    sn.set_neighbors(topn.unbonded_neighbors)
    un = LangevinIntegrator(sn, dt=0.003, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=3)
    un.set_unfused()
    cn, qn = _dev(trajn.center[2], torch.float64, sn), _dev(trajn.quaternions[2], torch.float64, sn)
    un.set_restraints(Restraints(tethers=[SelfTether([0], 5.0)]), cn)
    pn, Ln = un.init_momenta()
    with pytest.raises(ValueError, match="unfused"):
        un.run(cn, qn, pn, Ln, 2)
    un.set_unfused(False)  # the fused oxNA kernel steps with them
    un.run(cn, qn, pn, Ln, 2)
    assert torch.isfinite(cn).all()


# ------------------------------------------------------------------ 7. end to end
def test_the_stretch_torsion_protocol_end_to_end():
    """64 replicas of the reference's 80-nt duplex through HipMDSimulator(restraints=..., external_forces=...), both read
    from the reference's LAMMPS input; kT 0.1, salt 0.15 (the run's dh line), sequence-dependent stacking and hydrogen
    bonding as that run; 2 x 10^4 steps, a frame every 200, statistics from the second half.  With sigma = sqrt(kT / K):

     (a) the tether rms per component, over replicas and frames, lies within three standard errors of the golden frames'
         own (0.855 sigma; the SE is that of an rms from 132 samples taken as independent, rms / sqrt(2 * 132), computed
         from the fixture).  A stiffness wrong by a factor of two lands at 0.60 or 1.2 sigma, outside the band;
     (b) the xy sum of 38 + 41 has rms <= sigma (1 + 3 SE), SE from the replica blocks;
     (c) the mean ExtensionZ(bp1=(0, 79), bp2=(38, 41)) lies inside [min, max] of golden frames 1-11;
     (d) the mean TwistXY at torque +0.241412 exceeds the mean at -0.241412 by at least five standard errors, replicas as
         blocks: a sign-and-plumbing check, as test_a_pulled_duplex_is_longer is.

    The reference's LAMMPS energy has no bonded excluded volume and ours does (tests/test_gpu_oxdna_energy.py: LAMMPS's pair
    styles skip bonded neighbours); neither (a) nor (c) is sensitive to it at these widths."""
    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import ComposedEnergyFunction, Quaternion, RigidBody, space
    from mythos_amd.observables import ExtensionZ, TwistXY
    from mythos_amd.observables.base import get_duplex_quartets
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList

    top, traj, _ = H.load_lammps_regr(LAMMPS)
    n, n_rep, kT, K = top.n_nucleotides, 64, 0.1, 1217.58
    rs, const = read_lammps_restraints(LAMMPS_IN, n=n)
    gold = np.asarray(traj.center, dtype=np.float64)
    sigma = np.sqrt(kT / K)
    w = H.read_ss_weights(H.GOLDEN / "regr" / "simple-helix-oxdna2-ss" / "oxDNA2_sequence_dependent_parameters.txt")
    over = {"kT": kT, "salt_conc": 0.15, "half_charged_ends": False,
            "stacking": {"ss_stack_weights": torch.as_tensor(w["ss_stack_weights"]), "eps_stack_kt_coeff": w["eps_stack_kt_coeff"]},
            "hydrogen_bonding": {"ss_hb_weights": torch.as_tensor(w["ss_hb_weights"])}}
    disp, shift = space.free()
    ef = ComposedEnergyFunction.from_lists(energy_fns=dna2.default_energy_fns(), energy_configs=dna2.default_energy_configs(over),
                                           transform_fn=dna2.default_transform_fn(), displacement_fn=disp, topology=top)
    dev = torch.device("cuda", 0)
    init = RigidBody(center=torch.as_tensor(gold[0], device=dev), orientation=Quaternion(vec=torch.as_tensor(traj.quaternions[0], device=dev)))
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(kT / 2.5, kT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=0.005, kT=kT)
    plus = HipMDSimulator(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin,
                          neighbors=VerletNeighborList(3.25, 0.6, 20), save_every=200, n_replicas=n_rep, external_forces=const, restraints=rs)
    minus = dc.replace(plus, restraints=dc.replace(rs, torques=[dc.replace(q, torque=tuple(-np.asarray(q.torque))) for q in rs.torques]))
    _, cfg = defaults.default_configs_for("dna2")
    twist, ext = TwistXY(get_duplex_quartets(n // 2), disp, cfg["geometry"]), ExtensionZ((0, 79), (38, 41), disp)
    tw = {}
    for name, sim in (("plus", plus), ("minus", minus)):
        out = sim.run({}, init, 20000, key=3).observables[0]
        assert out.center.shape == (n_rep * 100, n, 3) and torch.isfinite(out.center).all()
        per_replica = twist(out).reshape(n_rep, 100)[:, 50:].mean(dim=1)
        tw[name] = (float(per_replica.mean()), float(per_replica.std() / np.sqrt(n_rep)))
        if name == "plus":
            x = out.center.double().cpu().numpy().reshape(n_rep, 100, n, 3)[:, 50:]
            extension = ext(out).reshape(n_rep, 100)[:, 50:]
    # (a)
    t = rs.tethers[0]
    g = gold[1:, list(t.index)] - gold[0, list(t.index)]
    gold_rms = np.sqrt((g * g).mean())
    gold_se = gold_rms / np.sqrt(2 * g.size)
    d = x[:, :, list(t.index)] - gold[0, list(t.index)]
    rms = np.sqrt((d * d).mean())
    print("(a) tether rms / sigma %.4f, golden %.4f +- %.4f" % (rms / sigma, gold_rms / sigma, gold_se / sigma))
    assert g.size == 132 and abs(rms - gold_rms) <= 3 * gold_se
    # (b)
    ssum = x[:, :, list(rs.sums[0].index)].sum(axis=2)[..., :2]
    per_rep = np.sqrt((ssum * ssum).mean(axis=(1, 2)))
    rms_s, se_s = np.sqrt((ssum * ssum).mean()), per_rep.std(ddof=1) / np.sqrt(n_rep)
    print("(b) sum rms / sigma %.4f +- %.4f" % (rms_s / sigma, se_s / sigma))
    assert rms_s <= sigma + 3 * se_s
    # (c)
    from tests.duplex_ref import extension_z  # (the NumPy form the golden frames are measured with)

    gold_ext = extension_z(gold[1:], (0, 79), (38, 41), None)
    print("(c) extension %.4f, golden %.4f ... %.4f" % (float(extension.mean()), gold_ext.min(), gold_ext.max()))
    assert gold_ext.min() <= float(extension.mean()) <= gold_ext.max()
    # (d)
    print("(d) twist: +T %.4f +- %.4f, -T %.4f +- %.4f" % (*tw["plus"], *tw["minus"]))
    assert tw["plus"][0] - tw["minus"][0] >= 5.0 * np.hypot(tw["plus"][1], tw["minus"][1]), tw
    _, integ, _ = next(iter(plus._resident.values()))
    assert integ.restraints is rs and integ.external_forces[0].size == 2 * n_rep
    plus.release()
    minus.release()
