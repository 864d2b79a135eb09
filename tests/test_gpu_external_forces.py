"""Constant external forces in the oxDNA Langevin integrator (mythos_langevin_set_external_forces): the kick launch in
front of every step launch, held to

 * the closed form for free nucleotides (leapfrog is exact for a constant force);
 * oracle/langevin_oracle.py with the force added, step by step, for oxDNA1 / oxDNA2 / oxRNA2 and both lane widths;
 * the unchanged kernel's own fp32 error;
 * bitwise identity where nothing should change: no forces, zero forces, forces set and cleared, advance(a); advance(b)
   against advance(a + b), a forced recovery, an aborted and repeated launch;
 * the refusals of the entry point;
 * and, with the duplex observables, the sign of the response: a pulled duplex is longer.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults, topology
from mythos_amd.utils import generators
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0


def _make(model, top, box, dtype, hce=False, salt=0.5):
    from mythos_amd.hip_system import OxdnaSystem

    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=salt, half_charged_ends=hce), _lib.param_names())
    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype)
    s.set_params(flat)
    return s


def _dev(a, dtype, s):
    return torch.as_tensor(a, dtype=dtype, device=s.device).contiguous()


def _pull(n):
    """+-0.3 along z on the two end pairs of a duplex of n nucleotides, plus one oblique force."""
    idx = np.array([0, n - 1, n // 2 - 1, n // 2, 3])
    f = np.array([[0, 0, 0.3], [0, 0, 0.3], [0, 0, -0.3], [0, 0, -0.3], [0.11, -0.2, 0.07]])
    return idx, f


def _oracle(model, top, box, dt, gam_t, gam_r, inertia, seed, idx, f, salt=0.5, hce=False):
    from oracle.langevin_oracle import LangevinOracle

    class Pulled(LangevinOracle):
        def forces(self, x, q):
            u, F, tau = super().forces(x, q)
            F = F.copy()
            np.add.at(F, idx, f)
            return u, F, tau

    return Pulled(model, H.oracle_params(model, salt=salt, half_charged_ends=hce), H.topo_tensors(top), box, dt, KT, gam_t, gam_r, 1.0, inertia, seed=seed)


def test_free_nucleotides_follow_the_closed_form():
    """No neighbours, no friction: x_k = x_0 + k dt p_0 / m + (k dt)^2 F / 2m and p_k = p_0 + k dt F, which the leapfrog
    reproduces exactly; the nucleotides without a force are, bit for bit, those of a run that never had any."""
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    n, steps, dt = 96, 50, 0.005
    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=True), _lib.param_names())
    s = OxdnaSystem(2, np.arange(n, dtype=np.int32) % 4, np.ones(n, dtype=np.int32), np.zeros((0, 2), dtype=np.int32), dtype=torch.float64)
    s.set_params(flat)
    s.set_neighbors(np.zeros((0, 2), dtype=np.int32))
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-20.0, 20.0, size=(n, 3))
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    p0, L0 = 0.3 * rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3))
    idx = np.arange(0, n, 2)
    f = rng.uniform(-2.0, 2.0, size=(idx.size, 3))
    out = []
    for forced in (True, False):
        integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=0.0, gamma_r=0.0, seed=7)
        if forced:
            integ.set_external_forces(idx, f)
        state = [_dev(a, torch.float64, s) for a in (x0, q0, p0, L0)]
        tc, _, _ = integ.run(*state, steps, save_every=1, want_energy=False)
        out.append((tc, *state))
    tc, c, q, p, L = out[0]
    F = np.zeros((n, 3))
    F[idx] = f
    for k in (1, 2, 17, steps):
        want = x0 + k * dt * p0 + 0.5 * (k * dt) ** 2 * F
        np.testing.assert_allclose(tc[k - 1].cpu().numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    want_p = p0 + steps * dt * F
    np.testing.assert_allclose(p.cpu().numpy(), want_p, rtol=1e-12, atol=1e-12 * np.abs(want_p).max())
    free = np.setdiff1d(np.arange(n), idx)
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a[..., free, :], b[..., free, :])
    assert not torch.equal(out[0][1][idx], out[1][1][idx])


@pytest.mark.parametrize(("model", "name", "salt"), [(2, "simple-helix", 0.5), (1, "simple-helix", 0.5), (3, "simple-helix-12bp", 1.0)])
def test_step_by_step_parity_with_the_oracle_under_force(model, name, salt, md_lanes):
    from mythos_amd.hip_system import LangevinIntegrator

    top, traj, _, _ = H.load_golden(model, name)
    s = _make(model, top, traj.box_size, torch.float64, salt=salt)
    s.set_neighbors(top.unbonded_neighbors)
    gam_t, gam_r, seed, inertia = KT / 2.5, KT / 7.5, 0x1234ABCD5678, (1.0, 1.3, 0.8)
    idx, f = _pull(top.n_nucleotides)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=gam_t, gamma_r=gam_r, mass=1.0, inertia=inertia, seed=seed)
    integ.set_external_forces(idx, f)
    c, q = _dev(traj.center[0], torch.float64, s), _dev(traj.quaternions[0], torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    n_steps = 6
    tc, tq, et = integ.run(c, q, p, L, n_steps, save_every=1)
    orc = _oracle(model, top, traj.box_size, 0.005, gam_t, gam_r, inertia, seed, idx, f, salt=salt)
    for k in range(n_steps):
        x, qq, pp, LL, u = orc.step(x, qq, pp, LL)
        np.testing.assert_allclose(tc[k].cpu().numpy(), x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(tq[k].cpu().numpy(), qq, rtol=0, atol=1e-10)
        assert abs(et[k, :8].sum().item() - u) < 1e-8 * abs(u)  # the rows hold the model's energy, not -F.x
    np.testing.assert_allclose(c.cpu().numpy(), x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(q.cpu().numpy(), qq, rtol=0, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=0, atol=1e-9)
    assert integ.step == n_steps


def _run_helix(dtype, forces, steps=20, zero=False, clear=False, call=True):
    from mythos_amd.hip_system import LangevinIntegrator

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    s = _make(2, top, traj.box_size, dtype)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=7)
    idx, f = _pull(top.n_nucleotides)
    if forces:
        integ.set_external_forces(idx, f)
    elif call:
        if zero:
            integ.set_external_forces(idx, np.zeros_like(f))
        if clear:
            integ.set_external_forces(idx, f)
            integ.set_external_forces()
    c, q = _dev(traj.center[0], dtype, s), _dev(traj.quaternions[0], dtype, s)
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, steps)
    return c, q, p, L


def test_fp32_under_force_is_as_close_to_fp64_as_without():
    """The distance between the fp32 and the fp64 run with forces is at most twice the distance the same two runs show
    with no force set: the bound is the unchanged kernel's own fp32 error, measured here, not a constant."""
    dist = {}
    for forces in (False, True):
        a, b = _run_helix(torch.float64, forces), _run_helix(torch.float32, forces)
        dist[forces] = [float((x.double() - y.double()).abs().max()) for x, y in zip(a[:2], b[:2])]
    print("fp32 - fp64 (positions, quaternions): no force", dist[False], "forces", dist[True])
    assert dist[False][0] > 0 and dist[False][1] > 0
    assert dist[True][0] <= 2 * dist[False][0] and dist[True][1] <= 2 * dist[False][1], dist
    moved = (_run_helix(torch.float64, True)[0] - _run_helix(torch.float64, False)[0]).abs().max()
    assert float(moved) > 100 * dist[False][0]  # (the forces did act)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nothing_changes_without_forces(dtype):
    never = _run_helix(dtype, False, steps=50, call=False)
    for kw in ({"zero": True}, {"clear": True}):
        got = _run_helix(dtype, False, steps=50, **kw)
        for a, b in zip(never, got):
            assert torch.equal(a, b), kw


@pytest.mark.parametrize("rows", [False, True])
def test_two_advances_continue_like_one(rows):
    """advance(3); advance(4) == advance(7), bit for bit, with forces - without rows, and with energy rows at a cadence
    of two steps (the first call saves at its step 2, the second at its steps 2 and 4, where it closes; the single call
    saves and closes at 7: energy-trace launches at different steps of the same trajectory).  A call that CLOSES in the
    middle - an energy row on the last step of the first call, or store - splits that step's external kick in two
    halves, which add up to the same kick to rounding, not to the bit: the oracle comparison below covers it."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, c0, q0 = generators.ideal_duplex(24, model=2, seed=3)
    idx, f = _pull(top.n_nucleotides)
    outs = []
    for plan in ((7,), (3, 4)):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = LangevinIntegrator(s, dt=0.003, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=99)
        integ.set_neighbor_policy(r_cut=3.3, skin=0.6, every=5)
        integ.set_external_forces(idx, f)
        c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
        p, L = integ.init_momenta()
        integ.load(c, q, p, L)
        for n in plan:
            if rows:
                integ.advance(n, save_every=7 if len(plan) == 1 else 2)
            else:
                integ.advance(n)
        integ.store(c, q, p, L)
        assert integ.step == 7
        outs.append((c, q, p, L))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    plain = _make(2, top, None, torch.float64, hce=True)
    integ = LangevinIntegrator(plain, dt=0.003, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=99)
    integ.set_neighbor_policy(r_cut=3.3, skin=0.6, every=5)
    c, q = _dev(c0, torch.float64, plain), _dev(q0, torch.float64, plain)
    p, L = integ.init_momenta()
    integ.run(c, q, p, L, 7)
    assert float((c - outs[0][0]).abs().max()) > 1e-8  # (the forces did act)


def test_two_runs_with_a_closing_launch_in_between_match_the_oracle():
    """run(3); run(4): the closing-only launch of the first run carries the step index of the first launch of the second -
    the stamp's closed / open bit keeps them apart, and both half kicks are applied."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    s = _make(2, top, traj.box_size, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    gam_t, gam_r, seed, inertia = KT / 2.5, KT / 7.5, 31, (1.0, 1.0, 1.0)
    idx, f = _pull(top.n_nucleotides)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=gam_t, gamma_r=gam_r, seed=seed)
    integ.set_external_forces(idx, f)
    c, q = _dev(traj.center[0], torch.float64, s), _dev(traj.quaternions[0], torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    integ.run(c, q, p, L, 3)
    integ.run(c, q, p, L, 4)
    orc = _oracle(2, top, traj.box_size, 0.005, gam_t, gam_r, inertia, seed, idx, f)
    for _ in range(7):
        x, qq, pp, LL, _u = orc.step(x, qq, pp, LL)
    np.testing.assert_allclose(c.cpu().numpy(), x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(q.cpu().numpy(), qq, rtol=0, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=0, atol=1e-9)
    # resident: advance(3); store (closes); advance(4); store - the same two half kicks
    integ2 = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=gam_t, gamma_r=gam_r, seed=seed)
    integ2.set_external_forces(idx, f)
    c2, q2 = _dev(traj.center[0], torch.float64, s), _dev(traj.quaternions[0], torch.float64, s)
    p2, L2 = integ2.init_momenta()
    integ2.load(c2, q2, p2, L2)
    integ2.advance(3)
    integ2.store(c2, q2, p2, L2)
    integ2.advance(4)
    integ2.store(c2, q2, p2, L2)
    # (not bit for bit the two runs: a run packs the state again and renormalises the quaternions, as without forces)
    for got, want, tol in ((c2, x, 1e-10), (q2, qq, 1e-10), (p2, pp, 1e-9), (L2, LL, 1e-9)):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=tol)


def test_a_forced_recovery_applies_every_kick_once():
    """Dynamic list, segments of four launches, the scheduled rebuild in front of launch 8 claims an overflow: the kick
    of launch 8 skips with the launch, the run recovers and resumes there.  Bit for bit the undisturbed run."""
    from mythos_amd.hip_system import LangevinIntegrator

    top, c0, q0 = generators.ideal_duplex(24, model=2, seed=77)
    rng = np.random.default_rng(8)
    c0 = c0 + 0.02 * rng.standard_normal(c0.shape)
    idx, f = _pull(top.n_nucleotides)
    results = []
    for inject in (False, True):
        s = _make(2, top, None, torch.float64, hce=True)
        integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=5)
        integ.set_neighbor_policy(3.3, 0.6, 4)
        integ.set_external_forces(idx, f)
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
    """The crowded blob of test_gpu_edge_cases.py (more than 16 angular neighbours of one nucleotide: the first launch
    aborts and is repeated with the wide work lists) with a force on every nucleotide, the crowded one included.  The kick
    of the aborted launch was applied in place to the frame the repeated launch reads; against the oracle - that test's
    comparison - the momenta are right only if the repeated launch's kick was a no-op.  (dt = 1e-9 and overlapping sites
    that push with 1e13 make momenta of 4e4, so that test's tolerance is 4e-4 on a momentum and 1e-12 on a position; forces
    of 1e9 make a kick of 0.5 per launch: a half kick too many is three digits above the first and, through dt p, two
    above the second.)"""
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
    idx = np.arange(n)
    f = 1e9 * np.random.default_rng(3).uniform(-1.0, 1.0, size=(n, 3))
    integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=12)
    integ.set_external_forces(idx, f)
    c, q = _dev(c0, torch.float64, s), _dev(q0, torch.float64, s)
    p, L = integ.init_momenta()
    x, qq, pp, LL = (t.cpu().numpy().copy() for t in (c, q, p, L))
    tc, tq, et = integ.run(c, q, p, L, 4, save_every=2)
    assert integ.last_recoveries() == 1 and integ.step == 4
    lo = _oracle(2, top, None, dt, KT / 2.5, KT / 7.5, (1.0, 1.0, 1.0), 12, idx, f)
    for k in range(4):
        x, qq, pp, LL, u = lo.step(x, qq, pp, LL)
        if k % 2 == 1:
            np.testing.assert_allclose(tc[k // 2].cpu().numpy(), x, rtol=1e-11, atol=1e-12)
            assert abs(et[k // 2, :8].sum().item() - u) <= 1e-9 * abs(u)
    np.testing.assert_allclose(p.cpu().numpy(), pp, rtol=1e-8, atol=1e-9 * np.abs(pp).max())
    np.testing.assert_allclose(L.cpu().numpy(), LL, rtol=1e-8, atol=1e-9 * np.abs(LL).max())
    kick = 0.5 * dt * np.abs(f).max()  # what the aborted first launch's kick, applied twice, would add
    assert kick > 100 * (1e-8 + 1e-9) * np.abs(pp).max() and dt * kick > 100 * 1e-12


def test_refusals():
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    s = _make(2, top, traj.box_size, torch.float64)
    s.set_neighbors(top.unbonded_neighbors)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=7)
    idx, f = _pull(top.n_nucleotides)
    lib = _lib.load()

    def raw(index, force):
        index = np.ascontiguousarray(index, dtype=np.int32)
        force = np.ascontiguousarray(force, dtype=np.float64)
        return lib.mythos_langevin_set_external_forces(integ._h, int(index.shape[0]), index.ctypes.data_as(_lib.c_int_p), force.ctypes.data_as(_lib.c_double_p))

    assert raw([0, top.n_nucleotides], np.zeros((2, 3))) == -1 and "out of range" in _lib.last_error()
    assert raw([-1], np.zeros((1, 3))) == -1 and "out of range" in _lib.last_error()
    assert raw([4, 2, 4], np.zeros((3, 3))) == -1 and "listed twice" in _lib.last_error()
    assert raw([1], [[0.0, np.nan, 0.0]]) == -1 and "finite" in _lib.last_error()
    # the Python side sums repeats before the call
    integ.set_external_forces([4, 2, 4], [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 2.0]])
    np.testing.assert_array_equal(integ.external_forces[0], [2, 4])
    np.testing.assert_array_equal(integ.external_forces[1], [[0, 1.0, 0], [1.0, 0, 2.0]])
    # valid before load and after store, refused while the frame is open
    c, q = _dev(traj.center[0], torch.float64, s), _dev(traj.quaternions[0], torch.float64, s)
    p, L = integ.init_momenta()
    integ.load(c, q, p, L)
    integ.set_external_forces(idx, f)
    integ.advance(2)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_external_forces(idx, 2 * f)
    with pytest.raises(ValueError, match="frame is open"):
        integ.set_external_forces()
    integ.store(c, q, p, L)
    integ.set_external_forces(idx, 2 * f)
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
    un.set_external_forces([0], [[0.0, 0.0, 0.3]])
    cn, qn = _dev(trajn.center[2], torch.float64, sn), _dev(trajn.quaternions[2], torch.float64, sn)
    pn, Ln = un.init_momenta()
    with pytest.raises(ValueError, match="unfused"):
        un.run(cn, qn, pn, Ln, 2)
    un.set_unfused(False)  # the fused oxNA kernel steps with them
    un.run(cn, qn, pn, Ln, 2)
    assert torch.isfinite(cn).all()


def test_a_pulled_duplex_is_longer():
    """Both parts together, a sign-and-plumbing check (not a modulus): 64 replicas of the 16-nt oxDNA2 helix through
    HipMDSimulator(external_forces=...), 2 x 10^4 steps with +-0.3 per nucleotide pulling the end pairs apart along z, and
    the same at zero force.  The mean ExtensionZ over the saved frames under force exceeds the unforced mean by at least
    five standard errors (the replicas are the blocks)."""
    import dataclasses as dc

    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import Quaternion, RigidBody, space
    from mythos_amd.observables import ExtensionZ
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    n, n_rep = top.n_nucleotides, 64
    assert n == 16
    disp, shift = space.free()
    ef = dna2.create_default_energy_fn(topology=top, displacement_fn=disp)
    dev = torch.device("cuda", 0)
    init = RigidBody(center=torch.as_tensor(traj.center[0], device=dev), orientation=Quaternion(vec=torch.as_tensor(traj.quaternions[0], device=dev)))
    bp1, bp2 = (0, n - 1), (n // 2 - 1, n // 2)
    z1 = float(traj.center[0][list(bp1), 2].mean())
    z2 = float(traj.center[0][list(bp2), 2].mean())
    sign = 1.0 if z1 > z2 else -1.0  # the upper pair is pulled up, the lower one down
    idx = np.array([*bp1, *bp2])
    f = np.array([[0, 0, 0.3 * sign]] * 2 + [[0, 0, -0.3 * sign]] * 2)
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=0.005, kT=KT)
    pulled = HipMDSimulator(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin,
                            neighbors=VerletNeighborList(3.25, 0.6, 20), save_every=200, n_replicas=n_rep, external_forces=(idx, f))
    free = dc.replace(pulled, external_forces=None)
    ext = ExtensionZ(bp1, bp2, disp)
    means = {}
    for name, sim in (("pulled", pulled), ("free", free)):
        out = sim.run({}, init, 20000, key=3).observables[0]
        assert out.center.shape == (n_rep * 100, n, 3) and torch.isfinite(out.center).all()
        per_replica = ext(out).reshape(n_rep, 100)[:, 50:].mean(dim=1)  # replica-major rows; the second half of each run
        means[name] = (float(per_replica.mean()), float(per_replica.std() / np.sqrt(n_rep)))
    _, integ, _ = next(iter(pulled._resident.values()))
    got_idx, got_f = integ.external_forces
    np.testing.assert_array_equal(got_idx, np.sort(np.concatenate([idx + r * n for r in range(n_rep)])))
    order = np.argsort(np.concatenate([idx + r * n for r in range(n_rep)]), kind="stable")
    np.testing.assert_array_equal(got_f, np.tile(f, (n_rep, 1))[order])
    _, integ0, _ = next(iter(free._resident.values()))
    assert integ0.external_forces[0].size == 0
    print("extension: pulled %.4f +- %.4f, free %.4f +- %.4f" % (*means["pulled"], *means["free"]))
    assert means["pulled"][0] - means["free"][0] >= 5.0 * np.hypot(means["pulled"][1], means["free"][1]), means
    pulled.release()
    free.release()


def test_the_simulator_reads_an_external_force_file(tmp_path):
    """``external_forces=path``: read with the replica's number of nucleotides (``particle = -1``), tiled per replica."""
    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import space
    from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList

    top, traj, _, _ = H.load_golden(2, "simple-helix")
    n = top.n_nucleotides
    path = tmp_path / "external.conf"
    path.write_text("{\ntype = string\nparticle = 0, 15\nF0 = 0.2\nrate = 0.\ndir = 0., 0., 2.\n}\n"
                    "{\ntype = string\nparticle = -1\nF0 = 0.01\nrate = 0\ndir = 1, 0, 0\n}\n")
    disp, shift = space.free()
    ef = dna2.create_default_energy_fn(topology=top, displacement_fn=disp)
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=0.005, kT=KT)
    sim = HipMDSimulator(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin,
                         neighbors=VerletNeighborList(3.25, 0.6, 20), save_every=0, n_replicas=3, external_forces=str(path))
    _, integ, _, n_rep, n_one = sim._prepare({}, 0, torch.device("cuda", 0))
    got_idx, got_f = integ.external_forces
    assert (n_rep, n_one) == (3, n)
    np.testing.assert_array_equal(got_idx, np.arange(3 * n))
    one = np.tile([0.01, 0.0, 0.0], (n, 1))
    one[[0, 15], 2] = 0.2
    np.testing.assert_array_equal(got_f, np.tile(one, (3, 1)))
    sim.release()
