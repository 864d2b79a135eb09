"""GPU tests of the MARTINI pressure kernel and barostat (mythos_martini_langevin_pressure / set_barostat / last_boxes).

The reference delegates MARTINI dynamics, pressure coupling included, to GROMACS, so nothing there pins these; the
references are tests/martini_npt_ref.py (the oracle's energies under the affine strain; the oracle integrator stepped from
event to event on the device's noise stream), itself pinned by tests/test_martini_npt_cpu.py.

  1  pressure() against the strain virial of the oracle on the bilayer and on the synthetic systems of
     tests/martini_synth.py (all-pairs builder, direct cells, slab, hashed table, partial workgroups, the hub bead);
     a closed frame is left bitwise unchanged
  2  step-by-step NPT parity in fp64, three modes
  3  split calls equal one call bitwise with a barostat set; a barostat switched off again changes nothing
  4  a laterally stretched bilayer relaxes (Berendsen, fixed height)
  5  volume statistics of stochastic cell rescaling on an ideal gas; a box that would shrink under 2 (r_cut + skin)
"""

import functools

import numpy as np
import pytest
import torch

from tests import martini_helpers as MH
from tests import martini_npt_ref as NR
from tests import martini_synth as S

pytestmark = pytest.mark.gpu

KB = 0.0083144626
T = 273.0
KT = KB * T
SEED = 0xABCDEF012345


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(n, ff = the oracle's force-field arguments (types ... angle_t0), angle_kind, mass, pos, box, skin)."""
    if name == "bilayer":
        s = MH.system()
        x, box, _ = MH.frames("lj")
        top = s["top"]
        ff = (s["types"], s["sigma"], s["eps"], np.asarray(top.bonded_neighbors), s["bond_k"], s["bond_r0"], np.asarray(top.angles),
              s["angle_k"], s["angle_t0"])
        return dict(n=len(s["types"]), ff=ff, angle_kind=0, mass=np.random.default_rng(5).uniform(40.0, 90.0, size=len(s["types"])),
                    pos=x[3].astype(np.float64), box=box[3].astype(np.float64), skin=0.25)
    s = S.get(name)
    S.check(s)
    ff = tuple(s[k] for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0"))
    # md37: the shortest edge is exactly 2 (r_cut + 0.25); the slab runs the harmonic angle, as in test_gpu_martini_shapes.py
    return dict(n=s["n"], ff=ff, angle_kind=1 if name == "slab1285" else 0, mass=s["mass"], pos=s["pos"][0], box=s["box"][0],
                skin={"md37": 0.2, "dilute520": 0.3}.get(name, 0.25))


def _system(c, dtype):
    from mythos_amd.hip_system import MartiniSystem

    return MartiniSystem(*c["ff"], angle_kind=c["angle_kind"], dtype=dtype)


def _integrator(c, sysm, *, dt=0.01, gamma=2.0, every=2, seed=SEED, skin=None):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=dt, kT=KT, gamma=gamma, mass=c["mass"], seed=seed)
    integ.set_neighbor_policy(c["skin"] if skin is None else skin, every)
    return integ


def _dev(a, sysm):
    return torch.tensor(np.asarray(a), dtype=sysm.dtype, device=sysm.device).contiguous()


@functools.lru_cache(maxsize=None)
def _reference_virial(name, fp32):
    """W of the oracle at the loaded frame (fp32: of the fp32-rounded positions, box and tables) - once, read-only."""
    c = _case(name)
    r = (lambda a: np.asarray(a).astype(np.float32).astype(np.float64)) if fp32 else (lambda a: np.asarray(a, dtype=np.float64))
    t, sg, ep, b, bk, br, an, ak, at = c["ff"]
    w = NR.strain_virial(r(c["pos"]), r(c["box"]), t, r(sg), r(ep), b, r(bk), r(br), an, r(ak), r(at), c["angle_kind"] == 0)
    w.setflags(write=False)
    return w


PRESSURE_SYSTEMS = ["bilayer", "md37", "md1285", "slab1285", "dilute520"]
# fp32: |W_gpu - W_oracle| / max |W_oracle| measured on an MI355X: bilayer 5.5e-7, md37 4.7e-6, md1285 3.0e-7, slab1285
# 2.8e-7, dilute520 1.6e-6 (fp64: 2e-16 ... 4e-15).  The bound is four times the largest, for another reduction order
# after a rebuild.
FP32_MEASURED = 4.7e-6


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", PRESSURE_SYSTEMS)
def test_pressure_kernel_against_the_oracle(name, dtype):
    """pressure() after load, velocities drawn at 273 K: K = sum m v^2 per axis, W = -dU/ds of the oracle's energies at
    pos * s, box * s, P = (K + W) / V x 16.6053907.  fp64: 1e-10 of max |W| (fp64 sums of ~1e5 terms; the energy
    comparison of test_gpu_martini_md.py holds the same).  fp32: 4 x FP32_MEASURED.  The kinetic part is a double sum of
    the stored velocities with m = 1 / (stored inverse mass): 1e-12 in fp64, 2^-22 in fp32 (the inverse mass rounded)."""
    c = _case(name)
    f64 = dtype == torch.float64
    sysm = _system(c, dtype)
    integ = _integrator(c, sysm)
    pos = _dev(c["pos"], sysm)
    vel = integ.init_velocities()
    integ.load(pos, vel, c["box"])
    out = integ.pressure()
    w_ref = _reference_virial(name, not f64)
    v = vel.cpu().numpy().astype(np.float64)
    k_ref = NR.kinetic_diag(c["mass"], v)
    vol = float(np.prod(c["box"]))
    err_w = np.abs(out["virial"] - w_ref).max() / np.abs(w_ref).max()
    err_k = np.abs(out["kinetic"] - k_ref).max() / k_ref.max()
    print(f"  {name} {'f64' if f64 else 'f32'}: W {out['virial']} (oracle {w_ref}), rel. error {err_w:.3e}; K {out['kinetic']}, rel. error "
          f"{err_k:.3e}; P {out['pressure']} bar, N kT / V {c['n'] * KT / vol * NR.BAR:.2f} bar")
    assert err_w <= (1e-10 if f64 else 4.0 * FP32_MEASURED)
    assert err_k <= (1e-12 if f64 else 2.0**-22)
    assert out["volume"] == pytest.approx(vol, rel=1e-15)
    p_ref = (out["kinetic"] + out["virial"]) / vol * NR.BAR
    np.testing.assert_allclose(out["pressure"], p_ref, rtol=1e-14, atol=1e-14 * np.abs(p_ref).max())
    assert out["p"] == pytest.approx(out["pressure"].mean())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_pressure_leaves_a_closed_frame_bitwise_and_closes_an_open_one(dtype):
    """Bilayer, dt -> 0 (the pattern of test_verlet_list_forces_equal_all_pairs_energy_kernel): pressure() on the loaded,
    closed frame changes no bit of positions or velocities; on an open frame (after advance) it supplies the closing half
    kick that store would, and twice in a row gives the same numbers."""
    c = _case("bilayer")
    sysm = _system(c, dtype)
    integ = _integrator(c, sysm, dt=1e-9, gamma=0.0, seed=1)
    pos = _dev(c["pos"], sysm)
    vel = integ.init_velocities()
    integ.load(pos, vel, c["box"])
    integ.pressure()
    p2, v2 = torch.empty_like(pos), torch.empty_like(vel)
    integ.store(p2, v2)
    assert torch.equal(p2, pos) and torch.equal(v2, vel)

    a, b = _integrator(c, sysm, dt=0.01), _integrator(c, sysm, dt=0.01)
    for integ in (a, b):
        integ.load(pos, vel, c["box"])
        integ.advance(3)
    first, second = a.pressure(), a.pressure()
    assert all(np.array_equal(first[k], second[k]) for k in ("kinetic", "virial", "pressure"))
    pa, va, pb, vb = (torch.empty_like(pos) for _ in range(4))
    a.store(pa, va)
    b.store(pb, vb)
    assert torch.equal(pa, pb) and torch.equal(va, vb)
    np.testing.assert_array_equal(a.box, c["box"])


NPT_MODES = {
    "berendsen-semi-zfixed": dict(kind="berendsen", coupling="semiisotropic", compressibility=(3e-4, 0.0)),
    "crescale-semi": dict(kind="c-rescale", coupling="semiisotropic", compressibility=(3e-4, 3e-4)),
    "crescale-iso": dict(kind="c-rescale", coupling="isotropic", compressibility=3e-4),
}


@pytest.mark.parametrize("mode", list(NPT_MODES))
def test_step_by_step_npt_parity_with_oracle_fp64(mode):
    """Bilayer, dt 0.01, gamma 2, masses 40 ... 90, list policy (0.25, 2); coupling every 2 steps with tau_p 0.1 and
    compressibility 3e-4 (|mu - 1| ~ 1e-3 per event), 6 steps = 3 events, rows every 2 steps.  Positions, velocities, box
    and last_boxes against the NPT oracle to 1e-9 nm, nm/ps: ten times the 1e-10 of the NVT parity over 5 steps, for the
    reduction order of the pressure sum entering mu."""
    c = _case("bilayer")
    m = NPT_MODES[mode]
    sysm = _system(c, torch.float64)
    integ = _integrator(c, sysm)
    baro = dict(ref_p=(1.0, 1.0), tau_p=0.1, every=2, **m)
    integ.set_barostat(**baro)
    pos = _dev(c["pos"], sysm)
    vel = integ.init_velocities()
    x, v = c["pos"].copy(), vel.cpu().numpy().copy()
    integ.load(pos, vel, c["box"])
    traj, _ = integ.advance(6, save_every=2)
    boxes = integ.last_boxes
    integ.store(pos, vel)
    orc = NR.NptOracle(c["ff"], True, c["box"], 0.01, KT, 2.0, c["mass"], SEED, m["kind"], m["coupling"], (1.0, 1.0),
                       m["compressibility"], 0.1, 2)
    rows_ref, boxes_ref = orc.run(x, v, 6, save_every=2)
    mus = np.array([e[2] for e in orc.events])
    print(f"  {mode}: events at {[e[0] for e in orc.events]}, mu - 1 {(mus - 1).tolist()}, box {integ.box} (oracle {orc.box}); "
          f"|dx| {np.abs(pos.cpu().numpy() - x).max():.2e} |dv| {np.abs(vel.cpu().numpy() - v).max():.2e} "
          f"|dbox| {np.abs(integ.box - orc.box).max():.2e}")
    assert len(orc.events) == 3 and np.abs(mus - 1).max() > 1e-5  # the scaling is visible
    np.testing.assert_allclose(pos.cpu().numpy(), x, rtol=0, atol=1e-9)
    np.testing.assert_allclose(vel.cpu().numpy(), v, rtol=0, atol=1e-9)
    np.testing.assert_allclose(integ.box, orc.box, rtol=0, atol=1e-9)
    assert boxes.shape == (3, 3) and boxes.dtype == torch.float64 and boxes.device == sysm.device
    np.testing.assert_allclose(boxes.cpu().numpy(), boxes_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(traj.cpu().numpy(), rows_ref, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(boxes[0].cpu().numpy(), c["box"])  # the row of step 2 is the state before its event
    if m["coupling"] == "semiisotropic" and m["compressibility"][1] == 0.0:
        assert integ.box[2] == c["box"][2] and (boxes[:, 2].cpu().numpy() == c["box"][2]).all()  # bitwise the input's
    assert integ.step == 6


def _npt_run(c, sysm, calls, save_every, want_energy, baro, n_policy=(0.3, 3)):
    """load; advance(n) for n in calls; store -> (pos, vel, box, {absolute step: (row, box row, energy row)})."""
    integ = _integrator(c, sysm, dt=0.02, gamma=1.0, every=n_policy[1], skin=n_policy[0], seed=2)
    for b in baro:
        integ.set_barostat(**b)
    pos = _dev(c["pos"], sysm)
    vel = _integrator(c, sysm, seed=2).init_velocities()
    integ.load(pos, vel, c["box"])
    rows, at = {}, 0
    for n in calls:
        traj, et = integ.advance(n, save_every=save_every, want_energy=want_energy)
        lb = integ.last_boxes
        assert lb.shape[0] == (n // save_every if save_every else 0)
        for r in range(lb.shape[0]):
            rows[at + (r + 1) * save_every] = (traj[r].cpu(), lb[r].cpu(), et[r].cpu() if et is not None else None)
        at += n
    integ.store(pos, vel)
    return pos.cpu(), vel.cpu(), integ.box, rows


CRESCALE = dict(kind="c-rescale", coupling="semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 3e-4), tau_p=0.5, every=4)


@pytest.mark.parametrize("want_energy", [True, False], ids=["energy-rows", "plain-rows"])
@pytest.mark.parametrize("save_every", [4, 2])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_split_calls_equal_one_call_bitwise_with_a_barostat(dtype, save_every, want_energy):
    """advance(5); advance(7); advance(12) against advance(24), coupling every 4 steps (events on the integrator's step
    counter, each one dropping the list), list rebuilds every 3: positions, velocities and box bitwise, and so is every
    saved row - positions, box, energies - that the two sequences save at the same step (rows count from the first step
    of their call, as without a barostat: steps 4, 16, 20, 24 at save_every 4)."""
    c = _case("bilayer")
    sysm = _system(c, dtype)
    one = _npt_run(c, sysm, [24], save_every, want_energy, [CRESCALE])
    split = _npt_run(c, sysm, [5, 7, 12], save_every, want_energy, [CRESCALE])
    assert torch.equal(one[0], split[0]) and torch.equal(one[1], split[1])
    np.testing.assert_array_equal(one[2], split[2])
    assert (one[2] != c["box"]).all()  # six events have happened
    shared = sorted(set(one[3]) & set(split[3]))
    assert set(shared) >= {4, 16, 20, 24}
    for s in shared:
        for a, b in zip(one[3][s], split[3][s]):
            assert (a is None and b is None) or torch.equal(a, b), s


def test_a_barostat_switched_off_changes_nothing_and_any_cadence_of_rows_is_served():
    """fp32 bilayer, 12 steps with rows every 4: never set, set and switched off again (kind None), and compressibility
    (0, 0) give the same bits, rows and energies included, and last_boxes is the loaded box on every row.  No combination
    of save_every and every is refused: rows every 3 steps with events every 4 are rows 3, 6, 9, 12 of the run that saves every step.
    Arguments that make no sense are refused with a message."""
    c = _case("bilayer")
    sysm = _system(c, torch.float32)
    never = _npt_run(c, sysm, [12], 4, True, [])
    off = _npt_run(c, sysm, [12], 4, True, [CRESCALE, dict(kind=None)])
    zero = _npt_run(c, sysm, [12], 4, True, [dict(CRESCALE, compressibility=(0.0, 0.0))])
    for other in (off, zero):
        assert torch.equal(never[0], other[0]) and torch.equal(never[1], other[1])
        np.testing.assert_array_equal(other[2], c["box"])
        for s in (4, 8, 12):
            assert all(torch.equal(a, b) for a, b in zip(never[3][s], other[3][s]))
            np.testing.assert_array_equal(other[3][s][1].numpy(), c["box"])
    every1 = _npt_run(c, sysm, [12], 1, False, [CRESCALE])
    every3 = _npt_run(c, sysm, [12], 3, False, [CRESCALE])
    assert torch.equal(every1[0], every3[0]) and torch.equal(every1[1], every3[1])
    for s in (3, 6, 9, 12):
        assert torch.equal(every1[3][s][0], every3[3][s][0]) and torch.equal(every1[3][s][1], every3[3][s][1])
    integ = _integrator(c, sysm)
    with pytest.raises(ValueError, match="tau_p > 0"):
        integ.set_barostat("berendsen", tau_p=0.0)
    with pytest.raises(ValueError, match="every >= 1"):
        integ.set_barostat("c-rescale", every=0)
    with pytest.raises(ValueError, match="kind must be"):
        integ.set_barostat("parrinello-rahman")
    with pytest.raises(Exception, match="no resident state"):
        integ.pressure()


def test_a_stretched_bilayer_relaxes_under_berendsen_coupling_fp32():
    """Lateral edges and positions stretched by 1.03; Berendsen, semi-isotropic, beta_z = 0, P0 = 1 bar, tau_p = 1 ps, an event
    every 10 steps, dt 0.02, gamma 1, 4 000 steps: the area falls from block to block of 1 000 steps or ends below its start,
    the height keeps its bits, the kinetic temperature of the second half is within 2 % of T (the bound of
    test_thermostat_holds_the_temperature_fp32).  No pressure is asserted: 1 280 beads fluctuate by hundreds of bar."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    c = _case("bilayer")
    sysm = _system(c, torch.float32)
    stretch = np.array([1.03, 1.03, 1.0])
    b0 = c["box"] * stretch
    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=KT, gamma=1.0, seed=11)
    integ.set_neighbor_policy(0.3, 5)
    integ.set_barostat("berendsen", "semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 0.0), tau_p=1.0, every=10)
    pos = _dev(c["pos"] * stretch, sysm)
    vel = integ.init_velocities()
    integ.load(pos, vel, b0)
    traj, et = integ.advance(4000, save_every=10)
    boxes = integ.last_boxes.cpu().numpy()
    area = boxes[:, 0] * boxes[:, 1]
    blocks = area.reshape(4, 100).mean(1)
    t_kin = 2.0 * et[200:, 3].cpu().numpy() / (3.0 * sysm.n * KB)
    print(f"  area {b0[0] * b0[1]:.3f} -> block means {blocks} nm^2, final box {integ.box}; T_kin {t_kin.mean():.1f} K; "
          f"recoveries {integ.last_recoveries()}")
    assert (np.diff(blocks) < 0).all() or blocks[-1] < b0[0] * b0[1]
    assert (boxes[:, 2] == b0[2]).all() and integ.box[2] == b0[2]
    assert abs(t_kin.mean() / T - 1.0) < 0.02
    integ.store(pos, vel)
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all()
    # the README's route: saved rows + last_boxes -> SimulatorTrajectory -> AreaPerLipid (angstrom^2, two leaflets of 64 lipids)
    from mythos_amd.energy.base import Quaternion
    from mythos_amd.observables import AreaPerLipid
    from mythos_amd.simulators.io import SimulatorTrajectory

    q = torch.zeros((5, sysm.n, 4), dtype=traj.dtype, device=traj.device)
    q[..., 0] = 1.0
    st = SimulatorTrajectory(center=traj[-5:], orientation=Quaternion(vec=q), box_size=integ.last_boxes[-5:])
    apl = AreaPerLipid(topology=MH.system()["top"], lipid_sel="name GL1 GL2")(st).cpu().numpy()
    print(f"  area per lipid of the last five rows {apl} A^2; box area / 64 {100.0 * area[-5:] / 64}")
    assert apl.shape == (5,) and np.isfinite(apl).all()
    np.testing.assert_allclose(apl, 100.0 * area[-5:] / 64, rtol=0.1)


IDEAL_N, IDEAL_KT, IDEAL_EDGE = 64, 2.27, 4.0
IDEAL_RANGE = (1.1, 0.1)  # r_cut, skin: the box needs edges above 2.4 nm
IDEAL_RANGE_TINY = (0.005, 0.01)  # ... above 0.03 nm


def _ideal_gas(coupling, beta_z_on=True, p0_factor=1.0, list_range=IDEAL_RANGE):
    """64 beads without interactions (LJ epsilon 0, no bonds, no angles), mass 72, kT 2.27, gamma 1, dt 0.02, in 4 x 4 x 4 nm;
    c-rescale at every step with P0 = 64 kT / 64 nm^3 (37.69 bar) and f P0 = 0.05: tau_p = 1 ps, beta = 0.05 / (P0 dt).
    Without interactions the cut-off is a free parameter: ``list_range`` = (r_cut, skin)."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator, MartiniSystem

    z = np.zeros(0)
    sysm = MartiniSystem(np.zeros(IDEAL_N, dtype=np.int32), np.array([[0.47]]), np.array([[0.0]]), np.zeros((0, 2), np.int32), z, z,
                         np.zeros((0, 3), np.int32), z, z, r_cut=list_range[0], dtype=torch.float64)
    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=IDEAL_KT, gamma=1.0, seed=77)
    integ.set_neighbor_policy(list_range[1], 10)
    p0 = IDEAL_N * IDEAL_KT / IDEAL_EDGE**3 * NR.BAR
    beta = 0.05 / (p0 * 0.02)
    integ.set_barostat("c-rescale", coupling, ref_p=p0 * p0_factor, compressibility=(beta, beta if beta_z_on else 0.0), tau_p=1.0, every=1)
    pos = torch.tensor(np.random.default_rng(3).uniform(0.0, IDEAL_EDGE, size=(IDEAL_N, 3)), dtype=torch.float64, device=sysm.device)
    vel = integ.init_velocities()
    integ.load(pos, vel, [IDEAL_EDGE] * 3)
    return sysm, integ, pos, vel


@pytest.mark.parametrize("coupling,beta_z_on", [("isotropic", True), ("semiisotropic", False), ("semiisotropic", True)],
                         ids=["iso", "semi-z-fixed", "semi"])
def test_ideal_gas_volume_statistics_of_stochastic_cell_rescaling(coupling, beta_z_on):
    """20 000 steps in fp64, V after every step, the first tenth dropped: |<V> - 65 kT / P0| <= 4 SE (50 block means) and
    0.75 <= Var V / <V>^2 x 65 <= 1.35 - the bounds tests/test_martini_npt_cpu.py holds the NumPy restatement to; a noise
    amplitude wrong by sqrt(2) puts the ratio near 0.5 or 2.
    Five standard deviations of V under its mean are edges of 2.9 nm (isotropic) and 2.5 nm (lateral, at the fixed height
    of 4 nm): those two runs also hold the box above 2.7 / 2.4 nm.  With both compressibilities set the SHAPE of an ideal
    gas's box has no restoring force - ln (L_z / L_xy) is a free random walk of 0.028 per event, 3.9 after 20 000 - and
    edges between 0.1 and 90 nm occur in the NumPy restatement.  The volume statistics do not care; that run takes a cut-off
    of 0.005 nm and a skin of 0.01 nm (an ideal gas has no interaction range), so its box may wander down to 0.03 nm."""
    free_shape = coupling == "semiisotropic" and beta_z_on
    list_range = IDEAL_RANGE_TINY if free_shape else IDEAL_RANGE
    sysm, integ, pos, vel = _ideal_gas(coupling, beta_z_on, list_range=list_range)
    integ.advance(20_000, save_every=1, want_energy=False)
    boxes = integ.last_boxes.cpu().numpy()
    assert boxes.shape == (20_000, 3)
    z, ratio = NR.volume_statistics(boxes.prod(1), IDEAL_N, IDEAL_KT, IDEAL_N * IDEAL_KT / IDEAL_EDGE**3)
    print(f"  {coupling} beta_z {'on' if beta_z_on else 'off'}: <V> {boxes[2000:].prod(1).mean():.2f} nm^3 of 65, z {z:+.2f}, "
          f"ratio {ratio:.3f}, smallest edge {boxes.min():.2f} nm")
    assert abs(z) <= 4.0
    assert 0.75 <= ratio <= 1.35
    assert boxes.min() > (2.0 * sum(list_range) if free_shape else (2.7 if coupling == "isotropic" else 2.4))
    if not beta_z_on:
        assert (boxes[:, 2] == IDEAL_EDGE).all()
    integ.store(pos, vel)
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all()


def test_a_box_that_would_shrink_under_the_minimum_image_ends_the_call_with_the_last_state_resident():
    """P0 a thousand times larger: ln mu = -50 / 3 at the first event.  The call ends with the error of a box too small,
    neither a NaN nor a hang; the state of that step - unscaled, in the box it had - stays resident and can be stored."""
    sysm, integ, pos, vel = _ideal_gas("isotropic", p0_factor=1000.0)
    with pytest.raises(ValueError, match=r"box smaller than twice \(r_cut \+ skin\)"):
        integ.advance(50, save_every=1, want_energy=False)
    assert integ.step == 1
    np.testing.assert_array_equal(integ.box, [IDEAL_EDGE] * 3)
    p1, v1 = torch.empty_like(pos), torch.empty_like(vel)
    integ.store(p1, v1)
    assert torch.isfinite(p1).all() and torch.isfinite(v1).all()
    assert 0 < (p1 - pos).abs().max() < 0.1  # one step of 0.02 ps
    integ.set_barostat(None)
    integ.advance(5)
    assert integ.step == 6
