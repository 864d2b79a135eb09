"""GPU tests of the lateral pressure profile of stored MARTINI frames (mythos_amd/csrc/stress_profile.hip,
MartiniSystem.stress_profile, observables.StressProfile / SurfaceTension) against tests/stress_profile_ref.py, which
tests/test_stress_profile_cpu.py pins.  The reference gets the values the kernels get: for an fp32 system every real rounded
to fp32 and widened back.  No bead of a test system lies within 1e-6 slab thicknesses of a slab edge (asserted by
``stress_profile_ref.case``), so slab counts are compared exactly.

Bounds.  fp64: 1e-10 of the frame's max |W_d| of the term (the project's NPT bound).  fp32: |W_gpu - W_ref| over the frame's
max |W_d| of the term was measured on an MI355X over the cases of section a (FP32_MEASURED, the largest by term below); the
bound is four times the largest, as tests/test_gpu_martini_npt.py sets its own.
"""

import functools
import types

import numpy as np
import pytest
import torch

from tests import martini_helpers as MH
from tests import stress_profile_ref as SR

pytestmark = pytest.mark.gpu

KB = 0.0083144626
KT = KB * 300.0
# measured on an MI355X, section a, largest over cases, slab counts, centrings, frames and slabs: lj 3.8e-6 (q259), bond 1.4e-6
# (q259), angle 2.2e-5 (n131, whose angle shares nearly cancel: max |W_d| of the term is 1.9 kJ/mol), coulomb 1.1e-6 (q259);
# fp64: lj 3.5e-15, bond 1.7e-15, angle 2.8e-14, coulomb 2.4e-15
FP32_MEASURED = 2.2e-5
TOL = {torch.float64: 1e-10, torch.float32: 4.0 * FP32_MEASURED}
RAW_CASES = ["n131", "n259", "slab259", "q259"]
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


@functools.lru_cache(maxsize=None)
def _promoted(name, fp32):
    return SR.promoted(_bilayer_case() if name == "bilayer" else SR.case(name), fp32)


@functools.lru_cache(maxsize=None)
def _bilayer_case():
    s = MH.system()
    x, box, _ = MH.frames("lj")
    top = s["top"]
    ff = (s["types"], s["sigma"], s["eps"], np.asarray(top.bonded_neighbors), s["bond_k"], s["bond_r0"], np.asarray(top.angles),
          s["angle_k"], s["angle_t0"])
    center = np.flatnonzero(np.isin(np.asarray(top.atom_names), ["C3A", "C3B"])).astype(np.int32)
    return dict(n=len(s["types"]), ff=ff, angle_kind=0, pos=x[3:6].astype(np.float64), box=box[3:6].astype(np.float64), charges=None,
                center=center)


@functools.lru_cache(maxsize=None)
def _ref(name, fp32, n_bins, centered):
    """(F, n_bins, 13) reference rows - once, read-only."""
    r = SR.reference_rows(_promoted(name, fp32), n_bins, centered=centered)
    r.setflags(write=False)
    return r


def _system(c, dtype):
    from mythos_amd.hip_system import MartiniSystem

    s = MartiniSystem(*c["ff"], angle_kind=c["angle_kind"], dtype=dtype)
    if c["charges"] is not None:
        s.set_charges(c["charges"])
    return s


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


def _scales(ref):
    """(F, 4): the frame's max |W_d| of every term (of the sum over slabs)."""
    return np.abs(ref[:, :, 1:].sum(1).reshape(ref.shape[0], 4, 3)).max(-1)


def _deviation(raw, ref):
    """-> (4,) largest |W_gpu - W_ref| / the frame's max |W_d|, per term; a term that is zero in the reference must be zero."""
    f, nb = ref.shape[:2]
    d = np.abs(raw[:, :, 1:] - ref[:, :, 1:]).reshape(f, nb, 4, 3).max(-1).max(1)  # (F, 4)
    sc = _scales(ref)
    assert not d[sc == 0.0].any()
    return np.where(sc > 0.0, d / np.where(sc > 0.0, sc, 1.0), 0.0).max(0)


# ---- a. raw rows against the reference ------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_rows_against_the_reference_per_slab_and_term(name, dtype):
    """Three frames with their own boxes in one call, n_bins in {1, 7, 64, 65, 200} (200 > n for n131), fixed to the box and
    centred, by_term: counts exact, W per slab and term within TOL of the frame's max |W_d| of the term; the un-split call
    is ((lj + bond) + angle) + coulomb of those columns, bitwise.  An uncharged system has zero Coulomb columns."""
    fp32 = dtype == torch.float32
    c = _promoted(name, fp32)
    sysm = _system(c, dtype)
    pos, box = _dev(c["pos"], dtype), _dev(c["box"], dtype)
    worst = np.zeros(4)
    for centered in (False, True):
        for nb in SR.N_BINS:
            ci = c["center"] if centered else None
            by = sysm.stress_profile(pos, box, nb, center_index=ci, by_term=True)
            assert by.shape == (3, nb, 13) and by.dtype == torch.float64 and by.is_cuda
            raw, ref = by.cpu().numpy(), _ref(name, fp32, nb, centered)
            assert np.array_equal(raw[:, :, 0], ref[:, :, 0]) and (raw[:, :, 0].sum(1) == c["n"]).all()
            worst = np.maximum(worst, _deviation(raw, ref))
            if c["charges"] is None:
                assert not raw[:, :, 10:].any()
            row = sysm.stress_profile(pos, box, nb, center_index=ci)
            assert row.shape == (3, nb, 4)
            w = by[:, :, 1:].reshape(3, nb, 4, 3)
            assert torch.equal(row[:, :, 1:], ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]) and torch.equal(row[:, :, 0], by[:, :, 0])
    print(f"  {name} {'f32' if fp32 else 'f64'}: largest deviation over the frame's max |W_d|, lj bond angle coulomb: {worst}")
    assert (worst <= TOL[dtype]).all()


# ---- b. the sum over slabs is the integrator's virial ------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", ["bilayer", "q259"])
def test_the_sum_over_slabs_is_the_virial_of_the_pressure_kernel(name, dtype):
    """Frame 0 loaded into a MartiniLangevinIntegrator of the same system: pressure()'s W against the slab sums of the same
    frame, 17 slabs centred, within TOL of max |W| - the bounds of section a.  Measured on an MI355X: 2e-16 in fp64; 1.7e-7
    (bilayer) and 6.2e-8 (q259) in fp32."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    c = _promoted(name, dtype == torch.float32)
    sysm = _system(c, dtype)
    integ = MartiniLangevinIntegrator(sysm, dt=0.01, kT=KT, gamma=2.0, seed=3)
    integ.set_neighbor_policy(0.25, 2)
    pos = _dev(c["pos"][0], dtype)
    integ.load(pos, integ.init_velocities(), c["box"][0])
    w_int = integ.pressure()["virial"]
    raw = sysm.stress_profile(pos, _dev(c["box"][0], dtype), 17, center_index=c["center"]).cpu().numpy()[0]
    w = raw[:, 1:].sum(0)
    err = np.abs(w - w_int).max() / np.abs(w_int).max()
    print(f"  {name}: slab sums {w}, pressure() {w_int}, rel. difference {err:.3e}")
    assert raw[:, 0].sum() == c["n"] and err <= TOL[dtype]


def _bilayer_energy_fn(**over):
    from mythos_amd.energy import martini as M

    s = MH.system()
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    fn = M.MartiniComposedEnergyFunction([
        M.LJ.from_topology(topology=s["top"], params=M.LJConfiguration(**s["lj_params"])),
        M.Bond.from_topology(topology=s["top"], params=M.BondConfiguration(**s["bond_params"])),
        M.Angle.from_topology(topology=s["top"], params=M.AngleConfiguration(**ap))])
    return fn.with_params(**over) if over else fn


def _bilayer_traj(dtype, frames=slice(0, 3), **extra):
    c = _bilayer_case()
    return types.SimpleNamespace(center=_dev(c["pos"][frames], dtype), box_size=_dev(c["box"][frames], torch.float64), **extra)


@DTYPES
def test_total_and_surface_tension_are_those_of_the_integrators_pressure(dtype):
    """Bilayer: .total() is pressure()'s P with K replaced by n kT, SurfaceTension is Lz (P_zz - 1/2 (P_xx + P_yy)) of those
    totals, both within TOL of max |W| as a pressure (the bounds of section a); the slab count and the centring do not enter."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator
    from mythos_amd.observables import StressProfile, SurfaceTension

    s, c = MH.system(), _promoted("bilayer", dtype == torch.float32)
    fn = _bilayer_energy_fn()
    traj = _bilayer_traj(dtype, slice(0, 1), temperature=torch.full((1,), KT, dtype=torch.float64))
    sysm = _system(c, dtype)
    integ = MartiniLangevinIntegrator(sysm, dt=0.01, kT=KT, gamma=2.0, seed=3)
    integ.set_neighbor_policy(0.25, 2)
    integ.load(traj.center[0].clone(), integ.init_velocities(), c["box"][0])
    out = integ.pressure()
    p_ref = (c["n"] * KT + out["virial"]) / out["volume"] * SR.BAR
    tol = TOL[dtype] * np.abs(out["virial"]).max() / out["volume"] * SR.BAR
    for nb, center in ((1, None), (40, "name C3A C3B"), (33, None)):
        sp = StressProfile(topology=s["top"], energy_fn=fn, n_bins=nb, center=center)
        total = sp.total(traj).cpu().numpy()
        assert total.shape == (1, 3) and np.abs(total[0] - p_ref).max() <= tol
        gamma = float(SurfaceTension(topology=s["top"], energy_fn=fn)(traj)[0])
        lat = sp.lateral(traj)
        assert gamma == pytest.approx(c["box"][0, 2] * (p_ref[2] - 0.5 * (p_ref[0] + p_ref[1])), abs=tol * c["box"][0, 2])
        assert float(lat.sum()) * c["box"][0, 2] / nb == pytest.approx(gamma, abs=1e-9 * abs(gamma) + 1e-9)
    print(f"  bilayer: P {p_ref} bar, gamma {gamma:.3f} bar nm = {gamma * 0.1:.3f} mN/m")


# ---- c. one slab is the total ---------------------------------------------------------------------------------------------

def test_one_slab_reproduces_the_total_and_the_terms_add_up_bitwise():
    """n_bins = 1 holds every bead and the frame's W; finer profiles sum to it to rounding.  The un-split row is the by_term
    columns added as ((lj + bond) + angle) + coulomb: bitwise (asserted for every case in section a, here for one slab)."""
    c = _promoted("q259", False)
    sysm = _system(c, torch.float64)
    pos, box = _dev(c["pos"], torch.float64), _dev(c["box"], torch.float64)
    one = sysm.stress_profile(pos, box, 1, by_term=True)
    assert (one[:, 0, 0] == c["n"]).all()
    ref = _ref("q259", False, 1, False)
    assert (_deviation(one.cpu().numpy(), ref) <= 1e-10).all()
    w1 = one[:, 0, 1:].reshape(3, 4, 3)
    assert torch.equal(sysm.stress_profile(pos, box, 1)[:, 0, 1:], ((w1[:, 0] + w1[:, 1]) + w1[:, 2]) + w1[:, 3])
    for nb in (7, 200):
        fine = sysm.stress_profile(pos, box, nb, center_index=c["center"], by_term=True)
        assert torch.allclose(fine[:, :, 1:].sum(1), one[:, 0, 1:], rtol=0, atol=1e-10 * float(one[:, 0, 1:].abs().max()))
        assert torch.equal(fine[:, :, 0].sum(1), one[:, 0, 0])


# ---- d. reproducibility -----------------------------------------------------------------------------------------------------

@DTYPES
def test_a_frames_row_has_the_same_bits_alone_in_a_batch_and_call_after_call(dtype):
    c = _promoted("q259", dtype == torch.float32)
    sysm = _system(c, dtype)
    pos, box = _dev(c["pos"], dtype), _dev(c["box"], dtype)
    kw = dict(center_index=c["center"], by_term=True)
    batch = sysm.stress_profile(pos, box, 65, **kw)
    assert torch.equal(batch, sysm.stress_profile(pos, box, 65, **kw))  # call after call
    alone = sysm.stress_profile(pos[1:2].contiguous(), box[1:2].contiguous(), 65, **kw)
    assert torch.equal(alone[0], batch[1])  # alone and as row 2 of 3
    swapped = sysm.stress_profile(pos.flip(0).contiguous(), box.flip(0).contiguous(), 65, **kw)
    assert torch.equal(swapped.flip(0), batch)


def test_a_frames_row_has_the_same_bits_on_either_side_of_a_launch_chunk():
    """61 beads, 65 537 frames: the launch takes 65 535 frames (grid.z), so frames 65 534 and 65 535 are the last of the
    first and the first of the second chunk, frame 65 536 the last of the call."""
    c = _promoted("n61", False)
    sysm = _system(c, torch.float64)
    pos3, box3 = _dev(c["pos"], torch.float64), _dev(c["box"], torch.float64)
    nf = 65537
    idx = torch.arange(nf, device="cuda") % 3
    out = sysm.stress_profile(pos3[idx].contiguous(), box3[idx].contiguous(), 7, center_index=c["center"])
    three = sysm.stress_profile(pos3, box3, 7, center_index=c["center"])
    ref = _ref("n61", False, 7, True)
    assert np.array_equal(three.cpu().numpy()[:, :, 0], ref[:, :, 0])
    for f in (0, 1, 2, 65533, 65534, 65535, 65536):
        assert torch.equal(out[f], three[f % 3]), f
    assert torch.equal(out[:65535].reshape(21845, 3, 7, 4), three[None].expand(21845, -1, -1, -1))


def test_an_fp32_trajectory_lands_in_the_slabs_of_the_fp64_call_on_the_same_values():
    """Counts, and with them every bead's slab, are bitwise those of the fp64 system on the widened fp32 values; W is summed in
    fp32 inside a bead's tile of partners and differs within the fp32 bound of section a."""
    c32, c = _promoted("n259", True), SR.case("n259")
    s32, s64 = _system(c32, torch.float32), _system(c32, torch.float64)
    p32, b32 = _dev(c["pos"], torch.float32), _dev(c["box"], torch.float32)
    for nb, ci in ((64, None), (65, c["center"]), (200, c["center"])):
        r32 = s32.stress_profile(p32, b32, nb, center_index=ci, by_term=True)
        r64 = s64.stress_profile(p32.double(), b32.double(), nb, center_index=ci, by_term=True)
        assert torch.equal(r32[:, :, 0], r64[:, :, 0])
        # (both calls have one reference - the fp32 values widened - and each its own bound against it)
        assert (_deviation(r32.cpu().numpy(), r64.cpu().numpy()) <= TOL[torch.float32] + TOL[torch.float64]).all()


# ---- e. symmetries --------------------------------------------------------------------------------------------------------

def test_shifting_z_by_whole_slabs_rolls_the_box_fixed_profile_and_leaves_the_centred_one():
    c = _promoted("n259", False)
    sysm = _system(c, torch.float64)
    nb, k = 64, 5
    pos, box = _dev(c["pos"], torch.float64), _dev(c["box"], torch.float64)
    shifted = pos.clone()
    shifted[:, :, 2] += (k * box[:, 2] / nb)[:, None]
    base = sysm.stress_profile(pos, box, nb, by_term=True)
    moved = sysm.stress_profile(shifted, box, nb, by_term=True)
    tol = 1e-10 * float(base[:, :, 1:].sum(1).abs().max())
    assert torch.equal(moved[:, :, 0], base[:, :, 0].roll(k, dims=1))
    assert float((moved[:, :, 1:] - base[:, :, 1:].roll(k, dims=1)).abs().max()) <= tol
    shifted[:, :, 2] += 0.3217  # (any rigid shift)
    cb = sysm.stress_profile(pos, box, nb, center_index=c["center"], by_term=True)
    cm = sysm.stress_profile(shifted, box, nb, center_index=c["center"], by_term=True)
    assert torch.equal(cm[:, :, 0], cb[:, :, 0]) and float((cm[:, :, 1:] - cb[:, :, 1:]).abs().max()) <= tol


@DTYPES
def test_without_interactions_the_profile_is_kT_times_the_density(dtype):
    """eps = 0, no bonds, no angles: every W is exactly zero, so P_d = n_b kT / V_slab in every direction."""
    from mythos_amd.energy import martini as M
    from mythos_amd.hip_system import MartiniSystem
    from mythos_amd.observables import StressProfile

    c = _promoted("n131", dtype == torch.float32)
    z = np.zeros(0)
    sysm = MartiniSystem(c["ff"][0], c["ff"][1], np.zeros_like(c["ff"][2]), np.zeros((0, 2), np.int32), z, z, np.zeros((0, 3), np.int32), z, z,
                         dtype=dtype)
    raw = sysm.stress_profile(_dev(c["pos"], dtype), _dev(c["box"], dtype), 7, by_term=True)
    assert not raw[:, :, 1:].any() and (raw[:, :, 0].sum(1) == c["n"]).all()
    s = MH.system()
    lj0 = M.LJ.from_topology(topology=s["top"], params=M.LJConfiguration(**{k: (0.0 if k.startswith("lj_epsilon_") else v)
                                                                            for k, v in s["lj_params"].items()}))
    sp = StressProfile(topology=s["top"], energy_fn=lj0, n_bins=20, kT=KT)  # a single term: the others neutral
    traj = _bilayer_traj(dtype)
    p, rho = sp(traj), sp.density(traj)
    assert not sp.raw(traj)[:, :, 1:].any()
    assert torch.allclose(p, (KT * SR.BAR * rho)[:, :, None].expand(-1, -1, 3), rtol=1e-15, atol=0.0)  # (the products' own rounding)
    assert float((rho * (traj.box_size.prod(1) / 20)[:, None]).sum(1)[0]) == pytest.approx(1280.0, rel=1e-6)  # (fp32: the box as stored)


@DTYPES
def test_beads_on_slab_edges_land_in_the_slabs_of_the_formulas(dtype):
    """The device's slab function and its clamps where the other systems never go: beads exactly at z = 0, -0, Lz, one ulp
    under Lz, whole boxes outside, a tiny negative z (u rounds to 1), on the midplane, exactly half a box from it on either
    side and one ulp under half a box (t + 1/2 rounds to 1).  No interactions; every value is exact in the system's
    precision, the midpoint is one bead's z; counts against stress_profile_ref.slab_index, exactly."""
    from mythos_amd.hip_system import MartiniSystem

    npd = np.float32 if dtype == torch.float32 else np.float64
    lz = npd(4.0)
    z = np.array([1.5, 0.0, -0.0, lz, np.nextafter(lz, npd(0)), -lz, 2 * lz, -0.25, lz + npd(0.25), 3.5, -0.5, np.nextafter(npd(2.0), npd(0)),
                  -1e-30, np.nextafter(npd(1.5), npd(0)), 0.5, 1.0], dtype=npd)
    n = z.size
    pos = np.stack([0.7 * (np.arange(n) % 4), 0.7 * (np.arange(n) // 4), z.astype(np.float64)], axis=1)
    zero = np.zeros(0)
    sysm = MartiniSystem(np.zeros(n, np.int32), np.array([[0.47]]), np.array([[0.0]]), np.zeros((0, 2), np.int32), zero, zero,
                         np.zeros((0, 3), np.int32), zero, zero, dtype=dtype)
    p, b = _dev(pos[None], dtype), _dev([[3.0, 3.0, 4.0]], dtype)
    assert np.array_equal(p[0, :, 2].cpu().numpy().astype(np.float64), z.astype(np.float64))  # (nothing was rounded on the way)
    for nb in (1, 7, 8, 200):
        for centre in (None, 0, 1):  # fixed to the box; mid = 1.5 (bead 0); mid = 0 (bead 1)
            raw = sysm.stress_profile(p, b, nb, center_index=None if centre is None else [centre]).cpu().numpy()[0]
            want = np.bincount(SR.slab_index(z.astype(np.float64), 4.0, nb, None if centre is None else float(z[centre])), minlength=nb)
            assert np.array_equal(raw[:, 0], want), (nb, centre, raw[:, 0], want)
            assert not raw[:, 1:].any()


def test_the_box_check_can_be_left_out_and_changes_nothing():
    """check_boxes=False: the boxes stay on the device (no read-back), the rows are bitwise those of the checked call; a box
    under 2 r_cut is then the caller's to refuse."""
    c = _promoted("n131", False)
    sysm = _system(c, torch.float64)
    pos, box = _dev(c["pos"], torch.float64), _dev(c["box"], torch.float64)
    assert torch.equal(sysm.stress_profile(pos, box, 7, center_index=c["center"], check_boxes=False),
                       sysm.stress_profile(pos, box, 7, center_index=c["center"]))
    small = box.clone()
    small[1, 2] = 2.0
    with pytest.raises(ValueError, match="frame 1: box edge 2"):
        sysm.stress_profile(pos, small, 7)


# ---- f. the Python layer ------------------------------------------------------------------------------------------------------

def test_shapes_units_and_reweighting_against_the_reference():
    from mythos_amd.observables import StressProfile, SurfaceTension
    from mythos_amd.observables.stress_profile import TERMS, to_mN_per_m

    s, c = MH.system(), _promoted("bilayer", True)
    fn = _bilayer_energy_fn()
    kT = torch.tensor([KT, 1.1 * KT, 0.9 * KT], dtype=torch.float64)
    traj = _bilayer_traj(torch.float32, temperature=kT)
    nb = 24
    sp = StressProfile(topology=s["top"], energy_fn=fn, n_bins=nb, center="name C3A C3B")
    by = StressProfile(topology=s["top"], energy_fn=fn, n_bins=nb, center="name C3A C3B", by_term=True)
    p, pt = sp(traj), by(traj)
    assert p.shape == (3, nb, 3) and pt.shape == (3, nb, 5, 3) and len(TERMS) == 5 and p.dtype == torch.float64 and p.is_cuda
    assert sp.raw(traj).shape == (3, nb, 4) and by.raw(traj).shape == (3, nb, 13)
    assert sp.lateral(traj).shape == sp.density(traj).shape == sp.z(traj).shape == (3, nb) and sp.total(traj).shape == (3, 3)
    assert not pt[:, :, 4].any()  # no charges: no Coulomb part
    assert torch.allclose(pt.sum(2), p, rtol=0, atol=1e-9 * float(p.abs().max()))
    ref = _ref("bilayer", True, nb, True)
    ref4 = np.concatenate([ref[:, :, :1], ref[:, :, 1:].reshape(3, nb, 4, 3).sum(2)], axis=2)
    p_ref = np.stack([SR.pressures(ref4[f], c["box"][f], float(kT[f])) for f in range(3)])
    # a slab's W_d is within TOL of each term's scale: the sum of the four scales, as a pressure in the smallest slab volume
    bound = TOL[torch.float32] * _scales(ref).sum(1).max() / (c["box"].prod(1).min() / nb) * SR.BAR
    assert np.abs(p.cpu().numpy() - p_ref).max() <= bound
    z = sp.z(traj).cpu().numpy()
    # (the difference with 1/2 cancels: a few ulp of Lz / 2, not of the slab centre)
    np.testing.assert_allclose(z, ((np.arange(nb) + 0.5) / nb - 0.5)[None, :] * c["box"][:, 2:3], rtol=0, atol=4e-16 * c["box"][:, 2].max())
    np.testing.assert_allclose(StressProfile(topology=s["top"], energy_fn=fn, n_bins=nb).z(traj).cpu().numpy()[:, 0], 0.5 * c["box"][:, 2] / nb, rtol=1e-15)
    np.testing.assert_allclose(sp.density(traj).cpu().numpy(), ref4[:, :, 0] * nb / c["box"].prod(1)[:, None], rtol=1e-15)
    gamma = SurfaceTension(topology=s["top"], energy_fn=fn)(traj).cpu().numpy()
    g_ref = np.array([SR.surface_tension(ref4[f], c["box"][f], float(kT[f])) for f in range(3)])
    assert gamma.shape == (3,) and np.abs(gamma - g_ref).max() <= 2.0 * c["box"][:, 2].max() * bound / nb  # (one slab)
    assert to_mN_per_m == 0.1
    # kT= overrides the trajectory's temperature; the kinetic part scales with it
    hot = StressProfile(topology=s["top"], energy_fn=fn, n_bins=nb, center="name C3A C3B", by_term=True, kT=2.0 * KT)(traj)
    assert torch.allclose(hot[0, :, 0], 2.0 * pt[0, :, 0], rtol=1e-15) and torch.equal(hot[:, :, 1:], pt[:, :, 1:])
    # reweighting: weights @ the per-frame vectors, differentiable in the weights
    w = torch.tensor([0.2, 0.5, 0.3], dtype=torch.float64, device="cuda", requires_grad=True)
    mean = w @ p.reshape(3, -1)
    assert np.abs(mean.detach().cpu().numpy() - np.tensordot([0.2, 0.5, 0.3], p_ref, 1).reshape(-1)).max() <= bound
    mean.sum().backward()
    assert torch.allclose(w.grad, p.reshape(3, -1).sum(1))
    assert not p.requires_grad  # no gradient with respect to the parameters is handed out


def test_with_params_changes_the_profile_as_the_reference_under_the_new_tables():
    from mythos_amd.observables import StressProfile

    s, c = MH.system(), _bilayer_case()
    key = "bond_k_DMPC_GL1_GL2"
    new = 1.5 * s["bond_params"][key]
    traj = _bilayer_traj(torch.float64, slice(0, 1))
    nb = 12
    before = StressProfile(topology=s["top"], energy_fn=_bilayer_energy_fn(), n_bins=nb, by_term=True, kT=KT).raw(traj)
    after = StressProfile(topology=s["top"], energy_fn=_bilayer_energy_fn(**{key: new}), n_bins=nb, by_term=True, kT=KT).raw(traj)
    t, sg, ep, b, bk, br, an, ak, at = c["ff"]
    bk2 = np.where(np.asarray(s["top"].bond_names) == "DMPC_GL1_GL2", new, bk)
    assert (bk2 != bk).sum() > 0
    c2 = dict(c, ff=(t, sg, ep, b, bk2, br, an, ak, at), pos=c["pos"][:1], box=c["box"][:1])
    ref = SR.reference_rows(c2, nb)
    assert (_deviation(after.cpu().numpy(), ref) <= 1e-10).all()
    assert torch.equal(after[:, :, :4], before[:, :, :4]) and torch.equal(after[:, :, 7:], before[:, :, 7:])  # lj, angle, coulomb as before
    assert not torch.equal(after[:, :, 4:7], before[:, :, 4:7])


def test_errors_by_name():
    from mythos_amd import _lib
    from mythos_amd.observables import StressProfile, SurfaceTension

    s = MH.system()
    fn = _bilayer_energy_fn()
    traj = _bilayer_traj(torch.float64, slice(0, 1))
    sp = StressProfile(topology=s["top"], energy_fn=fn, n_bins=8)
    with pytest.raises(ValueError, match="neither trajectory.temperature nor kT= is given"):
        sp(traj)
    with pytest.raises(ValueError, match="neither trajectory.temperature nor kT= is given"):
        SurfaceTension(topology=s["top"], energy_fn=fn)(traj)
    with pytest.raises(ValueError, match="need trajectory.box_size"):
        sp(types.SimpleNamespace(center=traj.center, temperature=KT))
    with pytest.raises(ValueError, match="trajectory has 1279 beads, the topology 1280"):
        sp(types.SimpleNamespace(center=traj.center[:, :1279].contiguous(), box_size=traj.box_size, temperature=KT))
    with pytest.raises(_lib.MythosHipError, match="must live on a GPU"):
        sp(types.SimpleNamespace(center=traj.center.cpu(), box_size=traj.box_size.cpu(), temperature=KT))
    with pytest.raises(ValueError, match=r"n_bins 1025: expected an integer in \[1, 1024\]"):
        StressProfile(topology=s["top"], energy_fn=fn, n_bins=1025)
    with pytest.raises(ValueError, match="matches no bead"):
        StressProfile(topology=s["top"], energy_fn=fn, n_bins=8, center="name NOPE")
    with pytest.raises(TypeError, match="MartiniComposedEnergyFunction or a single MARTINI term"):
        StressProfile(topology=s["top"], energy_fn=object(), n_bins=8)
    small = types.SimpleNamespace(center=traj.center, box_size=torch.tensor([[6.0, 6.0, 2.0]], dtype=torch.float64, device="cuda"), temperature=KT)
    with pytest.raises(ValueError, match="frame 0: box edge 2 = 2.0+ is shorter than 2 r_cut"):
        sp(small)
    sysm = sp._system(torch.float64, traj.center.device)
    with pytest.raises(ValueError, match=r"centre index 1280 \(entry 0\) is outside \[0, 1280\)"):
        sysm.stress_profile(traj.center, traj.box_size, 8, center_index=[1280])
