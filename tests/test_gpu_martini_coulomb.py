"""GPU tests of MARTINI reaction-field Coulomb: mythos_martini_coulomb, the COUL instantiations of the step and pressure
kernels, and the Python ``Coulomb`` term, against tests/martini_rf_ref.py (fp64 NumPy, all pairs).

The reference ships no Coulomb energies; the formula of the GROMACS manual, restated in martini_rf_ref.py, is the pin.
Tolerances are the ones the existing MARTINI tests hold LJ to at the same precision: energy and forces 1e-7 / 1e-3
(test_gpu_martini.py), step by step 1e-10 nm, nm/ps and rtol 1e-9 / atol 1e-7 kJ/mol (test_gpu_martini_md.py), virial 1e-10
of its largest component in fp64 (test_gpu_martini_npt.py).
"""

import dataclasses as dc
import functools

import numpy as np
import pytest
import torch

from mythos_amd.energy import martini as M
from oracle import martini_oracle as mo
from tests import martini_helpers as MH
from tests import martini_rf_ref as RF
from tests import martini_synth as S

pytestmark = pytest.mark.gpu

KB = 0.0083144626
T = 273.0
R_CUT = 1.1
TOL = {torch.float64: 1e-7, torch.float32: 1e-3}  # test_gpu_martini.py::test_terms_and_forces_match_oracle


@dc.dataclass
class Traj:
    center: torch.Tensor
    box_size: torch.Tensor


# ---- systems ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(name):
    """A system of tests/martini_synth.py with charges chosen so that it holds: a charged bonded pair (+1, -1), a charged -
    uncharged bonded pair (+0.5, 0), a charged pair just inside r_c and one just outside (first frame), a bead whose
    charge value no other bead has (0.3), five distinct non-zero values in all."""
    s = S.get(name)
    S.check(s)
    n, bonds = s["n"], s["bonds"].astype(np.int64)
    x, box = s["pos"][0], s["box"][0]
    q = np.zeros(n)
    used = set()

    def take(beads, values):
        for b, v in zip(beads, values):
            assert int(b) not in used
            q[int(b)] = v
            used.add(int(b))

    take(bonds[0], (1.0, -1.0))
    mixed = next(b for b in bonds if not (set(b.tolist()) & used))
    take(mixed, (0.5, 0.0))
    _, r = next(S.pair_distances(x, box, block=n))
    r = np.where(S.bonded_mask(s), np.inf, r)
    gaps = {}
    for label, values in (("inside", (-0.5, 1.0)), ("outside", (1.0, 1.0))):
        free = np.array([i not in used for i in range(n)])
        ok = free[:, None] & free[None, :] & ((r < R_CUT) if label == "inside" else (r > R_CUT)) & np.isfinite(r)
        d = np.where(ok, np.abs(r - R_CUT), np.inf)
        i, j = np.unravel_index(np.argmin(d), d.shape)
        gaps[label] = r[i, j] - R_CUT
        take((i, j), values)
    assert -0.05 < gaps["inside"] < 0.0 < gaps["outside"] < 0.05, gaps
    take([next(i for i in range(n) if i not in used)], (0.3,))
    assert len(set(q[q != 0.0].tolist())) == 5 and n % 16 != 0 and n % 256 != 0 and len(set(box.tolist())) == 3
    q.setflags(write=False)
    return s, q


def _synthetic_system(name, dtype):
    from mythos_amd.hip_system import MartiniSystem

    s, q = _synthetic(name)
    sysm = MartiniSystem(s["types"], s["sigma"], s["eps"], s["bonds"], s["bond_k"], s["bond_r0"], s["angles"], s["angle_k"],
                         s["angle_t0"], dtype=dtype)
    sysm.set_charges(q)
    return s, q, sysm


def _bilayer_system(dtype):
    from mythos_amd.hip_system import MartiniSystem

    s = MH.system()
    top = s["top"]
    sysm = MartiniSystem(s["types"], s["sigma"], s["eps"], top.bonded_neighbors, s["bond_k"], s["bond_r0"], top.angles,
                         s["angle_k"], s["angle_t0"], dtype=dtype)
    sysm.set_charges(top.charges)
    return s, np.asarray(top.charges), sysm


@functools.lru_cache(maxsize=None)
def _bilayer_reference(frame):
    s = MH.system()
    x, box, _ = MH.frames("lj")
    return RF.coulomb(x[frame], box[frame], s["top"].charges, s["top"].bonded_neighbors, R_CUT)


def _dev(a, sysm):
    return torch.tensor(np.asarray(a), dtype=sysm.dtype, device=sysm.device).contiguous()


def _check_energy_and_forces(sysm, pos, box, refs, dtype):
    e, g = sysm.coulomb(_dev(pos, sysm), _dev(box, sysm), grads=True)
    tol = TOL[dtype]
    for k, ref in enumerate(refs):
        got, f = e[k].item(), -g[k].cpu().double().numpy()
        err_f = np.abs(f - ref["f"]).max() / np.abs(ref["f"]).max()
        print(f"  frame {k}: E {got:.9g} (reference {ref['e']:.9g}: pair {ref['energy']['pair']:.6g}, excluded "
              f"{ref['energy']['excluded']:.6g}, self {ref['energy']['self']:.6g}), force error {err_f:.2e} of {np.abs(ref['f']).max():.4g}")
        assert np.allclose(got, ref["e"], rtol=max(tol, 1e-9), atol=tol * abs(ref["e"]))
        assert err_f <= tol


# ---- 1, 2: energy and forces of stored frames ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_coulomb_energy_and_forces_on_the_bilayer(dtype):
    _, _, sysm = _bilayer_system(dtype)
    x, box, _ = MH.frames("lj")
    frames = [0, 4]
    refs = [_bilayer_reference(f) for f in frames]
    assert all(r["energy"]["excluded"] != 0.0 for r in refs)  # NC3 - PO4 are bonded: the excluded-pair term is live
    _check_energy_and_forces(sysm, x[frames], box[frames], refs, dtype)
    # the LJ / bond / angle entry point does not see the charges
    e_charged, _ = sysm.energy(_dev(x[0], sysm), _dev(box[0], sysm))
    sysm.set_charges(None)
    e_plain, _ = sysm.energy(_dev(x[0], sysm), _dev(box[0], sysm))
    assert torch.equal(e_charged, e_plain)
    e0, g0 = sysm.coulomb(_dev(x[0], sysm), _dev(box[0], sysm), grads=True)
    assert e0.item() == 0.0 and not g0.any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["n257", "md37"])
def test_coulomb_energy_and_forces_on_synthetic_systems(name, dtype):
    s, q, sysm = _synthetic_system(name, dtype)
    ref = RF.coulomb(s["pos"][0], s["box"][0], q, s["bonds"], R_CUT)
    assert ref["energy"]["pair"] != 0.0 and ref["energy"]["excluded"] != 0.0
    _check_energy_and_forces(sysm, s["pos"][:1], s["box"][:1], [ref], dtype)
    # finite epsilon_rf: another k_rf, a force that does not vanish at the cut-off
    sysm.set_charges(q, epsilon_r=4.0, epsilon_rf=62.0)
    ref = RF.coulomb(s["pos"][0], s["box"][0], q, s["bonds"], R_CUT, 4.0, 62.0)
    _check_energy_and_forces(sysm, s["pos"][:1], s["box"][:1], [ref], dtype)


def test_refused_charges():
    s, q, sysm = _synthetic_system("md37", torch.float64)
    many = np.zeros(s["n"])
    many[:8] = 0.1 * np.arange(1, 9)  # eight non-zero values and 0: nine classes for a table of eight
    with pytest.raises(ValueError, match="distinct charge values"):
        sysm.set_charges(many)
    bad = q.copy()
    bad[3] = np.nan
    for args in ((q, 0.0, 0.0), (q, -1.0, 0.0), (q, 15.0, -1.0), (q, np.inf, 0.0), (bad, 15.0, 0.0)):
        with pytest.raises(ValueError, match="set_charges"):
            sysm.set_charges(*args)
    # a refused call changes nothing
    ref = RF.coulomb(s["pos"][0], s["box"][0], q, s["bonds"], R_CUT)
    e, _ = sysm.coulomb(_dev(s["pos"][0], sysm), _dev(s["box"][0], sysm))
    assert abs(e.item() - ref["e"]) <= 1e-7 * abs(ref["e"])


# ---- 3: MD against velocity Verlet in NumPy ------------------------------------------------------------------------------
def _integrator(s, sysm, *, dt=0.01, gamma=0.0, skin=0.2, every=2, inner=None, seed=11):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=dt, kT=KB * T, gamma=gamma, mass=s["mass"], seed=seed)
    integ.set_neighbor_policy(skin, every)
    if inner is not None:
        integ.set_inner_list(*inner)
    return integ


@functools.lru_cache(maxsize=None)
def _verlet_reference(n_steps, dt):
    """md37, charged: (v0, x (n_steps, n, 3), v, Coulomb energy per step) of velocity Verlet with the forces of
    oracle/martini_oracle.py plus the reference Coulomb forces.  v0 is drawn by the integrator's own generator."""
    s, q, sysm = _synthetic_system("md37", torch.float64)
    v0 = _integrator(s, sysm).init_velocities().cpu().numpy().copy()
    a = S.oracle_args(s)
    box = s["box"][0]

    def force(x):
        _, g = mo.energies_and_forces(torch.as_tensor(x), *a[1:], True)
        c = RF.coulomb(x, box, q, s["bonds"], R_CUT)
        return -g.numpy() + c["f"], c["e"]

    x, v, im = s["pos"][0].copy(), v0.copy(), (1.0 / s["mass"])[:, None]
    f, _ = force(x)
    xs, vs, es = [], [], []
    for _ in range(n_steps):
        v = v + 0.5 * dt * f * im
        x = x + dt * v
        f, e = force(x)
        v = v + 0.5 * dt * f * im
        xs.append(x.copy()), vs.append(v.copy()), es.append(e)
    return v0, np.array(xs), np.array(vs), np.array(es)


@pytest.mark.parametrize("inner", [None, (0.1, 2)], ids=["verlet-rows", "pruned-rows"])
def test_twenty_steps_against_velocity_verlet_fp64(inner):
    """gamma = 0: c1 = 1 and no noise, so BAOAB is velocity Verlet."""
    n_steps, dt = 20, 0.01
    s, q, sysm = _synthetic_system("md37", torch.float64)
    v0, xs, vs, es = _verlet_reference(n_steps, dt)
    integ = _integrator(s, sysm, dt=dt, inner=inner)
    pos, vel = _dev(s["pos"][0], sysm), _dev(v0, sysm)
    traj, et = integ.run(pos, vel, s["box"][0], n_steps, save_every=1)
    print(f"  max |dx| {np.abs(pos.cpu().numpy() - xs[-1]).max():.2e} |dv| {np.abs(vel.cpu().numpy() - vs[-1]).max():.2e} "
          f"|dE_coul| {np.abs(et[:, 4].cpu().numpy() - es).max():.2e}; moved {np.abs(xs[-1] - s['pos'][0]).max():.3f} nm")
    np.testing.assert_allclose(pos.cpu().numpy(), xs[-1], rtol=0, atol=1e-10)
    np.testing.assert_allclose(vel.cpu().numpy(), vs[-1], rtol=0, atol=1e-10)
    np.testing.assert_allclose(traj.cpu().numpy(), xs, rtol=0, atol=1e-10)
    np.testing.assert_allclose(et[:, 4].cpu().numpy(), es, rtol=1e-9, atol=1e-7)
    if inner is not None:
        _, lens_in = integ.rows(True)
        _, lens = integ.rows(False)
        assert (lens_in <= lens).all() and lens_in.sum() < lens.sum()


# ---- 4: bitwise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_split_advances_are_bitwise_one_advance_with_charges(dtype):
    s, q, sysm = _synthetic_system("md37", dtype)
    for inner in (None, (0.1, 3)):
        outs = []
        for calls in ((24,), (7, 0, 11, 6)):
            integ = _integrator(s, sysm, gamma=2.0, every=5, inner=inner)
            pos = _dev(s["pos"][0], sysm)
            vel = integ.init_velocities()
            integ.load(pos, vel, s["box"][0])
            for c in calls:
                integ.advance(c)
            integ.store(pos, vel)
            outs.append((pos.clone(), vel.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), inner
        assert torch.isfinite(outs[0][0]).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_all_zero_charges_are_bitwise_no_charges(dtype):
    from mythos_amd.hip_system import MartiniSystem

    s, q = _synthetic("md37")
    outs = []
    for how in ("never", "zeros", "set-then-cleared", "charged"):
        sysm = MartiniSystem(s["types"], s["sigma"], s["eps"], s["bonds"], s["bond_k"], s["bond_r0"], s["angles"], s["angle_k"],
                             s["angle_t0"], dtype=dtype)
        integ = _integrator(s, sysm, gamma=2.0)
        if how == "zeros":
            sysm.set_charges(np.zeros(s["n"]))
        elif how != "never":
            sysm.set_charges(q)
        pos = _dev(s["pos"][0], sysm)
        vel = integ.init_velocities()
        if how == "set-then-cleared":
            integ.load(pos, vel, s["box"][0])  # the integrator has seen the charges
            sysm.set_charges(None)
        traj, et = integ.run(pos, vel, s["box"][0], 12, save_every=4)
        assert et.shape == (3, 5 if how == "charged" else 4)
        outs.append((pos.clone(), vel.clone(), et.clone()))
    for other in outs[1:3]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    assert not torch.equal(outs[0][0], outs[3][0])


# ---- 5: trace -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_the_fifth_trace_column_is_the_coulomb_energy_of_the_saved_frame(dtype):
    s, q, sysm = _bilayer_system(dtype)
    x, box, _ = MH.frames("lj")
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=0.01, kT=KB * T, gamma=2.0, seed=3)
    integ.set_neighbor_policy(0.25, 3)
    pos = _dev(x[3], sysm)
    vel = integ.init_velocities()
    traj, et = integ.run(pos, vel, box[3], 6, save_every=3)
    assert et.shape == (2, 5) and torch.isfinite(et).all()
    e, _ = sysm.coulomb(traj, _dev(np.tile(box[3], (2, 1)), sysm))
    tol = TOL[dtype]
    print(f"  trace {et[:, 4].tolist()}, mythos_martini_coulomb {e.tolist()}")
    assert np.allclose(et[:, 4].cpu().numpy(), e.cpu().numpy(), rtol=max(tol, 1e-9), atol=tol * e.abs().max().item())
    sysm.set_charges(None)
    _, et = integ.run(pos, vel, box[3], 3, save_every=3)
    assert et.shape == (1, 4)


# ---- 6: pressure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bilayer", "md37"])
def test_coulomb_virial_is_the_pressure_difference_fp64(name):
    if name == "bilayer":
        s0, q, sysm = _bilayer_system(torch.float64)
        x, box, _ = MH.frames("lj")
        pos0, box0, bonds, mass, skin = x[3], box[3], s0["top"].bonded_neighbors, None, 0.25
    else:
        s0, q, sysm = _synthetic_system("md37", torch.float64)
        pos0, box0, bonds, mass, skin = s0["pos"][0], s0["box"][0], s0["bonds"], s0["mass"], 0.2
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=0.01, kT=KB * T, gamma=2.0, mass=mass, seed=5)
    integ.set_neighbor_policy(skin, 2)
    pos = _dev(pos0, sysm)
    integ.load(pos, integ.init_velocities(), box0)
    charged = integ.pressure()
    sysm.set_charges(None)
    plain = integ.pressure()
    sysm.set_charges(q)
    again = integ.pressure()
    ref = RF.coulomb(pos0, box0, q, bonds, R_CUT)
    dw = charged["virial"] - plain["virial"]
    err = np.abs(dw - ref["w"]).max() / np.abs(ref["w"]).max()
    print(f"  {name}: W_coul {dw} (reference {ref['w']}: excluded pairs {ref['virial']['excluded']}), rel. error {err:.2e}")
    assert err <= 1e-10  # test_gpu_martini_npt.py::test_pressure_kernel_against_the_oracle, fp64
    assert np.array_equal(charged["kinetic"], plain["kinetic"])
    assert all(np.array_equal(charged[k], again[k]) for k in ("kinetic", "virial", "pressure"))


def test_a_semi_isotropic_coupling_event_on_a_charged_bilayer():
    s, q, sysm = _bilayer_system(torch.float32)
    x, box, _ = MH.frames("lj")
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=KB * T, gamma=1.0, seed=9)
    integ.set_neighbor_policy(0.25, 5)
    integ.set_barostat("c-rescale", "semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 3e-4), tau_p=1.0, every=5)
    pos = _dev(x[3], sysm)
    vel = integ.init_velocities()
    traj, et = integ.run(pos, vel, box[3], 6, save_every=6)
    new = integ.box
    assert (new != box[3]).all() and new[0] / box[3][0] == pytest.approx(new[1] / box[3][1], rel=1e-12)
    assert np.abs(new / box[3] - 1.0).max() < 0.05
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all() and torch.isfinite(et).all() and et.shape == (1, 5)


# ---- 7: the Python term -------------------------------------------------------------------------------------------------------
def test_coulomb_energy_function_autograd_and_composition():
    s = MH.system()
    x, box, _ = MH.frames("lj")
    frames = [0, 4]
    dev = torch.device("cuda", 0)
    traj = Traj(torch.as_tensor(x[frames], device=dev), torch.as_tensor(box[frames], device=dev))
    refs = np.array([_bilayer_reference(f)["e"] for f in frames])

    eps_r = torch.tensor(15.0, dtype=torch.float64, requires_grad=True)
    fn = M.Coulomb.from_topology(topology=s["top"], params=M.CoulombConfiguration(epsilon_r=eps_r))
    assert set(fn.opt_params()) == {"epsilon_r"}
    e = fn.map(traj)
    np.testing.assert_allclose(e.detach().cpu().numpy(), refs, rtol=1e-7)
    w = torch.tensor([1.0, -0.5], dtype=torch.float64, device=dev)
    (g,) = torch.autograd.grad((e * w).sum(), eps_r)
    assert g.item() == pytest.approx(-(refs * np.array([1.0, -0.5])).sum() / 15.0, rel=1e-7)
    # another epsilon_r through with_params: E scales with 1 / epsilon_r
    np.testing.assert_allclose(fn.with_params(epsilon_r=30.0).map(traj).cpu().numpy(), refs / 2.0, rtol=1e-7)
    # positions: autograd hands back the kernel's dU/dpos
    p = traj.center[:1].clone().requires_grad_(True)
    (gp,) = torch.autograd.grad(fn.map(Traj(p, traj.box_size[:1])).sum(), p)
    f_ref = _bilayer_reference(0)["f"]
    assert np.abs(-gp[0].cpu().numpy() - f_ref).max() <= 1e-7 * np.abs(f_ref).max()
    with pytest.raises(ValueError, match="epsilon_rf = 0"):
        M.CoulombConfiguration(epsilon_r=eps_r, epsilon_rf=78.0)
    with pytest.raises(ValueError, match="charges"):
        M.Coulomb.from_topology(topology=dc.replace(s["top"], charges=None))

    ang = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    parts = [M.LJ.from_topology(topology=s["top"], params=M.LJConfiguration(**s["lj_params"])),
             M.Bond.from_topology(topology=s["top"], params=M.BondConfiguration(**s["bond_params"])),
             M.Angle.from_topology(topology=s["top"], params=M.AngleConfiguration(**ang)),
             M.Coulomb.from_topology(topology=s["top"])]
    total = M.MartiniComposedEnergyFunction(parts).map(traj)
    each = [fn_k.map(traj) for fn_k in parts]
    assert torch.equal(total, each[0] + each[1] + each[2] + each[3])
    np.testing.assert_allclose(each[3].cpu().numpy(), refs, rtol=1e-7)
    composed = M.MartiniComposedEnergyFunction(parts).with_params(epsilon_r=30.0)
    np.testing.assert_allclose(composed.map(traj).cpu().numpy(), (each[0] + each[1] + each[2]).cpu().numpy() + refs / 2.0, rtol=1e-7)
