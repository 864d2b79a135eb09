"""The MARTINI kernels at the sizes, boxes and type tables the bilayer fixture never reaches (tests/martini_synth.py).

The fixture is 1 280 = 5 x 256 = 80 x 16 beads (or 16 tiles of it), 10 frames, four bead types that all occur: it lines
up with every structural boundary of mythos_amd/csrc/martini.hip and martini_md.hip.  Here, every case first asserts on
its inputs - restating the host code's rule in Python - that the path it is about is the one taken:

  energy path  (a) one tile or less, a partial last tile and workgroup, n = 1 and 2   (b) more than 16 frames with the
               partner tiles still split over blockIdx.y   (c) more than 4 096 frames: chunked launches, in the energy
               and in the parameter-gradient entry point   (d) the limits of the incidence lists and their refusals
  MD path      (e) all-pairs row builder under 512 beads, a partial last workgroup, blocks of the XCD-ordered map that
               return early   (f) cell builder, direct table, partial workgroup   (g) all-pairs builder above 512 beads
               (a slab two cells thick)   (h) hashed cell table   (i) fp32   (j) pruned rows on a partial workgroup
  everywhere   a bead with 8 bonds and 12 angle memberships as bead n - 1, bead types {1, 4, 6} of a 7-type table,
               unwrapped coordinates, a non-cubic box, near-straight harmonic angles.

References: oracle/martini_oracle.py (torch fp64, autograd) and oracle/martini_langevin_oracle.py; for fp32 the oracle
is fed the fp32-rounded positions, boxes and tables.  Tolerances are those of tests/test_gpu_martini.py and
tests/test_gpu_martini_md.py.  The floor under them - the oracle against the double host build of the kernels' term
functions on these same systems, as tests/test_martini_synth_cpu.py prints it:

  system     rel. energy difference (lj / bond / angle, worst of both angle kinds)   force difference / max|g|
  n2         0       / 4.2e-15 / 0         1.9e-15
  n3         1.1e-15 / 1.3e-15 / 5.6e-15   6.4e-16
  n65        2.4e-15 / 1.8e-15 / 2.2e-16   4.8e-15
  n255       1.9e-15 / 5.9e-16 / 4.8e-16   8.5e-15
  n257       5.7e-15 / 2.2e-16 / 2.8e-16   1.3e-14
  n1100      2.5e-16 / 8.9e-16 / 3.0e-16   2.1e-14
  md37       7.2e-15 / 2.6e-16 / 9.5e-16   3.0e-15
  md1285     0       / 3.4e-16 / 0         2.0e-14
  slab1285   2.2e-16 / 3.2e-16 / 4.4e-16   2.5e-14
  dilute520  7.5e-15 / 3.9e-16 / 5.7e-16   6.9e-14
  five Langevin steps: md37 |dx| 3.3e-16 nm, |dv| 5.1e-15 nm/ps, energies 4.5e-13 of 493 kJ/mol;
                       dilute520 |dx| 7.1e-15, |dv| 1.9e-13, energies 5.5e-12 of 1.38e4

- six orders of magnitude and more under the fp64 tolerances (1e-9 / 1e-7 relative, 1e-10 nm).
"""

import functools

import numpy as np
import pytest
import torch

from oracle import martini_oracle as mo
from tests import martini_synth as S

pytestmark = pytest.mark.gpu

KB = 0.0083144626
T = 273.0
SEED = 0xABCDEF012345
R_C = S.R_CUT
LJ_BLOCK = 256  # kLjBlock: beads per workgroup and per partner tile of the energy path
MD_PPB = 16  # kMmPPB: beads per workgroup of the step kernel
THETA_KEYS = ("sigma", "eps", "bond_k", "bond_r0", "angle_k", "angle_t0")


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _system(s, dtype, angle_kind=0, **over):
    from mythos_amd.hip_system import MartiniSystem

    a = {k: over.get(k, s[k]) for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0")}
    return MartiniSystem(a["types"], a["sigma"], a["eps"], a["bonds"], a["bond_k"], a["bond_r0"], a["angles"], a["angle_k"],
                         a["angle_t0"], angle_kind=angle_kind, dtype=dtype)


def _dev(a, sysm):
    """A fresh device tensor of the system's dtype (the generator's arrays are read-only)."""
    return torch.tensor(np.asarray(a), dtype=sysm.dtype, device=sysm.device).contiguous()


def _device_frames(s, sysm, frames=None):
    sel = slice(None) if frames is None else frames
    return _dev(s["pos"][sel], sysm), _dev(s["box"][sel], sysm)


@functools.lru_cache(maxsize=None)
def _reference(name, frame, angle_kind, fp32):
    """Oracle [lj, bond, angle], dU/dpos and the gradients with respect to the six parameter arrays (LJ tables: of the
    oracle's symmetric table, every pair i < j entered once at [type_i][type_j]) - computed once, shared, read-only."""
    s = S.get(name)
    pos, box, types, sig, eps, bonds, bk, br, angles, ak, at = S.oracle_args(s, frame, np.float32 if fp32 else None)
    leaves = [pos, sig, eps, bk, br, ak, at]
    for t in leaves:
        t.requires_grad_(True)
    e = torch.stack([mo.lj_energy(pos, box, types, sig, eps, bonds), mo.bond_energy(pos, box, bonds, bk, br),
                     mo.angle_energy(pos, box, angles, ak, at, angle_kind == 0)])
    grads = [torch.zeros_like(t) for t in leaves]
    for k in range(3):  # (a term is a constant when it has no pair, bond or angle)
        if e[k].requires_grad:
            for acc, g in zip(grads, torch.autograd.grad(e[k], leaves, retain_graph=True, allow_unused=True)):
                if g is not None:
                    acc += g
    out = dict(e=e.detach().numpy(), g=grads[0].numpy(), **{k: g.numpy() for k, g in zip(THETA_KEYS, grads[1:])})
    for v in out.values():
        v.setflags(write=False)
    return out


def _sym(t):
    """Ordered-pair table(s) (..., T, T) -> gradient per unordered pair: out[a][b] + out[b][a], the diagonal once."""
    return np.triu(t + np.swapaxes(t, -1, -2)) - np.triu(np.tril(t))


def _within(label, err, bound):
    print(f"    {label}: {err:.3e} (bound {bound:.3e})")
    return err <= bound


def _compare(label, dtype, e, g, pg, ref):
    """Energies, forces and all six parameter gradients of one frame against ``ref`` at the project's tolerances."""
    f64 = dtype == torch.float64
    tol = 1e-7 if f64 else 1e-3
    print(f"  {label}")
    e, e_ref = np.asarray(e), ref["e"]
    for k, term in enumerate(("lj", "bond", "angle")):
        assert _within(f"energy {term} {e[k]:.6g}", abs(e[k] - e_ref[k]), (1e-9 if f64 else tol) * abs(e_ref[k]) + tol * np.abs(e_ref).max())
    assert _within("forces", np.abs(np.asarray(g, dtype=np.float64) - ref["g"]).max(), tol * np.abs(ref["g"]).max())
    tol_lj = 1e-8 if f64 else 2e-3
    for key in ("sigma", "eps"):
        assert _within(f"d/d{key}", np.abs(_sym(pg[key]) - _sym(ref[key])).max(), tol_lj * np.abs(ref[key]).max())
    # fp64: per entry.  fp32: per array, as for the forces - a bond's length carries a few ulp of the largest coordinate
    # (2e-6 nm at 16 nm, unwrapped beads), k times that in dU/dr0 whatever the entry's own size (0 where r = r0)
    for key in ("bond_k", "bond_r0", "angle_k", "angle_t0"):
        if ref[key].size:
            bound = 1e-9 * np.maximum(1.0, np.abs(ref[key])) if f64 else np.full(ref[key].shape, 1e-3 * max(1.0, np.abs(ref[key]).max()))
            err = np.abs(pg[key] - ref[key])
            worst = int(np.argmax(err / bound))
            assert _within(f"d/d{key}[{worst}] ({ref[key][worst]:.4g})", err[worst], bound[worst])


def _all_outputs(sysm, pos, box):
    e, g = sysm.energy(pos, box, grads=True)
    pg = sysm.param_grads(pos, box)
    return e, g, pg


def _frame(e, g, pg, k):
    return e[k].cpu().numpy(), g[k].cpu().numpy(), {key: pg[key][k].cpu().numpy() for key in THETA_KEYS}


# ---- (a) sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("angle_kind", [0, 1], ids=["g96", "harmonic"])
@pytest.mark.parametrize("name", ["n1", "n2", "n65", "n255", "n257", "n1100"])
def test_sizes_off_the_tile(name, angle_kind, dtype):
    """n = 1, 2, 65, 255 (one tile, n_js == 1: jl < n and cnt < 256 in lj_tile_sweep), 257 (a tile of one bead, a workgroup
    with one live thread), 1 100 (five tiles, the last of 76 beads, spread over blockIdx.y): energies, forces, all six
    parameter gradients - every bead, every entry - and the sum of the forces."""
    s = S.get(name)
    S.check(s)
    n = s["n"]
    assert (np.abs(s["shift"]).max() == 2 or n < 3) and len(set(s["box"][0])) == 3  # unwrapped beads, non-cubic box
    n_tiles = -(-n // LJ_BLOCK)
    assert (n % LJ_BLOCK != 0) and n_tiles == {1: 1, 2: 1, 65: 1, 255: 1, 257: 2, 1100: 5}[n]
    occurring = np.unique(s["types"])
    assert set(occurring.tolist()) < {1, 4, 6} or n >= 27 and set(occurring.tolist()) == {1, 4, 6}  # of 7 types
    sysm = _system(s, dtype, angle_kind)
    pos, box = _device_frames(s, sysm)
    e, g, pg = _all_outputs(sysm, pos, box)
    e0, g0, pg0 = _frame(e, g, pg, 0)
    ref = _reference(name, 0, angle_kind, dtype == torch.float32)
    _compare(f"{name} kind {angle_kind} {dtype}", dtype, e0, g0, pg0, ref)
    if n == 1:
        assert (e0 == 0.0).all() and (g0 == 0.0).all()
    if n == 2:  # the only pair is bonded
        assert e0[0] == 0.0 and e0[2] == 0.0 and e0[1] > 0.0
        e_nb, g_nb = _system(s, dtype, angle_kind, bond_k=np.zeros(1)).energy(pos, box, grads=True)  # the exclusion stays, the bond force goes
        assert (e_nb.cpu().numpy() == 0.0).all() and (g_nb.cpu().numpy() == 0.0).all()
        assert (pg0["sigma"] == 0.0).all() and (pg0["eps"] == 0.0).all()
    # no gradient for a type that does not occur: rows and columns of the ordered-pair tables are exactly zero
    absent = np.setdiff1d(np.arange(7), occurring)
    assert absent.size >= 4
    for key in ("sigma", "eps"):
        assert (pg0[key][absent, :] == 0.0).all() and (pg0[key][:, absent] == 0.0).all()
        if n >= 27:
            assert (_sym(pg0[key])[np.ix_(occurring, occurring)][np.triu_indices(3)] != 0.0).all()
    # sum of the forces: the two halves of a pair are exact negatives of each other (rint is odd), so what is left is
    # rounding: of each bead's own sum - under 300 terms (the sites of a 0.5 nm lattice inside r_c, 8 bonds, 12 angles),
    # one rounding each relative to the largest term, for which four times the largest net force stands in - and of
    # the sum over the n beads.  (fp64: ~1e-10 of max|g| at 1 100 beads, a thousand times under the per-bead tolerance)
    eps_r = float(np.finfo(_np_dtype(dtype)).eps)
    assert _within("sum of forces", np.abs(g0.astype(np.float64).sum(0)).max(), n * 300 * 4 * eps_r * max(np.abs(ref["g"]).max(), 1.0))


# ---- (b) more than 16 frames, partner tiles still split ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_seventeen_frames_with_split_partner_tiles(dtype):
    """n = 2 000: nbx = 8 workgroups and tiles, the last of 208 beads; gridDim.y (n_js) is 8 up to 16 frames and 8 / 4 = 2
    above, so each workgroup strides over four tiles - in the energy and in the LJ parameter-gradient kernel.  17 frames,
    each with its own box: frames 0, 8, 16 against the oracle, every frame against its own call of one frame (n_js = 8:
    another order of the partial sums, so no bitwise equality)."""
    s = S.get("n2000")
    S.check(s)
    n, nf = s["n"], s["pos"].shape[0]
    nbx = -(-n // LJ_BLOCK)
    n_js = lambda frames: max(1, min(nbx, max(1, 768 // nbx)) // (4 if frames > 16 else 1))  # noqa: E731  (martini_energy_typed)
    assert nbx == 8 and n - 7 * LJ_BLOCK == 208 and nf == 17 and n_js(1) == 8 and n_js(nf) == 2
    assert np.ptp(s["box"], axis=0).min() > 0.0
    sysm = _system(s, dtype, 0)
    pos, box = _device_frames(s, sysm)
    e, g, pg = _all_outputs(sysm, pos, box)
    for f in (0, 8, 16):
        _compare(f"n2000 frame {f} of 17 {dtype}", dtype, *_frame(e, g, pg, f), _reference("n2000", f, 0, dtype == torch.float32))
    for f in range(nf):
        e1, g1, pg1 = _all_outputs(sysm, pos[f:f + 1], box[f:f + 1])
        one = dict(e=e1[0].cpu().numpy(), g=g1[0].cpu().double().numpy(), **{k: pg1[k][0].cpu().numpy() for k in THETA_KEYS})
        _compare(f"n2000 frame {f}: call of 17 against call of 1", dtype, *_frame(e, g, pg, f), one)


# ---- (c) more than 4 096 frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("angle_kind", [0, 1], ids=["g96", "harmonic"])
def test_more_frames_than_one_launch_takes(angle_kind, dtype):
    """4 100 frames of a three-bead chain (two bonds, one angle, one unbonded pair inside r_c), each with its own box: the
    second launch of mythos_martini_energy and of mythos_martini_param_grads starts at frame 4 096 - f0-offset pointers
    for e_terms, dU and the six gradient arrays.  At nbx = 1 every launch shape is the same whatever the frame count, so
    the one call equals the calls on [:4096] and [4096:] bitwise."""
    s = S.get("n3")
    S.check(s)
    nf = s["pos"].shape[0]
    assert s["n"] == 3 and nf == 4100 > 4096 and s["bonds"].shape[0] == 2 and s["angles"].shape[0] == 1
    sysm = _system(s, dtype, angle_kind)
    pos, box = _device_frames(s, sysm)
    e, g, pg = _all_outputs(sysm, pos, box)
    assert (e[:, 0] != 0.0).all()  # the unbonded pair is inside the cut-off in every frame
    for f in (0, 1, 4095, 4096, 4097, 4099):
        _compare(f"n3 frame {f} kind {angle_kind} {dtype}", dtype, *_frame(e, g, pg, f), _reference("n3", f, angle_kind, dtype == torch.float32))
    for part in (slice(0, 4096), slice(4096, nf)):
        ep, gp, pgp = _all_outputs(sysm, pos[part], box[part])
        assert torch.equal(e[part], ep) and torch.equal(g[part], gp)
        for key in THETA_KEYS:
            assert torch.equal(pg[key][part], pgp[key]), key


# ---- (d) limits --------------------------------------------------------------------------------------------------------
def test_incidence_limits_and_refusals():
    """8 bonds (kMaxExcl, kMaxBeadBonds) and 12 angle memberships (kMaxBeadAngles) on one bead are accepted, one more is
    refused by mythos_martini_create on the host, and so are a bond of a bead with itself and an index == n."""
    from mythos_amd import _lib
    from mythos_amd.hip_system import MartiniSystem

    def create(n, bonds, angles):
        bonds, angles = np.asarray(bonds, dtype=np.int32).reshape(-1, 2), np.asarray(angles, dtype=np.int32).reshape(-1, 3)
        nb, na = bonds.shape[0], angles.shape[0]
        return MartiniSystem(np.zeros(n, np.int32), np.full((1, 1), 0.47), np.full((1, 1), 3.0), bonds, np.full(nb, 1250.0), np.full(nb, 0.47),
                             angles, np.full(na, 25.0), np.full(na, 2.3), dtype=torch.float64)

    star = lambda k: [(0, j) if j % 2 else (j, 0) for j in range(1, k + 1)]  # noqa: E731
    fan = lambda k: [((0, j, j + 1), (j, 0, j + 1), (j, j + 1, 0))[j % 3] for j in range(1, k + 1)]  # noqa: E731
    assert create(30, star(8), fan(12)).n == 30
    with pytest.raises(_lib.MythosHipError, match="more than 8 bonds on one bead"):
        create(30, star(9), [])
    with pytest.raises(_lib.MythosHipError, match="more than 12 angles on one bead"):
        create(30, [], fan(13))
    with pytest.raises(_lib.MythosHipError, match="bad bond"):
        create(30, [(1, 2), (3, 3)], [])
    with pytest.raises(_lib.MythosHipError, match="bad bond"):
        create(30, [(1, 2), (29, 30)], [])
    with pytest.raises(_lib.MythosHipError, match="bad angle"):
        create(30, [], [(1, 2, 30)])


# ---- MD path -----------------------------------------------------------------------------------------------------------
def _builder(n, box, r_list):
    """The row builder mm_rebuild chooses (cell_grid, cell_list.h): all pairs under 512 beads or under three cells on an
    edge; else cells, in a direct-mapped table while there are at most 8 n of them, in a hashed one above."""
    nc = np.floor(np.asarray(box) / r_list).astype(int)
    if n < 512 or (nc < 3).any():
        return "allpairs", nc
    return ("direct" if int(nc.prod()) <= 8 * n else "hashed"), nc


def _workgroups(n):
    """(workgroups with beads, beads in the last one, blocks launched): the XCD-ordered map rounds the grid up to 8."""
    blocks = -(-n // MD_PPB)
    return blocks, n - (blocks - 1) * MD_PPB, 8 * (-(-blocks // 8))


def _integrator(s, sysm, *, dt=0.01, gamma=2.0, skin=0.25, every=2, inner=None, seed=SEED):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    integ = MartiniLangevinIntegrator(sysm, dt=dt, kT=KB * T, gamma=gamma, mass=s["mass"], seed=seed)
    integ.set_neighbor_policy(skin, every)
    if inner is not None:
        integ.set_inner_list(*inner)
    return integ


def _rows_against_brute_force(s, integ, x, r_list):
    """The Verlet rows after load + advance(1) (built at the loaded positions) against all minimum-image pairs in NumPy:
    every unbonded pair inside r_l - 1e-9 is there, nothing beyond r_l + 1e-9, no duplicate, no self, no bonded partner."""
    rows, lens = integ.rows(False)
    bonded = S.bonded_mask(s)
    box = s["box"][0]
    out = []
    for i0, r in S.pair_distances(np.asarray(x, dtype=np.float64), box):
        for k in range(r.shape[0]):
            i = i0 + k
            got = rows[i, :lens[i]].tolist()
            have = set(got)
            must = set(np.nonzero((r[k] < r_list - 1e-9) & ~bonded[i])[0].tolist())
            may = set(np.nonzero(r[k] < r_list + 1e-9)[0].tolist())
            assert len(have) == len(got) and i not in have and not (have & set(np.nonzero(bonded[i])[0].tolist())), i
            assert must <= have <= may, (i, sorted(must - have), sorted(have - may))
            out.append(have)
    return out, lens


def _steps_against_oracle(s, sysm, n_steps, angle_kind, x0, **policy):
    from oracle.martini_langevin_oracle import MartiniLangevinOracle

    integ = _integrator(s, sysm, **policy)
    b0 = s["box"][0].copy()
    pos = _dev(x0, sysm)
    vel = integ.init_velocities()
    v0 = vel.cpu().numpy().copy()
    traj, et = integ.run(pos, vel, b0, n_steps, save_every=1)
    a = S.oracle_args(s)
    orc = MartiniLangevinOracle(*a[2:], angle_kind == 0, b0, policy.get("dt", 0.01), KB * T, policy.get("gamma", 2.0), s["mass"], seed=SEED)
    xo, vo = np.array(x0, dtype=np.float64), v0.copy()
    e_ref = orc.run(xo, vo, n_steps)
    print(f"  {n_steps} steps: max |dx| {np.abs(pos.cpu().numpy() - xo).max():.2e} |dv| {np.abs(vel.cpu().numpy() - vo).max():.2e} "
          f"|dE| {np.abs(et.cpu().numpy() - e_ref).max():.2e}; moved {np.abs(xo - x0).max():.3f} nm, recoveries {integ.last_recoveries()}")
    np.testing.assert_allclose(pos.cpu().numpy(), xo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(vel.cpu().numpy(), vo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(et.cpu().numpy(), e_ref, rtol=1e-9, atol=1e-7)
    assert traj.shape == (n_steps, s["n"], 3)
    return traj.cpu().numpy()


def _first_rows(s, sysm, x0, r_list, **policy):
    integ = _integrator(s, sysm, **policy)
    pos = _dev(x0, sysm)
    integ.load(pos, integ.init_velocities(), s["box"][0])
    integ.advance(1)
    return _rows_against_brute_force(s, integ, pos.cpu().numpy(), r_list)


@pytest.mark.parametrize("angle_kind", [0, 1], ids=["g96", "harmonic"])
def test_md_small_system_allpairs_builder_partial_workgroup(angle_kind):
    """(e) 37 beads, unwrapped by up to two boxes: mm_build_rows_allpairs_kernel, three workgroups of the step kernel of
    which the last holds five beads (valid == false, ii = n - 1, ib < n), and five of the eight blocks launched return at
    bid >= n_blocks.  Five steps against the oracle; the same again from the wrapped beads: the same rows, the same
    trajectory up to the whole boxes."""
    s = S.get("md37")
    S.check(s)
    skin = 0.2
    assert _builder(s["n"], s["box"][0], R_C + skin)[0] == "allpairs" and s["n"] < 512
    assert _workgroups(s["n"]) == (3, 5, 8) and np.abs(s["shift"]).max() == 2
    sysm = _system(s, torch.float64, angle_kind)
    x0 = s["pos"][0]
    xw = x0 - s["shift"] * s["box"][0]
    assert (xw > 0).all() and (xw < s["box"][0]).all()
    policy = dict(skin=skin, every=2)
    rows, lens = _first_rows(s, sysm, x0, R_C + skin, **policy)
    rows_w, _ = _first_rows(s, sysm, xw, R_C + skin, **policy)
    assert rows == rows_w and (lens > 0).all()
    traj = _steps_against_oracle(s, sysm, 5, angle_kind, x0, **policy)
    traj_w = _steps_against_oracle(s, sysm, 5, angle_kind, xw, **policy)
    np.testing.assert_allclose(traj_w + s["shift"] * s["box"][0], traj, rtol=0, atol=1e-9)


def test_md_cell_builder_direct_table_partial_workgroup():
    """(f) 1 285 beads, four cells per edge in a direct-mapped table: 81 workgroups, the last with five beads, in a grid
    of 88; the cell-row kernel's last workgroup is partial too (16 beads each)."""
    s = S.get("md1285")
    S.check(s)
    skin = 0.25
    kind, nc = _builder(s["n"], s["box"][0], R_C + skin)
    assert kind == "direct" and (nc >= 3).all() and _workgroups(s["n"]) == (81, 5, 88)
    sysm = _system(s, torch.float64, 0)
    _first_rows(s, sysm, s["pos"][0], R_C + skin, skin=skin, every=2)
    _steps_against_oracle(s, sysm, 3, 0, s["pos"][0], skin=skin, every=2)


def test_md_slab_takes_the_allpairs_builder_above_512_beads():
    """(g) 1 285 beads in a box two cells thick: z edge in [2 r_l, 3 r_l)."""
    s = S.get("slab1285")
    S.check(s)
    skin = 0.25
    r_l = R_C + skin
    kind, nc = _builder(s["n"], s["box"][0], r_l)
    assert kind == "allpairs" and s["n"] >= 512 and 2 * r_l <= s["box"][0][2] < 3 * r_l and nc[2] == 2 and (nc[:2] >= 3).all()
    sysm = _system(s, torch.float64, 1)
    _first_rows(s, sysm, s["pos"][0], r_l, skin=skin, every=2)
    _steps_against_oracle(s, sysm, 2, 1, s["pos"][0], skin=skin, every=2)


def test_md_dilute_system_takes_the_hashed_cell_table():
    """(h) 520 beads in eight blobs in a 24 nm box: 17^3 cells, more than 8 n, so buckets are found by hash (!g.direct) and
    a candidate counts only for the cell it lies in."""
    s = S.get("dilute520")
    S.check(s)
    skin = 0.3
    kind, nc = _builder(s["n"], s["box"][0], R_C + skin)
    assert kind == "hashed" and (nc == 17).all() and 17**3 > 8 * s["n"] and s["n"] >= 512
    sysm = _system(s, torch.float64, 0)
    _, lens = _first_rows(s, sysm, s["pos"][0], R_C + skin, skin=skin, every=2)
    assert (lens > 0).sum() >= 400
    _steps_against_oracle(s, sysm, 3, 0, s["pos"][0], skin=skin, every=2)


@pytest.mark.parametrize("name,skin", [("md37", 0.2), ("md1285", 0.25)])
def test_md_fp32_energies_on_partial_workgroups(name, skin):
    """(i) fp32 on (e) and (f): one step with dt -> 0 moves nothing, so the saved energies are those of the loaded beads:
    equal to the all-pairs energy kernel's (2e-5) and to the oracle's on the fp32-rounded inputs (1e-3).  Then 20
    thermostatted steps: every position finite, the beads of the partial workgroup have moved."""
    s = S.get(name)
    S.check(s)
    assert _workgroups(s["n"])[1] == 5
    sysm = _system(s, torch.float32, 0)
    x0, b0 = s["pos"][0], s["box"][0]
    integ = _integrator(s, sysm, dt=1e-9, gamma=0.0, skin=skin, every=2, seed=1)
    pos = _dev(x0, sysm)
    start = pos.clone()
    _, et = integ.run(pos, torch.zeros_like(pos), b0, 1, save_every=1)
    got = et[0, :3].cpu().numpy()
    e, _ = sysm.energy(start, _dev(b0, sysm), grads=False)
    e = e.cpu().numpy()
    e_ref = _reference(name, 0, 0, True)["e"]
    print(f"  {name}: step kernel {got}, energy kernel {e}, oracle {e_ref}")
    np.testing.assert_allclose(got, e, rtol=2e-5, atol=2e-5 * np.abs(e).max())
    np.testing.assert_allclose(got, e_ref, rtol=1e-3, atol=1e-3 * np.abs(e_ref).max())
    integ = _integrator(s, sysm, skin=skin, every=2)
    vel = integ.init_velocities()
    integ.run(pos, vel, b0, 20)
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all()
    assert ((pos - start).abs().max(dim=1).values[-5:] > 0).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_md_pruned_rows_on_a_partial_workgroup(dtype):
    """(j) set_inner_list(0.2, 4) on (f) with a skin of 0.4 nm: the EMIT launch writes, and the three launches behind it
    walk, the pruned rows of a last workgroup with five beads.  For beads 1 270 ... 1 284 the pruned row is the subsequence
    of the Verlet row inside r_c + margin; the trajectory is the unpruned one; split calls are bitwise equal."""
    s = S.get("md1285")
    S.check(s)
    skin, margin, n = 0.4, 0.2, s["n"]
    assert _builder(n, s["box"][0], R_C + skin)[0] == "direct" and _workgroups(n) == (81, 5, 88) and 0 < margin < skin
    sysm = _system(s, dtype, 0)
    x0, b = s["pos"][0], s["box"][0]

    def fresh(inner=(margin, 4)):
        # (a time step of 1 fs: the lattice starts far from equilibrium, and a bead may move (margin / 2) / 3 per step)
        integ = _integrator(s, sysm, dt=0.001, gamma=1.0, skin=skin, every=8, inner=inner, seed=31)
        pos = _dev(x0, sysm)
        vel = integ.init_velocities()
        integ.load(pos, vel, b)
        return integ, pos, vel

    integ, pos, vel = fresh()
    integ.advance(1)
    rows, lens = integ.rows(False)
    rows_in, lens_in = integ.rows(True)
    xk = pos.cpu().numpy().astype(np.float64)  # the positions as the kernel saw them
    for i in range(1270, n):
        j = rows[i, :lens[i]]
        d = xk[i] - xk[j]
        d -= b * np.round(d / b)
        r2 = (d * d).sum(1)
        edge = np.abs(np.sqrt(r2) - (R_C + margin)) < (1e-5 if dtype == torch.float32 else 1e-12)  # (rounding at the very edge)
        keep = r2 < (R_C + margin) ** 2
        got = rows_in[i, :lens_in[i]]
        if edge.any():
            assert set(j[keep & ~edge]) <= set(got) <= set(j[keep | edge]), i
        else:
            assert np.array_equal(got, j[keep]), i
        assert 0 < lens_in[i] < lens[i]
    n_steps = 12
    integ, pos, vel = fresh()
    tr_on, _ = integ.advance(n_steps, save_every=1, want_energy=False)
    assert integ.last_recoveries() == 0
    integ, pos, vel = fresh(inner=(0.0, 0))
    tr_off, _ = integ.advance(n_steps, save_every=1, want_energy=False)
    tol = 2e-4 if dtype == torch.float32 else 1e-10
    print(f"  pruned against unpruned, {n_steps} steps: {(tr_on - tr_off).abs().max().item():.2e} (bound {tol:.0e})")
    assert (tr_on - tr_off).abs().max().item() < tol
    integ, pos, vel = fresh()
    integ.advance(5)
    integ.advance(7)
    integ.store(pos, vel)
    assert torch.equal(tr_on[-1], pos)
