"""GPU tests of the MARTINI temperature ensemble (MartiniEnsembleIntegrator / mythos_martini_langevin_create_ensemble).

The invariant: replica r of an ensemble is, bit for bit, the single integrator made with seed_r and kT_r and loaded with
box_r - positions, velocities, saved rows, energy rows, last_boxes, pressure(), the neighbour rows and init_velocities -
as long as neither side reports a recovery.  The single integrator is the yardstick: its code path is the parent's, pinned
to MartiniLangevinOracle by tests/test_gpu_martini_md.py and tests/test_gpu_martini_npt.py.

  1  md37 x 5 (all-pairs builder, three workgroups per replica, the last with 5 of 16 beads): energy rows and plain rows,
     pruned rows on and off
  2  md1285 x 3 (direct cells, partial last workgroup), slab1285 x 2 (harmonic angle), dilute520 x 2 (hashed table)
  3  the bilayer x 2 with charges: the ensemble and the Coulomb instantiations together
  4  NPT: c-rescale semi-isotropic and Berendsen isotropic on md1285 x 3; boxes diverge
  5  split calls equal one call, with and without a barostat
  6  a skin the hottest replica leaves early: recoveries happen, the call completes, split equals unsplit, and the energy
     rows are the oracle's energies of the saved positions in the replica's box
  7  a coupling event that would push ONE replica's box under the limit: the error names it, nobody is scaled
  8  R = 1 on the ensemble path
"""

import functools

import numpy as np
import pytest
import torch

from tests import martini_helpers as MH
from tests import martini_synth as S

pytestmark = pytest.mark.gpu

KB = 0.0083144626
KT = KB * 273.0
SEEDS = [0xABCDEF012345, 7, 2**63 + 11, 12345678901234567, 3]
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(n, ff, angle_kind, mass, pos, box, charges): the systems of tests/test_gpu_martini_npt.py."""
    if name == "bilayer":
        s = MH.system()
        x, box, _ = MH.frames("lj")
        top = s["top"]
        ff = (s["types"], s["sigma"], s["eps"], np.asarray(top.bonded_neighbors), s["bond_k"], s["bond_r0"], np.asarray(top.angles),
              s["angle_k"], s["angle_t0"])
        return dict(n=len(s["types"]), ff=ff, angle_kind=0, mass=np.random.default_rng(5).uniform(40.0, 90.0, size=len(s["types"])),
                    pos=x[3].astype(np.float64), box=box[3].astype(np.float64), charges=np.asarray(top.charges, dtype=np.float64))
    s = S.get(name)
    ff = tuple(s[k] for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0"))
    return dict(n=s["n"], ff=ff, angle_kind=1 if name == "slab1285" else 0, mass=s["mass"], pos=s["pos"][0], box=s["box"][0], charges=None)


def _system(c, dtype, charged=False):
    from mythos_amd.hip_system import MartiniSystem

    sysm = MartiniSystem(*c["ff"], angle_kind=c["angle_kind"], dtype=dtype)
    if charged:
        sysm.set_charges(c["charges"])
    return sysm


def _boxes(c, n_rep):
    """Replica boxes enlarged by 0 - 3 % per replica and axis, never shrunk (md37's shortest edge sits on the limit);
    replica 0 keeps the system's box."""
    f = 1.0 + 0.03 * np.random.default_rng(17).uniform(size=(n_rep, 3))
    f[0] = 1.0
    return c["box"][None, :] * f


def _start(c, box):
    """The system's positions scaled with the replica's box (bonds of the lattices cross the periodic boundary: a larger
    box around unscaled positions would stretch them by the whole enlargement)."""
    return c["pos"] * (np.asarray(box) / c["box"])


def _setup(integ, cfg):
    integ.set_neighbor_policy(*cfg["policy"])
    if cfg.get("inner"):
        integ.set_inner_list(*cfg["inner"])
    if cfg.get("baro"):
        integ.set_barostat(**cfg["baro"])


def _drive(integ, pos, boxes, calls, save_every, want_energy, with_rows):
    """init_velocities; load; advance(n) for n in calls; pressure; store -> dict: v0, the rows after the first call
    (with_rows; a call that ends on a coupling event leaves no list behind),
    out = {absolute step: (row, box row, energy row or None)}, the final state, recoveries summed over the calls."""
    vel = integ.init_velocities()
    v0 = vel.cpu().clone()
    integ.load(pos, vel, boxes)
    out, at, rec, rows, lens = {}, 0, 0, None, None
    for n in calls:
        traj, et = integ.advance(n, save_every=save_every, want_energy=want_energy)
        rec += integ.last_recoveries()
        lb = integ.last_boxes
        assert lb.shape[0] == (n // save_every if save_every else 0)
        for k in range(lb.shape[0]):
            out[at + (k + 1) * save_every] = (traj[k].cpu(), lb[k].cpu(), et[k].cpu() if et is not None else None)
        at += n
        if rows is None and with_rows:
            rows, lens = integ.rows()
    p = integ.pressure()
    integ.store(pos, vel)
    return dict(v0=v0, rows=rows, lens=lens, out=out, pos=pos.cpu(), vel=vel.cpu(), box=integ.box, p=p, recoveries=rec, step=integ.step,
                integ=integ)


def _run_singles(c, sysm, kTs, seeds, boxes, cfg, calls, save_every=0, want_energy=True):
    """One MartiniLangevinIntegrator per replica, one after the other."""
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    outs = []
    for kT, seed, box in zip(kTs, seeds, boxes):
        integ = MartiniLangevinIntegrator(sysm, dt=cfg["dt"], kT=kT, gamma=cfg["gamma"], mass=c["mass"], seed=seed)
        _setup(integ, cfg)
        pos = torch.tensor(_start(c, box), dtype=sysm.dtype, device=sysm.device).contiguous()
        outs.append(_drive(integ, pos, box, calls, save_every, want_energy, not cfg.get("baro")))
    return outs


def _run_ensemble(c, sysm, kTs, seeds, boxes, cfg, calls, save_every=0, want_energy=True):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    n_rep = len(kTs)
    integ = MartiniEnsembleIntegrator(sysm, dt=cfg["dt"], kT=kTs, gamma=cfg["gamma"], mass=c["mass"], seeds=seeds)
    _setup(integ, cfg)
    pos = torch.tensor(np.stack([_start(c, b) for b in boxes]), dtype=sysm.dtype, device=sysm.device).contiguous()
    return _drive(integ, pos, boxes, calls, save_every, want_energy, not cfg.get("baro"))


def _assert_replicas_are_the_singles(ens, singles, n):
    """Everything the invariant names, bitwise."""
    assert ens["recoveries"] == 0 and all(s["recoveries"] == 0 for s in singles)
    for r, s in enumerate(singles):
        sl = slice(r * n, (r + 1) * n)
        assert torch.equal(ens["v0"][r], s["v0"]), f"init_velocities of replica {r}"
        assert (ens["rows"] is None) == (s["rows"] is None)
        if s["rows"] is not None:
            np.testing.assert_array_equal(ens["lens"][sl], s["lens"])
            stride = min(ens["rows"].shape[1], s["rows"].shape[1])
            assert s["lens"].max() <= stride
            live = np.arange(stride)[None, :] < s["lens"][:, None]  # entry for entry, up to each row's length
            np.testing.assert_array_equal(ens["rows"][sl, :stride][live], s["rows"][:, :stride][live])
        assert torch.equal(ens["pos"][r], s["pos"]), f"positions of replica {r}"
        assert torch.equal(ens["vel"][r], s["vel"]), f"velocities of replica {r}"
        np.testing.assert_array_equal(ens["box"][r], s["box"])
        assert set(ens["out"]) == set(s["out"])
        for step, (row, box_row, e_row) in ens["out"].items():
            srow, sbox, se = s["out"][step]
            assert torch.equal(row[r], srow), (r, step)
            assert torch.equal(box_row[r], sbox), (r, step)
            assert (e_row is None and se is None) or torch.equal(e_row[r], se), (r, step)
        for key in ("kinetic", "virial", "pressure"):
            np.testing.assert_array_equal(ens["p"][key][r], s["p"][key])
        assert ens["p"]["volume"][r] == s["p"]["volume"] and ens["p"]["p"][r] == s["p"]["p"]
        assert ens["step"] == s["step"]


def _compare(name, dtype, n_rep, kTs, cfg, calls, save_every=0, want_energy=True, charged=False, boxes=None):
    c = _case(name)
    sysm = _system(c, dtype, charged)
    boxes = _boxes(c, n_rep) if boxes is None else boxes
    seeds = SEEDS[:n_rep]
    ens = _run_ensemble(c, sysm, kTs, seeds, boxes, cfg, calls, save_every, want_energy)
    singles = _run_singles(c, sysm, kTs, seeds, boxes, cfg, calls, save_every, want_energy)
    _assert_replicas_are_the_singles(ens, singles, c["n"])
    return ens, singles


@pytest.mark.parametrize("inner", [None, (0.12, 3)], ids=["verlet-rows", "pruned-rows"])
@pytest.mark.parametrize("want_energy", [True, False], ids=["energy-rows", "plain-rows"])
@DTYPES
def test_md37_five_replicas_are_five_single_runs_bitwise(dtype, want_energy, inner):
    """md37 x 5: all-pairs builder, 15 workgroups on a grid padded to 16, kT 2.0 ... 3.2, skin 0.25 rebuilt every 2 steps
    (the npt tests' 0.2 widened as far as md37's box allows: replica 0 keeps the box whose shortest edge is
    2 (r_cut + 0.25)), 24 steps, rows every 4.  dt 0.002: at 0.01 the single integrator at kT 3.2 itself leaves the skin
    (4 recoveries in 24 steps, measured), which the invariant excludes."""
    cfg = dict(dt=0.002, gamma=2.0, policy=(0.25, 2), inner=inner)
    ens, _ = _compare("md37", dtype, 5, np.linspace(2.0, 3.2, 5), cfg, [24], save_every=4, want_energy=want_energy)
    assert len(ens["out"]) == 6
    if inner:
        rows_in, lens_in = ens["integ"].rows(pruned=True)
        assert rows_in.shape[0] == 5 * 37 and (lens_in <= ens["lens"]).all() and lens_in.sum() < ens["lens"].sum()


# The lattices of tests/martini_synth.py start far from equilibrium: a time step of 1 fs and the skin of 0.4 nm that
# tests/test_gpu_martini_shapes.py runs them with (0.35 where the slab's height of 3.0 nm asks for it).
LATTICE = dict(dt=0.001, gamma=2.0, policy=(0.4, 3))


@pytest.mark.parametrize("name,n_rep,skin", [("md1285", 3, 0.4), ("slab1285", 2, 0.35), ("dilute520", 2, 0.4)])
@DTYPES
def test_cell_builders_three_systems(dtype, name, n_rep, skin):
    """Direct cell table with a partial last workgroup per replica (1 285 = 80 x 16 + 5), the harmonic angle with two cells
    in z, the hashed table: 12 steps, rows rebuilt every 3, get_rows equal entry for entry after the first build."""
    cfg = dict(LATTICE, policy=(skin, 3))
    _compare(name, dtype, n_rep, KT * np.linspace(1.0, 1.2, n_rep), cfg, [12], save_every=4)


@DTYPES
def test_charged_bilayer_two_replicas(dtype):
    """The ensemble and the reaction-field instantiations together: five trace columns, the Coulomb one bitwise too."""
    cfg = dict(dt=0.01, gamma=2.0, policy=(0.3, 3), inner=(0.15, 3))
    ens, _ = _compare("bilayer", dtype, 2, [KT, 1.17 * KT], cfg, [12], save_every=4, charged=True)
    e = ens["out"][12][2]
    assert e.shape == (2, 5) and (e[:, 4] != 0).all() and not torch.equal(e[0], e[1])


# Compressibility 1e-7 / bar: f = beta every dt / tau_p = 6e-10 / bar keeps |ln mu| under 0.02 per event up to 1e8 bar - the
# lattice's pressure is far from 1 bar - while the noise term of c-rescale, sqrt(2 kT' f / V) / 3 ~ 5e-6, moves every edge.
NPT = {
    "crescale-semi": dict(kind="c-rescale", coupling="semiisotropic", ref_p=(1.0, 1.0), compressibility=(1e-7, 1e-7), tau_p=0.5, every=3),
    "berendsen-iso": dict(kind="berendsen", coupling="isotropic", ref_p=1.0, compressibility=1e-7, tau_p=0.5, every=3),
}


@pytest.mark.parametrize("want_energy", [True, False], ids=["energy-rows", "plain-rows"])
@pytest.mark.parametrize("mode", list(NPT))
@DTYPES
def test_npt_three_replicas_own_boxes(dtype, mode, want_energy):
    """md1285 x 3 at kT, 1.1 kT, 1.2 kT from ONE box, coupling every 3 steps, 18 steps = six events, rows every 3 (each
    the state before the event of its step): states, last_boxes and pressure() bitwise, and the boxes have diverged."""
    c = _case("md1285")
    cfg = dict(LATTICE, baro=NPT[mode])
    boxes = np.broadcast_to(c["box"], (3, 3)).copy()
    ens, _ = _compare("md1285", dtype, 3, KT * np.array([1.0, 1.1, 1.2]), cfg, [18], save_every=3, want_energy=want_energy, boxes=boxes)
    b = ens["box"]
    print(f"  {mode}: box / box_0 - 1 per replica {(b / c['box'] - 1.0).tolist()}")
    assert (b != c["box"]).all()
    assert not np.array_equal(b[0], b[1]) and not np.array_equal(b[1], b[2]) and not np.array_equal(b[0], b[2])
    np.testing.assert_array_equal(ens["out"][3][1].numpy(), boxes)  # the row of step 3: before the first event
    lb = ens["integ"].last_boxes
    assert lb.shape == (6, 3, 3) and lb.dtype == torch.float64


@pytest.mark.parametrize("baro", [None, "crescale-semi"], ids=["nvt", "npt"])
@DTYPES
def test_split_calls_equal_one_call(dtype, baro):
    """advance(5); advance(7); advance(6) against advance(18) inside the ensemble, and either against the single runs."""
    c = _case("md1285")
    sysm = _system(c, dtype)
    cfg = dict(LATTICE, baro=NPT[baro] if baro else None)
    kTs, boxes = KT * np.array([1.0, 1.2]), _boxes(c, 2)
    one = _run_ensemble(c, sysm, kTs, SEEDS[:2], boxes, cfg, [18], save_every=2)
    split = _run_ensemble(c, sysm, kTs, SEEDS[:2], boxes, cfg, [5, 7, 6], save_every=2)
    assert one["recoveries"] == 0 and split["recoveries"] == 0
    assert torch.equal(one["pos"], split["pos"]) and torch.equal(one["vel"], split["vel"])
    np.testing.assert_array_equal(one["box"], split["box"])
    shared = sorted(set(one["out"]) & set(split["out"]))
    assert set(shared) >= {2, 4, 14, 16, 18}  # (rows count from the first step of their call)
    for s in shared:
        for a, b in zip(one["out"][s], split["out"][s]):
            assert torch.equal(a, b), s
    singles = _run_singles(c, sysm, kTs, SEEDS[:2], boxes, cfg, [5, 7, 6], save_every=2)
    _assert_replicas_are_the_singles(split, singles, c["n"])


def test_r_equal_one_is_the_single_integrator():
    cfg = dict(LATTICE, baro=NPT["crescale-semi"])
    for dtype in (torch.float64, torch.float32):
        _compare("md1285", dtype, 1, [1.1 * KT], cfg, [9], save_every=3)


def test_a_thin_skin_recovers_and_split_still_equals_unsplit():
    """md1285 x 2 in fp64, kT and 1.6 kT, dt 1 fs, skin 0.01 nm (thermal speeds of 0.3 nm/ps cross 0.005 nm in under 20 steps) and no scheduled rebuild inside the call: the hot replica leaves
    its skin first, every replica is rebuilt, the call completes.  Recoveries are the precondition.  Split equals unsplit
    bitwise: a halt and the launch that resumes are functions of the state.  Against single runs no bitwise match is
    claimed here - a single cold replica would not have rebuilt where the hot one forced it to - so the energy rows are
    checked against the oracle at the saved positions in the replica's box, at the tolerances of the trace comparison of
    tests/test_gpu_martini_md.py (rtol 1e-9, atol 1e-7)."""
    from oracle import martini_oracle as MO

    c = _case("md1285")
    sysm = _system(c, torch.float64)
    cfg = dict(dt=0.001, gamma=1.0, policy=(0.01, 1000))
    kTs, boxes = KT * np.array([1.0, 1.6]), _boxes(c, 2)
    one = _run_ensemble(c, sysm, kTs, SEEDS[:2], boxes, cfg, [30], save_every=10)
    split = _run_ensemble(c, sysm, kTs, SEEDS[:2], boxes, cfg, [10, 20], save_every=10)
    print(f"  recoveries: one call {one['recoveries']}, split {split['recoveries']}")
    assert one["recoveries"] > 0 and split["recoveries"] > 0
    assert one["step"] == 30 and split["step"] == 30
    assert torch.equal(one["pos"], split["pos"]) and torch.equal(one["vel"], split["vel"])
    for s in (10, 20, 30):
        for a, b in zip(one["out"][s], split["out"][s]):
            assert torch.equal(a, b), s
    tt = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    t, sg, ep, b, bk, br, an, ak, at = c["ff"]
    for s in (10, 20, 30):  # every saved row
        row, box_row, e_row = one["out"][s]
        for r in range(2):
            ref, _ = MO.energies_and_forces(row[r].double(), box_row[r].double(), torch.as_tensor(np.asarray(t), dtype=torch.long), tt(sg),
                                            tt(ep), b, tt(bk), tt(br), an, tt(ak), tt(at), True)
            got = e_row[r, :3].numpy()
            print(f"  step {s} replica {r}: trace {got}, oracle {ref.numpy()}")
            np.testing.assert_allclose(got, ref.numpy(), rtol=1e-9, atol=1e-7)


def test_a_replica_box_under_the_limit_names_the_replica_and_scales_nobody():
    """Three ideal gases of 64 beads (the single-copy test's), boxes 4.0, 2.45 and 4.0 nm, r_cut + skin = 1.2 nm: Berendsen
    at every step towards eight times the pressure of the 4 nm box shrinks every box by 4 - 11 %, which takes replica 1 -
    and only it - under 2.4 nm.  The call ends at step 1 naming replica 1; all three keep their boxes and the unscaled
    state of that step, which is the state a run without a barostat reaches, bit for bit."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniSystem

    n, kT, edge = 64, 2.27, np.array([4.0, 2.45, 4.0])
    z = np.zeros(0)
    sysm = MartiniSystem(np.zeros(n, dtype=np.int32), np.array([[0.47]]), np.array([[0.0]]), np.zeros((0, 2), np.int32), z, z,
                         np.zeros((0, 3), np.int32), z, z, r_cut=1.1, dtype=torch.float64)
    p0 = n * kT / 4.0**3 * 16.6053907
    boxes = np.repeat(edge[:, None], 3, axis=1)
    u = np.random.default_rng(3).uniform(0.0, 1.0, size=(3, n, 3))
    states = []
    for baro in (True, False):
        integ = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=[kT] * 3, gamma=1.0, seeds=77)
        integ.set_neighbor_policy(0.1, 10)
        if baro:
            integ.set_barostat("berendsen", "isotropic", ref_p=8.0 * p0, compressibility=0.05 / (p0 * 0.02), tau_p=1.0, every=1)
        pos = torch.tensor(u * edge[:, None, None], dtype=torch.float64, device=sysm.device)
        vel = integ.init_velocities()
        integ.load(pos, vel, boxes)
        if baro:
            with pytest.raises(ValueError, match=r"box of replica 1 smaller than twice \(r_cut \+ skin\)"):
                integ.advance(50, save_every=1, want_energy=False)
            # the rows saved before the refusal stay, the same number in every log
            assert integ.last_boxes.shape[0] == integ.last_ladder.shape[0] == integ.last_windows.shape[0]
        else:
            integ.advance(1)
        assert integ.step == 1
        np.testing.assert_array_equal(integ.box, boxes)
        p1, v1 = torch.empty_like(pos), torch.empty_like(vel)
        integ.store(p1, v1)
        assert torch.isfinite(p1).all() and 0 < (p1 - pos).abs().max() < 0.1
        states.append((p1.cpu(), v1.cpu()))
        if baro:
            integ.set_barostat(None)
            integ.advance(5)
            assert integ.step == 6
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
