"""GPU tests of window exchange in the MARTINI ensemble (MartiniEnsembleIntegrator.set_window_exchange /
mythos_martini_langevin_set_window_exchange; the rule is stated in include/mythos_hip.h and restated in
tests/martini_window_exchange_ref.py): Hamiltonian replica exchange between the parameter rows of the installed restraints.

The yardstick is that of tests/test_gpu_martini_exchange.py: between two events a run with window exchange IS the plain
ensemble - restarted at the event's step, given set_restraints with the rows as the log permuted them, loaded with the
stored state - bit for bit, because an event drops the neighbour rows as a load does.

  1  the log against the rule (n257, every term kind, R = 2, 3, 5, the step counter started at 12 345)
  2  window exchange = plain ensemble runs glued by the rule      5  set_windows against set_restraints with permuted rows
  3  identical windows                                            6  statistics of 64 distinct windows on free beads
  4  split calls; switched off again                              7  HipMartiniSimulator       8  refusals through the handle
"""

import dataclasses as dc
import functools
import math

import numpy as np
import pytest
import torch

from mythos_amd.simulators.martini_restraints import MartiniRestraints, PullCoordinate, PullGroup, round_trips
from tests import martini_restraints_cases as CS
from tests import martini_window_exchange_ref as W
from tests.test_gpu_martini_restraints import DTYPES, KT, _bilayer, _dev, _ensemble, _ff, _system, _tolerances

pytestmark = pytest.mark.gpu

SEEDS = [0xABCDEF012345, 7, 2**63 + 11, 99, 2**40 + 3]
STEP0, EVERY, STEPS, XSEED = 12345, 5, 40, 77  # 12 345 is a multiple of 5: rows saved every 5 steps fall on the events


@functools.lru_cache(maxsize=None)
def _case(n_rep, identical=False):
    """n257 for ``n_rep`` replicas: the same start in every slot, boxes that differ by 0.1 % per replica (minimum images are
    the configuration's own), and the set with every term kind (tests/martini_restraints_cases.py, "full") made
    window-wise: init and k of the two umbrella coordinates per window, the references left None - half the position
    restraints and a flat-bottom term - from per-window reference states up to 0.002 nm per axis apart.  The windows are
    close enough for exchanges to be accepted: the cross terms of d scale with the distance between two windows."""
    c, full = CS.n257(), CS.sets()["full"]
    w = np.arange(n_rep, dtype=np.float64)
    boxes = c["boxes"][0][None, :] * (1.0 + 0.001 * w)[:, None]
    pos = np.broadcast_to(c["pos"][0], (n_rep, c["n"], 3)).copy()
    ref = c["ref"][0][None] + np.random.default_rng(7).uniform(-0.002, 0.002, size=(n_rep, c["n"], 3))
    init = [0.4 + 0.01 * w, -0.2 + 0.01 * w]
    k = [1500.0 - 20.0 * w, 800.0 + 30.0 * w]
    if identical:
        ref = np.broadcast_to(ref[0], ref.shape).copy()
        boxes = np.broadcast_to(boxes[0], boxes.shape).copy()
        init, k = [np.full(n_rep, v[0]) for v in init], [np.full(n_rep, v[0]) for v in k]
    pulls = [dc.replace(p, init=tuple(init[j]), k=tuple(k[j])) if j < 2 else p for j, p in enumerate(full.pulls)]
    assert pulls[0].rate != 0.0 and pulls[1].rate != 0.0
    return dict(c=c, rs=dc.replace(full, pulls=pulls), boxes=boxes, pos=pos, ref=ref, n_rep=n_rep)


def _permuted(case, windows):
    """(set, reference state) whose replica s carries the row of window windows[s]."""
    windows = np.asarray(windows, dtype=np.int64)
    pick = lambda v: tuple(np.asarray(v, dtype=np.float64)[windows]) if np.ndim(v) else v  # noqa: E731
    rs = case["rs"]
    return dc.replace(rs, pulls=[dc.replace(p, init=pick(p.init), k=pick(p.k)) for p in rs.pulls]), case["ref"][windows]


def _make(case, sysm, windows=None, exchange=None):
    n_rep = case["n_rep"]
    integ = _ensemble(sysm, case["c"]["masses"], [KT] * n_rep, seeds=SEEDS)
    if exchange:
        integ.set_window_exchange(*exchange)
    rs, ref = _permuted(case, np.arange(n_rep) if windows is None else windows)
    integ.set_restraints(rs, reference_pos=ref, box=case["boxes"])
    return integ


def _drive(integ, pos, vel, boxes, calls, save_every=EVERY, want_energy=True):
    """load; advance(n) for n in calls; store -> rows / energy rows / assignment rows by absolute step, the logs
    concatenated, the final state."""
    integ.load(pos, vel, boxes)
    rows, log, at, rec, launches = {}, [], integ.step, 0, 0
    for n in calls:
        traj, et = integ.advance(n, save_every=save_every, want_energy=want_energy)
        rec += integ.last_recoveries()
        launches += integ.last_kernel_ms()["launches"]
        lw = integ.last_windows
        n_rows = n // save_every if save_every else 0
        assert lw.shape == (n_rows, integ.n_rep) and lw.dtype == torch.int64 and lw.device == pos.device
        for j in range(n_rows):
            rows[at + (j + 1) * save_every] = (traj[j].cpu(), et[j].cpu() if et is not None else None, lw[j].cpu().numpy())
        log.append(integ.last_window_exchanges)
        at += n
    integ.store(pos, vel)
    log = {key: np.concatenate([l[key] for l in log]) for key in log[0]}
    return dict(rows=rows, log=log, pos=pos.cpu(), vel=vel.cpu(), windows=integ.windows, recoveries=rec, step=integ.step, integ=integ,
                launches=launches, counts=integ.window_exchange_counts())


@functools.lru_cache(maxsize=None)
def _run(dtype, n_rep, identical=False):
    """The shared run of tests 1 - 4: n257 x n_rep, window exchange every 5 steps from step 12 345, 40 steps, rows every 5."""
    case = _case(n_rep, identical)
    sysm = _system(_ff(case["c"]["s"]), dtype)
    integ = _make(case, sysm, exchange=(EVERY, XSEED))
    integ.restart(SEEDS[:n_rep], step=STEP0)
    vel = integ.init_velocities()
    out = _drive(integ, _dev(case["pos"], sysm), vel.clone(), case["boxes"], [STEPS])
    out.update(v0=vel.cpu(), case=case)
    return out


def _swapped(windows, pairs):
    new = np.array(windows).copy()
    for a, b in pairs:
        new[a], new[b] = windows[b], windows[a]
    return new


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n_rep", [2, 3, 5])
def test_the_log_is_the_rule(dtype, n_rep):
    """Every record of the log against the reference on the saved state of its step: the four cross energies to the bound
    of test_field_and_energies_of_three_replicas_against_the_reference (1e-12 of the scale plus the summation-order
    bound; fp32: the reference in double on the stored fp32 positions), u exactly, d to that bound, the decision from the
    logged d and u, the assignment rows from the accepted pairs, the counts from the log.  R = 2 has attempts without a
    pair, R = 3 a window that sits out at either parity, R = 5 two pairs at both parities."""
    r = _run(dtype, n_rep)
    case, log, rows = r["case"], r["log"], r["rows"]
    c, rs = case["c"], case["rs"]
    assert r["recoveries"] == 0 and r["step"] == STEP0 + STEPS
    steps = list(range(STEP0 + EVERY, STEP0 + STEPS + 1, EVERY))
    want_pairs = [(s, t) for s in steps for t in W.schedule(n_rep, s // EVERY)]
    assert list(zip(log["step"].tolist(), log["rung"].tolist())) == want_pairs and len(want_pairs) == {2: 4, 3: 8, 5: 16}[n_rep]
    worst = 0.0
    for j, (s, t) in enumerate(want_pairs):
        traj, _, windows = rows[s]
        a, b = int(log["slot_a"][j]), int(log["slot_b"][j])
        assert windows[a] == t and windows[b] == t + 1, (s, t)
        assert log["u"][j] == W.uniform(XSEED, t, s), (s, t)
        got = [log[key][j] for key in ("e_t_a", "e_t1_a", "e_t_b", "e_t1_b")]
        want, tol = [], []
        for slot, window in ((a, t), (a, t + 1), (b, t), (b, t + 1)):
            x = traj[slot].double().numpy()  # (the stored positions, widened: what the device read)
            (_, e, _), (_, te, _) = _tolerances(rs, x, c["masses"], case["boxes"][slot], s, window, case["ref"][window], dtype)
            assert e.sum() == pytest.approx(W.cross_energy(rs, x, c["masses"], case["boxes"][slot], s, CS.DT, window, case["ref"]), rel=1e-13)
            want.append(e.sum()), tol.append(te)
        for g, e, te in zip(got, want, tol):
            worst = max(worst, abs(g - e) / te)
            assert abs(g - e) <= te, (s, t, g, e, te)
        np.testing.assert_allclose(log["d"][j], W.delta(KT, *got), rtol=1e-12, atol=1e-300)
        assert abs(log["d"][j] - W.delta(KT, *want)) <= sum(tol) / KT, (s, t)
        assert bool(log["accepted"][j]) == W.accepts(log["d"][j], log["u"][j]), (s, t)
    n_acc = int(log["accepted"].sum())
    print(f"  R = {n_rep}: {n_acc} of {len(want_pairs)} accepted; worst |dE| / tol {worst:.2e}; d in [{log['d'].min():.3g}, {log['d'].max():.3g}]")
    for s in steps:
        sel = (log["step"] == s) & log["accepted"]
        after = _swapped(rows[s][2], list(zip(log["slot_a"][sel].tolist(), log["slot_b"][sel].tolist())))
        nxt = rows[s + EVERY][2] if s + EVERY in rows else r["windows"]
        np.testing.assert_array_equal(nxt, after, err_msg=f"assignment behind the event of step {s}")
    assert sorted(r["windows"].tolist()) == list(range(n_rep))
    attempts, accepts = r["counts"]
    for t in range(n_rep - 1):
        assert attempts[t] == (log["rung"] == t).sum() and accepts[t] == ((log["rung"] == t) & log["accepted"]).sum()


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------
def _hand_chain(dtype, case, v0, log=None):
    """Plain ensembles glued by the log through the API that existed before window exchange did: per segment advance(5) with
    a row at its end; store; a fresh ensemble restarted at the step with set_restraints of the rows permuted by the
    accepted pairs of the log (None: no swap), loaded with the stored state."""
    sysm = _system(_ff(case["c"]["s"]), dtype)
    n_rep = case["n_rep"]
    windows = np.arange(n_rep)
    pos, vel = _dev(case["pos"], sysm), v0.to(sysm.device).clone()
    rows, rec, s = {}, 0, STEP0
    while s < STEP0 + STEPS:
        integ = _make(case, sysm, windows=windows)
        integ.restart(SEEDS[:n_rep], step=s)
        integ.load(pos, vel, case["boxes"])
        traj, et = integ.advance(EVERY, save_every=EVERY, want_energy=True)
        rec += integ.last_recoveries()
        integ.store(pos, vel)
        s += EVERY
        rows[s] = (traj[0].cpu(), et[0].cpu(), windows.copy())
        if log is not None:
            sel = (log["step"] == s) & log["accepted"]
            windows = _swapped(windows, list(zip(log["slot_a"][sel].tolist(), log["slot_b"][sel].tolist())))
    return dict(rows=rows, pos=pos.cpu(), vel=vel.cpu(), windows=windows, recoveries=rec)


@DTYPES
def test_a_run_with_window_exchange_is_plain_ensemble_runs_glued_by_the_rule(dtype):
    """One advance(40) with window exchange on (R = 5) against the hand chain: saved rows, energy rows, final positions and
    velocities and the assignment, bit for bit; the assignment has moved; neither side reports a recovery."""
    r = _run(dtype, 5)
    h = _hand_chain(dtype, r["case"], r["v0"], r["log"])
    assert r["recoveries"] == 0 and h["recoveries"] == 0 and set(r["rows"]) == set(h["rows"])
    for s, (row, e_row, windows) in h["rows"].items():
        assert torch.equal(r["rows"][s][0], row), s
        assert torch.equal(r["rows"][s][1], e_row), s
        np.testing.assert_array_equal(r["rows"][s][2], windows)
    assert torch.equal(r["pos"], h["pos"]) and torch.equal(r["vel"], h["vel"])
    np.testing.assert_array_equal(r["windows"], h["windows"])
    assert r["log"]["accepted"].any() and not np.array_equal(h["windows"], np.arange(5))
    plain = _hand_chain(dtype, r["case"], r["v0"], None)
    assert not torch.equal(plain["pos"], h["pos"])  # and the exchanges do change the run


@DTYPES
def test_identical_windows_always_swap_and_change_nothing(dtype):
    """R = 3, every window the same row: the cross energies of a configuration are equal bit for bit, so d == 0.0 and every
    attempt is accepted; the assignment follows the odd-even transposition pattern; positions and velocities are those of
    the glued run, which with identical rows is the hand chain whatever it swaps."""
    r = _run(dtype, 3, True)
    log = r["log"]
    assert len(log["d"]) == 8 and (log["d"] == 0.0).all() and log["accepted"].all()
    assert (log["e_t_a"] == log["e_t1_a"]).all() and (log["e_t_b"] == log["e_t1_b"]).all()
    windows = np.arange(3)
    for s in range(STEP0 + EVERY, STEP0 + STEPS + 1, EVERY):
        np.testing.assert_array_equal(r["rows"][s][2], windows, err_msg=f"step {s}")
        for t in W.schedule(3, s // EVERY):
            a, b = int(np.nonzero(windows == t)[0][0]), int(np.nonzero(windows == t + 1)[0][0])
            windows[a], windows[b] = t + 1, t
    np.testing.assert_array_equal(r["windows"], windows)
    h = _hand_chain(dtype, r["case"], r["v0"], log)
    assert r["recoveries"] == 0 and h["recoveries"] == 0
    assert torch.equal(r["pos"], h["pos"]) and torch.equal(r["vel"], h["vel"])
    for s, (row, e_row, _) in h["rows"].items():
        assert torch.equal(r["rows"][s][0], row) and torch.equal(r["rows"][s][1], e_row), s


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_split_calls_equal_one_call(dtype):
    """advance(7); advance(13); advance(20) against advance(40), none of 7, 13, 20 + 7 a multiple of 5: events follow the
    absolute step counter, the logs concatenate to the one call's, the rows at shared steps, the final state, the assignment
    and the counts are equal bit for bit.  The split calls save plain rows: a row WITH energies at a step that is no event
    is issued as a closing and an opening launch with two external half kicks (csrc/martini_md.hip) where the one call
    issues one whole kick there, which rounds differently - by design, and not what is compared here."""
    r = _run(dtype, 3)
    case = r["case"]
    sysm = _system(_ff(case["c"]["s"]), dtype)
    integ = _make(case, sysm, exchange=(EVERY, XSEED))
    integ.restart(SEEDS[:3], step=STEP0)
    sp = _drive(integ, _dev(case["pos"], sysm), r["v0"].to(sysm.device).clone(), case["boxes"], [7, 13, 20], want_energy=False)
    assert sp["recoveries"] == 0 and sp["step"] == STEP0 + STEPS
    for key in r["log"]:
        np.testing.assert_array_equal(sp["log"][key], r["log"][key], err_msg=key)
    assert torch.equal(sp["pos"], r["pos"]) and torch.equal(sp["vel"], r["vel"])
    np.testing.assert_array_equal(sp["windows"], r["windows"])
    shared = sorted(set(sp["rows"]) & set(r["rows"]))
    assert shared == [STEP0 + 5, STEP0 + 25, STEP0 + 30, STEP0 + 35, STEP0 + 40]
    for s in shared:
        assert torch.equal(sp["rows"][s][0], r["rows"][s][0]) and sp["rows"][s][1] is None, s
        np.testing.assert_array_equal(sp["rows"][s][2], r["rows"][s][2])
    np.testing.assert_array_equal(sp["counts"][0], r["counts"][0])
    np.testing.assert_array_equal(sp["counts"][1], r["counts"][1])


@DTYPES
def test_switched_off_again_is_the_handle_that_never_had_it(dtype):
    case = _case(3)
    sysm = _system(_ff(case["c"]["s"]), dtype)
    outs = []
    for touched in (True, False):
        integ = _make(case, sysm)
        if touched:
            integ.set_window_exchange(EVERY, XSEED)
            integ.set_window_exchange(0)
        integ.restart(SEEDS[:3], step=STEP0)
        outs.append(_drive(integ, _dev(case["pos"], sysm), integ.init_velocities(), case["boxes"], [20]))
    a, b = outs
    assert len(a["log"]["step"]) == 0 and a["counts"][0].sum() == 0
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["vel"], b["vel"])
    assert a["launches"] == b["launches"] and a["launches"] > 0
    for s in b["rows"]:
        assert torch.equal(a["rows"][s][0], b["rows"][s][0]) and torch.equal(a["rows"][s][1], b["rows"][s][1])
        np.testing.assert_array_equal(a["rows"][s][2], np.arange(3))


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_set_windows_is_set_restraints_with_permuted_rows(dtype):
    case = _case(5)
    sysm = _system(_ff(case["c"]["s"]), dtype)
    pos = _dev(case["pos"] + np.random.default_rng(3).uniform(-0.02, 0.02, size=case["pos"].shape), sysm)
    moved = _make(case, sysm)
    np.testing.assert_array_equal(moved.windows, np.arange(5))
    for perm in ([2, 0, 4, 1, 3], [4, 3, 2, 1, 0], [0, 1, 2, 3, 4], [1, 2, 3, 4, 0]):  # each from the one before
        moved.set_windows(perm)
        np.testing.assert_array_equal(moved.windows, perm)
        direct = _make(case, sysm, windows=perm)
        for got, want in zip(moved.external_field(pos, step=STEP0), direct.external_field(pos, step=STEP0)):
            assert torch.equal(got, want), perm
    identity = _make(case, sysm).external_field(pos, step=STEP0)
    moved.set_windows([3, 1, 0, 2, 4])
    assert not torch.equal(moved.external_field(pos, step=STEP0)[1], identity[1])
    rs, ref = _permuted(case, np.arange(5))
    moved.set_restraints(rs, reference_pos=ref, box=case["boxes"])  # the assignment is the identity again
    np.testing.assert_array_equal(moved.windows, np.arange(5))
    assert torch.equal(moved.external_field(pos, step=STEP0)[1], identity[1])
    with pytest.raises(ValueError, match="window_of_slot must be a permutation"):
        moved.set_windows([0, 1, 1, 3, 4])


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_distinct_windows_sample_their_mean_and_variance_and_exchange_at_the_expected_rate():
    """The system of test_umbrella_windows_sample_their_mean_and_variance - free beads of 72 amu, k = 500, kT = 2.5,
    gamma = 3, dt = 0.02, policy (1.0, 10), 1 000 + 20 000 steps saved every 100, fp32 - with R = 64 DISTINCT windows
    init = 0.5 + 0.07 w and set_window_exchange(100).  xi gathered by window: the pooled xi - init_w in blocks of 20 samples
    has mean 0 and variance kT / k within 4 standard errors of the block means - the exchanges keep every window's
    distribution.  Every rung pair is accepted at least once; the mean per-pair acceptance rate is within 4 standard errors
    (from the spread of the 63 pairs' own rates) of erfc(0.07 / 2 sigma) = 0.484, sigma = sqrt(kT / k).  A pair is attempted
    every 200 steps, above the autocorrelation time of 70 steps, so its attempts are independent.
    Observed when written: mean - init +1.9e-3 nm (standard error 0.7e-3), variance 4.977e-3 (0.06e-3), acceptance 0.4822
    (0.0064), 105 attempts per pair, the least accepted pair 36 times."""
    n, n_rep, kT, k = 16, 64, 2.5, 500.0
    f = CS.free_beads(n)
    inits = 0.5 + 0.07 * np.arange(n_rep)
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=tuple(range(0, 5))), group_b=PullGroup(members=tuple(range(5, 10))),
                                                 geometry="direction", vec=(0, 0, 1), k=k, init=inits, periodic=False)])
    sysm = _system(f["ff"], torch.float32)
    integ = _ensemble(sysm, np.full(n, 72.0), [kT] * n_rep, gamma=3.0, seeds=list(range(100, 100 + n_rep)), dt=0.02, policy=(1.0, 10))
    x0 = np.broadcast_to(f["pos"], (n_rep, n, 3)).copy()
    off = inits - (x0[:, 5:10, 2].mean(1) - x0[:, 0:5, 2].mean(1))  # start at xi = init, the two groups moved apart symmetrically
    x0[:, 5:10, 2] += 0.5 * off[:, None]
    x0[:, 0:5, 2] -= 0.5 * off[:, None]
    integ.set_restraints(rs)
    integ.set_window_exchange(100, seed=5)
    pos, vel = _dev(x0, sysm), integ.init_velocities()
    integ.load(pos, vel, f["box"])
    integ.advance(1000)
    traj, _ = integ.advance(20000, save_every=100, want_energy=False)
    xi = integ.pull_values(traj)[:, :, 0]  # (200, 64), slot-major
    lw = integ.last_windows
    assert xi.shape == (200, n_rep) and lw.shape == (200, n_rep)
    by_window = torch.gather(xi, 1, torch.argsort(lw, dim=1)).cpu().numpy()
    dev = by_window - inits[None, :]
    blocks = dev.T.reshape(n_rep * 10, 20)
    m, v = blocks.mean(1), (blocks**2).mean(1)
    se_m, se_v = m.std(ddof=1) / np.sqrt(m.size), v.std(ddof=1) / np.sqrt(v.size)
    attempts, accepts = integ.window_exchange_counts()
    rates = accepts / attempts
    want = math.erfc(0.07 / (2.0 * math.sqrt(kT / k)))
    se_r = rates.std(ddof=1) / np.sqrt(rates.size)
    trips = round_trips(lw)
    print(f"  mean - init {m.mean():+.2e} (se {se_m:.1e})  variance {v.mean():.4e} (kT / k {kT / k:.4e}, se {se_v:.1e})")
    print(f"  attempts per pair {attempts.min()} .. {attempts.max()}, acceptance {rates.mean():.4f} (erfc {want:.4f}, se {se_r:.1e}), "
          f"least accepted pair {accepts.min()}, round trips {int(trips.sum())}")
    assert attempts.sum() == 105 * 31 + 105 * 32  # 210 events: the odd attempts try 31 pairs, the even ones 32
    assert abs(want - 0.484) < 1e-3
    assert abs(m.mean()) <= 4 * se_m and abs(v.mean() - kT / k) <= 4 * se_v
    assert accepts.min() >= 1
    assert abs(rates.mean() - want) <= 4 * se_r
    assert not np.array_equal(integ.windows, np.arange(n_rep))
    # slot-major the same samples do NOT sit around their slot's first window: the gather matters
    assert np.abs((xi.cpu().numpy() - inits[None, :])[100:]).mean() > 4 * np.abs(dev[100:]).mean()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_simulator_trajectories_follow_the_windows():
    """The bilayer of test_the_bilayer_follows_an_umbrella_on_the_distance_between_its_leaflets with 4 windows 0.02 nm apart
    (k = 5000: sigma = 0.022 nm) and window_exchange_every = 10."""
    from mythos_amd.observables.mbar import mbar_umbrella
    from mythos_amd.simulators.hip_martini import KB, HipMartiniSimulator
    from tests import martini_restraints_ref as REF

    b = _bilayer()
    m = np.full(len(b["x"]), 72.0)
    z = [REF.group_com(b["x"], m, g, b["box"], int(g[0]))[0][2] for g in (b["lower"], b["upper"])]
    d0 = abs(z[1] - z[0])
    inits = d0 + 0.02 * np.arange(4)
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=tuple(b["lower"]), pbc_ref=int(b["lower"][0])),
                                                 group_b=PullGroup(members=tuple(b["upper"]), pbc_ref=int(b["upper"][0])),
                                                 geometry="distance", dim=(False, False, True), k=5000.0, init=inits, periodic=True)])
    kw = dict(energy_fn=b["fn"], topology=b["top"], init_positions=b["x"], box=b["box"], temperatures=[300.0] * 4, dt=0.02, gamma=1.0,
              equilibration_steps=100, simulation_steps=200, save_every=10, neighbors=(0.4, 5), restraints=rs, precision="float32")
    sim = HipMartiniSimulator(**kw, window_exchange_every=10, name="wx")
    out = sim.run({}, seed=5)
    integ = sim._resident["integrator"]
    lw = integ.last_windows  # (20, 4): the production call's rows
    pull, st = out.state["pull"], out.state
    assert lw.shape == (20, 4) and pull.shape == (20, 4, 1) and pull.dtype == torch.float64 and pull.is_cuda
    assert set(st) == {"positions", "velocities", "boxes", "seed", "pull", "windows", "window_exchange"} and st["seed"] == 5 + 4 + 1
    np.testing.assert_array_equal(st["windows"], integ.windows)
    att, acc = st["window_exchange"]["attempts"], st["window_exchange"]["accepts"]
    print(f"  attempts {att.tolist()} accepts {acc.tolist()} windows {st['windows'].tolist()}")
    assert att.sum() == 30 + 15 and acc.sum() >= 1  # 30 events of (0,1),(2,3) | (1,2)
    # slot-major rows rebuilt through the assignment: slot s at row k is the frame of window lw[k, s]
    by_window = torch.stack([o.center for o in out.observables], dim=1)  # (20, 4, n, 3)
    rows = torch.arange(20, device=lw.device)
    slot_major = torch.stack([by_window[rows, lw[:, s]] for s in range(4)], dim=1).contiguous()
    xi_slot = integ.pull_values(slot_major)
    pick = torch.argsort(lw, dim=1)
    for w in range(4):
        assert torch.equal(out.observables[w].center, slot_major[rows, pick[:, w]]), w
        assert torch.equal(pull[:, w], xi_slot[rows, pick[:, w]]), w
    # the last saved row is the final state, which is slot-major: the gather runs in the right direction
    assert torch.equal(slot_major[-1], st["positions"])
    res = mbar_umbrella(pull, rs, KB * 300.0)
    assert torch.isfinite(res.f).all() and res.delta <= 1e-10
    sim.release()
    # resumed without equilibration: the first production row - saved before the event of its step - has the stored assignment
    resume = HipMartiniSimulator(**dict(kw, equilibration_steps=0), window_exchange_every=10, name="resume")
    out2 = resume.run({}, seed=st["seed"], state=st)
    lw2 = resume._resident["integrator"].last_windows
    np.testing.assert_array_equal(lw2[0].cpu().numpy(), st["windows"])
    first = torch.argsort(lw2[0])
    assert sorted(out2.state["windows"].tolist()) == [0, 1, 2, 3] and out2.state["pull"].shape == (20, 4, 1)
    moved = (out2.observables[0].center[0] - st["positions"][first[0]]).abs().max().item()
    assert 0.0 < moved < 0.5  # window 0's first frame is ten steps on from the slot that held window 0
    resume.release()
    # off: the default simulator's outputs, state keys and seed
    off, plain = HipMartiniSimulator(**kw, window_exchange_every=0, name="off"), HipMartiniSimulator(**kw, name="plain")
    o1, o2 = off.run({}, seed=5), plain.run({}, seed=5)
    off.release(), plain.release()
    assert set(o1.state) == set(o2.state) == {"positions", "velocities", "boxes", "seed", "pull"} and o1.state["seed"] == o2.state["seed"] == 9
    assert torch.equal(o1.state["pull"], o2.state["pull"]) and all(torch.equal(p.center, q.center) for p, q in zip(o1.observables, o2.observables))


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_handle_in_both_orders():
    case = _case(3)
    c = case["c"]
    sysm = _system(_ff(c["s"]), torch.float64)
    baro = dict(kind="berendsen", coupling="isotropic", ref_p=1.0, compressibility=4.5e-5, tau_p=1.0, every=10)
    # temperature exchange
    ens = _ensemble(sysm, c["masses"], [KT] * 3, seeds=SEEDS)
    ens.set_exchange(10, seed=1)
    with pytest.raises(ValueError, match="window exchange together with temperature replica exchange is refused"):
        ens.set_window_exchange(10, seed=1)
    ens.set_exchange(0)
    ens.set_window_exchange(10, seed=1)
    with pytest.raises(ValueError, match="set_exchange: window exchange together with temperature replica exchange is refused"):
        ens.set_exchange(10, seed=1)
    # a barostat
    ens.set_window_exchange(0)
    ens.set_barostat(**baro)
    with pytest.raises(ValueError, match="window exchange together with a barostat is refused"):
        ens.set_window_exchange(10)
    ens.set_barostat(None)
    ens.set_window_exchange(10)
    with pytest.raises(ValueError, match="set_barostat: window exchange together with a barostat is refused"):
        ens.set_barostat(**baro)
    # unequal kT (fixed at creation: one order)
    hot = _ensemble(sysm, c["masses"], [KT, KT, 1.1 * KT], seeds=SEEDS)
    with pytest.raises(ValueError, match="every replica at the same kT"):
        hot.set_window_exchange(10)
    hot.set_window_exchange(0)
    # what stays refused: temperature exchange with a set, in either order
    rs, ref = _permuted(case, np.arange(3))
    ens.set_window_exchange(0)
    ens.set_restraints(rs, reference_pos=ref, box=case["boxes"])
    with pytest.raises(ValueError, match="exchange together with restraints"):
        ens.set_exchange(10, seed=1)
    # window exchange on and no set: NOT_READY at advance; a set whose vec differs between replicas, in either order
    ens.set_restraints(None)
    ens.set_window_exchange(10)
    pos, vel = _dev(case["pos"], sysm), ens.init_velocities()
    ens.load(pos, vel, case["boxes"])
    with pytest.raises((ValueError, RuntimeError), match="no set of restraints is installed"):
        ens.advance(10)
    from mythos_amd.simulators import martini_restraints as mr

    low = rs.lower(n_rep=3, boxes=case["boxes"], reference_pos=ref)
    low["p_param"][1, 1, 3:6] = (0.0, 0.0, 1.0)
    rc = ens._lib.mythos_martini_langevin_set_restraints(ens._h, *mr.c_args(low))
    from mythos_amd import _lib

    assert rc == -1 and "pull coordinate 1: window exchange needs the same vec in every replica" in _lib.last_error()
    ens.set_window_exchange(0)
    assert ens._lib.mythos_martini_langevin_set_restraints(ens._h, *mr.c_args(low)) == 0
    with pytest.raises(ValueError, match="window exchange needs the same vec in every replica"):
        ens.set_window_exchange(10)
    # set_windows on an open resident frame
    ens.set_restraints(rs, reference_pos=ref, box=case["boxes"])
    ens.load(pos, vel, case["boxes"])
    ens.advance(3)
    with pytest.raises((ValueError, RuntimeError), match="the resident frame is open"):
        ens.set_windows([1, 0, 2])
    ens.store(pos, vel)
    ens.set_windows([1, 0, 2])
