"""GPU tests of replica exchange between the temperatures of the MARTINI ensemble (MartiniEnsembleIntegrator.set_exchange /
mythos_martini_langevin_set_exchange; the rule is stated in include/mythos_hip.h and restated in tests/martini_exchange_ref.py).

The yardstick: between two exchange events a run with exchange IS the plain ensemble - created with the slots' current kT,
restarted at the event's step, loaded with the stored state - bit for bit, because an event drops the neighbour rows as a
load does.  Test 3 glues such runs by hand with the rule; the plain ensemble itself is pinned to the single integrator by
tests/test_gpu_martini_ensemble.py and that to the CPU oracle by tests/test_gpu_martini_md.py.

  0  the parent's property the yardstick stands on: advance(E); store; load into a fresh ensemble restarted at E; advance(E)
     equals advance(2 E) across a coupling event's list drop
  1  the log against the rule (md37 x 4)            5  split calls
  2  the chain against the CPU oracle               6  switching off
  3  exchange = plain runs glued by the rule        7  NPT: p V, exchange before coupling, the refusal
  4  equal temperatures                             8  charged bilayer: the Coulomb column in U     9  HipMartiniSimulator
"""

import functools

import numpy as np
import pytest
import torch

from tests import martini_exchange_ref as X
from tests import martini_synth as S
from tests.test_gpu_martini_ensemble import KT, LATTICE, NPT, SEEDS, _case, _system

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
# md37 (three workgroups per replica, the last with 5 of 16 beads), as tests/test_gpu_martini_ensemble.py runs it
MD37 = dict(dt=0.002, gamma=2.0, policy=(0.25, 2))
# The CPU oracle chain alone, from the device's initial velocities restated on the host (X.host_init_velocities), gives 9
# accepted and 9 rejected among the 18 attempts of these settings, every |u - exp(d)| above 0.065: the ladder stays as the
# issue gives it.
KTS = np.array([2.0, 2.5, 3.2, 4.0])
EVERY, XSEED, STEPS, SAVE = 4, 99, 48, 4


def _ensemble(c, sysm, kTs, cfg, seeds=None, exchange=None):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    integ = MartiniEnsembleIntegrator(sysm, dt=cfg["dt"], kT=kTs, gamma=cfg["gamma"], mass=c["mass"], seeds=seeds or SEEDS[:len(kTs)])
    integ.set_neighbor_policy(*cfg["policy"])
    if cfg.get("inner"):
        integ.set_inner_list(*cfg["inner"])
    if cfg.get("baro"):
        integ.set_barostat(**cfg["baro"])
    if exchange:
        integ.set_exchange(*exchange)
    return integ


def _start(c, sysm, n_rep):
    return torch.tensor(np.broadcast_to(c["pos"], (n_rep, c["n"], 3)).copy(), dtype=sysm.dtype, device=sysm.device).contiguous()


def _drive(integ, pos, vel, box, calls, save_every=SAVE, want_energy=True):
    """load; advance(n) for n in calls; store -> dict: rows / boxes / energy rows / ladder rows by absolute step, the logs
    concatenated, the final state."""
    integ.load(pos, vel, box)
    rows, log, at, rec = {}, [], 0, 0
    for n in calls:
        traj, et = integ.advance(n, save_every=save_every, want_energy=want_energy)
        rec += integ.last_recoveries()
        lb, ll = integ.last_boxes, integ.last_ladder
        n_rows = n // save_every if save_every else 0
        assert lb.shape[0] == n_rows and ll.shape == (n_rows, integ.n_rep) and ll.dtype == torch.int64 and ll.device == pos.device
        for k in range(n_rows):
            rows[at + (k + 1) * save_every] = (traj[k].cpu(), lb[k].cpu().numpy(), et[k].cpu() if et is not None else None, ll[k].cpu().numpy())
        log.append(integ.last_exchanges)
        at += n
    integ.store(pos, vel)
    log = {k: np.concatenate([l[k] for l in log]) for k in log[0]}
    return dict(rows=rows, log=log, pos=pos.cpu(), vel=vel.cpu(), ladder=integ.ladder, recoveries=rec, step=integ.step, integ=integ, box=integ.box)


@functools.lru_cache(maxsize=None)
def _md37_run(dtype, n_rep=4, equal=False):
    """The shared run of tests 1 - 5: md37 x n_rep from the same positions in the system's box, exchange every 4 steps, 48
    steps, energy rows every 4."""
    c = _case("md37")
    sysm = _system(c, dtype)
    kTs = np.full(n_rep, 2.5) if equal else KTS[:n_rep]
    integ = _ensemble(c, sysm, kTs, MD37, exchange=(EVERY, XSEED))
    vel = integ.init_velocities()
    v0 = vel.cpu().clone()
    out = _drive(integ, _start(c, sysm, n_rep), vel, c["box"], [STEPS])
    out.update(v0=v0, kTs=kTs, counts=integ.exchange_counts(), kT_now=integ.kT_now)
    return out


def _swapped(ladder, pairs):
    new = np.array(ladder).copy()
    for a, b in pairs:
        new[a], new[b] = ladder[b], ladder[a]
    return new


# ---- 0 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_the_plain_ensemble_reloaded_behind_a_coupling_event_continues_bitwise(dtype):
    """What test 3's yardstick stands on, on code this feature does not touch: md1285 x 2 under c-rescale every 4 steps;
    advance(4) ends on the event (frame closed, rows dropped); store; a fresh ensemble restarted at step 4 and loaded with
    the stored state and boxes; advance(4): positions, velocities, rows and boxes equal those of one advance(8), bitwise."""
    c = _case("md1285")
    sysm = _system(c, dtype)
    cfg = dict(LATTICE, baro=dict(NPT["crescale-semi"], every=4))
    kTs = KT * np.array([1.0, 1.2])
    one = _ensemble(c, sysm, kTs, cfg)
    vel = one.init_velocities()
    v0 = vel.clone()
    a = _drive(one, _start(c, sysm, 2), vel, c["box"], [8])
    first = _ensemble(c, sysm, kTs, cfg)
    pos, vel = _start(c, sysm, 2), v0.clone()
    first.load(pos, vel, c["box"])
    t1, e1 = first.advance(4, save_every=4)
    first.store(pos, vel)
    second = _ensemble(c, sysm, kTs, cfg)
    second.restart(SEEDS[:2], step=4)
    second.load(pos, vel, first.box)
    t2, e2 = second.advance(4, save_every=4)
    second.store(pos, vel)
    assert a["recoveries"] == 0 and first.last_recoveries() == 0 and second.last_recoveries() == 0
    assert torch.equal(a["rows"][4][0], t1[0].cpu()) and torch.equal(a["rows"][4][2], e1[0].cpu())
    assert torch.equal(a["rows"][8][0], t2[0].cpu()) and torch.equal(a["rows"][8][2], e2[0].cpu())
    assert torch.equal(a["pos"], pos.cpu()) and torch.equal(a["vel"], vel.cpu())
    np.testing.assert_array_equal(a["box"], second.box)
    assert (a["box"] != c["box"]).any()


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_the_log_is_the_rule(dtype):
    """md37 x 4 at kT = (2.0, 2.5, 3.2, 4.0), seeds SEEDS[:4], exchange seed 99, every 4 steps, 48 steps, energy rows every
    4: every record against the numpy restatement, the ladder rows against the accepted pairs, the counts against the log.
    (Ladder spacing: the issue's; the oracle chain from host-restated initial velocities gave 9 / 9 accepted / rejected.)"""
    r = _md37_run(dtype)
    log, rows, kTs = r["log"], r["rows"], r["kTs"]
    assert r["recoveries"] == 0 and r["step"] == STEPS
    want_pairs = [(s, t) for s in range(EVERY, STEPS + 1, EVERY) for t in X.schedule(4, s // EVERY)]
    assert list(zip(log["step"].tolist(), log["rung"].tolist())) == want_pairs and len(want_pairs) == 18
    n_acc = int(log["accepted"].sum())
    print(f"  {n_acc} accepted, {18 - n_acc} rejected; min |u - exp(d)| {np.abs(log['u'] - np.exp(np.minimum(log['d'], 50.0))).min():.3e}")
    ladder_after = None
    for k, (s, t) in enumerate(want_pairs):
        _, box_row, e_row, ladder = rows[s]
        a, b = int(log["slot_a"][k]), int(log["slot_b"][k])
        assert ladder[a] == t and ladder[b] == t + 1, (s, t)
        assert log["u"][k] == X.uniform(XSEED, t, s), (s, t)
        assert log["u_a"][k] == X.potential(e_row[a].numpy()) and log["u_b"][k] == X.potential(e_row[b].numpy()), (s, t)
        assert log["v_a"][k] == X.volume(box_row[a]) and log["v_b"][k] == X.volume(box_row[b])
        d = X.delta(kTs[t], kTs[t + 1], log["u_a"][k], log["v_a"][k], log["u_b"][k], log["v_b"][k], 0.0)
        np.testing.assert_allclose(log["d"][k], d, rtol=1e-12, atol=0)
        assert abs(log["u"][k] - np.exp(min(log["d"][k], 50.0))) >= 1e-9, (s, t)
        assert bool(log["accepted"][k]) == X.accepts(log["d"][k], log["u"][k]), (s, t)
    for s in range(EVERY, STEPS + 1, EVERY):
        sel = (log["step"] == s) & log["accepted"]
        ladder_after = _swapped(rows[s][3], list(zip(log["slot_a"][sel].tolist(), log["slot_b"][sel].tolist())))
        nxt = rows[s + SAVE][3] if s + SAVE in rows else r["ladder"]
        np.testing.assert_array_equal(nxt, ladder_after, err_msg=f"ladder behind the event of step {s}")
    assert sorted(r["ladder"].tolist()) == [0, 1, 2, 3]
    np.testing.assert_array_equal(r["kT_now"], kTs[r["ladder"]])
    attempts, accepts = r["counts"]
    for t in range(3):
        assert attempts[t] == (log["rung"] == t).sum() and accepts[t] == ((log["rung"] == t) & log["accepted"]).sum()
    assert n_acc >= 3 and 18 - n_acc >= 3


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_the_chain_against_the_cpu_oracle():
    """The fp64 run of test 1 against X.OracleChain - four MartiniLangevinOracles driven with the device's initial
    velocities and the device's DECISIONS (forced: a flip near the threshold must not become a trajectory comparison), the
    rule's swap of kT and velocity factors between them.  Tolerances: those tests/test_gpu_martini_shapes.py holds the single
    integrator to step by step - positions and velocities atol 1e-10, energy rows rtol 1e-9 atol 1e-7."""
    r = _md37_run(torch.float64)
    c = _case("md37")
    log = r["log"]
    forced = {(int(s), int(t)): bool(a) for s, t, a in zip(log["step"], log["rung"], log["accepted"])}
    a = S.oracle_args(S.get("md37"))
    chain = X.OracleChain(a[2:], True, [c["box"]] * 4, MD37["dt"], KTS, MD37["gamma"], c["mass"], SEEDS[:4], EVERY, XSEED, forced=forced)
    x = np.stack([np.array(c["pos"], dtype=np.float64)] * 4)
    v = r["v0"].numpy().copy()
    ref = chain.run(x, v, STEPS, SAVE)
    assert set(ref) == set(r["rows"])
    worst = [0.0, 0.0]
    for s, (xs, _, es, ladder) in ref.items():
        row, _, e_row, lad = r["rows"][s]
        worst = [max(worst[0], np.abs(row.numpy() - xs).max()), max(worst[1], np.abs(e_row.numpy() - es).max())]
        np.testing.assert_allclose(row.numpy(), xs, rtol=0, atol=1e-10)
        np.testing.assert_allclose(e_row.numpy(), es, rtol=1e-9, atol=1e-7)
        np.testing.assert_array_equal(lad, ladder)
    print(f"  max |dx| {worst[0]:.2e}, |dE| {worst[1]:.2e}, final |dv| {np.abs(r['vel'].numpy() - v).max():.2e}")
    np.testing.assert_allclose(r["pos"].numpy(), x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(r["vel"].numpy(), v, rtol=0, atol=1e-10)
    np.testing.assert_array_equal(r["ladder"], chain.ladder)
    for k, rec in enumerate(chain.log):  # the oracle's own d and u at the device's decisions
        assert rec["u"] == log["u"][k]
        np.testing.assert_allclose(log["d"][k], rec["d"], rtol=1e-6, atol=1e-7)


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------
def _hand_chain(dtype, kTs, v0, swap=True):
    """Plain ensembles glued by the rule through the API that existed before exchange did: per segment advance(E) with an
    energy row at its end; store; the decision on the host from that row; velocities scaled with torch in the system's dtype;
    a fresh ensemble with the permuted kT, restarted at the step, loaded."""
    c = _case("md37")
    sysm = _system(c, dtype)
    n_rep, npdt = len(kTs), (np.float32 if dtype == torch.float32 else np.float64)
    ladder, seeds = np.arange(n_rep), SEEDS[:n_rep]
    integ = _ensemble(c, sysm, kTs[ladder], MD37)
    pos, vel = _start(c, sysm, n_rep), v0.to(sysm.device).clone()
    integ.load(pos, vel, c["box"])
    rows, rec = {}, 0
    boxes = np.broadcast_to(c["box"], (n_rep, 3))
    for s in range(EVERY, STEPS + 1, EVERY):
        traj, et = integ.advance(EVERY, save_every=SAVE, want_energy=True)
        rec += integ.last_recoveries()
        integ.store(pos, vel)
        rows[s] = (traj[0].cpu(), et[0].cpu(), ladder.copy())
        if swap:
            new, _, _ = X.decide(ladder, kTs, et[0].cpu().numpy(), boxes, s, EVERY, XSEED)
        else:
            new = ladder
        for r in range(n_rep):
            if new[r] != ladder[r]:
                vel[r] *= float(X.factor(kTs[ladder[r]], kTs[new[r]], npdt))
        ladder = new
        integ = _ensemble(c, sysm, kTs[ladder], MD37)
        integ.restart(seeds, step=s)
        integ.load(pos, vel, c["box"])
    return dict(rows=rows, pos=pos.cpu(), vel=vel.cpu(), ladder=ladder, recoveries=rec)


@DTYPES
def test_a_run_with_exchange_is_plain_ensemble_runs_glued_by_the_rule(dtype):
    """One advance(48) with exchange on against the hand chain: saved rows, energy rows, final positions and velocities and
    the ladder, bit for bit; neither side reports a recovery."""
    r = _md37_run(dtype)
    h = _hand_chain(dtype, KTS, r["v0"])
    assert r["recoveries"] == 0 and h["recoveries"] == 0
    assert set(r["rows"]) == set(h["rows"])
    for s, (row, e_row, ladder) in h["rows"].items():
        assert torch.equal(r["rows"][s][0], row), s
        assert torch.equal(r["rows"][s][2], e_row), s
        np.testing.assert_array_equal(r["rows"][s][3], ladder)
    assert torch.equal(r["pos"], h["pos"]) and torch.equal(r["vel"], h["vel"])
    np.testing.assert_array_equal(r["ladder"], h["ladder"])
    assert not np.array_equal(h["ladder"], np.arange(4))


@DTYPES
def test_equal_temperatures_always_swap_and_change_nothing(dtype):
    """md37 x 3, every kT 2.5: d = 0, so every attempt is accepted and the ladder follows the odd-even transposition
    pattern; every factor is exactly 1, so positions and velocities are those of the hand chain with no swap applied."""
    r = _md37_run(dtype, 3, True)
    log = r["log"]
    assert log["accepted"].all() and (log["d"] == 0.0).all() and len(log["d"]) == 12
    ladder = np.arange(3)
    for s in range(EVERY, STEPS + 1, EVERY):
        np.testing.assert_array_equal(r["rows"][s][3], ladder, err_msg=f"step {s}")
        for t in X.schedule(3, s // EVERY):
            a, b = int(np.nonzero(ladder == t)[0][0]), int(np.nonzero(ladder == t + 1)[0][0])
            ladder[a], ladder[b] = t + 1, t
    np.testing.assert_array_equal(r["ladder"], ladder)
    assert (r["kT_now"] == 2.5).all()
    h = _hand_chain(dtype, np.full(3, 2.5), r["v0"], swap=False)
    assert r["recoveries"] == 0 and h["recoveries"] == 0
    assert torch.equal(r["pos"], h["pos"]) and torch.equal(r["vel"], h["vel"])
    for s, (row, e_row, _) in h["rows"].items():
        assert torch.equal(r["rows"][s][0], row) and torch.equal(r["rows"][s][2], e_row), s


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_energy", [True, False], ids=["energy-rows", "plain-rows"])
@DTYPES
def test_split_calls_equal_one_call(dtype, want_energy):
    """advance(10); advance(14); advance(24) against advance(48): events follow the absolute step counter, the logs
    concatenate to the one call's, rows at shared steps, final state and ladder are equal bit for bit.  plain-rows: the
    caller takes no energies - the event's own row goes to the integrator's buffer, and a row saved at an event step is
    written by the energy-trace launch."""
    r = _md37_run(dtype)
    c = _case("md37")
    sysm = _system(c, dtype)
    integ = _ensemble(c, sysm, KTS, MD37, exchange=(EVERY, XSEED))
    sp = _drive(integ, _start(c, sysm, 4), r["v0"].to(sysm.device).clone(), c["box"], [10, 14, 24], want_energy=want_energy)
    assert sp["recoveries"] == 0 and sp["step"] == STEPS
    for k in r["log"]:
        np.testing.assert_array_equal(sp["log"][k], r["log"][k], err_msg=k)
    assert torch.equal(sp["pos"], r["pos"]) and torch.equal(sp["vel"], r["vel"])
    np.testing.assert_array_equal(sp["ladder"], r["ladder"])
    shared = sorted(set(sp["rows"]) & set(r["rows"]))
    assert shared == [4, 8, 28, 32, 36, 40, 44, 48]
    for s in shared:
        assert torch.equal(sp["rows"][s][0], r["rows"][s][0]), s
        assert (sp["rows"][s][2] is None) if not want_energy else torch.equal(sp["rows"][s][2], r["rows"][s][2]), s
        np.testing.assert_array_equal(sp["rows"][s][3], r["rows"][s][3])
    np.testing.assert_array_equal(sp["integ"].exchange_counts()[0], r["counts"][0])
    np.testing.assert_array_equal(sp["integ"].exchange_counts()[1], r["counts"][1])


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_switched_off_again_is_the_handle_that_never_had_it(dtype):
    c = _case("md37")
    sysm = _system(c, dtype)
    outs = []
    for touched in (True, False):
        integ = _ensemble(c, sysm, KTS, MD37)
        if touched:
            integ.set_exchange(EVERY, XSEED)
            integ.set_exchange(0)
        outs.append(_drive(integ, _start(c, sysm, 4), integ.init_velocities(), c["box"], [24]))
    a, b = outs
    assert len(a["log"]["step"]) == 0 and a["integ"].exchange_counts()[0].sum() == 0
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["vel"], b["vel"])
    for s in b["rows"]:
        assert torch.equal(a["rows"][s][0], b["rows"][s][0]) and torch.equal(a["rows"][s][2], b["rows"][s][2])
        np.testing.assert_array_equal(a["rows"][s][3], np.arange(4))
    on = _md37_run(dtype)
    assert not torch.equal(on["rows"][24][0], a["rows"][24][0])  # and exchange does change the run


# ---- 7 ------------------------------------------------------------------------------------------------------------------
NPT_X = dict(NPT["crescale-semi"], every=4)


@DTYPES
def test_npt_the_work_term_and_exchange_before_coupling(dtype):
    """md1285 x 3 at kT (1.0, 1.1, 1.2) from one box, c-rescale semi-isotropic every 4, exchange every 6, rows every 2, 24
    steps: steps 6 and 18 carry an exchange alone, 12 and 24 exchange and coupling, each with a saved row - the state before
    both.  V of the log is the product of that row's last_boxes bitwise, d the numpy value with p (V_A - V_B), p = 1 bar.
    fp64: rows and last_boxes against X.OracleChain with the device's decisions and exchange before coupling, at atol 1e-9
    (tests/test_gpu_martini_npt.py).  The lattice is far from equilibrium: d may saturate; the test is about the term and the
    order of events."""
    c = _case("md1285")
    sysm = _system(c, dtype)
    kTs = KT * np.array([1.0, 1.1, 1.2])
    cfg = dict(LATTICE, baro=NPT_X)
    integ = _ensemble(c, sysm, kTs, cfg, exchange=(6, XSEED))
    vel = integ.init_velocities()
    v0 = vel.cpu().numpy().astype(np.float64)
    r = _drive(integ, _start(c, sysm, 3), vel, c["box"], [24], save_every=2)
    log = r["log"]
    p = 1.0 / 16.6053907
    assert log["step"].tolist() == [6, 12, 18, 24] and log["rung"].tolist() == [1, 0, 1, 0]
    assert list(zip(log["step"].tolist(), log["rung"].tolist())) == [(s, t) for s in (6, 12, 18, 24) for t in X.schedule(3, s // 6)]
    for k in range(len(log["step"])):
        s, t, a, b = int(log["step"][k]), int(log["rung"][k]), int(log["slot_a"][k]), int(log["slot_b"][k])
        _, box_row, e_row, ladder = r["rows"][s]
        assert ladder[a] == t and ladder[b] == t + 1
        assert log["v_a"][k] == X.volume(box_row[a]) and log["v_b"][k] == X.volume(box_row[b]), s
        assert log["u_a"][k] == X.potential(e_row[a].numpy()) and log["u_b"][k] == X.potential(e_row[b].numpy()), s
        np.testing.assert_allclose(log["d"][k], X.delta(kTs[t], kTs[t + 1], log["u_a"][k], log["v_a"][k], log["u_b"][k], log["v_b"][k], p),
                                   rtol=1e-12, atol=0)
        assert bool(log["accepted"][k]) == X.accepts(log["d"][k], log["u"][k]) and log["u"][k] == X.uniform(XSEED, t, s)
    # the boxes: constant up to the row of step 4, moved by the events of 4, 8, ...; the row of step 12 is before its event
    np.testing.assert_array_equal(r["rows"][4][1], np.broadcast_to(c["box"], (3, 3)))
    assert (r["rows"][6][1] != c["box"]).any() and np.array_equal(r["rows"][6][1], r["rows"][8][1]) and not np.array_equal(r["rows"][8][1], r["rows"][10][1])
    assert (log["v_a"][log["step"] >= 12] != log["v_b"][log["step"] >= 12]).all()  # the boxes have diverged: p dV is in d
    if dtype != torch.float64:
        return
    forced = {(int(s), int(t)): bool(a) for s, t, a in zip(log["step"], log["rung"], log["accepted"])}
    chain = X.OracleChain(c["ff"], True, [c["box"]] * 3, LATTICE["dt"], kTs, LATTICE["gamma"], c["mass"], SEEDS[:3], 6, XSEED, baro=NPT_X, forced=forced)
    x, v = np.stack([np.array(c["pos"], dtype=np.float64)] * 3), v0.copy()
    ref = chain.run(x, v, 24, 2)
    for s, (xs, bs, _, ladder) in ref.items():
        np.testing.assert_allclose(r["rows"][s][0].numpy(), xs, rtol=0, atol=1e-9, err_msg=f"row of step {s}")
        np.testing.assert_allclose(r["rows"][s][1], bs, rtol=0, atol=1e-9, err_msg=f"boxes of step {s}")
        np.testing.assert_array_equal(r["rows"][s][3], ladder)
    np.testing.assert_allclose(r["pos"].numpy(), x, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["vel"].numpy(), v, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["box"], chain.boxes, rtol=0, atol=1e-9)


def test_an_anisotropic_reference_pressure_is_refused_at_advance():
    """Both compressibilities non-zero and ref_p = (1.0, 2.0): advance is refused, the message names the reason, and the
    state is the one loaded."""
    c = _case("md1285")
    sysm = _system(c, torch.float64)
    cfg = dict(LATTICE, baro=dict(NPT_X, ref_p=(1.0, 2.0)))
    integ = _ensemble(c, sysm, KT * np.array([1.0, 1.1, 1.2]), cfg, exchange=(6, XSEED))
    pos, vel = _start(c, sysm, 3), integ.init_velocities()
    p0, v0 = pos.clone(), vel.clone()
    integ.load(pos, vel, c["box"])
    with pytest.raises(ValueError, match=r"both compressibilities non-zero needs ref_p\[0\] == ref_p\[1\].*no scalar work term"):
        integ.advance(24, save_every=2)
    assert integ.step == 0 and len(integ.last_exchanges["step"]) == 0
    np.testing.assert_array_equal(integ.box, np.broadcast_to(c["box"], (3, 3)))
    integ.store(pos, vel)
    assert torch.equal(pos, p0) and torch.equal(vel, v0)
    integ.set_exchange(0)  # and without exchange the same settings run
    integ.advance(4)
    assert integ.step == 4


# ---- 8 ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_charged_bilayer_u_includes_the_coulomb_column(dtype):
    """The bilayer x 2 with charges (five trace columns), exchange every 4: attempt 1 has no pair for two rungs, attempt 2
    (step 8) has the one event.  U of the record is the five-column row's lj + bond + angle + coulomb, bit for bit."""
    c = _case("bilayer")
    sysm = _system(c, dtype, charged=True)
    cfg = dict(dt=0.01, gamma=2.0, policy=(0.3, 3), inner=(0.15, 3))
    kTs = np.array([KT, 1.17 * KT])
    integ = _ensemble(c, sysm, kTs, cfg, exchange=(4, XSEED))
    r = _drive(integ, _start(c, sysm, 2), integ.init_velocities(), c["box"], [8])
    log = r["log"]
    assert log["step"].tolist() == [8] and log["rung"].tolist() == [0] and log["slot_a"].tolist() == [0] and log["slot_b"].tolist() == [1]
    e = r["rows"][8][2].numpy()
    assert e.shape == (2, 5) and (e[:, 4] != 0).all()
    for k, key in enumerate(("u_a", "u_b")):
        assert log[key][0] == ((e[k, 0] + e[k, 1]) + e[k, 2]) + e[k, 4]
        assert log[key][0] != (e[k, 0] + e[k, 1]) + e[k, 2]
    np.testing.assert_allclose(log["d"][0], X.delta(kTs[0], kTs[1], log["u_a"][0], 0.0, log["u_b"][0], 0.0), rtol=1e-12, atol=0)
    assert bool(log["accepted"][0]) == X.accepts(log["d"][0], log["u"][0])


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_simulator_trajectories_follow_the_temperatures():
    """The bilayer of tests/test_gpu_martini_simulator.py at three temperatures, exchange every 10: observables[t] is the
    gather of a hand-driven ensemble's rows by last_ladder with that slot's box and the rung's temperature, the state is
    slot-major with the ladder and the counts, the next seed is seed + R + 1.  A continuation run(state=...) is the hand-driven
    ensemble restarted with the continuation's seeds, given the ladder by set_ladder and loaded with the state - every
    simulator run restarts the step counter and takes new seeds, with or without exchange, so "one longer run" can only be
    held in this form.  exchange_every = 0: outputs, state keys and the returned seed are those of the default simulator."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniSystem
    from mythos_amd.simulators.hip_martini import lower_martini
    from tests import martini_helpers as MH
    from tests.test_gpu_martini_simulator import KB, TEMPS, _energy_fn, _simulator

    sim = _simulator(exchange_every=10)
    out = sim.run({}, seed=5)
    more = sim.run({}, seed=out.state["seed"], state=out.state)
    s = MH.system()
    x, box, _ = MH.frames("lj")
    low = lower_martini(_energy_fn(s))
    sysm = MartiniSystem(low["types"], low["sigma"], low["eps"], low["bonds"], low["bond_k"], low["bond_r0"], low["angles"], low["angle_k"],
                         low["angle_t0"], angle_kind=low["angle_kind"], dtype=torch.float32)
    integ = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=KB * np.array(TEMPS), gamma=1.0, seeds=5)
    integ.set_neighbor_policy(0.4, 5)
    integ.set_barostat("c-rescale", "semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 0.0), tau_p=8.0, every=10)
    pos = torch.tensor(np.broadcast_to(x[3], (3, 1280, 3)).copy(), dtype=torch.float32, device=sysm.device)
    vel, boxes = integ.init_velocities(), box[3]
    for seed, result in ((5, out), (9, more)):
        integ.restart([seed, seed + 1, seed + 2], 0)
        integ.set_exchange(10, seed + 3)
        if seed == 9:
            integ.set_ladder(out.state["ladder"])
        integ.load(pos, vel, boxes)
        integ.advance(10)
        traj, _ = integ.advance(40, save_every=10, want_energy=False)
        lb, ll = integ.last_boxes, integ.last_ladder.cpu().numpy()
        integ.store(pos, vel)
        boxes = integ.box
        for t, tr in enumerate(result.observables):
            slots = [int(np.nonzero(ll[k] == t)[0][0]) for k in range(4)]
            assert torch.equal(tr.center, torch.stack([traj[k, slots[k]] for k in range(4)])), (seed, t)
            assert torch.equal(tr.box_size, torch.stack([lb[k, slots[k]] for k in range(4)])), (seed, t)
            assert torch.equal(tr.temperature.cpu(), torch.full((4,), KB * TEMPS[t], dtype=torch.float64))
        st = result.state
        assert torch.equal(st["positions"], pos) and torch.equal(st["velocities"], vel) and st["seed"] == seed + 4
        np.testing.assert_array_equal(st["boxes"], boxes)
        np.testing.assert_array_equal(st["ladder"], integ.ladder)
        att, acc = integ.exchange_counts()
        np.testing.assert_array_equal(st["exchange"]["attempts"], att)
        np.testing.assert_array_equal(st["exchange"]["accepts"], acc)
        assert att.tolist() == [2, 3] and (acc <= att).all()  # attempts 1 .. 5: pairs (1, 2), (0, 1), (1, 2), (0, 1), (1, 2)
    sim.release()
    off, plain = _simulator(exchange_every=0), _simulator()
    a, b = off.run({}, seed=5), plain.run({}, seed=5)
    assert set(a.state) == {"positions", "velocities", "boxes", "seed"} and a.state["seed"] == 8 == b.state["seed"]
    for ta, tb in zip(a.observables, b.observables):
        assert torch.equal(ta.center, tb.center) and torch.equal(ta.box_size, tb.box_size) and torch.equal(ta.temperature, tb.temperature)
    assert torch.equal(a.state["positions"], b.state["positions"]) and torch.equal(a.state["velocities"], b.state["velocities"])
    off.release(), plain.release()
