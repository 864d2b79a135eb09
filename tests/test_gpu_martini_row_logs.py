"""GPU test of the row logs of the MARTINI ensemble integrator: ``last_boxes``, ``last_ladder`` and ``last_windows`` hold one
row per saved row of the last call - the same number in all three, whatever events cut the call - and a row is the state
BEFORE the events of its step.

md37 (tests/martini_synth.py) x 3 replicas, so that the even and the odd attempts have one pair each; twelve steps as one
call and as calls of 5 and 7, rows never, at every step and every 5 steps (never on an event step, which are 3, 6, 9, 12
and 4, 8, 12), with and without energy rows - which moves the energy row of a temperature event between the caller's row
and the exchange's own.  Modes: no events (one call of the driver), a barostat, temperature exchange, both, window
exchange.  Rows of a permutation that no event of the mode moves equal the handle's; rows of one that does are replayed
from the accepted records of the log.
"""

import numpy as np
import pytest
import torch

from mythos_amd.simulators.martini_restraints import MartiniRestraints, PositionRestraint, PullCoordinate, PullGroup
from tests.test_gpu_martini_ensemble import NPT, SEEDS, _case, _system

pytestmark = pytest.mark.gpu

R, STEPS = 3, 12
BARO = dict(NPT["crescale-semi"], every=3)
MODES = {  # kT per replica, barostat, temperature exchange (every, seed), window exchange (every, seed)
    "plain": dict(kT=(2.0, 2.5, 3.2)),
    "barostat": dict(kT=(2.0, 2.5, 3.2), baro=BARO),
    "exchange": dict(kT=(2.0, 2.5, 3.2), exchange=(4, 99)),
    "both": dict(kT=(2.0, 2.5, 3.2), baro=BARO, exchange=(4, 99)),
    "windows": dict(kT=(2.5, 2.5, 2.5), windows=(4, 77)),
}


def _windowed_set(c):
    """Restraints made window-wise as in tests/test_gpu_martini_window_exchange.py: position restraints whose references,
    left None, come from per-window reference states 0.002 nm apart, and an umbrella on the length of the first bond with
    init and k per window - windows close enough for exchanges to be accepted."""
    w = np.arange(R, dtype=np.float64)
    i, j = (int(b) for b in np.asarray(c["ff"][3])[0])
    d0 = float(np.linalg.norm(c["pos"][j] - c["pos"][i]))
    ref = c["pos"][None] + np.random.default_rng(7).uniform(-0.002, 0.002, size=(R, c["n"], 3))
    rs = MartiniRestraints(position=[PositionRestraint(index=k, k=500.0) for k in range(0, c["n"], 2)],
                           pulls=[PullCoordinate(group_a=PullGroup(members=(i,)), group_b=PullGroup(members=(j,)), kind="umbrella",
                                                 geometry="distance", k=tuple(1500.0 - 20.0 * w), init=tuple(d0 + 0.01 * w), periodic=False)])
    return rs, ref


def _integrator(c, sysm, mode):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    m = MODES[mode]
    integ = MartiniEnsembleIntegrator(sysm, dt=0.002, kT=m["kT"], gamma=2.0, mass=c["mass"], seeds=SEEDS[:R])
    integ.set_neighbor_policy(0.2, 2)  # (md37's shortest edge is 2 (r_cut + 0.25): room for the coupling to shrink it)
    if "baro" in m:
        integ.set_barostat(**m["baro"])
    if "exchange" in m:
        integ.set_exchange(*m["exchange"])
    if "windows" in m:
        integ.set_window_exchange(*m["windows"])
        rs, ref = _windowed_set(c)
        integ.set_restraints(rs, reference_pos=ref, box=np.broadcast_to(c["box"], (R, 3)).copy())
    return integ


def _replayed(start, log, row_steps):
    """The permutation in front of every step of row_steps, and behind the whole log: ``start`` with the accepted records
    below that step applied in order, each swapping what its two slots hold."""
    def at(step):
        p = np.array(start).copy()
        for s, a, b, ok in zip(log["step"], log["slot_a"], log["slot_b"], log["accepted"]):
            if ok and s < step:
                p[a], p[b] = p[b], p[a]
        return p

    return [at(s) for s in row_steps], at(np.inf)


@pytest.mark.parametrize("save_every", [0, 1, 5])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_log_has_the_rows_of_the_call_and_each_row_is_the_state_before_its_events(mode, save_every):
    c = _case("md37")
    sysm = _system(c, torch.float64)
    moved = {"exchange": "ladder", "both": "ladder", "windows": "windows"}.get(mode)
    for calls in ((STEPS,), (5, 7)):
        for want_energy in (True, False):
            integ = _integrator(c, sysm, mode)
            pos = torch.tensor(np.broadcast_to(c["pos"], (R, c["n"], 3)).copy(), dtype=sysm.dtype, device=sysm.device)
            integ.load(pos, integ.init_velocities(), np.broadcast_to(c["box"], (R, 3)).copy())
            at, attempts = 0, 0
            for n in calls:
                before = {"ladder": integ.ladder, "windows": integ.windows}
                integ.advance(n, save_every=save_every, want_energy=want_energy)
                n_rows = n // save_every if save_every else 0
                rows = {"ladder": integ.last_ladder.cpu().numpy(), "windows": integ.last_windows.cpu().numpy()}
                assert integ.last_boxes.shape[0] == rows["ladder"].shape[0] == rows["windows"].shape[0] == n_rows, (calls, want_energy, n)
                logs = {"ladder": integ.last_exchanges, "windows": integ.last_window_exchanges}
                row_steps = [at + (k + 1) * save_every for k in range(n_rows)]
                for name in ("ladder", "windows"):
                    now = getattr(integ, name)
                    if name != moved:  # no event of this mode moves it: every row is the handle's, and nothing was logged
                        assert len(logs[name]["step"]) == 0 and (now == before[name]).all()
                        assert (rows[name] == now[None, :]).all() and rows[name].shape == (n_rows, R)
                        continue
                    log = logs[name]
                    want_steps = [s for s in range(at + 1, at + n + 1) if s % 4 == 0]  # one pair per attempt with R = 3
                    assert log["step"].tolist() == want_steps, (calls, n)
                    want_rows, after = _replayed(before[name], log, row_steps)
                    assert (after == now).all() and sorted(now.tolist()) == list(range(R))
                    for k in range(n_rows):
                        assert (rows[name][k] == want_rows[k]).all(), (calls, want_energy, n, k)
                    attempts += len(want_steps)
                at += n
            assert integ.step == STEPS and attempts == (3 if moved else 0)
