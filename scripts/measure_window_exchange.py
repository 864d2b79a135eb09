#!/usr/bin/env python3
"""dev: the cost of a window-exchange event of the MARTINI ensemble (mythos_martini_langevin_set_window_exchange,
csrc/martini_window_exchange.inc) against the temperature-exchange event, and the control of the step path.  A tool: it
belongs to neither the benchmark nor the tests.

System: the 1 280-bead DMPC bilayer of the golden frames, R = 8 replicas at 300 K, one pull coordinate - the z distance
between the leaflets' PO4 centres of mass, k = 5 000 kJ/mol/nm^2, windows 0.02 nm apart -, dt = 0.02 ps, neighbour policy
(0.4, 5), fp32 and fp64.

``events``  per precision, ``--steps`` steps (a multiple of 100) timed on the host clock around one ``advance`` that ends in
            a synchronise, after a warm-up call; exchange every 100 steps against exchange off on the same handle, the two
            alternated repeat by repeat; the cost per event is the difference of the two wall times over the number of
            events.  The same for the temperature-exchange event on the same build in the same process: the same ensemble
            without the set, kT = 300 ... 320 K.  Median and min ... max over ``--repeats``; the acceptance per rung pair.
``control`` the section 3.5n figure: the single integrator with that one pull coordinate, ``loop_ms_per_launch`` of
            ``set_timing`` over 2 000 steps, five repeats.  ``--parent-lib PATH`` runs it on another build of the library - the
            parent commit's, which lacks the new entry points.
Prints one JSON line per result; ``--out`` also writes them to a file.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KB = 0.0083144626
NEW = ("mythos_martini_window_exchange_check", "mythos_martini_langevin_set_window_exchange", "mythos_martini_langevin_set_windows",
       "mythos_martini_langevin_get_windows", "mythos_martini_langevin_last_windows", "mythos_martini_langevin_last_window_exchanges",
       "mythos_martini_langevin_window_exchange_counts")


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def bilayer():
    from mythos_amd.energy import martini as M
    from mythos_amd.simulators.hip_martini import lower_martini
    from tests import martini_helpers as MH

    s = MH.system()
    x, box, _ = MH.frames("lj")
    top = s["top"]
    ap = {k: (np.deg2rad(v) if k.startswith("angle_theta0_") else v) for k, v in s["angle_params"].items()}
    fn = M.MartiniComposedEnergyFunction([M.LJ.from_topology(topology=top, params=M.LJConfiguration(**s["lj_params"])),
                                          M.Bond.from_topology(topology=top, params=M.BondConfiguration(**s["bond_params"])),
                                          M.Angle.from_topology(topology=top, params=M.AngleConfiguration(**ap))])
    po4 = np.flatnonzero(np.asarray(top.atom_names) == "PO4")
    z = x[3][po4, 2]
    return dict(low=lower_martini(fn), x=x[3], box=box[3], lower=po4[z < z.mean()], upper=po4[z >= z.mean()])


def restraints(b, n_rep):
    from mythos_amd.simulators.martini_restraints import MartiniRestraints, PullCoordinate, PullGroup

    d0 = abs(b["x"][b["upper"], 2].mean() - b["x"][b["lower"], 2].mean())
    init = d0 + 0.02 * np.arange(n_rep) if n_rep > 1 else d0
    return MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(members=tuple(b["lower"]), pbc_ref=int(b["lower"][0])),
                                                   group_b=PullGroup(members=tuple(b["upper"]), pbc_ref=int(b["upper"][0])),
                                                   geometry="distance", dim=(False, False, True), k=5000.0, init=init, periodic=True)])


def system(b, dtype):
    from mythos_amd.hip_system import MartiniSystem

    low = b["low"]
    return MartiniSystem(low["types"], low["sigma"], low["eps"], low["bonds"], low["bond_k"], low["bond_r0"], low["angles"], low["angle_k"],
                         low["angle_t0"], angle_kind=low["angle_kind"], dtype=dtype)


def timed_advance(integ, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    integ.advance(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(b, dtype, args):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    R, out = 8, {}
    sysm = system(b, dtype)
    for mode in ("window", "temperature"):
        kT = KB * (np.full(R, 300.0) if mode == "window" else np.linspace(300.0, 320.0, R))
        integ = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=kT, gamma=1.0, seeds=11)
        integ.set_neighbor_policy(0.4, 5)
        switch = integ.set_window_exchange if mode == "window" else integ.set_exchange
        if mode == "window":
            integ.set_restraints(restraints(b, R), box=b["box"])
        pos = torch.tensor(np.broadcast_to(b["x"], (R, *b["x"].shape)).copy(), dtype=dtype, device=sysm.device).contiguous()
        integ.load(pos, integ.init_velocities(), b["box"])
        switch(100, 3)
        integ.advance(args.steps)  # warm-up, and the windows spread
        wall = {"on": [], "off": []}
        for _ in range(args.repeats):
            for key, every in (("off", 0), ("on", 100)):
                switch(every, 3)
                wall[key].append(timed_advance(integ, args.steps))
        n_events = args.steps // 100
        per_event = [(a - o) / n_events for a, o in zip(wall["on"], wall["off"])]
        att, acc = integ.window_exchange_counts() if mode == "window" else integ.exchange_counts()
        out[mode] = dict(mode=mode, precision=str(dtype).split(".")[-1], replicas=R, steps=args.steps, events_per_call=n_events,
                         wall_ms_on=stats(wall["on"]), wall_ms_off=stats(wall["off"]), ms_per_event=stats(per_event),
                         attempts=att.tolist(), accepts=acc.tolist(), acceptance=[round(float(a) / max(int(n), 1), 3) for a, n in zip(acc, att)])
        integ.close()
    sysm.close()
    return list(out.values())


def control(b, dtype, args):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    sysm = system(b, dtype)
    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=KB * 300.0, gamma=1.0, seed=11)
    integ.set_neighbor_policy(0.4, 5)
    integ.set_restraints(restraints(b, 1), box=b["box"])
    integ.set_timing(2000)
    pos = torch.tensor(b["x"], dtype=dtype, device=sysm.device).contiguous()
    integ.load(pos, integ.init_velocities(), b["box"])
    integ.advance(2000)
    loop = []
    for _ in range(5):
        integ.advance(2000)
        torch.cuda.synchronize()
        loop.append(integ.last_kernel_ms()["loop_ms_per_launch"] * 1e3)
    integ.close()
    sysm.close()
    return [dict(mode="control: one pull coordinate, single integrator", precision=str(dtype).split(".")[-1], parent=bool(args.parent_lib),
                 loop_us_per_launch=stats(loop))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("events", "control"))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="control only: a build without the new entry points")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_window_exchange.py needs a GPU: it does not fall back")
    if args.steps % 100 or args.steps < 100:
        raise SystemExit("--steps must be a positive multiple of 100")
    if args.parent_lib:
        if args.what != "control":
            raise SystemExit("--parent-lib serves the control alone")
        os.environ["MYTHOS_HIP_LIB"] = str(Path(args.parent_lib).resolve())
        from mythos_amd import _lib

        for name in NEW:
            _lib._SIGS.pop(name)
    b = bilayer()
    lines = []
    for dtype in (torch.float32, torch.float64):
        for rec in (events if args.what == "events" else control)(b, dtype, args):
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
