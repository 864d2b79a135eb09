#!/usr/bin/env python3
"""dev: aggregate rate of the MARTINI temperature ensemble against the same replicas run one after another.

The DMPC bilayer fixture (1 280 beads, tests/golden/martini), dt 0.02 ps, gamma 1 / ps, temperatures 273 K ... 320 K spread
over the replicas, list policy skin 0.5 nm rebuilt every 12 steps (bench.py's MARTINI policy), NVT and NPT (c-rescale
semi-isotropic every 12 steps, compressibility 3e-4 / bar in xy and z, tau_p 12 ps: the md.mdp's coupling type with the
height free as well, so that every edge of every replica moves).  For R in --replicas: MartiniEnsembleIntegrator against R
MartiniLangevinIntegrator of the same build stepped in sequence, replica-steps / s from wall-clock time around
synchronised calls (best of --repeats), and from the integrator's timing getters the sampled step-kernel time and the
loop time per launch - their difference is what list builds, coupling events and gaps cost.

usage: python scripts/bench_martini_ensemble.py [--steps 2000] [--replicas 1,2,4,8,16] [--dtypes f32,f64] [--out FILE.json]
Prints one JSON line per configuration and a markdown table at the end.

--exchange-every 0,1000,100: the replica-exchange study instead (set_exchange; NVT, or NPT with --npt): for every R and every
value E the ensemble's replica-steps / s (best of --repeats, every repeat's time kept to show the spread), the acceptance
rate per rung pair, and the cost per event against the E = 0 run of the same build: (t_E - t_0) / events.  The sequential
single integrators are not run."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

KB = 0.0083144626
BARO = dict(kind="c-rescale", coupling="semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 3e-4), tau_p=12.0, every=12)


def timed(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def timed_all(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def exchange_study(args, sysm, dname, x, box):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    results = []
    for n_rep in (int(r) for r in args.replicas.split(",")):
        kTs = KB * np.linspace(273.0, 320.0, n_rep)
        base = None
        for every in (int(e) for e in args.exchange_every.split(",")):
            ens = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=kTs, gamma=1.0, seeds=1)
            ens.set_neighbor_policy(0.5, 12)
            if args.npt:
                ens.set_barostat(**BARO)
            if every:
                ens.set_exchange(every, 20260317)
            pos = torch.tensor(np.broadcast_to(x[3], (n_rep, *x[3].shape)).copy(), dtype=sysm.dtype, device=sysm.device)
            ens.load(pos, ens.init_velocities(), box[3])
            ens.advance(args.warmup)
            step0 = ens.step
            times = timed_all(lambda: ens.advance(args.steps), args.repeats)
            t = min(times)
            events = ((step0 + args.steps) // every - step0 // every) if every else 0  # of the first repeat; the others' differ by at most one
            att, acc = ens.exchange_counts()
            row = dict(dtype=dname, ensemble="NPT" if args.npt else "NVT", replicas=n_rep, steps=args.steps, exchange_every=every,
                       replica_steps_per_s=n_rep * args.steps / t, seconds=times, events_per_call=events, recoveries=ens.last_recoveries(),
                       attempts=att.tolist(), accepts=acc.tolist(), acceptance=[(a / n if n else None) for a, n in zip(acc.tolist(), att.tolist())])
            if every == 0:
                base = t
            if every and base is not None and events:
                row["us_per_event"] = 1e6 * (t - base) / events
                row["slowdown_vs_exchange_off"] = t / base - 1.0
            print(json.dumps(row), flush=True)
            results.append(row)
            del ens
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--replicas", default="1,2,4,8,16")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--exchange-every", default=None, help="e.g. 0,1000,100: the replica-exchange study (see the module docstring)")
    ap.add_argument("--npt", action="store_true", help="the exchange study under the barostat")
    args = ap.parse_args()
    from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniLangevinIntegrator, MartiniSystem
    from tests import martini_helpers as MH

    s = MH.system()
    top = s["top"]
    x, box, _ = MH.frames("lj")
    ff = (s["types"], s["sigma"], s["eps"], np.asarray(top.bonded_neighbors), s["bond_k"], s["bond_r0"], np.asarray(top.angles),
          s["angle_k"], s["angle_t0"])
    results = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        sysm = MartiniSystem(*ff, dtype=dtype)
        if args.exchange_every is not None:
            results += exchange_study(args, sysm, dname, x, box)
            continue
        for npt in (False, True):
            for n_rep in (int(r) for r in args.replicas.split(",")):
                kTs = KB * np.linspace(273.0, 320.0, n_rep) if n_rep > 1 else np.array([KB * 273.0])

                def setup(integ):
                    integ.set_neighbor_policy(0.5, 12)
                    integ.set_timing(8)
                    if npt:
                        integ.set_barostat(**BARO)

                ens = MartiniEnsembleIntegrator(sysm, dt=0.02, kT=kTs, gamma=1.0, seeds=1)
                setup(ens)
                pos = torch.tensor(np.broadcast_to(x[3], (n_rep, *x[3].shape)).copy(), dtype=dtype, device=sysm.device)
                ens.load(pos, ens.init_velocities(), box[3])
                ens.advance(args.warmup)
                t_ens = timed(lambda: ens.advance(args.steps), args.repeats)
                tm = ens.last_kernel_ms()
                rec = ens.last_recoveries()
                singles = []
                for r in range(n_rep):
                    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=float(kTs[r]), gamma=1.0, seed=1 + r)
                    setup(integ)
                    integ.load(pos[r].contiguous(), integ.init_velocities(), box[3])
                    integ.advance(args.warmup)
                    singles.append(integ)

                def sequential():
                    for integ in singles:
                        integ.advance(args.steps)

                t_seq = timed(sequential, args.repeats)
                ts = singles[0].last_kernel_ms()
                row = dict(dtype=dname, ensemble="NPT" if npt else "NVT", replicas=n_rep, steps=args.steps,
                           ensemble_replica_steps_per_s=n_rep * args.steps / t_ens, sequential_replica_steps_per_s=n_rep * args.steps / t_seq,
                           ensemble_kernel_ms=tm["kernel_ms"], ensemble_loop_ms_per_launch=tm["loop_ms_per_launch"],
                           ensemble_builds_events_gaps_share=1.0 - tm["kernel_ms"] / tm["loop_ms_per_launch"] if tm["loop_ms_per_launch"] else None,
                           single_kernel_ms=ts["kernel_ms"], single_loop_ms_per_launch=ts["loop_ms_per_launch"], ensemble_recoveries=rec)
                print(json.dumps(row), flush=True)
                results.append(row)
                del ens, singles
    if args.exchange_every is not None:
        print("\n| dtype | ensemble | R | exchange every | replica-steps/s | repeats (s) | us / event | against exchange off | acceptance per rung pair |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in results:
            acc = ", ".join("-" if a is None else f"{a:.2f}" for a in r["acceptance"])
            print(f"| {r['dtype']} | {r['ensemble']} | {r['replicas']} | {r['exchange_every']} | {r['replica_steps_per_s']:.0f} | "
                  f"{', '.join(f'{t:.4f}' for t in r['seconds'])} | {r.get('us_per_event', float('nan')):.1f} | "
                  f"{100 * r.get('slowdown_vs_exchange_off', 0.0):+.2f} % | {acc} |")
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(results, indent=1))
        return
    print("\n| dtype | ensemble | R | ensemble replica-steps/s | sequential replica-steps/s | ratio | step kernel ms | loop ms / launch | builds + events + gaps |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in results:
        share = r["ensemble_builds_events_gaps_share"]
        print(f"| {r['dtype']} | {r['ensemble']} | {r['replicas']} | {r['ensemble_replica_steps_per_s']:.0f} | {r['sequential_replica_steps_per_s']:.0f} | "
              f"{r['ensemble_replica_steps_per_s'] / r['sequential_replica_steps_per_s']:.2f} | {r['ensemble_kernel_ms']:.4f} | "
              f"{r['ensemble_loop_ms_per_launch']:.4f} | {'' if share is None else f'{100 * share:.0f} %'} |")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
