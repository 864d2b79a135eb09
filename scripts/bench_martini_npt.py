#!/usr/bin/env python3
"""dev: what pressure coupling costs the MARTINI integrator, on bench.py's bilayer (the golden membrane tiled 4 x 4,
20 480 beads, fp32, dt 0.02 ps, 273 K) at bench.py's policy (skin 0.5 nm, rebuild every 12, pruned rows 0.2 nm / 4).

  nvt        steps/s of advance(steps) without a barostat - every repeat printed, for the run-to-run spread.  Uses nothing
             a commit without the barostat lacks: ``--root DIR`` imports the package of another checkout, so that two
             commits can be timed in alternating fresh processes.
  npt        the same with stochastic cell rescaling every 12 steps (semi-isotropic, 3e-4 / 0 per bar, 1 bar, tau_p 1 ps):
             steps/s, and from the difference the wall time of one event - closing launch, pressure launch, mu, scaling,
             synchronisation, and the list rebuild it forces
  pressure   wall time of one pressure() call on a closed frame with a valid list: pressure launch + reduction + the
             synchronisation

One JSON line on stdout; ``--out FILE`` writes it too.  Every figure over at least ``--repeats`` x ``--steps`` steps,
each repeat ended by a device synchronise.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="checkout whose package and bench.py are imported")
ap.add_argument("--steps", type=int, default=2400)
ap.add_argument("--warmup", type=int, default=600)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--nvt-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
import bench  # noqa: E402
from mythos_amd.hip_system import MartiniLangevinIntegrator  # noqa: E402

EVERY = 12
dev = torch.device("cuda", 0)
system, _, xt, bt = bench.martini_system(dev, torch.float32)
kT = 0.0083144626 * 273.0


def integrator():
    integ = MartiniLangevinIntegrator(system, dt=0.02, kT=kT, gamma=1.0, seed=0)
    integ.set_neighbor_policy(0.5, 12)
    integ.set_inner_list(0.2, 4)
    pos = torch.as_tensor(xt, dtype=torch.float32, device=dev).contiguous()
    integ.load(pos, integ.init_velocities(), bt)
    return integ


def rates(integ):
    integ.advance(args.warmup)
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        integ.advance(args.steps)
        torch.cuda.synchronize(dev)
        out.append(args.steps / (time.perf_counter() - t0))
    return out


res = {"root": args.root, "n": system.n, "steps": args.steps, "repeats": args.repeats}
nvt = rates(integrator())
res["nvt_steps_per_s"] = nvt
if not args.nvt_only:
    integ = integrator()
    integ.set_barostat("c-rescale", "semiisotropic", ref_p=(1.0, 1.0), compressibility=(3e-4, 0.0), tau_p=1.0, every=EVERY)
    npt = rates(integ)
    res["npt_steps_per_s"] = npt
    res["box_after_npt"] = integ.box.tolist()
    t_nvt, t_npt = args.steps / (sum(nvt) / len(nvt)), args.steps / (sum(npt) / len(npt))
    res["event_us"] = 1e6 * (t_npt - t_nvt) / (args.steps / EVERY)
    integ.pressure()  # (closes the frame; the list is valid)
    t0 = time.perf_counter()
    for _ in range(200):
        p = integ.pressure()
    res["pressure_call_us"] = 1e6 * (time.perf_counter() - t0) / 200
    res["pressure_bar"] = p["pressure"].tolist()
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).write_text(line + "\n")
