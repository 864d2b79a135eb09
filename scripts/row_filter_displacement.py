#!/usr/bin/env python
"""The curve behind the two constants of mythos_amd/csrc/row_filter_plan.h, without a GPU: the largest centre displacement
of any nucleotide of the benchmark's duplex over 50 ... 800 steps, and the neighbours per nucleotide by centre distance,
on the fp64 C++/OpenMP port (oracle/cpu_port) - thermalised, then a number of windows.

    python scripts/row_filter_displacement.py --bp 12000 --thermalise 600 --windows 3

The rule: margin >= 1.15 * 2 * the displacement over kCandEvery * 50 steps.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

R_CUT, SKIN, EVERY = 3.25, 0.9, 50  # the benchmark's policy (bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=12000)
    ap.add_argument("--thermalise", type=int, default=600)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dt", type=float, default=0.005)
    args = ap.parse_args()

    from scipy.spatial import cKDTree

    from mythos_amd import _lib
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.input import defaults
    from mythos_amd.utils import generators
    from oracle import cpu_port

    sim, cfg = defaults.default_configs_for("dna2")
    kT = sim["kT"]
    top, c0, q0 = generators.ideal_duplex(args.bp, model=2, seed=1234)
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=kT, salt_conc=sim["salt_conc"], half_charged_ends=True), _lib.param_names())
    cpu_port.set_threads(args.threads)
    port = cpu_port.CpuPort(2, top.seq, top.is_end, top.bonded_neighbors, flat.detach().numpy())
    kw = dict(dt=args.dt, kT=kT, gamma_t=kT / sim["diff_coef"], gamma_r=kT / sim["rot_diff_coef"], mass=sim["nucleotide_mass"],
              inertia=sim["moment_of_inertia"], seed=0, r_cut=R_CUT, skin=SKIN, rebuild_every=EVERY)
    x, q = np.array(c0, dtype=np.float64), np.array(q0, dtype=np.float64)
    p, L = np.zeros_like(x), np.zeros_like(x)
    port.run(x, q, p, L, args.thermalise, step0=0, **kw)
    done = args.thermalise
    marks = (50, 100, 200, 400, 800)
    print(f"{top.n_nucleotides} nucleotides, thermalised {args.thermalise} steps; largest centre displacement by window")
    print("window  " + "  ".join(f"{m:>6d}" for m in marks))
    for w in range(args.windows):
        x0, at, row = x.copy(), 0, []
        for m in marks:
            port.run(x, q, p, L, m - at, step0=done, **kw)
            done += m - at
            at = m
            row.append(float(np.linalg.norm(x - x0, axis=1).max()))
        print(f"{w:>6d}  " + "  ".join(f"{v:6.3f}" for v in row), flush=True)
    tree = cKDTree(x)
    radii = (R_CUT + SKIN, 4.65, 5.15, 5.75, 6.15, 6.65)
    counts = [tree.query_pairs(r, output_type="ndarray").shape[0] * 2.0 / x.shape[0] for r in radii]
    print("neighbours per nucleotide by centre distance (bonded ones included): " +
          ", ".join(f"{c:.1f} within {r:.2f}" for r, c in zip(radii, counts)))


if __name__ == "__main__":
    main()
