#!/usr/bin/env python3
"""dev: the Gram and segment-moment launches of MBAR (mythos_mbar_gram, mythos_mbar_segment_moments, csrc/mbar.hip) and
the Newton solve against the fixed-point solve.  A tool: it belongs to neither the benchmark nor the tests; the sibling of
scripts/measure_mbar.py, whose windows it takes.

Shape: 64 umbrella windows of 10 000 exact Gaussian frames each, 1.5 sigma apart, one coordinate (``--shape small``: 8 x
1 000), from the window table and from the materialised matrix.

One ``gram`` call (with and without the column sums) and one ``segment_moments`` call with one segment are timed with device
events around ``--batch`` back-to-back calls, nothing read back, after a warm-up; the two sources alternate repeat by repeat
in this one process, and median and min ... max over ``--rounds`` are reported.  The solves are timed on the host clock around
a call that ends in a synchronise - median over ``--solves`` calls after one warm-up call - with the iterations they took.

``--parent-lib PATH`` loads another build of the library - the parent commit's, which has neither new entry point - and
times the fixed-point solve alone: the figure the Newton solve is compared with.
Prints one JSON line per source; ``--out`` also writes them to a file.
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
sys.path.insert(0, str(ROOT / "scripts"))

NEW = ("mythos_mbar_gram", "mythos_mbar_segment_moments")


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def timed_solve(plan, solver, args):
    wall, it = [], 0
    for i in range(args.solves + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, it, d = plan.solve(args.tol, args.max_iter, 32, solver=solver) if solver else plan.solve(args.tol, args.max_iter, 32)
        torch.cuda.synchronize()
        if i:  # the first call warms up
            wall.append(time.perf_counter() - t0)
    return dict(wall_s=stats(wall), iterations=it, delta=d, tol=args.tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="large", choices=["large", "small"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="a build without the new entry points: the fixed-point solve alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_mbar_newton.py needs a GPU: it does not fall back")
    if args.parent_lib:
        os.environ["MYTHOS_HIP_LIB"] = str(Path(args.parent_lib).resolve())
    from mythos_amd import _lib

    if args.parent_lib:
        for name in NEW:
            _lib._SIGS.pop(name)
    import importlib

    import measure_mbar as MM

    M = importlib.import_module("mythos_amd.observables.mbar")
    dev = torch.device("cuda", 0)
    K, per = MM.SHAPES[args.shape]
    xi_h, table, n_k, kT = MM.windows(K, per)
    N = K * per
    xi = torch.tensor(xi_h, device=dev)
    u = torch.tensor(0.5 * table[:, 0, 1, None] * (xi_h[None, :, 0] - table[:, 0, 2, None]) ** 2 / kT, device=dev)
    plans = {"table": M._MbarPlan(N, K, dev), "matrix": M._MbarPlan(N, K, dev)}
    plans["table"].set_windows(table, np.full(K, kT), n_k, xi)
    plans["matrix"].set_matrix(u, n_k)
    out = {src: dict(shape=args.shape, K=K, N=N, source=src, library=str(_lib.lib_path())) for src in plans}
    if not args.parent_lib:
        f = torch.linspace(0.0, 3.0, K, dtype=torch.float64, device=dev)
        calls = {"gram": lambda p: p.gram(f, colsum=False), "gram_colsum": lambda p: p.gram(f), "segment_moments": lambda p: p.segment_moments(f)}
        ga, gb = (p.gram(f)[0] for p in plans.values())
        assert float((ga - gb).abs().max()) < 1e-10, "the sources disagree"
        ms = {src: {c: [] for c in calls} for src in plans}
        for rnd in range(args.rounds + 1):
            for src, p in plans.items():
                for c, fn in calls.items():
                    t = MM.event_ms(lambda: fn(p), args.batch if rnd else 2)
                    if rnd:  # round 0 warms up: code objects, the lazily allocated partials
                        ms[src][c].append(t)
        for src in plans:
            out[src]["call_ms"] = {c: stats(v) for c, v in ms[src].items()}
    for src, p in plans.items():
        if not args.parent_lib:
            out[src]["newton"] = timed_solve(p, "newton", args)
        out[src]["fixed_point"] = timed_solve(p, None if args.parent_lib else "fixed-point", args)
        p.close()
    lines = [json.dumps(o) for o in out.values()]
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
