#!/usr/bin/env python3
"""dev: the MBAR iteration (mythos_mbar_iterate, csrc/mbar.hip) against the same iteration written in torch on the same GPU,
and a full solve.  A tool: it belongs to neither the benchmark nor the tests.

Shapes: K umbrella windows of ``per`` exact Gaussian frames each, 1.5 sigma apart, one coordinate - 64 x 10 000 (the size
of a production PMF) and 8 x 1 000.

The yardstick is what a user would write today: the (K, N) bias matrix materialised once, then per iteration two
``torch.logsumexp`` over it (L_n over the windows, f_k over the frames).  One iteration of each path from the same f is
compared before anything is timed.  Times are device events around ``--batch`` back-to-back iterations, nothing read back,
after a warm-up; the three paths - HIP from the window table, HIP from the matrix, torch - alternate repeat by repeat in
this one process, and mean and min ... max over ``--rounds`` are reported.  The solve is timed on the host clock around a
call that ends in a synchronise, with the iterations it took.

The share of the solve spent in launch gaps is 1 - (kernel time) / (wall time): kernel time is the sum over the two
kernels in a ``rocprofv3 --kernel-trace --stats -- python scripts/measure_mbar.py --solve-only ...`` run of its own (the
trace slows the host: the wall time is taken from the run without it).
Prints one JSON line per shape; ``--out`` also writes them to a file.
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
M = importlib.import_module("mythos_amd.observables.mbar")  # noqa: E402

SHAPES = {"large": (64, 10_000), "small": (8, 1_000)}


def windows(K, per, spacing_sigma=1.5, k0=2.0, k=8.0, kT=1.0, seed=0):
    """Exact samples of K harmonic windows on a harmonic base (reduced units): xi (N, 1), table (K, 1, 4), n_k."""
    sigma = np.sqrt(kT / (k0 + k))
    c = (np.arange(K) - 0.5 * (K - 1)) * spacing_sigma * sigma * (k0 + k) / k
    xi = (k * c / (k0 + k))[:, None] + sigma * np.random.default_rng(seed).standard_normal((K, per))
    table = np.zeros((K, 1, 4))
    table[:, 0, 1], table[:, 0, 2] = k, c
    return xi.reshape(-1, 1), table, np.full(K, per, dtype=np.int64), kT


def torch_iteration(u, ln_n, f):
    L = torch.logsumexp((ln_n + f)[:, None] - u, dim=0)
    g = -torch.logsumexp(-u - L[None, :], dim=1)
    return g - g[0]


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def stats(v):
    return dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))


def measure(name, args, dev):
    K, per = SHAPES[name]
    xi_h, table, n_k, kT = windows(K, per)
    N = K * per
    xi = torch.tensor(xi_h, device=dev)
    u = torch.tensor(0.5 * table[:, 0, 1, None] * (xi_h[None, :, 0] - table[:, 0, 2, None]) ** 2 / kT, device=dev)
    ln_n = torch.log(torch.tensor(n_k, dtype=torch.float64, device=dev))
    by_table, by_matrix = M._MbarPlan(N, K, dev), M._MbarPlan(N, K, dev)
    by_table.set_windows(table, np.full(K, kT), n_k, xi)
    by_matrix.set_matrix(u, n_k)
    delta = torch.empty(1, dtype=torch.float64, device=dev)
    out = dict(shape=name, K=K, N=N)
    if not args.solve_only:
        f0 = torch.linspace(0.0, 3.0, K, dtype=torch.float64, device=dev)
        want = torch_iteration(u, ln_n, f0)
        for plan in (by_table, by_matrix):
            f = f0.clone()
            plan.iterate(f, 1, delta)
            assert float((f - want).abs().max()) < 1e-10, "the paths disagree"
        state = {p: torch.zeros(K, dtype=torch.float64, device=dev) for p in ("table", "matrix", "torch")}

        def step_torch():
            state["torch"] = torch_iteration(u, ln_n, state["torch"])

        paths = {"table": lambda: by_table.iterate(state["table"], 1, delta), "matrix": lambda: by_matrix.iterate(state["matrix"], 1, delta),
                 "torch": step_torch}
        for fn in paths.values():  # warm-up: code objects, the allocator's blocks
            event_ms(fn, 3)
        ms = {p: [] for p in paths}
        for _ in range(args.rounds):
            for p, fn in paths.items():
                ms[p].append(event_ms(fn, args.batch))
        out["iteration_ms"] = {p: stats(v) for p, v in ms.items()}
        out["torch_over_table"] = out["iteration_ms"]["torch"]["mean"] / out["iteration_ms"]["table"]["mean"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f, iterations, d = by_table.solve(args.tol, args.max_iter, 32)
    torch.cuda.synchronize()
    out["solve"] = dict(wall_s=time.perf_counter() - t0, iterations=iterations, delta=d, tol=args.tol)
    by_table.close(), by_matrix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=20, help="back-to-back iterations per timed sample")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=200_000)
    ap.add_argument("--solve-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_mbar.py needs a GPU: it does not fall back")
    dev = torch.device("cuda", 0)
    lines = []
    for name in args.shapes.split(","):
        lines.append(json.dumps(measure(name, args, dev)))
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
