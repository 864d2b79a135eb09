#!/usr/bin/env python3
"""dev: the block bootstrap of MBAR - the batched weighted solve (mythos_mbar_boot_colsums, mythos_mbar_boot_binned,
csrc/mbar.hip), the statistical inefficiency (csrc/timeseries.hip) - against the same bootstrap written as a loop over the
public interface of the commit before it.  A tool: it belongs to neither the benchmark nor the tests; the sibling of
scripts/measure_mbar_newton.py.

Shapes: 64 umbrella windows of 10 000 frames each (``large``) and 8 x 1 000 (``small``), exact Gaussian marginals 1.5 sigma
apart with AR(1) frames at phi = 0.8 (g = 9) inside a window; B = ``--replicates`` (200) moving-block replicates of block
length ``--block`` (27 = 3 g) - the same starts, from ``numpy.random.default_rng(seed)``, for both paths.

The loop (``--loop-only`` runs nothing else and uses only names the parent commit has; run it in a checkout of that commit):
per replicate, gather the resampled frames on the device and call ``mbar_umbrella(..., solver="newton")`` on them.
The batched path: ``mbar_umbrella(..., solver="newton", bootstrap=B, block=l)``, whole - the central solve, the
multiplicities and the chord iterations included - and the central solve alone next to it.
Both are timed on the host clock around calls that end in a synchronise; medians over ``--repeats`` after one warm-up.
Without ``--loop-only`` the script also times, with device events around ``--batch`` back-to-back calls, one
``boot_colsums`` call of B and of 2 B rows, one weighted ``uncertainty(method="bootstrap", weights=w)`` call (host clock: it
reads back), and ``statistical_inefficiency``.  Prints one JSON line per shape; ``--out`` also writes them to a file.
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

SHAPES = {"large": (64, 10_000), "small": (8, 1_000)}


def windows(K, per, phi=0.8, spacing_sigma=1.5, k0=2.0, k=8.0, kT=1.0, seed=0):
    """K harmonic windows on a harmonic base (reduced units), AR(1) frames inside a window: xi (N, 1), centres, k, n_k, kT."""
    sigma = np.sqrt(kT / (k0 + k))
    c = (np.arange(K) - 0.5 * (K - 1)) * spacing_sigma * sigma * (k0 + k) / k
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((K, per))
    for t in range(1, per):
        z[:, t] = phi * z[:, t - 1] + np.sqrt(1.0 - phi * phi) * z[:, t]
    xi = (k * c / (k0 + k))[:, None] + sigma * z
    return np.ascontiguousarray(xi.reshape(-1, 1)), c, k, np.full(K, per, dtype=np.int64), kT


def restraint_set(c, k):
    from mythos_amd.simulators.martini_restraints import MartiniRestraints, PullCoordinate, PullGroup

    return MartiniRestraints(pulls=[PullCoordinate(group_a=None, group_b=PullGroup(members=(0,)), geometry="direction", vec=(0, 0, 1),
                                                   k=k, init=c.copy(), periodic=False)])


def block_starts(n_k, block, n_boot, seed):
    """The starts of ``block_resample`` (its documented order of draws), with numpy alone."""
    rng = np.random.default_rng(seed)
    starts, lengths = [], []
    for n in n_k:
        count = -(-int(n) // block)
        length = np.full(count, block, dtype=np.int64)
        length[-1] = n - (count - 1) * block
        starts.append(rng.integers(0, n - length + 1, size=(n_boot, count), dtype=np.int64))
        lengths.append(length)
    return starts, lengths


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def wall(fn, repeats):
    out = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:  # the first call warms up
            out.append(time.perf_counter() - t0)
    return stats(out)


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--block", type=int, default=27)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=5, help="back-to-back calls per timed sample")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--loop-only", action="store_true", help="the per-replicate loop alone, with the parent commit's names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_mbar_bootstrap.py needs a GPU: it does not fall back")
    M = importlib.import_module("mythos_amd.observables.mbar")
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        K, per = SHAPES[shape]
        xi_h, c, k, n_k, kT = windows(K, per)
        N, B = K * per, args.replicates
        xi, rs = torch.tensor(xi_h, device=dev), restraint_set(c, k)
        out = dict(shape=shape, K=K, N=N, replicates=B, block=args.block, library=str(M._lib.lib_path()))
        if args.loop_only:
            starts, lengths = block_starts(n_k, args.block, B, args.seed)
            off = np.concatenate([[0], np.cumsum(n_k)])
            span = [np.concatenate([np.arange(length) for length in ls]) for ls in lengths]  # a frame's place inside its block

            def loop():
                fs = []
                for b in range(B):
                    idx = np.concatenate([off[w] + np.repeat(starts[w][b], lengths[w]) + span[w] for w in range(K)])
                    frames = xi[torch.as_tensor(idx, device=dev)].contiguous()
                    fs.append(M.mbar_umbrella(frames, rs, kT, n_k=n_k, solver="newton").f)
                return torch.stack(fs)

            out["loop_wall_s"] = wall(loop, args.repeats)
            boot_f = loop()
            out["loop_sigma_last_first"] = float((boot_f[:, -1] - boot_f[:, 0]).std())
        else:
            out["central_wall_s"] = wall(lambda: M.mbar_umbrella(xi, rs, kT, n_k=n_k, solver="newton"), args.repeats)
            out["batched_wall_s"] = wall(lambda: M.mbar_umbrella(xi, rs, kT, n_k=n_k, solver="newton", bootstrap=B, block=args.block,
                                                                 boot_seed=args.seed), args.repeats)
            res = M.mbar_umbrella(xi, rs, kT, n_k=n_k, solver="newton", bootstrap=B, block=args.block, boot_seed=args.seed)
            out["batched_sigma_last_first"] = float((res.boot_f[:, -1] - res.boot_f[:, 0]).std())
            out["inefficiency_wall_s"] = wall(lambda: M.statistical_inefficiency(xi, n_k), args.repeats)
            out["g_mean"] = float(M.statistical_inefficiency(xi, n_k).mean())
            resample = M.block_resample(n_k, args.block, B, args.seed)
            m = resample.multiplicities(0, min(B, resample.batch_size()), dev)
            rows = int(m.shape[0])
            out["multiplicities_wall_s"] = wall(lambda: resample.multiplicities(0, rows, dev), args.repeats)
            plan = M._MbarPlan(N, K, dev)
            table = M.window_table(rs, K)
            plan.set_windows(table, np.full(K, kT), n_k, xi)
            delta = 0.01 * torch.randn(rows, K, dtype=torch.float64, device=dev)
            both = torch.cat([m.view(torch.int16), m.view(torch.int16)]).contiguous().view(torch.uint16)
            delta2 = torch.cat([delta, delta]).contiguous()
            calls = {f"boot_colsums_{rows}_rows": lambda: plan.boot_colsums(res.f, delta, m),
                     f"boot_colsums_{2 * rows}_rows": lambda: plan.boot_colsums(res.f, delta2, both)}
            ms = {name: [] for name in calls}
            for rnd in range(args.rounds + 1):
                for name, fn in calls.items():
                    t = event_ms(fn, args.batch if rnd else 2)
                    if rnd:
                        ms[name].append(t)
            out["call_ms"] = {name: stats(v) for name, v in ms.items()}
            plan.close()
            x = xi_h[:, 0]
            pmf = M.UmbrellaPMF(restraints=rs, kT=kT, edges=np.linspace(x.min(), x.max() + 1e-9, 41), solver="newton")
            pmf.fit(xi, n_k=n_k, bootstrap=B, block=args.block, boot_seed=args.seed)
            w = torch.rand(N, dtype=torch.float64, device=dev) + 0.5
            out["weighted_uncertainty_wall_s"] = wall(lambda: pmf.uncertainty(method="bootstrap", weights=w), args.repeats)
            pmf.release()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
