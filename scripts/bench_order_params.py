#!/usr/bin/env python3
"""dev: the order-parameter call against its yardstick, the energy call (no gradients) of the same frames, on the
umbrella-sampling run of tests/golden/melting_temp (12 nt, oxDNA1, periodic box 20, the op.txt of the run: ``bond`` and
``mindistance`` over the six native pairs): its 384 frames, and the same frames tiled to 65 535.

Per shape and precision, the two calls alternating in one process after warm-up: ms per call with a device synchronise at
the end of the window (median, min, max of the repeats), and the host share - the time until the call RETURNS, the work
still queued.  One JSON line per shape and precision.

--once: one call of each per shape and precision, for a kernel trace (rocprofv3 --kernel-trace --stats, a run of its own).
"""
import argparse
import gzip
import json
import statistics
import sys
import tempfile
import time
import warnings
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mythos_amd import _lib  # noqa: E402
from mythos_amd.energy import flat_params as fp  # noqa: E402
from mythos_amd.hip_system import OxdnaSystem  # noqa: E402
from mythos_amd.input import defaults, topology, trajectory  # noqa: E402
from mythos_amd.input.order_parameters import read_order_parameters  # noqa: E402


def load(fixture_dir: Path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        top = topology.from_oxdna_file(fixture_dir / "sys.top")
    with tempfile.TemporaryDirectory() as tmp:  # (the fixture keeps its trajectory compressed)
        plain = Path(tmp) / "trajectory.dat"
        plain.write_bytes(gzip.decompress((fixture_dir / "trajectory.dat.gz").read_bytes()))
        traj = trajectory.from_file(plain, top.strand_counts, is_5p_3p=False)
    return top, traj, read_order_parameters(fixture_dir / "op.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[384, 65535])
    ap.add_argument("--fixture", type=Path, default=ROOT / "tests" / "golden" / "melting_temp")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_order_params.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    top, traj, ops = load(args.fixture)
    sim, cfg = defaults.default_configs_for("dna1")
    flat = fp.pack_flat(fp.derive_flat(1, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=False), _lib.param_names())
    for dtype in (torch.float32, torch.float64):
        s = OxdnaSystem(1, top.seq, top.is_end, top.bonded_neighbors, box=np.full(3, 20.0), dtype=dtype, device=dev)
        s.set_params(flat)
        s.set_neighbors(top.unbonded_neighbors)
        for n_frames in args.frames:
            reps = -(-n_frames // traj.center.shape[0])
            c = torch.as_tensor(traj.center, dtype=dtype, device=dev).repeat(reps, 1, 1)[:n_frames].contiguous()
            q = torch.as_tensor(traj.quaternions, dtype=dtype, device=dev).repeat(reps, 1, 1)[:n_frames].contiguous()
            calls = {"order_params": lambda: s.order_params(c, q, ops), "energy": lambda: s.energy(c, q)[0]}
            wall = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for k in range((0 if args.once else args.warmup) + (1 if args.once else args.repeats)):
                for name, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = call()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if args.once or k >= args.warmup:
                        wall[name].append(1e3 * (t2 - t0))
                        host[name].append(1e3 * (t1 - t0))
                    del out
            line = {"dtype": str(dtype).split(".")[-1], "frames": n_frames, "nt": int(c.shape[1]), "pairs": sum(len(o.pairs) for o in ops),
                    "repeats": len(wall["energy"])}
            for name in calls:
                line[f"{name}_ms_median"] = round(statistics.median(wall[name]), 4)
                line[f"{name}_ms_min"] = round(min(wall[name]), 4)
                line[f"{name}_ms_max"] = round(max(wall[name]), 4)
                line[f"{name}_host_ms_median"] = round(statistics.median(host[name]), 4)
            line["energy_over_order_params"] = round(line["energy_ms_median"] / line["order_params_ms_median"], 3)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
