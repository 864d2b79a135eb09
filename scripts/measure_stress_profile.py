#!/usr/bin/env python3
"""dev: what the lateral pressure profile of stored MARTINI frames costs (mythos_martini_stress_profile,
csrc/stress_profile.hip).  A tool: it belongs to neither the benchmark nor the tests.

Shapes: ``--frames`` (200) stored fp32 frames of the 1 280-bead DMPC bilayer of tests/golden/martini (its ten frames,
repeated) and of bench.py's 4 x 4 tiling of it (20 480 beads, one frame repeated), ``--bins`` (100) slabs centred on the
tail ends, all four terms in one column.

The yardstick is ``MartiniSystem.energy(grads=True)`` on the same frames, the same system handle and the same build: the
same all-pairs tile sweep with less work per pair (no per-axis products, no double partials per bead).  Nobody had
measured either; the numbers are stated, not gated.  Times are device events around ``--batch`` back-to-back calls,
nothing read back (the profile's box check reads the boxes once per call: it is part of the call), after a warm-up; the
two paths alternate round by round in this one process, and the median and min ... max over ``--rounds`` are reported.
Prints one JSON line per shape; ``--out`` also writes them to a file.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from mythos_amd.hip_system import MartiniSystem  # noqa: E402
from tests import martini_helpers as MH  # noqa: E402


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def shape(name, frames, dev):
    """-> (system, pos (F, n, 3) fp32, box (F, 3) fp32, centre indices)"""
    s = MH.system()
    names = np.asarray(s["top"].atom_names)
    if name == "bilayer":
        x, box, _ = MH.frames("lj")
        reps = -(-frames // x.shape[0])
        x, box = np.tile(x, (reps, 1, 1))[:frames], np.tile(box, (reps, 1))[:frames]
        system = MartiniSystem(s["types"], s["sigma"], s["eps"], s["top"].bonded_neighbors, s["bond_k"], s["bond_r0"], s["top"].angles,
                               s["angle_k"], s["angle_t0"], dtype=torch.float32, device=dev)
    else:
        system, _, xt, bt = bench.martini_system(dev, torch.float32)
        x, box = np.broadcast_to(xt, (frames, *xt.shape)), np.broadcast_to(bt, (frames, 3))
        names = np.tile(names, 16)
    center = np.flatnonzero(np.isin(names, ["C3A", "C3B"])).astype(np.int32)
    return (system, torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev),
            torch.as_tensor(np.ascontiguousarray(box), dtype=torch.float32, device=dev), center)


def measure(name, args, dev):
    system, pos, box, center = shape(name, args.frames, dev)
    paths = {"stress_profile": lambda: system.stress_profile(pos, box, args.bins, center_index=center),
             "energy_grads": lambda: system.energy(pos, box, grads=True)}
    raw = paths["stress_profile"]()
    assert float(raw[:, :, 0].sum()) == args.frames * system.n and torch.isfinite(raw).all()
    for fn in paths.values():  # warm-up: code objects, the scratch buffers, the allocator's blocks
        event_ms(fn, 2)
    ms = {p: [] for p in paths}
    for _ in range(args.rounds):
        for p, fn in paths.items():
            ms[p].append(event_ms(fn, args.batch))
    out = dict(shape=name, beads=system.n, frames=args.frames, bins=args.bins, ms_per_call={p: stats(v) for p, v in ms.items()})
    out["profile_over_energy"] = out["ms_per_call"]["stress_profile"]["median"] / out["ms_per_call"]["energy_grads"]["median"]
    system.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bilayer,tiled")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3, help="back-to-back calls per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_stress_profile.py needs a GPU: it does not fall back")
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
