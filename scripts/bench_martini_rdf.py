#!/usr/bin/env python3
"""dev: the RDF launch (mythos_rdf_eval) against what a user composes from torch ops on the same GPU.

Shape: the ten golden bilayer frames (1 280 beads, DMPC, no solvent in the fixture) repeated to 512 frames, fp32
positions, two pairs of selections in one handle - the 768 tail beads against themselves and the 128 PO4 against the
tails - 200 bins below 2.0 nm.

The yardstick is a chunked torch composition in double: broadcast differences, minimum image, norm, then per frame
``bucketize`` + ``bincount`` of the admissible pairs inside r_max - producing the same int64 counts, asserted equal
before anything is timed.  Times: wall time per call with a device synchronise (what the user waits for, the launch's
flag read included), the median of ``--rounds`` samples after a warm-up, the two paths alternating; and the launch's own
time between two HIP events around back-to-back launches with nothing read back.  Writes profiles/martini_rdf.json.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mythos_amd import _lib  # noqa: E402
from mythos_amd.hip_system import martini_frames  # noqa: E402
from mythos_amd.input import gromacs  # noqa: E402
from mythos_amd.observables import RadialDistribution  # noqa: E402
from mythos_amd.observables.rdf import _RdfSet  # noqa: E402

MG = ROOT / "tests" / "golden" / "martini"
TAILS = "name C1A C2A C3A C1B C2B C3B"
PAIRS = {"tail-tail": (TAILS, TAILS), "PO4-tail": ("name PO4", TAILS)}


def torch_counts(pos, box, lists, n_bins, r_max, chunk):
    """(F, G, n_bins) int64 from eager torch: F |A| |B| doubles per chunk of frames, one bucketize + bincount per frame."""
    edges = torch.arange(1, n_bins, dtype=torch.float64, device=pos.device) * (r_max / n_bins)
    out = torch.zeros((pos.shape[0], len(lists), n_bins), dtype=torch.int64, device=pos.device)
    for g, (a, b) in enumerate(lists):
        ok = a[:, None] != b[None, :]
        for f0 in range(0, pos.shape[0], chunk):
            x, l = pos[f0:f0 + chunk].double(), box[f0:f0 + chunk].double()[:, None, None, :]
            d = x[:, a][:, :, None, :] - x[:, b][:, None, :, :]
            d = d - l * torch.round(d / l)
            r = torch.linalg.norm(d, dim=-1)
            hit = ok[None] & (r < r_max)
            for f in range(r.shape[0]):
                out[f0 + f, g] = torch.bincount(torch.bucketize(r[f][hit[f]], edges, right=True), minlength=n_bins)
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


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
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--r-max", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=16, help="frames per chunk of the torch composition")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    top = gromacs.MartiniTopology.from_top(MG / "template" / "topol.top")
    x, box, _ = gromacs.read_trr(MG / "m2" / "lj" / "test.trr")
    reps = -(-args.frames // x.shape[0])
    pos = torch.as_tensor(np.tile(x, (reps, 1, 1))[:args.frames], dtype=torch.float32, device=dev).contiguous()
    boxes = torch.as_tensor(np.tile(box, (reps, 1))[:args.frames], dtype=torch.float32, device=dev).contiguous()

    class Traj:
        center = pos
        box_size = boxes

    obs = RadialDistribution(topology=top, pairs=PAIRS, r_max=args.r_max, n_bins=args.bins)
    names, lists, block, n_pairs = obs.plan()
    tl = [(torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)) for a, b in lists]
    hip = obs.counts(Traj)
    ref = torch_counts(pos, boxes, tl, args.bins, args.r_max, args.torch_chunk)
    for g, name in enumerate(names):
        assert torch.equal(hip[name], ref[:, g]), name  # the same counts before anything is timed
    p, b = martini_frames(pos, boxes)
    rs = _RdfSet(int(p.shape[1]), lists, block, args.bins, args.r_max, "xyz", dev)

    samples = {"hip_call_ms": [], "torch_ms": [], "hip_launch_event_ms": []}
    wall_ms(lambda: obs.counts(Traj)), wall_ms(lambda: torch_counts(pos, boxes, tl, args.bins, args.r_max, args.torch_chunk))  # warm-up
    for _ in range(args.rounds):  # alternate
        samples["torch_ms"].append(wall_ms(lambda: torch_counts(pos, boxes, tl, args.bins, args.r_max, args.torch_chunk)))
        samples["hip_call_ms"].append(wall_ms(lambda: obs.counts(Traj)))
        samples["hip_launch_event_ms"].append(event_ms(lambda: rs.launch(p, b), 20))
    med = {k: float(np.median(v)) for k, v in samples.items()}
    ordered = args.frames * sum(n_pairs.values())
    # distances the kernel evaluates: a list against itself is walked once per unordered pair
    evaluated = args.frames * sum(len(a) * (len(a) - 1) // 2 if np.array_equal(a, bb) else len(a) * len(bb) for a, bb in lists)
    result = {
        "shape": {"beads": int(pos.shape[1]), "frames": args.frames, "dtype": "fp32", "n_bins": args.bins, "r_max": args.r_max,
                  "pairs": {k: [len(a), len(bb)] for k, (a, bb) in zip(names, lists)}, "counted_pairs": int(hip["tail-tail"].sum() + hip["PO4-tail"].sum())},
        "median_ms": med, "all_ms": samples, "torch_over_hip_call": med["torch_ms"] / med["hip_call_ms"],
        "ordered_pairs_per_call": ordered, "distances_evaluated_per_call": evaluated,
        "ordered_pairs_per_s_kernel": ordered / (1e-3 * med["hip_launch_event_ms"]),
        "distances_per_s_kernel": evaluated / (1e-3 * med["hip_launch_event_ms"]),
        "library": _lib.load().mythos_version().decode(),
    }
    out = Path(args.out or ROOT / "profiles" / "martini_rdf.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
