#!/usr/bin/env python3
"""dev: one melting-temperature evaluation WITH its gradient at T = 20 temperatures, ms per evaluation (host + device, the
window ends in a device synchronise; median of the repeats after warm-up), on two shapes:

  fixture   the umbrella-sampling run of tests/golden/melting_temp: 384 frames x 12 nt, oxDNA1, periodic box 20
  dna2      the oxDNA2 golden duplex (tests/golden/dna2/simple-helix, 100 frames x 16 nt) tiled to 1000 frames, with
            made-up bind states and weights (a timing, not physics)

--mode loop   the temperature sweep as T + 1 energy calls written with ``with_params(kt=...)`` / ``map`` only, and the
              reweighting algebra written out below: runs on any commit of the project, which is how the comparator is
              measured on the commit BEFORE ``map_kt`` existed (check that commit out next to this script and the fixture).
--mode fused  the same evaluation through ``map_kt`` (one energy launch, one Debye-Hueckel sweep launch).
--mode both   the two alternating in one process (spread; not the comparison against the earlier commit).

One JSON line per shape.  fp64 frames (what a reparameterisation uses).
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
from mythos_amd.energy import dna1, dna2  # noqa: E402
from mythos_amd.energy.base import Quaternion, RigidBody, space  # noqa: E402
from mythos_amd.input import topology, trajectory  # noqa: E402
from mythos_amd.utils.units import get_kt  # noqa: E402

KT_SIM = 0.10238333333333333


def ratios_to_tm(e0, et, kts, bind, weights):
    """mythos/observables/melting_temp.py:130-140, 40-56 on a (T, F) tensor (the shift of the exponent cancels in the ratio)."""
    expo = (e0 / KT_SIM)[None, :] - et / kts[:, None]
    counts = torch.exp(expo - expo.detach().max(dim=1, keepdim=True).values) / weights[None, :]
    unbound = torch.where((bind == 0)[None, :], counts, torch.zeros_like(counts)).sum(1)
    bound = torch.where((bind != 0)[None, :], counts, torch.zeros_like(counts)).sum(1)
    phi = bound / unbound
    finf = 1 + 1 / (2 * phi) - torch.sqrt((1 + 1 / (2 * phi)) ** 2 - 1)
    order = torch.argsort(finf.detach())
    xs, ys = finf[order], kts[order]
    i = int(torch.clamp(torch.searchsorted(xs.detach(), torch.tensor(0.5, dtype=xs.dtype, device=xs.device), right=True), 1, xs.shape[0] - 1))
    return ys[i - 1] + (0.5 - xs[i - 1]) / (xs[i] - xs[i - 1]) * (ys[i] - ys[i - 1])


def shapes(fixture_dir: Path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        top = topology.from_oxdna_file(fixture_dir / "sys.top")
        top2 = topology.from_oxdna_file(ROOT / "tests" / "golden" / "dna2" / "simple-helix" / "generated.top")
    with tempfile.TemporaryDirectory() as tmp:  # (the fixture keeps its trajectory compressed)
        plain = Path(tmp) / "trajectory.dat"
        plain.write_bytes(gzip.decompress((fixture_dir / "trajectory.dat.gz").read_bytes()))
        traj = trajectory.from_file(plain, top.strand_counts, is_5p_3p=False)
    rows = np.loadtxt(fixture_dir / "energy.dat", skiprows=1)  # time, U, three acceptance ratios, bond, mindistance, weight
    n = traj.center.shape[0]
    ef = dna1.create_default_energy_fn(top, space.periodic(20.0)[0]).with_params(kt=KT_SIM)
    yield ("fixture", ef, traj.center, traj.quaternions, rows[:n, 5], rows[:n, 7], ("eps_stack_base", "eps_stack_kt_coeff", "a_stack", "eps_hb"))
    traj2 = trajectory.from_file(ROOT / "tests" / "golden" / "dna2" / "simple-helix" / "output.dat", top2.strand_counts, is_5p_3p=False)
    c, q = np.tile(traj2.center, (10, 1, 1)), np.tile(traj2.quaternions, (10, 1, 1))
    bind = (np.arange(c.shape[0]) % 3 != 0).astype(np.float64)
    ef2 = dna2.create_default_energy_fn(top2, space.periodic(traj2.box_size)[0]).with_params(kt=KT_SIM)
    yield ("dna2", ef2, c, q, bind, np.ones(c.shape[0]), ("eps_stack_base", "eps_stack_kt_coeff", "a_stack", "eps_hb", "q_eff", "lambda_factor"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loop", "fused", "both"), default="both")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fixture", type=Path, default=ROOT / "tests" / "golden" / "melting_temp")
    ap.add_argument("--once", action="store_true", help="one evaluation of each mode and shape (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_melting.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    kts_np = np.asarray([get_kt(t) for t in np.linspace(280.0, 350.0, 20)])
    kts = torch.as_tensor(kts_np, device=dev)
    modes = ("loop", "fused") if args.mode == "both" else (args.mode,)
    for name, ef, c, q, bind, weights, names in shapes(args.fixture):
        body = RigidBody(center=torch.as_tensor(c, dtype=torch.float64, device=dev),
                         orientation=Quaternion(vec=torch.as_tensor(q, dtype=torch.float64, device=dev)))
        bind_d, w_d = torch.as_tensor(bind, device=dev), torch.as_tensor(weights, dtype=torch.float64, device=dev)
        values = {k: float(ef.params_dict()[k]) for k in names}

        def evaluate(mode):
            opt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in values.items()}
            fn = ef.with_params(opt)
            e0 = fn.map(body)
            if mode == "loop":
                et = torch.stack([fn.with_params(kt=float(k)).map(body) for k in kts_np])
            else:
                et = fn.map_kt(body, kts_np, sweep="fused")
            tm = ratios_to_tm(e0, et, kts, bind_d, w_d)
            grads = torch.autograd.grad(tm, list(opt.values()))
            torch.cuda.synchronize()
            return float(tm.detach()), [float(g) for g in grads]

        times = {m: [] for m in modes}
        result = {}
        for k in range((0 if args.once else args.warmup) + (1 if args.once else args.repeats)):
            for m in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                result[m] = evaluate(m)
                if args.once or k >= args.warmup:
                    times[m].append(1e3 * (time.perf_counter() - t0))
        line = {"shape": name, "frames": int(c.shape[0]), "nt": int(c.shape[1]), "temperatures": 20, "repeats": len(times[modes[0]])}
        for m in modes:
            line[f"{m}_ms_median"] = round(statistics.median(times[m]), 4)
            line[f"{m}_ms_min"] = round(min(times[m]), 4)
            line[f"{m}_tm"] = result[m][0]
        if len(modes) == 2:
            line["loop_over_fused"] = round(line["loop_ms_median"] / line["fused_ms_median"], 3)
            line["tm_difference"] = abs(result["loop"][0] - result["fused"][0])
            scale = max(abs(a) for a in result["loop"][1])
            line["grad_max_difference_over_largest"] = max(abs(a - b) for a, b in zip(*(result[m][1] for m in modes))) / scale
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
