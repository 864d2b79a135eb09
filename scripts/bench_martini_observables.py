#!/usr/bin/env python3
"""dev: the MARTINI bond / angle Wasserstein path at the bilayer size - the golden membrane tiled 4 x 4 (20 480 beads,
2 048 DMPC), 200 frames stored by MartiniLangevinIntegrator.advance, all 15 names, 1e5 seeded reference samples each.

Times, alternating in one process, every phase ended by a device synchronise, each figure over at least 0.5 s:
  (a) a torch restatement on the same GPU of the reference's per-step algorithm (three sorts + cumsum per name,
      autograd backward; mythos/observables/wasserstein.py:42-78)
  (b) the plan build (sorts + plan kernel), once per trajectory
  (c) mythos_w1_eval, forward + gradient, per optimisation step
  (d) the geometry launch
and writes them with launch counts and the bytes each kernel must move (from shapes) to profiles/martini_w1.json.

``--membrane`` measures the membrane launch instead (mythos_membrane_eval: leaflets, thickness, area per lipid) at 1 280
beads and at the 16-fold tiled system, the same number of frames each: time per call by HIP events over back-to-back
calls, next to the same quantities composed from torch ops on the same device tensors (index_select, means, a
comparison, masked means - the yardstick, ``torch_membrane`` below), alternating, and writes
profiles/martini_membrane.json.  ``--kernel-stats CSV`` adds the rows of a rocprofv3 --kernel-trace --stats table of a
separate run of the same command (``--profile-run``: few repetitions, nothing written) to that file.
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
from mythos_amd.hip_system import MartiniLangevinIntegrator, MartiniSystem  # noqa: E402
from mythos_amd.input import gromacs  # noqa: E402
from mythos_amd.observables import AreaPerLipid, BondDistancesMapped, MembraneThickness, TripletAnglesMapped  # noqa: E402
from mythos_amd.observables.wasserstein import W1Plan  # noqa: E402
from mythos_amd.utils.generators import tiled_martini_box  # noqa: E402

MG = ROOT / "tests" / "golden" / "martini"
CHUNK = 2048


def system(dev, reps):
    top = gromacs.MartiniTopology.from_top(MG / "template" / "topol.top")
    lj = json.loads((MG / "m2" / "lj" / "ljconf.json").read_text())
    bead_types = sorted({t for k in lj for t in k.split("_")[2:4]})
    idx = {t: i for i, t in enumerate(bead_types)}
    table = lambda p: np.array([[lj.get(f"lj_{p}_{a}_{b}", lj.get(f"lj_{p}_{b}_{a}")) for b in bead_types] for a in bead_types])  # noqa: E731
    bp = json.loads((MG / "m2" / "bond" / "bond_params.json").read_text())
    ap = json.loads((MG / "m2" / "angle" / "angle_params.json").read_text())
    x, box, _ = gromacs.read_trr(MG / "m2" / "lj" / "test.trr")
    big, xt, bt = tiled_martini_box(top, x[3], box[3], reps)
    types = np.array([idx[t] for t in big.atom_types], dtype=np.int32)
    sysm = MartiniSystem(types, table("sigma"), table("epsilon"), big.bonded_neighbors,
                         np.array([bp["bond_k_" + n] for n in big.bond_names]), np.array([bp["bond_r0_" + n] for n in big.bond_names]),
                         big.angles, np.array([ap["angle_k_" + n] for n in big.angle_names]),
                         np.deg2rad(np.array([ap["angle_theta0_" + n] for n in big.angle_names])), dtype=torch.float32, device=dev)
    return big, sysm, xt, bt


def torch_reference_step(values, refs, weights):
    """(a): per name three sorts + cumsum, then backward to the frame weights."""
    w = weights.clone().requires_grad_(True)
    total = 0.0
    for u, v in zip(values, refs):
        m = u.shape[1]
        uw = torch.repeat_interleave(w, m) / m
        vw = torch.full(v.shape, 1.0 / v.numel(), dtype=torch.float64, device=v.device)
        uf = u.reshape(-1)
        ui, vi = torch.argsort(uf), torch.argsort(v)
        vals, wts = torch.cat([uf[ui], v[vi]]), torch.cat([uw[ui], -vw[vi]])
        si = torch.argsort(vals)
        vals, wts = vals[si], wts[si]
        total = total + torch.sum((vals[1:] - vals[:-1]) * torch.abs(torch.cumsum(wts, 0)[:-1]))
    (g,) = torch.autograd.grad(total, w)
    return total.detach(), g


def timed(fn, min_s=0.5):
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= min_s:
            return (time.perf_counter() - t0) / n, n


def torch_membrane(pos, box, sel, per_lipid, thick, thick_lipid):
    """The membrane launch's quantities from torch ops, for lipids of ``per_lipid`` selected beads each, stored together:
    (thickness, area per lipid, leaflets).  Eager torch: about a dozen kernels and their temporaries."""
    z = pos[:, :, 2].double()
    zs = z.index_select(1, sel)                                   # (S, n_sel)
    mid = zs.mean(1, keepdim=True)                                # over beads
    lipid_z = zs.view(zs.shape[0], -1, per_lipid).mean(2)         # (S, n_lipids)
    up = lipid_z > mid
    n_up = up.sum(1)
    zt, tu = z.index_select(1, thick), up.index_select(1, thick_lipid)
    z_up = (zt * tu).sum(1) / tu.sum(1)
    z_lo = (zt * ~tu).sum(1) / (~tu).sum(1)
    occupied = (n_up > 0).double() + (n_up < up.shape[1]).double()
    area = box[:, 0].double() * box[:, 1].double() * occupied / up.shape[1]
    return z_up - z_lo, area, torch.where(up, 1, -1).to(torch.int8)


def event_ms(fn, calls=None, window_ms=500.0):
    """Milliseconds per call between two HIP events around back-to-back calls: ``calls`` of them, or as many as fill
    ``window_ms`` (sized from a first batch of 50)."""
    def batch(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    fn()
    torch.cuda.synchronize()
    if calls is None:
        calls = max(50, int(window_ms / max(batch(50), 1e-4)))
    return batch(calls)


def stored_frames(dev, reps, n_frames):
    top, sysm, xt, bt = system(dev, reps)
    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=0.0083144626 * 310.0, gamma=1.0, seed=0)
    integ.set_neighbor_policy(0.4, 8)
    integ.load(torch.as_tensor(xt, dtype=torch.float32, device=dev).contiguous(), integ.init_velocities(), bt)
    integ.advance(200)
    frames, _ = integ.advance(n_frames * 10, save_every=10, want_energy=False)
    return top, frames, torch.as_tensor(bt, dtype=torch.float32, device=dev).expand(n_frames, 3).contiguous()


def membrane_main(args):
    dev = torch.device("cuda", 0)
    calls = 20 if args.profile_run else None
    result = {"frames": args.frames, "window_ms_per_sample": 500.0, "rounds": args.rounds, "sizes": {}}
    for reps in (1, args.reps):
        top, frames, boxes = stored_frames(dev, reps, args.frames)

        class Traj:
            center = frames
            box_size = boxes

        thick = MembraneThickness(topology=top, lipid_sel="name GL1 GL2", thickness_sel="name PO4")
        area = AreaPerLipid(topology=top, lipid_sel="name GL1 GL2")
        _, start, sel, tb, tl = thick.index_lists()
        assert np.all(np.diff(start) == 2)
        idx = [torch.as_tensor(a, dtype=torch.int64, device=dev) for a in (sel, tb, tl)]
        rows, leaf = thick.rows(Traj), thick.leaflets(Traj)
        t_ref, a_ref, l_ref = torch_membrane(frames, boxes, idx[0], 2, idx[1], idx[2])
        agree = {"thickness_max_abs_diff_nm": float((rows[:, 0] - t_ref).abs().max()), "area_max_rel_diff": float((rows[:, 1] / a_ref - 1).abs().max()),
                 "leaflets_equal": bool(torch.equal(leaf, l_ref)), "upper_leaflet_min_max": [int(rows[:, 3].min()), int(rows[:, 3].max())]}
        samples = {"hip_rows_ms": [], "hip_rows_and_leaflets_ms": [], "hip_area_only_ms": [], "torch_ms": []}
        for _ in range(1 if args.profile_run else args.rounds):  # alternate
            samples["torch_ms"].append(event_ms(lambda: torch_membrane(frames, boxes, idx[0], 2, idx[1], idx[2]), calls))
            samples["hip_rows_ms"].append(event_ms(lambda: thick.rows(Traj), calls))
            samples["hip_rows_and_leaflets_ms"].append(event_ms(lambda: thick.leaflets(Traj), calls))
            samples["hip_area_only_ms"].append(event_ms(lambda: area.rows(Traj), calls))
        n, n_lip = int(frames.shape[1]), len(start) - 1
        result["sizes"][str(n)] = {
            "beads": n, "lipids": n_lip, "median_ms_per_call": {k: float(np.median(v)) for k, v in samples.items()}, "all_ms_per_call": samples,
            "launches_per_call": {"hip": 1, "torch": "see the kernel-trace summary"},
            # per frame: the selection's z for the midpoint, again per lipid, the thickness beads' z and their lipids' z again
            "gathered_z_per_frame": 2 * len(sel) + len(tb) * 3, "agreement_with_torch": agree}
    if args.profile_run:
        print(json.dumps(result))
        return
    if args.kernel_stats:
        import csv
        with open(args.kernel_stats) as f:
            table = list(csv.DictReader(f))
        keep = [r for r in table if "membrane_kernel" in r["Name"]] + [r for r in table if "at::native" in r["Name"] or "rocprim" in r["Name"]][:12]
        result["rocprofv3_kernel_stats"] = {
            "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_martini_observables.py --membrane --profile-run",
            "rows": [{"name": r["Name"][:160], "calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": int(r["MinNs"]),
                      "max_ns": int(r["MaxNs"]), "total_ns": int(r["TotalDurationNs"])} for r in keep]}
    out = Path(args.out or ROOT / "profiles" / "martini_membrane.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--n-ref", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/martini_w1.json, or profiles/martini_membrane.json with --membrane")
    ap.add_argument("--membrane", action="store_true", help="measure the membrane launch instead (profiles/martini_membrane.json)")
    ap.add_argument("--profile-run", action="store_true", help="--membrane: a short run for rocprofv3, writes nothing")
    ap.add_argument("--kernel-stats", default=None, help="--membrane: a rocprofv3 kernel_stats.csv of a --profile-run to record")
    args = ap.parse_args()
    if args.membrane:
        return membrane_main(args)
    dev = torch.device("cuda", 0)
    top, sysm, xt, bt = system(dev, args.reps)
    integ = MartiniLangevinIntegrator(sysm, dt=0.02, kT=0.0083144626 * 310.0, gamma=1.0, seed=0)
    integ.set_neighbor_policy(0.4, 8)
    pos = torch.as_tensor(xt, dtype=torch.float32, device=dev).contiguous()
    integ.load(pos, integ.init_velocities(), bt)
    integ.advance(200)
    frames, _ = integ.advance(args.frames * 10, save_every=10, want_energy=False)

    class Traj:
        center = frames
        box_size = torch.as_tensor(bt, dtype=torch.float32, device=dev).expand(args.frames, 3).contiguous()

    bnames, anames = tuple(sorted(set(top.bond_names))), tuple(sorted(set(top.angle_names)))
    observables = [BondDistancesMapped(topology=top, bond_names=bnames), TripletAnglesMapped(topology=top, angle_names=anames)]
    packed = [o.packed(Traj) for o in observables]
    rng = np.random.default_rng(0)
    values, refs, plan_args = [], [], []
    for o, (block, s, members) in zip(observables, packed):
        per, at = [], 0
        for m in members:
            u = block[at:at + s * m].view(s, m)
            at += s * m
            per.append(torch.as_tensor(rng.normal(float(u.mean()), float(u.std()), size=args.n_ref), device=dev))
            values.append(u)
        refs += per
        plan_args.append((block, [s] * len(members), list(members), per, [None] * len(members)))
    wts = rng.uniform(0.5, 1.5, size=args.frames)
    weights = torch.as_tensor(wts / wts.sum(), device=dev)

    plans = [W1Plan(*a) for a in plan_args]

    def hip_step():
        return [p.eval(weights, True) for p in plans]

    def build():
        for p in [W1Plan(*a) for a in plan_args]:
            p.close()

    def geometry():
        return [o.packed(Traj) for o in observables]

    # the two paths agree before anything is timed
    w_ref, g_ref = torch_reference_step(values, refs, weights)
    out = hip_step()
    w_hip = sum(o[0].sum() for o in out)
    g_hip = sum(o[1].sum(0) for o in out)
    agree = {"w_abs_diff": float((w_hip - w_ref).abs()), "grad_max_abs_diff": float((g_hip - g_ref).abs().max())}

    rows = {"a_torch_step_s": [], "b_plan_build_s": [], "c_w1_eval_s": [], "d_geometry_s": []}
    for _ in range(args.rounds):  # alternate the phases
        rows["a_torch_step_s"].append(timed(lambda: torch_reference_step(values, refs, weights))[0])
        rows["c_w1_eval_s"].append(timed(hip_step)[0])
        rows["b_plan_build_s"].append(timed(build)[0])
        rows["d_geometry_s"].append(timed(geometry)[0])
    entries = sum(s * m + args.n_ref for (_, fr, mem, _, _) in plan_args for s, m in zip(fr, mem))
    padded = sum(-(-(s * m + args.n_ref) // CHUNK) * CHUNK for (_, fr, mem, _, _) in plan_args for s, m in zip(fr, mem))
    samples = sum(s * m for (_, fr, mem, _, _) in plan_args for s, m in zip(fr, mem))
    items = sum(sum(mem) for (_, _, mem, _, _) in plan_args)
    n_b, n_a = sum(packed[0][2]), sum(packed[1][2])
    result = {
        "size": {"beads": int(xt.shape[0]), "frames": args.frames, "names": len(values), "n_ref": args.n_ref,
                 "merged_entries": entries, "padded_entries": padded, "u_samples": samples},
        "median_s": {k: float(np.median(v)) for k, v in rows.items()}, "all_s": rows,
        "launches": {"c_w1_eval": 5 * len(plans), "d_geometry": len(observables), "b_plan_build_kernel": len(plans),
                     "b_plan_build_sorts": len(values)},
        "bytes_min": {"w1_chunk_sum": 8 * padded, "w1_scan": 24 * padded, "w1_suffix": 16 * padded, "w1_frame_sum": 12 * samples,
                      "w1_plan_kernel": 24 * padded + 4 * samples + 16 * entries,
                      "martini_obs": args.frames * (n_b * (2 * 12 + 8) + n_a * (3 * 12 + 8)) + 32 * items},
        "agreement_with_torch": agree,
    }
    result["bytes_min"]["c_w1_eval_total"] = sum(result["bytes_min"][k] for k in ("w1_chunk_sum", "w1_scan", "w1_suffix", "w1_frame_sum"))
    result["c_w1_eval_GBps"] = result["bytes_min"]["c_w1_eval_total"] / result["median_s"]["c_w1_eval_s"] / 1e9
    out = Path(args.out or ROOT / "profiles" / "martini_w1.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
