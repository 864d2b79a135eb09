"""DiffTRe end to end on the GPU (BASELINE configs[4] in miniature): simulate, reweight, differentiate, update.

 * the reweighted-observable gradient from the HIP dU/dtheta rows equals central finite differences of the
   reweighted mean on the same stored frames (no oracle needed: both sides are functions of stored frames);
 * DiffTReObjective follows the reference's protocol (objective.py:239-389): missing observables, n_eff threshold,
   max_valid_opt_steps, state hand-over;
 * SimpleOptimizer + Adam move the propeller twist of a 16-nt duplex towards its target over a few iterations.
"""

import math

import numpy as np
import pytest
import torch

from mythos_amd.energy import dna2
from mythos_amd.energy.base import Quaternion, RigidBody
from mythos_amd.observables import PropellerTwist
from mythos_amd.optimization import objective as O
from mythos_amd.optimization.optimization import Adam, SimpleOptimizer
from mythos_amd.simulators.hip_md import HipMDSimulator, StaticSimulatorParams
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0
OPT = {"eps_stack_base": 1.3523, "theta0_hb_4": math.pi}


def _setup(n_steps=3000, save_every=30):
    top, traj, _, _ = H.load_golden(2, "simple-helix")
    dev = torch.device("cuda", 0)
    from mythos_amd.energy.base import space

    disp, _ = space.periodic(traj.box_size)
    efn = dna2.create_default_energy_fn(topology=top, displacement_fn=disp)
    init = RigidBody(center=torch.as_tensor(traj.center[0], device=dev), orientation=Quaternion(vec=torch.as_tensor(traj.quaternions[0], device=dev)))
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5),
                               bonded_neighbors=top.bonded_neighbors, checkpoint_every=0, dt=0.005, kT=KT)
    sim = HipMDSimulator(name="md", energy_fn=efn, simulator_params=sp, save_every=save_every, dtype=torch.float64,
                         init_state=init, n_steps=n_steps, key=7)
    n = top.n_nucleotides
    pairs = np.stack([np.arange(n // 2), n - 1 - np.arange(n // 2)], axis=1)[1:-1]  # interior base pairs of the duplex
    return top, efn, sim, PropellerTwist(pairs)


def _loss_fn(ptwist, target):
    def fn(ref_states, weights, energy_fn, opt_params, observables):  # noqa: ARG001
        obs = ptwist(ref_states).to(weights.dtype)
        expected = (weights * obs).sum()
        return (expected - target) ** 2, (("propeller_twist", expected.detach()), {})

    return fn


def test_reweighted_gradient_equals_finite_differences():
    top, efn, sim, ptwist = _setup()
    out = sim.run(OPT)
    traj = out.observables[0]
    assert traj.length() == 100
    beta = 1.0 / KT
    ref_e = efn.with_params(OPT).map(traj).detach()
    loss_fn = _loss_fn(ptwist, 21.7)
    (loss, (neff, measured, _)), grads = O.compute_loss_and_grad(OPT, efn, beta, loss_fn, traj, ref_e, [traj])
    assert abs(float(neff) - 1.0) < 1e-12  # same parameters: uniform weights
    for name, h in (("eps_stack_base", 1e-5), ("theta0_hb_4", 1e-5)):
        vals = []
        for sgn in (+1, -1):
            pp = dict(OPT)
            pp[name] = OPT[name] + sgn * h
            lo, _ = O.compute_loss(pp, efn, beta, loss_fn, traj, ref_e, [traj])
            vals.append(float(lo))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(float(grads[name]) - fd) <= 1e-5 * max(1.0, abs(fd)), (name, float(grads[name]), fd)
    assert float(loss) > 0 and measured[0] == "propeller_twist"


def test_difftre_objective_protocol():
    top, efn, sim, ptwist = _setup(n_steps=1500, save_every=30)
    key = sim.exposes()[0]
    obj = O.DiffTReObjective(name="ptwist", required_observables=(key,), grad_or_loss_fn=_loss_fn(ptwist, 21.7),
                             energy_fn=efn, n_equilibration_steps=10, min_n_eff_factor=0.95, max_valid_opt_steps=3)
    first = obj.calculate({}, opt_params=OPT)
    assert not first.is_ready and first.needs_update == (key,)
    traj = sim.run(OPT).observables[0]
    ready = obj.calculate({key: traj}, opt_params=OPT)
    assert ready.is_ready and set(ready.grads) == set(OPT) and ready.state["opt_steps"] == 1
    assert abs(ready.observables["neff"] - 1.0) < 1e-12
    far = dict(OPT, eps_stack_base=OPT["eps_stack_base"] * 1.5)  # reweighting that far collapses n_eff
    stale = obj.calculate({key: traj}, opt_params=far, **ready.state)
    assert not stale.is_ready and stale.observables["neff"] < 0.95 and stale.state == {"opt_steps": 0}
    spent = obj.calculate({key: traj}, opt_params=OPT, opt_steps=3)
    assert not spent.is_ready and spent.needs_update == (key,)
    with pytest.raises(ValueError, match="no states"):
        O.DiffTReObjective(name="x", required_observables=(key,), grad_or_loss_fn=_loss_fn(ptwist, 21.7), energy_fn=efn,
                           n_equilibration_steps=10_000).calculate({key: traj}, opt_params=OPT)


def test_simple_optimizer_moves_the_observable_towards_the_target():
    top, efn, sim, ptwist = _setup(n_steps=4000, save_every=20)
    key = sim.exposes()[0]
    traj0 = sim.run(OPT).observables[0]
    start = float(ptwist(traj0.slice(slice(20, None, None))).mean())
    target = start + 1.0  # one degree away from where the default model sits
    obj = O.DiffTReObjective(name="ptwist", required_observables=(key,), grad_or_loss_fn=_loss_fn(ptwist, target),
                             energy_fn=efn, n_equilibration_steps=20, min_n_eff_factor=0.8, max_valid_opt_steps=5)
    opt = SimpleOptimizer(objective=obj, simulator=sim, optimizer=Adam(learning_rate=2e-3))
    losses = []

    def cb(optimizer_output, step):  # noqa: ARG001
        losses.append(float(optimizer_output.observables["ptwist"]["loss"]))
        return None, True

    out = opt.run(dict(OPT), n_steps=6, callback=cb)
    assert all(math.isfinite(x) for x in losses)
    assert set(out.opt_params) == set(OPT) and any(abs(float(out.opt_params[k]) - OPT[k]) > 1e-4 for k in OPT)
    # the reweighted estimate on a fixed trajectory is deterministic: within one trajectory's validity window the
    # loss decreases monotonically under a small Adam step
    assert losses[1] < losses[0]


def _run_ranks(extra, nproc=None):
    """scripts/difftre_ranks.py as child processes (never exec'ed from this GPU-holding process)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    script = str(root / "scripts" / "difftre_ranks.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if nproc is None:
        cmd = [sys.executable, script, *extra]
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), script, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, check=False)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def test_rank_sharded_difftre_equals_the_single_process_gradient():
    """BASELINE configs[4] through the multi-rank driver: 64 replicas of the 32 bp duplex; frames stay on their rank,
    4 + 2K doubles are all-reduced, and the gradient equals single-process autograd on the gathered frames (1e-10).
    One rank, then two ranks sharing this GPU over gloo (the driver's 8-GPU run uses RCCL on the same code path)."""
    one = _run_ranks(["--replicas", "64", "--steps", "600", "--save-every", "100", "--equilibration-frames", "2",
                      "--iterations", "2", "--check"])
    assert len(one) == 2 and one[0]["frames_total"] == 64 * 4 and one[0]["check"]["frames"] == 256
    assert one[0]["check"]["max_rel_grad_err"] <= 1e-10 and 0.0 < one[0]["neff"] <= 1.0 + 1e-12  # (equal weights: 1 up to rounding)
    assert any(abs(v) > 0 for v in one[0]["grads"].values())
    two = _run_ranks(["--replicas", "64", "--steps", "600", "--save-every", "100", "--equilibration-frames", "2",
                      "--iterations", "2", "--check", "--rehearse-on-one-gpu"], nproc=2)
    assert len(two) == 2 and two[0]["world"] == 2 and two[0]["replicas_this_rank"] == 32
    assert two[1]["check"]["max_rel_grad_err"] <= 1e-10 and two[0]["check"]["frames"] == 256


def test_bench_with_two_ranks_prints_one_line_of_the_contract():
    """`python bench.py --gpus 2` starts its own two ranks (torch.distributed.run on 127.0.0.1; here both on this GPU over
    gloo: --rehearse-on-one-gpu).  Exactly ONE JSON line comes out, from rank 0, with n_gpus 2, weak scaling, two replicas,
    strings short enough for the driver's parsed copy, every timed sample listed and the rebuild count of each."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--full", "--gpus", "2", "--rehearse-on-one-gpu", "--bp", "300", "--steps", "20",
                        "--warmup", "5", "--cpu-steps", "0", "--repeats", "3"], capture_output=True, text=True, env=env, timeout=900,
                       cwd=root, check=False)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["replicas"] == 2 and d["steps"] == 20 and d["warmup"] == 5
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["value"] > 0 and d["dtype"] == "f32"
    assert len(d["config"]["samples_ms"]) == 3 == len(d["config"]["scheduled_rebuilds_per_sample"])
    # value: all repeats over their total time (every list rebuild inside them counts); the median sample beside it
    total_ms = sum(d["config"]["samples_ms"])
    assert abs(d["ms_per_step"] - total_ms / (3 * 20)) < 1e-9
    assert d["value"] == pytest.approx(2 * 3 * 20 / (total_ms * 1e-3)) and d["steps_per_s_mean"] == d["value"]
    assert d["steps_per_s_median"] == pytest.approx(2 * 20 / (sorted(d["config"]["samples_ms"])[1] * 1e-3))
    assert "secondary" not in d  # (the other configs are single-GPU measurements)
    assert "rehearsal" in d["config"] and d["f64_steps_per_s"] > 0 and "f64" in d["config"]["timed_region"]
    for text in (d["config"]["workload"], d["config"]["timed_region"], d["metric"]):
        assert len(text) <= 120, text


def test_plain_bench_times_its_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    """`python bench.py` without --full: one sample of exactly --steps steps, no measurement beside the headline, and
    --dump-outputs writes the state after the last timed step: bitwise what one LangevinIntegrator.run of W + K steps
    from the same duplex, seed and list policy hands back (advance(a); advance(b) is advance(a + b), store closes the
    frame), from two processes whose clock ramps before the warm-up differ in length."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    from mythos_amd import _lib
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem
    from mythos_amd.input import defaults
    from mythos_amd.utils import generators

    root = Path(__file__).resolve().parent.parent
    lines = []
    for d, ramp_ms in (("a", "30"), ("b", "400")):
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--bp", "300", "--steps", "60", "--warmup", "10",
                            "--min-warmup-ms", ramp_ms, "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, cwd=root, check=False)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines.append([json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")])
    for ln in lines:
        assert len(ln) == 1
        d = ln[0]
        assert d["steps"] == 60 and d["warmup"] == 10 and d["dtype"] == "f32" and d["unit"] == "steps/s" and d["higher_is_better"] is True
        assert len(d["config"]["samples_ms"]) == 1 and d["config"]["full"] is False
        assert d["ms_per_step"] == pytest.approx(d["config"]["samples_ms"][0] / 60) and d["value"] == pytest.approx(1e3 / d["ms_per_step"])
        assert d["roofline"] is None and d["cpu_baseline"] is None and "secondary" not in d and "f64_steps_per_s" not in d
        assert "save_every_1" not in d["config"] and "f64" not in d["config"]
    assert lines[0][0]["config"]["warmup_steps_done"] < lines[1][0]["config"]["warmup_steps_done"]  # the ramps differ

    # the reference: the same system stepped W + K = 70 steps in one run (bench.py's defaults: dt 0.005, seed = rank 0,
    # skin 0.9, rebuild every 50, oxDNA2 with salt 0.5 and half-charged ends)
    sim, cfg = defaults.default_configs_for("dna2")
    kT = sim["kT"]
    top, c0, q0 = generators.ideal_duplex(300, model=2, seed=1234)
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=kT, salt_conc=sim["salt_conc"], half_charged_ends=True), _lib.param_names())
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=None, dtype=torch.float32, device="cuda:0")
    s.set_params(flat)
    integ = LangevinIntegrator(s, dt=0.005, kT=kT, gamma_t=kT / sim["diff_coef"], gamma_r=kT / sim["rot_diff_coef"],
                               mass=sim["nucleotide_mass"], inertia=sim["moment_of_inertia"], seed=0)
    integ.set_neighbor_policy(3.25, 0.9, 50)
    c = torch.as_tensor(c0, dtype=torch.float32, device="cuda:0").contiguous()
    q = torch.as_tensor(q0, dtype=torch.float32, device="cuda:0").contiguous()
    p, ang = integ.init_momenta()
    integ.run(c, q, p, ang, 70)
    ref = {"center": c, "quaternion": q, "momentum": p, "angular_momentum": ang}
    assert not np.array_equal(c.cpu().numpy(), c0.astype(np.float32))

    assert {f.stem for f in (tmp_path / "a").glob("*.npy")} == set(ref)
    for name, want in ref.items():
        want = want.cpu().numpy()
        for d in ("a", "b"):
            got = np.load(tmp_path / d / f"{name}.npy")
            assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
            np.testing.assert_array_equal(got, want, err_msg=f"{d}/{name}")
    integ.close()
    s.close()


def test_the_collectives_run_through_rccl_on_this_gpu():
    """The N > 1 path of bench.py and the DiffTRe driver is `torch.distributed` backend "nccl" = RCCL; the tests above
    share ONE GPU between two ranks and therefore use gloo (RCCL refuses two ranks on one device).  Here the same
    functions of mythos_amd/distributed.py issue their collectives through RCCL in a group of one on this GPU:
    library load, communicator set-up, all_gather_into_tensor, all_reduce and barrier execute on the device."""
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    code = """
import json, torch, torch.distributed as dist
from mythos_amd import distributed as md
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
rows = torch.arange(12, dtype=torch.float64, device="cuda").reshape(4, 3)
g = md.all_gather_observables(rows, n_total=4, force=True)
g2 = md.all_gather_observables(rows, force=True)
t = md.all_reduce_sum(torch.tensor([1.5, -2.0], dtype=torch.float64, device="cuda"), force=True)
dist.barrier(device_ids=[0])
torch.cuda.synchronize()
print(json.dumps({"backend": dist.get_backend(), "gather": bool(torch.equal(g, rows)), "gather_counts": bool(torch.equal(g2, rows)),
                  "reduce": t.tolist(), "own_storage": g.data_ptr() != rows.data_ptr()}))
dist.destroy_process_group()
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=root, check=False)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import json

    d = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][0]
    assert d == {"backend": "nccl", "gather": True, "gather_counts": True, "reduce": [1.5, -2.0], "own_storage": True}
