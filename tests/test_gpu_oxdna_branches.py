"""The oxDNA energy kernel and the MD step kernel on the branch-pose fixtures (tests/golden/branch_poses): dimers that put live
poses into every reachable branch of f1 .. f6, the smoothed FENE and the Debye-Hueckel term - the smoothing tails the
trajectories the kernels are otherwise stepped on never visit, and which the fp32 step kernel evaluates with its own
branch-free bodies (MYTHOS_LEAN_MATH).  Reference: the oracle and its autograd.  The comparisons and their tolerances are those
of tests/oxdna_branch_poses.py; tests/test_oxdna_branch_poses_cpu.py shows that a 1 % error in any one cell fails them.

Dimers lie on a grid of 8 units; unbonded dimers come in through set_neighbors, bonded ones through the topology; the rows
are static.  A failure names the cells of the poses that are off, the worst pose, what was got and what was wanted."""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from tests import oxdna_branch_poses as BP

pytestmark = pytest.mark.gpu

DTYPE = {"fp64": torch.float64, "fp32": torch.float32}


@functools.lru_cache(maxsize=None)
def _reference(model):
    """The oracle on the fixture, once per model: energies and gradients, dU/dtheta, the frictionless step from rest."""
    poses = BP.load_fixture(model)
    return poses, BP.oracle_energy(poses), BP.oracle_param_grads(poses), BP.oracle_step(poses)


def _system(model, poses, dtype):
    from mythos_amd.hip_system import OxdnaSystem

    sim, cfg, leaves = BP.leaf_cfg(model)
    flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=BP.SALT[model], half_charged_ends=BP.HCE[model]), _lib.param_names())
    s = OxdnaSystem(model, poses.seq, poses.is_end, poses.pairs(True), box=None, dtype=dtype)
    s.set_params(flat.detach())
    s.set_neighbors(poses.pairs(False))
    return s, sim, flat, leaves


def _report(what, got, ref):
    print(f"{what}: largest difference {np.abs(got - ref).max():.3e}, largest reference {np.abs(ref).max():.3e}, rms {np.sqrt((ref ** 2).mean()):.3e}")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("model", BP.MODELS)
def test_energy_kernel_on_every_branch(model, precision):
    """The eight term energies, dU/dcentre and dU/dquat per nucleotide against oracle autograd (fp64 1e-9; fp32 1e-3 of a
    nucleotide's own largest component + the rms of the set, body torque only); fp64 also dU/dtheta of every leaf through the
    flat_params chain rule (1e-6 max(|ref|, 1e-3 max |ref|))."""
    poses, (e_ref, gc_ref, gq_ref), (keys, pg_ref), _ = _reference(model)
    dtype = DTYPE[precision]
    s, _, flat, leaves = _system(model, poses, dtype)
    c = torch.as_tensor(poses.center[None], dtype=dtype, device=s.device)
    q = torch.as_tensor(poses.quat[None], dtype=dtype, device=s.device)
    e, gc, gq, gflat = s.energy(c, q, grads=True, param_grads=precision == "fp64")
    e, gc, gq = e[0].cpu().numpy(), gc[0].double().cpu().numpy(), gq[0].double().cpu().numpy()
    _report("term energies", e, e_ref)
    _report("dU/dcentre", gc, gc_ref)
    _report("body torque", BP.body_torque(poses.quat, gq), BP.body_torque(poses.quat, gq_ref))
    failures = BP.compare_energies(poses, e, e_ref, precision) + BP.compare_gradients(poses, gc, gq, gc_ref, gq_ref, precision)
    if precision == "fp64":
        g = torch.autograd.grad(flat, [leaves[k] for k in keys], grad_outputs=gflat[0].cpu(), allow_unused=True)
        pg = np.array([0.0 if x is None else float(x) for x in g])
        _report("dU/dtheta", pg, pg_ref)
        assert np.count_nonzero(pg_ref) >= 60
        failures += BP.compare_param_grads(keys, pg, pg_ref)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("model", BP.MODELS)
def test_step_kernel_on_every_branch(model, precision, md_lanes):
    """One frictionless step from rest on the static rows, save_every=1: momenta and angular momenta per nucleotide against
    oracle forces and torques pushed through oracle/langevin_oracle.py's drift (fp64 1e-9 max(1, largest); fp32 1e-3 (own +
    rms)), and the eight columns of the energy-trace row against the oracle's term energies at its stepped state."""
    from mythos_amd.hip_system import LangevinIntegrator

    poses, _, _, (p_ref, L_ref, e_ref) = _reference(model)
    dtype = DTYPE[precision]
    s, sim, _, _ = _system(model, poses, dtype)
    integ = LangevinIntegrator(s, dt=BP.DT, kT=sim["kT"], gamma_t=0.0, gamma_r=0.0, mass=1.0, inertia=tuple(BP.INERTIA), seed=1)
    c = torch.as_tensor(poses.center, dtype=dtype, device=s.device).contiguous()
    q = torch.as_tensor(poses.quat, dtype=dtype, device=s.device).contiguous()
    p, L = torch.zeros_like(c), torch.zeros_like(c)
    _, _, et = integ.run(c, q, p, L, 1, save_every=1)
    p, L, e = p.double().cpu().numpy(), L.double().cpu().numpy(), et[0, :8].double().cpu().numpy()
    _report("momenta", p, p_ref)
    _report("angular momenta", L, L_ref)
    _report("energy-trace row", e, e_ref)
    failures = BP.compare_step(poses, p, L, e, p_ref, L_ref, e_ref, precision)
    assert not failures, "\n".join(failures)
