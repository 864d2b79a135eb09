"""Conditions on the branch-pose fixtures (tests/golden/branch_poses, built by tests/oxdna_branch_poses.py), on the CPU
with the oracle alone: every reachable branch cell of every pair term holds live poses, the comparisons the GPU tests make
would notice a 1 % error in any one of them, and the exact-math CPU port of the pair templates agrees with the oracle
there (so a GPU failure on these poses is about the lean fp32 bodies or the launch, not the templates)."""

import subprocess

import numpy as np
import pytest
import torch

from oracle import cpu_port
from oracle import oxdna_oracle as orc
from tests import helpers as H
from tests import oxdna_branch_poses as BP


@pytest.fixture(scope="module")
def plain():
    """The plain oracle on the whole fixture of a model, computed once: energies, gradients, dU/dtheta, the step."""
    cache = {}

    def get(model):
        if model not in cache:
            poses = BP.load_fixture(model)
            cache[model] = {"poses": poses, "energy": BP.oracle_energy(poses), "params": BP.oracle_param_grads(poses),
                            "step": BP.oracle_step(poses), "table": BP.cell_table(poses), "eval": BP.evaluate(poses)}
        return cache[model]

    return get


def test_the_recorder_changes_nothing_and_puts_the_oracle_back():
    poses = BP.load_fixture(2)
    before = {name: getattr(orc, name) for name in (*BP._INTERVALS, *BP._PAIR_FUNCS)}
    e_rec, gc_rec, _ = BP.oracle_energy(poses)
    assert all(getattr(orc, name) is fn for name, fn in before.items())
    c = torch.as_tensor(poses.center)
    e = orc.energy_terms(2, BP.params(2), c, torch.as_tensor(poses.quat), *poses.tensors()).numpy()
    assert np.array_equal(e, e_rec)
    _, gc, _ = orc.energy_and_grads(2, BP.params(2), c, torch.as_tensor(poses.quat), *poses.tensors())
    assert np.array_equal(gc.numpy(), gc_rec)
    with pytest.raises(ZeroDivisionError):
        with BP.Recorder():
            1 / 0
    assert all(getattr(orc, name) is fn for name, fn in before.items())
    # a mutation scales the energy of the poses in that branch, and of no other
    cell = ("hydrogen_bonding", "f1#0", "low_tail")
    terms, masks, _ = BP.evaluate(poses)
    mutated, _, _ = BP.evaluate(poses, mutate=cell)
    hb, hb_m = terms["hydrogen_bonding"], mutated["hydrogen_bonding"]
    assert np.allclose(hb_m[masks[cell]], 1.01 * hb[masks[cell]], rtol=1e-12, atol=0) and np.array_equal(hb_m[~masks[cell]], hb[~masks[cell]])
    assert all(np.array_equal(mutated[k], terms[k]) for k in terms if k != "hydrogen_bonding")


@pytest.mark.parametrize("model", BP.MODELS)
def test_every_reachable_cell_holds_live_poses(model, plain):
    """Coverage: the committed poses, re-evaluated under the recorder, put at least K_LIVE live, eligible poses into every
    interval-reachable cell.  Exempt are the waived cells (no draw reached them; a tail, with a geometric reason) and the
    cells PROVEN_DEAD checks to be zero by construction.  One of those, oxRNA2 stacking f5#0 core, is a core branch: the rule
    that a core branch cannot be waived is relaxed for a cell a test shows to be identically zero, and only for such a cell.
    Waived, dead and fp32-blind cells together are at most 5 % of the reachable cells of a model."""
    poses = plain(model)["poses"]
    rows, text = plain(model)["table"]
    print(text)
    assert [c for c, _, _ in rows] == poses.cells  # the ids in the fixture name these cells
    waived = {c[1:] for c in BP.WAIVERS if c[0] == model}
    dead = {c[1:] for c in BP.PROVEN_DEAD if c[0] == model}
    reachable = {c for c, _, _ in rows}
    assert waived <= reachable and dead <= reachable and not (waived & dead)
    assert all(c[2] != "core" for c in waived), "a core branch cannot be waived"
    blind = {c[1:] for c in BP.FP32_BLIND if c[0] == model}  # (exempt from the fp32 leg of the sensitivity test only)
    assert blind <= reachable and len(waived) + len(dead) + len(blind) <= 0.05 * len(reachable)
    short = [(c, n) for c, n, _ in rows if n < BP.K_LIVE and c not in waived and c not in dead]
    assert not short, short
    print(f"model {model}: {len(reachable)} reachable cells, {len(waived)} waived, {len(dead)} proven dead, {poses.n} poses")
    # the aligned family is on the edge of the clamped acos: cosines of the shared axes within rounding of +-1
    al = poses.subset(np.nonzero(poses.cell < 0)[0])
    a1, _, a3 = (a.numpy() for a in orc.quat_to_axes(torch.as_tensor(al.quat / np.linalg.norm(al.quat, axis=1, keepdims=True))))
    on_edge = np.maximum(np.abs((a1[0::2] * a1[1::2]).sum(1)), np.abs((a3[0::2] * a3[1::2]).sum(1))) > 1.0 - 1e-6
    assert al.n >= 12 and on_edge.sum() >= 8


@pytest.mark.parametrize("model", BP.MODELS)
def test_cells_exempt_as_dead_are_zero_by_construction(model):
    """PROVEN_DEAD: wherever the argument of the named factor is in the named branch, another factor of the same product is
    zero.  Checked on 200 000 uniform directions of the backbone separation in the body frame, from the parameters."""
    for (m, term, factor, branch), check in BP.PROVEN_DEAD.items():
        if m == model:
            in_branch, other_factor = check(np.random.default_rng(0), 200_000)
            assert in_branch.sum() > 1000 and np.abs(other_factor[in_branch]).max() == 0.0, (term, factor, branch)


@pytest.mark.parametrize("model", BP.MODELS)
def test_a_one_percent_error_in_any_one_cell_fails_the_comparisons(model, plain):
    """Sensitivity: one branch of one factor scaled by 1.01 inside the recorder; the mutated oracle stands in for the
    kernel.  For every cell that is not exempt, the energy-kernel comparisons fail at the fp64 and at the fp32 tolerance, the
    dU/dtheta comparison fails, and the step comparisons fail at both tolerances.  (The mutation changes only the poses in
    that branch: those are re-evaluated, the rest of the set keeps the plain values.)"""
    ref = plain(model)
    poses = ref["poses"]
    e0, gc0, gq0 = ref["energy"]
    keys, pg0 = ref["params"]
    p0, L0, e1 = ref["step"]
    _, masks, _ = ref["eval"]
    exempt = {c[1:] for c in (*BP.WAIVERS, *BP.PROVEN_DEAD) if c[0] == model}
    blind = {c[1:] for c in BP.FP32_BLIND if c[0] == model}
    escaped = []
    for cell in poses.cells:
        if cell in exempt:
            continue
        idx = np.nonzero(masks[cell])[0]
        nuc = np.stack([2 * idx, 2 * idx + 1], 1).reshape(-1)
        sub = poses.subset(idx)

        def spliced(full, a, b, rows=nuc):
            out = full.copy()
            if rows is None:
                return out + (b - a)
            out[rows] += b - a
            return out

        (ea, gca, gqa), (eb, gcb, gqb) = BP.oracle_energy(sub), BP.oracle_energy(sub, mutate=cell)
        em, gcm, gqm = spliced(e0, ea, eb, None), spliced(gc0, gca, gcb), spliced(gq0, gqa, gqb)
        pgm = spliced(pg0, BP.oracle_param_grads(sub)[1], BP.oracle_param_grads(sub, mutate=cell)[1], None)
        (pa, La, e1a), (pb, Lb, e1b) = BP.oracle_step(sub), BP.oracle_step(sub, mutate=cell)
        pm, Lm, e1m = spliced(p0, pa, pb), spliced(L0, La, Lb), spliced(e1, e1a, e1b, None)
        caught = {
            "energy fp64": BP.compare_energies(poses, em, e0, "fp64") + BP.compare_gradients(poses, gcm, gqm, gc0, gq0, "fp64"),
            "energy fp32": BP.compare_energies(poses, em, e0, "fp32") + BP.compare_gradients(poses, gcm, gqm, gc0, gq0, "fp32"),
            "dU/dtheta": BP.compare_param_grads(keys, pgm, pg0),
            "step fp64": BP.compare_step(poses, pm, Lm, e1m, p0, L0, e1, "fp64"),
            "step fp32": BP.compare_step(poses, pm, Lm, e1m, p0, L0, e1, "fp32"),
        }
        for what, failures in caught.items():
            if not failures and not (cell in blind and what.endswith("fp32")):
                escaped.append((cell, what))
    assert not escaped, escaped


@pytest.mark.parametrize("cell", sorted(BP.FP32_BLIND))
def test_cells_exempt_from_the_fp32_sensitivity_cannot_be_shown_in_fp32(cell):
    """FP32_BLIND: on a fresh pool of 40 000 draws aimed at the cell, every eligible live pose in it has forces above 50 on
    both nucleotides (excluded volume) beside a coaxial term below 0.2, and a 1 % error in the cell moves no force or torque
    component by more than a tenth of the 1e-3 of its own size that the fp32 bound allows at the least - no selection of
    poses can make the fp32 comparison see it.  (fp64 and dU/dtheta see it: the sensitivity test holds them.)"""
    ratio, force, term = BP.fp32_blind_evidence(cell[0], cell[1:])
    print(f"{cell}: {len(ratio)} poses, largest ratio {ratio.max():.4f}, smallest force {force.min():.1f}, largest term {term.max():.4f}")
    assert len(ratio) >= 50
    assert ratio.max() < 0.1 and force.min() > 50.0 and term.max() < 0.2


@pytest.mark.parametrize("model", BP.MODELS)
def test_cpu_port_matches_the_oracle_on_the_branch_poses(model, plain):
    """oracle/cpu_port compiles the pair templates of the kernels with exact math: on the fixture it agrees with the oracle
    at the tolerance of tests/test_cpu_port.py::test_random_dimers_match_oracle (the quaternion gradient outside the aligned
    family, the body torque everywhere: on the clamp of acos the component along q is a matter of rounding)."""
    from tests.test_cpu_port import _flat

    if not cpu_port.LIB.exists():
        subprocess.run(["make", "-C", str(cpu_port.BUILD.parent)], check=True, capture_output=True)
    poses = plain(model)["poses"]
    e_ref, gc_ref, gq_ref = plain(model)["energy"]
    port = cpu_port.CpuPort(model, poses.seq.astype(np.int32), poses.is_end.astype(np.int32), poses.pairs(True), _flat(model, BP.HCE[model]), box=None)
    port.set_pairs(poses.pairs(False))
    e, gc, gq, tb = port.energy(poses.center, poses.quat)
    np.testing.assert_allclose(e[:8], e_ref, rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(gc, gc_ref, rtol=1e-9, atol=1e-9)
    free = np.repeat(poses.cell >= 0, 2)
    np.testing.assert_allclose(gq[free], gq_ref[free], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(BP.body_torque(poses.quat, gq), BP.body_torque(poses.quat, gq_ref), rtol=1e-9, atol=1e-9)
