"""The oxDNA energy kernel and the Debye-Hueckel sweep on the paths no golden fixture reaches (tests/oxdna_energy_shapes.py
has the systems, tests/test_oxdna_energy_shapes_cpu.py what is assumed about them): rows walked in segments, calls cut
into frame and temperature chunks, and the minimum image with pairs that need one - each against the fp64 CPU oracle.

A. Segmented walk (``gather_row<SEGMENTED>``, reached on 16 - 120 nt through the ``energy_list_cap`` hook, put back to 0
   in a ``finally``): the golden helices of oxDNA1, oxDNA2, oxRNA2, oxNA and the ring, in the middle of their box and
   across three faces of it, three frames, fp64 and fp32, caps 8 / interior - 4 / end - 4 / 0 from the row lengths, four
   calls each - energies, + forces, + dU/dtheta, + dU/d(distribution) where the model has one (soft distribution).
   Against the oracle under the bounds of tests/test_gpu_oxdna_energy.py (terms: fp64 rtol 1e-9 + 1e-11 per nucleotide,
   fp32 1e-3 of sum|terms|; forces 1e-5 / 1e-3 of the largest component; dU/dtheta fp64 1e-5 of max(|ref|, 1e-3 max|ref|))
   and tests/test_gpu_pseq.py (distribution: 1e-9 max(1, max|ref|), fp32 2e-3 max|ref|); fp32 dU/dtheta, which no earlier
   test compares with the oracle, under the fp32 bound of the forces, 1e-3 of the largest component.  Every segmented
   result against the unsegmented one of the same call (1e-11 max(1, max|a|) in fp64, 2e-5 of that in fp32: the bound
   of the 1 000-nt test), and two calls with the same cap bit for bit.  The 120-nt duplex (stride 128, four workgroups,
   the last partial, fifteen segments at cap 8) with forces and dU/dtheta, two frames.
B. Chunks.  Synthetic frames (golden frame k mod 100 + noise seeded with k // 100), F = chunk + 70: energies, forces,
   dU/dtheta, dU/d(distribution) and the rows of an ObservableSet on 16 nt (the grid cuts at 65 535 frames), dU/dtheta on
   120 nt (256 MiB of partials cut near 32 000).  Eight frames around the boundary against the oracle; three slices of
   the frames as calls of their own must reproduce the whole call bit for bit.  The sweep: 129 temperatures (two passes)
   x 10 992 frames (64 MiB of partials cut at 10 922) with the gradients of the constants, mid-box and crossing: the
   Debye term of seven temperatures on the boundary frames against the oracle initialised at each, the row of the
   system's own kT against the energy kernel's Debye column and DH_* partials on every frame, slices along both axes
   bit for bit; ``map_kt`` fused at 129 temperatures on three crossing frames against the loop and the oracle.

Measured on an MI355X (worst over the cases; the bound in brackets):
   A, against the oracle   terms: fp64 5.2e-5 of the bound [1], fp32 9.6e-7 of sum|terms| [1e-3]   (120 nt: 1.8e-5, 1.6e-7)
                           forces, dU/dq: fp64 1.5e-13 [1e-5], fp32 7.4e-5 [1e-3]   (120 nt: 1.4e-13, 2.2e-5)
                           dU/dtheta: fp64 1.6e-12 [1e-5], fp32 2.1e-5 [1e-3]   (120 nt fp64: 1.0e-13)
                           dU/d(distribution): fp64 1.7e-14 [1e-9]
   A, segmented - unsegmented   fp64 2.6e-16 [1e-11], fp32 1.0e-7 [2e-5]   (120 nt: 2.5e-16, 1.5e-7); same cap twice: bitwise
   B, against the oracle   terms fp64 1.2e-4 of the bound, fp32 2.0e-6; forces fp64 1.4e-13, fp32 5.4e-4; dU/dtheta fp64 8.3e-13,
                           fp32 5.1e-6; sweep rows fp64 8.0e-7 of the bound; map_kt fp64 1.5e-15 of sum|terms|
   B, sweep row of the own kT - energy kernel: 5.4e-16 relative in fp64 [1e-12], 4.3e-8 in fp32 [2e-6]
   B, every slice comparison (frames, temperatures): bitwise
   the file: 36 cases in 8.3 s, the slowest 1.3 s (the first oracle).
Four libraries with one line changed each - a segment one entry short, the centre filter without the minimum image, the
centres of a chunk without its frame offset, the sweep's reduce without its frame offset - each turned part of this file red
(22, 14, 8 and 4 cases), the last two no earlier test.
"""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults
from mythos_amd.input import sequence_constraints as scm
from tests import helpers as H
from tests import melting_ref as M
from tests import oxdna_energy_shapes as E
from tests import oxdna_periodic_synth as S

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
SYSTEM_IDS = [E.system_id(m, n) for m, n in E.SYSTEMS]
WORST = {}  # figure -> worst value seen, printed by every test that adds to it


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    return value


def _report(prefix):
    for k in sorted(WORST):
        if k.startswith(prefix):
            print(f"worst {k}: {WORST[k]:.2e}")


# ---- the library side ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat(model, name):
    """(flat parameter vector with its graph, leaves in the oracle's key order + kT)."""
    sim, cfg, leaves = E.leaf_cfg(model)
    kt = torch.tensor(sim["kT"], dtype=torch.float64, requires_grad=True)
    if model == 4:
        flat = fp.pack_flat_na1(fp.derive_flat_na1(cfg["dna"], cfg["rna"], cfg["drh"], kt=kt, salt_conc=S.SALT[4], half_charged_ends=False), _lib.param_names())
    else:
        flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=kt, salt_conc=S.SALT[model], half_charged_ends=E.half_charged_ends(name)), _lib.param_names())
    return flat, [*leaves.values(), kt]


def _system(model, name, top, box, dtype):
    from mythos_amd.hip_system import OxdnaSystem

    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype, is_rna=S.is_rna(top) if model == 4 else None)
    s.set_params(_flat(model, name)[0].detach())
    pairs = E.pair_list(top)
    s.set_neighbors(pairs)
    _, lens = E.rows_of(top, pairs)
    assert s.neighbor_stats()[0] == lens.max() - E.BONDED_SLOTS
    return s, lens


def _device(a, s):
    return torch.as_tensor(a, dtype=s.dtype, device=s.device)


def _soft(s, model, n, on=True):
    if on:
        s.set_pseq(*scm.kernel_tables(E.soft_distribution(n), E.constraints(n)), 2 if model == 4 else 3)
    else:
        s.set_pseq()


def _call(s, c, q, kind, model):
    """The outputs of one of the four calls, as a dict of tensors."""
    if kind == "energy":
        return {"e": s.energy(c, q)[0]}
    if kind == "grads":
        e, gc, gq, _ = s.energy(c, q, grads=True)
        return {"e": e, "gc": gc, "gq": gq}
    if kind == "both":
        e, gc, gq, gp = s.energy(c, q, grads=True, param_grads=True)
        return {"e": e, "gc": gc, "gq": gq, "gp": gp}
    if kind == "param":
        e, _, _, gp = s.energy(c, q, param_grads=True)
        return {"e": e, "gp": gp}
    _soft(s, model, s.n)
    try:
        e, _, _, gp, gm, gb = s.energy(c, q, param_grads=True, pseq_grads=True)
    finally:
        _soft(s, model, s.n, on=False)
    return {"e": e, "gp": gp, "gm": gm, "gb": gb}


def _kinds(model):
    return ("energy", "grads", "param") + (("pseq",) if model in E.PSEQ_MODELS else ())


# ---- comparisons with the oracle ---------------------------------------------------------------------------------------------
def _check_terms(e, ref, n, dtype, tag):
    e = e.cpu().numpy()
    if dtype == torch.float64:  # test_fp64_terms_match_oracle_and_golden: per nucleotide rtol 1e-9, atol 1e-11
        _note(f"{tag} terms fp64 (fraction of the bound)", (np.abs(e - ref) / (1e-9 * np.abs(ref) + 1e-11 * n)).max())
        np.testing.assert_allclose(e / n, ref / n, rtol=1e-9, atol=1e-11)
    else:  # test_fp32_terms_within_1e3
        tot = np.abs(ref).sum(-1, keepdims=True)
        assert _note(f"{tag} terms fp32 (of sum|terms|)", (np.abs(e - ref) / tot).max()) < 1e-3
        np.testing.assert_allclose(e.sum(-1), ref.sum(-1), rtol=1e-3)


def _check_forces(out, ref, frames, dtype, tag):
    tol = 1e-5 if dtype == torch.float64 else 1e-3  # test_forces_and_quaternion_gradients
    prec = "fp64" if dtype == torch.float64 else "fp32"
    for k, f in enumerate(frames):
        u = ref["terms"][f].sum()
        assert abs(out["e"][k].sum().item() - u) <= tol * abs(u)
        for key in ("gc", "gq"):
            want = ref[key][f]
            err = np.abs(out[key][k].double().cpu().numpy() - want).max() / np.abs(want).max()
            assert _note(f"{tag} forces {prec} (of the largest component)", err) <= tol, (key, f, err)


def _check_dtheta(gp, ref, frames, model, name, dtype, tag):
    flat, leaves = _flat(model, name)
    for k, f in enumerate(frames):
        g = torch.autograd.grad(flat, leaves, grad_outputs=gp[k].cpu(), retain_graph=True, allow_unused=True)
        got = np.array([0.0 if x is None else float(x) for x in g])
        want = ref["dtheta"][f]
        scale = np.abs(want).max()
        assert np.count_nonzero(want) >= 15  # the comparison is not vacuous
        if dtype == torch.float64:  # test_parameter_gradients_chain_rule
            floor = np.maximum(np.abs(want), 1e-3 * scale)
            _note(f"{tag} dU/dtheta fp64 (of max(|ref|, 1e-3 max|ref|))", (np.abs(got - want) / floor).max())
            bad = np.abs(got - want) > 1e-5 * floor
        else:  # no earlier test holds the fp32 partials against the oracle: the fp32 bound of the forces, on the largest component
            _note(f"{tag} dU/dtheta fp32 (of the largest component)", np.abs(got - want).max() / scale)
            bad = np.abs(got - want) > 1e-3 * scale
        assert not bad.any(), [(ref["keys"][i], got[i], want[i]) for i in np.nonzero(bad)[0]]


def _check_pseq(out, ref, frames, n, dtype, tag):
    sc = E.constraints(n)
    up, bp = (torch.tensor(a, requires_grad=True) for a in E.soft_distribution(n))
    marg, bp_rows = scm.kernel_tables_torch((up, bp), sc)
    for k, f in enumerate(frames):
        g = torch.autograd.grad((marg, bp_rows), (up, bp), grad_outputs=(out["gm"][k].cpu(), out["gb"][k].cpu()), retain_graph=True)
        for got, want in zip(g, (ref["g_up"][f], ref["g_bp"][f])):
            top = np.abs(want).max()
            assert top > 1e-3
            err = np.abs(got.numpy() - want).max()
            if dtype == torch.float64:  # test_gradient_with_respect_to_the_distribution
                assert _note(f"{tag} dU/d(distribution) fp64 (of max(1, max|ref|))", err / max(1.0, top)) <= 1e-9
            else:
                assert _note(f"{tag} dU/d(distribution) fp32 (of max|ref|)", err / top) <= 2e-3


def _check_call(kind, out, ref, frames, model, name, n, dtype, tag):
    """One call's outputs for the frames ``frames`` of the oracle's."""
    idx = list(frames)
    _check_terms(out["e"], ref["soft_terms" if kind == "pseq" else "terms"][idx], n, dtype, tag)
    if "gc" in out:
        _check_forces(out, ref, frames, dtype, tag)
    if kind in ("param", "both"):
        _check_dtheta(out["gp"], ref, frames, model, name, dtype, tag)
    if kind == "pseq":
        _check_pseq(out, ref, frames, n, dtype, tag)


def _check_segmented(seg, plain, dtype, tag):
    tol = 1e-11 if dtype == torch.float64 else 2e-5  # test_reference_all_pairs_list_of_a_1000_nt_system_goes_through_the_energy_kernel
    for key, a in plain.items():
        scale = max(1.0, float(a.abs().max()))
        err = float((seg[key].double() - a.double()).abs().max()) / scale
        assert _note(f"{tag} segmented - unsegmented {'fp64' if dtype == torch.float64 else 'fp32'}", err) <= tol, (key, err)


def _with_cap(cap, fn):
    _lib.debug_set("energy_list_cap", cap)
    try:
        assert _lib.debug_get("energy_list_cap") == cap
        return fn()
    finally:
        _lib.debug_set("energy_list_cap", 0)


# ---- A. the segmented walk ---------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("place", E.PLACES)
@pytest.mark.parametrize(("model", "name"), E.SYSTEMS, ids=SYSTEM_IDS)
def test_segmented_row_walk_against_the_oracle(model, name, place, dtype):
    top, c0, q0, box = E.system_frames(model, name, place)
    n = int(top.n_nucleotides)
    ref = E.oracle(model, name, place)
    s, lens = _system(model, name, top, box, dtype)
    c, q = _device(c0, s), _device(q0, s)
    caps = E.caps(lens)
    assert caps[-1] == 0 and len(caps) == 4
    frames = range(len(E.FRAMES))
    results = {}
    for cap in caps:
        results[cap] = _with_cap(cap, lambda: {kind: _call(s, c, q, kind, model) for kind in _kinds(model)})
        if cap:  # the same cap again: the PARK atomics and the parameter-partial copies add in a fixed order
            again = _with_cap(cap, lambda: {kind: _call(s, c, q, kind, model) for kind in _kinds(model)})
            for kind, out in again.items():
                for key, a in out.items():
                    assert torch.equal(a, results[cap][kind][key]), (cap, kind, key)
    assert _lib.debug_get("energy_list_cap") == 0
    for cap in caps:
        for kind, out in results[cap].items():
            _check_call(kind, out, ref, frames, model, name, n, dtype, "A")
            if cap:
                _check_segmented(out, results[0][kind], dtype, "A")
    _report("A ")


@DTYPES
def test_segmented_walk_of_a_120_nt_row_in_four_workgroups(dtype):
    """Rows of 117 / 118 entries in a stride of 128: fifteen segments at cap 8, one full segment (interior rows) or a full
    one and a single entry (end rows) at cap 117; 120 nt are four workgroups, the last with 24 of 32 places; the second
    frame is the first translated (blockIdx.y > 0; the oracle evaluates both)."""
    model, name = 2, E.LONG
    top, c0, q0, box = E.system_frames(model, name, "mid")
    n = int(top.n_nucleotides)
    assert n == 120 and -(-n // E.TILE) == 4 and n % E.TILE != 0
    ref = E.oracle(model, name, "mid")
    assert np.abs(ref["terms"][1] - ref["terms"][0]).max() < 1e-10  # a translation
    s, lens = _system(model, name, top, box, dtype)
    c, q = _device(c0, s), _device(q0, s)
    caps = E.long_caps(lens)
    assert caps == (8, 117) and len(E.segments(int(lens.max()), 8)) == 15
    plain = _call(s, c, q, "both", model)
    _check_call("both", plain, ref, range(2), model, name, n, dtype, "A 120 nt")
    for cap in caps:
        out = _with_cap(cap, lambda: _call(s, c, q, "both", model))
        again = _with_cap(cap, lambda: _call(s, c, q, "both", model))
        assert all(torch.equal(out[k], again[k]) for k in out)
        _check_call("both", out, ref, range(2), model, name, n, dtype, "A 120 nt")
        _check_segmented(out, plain, dtype, "A 120 nt")
    _report("A 120 nt")


# ---- B. frame chunks ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames16():
    """The synthetic frames of the 16-nt oxDNA2 helix for the calls the grid cuts, built once."""
    top, c, q, box = E.synthetic_frames(2, "simple-helix", "mid", E.GRID_Y + E.TAIL)
    return top, c, q, box


def _observable_set(s, box):
    from mythos_amd.observables import get_duplex_quartets
    from mythos_amd.observables import base as PB

    _, cfg = defaults.default_configs_for("dna2")
    bp = s.n // 2
    pairs = np.stack([np.arange(bp), 2 * bp - 1 - np.arange(bp)], axis=1)[1:-1]
    return PB.ObservableSet(s.n, 2, cfg["geometry"], box, pairs, get_duplex_quartets(bp), True, s.dtype, s.device)


CHUNK_CASES = [  # kind, nucleotides, dtype
    ("energy", 16, torch.float64), ("energy", 16, torch.float32), ("grads", 16, torch.float64), ("grads", 16, torch.float32),
    ("param", 16, torch.float64), ("param", 120, torch.float32), ("pseq", 16, torch.float64), ("obs", 16, torch.float64),
]


@pytest.mark.parametrize(("kind", "n", "dtype"), CHUNK_CASES, ids=[f"{k}-{n}nt-{'fp64' if d == torch.float64 else 'fp32'}" for k, n, d in CHUNK_CASES])
def test_frame_chunks_of_an_energy_call(kind, n, dtype):
    model, name = 2, ("simple-helix" if n == 16 else E.LONG)
    chunk = E.energy_chunk(n, kind in ("param", "pseq"))
    n_frames = chunk + E.TAIL
    assert n_frames > chunk == (E.GRID_Y if n == 16 else E.ENERGY_SCRATCH // (4 * E.param_count() * 8))  # the premise: a second, short chunk
    if n == 16:
        top, c0, q0, box = _frames16()
        assert c0.shape[0] == n_frames
    else:
        top, c0, q0, box = E.synthetic_frames(model, name, "mid", n_frames)
    s, _ = _system(model, name, top, box, dtype)
    c, q = _device(c0, s), _device(q0, s)
    del c0, q0
    oset = _observable_set(s, box) if kind == "obs" else None

    def call(cc, qq):
        if kind != "obs":
            return _call(s, cc, qq, kind, model)
        e, _, _, _, rows = s.energy(cc, qq, observables=oset)
        return {"e": e, "rows": rows}

    whole = call(c, q)
    assert all(int(a.shape[0]) == n_frames for a in whole.values())
    # a frame's result does not depend on the chunk it is in, and the partial sums are added in a fixed order
    for sl in E.slices(chunk, n_frames):
        part = call(c[sl].contiguous(), q[sl].contiguous())
        for key, a in part.items():
            assert torch.equal(a, whole[key][sl]), (kind, key, sl, float((a.double() - whole[key][sl].double()).abs().max()))
    if kind == "obs":
        assert torch.equal(whole["rows"], oset.eval(c, q)) and float(whole["rows"][chunk:].abs().max()) > 1e-3
    seen = E.boundary_frames(chunk, n_frames)
    ref = E.oracle(model, name, "mid", frames=seen)
    idx = torch.as_tensor(seen, device=s.device)
    out = {key: a[idx] for key, a in whole.items()}
    _check_call("energy" if kind == "obs" else kind, out, ref, range(len(seen)), model, name, n, dtype, "B")
    assert np.ptp(ref["terms"].sum(1)) > 1e-2  # the frames differ
    _report("B ")


# ---- B. the Debye-Hueckel sweep ----------------------------------------------------------------------------------------------
def _own_kt():
    return defaults.default_configs_for("dna2")[0]["kT"]


@functools.lru_cache(maxsize=None)
def _sweep_oracle(place, frames, temps):
    """(T, F, 8) oracle terms of the synthetic 16-nt frames ``frames`` at the temperatures ``temps`` of the table."""
    top, c, q, box = E.synthetic_frames(2, "simple-helix", place, np.asarray(frames))
    _, cfg, _ = M.oracle_cfg(2)
    kts = E.sweep_kts(_own_kt())[list(temps)]
    out = M.oracle_sweep(2, cfg, top, c, q, kts, box=box, salt=S.SALT[2], hce=False, terms=True).numpy()
    out.setflags(write=False)
    return out


@DTYPES
@pytest.mark.parametrize("place", E.PLACES)
def test_temperature_and_frame_chunks_of_the_debye_sweep(place, dtype):
    from mythos_amd.hip_system import OxdnaSystem

    kts = E.sweep_kts(_own_kt())
    chunk = E.sweep_chunk(16, len(kts), True)
    n_frames = chunk + E.TAIL
    assert len(kts) == E.SWEEP_MAX_T + 1 and 10000 < chunk < 12000 and n_frames > chunk  # the premise: 128 + 1 temperatures, two frame chunks
    top, c0, q0, box = E.synthetic_frames(2, "simple-helix", place, n_frames)
    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=S.SALT[2], half_charged_ends=False), _lib.param_names())
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype)
    s.set_params(flat)
    s.set_neighbors(E.pair_list(top))
    c, q = _device(c0, s), _device(q0, s)
    _, table = fp.kt_sweep_tables(2, cfg, kts, kt=sim["kT"], salt_conc=S.SALT[2])
    assert table.shape == (129, 5) and table[:128, 3].argmax() == 126
    e_dh, de = s.debye_sweep(c, q, table, const_grads=True)
    assert e_dh.shape == (129, n_frames) and de.shape == (129, n_frames, 5)
    e2, de2 = s.debye_sweep(c, q, table, const_grads=True)
    assert torch.equal(e2, e_dh) and torch.equal(de2, de)
    assert (e_dh[127] == 0).all() and (de[127] == 0).all() and (e_dh[128] > 0).all() and (e_dh[:127] > 0).all()
    # the oracle initialised at seven temperatures of both passes, on the frames around the boundary
    seen, temps = E.boundary_frames(chunk, n_frames), E.SWEEP_T_ORACLE
    ref = _sweep_oracle(place, seen, temps)
    got = e_dh[list(temps)][:, list(seen)].cpu().numpy()
    if dtype == torch.float64:
        bound = 1e-9 * np.abs(ref[..., 7]) + 1e-11 * 16
        _note("B sweep fp64 (fraction of the bound)", (np.abs(got - ref[..., 7]) / bound).max())
    else:
        bound = 1e-3 * np.abs(ref).sum(-1)
        _note("B sweep fp32 (of sum|terms|)", (np.abs(got - ref[..., 7]) / np.abs(ref).sum(-1)).max())
    assert (np.abs(got - ref[..., 7]) <= bound).all(), np.abs(got - ref[..., 7]).max()
    assert np.abs(ref[0, :, 7]).min() > 1e-2 and np.abs(ref[-1, :, 7]).min() > 1e-2 and np.abs(ref[5, :, 7]).max() == 0.0
    # the row at the system's own constants is the Debye column of the energy call, its partials the DH_* columns of dU/dparams - on every frame
    e, _, _, gp = s.energy(c, q, param_grads=True)
    rtol = 1e-12 if dtype == torch.float64 else 2e-6  # (test_sweep_kernel_rows_against_the_energy_kernel)
    _note(f"B sweep row - energy kernel {'fp64' if dtype == torch.float64 else 'fp32'} (relative)", ((e_dh[0] - e[:, 7]).abs() / e[:, 7].abs()).max())
    torch.testing.assert_close(e_dh[0], e[:, 7], rtol=rtol, atol=0)
    cols = [_lib.param_names().index(k) for k in fp.DEBYE_KT_NAMES]
    torch.testing.assert_close(de[0], gp[:, cols], rtol=rtol * 10, atol=rtol * float(gp[:, cols].abs().max()))
    # slices along the frames, and along the temperatures (each holding the widest cut-off of its pass, so that the packed pair list
    # is the whole call's: tests/oxdna_energy_shapes.py), reproduce the whole call bit for bit
    for sl in E.slices(chunk, n_frames):
        e_s, de_s = s.debye_sweep(c[sl].contiguous(), q[sl].contiguous(), table, const_grads=True)
        assert torch.equal(e_s, e_dh[:, sl]) and torch.equal(de_s, de[:, sl]), sl
    for ts in E.SWEEP_T_SLICES:
        e_s, de_s = s.debye_sweep(c, q, table[list(ts)], const_grads=True)
        assert torch.equal(e_s, e_dh[list(ts)]) and torch.equal(de_s, de[list(ts)]), ts
    e_only, none = s.debye_sweep(c, q, table)  # without the gradients the 64 MiB hold every frame: one chunk, the same rows
    assert none is None and E.sweep_chunk(16, len(kts), False) > n_frames and torch.equal(e_only, e_dh)
    _report("B sweep")


@functools.lru_cache(maxsize=None)
def _map_kt_oracle():
    top, c, q, box = E.system_frames(2, "simple-helix", "crossing")
    _, cfg, _ = M.oracle_cfg(2)
    out = M.oracle_sweep(2, cfg, top, c, q, E.sweep_kts(_own_kt()), box=box, salt=S.SALT[2], hce=False, terms=True).numpy()
    out.setflags(write=False)
    return out


@DTYPES
def test_fused_sweep_of_129_temperatures_on_crossing_frames(dtype):
    """``map_kt`` with a table one longer than a sweep launch takes, on frames whose strands are images of each other: the
    fused path against the per-temperature loop and the oracle, under the bounds of
    tests/test_gpu_melting.py::test_fused_sweep_against_the_loop_and_the_oracle."""
    from mythos_amd.energy import base as B
    from mythos_amd.energy import dna2
    from mythos_amd.energy.base import Quaternion, RigidBody, space

    top, c0, q0, box = E.system_frames(2, "simple-helix", "crossing")
    ef = dna2.create_default_energy_fn(top, space.periodic(box)[0]).with_params(salt_conc=S.SALT[2], half_charged_ends=False)
    dev = torch.device("cuda", 0)
    body = RigidBody(center=torch.as_tensor(c0, dtype=dtype, device=dev), orientation=Quaternion(vec=torch.as_tensor(q0, dtype=dtype, device=dev)))
    kts = E.sweep_kts(_own_kt())
    fused = ef.map_kt(body, kts, sweep="fused")
    assert B.LAST_MAP_KT["path"] == "fused" and B.LAST_MAP_KT["sweep_launch"]
    loop = ef.map_kt(body, kts, sweep="per_temperature")
    assert B.LAST_MAP_KT["path"] == "per_temperature" and fused.shape == loop.shape == (129, 3)
    ref = _map_kt_oracle()
    total, scale = ref.sum(-1), np.abs(ref).sum(-1)
    tol = 1e-9 * scale + 8e-11 * 16 if dtype == torch.float64 else 1e-3 * scale
    for got in (fused.cpu().numpy(), loop.cpu().numpy()):
        _note(f"B map_kt {'fp64' if dtype == torch.float64 else 'fp32'} (of sum|terms|)", (np.abs(got - total) / scale).max())
        assert (np.abs(got - total) <= tol).all() if dtype == torch.float64 else (np.abs(got - total) < tol).all()
    assert (np.abs(fused.cpu().numpy() - loop.cpu().numpy()) <= tol).all()
    plain = ef.map(body).cpu().numpy()  # the first row is the function's own temperature: the plain energy call
    np.testing.assert_allclose(fused[0].cpu().numpy(), plain, rtol=1e-12 if dtype == torch.float64 else 1e-5)
    assert np.abs(ref[128, :, 7]).min() > 1e-2 and np.abs(total[128] - total[0]).min() > 1e-3
    _report("B map_kt")
