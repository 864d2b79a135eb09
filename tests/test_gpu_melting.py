"""Temperature sweep of the energy (``map_kt``: one energy launch + one Debye-Hueckel sweep launch) and the melting
temperature built on it, on the GPU, against the per-temperature loop and against the oracle initialised at every kT.

Bounds between kernel and oracle are those of tests/test_gpu_oxdna_energy.py: fp64 every TERM within rtol 1e-9 + atol 1e-11
per nucleotide - so a total within 1e-9 sum|terms| + 8e-11 per nucleotide; fp32 within 1e-3 of sum|terms|.
"""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import base as B
from mythos_amd.energy import dna1, dna2, na1, rna2
from mythos_amd.energy import flat_params as fp
from mythos_amd.energy.base import Quaternion, RigidBody, space
from mythos_amd.input import defaults
from mythos_amd.observables import MeltingTemp
from tests import helpers as H
from tests import melting_ref as M

pytestmark = pytest.mark.gpu

KT_LOW = 1e-4  # r_cut of the Debye-Hueckel term is about 0.06 there: no backbone pair is that close


def _own_kt(model):
    return defaults.default_configs_for(H.model_dir(model))[0]["kT"]


def _ranges(model):
    own = _own_kt(model)
    return {
        "T1": np.array([0.0987]),
        "T2": np.array([0.0933, 0.1166]),
        "T3": np.array([own, KT_LOW, 0.11]),
        "T20": M.kelvin_range(),
        "T65": np.concatenate([np.linspace(0.09, 0.12, 63), [own, KT_LOW]]),  # one past a wavefront
    }


def _sixty(name):
    from tests.test_oracle_golden import _sixty_bp

    return _sixty_bp(name)[:2]


# name -> (model, loader, salt, half-charged ends)
SYSTEMS = {
    "dna2/simple-helix": (2, lambda: H.load_golden(2, "simple-helix")[:2], 0.5, False),
    "dna2/simple-helix-salt0.15": (2, lambda: H.load_golden(2, "simple-helix")[:2], 0.15, False),
    "dna2/simple-helix-half-charged-ends": (2, lambda: H.load_golden(2, "simple-helix-half-charged-ends")[:2], 0.5, True),
    "regr/simple-helix-60bp-oxdna2": (2, lambda: _sixty("simple-helix-60bp-oxdna2"), 0.5, True),  # 120 nt: 4 tiles, the last partial
    "rna2/simple-helix-12bp": (3, lambda: H.load_golden(3, "simple-helix-12bp")[:2], 1.0, False),
}
CASES = [
    ("dna2/simple-helix", (0,), "T65"),
    ("dna2/simple-helix", (3, 50, 99), "T20"),
    ("dna2/simple-helix", tuple(range(100)), "T2"),
    ("dna2/simple-helix", (7,), "T1"),
    ("dna2/simple-helix-salt0.15", (3, 50), "T3"),
    ("dna2/simple-helix-half-charged-ends", (0, 40, 99), "T20"),
    ("regr/simple-helix-60bp-oxdna2", tuple(range(8)), "T3"),
    ("rna2/simple-helix-12bp", (0, 50, 99), "T20"),
]


def _energy_fn(name, periodic, weights=None):
    model, load, salt, hce = SYSTEMS[name]
    top, traj = load()
    disp = space.periodic(traj.box_size)[0] if periodic else space.free()[0]
    ef = (dna2 if model == 2 else rna2).create_default_energy_fn(top, disp).with_params(salt_conc=salt, half_charged_ends=hce)
    return (ef if weights is None else ef.replace(weights=torch.as_tensor(weights, dtype=torch.float64))), top, traj


def _body(traj, frames, dtype):
    idx = list(frames)
    dev = torch.device("cuda", 0)
    return RigidBody(center=torch.as_tensor(traj.center[idx], dtype=dtype, device=dev),
                     orientation=Quaternion(vec=torch.as_tensor(traj.quaternions[idx], dtype=dtype, device=dev)))


@functools.lru_cache(maxsize=None)
def _oracle(name, frames, rng, periodic):
    """(T, F, 8) oracle terms: computed once per case, shared by the precisions."""
    model, load, salt, hce = SYSTEMS[name]
    top, traj = load()
    _, cfg, _ = M.oracle_cfg(model)
    idx = list(frames)
    out = M.oracle_sweep(model, cfg, top, traj.center[idx], traj.quaternions[idx], _ranges(model)[rng],
                         box=traj.box_size if periodic else None, salt=salt, hce=hce, terms=True).numpy()
    out.setflags(write=False)
    return out


def _check(got, terms_ref, n, dtype, weights=None):
    w = np.ones(8) if weights is None else np.asarray(weights)
    ref = terms_ref @ w
    scale = np.abs(terms_ref * w).sum(-1)
    if dtype == torch.float64:
        assert (np.abs(got - ref) <= 1e-9 * scale + 8e-11 * n).all(), np.abs(got - ref).max()
    else:
        assert (np.abs(got - ref) / scale).max() < 1e-3


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("periodic", [False, True], ids=["free", "box"])
@pytest.mark.parametrize(("name", "frames", "rng"), CASES, ids=[f"{c[0]}-{len(c[1])}f-{c[2]}" for c in CASES])
def test_fused_sweep_against_the_loop_and_the_oracle(name, frames, rng, periodic, dtype):
    ef, top, traj = _energy_fn(name, periodic)
    model = SYSTEMS[name][0]
    kts = _ranges(model)[rng]
    body = _body(traj, frames, dtype)
    fused = ef.map_kt(body, kts, sweep="fused")
    assert B.LAST_MAP_KT == {"path": "fused", "reason": "stacking scale and Debye-Hueckel sweep", "sweep_launch": True}
    again = ef.map_kt(body, kts)  # the automatic choice takes the same path; two fused calls are bitwise equal
    assert B.LAST_MAP_KT["path"] == "fused" and torch.equal(fused, again)
    loop = ef.map_kt(body, kts, sweep="per_temperature")
    assert B.LAST_MAP_KT["path"] == "per_temperature" and not B.LAST_MAP_KT["sweep_launch"]
    assert fused.shape == loop.shape == (len(kts), len(frames)) and fused.dtype == torch.float64
    ref = _oracle(name, frames, rng, periodic)
    n = top.n_nucleotides
    _check(fused.cpu().numpy(), ref, n, dtype)
    _check(loop.cpu().numpy(), ref, n, dtype)
    scale = np.abs(ref).sum(-1)
    tol = 1e-9 * scale + 8e-11 * n if dtype == torch.float64 else 1e-3 * scale
    assert (np.abs(fused.cpu().numpy() - loop.cpu().numpy()) <= tol).all()
    own = np.nonzero(kts == _own_kt(model))[0]
    if len(own):  # rho = 1 and the function's own Debye constants: the plain energy call
        plain = ef.map(body).cpu().numpy()
        np.testing.assert_allclose(fused[own[0]].cpu().numpy(), plain, rtol=1e-12 if dtype == torch.float64 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["dna2/simple-helix-half-charged-ends", "regr/simple-helix-60bp-oxdna2", "rna2/simple-helix-12bp"])
def test_sweep_kernel_rows_against_the_energy_kernel(name, dtype):
    """The C entry point itself: the row at the system's own constants is the Debye column of the energy call and its
    partials are the DH_* columns of dU/dparams; a temperature whose r_cut excludes every pair gives a row of exact
    zeros; two calls agree bit for bit; a table longer than one launch takes gives the same rows.  (The 120-nt system walks
    its 116-entry rows in four segments and has four tiles, the last one partial.)"""
    from mythos_amd.hip_system import OxdnaSystem

    model, load, salt, hce = SYSTEMS[name]
    top, traj = load()
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=salt, half_charged_ends=hce), _lib.param_names())
    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=traj.box_size, dtype=dtype)
    s.set_params(flat)
    s.set_neighbors(top.unbonded_neighbors)
    body = _body(traj, range(min(5, traj.center.shape[0])), dtype)
    c, q = body.center, body.orientation.vec
    kts = np.array([sim["kT"], KT_LOW, 0.0933, 0.1166, 0.3])
    _, table = fp.kt_sweep_tables(model, cfg, kts, kt=sim["kT"], salt_conc=salt)
    e, _, _, gp = s.energy(c, q, param_grads=True)
    e_dh, de = s.debye_sweep(c, q, table, const_grads=True)
    e_only, none = s.debye_sweep(c, q, table)
    assert none is None and torch.equal(e_only, e_dh)
    e2, de2 = s.debye_sweep(c, q, table, const_grads=True)
    assert torch.equal(e2, e_dh) and torch.equal(de2, de)
    rtol = 1e-12 if dtype == torch.float64 else 2e-6  # fp32: the energy kernel sums the pairs in fp32, the sweep in fp64
    torch.testing.assert_close(e_dh[0], e[:, 7], rtol=rtol, atol=0)
    cols = [_lib.param_names().index(n) for n in fp.DEBYE_KT_NAMES]
    torch.testing.assert_close(de[0], gp[:, cols], rtol=rtol * 10, atol=rtol * float(gp[:, cols].abs().max()))
    assert (de[:, :, 4] == 0).all() and (de[0, :, :2] != 0).all()  # r_high enters through the branch only
    assert (e_dh[1] == 0).all() and (de[1] == 0).all()
    assert (e_dh[[0, 2, 3, 4]] > 0).all() and (e_dh[4] > e_dh[3]).all()  # the screening length grows with kT
    # T = 130: more than one launch's table (128 temperatures per launch); every row equals the row of a short call
    many = np.concatenate([np.tile(table, (26, 1))])
    e_many, de_many = s.debye_sweep(c, q, many, const_grads=True)
    assert torch.equal(e_many.reshape(26, 5, -1)[0], e_dh) and torch.equal(e_many.reshape(26, 5, -1)[25], e_dh)
    assert torch.equal(de_many.reshape(26, 5, -1, 5)[25], de)
    # ABI edges: an empty table and an empty batch return cleanly
    e0, _ = s.debye_sweep(c, q, np.zeros((0, 5)))
    assert e0.shape == (0, c.shape[0])
    ee, _ = s.debye_sweep(c[:0], q[:0], table)
    assert ee.shape == (5, 0)
    with pytest.raises(ValueError, match="NaN"):
        s.debye_sweep(c, q, np.full((1, 5), np.nan))


def test_model1_takes_the_fused_path_without_a_sweep_launch_and_honours_noopt():
    top, traj, _ = M.load_run()
    ef = dna1.create_default_energy_fn(top, space.periodic(M.BOX)[0]).with_noopt("ss_stack_weights", "ss_hb_weights", "kt").with_params(kt=M.KT_SIM)
    frames = tuple(range(0, 384, 16))
    body = _body(traj, frames, torch.float64)
    kts = M.kelvin_range()
    assert ef.map_kt_plan(body) == ("fused", "stacking scale only: no Debye-Hueckel term to sweep")
    fused = ef.map_kt(body, kts)
    assert B.LAST_MAP_KT == {"path": "fused", "reason": "stacking scale only: no Debye-Hueckel term to sweep", "sweep_launch": False}
    loop = ef.map_kt(body, kts, sweep="per_temperature")
    ref = M.fixture_reference()["et"][:, list(frames)]
    np.testing.assert_allclose(fused.cpu().numpy(), ref, rtol=1e-9, atol=8e-11 * 12)
    np.testing.assert_allclose(fused.cpu().numpy(), loop.cpu().numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_composed_weights_are_honoured(dtype):
    w = [1.0, 0.5, 1.7, 2.0, 0.8, 1.25, 3.0, 0.6]
    ef, top, traj = _energy_fn("dna2/simple-helix", True, weights=w)
    frames, rng = (3, 50, 99), "T20"
    body = _body(traj, frames, dtype)
    kts = _ranges(2)[rng]
    fused = ef.map_kt(body, kts, sweep="fused").cpu().numpy()
    loop = ef.map_kt(body, kts, sweep="per_temperature").cpu().numpy()
    ref = _oracle("dna2/simple-helix", frames, rng, True)
    _check(fused, ref, top.n_nucleotides, dtype, weights=w)
    _check(loop, ref, top.n_nucleotides, dtype, weights=w)
    assert np.abs(fused - ref.sum(-1)).max() > 1.0  # the weights matter
    # a function without the Debye term: the fused path scales the stacking term and launches no sweep
    short = ef.without_terms("Debye")
    got = short.map_kt(body, kts)
    assert B.LAST_MAP_KT["path"] == "fused" and not B.LAST_MAP_KT["sweep_launch"]
    _check(got.cpu().numpy(), ref, top.n_nucleotides, dtype, weights=[*w[:7], 0.0])


def test_oxna_takes_the_fallback_and_the_entry_point_refuses_it():
    top, traj, _, _ = H.load_golden_na1("simple-helix-dna-rna")
    ef = na1.create_default_energy_fn(top, space.periodic(traj.box_size)[0])
    body = _body(traj, (0, 30), torch.float64)
    kts = np.array([0.0933, 0.1, 0.1166])
    assert ef.map_kt_plan(body)[0] == "per_temperature"
    got = ef.map_kt(body, kts)
    assert B.LAST_MAP_KT["path"] == "per_temperature" and "oxNA" in B.LAST_MAP_KT["reason"]
    want = torch.stack([ef.with_params(kt=float(k)).map(body) for k in kts])
    assert torch.equal(got, want) and float((got[0] - got[2]).abs().min()) > 1e-3
    with pytest.raises(ValueError, match="oxNA"):
        ef.map_kt(body, kts, sweep="fused")
    system = next(e["sys"] for k, e in B._SYSTEMS.items() if k[0] == 4)
    with pytest.raises(ValueError, match="oxNA system has three"):
        system.debye_sweep(body.center, body.orientation.vec, np.ones((2, 5)))


def test_fused_refuses_coordinate_gradients_and_the_automatic_choice_falls_back():
    ef, top, traj = _energy_fn("dna2/simple-helix", True)
    body = _body(traj, (0, 1), torch.float64)
    moving = RigidBody(center=body.center.clone().requires_grad_(True), orientation=body.orientation)
    with pytest.raises(NotImplementedError):
        ef.map_kt(moving, [0.1], sweep="fused")
    e = ef.map_kt(moving, [0.1])
    assert B.LAST_MAP_KT["path"] == "per_temperature" and "coordinates" in B.LAST_MAP_KT["reason"]
    (g,) = torch.autograd.grad(e.sum(), moving.center)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


# ---- the observable end to end --------------------------------------------------------------------------------------------
def _melting_setup(dtype, sweep=None):
    top, traj, en = M.load_run()
    ef = dna1.create_default_energy_fn(top, space.periodic(M.BOX)[0]).with_noopt("ss_stack_weights", "ss_hb_weights", "kt").with_params(kt=M.KT_SIM)
    mt = MeltingTemp(sim_temperature=M.KT_SIM, temperature_range=M.kelvin_range(), energy_fn=ef, sweep=sweep)
    return mt, ef, _body(traj, range(384), dtype), en


def test_melting_temperature_of_the_fixture_fp64():
    """Tm within 1e-8 of the oracle's: a 1e-9 per-nucleotide energy error over 12 nt at kT ~ 0.09 is ~1.3e-7 in a frame's
    weight, and the curve's slope near 0.5 (about 0.15 per 0.0015 in kT) turns that into ~3e-9."""
    mt, ef, body, en = _melting_setup(torch.float64)
    ref = M.fixture_reference()
    args = (body, en["bond"], en["weight"], ef.opt_params())
    tm = mt(*args)
    assert B.LAST_MAP_KT["path"] == "fused"
    assert abs(float(tm) - ref["tm"]) <= 1e-8 and abs(float(tm) - 0.10144342) <= 1e-8
    temps, curve = mt.get_melting_curve(*args)
    np.testing.assert_allclose(temps.cpu().numpy(), ref["kts"], rtol=0, atol=0)
    # the same 1.3e-7 per weight, relative, on every ratio of sums of weights (and a little through the correction)
    np.testing.assert_allclose(curve.cpu().numpy(), ref["ratios"], rtol=1e-6)
    assert (np.diff(curve.cpu().numpy()) < 0).all()
    assert abs(float(mt.get_melting_curve_width(*args)) - ref["width"]) <= 1e-8
    loop = MeltingTemp(sim_temperature=M.KT_SIM, temperature_range=M.kelvin_range(), energy_fn=ef, sweep="per_temperature")
    assert abs(float(loop(*args)) - float(tm)) <= 1e-8


def test_melting_temperature_of_the_fixture_fp32_frames():
    """fp32 frames: the fused path against the fp32 per-temperature path.  Both read the same fp32 frames with the same
    fp32 pair arithmetic; they differ in how the stacking term reaches kT_t - scaled in fp64 after the sum, or summed in
    fp32 with the scaled strength: at worst the rounding of ~30 fp32 additions (6e-8 each) on a term of magnitude <= 17 for
    12 nt, 3e-5 in E_t(f), 3e-4 in a frame's exponent at kT ~ 0.1, so at most 3e-4 x 0.25 in a ratio near 0.5, which the
    curve's slope (about 100 per unit of kT) turns into 7.5e-7 in Tm: bound 1e-6.  (The difference from the fp64 oracle is
    printed, not asserted.)"""
    mt, ef, body, en = _melting_setup(torch.float32)
    args = (body, en["bond"], en["weight"], ef.opt_params())
    tm = float(mt(*args))
    loop = MeltingTemp(sim_temperature=M.KT_SIM, temperature_range=M.kelvin_range(), energy_fn=ef, sweep="per_temperature")
    tm_loop = float(loop(*args))
    print(f"fp32 Tm fused {tm:.10f} loop {tm_loop:.10f} oracle {M.fixture_reference()['tm']:.10f}")
    assert abs(tm - tm_loop) <= 1e-6


# ---- gradients --------------------------------------------------------------------------------------------------------------
# d(Tm)/d(theta).  oxDNA1 as the reference's fixture has it (there d(Tm)/d(eps_stack_kt_coeff) vanishes identically: with the
# average-sequence strength eps = base + c kT the exponent E_0 / kT_sim - E_t / kT_t has no c in it - the fused path must
# cancel it to rounding).  oxDNA2 on the same frames with a fixed sequence-dependent stacking table, eps = W (1 - c + 9 c kT):
# there eps_stack_kt_coeff carries d(rho_t)/d(theta), and eps_stack_base is not a parameter of the function.  Of the 384
# frames the oxDNA2 case keeps those without steric clashes under the oxDNA2 backbone site (oracle energy at kT_sim below
# zero: 102 frames, 46 unbound); with the others E is up to 1.6e6 and the reference's own exp overflows.
GRAD_NAMES = {1: ("eps_stack_base", "eps_stack_kt_coeff", "a_stack", "eps_hb"),
              2: ("eps_stack_kt_coeff", "a_stack", "eps_hb", "prefactor_coeff", "q_eff", "lambda_factor")}
SECTION = {"eps_stack_base": "stacking", "eps_stack_kt_coeff": "stacking", "a_stack": "stacking", "eps_hb": "hydrogen_bonding",
           "prefactor_coeff": "debye", "q_eff": "debye", "lambda_factor": "debye"}
SS_STACK = 1.0 + 0.05 * np.arange(16.0).reshape(4, 4) / 15.0
# worst deviation of d(Tm)/d(theta) from the oracle's autograd relative to max(|reference|, 1e-3 max over the parameters |reference|)
# (the scale of the dU/dtheta tests): measured on an MI355X, asserted at 100 x that and never looser than 1e-6
GRAD_BOUND = 2.6e-10  # measured: 2.6e-12 (oxDNA1), 1.0e-12 (oxDNA2)


@functools.lru_cache(maxsize=None)
def _grad_frames(model):
    top, traj, _ = M.load_run()
    if model == 1:
        return tuple(range(0, 384, 2))
    _, cfg, _ = M.oracle_cfg(2)
    e = M.oracle_sweep(2, cfg, top, traj.center, traj.quaternions, [M.KT_SIM], box=np.full(3, M.BOX), salt=0.5, hce=True)[0].numpy()
    return tuple(int(k) for k in np.nonzero(e < 0)[0])


@functools.lru_cache(maxsize=None)
def _oracle_tm_grads(model):
    """(Tm, {name: dTm/dname}) by autograd through the oracle, on the melting fixture's frames."""
    top, traj, en = M.load_run()
    idx = list(_grad_frames(model))
    _, cfg, leaves = M.oracle_cfg(model, leaves=True)
    if model == 2:
        cfg["stacking"]["ss_stack_weights"] = torch.as_tensor(SS_STACK)
    kts = M.kelvin_range()
    kw = dict(box=np.full(3, M.BOX), salt=0.5, hce=True)
    e0 = M.oracle_sweep(model, cfg, top, traj.center[idx], traj.quaternions[idx], [M.KT_SIM], **kw)[0]
    et = M.oracle_sweep(model, cfg, top, traj.center[idx], traj.quaternions[idx], kts, **kw)
    tm = M.ref_tm(kts, M.ref_ratios(e0, et, M.KT_SIM, kts, en["bond"][idx], en["weight"][idx]))
    names = GRAD_NAMES[model]
    g = torch.autograd.grad(tm, [leaves[(SECTION[n], n)] for n in names])
    return float(tm.detach()), {n: float(x) for n, x in zip(names, g)}


@pytest.mark.parametrize("model", [1, 2], ids=["dna1", "dna2"])
def test_melting_temperature_gradient(model):
    top, traj, en = M.load_run()
    idx = list(_grad_frames(model))
    assert len(idx) == (192 if model == 1 else 102) and 40 < int((en["bond"][idx] == 0).sum()) < len(idx) - 40
    mod = dna1 if model == 1 else dna2
    ef = mod.create_default_energy_fn(top, space.periodic(M.BOX)[0]).with_params(kt=M.KT_SIM)
    if model == 2:
        ef = ef.with_params(salt_conc=0.5, half_charged_ends=True, ss_stack_weights=torch.as_tensor(SS_STACK))
    body = _body(traj, idx, torch.float64)
    names = GRAD_NAMES[model]
    tm_ref, g_ref = _oracle_tm_grads(model)
    kts = M.kelvin_range()
    assert kts[0] < tm_ref < kts[-1]  # the curve crosses 0.5 inside the range: Tm depends on the parameters
    got = {}
    for sweep in ("fused", "per_temperature"):
        opt = {n: torch.tensor(float(ef.params_dict()[n]), dtype=torch.float64, requires_grad=True) for n in names}
        mt = MeltingTemp(sim_temperature=M.KT_SIM, temperature_range=kts, energy_fn=ef, sweep=sweep)
        tm = mt(body, en["bond"][idx], en["weight"][idx], opt)
        assert B.LAST_MAP_KT["path"] == sweep and abs(float(tm) - tm_ref) <= 1e-8
        g = torch.autograd.grad(tm, [opt[n] for n in names])
        got[sweep] = {n: float(x) for n, x in zip(names, g)}
    top_ref = max(abs(v) for v in g_ref.values())
    assert sum(abs(v) > 1e-3 * top_ref for v in g_ref.values()) >= len(names) - (1 if model == 1 else 0)
    worst = 0.0
    for n in names:
        scale = max(abs(g_ref[n]), 1e-3 * top_ref)
        dev = {s: abs(got[s][n] - g_ref[n]) / scale for s in got}
        print(f"dTm/d{n}: oracle {g_ref[n]:+.12e} fused {got['fused'][n]:+.12e} (dev {dev['fused']:.2e}) loop dev {dev['per_temperature']:.2e}")
        worst = max(worst, dev["fused"], dev["per_temperature"], abs(got["fused"][n] - got["per_temperature"][n]) / scale)
    print(f"worst relative deviation, model {model}: {worst:.3e}")
    assert worst <= GRAD_BOUND
