"""Stream-order tests: every entry of include/mythos_hip.h that takes a stream, sets a table or reads one back runs on a
non-default, non-blocking stream behind a forced delay (tests/stream_order.py has the method and the four hazard kinds).

The rest of the suite runs on torch's current stream, which is the legacy null stream: there every blocking copy, memset and
``hipStreamSynchronize(nullptr)`` of the library is ordered with every kernel by accident, so work issued on the wrong
stream, a host read that does not wait for the launch stream and a setter that overwrites a table under a queued launch all
pass unseen.  The intended caller (a jax.custom_vjp on XLA's stream) never uses the null stream.

The table.  CASES holds one ``stream_order.Case`` per entry family; ``covers`` names the C exports a case drives and the
hazard kinds it drives them under.  tests/test_stream_cases_cpu.py parses the header and fails when an export with a stream
parameter, a setter or a getter has neither a case here nor a reason in EXCLUDED.  Equality is bitwise (the header says
"reproducible bit for bit", or an existing test asserts bitwise repeats: tests/test_gpu_oxdna_energy.py
test_parameter_gradients_are_bitwise_reproducible, tests/test_gpu_pseq.py:252, tests/test_gpu_martini.py:199,
tests/test_gpu_martini_coulomb.py:241, tests/test_gpu_energy_shapes.py:379, the split-call tests of the integrators) with
one exception, named at its case: dU/d(distribution) of mythos_oxdna_energy_dpseq (fp64 atomics).

Systems: the 16-nt dna2/simple-helix golden in its periodic box (frames 0 and -1 as A and B), the 24-nt
rna2/simple-helix-12bp golden for the second handle, the na1 dna-rna helix for the nucleotide types, md37 and n257 of
tests/martini_synth.py (A: the system's frame, B: the same frame scaled by 1.001 with every bead moved by up to 0.02 nm),
3 replicas for ensembles, 6 - 12 MD steps.

Cost on the MI355X (one run of this file; the delay of 50 ms dominates a case, a case that synchronises arms it twice or
three times):
    53 tests (31 IN / OUT / GET cases, 20 SET cases, 2 two-handle tests)    slowest case: 0.38 s (the first one: library
    load and calibration)    file: 6.7 s    the rest of the GPU suite with the parent commit's library, same machine:
    1213 tests in 117 s (with this file: 1266 in 125 s)

What the cases found in the library as it stood before them (each is fixed; the case is named):
    oxdna_set_neighbors        mythos_oxdna_set_neighbors replaced the rows with blocking null-stream copies and waited for
                               nothing: an energy launch queued behind the delay ran on the NEW rows (the first launch
                               returned the result of state B).  Now it synchronises the device first, as its siblings do.
    oxdna_build_neighbors, martini_run, martini_load_advance_store (the neighbor_stats GET cases)
                               pass before and after: the null-stream copy of row_stats was never ordered with the stream
                               that builds the rows, but every call that writes rows - build_neighbors, run, advance, the
                               closing launch of store - ends with a synchronisation of its stream, so one host thread
                               cannot have a build in flight when it asks.  The getters now synchronise the device, which
                               is what the header promises and what the *_get_rows entries did.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults
from tests import helpers as H
from tests import martini_synth as S
from tests import stream_order as SO
from tests.stream_order import GET, IN, OUT, SET, Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KT_OX = 296.15 * 0.1 / 300.0
KB = 0.0083144626
KT_M = KB * 273.0

CASES: list = []
SET_CASES: list = []

# Exports that match the patterns of tests/test_stream_cases_cpu.py and have no case, each with its reason.
EXCLUDED = {
    "mythos_last_error": "host only: the thread-local text of the last error, no device and no stream behind it",
    "mythos_langevin_set_option": "host flag read at the next load; its one option is the unfused oxNA path, a second "
                                  "implementation kept as a cross-check that no stream caller runs",
    "mythos_langevin_set_neighbor_policy": "host numbers read when the next advance builds its list; set in the setup of every oxDNA MD case here",
    "mythos_martini_langevin_set_neighbor_policy": "host numbers read when the next advance builds its list; set in the setup of every MARTINI MD case here",
    "mythos_martini_langevin_set_inner_list": "host numbers read when the next advance builds its list; set in the setup of martini_run",
}
# Covered exports whose header comment says nothing about streams or synchronisation.  Empty: the header documents every one.
UNDOCUMENTED: list = []


def io(name, covers, setup, inputs, call, **kw):
    CASES.append(Case(name, covers, setup, inputs, call, **kw))


def setter(name, covers, setup, inputs, call, install, **kw):
    SET_CASES.append(Case(name, covers, setup, inputs, call, install=install, **kw))


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


# ======================================================================================================== oxDNA system
@functools.lru_cache(maxsize=None)
def _ox_flat(model, kt_scale=1.0):
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    return fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"] * kt_scale, salt_conc=1.0 if model == 3 else 0.5, half_charged_ends=False),
                        _lib.param_names()).detach()


def _ox_golden(model):
    return H.load_golden(model, "simple-helix" if model != 3 else "simple-helix-12bp")


def _ox_system(model=2, dtype=torch.float64, neighbors=True):
    from mythos_amd.hip_system import OxdnaSystem

    top, traj, _, _ = _ox_golden(model)
    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=traj.box_size, dtype=dtype, device=DEV)
    s.set_params(_ox_flat(model))
    if neighbors:
        s.set_neighbors(top.unbonded_neighbors)
    return s


def _ox_frames(model=2, dtype=torch.float64, count=1):
    """{"A": frames 0 .., "B": frames -1, -2 ..} of the golden trajectory as (count, n, .) tensors ((n, .) for count = 1)."""
    _, traj, _, _ = _ox_golden(model)
    out = {}
    for which, idx in (("A", list(range(count))), ("B", [-1 - k for k in range(count)])):
        c, q = _t(np.asarray(traj.center)[idx], dtype), _t(np.asarray(traj.quaternions)[idx], dtype)
        out[which] = {"c": c[0].contiguous(), "q": q[0].contiguous()} if count == 1 else {"c": c, "q": q}
    return out


def _pseq_tables(seed):
    from mythos_amd.input import sequence_constraints as scm
    from tests import oxdna_energy_shapes as E

    sc = E.constraints(16)
    rng = np.random.default_rng(seed)

    def dist(rows):
        a = rng.random((rows, 4)) + 0.05
        return a / a.sum(1, keepdims=True)

    return scm.kernel_tables((dist(sc.n_unpaired), dist(sc.n_bp)), sc)


def _energy_case(variant):
    def setup():
        s = _ox_system()
        if variant == "dpseq":
            s.set_pseq(*_pseq_tables(11), 3)
        return {"s": s}

    def call(ctx, b, probe):
        s = ctx["s"]
        out = s.energy(b["c"], b["q"], grads=variant in ("forces", "dtheta"), param_grads=variant in ("dtheta", "dpseq"),
                       pseq_grads=variant == "dpseq")
        probe.after()
        return out

    # dU/d(distribution): "accumulated with fp64 atomics: equal to rounding between runs, not bit for bit"
    # (include/mythos_hip.h).  No repeat test exists for it; the bound is the one tests/test_gpu_energy_shapes.py
    # (_check_pseq, fp64) holds the same outputs to: 1e-9 of max(1, max|ref|).
    def rounding(a, b):
        return bool((a - b).abs().max() <= 1e-9 * max(1.0, float(b.abs().max())))

    entry = "mythos_oxdna_energy_dpseq" if variant == "dpseq" else "mythos_oxdna_energy"
    io(f"oxdna_energy[{variant}]", {entry: [IN, OUT]}, setup, lambda ctx: _ox_frames(count=3), call,
       close={"out[4]": rounding, "out[5]": rounding} if variant == "dpseq" else None)


for _v in ("energies", "forces", "dtheta", "dpseq"):
    _energy_case(_v)


def _duplex_lists():
    from mythos_amd.observables.base import get_duplex_quartets

    return [[k, 15 - k] for k in range(8)], get_duplex_quartets(8).numpy()


def _obs_set(dtype=torch.float64):
    from mythos_amd.observables.base import ObservableSet

    _, traj, _, _ = _ox_golden(2)
    _, cfg = defaults.default_configs_for("dna2")
    pairs, quartets = _duplex_lists()
    return ObservableSet(16, 2, cfg["geometry"], traj.box_size, pairs, quartets, True, dtype, DEV)


def _call_energy_obs(ctx, b, probe):
    out = ctx["s"].energy(b["c"], b["q"], grads=True, observables=ctx["obs"])
    probe.after()
    return out


io("oxdna_energy_obs", {"mythos_oxdna_energy_obs": [IN, OUT]}, lambda: {"s": _ox_system(), "obs": _obs_set()},
   lambda ctx: _ox_frames(count=3), _call_energy_obs)


def _call_obs_eval(ctx, b, probe):
    out = ctx["obs"].eval(b["c"], b["q"])
    probe.after()
    return out


io("observables_eval", {"mythos_observables_eval": [IN, OUT]}, lambda: {"obs": _obs_set()}, lambda ctx: _ox_frames(count=3), _call_obs_eval)


def _duplex_set():
    from mythos_amd.observables.base import DuplexSet

    _, traj, _, _ = _ox_golden(2)
    _, cfg = defaults.default_configs_for("dna2")
    pairs, quartets = _duplex_lists()
    c0 = np.asarray(traj.center[0], dtype=np.float64)
    return DuplexSet(16, 2, cfg["geometry"], traj.box_size, pairs, quartets, end_pairs=[0, 15, 7, 8], target=c0 - c0.mean(0), device=DEV)


io("duplex_obs_eval", {"mythos_duplex_obs_eval": [IN, OUT]}, lambda: {"obs": _duplex_set()}, lambda ctx: _ox_frames(count=3), _call_obs_eval)


def _sweep_table():
    names = _lib.param_names()
    cols = [names.index(k) for k in ("DH_KAPPA", "DH_PREFACTOR", "DH_BSMOOTH", "DH_RCUT", "DH_RHIGH")]
    return np.stack([_ox_flat(2, f).numpy()[cols] for f in (1.0, 0.95, 1.07)])


def _call_sweep(ctx, b, probe):
    out = ctx["s"].debye_sweep(b["c"], b["q"], _sweep_table(), const_grads=True)
    probe.after()
    return out


io("oxdna_debye_sweep", {"mythos_oxdna_debye_sweep": [IN, OUT]}, lambda: {"s": _ox_system()}, lambda ctx: _ox_frames(count=3), _call_sweep)


def _ops(which):
    from tests import order_param_ref as R

    return R.native_ops(8) if which == 0 else R.native_ops(8, kinds=("mindistance", "bond"), interfaces=(0.8, 1.5))


def _setup_order_params():
    s = _ox_system()
    fr = _ox_frames(count=3)["A"]
    s.order_params(fr["c"], fr["q"], _ops(0), raw=True)  # the lists are on the device: a call with the same lists does not wait
    torch.cuda.synchronize()
    return {"s": s}


def _call_order_params(ctx, b, probe):
    out = ctx["s"].order_params(b["c"], b["q"], _ops(0), raw=True)
    probe.after()
    return out


def _call_order_params_new_lists(ctx, b, probe):
    """The "waits for `stream`" clause: the second call brings other lists while the first one is still queued; it must wait
    for it (the first call then still sees its own lists) and is then ordered itself."""
    first = ctx["s"].order_params(b["c"], b["q"], _ops(0), raw=True)
    probe.after()
    second = ctx["s"].order_params(b["c"], b["q"], _ops(1), raw=True)
    probe.rearm()
    return first, second


io("oxdna_order_params", {"mythos_oxdna_order_params": [IN, OUT]}, _setup_order_params, lambda ctx: _ox_frames(count=3), _call_order_params)
io("oxdna_order_params[new lists]", {"mythos_oxdna_order_params": [IN, OUT, SET]}, _setup_order_params, lambda ctx: _ox_frames(count=3),
   _call_order_params_new_lists)


def _call_build_neighbors(ctx, b, probe):
    s = ctx["s"]
    probe.before()
    s.build_neighbors(b["c"], r_cut=3.25, skin=0.4)  # (grows rows until they fit: synchronises the stream)
    probe.rearm()
    e = s.energy(b["c"], b["q"], grads=True)
    probe.after()
    return e, s.neighbor_stats(), s.rows()  # the getters wait for the device: the energy launch is still behind its delay


io("oxdna_build_neighbors", {"mythos_oxdna_build_neighbors": [IN, OUT], "mythos_oxdna_neighbor_stats": [GET], "mythos_oxdna_get_rows": [GET]},
   lambda: {"s": _ox_system(neighbors=False)}, lambda ctx: _ox_frames(), _call_build_neighbors)


# ---- SET on the system's tables: an energy launch queued behind the delay, the setter from the host, a second launch ----
def _call_energy_forces(ctx, b, probe):
    out = ctx["s"].energy(b["c"], b["q"], grads=True)
    probe.after()
    return out


setter("oxdna_set_params", {"mythos_oxdna_set_params": [SET]}, lambda: {"s": _ox_system()}, lambda ctx: _ox_frames(), _call_energy_forces,
       lambda ctx, w: ctx["s"].set_params(_ox_flat(2, 1.0 if w == "A" else 1.05)))
setter("oxdna_set_pseq", {"mythos_oxdna_set_pseq": [SET]}, lambda: {"s": _ox_system()}, lambda ctx: _ox_frames(), _call_energy_forces,
       lambda ctx, w: ctx["s"].set_pseq(*_pseq_tables(11 if w == "A" else 12), 3))


def _pair_lists():
    top, _, _, _ = _ox_golden(2)
    pairs = np.asarray(top.unbonded_neighbors, dtype=np.int32).reshape(-1, 2)
    native = {(k, 15 - k) for k in (0, 3, 4)}
    fewer = np.array([p for p in pairs.tolist() if (min(p), max(p)) not in native], dtype=np.int32)
    assert 0 < fewer.shape[0] < pairs.shape[0]
    return {"A": pairs, "B": fewer}  # (rows of the same stride: the setter replaces them in place)


setter("oxdna_set_neighbors", {"mythos_oxdna_set_neighbors": [SET]}, lambda: {"s": _ox_system(neighbors=False)}, lambda ctx: _ox_frames(),
       _call_energy_forces, lambda ctx, w: ctx["s"].set_neighbors(_pair_lists()[w]))


def _install_built_rows(ctx, w):
    c = _ox_frames()["A"]["c"]
    ctx["s"].build_neighbors(c.clone(), r_cut=3.25 if w == "A" else 1.2, skin=0.4 if w == "A" else 0.1)


setter("oxdna_build_neighbors[set]", {"mythos_oxdna_build_neighbors": [SET]}, lambda: {"s": _ox_system(neighbors=False)}, lambda ctx: _ox_frames(),
       _call_energy_forces, _install_built_rows)


def _na1_system():
    from mythos_amd.hip_system import OxdnaSystem

    top, traj, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    sim, cfg = defaults.default_configs_for("na1")
    flat = fp.pack_flat_na1(fp.derive_flat_na1(cfg["dna"], cfg["rna"], cfg["drh"], kt=sim["kT"], salt_conc=0.5, half_charged_ends=False),
                            _lib.param_names()).detach()
    s = OxdnaSystem(4, top.seq, top.is_end, top.bonded_neighbors, box=traj.box_size, dtype=torch.float64, device=DEV, is_rna=is_rna)
    s.set_params(flat)
    s.set_neighbors(top.unbonded_neighbors)
    return {"s": s, "is_rna": np.asarray(is_rna, dtype=bool)}


def _na1_frames(ctx):
    _, traj, _, _ = H.load_golden_na1("simple-helix-dna-rna")
    return {w: {"c": _t(traj.center[i]), "q": _t(traj.quaternions[i])} for w, i in (("A", 0), ("B", -1))}


def _install_types(ctx, w):
    t = np.ascontiguousarray(ctx["is_rna"] if w == "A" else ~ctx["is_rna"], dtype=np.uint8)  # B: the strands' types swapped
    _lib.check(ctx["s"]._lib.mythos_oxdna_set_nucleotide_types(ctx["s"]._h, t.ctypes.data_as(_lib.c_uint8_p)), "set_nucleotide_types")


setter("oxdna_set_nucleotide_types", {"mythos_oxdna_set_nucleotide_types": [SET]}, _na1_system, _na1_frames, _call_energy_forces, _install_types)


# ==================================================================================================== oxDNA integrator
def _ox_integrator(dtype=torch.float32, skin=0.02, every=1000, seed=7):
    """Thin skin, no scheduled rebuild inside a call: a site leaves its skin within a few steps, the launches halt, the
    run rebuilds and resumes - inside the delayed call."""
    from mythos_amd.hip_system import LangevinIntegrator

    s = _ox_system(dtype=dtype, neighbors=False)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT_OX, gamma_t=KT_OX / 2.5, gamma_r=KT_OX / 7.5, seed=seed)
    integ.set_neighbor_policy(r_cut=3.3, skin=skin, every=every)
    return {"s": s, "integ": integ}


def _ox_states(dtype=torch.float32):
    fr = _ox_frames(dtype=dtype)
    out = {}
    for k, (w, b) in enumerate(fr.items()):
        g = torch.Generator().manual_seed(100 + k)
        p = (KT_OX ** 0.5) * torch.randn(16, 3, generator=g, dtype=torch.float64)
        ang = (KT_OX ** 0.5) * torch.randn(16, 3, generator=g, dtype=torch.float64)
        out[w] = dict(b, p=p.to(DEV, dtype).contiguous(), ang=ang.to(DEV, dtype).contiguous())
    return out


def _md_figures(integ):
    ms = integ.last_kernel_ms()
    return {"recoveries": integ.last_recoveries(), "rebuilds": integ.last_rebuilds(), "step": integ.step, "launches": ms["launches"],
            "samples": ms["samples"]}


def _call_ox_run(ctx, b, probe):
    integ = ctx["integ"]
    integ.set_timing(2)
    probe.before()
    rows = integ.run(b["c"], b["q"], b["p"], b["ang"], 12, save_every=4, want_energy=True)  # energy rows
    probe.rearm()
    ctx["recoveries"] = integ.last_recoveries()
    fig = _md_figures(integ)
    plain = integ.run(b["c"], b["q"], b["p"], b["ang"], 6, save_every=3, want_energy=False)  # plain rows
    return rows, fig, plain, _md_figures(integ), b


def _recovered(ctx):
    assert ctx["recoveries"] >= 1, "no halt-rebuild-resume inside the call: not the scenario intended"


_MD_GETTERS = {"mythos_langevin_last_recoveries": [GET], "mythos_langevin_last_rebuilds": [GET], "mythos_langevin_get_step": [GET],
               "mythos_langevin_last_kernel_ms": [GET], "mythos_langevin_set_timing": [SET]}
io("langevin_run", {"mythos_langevin_run": [IN, OUT], **_MD_GETTERS}, _ox_integrator, lambda ctx: _ox_states(), _call_ox_run, check_default=_recovered)


def _call_ox_resident(ctx, b, probe):
    integ = ctx["integ"]
    integ.load(b["c"], b["q"], b["p"], b["ang"])
    probe.after()  # load is asynchronous
    first = integ.advance(6, save_every=3, want_energy=False)  # one synchronisation per call; leaves the frame open
    ctx["recoveries"] = integ.last_recoveries()
    fig = _md_figures(integ)
    probe.rearm()
    second = integ.advance(6, save_every=2, want_energy=True)  # its last step saves an energy row: the frame is closed
    probe.rearm()
    out = {k: torch.empty_like(v) for k, v in b.items()}
    integ.store(out["c"], out["q"], out["p"], out["ang"])
    probe.after()  # store of a closed frame is asynchronous
    return first, fig, second, _md_figures(integ), out


io("langevin_load_advance_store", {"mythos_langevin_load": [IN, OUT], "mythos_langevin_advance": [IN, OUT], "mythos_langevin_store": [IN, OUT]},
   _ox_integrator, lambda ctx: _ox_states(), _call_ox_resident, check_default=_recovered)


def _ext_sets(w):
    from mythos_amd.simulators.restraints import (GroupTorque, MovingString, MutualTrap, PointForces, RepulsionSphere, Restraints, SelfTether,
                                                  SumRestraint, Trap)

    _, traj, _, _ = _ox_golden(2)
    x = np.asarray(traj.center[0], dtype=np.float64)
    f = 1.0 if w == "A" else 1.5
    forces = ([0, 15], [[0.0, 0.0, 0.1 * f], [0.0, 0.05, -0.1 * f]])
    rs = Restraints(tethers=[SelfTether([1, 14], 5.0 * f, x[[1, 14]] + 0.05)], sums=[SumRestraint([3, 4], 2.0 * f, x[3] + x[4] + 0.1)],
                    torques=[GroupTorque([5, 6, 9, 10], (0.0, 0.1, 0.3 * f))])
    pf = PointForces([Trap(2, x[2] + (0.1, -0.2, 0.05), 10.0 * f, 1e-3, (1, 0, 0)), MovingString(8, 0.2 * f, 1e-2, (0, 0, 1)),
                      MutualTrap(0, 15, 5.0 * f, 1.0), RepulsionSphere(7, x.mean(0), 0.5, 5.0 * f)])
    return forces, rs, pf


def _install_ext(ctx, w, what=("forces", "restraints", "points")):
    forces, rs, pf = _ext_sets(w)
    if "forces" in what:
        ctx["integ"].set_external_forces(*forces)
    if "restraints" in what:
        ctx["integ"].set_restraints(rs)
    if "points" in what:
        ctx["integ"].set_point_forces(pf)


def _setup_ext(what=("forces", "restraints", "points")):
    ctx = _ox_integrator(dtype=torch.float64)
    _install_ext(ctx, "A", what)
    return ctx


def _call_eval_external(ctx, b, probe):
    plain = ctx["integ"].external_field(b["c"])
    at = ctx["integ"].external_field_at(b["c"], 250.0)
    probe.after()
    return plain, at


io("langevin_eval_external", {"mythos_langevin_eval_external": [IN, OUT], "mythos_langevin_eval_external_at": [IN, OUT]}, _setup_ext,
   lambda ctx: _ox_frames(), _call_eval_external)
for _what, _entry in (("forces", "mythos_langevin_set_external_forces"), ("restraints", "mythos_langevin_set_restraints"),
                      ("points", "mythos_langevin_set_point_forces")):
    setter(f"langevin_{_entry.split('_set_')[1]}", {_entry: [SET]}, lambda: _ox_integrator(dtype=torch.float64), lambda ctx: _ox_frames(),
           _call_eval_external, functools.partial(_install_ext, what=(_what,)))


def _call_init_momenta(ctx, b, probe):
    out = ctx["integ"].init_momenta()
    probe.after()
    return out, ctx["integ"].step


def _install_seed(ctx, w):
    ctx["integ"].set_seed(11 if w == "A" else 0xABCDEF0123)
    ctx["integ"].step = 5 if w == "A" else 12345


def _call_seeded_run(ctx, b, probe):
    """init_momenta is the asynchronous reader of the seed; the short run behind it reads seed and step counter too."""
    integ = ctx["integ"]
    p, ang = integ.init_momenta()
    probe.after()
    rows = integ.run(b["c"], b["q"], p, ang, 4, save_every=2)
    return p.clone(), ang.clone(), rows, integ.step, b


setter("langevin_set_seed_step", {"mythos_langevin_set_seed": [SET], "mythos_langevin_set_step": [SET], "mythos_langevin_init_momenta": [OUT]},
       lambda: _ox_integrator(skin=0.6, every=10), lambda ctx: _ox_states(), _call_seeded_run, _install_seed)


def _umbrella_table(w):
    from mythos_amd.simulators import umbrella as U

    shape = U.reachable_shape(_ops(0))
    return np.ones(shape) if w == "A" else 0.2 + np.random.default_rng(3).random(shape)


def _install_umbrella(ctx, w):
    ctx["integ"].set_umbrella(_ops(0), _umbrella_table(w), segment_steps=3)


def _setup_umbrella():
    ctx = _ox_integrator(dtype=torch.float64, skin=0.6, every=10)
    _install_umbrella(ctx, "B")
    return ctx


def _call_umbrella(ctx, b, probe):
    integ = ctx["integ"]
    integ.load(b["c"], b["q"], b["p"], b["ang"])
    probe.before()
    out = integ.advance_umbrella(4, sample_every=2, proposals=True)  # one synchronisation per segment
    # the decision and commit launches of the last boundary are still queued: the counts wait for the device
    counts = integ.umbrella_counts()
    probe.rearm()
    return out, counts


io("langevin_advance_umbrella", {"mythos_langevin_advance_umbrella": [IN, OUT], "mythos_langevin_umbrella_counts": [GET]}, _setup_umbrella,
   lambda ctx: _ox_states(torch.float64), _call_umbrella)
setter("langevin_set_umbrella", {"mythos_langevin_set_umbrella": [SET]}, lambda: _ox_integrator(dtype=torch.float64, skin=0.6, every=10),
       lambda ctx: _ox_states(torch.float64), _call_umbrella, _install_umbrella,
       note="the launch synchronises (one synchronisation per segment): the setter finds the stream drained, the case checks the stream")


# ====================================================================================================== MARTINI system
def _m_arrays(name):
    s = S.get(name)
    return s, tuple(s[k] for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0"))


def _charges(n, w="A"):
    q = np.zeros(n)
    if w == "A":
        q[0::5], q[1::5] = 1.0, -1.0
    else:
        q[0::3], q[1::3] = 0.5, -0.5
    return q


def _m_system(name="n257", dtype=torch.float64, charged=False):
    from mythos_amd.hip_system import MartiniSystem

    s, ff = _m_arrays(name)
    sysm = MartiniSystem(*ff, dtype=dtype, device=DEV)
    if charged:
        sysm.set_charges(_charges(s["n"]))
    return sysm


def _m_frames(name="n257", dtype=torch.float64, count=2):
    """A: the system's frame (and copies moved rigidly by whole boxes); B: scaled by 1.001, beads moved by up to 0.02 nm."""
    s = S.get(name)
    x, box = np.asarray(s["pos"][0]), np.asarray(s["box"][0])
    rng = np.random.default_rng(5)
    a = np.stack([x + k * box for k in range(count)])
    b = np.stack([1.001 * (x + rng.uniform(-0.02, 0.02, size=x.shape)) for _ in range(count)])
    return {"A": {"pos": _t(a, dtype), "box": _t(np.broadcast_to(box, (count, 3)), dtype)},
            "B": {"pos": _t(b, dtype), "box": _t(np.broadcast_to(1.001 * box, (count, 3)), dtype)}}


def _call_m_energy(ctx, b, probe):
    out = ctx["m"].energy(b["pos"], b["box"], grads=True)
    probe.after()
    return out


def _call_m_param_grads(ctx, b, probe):
    out = ctx["m"].param_grads(b["pos"], b["box"])
    probe.after()
    return out


def _call_m_coulomb(ctx, b, probe):
    out = ctx["m"].coulomb(b["pos"], b["box"], grads=True)
    probe.after()
    return out


CENTER = list(range(0, 40, 3))


def _setup_stress():
    m = _m_system(charged=True)
    fr = _m_frames()["A"]
    m.stress_profile(fr["pos"], fr["box"], 8, center_index=CENTER, by_term=True, check_boxes=False)  # (the centre list is on the device)
    torch.cuda.synchronize()
    return {"m": m}


def _call_m_stress(ctx, b, probe):
    out = ctx["m"].stress_profile(b["pos"], b["box"], 8, center_index=CENTER, by_term=True, check_boxes=False)
    probe.after()
    other = ctx["m"].stress_profile(b["pos"], b["box"], 8, center_index=CENTER[:5], by_term=False, check_boxes=False)  # a new list: waits
    probe.rearm()
    return out, other


io("martini_energy", {"mythos_martini_energy": [IN, OUT]}, lambda: {"m": _m_system()}, lambda ctx: _m_frames(), _call_m_energy)
io("martini_param_grads", {"mythos_martini_param_grads": [IN, OUT]}, lambda: {"m": _m_system()}, lambda ctx: _m_frames(), _call_m_param_grads)
io("martini_coulomb", {"mythos_martini_coulomb": [IN, OUT]}, lambda: {"m": _m_system(charged=True)}, lambda ctx: _m_frames(), _call_m_coulomb)
io("martini_stress_profile", {"mythos_martini_stress_profile": [IN, OUT]}, _setup_stress, lambda ctx: _m_frames(), _call_m_stress)


def _install_m_params(ctx, w):
    s = S.get("n257")
    f = 1.0 if w == "A" else 1.1
    ctx["m"].set_params(sigma=s["sigma"], eps=f * s["eps"], bond_k=f * s["bond_k"], bond_r0=s["bond_r0"], angle_k=f * s["angle_k"], angle_t0=s["angle_t0"])


setter("martini_set_params", {"mythos_martini_set_params": [SET]}, lambda: {"m": _m_system()}, lambda ctx: _m_frames(), _call_m_energy, _install_m_params)
setter("martini_set_charges", {"mythos_martini_set_charges": [SET]}, lambda: {"m": _m_system()}, lambda ctx: _m_frames(), _call_m_coulomb,
       lambda ctx, w: ctx["m"].set_charges(_charges(257, w)))


# ================================================================================ MARTINI integrator, single and ensemble
def _m_wrapped(name):
    """Positions inside the box (the integrator's restraints and pull groups take coordinates as stored)."""
    s = S.get(name)
    return np.asarray(s["pos"][0]) - np.asarray(s["shift"]) * np.asarray(s["box"][0]), np.asarray(s["box"][0])


def _m_integrator(name="md37", dtype=torch.float32, charged=False, inner=False, dt=0.002, seed=0xABCDEF012345):
    from mythos_amd.hip_system import MartiniLangevinIntegrator

    m = _m_system(name, dtype, charged)
    integ = MartiniLangevinIntegrator(m, dt=dt, kT=KT_M, gamma=2.0, mass=S.get(name)["mass"], seed=seed)
    integ.set_neighbor_policy(0.25, 2)
    if inner:
        integ.set_inner_list(0.1, 2)
    return {"m": m, "integ": integ, "box": _m_wrapped(name)[1]}


def _m_states(name="md37", dtype=torch.float32, n_rep=0):
    x, box = _m_wrapped(name)
    n = x.shape[0]
    out = {}
    for k, w in enumerate("AB"):
        g = torch.Generator().manual_seed(200 + k)
        lead = (n_rep,) if n_rep else ()
        v = 0.2 * torch.randn(*lead, n, 3, generator=g, dtype=torch.float64)
        pos = np.broadcast_to(x, (*lead, n, 3)) + (0.0 if w == "A" else np.random.default_rng(9).uniform(-0.02, 0.02, size=(*lead, n, 3)))
        out[w] = {"pos": _t(pos, dtype), "vel": v.to(DEV, dtype).contiguous()}
    return out


def _m_rows(integ, pruned=False):
    """(rows with the places behind each row's length set to -1 - they hold whatever an earlier build left -, lengths)."""
    rows, lens = integ.rows(pruned=pruned)
    return np.where(np.arange(rows.shape[1])[None, :] < lens[:, None], rows, -1), lens


def _m_figures(integ):
    ms = integ.last_kernel_ms()
    return {"recoveries": integ.last_recoveries(), "rebuilds": integ.last_rebuilds(), "step": integ.step, "launches": ms["launches"],
            "samples": ms["samples"], "stats": integ.neighbor_stats(), "rows": _m_rows(integ), "box": integ.box, "last_boxes": integ.last_boxes}


def _call_m_run(ctx, b, probe):
    integ = ctx["integ"]
    integ.set_timing(2)
    probe.before()
    rows = integ.run(b["pos"], b["vel"], ctx["box"], 8, save_every=4, want_energy=True)
    fig = _m_figures(integ)
    pruned = _m_rows(integ, pruned=True)
    probe.rearm()
    plain = integ.run(b["pos"], b["vel"], ctx["box"], 6, save_every=3, want_energy=False)
    return rows, fig, pruned, plain, _m_figures(integ), b


_M_GETTERS = {"mythos_martini_langevin_last_recoveries": [GET], "mythos_martini_langevin_last_rebuilds": [GET],
              "mythos_martini_langevin_get_step": [GET], "mythos_martini_langevin_last_kernel_ms": [GET],
              "mythos_martini_langevin_set_timing": [SET], "mythos_martini_langevin_neighbor_stats": [GET],
              "mythos_martini_langevin_get_rows": [GET], "mythos_martini_langevin_get_box": [GET], "mythos_martini_langevin_last_boxes": [GET]}
io("martini_run", {"mythos_martini_langevin_run": [IN, OUT], **_M_GETTERS}, lambda: _m_integrator(charged=True, inner=True),
   lambda ctx: _m_states(), _call_m_run)


def _call_m_resident(ctx, b, probe):
    integ = ctx["integ"]
    v0 = integ.init_velocities()
    integ.load(b["pos"], b["vel"], ctx["box"])
    probe.after()  # init_velocities and a single copy's load are asynchronous
    first = integ.advance(5, save_every=0)
    probe.rearm()
    second = integ.advance(6, save_every=3, want_energy=True)
    probe.rearm()
    stats, rows = integ.neighbor_stats(), _m_rows(integ)
    p = integ.pressure()  # synchronises the stream
    probe.rearm()
    out = {k: torch.empty_like(v) for k, v in b.items()}
    integ.store(out["pos"], out["vel"])
    return v0, first, second, stats, rows, p, out, integ.step


io("martini_load_advance_store", {"mythos_martini_langevin_init_velocities": [OUT], "mythos_martini_langevin_load": [IN, OUT],
                                  "mythos_martini_langevin_advance": [IN, OUT], "mythos_martini_langevin_store": [IN, OUT],
                                  "mythos_martini_langevin_pressure": [IN, OUT]},
   _m_integrator, lambda ctx: _m_states(), _call_m_resident)

BAROSTAT = dict(kind="c-rescale", coupling="semiisotropic", ref_p=(1.0, 1.0), compressibility=(1e-7, 1e-7), tau_p=0.5, every=3)


def _setup_m_barostat():
    ctx = _m_integrator("n257", torch.float64, dt=0.001)
    ctx["integ"].set_barostat(**BAROSTAT)
    return ctx


def _call_m_chunked(ctx, b, probe):
    """One chunked advance: a handful of steps with coupling events inside the call."""
    integ = ctx["integ"]
    integ.load(b["pos"], b["vel"], ctx["box"])
    probe.before()
    rows = integ.advance(7, save_every=3, want_energy=True)
    fig = {"box": integ.box, "last_boxes": integ.last_boxes, "step": integ.step, "recoveries": integ.last_recoveries()}
    probe.rearm()
    p = integ.pressure()
    out = {k: torch.empty_like(v) for k, v in b.items()}
    integ.store(out["pos"], out["vel"])
    return rows, fig, p, out


io("martini_advance[barostat]", {"mythos_martini_langevin_advance": [IN, OUT], "mythos_martini_langevin_get_box": [GET],
                                 "mythos_martini_langevin_last_boxes": [GET]},
   _setup_m_barostat, lambda ctx: _m_states("n257", torch.float64), _call_m_chunked)


def _install_barostat(ctx, w):
    ctx["integ"].set_barostat(**(BAROSTAT if w == "B" else dict(kind=None)))


def _call_m_short_run(ctx, b, probe):
    integ = ctx["integ"]
    probe.before()
    rows = integ.run(b["pos"], b["vel"], ctx["box"], 6, save_every=3)
    return rows, integ.box, integ.last_boxes, b


setter("martini_set_barostat", {"mythos_martini_langevin_set_barostat": [SET]}, lambda: _m_integrator("n257", torch.float64, dt=0.001),
       lambda ctx: _m_states("n257", torch.float64), _call_m_short_run, _install_barostat,
       note="host numbers; the launch (run) synchronises, so the case checks the stream, not an overlap")


def _m_restraints(w, n_rep=1):
    from mythos_amd.simulators.martini_restraints import MartiniRestraints, PositionRestraint, PullCoordinate, PullGroup

    x, _ = _m_wrapped("n257")
    f = 1.0 if w == "A" else 1.3
    init = tuple(0.4 + 0.01 * r for r in range(n_rep)) if n_rep > 1 else 0.4
    return MartiniRestraints(
        position=[PositionRestraint(index=i, k=(900.0 * f, 400.0, 250.0), reference=tuple(x[i] + 0.05)) for i in range(3)],
        pulls=[PullCoordinate(group_a=PullGroup(members=tuple(range(4, 9))), group_b=PullGroup(members=tuple(range(9, 14))), geometry="direction",
                              vec=(1.0, 2.0, -1.0), k=800.0 * f, init=init, periodic=False),
               PullCoordinate(group_a=PullGroup(members=(50, 51)), group_b=PullGroup(members=(60,)), kind="constant-force", geometry="distance",
                              k=75.0 * f, periodic=False)])


def _call_m_eval_external(ctx, b, probe):
    integ = ctx["integ"]
    rows = torch.stack([b["pos"], b["pos"] + 0.01])
    xi = integ.pull_values(rows)  # (first: the scratch rows the two entries share only grow, and growing waits for the device)
    field = integ.external_field(b["pos"], step=40.0)
    probe.after()
    return field, xi


def _setup_m_external():
    ctx = _m_integrator("n257", torch.float64, dt=0.001)
    ctx["integ"].set_restraints(_m_restraints("A"), box=ctx["box"])
    return ctx


def _m_pos(n_rep=0):
    return {w: {"pos": v["pos"]} for w, v in _m_states("n257", torch.float64, n_rep).items()}


io("martini_eval_external", {"mythos_martini_langevin_eval_external": [IN, OUT], "mythos_martini_langevin_pull_values": [IN, OUT]},
   _setup_m_external, lambda ctx: _m_pos(), _call_m_eval_external)
setter("martini_set_restraints", {"mythos_martini_langevin_set_restraints": [SET]}, lambda: _m_integrator("n257", torch.float64, dt=0.001),
       lambda ctx: _m_pos(), _call_m_eval_external, lambda ctx, w: ctx["integ"].set_restraints(_m_restraints(w), box=ctx["box"]))

N_REP = 3
SEEDS = [0xABCDEF012345, 7, 2**63 + 11]


def _m_ensemble(kTs, dtype=torch.float64, seeds=SEEDS):
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    m = _m_system("n257", dtype)
    integ = MartiniEnsembleIntegrator(m, dt=0.001, kT=list(kTs), gamma=2.0, mass=S.get("n257")["mass"], seeds=list(seeds))
    integ.set_neighbor_policy(0.25, 2)
    return {"m": m, "integ": integ, "box": np.broadcast_to(_m_wrapped("n257")[1], (N_REP, 3)).copy()}


HOT = KT_M * np.array([1.0, 1.02, 1.04])  # close rungs: exchanges are accepted


def _setup_exchange():
    ctx = _m_ensemble(HOT)
    ctx["integ"].set_exchange(2, seed=99)
    return ctx


def _call_m_exchange(ctx, b, probe):
    integ = ctx["integ"]
    v0 = integ.init_velocities()
    probe.after()
    integ.load(b["pos"], b["vel"], ctx["box"])  # an ensemble's load waits for the stream (the staging buffer of its replica table)
    probe.rearm()
    rows = integ.advance(7, save_every=2, want_energy=True)
    log = {"ladder": integ.ladder, "last_ladder": integ.last_ladder, "last_exchanges": integ.last_exchanges, "counts": integ.exchange_counts(),
           "box": integ.box, "last_boxes": integ.last_boxes, "step": integ.step}
    probe.rearm()
    p = integ.pressure()
    out = {k: torch.empty_like(v) for k, v in b.items()}
    integ.store(out["pos"], out["vel"])
    return v0, rows, log, p, out


def _exchanged(ctx):
    assert ctx["integ"].exchange_counts()[0].sum() >= 3, "no exchange event inside the call: not the scenario intended"


io("martini_advance[temperature exchange]",
   {"mythos_martini_langevin_advance": [IN, OUT], "mythos_martini_langevin_pressure_ensemble": [IN, OUT], "mythos_martini_langevin_get_ladder": [GET],
    "mythos_martini_langevin_last_ladder": [GET], "mythos_martini_langevin_last_exchanges": [GET], "mythos_martini_langevin_exchange_counts": [GET],
    "mythos_martini_langevin_get_box_ensemble": [GET], "mythos_martini_langevin_last_boxes": [GET], "mythos_martini_langevin_init_velocities": [OUT]},
   _setup_exchange, lambda ctx: _m_states("n257", torch.float64, N_REP), _call_m_exchange, check_default=_exchanged)


def _setup_windows(every=2):
    ctx = _m_ensemble([KT_M] * N_REP)
    if every:
        ctx["integ"].set_window_exchange(every, seed=77)
    ctx["integ"].set_restraints(_m_restraints("A", N_REP), box=ctx["box"])
    return ctx


def _call_m_window_exchange(ctx, b, probe):
    integ = ctx["integ"]
    integ.load(b["pos"], b["vel"], ctx["box"])
    probe.rearm()
    rows = integ.advance(7, save_every=2, want_energy=False)
    log = {"windows": integ.windows, "last_windows": integ.last_windows, "last": integ.last_window_exchanges,
           "counts": integ.window_exchange_counts(), "step": integ.step}
    probe.rearm()
    field = integ.external_field(b["pos"], step=3.0)
    probe.after()
    return rows, log, field


def _windows_tried(ctx):
    assert ctx["integ"].window_exchange_counts()[0].sum() >= 3, "no window-exchange event inside the call: not the scenario intended"


io("martini_advance[window exchange]",
   {"mythos_martini_langevin_advance": [IN, OUT], "mythos_martini_langevin_get_windows": [GET], "mythos_martini_langevin_last_windows": [GET],
    "mythos_martini_langevin_last_window_exchanges": [GET], "mythos_martini_langevin_window_exchange_counts": [GET],
    "mythos_martini_langevin_eval_external": [IN, OUT]},
   _setup_windows, lambda ctx: _m_states("n257", torch.float64, N_REP), _call_m_window_exchange, check_default=_windows_tried)


def _call_m_init_velocities(ctx, b, probe):
    out = ctx["integ"].init_velocities()
    probe.after()
    return out, ctx["integ"].ladder, ctx["integ"].step


setter("martini_set_ladder", {"mythos_martini_langevin_set_ladder": [SET], "mythos_martini_langevin_get_ladder": [GET]},
       lambda: _m_ensemble(KT_M * np.array([1.0, 1.3, 1.7])), lambda ctx: {"A": {}, "B": {}}, _call_m_init_velocities,
       lambda ctx, w: ctx["integ"].set_ladder([0, 1, 2] if w == "A" else [2, 0, 1]))
setter("martini_restart", {"mythos_martini_langevin_restart": [SET]}, lambda: _m_ensemble(HOT), lambda ctx: {"A": {}, "B": {}},
       _call_m_init_velocities, lambda ctx, w: ctx["integ"].restart(SEEDS if w == "A" else [5, 6, 2**40 + 1], 0 if w == "A" else 777))


def _call_m_field(ctx, b, probe):
    out = ctx["integ"].external_field(b["pos"], step=3.0)
    probe.after()
    return out, ctx["integ"].windows


setter("martini_set_windows", {"mythos_martini_langevin_set_windows": [SET], "mythos_martini_langevin_get_windows": [GET]}, _setup_windows,
       lambda ctx: _m_pos(N_REP), _call_m_field, lambda ctx, w: ctx["integ"].set_windows([0, 1, 2] if w == "A" else [1, 2, 0]))


def _call_m_ensemble_run(ctx, b, probe):
    integ = ctx["integ"]
    probe.before()
    rows = integ.run(b["pos"], b["vel"], ctx["box"], 6, save_every=3)
    return rows, integ.last_exchanges, integ.last_window_exchanges, b


setter("martini_set_exchange", {"mythos_martini_langevin_set_exchange": [SET]}, lambda: _m_ensemble(HOT),
       lambda ctx: _m_states("n257", torch.float64, N_REP), _call_m_ensemble_run,
       lambda ctx, w: ctx["integ"].set_exchange(2 if w == "A" else 3, seed=99),
       note="host numbers; the launch (run) synchronises, so the case checks the stream, not an overlap")
setter("martini_set_window_exchange", {"mythos_martini_langevin_set_window_exchange": [SET]}, lambda: _setup_windows(every=0),
       lambda ctx: _m_states("n257", torch.float64, N_REP), _call_m_ensemble_run,
       lambda ctx, w: ctx["integ"].set_window_exchange(2 if w == "A" else 3, seed=77),
       note="host numbers; the launch (run) synchronises, so the case checks the stream, not an overlap")


# ==================================================================================== stored-frame observables, statistics
def _geometry_set():
    from mythos_amd.observables.martini_geometry import GeometrySet

    s = S.get("n257")
    return GeometrySet(257, [2, 3], [np.asarray(s["bonds"][:40]), np.asarray(s["angles"][:30])], DEV)


def _call_geometry(ctx, b, probe):
    out = ctx["g"].eval(b["pos"], b["box"])
    probe.after()
    return out


io("martini_obs_eval", {"mythos_martini_obs_eval": [IN, OUT]}, lambda: {"g": _geometry_set()}, lambda ctx: _m_frames(count=3), _call_geometry)


def _w1_inputs(ctx):
    g = torch.Generator().manual_seed(4)
    out = {}
    for w in "AB":
        out[w] = {"block": torch.rand(6 * 5 + 6 * 2, generator=g, dtype=torch.float64).to(DEV),
                  "weights": torch.softmax(torch.randn(6, generator=g, dtype=torch.float64), 0).to(DEV)}
    return out


def _call_w1(ctx, b, probe):
    from mythos_amd.observables.wasserstein import W1Plan

    probe.before()
    plan = W1Plan(b["block"], [6, 6], [5, 2], [ctx["ref"][:9], ctx["ref"][9:]], [None, ctx["ref_w"]])  # synchronises the stream
    probe.rearm()
    uniform = plan.eval(None, True)
    weighted = plan.eval(b["weights"], True)
    probe.after()
    ctx["plan"] = plan  # (alive until the stream has run)
    return uniform, weighted


def _setup_w1():
    g = torch.Generator().manual_seed(8)
    w = torch.rand(7, generator=g, dtype=torch.float64)
    return {"ref": torch.rand(16, generator=g, dtype=torch.float64).to(DEV), "ref_w": (w / w.sum()).to(DEV)}


io("w1_plan_and_eval", {"mythos_w1_plan_create": [IN, OUT], "mythos_w1_eval": [IN, OUT]}, _setup_w1, _w1_inputs, _call_w1)


def _membrane_set():
    from mythos_amd.observables.membrane import MembraneSet

    x, _ = np.asarray(S.get("n257")["pos"][0]), None
    order = np.argsort(x[:, 2])  # lipids of four beads each, half of them from the low and half from the high end in z
    beads = np.concatenate([order[:16], order[-16:]])
    return MembraneSet(257, np.arange(0, 33, 4), beads, beads[::4], np.arange(8), DEV)


def _call_membrane(ctx, b, probe):
    out = ctx["mem"].eval(b["pos"], b["box"], want_leaflets=True)
    probe.after()
    return out


io("membrane_eval", {"mythos_membrane_eval": [IN, OUT]}, lambda: {"mem": _membrane_set()}, lambda ctx: _m_frames(count=3), _call_membrane)


def _rdf_set():
    from mythos_amd.observables.rdf import _RdfSet

    a, b = np.arange(0, 100), np.arange(60, 257)
    return _RdfSet(257, [(a, b), (a, a)], None, 16, 1.1, "xyz", DEV)


def _call_rdf(ctx, b, probe):
    out = ctx["rdf"].launch(b["pos"], b["box"])
    probe.after()
    return out


io("rdf_eval", {"mythos_rdf_eval": [IN, OUT]}, lambda: {"rdf": _rdf_set()}, lambda ctx: _m_frames(count=3), _call_rdf)

_I64P = C.POINTER(C.c_int64)


def _series_inputs(ctx):
    g = torch.Generator().manual_seed(21)
    return {w: {"x": torch.randn(90, 2, generator=g, dtype=torch.float64).cumsum(0).to(DEV).contiguous()} for w in "AB"}


def _call_timeseries(ctx, b, probe):
    lib = _lib.load()
    off = np.ascontiguousarray([0, 40, 90], dtype=np.int64)
    off_d = ctx["off_d"]
    mean, var = (torch.empty(2, 2, dtype=torch.float64, device=DEV) for _ in range(2))
    out = torch.empty(2, 2, 12, dtype=torch.float64, device=DEV)
    head = (_lib.ptr(b["x"]), 90, 2, 2, off.ctypes.data_as(_I64P), _lib.ptr(off_d))
    st = _lib.stream(torch.device(DEV))
    _lib.check(lib.mythos_timeseries_moments(*head, _lib.ptr(mean), _lib.ptr(var), 0, st), "timeseries_moments")
    _lib.check(lib.mythos_timeseries_autocorr(*head, _lib.ptr(mean), _lib.ptr(var), 1, 12, _lib.ptr(out), 0, st), "timeseries_autocorr")
    probe.after()
    return mean, var, out


io("timeseries", {"mythos_timeseries_moments": [IN, OUT], "mythos_timeseries_autocorr": [IN, OUT]},
   lambda: {"off_d": torch.tensor([0, 40, 90], dtype=torch.int64, device=DEV)}, _series_inputs, _call_timeseries,
   note="through ctypes: the one Python caller (statistical_inefficiency) reads the series back to the host first")

MB_N, MB_K, MB_BOOT = 60, 3, 4
MB_NK = np.array([20, 25, 15], dtype=np.int64)


def _mbar_table(w):
    t = np.zeros((MB_K, 1, 4))
    t[:, 0, 1] = 800.0 if w == "A" else 600.0
    t[:, 0, 2] = [0.4, 0.5, 0.6]
    return t


def _mbar_install(ctx, w):
    from mythos_amd.observables.mbar import _MbarPlan

    if "plan" not in ctx:
        ctx["plan"] = _MbarPlan(MB_N, MB_K, DEV)
    if w == "A":
        ctx["plan"].set_windows(_mbar_table("A"), np.full(MB_K, KT_M), MB_NK, ctx["xi"])
    else:
        ctx["plan"].set_matrix(ctx["u_kn"], MB_NK)


def _setup_mbar(install=True):
    g = torch.Generator().manual_seed(31)
    ctx = {"xi": (0.5 + 0.05 * torch.randn(MB_N, 1, generator=g, dtype=torch.float64)).to(DEV).contiguous(),
           "u_kn": (2.0 * torch.rand(MB_K, MB_N, generator=g, dtype=torch.float64)).to(DEV).contiguous(),
           "order": torch.randperm(MB_N, generator=g).to(DEV), "seg": torch.tensor([0, 20, 45, 60], dtype=torch.int64, device=DEV),
           "mult": torch.randint(0, 3, (MB_BOOT, MB_N), generator=g, dtype=torch.int32).to(torch.uint16).to(DEV).contiguous(),
           "delta": (0.05 * torch.randn(MB_BOOT, MB_K, generator=g, dtype=torch.float64)).to(DEV).contiguous()}
    if install:
        _mbar_install(ctx, "A")
        ctx["xi_buf"] = ctx["xi"]  # BORROWED by the handle: the case writes its input set into this very tensor
    return ctx


def _mbar_inputs(ctx):
    g = torch.Generator().manual_seed(32)
    out = {}
    for w in "AB":
        out[w] = {"xi": (0.5 + 0.05 * torch.randn(MB_N, 1, generator=g, dtype=torch.float64)).to(DEV).contiguous(),
                  "f": torch.cat([torch.zeros(1, dtype=torch.float64), 0.3 * torch.randn(MB_K - 1, generator=g, dtype=torch.float64)]).to(DEV),
                  "v": torch.rand(MB_N, generator=g, dtype=torch.float64).to(DEV)}
    return out


def _call_mbar(ctx, b, probe):
    plan = ctx["plan"]
    ctx["xi_buf"].copy_(b["xi"])  # on the stream: the borrowed tensor takes the input set behind the delay
    f = b["f"].clone()
    delta = torch.empty(1, dtype=torch.float64, device=DEV)
    plan.iterate(f, 3, delta)
    lw = plan.log_weights(f)
    binned = plan.binned_sum(ctx["seg"], ctx["order"], lw, b["v"], 0.0)
    gram = plan.gram(f)
    moments = plan.segment_moments(f, ctx["seg"], ctx["order"], b["v"])
    cols = plan.boot_colsums(f, ctx["delta"], ctx["mult"])
    boot = plan.boot_binned(f, ctx["delta"], ctx["mult"], ctx["seg"], ctx["order"], b["v"][:, None].contiguous(), 0.0)
    probe.after()
    return f, delta, lw, binned, gram, moments, cols, boot


io("mbar", {f"mythos_mbar_{k}": [IN, OUT] for k in ("iterate", "log_weights", "binned_sum", "gram", "segment_moments", "boot_colsums", "boot_binned")},
   _setup_mbar, _mbar_inputs, _call_mbar)


def _call_mbar_weights(ctx, b, probe):
    out = ctx["plan"].log_weights(b["f"])
    probe.after()
    return out


setter("mbar_set_windows_matrix", {"mythos_mbar_set_windows": [SET], "mythos_mbar_set_matrix": [SET]}, lambda: _setup_mbar(install=False),
       lambda ctx: {w: {"f": v["f"]} for w, v in _mbar_inputs(ctx).items()}, _call_mbar_weights, _mbar_install)


# ================================================================================================================ the tests
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_inputs_and_outputs_are_ordered_on_the_stream(case):
    SO.in_out(case)
    ms, ref = SO.HOST_MS[case.name]
    print(f"  {case.name}: host time of the covered calls {ms:.2f} ms behind the delay, {ref:.2f} ms on the default stream")


@pytest.mark.parametrize("case", SET_CASES, ids=repr)
def test_a_setter_does_not_reach_a_launch_queued_before_it(case):
    SO.set_hazard(case)


def test_two_oxdna_systems_on_two_streams():
    """"handles are independent: one handle per thread / stream": two systems, each behind its own delay on its own stream,
    the calls interleaved from one host thread; each handle's results are its solo default-stream results."""
    sx, sy = _ox_system(2), _ox_system(3)
    fx, fy = _ox_frames(2, count=3), _ox_frames(3, count=3)
    want_x = [t.cpu() for t in sx.energy(fx["A"]["c"], fx["A"]["q"], grads=True, param_grads=True)]
    want_y = [t.cpu() for t in sy.energy(fy["A"]["c"], fy["A"]["q"], grads=True, param_grads=True)]
    assert not torch.equal(want_x[0], sx.energy(fx["B"]["c"], fx["B"]["q"])[0].cpu())
    assert not torch.equal(want_y[0], sy.energy(fy["B"]["c"], fy["B"]["q"])[0].cpu())
    bx, by = {k: v.clone() for k, v in fx["B"].items()}, {k: v.clone() for k, v in fy["B"].items()}
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        e1, e2 = SO.arm(s1), SO.arm(s2)
        got_x, got_y = [], []
        for rnd in range(2):
            with torch.cuda.stream(s1):
                if rnd == 0:
                    for k in bx:
                        bx[k].copy_(fx["A"][k])
                got_x.append([t.clone() for t in sx.energy(bx["c"], bx["q"], grads=True, param_grads=True)])
            with torch.cuda.stream(s2):
                if rnd == 0:
                    for k in by:
                        by[k].copy_(fy["A"][k])
                got_y.append([t.clone() for t in sy.energy(by["c"], by["q"], grads=True, param_grads=True)])
        assert SO.pending(e1) and SO.pending(e2)
    finally:
        s1.synchronize()
        s2.synchronize()
    for got, want in ((got_x, want_x), (got_y, want_y)):
        for rnd in got:
            assert all(torch.equal(a.cpu(), b) for a, b in zip(rnd, want))


def test_two_martini_integrators_on_two_streams():
    """Two integrators on two systems (md37 in fp32, n257 in fp64), load / advance / store interleaved from one host thread,
    each on its own stream behind its own delay: the states and rows of each are those of its solo default-stream run."""
    def solo(ctx, st):
        integ = ctx["integ"]
        b = {k: v.clone() for k, v in st.items()}
        integ.load(b["pos"], b["vel"], ctx["box"])
        rows = integ.advance(6, save_every=3)
        integ.store(b["pos"], b["vel"])
        torch.cuda.synchronize()
        return [t.cpu() for t in (*rows, b["pos"], b["vel"])]

    make = (lambda: _m_integrator("md37", torch.float32), lambda: _m_integrator("n257", torch.float64, dt=0.001))
    states = (_m_states("md37", torch.float32), _m_states("n257", torch.float64))
    want = [solo(m(), st["A"]) for m, st in zip(make, states)]
    other = [solo(m(), st["B"]) for m, st in zip(make, states)]
    assert all(not torch.equal(a[-2], b[-2]) for a, b in zip(want, other))
    ctxs = [m() for m in make]
    bufs = [{k: v.clone() for k, v in st["B"].items()} for st in states]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rows = [None, None]
    try:
        events = [SO.arm(s) for s in streams]
        for ctx, b, st, s in zip(ctxs, bufs, states, streams):
            with torch.cuda.stream(s):
                for k in b:
                    b[k].copy_(st["A"][k])
                ctx["integ"].load(b["pos"], b["vel"], ctx["box"])
        assert all(SO.pending(e) for e in events)
        for k, (ctx, s) in enumerate(zip(ctxs, streams)):
            with torch.cuda.stream(s):
                rows[k] = ctx["integ"].advance(6, save_every=3)
        for ctx, b, s in zip(ctxs, bufs, streams):
            with torch.cuda.stream(s):
                ctx["integ"].store(b["pos"], b["vel"])
    finally:
        for s in streams:
            s.synchronize()
    for k in range(2):
        got = [t.cpu() for t in (*rows[k], bufs[k]["pos"], bufs[k]["vel"])]
        assert all(torch.equal(a, b) for a, b in zip(got, want[k])), k
