"""Scheduled oxDNA list rebuilds that FILTER candidate rows (mythos_amd/csrc/neighbors.hip: filter_rows_kernel; the
schedule: mythos_amd/csrc/row_filter_plan.h) against the full builder: ``rows_filter`` = 1 (the default) and 0 (every
rebuild by build_rows_cells_kernel, the A/B reference) must leave the same rows, entry for entry, and the same state, bit
for bit - through wide builds, filters, the carry-over between two ``advance`` calls, candidates gone stale (a halt and a
recovery at the frame the scheduled build would have used), a candidate stride that is too short, a new neighbour
policy and a new state.  The filtered rows are also held to the brute-force contract (tests/oxdna_rows_ref.py) at the
frame they were built from.

Systems: the cases of tests/oxdna_rows_ref.py that take the cell builder - 512 to 576 nucleotides (the smallest it
accepts), workgroups full and not, free space and a periodic box crossed at every face, rows beyond a stride of 64,
oxNA with non-zero slack - in both precisions, at 8 and 16 lanes per nucleotide of the step kernel.  The periodic box
(13 x 39 x 13) holds three cells of the list range 3.9 per edge and of nothing wider than 4.33: those cases run with a
candidate margin of 0.4, the others with 1.0.
"""

import dataclasses as dc
import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from tests import oxdna_rows_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"f64": torch.float64, "f32": torch.float32}
DTYPES = ("f64", "f32")
KT = 296.15 * 0.1 / 300.0
DT_ROWS = 1e-4   # the perturbed frames are strained: steps short enough to stay finite (tests/test_gpu_oxdna_rows.py)
DT_THERMAL = 0.005
EVERY = 5        # steps per list rebuild
CAND_EVERY = 3   # rebuilds per wide build: builds before steps 0, 15, 30 are wide, the others filter only
CASES = R.CELL_CASES + (R.LONG_ROW_CASE, "hybrid-tiled")
MARGIN_MILLI = {name: 400 if name in R.PERIODIC_CELL_CASES else 1000 for name in CASES}


def _filter_applies(cs, margin_milli):
    """rows_filter_applies (neighbors.hip): the cell builder serves the list range and the candidates' range."""
    return R.uses_cells(cs.n, cs.box, cs.r_list) and R.uses_cells(cs.n, cs.box, cs.r_list + 1e-3 * margin_milli)


class _switches:
    """The three debug keys for the length of a with block (rows_filter goes back to its default, 1)."""

    def __init__(self, rows_filter, cand_every=CAND_EVERY, margin_milli=0):
        self.v = dict(rows_filter=rows_filter, rows_cand_every=cand_every, rows_cand_margin=margin_milli)

    def __enter__(self):
        for k, v in self.v.items():
            _lib.debug_set(k, v)

    def __exit__(self, *exc):
        _lib.debug_set("rows_filter", 1)
        _lib.debug_set("rows_cand_every", 0)
        _lib.debug_set("rows_cand_margin", 0)
        assert _lib.debug_get("rows_filter") == 1 and _lib.debug_get("rows_cand_every") == 0 and _lib.debug_get("rows_cand_margin") == 0


def _integrator(cs, dtype, dt, seed=17, skin=None, every=EVERY):
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    s = OxdnaSystem(cs.model, cs.top.seq, cs.top.is_end, cs.top.bonded_neighbors, box=cs.box, dtype=TORCH[dtype], is_rna=cs.is_rna)
    s.set_params(torch.as_tensor(R.flat_for(cs.model)[0]))
    integ = LangevinIntegrator(s, dt=dt, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=seed)
    integ.set_neighbor_policy(r_cut=cs.r_cut, skin=cs.skin if skin is None else skin, every=every)
    return s, integ


def _start(cs, s, integ, dtype):
    to = dict(dtype=TORCH[dtype], device=s.device)
    c, q = torch.as_tensor(cs.c, **to).contiguous(), torch.as_tensor(cs.q, **to).contiguous()
    p, L = integ.init_momenta()
    return c, q, p, L


def _result(s, state):
    rows, ln, close = s.rows()
    return dict(state=[t.clone() for t in state], rows=np.array(rows), ln=np.array(ln), close=np.array(close))


def _assert_same(a, b, what):
    assert a["rows"].shape == b["rows"].shape, (what, a["rows"].shape, b["rows"].shape)
    assert (a["ln"] == b["ln"]).all() and (a["close"] == b["close"]).all(), what
    used = np.arange(a["rows"].shape[1])[None, :] < a["ln"][:, None]
    differ = np.nonzero(((a["rows"] != b["rows"]) & used).any(1))[0]
    assert differ.size == 0, (what, "rows of", differ[:8].tolist())
    for x, y, name in zip(a["state"], b["state"], ("centres", "quaternions", "momenta", "angular momenta")):
        assert torch.equal(x, y), (what, name, float((x - y).abs().max()))


def _advance(cs, dtype, rows_filter, plan, *, dt=DT_ROWS, margin_milli=None, cand_every=CAND_EVERY, seed=17):
    """load; advance(n) for n in plan; store - the state, the rows, and the recoveries and rebuilds of each call."""
    margin_milli = MARGIN_MILLI.get(cs.name, 1000) if margin_milli is None else margin_milli
    assert _filter_applies(cs, margin_milli)
    with _switches(rows_filter, cand_every, margin_milli):
        s, integ = _integrator(cs, dtype, dt, seed)
        state = _start(cs, s, integ, dtype)
        integ.load(*state)
        counts = []
        for n in plan:
            integ.advance(n)
            counts.append((integ.last_recoveries(), integ.last_rebuilds()))
        integ.store(*state)
        out = _result(s, state)
    out["counts"] = counts
    return out


def _assert_contract(rows, must, may, what):
    gc, gf, bad = R.decode(*rows)
    assert not bad, (what, bad[:4])
    listed = int(may.listed.sum()) // 2
    assert int(may.band.sum()) // 2 <= R.BAND_CAP * listed and int(must.band.sum()) // 2 <= R.BAND_CAP * listed  # (of the inputs)
    msgs = R.contract_failures(gc, gf, must, may)
    assert not msgs, what + "\n" + "\n".join(msgs)
    assert gc.any()


# ---- 1: rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_filtered_rows_and_state_equal_the_full_builders(name, dtype, md_lanes):
    """41 steps in two calls: builds before steps 0, 5, ... 40, wide before 0, 15 and 30, the second call starting three
    steps into an interval whose candidates the first call left."""
    cs = R.case(name)
    plan = (13, 28)
    on, off = _advance(cs, dtype, 1, plan), _advance(cs, dtype, 0, plan)
    assert on["counts"] == off["counts"] == [(0, 2), (0, 6)], (on["counts"], off["counts"])
    _assert_same(on, off, f"{name} {dtype} lanes {md_lanes}")
    if name == R.LONG_ROW_CASE:
        assert on["rows"].shape[1] > 64 and int(on["ln"].max()) > 64


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_filtered_rows_meet_the_contract_at_their_frame(name, dtype):
    """The recipe of test_gpu_oxdna_rows.py's third build: eleven steps, builds before steps 0, 5 and 10 - the third a
    filter of the candidates of the first -, the rows the run leaves are those of saved frame 9."""
    cs = R.case(name)
    margin = MARGIN_MILLI[name]
    assert _filter_applies(cs, margin)
    with _switches(1, CAND_EVERY, margin):
        s, integ = _integrator(cs, dtype, DT_ROWS)
        c, q, p, L = _start(cs, s, integ, dtype)
        tc, tq, _ = integ.run(c, q, p, L, 2 * EVERY + 1, save_every=1)
        assert integ.last_rebuilds() == 2 and integ.last_recoveries() == 0
        rows = s.rows()
    at = 2 * EVERY - 1
    fc, fq = tc[at].cpu().numpy().astype(np.float64), tq[at].cpu().numpy().astype(np.float64)
    assert np.abs(fc - cs.c).max() > 10 * R.BAND[dtype]  # (another frame than the wide build's)
    must, may = cs.reference(dtype, c=fc, q=fq)
    _assert_contract(rows, must, may, f"filtered third build {name} {dtype}")


# ---- 2: candidates that no longer vouch -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _relaxed_bundle():
    """bundle512's system at the generator's own frame (not strained: it takes the thermal time step)."""
    from mythos_amd.utils import generators

    _, c, q = generators.duplex_bundle(32, 8, spacing=3.2)
    return dc.replace(R.case("bundle512"), c=np.ascontiguousarray(c, dtype=np.float64), q=np.ascontiguousarray(q, dtype=np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_candidates_halt_and_recover_on_the_same_trajectory(dtype, md_lanes):
    """Thermal steps, a margin of 0.05: a wide build every 40 steps, and centres (thermal speed ~0.3: 0.0015 a step) more
    than 0.025 from the candidate frame within some twenty.  The filter that finds them there halts the launches behind
    it; the recovery builds at the frame the scheduled build would have used, so the trajectory is the full builder's."""
    cs = _relaxed_bundle()
    on = _advance(cs, dtype, 1, (60,), dt=DT_THERMAL, margin_milli=50, cand_every=8)
    off = _advance(cs, dtype, 0, (60,), dt=DT_THERMAL, margin_milli=50, cand_every=8)
    assert off["counts"][0][0] == 0 and on["counts"][0][0] >= 1, (on["counts"], off["counts"])
    assert off["counts"][0][1] == 11 and on["counts"][0][1] >= 11  # (rebuilds queued behind a halt are issued again)
    assert all(bool(torch.isfinite(t).all()) for t in on["state"])
    _assert_same(on, off, f"stale {dtype} lanes {md_lanes}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_candidate_stride_too_short_halts_and_recovers(dtype):
    """A first state sizes the candidate rows for a margin of 0.1 (with a quarter of headroom); the state is then loaded
    again with a margin of 1.2, whose candidates - half as many again - do not fit: the wide build in front of the first
    launch overflows, the filter behind it says so, the launch halts and the recovery grows the store.  With the overflow
    hook of the rows themselves (md_overflow_at) in the same run."""
    cs = R.case(R.LONG_ROW_CASE)

    def two_loads(rows_filter):
        with _switches(rows_filter, CAND_EVERY, 100):
            s, integ = _integrator(cs, dtype, DT_ROWS)
            state = _start(cs, s, integ, dtype)
            integ.load(*state)
            integ.advance(7)
            first = integ.last_recoveries()
            _lib.debug_set("rows_cand_margin", 1200)
            assert _filter_applies(cs, 1200)
            integ.store(*state)
            integ.load(*state)
            integ.advance(7)
            second = integ.last_recoveries()
            _lib.debug_set("md_overflow_at", 4)  # the rebuild in front of launch 3 of the next call (10 steps since the build)
            integ.advance(9)
            third = integ.last_recoveries()
            assert _lib.debug_get("md_overflow_at") == 0
            integ.store(*state)
            return _result(s, state), (first, second, third)

    on, rec_on = two_loads(1)
    off, rec_off = two_loads(0)
    assert rec_off == (0, 0, 1) and rec_on[0] == 0 and rec_on[1] >= 1 and rec_on[2] == 1, (rec_on, rec_off)
    _assert_same(on, off, f"short candidate stride {dtype}")


# ---- 3: advance(a); advance(b) is advance(a + b) ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _whole(name, dtype, lanes):
    return _advance(R.case(name), dtype, 1, (31,))


@pytest.mark.parametrize("a", [14, 15, 16], ids=["before", "on", "after"])
@pytest.mark.parametrize("name", ["bundle516", "lattice576-wrapped"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_split_around_a_wide_build_changes_nothing(name, dtype, a, md_lanes):
    """The rebuild before step 15 is wide (CAND_EVERY = 3 rebuilds of 5 steps): the first call ends one launch before it,
    on it (the next call's first launch rebuilds) and one behind it."""
    whole = _whole(name, dtype, md_lanes)
    split = _advance(R.case(name), dtype, 1, (a, 31 - a))
    assert whole["counts"] == [(0, 6)] and [c[0] for c in split["counts"]] == [0, 0] and sum(c[1] for c in split["counts"]) == 6
    _assert_same(split, whole, f"{name} {dtype} split at {a}")


# ---- 4: a new policy and a new state start from a wide build -----------------------------------------------------------

@pytest.mark.parametrize("what", ["policy", "load"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_new_policy_or_state_starts_from_a_wide_build(dtype, what):
    """Twelve steps, then another skin (other rows from the same state) or another state (the whole system moved by 0.8,
    more than half the margin: candidates kept across the load would halt the first launch), then twelve more."""
    cs = R.case("bundle516")

    def run(rows_filter):
        with _switches(rows_filter, CAND_EVERY, 1000):
            s, integ = _integrator(cs, dtype, DT_ROWS)
            state = _start(cs, s, integ, dtype)
            integ.load(*state)
            integ.advance(12)
            integ.store(*state)
            if what == "policy":
                integ.set_neighbor_policy(r_cut=cs.r_cut, skin=0.9, every=EVERY)
            else:
                state[0].add_(torch.tensor([0.8, 0.0, 0.0], dtype=TORCH[dtype], device=s.device))
                integ.load(*state)
            integ.advance(12)
            assert integ.last_recoveries() == 0
            integ.store(*state)
            return _result(s, state)

    _assert_same(run(1), run(0), f"{what} {dtype}")
