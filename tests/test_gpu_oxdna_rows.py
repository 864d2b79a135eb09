"""The oxDNA neighbour rows, read back from the device and compared ENTRY FOR ENTRY with a brute-force classification
(tests/oxdna_rows_ref.py: must <= row <= may, segment by segment, pairs inside the margin band excepted), and the skin
guarantee of the step kernel's displacement check, by physics.

Every other check of the rows compares energies or forces at or near the frame a list was built from, where a pair in
the wrong segment or missing from the skin shell costs nothing: it loses its terms only once it has moved into range.

Rows: the integrator's lists (site criteria; build_rows_allpairs_kernel under 512 nucleotides or three cells per
periodic edge, build_rows_cells_kernel otherwise - free space and periodic, workgroups full and not, buckets of three
places so that candidates come through the spill list, rows that outgrow the first stride of 64, oxNA with non-zero
slack terms, oxDNA1 and oxRNA2), the energy-path builder (centre criterion), and the rows of the third build of a run.
tests/test_oxdna_rows_ref_cpu.py asserts without a GPU that each case takes the builder named here and fills what it is
said to fill.

Skin guarantee: two free nucleotides approach by translation, by a swing of the base site alone and by a swing of the
backbone site (tests/oxdna_approach_scenarios.py) on a list that only the displacement check can rebuild; the run must
equal the one on a static all-pairs list.
"""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from tests import oxdna_approach_scenarios as A
from tests import oxdna_rows_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"f64": torch.float64, "f32": torch.float32}
DTYPES = ("f64", "f32")
KT = 296.15 * 0.1 / 300.0
DT_ROWS = 1e-4  # the perturbed frames are strained (overlaps, stretched bonds): steps short enough to stay finite and near


def _system(cs, dtype):
    from mythos_amd.hip_system import OxdnaSystem

    s = OxdnaSystem(cs.model, cs.top.seq, cs.top.is_end, cs.top.bonded_neighbors, box=cs.box, dtype=TORCH[dtype], is_rna=cs.is_rna)
    s.set_params(torch.as_tensor(R.flat_for(cs.model)[0]))
    return s


def _state(cs, s, dtype, c=None):
    to = dict(dtype=TORCH[dtype], device=s.device)
    return torch.as_tensor(cs.c if c is None else c, **to).contiguous(), torch.as_tensor(cs.q, **to).contiguous()


def _integrator_rows(cs, dtype):
    """Decoded rows of the list the integrator builds at the case's frame: one step from zero momenta on a list that is
    built once (the rows are those of the input frame, as tests/test_gpu_md_row_sweep.py relies on)."""
    from mythos_amd.hip_system import LangevinIntegrator

    s = _system(cs, dtype)
    integ = LangevinIntegrator(s, dt=DT_ROWS, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=3)
    integ.set_neighbor_policy(r_cut=cs.r_cut, skin=cs.skin, every=1000)
    c, q = _state(cs, s, dtype)
    p, L = torch.zeros_like(c), torch.zeros_like(c)
    integ.run(c, q, p, L, 1)
    assert integ.last_recoveries() == 0
    rows, ln, close = s.rows()
    return rows, ln, close


def _assert_contract(rows, must, may, what):
    gc, gf, bad = R.decode(*rows)
    assert not bad, (what, bad[:4])
    listed = int(may.listed.sum()) // 2
    assert int(may.band.sum()) // 2 <= R.BAND_CAP * listed and int(must.band.sum()) // 2 <= R.BAND_CAP * listed  # (of the inputs)
    msgs = R.contract_failures(gc, gf, must, may)
    assert not msgs, what + "\n" + "\n".join(msgs)
    return gc, gf


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    return R.case(name).reference(dtype)


@functools.lru_cache(maxsize=None)
def _plain_rows(name, dtype):
    """Rows of a case with the buckets at their managed size, decoded - shared by the tests that compare with them."""
    cs = R.case(name)
    must, may = _reference(name, dtype)
    return _assert_contract(_integrator_rows(cs, dtype), must, may, f"{name} {dtype}")


# ---- (a) - (g): the integrator's rows ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SITE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_integrator_rows_hold_must_and_nothing_outside_may(name, dtype):
    cs = R.case(name)
    assert R.uses_cells(cs.n, cs.box, cs.r_list) == cs.cells  # the builder this case is here for
    gc, gf = _plain_rows(name, dtype)
    must, _ = _reference(name, dtype)
    assert gc.any() and (gf.any() or not must.far.any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_outgrow_the_first_stride(dtype):
    cs = R.case(R.LONG_ROW_CASE)
    rows, ln, close = _integrator_rows(cs, dtype)
    assert rows.shape[1] > 64 and int(ln.max()) > 64
    _assert_contract((rows, ln, close), *_reference(cs.name, dtype), f"{cs.name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrapped_and_unwrapped_coordinates_give_the_same_rows(dtype):
    a, b = _plain_rows("lattice576", dtype), _plain_rows("lattice576-wrapped", dtype)
    unsure = np.zeros_like(a[0])
    for name in R.PERIODIC_CELL_CASES:
        for ref in _reference(name, dtype):
            unsure |= ref.band
    for x, y, seg in zip(a, b, ("close", "far")):
        ii, jj = np.nonzero((x != y) & ~unsure)
        assert ii.size == 0, (seg, list(zip(ii.tolist(), jj.tolist()))[:8])


# ---- (d): candidates through the spill list, with sites ------------------------------------------------------------

@pytest.mark.parametrize("name", R.CELL_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_through_the_spill_list_are_the_same_rows(name, dtype):
    """Buckets of three places (tests/test_oxdna_rows_ref_cpu.py: cells of these cases hold more): most candidates
    reach a row through the spill branch of build_rows_cells_kernel, which fetches their offsets and base vectors by
    index.  The decisions are the same arithmetic on the same numbers: the same rows, not merely rows within the contract."""
    cs = R.case(name)
    plain = _plain_rows(name, dtype)
    _lib.debug_set("cell_bucket_cap", R.SPILL_BUCKET_CAP)
    try:
        rows = _integrator_rows(cs, dtype)
    finally:
        _lib.debug_set("cell_bucket_cap", 0)
    assert _lib.debug_get("cell_bucket_cap") == 0
    gc, gf = _assert_contract(rows, *_reference(name, dtype), f"{name} {dtype} spill")
    assert (gc == plain[0]).all() and (gf == plain[1]).all()


# ---- (h): the energy path's builder --------------------------------------------------------------------------------

@pytest.mark.parametrize("spill", [False, True], ids=["buckets", "spill"])
@pytest.mark.parametrize("name", R.CELL_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_energy_path_rows_are_the_centre_criterion(name, dtype, spill):
    """OxdnaSystem.build_neighbors with parameters set: listed iff the centres are within r_cut + skin, close iff within the
    close range + skin - the pairs themselves, not their number."""
    cs = R.case(name)
    ref = cs.centre_reference(dtype)
    s = _system(cs, dtype)
    c, _ = _state(cs, s, dtype)
    _lib.debug_set("cell_bucket_cap", R.SPILL_BUCKET_CAP if spill else 0)
    try:
        s.build_neighbors(c, cs.r_cut, cs.skin)
    finally:
        _lib.debug_set("cell_bucket_cap", 0)
    gc, gf = _assert_contract(s.rows(), ref, ref, f"{name} {dtype} energy path")
    assert gc.any() and gf.any()


# ---- (i): rows of a later build ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_the_third_build_belong_to_the_frame_it_was_made_from(dtype):
    """A rebuild every five steps, eleven steps: builds before steps 0, 5 and 10 - the third through the double-buffered
    cell counters' first half again.  The rows the run leaves are those of the state after ten steps, saved frame 9."""
    from mythos_amd.hip_system import LangevinIntegrator

    every = 5
    cs = R.case("bundle512")
    s = _system(cs, dtype)
    integ = LangevinIntegrator(s, dt=DT_ROWS, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=17)
    integ.set_neighbor_policy(r_cut=cs.r_cut, skin=cs.skin, every=every)
    c, q = _state(cs, s, dtype)
    p, L = integ.init_momenta()
    tc, tq, _ = integ.run(c, q, p, L, 2 * every + 1, save_every=1)
    assert integ.last_rebuilds() == 2 and integ.last_recoveries() == 0
    at = 2 * every - 1
    fc, fq = tc[at].cpu().numpy().astype(np.float64), tq[at].cpu().numpy().astype(np.float64)
    assert np.abs(fc - cs.c).max() > 10 * R.BAND[dtype]  # (another frame than the first build's)
    must, may = cs.reference(dtype, c=fc, q=fq)
    _assert_contract(s.rows(), must, may, f"third build {dtype}")


# ---- the skin guarantee under approach -----------------------------------------------------------------------------

def _approach_run(sc, dynamic):
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    top = A.two_free_nucleotides()
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=None, dtype=torch.float64)
    s.set_params(torch.as_tensor(R.flat_for(2)[0]))
    integ = LangevinIntegrator(s, dt=A.DT, kT=A.KT, gamma_t=A.GAMMA_T, gamma_r=A.GAMMA_R, mass=1.0, inertia=(1.0, 1.0, 1.0), seed=A.SEED)
    if dynamic:
        integ.set_neighbor_policy(r_cut=R.R_CUT, skin=sc.skin, every=1000)  # only the displacement check can rebuild
    else:
        s.set_neighbors(np.array([[0, 1]], dtype=np.int32))
    to = dict(dtype=torch.float64, device=s.device)
    c, q, p, L = (torch.as_tensor(x, **to).contiguous() for x in (sc.c, sc.q, sc.p, sc.L))
    tc, tq, et = integ.run(c, q, p, L, sc.steps, save_every=1)
    return torch.cat([c.reshape(-1), q.reshape(-1), p.reshape(-1), L.reshape(-1)]), tc, tq, et, integ.last_recoveries()


@pytest.mark.parametrize("name", list(A.SCENARIOS))
def test_a_pair_that_approaches_between_builds_is_listed_in_time(name, md_lanes):
    """Final state, saved frames and traced energies equal those on a static all-pairs list (the tolerances of
    tests/test_gpu_langevin.py::test_a_site_leaving_its_skin_halts_rebuilds_and_resumes_exactly).  Not vacuous: at the
    build frame the pair is not in the class whose term acts later, that term does become non-zero, the list was rebuilt
    out of turn - and in the swings the centres have not left their skin by then: a site clause asked for it."""
    sc = A.SCENARIOS[name]
    flat, names = R.flat_for(2)
    ref_state, ref_tc, ref_tq, ref_et, ref_rec = _approach_run(sc, dynamic=False)
    state, tc, tq, et, rec = _approach_run(sc, dynamic=True)

    def classes(c, q):
        must, _ = R.site_rows(c, q, 2, flat, names, skin=sc.skin, band=R.BAND["f64"])
        assert not must.band[0, 1]
        return {"close": bool(must.close[0, 1]), "far": bool(must.far[0, 1])}

    # the scenario, on the all-pairs run: outside the class at the build frame, the term acts later and for a while (a run
    # that missed it ends up elsewhere), the pair is in the class by then
    assert ref_rec == 0 and not classes(sc.c, sc.q)[sc.cls]
    on = np.nonzero(ref_et[:, sc.term].cpu().numpy() != 0)[0]
    assert on.size >= 20 and on[0] > 0, on[:4]
    first = int(on[0])
    assert classes(ref_tc[first].cpu().numpy(), ref_tq[first].cpu().numpy())[sc.cls]

    torch.testing.assert_close(state, ref_state, rtol=0, atol=1e-9)
    torch.testing.assert_close(tc, ref_tc, rtol=0, atol=1e-9)
    torch.testing.assert_close(tq, ref_tq, rtol=0, atol=1e-9)
    torch.testing.assert_close(et, ref_et, rtol=1e-9, atol=1e-9)

    # and it was the displacement check that listed the pair - in the swings a site clause: the centres were still
    # inside their skin when the term began to act
    assert rec >= 1, rec
    assert et[first, sc.term].item() != 0
    if sc.centres_stay:
        assert np.linalg.norm(tc[: first + 1].cpu().numpy() - sc.c, axis=-1).max() < 0.5 * sc.skin
