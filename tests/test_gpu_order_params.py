"""oxDNA's ``bond`` and ``mindistance`` order parameters of stored frames on the GPU (mythos_oxdna_order_params), against
oxDNA's own columns of the melting fixture and against the oracle's per-pair rows (tests/order_param_ref.py).

Bounds between kernel and oracle are the project's (tests/test_gpu_oxdna_energy.py): a per-pair energy in fp64 within rtol
1e-9 + atol 1e-11, in fp32 within 1e-3 of max|e|; the distances get the same relative bounds.
"""

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import dna1
from mythos_amd.energy import flat_params as fp
from mythos_amd.energy.base import Quaternion, RigidBody, space
from mythos_amd.hip_system import OxdnaSystem
from mythos_amd.input import defaults
from mythos_amd.input.order_parameters import OrderParameter
from mythos_amd.observables import MeltingTemp, OrderParameters
from tests import helpers as H
from tests import melting_ref as M
from tests import order_param_ref as R
from tests import oxdna_periodic_synth as S

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
DEV = "cuda:0"


def _system(model, top, box, dtype, hce=False, salt=0.5, overrides=None):
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    for sec, d in (overrides or {}).items():
        cfg[sec].update(d)
    flat = fp.pack_flat(fp.derive_flat(model, cfg, kt=sim["kT"], salt_conc=salt, half_charged_ends=hce), _lib.param_names())
    s = OxdnaSystem(model, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype, device=DEV)
    s.set_params(flat)  # (no neighbour rows: the order parameters read their own pair lists)
    return s


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def _call(s, c, q, ops, dtype, **kw):
    """One raw call, checked for what holds whatever the input: a second call is bitwise equal, the call without the raw
    rows gives the same values, and the values are the count / the minimum of the kernel's OWN rows, exactly."""
    c, q = _dev(c, dtype), _dev(q, dtype)
    val, hb, dist = s.order_params(c, q, ops, raw=True, **kw)
    val2, hb2, dist2 = s.order_params(c, q, ops, raw=True, **kw)
    assert torch.equal(val, val2) and torch.equal(hb, hb2) and torch.equal(dist, dist2)
    assert torch.equal(s.order_params(c, q, ops, **kw), val)
    val, hb, dist = val.cpu().numpy(), hb.cpu().numpy(), dist.cpu().numpy()
    assert val.shape == (c.shape[0], len(ops)) and hb.shape == dist.shape == (c.shape[0], sum(len(o.pairs) for o in ops))
    np.testing.assert_array_equal(val, R.values_from_rows(hb, dist, ops, kw.get("hb_cutoff", R.HB_CUTOFF)))
    return val, hb, dist


def _check_rows(hb, dist, hb_ref, dist_ref, dtype):
    fp64 = dtype == torch.float64
    print(f"max |hb - oracle| {np.abs(hb - hb_ref).max():.3e}  max |dist - oracle| {np.abs(dist - dist_ref).max():.3e}")
    assert (np.abs(hb - hb_ref) <= R.bounds(hb_ref, fp64)).all(), np.abs(hb - hb_ref).max()
    assert (np.abs(dist - dist_ref) <= R.bounds(dist_ref, fp64)).all(), np.abs(dist - dist_ref).max()


# ---- 1. the golden run -----------------------------------------------------------------------------------------------------
def _golden_setup(dtype):
    top, traj, en = M.load_run()
    ef = dna1.create_default_energy_fn(top, space.periodic(M.BOX)[0]).with_noopt("ss_stack_weights", "ss_hb_weights", "kt").with_params(kt=M.KT_SIM)
    body = RigidBody(center=_dev(traj.center, dtype), orientation=Quaternion(vec=_dev(traj.quaternions, dtype)))
    return ef, body, en


@DTYPES
def test_states_of_the_melting_fixture_are_oxdnas_columns(dtype):
    """dna1 defaults, periodic box 20, all 384 frames.  fp64: both columns on every frame.  fp32: mindistance on every frame;
    bond may differ only on frames where a listed pair's ORACLE energy lies within 1e-3 max|e_hb| of the cutoff (the oracle
    alone puts one of the 2 304 entries there), three frames at most."""
    ef, body, en = _golden_setup(dtype)
    ops, hb_ref, _, _ = R.golden_rows()
    op = OrderParameters(R.OP_FILE, ef)
    states = op(body)
    assert states.shape == (384, 2) and states.dtype == torch.int64 and states.device == body.center.device and not states.requires_grad
    assert torch.equal(states, op(body, ef.opt_params()))
    got = states.cpu().numpy()
    assert np.array_equal(got[:, 1], en["mindistance"])
    differ = got[:, 0] != en["bond"]
    print(f"{dtype}: bond differs from oxDNA's column on {int(differ.sum())} frame(s)")
    if dtype == torch.float64:
        assert not differ.any()
    else:
        allowed = R.near_cutoff(hb_ref[:, :6], 1e-3 * np.abs(hb_ref).max()).any(1)
        assert allowed.sum() <= 3 and not (differ & ~allowed).any()
    values = op.values(body)
    assert values.dtype == torch.float64 and torch.equal(op.states_of(values), states)


def test_weights_and_melting_temperature_from_frames_alone():
    """States from the frames, weights from a table: the melting temperature is bit for bit the one the energy file's
    columns give (0.10144342 on this prefix)."""
    ef, body, en = _golden_setup(torch.float64)
    op = OrderParameters(R.OP_FILE, ef)
    states = op(body)
    weights = op.weights(states, R.weight_table(en))
    assert weights.device == states.device and np.array_equal(weights.cpu().numpy(), en["weight"])
    mt = MeltingTemp(sim_temperature=M.KT_SIM, temperature_range=M.kelvin_range(), energy_fn=ef)
    tm = mt(body, states[:, 0], weights, ef.opt_params())
    tm_file = mt(body, en["bond"], en["weight"], ef.opt_params())
    assert float(tm) == float(tm_file) and abs(float(tm) - 0.10144342) <= 1e-8


# ---- 2. raw rows against the oracle ----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", list(R.RAW_CASES))
def test_raw_rows_against_the_oracle(name, dtype):
    k = R.raw_case(name)
    s = _system(k["model"], k["top"], k["box"], dtype, hce=k["hce"], salt=k["salt"])
    ops = k["ops"]
    val, hb, dist = _call(s, k["center"], k["quat"], ops, dtype)
    _check_rows(hb, dist, k["hb"], k["dist"], dtype)
    fp64 = dtype == torch.float64
    # states: the oracle's thresholded rows, entry by entry, except within the bound of the cutoff / of an interface
    near = R.near_cutoff(k["hb"], R.bounds(k["hb"], fp64))
    assert near.sum() <= 0.01 * near.size
    assert (((hb < R.HB_CUTOFF) == (k["hb"] < R.HB_CUTOFF)) | near).all()
    want = R.states_from_rows(k["hb"], k["dist"], ops)
    got = R.states_from_values(val, ops)
    n_bp = len(ops[0].pairs)
    frame_near = near[:, :n_bp].any(1)
    assert ((got[:, 0] == want[:, 0]) | frame_near).all()
    md = k["dist"][:, n_bp:].min(1)
    iface_near = (np.abs(md[:, None] - np.asarray(ops[1].interfaces)[None, :]) <= R.bounds(k["dist"], fp64).max()).any(1)
    assert iface_near.sum() <= 0.01 * iface_near.size and ((got[:, 1] == want[:, 1]) | iface_near).all()
    if name == "crossing-helix-free":  # the second strand is a lattice vector away: nothing binds, every energy is exactly 0
        assert (hb == 0).all() and (got[:, 0] == 0).all() and (got[:, 1] == 3).all()
    if name == "crossing-helix-periodic":
        assert (got[:, 0] == n_bp).all() and (got[:, 1] == 0).all()


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------
def _lattice():
    top, c, q, box = S.duplex_lattice(13.0)
    native = [(24 * d + k, 24 * d + 23 - k) for d in range(24) for k in range(12)]
    return top, S.wrapped(c, box), q, box, native


_LATTICE_REF = {}


def _lattice_ref(pairs):
    """Oracle rows of lattice pairs, computed once per pair list."""
    key = tuple(map(tuple, pairs))
    if key not in _LATTICE_REF:
        top, c, q, box, _ = _lattice()
        _LATTICE_REF[key] = R.oracle_rows(2, H.oracle_params(2), top.seq, c[None], q[None], np.asarray(pairs), box=box)
    return _LATTICE_REF[key]


@DTYPES
@pytest.mark.parametrize("n_pairs", [1, 6, 63, 64, 65, 257])
def test_pair_list_lengths_on_the_folded_lattice(n_pairs, dtype):
    """Native pairs of the 576-nt lattice, folded into its box: 120 of the first 257 go through an image.  64 lanes at
    most own a slice, so 65 and 257 pairs make them stride; 1 ... 64 change the group width."""
    top, c, q, box, native = _lattice()
    pairs = tuple(native[:n_pairs])
    assert n_pairs < 257 or (np.abs(S.image_of_pairs(c, np.asarray(pairs), box)).sum(1) > 0).sum() == 120
    ops = (OrderParameter("bond", "b", pairs), OrderParameter("mindistance", "d", pairs, (0.3, 0.4)))
    s = _system(2, top, box, dtype)
    val, hb, dist = _call(s, c[None], q[None], ops, dtype)
    hb_ref, dist_ref = _lattice_ref(pairs + pairs)
    _check_rows(hb, dist, hb_ref, dist_ref, dtype)
    assert val[0, 0] == n_pairs == (hb_ref[0, :n_pairs] < R.HB_CUTOFF).sum()  # (no energy within 0.3 of the cutoff)
    assert abs(val[0, 1] - dist_ref[0, n_pairs:].min()) <= R.bounds(dist_ref, dtype == torch.float64).max()


@DTYPES
def test_four_order_parameters_with_slices_inside_a_tile(dtype):
    """Slices of 1, 65, 6 and 64 pairs, the kinds interleaved, at a cutoff in the middle of the energies so the counts
    discriminate; then the same pair as (j, i), a pair listed twice, and a non-complementary pair."""
    top, c, q, box, native = _lattice()
    cuts = np.cumsum([0, 1, 65, 6, 64])
    ops = tuple(OrderParameter(kind, f"op{k}", tuple(native[cuts[k]:cuts[k + 1]]), (0.36, 0.4) if kind == "mindistance" else ())
                for k, kind in enumerate(("bond", "mindistance", "mindistance", "bond")))
    hb_ref, dist_ref = _lattice_ref(tuple(native[:136]))
    e_sorted = np.sort(hb_ref[0])
    cutoff = 0.5 * (e_sorted[67] + e_sorted[68])
    assert e_sorted[68] - e_sorted[67] > 1e-5  # (wider than the fp64 bound; fp32 excludes what is nearer than its own)
    s = _system(2, top, box, dtype)
    val, hb, dist = _call(s, c[None], q[None], ops, dtype, hb_cutoff=cutoff)
    _check_rows(hb, dist, hb_ref, dist_ref, dtype)
    fp64 = dtype == torch.float64
    near = R.near_cutoff(hb_ref, R.bounds(hb_ref, fp64), cutoff)
    want = R.values_from_rows(hb_ref, dist_ref, ops, cutoff)
    for k, (a, b) in enumerate(R.slices(ops)):
        if ops[k].kind == "bond":
            assert abs(val[0, k] - want[0, k]) <= near[0, a:b].sum()
        else:
            assert abs(val[0, k] - want[0, k]) <= R.bounds(dist_ref, fp64).max()
    assert 0 < want[0, 3] < 64 and near.sum() <= 0.01 * near.size
    # (j, i) gives what (i, j) gives; a pair listed twice counts twice; bitwise, in either precision
    i, j = native[5]
    seq = np.asarray(top.seq)
    odd = next((24 * d + k, 24 * d + 22 - k) for d in range(24) for k in range(11) if seq[24 * d + k] + seq[24 * d + 22 - k] != 3)
    more = (OrderParameter("bond", "fwd", ((i, j),)), OrderParameter("bond", "rev", ((j, i),)), OrderParameter("bond", "twice", ((i, j), (j, i))),
            OrderParameter("mindistance", "twice_d", ((j, i), (i, j)), (1.0,)), OrderParameter("bond", "odd", (odd,)),
            OrderParameter("mindistance", "odd_d", (odd,), (1.0,)))
    val, hb, dist = _call(s, c[None], q[None], more, dtype)
    assert (hb[0, :6] == hb[0, 0]).all() and (dist[0, :6] == dist[0, 0]).all() and hb[0, 0] < -0.3
    assert list(val[0, :3]) == [1.0, 1.0, 2.0] and val[0, 3] == dist[0, 0]
    assert hb[0, 6] == 0 and hb[0, 7] == 0 and val[0, 4] == 0 and 0.3 < val[0, 5] == dist[0, 7] < 1.0  # close, and never bonded


@DTYPES
@pytest.mark.parametrize("n_frames", [1, 2, 100])
def test_frame_counts(n_frames, dtype):
    top, traj, en = M.load_run()
    ops, hb_ref, dist_ref, _ = R.golden_rows()
    s = _system(1, top, np.full(3, M.BOX), dtype)
    val, hb, dist = _call(s, traj.center[:n_frames], traj.quaternions[:n_frames], ops, dtype)
    _check_rows(hb, dist, hb_ref[:n_frames], dist_ref[:n_frames], dtype)
    got = R.states_from_values(val, ops)
    allowed = R.near_cutoff(hb_ref[:n_frames, :6], R.bounds(hb_ref, dtype == torch.float64)[:n_frames, :6]).any(1)
    assert ((got[:, 0] == en["bond"][:n_frames]) | allowed).all() and np.array_equal(got[:, 1], en["mindistance"][:n_frames])
    single = s.order_params(_dev(traj.center[0], dtype), _dev(traj.quaternions[0], dtype), ops)  # one frame without the frame axis
    assert single.shape == (1, 2) and np.array_equal(single.cpu().numpy(), val[:1])


def test_a_trajectory_one_short_chunk_longer_than_a_launch():
    """65 535 frames ride one launch; 65 535 + 17 frames of the 12-nt system - the fixture's 384 frames tiled - take a second,
    short one.  Frame for frame the tiled answer, raw rows included."""
    top, traj, en = M.load_run()
    ops = R.golden_ops()
    dtype = torch.float32
    s = _system(1, top, np.full(3, M.BOX), dtype)
    c, q = _dev(traj.center, dtype), _dev(traj.quaternions, dtype)
    val, hb, dist = s.order_params(c, q, ops, raw=True)
    total = 65535 + 17
    reps = -(-total // 384)
    big_c, big_q = c.repeat(reps, 1, 1)[:total].contiguous(), q.repeat(reps, 1, 1)[:total].contiguous()
    bval, bhb, bdist = s.order_params(big_c, big_q, ops, raw=True)
    assert bval.shape == (total, 2)
    assert torch.equal(bval, val.repeat(reps, 1)[:total]) and torch.equal(bhb, hb.repeat(reps, 1)[:total])
    assert torch.equal(bdist, dist.repeat(reps, 1)[:total])
    assert torch.equal(s.order_params(big_c, big_q, ops), bval)


# ---- 4. the system's parameters are used -----------------------------------------------------------------------------------
def test_a_weaker_hydrogen_bond_changes_the_counts_as_the_oracle_says():
    ef, body, en = _golden_setup(torch.float64)
    top, traj, _ = M.load_run()
    op = OrderParameters(R.OP_FILE, ef)
    eps = 0.7 * float(ef.params_dict()["eps_hb"])
    weak = op(body, {"eps_hb": eps}).cpu().numpy()
    P = H.oracle_params(1, overrides={"hydrogen_bonding": {"eps_hb": eps}})
    hb_ref, dist_ref = R.oracle_rows(1, P, top.seq, traj.center, traj.quaternions, R.all_pairs(op.ops), box=M.BOX)
    assert np.abs(hb_ref + 0.1).min() > 1e-6  # (no entry within the fp64 bound of the cutoff: equality, frame for frame)
    assert np.array_equal(weak, R.states_from_rows(hb_ref, dist_ref, op.ops))
    assert (weak[:, 0] != en["bond"]).any() and (weak[:, 0] <= en["bond"]).all() and np.array_equal(weak[:, 1], en["mindistance"])
    assert np.array_equal(op(body).cpu().numpy()[:, 0], en["bond"])  # and back, on the same system handle


@DTYPES
def test_sequence_dependent_hydrogen_bonding_table(dtype):
    top, traj, _, _ = H.load_regr("simple-helix-oxdna2-ss")
    w = H.read_ss_weights(H.GOLDEN / "regr" / "simple-helix-oxdna2-ss" / "oxDNA2_sequence_dependent_parameters.txt")
    ov = {"hydrogen_bonding": {"ss_hb_weights": torch.as_tensor(w["ss_hb_weights"])}}
    ops = R.native_ops(int(top.n_nucleotides) // 2)
    box = np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()
    c, q = np.asarray(traj.center[:10]), np.asarray(traj.quaternions[:10])
    hb_ref, dist_ref = R.oracle_rows(2, H.oracle_params(2, overrides=ov), top.seq, c, q, R.all_pairs(ops), box=box)
    hb_sa, _ = R.oracle_rows(2, H.oracle_params(2), top.seq, c, q, R.all_pairs(ops), box=box)
    assert np.abs(hb_ref - hb_sa).max() > 0.05  # the table matters: the average-sequence rows are far outside any bound
    val, hb, dist = _call(_system(2, top, box, dtype, overrides=ov), c, q, ops, dtype)
    _check_rows(hb, dist, hb_ref, dist_ref, dtype)
    near = R.near_cutoff(hb_ref, R.bounds(hb_ref, dtype == torch.float64))
    n_bp = len(ops[0].pairs)
    assert near.sum() <= 0.01 * near.size
    assert ((R.states_from_values(val, ops)[:, 0] == R.states_from_rows(hb_ref, dist_ref, ops)[:, 0]) | near[:, :n_bp].any(1)).all()


# ---- 5. refusals and edges -------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls():
    top, traj, _ = M.load_run()
    ops = R.golden_ops()
    s = _system(1, top, np.full(3, M.BOX), torch.float64)
    c, q = _dev(traj.center[:3], torch.float64), _dev(traj.quaternions[:3], torch.float64)
    empty = s.order_params(c[:0], q[:0], ops)
    assert empty.shape == (0, 2) and empty.dtype == torch.float64
    val, hb, dist = s.order_params(c[:0], q[:0], ops, raw=True)
    assert hb.shape == dist.shape == (0, 12)
    assert s.order_params(c, q, ()).shape == (3, 0)
    with pytest.raises(ValueError, match="names nucleotide 12"):
        s.order_params(c, q, (OrderParameter("bond", "far", ((0, 12),)),))
    s.set_pseq(np.full((12, 4), 0.25), np.full(12, -1), np.zeros((0, 4)), terms=2)
    with pytest.raises(ValueError, match="probabilistic sequence"):
        s.order_params(c, q, ops)
    s.set_pseq()
    assert s.order_params(c, q, ops).shape == (3, 2)
    fresh = OxdnaSystem(1, top.seq, top.is_end, top.bonded_neighbors, box=np.full(3, M.BOX), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.MythosHipError, match="parameters must be set first"):
        fresh.order_params(c, q, ops)
    top4, traj4, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    s4 = OxdnaSystem(4, top4.seq, top4.is_end, top4.bonded_neighbors, box=traj4.box_size, dtype=torch.float64, device=DEV, is_rna=is_rna)
    n4 = int(top4.n_nucleotides)
    with pytest.raises(ValueError, match="oxNA system has three hydrogen-bonding"):
        s4.order_params(_dev(traj4.center[:1], torch.float64), _dev(traj4.quaternions[:1], torch.float64), R.native_ops(n4 // 2))
