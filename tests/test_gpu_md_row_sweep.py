"""The radial pass of md_step_kernel walks a nucleotide's unbonded row - close segment, then far segment - in ONE sweep of
strides of G lanes.  What can go wrong there sits at the segment boundaries, not in the size: a close segment or a row
that ends on a stride boundary, one entry past it or one short of it; a stride that holds close and far entries; a row
with no close, no far or no unbonded entry at all; a row long enough for the pipeline to reach its steady state.

Systems: the 16-nt golden duplex with its pair list (every entry close, no far segment), a 40 bp ideal duplex with
device-built rows at five skins (skin 0: a static list by the centre criteria; the others: the integrator's own lists,
close and far segments by the site criteria), two free nucleotides far apart (rows of nothing but the bonded slots) and
two back to back (an empty close segment before a far one).  Each at 8 and 16 lanes per nucleotide (the 16-lane
instantiations walk the two segments as two pipelines: the same rows, the same checks), fp64 and fp32.
 * the rows themselves, read back: in range, segments ordered as the builder documents, lengths as neighbor_stats has them,
   and - over the systems - every class of boundary named above is present (a condition of this file, not a measurement),
 * fp64 step-by-step parity with the oracle on the all-pairs list (tolerances of tests/test_gpu_langevin.py),
 * device-built list == static all-pairs list to the order of the sums (same file, same tolerance),
 * split runs == one run and energy-trace instantiation == plain one, bitwise.
"""

import functools
import types

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import flat_params as fp
from mythos_amd.input import defaults
from mythos_amd.utils import generators
from tests import helpers as H

pytestmark = pytest.mark.gpu

KT = 296.15 * 0.1 / 300.0
R_CUT = 3.3
SKINS = (0.0, 0.3, 0.9, 1.2, 1.5)  # (1.2: the close segments of the inner nucleotides are 16 entries, one stride of 16 lanes)
N_BP = 40
BONDED = 4  # slots at the head of every row
ROLE_Q = 1 << 30
SEED = 0x1234ABCD5678
INERTIA = (1.0, 1.3, 0.8)
N_STEPS = 3
DTYPES = (torch.float64, torch.float32)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(topology, centres, quaternions, box) of a system."""
    if kind == "golden":
        top, traj, _, _ = H.load_golden(2, "simple-helix")
        return top, traj.center[0], traj.quaternions[0], traj.box_size
    if kind == "duplex":
        top, c, q = generators.ideal_duplex(N_BP, model=2, seed=3)
        return top, c, q, None
    # two free nucleotides.  "free": far apart, nothing in any row.  "backs": back to back, 2.0 apart along x with the
    # bases pointing away from each other - the backbone sites 1.5 apart, inside the Debye-Hueckel range (1.52 at this
    # salt), every base, stacking and backbone-base distance beyond 2.0 where the largest close range is 0.75: with the
    # integrator's lists each is the other's only entry, in the FAR segment behind an empty close one
    assert kind in ("free", "backs")
    top = types.SimpleNamespace(seq=np.array([0, 3], dtype=np.int32), is_end=np.ones(2, dtype=np.int32),
                                bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                                unbonded_neighbors=np.zeros((0, 2), dtype=np.int32), n_nucleotides=2)
    if kind == "free":
        c = np.array([[0.0, 0.0, 0.0], [40.0, 3.0, -7.0]])
        q = np.array([[1.0, 0.0, 0.0, 0.0], [0.6, 0.0, 0.8, 0.0]])
    else:
        c = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
        q = np.array([[0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0]])  # a1 = -x and +x
    return top, c, q, None


def _integrator(kind, dtype, skin=None):
    """System + integrator with the rows of the case in place: (system, integrator, c, q).  skin None: the pair list of
    the topology; 0: device-built once, static; > 0: the integrator's own lists."""
    from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem

    top, c0, q0, box = _case(kind)
    sim, cfg = defaults.default_configs_for("dna2")
    flat = fp.pack_flat(fp.derive_flat(2, cfg, kt=sim["kT"], salt_conc=0.5, half_charged_ends=False), _lib.param_names())
    s = OxdnaSystem(2, top.seq, top.is_end, top.bonded_neighbors, box=box, dtype=dtype)
    s.set_params(flat)
    integ = LangevinIntegrator(s, dt=0.005, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, mass=1.0, inertia=INERTIA, seed=SEED)
    c = torch.as_tensor(c0, dtype=dtype, device=s.device).contiguous()
    q = torch.as_tensor(q0, dtype=dtype, device=s.device).contiguous()
    if skin is None:
        s.set_neighbors(top.unbonded_neighbors)
    elif skin == 0.0:
        s.build_neighbors(c, R_CUT, 0.0)
    else:
        integ.set_neighbor_policy(r_cut=R_CUT, skin=skin, every=1000)
    return s, integ, c, q


def _run(kind, dtype, skin, plan, save_every=0):
    """State (c, q, p, L) after the runs of `plan` and the system (for its rows)."""
    s, integ, c, q = _integrator(kind, dtype, skin)
    p, L = integ.init_momenta()
    for n in plan:
        integ.run(c, q, p, L, n, save_every=save_every)
    return (c, q, p, L), s


CASES = [("golden", None), ("free", None), ("backs", 0.3), ("duplex", None)] + [("duplex", skin) for skin in SKINS]
CASE_IDS = [f"{k}-{'pairs' if sk is None else sk}" for k, sk in CASES]


# ---- the rows ------------------------------------------------------------------------------------------------------

def _rows_of(kind, skin, dtype=torch.float64):
    _, s = _run(kind, dtype, skin, (1,))
    return s, s.rows()


@pytest.mark.parametrize(("kind", "skin"), CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rows_are_in_range_ordered_and_as_long_as_the_stats_say(kind, skin, dtype):
    s, (rows, ln, close) = _rows_of(kind, skin, dtype)
    n = s.n
    assert rows.shape[0] == n and ln.shape == (n,) and close.shape == (n,)
    assert (ln >= BONDED).all() and (ln <= rows.shape[1]).all() and (close >= BONDED).all() and (close <= ln).all()
    mx, mean = s.neighbor_stats()
    assert mx == int(ln.max()) - BONDED and abs(mean - float((ln - BONDED).mean())) < 1e-9
    for i in range(n):
        ent = rows[i, BONDED:ln[i]]
        idx = ent & (ROLE_Q - 1)
        assert (ent >= 0).all() and (idx < n).all() and (idx != i).all()
        assert len(set(idx.tolist())) == len(idx)
        if skin is not None:  # device-built: the lower index of a pair plays the first role, each segment ascends
            assert (((ent & ROLE_Q) != 0) == (idx < i)).all()
            for seg in (idx[: close[i] - BONDED], idx[close[i] - BONDED:]):
                assert (np.diff(seg) > 0).all(), (i, seg)
        else:  # a pair list carries no distance classes: everything is close
            assert close[i] == ln[i]


def test_the_systems_cover_every_class_of_segment_boundary():
    """Over the systems: (close - 4) mod G and (len - 4) mod G each take 0, 1 and G - 1, for G = 8 and 16 (0 with a
    non-empty segment / row); a row with an empty close segment and a far one; a row without far segment; a row of the
    bonded slots alone; a row longer than three strides."""
    close_l, len_l, stats = [], [], []
    for kind, skin in CASES:
        _, (_, ln, close) = _rows_of(kind, skin)
        close_l.append(close - BONDED), len_l.append(ln - BONDED)
        stats.append((kind, skin, sorted(set((close - BONDED).tolist())), sorted(set((ln - BONDED).tolist()))))
    nc, nl = np.concatenate(close_l), np.concatenate(len_l)
    print(stats)
    for G in (8, 16):
        for r in (0, 1, G - 1):
            assert ((nc % G == r) & (nc > 0)).any(), (G, r, "close", stats)
            assert ((nl % G == r) & (nl > 0)).any(), (G, r, "len", stats)
        assert (nl > 3 * G).any(), (G, stats)
    assert ((nc == 0) & (nl > 0)).any(), stats
    assert ((nl == nc) & (nl > 0)).any(), stats
    assert (nl == 0).any(), stats


# ---- results -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_states(kind, p0_bytes, l0_bytes):
    """The oracle's (x, q, p, L, u) after each of N_STEPS steps on the topology's full pair list, computed once per system."""
    from oracle.langevin_oracle import LangevinOracle

    top, c0, q0, box = _case(kind)
    n = c0.shape[0]
    if kind in ("free", "backs"):  # the oracle evaluates the one pair there is (40 length units apart it adds nothing)
        top = types.SimpleNamespace(**{**top.__dict__, "unbonded_neighbors": np.array([[0, 1]], dtype=np.int32)})
    orc = LangevinOracle(2, H.oracle_params(2, salt=0.5, half_charged_ends=False), H.topo_tensors(top), box, 0.005, KT, KT / 2.5,
                         KT / 7.5, 1.0, INERTIA, seed=SEED)
    x, qq = np.array(c0, dtype=np.float64), np.array(q0, dtype=np.float64)
    pp = np.frombuffer(p0_bytes, dtype=np.float64).reshape(n, 3).copy()
    LL = np.frombuffer(l0_bytes, dtype=np.float64).reshape(n, 3).copy()
    out = []
    for _ in range(N_STEPS):
        x, qq, pp, LL, u = orc.step(x, qq, pp, LL)
        out.append((x, qq, pp, LL, u))
    return out


@pytest.mark.parametrize(("kind", "skin"), CASES, ids=CASE_IDS)
def test_step_by_step_parity_with_the_oracle_fp64(kind, skin, md_lanes):
    s, integ, c, q = _integrator(kind, torch.float64, skin)
    p, L = integ.init_momenta()
    ref = _oracle_states(kind, p.cpu().numpy().tobytes(), L.cpu().numpy().tobytes())
    tc, tq, et = integ.run(c, q, p, L, N_STEPS, save_every=1)
    for k, (x, qq, pp, LL, u) in enumerate(ref):
        np.testing.assert_allclose(tc[k].cpu().numpy(), x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(tq[k].cpu().numpy(), qq, rtol=0, atol=1e-10)
        assert abs(et[k, :8].sum().item() - u) <= 1e-8 * abs(u)
    x, qq, pp, LL, _ = ref[-1]
    np.testing.assert_allclose(c.cpu().numpy(), x, atol=1e-10)
    np.testing.assert_allclose(p.cpu().numpy(), pp, atol=1e-9)
    np.testing.assert_allclose(L.cpu().numpy(), LL, atol=1e-9)


@pytest.mark.parametrize("skin", SKINS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_device_built_rows_match_the_static_all_pairs_list(skin, dtype, md_lanes):
    """One step: the momenta it leaves are the forces of both its half kicks.  fp64 to the order of the sums (the
    tolerance of test_dynamic_verlet_list_matches_static_all_pairs).  fp32: the same terms summed in another order -
    a row of at most 80 terms, each rounding half an ulp of the running sum, which the largest momentum bounds - on
    the momenta; the stored centres and quaternions within two roundings of their largest value."""
    a, _ = _run("duplex", dtype, skin, (1,))
    b, _ = _run("duplex", dtype, None, (1,))
    for x, y, ulps in zip(a, b, (2, 2, 40, 40)):
        atol = 1e-9 if dtype == torch.float64 else ulps * 2.0**-24 * float(y.abs().max())
        torch.testing.assert_close(x, y, rtol=0, atol=atol)


@pytest.mark.parametrize("skin", SKINS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_split_runs_and_the_energy_trace_instantiation_are_bitwise_the_plain_run(skin, dtype, md_lanes):
    """(split: advance(2); advance(4) on the resident state - two run() calls hand the state through the caller's arrays
    and re-normalise the quaternions on entry, an ulp)"""
    one, _ = _run("duplex", dtype, skin, (6,))
    traced, _ = _run("duplex", dtype, skin, (6,), save_every=1)
    _, integ, c, q = _integrator("duplex", dtype, skin)
    p, L = integ.init_momenta()
    integ.load(c, q, p, L)
    integ.advance(2)
    integ.advance(4)
    integ.store(c, q, p, L)
    split = (c, q, p, L)
    for a, b, c in zip(one, split, traced):
        assert torch.equal(a, b)
        assert torch.equal(a, c)
