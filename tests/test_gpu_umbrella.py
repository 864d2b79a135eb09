"""Umbrella sampling on the resident Langevin state (mythos_langevin_set_umbrella / _advance_umbrella) on the GPU.

The system is the melting fixture's 12-nt dna1 duplex with its op.txt, at melting_ref.KT_SIM: 64 replicas in free space,
and once as one system in the periodic box of 20.  What is held bitwise: a flat table against the plain integrator's loop
load; advance(L); store, the restore of a rejected replica, the replay of every decision on the host (tests/umbrella_ref.py),
reproducibility and resumption.  What is statistical: the sampling law on a four-nucleotide system whose unbiased law the
plain integrator gives."""

import functools

import numpy as np
import pytest
import torch

from mythos_amd import _lib
from mythos_amd.energy import dna1
from mythos_amd.energy import flat_params as fp
from mythos_amd.energy.base import Quaternion, RigidBody, space
from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem
from mythos_amd.input import defaults, topology
from mythos_amd.input.order_parameters import OrderParameter
from mythos_amd.observables import MeltingTemp
from mythos_amd.observables.order_parameters import reweight_from_histogram, umbrella_histogram
from mythos_amd.simulators import HipUmbrellaSampler, UmbrellaInfo
from mythos_amd.simulators.replicas import ReplicaLayout
from mythos_amd.simulators.restraints import PointForces, RepulsionSphere
from tests import helpers as H
from tests import melting_ref as M
from tests import order_param_ref as R
from tests import umbrella_ref as UR

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
CASES = pytest.mark.parametrize("case", ["replicas", "periodic"])
DEV = "cuda:0"
KT = M.KT_SIM
DT = 0.005
SEED = 11
N_REP = 64


@functools.lru_cache(maxsize=None)
def _flat():
    _, cfg = defaults.default_configs_for("dna1")
    return fp.pack_flat(fp.derive_flat(1, cfg, kt=KT, salt_conc=0.5, half_charged_ends=False), _lib.param_names())


def _integrator(s, seed=SEED):
    integ = LangevinIntegrator(s, dt=DT, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=seed)
    integ.set_neighbor_policy(3.25, 0.6, 10)
    return integ


def _partly_bound_frames(count):
    """The first ``count`` frames of the fixture with one to three native bonds: the states whose weights differ most."""
    _, _, en = M.load_run()
    return np.flatnonzero((en["bond"] >= 1) & (en["bond"] <= 3))[:count]


def _joined(center):
    """Frames of the fixture (F, 12, 3) with the second strand moved by the lattice vector of the box of 20 that puts it next
    to the first: the run was periodic, and in free space a strand one image away is 20 units away."""
    c = np.array(center, dtype=np.float64)
    shift = M.BOX * np.round((c[:, :6].mean(1) - c[:, 6:].mean(1)) / M.BOX)
    c[:, 6:] += shift[:, None, :]
    return c


class _Case:
    """A system, an integrator on it and a start: 64 replicas of the duplex in free space, each from its own partly bound
    frame of the fixture (``same_start``: all from the first), or the duplex alone in the periodic box."""

    def __init__(self, kind, dtype, same_start=False, seed=SEED):
        top, traj, _ = M.load_run()
        self.n_one = int(top.n_nucleotides)
        self.n_rep = N_REP if kind == "replicas" else 1
        self.box = None if kind == "replicas" else np.full(3, M.BOX)
        self.dtype = dtype
        layout = ReplicaLayout(self.n_rep, self.n_one)
        seq, is_end, bonded, _ = layout.topology(top.seq, top.is_end, top.bonded_neighbors)
        self.system = OxdnaSystem(1, seq, is_end, bonded, box=self.box, dtype=dtype, device=DEV)
        self.system.set_params(_flat())
        self.integ = _integrator(self.system, seed)
        frames = _partly_bound_frames(self.n_rep)
        if same_start:
            frames = np.repeat(frames[:1], self.n_rep)
        c = torch.as_tensor(_joined(np.asarray(traj.center)[frames]), dtype=dtype, device=DEV)
        q = torch.as_tensor(np.asarray(traj.quaternions)[frames], dtype=dtype, device=DEV)
        if self.n_rep == 1:
            c, q = c[0], q[0]
        self.c, self.q, _ = layout.place(c.contiguous(), q.contiguous(), 3.85)
        self.p, self.ang = self.integ.init_momenta()
        # the duplex alone, for the order parameters of rows: (F, n_rep * n_one, .) -> (F * n_rep, n_one, .)
        self.one = OxdnaSystem(1, top.seq, top.is_end, top.bonded_neighbors, box=self.box, dtype=dtype, device=DEV)
        self.one.set_params(_flat())
        self.seq = top.seq

    def state(self):
        return tuple(t.clone() for t in (self.c, self.q, self.p, self.ang))

    def values(self, c, q, ops):
        """(F, n_rep, n_ops) order-parameter values of rows (F, n, .) from mythos_oxdna_order_params on the duplex alone."""
        f = c.shape[0]
        v = self.one.order_params(c.reshape(f * self.n_rep, self.n_one, 3).contiguous(), q.reshape(f * self.n_rep, self.n_one, 4).contiguous(), ops)
        return v.reshape(f, self.n_rep, len(ops))

    def plain_loop(self, n_seg, steps):
        """load; advance(steps); store, n_seg times, on this case's integrator -> the stored states, one tuple per segment."""
        c, q, p, ang = self.state()
        out = []
        for _ in range(n_seg):
            self.integ.load(c, q, p, ang)
            self.integ.advance(steps)
            self.integ.store(c, q, p, ang)
            out.append((c.clone(), q.clone(), p.clone(), ang.clone()))
        return out

    def loaded_state(self):
        """What load; store hands back of the start (the quaternions normalised as load normalises them)."""
        c, q, p, ang = self.state()
        self.integ.load(c, q, p, ang)
        self.integ.store(c, q, p, ang)
        return c, q, p, ang


def _equal(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. a flat table is plain MD ----------------------------------------------------------------------------------------
@CASES
@DTYPES
def test_a_flat_table_is_the_plain_loop_bit_for_bit(case, dtype):
    n_seg, steps = 6, 25
    ops = R.golden_ops()
    k = _Case(case, dtype)
    k.integ.set_umbrella(ops, np.ones((7, 2)), steps, n_rep=k.n_rep)
    c, q, p, ang = k.state()
    k.integ.load(c, q, p, ang)
    tc, tq, rec = k.integ.advance_umbrella(n_seg)
    k.integ.store(c, q, p, ang)
    assert k.integ.step == n_seg * steps and k.integ.umbrella_counts() == (n_seg * k.n_rep, n_seg * k.n_rep)
    assert rec.accept.shape == (n_seg, k.n_rep) and bool(rec.accept.all())
    assert bool((rec.w_old == 1).all()) and bool((rec.w_new == 1).all())
    plain = _Case(case, dtype).plain_loop(n_seg, steps)
    for b in range(n_seg):
        assert _equal(tc[b], plain[b][0]) and _equal(tq[b], plain[b][1]), f"sample row {b}"
    for got, want, name in zip((c, q, p, ang), plain[-1], ("center", "quat", "p_lin", "p_ang")):
        assert _equal(got, want), name
    assert float((tc[-1] - k.c).abs().max()) > 1e-3  # (it moved)
    # clearing the bias: the integrator steps as it did
    k.integ.set_umbrella()
    with pytest.raises(ValueError, match="no bias is set"):
        k.integ.advance_umbrella(1)
    rc = k.integ._lib.mythos_langevin_advance_umbrella(k.integ._h, 1, 1, None, None, None, None, None, _lib.stream(k.system.device))
    assert rc == -4 and "no bias is set" in _lib.last_error()
    k.integ.advance(5)
    assert k.integ.step == n_seg * steps + 5


# ---- 2. the restore is exact -----------------------------------------------------------------------------------------------
@DTYPES
def test_a_rejected_replica_is_restored_exactly_with_reversed_momenta(dtype):
    """One mindistance parameter over the native pairs with 64 interfaces 0.01 apart, every replica from the same frame and
    the table's only weight at that frame's state: after one segment a replica whose smallest distance left its 0.01 bin is
    rejected."""
    steps = 10
    pairs = R.golden_ops()[0].pairs
    ops = (OrderParameter("mindistance", "fine", pairs, tuple(0.1 + 0.01 * j for j in range(64))),)
    k = _Case("replicas", dtype, same_start=True)
    c0, q0, p0, ang0 = k.loaded_state()
    assert _equal(c0, k.c) and _equal(p0, k.p) and _equal(ang0, k.ang)  # (a closed frame goes out as it came in)
    start = R.states_from_values(k.values(k.c[None], k.q[None], ops)[0].cpu().numpy(), ops)[:, 0]
    assert len(set(start.tolist())) == 1 and 0 < start[0] < 64
    table = np.zeros(65)
    table[start[0]] = 1.0
    k.integ.set_umbrella(ops, table, steps, n_rep=k.n_rep)
    c, q, p, ang = k.state()
    k.integ.load(c, q, p, ang)
    _, _, rec = k.integ.advance_umbrella(1, sample_every=0)
    k.integ.store(c, q, p, ang)
    acc = rec.accept[0]
    n_acc = int(acc.sum())
    print(f"{dtype}: {n_acc} of {k.n_rep} replicas stayed in their bin")
    assert n_acc < k.n_rep and k.integ.umbrella_counts() == (n_acc, k.n_rep)
    assert _equal(acc, rec.states[0, :, 0] == int(start[0]))
    per = lambda t: t.reshape(k.n_rep, k.n_one, -1)  # noqa: E731
    rej = ~acc
    assert _equal(per(c)[rej], per(c0)[rej]) and _equal(per(q)[rej], per(q0)[rej])
    assert _equal(per(p)[rej], -per(p0)[rej]) and _equal(per(ang)[rej], -per(ang0)[rej])
    plain = _Case("replicas", dtype, same_start=True).plain_loop(1, steps)[0]
    for got, want, name in zip((c, q, p, ang), plain, ("center", "quat", "p_lin", "p_ang")):
        assert _equal(per(got)[acc], per(want)[acc]), name
        assert not _equal(per(got)[rej], per(want)[rej]), name
    # a second rejection in a row reverses the momenta the replica holds, (x, -p), again: back to (x, p)
    _, _, rec2 = k.integ.advance_umbrella(1, sample_every=0)
    k.integ.store(c, q, p, ang)
    twice = rej & ~rec2.accept[0]
    print(f"{dtype}: {int(twice.sum())} replicas were rejected twice")
    assert int(twice.sum()) > 0
    assert _equal(per(c)[twice], per(c0)[twice]) and _equal(per(q)[twice], per(q0)[twice])
    assert _equal(per(p)[twice], per(p0)[twice]) and _equal(per(ang)[twice], per(ang0)[twice])


@DTYPES
def test_unbiased_steps_in_between_start_the_chain_again(dtype):
    """advance_umbrella; advance; advance_umbrella: the snapshot and the weights held before the plain steps are not the
    state's any more.  The next boundary decides against the weight of the state the plain steps ended in, and a replica it
    rejects goes back there, not across them.  Every state has its own weight, so a stale one would show."""
    steps = 10
    ops = (OrderParameter("mindistance", "fine", R.golden_ops()[0].pairs, tuple(0.1 + 0.01 * j for j in range(64))),)
    table = 1.0 + np.arange(65.0)
    k = _Case("replicas", dtype)
    k.integ.set_umbrella(ops, table, steps, n_rep=k.n_rep)
    c, q, p, ang = k.state()
    k.integ.load(c, q, p, ang)
    _, _, first = k.integ.advance_umbrella(1, sample_every=0)
    k.integ.advance(30)
    k.integ.store(c, q, p, ang)
    c2, q2, p2, ang2 = (t.clone() for t in (c, q, p, ang))
    now = R.states_from_values(k.values(c2[None], q2[None], ops)[0].cpu().numpy(), ops)[:, 0]
    assert (now != first.held[0, :, 0].cpu().numpy()).mean() > 0.5  # (the plain steps moved most replicas to another state)
    _, _, rec = k.integ.advance_umbrella(1, sample_every=0)
    k.integ.store(c, q, p, ang)
    assert np.array_equal(rec.w_old[0].cpu().numpy(), table[now])
    rej = ~rec.accept[0]
    per = lambda t: t.reshape(k.n_rep, k.n_one, -1)  # noqa: E731
    assert int(rej.sum()) > 0
    assert _equal(per(c)[rej], per(c2)[rej]) and _equal(per(q)[rej], per(q2)[rej])
    assert _equal(per(p)[rej], -per(p2)[rej]) and _equal(per(ang)[rej], -per(ang2)[rej])
    assert np.array_equal(rec.held[0, :, 0].cpu().numpy()[rej.cpu().numpy()], now[rej.cpu().numpy()])


# ---- 3. every decision replays on the host ---------------------------------------------------------------------------------
@DTYPES
def test_decisions_replay_on_the_host(dtype):
    """40 boundaries of 50 steps under the fixture's own weights.  fp32 states may differ from the oracle's only where the
    oracle's own hydrogen-bonding energy of a native pair lies within the project's fp32 bound (1e-3 max|e_hb|) of the
    cutoff."""
    n_seg, steps = 40, 50
    _, _, en = M.load_run()
    ops = R.golden_ops()
    dense = UR.dense_table(ops, R.weight_table(en))
    k = _Case("replicas", dtype)
    k.integ.set_umbrella(ops, R.weight_table(en), steps, n_rep=k.n_rep)
    c, q, p, ang = k.state()
    k.integ.load(c, q, p, ang)
    tc, tq, rec = k.integ.advance_umbrella(n_seg, proposals=True)
    assert tc.shape == (n_seg, k.n_rep * k.n_one, 3) and rec.prop_quat.shape == (n_seg, k.n_rep * k.n_one, 4)
    acc, u, w_old, w_new = (t.cpu().numpy() for t in (rec.accept, rec.u, rec.w_old, rec.w_new))
    states = rec.states.cpu().numpy()
    # the uniform, the table entry, the chain of held weights and the rule
    for b in range(n_seg):
        assert np.array_equal(u[b], UR.uniform(SEED, np.arange(k.n_rep), (b + 1) * steps)), f"u at boundary {b}"
    assert np.array_equal(w_new, dense[states[..., 0], states[..., 1]])
    start = R.states_from_values(k.values(k.c[None], k.q[None], ops)[0].cpu().numpy(), ops)
    w_start = dense[start[:, 0], start[:, 1]]
    assert (w_start > 0).all()
    acc_ref, old_ref = UR.chain(w_start, w_new, u)
    assert np.array_equal(w_old, old_ref) and np.array_equal(acc, acc_ref)
    assert np.array_equal(acc, UR.accepts(u, w_old, w_new))
    assert k.integ.umbrella_counts() == (int(acc.sum()), acc.size)
    # the states held after each decision: the proposal's where accepted, the ones held before otherwise
    held, before = rec.held.cpu().numpy(), start
    for b in range(n_seg):
        assert np.array_equal(held[b], np.where(acc[b][:, None], states[b], before)), f"held states at boundary {b}"
        before = held[b]
    assert np.array_equal(rec.w_held.cpu().numpy(), dense[held[..., 0], held[..., 1]])
    # a sample row is the proposal where accepted and the previous sample row where rejected
    c0, q0, _, _ = _Case("replicas", dtype).loaded_state()
    per = lambda t: t.reshape(k.n_rep, k.n_one, -1)  # noqa: E731
    prev_c, prev_q = c0, q0
    for b in range(n_seg):
        a = rec.accept[b]
        assert _equal(per(tc[b])[a], per(rec.prop_center[b])[a]) and _equal(per(tq[b])[a], per(rec.prop_quat[b])[a]), f"accepted rows of {b}"
        assert _equal(per(tc[b])[~a], per(prev_c)[~a]) and _equal(per(tq[b])[~a], per(prev_q)[~a]), f"rejected rows of {b}"
        prev_c, prev_q = tc[b], tq[b]
    # the record's values are mythos_oxdna_order_params of the proposal rows, bit for bit
    assert _equal(rec.values, k.values(rec.prop_center, rec.prop_quat, ops))
    # the record's states against the oracle on the proposal rows
    pc = rec.prop_center.double().cpu().numpy().reshape(n_seg * k.n_rep, k.n_one, 3)
    pq = rec.prop_quat.double().cpu().numpy().reshape(n_seg * k.n_rep, k.n_one, 4)
    hb_ref, dist_ref = R.oracle_rows(1, H.oracle_params(1, kt=KT), k.seq, pc, pq, R.all_pairs(ops))
    want = R.states_from_rows(hb_ref, dist_ref, ops).reshape(n_seg, k.n_rep, 2)
    if dtype == torch.float64:
        compared = np.ones(acc.shape, dtype=bool)
    else:
        compared = ~R.near_cutoff(hb_ref[:, :6], 1e-3 * np.abs(hb_ref).max()).any(1).reshape(n_seg, k.n_rep)
    excluded = 1.0 - compared.mean()
    accepted, rejected = acc[compared].mean(), (~acc)[compared].mean()
    print(f"{dtype}: excluded {excluded:.4f}, accepted {accepted:.4f}, rejected {rejected:.4f} of the compared decisions; "
          f"states visited {sorted(set(map(tuple, states.reshape(-1, 2).tolist())))}")
    assert np.array_equal(states[compared], want[compared])
    assert excluded <= 0.10
    assert accepted >= 0.10 and rejected >= 0.10


# ---- 4. reproducible and resumable -----------------------------------------------------------------------------------------
@CASES
@DTYPES
def test_same_seed_twice_and_three_plus_five_segments(case, dtype):
    steps = 20
    _, _, en = M.load_run()
    ops, table = R.golden_ops(), R.weight_table(en)

    def run(parts):
        k = _Case(case, dtype)
        k.integ.set_umbrella(ops, table, steps, n_rep=k.n_rep)
        c, q, p, ang = k.state()
        k.integ.load(c, q, p, ang)
        outs = [k.integ.advance_umbrella(n, proposals=True) for n in parts]
        k.integ.store(c, q, p, ang)
        rows = [torch.cat([o[i] for o in outs]) for i in (0, 1)]
        recs = [torch.cat([getattr(o[2], f) for o in outs]) for f in ("values", "states", "w_old", "w_new", "u", "accept", "held", "prop_center", "prop_quat")]
        return rows + recs + [c, q, p, ang], k.integ.umbrella_counts()

    one, counts = run([8])
    again, counts2 = run([8])
    split, counts3 = run([3, 5])
    assert counts == counts2 == counts3 and counts[1] == 8 * (N_REP if case == "replicas" else 1)
    for a, b, s in zip(one, again, split):
        assert _equal(a, b) and _equal(a, s)


# ---- 5. the sampling law ---------------------------------------------------------------------------------------------------
LAW_REP, LAW_STEPS, LAW_SEG = 256, 60_000, 40
LAW_IFACES = (1.0, 2.0, 4.0)
LAW_R0, LAW_STIFF = 2.5, 10.0
LAW_SEQ = (0, 1, 1, 1)  # no two of them complementary


class _TwoDimers:
    """Two 2-nt strands - nucleotides 0, 1 and 14, 15 of the golden 16-nt helix as they stand there, (0, 3) facing each
    other - 256 replicas, each in its own repulsion sphere of radius 2.5 about the start's centroid: the (0, 3) distance visits
    all four states.  The sequence has no complementary pair: a hydrogen-bonded pair at this kT (the bond is worth 10 kT)
    outlives the run, and a run whose states do not mix measures its start, not its law.  Tuned on the GPU within 60 000 step
    launches per run: with complementary strands and r0 = 3 the standard errors were 0.026 (over the bound); with r0 = 3 and
    this sequence the biased run, which starts on the near side of the shell of weight 0.2, had not relaxed after a third of
    60 000 steps (2.9 standard errors off, 0.8 after 180 000); r0 = 2.5 relaxes within the discarded third."""

    def __init__(self, seed, seq=LAW_SEQ, r0=LAW_R0, seg=LAW_SEG):
        _, traj, _, _ = H.load_golden(2, "simple-helix")
        keep = [0, 1, 14, 15]
        c0 = np.asarray(traj.center[0], dtype=np.float64)[keep]
        q0 = np.asarray(traj.quaternions[0], dtype=np.float64)[keep]
        top = topology.from_arrays(np.asarray(seq), [2, 2])
        self.seg = seg
        self.ops = (OrderParameter("mindistance", "d03", ((0, 3),), LAW_IFACES),)
        self.layout = layout = ReplicaLayout(LAW_REP, 4)
        seq, is_end, bonded, _ = layout.topology(top.seq, top.is_end, top.bonded_neighbors)
        self.system = OxdnaSystem(1, seq, is_end, bonded, dtype=torch.float64, device=DEV)
        self.system.set_params(_flat())
        self.integ = _integrator(self.system, seed)
        c = torch.as_tensor(c0, device=DEV)
        self.c, self.q, offsets = layout.place(c, torch.as_tensor(q0, device=DEV), 3.85)
        _, off = layout.restraint_frames(c, offsets)
        centre = c0.mean(axis=0)
        self.integ.set_point_forces(PointForces([RepulsionSphere(i, centre, r0, LAW_STIFF) for i in range(4)]), n_one=4, n_rep=LAW_REP, offsets=off)
        self.p, self.ang = self.integ.init_momenta()
        self.one = OxdnaSystem(1, top.seq, top.is_end, top.bonded_neighbors, dtype=torch.float64, device=DEV)
        self.one.set_params(_flat())

    def states(self, tc, tq):
        """(S, n_rep) states of rows (S, n, .)."""
        s = tc.shape[0]
        v = self.one.order_params(tc.reshape(s * LAW_REP, 4, 3).contiguous(), tq.reshape(s * LAW_REP, 4, 4).contiguous(), self.ops)
        iface = torch.as_tensor(LAW_IFACES, dtype=torch.float64, device=v.device)
        return (v[:, :1] > iface[None, :]).sum(1).reshape(s, LAW_REP).cpu().numpy()

    def biased(self, w, n_steps):
        self.integ.set_umbrella(self.ops, np.asarray(w, dtype=np.float64), self.seg, n_rep=LAW_REP)
        c, q, p, ang = (t.clone() for t in (self.c, self.q, self.p, self.ang))
        self.integ.load(c, q, p, ang)
        tc, tq, rec = self.integ.advance_umbrella(n_steps // self.seg)
        return self.states(tc, tq), rec

    def unbiased(self, n_steps):
        c, q, p, ang = (t.clone() for t in (self.c, self.q, self.p, self.ang))
        self.integ.load(c, q, p, ang)
        tc, tq, _ = self.integ.advance(n_steps, save_every=self.seg, want_energy=False)
        return self.states(tc, tq)


def _law(states, w):
    """p_k proportional to count_k / W_k pooled over the replicas, after the first third of the run; the standard error
    from the jackknife over replicas."""
    st = states[states.shape[0] // 3:]
    counts = np.stack([(st == k).sum(0) for k in range(4)], axis=1).astype(np.float64)  # (n_rep, 4)
    w = np.asarray(w, dtype=np.float64)
    est = lambda c: (c / w) / (c / w).sum()  # noqa: E731
    total = counts.sum(0)
    p = est(total)
    loo = np.stack([est(total - counts[r]) for r in range(counts.shape[0])])
    n = counts.shape[0]
    return p, np.sqrt((n - 1) / n * ((loo - loo.mean(0)) ** 2).sum(0))


def test_the_sampling_law_is_the_unbiased_one_times_the_weights():
    """W = (1, 5, 0.2, 2) on the four states of the (0, 3) distance against the plain integrator: |p_k - p_k'| within 4
    combined standard errors for every state, each standard error at most 0.02.
    60 000 step launches per run (1 500 segments of 40), 256 replicas.  Observed: biased p (0.0234, 0.2011, 0.6829, 0.0926)
    with standard errors (0.0020, 0.0105, 0.0125, 0.0077), unbiased p (0.0205, 0.2027, 0.6844, 0.0924) with (0.0010,
    0.0037, 0.0038, 0.0029): 1.29, 0.15, 0.12 and 0.03 combined standard errors apart; acceptance 0.944."""
    w = (1.0, 5.0, 0.2, 2.0)
    biased, rec = _TwoDimers(seed=5).biased(w, LAW_STEPS)
    plain = _TwoDimers(seed=6).unbiased(LAW_STEPS)
    p_b, se_b = _law(biased, w)
    p_u, se_u = _law(plain, np.ones(4))
    se = np.sqrt(se_b ** 2 + se_u ** 2)
    print(f"biased   p {np.round(p_b, 4)} se {np.round(se_b, 4)}  acceptance {float(rec.accept.double().mean()):.3f}\n"
          f"unbiased p {np.round(p_u, 4)} se {np.round(se_u, 4)}\n|dp| / se {np.round(np.abs(p_b - p_u) / se, 2)}")
    assert (se_b <= 0.02).all() and (se_u <= 0.02).all()
    assert (np.abs(p_b - p_u) <= 4.0 * se).all()
    assert (p_u > 0.01).all()  # (every state is populated: the comparison says something about each)


def test_a_state_of_weight_zero_is_never_sampled():
    k = _TwoDimers(seed=7)
    states, rec = k.biased((1.0, 1.0, 1.0, 0.0), 10_000)
    assert (states <= 2).all() and (states == 2).any()
    proposed = rec.states[..., 0]
    assert bool((proposed == 3).any()) and not bool(rec.accept[proposed == 3].any())  # (it was proposed, and refused)


def test_a_start_of_weight_zero_names_the_replica_and_the_state():
    k = _TwoDimers(seed=7)
    k.integ.set_umbrella(k.ops, np.asarray([0.0, 1.0, 1.0, 1.0]), LAW_SEG, n_rep=LAW_REP)
    k.integ.load(k.c.clone(), k.q.clone(), k.p.clone(), k.ang.clone())
    with pytest.raises(ValueError, match=r"replica 0 starts in state \(0\), which has weight 0"):
        k.integ.advance_umbrella(1)


def test_refusals_with_a_resident_state():
    from mythos_amd.simulators.restraints import Trap

    k = _Case("periodic", torch.float64)
    ops = R.golden_ops()
    ones = np.ones((7, 2))
    with pytest.raises(ValueError, match=r"a weights table of shape \(6, 2\) is too short"):
        k.integ.set_umbrella(ops, ones[:6], 10)
    with pytest.raises(ValueError, match="lists backbone neighbours"):
        k.integ.set_umbrella((OrderParameter("bond", "b", ((3, 4),)),), np.ones(2), 10)
    with pytest.raises(ValueError, match="segment_steps must be at least 1"):
        k.integ.set_umbrella(ops, ones, 0)
    k.integ.set_point_forces(PointForces([Trap(0, (0.0, 0.0, 0.0), 1.0, 1e-3, (1, 0, 0))]))
    with pytest.raises(ValueError, match=r"a point force moves \(rate != 0\)"):
        k.integ.set_umbrella(ops, ones, 10)
    k.integ.set_point_forces()
    k.system.set_pseq(np.full((12, 4), 0.25), np.full(12, -1), np.zeros((0, 4)), terms=2)
    with pytest.raises(ValueError, match="probabilistic sequence"):
        k.integ.set_umbrella(ops, ones, 10)
    k.system.set_pseq()
    k.integ.set_umbrella(ops, ones, 10)
    c, q, p, ang = k.state()
    k.integ.load(c, q, p, ang)
    k.integ.advance(3)
    with pytest.raises(ValueError, match="the resident frame is open"):
        k.integ.set_umbrella(ops, ones, 10)
    tc, _, rec = k.integ.advance_umbrella(2)  # (an open frame is closed first)
    assert tc.shape == (2, 12, 3) and k.integ.step == 23 and bool(rec.accept.all())
    top4, traj4, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    s4 = OxdnaSystem(4, top4.seq, top4.is_end, top4.bonded_neighbors, box=traj4.box_size, dtype=torch.float64, device=DEV, is_rna=is_rna)
    i4 = LangevinIntegrator(s4, dt=DT, kT=KT, gamma_t=KT / 2.5, gamma_r=KT / 7.5, seed=1)
    with pytest.raises(ValueError, match=r"oxNA system \(model 4\)"):
        i4.set_umbrella(R.native_ops(int(top4.n_nucleotides) // 2), np.ones((int(top4.n_nucleotides) // 2 + 1, 4)), 10)


# ---- 6. the sampler ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_the_sampler_returns_frames_states_weights_and_the_next_table(dtype):
    from mythos_amd.simulators.hip_md import StaticSimulatorParams, nvt_langevin
    from mythos_amd.simulators.neighbors import VerletNeighborList

    top, traj, en = M.load_run()
    n, n_rep, steps, n_seg, every = int(top.n_nucleotides), 8, 25, 8, 2
    disp, shift = space.free()
    ef = dna1.create_default_energy_fn(top, disp).with_noopt("ss_stack_weights", "ss_hb_weights", "kt").with_params(kt=KT)
    sp = StaticSimulatorParams(seq=top.seq, mass=(1.0, (1.0, 1.0, 1.0)), gamma=(KT / 2.5, KT / 7.5), bonded_neighbors=top.bonded_neighbors,
                               checkpoint_every=0, dt=DT, kT=KT)
    table = R.weight_table(en)
    sampler = HipUmbrellaSampler(energy_fn=ef, simulator_params=sp, space=(disp, shift), simulator_init=nvt_langevin,
                                 neighbors=VerletNeighborList(3.25, 0.6, 10), n_replicas=n_rep, dtype=dtype, order_parameters=R.OP_FILE,
                                 weights=table, segment_steps=steps, sample_every=every)
    # four replicas start unbound, four with one to three bonds: the frames hold both kinds, as MeltingTemp needs
    frames = np.concatenate([np.flatnonzero(en["bond"] == 0)[:4], _partly_bound_frames(4)])
    dev = torch.device(DEV)
    init = RigidBody(center=torch.as_tensor(_joined(np.asarray(traj.center)[frames]), device=dev),
                     orientation=Quaternion(vec=torch.as_tensor(np.asarray(traj.quaternions)[frames], device=dev)))
    out = sampler.run({}, init, n_seg * steps, key=3)
    trj, info = out.observables
    s = n_seg // every
    assert isinstance(info, UmbrellaInfo) and info.names == ("all_native_bonds", "caca1")
    assert trj.center.shape == (n_rep * s, n, 3) and trj.orientation.vec.shape == (n_rep * s, n, 4) and trj.center.is_cuda
    assert info.states.shape == (n_rep * s, 2) and info.states.dtype == torch.int64 and info.states.is_cuda
    assert info.weight.shape == (n_rep * s,) and info.weight.dtype == torch.float64 and info.weight.is_cuda
    dense = UR.dense_table(R.golden_ops(), table)
    st = info.states.cpu().numpy()
    assert np.array_equal(info.weight.cpu().numpy(), dense[st[:, 0], st[:, 1]])  # (row for row the weight of the frame's state)
    assert np.array_equal(out.state["weights"], reweight_from_histogram(umbrella_histogram(info.states, info.weight, shape=(7, 2))))
    assert out.state["weights"].shape == (7, 2) and 0.0 < out.state["acceptance"] <= 1.0 and out.state["steps"] == n_seg * steps
    # replica-major: the last row of replica r's block is the state the run ended in (the last boundary is a sampling one)
    final = out.state["final_state"]
    assert _equal(trj.center.reshape(n_rep, s, n, 3)[:, -1], final.center) and _equal(trj.orientation.vec.reshape(n_rep, s, n, 4)[:, -1], final.orientation.vec)
    mt = MeltingTemp(sim_temperature=KT, temperature_range=M.kelvin_range(), energy_fn=ef)
    tm = mt(trj, info.states[:, 0], info.weight, ef.opt_params())
    assert tm.shape == () and bool(torch.isfinite(tm))
    # a second run, from the state of the first, under a flat table given for this run: the handles are the first run's
    entry = next(iter(sampler._resident.values()))
    out2 = sampler.run({}, **{**out.state, "weights": np.ones((7, 2))}, n_steps=n_seg * steps)
    assert len(sampler._resident) == 1 and next(iter(sampler._resident.values()))[1] is entry[1]
    assert out2.state["acceptance"] == 1.0 and bool((out2.observables[1].weight == 1).all()) and out2.state["key"] == 5
    assert out2.observables[0].center.shape == (n_rep * s, n, 3)
    sampler.release()
