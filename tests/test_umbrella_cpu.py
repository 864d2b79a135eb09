"""Umbrella sampling, the parts that need no GPU: the refusals of mythos_umbrella_check, the lowering of a weights table,
the bookkeeping round trip from UmbrellaInfo to the next round's weights, and the acceptance rule on a chain small enough
to solve."""

import numpy as np
import pytest
import torch

from mythos_amd.input.order_parameters import OrderParameter
from mythos_amd.observables.order_parameters import reweight_from_histogram, umbrella_histogram
from mythos_amd.simulators import UmbrellaInfo
from mythos_amd.simulators import umbrella as U
from tests import melting_ref as M
from tests import order_param_ref as R
from tests import umbrella_ref as UR


def _fixture():
    top, _, en = M.load_run()
    return top, R.golden_ops(), R.weight_table(en)


def _bonded(top):
    return np.asarray(top.bonded_neighbors, dtype=np.int32).reshape(-1, 2)


# ---- 1. refusals -----------------------------------------------------------------------------------------------------------
def test_the_fixture_passes_the_checks_alone_and_as_replicas():
    top, ops, table = _fixture()
    n = int(top.n_nucleotides)
    dense = U.lower_table(ops, table)
    assert dense.shape == (7, 2)
    U.check_umbrella(n, 1, 1, _bonded(top), ops, dense, 50)
    U.check_umbrella(64 * n, 64, 1, _bonded(top), ops, table, 1)
    U.check_umbrella(n, 1, 2, _bonded(top), ops, np.ones((9, 2)), 50)  # (an axis may be longer than the reachable states)


def test_refusals_of_the_check_by_name():
    top, ops, table = _fixture()
    n = int(top.n_nucleotides)
    dense = U.lower_table(ops, table)
    bonded = _bonded(top)
    with pytest.raises(ValueError, match=r"axis 0 of the weights table holds 6 states; order parameter 0 reaches 7"):
        U.check_umbrella(n, 1, 1, bonded, ops, dense[:6], 50)
    with pytest.raises(ValueError, match=r"axis 1 of the weights table holds 1 states; order parameter 1 reaches 2"):
        U.check_umbrella(n, 1, 1, bonded, ops, dense[:, :1], 50)
    neighbours = (OrderParameter("bond", "b", ((0, 11), (3, 4))),)
    with pytest.raises(ValueError, match=r"pair 1 \(3, 4\) lists backbone neighbours"):
        U.check_umbrella(n, 1, 1, bonded, neighbours, np.ones(3), 50)
    with pytest.raises(ValueError, match=r"pair 1 \(4, 3\) lists backbone neighbours"):
        U.check_umbrella(n, 1, 1, bonded, (OrderParameter("bond", "b", ((0, 11), (4, 3))),), np.ones(3), 50)
    for bad in (-1.0, np.nan, np.inf):
        w = dense.copy()
        w[2, 1] = bad
        with pytest.raises(ValueError, match=r"weight 5 of the table is negative or not finite"):
            U.check_umbrella(n, 1, 1, bonded, ops, w, 50)
    with pytest.raises(ValueError, match=r"every weight of the table is 0"):
        U.check_umbrella(n, 1, 1, bonded, ops, np.zeros((7, 2)), 50)
    with pytest.raises(ValueError, match=r"oxNA system \(model 4\)"):
        U.check_umbrella(n, 1, 4, bonded, ops, dense, 50)
    for steps in (0, -3):
        with pytest.raises(ValueError, match=r"segment_steps must be at least 1"):
            U.check_umbrella(n, 1, 1, bonded, ops, dense, steps)
    with pytest.raises(ValueError, match=r"names a nucleotide outside one replica \[0, 12\)"):
        U.check_umbrella(2 * n, 2, 1, bonded, (OrderParameter("bond", "b", ((0, 12),)),), np.ones(2), 50)
    with pytest.raises(ValueError, match=r"are not 5 replicas of one system"):
        U.check_umbrella(n, 5, 1, bonded, ops, dense, 50)


def test_an_empty_slice_is_refused():
    """OrderParameter refuses an empty pair list itself, so the slice is emptied in the lowered lists."""
    from mythos_amd import _lib

    top, ops, table = _fixture()
    dense = U.lower_table(ops, table)
    keep, args = U._bias_args(ops, dense)
    keep[0]["first"][1] = 0  # order parameter 0 owns pairs [0, 0)
    bonded = _bonded(top)
    rc = _lib.load().mythos_umbrella_check(int(top.n_nucleotides), 1, 1, int(bonded.shape[0]), bonded.ctypes.data_as(_lib.c_int_p), *args, 50)
    assert rc == -1 and "order parameter 0 has an empty slice of pairs" in _lib.last_error()


def test_the_fixture_leaves_few_decisions_to_exclude_in_fp32():
    """The GPU replay test compares fp32 states with the oracle's except where the oracle's own hydrogen-bonding energy of
    a native pair lies within the project's fp32 bound (1e-3 max|e_hb|) of the cutoff, and asks that at most 10 % of the
    decisions are excluded that way.  A condition on the inputs: over the fixture's 384 frames the oracle puts 0.26 % of
    the frames there."""
    _, hb, _, _ = R.golden_rows()
    near = R.near_cutoff(hb[:, :6], 1e-3 * np.abs(hb).max()).any(1)
    assert near.mean() <= 0.10


# ---- 2. table lowering -----------------------------------------------------------------------------------------------------
def test_table_lowering_from_a_dict_and_from_an_array():
    _, ops, table = _fixture()
    dense = U.lower_table(ops, table)
    assert dense.dtype == np.float64 and dense.flags["C_CONTIGUOUS"] and dense.shape == UR.reachable_shape(ops) == (7, 2)
    assert np.array_equal(dense, UR.dense_table(ops, table))
    for key, w in table.items():
        assert dense[key] == w
    assert (dense > 0).sum() == len(table) < dense.size  # (the states the run never visited have no row: weight 0)
    # an array goes through as it is; a missing row of a dict is weight 0; a one-parameter dict may be keyed by ints
    assert np.array_equal(U.lower_table(ops, dense), dense) and np.array_equal(U.lower_table(ops, dense.tolist()), dense)
    one = (ops[0],)
    assert np.array_equal(U.lower_table(one, {0: 2.0, 6: 0.5, (3,): 1.5}), [2.0, 0, 0, 1.5, 0, 0, 0.5])
    with pytest.raises(ValueError, match="too short"):
        U.lower_table(ops, dense[:6])
    with pytest.raises(ValueError, match="too short"):
        U.lower_table(ops, dense[:, 0])
    with pytest.raises(ValueError, match=r"row for the state \(7, 0\)"):
        U.lower_table(ops, {(7, 0): 1.0})
    lists = U.lower_ops(ops)
    assert lists["kind"].tolist() == [0, 1] and lists["first"].tolist() == [0, 6, 12] and lists["iface_first"].tolist() == [0, 0, 1]
    assert lists["interfaces"].tolist() == [4.0] and lists["pairs"].shape == (12, 2)


# ---- 3. bookkeeping round trip ---------------------------------------------------------------------------------------------
def test_info_to_histogram_to_weights_round_trip():
    """Frames drawn from a known biased law p_k W_k: the weights of the next round flatten it - W'_k p_k is the same for
    every visited state - and a second round under W' returns W' itself up to the normalisation."""
    _, ops, _ = _fixture()
    rng = np.random.default_rng(3)
    # unbiased law over (bond, mindistance): unbound and far, unbound and close, then one to six bonds, all close
    p = np.asarray([[0.05, 0.45], [0.2, 0.0], [0.1, 0.0], [0.08, 0.0], [0.06, 0.0], [0.04, 0.0], [0.02, 0.0]])
    w = np.where(p > 0, 1.0 / np.maximum(p, 1e-300), 0.0) * rng.uniform(0.5, 2.0, p.shape)
    law = (p * w).ravel() / (p * w).sum()
    flat = rng.choice(law.size, size=200_000, p=law)
    states = np.stack(np.unravel_index(flat, p.shape), axis=1)
    info = UmbrellaInfo(states=torch.as_tensor(states), weight=torch.as_tensor(w.ravel()[flat]), names=tuple(o.name for o in ops))
    assert info.states.shape == (200_000, 2) and info.states.dtype == torch.int64 and info.weight.dtype == torch.float64
    hist = umbrella_histogram(info.states, info.weight, shape=p.shape)
    assert hist["count"].sum() == 200_000 and np.array_equal(hist["count"] > 0, p > 0)
    nxt = reweight_from_histogram(hist)
    assert nxt.shape == p.shape and np.array_equal(nxt > 0, p > 0) and nxt[p > 0].min() == 1.0
    flatness = (nxt * p)[p > 0]
    # the biased law p W is flat within a factor of 4 over 8 states: a state holds 200 000 / 32 = 6 250 frames at the least,
    # a relative error of 1 / sqrt(6 250) = 1.3 % per state; five of those
    assert np.abs(flatness / flatness.mean() - 1.0).max() < 0.065
    # exact unbiased counts N p_k give W' = 1 / (N p_k) over its smallest value: W' p is max(p) for every visited state
    exact = reweight_from_histogram(p)
    assert np.allclose(exact[p > 0] * p[p > 0], p.max(), rtol=1e-14, atol=0)
    # and the table goes back into the sampler as it is
    assert np.array_equal(U.lower_table(ops, nxt), nxt)


# ---- 4. the rule on a chain that can be solved -----------------------------------------------------------------------------
def _proposal(pi, rng):
    """A 4-state proposal reversible with respect to pi: symmetric flows S_ij, q_ij = S_ij / pi_i (pi uniform: q symmetric)."""
    S = rng.uniform(0.01, 0.05, (4, 4))
    S = 0.5 * (S + S.T)
    np.fill_diagonal(S, 0.0)
    q = S / pi[:, None]
    assert (q.sum(1) < 1).all()
    return q


@pytest.mark.parametrize("w", [(1.0, 4.0, 0.25, 2.0), (1.0, 4.0, 0.0, 2.0), (8.0, 8.0, 8.0, 8.0)], ids=["mixed", "forbidden", "flat"])
def test_the_rule_on_a_four_state_chain_has_the_law_pi_w(w):
    """A symmetric proposal matrix (pi uniform), then one reversible under a non-uniform pi; the weights are powers of two,
    so the 2^32 values of u accept with probability min(1, W_j / W_i) exactly and the stationary law is pi W to round-off."""
    w = np.asarray(w)
    rng = np.random.default_rng(11)
    for pi in (np.full(4, 0.25), np.asarray([0.4, 0.3, 0.2, 0.1])):
        q = _proposal(pi, rng)
        if np.ptp(pi) == 0:
            assert np.array_equal(q, q.T)
        law = UR.stationary(q, w)
        want = pi * w / (pi * w).sum()
        assert np.abs(law - want).max() <= 1e-12, (law, want)
        assert (law[w == 0] == 0).all()


def test_the_acceptance_probability_of_the_rule():
    assert UR.accept_probability(1.0, 4.0) == 1.0 and UR.accept_probability(4.0, 1.0) == 0.25 and UR.accept_probability(2.0, 2.0) == 1.0
    assert UR.accept_probability(1.0, 0.0) == 0.0
    assert abs(UR.accept_probability(3.0, 1.0) - 1.0 / 3.0) <= 2.0 ** -32
    # u is never 0 and never 1: equal weights always accept, a proposal of weight 0 never does
    u = UR.uniform(5, np.arange(1000), 12345)
    assert ((u > 0) & (u < 1)).all() and UR.accepts(u, 1.0, 1.0).all() and not UR.accepts(u, 1.0, 0.0).any()
    assert abs(u.mean() - 0.5) < 0.05 and len(np.unique(u)) == 1000
    # the chain of held weights
    acc, old = UR.chain([1.0, 1.0], np.asarray([[0.5, 2.0], [0.0, 1.0], [0.5, 4.0]]), np.asarray([[0.6, 0.9], [0.1, 0.4], [0.4, 0.9]]))
    assert acc.tolist() == [[False, True], [False, True], [True, True]] and old.tolist() == [[1.0, 1.0], [1.0, 2.0], [1.0, 1.0]]
