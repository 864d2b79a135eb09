"""The periodic oxDNA configurations of tests/oxdna_periodic_synth.py on the host: what tests/test_gpu_periodic_md.py
relies on.  The oracle is a valid reference across faces (its energies and gradients of a crossing helix are those of
the whole golden frame), the lattices reach the cell grids they are meant for, a good share of their pairs needs an
image along every axis, and no contact is singular."""

import numpy as np
import pytest
import torch

from mythos_amd.simulators.neighbors import verlet_pairs_numpy
from oracle import oxdna_oracle as orc
from tests import helpers as H
from tests import oxdna_periodic_synth as S


def _oracle(model, top, c, q, box, pairs, hce=False):
    tt = (torch.as_tensor(top.seq, dtype=torch.long), torch.as_tensor(top.is_end, dtype=torch.long),
          torch.as_tensor(top.bonded_neighbors, dtype=torch.long).reshape(-1, 2), torch.as_tensor(pairs, dtype=torch.long).reshape(-1, 2))
    ct, qt = torch.as_tensor(c), torch.as_tensor(q)
    if model == 4:
        P, rna = H.oracle_params_na1(), torch.as_tensor(S.is_rna(top))
        e = orc.energy_terms_na1(P, ct, qt, tt[0], rna, *tt[1:], box=box)
        _, gc, gq = orc.energy_and_grads_na1(P, ct, qt, tt[0], rna, *tt[1:], box=box)
    else:
        P = H.oracle_params(model, salt=S.SALT[model], half_charged_ends=hce)
        e = orc.energy_terms(model, P, ct, qt, *tt, box=box)
        _, gc, gq = orc.energy_and_grads(model, P, ct, qt, *tt, box=box)
    return e.numpy(), gc.numpy(), gq.numpy()


@pytest.mark.parametrize(("model", "name"), S.CROSSING)
def test_crossing_helix_has_the_energies_and_gradients_of_the_whole_frame(model, name):
    top, c0, q, box, move = S.placement(model, name)
    _, c, _, _ = S.crossing_helix(model, name)
    np.testing.assert_array_equal(c, c0 + move)
    n0 = int(top.strand_counts[0])
    # the molecule straddles a face of every axis (nucleotides on both sides), and every pair between the strands
    # goes through an image in all three components; in the ring two bonded pairs do as well
    face = box * np.array([1.0, 0.0, 1.0])
    shifted = c0 + move[0]
    for a in range(3):
        assert (shifted[:, a] < face[a]).sum() >= 2 and (shifted[:, a] > face[a]).sum() >= 2, (a, shifted[:, a])
    cross = np.array([(i, j) for i in range(n0) for j in range(n0, top.n_nucleotides)])
    img = np.abs(S.image_of_pairs(c, cross, box))  # (the moved half of the ring is two edges from the second strand)
    assert (img >= 1).all() and (img <= (2 if name == "circular" else 1)).all()
    bonded = np.asarray(top.bonded_neighbors).reshape(-1, 2)
    n_bonded_images = int((S.image_of_pairs(c, bonded, box) != 0).any(1).sum())
    assert n_bonded_images == (2 if name == "circular" else 0)
    assert np.abs(move).max() <= 2.0 * box.max() + 1e-9 and np.array_equal(move * S.GRID, np.round(move * S.GRID))
    e_ref, gc_ref, gq_ref = _oracle(model, top, c0, q, box, top.unbonded_neighbors)
    e, gc, gq = _oracle(model, top, c, q, box, top.unbonded_neighbors)
    print(f"{model} {name}: terms differ by {np.abs(e - e_ref).max():.1e}, dU/dc by {np.abs(gc - gc_ref).max():.1e} of "
          f"{np.abs(gc_ref).max():.3g}, dU/dq by {np.abs(gq - gq_ref).max():.1e} of {np.abs(gq_ref).max():.3g}")
    assert np.abs(e_ref).max() > 1.0
    np.testing.assert_allclose(e, e_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gc, gc_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(gq, gq_ref, rtol=0, atol=1e-10)


@pytest.mark.parametrize(("box_x", "nc"), [(13.0, (3, 10, 3)), (11.0, (2, 10, 3))])
def test_duplex_lattice_reaches_its_cell_grid_and_crosses_every_face(box_x, nc):
    top, c, q, box = S.duplex_lattice(box_x)
    assert top.n_nucleotides == S.LATTICE_N >= 512 and np.array_equal(box, [box_x, 39.0, 13.0])
    assert S.cells_per_edge(box) == nc
    again = S.duplex_lattice(box_x)
    assert np.array_equal(again[1], c) and np.array_equal(again[2], q)
    bonded = np.asarray(top.bonded_neighbors)
    pairs = verlet_pairs_numpy(c, bonded, 3.9, box=box)
    img = S.image_of_pairs(c, pairs, box)
    through = (img != 0).any(1)
    print(f"box_x {box_x}: {len(pairs)} pairs within 3.9, {int(through.sum())} through an image "
          f"(x {int((img[:, 0] != 0).sum())}, y {int((img[:, 1] != 0).sum())}, z {int((img[:, 2] != 0).sum())})")
    assert len(pairs) > 5000 and through.mean() >= 0.05
    # listed pairs whose members lie on either side of a face, per axis; folded into the box they need an image there
    side = np.floor(c / box).astype(np.int64)
    straddle = side[pairs[:, 0]] != side[pairs[:, 1]]
    print(f"box_x {box_x}: pairs across a face of x, y, z: {straddle.sum(0).tolist()}")
    assert (straddle.sum(0) >= 20).all()
    # unwrapped coordinates that leave the box on every axis; folding them breaks molecules (bonded pairs through images)
    w = S.wrapped(c, box)
    assert ((c < 0) | (c >= box)).any(0).all() and (w >= 0).all() and (w < box).all()
    assert (S.image_of_pairs(w, bonded, box) != 0).any(1).sum() >= 10
    assert ((S.image_of_pairs(w, pairs, box) != 0).sum(0) >= 20).all()
    assert np.array_equal(verlet_pairs_numpy(w, bonded, 3.9, box=box), pairs)
    e, gc, gq = _oracle(2, top, c, q, box, pairs, hce=True)
    e_w, _, _ = _oracle(2, top, w, q, box, pairs, hce=True)
    np.testing.assert_allclose(e_w, e, rtol=1e-12, atol=1e-12)
    # what the images carry: between the unwrapped duplexes only the Debye-Hueckel tail across the 2.2-unit gap along z
    # (their other contacts are whole), in the folded configuration every term of the duplexes cut by a face
    e_free, _, _ = _oracle(2, top, c, q, None, pairs, hce=True)
    e_free_w, _, _ = _oracle(2, top, w, q, None, pairs, hce=True)
    print(f"box_x {box_x}: without the box the energies change by {np.abs(e_free - e).max():.2g} (unwrapped), {np.abs(e_free_w - e).max():.3g} (folded)")
    assert np.abs(e_free - e).max() > 1e-5 and (np.abs(e_free_w - e)[[0, 2, 4, 5]] > 1.0).all()
    tau = orc.quat_grad_to_body_torque(torch.as_tensor(q), torch.as_tensor(gq)).numpy()
    for f in (gc, tau):
        rms = np.sqrt((f**2).mean())
        print(f"box_x {box_x}: rms {rms:.3g}, largest {np.abs(f).max():.4g}")
        assert rms > 1.0 and np.abs(f).max() < 200.0 * rms  # something to compare, and no singular contact
