"""What tests/test_gpu_energy_shapes.py relies on, on the host (tests/oxdna_energy_shapes.py): the row layout of
``set_neighbors`` restated, every segment position of every (system, cap) holding a pair the oracle feels - a dropped
segment would otherwise be a segment of zeros -, in the crossing systems a pair that needs an image in a later segment,
and the arithmetic of the two chunk rules with the frame counts the chunk tests use."""

import numpy as np
import pytest

from tests import oxdna_energy_shapes as E
from tests import oxdna_periodic_synth as S

ALL = E.SYSTEMS + ((2, E.LONG),)
IDS = [E.system_id(m, n) for m, n in ALL]


def _caps(name, lens):
    return E.long_caps(lens) if name == E.LONG else E.caps(lens)


@pytest.mark.parametrize(("model", "name"), ALL, ids=IDS)
def test_rows_are_the_bonded_slots_then_the_pairs_in_list_order(model, name):
    top, _, _, _ = E.system_frames(model, name, "mid")
    pairs = E.pair_list(top)
    rows, lens = E.rows_of(top, pairs)
    n = int(top.n_nucleotides)
    assert sorted(map(tuple, np.sort(pairs, 1))) == sorted(map(tuple, np.sort(np.asarray(top.unbonded_neighbors).reshape(-1, 2), 1)))  # a permutation
    # strides and lengths: all pairs but the bonded ones, so 17 / 18 places for 16 nt (two bonded partners / one) in a stride of 32
    bonded = np.asarray(top.bonded_neighbors).reshape(-1, 2)
    n_bonded = np.bincount(bonded.reshape(-1), minlength=n)
    assert np.array_equal(lens, E.BONDED_SLOTS + (n - 1) - n_bonded)
    assert rows.shape[1] % 16 == 0 and lens.max() <= rows.shape[1] < lens.max() + 16
    assert rows.shape[1] == {16: 32, 24: 32, 120: 128}[n] and sorted(set(lens.tolist())) == [n + 1, n + 2]
    # bonded slots: partner j of a bond (i, j) in an odd slot of row i, i in an even slot of row j; a second bond of the same role (a ring) in slots 2 / 3
    slots = rows[:, :E.BONDED_SLOTS]
    for i, j in bonded:
        assert j in slots[i, 1::2] and i in slots[j, 0::2]
    assert (slots >= 0).sum() == 2 * len(bonded) and ((slots[:, 2:] >= 0).any() == (name == "circular"))
    # entries: replaying the list gives each row's entries in order, i receives j and j receives i | ROLE_Q
    want = [[] for _ in range(n)]
    for i, j in pairs:
        want[i].append(int(j))
        want[j].append(int(i) | E.ROLE_Q)
    for i in range(n):
        assert rows[i, E.BONDED_SLOTS:lens[i]].tolist() == want[i] and (rows[i, lens[i]:] == -1).all()
    # the caps come from the lengths: 8, interior rows exactly one segment (end rows a tail of one), end rows exactly full
    caps = E.caps(lens)
    assert caps == (8, n - 3, n - 2, 0) and all(c == 0 or E.CAP_MIN <= c <= E.CAP_MAX for c in caps)
    assert all(E.is_segmented(rows.shape[1], c) for c in caps[:-1]) and not E.is_segmented(rows.shape[1], 0)
    interior, end = int(lens.min()), int(lens.max())
    assert [b - a for a, b in E.segments(interior, caps[1])] == [caps[1]] and [b - a for a, b in E.segments(end, caps[1])] == [caps[1], 1]
    assert [b - a for a, b in E.segments(end, caps[2])] == [caps[2]] and [b - a for a, b in E.segments(interior, caps[2])] == [caps[2] - 1]
    assert len(E.segments(end, 8)) == (15 if n == 120 else 3 if n == 24 else 2) and E.segments(end, 8)[-1][1] - E.segments(end, 8)[-1][0] < 8


@pytest.mark.parametrize("place", E.PLACES)
@pytest.mark.parametrize(("model", "name"), ALL, ids=IDS)
def test_every_segment_position_holds_a_pair_the_oracle_feels(model, name, place):
    top, c, q, box = E.system_frames(model, name, place)
    pairs = E.pair_list(top)
    rows, lens = E.rows_of(top, pairs)
    energy = E.pair_energies(model, name, top, c[0], q[0], pairs, box)
    image = (S.image_of_pairs(c[0], pairs, box) != 0).any(1)
    if place == "crossing" and name != E.LONG:
        n0 = int(top.strand_counts[0])
        assert image[(pairs[:, 0] < n0) != (pairs[:, 1] < n0)].all()  # every pair between the strands
    else:
        assert not image.any()
    live, far = {}, {}
    for (i, j), e, m in zip(pairs.tolist(), energy, image):
        live[(i, j)] = live[(j, i)] = abs(e) > E.INTERACTS
        far[(i, j)] = far[(j, i)] = bool(m)
    assert sum(live.values()) // 2 >= 20
    for cap in _caps(name, lens):
        if cap == 0:
            continue
        n_seg = max(len(E.segments(int(length), cap)) for length in lens)
        cover, first, last = np.zeros(n_seg, int), np.zeros(n_seg, int), np.zeros(n_seg, int)
        tails = live_tails = fulls = live_full_ends = late_images = 0
        for i, length in enumerate(lens):
            for k, (a, b) in enumerate(E.segments(int(length), cap)):
                partner = [int(rows[i, s]) & (E.ROLE_Q - 1) for s in range(a, b)]
                on = [live[(i, j)] for j in partner]
                cover[k] += any(on)
                first[k] += on[0]
                last[k] += on[-1]
                tails += b - a == 1
                live_tails += b - a == 1 and on[0]
                fulls += b - a == cap
                live_full_ends += b - a == cap and on[-1]
                late_images += k > 0 and any(o and far[(i, j)] for o, j in zip(on, partner))
        print(f"{E.system_id(model, name)} {place} cap {cap}: rows with a live pair per segment {cover.tolist()}, live first entries "
              f"{first.tolist()}, live last entries {last.tolist()}, live single-entry tails {live_tails} of {tails}, "
              f"live ends of full segments {live_full_ends} of {fulls}, later segments with a live image pair {late_images}")
        # every segment index, and the first and the last place of it, hold an interacting pair for some nucleotide
        assert (cover > 0).all() and (first > 0).all() and (last > 0).all()
        assert fulls > 0 and live_full_ends > 0
        if cap == int(lens.min()) - E.BONDED_SLOTS:
            assert tails == int((lens == lens.max()).sum()) and live_tails > 0
        if place == "crossing" and name != E.LONG and n_seg > 1:
            assert late_images > 0


def test_chunk_rules_and_the_frame_counts_of_the_chunk_tests():
    width = E.param_count()
    assert 200 < width < 400
    # the 16-nt calls are cut by the grid, whatever the row width; the 120-nt dU/dtheta call by the 256 MiB of partials
    assert E.energy_chunk(16, False) == E.energy_chunk(16, True) == E.GRID_Y == 65535
    long = E.energy_chunk(120, True)
    assert long == (256 << 20) // (4 * width * 8) and 30000 < long < 35000 and E.energy_chunk(120, False) == 65535
    assert E.energy_chunk(16, True, param_sets=3) == (256 << 20) // (3 * width * 8) < 65535  # (oxNA: three vectors; no chunk case of its own)
    assert E.energy_chunk(32 * 10**6, True) == 1
    # the sweep: 64 MiB of (tiles, 128 temperatures, 6 columns) partials; a table of 129 is two passes of the same chunk
    sweep = E.sweep_chunk(16, 129, True)
    assert sweep == E.sweep_chunk(16, 128, True) == (64 << 20) // (128 * 6 * 8) == 10922
    assert E.sweep_chunk(16, 129, False) == 65535 and E.sweep_chunk(120, 5, True) == 65535
    kts = E.sweep_kts(0.0987)
    assert len(kts) == E.SWEEP_MAX_T + 1 and kts[0] == 0.0987 and kts[127] == E.KT_LOW and kts[:127].argmax() == 126 and kts[128] > 0.1
    assert all(126 in s or min(s) >= 128 for s in E.SWEEP_T_SLICES) and {0, 1, 127, 128} <= set(E.SWEEP_T_ORACLE) and len(E.SWEEP_T_ORACLE) == 7
    for chunk in (65535, long, sweep):
        n_frames = chunk + E.TAIL
        seen = E.boundary_frames(chunk, n_frames)
        assert {0, chunk - 1, chunk, n_frames - 1} <= set(seen) and len(seen) == 8 and max(seen) < n_frames
        a, b, c = E.slices(chunk, n_frames)
        assert a.stop <= chunk and b.start < chunk < b.stop and c.start >= chunk and c.stop == n_frames


def test_synthetic_frames_are_the_same_whichever_call_asks_for_them():
    top, c, q, box = E.synthetic_frames(2, "simple-helix", "mid", 350)
    assert c.shape == (350, 16, 3) and q.shape == (350, 16, 4) and np.allclose(np.linalg.norm(q, axis=-1), 1.0, atol=1e-14)
    idx = np.array([0, 99, 100, 249, 349])
    _, c2, q2, _ = E.synthetic_frames(2, "simple-helix", "mid", idx)
    assert np.array_equal(c2, c[idx]) and np.array_equal(q2, q[idx])
    # distinct frames: the same golden frame under another seed differs, by the noise asked for
    gold = np.asarray(E._golden(2, "simple-helix")[1].center)
    assert 0.008 < (c[:100] - gold[:100]).std() < 0.012 and 0.01 < np.abs(c[100:200] - c[:100]).mean() < 0.02
    assert len({a.tobytes() for a in c}) == 350
    _, cx, qx, _ = E.synthetic_frames(2, "simple-helix", "crossing", idx)
    assert np.array_equal(cx, c[idx] + S.placement(2, "simple-helix")[4]) and np.array_equal(qx, q[idx])
    # the shorter trajectory of the 120-nt duplex is walked round
    top_l, cl, _, _ = E.synthetic_frames(2, E.LONG, "mid", 120)
    assert cl.shape == (120, 120, 3) and len({a.tobytes() for a in cl}) == 120
