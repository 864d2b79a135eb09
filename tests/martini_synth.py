"""Deterministic synthetic MARTINI systems for the tests (NumPy only): sizes, boxes and type tables that the
1 280-bead bilayer of tests/golden/martini never reaches.

``make`` returns the arrays that ``MartiniSystem``, ``oracle.martini_oracle`` and ``MartiniLangevinOracle`` take;
``check`` asserts what the comparisons built on them rely on; ``get(name)`` holds the systems the test files name.

Geometry.  Beads sit on a cubic lattice with uniform jitter of at most +-0.04 nm per component.  The lattice constant
is 0.5 nm stretched per axis to ``edge / floor(edge / 0.5)`` (so 0.5 nm exactly for an edge that is a multiple of it,
under 0.6 nm otherwise): the lattice is then periodic with the box and no pair can come closer than 0.42 nm.  Sites are
filled outwards from a set of centres, in the order of their periodic distance to the nearest centre plus 1.5 lattice
constants of noise: one centre on the corner of the box for an ordinary system - a sparse system is then a ragged blob
across all three pairs of faces and still has the neighbours a cut-off of 1.1 nm needs, a dense one fills the box -,
eight centres for a dilute one, four of which lie on a face, an edge or the corner.

Topology.  Chains of 3-5 lattice neighbours, straight (theta ~ pi - 0.1...0.3 with the jitter, where the harmonic
form's 1/sin(theta) matters) or with one right-angle turn (theta ~ pi/2); bonds along the chain, angles on consecutive
triplets.  From 27 beads on, a hub with 8 bonds (its 6 nearest and 2 next-nearest sites) and 12 angle memberships (8 as
the centre - straight, 90 and 135 degrees -, 2 as the first and 2 as the last bead), the limits of the kernels' incidence
lists.  Bead indices run against the order of placement, so the hub is bead n - 1: the last bead of the last, partial
tile or workgroup.  Every second bond and every third angle is listed backwards.
"""

from __future__ import annotations

import functools

import numpy as np

A0 = 0.5  # nm, lattice constant before stretching
JITTER = 0.04
R_CUT = 1.1
THETA0 = (np.pi, 2.3, 1.7)
MIN_SIN = 0.02


def _unit(axis, sign=1):
    v = np.zeros(3, dtype=np.int64)
    v[axis] = sign
    return v


def _centres(dims, dilute):
    nx, ny, nz = dims
    if not dilute:
        return np.array([[0, 0, 0]])
    return np.array([[0, 0, 0], [0, ny // 2, nz // 3], [nx // 2, 0, 2 * nz // 3], [nx // 3, ny // 3, 0],
                     [nx // 2, ny // 2, 0], [nx // 4, 3 * ny // 4, nz // 2], [3 * nx // 4, ny // 4, nz // 3],
                     [2 * nx // 3, 2 * ny // 3, 3 * nz // 4]])


def _topology(dims, n, centres, rng):
    """Sites (n, 3), bonds, angles, in the order of placement."""
    dims = np.asarray(dims, dtype=np.int64)
    occ = {}
    sites, bonds, angles = [], [], []

    def key(s):
        return tuple(int(v) for v in np.mod(s, dims))

    def place(s):
        k = key(s)
        assert k not in occ
        occ[k] = len(sites)
        sites.append(k)
        return occ[k]

    if n >= 27:
        assert (dims >= 5).all(), "the hub's arms need five sites per edge"
        c = centres[0]
        hub = place(c)
        ex, ey, ez = _unit(0), _unit(1), _unit(2)
        near = [ex, -ex, ey, -ey, ez, -ez]
        p = [place(c + d) for d in near] + [place(c + ex + ey), place(c - ey + ez)]
        bonds += [(hub, q) for q in p]
        # the hub as the centre: three straight angles, three right ones, two of 135 degrees
        angles += [(p[0], hub, p[1]), (p[2], hub, p[3]), (p[4], hub, p[5]), (p[0], hub, p[2]), (p[2], hub, p[4]),
                   (p[6], hub, p[4]), (p[6], hub, p[1]), (p[7], hub, p[2])]
        # four arms one site longer: the hub as the first bead of two angles and as the last bead of two
        for k, arm in enumerate((0, 1, 2, 4)):
            q = place(c + 2 * near[arm])
            bonds.append((p[arm], q))
            angles.append((hub, p[arm], q) if k < 2 else (q, p[arm], hub))

    grid = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    dist = np.full(grid.shape[0], np.inf)
    for c in centres:
        d = grid - c
        d = d - dims * np.round(d / dims)
        dist = np.minimum(dist, np.sqrt((d * d).sum(1)))
    order = np.argsort(dist + rng.uniform(0.0, 1.5, size=grid.shape[0]), kind="stable")
    for s in grid[order]:
        if len(sites) >= n:
            break
        if key(s) in occ:
            continue
        length = min(int(rng.integers(3, 6)), n - len(sites))
        bent = rng.random() < 0.4
        axis, sign = int(rng.integers(3)), int(rng.choice([-1, 1]))
        step = _unit(axis, sign)
        cur = np.array(s)
        chain = [place(cur)]
        for k in range(1, length):
            if bent and k == 2:
                step = _unit((axis + 1 + int(rng.integers(2))) % 3, int(rng.choice([-1, 1])))
            tries = [step] + [_unit(a, sg) for a in rng.permutation(3) for sg in (1, -1)]
            nxt = next((t for t in tries if key(cur + t) not in occ), None)
            if nxt is None:
                break
            step, cur = nxt, cur + nxt
            chain.append(place(cur))
        bonds += list(zip(chain[:-1], chain[1:]))
        angles += list(zip(chain[:-2], chain[1:-1], chain[2:]))
    assert len(sites) == n, "the lattice of this box has too few sites"
    return np.array(sites, dtype=np.int64), np.array(bonds, dtype=np.int64).reshape(-1, 2), np.array(angles, dtype=np.int64).reshape(-1, 3)


def _pair_table(n_types, lo, hi, rng):
    """Symmetric (T, T) table with a distinct value for every unordered pair, evenly spaced over [lo, hi]."""
    iu = np.triu_indices(n_types)
    vals = lo + (hi - lo) * rng.permutation(iu[0].shape[0]) / max(1, iu[0].shape[0] - 1)
    t = np.zeros((n_types, n_types))
    t[iu] = vals
    return np.maximum(t, t.T)


def _min_image(d, box):
    return d - box * np.round(d / box)


def _sin_theta(pos, box, angles):
    """(F, n_angles) sine of every angle, minimum image per frame."""
    u = _min_image(pos[:, angles[:, 0]] - pos[:, angles[:, 1]], box[:, None, :])
    v = _min_image(pos[:, angles[:, 2]] - pos[:, angles[:, 1]], box[:, None, :])
    cr = np.cross(u, v)
    return np.sqrt((cr * cr).sum(-1)) / np.sqrt((u * u).sum(-1) * (v * v).sum(-1))


def make(n, box, *, seed, n_types=7, used_types=(1, 4, 6), frames=1, images=0, box_jitter=0.0, dilute=None):
    """-> dict: n, types (n,), sigma / eps (T, T), bonds (nb, 2), bond_k / bond_r0 (nb,), angles (na, 3), angle_k /
    angle_t0 (na,), mass (n,), pos (frames, n, 3), box (frames, 3), shift (n, 3) - the whole box edges added to every
    bead (``images``) -, r_cut.  ``dilute``: several blobs instead of one; by default from 100 beads on when the lattice has more
    than 50 sites per bead."""
    rng = np.random.default_rng(seed)
    box0 = np.asarray(box, dtype=np.float64).reshape(3)
    dims = np.floor(box0 / A0 + 1e-9).astype(np.int64)
    assert (box0 >= 2.0 * R_CUT).all() and (dims >= 3).all(), "one minimum image per pair needs edges of 2 r_c"
    if dilute is None:
        dilute = n >= 100 and int(dims.prod()) > 50 * n
    sites, bonds, angles = _topology(dims, n, _centres(dims, dilute), rng)
    # indices against the order of placement: the hub becomes bead n - 1
    sites = sites[::-1].copy()
    bonds, angles = n - 1 - bonds, n - 1 - angles
    bonds[1::2] = bonds[1::2, ::-1]
    angles[2::3] = angles[2::3, ::-1]

    frac = (sites + 0.25) / dims  # the faces of the box lie between the last and the first site of an edge
    scale = 1.0 + box_jitter * rng.uniform(-1.0, 1.0, size=(frames, 3))
    boxes = box0 * scale
    jit = rng.uniform(-JITTER, JITTER, size=(frames, n, 3))
    for _ in range(100):  # (re-draw the centre bead of an angle that came out straight)
        pos = (frac * box0 + jit) * scale[:, None, :]
        if angles.shape[0] == 0:
            break
        f, a = np.nonzero(_sin_theta(pos, boxes, angles) < 1.5 * MIN_SIN)
        if f.size == 0:
            break
        jit[f, angles[a, 1]] = rng.uniform(-JITTER, JITTER, size=(f.size, 3))
    else:
        raise AssertionError("could not bend every angle away from pi")
    shift = rng.integers(-images, images + 1, size=(n, 3)) if images else np.zeros((n, 3), dtype=np.int64)
    pos = pos + shift * boxes[:, None, :]

    used = np.asarray(used_types, dtype=np.int32)
    assert used.min() >= 0 and used.max() < n_types and len(set(used.tolist())) == used.size < n_types
    nb, na = bonds.shape[0], angles.shape[0]
    out = dict(
        n=int(n), r_cut=R_CUT,
        types=used[rng.integers(0, used.size, size=n)].astype(np.int32),
        sigma=_pair_table(n_types, 0.43, 0.62, rng), eps=_pair_table(n_types, 2.0, 5.6, rng),
        bonds=bonds.astype(np.int32), bond_k=rng.uniform(1000.0, 5000.0, size=nb), bond_r0=rng.uniform(0.4, 0.55, size=nb),
        angles=angles.astype(np.int32), angle_k=rng.uniform(20.0, 45.0, size=na),
        angle_t0=np.asarray(THETA0)[rng.integers(0, 3, size=na)],
        mass=rng.uniform(40.0, 90.0, size=n), pos=pos, box=boxes, shift=shift,
    )
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pair_distances(x, box, block=512):
    """Yields (i0, r (b, n)) over blocks of rows: the minimum-image distance of every pair, inf on the diagonal."""
    n = x.shape[0]
    for i0 in range(0, n, block):
        d = _min_image(x[i0:i0 + block, None, :] - x[None, :, :], box)
        r = np.sqrt((d * d).sum(-1))
        r[np.arange(r.shape[0]), i0 + np.arange(r.shape[0])] = np.inf
        yield i0, r


def bonded_mask(system):
    n = system["n"]
    m = np.zeros((n, n), dtype=bool)
    b = system["bonds"]
    m[b[:, 0], b[:, 1]] = m[b[:, 1], b[:, 0]] = True
    return m


def check(system) -> None:
    """The conditions the comparisons rely on (every frame); memoised per system, the arrays are read-only."""
    from scipy.spatial import cKDTree  # (the pairs inside the cut-off; ``make`` itself is NumPy only)

    if system.get("_checked"):
        return
    n, bonds, angles = system["n"], system["bonds"].astype(np.int64), system["angles"].astype(np.int64)
    n_bonds = np.bincount(bonds.ravel(), minlength=n)
    n_angles = np.bincount(angles.ravel(), minlength=n)
    assert n_bonds.max(initial=0) <= 8 and n_angles.max(initial=0) <= 12
    assert (bonds[:, 0] != bonds[:, 1]).all() and len({(min(a, b), max(a, b)) for a, b in bonds}) == bonds.shape[0]
    if bonds.shape[0] > 1:
        assert (bonds[:, 0] < bonds[:, 1]).any() and (bonds[:, 0] > bonds[:, 1]).any()
    bm = bonded_mask(system)
    if n >= 27:
        assert n_bonds.max() == 8 and n_angles.max() == 12
        hub = int(np.argmax(n_bonds))
        roles = {r for a in angles for r in range(3) if a[r] == hub}
        assert n_angles[hub] == 12 and roles == {0, 1, 2}
    for f in range(system["pos"].shape[0]):
        x, box = system["pos"][f], system["box"][f]
        half = 0.5 * box

        def clear_of_half(d):
            assert (np.abs(np.abs(d) - half) > 1e-6).all(), "a displacement component at half the box"

        if bonds.shape[0]:
            d = _min_image(x[bonds[:, 0]] - x[bonds[:, 1]], box)
            assert np.sqrt((d * d).sum(1)).min() >= 0.3
            clear_of_half(d)
        if angles.shape[0]:
            assert _sin_theta(x[None], box[None], angles).min() >= MIN_SIN
            clear_of_half(_min_image(x[angles[:, 0]] - x[angles[:, 1]], box))
            clear_of_half(_min_image(x[angles[:, 2]] - x[angles[:, 1]], box))
        xw = np.mod(x, box)  # a pair crosses a face when its minimum image is not the difference of the wrapped beads
        xw[xw >= box] = 0.0
        pi, pj = cKDTree(xw, boxsize=box).query_pairs(R_CUT, output_type="ndarray").T
        raw = xw[pi] - xw[pj]
        d = _min_image(raw, box)
        assert (d * d).sum(1).min(initial=np.inf) >= 0.38**2, "two beads closer than 0.38 nm"
        lj = ~bm[pi, pj]
        clear_of_half(d[lj])
        n_lj = int(lj.sum())
        lj_cross = (np.abs(raw - d) > 0.5 * box)[lj].any(0)
        if n >= 27:
            assert n_lj >= 4 * n, (n_lj, n)
            db = xw[bonds[:, 0]] - xw[bonds[:, 1]]
            assert (np.abs(db - _min_image(db, box)) > 0.5 * box).any(0).all(), "no bond across a face in x, y and z"
            assert lj_cross.all(), "no LJ pair across a face in x, y and z"
    system["_checked"] = True


# The systems the tests name.  Boxes are non-cubic; edges that are no multiple of 0.5 nm stretch the lattice.
SYSTEMS = {
    # energy path, section (a): one tile or less, one bead over a tile, a partial fifth tile
    "n1": dict(n=1, box=(2.5, 3.0, 3.5), seed=101, images=2),
    "n2": dict(n=2, box=(2.5, 3.0, 3.5), seed=102, images=2),
    "n65": dict(n=65, box=(2.5, 2.7, 3.0), seed=165, images=2),
    "n255": dict(n=255, box=(3.0, 3.5, 3.7), seed=255, images=2),
    "n257": dict(n=257, box=(3.0, 3.5, 3.7), seed=257, images=2),
    "n1100": dict(n=1100, box=(5.0, 5.5, 6.2), seed=1100, images=2),
    # (b) eight tiles, the last of 208 beads; 17 frames with their own boxes
    "n2000": dict(n=2000, box=(6.5, 6.7, 7.0), seed=2000, frames=17, box_jitter=0.01),
    # (c) one three-bead chain over more frames than one launch takes
    "n3": dict(n=3, box=(3.0, 3.5, 4.0), seed=3, frames=4100, box_jitter=0.01),
    # MD path: (e) all-pairs builder under 512 beads, (f) cells + direct table, (g) slab: two cells in z, (h) hashed table
    "md37": dict(n=37, box=(2.7, 3.0, 3.4), seed=37, images=2),
    "md1285": dict(n=1285, box=(5.5, 6.0, 5.7), seed=1285, images=1),
    "slab1285": dict(n=1285, box=(7.5, 7.6, 3.0), seed=1286, images=1),
    "dilute520": dict(n=520, box=(24.0, 24.0, 24.0), seed=520, images=1),
}


@functools.lru_cache(maxsize=None)
def get(name: str) -> dict:
    return make(**SYSTEMS[name])


def oracle_args(system, frame=0, cast=None):
    """(pos, box, types, sigma, eps, bonds, bond_k, bond_r0, angles, angle_k, angle_t0) as the oracle takes them, float64
    torch tensors; ``cast`` (a numpy dtype): every real rounded to it first and widened back."""
    import torch

    r = (lambda a: np.asarray(a).astype(cast).astype(np.float64)) if cast is not None else (lambda a: np.asarray(a, dtype=np.float64))
    t = lambda a: torch.as_tensor(r(a).copy())  # noqa: E731
    s = system
    return (t(s["pos"][frame]), t(s["box"][frame]), s["types"].copy(), t(s["sigma"]), t(s["eps"]), s["bonds"].copy(), t(s["bond_k"]),
            t(s["bond_r0"]), s["angles"].copy(), t(s["angle_k"]), t(s["angle_t0"]))
