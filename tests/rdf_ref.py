"""NumPy brute force of the pair-distance histogram behind g(r): the restatement the RDF tests compare the kernel's
counts with, EXACTLY.  Double precision, every ordered pair as a dense |A| x |B| table per frame.

The rule: every ordered pair (i in a, j in b) with i != j and, where ``block`` is given, block[i] != block[j]; r is the
length of d - L rint(d / L) over x, y, z (``dims="xyz"``) or x, y (``"xy"``) with the frame's own box; r < r_max adds 1 to
bin floor(r n_bins / r_max), at most n_bins - 1.

Exact comparison is fair only where no pair sits within rounding of a bin edge or of r_max, so ``counts`` also returns
the MARGIN: with u = r n_bins / r_max, the smallest |u - e| over the admissible pairs and the edges e = 1 ... n_bins (edge
0 cannot be crossed: r >= 0), pairs beyond r_max included.  The tests assert margin > 1e-7 (bin widths): a difference of
an ulp or two between host and device in the image or the square root (1e-16 relative) then moves no pair.
"""

from __future__ import annotations

import math

import numpy as np

MIN_MARGIN = 1e-7  # bin widths


def admissible(a, b, block=None) -> np.ndarray:
    """(|a|, |b|) bool: the ordered pairs the rule admits."""
    a, b = np.asarray(a), np.asarray(b)
    ok = a[:, None] != b[None, :]
    if block is not None:
        block = np.asarray(block)
        ok &= block[a][:, None] != block[b][None, :]
    return ok


def distances(x, box, a, b, dims="xyz") -> np.ndarray:
    """(|a|, |b|) minimum-image distances of one frame x (n, 3) under box (3,)."""
    k = {"xyz": 3, "xy": 2}[dims]
    d = x[np.asarray(a)][:, None, :k] - x[np.asarray(b)][None, :, :k]
    d = d - box[:k] * np.rint(d / box[:k])
    return np.sqrt((d * d).sum(-1))


def counts(x, box, a, b, n_bins, r_max, block=None, dims="xyz"):
    """x (F, n, 3), box (F, 3) float64 -> ((F, n_bins) int64 counts, margin in bin widths)."""
    x, box = np.asarray(x, dtype=np.float64), np.asarray(box, dtype=np.float64)
    ok = admissible(a, b, block)
    out = np.zeros((x.shape[0], n_bins), dtype=np.int64)
    margin = math.inf
    for f in range(x.shape[0]):
        r = distances(x[f], box[f], a, b, dims)[ok]
        u = r * n_bins / r_max
        edge = np.rint(u)
        near = (edge >= 1) & (edge <= n_bins)
        if near.any():
            margin = min(margin, float(np.abs(u - edge)[near].min()))
        hit = r < r_max
        bins = np.minimum(np.floor(u[hit]).astype(np.int64), n_bins - 1)
        out[f] = np.bincount(bins, minlength=n_bins)
    return out, margin


def shells(n_bins, r_max, dims="xyz") -> np.ndarray:
    e = np.arange(n_bins + 1, dtype=np.float64) * (r_max / n_bins)
    if dims == "xyz":
        return 4.0 / 3.0 * math.pi * (e[1:] ** 3 - e[:-1] ** 3)
    return math.pi * (e[1:] ** 2 - e[:-1] ** 2)


def g_of(c, box, n_pairs, r_max, dims="xyz") -> np.ndarray:
    """g[f, b] = counts[f, b] V_f / (N_pairs v_b) with the frame's own volume (area for ``xy``)."""
    box = np.asarray(box, dtype=np.float64)
    volume = box[:, 0] * box[:, 1] * (box[:, 2] if dims == "xyz" else 1.0)
    return c.astype(np.float64) * volume[:, None] / (float(n_pairs) * shells(c.shape[1], r_max, dims))[None, :]
