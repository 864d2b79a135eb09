"""Stretch-torsion observables and moduli (mythos/observables/stretch_torsion.py:16-230).

``TwistXY`` - the total twist of a duplex, the sum over adjacent base pairs of the angle between their base-base vectors
in the x-y plane (radians) - and ``ExtensionZ`` - the |z| distance between the midpoints of two base pairs (oxDNA length
units) - are evaluated per frame by the HIP library (csrc/duplex_obs.hip).  ``stretch``, ``torsion`` and
``stretch_torsion`` (Assenza and Perez, JCTC 2022) are least-squares lines in closed form, torch fp64 on whatever device
their inputs are on, and differentiable."""

from __future__ import annotations

import numpy as np
import torch

from mythos_amd.observables import base as B


class TwistXY(B.DuplexObservable):
    def __init__(self, quartets, displacement_fn, geometry: dict, model: int = 2):
        self.quartets = np.asarray(quartets, dtype=np.int64).reshape(-1, 2, 2)
        self.displacement_fn, self.geometry, self.model = displacement_fn, geometry, model

    def __call__(self, trajectory) -> torch.Tensor:
        """(n_states,) total twist in radians."""
        return self.rows(trajectory)[:, B.COL_TWIST]


class ExtensionZ(B.DuplexObservable):
    def __init__(self, bp1, bp2, displacement_fn):
        self.bp1, self.bp2 = np.asarray(bp1, dtype=np.int64).reshape(2), np.asarray(bp2, dtype=np.int64).reshape(2)
        self.end_pairs = np.concatenate([self.bp1, self.bp2])
        self.displacement_fn = displacement_fn

    def __call__(self, trajectory) -> torch.Tensor:
        """(n_states,) extension in simulation units."""
        return self.rows(trajectory)[:, B.COL_EXTENSION]


def _t(x):
    return x.to(torch.float64) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def _line(x, y):
    """Least-squares (slope, offset) of y against x."""
    x, y = _t(x), _t(y).to(_t(x).device)
    xm, ym = x.mean(), y.mean()
    slope = ((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum()
    return slope, ym - slope * xm


def stretch(forces, extensions):
    """-> (a1, l0, s_eff): slope and offset of the linear force-extension fit and the effective stretch modulus l0 / a1
    (l0 is fitted, not fixed to the extension at zero force)."""
    a1, l0 = _line(forces, extensions)
    return a1, l0, l0 / a1


def torsion(torques, extensions, twists):
    """-> (a3, a4): slopes of the linear fits of extension and twist against torque."""
    return _line(torques, extensions)[0], _line(torques, twists)[0]


def stretch_torsion(forces, force_extensions, torques, torque_extensions, torque_twists):
    """-> (s_eff, c, g): effective stretch modulus, torsional modulus, twist-stretch coupling."""
    a1, l0, s_eff = stretch(forces, force_extensions)
    a3, a4 = torsion(torques, torque_extensions, torque_twists)
    c = a1 * l0 / (a4 * a1 - a3**2)
    g = -(a3 * l0) / (a4 * a1 - a3**2)
    return s_eff, c, g
