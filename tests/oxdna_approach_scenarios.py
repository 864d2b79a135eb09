"""Two free complementary nucleotides (A, T; oxDNA2 at salt 0.5) that come into range of a term BETWEEN list builds, for
the skin guarantee of tests/test_gpu_oxdna_rows.py: at the build frame the pair is not in the class whose term acts
later, so only a rebuild forced by the displacement check of md_step_kernel can put it there in time (NumPy only).

``translation``     bases face each other, centres 2.6 apart at skin 0.6 - unlisted; opposite momenta bring them together
                    and the hydrogen bond switches on.  The centre clause of the check.
``base swing``      centres 1.35 apart at skin 0.2; nucleotide 1 starts half a turn away, about the axis through its centre
                    and its BACKBONE site, from facing nucleotide 0: base-base 1.03, outside the hydrogen bond's range +
                    skin.  Spinning about that axis leaves its centre and its backbone site where they are - only the
                    base site travels (0.57 sin(angle / 2)), so only the base-site clause can ask for the rebuild that
                    lists the pair as close before the hydrogen bond acts.
``backbone swing``  centres 2.5 apart at skin 0.2, bases pointing the same way: backbone-backbone 2.59, outside the
                    Debye-Hueckel range (2.29 with the default parameters) + skin - unlisted; nucleotide 1 turns about its
                    a3 and its backbone site comes within 1.82 of the other's (the base site never comes within reach of
                    anything): the backbone clause fires first, the backbone site being farther from the axis.

Tuned with oracle/langevin_oracle.py on the CPU: the hydrogen bond first acts at saved frame 169 (translation) and 147
(base swing), Debye-Hueckel at 116 (backbone swing); in the swings the centres have moved by less than 1e-3 by then.
"""

from __future__ import annotations

import dataclasses as dc
import types

import numpy as np

from mythos_amd.input.trajectory import axes_to_quaternion

DT = 0.003
KT = 1e-4          # small: the approach is the prescribed one
GAMMA_T = GAMMA_R = 1e-3
SEED = 0x5EED0A11
TERM_HB, TERM_DEBYE = 4, 7  # columns of the energy trace


def two_free_nucleotides():
    return types.SimpleNamespace(seq=np.array([0, 3], dtype=np.int32), is_end=np.ones(2, dtype=np.int32),
                                 bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                                 unbonded_neighbors=np.zeros((0, 2), dtype=np.int32), n_nucleotides=2)


@dc.dataclass(frozen=True)
class Scenario:
    c: np.ndarray
    q: np.ndarray
    p: np.ndarray     # linear momenta
    L: np.ndarray     # angular momenta, body frame
    skin: float
    steps: int
    term: int         # the column of the energy trace that switches on
    cls: str          # the class the pair has to be in by then: "close" or "far"
    centres_stay: bool  # the centres stay within skin / 2 of the build frame until the term acts (the swings)


def _rotated(v, axis, angle):
    axis = axis / np.linalg.norm(axis)
    return v * np.cos(angle) + np.cross(axis, v) * np.sin(angle) + axis * (axis @ v) * (1.0 - np.cos(angle))


X, Y, Z = np.eye(3)
BACK_A1, BACK_A2 = -0.34, 0.3408  # oxDNA2's backbone site in the body frame (a1, a2)


def _translation():
    c = np.array([[0.0, 0.0, 0.0], [2.6, 0.0, 0.0]])
    q = axes_to_quaternion(np.array([X, -X]), np.array([Z, -Z]))
    p = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    return Scenario(c, q, p, np.zeros((2, 3)), 0.6, 220, TERM_HB, "close", False)


def _base_swing(omega=6.0, steps=200):
    c = np.array([[0.0, 0.0, 0.0], [1.35, 0.0, 0.0]])
    a1, a3 = -X, -Z                    # nucleotide 1 when it faces nucleotide 0
    a2 = np.cross(a3, a1)
    u = BACK_A1 * a1 + BACK_A2 * a2    # the axis through its centre and its backbone site (fixed in body and world)
    a1s, a3s = _rotated(a1, u, -np.pi), _rotated(a3, u, -np.pi)
    q = axes_to_quaternion(np.array([X, a1s]), np.array([Z, a3s]))
    ub = np.array([BACK_A1, BACK_A2, 0.0]) / np.hypot(BACK_A1, BACK_A2)
    L = np.array([[0.0, 0.0, 0.0], omega * ub])
    return Scenario(c, q, np.zeros((2, 3)), L, 0.2, steps, TERM_HB, "close", True)


def _backbone_swing(omega=6.0, steps=200):
    c = np.array([[0.0, 0.0, 0.0], [2.5, 0.0, 0.0]])
    q = axes_to_quaternion(np.array([-X, -X]), np.array([Z, -Z]))
    L = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, omega]])
    return Scenario(c, q, np.zeros((2, 3)), L, 0.2, steps, TERM_DEBYE, "far", True)


SCENARIOS = {"translation": _translation(), "base-swing": _base_swing(), "backbone-swing": _backbone_swing()}
