"""Helical diameter (mythos/observables/diameter.py:16-91): per frame, the mean over the hydrogen-bonded base pairs of
the distance between their backbone sites plus the excluded-volume distance ``sigma_backbone``, in Angstrom.  The
distances come from the HIP library (csrc/duplex_obs.hip); ``sigma_backbone`` is added here, so it may be a tensor that
requires a gradient, as the reference's objective differentiates it."""

from __future__ import annotations

import numpy as np
import torch

from mythos_amd.observables import base as B

TARGETS = {
    "oxDNA": 23.0,  # Angstroms. Experimental value for helical radius is 11.5-12 A
}

ERR_DISPLACEMENT_FN_REQUIRED = "A displacement function is required for computing the helical diameter."


class Diameter(B.DuplexObservable):
    def __init__(self, h_bonded_base_pairs, displacement_fn, geometry: dict, model: int = 2):
        if displacement_fn is None:
            raise ValueError(ERR_DISPLACEMENT_FN_REQUIRED)
        self.h_bonded_base_pairs = np.asarray(h_bonded_base_pairs, dtype=np.int64).reshape(-1, 2)
        self.base_pairs = self.h_bonded_base_pairs
        self.displacement_fn, self.geometry, self.model = displacement_fn, geometry, model

    def __call__(self, trajectory, sigma_backbone) -> torch.Tensor:
        """(n_states,) mean helical diameter in Angstrom."""
        return (self.rows(trajectory)[:, B.COL_BACKBONE_DISTANCE] + sigma_backbone) * B.ANGSTROMS_PER_OXDNA_LENGTH
