"""Per-frame observables used by DiffTRe objectives (a small part of mythos/observables/: SURVEY.md 8f-3), evaluated
by the HIP library - stand-alone, or in the same call as the energy launch (``energy_fn.with_observables``) - and the
MARTINI bond-length / triplet-angle distributions with their weighted Wasserstein distance to reference distributions, and
the membrane observables of a bilayer: thickness, area per lipid and the melting temperature fitted to it."""

from mythos_amd.observables.base import ObservableSet, get_duplex_quartets
from mythos_amd.observables.bond_distances import BondDistances, BondDistancesMapped
from mythos_amd.observables.membrane import AreaPerLipid, MembraneThickness
from mythos_amd.observables.membrane_melting_temp import (MembraneMeltingTemp, apl_residual, calculate_apl, compute_membrane_tm,
                                                          fit_apl_sigmoid, get_initial_guess)
from mythos_amd.observables.persistence_length import PersistenceLength, persistence_length_fit
from mythos_amd.observables.pitch import PitchAngle, compute_pitch
from mythos_amd.observables.propeller import PropellerTwist
from mythos_amd.observables.rise import Rise
from mythos_amd.observables.triplet_angles import TripletAngles, TripletAnglesMapped
from mythos_amd.observables.wasserstein import WassersteinDistance, WassersteinDistanceMapped, wasserstein_1d

__all__ = ["AreaPerLipid", "BondDistances", "BondDistancesMapped", "MembraneMeltingTemp", "MembraneThickness", "ObservableSet",
           "PersistenceLength", "PitchAngle", "PropellerTwist", "Rise", "TripletAngles", "TripletAnglesMapped",
           "WassersteinDistance", "WassersteinDistanceMapped", "apl_residual", "calculate_apl", "compute_membrane_tm",
           "compute_pitch", "fit_apl_sigmoid", "get_duplex_quartets", "get_initial_guess", "persistence_length_fit",
           "wasserstein_1d"]
