"""Per-frame observables used by DiffTRe objectives (a small part of mythos/observables/: SURVEY.md 8f-3), evaluated
by the HIP library - stand-alone, or in the same call as the energy launch (``energy_fn.with_observables``) - and the
MARTINI bond-length / triplet-angle distributions with their weighted Wasserstein distance to reference distributions."""

from mythos_amd.observables.base import ObservableSet, get_duplex_quartets
from mythos_amd.observables.bond_distances import BondDistances, BondDistancesMapped
from mythos_amd.observables.persistence_length import PersistenceLength, persistence_length_fit
from mythos_amd.observables.pitch import PitchAngle, compute_pitch
from mythos_amd.observables.propeller import PropellerTwist
from mythos_amd.observables.rise import Rise
from mythos_amd.observables.triplet_angles import TripletAngles, TripletAnglesMapped
from mythos_amd.observables.wasserstein import WassersteinDistance, WassersteinDistanceMapped, wasserstein_1d

__all__ = ["BondDistances", "BondDistancesMapped", "ObservableSet", "PersistenceLength", "PitchAngle", "PropellerTwist", "Rise",
           "TripletAngles", "TripletAnglesMapped", "WassersteinDistance", "WassersteinDistanceMapped", "compute_pitch",
           "get_duplex_quartets", "persistence_length_fit", "wasserstein_1d"]
