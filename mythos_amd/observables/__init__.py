"""Per-frame observables used by DiffTRe objectives (a small part of mythos/observables/: SURVEY.md 8f-3), evaluated
by the HIP library - stand-alone, or in the same call as the energy launch (``energy_fn.with_observables``) - and the
MARTINI bond-length / triplet-angle distributions with their weighted Wasserstein distance to reference distributions, and
the membrane observables of a bilayer: thickness, area per lipid and the melting temperature fitted to it, and the
duplex-mechanics set: helical diameter, extension, twist, RMSE to a target, the stretch / torsion moduli and the
worm-like-chain fit, and the duplex melting temperature by histogram reweighting of an umbrella-sampled trajectory, with
oxDNA's ``bond`` / ``mindistance`` order parameters of stored frames and the umbrella histogram and weights built on them,
and the radial distribution functions between selections of MARTINI beads, and MBAR over umbrella windows with the
free-energy profile along a pull coordinate, and the lateral pressure profile and surface tension of stored MARTINI frames."""

from mythos_amd.observables.base import ObservableSet, get_duplex_quartets
from mythos_amd.observables.bond_distances import BondDistances, BondDistancesMapped
from mythos_amd.observables.diameter import Diameter
from mythos_amd.observables.mbar import (BlockResample, MbarNotConverged, MbarResult, UmbrellaPMF, auto_block, block_resample, mbar, mbar_umbrella,
                                         statistical_inefficiency, subsample_correlated)
from mythos_amd.observables.melting_temp import (TARGETS, MeltingTemp, compute_curve_width, compute_finf, extrapolated_ratios,
                                                 find_melting_temp, interp1d)
from mythos_amd.observables.membrane import AreaPerLipid, MembraneThickness
from mythos_amd.observables.membrane_melting_temp import (MembraneMeltingTemp, apl_residual, calculate_apl, compute_membrane_tm,
                                                          fit_apl_sigmoid, get_initial_guess)
from mythos_amd.observables.order_parameters import (OrderParameters, extrapolated_histogram, reweight_from_histogram,
                                                     umbrella_histogram)
from mythos_amd.observables.persistence_length import PersistenceLength, persistence_length_fit
from mythos_amd.observables.pitch import PitchAngle, compute_pitch
from mythos_amd.observables.propeller import PropellerTwist
from mythos_amd.observables.rdf import RadialDistribution, RadialDistributionPair
from mythos_amd.observables.rise import Rise
from mythos_amd.observables.rmse import RMSE
from mythos_amd.observables.stress_profile import StressProfile, SurfaceTension
from mythos_amd.observables.stretch_torsion import ExtensionZ, TwistXY, stretch, stretch_torsion, torsion
from mythos_amd.observables.triplet_angles import TripletAngles, TripletAnglesMapped
from mythos_amd.observables.wasserstein import WassersteinDistance, WassersteinDistanceMapped, wasserstein_1d
from mythos_amd.observables.wlc import calculate_extension, coth, fit_wlc, loss

__all__ = ["BlockResample", "MbarNotConverged", "MbarResult", "UmbrellaPMF", "auto_block", "block_resample", "mbar", "mbar_umbrella",
           "statistical_inefficiency", "subsample_correlated", "AreaPerLipid", "BondDistances", "BondDistancesMapped", "Diameter", "ExtensionZ", "MeltingTemp", "MembraneMeltingTemp", "MembraneThickness",
           "ObservableSet", "OrderParameters", "StressProfile", "SurfaceTension", "PersistenceLength", "PitchAngle", "PropellerTwist", "RMSE", "RadialDistribution", "RadialDistributionPair", "Rise", "TripletAngles", "TripletAnglesMapped",
           "TwistXY", "WassersteinDistance", "WassersteinDistanceMapped", "apl_residual", "calculate_apl", "calculate_extension",
           "compute_membrane_tm", "compute_pitch", "coth", "fit_apl_sigmoid", "fit_wlc", "get_duplex_quartets", "get_initial_guess",
           "loss", "persistence_length_fit", "stretch", "stretch_torsion", "torsion", "wasserstein_1d", "TARGETS", "compute_curve_width",
           "compute_finf", "extrapolated_ratios", "find_melting_temp", "interp1d", "extrapolated_histogram", "reweight_from_histogram", "umbrella_histogram"]
