"""Operator surface of the map-making hot path, with the reference's class names
(``toast.ops.*``): drop-in for that path."""

from .arithmetic import Combine
from .mapmaker import ApplyAmplitudes, MapMaker, SolveAmplitudes
from .mapmaker_ops import (
    BinMap,
    BuildHitMap,
    BuildInverseCovariance,
    BuildNoiseWeighted,
    Copy,
    CovarianceAndHits,
    Delete,
    NoiseWeight,
    ScanMap,
    ScanMask,
)
from .mapmaker_solve import SolverLHS, SolverRHS, TemplateMatrix, solve
from .demodulation import Demodulate, StokesWeightsDemod
from .filterbin import FilterBin
from .ground_filter import GroundFilter
from .hwpss_model import HWPSynchronousModel
from .noise_estimation import NoiseEstim
from .noise_filter import NoiseFilter
from .operator import Operator
from .pipeline import Pipeline
from .poly_filter import CommonModeFilter, PolyFilter, PolyFilter2D
from .pointing import BuildPixelDistribution, PixelsHealpix, PointingDetectorSimple, StokesWeights
from .sim_ground import SimGround
from .sim_tod_atm_observe import ObserveAtmosphere
from .sim_tod_dipole import SimDipole
from .sim_tod_noise import SimNoise
from .time_constant import TimeConstant
