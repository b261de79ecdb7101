# coding=utf-8
"""
deconv3d_amd -- MI355X-native likelihood path of irap-omp/deconv3d behind the
reference's own ``Run / Instrument / SpreadFunction / LineModel`` API
(reference facade: __init__.py:10-14).
"""
from .cube import Axis, Cube, HyperspectralCube  # noqa: F401
from .instruments import MUSE, Instrument  # noqa: F401
from .line_models import (GaussianMultipletLineModel, LineModel, SingleGaussianLineModel,  # noqa: F401
                          TabulatedLineModel)
from .masks import above_percentile, above_snr  # noqa: F401
from .math_utils import median_clip  # noqa: F401
from . import adapt  # noqa: F401
from . import posterior  # noqa: F401
from .posterior import PosteriorHistograms, PosteriorMoments  # noqa: F401
from . import predictive  # noqa: F401
from .predictive import PredictiveAccuracy  # noqa: F401
from . import noise  # noqa: F401
from .noise import NoiseReport  # noqa: F401
from . import prepare  # noqa: F401
from .prepare import Prepared, prepare_cube  # noqa: F401
from . import regions  # noqa: F401
from .regions import RegionPosterior  # noqa: F401
from .run import Run, logger  # noqa: F401
from . import search  # noqa: F401
from .search import LineSearch, line_search  # noqa: F401
from .spread_functions import (  # noqa: F401
    FieldSpreadFunction, GaussianFieldSpreadFunction, GaussianLineSpreadFunction,
    ImageFieldSpreadFunction, LineSpreadFunction, MoffatFieldSpreadFunction,
    MUSELineSpreadFunction, NoFieldSpreadFunction, VectorLineSpreadFunction)

__version__ = "0.1.0"
