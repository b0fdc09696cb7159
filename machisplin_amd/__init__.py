"""machisplin_amd -- MI355X (gfx950) backend for MACHISPLIN's data-parallel hot path.

The package holds only what the path needs: ``csrc/`` (hand-written HIP kernels and the
C ABI of include/machisplin_hip.h, built into ``libmachisplin_hip.so``) and the host-side
mirror of the reference's interface for the path (``Tps``/``interpolate``/``predict`` as
``machisplin.mltps`` calls them, V73:442-930).  Importing the package needs neither a GPU
nor the built library; every compute entry point does, and raises without them.
"""
from . import _lib
from ._lib import MhsError, init
from .raster import Geometry, RasterStack
from . import models
from .models import predict, ensemble_predict, nnet_fit_many, ksvm_fit_many, sigest
from . import tps
from .tps import Tps, fit_many, interpolate, interpolate_se, eval_mode, EVAL_AUTO, EVAL_DIRECT, EVAL_FAR_FIELD
from .tps import se_max_n, se_build_mode, SE_BUILD_AUTO, SE_BUILD_HOST, SE_BUILD_DEVICE
from . import tiles, mltps, cv, varimp, mess, terrain
from . import resample
from .resample import extract, align      # resample.resample: the module keeps its name, as terrain does
from . import proximity                   # proximity.proximity: the module keeps its name, as resample does
from . import flowpath                    # flowpath.flowpath: likewise
from . import project                     # project.project, project.warp: rasters into another coordinate system
from . import focal                       # focal.focal: window statistics at any radius
from . import patches                     # patches.patches, patches.sieve: connected patches of a mask and the size filter
from . import zonal                       # zonal.zonal: a layer's statistics per zone of an integer zone plane
from . import classes                     # classes.crosstab, classes.aggregate, classes.focal: categorical layers per zone, cell, window
from . import vector                      # vector.Features, vector.read_geojson: points, lines and polygons as flat arrays
from . import rasterize                   # rasterize.rasterize: vector features burned onto the grid
from .mess import Mess
from .terrain import relief, geomorphon, hydro, hydro_mfd, covariates, solar, sun_tables, SunTables      # the 3 x 3 variables: terrain.terrain (the module keeps its name)
from .cv import fit_layer, fit_nnet_folds, fit_ksvm_folds, kfold
from .mltps import mltps as mltps_layers, mltps_predict, tps_residual_surface, tps_residual_surface_se

__all__ = ["MhsError", "init", "Geometry", "RasterStack", "Tps", "interpolate", "interpolate_se", "eval_mode", "EVAL_AUTO", "EVAL_DIRECT", "EVAL_FAR_FIELD",
           "se_max_n", "se_build_mode", "SE_BUILD_AUTO", "SE_BUILD_HOST", "SE_BUILD_DEVICE", "predict",
           "ensemble_predict", "models", "tiles", "mltps", "mltps_predict",
           "tps_residual_surface", "tps_residual_surface_se", "nnet_fit_many", "ksvm_fit_many", "sigest", "fit_layer",
           "fit_nnet_folds", "fit_ksvm_folds", "kfold", "varimp", "mess", "Mess", "terrain", "relief", "geomorphon", "hydro", "hydro_mfd", "covariates", "solar", "sun_tables",
           "SunTables", "resample", "extract", "align", "proximity", "flowpath", "project", "focal", "patches", "zonal", "classes", "vector", "rasterize", "_lib"]
