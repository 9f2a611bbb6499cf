"""sitrack_amd -- MI355X-native per-buoy advection for the `sitrack` sea-ice tracker.

Import as `import sitrack_amd as sit`: the hot-path functions keep the reference's
names (`sit.SeedInit`, `sit.CartNPSkm2Geo1D`, `sit.GetTimeSpan`, ...).
"""
from ._lib import Context, SitrkError, FillValue, build, lib, SO_PATH      # noqa: F401
from .tracking import (SeedInit, FindContainingCell, CartNPSkm2Geo1D, Geo2CartNPSkm1D, GetTimeSpan,  # noqa: F401
                       ConvertGeo2CartesianNPSkm, ConvertCartesianNPSkm2Geo,
                       IceTracker, vertices_of, default_context, rmin_conc, rFoundKM)
from .predicates import (_ccw_, intersect2Seg, IsInsideQuadrangle, CrossedEdge, NewHostCell, UpdtInd4NewCell,  # noqa: F401
                         Survive, Haversine, NearestPoint)
from .ncio import (GetModelGrid, GetModelUVGrid, LoadNCtime, LoadNCdata, SeedFileTimeInfo, ModelFileTimeInfo,  # noqa: F401
                   ncSaveCloudBuoys, chck4f)
from .seeding import SubSampCloud                                            # noqa: F401
from .overlap import CancelTooClose                                          # noqa: F401
from .deformation import DeformCells, lattice_cells                          # noqa: F401
from .quadmesh import Tri2Quad                                                # noqa: F401
from .delaunay import DelaunayTris                                           # noqa: F401
from .raster import RasterCells, raster_grid                                  # noqa: F401
from .coarse import CoarseCells, scaling_exponents                            # noqa: F401
from .dispersion import PairDispersion, dispersion_curve, dispersion_exponents, pair_edges, pairs_arg   # noqa: F401
from .distribution import (ValueDistribution, log_edges, lin_edges, pdf_from_counts, tail_exponent,   # noqa: F401
                           percentile_threshold, pdf_arg)
from .features import SkeletonRaster, node_yx, skeleton_table                                                            # noqa: F401
from .features import LabelRaster, MatchLabels, feature_table, feature_tracks, link_features                              # noqa: F401
from ._lib import FEAT_COLS, FEAT_WHAT                                        # noqa: F401
from .coast import DistToCoast, MaskCoastal                                  # noqa: F401
from . import synthetic                                                      # noqa: F401
