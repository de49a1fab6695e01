"""jackal_navigation_amd — MI355X (gfx950) implementation of jackal_nav's `point_cloud` hot path.

Rectified stereo pair -> ELAS disparity -> u8 depth map -> Q reprojection -> ground-plane filter ->
90-bin obstacle scan, as hand-written HIP kernels behind a C ABI (include/jn_stereo.h,
libjn_stereo.so).  This package is the thin host-side mirror of the reference interfaces; all
compute lives in csrc/.  Importing the compute API requires the built library; there is no CPU path.
"""
from ._lib import load, hooks_library, JnError, ElasParams, ScanParams, EXPORTS, LIB_PATH, HOOKS_LIB_PATH  # noqa: F401
from .elas import Elas  # noqa: F401
from . import node, device, parallel, navigate  # noqa: F401
from .sgm import Sgm, SgmCostParams, SGM_EXPORTS, SGM_COST_EXPORTS  # noqa: F401
from .bm import Bm, BM_EXPORTS  # noqa: F401
from . import costmap  # noqa: F401
from .costmap import CostmapParams, COSTMAP_EXPORTS  # noqa: F401
from . import subpix  # noqa: F401
from .subpix import SubpixParams, SUBPIX_EXPORTS, subpix_scan, subpix_costmap, subpix_point_cloud  # noqa: F401
from . import localmap  # noqa: F401
from .localmap import LocalMap, LocalMapParams, Pose2D, LOCALMAP_EXPORTS, localmap_params  # noqa: F401
from . import plan  # noqa: F401
from .plan import Plan, PlanParams, PlanRecord, PlanCmd, PLAN_EXPORTS, plan_params  # noqa: F401
from . import route  # noqa: F401
from .route import Route, RouteParams, RouteStats, ROUTE_EXPORTS, route_params  # noqa: F401
from . import postfilter  # noqa: F401
from .postfilter import PostfilterParams, POSTFILTER_EXPORTS, postfilter_params, disparity_postfilter  # noqa: F401
from . import ground, calib  # noqa: F401
from .ground import GroundParams, GroundPlane, GROUND_EXPORTS  # noqa: F401
from .calib import load_calibration, save_calibration, CALIB_EXPORTS  # noqa: F401
