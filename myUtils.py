"""Drop-in alias of the reference's `myUtils` (imported as `utils` by its entry scripts)."""
from fal_net_amd.myUtils import *  # noqa: F401,F403
from fal_net_amd.myUtils import (compute_make_errors, disps_to_depths_make, kitti_error_names, make_error_names,  # noqa: F401
                                 width_to_baseline, width_to_focal)
