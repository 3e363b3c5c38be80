"""Mirror of `fetalsyngen.generator.artifacts.svort` (reference svort/__init__.py:1-10)."""
from .autograd import axisangle2mat_autograd  # noqa: F401
from .rigid import (RigidTransform, ax_update_resolution, axisangle2mat, init_stack_transform, init_zero_transform,  # noqa: F401
                    mat2axisangle, mat_transform_points, mat_update_resolution, random_angle,
                    random_init_stack_transforms, reset_transform, transform_points)
from .scan import (get_PSF, get_trajectory, interleave_index, random_stack, resolution2sigma, sample_motion,  # noqa: F401
                   set_trajectory_bank, synthetic_trajectory_bank)
from .slice_acq import get_semantics, set_semantics, slice_acquisition, slice_acquisition_adjoint  # noqa: F401
from .outlier import robust_weights  # noqa: F401
from .intensity import intensity_match  # noqa: F401
from .srr import SRR, srr  # noqa: F401
from .svr import SVR, svr  # noqa: F401
from .align import align_stacks  # noqa: F401
# the device-resident, differentiable conversions live in their module: `axisangle2mat`, `mat2axisangle` and `RigidTransform`
# of this namespace stay rigid.py's detaching host versions, which the generator relies on
from . import transform_convert  # noqa: F401,E402
from .transform_convert import DeviceRigidTransform  # noqa: F401,E402
