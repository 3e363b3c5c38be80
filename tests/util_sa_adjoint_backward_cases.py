"""Inputs of tests/test_sa_adjoint_backward_gpu.py, built on the host with numpy from tests/util_sa_backward_cases.py (so the
CPU can examine the same cases): the roles change, the arrays do not.  Its `vol` plays grad_vol and its `g` plays the slices.

equalize    `vol` and `vol_weight` of the backward come from the float64 restatement of the adjoint forward
            (util_sa_adjoint_backward64.adjoint64) rounded to fp32, so the forward kernel's atomics do not enter a comparison.
            exact cases: every positive vol_weight is replaced by the nearest power of two, so the division of the gradient
            is exact in fp32, and every 17th reached voxel gets 2^-11, below the 1e-3 floor of the rule.
"""
import numpy as np

from tests import util_sa_backward_cases as CS
from tests.util_sa_adjoint_backward64 import adjoint64, adjoint_backward64

VS, N, EXACT, GENERAL = CS.VS, CS.N, CS.EXACT, CS.GENERAL


def _roles(c):
    return dict(tr=c["tr"], gvol=c["vol"], vm=c["vm"], psf=c["psf"], sl=c["g"], sm=c["sm"], res=c["res"], vol=None, vw=None)


def _with_forward(case, interp_psf, pow2):
    f = adjoint64(case["tr"], case["psf"], case["sl"], case["sm"], case["vm"], VS, case["res"], interp_psf, True)
    vw = f["vol_weight"].astype(np.float32)
    if pow2:
        pos = vw > 0
        vw[pos] = np.exp2(np.round(np.log2(vw[pos].astype(np.float64)))).astype(np.float32)
        idx = np.flatnonzero(pos.reshape(-1))[::17]
        vw.reshape(-1)[idx] = np.float32(2.0 ** -11)
    return dict(case, vol=f["vol"].astype(np.float32), vw=vw)


def exact_case(name, masks, interp_psf=False, equalize=False, **kw):
    case = _roles(CS.exact_case(name, masks, **kw))
    return _with_forward(case, interp_psf, True) if equalize else case


def general_case(name, interp_psf, equalize=False):
    case = _roles(CS.general_case(name, interp_psf))
    # the mask of CS.general_case comes from the backward of the forward: the same taps and the same four decision kinds
    return _with_forward(case, interp_psf, False) if equalize else case


def reference(case, interp_psf, fn=adjoint_backward64):
    eq = case["vol"] is not None
    return fn(case["tr"], case["gvol"], case["psf"], case["sl"], case["sm"], case["vm"], case["res"], interp_psf, equalize=eq,
              vol=case["vol"], vol_weight=case["vw"])
