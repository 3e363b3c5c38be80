"""Regridding of real volumes: the geometry on the host (float64 numpy), the resampling on the device.

The reference brings a raw BIDS derivative onto its 0.5 mm, 256^3 working grid offline with monai (scripts/resample.py:
Spacingd, Orientationd("RAS"), CenterSpatialCropd, SpatialPadd) and applies the same kind of chain, plus a foreground
crop, to validation data (configs/dataset/transforms/inference.yaml).  Every step of such a chain maps voxel grids
affinely, so here the chain is composed on the host into ONE 3x4 map `M` from output voxel index to source voxel
coordinate plus the source index box that counts as inside, and `kernels.affine_resample` (csrc/fsg_regrid.hip) makes one
pass over the output: image trilinear, label by nearest voxel.  The same operator with the inverse map takes a
prediction back to the native grid.

Centring rule: output voxel coordinate (size - 1) / 2 is the world position of the centre (lo + hi) / 2 of the source box
(the whole volume, or the foreground box).  monai is absent, so parity with its output is unpinned: its output-shape
rounding after `Spacing` and the parity of its pad / crop on odd sizes can shift the result by up to about one output
voxel against this rule.
"""
from __future__ import annotations

import numpy as np

from .utils.image_reading import io_orientation


def _box6(box, shape):
    if box is None:
        return np.array([0, shape[0] - 1, 0, shape[1] - 1, 0, shape[2] - 1], dtype=np.int32)
    box = np.asarray(box, dtype=np.int64).reshape(6)
    for a in range(3):
        if not 0 <= box[2 * a] <= box[2 * a + 1] < shape[a]:
            raise ValueError(f"box {box.tolist()} is empty or leaves the volume of shape {tuple(shape)}")
    return box.astype(np.int32)


def map_between(affine_src, affine_dst) -> np.ndarray:
    """3x4 map from voxel indices of the grid `affine_dst` to voxel coordinates of the grid `affine_src`."""
    full = np.linalg.inv(np.asarray(affine_src, dtype=np.float64)) @ np.asarray(affine_dst, dtype=np.float64)
    return np.ascontiguousarray(full[:3, :])


def working_grid(shape, affine, pixdim=(0.5, 0.5, 0.5), size=(256, 256, 256), align="input", box=None):
    """-> (affine_out 4x4, M 3x4, box int32[6]) of the working grid for a volume of `shape` with voxel->world `affine`.

    align="input" (the reference's behaviour): monai's `Spacing` rescales the columns of the affine and keeps their
    directions, `Orientation("RAS")` permutes and flips them to the closest canonical order -- the output axes are the
    input's own normalised axes, reordered and flipped by `io_orientation`, scaled to `pixdim` (R, A, S order).  An
    oblique volume stays oblique in world space and is sampled along its own axes.
    align="world": the output axes are the world axes, affine_out[:3,:3] = diag(pixdim): de-obliques the volume.
    `box`: inclusive source index box lo0,hi0,lo1,hi1,lo2,hi2 (None: the whole volume); its centre goes to the centre
    (size - 1) / 2 of the output grid."""
    affine = np.asarray(affine, dtype=np.float64)
    if affine.shape != (4, 4):
        raise ValueError("affine must be 4x4")
    pixdim = np.asarray(pixdim, dtype=np.float64).reshape(3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    if (pixdim <= 0).any() or (size <= 0).any():
        raise ValueError("pixdim and size must be positive")
    box = _box6(box, shape)
    out = np.eye(4)
    if align == "input":
        rzs = affine[:3, :3]
        zooms = np.sqrt((rzs * rzs).sum(axis=0))
        if (zooms == 0).any():
            raise ValueError("degenerate affine: a voxel axis has no direction")
        ornt = io_orientation(affine)
        for in_ax in range(3):
            o = int(ornt[in_ax, 0])
            out[:3, o] = ornt[in_ax, 1] * rzs[:, in_ax] / zooms[in_ax] * pixdim[o]
    elif align == "world":
        out[:3, :3] = np.diag(pixdim)
    else:
        raise ValueError("align must be 'input' or 'world'")
    centre_src = np.array([(box[0] + box[1]) / 2.0, (box[2] + box[3]) / 2.0, (box[4] + box[5]) / 2.0, 1.0])
    world = affine @ centre_src
    out[:3, 3] = world[:3] - out[:3, :3] @ ((size - 1) / 2.0)
    return out, map_between(affine, out), box


def inverse_map(native_shape, native_affine, affine_out, size):
    """-> (M 3x4, box int32[6]) that take the working grid (`affine_out`, `size`) back onto the native grid: M maps a native
    voxel index to a working-grid coordinate, the box is the whole working grid."""
    del native_shape  # the native grid's extent is the output shape of the resample, not part of the map
    size = np.asarray(size, dtype=np.int64).reshape(3)
    return map_between(affine_out, native_affine), _box6(None, size)


# ---- device entry points ------------------------------------------------------------------------------------------------
def foreground_box(image, threshold: float = 0.0):
    """Inclusive index box of `image > threshold` (device tensor, 3-D float32) as six ints, or None when no voxel is.
    What monai's CropForeground (select_fn = x > 0, margin 0) crops to.  Reads six words back: synchronises."""
    from . import kernels as K

    box = K.bbox_gt(image, threshold).cpu().numpy()
    if box[1] < box[0]:
        return None
    return [int(v) for v in box]


def resample(image, label, M, box, out_shape, fill=0.0, fill_label=0, nan_is_zero=True):
    """One pass of `fsg_affine_resample`: -> (image float32 | None, label in its own dtype | None) of `out_shape`."""
    from . import kernels as K

    return K.affine_resample(image, label, M, box, out_shape, fill=fill, fill_label=fill_label, nan_is_zero=nan_is_zero)


def regrid(image, label, affine, pixdim=(0.5, 0.5, 0.5), size=(256, 256, 256), align="input", crop_foreground=False):
    """Volume(s) with voxel->world `affine` onto the working grid: -> (image, label, affine_out, M, box).  `crop_foreground`:
    the inside box is the box of `image > 0` (the whole volume when nothing is); everything outside it reads as 0."""
    ref = image if image is not None else label
    shape = tuple(int(n) for n in ref.shape)
    box = foreground_box(image) if (crop_foreground and image is not None) else None
    affine_out, M, box = working_grid(shape, affine, pixdim, size, align, box)
    out_img, out_lab = resample(image, label, M, box, tuple(int(s) for s in np.asarray(size).reshape(3)))
    return out_img, out_lab, affine_out, M, box
