"""`python -m fetalsyngen_amd.resample --bids_path B --out_path O [--res 0.5] [--size 256] [--image_suffix T2w]
[--label_suffix dseg] [--align input|world]`

What the reference's scripts/resample.py does with monai: every `sub-*/ses-*/anat/` (or `sub-*/anat/`) image and
segmentation of a BIDS derivative goes onto the `res` mm isotropic, `size`^3 working grid (`regrid.regrid`: image
trilinear, label nearest, one device pass) and is written to `O/sub/ses/anat/<same file name>`: the image as float32,
the label in its own dtype, the working grid's affine as the sform.  A subject that fails is reported and skipped.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m fetalsyngen_amd.resample", description=__doc__.split("\n\n")[1])
    ap.add_argument("--bids_path", required=True, type=Path)
    ap.add_argument("--out_path", required=True, type=Path)
    ap.add_argument("--res", type=float, default=0.5, help="isotropic voxel size of the working grid in mm")
    ap.add_argument("--size", type=int, default=256, help="edge length of the working grid in voxels")
    ap.add_argument("--image_suffix", default="T2w")
    ap.add_argument("--label_suffix", default="dseg")
    ap.add_argument("--align", choices=("input", "world"), default="input")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.res <= 0 or args.size <= 0:
        ap.error("--res and --size must be positive")
    return args


def find_pairs(bids_path: Path, image_suffix: str, label_suffix: str):
    """[(anat folder relative to bids_path, image file, label file | None)]; raises for an anat folder without one image."""
    out = []
    for sub in sorted(p for p in Path(bids_path).glob("sub-*") if p.is_dir()):
        anats = sorted(sub.glob("ses-*/anat")) + ([sub / "anat"] if (sub / "anat").is_dir() else [])
        for anat in anats:
            out.append((anat.relative_to(bids_path), sorted(anat.glob(f"*_{image_suffix}.nii.gz")),
                        sorted(anat.glob(f"*_{label_suffix}.nii.gz"))))
    return out


def _label_dtype(arr):
    """The array as the resample kernel reads it, and the dtype the result is written in (the file's own)."""
    if arr.dtype in (np.uint8, np.int16, np.float32):
        return arr, arr.dtype
    if arr.dtype == np.int8 or (arr.dtype in (np.uint16, np.int32, np.uint32) and arr.size and -32768 <= arr.min() and arr.max() <= 32767):
        return arr.astype(np.int16), arr.dtype
    return arr.astype(np.float32), arr.dtype  # float64 labels, or integers too wide for 16 bits (exact up to 2^24)


def regrid_arrays(image, label, affine, res, size, align, device):
    """Host arrays in, host arrays out: (image float32 | None, label | None, affine_out).  The one device call of the CLI."""
    import torch

    from . import regrid as R

    img = None if image is None else torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
    lab = None if label is None else torch.from_numpy(np.ascontiguousarray(label)).to(device)
    out, out_lab, affine_out, _M, _box = R.regrid(img, lab, affine, (res,) * 3, (size,) * 3, align)
    return (None if out is None else out.cpu().numpy(), None if out_lab is None else out_lab.cpu().numpy(), affine_out)


def process(anat_rel: Path, images, labels, args, regrid_fn=regrid_arrays):
    from .utils.image_reading import read_nifti, write_nifti

    if len(images) != 1:
        raise RuntimeError(f"{len(images)} files match *_{args.image_suffix}.nii.gz in {anat_rel}")
    if len(labels) > 1:
        raise RuntimeError(f"{len(labels)} files match *_{args.label_suffix}.nii.gz in {anat_rel}")
    image, affine, _ = read_nifti(images[0])
    label = out_dtype = None
    if labels:
        raw, _label_affine, _ = read_nifti(labels[0])
        if raw.shape != image.shape:
            raise RuntimeError(f"image {image.shape} and label {raw.shape} differ in shape")
        label, out_dtype = _label_dtype(raw)
    out, out_lab, affine_out = regrid_fn(image, label, affine, args.res, args.size, args.align, args.device)
    dest = args.out_path / anat_rel
    dest.mkdir(parents=True, exist_ok=True)
    written = [dest / images[0].name]
    write_nifti(written[0], np.asarray(out, dtype=np.float32), affine_out)
    if labels:
        written.append(dest / labels[0].name)
        write_nifti(written[1], np.asarray(out_lab).astype(out_dtype), affine_out)
    return written


def main(argv=None, regrid_fn=regrid_arrays) -> int:
    args = parse_args(argv)
    pairs = find_pairs(args.bids_path, args.image_suffix, args.label_suffix)
    print(f"Found {len(pairs)} anat folders in {args.bids_path}")
    failed = 0
    for anat_rel, images, labels in pairs:
        try:
            for path in process(anat_rel, images, labels, args, regrid_fn):
                print(f"wrote {path}")
        except Exception as e:  # as the reference: report, go on with the next subject
            failed += 1
            print(f"Error processing {anat_rel} due to {e}")
    return 1 if failed and failed == len(pairs) else 0


if __name__ == "__main__":
    raise SystemExit(main())
