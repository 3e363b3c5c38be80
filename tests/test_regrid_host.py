"""CPU: the host geometry of fetalsyngen_amd/regrid.py, FetalTestDataset without transforms, the resample CLI with the
device call stubbed out, and the argument checks of the two regrid entry points (no launch happens)."""
import ctypes

import numpy as np
import pytest
import torch

from fetalsyngen_amd import _lib, regrid
from fetalsyngen_amd.utils.image_reading import io_orientation, ras_reorient, ras_reorient_affine, read_nifti, write_nifti
from tests import util_regrid64 as R64

SHAPE = (12, 9, 21)


def full(M):
    return np.vstack([M, [0, 0, 0, 1]])


def test_diagonal_ras_affine_is_scale_and_shift():
    affine = np.diag([1.0, 1.0, 1.0, 1.0])
    affine[:3, 3] = [-7.0, 3.0, 11.0]
    out, M, box = regrid.working_grid((19, 23, 17), affine, (0.5, 0.5, 0.5), (38, 46, 34))
    assert box.tolist() == [0, 18, 0, 22, 0, 16] and box.dtype == np.int32
    assert np.array_equal(M[:, :3], np.diag([0.5, 0.5, 0.5]))
    assert np.allclose(M[:, 3], [-0.25, -0.25, -0.25], atol=1e-12)  # (n-1)/2 - 0.5 (2n-1)/2
    assert np.allclose(out[:3, :3], np.diag([0.5, 0.5, 0.5])) and np.allclose(out[:3, 3], affine[:3, 3] - 0.25)


def _affines():
    lps = np.diag([-0.8, -0.8, 0.8, 1.0])
    lps[:3, 3] = [40.0, 35.0, -12.0]
    perm = np.zeros((4, 4))
    perm[0, 2], perm[1, 0], perm[2, 1], perm[3, 3] = 0.9, -1.1, 1.0, 1.0  # voxel axes run A-, S+, R+
    perm[:3, 3] = [5.0, -6.0, 7.0]
    return {"lps": lps, "perm": perm}


@pytest.mark.parametrize("name", ["lps", "perm"])
def test_flipped_and_permuted_inputs_land_on_the_ras_array(name):
    affine = _affines()[name]
    rng = np.random.default_rng(4)
    arr = rng.random(SHAPE)
    lab = rng.integers(0, 7, SHAPE).astype(np.uint8)
    size = (20, 24, 18)
    _o, M, box = regrid.working_grid(SHAPE, affine, (0.5, 0.5, 0.5), size)
    direct, direct_lab, _p, _ok = R64.resample(arr, lab, M, box, size)
    ras, ras_lab = ras_reorient(arr, affine), ras_reorient(lab, affine)
    ras_affine = ras_reorient_affine(affine, SHAPE)
    assert np.array_equal(io_orientation(ras_affine), [[0, 1], [1, 1], [2, 1]])
    _o2, M2, box2 = regrid.working_grid(ras.shape, ras_affine, (0.5, 0.5, 0.5), size)
    assert np.allclose(M2[:, :3], np.diag(np.diag(M2[:, :3]))) and (np.diag(M2[:, :3]) > 0).all()  # axis aligned
    two_step, two_step_lab, _p, _ok = R64.resample(ras, ras_lab, M2, box2, size)
    assert np.allclose(direct, two_step, atol=1e-12) and np.array_equal(direct_lab, two_step_lab)
    assert np.allclose(_o, _o2, atol=1e-12)


def test_oblique_affine_keeps_or_loses_its_obliquity():
    A = R64.rotation(12, 5, -8) @ np.diag([0.8, 0.8, 1.2])
    affine = np.eye(4)
    affine[:3, :3], affine[:3, 3] = A, [-30.0, -20.0, 10.0]
    out_in, M_in, _b = regrid.working_grid(SHAPE, affine, (0.5, 0.5, 0.5), (32, 32, 32), align="input")
    out_w, M_w, _b = regrid.working_grid(SHAPE, affine, (0.5, 0.5, 0.5), (32, 32, 32), align="world")
    assert np.allclose(out_in[:3, :3], R64.rotation(12, 5, -8) * 0.5, atol=1e-12)   # the input's own directions
    assert np.allclose(M_in[:, :3], np.diag([0.5 / 0.8, 0.5 / 0.8, 0.5 / 1.2]), atol=1e-12)  # sampled along its own axes
    assert np.array_equal(out_w[:3, :3], np.diag([0.5, 0.5, 0.5]))
    off = M_w[:, :3] - np.diag(np.diag(M_w[:, :3]))
    assert np.abs(off).max() > 0.05  # the native grid is oblique to the world grid: M carries the rotation
    with pytest.raises(ValueError):
        regrid.working_grid(SHAPE, affine, align="diagonal")


@pytest.mark.parametrize("align", ["input", "world"])
@pytest.mark.parametrize("box", [None, [2, 8, 1, 5, 4, 19]])
def test_centre_maps_to_the_box_centre_and_inverse_is_the_identity(align, box):
    affines = dict(_affines())
    obl = np.eye(4)
    obl[:3, :3], obl[:3, 3] = R64.rotation(20, -11, 7) @ np.diag([1.0, 0.7, 0.9]), [3.0, 4.0, 5.0]
    affines["oblique"] = obl
    for affine in affines.values():
        size = (31, 40, 26)
        out, M, b = regrid.working_grid(SHAPE, affine, (0.5, 0.6, 0.7), size, align=align, box=box)
        want = [(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2]
        centre = np.array([(s - 1) / 2 for s in size] + [1.0])
        assert np.allclose(M @ centre, want, atol=1e-10)
        assert np.allclose(np.sqrt((out[:3, :3] ** 2).sum(0)), (0.5, 0.6, 0.7), atol=1e-12)
        Minv, binv = regrid.inverse_map(SHAPE, affine, out, size)
        assert binv.tolist() == [0, 30, 0, 39, 0, 25]
        assert np.allclose(full(M) @ full(Minv), np.eye(4), atol=1e-12)
        assert np.allclose(full(Minv) @ full(M), np.eye(4), atol=1e-12)


def test_bad_boxes_and_sizes_raise():
    with pytest.raises(ValueError):
        regrid.working_grid(SHAPE, np.eye(4), box=[3, 2, 0, 8, 0, 20])
    with pytest.raises(ValueError):
        regrid.working_grid(SHAPE, np.eye(4), box=[0, 12, 0, 8, 0, 20])
    with pytest.raises(ValueError):
        regrid.working_grid(SHAPE, np.eye(4), pixdim=(0.5, 0.0, 0.5))


def test_device_entry_points_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regrid.resample(torch.zeros(4, 4, 4), None, np.eye(4)[:3], [0, 3, 0, 3, 0, 3], (4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regrid.foreground_box(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regrid.regrid(None, torch.zeros(4, 4, 4, dtype=torch.uint8), np.eye(4))


# ---- ABI: argument checks come before any launch -------------------------------------------------------------------
def test_regrid_entry_points_reject_bad_arguments():
    lib = _lib.load()
    null, a, b, c, d = (ctypes.c_void_p(v) for v in (0, 4096, 8192, 12288, 16384))
    M = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    box = (ctypes.c_int32 * 6)(0, 3, 0, 3, 0, 3)

    def call(src=a, lab=b, dtype=_lib.LABEL_U8, s=(4, 4, 4), m=M, bx=box, dd=(4, 4, 4), out=c, out_lab=d):
        return lib.fsg_affine_resample(src, lab, dtype, *s, m, bx, *dd, out, out_lab, 0.0, 0.0, 1, null)

    E = _lib.E_BADARG
    assert call(src=null, lab=null, out=null, out_lab=null) == E      # neither image nor label
    assert call(out=null) == E and call(out_lab=null) == E            # a pair given by half
    assert call(src=null) == E and call(lab=null) == E
    assert call(out=a) == E and call(out_lab=b) == E                   # in place
    assert call(m=null) == E and call(bx=null) == E
    assert call(dtype=3) == E and call(dtype=-1) == E
    assert call(s=(0, 4, 4)) == E and call(dd=(4, -1, 4)) == E
    assert call(bx=(ctypes.c_int32 * 6)(2, 1, 0, 3, 0, 3)) == E        # empty box
    assert call(bx=(ctypes.c_int32 * 6)(0, 4, 0, 3, 0, 3)) == E        # box leaves the source
    assert call(bx=(ctypes.c_int32 * 6)(-1, 3, 0, 3, 0, 3)) == E
    assert call(m=(ctypes.c_float * 12)(*([float("nan")] + [0.0] * 11))) == E
    big = (ctypes.c_int32 * 6)(0, 3, 0, 3, 0, 3)
    assert call(s=(1025, 4, 4), bx=big) == _lib.E_TOOBIG and call(dd=(4, 4, 1025)) == _lib.E_TOOBIG
    assert call(s=(1024, 4, 4), dd=(0, 4, 4)) == E
    assert lib.fsg_bbox_gt_f32(null, 4, 4, 4, 0.0, a, null) == E
    assert lib.fsg_bbox_gt_f32(a, 4, 4, 4, 0.0, null, null) == E
    assert lib.fsg_bbox_gt_f32(a, 4, 0, 4, 0.0, b, null) == E
    assert lib.fsg_bbox_gt_f32(a, 2048, 2048, 2048, 0.0, b, null) == _lib.E_TOOBIG
    assert (_lib.LABEL_U8, _lib.LABEL_I16, _lib.LABEL_F32) == (0, 1, 2)
    assert "fsg_regrid.hip" in __import__("fetalsyngen_amd._build", fromlist=["SOURCES"]).SOURCES


# ---- FetalTestDataset without transforms ---------------------------------------------------------------------------
def test_fetal_test_dataset_returns_raw_volumes(tmp_path):
    from fetalsyngen_amd import compat
    from fetalsyngen_amd.data.datasets import FetalTestDataset
    from tests.util_bids import write_tree

    bids, _seeds = write_tree(tmp_path, (16, 20, 12), ["sub-a01", "sub-b02"])
    ds = FetalTestDataset(str(bids), None)
    assert len(ds) == 2
    item = ds[1]
    assert item["name"] == "sub-b02"
    assert tuple(item["image"].shape) == (1, 16, 20, 12) and tuple(item["label"].shape) == (1, 16, 20, 12)
    assert item["image"].dtype == torch.float32 and item["label"].dtype == torch.int64
    seg = read_nifti(ds.segm_paths[1])[0]
    assert np.array_equal(item["label"][0].numpy(), seg.astype(np.int64))
    assert np.allclose(item["affine"], [[0.5, 0, 0, -10], [0, 0.5, 0, -10], [0, 0, 0.5, -10], [0, 0, 0, 1]])
    back = ds.reverse_transform(item)
    assert back is item  # no transforms: the identity
    only = FetalTestDataset(str(bids), ["sub-a01"])
    assert len(only) == 1 and only[0]["name"] == "sub-a01"
    compat.install(force=True)
    import fetalsyngen.data.datasets as mirrored

    assert mirrored.FetalTestDataset is FetalTestDataset

    calls = []

    class Tf:
        def __call__(self, data):
            calls.append("fwd")
            return {**data, "label": data["label"].float()}

        def inverse(self, data):
            calls.append("inv")
            return data

    ds2 = FetalTestDataset(str(bids), None, transforms=Tf())
    out = ds2[0]
    assert out["label"].dtype == torch.int64 and calls == ["fwd"]
    ds2.reverse_transform(out)
    assert calls == ["fwd", "inv"]


# ---- CLI -----------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    from fetalsyngen_amd import resample as cli

    args = cli.parse_args(["--bids_path", "B", "--out_path", "O"])
    assert (args.res, args.size, args.image_suffix, args.label_suffix, args.align) == (0.5, 256, "T2w", "dseg", "input")
    args = cli.parse_args(["--bids_path", "B", "--out_path", "O", "--res", "0.8", "--size", "128", "--align", "world",
                           "--image_suffix", "T1w", "--label_suffix", "drawem9_dseg"])
    assert (args.res, args.size, args.align, args.image_suffix, args.label_suffix) == (0.8, 128, "world", "T1w", "drawem9_dseg")
    for bad in (["--out_path", "O"], ["--bids_path", "B", "--out_path", "O", "--align", "x"],
                ["--bids_path", "B", "--out_path", "O", "--res", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_cli_writes_the_reference_tree(tmp_path, capsys):
    from fetalsyngen_amd import resample as cli

    bids = tmp_path / "bids"
    affine = np.diag([1.0, 1.0, 1.0, 1.0])
    rng = np.random.default_rng(2)
    for sub, ses in (("sub-01", "ses-01"), ("sub-01", "ses-02"), ("sub-02", None)):
        anat = bids / sub / (ses or "") / "anat"
        anat.mkdir(parents=True)
        stem = f"{sub}_{ses}" if ses else sub
        write_nifti(anat / f"{stem}_T2w.nii.gz", rng.random((6, 7, 8)).astype(np.float32), affine)
        write_nifti(anat / f"{stem}_dseg.nii.gz", rng.integers(0, 5, (6, 7, 8)).astype(np.int16), affine)
    (bids / "sub-03" / "ses-01" / "anat").mkdir(parents=True)  # no image: reported and skipped
    seen = []

    def stub(image, label, aff, res, size, align, device):  # stands in for the one device call
        seen.append((image.shape, image.dtype, label.dtype, res, size, align))
        out_aff, M, box = regrid.working_grid(image.shape, aff, (res,) * 3, (size,) * 3, align)
        out, lab, _p, _ok = R64.resample(image, label, M, box, (size,) * 3)
        return out.astype(np.float32), lab, out_aff

    rc = cli.main(["--bids_path", str(bids), "--out_path", str(tmp_path / "out"), "--res", "0.5", "--size", "16"], regrid_fn=stub)
    assert rc == 0 and len(seen) == 3 and seen[0] == ((6, 7, 8), np.float32, np.int16, 0.5, 16, "input")
    assert "Error processing sub-03/ses-01/anat" in capsys.readouterr().out
    files = sorted(str(p.relative_to(tmp_path / "out")) for p in (tmp_path / "out").rglob("*.nii.gz"))
    assert files == ["sub-01/ses-01/anat/sub-01_ses-01_T2w.nii.gz", "sub-01/ses-01/anat/sub-01_ses-01_dseg.nii.gz",
                     "sub-01/ses-02/anat/sub-01_ses-02_T2w.nii.gz", "sub-01/ses-02/anat/sub-01_ses-02_dseg.nii.gz",
                     "sub-02/anat/sub-02_T2w.nii.gz", "sub-02/anat/sub-02_dseg.nii.gz"]
    img, aff, pix = read_nifti(tmp_path / "out" / "sub-02" / "anat" / "sub-02_T2w.nii.gz")
    lab, aff_l, _ = read_nifti(tmp_path / "out" / "sub-02" / "anat" / "sub-02_dseg.nii.gz")
    assert img.shape == (16, 16, 16) and img.dtype == np.float32 and lab.dtype == np.int16
    assert np.allclose(pix, 0.5) and np.allclose(aff, aff_l)
    want_aff, _M, _b = regrid.working_grid((6, 7, 8), affine, (0.5,) * 3, (16,) * 3)
    assert np.allclose(aff, want_aff, atol=1e-6)
