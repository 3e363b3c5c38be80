"""GPU: the affine resample and the foreground box (csrc/fsg_regrid.hip, fetalsyngen_amd/regrid.py) against the float64
restatement tests/util_regrid64.py, which tests/test_regrid64_reference.py pins to scipy on the CPU; InferenceTransform,
FetalTestDataset and the dataset's regrid hook end to end.

Exact cases use integer-valued images (0..1023) and maps whose products and sums are representable in float32: every weight
is a multiple of 1/4, so the kernel's float32 blends are exact and the comparison is bit for bit.

General affines.  Coordinates are float32, within 2^-13 of their float64 value (tests/test_regrid64_reference.py).  Labels must
equal the restatement except at voxels whose float64 coordinate lies within DELTA = 2^-12 of a half-integer (label ties; the
faces of the inside box sit on half-integers too); those voxels are excluded and must be <= 0.5 % (the restatement alone:
0.137 % for transform A, 0.146 % for B).  Image: |diff| <= 3 * 2^-13 * G + 8 * 2^-24 * V, G the largest face-neighbour
difference of the input, V its largest absolute value -- coordinate error times slope plus the rounding of the blend.
Measured on the MI355X: A: 0.137 % excluded, 0 labels differ, largest image difference 1.785e-6 (bound
3.665e-4); B: 0.146 % excluded, 0 labels differ outside the exclusion (13 inside it), 1.372e-5 (bound 3.666e-4); round trip on
an odd-sized working grid: labels and image exact.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import util_regrid64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "sub-sta21_rec-irtk_T2w_dseg.nii.gz"
DELTA = 2.0 ** -12
LABEL_DTYPES = {"uint8": np.uint8, "int16": np.int16, "float32": np.float32}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(image, label, M, box, out_shape, **kw):
    from fetalsyngen_amd import regrid

    out, lab = regrid.resample(dev(image), dev(label), M, box, out_shape, **kw)
    torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy()), (None if lab is None else lab.cpu().numpy())


def whole(shape):
    return [0, shape[0] - 1, 0, shape[1] - 1, 0, shape[2] - 1]


def source(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1024, shape).astype(np.float32), rng.integers(0, 200, shape)


def perm_flip_map(shape, perm, flips):
    """Output axis a reads source axis a from output axis perm[a], mirrored when flips[a]."""
    M = np.zeros((3, 4))
    out_shape = [0, 0, 0]
    for a in range(3):
        M[a, perm[a]] = -1.0 if flips[a] else 1.0
        M[a, 3] = shape[a] - 1 if flips[a] else 0.0
        out_shape[perm[a]] = shape[a]
    return M, tuple(out_shape)


def exact_cases():
    import itertools

    cases = []
    up = np.concatenate([np.diag([0.5, 0.5, 0.5]), np.zeros((3, 1))], axis=1)
    cases.append(("2x_half_integers", (19, 23, 17), (38, 46, 34), up, None))        # p = 0, 0.5, 1, ..: ties; last = hi + 0.5
    quarter = up.copy()
    quarter[:, 3] = -0.25
    cases.append(("2x_working_grid", (19, 23, 17), (38, 46, 34), quarter, None))     # working_grid's own 1 mm -> 0.5 mm map
    for perm in itertools.permutations(range(3)):
        for flips in itertools.product((0, 1), repeat=3):
            M, out_shape = perm_flip_map((5, 7, 6), perm, flips)
            cases.append((f"perm{perm}_flip{flips}", (5, 7, 6), out_shape, M, None))
    shift = np.concatenate([np.eye(3), np.array([[-2.0], [4.0], [-3.0]])], axis=1)
    cases.append(("shift_pad_crop", (12, 9, 21), (16, 16, 16), shift, None))          # pad on one side, crop on the other
    thin = np.array([[1.0, 0, 0, -1.0], [0, 0.25, 0, -0.5], [0, 0, 0.5, 0.0]])
    cases.append(("extent_one", (7, 1, 9), (8, 5, 17), thin, None))
    away = np.concatenate([np.eye(3), np.array([[100.0], [0.0], [0.0]])], axis=1)
    cases.append(("all_outside", (12, 9, 21), (6, 5, 21), away, None))
    inner = np.array([[0.5, 0, 0, 0.0], [0, 0.5, 0, 0.0], [0, 0, 1.0, 0.0]])
    cases.append(("inner_box", (12, 9, 21), (24, 18, 21), inner, [2, 8, 1, 6, 4, 15]))
    return cases


@pytest.mark.parametrize("mode", ["uint8", "int16", "float32", "image_only", "label_only"])
def test_exact_cases_bit_for_bit(mode):
    zs = set()
    for name, shape, out_shape, M, box in exact_cases():
        img, lab = source(shape, len(name))
        lab = lab.astype(LABEL_DTYPES.get(mode, np.uint8))
        if mode == "int16":
            lab = (lab * 150 - 15000).astype(np.int16)  # values beyond 8 bits, negative ones too
        image = None if mode == "label_only" else img
        label = None if mode == "image_only" else lab
        box = whole(shape) if box is None else box
        M32 = M.astype(np.float32)
        ref, ref_lab, _p, ok = R.resample(image, label, M32, box, out_shape, fill=-3.0, fill_label=7)
        got, got_lab = run(image, label, M32, box, out_shape, fill=-3.0, fill_label=7)
        if name == "all_outside":
            assert not ok.any()
        elif name in ("shift_pad_crop", "inner_box"):
            assert ok.any() and not ok.all()
        if image is not None:
            assert got.dtype == np.float32 and got.shape == tuple(out_shape)
            assert np.array_equal(got, ref.astype(np.float32)), f"{name}: image differs at {int((got != ref).sum())} voxels"
        else:
            assert got is None
        if label is not None:
            assert got_lab.dtype == lab.dtype and np.array_equal(got_lab, ref_lab), f"{name}: labels differ"
        else:
            assert got_lab is None
        zs.add(out_shape[2])
    assert {17, 21, 34} <= zs  # z extents that are no multiple of four: quads that wrap rows, and the scalar tail


def test_nan_reads_as_zero_only_when_asked():
    img, lab = source((12, 9, 21), 5)
    img[3:5, 2, 7:9] = np.nan
    M = np.concatenate([np.diag([0.5, 0.5, 0.5]), np.zeros((3, 1))], axis=1).astype(np.float32)
    for flag in (True, False):
        ref, _l, _p, _ok = R.resample(img, None, M, whole(img.shape), (24, 18, 42), nan_is_zero=flag)
        got, _gl = run(img, None, M, whole(img.shape), (24, 18, 42), nan_is_zero=flag)
        assert np.isnan(ref).any() != flag
        assert np.array_equal(got, ref.astype(np.float32), equal_nan=True)


GENERAL = {"A": (0.43, (3.1, 9.7, 2.2), (19, 23, 17), (37, 30, 42)),
           "B": (0.77, (20.3, -11.7, 31.9), (96, 96, 96), (128, 128, 128))}


def image_bound(img):
    G, V = R.face_gradient(img)
    return 3 * 2.0 ** -13 * G + 8 * 2.0 ** -24 * V


@pytest.mark.parametrize("which", ["A", "B"])
def test_general_affine(which):
    scale, offset, shape, out_shape = GENERAL[which]
    M = np.concatenate([R.rotation(20, -11, 7) * scale, np.asarray(offset)[:, None]], axis=1).astype(np.float32)
    rng = np.random.default_rng(11)
    img = rng.random(shape, dtype=np.float32)
    lab = rng.integers(0, 250, shape).astype(np.uint8)
    ref, ref_lab, p, ok = R.resample(img, lab, M, whole(shape), out_shape)
    got, got_lab = run(img, lab, M, whole(shape), out_shape)
    excluded = R.near_decision(p, whole(shape), DELTA)
    share = float(excluded.mean())
    wrong = (got_lab != ref_lab) & ~excluded
    err = float(np.abs(got.astype(np.float64) - ref)[~excluded].max())
    bound = image_bound(img)
    print(f"{which}: excluded {100 * share:.3f} %, inside {100 * ok.mean():.1f} %, labels differing outside the exclusion "
          f"{int(wrong.sum())} (inside it {int(((got_lab != ref_lab) & excluded).sum())}), max |image diff| {err:.3e}, bound {bound:.3e}")
    assert ok.any() and not ok.all()
    assert share <= 0.005
    assert not wrong.any()
    assert err <= bound


def test_bbox():
    from fetalsyngen_amd import kernels as K

    rng = np.random.default_rng(3)
    vols = []
    for shape in ((33, 5, 70), (40, 36, 44), (1, 1, 1), (300, 3, 2)):
        v = np.zeros(shape, dtype=np.float32)
        idx = rng.integers(0, v.size, max(v.size // 500, 1))
        v.reshape(-1)[idx] = rng.random(idx.size, dtype=np.float32) + 0.01
        vols.append(v)
        w = -rng.random(shape, dtype=np.float32)  # nothing above the threshold 0 ...
        w.reshape(-1)[idx[:3]] = 0.5
        vols.append(w)
    for corner in np.ndindex(2, 2, 2):
        v = np.zeros((33, 5, 70), dtype=np.float32)
        v[tuple(c * (n - 1) for c, n in zip(corner, v.shape))] = 2.0
        vols.append(v)
    vols.append(np.zeros((33, 5, 70), dtype=np.float32))
    nan = np.zeros((33, 5, 70), dtype=np.float32)
    nan[0, 0, 0] = nan[32, 4, 69] = np.nan
    nan[10:12, 2, 30:33] = 1.0
    vols.append(nan)
    vols.append(np.full((6, 5, 7), np.nan, dtype=np.float32))
    for v in vols:
        for thr in (0.0, 0.4):
            got = K.bbox_gt(dev(v), thr).cpu().numpy().tolist()
            assert got == R.bbox_gt(v, thr), (v.shape, thr)
    from fetalsyngen_amd import regrid

    assert regrid.foreground_box(dev(vols[-1])) is None and regrid.foreground_box(dev(nan)) == [10, 11, 2, 2, 30, 32]


def test_round_trip_through_the_working_grid():
    from fetalsyngen_amd import regrid
    from fetalsyngen_amd.phantom import make_seed_volumes

    shape = (40, 36, 44)
    seg, _seeds = make_seed_volumes(shape)
    lab = seg.astype(np.uint8)
    rng = np.random.default_rng(8)
    img = (seg * 30 + rng.random(shape) * 5).astype(np.float32)
    affine = np.diag([1.0, 1.0, 1.0, 1.0])
    affine[:3, 3] = [-20.0, -18.0, -22.0]
    # 0.5 mm grid that holds the 79 x 71 x 87 positions the phantom spans.  Odd sizes: under the centring rule native voxel n then
    # sits ON working voxel 2 n + const (an even size would put it half-way between two, and linear up-sampling followed by
    # linear down-sampling between samples is a smoothing, not a round trip)
    size = (95, 81, 97)
    affine_out, M, box = regrid.working_grid(shape, affine, (0.5, 0.5, 0.5), size)
    assert np.allclose(2 * M[:, 3], np.rint(2 * M[:, 3]), atol=1e-12)
    fwd, fwd_lab = regrid.resample(dev(img), dev(lab), M, box, size)
    Minv, binv = regrid.inverse_map(shape, affine, affine_out, size)
    back, back_lab = regrid.resample(fwd, fwd_lab, Minv, binv, shape)
    torch.cuda.synchronize()
    assert np.array_equal(back_lab.cpu().numpy(), lab)
    err = float(np.abs(back.cpu().numpy().astype(np.float64) - img).max())
    print(f"round trip: max |image diff| {err:.3e}, bound {image_bound(img):.3e}")
    assert err <= image_bound(img)


# ---- end to end on the bundled segmentation ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(tmp_path_factory):
    """A BIDS subject cut from the bundled 0.5 mm segmentation (its float copy is the image).  The centring rule puts the
    centre of the foreground box on the centre of the output grid: with an even output size that is a whole-voxel shift
    -- which restoring labels exactly needs -- only on axes where the box has an even extent, so the image's foreground is
    trimmed by one plane on the axes where it is odd."""
    from fetalsyngen_amd.utils.image_reading import read_nifti, write_nifti

    arr, affine, _ = read_nifti(GOLDEN)
    cut = (slice(56, 192), slice(60, 212), slice(72, 208))
    seg = np.ascontiguousarray(arr[cut]).astype(np.float32)
    affine = affine.copy()
    affine[:3, 3] += affine[:3, :3] @ np.array([56.0, 60.0, 72.0])
    image = seg.copy()
    box = R.bbox_gt(image)
    for a in range(3):
        if (box[2 * a + 1] - box[2 * a]) % 2 == 0:  # odd extent
            image[tuple(slice(None) if b != a else box[2 * a] for b in range(3))] = 0.0
    box = R.bbox_gt(image)
    assert all((box[2 * a + 1] - box[2 * a]) % 2 == 1 for a in range(3))
    root = tmp_path_factory.mktemp("regrid_bids")
    anat = root / "bids" / "sub-sta21" / "anat"
    anat.mkdir(parents=True)
    write_nifti(anat / "sub-sta21_rec-irtk_T2w.nii.gz", image, affine)
    write_nifti(anat / "sub-sta21_rec-irtk_T2w_dseg.nii.gz", seg, affine)
    return root / "bids", image, seg, affine, box


def test_inference_transform_end_to_end(subject):
    from fetalsyngen_amd.data.datasets import FetalTestDataset, InferenceTransform

    bids, image, seg, affine, box = subject
    tf = InferenceTransform(pixdim=(0.5, 0.5, 0.5), size=(64, 64, 64), device=DEV)
    ds = FetalTestDataset(str(bids), None, transforms=tf)
    item = ds[0]
    im, lab = item["image"], item["label"]
    assert tuple(im.shape) == (1, 64, 64, 64) and im.dtype == torch.float32 and not im.is_cuda
    assert tuple(lab.shape) == (1, 64, 64, 64) and lab.dtype == torch.int64 and item["name"] == "sub-sta21"
    assert float(im.min()) == 0.0 and float(im.max()) == 1.0
    assert set(np.unique(lab.numpy()).tolist()) <= set(np.unique(seg).astype(np.int64).tolist())
    assert item["native_shape"] == seg.shape and np.allclose(item["native_affine"], affine, atol=1e-5)
    assert item["box"] == box
    M = np.asarray(item["M"])
    centre = np.array([(box[0] + box[1]) / 2, (box[2] + box[3]) / 2, (box[4] + box[5]) / 2])
    assert np.allclose(M @ np.array([31.5, 31.5, 31.5, 1.0]), centre, atol=1e-9)
    # against the restatement: same labels, image = scaled trilinear sample (an integer shift here: exact)
    ref, ref_lab, p, ok = R.resample(image, seg.astype(np.int64), M.astype(np.float32), box, (64, 64, 64))
    assert np.array_equal(lab[0].numpy(), ref_lab)
    assert np.allclose(im[0].numpy(), (ref - ref.min()) / (ref.max() - ref.min()), atol=2e-7)
    back = ds.reverse_transform(item)
    bl = back["label"]
    assert tuple(bl.shape) == (1,) + seg.shape and tuple(back["image"].shape) == (1,) + seg.shape
    shift = np.rint(M[:, 3]).astype(int)
    assert np.allclose(M[:, :3], np.eye(3), atol=1e-12) and np.allclose(M[:, 3], shift, atol=1e-9)
    covered = np.zeros(seg.shape, dtype=bool)
    inner = tuple(slice(max(s, box[2 * a]), min(s + 64, box[2 * a + 1] + 1)) for a, s in enumerate(shift))
    covered[inner] = True  # native voxels that the working grid holds and that lie in the foreground box
    assert covered.sum() > 50 ** 3
    assert np.array_equal(bl[0].numpy()[covered], seg.astype(np.int64)[covered])
    outside = np.ones(seg.shape, dtype=bool)
    outside[tuple(slice(s, s + 64) for s in shift)] = False
    assert (bl[0].numpy()[outside] == 0).all()


def test_synth_dataset_regrids_on_load(subject):
    from fetalsyngen_amd.data.datasets import FetalSynthDataset
    from fetalsyngen_amd.generator.intensity.rand_gmm import ImageFromSeeds
    from tests.util_cases import DEFAULT_GEN_CLASSES, DEFAULT_SEED_LABELS, make_generator

    bids, _image, seg, _affine, _box = subject
    gen = make_generator((48, 48, 48), DEV, rng="keyed")
    gen.intensity_generator = ImageFromSeeds(1, 2, DEFAULT_SEED_LABELS, DEFAULT_GEN_CLASSES)  # subclass counts 1..2
    with pytest.raises(ValueError, match="regrid"):
        FetalSynthDataset(str(bids), gen, str(bids), None, regrid=((0.5, 0.5, 0.5), (48, 48, 48)))
    ds = FetalSynthDataset(str(bids), gen, None, None, base_seed=5, seeds_from_images=2, regrid=(0.5, 48))
    item = ds[0]
    assert tuple(item["image"].shape) == (1, 48, 48, 48) and tuple(item["label"].shape) == (1, 48, 48, 48)
    assert torch.isfinite(item["image"]).all() and 0.0 <= float(item["image"].min()) and float(item["image"].max()) <= 1.0
    assert set(np.unique(item["label"].numpy()).tolist()) <= set(np.unique(seg).astype(np.int64).tolist())
    bank, dev_seg, _twin = ds._subject(0)
    assert tuple(dev_seg.shape) == (48, 48, 48) and bank.shape == (48, 48, 48) and sorted(bank.vol) == [1, 2]
    c = [(n - 48) // 2 for n in seg.shape]  # whole-voxel centre crop: even extents, even size
    assert np.array_equal(dev_seg.cpu().numpy(), seg[c[0]:c[0] + 48, c[1]:c[1] + 48, c[2]:c[2] + 48])
