"""Dataset boundary: mirror of `fetalsyngen.data.datasets.FetalSynthDataset`
(reference datasets.py:189-370; base-class file discovery :17-103).

Same constructor, `__len__`, `__getitem__`, `sample`, `sample_with_meta`, same output dict
(`image` float32 (1,H,W,D) on the CPU in [0,1], `label` int64 (1,H,W,D) on the CPU, `name`), same
`generation_params` keys, same `FileNotFoundError` / `RuntimeError` on missing / ambiguous files.

MI355X-side additions (opt-in, defaults keep the reference's contract):
  * decoded label volumes are cached on the device as uint8 (`SeedBank`) -- the reference re-reads
    and gunzips five NIfTI files per sample;
  * `return_device=True` keeps outputs on the GPU (uint8 labels) for device-side consumers;
  * `ShardedSynthStream` partitions a sample-index range over ranks (one process per GPU).
"""
from __future__ import annotations

import time
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from ..generator.model import FetalSynthGen
from ..utils.image_reading import NiftiReader, ras_reorient_affine, read_nifti


class SeedBank:
    """Per-subject decoded seed volumes, device resident (uint8), combined on demand.

    Pickling (DataLoader workers, reference fetalsyngen/test_dl.py:17-24): the state that travels is the HOST copy of the
    volumes (uint8 numpy arrays) and the device string; the worker uploads them on first use.  No device tensor, no
    address of the parent process crosses the process boundary."""

    def __init__(self, volumes: dict, device):
        self.device = device
        self._host = None
        self._vol = {
            n: {m: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(torch.uint8).to(device) for m, v in d.items()}
            for n, d in volumes.items()
        }
        self._cache = {}

    @property
    def vol(self):
        if self._vol is None:  # unpickled in another process: upload now
            self._vol = {n: {m: torch.from_numpy(v).to(self.device) for m, v in d.items()} for n, d in self._host.items()}
            self._host = None
        return self._vol

    def __getstate__(self):
        host = self._host
        if host is None:
            host = {n: {m: v.cpu().numpy() for m, v in d.items()} for n, d in self._vol.items()}
        return {"device": self.device, "host": host}

    def __setstate__(self, state):
        self.device, self._host, self._vol, self._cache = state["device"], state["host"], None, {}

    @property
    def nbytes(self) -> int:
        src = self._vol if self._vol is not None else self._host
        return sum(int(np.prod(v.shape)) for d in src.values() for v in d.values())

    def parts(self, mlabel2subclusters: dict):
        """The selected per-meta-label volumes (disjoint supports); `fsg_gmm_sample_u8x4` sums them on the fly."""
        vol = self._vol if self._vol is not None else self.vol
        return [vol[n][m] for m, n in sorted(mlabel2subclusters.items())]

    @property
    def shape(self):
        return tuple(next(iter(next(iter(self.vol.values())).values())).shape)

    def transformed(self, fn) -> "SeedBank":
        """A new bank whose volumes are `fn(volume)` of this one's (device-side, e.g. a roll or a flip: a cheap way to
        more distinct synthetic subjects)."""
        other = SeedBank.__new__(SeedBank)
        other.device = self.device
        other._host = None
        other._vol = {n: {m: fn(v).contiguous() for m, v in d.items()} for n, d in self.vol.items()}
        other._cache = {}
        return other

    def combined(self, mlabel2subclusters: dict) -> torch.Tensor:
        key = tuple(sorted(mlabel2subclusters.items()))
        hit = self._cache.get(key)
        if hit is None:
            hit = None
            for m, n in mlabel2subclusters.items():
                v = self.vol[n][m]
                hit = v.clone() if hit is None else hit + v  # disjoint supports: values stay < 50
            if len(self._cache) >= 8:
                self._cache.pop(next(iter(self._cache)))
            self._cache[key] = hit
        return hit


class LabelCache:
    """Byte-budgeted LRU of device-resident label volumes (per subject: the seed bank, the float32 segmentation and its
    uint8 twin -- 464 MiB at 256^3 with 6 x 4 seed volumes).

    The reference keeps nothing: it re-reads and gunzips five NIfTI files per sample (data/datasets.py:280-296,
    rand_gmm.py:82-99).  Here a subject's decoded volumes stay in HBM until the budget is exceeded; then the least recently
    used subjects are dropped and re-read from their files when they come up again (same values: the files are the source).
    `budget_bytes=None`: half of the HBM that is free when the first subject is inserted.  The most recent entry is never
    evicted (a budget smaller than one subject degrades to the reference's read-per-sample behaviour, not to an error).

    Eviction and in-flight kernels: the host runs several samples ahead of the GPU, so kernels already enqueued may still
    read an evicted volume.  Eviction happens only on a miss, i.e. next to tens of milliseconds of file decoding, so it
    simply waits for the device to drain (`torch.cuda.synchronize`) before the references are dropped -- stronger than
    `record_stream` marks and free of per-sample cost."""

    def __init__(self, device, budget_bytes: int | None = None, fraction: float = 0.5):
        from collections import OrderedDict

        self.device, self.budget_bytes, self.fraction = device, budget_bytes, fraction
        self.entries = OrderedDict()  # key -> (value, nbytes)
        self.bytes, self.hits, self.misses, self.evictions = 0, 0, 0, 0

    def __getstate__(self):  # a worker process starts with an empty cache of the same budget
        return {"device": self.device, "budget_bytes": self.budget_bytes, "fraction": self.fraction}

    def __setstate__(self, state):
        self.__init__(state["device"], state["budget_bytes"], state["fraction"])

    def __contains__(self, key):
        return key in self.entries

    def __len__(self):
        return len(self.entries)

    def peek(self, key):
        hit = self.entries.get(key)
        return None if hit is None else hit[0]

    def get(self, key, build):
        """The cached value of `key`, or `build() -> (value, nbytes)` inserted as the most recent entry."""
        hit = self.entries.get(key)
        if hit is not None:
            self.hits += 1
            self.entries.move_to_end(key)
            return hit[0]
        self.misses += 1
        value, nbytes = build()
        if self.budget_bytes is None:
            free = torch.cuda.mem_get_info(torch.device(self.device))[0] if torch.cuda.is_available() else (1 << 62)
            self.budget_bytes = int((free + nbytes) * self.fraction)
        self.entries[key] = (value, int(nbytes))
        self.bytes += int(nbytes)
        if self.bytes > self.budget_bytes and len(self.entries) > 1:
            if torch.cuda.is_available():
                torch.cuda.synchronize(torch.device(self.device))  # kernels in flight may still read what goes now
            while self.bytes > self.budget_bytes and len(self.entries) > 1:
                _k, (_v, nb) = self.entries.popitem(last=False)
                self.bytes -= nb
                self.evictions += 1
        return value


class FetalDataset:
    """Subject / session discovery in a BIDS tree."""

    def __init__(self, bids_path: str, sub_list: list[str] | None):
        self.bids_path = Path(bids_path)
        found = sorted(p.name for p in self.bids_path.glob("sub-*"))
        self.subjects = found if sub_list is None else [s for s in found if s in set(sub_list)]
        self.sub_ses = [(s, ses) for s in self.subjects for ses in self._get_ses(self.bids_path, s)]
        self.loader = NiftiReader()
        self.img_paths = self._load_bids_path(self.bids_path, "T2w")
        self.segm_paths = self._load_bids_path(self.bids_path, "dseg")

    @staticmethod
    def _sub_ses_string(sub, ses):
        return sub if ses is None else f"{sub}_{ses}"

    def _sub_ses_idx(self, idx):
        return self._sub_ses_string(*self.sub_ses[idx])

    @staticmethod
    def _get_ses(bids_path, sub):
        names = [d.name for d in (bids_path / sub).iterdir() if d.is_dir()]
        return sorted([None if "anat" in n else n for n in names], key=lambda x: x or "")

    @staticmethod
    def _get_pattern(sub, ses, suffix, extension=".nii.gz"):
        if ses is None:
            return f"{sub}/anat/{sub}*_{suffix}{extension}"
        return f"{sub}/{ses}/anat/{sub}_{ses}*_{suffix}{extension}"

    def _load_bids_path(self, path, suffix):
        out = []
        for sub, ses in self.sub_ses:
            pattern = self._get_pattern(sub, ses, suffix)
            files = list(Path(path).glob(pattern))
            if not files:
                raise FileNotFoundError(
                    f"No files found for requested subject {sub} in {path} ({pattern} returned nothing)")
            if len(files) > 1:
                raise RuntimeError(
                    f"Multiple files found for requested subject {sub} in {path} ({pattern} returned {files})")
            out.append(files[0])
        return out

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, idx):
        raise NotImplementedError("This method should be implemented in the child class.")


def _compact_label(label: torch.Tensor) -> torch.Tensor:
    """An integer label volume in the narrowest dtype the resample kernel reads (uint8 / int16), float32 as it is."""
    if label.dtype in (torch.uint8, torch.int16, torch.float32):
        return label
    if label.is_floating_point():
        return label.float()
    lo, hi = (int(label.min()), int(label.max())) if label.numel() else (0, 0)
    if 0 <= lo and hi <= 255:
        return label.to(torch.uint8)
    if -32768 <= lo and hi <= 32767:
        return label.to(torch.int16)
    raise ValueError(f"label values {lo}..{hi} do not fit the 16-bit labels the resample kernel reads")


class InferenceTransform:
    """The chain of the reference's configs/dataset/transforms/inference.yaml -- Orientation("RAS"), SignalFillEmpty,
    CropForeground (image > 0), Spacing (image bilinear, label nearest), SpatialPad + CenterSpatialCrop to `size`,
    ScaleIntensity(0, 1) -- as ONE resample on the device (`regrid.working_grid` + `kernels.affine_resample`) followed
    by the min/max and scale kernels, and its inverse.

    Callable on {"image", "label", "name", "affine"}: image / label (H,W,D) or (1,H,W,D), on any device; `affine` the
    voxel->world affine of those arrays (absent: the identity).  Returns a new dict: image (1,*size) float32 in [0,1],
    label (1,*size) in the dtype it came in, `affine` = the working grid's, and `native_shape`, `native_affine`, `M`
    (3x4 float64, working voxel index -> native voxel coordinate) and `box` for the way back.  `inverse(data)` resamples
    image (linear) and label (nearest) onto the native grid; intensities stay scaled, as with monai's ScaleIntensity.
    Outputs are on the CPU unless `return_device`."""

    def __init__(self, pixdim=(0.5, 0.5, 0.5), size=(256, 256, 256), crop_foreground=True, fill_empty=True, scale01=True,
                 align="input", device="cuda:0", return_device=False):
        self.pixdim = tuple(float(v) for v in np.broadcast_to(np.asarray(pixdim, dtype=np.float64), (3,)))
        self.size = tuple(int(v) for v in np.broadcast_to(np.asarray(size), (3,)))
        self.crop_foreground, self.fill_empty, self.scale01 = crop_foreground, fill_empty, scale01
        self.align, self.device, self.return_device = align, device, return_device

    def _volume(self, t, name):
        if t is None:
            return None, None
        t = torch.as_tensor(t)
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"{name}: expected (H,W,D) or (1,H,W,D), got {tuple(t.shape)}")
        return t, t.dtype

    def _resample(self, data, M, box, out_shape):
        from .. import kernels as K

        image, _ = self._volume(data.get("image"), "image")
        label, label_dtype = self._volume(data.get("label"), "label")
        if image is not None:
            image = image.to(self.device).float().contiguous()
        if label is not None:
            label = _compact_label(label.to(self.device)).contiguous()
        out, lab = K.affine_resample(image, label, M, box, out_shape, nan_is_zero=self.fill_empty)
        if lab is not None:
            lab = lab.to(label_dtype)
        return image, out, lab

    def _finish(self, data, out, lab, **extra):
        res = dict(data)
        if out is not None:
            res["image"] = (out if self.return_device else out.cpu()).unsqueeze(0)
        if lab is not None:
            res["label"] = (lab if self.return_device else lab.cpu()).unsqueeze(0)
        res.update(extra)
        return res

    def __call__(self, data: dict) -> dict:
        from .. import kernels as K
        from .. import regrid as R

        ref, _ = self._volume(data.get("image") if data.get("image") is not None else data.get("label"), "image")
        if ref is None:
            raise ValueError("need an image or a label")
        shape = tuple(int(n) for n in ref.shape)
        affine = np.asarray(data.get("affine", np.eye(4)), dtype=np.float64)
        box = None
        if self.crop_foreground and data.get("image") is not None:
            box = R.foreground_box(self._volume(data["image"], "image")[0].to(self.device).float().contiguous())
        affine_out, M, box = R.working_grid(shape, affine, self.pixdim, self.size, self.align, box)
        _src, out, lab = self._resample(data, M, box, self.size)
        if out is not None and self.scale01:
            out = K.scale(out, K.reduce_minmax(out), mode=1)
        return self._finish(data, out, lab, affine=affine_out, native_shape=shape, native_affine=affine, M=M,
                            box=[int(v) for v in box])

    def inverse(self, data: dict) -> dict:
        from .. import regrid as R

        for key in ("native_shape", "native_affine", "affine"):
            if key not in data:
                raise KeyError(f"inverse needs the {key!r} this transform recorded")
        shape = tuple(int(n) for n in data["native_shape"])
        M, box = R.inverse_map(shape, data["native_affine"], data["affine"], self.size)
        _src, out, lab = self._resample(data, M, box, shape)
        res = self._finish(data, out, lab, affine=np.asarray(data["native_affine"], dtype=np.float64))
        for key in ("native_shape", "native_affine", "M", "box"):
            res.pop(key, None)
        return res


class FetalTestDataset(FetalDataset):
    """Mirror of `fetalsyngen.data.datasets.FetalTestDataset` (reference datasets.py:106-186): loads image and
    segmentation of a subject for validation / inference.  `transforms`: any callable on the data dict with an optional
    `.inverse` (the reference passes a monai Compose; `InferenceTransform` is the device-side equivalent of its
    inference.yaml).  None returns the raw volumes, as the reference does; that path needs no GPU.  The dict additionally
    carries `affine`, the voxel->world affine of the RAS-oriented arrays (the reference's MetaTensors carry theirs)."""

    def __init__(self, bids_path: str, sub_list: list[str] | None, transforms=None):
        super().__init__(bids_path, sub_list)
        self.transforms = transforms

    def _load_data(self, idx):
        image = self.loader(self.img_paths[idx])
        segm = self.loader(self.segm_paths[idx])
        raw, affine, _ = read_nifti(self.img_paths[idx])
        if len(image.shape) == 3:
            image = image.unsqueeze(0)
            segm = segm.unsqueeze(0)
        elif len(image.shape) != 4:
            raise ValueError(f"Expected 3D or 4D image, got {len(image.shape)}D image.")
        name = self._sub_ses_string(*self.sub_ses[idx])
        return {"image": image, "label": segm.long(), "name": name, "affine": ras_reorient_affine(affine, raw.shape[:3])}

    def __getitem__(self, idx) -> dict:
        data = self._load_data(idx)
        if self.transforms:
            data = self.transforms(data)
        data["label"] = data["label"].long()
        return data

    def reverse_transform(self, data: dict) -> dict:
        if self.transforms:
            data = self.transforms.inverse(data)
        return data


class FetalSynthDataset(FetalDataset):
    seeds_from_images = None  # subclasses that build themselves without this constructor read seeds from what they were given
    regrid = None             # ... and their volumes are on the working grid already

    def __init__(
        self,
        bids_path: str,
        generator: FetalSynthGen,
        seed_path: str | None,
        sub_list: list[str] | None,
        load_image: bool = False,
        image_as_intensity: bool = False,
        cache_on_device: bool = True,
        return_device: bool = False,
        cache_bytes: int | None = None,
        base_seed: int | None = None,
        seeds_from_images: int | None = None,
        regrid=None,
    ):
        """`cache_bytes`: HBM budget of the decoded-label cache (`LabelCache`; None = half of the free HBM).
        `base_seed`: None keeps the reference's behaviour (`__getitem__` draws from the global generators as they stand);
        an integer makes `__getitem__(idx)` re-seed numpy's and torch's CPU generators with the key
        `(base_seed, epoch * len(self) + idx)` first (`sharding.seed_for_sample`), so a sample depends on its index only --
        not on which DataLoader worker produced it, nor on how many workers there are (`set_epoch` moves to fresh keys).
        `seeds_from_images`: None keeps the reference's behaviour (seeds come from the files under `seed_path`).  An integer,
        with `seed_path=None`: a subject's seed volumes for 1..`seeds_from_images` subclasses are generated on the device from
        its T2w + dseg on first use (`seedgen.generate_seeds`, key `seedgen.subject_key(base_seed, idx)`) and cached like
        file-loaded ones.
        `regrid`: None keeps today's behaviour (the files are on the working grid already).  `(pixdim, size)`: the T2w and
        dseg of a subject are regridded on load (`regrid.working_grid` with the file's affine, one `affine_resample`),
        before seed generation and the label cache see them; excludes `seed_path`, whose files are on the old grid."""
        if regrid is not None and seed_path is not None:
            raise ValueError("regrid and seed_path exclude each other: seed files are on the grid the volumes had before")
        if seed_path is not None and seeds_from_images is not None:
            raise ValueError("seed_path and seeds_from_images exclude each other: seeds are read from files or generated, not both")
        super().__init__(bids_path, sub_list)
        self.seeds_from_images = None if seeds_from_images is None else int(seeds_from_images)
        self.seeds_annotation = "feta"
        self.seed_path = Path(seed_path) if isinstance(seed_path, str) else None
        self.load_image = load_image
        self.generator = generator
        self.image_as_intensity = image_as_intensity
        self.cache_on_device = cache_on_device
        self.return_device = return_device
        self.base_seed, self.epoch = base_seed, 0
        self.regrid = None
        if regrid is not None:
            pixdim, size = regrid
            self.regrid = (tuple(float(v) for v in np.broadcast_to(np.asarray(pixdim, dtype=np.float64), (3,))),
                           tuple(int(v) for v in np.broadcast_to(np.asarray(size), (3,))))
        self._labels = LabelCache(generator.device, cache_bytes)
        if not self.image_as_intensity and isinstance(self.seed_path, Path):
            if not self.seed_path.exists():
                raise FileNotFoundError(f"Provided seed path {self.seed_path} does not exist.")
            self._load_seed_path()

    def _load_seed_path(self):
        self.seed_paths = {self._sub_ses_string(s, ses): defaultdict(dict) for s, ses in self.sub_ses}
        avail = [int(p.name.replace("subclasses_", "")) for p in self.seed_path.glob("subclasses_*")]
        for n_sub in range(min(avail), max(avail) + 1):
            folder = self.seed_path / f"subclasses_{n_sub}"
            if not folder.exists():
                raise FileNotFoundError(f"Provided seed path {folder} does not exist.")
            for m in range(1, 5):
                files = self._load_bids_path(folder, f"mlabel_{m}")
                for (s, ses), f in zip(self.sub_ses, files):
                    self.seed_paths[self._sub_ses_string(s, ses)][n_sub][m] = f

    def set_epoch(self, epoch: int):
        """With `base_seed`: sample keys become (base_seed, epoch * len(self) + idx)."""
        self.epoch = int(epoch)

    # A pickled dataset (DataLoader worker, reference fetalsyngen/test_dl.py:17-24) carries paths and configuration only: the
    # worker's LabelCache starts empty and re-reads the label files on first use.
    def __getstate__(self):
        return dict(self.__dict__)  # LabelCache / FetalSynthGen / SeedBank drop their process-local state themselves

    def _regridded(self, idx):
        """(float32 device image, float32 device segmentation) of subject `idx` on the working grid of `self.regrid`."""
        from .. import kernels as K
        from .. import regrid as R

        img, affine, _ = read_nifti(self.img_paths[idx])
        seg, _seg_affine, _ = read_nifti(self.segm_paths[idx])
        if img.shape != seg.shape or img.ndim != 3:
            raise ValueError(f"{self.img_paths[idx]}: image {img.shape} and segmentation {seg.shape} must be 3-D and of one shape")
        dev = self.generator.device
        _affine_out, M, box = R.working_grid(img.shape, affine, self.regrid[0], self.regrid[1])
        image = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(dev)
        label = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.float32)).to(dev)
        return K.affine_resample(image, label, M, box, self.regrid[1])

    def _keyed_images(self) -> bool:
        """Keyed mode with `load_image`: the subject's device image (and, without seeds, its intensity prior) are cached with
        its labels, so that the sample takes the keyed single-call path.  The other modes load the image per sample as before."""
        return bool(self.load_image and self.cache_on_device and self.generator._is_keyed())

    def _has_seeds(self) -> bool:
        return (self.seed_path is not None or self.seeds_from_images is not None) and not self.image_as_intensity

    def _subject(self, idx):
        """(bank | None, float32 device segmentation, uint8 twin | None[, device image, prior | None]) of subject `idx` through
        the LRU; the last two in keyed mode with `load_image` only (`_keyed_images`), counted against the byte budget."""
        name = self._sub_ses_idx(idx)

        def build():
            bank, nbytes = None, 0
            if self.seed_path is not None and not self.image_as_intensity:
                vols = {n: {m: self.loader(p).numpy() for m, p in d.items()} for n, d in self.seed_paths[name].items()}
                bank = SeedBank(vols, self.generator.device)
                nbytes += bank.nbytes
            if self.regrid is not None:
                image, dev = self._regridded(idx)
                host = dev.cpu()
            else:
                image = None
                host = self.loader(self.segm_paths[idx]).float()
                dev = host.to(self.generator.device)
            if self.seeds_from_images is not None and not self.image_as_intensity:
                from .. import seedgen

                if image is None:
                    image = self.loader(self.img_paths[idx]).float().to(self.generator.device)
                bank = SeedBank(seedgen.generate_seeds(image, dev, self.seeds_from_images, self.seeds_annotation,
                                                       key=seedgen.subject_key(self.base_seed, idx)), self.generator.device)
                nbytes += bank.nbytes
            # uint8 twin for the label gather when the segmentation is integer valued in 0..255 (always the
            # case for dseg files); results are identical, the kernel reads 1 byte instead of 4 per voxel
            ok = bool(torch.equal(host, host.round()) and host.min() >= 0 and host.max() <= 255)
            twin = dev.to(torch.uint8) if ok else None
            if ok:
                self.generator.register_label_twin(dev, twin)
            nbytes += dev.numel() * 4 + (dev.numel() if ok else 0)
            if self._keyed_images():
                if image is None:
                    image = self.loader(self.img_paths[idx]).float().to(self.generator.device)
                image, prior = image.contiguous(), None
                nbytes += image.numel() * 4
                if not self._has_seeds():  # the image is the intensity prior: a constant of the subject
                    prior = self.generator._intensity_prior(image)
                    self.generator.register_image_prior(image, prior)
                    nbytes += prior.numel() * 4
                return (bank, dev, twin, image, prior), nbytes
            return (bank, dev, twin), nbytes

        return self._labels.get(idx, build)

    def _seeds_for(self, name, idx=None):
        if not self.cache_on_device and self.seeds_from_images is None:
            return self.seed_paths[name]
        if idx is None:
            idx = [self._sub_ses_idx(k) for k in range(len(self.sub_ses))].index(name)
        return self._subject(idx)[0]

    def _segmentation(self, idx):
        if not self.cache_on_device:
            return self._regridded(idx)[1] if self.regrid is not None else self.loader(self.segm_paths[idx])
        return self._subject(idx)[1]

    def _segmentation_u8(self, idx):
        if not self.cache_on_device:
            return None
        hit = self._labels.peek(idx)
        return hit[2] if hit is not None else None

    def sample(self, idx, genparams: dict = {}):
        image = None
        if self._keyed_images():
            image = self._subject(idx)[3]
        elif self.load_image:
            image = self._regridded(idx)[0] if self.regrid is not None else self.loader(self.img_paths[idx]).float()
        segm = self._segmentation(idx)
        name = self._sub_ses_idx(idx)
        seeds = None
        if (self.seed_path is not None or self.seeds_from_images is not None) and not self.image_as_intensity:
            seeds = self._seeds_for(name, idx)
        generation_params = {
            "idx": idx,
            "img_paths": str(self.img_paths[idx]),
            "segm_paths": str(self.img_paths[idx]),  # sic: the reference logs the image path here (ref :301)
            "seeds": str(self.seed_path),
        }
        key = None
        if genparams and self.base_seed is not None and "key" not in genparams and self.generator._is_keyed():
            # keyed mode: `sample_with_meta(idx, {...})` is `self[idx]` with those parameters fixed
            from .. import sharding

            key = sharding.sample_key(self.base_seed, self.epoch * len(self) + int(idx))
        t0 = time.time()
        gen_output, segmentation, image, synth_params = self.generator._pipeline(
            image, segm, seeds, genparams, scale01=True, key=key,
            segmentation_u8=self._segmentation_u8(idx) if self.return_device else None, labels_u8=self.return_device)
        if image is not None:
            from .. import kernels as K

            image = K.scale(image.contiguous(), K.reduce_minmax(image.contiguous()), mode=1)
        if self.return_device:
            label = segmentation if segmentation.dtype == torch.uint8 else segmentation.to(torch.uint8)
        else:
            gen_output = gen_output.cpu()
            label = segmentation.cpu().long()
            image = image.cpu() if image is not None else None
        generation_params = {**generation_params, **synth_params}
        generation_params["generation_time"] = time.time() - t0
        data_out = {"image": gen_output.unsqueeze(0), "label": label.unsqueeze(0), "name": name}
        return data_out, generation_params

    def sample_batch(self, indices, genparams_list=None, streams: int = 1):
        """B subjects with one `FetalSynthGen.sample_batch` call (cached label volumes): what a
        DataLoader with batch_size=B would collate from B `__getitem__` calls (reference data/datasets.py:310-325) --
        {"image": (B,1,H,W,D) float32 in [0,1], "label": (B,1,H,W,D) int64, "name": [B]} on the CPU, or on the device with
        uint8 labels when `return_device` -- and the list of B generation_params.  Same draws, same values as B
        consecutive `sample` calls.
        With `load_image` the batch also carries "real_image": the deformed images scaled to [0,1] as `sample` scales them,
        (B,1,H,W,D) float32.  In keyed mode with a `base_seed` such a batch takes the keyed path, sample b under the key
        `__getitem__(indices[b])` would announce, so it equals B `__getitem__` calls bit for bit."""
        has_seeds = self._has_seeds()
        if self.image_as_intensity and not self.load_image:
            raise ValueError("If no seeds are passed, an image must be loaded to be used as intensity prior!")
        if (not has_seeds and not self.load_image) or not self.cache_on_device:
            raise ValueError("sample_batch serves device-cached subjects (cache_on_device=True) with seeds, an image "
                             "(load_image=True), or both")
        indices = [int(i) for i in indices]
        names = [self._sub_ses_idx(i) for i in indices]
        t0 = time.time()
        keys = None
        if self._keyed_images():
            images = [self._subject(i)[3] for i in indices]
            if self.base_seed is not None:  # (with a genparams_list too: sample b is its key's sample with those values fixed)
                from .. import sharding

                keys = [sharding.sample_key(self.base_seed, self.epoch * len(self) + i) for i in indices]
        elif self.load_image:
            images = [self._regridded(i)[0] if self.regrid is not None else self.loader(self.img_paths[i]).float() for i in indices]
        else:
            images = [None] * len(indices)
        items = [(img, self._segmentation(i), self._seeds_for(n, i) if has_seeds else None)
                 for img, i, n in zip(images, indices, names)]
        out, seg, imgs, params = self.generator.sample_batch(items, genparams_list, scale01=True, streams=streams,
                                                             labels_u8=self.return_device, keys=keys)
        if not torch.is_tensor(out):
            raise ValueError("sample_batch needs subjects of one shape")
        real = None
        if self.load_image:
            from .. import kernels as K

            real = torch.stack([K.scale(im.contiguous(), K.reduce_minmax(im.contiguous()), mode=1) for im in imgs]).unsqueeze(1)
        if self.return_device:
            image, label = out.unsqueeze(1), seg.unsqueeze(1)
        else:
            image, label = out.cpu().unsqueeze(1), seg.cpu().long().unsqueeze(1)
            real = real.cpu() if real is not None else None
        dt = time.time() - t0
        gps = []
        for i, p_ in zip(indices, params):
            gps.append({"idx": i, "img_paths": str(self.img_paths[i]), "segm_paths": str(self.img_paths[i]),
                        "seeds": str(self.seed_path), **p_, "generation_time": dt / max(len(indices), 1)})
        batch = {"image": image, "label": label, "name": names}
        if real is not None:
            batch["real_image"] = real
        return batch, gps

    def __getitem__(self, idx) -> dict:
        if self.base_seed is not None:
            from .. import sharding

            if self.generator._is_keyed():
                sharding.announce_key(self.base_seed, self.epoch * len(self) + int(idx))
            else:
                sharding.seed_for_sample(self.base_seed, self.epoch * len(self) + int(idx))
        data_out, generation_params = self.sample(idx)
        self.generation_params = generation_params
        return data_out

    def sample_with_meta(self, idx: int, genparams: dict = {}) -> dict:
        data, generation_params = self.sample(idx, genparams=genparams)
        data["generation_params"] = generation_params
        return data


class MemorySynthDataset(FetalSynthDataset):
    """`FetalSynthDataset` over label volumes that are already decoded (no BIDS tree, no files): subject k is
    `(segmentations[k], seed_volumes[k])` with `seed_volumes[k][n_sub][mlabel] -> integer array`, uploaded once.
    Same `sample` / `__getitem__` / `sample_with_meta` contract; used by the synthetic-label benchmarks
    (BASELINE configs 2, 3, 5) and wherever the labels come from somewhere other than NIfTI files."""

    def __init__(self, generator: FetalSynthGen, segmentations, seed_volumes, return_device: bool = False,
                 names=None, base_seed: int | None = None):
        if len(segmentations) != len(seed_volumes) or not len(segmentations):
            raise ValueError("need one seed-volume table per segmentation (and at least one subject)")
        self.bids_path, self.seed_path = Path("<memory>"), Path("<memory>")
        self.subjects = list(names) if names is not None else [f"sub-mem{k:03d}" for k in range(len(segmentations))]
        self.sub_ses = [(s, None) for s in self.subjects]
        self.loader = NiftiReader()
        self.img_paths = self.segm_paths = ["<memory>"] * len(self.subjects)
        self.load_image, self.image_as_intensity = False, False
        self.generator = generator
        self.cache_on_device, self.return_device = True, return_device
        self.base_seed, self.epoch = base_seed, 0
        self._labels = None  # nothing to evict: there are no files to re-read from
        self._mem = []       # per subject: (bank, float32 device segmentation, uint8 twin)
        dev = generator.device
        for seg, vols in zip(segmentations, seed_volumes):
            d = torch.as_tensor(np.asarray(seg) if not torch.is_tensor(seg) else seg).float().to(dev).contiguous()
            self._mem.append((vols if isinstance(vols, SeedBank) else SeedBank(vols, dev), d, d.to(torch.uint8)))
            generator.register_label_twin(d, self._mem[-1][2])

    # Pickling: the label volumes themselves travel (host copies; there is no file to re-read them from) and are uploaded by
    # the worker on first use.
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mem"] = [(bank, seg.cpu().numpy() if torch.is_tensor(seg) else seg, None) for bank, seg, _t in self._mem]
        return state

    def _subject(self, idx):
        bank, seg, twin = self._mem[idx]
        if not torch.is_tensor(seg):  # unpickled in another process: upload now
            seg = torch.from_numpy(seg).to(self.generator.device).contiguous()
            bank, seg, twin = self._mem[idx] = (bank, seg, seg.to(torch.uint8))
            self.generator.register_label_twin(seg, twin)
        return bank, seg, twin

    def _segmentation_u8(self, idx):
        return self._subject(idx)[2]
