"""Seed generation on the GPU: what the reference does offline with `scripts/generate_seeds.py` (sklearn + monai).

Per subject: fuse the dseg labels into the four meta-labels (CSF, GM, WM, non-brain), then, for every subclass count
k = 2..max_subclasses and meta-label m, fit a 1-D Gaussian mixture to the T2w intensities inside m (EM, five k-means++
initialisations, best lower bound wins) and write `10 * m + c` for the component c a voxel falls in.  All (m, k, init) fits of
a subject are one batch of jobs for `fsg_em1d_fit`; nothing but the job tables, a 4 x 4096 intensity subsample (for the
initial centres) and the lower bounds (to pick the winners) crosses the host boundary.

Differences from the reference, by design:
  * components are numbered by ascending mean (sklearn leaves them in initialisation order, which depends on its random
    state; the generator draws every subclass's intensity i.i.d., so the numbering carries no meaning for it);
  * the result is a function of (image, segmentation, key): same key -> byte-identical volumes on every run and device count.

Command line (the reference's arguments and output tree):
    python -m fetalsyngen_amd.seedgen --bids_path BIDS --out_path OUT --max_subclasses 10 --annotation feta
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from pathlib import Path

import numpy as np
import torch

from . import _lib

KMAX = 16
N_INIT = 5
INIT_SAMPLE = 4096  # intensities per meta-label gathered for k-means++
FETA2META = {1: 1, 4: 1, 2: 2, 6: 2, 5: 3, 7: 3, 3: 3}
DHCP2META = {1: 1, 5: 1, 2: 2, 7: 2, 9: 2, 3: 3, 6: 3, 8: 3}
_M32 = np.uint64(0xFFFFFFFF)


# ----------------------------------------------------------------------------------------------------------------------
# host side of the initialisation: Philox4x32-10 (Salmon et al., SC'11; the counter layout of fsg_common.h) and k-means++
# ----------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key: int) -> np.ndarray:
    """(n, 4) uint32 blocks for counters `ctr` (n, 4) under the 64-bit `key`."""
    c = [np.asarray(ctr, np.uint64)[:, i] & _M32 for i in range(4)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c, axis=1).astype(np.uint32)


def init_stream(m: int, k: int, init: int) -> int:
    """Philox stream id of initialisation `init` of the (meta-label m, k components) fit."""
    return (0x5EED << 32) | (int(m) << 16) | (int(k) << 8) | int(init)


def uniforms(key: int, stream: int, count: int) -> np.ndarray:
    """`count` float64 uniforms in [0, 1) of stream `stream` under `key` (two per Philox block, 53 bits each)."""
    nblk = (count + 1) // 2
    ctr = np.zeros((nblk, 4), np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 2], ctr[:, 3] = stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF
    r = philox4x32_10(ctr, key).astype(np.uint64)
    hi = np.stack([r[:, 0], r[:, 2]], axis=1).reshape(-1) >> np.uint64(5)
    lo = np.stack([r[:, 1], r[:, 3]], axis=1).reshape(-1) >> np.uint64(6)
    return ((hi * np.uint64(1 << 26) + lo).astype(np.float64) / float(1 << 53))[:count]


def subsample_index(n: int, size: int = INIT_SAMPLE) -> np.ndarray:
    """Evenly spaced positions of the `size`-element subsample of a packed array of n intensities (all of them if n <= size)."""
    if n <= size:
        return np.arange(n, dtype=np.int64)
    return ((np.arange(size, dtype=np.float64) + 0.5) * (n / size)).astype(np.int64)


def kmeanspp_means(sample: np.ndarray, k: int, key: int, m: int, init: int) -> np.ndarray:
    """k initial centres from `sample` by k-means++ (Arthur & Vassilvitskii 2007: D^2 sampling, with the usual greedy
    variant of 2 + floor(ln k) candidates per step, the one of lowest potential kept).  Pure function of its arguments."""
    x = np.asarray(sample, np.float64)
    trials = 2 + int(math.log(k))
    u = uniforms(int(key), init_stream(m, k, init), 1 + (k - 1) * trials)
    centres = [x[min(int(u[0] * x.size), x.size - 1)]]
    d2 = (x - centres[0]) ** 2
    for c in range(1, k):
        pot = d2.sum()
        if not pot > 0:  # every sample coincides with a centre already
            centres.append(centres[-1])
            continue
        cdf = np.cumsum(d2)
        cand = np.minimum(np.searchsorted(cdf, u[1 + (c - 1) * trials: 1 + c * trials] * pot, side="right"), x.size - 1)
        nd2 = np.minimum(d2[None, :], (x[None, :] - x[cand][:, None]) ** 2)
        best = int(np.argmin(nd2.sum(axis=1)))
        centres.append(x[cand[best]])
        d2 = nd2[best]
    return np.array(centres, np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------
def _need_gpu(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("fetalsyngen_amd.seedgen runs on an MI355X (device='cuda:N') only; there is no CPU fallback")


def _stream(t):
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(t.device.index))


def _p(t):
    return C.c_void_p(t.data_ptr())


def meta_table(annotation):
    """(256-entry uint8 table, label cleared before the fusion or -1)."""
    if isinstance(annotation, str):
        if annotation not in ("feta", "dhcp"):
            raise ValueError("Unknown annotation type. Should be either 'feta' or 'dhcp'")
        mapping = FETA2META if annotation == "feta" else DHCP2META
    else:
        mapping = dict(annotation)
    table = np.zeros(256, np.uint8)
    for lab, meta in mapping.items():
        if not (0 < int(lab) < 256 and 0 <= int(meta) <= 4):
            raise ValueError(f"label -> meta-label entry {lab}: {meta} outside 1..255 -> 0..4")
        table[int(lab)] = int(meta)
    clear = 4 if annotation == "dhcp" else -1
    if clear >= 0:
        table[clear] = 0
    return table, clear


def _fuse(image, segmentation, annotation):
    _need_gpu(image, segmentation)
    if image.shape != segmentation.shape:
        raise ValueError(f"image {tuple(image.shape)} and segmentation {tuple(segmentation.shape)} differ in shape")
    img = image.contiguous()
    if img.dtype != torch.float32:
        img = img.float()
    seg = segmentation.contiguous()
    if seg.dtype not in (torch.uint8, torch.float32):
        seg = seg.float()
    lib = _lib.load()
    table, clear = meta_table(annotation)
    dev = img.device
    n = img.numel()
    table_d = torch.from_numpy(table).to(dev)
    meta = torch.empty(img.shape, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    px = torch.empty(n, dtype=torch.float32, device=dev)
    pidx = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(max(int(lib.fsg_seed_meta_work_bytes(n)), 16), dtype=torch.uint8, device=dev)
    u8 = seg.dtype == torch.uint8
    _lib.check(lib.fsg_seed_meta_pack(_p(seg) if u8 else None, None if u8 else _p(seg), _p(img), n, _p(table_d), clear, _p(meta),
                                      _p(counts), _p(px), _p(pidx), _p(work), _stream(img)), "fsg_seed_meta_pack")
    return meta, counts, px, pidx


def meta_labels(image, segmentation, annotation="feta") -> torch.Tensor:
    """uint8 device volume of meta-labels (1 CSF, 2 GM, 3 WM, 4 non-brain, 0 nothing) of a T2w + dseg pair."""
    return _fuse(image, segmentation, annotation)[0]


def meta_pack(image, segmentation, annotation="feta"):
    """-> (meta volume, counts[4] (host ints), packed intensities, packed voxel indices): the intensities of meta-label 1, then
    2, 3, 4, each in voxel order, with the flat voxel index of each."""
    meta, counts, px, pidx = _fuse(image, segmentation, annotation)
    return meta, [int(v) for v in counts.cpu().tolist()], px, pidx


class _Batch:
    """Job tables of one `fsg_em1d_fit` call."""

    def __init__(self, lib):
        self.tile = int(lib.fsg_em1d_tile())
        self.rows, self.tol, self.params = [], [], []

    def add(self, xoff, n, k, max_iter, mode, tol, w=None, mu=None, var=None):
        p = np.zeros((3, KMAX), np.float64)
        p[0, :k] = 1.0 / k if w is None else w
        p[1, :k] = 0.0 if mu is None else mu
        p[2, :k] = 1.0 if var is None else var
        self.rows.append([int(xoff), int(n), int(k), 0, 0, int(max_iter), int(mode), 0])
        self.tol.append(float(tol))
        self.params.append(p)
        return len(self.rows) - 1

    def tables(self, order=None):
        order = list(range(len(self.rows))) if order is None else list(order)
        jobs = np.array([self.rows[i] for i in order], np.int64).reshape(-1, 8)
        nblk = (jobs[:, 1] + self.tile - 1) // self.tile
        jobs[:, 4] = nblk
        jobs[:, 3] = np.cumsum(nblk) - nblk
        tol = np.array([self.tol[i] for i in order], np.float64)
        params = np.stack([self.params[i] for i in order])
        return np.ascontiguousarray(jobs), tol, params, int(nblk.sum())


class _Fit:
    """A batch that ran: device results + the tables they belong to (kept alive until read)."""

    def __init__(self, x, batch, order=None):
        lib = _lib.load()
        self.x, self.order = x, (list(range(len(batch.rows))) if order is None else list(order))
        self.jobs, self.tol, params, self.nblocks = batch.tables(self.order)
        dev = x.device
        nj = len(self.order)
        self.params = torch.from_numpy(params).to(dev)
        self.lb = torch.empty(nj, dtype=torch.float64, device=dev)
        self.status = torch.empty((nj, 4), dtype=torch.int32, device=dev)
        self.work_bytes = int(lib.fsg_em1d_work_bytes(nj, self.nblocks))
        self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.fsg_em1d_fit(_p(x), x.numel(), nj, self.jobs.ctypes.data_as(C.c_void_p), self.tol.ctypes.data_as(C.c_void_p),
                                    _p(self.params), _p(self.lb), _p(self.status), _p(self.work), self.work_bytes, _stream(x)),
                   "fsg_em1d_fit")
        self.slot = {job: pos for pos, job in enumerate(self.order)}  # batch index -> row of the tables

    def results(self):
        """Host copies in batch order: params (nj, 3, 16), lower bounds, status (n_iter, converged, done, 0)."""
        inv = [self.slot[j] for j in range(len(self.order))]
        return self.params.cpu().numpy()[inv], self.lb.cpu().numpy()[inv], self.status.cpu().numpy()[inv]

    def assign(self, pidx, wins):
        """wins: [(batch index, zero-filled uint8 volume, base value)]."""
        lib = _lib.load()
        rows, blk = [], 0
        for job, vol, base in wins:
            r = self.slot[job]
            rows.append([r, vol.data_ptr(), int(base), blk])
            blk += int(self.jobs[r, 4])
        tab = np.array(rows, np.int64).reshape(-1, 4)
        _lib.check(lib.fsg_seed_assign(_p(self.x), self.x.numel(), _p(pidx), len(self.order), self.jobs.ctypes.data_as(C.c_void_p),
                                       len(rows), tab.ctypes.data_as(C.c_void_p), _p(self.params), _p(self.work), self.work_bytes,
                                       _stream(self.x)), "fsg_seed_assign")
        torch.cuda.current_stream(self.x.device).synchronize()  # the host tables above are read by copies on the stream


def fit_gmm1d(x, k=None, *, weights_init=None, means_init=None, vars_init=None, tol=1e-3, max_iter=100, n_init=N_INIT, key=0):
    """Fit a k-component 1-D Gaussian mixture to the float32 device vector `x` by EM.

    With `weights_init`, `means_init` and `vars_init`: exactly one run from these parameters (k is their length).  Otherwise
    `n_init` k-means++ initialisations under `key`, the fit of the highest lower bound returned.  `tol=0` runs exactly `max_iter`
    iterations.  -> dict(weights, means, variances (float64 numpy, initialisation order), lower_bound, n_iter, converged)."""
    _need_gpu(x)
    x = x.contiguous().reshape(-1)
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, got {x.dtype}")
    lib = _lib.load()
    batch = _Batch(lib)
    given = [a is not None for a in (weights_init, means_init, vars_init)]
    if all(given):
        w, mu, var = (np.asarray(a, np.float64).reshape(-1) for a in (weights_init, means_init, vars_init))
        if not (w.size == mu.size == var.size) or (k is not None and k != w.size):
            raise ValueError("weights_init, means_init and vars_init must have one length (k)")
        batch.add(0, x.numel(), w.size, max_iter, 0, tol, w, mu, var)
    elif any(given):
        raise ValueError("give all of weights_init, means_init, vars_init or none of them")
    else:
        if k is None:
            raise ValueError("k is needed when no initial parameters are given")
        sample = x[torch.from_numpy(subsample_index(x.numel())).to(x.device)].cpu().numpy() if x.numel() else np.zeros(0)
        for init in range(int(n_init)):
            batch.add(0, x.numel(), k, max_iter, 1, tol, mu=kmeanspp_means(sample, k, key, 0, init) if x.numel() else None)
    params, lb, status = _Fit(x, batch).results()
    best = int(np.argmax(lb))  # first of equals, as a strict "better than" scan
    kk = batch.rows[best][2]
    return dict(weights=params[best, 0, :kk].copy(), means=params[best, 1, :kk].copy(), variances=params[best, 2, :kk].copy(),
                lower_bound=float(lb[best]), n_iter=int(status[best, 0]), converged=bool(status[best, 1]))


def assign_labels(x, weights, means, variances) -> torch.Tensor:
    """uint8 device vector: for every sample of `x` the component of the largest weighted log-density (ties -> lowest),
    numbered by ascending mean -- the assignment kernel of `generate_seeds` on given parameters."""
    _need_gpu(x)
    x = x.contiguous().reshape(-1)
    w, mu, var = (np.asarray(a, np.float64).reshape(-1) for a in (weights, means, variances))
    batch = _Batch(_lib.load())
    job = batch.add(0, x.numel(), w.size, 1, 2, 0.0, w, mu, var)
    fit = _Fit(x, batch)
    out = torch.zeros(x.numel(), dtype=torch.uint8, device=x.device)
    fit.assign(torch.arange(x.numel(), dtype=torch.int32, device=x.device), [(job, out, 0)])
    return out


def generate_seeds(image, segmentation, max_subclasses=10, annotation="feta", key=0, *, n_init=N_INIT, tol=1e-3, max_iter=100,
                   return_fits=False, _reverse_jobs=False):
    """Seed volumes of one subject: `{n_sub: {mlabel: uint8 device tensor}}` for n_sub = 1..max_subclasses, mlabel = 1..4 --
    what `SeedBank` and `MemorySynthDataset` take.  Volume (n_sub, m) is `10 * m + c` on the voxels of meta-label m (c < n_sub
    the subclass, numbered by ascending mean intensity) and 0 elsewhere.

    `return_fits`: also return `{(m, n_sub): dict(weights, means, variances, lower_bound, n_iter, converged, init)}` of the
    winning fits (components in ascending-mean order).  `_reverse_jobs` submits the job batch in reversed order (the results do
    not depend on it; tests hold the kernels to that)."""
    max_subclasses = int(max_subclasses)
    if not 1 <= max_subclasses <= KMAX:
        raise ValueError(f"max_subclasses must be in 1..{KMAX}")
    meta, counts, px, pidx = meta_pack(image, segmentation, annotation)
    dev = px.device
    lib = _lib.load()
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    # one gather + one copy: the k-means++ subsamples of the four meta-labels
    sidx = [subsample_index(counts[m]) + offs[m] for m in range(4)]
    flat = np.concatenate(sidx) if sum(len(s) for s in sidx) else np.zeros(0, np.int64)
    host = px[torch.from_numpy(flat).to(dev)].cpu().numpy() if flat.size else np.zeros(0, np.float32)
    cuts = np.cumsum([0] + [len(s) for s in sidx])
    samples = [host[cuts[m]: cuts[m + 1]] for m in range(4)]

    batch = _Batch(lib)
    ident, ones = {}, {}
    for m in range(1, 5):
        n = counts[m - 1]
        ones[m] = batch.add(offs[m - 1], n, 1, 1, 2, 0.0)
        for k in range(2, max_subclasses + 1):
            if n == 0:
                continue
            for init in range(int(n_init)):
                ident[(m, k, init)] = batch.add(offs[m - 1], n, k, max_iter, 1, tol, mu=kmeanspp_means(samples[m - 1], k, key, m, init))
    order = list(range(len(batch.rows)))
    fit = _Fit(px, batch, order[::-1] if _reverse_jobs else order)
    params, lb, status = fit.results()

    seeds = {k: {m: torch.zeros(meta.shape, dtype=torch.uint8, device=dev) for m in range(1, 5)} for k in range(1, max_subclasses + 1)}
    wins, fits = [], {}
    for m in range(1, 5):
        if counts[m - 1] == 0:
            continue
        wins.append((ones[m], seeds[1][m], 10 * m))
        for k in range(2, max_subclasses + 1):
            cand = [ident[(m, k, i)] for i in range(int(n_init))]
            best = cand[int(np.argmax(lb[cand]))]
            wins.append((best, seeds[k][m], 10 * m))
            srt = np.argsort(params[best, 1, :k], kind="stable")
            fits[(m, k)] = dict(weights=params[best, 0, :k][srt], means=params[best, 1, :k][srt], variances=params[best, 2, :k][srt],
                                lower_bound=float(lb[best]), n_iter=int(status[best, 0]), converged=bool(status[best, 1]),
                                init=cand.index(best))
    if wins:
        fit.assign(pidx, wins)
    return (seeds, fits) if return_fits else seeds


def subject_key(base_seed, index: int) -> int:
    """Key of subject `index` of a dataset: from `base_seed` and the index, 0 without a base seed."""
    if base_seed is None:
        return 0
    from . import sharding

    return sharding.sample_key(int(base_seed), int(index))


# ----------------------------------------------------------------------------------------------------------------------
# files and the command line
# ----------------------------------------------------------------------------------------------------------------------
def seed_file(out_path, subject: str, like, n_sub: int, mlabel: int, session: str = "") -> Path:
    """Path of seed volume (n_sub, mlabel) in the reference's tree: subclasses_{n}/{sub}/[ses/]anat/{dseg stem}_mlabel_{m}.nii.gz."""
    stem = Path(like).name
    stem = stem[: -len(".nii.gz")] if stem.endswith(".nii.gz") else Path(stem).stem
    folder = Path(out_path) / f"subclasses_{n_sub}" / subject
    if session:
        folder = folder / session
    return folder / "anat" / f"{stem}_mlabel_{mlabel}.nii.gz"


def write_seeds(seeds, out_path, subject: str, like, session: str = ""):
    """Write `generate_seeds` output as int8 NIfTI-1 files carrying the affine of the dseg file `like`, laid out as the reference
    lays them out.  The volumes must be in the file's own voxel orientation.  -> list of written paths."""
    from .utils.image_reading import read_nifti, write_nifti

    _arr, affine, _pix = read_nifti(like)
    written = []
    for n_sub, per_label in seeds.items():
        for mlabel, vol in per_label.items():
            path = seed_file(out_path, subject, like, n_sub, mlabel, session)
            path.parent.mkdir(parents=True, exist_ok=True)
            arr = vol.cpu().numpy() if torch.is_tensor(vol) else np.asarray(vol)
            write_nifti(path, arr.astype(np.int8), affine)
            written.append(path)
    return written


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="python -m fetalsyngen_amd.seedgen", description="Generate seeds for FetalSynthGen",
        epilog="Example: python -m fetalsyngen_amd.seedgen --bids_path /path/to/bids --out_path /path/to/out "
               "--max_subclasses 6 --annotation feta")
    ap.add_argument("--bids_path", type=str, required=True,
                    help="Path to BIDS folder with the segmentations and images for seeds generation")
    ap.add_argument("--out_path", type=str, required=True, help="Path to save the seeds")
    ap.add_argument("--max_subclasses", type=int, default=10,
                    help="How many subclasses to simulate for each tissue type (meta-label)")
    ap.add_argument("--annotation", type=str, required=True, choices=["feta", "dhcp"],
                    help="Annotation type. Should be either 'feta' or 'dhcp'")
    ap.add_argument("--key", type=int, default=0, help="Base key of the k-means++ draws (subject i uses a key derived from it)")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils.image_reading import read_nifti

    bids, out = Path(args.bids_path).absolute(), Path(args.out_path).absolute()
    subjects = sorted(bids.glob("sub-*"))
    print(f"Found {len(subjects)} subjects in {bids}")
    for i, sub in enumerate(subjects):
        img_path = sorted(sub.glob("**/anat/*_T2w.nii.gz"))[0]
        seg_path = sorted(sub.glob("**/anat/*_dseg.nii.gz"))[0]
        image = torch.from_numpy(read_nifti(img_path)[0].astype(np.float32)).to(args.device)
        seg = torch.from_numpy(read_nifti(seg_path)[0].astype(np.float32)).to(args.device)
        seeds = generate_seeds(image, seg, args.max_subclasses, args.annotation, key=subject_key(args.key, i))
        session = seg_path.parent.parent.name if seg_path.parent.parent != sub else ""
        write_seeds(seeds, out, sub.name, like=seg_path, session=session)
        print(f"{sub.name}: {4 * args.max_subclasses} seed volumes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
