"""Generator orchestration: mirror of `fetalsyngen.generator.model.FetalSynthGen`
(reference model.py:27-276).

Same constructor keywords, attributes (`shape, resolution, intensity_generator, spatial_deform,
resampled, biasfield, gamma, noise, artifacts, device`), methods and return tuples, same
`synth_params` schema, same stage order and the same consumption order of the numpy / torch global
generators.  `sample()` first collects every stage's random plan on the host, uploads all small
arrays in one copy, then runs the fused kernel sequence

    gmm -> coords min/max -> warp(+gamma+bias, labels) -> blur x,y,z -> resample+noise
        -> zoom min/max -> zoom+normalise

`generate()` / `augment()` remain individually callable (stage by stage, un-fused).
The optional SR-artifact stages (`blur_cortex`, `struct_noise`, `simulate_motion`, `boundaries`; mirrors in
`fetalsyngen_amd.generator.augmentation.artifacts`) are applied after `resize_back` in the reference's order
(model.py:207-219); any callable with the reference's artifact signature is accepted.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import Iterable

import numpy as np
import torch

from .. import kernels as K
from .. import rng as _rng
from .. import tables as T
from .. import _lib
from ..identity import IdentityCache
from ..utils.generation import make_affine_matrix
from .augmentation.synthseg import BiasPlan, NoisePlan, RandBiasField, RandGamma, RandNoise, RandResample, ResamplePlan
from .deformation.affine_nonrigid import DeformPlan, SpatialDeformation
from .intensity.rand_gmm import GMMPlan, ImageFromSeeds


# [+inf x4 | -inf x4] as the order-preserving int32 keys of fsg_minmax_init (csrc/fsg_common.h: fsg_f2key)
_MM8_INIT = np.array([0x7F800000] * 4 + [-2139095041] * 4, dtype=np.int32)
_MM8_INIT.setflags(write=False)
# K9's min / max keys sharded over 64 slots, each {key(+inf), key(-inf), 0...}:
# the min/max pass ends every workgroup with two atomics nobody waits for (csrc/fsg_zoom.hip: zoom_mm_update)
MM_NSLOTS = 64
_MM_SLOTS_INIT = np.zeros((MM_NSLOTS, _lib.MM_SLOT_STRIDE), dtype=np.int32)
_MM_SLOTS_INIT[:, 0], _MM_SLOTS_INIT[:, 1] = 0x7F800000, -2139095041
_MM_SLOTS_INIT.setflags(write=False)
_SEEN_ONCE, _NO_TWIN = object(), object()  # what `_twins` holds for a label volume that has no uint8 twin


def _label_bricks_bytes(vol):
    """Bytes of the brick table of the device label volume `vol` (one per 8x8x8 brick), 0 where the warp could not use one."""
    shape = vol.shape
    if vol.device.type != "cuda" or len(shape) != 3 or not _lib.load().fsg_label_bricks_usable(*[int(n) for n in shape]):
        return 0
    return ((shape[0] + 7) // 8) * ((shape[1] + 7) // 8) * ((shape[2] + 7) // 8)


def _detach_label_bricks(ptr):
    _lib.load().fsg_label_bricks_detach(ptr)


def _attach_label_bricks(twin):
    """Build the brick table of the uint8 label volume `twin` (csrc/fsg_label_bricks.hip: which 8x8x8 bricks hold one label)
    and attach it, so that the fused warp drops the label gathers of those bricks.  The table lives as long as the twin (it
    hangs on the tensor object) and is detached when the twin dies -- eviction, `invalidate_label_twins`, a new `_version`
    and the death of the caller's volume all end there, before the memory can be reused.  Returns the table's bytes."""
    nbytes = _label_bricks_bytes(twin) if twin.is_contiguous() else 0
    if nbytes == 0:
        return 0
    lib = _lib.load()
    table = torch.empty(nbytes, dtype=torch.uint8, device=twin.device)
    stream = torch.cuda.current_stream(twin.device)
    _lib.check(lib.fsg_label_bricks_u8(twin.data_ptr(), *[int(n) for n in twin.shape], table.data_ptr(), stream.cuda_stream),
               "fsg_label_bricks_u8")
    stream.synchronize()  # once per subject: the table is complete before a sample on any stream reads it
    if lib.fsg_label_bricks_attach(twin.data_ptr(), *[int(n) for n in twin.shape], table.data_ptr()) != 0:
        return 0  # registry full: this volume's labels are gathered as before
    if getattr(twin, "_fsg_bricks", None) is None:
        weakref.finalize(twin, _detach_label_bricks, twin.data_ptr())
    twin._fsg_bricks = table
    return nbytes


class _Ctx:
    """One prepared sample: its plans, arena offsets and (after _resolve) device views."""


class StageTrace:
    """HIP events behind every launch of ONE sample (fsg_sample_plan::trace_events): per-launch times on the launch stream,
    measured where the launches happen.  Measurement only: each record is a barrier packet (~5 us of bubble)."""

    CAP = 16

    def __init__(self):
        lib = _lib.load()
        self.events = (C.c_void_p * self.CAP)(*[lib.fsg_event_create() for _ in range(self.CAP)])
        self.ids = np.zeros(self.CAP + 1, dtype=np.int32)
        self.meta = None

    def slots(self):
        return C.addressof(self.events), self.ids.ctypes.data, self.CAP

    def elapsed_us(self):
        """[(stage name, microseconds between the previous event and this launch's event)]; synchronises."""
        lib, ms, out = _lib.load(), C.c_float(), []
        n = int(self.ids[self.CAP])
        for k in range(1, n):
            _lib.check(lib.fsg_event_elapsed_ms(self.events[k - 1], self.events[k], C.byref(ms)), "fsg_event_elapsed_ms")
            out.append((_lib.STAGE_NAMES[int(self.ids[k])], ms.value * 1e3))
        return out

    def close(self):
        lib = _lib.load()
        for e in self.events:
            if e:
                lib.fsg_event_destroy(e)
        self.events = ()


class FetalSynthGen:
    def __init__(
        self,
        shape: Iterable[int],
        resolution: Iterable[float],
        device: str,
        intensity_generator: ImageFromSeeds,
        spatial_deform: SpatialDeformation,
        resampler: RandResample,
        bias_field: RandBiasField,
        noise: RandNoise,
        gamma: RandGamma,
        blur_cortex=None,
        struct_noise=None,
        simulate_motion=None,
        boundaries=None,
        rng: str | None = None,
    ):
        if not str(device).startswith("cuda"):
            raise RuntimeError(
                f"fetalsyngen_amd.FetalSynthGen runs on an MI355X only (device='cuda:N'), got device={device!r}; "
                "there is no CPU fallback"
            )
        self.shape = shape
        self.resolution = resolution
        self.intensity_generator = intensity_generator
        self.spatial_deform = spatial_deform
        self.resampled = resampler
        self.biasfield = bias_field
        self.gamma = gamma
        self.noise = noise
        self.artifacts = {
            "blur_cortex": blur_cortex,
            "struct_noise": struct_noise,
            "simulate_motion": simulate_motion,
            "boundaries": boundaries,
        }
        self.device = device
        self.rng = rng  # None: module default (fetalsyngen_amd.rng.get_mode())
        self.native_pipeline = True  # one native call per sample when the inputs allow it
        self.blur_events = None      # set to a list: (begin, end, [(axis, radius)], low-res shape) per sample, HIP events recorded
                                     # around the blur (+ down-sampling, when fused) launches inside the native call
        self.blur_events_every = 1   # ... of every k-th sample only (an event record is a barrier packet: ~5.5 us of bubble)
        self._blur_tick = 0
        self.stage_traces = None     # set to a list: every fused sample appends a StageTrace (per-launch HIP events)
        self._ws = {}

    # Everything below lives and dies with ONE process: raw host addresses (`_flat`: ivp / fvp / tbp are `ndarray.ctypes.data`
    # integers), device tensors (`_ws`, `_twins`), HIP events and streams, caches keyed by `id()` of tensors of
    # this process.  None of it is configuration, all of it is rebuilt on first use -- so a pickled generator (the reference's
    # DataLoader pattern: `num_workers=2, multiprocessing_context="spawn"`, fetalsyngen/test_dl.py:17-24, docs/datasets.md:4-6)
    # carries none of it into the worker.
    _PROCESS_LOCAL = ("_ws", "_flat", "_twins", "_rs_dt", "_batch_streams", "blur_events", "_blur_tick", "_keyed",
                      "stage_traces", "_priors")

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._PROCESS_LOCAL}

    def __setstate__(self, state):
        self.__dict__.update({k: v for k, v in state.items() if k not in self._PROCESS_LOCAL})
        self.blur_events, self._blur_tick, self._ws, self.stage_traces = None, 0, {}, None

    def prewarm(self, shape=None) -> int:
        """Build and upload every per-axis table this configuration can ask for (the low-res size of
        RandResample takes at most shape*(1 - min/max resolution) distinct values per axis; the coarse
        deformation / bias grids a handful).  Optional: tables are otherwise cached on first use.
        Returns the number of tables now resident."""
        shape = tuple(int(v) for v in (shape or self.shape))
        res = np.array(self.resolution, dtype=np.float64)
        rs, sd, bf = self.resampled, self.spatial_deform, self.biasfield
        n = 0
        for a in range(3):
            size = shape[a]
            lo = int(size * res[a] / max(rs.max_resolution, res[a]))
            for m in range(max(lo - 1, 1), size + 1):
                K._device_table(T.axis_table(_lib.KT.RESAMPLE, m, size), self.device)
                K._device_table(T.axis_table(_lib.KT.BACK, m, size), self.device)
                n += 2
            for kind, lo_s, hi_s in ((_lib.KT.FIELD, sd.nonlin_scale_min, sd.nonlin_scale_max), (_lib.KT.BIAS, bf.scale_min, bf.scale_max)):
                for s_ in range(max(int(np.floor(lo_s * size)) - 1, 1), int(np.ceil(hi_s * size)) + 2):
                    K._device_table(T.axis_table(kind, s_, size), self.device)
                    n += 1
        return n

    def reserve(self, shape=None, samples_in_flight: int = 8) -> int:
        """Pre-size the device memory pool for `samples_in_flight` samples whose outputs are alive at once (the host runs
        several samples ahead of the GPU, and a consumer may hold a few): allocates and releases that many image / label
        volumes and parameter arenas through torch's caching allocator, so that the first samples do not pay for
        hipMalloc calls (0.2-1 ms each) in the middle of the launch stream.  Returns the bytes reserved."""
        shape = tuple(int(v) for v in (shape or self.shape))
        dev = torch.device(self.device)
        hold = []
        for _ in range(int(samples_in_flight)):
            hold.append(torch.empty(shape, dtype=torch.float32, device=dev))   # image
            hold.append(torch.empty(shape, dtype=torch.float32, device=dev))   # labels
            hold.append(torch.empty(1 << 16, dtype=torch.uint8, device=dev))   # parameter arena
        total = sum(t.numel() * t.element_size() for t in hold)
        del hold
        return total

    # ---- native fused path -------------------------------------------------------------------------
    def _workspace(self, shape, need_rows):
        """Per (shape, stream) scratch volumes, reused by consecutive samples on that stream.

        Eviction (a fifth key appears) and growth of the row workspace drop tensors that kernels already
        enqueued may still read.  That is safe because every block here is allocated while its key's stream is
        the current one: the caching allocator hands a freed block only to later requests on the block's OWN
        allocation stream, which are ordered behind those kernels (tests/test_hip_parity.py::
        test_workspace_eviction_across_streams)."""
        dev = torch.device(self.device)
        key = (shape, dev.index, K._stream(dev).value)
        ws = self._ws.get(key)
        n = int(np.prod(shape))
        if ws is None:
            ws = {"ws0": torch.empty(n, dtype=torch.float32, device=dev),
                  "ws1": torch.empty(n, dtype=torch.float32, device=dev),
                  "low": torch.empty(n, dtype=torch.float32, device=dev),
                  "mm8": torch.empty(8, dtype=torch.int32, device=dev), "rows": None, "stride": 0}
            if len(self._ws) >= 4:
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        if need_rows > ws["stride"]:
            ws["stride"] = (max(need_rows, 64) + 3) // 4 * 4
            ws["rows"] = torch.empty(shape[0] * shape[1] * ws["stride"], dtype=torch.float32, device=dev)
        return ws

    label_twin_budget_bytes = 1 << 30  # HBM the uint8 twins of caller-owned label volumes may take (64 at 256^3)

    def _cache(self, name):
        """The generator's IdentityCache `name` (`_twins`, `_priors`): process-local, made on first use."""
        cache = self.__dict__.get(name)
        return cache if cache is not None else self.__dict__.setdefault(name, IdentityCache())

    def register_label_twin(self, seg, twin):
        """Hand over a uint8 copy of the float32 label volume `seg` (same values) that the caller already holds -- the
        datasets do, for every subject they cache -- so that no check and no second copy is made here."""
        if twin is None or twin.dtype != torch.uint8 or twin.shape != seg.shape or twin.device != seg.device:
            raise ValueError("label twin must be a uint8 tensor of the segmentation's shape on its device")
        twins = self._cache("_twins")
        twins.drop(seg)
        twins.put(seg, twin, twin.numel() + _attach_label_bricks(twin), seg._version)

    def invalidate_label_twins(self):
        """Forget every cached uint8 label twin.  The cache notices a new tensor object and an in-place torch write
        (`_version`); it cannot notice a label volume rewritten through its raw pointer (another HIP library, the `fsg_*`
        entry points themselves) -- call this after such a write."""
        for cache in (self._cache("_twins"), self._cache("_priors"), self._flat_buffers()["validated"]):
            cache.clear()
        for kc in (self.__dict__.get("_keyed") or {}).values():  # keyed mode: the subjects' pointer blocks and code volumes
            kc.forget_subjects()

    def _label_twin(self, seg):
        """uint8 copy of a float32 label volume whose values are integers in 0..255 (dseg volumes always are): the fused warp
        then gathers 1 B/voxel instead of 4, the output stays float32.  Cached per tensor OBJECT and in-place version
        (identity.IdentityCache: nothing keeps a caller's volume alive).  A volume is converted on its SECOND sighting: a caller who passes a fresh segmentation on every call never pays the
        synchronising integer check and the extra passes, a caller who re-uses volumes pays them once.  Twins take at most
        `label_twin_budget_bytes` (oldest dropped first).  None: no twin (yet), the warp reads the float32 volume."""
        twins = self._cache("_twins")
        twin = twins.get(seg, seg._version)
        if twin is None:
            twins.put(seg, _SEEN_ONCE, 0, seg._version)
            return None
        if twin is _SEEN_ONCE:  # second sighting: check and convert (synchronises once per volume)
            twin, nbytes = _NO_TWIN, 0
            ok = bool(torch.equal(seg.round(), seg)) and float(seg.min()) >= 0 and float(seg.max()) <= 255
            if ok and twins.make_room(seg.numel() + _label_bricks_bytes(seg), self.label_twin_budget_bytes):
                twin = seg.to(torch.uint8)
                nbytes = seg.numel() + _attach_label_bricks(twin)
            twins.put(seg, twin, nbytes, seg._version)  # (in the place of its first sighting)
        return None if twin is _NO_TWIN else twin

    # ---- per-subject constant of a real image: its intensity prior --------------------------------------------------------
    def register_image_prior(self, image, prior):
        """Hand over the intensity prior of the device image `image` (what `_intensity_prior(image)` returns) that the caller
        already holds and accounts for -- the datasets do, per cached subject -- so that keyed samples do not recompute it.
        It holds no bytes here: it is not counted and never evicted."""
        if prior.dtype != torch.float32 or prior.shape != image.shape or prior.device != image.device or not prior.is_contiguous():
            raise ValueError("image prior must be a contiguous float32 tensor of the image's shape on its device")
        priors = self._cache("_priors")
        priors.drop(image)
        priors.put(image, prior, 0, image._version)

    def _image_prior(self, image):
        """`_intensity_prior(image)` -- (x - min) / (max - min) * 255, a constant of the subject -- computed once per image
        tensor OBJECT with the same two kernels, so the very bits the stage-wise path produces on every sample.  Cached with
        the tensor's in-place version, like the label twins.  The priors have a byte count of their own, held to the size
        `label_twin_budget_bytes` also gives the twins (so the two caches together may take twice that; oldest prior dropped
        first; a prior that does not fit is computed per sample)."""
        priors = self._cache("_priors")
        prior = priors.get(image, image._version)
        if prior is None:
            prior = self._intensity_prior(image)
            nbytes = prior.numel() * 4
            if priors.make_room(nbytes, self.label_twin_budget_bytes):
                priors.put(image, prior, nbytes, image._version)
        return prior

    def _native_ok(self, c, labels_u8: bool = False) -> bool:
        """labels_u8: the caller wants uint8 labels -- the fused path then writes them itself and a caller-supplied uint8
        copy of the segmentation (the stage-by-stage path's way to uint8 labels) does not keep the sample off it."""
        return (self.native_pipeline and c.label_parts is not None and c.image is None and not c.has_art
                and (c.segmentation_u8 is None or labels_u8))

    def _native_operands(self, c):
        """Shape / dtype / device checks of everything the C side only sees as pointers (a mismatched volume would make
        the fused kernels gather outside a smaller buffer); sets `c.seg`, the segmentation as a contiguous float32 device
        tensor.  A caller's segmentation that already is one is used as it is, and it and the seed volumes are checked once
        per tensor OBJECT (id + weak reference: a new tensor at a recycled address is a new object) together with the sample
        shape -- per tensor, not per combination: the seed volumes of a subject combine in up to 6^4 ways.  Any other
        segmentation (host, other dtype, not contiguous) is converted, and the copy is checked, on every call."""
        shape = c.shape = tuple(int(v) for v in c.shape)
        seg = c.segmentation
        val = self._flat_buffers()["validated"]
        known = torch.is_tensor(seg) and seg.is_cuda and seg.dtype == torch.float32 and seg.is_contiguous()
        checked = val.get
        for t_ in (seg, *c.label_parts) if known else ():
            if checked(t_) != shape:
                known = False
                break
        if not known:
            dev = torch.device(self.device)
            seg = seg.to(dev)
            if seg.dtype != torch.float32:
                seg = seg.float()
            seg = seg.contiguous()
            if tuple(seg.shape) != shape:
                raise ValueError(f"segmentation shape {tuple(seg.shape)} differs from the seed volumes' shape {shape}")
            if not 1 <= len(c.label_parts) <= 4:
                raise ValueError(f"{len(c.label_parts)} seed label volumes: the fused path takes 1..4")
            for q, part in enumerate(c.label_parts):
                off_dev = part.device.type != dev.type or (dev.index is not None and part.device.index != dev.index)
                if tuple(part.shape) != shape or part.dtype != torch.uint8 or not part.is_contiguous() or off_dev:
                    raise ValueError(
                        f"seed label volume {q}: expected a contiguous uint8 tensor of shape {shape} on {dev}, got "
                        f"{part.dtype} {tuple(part.shape)} on {part.device} (contiguous={part.is_contiguous()})")
            if seg is c.segmentation:
                for t_ in (seg, *c.label_parts):
                    val.put(t_, shape)
        c.seg = seg
        if not 1 <= c.gm_off[2] <= 256:
            raise ValueError(f"mus / sigmas tables of {c.gm_off[2]} entries (need 1..256)")

    def _twin_of(self, c):
        """The cached uint8 copy of the segmentation (_label_twin), only for a caller-owned device tensor (stable identity):
        a converted copy would be a new cache entry per call."""
        return self._label_twin(c.seg) if c.seg is c.segmentation else None

    def _rows_needed(self, c) -> int:
        """Row workspace of the fused head: three components of the coarse deformation field and the bias field per row."""
        if not c.dplan.active:
            return 0
        f2 = int(c.sb.pending[1][2]) if c.sb.pending is not None else 0
        b2 = int(c.bplan.grid.shape[2]) if c.bplan.active else 0
        return 3 * f2 + b2

    # ---- the per-sample plan -------------------------------------------------------------------------------------------
    # fsg_sample_plan as two flat arrays (FSG_PLAN_I_* / FSG_PLAN_F_* in include/fsg_hip.h) handed over with ONE native call
    # (fsg_sample_pack_run; fsg_sample_plan_pack for a batch): filling the ctypes struct field by field cost 41 us per sample,
    # the spec / view objects 28 us (profiles/r02_c_host_phases.txt).
    def _flat_buffers(self):
        fb = self.__dict__.get("_flat")
        if fb is None:
            iv = np.zeros(_lib.PLAN_I.COUNT, dtype=np.int64)
            fv = np.zeros(_lib.PLAN_F.COUNT, dtype=np.float64)
            tb = np.zeros((3, _lib.PLAN_TAPS_STRIDE), dtype=np.float32)
            centre = (np.array(self.spatial_deform.size) - 1) / 2
            fb = self._flat = dict(iv=iv, fv=fv, tb=tb, ivp=iv.ctypes.data, fvp=fv.ctypes.data, tbp=tb.ctypes.data,
                                   centre=np.asarray(centre, dtype=np.float32).tolist(), validated=IdentityCache())
        return fb

    def _flat_plan(self, c, scale01, out, seg_out, ws, twin=None):
        """The two flat arrays of prepared sample `c` (arena uploaded, _native_operands done, no _resolve needed) in the
        generator's `_flat` buffers, which hold one plan at a time.  `seg_out`: where the deformed labels go, uint8 only
        with `twin`, the uint8 copy of the segmentation.  Returns False when the sample is outside the fused path's domain
        (blur radius beyond the tap capacity, uint8 labels without a twin)."""
        I, F = _lib.PLAN_I, _lib.PLAN_F
        fb = self._flat_buffers()
        iv, fv, tb = [0] * I.COUNT, [0.0] * F.COUNT, fb["tb"]
        base = c.arena.base
        shape = c.shape
        iv[I.SHAPE:I.SHAPE + 3] = shape
        for q, part in enumerate(c.label_parts):
            iv[I.LABEL_PARTS + q] = part.data_ptr()
        iv[I.MUS], iv[I.SIGMAS], iv[I.NTAB] = base + c.gm_off[0], base + c.gm_off[1], c.gm_off[2]
        f = c.gmm_plan.field
        if f.host is not None:
            z = f.device_tensor(torch.device(self.device))
            c.keep.append(z)
            iv[I.GMM_NOISE] = z.data_ptr()
        else:
            iv[I.GMM_SEED], iv[I.GMM_STREAM] = f.seed, f.stream_id
        dplan = c.dplan
        if dplan.active:
            iv[I.DEFORM_ACTIVE] = 1
            iv[I.FLIP] = int(bool(dplan.flip))
            a_np, c2_np = dplan.A_np, dplan.c2_np  # left by _draw_all_fast (no torch round trip)
            fv[F.A:F.A + 9] = a_np.ravel().tolist() if a_np is not None else dplan.A.reshape(-1).tolist()
            fv[F.CENTRE:F.CENTRE + 3] = fb["centre"]
            fv[F.C2:F.C2 + 3] = c2_np.astype(np.float32).tolist() if c2_np is not None else dplan.c2.to(torch.float32).tolist()
            if c.sb.pending is not None:
                off, fshape = c.sb.pending
                iv[I.FIELD_DIMS:I.FIELD_DIMS + 3] = fshape[:3]
                iv[I.FIELD] = base + off
                iv[I.FIELD_TABS:I.FIELD_TABS + 3] = c.sb.tabs.ptrs_i
            if twin is not None:
                iv[I.SEG_IN_U8] = twin.data_ptr()
            iv[I.SEG_IN] = c.seg.data_ptr()
            if seg_out.dtype == torch.uint8:  # uint8 labels out (device-resident hand-over): needs the uint8 source
                if twin is None:
                    return False
                iv[I.SEG_OUT_U8] = seg_out.data_ptr()
            else:
                iv[I.SEG_OUT] = seg_out.data_ptr()
        if c.g is not None:
            fv[F.GAMMA] = float(np.float32(float(c.g)))
        if c.bplan.active:
            iv[I.BIAS_DIMS:I.BIAS_DIMS + 3] = c.bplan.grid.shape
            iv[I.BIAS] = base + c.bias_off
            iv[I.BIAS_TABS:I.BIAS_TABS + 3] = c.bias_tabs.ptrs_i
        rplan, nplan = c.rplan, c.nplan
        if rplan.active:
            iv[I.RESAMPLE_ACTIVE] = 1
            iv[I.LOW_SHAPE:I.LOW_SHAPE + 3] = rplan.new_size
            iv[I.RS_TABS:I.RS_TABS + 3] = c.rs_tabs.ptrs_i
            iv[I.BACK_TABS:I.BACK_TABS + 3] = c.back_tabs.ptrs_i
            for a_ in range(3):
                if rplan.stds[a_] > 0:
                    taps = T.gaussian_taps(float(rplan.stds[a_]))
                    n = len(taps)
                    if n > 129:
                        return False
                    iv[I.BLUR_NTAPS + a_] = n
                    tb[a_, :n] = taps
        if nplan.active:
            nf = nplan.field
            fv[F.NOISE_STD] = nplan.std32
            if nf.host is not None:
                zn = nf.device_tensor(torch.device(self.device))
                c.keep.append(zn)
                iv[I.NOISE_MODE], iv[I.NOISE] = 1, zn.data_ptr()
            else:
                iv[I.NOISE_MODE], iv[I.NOISE_SEED], iv[I.NOISE_STREAM] = 2, nf.seed, nf.stream_id
        iv[I.SCALE01] = int(bool(scale01))
        iv[I.WS0], iv[I.WS1], iv[I.WS_LOW] = ws["ws0"].data_ptr(), ws["ws1"].data_ptr(), ws["low"].data_ptr()
        if ws["rows"] is not None:
            iv[I.WS_ROWS], iv[I.ROW_STRIDE] = ws["rows"].data_ptr(), ws["stride"]
        iv[I.MM8], iv[I.MM8_PRESET] = base + c.mm_off, 1
        if c.slots_off is not None:
            iv[I.MM_SLOTS], iv[I.MM_NSLOTS] = base + c.slots_off, MM_NSLOTS
        iv[I.OUT] = out.data_ptr()
        fb["iv"][:] = iv
        fb["fv"][:] = fv
        return True

    def _instrument(self, resampling=True):
        """(blur events | None, StageTrace | None) of the sample about to be enqueued.  Events: for every `blur_events_every`-th
        sample that resamples (a caller that cannot know yet destroys those of a sample that did not); trace: for every sample."""
        events = None
        if self.blur_events is not None and resampling:
            self._blur_tick += 1
            if self._blur_tick % self.blur_events_every == 0:
                events = (_lib.load().fsg_event_create(), _lib.load().fsg_event_create())
        return events, (StageTrace() if self.stage_traces is not None else None)

    def _keep_blur_events(self, events, blur_ntaps, low_shape):
        self.blur_events.append((events[0], events[1], [(a_, int(blur_ntaps[a_]) // 2) for a_ in range(3) if blur_ntaps[a_]],
                                 tuple(int(v) for v in low_shape)))

    def _run_native(self, c, scale01, labels_u8=False):
        """Enqueue prepared sample `c` (arena uploaded) with one fsg_sample_pack_run call.  Returns (image, labels), or None
        when the sample is outside the fused kernels' domain (the caller then launches stage by stage).  labels_u8: the
        labels as a uint8 volume (written by the warp itself; without a deformation the cached uint8 copy of the input), or
        as float32 while no uint8 copy is cached (the caller converts them)."""
        self._native_operands(c)
        dev = torch.device(self.device)
        ws = self._workspace(c.shape, self._rows_needed(c))
        out = torch.empty(c.shape, dtype=torch.float32, device=dev)
        twin = self._twin_of(c) if (c.dplan.active or labels_u8) else None
        if labels_u8 and twin is not None:
            seg_out = torch.empty(c.shape, dtype=torch.uint8, device=dev) if c.dplan.active else twin
        else:
            seg_out = torch.empty_like(c.seg) if c.dplan.active else c.seg
        if not self._flat_plan(c, scale01, out, seg_out, ws, twin):
            return None
        I, fb, lib = _lib.PLAN_I, self._flat, _lib.load()
        iv = fb["iv"]
        events, tr = self._instrument(c.rplan.active)
        if events is not None:
            iv[I.EV_BEGIN], iv[I.EV_END] = events
            self._keep_blur_events(events, iv[I.BLUR_NTAPS:I.BLUR_NTAPS + 3].tolist(), c.rplan.new_size)
        if tr is not None:
            tr.meta = {"shape": tuple(c.shape), "low_shape": tuple(c.rplan.new_size) if c.rplan.active else None,
                       "blur_ntaps": iv[I.BLUR_NTAPS:I.BLUR_NTAPS + 3].tolist()}
            iv[I.TRACE_EVENTS], iv[I.TRACE_IDS], iv[I.TRACE_CAP] = tr.slots()
            self.stage_traces.append(tr)
        rc = lib.fsg_sample_pack_run(fb["ivp"], I.COUNT, fb["fvp"], _lib.PLAN_F.COUNT, fb["tbp"], K._stream(dev))
        if rc in (_lib.E_ALIGN, _lib.E_TOOBIG):
            return None
        _lib.check(rc, "fsg_sample_pack_run")
        self._intensity_views(c)
        return out, seg_out

    @staticmethod
    def _params(selected_seeds, seed_intensities, dplan, g, bplan, rplan, nplan, artifacts):
        return {
            "selected_seeds": selected_seeds,
            "seed_intensities": seed_intensities,
            "deform_params": dplan.params,
            "gamma_params": {"gamma": g},
            "bf_params": bplan.params,
            "resample_params": {"spacing": rplan.spacing.tolist() if rplan.active else None},
            "noise_params": {"noise_std": nplan.std32 if nplan.active else None},
            "artifacts": artifacts,
        }

    def _validated_genparams(self, d):
        if not isinstance(d, dict):
            return d
        return {k: self._validated_genparams(v) for k, v in d.items() if v is not None}

    # ---- stage-by-stage API ---------------------------------------------------------------------
    def _intensity_prior(self, image):
        img = image.to(self.device).float().contiguous()
        return K.scale(img, K.reduce_minmax(img), mode=2)  # (x-min)/(max-min)*255, ref :138

    def generate(self, image, segmentation, seeds, genparams: dict = {}):
        with _rng.use(self.rng):
            if seeds is not None:
                seeds, selected_seeds = self.intensity_generator.load_seeds(
                    seeds=seeds, genparams=genparams.get("selected_seeds", {}))
                output, seed_intensities = self.intensity_generator.sample_intensities(
                    seeds=seeds, device=self.device, genparams=genparams.get("seed_intensities", {}))
            else:
                if image is None:
                    raise ValueError(
                        "If no seeds are passed, an image must be loaded to be used as intensity prior!")
                output = self._intensity_prior(image)
                selected_seeds, seed_intensities = {}, {}
            segmentation = segmentation.to(self.device)
            image = image.to(self.device) if image is not None else None
            image, segmentation, output, deform_params = self.spatial_deform.deform(
                image=image, segmentation=segmentation, output=output,
                genparams=genparams.get("deform_params", {}))
        return output, segmentation, image, {
            "selected_seeds": selected_seeds,
            "seed_intensities": seed_intensities,
            "deform_params": deform_params,
        }

    def _apply_artifacts(self, output, segmentation, genparams, key=None):
        """The configured SR-artifact stages in the reference's order.  key (keyed mode): stage `name` runs inside
        `keyed_scope(key, STAGE_STREAMS[name])`, so its host draws depend on nothing but the key and its own inputs."""
        artifacts = {}
        for name, artifact in self.artifacts.items():
            if artifact is not None:
                with _rng.keyed_scope(key, _rng.STAGE_STREAMS[name]) if key is not None else contextlib.nullcontext():
                    output, metadata = artifact(output, segmentation, self.device, genparams.get("artifact_params", {}),
                                                resolution=self.resolution)
                artifacts[name] = metadata
        return output, artifacts

    def _artifact_tail(self, output, segmentation, genparams, scale01, key=None):
        """The configured stages, then -- last, and only with stages: any other sample was scaled before -- the [0,1] scaling."""
        output, artifacts = self._apply_artifacts(output, segmentation, genparams, key)
        if scale01 and artifacts:
            output = output.contiguous()
            output = K.scale(output, K.reduce_minmax(output), mode=1)
        return output, artifacts

    def augment(self, image, segmentation, genparams: dict = {}):
        with _rng.use(self.rng):
            output, gamma_params = self.gamma(image, self.device, genparams=genparams.get("gamma_params", {}))
            output, bf_params = self.biasfield(output, self.device, genparams=genparams.get("bf_params", {}))
            output, factors, resample_params = self.resampled(
                output, np.array(self.resolution), self.device, genparams=genparams.get("resample_params", {}))
            output, noise_params = self.noise(output, self.device, genparams=genparams.get("noise_params", {}))
            output = self.resampled.resize_back(output, factors)
            output, artifacts = self._apply_artifacts(output, segmentation, genparams)
        return output, {
            "gamma_params": gamma_params,
            "bf_params": bf_params,
            "resample_params": resample_params,
            "noise_params": noise_params,
            "artifacts": artifacts,
        }

    # ---- fused path -----------------------------------------------------------------------------
    def sample(self, image, segmentation, seeds, genparams: dict = {}, key: int | None = None):
        """`key`: keyed mode only (`rng="keyed"`), the sample's 64-bit key."""
        return self._pipeline(image, segmentation, seeds, genparams, scale01=False, key=key)

    def _resolution64(self):
        res = self.__dict__.get("_res64")
        if res is None:
            res = self._res64 = np.array(self.resolution)
        return res

    def _draw_plans(self, shape, genparams):
        """Host draws of everything after the intensity plan, in the reference's order:
        deformation, gamma, bias field, resampling, noise.  No device work."""
        dplan = self.spatial_deform.plan(shape, random_shift=True, genparams=genparams.get("deform_params", {}))
        g = self.gamma.plan(genparams.get("gamma_params", {}))
        bplan = self.biasfield.plan(shape, genparams.get("bf_params", {}))
        rplan = self.resampled.plan(shape, self._resolution64(), genparams.get("resample_params", {}))
        low_shape = rplan.new_size if rplan.active else shape
        nplan = self.noise.plan(low_shape, genparams.get("noise_params", {}))
        return dplan, g, bplan, rplan, nplan

    def plan_only(self, shape, genparams: dict = {}, fast: bool | None = None):
        """Every host draw of one seeds-based sample, nothing enqueued (bench.py --dry-plan, host profiling).
        fast=None: the bulk-draw form when there are no genparams (what `_prepare` uses); False: the per-stage plan()s."""
        with _rng.use(self.rng):
            if (fast is None and not genparams) or fast:
                return self._draw_all_fast(tuple(shape))
            m2s = self.intensity_generator.draw_subclusters(genparams.get("selected_seeds", {}))
            gmm_plan = self.intensity_generator.plan_intensities(tuple(shape), genparams.get("seed_intensities", {}))
            return (m2s, gmm_plan) + self._draw_plans(tuple(shape), genparams)

    def _draw_all_fast(self, shape):
        """All host draws of a seeds-based sample WITHOUT genparams, same values and same generator states as
        `draw_subclusters` + `plan_intensities` + `_draw_plans` (tests/test_host_plans.py::test_bulk_draws_equal_per_stage_plans),
        with fewer interpreter round trips: numpy's legacy generator hands out the same doubles whether they are asked for one
        `rand()` at a time or as `random_sample(n)`, and `randint(lo, hi, size=4)` equals four scalar calls, so the draws
        between two gates are fetched in one call (gates still short-circuit: nothing behind a failed gate is drawn);
        `torch.rand(2n)` equals two `torch.rand(n)`.  Scalars are combined as Python floats (the same IEEE doubles as the
        0-d numpy arithmetic of the per-stage code)."""

        ig, sd, bf, rs_, nz, gm = (self.intensity_generator, self.spatial_deform, self.biasfield, self.resampled, self.noise,
                                   self.gamma)
        rs = np.random.random_sample
        # ---- seeds + intensities (rand_gmm.py:81-87, :120-148)
        picks = np.random.randint(ig.min_subclusters, ig.max_subclusters + 1, size=ig.meta_labels).tolist()
        m2s = {m + 1: picks[m] for m in range(ig.meta_labels)}
        nlabels = max(ig.seed_labels) + 1
        u2 = torch.rand(2 * nlabels, dtype=torch.float32).numpy()
        mus = np.float32(25) + np.float32(200) * u2[:nlabels]
        sigmas = np.float32(5) + np.float32(20) * u2[nlabels:]
        if ig.generation_classes != ig.seed_labels:
            if ig._idx is None:
                ig._idx = (np.asarray(ig.generation_classes), np.asarray(ig.seed_labels))
            z = torch.randn(len(ig.seed_labels), dtype=torch.float32).numpy()
            tied = mus[ig._idx[0]] + np.float32(25) * z
            mus[ig._idx[1]] = np.minimum(np.maximum(tied, np.float32(0)), np.float32(225))
        gmm_plan = GMMPlan(torch.from_numpy(mus), torch.from_numpy(sigmas), _rng.normal_field(shape, stream_id=1))
        # ---- deformation (affine_nonrigid.py:140-145, :248-263, :284, :303-318)
        dplan = DeformPlan()
        if rs(1)[0] < sd.prob:
            nl = bool(sd.nonlinear_transform)
            u = rs(13 if nl else 11)  # flip, rot x3, shear x3, scale x3 [, nonlin scale, nonlin std], then the gamma gate
            dplan.active = True
            dplan.flip = bool(u[0] < sd.flip_prb)
            shp, centre32, room64 = sd._shape_constants(tuple(shape)[0:3])
            ul = u.tolist()  # Python floats: the same IEEE doubles, a tenth of the cost of 0-d / 3-element numpy arithmetic
            mr2, mr, ms2, ms, mc2, mc, pi = 2 * sd.max_rotation, sd.max_rotation, 2 * sd.max_shear, sd.max_shear, 2 * sd.max_scaling, sd.max_scaling, np.pi
            rot = np.array([(mr2 * ul[1] - mr) / 180.0 * pi, (mr2 * ul[2] - mr) / 180.0 * pi, (mr2 * ul[3] - mr) / 180.0 * pi])
            shr = np.array([ms2 * ul[4] - ms, ms2 * ul[5] - ms, ms2 * ul[6] - ms])
            scl = np.array([1 + (mc2 * ul[7] - mc), 1 + (mc2 * ul[8] - mc), 1 + (mc2 * ul[9] - mc)])
            dplan.A_np = make_affine_matrix(rot, shr, scl).astype(np.float32)
            dplan.A = torch.from_numpy(dplan.A_np)
            ut = torch.rand(3, dtype=torch.float64).tolist()  # float64 draw, always consumed
            c32, r64 = sd._shape_lists(tuple(shape)[0:3])
            centre = np.array([c32[0] + (2 * (r64[0] * ut[0]) - r64[0]), c32[1] + (2 * (r64[1] * ut[1]) - r64[1]),
                               c32[2] + (2 * (r64[2] * ut[2]) - r64[2])])
            dplan.c2_np = centre
            dplan.c2 = torch.from_numpy(centre)
            nr_params = {}
            if nl:
                scale = sd.nonlin_scale_min + u[10:11] * (sd.nonlin_scale_max - sd.nonlin_scale_min)
                sc = float(scale[0])
                small = [int(round(sc * float(shp[0]))), int(round(sc * float(shp[1]))), int(round(sc * float(shp[2])))]
                std = sd.nonlin_std_max * ul[11]
                dplan.field_small = std * torch.randn([*small, 3], dtype=torch.float32)
                nr_params = {"nonlin_scale": scale, "nonlin_std": std, "size_F_small": small}
            dplan.params = {"affine": {"rotations": rot, "shears": shr, "scalings": scl}, "non_rigid": nr_params,
                            "flip": dplan.flip}
            gate_gamma = u[-1]
        else:
            gate_gamma = rs(1)[0]
        # ---- gamma (synthseg.py:263-268)
        g = np.exp(gm.gamma_std * np.random.randn(1)[0]) if gate_gamma < gm.prob else None
        # ---- bias field (synthseg.py:157-176), then the resampling gate
        bplan = BiasPlan()
        if rs(1)[0] < bf.prob:
            u = rs(3)
            bplan.active = True
            scale = bf.scale_min + u[0:1] * (bf.scale_max - bf.scale_min)
            sc = float(scale[0])
            size = [max(int(round(sc * float(shape[0]))), 1), max(int(round(sc * float(shape[1]))), 1),
                    max(int(round(sc * float(shape[2]))), 1)]
            std = bf.std_min + (bf.std_max - bf.std_min) * u[1:2]
            std32 = np.asarray(std, dtype=np.float32)
            bplan.grid = torch.from_numpy(std32 * torch.randn(size, dtype=torch.float32).numpy())
            bplan.params = {"bf_scale": scale, "bf_std": std, "bf_size": size}
            gate_res = u[2]
        else:
            gate_res = rs(1)[0]
        # ---- resampling (synthseg.py:63-80), then the noise gate
        rplan = ResamplePlan()
        if gate_res < rs_.prob:
            u = rs(3)
            rplan.active = True
            # np.random.uniform(lo, hi) == lo + (hi - lo) * random_sample()
            spacing = np.array([1.0, 1.0, 1.0]) * (rs_.min_resolution + (rs_.max_resolution - rs_.min_resolution) * float(u[0]))
            rplan.spacing = spacing
            rplan.stds, rplan.new_size, rplan.factors, rplan.tabs = T.resample_plan(tuple(shape), self._resolution64(), spacing, float(u[1]))
            gate_noise = u[2]
        else:
            gate_noise = rs(1)[0]
        # ---- noise (synthseg.py:218-232)
        nplan = NoisePlan()
        if gate_noise < nz.prob:
            nplan.active = True
            std = nz.std_min + (nz.std_max - nz.std_min) * rs(1)
            nplan.std32 = float(np.asarray(std, dtype=np.float32).reshape(-1)[0])
            nplan.field = _rng.normal_field(tuple(rplan.new_size if rplan.active else shape), stream_id=2)
        return m2s, gmm_plan, dplan, g, bplan, rplan, nplan

    # A sample goes through these host phases so that B samples can share one parameter upload and one native call:
    #   _prepare : every random draw, in the reference's order, and the small arrays added to the arena   (no device work)
    #   arena.upload
    # then either its plan (_flat_plan) and one fsg_sample_pack_run / fsg_sample_run_batch call, or _resolve (device views of
    # the uploaded arrays) and the stage-by-stage launches (_run_stagewise).
    def _prepare(self, image, segmentation, seeds, genparams, arena, segmentation_u8=None):
        if genparams:
            genparams = self._validated_genparams(genparams)
        dev = self.device
        ig, sd = self.intensity_generator, self.spatial_deform
        c = _Ctx()
        c.arena, c.image, c.segmentation, c.segmentation_u8, c.genparams = arena, image, segmentation, segmentation_u8, genparams
        c.labels, c.label_parts, c.gmm_plan, c.selected_seeds = None, None, None, {}
        drawn = False
        if seeds is not None:
            gs = genparams.get("selected_seeds", {})
            if hasattr(seeds, "parts") and ig.meta_labels <= 4 and not genparams:
                # the common case (device-resident SeedBank, nothing fixed by the caller): every draw of the sample in bulk
                shape = tuple(seeds.shape)
                m2s, c.gmm_plan, c.dplan, c.g, c.bplan, c.rplan, c.nplan = self._draw_all_fast(shape)
                c.label_parts, c.selected_seeds = seeds.parts(m2s), {"mlabel2subclusters": m2s}
                drawn = True
            elif hasattr(seeds, "parts") and ig.meta_labels <= 4:  # device-resident SeedBank
                m2s = ig.draw_subclusters(gs)
                c.label_parts, c.selected_seeds = seeds.parts(m2s), {"mlabel2subclusters": m2s}
                shape = tuple(c.label_parts[0].shape)
            else:
                c.labels, c.selected_seeds = ig.load_seeds(seeds=seeds, genparams=gs)
                shape = tuple(c.labels.shape)
            if not drawn:
                c.gmm_plan = ig.plan_intensities(shape, genparams.get("seed_intensities", {}))
        else:
            if image is None:
                raise ValueError(
                    "If no seeds are passed, an image must be loaded to be used as intensity prior!")
            shape = tuple(image.shape)
        c.shape = shape
        if not drawn:
            c.dplan, c.g, c.bplan, c.rplan, c.nplan = self._draw_plans(shape, genparams)
        dplan, bplan, rplan = c.dplan, c.bplan, c.rplan

        c.sb = sd.make_spec(dplan, shape, flip_in_kernel=True, arena=arena) if dplan.active else None
        c.bias_tabs, c.bias_off = None, None
        if bplan.active:
            c.bias_tabs = K.device_tables_for(self.biasfield.tables(bplan, shape), dev)
            c.bias_off = arena.add(bplan.grid.numpy())
        c.rs_tabs = c.back_tabs = None
        if rplan.active:
            # the three per-axis tables depend on (low-res size, size) only: one DeviceTables object per pair
            rs_cache = self.__dict__.setdefault("_rs_dt", {})
            rs_key = (tuple(rplan.new_size), shape)
            c.rs_tabs = rs_cache.get(rs_key)
            if c.rs_tabs is None:
                if len(rs_cache) > 4096:
                    rs_cache.clear()
                c.rs_tabs = rs_cache[rs_key] = K.DeviceTables(rplan.tabs, dev, arena)
            # zoom-back by 1 / factors, factors = new_size / size (tables.resample_plan): a function of the two shapes
            bt, new = T.zoom_tables_between(tuple(rplan.new_size), shape, True)
            c.back_tabs = K.device_tables_for(bt, dev)
        c.mm_off = arena.add(_MM8_INIT)  # the sample's min/max keys arrive initialised with its parameters
        c.slots_off = arena.add(_MM_SLOTS_INIT) if rplan.active else None
        c.gm_off = None
        if c.gmm_plan is not None:
            c.gm_off = (arena.add(c.gmm_plan.mus.numpy()), arena.add(c.gmm_plan.sigmas.numpy()), c.gmm_plan.mus.numel())
        c.has_art = any(a is not None for a in self.artifacts.values())
        c.keep = []
        return c

    @staticmethod
    def _intensity_views(c):
        """mus / sigmas of the sample as device views of its uploaded arena."""
        c.seed_intensities, c.mus, c.sigmas = {}, None, None
        if c.gmm_plan is not None:
            off_mus, off_sigmas, ntab = c.gm_off
            c.mus, c.sigmas = c.arena.f32(off_mus, (ntab,)), c.arena.f32(off_sigmas, (ntab,))
            c.seed_intensities = {"mus": c.mus, "sigmas": c.sigmas}

    def _resolve(self, c):
        self._intensity_views(c)
        c.bias_dev = c.arena.f32(c.bias_off, tuple(c.bplan.grid.shape)) if c.bplan.active else None
        c.gam = float(c.g) if c.g is not None else None
        c.spec = c.sb.build() if c.dplan.active else None

    def _synth_params(self, c, artifacts):
        return self._params(c.selected_seeds, c.seed_intensities, c.dplan, c.g, c.bplan, c.rplan, c.nplan, artifacts)

    # ---- keyed mode (fetalsyngen_amd/keyed.py, csrc/fsg_keyed.hip) -----------------------------------------------------
    def keyed_context(self, shape):
        from .. import keyed

        ctxs = self.__dict__.setdefault("_keyed", {})
        shape = tuple(int(v) for v in shape)
        kc = ctxs.get(shape)
        if kc is None:
            if len(ctxs) >= 4:
                ctxs.pop(next(iter(ctxs))).close()
            kc = ctxs[shape] = keyed.KeyedContext(self, shape)
        return kc

    def _is_keyed(self) -> bool:
        return (self.rng or _rng.get_mode()) == "keyed"

    def _keyed_applies(self, image, segmentation, seeds, genparams, segmentation_u8, labels_u8) -> bool:
        """image: None, or a CUDA float32 contiguous tensor of the segmentation's shape (anything else takes the fallback);
        seeds: a device-resident bank, or None with an image (the image is the intensity prior).  `genparams` do not
        matter: the keyed path honours them (`keyed.overrides_of`)."""
        if image is not None:
            if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.is_contiguous()
                    and torch.is_tensor(segmentation) and image.shape == segmentation.shape and image.device == segmentation.device):
                return False
        return (self.native_pipeline and (hasattr(seeds, "parts") or (seeds is None and image is not None))
                and self.intensity_generator.meta_labels <= 4 and torch.is_tensor(segmentation) and segmentation.is_cuda
                and segmentation.dtype == torch.float32 and segmentation.is_contiguous()
                and (segmentation_u8 is None or labels_u8))

    def _pipeline_keyed(self, segmentation, bank, key, scale01, labels_u8, out=None, seg_out=None, next_key=None, image=None,
                        image_out=None, genparams=None):
        """One keyed sample: the generator's own (label twin, image prior, workspace, outputs, instrumentation) handed to
        `KeyedContext.run` -- ONE native call -- then the pass-through of unwarped volumes, `synth_params` and the SR-artifact
        stages.  Returns (image, labels, warped real image | None, synth_params), or None outside the fused kernels' domain.

        image: the subject's real image (checked by `_keyed_applies`), deformed by the same warp launch as the labels.  With
        `bank=None` its cached prior (`_image_prior`) takes the place of the GMM draw; with a bank the synthetic channel is that
        of the same key without an image.  next_key (a batch, a stream of indices) and genparams (validated; what cannot be
        honoured raises ValueError): see `run`.  SR-artifact stages: the fused call leaves the image divided by its maximum, as
        the stage-wise path hands it to them; `_artifact_tail` runs them under the key.  They synchronise with the host (picks,
        plans), so on several streams they serialise the streams' host side; their kernels still run on the sample's stream."""
        from .. import keyed

        shape = tuple(segmentation.shape)
        kc = self.keyed_context(shape)
        kc.register_tables()
        twin = self._label_twin(segmentation)
        if labels_u8 and twin is None:
            return None
        ent = kc.subject(bank, segmentation, twin)
        dev = segmentation.device
        prior = self._image_prior(image) if (image is not None and bank is None) else None
        img_given, given, out_given = image_out is not None, seg_out is not None, out is not None
        if image is not None and image_out is None:
            image_out = torch.empty(shape, dtype=torch.float32, device=dev)
        has_art = any(a is not None for a in self.artifacts.values())
        events, tr = self._instrument()  # (whether this sample resamples is drawn inside the call)
        got = None
        try:
            got = kc.run(key, ent, self._workspace, dev, out, seg_out, labels_u8, scale01 and not has_art, events=events, tr=tr,
                         next_key=next_key, image=image, image_out=image_out, prior=prior, genparams=genparams)
        finally:  # (also when the call raises: genparams that cannot be honoured, an error of the native call)
            if events is not None and (got is None or not got[0].resample_active):
                for e in events:
                    _lib.load().fsg_event_destroy(e)
            if tr is not None and got is None:
                tr.close()
        if got is None:
            return None
        d, block, carried, out, seg_out = got
        if events is not None and d.resample_active:
            self._keep_blur_events(events, d.blur_ntaps, d.low_shape)
        if tr is not None:
            tr.meta = {"shape": shape, "low_shape": tuple(d.low_shape) if d.resample_active else None,
                       "blur_ntaps": list(d.blur_ntaps), "label_bytes": 2 if ent.codes else 4, "draw_carried": carried}
            self.stage_traces.append(tr)
        if not d.deform_active:  # no warp ran: the labels pass through, and so does the image
            passed = twin if labels_u8 else segmentation
            seg_out = seg_out.copy_(passed) if given else passed
            if image is not None:
                image_out = image_out.copy_(image) if img_given else image
        params = keyed.params_of(d, block)
        if bank is None:  # no seeds were selected and no intensities drawn, as in the stage-by-stage path
            params["selected_seeds"], params["seed_intensities"] = {}, {}
        if has_art:
            result, params["artifacts"] = self._artifact_tail(out, seg_out, genparams or {}, scale01, key)
            if result is not out:
                out = out.copy_(result) if out_given else result
        return out, seg_out, image_out, params

    def _pipeline(self, image, segmentation, seeds, genparams, scale01: bool, segmentation_u8=None, labels_u8: bool = False,
                  key: int | None = None, next_key: int | None = None):
        """labels_u8: return the labels as uint8 (same values; written as such by the fused warp where the fused path runs,
        converted afterwards otherwise).  key (keyed mode): the sample's 64-bit key; None = the key announced by
        `sharding.seed_for_sample` / `announce_key`, else one drawn from numpy's global generator."""
        if self._is_keyed():
            from .. import sharding

            if genparams:
                genparams = self._validated_genparams(genparams)
            announced = sharding.take_key()  # consumed whichever key is used: it must not reach a later call
            if key is None and genparams and "key" in genparams:  # a keyed sample's own synth_params handed back
                key = int(genparams["key"])
            if key is None:
                key = announced
            if key is None:
                key = int(np.random.randint(0, 1 << 62)) << 1
            key &= 0xFFFFFFFFFFFFFFFF
            if self._keyed_applies(image, segmentation, seeds, genparams, segmentation_u8, labels_u8):
                got = self._pipeline_keyed(segmentation, seeds, key, scale01, labels_u8, next_key=next_key, image=image,
                                           genparams=genparams)
                if got is not None:
                    return got
            # outside the keyed path's domain: a "device"-mode sample of the global generators seeded from the key
            np.random.seed(key & 0xFFFFFFFF)
            torch.default_generator.manual_seed(key >> 1)
        if labels_u8:
            out, seg, img, params = self._pipeline_f(image, segmentation, seeds, genparams, scale01, segmentation_u8, True)
            return out, (seg if seg.dtype == torch.uint8 else seg.to(torch.uint8)), img, params
        return self._pipeline_f(image, segmentation, seeds, genparams, scale01, segmentation_u8, False)

    def _pipeline_f(self, image, segmentation, seeds, genparams, scale01: bool, segmentation_u8=None, labels_u8: bool = False):
        with _rng.use(self.rng):
            arena = T.Arena()
            c = self._prepare(image, segmentation, seeds, genparams, arena, segmentation_u8)
            arena.upload(self.device)
            if self._native_ok(c, labels_u8):
                native = self._run_native(c, scale01, labels_u8)
                if native is not None:
                    return native[0], native[1], None, self._synth_params(c, {})
            self._resolve(c)
            return self._run_stagewise(c, scale01)

    def sample_batch(self, items, genparams_list=None, scale01: bool = False, streams: int = 1, lazy_items: int | None = None,
                     labels_u8: bool = False, keys=None):
        """B samples with one parameter upload and one native call.

        items: sequence of (image | None, segmentation, seeds) as for `sample`; the host draws are made sample by sample
        in this order, so the results are bit-identical to B consecutive `sample` calls under the same generator state
        (reference: B x FetalSynthGen.sample, generator/model.py:231-276).
        Returns (images (B,H,W,D) float32, labels (B,H,W,D) float32, [image_b | None], [synth_params_b]) -- one tensor per
        output, so a stager moves the batch with one copy.  streams > 1: consecutive samples are enqueued round-robin on
        that many side streams (their kernel tails overlap); the current stream waits for all of them before returning.
        Samples outside the fused path's domain fall back to the per-sample path, with the draws already made.
        lazy_items=B: `items` is an iterator of B entries consumed one at a time, each right before that sample's host
        draws (callers that re-seed the global generators per sample, e.g. PrefetchingStream).
        labels_u8: the labels tensor as uint8 (same values), written as such by the fused warp."""
        if lazy_items is None:
            items = list(items)
            B = len(items)
        else:
            B = int(lazy_items)
        if keys is not None and self._is_keyed():
            items = list(items)
            got = self._sample_batch_keyed(items, [int(k) for k in keys], scale01, streams, labels_u8, genparams_list)
            if got is not None:
                return got
            if genparams_list is None:
                    raise ValueError("keyed sample_batch: items outside the fused keyed path (need subjects of one shape with device-resident "
                                 "volumes -- a SeedBank, or a float32 image as intensity prior)")
        genparams_list = list(genparams_list) if genparams_list is not None else [{}] * B
        if len(genparams_list) != B:
            raise ValueError("genparams_list must have one entry per item")
        with _rng.use(self.rng):
            arena = T.Arena()
            ctxs = [self._prepare(img, seg, seeds, gp, arena) for (img, seg, seeds), gp in zip(items, genparams_list)]
            if len(ctxs) != B:
                raise ValueError(f"items yielded {len(ctxs)} entries, expected {B}")
            arena.upload(self.device)
            for c in ctxs:
                self._resolve(c)
            shapes = {c.shape for c in ctxs}
            fused = B > 0 and len(shapes) == 1 and all(self._native_ok(c) for c in ctxs)
            if fused:
                for c in ctxs:
                    self._native_operands(c)
                shape = ctxs[0].shape
                out_all, seg_all, nstreams, main, side, wss = self._batch_outputs(B, shape, streams, labels_u8,
                                                                                  max(self._rows_needed(c) for c in ctxs))
                plans = (_lib.SamplePlan * B)()
                lib, fb, ok = _lib.load(), self._flat, True
                for b, c in enumerate(ctxs):
                    if not c.dplan.active:
                        seg_all[b].copy_(c.seg)  # no deformation: labels pass through (same stream as the upload)
                    ok = ok and self._flat_plan(c, scale01, out_all[b], seg_all[b], wss[b % nstreams],
                                                self._twin_of(c) if c.dplan.active else None)
                    if ok:  # _flat holds one plan: pack it before the next one is built
                        _lib.check(lib.fsg_sample_plan_pack(C.byref(plans[b]), fb["ivp"], _lib.PLAN_I.COUNT, fb["fvp"], _lib.PLAN_F.COUNT,
                                                            fb["tbp"]), "fsg_sample_plan_pack")
                if ok:
                    handles = (C.c_void_p * nstreams)(*[s_.cuda_stream for s_ in side])
                    with self._forked(main, side):
                        rc = lib.fsg_sample_run_batch(plans, B, handles, nstreams)
                    if rc not in (_lib.E_ALIGN, _lib.E_TOOBIG):
                        _lib.check(rc, "fsg_sample_run_batch")
                        return out_all, seg_all, [None] * B, [self._synth_params(c, {}) for c in ctxs]
                    fused = False  # nothing usable was produced: per-sample path below (same plans, no new draws)
            outs = []
            for c in ctxs:
                native = self._run_native(c, scale01) if self._native_ok(c) else None
                outs.append((native[0], native[1], None, self._synth_params(c, {})) if native is not None
                            else self._run_stagewise(c, scale01))
        same = len({tuple(o[0].shape) for o in outs}) == 1 if outs else False
        images = torch.stack([o[0] for o in outs]) if same else [o[0] for o in outs]
        ldt = torch.uint8 if labels_u8 else torch.float32
        labels = torch.stack([o[1].to(ldt) for o in outs]) if same else [o[1].to(ldt) if labels_u8 else o[1] for o in outs]
        return images, labels, [o[2] for o in outs], [o[3] for o in outs]

    def _sample_batch_keyed(self, items, keys, scale01, streams, labels_u8, genparams_list=None):
        """B keyed samples written straight into one (B,H,W,D) tensor per output; sample b is `sample(..., key=keys[b])`, with
        `genparams=genparams_list[b]` where that list is given.  Configured SR-artifact stages run per sample on the sample's
        stream; their host synchronisations serialise the streams (accepted: the stages dominate such a sample anyway)."""
        B = len(items)
        if B == 0 or len(keys) != B:
            return None
        gps = [self._validated_genparams(gp) if gp else None for gp in genparams_list] if genparams_list is not None else [None] * B
        if len(gps) != B:
            raise ValueError("genparams_list must have one entry per item")
        if not all(self._keyed_applies(img, seg, seeds, {}, None, labels_u8) for img, seg, seeds in items):
            return None
        shapes = {tuple(seg.shape) for _i, seg, _s in items}
        if len(shapes) != 1:
            return None
        shape = shapes.pop()
        out_all, seg_all, nstreams, main, side, _wss = self._batch_outputs(B, shape, streams, labels_u8)
        params, images = [], [None] * B
        with_img = [b for b, (img, _s, _b) in enumerate(items) if img is not None]
        if with_img:  # the deformed real images of the batch as one tensor, like the other outputs
            img_all = torch.empty((len(with_img), *shape), dtype=torch.float32, device=out_all.device)
            for q, b in enumerate(with_img):
                images[b] = img_all[q]
            for img, _s, bank in items:  # priors are subject constants: computed (once) on the main stream, ahead of the fork
                if img is not None and bank is None:
                    self._image_prior(img)
        with self._forked(main, side):
            for b, ((img, seg, seeds), key) in enumerate(zip(items, keys)):
                with torch.cuda.stream(side[b % nstreams]):  # (the next sample of THIS stream: its draw job rides along)
                    nxt = b + nstreams  # (named only when it has nothing fixed: a carried block holds the key's own tables)
                    got = self._pipeline_keyed(seg, seeds, key & 0xFFFFFFFFFFFFFFFF, scale01, labels_u8, out=out_all[b],
                                               seg_out=seg_all[b], next_key=keys[nxt] if nxt < B and not gps[nxt] else None,
                                               image=img, image_out=images[b], genparams=gps[b])
                if got is None:
                    return None
                params.append(got[3])
        return out_all, seg_all, images, params

    def _batch_outputs(self, B, shape, streams, labels_u8, rows=None):
        """(images, labels, stream count, current stream, the streams its samples go round-robin on, [with `rows`: one scratch
        set of that many rows per stream, allocated ahead of the outputs]) of a fused batch."""
        dev = torch.device(self.device)
        nstreams = max(1, min(int(streams), B))
        main = torch.cuda.current_stream(dev)
        side = self._side_streams(nstreams) if nstreams > 1 else [main]
        wss = []
        for q in range(nstreams if rows is not None else 0):
            with torch.cuda.stream(side[q]):
                wss.append(self._workspace(shape, rows))
        out_all = torch.empty((B, *shape), dtype=torch.float32, device=dev)
        seg_all = torch.empty((B, *shape), dtype=torch.uint8 if labels_u8 else torch.float32, device=dev)
        return out_all, seg_all, nstreams, main, side, wss

    @staticmethod
    @contextlib.contextmanager
    def _forked(main, side):
        """What the block enqueues on the `side` streams starts after what `main` holds now (one fork event), and `main` waits
        for it afterwards (one join event per side stream).  `[main]`: nothing to order.  A block that raises is not joined."""
        if len(side) > 1:
            fork = torch.cuda.Event()
            fork.record(main)
            for s_ in side:
                s_.wait_event(fork)
        yield
        if len(side) > 1:
            for s_ in side:
                join = torch.cuda.Event()
                join.record(s_)
                main.wait_event(join)

    def _side_streams(self, n):
        cur = self.__dict__.setdefault("_batch_streams", [])
        while len(cur) < n:
            cur.append(torch.cuda.Stream(device=torch.device(self.device)))
        return cur[:n]

    def _run_stagewise(self, c, scale01):
        """Stage-by-stage launches of a prepared sample (images as intensity prior, SR-artifact stages, host label
        tensors, uint8 label output, configurations outside the fused kernels' domain)."""
        dev = self.device
        sd = self.spatial_deform
        image, segmentation, genparams = c.image, c.segmentation, c.genparams
        gmm_plan, dplan, bplan, rplan, nplan = c.gmm_plan, c.dplan, c.bplan, c.rplan, c.nplan
        mus, sigmas, gam, bias_dev, bias_tabs, spec = c.mus, c.sigmas, c.gam, c.bias_dev, c.bias_tabs, c.spec
        rs_tabs, back_tabs, has_art = c.rs_tabs, c.back_tabs, c.has_art
        if gmm_plan is not None:
            f = gmm_plan.field
            z = f.device_tensor(dev) if f.host is not None else None
            if c.label_parts is not None:
                output = K.gmm_sample_parts(c.label_parts, mus, sigmas, noise=z, seed=f.seed or 0,
                                            stream_id=f.stream_id)
            else:
                labels = c.labels
                if labels.dtype not in (torch.uint8, torch.int64):
                    labels = labels.long()
                labels = labels.to(dev).contiguous()
                output = K.gmm_sample(labels, mus, sigmas, noise=z, seed=f.seed or 0, stream_id=f.stream_id)
        else:
            output = self._intensity_prior(image)
        image = image.to(dev) if image is not None else None
        # one init launch for every min/max key of the sample: [min x,y,z | zoom min] [zoom max | unused x3]
        mm8 = K.new_minmax(dev, 4, 4)
        if dplan.active:
            image, segmentation, output = sd.run(dplan, image, segmentation, output, spec=spec,
                                                 mm6=K.coords_floormin(spec, mm8), gamma=gam, bias=bias_dev,
                                                 bias_tabs=bias_tabs, segmentation_u8=c.segmentation_u8)
        else:
            segmentation = segmentation.to(dev)
            if gam is not None:
                output = K.gamma(output, gam)
            if bplan.active:
                output = K.bias_mul(output, bias_dev, bias_tabs)

        fuse_scale = scale01 and not has_art
        f = nplan.field if nplan.active else None
        z = f.device_tensor(dev) if (f is not None and f.host is not None) else None
        if rplan.active:
            low = self.resampled.blur_resample(output.contiguous(), rplan.stds, rs_tabs,
                                               noise_std=nplan.std32 if nplan.active else 0.0, noise=z,
                                               seed=(f.seed if (f is not None and f.host is None) else None),
                                               stream_id=f.stream_id if f is not None else 0)
            mm2 = K.zoom_minmax(low, back_tabs, mm=mm8[3:5])
            output = K.zoom_normalise(low, back_tabs, mm2, mode=1 if fuse_scale else 0)
        else:
            if nplan.active:
                output = K.add_noise(output, nplan.std32, noise=z, seed=f.seed or 0, stream_id=f.stream_id)
            if fuse_scale:
                output = K.scale(output, K.reduce_minmax(output), mode=1)
        output, artifacts = self._artifact_tail(output, segmentation, genparams, scale01)
        return output, segmentation, image, self._synth_params(c, artifacts)
