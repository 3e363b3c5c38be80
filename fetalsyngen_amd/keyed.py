"""Keyed mode (`rng="keyed"`): host side of `fsg_keyed_*` (include/fsg_hip.h, csrc/fsg_keyed.hip).

The reference's generator draws ~30 scalars and three small tensors per sample from numpy's / torch's global generators,
one interpreter round trip each; replaying that tape costs the host ~230 us per 256^3 sample -- as much
as the GPU needs for the whole sample.  In keyed mode a sample is a pure function of its 64-bit key
(`sharding.sample_key(base_seed, index)`): every draw comes from Philox4x32-10 under that key, the scalars in C inside
ONE native call, the small tensors on the device.  Python hands over pointers and the key, and turns the exported draws
(`fsg_keyed_draws`) into the reference's `synth_params` dictionary.

Distributions and the arithmetic from draw to parameter are the reference's; the random numbers are not (by design -- use
`rng="reference"` for same-seed parity with a CPU run of the reference).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from . import kernels as K
from . import seedcodes
from . import tables as T
from .identity import IdentityCache


def config_of(gen, shape) -> _lib.KeyedConfig:
    """fsg_keyed_config of a FetalSynthGen (its stage objects hold the reference's YAML keys)."""
    ig, sd, bf, rs, nz, gm = (gen.intensity_generator, gen.spatial_deform, gen.biasfield, gen.resampled, gen.noise, gen.gamma)
    c = _lib.KeyedConfig()
    c.shape[:] = [int(v) for v in shape]
    c.size[:] = [int(v) for v in sd.size]
    c.resolution[:] = [float(v) for v in gen.resolution]
    c.min_subclusters, c.max_subclusters, c.meta_labels = int(ig.min_subclusters), int(ig.max_subclusters), int(ig.meta_labels)
    c.nlabels = max(ig.seed_labels) + 1
    c.n_seed_labels = len(ig.seed_labels)
    c.tie_classes = int(ig.generation_classes != ig.seed_labels)
    if c.nlabels > 256 or c.n_seed_labels > 256:
        raise ValueError("keyed mode takes label values < 256")
    for j, (a, b) in enumerate(zip(ig.seed_labels, ig.generation_classes)):
        c.seed_labels[j], c.generation_classes[j] = int(a), int(b)
    c.deform_prob, c.flip_prb = float(sd.prob), float(sd.flip_prb)
    c.max_rotation, c.max_shear, c.max_scaling = float(sd.max_rotation), float(sd.max_shear), float(sd.max_scaling)
    c.nonlinear = int(bool(sd.nonlinear_transform))
    c.nonlin_scale_min, c.nonlin_scale_max, c.nonlin_std_max = float(sd.nonlin_scale_min), float(sd.nonlin_scale_max), float(sd.nonlin_std_max)
    c.gamma_prob, c.gamma_std = float(gm.prob), float(gm.gamma_std)
    c.bias_prob, c.bf_scale_min, c.bf_scale_max = float(bf.prob), float(bf.scale_min), float(bf.scale_max)
    c.bf_std_min, c.bf_std_max = float(bf.std_min), float(bf.std_max)
    c.resample_prob, c.min_resolution, c.max_resolution = float(rs.prob), float(rs.min_resolution), float(rs.max_resolution)
    c.noise_prob, c.noise_std_min, c.noise_std_max = float(nz.prob), float(nz.std_min), float(nz.std_max)
    return c


def config_dict(cfg: _lib.KeyedConfig) -> dict:
    """The configuration as plain Python values (what tests hand to the oracle's restatement)."""
    out = {}
    for name, _t in cfg._fields_:
        v = getattr(cfg, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    out["seed_labels"] = out["seed_labels"][: cfg.n_seed_labels]
    out["generation_classes"] = out["generation_classes"][: cfg.n_seed_labels]
    return out


# slots of fsg_keyed_sample_run's argument array as plain module names: KeyedContext.fill writes them once per sample
_KI, _KF = _lib.KEYED_I, _lib.KEYED_FLAG
_K_KEY, _K_OUT, _K_SEG_OUT, _K_SEG_OUT_U8, _K_SEG_IN, _K_SEG_IN_U8 = _KI.KEY, _KI.OUT, _KI.SEG_OUT, _KI.SEG_OUT_U8, _KI.SEG_IN, _KI.SEG_IN_U8
_K_BLOCK, _K_WS0, _K_WS1, _K_WS_LOW, _K_WS_ROWS, _K_ROW_STRIDE = _KI.BLOCK, _KI.WS0, _KI.WS1, _KI.WS_LOW, _KI.WS_ROWS, _KI.ROW_STRIDE
_K_SCALE01, _K_TRACE_EVENTS, _K_TRACE_IDS, _K_TRACE_CAP, _K_BANK = _KI.SCALE01, _KI.TRACE_EVENTS, _KI.TRACE_IDS, _KI.TRACE_CAP, _KI.BANK
_K_EV_BLUR_BEGIN, _K_EV_BLUR_END, _K_CODES, _K_CODE_TUPLES = _KI.EV_BLUR_BEGIN, _KI.EV_BLUR_END, _KI.CODES, _KI.CODE_TUPLES
_K_CODE_NTUPLES, _K_CODE_STRIDE, _K_FLAGS, _K_NEXT_KEY, _K_NEXT_BLOCK = _KI.CODE_NTUPLES, _KI.CODE_STRIDE, _KI.FLAGS, _KI.NEXT_KEY, _KI.NEXT_BLOCK
_K_IMAGE_IN, _K_IMAGE_OUT, _K_PRIOR_IN, _K_OVERRIDES, _K_BLOCK_BYTES = _KI.IMAGE_IN, _KI.IMAGE_OUT, _KI.PRIOR_IN, _KI.OVERRIDES, _KI.BLOCK_BYTES
_KF_BLOCK_FILLED, _KF_NEXT_NAMED = _KF.BLOCK_FILLED, _KF.NEXT_NAMED


KT_CAP = 1024  # largest low-res / coarse-grid size a tap table can be registered for (csrc/fsg_keyed.hip)


def _vec3(v, what):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 3:
        raise ValueError(f"keyed genparams: {what} takes three values, got {a.size}")
    return a.tolist()


def _scalar(v, what):
    a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
    if a.size != 1:  # (params_of emits 1-element arrays where the reference does: nonlin_scale, bf_scale, bf_std)
        raise ValueError(f"keyed genparams: {what} takes one value, got {a.size}")
    return float(a[0])


def _table(v, n, device, what):
    """A given GMM table as a float32 device tensor of `n` entries (host values are uploaded)."""
    t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32))
    t = t.detach().reshape(-1)
    if t.numel() != n:
        raise ValueError(f"keyed genparams: {what} takes {n} entries (max(seed_labels) + 1), got {t.numel()}")
    dev = torch.device(device)
    if t.dtype != torch.float32 or t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
        t = t.to(device=dev, dtype=torch.float32)
    return t.contiguous()


class Overrides:
    """A `fsg_keyed_overrides` and the device tables it points to (alive as long as this object)."""

    __slots__ = ("c", "keep")

    def __init__(self):
        self.c, self.keep = _lib.KeyedOverrides(), []


def overrides_of(genparams, cfg: _lib.KeyedConfig, device) -> Overrides | None:
    """The reference's `genparams` (None values already stripped: `FetalSynthGen._validated_genparams`) as a
    `fsg_keyed_overrides`; None when nothing in them counts.  The keys that count are the ones the stage plan() methods
    read (ImageFromSeeds.draw_subclusters / plan_intensities, SpatialDeformation.plan, RandGamma / RandBiasField /
    RandResample / RandNoise.plan); a stage's gate is forced where its plan() forces it.  Values that the C side would
    refuse raise ValueError here, in words.  Host "mus" / "sigmas" are uploaded to `device` (nothing else needs one)."""
    KO = _lib.KO
    ov = Overrides()
    o = ov.c
    mask = 0

    def finite(vals, what):
        if not np.all(np.isfinite(vals)):
            raise ValueError(f"keyed genparams: {what} is not finite")
        return vals

    m2s = genparams.get("selected_seeds", {}).get("mlabel2subclusters")
    if m2s is not None:
        for m in range(cfg.meta_labels):
            n = m2s.get(m + 1, m2s.get(str(m + 1)))
            if n is None or not (cfg.min_subclusters <= int(n) <= cfg.max_subclusters):
                raise ValueError(f"keyed genparams: mlabel2subclusters[{m + 1}] = {n!r} outside "
                                 f"[{cfg.min_subclusters}, {cfg.max_subclusters}]")
            o.subclusters[m] = int(n)
        mask |= KO.SUBCLUSTERS
    si = genparams.get("seed_intensities", {})
    for name, bit in (("mus", KO.MUS), ("sigmas", KO.SIGMAS)):
        if name in si:
            t = _table(si[name], cfg.nlabels, device, name)
            ov.keep.append(t)
            setattr(o, name + "_dev", t.data_ptr())
            o.ntab = cfg.nlabels
            mask |= bit
    dp = genparams.get("deform_params", {})
    if len(dp) > 0:  # SpatialDeformation.plan: any key forces the stage ({"flip": False} alone does)
        mask |= KO.FORCE_DEFORM
        if "flip" in dp:
            o.flip = int(bool(dp["flip"]))
            mask |= KO.FLIP
        ga = dp.get("affine", {})
        for name, bit in (("rotations", KO.ROTATIONS), ("shears", KO.SHEARS), ("scalings", KO.SCALINGS)):
            if name in ga:
                getattr(o, name)[:] = finite(_vec3(ga[name], name), name)
                mask |= bit
        gn = dp.get("non_rigid", {}) if cfg.nonlinear else {}
        if "nonlin_scale" in gn:
            o.nonlin_scale = finite(_scalar(gn["nonlin_scale"], "nonlin_scale"), "nonlin_scale")
            mask |= KO.NONLIN_SCALE
        if "nonlin_std" in gn:
            o.nonlin_std = finite(_scalar(gn["nonlin_std"], "nonlin_std"), "nonlin_std")
            mask |= KO.NONLIN_STD
        if "size_F_small" in gn:
            dims = [int(v) for v in np.asarray(gn["size_F_small"]).reshape(-1)]
            if len(dims) != 3 or min(dims) < 1 or max(dims) > KT_CAP:
                raise ValueError(f"keyed genparams: size_F_small {dims} must be three sizes in [1, {KT_CAP}]")
            o.field_dims[:] = dims
            mask |= KO.FIELD_DIMS
        elif "nonlin_scale" in gn:
            dims = [int(np.round(o.nonlin_scale * n)) for n in cfg.shape]
            if min(dims) < 1 or max(dims) > KT_CAP:
                raise ValueError(f"keyed genparams: nonlin_scale {o.nonlin_scale} gives the grid {dims}, outside [1, {KT_CAP}]")
    gp = genparams.get("gamma_params", {})
    if "gamma" in gp:
        o.gamma = finite(_scalar(gp["gamma"], "gamma"), "gamma")
        if not o.gamma > 0:
            raise ValueError(f"keyed genparams: gamma {o.gamma} must be positive")
        mask |= KO.GAMMA
    bp = genparams.get("bf_params", {})
    if len(bp) > 0:  # RandBiasField.plan: any key forces the stage; "bf_size" is not read (the size follows bf_scale)
        mask |= KO.FORCE_BIAS
        if "bf_scale" in bp:
            o.bf_scale = finite(_scalar(bp["bf_scale"], "bf_scale"), "bf_scale")
            if max(int(np.round(o.bf_scale * n)) for n in cfg.shape) > KT_CAP:
                raise ValueError(f"keyed genparams: bf_scale {o.bf_scale} gives a grid above {KT_CAP}")
            mask |= KO.BF_SCALE
        if "bf_std" in bp:
            o.bf_std = finite(_scalar(bp["bf_std"], "bf_std"), "bf_std")
            mask |= KO.BF_STD
    rp = genparams.get("resample_params", {})
    if "spacing" in rp:
        sp = finite(_vec3(rp["spacing"], "spacing"), "spacing")
        for a in range(3):
            low = cfg.shape[a] * cfg.resolution[a] / sp[a] if sp[a] > 0 else 0
            if not (sp[a] > 0 and 1 <= low < KT_CAP + 1):
                raise ValueError(f"keyed genparams: spacing {sp} (axis {a}: low-res size {int(low)}) must be positive and give "
                                 f"sizes in [1, {KT_CAP}]")
        o.spacing[:] = sp
        mask |= KO.SPACING
    npar = genparams.get("noise_params", {})
    if "noise_std" in npar:
        o.noise_std = finite(_scalar(npar["noise_std"], "noise_std"), "noise_std")
        mask |= KO.NOISE_STD
    if not mask:
        return None
    o.mask = mask
    return ov


BANK_SLOTS = 64  # seed volumes the BANK slots of fsg_keyed_sample_run's argument array hold: 4 meta labels x 16 sub-cluster counts


class Subject:
    """Addresses of one subject's volumes as fsg_keyed_sample_run takes them (the C side only sees addresses); which objects
    they were taken from is the business of `KeyedContext._subjects`."""

    __slots__ = ("bank_ptrs", "twin_ptr", "seg_ptr", "codes", "code_tuples", "code_ntuples", "code_stride")

    def __init__(self, seg, bank_ptrs, twin_ptr):
        self.bank_ptrs, self.twin_ptr, self.seg_ptr = bank_ptrs, twin_ptr, seg.data_ptr()  # twin_ptr 0: no uint8 twin yet
        self.codes = self.code_tuples = self.code_ntuples = self.code_stride = 0  # 0: no code volume (KeyedContext._codes)


class KeyedContext:
    """One `fsg_keyed_ctx` (host-only object) for a (generator configuration, volume shape) pair."""

    def __init__(self, gen, shape):
        self.lib = _lib.load()
        self.shape = tuple(int(v) for v in shape)
        self.cfg = config_of(gen, self.shape)
        self.device = gen.device
        h = C.c_void_p()
        _lib.check(self.lib.fsg_keyed_create(C.byref(self.cfg), C.byref(h)), "fsg_keyed_create")
        self.handle = h
        self.block_bytes = int(self.lib.fsg_keyed_block_bytes(h))
        self.iv = np.zeros(_lib.KEYED_I.COUNT_OV, dtype=np.int64)  # with the two override slots behind COUNT
        self.ivp, self._uv = self.iv.ctypes.data, self.iv.view(np.uint64)  # (_uv: the same slots for the unsigned 64-bit keys)
        self._subjects = IdentityCache()  # (bank | None, segmentation) under the segmentation's version -> Subject
        self._banks = weakref.WeakSet()   # every bank a subject was made of: `forget_subjects` drops their code volumes
        self.use_codes = True  # the subject's seed volumes as one uint16 code volume (seedcodes.py, built on first use)
        self._tables_ready = False
        self._keep = []  # device tables registered with the context
        self._have = set()  # (kind, axis, n) of them
        self._carried = {}  # launch stream -> (key, parameter block) the previous sample on it filled for its next one (`run`)
        # rows of the per-(x,y) coarse workspace the largest grids need (3 * field_dims[2] + bias_dims[2])
        f2 = int(np.round(self.cfg.nonlin_scale_max * self.shape[2])) if self.cfg.nonlinear else 0
        b2 = max(int(np.round(self.cfg.bf_scale_max * self.shape[2])), 1)
        self.rows_need = 3 * f2 + b2

    def close(self):
        self._carried.clear()
        if self.handle:
            self.lib.fsg_keyed_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables: built by the same cached builders as the other modes, registered by device pointer ----------------------
    def _register(self, kind, axis, n):
        self._have.add((kind, axis, int(n)))
        d = K._device_table(T.axis_table(kind, n, self.shape[axis]), self.device)
        self._keep.append(d)
        _lib.check(self.lib.fsg_keyed_set_table(self.handle, kind, axis, int(n), C.c_void_p(d.data_ptr())), "fsg_keyed_set_table")

    def register_tables(self):
        """Every tap table a sample of this configuration can ask for (bounded: the low-res size takes at most
        size * (1 - min / max resolution) values per axis, the coarse grids a handful)."""
        if self._tables_ready:
            return
        c = self.cfg
        for a in range(3):
            size = self.shape[a]
            lo = int(size * c.resolution[a] / max(c.max_resolution, c.resolution[a]))
            hi = int(size * c.resolution[a] / c.min_resolution)
            for m in range(max(lo - 1, 1), min(max(hi, lo) + 1, 4 * size) + 1):
                self._register(_lib.KT.RESAMPLE, a, m)
                self._register(_lib.KT.BACK, a, m)
            if c.nonlinear:
                for s_ in range(max(int(np.floor(c.nonlin_scale_min * size)) - 1, 1), int(np.ceil(c.nonlin_scale_max * size)) + 2):
                    self._register(_lib.KT.FIELD, a, s_)
            for s_ in range(max(int(np.floor(c.bf_scale_min * size)) - 1, 1), int(np.ceil(c.bf_scale_max * size)) + 2):
                self._register(_lib.KT.BIAS, a, s_)
        self._tables_ready = True

    def ensure_tables(self, d: _lib.KeyedDraws):
        """Register what the sample of draws `d` needs beyond `register_tables` (overrides reach sizes the configuration's
        ranges do not: a spacing outside [min, max] resolution, a given grid size)."""
        kinds = ((_lib.KT.RESAMPLE, d.resample_active, d.low_shape), (_lib.KT.BACK, d.resample_active, d.low_shape),
                 (_lib.KT.FIELD, d.deform_active and d.nonlinear, d.field_dims), (_lib.KT.BIAS, d.bias_active, d.bias_dims))
        for kind, a, n in [(kind, a, dims[a]) for kind, active, dims in kinds if active for a in range(3)]:
            if (kind, a, n) not in self._have:
                if not 1 <= n <= KT_CAP:
                    raise ValueError(f"keyed genparams: a tap table of size {n} is outside [1, {KT_CAP}]")
                self._register(kind, a, n)

    # ---- per-subject pointer block --------------------------------------------------------------------------------------
    def subject(self, bank, seg, twin):
        """The `Subject` of (bank slots, float32 segmentation, its uint8 twin), validated once per (bank, segmentation) object
        pair -- the C side only sees addresses."""
        ent = self._subjects.get((bank, seg), seg._version)
        if ent is not None:
            if twin is not None and ent.twin_ptr == 0:
                ent.twin_ptr = twin.data_ptr()
            self._codes(bank, ent)  # (built once per bank object; a rewrite of a seed volume through torch rebuilds it)
            return ent
        c, shape = self.cfg, self.shape
        dev = torch.device(self.device)
        if tuple(seg.shape) != shape or seg.dtype != torch.float32 or not seg.is_cuda or not seg.is_contiguous():
            raise ValueError(f"segmentation: expected a contiguous float32 tensor of shape {shape} on {dev}")
        ptrs = np.zeros(BANK_SLOTS, dtype=np.int64)
        vol = bank.vol if bank is not None else {}
        for n in range(c.min_subclusters, c.max_subclusters + 1) if bank is not None else ():
            for m in range(1, c.meta_labels + 1):
                part = vol[n][m]
                off_dev = part.device.type != dev.type or (dev.index is not None and part.device.index != dev.index)
                if tuple(part.shape) != shape or part.dtype != torch.uint8 or not part.is_contiguous() or off_dev:
                    raise ValueError(f"seed volume ({n}, {m}): expected a contiguous uint8 tensor of shape {shape} on {dev}, "
                                     f"got {part.dtype} {tuple(part.shape)} on {part.device}")
                ptrs[4 * (n - c.min_subclusters) + (m - 1)] = part.data_ptr()
        ent = Subject(seg, ptrs, 0 if twin is None else twin.data_ptr())
        self._codes(bank, ent)  # ~1 ms once per bank object (one pass over its volumes), little next to loading the subject
        self._subjects.put((bank, seg), ent, stamp=seg._version)
        if bank is not None:  # (None: a subject without seeds -- its image is the intensity prior -- reads no seed volume)
            self._banks.add(bank)
        return ent

    def forget_subjects(self):
        """Drop every pointer block, and the code volume of every bank one was made of (`FetalSynthGen.invalidate_label_twins`)."""
        self._subjects.clear()
        for bank in self._banks:
            bank.__dict__.pop("_seed_codes", None)

    def _codes(self, bank, ent):
        """The code fields of `ent` = the subject's code volume (seedcodes.build), kept ON the bank object so that it lives and dies with it.
        A seed volume rewritten through torch bumps its `_version`: the codes are rebuilt; a rewrite through a raw pointer needs
        `FetalSynthGen.invalidate_label_twins()` (which drops them)."""
        if not self.use_codes or bank is None:
            ent.codes = ent.code_tuples = ent.code_ntuples = ent.code_stride = 0
            return
        c = self.cfg
        vol = bank.vol
        parts = [vol[n][m] for n in range(c.min_subclusters, c.max_subclusters + 1) for m in range(1, c.meta_labels + 1)]
        ver = sum(p._version for p in parts)
        have = getattr(bank, "_seed_codes", None)
        if have is None or have[0] != ver or have[1] != self.shape:
            cols = []
            for n in range(c.min_subclusters, c.max_subclusters + 1):
                for m in range(1, 5):
                    cols.append(vol[n][m] if m <= c.meta_labels else None)
            stride = len(cols) + 1
            zero = None
            dense = []
            for col in cols:
                if col is None:
                    zero = torch.zeros_like(parts[0]) if zero is None else zero
                    col = zero
                dense.append(col)
            built = seedcodes.build_device(dense, stride) if (parts[0].numel() % 8 == 0 and parts[0].numel() <= (1 << 30)) else None
            have = (ver, self.shape, built, stride)
            bank._seed_codes = have
        built = have[2]
        if built is None:
            ent.codes = ent.code_tuples = ent.code_ntuples = ent.code_stride = 0
        else:
            ent.codes, ent.code_tuples = built[0].data_ptr(), built[1].data_ptr()
            ent.code_ntuples, ent.code_stride = int(built[1].shape[0]), int(have[3])

    def draws(self, key: int, overrides: Overrides | None = None) -> _lib.KeyedDraws:
        """Host draws of `key` (with `overrides_of(...)` honoured).  What the C side refuses of an override is a ValueError."""
        d = _lib.KeyedDraws()
        if overrides is None:
            _lib.check(self.lib.fsg_keyed_draw(self.handle, C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.byref(d)), "fsg_keyed_draw")
            return d
        rc = self.lib.fsg_keyed_draw_with(self.handle, C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.byref(overrides.c), C.byref(d))
        if rc in (_lib.E_BADARG, _lib.E_TOOBIG):
            raise ValueError(f"keyed genparams cannot be honoured for key {key}: "
                             + ("a value is non-finite, non-positive or outside its range" if rc == _lib.E_BADARG
                                else f"a grid or low-res size is above {KT_CAP}, or the parameter block above 2 GiB"))
        _lib.check(rc, "fsg_keyed_draw_with")
        return d

    def fill(self, key, ent, ws, out, seg_out, labels_u8, scale01, block, flags=0, low=None, events=None, tr=None,
             image=None, image_out=None, prior=None, next_key=0, nblock=None, ov=None, block_bytes=0):
        """EVERY slot of `fsg_keyed_sample_run`'s argument array (`self.iv`): nothing of the previous call survives.  key,
        next_key: in [0, 2^64) (they are stored through the array's uint64 view; callers mask).  ent: the
        `Subject`; ws: the generator's workspace entry (low: a larger low-res scratch in the place of its own); block, nblock:
        the parameter blocks of this key and of `next_key`; events, tr: the generator's blur event pair and StageTrace."""
        iv, uv = self.iv, self._uv
        uv[_K_KEY] = key
        iv[_K_OUT] = out.data_ptr()
        iv[_K_SEG_OUT], iv[_K_SEG_OUT_U8] = (0, seg_out.data_ptr()) if labels_u8 else (seg_out.data_ptr(), 0)
        iv[_K_SEG_IN], iv[_K_SEG_IN_U8], iv[_K_BLOCK] = ent.seg_ptr, ent.twin_ptr, block.data_ptr()
        iv[_K_WS0], iv[_K_WS1], iv[_K_WS_LOW] = ws["ws0"].data_ptr(), ws["ws1"].data_ptr(), (low if low is not None else ws["low"]).data_ptr()
        iv[_K_WS_ROWS], iv[_K_ROW_STRIDE] = (ws["rows"].data_ptr() if ws["rows"] is not None else 0), ws["stride"]
        iv[_K_SCALE01] = int(bool(scale01))
        iv[_K_OVERRIDES], iv[_K_BLOCK_BYTES] = (C.addressof(ov.c), block_bytes) if ov is not None else (0, 0)
        iv[_K_TRACE_EVENTS], iv[_K_TRACE_IDS], iv[_K_TRACE_CAP] = tr.slots() if tr is not None else (0, 0, 0)
        iv[_K_BANK:_K_BANK + BANK_SLOTS] = ent.bank_ptrs
        iv[_K_EV_BLUR_BEGIN], iv[_K_EV_BLUR_END] = events if events is not None else (0, 0)
        # the subject's code volume (0: four label volumes)
        iv[_K_CODES], iv[_K_CODE_TUPLES], iv[_K_CODE_NTUPLES], iv[_K_CODE_STRIDE] = ent.codes, ent.code_tuples, ent.code_ntuples, ent.code_stride
        iv[_K_IMAGE_IN], iv[_K_IMAGE_OUT] = (image.data_ptr(), image_out.data_ptr()) if image is not None else (0, 0)
        iv[_K_PRIOR_IN] = prior.data_ptr() if prior is not None else 0
        iv[_K_FLAGS] = flags
        uv[_K_NEXT_KEY], iv[_K_NEXT_BLOCK] = (next_key, nblock.data_ptr()) if nblock is not None else (0, 0)

    def run(self, key, ent, workspace, dev, out, seg_out, labels_u8, scale01, events=None, tr=None, next_key=None, image=None,
            image_out=None, prior=None, genparams=None):
        """The sample of `key` on the current stream in ONE native call (draws, the draw kernel, the launch sequence).  Returns
        (draws, parameter block, whether that block was carried, image, labels), or None outside the fused kernels' domain.
        workspace(shape, rows): the caller's scratch entry; out, seg_out: the caller's output tensors, None: made here, behind
        the workspace (the order the memory pool has always seen).  next_key: the key this context will be asked for NEXT on this
        stream; its draw job rides in this sample's head launch and the block it fills waits in `_carried` (a call for
        another key drops it).  genparams (validated): the values the caller fixed (`overrides_of`); such a sample uses no
        carried block (that one holds the key's own tables) and sizes its block, row workspace and low-res scratch itself."""
        ov = overrides_of(genparams, self.cfg, dev) if genparams else None
        rows_need, block_bytes, low = self.rows_need, self.block_bytes, None
        if ov is not None:
            d0 = self.draws(key, ov)
            self.ensure_tables(d0)
            rows_need = max(rows_need, 3 * d0.field_dims[2] + d0.bias_dims[2])
            block_bytes = max(block_bytes, d0.block_bytes)
            if d0.resample_active and int(np.prod(list(d0.low_shape))) > int(np.prod(self.shape)):  # a spacing below the resolution
                low = torch.empty(int(np.prod(list(d0.low_shape))), dtype=torch.float32, device=dev)
        ws = workspace(self.shape, rows_need)
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=dev)
        if seg_out is None:
            seg_out = torch.empty(self.shape, dtype=torch.uint8 if labels_u8 else torch.float32, device=dev)
        # what the previous call carried for this one: the parameter block of exactly this key, on this stream
        stream = K._stream(dev)
        pre = self._carried.pop(stream.value, None)  # one carried block per launch stream
        if pre is not None and pre[0] == key and ov is None:
            block, flags = pre[1], _KF_BLOCK_FILLED
        else:
            block, flags = torch.empty(block_bytes, dtype=torch.uint8, device=dev), 0
        nblock = None
        if next_key is not None:
            next_key &= 0xFFFFFFFFFFFFFFFF
            nblock = torch.empty(self.block_bytes, dtype=torch.uint8, device=dev)
            flags |= _KF_NEXT_NAMED
        self.fill(key, ent, ws, out, seg_out, labels_u8, scale01, block, flags=flags, low=low, events=events, tr=tr, image=image,
                  image_out=image_out, prior=prior, next_key=next_key, nblock=nblock, ov=ov, block_bytes=block_bytes)
        d = _lib.KeyedDraws()
        rc = self.lib.fsg_keyed_sample_run(self.handle, self.ivp, len(self.iv), C.byref(d), stream)
        if rc in (_lib.E_ALIGN, _lib.E_TOOBIG):
            return None
        _lib.check(rc, "fsg_keyed_sample_run")
        if nblock is not None and d.rode:
            if len(self._carried) > 8:
                self._carried.clear()
            self._carried[stream.value] = (next_key, nblock)
        return d, block, flags & _KF_BLOCK_FILLED, out, seg_out


def params_of(d: _lib.KeyedDraws, block: torch.Tensor | None) -> dict:
    """The reference's `synth_params` dictionary (generator/model.py:231-276: selected_seeds, seed_intensities,
    deform_params, gamma_params, bf_params, resample_params, noise_params, artifacts) from exported draws.  `block`: the
    sample's device parameter block (mus / sigmas are views of it, device tensors as in the reference)."""
    m2s = {m + 1: int(d.subclusters[m]) for m in range(4) if d.subclusters[m]}
    si = {}
    if block is not None:
        f = block.view(torch.float32)
        si = {"mus": f[d.off_mus >> 2:(d.off_mus >> 2) + d.ntab], "sigmas": f[d.off_sigmas >> 2:(d.off_sigmas >> 2) + d.ntab]}
    if d.deform_active:
        nr = {}
        if d.nonlinear:
            nr = {"nonlin_scale": np.array([d.nonlin_scale]), "nonlin_std": d.nonlin_std, "size_F_small": list(d.field_dims)}
        dp = {"affine": {"rotations": np.array(d.rotations), "shears": np.array(d.shears), "scalings": np.array(d.scalings)},
              "non_rigid": nr, "flip": bool(d.flip)}
    else:
        dp = {"affine": None, "non_rigid": None, "flip": False}
    if d.bias_active:
        bp = {"bf_scale": np.array([d.bf_scale]), "bf_std": np.array([d.bf_std]), "bf_size": list(d.bias_dims)}
    else:
        bp = {"bf_scale": None, "bf_std": None, "bf_size": None}
    return {
        "selected_seeds": {"mlabel2subclusters": m2s},
        "seed_intensities": si,
        "deform_params": dp,
        "gamma_params": {"gamma": d.gamma if d.gamma_active else None},
        "bf_params": bp,
        "resample_params": {"spacing": list(d.spacing3) if d.resample_active else None},
        "noise_params": {"noise_std": float(d.noise_std32) if d.noise_active else None},
        "artifacts": {},
        "key": int(d.key),
    }
