"""Torch-tensor front-end of the C ABI: pointer/shape plumbing only, no arithmetic.

Every function validates device / dtype / contiguity on the host (a faulting kernel can take the whole
node down), launches on torch's current HIP stream and returns freshly allocated device tensors.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .tables import Arena, TAP_DTYPE, is_down_table

F32 = torch.float32


def _stream(ref=None):
    """Raw hipStream_t of torch's current stream on `ref`'s device (tensor, device or None).

    `torch.cuda.current_stream()` walks through availability checks (environment lookups) on every
    call; the raw getter is ~100x cheaper and this sits in front of every launch."""
    if isinstance(ref, torch.Tensor):
        idx = ref.device.index
    elif ref is None:
        idx = torch.cuda.current_device()
    else:
        idx = torch.device(ref).index
    if idx is None:
        idx = torch.cuda.current_device()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def _need_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(
                "fetalsyngen_amd kernels run on an MI355X (device='cuda:N') only; there is no CPU fallback"
            )
        if not t.is_contiguous():
            raise ValueError("tensor must be contiguous")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _f32(t, name="tensor"):
    if t.dtype != F32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t


def _dims3(t):
    if t.dim() != 3:
        raise ValueError(f"expected a 3-D volume, got shape {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


# ---- argument checks the slice-acquisition entries and the reconstruction solvers share ----
def _mask(m, name, shape, device=None):
    """A bool/uint8 contiguous device mask of `shape` (leading dimensions of 1 aside; an int: that many elements in any
    shape), on `device` where one is given.  None stays None."""
    if m is None:
        return None
    _need_gpu(m)
    if m.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{name} must be bool/uint8, got {m.dtype}")
    if isinstance(shape, int):
        fits = m.numel() == shape
    else:
        fits = tuple(m.shape[-len(shape):]) == tuple(shape) and m.numel() == math.prod(shape)
    if not fits:
        raise ValueError(f"{name} shape {tuple(m.shape)} does not match {shape}")
    _same_device(device, "its operands", (name, m))
    return m


def _same_device(device, what, *named):
    """every (name, tensor or None) is on `device`, the device of `what` (None: nothing to hold them to)"""
    for name, t in named:
        if device is not None and t is not None and t.device != device:
            raise ValueError(f"{name} is on {t.device}, {what} on {device}")


def _nhw(t, name, n):
    """`t` is (n,h,w); returns (h, w)"""
    if t.dim() != 3 or int(t.shape[0]) != n:
        raise ValueError(f"{name} must be (n,h,w) with n={n}, got {tuple(t.shape)}")
    return int(t.shape[1]), int(t.shape[2])


def _pow2_scale(v, name):
    """the scale of a fixed-point accumulation: a power of two in [2^-20, 2^20]"""
    m, e = math.frexp(float(v))
    if m != 0.5 or not -20 <= e - 1 <= 20:
        raise ValueError(f"{name} must be a power of two in [2^-20, 2^20], got {v!r}")


class _StateBlock:
    """A device block whose layout include/fsg_hip.h states: `buf` (int64, `nbytes` bytes as the library counts them) and one
    attribute per field, a view of `buf`, carved in the header's order from a table of (name, dtype, shape)."""

    def _carve(self, entry, args, device, fields):
        self.nbytes = int(getattr(_lib.load(), entry)(*args))
        self.buf = torch.empty(self.nbytes // 8, dtype=torch.int64, device=device)
        raw, off = self.buf.view(torch.uint8), 0
        for name, dtype, shape in fields:
            size = math.prod(shape) * dtype.itemsize
            setattr(self, name, raw[off:off + size].view(dtype).view(shape))
            off += size
        if (off + 7) // 8 * 8 != self.nbytes:
            raise RuntimeError(f"{entry}{args} = {self.nbytes}, the layout of fsg_hip.h needs {off}")


class _PixelState(_StateBlock):
    """A state block for n slices plus `part` (int64), the workspace of the per-workgroup partials for (h, w) slices, sized
    by the library's entry `ws_entry`(n, h, w)."""

    def _carve_pixels(self, entry, ws_entry, args, device, fields, slice_shape):
        self._carve(entry, args, device, fields)
        self._ws_entry, self.part, self.slice_shape = ws_entry, None, None
        if slice_shape is not None:
            self.reserve(slice_shape)

    def reserve(self, slice_shape):
        """the workspace for (h, w) slices"""
        h, w = (int(v) for v in slice_shape)
        if self.slice_shape != (h, w):
            need = int(getattr(_lib.load(), self._ws_entry)(self.n, h, w))
            if need == 0:
                raise ValueError(f"no workspace for {self.n} slices of {(h, w)}")
            self.part = torch.empty(need // 8, dtype=torch.int64, device=self.buf.device)
            self.slice_shape = (h, w)
        return self.part


def _slice_count(n):
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    return n


def _iterations(name, v):
    v = int(v)
    if not 1 <= v <= _lib.SOLVER_MAX_ITER:
        raise ValueError(f"{name} must be in 1..{_lib.SOLVER_MAX_ITER}, got {v}")
    return v


_DEV_TABLES: dict = {}  # (device, id(host table)) -> (device bytes, host table kept alive)
_DEV_TABLES_MAX = 2048


_DEV_KEYS: dict = {}


def _device_key(device):
    """Stable string for a device argument (str / torch.device), memoised: this runs a dozen times per sample."""
    k = _DEV_KEYS.get(device)
    if k is None:
        k = _DEV_KEYS[device] = str(device)
    return k


def _device_table(tab, device):
    key = (_device_key(device), id(tab))
    hit = _DEV_TABLES.get(key)
    if hit is not None and hit[1] is tab:
        return hit[0]
    if tab.dtype != TAP_DTYPE:
        raise TypeError("tap table dtype")
    raw = np.ascontiguousarray(tab).view(np.uint8).reshape(-1)
    host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)  # pinned: the copy below is async
    host.numpy()[:] = raw
    d = host.to(device, non_blocking=True)
    if len(_DEV_TABLES) >= _DEV_TABLES_MAX:
        _DEV_TABLES.pop(next(iter(_DEV_TABLES)))
    _DEV_TABLES[key] = (d, tab)
    return d


_DOWN_INFO: dict = {}  # id(host table) -> (tables.is_down_table, rows it reads: max hi + 1, host table kept alive)


def _down_info(tab):
    hit = _DOWN_INFO.get(id(tab))
    if hit is not None and hit[2] is tab:
        return hit[0], hit[1]
    info = (is_down_table(tab), int(tab["hi"].max()) + 1 if len(tab) else 0)
    if len(_DOWN_INFO) >= _DEV_TABLES_MAX:
        _DOWN_INFO.pop(next(iter(_DOWN_INFO)))
    _DOWN_INFO[id(tab)] = (*info, tab)
    return info


class DeviceTables:
    """Three per-axis tap tables resident on the device.

    Tables produced by the cached builders in `tables.py` are uploaded once per device and reused
    (the host array object is the cache key); ad-hoc tables are uploaded on first use.  `down` / `reach`: per axis, whether
    the host table is a down-sampling table (tables.is_down_table: what the fused blur + resample kernels assume) and how
    many source rows it reads."""

    def __init__(self, tabs, device, arena: Arena | None = None):
        self.lengths = tuple(len(t) for t in tabs)
        info = [_down_info(t) for t in tabs]
        self.down = tuple(i[0] for i in info)
        self.reach = tuple(i[1] for i in info)
        self._dev = [_device_table(t, device) for t in tabs]
        self.ptrs = tuple(C.c_void_p(d.data_ptr()) for d in self._dev)  # the device copies never move
        self.ptrs_i = tuple(int(d.data_ptr()) for d in self._dev)        # the same as plain integers (flat plan arrays)


_DT_CACHE: dict = {}  # (id(host table list), device) -> (DeviceTables, the list kept alive)


def device_tables_for(tabs_list, device) -> DeviceTables:
    """DeviceTables for a table list with a stable identity (tables.zoom_tables_between memoises its lists): one dict hit
    per call instead of three table look-ups and a fresh pointer tuple."""
    key = (id(tabs_list), _device_key(device))
    hit = _DT_CACHE.get(key)
    if hit is not None and hit[1] is tabs_list:
        return hit[0]
    dt = DeviceTables(tabs_list, device)
    if len(_DT_CACHE) >= 4096:
        _DT_CACHE.pop(next(iter(_DT_CACHE)))
    _DT_CACHE[key] = (dt, tabs_list)
    return dt


def new_minmax(device, nmin=1, nmax=1):
    mm = torch.empty(nmin + nmax, dtype=torch.int32, device=device)
    _lib.check(_lib.load().fsg_minmax_init(_p(mm), nmin, nmax, _stream(mm)), "fsg_minmax_init")
    return mm


def key_to_float(key: int) -> float:
    return float(_lib.load().fsg_key_to_float(int(key)))


# ---- RNG / K1 ---------------------------------------------------------------------------------
def randn(shape, seed: int, stream_id: int, device) -> torch.Tensor:
    out = torch.empty(tuple(shape), dtype=F32, device=device)
    _need_gpu(out)
    _lib.check(_lib.load().fsg_randn_f32(_p(out), out.numel(), seed, stream_id, _stream(out)), "fsg_randn_f32")
    return out


def gmm_sample(labels, mus, sigmas, noise=None, seed=0, stream_id=0) -> torch.Tensor:
    _need_gpu(labels, mus, sigmas, noise)
    _f32(mus), _f32(sigmas)
    ntab = int(mus.numel())
    if sigmas.numel() != ntab or not (0 < ntab <= 256):
        raise ValueError("mus/sigmas must have the same length in 1..256")
    if noise is not None and (_f32(noise).numel() != labels.numel()):
        raise ValueError("noise must match labels")
    out = torch.empty(labels.shape, dtype=F32, device=labels.device)
    lib = _lib.load()
    if labels.dtype == torch.uint8:
        fn, name = lib.fsg_gmm_sample_u8, "fsg_gmm_sample_u8"
    elif labels.dtype == torch.int64:
        fn, name = lib.fsg_gmm_sample_i64, "fsg_gmm_sample_i64"
    else:
        raise TypeError("labels must be uint8 or int64")
    _lib.check(fn(_p(labels), labels.numel(), _p(mus), _p(sigmas), ntab, _p(noise), seed, stream_id, _p(out),
                  _stream(out)), name)
    return out


def _gmm_tables(mus, sigmas) -> int:
    """The table length the kernels are told: they read `ntab` entries of BOTH tables, so the two must agree (host check, before
    anything could be launched)."""
    ntab = int(mus.numel())
    if sigmas.numel() != ntab or not (0 < ntab <= 256):
        raise ValueError("mus/sigmas must have the same length in 1..256")
    return ntab


def gmm_sample_parts(parts, mus, sigmas, noise=None, seed=0, stream_id=0) -> torch.Tensor:
    """GMM draw from the per-meta-label seed volumes (uint8, disjoint supports) without summing them."""
    parts = [p for p in parts if p is not None]
    if not 1 <= len(parts) <= 4:
        raise ValueError("1..4 label volumes expected")
    _gmm_tables(mus, sigmas)
    _need_gpu(*parts, mus, sigmas, noise)
    for p in parts:
        if p.dtype != torch.uint8 or p.shape != parts[0].shape:
            raise TypeError("label parts must be uint8 volumes of one shape")
    _f32(mus), _f32(sigmas)
    ntab = int(mus.numel())
    if noise is not None and _f32(noise).numel() != parts[0].numel():
        raise ValueError("noise must match labels")
    out = torch.empty(parts[0].shape, dtype=F32, device=parts[0].device)
    ptrs = [_p(p) for p in parts] + [C.c_void_p(0)] * (4 - len(parts))
    _lib.check(_lib.load().fsg_gmm_sample_u8x4(*ptrs, out.numel(), _p(mus), _p(sigmas), ntab, _p(noise), seed,
                                               stream_id, _p(out), _stream(out)), "fsg_gmm_sample_u8x4")
    return out


def sample_head(parts, mus, sigmas, spec: "DeformSpec", bias=None, bias_tabs=None, noise=None, seed=0, stream_id=0,
                mm3=None):
    """Head of a sample as one launch (fsg_sample_head_f32): the GMM draw of `gmm_sample_parts`, the per-row coarse values of
    `DeformSpec.prepare_rows` and the first floor(min) pass of `coords_floormin`.  `mm3` must hold initialised keys
    (`new_minmax(dev, 3, 0)` when omitted); `coords_floormin_rest` completes them.  Returns (image, mm3); the rows are
    attached to `spec` as `prepare_rows` would."""
    parts = [p for p in parts if p is not None]
    if not 1 <= len(parts) <= 4:
        raise ValueError("1..4 label volumes expected")
    _gmm_tables(mus, sigmas)
    _need_gpu(*parts, mus, sigmas, noise)
    out = torch.empty(parts[0].shape, dtype=F32, device=parts[0].device)
    if mm3 is None:
        mm3 = new_minmax(out.device, 3, 0)
    need = 3 * int(spec.c.field_dims[2]) + (int(bias.shape[2]) if bias is not None else 0)
    stride = (max(need, 1) + 3) // 4 * 4
    rows = torch.empty(spec.shape[0] * spec.shape[1] * stride, dtype=F32, device=out.device)
    epi = _epilogue(None, bias, bias_tabs, spec.shape)
    spec.c.rows, spec.c.row_stride = None, 0
    ptrs = [_p(p) for p in parts] + [C.c_void_p(0)] * (4 - len(parts))
    _lib.check(_lib.load().fsg_sample_head_f32(*ptrs, out.numel(), _p(mus), _p(sigmas), int(mus.numel()), _p(noise), seed,
                                               stream_id, _p(out), C.byref(spec.c), C.byref(epi), _p(rows), stride,
                                               _p(mm3), _stream(out)), "fsg_sample_head_f32")
    spec.c.rows, spec.c.row_stride = rows.data_ptr(), stride
    spec._keep.append(rows)
    spec._rows_bias = int(bias.shape[2]) if bias is not None else 0
    return out, mm3


def coords_floormin_rest(spec: "DeformSpec", mm3) -> torch.Tensor:
    """Conditional full pass that completes the floor(min) keys after `sample_head` (fsg_coords_floormin_rest_f32)."""
    _lib.check(_lib.load().fsg_coords_floormin_rest_f32(C.byref(spec.c), _p(mm3), _stream(mm3)),
               "fsg_coords_floormin_rest_f32")
    return mm3


def label_stats(labels_u8, values, nlabels: int):
    """(count int64[nlabels], mean f64, var f64) per label -- wave-level reductions on the device."""
    _need_gpu(labels_u8, values)
    if labels_u8.dtype != torch.uint8 or labels_u8.numel() != _f32(values).numel():
        raise TypeError("labels uint8 and values float32 of equal size expected")
    dev = values.device
    cnt = torch.zeros(nlabels, dtype=torch.int64, device=dev)
    s1 = torch.zeros(nlabels, dtype=torch.float64, device=dev)
    s2 = torch.zeros(nlabels, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().fsg_label_stats_u8(_p(labels_u8), _p(values), values.numel(), nlabels, _p(cnt), _p(s1),
                                              _p(s2), _stream(values)), "fsg_label_stats_u8")
    n = cnt.clamp(min=1).double()
    mean = s1 / n
    return cnt, mean, s2 / n - mean * mean


# ---- zoom family --------------------------------------------------------------------------------
def _zoom_args(src, tabs: DeviceTables, nch=1):
    _need_gpu(src)
    _f32(src)
    if nch == 1:
        sx, sy, sz = _dims3(src)
    else:
        if src.dim() != 4 or src.shape[3] != nch:
            raise ValueError("channel-last 4-D source expected")
        sx, sy, sz = (int(v) for v in src.shape[:3])
    return sx, sy, sz


def zoom3d(src, tabs: DeviceTables) -> torch.Tensor:
    nch = 1 if src.dim() == 3 else int(src.shape[3])
    if nch not in (1, 3):
        raise ValueError("1 or 3 channels supported")
    sx, sy, sz = _zoom_args(src, tabs, nch)
    dx, dy, dz = tabs.lengths
    shape = (dx, dy, dz) if nch == 1 else (dx, dy, dz, nch)
    dst = torch.empty(shape, dtype=F32, device=src.device)
    tx, ty, tz = tabs.ptrs
    _lib.check(_lib.load().fsg_zoom3d_f32(_p(src), sx, sy, sz, nch, tx, ty, tz, _p(dst), dx, dy, dz, _stream(src)),
               "fsg_zoom3d_f32")
    return dst


def resample_noise(src, tabs: DeviceTables, noise_std=0.0, noise=None, seed=None, stream_id=0) -> torch.Tensor:
    sx, sy, sz = _zoom_args(src, tabs)
    dx, dy, dz = tabs.lengths
    dst = torch.empty((dx, dy, dz), dtype=F32, device=src.device)
    mode = 0
    if noise is not None:
        _need_gpu(noise)
        if _f32(noise).numel() != dst.numel():
            raise ValueError("noise size")
        mode = 1
    elif seed is not None:
        mode = 2
    tx, ty, tz = tabs.ptrs
    _lib.check(_lib.load().fsg_resample_noise_f32(_p(src), sx, sy, sz, tx, ty, tz, _p(dst), dx, dy, dz, mode,
                                                  _p(noise), seed or 0, stream_id, float(noise_std), _stream(src)),
               "fsg_resample_noise_f32")
    return dst


def zoom_minmax(src, tabs: DeviceTables, mm=None) -> torch.Tensor:
    sx, sy, sz = _zoom_args(src, tabs)
    dx, dy, dz = tabs.lengths
    if mm is None:
        mm = new_minmax(src.device)
    tx, ty, tz = tabs.ptrs
    _lib.check(_lib.load().fsg_zoom3d_minmax_f32(_p(src), sx, sy, sz, tx, ty, tz, dx, dy, dz, _p(mm), _stream(src)),
               "fsg_zoom3d_minmax_f32")
    return mm


MM_SLOT_STRIDE = _lib.MM_SLOT_STRIDE


def zoom_minmax_sharded(src, tabs: DeviceTables, nslots: int = 32) -> torch.Tensor:
    """K9 pass A with the two keys sharded over `nslots` slots (nslots x 16 int32; what fsg_sample_run uses): a workgroup
    updates slot (its index % nslots), `zoom_normalise` reduces the slots."""
    sx, sy, sz = _zoom_args(src, tabs)
    dx, dy, dz = tabs.lengths
    init = np.zeros((nslots, MM_SLOT_STRIDE), dtype=np.int32)
    init[:, 0], init[:, 1] = 0x7F800000, -2139095041  # key(+inf), key(-inf)
    slots = torch.from_numpy(init).to(src.device)
    tx, ty, tz = tabs.ptrs
    _lib.check(_lib.load().fsg_zoom3d_minmax_sharded_f32(_p(src), sx, sy, sz, tx, ty, tz, dx, dy, dz, _p(slots), nslots,
                                                         _stream(src)), "fsg_zoom3d_minmax_sharded_f32")
    return slots


def zoom_normalise(src, tabs: DeviceTables, mm, mode: int) -> torch.Tensor:
    """`mm`: the two keys of `zoom_minmax`, or the (nslots, 16) slots of `zoom_minmax_sharded`."""
    sx, sy, sz = _zoom_args(src, tabs)
    _need_gpu(mm)
    dx, dy, dz = tabs.lengths
    dst = torch.empty((dx, dy, dz), dtype=F32, device=src.device)
    tx, ty, tz = tabs.ptrs
    if mm.dim() == 2 and mm.shape[1] == MM_SLOT_STRIDE:
        _lib.check(_lib.load().fsg_zoom3d_normalise_sharded_f32(_p(src), sx, sy, sz, tx, ty, tz, _p(dst), dx, dy, dz,
                                                                _p(mm), int(mm.shape[0]), mode, _stream(src)),
                   "fsg_zoom3d_normalise_sharded_f32")
        return dst
    _lib.check(_lib.load().fsg_zoom3d_normalise_f32(_p(src), sx, sy, sz, tx, ty, tz, _p(dst), dx, dy, dz, _p(mm),
                                                    mode, _stream(src)), "fsg_zoom3d_normalise_f32")
    return dst


# ---- deformation ----------------------------------------------------------------------------------
class DeformSpec:
    """Host-side description of one spatial deformation + its device-resident small arrays."""

    def __init__(self, shape, A32, centre32, c2_32, flip, field_small=None, field_tabs=None, device=None):
        self.shape = tuple(int(v) for v in shape)
        self.device = device
        d = _lib.Deform()
        d.shape[:] = self.shape
        d.A[:] = np.asarray(A32, dtype=np.float32).reshape(-1).tolist()
        d.centre[:] = np.asarray(centre32, dtype=np.float32).tolist()
        d.c2[:] = np.asarray(c2_32, dtype=np.float32).tolist()
        d.flip = int(bool(flip))
        self._keep = []
        if field_small is not None:
            _need_gpu(field_small)
            _f32(field_small)
            if field_small.dim() != 4 or field_small.shape[3] != 3:
                raise ValueError("coarse field must be (s0,s1,s2,3)")
            if field_tabs.lengths != self.shape:
                raise ValueError("field tables must have the grid's lengths")
            d.field_dims[:] = [int(v) for v in field_small.shape[:3]]
            d.field = field_small.data_ptr()
            tx, ty, tz = field_tabs.ptrs
            d.tx, d.ty, d.tz = tx.value, ty.value, tz.value
            self._keep += [field_small, field_tabs]
        else:
            d.field_dims[:] = [0, 0, 0]
        d.rows, d.row_stride = None, 0
        self.c = d

    def prepare_rows(self, bias=None, bias_tabs=None):
        """Precompute the per-(x,y) coarse rows (displacement, and bias when it will be fused into the
        warp) into a workspace; later min/max and warp launches start each row with one coalesced load."""
        f2 = int(self.c.field_dims[2])
        b2 = int(bias.shape[2]) if bias is not None else 0
        need = 3 * f2 + b2
        if need == 0 or need > 512:
            return self
        stride = (need + 3) // 4 * 4
        rows = torch.empty(self.shape[0] * self.shape[1] * stride, dtype=F32, device=self.device)
        epi = _epilogue(None, bias, bias_tabs, self.shape)
        _lib.check(_lib.load().fsg_deform_rows_f32(C.byref(self.c), C.byref(epi), _p(rows), stride, _stream(rows)),
                   "fsg_deform_rows_f32")
        self.c.rows, self.c.row_stride = rows.data_ptr(), stride
        self._keep.append(rows)
        self._rows_bias = b2
        return self


def _epilogue(gamma, bias, bias_tabs, shape):
    epi = _lib.Epilogue()
    epi.gamma = float(np.float32(gamma)) if gamma is not None else 0.0
    if bias is not None:
        _need_gpu(bias)
        _f32(bias)
        if bias_tabs.lengths != tuple(shape):
            raise ValueError("bias tables must have the grid's lengths")
        epi.bias_dims[:] = _dims3(bias)
        epi.bias = bias.data_ptr()
        bx, by, bz = bias_tabs.ptrs
        epi.bx, epi.by, epi.bz = bx.value, by.value, bz.value
    return epi


def coords_minmax(spec: DeformSpec) -> torch.Tensor:
    mm6 = new_minmax(spec.device, 3, 3)
    _lib.check(_lib.load().fsg_coords_minmax_f32(C.byref(spec.c), _p(mm6), _stream(mm6)), "fsg_coords_minmax_f32")
    return mm6


def coords_floormin(spec: DeformSpec, mm3=None) -> torch.Tensor:
    """Keys whose floor is floor(min coordinate) per axis (faces first, full pass only if needed)."""
    if mm3 is None:
        mm3 = new_minmax(spec.device, 3, 0)
    rc = _lib.load().fsg_coords_floormin_f32(C.byref(spec.c), _p(mm3), _stream(mm3))
    if rc == _lib.E_TOOBIG:
        return coords_minmax(spec)
    _lib.check(rc, "fsg_coords_floormin_f32")
    return mm3


def coords(spec: DeformSpec, mm6):
    out = [torch.empty(spec.shape, dtype=F32, device=spec.device) for _ in range(3)]
    _lib.check(_lib.load().fsg_coords_f32(C.byref(spec.c), _p(mm6), _p(out[0]), _p(out[1]), _p(out[2]), _stream(mm6)),
               "fsg_coords_f32")
    return out


def warp(spec: DeformSpec, mm6, src_lin=None, src_nn=None, gamma=None, bias=None, bias_tabs=None, nn_out=None, src_img=None):
    """Fused warp: returns (out_lin | None, out_nn | None), and (out_lin, out_nn | None, out_img) when `src_img` is given.

    `src_nn` float32 -> float32 labels (reference contract); uint8 -> uint8, or float32 when
    `nn_out=torch.float32` (uint8 device copy of a float32 segmentation, exact for 0..255).
    `src_img`: a second float32 volume sampled trilinearly at `src_lin`'s positions in the same launch, without the
    gamma / bias epilogue (fsg_warp_dual_f32); outside the lean kernel's domain it is a second launch, same values."""
    _need_gpu(mm6, src_lin, src_nn, bias)
    if src_img is not None:
        return _warp_dual(spec, mm6, src_lin, src_nn, gamma, bias, bias_tabs, nn_out, src_img)
    for s_ in (src_lin, src_nn):
        if s_ is not None and tuple(s_.shape) != spec.shape:
            raise ValueError(f"volume shape {tuple(s_.shape)} != grid {spec.shape}")
    out_lin = torch.empty_like(_f32(src_lin)) if src_lin is not None else None
    epi = _epilogue(gamma, bias, bias_tabs, spec.shape)
    if spec.c.rows and (int(bias.shape[2]) if bias is not None else 0) > getattr(spec, "_rows_bias", 0):
        raise ValueError("row workspace was prepared without this bias grid; call prepare_rows(bias, bias_tabs)")
    lib = _lib.load()
    args = lambda src, out: (C.byref(spec.c), _p(mm6), _p(src_lin), _p(out_lin), _p(src), _p(out), C.byref(epi),
                             _stream(mm6))
    if src_nn is None or src_nn.dtype == F32:
        out_nn = torch.empty_like(src_nn) if src_nn is not None else None
        _lib.check(lib.fsg_warp_f32(*args(src_nn, out_nn)), "fsg_warp_f32")
    elif src_nn.dtype == torch.uint8:
        if nn_out in (None, torch.uint8):
            out_nn = torch.empty_like(src_nn)
            _lib.check(lib.fsg_warp_f32_u8(*args(src_nn, out_nn)), "fsg_warp_f32_u8")
        elif nn_out == F32:
            out_nn = torch.empty(src_nn.shape, dtype=F32, device=src_nn.device)
            rc = lib.fsg_warp_f32_u8_to_f32(*args(src_nn, out_nn))
            if rc == _lib.E_ALIGN:  # outside the lean kernel's domain: float32 label volume through fsg_warp_f32
                _lib.check(lib.fsg_warp_f32(*args(src_nn.to(F32), out_nn)), "fsg_warp_f32")
            else:
                _lib.check(rc, "fsg_warp_f32_u8_to_f32")
        else:
            raise TypeError("nn_out must be torch.uint8 or torch.float32")
    else:
        raise TypeError("nearest-neighbour volume must be float32 or uint8")
    return out_lin, out_nn


def _warp_dual(spec, mm6, src_lin, src_nn, gamma, bias, bias_tabs, nn_out, src_img):
    _need_gpu(src_img)
    if src_lin is None:
        raise ValueError("src_img rides on src_lin's sampling positions: src_lin is required")
    for s_ in (src_lin, src_nn, src_img):
        if s_ is not None and tuple(s_.shape) != spec.shape:
            raise ValueError(f"volume shape {tuple(s_.shape)} != grid {spec.shape}")
    if src_nn is not None and src_nn.dtype not in (F32, torch.uint8):
        raise TypeError("nearest-neighbour volume must be float32 or uint8")
    if nn_out not in (None, torch.uint8, F32) or (nn_out == torch.uint8 and src_nn is not None and src_nn.dtype == F32):
        raise TypeError("nn_out must be torch.uint8 or torch.float32 (float32 labels stay float32)")
    if spec.c.rows and (int(bias.shape[2]) if bias is not None else 0) > getattr(spec, "_rows_bias", 0):
        raise ValueError("row workspace was prepared without this bias grid; call prepare_rows(bias, bias_tabs)")
    out_lin, out_img = torch.empty_like(_f32(src_lin)), torch.empty_like(_f32(src_img, "src_img"))
    out_nn, din, dout = None, _lib.LABEL_F32, _lib.LABEL_F32
    if src_nn is not None:
        odt = src_nn.dtype if nn_out is None else nn_out
        out_nn = torch.empty(src_nn.shape, dtype=odt, device=src_nn.device)
        din = _lib.LABEL_U8 if src_nn.dtype == torch.uint8 else _lib.LABEL_F32
        dout = _lib.LABEL_U8 if odt == torch.uint8 else _lib.LABEL_F32
    epi = _epilogue(gamma, bias, bias_tabs, spec.shape)
    rc = _lib.load().fsg_warp_dual_f32(C.byref(spec.c), _p(mm6), _p(src_lin), _p(out_lin), _p(src_img), _p(out_img),
                                       src_img.numel(), _p(src_nn), _p(out_nn), din, dout, C.byref(epi), _stream(mm6))
    if rc == _lib.E_ALIGN:  # outside the lean kernel's domain: the two launches it stands for
        out_lin, out_nn = warp(spec, mm6, src_lin=src_lin, src_nn=src_nn, gamma=gamma, bias=bias, bias_tabs=bias_tabs, nn_out=nn_out)
        out_img, _ = warp(spec, mm6, src_lin=src_img)
        return out_lin, out_nn, out_img
    _lib.check(rc, "fsg_warp_dual_f32")
    return out_lin, out_nn, out_img


def interp3d(src, ii, jj, kk, mode: str, default_value=0.0) -> torch.Tensor:
    _need_gpu(src, ii, jj, kk)
    sx, sy, sz = _dims3(_f32(src))
    if not (ii.shape == jj.shape == kk.shape):
        raise ValueError("coordinate shapes differ")
    for c in (ii, jj, kk):
        _f32(c)
    if mode not in ("linear", "nearest"):
        raise Exception("mode must be linear or nearest")
    dst = torch.empty(ii.shape, dtype=F32, device=src.device)
    _lib.check(_lib.load().fsg_interp3d_f32(_p(src), sx, sy, sz, _p(ii), _p(jj), _p(kk), ii.numel(),
                                            1 if mode == "nearest" else 0, float(default_value), _p(dst), _stream(src)),
               "fsg_interp3d_f32")
    return dst


# ---- pointwise / blur / reductions ------------------------------------------------------------
def gamma(x, g: float) -> torch.Tensor:
    _need_gpu(x)
    out = torch.empty_like(_f32(x))
    _lib.check(_lib.load().fsg_gamma_f32(_p(x), x.numel(), float(np.float32(g)), _p(out), _stream(x)), "fsg_gamma_f32")
    return out


def cast_f16(x) -> torch.Tensor:
    """float32 -> float16 copy (round to nearest even) by fsg_cast_f32_to_f16: the optional half-precision image."""
    _need_gpu(x)
    x = _f32(x).contiguous()
    out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().fsg_cast_f32_to_f16(_p(x), x.numel(), _p(out), _stream(x)), "fsg_cast_f32_to_f16")
    return out


def bias_mul(x, bias, bias_tabs: DeviceTables) -> torch.Tensor:
    _need_gpu(x, bias)
    nx, ny, nz = _dims3(_f32(x))
    b0, b1, b2 = _dims3(_f32(bias))
    if bias_tabs.lengths != (nx, ny, nz):
        raise ValueError("bias tables must have the volume's lengths")
    out = torch.empty_like(x)
    bx, by, bz = bias_tabs.ptrs
    _lib.check(_lib.load().fsg_bias_mul_f32(_p(x), nx, ny, nz, _p(bias), b0, b1, b2, bx, by, bz, _p(out), _stream(x)),
               "fsg_bias_mul_f32")
    return out


def add_noise(x, noise_std: float, noise=None, seed=0, stream_id=0) -> torch.Tensor:
    _need_gpu(x, noise)
    out = torch.empty_like(_f32(x))
    if noise is not None and _f32(noise).numel() != x.numel():
        raise ValueError("noise size")
    _lib.check(_lib.load().fsg_add_noise_f32(_p(x), x.numel(), _p(noise), seed, stream_id, float(noise_std), _p(out),
                                             _stream(x)), "fsg_add_noise_f32")
    return out


def blur_axis(x, axis: int, taps: np.ndarray, force_generic=False) -> torch.Tensor:
    _need_gpu(x)
    nx, ny, nz = _dims3(_f32(x))
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    if taps.ndim != 1 or len(taps) % 2 == 0:
        raise ValueError("odd number of taps expected")
    out = torch.empty_like(x)
    lib = _lib.load()
    rc = _lib.E_ALIGN
    if not force_generic and len(taps) <= 129:
        rc = lib.fsg_blur_axis_taps_host_f32(_p(x), _p(out), nx, ny, nz, axis,
                                             taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps), _stream(x))
    if rc == _lib.E_ALIGN:  # shape not covered by the tuned kernels -> generic kernel (still HIP)
        tdev = torch.from_numpy(taps).to(x.device)
        rc = lib.fsg_blur_axis_f32(_p(x), _p(out), nx, ny, nz, axis, _p(tdev), len(taps), _stream(x))
    _lib.check(rc, "fsg_blur_axis")
    return out


def blur_yz(x, taps_y: np.ndarray, taps_z: np.ndarray):
    """Axis-1 then axis-2 blur in one launch (fsg_blur_yz_taps_host_f32); None when the shape / radii are outside the
    fused kernel's domain (the caller then runs the two single-axis passes)."""
    _need_gpu(x)
    nx, ny, nz = _dims3(_f32(x))
    ty = np.ascontiguousarray(taps_y, dtype=np.float32)
    tz = np.ascontiguousarray(taps_z, dtype=np.float32)
    out = torch.empty_like(x)
    fp = C.POINTER(C.c_float)
    rc = _lib.load().fsg_blur_yz_taps_host_f32(_p(x), _p(out), nx, ny, nz, ty.ctypes.data_as(fp), len(ty),
                                               tz.ctypes.data_as(fp), len(tz), _stream(x))
    if rc == _lib.E_ALIGN:
        return None
    _lib.check(rc, "fsg_blur_yz_taps_host_f32")
    return out


def blur_resample(x, tabs: DeviceTables, taps, noise_std=0.0, noise=None, seed=None, stream_id=0, keep_mid=False):
    """K6 + K7 (+ K8) as the fused pair of launches (fsg_blur_resample_x_f32, fsg_blur_resample_yz_noise_f32): `taps` = the
    three per-axis Gaussian tap arrays.  None when the configuration is outside the fused kernels' domain: shapes and radii
    (fsg_blur_resample_supported), tables that are not down-sampling tables of these axes, an input not 16-byte aligned."""
    _need_gpu(x, noise)
    n0, n1, n2 = _dims3(_f32(x))
    m0, m1, m2 = tabs.lengths
    if not all(tabs.down) or any(r > n for r, n in zip(tabs.reach, (n0, n1, n2))) or x.data_ptr() & 15:
        return None
    tp = [np.ascontiguousarray(t, dtype=np.float32) for t in taps]
    lib = _lib.load()
    if not lib.fsg_blur_resample_supported(n0, n1, n2, m0, m1, m2, len(tp[0]), len(tp[1]), len(tp[2])):
        return None
    fp = C.POINTER(C.c_float)
    mid = torch.empty((m0, n1, n2), dtype=F32, device=x.device)
    out = torch.empty((m0, m1, m2), dtype=F32, device=x.device)
    tx, ty, tz = tabs.ptrs
    _lib.check(lib.fsg_blur_resample_x_f32(_p(x), n0, n1, n2, tx, m0, tp[0].ctypes.data_as(fp), len(tp[0]), _p(mid), _stream(x)),
               "fsg_blur_resample_x_f32")
    mode = 0
    if noise is not None:
        if _f32(noise).numel() != out.numel():
            raise ValueError("noise size")
        mode = 1
    elif seed is not None:
        mode = 2
    _lib.check(lib.fsg_blur_resample_yz_noise_f32(_p(mid), m0, n1, n2, ty, tz, m1, m2, tp[1].ctypes.data_as(fp), len(tp[1]),
                                                  tp[2].ctypes.data_as(fp), len(tp[2]), mode, _p(noise), seed or 0, stream_id,
                                                  float(noise_std), _p(out), _stream(x)), "fsg_blur_resample_yz_noise_f32")
    return (out, mid) if keep_mid else out


def reduce_minmax(x) -> torch.Tensor:
    _need_gpu(x)
    mm = new_minmax(x.device)
    _lib.check(_lib.load().fsg_reduce_minmax_f32(_p(_f32(x)), x.numel(), _p(mm), _stream(x)), "fsg_reduce_minmax_f32")
    return mm


def scale(x, mm, mode: int) -> torch.Tensor:
    _need_gpu(x, mm)
    out = torch.empty_like(_f32(x))
    _lib.check(_lib.load().fsg_scale_f32(_p(x), x.numel(), _p(mm), mode, _p(out), _stream(x)), "fsg_scale_f32")
    return out


# ---- SR-artifact slice-stack simulation (fsg_slice_acq.hip) -------------------------------------------
SA_MODES = {"linear": _lib.SA.LINEAR, "nearest_psf": _lib.SA.NEAREST_PSF, "torch": _lib.SA.TORCH}


def _sa_mode(semantics: str, interp_psf: bool) -> int:
    if semantics == "torch":
        return SA_MODES["torch"]
    if semantics != "cuda":
        raise ValueError(f"semantics must be 'cuda' or 'torch', got {semantics!r}")
    return SA_MODES["nearest_psf"] if interp_psf else SA_MODES["linear"]


def _sa_mask(m, shape, name, device=None):
    """`_mask`, for the entries whose callers hand an empty tensor for "no mask" as the reference's do"""
    return None if m is None or m.numel() == 0 else _mask(m, name, tuple(shape), device)


def _sa_common(transforms, psf):
    _need_gpu(transforms, psf)
    _f32(transforms, "transforms"), _f32(psf, "psf")
    if transforms.dim() != 3 or tuple(transforms.shape[1:]) != (3, 4):
        raise ValueError(f"transforms must be (n,3,4), got {tuple(transforms.shape)}")
    if psf.dim() != 3:
        raise ValueError(f"psf must be 3-D, got {tuple(psf.shape)}")
    return int(transforms.shape[0]), tuple(int(v) for v in psf.shape)


def slice_acq_forward(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight=False,
                      interp_psf=False, semantics="cuda"):
    """(n,3,4) transforms x (D,H,W) volume -> (n,h,w) slices [, weights]  (fsg_slice_acq_forward_f32)."""
    n, (pd, ph, pw) = _sa_common(transforms, psf)
    _need_gpu(vol)
    D, H, W = _dims3(_f32(vol, "vol"))
    h, w = int(slice_shape[0]), int(slice_shape[1])
    vm, sm = _sa_mask(vol_mask, (D, H, W), "vol_mask"), _sa_mask(slices_mask, (n, h, w), "slices_mask")
    out = torch.empty((n, h, w), dtype=F32, device=vol.device)
    wgt = torch.empty_like(out) if need_weight else None
    rc = _lib.load().fsg_slice_acq_forward_f32(_p(transforms), _p(vol), _p(vm), _p(psf), pd, ph, pw, _p(sm), _p(out),
                                               _p(wgt), D, H, W, n, h, w, float(res_slice),
                                               _sa_mode(semantics, interp_psf), _stream(vol))
    _lib.check(rc, "fsg_slice_acq_forward_f32")
    return (out, wgt) if need_weight else out


def slice_acq_backward(transforms, vol, vol_mask, slices_mask, psf, grad_slices, res_slice, interp_psf=False,
                       need_vol_grad=True, need_transforms_grad=True, deterministic=False, grad_scale=1.0):
    """Backward of `slice_acq_forward` in the CUDA semantics (fsg_slice_acq_backward_f32): (n,h,w) grad_slices ->
    (grad_vol (D,H,W) | None, grad_transforms (n,3,4) | None).  grad_transforms is reduced in a fixed order and is bit-identical
    for the same inputs.  grad_vol is accumulated with fp32 atomics (its last bits change from run to run) unless
    deterministic: then every contribution is quantised once and summed in fixed point, two 64-bit limbs
    (fsg_slice_acq_backward_det_f32), and grad_vol is a pure function of the inputs, whatever the run, the stream or the slice
    order; grad_transforms has the same bits either way.  grad_scale: a power of two in [2^-20, 2^20] the contributions are
    divided by before they are quantised (1 for gradients of about unit size)."""
    if deterministic:
        _pow2_scale(grad_scale, "grad_scale")
    if not (need_vol_grad or need_transforms_grad):
        return None, None
    n, (pd, ph, pw) = _sa_common(transforms, psf)
    _need_gpu(vol, grad_slices)
    D, H, W = _dims3(_f32(vol, "vol"))
    _f32(grad_slices, "grad_slices")
    h, w = _nhw(grad_slices, "grad_slices", n)
    vm, sm = _sa_mask(vol_mask, (D, H, W), "vol_mask"), _sa_mask(slices_mask, (n, h, w), "slices_mask")
    gvol = torch.empty((D, H, W), dtype=F32, device=vol.device) if need_vol_grad else None
    gtr = torch.empty((n, 3, 4), dtype=F32, device=vol.device) if need_transforms_grad else None
    lib = _lib.load()
    need = int(lib.fsg_slice_acq_backward_ws_bytes(n, h, w)) if need_transforms_grad else 0
    ws = torch.empty(need // 8, dtype=torch.int64, device=vol.device) if need else None  # 48 bytes per tile: a multiple of 8
    if deterministic:
        dneed = int(lib.fsg_slice_acq_backward_det_ws_bytes(D, H, W)) if need_vol_grad else 0
        dws = torch.empty(dneed // 8, dtype=torch.int64, device=vol.device) if dneed else None  # zeroed by the call
        rc = lib.fsg_slice_acq_backward_det_f32(_p(transforms), _p(vol), _p(vm), _p(psf), pd, ph, pw, _p(grad_slices), _p(sm),
                                                _p(gvol), _p(gtr), D, H, W, n, h, w, float(res_slice),
                                                _sa_mode("cuda", interp_psf), _p(ws), need, _p(dws), dneed, float(grad_scale),
                                                _stream(vol))
        _lib.check(rc, "fsg_slice_acq_backward_det_f32")
        return gvol, gtr
    rc = lib.fsg_slice_acq_backward_f32(_p(transforms), _p(vol), _p(vm), _p(psf), pd, ph, pw, _p(grad_slices), _p(sm),
                                        _p(gvol), _p(gtr), D, H, W, n, h, w, float(res_slice),
                                        _sa_mode("cuda", interp_psf), _p(ws), need, _stream(vol))
    _lib.check(rc, "fsg_slice_acq_backward_f32")
    return gvol, gtr


def slice_acq_adjoint_backward(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf=False,
                               equalize=False, vol=None, vol_weight=None, need_slices_grad=True, need_transforms_grad=True):
    """Backward of `slice_acq_adjoint` in the CUDA semantics (fsg_slice_acq_adjoint_backward_f32): (D,H,W) grad_vol ->
    (grad_slices (n,h,w) | None, grad_transforms (n,3,4) | None).  equalize: the backward of the equalised adjoint; `vol` is its
    (equalised) output and `vol_weight` its weight (`return_weight=True`).  grad_vol is never written.  Both outputs are
    gathered and reduced in a fixed order: bit-identical for the same inputs, each whether or not the other is requested."""
    if not (need_slices_grad or need_transforms_grad):
        return None, None
    if equalize and (vol is None or vol_weight is None):
        raise ValueError("equalize=True needs vol (the equalised output of the adjoint) and vol_weight")
    n, (pd, ph, pw) = _sa_common(transforms, psf)
    _need_gpu(grad_vol, slices)
    D, H, W = _dims3(_f32(grad_vol, "grad_vol"))
    _f32(slices, "slices")
    h, w = _nhw(slices, "slices", n)
    vm, sm = _sa_mask(vol_mask, (D, H, W), "vol_mask"), _sa_mask(slices_mask, (n, h, w), "slices_mask")
    if equalize:
        _need_gpu(vol, vol_weight)
        for t, name in ((vol, "vol"), (vol_weight, "vol_weight")):
            if _dims3(_f32(t, name)) != (D, H, W):
                raise ValueError(f"{name} shape {tuple(t.shape)} does not match grad_vol {(D, H, W)}")
    else:
        vol = vol_weight = None
    gsl = torch.empty((n, h, w), dtype=F32, device=grad_vol.device) if need_slices_grad else None
    gtr = torch.empty((n, 3, 4), dtype=F32, device=grad_vol.device) if need_transforms_grad else None
    lib = _lib.load()
    need = int(lib.fsg_slice_acq_adjoint_backward_ws_bytes(D, H, W, n, h, w, int(bool(equalize)), int(need_transforms_grad)))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=grad_vol.device) if need else None
    rc = lib.fsg_slice_acq_adjoint_backward_f32(_p(transforms), _p(grad_vol), _p(vol_weight), _p(vol), _p(vm), _p(psf), pd, ph,
                                                pw, _p(slices), _p(sm), _p(gsl), _p(gtr), D, H, W, n, h, w, float(res_slice),
                                                _sa_mode("cuda", interp_psf), int(bool(equalize)), _p(ws), need,
                                                _stream(grad_vol))
    _lib.check(rc, "fsg_slice_acq_adjoint_backward_f32")
    return gsl, gtr


def slice_acq_adjoint(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf=False,
                      equalize=False, semantics="cuda", return_weight=False, slice_ids=None, deterministic=False,
                      value_scale=1.0):
    """(n,h,w) slices -> (D,H,W) volume  (fsg_slice_acq_adjoint_f32 + fsg_equalize_f32).
    slice_ids (host integer tensor, len(transforms)): use slices[slice_ids[z]] for transform z (subset without a copy).
    deterministic: accumulate in fixed point, two 64-bit limbs (fsg_slice_acq_adjoint_det_f32): the result is a pure function
    of the inputs, whatever the tuning, the slice order or the run; `semantics="cuda"` only.  value_scale: a power of two in
    [2^-20, 2^20] the slice values are divided by before they are quantised (1 for slices scaled to about [0, 1])."""
    if deterministic and semantics == "torch":
        raise ValueError("the deterministic adjoint follows the CUDA semantics only (semantics='cuda')")
    if deterministic:
        _pow2_scale(value_scale, "value_scale")
    n, (pd, ph, pw) = _sa_common(transforms, psf)
    _need_gpu(slices)
    _f32(slices, "slices")
    ns = int(slices.shape[0])
    h, w = _nhw(slices, "slices", n if slice_ids is None else ns)
    if slice_ids is not None:
        # host tensor on purpose: the ids index device memory, so they are range-checked here before a kernel sees them
        if slice_ids.is_cuda or slice_ids.numel() != n:
            raise ValueError("slice_ids must be a host integer tensor with one entry per transform")
        ids = slice_ids.to(torch.int64)
        if n and (int(ids.min()) < 0 or int(ids.max()) >= ns):
            raise IndexError(f"slice_ids out of range for {ns} slices")
        slice_ids = _upload(ids.to(torch.int32).contiguous(), slices.device)
    D, H, W = (int(v) for v in vol_shape)
    vm, sm = _sa_mask(vol_mask, (D, H, W), "vol_mask"), _sa_mask(slices_mask, (ns, h, w), "slices_mask")
    vol = torch.empty((D, H, W), dtype=F32, device=slices.device)
    wgt = torch.empty_like(vol) if (equalize or return_weight) else None
    mode = _sa_mode(semantics, interp_psf)
    lib, st = _lib.load(), _stream(slices)
    if deterministic:
        need = int(lib.fsg_slice_acq_adjoint_det_ws_bytes(D, H, W, int(wgt is not None)))
        ws = torch.empty(need // 8, dtype=torch.int64, device=slices.device)  # zeroed by the call
        rc = lib.fsg_slice_acq_adjoint_det_f32(_p(transforms), _p(psf), pd, ph, pw, _p(slices), _p(sm), _p(slice_ids),
                                               _p(vm), _p(vol), _p(wgt), D, H, W, n, h, w, float(res_slice), mode, _p(ws),
                                               need, float(value_scale), st)
        _lib.check(rc, "fsg_slice_acq_adjoint_det_f32")
    else:
        rc = lib.fsg_slice_acq_adjoint_f32(_p(transforms), _p(psf), pd, ph, pw, _p(slices), _p(sm), _p(slice_ids), _p(vm),
                                           _p(vol), _p(wgt), D, H, W, n, h, w, float(res_slice), mode, st)
        _lib.check(rc, "fsg_slice_acq_adjoint_f32")
    torch_sem = mode == SA_MODES["torch"]
    if equalize or (torch_sem and vm is not None):
        rc = lib.fsg_equalize_f32(_p(vol), _p(wgt if equalize else None), _p(vm if torch_sem else None),
                                  1e-2 if torch_sem else 0.0, vol.numel(), st)
        _lib.check(rc, "fsg_equalize_f32")
    return (vol, wgt) if return_weight else vol


# ---- pose conversions (fsg_transform_convert.hip) ----------------------------------------------------------
def _tc_rows(t, name, shape):
    """`t` is a contiguous fp32 device tensor (n, *shape); returns n."""
    _need_gpu(t)
    _f32(t, name)
    if t.dim() != 1 + len(shape) or tuple(t.shape[1:]) != shape:
        raise ValueError(f"{name} must be (n,{','.join(map(str, shape))}), got {tuple(t.shape)}")
    return int(t.shape[0])


def _tc_same(n, m, a, b, ta, tb):
    """both tensors of a backward call: as many rows, and on ONE device (the output and the stream follow the second)"""
    if n != m:
        raise ValueError(f"{a} has {n} rows, {b} has {m}")
    _same_device(tb.device, b, (a, ta))


def axisangle2mat(axisangle) -> torch.Tensor:
    """(n,6) [rotation vector | translation] -> (n,3,4) [R | t]  (fsg_axisangle2mat_f32)."""
    n = _tc_rows(axisangle, "axisangle", (6,))
    mat = torch.empty((n, 3, 4), dtype=F32, device=axisangle.device)
    _lib.check(_lib.load().fsg_axisangle2mat_f32(_p(axisangle), _p(mat), n, _stream(axisangle)), "fsg_axisangle2mat_f32")
    return mat


def axisangle2mat_backward(grad_mat, axisangle) -> torch.Tensor:
    """(n,3,4) grad_mat at the (n,6) axisangle -> (n,6) grad_axisangle  (fsg_axisangle2mat_backward_f32)."""
    n = _tc_rows(axisangle, "axisangle", (6,))
    _tc_same(_tc_rows(grad_mat, "grad_mat", (3, 4)), n, "grad_mat", "axisangle", grad_mat, axisangle)
    out = torch.empty((n, 6), dtype=F32, device=axisangle.device)
    _lib.check(_lib.load().fsg_axisangle2mat_backward_f32(_p(grad_mat), _p(axisangle), _p(out), n, _stream(axisangle)),
               "fsg_axisangle2mat_backward_f32")
    return out


def mat2axisangle(mat) -> torch.Tensor:
    """(n,3,4) [R | t] -> (n,6) [rotation vector | translation]  (fsg_mat2axisangle_f32)."""
    n = _tc_rows(mat, "mat", (3, 4))
    ax = torch.empty((n, 6), dtype=F32, device=mat.device)
    _lib.check(_lib.load().fsg_mat2axisangle_f32(_p(mat), _p(ax), n, _stream(mat)), "fsg_mat2axisangle_f32")
    return ax


def mat2axisangle_backward(mat, grad_axisangle) -> torch.Tensor:
    """(n,6) grad_axisangle at the (n,3,4) mat -> (n,3,4) grad_mat, all 12 entries of a row free
    (fsg_mat2axisangle_backward_f32; the reference's rule, not the derivative for rotations of 2e-3 rad or less: DESIGN.md
    section 21)."""
    n = _tc_rows(mat, "mat", (3, 4))
    _tc_same(_tc_rows(grad_axisangle, "grad_axisangle", (6,)), n, "grad_axisangle", "mat", grad_axisangle, mat)
    out = torch.empty((n, 3, 4), dtype=F32, device=mat.device)
    _lib.check(_lib.load().fsg_mat2axisangle_backward_f32(_p(mat), _p(grad_axisangle), _p(out), n, _stream(mat)),
               "fsg_mat2axisangle_backward_f32")
    return out


# ---- conjugate gradients around the slice-acquisition operators (fsg_cg.hip) ------------------------------------
CG_RELU = _lib.CG_RELU
CG_MAX_ITER = _lib.SOLVER_MAX_ITER


class CGWorkspace(_StateBlock):
    """The device block of a solve's scalars (include/fsg_hip.h, fsg_cg_*): `buf` (int64) and, as views of it, the histories
    rr, pq (float64), alpha, beta (float32), frozen (int32), each of n_iter + 1 slots indexed by iteration."""

    def __init__(self, n: int, n_iter: int, device):
        self.n, self.n_iter = n, n_iter = int(n), _iterations("n_iter", n_iter)
        s, b = (n_iter + 1,), (min(max((n + 1023) // 1024, 1), 1024),)
        self._carve("fsg_cg_ws_bytes", (n, n_iter), device,
                    (("rr", torch.float64, s), ("pq", torch.float64, s), ("partial_rr", torch.float64, b),
                     ("partial_pq", torch.float64, b), ("alpha", F32, s), ("beta", F32, s), ("frozen", torch.int32, s)))

    def info(self):
        return {k: getattr(self, k) for k in ("rr", "pq", "alpha", "beta", "frozen")}


def cg_workspace(n: int, n_iter: int, device) -> CGWorkspace:
    return CGWorkspace(n, n_iter, device)


def _cg_vectors(ws, *named):
    """fp32 contiguous device vectors of ws.n elements each (None allowed where the entry allows it), on ws's device"""
    for name, t in named:
        if t is None:
            continue
        _need_gpu(t)
        _f32(t, name)
        if t.numel() != ws.n:
            raise ValueError(f"{name} has {t.numel()} elements, the workspace was made for {ws.n}")
    _same_device(ws.buf.device, "the workspace", *named)


def _cg_mask(ws, mask):
    return _mask(mask, "mask", ws.n, ws.buf.device)


def cg_init(ws: CGWorkspace, b, r, p, x, mask=None, mu=0.0, z=None, x0=None, t0=None):
    """r = V(b + mu z) - V(t0 + mu x0), p = r, x = V x0 or 0, partials of <r,r>  (fsg_cg_init_f32); writes r, p, x."""
    if (x0 is None) != (t0 is None):
        raise ValueError("x0 and t0 = A^T P W A x0 are given together")
    _cg_vectors(ws, ("b", b), ("r", r), ("p", p), ("x", x), ("z", z), ("x0", x0), ("t0", t0))
    mask = _cg_mask(ws, mask)
    rc = _lib.load().fsg_cg_init_f32(_p(b), _p(z), _p(t0), _p(x0), _p(mask), float(mu), ws.n, ws.n_iter, _p(r), _p(p), _p(x),
                                     _p(ws.buf), ws.nbytes, _stream(b))
    _lib.check(rc, "fsg_cg_init_f32")


def cg_q(ws: CGWorkspace, k: int, p, t, mask=None, mu=0.0, tol=0.0):
    """q = V(t + mu p) over t, partials of <p,q>  (fsg_cg_q_f32)."""
    _cg_vectors(ws, ("p", p), ("t", t))
    mask = _cg_mask(ws, mask)
    rc = _lib.load().fsg_cg_q_f32(_p(p), _p(t), _p(mask), float(mu), float(tol), ws.n, int(k), ws.n_iter, _p(ws.buf), ws.nbytes,
                                  _stream(p))
    _lib.check(rc, "fsg_cg_q_f32")


def cg_step(ws: CGWorkspace, k: int, p, q, x, r, relu=False):
    """alpha[k]; x += alpha p; r -= alpha q; partials of the new <r,r>; relu: x = max(x, 0) when k is the last iteration
    (fsg_cg_step_f32)."""
    _cg_vectors(ws, ("p", p), ("q", q), ("x", x), ("r", r))
    rc = _lib.load().fsg_cg_step_f32(_p(p), _p(q), _p(x), _p(r), ws.n, int(k), ws.n_iter, CG_RELU if relu else 0, _p(ws.buf),
                                     ws.nbytes, _stream(p))
    _lib.check(rc, "fsg_cg_step_f32")


def cg_dir(ws: CGWorkspace, k: int, r, p, tol=0.0):
    """rr[k], beta[k], frozen[k]; p = r + beta p  (fsg_cg_dir_f32)."""
    _cg_vectors(ws, ("r", r), ("p", p))
    rc = _lib.load().fsg_cg_dir_f32(_p(r), _p(p), float(tol), ws.n, int(k), ws.n_iter, _p(ws.buf), ws.nbytes, _stream(p))
    _lib.check(rc, "fsg_cg_dir_f32")


def tk1_apply(p, t, shape, lam, mask=None, guide=None, delta=None, out=None):
    """out = t + lam * L p over (D,H,W) = `shape` volumes (fsg_tk1_apply_f32): L the graph Laplacian of the 6-neighbour grid
    inside `mask`, its edges weighted by Huber's min(1, delta / |g_i - g_j|) with a `guide` g.  `out` may be `t` (in place);
    default: a new tensor.  Returns out."""
    D, H, W = (int(v) for v in shape)
    n = D * H * W
    if out is None:
        out = torch.empty_like(t)
    for name, v in (("p", p), ("t", t), ("guide", guide), ("out", out)):
        if v is None:
            continue
        _need_gpu(v)
        _f32(v, name)
        if v.numel() != n:
            raise ValueError(f"{name} has {v.numel()} elements, shape {(D, H, W)} has {n}")
    _same_device(p.device, "p", ("t", t), ("guide", guide), ("out", out))
    mask = _mask(mask, "mask", n, p.device)
    if (guide is None) != (delta is None):
        raise ValueError("guide and delta are given together")
    rc = _lib.load().fsg_tk1_apply_f32(_p(p), _p(t), _p(mask), _p(guide), 0.0 if delta is None else float(delta), float(lam),
                                       D, H, W, _p(out), _stream(p))
    _lib.check(rc, "fsg_tk1_apply_f32")
    return out


# ---- per-slice Levenberg-Marquardt slice-to-volume registration (fsg_svr.hip) -----------------------------------
SVR_MAX_ITER = _lib.SOLVER_MAX_ITER
SVR_SLOTS = _lib.SVR_SLOTS  # doubles per slice in `stats`: H (21, upper triangle), g (6), sum w e^2, sum w, m, two zeros


def svr_ws_bytes(n: int, h: int, w: int) -> int:
    return int(_lib.load().fsg_svr_ws_bytes(int(n), int(h), int(w)))


def svr_normal(transforms, jac, vol, psf, slices, slices_mask, slices_weight, res_slice, min_weight=0.5, out=None, ws=None):
    """Per-slice normal equations of e = slice_acq_forward(vol) - slices in the LINEAR geometry (fsg_svr_normal_f32):
    transforms (n,3,4), jac (n,12,6) = d transforms / d pose -> stats (n,32) float64: H = sum w J J^T (upper triangle, 21),
    g = sum w e J (6), sum w e^2, sum w, the pixel count m, two zeros.  Reduced in a fixed order without atomics: a slice's row is
    a pure function of that slice's inputs.  `out` (n,32) float64 and `ws` (int64, svr_ws_bytes(n,h,w) bytes) may be passed to
    keep a loop free of allocations."""
    n, (pd, ph, pw) = _sa_common(transforms, psf)
    _need_gpu(jac, vol, slices, slices_weight, out, ws)
    D, H, W = _dims3(_f32(vol, "vol"))
    _f32(jac, "jac"), _f32(slices, "slices")
    if tuple(jac.shape) != (n, 12, 6):
        raise ValueError(f"jac must be (n,12,6) with n={n}, got {tuple(jac.shape)}")
    h, w = _nhw(slices, "slices", n)
    sm = _sa_mask(slices_mask, (n, h, w), "slices_mask")
    if slices_weight is not None:
        _f32(slices_weight, "slices_weight")
        if tuple(slices_weight.shape) != (n, h, w):
            raise ValueError(f"slices_weight shape {tuple(slices_weight.shape)} does not match {(n, h, w)}")
    if not float(min_weight) >= 0.0:
        raise ValueError(f"min_weight must be >= 0, got {min_weight!r}")
    _same_device(vol.device, "vol", ("jac", jac), ("slices", slices), ("psf", psf), ("transforms", transforms),
                 ("slices_mask", sm), ("slices_weight", slices_weight), ("out", out), ("ws", ws))
    need = svr_ws_bytes(n, h, w)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.int64, device=vol.device)  # 128 bytes per tile
    elif ws.dtype != torch.int64 or ws.numel() * 8 < need:
        raise ValueError(f"ws must be int64 with at least {need // 8} elements")
    if out is None:
        out = torch.empty((n, SVR_SLOTS), dtype=torch.float64, device=vol.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n, SVR_SLOTS):
        raise ValueError(f"out must be float64 ({n},{SVR_SLOTS}), got {out.dtype} {tuple(out.shape)}")
    rc = _lib.load().fsg_svr_normal_f32(_p(transforms), _p(jac), _p(vol), _p(psf), pd, ph, pw, _p(slices), _p(sm),
                                        _p(slices_weight), _p(out), D, H, W, n, h, w, float(res_slice), float(min_weight),
                                        SA_MODES["linear"], _p(ws), ws.numel() * 8, _stream(vol))
    _lib.check(rc, "fsg_svr_normal_f32")
    return out


class SVRState(_StateBlock):
    """The device block of a registration's per-slice state (include/fsg_hip.h, fsg_svr_update_f32): `buf` (int64) and, as views
    of it, stats_cur (n,32), lam (n), m0 (n) float64, theta_cur (n,6) float32, frozen_now (n) int32 and the histories cost,
    lambda (float64), accepted, frozen (int32), each (n_iter + 1, n), row k for iteration slot k."""

    def __init__(self, n: int, n_iter: int, device):
        self.n, self.n_iter = n, n_iter = _slice_count(n), _iterations("n_iter", n_iter)
        s = n_iter + 1
        self._carve("fsg_svr_state_bytes", (n, n_iter), device,
                    (("stats_cur", torch.float64, (n, SVR_SLOTS)), ("lam", torch.float64, (n,)), ("m0", torch.float64, (n,)),
                     ("cost", torch.float64, (s, n)), ("lambda_hist", torch.float64, (s, n)), ("theta_cur", F32, (n, 6)),
                     ("frozen_now", torch.int32, (n,)), ("accepted", torch.int32, (s, n)), ("frozen", torch.int32, (s, n))))

    def info(self):
        return {"cost": self.cost, "lambda": self.lambda_hist, "accepted": self.accepted, "frozen": self.frozen}


def svr_state(n: int, n_iter: int, device) -> SVRState:
    return SVRState(n, n_iter, device)


def svr_update(state: SVRState, k: int, stats_trial, theta_trial, lambda0=1e-3, factor=10.0, lambda_min=1e-9, lambda_max=1e10,
               min_overlap=0.5, tol=0.0):
    """Slot k of a registration (fsg_svr_update_f32): accept or reject the trial whose normal equations are `stats_trial`
    (n,32) float64, adapt lambda, and overwrite theta_trial (n,6) with the next trial (the current pose for a frozen slice and
    for k == n_iter)."""
    _need_gpu(stats_trial, theta_trial)
    _f32(theta_trial, "theta_trial")
    if stats_trial.dtype != torch.float64 or tuple(stats_trial.shape) != (state.n, SVR_SLOTS):
        raise ValueError(f"stats_trial must be float64 ({state.n},{SVR_SLOTS}), got {stats_trial.dtype} {tuple(stats_trial.shape)}")
    if tuple(theta_trial.shape) != (state.n, 6):
        raise ValueError(f"theta_trial must be ({state.n},6), got {tuple(theta_trial.shape)}")
    _same_device(state.buf.device, "the state", ("stats_trial", stats_trial), ("theta_trial", theta_trial))
    rc = _lib.load().fsg_svr_update_f32(_p(stats_trial), _p(theta_trial), _p(state.buf), state.nbytes, state.n, int(k),
                                        state.n_iter, float(lambda0), float(factor), float(lambda_min), float(lambda_max),
                                        float(min_overlap), float(tol), _stream(theta_trial))
    _lib.check(rc, "fsg_svr_update_f32")


def _i32_rows(t, name, numel):
    """`t` is a contiguous int32 device vector of `numel` elements"""
    _need_gpu(t)
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != numel:
        raise ValueError(f"{name} must be int32 of {numel} elements, got {t.dtype} {tuple(t.shape)}")
    return t


def svr_compose(group_mat, group_jac, base, group, out=None):
    """Slices that move with their group (fsg_svr_compose_f32): group_mat (G,3,4) = [Q | d], group_jac (G,12,6) its Jacobian,
    base (n,3,4), group (n) int32 (an id outside [0, G), -1 by convention: the slice is fixed) -> transforms (n,3,4) with
    R' = Q R, t' = t + R'^T d, and jac (n,12,6) = d transforms / d the GROUP's 6 parameters (0 for a fixed slice): the operands
    of svr_normal.  `out` = (transforms, jac) may be passed to keep a loop free of allocations."""
    G = _tc_rows(group_mat, "group_mat", (3, 4))
    n = _tc_rows(base, "base", (3, 4))
    if _tc_rows(group_jac, "group_jac", (12, 6)) != G:
        raise ValueError(f"group_jac must be (G,12,6) with G={G}, got {tuple(group_jac.shape)}")
    _i32_rows(group, "group", n)
    if out is None:
        out = (torch.empty((n, 3, 4), dtype=F32, device=base.device), torch.empty((n, 12, 6), dtype=F32, device=base.device))
    tr, jac = out
    if _tc_rows(tr, "out[0]", (3, 4)) != n or _tc_rows(jac, "out[1]", (12, 6)) != n:
        raise ValueError(f"out must be ((n,3,4), (n,12,6)) with n={n}, got {tuple(tr.shape)}, {tuple(jac.shape)}")
    _same_device(base.device, "base", ("group_mat", group_mat), ("group_jac", group_jac), ("group", group), ("out[0]", tr),
                 ("out[1]", jac))
    rc = _lib.load().fsg_svr_compose_f32(_p(group_mat), _p(group_jac), _p(base), _p(group), _p(tr), _p(jac), n, G, _stream(base))
    _lib.check(rc, "fsg_svr_compose_f32")
    return tr, jac


def svr_group_reduce(stats, members, offsets, out=None):
    """A group's normal equations = the sum of its slices' (fsg_svr_group_reduce_f64): stats (n,32) float64, members int32
    slice indices, offsets (G+1) int32 into members -> gstats (G,32) float64, a group's members added in the listed order from
    +0.0 (an empty group: zeros).  No atomics: a group's row is a pure function of its members' rows."""
    _need_gpu(stats, members, offsets, out)
    if stats.dtype != torch.float64 or stats.dim() != 2 or int(stats.shape[1]) != SVR_SLOTS:
        raise ValueError(f"stats must be float64 (n,{SVR_SLOTS}), got {stats.dtype} {tuple(stats.shape)}")
    n, G = int(stats.shape[0]), int(offsets.numel()) - 1
    _i32_rows(members, "members", members.numel()), _i32_rows(offsets, "offsets", G + 1)
    if G < 1:
        raise ValueError("offsets must have G + 1 >= 2 elements")
    if out is None:
        out = torch.empty((G, SVR_SLOTS), dtype=torch.float64, device=stats.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (G, SVR_SLOTS):
        raise ValueError(f"out must be float64 ({G},{SVR_SLOTS}), got {out.dtype} {tuple(out.shape)}")
    _same_device(stats.device, "stats", ("members", members), ("offsets", offsets), ("out", out))
    rc = _lib.load().fsg_svr_group_reduce_f64(_p(stats), _p(members), _p(offsets), _p(out), n, int(members.numel()), G,
                                              _stream(stats))
    _lib.check(rc, "fsg_svr_group_reduce_f64")
    return out


# ---- outlier weights: robust-statistics EM over the residual of a reconstruction (fsg_robust.hip) -----------------
ROBUST_MAX_EM = _lib.SOLVER_MAX_ITER
ROBUST_LEVELS = {"slice": _lib.ROBUST_SLICE, "both": _lib.ROBUST_BOTH}
ROBUST_ROW = _lib.ROBUST_ROW  # doubles of a slice's row: N, sum p, sum p e^2, sum (1-p)^2, min y, max y


class RobustState(_PixelState):
    """The device blocks of one EM (include/fsg_hip.h, fsg_robust_*): `buf` (int64), the state, and as views of it consts (4:
    R, m, sigma_min, 0), rows (n,6), u (n), the histories sigma, c, mu1, mu2 (float64), frozen (int32), each of n_em + 1 slots,
    ws (n_em + 1, n) float64 and scal (2 float32: kappa, inv2var); `part` (int64) is the workspace of the per-workgroup
    partials for (h, w) slices."""

    def __init__(self, n: int, n_em: int, device, slice_shape=None):
        self.n, self.n_em = n, n_em = _slice_count(n), _iterations("n_em", n_em)
        s = n_em + 1
        self._carve_pixels("fsg_robust_state_bytes", "fsg_robust_ws_bytes", (n, n_em), device,
                           (("consts", torch.float64, (4,)), ("rows", torch.float64, (n, ROBUST_ROW)), ("u", torch.float64, (n,)),
                            ("sigma", torch.float64, (s,)), ("c", torch.float64, (s,)), ("mu1", torch.float64, (s,)),
                            ("mu2", torch.float64, (s,)), ("ws", torch.float64, (s, n)), ("scal", F32, (2,)),
                            ("frozen", torch.int32, (s,))), slice_shape)

    def info(self):
        return {k: getattr(self, k) for k in ("sigma", "c", "mu1", "mu2", "frozen", "ws", "u")}


def robust_state(n: int, n_em: int, device, slice_shape=None) -> RobustState:
    return RobustState(n, n_em, device, slice_shape)


def _pixel_arrays(state, named, slices_mask=None, min_weight=0.0):
    """named: (name, (n,h,w) fp32 contiguous device array or None), the first one present; all on the device of `state`, the
    block of a robust EM or an intensity matching -> (h, w, mask as bytes)"""
    _need_gpu(slices_mask, *(v for _, v in named))
    shape = (state.n, *_nhw(named[0][1], named[0][0], state.n))
    for name, v in named:
        if v is None:
            continue
        _f32(v, name)
        if tuple(v.shape) != shape:
            raise ValueError(f"{name} shape {tuple(v.shape)} does not match {shape}")
    _same_device(state.buf.device, "the state", *named)
    sm = _sa_mask(slices_mask, shape, "slices_mask", state.buf.device)
    if not float(min_weight) >= 0.0:
        raise ValueError(f"min_weight must be >= 0, got {min_weight!r}")
    return shape[1], shape[2], sm


def robust_estep(state: RobustState, t: int, y, s, slices_mask=None, sim_weight=None, min_weight=0.5):
    """Slot t of the EM, the pixel pass (fsg_robust_estep_f32): the posteriors p of e = y - s under the scalars update(t - 1)
    stored (p = 1 at t == 0) and one partial of the per-slice sums per workgroup, into state.part."""
    named = (("slices", y), ("simulated", s), ("sim_weight", sim_weight))
    h, w, sm = _pixel_arrays(state, named, slices_mask, min_weight)
    part = state.reserve((h, w))
    rc = _lib.load().fsg_robust_estep_f32(_p(y), _p(s), _p(sm), _p(sim_weight), float(min_weight), state.n, h, w, int(t),
                                          state.n_em, _p(state.buf), state.nbytes, _p(part), part.numel() * 8, _stream(y))
    _lib.check(rc, "fsg_robust_estep_f32")


def robust_update(state: RobustState, t: int, c0=0.9, sigma_floor=0.04, slice_floor=0.025, min_pixels=4):
    """Slot t of the EM, the scalar pass (fsg_robust_update_f32): the slices' rows, sigma, c, one sweep of the slice mixture,
    ws[t], and the kappa and inv2var of the next pixel pass.  After robust_estep(state, t, ...), on the same stream."""
    if state.part is None:
        raise ValueError("robust_update follows robust_estep: the state has no partials yet")
    h, w = state.slice_shape
    rc = _lib.load().fsg_robust_update_f32(_p(state.buf), state.nbytes, _p(state.part), state.part.numel() * 8, state.n, h, w,
                                           int(t), state.n_em, float(c0), float(sigma_floor), float(slice_floor),
                                           int(min_pixels), _stream(state.buf))
    _lib.check(rc, "fsg_robust_update_f32")


def robust_weights(state: RobustState, y, s, slices_mask=None, sim_weight=None, min_weight=0.5, level="slice", out=None):
    """out (n,h,w) fp32 = ws[n_em][k] on the pixels that take part, 0 elsewhere; level "both": times the pixel posterior
    under the last scalars (fsg_robust_weights_f32)."""
    if level not in ROBUST_LEVELS:
        raise ValueError(f"level must be one of {sorted(ROBUST_LEVELS)}, got {level!r}")
    if out is None and isinstance(y, torch.Tensor):
        out = torch.empty_like(y)
    named = (("slices", y), ("simulated", s), ("sim_weight", sim_weight), ("out", out))
    h, w, sm = _pixel_arrays(state, named, slices_mask, min_weight)
    rc = _lib.load().fsg_robust_weights_f32(_p(y), _p(s), _p(sm), _p(sim_weight), float(min_weight), state.n, h, w, state.n_em,
                                            ROBUST_LEVELS[level], _p(state.buf), state.nbytes, _p(out), _stream(y))
    _lib.check(rc, "fsg_robust_weights_f32")
    return out


# ---- slice intensity matching: per-slice scale and smooth bias field (fsg_imatch.hip) ------------------------------
IMATCH_ROW = _lib.IMATCH_ROW  # doubles of a slice's row: N, sum omega c s, sum omega c c, min y, max y
IMATCH_MAX_RADIUS = _lib.IMATCH_MAX_RADIUS  # the largest ceil(3 sigma)


class ImatchState(_PixelState):
    """The device blocks of one matching (include/fsg_hip.h, fsg_imatch_*): `buf` (int64), the state, and as views of it consts
    (4: R, floor, g, the number of ok slices), rows (n,5), raw (n), mean (n) float64, scale (n) float32, ok (n) and frozen (1)
    int32; `part` (int64) is the workspace of the per-workgroup partials and `planes` (float32, made on first use) that of the
    bias field's two passes, both for (h, w) slices."""

    def __init__(self, n: int, device, slice_shape=None):
        self.n = n = _slice_count(n)
        self.planes = None
        self._carve_pixels("fsg_imatch_state_bytes", "fsg_imatch_ws_bytes", (n,), device,
                           (("consts", torch.float64, (4,)), ("rows", torch.float64, (n, IMATCH_ROW)), ("raw", torch.float64, (n,)),
                            ("mean", torch.float64, (n,)), ("scale", F32, (n,)), ("ok", torch.int32, (n,)),
                            ("frozen", torch.int32, (1,))), slice_shape)

    def reserve(self, slice_shape):
        """the workspace for (h, w) slices; the planes of another shape go"""
        was = self.slice_shape
        part = super().reserve(slice_shape)
        if self.slice_shape != was:
            self.planes = None
        return part

    def reserve_planes(self):
        """the planes between the row and the column pass, for the slices `reserve` was given"""
        if self.planes is None:
            need = int(_lib.load().fsg_imatch_plane_bytes(self.n, *self.slice_shape))
            self.planes = torch.empty(need // 4, dtype=F32, device=self.buf.device)
        return self.planes

    def info(self):
        return {k: getattr(self, k) for k in ("scale", "ok", "frozen", "raw", "rows", "mean", "consts")}


def imatch_state(n: int, device, slice_shape=None) -> ImatchState:
    return ImatchState(n, device, slice_shape)


def imatch_sums(state: ImatchState, y, s, slices_mask=None, sim_weight=None, min_weight=0.5, weights=None, bias0=None):
    """The pixel pass (fsg_imatch_sums_f32): one partial of the per-slice sums N, sum omega c s, sum omega c c, min y, max y per
    workgroup, into state.part; c = expf(-bias0) * y, omega = `weights` (None: 1)."""
    named = (("slices", y), ("simulated", s), ("sim_weight", sim_weight), ("weights", weights), ("bias0", bias0))
    h, w, sm = _pixel_arrays(state, named, slices_mask, min_weight)
    part = state.reserve((h, w))
    rc = _lib.load().fsg_imatch_sums_f32(_p(y), _p(s), _p(sm), _p(sim_weight), float(min_weight), _p(weights), _p(bias0), state.n,
                                         h, w, _p(part), part.numel() * 8, _stream(y))
    _lib.check(rc, "fsg_imatch_sums_f32")


def imatch_scale(state: ImatchState, log_floor=0.01, min_pixels=4):
    """The scalar pass (fsg_imatch_scale_f32): the slices' rows, their gains raw, the gauge g, scale = raw / g, ok, the floor
    log_floor * (max y - min y) and frozen.  After imatch_sums(state, ...), on the same stream."""
    if state.part is None:
        raise ValueError("imatch_scale follows imatch_sums: the state has no partials yet")
    h, w = state.slice_shape
    rc = _lib.load().fsg_imatch_scale_f32(_p(state.buf), state.nbytes, _p(state.part), state.part.numel() * 8, state.n, h, w,
                                          float(log_floor), int(min_pixels), _stream(state.buf))
    _lib.check(rc, "fsg_imatch_scale_f32")


def imatch_bias(state: ImatchState, y, s, sigma, slices_mask=None, sim_weight=None, min_weight=0.5, weights=None, bias0=None,
                out=None):
    """out (n,h,w) fp32 = b1, bias0 plus the normalised Gaussian blur (sigma, in pixels) of omega * log(scale c / s) over the
    pixels above the floor, and state.mean, its weighted mean per slice (fsg_imatch_bias_f32: the row pass, the column pass and
    the means).  After imatch_scale(state), on the same stream, with the arrays imatch_sums was given."""
    if state.part is None:
        raise ValueError("imatch_bias follows imatch_sums and imatch_scale: the state has no partials yet")
    if out is None and isinstance(y, torch.Tensor):
        out = torch.empty_like(y)
    named = (("slices", y), ("simulated", s), ("sim_weight", sim_weight), ("weights", weights), ("bias0", bias0), ("out", out))
    h, w, sm = _pixel_arrays(state, named, slices_mask, min_weight)
    if (h, w) != state.slice_shape:
        raise ValueError(f"slices are {(h, w)}, the sums were taken over {state.slice_shape}")
    planes = state.reserve_planes()
    rc = _lib.load().fsg_imatch_bias_f32(_p(y), _p(s), _p(sm), _p(sim_weight), float(min_weight), _p(weights), _p(bias0),
                                         float(sigma), state.n, h, w, _p(state.buf), state.nbytes, _p(planes), planes.numel() * 4,
                                         _p(state.part), state.part.numel() * 8, _p(out), _stream(y))
    _lib.check(rc, "fsg_imatch_bias_f32")
    return out


def imatch_apply(state: ImatchState, y, bias=None, bias0=None, corrected=None):
    """-> (corrected, bias), both (n,h,w) fp32 (fsg_imatch_apply_f32).  `bias` given: it is imatch_bias's b1 and becomes
    b1 - mean on the ok slices, in place.  `bias` None (scale only): a new array, bias0 or zeros.  corrected =
    scale * expf(-bias) * y on every pixel."""
    with_bias = bias is not None
    if isinstance(y, torch.Tensor):
        bias = torch.empty_like(y) if bias is None else bias
        corrected = torch.empty_like(y) if corrected is None else corrected
    named = (("slices", y), ("bias", bias), ("bias0", bias0), ("corrected", corrected))
    h, w, _ = _pixel_arrays(state, named)
    rc = _lib.load().fsg_imatch_apply_f32(_p(y), _p(None if with_bias else bias0), _lib.IMATCH_WITH_BIAS if with_bias else
                                          _lib.IMATCH_SCALE_ONLY, state.n, h, w, _p(state.buf), state.nbytes, _p(bias),
                                          _p(corrected), _stream(y))
    _lib.check(rc, "fsg_imatch_apply_f32")
    return corrected, bias


# ---- SR-artifact volumetric helpers (fsg_artifacts.hip) ----------------------------------------------------
def _upload(host: torch.Tensor, device):
    """Small host tensor -> device through a pinned staging copy (async on the current stream)."""
    pin = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
    pin.copy_(host)
    return pin.to(device, non_blocking=True)


def mog3d(shape, centers, sigmas, device) -> torch.Tensor:
    """clamp(sum of k anisotropic Gaussians, 0, 1) on a (D,H,W) grid; centers/sigmas (k,3) in the (x0,y0,z0) order
    `mog_3d_tensor` unpacks (x pairs with the LAST axis).  Host arrays or device tensors."""
    D, H, W = (int(v) for v in shape)

    def dev(a):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.to(F32).contiguous()
        return _upload(torch.as_tensor(np.asarray(a, dtype=np.float32)).reshape(-1, 3), device)

    c, s = dev(centers), dev(sigmas)
    k = int(c.shape[0])
    if tuple(c.shape) != (k, 3) or tuple(s.shape) != (k, 3) or k == 0:
        raise ValueError("centers and sigmas must be (k,3) with k >= 1")
    out = torch.empty((D, H, W), dtype=F32, device=device)
    tab = torch.empty(k * 3 * max(D, H, W), dtype=F32, device=device)
    _lib.check(_lib.load().fsg_mog3d_f32(_p(c), _p(s), k, D, H, W, _p(tab), _p(out), _stream(out)), "fsg_mog3d_f32")
    return out


class PerlinPlan:
    """Device-resident lattices of one fractal-noise draw: per octave the gradient lattice and the per-axis
    linspace coordinates (built on the host in the reference's arithmetic, uploaded in one copy)."""

    def __init__(self, shape, octaves, device):
        # octaves: list of (grad (r0+1,r1+1,r2+1,3) fp32, [lin0, lin1, lin2] fp32, (r0,r1,r2), amplitude)
        self.shape = tuple(int(v) for v in shape)
        self.n = len(octaves)
        if not 1 <= self.n <= 8:
            raise ValueError("1..8 octaves")
        flat, offs = [], []
        pos = 0
        for g, lins, r, _amp in octaves:
            if tuple(g.shape) != (r[0] + 1, r[1] + 1, r[2] + 1, 3) or [len(v) for v in lins] != list(self.shape):
                raise ValueError("perlin octave: lattice / axis table shapes do not match")
            a = g.reshape(-1).to(F32)
            b = torch.cat([v.to(F32) for v in lins])
            offs.append((pos, pos + a.numel()))
            flat += [a, b]
            pos += a.numel() + b.numel()
        self.buf = _upload(torch.cat(flat), device)
        base = self.buf.data_ptr()
        self.grads = (C.c_void_p * self.n)(*[base + 4 * o[0] for o in offs])
        self.lins = (C.c_void_p * self.n)(*[base + 4 * o[1] for o in offs])
        self.res = (C.c_int32 * (3 * self.n))(*[int(v) for o in octaves for v in o[2]])
        self.amps = (C.c_float * self.n)(*[float(o[3]) for o in octaves])


def perlin_fractal(plan: PerlinPlan, mm=None):
    """Raw fractal noise volume + its (min,max) keys."""
    dev = plan.buf.device
    out = torch.empty(plan.shape, dtype=F32, device=dev)
    if mm is None:
        mm = new_minmax(dev, 1, 1)
    n0, n1, n2 = plan.shape
    rc = _lib.load().fsg_perlin_fractal_f32(plan.grads, plan.lins, plan.res, plan.amps, plan.n, n0, n1, n2, _p(out), _p(mm),
                                            _stream(out))
    _lib.check(rc, "fsg_perlin_fractal_f32")
    return out, mm


def blend(a, b, w, w_mm=None, increase=0.0, seg=None, noise_std=None, b_mm=None, a_mm=None, want_weight=False,
          want_out=True):
    """out = (1-w) a + w b (see fsg_blend_f32).  w_mm given: w is raw Perlin noise; noise_std given: b is the
    multi-scale noise field of StructNoise (needs b_mm, a_mm)."""
    _need_gpu(a, b, w, seg, w_mm, b_mm, a_mm)
    n = int(w.numel())
    for t_ in (a, b, seg):
        if t_ is not None and (t_.numel() != n or t_.dtype != F32):
            raise ValueError("blend operands must be float32 volumes of one size")
    out = torch.empty_like(w) if want_out else None
    w_out = torch.empty_like(w) if want_weight else None
    rc = _lib.load().fsg_blend_f32(_p(a), _p(b), _p(w), n, 1 if w_mm is not None else 0, _p(w_mm), float(increase), _p(seg),
                                   1 if noise_std is not None else 0, _p(b_mm), _p(a_mm),
                                   float(noise_std if noise_std is not None else 0.0), _p(out), _p(w_out), _stream(w))
    _lib.check(rc, "fsg_blend_f32")
    return (out, w_out) if want_weight else out


def slice_noise_(slices, threshold, sigma, noise1=None, noise2=None, seed=0, stream_id=0):
    _need_gpu(slices, noise1, noise2)
    _f32(slices, "slices")
    rc = _lib.load().fsg_slice_noise_f32(_p(slices), slices.numel(), float(threshold), float(sigma), _p(noise1), _p(noise2),
                                         int(seed), int(stream_id), _stream(slices))
    _lib.check(rc, "fsg_slice_noise_f32")
    return slices


def slice_void_(slices, slice_ids, params, ylin, xlin):
    """slices (n,h,w) modified in place on rows slice_ids; params (nvoid,7) device fp32.  slice_ids: HOST int32 tensor of
    distinct ids in [0, n) -- checked here, where they still are on the host: fsg_slice_void_f32 gives every void a workgroup
    row of its own, so two voids naming one slice would race (and an id outside the stack would write outside it)."""
    _need_gpu(slices, params, ylin, xlin)
    _f32(slices, "slices")
    n, h, w = (int(v) for v in slices.shape)
    if not isinstance(slice_ids, torch.Tensor) or slice_ids.is_cuda or slice_ids.dtype != torch.int32:
        raise TypeError("slice_void_: slice_ids must be a host int32 tensor")
    nv = int(slice_ids.numel())
    if tuple(params.shape) != (nv, 7) or ylin.numel() != h or xlin.numel() != w:
        raise ValueError("slice_void_: bad argument shapes")
    ids = slice_ids.reshape(-1).numpy()
    if nv and (ids.min() < 0 or ids.max() >= n or np.unique(ids).size != nv):
        raise ValueError("slice_void_: slice ids must be distinct and inside the stack")
    d_ids = _upload(slice_ids.reshape(-1), slices.device)
    rc = _lib.load().fsg_slice_void_f32(_p(slices), h, w, _p(d_ids), _p(params), nv, _p(ylin), _p(xlin), _stream(slices))
    _lib.check(rc, "fsg_slice_void_f32")
    return slices


def slice_sums(slices) -> torch.Tensor:
    _need_gpu(slices)
    _f32(slices, "slices")
    n = int(slices.shape[0])
    out = torch.empty(n, dtype=F32, device=slices.device)
    rc = _lib.load().fsg_slice_sums_f32(_p(slices), n, slices.numel() // n, _p(out), _stream(slices))
    _lib.check(rc, "fsg_slice_sums_f32")
    return out


NZ_BUCKET = _lib.NZ_BUCKET
_NZ_MODES = {">": 0, "==": 1, "!=": 2}


def nonzero_ranks(vol, op=">", value=0.0):
    """Number of voxels of `vol` (float32 / bool / uint8, any shape) satisfying `vol op value`, and a function mapping
    ranks (raster order among those voxels, int64 host tensor) to their coordinates, (k, vol.dim()) int64 on the host.
    One host sync for the count, one per selection."""
    _need_gpu(vol)
    lib, st = _lib.load(), _stream(vol)
    u8 = vol.dtype in (torch.bool, torch.uint8)
    if not u8:
        _f32(vol, "vol")
    n, mode = int(vol.numel()), _NZ_MODES[op]
    nb = (n + NZ_BUCKET - 1) // NZ_BUCKET
    counts = torch.empty(nb, dtype=torch.int32, device=vol.device)
    cnt_fn = lib.fsg_nonzero_count_u8 if u8 else lib.fsg_nonzero_count_f32
    sel_fn = lib.fsg_nonzero_select_u8 if u8 else lib.fsg_nonzero_select_f32
    _lib.check(cnt_fn(_p(vol), n, mode, float(value), _p(counts), st), "fsg_nonzero_count")
    ends = np.cumsum(counts.cpu().numpy().astype(np.int64))
    total = int(ends[-1]) if nb else 0
    shape = tuple(vol.shape)

    def select(ranks, flat_device=False):
        r = np.asarray(ranks, dtype=np.int64).reshape(-1)
        if r.size == 0:
            return torch.zeros((0,) if flat_device else (0, len(shape)), dtype=torch.int64,
                               device=vol.device if flat_device else "cpu")
        if r.min() < 0 or r.max() >= total:
            raise IndexError("rank out of range")
        b = np.searchsorted(ends, r, side="right")
        local = r - (ends[b] - counts_host[b])
        req = torch.from_numpy(np.stack([b, local]).astype(np.int32))
        d = _upload(req, vol.device)
        out = torch.empty(r.size, dtype=torch.int64, device=vol.device)
        _lib.check(sel_fn(_p(vol), n, mode, float(value), _p(d[0]), _p(d[1]), int(r.size), _p(out), _stream(vol)),
                   "fsg_nonzero_select")
        if flat_device:
            return out
        flat = out.cpu().numpy()
        if (flat < 0).any():
            raise RuntimeError("nonzero_select: volume changed between count and select")
        return torch.from_numpy(np.stack(np.unravel_index(flat, shape), -1).astype(np.int64))

    counts_host = np.diff(np.concatenate([[0], ends]))
    return total, select


def voxel_pick(pred, op, value, k: int, u, weight=None, out=None) -> torch.Tensor:
    """fsg_voxel_pick_* (contract in fsg_hip.h): the device tensor `out` of k + 2 int64 -- eligible voxels, distinct picks
    found, then the flat indices of the first k distinct candidates in the order of `u`, padded with -1.  `pred`: float32 /
    uint8 / bool of any shape; `u`: float64 uniforms in [0,1), host or device; `weight`: float32 of pred's size or None
    (1 per voxel).  Four launches on the current stream, no host synchronisation."""
    _need_gpu(pred, weight, out)
    u8 = pred.dtype in (torch.bool, torch.uint8)
    if not u8:
        _f32(pred, "pred")
    n, k = int(pred.numel()), int(k)
    if weight is not None and (_f32(weight, "weight").numel() != n):
        raise ValueError("weight and pred must have one size")
    if not (isinstance(u, torch.Tensor) and u.dtype == torch.float64 and u.dim() == 1):
        raise TypeError("u must be a 1-D float64 tensor")
    if not u.is_cuda:
        u = _upload(u, pred.device)
    _need_gpu(u)
    if out is None:
        out = torch.empty(max(k, 0) + 2, dtype=torch.int64, device=pred.device)
    elif out.dtype != torch.int64 or out.numel() < k + 2:
        raise ValueError("out must hold k + 2 int64")
    lib = _lib.load()
    need = int(lib.fsg_voxel_pick_ws_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=pred.device)
    fn = lib.fsg_voxel_pick_u8 if u8 else lib.fsg_voxel_pick_f32
    _lib.check(fn(_p(pred), n, _NZ_MODES[op], float(value), _p(weight), _p(u), int(u.numel()), k, _p(out), _p(ws), need,
                  _stream(pred)), "fsg_voxel_pick")
    return out


def pick_voxels(pred, op, value, k: int, u, weight=None):
    """(eligible, coords): the number of voxels with `pred op value` and weight > 0, and the coordinates, (found, pred.dim())
    int64 on the host, of the first k distinct voxels that the uniforms `u` select with probability proportional to `weight`
    (None: uniformly).  One small device -> host copy of k + 2 words."""
    got = voxel_pick(pred, op, value, k, u, weight).cpu().numpy()
    eligible, found = int(got[0]), int(got[1])
    flat = got[2:2 + found]
    return eligible, torch.from_numpy(np.stack(np.unravel_index(flat, tuple(pred.shape)), -1).astype(np.int64).reshape(found, pred.dim()))


def box_sum3d(v, k: int) -> torch.Tensor:
    """Zero-padded k x k x k box sum (the reference convolves with a ones kernel, padding k//2): three passes of the blur kernels
    with unit taps (exact for the small integers of a binary mask)."""
    ones = np.ones(int(k), np.float32)
    for axis in range(3):
        v = blur_axis(v.contiguous(), axis, ones)
    return v


def compact_values(values, pred, op=">", value=0.0):
    """values[pred op value] in raster order (device tensor) -- the boolean-mask gather, without the mask."""
    _need_gpu(values, pred)
    _f32(values, "values"), _f32(pred, "pred")
    n, mode = int(pred.numel()), _NZ_MODES[op]
    if values.numel() != n:
        raise ValueError("values and pred must have one size")
    lib = _lib.load()
    nb = (n + NZ_BUCKET - 1) // NZ_BUCKET
    counts = torch.empty(nb, dtype=torch.int32, device=pred.device)
    _lib.check(lib.fsg_nonzero_count_f32(_p(pred), n, mode, float(value), _p(counts), _stream(pred)), "fsg_nonzero_count")
    c = counts.cpu().numpy().astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(c)[:-1]]) if nb else np.zeros(0, np.int64)
    total = int(c.sum())
    out = torch.empty(total, dtype=F32, device=pred.device)
    if total:
        d = _upload(torch.from_numpy(offs.astype(np.int64)), pred.device)
        _lib.check(lib.fsg_compact_f32(_p(values), _p(pred), n, mode, float(value), _p(d), _p(out), _stream(pred)),
                   "fsg_compact_f32")
    return out


_EWISE = {"add": 0, "gt": 1, "eq": 2, "mul": 3, "mul_gt": 4, "max": 5, "sub_gt": 6, "le": 7}


def _ewise(op, a, b=None, value=0.0):
    _need_gpu(a, b)
    _f32(a, "a")
    if b is not None and (_f32(b, "b").numel() != a.numel()):
        raise ValueError("operands must have one size")
    out = torch.empty_like(a)
    _lib.check(_lib.load().fsg_ewise_f32(_p(a), _p(b), a.numel(), _EWISE[op], float(value), _p(out), _stream(a)),
               "fsg_ewise_f32")
    return out


def axpy(a, b):
    """a + b."""
    return _ewise("add", a, b)


def threshold(a, value=0.0):
    """(a > value) as float32 0/1."""
    return _ewise("gt", a, None, value)


def equals(a, value):
    return _ewise("eq", a, None, value)


def mul(a, b):
    return _ewise("mul", a, b)


def mask_mul(a, b, value=0.0):
    """a * (b > value)."""
    return _ewise("mul_gt", a, b, value)


def maximum(a, b):
    return _ewise("max", a, b)


def sub_gt(a, b, value=0.0):
    """((a - b) > value) as float32 0/1."""
    return _ewise("sub_gt", a, b, value)


def less_equal(a, value):
    return _ewise("le", a, None, value)


def distance_to_mask(mask, radius: int, metric: str) -> torch.Tensor:
    """Capped distance transform of a float 0/1 mask: squared Euclidean ("euclid2", exact where <= radius^2) or
    city block ("l1", exact where <= radius); three axis passes of fsg_dist_pass_f32."""
    _need_gpu(mask)
    n0, n1, n2 = _dims3(_f32(mask, "mask"))
    m = {"euclid2": 0, "l1": 1}[metric]
    lib, st = _lib.load(), _stream(mask)
    src, first = mask, 1
    for axis in (2, 1, 0):
        dst = torch.empty_like(mask)
        _lib.check(lib.fsg_dist_pass_f32(_p(src), _p(dst), n0, n1, n2, axis, int(radius), m, first, st), "fsg_dist_pass_f32")
        src, first = dst, 0
    return src


def boundary_mask(image, mask, mask_modif, mog, dist, n_dilate: int, want_mask=False):
    _need_gpu(image, mask, mask_modif, mog, dist)
    n = int(mask.numel())
    for t_ in (image, mask, mask_modif, mog, dist):
        if t_ is not None and (_f32(t_).numel() != n):
            raise ValueError("boundary_mask operands must have one size")
    out = torch.empty_like(mask) if image is not None else None
    mo = torch.empty_like(mask) if want_mask else None
    rc = _lib.load().fsg_boundary_mask_f32(_p(image), _p(mask), _p(mask_modif), _p(mog), _p(dist), int(n_dilate), n, _p(out),
                                           _p(mo), _stream(mask))
    _lib.check(rc, "fsg_boundary_mask_f32")
    return (out, mo) if want_mask else out


def bernoulli_keep(a, p: float, seed: int, stream_id: int = 0):
    _need_gpu(a)
    out = torch.empty_like(_f32(a))
    _lib.check(_lib.load().fsg_bernoulli_keep_f32(_p(a), a.numel(), float(p), int(seed), int(stream_id), _p(out), _stream(a)),
               "fsg_bernoulli_keep_f32")
    return out


def scatter_ones(shape, flat_idx, device):
    """Zero float volume of `shape` with ones at the flat (int64, device) indices."""
    _need_gpu(flat_idx)
    out = torch.zeros(tuple(shape), dtype=F32, device=device)
    if flat_idx.numel():
        _lib.check(_lib.load().fsg_scatter_const_f32(_p(out), out.numel(), _p(flat_idx.contiguous()), int(flat_idx.numel()),
                                                     1.0, _stream(out)), "fsg_scatter_const_f32")
    return out


# ---- regridding of real volumes (fsg_regrid.hip) -------------------------------------------------------
_LABEL_DTYPES = {torch.uint8: _lib.LABEL_U8, torch.int16: _lib.LABEL_I16, torch.float32: _lib.LABEL_F32}


def affine_resample(image, label, M, box, out_shape, fill=0.0, fill_label=0, nan_is_zero=True):
    """`fsg_affine_resample`: image (float32, trilinear) and / or label (uint8 / int16 / float32, nearest voxel) of one
    source shape through the 3x4 map `M` (output voxel index -> source voxel coordinate, rounded to float32 here) with the
    inclusive source index `box` as the inside region -> (image | None, label | None) of `out_shape`."""
    _need_gpu(image, label)
    if image is None and label is None:
        raise ValueError("give an image, a label volume or both")
    ref = image if image is not None else label
    s0, s1, s2 = _dims3(ref)
    if image is not None:
        _f32(image, "image")
    code = 0
    if label is not None:
        if label.dtype not in _LABEL_DTYPES:
            raise TypeError(f"label must be uint8, int16 or float32, got {label.dtype}")
        if label.device != ref.device or tuple(label.shape) != (s0, s1, s2):
            raise ValueError("image and label must share device and shape")
        code = _LABEL_DTYPES[label.dtype]
    Mh = np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(3, 4), dtype=np.float32)
    bh = np.ascontiguousarray(np.asarray(box).reshape(6), dtype=np.int32)
    d0, d1, d2 = (int(v) for v in out_shape)
    out = torch.empty((d0, d1, d2), dtype=F32, device=ref.device) if image is not None else None
    out_lab = torch.empty((d0, d1, d2), dtype=label.dtype, device=ref.device) if label is not None else None
    _lib.check(_lib.load().fsg_affine_resample(_p(image), _p(label), code, s0, s1, s2, Mh.ctypes.data_as(C.POINTER(C.c_float)),
                                               bh.ctypes.data_as(C.POINTER(C.c_int32)), d0, d1, d2, _p(out), _p(out_lab),
                                               float(fill), float(fill_label), 1 if nan_is_zero else 0, _stream(ref)),
               "fsg_affine_resample")
    return out, out_lab


def bbox_gt(v, threshold: float = 0.0) -> torch.Tensor:
    """`fsg_bbox_gt_f32`: device int32[6] = lo0,hi0,lo1,hi1,lo2,hi2 of `v > threshold`; empty set: lo = n, hi = -1."""
    _need_gpu(v)
    n0, n1, n2 = _dims3(_f32(v))
    box = torch.empty(6, dtype=torch.int32, device=v.device)
    _lib.check(_lib.load().fsg_bbox_gt_f32(_p(v), n0, n1, n2, float(threshold), _p(box), _stream(v)), "fsg_bbox_gt_f32")
    return box
