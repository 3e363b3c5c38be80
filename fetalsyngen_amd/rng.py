"""Where the two large Gaussian fields of a sample come from.

The reference draws them with `torch.randn(shape, device=device)` from the global generator of
`device` (rand_gmm.py:146-148, synthseg.py:230-232).  Two modes here:

  "reference": draw with `torch.randn(shape)` from the CPU global generator at the same point of the
               draw order and upload -- bit-identical noise to the reference's CPU path under the
               same `torch.manual_seed`; costs a 4 B/voxel host draw + PCIe copy per field.
  "device":    in-kernel Philox4x32-10; the 64-bit key of each field is taken from the CPU global
               generator (so runs are still reproducible under `torch.manual_seed`), nothing else
               touches the host.  `fsg_randn_f32` regenerates the identical field for checking.

  "keyed":     (fetalsyngen_amd/keyed.py) a sample is a function of its 64-bit key: every draw of the hot path, small and
               large, from Philox4x32-10 under that key, inside one native call.  The SR-artifact stages of such a sample keep
               their numpy / torch calls, each stage inside `keyed_scope(key, its stream)`: the global generators are seeded
               from (key, stream) for the stage and restored bit for bit afterwards, so the caller's generators are neither
               read nor advanced and a stage's draws never shift another stage's.  Random voxel picks inside a scope run on
               the device (`scoped_pick`, fsg_voxel_pick_*).  Where the fused keyed path does not apply (host label tensors,
               more than four meta-labels, stage-by-stage API) the global generators are seeded from the key and the sample is
               made as in "device" mode.

Streams of a key: 1-6 belong to the fused call; the stages own STAGE_STREAMS (blur_cortex 16, struct_noise 17,
simulate_motion 18, boundaries 19).

All SMALL draws (GMM tables, coarse displacement grid, bias grid, scalars) use numpy's / torch's CPU
global generators with the reference's calls in the reference's order in the first two modes.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

_MODE = os.environ.get("FSG_RNG", "device")
_VALID = ("reference", "device", "keyed")
STAGE_STREAMS = {"blur_cortex": 16, "struct_noise": 17, "simulate_motion": 18, "boundaries": 19}
_SCOPE = False


def get_mode() -> str:
    return _MODE


def set_mode(mode: str) -> None:
    global _MODE
    if mode not in _VALID:
        raise ValueError(f"rng mode must be one of {_VALID}")
    _MODE = mode


@contextlib.contextmanager
def use(mode: str | None):
    global _MODE
    if mode is None:
        yield
        return
    prev = _MODE
    set_mode(mode)
    try:
        yield
    finally:
        _MODE = prev


def in_keyed_scope() -> bool:
    return _SCOPE


@contextlib.contextmanager
def keyed_scope(key: int, stream: int):
    """The host draws of the block become a function of (key, stream): numpy's global generator and torch's CPU default
    generator are saved, seeded from splitmix64(key + stream * 0x9E3779B97F4A7C15), and restored bit for bit when the block
    ends, also when it raises.  Inside, the draw mode is "device" and `in_keyed_scope()` is true.  Scopes do not nest.

    The scope swaps process-global state: it is exactly as thread-safe as the stages' own use of those generators, that is,
    not at all -- one thread per process may draw while a scope is open.  DataLoader workers are processes, each with its
    own generators, so they are unaffected."""
    global _MODE, _SCOPE
    if _SCOPE:
        raise RuntimeError("keyed_scope does not nest")
    from .sharding import splitmix64

    s = splitmix64((int(key) + int(stream) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    np_state, torch_state, prev = np.random.get_state(), torch.get_rng_state(), _MODE
    _SCOPE, _MODE = True, "device"
    try:
        np.random.seed([s & 0xFFFFFFFF, s >> 32])
        torch.default_generator.manual_seed(s)  # torch.manual_seed(s) for the CPU generator; the devices' generators stay untouched
        yield
    finally:
        np.random.set_state(np_state)
        torch.set_rng_state(torch_state)
        _SCOPE, _MODE = False, prev


PICK_MAX_K = 1024  # fsg_voxel_pick_*: k <= 1024, m = 2k + 8 <= 4096


def scoped_pick(pred, op, value, k: int, weight=None) -> torch.Tensor:
    """Inside a keyed scope: the coordinates, (<= k, pred.dim()) int64 on the host, of k distinct voxels with `pred op value`,
    drawn sequentially with probability proportional to `weight` (device float32 volume; None: uniformly) -- the
    distribution of `distinct_ranks` / `multinomial_distinct`, with the O(mask) work on the device (kernels.pick_voxels).

    m = 2k + 8 float64 uniforms from the scoped torch generator per round; a second round only if the first left fewer than k
    distinct voxels.  Tiny masks (k >= eligible // 2) and k > PICK_MAX_K take the bucket-count route (`nonzero_ranks` +
    randperm, or torch.multinomial over the few eligible weights), from the scoped generator as well."""
    from . import kernels as K

    k = int(k)
    pred = pred.contiguous()
    if k <= 0:
        return torch.zeros((0, pred.dim()), dtype=torch.int64)
    eligible = None
    if k <= PICK_MAX_K:
        m = 2 * k + 8
        eligible, coords = K.pick_voxels(pred, op, value, k, torch.rand(m, dtype=torch.float64), weight)
        if len(coords) == k:
            return coords
        if eligible // 2 > k:
            seen = {tuple(c) for c in coords.tolist()}
            out = coords.tolist()
            while len(out) < k:
                _e, more = K.pick_voxels(pred, op, value, k, torch.rand(m, dtype=torch.float64), weight)
                for c in more.tolist():
                    if tuple(c) not in seen:
                        seen.add(tuple(c))
                        out.append(c)
                        if len(out) == k:
                            break
            return torch.tensor(out, dtype=torch.int64).reshape(-1, pred.dim())
    count, select = K.nonzero_ranks(pred, op, value)
    if weight is None:
        return select(distinct_ranks(count, k))
    w = torch.nan_to_num(K.compact_values(weight.contiguous(), pred.float(), op, value).cpu().double(), nan=0.0).clamp_(min=0.0)
    kk = min(k, int((w > 0).sum()))
    if kk == 0:
        return torch.zeros((0, pred.dim()), dtype=torch.int64)
    return select(torch.multinomial(w, kk))


class Field:
    """A standard-normal field that is either host values or a Philox key."""

    __slots__ = ("shape", "host", "seed", "stream_id")

    def __init__(self, shape, host=None, seed=None, stream_id=0):
        self.shape, self.host, self.seed, self.stream_id = tuple(shape), host, seed, stream_id

    def device_tensor(self, device):
        """Materialise on the device (only needed by the un-fused API paths and by tests)."""
        from . import kernels as K

        if self.host is not None:
            h = self.host.pin_memory() if torch.cuda.is_available() else self.host
            return h.to(device, non_blocking=True)
        return K.randn(self.shape, self.seed, self.stream_id, device)


def normal_field(shape, stream_id: int = 0) -> Field:
    if _MODE == "reference":
        return Field(shape, host=torch.randn(tuple(shape), dtype=torch.float32))
    key = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
    return Field(shape, seed=key, stream_id=stream_id)


def distinct_ranks(count: int, k: int) -> torch.Tensor:
    """k distinct uniform integers in [0, count) (all of them, shuffled, if k >= count).

    "reference": `torch.randperm(count)[:k]`, the reference's own draw (simulate_reco.py:662, artifacts.py:200, :566) --
    O(count) host work, count = voxels of a mask.  "device": sequential draws with rejection of repeats from the same
    CPU generator -- the same distribution, O(k) work."""
    count, k = int(count), int(k)
    if _MODE == "reference" or k >= count // 2:
        return torch.randperm(count)[:k]
    seen, out = set(), []
    while len(out) < k:
        for v in torch.randint(0, count, (2 * (k - len(out)) + 8,), dtype=torch.int64).tolist():
            if v not in seen:
                seen.add(v)
                out.append(v)
                if len(out) == k:
                    break
    return torch.tensor(out, dtype=torch.int64)


def multinomial_distinct(prob: torch.Tensor, k: int) -> torch.Tensor:
    """k distinct indices drawn sequentially with probability proportional to `prob` (host tensor, need not be normalised).

    "reference": `torch.multinomial(prob, k)` (artifacts.py:110).  "device": inverse-CDF draws with rejection of repeats
    (sequential sampling without replacement, the same distribution) -- one cumulative sum instead of torch's
    per-element exponential race."""
    if _MODE == "reference" or k >= prob.numel() // 2:
        return torch.multinomial(prob, k)
    # numpy for the million-element pass: single-threaded by construction (a torch CPU op of this size wakes the whole
    # intra-op pool, see hostenv.py); the same sequential float64 running sum as torch.cumsum(prob.double())
    cdf = np.cumsum(prob.numpy(), dtype=np.float64)
    total = float(cdf[-1])
    seen, out = set(), []
    while len(out) < k:
        u = torch.rand(2 * (k - len(out)) + 8, dtype=torch.float64).numpy() * total
        for v in np.minimum(np.searchsorted(cdf, u, side="right"), prob.numel() - 1).tolist():
            if v not in seen:
                seen.add(v)
                out.append(v)
                if len(out) == k:
                    break
    return torch.tensor(out, dtype=torch.int64)
