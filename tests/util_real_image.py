"""Shared pieces of the real-image tests: the phantom image, the oracle's stages run on exported keyed draws with an image."""
import ctypes as C

import numpy as np
import torch

from oracle import fsg_oracle as O

DEV = "cuda:0"
SHAPE = (64, 56, 72)  # the shape at which tests/test_keyed_draws.py exercises the keyed path with look-ahead
KW = dict(nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))


def phantom_image(shape, variant=0):
    """tests/test_hip_parity.py::_phantom_image, with a per-subject offset so that two subjects differ."""
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (100 * np.exp(-(g[0] ** 2 + 1.5 * g[1] ** 2 + 2 * g[2] ** 2)) + 20 * np.sin((5 + variant) * g[0] * g[1]) + 30).astype(np.float32)


def export_draws(kc, K, key):
    """(fsg_keyed_draws, the oracle's `draws=` dict) of `key`: the draws and the device block the draw kernel fills."""
    from fetalsyngen_amd import _lib
    from tests.test_keyed_draws import _export

    d = kc.draws(key)
    block = torch.empty(kc.block_bytes, dtype=torch.uint8, device=DEV)
    _lib.check(kc.lib.fsg_keyed_fill_block(kc.handle, C.byref(d), C.c_void_p(block.data_ptr()), K._stream(block)), "fill")
    torch.cuda.synchronize()
    return d, _export(kc, d, block)


def oracle_with_image(K, shape, key, seg, seeds, image, ex, cfg_kw):
    """The oracle on exported draws for a sample that carries an image.  `O.run_sample(draws=...)` takes seeds only, so the
    same stage functions are chained here in its order (oracle/fsg_oracle.py::_run_sample_injected): with seeds the synthetic
    channel is run_sample's own; without, the prior of run_sample's image branch replaces the GMM volume.  The image goes
    through `apply_deformation` on the coordinates of the same draws.  Returns dict(scaled, seg, image)."""
    cfg = O.Config(shape, **cfg_kw)
    seg_t, img_t = torch.from_numpy(seg), torch.from_numpy(image)
    dd = ex.get("deform")
    coords, flip = None, False
    if dd is not None:
        flip = bool(dd["flip"])
        field = O.nonlinear_field(dd["f_small"], shape) if dd.get("f_small") is not None else None
        ii, jj, kk, _m = O.deformation_coords(shape, cfg.size, dd["A"], dd["c2"], field)
        coords = (ii, jj, kk)
    if coords is None:
        img_w = img_t  # the generator passes the image through untouched when no deformation is drawn
    else:
        img_w, _ = O.apply_deformation(img_t, seg_t, coords, flip)
    if seeds is not None:
        r = O.run_sample(cfg, seg_t, seeds, draws=ex, noise_gmm=lambda shp: K.randn(shp, key, 1, DEV).cpu(),
                         noise_lowres=lambda shp: K.randn(shp, key, 2, DEV).cpu())
        return {"scaled": r["scaled"], "seg": r["seg"], "image": img_w}
    out = (img_t - img_t.min()) / (img_t.max() - img_t.min()) * 255
    if coords is None:
        seg_w = seg_t
    else:
        out, seg_w = O.apply_deformation(out, seg_t, coords, flip)
    if ex.get("gamma") is not None:
        out = O.gamma_transform(out, float(ex["gamma"]))
    if ex.get("bias") is not None:
        out = O.bias_multiply(out, ex["bias"])
    factors, rs = None, ex.get("resample")
    if rs is not None:
        out, factors = O.resample_down(out, cfg.resolution, np.array([1.0, 1.0, 1.0]) * float(rs["spacing"]), float(rs["u_std"]))
    if ex.get("noise_std") is not None:
        out = O.add_noise(out, np.array([ex["noise_std"]], dtype=np.float64), K.randn(tuple(out.shape), key, 2, DEV).cpu())
    out = O.resize_back(out, factors)
    return {"scaled": O.scale01(out), "seg": seg_w, "image": img_w}
