"""Helpers of the keyed-override tests (tests/test_keyed_overrides_host.py, tests/test_keyed_overrides_gpu.py).

`apply_overrides`: numpy restatement of what `genparams` do to a key's host draws (fsg_keyed_overrides in include/fsg_hip.h),
written on top of oracle/fsg_keyed_draws.py and independent of the C code: no draw moves, a stage is forced where the
reference's plan() methods force it, derived quantities are recomputed by the reference's arithmetic.
`export` / `oracle_sample`: hand-over of exported draws to the pinned oracle, with the per-axis spacing the oracle's injected
run does not take (the same public stage functions in the same order).
"""
import ctypes as C

import numpy as np
import torch

from oracle import fsg_keyed_draws as R
from oracle import fsg_oracle as O

DEV = "cuda:0"

DEFORM = ("deform_active", "flip", "rotations", "shears", "scalings", "A", "c2", "nonlinear", "nonlin_scale", "nonlin_std",
          "field_dims")
GAMMA = ("gamma_active", "gamma")
BIAS = ("bias_active", "bf_scale", "bf_std", "bias_dims")
RESAMPLE = ("resample_active", "spacing", "spacing3", "u_std", "stds", "low_shape", "blur_ntaps")
NOISE = ("noise_active", "noise_std", "noise_std32")
LAYOUT = ("off_field", "block_bytes")  # the field follows the bias grid in the block: both sizes move them


def all_gates(cfg: dict) -> dict:
    """`cfg` with every gate certain: `R.host_draws` of it gives the key's slot values of every stage."""
    return {**cfg, "deform_prob": 2.0, "gamma_prob": 2.0, "bias_prob": 2.0, "resample_prob": 2.0, "noise_prob": 2.0}


def apply_overrides(cfg: dict, r: dict, gp: dict) -> dict:
    """`r = R.host_draws(cfg, key)` with the genparams `gp` (None values already stripped) honoured."""
    key = r["key"]
    full = R.host_draws(all_gates(cfg), key)
    shape, res = np.array(cfg["shape"]), np.array(cfg["resolution"], dtype=np.float64)
    d = dict(r)
    if d["resample_active"]:
        d["spacing3"] = [d["spacing"]] * 3
    m2s = gp.get("selected_seeds", {}).get("mlabel2subclusters")
    if m2s is not None:
        d["subclusters"] = [int(m2s[m + 1]) for m in range(cfg["meta_labels"])]
    dp = gp.get("deform_params", {})
    if len(dp) > 0:
        ga, gn = dp.get("affine", {}), dp.get("non_rigid", {})
        d["deform_active"] = True
        d["flip"] = bool(dp["flip"]) if "flip" in dp else full["flip"]
        for name in ("rotations", "shears", "scalings"):
            d[name] = np.asarray(ga[name], dtype=np.float64) if name in ga else full[name]
        d["A"] = R.affine_matrix(d["rotations"], d["shears"], d["scalings"]).astype(np.float32)
        d["c2"] = full["c2"]
        d["nonlinear"] = bool(cfg["nonlinear"])
        if d["nonlinear"]:
            d["nonlin_scale"] = float(np.asarray(gn["nonlin_scale"]).reshape(-1)[0]) if "nonlin_scale" in gn else full["nonlin_scale"]
            d["nonlin_std"] = float(gn["nonlin_std"]) if "nonlin_std" in gn else full["nonlin_std"]
            d["field_dims"] = ([int(v) for v in gn["size_F_small"]] if "size_F_small" in gn
                               else np.round(d["nonlin_scale"] * shape).astype(int).tolist())
    if "gamma" in gp.get("gamma_params", {}):
        d["gamma_active"], d["gamma"] = True, float(gp["gamma_params"]["gamma"])
    bp = gp.get("bf_params", {})
    if len(bp) > 0:
        d["bias_active"] = True
        d["bf_scale"] = float(np.asarray(bp["bf_scale"]).reshape(-1)[0]) if "bf_scale" in bp else full["bf_scale"]
        d["bf_std"] = float(np.asarray(bp["bf_std"]).reshape(-1)[0]) if "bf_std" in bp else full["bf_std"]
        d["bias_dims"] = np.maximum(np.round(d["bf_scale"] * shape).astype(int), 1).tolist()
    if "spacing" in gp.get("resample_params", {}):
        sp = np.asarray(gp["resample_params"]["spacing"], dtype=np.float64)
        d["resample_active"], d["spacing"], d["spacing3"], d["u_std"] = True, float(sp[0]), sp.tolist(), full["u_std"]
        stds = (0.85 + 0.3 * d["u_std"]) * np.log(5) / np.pi * sp / res  # synthseg.py:70-76, per axis
        stds[sp <= res] = 0.0
        d["stds"] = stds
        d["low_shape"] = (shape * res / sp).astype(int).tolist()
    if "noise_std" in gp.get("noise_params", {}):
        d["noise_active"], d["noise_std"] = True, float(gp["noise_params"]["noise_std"])
    return d


def check_draws(d, w: dict, cfg: dict):
    """The C struct `d` against the restated draws `w`, to the tolerances of
    tests/test_keyed_draws.py::test_c_draws_equal_the_numpy_restatement (exact for draws and sizes; cos / sin / exp / log come
    from glibc here and from numpy there: atol 2e-7 on A, rtol 1e-15 elsewhere)."""
    assert d.key == w["key"] and list(d.subclusters)[: cfg["meta_labels"]] == w["subclusters"]
    for g in ("deform", "gamma", "bias", "resample", "noise"):
        assert bool(getattr(d, g + "_active")) == bool(w[g + "_active"]), g
    assert list(d.low_shape) == w["low_shape"]
    if w["deform_active"]:
        assert bool(d.flip) == bool(w["flip"])
        for name in ("rotations", "shears", "scalings", "c2"):
            np.testing.assert_allclose(np.array(getattr(d, name)), w[name], rtol=1e-15, atol=0, err_msg=name)
        np.testing.assert_allclose(np.array(d.A).reshape(3, 3), w["A"], rtol=0, atol=2e-7)
        assert bool(d.nonlinear) == w["nonlinear"]
        if w["nonlinear"]:
            assert list(d.field_dims) == w["field_dims"]
            assert d.nonlin_scale == w["nonlin_scale"] and d.nonlin_std == w["nonlin_std"]
    if w["gamma_active"]:
        assert abs(d.gamma - w["gamma"]) <= 1e-14 * w["gamma"]
    if w["bias_active"]:
        assert list(d.bias_dims) == w["bias_dims"] and d.bf_scale == w["bf_scale"] and d.bf_std == w["bf_std"]
    if w["resample_active"]:
        assert d.spacing == w["spacing"] and list(d.spacing3) == w["spacing3"] and d.u_std == w["u_std"]
        np.testing.assert_allclose(np.array(d.stds), w["stds"], rtol=1e-15, atol=0)
        for a in range(3):
            assert d.blur_ntaps[a] == (2 * int(np.ceil(3 * w["stds"][a])) + 1 if w["stds"][a] > 0 else 0)
    if w["noise_active"]:
        assert d.noise_std == w["noise_std"] and d.noise_std32 == np.float32(w["noise_std"])


def field_bytes(d) -> dict:
    """{field name: bytes} of a ctypes struct."""
    out = {}
    for name, _t in d._fields_:
        v = getattr(d, name)
        out[name] = bytes(v) if isinstance(v, C.Array) else v
    return out


def context(shape, **kw):
    """(generator, KeyedContext, configuration as a dict) -- host objects: no GPU call is made."""
    from fetalsyngen_amd import keyed
    from tests.util_cases import make_generator

    gen = make_generator(shape, DEV, rng="keyed", **kw)
    kc = keyed.KeyedContext(gen, shape)
    return gen, kc, keyed.config_dict(kc.cfg)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def export(d, block) -> dict:
    """Exported draws + the device block read back -> the oracle's `draws=` dict (as tests/test_keyed_draws.py::_export)."""
    f = block.view(torch.float32).cpu()
    ex = {"m2s": {m + 1: int(d.subclusters[m]) for m in range(4)},
          "mus": f[d.off_mus // 4: d.off_mus // 4 + d.ntab].clone(), "sigmas": f[d.off_sigmas // 4: d.off_sigmas // 4 + d.ntab].clone(),
          "deform": None, "gamma": d.gamma if d.gamma_active else None, "bias": None, "resample": None,
          "noise_std": d.noise_std if d.noise_active else None}
    if d.deform_active:
        fs = None
        if d.nonlinear:
            n = int(np.prod(list(d.field_dims))) * 3
            fs = f[d.off_field // 4: d.off_field // 4 + n].reshape(*d.field_dims, 3).clone()
        ex["deform"] = {"flip": bool(d.flip), "A": torch.tensor(np.array(d.A, dtype=np.float32).reshape(3, 3)),
                        "c2": torch.tensor(np.array(d.c2, dtype=np.float64)), "f_small": fs}
    if d.bias_active:
        n = int(np.prod(list(d.bias_dims)))
        ex["bias"] = f[d.off_bias // 4: d.off_bias // 4 + n].reshape(*d.bias_dims).clone()
    if d.resample_active:
        ex["resample"] = {"spacing": d.spacing, "u_std": d.u_std, "spacing3": list(d.spacing3)}
    return ex


def oracle_sample(kc, K, shape, key, seg, seeds, cfg_kw, genparams=None):
    """(draws, exported draws, oracle result) of sample `key` with `genparams` fixed: the draw kernel fills a block of the
    overridden draws, the pinned oracle runs the reference's arithmetic on what it holds."""
    from fetalsyngen_amd import _lib, keyed

    ov = keyed.overrides_of(genparams, kc.cfg, DEV) if genparams else None
    d = kc.draws(key, ov)
    block = torch.empty(max(kc.block_bytes, d.block_bytes), dtype=torch.uint8, device=DEV)
    _lib.check(kc.lib.fsg_keyed_fill_block(kc.handle, C.byref(d), C.c_void_p(block.data_ptr()), K._stream(block)), "fill")
    torch.cuda.synchronize()
    ex = export(d, block)
    cfg = O.Config(shape, **cfg_kw)
    gmm = lambda shp: K.randn(shp, key, 1, DEV).cpu()  # noqa: E731
    low = lambda shp: K.randn(shp, key, 2, DEV).cpu()  # noqa: E731
    seg_t = torch.from_numpy(seg)
    rs = ex["resample"]
    if rs is None or len(set(rs["spacing3"])) == 1:
        return d, ex, O.run_sample(cfg, seg_t, seeds, draws=ex, noise_gmm=gmm, noise_lowres=low)
    # a vector spacing: the injected run takes a scalar only, so the stages behind the bias field are applied here
    r = O.run_sample(cfg, seg_t, seeds, draws=dict(ex, resample=None, noise_std=None), noise_gmm=gmm, noise_lowres=low,
                     keep_stages=True)
    out, factors = O.resample_down(r["stages"]["bias"], cfg.resolution, np.array(rs["spacing3"]), float(rs["u_std"]))
    if ex["noise_std"] is not None:
        out = O.add_noise(out, np.array([ex["noise_std"]], dtype=np.float64), low(tuple(out.shape)))
    out = O.resize_back(out, factors)
    return d, ex, {"out": out, "seg": r["seg"], "scaled": O.scale01(out)}
