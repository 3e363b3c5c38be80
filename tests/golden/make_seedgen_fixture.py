#!/usr/bin/env python3
"""Record scikit-learn's Gaussian-mixture fits on the reference's sample subject as a data fixture.

Run by hand where the reference tree and scikit-learn exist; never by a test.  Reads the reference's bundled
`sub-sta21` T2w + dseg, sub-samples both `[::2, ::2, ::2]` (128^3), fuses the meta-labels and fits, for every
meta-label and k in KS, `sklearn.mixture.GaussianMixture` (1-D, "full" covariance):

  * from a fixed initialisation (quantile means, equal weights, var(x) / k^2), once with tol=0 / max_iter=20 and once
    with the defaults (tol=1e-3, max_iter=100): weights, means, covariances, n_iter_, lower_bound_, predict labels;
  * with n_init=5, init_params="k-means++" under 8 random_states: lower_bound_ only (the reference's own scatter).

Output: tests/golden/seedgen_sta21_s2.npz -- arrays only.

Usage: python tests/golden/make_seedgen_fixture.py --ref REFERENCE_CHECKOUT
"""
from __future__ import annotations

import argparse
import sys
import warnings
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

KS = (2, 3, 4, 7, 10)
N_STATES = 8


def fits_for(args):
    x, m, k = args
    from sklearn.mixture import GaussianMixture

    from tests import util_em64 as E

    warnings.simplefilter("ignore")
    X = x.astype(np.float64).reshape(-1, 1)
    w0, mu0, var0 = E.quantile_init(x, k)
    out = {f"init_w_{m}_{k}": w0, f"init_mu_{m}_{k}": mu0, f"init_var_{m}_{k}": var0}
    for tag, kw in (("fix20", dict(tol=0.0, max_iter=20)), ("dflt", dict())):
        g = GaussianMixture(n_components=k, weights_init=w0, means_init=mu0.reshape(-1, 1),
                            precisions_init=(1.0 / var0).reshape(-1, 1, 1), **kw).fit(X)
        p = f"{tag}_{m}_{k}"
        out[f"w_{p}"], out[f"mu_{p}"], out[f"var_{p}"] = g.weights_, g.means_[:, 0], g.covariances_[:, 0, 0]
        out[f"niter_{p}"], out[f"lb_{p}"] = np.int64(g.n_iter_), np.float64(g.lower_bound_)
        out[f"labels_{p}"] = g.predict(X).astype(np.uint8)
    lbs = [GaussianMixture(n_components=k, n_init=5, init_params="k-means++", random_state=s).fit(X).lower_bound_
           for s in range(N_STATES)]
    out[f"lb8_{m}_{k}"] = np.array(lbs, np.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    from fetalsyngen_amd.utils.image_reading import NiftiReader
    from tests import util_em64 as E

    anat = Path(args.ref) / "data" / "sub-sta21" / "anat"
    reader = NiftiReader()
    image = reader(anat / "sub-sta21_rec-irtk_T2w.nii.gz").numpy().astype(np.float32)[::2, ::2, ::2]
    dseg = reader(anat / "sub-sta21_rec-irtk_T2w_dseg.nii.gz").numpy()[::2, ::2, ::2]
    assert np.array_equal(dseg, dseg.astype(np.uint8))
    image, dseg = np.ascontiguousarray(image), np.ascontiguousarray(dseg.astype(np.uint8))
    meta = E.meta_labels(image, dseg, "feta")
    out = {"image": image, "dseg": dseg, "ks": np.array(KS), "counts": np.array([(meta == m).sum() for m in range(1, 5)])}
    tasks = [(E.packed(image, meta, m), m, k) for m in range(1, 5) for k in KS]
    with ProcessPoolExecutor(args.jobs) as pool:
        for res in pool.map(fits_for, tasks):
            out.update(res)
    np.savez_compressed(HERE / "seedgen_sta21_s2.npz", **out)
    print("wrote seedgen_sta21_s2.npz:", (HERE / "seedgen_sta21_s2.npz").stat().st_size, "bytes; counts", out["counts"])


if __name__ == "__main__":
    main()
