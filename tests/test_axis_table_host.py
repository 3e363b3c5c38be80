"""CPU: `tables.axis_table`, the one builder behind prewarming and the keyed table registration, byte for byte against the
per-sample plans' own paths to the same tables; and the number of tables `prewarm()` asks it for."""
import hashlib

import numpy as np
import pytest
import torch

from fetalsyngen_amd import _lib
from fetalsyngen_amd import kernels as K
from fetalsyngen_amd import tables as T
from fetalsyngen_amd.generator.augmentation.synthseg import BiasPlan, RandBiasField

KT = _lib.KT
SIZES = (13, 16)
# prewarm() of bench.build_generator((256,) * 3, ...) on the parent of the commit that introduced axis_table: the count it
# returned, and the SHA-256 of the tables it uploaded, concatenated in upload order
PREWARM_TABLES_256 = 1095
PREWARM_SHA256_256 = "bb52116aca9b78e255dcfd63e260056e2e0a7ae7f2a5a12da7625170dc75db22"


def ns(size, beyond):
    return (1, size - 1, size) + ((size + 3,) if beyond else ())


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", SIZES)
def test_resample_tables_are_those_of_resample_plan(size):
    for n in ns(size, True):  # (n > size: a spacing below the resolution, which only a caller's genparams reach)
        spacing = np.full(3, size / (n + 0.5))
        _stds, new_size, _factors, tabs = T.resample_plan((size,) * 3, np.ones(3), spacing, 0.5)
        assert new_size == (n,) * 3
        for a in range(3):
            assert same(T.axis_table(KT.RESAMPLE, n, size), tabs[a]), (size, n, a)


@pytest.mark.parametrize("size", SIZES)
def test_back_tables_are_those_of_the_zoom_back(size):
    for n in ns(size, True):
        tabs, new = T.zoom_tables_between((n,) * 3, (size,) * 3, True)
        assert new == (size,) * 3
        for a in range(3):
            assert same(T.axis_table(KT.BACK, n, size), tabs[a]), (size, n, a)


@pytest.mark.parametrize("size", SIZES)
def test_field_tables_are_those_of_the_coarse_grid_zoom(size):
    for n in ns(size, True):
        tabs, new = T.zoom_tables_between((n,) * 3, (size,) * 3)  # (SpatialDeformation.make_spec's call)
        assert new == (size,) * 3
        for a in range(3):
            assert same(T.axis_table(KT.FIELD, n, size), tabs[a]), (size, n, a)


@pytest.mark.parametrize("size", SIZES)
def test_bias_tables_are_those_of_the_bias_plan(size):
    for n in ns(size, False):
        plan = BiasPlan()
        plan.grid = torch.zeros((n, n, n), dtype=torch.float32)
        tabs = RandBiasField.tables(plan, (size,) * 3)
        for a in range(3):
            assert same(T.axis_table(KT.BIAS, n, size), tabs[a]), (size, n, a)


def test_axes_of_different_sizes_and_an_unknown_kind():
    shape, low = (13, 16, 7), (5, 16, 9)
    back, _new = T.zoom_tables_between(low, shape, True)
    field, _new = T.zoom_tables_between(low, shape)
    for a in range(3):
        assert same(T.axis_table(KT.BACK, low[a], shape[a]), back[a]) and same(T.axis_table(KT.FIELD, low[a], shape[a]), field[a])
    with pytest.raises(ValueError):
        T.axis_table(99, 4, 8)


def test_prewarm_asks_for_the_tables_it_always_did(monkeypatch):
    from bench import build_generator

    sha, calls = hashlib.sha256(), []

    def upload(tab, device):
        calls.append(tab.shape)
        sha.update(tab.tobytes())

    monkeypatch.setattr(K, "_device_table", upload)
    gen = build_generator((256,) * 3, "cuda:0", "keyed")
    assert gen.prewarm() == PREWARM_TABLES_256 == len(calls)
    assert sha.hexdigest() == PREWARM_SHA256_256
