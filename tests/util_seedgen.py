"""Inputs shared by the seed-generation tests (CPU reference pin and GPU parity)."""
import numpy as np


def synthetic_job(n=3_000_000, seed=7):
    """A 3 M-sample, 3-component job (many workgroups per job) and its fixed initialisation."""
    rng = np.random.default_rng(seed)
    comp = rng.choice(3, size=n, p=[0.5, 0.3, 0.2])
    x = (np.array([800.0, 1500.0, 2300.0])[comp] + np.array([60.0, 150.0, 90.0])[comp] * rng.standard_normal(n)).astype(np.float32)
    init = (np.full(3, 1 / 3), np.array([700.0, 1400.0, 2500.0]), np.full(3, 200.0**2))
    return x, init
