"""Shared by tests/test_gpu_kinematics.py and tests/golden/make_golden_kinematics.py: the comparison of two runs of one panchromatic scene
block by block AND wavelength bin by wavelength bin, with the Monte Carlo noise of both, and the mean line-of-sight velocity per column
of a frame.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

from electron_checks import read_fits

FRAMES = ("total", "stats0", "stats1", "stats2")
C_LIGHT = 2.99792458e8


def rebin_cube(cube, f=8):
    """sums over f x f blocks of the pixels of every wavelength plane of a cube [wavelength][y][x]"""
    nl, ny, nx = cube.shape
    return cube.reshape(nl, ny // f, f, nx // f, f).sum(axis=(2, 4))


def rebinned_cubes(outdir, prefix, instruments):
    """{"<instrument>_<frame>": blocks[wavelength][by][bx]} of the output files of one run"""
    return {f"{inst}_{name}": rebin_cube(read_fits(os.path.join(outdir, f"{prefix}_{inst}_{name}.fits"))) for inst in instruments for name in FRAMES}


def all_light(a, n_a, b, n_b, instruments):
    """The method of electron_checks.scattered_light on every block of every wavelength bin (direct and scattered light alike): a block's
    relative error is R = sqrt(S2 / S1^2 - 1 / N) from the run's own sums of w and w^2, sigma^2 = (R_a F_a)^2 + (R_b F_b)^2; blocks with
    at least 30 contributions in both runs count.  Returns (reduced chi^2, largest |z|, difference of the integrated flux over its sigma,
    number of blocks) over all instruments together."""
    zs, diff, var = [], 0., 0.
    for inst in instruments:
        fa, fb = a[f"{inst}_total"], b[f"{inst}_total"]
        rel = []
        for run, n in ((a, n_a), (b, n_b)):
            s1, s2 = run[f"{inst}_stats1"], run[f"{inst}_stats2"]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel.append(np.sqrt(np.maximum(np.where(s1 > 0, s2 / s1 ** 2 - 1.0 / n, np.inf), 0)))
        good = (a[f"{inst}_stats0"] >= 30) & (b[f"{inst}_stats0"] >= 30)
        with np.errstate(invalid="ignore"):
            sigma = np.sqrt((rel[0] * fa) ** 2 + (rel[1] * fb) ** 2)
        zs.append((fa - fb)[good] / sigma[good])
        diff += fa[good].sum() - fb[good].sum()
        var += np.sum(sigma[good] ** 2)
    z = np.concatenate(zs)
    if z.size == 0:
        return float("inf"), float("inf"), float("inf"), 0
    return float(np.mean(z ** 2)), float(np.abs(z).max()), float(abs(diff) / np.sqrt(var)), int(z.size)


def column_velocities(blocks, wavelengths, rest_wavelength):
    """mean line-of-sight velocity (m/s, positive: receding) per block column of a rebinned total-flux cube [wavelength][by][bx]: the flux-weighted
    mean wavelength of the column against the rest wavelength of the line"""
    per_column = blocks.sum(axis=1)                                     # [wavelength][bx]
    mean = (per_column * np.asarray(wavelengths)[:, None]).sum(axis=0) / per_column.sum(axis=0)
    return C_LIGHT * (mean / rest_wavelength - 1.)
