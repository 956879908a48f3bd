"""Shared by tests/test_gpu_electrons.py and tests/golden/make_golden_electrons.py: the comparison of the SCATTERED light of two runs of
one scene, block by block, with the Monte Carlo noise of both.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

FRAMES = ("total", "primarydirect", "stats0", "stats1", "stats2")


def read_fits(path):
    """primary image of a FITS file written by FITSInOut::write / the host layer: float32, big endian"""
    raw = open(path, "rb").read()
    cards = {}
    pos = 0
    while True:
        card = raw[pos:pos + 80].decode("ascii")
        pos += 80
        if card.startswith("END"):
            break
        if "=" in card[:10]:
            cards[card[:8].strip()] = card[10:].split("/")[0].strip()
    pos = (pos + 2879) // 2880 * 2880
    shape = [int(cards[f"NAXIS{i}"]) for i in range(int(cards["NAXIS"]), 0, -1)]
    count = int(np.prod(shape))
    return np.frombuffer(raw[pos:pos + 4 * count], dtype=">f4").astype(np.float64).reshape(shape)


def rebin(a, f=8):
    """sums over f x f blocks of the pixels of one frame"""
    a = a.reshape(a.shape[-2], a.shape[-1])
    ny, nx = a.shape
    return a.reshape(ny // f, f, nx // f, f).sum(axis=(1, 3))


def rebinned_files(outdir, prefix, instruments):
    """{"<instrument>_<frame>": blocks} of the output files of one run (oligochromatic, one wavelength)"""
    return {f"{inst}_{name}": rebin(read_fits(os.path.join(outdir, f"{prefix}_{inst}_{name}.fits"))) for inst in instruments for name in FRAMES}


def scattered_light(a, n_a, b, n_b, instruments):
    """The method of test_gpu_parity.test_fits_cube_within_noise_of_the_reference on the blocks of `rebinned_files`, restricted to the
    blocks the direct light of the source does not reach in either run (primarydirect == 0): the total flux there is scattered light.
    A block's relative error is R = sqrt(S2 / S1^2 - 1 / N) from the run's own sums of w and w^2, sigma^2 = (R_a F_a)^2 + (R_b F_b)^2;
    blocks with at least 30 contributions in both runs count.  Returns (reduced chi^2, largest |z|, difference of the integrated flux
    over its sigma, number of blocks) over all instruments together."""
    zs, diff, var = [], 0., 0.
    for inst in instruments:
        fa, fb = a[f"{inst}_total"], b[f"{inst}_total"]
        rel = []
        for run, n in ((a, n_a), (b, n_b)):
            s1, s2 = run[f"{inst}_stats1"], run[f"{inst}_stats2"]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel.append(np.sqrt(np.maximum(np.where(s1 > 0, s2 / s1 ** 2 - 1.0 / n, np.inf), 0)))
        good = (a[f"{inst}_stats0"] >= 30) & (b[f"{inst}_stats0"] >= 30) & (a[f"{inst}_primarydirect"] == 0) & (b[f"{inst}_primarydirect"] == 0)
        with np.errstate(invalid="ignore"):
            sigma = np.sqrt((rel[0] * fa) ** 2 + (rel[1] * fb) ** 2)
        zs.append((fa - fb)[good] / sigma[good])
        diff += fa[good].sum() - fb[good].sum()
        var += np.sum(sigma[good] ** 2)
    z = np.concatenate(zs)
    return float(np.mean(z ** 2)), float(np.abs(z).max()), float(abs(diff) / np.sqrt(var)), int(z.size)


def meets_stated_criteria(chi2, zmax, flux_sigmas, blocks):
    """the criteria test_fits_cube_within_noise_of_the_reference states: reduced chi^2 in [0.85, 1.2], no block beyond 5.5 sigma, the
    integrated flux within 3 sigma (and enough blocks for the chi^2 to mean something)"""
    return blocks > 500 and 0.85 <= chi2 <= 1.2 and zmax < 5.5 and flux_sigmas <= 3
