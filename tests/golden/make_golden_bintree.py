#!/usr/bin/env python3
"""Regenerates the fixtures of the binary-tree grid (PolicyTreeSpatialGrid with treeType BinTree) from the UNMODIFIED reference
(oracle/_ref, built by `make -f oracle/Makefile.ref`).  The fixtures are data and are committed.

  python tests/golden/make_golden_bintree.py [--check] [cfg2bin] [cfg2bindeep]

Fixtures:
  cfg2bin_cells.npz, cfg2bindeep_cells.npz   the reference's cell table (skirt_ref cells): per cell the centre of its box, its volume and
               the number density of the dust, as the doubles the reference holds (bit patterns), and the dust cross sections at 0.55 micron
  cfg2bin_rays.txt, cfg2bindeep_rays.txt, *_rays_ref.txt   48 fixed rays (random, the special rays of make_golden.rays, nearly in the
               mid-plane, and aimed at dyadic points of the domain: corners and edges of nodes) and the reference's (m, ds) sequences
               (C99 hex floats)
  cfg2bin_rebinned.npz, cfg2bin_seed1_rebinned.npz   the photon loop of tests/ski/cfg2bin.ski (10^6 packets, one thread) with the
               reference's own generator at seed 0 and at seed 1: per instrument the total and the transparent flux and the statistics frames
               w^0 .. w^2, summed over 8 x 8 blocks of the 128^2 pixels in double precision
  --check      prints the comparison of the seed-1 run with the seed-0 run by tests/bintree_checks.within_noise (the criteria that
               test_gpu_bintree states for the GPU against seed 0)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bintree_checks as B  # noqa: E402
from make_golden import rays  # noqa: E402

PC = 3.08567758e16
N = 1000000
# (scale of the random rays, factor on the dyadic points: the cusp of cfg2bindeep is refined around the origin)
SCENES = {"cfg2bin": (4000 * PC, 1.0), "cfg2bindeep": (300 * PC, 1.0 / 64)}


def fixed_rays(scale, shrink):
    """48 rays: 20 random and the 8 special ones of make_golden.rays, 6 nearly in the mid-plane, 14 through dyadic points of the box
    (+-20 kpc x +-20 kpc x +-4 kpc) along diagonals and axes -- corners and edges of nodes: ties between exit walls"""
    out = rays(scale, 20, 11)
    rng = np.random.default_rng(12)
    for i in range(6):
        r = (rng.random(3) - 0.5) * 2 * scale * np.array([1.0, 1.0, 0.05])
        k = rng.normal(size=3)
        k[2] *= 0.02
        out.append((r, k / np.linalg.norm(k)))
    ext = np.array([20000 * PC, 20000 * PC, 4000 * PC]) * shrink
    s2, s3 = 1 / np.sqrt(2.0), 1 / np.sqrt(3.0)
    for frac, k in (((0.0, 0.0, 0.0), (s3, s3, s3)), ((0.25, 0.125, 0.0), (s2, -s2, 0.0)), ((0.03125, -0.0625, 0.015625), (s3, -s3, s3)),
                    ((-0.5, 0.25, 0.0), (0.0, s2, s2)), ((0.0078125, 0.0078125, 0.0), (1.0, 0.0, 0.0)),
                    ((0.001953125, -0.00390625, 0.0009765625), (-s3, s3, s3)), ((0.0, 0.0, 0.001953125), (s2, s2, 0.0)),
                    ((0.5, 0.5, 0.5), (-s3, -s3, -s3)), ((0.0625, 0.0, 0.0), (0.0, 0.0, 1.0)), ((0.0, 0.03125, 0.0), (0.6, 0.0, 0.8)),
                    ((0.015625, 0.015625, 0.015625), (0.0, -0.6, 0.8)), ((0.125, 0.125, 0.0), (-s2, -s2, 0.0)),
                    ((0.0009765625, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.00390625, 0.00390625, 0.00390625), (s3, s3, -s3))):
        out.append((np.array(frac) * ext, np.array(k) / np.linalg.norm(k)))
    assert len(out) == 48
    return out


def reference_run(ski, prefix, tmp):
    subprocess.check_call([REF, "run", ski, "-t", "1", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
    return B.rebinned_files(tmp, prefix)


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    check = "--check" in sys.argv[1:]
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, (scale, shrink) in SCENES.items():
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        with tempfile.TemporaryDirectory() as tmp:
            cells = os.path.join(tmp, "cells.txt")
            subprocess.check_call([REF, "cells", ski, cells, "-w", "0.55e-6", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
            centre, vol, dens, mix, count = [], [], [], None, None
            for line in open(cells):
                t = line.split()
                if t[0] == "cells":
                    count = int(t[1])
                    continue
                if t[0] == "mix":
                    mix = [float.fromhex(v) for v in t[1:]]
                    continue
                centre.append([float.fromhex(v) for v in t[1:4]])
                vol.append(float.fromhex(t[4]))
                dens.append(float.fromhex(t[5]))
            assert count == len(dens)
            np.savez_compressed(os.path.join(HERE, name + "_cells.npz"), centre=np.array(centre), volume=np.array(vol), density=np.array(dens),
                                mix=np.array(mix))
            rayfile = os.path.join(HERE, name + "_rays.txt")
            with open(rayfile, "w") as fh:
                for r, k in fixed_rays(scale, shrink):
                    fh.write(" ".join(float(v).hex() for v in list(r) + list(k)) + "\n")
            subprocess.check_call([REF, "rays", ski, rayfile, os.path.join(HERE, name + "_rays_ref.txt"), "-o", tmp], cwd=tmp,
                                  stdout=subprocess.DEVNULL)
            if name != "cfg2bin":
                continue
            text = open(ski).read()
            assert 'numPackets="1e6"' in text and '<Random seed="0"/>' in text
            first = reference_run(ski, name, tmp)
            np.savez_compressed(os.path.join(HERE, name + "_rebinned.npz"), **first)
            other = os.path.join(tmp, "seed1")
            os.makedirs(other)
            again = os.path.join(other, name + ".ski")
            open(again, "w").write(text.replace('<Random seed="0"/>', '<Random seed="1"/>'))
            second = reference_run(again, name, other)
            np.savez_compressed(os.path.join(HERE, name + "_seed1_rebinned.npz"), **second)
            if check:
                result = B.within_noise(second, N, first, N)
                print(name, "reference seed 1 against seed 0 (chi2, largest |z|, flux sigmas, blocks):", result,
                      "meets the criteria" if B.meets_stated_criteria(*result) else "MISSES the criteria", flush=True)
    print("binary-tree fixtures regenerated")


if __name__ == "__main__":
    main()
