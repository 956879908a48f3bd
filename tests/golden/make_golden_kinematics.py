#!/usr/bin/env python3
"""Regenerates the golden fixtures of the scenes with moving sources from the UNMODIFIED reference (oracle/_ref, built by
`make -f oracle/Makefile.ref`), as make_golden_electrons.py does for the electron scenes.  Runs only where the reference build exists; the
fixtures are data and are committed.

  python tests/golden/make_golden_kinematics.py [--check]

Fixtures:
  cfg1kin_cells.npz   tests/ski/cfg1kinsteep.ski (cfg1kin with a dust mix that is steep across 0.4-0.75 micron): per-cell volume and number
               density as the reference computed them (bit patterns), and its cross sections (`mix`: rows of wavelength, extinction,
               scattering, asymmetry parameter) at wavelengths that lie inside the simulation's wavelength range only because a moving
               source widens it by 1/3 (Configuration.cpp:573): without the widening the dust tables end near 0.52 and 0.59 micron and
               the values there are those of the table's ends
  cfg3kin_rebinned.npz   tests/ski/cfg3kin.ski at 10^6 packets, seed 0: per instrument the total flux cube and the statistics cubes w^0 .. w^2,
               summed over 8 x 8 blocks of the 64^2 pixels per wavelength bin in double precision (tests/kinematics_checks.py; the FITS files
               themselves are not committed), and the instruments' wavelengths

--check also runs the reference with seed 1, and with seed 1 on the STATIC scene (every velocity zero), and holds both against the fixture
with kinematics_checks.all_light -- every block of every wavelength bin -- under electron_checks.meets_stated_criteria (reduced chi^2 in
[0.85, 1.2], no block beyond 5.5 sigma, integrated flux within 3 sigma, more than 500 blocks): the moving run must meet them, the static one
must not; it fails otherwise.  It also prints the mean velocity per block column of the edge-on and the face-on frame.
Recorded when the fixtures were made (reduced chi^2, largest |z|, integrated flux in sigma, blocks):
  cfg3kin  reference seed 1 against seed 0:                      1.048    3.35    0.29   792
  cfg3kin  reference seed 1, STATIC scene, against seed 0:    1723.8   175.05  282.66   160
  cfg3kin  edge-on, mean velocity per block column (km/s):  -2144 -2012 -1739 -921 936 1745 2017 2150  (the disk rotates at 2400 km/s)
  cfg3kin  face-on: within 5 km/s of zero outside the central columns, where the point source approaches at 1200 km/s
(The runs use four threads: which packet lands in which thread's order differs from run to run, the statistics do not.)
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import electron_checks as E  # noqa: E402
import kinematics_checks as K  # noqa: E402

INSTRUMENTS = ("edge", "face")
N = 1000000
PINNED_WAVELENGTHS = (0.41e-6, 0.45e-6, 0.50e-6, 0.62e-6, 0.70e-6, 0.74e-6)


def reference_run(ski, prefix, tmp):
    subprocess.check_call([REF, "run", ski, "-t", "4", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
    return K.rebinned_cubes(tmp, prefix, INSTRUMENTS)


def wavelengths_of(tmp, prefix):
    return np.loadtxt(os.path.join(tmp, f"{prefix}_edge_sed.dat"))[:, 0] * 1e-6


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    check = "--check" in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        ski = os.path.join(ROOT, "tests", "ski", "cfg1kinsteep.ski")
        vol, dens, mix = [], [], []
        for w in PINNED_WAVELENGTHS:
            cells = os.path.join(tmp, "cells.txt")
            subprocess.check_call([REF, "cells", ski, cells, "-w", repr(w), "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
            first = not vol
            for line in open(cells):
                t = line.split()
                if t[0] == "cells":
                    continue
                if t[0] == "mix":
                    mix.append([float.fromhex(v) for v in t[1:]])
                    continue
                if first:
                    vol.append(float.fromhex(t[4]))
                    dens.append(float.fromhex(t[5]))
        np.savez_compressed(os.path.join(HERE, "cfg1kin_cells.npz"), volume=np.array(vol), density=np.array(dens), mix=np.array(mix))
    with tempfile.TemporaryDirectory() as tmp:
        name = "cfg3kin"
        text = open(os.path.join(ROOT, "tests", "ski", name + ".ski")).read()
        full = os.path.join(tmp, name + ".ski")
        open(full, "w").write(re.sub(r'numPackets="[^"]*"', 'numPackets="1e6"', text))
        first = reference_run(full, name, tmp)
        first["wavelengths"] = wavelengths_of(tmp, name)
        np.savez_compressed(os.path.join(HERE, name + "_rebinned.npz"), **first)
        for inst in INSTRUMENTS:
            print(name, inst, "mean velocity per block column (km/s):", np.round(K.column_velocities(first[f"{inst}_total"], first["wavelengths"], 0.55e-6) / 1e3, 1), flush=True)
        if check:
            seeded = open(full).read().replace('<Random seed="0"/>', '<Random seed="1"/>')
            static = re.sub(r'velocity(X|Y|Z|Magnitude)="[^"]*"', lambda m: 'velocity%s="0 km/s"' % m.group(1), seeded)
            results = {}
            for label, variant in (("moving", seeded), ("static", static)):
                other = os.path.join(tmp, label)
                os.makedirs(other)
                open(os.path.join(other, name + ".ski"), "w").write(variant)
                second = reference_run(os.path.join(other, name + ".ski"), name, other)
                results[label] = K.all_light(second, N, first, N, INSTRUMENTS)
                print(name, f"reference seed 1 ({label}) against seed 0:", results[label], flush=True)
            if not E.meets_stated_criteria(*results["moving"]):
                sys.exit("two runs of the reference do not meet the stated criteria: change the scene")
            if E.meets_stated_criteria(*results["static"]):
                sys.exit("the static scene meets the stated criteria: the comparison does not see the kinematics")
    print("kinematics fixtures regenerated")


if __name__ == "__main__":
    main()
