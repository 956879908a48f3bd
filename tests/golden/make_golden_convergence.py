#!/usr/bin/env python3
"""Regenerates the golden fixtures of the convergence-cut scenes (ConvergenceCutsProbe) from the UNMODIFIED reference (oracle/_ref, built
by `make -f oracle/Makefile.ref`), as make_golden_probes.py does for the probe maps.  Runs only where the reference build exists; the
fixtures are data and are committed.

  python tests/golden/make_golden_convergence.py [scene ...]

The reference runs in emulation mode (skirt_ref run -e -t 1: setup, no photon packets, every probe written).  A cut is a FITS image of
1024 x 1024 pixels: 4 MB, too large to commit.  Per scene of tests/convergence_checks.CUT_SCENES one file <scene>_cuts.npz holds, for every
cut file the reference writes,

  digest/<file name>   the sha256 (as 32 bytes) of the file's bytes with the DATE card blanked: what the tests compare
  pixels/<file name>   a 64 x 64 decimation of the image, every 16th pixel in both directions from pixel (0, 0), as float64: what lets a
                       failing digest be localised

Per scene of INFO_SCENES (both convergence probes, as the ski-file wizard proposes them) the text file <scene>_inf_convergence.dat of the
ConvergenceInfoProbe is committed as written.

For the Voronoi scene only the cuts of the true density (_t_) are kept: the tessellation is the host layer's own, so the cells, and with
them the gridded cuts, are not the reference's.
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from convergence_checks import CUT_SCENES, INFO_SCENES, PROBE_NAME, TRUE_CUTS_ONLY, cut_digest, cut_pixels, info_file  # noqa: E402


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name in CUT_SCENES:
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", "-e", ski, "-t", "1", "-o", tmp], cwd=os.path.dirname(ski), stdout=subprocess.DEVNULL)
            written = sorted(f for f in os.listdir(tmp) if f.startswith(f"{name}_{PROBE_NAME}_") and f.endswith(".fits"))
            assert written, name
            if name in TRUE_CUTS_ONLY:
                written = [f for f in written if "_t_" in f]
            arrays = {}
            for f in written:
                data = open(os.path.join(tmp, f), "rb").read()
                arrays["digest/" + f] = np.frombuffer(cut_digest(data), dtype=np.uint8)
                arrays["pixels/" + f] = cut_pixels(data)[::16, ::16].astype(np.float64)
            np.savez_compressed(os.path.join(HERE, name + "_cuts.npz"), **arrays)
            print(name, len(written), "files:", " ".join(written))
    for name in INFO_SCENES:
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", "-e", ski, "-t", "1", "-o", tmp], cwd=os.path.dirname(ski), stdout=subprocess.DEVNULL)
            shutil.copy(os.path.join(tmp, info_file(name)), os.path.join(HERE, info_file(name)))
            print(name, info_file(name))


if __name__ == "__main__":
    main()
