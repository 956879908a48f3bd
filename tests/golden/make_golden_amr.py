#!/usr/bin/env python3
"""Regenerates the golden fixtures of the adaptive-mesh scenes (AdaptiveMeshMedium) from the UNMODIFIED reference (oracle/_ref, built by
`make -f oracle/Makefile.ref`), as make_golden.py and make_golden_convergence.py do for the other scenes.  Runs only where the reference
build exists; the fixtures are recorded results and are committed.

  python tests/golden/make_golden_amr.py [scene ...]

Fixtures:
  cfg6amr_i0_*.fits, cfg6amr_i0_sed.dat, cfg6amr_i0_sedstats.dat   the reference's output files of cfg6amr (2x10^4 packets, seed 0, one thread)
  cfg6amr_cells.npz, cfg6amrnum_cells.npz, cfg6amrelec_cells.npz   per-cell volume and number density of medium component 0 as the reference
               computed them (bit patterns), and its cross sections at 0.55 micron (`mix`)
  cfg6amrconv_inf_convergence.dat   the ConvergenceInfoProbe's file as written (emulation mode: setup, no photon packets)
  cfg6amrconv_cuts.npz              per cut file of the ConvergenceCutsProbe the sha256 with the DATE card blanked (digest/<file>) and a
               64 x 64 decimation of the image (pixels/<file>), in the form of make_golden_convergence.py
The mesh files themselves (tests/ski/cfg6amr_mesh.txt, cfg6amrsym_mesh.txt) come from tools/make_amr.py.
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SKI = os.path.join(ROOT, "tests", "ski")
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from convergence_checks import PROBE_NAME, cut_digest, cut_pixels, info_file  # noqa: E402

FILE_SCENES = ("cfg6amr",)
CELL_SCENES = ("cfg6amr", "cfg6amrnum", "cfg6amrelec")
CONVERGENCE_SCENES = ("cfg6amrconv",)


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    wanted = lambda name: not only or name in only  # noqa: E731
    # (input files named in a ski file are read from the working directory: FilePaths::input)
    for name in filter(wanted, FILE_SCENES):
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", os.path.join(SKI, name + ".ski"), "-t", "1", "-o", tmp], cwd=SKI, stdout=subprocess.DEVNULL)
            written = sorted(f for f in os.listdir(tmp) if f.startswith(name + "_i") and (f.endswith(".fits") or f.endswith(".dat")))
            assert written, name
            for f in written:
                shutil.copy(os.path.join(tmp, f), os.path.join(HERE, f))
            print(name, len(written), "files")
    for name in filter(wanted, CELL_SCENES):
        with tempfile.TemporaryDirectory() as tmp:
            cells = os.path.join(tmp, "cells.txt")
            subprocess.check_call([REF, "cells", os.path.join(SKI, name + ".ski"), cells, "-w", "0.55e-6", "-o", tmp], cwd=SKI,
                                  stdout=subprocess.DEVNULL)
            vol, dens, mix = [], [], None
            for line in open(cells):
                t = line.split()
                if t[0] == "cells":
                    continue
                if t[0] == "mix":
                    mix = [float.fromhex(v) for v in t[1:]]
                    continue
                vol.append(float.fromhex(t[4]))
                dens.append(float.fromhex(t[5]))
            np.savez_compressed(os.path.join(HERE, name + "_cells.npz"), volume=np.array(vol), density=np.array(dens), mix=np.array(mix))
            print(name, len(dens), "cells")
    for name in filter(wanted, CONVERGENCE_SCENES):
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", "-e", os.path.join(SKI, name + ".ski"), "-t", "1", "-o", tmp], cwd=SKI, stdout=subprocess.DEVNULL)
            shutil.copy(os.path.join(tmp, info_file(name)), os.path.join(HERE, info_file(name)))
            written = sorted(f for f in os.listdir(tmp) if f.startswith(f"{name}_{PROBE_NAME}_") and f.endswith(".fits"))
            assert written, name
            arrays = {}
            for f in written:
                data = open(os.path.join(tmp, f), "rb").read()
                arrays["digest/" + f] = np.frombuffer(cut_digest(data), dtype=np.uint8)
                arrays["pixels/" + f] = cut_pixels(data)[::16, ::16].astype(np.float64)
            np.savez_compressed(os.path.join(HERE, name + "_cuts.npz"), **arrays)
            print(name, info_file(name), len(written), "cut files:", " ".join(written))


if __name__ == "__main__":
    main()
