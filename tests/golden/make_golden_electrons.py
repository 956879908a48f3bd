#!/usr/bin/env python3
"""Regenerates the golden fixtures of the electron scenes (ElectronMix: Thomson scattering, dipole phase function) from the UNMODIFIED
reference (oracle/_ref, built by `make -f oracle/Makefile.ref`), as make_golden.py does for the other scenes.  Runs only where the
reference build exists; the fixtures are data and are committed.

  python tests/golden/make_golden_electrons.py [--check] [scene ...]

Fixtures:
  cfg1elec_cells.npz, cfg2agnelec_cells.npz   per-cell volume and number density of medium component 0 -- the electrons in both scenes --
               as the reference computed them (bit patterns), and its cross sections at 0.55 micron (`mix`: wavelength, extinction,
               scattering, asymmetry parameter)
  cfg1elec_rebinned.npz, cfg2agnelec_rebinned.npz   the photon loop at 10^6 packets, seed 0, one thread: per instrument the total and
               primary-direct flux frames and the statistics frames w^0 .. w^2, summed over 8 x 8 blocks of the 256^2 pixels in double
               precision (tests/electron_checks.py; the FITS files themselves are not committed)

--check also runs the reference with seed 1 and the project's CPU oracle (which treats the electrons as an isotropic scatterer: it has no
dipole) at 10^6 packets, and prints the scattered-light comparison of electron_checks.scattered_light for both pairs.  Recorded when the
fixtures were made (reduced chi^2, largest |z|, integrated flux in sigma, blocks):
  cfg1elec     reference seed 1 against seed 0:        1.053   4.26   0.30   2651
  cfg1elec     isotropic oracle against the reference: 8.179  16.85   0.52   2652
  cfg2agnelec  reference seed 1 against seed 0:        1.132   5.16   2.30   1049
  cfg2agnelec  isotropic oracle against the reference: 17.36  51.91  49.09   1058
(The seed of the reference also drives its setup -- the sample positions of the tree policy and of the cell densities --, so the two reference
runs of cfg2agnelec differ in their grid and densities as well, not only in their photon packets; with a cusped electron density inside the
innermost cells that difference alone was 7.8 sigma of the integrated flux, which is why the shell of cfg2agnelec is uniform and starts two
cells from the centre.  The engine's runs share the setup of seed 0 with the fixture.)
The reference-against-reference pairs meet the criteria of test_fits_cube_within_noise_of_the_reference (chi^2 in [0.85, 1.2], no block
beyond 5.5 sigma, flux within 3 sigma); the isotropic runs are far outside: the comparison tells the dipole from an isotropic scatterer.
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

SCENES = {"cfg1elec": ("i30", "i90", "i150"), "cfg2agnelec": ("i0", "i1")}
N = 1000000


def reference_run(ski, prefix, instruments, tmp):
    subprocess.check_call([REF, "run", ski, "-t", "1", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
    return E.rebinned_files(tmp, prefix, instruments)


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    check = "--check" in sys.argv[1:]
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, instruments in SCENES.items():
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        text = open(ski).read()
        assert 'numPackets="1e6"' in text or 'numPackets="2e4"' in text
        with tempfile.TemporaryDirectory() as tmp:
            cells = os.path.join(tmp, "cells.txt")
            subprocess.check_call([REF, "cells", ski, cells, "-w", "0.55e-6", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
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
            # the photon loop at 10^6 packets (the ski files of the octree scenes ask for fewer: a copy with the number changed)
            full = os.path.join(tmp, name + ".ski")
            open(full, "w").write(re.sub(r'numPackets="[^"]*"', 'numPackets="1e6"', text))
            first = reference_run(full, name, instruments, tmp)
            np.savez_compressed(os.path.join(HERE, name + "_rebinned.npz"), **first)
            if check:
                other = os.path.join(tmp, "seed1")
                os.makedirs(other)
                again = os.path.join(other, name + ".ski")
                open(again, "w").write(open(full).read().replace('<Random seed="0"/>', '<Random seed="1"/>'))
                second = reference_run(again, name, instruments, other)
                print(name, "reference seed 1 against seed 0:", E.scattered_light(second, N, first, N, instruments), flush=True)
                import oracle_lib as O
                from skirt9_amd.host import Simulation
                sim = Simulation(ski, num_packets=N).setup()
                frames, _ = O.run_primary(sim, 0, N, O.RNG_PHILOX, seed=20260929)
                iso = os.path.join(tmp, "oracle")
                sim.write(frames, iso)
                print(name, "isotropic oracle against the reference:", E.scattered_light(E.rebinned_files(iso, name, instruments), N, first, N, instruments), flush=True)
    print("electron fixtures regenerated")


if __name__ == "__main__":
    main()
