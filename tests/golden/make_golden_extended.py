#!/usr/bin/env python3
"""Regenerates, from the UNMODIFIED reference (oracle/_ref, built by `make -f oracle/Makefile.ref`), the output files that pin the oracle's
dipole phase function, moving sources and binary tree byte for byte (tests/test_oracle_extended.py), in the style of make_golden.py: the
reference's own generator at seed 0, ONE thread.  Runs only where the reference build exists; the fixtures are data and are committed.

  python tests/golden/make_golden_extended.py [scene ...]

Scenes (tests/ski/<name>.ski) -> <name>_<instrument>_*.fits, *_sed.dat, *_sedstats.dat:
  cfg1elecg       free electrons on the Cartesian grid, forced scattering, two scattering levels recorded (cfg1elec at 2e4 packets, 16^2 pixels)
  cfg2agneleceag  electrons and dust on an octree, explicit absorption (cfg2agnelecea at 16^2 pixels)
  cfg1elecnfg     free electrons without forced scattering (cfg1elecnf at 2e4 packets, 16^2 pixels)
  cfg1king        a moving point source, five instruments: one observer shared, one in the observer frame of a redshift (cfg1kin with
                  coarser wavelength grids and frames)
  cfg3king        a rotating disk (cylindrical field) and a moving point source in dust that is steep in wavelength (cfg3kin likewise)
  cfg2bindeep     the binary tree of 36 levels, as it is
  cfg2bing        cfg2bin at 2e4 packets, 16^2 pixels
  cfg2binall      everything at once: a binary tree holding one electron component, panchromatic, a rotating disk of sources, three observers

Budget: no file larger than LARGEST bytes, everything of this generator below TOTAL bytes.  Every table (SED, SED statistics) is kept; the
cubes of a scene are kept instrument by instrument, in the ski file's order, as long as they fit (make_golden.py's "sed" scenes are the
precedent for a scene pinned by its tables alone).
"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")

SCENES = ("cfg1elecg", "cfg2agneleceag", "cfg1elecnfg", "cfg1king", "cfg3king", "cfg2bindeep", "cfg2bing", "cfg2binall")
LARGEST = 650 * 1000
TOTAL = 3 * 1000 * 1000


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    chosen = [s for s in SCENES if len(sys.argv) == 1 or s in sys.argv[1:]]
    # (what the scenes that are not regenerated hold already counts towards the budget)
    total = sum(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                if any(f.startswith(s + "_") for s in SCENES if s not in chosen) and (f.endswith(".fits") or f.endswith(".dat")) and "_rays" not in f)
    for name in chosen:
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        for f in os.listdir(HERE):
            if f.startswith(name + "_") and (f.endswith(".fits") or f.endswith("_sed.dat") or f.endswith("_sedstats.dat")):
                os.remove(os.path.join(HERE, f))
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", ski, "-t", "1", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
            files = sorted(f for f in os.listdir(tmp) if f.endswith(".fits") or f.endswith("_sed.dat") or f.endswith("_sedstats.dat"))
            tables = [f for f in files if f.endswith(".dat")]
            for f in tables:
                shutil.copy(os.path.join(tmp, f), os.path.join(HERE, f))
                total += os.path.getsize(os.path.join(tmp, f))
            # instruments in the ski file's order
            text = open(ski).read()
            import re
            for inst in re.findall(r'instrumentName="([^"]*)"', text):
                cubes = [f for f in files if f.startswith(f"{name}_{inst}_") and f.endswith(".fits")]
                size = sum(os.path.getsize(os.path.join(tmp, f)) for f in cubes)
                if not cubes:
                    continue
                if max(os.path.getsize(os.path.join(tmp, f)) for f in cubes) > LARGEST or total + size > TOTAL:
                    print(f"{name}: the cubes of instrument {inst} ({size} bytes) do not fit: tables only")
                    continue
                for f in cubes:
                    shutil.copy(os.path.join(tmp, f), os.path.join(HERE, f))
                total += size
        print(f"{name}: {total} bytes so far", flush=True)
    assert total <= TOTAL
    print("extended fixtures regenerated")


if __name__ == "__main__":
    main()
