#!/usr/bin/env python3
"""Regenerates the golden fixtures of the probe scenes (DensityProbe, OpacityProbe; PerCellForm, ParallelProjectionForm) from the UNMODIFIED
reference (oracle/_ref, built by `make -f oracle/Makefile.ref`), as make_golden.py does for the other scenes.  Runs only where the
reference build exists; the fixtures are data and are committed.

  python tests/golden/make_golden_probes.py [scene ...]

The reference runs in emulation mode (skirt_ref run -e: setup, no photon packets, every probe written); the probes are deterministic, so
the files it writes are compared byte for byte (tests/test_host_probes.py, tests/test_gpu_probes.py; FITS files apart from the DATE card).

Fixtures, per scene of tests/probe_checks.GOLDEN_SCENES: the probe files alone -- <scene>_<probeName>_<fileid>.fits as written, the text
files <scene>_<probeName>_<fileid>.dat gzipped -- not the instrument files nor the log.  Only cfg1probe (3072 cells) has per-cell files: those
of the tree scenes would take hundreds of KB each.
"""
import gzip
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "release", "SKIRT", "main", "skirt_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_checks import GOLDEN_SCENES  # noqa: E402


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name in GOLDEN_SCENES:
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        probes = re.findall(r'<(?:DensityProbe|OpacityProbe) probeName="([^"]+)"', open(ski).read())
        assert probes, name
        for old in os.listdir(HERE):
            if old.startswith(name + "_"):
                os.remove(os.path.join(HERE, old))
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", "-e", ski, "-t", "1", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
            written = sorted(f for f in os.listdir(tmp) if any(f.startswith(f"{name}_{probe}_") for probe in probes))
            assert written, name
            for f in written:
                if f.endswith(".fits"):
                    shutil.copy(os.path.join(tmp, f), os.path.join(HERE, f))
                else:
                    with open(os.path.join(tmp, f), "rb") as src, open(os.path.join(HERE, f + ".gz"), "wb") as raw:
                        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as dst:  # (no time stamp: the same bytes every time)
                            dst.write(src.read())
            print(name, len(written), "files:", " ".join(written))


if __name__ == "__main__":
    main()
