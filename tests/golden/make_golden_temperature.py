#!/usr/bin/env python3
"""Regenerates the golden fixtures of the dust temperature scenes (TemperatureProbe with PerCellForm and ParallelProjectionForm,
DustAbsorptionPerCellProbe, RadiationFieldProbe) from the UNMODIFIED reference (oracle/_ref, built by `make -f oracle/Makefile.ref`), in the
manner of make_golden_probes.py.  Runs only where the reference build exists; the fixtures are data and are committed.

  python tests/golden/make_golden_temperature.py [scene ...]

The temperatures come from the radiation field, so the reference runs its photon packets here (skirt_ref run, no -e) on ONE thread (-t 1): the
single-thread random stream is the one the test oracle continues (tests/test_host_temperature.py), and with it the stored field -- and every
file made from it -- is reproduced byte for byte (FITS files apart from the DATE card).

Fixtures, per scene of tests/temperature_checks.GOLDEN_SCENES: the probe files alone -- <scene>_<probeName>_<fileid>.fits as written, the text
files gzipped without a time stamp -- not the instrument files nor the log.  <scene>_rf_J.dat.gz pins the field itself.  The scenes are small
(at most about 3100 cells), so every one keeps its per-cell files.

What the fixtures must show is asserted here, and again by the tests on the committed files: every per-cell temperature file has T > 0 in at
least 95 % of its cells, every map is nonzero in at least half of its pixels, and the file of the second dust component of cfg3mmtemp has
cells with and cells without a temperature.
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
import temperature_checks as T  # noqa: E402

MAX_BYTES = 300 * 1024


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -f oracle/Makefile.ref -j8")
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name in T.GOLDEN_SCENES:
        if only and name not in only:
            continue
        ski = os.path.join(ROOT, "tests", "ski", name + ".ski")
        probes = re.findall(r'<(?:TemperatureProbe|DustAbsorptionPerCellProbe|RadiationFieldProbe) probeName="([^"]+)"', open(ski).read())
        assert probes, name
        for old in os.listdir(HERE):
            if old.startswith(name + "_"):
                os.remove(os.path.join(HERE, old))
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([REF, "run", ski, "-t", "1", "-o", tmp], cwd=tmp, stdout=subprocess.DEVNULL)
            written = sorted(f for f in os.listdir(tmp) if any(f.startswith(f"{name}_{probe}_") for probe in probes))
            assert written, name
            for f in written:
                if f.endswith(".fits"):
                    shutil.copy(os.path.join(tmp, f), os.path.join(HERE, f))
                else:
                    with open(os.path.join(tmp, f), "rb") as src, open(os.path.join(HERE, f + ".gz"), "wb") as raw:
                        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as dst:  # (no time stamp: the same bytes every time)
                            dst.write(src.read())
        files = T.golden_files(name)
        assert sorted(files) == written
        for f, path in files.items():
            assert os.path.getsize(path) <= MAX_BYTES, (f, os.path.getsize(path))
        facts = T.assert_golden_is_meaningful(name)
        print(name, len(written), "files:", " ".join(written))
        for f, fact in facts.items():
            print("   ", f, fact)


if __name__ == "__main__":
    main()
