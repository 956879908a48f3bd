"""What tests/test_host_probes.py and tests/test_gpu_probes.py share: the path sum that defines a ray integral, the list of golden probe
scenes and the comparison of written probe files with the reference's (tests/golden/make_golden_probes.py)."""
import gzip
import os

import numpy as np

from conftest import golden

GOLDEN_SCENES = ["cfg1probe", "cfg2probe", "cfg2elecprobe", "cfg3probe", "cfg2binprobe"]


def path_sum(m, ds, q):
    """sum of ds * q[:, m] over the segments with m >= 0, in path order: one IEEE product and one IEEE sum per segment and value (numpy's
    element-wise operations do not contract); q: [V][num_cells]"""
    total = np.zeros(q.shape[0])
    for cell, length in zip(m.tolist(), ds.tolist()):
        if cell >= 0:
            total = total + length * q[:, cell]
    return total


def golden_files(name):
    """the reference's probe files of scene `name`: {file name as written: path of the fixture (text files gzipped)}"""
    found = {}
    for f in sorted(os.listdir(golden(""))):
        if not f.startswith(name + "_"):
            continue
        plain = f[:-3] if f.endswith(".gz") else f
        found[plain] = golden(f)
    return found


def _read(path):
    return gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()


def same_file(path_golden, path_written):
    """as tests/test_oracle_golden._same_file: all bytes, for a FITS file apart from the DATE card -- which is card 11 of a cube (offset 880,
    as there) and card 10 of a plain image, which has no NAXIS3 card (offset 800)"""
    a, b = bytearray(_read(path_golden)), bytearray(open(path_written, "rb").read())
    if path_written.endswith(".fits"):
        at = 880 if a[160:168] == b"NAXIS   " and a[160:240].split(b"/")[0].split(b"=")[1].strip() == b"3" else 800
        assert a[at:at + 8] == b"DATE    " and b[at:at + 8] == b"DATE    "
        a[at:at + 80] = b" " * 80
        b[at:at + 80] = b" " * 80
    return a == b


def assert_files_equal_golden(name, outdir, suffixes=(".fits", ".dat")):
    files = {f: p for f, p in golden_files(name).items() if f.endswith(suffixes)}
    assert files, name
    for f, path in files.items():
        written = os.path.join(outdir, f)
        assert os.path.exists(written), f
        assert same_file(path, written), f"{f} differs from the reference output"
    return sorted(files)
