"""The host model layer's reading and setup (skirt9_amd/host/ski_reader.cpp, simulation.cpp and what they call) under the address and
undefined-behaviour sanitizers: a stand-alone program (tools/ski_read_check.cpp) compiled together with the host sources -- not linked against
libskirthost.so, so every one of them is instrumented -- loads a ski file, sets it up and saves the scene.  It runs on the smallest scene of
every grid kind, where its scene file must be the one the library writes, and on broken variants, where the throw paths abandon a half-built
model: the refusal must be the expected one and the sanitizers' log empty.  Nothing here is loaded into python.  No GPU."""
import filecmp
import glob
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT, ski
from skirt9_amd.host import Simulation
from test_host_ski_refusals import ORDER, ROWS


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or "g++"
    build = tmp_path_factory.mktemp("ski_read")
    exe = str(build / "ski_read_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    sources = sorted(s for s in glob.glob(os.path.join(ROOT, "skirt9_amd", "host", "*.cpp")) if os.path.basename(s) != "main.cpp")
    sources.append(os.path.join(ROOT, "tools", "ski_read_check.cpp"))
    objects = [str(build / (os.path.basename(s)[:-4] + ".o")) for s in sources]
    # (one compiler per source at a time, a few at once: the sources together take two minutes in a row)
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda pair: subprocess.check_call([cxx, *flags, "-c", pair[0], "-o", pair[1]]), zip(sources, objects)))
    subprocess.check_call([cxx, *flags, *objects, "-pthread", "-o", exe])

    def run(ski_file, scene_file):
        done = subprocess.run([exe, ski_file, scene_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, SKH_INPUT_PATH=ski("")))
        assert done.returncode == 0, done.stdout[-4000:]
        lines = done.stdout.splitlines()
        assert len(lines) == 1, done.stdout[-4000:]  # (a clean sanitizer log: nothing but the program's one line)
        return lines[0]

    return run


# Cartesian | octree | binary tree | several components | Voronoi | imported particles | no medium | moving sources
@pytest.mark.parametrize("name", ["cfg1.ski", "cfg2small.ski", "cfg2bin.ski", "cfg3mm.ski", "cfg5small.ski", "cfg4small.ski", "cfg1nomed.ski", "cfg3kin.ski"])
def test_reading_and_setup_under_the_sanitizers(check, tmp_path, name):
    line = check(ski(name), str(tmp_path / "checked.bin"))
    assert line.startswith("ok ") and len(line) == 3 + 16, line
    Simulation(ski(name)).setup().save_scene(str(tmp_path / "library.bin"))
    assert filecmp.cmp(str(tmp_path / "checked.bin"), str(tmp_path / "library.bin"), shallow=False)


def _broken():
    """a handful of the refusal table's variants: throws from the depth of a source, a medium, a grid, an instrument and a probe, with the
    models read before them in place; from setup() with the grid built and the scene half flattened; and two of the rows with two defects"""
    wanted = ("SpheroidalGeometryDecorator of UniformBoxGeometry", "vector field HollowRadialVectorField", "SED must have at least two",
              "a moving source together with storeRadiationField", "ElectronMix in a ParticleMedium", "The mesh data file has negative points",
              "VoronoiMeshSpatialGrid lacks a filename", "Instrument distance and model redshift are both zero", "TemperatureProbe has no wavelengthGrid",
              "Cannot find a wavelength grid", "Wavelength distribution range does not overlap", "The total luminosity of the source system is zero",
              "Theta should be between 0 and pi.")
    rows = [next(row for row in ROWS if part in row[2]) for part in wanted]
    return rows + [ORDER[0], ORDER[-1]]


@pytest.mark.parametrize("fixture,edits,message", _broken(), ids=["%d-%s" % (index, row[0][:-4]) for index, row in enumerate(_broken())])
def test_refusals_under_the_sanitizers(check, tmp_path, fixture, edits, message):
    text = open(ski(fixture)).read()
    for old, new in edits:
        text = old.sub(new, text, count=1) if hasattr(old, "sub") else text.replace(old, new, 1)
    (tmp_path / fixture).write_text(text)
    assert check(str(tmp_path / fixture), str(tmp_path / "scene.bin")) == "refused: " + message
