"""Scene creation's host code (skirt9_amd/csrc/pmc_scene_build.h, pmc_tables.h: validation, DevScene, every table that pmc_create puts on the
device) is plain host code: a stand-alone program (tools/scene_build_check.cpp) runs the stages of pmc_create on scene files through a sink that
hashes what it is given, checks the structural invariants of the tables, and breaks a scene one field at a time -- built with the address and
undefined-behaviour sanitizers.  The program is linked against libskirthost.so (which reads the scene file and is not sanitized).  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, ski
from skirt9_amd.host import Simulation


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or "g++"
    exe = str(tmp_path_factory.mktemp("scene_build") / "scene_build_check")
    libdir = os.path.join(ROOT, "skirt9_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "scene_build_check.cpp"), "-L" + libdir, "-lskirthost", "-pthread", "-Wl,-rpath," + libdir, "-o", exe])

    def run(scene_file, *options):
        done = subprocess.run([exe, scene_file, *options], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = done.stdout.splitlines()
        assert done.returncode == 0, done.stdout[-4000:]
        assert lines[-1] == "scene build: ok" and lines[-2].startswith("devscene "), done.stdout[-4000:]
        # (a clean sanitizer log: nothing but the sink's lines)
        assert all(line.split()[0] in ("upload", "allocate") for line in lines[:-2]), done.stdout[-4000:]
        return lines

    return run


def _scene_file(tmp_path, name):
    path = str(tmp_path / "scene.bin")
    Simulation(ski(name)).setup().save_scene(path)
    return path


# the smallest scenes of every path: Cartesian with one wavelength | octree | level 14, coordinate table not in LDS | binary tree | octree through
# the binary tree's tables | the octree's cells in shuffled groups of 32 (padding behind the last group) and in the caller's order | several
# components | Voronoi with four instruments, as it is, with runs whose count the link cannot name (the program
# checks that there are some), with the exact cull off
@pytest.mark.parametrize("name,options", [("cfg1.ski", ("--defects",)), ("cfg2small.ski", ()), ("cfg2deeper.ski", ()), ("cfg2bin.ski", ()),
                                          ("cfg2small.ski", ("--tree-as-bintree",)), ("cfg2small.ski", ("--cell-shuffle", "5")), ("cfg2small.ski", ("--cell-order-ref",)),
                                          ("cfg3mm.ski", ()), ("cfg5small.ski", ()),
                                          ("cfg5small.ski", ("--link-count-max", "4")), ("cfg5small.ski", ("--cone-cull-only",))])
def test_scene_tables_under_the_sanitizers(check, tmp_path, name, options):
    lines = check(_scene_file(tmp_path, name), *options)
    assert sum(line.startswith("allocate ") for line in lines) >= 2  # frames and counters at the least


@pytest.mark.parametrize("sites", [["0 0 0"], ["-5000 0 0", "5000 100 50"]])
def test_voronoi_cells_with_domain_walls_for_neighbours(check, tmp_path, sites):
    """one site, the fewest the host layer sets up (policy File): a cell whose neighbours are the six walls of the domain; and two: five walls and a site"""
    text = open(ski("cfg5small.ski")).read().replace('policy="Uniform" numSites="1500"', 'policy="File" filename="sites.txt"')
    (tmp_path / "sites.txt").write_text("\n".join(sites) + "\n")
    (tmp_path / "v.ski").write_text(text)
    path = str(tmp_path / "scene.bin")
    Simulation(str(tmp_path / "v.ski")).setup().save_scene(path)
    check(path)
