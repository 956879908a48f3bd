"""The adaptive mesh import (skirt9_amd/host/adaptive_mesh.cpp, the column file reader of particles.cpp) under the address and
undefined-behaviour sanitizers: the stand-alone program of tests/test_ski_read_check.py (tools/ski_read_check.cpp compiled together with the host
sources), on the scene of the mesh fixture, where its scene file must be the one the library writes, and on three broken mesh files, where
the throw leaves a half-read tree behind.  Nothing here is loaded into python.  No GPU."""
import filecmp

import pytest

import amr_checks as A
from conftest import ski
from skirt9_amd.host import Simulation
from test_ski_read_check import check  # noqa: F401  (the module-scoped fixture that builds the program)


def test_mesh_scene_under_the_sanitizers(check, tmp_path):  # noqa: F811
    line = check(ski("cfg6amr.ski"), str(tmp_path / "checked.bin"))
    assert line.startswith("ok ") and len(line) == 3 + 16, line
    Simulation(ski("cfg6amr.ski")).setup().save_scene(str(tmp_path / "library.bin"))
    assert filecmp.cmp(str(tmp_path / "checked.bin"), str(tmp_path / "library.bin"), shallow=False)


@pytest.mark.parametrize("mesh_text,message", [
    ("! 2 2 2\n1\n2\n! 3 2 1\n4\n5\n", "Reached end of file in adaptive mesh data before all nodes were read"),
    ("! 2 1 1\n! 1 1 2\n1\n2\n! 2 two 2\n", "Nonleaf subdivision specifiers are missing or not formatted as integers"),
    ("! 1 2 1\n1\n2\n3\n", "Superfluous lines in adaptive mesh data after all nodes were read"),
], ids=["truncated", "not-integers", "superfluous"])
def test_broken_mesh_files_under_the_sanitizers(check, tmp_path, mesh_text, message):  # noqa: F811
    path = tmp_path / "broken_mesh.txt"
    path.write_text(mesh_text)
    scene = A.mesh_ski(tmp_path, "broken", str(path))
    assert check(scene, str(tmp_path / "scene.bin")) == "refused: " + message
