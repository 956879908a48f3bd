"""The measurement experiments of profiles/experiments that were taken out of the kernels (perturbation, ablation and
fold-octant builds) still apply to the tree, and the tree itself holds none of their macros."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "skirt9_amd", "csrc")
PATCHES = ["perturb_octree_step", "ablate_walk_side", "ablate_transition_side", "fold_octant"]
MOVED = ["PMC_ABLATE_", "PMC_PERTURB", "PMC_EXPERIMENT_FOLD_OCTANT", "PMC_EXPERIMENT_PROP_SGN0", "PMC_VORO_PAIRS", "PMC_VORO_RUN_SERIAL"]


@pytest.mark.skipif(shutil.which("git") is None, reason="git is not on the path")
@pytest.mark.parametrize("name", PATCHES)
def test_patch_applies_to_the_tree(name):
    patch = os.path.join("profiles", "experiments", name + ".patch")
    text = open(os.path.join(ROOT, patch)).read()
    assert "make variant NAME=" in text.split("diff --git")[0]  # (the header says how to build the patched tree)
    assert "+#define PMC_EXPERIMENT_BUILD 1\n" in text
    done = subprocess.run(["git", "apply", "--check", patch], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_tree_is_no_experiment_build():
    guards = []
    for name in sorted(os.listdir(CSRC)):
        for number, line in enumerate(open(os.path.join(CSRC, name), errors="replace"), 1):
            for macro in MOVED:
                assert macro not in line, f"{name}:{number}: {line.strip()}"
            if "PMC_EXPERIMENT_BUILD" in line:
                guards.append(line.strip())
    # the one guard that lets a patched tree identify itself; nothing in the tree defines the macro
    assert guards == ["#ifdef PMC_EXPERIMENT_BUILD"]
    assert "PMC_EXPERIMENT_BUILD" not in open(os.path.join(ROOT, "Makefile")).read()
    # a library that is already built says the same (the test builds nothing)
    path = os.path.join(ROOT, "skirt9_amd", "lib", "libpmc.so")
    if os.path.exists(path):
        assert C.CDLL(path).pmcExperimentBuild() == 0
