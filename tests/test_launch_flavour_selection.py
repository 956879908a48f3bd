"""The launch flavour of a source system (skirt9_amd/csrc/pmc_device.h pmcLaunchFlavourOf) is plain host code: a stand-alone program
(tools/launch_flavour_check.cpp) runs it on hand-filled source arrays, built with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess


from conftest import ROOT


def test_flavour_selection_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or "g++"
    exe = str(tmp_path / "launch_flavour_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "launch_flavour_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "launch flavour selection: ok" in run.stdout
