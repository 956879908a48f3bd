"""The host layer of the density and opacity probes (skirt9_amd/host/probes.cpp), without a GPU: the files it writes against the files of the
UNMODIFIED reference (tests/golden/make_golden_probes.py), byte for byte.  The line integrals of the projected maps come from a Python callable
here -- the sum of ds * q[m] over the segments of oracle_lib.trace_ray --, so that rays, sub-sample averaging, unit factors and headers are
proven on the CPU; tests/test_gpu_probes.py repeats the comparison with the engine's integrator."""
import hashlib
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import probe_checks as P
from conftest import ski
from skirt9_amd.host import Simulation


def _variant(tmp_path, base, name, edit):
    """a copy of tests/ski/<base>.ski, edited, as <tmp>/<sub>/<name>.ski (the file name is the prefix of the output files)"""
    text = edit(open(ski(base + ".ski")).read())
    folder = tmp_path / f"v{len(os.listdir(tmp_path))}"
    folder.mkdir()
    path = folder / (name + ".ski")
    path.write_text(text)
    return str(path)


def _with_probes(text, probes):
    empty = '<probeSystem type="ProbeSystem"><ProbeSystem/></probeSystem>'
    assert empty in text
    return text.replace(empty, '<probeSystem type="ProbeSystem"><ProbeSystem><probes type="Probe">' + probes + '</probes></ProbeSystem></probeSystem>')


PROJECTION = ('<form type="Form"><ParallelProjectionForm inclination="30 deg" fieldOfViewX="2 pc" numPixelsX="4" fieldOfViewY="2 pc" '
              'numPixelsY="4"/></form>')


@pytest.mark.parametrize("name", [n for n in P.GOLDEN_SCENES if any(f.endswith(".dat") for f in P.golden_files(n))])
def test_per_cell_files_are_the_reference_s(name, tmp_path):
    """the scene without its projected probes, written without an integrator: cell values, unit factors and the text format, no ray involved"""
    path = _variant(tmp_path, name, name, lambda t: re.sub(r"\n\s*<(DensityProbe|OpacityProbe)[^\n]*<ParallelProjectionForm[^\n]*", "", t))
    assert "ParallelProjectionForm" not in open(path).read() and "PerCellForm" in open(path).read()
    sim = Simulation(path).setup()
    assert sim.probe_maps() == []
    out = tmp_path / "out"
    sim.write_probes(str(out))
    assert len(P.assert_files_equal_golden(name, str(out), suffixes=(".dat",))) >= 2


def test_some_scene_has_per_cell_goldens():
    assert any(f.endswith(".dat") for n in P.GOLDEN_SCENES for f in P.golden_files(n))


@pytest.mark.parametrize("name", P.GOLDEN_SCENES)
def test_all_probe_files_are_the_reference_s(name, tmp_path):
    """write_probes with a callable that integrates along the oracle's ray segments: every file of the scene, every pixel"""
    sim = Simulation(ski(name + ".ski")).setup()
    calls = []

    def integrate(origins, directions, cell_values):
        calls.append(len(origins))
        sums = np.zeros((len(origins), cell_values.shape[0]))
        for i in range(len(origins)):
            m, ds = O.trace_ray(sim, origins[i], directions[i], cap=65536)
            assert len(m) < 65536
            sums[i] = P.path_sum(m, ds, cell_values)
        return sums

    sim.write_probes(str(tmp_path), integrate)
    files = P.assert_files_equal_golden(name, str(tmp_path))
    maps = sim.probe_maps()
    assert sorted(f for f in files if f.endswith(".fits")) == sorted(m["file_name"] for m in maps)
    assert calls == [m["num_rays"] for m in maps]
    assert sorted(os.listdir(tmp_path)) == files  # (nothing else is written)


def test_setup_and_run_probes_are_written_apart(tmp_path):
    """probeAfter: the driver writes the Setup probes before the photon loop and the others after it; together they are all files"""
    sim = Simulation(ski("cfg1probe.ski")).setup()
    zeros = lambda r, k, q: np.zeros((len(r), q.shape[0]))  # noqa: E731
    sim.write_probes(str(tmp_path / "setup"), zeros, when="Setup")
    sim.write_probes(str(tmp_path / "run"), zeros, when="Run")
    assert sorted(os.listdir(tmp_path / "setup")) == ["cfg1probe_dns_dust_rho.dat", "cfg1probe_opc_k.dat"]
    assert sorted(os.listdir(tmp_path / "run")) == ["cfg1probe_dnp_dust_Sigma.fits", "cfg1probe_opp_tau.fits"]
    assert [m["after_setup"] for m in sim.probe_maps()] == [False, False]


def test_a_failing_integrator_is_an_error(tmp_path):
    sim = Simulation(ski("cfg1probe.ski")).setup()

    def broken(r, k, q):
        raise ZeroDivisionError("no integrals today")

    with pytest.raises(ZeroDivisionError):
        sim.write_probes(str(tmp_path), broken)
    with pytest.raises(RuntimeError, match="needs an integrator"):
        sim.write_probes(str(tmp_path))


def test_the_four_entry_points_write_the_same_files(tmp_path):
    """skh_write_probes, skh_write_probes_when(-1), skh_write_probes_with and skh_write_probes_sampled without a sampler, each with the same
    Python integrator handed over as a C function: the same set of files with the same bytes (the DATE card of a FITS file, a time stamp,
    apart as everywhere)"""
    import ctypes as C
    from skirt9_amd import host as H
    sim = Simulation(ski("cfg1probe.ski")).setup()
    num_cells = int(H.scene_head(sim).grid.num_cells)
    calls = []

    def integrate(_, n, origins, directions, num_values, values, sums):
        r = np.ctypeslib.as_array(origins, shape=(n, 3))
        k = np.ctypeslib.as_array(directions, shape=(n, 3))
        q = np.ctypeslib.as_array(values, shape=(num_values, num_cells))
        calls.append(n)
        np.ctypeslib.as_array(sums, shape=(n, num_values))[:] = ((r * k) @ np.array([1., 2., 3.]))[:, None] * q.sum(axis=1)[None, :]
        return 0

    fn = H.INTEGRATE_FN(integrate)
    pointer = C.cast(fn, C.c_void_p)
    engine = H.ProbeEngine()
    engine.integrate = pointer
    L = H.lib()
    out = [str(tmp_path / name) for name in ("plain", "when", "with", "sampled")]
    for folder in out:
        os.makedirs(folder)
    assert L.skh_write_probes(sim._h, pointer, None, os.fsencode(out[0])) == 0
    assert L.skh_write_probes_when(sim._h, pointer, None, os.fsencode(out[1]), -1) == 0
    assert L.skh_write_probes_with(sim._h, C.byref(engine), os.fsencode(out[2]), -1) == 0
    assert L.skh_write_probes_sampled(sim._h, C.byref(engine), None, os.fsencode(out[3]), -1) == 0
    maps = sim.probe_maps()
    assert calls == 4 * [m["num_rays"] for m in maps] and calls
    files = sorted(os.listdir(out[0]))
    assert files == sorted(["cfg1probe_dns_dust_rho.dat", "cfg1probe_opc_k.dat"] + [m["file_name"] for m in maps])
    for folder in out[1:]:
        assert sorted(os.listdir(folder)) == files
        for f in files:
            assert P.same_file(os.path.join(out[0], f), os.path.join(folder, f)), (folder, f)


def test_null_engine_rules_of_the_entry_points(tmp_path):
    """skh_write_probes_with refuses a null engine; skh_write_probes_sampled takes one (and no sampler) where no probe needs either"""
    from skirt9_amd import host as H
    path = _variant(tmp_path, "cfg1probe", "cfg1probe", lambda t: re.sub(r"\n\s*<(DensityProbe|OpacityProbe)[^\n]*<ParallelProjectionForm[^\n]*", "", t))
    sim = Simulation(path).setup()
    assert sim.probe_maps() == []
    L = H.lib()
    out = tmp_path / "out"
    out.mkdir()
    assert L.skh_write_probes_with(sim._h, None, os.fsencode(str(out)), -1) != 0
    assert "invalid argument" in L.skh_last_error().decode()
    assert os.listdir(out) == []
    assert L.skh_write_probes_sampled(sim._h, None, None, os.fsencode(str(out)), -1) == 0
    assert sorted(os.listdir(out)) == ["cfg1probe_dns_dust_rho.dat", "cfg1probe_opc_k.dat"]
    P.assert_files_equal_golden("cfg1probe", str(out), suffixes=(".dat",))


def _reference_rays(form, nx, ny, ns):
    """ParallelProjectionForm.cpp:22-51, 67-88 restated with numpy; form: angles in rad, lengths in m"""
    ct, st = np.cos(form["inclination"]), np.sin(form["inclination"])
    cp, sp = np.cos(form["azimuth"]), np.sin(form["azimuth"])
    co, so = np.cos(form["roll"]), np.sin(form["roll"])
    zp = 10. * (form["fovx"] + form["fovy"])
    j, i, a, b = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(ns), np.arange(ns), indexing="ij")
    xp = form["cx"] - 0.5 * form["fovx"] + (i + (a + 1.) / (ns + 1.)) * (form["fovx"] / nx)
    yp = form["cy"] - 0.5 * form["fovy"] + (j + (b + 1.) / (ns + 1.)) * (form["fovy"] / ny)
    xpp, ypp = so * xp - co * yp, co * xp + so * yp
    x = cp * ct * xpp - sp * ypp + cp * st * zp
    y = sp * ct * xpp + cp * ypp + sp * st * zp
    z = -st * xpp + ct * zp
    origins = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    return origins, np.array([-cp * st, -sp * st, -ct]), zp


def test_rays_follow_the_reference_s_transform():
    """origins to 1e-14 of zp, directions to 1e-15, nx * ny * sampling^2 rays ordered by pixel (j, i) and sub-sample (is, js)"""
    pc, deg = 3.08567758e16, np.pi / 180.
    sim = Simulation(ski("cfg1probe.ski")).setup()
    form = {"inclination": 60 * deg, "azimuth": 30 * deg, "roll": 15 * deg, "fovx": 2.8 * pc, "fovy": 2.2 * pc, "cx": 0.2 * pc, "cy": -0.1 * pc}
    maps = sim.probe_maps()
    assert [(m["nx"], m["ny"], m["sampling"], m["num_values"]) for m in maps] == [(7, 5, 2, 1), (7, 5, 2, 2)]
    for m in maps:
        origins, direction, zp = _reference_rays(form, 7, 5, 2)
        assert m["num_rays"] == 7 * 5 * 2 * 2 == len(m["origins"]) == len(m["directions"])
        assert np.abs(m["origins"] - origins).max() <= 1e-14 * zp
        assert np.abs(m["directions"] - direction).max() <= 1e-15
    sim = Simulation(ski("cfg2probe.ski")).setup()
    edge = sim.probe_maps()[1]
    assert (edge["nx"], edge["ny"], edge["sampling"], edge["num_rays"]) == (11, 5, 3, 11 * 5 * 9)
    form = {"inclination": 90 * deg, "azimuth": 0., "roll": 0., "fovx": 44000 * pc, "fovy": 9000 * pc, "cx": 0., "cy": 0.}
    origins, direction, zp = _reference_rays(form, 11, 5, 3)
    assert np.abs(edge["origins"] - origins).max() <= 1e-14 * zp
    assert np.abs(edge["directions"] - direction).max() <= 1e-15
    # the central sub-samples of the central row run in the mid-plane of the grid (z = 0 to rounding: cos 90 deg is 6e-17)
    central = edge["origins"].reshape(5, 11, 3, 3, 3)[2, :, :, 1, 2]
    assert np.abs(central).max() <= 1e-15 * zp


DENSITY = '<DensityProbe probeName="d" %s>%s</DensityProbe>'
CELLS = '<form type="Form"><PerCellForm/></form>'


@pytest.mark.parametrize("probes,named", [
    (DENSITY % ("", '<form type="Form"><AllSkyProjectionForm/></form>'), "AllSkyProjectionForm"),
    (DENSITY % ("", '<form type="Form"><DefaultCutsForm/></form>'), "DefaultCutsForm"),
    (DENSITY % ("", ""), "DefaultCutsForm"),  # (the default form)
    (DENSITY % ("", '<form type="Form"><PlanarCutsForm/></form>'), "PlanarCutsForm"),
    (DENSITY % ("", '<form type="Form"><LinearCutForm/></form>'), "LinearCutForm"),
    (DENSITY % ("", '<form type="Form"><MeridionalCutForm/></form>'), "MeridionalCutForm"),
    (DENSITY % ("", '<form type="Form"><AtPositionsForm filename="p.txt"/></form>'), "AtPositionsForm"),
    (DENSITY % ('aggregation="Fragment"', CELLS), "aggregation Fragment"),
    ('<OpacityProbe probeName="o" aggregation="Fragment">' + CELLS + "</OpacityProbe>", "aggregation Fragment"),
    (DENSITY % ('probeAfter="Primary"', CELLS), "probeAfter Primary"),
    (DENSITY % ('probeAfter="Secondary"', CELLS), "probeAfter Secondary"),
    ('<TemperatureProbe probeName="t">' + CELLS + "</TemperatureProbe>", "TemperatureProbe"),
    ('<VelocityProbe probeName="v">' + CELLS + "</VelocityProbe>", "VelocityProbe"),
    ('<MagneticFieldProbe probeName="b">' + CELLS + "</MagneticFieldProbe>", "MagneticFieldProbe"),
    ('<ImportedMediumDensityProbe probeName="i">' + CELLS + "</ImportedMediumDensityProbe>", "ImportedMediumDensityProbe"),
    ('<ImportedSourceLuminosityProbe probeName="i">' + CELLS + "</ImportedSourceLuminosityProbe>", "ImportedSourceLuminosityProbe"),
])
def test_what_is_out_of_scope_is_refused_by_name(probes, named, tmp_path):
    path = _variant(tmp_path, "cfg1", "refused", lambda t: _with_probes(t, probes))
    with pytest.raises(RuntimeError) as err:
        Simulation(path)
    assert named in str(err.value) and "not supported" in str(err.value)


def test_a_simulation_without_a_medium_writes_nothing(tmp_path):
    """DensityProbe.cpp:16, OpacityProbe.cpp:39"""
    probes = (DENSITY % ("", CELLS)) + '<OpacityProbe probeName="o" aggregation="System">' + PROJECTION + "</OpacityProbe>"
    path = _variant(tmp_path, "cfg1nomed", "nomed", lambda t: _with_probes(t, probes))
    sim = Simulation(path).setup()
    assert sim.probe_maps() == []
    sim.write_probes(str(tmp_path / "out"))
    assert os.listdir(tmp_path / "out") == []


def _scene_digest(path, tmp_path):
    sim = Simulation(path).setup()
    maps = sim.probe_maps()
    target = str(tmp_path / "scene.bin")
    sim.save_scene(target)
    return hashlib.sha256(open(target, "rb").read()).hexdigest(), maps


def test_scenes_without_probes_are_what_they_were(tmp_path):
    """cfg1.ski has no probe map; its scene file (skh_scene_save: every table the engine gets) has the same bytes before and after a copy with
    probes on the default grids was set up in the same process, and that copy's scene file has them too: probes that bring no wavelength
    grid of their own leave the dust tables alone.  A probe with its own grid adds its wavelengths (cfg3probe: the file differs)."""
    before, maps = _scene_digest(ski("cfg1.ski"), tmp_path)
    assert maps == []
    probes = (DENSITY % ("", PROJECTION)) + '<OpacityProbe probeName="o" aggregation="System">' + CELLS + "</OpacityProbe>"
    copy, maps = _scene_digest(_variant(tmp_path, "cfg1", "cfg1", lambda t: _with_probes(t, probes)), tmp_path)
    assert [m["file_name"] for m in maps] == ["cfg1_d_dust_Sigma.fits"]
    after, _ = _scene_digest(ski("cfg1.ski"), tmp_path)
    assert before == copy == after
    plain, _ = _scene_digest(_variant(tmp_path, "cfg3probe", "cfg3probe", lambda t: re.sub(r"<wavelengthGrid type=\"WavelengthGrid\"><ListWavelengthGrid[^>]*/></wavelengthGrid>", "", t)), tmp_path)
    own, _ = _scene_digest(ski("cfg3probe.ski"), tmp_path)
    assert plain != own
