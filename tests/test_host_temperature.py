"""The host layer of the dust temperature probes (skirt9_amd/host/temperature.cpp, probes.cpp), without a GPU: the files it writes against the
files of the UNMODIFIED reference (tests/golden/make_golden_temperature.py), byte for byte.  The radiation field comes from the test oracle run
with the reference's random stream, the averages along the rays of the maps from a Python callable over the oracle's ray segments; the
temperatures are computed by the host's restatement of the engine's kernel.  tests/test_gpu_temperature.py repeats the comparison with the
engine."""
import hashlib
import os

import numpy as np
import pytest

import probe_checks as P
import temperature_checks as T
from conftest import ski
from skirt9_amd import host
from skirt9_amd.host import Simulation


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", T.GOLDEN_SCENES)
def test_the_fixtures_show_what_they_are_meant_to_show(name):
    facts = T.assert_golden_is_meaningful(name)
    assert len(facts) >= 6
    for f, path in T.golden_files(name).items():
        assert os.path.getsize(path) <= 300 * 1024, f


@pytest.mark.parametrize("name", T.GOLDEN_SCENES)
def test_every_probe_file_is_the_reference_s(name, tmp_path):
    """_T.dat, _T.fits, _Labs.dat and _J.dat, byte for byte (FITS: apart from the DATE card); nothing else is written"""
    sim, rf = T.oracle_field(name)
    assert rf.min() >= 0 and rf.max() > 0
    sim.write_radiation_field(rf, str(tmp_path))
    sim.write_probes(str(tmp_path), weighted=T.oracle_weighted_integrator(sim), rf=rf)
    files = P.assert_files_equal_golden(name, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == files
    maps = sim.probe_maps()
    assert all(m["averaged"] and m["num_values"] == 1 and not m["after_setup"] for m in maps)
    assert sorted(f for f in files if f.endswith(".fits")) == sorted(m["file_name"] for m in maps)


def test_temperatures_can_come_from_a_callable(tmp_path):
    """the `temperatures` callable stands where the engine's pmc_dust_temperatures stands: with the numpy restatement in its place the files
    are the same; and probes with probeAfter Run are not written with the Setup probes"""
    sim, rf = T.oracle_field("cfg3mmtemp")
    sim.write_probes(str(tmp_path / "setup"), when="Setup")
    assert os.listdir(tmp_path / "setup") == []
    seen = []

    def temperatures(tables):
        seen.append(tables["sigma"].shape)
        return T.numpy_temperatures(tables, rf)

    sim.write_probes(str(tmp_path / "run"), weighted=T.oracle_weighted_integrator(sim), temperatures=temperatures, rf=rf, when="Run")
    assert seen == [(2, 6)]
    assert len(P.assert_files_equal_golden("cfg3mmtemp", str(tmp_path / "run"), suffixes=("_T.dat", "_T.fits", "_Labs.dat"))) == 7


def test_what_a_probe_needs_must_be_handed_over(tmp_path):
    sim, rf = T.oracle_field("cfg1temp")
    with pytest.raises(RuntimeError, match="needs the radiation field"):
        sim.write_probes(str(tmp_path))
    with pytest.raises(RuntimeError, match="needs an integrator"):
        sim.write_probes(str(tmp_path), rf=rf)

    def broken(r, k, w, q):
        raise ZeroDivisionError("no averages today")

    with pytest.raises(ZeroDivisionError):
        sim.write_probes(str(tmp_path), weighted=broken, rf=rf)


@pytest.mark.parametrize("name", ["cfg3mmtemp", "cfg1temp"])
def test_host_temperatures_equal_the_numpy_restatement(name):
    """skh_dust_temperatures on the simulation's own tables, on the oracle's field and on random tables and fields: bit for bit"""
    sim, rf = T.oracle_field(name)
    tables = sim.temperature_tables()
    H = len(sim.dust_components())
    assert tables["sigma"].shape == (H, 6) and tables["planckabs"].shape == (H, 1001)
    out = sim.dust_temperatures(rf)
    assert out.shape == (H + 1, tables["cell_factor"].size)
    assert np.array_equal(_bits(out), _bits(T.numpy_temperatures(tables, rf)))
    assert np.array_equal(_bits(out), _bits(host.dust_temperatures(tables, rf)))
    if name == "cfg3mmtemp":
        # electrons have no row; where the second dust component has no mass it has no temperature and the aggregate is the first's
        assert sim.dust_components() == [0, 1]
        empty = tables["mass_density"][1] == 0
        assert empty.any() and (~empty).any() and np.all(out[1][empty] == 0.)
        assert np.array_equal(_bits(out[2][empty]), _bits(((tables["mass_density"][0] * out[0]) / tables["mass_density"][0])[empty]))
    cells = tables["cell_factor"].size
    for H2, L, seed in ((1, 1, 3), (2, 6, 4), (4, 65, 5)):
        random = T.random_tables(cells, L, H2, seed)
        field = np.random.default_rng(seed).random(cells * L) * 1e30
        field, spots = T.special_rows(random, field, seed)
        got = host.dust_temperatures(random, field)
        assert np.array_equal(_bits(got), _bits(T.numpy_temperatures(random, field))), (H2, L)
        assert np.all(got[:, spots["zero"]] == 0.)
        assert np.all(got[0][spots["hot"]] == 5000.)
        first = random["temperature"][1]
        assert np.all((got[0][spots["faint"]] > 0.) & (got[0][spots["faint"]] < first))
        nodes = [100, 137, 174]  # (an input that equals a node gives the node's temperature)
        assert [got[0][m] for m in spots["node"]] == [random["temperature"][i] for i in nodes]


def test_temperature_grid_and_planck_table():
    """NR::buildPowerLawGrid(0, 5000, 1000, 500): T_i = 5000 (1 - q^i) / (1 - q^1000) with q = 500^(1/999); the Planck-integrated
    absorption rises with the temperature"""
    sim = Simulation(ski("cfg3temp.ski")).setup()
    tables = sim.temperature_tables()
    Tv = tables["temperature"]
    q = 500. ** (1. / 999.)
    assert Tv.size == 1001 and Tv[0] == 0. and Tv[1000] == 5000.
    for i in (1, 500, 1000):
        assert abs(Tv[i] - 5000. * (1. - q ** i) / (1. - q ** 1000)) <= 1e-12 * Tv[i]
    assert abs((Tv[1000] - Tv[999]) / (Tv[1] - Tv[0]) / 500. - 1.) < 1e-9
    planck = tables["planckabs"]
    assert planck.shape == (1, 1001) and planck[0, 0] == 0.
    assert np.all(np.diff(planck[0, 1:]) > 0) and planck[0, 1] > 0
    # the cross sections on the field grid: log-log interpolation of the mix's list (a power law between its nodes)
    assert np.all(tables["sigma"] > 0) and np.all(np.diff(tables["sigma"][0]) < 0)
    assert np.all(tables["width"] > 0) and np.all(tables["cell_factor"] > 0)


PER_CELL = '<form type="Form"><PerCellForm/></form>'
TEMPERATURE = '<TemperatureProbe probeName="t" %s>%s</TemperatureProbe>'


def _variant(tmp_path, base, edit):
    text = edit(open(ski(base + ".ski")).read())
    folder = tmp_path / f"v{len(os.listdir(tmp_path))}"
    folder.mkdir()
    path = folder / "refused.ski"
    path.write_text(text)
    return str(path)


def _with_probes(text, probes):
    a, b = text.index("<probeSystem"), text.index("</probeSystem>") + len("</probeSystem>")
    return text[:a] + '<probeSystem type="ProbeSystem"><ProbeSystem><probes type="Probe">' + probes + "</probes></ProbeSystem></probeSystem>" + text[b:]


@pytest.mark.parametrize("base,probes,named", [
    ("cfg1", TEMPERATURE % ("", PER_CELL), "TemperatureProbe"),  # (oligochromatic, no field)
    ("cfg1rf", TEMPERATURE % ("", PER_CELL), "TemperatureProbe"),  # (oligochromatic with a field)
    ("cfg3", TEMPERATURE % ("", PER_CELL), "TemperatureProbe"),  # (panchromatic without a field)
    ("cfg1", '<DustAbsorptionPerCellProbe probeName="a"/>', "DustAbsorptionPerCellProbe"),
    ("cfg1rf", '<DustAbsorptionPerCellProbe probeName="a"/>', "DustAbsorptionPerCellProbe"),
    ("cfg3", '<DustAbsorptionPerCellProbe probeName="a"/>', "DustAbsorptionPerCellProbe"),
    ("cfg3rf", TEMPERATURE % ('probeAfter="Setup"', PER_CELL), "TemperatureProbe probeAfter Setup"),
    ("cfg3rf", TEMPERATURE % ('probeAfter="Primary"', PER_CELL), "TemperatureProbe probeAfter Primary"),
    ("cfg3rf", TEMPERATURE % ('probeAfter="Secondary"', PER_CELL), "TemperatureProbe probeAfter Secondary"),
    ("cfg3rf", TEMPERATURE % ('aggregation="Fragment"', PER_CELL), "TemperatureProbe aggregation Fragment"),
    ("cfg3rf", TEMPERATURE % ("", ""), "TemperatureProbe form DefaultCutsForm"),  # (the default form)
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><DefaultCutsForm/></form>'), "TemperatureProbe form DefaultCutsForm"),
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><AllSkyProjectionForm/></form>'), "TemperatureProbe form AllSkyProjectionForm"),
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><PlanarCutsForm/></form>'), "TemperatureProbe form PlanarCutsForm"),
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><LinearCutForm/></form>'), "TemperatureProbe form LinearCutForm"),
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><MeridionalCutForm/></form>'), "TemperatureProbe form MeridionalCutForm"),
    ("cfg3rf", TEMPERATURE % ("", '<form type="Form"><AtPositionsForm filename="p.txt"/></form>'), "TemperatureProbe form AtPositionsForm"),
    ("cfg3rf", '<DustAbsorptionPerCellProbe probeName="a" writeWavelengthGrid="true"/>', "DustAbsorptionPerCellProbe writeWavelengthGrid"),
    ("cfg3rf", '<VelocityProbe probeName="v">' + PER_CELL + "</VelocityProbe>", "VelocityProbe"),
    ("cfg3rf", '<MagneticFieldProbe probeName="b">' + PER_CELL + "</MagneticFieldProbe>", "MagneticFieldProbe"),
])
def test_what_is_out_of_scope_is_refused_by_name(base, probes, named, tmp_path):
    path = _variant(tmp_path, base, lambda t: _with_probes(t, probes))
    with pytest.raises(RuntimeError) as err:
        Simulation(path)
    assert named in str(err.value) and "not supported" in str(err.value)


def test_the_default_of_probe_after_is_run(tmp_path):
    """SpatialGridWhenFormProbe.hpp:31"""
    path = _variant(tmp_path, "cfg3rf", lambda t: _with_probes(t, TEMPERATURE % ("", PER_CELL)))
    sim = Simulation(path, num_packets=10).setup()
    rf = np.ones(sim.radiation_field_size)
    sim.write_probes(str(tmp_path / "setup"), rf=rf, when="Setup")
    sim.write_probes(str(tmp_path / "run"), rf=rf, when="Run")
    assert os.listdir(tmp_path / "setup") == [] and os.listdir(tmp_path / "run") == ["refused_t_dust_T.dat"]


def test_a_simulation_without_dust_writes_nothing(tmp_path):
    """TemperatureProbe.cpp:45, DustAbsorptionPerCellProbe.cpp:27 (MediumSystem::hasDust): cfg3temp with free electrons in the place of its
    dust has no dust component, no map, needs no field and writes no temperature and no absorbed luminosity"""
    import re
    electrons = ('<materialMix type="MaterialMix"><ElectronMix includePolarization="false" includeThermalDispersion="false" '
                 'defaultTemperature="1e4 K"/></materialMix><normalization type="MaterialNormalization"><NumberMaterialNormalization '
                 'number="8e67"/></normalization>')
    pattern = (r'<materialMix type="MaterialMix"><MeanListDustMix[^>]*/></materialMix>\s*<normalization type="MaterialNormalization">'
               r"<OpticalDepthMaterialNormalization[^>]*/></normalization>")
    path = _variant(tmp_path, "cfg3temp", lambda t: re.sub(pattern, electrons, t))
    assert "ElectronMix" in open(path).read() and "MeanListDustMix" not in open(path).read()
    sim = Simulation(path, num_packets=10).setup()
    assert sim.radiation_field_size > 0 and sim.dust_components() == [] and sim.probe_maps() == []
    assert host.lib().skh_probes_need_radiation_field(sim._h, -1) == 0
    with pytest.raises(RuntimeError, match="has a dust component"):
        sim.temperature_tables()
    sim.write_probes(str(tmp_path / "out"))
    sim.write_probes(str(tmp_path / "out"), rf=np.ones(sim.radiation_field_size))
    assert os.listdir(tmp_path / "out") == []


def test_the_field_is_fetched_only_for_the_probes_that_read_it(tmp_path):
    """write_probes with an engine copies the radiation field table to the host only when a TemperatureProbe or DustAbsorptionPerCellProbe
    is among the probes it writes, and asks only then for the entry points that an older engine lacks"""
    class Recorder:
        radiation_field_size = 0
        asked = []

        def integrate_callback(self):
            self.asked.append("integrate")
            return None, None

        def download_radiation_field(self):
            self.asked.append("download")
            return np.ones(self.radiation_field_size)

    # a scene that stores the field and has density probes only
    density = '<DensityProbe probeName="d" probeAfter="Run">' + PER_CELL + "</DensityProbe>"
    sim = Simulation(_variant(tmp_path, "cfg3temp", lambda t: _with_probes(t, density)), num_packets=10).setup()
    assert host.lib().skh_probes_need_radiation_field(sim._h, -1) == 0
    old = Recorder()
    old.radiation_field_size = sim.radiation_field_size
    sim.write_probes(str(tmp_path / "density"), old)
    assert old.asked == ["integrate"] and os.listdir(tmp_path / "density") == ["refused_d_dust_rho.dat"]
    # cfg1temp: its probes are written after the run and read the field
    sim, rf = T.oracle_field("cfg1temp")
    need = host.lib().skh_probes_need_radiation_field
    assert (need(sim._h, 0), need(sim._h, 1), need(sim._h, -1)) == (0, 1, 1)
    Recorder.asked = []
    engine = Recorder()
    engine.radiation_field_size = sim.radiation_field_size
    sim.write_probes(str(tmp_path / "setup"), engine, when="Setup")
    assert engine.asked == ["integrate"]
    with pytest.raises(RuntimeError, match="needs an integrator"):  # (no weighted integrator in this engine: the per-cell files come first)
        sim.write_probes(str(tmp_path / "run"), engine, when="Run")
    assert engine.asked == ["integrate", "integrate", "download"]
    assert "cfg1temp_tc_dust_T.dat" in os.listdir(tmp_path / "run")


# sha256 of the scene files (skh_scene_save: every table the engine gets) at the commit before the temperature probes
SCENE_DIGESTS = {
    "cfg1": "4e7d2e36140f8ff36ea5fb83253dfd3281b83d0e9da4b5ae4a416020ca27dfc6",
    "cfg3rf": "4b2922d12e3854e29b55c94cb80554c2be57214877de6e9a33ae21d19119ae23",
}


@pytest.mark.parametrize("name", sorted(SCENE_DIGESTS))
def test_scenes_without_these_probes_are_what_they_were(name, tmp_path):
    sim = Simulation(ski(name + ".ski")).setup()
    target = str(tmp_path / "scene.bin")
    sim.save_scene(target)
    assert hashlib.sha256(open(target, "rb").read()).hexdigest() == SCENE_DIGESTS[name]
