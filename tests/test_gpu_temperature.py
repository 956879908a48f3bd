"""Dust temperatures from the stored radiation field (pmc_dust_temperatures) and the averages along rays behind the TemperatureProbe maps
(pmc_integrate_weighted_rays), on the MI355X.

The temperature kernel stages the rows of the radiation field table through LDS and lets every lane add up its own row in the order of the
reference: its results must EQUAL the host's restatement (skh_dust_temperatures) bit for bit, for every number of bins around the tile size, for
1, 2 and 4 dust components, and for the rows at which the table lookup takes another path.  The weighted integrator must equal the weighted sum
over pmc_trace_ray's segments bit for bit.  The files written through both are the reference's byte for byte
(tests/golden/make_golden_temperature.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import probe_checks as P
import temperature_checks as T
from conftest import ROOT, ski
from scene_variants import with_field_grid
from skirt9_amd import host
from skirt9_amd.engine import INTEGRATE_BATCH_RAYS, INTEGRATE_PASS_VALUES, Engine, clear_tuning, lib, set_tuning
from skirt9_amd.host import Simulation, scene_head

pytestmark = pytest.mark.gpu

# The radiation field tables of these tests are torch tensors bound with bind_radiation_field.  torch brings a HIP runtime of its own, and in a
# process in which the engine's runtime has opened the device first, torch finds none ("No HIP GPUs are available"); the other order works
# (bench.py, tools/sweep.py: torch first).  pytest imports every test module before it runs a test, so torch looks at the device here, ahead of
# the first Engine of any module.  Without a GPU this is a quick no.
TORCH_PROBLEM = None
try:
    import torch
except ImportError as error:
    TORCH_PROBLEM = f"torch cannot be imported: {error}"
else:
    if torch.cuda.is_available():
        try:
            torch.cuda.init()
        except RuntimeError as error:
            TORCH_PROBLEM = f"torch sees a GPU and cannot open it: {error}"
    else:
        TORCH_PROBLEM = "torch sees no GPU"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _bound_field(eng, rf):
    """rf in a torch tensor on the device, bound to the engine as its radiation field table"""
    assert TORCH_PROBLEM is None, f"the field tables of these tests are torch tensors: {TORCH_PROBLEM}"
    table = torch.from_numpy(np.array(rf, dtype=np.float64)).to("cuda:0")
    eng.bind_radiation_field(table.data_ptr(), table.numel())
    return table


# Cartesian (3072 cells), octree, binary tree, Voronoi (1500 cells); bins 1, 6, 64 and 65 (a tile holds 8); 1, 2 and 4 components
KERNEL_CASES = [("cfg1temp", 1, 1), ("cfg1temp", 6, 2), ("cfg1temp", 64, 4), ("cfg1temp", 65, 4), ("cfg3temp", 6, 1), ("cfg3temp", 65, 2),
                ("cfg2bintemp", 6, 4), ("cfg2bintemp", 64, 1), ("cfg5small", 6, 2), ("cfg5small", 65, 4), ("cfg5small", 1, 1)]


@pytest.mark.parametrize("base,bins,components", KERNEL_CASES)
def test_kernel_equals_the_host_restatement(base, bins, components, tmp_path):
    """on tables bound with bind_radiation_field: random positive rows, and in cell 0, in the last cell and at indices that are no multiple of
    64 an all-zero row (T = 0), a row above the table (exactly 5000 K), a row below its first node and a row that hits a node exactly; which
    kinds sit in cell 0 and in the last cell turns from case to case, so that over the cases every kind has been in both"""
    turn = KERNEL_CASES.index((base, bins, components))
    sim = Simulation(with_field_grid(tmp_path, base, bins), num_packets=100).setup()
    cells = scene_head(sim).grid.num_cells
    assert sim.radiation_field_size == cells * bins
    tables = T.random_tables(cells, bins, components, seed=bins * 10 + components)
    rf = np.random.default_rng(bins).random(cells * bins) * 1e30
    rf, spots = T.special_rows(tables, rf, seed=turn)
    assert 0 in spots[list(spots)[turn % 4]] and cells - 1 in spots[list(spots)[(turn + 1) % 4]]
    want = host.dust_temperatures(tables, rf)
    # (from the restatement alone: the rows do what they are meant to do)
    assert np.all(want[:, spots["zero"]] == 0.) and np.all(want[0][spots["hot"]] == 5000.)
    assert np.all((want[0][spots["faint"]] > 0.) & (want[0][spots["faint"]] < tables["temperature"][1]))
    assert [want[0][m] for m in spots["node"]] == [tables["temperature"][i] for i in (100, 137, 174)]
    assert (want[:components] > 0).mean() > 0.6
    eng = Engine(sim.scene, 0)
    table = _bound_field(eng, rf)
    got = eng.dust_temperatures(tables)
    assert got.shape == (components + 1, cells)
    assert _same_bits(got, want), (base, bins, components, int((_bits(got) != _bits(want)).sum()))
    # the simulation's own tables (one dust component) on the same field
    own = sim.temperature_tables()
    assert _same_bits(eng.dust_temperatures(own), sim.dust_temperatures(rf))
    assert eng.last_temperature_ms() > 0.
    del table
    eng.close()


def test_argument_errors_are_reported(tmp_path):
    sim = Simulation(ski("cfg1temp.ski"), num_packets=100).setup()
    tables = sim.temperature_tables()
    eng = Engine(sim.scene, 0)
    wrong = dict(tables, width=tables["width"][:5], sigma=tables["sigma"][:, :5])
    with pytest.raises(RuntimeError, match="do not match"):
        eng.dust_temperatures(wrong)
    cells = tables["cell_factor"].size
    five = T.random_tables(cells, 6, 5, seed=1)
    with pytest.raises(RuntimeError, match="pmc error -2"):
        eng.dust_temperatures(five)
    assert lib().pmc_dust_temperatures(eng._h, None, None) == -1
    assert lib().pmc_integrate_weighted_rays(eng._h, 1, None, None, 1, None, None, None) == -1 and b"null" in lib().pmc_last_error()
    eng.close()
    plain = Simulation(ski("cfg1.ski"), num_packets=100).setup()  # (stores no field)
    eng = Engine(plain.scene, 0)
    with pytest.raises(RuntimeError, match="does not store the radiation field"):
        eng.dust_temperatures(tables)
    eng.close()


@pytest.mark.parametrize("name", ["cfg3temp", "cfg3mmtemp"])
def test_after_a_run_the_engine_s_temperatures_are_the_host_s(name):
    """2e4 packets; again after a second segment has accumulated more"""
    sim = Simulation(ski(name + ".ski")).setup()
    n = sim.num_packets
    assert n == 20000
    tables = sim.temperature_tables()
    eng = Engine(sim.scene, 0)
    before = None
    for segment in range(2):
        eng.run_primary(segment * n, n, sim.seed)
        gpu = eng.dust_temperatures(tables)
        rf = eng.download_radiation_field()
        assert _same_bits(gpu, sim.dust_temperatures(rf)), (name, segment)
        assert (gpu[-1] > 0).mean() >= 0.95
        if before is not None:
            assert not np.array_equal(gpu, before)  # (the second segment has changed the field)
        before = gpu
    if name == "cfg3mmtemp":
        assert gpu.shape[0] == 3 and (gpu[1] == 0).any() and (gpu[1] > 0).any()
    eng.close()


# ---- averages along rays

RAY_SCENES = ["cfg1", "cfg2small", "cfg2deep", "cfg2bin", "cfg5small"]  # Cartesian, octree (10-bit indices), octree (21-bit), binary tree, Voronoi
V = INTEGRATE_PASS_VALUES  # the weight and three values fill a pass: four values take two
NUM_RAYS = 1000
CAP = 65536


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sim, origins, directions, weights [num_cells], values [V][num_cells], reference sums [NUM_RAYS][1 + V]): the rays of
    tests/test_gpu_probes.py; the reference is the weighted sum over Engine.trace_ray's segments, computed once per scene"""
    from test_gpu_probes import _rays
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    r, k = _rays(sim)
    num_cells = scene_head(sim).grid.num_cells
    rng = np.random.default_rng(17)
    w = rng.random(num_cells) + 0.5
    w[::7] = 0.  # (cells without weight)
    q = rng.random((V, num_cells)) * 10. + 0.5
    eng = Engine(sim.scene, 0)
    ref = np.zeros((NUM_RAYS, 1 + V))
    last = None
    for i in range(NUM_RAYS):
        if last is not None and np.array_equal(r[i], r[last]) and np.array_equal(k[i], k[last]):
            ref[i] = ref[last]
            continue
        m, ds = eng.trace_ray(r[i], k[i], cap=CAP)
        assert len(m) < CAP
        ref[i] = T.weighted_path_sum(m, ds, w, q)
        last = i
    eng.close()
    for a in (r, k, w, q, ref):
        a.setflags(write=False)
    return sim, r, k, w, q, ref


@pytest.mark.parametrize("name", RAY_SCENES)
def test_weighted_sums_equal_the_sum_over_the_traced_segments(name):
    """bit for bit, for 0, 1, 63, 64, 65 and 1000 rays, for 1 and 4 values, for permuted rays; all-zero weights give all-zero sums"""
    sim, r, k, w, q, ref = _case(name)
    assert (ref[:, 0] == 0).sum() >= 50 and (ref[:, 0] > 0).sum() > 500
    eng = Engine(sim.scene, 0)
    for n in (0, 1, 63, 64, 65, NUM_RAYS):
        first = 0 if n == NUM_RAYS else 32  # (a window over the end of the identical rays and the start of the random ones)
        sel = slice(first, first + n)
        many = eng.integrate_weighted_rays(r[sel], k[sel], w, q)
        assert many.shape == (n, 1 + V)
        assert _same_bits(many, ref[sel]), (name, n, int((many != ref[sel]).sum()))
        one = eng.integrate_weighted_rays(r[sel], k[sel], w, q[0])
        assert one.shape == (n, 2)
        assert _same_bits(one, ref[sel, :2]), (name, n)
    work = eng.last_integrate_work()
    assert work["lane_steps"] > 0 and 0 < work["wave_steps"] <= work["lane_steps"]
    perm = np.random.default_rng(11).permutation(NUM_RAYS)
    assert _same_bits(eng.integrate_weighted_rays(r[perm], k[perm], w, q), ref[perm])
    assert np.all(eng.integrate_weighted_rays(r, k, np.zeros_like(w), q) == 0.)
    # the plain integrals of the same context are what they were: the weights as the only value
    plain = eng.integrate_rays(r, k, w)
    assert _same_bits(plain, ref[:, 0])
    eng.close()


def test_more_weighted_rays_than_one_batch():
    """INTEGRATE_BATCH_RAYS + 65 rays on cfg5small (1500 cells: the smallest grid of RAY_SCENES), the ray set tiled (ray i = set[i % NUM_RAYS]), V values: two
    batches -- the second a wave and one lane -- of two passes each, a pass the weight and three values.  The sum of the weights is taken
    from the first pass, in the first batch and in the second"""
    sim, r, k, w, q, ref = _case("cfg5small")
    tile =np.arange(INTEGRATE_BATCH_RAYS + 65) % NUM_RAYS
    eng = Engine(sim.scene, 0)
    sums = eng.integrate_weighted_rays(r[tile], k[tile], w, q)
    eng.close()
    assert sums.shape == (len(tile), 1 + V)
    for batch in (slice(0, INTEGRATE_BATCH_RAYS), slice(INTEGRATE_BATCH_RAYS, None)):
        assert _same_bits(sums[batch, 0], ref[tile[batch], 0]), batch
    assert _same_bits(sums, ref[tile]), int((sums != ref[tile]).any(axis=1).sum())


# ---- the probe files

@pytest.mark.parametrize("name", T.GOLDEN_SCENES)
def test_probe_files_are_the_reference_s(name, tmp_path):
    """the test oracle's field (the reference's random stream) bound to the engine; temperatures and averages from the engine"""
    sim, rf = T.oracle_field(name)
    eng = Engine(sim.scene, 0)
    table = _bound_field(eng, rf)
    sim.write_radiation_field(eng.download_radiation_field(), str(tmp_path))
    sim.write_probes(str(tmp_path), eng)
    files = P.assert_files_equal_golden(name, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == files
    del table
    eng.close()


def test_results_do_not_depend_on_what_device_memory_held(tmp_path):
    """PMC_POISON_ALLOCATIONS fills what the engine allocates without initialising with 0xA5 bytes -- the result buffers of the two calls
    too --: the kernel cases with the most tiles and components, the ray cases of an octree and of the Voronoi grid, and the files of two
    golden scenes come out the same"""
    set_tuning("PMC_POISON_ALLOCATIONS")
    try:
        for base, bins, components in (("cfg1temp", 65, 4), ("cfg5small", 6, 2)):
            sim = Simulation(with_field_grid(tmp_path, base, bins), num_packets=100).setup()
            cells = scene_head(sim).grid.num_cells
            tables = T.random_tables(cells, bins, components, seed=bins * 10 + components)
            rf, _ = T.special_rows(tables, np.random.default_rng(bins).random(cells * bins) * 1e30, seed=components)
            eng = Engine(sim.scene, 0)
            table = _bound_field(eng, rf)
            assert _same_bits(eng.dust_temperatures(tables), host.dust_temperatures(tables, rf)), (base, bins, components)
            del table
            eng.close()
        for name in ("cfg2small", "cfg5small"):
            sim, r, k, w, q, ref = _case(name)
            eng = Engine(sim.scene, 0)
            assert _same_bits(eng.integrate_weighted_rays(r, k, w, q), ref), name
            assert _same_bits(eng.integrate_weighted_rays(r[:65], k[:65], w, q[0]), ref[:65, :2]), name
            eng.close()
        for name in ("cfg3mmtemp", "cfg2bintemp"):
            sim, rf = T.oracle_field(name)
            eng = Engine(sim.scene, 0)
            table = _bound_field(eng, rf)
            assert _same_bits(eng.dust_temperatures(sim.temperature_tables()), sim.dust_temperatures(rf))
            sim.write_probes(str(tmp_path / name), eng)
            del table
            eng.close()
            assert len(P.assert_files_equal_golden(name, str(tmp_path / name), suffixes=("_T.dat", "_T.fits", "_Labs.dat"))) >= 5
    finally:
        clear_tuning()


def test_the_photon_loop_is_untouched(monkeypatch):
    """two segments on cfg1temp with and without dust_temperatures and integrate_weighted_rays between them: the same frames, element for
    element.  As in tests/test_gpu_probes.py the photon loop runs in the configuration in which its frames are reproducible (one slot group,
    one wave of slots, statistics by atomics), which two plain runs prove first.  The field is added to by atomics in an order that varies
    from run to run even then (two plain runs differ in its last bits), so it is compared to rounding: sums of up to 1e4 positive terms in
    another order differ by less than 1e4 * 2^-53 ~ 1e-12 of their value; 1e-10 is asked."""
    n = 3000
    sim = Simulation(ski("cfg1temp.ski"), num_packets=2 * n).setup()
    tables = sim.temperature_tables()
    maps = sim.probe_maps()
    monkeypatch.setenv("PMC_NUM_GROUPS", "1")
    set_tuning("PMC_STAT_ATOMICS")

    def photon_loop(between):
        eng = Engine(sim.scene, 0)
        eng.set_num_slots(64)
        eng.run_primary(0, n, 99)
        if between:
            temperatures = eng.dust_temperatures(tables)
            assert _same_bits(temperatures, sim.dust_temperatures(eng.download_radiation_field()))
            sums = eng.integrate_weighted_rays(maps[1]["origins"], maps[1]["directions"], maps[1]["cell_values"][0], temperatures[-1])
            assert sums.shape == (maps[1]["num_rays"], 2) and (sums[:, 0] > 0).mean() > 0.5
        eng.run_primary(n, n, 99)
        result = eng.download(), eng.download_radiation_field(), eng.counters()
        eng.close()
        return result

    base = photon_loop(False)
    again = photon_loop(False)
    assert base[2]["histories"] == 2 * n and base[0].sum() > 0 and base[1].sum() > 0
    assert again[2] == base[2] and np.array_equal(again[0], base[0])  # (the configuration is reproducible)
    frames, rf, counters = photon_loop(True)
    assert counters == base[2]
    assert np.array_equal(frames, base[0]), int((frames != base[0]).sum())
    assert np.array_equal(rf == 0, base[1] == 0) and np.allclose(rf, base[1], rtol=1e-10, atol=0.)


@pytest.mark.parametrize("name", ["cfg3temp", "cfg3mmtemp"])
def test_driver_writes_the_probe_files(name, tmp_path, monkeypatch):
    """skirt_mi355x writes the file names of the golden set, with and without -g 0, and the bytes of the Python path from the same engine run:
    the same histories in the reproducible configuration of the photon loop (one slot group, one wave of slots; PMC_NUM_GROUPS and
    PMC_NUM_SLOTS are the library's own settings), so that the driver's field is the Python path's bit for bit"""
    n = 2000
    monkeypatch.setenv("PMC_NUM_GROUPS", "1")
    monkeypatch.setenv("PMC_NUM_SLOTS", "64")
    exe = os.path.join(ROOT, "skirt9_amd", "lib", "skirt_mi355x")
    sim = Simulation(ski(name + ".ski"), num_packets=n).setup()
    eng = Engine(sim.scene, 0)
    eng.run_primary(0, n, sim.seed)
    python = tmp_path / "python"
    sim.write_radiation_field(eng.download_radiation_field(), str(python))
    sim.write_probes(str(python), eng)
    eng.close()
    names = sorted(T.golden_files(name))
    assert sorted(os.listdir(python)) == names
    for extra in ([], ["-g", "0"]):
        out = tmp_path / ("plain" if not extra else "g0")
        out.mkdir()
        subprocess.check_call([exe, "-o", str(out), "-n", str(n)] + extra + [ski(name + ".ski")], cwd=ROOT, timeout=300, stdout=subprocess.DEVNULL)
        assert sorted(f for f in os.listdir(out) if f in names) == names
        assert not [f for f in os.listdir(out) if f.endswith(("_T.dat", "_T.fits", "_Labs.dat", "_J.dat")) and f not in names]
        for f in names:
            assert P.same_file(str(python / f), str(out / f)), f
