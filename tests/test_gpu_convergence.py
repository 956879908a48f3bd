"""The point sampler on the MI355X (pmc_sample_cells: locateCellsKernel, gatherCellsKernel).

Engine.sample_cells answers SpatialGrid::cellIndex for many positions and reads cell values there.  Its cells must EQUAL the host restatement
(Simulation.cell_indices, itself checked against the oracle in test_host_convergence.py) on all five forms of the kernel, positions on cell
walls, on the domain's boundary and outside it included; its values are copies of the caller's doubles, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import convergence_checks as K
from conftest import ROOT
from skirt9_amd.engine import INTEGRATE_PASS_VALUES, SAMPLE_CHUNK_POINTS, Engine, clear_tuning, lib, set_tuning

pytestmark = pytest.mark.gpu

NUM_POINTS = 1000
COUNTS = (0, 1, 63, 64, 65, NUM_POINTS)
# cells only; one value; a full pass; two passes, the second with one value; three passes
VALUE_COUNTS = (0, 1, INTEGRATE_PASS_VALUES, INTEGRATE_PASS_VALUES + 1, 2 * INTEGRATE_PASS_VALUES + 1)
PMC_ERR_INVALID = -1


def _case(name):
    """(sim, points [NUM_POINTS][3], the host's cells, cell values [9][num_cells])"""
    sim = K.simulation(name)
    points = K.point_set(name, NUM_POINTS)
    return sim, points, _host_cells(name), _values(name)


_cache = {}


def _host_cells(name):
    if ("cells", name) not in _cache:
        _cache["cells", name] = K.simulation(name).cell_indices(K.point_set(name, NUM_POINTS))
    return _cache["cells", name]


def _values(name):
    if ("values", name) not in _cache:
        num_cells = K.scene_head(K.simulation(name)).grid.num_cells
        q = np.random.default_rng(7).random((max(VALUE_COUNTS), num_cells)) + 0.5
        q[0, ::7] = 0.  # (a cell value of zero is a value like any other)
        _cache["values", name] = q
    return _cache["values", name]


def _expected(q, cells):
    """q[:, cells] with 0 where the cell is -1"""
    out = q[:, np.maximum(cells, 0)].copy()
    out[:, cells < 0] = 0.
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", K.SCENES)
def test_cells_equal_the_host_s_and_values_are_copies(name):
    sim, points, cells, q = _case(name)
    # from the point set alone: it holds what it is meant to hold
    inside, outside = K.boundary_points(sim)
    assert (cells == -1).sum() == len(outside) and (cells >= 0).sum() == NUM_POINTS - len(outside)
    if name in K.BOX_SCENES:
        boxes = K.cell_boxes(sim)[np.maximum(cells, 0)]
        on_wall = np.any((points == boxes[:, :3]) | (points == boxes[:, 3:]), axis=1) & (cells >= 0)
        assert on_wall.sum() > 300
    eng = Engine(sim.scene, 0)
    for n in COUNTS:
        first = 0 if n == NUM_POINTS else 32
        sel = slice(first, first + n)
        for v in VALUE_COUNTS:
            values, got = eng.sample_cells(points[sel], q[:v] if v else None)
            assert got.dtype == np.int32 and np.array_equal(got, cells[sel]), (name, n, v, int((got != cells[sel]).sum()))
            if v == 0:
                assert values is None
            else:
                assert _same_bits(values, _expected(q[:v], cells[sel])), (name, n, v)
    # one row of values: a vector back; without an array for the cells: the same values
    values, got = eng.sample_cells(points, q[1])
    assert values.shape == (NUM_POINTS,) and _same_bits(values, _expected(q[1:2], cells)[0])
    values, got = eng.sample_cells(points, q[:5], cells=False)
    assert got is None and _same_bits(values, _expected(q[:5], cells))
    assert eng.last_sample_ms() > 0.
    eng.close()


def test_more_points_than_one_chunk():
    """SAMPLE_CHUNK_POINTS + 37 positions in and around the grid of cfg2small, five values: two chunks of two passes each"""
    sim = K.simulation("cfg2small")
    lo, hi = K.domain(sim)
    n = SAMPLE_CHUNK_POINTS + 37
    points = lo + (hi - lo) * (np.random.default_rng(23).random((n, 3)) * 1.1 - 0.05)
    points[-37:] = K.point_set("cfg2small", NUM_POINTS)[:37]
    cells = sim.cell_indices(points)
    assert 0.1 * n < (cells < 0).sum() < 0.4 * n
    q = _values("cfg2small")[:5]
    eng = Engine(sim.scene, 0)
    values, got = eng.sample_cells(points, q)
    eng.close()
    assert np.array_equal(got, cells)
    assert _same_bits(values, _expected(q, cells))


@pytest.mark.parametrize("name", K.SCENES)
def test_order_of_the_points_does_not_matter(name):
    sim, points, cells, q = _case(name)
    perm = np.random.default_rng(11).permutation(NUM_POINTS)
    eng = Engine(sim.scene, 0)
    values, got = eng.sample_cells(points[perm], q[:5])
    eng.close()
    assert np.array_equal(got, cells[perm])
    assert _same_bits(values, _expected(q[:5], cells)[:, perm])


@pytest.mark.parametrize("name", ["cfg2small", "cfg5small"])
def test_results_do_not_depend_on_what_device_memory_held(name):
    """PMC_POISON_ALLOCATIONS fills what the engine allocates without initialising with 0xA5 bytes (the sampler's own buffers too)"""
    sim, points, cells, q = _case(name)
    set_tuning("PMC_POISON_ALLOCATIONS")
    try:
        eng = Engine(sim.scene, 0)
        values, got = eng.sample_cells(points, q[:5])
        eng.close()
    finally:
        clear_tuning()
    assert np.array_equal(got, cells)
    assert _same_bits(values, _expected(q[:5], cells))


def test_the_photon_loop_is_untouched(monkeypatch):
    """run_primary after sample_cells on the same context gives the frames it gives without: cfg1, 10^4 packets, every element equal, in
    the engine's reproducible configuration (one slot group, one wave of slots, statistics by atomics; see the test of the same name in
    test_gpu_probes.py); and the sampler gives its own result before and after the photon loop"""
    n = 10000
    sim, points, cells, q = _case("cfg1")
    monkeypatch.setenv("PMC_NUM_GROUPS", "1")
    set_tuning("PMC_STAT_ATOMICS")

    def check(eng):
        values, got = eng.sample_cells(points, q[:5])
        assert np.array_equal(got, cells) and _same_bits(values, _expected(q[:5], cells))

    def photon_loop(sample):
        eng = Engine(sim.scene, 0)
        eng.set_num_slots(64)
        if sample:
            check(eng)
        eng.run_primary(0, n, 99)
        frames, counters = eng.download(), eng.counters()
        if sample:
            check(eng)
        eng.close()
        return frames, counters

    base, base_counters = photon_loop(False)
    again, again_counters = photon_loop(False)
    assert base_counters["histories"] == n and base.sum() > 0
    assert again_counters == base_counters and np.array_equal(again, base)  # (the configuration is reproducible)
    frames, counters = photon_loop(True)
    assert counters == base_counters
    assert np.array_equal(frames, base), int((frames != base).sum())


def test_input_errors_are_reported_and_the_context_stays_usable():
    sim, points, cells, q = _case("cfg2small")
    eng = Engine(sim.scene, 0)
    for bad in (np.nan, np.inf, -np.inf):
        broken = points[:100].copy()
        broken[57, 1] = bad
        out = np.zeros(100, dtype=np.int32)
        rc = lib().pmc_sample_cells(eng._h, 100, broken.ctypes.data, 0, None, None, out.ctypes.data)
        assert rc == PMC_ERR_INVALID and b"not finite" in lib().pmc_last_error() and b"point 57" in lib().pmc_last_error()
        with pytest.raises(RuntimeError, match="not finite"):
            eng.sample_cells(broken, q[:1])
    assert lib().pmc_sample_cells(eng._h, -1, None, 0, None, None, None) == PMC_ERR_INVALID and b"negative" in lib().pmc_last_error()
    assert lib().pmc_sample_cells(eng._h, 1, None, 0, None, None, None) == PMC_ERR_INVALID and b"null" in lib().pmc_last_error()
    assert lib().pmc_sample_cells(eng._h, 1, points.ctypes.data, 1, None, None, None) == PMC_ERR_INVALID and b"null" in lib().pmc_last_error()
    with pytest.raises(ValueError):
        eng.sample_cells(points[:4], q[:2, :-1])
    values, got = eng.sample_cells(points, q[:5])
    assert np.array_equal(got, cells) and _same_bits(values, _expected(q[:5], cells))
    start = K.random_interior(sim, 1, seed=9)[0]
    m0, _ = eng.trace_ray(start, np.ones(3) / np.sqrt(3.))
    assert len(m0) > 0 and m0[0] == sim.cell_indices(start)[0]
    eng.close()


# ---------------------------------------------------------------- ConvergenceCutsProbe through the engine

@pytest.mark.parametrize("name", ["cfg1cuts", "cfg2deepcuts", "cfg2eleccuts", "cfg2bincuts", "cfg5smallcuts"])
def test_cut_files_through_the_engine_are_the_reference_s(name, tmp_path):
    """write_probes with the engine as the sampler: the file set by dimension and material type, every recorded file's bytes (Voronoi: the
    cuts of the true density; the gridded ones are written from the host layer's own tessellation)"""
    sim = K.simulation(name)
    eng = Engine(sim.scene, 0)
    sim.write_probes(str(tmp_path), eng, sampler=eng)
    assert eng.last_sample_ms() > 0.
    eng.close()
    assert sorted(os.listdir(tmp_path)) == K.cut_files(name)
    assert K.assert_cuts_equal_golden(name, str(tmp_path))


def test_the_engine_s_cuts_without_a_sampler_fail_loudly(tmp_path):
    sim = K.simulation("cfg1cuts")
    eng = Engine(sim.scene, 0)
    with pytest.raises(RuntimeError, match="needs a sampler"):
        sim.write_probes(str(tmp_path), eng)
    eng.close()
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("name", ["cfg1conv", "cfg2deepconv", "cfg2elecconv", "cfg2binconv"])
def test_both_probes_through_the_engine_are_the_reference_s(name, tmp_path):
    """a scene with the two convergence probes of the ski-file wizard, integrator and sampler the engine: the info file's bytes (six rays per
    material type through pmc_integrate_rays) and the cut files' digests"""
    sim = K.simulation(name)
    eng = Engine(sim.scene, 0)
    sim.write_probes(str(tmp_path), eng, sampler=eng)
    eng.close()
    scene = K.INFO_SCENES[name]
    cuts = K.cut_files(name, scene)
    assert sorted(os.listdir(tmp_path)) == sorted(cuts + [K.info_file(name)])
    K.assert_info_equals_golden(name, str(tmp_path))
    K.assert_cuts_of(name, scene, str(tmp_path))


@pytest.mark.parametrize("name", ["cfg1conv", "cfg2elecconv"])
def test_driver_writes_both_probes(name, tmp_path):
    """skirt_mi355x on a scene with both probes: the reference's info file and cut files next to the instrument files.  Probes with probeAfter
    Setup (cfg1conv) are written BEFORE the photon loop: the driver's log has its lines in that order, and between the last probe file and
    the first instrument file lies at least the time the log gives for the loop itself ("Photon loop on the first device: T s", around
    pmc_run_primary alone) less 30 ms for the coarse clock of the file times (4e7 packets: the loop takes some 0.4 s on this scene); written after the loop, the files would be milliseconds
    apart.  With probeAfter Run (cfg2elecconv) the setup output is empty and probes and frames both follow the loop"""
    exe = os.path.join(ROOT, "skirt9_amd", "lib", "skirt_mi355x")
    log = subprocess.run([exe, "-o", str(tmp_path), "-n", "40000000" if name == "cfg1conv" else "100000", K.ski(name + ".ski")], cwd=ROOT, timeout=300, check=True,
                         capture_output=True, text=True).stdout
    scene = K.INFO_SCENES[name]
    probe_files = sorted(K.cut_files(name, scene) + [K.info_file(name)])
    written = sorted(os.listdir(tmp_path))
    assert [f for f in written if f"_{K.PROBE_NAME}_" in f or f"_{K.INFO_PROBE_NAME}_" in f] == probe_files
    K.assert_info_equals_golden(name, str(tmp_path))
    K.assert_cuts_of(name, scene, str(tmp_path))
    frames = [f for f in written if f.endswith("_total.fits")]
    assert frames
    stamp = lambda f: os.stat(os.path.join(tmp_path, f)).st_mtime  # noqa: E731
    setup_output = re.search(r"Finished setup output in ([0-9.]+) s", log)
    loop = re.search(r"Photon loop on the first device: ([0-9.]+) s", log)
    assert setup_output and loop and log.index("Finished setup output") < log.index("Photon loop on the first device")
    gap = min(stamp(f) for f in frames) - max(stamp(f) for f in probe_files)
    if name in K.INFO_RUN_SCENES:
        assert float(setup_output.group(1)) < 0.05 and 0. <= -gap < 1.  # (the frames first, then the Run probes, in one go)
    else:
        assert float(loop.group(1)) > 0.1, log  # (a loop long enough to tell)
        assert gap >= float(loop.group(1)) - 0.03, (gap, log)
