"""SpatialGrid::cellIndex on the host (Simulation.cell_indices, skh_cell_indices): the CPU yardstick of the engine's point sampler.

The yardstick itself is checked against the oracle's ray tracer: for a position strictly inside the grid, the first segment of a ray from it
lies in the cell cellIndex gives (the path generator's State::Unknown branch calls cellIndex when the start lies inside).  The ray runs along
(1, 1, 1) / sqrt(3): towards the upper side on every axis, i.e. into the cell that the rule "a position on a shared wall belongs to the upper
cell" picks, so that the first segment has a positive length there as well.  On the Voronoi grid the reference is the nearest site by brute
force."""
import hashlib
import os
import shutil

import numpy as np
import pytest

import convergence_checks as K
import oracle_lib as O
import probe_checks as P
from skirt9_amd.host import Simulation

DIAGONAL = np.ones(3) / np.sqrt(3.)


def _first_cells(sim, points):
    """cell of the first segment of the oracle's ray from every point along the diagonal; -2 where the oracle emits no segment"""
    out = np.full(len(points), -2, dtype=np.int64)
    for i, r in enumerate(points):
        m, _ = O.trace_ray(sim, r, DIAGONAL, cap=8)
        if len(m):
            out[i] = m[0]
    return out


def _assert_cells_are_the_oracle_s(sim, points, what):
    assert K.strictly_inside(sim, points).all()
    cells = sim.cell_indices(points)
    first = _first_cells(sim, points)
    silent = first == -2
    # (the oracle may emit nothing for a start so close under the upper boundary that the step out of the first cell has length zero:
    # exactly those points are left out, and they must be few)
    print(f"{what}: {len(points)} points, {int(silent.sum())} without a segment from the oracle")
    assert silent.sum() < 0.01 * len(points), (what, int(silent.sum()))
    bad = np.flatnonzero(~silent & (cells != first))
    assert bad.size == 0, (what, bad.size, points[bad[:3]].tolist(), cells[bad[:3]].tolist(), first[bad[:3]].tolist())
    assert (cells[~silent] >= 0).all()


@pytest.mark.parametrize("name", K.BOX_SCENES)
def test_random_interior_points_lie_in_the_oracle_s_first_cell(name):
    sim = K.simulation(name)
    _assert_cells_are_the_oracle_s(sim, K.random_interior(sim, 1000, seed=1), name + " random")


@pytest.mark.parametrize("name", K.BOX_SCENES)
def test_points_on_cell_walls_belong_to_the_upper_cell_as_in_the_oracle(name):
    """every corner, edge midpoint and face centre of 200 cells, the deepest ones among them: positions shared by up to eight cells"""
    sim = K.simulation(name)
    points = K.cell_feature_points(sim, max_cells=200)
    points = points[K.strictly_inside(sim, points)]
    assert len(points) > 2600  # (of 200 x 26; cells on the domain's boundary lose the features that lie on it: at most half of them)
    _assert_cells_are_the_oracle_s(sim, points, name + " features")
    # the rule itself, from the boxes: the cell found holds the point in its closed box and never has it on an upper wall -- unless that wall
    # is the domain's, which the strictly inside points exclude
    boxes = K.cell_boxes(sim)[sim.cell_indices(points)]
    assert np.all((points >= boxes[:, :3]) & (points < boxes[:, 3:]))


def test_the_deep_octree_has_cells_whose_walls_the_pixels_of_a_cut_hit():
    """cfg2deep reaches level 11: the centres (i + 0.5) / 1024 of a 1024-pixel cut are walls of such cells"""
    sim = K.simulation("cfg2deep")
    g = K.scene_head(sim).grid
    level = np.ctypeslib.as_array(g.node_level, shape=(g.num_nodes,))
    cell = np.ctypeslib.as_array(g.node_cell, shape=(g.num_nodes,))
    assert level[cell >= 0].max() >= 11


def test_voronoi_cells_are_the_nearest_sites():
    sim = K.simulation(K.VORONOI_SCENE)
    site = K.sites(sim)
    lo, hi = K.domain(sim)
    assert np.all((site >= lo) & (site <= hi))
    assert np.array_equal(sim.cell_indices(site), np.arange(len(site)))
    points = K.random_interior(sim, 1000, seed=2)
    nearest, clear = K.brute_force_nearest(site, points)
    assert clear.sum() > 990
    cells = sim.cell_indices(points)
    assert np.array_equal(cells[clear], nearest[clear])
    # ... and the oracle's ray from the point starts in that cell
    first = _first_cells(sim, points[:200])
    assert np.array_equal(first[clear[:200]], nearest[:200][clear[:200]])


@pytest.mark.parametrize("name", K.SCENES)
def test_the_domain_box_is_closed_and_nothing_lies_outside_it(name):
    sim = K.simulation(name)
    inside, outside = K.boundary_points(sim)
    assert len(inside) == 26
    cells = sim.cell_indices(inside)
    num_cells = K.scene_head(sim).grid.num_cells
    assert np.all((cells >= 0) & (cells < num_cells)), cells.tolist()
    assert len(outside) == 8 * 3 + 12 * 2 + 6 * 1 + 7
    assert np.all(sim.cell_indices(outside) == -1)
    if name in K.BOX_SCENES:
        # a point on the outer upper wall belongs to the last cell along that axis: the cell's closed box holds it
        boxes = K.cell_boxes(sim)[cells]
        assert np.all((inside >= boxes[:, :3]) & (inside <= boxes[:, 3:]))


def test_no_points_is_no_error():
    sim = K.simulation("cfg1")
    assert sim.cell_indices(np.zeros((0, 3))).shape == (0,)


def test_the_cartesian_borders_at_zero_belong_to_the_upper_bins():
    """cfg1 has 32 bins per axis on [-1 pc, 1 pc]: the origin is the lower corner of cell (16, 16, 16)"""
    sim = K.simulation("cfg1")
    g = K.scene_head(sim).grid
    assert (g.nx, g.ny, g.nz) == (32, 32, 32)
    assert sim.cell_indices(np.zeros((1, 3)))[0] == 16 + 32 * 16 + 32 * 32 * 16
    below = np.nextafter(0., -1.)
    assert sim.cell_indices(np.array([[below, 0., 0.]]))[0] == 16 + 32 * 16 + 32 * 32 * 15
    assert sim.cell_indices(np.array([[0., 0., below]]))[0] == 15 + 32 * 16 + 32 * 32 * 16


# ---------------------------------------------------------------- ConvergenceCutsProbe (skirt9_amd/host/probes.cpp), without a GPU: the files
# against the digests of the files of the UNMODIFIED reference (tests/golden/make_golden_convergence.py).  The gridded cuts come from a
# Python sampler built on cell_indices here; tests/test_gpu_convergence.py repeats the comparison with the engine's sampler.

def _variant(tmp_path, base, name, edit):
    """a copy of tests/ski/<base>.ski, edited, as <tmp>/<sub>/<name>.ski (the file name is the prefix of the output files)"""
    text = edit(open(K.ski(base + ".ski")).read())
    folder = tmp_path / f"v{len(os.listdir(tmp_path))}"
    folder.mkdir()
    for f in os.listdir(os.path.dirname(K.ski(base + ".ski"))):
        if f.endswith(".txt"):
            shutil.copy(K.ski(f), folder)
    path = folder / (name + ".ski")
    path.write_text(text)
    return str(path)


def _with_probes(text, probes):
    empty = '<probeSystem type="ProbeSystem"><ProbeSystem/></probeSystem>'
    assert empty in text
    return text.replace(empty, '<probeSystem type="ProbeSystem"><ProbeSystem><probes type="Probe">' + probes + '</probes></ProbeSystem></probeSystem>')


def _python_sampler(sim, calls=None):
    def sample(positions, cell_values):
        cells = sim.cell_indices(positions)
        if calls is not None:
            calls.append((len(positions), cell_values.shape[0], int((cells < 0).sum())))
        out = cell_values[:, np.maximum(cells, 0)].copy()
        out[:, cells < 0] = 0.
        return out
    return sample


@pytest.mark.parametrize("name", list(K.CUT_SCENES))
def test_cut_files_are_the_reference_s(name, tmp_path):
    """names and number of the files by dimension (xy; xz from dimension 2; yz for dimension 3) and material types, and every file's bytes"""
    sim = K.simulation(name)
    dimension, types = K.CUT_SCENES[name]
    assert sim.dimension() == dimension
    calls = []
    sim.write_probes(str(tmp_path), sampler=_python_sampler(sim, calls))
    assert sorted(os.listdir(tmp_path)) == K.cut_files(name) and len(K.cut_files(name)) == 2 * dimension * len(types)
    # one sampler call per gridded cut: 1024 x 1024 positions inside the grid, one value
    assert calls == [(1024 * 1024, 1, 0)] * (dimension * len(types))
    assert len(K.assert_cuts_equal_golden(name, str(tmp_path))) == (dimension if name in K.TRUE_CUTS_ONLY else 2 * dimension) * len(types)
    assert sim.probe_maps() == []  # (these probes add no projected map)


def test_every_pixel_of_a_cut_lies_on_a_cell_wall():
    """what makes the tie rule the normal case: the grid of cfg2deepcuts is symmetric about the origin, so the cut z = 0 lies on the wall
    between two cells with every pixel, and each belongs to the upper one"""
    sim = K.simulation("cfg2deepcuts")
    lo, hi = K.domain(sim)
    size = (hi - lo) / 1024
    x = lo[0] + 0.5 * size[0] + np.arange(1024) * size[0]
    y = lo[1] + 0.5 * size[1] + np.arange(1024) * size[1]
    points = np.stack([x, y, np.zeros(1024)], axis=1)
    boxes = K.cell_boxes(sim)[sim.cell_indices(points)]
    assert np.all(boxes[:, 2] == 0.) and np.all(boxes[:, 5] > 0.)


@pytest.mark.parametrize("when,expected", [("Setup", {"cfg1cuts": True, "cfg2eleccuts": False}), ("Run", {"cfg1cuts": False, "cfg2eleccuts": True})])
def test_cuts_follow_probe_after(when, expected, tmp_path):
    for name, written in expected.items():
        sim = K.simulation(name)
        out = tmp_path / name
        sim.write_probes(str(out), sampler=_python_sampler(sim), when=when)
        assert sorted(os.listdir(out)) == (K.cut_files(name) if written else [])


def test_without_a_sampler_the_probe_fails_loudly(tmp_path):
    sim = K.simulation("cfg1cuts")
    for call in (lambda: sim.write_probes(str(tmp_path / "a")), lambda: sim.write_probes(str(tmp_path / "b"), when="Setup"),
                 lambda: sim.write_probes(str(tmp_path / "c"), integrator=lambda r, k, q: np.zeros((len(r), len(q))))):
        with pytest.raises(RuntimeError, match="needs a sampler"):
            call()
    assert not any(os.listdir(tmp_path / d) for d in "abc")
    sim.write_probes(str(tmp_path / "d"), when="Run")  # (nothing is due: no sampler is asked for)
    assert os.listdir(tmp_path / "d") == []
    # the C entry points without a sampler say the same
    from skirt9_amd.host import lib
    os.makedirs(tmp_path / "e")
    assert lib().skh_write_probes(sim._h, None, None, os.fsencode(str(tmp_path / "e"))) != 0 and b"needs a sampler" in lib().skh_last_error()
    assert lib().skh_write_probes_sampled(sim._h, None, None, os.fsencode(str(tmp_path / "e")), -1) != 0 and b"needs a sampler" in lib().skh_last_error()
    assert os.listdir(tmp_path / "e") == []


def test_a_failing_sampler_fails_the_probe(tmp_path):
    sim = K.simulation("cfg1cuts")

    def broken(positions, cell_values):
        raise ZeroDivisionError("no sampler today")

    with pytest.raises(ZeroDivisionError):
        sim.write_probes(str(tmp_path), sampler=broken)


CUTS = '<ConvergenceCutsProbe probeName="c" %s/>'


@pytest.mark.parametrize("probes,named", [
    (CUTS % 'probeAfter="Primary"', "ConvergenceCutsProbe probeAfter Primary"),
    (CUTS % 'probeAfter="Secondary"', "ConvergenceCutsProbe probeAfter Secondary"),
    ('<ConvergenceInfoProbe probeName="i" probeAfter="Primary"/>', "ConvergenceInfoProbe probeAfter Primary"),
    ('<ConvergenceInfoProbe probeName="i" probeAfter="Secondary"/>', "ConvergenceInfoProbe probeAfter Secondary"),
])
def test_probe_after_primary_and_secondary_are_refused_by_name(probes, named, tmp_path):
    path = _variant(tmp_path, "cfg1", "refused", lambda t: _with_probes(t, probes))
    with pytest.raises(RuntimeError) as err:
        Simulation(path)
    assert named in str(err.value) and "not supported" in str(err.value)


def test_a_simulation_without_a_medium_writes_no_cuts(tmp_path):
    """ConvergenceCutsProbe.cpp:25"""
    path = _variant(tmp_path, "cfg1nomed", "nomed", lambda t: _with_probes(t, CUTS % ""))
    sim = Simulation(path).setup()
    sim.write_probes(str(tmp_path / "out"))  # (not even a sampler is asked for)
    assert os.listdir(tmp_path / "out") == []


def test_the_probe_leaves_the_scene_alone(tmp_path):
    """the scene file (skh_scene_save: every table the engine gets) of cfg1.ski, of cfg1cuts.ski and of cfg1.ski again, in one process: the
    same bytes -- the probe adds no wavelength, no map and no table"""
    def digest(path):
        sim = Simulation(path).setup()
        target = str(tmp_path / "scene.bin")
        sim.save_scene(target)
        return hashlib.sha256(open(target, "rb").read()).hexdigest()
    before = digest(K.ski("cfg1.ski"))
    assert digest(K.ski("cfg1cuts.ski")) == before == digest(K.ski("cfg1.ski"))


@pytest.mark.parametrize("name,dimension", [("cfg1", 3), ("cfg2small", 2), ("cfg2deep", 1), ("cfg3off", 3), ("cfg3flat", 2), ("cfg4small", 3),
                                            ("cfg2agnelec", 2), ("cfg3plum", 2)])
def test_dimension_of_the_medium_system(name, dimension):
    """MediumSystem::dimension from the classes' own dimension() in the reference: UniformBoxGeometry (GenGeometry) 3; ExpDiskGeometry (SepAxGeometry)
    2 (cfg2small; cfg3plum, whose Plummer sphere is the SOURCE: sources do not count); PlummerGeometry (SpheGeometry) 1 (cfg2deep);
    OffsetGeometryDecorator with an offset in x or y 3; SpheroidalGeometryDecorator (AxGeometry) 2 (cfg3flat); ImportedMedium 3; a TorusGeometry
    (AxGeometry) of dust next to a ShellGeometry (SpheGeometry) of electrons: the larger, 2.  For the seven cut scenes the reference's own file
    names confirm the value (test_cut_files_are_the_reference_s)"""
    assert K.simulation(name).dimension() == dimension


# ---------------------------------------------------------------- ConvergenceInfoProbe: <prefix>_<probe>_convergence.dat against the file of the
# UNMODIFIED reference, byte for byte.  The gridded optical depths come from a Python callable that adds up the oracle's ray segments here
# (as in tests/test_host_probes.py); tests/test_gpu_convergence.py repeats the comparison with the engine's integrator.

def _oracle_integrator(sim, calls=None):
    def integrate(origins, directions, cell_values):
        if calls is not None:
            calls.append((origins.copy(), directions.copy(), cell_values.shape[0]))
        out = np.zeros((len(origins), len(cell_values)))
        for i in range(len(origins)):
            m, ds = O.trace_ray(sim, origins[i], directions[i], cap=65536)
            assert len(m) < 65536
            out[i] = P.path_sum(m, ds, cell_values)
        return out
    return integrate


@pytest.mark.parametrize("name", list(K.INFO_SCENES))
def test_info_files_are_the_reference_s(name, tmp_path):
    """every scene with both probes: the info file's bytes, and next to it the cut files of the scene's dimension -- the ski file of the
    wizard loads and writes everything.  cfg1conv has the probe's wavelength (2 micron) outside the source and instrument range"""
    sim = K.simulation(name)
    calls = []
    sim.write_probes(str(tmp_path), _oracle_integrator(sim, calls), sampler=_python_sampler(sim))
    cuts = K.cut_files(name, K.INFO_SCENES[name])
    assert sorted(os.listdir(tmp_path)) == sorted(cuts + [K.info_file(name)])
    K.assert_info_equals_golden(name, str(tmp_path))
    K.assert_cuts_of(name, K.INFO_SCENES[name], str(tmp_path))
    # six rays per material type in one call: from (eps, eps, eps) along and against every axis, one value
    types = len(K.CUT_SCENES[K.INFO_SCENES[name]][1])
    assert len(calls) == types
    lo, hi = K.domain(sim)
    eps = 1e-15 * np.sqrt(((hi - lo) ** 2).sum())
    for origins, directions, num_values in calls:
        assert num_values == 1 and origins.shape == (6, 3) and np.all(origins == eps)
        assert np.array_equal(directions, np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=float))


@pytest.mark.parametrize("when", ["Setup", "Run"])
def test_info_file_follows_probe_after(when, tmp_path):
    for name in ("cfg1conv", "cfg2elecconv"):
        sim = K.simulation(name)
        out = tmp_path / name
        sim.write_probes(str(out), _oracle_integrator(sim), sampler=_python_sampler(sim), when=when)
        assert (K.info_file(name) in os.listdir(out)) == ((name in K.INFO_RUN_SCENES) == (when == "Run"))


def test_the_probe_s_wavelength_joins_the_simulation_s_wavelengths(tmp_path):
    """ConvergenceInfoProbe is a MaterialWavelengthRangeInterface item (SpecialtyWavelengthProbe.cpp): at 0.55 micron in cfg1, which is
    oligochromatic at 0.55 micron, it changes nothing -- the scene file keeps its bytes --; at 2 micron (cfg1conv) the dust tables are built on
    a wider range and the scene file differs.  That the wider tables are the reference's shows in cfg1conv's info file: its optical depths at
    2 micron are the reference's to the last digit"""
    def digest(path):
        sim = Simulation(path).setup()
        target = str(tmp_path / "scene.bin")
        sim.save_scene(target)
        return hashlib.sha256(open(target, "rb").read()).hexdigest()
    info = '<ConvergenceInfoProbe probeName="i" %s/>'
    plain = digest(K.ski("cfg1.ski"))
    assert digest(_variant(tmp_path, "cfg1", "cfg1", lambda t: _with_probes(t, info % ""))) == plain
    assert digest(_variant(tmp_path, "cfg1", "cfg1", lambda t: _with_probes(t, info % 'wavelength="0.55 micron"'))) == plain
    assert digest(K.ski("cfg1conv.ski")) != plain


@pytest.mark.parametrize("wavelength", ["0.5 pm", "2 m"])
def test_a_wavelength_out_of_range_is_an_error(wavelength, tmp_path):
    path = _variant(tmp_path, "cfg1", "bad", lambda t: _with_probes(t, f'<ConvergenceInfoProbe probeName="i" wavelength="{wavelength}"/>'))
    with pytest.raises(RuntimeError, match="out of range"):
        Simulation(path)


def test_the_info_probe_needs_an_integrator_and_a_medium(tmp_path):
    info = '<ConvergenceInfoProbe probeName="i"/>'
    sim = Simulation(_variant(tmp_path, "cfg1", "lone", lambda t: _with_probes(t, info))).setup()
    with pytest.raises(RuntimeError, match="needs an integrator"):
        sim.write_probes(str(tmp_path / "a"))
    assert os.listdir(tmp_path / "a") == []
    sim.write_probes(str(tmp_path / "b"), _oracle_integrator(sim))  # (no cuts probe: no sampler is asked for)
    assert os.listdir(tmp_path / "b") == ["lone_i_convergence.dat"]
    # ConvergenceInfoProbe.cpp:152: without a medium nothing is written, and nothing is asked for
    sim = Simulation(_variant(tmp_path, "cfg1nomed", "nomed", lambda t: _with_probes(t, info))).setup()
    sim.write_probes(str(tmp_path / "c"))
    assert os.listdir(tmp_path / "c") == []
