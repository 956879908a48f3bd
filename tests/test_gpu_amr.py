"""The density of an adaptive mesh medium on the MI355X (pmc_sampler_create_mesh: sampleMeshDensityKernel).

MeshSampler.density must EQUAL the pure-Python restatement of the reference's descent (tests/amr_checks.py) bit for bit -- on synthetic
meshes whose leaves all carry different densities, so that an equal density means the same leaf, and on the fixture mesh; positions on cell
walls, one ulp beside them, on the domain's boundary, outside it and not-a-number included.  With the sampler bound to the host layer, the
setup of the mesh scenes gives the reference's recorded cell densities and convergence files, and the photon loop matches the oracle.  No
test provokes the device error path."""
import os
import subprocess

import numpy as np
import pytest

import amr_checks as A
import oracle_lib as O
from conftest import ROOT, golden, ski
from skirt9_amd.engine import Engine, MeshSampler
from skirt9_amd.host import Simulation, scene_head
from test_gpu_parity import _compare_frames
from test_host_amr import assert_convergence_files

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 65, 1000)
MESHES = list(A.SYNTHETIC) + ["fixture"]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fixture_simulation():
    """cfg6amr set up on the host cores: the yardstick"""
    if "sim" not in _cache:
        _cache["sim"] = Simulation(ski("cfg6amr.ski")).setup()
    return _cache["sim"]


def _case(kind):
    """(tables, 1000 positions of the point sets in a fixed mixed order, the restatement's densities there), computed once"""
    if kind not in _cache:
        mesh = _fixture_simulation().adaptive_mesh(0) if kind == "fixture" else A.SYNTHETIC[kind]()
        sets = A.point_sets(mesh, upper_walls=kind in A.DYADIC, num_random=400)
        # the domain's corners, the outside points and the odd ones always; of the rest -- walls, their neighbours, centres, random points --
        # a fixed draw; the whole in a fixed mixed order
        always = np.concatenate([sets[key] for key in ("corners", "outside", "odd")])
        rest = np.concatenate([sets[key] for key in ("walls", "near_walls", "centres", "random")])
        rest = rest[np.random.default_rng(23).permutation(len(rest))]
        while len(always) + len(rest) < 1000:
            rest = np.concatenate([rest, rest])
        points = np.concatenate([always, rest])[:1000]
        points = np.ascontiguousarray(points[np.random.default_rng(29).permutation(1000)])
        assert A.cannot_locate(mesh, points) == []
        _cache[kind] = (mesh, points, A.Descent(mesh).densities(points))
    return _cache[kind]


@pytest.mark.parametrize("kind", MESHES)
def test_densities_equal_the_restatement(kind):
    mesh, points, want = _case(kind)
    assert (want == 0).sum() >= 8 and (want > 0).sum() >= 500  # (outside and odd points, and points inside)
    sampler = MeshSampler(mesh, 0)
    for n in COUNTS:
        first = 0 if n == 1000 else 32
        got = sampler.density(points[first:first + n])
        assert got.shape == (n,) and np.array_equal(_bits(got), _bits(want[first:first + n])), (kind, n)
    # the order of the positions does not matter
    order = np.random.default_rng(4).permutation(1000)
    assert np.array_equal(_bits(sampler.density(points[order])), _bits(want[order]))
    sampler.close()


def test_depth_1_and_depth_30_inside_one_wave():
    """the chain: lanes that stop at the first level next to lanes that descend 30 levels, alternating inside every wave"""
    mesh = A.SYNTHETIC["chain"]()
    boxes, level = A.leaf_boxes(mesh), A.leaf_levels(mesh)
    assert level.max() == 30
    deep = boxes[level == 30]
    shallow = boxes[level == 1]
    u = np.random.default_rng(9).random((256, 3))
    points = np.empty((256, 3))
    points[0::2] = deep[np.arange(128) % len(deep), :3] + u[0::2] * (deep[np.arange(128) % len(deep), 3:] - deep[np.arange(128) % len(deep), :3])
    points[1::2] = shallow[np.arange(128) % len(shallow), :3] + u[1::2] * (shallow[np.arange(128) % len(shallow), 3:] - shallow[np.arange(128) % len(shallow), :3])
    points[5] = deep[0, :3]   # the corner of the domain, 30 levels down
    points[7] = deep[-1, 3:]  # the upper corner of the deepest octet: a corner of eight leaves
    descent = A.Descent(mesh)
    cells = descent.cells(points)
    assert set(level[cells[0::2]]) == {30} and set(level[cells[1::2][4:]]) == {1}
    sampler = MeshSampler(mesh, 0)
    assert np.array_equal(_bits(sampler.density(points)), _bits(descent.densities(points)))
    sampler.close()


def test_two_batches_equal_the_host():
    """2^22 + 37 positions: two batches through the sampler's buffers, against the host cores' evaluation of the same snapshot"""
    sim = _fixture_simulation()
    mesh = sim.adaptive_mesh(0)
    n = (1 << 22) + 37
    lo, hi = mesh["node_box"][0, :3], mesh["node_box"][0, 3:]
    u = np.random.default_rng(31).random((n, 3)) * 1.02 - 0.01  # (one position in twenty outside the domain)
    points = lo + (hi - lo) * u
    _, special, _ = _case("fixture")
    points[-1000:] = special  # (the last ones, in the second batch: walls, neighbours, NaN)
    want = sim.imported_densities(0, points)
    sampler = MeshSampler(mesh, 0)
    got = sampler.density(points)
    sampler.close()
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[: 1 << 22] > 0).sum() > 3000000 and (got[1 << 22:] > 0).any()


@pytest.mark.parametrize("what,tables,words", A.malformed_tables(), ids=[row[0] for row in A.malformed_tables()])
def test_malformed_tables_are_refused(what, tables, words):
    """PMC_ERR_INVALID from the check of the table, which comes before any device call: no kernel runs"""
    with pytest.raises(RuntimeError, match=r"^pmc error -1: adaptive mesh: " + words):
        MeshSampler(tables, 0)


@pytest.mark.parametrize("name", ["cfg6amr", "cfg6amrnum", "cfg6amrelec"])
def test_setup_with_the_device_sampler_gives_the_reference_s_cells(name):
    """the tree policy's 100 densities per node and the 100 per cell through the kernel: the reference's cells and densities, bit for bit"""
    sim = Simulation(ski(name + ".ski")).use_device_sampler(0).setup()
    gold = np.load(golden(name + "_cells.npz"))
    head = scene_head(sim)
    assert head.grid.num_cells == len(gold["density"])
    density = np.ctypeslib.as_array(head.medium.number_density, shape=(head.grid.num_cells,))
    assert np.array_equal(_bits(density), _bits(gold["density"]))
    if name == "cfg6amr":
        host = scene_head(_fixture_simulation()).grid
        assert host.num_nodes == head.grid.num_nodes
        assert np.array_equal(np.ctypeslib.as_array(host.node_box, shape=(host.num_nodes, 6)), np.ctypeslib.as_array(head.grid.node_box, shape=(host.num_nodes, 6)))
        points = _case("fixture")[1]
        assert np.array_equal(_bits(sim.imported_densities(0, points)), _bits(_case("fixture")[2]))  # (skh_imported_densities on the device)


def test_convergence_probes_through_the_engine(tmp_path):
    """cfg6amrconv with sampler, integrator and cell sampler on the device: the reference's info file (Snapshot::SigmaX/Y/Z through the
    kernel, on cell walls) and its six cuts (the true density at 3 x 2^20 positions ON cell walls through the kernel)"""
    sim = Simulation(ski("cfg6amrconv.ski")).use_device_sampler(0).setup()
    eng = Engine(sim.scene, 0)
    sim.write_probes(str(tmp_path), eng, sampler=eng)
    eng.close()
    assert_convergence_files(str(tmp_path))


def test_convergence_probes_through_the_driver(tmp_path):
    """skirt_mi355x -s hands the mesh sampler over where it hands over the particle sampler"""
    exe = os.path.join(ROOT, "skirt9_amd", "lib", "skirt_mi355x")
    subprocess.run([exe, "-s", "-o", str(tmp_path), ski("cfg6amrconv.ski")], cwd=ROOT, timeout=300, check=True, capture_output=True, text=True)
    probes = tmp_path / "probes"
    probes.mkdir()
    for f in os.listdir(tmp_path):
        if "_cnv_" in f or "_inf_" in f:
            os.rename(tmp_path / f, probes / f)
    assert_convergence_files(str(probes))
    assert (tmp_path / "cfg6amrconv_i0_total.fits").exists()


def test_photon_loop_matches_the_oracle():
    n = 20000
    sim = Simulation(ski("cfg6amr.ski"), num_packets=n).use_device_sampler(0).setup()
    eng = Engine(sim.scene, 0)
    eng.run_primary(0, n, 12345)
    gpu = eng.download()
    ref, counters = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=12345)
    c = eng.counters()
    eng.close()
    assert c["histories"] == n and c["stat_overflows"] == 0
    assert abs(c["cell_visits"] - counters.cell_visits) <= 1e-4 * counters.cell_visits
    _compare_frames(sim, gpu, ref, n)


def test_a_particle_sampler_and_a_mesh_sampler_side_by_side():
    """both kinds of sampler alive at once behind the same three entry points: each gives its own snapshot's densities"""
    particles_host = Simulation(ski("cfg4small.ski")).setup()
    particles = Simulation(ski("cfg4small.ski")).use_device_sampler(0).setup()
    mesh = Simulation(ski("cfg6amr.ski")).use_device_sampler(0).setup()
    points = _case("fixture")[1]
    finite = points[np.isfinite(points).all(axis=1)]
    for _ in range(2):
        assert np.array_equal(_bits(mesh.imported_densities(0, points)), _bits(_case("fixture")[2]))
        assert np.array_equal(_bits(particles.imported_densities(0, finite)), _bits(particles_host.imported_densities(0, finite)))
    assert (particles_host.imported_densities(0, finite) > 0).sum() > 100
    mesh.close()
    assert np.array_equal(_bits(particles.imported_densities(0, finite)), _bits(particles_host.imported_densities(0, finite)))
