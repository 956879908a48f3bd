"""Binary-tree grids (PolicyTreeSpatialGrid with treeType BinTree) on the MI355X: the kernels of the binary tree against the ray dumps and
the output files of the UNMODIFIED reference (tests/golden/make_golden_bintree.py), and -- with the switch PMC_TREE_AS_BINTREE, which runs an
OCTREE scene through the same tables and kernels -- against the oracle on the same Philox histories and against the octree kernels."""
import functools

import numpy as np
import pytest

import bintree_checks as B
import oracle_lib as O
from conftest import golden, ski
from skirt9_amd.engine import Engine, clear_tuning, set_tuning
from skirt9_amd.host import Simulation
from test_gpu_parity import _compare_frames

pytestmark = pytest.mark.gpu

N = 20000
OCTREE_SCENES = ["cfg2small", "cfg2deep", "cfg2nf", "cfg2ea", "cfg2mm", "cfg3small", "cfg3rf"]


def _as_bintree(sim):
    """an engine that runs the (octree) scene through the binary tree's tables and kernels: the switch is read at pmc_create"""
    set_tuning("PMC_TREE_AS_BINTREE")
    try:
        return Engine(sim.scene, 0)
    finally:
        clear_tuning()


@pytest.mark.parametrize("name", ["cfg2bin", "cfg2bindeep"])
def test_trace_ray_equals_the_reference(name):
    """pmc_trace_ray against the reference's own (m, ds) dump of the 48 fixed rays, bit for bit (TreeSpatialGrid.cpp:140-216 on BinTreeNode)"""
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    rays = B.read_rays(golden(name + "_rays.txt"))
    dump = B.read_ray_dump(golden(name + "_rays_ref.txt"))
    assert len(rays) == len(dump) == 48
    if name == "cfg2bindeep":
        # from the fixture alone: some ray passes a cell of the finest level of the tree
        tree = B.Tree(sim)
        finest = set(tree.cell_array[(tree.first_array < 0) & (tree.level_array == tree.level_array.max())].tolist())
        assert tree.level_array.max() > 20 and any(finest & set(m) for _, m, _ in dump)
    eng = Engine(sim.scene, 0)
    total = 0
    for i, ((r, _), (k, m_ref, ds_ref)) in enumerate(zip(rays, dump)):
        m, ds = eng.trace_ray(np.array(r), np.array(k))
        assert len(m) == len(m_ref), (i, len(m), len(m_ref))
        assert np.array_equal(m, np.array(m_ref, dtype=np.int32)), i
        assert np.array_equal(ds.view(np.uint64), np.array(ds_ref).view(np.uint64)), i
        total += len(m)
    assert total == sum(len(m) for _, m, _ in dump) > 400
    eng.close()


@functools.lru_cache(maxsize=None)
def _octree_run(name, switch):
    """(frames, counters, radiation field or None) of N histories, seed 12345, of an octree scene; switch: through the binary tree's kernels"""
    sim = Simulation(ski(name + ".ski"), num_packets=N).setup()
    eng = _as_bintree(sim) if switch else Engine(sim.scene, 0)
    eng.run_primary(0, N, 12345)
    frames, counters = eng.download(), eng.counters()
    rf = eng.download_radiation_field() if sim.radiation_field_size else None
    eng.close()
    return frames, counters, rf


@pytest.mark.parametrize("name", OCTREE_SCENES)
def test_octree_scenes_through_the_new_kernels_match_the_oracle(name):
    """PMC_TREE_AS_BINTREE: every octree node as its three levels of splits, the octree's own boxes and neighbour lists in the cell records;
    the oracle follows the same histories.  Tolerances: those of tests/test_gpu_parity.py (_compare_frames; the radiation field as
    test_radiation_field_matches_oracle)."""
    sim = Simulation(ski(name + ".ski"), num_packets=N).setup()
    gpu, c, gpu_rf = _octree_run(name, True)
    if sim.radiation_field_size:
        ref, ref_rf, counters = O.run_primary_rf(sim, 0, N, O.RNG_PHILOX, seed=12345)
        assert abs(gpu_rf.sum() - ref_rf.sum()) <= 1e-9 * ref_rf.sum()
        assert np.array_equal(gpu_rf > 0, ref_rf > 0)
        bad = np.abs(gpu_rf - ref_rf) > 1e-6 * np.abs(ref_rf) + 1e-13 * ref_rf.max()
        assert bad.sum() == 0, int(bad.sum())
    else:
        ref, counters = O.run_primary(sim, 0, N, O.RNG_PHILOX, seed=12345)
    assert c["histories"] == N and c["stat_overflows"] == 0
    assert abs(c["cell_visits"] - counters.cell_visits) <= 1e-4 * counters.cell_visits
    assert abs(c["scatterings"] - counters.scatterings) <= 1e-4 * counters.scatterings + 2
    _compare_frames(sim, gpu, ref, N)


@pytest.mark.parametrize("name", OCTREE_SCENES + ["cfg3kin", "cfg2agnelec"])
def test_the_two_kernel_forms_agree_on_one_scene(name):
    """the same scene once through the octree kernels and once, with the switch, through the binary tree's: the same histories do the same
    work (counters equal as integers) and fill the same frames (the bound test_config5_walk_kernel_forms_agree uses for two forms of one walk)"""
    octree, c0, rf0 = _octree_run(name, False)
    binary, c1, rf1 = _octree_run(name, True)
    for key in ("histories", "paths", "cell_visits", "scatterings"):
        assert c0[key] == c1[key], (key, c0[key], c1[key])
    assert np.allclose(binary, octree, rtol=1e-10, atol=1e-13 * np.abs(octree).max())
    if rf0 is not None:
        assert np.allclose(rf1, rf0, rtol=1e-10, atol=1e-13 * np.abs(rf0).max())


def test_fits_files_within_noise_of_the_reference(tmp_path):
    """tests/ski/cfg2bin.ski with 10^6 packets on the GPU (Philox streams) against the files the UNMODIFIED reference wrote with its own
    generator at seed 0 (tests/golden/cfg2bin_rebinned.npz: three instruments of 128^2 pixels, summed over 8 x 8 blocks), by the method and
    the criteria of test_gpu_parity.test_fits_cube_within_noise_of_the_reference on blocks (bintree_checks.within_noise): blocks with at
    least 30 contributions in both runs, sigma from each run's own sums of w and w^2; reduced chi^2 in [0.85, 1.2], no block beyond 5.5
    sigma, the integrated flux within 3 sigma, more than 500 blocks.
    The reference's seed-1 run against its seed-0 run (make_golden_bintree.py --check): chi^2 0.971, largest |z| 3.36, integrated flux
    0.15 sigma, 672 blocks -- two runs of the reference meet the criteria."""
    n = 1000000
    sim = Simulation(ski("cfg2bin.ski"), num_packets=n).setup()
    eng = Engine(sim.scene, 0)
    eng.run_primary(0, n, 20260929)
    assert eng.counters()["histories"] == n
    sim.write(eng.download(), str(tmp_path))
    eng.close()
    gpu = B.rebinned_files(str(tmp_path), "cfg2bin")
    gold = np.load(golden("cfg2bin_rebinned.npz"))
    chi2, zmax, flux_sigmas, blocks = B.within_noise(gpu, n, gold, n)
    print(f"cfg2bin against the reference: chi2 {chi2:.4f}, largest |z| {zmax:.3f}, integrated flux {flux_sigmas:.3f} sigma, {blocks} blocks")
    assert blocks > 500
    assert 0.85 <= chi2 <= 1.2, chi2
    assert zmax < 5.5, zmax
    assert flux_sigmas <= 3, flux_sigmas


def _variant(tmp_path, tag, changes):
    text = open(ski("cfg2bin.ski")).read()
    for old, new in changes.items():
        assert old in text
        text = text.replace(old, new)
    path = tmp_path / f"cfg2bin{tag}.ski"
    path.write_text(text)
    return str(path)


@pytest.mark.parametrize("forced", [True, False])
def test_conservation(tmp_path, forced):
    """Detection and bookkeeping on the binary tree.  forced: minWeightReduction 1 and no path-length bias, so that the weight test ends
    every history after its first forced path (no scattering); not forced: the usual cycle without forced scattering.
    The transparent component (the emission peel-off without extinction: it depends on the source and the detectors alone) equals that
    of the same histories in a medium of optical depth 1e-30 -- an empty one -- to 1e-9.  Counters: every cycle starts one peel-off walk
    per observer and one propagation walk; a forced propagation walk that finds optical depth is walked a second time."""
    changes = ({'minWeightReduction="1e4"': 'minWeightReduction="1"', 'pathLengthBias="0.5"': 'pathLengthBias="0"'} if forced
               else {'forceScattering="true"': 'forceScattering="false"'})
    empty = dict(changes)
    empty['opticalDepth="1"'] = 'opticalDepth="1e-30"'
    runs = []
    for tag, ch in (("a", changes), ("b", empty)):
        sim = Simulation(_variant(tmp_path, tag + ("f" if forced else "n"), ch), num_packets=N).setup()
        eng = Engine(sim.scene, 0)
        eng.run_primary(0, N, 77)
        runs.append((sim, eng.download(), eng.counters()))
        eng.close()
    (sim, frames, c), (_, frames_empty, _) = runs
    observers = 3
    for inst in range(observers):
        li = sim.layout(inst)
        assert li.num_components >= 3
        for at, count in ((li.sed_offset, li.num_lambda), (li.ifu_offset, li.npix * li.num_lambda)):   # component 0: transparent
            a, b = frames[at:at + count], frames_empty[at:at + count]
            assert b.sum() > 0
            assert abs(a.sum() - b.sum()) <= 1e-9 * b.sum()
            assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * b.max())
    assert c["histories"] == N
    cycles = N + c["scatterings"]
    if forced:
        assert c["scatterings"] == 0
        # (the second pass: every history whose path crosses the medium, and none more than once)
        assert (observers + 1) * cycles < c["paths"] <= (observers + 2) * cycles
    else:
        assert c["scatterings"] > 0
        assert c["paths"] == (observers + 1) * cycles


def test_results_do_not_depend_on_what_device_memory_held():
    """as tests/test_gpu_parity.py checks the other grids: with every array the engine does not initialise filled with 0xA5 bytes
    (PMC_POISON_ALLOCATIONS) the same histories do the same work and fill the same frames -- the tables of the binary tree and the branch of
    the cycle start kernel that serves it write every task word before it is read"""
    sim = Simulation(ski("cfg2bin.ski"), num_packets=N).setup()

    def run(engine):
        engine.clear()
        engine.reset_counters()
        engine.run_primary(0, N, 4242)
        c = engine.counters()
        return engine.download(), (c["histories"], c["paths"], c["cell_visits"], c["scatterings"], c["detector_updates"])

    keep = Engine(sim.scene, 0)
    base, base_counts = run(keep)
    set_tuning("PMC_POISON_ALLOCATIONS")
    try:
        poisoned, counts = run(Engine(sim.scene, 0))
    finally:
        clear_tuning()
    assert counts == base_counts
    assert np.allclose(poisoned, base, rtol=1e-10, atol=1e-13 * np.abs(base).max())
    first = Engine(sim.scene, 0)
    run(first)
    del first
    again, counts = run(Engine(sim.scene, 0))
    assert counts == base_counts
    assert np.allclose(again, base, rtol=1e-10, atol=1e-13 * np.abs(base).max())
