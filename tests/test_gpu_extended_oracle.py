"""The HIP engine against the oracle that follows the scene's extension (run with `pytest -m gpu`): electron media with the dipole phase
function, moving sources, binary trees, and all three in one scene -- history by history on the same Philox streams, the WHOLE frame buffer
(scattered components and statistics included) under _compare_frames' tolerances and the counted work under those of
test_photon_loop_matches_oracle.  The oracle itself is pinned byte for byte by files of the unmodified reference
(tests/test_oracle_extended.py).

Every comparison proves that it compares: the same GPU frames fail against the oracle run without the extension (for the binary tree,
which has none: against the oracle on other histories).  And no scene passes vacuously: more scatterings than half the histories, every
scattered-light block non-zero in the oracle, velocities that spread the line over several wavelength bins, rays and histories that reach
the finest level of the deep binary tree -- asserted on the oracle's side alone."""
import os

import numpy as np
import pytest

import bintree_checks as B
import oracle_lib as O
from conftest import ski
from skirt9_amd.host import Simulation
from test_gpu_electrons import SCENES as ELECTRON_SCENES
from test_gpu_electrons import _component_blocks, _engine_and_oracle, _num_instruments, _radiation_field_variant
from test_gpu_kinematics import CASES as KINEMATICS_CASES
from test_gpu_kinematics import N, SEED, _moving_and_twin
from test_gpu_parity import RF_ON, SECOND_COMPONENT, _compare_frames, _engine, _rays

pytestmark = pytest.mark.gpu

PC = 3.0857e16
PRIMARY_SCATTERED = 2


def _report(label, sim, gpu, ref):
    """prints how close a comparison comes to _compare_frames' allowance (the bound itself is _compare_frames' own)"""
    bad = 0
    for inst in range(_num_instruments(sim)):
        li = sim.layout(inst)
        blocks = []
        if li.sed_offset >= 0:
            blocks.append((li.sed_offset, li.num_components * li.num_lambda))
        if li.ifu_offset >= 0:
            blocks.append((li.ifu_offset, li.num_components * li.num_lambda * li.npix))
        for k in range(5):
            if li.wsed_offset >= 0:
                blocks.append((li.wsed_offset + k * li.num_lambda, li.num_lambda))
            if li.wifu_offset >= 0:
                blocks.append((li.wifu_offset + k * li.num_lambda * li.npix, li.num_lambda * li.npix))
        for at, count in blocks:
            a, b = gpu[at:at + count], ref[at:at + count]
            bad += int((np.abs(a - b) > (1e-6 * np.abs(b) + 1e-12 * np.abs(b).max())).sum())
    nz = max(1, np.count_nonzero(ref))
    print(f"{label}: {bad} of {nz} non-zero elements differ (allowance {max(4, int(1e-3 * nz))})")


def _scattered_blocks_are_filled(sim, ref):
    """every scattered-light block that is compared holds light in the oracle: PrimaryScattered and each recorded level, SED and IFU"""
    checked = 0
    for inst in range(_num_instruments(sim)):
        for component in range(PRIMARY_SCATTERED, sim.layout(inst).num_components):
            for at, count in _component_blocks(sim, inst, component):
                assert np.count_nonzero(ref[at:at + count]) > 0, (inst, component)
                checked += 1
    assert checked > 0


def _same_work(c, counters, n):
    assert c["histories"] == n and c["stat_overflows"] == 0
    assert abs(c["cell_visits"] - counters.cell_visits) <= 1e-4 * counters.cell_visits
    assert abs(c["scatterings"] - counters.scatterings) <= 1e-4 * counters.scatterings + 2
    assert counters.scatterings > n // 2


# ---------------------------------------------------------------------------------------------------------------- electrons

@pytest.mark.parametrize("name,n", ELECTRON_SCENES)
def test_electron_scenes_match_the_oracle(name, n):
    """every scene of test_gpu_electrons: Cartesian, octree and Voronoi grid, forced and non-forced scattering, electrons alone and next to
    dust, explicit absorption -- the direction after a dipole scattering, the weights next to dust components, the scattering levels and the
    statistics arrays, history by history"""
    sim, gpu, isotropic, c = _engine_and_oracle(name, n)
    ref, counters = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=12345, ext=True)
    _same_work(c, counters, n)
    _scattered_blocks_are_filled(sim, ref)
    _report(name, sim, gpu, ref)
    _compare_frames(sim, gpu, ref, n)
    with pytest.raises(AssertionError):
        _compare_frames(sim, gpu, isotropic, n)


def test_radiation_field_with_electrons_matches_the_oracle(tmp_path):
    """cfg2agnelecea with the radiation field stored and the usual histories (several scatterings each): the table under the bounds of
    test_radiation_field_matches_oracle, the frames under _compare_frames'"""
    n = 20000
    sim = Simulation(_radiation_field_variant(tmp_path, False), num_packets=n).setup()
    eng = _engine(sim)
    eng.run_primary(0, n, 5)
    gpu, gpu_rf, c = eng.download(), eng.download_radiation_field(), eng.counters()
    eng.close()
    ref, ref_rf, counters = O.run_primary_rf(sim, 0, n, O.RNG_PHILOX, seed=5, ext=True)
    _same_work(c, counters, n)
    assert counters.scatterings > n and ref_rf.sum() > 0
    assert abs(gpu_rf.sum() - ref_rf.sum()) <= 1e-9 * ref_rf.sum()
    assert np.array_equal(gpu_rf > 0, ref_rf > 0)
    bad = np.abs(gpu_rf - ref_rf) > 1e-6 * np.abs(ref_rf) + 1e-13 * ref_rf.max()
    assert bad.sum() == 0, int(bad.sum())
    _report("cfg2agnelecea with the radiation field", sim, gpu, ref)
    _compare_frames(sim, gpu, ref, n)
    # read as an isotropic scatterer the scene gives another table and other frames
    plain, plain_rf, _ = O.run_primary_rf(sim, 0, n, O.RNG_PHILOX, seed=5)
    assert (np.abs(gpu_rf - plain_rf) > 1e-6 * np.abs(plain_rf) + 1e-13 * plain_rf.max()).sum() > 0
    with pytest.raises(AssertionError):
        _compare_frames(sim, gpu, plain, n)


# ---------------------------------------------------------------------------------------------------------------- kinematics

def _moving_against_the_oracle(label, sim, gpu, c, n, seed):
    ref, counters = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=seed, ext=True)
    _same_work(c, counters, n)
    _scattered_blocks_are_filled(sim, ref)
    _report(label, sim, gpu, ref)
    _compare_frames(sim, gpu, ref, n, two_bins_per_history=True)
    at_rest, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=seed)
    with pytest.raises(AssertionError):
        _compare_frames(sim, gpu, at_rest, n, two_bins_per_history=True)
    return ref


@pytest.mark.parametrize("name,forced,ea", KINEMATICS_CASES)
def test_moving_scenes_match_the_oracle(tmp_path_factory, name, forced, ea):
    """the five cases of test_gpu_kinematics, moving scene against the oracle on the MOVING scene: the whole buffer -- the scattered light of a
    shifted packet, and the statistics of histories that reach two wavelength bins of an SED (PMC_STAT_EMISSION_BIN, flushStatistics<KIN>,
    SlotArrays::obsEll / obsLambda)"""
    sim, gpu, _, c, _ = _moving_and_twin(tmp_path_factory, name, forced, ea)
    ref = _moving_against_the_oracle(f"{name} forced={forced} ea={ea}", sim, gpu, c, N, SEED)
    lay = sim.layout(0)
    assert ref[lay.wsed_offset:lay.wsed_offset + lay.num_lambda].sum() > N      # (histories do reach two bins)


@pytest.mark.parametrize("name", ["cfg3kin", "cfg1kinsteep"])
def test_position_dependent_velocities_and_steep_dust_match_the_oracle(name):
    """cfg3kin at 2e4 packets: two sources with different velocities, one of them a cylindrical field (the velocity depends on the launch
    position), in dust that is steep in wavelength; cfg1kinsteep: each packet's cross sections at its own wavelength"""
    sim = Simulation(ski(name + ".ski"), num_packets=N).setup()
    eng = _engine(sim)
    eng.run_primary(0, N, SEED)
    gpu, c = eng.download(), eng.counters()
    eng.close()
    ref = _moving_against_the_oracle(name, sim, gpu, c, N, SEED)
    # the line is spread over the instrument's bins: more than three of them hold transparent light
    lay = sim.layout(0)
    assert np.count_nonzero(ref[lay.sed_offset:lay.sed_offset + lay.num_lambda]) > 3


# ---------------------------------------------------------------------------------------------------------------- binary trees

def _finest_cells(sim):
    tree = B.Tree(sim)
    finest = tree.cell_array[(tree.first_array < 0) & (tree.level_array == tree.level_array.max())]
    return int(tree.level_array.max()), finest


@pytest.mark.parametrize("name,scale", [("cfg2bin", 4000 * PC), ("cfg2bindeep", 300 * PC)])
def test_trace_ray_on_binary_trees_equals_the_oracle(name, scale):
    """pmc_trace_ray against the oracle (BinTreeNode::child in its descent; pinned by the reference's ray dumps in
    test_ray_segments_bit_exact) on 200 random and 7 degenerate rays, bit for bit"""
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    level, finest = _finest_cells(sim)
    eng = _engine(sim)
    rays = _rays(sim, 200, 1, scale)
    assert len(rays) == 207
    total = deepest = 0
    for r, k in rays:
        m_ref, ds_ref = O.trace_ray(sim, r, k)
        m_gpu, ds_gpu = eng.trace_ray(r, k)
        assert len(m_ref) == len(m_gpu), (r, k)
        assert np.array_equal(m_ref, m_gpu), (r, k)
        assert np.array_equal(ds_ref.view(np.uint64), ds_gpu.view(np.uint64)), (r, k)
        total += len(m_ref)
        deepest += int(np.isin(m_ref, finest).any())
    eng.close()
    assert total > 1000      # (a ray that enters a tree of at least 7 levels crosses more than a handful of cells)
    if name == "cfg2bindeep":
        assert level > 20 and deepest > 0      # some ray reaches the finest level


def _bintree_against_the_oracle(label, sim, n, seed):
    eng = _engine(sim)
    eng.run_primary(0, n, seed)
    gpu, c = eng.download(), eng.counters()
    gpu_rf = eng.download_radiation_field() if sim.radiation_field_size else None
    eng.close()
    if gpu_rf is not None:
        ref, ref_rf, counters = O.run_primary_rf(sim, 0, n, O.RNG_PHILOX, seed=seed)
        assert ref_rf.sum() > 0
        assert abs(gpu_rf.sum() - ref_rf.sum()) <= 1e-9 * ref_rf.sum()
        assert np.array_equal(gpu_rf > 0, ref_rf > 0)
        bad = np.abs(gpu_rf - ref_rf) > 1e-6 * np.abs(ref_rf) + 1e-13 * ref_rf.max()
        assert bad.sum() == 0, int(bad.sum())
    else:
        ref, counters = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=seed)
    _same_work(c, counters, n)
    _scattered_blocks_are_filled(sim, ref)
    _report(label, sim, gpu, ref)
    _compare_frames(sim, gpu, ref, n)
    # (a binary tree has no extension to leave out: the comparison tells these histories from others)
    other, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=seed + 1)
    with pytest.raises(AssertionError):
        _compare_frames(sim, gpu, other, n)


@pytest.mark.parametrize("name", ["cfg2bin", "cfg2bindeep"])
def test_photon_loop_on_binary_trees_matches_the_oracle(name, tmp_path):
    """real BinTree scenes, the photon loop's resume path included; cfg2bindeep: more than 20 levels, cell records that carry their own
    boxes -- and histories that reach its finest level: with the radiation field stored (which changes no history) the oracle adds to cells
    of that level"""
    sim = Simulation(ski(name + ".ski"), num_packets=N).setup()
    if name == "cfg2bindeep":
        text = open(ski(name + ".ski")).read()
        assert '<RadiationFieldOptions storeRadiationField="false"/>' in text
        (tmp_path / "deeprf.ski").write_text(text.replace('<RadiationFieldOptions storeRadiationField="false"/>', RF_ON))
        probe = Simulation(str(tmp_path / "deeprf.ski"), num_packets=N).setup()
        level, finest = _finest_cells(probe)
        frames, field, _ = O.run_primary_rf(probe, 0, N, O.RNG_PHILOX, seed=12345)
        plain, _ = O.run_primary(sim, 0, N, O.RNG_PHILOX, seed=12345)
        assert np.array_equal(frames, plain)
        assert level > 20 and field.reshape(-1, probe.radiation_field_size // B.Tree(probe).num_cells)[finest].sum() > 0
    _bintree_against_the_oracle(name, sim, N, 12345)


BINTREE_VARIANTS = {"nf": ({'forceScattering="true"': 'forceScattering="false"'}, 50000),
                    "ea": ({'explicitAbsorption="false"': 'explicitAbsorption="true"'}, N),
                    "mm": ({"</GeometricMedium>": SECOND_COMPONENT}, N),
                    "rf": ({'<RadiationFieldOptions storeRadiationField="false"/>': RF_ON}, N),
                    "mmearf": ({"</GeometricMedium>": SECOND_COMPONENT, 'explicitAbsorption="false"': 'explicitAbsorption="true"',
                                '<RadiationFieldOptions storeRadiationField="false"/>': RF_ON}, N)}


@pytest.mark.parametrize("tag", list(BINTREE_VARIANTS))
def test_photon_cycle_variants_on_a_binary_tree_match_the_oracle(tag, tmp_path):
    """cfg2bin without forced scattering, with explicit absorption, with a second component, with the radiation field stored, and with the
    last three together: text substitutions as in test_gpu_parity.py"""
    changes, n = BINTREE_VARIANTS[tag]
    text = open(ski("cfg2bin.ski")).read()
    for old, new in changes.items():
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    path = tmp_path / f"cfg2bin{tag}.ski"
    path.write_text(text)
    sim = Simulation(str(path), num_packets=n).setup()
    assert (sim.radiation_field_size > 0) == ("rf" in tag)
    _bintree_against_the_oracle("cfg2bin " + tag, sim, n, 777)


# ---------------------------------------------------------------------------------------------------------------- all three together

_combined = {}


def _combined_scene():
    """cfg2binall: one oracle run with the extension, one without; shared, and nobody changes the arrays"""
    if not _combined:
        sim = Simulation(ski("cfg2binall.ski"), num_packets=N).setup()
        assert sim.phase_functions[0] == 1 and sim.source_velocities[0]["kind"] == 3 and B.Tree(sim).kind == 4
        ref, counters = O.run_primary(sim, 0, N, O.RNG_PHILOX, seed=SEED, ext=True)
        plain, _ = O.run_primary(sim, 0, N, O.RNG_PHILOX, seed=SEED)
        ref.setflags(write=False)
        plain.setflags(write=False)
        # the velocities differ by more than one wavelength bin across the launch positions: the edge-on observer sees the line in
        # more than three bins, the scene at rest in at most two
        lay = sim.layout(0)
        row = slice(lay.sed_offset, lay.sed_offset + lay.num_lambda)
        assert np.count_nonzero(ref[row]) > 3 and np.count_nonzero(plain[row]) <= 2
        _scattered_blocks_are_filled(sim, ref)
        _combined.update(sim=sim, ref=ref, plain=plain, counters=counters)
    return _combined["sim"], _combined["ref"], _combined["plain"], _combined["counters"]


@pytest.mark.parametrize("slots,groups", [(None, None), (4096, "1"), (4096, "3")])
def test_dipole_and_doppler_on_a_binary_tree_match_the_oracle(monkeypatch, slots, groups):
    """cfg2binall -- a binary tree holding one electron component, panchromatic, a rotating disk of sources, three observers and a shared
    one -- runs transitionKinDipoleKernel on the binary tree's walk kernels: the whole buffer against the oracle; and again in 4096
    slots, each taken up by five histories with its per-observer values, in one slot group and in three"""
    sim, ref, plain, counters = _combined_scene()
    if groups:
        monkeypatch.setenv("PMC_NUM_GROUPS", groups)   # (read by pmc_create)
    eng = _engine(sim)
    if slots:
        eng.set_num_slots(slots)
    eng.run_primary(0, N, SEED)
    gpu, c = eng.download(), eng.counters()
    if slots:
        assert eng.last_timing()["generations"] >= N / slots
    eng.close()
    _same_work(c, counters, N)
    _report(f"cfg2binall slots={slots} groups={groups}", sim, gpu, ref)
    _compare_frames(sim, gpu, ref, N, two_bins_per_history=True)
    with pytest.raises(AssertionError):
        _compare_frames(sim, gpu, plain, N, two_bins_per_history=True)
