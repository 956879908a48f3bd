"""Reused photon slots against the oracle (run on the MI355X box with `pytest -m gpu`).

The engine keeps a fixed pool of slots; once a slot's history ends, the launch kernel gives it the next history index
(endedScanKernel counts and scans the ended histories per 64-slot tile and reserves a range of the shared cursor;
launchKernel flushes the ended history's statistics list, returns its pool blocks and launches the next history into
the slot).  The parity tests of test_gpu_parity run at most 250 000 histories, fewer than the default pool holds, so
every history there gets a fresh slot.  Here the pool is capped (pmc_set_num_slots, PMC_NUM_GROUPS) far below the
number of histories, so every slot runs many histories one after the other -- in one wave, in partial 64-slot tiles,
in several slot groups with a partial last group, with slot counts that change on one context, at history indices
beyond 32 bits -- and the frames, the counted work and the radiation field must agree with the oracle, which keys every
Philox stream by (seed, history index) and does not know about slots.  Tolerances are those of test_gpu_parity.
"""
import numpy as np
import pytest

import oracle_lib as O
from conftest import ski
from skirt9_amd.engine import set_tuning
from skirt9_amd.host import Simulation
from test_gpu_multi import _many_events
from test_gpu_parity import _compare_frames

pytestmark = pytest.mark.gpu

SEED = 271828
OCTREE = ("cfg2", "cfg4")

_sims = {}
_oracle = {}


def _sim(path, n):
    key = (path, n)
    if key not in _sims:
        _sims[key] = Simulation(path, num_packets=n).setup()
    return _sims[key]


def _reference(path, first, n, seed, rf=False, ext=False):
    """oracle frames (and field) of histories [first, first + n) of the scene at `path`: once per module, whatever the slot count
    (ext: the oracle follows the scene's dipole phase functions and moving sources, oracle_lib.run_primary)"""
    key = (path, first, n, seed, rf, ext)
    if key not in _oracle:
        sim = _sim(path, n)
        if rf:
            _oracle[key] = O.run_primary_rf(sim, first, n, O.RNG_PHILOX, seed=seed, ext=ext)
        else:
            frames, counters = O.run_primary(sim, first, n, O.RNG_PHILOX, seed=seed, ext=ext)
            _oracle[key] = (frames, None, counters)
    return _oracle[key]


def _engine(sim, slots):
    from skirt9_amd.engine import Engine
    eng = Engine(sim.scene, 0)
    eng.set_num_slots(slots)
    return eng


def _check_counters(c, counters, n):
    assert c["histories"] == n
    assert c["stat_overflows"] == 0
    assert abs(c["cell_visits"] - counters.cell_visits) <= 1e-4 * counters.cell_visits
    assert abs(c["scatterings"] - counters.scatterings) <= 1e-4 * counters.scatterings + 2


def _check_field(gpu_rf, ref_rf):
    assert abs(gpu_rf.sum() - ref_rf.sum()) <= 1e-9 * ref_rf.sum()
    assert np.array_equal(gpu_rf > 0, ref_rf > 0)
    bad = np.abs(gpu_rf - ref_rf) > 1e-6 * np.abs(ref_rf) + 1e-13 * ref_rf.max()
    assert bad.sum() == 0, int(bad.sum())


def _check_pool(eng, name, slots, n):
    """the cap was applied: the octree's pool holds `slots` slots; every scene ran at least n / slots generations"""
    if name.startswith(OCTREE):
        assert eng.debug_tables().num_slots == slots
    assert eng.last_timing()["generations"] >= n / slots


def _run_and_compare(path, name, n, slots, first=0, seed=SEED, ext=False, two_bins_per_history=False):
    """returns the engine's frames and counters"""
    sim = _sim(path, n)
    eng = _engine(sim, slots)
    eng.run_primary(first, n, seed)
    gpu = eng.download()
    c = eng.counters()
    _check_pool(eng, name, slots, n)
    eng.close()
    ref, _, counters = _reference(path, first, n, seed, ext=ext)
    _check_counters(c, counters, n)
    _compare_frames(sim, gpu, ref, n, two_bins_per_history=two_bins_per_history)
    return gpu, c


SCENES = [("cfg1.ski", 20000), ("cfg1mesh2.ski", 20000), ("cfg1nf.ski", 50000), ("cfg1nfea.ski", 50000), ("cfg1laser.ski", 20000),
          ("cfg1sed.ski", 20000), ("cfg1nomed.ski", 20000),
          ("cfg2small.ski", 20000), ("cfg2deep.ski", 20000), ("cfg2deeper.ski", 20000), ("cfg4deepest.ski", 20000), ("cfg2nf.ski", 50000),
          ("cfg2ea.ski", 20000), ("cfg2mm.ski", 20000), ("cfg2mmea.ski", 20000), ("cfg2agn.ski", 20000), ("cfg4small.ski", 20000),
          ("cfg3small.ski", 20000), ("cfg3ten.ski", 20000), ("cfg3twelve.ski", 20000), ("cfg3z.ski", 20000), ("cfg3sed.ski", 20000),
          ("cfg5small.ski", 20000)]


@pytest.mark.parametrize("name,n", SCENES)
def test_scene_in_1000_reused_slots(name, n):
    """one scene per kernel flavour in 1000 slots: 20-50 histories per slot; 1000 is not a multiple of 64 (a partial last wave tile)
    and below the 1024-slot alignment of the slot groups.  (cfg1nomed, a point source without a medium, gives every history the same
    contribution: it checks the counts and the emission peel-off kernel, not which histories ran.)"""
    _run_and_compare(ski(name), name, n, 1000)


@pytest.mark.parametrize("name", ["cfg1.ski", "cfg2small.ski", "cfg3small.ski", "cfg5small.ski", "cfg2nf.ski"])
def test_scene_in_one_wave_of_slots(name):
    """64 slots, one wave: every generation launches into the same 64 slots, about 80 histories each"""
    _run_and_compare(ski(name), name, 5000, 64)


@pytest.mark.parametrize("name,n,slots,groups,log", [("cfg1.ski", 600000, 200003, None, None), ("cfg2small.ski", 600000, 200003, None, None),
                                                     ("cfg3small.ski", 600000, 200003, None, None), ("cfg5small.ski", 600000, 200003, "3", None),
                                                     ("cfg2small.ski", 800000, 266241, "4", None), ("cfg2small.ski", 600000, 200003, None, "4096")])
def test_several_slot_groups_with_refills(name, n, slots, groups, log, monkeypatch):
    """three (four) slot groups over one history cursor, the last group partial, each slot refilled two to three times; Voronoi runs
    one group unless PMC_NUM_GROUPS asks for more; with a statistics log of one chunk per group the log fills and is flushed between
    the refills"""
    if groups:
        monkeypatch.setenv("PMC_NUM_GROUPS", groups)   # (read by pmc_create)
    if log:
        set_tuning("PMC_STAT_LOG_ENTRIES", log)
    _run_and_compare(ski(name), name, n, slots)


@pytest.mark.parametrize("slots,pool", [(64, None), (1000, None), (64, "16"), (1000, "16")])
def test_statistics_lists_in_reused_slots(tmp_path, monkeypatch, slots, pool):
    """histories of 120 scattering events leave more than 48 distinct pixels, which continue in chained blocks of the group's pool; the
    blocks a history held go back to the free stack when its slot is refilled and are taken again by later histories.  What
    test_statistics_lists_are_unbounded asserts, in 64 and in 1000 slots, with the default pool and with 16 blocks (the pool grows)."""
    if pool:
        monkeypatch.setenv("PMC_STAT_POOL_BLOCKS", pool)
    n = 2000
    path = _many_events(tmp_path, 120)
    sim = Simulation(path, num_packets=n).setup()
    eng = _engine(sim, slots)
    eng.run_primary(0, n, 1)
    gpu = eng.download()
    c = eng.counters()
    assert eng.debug_tables().num_slots == slots
    eng.close()
    assert c["histories"] == n
    assert c["stat_overflows"] == 0 and c["scatterings"] >= 100 * n
    key = ("events120", 0, n, 1)
    if key not in _oracle:
        _oracle[key] = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=1)
    ref, counters = _oracle[key]
    assert abs(c["cell_visits"] - counters.cell_visits) <= 1e-4 * counters.cell_visits
    _compare_frames(sim, gpu, ref, n)
    lay = sim.layout(0)
    npix = lay.npix * lay.num_lambda
    for k in range(5):
        a = gpu[lay.wifu_offset + k * npix:lay.wifu_offset + (k + 1) * npix]
        b = ref[lay.wifu_offset + k * npix:lay.wifu_offset + (k + 1) * npix]
        assert abs(a.sum() - b.sum()) <= 1e-9 * np.abs(b).sum()
    assert ref[lay.wifu_offset:lay.wifu_offset + npix].sum() > 50 * n
    assert gpu[lay.wifu_offset:lay.wifu_offset + npix].sum() == ref[lay.wifu_offset:lay.wifu_offset + npix].sum()


@pytest.mark.parametrize("name", ["cfg1rf.ski", "cfg3rf.ski", "cfg1mmrf.ski"])
def test_radiation_field_in_reused_slots(name):
    """the radiation field and the frames in 1000 slots (octree: a per-slot log of 128 entries over 1000 slots is small, waves that find
    it full add their contributions atomically -- the two mix) against run_primary_rf, with the tolerances of
    test_radiation_field_matches_oracle"""
    n, slots = 20000, 1000
    path = ski(name)
    sim = _sim(path, n)
    eng = _engine(sim, slots)
    assert eng.radiation_field_size == sim.radiation_field_size > 0
    eng.run_primary(0, n, SEED)
    gpu = eng.download()
    gpu_rf = eng.download_radiation_field()
    c = eng.counters()
    _check_pool(eng, name, slots, n)
    eng.close()
    ref, ref_rf, counters = _reference(path, 0, n, SEED, rf=True)
    _check_counters(c, counters, n)
    _check_field(gpu_rf, ref_rf)
    _compare_frames(sim, gpu, ref, n)


@pytest.mark.parametrize("name", ["cfg2small.ski", "cfg5small.ski"])
def test_slot_counts_that_change_on_one_context(name):
    """one context, three segments: [0, 6000) in 4097 slots, [6000, 9000) in 64 (fewer slots than the pool holds), [9000, 30000) in
    30000 (the pool grows: slot arrays, peel-off records and the statistics pool are allocated again); the frames accumulate and
    must equal the oracle's over [0, 30000)"""
    n = 30000
    path = ski(name)
    sim = _sim(path, n)
    from skirt9_amd.engine import Engine
    eng = Engine(sim.scene, 0)
    for first, count, slots, pool in ((0, 6000, 4097, 4097), (6000, 3000, 64, 4097), (9000, 21000, 30000, 21000)):
        eng.set_num_slots(slots)
        eng.run_primary(first, count, SEED)
        eng.sync()
        if name.startswith(OCTREE):
            assert eng.debug_tables().num_slots == pool   # (the pool grows to the segment's histories at most, and never shrinks)
        assert eng.last_timing()["generations"] >= count / min(slots, count)
    gpu = eng.download()
    c = eng.counters()
    eng.close()
    ref, _, counters = _reference(path, 0, n, SEED)
    _check_counters(c, counters, n)
    _compare_frames(sim, gpu, ref, n)


@pytest.mark.parametrize("first", [2 ** 32 - 9000, 2 ** 40 + 12345])
@pytest.mark.parametrize("name", ["cfg2small.ski", "cfg5small.ski"])
def test_history_indices_beyond_32_bits(name, first):
    """history indices that cross 2^32 in the refills (the boundary between the two counter words of pmc_philox.h), or start beyond 2^40"""
    _run_and_compare(ski(name), name, 20000, 1000, first=first)
