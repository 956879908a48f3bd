"""Batched ray integrals (pmc_integrate_rays) and the probe maps built on them, on the MI355X.

The integrator walks many rays at once, one per lane, with the traversal functions of the single-ray tracer, and adds ds * q[m] in path order
without contraction: its double results must EQUAL the sum over pmc_trace_ray's segments bit for bit, on every grid kind, for every ray
count around the wave size, and whatever the order of the rays.  The probe files written through it are the reference's byte for byte
(tests/golden/make_golden_probes.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import probe_checks as P
from conftest import ROOT, ski
from skirt9_amd.engine import INTEGRATE_BATCH_RAYS, INTEGRATE_PASS_VALUES, Engine, clear_tuning, set_tuning
from skirt9_amd.host import Simulation, scene_head

pytestmark = pytest.mark.gpu

SCENES = ["cfg1", "cfg2small", "cfg2deep", "cfg2bin", "cfg5small"]  # Cartesian, octree (10-bit indices), octree (21-bit), binary tree, Voronoi
V = INTEGRATE_PASS_VALUES + 1  # one more than a pass holds: two passes, the second with one value
NUM_RAYS = 1000
CAP = 65536


def _rays(sim):
    """NUM_RAYS rays: [0, 64) the same ray in every lane of a wave; then rays from random points inside the grid, rays from outside aimed at
    the grid, rays from outside that miss it, and axis-parallel rays from outside that run in planes where cell faces lie (the borders of
    a Cartesian grid, the dyadic planes of a tree's root box)"""
    g = scene_head(sim).grid
    lo, hi = np.array([g.xmin, g.ymin, g.zmin]), np.array([g.xmax, g.ymax, g.zmax])
    rng = np.random.default_rng(20261018)

    def unit(n):
        k = rng.normal(size=(n, 3))
        return k / np.linalg.norm(k, axis=1)[:, None]

    r, k = [], []
    one_r, one_k = lo + (hi - lo) * np.array([0.31, 0.47, 0.62]), unit(1)[0]
    r += [one_r] * 64
    k += [one_k] * 64
    n_in, n_out, n_miss, n_axis = 400, 300, 100, 136
    r += list(lo + (hi - lo) * rng.random((n_in, 3)))
    k += list(unit(n_in))
    centre, radius = 0.5 * (lo + hi), np.linalg.norm(hi - lo)
    for _ in range(n_out):
        origin = centre + 2. * radius * unit(1)[0]
        aim = lo + (hi - lo) * rng.random(3)
        d = aim - origin
        r.append(origin)
        k.append(d / np.linalg.norm(d))
    for _ in range(n_miss):
        away = unit(1)[0]
        r.append(centre + 2. * radius * away)
        if rng.random() < 0.5:
            k.append(away)  # (away from the grid)
        else:
            t = np.cross(away, unit(1)[0])  # (past it: the line keeps two diagonals' distance from the centre)
            k.append(t / np.linalg.norm(t))
    fractions = [0.5, 0.25, 0.75, 0.125, 0.375, 0.0, 1.0]
    for i in range(n_axis):
        axis, sign = i % 3, 1. if (i // 3) % 2 == 0 else -1.
        a, b = (axis + 1) % 3, (axis + 2) % 3
        origin = np.empty(3)
        origin[axis] = centre[axis] - sign * 2. * radius
        origin[a] = lo[a] + (hi[a] - lo[a]) * fractions[(i // 6) % len(fractions)]
        origin[b] = lo[b] + (hi[b] - lo[b]) * (fractions[(i // 42) % len(fractions)] if i % 2 else rng.random())
        d = np.zeros(3)
        d[axis] = sign
        r.append(origin)
        k.append(d)
    assert len(r) == NUM_RAYS
    return np.array(r), np.array(k)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sim, origins, directions, cell values [V][num_cells], reference sums [NUM_RAYS][V], segments per ray): the reference is the sum over
    Engine.trace_ray's segments with m >= 0, in order, one IEEE product and one IEEE sum each; computed once per scene"""
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    r, k = _rays(sim)
    num_cells = scene_head(sim).grid.num_cells
    q = np.random.default_rng(7).random((V, num_cells)) + 0.5
    eng = Engine(sim.scene, 0)
    ref = np.zeros((NUM_RAYS, V))
    count = np.zeros(NUM_RAYS, dtype=np.int64)
    last = None
    for i in range(NUM_RAYS):
        if last is not None and np.array_equal(r[i], r[last]) and np.array_equal(k[i], k[last]):
            ref[i], count[i] = ref[last], count[last]
            continue
        m, ds = eng.trace_ray(r[i], k[i], cap=CAP)
        assert len(m) < CAP
        ref[i] = P.path_sum(m, ds, q)
        count[i] = (m >= 0).sum()
        last = i
    eng.close()
    return sim, r, k, q, ref, count


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", SCENES)
def test_integrals_equal_the_sum_over_the_traced_segments(name):
    """bit for bit, for 0, 1, 63, 64, 65 and 1000 rays and for V = 1 and V = one more than a pass holds"""
    sim, r, k, q, ref, count = _case(name)
    # from the ray set alone: it holds what it is meant to hold
    assert (count == 0).sum() >= 50 and np.all(ref[count == 0] == 0.) and (count > 1).sum() > 500
    eng = Engine(sim.scene, 0)
    for n in (0, 1, 63, 64, 65, NUM_RAYS):
        first = 0 if n == NUM_RAYS else 32  # (a window over the end of the identical rays and the start of the random ones)
        sel = slice(first, first + n)
        many = eng.integrate_rays(r[sel], k[sel], q)
        assert many.shape == (n, V)
        assert _same_bits(many, ref[sel]), (name, n, int((many != ref[sel]).sum()))
        one = eng.integrate_rays(r[sel], k[sel], q[0])
        assert one.shape == (n,)
        assert _same_bits(one, ref[sel, 0]), (name, n)
    work = eng.last_integrate_work()
    assert work["lane_steps"] == count.sum() and 0 < work["wave_steps"] <= work["lane_steps"]
    eng.close()


@pytest.mark.parametrize("name", SCENES)
def test_order_of_the_rays_does_not_matter(name):
    sim, r, k, q, ref, _ = _case(name)
    perm = np.random.default_rng(11).permutation(NUM_RAYS)
    eng = Engine(sim.scene, 0)
    assert _same_bits(eng.integrate_rays(r[perm], k[perm], q), ref[perm])
    eng.close()


def test_more_rays_than_one_batch():
    """INTEGRATE_BATCH_RAYS + 65 rays on cfg1, the ray set tiled (ray i = set[i % NUM_RAYS]), V values: two batches of two passes each, the
    second batch a wave and one lane -- where a batch offset and a pass offset meet"""
    sim, r, k, q, ref, count = _case("cfg1")
    tile = np.arange(INTEGRATE_BATCH_RAYS + 65) % NUM_RAYS
    eng = Engine(sim.scene, 0)
    sums = eng.integrate_rays(r[tile], k[tile], q)
    work = eng.last_integrate_work()
    eng.close()
    assert sums.shape == (len(tile), V)
    assert _same_bits(sums, ref[tile]), int((sums != ref[tile]).any(axis=1).sum())
    # the tiled segment count, once per pass: each of the two passes walks every ray of its batch (224 202 842 = 2 x 112 101 421)
    assert work["lane_steps"] == 2 * count[tile].sum()


def test_argument_errors_are_reported():
    sim, r, k, q, _, _ = _case("cfg1")
    eng = Engine(sim.scene, 0)
    with pytest.raises(ValueError):
        eng.integrate_rays(r[:4], k[:4], q[:, :-1])
    with pytest.raises(ValueError):
        eng.integrate_rays(r[:4], k[:3], q)
    from skirt9_amd.engine import lib
    assert lib().pmc_integrate_rays(eng._h, -1, None, None, 1, None, None) != 0
    assert b"negative" in lib().pmc_last_error()
    assert lib().pmc_integrate_rays(eng._h, 1, None, None, 1, None, None) != 0
    assert b"null" in lib().pmc_last_error()
    eng.close()


@pytest.mark.parametrize("name", ["cfg2small", "cfg5small"])
def test_sums_do_not_depend_on_what_device_memory_held(name):
    """PMC_POISON_ALLOCATIONS fills what the engine allocates without initialising with 0xA5 bytes (the integrator's own buffers too)"""
    sim, r, k, q, ref, _ = _case(name)
    set_tuning("PMC_POISON_ALLOCATIONS")
    try:
        eng = Engine(sim.scene, 0)
        poisoned = eng.integrate_rays(r, k, q)
        eng.close()
    finally:
        clear_tuning()
    assert _same_bits(poisoned, ref)


def test_the_photon_loop_is_untouched(monkeypatch):
    """run_primary after integrate_rays on the same context gives the frames it gives without the integration: cfg1, 10^4 packets, equality
    of every element.

    Equality of two runs needs a photon loop that is reproducible to the bit, which it is not in its default configuration: the statistics
    log adds a bin's w^k in the order the waves claimed their entries (two plain runs differ in about 7000 of the 20480 entries of the statistics
    frames, by up to 2e-15 of the largest; the flux arrays are equal already).  With the engine's own settings for one slot group,
    64 slots -- one wave -- and the statistics added by atomics (PMC_NUM_GROUPS, pmc_set_num_slots, PMC_STAT_ATOMICS) the same histories
    give the same bits every time: the test first proves that on two plain runs, so that the comparison with the run behind the integration
    says something, and then asks for the same bits there.  The integrator also gives its own bits before and after the photon loop."""
    n = 10000
    sim, r, k, q, ref, _ = _case("cfg1")
    monkeypatch.setenv("PMC_NUM_GROUPS", "1")
    set_tuning("PMC_STAT_ATOMICS")

    def photon_loop(integrate):
        eng = Engine(sim.scene, 0)
        eng.set_num_slots(64)
        if integrate:
            assert _same_bits(eng.integrate_rays(r, k, q), ref)
        eng.run_primary(0, n, 99)
        frames, counters = eng.download(), eng.counters()
        if integrate:
            assert _same_bits(eng.integrate_rays(r, k, q), ref)
        eng.close()
        return frames, counters

    base, base_counters = photon_loop(False)
    again, again_counters = photon_loop(False)
    assert base_counters["histories"] == n and base.sum() > 0
    assert again_counters == base_counters and np.array_equal(again, base)  # (the configuration is reproducible)
    frames, counters = photon_loop(True)
    assert counters == base_counters
    assert np.array_equal(frames, base), int((frames != base).sum())


@pytest.mark.parametrize("name", P.GOLDEN_SCENES)
def test_probe_files_are_the_reference_s(name, tmp_path):
    """write_probes with the engine as the integrator: every file byte-identical to the reference's (FITS: apart from the DATE card)"""
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    eng = Engine(sim.scene, 0)
    sim.write_probes(str(tmp_path), eng)
    eng.close()
    P.assert_files_equal_golden(name, str(tmp_path))


def test_driver_writes_the_probe_files(tmp_path):
    """skirt_mi355x -o out tests/ski/cfg1probe.ski: the probe files next to the instrument files, the reference's bytes"""
    exe = os.path.join(ROOT, "skirt9_amd", "lib", "skirt_mi355x")
    subprocess.check_call([exe, "-o", str(tmp_path), ski("cfg1probe.ski")], cwd=ROOT, timeout=300)
    assert "cfg1probe_i0_total.fits" in os.listdir(tmp_path)
    P.assert_files_equal_golden("cfg1probe", str(tmp_path))
