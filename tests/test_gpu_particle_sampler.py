"""The density of a smoothed-particle medium on the MI355X (pmc_sampler_create: sampleDensityKernel<K>) at small shapes.

ParticleSampler.density must EQUAL the pure-Python restatement of the kernel (tests/particle_checks.py) bit for bit, for the cubic-spline and
for the uniform smoothing kernel, on hand-made tables: three blocks per axis, culled lists, one empty block; positions on the separators, at
u = 0, 0.5 and 1 of a particle (bit-exact by construction), far outside every sphere and not-a-number included.  No test provokes the device
error path."""
import numpy as np
import pytest

import particle_checks as P
from skirt9_amd.engine import ParticleSampler

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 65, 1000)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case(kernel):
    """(tables, 1000 positions in a fixed mixed order, the restatement's densities there), computed once"""
    if kernel not in _cache:
        tables = P.make_tables(kernel)
        points = P.point_set(tables)
        _cache[kernel] = (tables, points, P.densities(tables, kernel, points))
    return _cache[kernel]


@pytest.mark.parametrize("kernel", P.KERNELS, ids=["cubic_spline", "uniform"])
def test_densities_equal_the_restatement(kernel):
    tables, points, want = _case(kernel)
    assert (want == 0).sum() >= P.NUM_FAR + P.NUM_ODD and (want > 0).sum() >= 2 * P.NUM_PARTICLES  # (as tests/test_particle_checks.py checks on the host)
    sampler = ParticleSampler(tables, 0)
    for n in COUNTS:
        first = 0 if n == 1000 else 32
        got = sampler.density(points[first:first + n])
        assert got.shape == (n,) and np.array_equal(_bits(got), _bits(want[first:first + n])), (kernel, n)
    # the order of the positions does not matter
    order = np.random.default_rng(4).permutation(1000)
    assert np.array_equal(_bits(sampler.density(points[order])), _bits(want[order]))
    sampler.close()
