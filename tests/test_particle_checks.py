"""The yardstick of the particle sampler's GPU test (tests/particle_checks.py) checked against itself on the host: the hand-made tables are
what they claim to be, and culling the block lists by the spheres' bounding boxes changes no density."""
import numpy as np
import pytest

import particle_checks as P


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_tables_are_what_the_checks_need():
    tables = P.make_tables(P.KERNEL_CUBIC_SPLINE)
    particle, start, members = tables["particle"], tables["block_start"], tables["block_list"]
    assert particle.shape == (P.NUM_PARTICLES, 5) and (particle[:, 3:] > 0).all()
    assert (particle[:, :4] * 16 == np.round(particle[:, :4] * 16)).all()  # dyadic coordinates and smoothing lengths
    assert len(start) == P.NUM_BLOCKS ** 3 + 1 and start[0] == 0 and start[-1] == len(members)
    for b in range(P.NUM_BLOCKS ** 3):
        block = members[start[b]:start[b + 1]]
        assert (np.diff(block) > 0).all()  # ascending
    assert P.empty_blocks(tables) == [P.NUM_BLOCKS ** 3 - 1]  # the block of a not-a-number position, and only that one
    assert len(members) < P.NUM_PARTICLES * P.NUM_BLOCKS ** 3  # (the lists are culled)
    full = P.make_tables(P.KERNEL_CUBIC_SPLINE, culled=False)
    assert len(full["block_list"]) == P.NUM_PARTICLES * P.NUM_BLOCKS ** 3 and np.array_equal(full["particle"], particle)
    points = P.point_set(tables)
    assert points.shape == (1000, 3) and np.isnan(points).any(axis=1).sum() == P.NUM_ODD
    for axis in range(3):
        assert all((points[:, axis] == s).sum() >= 8 for s in P.SEPARATORS)  # points exactly on the separators


def test_locate_clip_on_the_separators():
    grid = [-float("inf"), -1.0, 1.5, float("inf")]
    assert [P.locate_clip(grid, x) for x in (-1e300, np.nextafter(-1.0, -2.), -1.0, 0., np.nextafter(1.5, 0.), 1.5, 1e300, float("inf"))] \
        == [0, 0, 1, 1, 1, 2, 2, 2]
    assert P.locate_clip(grid, float("nan")) == 2
    assert P.locate_clip([0., 1., 2.], -5.) == 0 and P.locate_clip([0., 1., 2.], 7.) == 1


def test_the_kernels_at_their_edges():
    assert P.cubic_spline(0.) == 8.0 / np.pi and P.cubic_spline(1.) == 0. and P.cubic_spline(np.nextafter(1., 0.)) > 0.
    assert P.cubic_spline(0.5) == 8.0 / np.pi * 2.0 * 0.5 * 0.5 * 0.5 == 8.0 / np.pi * (1.0 - 6.0 * 0.5 * 0.5 * 0.5)
    assert P.uniform(0.) == P.uniform(1.) == 0.75 / np.pi and P.uniform(np.nextafter(1., 2.)) == 0.


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_culled_lists_give_the_densities_of_full_lists(kernel):
    """a particle whose bounding box does not reach the block of a position is farther than h from it: its term is +0.0, and adding it
    changes no bit of the sum"""
    tables = P.make_tables(kernel)
    points = P.point_set(tables)
    got = P.densities(tables, kernel, points)
    want = P.densities(P.make_tables(kernel, culled=False), kernel, points)
    odd = np.isnan(points).any(axis=1)
    # (the position that is not a number: its block is empty, so 0; with full lists the device's uniform kernel, whose comparisons all fail for
    # a distance that is not a number, would count every particle -- particle_checks.py)
    assert (got[odd] == 0).all()
    if kernel == P.KERNEL_UNIFORM:
        assert (want[odd] > 0).all()
        got, want = got[~odd], want[~odd]
    assert np.array_equal(_bits(got), _bits(want))
    # both zero and positive densities: the far points and the odd one at least; the points at u = 0 and u = 0.5 of every particle at least
    got = P.densities(tables, kernel, points)
    assert (got == 0).sum() >= P.NUM_FAR + P.NUM_ODD and (got > 0).sum() >= 2 * P.NUM_PARTICLES
    assert np.isfinite(got).all() and (got >= 0).all()


def test_the_edge_of_a_sphere_counts_for_the_uniform_kernel_only():
    """u = 1 bit-exact by construction: a single particle in every block, a point at the offset h from it"""
    tables = P.make_tables(P.KERNEL_UNIFORM, culled=False)
    x, y, z, h, rho = tables["particle"][0].tolist()
    tables["block_list"] = np.zeros(P.NUM_BLOCKS ** 3, dtype=np.int32)
    tables["block_start"] = np.arange(P.NUM_BLOCKS ** 3 + 1, dtype=np.int64)
    edge = np.array([[x + h, y, z], [x, y - h, z], [x, y, z + h], [x + 0.5 * h, y, z], [x, y, z]])
    assert (P.densities(tables, P.KERNEL_UNIFORM, edge) == 0.75 / np.pi * rho).all()
    cubic = P.densities(tables, P.KERNEL_CUBIC_SPLINE, edge)
    assert (cubic[:3] == 0).all() and cubic[3] == 8.0 / np.pi * 2.0 * 0.5 * 0.5 * 0.5 * rho and cubic[4] == 8.0 / np.pi * rho
