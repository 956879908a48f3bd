"""Shared by tests/test_host_bintree.py, tests/test_gpu_bintree.py and tests/golden/make_golden_bintree.py: the flattened tree of a
set-up Simulation, a literal restatement of the reference's tree path generator over it, the ray fixtures, and the comparison of two
runs of one scene block by block with the Monte Carlo noise of both.  TEST INFRASTRUCTURE ONLY."""
import math
import os

import numpy as np

DBL_MAX = 1.7976931348623157e308

from electron_checks import read_fits, rebin  # noqa: F401

FRAMES = ("total", "transparent", "stats0", "stats1", "stats2")
INSTRUMENTS = ("i0", "i1", "i2")


class Tree:
    """the node arrays of pmc_grid (include/pmc.h) of a set-up Simulation, as Python lists (plain floats and ints)"""

    def __init__(self, sim):
        from skirt9_amd.host import scene_head
        g = scene_head(sim).grid
        n = g.num_nodes
        self.kind = int(g.kind)
        self.num_nodes = n
        self.num_cells = int(g.num_cells)
        self.eps = float(g.eps)
        self.extent = (g.xmin, g.ymin, g.zmin, g.xmax, g.ymax, g.zmax)
        self.box_array = np.ctypeslib.as_array(g.node_box, shape=(n, 6)).copy()
        self.level_array = np.ctypeslib.as_array(g.node_level, shape=(n,)).copy()
        self.first_array = np.ctypeslib.as_array(g.node_first_child, shape=(n,)).copy()
        self.cell_array = np.ctypeslib.as_array(g.node_cell, shape=(n,)).copy()
        self.start_array = np.ctypeslib.as_array(g.nbr_start, shape=(6 * n + 1,)).copy()
        self.list_array = np.ctypeslib.as_array(g.nbr_list, shape=(int(self.start_array[-1]),)).copy()
        self.box = self.box_array.tolist()
        self.level = self.level_array.tolist()
        self.first = self.first_array.tolist()
        self.cell = self.cell_array.tolist()
        self.start = self.start_array.tolist()
        self.list = self.list_array.tolist()


def octree_child(tree, node, r):
    """OctTreeNode::child (OctTreeNode.cpp:37-42): the child index from three `<` decisions against child 0's upper corner"""
    c0 = tree.box[tree.first[node]]
    return (0 if r[0] < c0[3] else 1) + (0 if r[1] < c0[4] else 2) + (0 if r[2] < c0[5] else 4)


def bintree_child(tree, node, r):
    """BinTreeNode::child (BinTreeNode.cpp:53-62): r.a < CHILD_0->max.a on the split axis level % 3"""
    axis = tree.level[node] % 3
    return 0 if r[axis] < tree.box[tree.first[node]][3 + axis] else 1


def _contains(b, r):
    """Box::contains (closed box)"""
    return b[0] <= r[0] <= b[3] and b[1] <= r[1] <= b[4] and b[2] <= r[2] <= b[5]


def trace(tree, r, k, num_children, child):
    """TreeSpatialGrid::MySegmentGenerator::next (TreeSpatialGrid.cpp:84-216), literally, over the flattened arrays: returns the list of
    (cell index m, ds).  `num_children` is what a subdivided node has (8 or 2, consecutive ids), `child(tree, node, r)` its child rule."""
    assert num_children in (2, 8)
    ext = tree.extent
    eps = tree.eps
    r = [float(v) for v in r]
    kx, ky, kz = (float(v) for v in k)
    out = []

    def leaf_child(r):
        # TreeNode::leafChild on the root: nullptr outside the (closed) root box
        node = 0
        if not _contains(tree.box[0], r):
            return -1
        while tree.first[node] >= 0:
            node = tree.first[node] + child(tree, node, r)
        return node

    def propagate(ds):
        r[0] += kx * ds
        r[1] += ky * ds
        r[2] += kz * ds

    # ---- State::Unknown: PathSegmentGenerator::moveInside(extent, eps) (PathSegmentGenerator.cpp:11-112): the coordinate that is
    # outside is SET to the wall plus or minus eps, the other two advance; then the closed-box test
    def move_inside():
        cumds = 0.
        for a in range(3):
            ka = (kx, ky, kz)[a]
            lo, hi = ext[a], ext[3 + a]
            if r[a] <= lo:
                if ka <= 0.0:
                    return None
                ds = (lo - r[a]) / ka
                target = lo + eps
            elif r[a] >= hi:
                if ka >= 0.0:
                    return None
                ds = (hi - r[a]) / ka
                target = hi - eps
            else:
                continue
            propagate(ds)
            r[a] = target
            cumds += ds
        if not _contains(ext, r):
            return None
        return cumds

    moved = move_inside()
    if moved is None:
        return out
    node = leaf_child(r)
    if node < 0:
        return out
    if moved > 0.:
        out.append((-1, moved))

    # ---- State::Inside
    while True:
        b = tree.box[node]
        xnext = b[0] if kx < 0.0 else b[3]
        ynext = b[1] if ky < 0.0 else b[4]
        znext = b[2] if kz < 0.0 else b[5]
        dsx = (xnext - r[0]) / kx if abs(kx) > 1e-15 else DBL_MAX
        dsy = (ynext - r[1]) / ky if abs(ky) > 1e-15 else DBL_MAX
        dsz = (znext - r[2]) / kz if abs(kz) > 1e-15 else DBL_MAX
        if dsx <= dsy and dsx <= dsz:
            ds = dsx
            wall = 0 if kx < 0.0 else 1
        elif dsy <= dsx and dsy <= dsz:
            ds = dsy
            wall = 2 if ky < 0.0 else 3
        else:
            ds = dsz
            wall = 4 if kz < 0.0 else 5
        propagate(ds + eps)
        out.append((tree.cell[node], ds))
        old = node
        # TreeNode::neighbor(wall, r): the first neighbour in list order whose closed box contains r
        node = -1
        for q in tree.list[tree.start[6 * old + wall]:tree.start[6 * old + wall + 1]]:
            if _contains(tree.box[q], r):
                node = q
                break
        if node < 0:
            node = leaf_child(r)
        if node == old:
            # PathSegmentGenerator::propagateToNextAfter
            r[0] = math.nextafter(r[0], -DBL_MAX if kx < 0. else DBL_MAX)
            r[1] = math.nextafter(r[1], -DBL_MAX if ky < 0. else DBL_MAX)
            r[2] = math.nextafter(r[2], -DBL_MAX if kz < 0. else DBL_MAX)
            node = leaf_child(r)
        if node < 0 or node == old:
            return out


def read_rays(path):
    """[(r, k)] of a *_rays.txt fixture (hex floats)"""
    rays = []
    for line in open(path):
        v = [float.fromhex(t) for t in line.split()]
        rays.append((v[:3], v[3:]))
    return rays


def read_ray_dump(path):
    """the reference's dump (skirt_ref rays): per ray (normalised direction, [m], [ds])"""
    out = []
    lines = open(path).read().split("\n")
    at = 0
    while at < len(lines) and lines[at].startswith("ray"):
        t = lines[at].split()
        n = int(t[2])
        k = [float.fromhex(v) for v in t[3:6]]
        seg = [lines[at + 1 + i].split() for i in range(n)]
        out.append((k, [int(s[0]) for s in seg], [float.fromhex(s[1]) for s in seg]))
        at += 1 + n
    return out


def rebinned_files(outdir, prefix, instruments=INSTRUMENTS):
    """{"<instrument>_<frame>": 8 x 8 block sums} of the output files of one run (oligochromatic, one wavelength)"""
    return {f"{inst}_{name}": rebin(read_fits(os.path.join(outdir, f"{prefix}_{inst}_{name}.fits"))) for inst in instruments for name in FRAMES}


def within_noise(a, n_a, b, n_b, instruments=INSTRUMENTS):
    """The method of test_gpu_parity.test_fits_cube_within_noise_of_the_reference on the blocks of `rebinned_files`: a block's relative
    error is R = sqrt(S2 / S1^2 - 1 / N) from the run's own sums of w and w^2, sigma^2 = (R_a F_a)^2 + (R_b F_b)^2; blocks with at least
    30 contributions in both runs count.  Returns (reduced chi^2, largest |z|, difference of the integrated flux over its sigma, number
    of blocks) over all instruments together."""
    zs, diff, var = [], 0., 0.
    for inst in instruments:
        fa, fb = a[f"{inst}_total"], b[f"{inst}_total"]
        rel = []
        for run, n in ((a, n_a), (b, n_b)):
            s1, s2 = run[f"{inst}_stats1"], run[f"{inst}_stats2"]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel.append(np.sqrt(np.maximum(np.where(s1 > 0, s2 / s1 ** 2 - 1.0 / n, np.inf), 0)))
        good = (a[f"{inst}_stats0"] >= 30) & (b[f"{inst}_stats0"] >= 30)
        with np.errstate(invalid="ignore"):
            sigma = np.sqrt((rel[0] * fa) ** 2 + (rel[1] * fb) ** 2)
        zs.append((fa - fb)[good] / sigma[good])
        # (integrated flux: the noise of the sum from the variances of all blocks with a finite one, as the per-pixel test does)
        finite = np.isfinite(sigma)
        diff += fa.sum() - fb.sum()
        var += np.sum(sigma[finite] ** 2)
    z = np.concatenate(zs)
    return float(np.mean(z ** 2)), float(np.abs(z).max()), float(abs(diff) / np.sqrt(var)), int(z.size)


def meets_stated_criteria(chi2, zmax, flux_sigmas, blocks):
    """reduced chi^2 in [0.85, 1.2], no block beyond 5.5 sigma, the integrated flux within 3 sigma, more than 500 blocks"""
    return blocks > 500 and 0.85 <= chi2 <= 1.2 and zmax < 5.5 and flux_sigmas <= 3
