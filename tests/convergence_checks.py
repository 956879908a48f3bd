"""Scenes and point sets for the checks of the point sampler: SpatialGrid::cellIndex on the host (Simulation.cell_indices) and on the device
(Engine.sample_cells).

The callers of the sampler -- the cut forms of the probes -- ask for the cell at positions that lie ON cell walls as a rule: a cut through
the origin of a grid that is symmetric about it does so with every pixel.  The point sets therefore hold, next to random interior points, the
corners, edge midpoints and face centres of cells (positions shared by up to eight cells), the same of the domain box (inside: the box is
closed), their neighbours one ulp outwards (outside) and points far away."""
import functools
import itertools

import numpy as np

from conftest import ski
from skirt9_amd.host import Simulation, scene_head

GRID_CARTESIAN, GRID_OCTREE, GRID_VORONOI, GRID_BINTREE = 1, 2, 3, 4

# the five forms of the locate kernel: Cartesian (32^3 cells, borders at 0), octree with 10-bit cell indices, octree with 21-bit indices (leaves
# down to level 11 and 12), binary tree, Voronoi
SCENES = ["cfg1", "cfg2small", "cfg2deep", "cfg2bin", "cfg5small"]
BOX_SCENES = ["cfg1", "cfg2small", "cfg2deep", "cfg2bin"]
VORONOI_SCENE = "cfg5small"

# the 26 features of a box in units of its edges from its lower corner: 8 corners, 12 edge midpoints, 6 face centres
FEATURES = np.array([f for f in itertools.product((0., 0.5, 1.), repeat=3) if f.count(0.5) < 3])
assert len(FEATURES) == 26


@functools.lru_cache(maxsize=None)
def simulation(name):
    return Simulation(ski(name + ".ski"), num_packets=1000).setup()


def domain(sim):
    g = scene_head(sim).grid
    return np.array([g.xmin, g.ymin, g.zmin]), np.array([g.xmax, g.ymax, g.zmax])


def cell_boxes(sim):
    """[num_cells][6] the boxes xmin, ymin, zmin, xmax, ymax, zmax of the cells of a Cartesian or tree grid, by cell index"""
    g = scene_head(sim).grid
    if g.kind == GRID_CARTESIAN:
        xv = np.ctypeslib.as_array(g.xv, shape=(g.nx + 1,))
        yv = np.ctypeslib.as_array(g.yv, shape=(g.ny + 1,))
        zv = np.ctypeslib.as_array(g.zv, shape=(g.nz + 1,))
        i, j, k = np.meshgrid(np.arange(g.nx), np.arange(g.ny), np.arange(g.nz), indexing="ij")  # m = k + nz j + nz ny i
        i, j, k = i.ravel(), j.ravel(), k.ravel()
        return np.stack([xv[i], yv[j], zv[k], xv[i + 1], yv[j + 1], zv[k + 1]], axis=1)
    assert g.kind in (GRID_OCTREE, GRID_BINTREE)
    box = np.ctypeslib.as_array(g.node_box, shape=(g.num_nodes, 6))
    cell = np.ctypeslib.as_array(g.node_cell, shape=(g.num_nodes,))
    out = np.empty((g.num_cells, 6))
    out[cell[cell >= 0]] = box[cell >= 0]
    return out


def sites(sim):
    g = scene_head(sim).grid
    assert g.kind == GRID_VORONOI
    return np.ctypeslib.as_array(g.site, shape=(g.num_cells, 3)).copy()


def box_features(boxes):
    """the 26 corners, edge midpoints and face centres of every box [n][6] -> [26 n][3].  A corner has the cell's own wall coordinates, so it
    lies on the walls of every neighbour that shares it; a midpoint lies in the interior of an edge or face (on a wall of a finer neighbour
    where there is one)"""
    lo, hi = boxes[:, None, :3], boxes[:, None, 3:]
    return (lo + FEATURES[None, :, :] * (hi - lo)).reshape(-1, 3)


def random_interior(sim, n, seed):
    lo, hi = domain(sim)
    u = np.random.default_rng(seed).random((n, 3))
    u = np.clip(u, 1e-9, 1. - 1e-9)
    return lo + (hi - lo) * u


def cell_feature_points(sim, max_cells=200, seed=3):
    """the features of up to max_cells cells: half of them drawn at random, half the smallest cells of the grid (the deepest leaves of a tree)"""
    boxes = cell_boxes(sim)
    n = len(boxes)
    if n > max_cells:
        volume = np.prod(boxes[:, 3:] - boxes[:, :3], axis=1)
        smallest = np.argsort(volume, kind="stable")[:max_cells // 2]
        drawn = np.random.default_rng(seed).choice(n, size=max_cells - len(smallest), replace=False)
        boxes = boxes[np.concatenate([smallest, drawn])]
    return box_features(boxes)


def strictly_inside(sim, points):
    lo, hi = domain(sim)
    return np.all((points > lo) & (points < hi), axis=1)


def boundary_points(sim):
    """(inside, outside): the 26 features of the domain box (the box is closed: each has a cell), and each of them moved one ulp outwards on
    every axis on which it lies on the boundary, one axis at a time, plus a few points far away (no cell)"""
    lo, hi = domain(sim)
    inside = box_features(np.concatenate([lo, hi])[None, :])
    outside = []
    for p in inside:
        for a in range(3):
            if p[a] == lo[a] or p[a] == hi[a]:
                q = p.copy()
                q[a] = np.nextafter(p[a], -np.inf if p[a] == lo[a] else np.inf)
                outside.append(q)
    centre, size = 0.5 * (lo + hi), hi - lo
    for a in range(3):
        for sign in (-1., 1.):
            q = centre.copy()
            q[a] += sign * 10. * size[a]
            outside.append(q)
    outside.append(centre + 1e6 * size)
    return inside, np.array(outside)


@functools.lru_cache(maxsize=None)
def point_set(name, n=1000):
    """n positions in a fixed mixed order: the domain's boundary points and their outside neighbours, features of cells (box grids) or the
    sites themselves (Voronoi), random interior points for the rest"""
    sim = simulation(name)
    inside, outside = boundary_points(sim)
    if scene_head(sim).grid.kind == GRID_VORONOI:
        special = sites(sim)[:300]
    else:
        special = cell_feature_points(sim, max_cells=20)  # 520 positions on walls, edges and corners of cells
    parts = [inside, outside, special]
    have = sum(len(p) for p in parts)
    assert have < n
    parts.append(random_interior(sim, n - have, seed=5))
    points = np.concatenate(parts)
    return np.ascontiguousarray(points[np.random.default_rng(17).permutation(n)])


# ---- ConvergenceCutsProbe: scenes, the reference's recorded cuts (tests/golden/make_golden_convergence.py) and the comparison with them

PROBE_NAME = "cnv"
# scene -> (MediumSystem::dimension as the reference's file names show it, material types present): a uniform box on a Cartesian grid with
# borders at 0 (GenGeometry: 3); a Plummer sphere on an octree with leaves of level 11 and 12 (SpheGeometry: 1); a torus of dust next to
# electrons, probeAfter Run (2); an exponential disk on a binary tree (2); geometries offset in x and y (3); imported particles (3); an
# exponential disk on a Voronoi grid (2)
CUT_SCENES = {"cfg1cuts": (3, ("dust",)), "cfg2deepcuts": (1, ("dust",)), "cfg2eleccuts": (2, ("dust", "elec")), "cfg2bincuts": (2, ("dust",)),
              "cfg3offcuts": (3, ("dust",)), "cfg4smallcuts": (3, ("dust",)), "cfg5smallcuts": (2, ("dust",))}
TRUE_CUTS_ONLY = ("cfg5smallcuts",)  # (the Voronoi tessellation is the host layer's own: its cells are not the reference's)
RUN_SCENES = ("cfg2eleccuts",)       # probeAfter="Run"


# scenes with both probes, as the ski-file wizard proposes them; the info file <scene>_inf_convergence.dat of each is a fixture as the
# reference writes it.  cfg1conv: oligochromatic at 0.55 micron with the probe at 2 micron, outside the source and instrument range; cfg2elecconv:
# dust next to electrons, probeAfter Run; cfg3offconv: panchromatic; cfg4smallconv: imported particles (Snapshot::SigmaX/Y/Z)
INFO_PROBE_NAME = "inf"
INFO_SCENES = {"cfg1conv": "cfg1cuts", "cfg2deepconv": "cfg2deepcuts", "cfg2elecconv": "cfg2eleccuts", "cfg2binconv": "cfg2bincuts",
               "cfg3offconv": "cfg3offcuts", "cfg4smallconv": "cfg4smallcuts"}  # -> the cut scene with the same media and grid
INFO_RUN_SCENES = ("cfg2elecconv",)


def info_file(name):
    return f"{name}_{INFO_PROBE_NAME}_convergence.dat"


def assert_info_equals_golden(name, outdir):
    import os

    from conftest import golden
    want = open(golden(info_file(name)), "rb").read()
    got = open(os.path.join(outdir, info_file(name)), "rb").read()
    if got != want:
        a, b = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(f"{info_file(name)} differs from the reference's at line {first + 1}: {a[first:first + 1]} for {b[first:first + 1]}")


def cut_files(name, scene=None):
    """the files a ConvergenceCutsProbe writes for scene `name`, sorted: xy always, xz from dimension 2, yz for dimension 3 (scene: the entry of
    CUT_SCENES with the same media, for a scene that is not in that table itself)"""
    dimension, types = CUT_SCENES[scene or name]
    planes = ["xy", "xz", "yz"][:dimension]
    return sorted(f"{name}_{PROBE_NAME}_{t}_{kind}_{plane}.fits" for t in types for kind in ("t", "g") for plane in planes)


def _blank_date(data):
    """the bytes of a plain FITS image with the DATE card (card 10: no NAXIS3 card) blanked"""
    data = bytearray(data)
    assert data[800:808] == b"DATE    ", bytes(data[800:808])
    data[800:880] = b" " * 80
    return bytes(data)


def cut_digest(data):
    import hashlib
    return hashlib.sha256(_blank_date(data)).digest()


def cut_pixels(data):
    """the image [ny][nx] of a plain FITS file (BITPIX -32, one header block)"""
    header = data[:2880].decode("ascii")
    cards = {header[i:i + 8].strip(): header[i + 10:i + 80].split("/")[0].strip() for i in range(0, 2880, 80)}
    assert cards["BITPIX"] == "-32" and cards["NAXIS"] == "2" and "END" in cards
    nx, ny = int(cards["NAXIS1"]), int(cards["NAXIS2"])
    return np.frombuffer(data, dtype=">f4", count=nx * ny, offset=2880).reshape(ny, nx)


def assert_cuts_equal_golden(name, outdir):
    """every recorded cut of scene `name` was written into outdir with the reference's bytes (apart from the DATE card); on a mismatch the
    decimated pixels say where the first difference lies"""
    import os

    from conftest import golden
    recorded = np.load(golden(name + "_cuts.npz"))
    files = sorted(k[len("digest/"):] for k in recorded.files if k.startswith("digest/"))
    expected = cut_files(name)
    assert files == ([f for f in expected if "_t_" in f] if name in TRUE_CUTS_ONLY else expected), (name, files)
    for f in files:
        data = open(os.path.join(outdir, f), "rb").read()
        if cut_digest(data) == recorded["digest/" + f].tobytes():
            continue
        got, want = cut_pixels(data)[::16, ::16].astype(np.float64), recorded["pixels/" + f]
        bad = np.argwhere(got != want)
        where = (f"first differing decimated pixel (row, column) = {(16 * bad[0]).tolist()}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}, "
                 f"{len(bad)} of {want.size} differ" if len(bad) else "the decimated pixels agree: the difference lies between them or in the header")
        raise AssertionError(f"{f} differs from the reference's file; {where}")
    return files


def assert_cuts_of(name, scene, outdir):
    """the cut files of `name`, a scene with the media and grid of the cut scene `scene` under another prefix, against the digests recorded
    for `scene` (a cut file does not hold the prefix)"""
    import os

    from conftest import golden
    recorded = np.load(golden(scene + "_cuts.npz"))
    for f in cut_files(name, scene):
        data = open(os.path.join(outdir, f), "rb").read()
        assert cut_digest(data) == recorded["digest/" + f.replace(name + "_", scene + "_", 1)].tobytes(), f


def brute_force_nearest(site, points):
    """(index of the nearest site, True where the two smallest squared distances differ by more than 1e-12 relative) per point"""
    nearest = np.empty(len(points), dtype=np.int64)
    clear = np.empty(len(points), dtype=bool)
    for first in range(0, len(points), 256):
        p = points[first:first + 256]
        d2 = ((p[:, None, :] - site[None, :, :]) ** 2).sum(axis=2)
        order = np.argsort(d2, axis=1)[:, :2]
        rows = np.arange(len(p))
        a, b = d2[rows, order[:, 0]], d2[rows, order[:, 1]]
        nearest[first:first + 256] = order[:, 0]
        clear[first:first + 256] = (b - a) > 1e-12 * b
    return nearest, clear
