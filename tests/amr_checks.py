"""A pure-Python restatement of the adaptive mesh import (AdaptiveMeshSnapshot.cpp:29-64,108-148, Box.hpp:163-176, TextInFile.cpp:478-523), the
yardstick of the host layer's snapshot (skirt9_amd/host/adaptive_mesh.cpp) and of the device sampler (pmc_sampler_create_mesh), plus synthetic
meshes and the point sets the checks use.

Python floats are IEEE doubles and `a + d * (b - a) / n` evaluates in the reference's order (the product, the quotient, the sum), so tables and
densities are compared bit for bit.  A mesh is a dict of numpy arrays as Simulation.adaptive_mesh returns it: node_box [nodes][6], node_dims
[nodes][3] (0, 0, 0: leaf), node_link [nodes] (id of child 0 | cell index), cell_density [cells]; node 0 is the root, a parent comes before
its children, the children of a node are consecutive ids in the order k, j, i (i fastest)."""
import itertools
import re

import numpy as np

PC = 3.08567758e16       # skirt9_amd/host/units.hpp
MSUN = 1.9891e30
CANNOT_LOCATE = "Can't locate the appropriate child node"

# the extents of the fixture meshes in pc as their ski files configure them (tools/make_amr.py PRESETS)
DISK_EXTENT_PC = (-19000., -16500., -3700., 17000., 18300., 3100.)
SYM_EXTENT_PC = (-16000., -16000., -4000., 16000., 16000., 4000.)


class LocateError(RuntimeError):
    pass


def frac_pos(lo, hi, d, n):
    """Box::fracPos(int...) (Box.hpp:163-167) for one axis"""
    return lo + d * (hi - lo) / n


def child_boxes(box, dims):
    """the boxes of the children of a node in the order k, j, i (AdaptiveMeshSnapshot.cpp:39-46)"""
    nx, ny, nz = dims
    return [(frac_pos(box[0], box[3], i, nx), frac_pos(box[1], box[4], j, ny), frac_pos(box[2], box[5], k, nz),
             frac_pos(box[0], box[3], i + 1, nx), frac_pos(box[1], box[4], j + 1, ny), frac_pos(box[2], box[5], k + 1, nz))
            for k in range(nz) for j in range(ny) for i in range(nx)]


class MeshBuilder:
    """the flattened tables, filled in the order of the file: the children of a node get their ids when the node is subdivided"""

    def __init__(self, extent):
        self.box, self.dims, self.link, self.rows = [tuple(extent)], [(0, 0, 0)], [-1], []

    def subdivide(self, node, dims):
        first = len(self.box)
        self.dims[node], self.link[node] = tuple(dims), first
        for b in child_boxes(self.box[node], dims):
            self.box.append(b)
            self.dims.append((0, 0, 0))
            self.link.append(-1)
        return range(first, first + dims[0] * dims[1] * dims[2])

    def leaf(self, node, row):
        self.link[node] = len(self.rows)
        self.rows.append(row)

    def tables(self, density):
        return {"node_box": np.array(self.box, dtype=np.float64).reshape(-1, 6), "node_dims": np.array(self.dims, dtype=np.int32).reshape(-1, 3),
                "node_link": np.array(self.link, dtype=np.int32), "cell_density": np.asarray(density, dtype=np.float64)}


HEADER = re.compile(r"#\s*column\s*(\d*)\s*:\s*([^()]*)\(\s*([a-zA-Z0-9/]*)\s*\)\s*", re.I)


def read_mesh_file(path, extent):
    """(builder, units): the tree of an adaptive mesh file over `extent` with the raw values of every leaf row, and the units of the
    "# column N: ... (unit)" header lines (empty without a header).  '#' lines and blank lines are skipped anywhere; a line that starts with
    '!' holds nx ny nz of a nonleaf node; any other line is the row of a leaf.  Raises ValueError with the reference's sentences."""
    lines, units = [], []
    for line in open(path):
        text = line.strip()
        if not text:
            continue
        if text.startswith("#"):
            m = HEADER.fullmatch(text)
            if m and not lines:
                units.append(m.group(3))
            continue
        lines.append(text)
    lines.reverse()  # (a stack: pop() gives the next line)
    builder = MeshBuilder(extent)
    pending = [0]
    while pending:
        node = pending.pop()
        if lines and lines[-1].startswith("!"):
            words = lines.pop()[1:].split()
            try:
                dims = [int(w) for w in words[:3]]
                assert len(dims) == 3
            except (ValueError, AssertionError):
                raise ValueError("Nonleaf subdivision specifiers are missing or not formatted as integers")
            pending.extend(reversed(builder.subdivide(node, dims)))
        else:
            if not lines:
                raise ValueError("Reached end of file in adaptive mesh data before all nodes were read")
            builder.leaf(node, [float(w) for w in lines.pop().split()])
    if lines:
        raise ValueError("Superfluous lines in adaptive mesh data after all nodes were read")
    return builder, units


def cell_volumes(mesh):
    box, leaf = mesh["node_box"], mesh["node_dims"][:, 0] == 0
    out = np.empty(len(mesh["cell_density"]))
    out[mesh["node_link"][leaf]] = [(b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b in box[leaf].tolist()]
    return out


def leaf_boxes(mesh):
    """[cells][6] the boxes of the leaves by cell index"""
    leaf = mesh["node_dims"][:, 0] == 0
    out = np.empty((len(mesh["cell_density"]), 6))
    out[mesh["node_link"][leaf]] = mesh["node_box"][leaf]
    return out


def leaf_levels(mesh):
    """[cells] the level of every leaf (root 0)"""
    dims, link = mesh["node_dims"], mesh["node_link"]
    level = np.zeros(len(link), dtype=np.int64)
    for n in range(len(link)):
        if dims[n, 0]:
            level[link[n]:link[n] + int(np.prod(dims[n]))] = level[n] + 1
    leaf = dims[:, 0] == 0
    out = np.empty(len(mesh["cell_density"]), dtype=np.int64)
    out[link[leaf]] = level[leaf]
    return out


def _holds(b, x, y, z):
    return b[0] <= x <= b[3] and b[1] <= y <= b[4] and b[2] <= z <= b[5]  # (False for a NaN)


def _estimate(n, x, lo, hi):
    """Box::cellIndices (Box.hpp:171-176) for one axis: the product first, then the quotient"""
    return max(0, min(n - 1, int(n * (x - lo) / (hi - lo))))


class Descent:
    """AdaptiveMeshSnapshot::cellIndex / density(Position) on the tables (plain Python lists: the descent is a scalar loop)"""

    def __init__(self, mesh):
        self.box = mesh["node_box"].tolist()
        self.dims = mesh["node_dims"].tolist()
        self.link = mesh["node_link"].tolist()
        self.rho = mesh["cell_density"].tolist()

    def cell(self, p):
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        if not _holds(self.box[0], x, y, z):
            return -1
        node = 0
        while self.dims[node][0]:
            nx, ny, nz = self.dims[node]
            b = self.box[node]
            i, j, k = _estimate(nx, x, b[0], b[3]), _estimate(ny, y, b[1], b[4]), _estimate(nz, z, b[2], b[5])
            child = self.link[node] + (k * ny + j) * nx + i
            c = self.box[child]
            if not _holds(c, x, y, z):
                i += -1 if x < c[0] else 1 if x > c[3] else 0
                j += -1 if y < c[1] else 1 if y > c[4] else 0
                k += -1 if z < c[2] else 1 if z > c[5] else 0
                if not (0 <= i < nx and 0 <= j < ny and 0 <= k < nz):
                    raise LocateError(CANNOT_LOCATE)
                child = self.link[node] + (k * ny + j) * nx + i
                if not _holds(self.box[child], x, y, z):
                    raise LocateError(CANNOT_LOCATE)
            node = child
        return self.link[node]

    def cells(self, points):
        return np.array([self.cell(p) for p in np.asarray(points, dtype=np.float64).reshape(-1, 3)], dtype=np.int64)

    def densities(self, points):
        return np.array([self.rho[m] if m >= 0 else 0. for m in self.cells(points)], dtype=np.float64)


def cannot_locate(mesh, points):
    """the indices of the points at which the restatement raises the reference's error"""
    descent, bad = Descent(mesh), []
    for index, p in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3)):
        try:
            descent.cell(p)
        except LocateError:
            bad.append(index)
    return bad


# ---------------------------------------------------------------- synthetic meshes: every leaf carries a different density, so that an equal
# density means the same leaf.  Their extents are dyadic, where fracPos is exact for the 2x2x2 subdivisions.

def _finish(builder):
    cells = 0
    for n in range(len(builder.box)):
        if builder.dims[n][0] == 0:
            builder.link[n] = cells
            cells += 1
    return builder.tables(1. + np.arange(cells, dtype=np.float64) / 1024.)


def single_leaf():
    return _finish(MeshBuilder((-1., -1., -1., 1., 1., 1.)))


def two_cubed():
    builder = MeshBuilder((-1., -2., -4., 1., 2., 4.))
    builder.subdivide(0, (2, 2, 2))
    return _finish(builder)


def corner_chain(levels=30):
    """refined 2x2x2 `levels` times into the lower corner: leaves at every level from 1 to `levels`"""
    builder = MeshBuilder((0., 0., 0., 1., 2., 4.))
    node = 0
    for _ in range(levels):
        node = builder.subdivide(node, (2, 2, 2))[0]
    return _finish(builder)


def nest_3x2x1():
    """3x2x1 inside 3x2x1 inside 3x2x1: dimensions that differ per axis, and a dimension of 1"""
    builder = MeshBuilder((0., 0., 0., 3., 2., 1.))
    first = builder.subdivide(0, (3, 2, 1))
    second = builder.subdivide(first[4], (3, 2, 1))
    builder.subdivide(second[1], (3, 2, 1))
    builder.subdivide(first[0], (1, 1, 2))
    return _finish(builder)


SYNTHETIC = {"single": single_leaf, "two_cubed": two_cubed, "chain": corner_chain, "nest": nest_3x2x1}
DYADIC = ("single", "two_cubed", "chain")  # (where points on the outer upper walls are taken: fracPos is exact there)


# ---------------------------------------------------------------- point sets

# the 26 features of a box in units of its edges from its lower corner: 8 corners, 12 edge midpoints, 6 face centres
FEATURES = np.array([f for f in itertools.product((0., 0.5, 1.), repeat=3) if f.count(0.5) < 3])


def box_features(boxes):
    lo, hi = boxes[:, None, :3], boxes[:, None, 3:]
    return (lo + FEATURES[None, :, :] * (hi - lo)).reshape(-1, 3)


def one_ulp_either_side(points):
    """every point moved one ulp down and one ulp up on every axis, one axis at a time"""
    out = []
    for a in range(3):
        for toward in (-np.inf, np.inf):
            q = points.copy()
            q[:, a] = np.nextafter(q[:, a], toward)
            out.append(q)
    return np.concatenate(out)


def point_sets(mesh, upper_walls, seed=11, max_leaves=200, num_random=2000):
    """dict of point sets [n][3] for a mesh: random interior points; every leaf centre; the corners, edge midpoints and face centres of up to
    max_leaves leaves -- the deepest first, the rest drawn --; the same one ulp either side of those walls; the domain's corners; points one
    ulp outside the domain and far away; NaN and inf.  Without upper_walls the points that lie on the outer upper walls of the domain (or
    beyond them by the ulp) are left to the dyadic meshes, where the last child's upper wall is its parent's exactly"""
    rng = np.random.default_rng(seed)
    root = mesh["node_box"][0]
    lo, hi = root[:3], root[3:]
    boxes = leaf_boxes(mesh)
    level = leaf_levels(mesh)
    chosen = np.argsort(-level, kind="stable")[:max_leaves // 2]
    rest = np.setdiff1d(np.arange(len(boxes)), chosen)
    if len(rest):
        chosen = np.concatenate([chosen, rng.choice(rest, size=min(len(rest), max_leaves - len(chosen)), replace=False)])
    walls = box_features(boxes[chosen])
    near = one_ulp_either_side(walls)
    corners = box_features(root[None, :])
    if not upper_walls:
        keep = lambda p: p[np.all(p < hi, axis=1)]  # noqa: E731
        walls, near, corners = keep(walls), keep(near), keep(corners)
    outside = []
    for p in box_features(root[None, :]):
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
    odd = np.array([[np.nan, centre[1], centre[2]], [centre[0], np.nan, centre[2]], [centre[0], centre[1], np.nan], [np.nan, np.nan, np.nan],
                    [np.inf, centre[1], centre[2]], [centre[0], -np.inf, centre[2]], [centre[0], centre[1], np.inf], [-np.inf, np.inf, np.nan]])
    u = np.clip(rng.random((num_random, 3)), 1e-9, 1. - 1e-9)
    return {"random": lo + (hi - lo) * u, "centres": 0.5 * (boxes[:, :3] + boxes[:, 3:]), "walls": walls, "near_walls": near, "corners": corners,
            "outside": np.array(outside), "odd": odd}


def all_points(mesh, upper_walls, **kwargs):
    return np.ascontiguousarray(np.concatenate(list(point_sets(mesh, upper_walls, **kwargs).values())))


# ---------------------------------------------------------------- files and scenes of synthetic meshes

def write_mesh_file(mesh, path, header=("# column 1: mass density (kg/m3)",), rows=None):
    """the tree of `mesh` as an adaptive mesh file, depth first; a leaf's row is its density (%r: the shortest text that reads back exactly) or
    rows[cell index].  The cells of the file are numbered in file order, which need not be the numbering of `mesh`"""
    dims, link, rho = mesh["node_dims"].tolist(), mesh["node_link"].tolist(), mesh["cell_density"].tolist()
    lines, stack = list(header), [0]
    while stack:
        n = stack.pop()
        if dims[n][0]:
            lines.append("! %d %d %d" % tuple(dims[n]))
            stack.extend(range(link[n] + dims[n][0] * dims[n][1] * dims[n][2] - 1, link[n] - 1, -1))
        else:
            lines.append(rows[link[n]] if rows is not None else repr(rho[link[n]]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def mesh_ski(folder, name, mesh_path, extent_m=None, replace=()):
    """tests/ski/cfg6amr.ski as <folder>/<name>.ski with the mesh file (an absolute path) and, unless None, the extent (metres) replaced, then
    the (old, new) pairs of `replace` applied to the text; returns the path"""
    import os

    from conftest import ski
    text = open(ski("cfg6amr.ski")).read()
    assert 'filename="cfg6amr_mesh.txt"' in text
    text = text.replace('filename="cfg6amr_mesh.txt"', 'filename="%s"' % mesh_path)
    for key, value in zip(("minX", "minY", "minZ", "maxX", "maxY", "maxZ"), extent_m or ()):
        text, count = re.subn(r'(<AdaptiveMeshMedium[^>]*? %s=")[^"]*(")' % key, lambda m: m.group(1) + repr(float(value)) + " m" + m.group(2), text)
        assert count == 1, key
    for old, new in replace:
        assert old in text, old
        text = text.replace(old, new)
    path = os.path.join(str(folder), name + ".ski")
    with open(path, "w") as fh:
        fh.write(text)
    return path


# ---------------------------------------------------------------- tables that pmc_sampler_create_mesh must refuse (PMC_ERR_INVALID) before any
# device call: on a machine without a GPU the refusal is the same

def malformed_tables():
    """[(what, tables, words of the message)]: the 2x2x2 mesh (nodes 0..8, cells 0..7) with one defect each"""
    def variant(node, dims=None, link=None):
        mesh = {key: value.copy() for key, value in two_cubed().items()}
        if dims is not None:
            mesh["node_dims"][node] = dims
        if link is not None:
            mesh["node_link"][node] = link
        return mesh
    return [("twelve children of the root, eight in the table", variant(0, dims=(2, 2, 3)), "child range outside the table"),
            ("children that start at the last node", variant(0, link=8), "child range outside the table"),
            ("a node that is its own child", variant(1, dims=(1, 1, 1), link=1), "child id not above its parent's"),
            ("a child below its parent", variant(5, dims=(1, 1, 1), link=2), "child id not above its parent's"),
            ("a dimension of zero next to others", variant(0, dims=(2, 0, 2)), "dimension below 1"),
            ("a negative dimension", variant(0, dims=(-1, 2, 2)), "dimension below 1"),
            ("nx * ny beyond 2^31", variant(0, dims=(65536, 65536, 1)), "product of the dimensions overflows"),
            ("nx * ny * nz beyond 2^31", variant(0, dims=(2048, 2048, 2048)), "product of the dimensions overflows"),
            ("a leaf link at the number of cells", variant(3, link=8), "leaf link outside the cells"),
            ("a negative leaf link", variant(8, link=-1), "leaf link outside the cells")]
