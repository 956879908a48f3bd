"""Host layer, PolicyTreeSpatialGrid with treeType BinTree (BinTreeNode.cpp): the tree that the host builds against the cell table and the
ray dumps of the UNMODIFIED reference (tests/golden/make_golden_bintree.py).  No GPU."""
import functools

import numpy as np
import pytest

import bintree_checks as B
from conftest import golden, ski
from skirt9_amd.host import SceneFile, SceneHead, Simulation, scene_head

SCENES = {"cfg2bin": (7494, 22), "cfg2bindeep": (906, 36)}   # cells of the reference's table, maxLevel of the ski file


@functools.lru_cache(maxsize=None)
def _scene(name):
    sim = Simulation(ski(name + ".ski"), num_packets=1000).setup()
    return sim, B.Tree(sim)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_cell_table_bit_exact(name):
    """count, every box (as the centre and the volume the reference dumps of it) and every density equal the reference's, bit for bit;
    the leaves are boxes of all three aspect shapes, and the node arrays describe a binary tree that splits along level % 3"""
    sim, tree = _scene(name)
    cells, max_level = SCENES[name]
    gold = np.load(golden(name + "_cells.npz"))
    assert len(gold["density"]) == cells
    head = scene_head(sim)
    assert head.grid.kind == 4 and head.abi_version == 9
    assert tree.num_cells == cells
    leaf = tree.first_array < 0
    assert leaf.sum() == cells and tree.num_nodes == 2 * cells - 1
    order = np.argsort(tree.cell_array[leaf])
    assert np.array_equal(tree.cell_array[leaf][order], np.arange(cells))
    box = tree.box_array[leaf][order]
    centre = np.stack([(box[:, a] + box[:, 3 + a]) / 2 for a in range(3)], axis=1)      # Box::center
    volume = (box[:, 3] - box[:, 0]) * (box[:, 4] - box[:, 1]) * (box[:, 5] - box[:, 2])  # Box::volume
    assert np.array_equal(centre.view(np.uint64), gold["centre"].view(np.uint64))
    assert np.array_equal(volume.view(np.uint64), gold["volume"].view(np.uint64))
    dens = np.ctypeslib.as_array(head.medium.number_density, shape=(cells,))
    assert np.array_equal(dens.view(np.uint64), gold["density"].view(np.uint64))
    # structure: two consecutive children, one level down, split at the parent's centre along level % 3
    internal = np.nonzero(~leaf)[0]
    for a in range(3):
        ids = internal[tree.level_array[internal] % 3 == a]
        c0, c1 = tree.first_array[ids], tree.first_array[ids] + 1
        assert np.array_equal(tree.level_array[c0], tree.level_array[ids] + 1) and np.array_equal(tree.level_array[c1], tree.level_array[ids] + 1)
        mid = (tree.box_array[ids, a] + tree.box_array[ids, 3 + a]) / 2
        assert np.array_equal(tree.box_array[c0, 3 + a], mid) and np.array_equal(tree.box_array[c1, a], mid)
        for b in range(3):
            if b != a:
                for c in (c0, c1):
                    assert np.array_equal(tree.box_array[c, b], tree.box_array[ids, b]) and np.array_equal(tree.box_array[c, 3 + b], tree.box_array[ids, 3 + b])
    levels = tree.level_array[leaf]
    assert levels.max() <= max_level and set(np.unique(levels % 3)) == {0, 1, 2}


def _check_rays(name, tree, num_children, child):
    rays = B.read_rays(golden(name + "_rays.txt"))
    dump = B.read_ray_dump(golden(name + "_rays_ref.txt"))
    assert len(rays) == len(dump)
    visited = set()
    for (r, _), (k, m_ref, ds_ref) in zip(rays, dump):
        seg = B.trace(tree, r, k, num_children, child)
        assert [s[0] for s in seg] == m_ref
        assert [s[1].hex() for s in seg] == [d.hex() for d in ds_ref]
        visited.update(m_ref)
    return visited


def test_literal_tracer_reproduces_the_octree_dump():
    """the restatement of TreeSpatialGrid::MySegmentGenerator::next is validated where the fixture is older than this grid: cfg2small"""
    sim = Simulation(ski("cfg2small.ski"), num_packets=1000).setup()
    tree = B.Tree(sim)
    assert tree.kind == 2
    assert len(_check_rays("cfg2small", tree, 8, B.octree_child)) > 100


@pytest.mark.parametrize("name", sorted(SCENES))
def test_literal_tracer_reproduces_the_reference_rays(name):
    """(m, ds) of the 48 fixed rays bit for bit: the neighbour lists and their order, which the cell table does not pin"""
    _, tree = _scene(name)
    rays = B.read_rays(golden(name + "_rays.txt"))
    assert len(rays) == 48
    visited = _check_rays(name, tree, 2, B.bintree_child)
    # (the rays pass cells of the finest level the tree has)
    finest = int(tree.level_array.max())
    cells_at_finest = set(tree.cell_array[(tree.first_array < 0) & (tree.level_array == finest)].tolist())
    assert visited & cells_at_finest


def test_neighbour_lists_are_symmetric_and_hold_leaves_only():
    _, tree = _scene("cfg2bin")
    comp = [1, 0, 3, 2, 5, 4]
    for i in np.nonzero(tree.first_array < 0)[0][:3000].tolist():
        for w in range(6):
            for q in tree.list[tree.start[6 * i + w]:tree.start[6 * i + w + 1]]:
                assert tree.first[q] < 0
                assert i in tree.list[tree.start[6 * q + comp[w]]:tree.start[6 * q + comp[w] + 1]]


def test_scene_file_round_trip(tmp_path):
    sim, tree = _scene("cfg2bin")
    path = tmp_path / "cfg2bin.scene"
    sim.save_scene(str(path))
    loaded = SceneFile(str(path))
    g = SceneHead.from_address(loaded.scene).grid
    n = g.num_nodes
    assert (g.kind, n, g.num_cells, g.eps) == (4, tree.num_nodes, tree.num_cells, tree.eps)
    assert (g.xmin, g.ymin, g.zmin, g.xmax, g.ymax, g.zmax) == tree.extent
    assert np.array_equal(np.ctypeslib.as_array(g.node_box, shape=(n, 6)).view(np.uint64), tree.box_array.view(np.uint64))
    assert np.array_equal(np.ctypeslib.as_array(g.node_level, shape=(n,)), tree.level_array)
    assert np.array_equal(np.ctypeslib.as_array(g.node_first_child, shape=(n,)), tree.first_array)
    assert np.array_equal(np.ctypeslib.as_array(g.node_cell, shape=(n,)), tree.cell_array)
    assert np.array_equal(np.ctypeslib.as_array(g.nbr_start, shape=(6 * n + 1,)), tree.start_array)
    assert np.array_equal(np.ctypeslib.as_array(g.nbr_list, shape=(len(tree.list),)), tree.list_array)
    live = scene_head(sim).medium
    dens = np.ctypeslib.as_array(SceneHead.from_address(loaded.scene).medium.number_density, shape=(tree.num_cells,))
    assert np.array_equal(dens.view(np.uint64), np.ctypeslib.as_array(live.number_density, shape=(tree.num_cells,)).view(np.uint64))
    assert loaded.frame_size == sim.frame_size and loaded.seed == sim.seed
    loaded.close()


def test_other_tree_types_are_refused_by_name(tmp_path):
    text = open(ski("cfg2bin.ski")).read()
    assert 'treeType="BinTree"' in text
    p = tmp_path / "bad.ski"
    p.write_text(text.replace('treeType="BinTree"', 'treeType="HexTree"'))
    with pytest.raises(RuntimeError, match="treeType HexTree"):
        Simulation(str(p)).setup()


def test_octree_is_unchanged_by_the_attribute(tmp_path):
    """treeType="OctTree" written out and the attribute left away give the same tree"""
    text = open(ski("cfg2deep.ski")).read()
    p = tmp_path / "default.ski"
    p.write_text(text.replace(' treeType="OctTree"', ""))
    a = B.Tree(Simulation(ski("cfg2deep.ski"), num_packets=1000).setup())
    b = B.Tree(Simulation(str(p), num_packets=1000).setup())
    assert a.kind == b.kind == 2 and a.num_nodes == b.num_nodes == 2649
    assert np.array_equal(a.box_array.view(np.uint64), b.box_array.view(np.uint64)) and np.array_equal(a.list_array, b.list_array)

