// pmc_tables.h -- the grid tables of a scene: the reference-shaped tables of pmc_grid become the device layout of pmc_device.h.  Plain C++17,
// no HIP: every builder is a function from pmc_grid (and the densities of component 0) to host vectors, and an upload function per grid kind
// hands them to a TableSink one by one -- in pmc_create the context, which copies them to the device; in tools/scene_build_check.cpp, under
// the sanitizers, a sink that hashes them.
//
// Octree: verify that every node box is consistent with one per-axis dyadic coordinate table (true for any tree built by recursive midpoint
// subdivision, OctTreeNode.cpp:22-33), build that table from the reference's own doubles, and replace the per-wall neighbour lists by links
// (per wall: the neighbour leaf covering it, or the internal node below which finer neighbours are found).  The reference lists themselves
// are uploaded too, re-indexed by cell, for the exact fallback path.
// Binary tree: self-contained cell records with one link per wall, and the table of binary splits (BinTreeBuild).
// Voronoi: cell records, neighbour entries, cone masks, and the tables of runs that the walk kernels read (per direction cone, per observer).
#ifndef PMC_TABLES_H
#define PMC_TABLES_H

#include "pmc_device.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

// error text of the calling thread (pmc_last_error); defined in pmc_api.hip
void pmcSetError(const std::string& message);
namespace
{
    inline int fail(int code, const std::string& message)
    {
        pmcSetError(message);
        return code;
    }
}

// where the tables of a scene go: pmc_ctx puts them into device memory
struct TableSink
{
    virtual int uploadBytes(const void* host, size_t elementBytes, size_t count, const void** out) = 0;
    virtual int allocateBytes(size_t bytes, void** out, bool zero) = 0;
    // free memory where the tables go: the tables that only accelerate a walk are left out where it is short
    virtual size_t freeBytes() = 0;

    template<typename T> int upload(const T* host, size_t count, const T** out)
    {
        *out = nullptr;
        if (!count) return PMC_OK;
        const void* d = nullptr;
        const int rc = uploadBytes(host, sizeof(T), count, &d);
        *out = static_cast<const T*>(d);
        return rc;
    }
    template<typename T> int allocate(size_t count, T** out, bool zero)
    {
        *out = nullptr;
        if (!count) return PMC_OK;
        void* d = nullptr;
        const int rc = allocateBytes(count * sizeof(T), &d, zero);
        *out = static_cast<T*>(d);
        return rc;
    }

protected:
    ~TableSink() = default;
};

// the tuning switches (include/pmc_tuning.h) that scene creation reads, read once by pmc_create (pmc_api.hip readSceneSwitches)
struct SceneSwitches
{
    bool treeAsBinTree{false};       // PMC_TREE_AS_BINTREE
    bool noMono{false};              // PMC_NO_MONO
    bool propNoCheckpoints{false};   // PMC_PROP_NO_CHECKPOINTS
    bool voroNoPeelKernel{false}, voroNoDeferredScan{false}, voroNoCull{false}, voroNoPropKernel{false}, voroNoConeTables{false};
    bool voroNoObserverLists{false}, voroConeCullOnly{false};                    // PMC_VORO_*
    uint32_t voroLinkCountMax{PMC_VORO_RUN_COUNT_UNKNOWN - 1u};                   // PMC_VORO_LINK_COUNT_MAX (it can only lower the limit)
    bool cellOrderRef{false};        // PMC_CELL_ORDER=ref
    int cellShuffle{-1};             // PMC_CELL_SHUFFLE (-1: not set)
    int walkBlocksPerCU{0}, peelBlocksPerCU{0};  // PMC_WALK_BLOCKS_PER_CU, PMC_PEEL_BLOCKS_PER_CU (0: not set)
};

namespace
{
    // ---- octree flattening -------------------------------------------------------------------------
    struct TreeBuild
    {
        int lmax{0};
        int tabn{0};
        std::vector<double> table;       // [3][tabn]
        std::vector<LeafRec> leaves;     // by cell index m
        std::vector<CellRec> cells;      // by device cell index: the walk step's hot record
        std::vector<NodeRec> internals;  // by internal index
        std::vector<int32_t> nbrStart, nbrList;
        uint32_t rootLink{0};
        int coarseLevel{0};
        std::vector<uint32_t> coarse;    // [2^Lc]^3 (z, y, x): link of the covering node at level <= Lc
        // device numbering of the cells: dev = perm[m], depth-first order of the tree (the eight leaves of a node whose
        // children are all leaves are consecutive, in child order); cellExt[dev] = m (or -1 for padding); cellSlots =
        // entries per device table
        std::vector<int32_t> perm, cellExt;
        int cellSlots{0};
    };

    // what the tables are built from: the finest level, the fine lower-corner indices of every node (from the topology alone), and per node id
    // its index among the internal nodes (-1: a leaf)
    struct TreeShape
    {
        int maxLevel{0};
        std::vector<int32_t> fx, fy, fz, internalIndex;
        int numInternal{0};
    };

    inline int treeShape(const pmc_grid& g, TreeShape& S)
    {
        const int numNodes = g.num_nodes;
        if (numNodes < 1) return fail(PMC_ERR_INVALID, "octree without nodes");
        for (int id = 0; id < numNodes; ++id) S.maxLevel = std::max(S.maxLevel, g.node_level[id]);
        if (S.maxLevel > PMC_MAX_LEVEL) return fail(PMC_ERR_UNSUPPORTED, "octree deeper than " + std::to_string(PMC_MAX_LEVEL) + " levels");
        S.fx.assign(numNodes, 0), S.fy.assign(numNodes, 0), S.fz.assign(numNodes, 0);
        S.internalIndex.assign(numNodes, -1);
        if (g.node_level[0] != 0) return fail(PMC_ERR_INVALID, "octree root is not at level 0");
        for (int id = 0; id < numNodes; ++id)
        {
            int first = g.node_first_child[id];
            if (first < 0) continue;
            S.internalIndex[id] = S.numInternal++;
            if (first + 8 > numNodes) return fail(PMC_ERR_INVALID, "octree child index out of range");
            int half = 1 << (S.maxLevel - g.node_level[id] - 1);
            for (int l = 0; l < 8; ++l)
            {
                int c = first + l;
                if (g.node_level[c] != g.node_level[id] + 1) return fail(PMC_ERR_INVALID, "octree child level mismatch");
                S.fx[c] = S.fx[id] + ((l & 1) ? half : 0);
                S.fy[c] = S.fy[id] + ((l & 2) ? half : 0);
                S.fz[c] = S.fz[id] + ((l & 4) ? half : 0);
            }
        }
        return PMC_OK;
    }

    // coordinate table from the reference's own box doubles, with consistency check
    inline int treeCoordinateTable(const pmc_grid& g, const TreeShape& S, TreeBuild& T)
    {
        const int maxLevel = S.maxLevel;
        T.lmax = maxLevel;
        T.tabn = (1 << maxLevel) + 1;
        const double unset = std::nan("");
        T.table.assign(3 * size_t(T.tabn), unset);
        auto put = [&](int axis, int index, double value) -> bool {
            double& slot = T.table[size_t(axis) * T.tabn + index];
            if (std::isnan(slot))
            {
                slot = value;
                return true;
            }
            return slot == value;
        };
        for (int id = 0; id < g.num_nodes; ++id)
        {
            const double* b = g.node_box + 6 * size_t(id);
            int size = 1 << (maxLevel - g.node_level[id]);
            bool ok = put(0, S.fx[id], b[0]) && put(0, S.fx[id] + size, b[3]) && put(1, S.fy[id], b[1]) && put(1, S.fy[id] + size, b[4])
                      && put(2, S.fz[id], b[2]) && put(2, S.fz[id] + size, b[5]);
            if (!ok)
                return fail(PMC_ERR_UNSUPPORTED,
                            "octree node boxes are not consistent with a dyadic coordinate table (node " + std::to_string(id) + ")");
        }
        // entries that are no node's wall (inside coarse leaves) get the dyadic midpoints: no decision ever depends on
        // them, but the table becomes strictly monotonic, which the index search of topDown (pmc_walk.inc) relies on
        for (int axis = 0; axis < 3; ++axis)
            for (int size = 1 << maxLevel; size >= 2; size >>= 1)
                for (int lo = 0; lo + size <= (1 << maxLevel); lo += size)
                {
                    double& mid = T.table[size_t(axis) * T.tabn + lo + size / 2];
                    if (std::isnan(mid))
                        mid = (T.table[size_t(axis) * T.tabn + lo] + T.table[size_t(axis) * T.tabn + lo + size]) / 2.;
                }
        return PMC_OK;
    }

    // device numbering of the cells: depth-first order of the tree, children in child order (tuning aids:
    // PMC_CELL_ORDER=ref keeps the caller's numbering -- breadth-first by level in SKIRT; PMC_CELL_SHUFFLE=g scatters
    // groups of 2^g cells of that numbering over the table)
    inline int treeNumbering(const pmc_grid& g, const SceneSwitches& sw, TreeBuild& T)
    {
        const int n = g.num_cells;
        T.perm.assign(n, -1);
        const int gb = sw.cellShuffle;
        if (gb >= 0 && gb <= 16)
        {
            const int groupSize = 1 << gb;
            const int numGroups = (n + groupSize - 1) / groupSize;
            std::vector<int32_t> where(numGroups);
            for (int i = 0; i < numGroups; ++i) where[i] = i;
            uint64_t state = 0x9E3779B97F4A7C15ull;  // fixed: the numbering is a pure function of the scene
            for (int i = numGroups - 1; i > 0; --i)
            {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                const int j = int((state >> 33) % uint64_t(i + 1));
                std::swap(where[i], where[j]);
            }
            T.cellSlots = numGroups * groupSize;
            for (int m = 0; m < n; ++m) T.perm[m] = where[m >> gb] * groupSize + (m & (groupSize - 1));
        }
        else if (sw.cellOrderRef)
        {
            T.cellSlots = n;
            for (int m = 0; m < n; ++m) T.perm[m] = m;
        }
        else
        {
            T.cellSlots = n;
            int next = 0;
            std::vector<int> stack{0};
            while (!stack.empty())
            {
                const int id = stack.back();
                stack.pop_back();
                const int first = g.node_first_child[id];
                if (first < 0)
                {
                    const int m = g.node_cell[id];
                    if (m < 0 || m >= n || T.perm[m] >= 0) return fail(PMC_ERR_INVALID, "octree leaf without a valid cell index");
                    T.perm[m] = next++;
                }
                else
                    for (int l = 7; l >= 0; --l) stack.push_back(first + l);
            }
            if (next != n) return fail(PMC_ERR_INVALID, "octree leaves and cells do not match");
        }
        T.cellExt.assign(T.cellSlots, -1);
        for (int m = 0; m < n; ++m) T.cellExt[T.perm[m]] = m;
        return PMC_OK;
    }

    // box code (pmc_walk.inc decodeBoxWords): the indices of the three lower walls in the coordinate table of their axis + size exponent
    // (e >= 15: the field holds 15 and the low bits of the x index, zero in such a box, hold e - 15)
    inline uint64_t treeBoxCode(const pmc_grid& g, const TreeShape& S, int id)
    {
        const uint64_t e = uint64_t(S.maxLevel - g.node_level[id]);
        uint64_t ix = uint64_t(S.fx[id]);
        const uint64_t iy = uint64_t(S.fy[id]), iz = uint64_t(S.fz[id]);
        if (e >= 15) ix |= e - 15;
        return ix | (iy << 20) | (iz << 40) | (std::min<uint64_t>(e, 15) << 60);
    }
    // link word (pmc_device.h): size exponent | index << PMC_LINK_EXP_BITS | node flag
    inline uint32_t treeLinkOf(const pmc_grid& g, const TreeShape& S, const TreeBuild& T, int id)
    {
        if (id < 0) return PMC_LINK_NONE;
        const uint32_t e = uint32_t(S.maxLevel - g.node_level[id]);
        return g.node_first_child[id] < 0 ? (e | (uint32_t(T.perm[g.node_cell[id]]) << PMC_LINK_EXP_BITS))
                                          : (e | (uint32_t(S.internalIndex[id]) << PMC_LINK_EXP_BITS) | PMC_LINK_NODE);
    }
    // the link of a cell record through a wall: as treeLinkOf, but an internal node whose children are all leaves with
    // consecutive device indices in child order becomes an octet link (the walk picks the child without a load)
    inline uint32_t treeWallLinkOf(const pmc_grid& g, const TreeShape& S, const TreeBuild& T, int id)
    {
        if (id < 0 || g.node_first_child[id] < 0) return treeLinkOf(g, S, T, id);
        const int first = g.node_first_child[id];
        for (int l = 0; l < 8; ++l)
            if (g.node_first_child[first + l] >= 0) return treeLinkOf(g, S, T, id);
        const int base = T.perm[g.node_cell[first]];
        for (int l = 1; l < 8; ++l)
            if (T.perm[g.node_cell[first + l]] != base + l) return treeLinkOf(g, S, T, id);
        return uint32_t(S.maxLevel - g.node_level[id]) | (uint32_t(base) << PMC_LINK_EXP_BITS) | PMC_LINK_OCTET;
    }

    // the child of `node` that holds the fine cell (px, py, pz)
    inline int treeChildAt(const pmc_grid& g, const TreeShape& S, int node, int px, int py, int pz)
    {
        const int half = 1 << (S.maxLevel - g.node_level[node] - 1);
        const int l = ((px - S.fx[node]) >= half ? 1 : 0) + ((py - S.fy[node]) >= half ? 2 : 0) + ((pz - S.fz[node]) >= half ? 4 : 0);
        return g.node_first_child[node] + l;
    }

    // top-down search table (pmc_walk.inc topDown): per cell of the regular grid of level Lc the node of level Lc
    // that covers it, or the coarser leaf
    inline void treeCoarseTable(const pmc_grid& g, const TreeShape& S, TreeBuild& T)
    {
        const int lc = std::min(S.maxLevel, 6);
        T.coarseLevel = lc;
        const int nc = 1 << lc;
        T.coarse.resize(size_t(nc) * nc * nc);
        for (int cz = 0; cz < nc; ++cz)
            for (int cy = 0; cy < nc; ++cy)
                for (int cx = 0; cx < nc; ++cx)
                {
                    const int px = cx << (S.maxLevel - lc), py = cy << (S.maxLevel - lc), pz = cz << (S.maxLevel - lc);
                    int node = 0;
                    while (g.node_first_child[node] >= 0 && g.node_level[node] < lc) node = treeChildAt(g, S, node, px, py, pz);
                    T.coarse[(size_t(cz) * nc + cy) * nc + cx] = treeLinkOf(g, S, T, node);
                }
    }

    // the node at level <= level(id) that covers the region just across `wall` of node id (-1: outside the grid)
    inline int treeCovering(const pmc_grid& g, const TreeShape& S, int id, int wall)
    {
        int axis = wall >> 1, side = wall & 1;
        int size = 1 << (S.maxLevel - g.node_level[id]);
        int px = S.fx[id], py = S.fy[id], pz = S.fz[id];  // a fine cell index inside the neighbour region
        int* pa = axis == 0 ? &px : axis == 1 ? &py : &pz;
        *pa += side ? size : -1;
        int full = 1 << S.maxLevel;
        if (*pa < 0 || *pa >= full) return -1;
        int node = 0;
        while (g.node_first_child[node] >= 0 && g.node_level[node] < g.node_level[id]) node = treeChildAt(g, S, node, px, py, pz);
        return node;
    }

    // the records: internal nodes, and per device cell the cold and the hot record and the reference's neighbour lists in device numbering
    inline int treeRecords(const pmc_grid& g, const TreeShape& S, const double* density, TreeBuild& T)
    {
        const int numNodes = g.num_nodes, numCells = g.num_cells, cellSlots = T.cellSlots;
        T.leaves.assign(cellSlots, LeafRec{});
        T.cells.assign(size_t(cellSlots), CellRec{});
        T.internals.assign(S.numInternal, NodeRec{});
        T.nbrStart.assign(6 * size_t(cellSlots) + 1, 0);
        T.nbrList.clear();
        std::vector<int32_t> nodeOfCell(numCells, -1);
        for (int id = 0; id < numNodes; ++id)
        {
            int m = g.node_cell[id];
            if (g.node_first_child[id] < 0)
            {
                if (m < 0 || m >= numCells) return fail(PMC_ERR_INVALID, "octree leaf without a valid cell index");
                nodeOfCell[m] = id;
            }
            else
            {
                NodeRec& rec = T.internals[S.internalIndex[id]];
                rec.code = treeBoxCode(g, S, id);
                for (int l = 0; l < 8; ++l) rec.child[l] = treeLinkOf(g, S, T, g.node_first_child[id] + l);
            }
        }
        for (int m = 0; m < numCells; ++m)
            if (nodeOfCell[m] < 0) return fail(PMC_ERR_INVALID, "cell without a leaf node");
        for (int dev = 0; dev < cellSlots; ++dev)
        {
            const int m = T.cellExt[dev];
            for (int wall = 0; wall < 6; ++wall) T.nbrStart[6 * size_t(dev) + wall] = (int32_t)T.nbrList.size();
            if (m < 0) continue;  // padding of the last group
            const int id = nodeOfCell[m];
            LeafRec& rec = T.leaves[dev];
            rec.code = treeBoxCode(g, S, id);
            rec.density = density[m];
            CellRec& hot = T.cells[dev];
            hot.density = density[m];
            for (int wall = 0; wall < 6; ++wall)
            {
                // the leaf across the wall (same size or coarser), or the same-size internal node (finer neighbours: the walk
                // picks the child by the index bits of its position), or "outside"
                hot.link[wall] = treeWallLinkOf(g, S, T, treeCovering(g, S, id, wall));
                // the reference's neighbour list of this leaf, in device numbering
                T.nbrStart[6 * size_t(dev) + wall] = (int32_t)T.nbrList.size();
                for (int qq = g.nbr_start[6 * size_t(id) + wall]; qq < g.nbr_start[6 * size_t(id) + wall + 1]; ++qq)
                {
                    int nb = g.nbr_list[qq];
                    if (g.node_first_child[nb] >= 0)
                        return fail(PMC_ERR_INVALID, "neighbour list of a leaf contains a non-leaf node");
                    T.nbrList.push_back(T.perm[g.node_cell[nb]]);
                }
            }
        }
        T.nbrStart[6 * size_t(cellSlots)] = (int32_t)T.nbrList.size();
        return PMC_OK;
    }

    inline int buildTree(const pmc_grid& g, const double* density, const SceneSwitches& sw, TreeBuild& T)
    {
        TreeShape S;
        int rc = PMC_OK;
        if ((rc = treeShape(g, S))) return rc;
        if ((rc = treeCoordinateTable(g, S, T))) return rc;
        if ((rc = treeNumbering(g, sw, T))) return rc;
        T.rootLink = treeLinkOf(g, S, T, 0);
        treeCoarseTable(g, S, T);
        return treeRecords(g, S, density, T);
    }

    // devToCell (here and for the binary tree): device cell index -> the caller's cell index (-1: padding), for the tables of the other stages
    inline int uploadOctreeGrid(const pmc_grid& g, const double* density, const SceneSwitches& sw, TableSink& sink, DevScene& D, std::vector<int32_t>& devToCell)
    {
        int rc = PMC_OK;
        TreeBuild T;
        if ((rc = buildTree(g, density, sw, T))) return rc;
        D.lmax = T.lmax;
        D.root_link = T.rootLink;
        if (size_t(T.cellSlots) > PMC_LINK_MAX_INDEX || T.internals.size() > PMC_LINK_MAX_INDEX)
            return fail(PMC_ERR_UNSUPPORTED, "octree with 2^25 cells or nodes or more (25-bit link index)");
        D.tab_stride_bytes = 8u * uint32_t(T.tabn);
        D.fine_scale[0] = double(1 << T.lmax) / (g.xmax - g.xmin);
        D.fine_scale[1] = double(1 << T.lmax) / (g.ymax - g.ymin);
        D.fine_scale[2] = double(1 << T.lmax) / (g.zmax - g.zmin);
        if ((rc = sink.upload(T.table.data(), T.table.size(), &D.coord_tab))) return rc;
        if ((rc = sink.upload(T.leaves.data(), T.leaves.size(), &D.leaves))) return rc;
        if ((rc = sink.upload(T.cells.data(), T.cells.size(), &D.cell_tab))) return rc;
        if ((rc = sink.upload(T.internals.data(), T.internals.size(), &D.nodes))) return rc;
        D.coarse_level = T.coarseLevel;
        if ((rc = sink.upload(T.coarse.data(), T.coarse.size(), &D.coarse_tab))) return rc;
        if ((rc = sink.upload(T.nbrStart.data(), T.nbrStart.size(), &D.nbr_start))) return rc;
        if ((rc = sink.upload(T.nbrList.data(), T.nbrList.size(), &D.nbr_list))) return rc;
        if ((rc = sink.upload(T.cellExt.data(), T.cellExt.size(), &D.cell_ext))) return rc;
        devToCell = std::move(T.cellExt);
        D.cell_slots = T.cellSlots;
        // (levels 13-20: 0.2 ... 25 MB: not in LDS; the walk reads the six walls of a step from global memory)
        D.tab_in_lds = T.lmax <= 12 ? 1 : 0;
        D.lds_grid_len = D.tab_in_lds ? 3 * T.tabn : 0;
        return rc;
    }

    // ---- binary tree -------------------------------------------------------------------------------
    // Binary tree (PMC_GRID_BINTREE), or -- under the switch PMC_TREE_AS_BINTREE -- an octree whose every node enters the table of binary nodes
    // as its three levels of splits (x, then y, then z, at CHILD_0's upper corner: the doubles and the `<` decisions of OctTreeNode::child,
    // OctTreeNode.cpp:37-42).  Cell records: the node boxes as they come, one link per wall; the reference's neighbour lists re-indexed by
    // cell for the exact fallback path (pmc_device.h BinCellRec, BinNodeRec; pmc_walk_bin.inc).
    struct BinTreeBuild
    {
        std::vector<int32_t> perm, cellExt;  // device numbering of the cells: dev = perm[m], cellExt[dev] = m; depth-first order of the tree
        std::vector<BinNodeRec> nodes;       // 1 (binary tree) or 7 (octree) records per subdivided node
        std::vector<BinCellRec> cells;       // by device cell index
        std::vector<double> density;         // likewise
        std::vector<int32_t> nbrStart, nbrList;
        int32_t rootLink{0};
    };

    // what the records are built from: children per subdivided node (consecutive ids), binary node records per subdivided node, and per node id
    // its index among the subdivided nodes (-1: a leaf)
    struct BinTreeShape
    {
        int fan{2}, perNode{1};
        std::vector<int32_t> internalIndex, nodeOfCell;
        int numInternal{0};
    };

    // device numbering of the cells: depth-first order of the tree, children in child order (siblings are neighbours in the table)
    inline int binTreeNumbering(const pmc_grid& g, BinTreeShape& S, std::vector<int32_t>& perm)
    {
        const int numNodes = g.num_nodes, numCells = g.num_cells;
        perm.assign(numCells, -1);
        S.internalIndex.assign(numNodes, -1);
        S.nodeOfCell.assign(numCells, -1);
        int next = 0;
        size_t visited = 0;
        std::vector<int> stack{0};
        while (!stack.empty())
        {
            const int id = stack.back();
            stack.pop_back();
            if (++visited > size_t(numNodes)) return fail(PMC_ERR_INVALID, "tree child links form no tree");
            const int first = g.node_first_child[id];
            if (first < 0)
            {
                const int m = g.node_cell[id];
                if (m < 0 || m >= numCells || perm[m] >= 0) return fail(PMC_ERR_INVALID, "tree leaf without a valid cell index");
                perm[m] = next++;
                S.nodeOfCell[m] = id;
                continue;
            }
            if (first < 1 || first + S.fan > numNodes) return fail(PMC_ERR_INVALID, "tree child index out of range");
            S.internalIndex[id] = S.numInternal++;
            for (int l = S.fan - 1; l >= 0; --l)
            {
                if (g.node_level[first + l] != g.node_level[id] + 1) return fail(PMC_ERR_INVALID, "tree child level mismatch");
                stack.push_back(first + l);
            }
        }
        if (next != numCells || visited != size_t(numNodes)) return fail(PMC_ERR_INVALID, "tree leaves and cells do not match");
        return PMC_OK;
    }

    inline int32_t binLinkOf(const pmc_grid& g, const BinTreeShape& S, const std::vector<int32_t>& perm, int id)
    {
        return g.node_first_child[id] < 0 ? perm[g.node_cell[id]] : PMC_BIN_NODE(S.internalIndex[id] * S.perNode);
    }

    inline std::vector<BinNodeRec> binTreeNodes(const pmc_grid& g, const BinTreeShape& S, const std::vector<int32_t>& perm)
    {
        std::vector<BinNodeRec> nodes(size_t(S.numInternal) * S.perNode, BinNodeRec{});
        for (int id = 0; id < g.num_nodes; ++id)
        {
            const int first = g.node_first_child[id];
            if (first < 0) continue;
            const double* c0 = g.node_box + 6 * size_t(first);  // CHILD_0
            BinNodeRec* rec = &nodes[size_t(S.internalIndex[id]) * S.perNode];
            if (S.fan == 2)
            {
                const int axis = g.node_level[id] % 3;
                rec[0].split = c0[3 + axis];
                rec[0].axis = axis;
                rec[0].child[0] = binLinkOf(g, S, perm, first), rec[0].child[1] = binLinkOf(g, S, perm, first + 1);
                continue;
            }
            // octree: record 0 decides x, records 1 + ix decide y, records 3 + ix + 2 iy decide z and name the child ix + 2 iy + 4 iz
            const int32_t base = S.internalIndex[id] * S.perNode;
            rec[0].split = c0[3], rec[0].axis = 0;
            rec[0].child[0] = PMC_BIN_NODE(base + 1), rec[0].child[1] = PMC_BIN_NODE(base + 2);
            for (int ix = 0; ix < 2; ++ix)
            {
                BinNodeRec& y = rec[1 + ix];
                y.split = c0[4], y.axis = 1;
                for (int iy = 0; iy < 2; ++iy)
                {
                    y.child[iy] = PMC_BIN_NODE(base + 3 + ix + 2 * iy);
                    BinNodeRec& z = rec[3 + ix + 2 * iy];
                    z.split = c0[5], z.axis = 2;
                    for (int iz = 0; iz < 2; ++iz) z.child[iz] = binLinkOf(g, S, perm, first + ix + 2 * iy + 4 * iz);
                }
            }
        }
        return nodes;
    }

    // the link through a wall of a leaf: the deepest node whose box covers the whole wall from the other side -- a leaf, or the internal node
    // whose split cuts the wall (finer neighbours: the walk descends with its position).  Descent by the split records alone: along the wall's
    // axis the side just beyond the wall decides, across it the wall's extent
    inline int32_t binWallLink(const pmc_grid& g, const std::vector<BinNodeRec>& nodes, int32_t rootLink, const double* box, int wall)
    {
        const int axis = wall >> 1, side = wall & 1;
        const double c = box[3 * side + axis];
        const double bound = side ? (axis == 0 ? g.xmax : axis == 1 ? g.ymax : g.zmax) : (axis == 0 ? g.xmin : axis == 1 ? g.ymin : g.zmin);
        if (c == bound) return PMC_BIN_OUTSIDE;
        int32_t link = rootLink;
        while (link < PMC_BIN_OUTSIDE)
        {
            const BinNodeRec& n = nodes[size_t(-2 - link)];
            if (n.axis == axis)
                link = n.child[side ? (c < n.split ? 0 : 1) : (c <= n.split ? 0 : 1)];
            else if (box[3 + n.axis] <= n.split)
                link = n.child[0];
            else if (box[n.axis] >= n.split)
                link = n.child[1];
            else
                break;
        }
        return link;
    }

    inline int buildBinTree(const pmc_grid& g, const double* density, BinTreeBuild& B)
    {
        const int numNodes = g.num_nodes, numCells = g.num_cells;
        if (numNodes < 1 || numCells < 1 || !g.node_box || !g.node_level || !g.node_first_child || !g.node_cell || !g.nbr_start || !g.nbr_list)
            return fail(PMC_ERR_INVALID, "tree grid tables are missing");
        if (size_t(numCells) > PMC_LINK_MAX_INDEX) return fail(PMC_ERR_UNSUPPORTED, "tree with 2^25 cells or more");
        if (g.node_level[0] != 0) return fail(PMC_ERR_INVALID, "tree root is not at level 0");
        BinTreeShape S;
        S.fan = g.kind == PMC_GRID_BINTREE ? 2 : 8;
        S.perNode = S.fan == 2 ? 1 : 7;
        if (int rc = binTreeNumbering(g, S, B.perm)) return rc;
        if (size_t(S.numInternal) * S.perNode > size_t(0x7FFFFFF0)) return fail(PMC_ERR_UNSUPPORTED, "tree with too many nodes");
        B.nodes = binTreeNodes(g, S, B.perm);
        B.rootLink = binLinkOf(g, S, B.perm, 0);
        B.cells.assign(size_t(numCells), BinCellRec{});
        B.density.assign(size_t(numCells), 0.);
        B.nbrStart.assign(6 * size_t(numCells) + 1, 0);
        B.nbrList.clear();
        B.cellExt.assign(numCells, -1);
        for (int m = 0; m < numCells; ++m) B.cellExt[B.perm[m]] = m;
        for (int dev = 0; dev < numCells; ++dev)
        {
            const int m = B.cellExt[dev];
            const int id = S.nodeOfCell[m];
            BinCellRec& rec = B.cells[dev];
            std::memcpy(rec.box, g.node_box + 6 * size_t(id), sizeof(rec.box));
            rec.density = B.density[dev] = density[m];
            for (int wall = 0; wall < 6; ++wall)
            {
                rec.link[wall] = binWallLink(g, B.nodes, B.rootLink, rec.box, wall);
                B.nbrStart[6 * size_t(dev) + wall] = (int32_t)B.nbrList.size();
                for (int q = g.nbr_start[6 * size_t(id) + wall]; q < g.nbr_start[6 * size_t(id) + wall + 1]; ++q)
                {
                    const int nb = g.nbr_list[q];
                    if (nb < 0 || nb >= numNodes || g.node_first_child[nb] >= 0)
                        return fail(PMC_ERR_INVALID, "neighbour list of a leaf contains a non-leaf node");
                    B.nbrList.push_back(B.perm[g.node_cell[nb]]);
                }
            }
        }
        B.nbrStart[6 * size_t(numCells)] = (int32_t)B.nbrList.size();
        return PMC_OK;
    }

    inline int uploadBinTreeGrid(const pmc_grid& g, const double* density, TableSink& sink, DevScene& D, std::vector<int32_t>& devToCell)
    {
        BinTreeBuild B;
        int rc = PMC_OK;
        if ((rc = buildBinTree(g, density, B))) return rc;
        if ((rc = sink.upload(B.cells.data(), B.cells.size(), &D.bin_cells))) return rc;
        if ((rc = sink.upload(B.nodes.data(), B.nodes.size(), &D.bin_nodes))) return rc;
        if ((rc = sink.upload(B.density.data(), B.density.size(), &D.cell_density))) return rc;
        if ((rc = sink.upload(B.nbrStart.data(), B.nbrStart.size(), &D.nbr_start))) return rc;
        if ((rc = sink.upload(B.nbrList.data(), B.nbrList.size(), &D.nbr_list))) return rc;
        if ((rc = sink.upload(B.cellExt.data(), B.cellExt.size(), &D.cell_ext))) return rc;
        D.bin_root = B.rootLink;
        D.cell_slots = g.num_cells;
        D.grid_kind = PMC_GRID_BINTREE;  // (also for an octree scene under the switch: every kernel and the run loop see a binary tree)
        D.lds_grid_len = 0;
        D.lmax = 0;
        devToCell = std::move(B.cellExt);
        return rc;
    }

    // ---- Voronoi -----------------------------------------------------------------------------------
    // what checkScene (pmc_scene_build.h) asks of a Voronoi grid before any table is built
    inline int checkVoronoiGrid(const pmc_grid& g)
    {
        if (g.num_cells < 1 || !g.site || !g.vnbr_start || !g.vnbr_list || g.vblock_n < 1 || !g.vblock_start || !g.vblock_list)
            return fail(PMC_ERR_INVALID, "Voronoi grid tables are missing");
        for (int m = 0; m < g.num_cells; ++m)
            for (int q = g.vnbr_start[m]; q < g.vnbr_start[m + 1]; ++q)
                if (g.vnbr_list[q] < -6 || g.vnbr_list[q] >= g.num_cells)
                    return fail(PMC_ERR_INVALID, "Voronoi neighbour list holds an invalid index");
        return PMC_OK;
    }

    // the cell records (DevScene::vsite): {site x, y, z, number density}
    inline std::vector<double> voroCellRecords(const pmc_grid& g, const double* density)
    {
        std::vector<double> rec(4 * size_t(g.num_cells));
        for (int m = 0; m < g.num_cells; ++m)
        {
            for (int a = 0; a < 3; ++a) rec[4 * size_t(m) + a] = g.site[3 * size_t(m) + a];
            rec[4 * size_t(m) + 3] = density[m];
        }
        return rec;
    }

    // the header record of a cell (DevScene::vhead)
    inline std::vector<double> voroHeaders(const pmc_grid& g, const double* density)
    {
        std::vector<double> head(8 * size_t(g.num_cells), 0.);
        for (int m = 0; m < g.num_cells; ++m)
        {
            for (int a = 0; a < 3; ++a) head[8 * size_t(m) + a] = g.site[3 * size_t(m) + a];
            head[8 * size_t(m) + 3] = density[m];
            const int32_t bounds[2] = {g.vnbr_start[m], g.vnbr_start[m + 1]};
            std::memcpy(&head[8 * size_t(m) + 4], bounds, sizeof(double));
        }
        return head;
    }

    // an entry {site x, y, z, neighbour index as the bit pattern of an int64} (a domain wall: zeros and its index -1 .. -6)
    inline void voroPackEntry(const pmc_grid& g, int mi, double* e)
    {
        e[0] = e[1] = e[2] = 0.;
        if (mi >= 0) e[0] = g.site[3 * size_t(mi)], e[1] = g.site[3 * size_t(mi) + 1], e[2] = g.site[3 * size_t(mi) + 2];
        const long long bits = mi;
        std::memcpy(&e[3], &bits, sizeof(double));
    }
    inline int voroEntryIndex(const double* e)
    {
        long long bits;
        std::memcpy(&bits, &e[3], sizeof(double));
        return int(bits);
    }

    // every neighbour of every cell as an entry, in list order: DevScene::vpair as it is, and what every table of runs takes its entries from
    inline std::vector<double> voroAllEntries(const pmc_grid& g)
    {
        const size_t np = size_t(g.vnbr_start[g.num_cells]);
        std::vector<double> all(4 * np);
        for (size_t q = 0; q < np; ++q) voroPackEntry(g, g.vnbr_list[q], &all[4 * q]);
        return all;
    }

    // neighbours that no direction of a cone can leave the cell through (DevScene::vcull), cells mFirst .. mLast - 1.  A cone = the directions with
    // one sign pattern and one order of |k_x|, |k_y|, |k_z|: the non-negative combinations of three extreme rays, so
    // n . k <= 0 on the cone <=> n . e <= 0 for the three rays; the margin (1e-9 |n| |e|) is far above the rounding of
    // the kernel's n . k.
    // 32-bit masks, 768 bytes per cell: a cell of the 10^5- and 10^6-site grids of the BASELINE scene has 15.2 / 15.4
    // neighbours on average, 99 % of the cells at most 24, 35 at most (neighbours beyond the 32nd are always read)
    inline void voroCullCells(const pmc_grid& g, int mFirst, int mLast, uint32_t* cull)
    {
        static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        // every cone is divided once more at the midpoints of its edges (PMC_VORO_CONES = 192: four sub-cones, the rays
        // e1, e1 + e2, e1 + e3 | e2, e1 + e2, e2 + e3 | e3, e1 + e3, e2 + e3 | e1 + e2, e1 + e3, e2 + e3)
        static const int sub[4][3][3] = {{{1, 0, 0}, {1, 1, 0}, {1, 0, 1}}, {{0, 1, 0}, {1, 1, 0}, {0, 1, 1}}, {{0, 0, 1}, {1, 0, 1}, {0, 1, 1}},
                                         {{1, 1, 0}, {1, 0, 1}, {0, 1, 1}}};
        const size_t ncell = size_t(g.num_cells);
        for (int m = mFirst; m < mLast; ++m)
            for (int q = g.vnbr_start[m]; q < g.vnbr_start[m + 1] && q - g.vnbr_start[m] < 32; ++q)
            {
                const int j = q - g.vnbr_start[m];
                const int mi = g.vnbr_list[q];
                double nv[3] = {0., 0., 0.};
                double norm = 0.;
                if (mi >= 0)
                {
                    for (int a = 0; a < 3; ++a) nv[a] = g.site[3 * size_t(mi) + a] - g.site[3 * size_t(m) + a];
                    norm = std::sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
                }
                for (int sgn = 0; sgn < 8; ++sgn)
                    for (int p = 0; p < 6; ++p)
                    {
                        // the extreme rays of the cone: e1 along the largest component, e2 = e1 + the second, e3 = e2 + the third
                        double e[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
                        for (int r = 0; r < 3; ++r)
                            for (int t = r; t < 3; ++t) e[t][perm[p][r]] = ((sgn >> perm[p][r]) & 1) ? -1. : 1.;
                        for (int c = 0; c < PMC_VORO_CONES / 48; ++c)
                        {
                            bool skip;
                            if (mi >= 0)
                            {
                                skip = norm > 0.;
                                for (int r = 0; r < 3 && skip; ++r)
                                {
                                    double ray[3];
                                    for (int a = 0; a < 3; ++a)
                                        ray[a] = PMC_VORO_CONES == 48 ? e[r][a] : sub[c][r][0] * e[0][a] + sub[c][r][1] * e[1][a] + sub[c][r][2] * e[2][a];
                                    const double dot = nv[0] * ray[0] + nv[1] * ray[1] + nv[2] * ray[2];
                                    if (!(dot <= -1e-9 * norm * 4.)) skip = false;
                                }
                            }
                            else
                            {
                                // walls -1 .. -6: x min, x max, y min, y max, z min, z max (reached only by k_a < 0 / k_a > 0)
                                const int wall = -mi - 1;
                                if (wall > 5) continue;
                                const bool negative = ((sgn >> (wall >> 1)) & 1) != 0;
                                skip = (wall & 1) ? negative : !negative;
                            }
                            // (cone-major: the masks of one cone are consecutive -- the walks towards an observer all use one cone)
                            if (skip) cull[size_t((sgn * 6 + p) * (PMC_VORO_CONES / 48) + c) * ncell + size_t(m)] |= 1u << j;
                        }
                    }
            }
    }

    // ... of all cells (they are independent: all host cores)
    inline std::vector<uint32_t> voroCullMasks(const pmc_grid& g)
    {
        const int ncell = g.num_cells;
        std::vector<uint32_t> cull(size_t(ncell) * PMC_VORO_CONES, 0u);
        const int workers = std::max(1, std::min<int>(64, (int)std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (int t = 0; t < workers; ++t)
            pool.emplace_back(voroCullCells, std::cref(g), int(int64_t(ncell) * t / workers), int(int64_t(ncell) * (t + 1) / workers), cull.data());
        for (auto& t : pool) t.join();
        return cull;
    }

    // the cone of a direction: as voroCone (pmc_walk_voro.inc)
    inline int voroConeOf(double kx, double ky, double kz)
    {
        const int sgn = (kx < 0. ? 1 : 0) | (ky < 0. ? 2 : 0) | (kz < 0. ? 4 : 0);
        const double ax = std::fabs(kx), ay = std::fabs(ky), az = std::fabs(kz);
        int pp;
        if (ax >= ay)
            pp = ay >= az ? 0 : ax >= az ? 1 : 4;
        else
            pp = ax >= az ? 2 : ay >= az ? 3 : 5;
        int cone = sgn * 6 + pp;
        if (PMC_VORO_CONES != 48)
        {
            const double x = std::fmax(ax, std::fmax(ay, az)), z = std::fmin(ax, std::fmin(ay, az)), y = (ax + ay + az) - x - z;
            const double a = x - y, b = y - z, c = z;
            const int subc = a >= b + c ? 0 : b >= a + c ? 1 : c >= a + b ? 2 : 3;
            cone = cone * 4 + subc;
        }
        return cone;
    }

    // the entries of a table of runs: of `all` those that numMasks cones (masks[i * num_cells + m]) do not ALL cull -- a neighbour beyond the 32nd is
    // always kept --, in list order (kept), and where every cell's entries start (first[num_cells + 1]).  kobs != null: ONE direction, an observer's;
    // the candidate test of the walk itself (voroCandidate: n . k > 0, the same doubles in the same order, no contraction) decides which sites can
    // ever be the exit -- half of them
    inline void voroKeptEntries(const pmc_grid& g, const std::vector<double>& all, const uint32_t* masks, int numMasks, const double* kobs,
                                std::vector<double>& kept, std::vector<int32_t>& first)
    {
        const int ncell = g.num_cells;
        kept.clear();
        kept.reserve(all.size() * 3 / 4);
        first.resize(size_t(ncell) + 1);
        for (int m = 0; m < ncell; ++m)
        {
            first[m] = int32_t(kept.size() / 4);
            uint32_t mask = 0xFFFFFFFFu;
            for (int i = 0; i < numMasks; ++i) mask &= masks[size_t(i) * size_t(ncell) + size_t(m)];
            for (int q = g.vnbr_start[m]; q < g.vnbr_start[m + 1]; ++q)
            {
                const int j = q - g.vnbr_start[m];
                if (j < 32 && ((mask >> j) & 1u)) continue;
                const double* e = &all[4 * size_t(q)];
                if (kobs && g.vnbr_list[q] >= 0)
                {
                    const double nx = e[0] - g.site[3 * size_t(m)], ny = e[1] - g.site[3 * size_t(m) + 1], nz = e[2] - g.site[3 * size_t(m) + 2];
                    const double ndotk = nx * kobs[0] + ny * kobs[1] + nz * kobs[2];
                    if (!(ndotk > 0)) continue;
                }
                kept.insert(kept.end(), e, e + 4);
            }
        }
        first[ncell] = int32_t(kept.size() / 4);
    }
    // per main cone (DevScene::vcone_run): what the masks of its four sub-cones keep
    inline void voroKeptOfCone(const pmc_grid& g, const std::vector<double>& all, const std::vector<uint32_t>& cull, int mainCone, std::vector<double>& kept,
                               std::vector<int32_t>& first)
    {
        voroKeptEntries(g, all, &cull[size_t(4 * mainCone) * size_t(g.num_cells)], 4, nullptr, kept, first);
    }
    // per observer (DevScene::vobs_run): what the mask of its direction's cone keeps and, unless exactCull is off, the walk's own test
    inline void voroKeptOfObserver(const pmc_grid& g, const std::vector<double>& all, const std::vector<uint32_t>& cull, const double kobs[3], bool exactCull,
                                   std::vector<double>& kept, std::vector<int32_t>& first)
    {
        voroKeptEntries(g, all, &cull[size_t(voroConeOf(kobs[0], kobs[1], kobs[2])) * size_t(g.num_cells)], 1, exactCull ? kobs : nullptr, kept, first);
    }

    // ---- a table of RUNS (DevScene::vobs_run, vcone_run, vgen_run): per cell ONE run of 64-byte units -- header {site, density, number of entries}, then its
    // entries (first[m] .. first[m + 1] of `entries`) in groups of PMC_VORO_RUN_LANES, a group as {x, y} of each entry followed by {z, tag} of each: the
    // lanes that share a walk read a group with two coalesced loads.  An entry's tag carries the unit at which its neighbour's run starts next to the
    // neighbour's index.  start[m]: the link to the run of cell m (pmc_device.h PMC_VORO_RUN_UNIT_BITS); it has num_cells + 1 elements, the last unused
    struct VoroRuns
    {
        std::vector<double> runs;
        std::vector<uint32_t> start;
    };
    // (cells with more entries than a link can name -- linkCountMax: 30 -- say so in their header)
    inline int voroPackRuns(const pmc_grid& g, const double* density, const std::vector<double>& entries, const std::vector<int32_t>& first, uint32_t linkCountMax,
                            VoroRuns& R)
    {
        constexpr size_t LANES = PMC_VORO_RUN_LANES, GROUP_UNITS = LANES / 2;
        const int ncell = g.num_cells;
        std::vector<uint32_t>& start = R.start;
        start.assign(size_t(ncell) + 1, 0u);
        size_t units = 0;
        for (int m = 0; m < ncell; ++m)
        {
            // (the link to the run: its first unit and, up to 30, the number of its entries)
            const uint32_t entriesOf = uint32_t(first[m + 1] - first[m]);
            start[m] = uint32_t(units & PMC_VORO_RUN_UNIT_MASK) | ((entriesOf > linkCountMax ? PMC_VORO_RUN_COUNT_UNKNOWN : entriesOf) << PMC_VORO_RUN_UNIT_BITS);
            units += 1 + GROUP_UNITS * ((size_t(entriesOf) + LANES - 1) / LANES);
        }
        if (units + PMC_VORO_RUN_PAD >= (size_t(1) << PMC_VORO_RUN_UNIT_BITS))
            return fail(PMC_ERR_UNSUPPORTED, "Voronoi table of runs beyond 2^27 units of 64 bytes");
        R.runs.assign(8 * (units + PMC_VORO_RUN_PAD), 0.);  // (padding: a walk may request a group that the run does not have)
        const unsigned long long noEntry = (unsigned long long)(uint32_t)(-7);
        for (int m = 0; m < ncell; ++m)
        {
            double* head = &R.runs[8 * size_t(start[m] & PMC_VORO_RUN_UNIT_MASK)];
            for (int a = 0; a < 3; ++a) head[a] = g.site[3 * size_t(m) + a];
            head[3] = density[m];
            const int32_t count[2] = {first[m + 1] - first[m], 0};
            std::memcpy(&head[4], count, sizeof(double));
            const size_t groups = (size_t(count[0]) + LANES - 1) / LANES;
            for (size_t e = 0; e < groups * LANES; ++e)
            {
                double* group = head + 8 + 4 * LANES * (e / LANES);
                double* xy = group + 2 * (e % LANES);
                double* zt = group + 2 * LANES + 2 * (e % LANES);
                unsigned long long tag = noEntry;
                if (e < size_t(count[0]))
                {
                    const double* src = &entries[4 * (size_t(first[m]) + e)];
                    xy[0] = src[0], xy[1] = src[1], zt[0] = src[2];
                    const int mi = voroEntryIndex(src);
                    tag = (unsigned long long)(uint32_t)mi | (mi >= 0 ? (unsigned long long)start[mi] << 32 : 0ull);
                }
                std::memcpy(&zt[1], &tag, sizeof(double));
            }
        }
        return PMC_OK;
    }

    inline int uploadVoroRuns(const pmc_grid& g, const double* density, const std::vector<double>& entries, const std::vector<int32_t>& first, const SceneSwitches& sw,
                              TableSink& sink, const double** runsOut, const uint32_t** startOut)
    {
        VoroRuns R;
        int rc = PMC_OK;
        if ((rc = voroPackRuns(g, density, entries, first, sw.voroLinkCountMax, R))) return rc;
        if ((rc = sink.upload(R.runs.data(), R.runs.size(), runsOut))) return rc;
        return sink.upload(R.start.data(), size_t(g.num_cells), startOut);
    }

    // per main cone the entries its sub-cones' masks keep, as tables of runs; built and handed over `workers` cones at a time (a table of the
    // 10^6-site scene takes about 0.8 GB of host memory while it is built)
    inline int uploadVoroConeRuns(const pmc_grid& g, const double* density, const std::vector<double>& all, const std::vector<uint32_t>& cull, const SceneSwitches& sw,
                                  TableSink& sink, DevScene& D)
    {
        const int workers = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
        for (int c0 = 0; c0 < 48; c0 += workers)
        {
            const int nc = std::min(workers, 48 - c0);
            std::vector<std::vector<double>> kept(nc);
            std::vector<std::vector<int32_t>> firstKept(nc);
            std::vector<std::thread> pool;
            for (int w = 0; w < nc; ++w) pool.emplace_back([&, w]() { voroKeptOfCone(g, all, cull, c0 + w, kept[w], firstKept[w]); });
            for (auto& t : pool) t.join();
            for (int w = 0; w < nc; ++w)
                if (int rc = uploadVoroRuns(g, density, kept[w], firstKept[w], sw, sink, &D.vcone_run[c0 + w], &D.vcone_start[c0 + w])) return rc;
        }
        return PMC_OK;
    }

    // per observer: the kept neighbour entries of its cone, packed (DevScene::vobs_*).  All peel-off walks towards an observer have ONE direction,
    // hence one cone and one mask per cell
    inline int uploadVoroObserverRuns(const pmc_scene& scene, const double* density, const std::vector<double>& all, const std::vector<uint32_t>& cull,
                                      const SceneSwitches& sw, TableSink& sink, DevScene& D)
    {
        const pmc_grid& g = scene.grid;
        int k = -1;
        for (int i = 0; i < scene.num_instruments; ++i)
        {
            const pmc_instrument& ins = scene.instruments[i];
            if (ins.same_observer_as_preceding)
            {
                D.vobs_of_inst[i] = (int8_t)k;
                continue;
            }
            // (memory: at most 32 B per neighbour entry + 64 B per cell and observer; the tables are an acceleration only, so an
            //  observer whose tables would take more than a quarter of the free device memory goes without, as do the later ones:
            //  their walks use the cone masks)
            const size_t need = 32 * size_t(g.vnbr_start[g.num_cells]) + 64 * size_t(g.num_cells);
            const size_t freeBytes = sink.freeBytes();
            if (need > freeBytes / 4)
            {
                fprintf(stderr, "libpmc: per-observer Voronoi tables left out from observer %d on (%.1f GiB each, %.1f GiB free): peel-off walks use the cone masks\n",
                        k + 1, double(need) / double(1 << 30), double(freeBytes) / double(1 << 30));
                break;
            }
            ++k;
            D.vobs_of_inst[i] = (int8_t)k;
            std::vector<double> kept;
            std::vector<int32_t> first;
            voroKeptOfObserver(g, all, cull, ins.kobs, !sw.voroConeCullOnly, kept, first);
            if (int rc = uploadVoroRuns(g, density, kept, first, sw, sink, &D.vobs_run[k], &D.vobs_start[k])) return rc;
        }
        return PMC_OK;
    }

    // build one table, hand it to the sink, drop the host copy: what is left out for want of memory depends on what went before
    // (the grid has passed checkVoronoiGrid)
    inline int uploadVoronoiGrid(const pmc_scene& scene, const double* density, const SceneSwitches& sw, TableSink& sink, DevScene& D)
    {
        const pmc_grid& g = scene.grid;
        const int ncell = g.num_cells;
        int rc = PMC_OK;
        {
            const std::vector<double> rec = voroCellRecords(g, density);
            if ((rc = sink.upload(rec.data(), rec.size(), &D.vsite))) return rc;
        }
        if ((rc = sink.upload(g.vnbr_start, size_t(ncell) + 1, &D.vnbr_start))) return rc;
        if ((rc = sink.upload(g.vnbr_list, size_t(g.vnbr_start[ncell]), &D.vnbr_list))) return rc;
        const std::vector<double> all = voroAllEntries(g);
        if ((rc = sink.upload(all.data(), all.size(), &D.vpair))) return rc;
        {
            const std::vector<double> head = voroHeaders(g, density);
            if ((rc = sink.upload(head.data(), head.size(), &D.vhead))) return rc;
        }
        D.vcull = nullptr;
        for (int i = 0; i < 16; ++i) D.vobs_of_inst[i] = -1;
        bool genRuns = false;
        if (!sw.voroNoCull)
        {
            const std::vector<uint32_t> cull = voroCullMasks(g);
            if ((rc = sink.upload(cull.data(), cull.size(), &D.vcull))) return rc;
            // all neighbours of a cell as a run (DevScene::vgen_run): what a PROPAGATION walk in voroPropKernel reads -- no mask, one run of
            // memory (4.75 lines per visit instead of header + mask + scattered entries: 6.2); left out where device memory is short
            const size_t need = 32 * size_t(g.vnbr_start[ncell]) + 96 * size_t(ncell);
            if (!sw.voroNoPropKernel && need <= sink.freeBytes() / 4)
            {
                std::vector<int32_t> firstAll(g.vnbr_start, g.vnbr_start + ncell + 1);
                if ((rc = uploadVoroRuns(g, density, all, firstAll, sw, sink, &D.vgen_run, &D.vgen_start))) return rc;
                genRuns = true;
                if (PMC_VORO_CONES == 192 && !sw.voroNoConeTables && 48 * need <= sink.freeBytes() / 4)
                    if ((rc = uploadVoroConeRuns(g, density, all, cull, sw, sink, D))) return rc;
            }
            int observers = 0;
            for (int i = 0; i < scene.num_instruments; ++i) observers += scene.instruments[i].same_observer_as_preceding ? 0 : 1;
            if (observers <= 4 && scene.num_instruments <= 16 && !sw.voroNoObserverLists)
                if ((rc = uploadVoroObserverRuns(scene, density, all, cull, sw, sink, D))) return rc;
        }
        // (bit 0: peel-off walks of voroPeelKernel, bit 1: propagation walks of voroPropKernel)
        D.voro_defer_scan = (!sw.voroNoPeelKernel && !sw.voroNoDeferredScan) ? 1 : 0;
        if (genRuns && !sw.voroNoDeferredScan) D.voro_defer_scan |= 2;
        const size_t nb3 = size_t(g.vblock_n) * g.vblock_n * g.vblock_n;
        D.vblock_n = g.vblock_n;
        if ((rc = sink.upload(g.vblock_start, nb3 + 1, &D.vblock_start))) return rc;
        if ((rc = sink.upload(g.vblock_list, size_t(g.vblock_start[nb3]), &D.vblock_list))) return rc;
        D.lds_grid_len = 0;
        D.lmax = 0;
        return rc;
    }
}

#endif
