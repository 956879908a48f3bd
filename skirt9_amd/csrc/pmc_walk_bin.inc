// pmc_walk_bin.inc -- binary-tree grids (PolicyTreeSpatialGrid with treeType BinTree; included by pmc_walk.inc): the step of the generic walk
// kernel over self-contained cell records (pmc_device.h BinCellRec, BinNodeRec).
//
// A walk on a binary tree keeps, as its pending segment, the cell w.cell (device index), the exit distance w.ds, the exit axis w.axis and
// -- in w.ci -- the cell record's link through the exit wall.  The step advances by ds + eps as the reference does
// (TreeSpatialGrid.cpp:186), follows that link (below an internal node: the child rule, one dependent gather per level), loads the
// candidate's record and accepts it only if the new position lies STRICTLY inside its box.  Leaves tile the domain, so at most one leaf
// holds a point strictly inside: the reference's neighbour-list scan with the closed box and its top-down search both end there.  Every
// other case -- a position on a wall, a link that led elsewhere -- goes to the service round, which runs the reference's algorithm
// literally (binStepSlow).  A wrong link can therefore cost time and never a wrong cell.

    // the leaf below `link` for a position (BinTreeNode::child, BinTreeNode.cpp:53-62: r.a < CHILD_0->max.a)
    __device__ __forceinline__ int binDescend(const DevScene& S, int link, double x, double y, double z)
    {
        while (link < PMC_BIN_OUTSIDE)
        {
            const BinNodeRec* node = S.bin_nodes + (-2 - link);
            const uint4 h = *reinterpret_cast<const uint4*>(node);  // split, axis, child 0
            const int other = node->child[1];
            const double split = __longlong_as_double(((long long)h.y << 32) | h.x);
            const double v = h.z == 0u ? x : h.z == 1u ? y : z;
            link = v < split ? (int)h.w : other;
        }
        return link;
    }
    // root()->leafChild(r) (TreeNode.cpp:66-76): -1 outside the closed root box
    __device__ __forceinline__ int binTopDown(const DevScene& S, double x, double y, double z)
    {
        if (!(x >= S.gx0 && x <= S.gx1 && y >= S.gy0 && y <= S.gy1 && z >= S.gz0 && z <= S.gz1)) return -1;
        return binDescend(S, S.bin_root, x, y, z);
    }
    // the pending segment of cell m from the walk's position (TreeSpatialGrid.cpp:160-185); with CHECK only if the position lies strictly
    // inside the cell's box (else false, w untouched)
    template<bool CHECK> __device__ __forceinline__ bool binEnter(const DevScene& S, Walk& w, int m)
    {
        const BinCellRec* rec = S.bin_cells + m;
        const double X0 = rec->box[0], Y0 = rec->box[1], Z0 = rec->box[2], X1 = rec->box[3], Y1 = rec->box[4], Z1 = rec->box[5];
        if (CHECK)
        {
            const bool inside = w.rx > X0 && w.rx < X1 && w.ry > Y0 && w.ry < Y1 && w.rz > Z0 && w.rz < Z1;
            if (!inside) return false;
        }
        double ds;
        int ax;
        exitDistance<false>(w, w.kx < 0.0 ? X0 : X1, w.ky < 0.0 ? Y0 : Y1, w.kz < 0.0 ? Z0 : Z1, ds, ax);
        w.ds = ds;
        w.axis = ax;
        w.cell = m;
        w.dens = rec->density;
        w.ci = rec->link[2 * ax + (((w.sgn >> ax) & 1u) ? 0 : 1)];
        return true;
    }
    // one step: returns the lane's state (ST_ACTIVE: the next pending segment is ready)
    __device__ __forceinline__ int binAdvance(const DevScene& S, Walk& w)
    {
        const double step = w.ds + S.eps;
        w.rx += w.kx * step;
        w.ry += w.ky * step;
        w.rz += w.kz * step;
        int link = w.ci;
        if (link == PMC_BIN_OUTSIDE)
        {
            // (no neighbour across this wall: the reference's top-down search returns no node once the position has left the closed root
            // box, and the path ends; a position that rounding has kept inside goes through the literal algorithm)
            const bool inside = w.rx >= S.gx0 && w.rx <= S.gx1 && w.ry >= S.gy0 && w.ry <= S.gy1 && w.rz >= S.gz0 && w.rz <= S.gz1;
            return inside ? ST_SLOW : ST_EXIT;
        }
        link = binDescend(S, link, w.rx, w.ry, w.rz);
        return (link >= 0 && binEnter<true>(S, w, link)) ? ST_ACTIVE : ST_SLOW;
    }
    // TreeSpatialGrid.cpp:192-207, literally, from the advanced position: the old cell's neighbour list in list order with the closed box
    // (TreeNode::neighbor, TreeNode.cpp:103-112), the top-down search, the next-after escape.  False: the path has left the grid.
    __device__ __forceinline__ bool binStepSlow(const DevScene& S, Walk& w)
    {
        const int old = w.cell;
        const int wall = 2 * w.axis + (((w.sgn >> w.axis) & 1u) ? 0 : 1);
        int next = -1;
        const int e = S.nbr_start[6 * (int64_t)old + wall + 1];
        for (int q = S.nbr_start[6 * (int64_t)old + wall]; q < e; ++q)
        {
            const int cand = S.nbr_list[q];
            const double* b = S.bin_cells[cand].box;
            if (w.rx >= b[0] && w.rx <= b[3] && w.ry >= b[1] && w.ry <= b[4] && w.rz >= b[2] && w.rz <= b[5])
            {
                next = cand;
                break;
            }
        }
        if (next < 0) next = binTopDown(S, w.rx, w.ry, w.rz);
        if (next == old)
        {
            // PathSegmentGenerator::propagateToNextAfter (PathSegmentGenerator.hpp:148-153)
            w.rx = nextAfterToward(w.rx, w.kx < 0.);
            w.ry = nextAfterToward(w.ry, w.ky < 0.);
            w.rz = nextAfterToward(w.rz, w.kz < 0.);
            next = binTopDown(S, w.rx, w.ry, w.rz);
        }
        if (next < 0 || next == old) return false;
        binEnter<false>(S, w, next);
        return true;
    }
    // the first cell of a walk whose position moveInside has left inside the root box: the hinted cell if the position lies strictly inside
    // it, else the top-down search
    __device__ __forceinline__ void binStart(const DevScene& S, Walk& w, int hint)
    {
        if (hint >= 0 && binEnter<true>(S, w, hint)) return;
        binEnter<false>(S, w, binTopDown(S, w.rx, w.ry, w.rz));
    }
