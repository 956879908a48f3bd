// pmc_walk.inc -- grid traversal and the walk kernel (included by pmc_kernels.hip inside its anonymous namespace).  The step of a Voronoi
// grid is in pmc_walk_voro.inc, that of a binary tree in pmc_walk_bin.inc; the Voronoi kernels of their own in pmc_walk_voro_run.inc.
//
// The hot loop of the engine is ONE straight-line step per cell visit (no data-dependent branch except the rare
// descent to a much finer neighbour): add the pending segment, test the stop condition, advance the position, follow
// ONE link to the next cell record, check that the position lies strictly inside it, compute the next exit distance.
// Everything that is rare for a lane but common for a 64-lane wave is DEFERRED: a lane whose walk has ended, or whose
// next cell cannot be decided by the strict test, only changes its state; the wave services all such lanes together
// (literal reference algorithm for the undecided ones, result write-out, start of the next walks) when enough of
// them have accumulated.
//
// Exit distances (TreeSpatialGrid.cpp:160-185, CartesianSpatialGrid.cpp:112-119): the reference evaluates the three
// quotients (wall - r)/k and applies its tie order.  The kernel evaluates the same three CORRECTLY ROUNDED quotients
// without a division instruction: with y = RN(1/k) (one true division per walk and axis) it refines q = d*y twice
// with fused multiply-adds, r = fma(-k, q, d), q = fma(r, y, q).  After the first refinement q is within half an ulp
// (plus 2^-105 relative) of d/k, and by Markstein's theorem the second one then yields RN(d/k), i.e. exactly what
// the IEEE division of the reference returns; then the reference's own comparisons are applied to the same doubles.
// (The theorem excludes divisors whose significand is all ones: probability 2^-52 per direction component.)

    // ------------------------------------------------------------------------------------------------
    // per-lane walk state (the PathSegmentGenerator of the reference plus the running sums of the caller)
    struct Walk
    {
        double rx, ry, rz;     // generator position (PathSegmentGenerator::_rx..)
        double kx, ky, kz;     // direction
        double ikx, iky, ikz;  // RN(1/k); NaN where the reference ignores the axis (|k| <= 1e-15)
        double tau, s;         // cumulative optical depth and path length of the segments emitted so far
        double ds;             // length of the pending segment (exit distance of the current cell)
        double dens;           // number density of the current cell
        uint32_t e;            // octree: size exponent of the current cell (its edge spans 2^e finest-level cells)
        uint64_t P;            // octree: fine lower-corner indices of the current cell, x | y << FB | z << 2 FB with FB = 10
                               // (trees up to level 10) or 21 (pmc_walk_tree.inc Pack)
        int ci, cj, ck;        // Cartesian indices
        int cell;              // cell index m of the pending segment
        int axis;              // exit axis 0,1,2 of the pending segment
        int lastm;             // cell of the last segment added to the path
        uint32_t sgn;          // bit a set: k_a < 0
    };

    struct GridLds
    {
        const double* grid;  // octree: coordinate tables [3][tabn]; Cartesian: xv | yv | zv
        const char* gtab;    // octree deeper than level 12: the coordinate table in global memory (it does not fit in LDS); else null
        uint32_t stride;     // octree: bytes per axis of the coordinate table
        uint32_t fieldBits;  // octree: bits per axis of the packed cell indices (Walk::P)
    };

    __device__ __forceinline__ GridLds makeGridLds(const DevScene& S, const double* lds)
    {
        GridLds L;
        L.grid = lds;
        L.gtab = (S.grid_kind == PMC_GRID_OCTREE && !S.tab_in_lds) ? reinterpret_cast<const char*>(S.coord_tab) : nullptr;
        L.stride = S.tab_stride_bytes;
        L.fieldBits = S.lmax > 10 ? 21u : 10u;
        return L;
    }

    // the octree coordinate table starts at LDS address 0 (the kernels that use it have no static LDS; checked at
    // kernel start), so a box-code offset IS the LDS address: no base add per access
    typedef __attribute__((address_space(3))) const double LdsDouble;
    __device__ __forceinline__ double ldsAt(const double*, uint32_t byteOffset)
    {
        return *reinterpret_cast<LdsDouble*>(static_cast<uintptr_t>(byteOffset));
    }
    // the same entry wherever the table lives: in LDS (gtab null: octrees up to level 12), or in global memory (a table of
    // 2^13 + 1 entries per axis and more does not fit in 160 KB); gtab is wave-uniform: a scalar branch
    __device__ __forceinline__ double tabAt(const char* gtab, uint32_t byteOffset)
    {
        if (gtab) return *reinterpret_cast<const double*>(gtab + byteOffset);
        return *reinterpret_cast<LdsDouble*>(static_cast<uintptr_t>(byteOffset));
    }
    __device__ __forceinline__ void requireLdsBaseZero(const double* dynamicLds)
    {
        typedef __attribute__((address_space(3))) const void LdsVoid;
        if (reinterpret_cast<uintptr_t>((LdsVoid*)dynamicLds) != 0) __builtin_trap();
    }

    // RN(d/k) from y = RN(1/k) (see the header); DBL_MAX for an ignored axis (y = NaN)
    __device__ __forceinline__ double exactQuotient(double d, double k, double y)
    {
        double q = d * y;
        double r = __builtin_fma(-k, q, d);
        q = __builtin_fma(r, y, q);
        r = __builtin_fma(-k, q, d);
        q = __builtin_fma(r, y, q);
        return fmin(q, DBL_MAX);
    }

    // selection of the exit wall: the axis and the exit distance with the reference's tie order
    // (TreeSpatialGrid.cpp:176-185; CartesianSpatialGrid.cpp:115-119 for CARTESIAN_TIES)
    template<bool CARTESIAN_TIES>
    __device__ __forceinline__ void exitDistance(const Walk& w, double xnext, double ynext, double znext, double& ds, int& axis)
    {
        const double dsx = exactQuotient(xnext - w.rx, w.kx, w.ikx);
        const double dsy = exactQuotient(ynext - w.ry, w.ky, w.iky);
        const double dsz = exactQuotient(znext - w.rz, w.kz, w.ikz);
        const bool selx = dsx <= dsy && dsx <= dsz;
        const bool sely = (CARTESIAN_TIES ? (dsy < dsx) : (dsy <= dsx)) && dsy <= dsz;
        double d = dsz;
        int a = 2;
        if (sely)
        {
            d = dsy;
            a = 1;
        }
        if (selx)
        {
            d = dsx;
            a = 0;
        }
        ds = d;
        axis = a;
    }

    __device__ __forceinline__ void setDirection(Walk& w, double kx, double ky, double kz)
    {
        const double ignored = __longlong_as_double(0x7ff8000000000000ll);
        w.kx = kx, w.ky = ky, w.kz = kz;
        w.ikx = (fabs(kx) > 1e-15) ? 1. / kx : ignored;
        w.iky = (fabs(ky) > 1e-15) ? 1. / ky : ignored;
        w.ikz = (fabs(kz) > 1e-15) ? 1. / kz : ignored;
        w.sgn = (kx < 0. ? 1u : 0u) | (ky < 0. ? 2u : 0u) | (kz < 0. ? 4u : 0u);
    }

    // ------------------------------------------------------------------------------------------------
    // octree helpers.  Box code (LeafRec::code, NodeRec::code): bits 0-19 index of the lower x wall in the coordinate table of its axis,
    // 20-39 lower y wall, 40-59 lower z wall, 60-63 size exponent e (box edge = 2^e finest cells) -- or 15 for e >= 15: the lower walls of such
    // a box are multiples of 2^15, and the low five bits of the x index hold e - 15 (trees of up to PMC_MAX_LEVEL = 20 levels; rounds 1-5 stored
    // byte offsets of the whole table here, which ends at level 15).  Decoded: byte offsets into the table of all three axes, and 8 << e.
    __device__ __forceinline__ void decodeBoxWords(uint32_t lo, uint32_t hi, uint32_t stride, uint32_t& ox, uint32_t& oy, uint32_t& oz, uint32_t& e)
    {
        uint32_t ix = lo & 0xFFFFFu;
        const uint32_t iy = ((lo >> 20) | (hi << 12)) & 0xFFFFFu;
        const uint32_t iz = (hi >> 8) & 0xFFFFFu;
        e = hi >> 28;
        if (e == 15u)
        {
            e += ix & 31u;
            ix &= ~31u;
        }
        ox = ix << 3;
        oy = (iy << 3) + stride;
        oz = (iz << 3) + 2u * stride;
    }
    __device__ __forceinline__ void decodeBox(uint64_t code, uint32_t stride, uint32_t& ox, uint32_t& oy, uint32_t& oz, uint32_t& szb)
    {
        uint32_t e;
        decodeBoxWords((uint32_t)code, (uint32_t)(code >> 32), stride, ox, oy, oz, e);
        szb = 8u << e;
    }

    // std::nextafter(x, negative ? -DBL_MAX : DBL_MAX) for finite |x| < DBL_MAX, without the library call
    __device__ __forceinline__ double nextAfterToward(double x, bool negative)
    {
        if (x == 0.) return negative ? -4.9406564584124654e-324 : 4.9406564584124654e-324;
        long long b = __double_as_longlong(x);
        b += ((x > 0.) != negative) ? 1 : -1;
        return __longlong_as_double(b);
    }

    // index of the finest-level interval [tab[i], tab[i+1]) of one axis that contains v (the last interval is closed):
    // exactly the sequence of `v < centre` decisions of the reference's descent, because every node centre IS an entry
    // of the coordinate table.  Arithmetic guess, corrected against the table in LDS.
    __device__ __forceinline__ int fineIndex(const DevScene& S, const GridLds& L, int axis, double v, double lo)
    {
        const int n = 1 << S.lmax;
        const uint32_t base = (uint32_t)axis * S.tab_stride_bytes;
        int i = (int)((v - lo) * S.fine_scale[axis]);
        i = max(0, min(n - 1, i));
        while (i > 0 && v < tabAt(L.gtab, base + 8u * (uint32_t)i)) --i;
        while (i < n - 1 && v >= tabAt(L.gtab, base + 8u * (uint32_t)(i + 1))) ++i;
        return i;
    }
    // root()->leafChild(r) (TreeNode.cpp:66-76, OctTreeNode.cpp:36-41): -1 if r is outside the (closed) root box.  The
    // octant decisions are taken once, as the finest-level indices of r; the search starts at the node of level Lc
    // from a table over the coarse cells (one gather from 1 MB) and follows ONE child link per remaining level, picked by
    // the index bits -- at most lmax - Lc dependent loads instead of two per level from the root.
    __device__ __forceinline__ int topDown(const DevScene& S, const GridLds& L, double x, double y, double z)
    {
        if (!(x >= S.gx0 && x <= S.gx1 && y >= S.gy0 && y <= S.gy1 && z >= S.gz0 && z <= S.gz1)) return -1;
        const int ix = fineIndex(S, L, 0, x, S.gx0), iy = fineIndex(S, L, 1, y, S.gy0), iz = fineIndex(S, L, 2, z, S.gz0);
        const int lc = S.coarse_level, sh = S.lmax - lc;
        uint32_t link = S.coarse_tab[((((int64_t)(iz >> sh) << lc) + (iy >> sh)) << lc) + (ix >> sh)];
        while ((int32_t)link < 0)
        {
            const int bit = (int)(link & PMC_LINK_EXP_MASK) - 1;  // the children's size exponent
            const int l = ((ix >> bit) & 1) | (((iy >> bit) & 1) << 1) | (((iz >> bit) & 1) << 2);
            link = S.nodes[(link >> PMC_LINK_EXP_BITS) & PMC_LINK_INDEX_MASK].child[l];
        }
        return link == PMC_LINK_NONE ? -1 : (int)(link >> PMC_LINK_EXP_BITS);
    }
    __device__ __forceinline__ bool leafContains(const DevScene& S, const GridLds& L, int m, double x, double y, double z)
    {
        uint32_t ox, oy, oz, szb;
        decodeBox(S.leaves[m].code, L.stride, ox, oy, oz, szb);
        return x >= tabAt(L.gtab, ox) && x <= tabAt(L.gtab, ox + szb) && y >= tabAt(L.gtab, oy) && y <= tabAt(L.gtab, oy + szb)
               && z >= tabAt(L.gtab, oz) && z <= tabAt(L.gtab, oz + szb);
    }
    // TreeNode::neighbor on the reference's neighbour list (TreeNode.cpp:103-112)
    __device__ __forceinline__ int listNeighbor(const DevScene& S, const GridLds& L, int m, int wall, double x, double y, double z)
    {
        int b = S.nbr_start[6 * (int64_t)m + wall], e = S.nbr_start[6 * (int64_t)m + wall + 1];
        for (int q = b; q < e; ++q)
        {
            int cand = S.nbr_list[q];
            if (leafContains(S, L, cand, x, y, z)) return cand;
        }
        return -1;
    }

    // loads the 16-byte head of the record of leaf m (box code + density; the links are not fetched here) and prepares
    // the pending segment (TreeSpatialGrid.cpp:160-185).  With CHECK, first verifies that the position lies STRICTLY
    // inside the box -- then no other leaf's closed box contains it, and both the reference's neighbour-list scan
    // and its top-down search end in this leaf; returns false (w untouched) otherwise.
    template<bool CHECK>
    __device__ __forceinline__ bool treeEnter(const char* leaves, const GridLds& L, Walk& w, int m)
    {
        const uint4 h = *reinterpret_cast<const uint4*>(leaves + ((uint32_t)m << 4));  // LeafRec: box code, density
        uint32_t ox, oy, oz, e;
        decodeBoxWords(h.x, h.y, L.stride, ox, oy, oz, e);
        const uint32_t szb = 8u << e;
        const double X0 = tabAt(L.gtab, ox), X1 = tabAt(L.gtab, ox + szb);
        const double Y0 = tabAt(L.gtab, oy), Y1 = tabAt(L.gtab, oy + szb);
        const double Z0 = tabAt(L.gtab, oz), Z1 = tabAt(L.gtab, oz + szb);
        const double rx = w.rx, ry = w.ry, rz = w.rz;
        if (CHECK)
        {
            const bool inside = rx > X0 && rx < X1 && ry > Y0 && ry < Y1 && rz > Z0 && rz < Z1;
            if (!inside) return false;
        }
        const bool nx = w.kx < 0.0, ny = w.ky < 0.0, nz = w.kz < 0.0;
        double ds;
        int ax;
        exitDistance<false>(w, nx ? X0 : X1, ny ? Y0 : Y1, nz ? Z0 : Z1, ds, ax);
        w.ds = ds;
        w.axis = ax;
        w.e = e;
        w.P = (uint64_t)(ox >> 3) | ((uint64_t)((oy - L.stride) >> 3) << L.fieldBits) | ((uint64_t)((oz - 2u * L.stride) >> 3) << (2u * L.fieldBits));
        w.cell = m;
        w.dens = __longlong_as_double(((long long)h.w << 32) | h.z);
        return true;
    }

    enum LaneState : int
    {
        ST_ACTIVE = 0,  // a pending segment is ready
        ST_HIT = 1,     // the stop condition holds in the pending segment (not yet added)
        ST_SLOW = 2,    // position advanced, next cell undecided: literal algorithm wanted
        ST_EXIT = 3,    // the path has left the grid
        ST_IDLE = 4,    // no walk
        ST_EDGE = 5,    // position advanced through a wall on the grid boundary: exit, unless rounding kept it inside
        ST_FIRST = 6    // (Voronoi) a walk in its first cell, whose exit the next step finds (the walk kernels; never seen by a service round)
    };

    // scene scalars of the fast step (wave-uniform; hoisted out of the hot loop)
    struct TreeConst
    {
        double gx0, gy0, gz0;  // lower corner of the root box
        double gx1, gy1, gz1;  // upper corner
        double sx8, sy8, sz8;  // 8 x finest-level cells per unit length: position -> 8 x fine cell index (a table byte offset)
        double bx8, by8, bz8;  // 8 x (-lower corner * cells per unit length)
        uint32_t stride;       // bytes per axis of the coordinate table
        const char* gtab;      // the coordinate table in global memory if it does not fit in LDS (levels 13-15), else null
        const char* cellTab;   // DevScene::cell_tab
        uint32_t numCells;
    };

    // TreeSpatialGrid.cpp:192-207, literally, from the advanced position: neighbour list of the old cell, top-down
    // search, next-after escape.  Returns false when the path leaves the grid (State::Outside).
    __device__ __forceinline__ bool treeStepSlow(const DevScene& S, const GridLds& L, Walk& w)
    {
        const int old = w.cell;
        const int wall = 2 * w.axis + (((w.sgn >> w.axis) & 1u) ? 0 : 1);
        int next = listNeighbor(S, L, old, wall, w.rx, w.ry, w.rz);
        if (next < 0) next = topDown(S, L, w.rx, w.ry, w.rz);
        if (next == old)
        {
            // PathSegmentGenerator::propagateToNextAfter (PathSegmentGenerator.hpp:148-153)
            w.rx = nextAfterToward(w.rx, w.kx < 0.);
            w.ry = nextAfterToward(w.ry, w.ky < 0.);
            w.rz = nextAfterToward(w.rz, w.kz < 0.);
            next = topDown(S, L, w.rx, w.ry, w.rz);
        }
        if (next < 0 || next == old) return false;
        treeEnter<false>(reinterpret_cast<const char*>(S.leaves), L, w, next);
        return true;
    }

    // ------------------------------------------------------------------------------------------------
    // Cartesian helpers (CartesianSpatialGrid.cpp:87-163)

    __device__ __forceinline__ void cartEnter(const DevScene& S, const GridLds& L, Walk& w)
    {
        const double* xv = L.grid;
        const double* yv = L.grid + (S.nx + 1);
        const double* zv = yv + (S.ny + 1);
        const int m = w.ck + S.nz * w.cj + S.nz * S.ny * w.ci;
        const double xE = (w.kx < 0.0) ? xv[w.ci] : xv[w.ci + 1];
        const double yE = (w.ky < 0.0) ? yv[w.cj] : yv[w.cj + 1];
        const double zE = (w.kz < 0.0) ? zv[w.ck] : zv[w.ck + 1];
        double ds;
        int ax;
        exitDistance<true>(w, xE, yE, zE, ds, ax);
        w.ds = ds;
        w.axis = ax;
        w.cell = m;
        w.dens = S.cell_density[m];
    }
    __device__ __forceinline__ bool cartAdvance(const DevScene& S, const GridLds& L, Walk& w)
    {
        const double* xv = L.grid;
        const double* yv = L.grid + (S.nx + 1);
        const double* zv = yv + (S.ny + 1);
        const double ds = w.ds;
        bool inside = true;
        if (w.axis == 0)
        {
            w.rx = (w.kx < 0.0) ? xv[w.ci] : xv[w.ci + 1];
            w.ry += w.ky * ds;
            w.rz += w.kz * ds;
            w.ci += (w.kx < 0.0) ? -1 : 1;
            if (w.ci >= S.nx || w.ci < 0) inside = false;
        }
        else if (w.axis == 1)
        {
            w.ry = (w.ky < 0.0) ? yv[w.cj] : yv[w.cj + 1];
            w.rx += w.kx * ds;
            w.rz += w.kz * ds;
            w.cj += (w.ky < 0.0) ? -1 : 1;
            if (w.cj >= S.ny || w.cj < 0) inside = false;
        }
        else
        {
            w.rz = (w.kz < 0.0) ? zv[w.ck] : zv[w.ck + 1];
            w.rx += w.kx * ds;
            w.ry += w.ky * ds;
            w.ck += (w.kz < 0.0) ? -1 : 1;
            if (w.ck >= S.nz || w.ck < 0) inside = false;
        }
        if (!inside) return false;
        cartEnter(S, L, w);
        return true;
    }

#include "pmc_walk_voro.inc"
#include "pmc_walk_bin.inc"

    // ------------------------------------------------------------------------------------------------
    // PathSegmentGenerator::moveInside (PathSegmentGenerator.cpp:11-112); returns false if the path misses the grid;
    // cumds receives the length of the initial segment outside the grid
    __device__ __forceinline__ bool moveInside(const DevScene& S, Walk& w, double& cumds)
    {
        const double eps = S.eps;
        cumds = 0.;
        if (w.rx <= S.gx0)
        {
            if (w.kx <= 0.0) return false;
            double d = (S.gx0 - w.rx) / w.kx;
            w.rx = S.gx0 + eps;
            w.ry += w.ky * d;
            w.rz += w.kz * d;
            cumds += d;
        }
        else if (w.rx >= S.gx1)
        {
            if (w.kx >= 0.0) return false;
            double d = (S.gx1 - w.rx) / w.kx;
            w.rx = S.gx1 - eps;
            w.ry += w.ky * d;
            w.rz += w.kz * d;
            cumds += d;
        }
        if (w.ry <= S.gy0)
        {
            if (w.ky <= 0.0) return false;
            double d = (S.gy0 - w.ry) / w.ky;
            w.rx += w.kx * d;
            w.ry = S.gy0 + eps;
            w.rz += w.kz * d;
            cumds += d;
        }
        else if (w.ry >= S.gy1)
        {
            if (w.ky >= 0.0) return false;
            double d = (S.gy1 - w.ry) / w.ky;
            w.rx += w.kx * d;
            w.ry = S.gy1 - eps;
            w.rz += w.kz * d;
            cumds += d;
        }
        if (w.rz <= S.gz0)
        {
            if (w.kz <= 0.0) return false;
            double d = (S.gz0 - w.rz) / w.kz;
            w.rx += w.kx * d;
            w.ry += w.ky * d;
            w.rz = S.gz0 + eps;
            cumds += d;
        }
        else if (w.rz >= S.gz1)
        {
            if (w.kz >= 0.0) return false;
            double d = (S.gz1 - w.rz) / w.kz;
            w.rx += w.kx * d;
            w.ry += w.ky * d;
            w.rz = S.gz1 - eps;
            cumds += d;
        }
        if (!(w.rx >= S.gx0 && w.rx <= S.gx1 && w.ry >= S.gy0 && w.ry <= S.gy1 && w.rz >= S.gz0 && w.rz <= S.gz1))
            return false;
        return true;
    }

    // start of a walk from (r, k): State::Unknown branch of next().  hint = a leaf that probably contains r
    // (octree only).  Returns false if the path has no cell segments at all; the initial outside segment, if any,
    // has been added to w.s.  located receives the start cell if the start position itself lies inside the grid.
    template<int GRID>
    __device__ __forceinline__ bool startWalk(const DevScene& S, const GridLds& L, Walk& w, int hint, int& located, bool deferScan = false)
    {
        w.tau = 0.;
        w.s = 0.;
        w.lastm = -1;
        located = -1;
        double cumds;
        if (!moveInside(S, w, cumds)) return false;
        if (cumds > 0.) w.s += cumds;  // SpatialGridPath::addSegment(-1, cumds)
        if (GRID == GRID_CART)
        {
            w.ci = locateClip(L.grid, S.nx + 1, w.rx);
            w.cj = locateClip(L.grid + (S.nx + 1), S.ny + 1, w.ry);
            w.ck = locateClip(L.grid + (S.nx + 1) + (S.ny + 1), S.nz + 1, w.rz);
            cartEnter(S, L, w);
            return true;
        }
        else if (GRID == GRID_VORO)
        {
            // (hint: VoronoiMeshSnapshot::cellIndex of the start position, valid if moveInside left the position alone)
            if (deferScan)
            {
                // the walk's kernel scans the first cell like every other one (voroPeelKernel): the cell only
                const int m = (hint >= 0 && cumds == 0.) ? hint : voroCellIndex(S, w.rx, w.ry, w.rz);
                if (m < 0) return false;
                w.cell = m;
                w.ds = 0.;
                w.ci = PMC_VORO_FIRST_SCAN;
                return true;
            }
            return voroLocateAndEnter(S, w, (hint >= 0 && cumds == 0.) ? hint : -2);
        }
        else if (GRID == GRID_BIN)
        {
            // (moveInside guarantees that r is inside the closed root box: the search finds a leaf)
            binStart(S, w, hint);
            if (cumds == 0.) located = w.cell;
            return true;
        }
        else
        {
            const char* leaves = reinterpret_cast<const char*>(S.leaves);
            // strictly inside the hinted leaf => the top-down search would end there as well
            bool entered = false;
            if (hint >= 0) entered = treeEnter<true>(leaves, L, w, hint);
            if (!entered)
            {
                // (moveInside guarantees that r is inside the root box, so m >= 0)
                const int m = topDown(S, L, w.rx, w.ry, w.rz);
                treeEnter<false>(leaves, L, w, m);
            }
            if (cumds == 0.) located = w.cell;
            return true;
        }
    }

    template<int GRID> __device__ __forceinline__ void stageGrid(const DevScene& S, double* g, int tid, int nthreads)
    {
        if (GRID == GRID_TREE)
        {
            const int ngrid = S.tab_in_lds ? 3 * ((1 << S.lmax) + 1) : 0;
            for (int i = tid; i < ngrid; i += nthreads) g[i] = S.coord_tab[i];
        }
        else if (GRID == GRID_CART)
        {
            for (int i = tid; i <= S.nx; i += nthreads) g[i] = S.xv[i];
            for (int i = tid; i <= S.ny; i += nthreads) g[(S.nx + 1) + i] = S.yv[i];
            for (int i = tid; i <= S.nz; i += nthreads) g[(S.nx + 1) + (S.ny + 1) + i] = S.zv[i];
        }
    }

    // ================================================================================================
    //  walk kernel
    // ================================================================================================

    // loads the start state of the walk in task record t (pmc_device.h TaskArrays; all loads independent); returns the
    // record's bits word (PMC_TASK_NONE: no walk)
    template<int GRID>
    __device__ __forceinline__ uint32_t loadTask(const DevScene& S, int64_t t, Walk& w, double& target)
    {
        const TaskArrays& K = S.tasks;
        const uint32_t bits = K.bits[t];
        // (a record is also read for a slot that turns out to have no walk -- bits == PMC_TASK_NONE --, and nothing but its flags has been written
        // then: the density gather below must not follow whatever the cell word holds)
        w.cell = bits != PMC_TASK_NONE ? K.cell[t] : 0;
        w.rx = K.rx[t], w.ry = K.ry[t], w.rz = K.rz[t];
        const double kx = K.kx[t], ky = K.ky[t], kz = K.kz[t];
        w.s = K.s0[t];
        w.ds = K.ds[t];
        target = K.target[t];
        // (RN(1/k) is formed again here, as the cycle start kernel formed it: a record does not carry it)
        setDirection(w, kx, ky, kz);
        if (GRID == GRID_CART)
        {
            // the cell's indices from its number m = k + nz j + nz ny i (CartesianSpatialGrid.cpp:19-24): any number of cells per axis
            const int q = w.cell / S.nz;
            w.ck = w.cell - q * S.nz;
            w.ci = q / S.ny;
            w.cj = q - w.ci * S.ny;
            w.dens = S.cell_density[w.cell];
        }
        if (GRID == GRID_VORO)
        {
            w.ci = K.cijk[t];  // the neighbour (or wall) through which the path leaves the first cell
            w.cj = -1;         // (its run in an observer's table: not known yet, voroAdvance)
            w.dens = S.vsite[4 * (int64_t)w.cell + 3];
        }
        w.axis = (bits >> 2) & 3u;
        if (GRID == GRID_BIN)
        {
            // the cell's density and its link through the exit wall of the first segment (the sign bit of the exit axis is in the record)
            const BinCellRec* rec = S.bin_cells + w.cell;
            w.dens = rec->density;
            w.ci = rec->link[2 * w.axis + (((bits >> (4 + w.axis)) & 1u) ? 0 : 1)];
        }
        w.sgn = (bits >> 4) & 7u;
        w.tau = 0.;
        w.lastm = -1;
        return bits;
    }

    // several medium components (DevScene::num_media > 1): the cross sections of component h at the wavelength of the slot's history
    __device__ __forceinline__ void mediumSections(const DevScene& S, const SlotArrays& A, int slot, int h, double& ext, double& sca, double& absn)
    {
        const DevMedium& M = S.med[h];
        if (S.mono)
            ext = M.mono_ext, sca = M.mono_sca, absn = M.mono_abs;
        else
        {
            const int il = A.dustIdx[(int64_t)h * A.num_slots + slot];
            ext = M.sigma_ext[il], sca = M.sigma_sca[il], absn = M.sigma_abs[il];
        }
    }
    // the optical depth(s) at the end of a segment of length ds through `cell` (device index; `dens` = density of component 0 there)
    // from those at its start, summed over the components in order: MediumSystem.cpp:880-885 / 1228-1238 (extinction: sigma n ds),
    // :944-951 / 1133-1140 (scattering and absorption apart: n ds first)
    template<bool EA>
    __device__ __forceinline__ void mediaSegment(const DevScene& S, int cell, double dens, double ds, bool apart, const double* mx, const double* ms,
                                                 const double* ma, double& tau, double& tabs)
    {
        for (int h = 0; h < S.num_media; ++h)
        {
            const double n = h == 0 ? dens : S.med[h].density[cell];
            if (EA && apart)
            {
                const double ns = n * ds;
                tau += ms[h] * ns;
                tabs += ma[h] * ns;
            }
            else
                tau += mx[h] * n * ds;
        }
    }

    // the interaction optical depth of simulateForcedPropagation (MonteCarloSimulation.cpp:709-722) from the uniforms the
    // transition kernel drew for it (startCycle): `uniform() < xi` picks the uniform or the exponential deviate
    // (Random::exponCutoff, Random.cpp:105-116; a rejection round, which only rounding can cause, continues the slot's
    // stream).  Stores tau_path and the sampled depth for the weights applied in onCycleDone.
    __device__ __forceinline__ double sampleForcedDepth(const DevScene& S, const SlotArrays& A, int slot, uint64_t seed, double taupath,
                                                        double u1, double u2)
    {
        const double xi = S.path_length_bias;
        double tau;
        if (xi != 0. && u1 < xi)
            tau = u2 * taupath;
        else if (taupath < 1e-10)
            tau = u2 * taupath;
        else
        {
            tau = -log(1.0 - u2 * (1.0 - exp(-taupath)));
            if (tau > taupath)
            {
                Rng rng;
                loadRng(A, slot, rng);
                while (tau > taupath) tau = -log(1.0 - rngUniform(rng, seed) * (1.0 - exp(-taupath)));
                storeRng(A, slot, rng);
            }
        }
        A.taupath[slot] = taupath;
        A.tausample[slot] = tau;
        return tau;
    }

    // The pass-1 checkpoints of the propagation kernels (walkPropKernel, pmc_walk_tree.inc, with the derivation; voroPropKernel,
    // pmc_walk_voro_run.inc): the decisions.  A kernel keeps two saved walker states of its own layout, A (certainly at or before the
    // interaction point) and B (a later candidate), and one word of flags: CK_SEL the buffer that holds B (A is in the other one),
    // CK_HASA / CK_HASB, CK_LIN the branch of sampleForcedDepth that the path's uniforms take (the sampled depth is u2 * tau_path).
    constexpr uint32_t CK_SEL = 1u, CK_HASA = 2u, CK_HASB = 4u, CK_LIN = 8u;
    // the flags of a new path: no checkpoint yet
    __device__ __forceinline__ uint32_t ckptStart(const DevScene& S, double u1) { return (S.path_length_bias != 0. && u1 < S.path_length_bias) ? CK_LIN : 0u; }
    // the tick of a pass-1 walk at depth tau > 0: true if the caller is to save its current state, as the new B, in buffer ck & CK_SEL (after the call).
    // Without a B that is the first one; with one, B is certain once the lower bound of the sampled depth has passed its depth tauB, and becomes A.
    __device__ __forceinline__ bool ckptTick(uint32_t& ck, double tau, double tauB, double u2)
    {
        if (ck & CK_HASB)
        {
            const double bound = u2 * tau;
            const double need = (ck & CK_LIN) ? tauB : tauB * (1. + tau) * (1. + 1e-13);
            if (!(bound >= need)) return false;
            ck = (ck ^ CK_SEL) | CK_HASA;
        }
        ck |= CK_HASB;
        return true;
    }
    // the buffer pass 2 resumes from once the depth `target` has been sampled: the later state that lies at or before the interaction point
    // (B is a candidate; A is certain but for a sampled depth that a rejection round has redrawn: checked as well), or -1: from the start
    __device__ __forceinline__ int ckptResume(uint32_t ck, double tauA, double tauB, double target)
    {
        if ((ck & CK_HASB) && tauB <= target) return (int)(ck & CK_SEL);
        if ((ck & CK_HASA) && tauA <= target) return (int)((ck & CK_SEL) ^ 1u);
        return -1;
    }

    // SpecialFunctions::lnmean(x1, x2, lnx1, lnx2) (SKIRT/utils/SpecialFunctions.cpp:860-880)
    __device__ __forceinline__ double lnmean(double x1, double x2, double lnx1, double lnx2)
    {
        if (x1 > x2)
        {
            double t = x1;
            x1 = x2, x2 = t;
            t = lnx1;
            lnx1 = lnx2, lnx2 = t;
        }
        if (x1 <= 0) return 0.;
        double x = x2 / x1 - 1.;
        if (x < 1e-3)
            return x1
                   / (1. - 1. / 2. * x + 1. / 3. * x * x - 1. / 4. * x * x * x + 1. / 5. * x * x * x * x - 1. / 6. * x * x * x * x * x);
        return (x2 - x1) / (lnx2 - lnx1);
    }

    // ------------------------------------------------------------------------------------------------
    // what the walk kernels share: the reference's semantics of a segment, of the end of a walk and of its start, and the claiming of tasks

    // the cross sections of the walk of `slot` at its packet's wavelength: extinction; EA scattering and absorption (the absorption depth
    // starts from 0); MM each component's
    template<bool EA, bool MM>
    __device__ __forceinline__ void loadSections(const DevScene& S, const SlotArrays& A, int slot, double& sext, double& ssca, double& sabs, double& tabs,
                                                 double* mx, double* msc, double* mab)
    {
        sext = S.mono ? S.mono_ext : A.dustExt[slot];
        if (EA)
        {
            ssca = S.mono ? S.mono_sca : A.dustSca[slot];
            sabs = S.mono ? S.mono_abs : A.dustAbs[slot];
            tabs = 0.;
        }
        if (MM)
            for (int h = 0; h < S.num_media; ++h) mediumSections(S, A, slot, h, mx[h], msc[h], mab[h]);
    }
    // (RF) a pass-1 walk starts: the packet's luminosity (PhotonPacket::luminosity()) and wavelength bin on this path
    // (MonteCarloSimulation.cpp:638-662), no extinction before its first segment
    __device__ __forceinline__ void rfStart(const DevScene& S, const SlotArrays& A, int slot, double& rfL, int& rfEll, double& rfExtBeg)
    {
        rfL = A.W[slot] / (S.mono ? S.mono_lambda : A.lambda[slot]);
        rfEll = A.rfell[slot];
        rfExtBeg = 1.;
    }

    // the optical depth(s) at the end of the pending segment (length ds through `cell`, density `dens`) from those at its start:
    // MediumSystem.cpp:863-871 (sigma n ds); `apart` (EA: a walk that sums scattering and absorption depths apart) :920-926 (n ds first,
    // then the two cross sections), non-forced :1099 (sigma_sca n ds); MM: mediaSegment
    template<bool EA, bool MM>
    __device__ __forceinline__ void segmentDepth(const DevScene& S, int cell, double dens, double ds, double tau, double tabs, bool apart, bool force,
                                                 double sext, double ssca, double sabs, const double* mx, const double* msc, const double* mab,
                                                 double& tau1, double& tabs1)
    {
        tau1 = tau + sext * dens * ds;
        tabs1 = 0.;
        if (MM)
        {
            tau1 = tau, tabs1 = tabs;
            mediaSegment<EA>(S, cell, dens, ds, apart, mx, msc, mab, tau1, tabs1);
        }
        else if (EA && apart)
        {
            const double ns = dens * ds;
            tau1 = force ? tau + ssca * ns : tau + ssca * dens * ds;
            tabs1 = tabs + sabs * ns;
        }
    }

    // (RF) the radiation-field contribution of a pass-1 segment of length ds > 0 (MonteCarloSimulation.cpp:648-661): L lnmean(e^-tau1, e^-tau0) ds
    // into rf1(m, ell), tau = Segment::tauExt() (SpatialGridPath.hpp:108: scattering + absorption depth in the explicit-absorption cycle);
    // extEnd = e^-tau1, the factor at the start of the next segment
    template<bool EA>
    __device__ __forceinline__ double rfSegment(double rfL, double rfExtBeg, double tau0, double tabs0, double tau1, double tabs1, double ds, double& extEnd)
    {
        const double lnExtEnd = EA ? -(tau1 + tabs1) : -tau1;
        extEnd = exp(lnExtEnd);
        return rfL * lnmean(extEnd, rfExtBeg, lnExtEnd, EA ? -(tau0 + tabs0) : -tau0) * ds;
    }

    // findInteractionPoint (SpatialGridPath.cpp:177-196) in the segment in which the walk stops, the first one with tau > target: its cell,
    // the distance interpolated in it, and the density there -- EA: the absorption depth at the point instead, interpolated like the distance
    // when the path was stored, or tau_sca x sigma_abs / sigma_sca in the non-forced walk (MediumSystem.cpp:1105-1106); several components:
    // interpolated in both cycles (MediumSystem.cpp:1147-1149).  The segment's depths are formed again from its start.
    template<bool EA, bool MM>
    __device__ __forceinline__ void storeInteraction(const DevScene& S, const SlotArrays& A, int slot, int cell, double dens, double ds, double s,
                                                     double tau, double tabs, double target, bool force, double sext, double ssca, double sabs,
                                                     const double* mx, const double* msc, const double* mab)
    {
        double tau1, tabs1;
        segmentDepth<EA, MM>(S, cell, dens, ds, tau, tabs, true, force, sext, ssca, sabs, mx, msc, mab, tau1, tabs1);
        const double f = (target - tau) / (tau1 - tau);
        A.mint[slot] = cell;
        A.sint[slot] = s + f * ((s + ds) - s);
        A.nint[slot] = EA && (MM || force) ? tabs + f * (tabs1 - tabs) : EA ? target * sabs / ssca : dens;
    }

    // the end of a pass-2 or non-forced walk that has not stopped in a segment: the interaction point beyond the last segment
    // (SpatialGridPath.cpp:198-204; `density(m)`: the grid's density of cell m), or none (non-forced: the packet escapes)
    template<bool EA, typename Density>
    __device__ __forceinline__ void storeWalkEnd(const SlotArrays& A, int slot, bool force, int lastm, double s, double tabs, Density density)
    {
        if (force && lastm >= 0)
        {
            A.mint[slot] = lastm;
            A.sint[slot] = s;
            A.nint[slot] = EA ? tabs : density(lastm);
        }
        else
            A.mint[slot] = -1;
    }

    // new tasks for the lanes of `want` from a wave-local pool that is refilled `chunk` tasks (a sparse generation's list of live slots: 64)
    // at a time from the cursor S.counters[cursor] (one device-scope atomic per chunk: a single word saturates near 90 returning atomics per
    // microsecond); returns the task index of this lane or -1
    __device__ __forceinline__ int claimSlots(const DevScene& S, int cursor, unsigned long long numTasks, int lane, bool want,
                                              unsigned long long& poolNext, unsigned long long& poolEnd, bool& exhausted,
                                              unsigned long long chunk = PMC_TASK_CHUNK)
    {
        const unsigned long long idle = __ballot(want);
        const int nidle = __popcll(idle);
        if (!nidle || exhausted) return -1;
        if (poolNext >= poolEnd)
        {
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(S.counters + cursor, chunk);
            got = __shfl(got, 0, 64);
            poolNext = got;
            poolEnd = got + chunk;
            if (poolEnd > numTasks) poolEnd = numTasks;
            if (poolNext >= poolEnd)
            {
                poolNext = poolEnd = 0;
                exhausted = true;
                return -1;
            }
        }
        const unsigned long long base = poolNext;
        const unsigned long long avail = poolEnd - poolNext;
        poolNext += (unsigned long long)nidle < avail ? (unsigned long long)nidle : avail;
        if (!want) return -1;
        const unsigned long long rank = __popcll(idle & ((1ull << lane) - 1ull));
        return rank < avail ? (int)(base + rank) : -1;
    }

    // the XCD this wave runs on (0-7): a hint for locality only, nothing depends on it for correctness
    __device__ __forceinline__ uint32_t xccId()
    {
        uint32_t v;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
        return v & 7u;
    }
    // claimSlots over a task range cut into eight segments with a cursor each: a wave takes chunks from segment `seg` (its XCD's to begin
    // with) until that is used up, then moves on to the next one; all eight used up: exhausted (the L2 of an XCD sees an eighth of the
    // cells the walks in flight run through)
    __device__ __forceinline__ int claimSegmented(unsigned long long* cursors, unsigned long long numTasks, int lane, bool want, unsigned long long& poolNext,
                                                  unsigned long long& poolEnd, bool& exhausted, uint32_t& seg, uint32_t& tried)
    {
        const unsigned long long idle = __ballot(want);
        const int nidle = __popcll(idle);
        if (!nidle || exhausted) return -1;
        while (poolNext >= poolEnd)
        {
            if (tried >= 8u)
            {
                poolNext = poolEnd = 0;
                exhausted = true;
                return -1;
            }
            const unsigned long long lo = (numTasks * seg) >> 3, hi = (numTasks * (seg + 1u)) >> 3;
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(cursors + seg, (unsigned long long)PMC_TASK_CHUNK);
            got = __shfl(got, 0, 64);
            if (lo + got < hi)
            {
                poolNext = lo + got;
                poolEnd = lo + got + PMC_TASK_CHUNK < hi ? lo + got + PMC_TASK_CHUNK : hi;
            }
            else
            {
                seg = (seg + 1u) & 7u;
                tried += 1u;
            }
        }
        const unsigned long long base = poolNext;
        const unsigned long long avail = poolEnd - poolNext;
        poolNext += (unsigned long long)nidle < avail ? (unsigned long long)nidle : avail;
        if (!want) return -1;
        const unsigned long long rank = __popcll(idle & ((1ull << lane) - 1ull));
        return rank < avail ? (int)(base + rank) : -1;
    }

    // the wave's walk counters at the end of a walk kernel: pass-2 paths, visits, re-walked segments (DevScene::counters 1, 2, 6)
    __device__ __forceinline__ void flushWalkCounters(const DevScene& S, int lane, uint32_t paths, uint32_t visits, uint32_t rewalks)
    {
        unsigned long long v;
        v = waveSum(paths);
        if (lane == 0 && v) atomicAdd(S.counters + 1, v);
        v = waveSum(visits);
        if (lane == 0 && v) atomicAdd(S.counters + 2, v);
        v = waveSum(rewalks);
        if (lane == 0 && v) atomicAdd(S.counters + 6, v);
    }

    // Generic walk kernel of the Cartesian, Voronoi and binary-tree grids (the octree has its own kernels, pmc_walk_tree.inc): persistent
    // wavefronts, one walk per lane; a lane runs the task records of a slot one after the other (record 0: propagation
    // walk, continued from pass 1 into pass 2; record 1 + g: peel-off walk towards observer g).
    // RF: the forced-scattering path walk (pass 1) also stores the radiation field (MonteCarloSimulation.cpp:638-662)
    // EA: the explicit-absorption photon cycle (PhotonPacketOptions::explicitAbsorption): the propagation walk sums scattering and
    // absorption optical depths apart (MediumSystem::setScatteringAndAbsorptionOpticalDepths, MediumSystem.cpp:905-932; non-forced:
    // setInteractionPointUsingScatteringAndAbsorption, :1075-1110), the interaction is sampled on the scattering depth, and the absorption
    // depth at the interaction point travels to the transition kernel in SlotArrays::nint (the albedo is not used in that cycle)
    // MM: several medium components (DevScene::num_media > 1): a segment's optical depth is summed over the components in order, the
    // densities of components 1.. are read from their own arrays where the segment is added
    template<int GRID, bool RF, bool EA, bool MM>
    __global__ __launch_bounds__(256, PMC_WALK_MIN_WAVES) void walkKernel(const int sceneSlot, const int taskBase, const int numTaskRecords,
                                                      const int taskCounter, const uint64_t seed, const WalkStreamArgs stream)
    {
        static_assert(GRID != GRID_TREE, "the octree walks run in walkPeelKernel / walkPropKernel");
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        stageGrid<GRID>(S, lds, tid, blockDim.x);
        __syncthreads();
        const GridLds L = makeGridLds(S, lds);
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        // (a stream of single walks: the group's slots for their propagation walks, then every sorted observer's list for its peel-off walks)
        unsigned long long listCount[PMC_SORT_OBS] = {0ull, 0ull, 0ull, 0ull};
        // (the propagation walks: the group's slots in slot order, or -- sorted -- the list of the slots that have one)
        const unsigned long long numProp = stream.propList ? *stream.propCount : (unsigned long long)numTaskRecords;
        unsigned long long numTasks = numProp;
        for (int k = 0; k < stream.numLists; ++k)
        {
            listCount[k] = *stream.count[k];
            numTasks += listCount[k];
        }
        const int numRecords = 1 + S.num_instruments;                              // task records per slot
        const bool force = S.force_scattering != 0;

        Walk w;
        w.cell = -1;
        w.ds = 0.;
        int slot = -1;
        int st = ST_IDLE;
        int mode = MODE_NONE;
        double sext = 0., target = 0.;
        double ssca = 0., sabs = 0., tabs = 0.;  // (EA) cross sections of the propagation walk, cumulative absorption optical depth
        double mx[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, msc[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, mab[PMC_MAX_MEDIA] = {0., 0., 0., 0.};  // (MM) per component
        uint32_t nseg = 0;  // segments of the current walk that the reference adds to its path
        int rec = 0;        // task record of the slot that the lane is walking (0: propagation, 1 + g: peel-off)
        int vtab = -1;      // (Voronoi) table of the observer of the lane's peel-off walk (DevScene::vobs_*), or -1
        int streamRec = 0;  // (task stream) the record of the task the lane has just taken
        uint32_t xcdSeg = xccId(), xcdTried = 0u;  // (task stream) the eighth of the stream this wave takes its tasks from (its XCD's to begin with)
        uint32_t todoRecs = 0;  // records of the slot that are still to be walked (bit r: record r)
        uint32_t visits = 0, rewalks = 0, paths = 0;
        // radiation field (RF only): luminosity of the packet on this path, its wavelength bin, and the extinction
        // factor at the start of the pending segment
        double rfL = 0., rfExtBeg = 1.;
        int rfEll = -1;
        bool exhausted = false;
        unsigned long long poolNext = 0, poolEnd = 0;  // wave-uniform

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            const int nactive = __popcll(activeMask);
            if (exhausted && !activeMask && !pendingMask) break;
            // ---------------- service: undecided steps, finished walks, refill.  Runs when enough lanes wait for it;
            // once the task list is exhausted idle lanes cannot be refilled and pending lanes are served at once
            const bool service = exhausted ? (pendingMask != 0ull) : (64 - nactive >= PMC_WALK_REFILL);
            if (service)
            {
                if (GRID == GRID_VORO && st == ST_SLOW) st = voroStepSlow(S, w) ? ST_ACTIVE : ST_EXIT;
                if (GRID == GRID_BIN && st == ST_SLOW) st = binStepSlow(S, w) ? ST_ACTIVE : ST_EXIT;
                // ---- finished walks: results (stores only), and what the lane does next:
                //      again: pass 1 ended with tau_path > 0 -> pass 2 over the same path (record 0 again)
                //      chain: the slot has another record of this cycle -> that walk
                //      else the lane is idle and takes a new slot from the pool
                bool again = false;
                double taupath = 0.;
                if (st != ST_ACTIVE && st != ST_IDLE)
                {
                    if (st == ST_HIT)
                    {
                        nseg += 1;  // the segment in which the walk stops
                        if (mode == MODE_PEEL)
                            A.ptau[(int64_t)(rec - 1) * A.num_slots + slot] = INFINITY;  // tau >= taumax (MediumSystem.cpp:1215-1218)
                        else
                            storeInteraction<EA, MM>(S, A, slot, w.cell, w.dens, w.ds, w.s, w.tau, tabs, target, force, sext, ssca, sabs, mx, msc, mab);
                    }
                    else if (mode == MODE_PASS1 && w.tau > 0.)
                    {
                        again = true;
                        taupath = w.tau;
                    }
                    else if (mode == MODE_PEEL)
                        A.ptau[(int64_t)(rec - 1) * A.num_slots + slot] = w.tau;
                    else if (mode == MODE_PASS1)
                        A.mint[slot] = -1;  // tau_path <= 0: the packet cannot scatter, the history ends
                    else
                        storeWalkEnd<EA>(A, slot, force, w.lastm, w.s, tabs,
                                         [&](int m) { return GRID == GRID_VORO ? S.vsite[4 * (int64_t)m + 3] : S.cell_density[m]; });
                    if (mode == MODE_PASS2 && force)
                        rewalks += nseg;
                    else
                        visits += nseg;
                    st = ST_IDLE;
                }
                const bool chain = st == ST_IDLE && !again && todoRecs != 0u;
                // ---- new tasks for the idle lanes: from the stream in eight segments with a cursor each, or from the one cursor
                const bool want = st == ST_IDLE && !again && !chain;
                const int got = stream.xcdCursor ? claimSegmented(stream.xcdCursor, numTasks, lane, want, poolNext, poolEnd, exhausted, xcdSeg,
                                                                  xcdTried)
                                                 : claimSlots(S, taskCounter, numTasks, lane, want, poolNext, poolEnd, exhausted);
                const bool refill = got >= 0;
                if (refill)
                {
                    unsigned long long j = (unsigned long long)got;
                    streamRec = 0;
                    if (j < numProp)
                        slot = stream.propList ? stream.propList[j] : taskBase + (int)j;
                    else
                    {
                        j -= numProp;
                        for (int k = 0; k < PMC_SORT_OBS; ++k)
                        {
                            if (k >= stream.numLists) break;
                            if (j < listCount[k])
                            {
                                slot = stream.list[k][j];
                                streamRec = stream.rec[k];
                                break;
                            }
                            j -= listCount[k];
                        }
                    }
                }
                // ---- ONE batch of loads for all three kinds of lanes: the start state in a task record (record 0 for
                // `again` and, speculatively, for a new slot; the next record of the cycle for `chain`), the random
                // stream of the `again` lanes, the record flags of a new slot
                if (chain)
                {
                    rec = __ffs((int)todoRecs) - 1;
                    todoRecs &= todoRecs - 1u;
                }
                if (again) rec = 0;
                if (refill) rec = streamRec;
                uint32_t bits = PMC_TASK_NONE;
                uint32_t have = 0;
                double recTarget = 0., u1 = 0., u2 = 0.;
                if (again || chain || refill)
                {
                    bits = loadTask<GRID>(S, (int64_t)rec * A.num_slots + slot, w, recTarget);
                    if (again)
                    {
                        // the uniforms drawn for this step by the transition kernel (see startCycle)
                        u1 = A.sint[slot];
                        u2 = A.nint[slot];
                    }
                    if (refill && stream.numLists > 0)
                        have = bits != PMC_TASK_NONE ? 1u << rec : 0u;  // (a task of the stream is one walk)
                    else if (refill)
                        for (int r = 0; r < numRecords; ++r)
                            if (K.bits[(int64_t)r * A.num_slots + slot] != PMC_TASK_NONE) have |= 1u << r;
                    loadSections<EA, MM>(S, A, slot, sext, ssca, sabs, tabs, mx, msc, mab);
                }
                if (again)
                {
                    // ---- simulateForcedPropagation between the two passes (MonteCarloSimulation.cpp:696-722): the whole
                    // path has been walked; the interaction optical depth follows from the pre-drawn uniforms, and the SAME
                    // path is walked again (its start state is still in record 0) up to that depth -- no generation boundary
                    // in between.  The path-length-bias weight follows in the transition kernel (onCycleDone).
                    target = sampleForcedDepth(S, A, slot, seed, taupath, u1, u2);
                    mode = MODE_PASS2;
                    nseg = 0;
                    paths += 1;
                    st = ST_ACTIVE;
                }
                else if (chain)
                {
                    mode = bits & 3u;
                    target = recTarget;
                    nseg = 0;
                    st = ST_ACTIVE;
                }
                else if (refill && have)
                {
                    todoRecs = have & (have - 1u);
                    if (!(have & 1u) && stream.numLists == 0)
                    {
                        // (rare: no propagation walk in this cycle) the first record that holds a walk
                        rec = __ffs((int)have) - 1;
                        bits = loadTask<GRID>(S, (int64_t)rec * A.num_slots + slot, w, recTarget);
                    }
                    mode = bits & 3u;
                    target = recTarget;
                    nseg = 0;
                    st = ST_ACTIVE;
                }
                // (Voronoi) a peel-off walk reads its observer's packed neighbour lists
                if (GRID == GRID_VORO) vtab = (st == ST_ACTIVE && mode == MODE_PEEL) ? (int)S.vobs_of_inst[rec - 1] : -1;
                if (RF && st == ST_ACTIVE && !again && (chain || refill) && mode == MODE_PASS1) rfStart(S, A, slot, rfL, rfEll, rfExtBeg);
                // (Voronoi) a walk whose first cell the cycle start kernel has located only: its first step finds the exit
                if (GRID == GRID_VORO && st == ST_ACTIVE && (again || chain || refill) && w.ci == PMC_VORO_FIRST_SCAN) st = ST_FIRST;
            }

            // ---------------- walk steps
#pragma unroll 1
            for (int it = 0; it < PMC_WALK_STEPS; ++it)
            {
                int enter = -1;
                if (st == ST_ACTIVE)
                {
                    // ---- the pending segment (m = w.cell, ds = w.ds): MediumSystem.cpp:863-871 (pass 1),
                    // SpatialGridPath.cpp:177-196 (pass 2: stop in the first segment with tau > target),
                    // MediumSystem.cpp:1207-1219 (peel-off: stop once tau >= taumax), :988-1008 (non-forced).
                    // A zero-length segment changes neither tau nor s, so it may be added unconditionally.
                    const double ds = w.ds;
                    double tau1, tabs1;
                    segmentDepth<EA, MM>(S, w.cell, w.dens, ds, w.tau, tabs, mode != MODE_PEEL, force, sext, ssca, sabs, mx, msc, mab, tau1, tabs1);
                    if (tau1 > target)
                        st = ST_HIT;
                    else
                    {
                        const double tau0 = w.tau;
                        const double tabs0 = tabs;
                        w.tau = tau1;
                        if (EA) tabs = tabs1;
                        w.s += ds;
                        // SpatialGridPath::addSegment keeps segments with ds > 0 only; the non-forced and the
                        // peel-off loops run over every segment the generator emits
                        if (ds > 0. || !force || mode == MODE_PEEL)
                        {
                            w.lastm = w.cell;
                            nseg += 1;
                        }
                        if (RF && mode == MODE_PASS1 && ds > 0.)
                        {
                            double extEnd;
                            const double rfValue = rfSegment<EA>(rfL, rfExtBeg, tau0, tabs0, tau1, tabs1, ds, extEnd);
                            // (binary tree: the table counts cells in the caller's numbering)
                            if (rfEll >= 0) unsafeAtomicAdd(S.rf + ((int64_t)(GRID == GRID_BIN ? S.cell_ext[w.cell] : w.cell) * S.rf_num_lambda + rfEll), rfValue);
                            rfExtBeg = extEnd;
                        }
                        if (GRID == GRID_VORO)
                        {
                            voroMove(S, w);
                            enter = w.ci;
                            if (enter < 0) st = ST_EXIT;
                        }
                        else if (GRID == GRID_BIN)
                            st = binAdvance(S, w);
                        else
                        {
                            if (!cartAdvance(S, L, w)) st = ST_EXIT;
                        }
                    }
                }
                // (Voronoi) the exit of the cell the walk has moved into -- or, for a walk in its first step, of the cell it starts in
                if (GRID == GRID_VORO)
                {
                    if (st == ST_FIRST) enter = w.cell;
                    if (enter >= 0) st = voroEnterNext(S, w, enter, vtab);
                }
            }
        }
        flushWalkCounters(S, lane, paths, visits, rewalks);
    }
