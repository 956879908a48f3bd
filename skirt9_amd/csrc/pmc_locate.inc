// pmc_locate.inc -- the cell of a position (included by pmc_kernels.hip inside its anonymous namespace, behind pmc_ray.inc): the point sampler of
// pmc_sample_cells, ProbeFormBridge::valuesAtPosition for the quantities that live on the grid.
//
// locateCellsKernel answers SpatialGrid::cellIndex(r) for one position per lane.  That is NOT the start of a walk: no moveInside, no direction,
// no epsilon shift -- a position on the boundary of the domain is inside, one next to it is outside, and a position on a wall between two
// cells belongs to the upper one.  Ties are the normal case for the callers (a cut through the origin of a symmetric grid lies on cell walls
// with every pixel), so each grid's rule is the reference's, literally:
//   octree        TreeNode::leafChild (TreeNode.cpp:66-76): null outside the closed root box, then r < centre ? lower : upper per axis and
//                 level (OctTreeNode.cpp:37-42) -- topDown (pmc_walk.inc)
//   binary tree   the same with BinTreeNode::child (BinTreeNode.cpp:53-62) -- binTopDown (pmc_walk_bin.inc), without binStart's hint
//   Cartesian     NR::locateFail per axis (CartesianSpatialGrid.cpp:60-69, NR.hpp:130-143, 186-191): -1 below the first and above the last
//                 border, the last border in the last bin.  (locateClip, which a walk starts with, puts an outside position in an outermost bin.)
//   Voronoi       VoronoiMeshSnapshot::cellIndex -- voroCellIndex (pmc_walk_voro.inc)
// gatherCellsKernel then reads the cell values at the located cells; nothing is computed with them.

    // NR::locateFail on the borders xv[n]
    __device__ __forceinline__ int locateFail(const double* xv, int n, double x)
    {
        if (x > xv[n - 1]) return -1;
        return locateBasic(xv, x, n - 1);
    }

    // SpatialGrid::cellIndex in the numbering the walk kernels use (octree, binary tree: device cells); -1 outside
    template<int GRID> __device__ __forceinline__ int locateCell(const DevScene& S, const GridLds& L, double x, double y, double z)
    {
        if constexpr (GRID == GRID_TREE)
            return topDown(S, L, x, y, z);
        else if constexpr (GRID == GRID_BIN)
            return binTopDown(S, x, y, z);
        else if constexpr (GRID == GRID_VORO)
            return voroCellIndex(S, x, y, z);
        else
        {
            const int i = locateFail(L.grid, S.nx + 1, x);
            const int j = locateFail(L.grid + (S.nx + 1), S.ny + 1, y);
            const int k = locateFail(L.grid + (S.nx + 1) + (S.ny + 1), S.nz + 1, z);
            return (i < 0 || j < 0 || k < 0) ? -1 : k + S.nz * j + S.nz * S.ny * i;
        }
    }

    struct LocateArgs
    {
        const double* positions;  // [numPoints][3]
        int32_t* walkCells;       // [numPoints]: the cell in the walk kernels' numbering (what gatherCellsKernel indexes q with), -1 outside
        int32_t* cells;           // [numPoints]: the cell in the caller's numbering (what pmc_trace_ray reports), -1 outside
        unsigned long long numPoints;
    };

    // one position per lane, grid-stride over the positions; the grid tables in LDS as in integrateRaysKernel
    template<int GRID, bool WIDE> __global__ __launch_bounds__(256) void locateCellsKernel(const int sceneSlot, const LocateArgs A)
    {
        static_assert(GRID == GRID_TREE || !WIDE, "only the octree has a wide form");
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        if (GRID == GRID_TREE) requireLdsBaseZero(lds);
        stageGrid<GRID>(S, lds, tid, blockDim.x);
        __syncthreads();
        GridLds L = makeGridLds(S, lds);
        if (GRID == GRID_TREE && !WIDE) L.gtab = nullptr;  // (octrees up to level 10 always have their table in LDS: the test folds away)
        constexpr bool RENUMBERED = GRID == GRID_TREE || GRID == GRID_BIN;
        const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
        for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + tid; p < A.numPoints; p += stride)
        {
            const double* r = A.positions + 3 * p;
            const int c = locateCell<GRID>(S, L, r[0], r[1], r[2]);
            A.walkCells[p] = c;
            A.cells[p] = (RENUMBERED && c >= 0) ? S.cell_ext[c] : c;
        }
    }

    // values[v][p] = q[cell of p][v], 0 outside: one pass of up to PMC_INTEGRATE_PASS_VALUES values over the cells located once.  q is laid out as
    // for integrateRaysKernel, [cell][PMC_INTEGRATE_PASS_VALUES] in the walk kernels' numbering; the stores of a wave are consecutive along p
    // ([numValues][numPoints] is the layout of the FITS cube).  The values are copied, never rounded.
    __global__ __launch_bounds__(256) void gatherCellsKernel(const int32_t* __restrict__ walkCells, const double* __restrict__ q, double* __restrict__ values,
                                                             const unsigned long long numPoints, const int numValues)
    {
        const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
        for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < numPoints; p += stride)
        {
            const int c = walkCells[p];
            double rec[PROBE_WIDTH];
#pragma unroll
            for (int v = 0; v < PROBE_WIDTH; ++v) rec[v] = c >= 0 ? q[(size_t)(uint32_t)c * PROBE_WIDTH + v] : 0.;
#pragma unroll
            for (int v = 0; v < PROBE_WIDTH; ++v)
                if (v < numValues) values[(size_t)v * numPoints + p] = rec[v];
        }
    }
