// pmc_probe.inc -- batched ray integrals (included by pmc_kernels.hip inside its anonymous namespace, behind the walk kernels).
//
// sums[i][v] = sum over the path of ray i of ds * q[v][m]: ProbeFormBridge::valuesAlongPath for the accumulated quantities
// (ProbeFormBridge.cpp:628-650, 707-725).  The traversal is the single-ray tracers' (traceRayKernel, traceTreeKernel: the same functions in
// the same order, so a ray's segments are pmc_trace_ray's bit for bit), run by every lane of a wave for a ray of its own: persistent waves take
// rays in chunks from a cursor, a lane whose ray has ended takes the next one (rays that miss the grid end at once), the products are added in
// path order without contraction.
//
// q is laid out for the step's gather: per pass of PMC_INTEGRATE_PASS_VALUES values one record [cell][PMC_INTEGRATE_PASS_VALUES] in the numbering
// the kernel walks in (octree, binary tree: device cells), rows beyond the caller's last value zero.  The sums of a pass are kept in registers.

    constexpr int PROBE_WIDTH = PMC_INTEGRATE_PASS_VALUES;
    constexpr unsigned long long PROBE_CHUNK = 64;  // rays a wave takes from the cursor at a time
    constexpr int PROBE_STEP_CAP = 100000;          // cell segments per ray (the guard of the single-ray tracers)
    // ProbeArgs::work
    constexpr int PROBE_WORK_CURSOR = 0, PROBE_WORK_CAPPED = 1, PROBE_WORK_LANE_STEPS = 2, PROBE_WORK_WAVE_STEPS = 3, PROBE_WORK_WORDS = 4;

    struct ProbeArgs
    {
        const double* origins;     // [numRays][3]
        const double* directions;  // [numRays][3]
        const double* q;           // [cells][PROBE_WIDTH]: the values of this pass
        double* sums;              // [numRays][PROBE_WIDTH]
        unsigned long long numRays;
        unsigned long long* work;  // [PROBE_WORK_WORDS]: ray cursor, rays stopped by the step cap, lane steps, wave steps
    };

    // claimSlots with a cursor of its own and 64-bit ray indices; ~0 for a lane that gets none
    __device__ __forceinline__ unsigned long long claimRays(unsigned long long* cursor, unsigned long long numRays, int lane, bool want,
                                                            unsigned long long& poolNext, unsigned long long& poolEnd, bool& exhausted)
    {
        const unsigned long long none = ~0ull;
        const unsigned long long idle = __ballot(want);
        const int nidle = __popcll(idle);
        if (!nidle || exhausted) return none;
        if (poolNext >= poolEnd)
        {
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(cursor, PROBE_CHUNK);
            got = __shfl(got, 0, 64);
            poolNext = got;
            poolEnd = got + PROBE_CHUNK;
            if (poolEnd > numRays) poolEnd = numRays;
            if (poolNext >= poolEnd)
            {
                poolNext = poolEnd = 0;
                exhausted = true;
                return none;
            }
        }
        const unsigned long long base = poolNext;
        const unsigned long long avail = poolEnd - poolNext;
        poolNext += (unsigned long long)nidle < avail ? (unsigned long long)nidle : avail;
        if (!want) return none;
        const unsigned long long rank = __popcll(idle & ((1ull << lane) - 1ull));
        return rank < avail ? base + rank : none;
    }

    // the state of a lane's ray: the generic Walk, or the octree kernels' TWalk and Dir
    template<int GRID, bool WIDE> struct ProbeWalk
    {
        Walk w;
    };
    template<bool WIDE> struct ProbeWalk<GRID_TREE, WIDE>
    {
        TWalk<WIDE> w;
        Dir d;
    };

    // start of a ray as in the single-ray tracers; false: no cell segment at all
    template<int GRID, bool WIDE>
    __device__ __forceinline__ bool probeStart(const DevScene& S, const GridLds& L, ProbeWalk<GRID, WIDE>& p, double rx, double ry, double rz, double kx,
                                               double ky, double kz)
    {
        Walk g;
        g.rx = rx, g.ry = ry, g.rz = rz;
        setDirection(g, kx, ky, kz);
        g.tau = 0., g.s = 0., g.lastm = -1;
        double cumds;
        if (!moveInside(S, g, cumds)) return false;
        if constexpr (GRID == GRID_TREE)
        {
            p.d.kx = g.kx, p.d.ky = g.ky, p.d.kz = g.kz;
            p.d.ikx = g.ikx, p.d.iky = g.iky, p.d.ikz = g.ikz;
            p.d.sgn = g.sgn;
            setDirMasks(p.d);
            const int m = topDown(S, L, g.rx, g.ry, g.rz);
            treeEnter<false>(reinterpret_cast<const char*>(S.leaves), L, g, m);
            TWalk<WIDE>& w = p.w;
            w.rx = g.rx, w.ry = g.ry, w.rz = g.rz;
            w.tau = 0., w.s = 0., w.lastm = -1;
            w.ds = g.ds, w.dens = g.dens;
            w.cell = (uint32_t)g.cell, w.axis = (uint32_t)g.axis;
            setBox<WIDE>(w, (typename Pack<WIDE>::T)g.P, g.e);
            return true;
        }
        else
        {
            bool ok = true;
            if (GRID == GRID_CART)
            {
                g.ci = locateClip(L.grid, S.nx + 1, g.rx);
                g.cj = locateClip(L.grid + (S.nx + 1), S.ny + 1, g.ry);
                g.ck = locateClip(L.grid + (S.nx + 1) + (S.ny + 1), S.nz + 1, g.rz);
                cartEnter(S, L, g);
            }
            else if (GRID == GRID_BIN)
                binStart(S, g, -1);
            else
                ok = voroLocateAndEnter(S, g);
            p.w = g;
            return ok;
        }
    }

    // the step behind the pending segment as in the single-ray tracers; false: the ray has left the grid
    template<int GRID, bool WIDE>
    __device__ __forceinline__ bool probeAdvance(const DevScene& S, const GridLds& L, const TreeConst& C, const char* nodes, ProbeWalk<GRID, WIDE>& p)
    {
        if constexpr (GRID == GRID_TREE)
        {
            TWalk<WIDE>& w = p.w;
            const Dir& d = p.d;
            CellLoad g;
            cellIssue(C, w.cell, g);
            const double step = w.ds + S.eps;
            const double nrx = w.rx + d.kx * step, nry = w.ry + d.ky * step, nrz = w.rz + d.kz * step;
            const uint32_t link = cellLink<-1>(g, d, w.axis);
            w.rx = nrx, w.ry = nry, w.rz = nrz;
#ifdef PMC_PROFILE
            WalkProf prof = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
#endif
            uint32_t cell2;
            int r = treeResolve<WIDE, -1>(C, nodes, d, w, link, nrx, nry, nrz, cell2 PMC_WPROF_PASS);
            if (r == ST_ACTIVE)
            {
                r = treeEnterBox<WIDE, -1>(C, d, w PMC_WPROF_PASS);
                if (r == ST_ACTIVE) w.cell = cell2;
            }
            if (r == ST_EDGE) r = treeEdgeStateAt(C, w.rx, w.ry, w.rz);
            if (r == ST_SLOW) return treeSlowStep<WIDE>(S, L, d, w);
            return r != ST_EXIT;
        }
        else if (GRID == GRID_BIN)
        {
            const int r = binAdvance(S, p.w);
            return r == ST_ACTIVE || (r == ST_SLOW && binStepSlow(S, p.w));
        }
        else if (GRID == GRID_VORO)
        {
            const int r = voroAdvance(S, p.w);
            if (r == ST_SLOW) return voroStepSlow(S, p.w);
            return r != ST_EXIT;
        }
        else
            return cartAdvance(S, L, p.w);
    }

    template<int GRID, bool WIDE> __global__ __launch_bounds__(256) void integrateRaysKernel(const int sceneSlot, const ProbeArgs A)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        if (GRID == GRID_TREE) requireLdsBaseZero(lds);
        stageGrid<GRID>(S, lds, tid, blockDim.x);
        __syncthreads();
        GridLds L = makeGridLds(S, lds);
        if (GRID == GRID_TREE && !WIDE) L.gtab = nullptr;  // (octrees up to level 10 always have their table in LDS: the test folds away)
        const char* nodes = reinterpret_cast<const char*>(S.nodes);
        TreeConst C;
        if (GRID == GRID_TREE) loadTreeConst(S, C);

        ProbeWalk<GRID, WIDE> p;
        double sum[PROBE_WIDTH];
        unsigned long long ray = ~0ull;
        int guard = 0;
        bool active = false;
        unsigned long long poolNext = 0, poolEnd = 0;
        bool exhausted = false;
        uint32_t laneSteps = 0, waveSteps = 0, capped = 0;
        while (true)
        {
            const unsigned long long got = claimRays(A.work + PROBE_WORK_CURSOR, A.numRays, lane, !active, poolNext, poolEnd, exhausted);
            if (!active && got != ~0ull)
            {
                ray = got;
                guard = 0;
#pragma unroll
                for (int v = 0; v < PROBE_WIDTH; ++v) sum[v] = 0.;
                const double* r = A.origins + 3 * ray;
                const double* k = A.directions + 3 * ray;
                active = probeStart<GRID, WIDE>(S, L, p, r[0], r[1], r[2], k[0], k[1], k[2]);
                if (!active)
                {
#pragma unroll
                    for (int v = 0; v < PROBE_WIDTH; ++v) A.sums[ray * PROBE_WIDTH + v] = 0.;
                }
            }
            if (!__ballot(active))
            {
                if (exhausted) break;
                continue;
            }
            ++waveSteps;
            if (active)
            {
                ++laneSteps;
                // the pending segment (m, ds): every cell of these grids has m >= 0
                const double ds = p.w.ds;
                const double* q = A.q + (size_t)(uint32_t)p.w.cell * PROBE_WIDTH;
#pragma unroll
                for (int v = 0; v < PROBE_WIDTH; ++v) sum[v] += ds * q[v];
                bool inside = probeAdvance<GRID, WIDE>(S, L, C, nodes, p);
                if (inside && ++guard >= PROBE_STEP_CAP)
                {
                    ++capped;
                    inside = false;
                }
                if (!inside)
                {
#pragma unroll
                    for (int v = 0; v < PROBE_WIDTH; ++v) A.sums[ray * PROBE_WIDTH + v] = sum[v];
                    active = false;
                }
            }
        }
        unsigned long long v;
        v = waveSum(capped);
        if (lane == 0 && v) atomicAdd(A.work + PROBE_WORK_CAPPED, v);
        v = waveSum(laneSteps);
        if (lane == 0 && v) atomicAdd(A.work + PROBE_WORK_LANE_STEPS, v);
        if (lane == 0 && waveSteps) atomicAdd(A.work + PROBE_WORK_WAVE_STEPS, (unsigned long long)waveSteps);
    }
