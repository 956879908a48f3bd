// pmc_ray.inc -- rays through the grid outside the photon loop (included by pmc_kernels.hip inside its anonymous namespace, behind the walk
// kernels): the ray cursor, the single-ray tracer on it (pmc_trace_ray) and the batched ray integrals (pmc_integrate_rays).
//
// The cursor is the walk kernels' traversal code for one ray: rayStart is startWalk (State::Unknown of PathSegmentGenerator::next) without a
// hint, rayAdvance the step behind the pending segment (m, ds) with the deferred cases -- the literal algorithm for an undecided step -- served
// at once.  Both kernels below run on this one copy, so a ray's segments in the integrator are pmc_trace_ray's bit for bit.

    // the state of a ray: the generic Walk, or the octree kernels' TWalk and Dir
    template<int GRID, bool WIDE> struct RayCursor
    {
        Walk w;
    };
    template<bool WIDE> struct RayCursor<GRID_TREE, WIDE>
    {
        TWalk<WIDE> w;
        Dir d;
    };

    // start of the ray (r, k); false: no cell segment at all.  outside receives the length of the initial segment outside the grid
    // (SpatialGridPath::addSegment(-1, cumds)), 0 if there is none
    template<int GRID, bool WIDE>
    __device__ __forceinline__ bool rayStart(const DevScene& S, const GridLds& L, RayCursor<GRID, WIDE>& p, double rx, double ry, double rz, double kx,
                                             double ky, double kz, double& outside)
    {
        Walk g;
        g.rx = rx, g.ry = ry, g.rz = rz;
        setDirection(g, kx, ky, kz);
        int located;
        const bool ok = startWalk<GRID>(S, L, g, /*hint*/ -1, located);
        outside = g.s;  // (0. + cumds: exact)
        if constexpr (GRID == GRID_TREE)
        {
            dirFromWalk(g, p.d);
            if (!ok) return false;
            p.w.tau = 0., p.w.s = g.s, p.w.lastm = -1;
            treeWalkFrom<WIDE>(g, p.w);
        }
        else
            p.w = g;
        return ok;
    }

    // the step behind the pending segment; false: the ray has left the grid.  SGNX: the sign octant of the direction the octree step is
    // specialised for, -1: the direction's own signs (pmc_walk_tree.inc dirUpX)
    template<int GRID, bool WIDE, int SGNX>
    __device__ __forceinline__ bool rayAdvance(const DevScene& S, const GridLds& L, const TreeConst& C, const char* nodes, RayCursor<GRID, WIDE>& p)
    {
        if constexpr (GRID == GRID_TREE)
        {
            TWalk<WIDE>& w = p.w;
            const Dir& d = p.d;
            CellLoad g;
            cellIssue(C, w.cell, g);
            const double step = w.ds + S.eps;
            const double nrx = w.rx + d.kx * step, nry = w.ry + d.ky * step, nrz = w.rz + d.kz * step;
            const uint32_t link = cellLink<SGNX>(g, d, w.axis);
            w.rx = nrx, w.ry = nry, w.rz = nrz;
#ifdef PMC_PROFILE
            WalkProf prof = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
#endif
            uint32_t cell2;
            int r = treeResolve<WIDE, SGNX>(C, nodes, d, w, link, nrx, nry, nrz, cell2 PMC_WPROF_PASS);
            if (r == ST_ACTIVE)
            {
                r = treeEnterBox<WIDE, SGNX>(C, d, w PMC_WPROF_PASS);
                if (r == ST_ACTIVE) w.cell = cell2;
            }
            if (r == ST_EDGE) r = treeEdgeStateAt(C, w.rx, w.ry, w.rz);
            if (r == ST_SLOW) return treeSlowStep<WIDE>(S, L, d, w);
            return r != ST_EXIT;
        }
        else if (GRID == GRID_BIN)
        {
            // (the step of the walk kernel, and its service round for an undecided one)
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

    // step(std::integral_constant<int, SGNX>()) for the sign octant SGNX = sgn of a direction
    template<typename Step> __device__ __forceinline__ void forSignOctant(uint32_t sgn, Step step)
    {
        switch (sgn & 7u)
        {
            case 0: step(std::integral_constant<int, 0>()); break;
            case 1: step(std::integral_constant<int, 1>()); break;
            case 2: step(std::integral_constant<int, 2>()); break;
            case 3: step(std::integral_constant<int, 3>()); break;
            case 4: step(std::integral_constant<int, 4>()); break;
            case 5: step(std::integral_constant<int, 5>()); break;
            case 6: step(std::integral_constant<int, 6>()); break;
            default: step(std::integral_constant<int, 7>()); break;
        }
    }

    // ================================================================================================
    //  single-ray tracer: the cursor in one lane, (m, ds) written out.
    //  UNIFORM (a choice on the octree only): the direction comes from kernel arguments (scalar registers) and the steps run in the
    //  instantiation for the direction's sign octant, as in the peel-off kernel; otherwise the direction comes from memory through the lane
    //  index (vector registers, signs at run time, as in the propagation kernel)
    // ================================================================================================
    template<int GRID, bool WIDE, bool UNIFORM>
    __global__ void traceRayKernel(const int sceneSlot, double rx, double ry, double rz, double kx, double ky, double kz, const double* kdev, int32_t* mOut,
                                   double* dsOut, int32_t cap, int32_t* nOut)
    {
        static_assert(GRID == GRID_TREE || (!WIDE && UNIFORM), "the other grids have one tracer each");
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        if (GRID == GRID_TREE) requireLdsBaseZero(lds);
        stageGrid<GRID>(S, lds, tid, blockDim.x);
        __syncthreads();
        if (tid != 0) return;
        GridLds L = makeGridLds(S, lds);
        if (GRID == GRID_TREE && !WIDE) L.gtab = nullptr;  // (octrees up to level 10 always have their table in LDS: the test folds away)
        const char* nodes = reinterpret_cast<const char*>(S.nodes);
        TreeConst C;
        if (GRID == GRID_TREE) loadTreeConst(S, C);
        if (!UNIFORM) kx = kdev[tid], ky = kdev[tid + 1], kz = kdev[tid + 2];

        RayCursor<GRID, WIDE> p;
        int n = 0;
        double outside;
        const bool ok = rayStart<GRID, WIDE>(S, L, p, rx, ry, rz, kx, ky, kz, outside);
        const auto record = [&](int32_t m, double ds) {
            if (n < cap)
            {
                mOut[n] = m;
                dsOut[n] = ds;
            }
            ++n;
        };
        if (outside > 0.) record(-1, outside);
        const auto steps = [&](auto sgnx) {
            bool inside = ok;
            int guard = 0;
            while (inside && guard++ < PMC_RAY_STEP_CAP)
            {
                record((GRID == GRID_TREE || GRID == GRID_BIN) ? S.cell_ext[p.w.cell] : (int32_t)p.w.cell, p.w.ds);
                inside = rayAdvance<GRID, WIDE, decltype(sgnx)::value>(S, L, C, nodes, p);
            }
        };
        if constexpr (GRID == GRID_TREE && UNIFORM)
            forSignOctant(p.d.sgn, steps);
        else
            steps(std::integral_constant<int, -1>());
        *nOut = n;
    }

    // ================================================================================================
    //  batched ray integrals: sums[i][v] = sum over the path of ray i of ds * q[v][m]: ProbeFormBridge::valuesAlongPath for the accumulated
    //  quantities (ProbeFormBridge.cpp:628-650, 707-725).  Every lane of a wave runs the cursor for a ray of its own: persistent waves take
    //  rays in chunks from a cursor, a lane whose ray has ended takes the next one (rays that miss the grid end at once), the products are
    //  added in path order without contraction.
    //
    //  q is laid out for the step's gather: per pass of PMC_INTEGRATE_PASS_VALUES values one record [cell][PMC_INTEGRATE_PASS_VALUES] in the
    //  numbering the kernel walks in (octree, binary tree: device cells), rows beyond the caller's last value zero.  The sums of a pass are
    //  kept in registers.
    //
    //  AVERAGED (pmc_integrate_weighted_rays, ProbeFormBridge.cpp:652-676): the cell record of a pass is (w, v0, v1, v2); a step adds
    //  weight = ds * w to sum[0] and weight * v to the sums behind it, and the raw sums go back: the caller divides.
    // ================================================================================================
    constexpr int PROBE_WIDTH = PMC_INTEGRATE_PASS_VALUES;
    constexpr unsigned long long PROBE_CHUNK = 64;  // rays a wave takes from the cursor at a time
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

    // claimSlots with a cursor of its own and 64-bit ray indices; ~0 for a lane that gets none.  (A copy: with claimSlots as a wrapper of one
    // shared function the walk kernels compile to other code, profiles/sweeps/ray_cursor_refactor.md.)
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

    template<int GRID, bool WIDE, bool AVERAGED> __global__ __launch_bounds__(256) void integrateRaysKernel(const int sceneSlot, const ProbeArgs A)
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

        RayCursor<GRID, WIDE> p;
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
                double outside;  // (the segment outside the grid adds nothing)
                active = rayStart<GRID, WIDE>(S, L, p, r[0], r[1], r[2], k[0], k[1], k[2], outside);
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
                if constexpr (AVERAGED)
                {
                    const double weight = ds * q[0];
                    sum[0] += weight;
#pragma unroll
                    for (int v = 1; v < PROBE_WIDTH; ++v) sum[v] += weight * q[v];
                }
                else
                {
#pragma unroll
                    for (int v = 0; v < PROBE_WIDTH; ++v) sum[v] += ds * q[v];
                }
                bool inside = rayAdvance<GRID, WIDE, -1>(S, L, C, nodes, p);
                if (inside && ++guard >= PMC_RAY_STEP_CAP)
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
