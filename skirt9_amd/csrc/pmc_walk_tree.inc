// pmc_walk_tree.inc -- the octree walk (included by pmc_kernels.hip after pmc_walk.inc, inside its anonymous namespace):
// the fast step, the pieces the kernels share (frame, step head and tail, undecided steps, epilogues, checkpoint packing,
// radiation-field log append) and the three walk kernels.
//
//   walkPeelKernel   all peel-off walks towards ONE observer (MediumSystem::getExtinctionOpticalDepth,
//                    MediumSystem.cpp:1192-1260).  Every walk of the launch has the same direction k_obs, so the
//                    direction, RN(1/k), the sign bits and everything derived from them are wave-uniform: they live in
//                    SGPRs, the wall selection is scalar, and a lane keeps only position, optical depth and cell.
//                    This form serves scenes with several media, and octrees whose LDS has no room for the task queues.
//   walkPeelKernel2  the same walks for every other scene: one instantiation per sign octant of k_obs, and a lane takes
//                    up its next walk by itself from a queue of task records that its wave keeps in LDS.
//   walkPropKernel   the propagation walk of every slot (MediumSystem::setExtinctionOpticalDepths, :849-901, and the
//                    interaction point, SpatialGridPath.cpp:164-206): pass 1 over the whole path, the sampled optical
//                    depth between the passes (MonteCarloSimulation.cpp:696-722), pass 2 up to it; per-lane directions.
//
// Not here: the checkpoint decisions of pass 1 (pmc_walk.inc: ckptStart, ckptTick, ckptResume, shared with voroPropKernel) and the
// kernels that sort and sum the logs behind the walks (pmc_log.inc).
//
// The step is software-pipelined around its ONE memory round trip: the hot record of a cell (CellRec: density + six
// links, 32 bytes) is requested as soon as the cell is known -- when the link through the exit wall of the previous
// cell has been read -- and BEFORE the arithmetic that enters the cell (walls from LDS, inside test, three exit
// distances), which therefore runs while the record is in flight.  What sits between the arrival of a record and the
// request for the next one is the link selection, the stop test and the integer bookkeeping of the box.
//
// Box bookkeeping.  A lane carries the box of its cell as the byte offsets of its three lower walls in the per-axis coordinate
// table (8 x the fine lower-corner index) and the byte distance to the upper walls (8 << size exponent): the six wall addresses of
// a step are these offsets (+ the axis base, + the distance) and nothing else.  The cell behind the exit wall is named by the link
// of the step's gather; when it is a leaf of the same size or coarser (it covers the whole wall) its box follows from the offsets by
// integer arithmetic alone -- step across the wall, align to the leaf's size -- and when finer neighbours share the wall, the octant
// decisions below the same-size internal node come from the index bits of the new position BELOW the node's size: without any load
// when the node's children are all leaves (octet link: consecutive cells in child order), with one 4-byte gather per level otherwise.
// (Rounds 2-4 carried the three indices packed in one integer: six more integer operations per step to take them apart again.)
// Either way the box is that of the leaf the link leads to, and the STRICT inside test of the new position against its
// table walls decides: inside => no other leaf's closed box contains the position, so the reference's neighbour-list scan
// and its top-down search both end in this leaf (TreeSpatialGrid.cpp:192-207); otherwise (shared boundary, a step that
// overshoots a second wall near an edge, a direction component too small to cross the wall) the literal algorithm runs.

#ifdef PMC_PROFILE
    // cycle stamps of the octree walk kernels (profiling builds only): wave cycles between stamps, all memory operations
    // drained first so that a phase owns its waits.  [0] step: issue + gather wait, [1] tau / position, [2] descent,
    // [3] walls from LDS, [4] inside test + exit distance, [5] service: finish + claim, [6] service: task loads,
    // [7] loop overhead
    struct WalkProf
    {
        long long t[8];
        long long last;
        uint32_t census[8];  // per lane: [0] literal-algorithm steps, [2] edge, [3] descents, [4] descent levels, [5] octet links, [6] hit, [7] exit
    };
    #define PMC_CENSUS(i, pred)              \
        do                                   \
        {                                    \
            if (pred) prof.census[i] += 1;   \
        } while (0)
    #define PMC_CENSUS_WAVE(i, pred) PMC_CENSUS(i, pred)
    #ifdef PMC_PROFILE_STAMPS
    #define PMC_WSTAMP(i)                                                         \
        do                                                                        \
        {                                                                         \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");           \
            const long long now_ = clock64();                                     \
            prof.t[i] += now_ - prof.last;                                        \
            prof.last = now_;                                                     \
        } while (0)
    #else
    #define PMC_WSTAMP(i)  // (census only: event counts without the draining time stamps)
    #endif
    #define PMC_WPROF_ARG , WalkProf& prof
    #define PMC_WPROF_PASS , prof
#else
    #define PMC_WSTAMP(i)
    #define PMC_CENSUS(i, pred)
    #define PMC_CENSUS_WAVE(i, pred)
    #define PMC_WPROF_ARG
    #define PMC_WPROF_PASS
#endif

    template<bool WIDE> struct Pack;
    template<> struct Pack<false>
    {
        typedef uint32_t T;
        static constexpr int FB = 10;  // octrees up to level 10
    };
    template<> struct Pack<true>
    {
        typedef uint64_t T;
        static constexpr int FB = 21;  // levels 11 and 12
    };

    template<bool WIDE> struct TWalk
    {
        double rx, ry, rz;   // generator position
        double tau, s;       // cumulative optical depth and path length of the segments emitted so far
        double ds;           // length of the pending segment
        double dens;         // number density of the cell of the pending segment
        uint32_t bx, by, bz; // the cell's lower walls: byte offsets in the per-axis coordinate table (8 x fine lower-corner index)
        uint32_t szb;        // byte distance to its upper walls: 8 << e (the box spans 2^e finest cells per axis)
        uint32_t cell, axis;
        int lastm;
    };
    // the box from the packed fine lower-corner indices and the size exponent of the task records (TaskArrays::pidx, bits)
    template<bool WIDE> __device__ __forceinline__ void setBox(TWalk<WIDE>& w, typename Pack<WIDE>::T P, uint32_t e)
    {
        typedef typename Pack<WIDE>::T PT;
        constexpr int FB = Pack<WIDE>::FB;
        constexpr PT FM = (PT(1) << FB) - 1;
        w.bx = (uint32_t)(P & FM) << 3;
        w.by = (uint32_t)((P >> FB) & FM) << 3;
        w.bz = (uint32_t)((P >> (2 * FB)) & FM) << 3;
        w.szb = 8u << e;
    }

    // direction of a walk; in the peel-off kernel every field is wave-uniform
    struct Dir
    {
        double kx, ky, kz;
        double ikx, iky, ikz;       // RN(1/k), NaN for an ignored axis
        uint32_t sgn;               // bit a: k_a < 0
        uint32_t posx, posy, posz;  // all ones where k_a >= 0, zero where k_a < 0
    };
    __device__ __forceinline__ void setDirMasks(Dir& d)
    {
        d.posx = (d.sgn & 1u) - 1u;
        d.posy = ((d.sgn >> 1) & 1u) - 1u;
        d.posz = ((d.sgn >> 2) & 1u) - 1u;
    }
    // the direction of the generic Walk
    __device__ __forceinline__ void dirFromWalk(const Walk& g, Dir& d)
    {
        d.kx = g.kx, d.ky = g.ky, d.kz = g.kz;
        d.ikx = g.ikx, d.iky = g.iky, d.ikz = g.ikz;
        d.sgn = g.sgn;
        setDirMasks(d);
    }
    // position, pending segment and cell of the generic Walk (treeEnter, treeStepSlow); the running sums stay the caller's
    template<bool WIDE> __device__ __forceinline__ void treeWalkFrom(const Walk& g, TWalk<WIDE>& w)
    {
        w.rx = g.rx, w.ry = g.ry, w.rz = g.rz;
        w.ds = g.ds;
        w.dens = g.dens;
        w.cell = (uint32_t)g.cell;
        w.axis = (uint32_t)g.axis;
        setBox<WIDE>(w, (typename Pack<WIDE>::T)g.P, g.e);
    }
    // SGN >= 0: the sign pattern of the direction is a compile-time constant (the peel-off kernel is instantiated per octant of the
    // observer's direction: every selection by sign folds away); SGN < 0: the direction's own (per lane, or in scalar registers)
    template<int SGN> __device__ __forceinline__ bool dirUpX(const Dir& d) { return SGN >= 0 ? !(SGN & 1) : d.posx != 0u; }
    template<int SGN> __device__ __forceinline__ bool dirUpY(const Dir& d) { return SGN >= 0 ? !(SGN & 2) : d.posy != 0u; }
    template<int SGN> __device__ __forceinline__ bool dirUpZ(const Dir& d) { return SGN >= 0 ? !(SGN & 4) : d.posz != 0u; }
    template<int SGN> __device__ __forceinline__ uint32_t dirSigns(const Dir& d) { return SGN >= 0 ? (uint32_t)SGN : d.sgn; }

    // the hot record of a cell on its way to the registers (two 16-byte loads of one 32-byte record)
    struct CellLoad
    {
        uint4 a;  // density (x, y), link[0], link[1]
        uint4 b;  // link[2] ... link[5]
    };
    __device__ __forceinline__ void cellIssue(const TreeConst& C, uint32_t cell, CellLoad& g)
    {
        const char* p = C.cellTab + ((uint64_t)cell << 5);
        g.a = *reinterpret_cast<const uint4*>(p);
        g.b = *reinterpret_cast<const uint4*>(p + 16);
    }
    __device__ __forceinline__ double cellDensity(const CellLoad& g)
    {
        return __longlong_as_double(((long long)g.a.y << 32) | g.a.x);
    }
    // the link through the wall of `axis` that the direction leaves by
    // the record has landed and is taken as a whole (with a compile-time sign octant the compiler would otherwise narrow the two 16-byte
    // loads to the 20 bytes in use -- three load instructions: a third load of a line costs the memory pipeline of a CU 40 % more than
    // two, profiles/microbench/cu_limit_mi355x.txt)
    __device__ __forceinline__ void cellLanded(CellLoad& g)
    {
        asm volatile("" : "+v"(g.a.x), "+v"(g.a.y), "+v"(g.a.z), "+v"(g.a.w), "+v"(g.b.x), "+v"(g.b.y), "+v"(g.b.z), "+v"(g.b.w));
    }
    template<int SGN> __device__ __forceinline__ uint32_t cellLink(const CellLoad& g, const Dir& d, uint32_t axis)
    {
        const uint32_t fx = dirUpX<SGN>(d) ? g.a.w : g.a.z, fy = dirUpY<SGN>(d) ? g.b.y : g.b.x, fz = dirUpZ<SGN>(d) ? g.b.w : g.b.z;
        return axis == 0u ? fx : axis == 1u ? fy : fz;
    }

    // Fast step, part 1 (TreeSpatialGrid.cpp:186-207): the leaf behind the exit wall of the current cell, named by `link`,
    // for the advanced position (nrx, nry, nrz): its device index, and its box (lower-wall offsets, distance to the upper walls) in w.
    // Returns ST_ACTIVE; ST_EDGE if the wall is on the grid boundary; ST_SLOW if the literal algorithm is needed.
    // Straight-line code except for the descent below a node with mixed children.
    template<bool WIDE, int SGN>
    __device__ __forceinline__ int treeResolve(const TreeConst& C, const char* nodes, const Dir& d, TWalk<WIDE>& w, uint32_t link, double nrx,
                                               double nry, double nrz, uint32_t& cellout PMC_WPROF_ARG)
    {
        if (link == PMC_LINK_NONE) return ST_EDGE;
        // across the wall: the first index beyond the upper wall, or one index below the lower corner; then the lower corner of the
        // leaf that covers the wall (same size or coarser), or of the same-size internal node: aligned to its size on every axis
        const uint32_t up = ((dirSigns<SGN>(d) >> w.axis) & 1u) - 1u;  // all ones when the walk moves up the exit axis
        const uint32_t across = (w.szb & up) | (~up & 0xFFFFFFF8u);     // + the cell's size, or - one finest cell
        uint32_t szb = 8u << (link & PMC_LINK_EXP_MASK);
        const uint32_t align = 0u - szb;
        uint32_t bx = (w.bx + (w.axis == 0u ? across : 0u)) & align;
        uint32_t by = (w.by + (w.axis == 1u ? across : 0u)) & align;
        uint32_t bz = (w.bz + (w.axis == 2u ? across : 0u)) & align;
        uint32_t cell = link >> PMC_LINK_EXP_BITS;
        if (link & (PMC_LINK_NODE | PMC_LINK_OCTET))
        {
            // finer neighbours: the octant decisions are the index bits of the position below the node's size (the indices only
            // steer: a wrongly rounded one leads to a leaf that fails the strict test).  ix = 8 x the fine index (bits 0-2: fraction)
            const uint32_t ix = (uint32_t)(int)__builtin_fma(nrx, C.sx8, C.bx8);
            const uint32_t iy = (uint32_t)(int)__builtin_fma(nry, C.sy8, C.by8);
            const uint32_t iz = (uint32_t)(int)__builtin_fma(nrz, C.sz8, C.bz8);
            uint32_t fine;  // size of the leaf found
            if ((int32_t)link < 0)
            {
                // children of mixed kinds: one 4-byte gather per level
                PMC_CENSUS(3, true);
                do
                {
                    PMC_CENSUS(4, true);
                    const uint32_t b = ((link & PMC_LINK_EXP_MASK) + 2u) & 31u;  // bit of the 8-fold index that selects the child: (e - 1) + 3
                    const uint32_t l = ((ix >> b) & 1u) | (((iy >> b) & 1u) << 1) | (((iz >> b) & 1u) << 2);
                    link = *reinterpret_cast<const uint32_t*>(nodes + ((((link >> PMC_LINK_EXP_BITS) & PMC_LINK_INDEX_MASK) << 6) + 8u + (l << 2)));
                } while ((int32_t)link < 0);
                if (link == PMC_LINK_NONE) return ST_SLOW;
                fine = 8u << (link & PMC_LINK_EXP_MASK);
                cell = link >> PMC_LINK_EXP_BITS;
            }
            else
            {
                // eight leaf children, consecutive cells in child order: no load
                PMC_CENSUS(5, true);
                const uint32_t b = ((link & PMC_LINK_EXP_MASK) + 2u) & 31u;
                const uint32_t l = ((ix >> b) & 1u) | (((iy >> b) & 1u) << 1) | (((iz >> b) & 1u) << 2);
                cell = ((link >> PMC_LINK_EXP_BITS) & PMC_LINK_INDEX_MASK) + l;
                fine = szb >> 1;
            }
            // the index bits of the position below the node's size and at or above the leaf's
            const uint32_t below = (szb - 1u) & (0u - fine);
            bx |= ix & below;
            by |= iy & below;
            bz |= iz & below;
            szb = fine;
        }
        // (the box of w is the candidate's from here on: the literal algorithm, should it be needed, starts from w.cell and the
        // position and sets the box anew)
        w.bx = bx, w.by = by, w.bz = bz;
        w.szb = szb;
        cellout = cell;
        return ST_ACTIVE;
    }

    // Fast step, part 2: the STRICT inside test of the position w.r against the table walls of the box that treeResolve left in w,
    // and the exit distance of the new cell (TreeSpatialGrid.cpp:160-185).  Returns ST_ACTIVE (w.ds, w.axis set); ST_SLOW (w.ds,
    // w.axis, w.cell untouched) if the literal algorithm is needed.  Straight-line code.
    template<bool WIDE, int SGN>
    __device__ __forceinline__ int treeEnterBox(const TreeConst& C, const Dir& d, TWalk<WIDE>& w PMC_WPROF_ARG)
    {
        const uint32_t bx = w.bx, by = w.by, bz = w.bz, szb = w.szb;
        const uint32_t oy = by + C.stride, oz = bz + 2u * C.stride;
        // wall - position for the six walls: strictly inside <=> every lower one is negative and every upper one positive
        const double rx = w.rx, ry = w.ry, rz = w.rz;
        double X0, X1, Y0, Y1, Z0, Z1;
        if (WIDE && C.gtab)
        {
            // (an octree of 13 to 20 levels: the table is read from global memory -- 0.2-0.8 MB up to level 15, L2-resident; 25 MB at level 20)
            X0 = *reinterpret_cast<const double*>(C.gtab + bx), X1 = *reinterpret_cast<const double*>(C.gtab + bx + szb);
            Y0 = *reinterpret_cast<const double*>(C.gtab + oy), Y1 = *reinterpret_cast<const double*>(C.gtab + oy + szb);
            Z0 = *reinterpret_cast<const double*>(C.gtab + oz), Z1 = *reinterpret_cast<const double*>(C.gtab + oz + szb);
        }
        else
        {
            X0 = ldsAt(nullptr, bx), X1 = ldsAt(nullptr, bx + szb);
            Y0 = ldsAt(nullptr, oy), Y1 = ldsAt(nullptr, oy + szb);
            Z0 = ldsAt(nullptr, oz), Z1 = ldsAt(nullptr, oz + szb);
        }
        const double x0 = X0 - rx, x1 = X1 - rx;
        const double y0 = Y0 - ry, y1 = Y1 - ry;
        const double z0 = Z0 - rz, z1 = Z1 - rz;
        const double clear = fmin(fmin(fmin(x1, -x0), fmin(y1, -y0)), fmin(z1, -z0));
        if (!(clear > 0.)) return ST_SLOW;
        // the walls ahead are the exit candidates
        const double ax = dirUpX<SGN>(d) ? x1 : x0, ay = dirUpY<SGN>(d) ? y1 : y0, az = dirUpZ<SGN>(d) ? z1 : z0;
        // exit distances: correctly rounded quotients and the reference's tie order (x before y before z on equality)
        const double dsx = exactQuotient(ax, d.kx, d.ikx);
        const double dsy = exactQuotient(ay, d.ky, d.iky);
        const double dsz = exactQuotient(az, d.kz, d.ikz);
        const double m = fmin(dsx, fmin(dsy, dsz));
        w.ds = m;
        w.axis = (dsx == m) ? 0u : (dsy == m) ? 1u : 2u;
        return ST_ACTIVE;
    }

    // the literal algorithm (TreeSpatialGrid.cpp:192-207) for a lane of the fast kernels: through the generic Walk
    // (inlined: an out-of-line call would put the callee's frame in scratch memory, and a kernel that owns scratch runs
    // 1.7x slower here even though the call is never taken -- profiles/README.md, r02 experiment 4)
    template<bool WIDE> __device__ __forceinline__ bool treeSlowStep(const DevScene& S, const GridLds& L, const Dir& d, TWalk<WIDE>& w)
    {
        Walk g;
        g.rx = w.rx, g.ry = w.ry, g.rz = w.rz;
        g.kx = d.kx, g.ky = d.ky, g.kz = d.kz;
        g.ikx = d.ikx, g.iky = d.iky, g.ikz = d.ikz;
        g.sgn = d.sgn;
        g.cell = (int)w.cell;
        g.axis = (int)w.axis;
        if (!treeStepSlow(S, L, g)) return false;
        treeWalkFrom<WIDE>(g, w);
        return true;
    }
    __device__ __forceinline__ int treeEdgeStateAt(const TreeConst& C, double rx, double ry, double rz)
    {
        const bool inRoot = rx >= C.gx0 && rx <= C.gx1 && ry >= C.gy0 && ry <= C.gy1 && rz >= C.gz0 && rz <= C.gz1;
        return inRoot ? ST_SLOW : ST_EXIT;
    }

    __device__ __forceinline__ void loadTreeConst(const DevScene& S, TreeConst& C)
    {
        C.gx0 = S.gx0, C.gy0 = S.gy0, C.gz0 = S.gz0;
        C.gx1 = S.gx1, C.gy1 = S.gy1, C.gz1 = S.gz1;
        // (scaling by 8 is exact: the integer part of 8 x is 8 floor(x) + the first three fraction bits)
        C.sx8 = 8. * S.fine_scale[0], C.sy8 = 8. * S.fine_scale[1], C.sz8 = 8. * S.fine_scale[2];
        C.bx8 = 8. * (-S.gx0 * S.fine_scale[0]), C.by8 = 8. * (-S.gy0 * S.fine_scale[1]), C.bz8 = 8. * (-S.gz0 * S.fine_scale[2]);
        C.stride = S.tab_stride_bytes;
        C.gtab = S.tab_in_lds ? nullptr : reinterpret_cast<const char*>(S.coord_tab);
        C.cellTab = reinterpret_cast<const char*>(S.cell_tab);
        C.numCells = (uint32_t)S.cell_slots;
    }

    // ---- what the three kernels share: the frame, the step, the undecided steps of a service round, the epilogues
    // the frame of a kernel: the coordinate table staged in LDS (all lanes of the workgroup: a barrier), the constants of the step
    template<bool WIDE> __device__ __forceinline__ GridLds treeFrame(const DevScene& S, double* lds, TreeConst& C)
    {
        requireLdsBaseZero(lds);
        stageGrid<GRID_TREE>(S, lds, threadIdx.x, blockDim.x);
        __syncthreads();
        GridLds L = makeGridLds(S, lds);
        if (!WIDE) L.gtab = nullptr;  // (octrees up to level 10 always have their table in LDS: the test folds away)
        loadTreeConst(S, C);
        return L;
    }
    // a lane without a walk
    template<bool WIDE> __device__ __forceinline__ void idleWalk(TWalk<WIDE>& w, CellLoad& g)
    {
        w.cell = 0, w.axis = 0, w.szb = 8u, w.bx = w.by = w.bz = 0u;
        w.ds = 0., w.tau = 0., w.s = 0., w.dens = 0., w.lastm = -1;
        w.rx = w.ry = w.rz = 0.;
        g.a = make_uint4(0, 0, 0, 0), g.b = make_uint4(0, 0, 0, 0);
    }
    // the direction towards an observer: wave-uniform (scalar loads from the scene)
    __device__ __forceinline__ void observerDir(const DevInstrument& I, Dir& d)
    {
        d.kx = I.kx, d.ky = I.ky, d.kz = I.kz;
        d.ikx = I.ikx, d.iky = I.iky, d.ikz = I.ikz;
        d.sgn = I.sgn;
        setDirMasks(d);
    }

    // The step, head: the position after the pending segment, r + k (ds + eps) (TreeSpatialGrid.cpp:186-191), which needs no memory; then, from the
    // record of the current cell, the density (w.dens) and the link through the exit wall (returned by value: with reference parameters walkPeelKernel
    // spills).  Between head and tail a kernel adds the pending segment to its sums and decides whether the walk stops.  (walkPeelKernel2: see there.)
    struct StepHead { double nrx, nry, nrz; uint32_t link; };
    template<bool WIDE, int SGN>
    __device__ __forceinline__ StepHead treeStepHead(const Dir& d, double eps, TWalk<WIDE>& w, const CellLoad& g PMC_WPROF_ARG)
    {
        const double step = w.ds + eps;
        StepHead h;
        h.nrx = w.rx + d.kx * step, h.nry = w.ry + d.ky * step, h.nrz = w.rz + d.kz * step;
        h.link = cellLink<SGN>(g, d, w.axis);
        w.dens = cellDensity(g);
        PMC_WSTAMP(0);
        return h;
    }
    // The step, tail: the walk moves to (nrx, nry, nrz) and enters the leaf behind the exit wall; that leaf's record is requested BEFORE
    // the arithmetic that enters it.  Returns the new state: ST_ACTIVE (w is in the new cell, g its record in flight), or ST_EDGE / ST_SLOW
    // (the next service round decides: treeServeUndecided).
    template<bool WIDE, int SGN>
    __device__ __forceinline__ int treeAdvance(const TreeConst& C, const char* nodes, const Dir& d, TWalk<WIDE>& w, CellLoad& g, uint32_t link,
                                               double nrx, double nry, double nrz PMC_WPROF_ARG)
    {
        w.rx = nrx, w.ry = nry, w.rz = nrz;
        uint32_t cell2;
        int st = treeResolve<WIDE, SGN>(C, nodes, d, w, link, nrx, nry, nrz, cell2 PMC_WPROF_PASS);
        PMC_WSTAMP(1);
        if (st == ST_ACTIVE)
        {
            cellIssue(C, cell2, g);
            st = treeEnterBox<WIDE, SGN>(C, d, w PMC_WPROF_PASS);
            if (st == ST_ACTIVE) w.cell = cell2;
            PMC_WSTAMP(4);
        }
        return st;
    }
    // The undecided steps of a service round (rare): the literal algorithm.  Returns true if the lane takes up a cell whose record has
    // not been requested yet.  (Profiling builds count here: edge, literal steps, and the walks that have ended.)
    template<bool WIDE>
    __device__ __forceinline__ bool treeServeUndecided(const DevScene& S, const GridLds& L, const TreeConst& C, const Dir& d, TWalk<WIDE>& w, int& st PMC_WPROF_ARG)
    {
        bool fresh = false;
        PMC_CENSUS(2, st == ST_EDGE);
        if (st == ST_EDGE) st = treeEdgeStateAt(C, w.rx, w.ry, w.rz);
        PMC_CENSUS(0, st == ST_SLOW);
        if (st == ST_SLOW)
        {
            st = treeSlowStep<WIDE>(S, L, d, w) ? ST_ACTIVE : ST_EXIT;
            fresh = st == ST_ACTIVE;
        }
        PMC_CENSUS(6, st == ST_HIT);
        PMC_CENSUS(7, st == ST_EXIT);
        return fresh;
    }
    // a finished peel-off walk: tau >= taumax (MediumSystem.cpp:1215-1218) or the optical depth of the whole path
    __device__ __forceinline__ void peelStoreResult(double* ptau, int slot, double tau, int& st)
    {
        if (st == ST_HIT || st == ST_EXIT)
        {
            ptau[slot] = st == ST_HIT ? INFINITY : tau;
            st = ST_IDLE;
        }
    }
    // the work counters of a wave of a peel-off kernel
    __device__ __forceinline__ void flushPeelWork(const DevScene& S, int lane, unsigned long long visits, unsigned long long waveSteps, unsigned long long services)
    {
        if (lane == 0 && visits)
        {
            atomicAdd(S.counters + 2, visits);
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 0, waveSteps);
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 1, visits);
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 2, services);
        }
    }
#ifdef PMC_PROFILE
    // the cycle stamps of a wave go to the eight counters from `base`, its census to those from base + 16 (208 / 224: peel-off, 216 / 232: propagation)
    __device__ __forceinline__ void flushWalkProf(const DevScene& S, int lane, const WalkProf& prof, int base, bool stamps)
    {
        if (stamps && lane == 0)
            for (int i = 0; i < 8; ++i) atomicAdd(S.counters + base + i, (unsigned long long)prof.t[i]);
        for (int i = 0; i < 8; ++i)
        {
            const unsigned long long c = waveSum(prof.census[i]);
            if (lane == 0 && c) atomicAdd(S.counters + base + 16 + i, c);
        }
    }
#endif

    // ================================================================================================
    //  peel-off walks towards observer `obs` (the instrument that starts an observer group) of the slots
    //  [slotBase, slotBase + numSlots): task record 1 + obs of every slot; result: SlotArrays::ptau
    // ================================================================================================
    // MM: several medium components (see walkKernel in pmc_walk.inc); such scenes use this form of the peel-off kernel
    template<bool WIDE, bool MM>
    __global__ __launch_bounds__(PMC_PEEL_BLOCK, PMC_PEEL_MIN_WAVES) void walkPeelKernel(const int sceneSlot, const int slotBase, const int numSlots,
                                                                            const int cursor, const int obs, const int* const list)
    {
        constexpr int SGNX = -1;  // (the direction's signs from scalar registers)
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int lane = threadIdx.x & 63;
        TreeConst C;
        const GridLds L = treeFrame<WIDE>(S, lds, C);
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const int64_t rec = (int64_t)(1 + obs) * A.num_slots;
        double* const ptau = A.ptau + (int64_t)obs * A.num_slots;
        const char* nodes = reinterpret_cast<const char*>(S.nodes);
        const double eps = S.eps;
        Dir d;
        observerDir(S.inst[obs], d);

        TWalk<WIDE> w;
        CellLoad g;  // the record of w.cell (in flight, or landed) whenever the lane is ST_ACTIVE
        idleWalk(w, g);
        int slot = -1;
        int st = ST_IDLE;
        double sext = 0., target = 0.;
        double mx[PMC_MAX_MEDIA] = {0., 0., 0., 0.};  // (MM) extinction cross section per component
        bool exhausted = false;
        unsigned long long poolNext = 0, poolEnd = 0;  // wave-uniform
        unsigned long long visits = 0;                 // wave-uniform: segments of all lanes
        unsigned long long waveSteps = 0, services = 0;
#ifdef PMC_PROFILE
        WalkProf prof = {{0, 0, 0, 0, 0, 0, 0, 0}, clock64(), {0, 0, 0, 0, 0, 0, 0, 0}};
#endif

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            if (exhausted && !activeMask && !pendingMask) break;
            const bool service = exhausted ? (pendingMask != 0ull) : (64 - __popcll(activeMask) >= PMC_PEEL_REFILL);
            PMC_WSTAMP(7);
            if (service)
            {
                services += 1;
                // ---- undecided steps, finished walks
                bool fresh = treeServeUndecided<WIDE>(S, L, C, d, w, st PMC_WPROF_PASS);  // the lane takes up a cell whose record has not been requested yet
                peelStoreResult(ptau, slot, w.tau, st);
                // ---- the next slots
                const int got = claimSlots(S, cursor, (unsigned long long)numSlots, lane, st == ST_IDLE, poolNext, poolEnd, exhausted, list ? 64ull : (unsigned long long)PMC_TASK_CHUNK);
                PMC_WSTAMP(5);
                if (got >= 0)
                {
                    // all fields of the record at once (one round trip; the first cell first, so that its record can be
                    // requested while the others are still on their way)
                    slot = list ? list[got] : slotBase + got;
                    const int64_t t = rec + slot;
                    const uint32_t cell0 = (uint32_t)K.cell[t];
                    const uint32_t bits = K.bits[t];
                    const auto P0 = (typename Pack<WIDE>::T)K.pidx[t];
                    const double rx0 = A.rx[slot], ry0 = A.ry[slot], rz0 = A.rz[slot];
                    const double ds0 = K.ds[t], target0 = K.target[t], sext0 = S.mono ? S.mono_ext : A.dustExt[slot];
                    if (bits != PMC_TASK_NONE)
                    {
                        w.cell = cell0;
                        setBox<WIDE>(w, P0, (bits >> 8) & PMC_TASK_EXP_MASK);
                        w.rx = rx0, w.ry = ry0, w.rz = rz0;
                        if (bits & PMC_TASK_MOVED) w.rx = K.rx[t], w.ry = K.ry[t], w.rz = K.rz[t];  // (the walk starts where moveInside left it)
                        w.ds = ds0;
                        target = target0;
                        sext = sext0;
                        if (MM)
                            for (int h = 0; h < S.num_media; ++h)
                            {
                                double sca, absn;
                                mediumSections(S, A, slot, h, mx[h], sca, absn);
                            }
                        w.axis = (bits >> 2) & 3u;
                        w.tau = 0.;
                        st = ST_ACTIVE;
                        fresh = true;
                    }
                }
                if (fresh) cellIssue(C, w.cell, g);
                PMC_WSTAMP(6);
            }
            // ---------------- walk steps
#pragma unroll 1
            for (int it = 0; it < PMC_WALK_STEPS; ++it)
            {
                visits += (unsigned long long)__popcll(__ballot(st == ST_ACTIVE));
                waveSteps += 1;
                PMC_WSTAMP(7);
                if (st == ST_ACTIVE)
                {
                    const StepHead h = treeStepHead<WIDE, SGNX>(d, eps, w, g PMC_WPROF_PASS);
                    // the pending segment (MediumSystem.cpp:1207-1219): stop once tau >= taumax
                    double tau1 = w.tau + sext * w.dens * w.ds;
                    if (MM)
                    {
                        double unused = 0.;
                        tau1 = w.tau;
                        mediaSegment<false>(S, (int)w.cell, w.dens, w.ds, false, mx, mx, mx, tau1, unused);
                    }
                    if (tau1 > target)
                        st = ST_HIT;
                    else
                    {
                        w.tau = tau1;
                        st = treeAdvance<WIDE, SGNX>(C, nodes, d, w, g, h.link, h.nrx, h.nry, h.nrz PMC_WPROF_PASS);
                    }
                }
            }
        }
        flushPeelWork(S, lane, visits, waveSteps, services);
#ifdef PMC_PROFILE
        flushWalkProf(S, lane, prof, 208, true);
#endif
    }

    // ================================================================================================
    //  peel-off walks towards observer `obs`, second form: a lane takes up its next walk BY ITSELF, in the step in which its
    //  walk ends, from a queue of task records that its wave keeps in LDS; the wave refills the queue 64 records at a time.
    //  Loads return in order, so every task record a wave requests (nine arrays, HBM latency) holds up the gathers it issues
    //  after it -- profiles/microbench/side_loads_mi355x.txt: nine streaming loads every 8 steps take 30 % off a gather
    //  chase, every 64 steps 5 % -- and a service round that waits for them stalls all lanes of the wave.  With the queue a
    //  wave pays that stall once per 64 walks, and no lane waits for a round: 70 % -> 95 % of the lanes have a gather in
    //  flight.
    // ================================================================================================
    constexpr int PEEL_QCAP = PMC_PEEL_QCAP;                    // queue entries per wave (a power of two)
    constexpr int PEEL_QBYTES = PEEL_QCAP * (6 * 8 + 8 + 3 * 4);  // rx ry rz ds target sext | P | cell bits slot
    // SGN: the sign pattern of the observer's direction (bit a: k_a < 0), a compile-time constant: one instantiation per octant
    template<bool WIDE, int SGN>
    __global__ __launch_bounds__(PMC_PEEL_BLOCK, PMC_PEEL2_MIN_WAVES) void walkPeelKernel2(const int sceneSlot, const int slotBase, const int numSlotsIn,
                                                                             const int cursor, const int obs, const int queueOffset,
                                                                             const int* const list, const PeelSortedArgs sorted)
    {
        // (sorted records, pmc_device.h PeelRec: as many tasks as the sort kept)
        const int numSlots = sorted.rec ? (int)*sorted.count : numSlotsIn;
        typedef typename Pack<WIDE>::T PT;
        constexpr int SGNX = SGN;
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        TreeConst C;
        const GridLds L = treeFrame<WIDE>(S, lds, C);
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const int64_t rec = (int64_t)(1 + obs) * A.num_slots;
        double* const ptau = A.ptau + (int64_t)obs * A.num_slots;
        const char* nodes = reinterpret_cast<const char*>(S.nodes);
        const double eps = S.eps;
        Dir d;
        observerDir(S.inst[obs], d);
        // the wave's queue of task records
        char* const qbase = reinterpret_cast<char*>(lds) + queueOffset + (tid >> 6) * PEEL_QBYTES;
        double* const qF = reinterpret_cast<double*>(qbase);                       // [6][PEEL_QCAP]
        unsigned long long* const qP = reinterpret_cast<unsigned long long*>(qF + 6 * PEEL_QCAP);
        uint32_t* const qCell = reinterpret_cast<uint32_t*>(qP + PEEL_QCAP);
        uint32_t* const qBits = qCell + PEEL_QCAP;
        int* const qSlot = reinterpret_cast<int*>(qBits + PEEL_QCAP);
        int qHead = 0, qCount = 0;  // wave-uniform
        uint32_t xcdSeg = xccId(), xcdTried = 0u;  // (sorted records) the segment of the tile order this wave takes its walks from

        TWalk<WIDE> w;
        CellLoad g;
        idleWalk(w, g);
        int slot = -1;
        int st = ST_IDLE;
        double sext = 0., target = 0.;
        bool exhausted = false;
        unsigned long long poolNext = 0, poolEnd = 0;
        unsigned long long visits = 0, waveSteps = 0, services = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
#ifdef PMC_PROFILE
        WalkProf prof = {{0, 0, 0, 0, 0, 0, 0, 0}, clock64(), {0, 0, 0, 0, 0, 0, 0, 0}};
#endif

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            const bool drained = exhausted && qCount == 0;
            if (drained && !activeMask && !pendingMask) break;
            // ---- round: when a few lanes wait (once nothing is left to hand out: as soon as a walk has ended)
            if (drained ? (pendingMask != 0ull) : (64 - __popcll(activeMask) >= PMC_PEEL2_REFILL))
            {
                services += 1;
                // undecided steps, finished walks
                bool fresh = treeServeUndecided<WIDE>(S, L, C, d, w, st PMC_WPROF_PASS);  // the lane takes up a cell whose record has not been requested yet
                peelStoreResult(ptau, slot, w.tau, st);
                // the queue is refilled with the records of the next 64 slots that hold a walk
                if (!exhausted && qCount <= PEEL_QCAP - 64)
                {
                    const int got = (sorted.rec && sorted.xcdCursor)
                                        ? claimSegmented(sorted.xcdCursor, (unsigned long long)numSlots, lane, true, poolNext, poolEnd, exhausted, xcdSeg, xcdTried)
                                        : claimSlots(S, cursor, (unsigned long long)numSlots, lane, true, poolNext, poolEnd, exhausted, list ? 64ull : (unsigned long long)PMC_TASK_CHUNK);
                    uint32_t bits = PMC_TASK_NONE;
                    int taken = -1;
                    uint4 r0, r1, r2, r3;
                    if (got >= 0)
                    {
                        if (sorted.rec)
                        {
                            const uint4* src = reinterpret_cast<const uint4*>(sorted.rec + got);
                            r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3];
                            bits = r3.y;
                            taken = (int)r3.z;
                        }
                        else
                        {
                            taken = list ? list[got] : slotBase + got;
                            bits = K.bits[rec + taken];
                        }
                    }
                    const bool keep = bits != PMC_TASK_NONE;
                    const unsigned long long km = __ballot(keep);
                    if (keep && sorted.rec)
                    {
                        const int pos = (qHead + qCount + __popcll(km & below)) & (PEEL_QCAP - 1);
                        qSlot[pos] = taken;
                        qBits[pos] = bits;
                        qCell[pos] = r3.x;
                        qP[pos] = (unsigned long long)r2.z | ((unsigned long long)r2.w << 32);
                        qF[0 * PEEL_QCAP + pos] = __hiloint2double((int)r0.y, (int)r0.x);
                        qF[1 * PEEL_QCAP + pos] = __hiloint2double((int)r0.w, (int)r0.z);
                        qF[2 * PEEL_QCAP + pos] = __hiloint2double((int)r1.y, (int)r1.x);
                        qF[3 * PEEL_QCAP + pos] = __hiloint2double((int)r1.w, (int)r1.z);
                        qF[4 * PEEL_QCAP + pos] = __hiloint2double((int)r2.y, (int)r2.x);
                        qF[5 * PEEL_QCAP + pos] = S.mono ? S.mono_ext : A.dustExt[taken];
                    }
                    else if (keep)
                    {
                        const int64_t t = rec + taken;
                        const int pos = (qHead + qCount + __popcll(km & below)) & (PEEL_QCAP - 1);
                        qSlot[pos] = taken;
                        qBits[pos] = bits;
                        qCell[pos] = (uint32_t)K.cell[t];
                        qP[pos] = K.pidx[t];
                        // (the walk starts at the slot's position unless moveInside has moved it)
                        const bool moved = (bits & PMC_TASK_MOVED) != 0u;
                        qF[0 * PEEL_QCAP + pos] = moved ? K.rx[t] : A.rx[taken];
                        qF[1 * PEEL_QCAP + pos] = moved ? K.ry[t] : A.ry[taken];
                        qF[2 * PEEL_QCAP + pos] = moved ? K.rz[t] : A.rz[taken];
                        qF[3 * PEEL_QCAP + pos] = K.ds[t];
                        qF[4 * PEEL_QCAP + pos] = K.target[t];
                        qF[5 * PEEL_QCAP + pos] = S.mono ? S.mono_ext : A.dustExt[taken];
                    }
                    qCount += __popcll(km);
                }
                // lanes without a walk take the next records of the queue
                const unsigned long long idle = __ballot(st == ST_IDLE);
                if (idle && qCount > 0)
                {
                    const int rank = __popcll(idle & below);
                    if (st == ST_IDLE && rank < qCount)
                    {
                        const int pos = (qHead + rank) & (PEEL_QCAP - 1);
                        slot = qSlot[pos];
                        const uint32_t bits = qBits[pos];
                        w.cell = qCell[pos];
                        setBox<WIDE>(w, (PT)qP[pos], (bits >> 8) & PMC_TASK_EXP_MASK);
                        w.rx = qF[0 * PEEL_QCAP + pos], w.ry = qF[1 * PEEL_QCAP + pos], w.rz = qF[2 * PEEL_QCAP + pos];
                        w.ds = qF[3 * PEEL_QCAP + pos];
                        target = qF[4 * PEEL_QCAP + pos];
                        sext = qF[5 * PEEL_QCAP + pos];
                        w.axis = (bits >> 2) & 3u;
                        w.tau = 0.;
                        st = ST_ACTIVE;
                        fresh = true;
                    }
                    const int taken = min(__popcll(idle), qCount);
                    qHead = (qHead + taken) & (PEEL_QCAP - 1);
                    qCount -= taken;
                }
                if (fresh) cellIssue(C, w.cell, g);
            }
            // ---- steps
#pragma unroll 1
            for (int it = 0; it < PMC_WALK_STEPS; ++it)
            {
                visits += (unsigned long long)__popcll(__ballot(st == ST_ACTIVE));
                waveSteps += 1;
                if (st == ST_ACTIVE)
                {
                    // (the head of the step, written out: the record counts as landed AFTER the position arithmetic.  Through treeStepHead this kernel was
                    // 7 % slower with cellLanded in front of the call and 2 % slower with it inside the helper -- profiles/sweeps/octree_step_once.md)
                    const double step = w.ds + eps;
                    StepHead h;  // (not plain locals: 0.4 ms, 2 %, slower, same file.  Fragile -- it is the allocator's answer to the source form: time any edit here)
                    h.nrx = w.rx + d.kx * step, h.nry = w.ry + d.ky * step, h.nrz = w.rz + d.kz * step;
#ifndef PMC_EXP_NARROW_LOADS
                    cellLanded(g);
#endif
                    h.link = cellLink<SGNX>(g, d, w.axis);
                    w.dens = cellDensity(g);
                    const double tau1 = w.tau + sext * w.dens * w.ds;
                    if (tau1 > target)
                        st = ST_HIT;
                    else
                    {
                        w.tau = tau1;
                        st = treeAdvance<WIDE, SGNX>(C, nodes, d, w, g, h.link, h.nrx, h.nry, h.nrz PMC_WPROF_PASS);
                    }
                }
            }
        }
        flushPeelWork(S, lane, visits, waveSteps, services);
#ifdef PMC_PROFILE
        flushWalkProf(S, lane, prof, 208, false);  // (the census only: this kernel has but the two stamps of treeAdvance, no phase breakdown)
#endif
    }

    // ================================================================================================
    //  propagation walks (task record 0) of the slots [slotBase, slotBase + numSlots) -- or, in a sparse generation, of the numSlots
    //  slots in `list` (TaskArrays::liveList)
    // ================================================================================================
    // Pass 2 without walking the whole path again: pass 1 keeps TWO walker states (nine doubles each) in LDS -- A, a state that is
    // CERTAIN to lie at or before the interaction point, and B, a later candidate -- and pass 2 resumes from the later one that turns
    // out to be valid once the interaction optical depth is known (else from the start of the path, whose state is still in the task
    // record).  The uniforms of simulateForcedPropagation are drawn BEFORE the walk (startCycle), so a lower bound of the sampled depth
    // is known while pass 1 runs: the sampled depth grows with the optical depth of the path, tau_path >= tau_c (the depth walked so
    // far), hence  tau* >= u tau_c  in the uniform branch of the path-length bias and  tau* >= u tau_c / (1 + tau_c)  in the exponential
    // one (-log(1 - x) >= x and 1 - e^-t >= t / (1 + t); the slack is of second order in tau, far above rounding, and the state that is
    // resumed from is checked against the sampled depth anyway).  Every PMC_WALK_STEPS steps (a wave-uniform tick) a lane whose bound
    // has passed B's depth makes B the new A and saves its current state as the new B: 2.7 saves and 5.9 re-walked segments per path
    // on configs[1] (counted with the oracle's paths), against 14.7 re-walked segments with the first five segments recorded (rounds 2-4)
    // and 19.1 without any record; 144 bytes of LDS per lane.  (ckptOffset < 0: no room in LDS, e.g. next to the coordinate table of a
    // 12-level octree: pass 2 walks the path from its start.)  Round 3 measured checkpoints in HBM (slower: their stores sit in the
    // step loop's in-order memory pipe); these never leave LDS.
    // The decisions (when B becomes A, which state pass 2 resumes from) are ckptTick and ckptResume in pmc_walk.inc, shared with voroPropKernel.
    constexpr int PROP_CKPT_BYTES = PMC_PROP_BLOCK * 2 * 9 * 8;
    // a checkpoint of a lane, q[field * PMC_PROP_BLOCK]; fields: position (3), tau, s, ds, bx | by << 32, cell | bz << 32, lastm | (axis | szb << 2) << 32
    template<bool WIDE> __device__ __forceinline__ void ckptSave(double* q, const TWalk<WIDE>& w)
    {
        q[0 * PMC_PROP_BLOCK] = w.rx, q[1 * PMC_PROP_BLOCK] = w.ry, q[2 * PMC_PROP_BLOCK] = w.rz;
        q[3 * PMC_PROP_BLOCK] = w.tau, q[4 * PMC_PROP_BLOCK] = w.s, q[5 * PMC_PROP_BLOCK] = w.ds;
        q[6 * PMC_PROP_BLOCK] = __longlong_as_double((long long)((unsigned long long)w.bx | ((unsigned long long)w.by << 32)));
        q[7 * PMC_PROP_BLOCK] = __longlong_as_double((long long)((unsigned long long)w.cell | ((unsigned long long)w.bz << 32)));
        q[8 * PMC_PROP_BLOCK] = __longlong_as_double((long long)((unsigned long long)(uint32_t)w.lastm | ((unsigned long long)(w.axis | (w.szb << 2)) << 32)));
    }
    template<bool WIDE> __device__ __forceinline__ void ckptLoad(const double* q, TWalk<WIDE>& w)
    {
        w.rx = q[0 * PMC_PROP_BLOCK], w.ry = q[1 * PMC_PROP_BLOCK], w.rz = q[2 * PMC_PROP_BLOCK];
        w.tau = q[3 * PMC_PROP_BLOCK], w.s = q[4 * PMC_PROP_BLOCK], w.ds = q[5 * PMC_PROP_BLOCK];
        const unsigned long long w6 = (unsigned long long)__double_as_longlong(q[6 * PMC_PROP_BLOCK]);
        const unsigned long long w7 = (unsigned long long)__double_as_longlong(q[7 * PMC_PROP_BLOCK]);
        const unsigned long long w8 = (unsigned long long)__double_as_longlong(q[8 * PMC_PROP_BLOCK]);
        w.bx = (uint32_t)w6, w.by = (uint32_t)(w6 >> 32);
        w.cell = (uint32_t)w7, w.bz = (uint32_t)(w7 >> 32);
        w.lastm = (int)(uint32_t)w8;
        w.axis = (uint32_t)(w8 >> 32) & 3u;
        w.szb = (uint32_t)(w8 >> 34);
    }

    // The wave's chunk of the group's log of radiation-field contributions (pmc_device.h RfLogArgs): wave-uniform.  The contributions go to
    // the log -- coalesced stores; partitioned by key range and summed in LDS after the generation (pmc_log.inc): as atomics into the table
    // (238 per history, every lane on a sector of its own) they cost 0.95 s per 1e8 packets, more than the walks themselves.
    struct RfLogWave
    {
        bool ok;                  // the log takes entries (false: none configured, or full -- atomics)
        unsigned long long base;  // first entry of the wave's chunk
        uint32_t fill;            // entries of it in use (PMC_RF_LOG_CHUNK: the wave holds no chunk yet)
    };
    // the contributions (key `at`: DEVICE numbering of the cells) of the lanes with `pending`, the wave converged: to its chunk, or, the log full, to the table
    __device__ __forceinline__ void rfLogAppend(const DevScene& S, const RfLogArgs& rl, RfLogWave& lw, int lane, bool pending, int64_t at, double value)
    {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) return;
        bool logged = false;
        if (lw.ok)
        {
            const uint32_t n = (uint32_t)__popcll(m);
            const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lw.fill + n > (uint32_t)PMC_RF_LOG_CHUNK)
            {
                // the rest of the chunk (fewer than n entries) is filled up, the next chunk claimed
                if (pending && lw.fill + rank < (uint32_t)PMC_RF_LOG_CHUNK) rl.keys[lw.base + lw.fill + rank] = rl.padKey;
                unsigned long long got = 0;
                if (lane == 0) got = atomicAdd(S.counters + rl.cursor, (unsigned long long)PMC_RF_LOG_CHUNK);
                got = __shfl(got, 0, 64);
                lw.fill = PMC_RF_LOG_CHUNK;
                if (got + PMC_RF_LOG_CHUNK > rl.cap)
                    lw.ok = false;  // (the log is full: atomics from here on)
                else
                {
                    lw.base = got;
                    lw.fill = 0;
                }
            }
            if (lw.ok)
            {
                if (pending)
                {
                    rl.keys[lw.base + lw.fill + rank] = (uint32_t)at;
                    rl.vals[lw.base + lw.fill + rank] = value;
                }
                lw.fill += n;
                logged = true;
            }
        }
        if (pending && !logged)
        {
            // (the caller's cell index is looked up here; for the log, when the sums are added to the table)
            const int64_t dev = at / S.rf_num_lambda;
            unsafeAtomicAdd(S.rf + ((int64_t)S.cell_ext[dev] * S.rf_num_lambda + (at - dev * S.rf_num_lambda)), value);
        }
    }
    // the unused rest of the wave's last chunk is filled up with pad keys
    __device__ __forceinline__ void rfLogEnd(const RfLogArgs& rl, const RfLogWave& lw, int lane)
    {
        if (rl.cap == 0ull) return;
        for (uint32_t i = lw.fill + (uint32_t)lane; i < (uint32_t)PMC_RF_LOG_CHUNK; i += 64u) rl.keys[lw.base + i] = rl.padKey;
    }
    // EA: the explicit-absorption photon cycle (see walkKernel in pmc_walk.inc): scattering and absorption optical depths apart, no pass-1
    // records (an interaction inside them would need the absorption depths as well)
    // MM: several medium components (see walkKernel in pmc_walk.inc): no pass-1 records either
    template<bool WIDE, bool RF, bool EA, bool MM>
    __global__ __launch_bounds__(PMC_PROP_BLOCK, PMC_PROP_MIN_WAVES) void walkPropKernel(const int sceneSlot, const int slotBase, const int numSlots,
                                                                            const int cursor, const uint64_t seed, const int ckptOffset,
                                                                            const RfLogArgs rfLog, const int* const list)
    {
        constexpr int SGNX = -1;  // (per-lane directions)
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        TreeConst C;
        const GridLds L = treeFrame<WIDE>(S, lds, C);
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const char* nodes = reinterpret_cast<const char*>(S.nodes);
        const double eps = S.eps;
        const bool force = S.force_scattering != 0;
        // the two pass-1 checkpoints of this lane: buffer b at ckState + b * 9 * PMC_PROP_BLOCK (ckptSave, ckptLoad)
        const bool ckpt = ckptOffset >= 0 && force && !EA && !MM;
        double* const ckState = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + (ckptOffset >= 0 ? ckptOffset : 0)) + tid;
        uint32_t ck = 0;            // the CK_ flags (pmc_walk.inc)
        double ckTauB = 0.;         // cumulative optical depth of state B
        double uni1 = 0., uni2 = 0.;  // the uniforms drawn for simulateForcedPropagation (see startCycle)

        TWalk<WIDE> w;
        CellLoad g;  // the record of w.cell (in flight, or landed) whenever the lane is ST_ACTIVE
        idleWalk(w, g);
        Dir d;
        d.kx = d.ky = d.kz = 0., d.ikx = d.iky = d.ikz = 0., d.sgn = 0;
        setDirMasks(d);
        int slot = -1;
        int st = ST_IDLE;
        int mode = MODE_NONE;
        double sext = 0., target = 0.;
        double ssca = 0., sabs = 0., tabs = 0.;  // (EA) cross sections of the walk, cumulative absorption optical depth
        double mx[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, msc[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, mab[PMC_MAX_MEDIA] = {0., 0., 0., 0.};  // (MM) per component
        uint32_t nseg = 0;  // segments of the current walk that the reference adds to its path
        uint32_t visits = 0, rewalks = 0, paths = 0;
        double rfL = 0., rfExtBeg = 1.;
        int rfEll = -1;
        RfLogWave logWave = {RF && rfLog.cap != 0ull, 0ull, PMC_RF_LOG_CHUNK};  // (RF; no chunk yet)
        bool exhausted = false;
        unsigned long long poolNext = 0, poolEnd = 0;  // wave-uniform
        unsigned long long waveSteps = 0, laneSteps = 0, services = 0;
#ifdef PMC_PROFILE
        WalkProf prof = {{0, 0, 0, 0, 0, 0, 0, 0}, clock64(), {0, 0, 0, 0, 0, 0, 0, 0}};
#endif

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            if (exhausted && !activeMask && !pendingMask) break;
            const bool service = exhausted ? (pendingMask != 0ull) : (64 - __popcll(activeMask) >= PMC_PROP_REFILL);
            PMC_WSTAMP(7);
            if (service)
            {
                services += 1;
                bool fresh = treeServeUndecided<WIDE>(S, L, C, d, w, st PMC_WPROF_PASS);  // the lane takes up a cell whose record has not been requested yet
                // ---- finished walks: the result, or pass 2 over the same path (`again`)
                bool again = false;
                bool resumed = false;  // pass 2 resumes from the state saved during pass 1
                double taupath = 0.;
                if (st == ST_HIT || st == ST_EXIT)
                {
                    if (st == ST_HIT)
                    {
                        nseg += 1;
                        storeInteraction<EA, MM>(S, A, slot, (int)w.cell, w.dens, w.ds, w.s, w.tau, tabs, target, force, sext, ssca, sabs, mx, msc, mab);
                    }
                    else if (mode == MODE_PASS1 && w.tau > 0.)
                    {
                        again = true;
                        taupath = w.tau;
                        // ---- simulateForcedPropagation between the two passes (MonteCarloSimulation.cpp:696-722): the interaction
                        // optical depth from the pre-drawn uniforms; the path-length-bias weight follows in the transition kernel
                        // (onCycleDone) from tau_path and the sampled depth
                        target = sampleForcedDepth(S, A, slot, seed, taupath, uni1, uni2);
                        paths += 1;
                        visits += nseg;
                        if (ckpt)
                        {
                            // pass 2 resumes from the later checkpoint that lies at or before the interaction point (A's depth waits in LDS)
                            const int from = ckptResume(ck, ckState[(((ck & CK_SEL) ^ 1u) * 9 + 3) * PMC_PROP_BLOCK], ckTauB, target);
                            if (from >= 0)
                            {
                                ckptLoad(ckState + from * 9 * PMC_PROP_BLOCK, w);
                                nseg = 0;
                                mode = MODE_PASS2;
                                st = ST_ACTIVE;
                                fresh = true;
                                again = false;
                                resumed = true;
                            }
                        }
                    }
                    else if (mode == MODE_PASS1)
                        A.mint[slot] = -1;  // tau_path <= 0: the packet cannot scatter, the history ends
                    else
                        storeWalkEnd<EA>(A, slot, force, w.lastm, w.s, tabs, [&](int m) { return S.leaves[m].density; });
                    if (!resumed)
                    {
                        if (mode == MODE_PASS2 && force)
                            rewalks += nseg;
                        else if (!(mode == MODE_PASS1 && taupath > 0.))  // (counted above)
                            visits += nseg;
                        st = ST_IDLE;
                    }
                }
                const int got = claimSlots(S, cursor, (unsigned long long)numSlots, lane, st == ST_IDLE && !again, poolNext, poolEnd, exhausted, list ? 64ull : (unsigned long long)PMC_TASK_CHUNK);
                if (got >= 0) slot = list ? list[got] : slotBase + got;
                PMC_WSTAMP(5);
                if (again || got >= 0)
                {
                    // the start state of the propagation walk (record 0): for a new slot, and again for pass 2
                    // (all fields of the record at once: one round trip; the first cell first, so that its record can be requested
                    // while the others are still on their way.  The cross sections -- loadSections -- follow once the flags have
                    // arrived, with the first cell's record: the first step waits for that record anyway)
                    const int64_t t = slot;
                    const uint32_t cell0 = (uint32_t)K.cell[t];
                    const uint32_t bits = K.bits[t];
                    // the uniforms drawn for simulateForcedPropagation by the transition kernel (see startCycle): they travel in
                    // the result fields of the walk
                    const double u1 = A.sint[slot], u2 = A.nint[slot];
                    const auto P0 = (typename Pack<WIDE>::T)K.pidx[t];
                    // (position and direction of the slot; the record holds the position only if moveInside has moved it)
                    const double rx0 = A.rx[slot], ry0 = A.ry[slot], rz0 = A.rz[slot];
                    const double kx0 = A.kx[slot], ky0 = A.ky[slot], kz0 = A.kz[slot];
                    // (forced scattering: every record is a pass 1, without a stop value)
                    const double ds0 = K.ds[t], target0 = force ? INFINITY : K.target[t];
                    double s0 = 0.;
                    if (bits != PMC_TASK_NONE)
                    {
                        w.cell = cell0;
                        fresh = true;
                        setBox<WIDE>(w, P0, (bits >> 8) & PMC_TASK_EXP_MASK);
                        w.rx = rx0, w.ry = ry0, w.rz = rz0;
                        if (bits & PMC_TASK_MOVED)
                        {
                            w.rx = K.rx[t], w.ry = K.ry[t], w.rz = K.rz[t];
                            s0 = K.s0[t];
                        }
                        d.kx = kx0, d.ky = ky0, d.kz = kz0;
                        // RN(1 / k) as setDirection forms it (pmc_walk.inc; the cycle start kernel found the first exit distance with
                        // the same values): NaN for an ignored axis
                        const double ignored = __longlong_as_double(0x7ff8000000000000ll);
                        d.ikx = (fabs(kx0) > 1e-15) ? 1. / kx0 : ignored;
                        d.iky = (fabs(ky0) > 1e-15) ? 1. / ky0 : ignored;
                        d.ikz = (fabs(kz0) > 1e-15) ? 1. / kz0 : ignored;
                        w.s = s0;
                        w.ds = ds0;
                        if (!again) target = target0;
                        w.axis = (bits >> 2) & 3u;
                        d.sgn = (bits >> 4) & 7u;
                        setDirMasks(d);
                        w.tau = 0.;
                        w.lastm = -1;
                        loadSections<EA, MM>(S, A, slot, sext, ssca, sabs, tabs, mx, msc, mab);
                        mode = bits & 3u;
                        nseg = 0;
                        st = ST_ACTIVE;
                        if (!again)
                        {
                            uni1 = u1, uni2 = u2;
                            ck = ckptStart(S, u1);
                        }
                    }
                    if (again)
                        mode = MODE_PASS2;  // (the same path again from its start, up to the depth sampled above)
                    else if (RF && st == ST_ACTIVE && mode == MODE_PASS1)
                        rfStart(S, A, slot, rfL, rfEll, rfExtBeg);
                }
                if (fresh) cellIssue(C, w.cell, g);
                PMC_WSTAMP(6);
            }
            // ---------------- checkpoints of the pass-1 walks (a wave-uniform tick, every PMC_WALK_STEPS steps)
            if (ckpt)
            {
                const bool p1 = st == ST_ACTIVE && mode == MODE_PASS1 && w.tau > 0.;
                if (p1 && ckptTick(ck, w.tau, ckTauB, uni2))
                {
                    ckptSave(ckState + (ck & CK_SEL) * 9 * PMC_PROP_BLOCK, w);
                    ckTauB = w.tau;
                }
            }
            // ---------------- walk steps
#pragma unroll 1
            for (int it = 0; it < PMC_WALK_STEPS; ++it)
            {
                laneSteps += (unsigned long long)__popcll(__ballot(st == ST_ACTIVE));
                waveSteps += 1;
                PMC_WSTAMP(7);
                bool rfPending = false;  // (RF) this lane has a contribution to the radiation field in this step
                int64_t rfAt = 0;
                double rfValue = 0.;
                if (st == ST_ACTIVE)
                {
                    const StepHead h = treeStepHead<WIDE, SGNX>(d, eps, w, g PMC_WPROF_PASS);
                    // the pending segment: MediumSystem.cpp:863-871 (pass 1), SpatialGridPath.cpp:177-196 (pass 2: stop in
                    // the first segment with tau > target), :988-1008 (non-forced)
                    const double ds = w.ds;
                    double tau1, tabs1;
                    segmentDepth<EA, MM>(S, (int)w.cell, w.dens, ds, w.tau, tabs, true, force, sext, ssca, sabs, mx, msc, mab, tau1, tabs1);
                    if (tau1 > target)
                        st = ST_HIT;
                    else
                    {
                        const double tau0 = w.tau;
                        const double tabs0 = tabs;
                        w.tau = tau1;
                        if (EA) tabs = tabs1;
                        w.s += ds;
                        // SpatialGridPath::addSegment keeps segments with ds > 0 only; the non-forced loop runs over every
                        // segment the generator emits
                        if (ds > 0. || !force)
                        {
                            w.lastm = (int)w.cell;
                            nseg += 1;
                        }
                        if (RF && mode == MODE_PASS1 && ds > 0.)
                        {
                            double extEnd;
                            const double value = rfSegment<EA>(rfL, rfExtBeg, tau0, tabs0, tau1, tabs1, ds, extEnd);
                            if (rfEll >= 0)
                            {
                                // (the contribution is handed over below, where the lanes of the wave have converged)
                                // (the key of the log counts cells in the DEVICE numbering: the caller's cell index is looked up when the
                                // sums are added to the table -- once per key and partition instead of once per step)
                                rfAt = (int64_t)w.cell * S.rf_num_lambda + rfEll;
                                rfValue = value;
                                rfPending = true;
                            }
                            rfExtBeg = extEnd;
                        }
                        st = treeAdvance<WIDE, SGNX>(C, nodes, d, w, g, h.link, h.nrx, h.nry, h.nrz PMC_WPROF_PASS);
                    }
                }
                // ---- the radiation-field contributions of this step (the lanes have converged)
                if (RF) rfLogAppend(S, rfLog, logWave, lane, rfPending, rfAt, rfValue);
            }
        }
        if (RF) rfLogEnd(rfLog, logWave, lane);
        flushWalkCounters(S, lane, paths, visits, rewalks);
        if (lane == 0 && waveSteps)
        {
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 3, waveSteps);
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 4, laneSteps);
            atomicAdd(S.counters + PMC_CTR_WALKWORK + 5, services);
        }
#ifdef PMC_PROFILE
        flushWalkProf(S, lane, prof, 216, true);
#endif
    }

