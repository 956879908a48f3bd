// pmc_walk_voro_run.inc -- the Voronoi kernels on the tables of runs (DevScene::vobs_run, vgen_run, vcone_run; included by pmc_kernels.hip
// after pmc_walk.inc, inside its anonymous namespace): PMC_VORO_RUN_LANES lanes per walk, every walk at its own place in its own cell.
// What voroPeelKernel and voroPropKernel have in common stands here once: the lanes of a walk, the claim of new walks, the scan step.

    // quad permutations of the lanes that share a walk: the value of lane ^ 1 / lane ^ 2
    __device__ __forceinline__ int quadXor1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false); }
    __device__ __forceinline__ int quadXor2(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false); }
    template<int MASK> __device__ __forceinline__ int quadXor(int v) { return MASK == 1 ? quadXor1(v) : quadXor2(v); }
    template<int MASK> __device__ __forceinline__ double quadXor(double v)
    {
        const long long b = __double_as_longlong(v);
        const uint32_t lo = (uint32_t)quadXor<MASK>((int)(uint32_t)b), hi = (uint32_t)quadXor<MASK>((int)(uint32_t)((unsigned long long)b >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }

    // lanes per walk: what bounds these kernels is the rate at which a CU's vector memory unit takes addresses (one per lane and load unless
    // neighbouring lanes read neighbouring words): the lanes of a walk read a group of entries with two coalesced loads and look at one
    // entry each.  Lane `lane & (RUN_LANES - 1)` of a walk; lane 0, its leader, writes the walk's results
    constexpr int RUN_LANES = PMC_VORO_RUN_LANES;
    static_assert(RUN_LANES == 2 || RUN_LANES == 4, "lanes per walk");
    constexpr unsigned long long RUN_LEADERS = RUN_LANES == 4 ? 0x1111111111111111ull : 0x5555555555555555ull;
    constexpr int RUN_NO_INDEX = -99;  // no exit (neighbours are >= 0, the domain walls -1..-6, "no entry" -7)

    // ---- the wave's place in the list of walks, which is cut into segments with a cursor each (wave-uniform)
    struct RunTasks
    {
        unsigned long long next = 0, end = 0;  // the chunk in hand
        uint32_t seg = 0u, tried = 0u;         // the segment the wave takes its chunks from (its XCD's to begin with), segments found used up
        bool exhausted = false;
    };
    // Walks for the idle walks of the wave (`idle`: the lanes of their leaders), as claimSegmented (pmc_walk.inc) with a run-time number of
    // segments and a caller's mask: chunks from segment T.seg until that is used up, then from the next one; all used up: exhausted.
    // The idle walk of rank r takes entry base + r of the list if r < the number returned.
    __device__ __forceinline__ unsigned long long runClaim(RunTasks& T, unsigned long long* cursors, unsigned long long numTasks, int segments, int lane,
                                                           unsigned long long idle, unsigned long long& base)
    {
        const int nidle = __popcll(idle);
        while (nidle && T.next >= T.end && !T.exhausted)
        {
            if (T.tried >= (uint32_t)segments)
            {
                T.next = T.end = 0;
                T.exhausted = true;
                break;
            }
            const unsigned long long lo = (numTasks * T.seg) / (uint32_t)segments, hi = (numTasks * (T.seg + 1u)) / (uint32_t)segments;
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(cursors + T.seg, (unsigned long long)PMC_TASK_CHUNK);
            got = __shfl(got, 0, 64);
            if (lo + got < hi)
            {
                T.next = lo + got;
                T.end = lo + got + PMC_TASK_CHUNK < hi ? lo + got + PMC_TASK_CHUNK : hi;
            }
            else
            {
                T.seg = T.seg + 1u < (uint32_t)segments ? T.seg + 1u : 0u;
                T.tried += 1u;
            }
        }
        base = T.next;
        const unsigned long long avail = T.end - T.next;
        T.next += (unsigned long long)nidle < avail ? (unsigned long long)nidle : avail;
        return avail;
    }

    // ---- the scan of a cell's run by the lanes of a walk.  A run (pmc_tables.h): the header -- site, density, number of entries -- and
    // groups of RUN_LANES entries, {x, y} of an entry at word `sub` of its group, {z, tag} RUN_LANES words on; the tag names the
    // neighbour (or wall) and that neighbour's run
    struct RunScan
    {
        uint32_t run = 0u;                               // the cell's run: its unit in the table | the number of entries as the link names it
        int q = 0, cnt = 0;                              // entries scanned so far (a multiple of RUN_LANES), entries of the cell
        double prx = 0., pry = 0., prz = 0., dens = 0.;  // the cell's site and density
        double sq = DBL_MAX;                             // this lane's nearest exit so far: distance, neighbour or wall, place in the list, and
        int mq = RUN_NO_INDEX, iq = 0x7fffffff;          // the neighbour's run
        uint32_t runq = 0u;
        __device__ __forceinline__ void enter(uint32_t r) { run = r, q = 0; }
    };
    // One scan step of the walk at r towards k in the cell of c.run: ROWS groups in one round trip (most cells have no more entries than that);
    // lane `sub` looks at entry q + e LANES + sub.  True after the cell's last group: every lane of the walk then holds the walk's exit
    // (c.sq, c.mq, c.runq; c.mq == RUN_NO_INDEX: the cell has none from here)
    template<int ROWS>
    __device__ __forceinline__ bool runScanStep(const DevScene& S, const double* runs, int sub, double rx, double ry, double rz, double kx, double ky,
                                                double kz, RunScan& c)
    {
        constexpr int LANES = RUN_LANES;
        const double* const cellRun = runs + 8 * (int64_t)(c.run & PMC_VORO_RUN_UNIT_MASK);
        const uint32_t linked = c.run >> PMC_VORO_RUN_UNIT_BITS;  // the number of entries as the link names it
        if (c.q == 0)
        {
            // the header: site, density, number of entries -- requested together with the first group behind it
            const double2 prxy = *reinterpret_cast<const double2*>(cellRun);
            const double2 przn = *reinterpret_cast<const double2*>(cellRun + 2);
            c.cnt = (int)linked;
            if (linked == PMC_VORO_RUN_COUNT_UNKNOWN) c.cnt = *reinterpret_cast<const int*>(cellRun + 4);
            c.prx = prxy.x, c.pry = prxy.y, c.prz = przn.x, c.dens = przn.y;
            c.sq = DBL_MAX;
            c.mq = RUN_NO_INDEX;
            c.iq = 0x7fffffff;
        }
        const double* const group = cellRun + 8 + 4 * c.q;  // (q: a multiple of LANES; 4 doubles per entry)
        double2 xy[ROWS], zi[ROWS];
#pragma unroll
        for (int e = 0; e < ROWS; ++e)
        {
            // (exactly the groups the cell has -- the link named their number --: groups beyond the run would be lines of other cells,
            // fetched from beyond L2 for nothing; a cell with more than 30 entries learns its number from the header, its first groups go
            // out unconditionally)
            // (no value: a group that is not requested is not looked at -- its candidate is "no entry" whatever the registers hold)
            asm volatile("" : "=v"(xy[e].x), "=v"(xy[e].y), "=v"(zi[e].x), "=v"(zi[e].y));
            if ((c.q == 0 && linked == PMC_VORO_RUN_COUNT_UNKNOWN) || c.q + e * LANES < c.cnt)
            {
                xy[e] = *reinterpret_cast<const double2*>(group + 4 * LANES * e + 2 * sub);
                zi[e] = *reinterpret_cast<const double2*>(group + 4 * LANES * e + 2 * LANES + 2 * sub);
            }
        }
#pragma unroll
        for (int e = 0; e < ROWS; ++e)
        {
            const long long tag = __double_as_longlong(zi[e].y);
            const int at = c.q + e * LANES + sub;
            const int before = c.mq;
            voroCandidatePair(S, rx, ry, rz, kx, ky, kz, c.prx, c.pry, c.prz, (at < c.cnt) ? (int)tag : -7, xy[e].x, xy[e].y, zi[e].x, c.sq, c.mq);
            if (c.mq != before) c.runq = (uint32_t)((unsigned long long)tag >> 32), c.iq = at;
        }
        c.q += ROWS * LANES;
        if (c.q < c.cnt) return false;
        // the smallest distance of the lanes' own (equal distances: the earlier entry of the list, as the reference's loop keeps it)
        {
            const double osq = quadXor<1>(c.sq);
            const int oiq = quadXor<1>(c.iq), omq = quadXor<1>(c.mq), orun = quadXor<1>((int)c.runq);
            if (osq < c.sq || (osq == c.sq && oiq < c.iq)) c.sq = osq, c.iq = oiq, c.mq = omq, c.runq = (uint32_t)orun;
        }
        if (LANES == 4)
        {
            const double osq = quadXor<2>(c.sq);
            const int oiq = quadXor<2>(c.iq), omq = quadXor<2>(c.mq), orun = quadXor<2>((int)c.runq);
            if (osq < c.sq || (osq == c.sq && oiq < c.iq)) c.sq = osq, c.iq = oiq, c.mq = omq, c.runq = (uint32_t)orun;
        }
        return true;
    }

    // a walk in a cell without an exit from its position (ST_SLOW): the literal algorithm (:1153-1164) on the plain tables, every lane of the
    // walk for itself with the same result.  True: the walk has a pending segment (length ds through `cell` of density dens, left through
    // ci) whose next cell's run has to be looked up; false: it has left the domain
    __device__ __forceinline__ bool voroSlowStep(const DevScene& S, double& rx, double& ry, double& rz, double kx, double ky, double kz, int& cell,
                                                 double& dens, double& ds, int& ci)
    {
        Walk w;
        w.rx = rx, w.ry = ry, w.rz = rz, w.kx = kx, w.ky = ky, w.kz = kz;
        if (!voroStepSlow(S, w)) return false;
        rx = w.rx, ry = w.ry, rz = w.rz;
        cell = w.cell, dens = w.dens, ds = w.ds, ci = w.ci;
        return true;
    }

    // ================================================================================================
    //  Voronoi: the peel-off walks towards ONE observer that has a table of runs (DevScene::vobs_run) as a kernel of their own.
    //  Of the generic kernel's lane state (three kinds of walks, two passes, sampling, records of a slot: 168 registers and scratch) such a
    //  walk needs position, depth, the pending segment and the next cell's run; the direction and the table are wave-uniform.  The walks
    //  come as the observer's list of slots in tile order (cycle start kernel), taken with the XCD affinity of the generic stream.
    //  MediumSystem::getExtinctionOpticalDepth (MediumSystem.cpp:1192-1260) on VoronoiMeshSnapshot::MySegmentGenerator (:1058-1188).
    // ================================================================================================
    // MM: several medium components (round 6): the extinction optical depth of a segment is summed over the components in order
    // (MediumSystem.cpp:1225-1242); the walk keeps the index of its cell for the densities of components 1.. (the header holds component 0's)
    template<bool MM>
    __global__ __launch_bounds__(256, PMC_VPEEL_MIN_WAVES) void voroPeelKernel(const int sceneSlot, const int rec, const int tab, const int32_t* __restrict__ list,
                                                                                const unsigned long long* __restrict__ count, unsigned long long* xcdCursor,
                                                                                const int segments)
    {
        const DevScene& S = c_scene[sceneSlot];
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const int lane = threadIdx.x & 63;
        const int sub = lane & (RUN_LANES - 1);
        const bool leader = sub == 0;
        const unsigned long long numTasks = *count;
        const DevInstrument& I = S.inst[rec - 1];
        const double kx = I.kx, ky = I.ky, kz = I.kz;  // (what the cycle start kernel wrote into every task record of this observer)
        const double* const runs = tab == 0 ? S.vobs_run[0] : tab == 1 ? S.vobs_run[1] : tab == 2 ? S.vobs_run[2] : S.vobs_run[3];
        const uint32_t* const starts = tab == 0 ? S.vobs_start[0] : tab == 1 ? S.vobs_start[1] : tab == 2 ? S.vobs_start[2] : S.vobs_start[3];
        // the lanes of a walk all carry the walk (position just inside the cell it scans, depth so far) and their part of the scan of that cell's
        // run (DevScene::vobs_run): one group of entries per step, every walk at its own place in its own cell -- no walk waits for the longest
        // list of the wave
        double rx = 0., ry = 0., rz = 0., tau = 0., target = 0., sext = 0.;
        RunScan c;
        int slot = -1;
        int cell = -1;  // (MM) the cell of the pending segment
        double mx[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, msc[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, mab[PMC_MAX_MEDIA] = {0., 0., 0., 0.};  // (MM) per component
        int st = ST_IDLE;
        uint32_t nseg = 0, visits = 0;
        RunTasks T;
        if (segments > 1) T.seg = xccId();

        // the pending segment (length len through a cell of density c.dens, left through neighbour or wall ci) joins the path
        // (MediumSystem.cpp:1207-1219: stop once tau >= taumax; every segment the generator emits counts), and the position moves to just beyond
        // its end (VoronoiMeshSnapshot.cpp:1169).  The run of the next cell: `next`, or table[ci] where the caller does not know it (looked up
        // only for a neighbour: ci may be a wall)
        const auto segment = [&](double len, int ci, const uint32_t* table, uint32_t next) __attribute__((always_inline)) {
            double tau1 = tau + sext * c.dens * len;
            if (MM)
            {
                double none = 0.;
                tau1 = tau;
                mediaSegment<false>(S, cell, c.dens, len, false, mx, msc, mab, tau1, none);
            }
            if (tau1 > target)
                st = ST_HIT;
            else
            {
                tau = tau1;
                nseg += 1;
                const double step = len + S.eps;
                rx += kx * step, ry += ky * step, rz += kz * step;
                if (ci < 0)
                    st = ST_EXIT;
                else
                {
                    if (MM) cell = ci;
                    c.enter(table ? table[ci] : next);
                    st = ST_ACTIVE;
                }
            }
        };

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            if (T.exhausted && !activeMask && !pendingMask) break;
            // ---------------- service: cells without an exit, finished walks, new walks (as the generic kernel's, for one kind of walk)
            if (T.exhausted ? (pendingMask != 0ull) : (64 - __popcll(activeMask) >= PMC_VPEEL_REFILL))
            {
                bool pending = false;  // a walk with a pending segment whose next cell's run has to be looked up
                double pds = 0.;
                int pci = -1;
                if (st == ST_SLOW)
                {
                    pending = voroSlowStep(S, rx, ry, rz, kx, ky, kz, cell, c.dens, pds, pci);
                    if (!pending) st = ST_EXIT;
                }
                if (st == ST_HIT || st == ST_EXIT)
                {
                    // tau >= taumax: the packet does not arrive (MediumSystem.cpp:1215-1218); else the depth of the whole path
                    if (leader)
                    {
                        A.ptau[(int64_t)(rec - 1) * A.num_slots + slot] = st == ST_HIT ? (double)INFINITY : tau;
                        visits += nseg + (st == ST_HIT ? 1u : 0u);
                    }
                    st = ST_IDLE;
                }
                if (!T.exhausted)
                {
                    const unsigned long long idle = __ballot(st == ST_IDLE) & RUN_LEADERS;
                    unsigned long long base;
                    const unsigned long long avail = runClaim(T, xcdCursor, numTasks, segments, lane, idle, base);
                    if (st == ST_IDLE && !T.exhausted)
                    {
                        // (the idle walks before this one in the wave: the lanes of a walk find the same rank)
                        const unsigned long long rank = __popcll(idle & ((1ull << (lane - sub)) - 1ull));
                        if (rank < avail)
                        {
                            slot = list[base + rank];
                            const int64_t t = (int64_t)rec * A.num_slots + slot;
                            if (K.bits[t] != PMC_TASK_NONE)
                            {
                                // the start state of the walk: position in its first cell, that cell's exit (cycle start kernel)
                                rx = K.rx[t], ry = K.ry[t], rz = K.rz[t];
                                pci = K.cijk[t];
                                target = K.target[t];
                                const int cell0 = K.cell[t];
                                if (MM)
                                {
                                    cell = cell0;
                                    for (int h = 0; h < S.num_media; ++h) mediumSections(S, A, slot, h, mx[h], msc[h], mab[h]);
                                }
                                sext = S.mono ? S.mono_ext : A.dustExt[slot];
                                tau = 0.;
                                nseg = 0;
                                if (pci == PMC_VORO_FIRST_SCAN)
                                {
                                    // (the cycle start kernel has located the first cell only: its scan is the first step of the walk)
                                    c.enter(starts[cell0]);
                                    st = ST_ACTIVE;
                                }
                                else
                                {
                                    pds = K.ds[t];
                                    c.dens = S.vsite[4 * (int64_t)cell0 + 3];
                                    pending = true;
                                }
                            }
                        }
                    }
                }
                if (pending) segment(pds, pci, starts, 0u);
            }
            // ---------------- scan steps: ROWS groups of entries of the walk's cell each; the last one of a cell ends its segment and enters
            // the next cell
#pragma unroll 1
            for (int it = 0; it < PMC_WALK_STEPS; ++it)
            {
                if (st == ST_ACTIVE && runScanStep<PMC_VPEEL_ROWS>(S, runs, sub, rx, ry, rz, kx, ky, kz, c))
                {
                    if (c.mq == RUN_NO_INDEX)
                        st = ST_SLOW;
                    else
                        segment(c.sq, c.mq, nullptr, c.runq);
                }
            }
        }
        const unsigned long long v = waveSum(visits);
        if (lane == 0 && v) atomicAdd(S.counters + 2, v);
    }

    // ================================================================================================
    //  Voronoi: the PROPAGATION walks (record 0 of the slots in `list`: the slots that have one, sorted by the sign octant of their direction) in the
    //  form of voroPeelKernel: two lanes per walk on the table of runs that holds ALL neighbours of a cell (DevScene::vgen_run: no mask, one run
    //  of memory per visit), every walk at its own place in its own cell.  Pass 1 over the whole path (setExtinctionOpticalDepths,
    //  MediumSystem.cpp:849-871), simulateForcedPropagation between the passes (MonteCarloSimulation.cpp:696-722), pass 2 from the start of the
    //  path up to the sampled depth (findInteractionPoint, SpatialGridPath.cpp:164-206); without forced scattering one walk up to the drawn depth.
    //  Flavours (round 6; rounds 4-5 ran them in walkKernel), as in the octree's propagation kernel: RF stores the radiation field along pass 1
    //  (MonteCarloSimulation.cpp:638-662; f64 atomics into the table: a Voronoi grid has no log), EA is the explicit-absorption cycle (scattering and
    //  absorption depths apart, MediumSystem.cpp:905-932, 1075-1110; no pass-1 checkpoints), MM sums a segment over several medium components
    //  (MediumSystem.cpp:874-887, 934-955; no checkpoints either).
    // ================================================================================================
    template<bool RF, bool EA, bool MM>
    __global__ __launch_bounds__(256, PMC_VPROP_MIN_WAVES) void voroPropKernel(const int sceneSlot, const int32_t* __restrict__ list,
                                                                                const unsigned long long* __restrict__ count, unsigned long long* xcdCursor,
                                                                                const int segments, const uint64_t seed)
    {
        const DevScene& S = c_scene[sceneSlot];
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const int lane = threadIdx.x & 63;
        constexpr int LANES = RUN_LANES;
        const int sub = lane & (LANES - 1);
        const bool leader = sub == 0;
        const unsigned long long numTasks = *count;
        // (the table of the walk's direction cone, or the one with all neighbours)
        const double* runs = S.vgen_run;
        const uint32_t* starts = S.vgen_start;
        const bool coneTables = S.vcone_run[0] != nullptr;
        const bool force = S.force_scattering != 0;
        double rx = 0., ry = 0., rz = 0., kx = 0., ky = 0., kz = 1., tau = 0., s = 0., ds = 0., target = 0., sext = 0.;
        RunScan c;
        int slot = -1, cell = -1, lastm = -1;
        int st = ST_IDLE;
        uint32_t mode = MODE_NONE;
        uint32_t nseg = 0, visits = 0, rewalks = 0, paths = 0;
        RunTasks T;
        if (segments > 1) T.seg = xccId();
        // pass 2 without walking the whole path again: the two walker states of the octree's propagation kernel (pmc_walk_tree.inc, there with the
        // derivation) -- A certainly at or before the interaction point, B a later candidate, advanced on a lower bound of the depth that will be
        // sampled (the uniforms are drawn before the walk) on a wave-uniform tick; pass 2 resumes from the later one that is valid for the depth
        // actually sampled.  A state = the walk between two cells (position in the cell it is about to scan, depth and length so far, that cell
        // and its run, the last cell of the path): valid at any moment, since a scan changes none of it.  In LDS, per walk.
        constexpr int WALKS = 256 / LANES;
        __shared__ double ckState[2 * 7 * WALKS];
        __shared__ double ckUniform[WALKS];
        const int walkIndex = (int)threadIdx.x / LANES;
        uint32_t ck = 0u;  // the CK_ flags (pmc_walk.inc, with the decisions: ckptStart, ckptTick, ckptResume)
        const bool checkpoints = force && S.voro_prop_checkpoints != 0 && !EA && !MM;
        double ssca = 0., sabs = 0., tabs = 0.;  // (EA) cross sections of the walk, cumulative absorption optical depth
        double mx[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, msc[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, mab[PMC_MAX_MEDIA] = {0., 0., 0., 0.};  // (MM) per component
        double rfL = 0., rfExtBeg = 1.;  // (RF) the packet's luminosity on this path, exp(-tau) at the start of the pending segment
        int rfEll = -1;

        // the pending segment (length len through `cell`, density c.dens, left through neighbour or wall ci): MediumSystem.cpp:863-871 (pass 1),
        // SpatialGridPath.cpp:177-196 (pass 2: stop in the first segment with tau > target), MediumSystem.cpp:988-1008 (non-forced); then the
        // position moves to just beyond its end (VoronoiMeshSnapshot.cpp:1169).  SpatialGridPath::addSegment keeps segments with ds > 0 only; the
        // non-forced loop runs over every segment the generator emits.  The next cell's run: as in voroPeelKernel
        const auto segment = [&](double len, int ci, const uint32_t* table, uint32_t next) __attribute__((always_inline)) {
            ds = len;
            double tau1 = tau + sext * c.dens * ds, tabs1 = 0.;
            if (MM)
            {
                tau1 = tau, tabs1 = tabs;
                mediaSegment<EA>(S, cell, c.dens, ds, true, mx, msc, mab, tau1, tabs1);
            }
            else if (EA)
            {
                const double ns = c.dens * ds;
                tau1 = force ? tau + ssca * ns : tau + ssca * c.dens * ds;
                tabs1 = tabs + sabs * ns;
            }
            if (tau1 > target)
                st = ST_HIT;
            else
            {
                const double tau0 = tau, tabs0 = tabs;
                tau = tau1;
                if (EA) tabs = tabs1;
                s += ds;
                if (ds > 0. || !force)
                {
                    lastm = cell;
                    nseg += 1;
                }
                if (RF && mode == MODE_PASS1 && ds > 0.)
                {
                    const double lnExtEnd = EA ? -(tau1 + tabs1) : -tau1;
                    const double extEnd = exp(lnExtEnd);
                    if (rfEll >= 0 && leader)
                        unsafeAtomicAdd(S.rf + ((int64_t)cell * S.rf_num_lambda + rfEll),
                                        rfL * lnmean(extEnd, rfExtBeg, lnExtEnd, EA ? -(tau0 + tabs0) : -tau0) * ds);
                    rfExtBeg = extEnd;
                }
                const double step = ds + S.eps;
                rx += kx * step, ry += ky * step, rz += kz * step;
                if (ci < 0)
                    st = ST_EXIT;
                else
                {
                    cell = ci;
                    c.enter(table ? table[ci] : next);
                    st = ST_ACTIVE;
                }
            }
        };

        while (true)
        {
            const unsigned long long activeMask = __ballot(st == ST_ACTIVE);
            const unsigned long long pendingMask = __ballot(st != ST_ACTIVE && st != ST_IDLE);
            if (T.exhausted && !activeMask && !pendingMask) break;
            // ---------------- service: cells without an exit, finished walks (results; pass 1 -> pass 2), new walks
            if (T.exhausted ? (pendingMask != 0ull) : (64 - __popcll(activeMask) >= PMC_VPROP_REFILL))
            {
                bool pending = false;  // a walk with a pending segment whose next cell's run has to be looked up
                double pds = 0.;
                int pci = -1;
                if (st == ST_SLOW)
                {
                    pending = voroSlowStep(S, rx, ry, rz, kx, ky, kz, cell, c.dens, pds, pci);
                    if (!pending) st = ST_EXIT;
                }
                bool again = false;
                double taupath = 0.;
                if (st == ST_HIT || st == ST_EXIT)
                {
                    const double dens = c.dens;
                    if (st == ST_HIT)
                    {
                        // findInteractionPoint (SpatialGridPath.cpp:177-196): first segment with tau > target
                        nseg += 1;
                        if (leader)
                        {
                            const double s1 = s + ds;
                            A.mint[slot] = cell;
                            if (MM)
                            {
                                double tau1 = tau, tabs1 = tabs;
                                mediaSegment<EA>(S, cell, dens, ds, true, mx, msc, mab, tau1, tabs1);
                                const double f = (target - tau) / (tau1 - tau);
                                A.nint[slot] = EA ? tabs + f * (tabs1 - tabs) : dens;
                                A.sint[slot] = s + f * (s1 - s);
                            }
                            else if (EA)
                            {
                                // (the absorption depth at the interaction point: as walkKernel forms it)
                                const double ns = dens * ds;
                                const double tau1 = force ? tau + ssca * ns : tau + ssca * dens * ds;
                                const double f = (target - tau) / (tau1 - tau);
                                A.nint[slot] = force ? tabs + f * ((tabs + sabs * ns) - tabs) : target * sabs / ssca;
                                A.sint[slot] = s + f * (s1 - s);
                            }
                            else
                            {
                                const double tau1 = tau + sext * dens * ds;
                                A.nint[slot] = dens;
                                A.sint[slot] = s + ((target - tau) / (tau1 - tau)) * (s1 - s);
                            }
                        }
                    }
                    else if (mode == MODE_PASS1 && tau > 0.)
                    {
                        again = true;
                        taupath = tau;
                    }
                    else if (leader)
                    {
                        if (mode != MODE_PASS1 && force && lastm >= 0)
                        {
                            // beyond the last segment (SpatialGridPath.cpp:198-204)
                            A.mint[slot] = lastm;
                            A.sint[slot] = s;
                            A.nint[slot] = EA ? tabs : S.vsite[4 * (int64_t)lastm + 3];
                        }
                        else
                            A.mint[slot] = -1;  // tau_path <= 0, or no forced scattering: the history ends / the packet escapes
                    }
                    if (leader)
                    {
                        if (mode == MODE_PASS2 && force)
                            rewalks += nseg;
                        else
                            visits += nseg;
                    }
                    st = ST_IDLE;
                }
                // ---- new walks for the idle pairs
                bool refill = false;
                if (!T.exhausted)
                {
                    const unsigned long long idle = __ballot(st == ST_IDLE && !again) & RUN_LEADERS;
                    unsigned long long base;
                    const unsigned long long avail = runClaim(T, xcdCursor, numTasks, segments, lane, idle, base);
                    if (st == ST_IDLE && !again && !T.exhausted)
                    {
                        const unsigned long long rank = __popcll(idle & ((1ull << (lane - sub)) - 1ull));
                        if (rank < avail)
                        {
                            slot = list[base + rank];
                            refill = true;
                        }
                    }
                }
                // ---- the start state in task record 0: for a new walk, and again for pass 2 over the same path
                if (again || refill)
                {
                    const int64_t t = slot;
                    const uint32_t bits = K.bits[t];
                    bool resumed = false;
                    if (again)
                    {
                        // simulateForcedPropagation between the two passes: the whole path has been walked; the interaction optical depth follows
                        // from the uniforms the transition kernel drew (startCycle), which wait in the result fields
                        double drawn = 0.;
                        if (leader) drawn = sampleForcedDepth(S, A, slot, seed, taupath, A.sint[slot], A.nint[slot]);
                        const double other = quadXor<1>(drawn);
                        target = (lane & 1) ? other : drawn;
                        if (LANES == 4)
                        {
                            const double other2 = quadXor<2>(target);
                            target = (lane & 2) ? other2 : target;
                        }
                        mode = MODE_PASS2;
                        if (leader) paths += 1;
                        // the later state that is valid for this depth: nothing before it can be the interaction segment if its depth has not
                        // passed the sampled one
                        const int b = (int)(ck & CK_SEL);
                        const int from = ckptResume(ck, ckState[((b ^ 1) * 7 + 3) * WALKS + walkIndex], ckState[(b * 7 + 3) * WALKS + walkIndex], target);
                        if (from >= 0)
                        {
                            const double* const p = ckState + from * 7 * WALKS + walkIndex;
                            rx = p[0 * WALKS], ry = p[1 * WALKS], rz = p[2 * WALKS];
                            tau = p[3 * WALKS], s = p[4 * WALKS];
                            const unsigned long long cr = (unsigned long long)__double_as_longlong(p[5 * WALKS]);
                            cell = (int)(uint32_t)cr;
                            c.enter((uint32_t)(cr >> 32));
                            lastm = (int)(uint32_t)(unsigned long long)__double_as_longlong(p[6 * WALKS]);
                            nseg = 0;
                            st = ST_ACTIVE;
                            resumed = true;
                        }
                    }
                    else
                    {
                        mode = bits & 3u;
                        target = K.target[t];
                        sext = S.mono ? S.mono_ext : A.dustExt[slot];
                        ck = 0u;
                        if (checkpoints && mode == MODE_PASS1 && bits != PMC_TASK_NONE)
                        {
                            // (the uniforms of this path's sampling wait in the result fields: startCycle)
                            const double u1 = A.sint[slot], u2 = A.nint[slot];
                            ck = ckptStart(S, u1);
                            if (leader) ckUniform[walkIndex] = u2;
                        }
                    }
                    if (EA)
                    {
                        ssca = S.mono ? S.mono_sca : A.dustSca[slot];
                        sabs = S.mono ? S.mono_abs : A.dustAbs[slot];
                        tabs = 0.;
                    }
                    if (MM)
                        for (int h = 0; h < S.num_media; ++h) mediumSections(S, A, slot, h, mx[h], msc[h], mab[h]);
                    if (RF && !again && mode == MODE_PASS1 && bits != PMC_TASK_NONE)
                    {
                        // the packet's luminosity and bin on this path (MonteCarloSimulation.cpp:638-662)
                        rfL = A.W[slot] / (S.mono ? S.mono_lambda : A.lambda[slot]);
                        rfEll = A.rfell[slot];
                        rfExtBeg = 1.;
                    }
                    if (bits != PMC_TASK_NONE && !resumed)
                    {
                        rx = K.rx[t], ry = K.ry[t], rz = K.rz[t];
                        kx = K.kx[t], ky = K.ky[t], kz = K.kz[t];
                        if (coneTables)
                        {
                            const int cone = voroCone(kx, ky, kz) >> 2;  // (the main cone of the four sub-cones of DevScene::vcull)
                            runs = S.vcone_run[cone];
                            starts = S.vcone_start[cone];
                        }
                        s = K.s0[t];
                        pci = K.cijk[t];
                        cell = K.cell[t];
                        tau = 0.;
                        lastm = -1;
                        nseg = 0;
                        if (pci == PMC_VORO_FIRST_SCAN)
                        {
                            // (the cycle start kernel has located the first cell only: its scan is the first step of the walk)
                            c.enter(starts[cell]);
                            st = ST_ACTIVE;
                        }
                        else
                        {
                            pds = K.ds[t];
                            c.dens = S.vsite[4 * (int64_t)cell + 3];
                            pending = true;
                        }
                    }
                }
                if (pending) segment(pds, pci, starts, 0u);
            }
            // ---------------- checkpoints of the pass-1 walks (a wave-uniform tick, every PMC_VPROP_STEPS scan steps)
            if (checkpoints)
            {
                // (B's depth and the path's uniform wait in LDS)
                const bool p1 = st == ST_ACTIVE && mode == MODE_PASS1 && tau > 0.;
                if (p1 && ckptTick(ck, tau, ckState[((int)(ck & CK_SEL) * 7 + 3) * WALKS + walkIndex], ckUniform[walkIndex]) && leader)
                {
                    double* const p = ckState + (int)(ck & CK_SEL) * 7 * WALKS + walkIndex;
                    p[0 * WALKS] = rx, p[1 * WALKS] = ry, p[2 * WALKS] = rz;
                    p[3 * WALKS] = tau, p[4 * WALKS] = s;
                    p[5 * WALKS] = __longlong_as_double((long long)((unsigned long long)(uint32_t)cell | ((unsigned long long)c.run << 32)));
                    p[6 * WALKS] = __longlong_as_double((long long)(unsigned long long)(uint32_t)lastm);
                }
            }
            // ---------------- scan steps: ROWS groups of entries of the walk's cell each, ROWS entries per lane; the last one of a cell ends its
            // segment and enters the next cell
#pragma unroll 1
            for (int it = 0; it < PMC_VPROP_STEPS; ++it)
            {
                if (st == ST_ACTIVE && runScanStep<PMC_VPROP_ROWS>(S, runs, sub, rx, ry, rz, kx, ky, kz, c))
                {
                    if (c.mq == RUN_NO_INDEX)
                        st = ST_SLOW;
                    else
                        segment(c.sq, c.mq, nullptr, c.runq);
                }
            }
        }
        flushWalkCounters(S, lane, paths, visits, rewalks);
    }
