// pmc_cycle.inc -- the start of a cycle (included by pmc_kernels.hip inside its anonymous namespace).
//
// Which observers get a peel-off packet (announceCycle: transition and launch kernels), the start state of every walk of the
// cycle (prepareWalk, startCycleWalks: cycleStartKernel), and the counting sort that puts the walks' records in tile order
// (peelSortCountKernel, peelSortOffsetsKernel, with cycleStartKernel as the scatter pass).

    enum Event : int { EV_NONE = 0, EV_LAUNCH = 1, EV_CYCLE_DONE = 2, EV_TASK = 5, EV_DEAD = 6 };

    // A history advances in CYCLES: at the start of a cycle (after the launch, or after a scattering event) the packet
    // sits at a position r with a propagation direction k, and all walks of the cycle start from r:
    //      record 0        the propagation walk along k (pass 1 + pass 2 for forced scattering, continued inside the walk
    //                      kernel; one walk for the non-forced mode)
    //      record 1 + g    the peel-off walk towards the observer whose instrument group starts at instrument g
    // Their start states go to the slot's task records (index record * num_slots + slot), the walk kernel runs them one
    // after the other in one lane, and the transition kernel then sees the whole cycle at once: it records the peel-off
    // detections, performs the interaction found by the propagation walk, and starts the next cycle.  A history
    // therefore costs ONE generation per scattering event.

    // The first observer at or after instrument g (g starts an observer group) for which FluxRecorder::detect would ask
    // for the optical depth: some instrument of the group records the packet (FluxRecorder.cpp:310-327: detect returns
    // before the optical depth is needed if the packet misses the frame of an instrument without SED, or if its
    // wavelength falls outside the instrument's grid).  Returns num_instruments if no observer is left.
    // EMISSION (a scene with a moving source, emission cycle): the bins of the observers' own wavelengths (SlotArrays::obsEll)
    template<bool EMISSION = false>
    __device__ __forceinline__ int nextObserver(const DevScene& S, int slot, double rx, double ry, double rz, int g)
    {
        const SlotArrays& A = S.slots;
        while (g < S.num_instruments)
        {
            bool need = false;
            int j = g;
            do
            {
                const DevInstrument& I = S.inst[j];
                const bool seen = (I.include_sed && insideAperture(I, rx, ry, rz)) || (I.include_ifu && pixelOnDetector(I, rx, ry, rz) >= 0);
                if (seen && (EMISSION ? A.obsEll[(int64_t)j * A.num_slots + slot] : S.mono ? S.inst[j].mono_ell : A.ell[(int64_t)j * A.num_slots + slot]) >= 0)
                    need = true;
                ++j;
            } while (j < S.num_instruments && S.inst[j].same_observer);
            if (need) return g;
            g = j;
        }
        return g;
    }

    // Start of one walk of a cycle: the State::Unknown branch of the path generator (PathSegmentGenerator::moveInside,
    // location of the first cell, first exit distance); the start state goes to task record `record` of the slot.  A
    // path without cell segments is resolved at once: its result is written and the record is marked empty.
    // hint: octree leaf that probably contains r (updated with the cell found).
    constexpr int PEEL_SORT_TILE = 2048;  // slots per sort tile of the sorted peel-off records (one workgroup pass of the count and cycle start kernels)
    // sort partition of a peel-off walk that starts at r towards the observer of instrument I: the tile of the plane through the grid's
    // centre perpendicular to the line of sight (the axes of FrameInstrument::pixelOnDetector, FrameInstrument.cpp:45-65, without roll; the
    // plane spans the grid's diagonal: PeelSortArgs::centre, scale)
    // (The count pass -- peelSortCountKernel -- and the scatter pass -- the cycle start kernel -- must find the SAME tile for a slot:
    // both call this function on the same stored doubles, and the engine is built with -ffp-contract=off, so the two instantiations
    // round alike.  A slot that the two passes would place differently runs a cursor over the end of its partition; a place beyond
    // the records' capacity is refused and counted (DevScene::counters[7]): pmc_run_primary then fails instead of writing out of bounds.)
    __device__ __forceinline__ uint32_t peelTile(const PeelSortArgs& ps, const DevInstrument& I, double x, double y, double z)
    {
        x -= ps.centre[0], y -= ps.centre[1], z -= ps.centre[2];
        const double xpp = -I.sinphi * x + I.cosphi * y;
        const double ypp = -I.cosphi * I.costheta * x - I.sinphi * I.costheta * y + I.sintheta * z;
        int tx = (int)(xpp * ps.scale + 0.5 * PMC_PEEL_TILES), ty = (int)(ypp * ps.scale + 0.5 * PMC_PEEL_TILES);
        tx = tx < 0 ? 0 : tx >= PMC_PEEL_TILES ? PMC_PEEL_TILES - 1 : tx;
        ty = ty < 0 ? 0 : ty >= PMC_PEEL_TILES ? PMC_PEEL_TILES - 1 : ty;
        return (uint32_t)(ty * PMC_PEEL_TILES + tx);
    }
    // sort partition of a PROPAGATION walk (Cartesian, Voronoi; PeelSortArgs::propIndex): the sign octant of its direction -- with the XCD
    // affinity of the walk stream an XCD then runs the walks of about one octant -- times the block of a 4 x 4 x 4 division of the grid
    // that the walk starts in: the walks in flight on an XCD at a time start in one region and head the same way.  (Count and scatter pass
    // call this on the same stored doubles: see peelTile.)
#ifndef PMC_PROP_KEY_CONES
#define PMC_PROP_KEY_CONES 1  // (configs[4]: walk kernels 506 -> 494 ms per 2e7 packets, profiles/sweeps/r05_i13)
#endif
#ifndef PMC_PROP_KEY_BLOCKS
#define PMC_PROP_KEY_BLOCKS 1  // (with octants, 1 / 2 / 4 blocks per axis on configs[4]: 2.245 / 2.21 / 2.22e7 packets/s; no list: 2.14e7 -- profiles/sweeps/r05_g2; with cones 1 / 2: the same -- r05_i14; keys x blocks^3 must stay below PMC_PEEL_TILES^2)
#endif
    __device__ __forceinline__ uint32_t propSortKey(const DevScene& S, double x, double y, double z, double kx, double ky, double kz)
    {
#if PMC_PROP_KEY_CONES
        // (Voronoi: the main direction cone -- octant-major, so the eighths of the XCD affinity stay octants -- : an XCD then works through one cone
        // table of voroPropKernel after the other instead of six at a time)
        const uint32_t oct = S.grid_kind == PMC_GRID_VORONOI ? (uint32_t)(voroCone(kx, ky, kz) >> 2)
                                                             : (kx < 0. ? 1u : 0u) | (ky < 0. ? 2u : 0u) | (kz < 0. ? 4u : 0u);
#else
        const uint32_t oct = (kx < 0. ? 1u : 0u) | (ky < 0. ? 2u : 0u) | (kz < 0. ? 4u : 0u);
#endif
        constexpr int B = PMC_PROP_KEY_BLOCKS;
        int ix = (int)((x - S.gx0) / (S.gx1 - S.gx0) * B), iy = (int)((y - S.gy0) / (S.gy1 - S.gy0) * B), iz = (int)((z - S.gz0) / (S.gz1 - S.gz0) * B);
        ix = ix < 0 ? 0 : ix >= B ? B - 1 : ix;
        iy = iy < 0 ? 0 : iy >= B ? B - 1 : iy;
        iz = iz < 0 ? 0 : iz >= B ? B - 1 : iz;
        return oct * (uint32_t)(B * B * B) + (uint32_t)((iz * B + iy) * B + ix);
    }
    // returns whether the walk exists (false: it ended before it began, its result is in place)
    template<int GRID>
    __device__ __forceinline__ bool prepareWalk(const DevScene& S, const GridLds& G, Counters& cnt, int slot, int record, int mode,
                                                double rx, double ry, double rz, double kx, double ky, double kz, double target,
                                                double sext, int& hint, PeelRec* sortedOut = nullptr, bool deferScan = false)
    {
        const SlotArrays& A = S.slots;
        const TaskArrays& K = S.tasks;
        const int64_t t = (int64_t)record * A.num_slots + slot;
        Walk w;
        w.rx = rx, w.ry = ry, w.rz = rz;
        setDirection(w, kx, ky, kz);
        // the walk kernel tests `tau > target` only: a pass-1 walk never stops inside the grid, and a peel-off walk
        // stops once tau >= taumax, i.e. tau > the double just below taumax
        if (mode == MODE_PASS1) target = INFINITY;
        const bool zeroPeel = mode == MODE_PEEL && target == -INFINITY;
        if (mode == MODE_PEEL && !zeroPeel) target = nextAfterToward(target, true);
        cnt.paths += 1;
        int located;
        const bool ok = startWalk<GRID>(S, G, w, (GRID == GRID_CART) ? -1 : hint, located, GRID == GRID_VORO && deferScan);
        if ((GRID == GRID_TREE || GRID == GRID_BIN) && located >= 0) hint = located;
        if (zeroPeel || !ok)
        {
            if (record == 0)
                A.mint[slot] = -1;  // no propagation: the history ends (or the packet escapes)
            else
                A.ptau[(int64_t)(record - 1) * A.num_slots + slot] = zeroPeel ? INFINITY : 0.;  // MediumSystem.cpp:1195-1196
            if (GRID == GRID_TREE && sortedOut)
                reinterpret_cast<uint4*>(sortedOut)[3] = make_uint4(0u, PMC_TASK_NONE, (uint32_t)slot, 0u);  // (its place in the sorted records stays empty)
            else
                K.bits[t] = PMC_TASK_NONE;
            return false;
        }
        if (GRID == GRID_TREE && sortedOut)
        {
            // (sorted peel-off records, pmc_device.h PeelRec: the start state goes to its place in tile order: one 64-byte record)
            const uint32_t bits = (uint32_t)mode | ((uint32_t)w.axis << 2) | (w.sgn << 4) | (w.e << 8);
            uint4* out = reinterpret_cast<uint4*>(sortedOut);
            const double2 a = make_double2(w.rx, w.ry), b = make_double2(w.rz, w.ds);
            const unsigned long long tbits = (unsigned long long)__double_as_longlong(target), P = (unsigned long long)w.P;
            out[0] = *reinterpret_cast<const uint4*>(&a);
            out[1] = *reinterpret_cast<const uint4*>(&b);
            out[2] = make_uint4((uint32_t)tbits, (uint32_t)(tbits >> 32), (uint32_t)P, (uint32_t)(P >> 32));
            out[3] = make_uint4((uint32_t)w.cell, bits, (uint32_t)slot, 0u);
            return true;
        }
        // octree: a walk that starts inside the grid -- nearly every walk -- starts at the slot's position, and a propagation walk
        // has the slot's direction: the octree walk kernels read both from the slot arrays, and the record holds the position (and
        // the length of the way to the grid) only if moveInside has moved it (PMC_TASK_MOVED)
        const bool moved = GRID != GRID_TREE || w.s != 0. || w.rx != rx || w.ry != ry || w.rz != rz;
        if (moved)
        {
            K.rx[t] = w.rx, K.ry[t] = w.ry, K.rz[t] = w.rz;
            // (an octree peel-off walk runs in the kernel of its observer: direction from the scene, no path length)
            if (GRID != GRID_TREE || record == 0) K.s0[t] = w.s;
        }
        if (GRID != GRID_TREE) K.kx[t] = w.kx, K.ky[t] = w.ky, K.kz[t] = w.kz;
        if (GRID == GRID_TREE) K.pidx[t] = w.P;
        K.ds[t] = w.ds;
        // (pass 1 of a forced-scattering propagation walk has no stop value: the octree propagation kernel does not read it)
        if (!(GRID == GRID_TREE && mode == MODE_PASS1)) K.target[t] = target;
        K.cell[t] = w.cell;
        K.bits[t] = (uint32_t)mode | ((uint32_t)w.axis << 2) | (w.sgn << 4) | ((GRID == GRID_TREE ? w.e : 0u) << 8)
                    | ((GRID == GRID_TREE && moved) ? PMC_TASK_MOVED : 0u);
        if (GRID == GRID_VORO) K.cijk[t] = w.ci;  // the neighbour (or wall) through which the path leaves the first cell
        return true;
    }

    // Start of a cycle at position r, first part (no grid needed): which observers get a peel-off packet and with what weight
    // (MonteCarloSimulation.cpp:617-634 peelOffEmission for pscatt == 0, :784-842 peelOffScattering with the phase function of
    // the INCOMING direction otherwise), and the random numbers of the propagation.  The walks themselves -- one towards every
    // such observer, one along the propagation direction -- are started by cycleStartKernel from the slot's state.
    // Several medium components: `shares` holds every component's share of the scattering opacity in the interaction cell and
    // `asyms` its asymmetry parameter; the peel-off weight is the sum of the components' phase functions weighted by the shares
    // (MediumSystem::peelOffScattering, consolidated form, MediumSystem.cpp:734-767; components with share 0 are skipped).
    template<bool DIPOLE = false, bool EMISSION = false>
    __device__ __forceinline__ void announceCycle(const DevScene& S, int slot, uint64_t seed, Rng& rng, double rx, double ry, double rz, double kinx,
                                                  double kiny, double kinz, double W, double asym, int pscatt, const double* shares = nullptr,
                                                  const double* asyms = nullptr, const DevSource* emitter = nullptr)
    {
        const SlotArrays& A = S.slots;
        const int64_t NS = A.num_slots;
        uint32_t pmask = 0;
        int g = nextObserver<EMISSION>(S, slot, rx, ry, rz, 0);
        for (int i = 0; i < S.num_instruments; ++i)
        {
            if (i != g) continue;
            const DevInstrument& I = S.inst[i];
            double pW = W;
            if (pscatt != 0 && shares)
            {
                const double costheta = kinx * I.kx + kiny * I.ky + kinz * I.kz;
                double sum = 0.;
                for (int h = 0; h < S.num_media; ++h)
                    if (shares[h] > 0.)
                    {
                        const double value = phaseValue<DIPOLE>(S, h, asyms[h], costheta);
                        sum += value * shares[h];
                    }
                pW = W * sum;
            }
            else if (pscatt != 0)
                pW = W * scatteringPeelFactor<DIPOLE>(S, asym, kinx, kiny, kinz, I);
            else if (emitter)
                pW = W * angularProbability(*emitter, I.kx, I.ky, I.kz);  // (an anisotropic point source: PhotonPacket::launchEmissionPeelOff)
            A.ppW[(int64_t)i * NS + slot] = pW;
            pmask |= 1u << i;
            int j = i + 1;
            while (j < S.num_instruments && S.inst[j].same_observer) ++j;
            g = nextObserver<EMISSION>(S, slot, rx, ry, rz, j);
        }
        if (!S.force_scattering)
            // the interaction optical depth is drawn now (Random::expon, MonteCarloSimulation.cpp:746-752); it travels in
            // SlotArrays::tausample, which the non-forced mode does not use otherwise
            A.tausample[slot] = -log(rngUniform(rng, seed));
        else
        {
            // the uniforms that simulateForcedPropagation will consume between the two passes
            // (MonteCarloSimulation.cpp:709-722: `uniform() < xi`, then the uniform or exponential deviate) are drawn
            // here, in stream order, so that the walk kernel needs no generator; they travel in the result fields of the
            // propagation walk, which are written only when that walk ends.  (A rejection round of exponCutoff, which
            // only rounding can cause, continues the stream in the walk kernel.)
            if (S.path_length_bias != 0.) A.sint[slot] = rngUniform(rng, seed);
            A.nint[slot] = rngUniform(rng, seed);
        }
        A.mode[slot] = MODE_ALIVE | (int)(pmask << 8);
    }

    // Start of a cycle, second part: the walks.  All of them start at the slot's position; a peel-off walk needs the weight
    // of its packet (taumax of MediumSystem::getExtinctionOpticalDepth), the propagation walk the direction.
    // returns the walks that exist: bit 1 + i = the peel-off walk towards observer i, bit 0 = the propagation walk
    // KIN (a scene with a moving source): in the emission cycle the packet towards observer i has its own wavelength -- its own taumax --
    // and its own cross section sigma_i.  The peel-off walk kernels are the ones every scene runs: they sum the optical depth with the
    // PACKET's cross section sigma (SlotArrays::dustExt).  With ONE medium component the two depths of a path differ by the factor
    // sigma_i / sigma, so the walk gets the stop value taumax sigma / sigma_i, and onCycleDone multiplies the depth it finds by sigma_i / sigma
    // (both exactly 1 where the cross sections agree; otherwise two roundings on a sum of thousands).  sigma = 0 < sigma_i leaves
    // nothing to scale: counted as an internal error (DevScene::counters[7]), pmc_run_primary fails.
    template<int GRID, bool KIN = false>
    __device__ __forceinline__ uint32_t startCycleWalks(const DevScene& S, const GridLds& G, Counters& cnt, int slot, int modeWord, const PeelSortArgs* ps = nullptr,
                                                        uint32_t* cursors = nullptr)
    {
        const SlotArrays& A = S.slots;
        const int64_t NS = A.num_slots;
        const double rx = A.rx[slot], ry = A.ry[slot], rz = A.rz[slot];
        const double kx = A.kx[slot], ky = A.ky[slot], kz = A.kz[slot];
        const double lambda = S.mono ? S.mono_lambda : A.lambda[slot];
        const double sext = S.mono ? S.mono_ext : A.dustExt[slot];
        // (the interaction cell of the propagation walk that led here is the leaf of this position; -1 after a launch)
        const int hint0 = A.mint[slot];
        const double drawn = S.force_scattering ? 0. : A.tausample[slot];
        const uint32_t pmask = ((uint32_t)modeWord >> 8) & 0xFFFFu;
        const bool emission = KIN && A.nscatt[slot] == 0;
        int hint = hint0;
        uint32_t made = 0u;
        // Voronoi: all walks of the cycle start at this position: its cell (VoronoiMeshSnapshot::cellIndex) is found once
        // (after a scattering event the walk has named the cell: confirmed against its neighbours instead of searched)
        if (GRID == GRID_VORO) hint = (hint0 >= 0 && voroIsNearest(S, hint0, rx, ry, rz)) ? hint0 : voroCellIndex(S, rx, ry, rz);
        // (ONE copy of the walk start in the code: the propagation walk is round num_instruments of the same loop)
#pragma unroll 1
        for (int i = 0; i <= S.num_instruments; ++i)
        {
            const bool prop = i == S.num_instruments;
            if (!prop && !((pmask >> i) & 1u))
            {
                S.tasks.bits[(int64_t)(1 + i) * NS + slot] = PMC_TASK_NONE;
                continue;
            }
            const DevInstrument& I = S.inst[prop ? 0 : i];
            // peel-off walk: up to taumax of the packet's weight; propagation walk: forced scattering walks the whole path first
            // (pass 1), otherwise up to the drawn optical depth
            double target = prop ? drawn : peelTaumax(A.ppW[(int64_t)i * NS + slot], (KIN && emission) ? A.obsLambda[(int64_t)i * NS + slot] : lambda);
            if (KIN && emission && !prop && target != -INFINITY)
            {
                const double sobs = A.obsExt[(int64_t)i * NS + slot];
                if (sobs != sext)
                {
                    if (sext == 0.) atomicAdd(S.counters + 7, 1ull);
                    target = sobs > 0. ? target * (sext / sobs) : INFINITY;
                }
            }
            // (sorted peel-off records: the walk's place in the tile order of its observer -- every slot with this bit of the mode word set
            // takes one, as peelSortCountKernel counted)
            PeelRec* place = nullptr;
            // (Voronoi: a walk that runs in voroPeelKernel -- sorted observer with a table -- or voroPropKernel gets its first cell located only; measured
            // for the propagation walks of the generic kernel too, which also knows ST_FIRST: the cycle start kernel gains less than that kernel loses)
            const bool deferScan = GRID == GRID_VORO && ps
                                   && (prop ? ((S.voro_defer_scan & 2) != 0 && ps->propIndex >= 0)
                                            : ((S.voro_defer_scan & 1) != 0 && ps->sortIndex[i] >= 0 && S.vobs_of_inst[i] >= 0));
            if (ps && !prop)
            {
                const int k = ps->sortIndex[i];
                if (k >= 0)
                {
                    const uint32_t at = atomicAdd(&cursors[(uint32_t)k * ps->numParts + peelTile(*ps, I, rx, ry, rz)], 1u);
                    if (at >= ps->cap)
                        atomicAdd(S.counters + 7, 1ull);  // (the two passes of the sort disagree: an internal error, reported by pmc_run_primary)
                    else if (GRID == GRID_TREE)
                        place = ps->out[k] + at;
                    else
                        ps->listOut[k][at] = slot;  // (Cartesian, Voronoi: the slot's place in the observer's list; the start state goes to TaskArrays)
                }
            }
            if (GRID != GRID_TREE && ps && prop && ps->propIndex >= 0)
            {
                // (the slot's place in the list of propagation walks, sorted by the sign octant of the direction: peelSortCountKernel counted likewise)
                const uint32_t at = atomicAdd(&cursors[(uint32_t)ps->propIndex * ps->numParts + propSortKey(S, rx, ry, rz, kx, ky, kz)], 1u);
                if (at >= ps->cap)
                    atomicAdd(S.counters + 7, 1ull);
                else
                    ps->listOut[ps->propIndex][at] = slot;
            }
            const bool exists = prepareWalk<GRID>(S, G, cnt, slot, prop ? 0 : 1 + i, prop ? (S.force_scattering ? MODE_PASS1 : MODE_PASS2) : MODE_PEEL,
                                                  rx, ry, rz, prop ? kx : I.kx, prop ? ky : I.ky, prop ? kz : I.kz, target, sext, hint,
                                                  place, deferScan);
            if (exists) made |= prop ? 1u : 2u << i;
        }
        return made;
    }

    // ================================================================================================
    //  cycle start kernel: one lane per slot of the group, in slot order; every live slot is at the start of a cycle here (its
    //  history has just been launched, or has just scattered) and gets the start state of the cycle's walks -- task record 0 for
    //  the propagation walk, 1 + i for the peel-off walk towards observer i (PathSegmentGenerator::moveInside, the first cell,
    //  the first exit distance).  The only kernel beside the walk kernels that reads the grid: its tables are staged once per
    //  persistent workgroup.  With listCounter >= 0 it also compacts the live slots into listOut (one of the group's two ranges of
    //  TaskArrays::liveList; counter S.counters[listCounter]): the kernels of a sparse generation run over that list -- this one
    //  too (listIn, listLen: the list the generation started with).
    // ================================================================================================
    //  KIN: the flavour of a scene with a moving source
    template<int GRID, bool KIN = false>
    __global__ __launch_bounds__(256, PMC_CYCLE_MIN_WAVES) void cycleStartKernel(const int sceneSlot, const int slotBase, const int numSlots,
                                                                                 const int listCounter, int* const listOut,
                                                                                 const int* const listIn, const int listLen, const PeelSortArgs ps)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        if (GRID == GRID_TREE) requireLdsBaseZero(lds);
        stageGrid<GRID>(S, lds, tid, blockDim.x);
        __syncthreads();
        const GridLds G = makeGridLds(S, lds);
        const SlotArrays& A = S.slots;
        Counters cnt = {0, 0, 0, 0, 0};
        const int slotEnd = slotBase + numSlots;
        const bool sparse = GRID == GRID_TREE && listIn != nullptr;  // this generation ran over the list of the previous one
        if (ps.numObs > 0 && !sparse)
        {
            // ---- sorted peel-off records: this workgroup takes the sort tiles blockIdx.x, + gridDim.x, ... as peelSortCountKernel's workgroup
            // of the same index did; its next free place in every partition of every observer's tile order is in LDS
            // (in the dynamic LDS behind the grid tables: the walk code addresses those from LDS offset 0)
            uint32_t* const cur = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + ps.ldsOffset);
            const int numLists = ps.numObs + (ps.propIndex >= 0 ? 1 : 0);  // (the list of the propagation walks follows the observers')
            for (int k = 0; k < numLists; ++k)
                for (uint32_t p = tid; p < ps.numParts; p += blockDim.x)
                    cur[(uint32_t)k * ps.numParts + p] = (uint32_t)ps.start[k][p] + ps.matrix[k][(size_t)blockIdx.x * ps.numParts + p];
            __syncthreads();
            const int tiles = (numSlots + PEEL_SORT_TILE - 1) / PEEL_SORT_TILE;
            for (int t = blockIdx.x; t < tiles; t += gridDim.x)
                for (int i = t * PEEL_SORT_TILE + tid; i < (t + 1) * PEEL_SORT_TILE && i < numSlots; i += blockDim.x)
                {
                    const int slot = slotBase + i;
                    const int md = A.mode[slot];
                    if (md & MODE_ALIVE) startCycleWalks<GRID, KIN>(S, G, cnt, slot, md, &ps, cur);
                }
        }
        else
        {
            const int end = sparse ? listLen : numSlots;
            for (int i0 = blockIdx.x * blockDim.x; i0 < end; i0 += gridDim.x * blockDim.x)
            {
                const int i = i0 + tid;
                const int slot = sparse ? (i < listLen ? listIn[i] : -1) : slotBase + i;
                const int md = (slot >= 0 && slot < slotEnd) ? A.mode[slot] : 0;
                if (md & MODE_ALIVE) startCycleWalks<GRID, KIN>(S, G, cnt, slot, md);
                if (GRID == GRID_TREE && listCounter >= 0)
                {
                    // a sparse generation follows: the live slots go to the group's list, in any order (one atomic per wave)
                    const unsigned long long m = __ballot((md & MODE_ALIVE) != 0);
                    if (m)
                    {
                        unsigned long long at = 0;
                        if (lane == __ffsll((long long)m) - 1) at = atomicAdd(S.counters + listCounter, (unsigned long long)__popcll(m));
                        at = __shfl(at, __ffsll((long long)m) - 1, 64);
                        if (md & MODE_ALIVE) listOut[(int)at + __popcll(m & ((1ull << lane) - 1ull))] = slot;
                    }
                }
            }
        }
        const unsigned long long v = waveSum(cnt.paths);
        if (lane == 0 && v) atomicAdd(S.counters + 1, v);
    }

    // ---- sorted peel-off records: a counting sort on the tile without any global atomic and without a pass of its own for the scatter.  Workgroup
    // b owns the sort tiles b, b + gridDim.x, ... (2048 slots each) in both kernels that look at the slots:
    //   peelSortCountKernel    (behind the transition / launch kernels) its slots with a walk per partition -> row b of a matrix [workgroups][partitions]
    //   peelSortOffsetsKernel  per partition: the rows' exclusive prefix in place, and the partition's total (rfScanKernel turns the totals
    //                          into the partitions' starts)
    //   cycleStartKernel       start + prefix = the workgroup's own cursor of every partition, in LDS: the place of a walk's record is one LDS
    //                          atomic away, and the start state goes straight there
    // (Claiming runs with a global atomic per partition and tile, as the radiation-field sort does, costs 0.3 ms per generation here: a group's
    // 683 tiles all claim from the few partitions of the image centre at the same moment.  A scatter pass of its own -- gather the start
    // states from the task arrays, write the records -- cost 0.2 ms per generation: 1.2e6 scattered 64-byte writes.)
    __global__ __launch_bounds__(256) void peelSortCountKernel(const int sceneSlot, const int slotBase, const int numSlots, const PeelSortArgs ps)
    {
        const DevScene& S = c_scene[sceneSlot];
        const SlotArrays& A = S.slots;
        __shared__ uint32_t h[PMC_SORT_OBS * PMC_PEEL_TILES * PMC_PEEL_TILES];
        const int tid = threadIdx.x;
        const int numLists = ps.numObs + (ps.propIndex >= 0 ? 1 : 0);
        for (uint32_t p = tid; p < (uint32_t)numLists * ps.numParts; p += blockDim.x) h[p] = 0u;
        __syncthreads();
        const int tiles = (numSlots + PEEL_SORT_TILE - 1) / PEEL_SORT_TILE;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x)
            for (int i = t * PEEL_SORT_TILE + tid; i < (t + 1) * PEEL_SORT_TILE && i < numSlots; i += blockDim.x)
            {
                // a live slot whose cycle has a peel-off packet for the observer (announceCycle: bit 8 + instrument of the mode word) will
                // get a record in that observer's order (the cycle start kernel goes by the same bits and the same position)
                const int slot = slotBase + i;
                const int md = A.mode[slot];
                if (!(md & MODE_ALIVE)) continue;
                const double x = A.rx[slot], y = A.ry[slot], z = A.rz[slot];
                for (int k = 0; k < ps.numObs; ++k)
                    if (((uint32_t)md >> (8 + ps.obs[k])) & 1u) atomicAdd(&h[(uint32_t)k * ps.numParts + peelTile(ps, S.inst[ps.obs[k]], x, y, z)], 1u);
                // (Cartesian, Voronoi: every live slot gets a place in the list of propagation walks, by the sign octant of its direction)
                if (ps.propIndex >= 0)
                    atomicAdd(&h[(uint32_t)ps.propIndex * ps.numParts + propSortKey(S, x, y, z, A.kx[slot], A.ky[slot], A.kz[slot])], 1u);
            }
        __syncthreads();
        for (int k = 0; k < numLists; ++k)
            for (uint32_t p = tid; p < ps.numParts; p += blockDim.x) ps.matrix[k][(size_t)blockIdx.x * ps.numParts + p] = h[(uint32_t)k * ps.numParts + p];
    }
    // (16 partitions x 16 runs of rows per workgroup: a lane sums its run of rows, the runs' sums are scanned in LDS, the lane writes the prefixes)
    __global__ __launch_bounds__(256) void peelSortOffsetsKernel(uint32_t* __restrict__ matrix, const uint32_t groups, const uint32_t numParts,
                                                                 unsigned long long* __restrict__ totals)
    {
        __shared__ uint32_t part[16][17];
        const uint32_t pl = threadIdx.x & 15u, run = threadIdx.x >> 4;
        const uint32_t p = blockIdx.x * 16u + pl;
        const uint32_t rows = (groups + 15u) / 16u;
        const uint32_t b0 = run * rows, b1 = b0 + rows < groups ? b0 + rows : groups;
        uint32_t sum = 0u;
        if (p < numParts)
            for (uint32_t b = b0; b < b1; ++b) sum += matrix[(size_t)b * numParts + p];
        part[run][pl] = sum;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t r = 0; r < 16u; ++r)
        {
            const uint32_t v = part[r][pl];
            if (r < run) before += v;
            all += v;
        }
        if (p < numParts)
        {
            for (uint32_t b = b0; b < b1; ++b)
            {
                const uint32_t c = matrix[(size_t)b * numParts + p];
                matrix[(size_t)b * numParts + p] = before;
                before += c;
            }
            if (run == 0u) totals[p] = all;
        }
    }
