// pmc_run.hip -- pmc_run_primary: the pool of packet slots and the generation loop over the slot groups (MonteCarloSimulation::runPrimaryEmission,
// MonteCarloSimulation.cpp:104-138: parallel->call(Npp, performLifeCycle) up to instrumentSystem()->flush()).
#include "pmc_context.h"

namespace
{
    int allocateSlotArrays(pmc_ctx* ctx, int64_t n);
    void releaseSlots(pmc_ctx* ctx)
    {
        for (void* p : ctx->slotAllocations) hipFree(p);
        ctx->slotAllocations.clear();
        ctx->allocatedSlots = 0;
    }

    // the slot pool of n histories in flight: first added up and held against the free device memory (a clear message instead of
    // a failed hipMalloc half-way), then allocated
    int allocateSlots(pmc_ctx* ctx, int64_t n)
    {
        hipSetDevice(ctx->device);
        releaseSlots(ctx);
        ctx->planning = true;
        ctx->plannedBytes = 0;
        int rc = allocateSlotArrays(ctx, n);
        ctx->planning = false;
        if (rc) return rc;
        size_t freeBytes = 0, totalBytes = 0;
        // (the default number of slots is sized for the 288 GB of an MI355X; on a device, or next to other contexts, where it would take
        // more than half of the free memory the default steps down -- a number the caller has set is taken as it is)
        if (!ctx->slotsConfigured && n > (int64_t(1) << 20) && hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && ctx->plannedBytes > freeBytes / 2)
        {
            // (the requested default, ctx->numSlots, stays as it is: a later segment asks again -- pmc_run_primary -- and gets the larger
            // pool once the memory is there)
            const int64_t less = std::max<int64_t>(int64_t(1) << 20, n / 2);
            fprintf(stderr, "libpmc: device %d has %.1f GB free, %lld packet slots would take %.1f GB: this segment runs with %lld slots (fewer histories in "
                            "flight, somewhat lower throughput; PMC_NUM_SLOTS / pmc_set_num_slots set the number)\n",
                    ctx->device, freeBytes * 1e-9, (long long)n, ctx->plannedBytes * 1e-9, (long long)less);
            ctx->steppedDownFree = freeBytes;
            return allocateSlots(ctx, less);
        }
        if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && ctx->plannedBytes > freeBytes)
        {
            char text[512];
            snprintf(text, sizeof(text),
                     "the state of %lld photon histories in flight needs %.2f GB of device memory (%.0f bytes per history), %.2f GB of %.2f GB are "
                     "free: lower the number with pmc_set_num_slots or PMC_NUM_SLOTS",
                     (long long)n, ctx->plannedBytes * 1e-9, double(ctx->plannedBytes) / double(n), freeBytes * 1e-9, totalBytes * 1e-9);
            return fail(PMC_ERR_NOMEM, text);
        }
        rc = allocateSlotArrays(ctx, n);
        // (the plan above was held against the memory that was free THEN: contexts of other processes that start on the same device at the same
        // time -- ranks of a job that share a device -- plan against the same free memory.  What is left now must still hold the segment's logs, sort
        // buffers and the kernels' own needs: if an allocation failed, or less than 4 GB is left, the default steps down and tries again)
        bool crowded = rc == PMC_ERR_DEVICE || rc == PMC_ERR_NOMEM;
        if (!rc && hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && freeBytes < (size_t(4) << 30)) crowded = true;
        if (crowded && !ctx->slotsConfigured && n > (int64_t(1) << 20))
        {
            releaseSlots(ctx);
            const int64_t less = std::max<int64_t>(int64_t(1) << 20, n / 2);
            fprintf(stderr, "libpmc: device %d is short of memory next to other contexts (%.1f GB left): this segment runs with %lld packet slots instead of %lld\n",
                    ctx->device, freeBytes * 1e-9, (long long)less, (long long)n);
            ctx->steppedDownFree = freeBytes + 1;
            return allocateSlots(ctx, less);
        }
        if (rc) releaseSlots(ctx);
        return rc;
    }

    int allocateSlotArrays(pmc_ctx* ctx, int64_t n)
    {
        SlotArrays& A = ctx->dev.slots;
        std::memset(&A, 0, sizeof(A));
        auto& own = ctx->slotAllocations;
        int rc;
        double** dbl[] = {&A.rx, &A.ry, &A.rz, &A.kx, &A.ky, &A.kz, &A.lambda, &A.W, &A.Lthreshold, &A.taupath, &A.tausample, &A.rngSpare, &A.sint,
                          &A.nint, &A.dustExt, &A.dustSca, &A.dustAsym};
        for (double** d : dbl)
            if ((rc = ctx->allocate<double>(n, d, false, &own))) return rc;
        if (ctx->dev.explicit_absorption && (rc = ctx->allocate<double>(n, &A.dustAbs, false, &own))) return rc;
        if (ctx->dev.num_media > 1 && !ctx->dev.mono && (rc = ctx->allocate<int32_t>(n * ctx->dev.num_media, &A.dustIdx, false, &own))) return rc;
        if ((rc = ctx->allocate<uint64_t>(n, &A.history, false, &own))) return rc;
        if ((rc = ctx->allocate<uint32_t>(n, &A.rngBlock, false, &own))) return rc;
        int32_t** ints[] = {&A.mode, &A.nscatt, &A.mint};
        for (int32_t** d : ints)
            if ((rc = ctx->allocate<int32_t>(n, d, true, &own))) return rc;
        if ((rc = ctx->allocate<double>(size_t(n) * size_t(ctx->dev.num_instruments), &A.ppW, false, &own))) return rc;
        if ((rc = ctx->allocate<double>(size_t(n) * size_t(ctx->dev.num_instruments), &A.ptau, false, &own))) return rc;
        if ((rc = ctx->allocate<int32_t>(size_t(n) * size_t(ctx->dev.num_instruments), &A.ell, true, &own))) return rc;
        if (ctx->dev.any_stats && (rc = ctx->allocate<int32_t>(size_t(n) * size_t(ctx->dev.num_instruments) * 16, &A.statHead, true, &own))) return rc;
        if (ctx->dev.rf_store && (rc = ctx->allocate<int32_t>(n, &A.rfell, true, &own))) return rc;
        if (ctx->dev.kin)
        {
            // (a moving source: the emission cycle's own wavelength, cross section and bin per instrument)
            const size_t per = size_t(n) * size_t(ctx->dev.num_instruments);
            if ((rc = ctx->allocate<double>(per, &A.obsLambda, false, &own))) return rc;
            if ((rc = ctx->allocate<double>(per, &A.obsExt, false, &own))) return rc;
            if ((rc = ctx->allocate<int32_t>(per, &A.obsEll, true, &own))) return rc;
        }
        if (ctx->dev.any_stats)
        {
            size_t entries = size_t(ctx->dev.num_instruments) * PMC_STAT_CAP * size_t(n);
            if ((rc = ctx->allocate<int32_t>(entries, &A.statBin, false, &own))) return rc;
            if ((rc = ctx->allocate<double>(entries, &A.statW, false, &own))) return rc;
            // continuation blocks of the lists (pmc_device.h DevScene::stat_pool_*): by default one block per four slots -- or,
            // for a ski file that asks for many scattering events per history (minScattEvents), what such histories need in
            // every slot at once; environment PMC_STAT_POOL_BLOCKS sets the number
            DevScene& D = ctx->dev;
            const int minEvents = D.min_scatt_events;
            int64_t blocks = minEvents > 16 ? n * int64_t((minEvents + 2 * PMC_STAT_CAP - 1) / PMC_STAT_CAP) : n / 4;
            blocks = std::max<int64_t>(blocks, 1024) * D.num_instruments;
            // (... and up to one block per slot and instrument where an eighth of the free device memory allows it: the sparse
            // generations at the end of a segment keep the blocks of retired histories out of the pool, and a long non-forced history
            // in an optically thick medium needs more than the default)
            {
                size_t freeBytes = 0, totalBytes = 0;
                if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess)
                {
                    const int64_t afford = int64_t(freeBytes / 8 / (PMC_STAT_CAP * 12 + 12));
                    blocks = std::max(blocks, std::min<int64_t>(n * int64_t(D.num_instruments), afford));
                }
            }
            if (const char* env = getenv("PMC_STAT_POOL_BLOCKS")) blocks = std::max<int64_t>(PMC_MAX_GROUPS, atoll(env));
            blocks = std::min<int64_t>(blocks, int64_t(1) << 30);
            if ((rc = ctx->allocate<int32_t>(size_t(blocks) * PMC_STAT_CAP, &D.stat_pool_bin, false, &own))) return rc;
            if ((rc = ctx->allocate<double>(size_t(blocks) * PMC_STAT_CAP, &D.stat_pool_w, false, &own))) return rc;
            if ((rc = ctx->allocate<int32_t>(size_t(blocks), &D.stat_pool_next, false, &own))) return rc;
            if ((rc = ctx->allocate<int32_t>(size_t(blocks), &D.stat_pool_free, false, &own))) return rc;
            if ((rc = ctx->allocate<int32_t>(size_t(blocks), &ctx->statPoolIota, false, &own))) return rc;
            if (!ctx->planning)
            {
                std::vector<int32_t> iota(static_cast<size_t>(blocks));
                for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int32_t)i;
                if (hipMemcpy(ctx->statPoolIota, iota.data(), iota.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
                    return fail(PMC_ERR_DEVICE, "hipMemcpy failed");
                ctx->statPoolBlocks = blocks;
            }
        }
        TaskArrays& K = ctx->dev.tasks;
        std::memset(&K, 0, sizeof(K));
        // task records: the propagation walk + one peel-off walk per instrument, per slot
        const size_t nt = size_t(n) * size_t(1 + ctx->dev.num_instruments);
        double** tdbl[] = {&K.rx, &K.ry, &K.rz, &K.kx, &K.ky, &K.kz, &K.s0, &K.ds, &K.target};
        for (double** d : tdbl)
            if ((rc = ctx->allocate<double>(nt, d, false, &own))) return rc;
        int32_t** tints[] = {&K.cell, &K.cijk};
        for (int32_t** d : tints)
            if ((rc = ctx->allocate<int32_t>(nt, d, false, &own))) return rc;
        // ended-history counts per tile of 64 slots (padded: the scan reads and writes 16 bytes at a time)
        if ((rc = ctx->allocate<uint32_t>(size_t(n) / 64 + 64, &K.endedCount, true, &own))) return rc;
        if ((rc = ctx->allocate<int32_t>(2 * size_t(n), &K.liveList, false, &own))) return rc;
        if ((rc = ctx->allocate<uint32_t>(nt, &K.bits, false, &own))) return rc;
    if (ctx->dev.grid_kind == PMC_GRID_OCTREE && (rc = ctx->allocate<uint64_t>(nt, &K.pidx, false, &own))) return rc;
        if (ctx->planning) return PMC_OK;
        A.num_slots = n;
        ctx->allocatedSlots = n;
        ctx->sceneDirty = true;
        return PMC_OK;
    }
}

int pmcAllocateSlots(pmc_ctx* ctx, int64_t n)
{
    return allocateSlots(ctx, n);
}

// ---- radiation field on an octree: the contributions of a generation go to a log per slot group (pmc_device.h RfLogArgs), which is
// partitioned by key range and summed after the generation.  Tables beyond 2^26 entries have more partitions than the counting sort's
// LDS histogram holds: atomics.  (The keys of the log count cells in the device numbering: cell_slots of them, padding included.)
// ---- statistics: the contributions of ended histories go to a log per slot group (pmc_device.h StatLogArgs), which is partitioned by
// record range and summed in LDS when it has filled up, and at the end of the segment
LogPlan pmcLogPlan(const pmc_ctx* ctx)
{
    const DevScene& D = ctx->dev;
    const bool octree = D.grid_kind == PMC_GRID_OCTREE;
    LogPlan L;
    L.rfKeys = octree ? int64_t(D.cell_slots) * D.rf_num_lambda : ctx->rfSize;
    L.rfParts = (L.rfKeys + (int64_t(1) << PMC_RF_BUCKET_BITS) - 1) >> PMC_RF_BUCKET_BITS;
    L.rfLogged = D.rf_store && octree && L.rfParts <= pmcRfMaxParts() && pmcTune("PMC_RF_ATOMICS") == nullptr;
    const int statBits = pmcStatBucketBits();
    L.statRecords = D.stat_acc_records;
    L.statParts = (D.stat_acc_records + (int64_t(1) << statBits) - 1) >> statBits;
    L.statLogged = D.any_stats && D.stat_acc_records > 0 && L.statParts <= pmcRfMaxParts() && pmcTune("PMC_STAT_ATOMICS") == nullptr;
    return L;
}

namespace
{
    // ---- one segment of pmc_run_primary: the plan (decided once, before the first kernel), the buffers it needs, the generations of the slot
    // groups until no slot is alive, the end of the segment
    struct SegmentPlan
    {
        uint64_t first, count, seed;
        // slot groups: group g owns the slots [base[g], base[g] + size[g]) and the stream groupStream[g].  The generations of different groups
        // are independent (histories come from one shared cursor), so while the host waits for one group the other groups' kernels keep the
        // device busy: the tail of a walk kernel and the latency-bound transition kernel overlap with the walk kernel of another group.
        int G;
        int base[PMC_MAX_GROUPS], size[PMC_MAX_GROUPS];
        bool octree;
        int walkFlavour;       // bit 0 radiation field, bit 1 explicit absorption, bit 2 several medium components (pmcLaunchWalk / Prop / VoroProp)
        int peelForm;          // octree peel-off: bit 0 wide, bit 1 several medium components, bit 2 task queues (pmcLaunchPeel)
        bool propCheckpoints;  // octree propagation: the pass-1 checkpoints in LDS (pmcPropHasCheckpoints)
        // sorted peel-off records (pmc_device.h PeelRec): an octree whose peel-off kernel runs with task queues, at most PMC_SORT_OBS observers
        // (their records are written by the cycle start kernel in slot order, sorted by detector tile, and read in tile order by the peel-off kernel)
        int numSortObs, sortObs[PMC_SORT_OBS];
        int propSortIndex, numSortLists;
        PeelSortArgs sortArgs;  // (all but `cap`, which is the group's)
        // sparse generations (the end of a segment, when no history is left to launch): the cycle start kernel compacts the live
        // slots of the group into a list, and the kernels of the next generation run over the list with as many workgroups as it
        // needs -- their time then follows the live histories, not the size of the slot pool (a third of the generations of a
        // 1e8-packet segment run fewer than a tenth of the slots).  Such a generation is walks -> transition -> cycle start: the
        // transition kernel retires the histories that end (nothing is left to launch into their slots), the cycle start kernel
        // writes the list of the generation after it into the other half of TaskArrays::liveList.
        bool sparseLists;
        int listTasksPerLane;  // walks per lane that size the walk kernels' grids in a sparse generation
        // radiation-field and statistics logs per slot group
        bool rfLogged, statLogged;
        int rfBuckets, statParts;
        uint32_t rfPadKey;
        unsigned long long rfLogPerSlot, statLogEntries;
        bool poolGrows;  // the statistics pool grows when a group could run out of blocks
        int statInstruments;
        int launchFlavour;  // the launch kernel of the scene (pmc_device.h PMC_LAUNCH_*)
        // launch geometry
        int launchBlocks, cycleBlocks, transitionBlocks;
        int voroPropGrid, voroPeelGrid, voroPropSegments;
        // tuning switches
        bool serialWalks, genDump, xcdAffinity, voroPeelKernels, voroPropKernel, voroWalksInSeries;
    };
    // what the generations of a segment leave for the ones after them
    struct SegmentRun
    {
        bool active[PMC_MAX_GROUPS], haveWalk[PMC_MAX_GROUPS];
        bool listBuilt[PMC_MAX_GROUPS];   // the group's last generation built a list of live slots (sparse generations)
        int listHalf[PMC_MAX_GROUPS];     // the half of liveList that holds the group's current list
        bool peelSorted[PMC_MAX_GROUPS];  // the group's last cycle start wrote sorted peel-off records / lists
        bool poolCannotGrow;
        float walkMs, transMs, peelMs, propMs;
        int generations;
    };

    // the slot pool of the segment: grown to the requested size where it can be (the default steps down where the device memory is short: allocateSlots)
    int provisionSlots(pmc_ctx* ctx, uint64_t count, int* numSlots)
    {
        const int64_t want = std::min<int64_t>(ctx->numSlots, (int64_t)std::min<uint64_t>(count, uint64_t(1) << 30));
        bool grow = want > ctx->allocatedSlots;
        if (grow && ctx->allocatedSlots > 0 && ctx->steppedDownFree)
        {
            // (a default pool that has stepped down: ask again only when more memory is free than there was then -- not a
            // reallocation per segment)
            size_t freeBytes = 0, totalBytes = 0;
            grow = hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && freeBytes > ctx->steppedDownFree + ctx->steppedDownFree / 4;
        }
        if (grow)
        {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            ctx->steppedDownFree = 0;
            int rc = allocateSlots(ctx, want);
            if (rc) return rc;
        }
        *numSlots = (int)std::min<int64_t>(want, ctx->allocatedSlots);
        HIP_TRY(sceneUpToDate(ctx));
        return PMC_OK;
    }

    // the launch kernel of the context's scene: the flavour its sources select, or (PMC_LAUNCH_GENERIC: tests, A/B runs) the generic kernel
    int launchFlavour(const pmc_ctx* ctx)
    {
        const DevScene& D = ctx->dev;
        if (pmcTune("PMC_LAUNCH_GENERIC") != nullptr) return D.kin ? PMC_LAUNCH_KIN : 0;
        return pmcLaunchFlavourOf(D.src, D.num_sources, D.kin);
    }

    SegmentPlan planSegment(const pmc_ctx* ctx, int numSlots, uint64_t first, uint64_t count, uint64_t seed)
    {
        const DevScene& D = ctx->dev;
        SegmentPlan P;
        std::memset(&P, 0, sizeof(P));
        P.first = first, P.count = count, P.seed = seed;
        P.octree = D.grid_kind == PMC_GRID_OCTREE;
        P.serialWalks = pmcTune("PMC_SERIAL_WALKS") != nullptr;  // tuning aid: peel-off and propagation kernels one after the other
        P.genDump = pmcTune("PMC_GEN_DUMP") != nullptr;          // tuning aid: live slots and kernel times of every generation
        const bool peelSort = pmcTune("PMC_NO_PEEL_SORT") == nullptr;
        int G = ctx->numGroups;
        if (numSlots < G * 65536) G = 1;
        {
            // (Voronoi: the walk kernel is nine tenths of the step, and its walks run as ONE stream in tile order: a second and third group would
            // put two more streams in flight next to it and triple the cells the L2s have to hold -- 5e7 packets: 2.18 / 2.13 / 2.04e7 packets/s
            // with one / two / three groups)
            int observers = 0;
            for (int i = 0; i < D.num_instruments; ++i) observers += D.inst[i].same_observer ? 0 : 1;
            if (D.grid_kind == PMC_GRID_VORONOI && observers <= PMC_SORT_OBS && !ctx->groupsConfigured && peelSort) G = 1;
        }
        P.G = G;
        // (ceil(numSlots / G): with the floor, 266 241 slots in four groups left the last slot idle -- test_gpu_slot_reuse, four-group case)
        const int per = ((numSlots + G - 1) / G + PMC_TRANSITION_ALIGN - 1) / PMC_TRANSITION_ALIGN * PMC_TRANSITION_ALIGN;
        for (int g = 0; g < G; ++g)
        {
            P.base[g] = std::min(numSlots, g * per);
            P.size[g] = std::min(per, numSlots - P.base[g]);
        }
        P.walkFlavour = (D.rf_store ? 1 : 0) | (D.explicit_absorption ? 2 : 0) | (D.num_media > 1 ? 4 : 0);
        P.peelForm = (ctx->wide ? 1 : 0) | (D.num_media > 1 ? 2 : 0);
        if (pmcPeelHasQueues(P.peelForm, ctx->walkLds)) P.peelForm |= 4;
        P.propCheckpoints = pmcPropHasCheckpoints(P.walkFlavour, ctx->walkLds);
        P.propSortIndex = -1;
        if (peelSort && (!P.octree || (P.peelForm & 4)))
        {
            int observers = 0;
            for (int i = 0; i < D.num_instruments; ++i)
                if (!D.inst[i].same_observer)
                {
                    if (observers < PMC_SORT_OBS) P.sortObs[observers] = i;
                    ++observers;
                }
            if (observers <= PMC_SORT_OBS) P.numSortObs = observers;  // (more observers than that: all of them from the task arrays)
        }
        // (Cartesian, Voronoi: one more list through the same sort -- the slots' PROPAGATION walks by the sign octant of their direction: with the
        // XCD affinity of the walk stream the L2 of an XCD then sees the propagation walks of about one octant)
        if (!P.octree && P.numSortObs > 0 && P.numSortObs < PMC_SORT_OBS && pmcTune("PMC_NO_PROP_SORT") == nullptr) P.propSortIndex = P.numSortObs;
        P.numSortLists = P.numSortObs + (P.propSortIndex >= 0 ? 1 : 0);
        PeelSortArgs& sa = P.sortArgs;
        sa.numObs = P.numSortObs;
        sa.propIndex = P.propSortIndex;
        for (int i = 0; i < 16; ++i) sa.sortIndex[i] = -1;
        for (int k = 0; k < P.numSortObs; ++k) sa.obs[k] = P.sortObs[k], sa.sortIndex[P.sortObs[k]] = (int8_t)k;
        const double gdx = D.gx1 - D.gx0, gdy = D.gy1 - D.gy0, gdz = D.gz1 - D.gz0;
        sa.centre[0] = 0.5 * (D.gx0 + D.gx1), sa.centre[1] = 0.5 * (D.gy0 + D.gy1), sa.centre[2] = 0.5 * (D.gz0 + D.gz1);
        sa.scale = PMC_PEEL_TILES / std::sqrt(gdx * gdx + gdy * gdy + gdz * gdz);
        P.xcdAffinity = pmcTune("PMC_NO_XCD_AFFINITY") == nullptr;
        P.sparseLists = P.octree && pmcTune("PMC_NO_LIVE_LISTS") == nullptr;
        P.listTasksPerLane = 1;
        if (const char* env = pmcTune("PMC_LIST_TASKS_PER_LANE")) P.listTasksPerLane = std::max(1, atoi(env));
        // Voronoi, one medium component: the peel-off walks towards an observer that has a table of runs go through a kernel of their own
        // (a switch set after pmc_create: the generic kernel knows a walk whose first cell is still to be scanned as well)
        P.voroPeelKernels = D.grid_kind == PMC_GRID_VORONOI && pmcTune("PMC_VORO_NO_PEEL_KERNEL") == nullptr;
        // ... and the propagation walks (every flavour since round 6), on the table of runs with all neighbours (when pmc_create built it)
        P.voroPropKernel = D.grid_kind == PMC_GRID_VORONOI && D.vgen_run && pmcTune("PMC_VORO_NO_PROP_KERNEL") == nullptr
                           && !(pmcTune("PMC_VORO_PLAIN_PROP_ONLY") && (D.num_media > 1 || D.rf_store || D.explicit_absorption));
        P.voroWalksInSeries = pmcTune("PMC_VORO_WALKS_IN_SERIES") != nullptr;
        P.voroPropSegments = (P.xcdAffinity && pmcTune("PMC_VPROP_XCD_SEGMENTS")) ? 8 : 1;
        int propBlocks = pmcVoroPropWavesPerSimd(), peelBlocks = pmcVoroPeelWavesPerSimd();
        if (const char* v = pmcTune("PMC_VPROP_BLOCKS_PER_CU")) propBlocks = std::max(1, atoi(v));
        if (const char* v = pmcTune("PMC_VPEEL_BLOCKS_PER_CU")) peelBlocks = std::max(1, atoi(v));
        P.voroPropGrid = ctx->numCU * propBlocks, P.voroPeelGrid = ctx->numCU * peelBlocks;
        // ---- the logs of the radiation field and of the statistics (pmcLogPlan).  Radiation field: 128 entries per slot (config 2: 60 per
        // propagation walk on average); a wave that finds the log full falls back to atomic adds into the table.
        const LogPlan logs = pmcLogPlan(ctx);
        P.rfLogged = logs.rfLogged;
        if (D.rf_store && P.octree && logs.rfParts > pmcRfMaxParts())
        {
            // (a table beyond 2^26 entries: one atomic per contribution, several times slower -- said once, not silently)
            static std::atomic<bool> said{false};
            if (!said.exchange(true))
                fprintf(stderr, "libpmc: the radiation field table has %lld entries, more than the log's counting sort partitions (%d x %d): contributions are added atomically\n",
                        (long long)logs.rfKeys, pmcRfMaxParts(), 1 << PMC_RF_BUCKET_BITS);
        }
        P.rfBuckets = P.rfLogged ? int(logs.rfParts) : 0;
        P.rfPadKey = uint32_t(P.rfBuckets) << PMC_RF_BUCKET_BITS;
        P.rfLogPerSlot = 128ull;
        if (const char* env = pmcTune("PMC_RF_LOG_PER_SLOT")) P.rfLogPerSlot = std::max(1, atoi(env));  // (tests: a log that overflows)
        P.statParts = int(logs.statParts);
        P.statLogged = logs.statLogged;
        // (3.7 entries per history on configs[1]: the log of a group holds a segment of 1e8 packets; it is flushed when half full)
        unsigned long long entries = (128ull << 20);
        if (const char* env = pmcTune("PMC_STAT_LOG_ENTRIES")) entries = std::max(1, atoi(env));  // (tests: a log that overflows)
        P.statLogEntries = std::max<unsigned long long>((entries + PMC_RF_LOG_CHUNK - 1) / PMC_RF_LOG_CHUNK, 1ull) * PMC_RF_LOG_CHUNK;
        for (int i = 0; i < D.num_instruments; ++i) P.statInstruments += D.inst[i].record_stats ? 1 : 0;
        P.poolGrows = D.any_stats && ctx->statPoolBlocks > 0 && pmcTune("PMC_STAT_POOL_NO_GROWTH") == nullptr;
        P.launchFlavour = launchFlavour(ctx);
        P.launchBlocks = ctx->numCU * 4;  // persistent launch workgroups, as the transition kernel's
        if (const char* env = pmcTune("PMC_LAUNCH_BLOCKS_PER_CU")) P.launchBlocks = ctx->numCU * std::max(1, atoi(env));
        P.cycleBlocks = ctx->numCU * 4;  // persistent cycle start workgroups (grid tables staged once per workgroup)
        if (const char* env = pmcTune("PMC_CYCLE_BLOCKS_PER_CU")) P.cycleBlocks = ctx->numCU * std::max(1, atoi(env));
        P.transitionBlocks = ctx->numCU * 4;  // persistent transition workgroups (tables staged once per workgroup)
        if (const char* env = pmcTune("PMC_TRANSITION_BLOCKS_PER_CU")) P.transitionBlocks = ctx->numCU * std::max(1, atoi(env));
        return P;
    }

    // a buffer of a slot group that grows with it: `bytes` at *ptr (zeroed, or not initialised)
    struct GroupBuffer
    {
        void** ptr;
        size_t bytes;
        bool zero;
        template<typename T> GroupBuffer(T*& p, size_t bytes, bool zero = false) : ptr(reinterpret_cast<void**>(&p)), bytes(bytes), zero(zero) {}
    };
    // the old buffers go first; then, if `bytes` leave `margin` of the free device memory (or the free memory is not known), every buffer is
    // allocated anew.  False: no room (or an allocation failed), none of the buffers is left -- the group falls back
    bool regrowGroupBuffers(pmc_ctx* ctx, size_t bytes, size_t margin, const std::vector<GroupBuffer>& buffers)
    {
        for (const GroupBuffer& b : buffers) ctx->release(*b.ptr, &ctx->segmentAllocations);
        size_t freeBytes = 0, totalBytes = 0;
        bool room = hipMemGetInfo(&freeBytes, &totalBytes) != hipSuccess || bytes + margin <= freeBytes;
        for (const GroupBuffer& b : buffers)
            room = room && ctx->allocate<uint8_t>(b.bytes, reinterpret_cast<uint8_t**>(b.ptr), b.zero, &ctx->segmentAllocations) == PMC_OK;
        if (!room)
            for (const GroupBuffer& b : buffers) ctx->release(*b.ptr, &ctx->segmentAllocations);
        return room;
    }

    // the walk kernels' cursors; per group and sorted observer the records (octree) or lists of slots (Cartesian, Voronoi) in tile order, and the
    // sort's counters
    int provisionSortBuffers(pmc_ctx* ctx, SegmentPlan& P)
    {
        // (per group PMC_SORT_OBS + 1 sets of eight: set 0 the generic kernel's stream, 1 + k the Voronoi peel-off kernel of sorted observer k, and the
        // octree's peel-off kernels sets 0 .. PMC_SORT_OBS - 1; one more set behind them all that is never written: a count of zero)
        if (!ctx->xcdCursors)
            if (int rc = ctx->allocate<unsigned long long>((size_t(PMC_MAX_GROUPS) * (PMC_SORT_OBS + 1) + 1) * 8, &ctx->xcdCursors, true, &ctx->segmentAllocations))
                return rc;
        for (int g = 0; g < P.G && P.numSortObs > 0; ++g)
        {
            const int padded = (P.size[g] + 4095) / 4096 * 4096;
            if (ctx->peelCap[g] >= padded && (P.octree ? (void*)ctx->peelRec[g][P.numSortObs - 1] : (void*)ctx->peelList[g][P.numSortLists - 1])) continue;
            HIP_TRY(hipDeviceSynchronize());
            // (a group that grows, or more observers than last time: the old buffers go first)
            for (int k = 0; k < PMC_SORT_OBS; ++k) ctx->release(ctx->peelRec[g][k], &ctx->segmentAllocations), ctx->release(ctx->peelList[g][k], &ctx->segmentAllocations);
            ctx->peelCap[g] = 0;
            std::vector<GroupBuffer> buffers;
            for (int k = 0; k < P.numSortLists; ++k)
            {
                buffers.push_back(P.octree ? GroupBuffer(ctx->peelRec[g][k], size_t(padded) * sizeof(PeelRec)) : GroupBuffer(ctx->peelList[g][k], size_t(padded) * sizeof(int32_t)));
                if (!ctx->peelTemp[g][k]) buffers.emplace_back(ctx->peelTemp[g][k], pmcPeelSortTempBytes());
            }
            // (no room for the records: the peel-off walks of every group run from the task arrays, in slot order)
            if (!regrowGroupBuffers(ctx, size_t(P.numSortLists) * (size_t(padded) * sizeof(PeelRec) + pmcPeelSortTempBytes()), size_t(1) << 30, buffers))
            {
                P.numSortObs = P.sortArgs.numObs = 0, P.propSortIndex = P.sortArgs.propIndex = -1, P.numSortLists = 0;
                break;
            }
            ctx->peelCap[g] = padded;
        }
        return PMC_OK;
    }

    int provisionLogs(pmc_ctx* ctx, const SegmentPlan& P)
    {
        // radiation field: no room for a group's log (24 bytes per entry): its contributions go to the table as atomics (cap 0)
        for (int g = 0; g < P.G && P.rfLogged; ++g)
        {
            // (positions in the partitioned log are 32-bit: at most 2^31 - 1 entries, in whole chunks; a wave that finds the log
            // full adds its contributions atomically)
            const unsigned long long want = std::min<unsigned long long>(
                std::max<unsigned long long>(((unsigned long long)P.size[g] * P.rfLogPerSlot + PMC_RF_LOG_CHUNK - 1) / PMC_RF_LOG_CHUNK, 1ull) * PMC_RF_LOG_CHUNK,
                (0x7FFFFFFFull / PMC_RF_LOG_CHUNK) * PMC_RF_LOG_CHUNK);
            if (want <= ctx->rfCap[g]) continue;
            HIP_TRY(hipDeviceSynchronize());
            ctx->rfCap[g] = 0;
            if (regrowGroupBuffers(ctx, size_t(want) * 24, size_t(1) << 30,
                                   {{ctx->rfKeys[g][0], want * sizeof(uint32_t)}, {ctx->rfVals[g][0], want * sizeof(double)}, {ctx->rfKeys[g][1], want * sizeof(uint32_t)},
                                    {ctx->rfVals[g][1], want * sizeof(double)}}))
                ctx->rfCap[g] = want;
        }
        if (P.rfLogged && ctx->rfTempBytes < pmcRfTempBytes(P.rfBuckets))
        {
            HIP_TRY(hipDeviceSynchronize());
            for (int h = 0; h < PMC_MAX_GROUPS; ++h) ctx->release(ctx->rfTemp[h], &ctx->segmentAllocations);
            ctx->rfTempBytes = pmcRfTempBytes(P.rfBuckets);
        }
        for (int g = 0; g < P.G && P.rfLogged; ++g)
            if (!ctx->rfTemp[g])
            {
                uint8_t* t = nullptr;
                if (int rc = ctx->allocate<uint8_t>(std::max<size_t>(ctx->rfTempBytes, 16), &t, false, &ctx->segmentAllocations)) return rc;
                ctx->rfTemp[g] = t;
            }
        // statistics: no room for a group's log: its sums are added atomically
        for (int g = 0; g < P.G && P.statLogged; ++g)
        {
            const unsigned long long want = P.statLogEntries;
            if (ctx->statCap[g] == want && ctx->statTemp[g] && ctx->statChunkFill[g]) continue;
            HIP_TRY(hipDeviceSynchronize());
            ctx->statCap[g] = 0;
            std::vector<GroupBuffer> buffers = {{ctx->statChunkFill[g], want / PMC_RF_LOG_CHUNK * sizeof(uint32_t)}};
            if (!ctx->statWaveBase[g])
                buffers.emplace_back(ctx->statWaveBase[g], PMC_STAT_LOG_WAVES * sizeof(unsigned long long), true),
                    buffers.emplace_back(ctx->statWaveFill[g], PMC_STAT_LOG_WAVES * sizeof(uint32_t));
            for (int k = 0; k < 2; ++k)
                buffers.emplace_back(ctx->statKeys[g][k], want * sizeof(uint32_t)), buffers.emplace_back(ctx->statVals[g][k], want * sizeof(double));
            if (!ctx->statTemp[g]) buffers.emplace_back(ctx->statTemp[g], pmcRfTempBytes(pmcRfMaxParts()));
            if (regrowGroupBuffers(ctx, size_t(want) * 24, size_t(2) << 30, buffers)) ctx->statCap[g] = want;
        }
        return PMC_OK;
    }

    unsigned long long* cursorSet(pmc_ctx* ctx, int g, int k) { return ctx->xcdCursors + (size_t(g) * (PMC_SORT_OBS + 1) + size_t(k)) * 8; }
    const unsigned long long* zeroCount(pmc_ctx* ctx) { return ctx->xcdCursors + size_t(PMC_MAX_GROUPS) * (PMC_SORT_OBS + 1) * 8; }

    StatLogArgs statLogOf(pmc_ctx* ctx, const SegmentPlan& P, int g)
    {
        StatLogArgs a = {nullptr, nullptr, 0ull, 0, nullptr, nullptr, nullptr};
        if (P.statLogged && ctx->statCap[g])
            a = {ctx->statKeys[g][0], ctx->statVals[g][0], ctx->statCap[g], PMC_CTR_STATLOG(g), ctx->statWaveBase[g], ctx->statWaveFill[g], ctx->statChunkFill[g]};
        return a;
    }
    // an empty log: no wave holds a chunk, every chunk counts as full until a wave leaves it open or short
    int statLogReset(pmc_ctx* ctx, const SegmentPlan& P, int g, hipStream_t stream)
    {
        if (!P.statLogged || !ctx->statCap[g]) return PMC_OK;
        HIP_TRY(hipMemsetAsync(ctx->dev.counters + PMC_CTR_STATLOG(g), 0, sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->statWaveFill[g]), (int)PMC_STAT_NO_CHUNK, PMC_STAT_LOG_WAVES, stream));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->statChunkFill[g]), PMC_RF_LOG_CHUNK, size_t(ctx->statCap[g] / PMC_RF_LOG_CHUNK), stream));
        return PMC_OK;
    }
    // the statistics log of group g (`claimed` entries) -> accumulator records, on `stream`; the cursor starts again at zero
    int statFlush(pmc_ctx* ctx, const SegmentPlan& P, int g, unsigned long long claimed, hipStream_t stream)
    {
        if (!P.statLogged || !ctx->statCap[g]) return PMC_OK;
        const unsigned long long n = std::min(claimed, ctx->statCap[g]) / PMC_RF_LOG_CHUNK * PMC_RF_LOG_CHUNK;
        if (n)
            HIP_TRY(pmcLaunchStatFlush(ctx->slot, ctx->statKeys[g][0], ctx->statVals[g][0], ctx->statKeys[g][1], ctx->statVals[g][1], n, P.statParts, ctx->statTemp[g],
                                       ctx->numCU, ctx->statChunkFill[g], stream));
        return statLogReset(ctx, P, g, stream);
    }
    // the radiation-field log of group g (`claimed` entries) -> table, on the group's stream
    int rfFlush(pmc_ctx* ctx, const SegmentPlan& P, int g, unsigned long long claimed)
    {
        const unsigned long long n = std::min(claimed, ctx->rfCap[g]);
        if (!P.rfLogged || n == 0) return PMC_OK;
        HIP_TRY(pmcLaunchRfFlush(ctx->slot, ctx->rfKeys[g][0], ctx->rfVals[g][0], ctx->rfKeys[g][1], ctx->rfVals[g][1], n, P.rfBuckets, ctx->rfTemp[g], ctx->numCU,
                                 ctx->groupStream[g]));
        return PMC_OK;
    }

    // every slot group starts with its share of the statistics pool, all of it free; the logs and counters start empty, the segment's clock starts
    int startSegment(pmc_ctx* ctx, const SegmentPlan& P)
    {
        DevScene& D = ctx->dev;
        hipStream_t st = ctx->stream;
        unsigned long long* ctr = D.counters;
        if (D.any_stats && ctx->statPoolBlocks)
        {
            const int64_t per = ctx->statPoolBlocks / P.G;
            unsigned long long freeCount[PMC_MAX_GROUPS] = {0, 0, 0, 0};
            bool changed = false;
            for (int g = 0; g < PMC_MAX_GROUPS; ++g)
            {
                const int32_t firstBlock = g < P.G ? int32_t(g * per) : 0, count = g < P.G ? int32_t(per) : 0;
                changed = changed || D.stat_pool_first[g] != firstBlock || D.stat_pool_count[g] != count;
                D.stat_pool_first[g] = firstBlock;
                D.stat_pool_count[g] = count;
                freeCount[g] = (unsigned long long)count;
            }
            if (changed)
            {
                HIP_TRY(hipStreamSynchronize(st));
                HIP_TRY(pmcUploadScene(ctx->slot, &D, st));
            }
            HIP_TRY(hipMemcpyAsync(D.stat_pool_free, ctx->statPoolIota, size_t(ctx->statPoolBlocks) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctr + PMC_CTR_STATFREE(0), freeCount, sizeof(freeCount), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));  // (freeCount lives on this frame)
        }
        for (int g = 0; g < P.G; ++g)
            if (int rc = statLogReset(ctx, P, g, st)) return rc;
        HIP_TRY(hipMemsetAsync(ctr + PMC_CTR_HISTORY, 0, sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(ctr + 32, 0, 4 * PMC_MAX_GROUPS * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(ctr + PMC_CTR_TASK(0, 0), 0, PMC_CTR_TASKS_PER_GROUP * PMC_MAX_GROUPS * sizeof(unsigned long long), st));
        HIP_TRY(hipEventRecord(ctx->evStart, st));
        for (int g = 0; g < PMC_MAX_GROUPS; ++g) ctx->readback[g].rfLogFill = 0, ctx->readback[g].statLogFill = 0;
        return PMC_OK;
    }


    // ---- statistics: the pool of list blocks GROWS when a slot group could run out of blocks in its next generation (round 6; rounds 1-5
    // failed the segment with PMC_ERR_OVERFLOW: the reference's list is a std::vector, FluxRecorder.hpp:327-338).  A history takes at most one
    // block per instrument and generation, so a group whose free blocks number at least its live slots x instruments with statistics cannot
    // run out; when they do not, everything in flight is waited for, the pool arrays are allocated anew with room for `add` more blocks (the
    // old contents copied, as a std::vector grows), the new blocks go to the free stack of the group that asked, and the scene constants are
    // uploaded again.  No device memory for it: the segment goes on with the pool it has (and fails loudly if that does run out).
    int growStatPool(pmc_ctx* ctx, int g, int64_t need)
    {
        DevScene& D = ctx->dev;
        unsigned long long* ctr = D.counters;
        HIP_TRY(hipDeviceSynchronize());
        unsigned long long freeNow[PMC_MAX_GROUPS] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(freeNow, ctr + PMC_CTR_STATFREE(0), sizeof(freeNow), hipMemcpyDeviceToHost));
        const int64_t old = ctx->statPoolBlocks;
        const int64_t add = std::min<int64_t>(std::max<int64_t>(2 * need, old), (int64_t(1) << 30) - old);
        if (add <= 0) return PMC_OK;
        size_t freeBytes = 0, totalBytes = 0;
        const size_t bytes = size_t(old + add) * (PMC_STAT_CAP * 12 + 12);
        if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && bytes + (size_t(1) << 30) > freeBytes)
        {
            static std::atomic<bool> said{false};
            if (!said.exchange(true))
                fprintf(stderr, "libpmc: the statistics lists of the histories in flight need more blocks than the pool of %lld has, and device %d has no room for "
                                "%.1f GB more: the segment goes on and fails if the pool does run out (PMC_NUM_SLOTS lowers the number of histories in flight)\n",
                        (long long)old, ctx->device, bytes * 1e-9);
            return PMC_OK;
        }
        int32_t *bin = nullptr, *next = nullptr, *stack = nullptr, *iota = nullptr;
        double* w = nullptr;
        auto* own = &ctx->slotAllocations;
        int rc;
        if ((rc = ctx->allocate<int32_t>(size_t(old + add) * PMC_STAT_CAP, &bin, false, own))) return rc;
        if ((rc = ctx->allocate<double>(size_t(old + add) * PMC_STAT_CAP, &w, false, own))) return rc;
        if ((rc = ctx->allocate<int32_t>(size_t(old + add), &next, false, own))) return rc;
        if ((rc = ctx->allocate<int32_t>(size_t(old + add), &stack, false, own))) return rc;
        if ((rc = ctx->allocate<int32_t>(size_t(old + add), &iota, false, own))) return rc;
        HIP_TRY(hipMemcpy(bin, D.stat_pool_bin, size_t(old) * PMC_STAT_CAP * sizeof(int32_t), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(w, D.stat_pool_w, size_t(old) * PMC_STAT_CAP * sizeof(double), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(next, D.stat_pool_next, size_t(old) * sizeof(int32_t), hipMemcpyDeviceToDevice));
        std::vector<int32_t> ids(static_cast<size_t>(old + add));
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)i;
        HIP_TRY(hipMemcpy(iota, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        // the free stacks: every group keeps its stack (its first freeNow entries), the new ids go on top of group g's
        int32_t first = 0;
        for (int h = 0; h < PMC_MAX_GROUPS; ++h)
        {
            const int32_t count = D.stat_pool_count[h] + (h == g ? int32_t(add) : 0);
            if (D.stat_pool_count[h] > 0 && freeNow[h] > 0)
                HIP_TRY(hipMemcpy(stack + first, D.stat_pool_free + D.stat_pool_first[h], size_t(freeNow[h]) * sizeof(int32_t), hipMemcpyDeviceToDevice));
            if (h == g) HIP_TRY(hipMemcpy(stack + first + freeNow[h], ids.data() + old, size_t(add) * sizeof(int32_t), hipMemcpyHostToDevice));
            D.stat_pool_first[h] = first;
            D.stat_pool_count[h] = count;
            first += count;
        }
        freeNow[g] += (unsigned long long)add;
        HIP_TRY(hipMemcpy(ctr + PMC_CTR_STATFREE(0), freeNow, sizeof(freeNow), hipMemcpyHostToDevice));
        // the old arrays
        ctx->release(D.stat_pool_bin, own), ctx->release(D.stat_pool_w, own), ctx->release(D.stat_pool_next, own), ctx->release(D.stat_pool_free, own);
        ctx->release(ctx->statPoolIota, own);
        D.stat_pool_bin = bin, D.stat_pool_w = w, D.stat_pool_next = next, D.stat_pool_free = stack;
        ctx->statPoolIota = iota;
        ctx->statPoolBlocks = old + add;
        ctx->readback[g].statFreeBlocks = freeNow[g];
        ctx->statPoolGrowths += 1;
        HIP_TRY(pmcUploadScene(ctx->slot, &D, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PMC_OK;
    }

    // octree: one peel-off kernel per observer on the group's side stream, next to the propagation kernel on the group's stream (they touch different
    // task records and result fields); listIn: the group's live slots (a sparse generation)
    int enqueueOctreeWalks(pmc_ctx* ctx, const SegmentPlan& P, const SegmentRun& S, int g, const int* listIn, int listLen)
    {
        const DevScene& D = ctx->dev;
        hipStream_t sg = ctx->groupStream[g], sp = P.serialWalks ? sg : ctx->peelStream[g];
        const int numTasks = listIn ? listLen : P.size[g];
        const int peelLanes = pmcPeelBlock() * P.listTasksPerLane, propLanes = pmcPropBlock() * P.listTasksPerLane;
        const int peelGrid = listIn ? std::max(1, std::min(ctx->peelGrid, (numTasks + peelLanes - 1) / peelLanes)) : ctx->peelGrid;
        const int propGrid = listIn ? std::max(1, std::min(ctx->grid, (numTasks + propLanes - 1) / propLanes)) : ctx->grid;
        HIP_TRY(hipStreamWaitEvent(sp, ctx->evA[g], 0));
        for (int i = 0; i < D.num_instruments; ++i)
            if (!D.inst[i].same_observer)
            {
                int k = -1;
                for (int q = 0; q < P.numSortObs; ++q)
                    if (P.sortObs[q] == i) k = q;
                const bool sorted = S.peelSorted[g] && !listIn && k >= 0;
                HIP_TRY(pmcLaunchPeel(ctx->slot, P.peelForm, P.base[g], numTasks, sorted ? nullptr : listIn, PMC_CTR_TASK(g, 1 + i), i, (int)D.inst[i].sgn, peelGrid,
                                      ctx->walkLds, sorted ? ctx->peelRec[g][k] : nullptr, sorted ? pmcPeelSortedCount(ctx->peelTemp[g][k]) : nullptr,
                                      sorted && P.xcdAffinity ? cursorSet(ctx, g, k) : nullptr, sp));
            }
        HIP_TRY(hipEventRecord(ctx->evJoin[g], sp));
        RfLogArgs log = {ctx->rfKeys[g][0], ctx->rfVals[g][0], P.rfLogged ? ctx->rfCap[g] : 0ull, PMC_CTR_RFLOG(g), P.rfPadKey};
        if (P.serialWalks) HIP_TRY(hipEventRecord(ctx->evProp[g], sg));  // (in series: the propagation kernel starts where the peel-off kernels end)
        HIP_TRY(pmcLaunchProp(ctx->slot, ctx->wide, P.walkFlavour, P.propCheckpoints, P.base[g], numTasks, listIn, PMC_CTR_TASK(g, 0), P.seed, propGrid, ctx->walkLds,
                              &log, sg));
        if (!P.serialWalks) HIP_TRY(hipEventRecord(ctx->evProp[g], sg));
        HIP_TRY(hipStreamWaitEvent(sg, ctx->evJoin[g], 0));
        return PMC_OK;
    }

    // Cartesian, Voronoi.  Sorted observers: one stream of single walks -- the propagation walks in slot order, then every observer's peel-off walks
    // in the order of the detector tile they start behind -- with the Voronoi kernels of their own taking their part of it
    int enqueueGenericWalks(pmc_ctx* ctx, const SegmentPlan& P, const SegmentRun& S, int g)
    {
        const DevScene& D = ctx->dev;
        hipStream_t sg = ctx->groupStream[g];
        // (the sorted observers whose peel-off walks the Voronoi peel-off kernel takes)
        auto ownPeel = [&](int k) { return P.voroPeelKernels && D.vobs_of_inst[P.sortObs[k]] >= 0; };
        WalkStreamArgs tasks;
        std::memset(&tasks, 0, sizeof(tasks));
        bool streamEmpty = false;
        if (S.peelSorted[g])
        {
            tasks.numLists = P.numSortObs;
            for (int k = 0; k < P.numSortObs; ++k)
                tasks.rec[k] = 1 + P.sortObs[k], tasks.list[k] = ctx->peelList[g][k], tasks.count[k] = pmcPeelSortedCount(ctx->peelTemp[g][k]);
            tasks.xcdCursor = P.xcdAffinity ? cursorSet(ctx, g, 0) : nullptr;
            if (P.propSortIndex >= 0)
                tasks.propList = ctx->peelList[g][P.propSortIndex], tasks.propCount = pmcPeelSortedCount(ctx->peelTemp[g][P.propSortIndex]);
            // (lists that the Voronoi peel-off kernel takes, below: empty for the stream)
            bool left = false;  // does the stream keep a list?
            for (int k = 0; k < P.numSortObs; ++k)
                if (ownPeel(k))
                    tasks.count[k] = zeroCount(ctx);
                else
                    left = true;
            // (the list is in cone order: ONE cursor, all XCDs on the same cone table at a time -- 490 against 493 ms of walk kernels per 2e7 packets
            // with an eighth of the list per XCD, profiles/sweeps/r05_i15)
            if (P.voroPropKernel && P.propSortIndex >= 0)
            {
                HIP_TRY(pmcLaunchVoroProp(ctx->slot, tasks.propList, tasks.propCount, cursorSet(ctx, g, PMC_SORT_OBS), P.voroPropSegments, P.seed, P.walkFlavour,
                                          P.voroPropGrid, sg));
                tasks.propCount = zeroCount(ctx);
            }
            else
                left = true;
            streamEmpty = !left;
        }
        if (!streamEmpty)
            HIP_TRY(pmcLaunchWalk(ctx->slot, D.grid_kind, P.walkFlavour, P.base[g], P.size[g], PMC_CTR_TASK(g, 0), P.seed, ctx->grid, ctx->block, ctx->walkLds,
                                  S.peelSorted[g] ? &tasks : nullptr, sg));
        if (!S.peelSorted[g]) return PMC_OK;
        // the peel-off kernels on the group's side stream next to the propagation kernel (as on the octree: one is bound by the lines it
        // gets from beyond L2, the others by instructions and the L1's access rate); `PMC_VORO_WALKS_IN_SERIES`: behind it, one stream
        bool anyPeel = false;
        for (int k = 0; k < P.numSortObs; ++k) anyPeel = anyPeel || ownPeel(k);
        const bool side = anyPeel && P.voroPropKernel && P.propSortIndex >= 0 && !P.serialWalks && !P.voroWalksInSeries;
        hipStream_t sp = side ? ctx->peelStream[g] : sg;
        if (side) HIP_TRY(hipStreamWaitEvent(sp, ctx->evA[g], 0));
        for (int k = 0; k < P.numSortObs; ++k)
            if (ownPeel(k))
                HIP_TRY(pmcLaunchVoroPeel(ctx->slot, 1 + P.sortObs[k], D.vobs_of_inst[P.sortObs[k]], ctx->peelList[g][k], pmcPeelSortedCount(ctx->peelTemp[g][k]),
                                          cursorSet(ctx, g, 1 + k), P.xcdAffinity ? 8 : 1, D.num_media > 1 ? 1 : 0, P.voroPeelGrid, sp));
        if (side)
        {
            HIP_TRY(hipEventRecord(ctx->evJoin[g], sp));
            HIP_TRY(hipStreamWaitEvent(sg, ctx->evJoin[g], 0));
        }
        return PMC_OK;
    }

    // every live slot of the group is at the start of a cycle now: the start states of its walks -- and, once the live slots of the previous
    // generation were fewer than half of the group's, their list for the next generation.  (The launch kernel fills every slot whose history has
    // ended as long as SourceSystem has an index left: fewer live slots than slots means that nothing is left to launch, and the live slots can
    // only become fewer.)  Then the words the host reads back with the generation.
    int enqueueCycleStart(pmc_ctx* ctx, const SegmentPlan& P, SegmentRun& S, int g, bool initial, const int* listIn, int listLen)
    {
        DevScene& D = ctx->dev;
        hipStream_t sg = ctx->groupStream[g];
        unsigned long long* ctr = D.counters;
        GroupReadback& rb = ctx->readback[g];
        const bool buildList = P.sparseLists && !initial && (listIn || rb.live < (unsigned long long)(P.size[g] / 2));
        if (listIn) S.listHalf[g] ^= 1;
        int* const listOut = D.tasks.liveList + int64_t(S.listHalf[g]) * D.slots.num_slots + P.base[g];
        const bool sortNow = P.numSortObs > 0 && !buildList && !listIn;
        PeelSortArgs sortArgs = P.sortArgs;
        sortArgs.cap = (uint32_t)ctx->peelCap[g];
        int sortGroups = 0;
        // (sorted peel-off records: the sort's count pass over the slots as the transition / launch kernels left them; the cycle start kernel,
        // with the same workgroups, is its scatter pass)
        if (sortNow)
            HIP_TRY(pmcLaunchPeelSortCounts(ctx->slot, P.base[g], P.size[g], &sortArgs, P.octree ? ctx->peelRec[g] : nullptr, P.octree ? nullptr : ctx->peelList[g],
                                            ctx->peelTemp[g], &sortGroups, sg));
        HIP_TRY(pmcLaunchCycleStart(ctx->slot, D.grid_kind, D.kin, P.base[g], P.size[g], buildList ? PMC_CTR_LIST(g) : -1, listOut, listIn, listLen,
                                    sortNow ? sortGroups : P.cycleBlocks, ctx->walkLds, sortNow ? &sortArgs : nullptr, sg));
        S.peelSorted[g] = sortNow;
        S.listBuilt[g] = buildList;
        HIP_TRY(hipEventRecord(ctx->evC[g], sg));
        const size_t word = sizeof(unsigned long long);
        HIP_TRY(hipMemcpyAsync(&rb.live, ctr + PMC_CTR_LIVE(g), word, hipMemcpyDeviceToHost, sg));
        if (P.rfLogged && !initial) HIP_TRY(hipMemcpyAsync(&rb.rfLogFill, ctr + PMC_CTR_RFLOG(g), word, hipMemcpyDeviceToHost, sg));
        if (ctx->progress) HIP_TRY(hipMemcpyAsync(&rb.historyCursor, ctr + PMC_CTR_HISTORY, word, hipMemcpyDeviceToHost, sg));
        if (P.statLogged && !initial && ctx->statCap[g]) HIP_TRY(hipMemcpyAsync(&rb.statLogFill, ctr + PMC_CTR_STATLOG(g), word, hipMemcpyDeviceToHost, sg));
        if (P.poolGrows) HIP_TRY(hipMemcpyAsync(&rb.statFreeBlocks, ctr + PMC_CTR_STATFREE(g), word, hipMemcpyDeviceToHost, sg));
        return PMC_OK;
    }

    // one generation of group g on its stream: the launch into every slot (initial), or the flushes of the logs its previous generation filled,
    // the walks, the transition and the launches into the slots whose history ended; then the start of the next cycle
    int enqueueGeneration(pmc_ctx* ctx, const SegmentPlan& P, SegmentRun& S, int g, bool initial)
    {
        const DevScene& D = ctx->dev;
        hipStream_t sg = ctx->groupStream[g];
        unsigned long long* ctr = D.counters;
        GroupReadback& rb = ctx->readback[g];
        // the list of live slots the previous generation left (as many as its live count, which came back with the stream)
        int* const listIn = (!initial && S.listBuilt[g]) ? D.tasks.liveList + int64_t(S.listHalf[g]) * D.slots.num_slots + P.base[g] : nullptr;
        const int listLen = listIn ? int(rb.live) : 0;
        if (initial)
        {
            if (g > 0) HIP_TRY(hipStreamWaitEvent(sg, ctx->evStart, 0));
            HIP_TRY(hipEventRecord(ctx->evB[g], sg));
            // (the same persistent workgroups as every later generation: every slot takes a history)
            HIP_TRY(pmcLaunchLaunch(ctx->slot, P.launchFlavour, P.base[g], P.size[g], g, P.first, P.count, P.seed, 1, P.launchBlocks, ctx->launchLds, nullptr, sg));
            return enqueueCycleStart(ctx, P, S, g, initial, listIn, listLen);
        }
        if (P.poolGrows)
        {
            // (the group's free blocks came back with its live count: enough for one block per live slot and instrument with statistics?)
            // (only once blocks have been taken at all -- histories of more than 48 distinct pixels exist in this scene --, or when the ski file asks for
            // many scattering events per history: a scene whose lists stay short never touches the pool, however small it is; and not again in a
            // segment in which the device had no room for more)
            const int64_t need = int64_t(rb.live) * P.statInstruments, freeBlocks = int64_t(rb.statFreeBlocks);
            const bool inUse = freeBlocks < int64_t(D.stat_pool_count[g]) || D.min_scatt_events > 16;
            if (inUse && freeBlocks < need && !S.poolCannotGrow)
            {
                const int64_t before = ctx->statPoolBlocks;
                if (int rc = growStatPool(ctx, g, need)) return rc;
                S.poolCannotGrow = ctx->statPoolBlocks == before;
            }
        }
        // (the radiation-field log of the group's previous generation: its size came back with the live count)
        if (int rc = rfFlush(ctx, P, g, rb.rfLogFill)) return rc;
        rb.rfLogFill = 0;
        // (the statistics log of the group, once half full: its fill came back with the live count)
        if (rb.statLogFill > ctx->statCap[g] / 2)
        {
            if (int rc = statFlush(ctx, P, g, rb.statLogFill, sg)) return rc;
            rb.statLogFill = 0;
        }
        HIP_TRY(hipMemsetAsync(ctr + PMC_CTR_TASK(g, 0), 0, PMC_CTR_TASKS_PER_GROUP * sizeof(unsigned long long), sg));  // task cursors
        if (ctx->xcdCursors) HIP_TRY(hipMemsetAsync(cursorSet(ctx, g, 0), 0, (PMC_SORT_OBS + 1) * 8 * sizeof(unsigned long long), sg));
        HIP_TRY(hipEventRecord(ctx->evA[g], sg));
        if (int rc = P.octree ? enqueueOctreeWalks(ctx, P, S, g, listIn, listLen) : enqueueGenericWalks(ctx, P, S, g)) return rc;
        S.haveWalk[g] = true;
        HIP_TRY(hipEventRecord(ctx->evB[g], sg));
        HIP_TRY(hipMemsetAsync(ctr + PMC_CTR_LIVE(g), 0, sizeof(unsigned long long), sg));
        const StatLogArgs statLog = statLogOf(ctx, P, g);
        HIP_TRY(pmcLaunchTransition(ctx->slot, (ctx->dev.any_dipole ? 1 : 0) | (ctx->dev.kin ? 2 : 0), P.base[g], P.size[g], g, P.seed, listIn, listLen, P.transitionBlocks, ctx->transitionLds, &statLog, P.count, sg));
        if (!listIn)
            HIP_TRY(pmcLaunchLaunch(ctx->slot, P.launchFlavour, P.base[g], P.size[g], g, P.first, P.count, P.seed, 0, P.launchBlocks, ctx->launchLds, &statLog, sg));
        return enqueueCycleStart(ctx, P, S, g, initial, listIn, listLen);
    }

    // the generations of all groups until none has a live slot: the host waits for the groups in turn and enqueues the next generation of the
    // one it has waited for
    int drive(pmc_ctx* ctx, const SegmentPlan& P, SegmentRun& S)
    {
        auto lastReport = std::chrono::steady_clock::now();
        const auto segmentStart = lastReport;
        uint64_t reported = 0;
        int remaining = 0;
        for (int g = 0; g < P.G; ++g)
        {
            S.active[g] = P.size[g] > 0;
            remaining += S.active[g] ? 1 : 0;
        }
        for (int g = 0; g < P.G; ++g)
            if (S.active[g])
                if (int rc = enqueueGeneration(ctx, P, S, g, true)) return rc;
        for (int g = 0; remaining > 0; g = (g + 1) % P.G)
        {
            if (!S.active[g]) continue;
            HIP_TRY(hipStreamSynchronize(ctx->groupStream[g]));
            GroupReadback& rb = ctx->readback[g];
            float ms = 0, walkOfGen = 0;
            if (S.haveWalk[g])
            {
                HIP_TRY(hipEventElapsedTime(&ms, ctx->evA[g], ctx->evB[g]));
                S.walkMs += ms;
                walkOfGen = ms;
                if (P.octree)
                {
                    // the two kernel kinds of the generation: side by side on two streams (each span starts at evA), or in series
                    HIP_TRY(hipEventElapsedTime(&ms, ctx->evA[g], ctx->evJoin[g]));
                    S.peelMs += ms;
                    if (P.serialWalks)
                        HIP_TRY(hipEventElapsedTime(&ms, ctx->evProp[g], ctx->evB[g]));
                    else
                        HIP_TRY(hipEventElapsedTime(&ms, ctx->evA[g], ctx->evProp[g]));
                    S.propMs += ms;
                }
            }
            HIP_TRY(hipEventElapsedTime(&ms, ctx->evB[g], ctx->evC[g]));
            S.transMs += ms;
            if (rb.live == 0)
            {
                // (the group's last log)
                if (int rc = rfFlush(ctx, P, g, rb.rfLogFill)) return rc;
                rb.rfLogFill = 0;
                S.active[g] = false;
                --remaining;
                continue;
            }
            ++S.generations;
            if (ctx->progress)
            {
                // (the history cursor came back with the group's live count; it runs past `count` when the last indices are handed out)
                const auto now = std::chrono::steady_clock::now();
                if (std::chrono::duration<double>(now - lastReport).count() >= ctx->progressInterval)
                {
                    lastReport = now;
                    // (every group copies the cursor into a word of its own, on its own stream; this group's copy is complete -- its
                    // stream has just been waited for -- and the report never goes backwards: a running maximum)
                    reported = std::max<uint64_t>(reported, std::min<uint64_t>(rb.historyCursor, P.count));
                    ctx->progress(ctx->progressUser, reported, P.count);
                }
            }
            if (P.genDump)
                fprintf(stderr, "PMC_GEN %d group %d live %llu walk_ms %.3f transition_ms %.3f at_ms %.3f\n", S.generations, g, rb.live,
                        S.haveWalk[g] ? walkOfGen : 0.f, ms, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - segmentStart).count());
            if (int rc = enqueueGeneration(ctx, P, S, g, false)) return rc;
        }
        return PMC_OK;
    }

    // the end of the segment: what is left in the groups' statistics logs -- the fills that came back with the groups' last generations are
    // final (drive has waited for every group); the groups' flushes run side by side on their streams --, the statistics merge, the clock
    int finish(pmc_ctx* ctx, const SegmentPlan& P)
    {
        if (P.statLogged)
            for (int g = 0; g < P.G; ++g)
                if (int rc = statFlush(ctx, P, g, ctx->readback[g].statLogFill, ctx->groupStream[g])) return rc;
        // (the last radiation-field logs of the groups are reduced on their streams too)
        if (P.rfLogged || P.statLogged)
            for (int g = 0; g < P.G; ++g) HIP_TRY(hipStreamSynchronize(ctx->groupStream[g]));
        // the segment's statistics: accumulator records -> wifu arrays
        if (ctx->dev.stat_acc_records) HIP_TRY(pmcLaunchStatMerge(ctx->slot, ctx->numCU * 8, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->evStop, ctx->stream));
        HIP_TRY(hipEventSynchronize(ctx->evStop));
        HIP_TRY(hipEventElapsedTime(&ctx->totalMs, ctx->evStart, ctx->evStop));
        return PMC_OK;
    }

    // on any failure in the generations or at the end: no kernel of this segment may still be running (or be timed) when the call returns
    int abandon(pmc_ctx* ctx, int code)
    {
        hipDeviceSynchronize();
        // (the statistics of the abandoned segment must not reach the frames with the next one)
        if (ctx->dev.stat_acc_records) hipMemset(ctx->dev.stat_acc, 0, size_t(ctx->dev.stat_acc_records) * 8 * sizeof(double));
        ctx->timed = false;
        return code;
    }

    // the errors the kernels count
    int checkKernelErrors(pmc_ctx* ctx)
    {
        const unsigned long long* ctr = ctx->dev.counters;
        // internal errors (a sorted peel-off record without a place: see peelTile, pmc_cycle.inc)
        {
            unsigned long long tail[3] = {0, 0, 0};  // counters 5 .. 7
            HIP_TRY(hipMemcpy(tail, ctr + 5, sizeof(tail), hipMemcpyDeviceToHost));
            if (tail[2] > ctx->internalErrorsSeen)
            {
                const unsigned long long fresh = tail[2] - ctx->internalErrorsSeen;
                ctx->internalErrorsSeen = tail[2];
                return fail(PMC_ERR_DEVICE, std::to_string(fresh) + " peel-off walks found no place in the sorted records (the two passes of the sort disagree): the segment's results are incomplete");
            }
        }
        // a history with more distinct pixels than the statistics list holds: the statistics arrays are wrong -- say so
        if (ctx->dev.any_stats)
        {
            unsigned long long overflows = 0;
            HIP_TRY(hipMemcpy(&overflows, ctr + 5, sizeof(overflows), hipMemcpyDeviceToHost));
            if (overflows > ctx->overflowsSeen)
            {
                const unsigned long long fresh = overflows - ctx->overflowsSeen;
                ctx->overflowsSeen = overflows;
                return fail(PMC_ERR_OVERFLOW, std::to_string(fresh) + " photon histories lost contributions to the statistics arrays: the pool of "
                                                  + std::to_string(ctx->statPoolBlocks) + " list blocks (" + std::to_string(PMC_STAT_CAP)
                                                  + " distinct pixels each) ran out; the statistics arrays of this segment are incomplete.  Raise "
                                                    "PMC_STAT_POOL_BLOCKS, or lower PMC_NUM_SLOTS (fewer histories in flight)");
            }
        }
        return PMC_OK;
    }

    // ---- test aid pmc_tune_walk_cycle (include/pmc_tuning.h): the cycle start and the walks of ONE generation of slot group 0 on slot states the
    // host supplies.  The plan, the buffers and the enqueue functions are pmc_run_primary's; what is the aid's own is the upload of the slot
    // state, the download of the walks' results and the bookkeeping around them.

    // what is wrong with the arguments, or an empty string
    std::string walkCycleProblem(const pmc_ctx* ctx, const pmc_walk_cycle_in& in, const pmc_walk_cycle_out& out, const std::vector<int32_t>& cellExt)
    {
        const DevScene& D = ctx->dev;
        const int64_t n = in.n;
        if (n < 1) return "at least one slot";
        if (!in.r || !in.k || !in.mask || !in.ppW || !in.hint || !in.nscatt) return "null array (r, k, mask, ppW, hint, nscatt)";
        if (!out.ptau || !out.sint || !out.nint || !out.mint || !out.taupath || !out.tausample) return "null result array";
        if (D.force_scattering ? (!in.u1 || !in.u2) : !in.depth) return D.force_scattering ? "forced scattering needs u1 and u2" : "the scene needs the drawn depth";
        if (!D.mono && (!in.lambda || !in.dust_ext || !in.dust_sca)) return "a scene with more than one wavelength needs lambda, dust_ext and dust_sca";
        if (!D.mono && D.explicit_absorption && !in.dust_abs) return "explicit absorption needs dust_abs";
        if (!D.mono && D.num_media > 1 && !in.dust_idx) return "several medium components need dust_idx";
        if (D.rf_store && (!in.W || !in.rfell)) return "a stored radiation field needs W and rfell";
        if (in.live_list != 0 && in.live_list != 1) return "live_list is 0 or 1";
        const bool numbered = !cellExt.empty();
        const int64_t cells = numbered ? int64_t(cellExt.size()) : int64_t(D.num_cells);
        uint32_t leaders = 0;
        for (int i = 0; i < D.num_instruments; ++i)
            if (!D.inst[i].same_observer) leaders |= 1u << i;
        for (int64_t i = 0; i < n; ++i)
        {
            const std::string at = " (slot " + std::to_string(i) + ")";
            double k2 = 0.;
            for (int a = 0; a < 3; ++a)
            {
                if (!std::isfinite(in.r[3 * i + a])) return "a position that is not finite" + at;
                if (!std::isfinite(in.k[3 * i + a])) return "a direction that is not finite" + at;
                k2 += in.k[3 * i + a] * in.k[3 * i + a];
            }
            if (!(std::fabs(std::sqrt(k2) - 1.) <= 1e-12)) return "a direction that is no unit vector" + at;
            const uint32_t mask = (uint32_t)in.mask[i];
            if (mask & ~0x00FFFF00u) return "a mask with bits outside 8-23" + at;
            if ((mask >> 8) & ~leaders) return "a mask that names an instrument which leads no observer group" + at;
            for (int q = 0; q < D.num_instruments; ++q)
                if (((mask >> (8 + q)) & 1u) && std::isnan(in.ppW[int64_t(q) * n + i])) return "a peel-off weight that is not a number" + at;
            if (in.hint[i] < -1 || in.hint[i] >= cells || (numbered && in.hint[i] >= 0 && cellExt[in.hint[i]] < 0)) return "a hint outside the cell table" + at;
            if (in.nscatt[i] < 1) return "nscatt must be positive: the aid starts no emission cycle" + at;
            if (D.force_scattering)
            {
                if (!(in.u1[i] >= 0. && in.u1[i] < 1.) || !(in.u2[i] >= 0. && in.u2[i] < 1.)) return "a uniform outside [0, 1)" + at;
            }
            else if (!(in.depth[i] >= 0.))
                return "a drawn depth that is negative or not a number" + at;
            if (!D.mono)
            {
                if (!(in.lambda[i] > 0.) || !std::isfinite(in.lambda[i])) return "a wavelength that is not positive and finite" + at;
                if (!(in.dust_ext[i] >= 0.) || !std::isfinite(in.dust_ext[i]) || !(in.dust_sca[i] >= 0.) || !std::isfinite(in.dust_sca[i]))
                    return "a cross section that is negative or not finite" + at;
                if (D.explicit_absorption && (!(in.dust_abs[i] >= 0.) || !std::isfinite(in.dust_abs[i]))) return "an absorption cross section that is negative or not finite" + at;
                for (int h = 0; D.num_media > 1 && h < D.num_media; ++h)
                    if (in.dust_idx[int64_t(h) * n + i] < 0 || in.dust_idx[int64_t(h) * n + i] >= D.med[h].num_lambda) return "a wavelength index outside a component's tables" + at;
            }
            if (D.rf_store)
            {
                if (!std::isfinite(in.W[i])) return "a weight that is not finite" + at;
                if (in.rfell[i] < -1 || in.rfell[i] >= D.rf_num_lambda) return "a bin outside the radiation field's grid" + at;
            }
        }
        if (in.live_list && in.list)
        {
            std::vector<char> seen(size_t(n), 0);
            for (int64_t i = 0; i < n; ++i)
            {
                if (in.list[i] < 0 || in.list[i] >= n || seen[in.list[i]]) return "the list is no permutation of the slots";
                seen[in.list[i]] = 1;
            }
        }
        return "";
    }

    // the plan of a segment over the whole pool, as pmc_run_primary makes it, with its buffers
    int planWalkCycle(pmc_ctx* ctx, SegmentPlan& P)
    {
        int numSlots = 0;
        if (int rc = provisionSlots(ctx, uint64_t(std::max<int64_t>(ctx->numSlots, 1)), &numSlots)) return rc;
        P = planSegment(ctx, numSlots, 0, uint64_t(numSlots), 0);
        if (int rc = provisionSortBuffers(ctx, P)) return rc;
        return provisionLogs(ctx, P);
    }

    template<typename T> hipError_t putSlots(hipError_t e, T* device, int base, const T* host, size_t count, hipStream_t stream)
    {
        if (e == hipSuccess && host && device) e = hipMemcpyAsync(device + base, host, sizeof(T) * count, hipMemcpyHostToDevice, stream);
        return e;
    }
    template<typename T> hipError_t getSlots(hipError_t e, T* host, const T* device, int base, size_t count, hipStream_t stream)
    {
        if (e == hipSuccess) e = hipMemcpyAsync(host, device + base, sizeof(T) * count, hipMemcpyDeviceToHost, stream);
        return e;
    }

    // the segment's start, the slot states, the generation, the results; after[32]: the counters behind the walks.  Any failure returns at
    // once: runWalkCycle abandons what is in flight
    int enqueueWalkCycle(pmc_ctx* ctx, const SegmentPlan& P, const pmc_walk_cycle_in& in, pmc_walk_cycle_out& out, unsigned long long* after)
    {
        DevScene& D = ctx->dev;
        const SlotArrays& A = D.slots;
        const TaskArrays& K = D.tasks;
        const int g = 0, base = P.base[g], size = P.size[g];
        const size_t n = size_t(in.n);
        const int64_t NS = A.num_slots;
        hipStream_t sg = ctx->groupStream[g];
        unsigned long long* ctr = D.counters;
        if (int rc = startSegment(ctx, P)) return rc;
        // ---- the group as the transition and launch kernels leave it when nothing is left to launch: no slot alive, no task record in use ...
        HIP_TRY(hipMemsetAsync(A.mode + base, 0, sizeof(int32_t) * size_t(size), sg));
        for (int r = 0; r <= D.num_instruments; ++r)
            HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(K.bits + int64_t(r) * NS + base), (int)PMC_TASK_NONE, size_t(size), sg));
        // ---- ... but for the first n slots, which hold what the host supplies: the state at the start of a cycle (announceCycle, onCycleDone)
        std::vector<double> soa[6];
        for (int a = 0; a < 3; ++a)
        {
            soa[a].resize(n), soa[3 + a].resize(n);
            for (size_t i = 0; i < n; ++i) soa[a][i] = in.r[3 * i + a], soa[3 + a][i] = in.k[3 * i + a];
        }
        std::vector<int32_t> mode(n);
        for (size_t i = 0; i < n; ++i) mode[i] = PMC_MODE_ALIVE | in.mask[i];
        const std::vector<double> unset(n, PMC_WALK_CYCLE_UNSET), zeros(n, 0.);
        std::vector<uint64_t> history(n);
        for (size_t i = 0; i < n; ++i) history[i] = i;
        const std::vector<uint32_t> noBlock(n, 0u);
        hipError_t e = hipSuccess;
        double* const pos[6] = {A.rx, A.ry, A.rz, A.kx, A.ky, A.kz};
        for (int a = 0; a < 6; ++a) e = putSlots(e, pos[a], base, soa[a].data(), n, sg);
        e = putSlots(e, A.mode, base, mode.data(), n, sg);
        e = putSlots(e, A.nscatt, base, in.nscatt, n, sg);
        e = putSlots(e, A.mint, base, in.hint, n, sg);
        for (int q = 0; q < D.num_instruments; ++q)
        {
            e = putSlots(e, A.ppW + int64_t(q) * NS, base, in.ppW + size_t(q) * n, n, sg);
            e = putSlots(e, A.ptau + int64_t(q) * NS, base, unset.data(), n, sg);
        }
        e = putSlots(e, A.sint, base, D.force_scattering ? in.u1 : unset.data(), n, sg);
        e = putSlots(e, A.nint, base, D.force_scattering ? in.u2 : unset.data(), n, sg);
        e = putSlots(e, A.tausample, base, D.force_scattering ? unset.data() : in.depth, n, sg);
        e = putSlots(e, A.taupath, base, unset.data(), n, sg);
        // (the random stream of a slot: read only by a rejection round of the exponential branch, which rounding alone can cause)
        e = putSlots(e, A.history, base, history.data(), n, sg);
        e = putSlots(e, A.rngBlock, base, noBlock.data(), n, sg);
        e = putSlots(e, A.rngSpare, base, zeros.data(), n, sg);
        if (!D.mono)
        {
            e = putSlots(e, A.lambda, base, in.lambda, n, sg);
            e = putSlots(e, A.dustExt, base, in.dust_ext, n, sg);
            e = putSlots(e, A.dustSca, base, in.dust_sca, n, sg);
            e = putSlots(e, A.dustAbs, base, in.dust_abs, n, sg);
            for (int h = 0; A.dustIdx && h < D.num_media; ++h) e = putSlots(e, A.dustIdx + int64_t(h) * NS, base, in.dust_idx + size_t(h) * n, n, sg);
        }
        if (D.rf_store)
        {
            e = putSlots(e, A.W, base, in.W, n, sg);
            e = putSlots(e, A.rfell, base, in.rfell, n, sg);
        }
        // the list of a sparse generation, as the cycle start kernel of the generation before it would have left it in one half of liveList
        SegmentRun S{};
        std::vector<int32_t> list(n);
        int* listIn = nullptr;
        if (in.live_list)
        {
            for (size_t i = 0; i < n; ++i) list[i] = base + (in.list ? in.list[i] : int32_t(i));
            listIn = K.liveList + int64_t(S.listHalf[g]) * NS + base;
            e = putSlots(e, K.liveList + int64_t(S.listHalf[g]) * NS, base, list.data(), n, sg);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(sg);  // (the host buffers above live on this frame)
        if (e != hipSuccess) return hipFail(e, "pmc_tune_walk_cycle: upload");
        // ---- the generation, as enqueueGeneration orders it: cursors, cycle start (a group most of whose slots are live: no list is built unless
        // the generation runs over one), walks
        ctx->readback[g].live = (unsigned long long)size;
        HIP_TRY(hipMemsetAsync(ctr + PMC_CTR_TASK(g, 0), 0, PMC_CTR_TASKS_PER_GROUP * sizeof(unsigned long long), sg));
        if (ctx->xcdCursors) HIP_TRY(hipMemsetAsync(cursorSet(ctx, g, 0), 0, (PMC_SORT_OBS + 1) * 8 * sizeof(unsigned long long), sg));
        if (int rc = enqueueCycleStart(ctx, P, S, g, false, listIn, listIn ? int(n) : 0)) return rc;
        HIP_TRY(hipEventRecord(ctx->evA[g], sg));
        if (int rc = P.octree ? enqueueOctreeWalks(ctx, P, S, g, listIn, listIn ? int(n) : 0) : enqueueGenericWalks(ctx, P, S, g)) return rc;
        // (the radiation-field log of the generation: its size, then the flush of the generation after it)
        unsigned long long rfFill = 0;
        if (P.rfLogged)
        {
            HIP_TRY(hipMemcpyAsync(&rfFill, ctr + PMC_CTR_RFLOG(g), sizeof(rfFill), hipMemcpyDeviceToHost, sg));
            HIP_TRY(hipStreamSynchronize(sg));
            if (int rc = rfFlush(ctx, P, g, rfFill)) return rc;
        }
        // ---- the results as the walk kernels leave them
        for (int q = 0; q < D.num_instruments; ++q) e = getSlots(e, out.ptau + size_t(q) * n, A.ptau + int64_t(q) * NS, base, n, sg);
        e = getSlots(e, out.sint, A.sint, base, n, sg);
        e = getSlots(e, out.nint, A.nint, base, n, sg);
        e = getSlots(e, out.mint, A.mint, base, n, sg);
        e = getSlots(e, out.taupath, A.taupath, base, n, sg);
        e = getSlots(e, out.tausample, A.tausample, base, n, sg);
        // (no slot stays alive, no record in use: nothing of the call is left for a kernel to find)
        if (e == hipSuccess) e = hipMemsetAsync(A.mode + base, 0, sizeof(int32_t) * size_t(size), sg);
        const hipError_t done = hipDeviceSynchronize();
        if (e == hipSuccess) e = done;
        if (e == hipSuccess) e = hipMemcpy(after, ctr, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hipFail(e, "pmc_tune_walk_cycle");
        return PMC_OK;
    }

    int runWalkCycle(pmc_ctx* ctx, const SegmentPlan& P, const pmc_walk_cycle_in& in, pmc_walk_cycle_out& out)
    {
        // (the counters of pmc_counters and pmc_walk_work as they stand: put back at the end, whichever way the call ends)
        unsigned long long before[32], after[32];
        unsigned long long* ctr = ctx->dev.counters;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(before, ctr, sizeof(before), hipMemcpyDeviceToHost));
        int rc = enqueueWalkCycle(ctx, P, in, out, after);
        // (a failure: nothing of the call may still be running when it returns, as in pmc_run_primary)
        if (rc) abandon(ctx, rc);
        ctx->timed = false;
        const hipError_t e = hipMemcpy(ctr, before, sizeof(before), hipMemcpyHostToDevice);
        if (rc) return rc;
        if (e != hipSuccess) return hipFail(e, "pmc_tune_walk_cycle");
        out.paths = after[1] - before[1], out.visits = after[2] - before[2], out.rewalks = after[6] - before[6], out.internal_errors = after[7] - before[7];
        return PMC_OK;
    }
}

extern "C" {

int pmc_tune_walk_cycle_limits(pmc_ctx* ctx, int64_t* max_slots, int32_t* live_lists, int32_t* num_instruments, int32_t* num_media)
{
    if (!ctx || !max_slots || !live_lists || !num_instruments || !num_media) return fail(PMC_ERR_INVALID, "pmc_tune_walk_cycle_limits: invalid argument");
    HIP_TRY(hipSetDevice(ctx->device));
    SegmentPlan P;
    if (int rc = planWalkCycle(ctx, P)) return rc;
    *max_slots = P.size[0];
    *live_lists = P.sparseLists ? 1 : 0;
    *num_instruments = ctx->dev.num_instruments;
    *num_media = std::max(1, ctx->dev.num_media);
    return PMC_OK;
}

int pmc_tune_walk_cycle(pmc_ctx* ctx, const pmc_walk_cycle_in* in, pmc_walk_cycle_out* out)
{
    if (!ctx || !in || !out) return fail(PMC_ERR_INVALID, "pmc_tune_walk_cycle: invalid argument");
    HIP_TRY(hipSetDevice(ctx->device));
    // (a tree grid: hints count cells in the device numbering, which has padding slots that hold no cell)
    std::vector<int32_t> cellExt;
    if (ctx->dev.cell_ext && ctx->dev.cell_slots > 0)
    {
        cellExt.resize(size_t(ctx->dev.cell_slots));
        HIP_TRY(hipMemcpy(cellExt.data(), ctx->dev.cell_ext, sizeof(int32_t) * cellExt.size(), hipMemcpyDeviceToHost));
    }
    const std::string problem = walkCycleProblem(ctx, *in, *out, cellExt);
    if (!problem.empty()) return fail(PMC_ERR_INVALID, "pmc_tune_walk_cycle: " + problem);
    SegmentPlan P;
    if (int rc = planWalkCycle(ctx, P)) return rc;
    if (in->n > P.size[0])
        return fail(PMC_ERR_INVALID, "pmc_tune_walk_cycle: " + std::to_string(in->n) + " slots, slot group 0 has " + std::to_string(P.size[0]));
    if (in->live_list && !P.sparseLists) return fail(PMC_ERR_INVALID, "pmc_tune_walk_cycle: the segment plan of this context keeps no lists of live slots");
    return runWalkCycle(ctx, P, *in, *out);
}

int pmc_launch_flavour(pmc_ctx* ctx, int32_t* flavour)
{
    if (!ctx || !flavour) return fail(PMC_ERR_INVALID, "pmc_launch_flavour: invalid argument");
    *flavour = launchFlavour(ctx);
    return PMC_OK;
}

int pmc_run_primary(pmc_ctx* ctx, uint64_t first, uint64_t count, uint64_t seed)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (count == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int numSlots = 0;
    if (int rc = provisionSlots(ctx, count, &numSlots)) return rc;
    SegmentPlan P = planSegment(ctx, numSlots, first, count, seed);
    if (int rc = provisionSortBuffers(ctx, P)) return rc;
    if (int rc = provisionLogs(ctx, P)) return rc;
    if (int rc = startSegment(ctx, P)) return rc;
    SegmentRun S{};
    if (int rc = drive(ctx, P, S)) return abandon(ctx, rc);
    // (a failure at the end leaves the segment abandoned like one in the generations)
    if (int rc = finish(ctx, P)) return abandon(ctx, rc);
    ctx->walkMs = S.walkMs;
    ctx->transitionMs = S.transMs;
    ctx->peelMs = S.peelMs;
    ctx->propMs = S.propMs;
    if (P.serialWalks && pmcTune("PMC_TIMING_DUMP"))
        fprintf(stderr, "PMC_TIMING peel %.2f ms prop %.2f ms transition+launch %.2f ms segment %.2f ms\n", S.peelMs, S.propMs, S.transMs, ctx->totalMs);
    ctx->generations = S.generations;
    ctx->timed = true;
    return checkKernelErrors(ctx);
}

}  // extern "C"
