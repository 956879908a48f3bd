// pmc_context.h -- what the translation units of the host side of libpmc.so share: the context behind a pmc_ctx handle (as a TableSink it is
// where the tables of a scene go: device memory), the launchers of pmc_kernels.hip, and the frame of a call that runs a kernel outside the
// photon loop (its device buffers, the scene refresh, the event pair, the cell records of a pass).  pmc_api.hip holds the ABI entry points of the
// context's life cycle (pmc_create: the stages of pmc_scene_build.h between the context's resources and the device-side configuration), pmc_tables.h
// the grid tables (octree flattening, binary tree, Voronoi run / cone / observer tables) and the error text of the calling thread, both plain
// host code; pmc_run.hip the generation loop (pmc_run_primary), pmc_comm.hip the RCCL calls, pmc_tuning.hip the switch table and the test aids of
// include/pmc_tuning.h, pmc_temperature.hip the dust temperatures (kernel and entry point), pmc_probe.hip the ray tracer, the ray integrator
// and the point sampler.
#ifndef PMC_CONTEXT_H
#define PMC_CONTEXT_H

#include "pmc_tables.h"
#include "../../include/pmc_layout.h"
#include "../../include/pmc_tuning.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <rccl/rccl.h>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <map>
#include <vector>

extern "C" const char* pmcTune(const char* name);
extern "C" hipError_t pmcUploadScene(int slot, const DevScene* scene, hipStream_t stream);
extern "C" hipError_t pmcConfigureKernels(size_t walkLds, size_t transitionLds);
extern "C" int pmcWalkBlocksPerCU(int gridKind, int kind, int wide, int block, size_t ldsBytes);
extern "C" hipError_t pmcLaunchStatMerge(int slot, int blocks, hipStream_t stream);
extern "C" int pmcPeelBlock(void);
extern "C" int pmcPropBlock(void);
extern "C" hipError_t pmcLaunchWalk(int slot, int gridKind, int flavour, int taskBase, int numTaskRecords, int taskCounter, uint64_t seed, int grid,
                                    int block, size_t ldsBytes, const WalkStreamArgs* tasks, hipStream_t stream);
extern "C" hipError_t pmcLaunchPeel(int slot, int form, int slotBase, int numSlots, const int* list, int cursor, int obs, int sgn, int grid, size_t ldsBytes,
                                    const PeelRec* sortedRec, const unsigned long long* sortedCount, unsigned long long* xcdCursor, hipStream_t stream);
extern "C" int pmcVoroPropWavesPerSimd(void);
extern "C" hipError_t pmcLaunchVoroProp(int slot, const int32_t* list, const unsigned long long* count, unsigned long long* xcdCursor, int segments, uint64_t seed,
                                        int flavour, int grid, hipStream_t stream);
extern "C" int pmcVoroPeelWavesPerSimd(void);
extern "C" hipError_t pmcLaunchVoroPeel(int slot, int rec, int tab, const int32_t* list, const unsigned long long* count, unsigned long long* xcdCursor, int segments,
                                        int severalMedia, int grid, hipStream_t stream);
extern "C" hipError_t pmcLaunchProp(int slot, int wide, int flavour, int checkpoints, int slotBase, int numSlots, const int* list, int cursor, uint64_t seed,
                                    int grid, size_t ldsBytes, const RfLogArgs* rfLog, hipStream_t stream);
extern "C" hipError_t pmcLaunchRfFlush(int slot, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                       int numParts, void* temp, int numCU, hipStream_t stream);
extern "C" int pmcPeelHasQueues(int form, size_t ldsBytes);
extern "C" int pmcPropHasCheckpoints(int flavour, size_t ldsBytes);
extern "C" int pmcExperimentBuild(void);
extern "C" const unsigned long long* pmcPeelSortedCount(void* temp);
extern "C" size_t pmcPeelSortTempBytes();
extern "C" hipError_t pmcLaunchPeelSortCounts(int slot, int slotBase, int numSlots, PeelSortArgs* ps, PeelRec* const* sorted, int32_t* const* lists, void* const* temp,
                                              int* groups, hipStream_t stream);
extern "C" size_t pmcRfTempBytes(int numParts);
extern "C" int pmcRfMaxParts();
extern "C" hipError_t pmcLaunchDipoleCosines(const double* u, int64_t n, double* out, hipStream_t stream);
extern "C" hipError_t pmcLaunchSourceVelocities(int slot, int source, const double* r, int64_t n, double* out, hipStream_t stream);
extern "C" hipError_t pmcLaunchDeviceFunction(int slot, int function, const double* args, int widthIn, int64_t n, double* out, int widthOut, hipStream_t stream);
extern "C" hipError_t pmcLaunchLocate(int kind, const double* nodes, int numNodes, const double* x, int64_t n, int32_t* out, hipStream_t stream);
extern "C" hipError_t pmcLaunchDetector(int slot, int instrument, const double* r, int64_t n, int32_t* pixel, int32_t* inside, hipStream_t stream);
extern "C" hipError_t pmcLaunchWavelengthBins(int slot, int instrument, const double* lambda, int64_t n, int32_t* ell, hipStream_t stream);
extern "C" hipError_t pmcLaunchAngularProbabilities(int slot, int source, const double* k, int64_t n, double* out, hipStream_t stream);
extern "C" hipError_t pmcLaunchTransition(int slot, int flavour, int slotBase, int numSlots, int group, uint64_t seed, const int* list, int listLen, int maxBlocks,
                                          size_t ldsBytes, const StatLogArgs* statLog, uint64_t count, hipStream_t stream);
extern "C" hipError_t pmcLaunchLaunch(int slot, int flavour, int slotBase, int numSlots, int group, uint64_t first, uint64_t count, uint64_t seed, int initial,
                                      int maxBlocks, size_t ldsBytes, const StatLogArgs* statLog, hipStream_t stream);
extern "C" hipError_t pmcLaunchStatFlush(int slot, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                         int numParts, void* temp, int numCU, const uint32_t* chunkFill, hipStream_t stream);
extern "C" int pmcStatBucketBits();
// test aids (include/pmc_tuning.h): the constants the log kernels are built with (the members of *out that do not depend on a context), and the
// counting sort alone (stat: the statistics log's instantiation)
extern "C" void pmcLogConstants(pmc_log_geometry_values* out);
extern "C" hipError_t pmcLaunchLogPartition(int stat, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                            int numParts, void* temp, int numCU, const uint32_t* fills, hipStream_t stream);
extern "C" hipError_t pmcLaunchCycleStart(int slot, int gridKind, int kin, int slotBase, int numSlots, int listCounter, int* listOut, const int* listIn,
                                          int listLen, int maxBlocks, size_t ldsBytes, const PeelSortArgs* sort, hipStream_t stream);
extern "C" hipError_t pmcLaunchTrace(int slot, int gridKind, int wide, int uniform, const double r[3], const double k[3],
                                     const double* kdev, int32_t* m, double* ds, int32_t cap, int32_t* n, size_t ldsBytes,
                                     hipStream_t stream);
extern "C" int pmcProbeWorkWords(void);
extern "C" hipError_t pmcLaunchIntegrate(int slot, int gridKind, int wide, int averaged, const double* origins, const double* directions, const double* q,
                                         double* sums, unsigned long long numRays, unsigned long long* work, int grid, size_t ldsBytes, hipStream_t stream);
extern "C" hipError_t pmcLaunchLocateCells(int slot, int gridKind, int wide, const double* positions, int32_t* walkCells, int32_t* cells,
                                           unsigned long long numPoints, int grid, size_t ldsBytes, hipStream_t stream);
extern "C" hipError_t pmcLaunchGatherCells(const int32_t* walkCells, const double* q, double* values, unsigned long long numPoints, int numValues, int grid,
                                           hipStream_t stream);

namespace
{
    inline int hipFail(hipError_t e, const char* what)
    {
        return fail(PMC_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }
}

#define HIP_TRY(call)                                           \
    do                                                          \
    {                                                           \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hipFail(e_, #call);        \
    } while (0)

// what comes back to the host with a generation of a slot group (pmc_run.hip), in pinned host memory
struct GroupReadback
{
    unsigned long long live;            // live slots after the generation
    unsigned long long rfLogFill;       // entries claimed in the group's radiation-field log
    unsigned long long statLogFill;     // entries claimed in the group's statistics log
    unsigned long long historyCursor;   // the segment's history cursor (progress reports)
    unsigned long long statFreeBlocks;  // free blocks of the group's share of the statistics pool
};

struct pmc_ctx final : TableSink
{
    int device{0};
    int slot{-1};
    bool sceneDirty{true};
    hipStream_t stream{nullptr};
    // slot groups: the generations of group g are enqueued on groupStream[g] (group 0 uses `stream`)
    int numGroups{3};
    hipStream_t groupStream[PMC_MAX_GROUPS]{};
    // octree: the peel-off kernels of a generation run on a side stream of the group, next to its propagation kernel
    hipStream_t peelStream[PMC_MAX_GROUPS]{};
    hipEvent_t evA[PMC_MAX_GROUPS]{}, evB[PMC_MAX_GROUPS]{}, evC[PMC_MAX_GROUPS]{}, evJoin[PMC_MAX_GROUPS]{}, evProp[PMC_MAX_GROUPS]{};
    hipEvent_t evStart{nullptr}, evStop{nullptr};
    bool timed{false};
    float totalMs{0}, walkMs{0}, transitionMs{0};
    float peelMs{0}, propMs{0};  // octree: the spans of the peel-off kernels and of the propagation kernel, summed over the generations
    int generations{0};
    // work of the most recent pmc_integrate_rays (pmc_last_integrate_work)
    float integrateMs{0};
    unsigned long long integrateLaneSteps{0}, integrateWaveSteps{0};
    float temperatureMs{0};  // kernel of the most recent pmc_dust_temperatures (pmc_last_temperature_ms)
    float sampleMs{0};       // kernels of the most recent pmc_sample_cells (pmc_last_sample_ms)
    DevScene dev{};
    std::vector<void*> allocations;
    std::vector<void*> slotAllocations;
    double* frames{nullptr};
    int64_t frameSize{0};
    int64_t rfSize{0};  // doubles of the radiation field table (0: not stored)
    size_t walkLds{0}, transitionLds{0}, launchLds{0};
    int block{256};
    int grid{0};          // workgroups of the generic walk kernel / the octree propagation kernel
    int peelGrid{0};      // workgroups of an octree peel-off kernel
    int wide{0};          // octree deeper than level 10: 21-bit index fields (pmc_walk_tree.inc Pack)
    int numCU{256};
    int64_t numSlots{0};         // requested pool size
    int64_t allocatedSlots{0};   // size of the allocated slot arrays
    GroupReadback* readback{nullptr};  // [PMC_MAX_GROUPS]
    unsigned long long internalErrorsSeen{0};
    pmc_progress_fn progress{nullptr};    // pmc_set_progress
    void* progressUser{nullptr};
    double progressInterval{3.};
    size_t steppedDownFree{0};            // free device memory when the default pool last stepped down (0: it has not)
    bool slotsConfigured{false};          // the number of slots was set explicitly (PMC_NUM_SLOTS, pmc_set_num_slots)
    bool groupsConfigured{false};         // the number of slot groups was set explicitly (PMC_NUM_GROUPS)
    unsigned long long overflowsSeen{0};  // statistics-list overflows already reported (pmc_run_primary)
    int32_t* statPoolIota{nullptr};       // 0, 1, 2, ...: the free list of a statistics pool none of whose blocks is in use
    int64_t statPoolBlocks{0};
    int statPoolGrowths{0};               // times the pool has grown (pmc_run_primary)
    // every buffer that pmc_run_primary provisions per segment (sort buffers, logs, cursors): kept from one segment to the next, grown when needed
    std::vector<void*> segmentAllocations;
    // radiation field on an octree: per slot group the log of a generation's contributions (two buffers each for the
    // partitioning sort) and the sort's temporary storage
    uint32_t* rfKeys[PMC_MAX_GROUPS][2]{};
    double* rfVals[PMC_MAX_GROUPS][2]{};
    unsigned long long rfCap[PMC_MAX_GROUPS]{};
    void* rfTemp[PMC_MAX_GROUPS]{};
    // sorted peel-off records (pmc_device.h PeelRec): per group the records in slot order and in tile order, the keys, the sort's counters
    PeelRec* peelRec[PMC_MAX_GROUPS][PMC_SORT_OBS]{};  // per group and sorted observer (octree)
    int32_t* peelList[PMC_MAX_GROUPS][PMC_SORT_OBS]{};  // (Cartesian, Voronoi) the slots in tile order instead
    void* peelTemp[PMC_MAX_GROUPS][PMC_SORT_OBS]{};
    unsigned long long* xcdCursors{nullptr};  // [PMC_MAX_GROUPS][PMC_SORT_OBS + 1][8] (+ 8 that stay zero) the walk kernels' cursors over the eighths of their sorted records / lists
    int peelCap[PMC_MAX_GROUPS]{};
    size_t rfTempBytes{0};
    // statistics log per slot group (pmc_device.h StatLogArgs): the log and its partitioned copy, the sort's counters
    uint32_t* statKeys[PMC_MAX_GROUPS][2]{};
    double* statVals[PMC_MAX_GROUPS][2]{};
    unsigned long long statCap[PMC_MAX_GROUPS]{};
    void* statTemp[PMC_MAX_GROUPS]{};
    unsigned long long* statWaveBase[PMC_MAX_GROUPS]{};
    uint32_t* statWaveFill[PMC_MAX_GROUPS]{};
    uint32_t* statChunkFill[PMC_MAX_GROUPS]{};

    // TableSink (upload<T>, the tables of pmc_create): device memory that lives as long as the context
    int uploadBytes(const void* host, size_t elementBytes, size_t count, const void** out) override
    {
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, count * elementBytes);
        if (e != hipSuccess) return hipFail(e, "hipMalloc");
        allocations.push_back(d);
        e = hipMemcpy(d, host, count * elementBytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "hipMemcpy");
        *out = d;
        return PMC_OK;
    }
    int allocateBytes(size_t bytes, void** out, bool zero) override
    {
        unsigned char* d = nullptr;
        const int rc = allocate(bytes, &d, zero);
        *out = d;
        return rc;
    }
    // (a device that does not say: plenty)
    size_t freeBytes() override
    {
        size_t freeNow = 0, total = 0;
        return hipMemGetInfo(&freeNow, &total) == hipSuccess ? freeNow : ~size_t(0);
    }
    // (planning pass of allocateSlots: the requests are only added up)
    bool planning{false};
    size_t plannedBytes{0};

    template<typename T> int allocate(size_t count, T** out, bool zero, std::vector<void*>* owner = nullptr)
    {
        *out = nullptr;
        if (!count) return PMC_OK;
        if (planning)
        {
            plannedBytes += (count * sizeof(T) + 255) & ~size_t(255);
            return PMC_OK;
        }
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, count * sizeof(T));
        if (e != hipSuccess) return hipFail(e, "hipMalloc");
        (owner ? *owner : allocations).push_back(d);
        if (zero)
        {
            e = hipMemset(d, 0, count * sizeof(T));
            if (e != hipSuccess) return hipFail(e, "hipMemset");
        }
        else if (pmcTune("PMC_POISON_ALLOCATIONS"))
        {
            // (test aid: what the engine does not initialise holds neither zeros -- fresh device memory -- nor plausible values -- memory of a
            // context destroyed before: a read of it shows)
            e = hipMemset(d, 0xA5, count * sizeof(T));
            if (e != hipSuccess) return hipFail(e, "hipMemset");
        }
        *out = static_cast<T*>(d);
        return PMC_OK;
    }
    // frees a buffer of `owner` (as in allocate) and forgets it
    template<typename T> void release(T*& p, std::vector<void*>* owner = nullptr)
    {
        if (!p) return;
        void* d = const_cast<void*>(static_cast<const void*>(p));
        std::vector<void*>& own = owner ? *owner : allocations;
        own.erase(std::remove(own.begin(), own.end(), d), own.end());
        hipFree(d);
        p = nullptr;
    }
};

// device buffers of one call (pmc_trace_ray, pmc_integrate_rays, pmc_sample_cells, pmc_dust_temperatures): freed when the call returns, whichever way
struct CallBuffers
{
    std::vector<void*> owned;
    ~CallBuffers()
    {
        for (void* d : owned) hipFree(d);
    }
    // room for `count` elements, filled from `host` if there is one
    template<typename T> hipError_t get(size_t count, T** out, const T* host = nullptr)
    {
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, std::max(count, size_t(1)) * sizeof(T));
        if (e != hipSuccess) return e;
        owned.push_back(d);
        *out = static_cast<T*>(d);
        if (host) return hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
        // (test aid, as in pmc_ctx::allocate: what the call does not write shows)
        if (pmcTune("PMC_POISON_ALLOCATIONS")) return hipMemset(d, 0xA5, std::max(count, size_t(1)) * sizeof(T));
        return hipSuccess;
    }
};

// ---- the frame of a call that runs a kernel outside the photon loop (pmc_probe.hip, pmc_temperature.hip, the test aids of pmc_tuning.hip)

// the scene in constant memory, brought up to date after whatever ctx->stream still runs (pmc_run_primary calls it per segment too)
inline hipError_t sceneUpToDate(pmc_ctx* ctx)
{
    if (!ctx->sceneDirty) return hipSuccess;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream);
    if (e == hipSuccess) ctx->sceneDirty = false;
    return e;
}

// the two HIP events around the kernels of a call: destroyed when the call returns, whichever way
struct EventPair
{
    hipEvent_t a{nullptr}, b{nullptr};
    ~EventPair()
    {
        if (a) hipEventDestroy(a);
        if (b) hipEventDestroy(b);
    }
    int create()
    {
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        return PMC_OK;
    }
    hipError_t start(hipStream_t stream) { return hipEventRecord(a, stream); }
    hipError_t stop(hipStream_t stream) { return hipEventRecord(b, stream); }
    // between start and stop, once the stream has been synchronised (0 where the runtime does not say)
    float elapsedMs() const
    {
        float ms = 0.f;
        return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
    }
};

// persistent waves: enough workgroups of four waves for every CU's share (the probe kernels stage the grid tables per workgroup), no more than
// the items fill
inline int persistentGrid(const pmc_ctx* ctx, size_t items)
{
    return int(std::max<size_t>(1, std::min<size_t>((items + 255) / 256, size_t(ctx->numCU) * 4)));
}

// the caller's cell values as the probe kernels gather them: per pass one record [slot][PMC_INTEGRATE_PASS_VALUES] in the numbering the kernels
// walk in -- device cells of a tree (cell_ext[device cell] = the caller's m, -1: none), else the caller's
struct CellRecords
{
    static constexpr int W = PMC_INTEGRATE_PASS_VALUES;
    bool renumbered{false};
    size_t numCells{0}, slots{0};
    std::vector<int32_t> ext;

    // `values`: the call has cell values to renumber (a tree's cell_ext is downloaded and checked)
    int prepare(const DevScene& D, const std::string& name, bool values)
    {
        numCells = size_t(D.num_cells);
        renumbered = D.grid_kind == PMC_GRID_OCTREE || D.grid_kind == PMC_GRID_BINTREE;
        slots = renumbered ? size_t(D.cell_slots) : numCells;
        if (!renumbered || !values) return PMC_OK;
        ext.resize(slots);
        HIP_TRY(hipMemcpy(ext.data(), D.cell_ext, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t m : ext)
            if (m >= D.num_cells) return fail(PMC_ERR_DEVICE, name + ": cell numbering table out of range");
        return PMC_OK;
    }
    // the record [slots][W] of pass `pass`: the cell's weight, where there are weights, and the next W (with weights W - 1) of the num_values
    // rows of cell_values [.][numCells]; zero where a slot has no cell and past the last value
    void build(double* record, int pass, int num_values, const double* cell_weights, const double* cell_values) const
    {
        const int lead = cell_weights ? 1 : 0, perPass = W - lead;
        const int v0 = pass * perPass, nv = std::min(perPass, num_values - v0);
        for (size_t c = 0; c < slots; ++c)
        {
            const int64_t m = renumbered ? int64_t(ext[c]) : int64_t(c);
            if (cell_weights) record[c * W] = m >= 0 ? cell_weights[size_t(m)] : 0.;
            for (int j = 0; j < perPass; ++j) record[c * W + lead + j] = (j < nv && m >= 0) ? cell_values[size_t(v0 + j) * numCells + size_t(m)] : 0.;
        }
    }
};

// pmc_run.hip: the pool of packet slots
int pmcAllocateSlots(pmc_ctx* ctx, int64_t n);

// pmc_run.hip: which of the context's sums go through a log, and in how many partitions (the segment plan of pmc_run_primary and
// pmc_tune_log_geometry; the switches PMC_RF_ATOMICS and PMC_STAT_ATOMICS are sampled here)
struct LogPlan
{
    int64_t rfKeys, rfParts;  // keys of the radiation-field log (cells counted in the device numbering on an octree, padding included), partitions
    bool rfLogged;
    int64_t statRecords, statParts;
    bool statLogged;
};
LogPlan pmcLogPlan(const pmc_ctx* ctx);

#endif
