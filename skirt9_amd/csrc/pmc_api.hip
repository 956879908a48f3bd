// pmc_api.hip -- the extern "C" ABI of include/pmc.h: context life time (pmc_create: the context's resources, the tuning switches of scene
// creation, the device-side configuration -- LDS limits, launch geometry, slot count), frames, radiation field, counters, the single-ray tracer
// and the ray integrator.  What pmc_create makes of the scene -- validation, DevScene, every table -- is the plain host code of
// pmc_scene_build.h and pmc_tables.h, which writes through the context as its TableSink; the generation loop (pmc_run_primary) lives in
// pmc_run.hip, the RCCL calls in pmc_comm.hip, the switch table of include/pmc_tuning.h in pmc_tuning.hip; pmc_context.h is what they share.
#include "pmc_context.h"
#include "pmc_scene_build.h"
#include <memory>

namespace
{
    thread_local std::string t_error;
    // constant-memory scene slots (pmc_kernels.hip c_scene): every device has its own copy of the symbol, so the table
    // of live contexts is per device; guarded, because contexts may be created from one host thread per GPU
    constexpr int MAX_DEVICES = 64;
    bool g_slotUsed[MAX_DEVICES][PMC_MAX_CONTEXTS] = {{false}};
    std::mutex g_slotMutex;
}

// error text of the calling thread, for the other translation units of the library (pmc_sampler.hip)
void pmcSetError(const std::string& message)
{
    t_error = message;
}


extern "C" {

int pmc_abi_version(void)
{
    return PMC_ABI_VERSION;
}

// what this binary was built with (the Makefile hands its HIPFLAGS over): results are bit-compatible with the reference only under
// -ffp-contract=off (the reference build has no fused multiply-add), and the detector atomics are hardware f64 adds
// only under -munsafe-fp-atomics
#define PMC_STRINGIFY2(x) #x
#define PMC_STRINGIFY(x) PMC_STRINGIFY2(x)
#ifndef PMC_BUILD_FLAGS
#define PMC_BUILD_FLAGS "unknown (not built by the Makefile)"
#endif
const char* pmc_build_info(void)
{
    return "libpmc ABI " PMC_STRINGIFY(PMC_ABI_VERSION) ", gfx950, " __VERSION__ ", flags: " PMC_BUILD_FLAGS
#if defined(__FP_FAST_FMA) || defined(__FAST_MATH__)
           " [fast-math macros defined]"
#endif
        ;
}

namespace
{
    // a * b + c with run-time operands: 0 when the product is rounded before the sum (-ffp-contract=off), -2^-60 when the compiler fused the two
    __global__ void contractionProbeKernel(double a, double b, double c, double* out) { out[0] = a * b + c; }

    // one launch per process and device, at the first pmc_create: a binary whose compiler contracted a * b + c computes other last bits than
    // the reference in every optical depth and exit distance, silently; it is refused instead
    int checkContraction(int device)
    {
        static std::mutex m;
        static bool checked[64] = {false};
        std::lock_guard<std::mutex> lock(m);
        if (device >= 0 && device < 64 && checked[device]) return PMC_OK;
        double* d = nullptr;
        double h = 1.;
        if (hipMalloc(&d, sizeof(double)) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipMalloc failed");
        hipLaunchKernelGGL(contractionProbeKernel, dim3(1), dim3(1), 0, 0, 1. + 0x1p-30, 1. - 0x1p-30, -1., d);
        const hipError_t e = hipMemcpy(&h, d, sizeof(double), hipMemcpyDeviceToHost);
        hipFree(d);
        if (e != hipSuccess) return hipFail(e, "contraction self-test");
        if (h != 0.)
            return fail(PMC_ERR_DEVICE, std::string("this libpmc.so was compiled with floating-point contraction (a * b + c fused): its results would differ from "
                                                    "the reference's in the last bits everywhere; rebuild with -ffp-contract=off.  ") + pmc_build_info());
        if (device >= 0 && device < 64) checked[device] = true;
        return PMC_OK;
    }
}

const char* pmc_last_error(void)
{
    return t_error.c_str();
}

int64_t pmc_frame_layout_of(const pmc_scene* scene, int32_t instrument, pmc_frame_layout* out)
{
    if (!scene) return fail(PMC_ERR_INVALID, "null scene");
    return pmc_layout_compute(scene, instrument, out);
}

void pmc_destroy(pmc_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    for (int g = 0; g < PMC_MAX_GROUPS; ++g)
    {
        if (ctx->groupStream[g]) hipStreamSynchronize(ctx->groupStream[g]);
        if (ctx->peelStream[g]) hipStreamSynchronize(ctx->peelStream[g]);
    }
    for (void* p : ctx->allocations) hipFree(p);
    for (void* p : ctx->slotAllocations) hipFree(p);
    for (void* p : ctx->segmentAllocations) hipFree(p);
    if (ctx->readback) hipHostFree(ctx->readback);
    for (hipEvent_t e : {ctx->evStart, ctx->evStop})
        if (e) hipEventDestroy(e);
    for (int g = 0; g < PMC_MAX_GROUPS; ++g)
    {
        for (hipEvent_t e : {ctx->evA[g], ctx->evB[g], ctx->evC[g], ctx->evJoin[g], ctx->evProp[g]})
            if (e) hipEventDestroy(e);
        if (g > 0 && ctx->groupStream[g]) hipStreamDestroy(ctx->groupStream[g]);
        if (ctx->peelStream[g]) hipStreamDestroy(ctx->peelStream[g]);
    }
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->slot >= 0)
    {
        std::lock_guard<std::mutex> lock(g_slotMutex);
        g_slotUsed[ctx->device][ctx->slot] = false;
    }
    delete ctx;
}

}  // extern "C"

// ---- pmc_create: checkScene | context resources | the tables of pmc_scene_build.h, with the context as their sink | device-side configuration
namespace
{
    // the switches that scene creation reads (SceneSwitches, pmc_tables.h), once
    SceneSwitches readSceneSwitches()
    {
        SceneSwitches sw;
        sw.treeAsBinTree = pmcTune("PMC_TREE_AS_BINTREE") != nullptr;
        sw.noMono = pmcTune("PMC_NO_MONO") != nullptr;
        sw.propNoCheckpoints = pmcTune("PMC_PROP_NO_CHECKPOINTS") != nullptr;
        sw.voroNoPeelKernel = pmcTune("PMC_VORO_NO_PEEL_KERNEL") != nullptr;
        sw.voroNoDeferredScan = pmcTune("PMC_VORO_NO_DEFERRED_SCAN") != nullptr;
        sw.voroNoCull = pmcTune("PMC_VORO_NO_CULL") != nullptr;
        sw.voroNoPropKernel = pmcTune("PMC_VORO_NO_PROP_KERNEL") != nullptr;
        sw.voroNoConeTables = pmcTune("PMC_VORO_NO_CONE_TABLES") != nullptr;
        sw.voroNoObserverLists = pmcTune("PMC_VORO_NO_OBSERVER_LISTS") != nullptr;
        sw.voroConeCullOnly = pmcTune("PMC_VORO_CONE_CULL_ONLY") != nullptr;
        // (cells with more entries than a link can name say so in their header; the switch lowers the limit: a test of that path)
        if (const char* v = pmcTune("PMC_VORO_LINK_COUNT_MAX")) sw.voroLinkCountMax = std::min<uint32_t>(sw.voroLinkCountMax, (uint32_t)std::max(0, atoi(v)));
        if (const char* v = pmcTune("PMC_CELL_ORDER")) sw.cellOrderRef = !strcmp(v, "ref");
        if (const char* v = pmcTune("PMC_CELL_SHUFFLE")) sw.cellShuffle = atoi(v);
        if (const char* v = pmcTune("PMC_WALK_BLOCKS_PER_CU")) sw.walkBlocksPerCU = std::max(1, atoi(v));
        if (const char* v = pmcTune("PMC_PEEL_BLOCKS_PER_CU")) sw.peelBlocksPerCU = std::max(1, atoi(v));
        return sw;
    }

    struct DestroyContext
    {
        void operator()(pmc_ctx* ctx) const { pmc_destroy(ctx); }
    };
    using ContextPtr = std::unique_ptr<pmc_ctx, DestroyContext>;

    // a context on `device` with its slot in the per-device table, streams, events and pinned readback
    int makeContext(int device, ContextPtr& made)
    {
        if (device >= MAX_DEVICES) return fail(PMC_ERR_UNSUPPORTED, "device index beyond the context table");
        ContextPtr ctx(new pmc_ctx());
        ctx->device = device;
        {
            std::lock_guard<std::mutex> lock(g_slotMutex);
            for (int sl = 0; sl < PMC_MAX_CONTEXTS && ctx->slot < 0; ++sl)
                if (!g_slotUsed[device][sl])
                {
                    g_slotUsed[device][sl] = true;
                    ctx->slot = sl;
                }
        }
        if (ctx->slot < 0) return fail(PMC_ERR_NOMEM, "too many live pmc contexts (at most " + std::to_string(PMC_MAX_CONTEXTS) + ")");
        auto makeStream = [](hipStream_t* out) { return hipStreamCreateWithPriority(out, hipStreamDefault, 0); };
        if (makeStream(&ctx->stream) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        ctx->groupStream[0] = ctx->stream;
        for (int g = 1; g < PMC_MAX_GROUPS; ++g)
            if (makeStream(&ctx->groupStream[g]) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        for (int g = 0; g < PMC_MAX_GROUPS; ++g)
            if (makeStream(&ctx->peelStream[g]) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        for (hipEvent_t* ev : {&ctx->evStart, &ctx->evStop})
            if (hipEventCreate(ev) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipEventCreate failed");
        for (int g = 0; g < PMC_MAX_GROUPS; ++g)
            for (hipEvent_t* ev : {&ctx->evA[g], &ctx->evB[g], &ctx->evC[g], &ctx->evJoin[g], &ctx->evProp[g]})
                if (hipEventCreate(ev) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipEventCreate failed");
        if (const char* env = getenv("PMC_NUM_GROUPS"))
        {
            ctx->numGroups = std::min(PMC_MAX_GROUPS, std::max(1, atoi(env)));
            ctx->groupsConfigured = true;  // (an explicit setting: also a Voronoi scene runs with it)
        }
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->readback), PMC_MAX_GROUPS * sizeof(GroupReadback)) != hipSuccess)
            return fail(PMC_ERR_DEVICE, "hipHostMalloc failed");
        made = std::move(ctx);
        return PMC_OK;
    }

    // what the device decides: the kernels' LDS limits, the launch geometry of the persistent walk kernels, the number of packet slots
    int configureDevice(pmc_ctx* ctx, const SceneSwitches& sw)
    {
        const DevScene& D = ctx->dev;
        if (pmcConfigureKernels(ctx->walkLds, ctx->launchLds) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipFuncSetAttribute failed");
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipGetDeviceProperties failed");
        ctx->numCU = prop.multiProcessorCount;
        ctx->block = 256;
        ctx->wide = D.grid_kind == PMC_GRID_OCTREE && D.lmax > 10;
        // persistent walk kernels: as many workgroups as stay resident (the transition / launch kernels of the other
        // slot group get the CUs between generations)
        int perCU = pmcWalkBlocksPerCU(D.grid_kind, D.grid_kind == PMC_GRID_OCTREE ? 2 : 0, ctx->wide,
                                       D.grid_kind == PMC_GRID_OCTREE ? pmcPropBlock() : ctx->block, ctx->walkLds);
        if (perCU < 1) perCU = 1;
        // (octree propagation kernel: ONE workgroup of 256 lanes per CU.  The walk kernels are bound by the memory system's
        // rate of random gathers, which falls when too many of them are in flight -- 32 MB table, 8 / 16 / 32 waves per CU:
        // 1.9 / 0.94 / 0.83e11 records/s, profiles/microbench/gather_modes_mi355x.txt -- and the kernels of three slot groups
        // overlap; 1 / 2 / 3 per CU: 697 / 720 / 756 ms per 1e8 packets)
        if (sw.walkBlocksPerCU) perCU = std::min(perCU, sw.walkBlocksPerCU);  // tuning aid
        else perCU = std::min(perCU, D.grid_kind == PMC_GRID_OCTREE ? 1 : 3);
        ctx->grid = ctx->numCU * perCU;
        if (D.grid_kind == PMC_GRID_OCTREE)
        {
            int peelPerCU = pmcWalkBlocksPerCU(D.grid_kind, 1, ctx->wide, pmcPeelBlock(), ctx->walkLds);
            // (one workgroup of 512 lanes per CU: with the pipelined step more resident waves only queue up in the memory
            // system -- 1 / 2 / 3 per CU: 97 / 111 / 124 ms per 5e7 packets, profiles/README.md)
            peelPerCU = std::min(std::max(peelPerCU, 1), 1);
            if (sw.peelBlocksPerCU) peelPerCU = sw.peelBlocksPerCU;
            ctx->peelGrid = ctx->numCU * peelPerCU;
        }
        // packet slots: 24 Mi histories in flight (about 1.7 KB of state per slot with one statistics-recording instrument: 40 GB of the 288).  A
        // segment of 1e8 packets then runs 83 generations instead of the 177 of 8 Mi slots -- fewer launches, fewer ragged kernel tails -- and gains
        // 3-7 % (8 / 12 / 16 / 24 / 32 Mi: 2.00 / 2.05 / 2.05 / 2.07 / 2.07e8 packets/s, profiles/sweeps/r05_d3_slots.txt)
        ctx->numSlots = 24 * 1024 * 1024;
        if (const char* env = getenv("PMC_NUM_SLOTS"))
        {
            ctx->numSlots = std::max<int64_t>(1024, atoll(env));
            ctx->slotsConfigured = true;
        }
        return PMC_OK;
    }
}

extern "C" {

int pmc_create(const pmc_scene* scene, int32_t device, pmc_ctx** out)
{
    return pmc_create_ext(scene, nullptr, device, out);
}

int pmc_create_ext(const pmc_scene* scene, const pmc_scene_ext* ext, int32_t device, pmc_ctx** out)
{
    if (!scene || !out) return fail(PMC_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = PMC_OK;
    SceneExtension extension;
    if ((rc = checkScene(*scene, ext, extension))) return rc;
    if (pmcExperimentBuild())
    {
        static std::atomic<bool> said{false};
        if (!said.exchange(true)) fprintf(stderr, "libpmc: this library was built with an ablation / perturbation macro (a tuning experiment): its results are NOT those of the engine\n");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return fail(PMC_ERR_DEVICE, "no HIP device available: the MI355X engine cannot run (there is no CPU fallback)");
    if (device < 0 || device >= count) return fail(PMC_ERR_INVALID, "invalid device index");
    HIP_TRY(hipSetDevice(device));
    if ((rc = checkContraction(device))) return rc;

    ContextPtr ctx;  // (destroyed with everything it holds by then, unless it is handed out)
    if ((rc = makeContext(device, ctx))) return rc;
    const SceneSwitches switches = readSceneSwitches();
    SceneTables tables;
    if ((rc = buildSceneTables(*scene, extension, switches, *ctx, ctx->dev, tables))) return rc;
    ctx->frameSize = tables.frameSize;
    ctx->rfSize = tables.rfSize;
    ctx->frames = ctx->dev.frames;
    ctx->walkLds = tables.lds.walkBytes, ctx->transitionLds = tables.lds.transitionBytes, ctx->launchLds = tables.lds.launchBytes;
    if ((rc = configureDevice(ctx.get(), switches))) return rc;
    *out = ctx.release();
    return PMC_OK;
}

int pmc_set_launch(pmc_ctx* ctx, int32_t block, int32_t grid)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (block > 0)
    {
        if (block % 64 || block > 256) return fail(PMC_ERR_INVALID, "block must be a multiple of 64 and at most 256");
        ctx->block = block;
    }
    if (grid > 0) ctx->grid = grid;
    return PMC_OK;
}

int pmc_set_num_slots(pmc_ctx* ctx, int64_t num_slots)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (num_slots < 1 || num_slots > (int64_t(1) << 30)) return fail(PMC_ERR_INVALID, "num_slots out of range");
    ctx->numSlots = num_slots;
    ctx->slotsConfigured = true;
    return PMC_OK;
}

int pmc_bind_frames(pmc_ctx* ctx, double* device_ptr, int64_t num_doubles)
{
    if (!ctx || !device_ptr) return fail(PMC_ERR_INVALID, "null argument");
    if (num_doubles != ctx->frameSize) return fail(PMC_ERR_INVALID, "frame buffer size mismatch");
    ctx->frames = device_ptr;
    ctx->dev.frames = device_ptr;
    ctx->sceneDirty = true;
    return PMC_OK;
}

int pmc_clear_frames(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->frames, 0, size_t(ctx->frameSize) * sizeof(double), ctx->stream));
    return PMC_OK;
}

int pmc_set_progress(pmc_ctx* ctx, pmc_progress_fn report, void* user, double interval_seconds)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    ctx->progress = report;
    ctx->progressUser = user;
    ctx->progressInterval = interval_seconds > 0. ? interval_seconds : 0.;
    return PMC_OK;
}

int pmc_sync(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PMC_OK;
}

int pmc_last_kernel_ms(pmc_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    *ms = ctx->walkMs;
    return PMC_OK;
}

int pmc_last_timing(pmc_ctx* ctx, float* total_ms, float* walk_ms, float* transition_ms, int32_t* generations)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    if (total_ms) *total_ms = ctx->totalMs;
    if (walk_ms) *walk_ms = ctx->walkMs;
    if (transition_ms) *transition_ms = ctx->transitionMs;
    if (generations) *generations = ctx->generations;
    return PMC_OK;
}

int pmc_last_walk_timing(pmc_ctx* ctx, float* peel_ms, float* prop_ms)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    if (peel_ms) *peel_ms = ctx->peelMs;
    if (prop_ms) *prop_ms = ctx->propMs;
    return PMC_OK;
}

int pmc_walk_work(pmc_ctx* ctx, pmc_walk_work_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long host[6];
    HIP_TRY(hipMemcpy(host, ctx->dev.counters + PMC_CTR_WALKWORK, sizeof(host), hipMemcpyDeviceToHost));
    out->peel_wave_steps = host[0], out->peel_lane_steps = host[1], out->peel_rounds = host[2];
    out->prop_wave_steps = host[3], out->prop_lane_steps = host[4], out->prop_rounds = host[5];
    return PMC_OK;
}

int pmc_debug_tables(pmc_ctx* ctx, pmc_debug_table_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    if (ctx->dev.grid_kind != PMC_GRID_OCTREE) return fail(PMC_ERR_INVALID, "not an octree scene");
    out->cell_table = ctx->dev.cell_tab;
    out->cell_slots = ctx->dev.cell_slots;
    out->loose_base = ctx->dev.cell_slots;
    out->task_cell = ctx->dev.tasks.cell;
    out->num_slots = ctx->allocatedSlots;
    return PMC_OK;
}

int pmc_download(pmc_ctx* ctx, double* host_frames, int64_t num_doubles)
{
    if (!ctx || !host_frames) return fail(PMC_ERR_INVALID, "null argument");
    if (num_doubles != ctx->frameSize) return fail(PMC_ERR_INVALID, "frame buffer size mismatch");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(host_frames, ctx->frames, size_t(num_doubles) * sizeof(double), hipMemcpyDeviceToHost));
    return PMC_OK;
}

double* pmc_frames_device(pmc_ctx* ctx)
{
    return ctx ? ctx->frames : nullptr;
}

int64_t pmc_frames_size(pmc_ctx* ctx)
{
    return ctx ? ctx->frameSize : 0;
}

int64_t pmc_radiation_field_size(pmc_ctx* ctx)
{
    return ctx ? ctx->rfSize : 0;
}

double* pmc_radiation_field_device(pmc_ctx* ctx)
{
    return ctx ? ctx->dev.rf : nullptr;
}

int pmc_bind_radiation_field(pmc_ctx* ctx, double* device_ptr, int64_t num_doubles)
{
    if (!ctx || !device_ptr) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->rfSize) return fail(PMC_ERR_INVALID, "the scene does not store the radiation field");
    if (num_doubles != ctx->rfSize) return fail(PMC_ERR_INVALID, "radiation field size mismatch");
    ctx->dev.rf = device_ptr;
    ctx->sceneDirty = true;
    return PMC_OK;
}

int pmc_download_radiation_field(pmc_ctx* ctx, double* host_rf, int64_t num_doubles)
{
    if (!ctx || !host_rf) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->rfSize) return fail(PMC_ERR_INVALID, "the scene does not store the radiation field");
    if (num_doubles != ctx->rfSize) return fail(PMC_ERR_INVALID, "radiation field size mismatch");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(host_rf, ctx->dev.rf, size_t(num_doubles) * sizeof(double), hipMemcpyDeviceToHost));
    return PMC_OK;
}

int pmc_clear_radiation_field(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (!ctx->rfSize) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->dev.rf, 0, size_t(ctx->rfSize) * sizeof(double), ctx->stream));
    return PMC_OK;
}

int pmc_counters(pmc_ctx* ctx, pmc_counter_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long host[PMC_NUM_COUNTERS];
    HIP_TRY(hipMemcpy(host, ctx->dev.counters, sizeof(host), hipMemcpyDeviceToHost));
    out->histories = host[0];
    out->paths = host[1];
    out->cell_visits = host[2];
    out->detector_updates = host[3];
    out->scatterings = host[4];
    out->stat_overflows = host[5];
    out->rewalk_visits = host[6];
    if (pmcTune("PMC_PROFILE_DUMP"))
    {
        // work counters of the octree walk kernels: lane utilisation = lane_steps / (64 wave_steps)
        const unsigned long long* w = host + PMC_CTR_WALKWORK;
        fprintf(stderr, "PMC_PROFILE peel: wave_steps %llu lane_steps %llu (%.1f %% of the lanes) service_rounds %llu\n", w[0], w[1],
                w[0] ? 100. * double(w[1]) / (64. * double(w[0])) : 0., w[2]);
        fprintf(stderr, "PMC_PROFILE prop: wave_steps %llu lane_steps %llu (%.1f %% of the lanes) service_rounds %llu\n", w[3], w[4],
                w[3] ? 100. * double(w[4]) / (64. * double(w[3])) : 0., w[5]);
    }
#ifdef PMC_PROFILE
    if (pmcTune("PMC_PROFILE_DUMP"))
    {
        for (int k = 0; k < 2; ++k)
        {
            const unsigned long long* t = host + 208 + 8 * k;
            fprintf(stderr, "PMC_PROFILE %s phases (wave cycles): gather %llu tau+position %llu descent %llu walls %llu inside+exit %llu "
                            "service-finish+claim %llu service-loads %llu loop %llu\n", k ? "prop" : "peel", t[0], t[1], t[2], t[3], t[4], t[5],
                    t[6], t[7]);
        }
        for (int k = 0; k < 2; ++k)
        {
            const unsigned long long* c = host + 224 + 8 * k;
            fprintf(stderr, "PMC_PROFILE %s census (lane events): literal-algorithm steps %llu, edge %llu, descents %llu over %llu levels, octet links %llu, "
                            "hit %llu, exit %llu\n", k ? "prop" : "peel", c[0], c[2], c[3], c[4], c[5], c[6], c[7]);
        }
        fprintf(stderr, "PMC_PROFILE transition (wave cycles): stage %llu mode-load %llu cycle-tail %llu append %llu loads+detect %llu scatter %llu start-cycle %llu flush %llu\n",
                host[192], host[193], host[194], host[195], host[196], host[197], host[198], host[199]);
        fprintf(stderr, "PMC_PROFILE launch (wave cycles): stage %llu list %llu stats-flush %llu start-cycle %llu draw+sample %llu - %llu flush %llu\n",
                host[200], host[201], host[202], host[203], host[204], host[205], host[206]);
    }
#endif
    return PMC_OK;
}

int pmc_reset_counters(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->dev.counters, 0, PMC_NUM_COUNTERS * sizeof(unsigned long long), ctx->stream));
    ctx->overflowsSeen = 0;
    ctx->internalErrorsSeen = 0;
    return PMC_OK;
}

int pmc_trace_ray(pmc_ctx* ctx, const double r[3], const double k[3], int32_t* m, double* ds, int32_t cap, int32_t* n)
{
    if (!ctx || !r || !k || !m || !ds || !n || cap < 0) return fail(PMC_ERR_INVALID, "invalid argument");
    HIP_TRY(hipSetDevice(ctx->device));
    // octree: the ray is traced with BOTH flavours of the step (direction in scalar registers as in the peel-off kernel,
    // in vector registers as in the propagation kernel); they must agree bit for bit
    const int flavours = ctx->dev.grid_kind == PMC_GRID_OCTREE ? 2 : 1;
    const size_t room = size_t(std::max(cap, 1));
    int32_t* dm = nullptr;
    double* dds = nullptr;
    int32_t* dn = nullptr;
    double* dk = nullptr;
    CallBuffers scratch;
    HIP_TRY(scratch.get(room * flavours, &dm));
    HIP_TRY(scratch.get(room * flavours, &dds));
    HIP_TRY(scratch.get(size_t(flavours), &dn));
    HIP_TRY(scratch.get(size_t(3), &dk));
    hipError_t e = hipMemcpy(dk, k, 3 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && ctx->sceneDirty)
    {
        e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream);
        if (e == hipSuccess) ctx->sceneDirty = false;
    }
    for (int f = 0; f < flavours && e == hipSuccess; ++f)
        e = pmcLaunchTrace(ctx->slot, ctx->dev.grid_kind, ctx->wide, f, r, k, dk, dm + f * room, dds + f * room, cap, dn + f, ctx->walkLds,
                           ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    int rc = PMC_OK;
    if (e != hipSuccess)
        rc = hipFail(e, "trace kernel");
    else
    {
        int32_t count[2] = {0, 0};
        hipMemcpy(count, dn, sizeof(int32_t) * flavours, hipMemcpyDeviceToHost);
        *n = count[0];
        const int32_t got = std::min(*n, cap);
        hipMemcpy(m, dm, sizeof(int32_t) * got, hipMemcpyDeviceToHost);
        hipMemcpy(ds, dds, sizeof(double) * got, hipMemcpyDeviceToHost);
        if (flavours == 2)
        {
            std::vector<int32_t> m2(got);
            std::vector<double> ds2(got);
            hipMemcpy(m2.data(), dm + room, sizeof(int32_t) * got, hipMemcpyDeviceToHost);
            hipMemcpy(ds2.data(), dds + room, sizeof(double) * got, hipMemcpyDeviceToHost);
            if (count[1] != count[0] || std::memcmp(m2.data(), m, sizeof(int32_t) * got) || std::memcmp(ds2.data(), ds, sizeof(double) * got))
                rc = fail(PMC_ERR_DEVICE, "octree traversal: the scalar-direction and vector-direction steps disagree on this ray");
        }
    }
    return rc;
}

}  // extern "C"

// pmc_integrate_rays (cell_weights == nullptr: sums [num_rays][num_values]) and pmc_integrate_weighted_rays (sums [num_rays][1 + num_values]: a pass
// carries the weight and PMC_INTEGRATE_PASS_VALUES - 1 values; the sum of the weights is the same in every pass and is taken from the first)
static int integrateRays(pmc_ctx* ctx, const std::string& name, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                         const double* cell_weights, const double* cell_values, double* sums)
{
    const bool weighted = cell_weights != nullptr;
    if (num_rays < 0) return fail(PMC_ERR_INVALID, name + ": negative number of rays");
    if (num_values < 0) return fail(PMC_ERR_INVALID, name + ": negative number of values");
    if (num_rays > 0 && (!origins || !directions)) return fail(PMC_ERR_INVALID, name + ": null ray arrays");
    if (num_values > 0 && !cell_values) return fail(PMC_ERR_INVALID, name + ": null cell values");
    if (num_rays > 0 && (num_values > 0 || weighted) && !sums) return fail(PMC_ERR_INVALID, name + ": null result array");
    ctx->integrateMs = 0.f;
    ctx->integrateLaneSteps = ctx->integrateWaveSteps = 0;
    if (num_rays == 0 || (num_values == 0 && !weighted)) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->sceneDirty)
    {
        HIP_TRY(pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream));
        ctx->sceneDirty = false;
    }
    const DevScene& D = ctx->dev;
    constexpr int W = PMC_INTEGRATE_PASS_VALUES;
    const size_t numCells = size_t(D.num_cells);
    // the numbering the kernel walks in: device cells of a tree (cell_ext[device cell] = the caller's m, -1: none), else the caller's
    const bool renumbered = D.grid_kind == PMC_GRID_OCTREE || D.grid_kind == PMC_GRID_BINTREE;
    const size_t slots = renumbered ? size_t(D.cell_slots) : numCells;
    std::vector<int32_t> ext;
    if (renumbered)
    {
        ext.resize(slots);
        HIP_TRY(hipMemcpy(ext.data(), D.cell_ext, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t m : ext)
            if (m >= D.num_cells) return fail(PMC_ERR_DEVICE, name + ": cell numbering table out of range");
    }
    const int64_t batchMax = int64_t(1) << 22;  // rays per launch (device memory: 10 doubles per ray)
    const size_t batchRoom = size_t(std::min(num_rays, batchMax));
    CallBuffers scratch;
    double *dOrigins = nullptr, *dDirections = nullptr, *dQ = nullptr, *dSums = nullptr;
    unsigned long long* dWork = nullptr;
    const int workWords = pmcProbeWorkWords();
    HIP_TRY(scratch.get(3 * batchRoom, &dOrigins));
    HIP_TRY(scratch.get(3 * batchRoom, &dDirections));
    HIP_TRY(scratch.get(slots * W, &dQ));
    HIP_TRY(scratch.get(W * batchRoom, &dSums));
    HIP_TRY(scratch.get(size_t(workWords), &dWork));
    hipEvent_t evA = nullptr, evB = nullptr;
    HIP_TRY(hipEventCreate(&evA));
    if (hipError_t e = hipEventCreate(&evB); e != hipSuccess)
    {
        hipEventDestroy(evA);
        return hipFail(e, "hipEventCreate");
    }
    std::vector<double> q(slots * W), part(W * batchRoom);
    std::vector<unsigned long long> work(workWords);
    unsigned long long capped = 0;
    hipError_t e = hipSuccess;
    const int perPass = weighted ? W - 1 : W;            // caller's values per pass
    const int lead = weighted ? 1 : 0;                   // members of a record (and of a ray's sums) in front of them
    const size_t stride = size_t(lead + num_values);     // the caller's sums per ray
    const int numPasses = std::max((num_values + perPass - 1) / perPass, 1);
    for (int64_t first = 0; first < num_rays && e == hipSuccess; first += batchMax)
    {
        const size_t n = size_t(std::min(batchMax, num_rays - first));
        e = hipMemcpy(dOrigins, origins + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dDirections, directions + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        // persistent waves: enough workgroups of four for every CU's share, no more than the rays fill
        const int grid = int(std::max<size_t>(1, std::min<size_t>((n + 255) / 256, size_t(ctx->numCU) * 4)));
        for (int pass = 0; pass < numPasses && e == hipSuccess; ++pass)
        {
            const int v0 = pass * perPass, nv = std::min(perPass, num_values - v0);
            for (size_t c = 0; c < slots; ++c)
            {
                const int64_t m = renumbered ? int64_t(ext[c]) : int64_t(c);
                if (weighted) q[c * W] = m >= 0 ? cell_weights[size_t(m)] : 0.;
                for (int j = 0; j < perPass; ++j) q[c * W + lead + j] = (j < nv && m >= 0) ? cell_values[size_t(v0 + j) * numCells + size_t(m)] : 0.;
            }
            e = hipMemcpy(dQ, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemsetAsync(dWork, 0, workWords * sizeof(unsigned long long), ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(evA, ctx->stream);
            if (e == hipSuccess)
                e = pmcLaunchIntegrate(ctx->slot, D.grid_kind, ctx->wide, weighted ? 1 : 0, dOrigins, dDirections, dQ, dSums, n, dWork, grid, ctx->walkLds, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(evB, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(part.data(), dSums, W * n * sizeof(double), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(work.data(), dWork, workWords * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, evA, evB) == hipSuccess) ctx->integrateMs += ms;
            capped += work[1];
            ctx->integrateLaneSteps += work[2];
            ctx->integrateWaveSteps += work[3];
            for (size_t i = 0; i < n; ++i)
            {
                if (weighted && pass == 0) sums[(size_t(first) + i) * stride] = part[i * W];
                for (int j = 0; j < nv; ++j) sums[(size_t(first) + i) * stride + size_t(lead + v0 + j)] = part[i * W + lead + j];
            }
        }
    }
    hipEventDestroy(evA);
    hipEventDestroy(evB);
    if (e != hipSuccess) return hipFail(e, name.c_str());
    if (capped)
        return fail(PMC_ERR_DEVICE, name + ": " + std::to_string(capped) + " ray walk(s) were still inside the grid after " PMC_STRINGIFY(PMC_RAY_STEP_CAP) " cells (traversal error)");
    return PMC_OK;
}

extern "C" {

int pmc_integrate_rays(pmc_ctx* ctx, int64_t num_rays, const double* origins, const double* directions, int32_t num_values, const double* cell_values,
                       double* sums)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    return integrateRays(ctx, "pmc_integrate_rays", num_rays, origins, directions, num_values, nullptr, cell_values, sums);
}

int pmc_integrate_weighted_rays(pmc_ctx* ctx, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                                const double* cell_weights, const double* cell_values, double* sums)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (!cell_weights) return fail(PMC_ERR_INVALID, "pmc_integrate_weighted_rays: null cell weights");
    return integrateRays(ctx, "pmc_integrate_weighted_rays", num_rays, origins, directions, num_values, cell_weights, cell_values, sums);
}

int pmc_last_integrate_work(pmc_ctx* ctx, float* kernel_ms, uint64_t* lane_steps, uint64_t* wave_steps)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (kernel_ms) *kernel_ms = ctx->integrateMs;
    if (lane_steps) *lane_steps = ctx->integrateLaneSteps;
    if (wave_steps) *wave_steps = ctx->integrateWaveSteps;
    return PMC_OK;
}

// the point sampler (pmc_locate.inc): the points go through the device in chunks of PMC_SAMPLE_CHUNK_POINTS, located once per chunk, the values
// gathered in passes of PMC_INTEGRATE_PASS_VALUES at the cells of the chunk.  Device memory of a call: 3 + PMC_INTEGRATE_PASS_VALUES doubles and two
// int32 per point of a chunk (64 MiB), and one pass of cell values
int pmc_sample_cells(pmc_ctx* ctx, int64_t num_points, const double* positions, int32_t num_values, const double* cell_values, double* values,
                     int32_t* cells)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (num_points < 0) return fail(PMC_ERR_INVALID, "pmc_sample_cells: negative number of points");
    if (num_values < 0) return fail(PMC_ERR_INVALID, "pmc_sample_cells: negative number of values");
    if (num_points > 0 && !positions) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null positions");
    if (num_values > 0 && !cell_values) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null cell values");
    if (num_points > 0 && num_values > 0 && !values) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null result array");
    ctx->sampleMs = 0.f;
    for (size_t i = 0, n = 3 * size_t(num_points); i < n; ++i)
        if (!std::isfinite(positions[i]))
            return fail(PMC_ERR_INVALID, "pmc_sample_cells: coordinate " + std::to_string(i % 3) + " of point " + std::to_string(i / 3) + " is not finite");
    if (num_points == 0 || (num_values == 0 && !cells)) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->sceneDirty)
    {
        HIP_TRY(pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream));
        ctx->sceneDirty = false;
    }
    const DevScene& D = ctx->dev;
    constexpr int W = PMC_INTEGRATE_PASS_VALUES;
    const size_t numCells = size_t(D.num_cells);
    // the cell values renumbered and interleaved as pmc_integrate_rays uploads them: one record [W] per cell of the walk kernels' numbering
    const bool renumbered = D.grid_kind == PMC_GRID_OCTREE || D.grid_kind == PMC_GRID_BINTREE;
    const size_t slots = renumbered ? size_t(D.cell_slots) : numCells;
    std::vector<int32_t> ext;
    if (renumbered && num_values > 0)
    {
        ext.resize(slots);
        HIP_TRY(hipMemcpy(ext.data(), D.cell_ext, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t m : ext)
            if (m >= D.num_cells) return fail(PMC_ERR_DEVICE, "pmc_sample_cells: cell numbering table out of range");
    }
    const int64_t chunkMax = PMC_SAMPLE_CHUNK_POINTS;
    const size_t chunkRoom = size_t(std::min(num_points, chunkMax));
    CallBuffers scratch;
    double *dPositions = nullptr, *dQ = nullptr, *dValues = nullptr;
    int32_t *dWalkCells = nullptr, *dCells = nullptr;
    HIP_TRY(scratch.get(3 * chunkRoom, &dPositions));
    HIP_TRY(scratch.get(chunkRoom, &dWalkCells));
    HIP_TRY(scratch.get(chunkRoom, &dCells));
    if (num_values > 0)
    {
        HIP_TRY(scratch.get(slots * W, &dQ));
        HIP_TRY(scratch.get(W * chunkRoom, &dValues));
    }
    hipEvent_t evA = nullptr, evB = nullptr;
    HIP_TRY(hipEventCreate(&evA));
    if (hipError_t e = hipEventCreate(&evB); e != hipSuccess)
    {
        hipEventDestroy(evA);
        return hipFail(e, "hipEventCreate");
    }
    const auto timed = [&](hipError_t launched) {
        hipError_t e = launched;
        if (e == hipSuccess) e = hipEventRecord(evB, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        if (e == hipSuccess && hipEventElapsedTime(&ms, evA, evB) == hipSuccess) ctx->sampleMs += ms;
        return e;
    };
    const int numPasses = (num_values + W - 1) / W;
    const size_t numChunks = size_t((num_points + chunkMax - 1) / chunkMax);
    // the records of every pass, built once on the host; with one pass they are uploaded once, with several once per chunk and pass (the
    // located cells of a chunk stay on the device for its passes, which is what bounds the device memory)
    std::vector<double> q(size_t(numPasses) * slots * W), part(num_values > 0 ? W * chunkRoom : 0);
    for (int pass = 0; pass < numPasses; ++pass)
    {
        const int v0 = pass * W, nv = std::min(W, num_values - v0);
        double* record = q.data() + size_t(pass) * slots * W;
        for (size_t c = 0; c < slots; ++c)
        {
            const int64_t m = renumbered ? int64_t(ext[c]) : int64_t(c);
            for (int j = 0; j < W; ++j) record[c * W + j] = (j < nv && m >= 0) ? cell_values[size_t(v0 + j) * numCells + size_t(m)] : 0.;
        }
    }
    hipError_t e = hipSuccess;
    for (size_t chunk = 0; chunk < numChunks && e == hipSuccess; ++chunk)
    {
        const size_t first = chunk * size_t(chunkMax);
        const size_t n = std::min(size_t(chunkMax), size_t(num_points) - first);
        // the locate kernel stages the grid tables per workgroup: no more workgroups than the CUs hold at once, no more than the points fill
        const int grid = int(std::max<size_t>(1, std::min<size_t>((n + 255) / 256, size_t(ctx->numCU) * 4)));
        e = hipMemcpy(dPositions, positions + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipEventRecord(evA, ctx->stream);
        if (e == hipSuccess)
            e = timed(pmcLaunchLocateCells(ctx->slot, D.grid_kind, ctx->wide, dPositions, dWalkCells, dCells, n, grid, ctx->walkLds, ctx->stream));
        if (e == hipSuccess && cells) e = hipMemcpy(cells + first, dCells, n * sizeof(int32_t), hipMemcpyDeviceToHost);
        for (int pass = 0; pass < numPasses && e == hipSuccess; ++pass)
        {
            const int v0 = pass * W, nv = std::min(W, num_values - v0);
            if (chunk == 0 || numPasses > 1)
                e = hipMemcpy(dQ, q.data() + size_t(pass) * slots * W, slots * W * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipEventRecord(evA, ctx->stream);
            if (e == hipSuccess) e = timed(pmcLaunchGatherCells(dWalkCells, dQ, dValues, n, nv, int((n + 255) / 256), ctx->stream));
            if (e == hipSuccess) e = hipMemcpy(part.data(), dValues, size_t(nv) * n * sizeof(double), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            for (int j = 0; j < nv; ++j) std::memcpy(values + size_t(v0 + j) * size_t(num_points) + first, part.data() + size_t(j) * n, n * sizeof(double));
        }
    }
    hipEventDestroy(evA);
    hipEventDestroy(evB);
    if (e != hipSuccess) return hipFail(e, "pmc_sample_cells");
    return PMC_OK;
}

int pmc_last_sample_ms(pmc_ctx* ctx, float* kernel_ms)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (kernel_ms) *kernel_ms = ctx->sampleMs;
    return PMC_OK;
}

}  // extern "C"
