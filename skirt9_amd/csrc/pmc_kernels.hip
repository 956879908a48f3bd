// pmc_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4) of the primary-emission photon loop.
//
// The life cycle of a photon history (MonteCarloSimulation.cpp:538-613 performLifeCycle) is a chain of grid walks
// separated by short "transitions":
//
//      launch -> [peel-off walk per observer] -> pass-1 walk (tau of the whole path) -> sample tau ->
//      pass-2 walk (same path again, up to the sampled tau) -> interaction -> [peel-off walk per observer] ->
//      scatter -> pass-1 walk ...
//
// >70 % of the work is in the walks: a pointer chase through the cell records in HBM / L2 with one dependent gather and
// about 120-150 f64 instructions per step.  The loop runs over a pool of `num_slots` concurrently live histories whose
// state lives in HBM (struct of arrays, pmc_device.h SlotArrays), divided into slot groups with a stream each; ONE
// generation of a group = one scattering cycle of every live slot of the group, and is these kernels (generation 6,
// DESIGN.md section 4):
//
//   walkPropKernel    (pmc_walk_tree.inc, octree) the propagation walk of every slot: pass 1 over the whole path, the
//                     sampled optical depth between the passes, pass 2 up to it -- from the first recorded segments in
//                     LDS where the interaction lies within them.  Persistent wavefronts, one walk per lane, per-lane
//                     directions; lanes whose walk has ended are served together in bookkeeping rounds.
//   walkPeelKernel2   (pmc_walk_tree.inc, octree; one launch per observer, on a side stream next to the propagation
//                     kernel) the peel-off walks towards one observer: the direction lives in scalar registers, every
//                     wave keeps a queue of task records in LDS from which a lane takes its next walk by itself.
//                     (walkKernel in pmc_walk.inc is the generic form for Cartesian and Voronoi grids: all walks of a
//                     slot one after the other in one lane; voroPeelKernel and voroPropKernel in pmc_walk_voro_run.inc
//                     take the walks of a Voronoi grid that has tables of runs, two lanes per walk.)
//   transitionKernel  (pmc_transition.inc) one lane per live slot, every wave working through its own compacted list:
//                     detection of the cycle's peel-off packets (FluxRecorder::detect, pmc_detect.inc: privatised SED bins
//                     and a claim-once hot-bin table in LDS in front of f64 atomics, per-history statistics lists), the
//                     interaction the propagation walk found (weights, termination), HG scattering (pmc_phase.inc) from the
//                     slot's Philox stream keyed by (seed, history index) (include/pmc_philox.h), and which observers get a
//                     peel-off packet in the next cycle (announceCycle, pmc_cycle.inc).
//   endedScanKernel   (pmc_transition.inc) exclusive scan of the per-tile counts of histories that ended: the history index
//                     a slot takes up next is a pure function of the slot order.
//   launchKernel      (pmc_launch.inc) one lane per ended history: flush of its statistics list, SourceSystem::launch of
//                     the next history, first cycle.
//   cycleStartKernel  (pmc_cycle.inc) the start state of every walk of the cycle that a live slot is about to begin (task
//                     records, pmc_device.h TaskArrays), with the counting sort that orders them (peelSort*Kernel).
//
// The host enqueues generations until no slot is alive (pmc_api.hip); one 8-byte readback per generation and group tells
// it when a group is done, and the kernels of the other groups keep the device busy meanwhile.
//
// Outside the photon loop, pmc_ray.inc runs single rays through the same traversal code: one ray cursor (rayStart, rayAdvance) under
// traceRayKernel (pmc_trace_ray: the (m, ds) of one ray, for the bit-exact check) and integrateRaysKernel (pmc_integrate_rays: one ray per lane,
// the probe maps' line integrals).  pmc_locate.inc answers SpatialGrid::cellIndex for many positions (pmc_sample_cells: locateCellsKernel, then
// gatherCellsKernel for the cell values there).
//
// The reference stores the whole path (<= 1000 x 40 B per thread) and binary-searches the interaction point
// (SpatialGridPath.cpp:164-206).  Here the path is walked twice with bit-identical arithmetic instead: pass 1 yields
// tau_path, pass 2 stops in the segment whose cumulative tau exceeds the sampled value and interpolates exactly as
// findInteractionPoint does.
//
// Arithmetic is IEEE double with contraction off (-ffp-contract=off): the reference build has no FMA, and the
// traversal must produce the same (m, ds) sequence bit for bit (pmc_trace_ray).  The only fused operations are the
// explicit ones in exactQuotient (pmc_walk.inc), which reproduce IEEE division.
//
// Octree traversal (TreeSpatialGrid.cpp:132-217): the reference hops through per-wall neighbour lists of heap nodes.
// Here a walk step gathers ONE 32-byte record of the cell it is in (pmc_device.h CellRec: density + the six links
// through its walls; two 16-byte loads of one sector), requested as soon as the cell is known, i.e. before the arithmetic
// that enters the cell; wall coordinates come from a per-axis table staged in LDS (exactly the reference's doubles).  A
// link names the leaf that covers the whole wall (same size or coarser) together with its size exponent, so that the
// box follows from the packed indices of the current cell without a load; or the same-size internal node (finer
// neighbours), from which the child follows from the index bits of the position -- without a load when the node's
// children are all leaves (consecutive cells in depth-first order).  This gives the reference's answer whenever the new
// position lies strictly inside the leaf found; in every other case (position on a shared boundary, corner overshoot,
// rounding, grid boundary) the code falls back to the literal reference algorithm on the neighbour lists kept in HBM in
// the reference's order, followed by the reference's top-down search and next-after escape.

#include "pmc_device.h"
#include "../../include/pmc_philox.h"
#include "../../include/pmc_tuning.h"
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <float.h>
#include <math.h>
#include <algorithm>
#include <mutex>
#include <array>
#include <type_traits>
#include <utility>

#ifndef PMC_WALK_REFILL
    #define PMC_WALK_REFILL 40  // waiting (idle or pending) lanes in a wave that trigger a service round (a round costs
                                // several hundred instructions whatever the number of lanes it serves)
#endif
#ifndef PMC_PEEL_REFILL
    #define PMC_PEEL_REFILL 32  // octree peel-off kernel: waiting lanes that trigger a service round (16 / 24 / 32 with the
                                // propagation kernel at 24 / 32 / 40: 413 / 387 / 376 ms per 5e7 packets, profiles/README.md)
#endif
#ifndef PMC_PROP_REFILL
    #define PMC_PROP_REFILL 40  // octree propagation kernel: likewise (its round includes the pass-1 -> pass-2 sampling)
#endif
#ifndef PMC_PEEL_BLOCK
    #define PMC_PEEL_BLOCK 768  // lanes per workgroup of the peel-off kernel (one coordinate table in LDS per workgroup): twelve waves, three per
                                // SIMD (107 registers).  On the sorted records with the round-5 step 512 / 640 / 768 / 896 / 1024 lanes: 27.1 / 26.3 /
                                // 24.5 / 25.1 / 25.9 ms per 2e7 packets in series; with the slot groups overlapped and 24 Mi slots 2.05 / 2.08 / 2.10e8
                                // packets/s for 512 / 640 / 768 (profiles/sweeps/r05_c2_peel_block.txt, r05_d6_peel768_24m.txt; with 8 Mi slots the
                                // larger workgroup gained nothing overlapped)
#endif
#ifndef PMC_PEEL_MIN_WAVES
    #define PMC_PEEL_MIN_WAVES 6  // waves per SIMD the peel-off kernel's register budget must allow (<= 80 VGPRs; it uses 75,
                                  // and must not spill: see treeSlowStep)
#endif
#ifndef PMC_PEEL2_MIN_WAVES
    #define PMC_PEEL2_MIN_WAVES 4  // peel-off kernel with the next task in registers (<= 128 VGPRs)
#endif
#ifndef PMC_PEEL2_REFILL
    #define PMC_PEEL2_REFILL 8  // peel-off kernel with task queues: waiting lanes that trigger a round (a round is cheap: the
                                // records come from LDS)
#endif
#ifndef PMC_PEEL_QCAP
    #define PMC_PEEL_QCAP 64  // task records per wave queue of the peel-off kernel (a power of two >= 64: refilled 64 at a time, when it is empty;
                              // 64 or 128 entries: the same times, and twelve queues of 64 fit next to the table of a 12-level octree)
#endif
#ifndef PMC_PROP_BLOCK
    #define PMC_PROP_BLOCK 768  // lanes per workgroup of the propagation kernel: ONE workgroup of twelve waves per CU -- three per SIMD, what
                                // the kernel's 157 registers allow -- sharing one coordinate table (24.6 KB at ten levels + 144 bytes of pass-1 checkpoints per lane = 135 KB).  With the slot groups overlapped, 1e8
                                // packets: 256 lanes (one to three workgroups per CU) 624-626 ms, 512: 645, 768: 602-608, 1024: 638-642
                                // (profiles/sweeps/r03_batch25_sweep.txt, r03_batch26_sweep.txt)
#endif
#ifndef PMC_PROP_MIN_WAVES
    #define PMC_PROP_MIN_WAVES 3  // likewise for the propagation kernel (<= 168 VGPRs; it uses 135-143)
#endif
#ifndef PMC_WALK_MIN_WAVES
    #define PMC_WALK_MIN_WAVES 3  // waves per SIMD the generic walk kernel's register budget must allow: the Voronoi walk takes 190
                                  // registers left to itself (two waves per SIMD) and runs 3 % faster with three (168 registers, 92
                                  // bytes of scratch): its visits are three dependent round trips
#endif
#ifndef PMC_LAUNCH_MIN_WAVES
    #define PMC_LAUNCH_MIN_WAVES 2  // launch kernel (statistics flush + source sampling)
#endif
#ifndef PMC_CYCLE_MIN_WAVES
    #define PMC_CYCLE_MIN_WAVES 4  // cycle start kernel (first cell and first exit distance of every walk of a cycle): 113 registers
#endif
#ifndef PMC_TRANSITION_MIN_WAVES
    #define PMC_TRANSITION_MIN_WAVES 2  // likewise for the transition and launch kernels (256 registers: two waves per SIMD; left to
                                        // itself the compiler takes 262 and halves the occupancy)
#endif
#ifndef PMC_VORO_UNROLL
    #define PMC_VORO_UNROLL 8  // Voronoi walk: neighbours whose gathers are in flight together (pmc_walk_voro.inc voroEnter)
#endif
#ifndef PMC_VPEEL_MIN_WAVES
    #define PMC_VPEEL_MIN_WAVES 4  // waves per SIMD the Voronoi peel-off kernel's register budget must allow
#endif
#ifndef PMC_VPROP_MIN_WAVES
    #define PMC_VPROP_MIN_WAVES 3  // waves per SIMD the Voronoi propagation kernel's register budget must allow
#endif
#ifndef PMC_VPROP_STEPS
    #define PMC_VPROP_STEPS 4  // scan steps of the Voronoi propagation kernel between two round checks = the tick of its checkpoints (3 / 4 / 6 / 8 / 12 on configs[4]: 514.7 / 514.9 / 516.7 / 518 / 524 ms of walk kernels per 2e7 packets)
#endif
#ifndef PMC_VPROP_ROWS
    #define PMC_VPROP_ROWS 6  // groups of PMC_VORO_RUN_LANES entries that the lanes of a propagation walk request together (one round trip)
#endif
#ifndef PMC_VPROP_REFILL
    #define PMC_VPROP_REFILL 16  // waiting lanes in a wave that trigger a service round of the Voronoi propagation kernel
#endif
#ifndef PMC_VPEEL_ROWS
    #define PMC_VPEEL_ROWS 4  // groups of PMC_VORO_RUN_LANES entries that the lanes of a walk request together (one round trip)
#endif
#ifndef PMC_VPEEL_REFILL
    #define PMC_VPEEL_REFILL 8  // waiting lanes (PMC_VORO_RUN_LANES per walk) in a wave that trigger a service round of the Voronoi peel-off kernel (2 / 4 / 8 / 16 / 32 on configs[4]: 551 / 549 / 549 / 558 / 593 ms of walk kernels per 2e7 packets)
#endif
#ifndef PMC_VORO_RUN_FIRST
    #define PMC_VORO_RUN_FIRST 4  // Voronoi peel-off walk: entries requested together with the header of a cell's run (voroEnterRun)
#endif
#ifndef PMC_VORO_CULL_ROUND
    #define PMC_VORO_CULL_ROUND 6  // Voronoi walk: neighbours per round of the masked exit search
#endif
#ifndef PMC_WALK_STEPS
    #define PMC_WALK_STEPS 8  // steps between two round checks (4 / 8 / 16 with 256 slots per claim: 597 / 592 / 594 ms per 1e8 packets)
#endif
#ifndef PMC_TRANSITION_BLOCK
    #define PMC_TRANSITION_BLOCK 256  // lanes per workgroup of the transition kernel: 256 measured 4 % faster than 512
                                      // (profiles/README.md); small enough to share a CU with the walk kernel
#endif
static_assert(PMC_TRANSITION_BLOCK <= 256 && PMC_TRANSITION_BLOCK % 64 == 0,
              "the per-wave slot lists of the transition and launch kernels are laid out for at most four waves per workgroup");
#ifndef PMC_SCAN_THREADS
    #define PMC_SCAN_THREADS 256  // lanes of the one-workgroup scan kernels (endedScanKernel, rfScanKernel): see endedScanKernel
#endif
#ifndef PMC_TASK_CHUNK
    #define PMC_TASK_CHUNK 256  // slots a wave takes from the global cursor at a time (64 / 128 / 256 / 512 / 1024: 611 / 597 / 592 / 600 /
                                // 623 ms per 1e8 packets, profiles/sweeps/r03_batch32_sweep.txt, r03_batch33_sweep.txt)
#endif

// A tree with one of the experiment patches of profiles/experiments applied (tuning aids: they change results or add work)
// identifies itself: every such patch defines the macro below, and pmc_create prints a warning for such a library (pmc_api.hip)
#ifdef PMC_EXPERIMENT_BUILD
extern "C" int pmcExperimentBuild(void) { return 1; }
#else
extern "C" int pmcExperimentBuild(void) { return 0; }
#endif
extern "C" const char* pmcTune(const char* name);  // tuning switches (pmc_api.hip, include/pmc_tuning.h)

// the scene of every live context, in constant memory: all accesses are scalar loads
__constant__ DevScene c_scene[PMC_MAX_CONTEXTS];

namespace
{
    enum Mode : int { MODE_PASS1 = 0, MODE_PASS2 = 1, MODE_PEEL = 2, MODE_NONE = 3 };
    enum Grid : int { GRID_CART = PMC_GRID_CARTESIAN, GRID_TREE = PMC_GRID_OCTREE, GRID_VORO = PMC_GRID_VORONOI, GRID_BIN = PMC_GRID_BINTREE };
    constexpr int MODE_ALIVE = PMC_MODE_ALIVE;
    constexpr int MODE_ENDED = 1 << 6;  // the history of the slot has ended: the launch kernel takes up the next one

    // ------------------------------------------------------------------------------------------------
    struct Rng
    {
        uint32_t h0, h1, block, have;
        double spare;
    };
    __device__ __forceinline__ double rngUniform(Rng& g, uint64_t seed)
    {
        if (g.have)
        {
            g.have = 0;
            return g.spare;
        }
        uint32_t c[4] = {g.h0, g.h1, g.block, 0x504d4331u};
        g.block += 1;
        pmc_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        g.spare = pmc_bits_to_unit(c[2], c[3]);
        g.have = 1;
        return pmc_bits_to_unit(c[0], c[1]);
    }

    __device__ __forceinline__ void loadRng(const SlotArrays& A, int slot, Rng& rng)
    {
        const uint64_t h = A.history[slot];
        const uint32_t rb = A.rngBlock[slot];
        rng.h0 = (uint32_t)h;
        rng.h1 = (uint32_t)(h >> 32);
        rng.block = rb >> 1;
        rng.have = rb & 1;
        rng.spare = A.rngSpare[slot];
    }
    __device__ __forceinline__ void storeRng(const SlotArrays& A, int slot, const Rng& rng)
    {
        A.rngBlock[slot] = (rng.block << 1) | (rng.have & 1);
        A.rngSpare[slot] = rng.spare;
    }

    __device__ __forceinline__ int locateBasic(const double* xv, double x, int n)
    {
        int jl = -1, ju = n;
        while (ju - jl > 1)
        {
            int jm = (ju + jl) >> 1;
            if (x < xv[jm])
                ju = jm;
            else
                jl = jm;
        }
        return jl;
    }
    __device__ __forceinline__ int locateClip(const double* xv, int n, double x)
    {
        if (x < xv[0]) return 0;
        return locateBasic(xv, x, n - 1);
    }
    __device__ __forceinline__ int locate(const double* xv, int n, double x)
    {
        if (x == xv[n - 1]) return n - 2;
        return locateBasic(xv, x, n);
    }

    __device__ __forceinline__ unsigned long long waveSum(uint32_t value)
    {
        unsigned long long v = value;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        return v;
    }

#include "pmc_walk.inc"
#include "pmc_walk_voro_run.inc"
#include "pmc_walk_tree.inc"
#include "pmc_log.inc"
#include "pmc_phase.inc"
#include "pmc_detect.inc"
#include "pmc_cycle.inc"
#include "pmc_transition.inc"
#include "pmc_launch.inc"
#include "pmc_ray.inc"
#include "pmc_locate.inc"
}

// ---------------------------------------------------------------------------------------------------
// launch wrappers used by pmc_api.hip

extern "C" hipError_t pmcUploadScene(int slot, const DevScene* scene, hipStream_t stream)
{
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(c_scene), scene, sizeof(DevScene), size_t(slot) * sizeof(DevScene),
                                  hipMemcpyHostToDevice, stream);
}

// LDS bytes of the task queues of one peel-off workgroup (walkPeelKernel2)
static size_t pmcPeelQueueBytes()
{
    return size_t(PMC_PEEL_BLOCK / 64) * PEEL_QBYTES;
}

// ---- the instantiations of every walk kernel family, each listed once: entry f of a family's table is the kernel of flavour f and the
// dynamic LDS it may be launched with beyond the grid tables (pmcConfigureKernels: min(walkLds + extraLds, 160 KiB))
template<typename Kernel> struct KernelFlavour
{
    Kernel kernel;
    size_t extraLds;
};
// entry f = make(f) for f = 0 .. N - 1 (f as a compile-time constant: decltype(f)::value)
template<typename Make, int... F> static auto expandFlavours(Make make, std::integer_sequence<int, F...>)
{
    return std::array<decltype(make(std::integral_constant<int, 0>())), sizeof...(F)>{{make(std::integral_constant<int, F>())...}};
}
template<int N, typename Make> static auto flavourTable(Make make) { return expandFlavours(make, std::make_integer_sequence<int, N>()); }
// walk flavour (pmcLaunchWalk, pmcLaunchProp, pmcLaunchVoroProp): bit 0 the radiation field is stored, bit 1 explicit absorption, bit 2 several
// medium components -- separate instantiations, so that the plain photon loop pays nothing for them
// (only the propagation kernel without explicit absorption and several media keeps pass-1 checkpoints next to the grid tables)
static bool flavourHasCheckpointRoom(int flavour) { return (flavour & 6) == 0; }
// octree propagation: flavour | 8 for a wide octree
typedef void (*PropKernel)(int, int, int, int, uint64_t, int, RfLogArgs, const int*);
static const auto propKernels = flavourTable<16>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<PropKernel>{walkPropKernel<(F & 8) != 0, (F & 1) != 0, (F & 2) != 0, (F & 4) != 0>, flavourHasCheckpointRoom(F) ? size_t(16 + PROP_CKPT_BYTES) : 0};
});
// generic walks (Cartesian, Voronoi): flavour | 8 on a Voronoi grid
typedef void (*WalkKernel)(int, int, int, int, uint64_t, WalkStreamArgs);
static const auto walkKernels = flavourTable<16>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<WalkKernel>{walkKernel<(F & 8) ? GRID_VORO : GRID_CART, (F & 1) != 0, (F & 2) != 0, (F & 4) != 0>, 0};
});
// generic walks on a binary tree (a table of its own: the entries of the table above stay what they were)
static const auto binWalkKernels = flavourTable<8>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<WalkKernel>{walkKernel<GRID_BIN, (F & 1) != 0, (F & 2) != 0, (F & 4) != 0>, 0};
});
// Voronoi propagation on the table of runs: static LDS only (launched without dynamic LDS; its limit is never raised)
typedef void (*VoroPropKernel)(int, const int32_t*, const unsigned long long*, unsigned long long*, int, uint64_t);
static const auto voroPropKernels = flavourTable<8>([](auto f) {
    constexpr int F = decltype(f)::value;
    return VoroPropKernel(voroPropKernel<(F & 1) != 0, (F & 2) != 0, (F & 4) != 0>);
});
// octree peel-off with service rounds: form & 3 (bit 0 wide, bit 1 several medium components)
typedef void (*PeelKernel)(int, int, int, int, int, const int*);
static const auto peelKernels = flavourTable<4>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<PeelKernel>{walkPeelKernel<(F & 1) != 0, (F & 2) != 0>, 0};
});
// octree peel-off with task queues: one instantiation per sign octant of the observer's direction (bit a of sgn: k_a < 0); sgn | 8 when wide
typedef void (*PeelKernel2)(int, int, int, int, int, int, const int*, PeelSortedArgs);
static const auto peel2Kernels = flavourTable<16>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<PeelKernel2>{walkPeelKernel2<(F & 8) != 0, F & 7>, 16 + pmcPeelQueueBytes()};
});

// ray kernels (pmc_ray.inc), member i of a family: the octree, the wide octree, the Cartesian, Voronoi and binary-tree grids
constexpr Grid RAY_GRIDS[5] = {GRID_TREE, GRID_TREE, GRID_CART, GRID_VORO, GRID_BIN};
static int rayKernelIndex(int gridKind, int wide)
{
    return gridKind == PMC_GRID_OCTREE ? (wide ? 1 : 0) : gridKind == PMC_GRID_VORONOI ? 3 : gridKind == PMC_GRID_BINTREE ? 4 : 2;
}
typedef void (*IntegrateKernel)(int, ProbeArgs);
static const auto integrateKernels = flavourTable<5>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<IntegrateKernel>{integrateRaysKernel<RAY_GRIDS[F], F == 1, false>, 0};
});
// ... and the weighted averages (pmc_integrate_weighted_rays)
static const auto integrateWeightedKernels = flavourTable<5>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<IntegrateKernel>{integrateRaysKernel<RAY_GRIDS[F], F == 1, true>, 0};
});
// the point sampler (pmc_locate.inc, pmc_sample_cells)
typedef void (*LocateKernel)(int, LocateArgs);
static const auto locateKernels = flavourTable<5>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<LocateKernel>{locateCellsKernel<RAY_GRIDS[F], F == 1>, 0};
});
// launch kernel: the launch flavour (pmc_device.h PMC_LAUNCH_*, pmcLaunchFlavourOf); flavour 0 (| PMC_LAUNCH_KIN) is the generic kernel
typedef void (*LaunchKernel)(int, int, int, int, uint64_t, uint64_t, uint64_t, int, StatLogArgs);
static const auto launchKernels = flavourTable<PMC_LAUNCH_FLAVOURS>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<LaunchKernel>{launchKernel<F>, 0};
});
// single-ray tracer: the five with the direction in scalar registers, then the octree's two with the direction in vector registers
typedef void (*TraceKernel)(int, double, double, double, double, double, double, const double*, int32_t*, double*, int32_t, int32_t*);
static const auto traceKernels = flavourTable<7>([](auto f) {
    constexpr int F = decltype(f)::value;
    return KernelFlavour<TraceKernel>{traceRayKernel<RAY_GRIDS[F % 5], F % 5 == 1, (F < 5)>, 0};
});

template<typename Table> static hipError_t raiseLdsLimits(const Table& table, size_t walkMax)
{
    for (const auto& k : table)
    {
        const size_t lds = k.extraLds ? std::min(walkMax + k.extraLds, size_t(160) * 1024) : walkMax;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the dynamic-LDS limit is a property of the kernel, not of a context: it is only ever raised (a small scene created
// after a large one must not lower the limit under the live context)
extern "C" hipError_t pmcConfigureKernels(size_t walkLds, size_t transitionLds)
{
    // (contexts are created concurrently by one host thread per device; the attribute is per device, so every pmc_create
    // sets it on its own current device)
    static std::mutex lock;
    std::lock_guard<std::mutex> guard(lock);
    static size_t walkMax = 0, transitionMax = 0;
    walkMax = std::max(walkMax, walkLds);
    transitionMax = std::max(transitionMax, transitionLds);
    {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rfReduceKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(double) << PMC_RF_BUCKET_BITS));
        if (e != hipSuccess) return e;
        const int scatterLds = (int)(size_t(RF_TILE) * (sizeof(double) + sizeof(uint32_t)) + size_t(2) * RF_MAX_PARTS * sizeof(uint32_t));
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rfScatterKernel<PMC_RF_BUCKET_BITS>), hipFuncAttributeMaxDynamicSharedMemorySize, scatterLds);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rfScatterKernel<PMC_STAT_BUCKET_BITS>), hipFuncAttributeMaxDynamicSharedMemorySize, scatterLds);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&statReduceKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(5 * sizeof(double) << PMC_STAT_BUCKET_BITS));
        if (e != hipSuccess) return e;
    }
    for (hipError_t e : {raiseLdsLimits(peelKernels, walkMax), raiseLdsLimits(peel2Kernels, walkMax), raiseLdsLimits(propKernels, walkMax),
                         raiseLdsLimits(walkKernels, walkMax), raiseLdsLimits(binWalkKernels, walkMax), raiseLdsLimits(traceKernels, walkMax),
                         raiseLdsLimits(integrateKernels, walkMax), raiseLdsLimits(integrateWeightedKernels, walkMax), raiseLdsLimits(locateKernels, walkMax)})
        if (e != hipSuccess) return e;
    const struct
    {
        const void* kernel;
        size_t lds;
    } all[] = {{reinterpret_cast<const void*>(&transitionKernel), transitionMax},
               {reinterpret_cast<const void*>(&transitionDipoleKernel), transitionMax},
               {reinterpret_cast<const void*>(&transitionKinKernel), transitionMax},
               {reinterpret_cast<const void*>(&transitionKinDipoleKernel), transitionMax},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_TREE, true>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_CART, true>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_VORO, true>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_TREE>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_CART>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_VORO>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_BIN, true>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)},
               {reinterpret_cast<const void*>(&cycleStartKernel<GRID_BIN>), walkMax + 16 + size_t(PMC_SORT_OBS) * PMC_PEEL_TILES * PMC_PEEL_TILES * sizeof(uint32_t)}};
    for (const auto& k : all)
    {
        hipError_t e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
        if (e != hipSuccess) return e;
    }
    return raiseLdsLimits(launchKernels, transitionMax);
}

// does the octree propagation kernel of this walk flavour keep its pass-1 checkpoints in LDS, behind the grid tables of ldsBytes?
extern "C" int pmcPropHasCheckpoints(int flavour, size_t ldsBytes)
{
    // (tuning aid PMC_PROP_NO_CHECKPOINTS: pass 2 walks every path from its start)
    return flavourHasCheckpointRoom(flavour) && !pmcTune("PMC_PROP_NO_CHECKPOINTS") && ((ldsBytes + 15) & ~size_t(15)) + PROP_CKPT_BYTES <= size_t(160) * 1024;
}
// does the peel-off kernel of this octree run with task queues (the form that can take sorted records)?  form: bit 0 wide, bit 1 several medium
// components (the form with service rounds); an octree of 12 levels leaves no room for the queues next to its coordinate table
extern "C" int pmcPeelHasQueues(int form, size_t ldsBytes)
{
    return (form & 2) == 0 && ((ldsBytes + 15) & ~size_t(15)) + pmcPeelQueueBytes() <= size_t(160) * 1024;
}

// resident workgroups per CU of a walk kernel: kind 0 = generic (Cartesian / Voronoi), 1 = octree peel-off, 2 = octree
// propagation
extern "C" int pmcWalkBlocksPerCU(int gridKind, int kind, int wide, int block, size_t ldsBytes)
{
    const void* kernel;
    if (gridKind == PMC_GRID_OCTREE && kind == 1)
        kernel = reinterpret_cast<const void*>(peelKernels[wide ? 1 : 0].kernel);
    else if (gridKind == PMC_GRID_OCTREE)
    {
        // (with the pass-1 checkpoints of pmcLaunchProp)
        if (pmcPropHasCheckpoints(0, ldsBytes)) ldsBytes = ((ldsBytes + 15) & ~size_t(15)) + PROP_CKPT_BYTES;
        kernel = reinterpret_cast<const void*>(propKernels[wide ? 8 : 0].kernel);
    }
    else if (gridKind == PMC_GRID_BINTREE)
        kernel = reinterpret_cast<const void*>(binWalkKernels[0].kernel);
    else
        kernel = reinterpret_cast<const void*>(walkKernels[gridKind == PMC_GRID_VORONOI ? 8 : 0].kernel);
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, ldsBytes) == hipSuccess ? n : 0;
}

extern "C" int pmcPeelBlock(void)
{
    return PMC_PEEL_BLOCK;
}
extern "C" int pmcPropBlock(void)
{
    return PMC_PROP_BLOCK;
}


// walks of the task records [taskBase, taskBase + numTaskRecords) of one slot group on a Cartesian or Voronoi grid;
// taskCounter = index of the group's (zeroed) cursor; flavour: the walk flavour (above)
extern "C" hipError_t pmcLaunchWalk(int slot, int gridKind, int flavour, int taskBase, int numTaskRecords, int taskCounter,
                                    uint64_t seed, int grid, int block, size_t ldsBytes, const WalkStreamArgs* tasks, hipStream_t stream)
{
    WalkStreamArgs ws;
    std::memset(&ws, 0, sizeof(ws));
    if (tasks) ws = *tasks;
    const WalkKernel kernel = gridKind == PMC_GRID_BINTREE ? binWalkKernels[flavour & 7].kernel : walkKernels[(flavour & 7) | (gridKind == PMC_GRID_VORONOI ? 8 : 0)].kernel;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), ldsBytes, stream, slot, taskBase, numTaskRecords, taskCounter, seed, ws);
    return hipGetLastError();
}

// Voronoi: the peel-off walks of the slots in `list` (their number: *count, device memory) towards the observer of task record `rec`, whose table of
// runs is DevScene::vobs_run[tab]; xcdCursor: `segments` (8 or 1) zeroed cursors over equal parts of the list
extern "C" int pmcVoroPeelWavesPerSimd(void) { return PMC_VPEEL_MIN_WAVES; }
extern "C" hipError_t pmcLaunchVoroPeel(int slot, int rec, int tab, const int32_t* list, const unsigned long long* count, unsigned long long* xcdCursor, int segments,
                                        int severalMedia, int grid, hipStream_t stream)
{
    hipLaunchKernelGGL(severalMedia ? voroPeelKernel<true> : voroPeelKernel<false>, dim3(grid), dim3(256), 0, stream, slot, rec, tab, list, count, xcdCursor,
                       segments);
    return hipGetLastError();
}

// Voronoi: the propagation walks (task record 0) of the slots in `list` on the table of runs DevScene::vgen_run
extern "C" int pmcVoroPropWavesPerSimd(void) { return PMC_VPROP_MIN_WAVES; }
// flavour: the walk flavour (above)
extern "C" hipError_t pmcLaunchVoroProp(int slot, const int32_t* list, const unsigned long long* count, unsigned long long* xcdCursor, int segments, uint64_t seed,
                                        int flavour, int grid, hipStream_t stream)
{
    hipLaunchKernelGGL(voroPropKernels[flavour & 7], dim3(grid), dim3(256), 0, stream, slot, list, count, xcdCursor, segments, seed);
    return hipGetLastError();
}

// sorted peel-off records (pmc_device.h PeelRec): the count pass of the sort over the slots of a group, behind its transition / launch kernels; the
// cycle start kernel, launched with the SAME number of workgroups (returned through `groups`), is the scatter pass.  temp: pmcPeelSortTempBytes();
// the number of sorted records is left at pmcPeelSortedCount(temp)
constexpr int PEEL_SORT_GROUPS = 1024;
constexpr int PEEL_SORT_PARTS = PMC_PEEL_TILES * PMC_PEEL_TILES;
extern "C" size_t pmcPeelSortTempBytes()
{
    // counters (totals, then starts: 2 * parts + 1) followed by the matrix [groups][parts]
    return (size_t(2) * PEEL_SORT_PARTS + 2) * sizeof(unsigned long long) + size_t(PEEL_SORT_GROUPS) * PEEL_SORT_PARTS * sizeof(uint32_t);
}
extern "C" const unsigned long long* pmcPeelSortedCount(void* temp) { return static_cast<const unsigned long long*>(temp) + 2 * PEEL_SORT_PARTS; }
// (ps: numObs, obs, sortIndex, centre, scale set by the caller; sorted[k] / temp[k]: the records and counters of observer k)
extern "C" hipError_t pmcLaunchPeelSortCounts(int slot, int slotBase, int numSlots, PeelSortArgs* ps, PeelRec* const* sorted, int32_t* const* lists, void* const* temp,
                                              int* groups, hipStream_t stream)
{
    ps->numParts = PEEL_SORT_PARTS;
    const int numLists = ps->numObs + (ps->propIndex >= 0 ? 1 : 0);
    for (int k = 0; k < numLists; ++k)
    {
        unsigned long long* totals = static_cast<unsigned long long*>(temp[k]);
        ps->out[k] = sorted ? sorted[k] : nullptr;
        ps->listOut[k] = lists ? lists[k] : nullptr;
        ps->matrix[k] = reinterpret_cast<uint32_t*>(totals + 2 * PEEL_SORT_PARTS + 2);
        ps->start[k] = totals + PEEL_SORT_PARTS;
    }
    const int tiles = (numSlots + PEEL_SORT_TILE - 1) / PEEL_SORT_TILE;
    *groups = std::max(1, std::min(tiles, PEEL_SORT_GROUPS));
    hipLaunchKernelGGL(peelSortCountKernel, dim3(*groups), dim3(256), 0, stream, slot, slotBase, numSlots, *ps);
    for (int k = 0; k < numLists; ++k)
    {
        unsigned long long* totals = static_cast<unsigned long long*>(temp[k]);
        hipLaunchKernelGGL(peelSortOffsetsKernel, dim3((PEEL_SORT_PARTS + 15) / 16), dim3(256), 0, stream, ps->matrix[k], (uint32_t)*groups, (uint32_t)PEEL_SORT_PARTS, totals);
        hipLaunchKernelGGL(rfScanKernel, dim3(1), dim3(PMC_SCAN_THREADS), 0, stream, totals, totals + PEEL_SORT_PARTS, (uint32_t)PEEL_SORT_PARTS);
    }
    return hipGetLastError();
}

// octree: the peel-off walks towards observer `obs` of the slots [slotBase, slotBase + numSlots); form: bit 0 wide, bit 1 several medium
// components, bit 2 task queues (pmcPeelHasQueues)
extern "C" hipError_t pmcLaunchPeel(int slot, int form, int slotBase, int numSlots, const int* list, int cursor, int obs, int sgn, int grid, size_t ldsBytes,
                                    const PeelRec* sortedRec, const unsigned long long* sortedCount, unsigned long long* xcdCursor, hipStream_t stream)
{
    if (!(form & 4))
        hipLaunchKernelGGL(peelKernels[form & 3].kernel, dim3(grid), dim3(PMC_PEEL_BLOCK), ldsBytes, stream, slot, slotBase, numSlots, cursor, obs, list);
    else
    {
        // (the waves' task queues follow the grid tables in LDS)
        // (sgn: the sign octant of the observer's direction, DevInstrument::sgn)
        const size_t queueOffset = (ldsBytes + 15) & ~size_t(15);
        const PeelSortedArgs sorted = {sortedRec, sortedCount, xcdCursor};
        hipLaunchKernelGGL(peel2Kernels[(form & 1) * 8 + (sgn & 7)].kernel, dim3(grid), dim3(PMC_PEEL_BLOCK), queueOffset + pmcPeelQueueBytes(), stream, slot,
                           slotBase, numSlots, cursor, obs, (int)queueOffset, list, sorted);
    }
    return hipGetLastError();
}

// octree: the propagation walks of the slots [slotBase, slotBase + numSlots); checkpoints: pmcPropHasCheckpoints (the pass-1 checkpoints follow
// the grid tables in LDS)
extern "C" hipError_t pmcLaunchProp(int slot, int wide, int flavour, int checkpoints, int slotBase, int numSlots, const int* list, int cursor, uint64_t seed,
                                    int grid, size_t ldsBytes, const RfLogArgs* rfLog, hipStream_t stream)
{
    const PropKernel kernel = propKernels[(flavour & 7) | (wide ? 8 : 0)].kernel;
    const size_t trimOffset = (ldsBytes + 15) & ~size_t(15);
    RfLogArgs none = {nullptr, nullptr, 0ull, 0, 0u};
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(PMC_PROP_BLOCK), checkpoints ? trimOffset + PROP_CKPT_BYTES : ldsBytes, stream, slot, slotBase, numSlots, cursor,
                       seed, checkpoints ? (int)trimOffset : -1, rfLog ? *rfLog : none, list);
    return hipGetLastError();
}

// radiation field: the log of a generation (n entries in whole chunks) partitioned by key range into (sortedKeys, sortedVals) and
// added to the table; temp = 2 * numParts + 1 counters (pmcRfTempBytes)
extern "C" size_t pmcRfTempBytes(int numParts) { return (size_t(2) * size_t(numParts) + 1) * sizeof(unsigned long long); }
extern "C" int pmcRfMaxParts() { return (int)RF_MAX_PARTS; }
// the counting sort of (key, value) pairs on key >> PMC_RF_BUCKET_BITS: n entries in whole tiles of RF_TILE -> (sortedKeys, sortedVals), pad
// keys dropped; temp = 2 * numParts + 1 counters: the partition starts are left at temp + numParts (numParts + 1 of them)
template<int BITS>
static hipError_t launchPartition(const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n, int numParts,
                                  void* temp, int numCU, hipStream_t stream, const uint32_t* fills = nullptr)
{
    unsigned long long* cursor = static_cast<unsigned long long*>(temp);
    unsigned long long* start = cursor + numParts;
    hipError_t e = hipMemsetAsync(cursor, 0, size_t(numParts) * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    const unsigned long long tiles = n / RF_TILE;
    const unsigned grid = (unsigned)std::min<unsigned long long>(tiles, (unsigned long long)numCU * 8ull);
    hipLaunchKernelGGL(rfHistKernel<BITS>, dim3(std::max(grid, 1u)), dim3(256), 0, stream, keys, n, (uint32_t)numParts, cursor, fills);
    hipLaunchKernelGGL(rfScanKernel, dim3(1), dim3(PMC_SCAN_THREADS), 0, stream, cursor, start, (uint32_t)numParts);
    const size_t sortLds = size_t(RF_TILE) * (sizeof(double) + sizeof(uint32_t)) + size_t(2) * size_t(numParts) * sizeof(uint32_t);
    const unsigned sortGrid = (unsigned)std::min<unsigned long long>(tiles, (unsigned long long)numCU * 3ull);
    hipLaunchKernelGGL(rfScatterKernel<BITS>, dim3(std::max(sortGrid, 1u)), dim3(RF_SORT_BLOCK), sortLds, stream, keys, vals, n, (uint32_t)numParts, cursor, sortedKeys,
                       sortedVals, fills);
    return hipGetLastError();
}
extern "C" hipError_t pmcLaunchRfFlush(int slot, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                       int numParts, void* temp, int numCU, hipStream_t stream)
{
    hipError_t e = launchPartition<PMC_RF_BUCKET_BITS>(keys, vals, sortedKeys, sortedVals, n, numParts, temp, numCU, stream);
    if (e != hipSuccess) return e;
    const unsigned long long* start = static_cast<const unsigned long long*>(temp) + numParts;
    const size_t lds = sizeof(double) << PMC_RF_BUCKET_BITS;  // (the limit is raised per device in pmcConfigureKernels)
    const unsigned long long blocks = (n + PMC_RF_REDUCE_SPAN - 1) / PMC_RF_REDUCE_SPAN;
    hipLaunchKernelGGL(rfReduceKernel, dim3((unsigned)blocks), dim3(RF_REDUCE_BLOCK), lds, stream, slot, sortedKeys, sortedVals, start, (uint32_t)numParts);
    return hipGetLastError();
}
// statistics: the log of a slot group (n entries in whole chunks) partitioned by record range into (sortedKeys, sortedVals) and summed into the
// accumulator records; temp = 2 * numParts + 1 counters (pmcRfTempBytes)
extern "C" int pmcStatBucketBits() { return PMC_STAT_BUCKET_BITS; }
extern "C" hipError_t pmcLaunchStatFlush(int slot, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                         int numParts, void* temp, int numCU, const uint32_t* chunkFill, hipStream_t stream)
{
    hipError_t e = launchPartition<PMC_STAT_BUCKET_BITS>(keys, vals, sortedKeys, sortedVals, n, numParts, temp, numCU, stream, chunkFill);
    if (e != hipSuccess) return e;
    const unsigned long long* start = static_cast<const unsigned long long*>(temp) + numParts;
    const size_t lds = 5 * sizeof(double) << PMC_STAT_BUCKET_BITS;
    const unsigned long long blocks = (n + PMC_RF_REDUCE_SPAN - 1) / PMC_RF_REDUCE_SPAN;
    hipLaunchKernelGGL(statReduceKernel, dim3((unsigned)blocks), dim3(RF_REDUCE_BLOCK), lds, stream, slot, sortedKeys, sortedVals, start, (uint32_t)numParts);
    return hipGetLastError();
}
// test aids (include/pmc_tuning.h): the constants the kernels above are built with, and the counting sort alone
extern "C" void pmcLogConstants(pmc_log_geometry_values* out)
{
    out->chunk = PMC_RF_LOG_CHUNK;
    out->rf_bucket_bits = PMC_RF_BUCKET_BITS;
    out->stat_bucket_bits = PMC_STAT_BUCKET_BITS;
    out->scan_threads = PMC_SCAN_THREADS;
    out->sort_block = RF_SORT_BLOCK;
    out->max_parts = RF_MAX_PARTS;
    out->reduce_span = (int64_t)PMC_RF_REDUCE_SPAN;
    out->rf_short_run = PMC_RF_SHORT_RUN;
    out->stat_short_run = PMC_STAT_SHORT_RUN;
}
extern "C" hipError_t pmcLaunchLogPartition(int stat, const uint32_t* keys, const double* vals, uint32_t* sortedKeys, double* sortedVals, unsigned long long n,
                                            int numParts, void* temp, int numCU, const uint32_t* fills, hipStream_t stream)
{
    return stat ? launchPartition<PMC_STAT_BUCKET_BITS>(keys, vals, sortedKeys, sortedVals, n, numParts, temp, numCU, stream, fills)
                : launchPartition<PMC_RF_BUCKET_BITS>(keys, vals, sortedKeys, sortedVals, n, numParts, temp, numCU, stream, fills);
}
// end of a segment: statistics accumulator -> wifu arrays of the frames
extern "C" hipError_t pmcLaunchStatMerge(int slot, int blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(statMergeKernel, dim3(blocks), dim3(256), 0, stream, slot);
    return hipGetLastError();
}

// transitions of the slots [slotBase, slotBase + numSlots) of slot group `group`, followed by the scan of the group's
// ended-history counts (the launch kernel's history indices)
// flavour: bit 0 some medium component has the dipole phase function (DevScene::any_dipole), bit 1 some source moves (DevScene::kin): the kernel
// flavour that knows them
extern "C" hipError_t pmcLaunchTransition(int slot, int flavour, int slotBase, int numSlots, int group, uint64_t seed, const int* list, int listLen, int maxBlocks,
                                          size_t ldsBytes, const StatLogArgs* statLog, uint64_t count, hipStream_t stream)
{
    const StatLogArgs none = {nullptr, nullptr, 0ull, 0, nullptr, nullptr, nullptr};
    const int block = PMC_TRANSITION_BLOCK;
    // (a sparse generation: one list entry per lane; otherwise persistent workgroups over runs of 256 slots per wave)
    const int grid = std::max(1, std::min(((list ? listLen : numSlots) + block - 1) / block, maxBlocks));
    const auto kernel = (flavour & 2) ? ((flavour & 1) ? transitionKinDipoleKernel : transitionKinKernel) : ((flavour & 1) ? transitionDipoleKernel : transitionKernel);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), ldsBytes, stream, slot, slotBase, numSlots, group, seed, list, listLen,
                       statLog ? *statLog : none);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || list) return e;  // (a sparse generation retires its ended histories in the transition kernel)
    hipLaunchKernelGGL(endedScanKernel, dim3(1), dim3(PMC_SCAN_THREADS), 0, stream, slot, slotBase, numSlots, group, (unsigned long long)count);
    return hipGetLastError();
}

// launches of new histories into the slots of the group whose history ended (initial: into all slots of the group); flavour: the launch
// flavour of the scene (pmcLaunchFlavourOf), or the generic one (PMC_LAUNCH_KIN alone where some source moves)
extern "C" hipError_t pmcLaunchLaunch(int slot, int flavour, int slotBase, int numSlots, int group, uint64_t first, uint64_t count, uint64_t seed, int initial,
                                      int maxBlocks, size_t ldsBytes, const StatLogArgs* statLog, hipStream_t stream)
{
    const StatLogArgs none = {nullptr, nullptr, 0ull, 0, nullptr, nullptr, nullptr};
    const int grid = std::max(1, std::min((numSlots + 255) / 256, maxBlocks));
    if (flavour < 0 || flavour >= PMC_LAUNCH_FLAVOURS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(launchKernels[flavour].kernel, dim3(grid), dim3(256), ldsBytes, stream, slot, slotBase, numSlots, group, first, count, seed, initial,
                       statLog ? *statLog : none);
    return hipGetLastError();
}

// the walks of the cycle that every live slot of the group is about to start (task records); kin: some source moves
extern "C" hipError_t pmcLaunchCycleStart(int slot, int gridKind, int kin, int slotBase, int numSlots, int listCounter, int* listOut, const int* listIn,
                                          int listLen, int maxBlocks, size_t ldsBytes, const PeelSortArgs* sort, hipStream_t stream)
{
    PeelSortArgs ps;
    std::memset(&ps, 0, sizeof(ps));
    if (sort) ps = *sort;
    if (ps.numObs > 0)
    {
        // (the sorts' cursors follow the grid tables in LDS; as many workgroups as the sort's count pass had: maxBlocks is that number then)
        ps.ldsOffset = int((ldsBytes + 15) & ~size_t(15));
        ldsBytes = size_t(ps.ldsOffset) + size_t(ps.numObs + (ps.propIndex >= 0 ? 1 : 0)) * PEEL_SORT_PARTS * sizeof(uint32_t);
    }
    const int grid = std::max(1, std::min(((listIn ? listLen : numSlots) + 255) / 256, maxBlocks));
    const auto kernel = kin ? (gridKind == PMC_GRID_OCTREE ? cycleStartKernel<GRID_TREE, true> : gridKind == PMC_GRID_VORONOI ? cycleStartKernel<GRID_VORO, true>
                               : gridKind == PMC_GRID_BINTREE ? cycleStartKernel<GRID_BIN, true> : cycleStartKernel<GRID_CART, true>)
                            : (gridKind == PMC_GRID_OCTREE ? cycleStartKernel<GRID_TREE> : gridKind == PMC_GRID_VORONOI ? cycleStartKernel<GRID_VORO>
                               : gridKind == PMC_GRID_BINTREE ? cycleStartKernel<GRID_BIN> : cycleStartKernel<GRID_CART>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), ldsBytes, stream, slot, slotBase, numSlots, listCounter, listOut, listIn, listLen, ps);
    return hipGetLastError();
}

// test aid (pmc_tuning.h pmc_tune_dipole_cosines): the transition kernel's own conversion of a uniform deviate into the scattering cosine of
// the dipole phase function, over n deviates in device memory
namespace
{
    __global__ __launch_bounds__(256) void dipoleCosineKernel(const double* __restrict__ u, const int64_t n, double* __restrict__ out)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) out[i] = PhaseDipole::cosineFor(u[i]);
    }
}
extern "C" hipError_t pmcLaunchDipoleCosines(const double* u, int64_t n, double* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(dipoleCosineKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, u, n, out);
    return hipGetLastError();
}

// test aid (pmc_tuning.h pmc_tune_source_velocities): the launch kernel's own velocity function of source `source` over n positions [n][3] in
// device memory
namespace
{
    __global__ __launch_bounds__(256) void sourceVelocityKernel(const int sceneSlot, const int source, const double* __restrict__ r, const int64_t n,
                                                                double* __restrict__ out)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        double vx, vy, vz;
        sourceVelocity(c_scene[sceneSlot].vel[source], r[3 * i], r[3 * i + 1], r[3 * i + 2], vx, vy, vz);
        out[3 * i] = vx, out[3 * i + 1] = vy, out[3 * i + 2] = vz;
    }
}
extern "C" hipError_t pmcLaunchSourceVelocities(int slot, int source, const double* r, int64_t n, double* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sourceVelocityKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, slot, source, r, n, out);
    return hipGetLastError();
}

// test aids (pmc_tuning.h pmc_tune_device_function, pmc_tune_locate, pmc_tune_detector, pmc_tune_wavelength_bins, pmc_tune_angular_probabilities):
// the scalar device functions of the transition, launch and walk kernels, one lane per host-supplied argument tuple.  Every lane calls the
// function the kernels call; nothing of it is restated here.
namespace
{
    // args[n][widthIn] -> out[n][widthOut] (the widths of `function`: pmc_tuning.hip deviceFunctionWidths)
    __global__ __launch_bounds__(256) void deviceFunctionKernel(const int sceneSlot, const int function, const double* __restrict__ args, const int widthIn,
                                                                const int64_t n, double* __restrict__ out, const int widthOut)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        const double* a = args + i * widthIn;
        double* o = out + i * widthOut;
        switch (function)
        {
            case PMC_FN_HG_VALUE: o[0] = PhaseHG(a[0]).value(a[1]); break;
            case PMC_FN_HG_CONE_MEAN: o[0] = PhaseHG(a[0]).coneMean(a[1]); break;
            case PMC_FN_PHASE_VALUE: o[0] = phaseValue<false>(c_scene[sceneSlot], 0, a[0], a[1]); break;
            case PMC_FN_HG_COSINE:
                o[0] = PhaseHG::cosineFor(a[0], a[1]);
                o[1] = PhaseHG::isotropic(a[0]) ? 1. : 0.;
                break;
            case PMC_FN_DIPOLE_VALUE: o[0] = PhaseDipole::value(a[0]); break;
            case PMC_FN_RANDOM_DIRECTION: randomDirectionFor(a[0], a[1], o[0], o[1], o[2]); break;
            case PMC_FN_DIRECTION_ABOUT: directionAboutFor(a[4], a[0], a[1], a[2], a[3], o[0], o[1], o[2]); break;
            case PMC_FN_LAMBERT_LOWER_BRANCH: o[0] = lambertLowerBranch(a[0]); break;
            case PMC_FN_GENERALIZED_EXP: o[0] = generalizedExp(a[0], a[1]); break;
            case PMC_FN_INTERPOLATE_LOGLOG: o[0] = interpolateLogLog(a[0], a[1], a[2], a[3], a[4]); break;
            case PMC_FN_LNMEAN: o[0] = lnmean(a[0], a[1], a[2], a[3]); break;
            case PMC_FN_PEEL_TAUMAX: o[0] = peelTaumax(a[0], a[1]); break;
            case PMC_FN_SHIFTED_WAVELENGTH: o[0] = shiftedEmissionWavelength(a[0], a[1], a[2], a[3], a[4], a[5], a[6]); break;
            default: break;
        }
    }
    // kind 0 locate, 1 locateClip, 2 locateBasic on the table nodes[numNodes] (numNodes >= 2)
    __global__ __launch_bounds__(256) void locateKernel(const int kind, const double* __restrict__ nodes, const int numNodes, const double* __restrict__ x,
                                                        const int64_t n, int32_t* __restrict__ out)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        out[i] = kind == 0 ? locate(nodes, numNodes, x[i]) : kind == 1 ? locateClip(nodes, numNodes, x[i]) : locateBasic(nodes, x[i], numNodes);
    }
    __global__ __launch_bounds__(256) void detectorKernel(const int sceneSlot, const int instrument, const double* __restrict__ r, const int64_t n,
                                                          int32_t* __restrict__ pixel, int32_t* __restrict__ inside)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        const DevInstrument& I = c_scene[sceneSlot].inst[instrument];
        pixel[i] = pixelOnDetector(I, r[3 * i], r[3 * i + 1], r[3 * i + 2]);
        inside[i] = insideAperture(I, r[3 * i], r[3 * i + 1], r[3 * i + 2]) ? 1 : 0;
    }
    __global__ __launch_bounds__(256) void wavelengthBinKernel(const int sceneSlot, const int instrument, const double* __restrict__ lambda, const int64_t n,
                                                               int32_t* __restrict__ ell)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) ell[i] = observedBin(c_scene[sceneSlot].inst[instrument], lambda[i]);
    }
    __global__ __launch_bounds__(256) void angularProbabilityKernel(const int sceneSlot, const int source, const double* __restrict__ k, const int64_t n,
                                                                    double* __restrict__ out)
    {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) out[i] = angularProbability(c_scene[sceneSlot].src[source], k[3 * i], k[3 * i + 1], k[3 * i + 2]);
    }
    unsigned blocksFor(int64_t n) { return (unsigned)((n + 255) / 256); }
}
extern "C" hipError_t pmcLaunchDeviceFunction(int slot, int function, const double* args, int widthIn, int64_t n, double* out, int widthOut, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(deviceFunctionKernel, dim3(blocksFor(n)), dim3(256), 0, stream, slot, function, args, widthIn, n, out, widthOut);
    return hipGetLastError();
}
extern "C" hipError_t pmcLaunchLocate(int kind, const double* nodes, int numNodes, const double* x, int64_t n, int32_t* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(locateKernel, dim3(blocksFor(n)), dim3(256), 0, stream, kind, nodes, numNodes, x, n, out);
    return hipGetLastError();
}
extern "C" hipError_t pmcLaunchDetector(int slot, int instrument, const double* r, int64_t n, int32_t* pixel, int32_t* inside, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(detectorKernel, dim3(blocksFor(n)), dim3(256), 0, stream, slot, instrument, r, n, pixel, inside);
    return hipGetLastError();
}
extern "C" hipError_t pmcLaunchWavelengthBins(int slot, int instrument, const double* lambda, int64_t n, int32_t* ell, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(wavelengthBinKernel, dim3(blocksFor(n)), dim3(256), 0, stream, slot, instrument, lambda, n, ell);
    return hipGetLastError();
}
extern "C" hipError_t pmcLaunchAngularProbabilities(int slot, int source, const double* k, int64_t n, double* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(angularProbabilityKernel, dim3(blocksFor(n)), dim3(256), 0, stream, slot, source, k, n, out);
    return hipGetLastError();
}

// one ray through the grid; octree: `uniform` picks the flavour of the step the ray is traced with (direction in scalar
// registers as in the peel-off kernel, or in vector registers as in the propagation kernel; kdev = the direction in
// device memory)
extern "C" hipError_t pmcLaunchTrace(int slot, int gridKind, int wide, int uniform, const double r[3], const double k[3],
                                     const double* kdev, int32_t* m, double* ds, int32_t cap, int32_t* n, size_t ldsBytes,
                                     hipStream_t stream)
{
    const TraceKernel kernel = traceKernels[rayKernelIndex(gridKind, wide) + (gridKind == PMC_GRID_OCTREE && !uniform ? 5 : 0)].kernel;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), ldsBytes, stream, slot, r[0], r[1], r[2], k[0], k[1], k[2], kdev, m, ds, cap, n);
    return hipGetLastError();
}

// batched ray integrals (pmc_ray.inc): one pass of PMC_INTEGRATE_PASS_VALUES values over numRays rays; `work` = the kernel's cursor and counters,
// zeroed by the caller (pmcProbeWorkWords words)
extern "C" int pmcProbeWorkWords(void) { return PROBE_WORK_WORDS; }
// (averaged: the records are (w, v0, v1, v2) and the sums the raw (sum of weights, weighted sums) of pmc_integrate_weighted_rays)
extern "C" hipError_t pmcLaunchIntegrate(int slot, int gridKind, int wide, int averaged, const double* origins, const double* directions, const double* q,
                                         double* sums, unsigned long long numRays, unsigned long long* work, int grid, size_t ldsBytes, hipStream_t stream)
{
    const ProbeArgs A = {origins, directions, q, sums, numRays, work};
    const IntegrateKernel kernel = (averaged ? integrateWeightedKernels : integrateKernels)[rayKernelIndex(gridKind, wide)].kernel;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), ldsBytes, stream, slot, A);
    return hipGetLastError();
}

// the point sampler (pmc_locate.inc): the cells of numPoints positions, in the walk kernels' numbering and in the caller's ...
extern "C" hipError_t pmcLaunchLocateCells(int slot, int gridKind, int wide, const double* positions, int32_t* walkCells, int32_t* cells,
                                           unsigned long long numPoints, int grid, size_t ldsBytes, hipStream_t stream)
{
    const LocateArgs A = {positions, walkCells, cells, numPoints};
    hipLaunchKernelGGL(locateKernels[rayKernelIndex(gridKind, wide)].kernel, dim3(grid), dim3(256), ldsBytes, stream, slot, A);
    return hipGetLastError();
}
// ... and one pass of numValues <= PMC_INTEGRATE_PASS_VALUES values read at them: values [numValues][numPoints], q as for pmcLaunchIntegrate
extern "C" hipError_t pmcLaunchGatherCells(const int32_t* walkCells, const double* q, double* values, unsigned long long numPoints, int numValues, int grid,
                                           hipStream_t stream)
{
    hipLaunchKernelGGL(gatherCellsKernel, dim3(grid), dim3(256), 0, stream, walkCells, q, values, numPoints, numValues);
    return hipGetLastError();
}
