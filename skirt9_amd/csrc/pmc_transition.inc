// pmc_transition.inc -- the transition kernel (included by pmc_kernels.hip inside its anonymous namespace).
//
// One lane per packet slot.  A lane consumes the result of the walk that just ended in its slot and performs the
// part of the life cycle between two walks (MonteCarloSimulation.cpp:538-613), leaving the next walk task in the
// slot -- or launching the next history when the current one ends.  Slot fields are read and written lazily, only
// those an event needs (the slot arrays are a struct of arrays, so every access is coalesced across the wave).
//
//   peel-off done   FluxRecorder::detect with the optical depth found by the walk; next observer, or start of the
//                   photon cycle (emission) / scattering event (DustMix::performScattering) and the next pass-1 walk
//   pass 1 done     simulateForcedPropagation: sample tau from tau_path, start pass 2
//   pass 2 done     interaction: albedo and escape weights, propagate, termination test, scattering peel-off
//   launch          flush the per-history statistics, SourceSystem::launch, emission peel-off
//
// This file: the pieces that the transition and launch kernels share (the LDS carve-up and its staging, the workgroup's
// epilogue, the counters), onCycleDone, the transition kernel in its four flavours, and endedScanKernel, which turns the
// transition kernel's counts of ended histories into the launch kernel's history indices.  The launch kernel itself is in
// pmc_launch.inc; what a cycle starts with in pmc_cycle.inc, detection and statistics in pmc_detect.inc, the phase functions and
// sampling primitives in pmc_phase.inc.

    // ================================================================================================
    //  shared pieces of the transition and launch kernels
    // ================================================================================================

    // LDS carve-up of the transition and launch kernels (DevScene::lds_*): privatised SED blocks, hot-bin table, integer scratch
    // for the per-wave slot lists; launch kernel: source and dust tables behind them.  (Neither kernel touches the grid: the
    // walks of a cycle are started by cycleStartKernel, which stages the grid tables.)
    struct BlockLds
    {
        DustLds L;
        int* sortSlot;                // the waves' lists of slots: [waves][256] slot indices, then [waves][256] mode words (DevScene::lds_sort_off
                                      // reserves 64 + 2 * 1024 + 8 integers)
    };

    // LAUNCH: the launch kernel also stages what only the launch of a history reads -- the Sersic tables and the index
    // borders of the dust mix, where the wavelength of every new history is located (DustMix::indexForLambda, a binary
    // search: eleven dependent reads of a 2102-point table); the cross sections and the asymmetry parameter of the bin found
    // are read once and travel in the slot (SlotArrays::dustExt ...), so the transition kernel needs no dust table at all
    template<bool LAUNCH> __device__ __forceinline__ void stageBlock(const DevScene& S, double* lds, int tid, int nthreads, BlockLds& B)
    {
        if (LAUNCH && S.dust_in_lds)
        {
            double* d = lds + S.lds_dust_off;
            for (int i = tid; i < S.num_lambda; i += nthreads) d[i] = S.lambda_border[i];
        }
        if (LAUNCH && S.num_sources == 1 && S.src[0].source_kind == PMC_SOURCE_SERSIC)
        {
            const DevSource& Q = S.src[0];
            double* sv = lds + S.lds_src_off;
            for (int i = tid; i < Q.sersic_n; i += nthreads)
            {
                sv[i] = Q.sersic_s[i];
                sv[Q.sersic_n + i] = Q.sersic_M[i];
            }
        }
        double* sed = lds + S.lds_sed_off;
        for (int i = tid; i < S.lds_sed_len; i += nthreads) sed[i] = 0.;
        DustLds& L = B.L;
        L.hotKey = reinterpret_cast<unsigned long long*>(lds + S.lds_hot_off);
        L.hotVal = lds + S.lds_hot_off + HOT_BINS;
        for (int i = tid; i < HOT_BINS; i += nthreads)
        {
            L.hotKey[i] = 0ull;
            L.hotVal[i] = 0.;
        }
        L.lamb = (LAUNCH && S.dust_in_lds) ? lds + S.lds_dust_off : S.lambda_border;
        L.sext = S.sigma_ext;
        L.ssca = S.sigma_sca;
        L.asym = S.asymmpar;
        L.src = lds + S.lds_src_off;
        L.sed = sed;
        int* ints = reinterpret_cast<int*>(lds + S.lds_sort_off);
        B.sortSlot = ints + 64;
        __syncthreads();
    }

    // workgroup epilogue: privatised SED blocks and hot bins go to HBM
    __device__ __forceinline__ void flushBlock(const DevScene& S, const DustLds& L, int tid, int nthreads)
    {
        __syncthreads();
        for (int i = 0; i < S.num_instruments; ++i)
        {
            const DevInstrument& I = S.inst[i];
            if (!I.include_sed) continue;
            const double* sed = L.sed + I.sed_lds_offset;
            const int nflux = I.num_components * I.num_lambda;
            for (int q = tid; q < nflux; q += nthreads)
                if (sed[q] != 0.) unsafeAtomicAdd(S.frames + I.sed_offset + q, sed[q]);
            if (I.record_stats)
                for (int q = tid; q < 5 * I.num_lambda; q += nthreads)
                    if (sed[nflux + q] != 0.) unsafeAtomicAdd(S.frames + I.wsed_offset + q, sed[nflux + q]);
        }
        for (int i = tid; i < HOT_BINS; i += nthreads)
            if (L.hotKey[i] != 0ull && L.hotVal[i] != 0.) unsafeAtomicAdd(S.frames + (int64_t)(L.hotKey[i] - 1ull), L.hotVal[i]);
    }

    __device__ __forceinline__ void addCounters(const DevScene& S, const Counters& cnt, int lane)
    {
        unsigned long long v;
        v = waveSum(cnt.histories);
        if (lane == 0 && v) atomicAdd(S.counters + 0, v);
        v = waveSum(cnt.paths);
        if (lane == 0 && v) atomicAdd(S.counters + 1, v);
        v = waveSum(cnt.updates);
        if (lane == 0 && v) atomicAdd(S.counters + 3, v);
        v = waveSum(cnt.scatterings);
        if (lane == 0 && v) atomicAdd(S.counters + 4, v);
        v = waveSum(cnt.overflows);
        if (lane == 0 && v) atomicAdd(S.counters + 5, v);
    }

    // ---- a cycle is done: detections of its peel-offs (FluxRecorder::detect with the optical depths the walks found),
    //      then the interaction the propagation walk found (MonteCarloSimulation.cpp:724-741 / 746-780): albedo and
    //      escape weights, termination test, scattering (DustMix::performScattering, HG), and the next cycle.
    //      All slot loads are issued as one batch first.
    template<bool DIPOLE, bool KIN = false>
    __device__ __forceinline__ int onCycleDone(const DevScene& S, const DustLds& L, Counters& cnt, int slot, int modeWord, uint64_t seed, int group)
    {
        const SlotArrays& A = S.slots;
        const int64_t NS = A.num_slots;
        const double rx0 = A.rx[slot], ry0 = A.ry[slot], rz0 = A.rz[slot];
        const double kx = A.kx[slot], ky = A.ky[slot], kz = A.kz[slot];
        const double lambda = S.mono ? S.mono_lambda : A.lambda[slot];
        const double W0 = A.W[slot];
        const double ssca = S.mono ? S.mono_sca : A.dustSca[slot], sext = S.mono ? S.mono_ext : A.dustExt[slot];
        const double asym = S.mono ? S.mono_asym : A.dustAsym[slot];
        const int nscatt = A.nscatt[slot];
        const int pscatt = nscatt;  // numScatt of the cycle's peel-off packets (PhotonPacket::launchScatteringPeelOff: 0 for emission)
        const int mint = A.mint[slot];
        const double nint = A.nint[slot];
        const double sint = A.sint[slot];
        const double taupath = A.taupath[slot];
        const double Lthreshold = A.Lthreshold[slot];
        Rng rng;
        loadRng(A, slot, rng);
        // ---- 1. the peel-off packets of this cycle, in instrument order; instruments that share the observer reuse the
        //         optical depth (FluxRecorder.cpp:329-338)
        const uint32_t pmask = ((uint32_t)modeWord >> 8) & 0xFFFFu;
        for (int g = 0; g < S.num_instruments; ++g)
        {
            if (!((pmask >> g) & 1u)) continue;
            // (KIN, emission cycle: the packet towards this observer has its own wavelength and cross section -- startCycleWalks)
            const bool emission = KIN && pscatt == 0;
            const double Lum = A.ppW[(int64_t)g * NS + slot] / (emission ? A.obsLambda[(int64_t)g * NS + slot] : lambda);
            double tau = A.ptau[(int64_t)g * NS + slot];
            if (emission)
            {
                const double sobs = A.obsExt[(int64_t)g * NS + slot];
                if (sobs != sext && tau != INFINITY) tau = tau * (sobs / sext);
            }
            int inst = g;
            do
            {
                detect<KIN>(S, L, cnt, inst, slot, rx0, ry0, rz0, Lum, tau, pscatt, group, emission);
                ++inst;
            } while (inst < S.num_instruments && S.inst[inst].same_observer);
        }
        PMC_T_STAMP(4);
        // ---- 2. the propagation result: no interaction => the history ends (tau_path <= 0, MonteCarloSimulation.cpp:709;
        //         non-forced: the packet escaped)
        if (mint < 0) return EV_LAUNCH;
        // MediumSystem::albedoForScattering (MediumSystem.cpp:678-693); in the explicit-absorption cycle the walk left the cumulative
        // absorption optical depth at the interaction point in `nint`, and exp(-tau_abs) takes the albedo's place
        // (MonteCarloSimulation.cpp:729-733, 758-766)
        double ksca = nint > 0. ? nint * ssca : 0.;
        double kext = nint > 0. ? nint * sext : 0.;
        // several components: the opacities of all of them in the interaction cell (MediumSystem.cpp:678-693, 697-730)
        const bool multi = S.num_media > 1;
        double shares[PMC_MAX_MEDIA] = {0., 0., 0., 0.}, asyms[PMC_MAX_MEDIA] = {0., 0., 0., 0.};
        if (multi)
        {
            ksca = 0., kext = 0.;
            for (int h = 0; h < S.num_media; ++h)
            {
                const DevMedium& M = S.med[h];
                const double n = M.density[mint];
                double ex, sc, ab;
                mediumSections(S, A, slot, h, ex, sc, ab);
                asyms[h] = S.mono ? M.mono_asym : M.asymmpar[A.dustIdx[(int64_t)h * NS + slot]];
                shares[h] = n > 0. ? n * sc : 0.;
                ksca += shares[h];
                kext += n > 0. ? n * ex : 0.;
            }
        }
        const double albedo = S.explicit_absorption ? exp(-nint) : kext > 0. ? ksca / kext : 0.;
        double W = W0;
        if (S.force_scattering)
        {
            // simulateForcedPropagation (MonteCarloSimulation.cpp:709-741): the path-length-bias weight of the interaction
            // optical depth the walk kernel sampled between the passes, then escape probability and albedo
            const double xi = S.path_length_bias;
            const double em1 = expm1(-taupath);
            if (xi != 0.)
            {
                const double pp = -exp(-A.tausample[slot]) / em1;
                const double q = (1.0 - xi) * pp + xi / taupath;
                W = W * (pp / q);
            }
            W *= (-em1 * albedo);
        }
        else
            W *= albedo;
        const double rx = rx0 + sint * kx, ry = ry0 + sint * ky, rz = rz0 + sint * kz;
        const double lum = W / lambda;
        const bool terminate = S.force_scattering ? (lum <= 0 || (lum <= Lthreshold && nscatt >= S.min_scatt_events)) : (lum <= 0);
        if (terminate) return EV_LAUNCH;
        A.rx[slot] = rx;
        A.ry[slot] = ry;
        A.rz[slot] = rz;
        A.W[slot] = W;
        // ---- 3. scattering: new direction (DustMix.cpp:490-511 with Random::direction(bfk, costheta), Random.cpp:130-164);
        //         the peel-off packets of the next cycle use the incoming direction
        double kxn, kyn, kzn;
        {
            double g = asym;
            int scatterer = 0;
            if (multi)
            {
                // the scattering component: ONE uniform deviate against the cumulative distribution of the components' scattering
                // opacities (MediumSystem.cpp:806-817, NR::cdf, Random::uniform, NR::locateClip)
                double X[PMC_MAX_MEDIA + 1];
                X[0] = 0.;
                for (int h = 0; h < S.num_media; ++h) X[h + 1] = X[h] + shares[h];
                const double norm = X[S.num_media];
                for (int h = 0; h <= S.num_media; ++h) X[h] /= norm;
                scatterer = locateClip(X, S.num_media + 1, rngUniform(rng, seed));
                g = asyms[scatterer];
            }
            if (DIPOLE && S.phase_kind[scatterer] == PMC_PHASE_DIPOLE)
            {
                // DipolePhaseFunction::performScattering (DipolePhaseFunction.cpp:164-172): ONE uniform deviate for the cosine, then
                // Random::direction(bfk, costheta) with one more
                const double costheta = PhaseDipole::cosineFor(rngUniform(rng, seed));
                directionAbout(rng, seed, kx, ky, kz, costheta, kxn, kyn, kzn);
            }
            else if (PhaseHG::isotropic(g))
                randomDirection(rng, seed, kxn, kyn, kzn);
            else
            {
                const double costheta = PhaseHG::cosineFor(g, rngUniform(rng, seed));
                directionAbout(rng, seed, kx, ky, kz, costheta, kxn, kyn, kzn);
            }
        }
        A.kx[slot] = kxn, A.ky[slot] = kyn, A.kz[slot] = kzn;
        A.nscatt[slot] = nscatt + 1;
        cnt.scatterings += 1;
        PMC_T_STAMP(5);
        if (multi)
        {
            // (MediumSystem::weightsForScattering: no peel-off packets at all from a cell in which no component scatters)
            const bool some = ksca > 0.;
            for (int h = 0; h < S.num_media; ++h) shares[h] = some ? shares[h] / ksca : 0.;
            announceCycle<DIPOLE>(S, slot, seed, rng, rx, ry, rz, kx, ky, kz, W, asym, nscatt + 1, shares, asyms);
        }
        else
            announceCycle<DIPOLE>(S, slot, seed, rng, rx, ry, rz, kx, ky, kz, W, asym, nscatt + 1);
        PMC_T_STAMP(6);
        storeRng(A, slot, rng);
        return EV_TASK;
    }

    // ================================================================================================
    //  transition kernel: one lane per slot of the group [slotBase, slotBase + numSlots)
    // ================================================================================================
    //  DIPOLE: the flavour of a scene in which some medium component has the dipole phase function (transitionDipoleKernel); every other
    //  scene runs transitionKernel, which holds no trace of it
    //  KIN: the flavour of a scene with a moving source (transitionKinKernel, transitionKinDipoleKernel)
    template<bool DIPOLE, bool KIN = false>
    __device__ __forceinline__ void transitionBody(const int sceneSlot, const int slotBase, const int numSlots, const int group, const uint64_t seed,
                                                   const int* const list, const int listLen, const StatLogArgs& statLog)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        BlockLds B;
        Counters cnt = {0, 0, 0, 0, 0};
        StatLogWave logWave = statLogBegin(statLog);
        PMC_T_PROF_BEGIN;
        stageBlock<false>(S, lds, tid, blockDim.x, B);
        PMC_T_STAMP(0);
        const DustLds& L = B.L;
        const SlotArrays& A = S.slots;

        uint32_t liveCount = 0;
        // persistent workgroups: the tables are staged once, the privatised SED blocks and hot bins are flushed once.  Every
        // WAVE serves runs of 256 slots (four wave tiles) and works through the live ones in its own compacted list, 64 at a
        // time: with all slots alive that is the slot order itself; while a segment drains (a third of its generations) the
        // kernel's time follows the number of live slots instead of the size of the pool.
        // A sparse generation (the end of a segment: no history is left to launch; `list` = the listLen live slots of the group,
        // TaskArrays::liveList) runs over the list, 64 entries per wave at a time, and retires the histories that end here itself --
        // statistics flush, slot dead -- so that neither the scan nor the launch kernel runs.
        const int wv = tid >> 6;
        const int perWave = list ? 64 : 256;
        const int span = perWave * ((int)blockDim.x >> 6);
        const int slotEnd = slotBase + numSlots;
        int* const myList = B.sortSlot + wv * 256;
        int* const myMode = B.sortSlot + 1024 + wv * 256;
        const unsigned long long below = (1ull << lane) - 1ull;
        const int numTiles = ((list ? listLen : numSlots) + span - 1) / span;
        for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
        {
            const int wbase = slotBase + tile * span + wv * 256;
            int n = 0;
            if (list)
            {
                const int at = tile * span + wv * 64;
                if (at >= listLen) continue;
                n = min(64, listLen - at);
                if (lane < n)
                {
                    const int s = list[at + lane];
                    myList[lane] = s;
                    myMode[lane] = A.mode[s];
                }
            }
            else
            {
                if (wbase >= slotEnd) continue;
                int md[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    const int s0 = wbase + 64 * j + lane;
                    md[j] = s0 < slotEnd ? A.mode[s0] : 0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    const bool alive = (md[j] & MODE_ALIVE) != 0;
                    const unsigned long long m = __ballot(alive);
                    if (alive)
                    {
                        const int at = n + __popcll(m & below);
                        myList[at] = (int)((uint32_t)(wbase + 64 * j + lane) | ((uint32_t)j << 30));
                        myMode[at] = md[j];
                    }
                    n += __popcll(m);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            PMC_T_STAMP(1);
            uint32_t endedOf[4] = {0u, 0u, 0u, 0u};  // histories that ended, per wave tile of the run (wave-uniform)
            for (int c = 0; c < n; c += 64)
            {
                int event = EV_NONE;
                int slot = -1, sub = 0;
                if (c + lane < n)
                {
                    const int entry = myList[c + lane];
                    slot = entry & 0x3FFFFFFF;
                    sub = (int)((unsigned)entry >> 30);
                    event = onCycleDone<DIPOLE, KIN>(S, L, cnt, slot, myMode[c + lane], seed, group);
                }
                PMC_T_STAMP(2);
                if (list)
                {
                    // the history has ended and none is left to take its slot (SourceSystem has handed out all indices): its statistics
                    // are flushed here and the slot dies
                    if (S.any_stats) flushStatistics<KIN>(S, L, cnt, slot, event == EV_LAUNCH, lane, group, false, statLog, logWave);
                    if (event == EV_LAUNCH)
                    {
                        A.mode[slot] = MODE_NONE;
                        for (int r = 0; r <= S.num_instruments; ++r) S.tasks.bits[(int64_t)r * A.num_slots + slot] = PMC_TASK_NONE;
                    }
                }
                else
                {
                    // the history has ended: the slot is marked for the launch kernel (statistics flush, next history)
                    if (event == EV_LAUNCH) A.mode[slot] = MODE_ENDED;
#pragma unroll
                    for (int j = 0; j < 4; ++j) endedOf[j] += (uint32_t)__popcll(__ballot(event == EV_LAUNCH && sub == j));
                }
                if (event == EV_TASK) liveCount += 1;
                PMC_T_STAMP(3);
            }
            // the run's counts of ended histories, per wave tile, for the scan that assigns the next history indices
            if (!list && lane < 4 && wbase + 64 * lane < slotEnd)
                S.tasks.endedCount[(wbase >> 6) + lane] = lane == 0 ? endedOf[0] : lane == 1 ? endedOf[1] : lane == 2 ? endedOf[2] : endedOf[3];
            // (the list is rewritten in the next round only after every lane has read its entries)
            __builtin_amdgcn_wave_barrier();
        }
        {
            const unsigned long long live = waveSum(liveCount);
            if (lane == 0 && live) atomicAdd(S.counters + PMC_CTR_LIVE(group), live);
        }
        statLogEnd(statLog, logWave, lane);
        flushBlock(S, L, tid, blockDim.x);
        PMC_T_STAMP(7);
        PMC_T_PROF_END(192);
        addCounters(S, cnt, lane);
    }
    __global__ __launch_bounds__(PMC_TRANSITION_BLOCK, PMC_TRANSITION_MIN_WAVES) void transitionKernel(const int sceneSlot, const int slotBase, const int numSlots,
                                                            const int group, const uint64_t seed, const int* const list, const int listLen,
                                                            const StatLogArgs statLog)
    {
        transitionBody<false>(sceneSlot, slotBase, numSlots, group, seed, list, listLen, statLog);
    }
    __global__ __launch_bounds__(PMC_TRANSITION_BLOCK, PMC_TRANSITION_MIN_WAVES) void transitionDipoleKernel(const int sceneSlot, const int slotBase,
                                                            const int numSlots, const int group, const uint64_t seed, const int* const list,
                                                            const int listLen, const StatLogArgs statLog)
    {
        transitionBody<true>(sceneSlot, slotBase, numSlots, group, seed, list, listLen, statLog);
    }
    __global__ __launch_bounds__(PMC_TRANSITION_BLOCK, PMC_TRANSITION_MIN_WAVES) void transitionKinKernel(const int sceneSlot, const int slotBase, const int numSlots,
                                                            const int group, const uint64_t seed, const int* const list, const int listLen,
                                                            const StatLogArgs statLog)
    {
        transitionBody<false, true>(sceneSlot, slotBase, numSlots, group, seed, list, listLen, statLog);
    }
    __global__ __launch_bounds__(PMC_TRANSITION_BLOCK, PMC_TRANSITION_MIN_WAVES) void transitionKinDipoleKernel(const int sceneSlot, const int slotBase,
                                                            const int numSlots, const int group, const uint64_t seed, const int* const list,
                                                            const int listLen, const StatLogArgs statLog)
    {
        transitionBody<true, true>(sceneSlot, slotBase, numSlots, group, seed, list, listLen, statLog);
    }

    // ================================================================================================
    //  scan of the ended-history counts of one slot group: endedCount[tile] becomes the number of ended histories in the
    //  tiles before it, and the group reserves that many history indices from the global cursor (PMC_CTR_HBASE).  The
    //  history a slot takes up next is then a pure function of the slot order: no list, no atomics in the launch kernel.
    //  One workgroup of PMC_SCAN_THREADS lanes (four waves of few registers: it finds room on a CU next to a resident propagation workgroup
    //  of another slot group, which a workgroup of 1024 lanes does not -- it then waits for a free CU, 1.3 ms on average with the groups
    //  overlapped, profiles/r05_v3_kernel_stats.csv); the group has at most 2^30 / 64 tiles.
    // ================================================================================================
    //  What a group may take this generation: [HBASE, HLIMIT), HLIMIT = `count`.
    __global__ __launch_bounds__(PMC_SCAN_THREADS) void endedScanKernel(const int sceneSlot, const int slotBase, const int numSlots, const int group,
                                                                        const unsigned long long count)
    {
        const DevScene& S = c_scene[sceneSlot];
        __shared__ unsigned int part[PMC_SCAN_THREADS];
        const int tid = threadIdx.x;
        uint32_t* counts = S.tasks.endedCount + (slotBase >> 6);
        const int n = (numSlots + 63) >> 6;
        const int chunk = (((n + PMC_SCAN_THREADS - 1) / PMC_SCAN_THREADS) + 3) & ~3;  // entries per lane, a multiple of 4 (16-byte accesses)
        const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
        unsigned int sum = 0;
        for (int i = lo; i < hi; i += 4)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(counts + i);  // (the array is padded: a read past n stays inside)
            sum += v.x + (i + 1 < hi ? v.y : 0u) + (i + 2 < hi ? v.z : 0u) + (i + 3 < hi ? v.w : 0u);
        }
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < PMC_SCAN_THREADS; off <<= 1)
        {
            const unsigned int add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        unsigned int run = part[tid] - sum;  // exclusive prefix of this lane's chunk
        if (tid == PMC_SCAN_THREADS - 1)
        {
            const unsigned long long ended = (unsigned long long)part[PMC_SCAN_THREADS - 1];
            // (the cursor may run past `count`: the launch kernel stops at it)
            S.counters[PMC_CTR_HBASE(group)] = atomicAdd(S.counters + PMC_CTR_HISTORY, ended);
            S.counters[PMC_CTR_HLIMIT(group)] = count;
        }
        for (int i = lo; i < hi; i += 4)
        {
            uint4 v = *reinterpret_cast<const uint4*>(counts + i);
            uint4 o;
            o.x = run, run += v.x;
            o.y = run, run += v.y;
            o.z = run, run += v.z;
            o.w = run, run += v.w;
            *reinterpret_cast<uint4*>(counts + i) = o;
        }
    }
