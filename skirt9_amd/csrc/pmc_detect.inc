// pmc_detect.inc -- detection and the per-history statistics (included by pmc_kernels.hip inside its anonymous namespace).
//
// FluxRecorder::detect for one peel-off packet (transition kernel), the list of a history's contributions that it fills, and
// flushStatistics, which turns the list into powers when the history ends (launch kernel; transition kernel in a sparse
// generation), through the wave's statistics log or atomics; statMergeKernel adds the accumulator to the frames at the end of a
// segment.  Also the workgroup's counters and the section timers of profiling builds (PMC_T_*), which every transition-side
// function takes along.
//
// Detector updates: SED bins are privatised per workgroup in LDS.  IFU/statistics bins go through a small
// claim-once hot-bin table in LDS (a point source or a galaxy nucleus sends a large share of all contributions to a
// few bins; one device-scope f64 atomic per contribution on the same address would serialise at ~1e8/s) and are
// flushed with one global_atomic_add_f64 per claimed bin at the end of the workgroup; misses go to HBM directly.

    struct DustLds
    {
        const double* lamb;            // launch kernel: index borders of the dust mix (LDS when they fit), and its properties
        const double* sext;
        const double* ssca;
        const double* asym;
        const double* src;             // launch kernel: Sersic s | M
        double* sed;                   // privatised SED blocks
        unsigned long long* hotKey;    // hot-bin table: frame offset + 1, or 0 = free
        double* hotVal;
    };
    constexpr int HOT_BINS = 256;

    struct Counters
    {
        uint32_t histories, paths, updates, scatterings, overflows;
#ifdef PMC_PROFILE
        long long tp[8];  // section timers (wave cycles), see PMC_T_STAMP
        long long tl;
#endif
    };

#ifdef PMC_PROFILE
    // section timers of the transition / launch kernels (profiling builds): wave cycles per section, summed by lane 0
    #define PMC_T_PROF_BEGIN cnt.tl = clock64()
    #define PMC_T_STAMP(i)                     \
        do                                     \
        {                                      \
            const long long now_ = clock64();  \
            cnt.tp[i] += now_ - cnt.tl;        \
            cnt.tl = now_;                     \
        } while (0)
    #define PMC_T_PROF_END(base)                                                                             \
        do                                                                                                   \
        {                                                                                                    \
            if (lane == 0)                                                                                   \
                for (int i_ = 0; i_ < 8; ++i_) atomicAdd(S.counters + (base) + i_, (unsigned long long)cnt.tp[i_]); \
        } while (0)
#else
    #define PMC_T_PROF_BEGIN
    #define PMC_T_STAMP(i)
    #define PMC_T_PROF_END(base)
#endif

    // accumulate into a detector bin: hot-bin table in LDS first (claim once per workgroup), HBM otherwise
    __device__ __forceinline__ void frameAdd(const DevScene& S, const DustLds& L, int64_t offset, double value)
    {
        const unsigned long long key = (unsigned long long)offset + 1ull;
        const int h = (int)((key * 0x9E3779B97F4A7C15ull) >> 56);  // 8 bits
        unsigned long long k = L.hotKey[h];
        if (k == 0ull) k = atomicCAS(&L.hotKey[h], 0ull, key);
        if (k == 0ull || k == key)
            atomicAdd(&L.hotVal[h], value);
        else
            unsafeAtomicAdd(S.frames + offset, value);
    }

    // FrameInstrument::pixelOnDetector (FrameInstrument.cpp:45-65)
    __device__ __forceinline__ int pixelOnDetector(const DevInstrument& I, double x, double y, double z)
    {
        double xpp = -I.sinphi * x + I.cosphi * y;
        double ypp = -I.cosphi * I.costheta * x - I.sinphi * I.costheta * y + I.sintheta * z;
        double xp = I.cosomega * xpp - I.sinomega * ypp;
        double yp = I.sinomega * xpp + I.cosomega * ypp;
        int i = (int)floor((xp - I.xpmin) / I.xpsiz);
        int j = (int)floor((yp - I.ypmin) / I.ypsiz);
        if (i < 0 || i >= I.nxp || j < 0 || j >= I.nyp) return -1;
        return i + I.nxp * j;
    }

    // ApertureInstrument::isInsideAperture (ApertureInstrument.cpp:22-43)
    __device__ __forceinline__ bool insideAperture(const DevInstrument& I, double x, double y, double z)
    {
        if (I.aperture_r2 == 0.) return true;
        double xpp = -I.sinphi * x + I.cosphi * y;
        double ypp = -I.cosphi * I.costheta * x - I.sinphi * I.costheta * y + I.sintheta * z;
        double radius2 = xpp * xpp + ypp * ypp;
        return !(radius2 > I.aperture_r2);
    }

    // FluxRecorder::detect for one peel-off packet whose optical depth is known (FluxRecorder.cpp:304-468)
    // one more block for a contribution list from the pool of slot group `group`, or -1 if the pool is empty
    __device__ __forceinline__ int statBlockTake(const DevScene& S, int group)
    {
        unsigned long long* nfree = S.counters + PMC_CTR_STATFREE(group);
        const long long pos = (long long)atomicAdd(nfree, ~0ull) - 1ll;  // (free count - 1)
        if (pos < 0)
        {
            atomicAdd(nfree, 1ull);
            return -1;
        }
        const int b = S.stat_pool_free[S.stat_pool_first[group] + (int)pos];
        S.stat_pool_next[b] = -1;
        return b;
    }
    __device__ __forceinline__ void statBlockReturn(const DevScene& S, int group, int block)
    {
        const unsigned long long pos = atomicAdd(S.counters + PMC_CTR_STATFREE(group), 1ull);
        S.stat_pool_free[S.stat_pool_first[group] + (int)pos] = block;
    }

    // KIN (a scene with a moving source): `emission` = the packet is an emission peel-off packet, whose wavelength bin is the observer's own
    // (SlotArrays::obsEll); a history can then contribute to TWO wavelength bins of an instrument, and the list entry of an emission
    // contribution to another bin than the packet's carries PMC_STAT_EMISSION_BIN on top of its pixel (flushStatistics)
    template<bool KIN = false>
    __device__ __forceinline__ void detect(const DevScene& S, const DustLds& L, Counters& cnt, int inst, int slot, double rx,
                                           double ry, double rz, double Lum, double tau, int numScatt, int group, bool emission = false)
    {
        const DevInstrument& I = S.inst[inst];
        const SlotArrays& A = S.slots;
        // the head record of the history's contribution list (requested first: it arrives with the slot's other state)
        const int64_t ni = (int64_t)inst * A.num_slots + slot;
        char* const head = reinterpret_cast<char*>(A.statHead) + ni * 64;
        int4 headBin = make_int4(-1, -1, -1, -1);
        double2 headW01 = make_double2(0., 0.), headW23 = make_double2(0., 0.);
        int2 headN = make_int2(0, -1);
        // (an emission peel-off is the first contribution of its history: the list is empty, as the launch kernel left it)
        if (I.record_stats && numScatt > 0)
        {
            headBin = *reinterpret_cast<const int4*>(head);
            headW01 = *reinterpret_cast<const double2*>(head + 16);
            headW23 = *reinterpret_cast<const double2*>(head + 32);
            headN = *reinterpret_cast<const int2*>(head + 48);
        }
        int l = pixelOnDetector(I, rx, ry, rz);
        if (!I.include_sed && l < 0) return;
        if (!insideAperture(I, rx, ry, rz)) return;
        const int ell = (KIN && emission) ? A.obsEll[ni] : S.mono ? I.mono_ell : A.ell[(int64_t)inst * A.num_slots + slot];
        if (ell < 0) return;
        const int pixel = l;
        // (the key of the contribution in the history's list: the pixel, or for an emission contribution to a bin of its own the marked pixel)
        if (KIN && emission && I.record_stats && ell != A.ell[ni]) l = pixel + PMC_STAT_EMISSION_BIN;
        const double Lext = Lum * exp(-tau);
        if (I.include_sed)
        {
            double* sed = L.sed + I.sed_lds_offset;
            const int nl = I.num_lambda;
            if (!I.record_components)
                atomicAdd(&sed[ell], Lext);
            else if (numScatt == 0)
            {
                atomicAdd(&sed[0 * nl + ell], Lum);
                atomicAdd(&sed[1 * nl + ell], Lext);
            }
            else
            {
                atomicAdd(&sed[2 * nl + ell], Lext);
                if (numScatt <= I.num_levels) atomicAdd(&sed[(3 + numScatt - 1) * nl + ell], Lext);
            }
        }
        if (I.include_ifu && pixel >= 0)
        {
            const int64_t len = I.npix * I.num_lambda;
            const int64_t at = I.ifu_offset + pixel + (int64_t)ell * I.npix;
            if (!I.record_components)
            {
                frameAdd(S, L, at, Lext);
                cnt.updates += 1;
            }
            else if (numScatt == 0)
            {
                frameAdd(S, L, at, Lum);
                frameAdd(S, L, at + len, Lext);
                cnt.updates += 2;
            }
            else
            {
                frameAdd(S, L, at + 2 * len, Lext);
                cnt.updates += 1;
                if (numScatt <= I.num_levels)
                {
                    frameAdd(S, L, at + (3 + numScatt - 1) * len, Lext);
                    cnt.updates += 1;
                }
            }
        }
        if (I.record_stats)
        {
            // The list of a history holds ONE entry per distinct bin: a contribution to a bin that is already listed is added
            // to that entry (FluxRecorder.cpp:962-1014 sums the contributions of a history to the same bin before it takes
            // the powers), so that the flush at the end of the history is linear in the list length.  Entries 0-3 live in the
            // head record, 4 .. PMC_STAT_CAP - 1 in the slot's own list, the rest in chained blocks of the group's pool.
            const int nword = headN.x;
            const int n = nword & ~PMC_STAT_POOL_EXHAUSTED;
            const int inHead = n < 4 ? n : 4;
            int k = -1;
            if (inHead > 0 && headBin.x == l) k = 0;
            if (inHead > 1 && headBin.y == l) k = 1;
            if (inHead > 2 && headBin.z == l) k = 2;
            if (inHead > 3 && headBin.w == l) k = 3;
            if (k >= 0)
            {
                const double w = k == 0 ? headW01.x : k == 1 ? headW01.y : k == 2 ? headW23.x : headW23.y;
                *reinterpret_cast<double*>(head + 16 + 8 * k) = w + Lext;
            }
            else if (n < 4)
            {
                *reinterpret_cast<int*>(head + 4 * n) = l;
                *reinterpret_cast<double*>(head + 16 + 8 * n) = Lext;
                *reinterpret_cast<int*>(head + 48) = nword + 1;
            }
            else
            {
                // slot-major list: the entries of one history are contiguous (16-byte aligned: PMC_STAT_CAP is a multiple of 4)
                const int64_t base = ni * PMC_STAT_CAP;
                const int listed = n < PMC_STAT_CAP ? n : PMC_STAT_CAP;
                int found = -1;
                for (int q = 4; q < listed; q += 4)
                {
                    const int4 b = *reinterpret_cast<const int4*>(A.statBin + base + q);
                    if (b.x == l) found = q;
                    if (b.y == l && q + 1 < listed) found = q + 1;
                    if (b.z == l && q + 2 < listed) found = q + 2;
                    if (b.w == l && q + 3 < listed) found = q + 3;
                }
                if (found >= 0)
                    A.statW[base + found] += Lext;
                else if (n < PMC_STAT_CAP)
                {
                    A.statBin[base + n] = l;
                    A.statW[base + n] = Lext;
                    *reinterpret_cast<int*>(head + 48) = nword + 1;
                }
                else
                {
                    // the list continues in chained blocks of the group's pool (FluxRecorder's list is unbounded,
                    // FluxRecorder.hpp:327-338): entries PMC_STAT_CAP, PMC_STAT_CAP + 1, ... in block order
                    const int chained = n - PMC_STAT_CAP;
                    int block = chained > 0 ? headN.y : -1, last = -1;
                    bool added = false;
                    for (int seen = 0; seen < chained && !added; seen += PMC_STAT_CAP)
                    {
                        const int here = chained - seen < PMC_STAT_CAP ? chained - seen : PMC_STAT_CAP;
                        const int64_t at = (int64_t)block * PMC_STAT_CAP;
                        for (int q = 0; q < here; q += 4)
                        {
                            const int4 b = *reinterpret_cast<const int4*>(S.stat_pool_bin + at + q);
                            int hit = -1;
                            if (b.x == l) hit = q;
                            if (b.y == l && q + 1 < here) hit = q + 1;
                            if (b.z == l && q + 2 < here) hit = q + 2;
                            if (b.w == l && q + 3 < here) hit = q + 3;
                            if (hit >= 0)
                            {
                                S.stat_pool_w[at + hit] += Lext;
                                added = true;
                                break;
                            }
                        }
                        last = block;
                        if (!added && seen + PMC_STAT_CAP < chained) block = S.stat_pool_next[block];
                    }
                    if (!added)
                    {
                        const int q = chained % PMC_STAT_CAP;
                        if (q == 0)
                        {
                            // every block so far is full: one more
                            block = statBlockTake(S, group);
                            if (block >= 0)
                            {
                                if (last < 0)
                                    *reinterpret_cast<int*>(head + 52) = block;
                                else
                                    S.stat_pool_next[last] = block;
                            }
                        }
                        else
                            block = last;
                        if (block >= 0)
                        {
                            S.stat_pool_bin[(int64_t)block * PMC_STAT_CAP + q] = l;
                            S.stat_pool_w[(int64_t)block * PMC_STAT_CAP + q] = Lext;
                            *reinterpret_cast<int*>(head + 48) = nword + 1;
                        }
                        else
                            *reinterpret_cast<int*>(head + 48) = nword | PMC_STAT_POOL_EXHAUSTED;  // the contribution is lost: reported by the launch kernel
                    }
                }
            }
        }
    }

    // FluxRecorder::recordContributions for the history that just ended (FluxRecorder.cpp:962-1014): the powers of the
    // history's summed contribution to every bin.  All contributions of a history share the wavelength bin; the list holds
    // one entry per distinct pixel (see detect), so the flush is one pass over the list, one lane per history.  The five
    // powers of an entry go to ONE 64-byte record of DevScene::stat_acc, and they go there together: the wave hands every
    // entry to eight lanes, lane k of which adds w^k -- one atomic instruction serves eight entries with eight sector
    // requests.  (The memory system executes atomics per sector request, not per lane: 2.4e10 f64 atomics/s with every lane
    // on a sector of its own, 1.85e11/s with the lanes of a wave on consecutive addresses, profiles/microbench/
    // atomic_kinds_mi355x.txt; five atomic instructions on one sector, on the other hand, serialise.)
    // giveBack: the chained blocks of the list return to the group's pool.  The free stack allows takers OR returners at a time, not
    // both: the launch kernel returns (the transition kernel, which takes, has finished); a transition kernel that retires histories
    // itself (sparse generations) keeps their blocks out of the pool until the segment ends -- no slot is reused then, so the blocks
    // in use never exceed one history's worth per slot.  The pool (allocateSlotArrays, pmc_api.hip) holds that for histories of
    // minScattEvents > 16 and, memory permitting, one block per slot and instrument otherwise; a segment that still exhausts it
    // returns PMC_ERR_OVERFLOW with complete flux arrays and incomplete statistics arrays.
    // the wave's chunk of the group's statistics log (pmc_device.h StatLogArgs): wave-uniform; kept over the kernel launches by wave index
    struct StatLogWave
    {
        bool ok;                  // the log takes entries (false: none configured, or full -- atomics)
        unsigned long long base;  // first entry of the wave's open chunk
        uint32_t fill;            // entries of it in use (PMC_STAT_NO_CHUNK: the wave holds no chunk)
        uint32_t wave;            // index of the wave in the grid
    };
    __device__ __forceinline__ StatLogWave statLogBegin(const StatLogArgs& log)
    {
        StatLogWave w = {false, 0ull, PMC_STAT_NO_CHUNK, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)};
        if (log.cap != 0ull && w.wave < (uint32_t)PMC_STAT_LOG_WAVES)
        {
            w.ok = true;
            w.base = log.waveBase[w.wave];
            w.fill = log.waveFill[w.wave];
        }
        return w;
    }
    // the wave's place in its open chunk, for the next launch; the flush learns how much of the chunk is there
    __device__ __forceinline__ void statLogEnd(const StatLogArgs& log, const StatLogWave& w, int lane)
    {
        if (log.cap == 0ull || w.wave >= (uint32_t)PMC_STAT_LOG_WAVES || lane != 0) return;
        log.waveBase[w.wave] = w.base;
        log.waveFill[w.wave] = w.fill;
        if (w.fill != PMC_STAT_NO_CHUNK) log.chunkFill[w.base / PMC_RF_LOG_CHUNK] = w.fill;  // (also a chunk that has just become full: its entry held a shorter fill)
    }
    // appends (rec, w) of the lanes with rec >= 0; returns false if the log is full (the caller adds atomically)
    __device__ __forceinline__ bool statLogAppend(const DevScene& S, const StatLogArgs& log, StatLogWave& lw, int lane, int64_t rec, double w)
    {
        if (!lw.ok) return false;
        const unsigned long long m = __ballot(rec >= 0);
        const uint32_t n = (uint32_t)__popcll(m);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lw.fill == PMC_STAT_NO_CHUNK || lw.fill + n > (uint32_t)PMC_RF_LOG_CHUNK)
        {
            // the open chunk stays as it is (fewer than n entries were left), the next chunk is claimed
            if (lane == 0 && lw.fill != PMC_STAT_NO_CHUNK) log.chunkFill[lw.base / PMC_RF_LOG_CHUNK] = lw.fill;
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(S.counters + log.cursor, (unsigned long long)PMC_RF_LOG_CHUNK);
            got = __shfl(got, 0, 64);
            lw.fill = PMC_STAT_NO_CHUNK;
            if (got + PMC_RF_LOG_CHUNK > log.cap)
            {
                lw.ok = false;  // (the log is full: atomics from here on, also in the launches that follow -- the wave has no chunk)
                return false;
            }
            lw.base = got;
            lw.fill = 0;
        }
        if (rec >= 0)
        {
            log.keys[lw.base + lw.fill + rank] = (uint32_t)rec;
            log.vals[lw.base + lw.fill + rank] = w;
        }
        lw.fill += n;
        return true;
    }

    // KIN: an entry marked PMC_STAT_EMISSION_BIN (detect) belongs to the wavelength bin of the emission peel-off packet (SlotArrays::obsEll); there is
    // at most one, and it is a bin of its own (FluxRecorder sums the contributions of a history per (ell, pixel))
    template<bool KIN = false>
    __device__ __forceinline__ void flushStatistics(const DevScene& S, const DustLds& L, Counters& cnt, int slot, bool flush,
                                                    int lane, int group, bool giveBack, const StatLogArgs& statLog, StatLogWave& logWave)
    {
        const SlotArrays& A = S.slots;
        const int64_t stride = A.num_slots;
        for (int inst = 0; inst < S.num_instruments; ++inst)
        {
            const DevInstrument& I = S.inst[inst];
            if (!I.record_stats) continue;
            int n = 0, ell = -1;
            int ellEmission = -1;    // (KIN) the bin of a marked entry
            double wsedEmission = 0.;
            bool anyEmission = false, anyOther = false;
            // (the head record: length of the list, first chained block, and the first four entries -- a history has 3.7 entries
            // on average -- in one round trip)
            int block = -1;
            int4 bin4 = make_int4(-1, -1, -1, -1);
            double2 w01 = make_double2(0., 0.), w23 = make_double2(0., 0.);
            if (flush)
            {
                char* const head = reinterpret_cast<char*>(A.statHead) + ((int64_t)inst * stride + slot) * 64;
                const int2 headN = *reinterpret_cast<const int2*>(head + 48);
                bin4 = *reinterpret_cast<const int4*>(head);
                w01 = *reinterpret_cast<const double2*>(head + 16);
                w23 = *reinterpret_cast<const double2*>(head + 32);
                ell = S.mono ? I.mono_ell : A.ell[(int64_t)inst * stride + slot];
                if (KIN) ellEmission = A.obsEll[(int64_t)inst * stride + slot];
                *reinterpret_cast<int2*>(head + 48) = make_int2(0, -1);
                n = headN.x;
                if (n & PMC_STAT_POOL_EXHAUSTED)
                {
                    cnt.overflows += 1;
                    n &= ~PMC_STAT_POOL_EXHAUSTED;
                }
                if (n < 0) n = 0;
                // (entries beyond the slot's own list: the chained block the lane is reading)
                if (n > PMC_STAT_CAP) block = headN.y;
            }
            const int total = n;
            if (ell < 0 && !(KIN && ellEmission >= 0)) n = 0;  // (no bin: nothing to add, but the blocks are returned below)
            const int64_t base = ((int64_t)inst * stride + (flush ? slot : 0)) * PMC_STAT_CAP;
            double wsed = 0.;
            for (int e = 0; __ballot(e < n) != 0ull; ++e)
            {
                int64_t rec = -1;
                double w = 0.;
                if (e < n)
                {
                    int bin;
                    if (e < 4)
                    {
                        bin = e == 0 ? bin4.x : e == 1 ? bin4.y : e == 2 ? bin4.z : bin4.w;
                        w = e == 0 ? w01.x : e == 1 ? w01.y : e == 2 ? w23.x : w23.y;
                    }
                    else if (e < PMC_STAT_CAP)
                    {
                        bin = A.statBin[base + e];
                        w = A.statW[base + e];
                    }
                    else
                    {
                        const int q = (e - PMC_STAT_CAP) % PMC_STAT_CAP;
                        if (q == 0 && e > PMC_STAT_CAP)
                        {
                            const int done = block;
                            block = S.stat_pool_next[block];
                            if (giveBack) statBlockReturn(S, group, done);
                        }
                        bin = S.stat_pool_bin[(int64_t)block * PMC_STAT_CAP + q];
                        w = S.stat_pool_w[(int64_t)block * PMC_STAT_CAP + q];
                    }
                    int binEll = ell;
                    if (KIN && bin >= PMC_STAT_EMISSION_BIN - 1)
                    {
                        bin -= PMC_STAT_EMISSION_BIN;
                        binEll = ellEmission;
                        wsedEmission += w;
                        anyEmission = true;
                    }
                    else
                    {
                        wsed += w;
                        anyOther = true;
                    }
                    if (bin >= 0 && I.include_ifu)
                    {
                        rec = I.stat_acc_offset + bin + (int64_t)binEll * I.npix;
                        cnt.updates += 5;
                    }
                }
                const unsigned long long have = __ballot(rec >= 0);
                // (the group's log takes the entry; a full log, or none: the five sums of an entry as one atomic instruction of eight lanes)
                if (have == 0ull || statLogAppend(S, statLog, logWave, lane, rec, w)) continue;
                const int k = lane & 7;
#pragma unroll 1
                for (int sub = 0; sub < 8; ++sub)
                {
                    if (!((have >> (8 * sub)) & 0xFFull)) continue;
                    const int src = 8 * sub + (lane >> 3);
                    const int64_t r = __shfl(rec, src, 64);
                    const double ww = __shfl(w, src, 64);
                    if (r >= 0 && k < 5)
                    {
                        const double w2 = ww * ww, w3 = w2 * ww, w4 = w3 * ww;
                        const double v = k == 0 ? 1. : k == 1 ? ww : k == 2 ? w2 : k == 3 ? w3 : w4;
                        unsafeAtomicAdd(S.stat_acc + (r << 3) + k, v);
                    }
                }
            }
            // the blocks the loop has not returned yet (the last one; all of them if the history has no bin)
            if (total > PMC_STAT_CAP)
                while (block >= 0)
                {
                    const int done = block;
                    block = S.stat_pool_next[block];
                    if (giveBack) statBlockReturn(S, group, done);
                }
            if (n > 0 && I.include_sed && (!KIN || anyOther))
            {
                double* sed = L.sed + I.sed_lds_offset + I.num_components * I.num_lambda;
                double wn = 1.;
                for (int k = 0; k <= 4; ++k)
                {
                    atomicAdd(&sed[k * I.num_lambda + ell], wn);
                    wn *= wsed;
                }
            }
            if (KIN && anyEmission && I.include_sed)
            {
                double* sed = L.sed + I.sed_lds_offset + I.num_components * I.num_lambda;
                double wn = 1.;
                for (int k = 0; k <= 4; ++k)
                {
                    atomicAdd(&sed[k * I.num_lambda + ellEmission], wn);
                    wn *= wsedEmission;
                }
            }
        }
    }

    // ================================================================================================
    //  end of a segment: the statistics accumulator (DevScene::stat_acc, one 64-byte record per bin) is added to the wifu
    //  arrays of the frames (FluxRecorder's layout: five arrays of npix * num_lambda doubles per instrument) and cleared
    // ================================================================================================
    __global__ __launch_bounds__(256) void statMergeKernel(const int sceneSlot)
    {
        const DevScene& S = c_scene[sceneSlot];
        for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < S.stat_acc_records; r += (int64_t)gridDim.x * blockDim.x)
        {
            int inst = 0;
            for (int i = 0; i < S.num_instruments; ++i)
                if (S.inst[i].record_stats && S.inst[i].include_ifu && r >= S.inst[i].stat_acc_offset) inst = i;
            const DevInstrument& I = S.inst[inst];
            const int64_t q = r - I.stat_acc_offset;
            const int64_t len = I.npix * I.num_lambda;
            double2* rec = reinterpret_cast<double2*>(S.stat_acc + (r << 3));
            const double2 a = rec[0], b = rec[1], c = rec[2];
            if (a.x == 0.) continue;  // sum of w^0: no history contributed to this bin in the segment
            double* out = S.frames + I.wifu_offset + q;
            out[0] += a.x;
            out[len] += a.y;
            out[2 * len] += b.x;
            out[3 * len] += b.y;
            out[4 * len] += c.x;
            rec[0] = make_double2(0., 0.);
            rec[1] = make_double2(0., 0.);
            rec[2] = make_double2(0., 0.);
        }
    }
