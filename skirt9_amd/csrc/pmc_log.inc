// pmc_log.inc -- the log kernels (included by pmc_kernels.hip after pmc_walk_tree.inc, inside its anonymous namespace): the counting sort and
// the reduce kernels behind the radiation-field log (written by walkPropKernel) and the statistics log (written by the transition side)
    // ================================================================================================
    //  radiation field: the log of one slot group and generation -> table.  The log is a sequence of chunks of PMC_RF_LOG_CHUNK
    //  entries, each written by one wave (filled up with pad keys).  Four kernels, launched behind the generation's walks:
    //      rfHistKernel      entries per partition (key >> PMC_RF_BUCKET_BITS), counted per workgroup in LDS
    //      rfScanKernel      start of every partition in the partitioned log (one workgroup)
    //      rfScatterKernel   every chunk sorted by partition in LDS (rank by an LDS counter per partition, runs claimed with
    //                        one atomic per partition present), then written out in runs: coalesced stores
    //      rfReduceKernel    equal shares of the partitioned log per workgroup -- the partitions of the dense centre hold most
    //                        entries --, summed per key in LDS (64 KB per partition), added to the table
    //  A counting sort on the partition index only: order inside a partition does not matter to a sum.  (Rounds 1-3 used
    //  hipcub::DeviceRadixSort for the partition and read spans with several partitions once per partition.)
    // ================================================================================================
    constexpr uint32_t RF_MAX_PARTS = 8192;           // partitions an LDS histogram holds: tables up to 2^26 entries are logged (10^6 cells x 64 bins)
    constexpr uint32_t RF_TILE = PMC_RF_LOG_CHUNK;    // entries per tile of the counting sort = one chunk of the log
    constexpr int RF_SORT_BLOCK = 512;
    constexpr unsigned long long PMC_RF_REDUCE_SPAN = 1ull << 17;
    constexpr int RF_REDUCE_BLOCK = 512;

    // (BITS: keys per partition = 2^BITS -- PMC_RF_BUCKET_BITS for the radiation-field log, PMC_STAT_BUCKET_BITS for the statistics log)
    template<int BITS>
    // (fills: entries of every tile that are there -- the statistics log, whose waves leave chunks open or short -- or null: all of them)
    __global__ __launch_bounds__(256) void rfHistKernel(const uint32_t* __restrict__ keys, const unsigned long long n, const uint32_t numParts,
                                                        unsigned long long* __restrict__ hist, const uint32_t* __restrict__ fills)
    {
        __shared__ uint32_t h[RF_MAX_PARTS];
        const uint32_t tid = threadIdx.x;
        for (uint32_t i = tid; i < numParts; i += blockDim.x) h[i] = 0u;
        __syncthreads();
        const unsigned long long tiles = n / RF_TILE;
        for (unsigned long long t = blockIdx.x; t < tiles; t += gridDim.x)
        {
            const uint4* k4 = reinterpret_cast<const uint4*>(keys + t * RF_TILE);
            const unsigned long long left = fills ? fills[t] : RF_TILE;  // entries of this tile that are there
            for (uint32_t j = tid; j < RF_TILE / 4u; j += blockDim.x)
            {
                if (4ull * j >= left) break;
                const uint4 k = k4[j];
                const uint32_t b0 = k.x >> BITS, b1 = k.y >> BITS, b2 = k.z >> BITS, b3 = k.w >> BITS;
                if (b0 < numParts) atomicAdd(&h[b0], 1u);  // (pad keys lie beyond every partition: dropped here and in the scatter)
                if (b1 < numParts && 4ull * j + 1 < left) atomicAdd(&h[b1], 1u);
                if (b2 < numParts && 4ull * j + 2 < left) atomicAdd(&h[b2], 1u);
                if (b3 < numParts && 4ull * j + 3 < left) atomicAdd(&h[b3], 1u);
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < numParts; i += blockDim.x)
            if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
    }

    // exclusive prefix sum of `mine` over the lanes of a workgroup of up to 1024 lanes (wave scans + the waves' totals in LDS)
    __device__ __forceinline__ unsigned long long blockExclusiveScan(unsigned long long mine, unsigned long long* waveTotals, unsigned long long& total)
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
        unsigned long long incl = mine;
        for (int d = 1; d < 64; d <<= 1)
        {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) waveTotals[wave] = incl;
        __syncthreads();
        unsigned long long before = 0ull, all = 0ull;
        for (int w = 0; w < waves; ++w)
        {
            const unsigned long long t = waveTotals[w];
            if (w < wave) before += t;
            all += t;
        }
        total = all;
        __syncthreads();
        return before + incl - mine;
    }

    // hist (counts) -> cursor (the same array: next free position of every partition) and start[0 .. numParts] (kept for the reduce)
    // (one workgroup of PMC_SCAN_THREADS lanes with few registers -- a prefix in LDS instead of wave shuffles of 64-bit values --: room on a
    // CU next to a resident propagation workgroup, see endedScanKernel)
    __global__ __launch_bounds__(PMC_SCAN_THREADS) void rfScanKernel(unsigned long long* __restrict__ hist, unsigned long long* __restrict__ start, const uint32_t numParts)
    {
        __shared__ unsigned long long part[PMC_SCAN_THREADS];
        const uint32_t tid = threadIdx.x;
        const uint32_t per = (numParts + PMC_SCAN_THREADS - 1u) / PMC_SCAN_THREADS;
        const uint32_t lo = tid * per, hi = lo + per < numParts ? lo + per : numParts;
        unsigned long long sum = 0ull;
        for (uint32_t b = lo; b < hi; ++b) sum += hist[b];
        part[tid] = sum;
        __syncthreads();
        for (uint32_t off = 1; off < PMC_SCAN_THREADS; off <<= 1)
        {
            const unsigned long long add = tid >= off ? part[tid - off] : 0ull;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        unsigned long long at = part[tid] - sum;
        for (uint32_t b = lo; b < hi; ++b)
        {
            const unsigned long long c = hist[b];
            hist[b] = at;
            start[b] = at;
            at += c;
        }
        if (tid == PMC_SCAN_THREADS - 1) start[numParts] = part[PMC_SCAN_THREADS - 1];
    }

    template<int BITS>
    __global__ __launch_bounds__(RF_SORT_BLOCK) void rfScatterKernel(const uint32_t* __restrict__ keys, const double* __restrict__ vals, const unsigned long long n,
                                                                     const uint32_t numParts, unsigned long long* __restrict__ cursor,
                                                                     uint32_t* __restrict__ outKeys, double* __restrict__ outVals, const uint32_t* __restrict__ fills)
    {
        extern __shared__ double rfLds[];
        __shared__ unsigned long long waveTotals[16];
        double* stageV = rfLds;                                                 // RF_TILE doubles
        uint32_t* stageK = reinterpret_cast<uint32_t*>(rfLds + RF_TILE);         // RF_TILE keys
        uint32_t* cnt = stageK + RF_TILE;                                       // per partition: entries of the tile, then start of its run in the tile
        uint32_t* delta = cnt + numParts;                                       // per partition: position of its run in the output - start in the tile (mod 2^32)
        constexpr uint32_t E = RF_TILE / RF_SORT_BLOCK;                         // entries per lane
        constexpr uint32_t MAXPER = RF_MAX_PARTS / RF_SORT_BLOCK;               // partitions per lane in the tile's scan
        const uint32_t tid = threadIdx.x;
        const uint32_t per = (numParts + RF_SORT_BLOCK - 1u) / RF_SORT_BLOCK;
        const uint32_t lo = tid * per, hi = lo + per < numParts ? lo + per : numParts;
        const unsigned long long tiles = n / RF_TILE;
        for (unsigned long long t = blockIdx.x; t < tiles; t += gridDim.x)
        {
            for (uint32_t i = tid; i < numParts; i += RF_SORT_BLOCK) cnt[i] = 0u;
            __syncthreads();
            // a lane's entries: E consecutive keys (two 16-byte loads) and values
            uint32_t k[E], rank[E];
            double v[E];
            const unsigned long long base = t * RF_TILE + (unsigned long long)tid * E;
            for (uint32_t j = 0; j < E; j += 4u)
            {
                const uint4 q = *reinterpret_cast<const uint4*>(keys + base + j);
                k[j] = q.x, k[j + 1] = q.y, k[j + 2] = q.z, k[j + 3] = q.w;
            }
            for (uint32_t j = 0; j < E; j += 2u)
            {
                const double2 q = *reinterpret_cast<const double2*>(vals + base + j);
                v[j] = q.x, v[j + 1] = q.y;
            }
            // (a tile of the statistics log that a wave has left open or short: the entries beyond its fill are not there)
            if (fills)
            {
                const uint32_t there = fills[t];
                for (uint32_t j = 0; j < E; ++j)
                    if (tid * E + j >= there) k[j] = 0xFFFFFFFFu;
            }
            for (uint32_t j = 0; j < E; ++j)
            {
                const uint32_t b = k[j] >> BITS;
                rank[j] = b < numParts ? atomicAdd(&cnt[b], 1u) : 0u;
            }
            __syncthreads();
            // runs of the tile: exclusive scan of the counts; every partition present claims its run in the output
            uint32_t c[MAXPER];
            uint32_t sum = 0u;
            for (uint32_t i = 0; i < MAXPER; ++i)
            {
                const uint32_t b = lo + i;
                c[i] = b < hi ? cnt[b] : 0u;
                sum += c[i];
            }
            unsigned long long total;
            uint32_t at = (uint32_t)blockExclusiveScan((unsigned long long)sum, waveTotals, total);
            for (uint32_t i = 0; i < MAXPER; ++i)
            {
                const uint32_t b = lo + i;
                if (b < hi)
                {
                    cnt[b] = at;
                    if (c[i]) delta[b] = (uint32_t)atomicAdd(&cursor[b], (unsigned long long)c[i]) - at;
                    at += c[i];
                }
            }
            __syncthreads();
            for (uint32_t j = 0; j < E; ++j)
            {
                const uint32_t b = k[j] >> BITS;
                if (b < numParts)
                {
                    const uint32_t pos = cnt[b] + rank[j];
                    stageK[pos] = k[j];
                    stageV[pos] = v[j];
                }
            }
            __syncthreads();
            const uint32_t live = (uint32_t)total;
            for (uint32_t pos = tid; pos < live; pos += RF_SORT_BLOCK)
            {
                const uint32_t key = stageK[pos];
                const uint32_t dest = pos + delta[key >> BITS];
                outKeys[dest] = key;
                outVals[dest] = stageV[pos];
            }
            __syncthreads();
        }
    }

    __global__ __launch_bounds__(RF_REDUCE_BLOCK) void rfReduceKernel(const int sceneSlot, const uint32_t* __restrict__ keys, const double* __restrict__ vals,
                                                                      const unsigned long long* __restrict__ start, const uint32_t numParts)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double acc[];
        constexpr uint32_t SIZE = 1u << PMC_RF_BUCKET_BITS;
        const uint32_t tid = threadIdx.x;
        const unsigned long long total = start[numParts];
        const unsigned long long first = (unsigned long long)blockIdx.x * PMC_RF_REDUCE_SPAN;
        if (first >= total) return;
        const unsigned long long last = first + PMC_RF_REDUCE_SPAN < total ? first + PMC_RF_REDUCE_SPAN : total;
        const int64_t size = (int64_t)S.cell_slots * S.rf_num_lambda;  // (keys count cells in the device numbering)
        const int nl = S.rf_num_lambda;
        // table index of a key: the caller's cell index from the device one (padding slots of the device numbering hold no cell)
        auto tableIndex = [&](int64_t key) -> int64_t {
            if (key >= size) return -1;
            const int64_t dev = nl == 1 ? key : key / nl;
            const int m = S.cell_ext[dev];
            return m < 0 ? -1 : (int64_t)m * nl + (key - dev * nl);
        };
        // the partition that holds entry `first`: the last one that starts at or before it
        uint32_t b = 0u, hiPart = numParts;
        while (hiPart - b > 1u)
        {
            const uint32_t mid = (b + hiPart) >> 1;
            if (start[mid] <= first)
                b = mid;
            else
                hiPart = mid;
        }
        unsigned long long pos = first;
        while (pos < last)
        {
            while (start[b + 1u] <= pos) ++b;  // (empty partitions)
            const unsigned long long end = start[b + 1u] < last ? start[b + 1u] : last;
            const int64_t partBase = (int64_t)b << PMC_RF_BUCKET_BITS;
            if (end - pos < (unsigned long long)PMC_RF_SHORT_RUN)
            {
                // a short run (the sparse outskirts; tables with many wavelength bins): not worth clearing and flushing 64 KB
                for (unsigned long long i = pos + tid; i < end; i += RF_REDUCE_BLOCK)
                {
                    const int64_t at = tableIndex(partBase + (keys[i] & (SIZE - 1u)));
                    if (at >= 0) unsafeAtomicAdd(S.rf + at, vals[i]);
                }
            }
            else
            {
                for (uint32_t i = tid; i < SIZE; i += RF_REDUCE_BLOCK) acc[i] = 0.;
                __syncthreads();
                for (unsigned long long i = pos + tid; i < end; i += RF_REDUCE_BLOCK) atomicAdd(&acc[keys[i] & (SIZE - 1u)], vals[i]);
                __syncthreads();
                for (uint32_t i = tid; i < SIZE; i += RF_REDUCE_BLOCK)
                {
                    const double v = acc[i];
                    if (v != 0.)
                    {
                        const int64_t at = tableIndex(partBase + i);
                        if (at >= 0) unsafeAtomicAdd(S.rf + at, v);
                    }
                }
                __syncthreads();
            }
            pos = end;
        }
    }

    // ================================================================================================
    //  statistics log -> accumulator records (pmc_device.h StatLogArgs): the log, partitioned by key range (2^PMC_STAT_BUCKET_BITS records
    //  per partition) by the counting sort above; every workgroup takes an equal share of it -- the partitions of the image centre hold
    //  most entries --, sums w^0 .. w^4 per record in LDS and adds the non-zero sums to DevScene::stat_acc (five consecutive doubles of
    //  a 64-byte record: lanes on consecutive addresses).  FluxRecorder.cpp:1000-1012.
    // ================================================================================================
    __global__ __launch_bounds__(RF_REDUCE_BLOCK) void statReduceKernel(const int sceneSlot, const uint32_t* __restrict__ keys, const double* __restrict__ vals,
                                                                        const unsigned long long* __restrict__ start, const uint32_t numParts)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double acc[];  // [5][SIZE]
        constexpr uint32_t SIZE = 1u << PMC_STAT_BUCKET_BITS;
        const uint32_t tid = threadIdx.x;
        const unsigned long long total = start[numParts];
        const unsigned long long first = (unsigned long long)blockIdx.x * PMC_RF_REDUCE_SPAN;
        if (first >= total) return;
        const unsigned long long last = first + PMC_RF_REDUCE_SPAN < total ? first + PMC_RF_REDUCE_SPAN : total;
        const int64_t records = S.stat_acc_records;
        // the partition that holds entry `first`: the last one that starts at or before it
        uint32_t b = 0u, hiPart = numParts;
        while (hiPart - b > 1u)
        {
            const uint32_t mid = (b + hiPart) >> 1;
            if (start[mid] <= first)
                b = mid;
            else
                hiPart = mid;
        }
        unsigned long long pos = first;
        while (pos < last)
        {
            while (start[b + 1u] <= pos) ++b;  // (empty partitions)
            const unsigned long long end = start[b + 1u] < last ? start[b + 1u] : last;
            const int64_t partBase = (int64_t)b << PMC_STAT_BUCKET_BITS;
            if (end - pos < (unsigned long long)PMC_STAT_SHORT_RUN)
            {
                // a short run (the outskirts of the image): not worth clearing and flushing 80 KB
                for (unsigned long long i = pos + tid; i < end; i += RF_REDUCE_BLOCK)
                {
                    const int64_t rec = partBase + (keys[i] & (SIZE - 1u));
                    if (rec < records)
                    {
                        // (powers as FluxRecorder.cpp:1003-1008 forms them, wn *= w: ((w w) w) w -- the same operations as the atomic path)
                        const double w = vals[i], w2 = w * w, w3 = w2 * w, w4 = w3 * w;
                        double* const at = S.stat_acc + (rec << 3);
                        unsafeAtomicAdd(at + 0, 1.), unsafeAtomicAdd(at + 1, w), unsafeAtomicAdd(at + 2, w2), unsafeAtomicAdd(at + 3, w3), unsafeAtomicAdd(at + 4, w4);
                    }
                }
            }
            else
            {
                for (uint32_t i = tid; i < 5u * SIZE; i += RF_REDUCE_BLOCK) acc[i] = 0.;
                __syncthreads();
                for (unsigned long long i = pos + tid; i < end; i += RF_REDUCE_BLOCK)
                {
                    const uint32_t k = keys[i] & (SIZE - 1u);
                    const double w = vals[i], w2 = w * w, w3 = w2 * w, w4 = w3 * w;
                    atomicAdd(&acc[k], 1.), atomicAdd(&acc[SIZE + k], w), atomicAdd(&acc[2u * SIZE + k], w2), atomicAdd(&acc[3u * SIZE + k], w3),
                        atomicAdd(&acc[4u * SIZE + k], w4);
                }
                __syncthreads();
                // (eight lanes per record, five of them add: consecutive addresses of one 64-byte record)
                for (uint32_t i = tid; i < 8u * SIZE; i += RF_REDUCE_BLOCK)
                {
                    const uint32_t k = i >> 3, p = i & 7u;
                    if (p < 5u && acc[k] != 0. && partBase + k < records) unsafeAtomicAdd(S.stat_acc + ((partBase + k) << 3) + p, acc[p * SIZE + k]);
                }
                __syncthreads();
            }
            pos = end;
        }
    }
