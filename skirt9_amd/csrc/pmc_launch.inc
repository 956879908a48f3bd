// pmc_launch.inc -- the launch of a history (included by pmc_kernels.hip inside its anonymous namespace).
//
// The kinematics of a moving source, launchHistory (SourceSystem::launch ... PhotonPacket::launch and the first cycle), and
// launchKernel, which runs it for every slot whose history has ended (with the shared pieces of pmc_transition.inc: LDS staging,
// workgroup epilogue, counters).

    // ---- SourceSystem::launch ... PhotonPacket::launch (SourceSystem.cpp:101-112, NormalizedSource.cpp:73-110,
    //      PointSource.cpp:32-43, GeometricSource.cpp:66-82, SpheGeometry.cpp:25-32, SersicGeometry.cpp:41-45) followed
    //      by the first cycle (emission peel-offs and first propagation walk); returns false for a zero-luminosity packet
    // the bulk velocity of a source at the launch position r (pmc.h pmc_source_velocity): magnitude * field(r), GeometricSource.cpp:66-82 with
    // UnidirectionalVectorField.cpp:28-31, RadialVectorField.cpp:17-35, CylindricalVectorField.cpp:17-36, OffsetVectorFieldDecorator.cpp:16-21; a
    // PointSource's velocity is magnitude 1 times the vector (SpecialtySource.cpp:48-51)
    __device__ __forceinline__ void sourceVelocity(const DevVelocity& V, double rx, double ry, double rz, double& vx, double& vy, double& vz)
    {
        vx = 0., vy = 0., vz = 0.;
        if (V.kind == PMC_VELOCITY_NONE) return;
        double ux = V.vec[0], uy = V.vec[1], uz = V.vec[2];
        if (V.kind != PMC_VELOCITY_CONSTANT)
        {
            const double x = rx - V.vec[0], y = ry - V.vec[1], z = rz - V.vec[2];
            const bool radial = V.kind == PMC_VELOCITY_RADIAL;
            ux = radial ? x : -y, uy = radial ? y : x, uz = radial ? z : 0.;
            const double r = sqrt(ux * ux + uy * uy + uz * uz);
            if (r == 0.) return;  // (the null vector at the centre resp. on the axis)
            ux /= r, uy /= r, uz /= r;
            double v = 1.;
            if (V.unity_radius > 0. && ((V.exponent > 0. && r < V.unity_radius) || (V.exponent < 0. && r > V.unity_radius)))
                v = pow(r / V.unity_radius, V.exponent);
            ux = v * ux, uy = v * uy, uz = v * uz;
        }
        vx = V.magnitude * ux, vy = V.magnitude * uy, vz = V.magnitude * uz;
    }
    // PhotonPacket::shiftedEmissionWavelength (PhotonPacket.cpp:133-136)
    __device__ __forceinline__ double shiftedEmissionWavelength(double lambda0, double kx, double ky, double kz, double vx, double vy, double vz)
    {
        return lambda0 * (1 - (kx * vx + ky * vy + kz * vz) / 2.99792458e8);
    }
    // the number of the n ascending borders that are <= lambda (std::upper_bound): the index into a wavelength grid's table of bins
    // (DisjointWavelengthGrid::bin, DisjointWavelengthGrid.cpp:334-345)
    __device__ __forceinline__ int bordersUpTo(const double* border, int n, double lambda)
    {
        int lo = 0, hi = n;
        while (lo < hi)
        {
            int mid = (lo + hi) >> 1;
            if (lambda < border[mid])
                hi = mid;
            else
                lo = mid + 1;
        }
        return lo;
    }
    // the wavelength bin of instrument I for a packet of rest wavelength lambda, or -1: the bin of its redshifted wavelength lambda (1 + z)
    // (FluxRecorder.cpp:309-310)
    __device__ __forceinline__ int observedBin(const DevInstrument& I, double lambda)
    {
        return I.ellv[bordersUpTo(I.border, I.num_border, lambda * I.zp1)];
    }

    // KIN (a scene with a moving source): the packet's wavelength is Doppler-shifted by the source's velocity along the launch direction
    // (PhotonPacket.cpp:18-40: the weight W = L lambda0 keeps the sampled wavelength), and so is, by the velocity along its line of sight,
    // that of the emission peel-off packet towards every observer (:66-85): SlotArrays::obsLambda, obsExt, obsEll
    // F: the launch flavour (pmc_device.h PMC_LAUNCH_*, pmcLaunchFlavourOf) -- what the scene fixes of the steps below is a constant here, and the
    // code of every other wavelength mode, source geometry and angular distribution is not in the kernel; the deviates drawn, and their order,
    // are those of the generic form (F = 0, or PMC_LAUNCH_KIN alone), which asks the source for each of them
    template<int F = 0>
    __device__ __forceinline__ bool launchHistory(const DevScene& S, const DustLds& L, Counters& cnt, int slot, uint64_t history, uint64_t seed)
    {
        constexpr bool KIN = (F & PMC_LAUNCH_KIN) != 0;
        constexpr bool OLIGO = (F & PMC_LAUNCH_OLIGO) != 0;
        constexpr bool ISOTROPIC = (F & PMC_LAUNCH_ISOTROPIC) != 0;
        constexpr int GEOM = F >> PMC_LAUNCH_GEOM_SHIFT;
        const SlotArrays& A = S.slots;
        // SourceSystem::launch (SourceSystem.cpp:100-107): the source that owns this history index (the Sersic flavour: the only one)
        int si = 0;
        if (GEOM != PMC_LAUNCH_GEOM_SERSIC)
            while (si + 1 < S.num_sources && history >= S.src_first[si + 1]) ++si;
        const DevSource& Q = S.src[si];
        const int sourceKind = GEOM == PMC_LAUNCH_GEOM_SERSIC ? PMC_SOURCE_SERSIC : GEOM == PMC_LAUNCH_GEOM_POINT ? PMC_SOURCE_POINT : Q.source_kind;
        const int angularKind = ISOTROPIC ? PMC_ANGULAR_ISOTROPIC : Q.angular_kind;
        Rng rng;
        rng.h0 = (uint32_t)history;
        rng.h1 = (uint32_t)(history >> 32);
        rng.block = 0;
        rng.have = 0;
        rng.spare = 0.;
        double lambda, w;
        if (OLIGO || Q.lambda_mode == PMC_LAMBDA_OLIGO)
        {
            (void)rngUniform(rng, seed);  // the `uniform() > xi` test of NormalizedSource::launch with xi = 1
            int index = (int)(rngUniform(rng, seed) * Q.num_oligo);
            if (index > Q.num_oligo - 1) index = Q.num_oligo - 1;
            lambda = Q.oligo_lambda[index];
            w = Q.oligo_weight[index];
        }
        else
        {
            const double xi = Q.lambda_bias;
            bool fromSed = true;
            if (xi != 0.) fromSed = rngUniform(rng, seed) > xi;
            if (fromSed)
            {
                // Random::cdfLogLog (Random.cpp:209-216)
                double X = rngUniform(rng, seed);
                int i = locateClip(Q.sed_P, Q.num_sed, X);
                double alpha = log(Q.sed_p[i + 1] / Q.sed_p[i]) / log(Q.sed_lambda[i + 1] / Q.sed_lambda[i]);
                lambda = Q.sed_lambda[i] * generalizedExp(-alpha, (X - Q.sed_P[i]) / (Q.sed_p[i] * Q.sed_lambda[i]));
            }
            else if (Q.bias_kind == PMC_BIAS_LIN)
                lambda = Q.bias_min + (Q.bias_max - Q.bias_min) * rngUniform(rng, seed);
            else
                lambda = exp(log(Q.bias_min) + (log(Q.bias_max) - log(Q.bias_min)) * rngUniform(rng, seed));
            if (xi == 0.)
                w = 1.;
            else
            {
                // SED::specificLuminosity: analytic for a black body (BlackBodySED.cpp:36-39, PlanckFunction.cpp:24-27),
                // otherwise log-log interpolation of the normalised table
                double sl = 0.;
                if (Q.sed_kind == PMC_SED_BLACKBODY)
                    sl = Q.sed_f2 / pow(lambda, 5) / (exp(Q.sed_f1 / lambda) - 1.0) / Q.sed_ltot;
                else if (lambda >= Q.sed_lambda[0] && lambda <= Q.sed_lambda[Q.num_sed - 1])
                {
                    int i = locate(Q.sed_lambda, Q.num_sed, lambda);
                    if (i < 0) i = 0;
                    sl = interpolateLogLog(lambda, Q.sed_lambda[i], Q.sed_lambda[i + 1], Q.sed_p[i], Q.sed_p[i + 1]);
                }
                if (sl == 0.)
                    w = 0.;
                else
                {
                    double b = 0.;
                    if (lambda >= Q.bias_min && lambda <= Q.bias_max)
                        b = Q.bias_kind == PMC_BIAS_LIN ? 1. / (Q.bias_max - Q.bias_min)
                                                        : 1. / ((log(Q.bias_max) - log(Q.bias_min)) * lambda);
                    w = sl / ((1 - xi) * sl + xi * b);
                }
            }
        }
        double rx, ry, rz;
        if (sourceKind == PMC_SOURCE_POINT)
        {
            rx = Q.src_pos[0];
            ry = Q.src_pos[1];
            rz = Q.src_pos[2];
        }
        else if (sourceKind == PMC_SOURCE_SERSIC)
        {
            // (the tables of a single source are staged in LDS)
            const bool staged = GEOM == PMC_LAUNCH_GEOM_SERSIC || S.num_sources == 1;
            const double* sv = staged ? L.src : Q.sersic_s;
            const double* Mv = staged ? L.src + Q.sersic_n : Q.sersic_M;
            double X = rngUniform(rng, seed);
            int n = Q.sersic_n;
            int i = locate(Mv, n, X);
            double s;
            if (i < 0)
                s = sv[0];
            else if (i >= n - 1)
                s = sv[n - 1];
            else
                s = interpolateLogLog(X, Mv[i], Mv[i + 1], sv[i], sv[i + 1]);
            double radius = Q.reff * s;
            double dx, dy, dz;
            randomDirection(rng, seed, dx, dy, dz);
            rx = dx * radius;
            ry = dy * radius;
            rz = dz * radius;
        }
        else if (sourceKind == PMC_SOURCE_EXP_DISK)
        {
            // ExpDiskGeometry::randomCylRadius / randomZ with SepAxGeometry::generatePosition
            const double hR = Q.src_box[0], hz = Q.src_box[1], Rmin = Q.src_box[2], Rmax = Q.src_box[3], zmax = Q.src_box[4];
            double R, X;
            do
            {
                X = rngUniform(rng, seed);
                R = hR * (-1.0 - lambertLowerBranch((X - 1.0) / M_E));
            } while ((Rmax > 0.0 && R >= Rmax) || R <= Rmin);
            const double phi = 2.0 * M_PI * rngUniform(rng, seed);
            double z;
            do
            {
                X = rngUniform(rng, seed);
                z = (X <= 0.5) ? hz * log(2.0 * X) : -hz * log(2.0 * (1.0 - X));
            } while (zmax > 0.0 && fabs(z) >= zmax);
            double sinphi, cosphi;
            sincos(phi, &sinphi, &cosphi);
            rx = R * cosphi;
            ry = R * sinphi;
            rz = z;
        }
        else if (sourceKind == PMC_SOURCE_PLUMMER)
        {
            const double t = pow(rngUniform(rng, seed), 1.0 / 3.0);
            const double radius = Q.src_box[0] * t / sqrt((1.0 - t) * (1.0 + t));
            double dx, dy, dz;
            randomDirection(rng, seed, dx, dy, dz);
            rx = radius * dx;
            ry = radius * dy;
            rz = radius * dz;
        }
        else
        {
            double x = rngUniform(rng, seed);
            double y = rngUniform(rng, seed);
            double z = rngUniform(rng, seed);
            rx = Q.src_box[0] + x * (Q.src_box[3] - Q.src_box[0]);
            ry = Q.src_box[1] + y * (Q.src_box[4] - Q.src_box[1]);
            rz = Q.src_box[2] + z * (Q.src_box[5] - Q.src_box[2]);
        }
        // SpheroidalGeometryDecorator::generatePosition (SpheroidalGeometryDecorator.cpp:19-25)
        if ((sourceKind == PMC_SOURCE_SERSIC || sourceKind == PMC_SOURCE_PLUMMER) && Q.src_box[5] != 0.) rz = Q.src_box[5] * rz;
        // OffsetGeometryDecorator::generatePosition (OffsetGeometryDecorator.cpp:33-39)
        if (sourceKind != PMC_SOURCE_POINT && (Q.src_pos[0] != 0. || Q.src_pos[1] != 0. || Q.src_pos[2] != 0.))
        {
            rx = rx + Q.src_pos[0];
            ry = ry + Q.src_pos[1];
            rz = rz + Q.src_pos[2];
        }
        double kx, ky, kz;
        if (angularKind != PMC_ANGULAR_ISOTROPIC)
        {
            // AxAngularDistribution::generateDirection (AxAngularDistribution.cpp:36-39) with the inclination cosine of
            // LaserAngularDistribution.cpp:20-23, ConicalAngularDistribution.cpp:29-36, NetzerAngularDistribution.cpp:42-45 (Random::cdfLinLin)
            double costheta = 1.;
            if (angularKind == PMC_ANGULAR_CONICAL)
            {
                const double X = rngUniform(rng, seed);
                if (X < 0.5)
                    costheta = 1.0 - 2.0 * X * (1.0 - Q.angular_cos_delta);
                else
                    costheta = 1.0 - 2.0 * Q.angular_cos_delta - 2.0 * X * (1.0 - Q.angular_cos_delta);
            }
            else if (angularKind == PMC_ANGULAR_NETZER)
            {
                const double X = rngUniform(rng, seed);
                const int i = locateClip(S.netzer_X, PMC_NETZER_POINTS + 1, X);
                costheta = S.netzer_cos[i] + ((X - S.netzer_X[i]) / (S.netzer_X[i + 1] - S.netzer_X[i])) * (S.netzer_cos[i + 1] - S.netzer_cos[i]);
            }
            directionAbout(rng, seed, Q.angular_axis[0], Q.angular_axis[1], Q.angular_axis[2], costheta, kx, ky, kz);
        }
        else
            randomDirection(rng, seed, kx, ky, kz);
        const double Lw = Q.packet_luminosity * w;
        const double W = Lw * lambda;
        const double lambda0 = lambda;
        double vx = 0., vy = 0., vz = 0.;
        if (KIN)
        {
            sourceVelocity(S.vel[si], rx, ry, rz, vx, vy, vz);
            lambda = shiftedEmissionWavelength(lambda0, kx, ky, kz, vx, vy, vz);
        }
        if (!(W / lambda > 0)) return false;
        A.rx[slot] = rx, A.ry[slot] = ry, A.rz[slot] = rz;
        A.kx[slot] = kx, A.ky[slot] = ky, A.kz[slot] = kz;
        if (!S.mono) A.lambda[slot] = lambda;
        A.W[slot] = W;
        A.history[slot] = history;
        A.nscatt[slot] = 0;
        A.mint[slot] = -1;  // (no hint for the first cell of the first cycle's walks)
        // dust properties at this wavelength (DustMix::indexForLambda, DustMix.cpp:276-279)
        const int il = locateClip(L.lamb, S.num_lambda, lambda);
        const double sext = L.sext[il], asym = L.asym[il];
        if (!S.mono)
        {
            A.dustExt[slot] = sext;
            A.dustSca[slot] = L.ssca[il];
            if (S.explicit_absorption) A.dustAbs[slot] = S.sigma_abs[il];
            A.dustAsym[slot] = asym;
            // (several components: each one's own wavelength bin; the walk and transition kernels read its tables through it)
            if (S.num_media > 1)
                for (int h = 0; h < S.num_media; ++h)
                    A.dustIdx[(int64_t)h * A.num_slots + slot] = locateClip(S.med[h].lambda_border, S.med[h].num_lambda, lambda);
        }
        // wavelength bin of every instrument (DisjointWavelengthGrid::bin, DisjointWavelengthGrid.cpp:334-345)
        for (int i = 0; i < S.num_instruments; ++i)
        {
            const DevInstrument& I = S.inst[i];
            // (one wavelength for every history: DevInstrument::mono_ell)
            if (!S.mono) A.ell[(int64_t)i * A.num_slots + slot] = observedBin(I, lambda);
            if (KIN)
            {
                // the emission peel-off packet towards this instrument's observer: wavelength, cross section there, bin
                const double lambdaPeel = shiftedEmissionWavelength(lambda0, I.kx, I.ky, I.kz, vx, vy, vz);
                const double lambdaPeelObs = lambdaPeel * I.zp1;
                const int plo = bordersUpTo(I.border, I.num_border, lambdaPeelObs);  // (observedBin, its load behind the stores)
                A.obsLambda[(int64_t)i * A.num_slots + slot] = lambdaPeel;
                A.obsExt[(int64_t)i * A.num_slots + slot] = L.sext[locateClip(L.lamb, S.num_lambda, lambdaPeel)];
                A.obsEll[(int64_t)i * A.num_slots + slot] = I.ellv[plo];
            }
            if (S.any_stats) *reinterpret_cast<int2*>(reinterpret_cast<char*>(A.statHead) + ((int64_t)i * A.num_slots + slot) * 64 + 48) = make_int2(0, -1);
        }
        if (S.rf_store)
        {
            // bin of the radiation field wavelength grid (DisjointWavelengthGrid::bin)
            A.rfell[slot] = S.rf_ellv[bordersUpTo(S.rf_border, S.rf_num_border, lambda)];
        }
        // the photon cycle starts with the emission peel-offs and the first propagation walk
        A.Lthreshold[slot] = (W / lambda) / S.min_weight_reduction;  // MonteCarloSimulation.cpp:566
        PMC_T_STAMP(4);
        announceCycle<false, KIN>(S, slot, seed, rng, rx, ry, rz, kx, ky, kz, W, asym, 0, nullptr, nullptr, angularKind != PMC_ANGULAR_ISOTROPIC ? &Q : nullptr);
        storeRng(A, slot, rng);
        return true;
    }

    // ================================================================================================
    //  launch kernel: one lane per slot of the group, in slot order (the slot arrays are read and written coalesced); the
    //  lanes whose history has ended (first generation: all) flush the per-history statistics, take up the next history --
    //  its index follows from the scanned counts -- launch it and start its first cycle
    // ================================================================================================
    //  F: the launch flavour (pmc_device.h PMC_LAUNCH_*: a moving source, and what the scene fixes of SourceSystem::launch); the statistics
    //  flush, the first cycle and the workgroup's epilogue are the same code in every flavour
    template<int F>
    __device__ __forceinline__ void launchBody(const int sceneSlot, const int slotBase, const int numSlots, const int group, const uint64_t first,
                                               const uint64_t count, const uint64_t seed, const int initial, const StatLogArgs& statLog)
    {
        const DevScene& S = c_scene[sceneSlot];
        extern __shared__ double lds[];
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        BlockLds B;
        constexpr bool KIN = (F & PMC_LAUNCH_KIN) != 0;
        Counters cnt = {0, 0, 0, 0, 0};
        StatLogWave logWave = statLogBegin(statLog);
        PMC_T_PROF_BEGIN;
        stageBlock<true>(S, lds, tid, blockDim.x, B);
        PMC_T_STAMP(0);
        const DustLds& L = B.L;
        const SlotArrays& A = S.slots;
        const unsigned long long hbase = initial ? 0ull : S.counters[PMC_CTR_HBASE(group)];
        // (the first history index this group may not take in this generation: endedScanKernel)
        const unsigned long long hlimit = initial ? count : min(count, (unsigned long long)S.counters[PMC_CTR_HLIMIT(group)]);
        uint32_t liveCount = 0;
        // Persistent workgroups (the tables are staged once).  Every WAVE serves runs of 256 slots.  In the first generation every slot
        // of the run takes a history; afterwards about a quarter have ended, and the wave compacts them into its own list in LDS: what
        // follows (statistics flush, source sampling, the start of a cycle) is long divergent code that then runs with full waves, in
        // slot order, and no wave waits for another one (with one list per workgroup the first wave did the work of a tile while the
        // other three sat at the barrier: half of the kernel's wave cycles).
        const int wv = tid >> 6;
        const int perWave = 256;
        const int span = perWave * ((int)blockDim.x >> 6);
        const int slotEnd = slotBase + numSlots;
        int* const myList = B.sortSlot + wv * 256;
        const int numTiles = (numSlots + span - 1) / span;
        for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x)
        {
            const int wbase = slotBase + tile * span + wv * perWave;
            int n = 0;
            unsigned long long h0 = 0;
            if (initial)
                n = max(0, min(perWave, slotEnd - wbase));
            else if (wbase < slotEnd)
            {
                int md[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    const int s0 = wbase + 64 * j + lane;
                    md[j] = s0 < slotEnd ? A.mode[s0] : 0;
                }
                // ended histories of the group before this run: the scanned count of its first wave tile
                h0 = hbase + S.tasks.endedCount[wbase >> 6];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    const bool ended = (md[j] & MODE_ENDED) != 0;
                    const unsigned long long m = __ballot(ended);
                    if (ended) myList[n + __popcll(m & ((1ull << lane) - 1ull))] = wbase + 64 * j + lane;
                    n += __popcll(m);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            PMC_T_STAMP(1);
            for (int c = 0; c < n; c += 64)
            {
                int slot = -1;
                unsigned long long h = 0;
                if (c + lane < n)
                {
                    slot = initial ? wbase + c + lane : myList[c + lane];
                    h = h0 + (unsigned long long)(c + lane);
                }
                const bool ended = slot >= 0;
                if (!initial && S.any_stats) flushStatistics<KIN>(S, L, cnt, slot, ended, lane, group, true, statLog, logWave);
                PMC_T_STAMP(2);
                int event = ended ? EV_LAUNCH : EV_NONE;
                // (first generation, and the rare zero-luminosity packet whose life cycle the reference skips: the index is drawn
                // from the global cursor, one atomic per wave)
                bool assigned = !initial;
                unsigned long long bound = initial ? count : hlimit;  // (an index drawn from the cursor itself: the segment's count)
                unsigned long long want;
                while ((want = __ballot(event == EV_LAUNCH)) != 0ull)
                {
                    if (!assigned)
                    {
                        bound = count;
                        unsigned long long hh = 0;
                        if (lane == __ffsll((long long)want) - 1) hh = atomicAdd(S.counters + PMC_CTR_HISTORY, (unsigned long long)__popcll(want));
                        hh = __shfl(hh, __ffsll((long long)want) - 1, 64);
                        h = hh + __popcll(want & ((1ull << lane) - 1ull));
                    }
                    assigned = false;
                    if (event == EV_LAUNCH)
                    {
                        if (h >= bound)
                        {
                            // no history left (for this group): the slot dies
                            event = EV_DEAD;
                            A.mode[slot] = MODE_NONE;
                            for (int r = 0; r <= S.num_instruments; ++r) S.tasks.bits[(int64_t)r * A.num_slots + slot] = PMC_TASK_NONE;
                        }
                        else
                        {
                            cnt.histories += 1;
                            if (launchHistory<F>(S, L, cnt, slot, first + h, seed)) event = EV_TASK;
                        }
                    }
                }
                if (event == EV_TASK) liveCount += 1;
                PMC_T_STAMP(3);
            }
            // (the list is rewritten in the next round only after every lane has read its entry)
            __builtin_amdgcn_wave_barrier();
        }
        {
            const unsigned long long live = waveSum(liveCount);
            if (lane == 0 && live) atomicAdd(S.counters + PMC_CTR_LIVE(group), live);
        }
        statLogEnd(statLog, logWave, lane);
        flushBlock(S, L, tid, blockDim.x);
        PMC_T_STAMP(6);
        PMC_T_PROF_END(200);
        addCounters(S, cnt, lane);
    }
    template<int F>
    __global__ __launch_bounds__(256, PMC_LAUNCH_MIN_WAVES) void launchKernel(const int sceneSlot, const int slotBase, const int numSlots, const int group,
                                                        const uint64_t first, const uint64_t count, const uint64_t seed, const int initial,
                                                        const StatLogArgs statLog)
    {
        launchBody<F>(sceneSlot, slotBase, numSlots, group, first, count, seed, initial, statLog);
    }
