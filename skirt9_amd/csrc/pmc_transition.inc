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

    // Henyey-Greenstein phase function of asymmetry g (DustMix.cpp:395-425): its value for a scattering cosine, and its mean
    // over the cone of half-angle 4 degrees around that cosine -- the reference's stand-in for the value when |g| > 0.95,
    // where the forward peak is narrower than a detector pixel.  The quantities that depend on g alone are formed once; the
    // operations on them are the reference's, in its order (the frames are compared with the oracle at 1e-9).
    struct PhaseHG
    {
        double g;
        double onePlusG2;  // 1 + g g
        double twoG;       // 2 g
        double norm;       // (1 - g)(1 + g)
        __device__ __forceinline__ explicit PhaseHG(double asym) : g(asym), onePlusG2(1. + asym * asym), twoG(2. * asym), norm((1. - asym) * (1. + asym)) {}
        // 1 + g^2 - 2 g cos(theta): the squared distance kernel of the phase function
        __device__ __forceinline__ double kernel(double c) const { return onePlusG2 - twoG * c; }
        __device__ __forceinline__ double value(double c) const
        {
            const double t = kernel(c);
            return norm / sqrt(t * t * t);
        }
        // integral of the phase function over cos(theta) from cosFar to cosNear (cosNear >= cosFar)
        __device__ __forceinline__ double between(double cosNear, double cosFar) const
        {
            const double rootNear = sqrt(kernel(cosNear));
            const double rootFar = sqrt(kernel(cosFar));
            const double scale = norm / g;
            const double span = (rootFar - rootNear) / (rootFar * rootNear);
            return scale * span;
        }
        __device__ __forceinline__ double coneMean(double c) const
        {
            const double halfAngle = 4. * M_PI / 180.;
            const double theta = acos(c);
            const double cosInner = cos(theta - halfAngle);  // edge of the cone towards the forward direction
            const double cosOuter = cos(theta + halfAngle);
            // a cone that contains the forward (backward) pole is folded there: both edges are measured from the pole
            if (theta < halfAngle) return (between(1., cosInner) + between(1., cosOuter)) / (2. - cosInner - cosOuter);
            if (theta > M_PI - halfAngle) return (between(cosInner, -1.) + between(cosOuter, -1.)) / (2. + cosInner + cosOuter);
            return between(cosInner, cosOuter) / (cosInner - cosOuter);
        }
        // the scattering cosine that belongs to a uniform deviate X, for |g| >= 1e-6 (DustMix.cpp:490-511: the inverse of the cumulative
        // distribution); next to |g| = 1e-6 and |g| = 1 the result can leave [-1, 1] by rounding, which directionAbout absorbs
        // (below that asymmetry the scattering event draws an isotropic direction instead: DustMix.cpp:501)
        static __device__ __forceinline__ bool isotropic(double g) { return fabs(g) < 1e-6; }
        static __device__ __forceinline__ double cosineFor(double g, double X)
        {
            double f = ((1.0 - g) * (1.0 + g)) / (1.0 - g + 2.0 * g * X);
            return (1.0 + g * g - f * f) / (2.0 * g);
        }
    };

    // Dipole phase function of Thomson scattering by free electrons, unpolarized (DipolePhaseFunction.cpp:47-59): its value for a
    // scattering cosine, and the cosine that belongs to a uniform deviate X (the inverse of the cumulative distribution, a cubic).
    // The operations are the reference's, in its order.
    struct PhaseDipole
    {
        static __device__ __forceinline__ double value(double c) { return 0.75 * (c * c + 1.); }
        static __device__ __forceinline__ double cosineFor(double X)
        {
            const double p = cbrt(4. * X - 2. + sqrt(16. * X * (X - 1.) + 5.));
            return p - 1. / p;
        }
    };
    // value of the phase function of medium component h (asymmetry parameter g where it is Henyey-Greenstein) for a scattering cosine
    // (DustMix.cpp:430-445, DipolePhaseFunction.cpp:122-133).  DIPOLE: the kernel flavour of a scene in which some component has the
    // dipole; the other flavour never looks at the kinds.
    template<bool DIPOLE> __device__ __forceinline__ double phaseValue(const DevScene& S, int h, double g, double costheta)
    {
        if (DIPOLE && S.phase_kind[h] == PMC_PHASE_DIPOLE) return PhaseDipole::value(costheta);
        const PhaseHG phase(g);
        return fabs(g) > 0.95 ? phase.coneMean(costheta) : phase.value(costheta);
    }

    // Direction(theta, phi) + Random::direction() (Direction.cpp:11-38, Random.cpp:121-126)
    // (the core: the direction that belongs to the two uniform deviates u1 (inclination) and u2 (azimuth))
    __device__ __forceinline__ void randomDirectionFor(double u1, double u2, double& kx, double& ky, double& kz)
    {
        double theta = acos(2.0 * u1 - 1.0);
        double phi = 2.0 * M_PI * u2;
        const double eps = 1e-8;
        if (theta <= eps)
        {
            kx = 0, ky = 0, kz = 1;
        }
        else if (theta >= M_PI - eps)
        {
            kx = 0, ky = 0, kz = -1;
        }
        else
        {
            double sintheta, costheta, sinphi, cosphi;
            sincos(theta, &sintheta, &costheta);
            sincos(phi, &sinphi, &cosphi);
            kx = sintheta * cosphi;
            ky = sintheta * sinphi;
            kz = costheta;
        }
    }
    __device__ __forceinline__ void randomDirection(Rng& rng, uint64_t seed, double& kx, double& ky, double& kz)
    {
        const double u1 = rngUniform(rng, seed);
        const double u2 = rngUniform(rng, seed);
        randomDirectionFor(u1, u2, kx, ky, kz);
    }

    __device__ __forceinline__ double interpolateLogLog(double x, double x1, double x2, double f1, double f2)
    {
        if (f1 <= 0 || f2 <= 0)
        {
            if (x == x1) return f1;
            if (x == x2) return f2;
            return 0;
        }
        return f1 * exp(log(x / x1) / log(x2 / x1) * (log(f2 / f1)));
    }
    // Lower branch W_-1 of the Lambert function on [-1/e, 0) (SpecialFunctions.cpp:578-625; the radius of an exponential
    // disk: ExpDiskGeometry.cpp:47-51): a twelve-term series in -sqrt(z + 1/e) by Horner's rule -- exact enough next to the
    // branch point -- then Halley iterations on w e^w = z, started from the series or, near zero, from the asymptotic
    // form log(-z) - log(-log(-z)) + ...  (the same sequence of operations as the host layer's lambertLowerBranch)
    __device__ __noinline__ double lambertLowerBranch(double z)
    {
        const double inverseE = 0.3678794411714423215955237701614608;
        const double series[12] = {-1.0, 2.331643981597124203363536062168, -1.812187885639363490240191647568,
                                   1.936631114492359755363277457668, -2.353551201881614516821543561516,
                                   3.066858901050631912893148922704, -4.175335600258177138854984177460,
                                   5.858023729874774148815053846119, -8.401032217523977370984161688514,
                                   12.250753501314460424, -18.100697012472442755, 27.029044799010561650};
        if (z == 0.0) return -DBL_MAX;
        const double fromBranchPoint = z + inverseE;
        const double root = -sqrt(fromBranchPoint);
        double estimate = series[11];
#pragma unroll
        for (int term = 10; term >= 0; --term) estimate = series[term] + root * estimate;
        if (fromBranchPoint < 3.0e-3) return estimate;
        double w = estimate;
        if (!(z < -1e-6))
        {
            const double outer = log(-z);
            const double inner = log(-outer);
            w = outer - inner + inner / outer;
        }
        for (int round = 0; round < 10; ++round)
        {
            const double ew = exp(w);
            const double next = w + 1.0;
            double correction = w * ew - z;
            correction /= ew * next - 0.5 * (next + 1.0) * correction / next;
            w -= correction;
            if (fabs(correction) < 1.0e-12 * (1.0 + fabs(w))) break;
        }
        return w;  // (ten rounds always suffice on [-1/e, 0]; the reference would raise "no convergence")
    }

    // generalised exponential (1 + (1 - p) x)^(1 / (1 - p)) -> e^x for p -> 1 (SpecialFunctions.cpp:822-836): the inverse of the
    // cumulative distribution of a power-law segment (Random::cdfLogLog).  Close to p = 1 the power loses its digits and
    // the third-order expansion in (1 - p) takes over.
    __device__ __noinline__ double generalizedExp(double p, double x)
    {
        const double deficit = 1.0 - p;
        if (deficit == 0.0) return exp(x);
        if (!(fabs(deficit) < 1e-3)) return pow(1.0 + deficit * x, 1.0 / deficit);
        const double xx = x * x;
        const double first = 0.5 * xx * deficit;
        const double second = 1.0 / 24.0 * x * xx * (8.0 + 3.0 * x) * deficit * deficit;
        const double third = 1.0 / 48.0 * xx * xx * (12.0 + 8.0 * x + xx) * deficit * deficit * deficit;
        return exp(x) * (1.0 - first + second - third);
    }

    struct Counters
    {
        uint32_t histories, paths, updates, scatterings, overflows;
#ifdef PMC_PROFILE
        long long tp[8];  // section timers (wave cycles), see PMC_T_STAMP
        long long tl;
#endif
    };

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
    // Random::direction(bfk, costheta) (Random.cpp:130-164): a direction at the given inclination to k, uniform in azimuth
    // (the core: the azimuth comes from the uniform deviate u)
    __device__ __forceinline__ void directionAboutFor(double u, double kx, double ky, double kz, double costheta, double& kxn, double& kyn, double& kzn)
    {
        double phi = 2.0 * M_PI * u;
        double sinphi, cosphi;
        sincos(phi, &sinphi, &cosphi);
        double sintheta = sqrt(fabs((1.0 - costheta) * (1.0 + costheta)));
        if (kz > 0.99999)
        {
            kxn = cosphi * sintheta;
            kyn = sinphi * sintheta;
            kzn = costheta;
        }
        else if (kz < -0.99999)
        {
            kxn = cosphi * sintheta;
            kyn = sinphi * sintheta;
            kzn = -costheta;
        }
        else
        {
            double root = sqrt((1.0 - kz) * (1.0 + kz));
            kxn = sintheta / root * (-kx * kz * cosphi + ky * sinphi) + kx * costheta;
            kyn = -sintheta / root * (ky * kz * cosphi + kx * sinphi) + ky * costheta;
            kzn = root * sintheta * cosphi + kz * costheta;
        }
    }
    __device__ __forceinline__ void directionAbout(Rng& rng, uint64_t seed, double kx, double ky, double kz, double costheta, double& kxn, double& kyn,
                                                   double& kzn)
    {
        directionAboutFor(rngUniform(rng, seed), kx, ky, kz, costheta, kxn, kyn, kzn);
    }
    // probability of the direction k for the emission of a point source with an axisymmetric angular distribution, relative to isotropic
    // emission (AxAngularDistribution.cpp:27-30; LaserAngularDistribution.cpp:11-16, ConicalAngularDistribution.cpp:19-25,
    // NetzerAngularDistribution.cpp:34-38): the bias of an emission peel-off packet (PhotonPacket.cpp:78)
    __device__ __forceinline__ double angularProbability(const DevSource& Q, double kx, double ky, double kz)
    {
        const double costheta = Q.angular_axis[0] * kx + Q.angular_axis[1] * ky + Q.angular_axis[2] * kz;
        if (Q.angular_kind == PMC_ANGULAR_LASER) return costheta > 0.99999 ? INFINITY : 0.;
        if (Q.angular_kind == PMC_ANGULAR_CONICAL) return fabs(costheta) > Q.angular_cos_delta ? 1.0 / (1.0 - Q.angular_cos_delta) : 0.;
        const double sign = costheta > 0 ? 1. : -1;
        return (6. / 7.) * costheta * (2. * costheta + sign);
    }
    // weight factor of a scattering peel-off packet towards instrument I (DustMix.cpp:430-445, MediumSystem.cpp:734-767)
    template<bool DIPOLE>
    __device__ __forceinline__ double scatteringPeelFactor(const DevScene& S, double g, double kx, double ky, double kz, const DevInstrument& I)
    {
        double costheta = kx * I.kx + ky * I.ky + kz * I.kz;
        double value = phaseValue<DIPOLE>(S, 0, g, costheta);
        return 0. + value * 1.;
    }
    // taumax of MediumSystem::getExtinctionOpticalDepth (MediumSystem.cpp:1195-1199); -inf flags a dead packet
    __device__ __forceinline__ double peelTaumax(double pW, double lambda)
    {
        const double lum = pW / lambda;
        if (lum <= 0) return -INFINITY;
        return log(lum) + 745;
    }

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
