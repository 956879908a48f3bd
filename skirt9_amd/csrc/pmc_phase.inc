// pmc_phase.inc -- phase functions and scalar sampling primitives (included by pmc_kernels.hip inside its anonymous namespace).
//
// Pure functions of their arguments and of a random stream: the Henyey-Greenstein and dipole phase functions, random directions,
// the special functions of the source sampling, and the weights of a peel-off packet.  Used by the transition kernel (onCycleDone,
// pmc_transition.inc), the launch kernel (launchHistory, pmc_launch.inc) and the cycle start (announceCycle, startCycleWalks,
// pmc_cycle.inc); the pmc_tune_device_function test aids (pmc_kernels.hip) run them one at a time.

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
