// Stand-alone check of pmcLaunchFlavourOf (skirt9_amd/csrc/pmc_device.h): the launch flavour selected for hand-filled source arrays.
// Plain host code, no device, meant to be built with the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/launch_flavour_check.cpp -o launch_flavour_check
// (tests/test_launch_flavour_selection.py does that).  Exit status 0: every case selects the expected flavour.
#include "../skirt9_amd/csrc/pmc_device.h"
#include <cstdio>
#include <cstring>
#include <vector>

namespace
{
    DevSource source(int kind, int lambdaMode, int angular)
    {
        DevSource q;
        std::memset(&q, 0, sizeof(q));
        q.source_kind = kind;
        q.lambda_mode = lambdaMode;
        q.angular_kind = angular;
        return q;
    }
    int flavour(int bits, int geometry) { return bits | (geometry << PMC_LAUNCH_GEOM_SHIFT); }

    int failures = 0;
    void expect(const char* what, const std::vector<DevSource>& src, int kin, int want)
    {
        // (exactly as many sources as the case has: the sanitizer sees a read past them)
        const int got = pmcLaunchFlavourOf(src.data(), int(src.size()), kin);
        if (got != want)
        {
            std::printf("FAIL %s: flavour %d, expected %d\n", what, got, want);
            ++failures;
        }
        if (got < 0 || got >= PMC_LAUNCH_FLAVOURS)
        {
            std::printf("FAIL %s: flavour %d is outside the kernel table\n", what, got);
            ++failures;
        }
    }
}

int main()
{
    const int O = PMC_LAMBDA_OLIGO, T = PMC_LAMBDA_TABULATED, ISO = PMC_ANGULAR_ISOTROPIC;
    expect("oligochromatic Sersic", {source(PMC_SOURCE_SERSIC, O, ISO)}, 0, flavour(PMC_LAUNCH_OLIGO | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_SERSIC));
    expect("sampled Sersic", {source(PMC_SOURCE_SERSIC, T, ISO)}, 0, flavour(PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_SERSIC));
    expect("moving sampled Sersic", {source(PMC_SOURCE_SERSIC, T, ISO)}, 1, flavour(PMC_LAUNCH_KIN | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_SERSIC));
    expect("oligochromatic point", {source(PMC_SOURCE_POINT, O, ISO)}, 0, flavour(PMC_LAUNCH_OLIGO | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_POINT));
    expect("conical point", {source(PMC_SOURCE_POINT, O, PMC_ANGULAR_CONICAL)}, 0, flavour(PMC_LAUNCH_OLIGO, PMC_LAUNCH_GEOM_POINT));
    expect("laser point, sampled", {source(PMC_SOURCE_POINT, T, PMC_ANGULAR_LASER)}, 0, flavour(0, PMC_LAUNCH_GEOM_POINT));
    expect("oligochromatic box", {source(PMC_SOURCE_UNIFORM_BOX, O, ISO)}, 0, flavour(PMC_LAUNCH_OLIGO | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_ANY));
    expect("sampled disk", {source(PMC_SOURCE_EXP_DISK, T, ISO)}, 0, flavour(PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_ANY));
    expect("moving Plummer", {source(PMC_SOURCE_PLUMMER, T, ISO)}, 1, flavour(PMC_LAUNCH_KIN | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_ANY));
    // several sources: point sources only keep a flavour (with what all of them share); every other system is the generic kernel's
    expect("two points", {source(PMC_SOURCE_POINT, T, ISO), source(PMC_SOURCE_POINT, T, ISO)}, 0, flavour(PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_POINT));
    expect("two points, one a cone", {source(PMC_SOURCE_POINT, O, ISO), source(PMC_SOURCE_POINT, O, PMC_ANGULAR_CONICAL)}, 0, flavour(PMC_LAUNCH_OLIGO, PMC_LAUNCH_GEOM_POINT));
    expect("two Sersic sources", {source(PMC_SOURCE_SERSIC, O, ISO), source(PMC_SOURCE_SERSIC, O, ISO)}, 0, 0);
    expect("Sersic, disk and point", {source(PMC_SOURCE_SERSIC, T, ISO), source(PMC_SOURCE_EXP_DISK, T, ISO), source(PMC_SOURCE_POINT, T, ISO)}, 0, 0);
    expect("moving mixed system", {source(PMC_SOURCE_EXP_DISK, T, ISO), source(PMC_SOURCE_POINT, T, ISO)}, 1, PMC_LAUNCH_KIN);
    expect("a full system of points", std::vector<DevSource>(PMC_MAX_SOURCES, source(PMC_SOURCE_POINT, O, ISO)), 0, flavour(PMC_LAUNCH_OLIGO | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_POINT));
    // no sources, more than a scene holds, no array: the generic kernel, nothing read
    expect("no source", {}, 0, 0);
    expect("three moving points", std::vector<DevSource>(3, source(PMC_SOURCE_POINT, O, ISO)), 1, PMC_LAUNCH_KIN | flavour(PMC_LAUNCH_OLIGO | PMC_LAUNCH_ISOTROPIC, PMC_LAUNCH_GEOM_POINT));
    if (pmcLaunchFlavourOf(nullptr, 2, 1) != PMC_LAUNCH_KIN || pmcLaunchFlavourOf(nullptr, PMC_MAX_SOURCES + 1, 0) != 0)
    {
        std::printf("FAIL null / oversized source array\n");
        ++failures;
    }
    std::printf("%s\n", failures ? "launch flavour selection: FAILED" : "launch flavour selection: ok");
    return failures ? 1 : 0;
}
