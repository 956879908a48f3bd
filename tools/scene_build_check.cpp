// Stand-alone check of scene creation's host code (skirt9_amd/csrc/pmc_scene_build.h, pmc_tables.h): the stages of pmc_create on a scene
// file (skh_scene_save), through a sink that keeps nothing and hashes everything.  No device, meant to be built with the sanitizers:
//   g++ -std=c++17 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_build_check.cpp
//       -Lskirt9_amd/lib -lskirthost -pthread -o scene_build_check
// (tests/test_scene_build.py does that).
//   scene_build_check FILE [--tree-as-bintree] [--cell-shuffle G] [--cell-order-ref] [--link-count-max N] [--cone-cull-only] [--defects]
// prints one line per sink call, in order -- "upload <element bytes> <count> <fnv1a-64>" or "allocate <bytes> <zero>" -- and a last line
// "devscene <fnv1a-64>" of the DevScene bytes (the sink hands out null pointers); then the structural invariants of the grid tables and of the
// LDS plan are checked on the builders' own vectors.  --defects: the loaded scene with one field broken at a time must be refused by
// checkScene with the code and the text that pmc_create has always given.  Exit status 0: all of it held.
#include "../skirt9_amd/csrc/pmc_scene_build.h"
#include "../include/skirt_host.h"
#include <cstdio>
#include <functional>
#include <set>
#include <utility>

namespace
{
    std::string lastError;
    int failures = 0;
    void complain(const std::string& what)
    {
        std::printf("FAIL %s\n", what.c_str());
        ++failures;
    }
    void require(bool ok, const std::string& what)
    {
        if (!ok) complain(what);
    }

    unsigned long long fnv1a(const void* data, size_t bytes)
    {
        unsigned long long h = 14695981039346656037ull;
        const unsigned char* p = static_cast<const unsigned char*>(data);
        for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
        return h;
    }

    struct HashSink final : TableSink
    {
        int uploadBytes(const void* host, size_t elementBytes, size_t count, const void** out) override
        {
            std::printf("upload %zu %zu %016llx\n", elementBytes, count, fnv1a(host, elementBytes * count));
            *out = nullptr;
            return PMC_OK;
        }
        int allocateBytes(size_t bytes, void** out, bool zero) override
        {
            std::printf("allocate %zu %d\n", bytes, zero ? 1 : 0);
            *out = nullptr;
            return PMC_OK;
        }
        size_t freeBytes() override { return ~size_t(0); }
    };

    // ---- invariants of the tree tables
    void checkPermutation(const std::vector<int32_t>& perm, const std::vector<int32_t>& cellExt, const std::string& what)
    {
        bool ok = true;
        size_t named = 0;
        for (size_t m = 0; m < perm.size() && ok; ++m) ok = perm[m] >= 0 && size_t(perm[m]) < cellExt.size() && cellExt[perm[m]] == int32_t(m);
        for (size_t dev = 0; dev < cellExt.size() && ok; ++dev)
        {
            if (cellExt[dev] < 0) continue;  // padding
            ok = size_t(cellExt[dev]) < perm.size() && perm[cellExt[dev]] == int32_t(dev);
            ++named;
        }
        require(ok && named == perm.size(), what + ": cellExt and perm are not inverse permutations");
    }
    void checkNeighbourLists(const std::vector<int32_t>& nbrStart, const std::vector<int32_t>& nbrList, size_t cellSlots, const std::string& what)
    {
        bool ok = nbrStart.size() == 6 * cellSlots + 1 && nbrStart.front() == 0 && size_t(nbrStart.back()) == nbrList.size();
        for (size_t i = 1; i < nbrStart.size() && ok; ++i) ok = nbrStart[i - 1] <= nbrStart[i];
        for (int32_t dev : nbrList) ok = ok && dev >= 0 && size_t(dev) < cellSlots;
        require(ok, what + ": a neighbour list leaves its table");
    }

    void checkOctree(const pmc_grid& g, const double* density, const SceneSwitches& sw)
    {
        TreeBuild T;
        if (buildTree(g, density, sw, T) != PMC_OK) return complain("buildTree: " + lastError);
        checkPermutation(T.perm, T.cellExt, "octree");
        checkNeighbourLists(T.nbrStart, T.nbrList, size_t(T.cellSlots), "octree");
        const auto linkOk = [&](uint32_t link) {
            if (link == PMC_LINK_NONE) return true;
            const size_t index = (link >> PMC_LINK_EXP_BITS) & PMC_LINK_INDEX_MASK;
            if (int(link & PMC_LINK_EXP_MASK) > T.lmax) return false;
            if (link & PMC_LINK_NODE) return index < T.internals.size();
            if (link & PMC_LINK_OCTET) return index + 7 < size_t(T.cellSlots);
            return index < size_t(T.cellSlots);
        };
        bool ok = linkOk(T.rootLink) && T.rootLink != PMC_LINK_NONE;
        for (const CellRec& c : T.cells)
            for (uint32_t link : c.link) ok = ok && linkOk(link);
        for (const NodeRec& n : T.internals)
            for (uint32_t link : n.child) ok = ok && linkOk(link) && link != PMC_LINK_NONE;
        for (uint32_t link : T.coarse) ok = ok && linkOk(link) && link != PMC_LINK_NONE;
        require(ok, "octree: a link index is outside its table");
        require(T.table.size() == 3 * size_t(T.tabn) && T.coarse.size() == size_t(1) << (3 * T.coarseLevel) && T.cells.size() == size_t(T.cellSlots)
                    && T.leaves.size() == size_t(T.cellSlots),
                "octree: table sizes");
    }

    void checkBinTree(const pmc_grid& g, const double* density)
    {
        BinTreeBuild B;
        if (buildBinTree(g, density, B) != PMC_OK) return complain("buildBinTree: " + lastError);
        const size_t numCells = size_t(g.num_cells);
        checkPermutation(B.perm, B.cellExt, "binary tree");
        checkNeighbourLists(B.nbrStart, B.nbrList, numCells, "binary tree");
        const auto linkOk = [&](int32_t link, bool outsideAllowed) {
            if (link >= 0) return size_t(link) < numCells;
            if (link == PMC_BIN_OUTSIDE) return outsideAllowed;
            return size_t(-2 - int64_t(link)) < B.nodes.size();
        };
        bool ok = linkOk(B.rootLink, false) && B.cells.size() == numCells && B.density.size() == numCells;
        for (const BinCellRec& c : B.cells)
            for (int32_t link : c.link) ok = ok && linkOk(link, true);
        for (const BinNodeRec& n : B.nodes) ok = ok && n.axis >= 0 && n.axis < 3 && linkOk(n.child[0], false) && linkOk(n.child[1], false);
        require(ok, "binary tree: a link index is outside its table");
    }

    // ---- invariants of the Voronoi tables
    // a table of runs: every entry index is inside the grid, every tag names the start word of the neighbour it carries, every run ends inside the
    // table including its padding.  Returns the number of runs whose count the link cannot name
    int checkRuns(const pmc_grid& g, const double* density, const std::vector<double>& entries, const std::vector<int32_t>& first, const SceneSwitches& sw,
                  const std::string& what)
    {
        constexpr size_t LANES = PMC_VORO_RUN_LANES, GROUP_UNITS = LANES / 2;
        VoroRuns R;
        if (voroPackRuns(g, density, entries, first, sw.voroLinkCountMax, R) != PMC_OK)
        {
            complain(what + ": " + lastError);
            return 0;
        }
        const size_t ncell = size_t(g.num_cells), units = R.runs.size() / 8;
        bool ok = R.start.size() == ncell + 1 && R.runs.size() % 8 == 0 && first.size() == ncell + 1 && size_t(first[ncell]) * 4 == entries.size();
        int unknown = 0;
        for (size_t m = 0; m < ncell && ok; ++m)
        {
            const size_t unit = R.start[m] & PMC_VORO_RUN_UNIT_MASK;
            const uint32_t linkCount = R.start[m] >> PMC_VORO_RUN_UNIT_BITS;
            const size_t count = size_t(first[m + 1] - first[m]), groups = (count + LANES - 1) / LANES;
            ok = unit + 1 + GROUP_UNITS * groups <= units;  // (the padding included)
            if (!ok) break;
            int32_t headCount[2];
            std::memcpy(headCount, &R.runs[8 * unit + 4], sizeof(double));
            ok = size_t(headCount[0]) == count && (linkCount == PMC_VORO_RUN_COUNT_UNKNOWN ? count > sw.voroLinkCountMax : linkCount == count);
            if (linkCount == PMC_VORO_RUN_COUNT_UNKNOWN) ++unknown;
            for (size_t e = 0; e < groups * LANES && ok; ++e)
            {
                const double* zt = &R.runs[8 * (unit + 1) + 4 * LANES * (e / LANES) + 2 * LANES + 2 * (e % LANES)];
                unsigned long long tag;
                std::memcpy(&tag, &zt[1], sizeof(double));
                const int mi = int(int32_t(uint32_t(tag)));
                if (e >= count)
                    ok = tag == (unsigned long long)(uint32_t)(-7);
                else if (mi >= 0)
                    ok = size_t(mi) < ncell && uint32_t(tag >> 32) == R.start[mi];
                else
                    ok = mi >= -6 && (tag >> 32) == 0;
            }
        }
        require(ok, what + ": a run or a tag leaves its table");
        return unknown;
    }

    void checkVoronoi(const pmc_scene& scene, const double* density, const SceneSwitches& sw)
    {
        const pmc_grid& g = scene.grid;
        const size_t ncell = size_t(g.num_cells);
        const std::vector<double> all = voroAllEntries(g);
        const std::vector<uint32_t> cull = voroCullMasks(g);
        require(all.size() == 4 * size_t(g.vnbr_start[ncell]) && cull.size() == ncell * PMC_VORO_CONES, "Voronoi: table sizes");
        int unknown = checkRuns(g, density, all, std::vector<int32_t>(g.vnbr_start, g.vnbr_start + ncell + 1), sw, "Voronoi runs of all neighbours");
        // per main cone: the kept neighbours of every cell, as sets of list positions
        std::vector<std::vector<double>> keptOfCone(48);
        std::vector<std::vector<int32_t>> firstOfCone(48);
        for (int c = 0; c < 48; ++c)
        {
            voroKeptOfCone(g, all, cull, c, keptOfCone[c], firstOfCone[c]);
            unknown += checkRuns(g, density, keptOfCone[c], firstOfCone[c], sw, "Voronoi runs of cone " + std::to_string(c));
        }
        for (int i = 0; i < scene.num_instruments; ++i)
        {
            const pmc_instrument& ins = scene.instruments[i];
            if (ins.same_observer_as_preceding) continue;
            const std::string what = "Voronoi runs of the observer of instrument " + std::to_string(i);
            std::vector<double> kept;
            std::vector<int32_t> first;
            const bool exactCull = !sw.voroConeCullOnly;
            voroKeptOfObserver(g, all, cull, ins.kobs, exactCull, kept, first);
            unknown += checkRuns(g, density, kept, first, sw, what);
            const int cone = voroConeOf(ins.kobs[0], ins.kobs[1], ins.kobs[2]);
            require(cone >= 0 && cone < PMC_VORO_CONES, what + ": cone out of range");
            const int mainCone = PMC_VORO_CONES == 192 ? cone / 4 : cone;
            bool subset = true, ahead = true;
            for (size_t m = 0; m < ncell; ++m)
            {
                std::multiset<int> ofCone;
                for (int32_t q = firstOfCone[mainCone][m]; q < firstOfCone[mainCone][m + 1]; ++q) ofCone.insert(voroEntryIndex(&keptOfCone[mainCone][4 * size_t(q)]));
                for (int32_t q = first[m]; q < first[m + 1]; ++q)
                {
                    const double* e = &kept[4 * size_t(q)];
                    const int mi = voroEntryIndex(e);
                    const auto found = ofCone.find(mi);
                    if (found == ofCone.end())
                        subset = false;
                    else
                        ofCone.erase(found);
                    if (exactCull && mi >= 0)
                    {
                        const double nx = e[0] - g.site[3 * m], ny = e[1] - g.site[3 * m + 1], nz = e[2] - g.site[3 * m + 2];
                        if (!(nx * ins.kobs[0] + ny * ins.kobs[1] + nz * ins.kobs[2] > 0)) ahead = false;
                    }
                }
            }
            require(subset, what + ": a kept entry that its cone does not keep");
            require(ahead, what + ": a kept site entry with n . k_obs <= 0");
        }
        if (sw.voroLinkCountMax < PMC_VORO_RUN_COUNT_UNKNOWN - 1u)
            require(unknown > 0, "Voronoi: no run has more entries than the lowered link count limit: the path is not exercised");
    }

    void checkLdsPlan(const LdsPlan& P, int gridLen, int sersicDoubles, int numLambda)
    {
        const std::pair<int, int> regions[] = {{P.sed_off, P.sed_len},
                                               {P.hot_off, PMC_LDS_HOT_DOUBLES},
                                               {P.sort_off, PMC_LDS_SORT_DOUBLES},
                                               {P.src_off, sersicDoubles},
                                               {P.dust_off, P.dust_in_lds ? numLambda : 0}};
        bool ok = P.sed_off == 0;
        int end = 0, sum = 0;
        for (int r = 0; r < 5; ++r)
        {
            ok = ok && regions[r].second >= 0 && regions[r].first >= end;  // (in order, none inside another)
            end = regions[r].first + regions[r].second;
            sum += regions[r].second;
            if (r == 2) ok = ok && P.total_transition == sum && end == sum;
        }
        ok = ok && P.total_launch == sum && end == sum && P.total_walk == gridLen;
        ok = ok && P.walkBytes == 8 * size_t(P.total_walk) && P.transitionBytes == 8 * size_t(P.total_transition) && P.launchBytes == 8 * size_t(P.total_launch);
        require(ok, "LDS plan: regions overlap or the totals are not the sum of the parts");
    }

    // ---- defective scenes: one field broken at a time
    void expectRefused(const char* what, const pmc_scene& scene, const pmc_scene_ext* ext, int code, const std::string& text)
    {
        SceneExtension X;
        lastError.clear();
        const int rc = checkScene(scene, ext, X);
        if (rc != code || lastError != text)
            complain(std::string("defect '") + what + "': code " + std::to_string(rc) + " \"" + lastError + "\", expected " + std::to_string(code) + " \"" + text + "\"");
    }

    void checkDefects(const pmc_scene& loaded, const pmc_scene_ext& loadedExt)
    {
        const int INVALID = PMC_ERR_INVALID, UNSUPPORTED = PMC_ERR_UNSUPPORTED;
        pmc_scene base = loaded;
        if (base.num_sources > 1) base.source = base.sources[0];
        if (base.num_media > 1) base.medium = base.media[0];
        base.num_sources = 1, base.num_media = 1;
        base.radiation_field.store = 0;
        pmc_scene_ext baseExt = loadedExt;
        for (pmc_source_velocity& v : baseExt.source_velocity) v = pmc_source_velocity{};
        {
            SceneExtension X;
            require(checkScene(base, &baseExt, X) == PMC_OK && checkScene(base, nullptr, X) == PMC_OK, "defects: the unbroken scene is refused: " + lastError);
        }
        // a broken copy of the scene (instruments, media and sources in arrays of the copy's own)
        struct Broken
        {
            pmc_scene scene;
            pmc_scene_ext ext;
            std::vector<pmc_instrument> instruments;
            std::vector<pmc_medium> media;
            std::vector<pmc_source> sources;
            std::vector<uint64_t> sourceFirst;
        };
        const auto with = [&](const std::function<void(Broken&)>& breakIt, const char* what, int code, const std::string& text, bool withExt = true) {
            Broken b{base, baseExt, std::vector<pmc_instrument>(base.instruments, base.instruments + base.num_instruments), {}, {}, {}};
            b.scene.instruments = b.instruments.data();
            breakIt(b);
            expectRefused(what, b.scene, withExt ? &b.ext : nullptr, code, text);
        };
        const auto severalMedia = [](Broken& b, int n) {
            b.media.assign(n, b.scene.medium);
            b.scene.num_media = n, b.scene.media = b.media.data();
        };
        const auto severalSources = [](Broken& b, int n) {
            b.sources.assign(n, b.scene.source);
            b.sourceFirst.assign(n + 1, 0);
            b.scene.num_sources = n, b.scene.sources = b.sources.data(), b.scene.source_first = b.sourceFirst.data();
        };
        const auto moving = [](Broken& b) {
            b.scene.source.lambda_mode = PMC_LAMBDA_TABULATED;
            b.ext.source_velocity[0].kind = PMC_VELOCITY_CONSTANT, b.ext.source_velocity[0].magnitude = 1e5;
        };
        with([](Broken& b) { b.scene.abi_version += 1; }, "ABI version", INVALID, "pmc_scene ABI version mismatch");
        with([](Broken& b) { b.ext.struct_size = 0; }, "extension size", INVALID, "pmc_scene_ext::struct_size is not set");
        with([](Broken& b) { b.ext.phase_function[0] = 7; }, "phase function", UNSUPPORTED, "unknown phase function kind 7 of medium component 0");
        with([](Broken& b) { b.ext.source_velocity[0].kind = 9; }, "velocity kind", UNSUPPORTED, "unknown velocity kind 9 of source 0");
        with([&](Broken& b) { moving(b), severalMedia(b, 2); }, "moving, two components", UNSUPPORTED, "a moving source together with more than one medium component");
        with([&](Broken& b) { moving(b), b.scene.radiation_field.store = 1; }, "moving, stored field", UNSUPPORTED, "a moving source together with a stored radiation field");
        with([&](Broken& b) { moving(b), b.instruments[0].nxp = 1 << 14, b.instruments[0].nyp = 1 << 14; }, "moving, large instrument", UNSUPPORTED,
             "a moving source together with an instrument of 2^28 pixels or more");
        with([&](Broken& b) { severalMedia(b, PMC_MAX_MEDIA + 1); }, "too many components", UNSUPPORTED, "more than PMC_MAX_MEDIA medium components");
        with([](Broken& b) { b.scene.num_media = 2, b.scene.media = nullptr; }, "media missing", INVALID, "num_media > 1 without pmc_scene::media");
        with([](Broken& b) { b.scene.num_instruments = 0; }, "no instrument", UNSUPPORTED, "between 1 and 16 instruments are supported");
        with([](Broken& b) { b.instruments.resize(17, b.instruments[0]), b.scene.instruments = b.instruments.data(), b.scene.num_instruments = 17; }, "17 instruments",
             UNSUPPORTED, "between 1 and 16 instruments are supported");
        with([](Broken& b) { b.scene.grid.kind = 9; }, "grid kind", UNSUPPORTED, "unsupported grid kind");
        with([](Broken& b) { b.instruments[0].same_observer_as_preceding = 1; }, "first observer shared", INVALID, "first instrument cannot share an observer");
        with([](Broken& b) { b.scene.medium.number_density = nullptr; }, "no density", INVALID, "medium component 0 without number_density");
        with([&](Broken& b) { severalMedia(b, 2), b.media[0].number_density = nullptr; }, "no density of component 0 of two", INVALID, "medium component 0 without number_density");
        if (base.grid.kind == PMC_GRID_CARTESIAN)
            with([](Broken& b) { b.scene.grid.num_cells += 1; }, "Cartesian cell count", INVALID, "Cartesian grid: cell count does not match the border arrays");
        with([](Broken& b) { b.scene.grid.kind = PMC_GRID_VORONOI, b.scene.grid.site = nullptr; }, "Voronoi tables", INVALID, "Voronoi grid tables are missing");
        {
            // (one cell whose only neighbour does not exist)
            static const double site[3] = {0., 0., 0.};
            static const int32_t nbrStart[2] = {0, 1}, nbrList[1] = {5}, blockStart[2] = {0, 1}, blockList[1] = {0};
            with([](Broken& b) {
                pmc_grid& g = b.scene.grid;
                g.kind = PMC_GRID_VORONOI, g.num_cells = 1, g.site = site, g.vnbr_start = nbrStart, g.vnbr_list = nbrList;
                g.vblock_n = 1, g.vblock_start = blockStart, g.vblock_list = blockList;
            }, "Voronoi neighbour", INVALID, "Voronoi neighbour list holds an invalid index");
        }
        with([](Broken& b) { b.scene.options.explicit_absorption = 1, b.scene.medium.sigma_abs = nullptr; }, "explicit absorption", INVALID,
             "explicit absorption needs pmc_medium::sigma_abs");
        with([&](Broken& b) { severalMedia(b, 2), b.media[1].sigma_ext = nullptr; }, "incomplete component", INVALID, "incomplete medium component 1");
        with([&](Broken& b) { severalMedia(b, 3), b.media[2].num_lambda = 0; }, "empty component", INVALID, "incomplete medium component 2");
        with([&](Broken& b) {
            b.scene.options.explicit_absorption = 1, b.scene.medium.sigma_abs = b.scene.medium.sigma_ext;
            severalMedia(b, 2), b.media[1].sigma_abs = nullptr;
        }, "explicit absorption, second component", INVALID, "explicit absorption needs pmc_medium::sigma_abs of every component");
        with([&](Broken& b) { severalSources(b, PMC_MAX_SOURCES + 1); }, "too many sources", UNSUPPORTED, "more than 16 sources");
        with([](Broken& b) { b.scene.num_sources = 2, b.scene.sources = nullptr; }, "source table missing", INVALID, "source tables missing");
        with([&](Broken& b) { severalSources(b, 2), b.scene.source_first = nullptr; }, "source ranges missing", INVALID, "source tables missing", false);
        with([](Broken& b) { b.scene.source.kind = PMC_SOURCE_POINT, b.scene.source.angular_kind = 9; }, "angular distribution", UNSUPPORTED,
             "unsupported angular distribution");
        with([](Broken& b) { b.scene.source.kind = PMC_SOURCE_SERSIC, b.scene.source.sersic_n = 1; }, "Sersic tables", INVALID, "Sersic source without tables");
        with([](Broken& b) { b.scene.source.kind = 99; }, "source kind", UNSUPPORTED, "unsupported source kind");
        with([](Broken& b) { b.scene.source.lambda_mode = PMC_LAMBDA_OLIGO, b.scene.source.num_oligo = 0; }, "no wavelengths", INVALID,
             "oligochromatic source without wavelengths");
        with([](Broken& b) { b.scene.source.lambda_mode = PMC_LAMBDA_TABULATED, b.scene.source.num_sed = 1; }, "no SED", INVALID, "tabulated source without SED table");
        with([](Broken& b) { b.scene.source.lambda_mode = 7; }, "wavelength mode", UNSUPPORTED, "unsupported wavelength sampling mode");
        with([&](Broken& b) {
            b.scene.source.lambda_mode = PMC_LAMBDA_OLIGO, b.scene.source.num_oligo = std::max(b.scene.source.num_oligo, 1);
            severalSources(b, 2);
            b.sources[1].lambda_mode = PMC_LAMBDA_TABULATED, b.sources[1].num_sed = 2;
        }, "wavelength regimes", INVALID, "sources with different wavelength regimes");
        with([](Broken& b) { b.instruments.back().redshift = -0.5; }, "redshift", INVALID, "negative instrument redshift");
        with([](Broken& b) { b.instruments[0].redshift = std::nan(""); }, "redshift not a number", INVALID, "negative instrument redshift");
        with([](Broken& b) { b.scene.radiation_field.store = 1, b.scene.options.force_scattering = 0; }, "stored field without forced scattering", INVALID,
             "the radiation field can only be stored with forced scattering (Configuration.cpp:476-482)");
        with([](Broken& b) { b.scene.radiation_field.store = 1, b.scene.options.force_scattering = 1, b.scene.radiation_field.border = nullptr; },
             "stored field without grid", INVALID, "radiation field wavelength grid is missing");
        // a shorter extension of an older caller: no velocities, and what lies beyond its size is not read
        {
            Broken b{base, baseExt, {}, {}, {}, {}};
            b.ext.struct_size = int32_t(offsetof(pmc_scene_ext, source_velocity)), b.ext.source_velocity[0].kind = 9;
            SceneExtension X;
            require(checkScene(b.scene, &b.ext, X) == PMC_OK && !X.moving, "defects: a velocity beyond the size of a shorter extension is read");
        }
    }
}

void pmcSetError(const std::string& message)
{
    lastError = message;
}

int main(int argc, char** argv)
{
    SceneSwitches sw;
    const char* path = nullptr;
    bool defects = false;
    for (int a = 1; a < argc; ++a)
    {
        const std::string arg = argv[a];
        if (arg == "--tree-as-bintree")
            sw.treeAsBinTree = true;
        else if (arg == "--cone-cull-only")
            sw.voroConeCullOnly = true;
        else if (arg == "--link-count-max" && a + 1 < argc)
            sw.voroLinkCountMax = std::min<uint32_t>(sw.voroLinkCountMax, (uint32_t)std::max(0, atoi(argv[++a])));
        else if (arg == "--cell-shuffle" && a + 1 < argc)
            sw.cellShuffle = atoi(argv[++a]);
        else if (arg == "--cell-order-ref")
            sw.cellOrderRef = true;
        else if (arg == "--defects")
            defects = true;
        else if (!path && arg[0] != '-')
            path = argv[a];
        else
            path = nullptr, a = argc;
    }
    if (!path)
    {
        std::fprintf(stderr, "usage: scene_build_check FILE [--tree-as-bintree] [--cell-shuffle G] [--cell-order-ref] [--link-count-max N] [--cone-cull-only] [--defects]\n");
        return 2;
    }
    skh_scene_file* file = skh_scene_load(path);
    if (!file)
    {
        std::fprintf(stderr, "scene_build_check: %s cannot be loaded\n", path);
        return 2;
    }
    const pmc_scene& scene = *skh_scene_file_scene(file);
    const pmc_scene_ext* ext = skh_scene_file_scene_ext(file);

    // the stages of pmc_create
    SceneExtension X;
    if (checkScene(scene, ext, X) != PMC_OK) complain("checkScene: " + lastError);
    if (!failures)
    {
        HashSink sink;
        DevScene D;
        std::memset(&D, 0, sizeof(D));
        SceneTables tables;
        if (buildSceneTables(scene, X, sw, sink, D, tables) != PMC_OK) complain("buildSceneTables: " + lastError);
        std::printf("devscene %016llx\n", fnv1a(&D, sizeof(D)));

        // the invariants, on the builders' own vectors
        const double* density = firstComponent(scene).number_density;
        const int sersicDoubles = numSourcesOf(scene) == 1 && sourceOf(scene, 0).kind == PMC_SOURCE_SERSIC ? 2 * sourceOf(scene, 0).sersic_n : 0;
        checkLdsPlan(tables.lds, D.lds_grid_len, sersicDoubles, D.num_lambda);
        if (scene.grid.kind == PMC_GRID_VORONOI)
            checkVoronoi(scene, density, sw);
        else if (scene.grid.kind == PMC_GRID_BINTREE || (scene.grid.kind == PMC_GRID_OCTREE && sw.treeAsBinTree))
            checkBinTree(scene.grid, density);
        else if (scene.grid.kind == PMC_GRID_OCTREE)
            checkOctree(scene.grid, density, sw);
        if (defects) checkDefects(scene, ext ? *ext : pmc_scene_ext{int32_t(sizeof(pmc_scene_ext)), {}, {}});
    }
    skh_scene_file_free(file);
    std::printf("%s\n", failures ? "scene build: FAILED" : "scene build: ok");
    return failures ? 1 : 0;
}
