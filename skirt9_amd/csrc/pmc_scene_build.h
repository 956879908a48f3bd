// pmc_scene_build.h -- a scene (pmc_scene, pmc_scene_ext) becomes the scalars of DevScene and the tables behind its pointers: the stages of
// pmc_create that need no device.  Plain C++17, no HIP (pmc_tables.h holds the grid tables and the TableSink that every table goes to):
//   checkScene       everything that can be refused before a device is touched
//   buildSceneTables grid, media, sources, one-wavelength constants, instruments, radiation field, LDS plan, outputs -- in this order, which is the
//                    order of the device allocations
// pmc_create (pmc_api.hip) runs them between the context's resources and the device-side configuration; tools/scene_build_check.cpp runs them
// under the sanitizers with a sink that hashes what it is given.
#ifndef PMC_SCENE_BUILD_H
#define PMC_SCENE_BUILD_H

#include "pmc_tables.h"
#include "../../include/pmc_layout.h"
#include <cstddef>

namespace
{
    // ---- what the extension says of the scene (a shorter pmc_scene_ext of an older caller: Henyey-Greenstein, every source at rest)
    struct SceneExtension
    {
        int32_t phaseKind[PMC_MAX_MEDIA];
        pmc_source_velocity velocity[PMC_MAX_SOURCES];
        bool moving;
    };
    static_assert(PMC_EXT_MAX_SOURCES == PMC_MAX_SOURCES, "one velocity per source slot");

    inline int readExtension(const pmc_scene& scene, const pmc_scene_ext* ext, SceneExtension& X)
    {
        for (int h = 0; h < PMC_MAX_MEDIA; ++h) X.phaseKind[h] = PMC_PHASE_HG;
        std::memset(X.velocity, 0, sizeof(X.velocity));
        X.moving = false;
        if (!ext) return PMC_OK;
        if (ext->struct_size < int32_t(sizeof(int32_t))) return fail(PMC_ERR_INVALID, "pmc_scene_ext::struct_size is not set");
        const int components = scene.num_media > 1 ? scene.num_media : 1;
        for (int h = 0; h < components && h < PMC_MAX_MEDIA; ++h)
        {
            if (size_t(ext->struct_size) < offsetof(pmc_scene_ext, phase_function) + sizeof(int32_t) * size_t(h + 1)) break;
            X.phaseKind[h] = ext->phase_function[h];
            if (X.phaseKind[h] != PMC_PHASE_HG && X.phaseKind[h] != PMC_PHASE_DIPOLE)
                return fail(PMC_ERR_UNSUPPORTED, "unknown phase function kind " + std::to_string(X.phaseKind[h]) + " of medium component " + std::to_string(h));
        }
        const int sources = scene.num_sources > 1 ? scene.num_sources : 1;
        for (int i = 0; i < sources && i < PMC_MAX_SOURCES; ++i)
        {
            if (size_t(ext->struct_size) < offsetof(pmc_scene_ext, source_velocity) + sizeof(pmc_source_velocity) * size_t(i + 1)) break;
            X.velocity[i] = ext->source_velocity[i];
            if (X.velocity[i].kind < PMC_VELOCITY_NONE || X.velocity[i].kind > PMC_VELOCITY_CYLINDRICAL)
                return fail(PMC_ERR_UNSUPPORTED, "unknown velocity kind " + std::to_string(X.velocity[i].kind) + " of source " + std::to_string(i));
            // (SpecialtySource.cpp:34-44, GeometricSource.cpp:31-41: no velocity in an oligochromatic simulation; a scene without its source
            // table is refused below)
            if (scene.num_sources > 1 && !scene.sources) continue;
            const pmc_source& src = scene.num_sources > 1 ? scene.sources[i] : scene.source;
            if (src.lambda_mode == PMC_LAMBDA_OLIGO) X.velocity[i] = pmc_source_velocity{};
            if (X.velocity[i].kind != PMC_VELOCITY_NONE) X.moving = true;
        }
        return PMC_OK;
    }

    inline const pmc_medium& firstComponent(const pmc_scene& scene)
    {
        // component 0 of the medium system: pmc_scene::media[0] when there are several components (pmc.h: `media` replaces `medium` then, which
        // the caller may leave zeroed), else pmc_scene::medium.  Its cell densities go into the hot cell records, its dust tables into DevScene.
        return scene.num_media > 1 ? scene.media[0] : scene.medium;
    }
    inline int numSourcesOf(const pmc_scene& scene) { return scene.num_sources > 1 ? scene.num_sources : 1; }
    inline const pmc_source& sourceOf(const pmc_scene& scene, int si) { return scene.num_sources > 1 ? scene.sources[si] : scene.source; }

    inline int checkSource(const pmc_source& src)
    {
        const int angular = src.kind == PMC_SOURCE_POINT ? src.angular_kind : PMC_ANGULAR_ISOTROPIC;
        if (angular < PMC_ANGULAR_ISOTROPIC || angular > PMC_ANGULAR_NETZER) return fail(PMC_ERR_UNSUPPORTED, "unsupported angular distribution");
        if (src.kind == PMC_SOURCE_SERSIC)
        {
            if (src.sersic_n < 2) return fail(PMC_ERR_INVALID, "Sersic source without tables");
        }
        else if (src.kind != PMC_SOURCE_POINT && src.kind != PMC_SOURCE_UNIFORM_BOX && src.kind != PMC_SOURCE_EXP_DISK && src.kind != PMC_SOURCE_PLUMMER)
            return fail(PMC_ERR_UNSUPPORTED, "unsupported source kind");
        if (src.lambda_mode == PMC_LAMBDA_OLIGO)
        {
            if (src.num_oligo < 1) return fail(PMC_ERR_INVALID, "oligochromatic source without wavelengths");
        }
        else if (src.lambda_mode == PMC_LAMBDA_TABULATED)
        {
            if (src.num_sed < 2) return fail(PMC_ERR_INVALID, "tabulated source without SED table");
        }
        else
            return fail(PMC_ERR_UNSUPPORTED, "unsupported wavelength sampling mode");
        return PMC_OK;
    }

    // Everything that can be refused without a device, in the order in which pmc_create has always looked: a scene with one defect gets the code
    // and the text it always got.  Fills X.
    inline int checkScene(const pmc_scene& scene, const pmc_scene_ext* ext, SceneExtension& X)
    {
        if (scene.abi_version != PMC_ABI_VERSION) return fail(PMC_ERR_INVALID, "pmc_scene ABI version mismatch");
        if (int rc = readExtension(scene, ext, X)) return rc;
        if (X.moving && scene.num_media > 1) return fail(PMC_ERR_UNSUPPORTED, "a moving source together with more than one medium component");
        if (X.moving && scene.radiation_field.store) return fail(PMC_ERR_UNSUPPORTED, "a moving source together with a stored radiation field");
        if (X.moving)
            for (int i = 0; i < scene.num_instruments && scene.instruments; ++i)
                if (int64_t(scene.instruments[i].nxp) * scene.instruments[i].nyp >= (int64_t(1) << 28))
                    return fail(PMC_ERR_UNSUPPORTED, "a moving source together with an instrument of 2^28 pixels or more");
        if (scene.num_media > PMC_MAX_MEDIA) return fail(PMC_ERR_UNSUPPORTED, "more than PMC_MAX_MEDIA medium components");
        if (scene.num_media > 1 && !scene.media) return fail(PMC_ERR_INVALID, "num_media > 1 without pmc_scene::media");
        if (scene.num_instruments < 1 || scene.num_instruments > PMC_MAX_INSTRUMENTS)
            return fail(PMC_ERR_UNSUPPORTED, "between 1 and " + std::to_string(PMC_MAX_INSTRUMENTS) + " instruments are supported");
        const pmc_grid& g = scene.grid;
        if (g.kind != PMC_GRID_CARTESIAN && g.kind != PMC_GRID_OCTREE && g.kind != PMC_GRID_VORONOI && g.kind != PMC_GRID_BINTREE)
            return fail(PMC_ERR_UNSUPPORTED, "unsupported grid kind");
        if (scene.instruments[0].same_observer_as_preceding) return fail(PMC_ERR_INVALID, "first instrument cannot share an observer");
        // ---- grid and media
        const pmc_medium& med = firstComponent(scene);
        if (!med.number_density) return fail(PMC_ERR_INVALID, "medium component 0 without number_density");
        if (g.kind == PMC_GRID_CARTESIAN && int64_t(g.nx) * g.ny * g.nz != int64_t(g.num_cells))
            return fail(PMC_ERR_INVALID, "Cartesian grid: cell count does not match the border arrays");
        if (g.kind == PMC_GRID_VORONOI)
            if (int rc = checkVoronoiGrid(g)) return rc;
        const bool explicitAbsorption = scene.options.explicit_absorption != 0;
        if (explicitAbsorption && !med.sigma_abs) return fail(PMC_ERR_INVALID, "explicit absorption needs pmc_medium::sigma_abs");
        for (int h = 0; h < scene.num_media && scene.num_media > 1; ++h)
        {
            const pmc_medium& mh = scene.media[h];
            if (!mh.number_density || !mh.lambda_border || !mh.sigma_ext || !mh.sigma_sca || !mh.asymmpar || mh.num_lambda < 1)
                return fail(PMC_ERR_INVALID, "incomplete medium component " + std::to_string(h));
            if (explicitAbsorption && !mh.sigma_abs) return fail(PMC_ERR_INVALID, "explicit absorption needs pmc_medium::sigma_abs of every component");
        }
        // ---- sources
        const int numSources = numSourcesOf(scene);
        if (numSources > PMC_MAX_SOURCES) return fail(PMC_ERR_UNSUPPORTED, "more than " + std::to_string(PMC_MAX_SOURCES) + " sources");
        if (numSources > 1 && (!scene.sources || !scene.source_first)) return fail(PMC_ERR_INVALID, "source tables missing");
        for (int si = 0; si < numSources; ++si)
            if (int rc = checkSource(sourceOf(scene, si))) return rc;
        for (int si = 1; si < numSources; ++si)
            if (sourceOf(scene, si).lambda_mode != sourceOf(scene, 0).lambda_mode) return fail(PMC_ERR_INVALID, "sources with different wavelength regimes");
        // ---- instruments, radiation field
        for (int i = 0; i < scene.num_instruments; ++i)
            if (!(scene.instruments[i].redshift >= 0.)) return fail(PMC_ERR_INVALID, "negative instrument redshift");
        const pmc_radiation_field& RF = scene.radiation_field;
        if (RF.store)
        {
            if (!scene.options.force_scattering)
                return fail(PMC_ERR_INVALID, "the radiation field can only be stored with forced scattering (Configuration.cpp:476-482)");
            if (RF.num_lambda < 1 || RF.num_border < 1 || !RF.border || !RF.ellv) return fail(PMC_ERR_INVALID, "radiation field wavelength grid is missing");
        }
        return PMC_OK;
    }

    // ---- grid: one stage per kind.  devToCell: a tree's device cell index -> the caller's cell index (else empty: the same numbering)
    inline int uploadCartesianGrid(const pmc_grid& g, const double* density, TableSink& sink, DevScene& D)
    {
        int rc = PMC_OK;
        D.nx = g.nx, D.ny = g.ny, D.nz = g.nz;
        if ((rc = sink.upload(g.xv, size_t(g.nx) + 1, &D.xv))) return rc;
        if ((rc = sink.upload(g.yv, size_t(g.ny) + 1, &D.yv))) return rc;
        if ((rc = sink.upload(g.zv, size_t(g.nz) + 1, &D.zv))) return rc;
        if ((rc = sink.upload(density, size_t(g.num_cells), &D.cell_density))) return rc;
        D.lds_grid_len = (g.nx + 1) + (g.ny + 1) + (g.nz + 1);
        D.lmax = 0;
        return rc;
    }

    inline int uploadGrid(const pmc_scene& scene, const SceneSwitches& sw, TableSink& sink, DevScene& D, std::vector<int32_t>& devToCell)
    {
        const pmc_grid& g = scene.grid;
        const double* density = firstComponent(scene).number_density;
        D.grid_kind = g.kind;
        D.gx0 = g.xmin, D.gy0 = g.ymin, D.gz0 = g.zmin;
        D.gx1 = g.xmax, D.gy1 = g.ymax, D.gz1 = g.zmax;
        D.eps = g.eps;
        D.num_cells = g.num_cells;
        D.voro_defer_scan = 0;
        if (g.kind == PMC_GRID_CARTESIAN) return uploadCartesianGrid(g, density, sink, D);
        if (g.kind == PMC_GRID_VORONOI) return uploadVoronoiGrid(scene, density, sw, sink, D);
        // (an octree under the verification switch runs through the binary tree's tables and kernels: D.grid_kind becomes PMC_GRID_BINTREE)
        if (g.kind == PMC_GRID_BINTREE || sw.treeAsBinTree) return uploadBinTreeGrid(g, density, sink, D, devToCell);
        return uploadOctreeGrid(g, density, sw, sink, D, devToCell);
    }

    // ---- media: the dust tables of component 0; of several components every one's densities (in the device numbering of the cells) and tables
    inline int uploadMedia(const pmc_scene& scene, const SceneExtension& X, const std::vector<int32_t>& devToCell, TableSink& sink, DevScene& D)
    {
        const pmc_medium& med = firstComponent(scene);
        int rc = PMC_OK;
        D.num_lambda = med.num_lambda;
        if ((rc = sink.upload(med.lambda_border, size_t(med.num_lambda), &D.lambda_border))) return rc;
        if ((rc = sink.upload(med.sigma_ext, size_t(med.num_lambda), &D.sigma_ext))) return rc;
        if ((rc = sink.upload(med.sigma_sca, size_t(med.num_lambda), &D.sigma_sca))) return rc;
        if ((rc = sink.upload(med.asymmpar, size_t(med.num_lambda), &D.asymmpar))) return rc;
        D.explicit_absorption = scene.options.explicit_absorption ? 1 : 0;
        D.sigma_abs = nullptr;
        if (D.explicit_absorption && (rc = sink.upload(med.sigma_abs, size_t(med.num_lambda), &D.sigma_abs))) return rc;
        D.num_media = scene.num_media > 1 ? scene.num_media : 1;
        std::memset(D.med, 0, sizeof(D.med));
        if (D.num_media > 1)
        {
            const size_t slots = devToCell.empty() ? size_t(scene.grid.num_cells) : devToCell.size();
            std::vector<double> dens(slots);
            for (int h = 0; h < D.num_media; ++h)
            {
                const pmc_medium& mh = scene.media[h];
                // (without explicit absorption the absorption cross sections are loaded with the others but never used)
                const std::vector<double> noAbs(mh.sigma_abs ? 0 : mh.num_lambda, 0.);
                const double* const sigmaAbs = mh.sigma_abs ? mh.sigma_abs : noAbs.data();
                for (size_t dev = 0; dev < slots; ++dev)
                {
                    const int64_t m = devToCell.empty() ? int64_t(dev) : int64_t(devToCell[dev]);
                    dens[dev] = m >= 0 ? mh.number_density[m] : 0.;
                }
                DevMedium& M = D.med[h];
                M.num_lambda = mh.num_lambda;
                if ((rc = sink.upload(dens.data(), dens.size(), &M.density))) return rc;
                if ((rc = sink.upload(mh.lambda_border, size_t(mh.num_lambda), &M.lambda_border))) return rc;
                if ((rc = sink.upload(mh.sigma_ext, size_t(mh.num_lambda), &M.sigma_ext))) return rc;
                if ((rc = sink.upload(mh.sigma_sca, size_t(mh.num_lambda), &M.sigma_sca))) return rc;
                if ((rc = sink.upload(sigmaAbs, size_t(mh.num_lambda), &M.sigma_abs))) return rc;
                if ((rc = sink.upload(mh.asymmpar, size_t(mh.num_lambda), &M.asymmpar))) return rc;
            }
        }
        D.any_dipole = 0;
        for (int h = 0; h < PMC_MAX_MEDIA; ++h)
        {
            D.phase_kind[h] = h < D.num_media ? X.phaseKind[h] : PMC_PHASE_HG;
            if (D.phase_kind[h] == PMC_PHASE_DIPOLE) D.any_dipole = 1;
        }
        return rc;
    }

    inline void setOptions(const pmc_scene& scene, const SceneSwitches& sw, DevScene& D)
    {
        D.force_scattering = scene.options.force_scattering;
        D.voro_prop_checkpoints = sw.propNoCheckpoints ? 0 : 1;
        D.min_weight_reduction = scene.options.min_weight_reduction;
        D.min_scatt_events = scene.options.min_scatt_events;
        D.path_length_bias = scene.options.path_length_bias;
    }

    // ---- sources
    // NetzerAngularDistribution::setupSelfBefore (NetzerAngularDistribution.cpp:12-30; NR::buildLinearGrid, NR.hpp:203-209)
    inline void netzerTable(std::vector<double>& ct, std::vector<double>& X)
    {
        const int n = PMC_NETZER_POINTS;
        ct.assign(n + 1, 0.), X.assign(n + 1, 0.);
        const double dx = (+1. - -1.) / n;
        for (int i = 0; i <= n; i++) ct[i] = -1. + i * dx;
        X[0] = 0;
        for (int i = 1; i < n; i++)
        {
            const double c = ct[i];
            const double sign = c > 0 ? 1. : -1;
            X[i] = (1. / 2.) + (2. / 7.) * c * c * c + sign * (3. / 14.) * c * c;
        }
        X[n] = 1.;
    }

    // (sersicDoubles: what the launch kernel of a scene with ONE source, a Sersic profile, stages of its tables in LDS)
    inline int uploadSources(const pmc_scene& scene, const SceneExtension& X, TableSink& sink, DevScene& D, int& sersicDoubles)
    {
        int rc = PMC_OK;
        const int numSources = numSourcesOf(scene);
        D.num_sources = numSources;
        sersicDoubles = 0;
        bool netzer = false;
        for (int si = 0; si < numSources; ++si)
        {
            const pmc_source& src = sourceOf(scene, si);
            DevSource& Q = D.src[si];
            D.src_first[si] = numSources > 1 ? scene.source_first[si] : 0;
            Q.source_kind = src.kind;
            std::memcpy(Q.src_pos, src.position, sizeof(Q.src_pos));
            Q.reff = src.reff;
            Q.sersic_n = src.sersic_n;
            std::memcpy(Q.src_box, src.box, sizeof(Q.src_box));
            Q.packet_luminosity = src.packet_luminosity;
            Q.lambda_mode = src.lambda_mode;
            Q.num_oligo = src.num_oligo;
            Q.lambda_bias = src.lambda_bias;
            Q.num_sed = src.num_sed;
            Q.bias_kind = src.bias_kind;
            Q.bias_min = src.bias_min;
            Q.bias_max = src.bias_max;
            Q.sed_kind = src.sed_kind;
            Q.sed_f1 = src.sed_f1;
            Q.sed_f2 = src.sed_f2;
            Q.sed_ltot = src.sed_ltot;
            Q.angular_kind = src.kind == PMC_SOURCE_POINT ? src.angular_kind : PMC_ANGULAR_ISOTROPIC;
            std::memcpy(Q.angular_axis, src.angular_axis, sizeof(Q.angular_axis));
            Q.angular_cos_delta = src.angular_cos_delta;
            if (Q.angular_kind == PMC_ANGULAR_NETZER && !netzer)
            {
                std::vector<double> ct, cumulative;
                netzerTable(ct, cumulative);
                if ((rc = sink.upload(ct.data(), ct.size(), &D.netzer_cos))) return rc;
                if ((rc = sink.upload(cumulative.data(), cumulative.size(), &D.netzer_X))) return rc;
                netzer = true;
            }
            if (src.kind == PMC_SOURCE_SERSIC)
            {
                if ((rc = sink.upload(src.sersic_s, size_t(src.sersic_n), &Q.sersic_s))) return rc;
                if ((rc = sink.upload(src.sersic_M, size_t(src.sersic_n), &Q.sersic_M))) return rc;
                if (numSources == 1) sersicDoubles += 2 * src.sersic_n;
            }
            if (src.lambda_mode == PMC_LAMBDA_OLIGO)
            {
                if ((rc = sink.upload(src.oligo_lambda, size_t(src.num_oligo), &Q.oligo_lambda))) return rc;
                if ((rc = sink.upload(src.oligo_weight, size_t(src.num_oligo), &Q.oligo_weight))) return rc;
            }
            else
            {
                if ((rc = sink.upload(src.sed_lambda, size_t(src.num_sed), &Q.sed_lambda))) return rc;
                if ((rc = sink.upload(src.sed_p, size_t(src.num_sed), &Q.sed_p))) return rc;
                if ((rc = sink.upload(src.sed_P, size_t(src.num_sed), &Q.sed_P))) return rc;
            }
        }
        D.src_first[numSources] = numSources > 1 ? scene.source_first[numSources] : ~0ull;
        D.kin = X.moving ? 1 : 0;
        for (int si = 0; si < PMC_MAX_SOURCES; ++si)
        {
            DevVelocity& V = D.vel[si];
            V.kind = X.velocity[si].kind;
            V.magnitude = X.velocity[si].magnitude;
            std::memcpy(V.vec, X.velocity[si].vector, sizeof(V.vec));
            V.unity_radius = X.velocity[si].unity_radius;
            V.exponent = X.velocity[si].exponent;
        }
        return rc;
    }

    // ---- one wavelength for every history: its dust properties and its bin in every instrument are found here once, as launchHistory finds them
    // DustMix::indexForLambda: NR::locateClip on the index borders
    inline int locateClip(const double* border, int n, double x)
    {
        if (x < border[0]) return 0;
        int jl = -1, ju = n - 1;
        while (ju - jl > 1)
        {
            const int jm = (ju + jl) >> 1;
            if (x < border[jm])
                ju = jm;
            else
                jl = jm;
        }
        return std::max(jl, 0);
    }
    // DisjointWavelengthGrid::bin: upper_bound on the borders
    inline int32_t wavelengthBin(const double* border, int numBorder, const int32_t* ellv, double lambda)
    {
        int lo = 0, hi = numBorder;
        while (lo < hi)
        {
            const int mid = (lo + hi) >> 1;
            if (lambda < border[mid])
                hi = mid;
            else
                lo = mid + 1;
        }
        return ellv[lo];
    }

    inline void setMonoConstants(const pmc_scene& scene, const SceneSwitches& sw, DevScene& D)
    {
        const int numSources = numSourcesOf(scene);
        D.mono = (sourceOf(scene, 0).lambda_mode == PMC_LAMBDA_OLIGO && !sw.noMono) ? 1 : 0;
        for (int si = 0; si < numSources && D.mono; ++si)
            if (sourceOf(scene, si).num_oligo != 1 || sourceOf(scene, si).oligo_lambda[0] != sourceOf(scene, 0).oligo_lambda[0]) D.mono = 0;
        D.mono_lambda = D.mono_ext = D.mono_sca = D.mono_asym = D.mono_abs = 0.;
        if (!D.mono) return;
        const pmc_medium& med = firstComponent(scene);
        const double lambda = sourceOf(scene, 0).oligo_lambda[0];
        const int il = locateClip(med.lambda_border, med.num_lambda, lambda);
        D.mono_lambda = lambda;
        D.mono_ext = med.sigma_ext[il], D.mono_sca = med.sigma_sca[il], D.mono_asym = med.asymmpar[il];
        if (D.explicit_absorption) D.mono_abs = med.sigma_abs[il];
        for (int h = 0; h < D.num_media && D.num_media > 1; ++h)
        {
            const pmc_medium& mh = scene.media[h];
            const int ih = locateClip(mh.lambda_border, mh.num_lambda, lambda);
            D.med[h].mono_ext = mh.sigma_ext[ih], D.med[h].mono_sca = mh.sigma_sca[ih], D.med[h].mono_abs = mh.sigma_abs ? mh.sigma_abs[ih] : 0.;
            D.med[h].mono_asym = mh.asymmpar[ih];
        }
    }

    // ---- instruments, frame layout and the statistics accumulator (after setMonoConstants).  sedDoubles: the privatised SED blocks of the
    // transition and launch kernels in LDS
    inline int uploadInstruments(const pmc_scene& scene, TableSink& sink, DevScene& D, int64_t& frameSize, int& sedDoubles)
    {
        int rc = PMC_OK;
        D.num_instruments = scene.num_instruments;
        sedDoubles = 0;
        D.any_stats = 0;
        D.stat_acc_records = 0;
        for (int i = 0; i < scene.num_instruments; ++i)
        {
            const pmc_instrument& I = scene.instruments[i];
            DevInstrument& d = D.inst[i];
            d.kx = I.kobs[0], d.ky = I.kobs[1], d.kz = I.kobs[2];
            // RN(1/k) as PathSegmentGenerator's users divide by it; an axis with |k| <= 1e-15 is ignored (TreeSpatialGrid.cpp:160-175)
            const double ignored = std::nan("");
            d.ikx = std::fabs(d.kx) > 1e-15 ? 1. / d.kx : ignored;
            d.iky = std::fabs(d.ky) > 1e-15 ? 1. / d.ky : ignored;
            d.ikz = std::fabs(d.kz) > 1e-15 ? 1. / d.kz : ignored;
            d.sgn = (d.kx < 0. ? 1u : 0u) | (d.ky < 0. ? 2u : 0u) | (d.kz < 0. ? 4u : 0u);
            d.costheta = I.costheta, d.sintheta = I.sintheta, d.cosphi = I.cosphi, d.sinphi = I.sinphi;
            d.cosomega = I.cosomega, d.sinomega = I.sinomega;
            d.xpmin = I.xpmin, d.xpsiz = I.xpsiz, d.ypmin = I.ypmin, d.ypsiz = I.ypsiz;
            d.nxp = I.nxp, d.nyp = I.nyp;
            d.same_observer = I.same_observer_as_preceding;
            d.include_sed = I.include_flux_density;
            d.include_ifu = I.include_surface_brightness;
            d.record_components = I.record_components;
            d.num_levels = I.num_scattering_levels;
            d.record_stats = I.record_statistics;
            d.aperture_r2 = I.aperture_radius2;
            d.zp1 = 1. + I.redshift;
            d.num_lambda = I.num_lambda;
            d.num_border = I.num_border;
            if ((rc = sink.upload(I.border, size_t(I.num_border), &d.border))) return rc;
            if ((rc = sink.upload(I.ellv, size_t(I.num_border) + 1, &d.ellv))) return rc;
            // (the bin of the redshifted wavelength)
            d.mono_ell = D.mono ? wavelengthBin(I.border, I.num_border, I.ellv, D.mono_lambda * d.zp1) : -1;
            pmc_frame_layout L;
            frameSize = pmc_layout_compute(&scene, i, &L);
            d.sed_offset = L.sed_offset, d.ifu_offset = L.ifu_offset, d.wsed_offset = L.wsed_offset, d.wifu_offset = L.wifu_offset;
            d.npix = L.npix;
            d.num_components = (int32_t)L.num_components;
            d.sed_lds_offset = sedDoubles;
            if (d.include_sed) sedDoubles += (d.num_components + (d.record_stats ? 5 : 0)) * d.num_lambda;
            if (d.record_stats) D.any_stats = 1;
            d.stat_acc_offset = D.stat_acc_records;
            if (d.record_stats && d.include_ifu) D.stat_acc_records += d.npix * d.num_lambda;
        }
        D.stat_acc = nullptr;
        if (D.stat_acc_records) rc = sink.allocate<double>(size_t(D.stat_acc_records) * 8, &D.stat_acc, true);
        return rc;
    }

    // ---- radiation field table (rfSize: its doubles, 0: not stored)
    inline int uploadRadiationField(const pmc_scene& scene, TableSink& sink, DevScene& D, int64_t& rfSize)
    {
        const pmc_radiation_field& RF = scene.radiation_field;
        int rc = PMC_OK;
        D.rf_store = RF.store ? 1 : 0;
        rfSize = 0;
        if (!D.rf_store) return rc;
        D.rf_num_lambda = RF.num_lambda;
        D.rf_num_border = RF.num_border;
        if ((rc = sink.upload(RF.border, size_t(RF.num_border), &D.rf_border))) return rc;
        if ((rc = sink.upload(RF.ellv, size_t(RF.num_border) + 1, &D.rf_ellv))) return rc;
        rfSize = int64_t(scene.grid.num_cells) * RF.num_lambda;
        return sink.allocate<double>(size_t(rfSize), &D.rf, true);
    }

    // ---- LDS plan (in doubles from the start of dynamic LDS; DevScene::lds_*).  Walk kernels and cycle start kernel: the grid tables, at offset 0.
    // Transition and launch kernels: no grid tables; privatised SED blocks, hot-bin table (pmc_detect.inc HOT_BINS keys + values), integer scratch
    // (regrouping arrays and list-append counters).  Launch kernel only, behind the regions the two share: Sersic tables, then the index borders of
    // the dust mix (DustMix::_lambdav: the binary search of every new history's wavelength) if they fit
    struct LdsPlan
    {
        int32_t sed_off, sed_len, hot_off, sort_off, total_transition, src_off, dust_off, dust_in_lds, total_launch, total_walk;
        size_t walkBytes, transitionBytes, launchBytes;
    };
    constexpr int PMC_LDS_HOT_DOUBLES = 2 * 256, PMC_LDS_SORT_DOUBLES = (64 + 2 * 1024 + 8) / 2;
    inline LdsPlan planLds(int gridLen, int sedDoubles, int sersicDoubles, int numLambda)
    {
        LdsPlan P{};
        P.sed_off = 0;
        P.sed_len = sedDoubles;
        P.hot_off = P.sed_off + P.sed_len;
        P.sort_off = P.hot_off + PMC_LDS_HOT_DOUBLES;
        P.total_transition = P.sort_off + PMC_LDS_SORT_DOUBLES;
        P.src_off = P.total_transition;
        P.dust_off = P.src_off + sersicDoubles;
        P.dust_in_lds = numLambda <= 8192 ? 1 : 0;
        P.total_launch = P.dust_off + (P.dust_in_lds ? numLambda : 0);
        P.total_walk = gridLen;
        P.walkBytes = size_t(P.total_walk) * sizeof(double);
        P.transitionBytes = size_t(P.total_transition) * sizeof(double);
        P.launchBytes = size_t(P.total_launch) * sizeof(double);
        return P;
    }
    inline int setLdsPlan(const LdsPlan& P, DevScene& D)
    {
        D.lds_sed_off = P.sed_off, D.lds_sed_len = P.sed_len, D.lds_hot_off = P.hot_off, D.lds_sort_off = P.sort_off;
        D.lds_total_transition = P.total_transition, D.lds_src_off = P.src_off, D.lds_dust_off = P.dust_off, D.dust_in_lds = P.dust_in_lds;
        D.lds_total_launch = P.total_launch, D.lds_total_walk = P.total_walk;
        if (P.walkBytes > 160 * 1024 || P.launchBytes > 160 * 1024) return fail(PMC_ERR_UNSUPPORTED, "scene tables need more than 160 KiB of LDS");
        return PMC_OK;
    }

    // ---- the stages in order; what the context keeps of them next to DevScene
    struct SceneTables
    {
        int64_t frameSize{0};
        int64_t rfSize{0};
        LdsPlan lds{};
    };
    inline int buildSceneTables(const pmc_scene& scene, const SceneExtension& X, const SceneSwitches& sw, TableSink& sink, DevScene& D, SceneTables& out)
    {
        int rc = PMC_OK;
        std::vector<int32_t> devToCell;
        int sersicDoubles = 0, sedDoubles = 0;
        if ((rc = uploadGrid(scene, sw, sink, D, devToCell))) return rc;
        if ((rc = uploadMedia(scene, X, devToCell, sink, D))) return rc;
        setOptions(scene, sw, D);
        if ((rc = uploadSources(scene, X, sink, D, sersicDoubles))) return rc;
        setMonoConstants(scene, sw, D);
        if ((rc = uploadInstruments(scene, sink, D, out.frameSize, sedDoubles))) return rc;
        if ((rc = uploadRadiationField(scene, sink, D, out.rfSize))) return rc;
        out.lds = planLds(D.lds_grid_len, sedDoubles, sersicDoubles, D.num_lambda);
        if ((rc = setLdsPlan(out.lds, D))) return rc;
        // outputs
        if ((rc = sink.allocate<double>(size_t(out.frameSize), &D.frames, true))) return rc;
        return sink.allocate<unsigned long long>(PMC_NUM_COUNTERS, &D.counters, true);
    }
}

#endif
