// capi.cpp -- C entry points of the host model layer (libskirthost.so), for ctypes and for the command line driver.
// See include/skirt_host.h for the declarations.

#include "../../include/skirt_host.h"
#include "simulation.hpp"
#include <algorithm>
#include <cstring>
#include <fstream>
#include <type_traits>

namespace
{
    thread_local std::string t_error;

    // the frame of an entry point that can fail: "invalid argument" unless `valid`, then what the body returns (0 for a body that returns
    // nothing); an exception leaves its text for skh_last_error and makes -1
    template<typename Body> int guarded(bool valid, Body&& body)
    {
        try
        {
            if (!valid) throw std::runtime_error("invalid argument");
            if constexpr (std::is_void_v<decltype(body())>)
            {
                body();
                return 0;
            }
            else
                return body();
        }
        catch (const std::exception& e)
        {
            t_error = e.what();
            return -1;
        }
    }
}

// error text of the calling thread, for the other translation units of the library (scenefile.cpp)
const char* skh_set_error_text(const std::string& text)
{
    t_error = text;
    return t_error.c_str();
}

struct skh_simulation
{
    std::unique_ptr<skh::Simulation> sim;
};

namespace
{
    bool loaded(const skh_simulation* h) { return h && h->sim; }

    // the one path of the four skh_write_probes* entry points: the caller's engine (null: none) and sampler as the simulation takes them
    int writeProbes(const skh_simulation* h, bool valid, const skh_probe_engine* engine, skh_sample_fn sample, const char* outdir, int32_t when)
    {
        return guarded(loaded(h) && valid && outdir, [&] {
            skh::Simulation::ProbeEngine e;
            if (engine)
            {
                e.integrate = engine->integrate;
                e.weighted = engine->integrate_weighted;
                e.temperatures = engine->temperatures;
                e.user = engine->user;
                e.rf = engine->rf;
            }
            e.sample = sample;
            h->sim->writeProbes(e, outdir, when);
        });
    }

    // the one body of skh_set_particle_sampler and skh_set_mesh_sampler: hands the entry points of the device sampler (include/pmc.h:
    // pmc_sampler_create or pmc_sampler_create_mesh, and pmc_sampler_density / _destroy, pmc_last_error, which serve both kinds) to the
    // simulation; the densities of an imported medium of that kind are then evaluated on the GPU during skh_setup
    template<class Create>
    int setSampler(skh_simulation* h, Create skh::SamplerApi::*create, void (skh::Simulation::*set)(const skh::SamplerApi&), void* entry,
                   void* density, void* destroy, void* last_error, int32_t device)
    {
        return guarded(loaded(h) && entry && density && destroy, [&] {
            skh::SamplerApi api;
            api.*create = reinterpret_cast<Create>(entry);
            api.density = reinterpret_cast<decltype(api.density)>(density);
            api.destroy = reinterpret_cast<decltype(api.destroy)>(destroy);
            api.lastError = reinterpret_cast<decltype(api.lastError)>(last_error);
            api.device = device;
            (h->sim.get()->*set)(api);
        });
    }
}

extern "C" {

const char* skh_last_error(void)
{
    return t_error.c_str();
}

skh_simulation* skh_load(const char* ski_path)
{
    skh_simulation* result = nullptr;
    // (the simulation first: a refused ski file leaves no handle behind)
    guarded(true, [&] { result = new skh_simulation{skh::Simulation::fromFile(ski_path)}; });
    return result;
}

void skh_free(skh_simulation* h)
{
    delete h;
}

int skh_set_num_packets(skh_simulation* h, uint64_t n)
{
    h->sim->setNumPackets(n);
    return 0;
}

int skh_set_particle_sampler(skh_simulation* h, void* create, void* density, void* destroy, void* last_error, int32_t device)
{
    return setSampler(h, &skh::SamplerApi::createParticles, &skh::Simulation::setParticleSampler, create, density, destroy, last_error, device);
}

int skh_set_mesh_sampler(skh_simulation* h, void* create_mesh, void* density, void* destroy, void* last_error, int32_t device)
{
    return setSampler(h, &skh::SamplerApi::createMesh, &skh::Simulation::setMeshSampler, create_mesh, density, destroy, last_error, device);
}

int skh_adaptive_mesh(const skh_simulation* h, int32_t component, pmc_adaptive_mesh* out)
{
    return guarded(loaded(h) && out, [&] {
        const skh::ImportedMedium& medium = h->sim->importedMedium(component);
        const skh::AdaptiveMeshMedium* mesh = dynamic_cast<const skh::AdaptiveMeshMedium*>(&medium);
        if (!mesh) throw std::runtime_error("medium component " + std::to_string(component) + " is a " + medium.type() + ", not an AdaptiveMeshMedium");
        if (!mesh->snapshot.numNodes()) throw std::runtime_error("the simulation has not been set up");
        *out = mesh->snapshot.tables();
    });
}

int skh_imported_mass(const skh_simulation* h, int32_t component, double* out)
{
    return guarded(loaded(h) && out, [&] { *out = h->sim->importedMedium(component).imported().mass(); });
}

int skh_imported_densities(const skh_simulation* h, int32_t component, int64_t n, const double* positions, double* out)
{
    return guarded(loaded(h) && n >= 0 && (n == 0 || (positions && out)), [&] {
        const skh::ImportedMedium& medium = h->sim->importedMedium(component);
        std::vector<skh::Vec3> r(static_cast<size_t>(n));
        for (int64_t p = 0; p < n; ++p) r[p] = skh::Vec3{positions[3 * p], positions[3 * p + 1], positions[3 * p + 2]};
        std::vector<double> density;
        medium.imported().densities(r, density);
        std::copy(density.begin(), density.end(), out);
    });
}

int skh_set_tree_topology_file(skh_simulation* h, const char* path)
{
    return guarded(true, [&] {
        // TreeSpatialGridTopologyProbe format (TreeSpatialGrid.cpp:225-251): comment lines, the number of children
        // of the root, then one "1"/"0" per node in depth-first order
        std::ifstream in(path);
        if (!in) throw std::runtime_error(std::string("cannot open tree topology file ") + path);
        std::vector<char> topology;
        std::string line;
        bool first = true;
        while (std::getline(in, line))
        {
            if (line.empty() || line[0] == '#') continue;
            if (first)
            {
                first = false;
                if (std::stoi(line) != 8 && std::stoi(line) != 0) throw std::runtime_error("topology is not an octree");
                continue;
            }
            topology.push_back(line[0] == '1');
        }
        h->sim->setTreeTopology(std::move(topology));
    });
}

int skh_setup(skh_simulation* h)
{
    return guarded(true, [&] { h->sim->setup(); });
}

const pmc_scene* skh_scene(const skh_simulation* h)
{
    return &h->sim->scene();
}

const pmc_scene_ext* skh_scene_ext(const skh_simulation* h)
{
    return &h->sim->sceneExt();
}

uint64_t skh_num_packets(const skh_simulation* h)
{
    return h->sim->numPackets();
}

int32_t skh_seed(const skh_simulation* h)
{
    return h->sim->seed();
}

double skh_packet_luminosity(const skh_simulation* h, int32_t index)
{
    const pmc_source& src = h->sim->scene().source;
    if (src.lambda_mode != PMC_LAMBDA_OLIGO || index < 0 || index >= src.num_oligo) return -1.;
    return src.packet_luminosity * src.oligo_weight[index];
}

uint64_t skh_setup_draws(const skh_simulation* h)
{
    return h->sim->setupDraws();
}

int64_t skh_frame_size(const skh_simulation* h)
{
    return h->sim->frameSize();
}

int skh_frame_layout(const skh_simulation* h, int32_t instrument, pmc_frame_layout* out)
{
    if (instrument < 0 || instrument >= h->sim->numInstruments()) return -1;
    *out = h->sim->layout(instrument);
    return 0;
}

int skh_write(const skh_simulation* h, double* frames, const char* outdir)
{
    return guarded(true, [&] { h->sim->write(frames, outdir); });
}

// number of doubles of the radiation field table (0: the simulation does not store it)
int64_t skh_radiation_field_size(const skh_simulation* h)
{
    return loaded(h) ? h->sim->radiationFieldSize() : 0;
}

int skh_write_fluxes_only(const skh_simulation* h, double* frames, const char* outdir)
{
    return guarded(true, [&] { h->sim->write(frames, outdir, false); });
}

// writes the RadiationFieldProbe files from the table rf[m * nbins + ell]
int skh_write_radiation_field(const skh_simulation* h, const double* rf, const char* outdir)
{
    return guarded(loaded(h) && rf && outdir, [&] { h->sim->writeRadiationField(rf, outdir); });
}

int32_t skh_num_probe_maps(const skh_simulation* h)
{
    return guarded(true, [&] { return loaded(h) ? h->sim->numProbeMaps() : 0; });
}

int skh_probe_map_info(const skh_simulation* h, int32_t map, skh_probe_map* out)
{
    return guarded(loaded(h) && out, [&] {
        const skh::Simulation::ProbeMapInfo info = h->sim->probeMapInfo(map);
        std::memset(out, 0, sizeof(*out));
        if (info.fileName.size() >= sizeof(out->file_name)) throw std::runtime_error("probe file name too long");
        std::strcpy(out->file_name, info.fileName.c_str());
        out->nx = info.nx, out->ny = info.ny;
        out->sampling = info.sampling;
        out->num_values = info.numValues;
        out->after_setup = info.afterSetup ? 1 : 0;
        out->num_rays = info.numRays;
    });
}

int32_t skh_probe_map_averaged(const skh_simulation* h, int32_t map)
{
    return guarded(loaded(h), [&] { return h->sim->probeMapInfo(map).averaged ? 1 : 0; });
}

int32_t skh_probes_need_radiation_field(const skh_simulation* h, int32_t when)
{
    return guarded(true, [&] { return loaded(h) && h->sim->probesNeedRadiationField(when) ? 1 : 0; });
}

int skh_probe_map_rays(const skh_simulation* h, int32_t map, double* origins, double* directions)
{
    return guarded(loaded(h) && origins && directions, [&] { h->sim->probeMapRays(map, origins, directions); });
}

int skh_probe_map_values(const skh_simulation* h, int32_t map, double* cell_values)
{
    return guarded(loaded(h) && cell_values, [&] { h->sim->probeMapValues(map, cell_values); });
}

int skh_write_probes_when(const skh_simulation* h, skh_integrate_fn integrate, void* user, const char* outdir, int32_t when)
{
    skh_probe_engine engine{};
    engine.integrate = integrate;
    engine.user = user;
    return writeProbes(h, true, &engine, nullptr, outdir, when);
}

int skh_write_probes(const skh_simulation* h, skh_integrate_fn integrate, void* user, const char* outdir)
{
    return skh_write_probes_when(h, integrate, user, outdir, -1);
}

int skh_write_probes_with(const skh_simulation* h, const skh_probe_engine* engine, const char* outdir, int32_t when)
{
    return writeProbes(h, engine != nullptr, engine, nullptr, outdir, when);
}

int skh_write_probes_sampled(const skh_simulation* h, const skh_probe_engine* engine, skh_sample_fn sample, const char* outdir, int32_t when)
{
    return writeProbes(h, true, engine, sample, outdir, when);
}

int32_t skh_dimension(const skh_simulation* h)
{
    return guarded(loaded(h), [&] { return h->sim->dimension(); });
}

int skh_dust_heating(const skh_simulation* h, pmc_dust_heating* out)
{
    return guarded(loaded(h) && out, [&] { *out = h->sim->dustHeating().flat; });
}

int32_t skh_dust_components(const skh_simulation* h, int32_t* components)
{
    return guarded(true, [&] {
        if (!loaded(h) || !h->sim->hasDustHeating()) return 0;
        const std::vector<int>& dust = h->sim->dustHeating().components;
        for (size_t b = 0; components && b != dust.size(); ++b) components[b] = dust[b];
        return static_cast<int>(dust.size());
    });
}

int skh_dust_temperatures(const skh_simulation* h, const double* rf, double* out)
{
    return guarded(loaded(h) && rf && out, [&] { h->sim->dustTemperatures(rf, out); });
}

int skh_dust_temperatures_from(const pmc_dust_heating* tables, const double* rf, double* out)
{
    return guarded(tables && rf && out, [&] {
        if (!tables->width || !tables->sigma || !tables->planckabs || !tables->temperature || !tables->cell_factor || !tables->mass_density)
            throw std::runtime_error("null table");
        skh::Simulation::dustTemperatures(*tables, rf, out);
    });
}

int skh_cell_indices(const skh_simulation* h, int64_t num_points, const double* positions, int32_t* cells)
{
    return guarded(loaded(h) && num_points >= 0 && (num_points == 0 || (positions && cells)), [&] {
        const skh::SpatialGrid& grid = h->sim->grid();
        for (int64_t p = 0; p < num_points; ++p)
            cells[p] = grid.cellIndex(skh::Vec3{positions[3 * p], positions[3 * p + 1], positions[3 * p + 2]});
    });
}

int skh_summary(const skh_simulation* h, char* buffer, int32_t capacity)
{
    std::string s = h->sim->summary();
    if (capacity > 0)
    {
        std::strncpy(buffer, s.c_str(), capacity - 1);
        buffer[capacity - 1] = 0;
    }
    return static_cast<int>(s.size());
}
}
