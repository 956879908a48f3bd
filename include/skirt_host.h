/* skirt_host.h -- C entry points of the host model layer (libskirthost.so).
 *
 * The host layer reads an unchanged SKIRT .ski file, performs the reference's setup for the classes the
 * primary-emission path supports (grid construction, density sampling, dust tables, source tables, instruments;
 * SKIRT/core/MonteCarloSimulation.cpp:20-37 setupSimulation) and flattens the result into the pmc_scene of
 * pmc.h.  After the photon loop it calibrates the detector arrays and writes the reference's output files
 * (FluxRecorder::calibrateAndWrite, SKIRT/core/FluxRecorder.cpp:484-846).  It contains NO photon loop.
 */
#ifndef SKIRT_HOST_H
#define SKIRT_HOST_H

#include "pmc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct skh_simulation skh_simulation;

const char* skh_last_error(void);
/* XmlHierarchyCreator::readFile: parse the ski file; NULL on error */
skh_simulation* skh_load(const char* ski_path);
void skh_free(skh_simulation* sim);
/* overrides applied before skh_setup */
int skh_set_num_packets(skh_simulation* sim, uint64_t n);
int skh_set_tree_topology_file(skh_simulation* sim, const char* treetop_path);
/* before skh_setup: evaluate the densities of an imported particle medium (ParticleMedium) on the GPU during setup.  The
   four pointers are libpmc.so's pmc_sampler_create, pmc_sampler_density, pmc_sampler_destroy and pmc_last_error (passed
   at run time so that this library does not link against the HIP engine); results are bit-identical to the host's */
int skh_set_particle_sampler(skh_simulation* sim, void* create, void* density, void* destroy, void* last_error, int32_t device);
/* the same for a medium imported from an adaptive mesh (AdaptiveMeshMedium): create_mesh is libpmc.so's pmc_sampler_create_mesh, the other
   three are as above */
int skh_set_mesh_sampler(skh_simulation* sim, void* create_mesh, void* density, void* destroy, void* last_error, int32_t device);
/* Simulation::setupSimulation */
int skh_setup(skh_simulation* sim);
/* valid after skh_setup, owned by the simulation */
const pmc_scene* skh_scene(const skh_simulation* sim);
/* what goes to pmc_create_ext next to the scene: the phase function of every medium component (valid after skh_setup, owned by the simulation) */
const pmc_scene_ext* skh_scene_ext(const skh_simulation* sim);
uint64_t skh_num_packets(const skh_simulation* sim);
int32_t  skh_seed(const skh_simulation* sim);
uint64_t skh_setup_draws(const skh_simulation* sim);
/* luminosity that one launched packet carries at oligochromatic wavelength `index` (SourceSystem.cpp:96,105-106 times the
   weight of NormalizedSource.cpp:91-105); negative if the simulation is not oligochromatic or the index is out of range */
double   skh_packet_luminosity(const skh_simulation* sim, int32_t index);
int64_t  skh_frame_size(const skh_simulation* sim);
int skh_frame_layout(const skh_simulation* sim, int32_t instrument, pmc_frame_layout* out);
/* calibrates `frames` in place and writes <prefix>_<instrument>_*.fits / _sed.dat / _sedstats.dat into outdir */
int skh_write(const skh_simulation* sim, double* frames, const char* outdir);
/* the same without the statistics files (_stats0..4.fits, _sedstats.dat): for a segment whose statistics arrays are incomplete
   (pmc_run_primary returned PMC_ERR_OVERFLOW: the flux arrays are complete, the sums of w^k are not) */
int skh_write_fluxes_only(const skh_simulation* sim, double* frames, const char* outdir);
/* radiation field (RadiationFieldOptions::storeRadiationField): doubles of the table rf[m * nbins + ell] that
   pmc_download_radiation_field fills (0: not stored), and the RadiationFieldProbe / PerCellForm files
   <prefix>_<probe>_J.dat written from it (RadiationFieldProbe.cpp:27-78, PerCellForm.cpp:14-32) */
int64_t  skh_radiation_field_size(const skh_simulation* sim);
int skh_write_radiation_field(const skh_simulation* sim, const double* rf, const char* outdir);
int skh_summary(const skh_simulation* sim, char* buffer, int32_t capacity);

/* Probes of the spatial grid: DensityProbe and OpacityProbe with a PerCellForm (<prefix>_<probe>_<fileid>.dat) or a ParallelProjectionForm
   (<prefix>_<probe>_<projectedFileid>.fits: one "projected map" per quantity, e.g. dust_Sigma, elec_N, tau).  The pixels of a map are sums
   over sub-sample rays of line integrals through the grid; the integrator is handed over at run time -- libpmc.so's pmc_integrate_rays
   with user = the pmc_ctx -- so that this library does not link against the HIP engine. */
typedef int (*skh_integrate_fn)(void* user, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                                const double* cell_values, double* sums);
typedef struct
{
    char file_name[256];    /* name of the FITS file, without directory */
    int32_t nx, ny;         /* pixels */
    int32_t sampling;       /* sub-samples per pixel and axis (numSampling) */
    int32_t num_values;     /* values per ray: 1, or the wavelengths of an opacity probe */
    int32_t after_setup;    /* probeAfter: 1 Setup, 0 Run */
    int64_t num_rays;       /* nx * ny * sampling^2 */
} skh_probe_map;
/* projected maps, in file order (valid after skh_setup; 0 for a simulation without a medium) */
int32_t skh_num_probe_maps(const skh_simulation* sim);
int skh_probe_map_info(const skh_simulation* sim, int32_t map, skh_probe_map* out);
/* 1: the map is a weighted average along its rays (a TemperatureProbe's: skh_probe_map_values then gives the weights [num_cells], num_values
   is 1), 0: a line integral, negative: error.  (A function of its own: skh_probe_map keeps its layout.) */
int32_t skh_probe_map_averaged(const skh_simulation* sim, int32_t map);
/* the rays [num_rays][3] of a map, ordered by pixel (j, i) and sub-sample (is, js), and its cell values [num_values][num_cells] in
   internal units (the unit factor of the projected quantity is applied to the integrals) */
int skh_probe_map_rays(const skh_simulation* sim, int32_t map, double* origins, double* directions);
int skh_probe_map_values(const skh_simulation* sim, int32_t map, double* cell_values);
/* writes every probe file into outdir; the per-cell files are written without calling `integrate`, which may be NULL when the ski file
   has no projected map.  skh_write_probes_when: only the probes with probeAfter Setup (when = 0) or Run (when = 1); -1: all */
int skh_write_probes(const skh_simulation* sim, skh_integrate_fn integrate, void* user, const char* outdir);
int skh_write_probes_when(const skh_simulation* sim, skh_integrate_fn integrate, void* user, const char* outdir, int32_t when);

/* Dust temperatures from the stored radiation field (TemperatureProbe; EquilibriumDustEmissionCalculator::equilibriumTemperature), for a
   panchromatic simulation that stores the field and has dust.  skh_dust_heating: the tables of pmc_dust_heating (include/pmc.h), owned by the
   simulation, built at the first call.  skh_dust_temperatures: the CPU restatement of pmc_dust_temperatures from a host copy of the table
   rf[m * nbins + ell]: out[H + 1][num_cells], the dust components in order, then their mass-weighted mean; skh_dust_temperatures_from: the same
   for any tables.  The engine's result equals these bit for bit. */
int skh_dust_heating(const skh_simulation* sim, pmc_dust_heating* out);
int skh_dust_temperatures(const skh_simulation* sim, const double* rf, double* out);
int skh_dust_temperatures_from(const pmc_dust_heating* tables, const double* rf, double* out);
/* the medium components that are dust (the rows of the tables), up to PMC_MAX_MEDIA indices; returns their number (0 without dust heating) */
int32_t skh_dust_components(const skh_simulation* sim, int32_t* components);

/* The probes that need the radiation field -- TemperatureProbe (per cell and projected: a density-weighted average along the rays) and
   DustAbsorptionPerCellProbe -- are written by skh_write_probes_with: next to the integrator it takes libpmc.so's
   pmc_integrate_weighted_rays and pmc_dust_temperatures (user = the pmc_ctx, as for the integrator) and a host copy of the table.  With
   temperatures == NULL the host computes the temperatures from rf; rf is needed by DustAbsorptionPerCellProbe in any case.  Members that
   the ski file's probes do not need may be NULL. */
typedef int (*skh_integrate_weighted_fn)(void* user, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                                         const double* cell_weights, const double* cell_values, double* sums);
typedef int (*skh_temperature_fn)(void* user, const pmc_dust_heating* tables, double* out);
typedef struct
{
    skh_integrate_fn integrate;
    skh_integrate_weighted_fn integrate_weighted;
    skh_temperature_fn temperatures;
    void* user;
    const double* rf;
} skh_probe_engine;
int skh_write_probes_with(const skh_simulation* sim, const skh_probe_engine* engine, const char* outdir, int32_t when);
/* 1 if a probe written with `when` (0 Setup, 1 Run, -1 all) reads the radiation field table (TemperatureProbe, DustAbsorptionPerCellProbe), else 0:
   a caller that keeps the table on the device copies it to the host only then */
int32_t skh_probes_need_radiation_field(const skh_simulation* sim, int32_t when);

/* ConvergenceInfoProbe (ConvergenceInfoProbe.cpp): <prefix>_<probe>_convergence.dat -- per material type the input and the gridded mass and
   optical depth along the coordinate axes at the probe's wavelength, then the optical depths of the cells' diagonals -- is written by every
   skh_write_probes* function; its gridded optical depths are six rays per material type through `integrate`, without which it fails.
   ConvergenceCutsProbe (ConvergenceCutsProbe.cpp, DefaultCutsForm.cpp, PlanarCutsForm::writePlanarCut): per material type present the true
   density <prefix>_<probe>_dust_t_xy.fits / _elec_t_xy.fits -- the media's own density at 1024 x 1024 positions over the grid's bounding box in
   the plane z = 0, computed by the host -- and the gridded density _dust_g_xy.fits / _elec_g_xy.fits -- the value of the cell that holds each
   position; the plane y = 0 (_xz) when skh_dimension is 2 or 3 and the plane x = 0 (_yz) when it is 3.  The gridded cuts come from a point
   sampler handed over at run time -- libpmc.so's pmc_sample_cells with user = the pmc_ctx (the `user` of `engine`) -- so that this library does
   not link the engine.  skh_write_probes_sampled is skh_write_probes_with plus the sampler; `engine` may be NULL or hold NULL members for what
   the ski file's probes do not need (the sampler's user is engine->user).  Without a sampler -- also through skh_write_probes,
   skh_write_probes_when and skh_write_probes_with -- a ski file with a ConvergenceCutsProbe that is due fails with "needs a sampler": the files
   are never left out silently and never computed on the CPU instead. */
typedef int (*skh_sample_fn)(void* user, int64_t num_points, const double* positions, int32_t num_values, const double* cell_values, double* values,
                             int32_t* cells);
int skh_write_probes_sampled(const skh_simulation* sim, const skh_probe_engine* engine, skh_sample_fn sample, const char* outdir, int32_t when);
/* MediumSystem::dimension (MediumSystem.cpp:403-408): 1 spherical, 2 axisymmetric, 3 neither -- the largest of the medium components */
int32_t skh_dimension(const skh_simulation* sim);

/* SpatialGrid::cellIndex(Position) of the simulation's grid for many positions [num_points][3] (valid after skh_setup): cells[p] = the cell
   that holds positions[p] in the numbering of pmc_trace_ray, -1 outside the grid.  A literal restatement of the reference's functions
   (TreeNode::leafChild with OctTreeNode::child / BinTreeNode::child; NR::locateFail per axis of a Cartesian grid; the nearest site of a
   Voronoi mesh), on one thread: the domain box is closed and a position on a wall between two cells belongs to the upper one.  It is the CPU
   yardstick of pmc_sample_cells, as skh_dust_temperatures is of pmc_dust_temperatures. */
int skh_cell_indices(const skh_simulation* sim, int64_t num_points, const double* positions, int32_t* cells);

/* Imported media (valid after skh_setup).  skh_adaptive_mesh: the tree of an AdaptiveMeshMedium component and the densities of its cells as
   the tables of pmc_adaptive_mesh (include/pmc.h) -- pointers into the simulation, valid until skh_free; an error for a component of another
   kind.  skh_imported_densities: Snapshot::density(Position) of an imported component (ParticleMedium, AdaptiveMeshMedium) at positions
   [n][3] -- the mass or number density as the file implies, before the conversion by the material mix --, on the device when a sampler is
   bound (skh_set_particle_sampler, skh_set_mesh_sampler), else on the host cores; a position that the reference cannot locate in an adaptive
   mesh fails with its words ("Can't locate the appropriate child node") and the lowest such index.  skh_imported_mass: Snapshot::mass(), the
   total effective mass or number of the component's entities after the policy of ImportedMedium (mass fraction, metallicity, temperature
   cutoff). */
int skh_imported_mass(const skh_simulation* sim, int32_t component, double* out);
int skh_adaptive_mesh(const skh_simulation* sim, int32_t component, pmc_adaptive_mesh* out);
int skh_imported_densities(const skh_simulation* sim, int32_t component, int64_t n, const double* positions, double* out);

/* A set-up scene as ONE file: everything pmc_create reads plus the numbers a driver of the photon loop needs.  In a job of
   one process per GPU, one process sets the simulation up (all host cores) and saves it, the others load it instead of
   repeating the setup -- the reference repeats Simulation::setupSimulation in every MPI process.  A loaded scene serves
   pmc_create_ext and the frame layout; the output files are written by the process that holds the simulation. */
int skh_scene_save(const skh_simulation* sim, const char* path);
typedef struct skh_scene_file skh_scene_file;
skh_scene_file* skh_scene_load(const char* path);
void skh_scene_file_free(skh_scene_file* file);
const pmc_scene* skh_scene_file_scene(const skh_scene_file* file);
/* the extension saved with the scene; a file written before scenes had one gives every component as Henyey-Greenstein */
const pmc_scene_ext* skh_scene_file_scene_ext(const skh_scene_file* file);
enum { SKH_SCENE_SEED = 0, SKH_SCENE_NUM_PACKETS = 1, SKH_SCENE_FRAME_SIZE = 2, SKH_SCENE_RADIATION_FIELD_SIZE = 3, SKH_SCENE_SETUP_DRAWS = 4 };
int64_t skh_scene_file_number(const skh_scene_file* file, int32_t what);
int skh_scene_file_layout(const skh_scene_file* file, int32_t instrument, pmc_frame_layout* out);

#ifdef __cplusplus
}
#endif
#endif
