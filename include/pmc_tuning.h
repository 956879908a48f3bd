/* pmc_tuning.h -- tuning aids of the MI355X photon-packet engine (libpmc.so): NOT part of the drop-in boundary (pmc.h).
   Nothing here has a counterpart in the reference; the parity tests use the switches to run one scene through two code paths
   of the engine (lists of live slots or not, sorted peel-off records or not, ...), tools/sweep.py and bench.py use them to time
   kernels in series.  The library reads none of this from the environment. */
#ifndef PMC_TUNING_H
#define PMC_TUNING_H

#include "pmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A process-wide table of named switches, consulted by pmc_create / pmc_run_primary where the names below are listed in
   skirt9_amd/csrc/pmc_api.hip and pmc_kernels.hip (a switch is "set" when it has a value; numeric ones are parsed with atoi):
     PMC_SERIAL_WALKS, PMC_TIMING_DUMP, PMC_GEN_DUMP, PMC_PROFILE_DUMP        measurement: kernels of a group in series, dumps to stderr
     PMC_NO_LIVE_LISTS, PMC_NO_PEEL_SORT, PMC_NO_PROP_SORT, PMC_NO_XCD_AFFINITY, PMC_NO_MONO,
     PMC_RF_ATOMICS, PMC_RF_LOG_PER_SLOT, PMC_STAT_ATOMICS, PMC_STAT_LOG_ENTRIES, PMC_STAT_POOL_NO_GROWTH, PMC_PROP_NO_CHECKPOINTS (octree: at run; Voronoi: at pmc_create),
     PMC_VORO_NO_CULL, PMC_VORO_NO_OBSERVER_LISTS, PMC_VORO_CONE_CULL_ONLY, PMC_VORO_NO_PEEL_KERNEL, PMC_VORO_NO_PROP_KERNEL, PMC_VORO_PLAIN_PROP_ONLY, PMC_VORO_NO_CONE_TABLES, PMC_VORO_NO_DEFERRED_SCAN, PMC_VORO_LINK_COUNT_MAX, PMC_VPROP_XCD_SEGMENTS, PMC_VORO_WALKS_IN_SERIES, PMC_VPROP_BLOCKS_PER_CU, PMC_VPEEL_BLOCKS_PER_CU,
     PMC_TREE_AS_BINTREE (at pmc_create: an octree scene runs through the tables and kernels of the binary tree, every octree node as its three levels of splits),
     PMC_POISON_ALLOCATIONS (test aid: device arrays the engine does not initialise are filled with 0xA5 bytes),
     PMC_LAUNCH_GENERIC (at run: the generic launch kernel whatever the scene's sources are)                                             alternative code paths (cross-checks, A/B)
     PMC_WALK_BLOCKS_PER_CU, PMC_PEEL_BLOCKS_PER_CU, PMC_LAUNCH_BLOCKS_PER_CU,
     PMC_CYCLE_BLOCKS_PER_CU, PMC_TRANSITION_BLOCKS_PER_CU,
     PMC_LIST_TASKS_PER_LANE, PMC_CELL_ORDER, PMC_CELL_SHUFFLE                launch geometry, order of the cell table
   value == NULL removes the switch.  Returns PMC_OK. */
int pmc_tuning_set(const char* name, const char* value);
/* removes every switch */
void pmc_tuning_clear(void);

/* threads per workgroup and workgroups of the persistent walk kernel (0 = default) */
int pmc_set_launch(pmc_ctx* ctx, int32_t block, int32_t grid);

/* counted work of the octree walk kernels since create/reset: a wave-step is one pass of a wavefront through the step
   code, a lane-step one cell visit by one lane (lane_steps / (64 wave_steps) = the fraction of the lanes that held a walk);
   rounds = bookkeeping rounds (finished walks stored, next walks taken up).  Propagation lane-steps include the second
   pass over a forced-scattering path.  No reference counterpart (roofline inputs). */
typedef struct pmc_walk_work_values
{
    uint64_t peel_wave_steps, peel_lane_steps, peel_rounds;
    uint64_t prop_wave_steps, prop_lane_steps, prop_rounds;
} pmc_walk_work_values;
int pmc_walk_work(pmc_ctx* ctx, pmc_walk_work_values* out);
/* Tuning aid: DEVICE addresses of the octree walk's hot table (see skirt9_amd/csrc/pmc_device.h) and of the first cells of the propagation walks the last generations left in
   the task records -- so that profiles/microbench/bridge.hip can replay the walk's memory accesses on the scene's own tables.
   No reference counterpart; nothing in the product reads it. */
typedef struct pmc_debug_table_values
{
    const void* cell_table;   /* [cell_slots] 32-byte records (pmc_device.h CellRec) */
    int64_t cell_slots;
    int64_t loose_base;       /* = cell_slots (the octet-line table of profiles/experiments/r04_octet_line_table.patch: first loose leaf) */
    const int32_t* task_cell; /* [num_slots] first cell of the propagation walk of every slot (stale after the segment's end) */
    int64_t num_slots;
} pmc_debug_table_values;
int pmc_debug_tables(pmc_ctx* ctx, pmc_debug_table_values* out);

/* Test aid: the launch kernel the next pmc_run_primary of this context runs (skirt9_amd/csrc/pmc_device.h PMC_LAUNCH_*: bit 0 a moving source, bit 1
   oligochromatic sources only, bit 2 isotropic emission only, bits 3-4 the geometry set: 0 any, 1 one Sersic source, 2 point sources only).  0, and bit 0
   alone, is the generic kernel -- of scenes no special flavour covers, and of every scene under the switch PMC_LAUNCH_GENERIC. */
int pmc_launch_flavour(pmc_ctx* ctx, int32_t* flavour);

/* Test aid: the device function with which the transition kernel turns a uniform deviate X into the scattering cosine of the dipole phase
   function (DipolePhaseFunction::generateCosineFromPhaseFunction), run over n host-supplied deviates u; cos_out: n doubles on the host. */
int pmc_tune_dipole_cosines(pmc_ctx* ctx, const double* u, int64_t n, double* cos_out);

/* Test aid: the device function with which the launch kernel evaluates the bulk velocity of source `source` (pmc_scene_ext::source_velocity;
   GeometricSource.cpp:66-82 with the vector fields) at n host-supplied launch positions r[n][3] (m); v_out: n x 3 doubles on the host (m/s).  A
   source at rest gives zeros. */
int pmc_tune_source_velocities(pmc_ctx* ctx, int32_t source, const double* r, int64_t n, double* v_out);

/* ---- Test aids: the counting sort and the reduce kernels behind the radiation-field log and the statistics log (skirt9_amd/csrc/pmc_log.inc:
   rfHistKernel, rfScanKernel, rfScatterKernel, rfReduceKernel, statReduceKernel), run on logs that the HOST supplies instead of the walk and launch
   kernels.  A log is n (key, value) pairs in whole chunks of `chunk` entries: n > 0, a multiple of `chunk`, at most `max_entries`.  Every aid checks
   its arguments and returns PMC_ERR_INVALID with a message instead of launching; it allocates the device buffers it needs and frees them, works on
   the context's stream, returns when its results are on the host, and leaves the context as pmc_run_primary expects it.  Any 32-bit value is a valid
   key: the kernels drop the keys beyond the partitions, and the reduce kernels those beyond the table.  No reference counterpart. */

/* The log geometry of this context and the constants the kernels are built with (every member an int64_t):
     cell_slots, rf_num_lambda   cells of the device numbering (padding slots included: pmc_tune_cell_numbering), bins of the stored field
     rf_keys, rf_parts           keys of the radiation-field log (cell_slots * rf_num_lambda on a tree grid) and its partitions of 2^rf_bucket_bits keys
     rf_logged                   1: the next pmc_run_primary of this context sends the field's contributions through the log (a stored field on an
                                 octree, at most max_parts partitions, no switch PMC_RF_ATOMICS), 0: it adds them atomically
     stat_records, stat_parts    records of the statistics accumulator and the partitions of 2^stat_bucket_bits records of its log
     stat_logged                 as rf_logged, for the statistics (switch PMC_STAT_ATOMICS)
     chunk                       entries per chunk of a log = per tile of the counting sort
     rf_bucket_bits, stat_bucket_bits
     scan_threads, sort_block    lanes of rfScanKernel and rfScatterKernel: with more partitions than lanes a lane takes several of them
     max_parts                   partitions the sort's LDS histograms hold
     reduce_span                 entries of the partitioned log per workgroup of the reduce kernels
     rf_short_run, stat_short_run   a run of a partition inside a span with fewer entries is added entry by entry instead of through LDS
     max_entries                 the largest n the aids below accept (2^24) */
typedef struct pmc_log_geometry_values
{
    int64_t cell_slots, rf_num_lambda, rf_keys, rf_parts, rf_logged;
    int64_t stat_records, stat_parts, stat_logged;
    int64_t chunk, rf_bucket_bits, stat_bucket_bits, scan_threads, sort_block, max_parts, reduce_span, rf_short_run, stat_short_run, max_entries;
} pmc_log_geometry_values;
int pmc_tune_log_geometry(pmc_ctx* ctx, pmc_log_geometry_values* out);

/* The counting sort alone (the three kernels in front of a reduce), on num_parts partitions of the caller's choice in [1, max_parts]; no table of the
   scene is involved.  stat = 0: partitions of 2^rf_bucket_bits keys, stat = 1: of 2^stat_bucket_bits.  fills: NULL, or per chunk the entries of it
   that are there (0 .. chunk; what lies behind them is never used).  The live entries are those that are there and whose partition, key >> bits, is
   below num_parts.  Out: start[num_parts + 1], the first place of every partition in the partitioned log (start[num_parts] = live entries), and
   sorted_keys[n], sorted_vals[n], of which the first start[num_parts] places hold the live entries by partition, in any order inside one; the
   places behind them hold zeros. */
int pmc_tune_log_partition(pmc_ctx* ctx, int32_t stat, int32_t num_parts, const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n,
                           uint32_t* sorted_keys, double* sorted_vals, uint64_t* start);

/* The radiation-field log as the end of a generation flushes it, with the context's own rf_parts: vals[i] is added to the context's radiation field table
   (its own or the bound one; see pmc_download_radiation_field) at [cell_ext[key / rf_num_lambda] * rf_num_lambda + key % rf_num_lambda], for the keys
   below rf_keys whose cell is no padding slot.  Adds to what the table holds.  PMC_ERR_INVALID unless rf_logged. */
int pmc_tune_rf_log_flush(pmc_ctx* ctx, const uint32_t* keys, const double* vals, int64_t n);

/* The statistics log as the end of a segment flushes it, with the context's own stat_parts: every entry that is there (fills as above, or NULL) with a
   key below stat_records adds 1, w, w^2, w^3, w^4 (w = its value, the powers formed as ((w w) w) w) to its record of the accumulator, which is copied
   to acc_out[stat_records][5] and cleared again: the frames are not touched.  PMC_ERR_INVALID unless stat_logged. */
int pmc_tune_stat_log_flush(pmc_ctx* ctx, const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n, double* acc_out);

/* ext_out[cell_slots]: the caller's cell index of every cell of the device numbering of a tree grid, -1 for a padding slot that holds no cell.
   PMC_ERR_INVALID on a grid without a device numbering. */
int pmc_tune_cell_numbering(pmc_ctx* ctx, int32_t* ext_out);

/* ---- Test aids: the scalar device functions of the transition, launch and walk kernels (skirt9_amd/csrc/pmc_phase.inc, pmc_detect.inc, pmc_launch.inc, pmc_walk.inc,
   pmc_kernels.hip), run over n argument tuples that the HOST supplies, one lane per tuple: the kernels reach some of their branches with one history
   in 10^5 or with none.  The lanes call the functions the kernels call.  Every aid checks its arguments and returns PMC_ERR_INVALID with a message
   instead of launching (a null context or buffer, n < 0 or n > 2^20, an unknown function or kind, a table of fewer than 2 nodes, an instrument or
   source the scene does not have); n = 0 does nothing.  It allocates the device buffers it needs and frees them, works on the context's stream, reads
   no device memory but those buffers and the scene's own tables, returns when its results are on the host, and leaves the context as pmc_run_primary
   expects it.  No reference counterpart. */

/* The scene-free functions: args[n][width_in] doubles -> out[n][width_out] doubles, with the tuples
     PMC_FN_HG_VALUE              (g, cos)                          -> PhaseHG::value
     PMC_FN_HG_CONE_MEAN          (g, cos)                          -> PhaseHG::coneMean (the kernels use it for |g| > 0.95)
     PMC_FN_PHASE_VALUE           (g, cos)                          -> phaseValue of a Henyey-Greenstein component: one of the two above
     PMC_FN_HG_COSINE             (g, X)                            -> (PhaseHG::cosineFor, 1 if the scattering event takes the isotropic branch for
                                                                       this g instead -- PhaseHG::isotropic -- else 0)
     PMC_FN_DIPOLE_VALUE          (cos)                             -> PhaseDipole::value
     PMC_FN_RANDOM_DIRECTION      (u1, u2)                          -> (kx, ky, kz): randomDirection with these two deviates
     PMC_FN_DIRECTION_ABOUT       (kx, ky, kz, cos, u)              -> (kx', ky', kz'): directionAbout with this deviate
     PMC_FN_LAMBERT_LOWER_BRANCH  (z)                               -> lambertLowerBranch
     PMC_FN_GENERALIZED_EXP       (p, x)                            -> generalizedExp
     PMC_FN_INTERPOLATE_LOGLOG    (x, x1, x2, f1, f2)               -> interpolateLogLog
     PMC_FN_LNMEAN                (x1, x2, ln x1, ln x2)            -> lnmean
     PMC_FN_PEEL_TAUMAX           (W, lambda)                       -> peelTaumax
     PMC_FN_SHIFTED_WAVELENGTH    (lambda0, kx, ky, kz, vx, vy, vz) -> shiftedEmissionWavelength
   No tuple is refused for its values: the functions are total (a value outside a function's domain gives what IEEE arithmetic makes of it). */
enum
{
    PMC_FN_HG_VALUE = 0,
    PMC_FN_HG_CONE_MEAN = 1,
    PMC_FN_PHASE_VALUE = 2,
    PMC_FN_HG_COSINE = 3,
    PMC_FN_DIPOLE_VALUE = 4,
    PMC_FN_RANDOM_DIRECTION = 5,
    PMC_FN_DIRECTION_ABOUT = 6,
    PMC_FN_LAMBERT_LOWER_BRANCH = 7,
    PMC_FN_GENERALIZED_EXP = 8,
    PMC_FN_INTERPOLATE_LOGLOG = 9,
    PMC_FN_LNMEAN = 10,
    PMC_FN_PEEL_TAUMAX = 11,
    PMC_FN_SHIFTED_WAVELENGTH = 12,
    PMC_FN_COUNT = 13
};
int pmc_tune_device_function(pmc_ctx* ctx, int32_t function, const double* args, int64_t n, double* out);
/* width_in and width_out of a function (pure host code; ctx is not involved); PMC_ERR_INVALID for an unknown function */
int pmc_tune_device_function_widths(int32_t function, int32_t* width_in, int32_t* width_out);

/* The table searches on the ascending table nodes[num_nodes] (num_nodes >= 2) that the call passes: kind 0 locate (NR::locate: the last node belongs
   to the last bin, -1 below the first node, num_nodes - 1 above the last), 1 locateClip (clipped to [0, num_nodes - 2]), 2 locateBasic (the index of the
   last node <= x, -1 .. num_nodes - 1); index_out: n int32. */
int pmc_tune_locate(pmc_ctx* ctx, int32_t kind, const double* nodes, int32_t num_nodes, const double* x, int64_t n, int32_t* index_out);

/* What the scene-bound aids below work with: the constants of instrument `instrument` as the device holds them (every integer an int64_t;
   include_ifu: it records frames, and only then do xpmin .. nyp describe one; include_sed: it records an SED), and its
   wavelength grid -- border[num_border] and ellv[num_border + 1], each copied if the pointer is not NULL (call once with NULL for num_border). */
typedef struct pmc_instrument_values
{
    double costheta, sintheta, cosphi, sinphi, cosomega, sinomega;
    double xpmin, xpsiz, ypmin, ypsiz;
    double aperture_r2, zp1;
    int64_t nxp, nyp, num_border, num_lambda, include_sed, include_ifu;
} pmc_instrument_values;
int pmc_tune_instrument(pmc_ctx* ctx, int32_t instrument, pmc_instrument_values* out, double* border, int32_t* ellv);
/* pixelOnDetector (pixel_out: i + nxp j, -1 off the frame) and insideAperture (inside_out: 1 or 0; 1 without an aperture) of instrument `instrument`
   for n positions r[n][3] (m) */
int pmc_tune_detector(pmc_ctx* ctx, int32_t instrument, const double* r, int64_t n, int32_t* pixel_out, int32_t* inside_out);
/* the wavelength bin of instrument `instrument` for n rest wavelengths lambda[n] (m), as the launch kernel finds it: ellv[number of borders <=
   lambda (1 + z)], -1 outside the grid */
int pmc_tune_wavelength_bins(pmc_ctx* ctx, int32_t instrument, const double* lambda, int64_t n, int32_t* ell_out);
/* angularProbability of source `source` (PMC_ANGULAR_LASER, _CONICAL or _NETZER; PMC_ERR_INVALID for an isotropic source, for which the kernels
   never call it) for n directions k[n][3]; kind_out, axis_out[3], cos_delta_out: the source's distribution as the device holds it (each may be NULL) */
int pmc_tune_angular_probabilities(pmc_ctx* ctx, int32_t source, const double* k, int64_t n, double* p_out, int32_t* kind_out, double* axis_out,
                                   double* cos_delta_out);

/* ---- Test aid: ONE cycle's walks of slot group 0 for n slots whose state the HOST supplies, through the code a generation of pmc_run_primary runs
   (the cycle start kernel -- with the peel sort's count pass where the segment plan sorts --, then the walk kernels the plan selects for the context's
   grid and flavour, on the context's streams, cursors and sort buffers), with the results as the walk kernels leave them, before any transition kernel.
   Slot i of the call is slot i of the group.  Per slot (every array [n] unless said otherwise):
     r, k            [n][3] position (finite) and propagation direction (a unit vector to 1e-12)
     mask            the observer bits of the mode word (bits 8-23: bit 8 + i = a peel-off walk towards instrument i, which must lead an observer
                     group); the aid adds the alive bit
     ppW             [num_instruments][n] weight of the peel-off packet (read where the mask names the instrument; <= 0: no contribution)
     u1, u2          forced scattering: the uniforms of simulateForcedPropagation, in [0, 1) (they travel in sint / nint as the transition kernel
                     leaves them)
     depth           no forced scattering: the drawn interaction depth (>= 0, inf allowed; it travels in tausample)
     hint            -1, or a cell that may hold the position (device numbering of a tree grid: pmc_tune_cell_numbering; no padding slot)
     nscatt          > 0 (the aid does not start emission cycles)
     lambda, dust_ext, dust_sca, dust_abs, dust_idx[num_media][n]
                     a scene with more than one wavelength: the packet's wavelength and the cross sections that travel with it (dust_abs with
                     explicit absorption, dust_idx with several medium components: each component's wavelength index); NULL otherwise
     W, rfell        a stored radiation field: the packet's weight and its bin of the field's grid (-1: outside); NULL otherwise.  The walks' contributions
                     are ADDED to the context's table (through the log where the plan logs them: flushed before the call returns)
   live_list = 0: the slots run as the group's slot range; 1 (an octree whose plan keeps lists of live slots): as the list of a sparse
   generation, in the order list[n] gives (a permutation of 0 .. n - 1; NULL: ascending).
   Out: ptau[num_instruments][n] (written by the walks the mask names; the others keep PMC_WALK_CYCLE_UNSET), sint, nint, mint (device numbering),
   taupath, tausample [n] (forced scattering: PMC_WALK_CYCLE_UNSET where no second pass ran; sint and nint then still hold u1 and u2); visits, rewalks, paths: what the call added to the counters of pmc_counters (cell_visits, rewalk_visits, paths -- the
   cycle start kernel counts one path per walk, the walk kernels one per second pass); internal_errors: what it added to the internal-error counter.
   Everything is checked first: PMC_ERR_INVALID with a message instead of a launch (n against the slots of group 0 -- pmc_set_num_slots sets the pool --,
   positions, directions, hints, masks, ranges of the other values, arrays the scene needs).  The counters of pmc_counters and pmc_walk_work are put back,
   and a following pmc_run_primary gives the frames it gives without the call.  No reference counterpart. */
#define PMC_WALK_CYCLE_UNSET (-1.)
typedef struct pmc_walk_cycle_in
{
    int64_t n;
    int32_t live_list;
    const int32_t* list;
    const double *r, *k;
    const int32_t* mask;
    const double* ppW;
    const double *u1, *u2, *depth;
    const int32_t *hint, *nscatt;
    const double *lambda, *dust_ext, *dust_sca, *dust_abs;
    const int32_t* dust_idx;
    const double* W;
    const int32_t* rfell;
} pmc_walk_cycle_in;
typedef struct pmc_walk_cycle_out
{
    double *ptau, *sint, *nint;
    int32_t* mint;
    double *taupath, *tausample;
    uint64_t visits, rewalks, paths, internal_errors;
} pmc_walk_cycle_out;
int pmc_tune_walk_cycle(pmc_ctx* ctx, const pmc_walk_cycle_in* in, pmc_walk_cycle_out* out);
/* the slots of group 0 under the segment plan of this context as it stands (the largest n of pmc_tune_walk_cycle), whether the plan keeps lists
   of live slots (live_list = 1 is accepted), the instruments of the scene (rows of ppW and ptau) and its medium components (rows of dust_idx; 1 for
   a scene with one medium); allocates the slot pool if it is not there yet */
int pmc_tune_walk_cycle_limits(pmc_ctx* ctx, int64_t* max_slots, int32_t* live_lists, int32_t* num_instruments, int32_t* num_media);

#ifdef __cplusplus
}
#endif
#endif
