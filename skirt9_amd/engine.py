"""ctypes binding of the HIP engine (libpmc.so, include/pmc.h).

The engine replaces the parallel section of ``MonteCarloSimulation::runPrimaryEmission``
(SKIRT/core/MonteCarloSimulation.cpp:126-129: ``parallel->call(Npp, performLifeCycle)`` followed by
``instrumentSystem()->flush()``).  There is NO CPU fallback: importing works anywhere (so that the build can be
checked on a machine without a GPU) but creating an ``Engine`` without a HIP device raises ``RuntimeError``.
"""
import ctypes as C
import os

import numpy as np

from .host import AdaptiveMesh, CounterValues, DustHeating, FrameLayout, SceneExt, SceneHead, heating_struct, mesh_struct

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")

# every symbol include/pmc.h and include/pmc_tuning.h declare
SYMBOLS = ["pmc_abi_version", "pmc_build_info", "pmc_last_error", "pmc_frame_layout_of", "pmc_create", "pmc_create_ext", "pmc_destroy", "pmc_bind_frames",
           "pmc_clear_frames", "pmc_run_primary", "pmc_set_progress", "pmc_sync", "pmc_download", "pmc_frames_device", "pmc_frames_size",
           "pmc_last_kernel_ms", "pmc_counters", "pmc_reset_counters", "pmc_trace_ray", "pmc_integrate_rays",
           "pmc_last_integrate_work", "pmc_integrate_weighted_rays", "pmc_sample_cells", "pmc_last_sample_ms", "pmc_dust_temperatures",
           "pmc_last_temperature_ms", "pmc_set_launch",
           "pmc_set_num_slots", "pmc_last_timing", "pmc_last_walk_timing", "pmc_walk_work", "pmc_radiation_field_size", "pmc_radiation_field_device",
           "pmc_download_radiation_field", "pmc_clear_radiation_field", "pmc_bind_radiation_field", "pmc_sampler_create",
           "pmc_sampler_density", "pmc_sampler_destroy", "pmc_sampler_create_mesh", "pmc_history_range", "pmc_comm_init_all", "pmc_comm_unique_id",
           "pmc_comm_init_rank", "pmc_comm_size", "pmc_comm_destroy", "pmc_reduce_frames", "pmc_allreduce_radiation_field",
           "pmc_debug_tables", "pmc_tuning_set", "pmc_tuning_clear", "pmc_tune_dipole_cosines", "pmc_tune_source_velocities",
           "pmc_launch_flavour", "pmc_tune_log_geometry", "pmc_tune_log_partition", "pmc_tune_rf_log_flush", "pmc_tune_stat_log_flush",
           "pmc_tune_cell_numbering", "pmc_tune_device_function", "pmc_tune_device_function_widths", "pmc_tune_locate", "pmc_tune_instrument",
           "pmc_tune_detector", "pmc_tune_wavelength_bins", "pmc_tune_angular_probabilities", "pmc_tune_walk_cycle", "pmc_tune_walk_cycle_limits"]

# the scene-free device functions of pmc_tune_device_function (include/pmc_tuning.h PMC_FN_*)
DEVICE_FUNCTIONS = {"hg_value": 0, "hg_cone_mean": 1, "phase_value": 2, "hg_cosine": 3, "dipole_value": 4, "random_direction": 5, "direction_about": 6,
                    "lambert_lower_branch": 7, "generalized_exp": 8, "interpolate_loglog": 9, "lnmean": 10, "peel_taumax": 11, "shifted_wavelength": 12}
LOCATE_KINDS = {"locate": 0, "locate_clip": 1, "locate_basic": 2}

_lib = None


class DebugTables(C.Structure):
    """pmc_debug_table_values (include/pmc_tuning.h): device addresses for profiles/microbench/bridge.hip"""
    _fields_ = [("cell_table", C.c_void_p), ("cell_slots", C.c_int64), ("loose_base", C.c_int64), ("task_cell", C.c_void_p), ("num_slots", C.c_int64)]


class WalkWork(C.Structure):
    """pmc_walk_work_values (include/pmc_tuning.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("peel_wave_steps", "peel_lane_steps", "peel_rounds", "prop_wave_steps",
                                          "prop_lane_steps", "prop_rounds")]


class InstrumentValues(C.Structure):
    """pmc_instrument_values (include/pmc_tuning.h)"""
    _fields_ = ([(n, C.c_double) for n in ("costheta", "sintheta", "cosphi", "sinphi", "cosomega", "sinomega", "xpmin", "xpsiz", "ypmin", "ypsiz",
                                           "aperture_r2", "zp1")]
                + [(n, C.c_int64) for n in ("nxp", "nyp", "num_border", "num_lambda", "include_sed", "include_ifu")])


class LogGeometry(C.Structure):
    """pmc_log_geometry_values (include/pmc_tuning.h)"""
    _fields_ = [(n, C.c_int64) for n in ("cell_slots", "rf_num_lambda", "rf_keys", "rf_parts", "rf_logged", "stat_records", "stat_parts", "stat_logged",
                                         "chunk", "rf_bucket_bits", "stat_bucket_bits", "scan_threads", "sort_block", "max_parts", "reduce_span",
                                         "rf_short_run", "stat_short_run", "max_entries")]


class WalkCycleIn(C.Structure):
    """pmc_walk_cycle_in (include/pmc_tuning.h)"""
    _fields_ = ([("n", C.c_int64), ("live_list", C.c_int32)]
                + [(n, C.c_void_p) for n in ("list", "r", "k", "mask", "ppW", "u1", "u2", "depth", "hint", "nscatt", "wavelength", "dust_ext", "dust_sca",
                                             "dust_abs", "dust_idx", "W", "rfell")])


class WalkCycleOut(C.Structure):
    """pmc_walk_cycle_out (include/pmc_tuning.h)"""
    _fields_ = ([(n, C.c_void_p) for n in ("ptau", "sint", "nint", "mint", "taupath", "tausample")]
                + [(n, C.c_uint64) for n in ("visits", "rewalks", "paths", "internal_errors")])


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("PMC_LIBRARY") or os.path.join(_LIBDIR, "libpmc.so")  # override: kernel A/B experiments
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the HIP engine has not been built (run `make` or "
                               "__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(path)
        L.pmc_abi_version.restype = C.c_int
        L.pmc_last_error.restype = C.c_char_p
        L.pmc_build_info.restype = C.c_char_p
        L.pmc_frame_layout_of.restype = C.c_int64
        L.pmc_frame_layout_of.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FrameLayout)]
        L.pmc_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        if hasattr(L, "pmc_create_ext"):  # (absent from engines built from an older commit and loaded through PMC_LIBRARY)
            L.pmc_create_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
            L.pmc_tune_dipole_cosines.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        if hasattr(L, "pmc_tune_source_velocities"):  # (likewise)
            L.pmc_tune_source_velocities.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.pmc_destroy.argtypes = [C.c_void_p]
        L.pmc_bind_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.pmc_clear_frames.argtypes = [C.c_void_p]
        L.pmc_run_primary.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
        L.pmc_sync.argtypes = [C.c_void_p]
        L.pmc_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.pmc_frames_device.restype = C.c_void_p
        L.pmc_frames_device.argtypes = [C.c_void_p]
        L.pmc_frames_size.restype = C.c_int64
        L.pmc_frames_size.argtypes = [C.c_void_p]
        L.pmc_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.pmc_counters.argtypes = [C.c_void_p, C.POINTER(CounterValues)]
        L.pmc_reset_counters.argtypes = [C.c_void_p]
        L.pmc_trace_ray.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        if hasattr(L, "pmc_integrate_rays"):  # (absent from engines built from an older commit and loaded through PMC_LIBRARY)
            L.pmc_integrate_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
            L.pmc_last_integrate_work.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "pmc_dust_temperatures"):  # (likewise)
            L.pmc_integrate_weighted_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pmc_dust_temperatures.argtypes = [C.c_void_p, C.POINTER(DustHeating), C.c_void_p]
            L.pmc_last_temperature_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        if hasattr(L, "pmc_sample_cells"):  # (likewise)
            L.pmc_sample_cells.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pmc_last_sample_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.pmc_set_launch.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.pmc_set_num_slots.argtypes = [C.c_void_p, C.c_int64]
        L.pmc_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_int32)]
        if hasattr(L, "pmc_walk_work"):
            # (absent only from engines built from an older commit and loaded through PMC_LIBRARY for kernel A/B experiments:
            # tools/sweep.py copes without these two; every other prototype below is still set)
            L.pmc_last_walk_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            L.pmc_walk_work.argtypes = [C.c_void_p, C.POINTER(WalkWork)]
        L.pmc_radiation_field_size.restype = C.c_int64
        L.pmc_radiation_field_size.argtypes = [C.c_void_p]
        L.pmc_radiation_field_device.restype = C.c_void_p
        L.pmc_radiation_field_device.argtypes = [C.c_void_p]
        L.pmc_download_radiation_field.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.pmc_clear_radiation_field.argtypes = [C.c_void_p]
        L.pmc_bind_radiation_field.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.pmc_history_range.restype = None
        L.pmc_history_range.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pmc_comm_init_all.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]
        L.pmc_comm_unique_id.argtypes = [C.c_void_p]
        L.pmc_comm_init_rank.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.pmc_comm_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.pmc_comm_destroy.restype = None
        L.pmc_comm_destroy.argtypes = [C.c_void_p]
        L.pmc_reduce_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.pmc_allreduce_radiation_field.argtypes = [C.c_void_p, C.c_void_p]
        L.pmc_sampler_create.argtypes = [C.POINTER(Particles), C.c_int32, C.POINTER(C.c_void_p)]
        L.pmc_sampler_density.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.pmc_sampler_destroy.restype = None
        L.pmc_sampler_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "pmc_sampler_create_mesh"):  # (absent from engines built from an older commit and loaded through PMC_LIBRARY)
            L.pmc_sampler_create_mesh.argtypes = [C.POINTER(AdaptiveMesh), C.c_int32, C.POINTER(C.c_void_p)]
        if hasattr(L, "pmc_tuning_set"):
            L.pmc_tuning_set.argtypes = [C.c_char_p, C.c_char_p]
            L.pmc_tuning_clear.restype = None
        if hasattr(L, "pmc_tune_log_geometry"):  # (absent from engines built from an older commit and loaded through PMC_LIBRARY)
            L.pmc_tune_log_geometry.argtypes = [C.c_void_p, C.POINTER(LogGeometry)]
            L.pmc_tune_log_partition.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
            L.pmc_tune_rf_log_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
            L.pmc_tune_stat_log_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
            L.pmc_tune_cell_numbering.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "pmc_tune_device_function"):  # (likewise)
            L.pmc_tune_device_function.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
            L.pmc_tune_device_function_widths.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.pmc_tune_locate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
            L.pmc_tune_instrument.argtypes = [C.c_void_p, C.c_int32, C.POINTER(InstrumentValues), C.c_void_p, C.c_void_p]
            L.pmc_tune_detector.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.pmc_tune_wavelength_bins.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
            L.pmc_tune_angular_probabilities.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                                         C.POINTER(C.c_double)]
        if hasattr(L, "pmc_tune_walk_cycle"):  # (likewise)
            L.pmc_tune_walk_cycle.argtypes = [C.c_void_p, C.POINTER(WalkCycleIn), C.POINTER(WalkCycleOut)]
            L.pmc_tune_walk_cycle_limits.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib = L
    return _lib


# settings the library itself reads from the environment (include/pmc.h); every other PMC_* name is a tuning switch
# values whose sums pmc_integrate_rays keeps in registers per pass over the rays (include/pmc.h PMC_INTEGRATE_PASS_VALUES)
INTEGRATE_PASS_VALUES = 4
# rays that pmc_integrate_rays keeps on the device at a time (include/pmc.h PMC_INTEGRATE_BATCH_RAYS)
INTEGRATE_BATCH_RAYS = 1 << 22
# points that pmc_sample_cells keeps on the device at a time (include/pmc.h PMC_SAMPLE_CHUNK_POINTS)
SAMPLE_CHUNK_POINTS = 1 << 20

ENVIRONMENT_SETTINGS = ("PMC_NUM_SLOTS", "PMC_NUM_GROUPS", "PMC_STAT_POOL_BLOCKS")


def set_tuning(name, value="1"):
    """a tuning switch of the engine (include/pmc_tuning.h pmc_tuning_set): alternative code paths for cross-checks and A/B
    timing; value None removes it.  (Engines built before the switch table existed read the same names from the environment.)"""
    L = lib()
    if hasattr(L, "pmc_tuning_set"):
        _check(L.pmc_tuning_set(name.encode(), None if value is None else str(value).encode()))
    elif value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def clear_tuning():
    L = lib()
    if hasattr(L, "pmc_tuning_clear"):
        L.pmc_tuning_clear()


def tuning_from_environment():
    """tools only (bench.py, tools/sweep.py): hands the PMC_* variables of the environment that are not library settings to the
    engine as tuning switches -- the library itself does not read them"""
    for key, value in os.environ.items():
        if key.startswith("PMC_") and key not in ENVIRONMENT_SETTINGS and key != "PMC_LIBRARY":
            set_tuning(key, value)


def _ptr(array):
    """the address of a numpy array for a void* argument; None: a null pointer"""
    return None if array is None else array.ctypes.data_as(C.c_void_p)


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"pmc error {rc}: {lib().pmc_last_error().decode()}")


def history_range(num_packets, rank, num_ranks):
    """[first, first + count) of rank `rank` of `num_ranks` for a segment of num_packets histories (pmc_history_range:
    the one implementation the CLI driver, the bench and the tests share; pure host code)"""
    first, count = C.c_uint64(0), C.c_uint64(0)
    lib().pmc_history_range(int(num_packets), int(rank), int(num_ranks), C.byref(first), C.byref(count))
    return int(first.value), int(count.value)


class Communicator:
    """RCCL communicator(s) behind the C ABI: ``Communicator.all(devices)`` for one process that drives several
    devices (one handle per device), ``Communicator.rank(device, num_ranks, rank, unique_id)`` for one process per
    device (``Communicator.unique_id()`` on rank 0, handed to the others by the launcher)."""

    def __init__(self, handles):
        self.handles = handles

    @classmethod
    def all(cls, devices):
        n = len(devices)
        dev = (C.c_int32 * n)(*devices)
        out = (C.c_void_p * n)()
        _check(lib().pmc_comm_init_all(n, dev, out))
        return cls([C.c_void_p(h) for h in out])

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().pmc_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def rank(cls, device, num_ranks, rank, unique_id):
        out = C.c_void_p()
        _check(lib().pmc_comm_init_rank(device, num_ranks, rank, C.c_char_p(unique_id), C.byref(out)))
        return cls([out])

    def size(self, index=0):
        """(ranks of the communicator, rank of handle `index` in it) as RCCL reports them"""
        n, me = C.c_int32(0), C.c_int32(0)
        _check(lib().pmc_comm_size(self.handles[index], C.byref(n), C.byref(me)))
        return int(n.value), int(me.value)

    def close(self):
        for h in self.handles:
            lib().pmc_comm_destroy(h)
        self.handles = []


class Particles(C.Structure):
    """pmc_particles (include/pmc.h)"""
    _fields_ = [("kernel", C.c_int32), ("num_particles", C.c_int64), ("particle", C.POINTER(C.c_double)), ("num_blocks", C.c_int32),
                ("xgrid", C.POINTER(C.c_double)), ("ygrid", C.POINTER(C.c_double)), ("zgrid", C.POINTER(C.c_double)),
                ("block_start", C.POINTER(C.c_int64)), ("block_list", C.POINTER(C.c_int32))]


KERNEL_CUBIC_SPLINE, KERNEL_UNIFORM = 1, 2  # PMC_KERNEL_* (include/pmc.h)


class _Sampler:
    """what the two kinds of density sampler share: pmc_sampler_density and pmc_sampler_destroy serve both"""
    _h = None

    def density(self, positions):
        """the density at the positions [n][3]"""
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        out = np.empty(r.shape[0], dtype=np.float64)
        _check(lib().pmc_sampler_density(self._h, _ptr(r), r.shape[0], _ptr(out)))
        return out

    def close(self):
        if self._h:
            lib().pmc_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshSampler(_Sampler):
    """The density of a medium imported from an adaptive mesh at many positions, on one MI355X (pmc_sampler_create_mesh,
    pmc_sampler_density): ``tables`` as ``skirt9_amd.host.Simulation.adaptive_mesh`` returns them.  A malformed table is refused before any
    device call; there is no CPU fallback.  ``density`` is 0 outside the root box; RuntimeError with the reference's words and the lowest
    failing index for a position that the reference's descent cannot locate."""

    def __init__(self, tables, device=0):
        struct, keep = mesh_struct(tables)
        self._h = C.c_void_p()
        _check(lib().pmc_sampler_create_mesh(C.byref(struct), device, C.byref(self._h)))
        del keep  # (the tables are copied to the device)


class ParticleSampler(_Sampler):
    """The density of a medium imported from smoothed particles at many positions, on one MI355X (pmc_sampler_create, pmc_sampler_density).
    ``tables``: a dict with the members of pmc_particles -- kernel (KERNEL_*), particle [n][5], xgrid / ygrid / zgrid [num_blocks + 1],
    block_start [num_blocks^3 + 1], block_list.  The lists are trusted as they come; there is no CPU fallback."""

    def __init__(self, tables, device=0):
        keep = {"particle": np.ascontiguousarray(tables["particle"], dtype=np.float64).reshape(-1, 5),
                "block_start": np.ascontiguousarray(tables["block_start"], dtype=np.int64).reshape(-1),
                "block_list": np.ascontiguousarray(tables["block_list"], dtype=np.int32).reshape(-1)}
        for axis in ("xgrid", "ygrid", "zgrid"):
            keep[axis] = np.ascontiguousarray(tables[axis], dtype=np.float64).reshape(-1)
        nb = keep["xgrid"].shape[0] - 1
        if keep["ygrid"].shape[0] != nb + 1 or keep["zgrid"].shape[0] != nb + 1 or keep["block_start"].shape[0] != nb ** 3 + 1:
            raise ValueError("xgrid, ygrid, zgrid and block_start must describe the same blocks")
        if keep["block_list"].shape[0] != keep["block_start"][-1]:
            raise ValueError("block_list must have block_start[-1] entries")
        struct = Particles(int(tables["kernel"]), keep["particle"].shape[0], num_blocks=nb)
        for name, array in keep.items():
            setattr(struct, name, array.ctypes.data_as(dict(Particles._fields_)[name]))
        self._h = C.c_void_p()
        _check(lib().pmc_sampler_create(C.byref(struct), device, C.byref(self._h)))
        del keep  # (the tables are copied to the device)


class Engine:
    """One engine context on one MI355X: device copies of a scene plus the detector arrays."""

    def __init__(self, scene_ptr, device=0):
        """scene_ptr: address of a pmc_scene (e.g. ``skirt9_amd.host.Simulation.scene``, which carries the address of the scene's
        extension along: ``skirt9_amd.host.ScenePointer``; a plain int means no extension)"""
        self._h = C.c_void_p()
        L = lib()
        ext = getattr(scene_ptr, "ext", None)
        if hasattr(L, "pmc_create_ext"):
            _check(L.pmc_create_ext(int(scene_ptr), ext, device, C.byref(self._h)))
        else:
            # (an engine from before the extension knows Henyey-Greenstein only: another phase function must not run as that)
            if ext and any(SceneExt.from_address(ext).phase_function):
                raise RuntimeError("this libpmc.so has no pmc_create_ext: it cannot run a scene with a dipole component")
            if ext and any(v.kind for v in SceneExt.from_address(ext).source_velocity):
                raise RuntimeError("this libpmc.so has no pmc_create_ext: it cannot run a scene with a moving source")
            _check(L.pmc_create(int(scene_ptr), device, C.byref(self._h)))
        self.device = device
        self.num_cells = int(SceneHead.from_address(int(scene_ptr)).grid.num_cells)

    def close(self):
        if getattr(self, "_h", None):
            lib().pmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def frame_size(self):
        return int(lib().pmc_frames_size(self._h))

    @property
    def frames_device_ptr(self):
        return int(lib().pmc_frames_device(self._h))

    def bind_frames(self, device_ptr, num_doubles):
        """accumulate into caller-owned device memory (e.g. ``tensor.data_ptr()`` of a zeroed float64 torch tensor)"""
        _check(lib().pmc_bind_frames(self._h, C.c_void_p(device_ptr), num_doubles))

    def set_launch(self, block=0, grid=0):
        _check(lib().pmc_set_launch(self._h, block, grid))

    def clear(self):
        _check(lib().pmc_clear_frames(self._h))

    def run_primary(self, first, count, seed):
        """asynchronous launch of histories [first, first+count); accumulates into the frames"""
        _check(lib().pmc_run_primary(self._h, first, count, seed))

    def set_progress(self, report, interval_seconds=3.0):
        """report(launched, count) is called from run_primary at most once per interval (MonteCarloSimulation::logProgress); None: off"""
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64)
        self._progress = proto(lambda user, launched, count: report(int(launched), int(count))) if report else None  # (kept alive)
        lib().pmc_set_progress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        _check(lib().pmc_set_progress(self._h, C.cast(self._progress, C.c_void_p) if self._progress else None, None, float(interval_seconds)))

    def sync(self):
        _check(lib().pmc_sync(self._h))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        _check(lib().pmc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_num_slots(self, n):
        _check(lib().pmc_set_num_slots(self._h, int(n)))

    def last_timing(self):
        """HIP-event times of the last segment: dict(total_ms, walk_ms, transition_ms, generations)"""
        t, w, x, g = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int32(0)
        _check(lib().pmc_last_timing(self._h, C.byref(t), C.byref(w), C.byref(x), C.byref(g)))
        return {"total_ms": float(t.value), "walk_ms": float(w.value), "transition_ms": float(x.value),
                "generations": int(g.value)}

    def last_walk_timing(self):
        """octree: HIP-event spans of the peel-off kernels and of the propagation kernel of the last segment (they overlap)"""
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().pmc_last_walk_timing(self._h, C.byref(a), C.byref(b)))
        return {"peel_ms": float(a.value), "prop_ms": float(b.value)}

    def walk_work(self):
        """counted wave-steps, lane-steps and bookkeeping rounds of the octree walk kernels since create / reset"""
        w = WalkWork()
        _check(lib().pmc_walk_work(self._h, C.byref(w)))
        return {n: int(getattr(w, n)) for n, _ in w._fields_}

    def debug_tables(self):
        """device addresses of the octree walk's hot table and of the task records' first cells (tuning aid)"""
        t = DebugTables()
        lib().pmc_debug_tables.argtypes = [C.c_void_p, C.POINTER(DebugTables)]
        _check(lib().pmc_debug_tables(self._h, C.byref(t)))
        return t

    def launch_flavour(self):
        """the launch kernel the next run_primary uses (include/pmc_tuning.h pmc_launch_flavour): 0 or 1 is the generic kernel"""
        f = C.c_int32(-1)
        lib().pmc_launch_flavour.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        _check(lib().pmc_launch_flavour(self._h, C.byref(f)))
        return int(f.value)

    def reduce_frames(self, comm_handle, root=0):
        """end of a segment on several devices: ONE ncclReduce (f64, sum) of the detector arrays onto `root`
        (ProcessManager::sumToRoot behind FluxRecorder::flush); the other ranks' arrays are cleared"""
        _check(lib().pmc_reduce_frames(self._h, comm_handle, root))

    def allreduce_radiation_field(self, comm_handle):
        """ncclAllReduce of the radiation field table (MediumSystem::communicateRadiationField)"""
        _check(lib().pmc_allreduce_radiation_field(self._h, comm_handle))

    def download(self):
        out = np.empty(self.frame_size, dtype=np.float64)
        _check(lib().pmc_download(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    @property
    def radiation_field_size(self):
        return int(lib().pmc_radiation_field_size(self._h))

    @property
    def radiation_field_device_ptr(self):
        """device address of the radiation field table (for an RCCL all-reduce across ranks)"""
        return int(lib().pmc_radiation_field_device(self._h) or 0)

    def bind_radiation_field(self, device_ptr, num_doubles):
        """accumulate the radiation field into caller-owned device memory (a zeroed float64 torch tensor), so that
        ``Engine.allreduce_radiation_field`` / pmc_allreduce_radiation_field sums it over the ranks"""
        _check(lib().pmc_bind_radiation_field(self._h, C.c_void_p(device_ptr), num_doubles))

    def download_radiation_field(self):
        """rf[m * nbins + ell] accumulated by the segments run so far (MediumSystem::_rf1)"""
        out = np.empty(self.radiation_field_size, dtype=np.float64)
        _check(lib().pmc_download_radiation_field(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def clear_radiation_field(self):
        _check(lib().pmc_clear_radiation_field(self._h))

    def counters(self):
        c = CounterValues()
        _check(lib().pmc_counters(self._h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        _check(lib().pmc_reset_counters(self._h))

    def dipole_cosines(self, u):
        """test aid (pmc_tune_dipole_cosines): the scattering cosines that the transition kernel's dipole sampler makes of the uniform deviates u"""
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.empty_like(u)
        _check(lib().pmc_tune_dipole_cosines(self._h, u.ctypes.data_as(C.c_void_p), u.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def source_velocities(self, source, positions):
        """test aid (pmc_tune_source_velocities): the velocity (m/s) that the launch kernel's velocity function gives source `source` at
        the positions [n][3] (m)"""
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(r)
        _check(lib().pmc_tune_source_velocities(self._h, int(source), r.ctypes.data_as(C.c_void_p), r.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def log_geometry(self):
        """test aid (pmc_tune_log_geometry): the geometry of this context's radiation-field and statistics logs and the constants their
        kernels are built with, as a dict of ints (the members of include/pmc_tuning.h pmc_log_geometry_values)"""
        g = LogGeometry()
        _check(lib().pmc_tune_log_geometry(self._h, C.byref(g)))
        return {n: int(getattr(g, n)) for n, _ in g._fields_}

    def _log_arrays(self, keys, vals, fills):
        """a host log as the aids take it: n = len(keys); None stays a null pointer (the library refuses it)"""
        keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.float64).reshape(-1)
        fills = None if fills is None else np.ascontiguousarray(fills, dtype=np.uint32).reshape(-1)
        n = 0 if keys is None else keys.size
        if vals is not None and keys is not None and vals.size != n:
            raise ValueError("keys and vals differ in length")
        if keys is None and vals is not None:
            n = vals.size
        if fills is not None and fills.size * self.log_geometry()["chunk"] < n:
            raise ValueError("fills has fewer entries than the log has chunks")
        return n, keys, vals, fills

    def log_partition(self, stat, num_parts, keys, vals, fills=None):
        """test aid (pmc_tune_log_partition): the counting sort of the logs alone, on a host-supplied log of len(keys) entries and `num_parts`
        partitions; stat: the statistics log's instantiation.  Returns (sorted_keys, sorted_vals, start[num_parts + 1])"""
        n, keys, vals, fills = self._log_arrays(keys, vals, fills)
        sorted_keys, sorted_vals = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.float64)
        start = np.zeros(max(int(num_parts), 0) + 1, dtype=np.uint64)
        _check(lib().pmc_tune_log_partition(self._h, int(stat), int(num_parts), _ptr(keys), _ptr(vals), _ptr(fills), n, _ptr(sorted_keys), _ptr(sorted_vals),
                                            _ptr(start)))
        return sorted_keys, sorted_vals, start

    def rf_log_flush(self, keys, vals):
        """test aid (pmc_tune_rf_log_flush): a host-supplied radiation-field log through the sort and rfReduceKernel into the context's table"""
        n, keys, vals, _ = self._log_arrays(keys, vals, None)
        _check(lib().pmc_tune_rf_log_flush(self._h, _ptr(keys), _ptr(vals), n))

    def stat_log_flush(self, keys, vals, fills=None):
        """test aid (pmc_tune_stat_log_flush): a host-supplied statistics log through the sort and statReduceKernel; returns the accumulator,
        [stat_records][5] = count, sums of w, w^2, w^3, w^4 per record, and leaves it cleared"""
        n, keys, vals, fills = self._log_arrays(keys, vals, fills)
        acc = np.empty((self.log_geometry()["stat_records"], 5), dtype=np.float64)
        _check(lib().pmc_tune_stat_log_flush(self._h, _ptr(keys), _ptr(vals), _ptr(fills), n, _ptr(acc)))
        return acc

    def cell_numbering(self):
        """test aid (pmc_tune_cell_numbering): the caller's cell index of every cell of the device numbering of a tree grid, -1: a padding slot"""
        ext = np.empty(self.log_geometry()["cell_slots"], dtype=np.int32)
        _check(lib().pmc_tune_cell_numbering(self._h, _ptr(ext)))
        return ext

    def device_function(self, function, args, n=None):
        """test aid (pmc_tune_device_function): the scalar device function `function` (a name of DEVICE_FUNCTIONS or a number) over the argument
        tuples args[n][width_in]; returns out[n][width_out].  n: the number of tuples, where it is not len(args) (None args: a null pointer)"""
        fn = DEVICE_FUNCTIONS.get(function, function)
        win, wout = C.c_int32(1), C.c_int32(1)
        lib().pmc_tune_device_function_widths(int(fn), C.byref(win), C.byref(wout))  # (an unknown function: the call below says so)
        a = None if args is None else np.ascontiguousarray(args, dtype=np.float64).reshape(-1, win.value)
        count = (0 if a is None else a.shape[0]) if n is None else int(n)
        out = np.empty((max(count, 0), wout.value), dtype=np.float64)
        _check(lib().pmc_tune_device_function(self._h, int(fn), _ptr(a), count, _ptr(out)))
        return out

    def locate(self, kind, nodes, x, num_nodes=None):
        """test aid (pmc_tune_locate): locate / locate_clip / locate_basic (LOCATE_KINDS, or a number) of the values x in the table `nodes`"""
        nodes = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        out = np.empty(x.size, dtype=np.int32)
        count = (0 if nodes is None else nodes.size) if num_nodes is None else int(num_nodes)
        _check(lib().pmc_tune_locate(self._h, int(LOCATE_KINDS.get(kind, kind)), _ptr(nodes), count, _ptr(x), x.size, _ptr(out)))
        return out

    def instrument_values(self, instrument):
        """test aid (pmc_tune_instrument): the constants of an instrument as the device holds them (a dict), with its wavelength grid as
        `border` and `ellv`"""
        v = InstrumentValues()
        _check(lib().pmc_tune_instrument(self._h, int(instrument), C.byref(v), None, None))
        border, ellv = np.empty(v.num_border, dtype=np.float64), np.empty(v.num_border + 1, dtype=np.int32)
        _check(lib().pmc_tune_instrument(self._h, int(instrument), C.byref(v), _ptr(border), _ptr(ellv)))
        values = {n: getattr(v, n) for n, _ in v._fields_}
        values.update(border=border, ellv=ellv)
        return values

    def detector(self, instrument, positions):
        """test aid (pmc_tune_detector): (pixel, inside) of the positions [n][3] (m): pixelOnDetector (-1 off the frame) and insideAperture"""
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        pixel, inside = np.empty(r.shape[0], dtype=np.int32), np.empty(r.shape[0], dtype=np.int32)
        _check(lib().pmc_tune_detector(self._h, int(instrument), _ptr(r), r.shape[0], _ptr(pixel), _ptr(inside)))
        return pixel, inside

    def wavelength_bins(self, instrument, wavelengths):
        """test aid (pmc_tune_wavelength_bins): the launch kernel's wavelength bin of the instrument for the rest wavelengths (m)"""
        lam = np.ascontiguousarray(wavelengths, dtype=np.float64).reshape(-1)
        ell = np.empty(lam.size, dtype=np.int32)
        _check(lib().pmc_tune_wavelength_bins(self._h, int(instrument), _ptr(lam), lam.size, _ptr(ell)))
        return ell

    def angular_probabilities(self, source, directions):
        """test aid (pmc_tune_angular_probabilities): (p, kind, axis, cos_delta): angularProbability of the directions [n][3] for an anisotropic
        point source, and its distribution as the device holds it"""
        k = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        p, axis = np.empty(k.shape[0], dtype=np.float64), np.empty(3, dtype=np.float64)
        kind, cos_delta = C.c_int32(0), C.c_double(0.)
        _check(lib().pmc_tune_angular_probabilities(self._h, int(source), _ptr(k), k.shape[0], _ptr(p), C.byref(kind), _ptr(axis), C.byref(cos_delta)))
        return p, kind.value, axis, cos_delta.value

    def walk_cycle_limits(self):
        """test aid (pmc_tune_walk_cycle_limits): (slots of group 0 -- the largest n of ``walk_cycle`` --, whether ``live_list`` is accepted,
        instruments of the scene, its medium components)"""
        n, lists, instruments, media = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(lib().pmc_tune_walk_cycle_limits(self._h, C.byref(n), C.byref(lists), C.byref(instruments), C.byref(media)))
        return int(n.value), bool(lists.value), int(instruments.value), int(media.value)

    def walk_cycle(self, r, k, mask, ppW, u1=None, u2=None, depth=None, hint=None, nscatt=None, live_list=False, order=None, wavelength=None,
                   dust_ext=None, dust_sca=None, dust_abs=None, dust_idx=None, W=None, rfell=None, n=None):
        """test aid (pmc_tune_walk_cycle): one cycle's walks of slot group 0 on the slot states given here, through the cycle start kernel and the
        walk kernels a generation of ``run_primary`` runs.  r, k: [n][3]; mask: [n] observer bits of the mode word (1 << (8 + instrument)); ppW:
        [num_instruments][n]; u1, u2 (forced scattering) or depth (not forced); hint: -1 or a cell of the device numbering (default -1); nscatt
        (default 1); live_list: the slots run as the list of a sparse generation, in the order `order` gives; the other arrays as the scene needs
        them (include/pmc_tuning.h).  n: the slot count, where it is not len(r).  Returns a dict: ptau [num_instruments][n], sint, nint, mint
        (device numbering), taupath, tausample, and the ints visits, rewalks, paths, internal_errors"""
        def arr(a, dtype, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            return a if shape is None else a.reshape(shape)
        r, k = arr(r, np.float64, (-1, 3)), arr(k, np.float64, (-1, 3))
        count = (0 if r is None else r.shape[0]) if n is None else int(n)
        room = max(count, 1)
        _, _, num_inst, num_media = self.walk_cycle_limits()
        ppW = arr(ppW, np.float64, (num_inst, -1))
        keep = {"r": r, "k": k, "mask": arr(mask, np.int32), "ppW": ppW, "u1": arr(u1, np.float64), "u2": arr(u2, np.float64),
                "depth": arr(depth, np.float64), "hint": np.full(room, -1, dtype=np.int32) if hint is None else arr(hint, np.int32),
                "nscatt": np.ones(room, dtype=np.int32) if nscatt is None else arr(nscatt, np.int32), "list": arr(order, np.int32),
                "wavelength": arr(wavelength, np.float64), "dust_ext": arr(dust_ext, np.float64), "dust_sca": arr(dust_sca, np.float64),
                "dust_abs": arr(dust_abs, np.float64), "dust_idx": arr(dust_idx, np.int32), "W": arr(W, np.float64), "rfell": arr(rfell, np.int32)}
        for name, value in keep.items():  # (the library reads n elements of every array it is given: a shorter one is refused here)
            per = {"r": 3, "k": 3, "ppW": num_inst, "dust_idx": num_media}.get(name, 1)
            if value is not None and value.size < per * count:
                raise ValueError(f"{name} has {value.size} elements, {count} slots need {per * count}")
        a = WalkCycleIn(n=count, live_list=1 if live_list else 0)
        for name, value in keep.items():
            setattr(a, name, None if value is None else value.ctypes.data)
        res = {"ptau": np.empty((num_inst, room)), "sint": np.empty(room), "nint": np.empty(room), "mint": np.empty(room, dtype=np.int32),
               "taupath": np.empty(room), "tausample": np.empty(room)}
        o = WalkCycleOut()
        for name, value in res.items():
            setattr(o, name, value.ctypes.data)
        _check(lib().pmc_tune_walk_cycle(self._h, C.byref(a), C.byref(o)))
        res = {name: value[..., :count] for name, value in res.items()}
        res.update(visits=int(o.visits), rewalks=int(o.rewalks), paths=int(o.paths), internal_errors=int(o.internal_errors))
        return res

    def trace_ray(self, r, k, cap=4096):
        r = np.ascontiguousarray(r, dtype=np.float64)
        k = np.ascontiguousarray(k, dtype=np.float64)
        m = np.zeros(cap, dtype=np.int32)
        ds = np.zeros(cap, dtype=np.float64)
        n = C.c_int32(0)
        _check(lib().pmc_trace_ray(self._h, r.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p),
                                   m.ctypes.data_as(C.c_void_p), ds.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return m[:n.value].copy(), ds[:n.value].copy()

    def integrate_rays(self, origins, directions, cell_values):
        """sums[i, v] = sum over the path of ray i of ds * cell_values[v, m] (pmc_integrate_rays: the probe maps' line integrals, the segments of
        ``trace_ray`` added up in path order on the device).  origins, directions: [n][3]; cell_values: [V][num_cells] or [num_cells]
        (then the result is [n]); cells in the numbering ``trace_ray`` reports"""
        r = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if r.shape != k.shape:
            raise ValueError("origins and directions differ in shape")
        q = np.ascontiguousarray(cell_values, dtype=np.float64)
        single = q.ndim == 1
        q = q.reshape(1, -1) if single else q
        if q.ndim != 2:
            raise ValueError("cell_values must be [V][num_cells]")
        out = np.zeros((r.shape[0], q.shape[0]), dtype=np.float64)
        if q.shape[1] != self.num_cells:
            raise ValueError(f"cell_values has {q.shape[1]} cells per value, the grid has {self.num_cells}")
        _check(lib().pmc_integrate_rays(self._h, r.shape[0], r.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), q.shape[0],
                                        q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out[:, 0].copy() if single else out

    def integrate_callback(self):
        """``integrate_rays`` as the C callback of skh_write_probes (include/skirt_host.h skh_integrate_fn): (function address, user pointer)"""
        return C.cast(lib().pmc_integrate_rays, C.c_void_p).value, self._h

    def integrate_weighted_rays(self, origins, directions, cell_weights, cell_values):
        """the raw sums of a weighted average along rays (pmc_integrate_weighted_rays): per segment weight = ds * cell_weights[m];
        sums[i, 0] += weight; sums[i, 1 + v] += weight * cell_values[v, m].  cell_weights: [num_cells]; cell_values: [V][num_cells] (V may
        be 0) or [num_cells]; returns [n][1 + V].  The average of value v along ray i is sums[i, 1 + v] / sums[i, 0] where that is not zero"""
        r = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if r.shape != k.shape:
            raise ValueError("origins and directions differ in shape")
        w = np.ascontiguousarray(cell_weights, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(cell_values, dtype=np.float64)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        if q.ndim != 2:
            raise ValueError("cell_values must be [V][num_cells]")
        if w.size != self.num_cells or (q.shape[0] and q.shape[1] != self.num_cells):
            raise ValueError(f"cell_weights and cell_values must have {self.num_cells} cells")
        out = np.zeros((r.shape[0], 1 + q.shape[0]), dtype=np.float64)
        _check(lib().pmc_integrate_weighted_rays(self._h, r.shape[0], r.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), q.shape[0],
                                                 w.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def weighted_callback(self):
        """``integrate_weighted_rays`` as the C callback of skh_write_probes_with (skh_integrate_weighted_fn): (function address, user pointer)"""
        if not hasattr(lib(), "pmc_integrate_weighted_rays"):  # (an engine built from an older commit and loaded through PMC_LIBRARY)
            return None, self._h
        return C.cast(lib().pmc_integrate_weighted_rays, C.c_void_p).value, self._h

    def sample_cells(self, positions, cell_values=None, cells=True):
        """(values, cells) at the positions [n][3] (pmc_sample_cells: the point sampler behind the cut forms of the probes).  cells[p] =
        SpatialGrid::cellIndex(positions[p]) in the numbering ``trace_ray`` reports, -1 outside the grid: the domain box is closed and a position on
        a wall between two cells belongs to the upper one.  values[v, p] = cell_values[v, cells[p]], 0 outside, copied bit for bit;
        cell_values: [V][num_cells], or [num_cells] (then values is [n]), or None (cells only: values is None).  cells=False: the call gets no array
        for the cells (NULL) and None is returned for them"""
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = r.shape[0]
        single = False
        q = out = None
        if cell_values is not None:
            q = np.ascontiguousarray(cell_values, dtype=np.float64)
            single = q.ndim == 1
            q = q.reshape(1, -1) if single else q
            if q.ndim != 2:
                raise ValueError("cell_values must be [V][num_cells]")
            if q.shape[0] and q.shape[1] != self.num_cells:
                raise ValueError(f"cell_values has {q.shape[1]} cells per value, the grid has {self.num_cells}")
            out = np.zeros((q.shape[0], n), dtype=np.float64)
        m = np.full(n, -2, dtype=np.int32) if cells else None
        num_values = q.shape[0] if q is not None else 0
        _check(lib().pmc_sample_cells(self._h, n, r.ctypes.data_as(C.c_void_p), num_values,
                                      q.ctypes.data_as(C.c_void_p) if num_values else None, out.ctypes.data_as(C.c_void_p) if num_values else None,
                                      m.ctypes.data_as(C.c_void_p) if cells else None))
        if out is not None and single:
            out = out[0].copy()
        return out, m

    def sample_callback(self):
        """``sample_cells`` as a C callback for the host layer's cut forms: (address of pmc_sample_cells, user pointer = the context)"""
        return C.cast(lib().pmc_sample_cells, C.c_void_p).value, self._h

    def last_sample_ms(self):
        """milliseconds in the kernels of the most recent sample_cells (HIP events)"""
        ms = C.c_float(0)
        _check(lib().pmc_last_sample_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def dust_temperatures(self, tables):
        """[H + 1][num_cells]: the equilibrium temperature of every dust component in every cell and their mass-weighted mean
        (pmc_dust_temperatures), from the radiation field table of this context as it stands on the device -- its own or the bound one.
        tables: ``Simulation.temperature_tables()``, or any dict of that form"""
        struct, keep = heating_struct(tables)
        out = np.empty((struct.num_components + 1, struct.num_cells), dtype=np.float64)
        _check(lib().pmc_dust_temperatures(self._h, C.byref(struct), out.ctypes.data_as(C.c_void_p)))
        del keep
        return out

    def temperature_callback(self):
        """``dust_temperatures`` as the C callback of skh_write_probes_with (skh_temperature_fn): (function address, user pointer)"""
        if not hasattr(lib(), "pmc_dust_temperatures"):  # (likewise)
            return None, self._h
        return C.cast(lib().pmc_dust_temperatures, C.c_void_p).value, self._h

    def last_temperature_ms(self):
        """milliseconds in the kernel of the most recent dust_temperatures (HIP events)"""
        ms = C.c_float(0)
        _check(lib().pmc_last_temperature_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def last_integrate_work(self):
        """the most recent integrate_rays or integrate_weighted_rays: dict(kernel_ms, lane_steps, wave_steps); lanes in use = lane_steps / (64 wave_steps)"""
        ms, a, b = C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().pmc_last_integrate_work(self._h, C.byref(ms), C.byref(a), C.byref(b)))
        return {"kernel_ms": float(ms.value), "lane_steps": int(a.value), "wave_steps": int(b.value)}
